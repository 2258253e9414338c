"""SolverSemiImplicit -- drop-in for newton.solvers.SolverSemiImplicit
(newton/_src/solvers/semi_implicit/solver_semi_implicit.py:73-217), rigid bodies only.

Penalty joints (``eval_body_joints``) + penalty contacts (``eval_body_contact``) + ``integrate_bodies`` run as ONE launch
of the gfx950 kernel ``semi_implicit_step_kernel`` through the C ABI ``nt_semi_implicit_step``; ``rollout`` runs a whole frame of
substeps -- clear_forces, collide, step, swap -- as ONE launch of ``semi_implicit_rollout_kernel`` (``nt_semi_implicit_rollout``),
bitwise equal to the call-by-call loop.
Difference to the reference, documented: ``state_in.body_f`` is never modified (the reference accumulates contact
forces into it when the model has no joints, solver_semi_implicit.py:160-163).
"""
from __future__ import annotations

import ctypes as C

from .. import _lib
from .solver import SolverBase


class SolverSemiImplicit(SolverBase):
    def __init__(self, model, *, angular_damping: float = 0.05, friction_smoothing: float = 1.0, joint_attach_ke: float = 1.0e4,
                 joint_attach_kd: float = 1.0e2, enable_tri_contact: bool = True, envs_per_block: int = 0):
        super().__init__(model)
        self.dm.require_fit("SolverSemiImplicit")
        self.angular_damping = angular_damping
        self.friction_smoothing = friction_smoothing
        self.joint_attach_ke = joint_attach_ke
        self.joint_attach_kd = joint_attach_kd
        self.enable_tri_contact = enable_tri_contact
        self.envs_per_block = int(envs_per_block)

    def _params(self):
        return _lib.nt_semi_implicit_params(float(self.angular_damping), float(self.friction_smoothing),
                                            float(self.joint_attach_ke), float(self.joint_attach_kd))

    def step(self, state_in, state_out, control, contacts, dt: float) -> None:
        dm = self.dm
        if control is None:
            if not hasattr(self, "_control"):
                self._control = self.model.control()
            control = self._control
        p = self._params()
        d_in, d_out, d_c = state_in._desc(), state_out._desc(), control._desc()
        d_in = self._state_desc_with_sdf_forces(state_in, contacts, self.friction_smoothing)
        d_ct = contacts._desc() if contacts is not None else None
        _lib.check(dm.lib.nt_semi_implicit_step(C.byref(dm.desc), C.byref(p), C.byref(d_in), C.byref(d_out), C.byref(d_c),
                                                C.byref(d_ct) if d_ct is not None else None, float(dt),
                                                self.envs_per_block, dm.stream()), "nt_semi_implicit_step")

    def rollout(self, state_0, state_1, control, contacts, dt: float, substeps: int):
        """substeps x {clear_forces; collide; step; swap} in ONE launch (``nt_semi_implicit_rollout``); returns the state
        object holding the result (state_0 for an even number of substeps, state_1 for odd -- the reference loop's swap)."""
        dm = self.dm
        if control is None:
            if not hasattr(self, "_control"):
                self._control = self.model.control()
            control = self._control
        leg = getattr(contacts, "_sdf_leg", None)
        if leg is not None:
            # the SDF legs of collide() are a chain of launches of their own (newton_amd/sdf_pipeline.py): run the reference loop
            # launch by launch, like the other solvers' rollouts do for such models (step adds the rows' penalty wrenches)
            cp = _lib.nt_collide_params(0, self.envs_per_block)
            for _ in range(int(substeps)):
                state_0.clear_forces()
                d_s, d_ct = state_0._desc(), contacts._desc()
                leg.export_pointers(d_ct)
                _lib.check(dm.lib.nt_collide(C.byref(dm.desc), C.byref(d_s), C.byref(d_ct), C.byref(cp), dm.stream()), "nt_collide")
                leg.collide(state_0, contacts._flat, dm.stream())
                contacts._generation += 1
                self.step(state_0, state_1, control, contacts, dt)
                state_0, state_1 = state_1, state_0
            return state_0
        p = self._params()
        cp = _lib.nt_collide_params(0, self.envs_per_block)
        d0, d1, d_c, d_ct = state_0._desc(), state_1._desc(), control._desc(), contacts._desc()
        _lib.check(dm.lib.nt_semi_implicit_rollout(C.byref(dm.desc), C.byref(p), C.byref(cp), C.byref(d0), C.byref(d1),
                                                   C.byref(d_c), C.byref(d_ct), float(dt), int(substeps), dm.stream()),
                   "nt_semi_implicit_rollout")
        contacts._generation += 1
        return state_1 if substeps % 2 else state_0
