"""The analytic contact pairs (nt_primitives.hpp, behind primitive_pair) against exact float64 geometry on the device: the tables, invariants
and allowances of tests/primitive_exact.py through CollisionPipeline.collide -- the checks of tests/test_primitive_exact_emu.py (see its
docstring for the constants and the measured error fractions), the reference's known answers through the collide kernel, and the contacts
of a 1-substep rollout of every solver against collide's, bit for bit.  Every table is one launch of a few hundred two-body worlds; the
error fraction of every table is printed."""
import json
import os

import numpy as np
import pytest

import primitive_exact as PX
import world_isolation_cases as wi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOWN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "primitive_known_answers.json")))["tables"]
DT = {"xpbd": 2e-3, "semi_implicit": 1e-4, "featherstone": 1e-3}


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _flat(ct):
    return {k: _np(getattr(ct, "rigid_contact_" + k)) for k in ("count",) + wi.FLAT}


def device_collide(model):
    import newton_amd as nt

    pipe = nt.CollisionPipeline(model)
    ct = pipe.contacts()
    pipe.collide(model.state(), ct)
    return _flat(ct)


@pytest.mark.parametrize("name", PX.TABLE_NAMES)
def test_table_against_exact_geometry(name):
    t = PX.table(name)
    model = t.model(device=DEV)
    PX.report("MI355X", t, PX.check_table(t, PX.decode(model, model.body_q, device_collide(model))))


@pytest.mark.parametrize("table_name", sorted(KNOWN))
def test_known_answers_through_the_kernel(table_name):
    for row in KNOWN[table_name]:
        model = PX.known_answer_scene(table_name, row, device=DEV)
        PX.check_known_answer(table_name, row, PX.decode(model, model.body_q, device_collide(model))[0])


@pytest.mark.parametrize("solver", sorted(DT))
@pytest.mark.parametrize("name", PX.ROLLOUT_TABLES)
def test_rollout_contacts_equal_collide_bits(name, solver):
    import newton_amd as nt

    model = PX.table(name).model(device=DEV)
    want = device_collide(model)
    cls = {"xpbd": nt.solvers.SolverXPBD, "semi_implicit": nt.solvers.SolverSemiImplicit, "featherstone": nt.solvers.SolverFeatherstone}
    ct = nt.CollisionPipeline(model).contacts()
    cls[solver](model).rollout(model.state(), model.state(), model.control(), ct, DT[solver], 1)
    got = _flat(ct)
    n = int(want["count"][0])
    assert n > 0 and int(got["count"][0]) == n
    for k in wi.FLAT:
        assert np.array_equal(wi.bits(got[k][:n]), wi.bits(want[k][:n])), f"{name} {solver}: {k} differs from collide's"
