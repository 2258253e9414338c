/* newton_hip_kinematics.h -- joint coordinates from body state on the device (extension of newton_hip.h).
 *
 * Reference interface replaced (paths relative to the Newton source tree):
 *   nt_eval_ik            <- newton.eval_ik(model, state, joint_q, joint_qd)     newton/_src/sim/articulation.py
 *
 * The maximal-coordinate solvers (nt_xpbd_step / _rollout, nt_semi_implicit_step / _rollout) advance body_q / body_qd and leave
 * nt_state.joint_q / joint_qd alone; this call recovers them: step, then nt_eval_ik, then read the joint arrays.  It is the
 * algebraic inverse of nt_eval_fk.  Per joint with parent p, child c and anchors X_p, X_c:
 *   X_wpj = body_q[p] X_p (X_p for p < 0),  X_wcj = body_q[c] X_c,  X_j = X_wpj^-1 X_wcj = (x_j, q_j);
 *   velocities undo eval_fk's composition, its COM-twist convention included: w_o = body_qd[c].ang, v_o = body_qd[c].lin -
 *   w_o x rot(q_c, com_c); ang_w = w_o - w_p, lin_origin = v_o - (v_p + w_p x (x_c - parent COM)); v_ang = ang_w and
 *   v_lin = lin_origin - ang_w x (x_c - x_wcj) (FREE / DISTANCE: lin_origin + ang_w x rot(q_c, com_c)) rotated into the parent
 *   anchor frame.
 *   PRISMATIC  q = axis . x_j, qd = axis . v_lin          REVOLUTE  q = 2 atan2(axis . q_j.xyz, q_j.w) in (-pi, pi], qd = axis . v_ang
 *   BALL       q = q_j, qd = v_ang                        FREE / DISTANCE  q = (x_j, q_j), qd = (v_lin, v_ang)
 *   FIXED      nothing is written                         D6  linear axes as PRISMATIC, one angular axis as REVOLUTE;
 *   D6 with two or three angular axes: the intrinsic Euler angles of q_j in the frame whose columns are the axes (eval_fk's
 *   q_2 q_1 q_0 about successively rotated axes equals r_0 r_1 r_2 about the fixed ones), the rates solve
 *   v_ang = a_0 qd_0 + a_1 qd_1 (+ a_2 qd_2) over eval_fk's rotated axes.  The axes of such a joint must be mutually orthogonal.
 *   The axes live in device memory (nt_model.dof_param) and this call does not synchronise, so it cannot look at them: the caller
 *   vouches for it (newton_amd.eval_ik checks the host model and refuses a non-orthogonal multi-axis D6 as unsupported).  At the
 *   Euler singularity of three axes (middle angle +-pi/2) the rates are not defined.
 * A violated joint (what a constraint solver leaves) is projected: the components a joint type does not carry are dropped.
 *
 * Every joint of the model is evaluated, inside an articulation or not.  art_mask selects: one byte per (world, articulation),
 * [env_count * nt_model.na]; the joints of unselected articulations and joints outside any articulation are neither computed nor
 * written.  No scratch state, one launch.  Precondition of a non-NULL art_mask: the joints of articulation k are the contiguous range
 * nt_model.art_start[k] .. art_start[k + 1] of every world, and so are their coordinate rows (joint_q_start / joint_qd_start rise
 * with the joint index) -- what the model builder makes.  The call cannot check it; a model whose articulations are laid out any
 * other way must be called without a mask.
 *
 * Same conventions as newton_hip.h: device pointers owned by the caller, work enqueued on `stream`, no allocation, no
 * synchronisation -- the call can be recorded by nt_graph_capture_begin / _end.  joint_q / joint_qd may be the input state's own
 * arrays.  Errors: null pointers NT_ERR_INVALID_ARG; nj <= 0, a tile that does not fit the CU's LDS, a build with NT_DEV_FAST:
 * NT_ERR_UNSUPPORTED. */
#ifndef NEWTON_HIP_KINEMATICS_H
#define NEWTON_HIP_KINEMATICS_H

#include "newton_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

nt_status nt_eval_ik(const nt_model* m, const nt_state* in, float* joint_q /*[nc][ES]*/, float* joint_qd /*[nd][ES]*/,
                     const uint8_t* art_mask /*[env_count*na] or NULL*/, void* stream);
/* the same with the tile named: envs_per_block 0 = what nt_eval_ik takes (replicated worlds, nt_model.params_uniform: 16
 * environments around ONE block-shared parameter copy; otherwise the widest of 16 / 8 / 4 / 1 that fits), or 1, 4, 8, 16 = that many
 * environments per workgroup, each with its own parameter rows (NT_ERR_UNSUPPORTED when it does not fit).  Every tile computes the
 * same bits. */
nt_status nt_eval_ik_tile(const nt_model* m, const nt_state* in, float* joint_q, float* joint_qd, const uint8_t* art_mask,
                          int32_t envs_per_block, void* stream);

#ifdef __cplusplus
}
#endif
#endif
