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

/* Articulation Jacobian and joint-space inertia (paths relative to the Newton source tree):
 *   nt_eval_jacobian      <- newton.eval_jacobian(model, state, J, joint_S_s, mask)                      newton/_src/sim/articulation.py
 *   nt_eval_mass_matrix   <- newton.eval_mass_matrix(model, state, H, J, body_I_s, joint_S_s, mask)      newton/_src/sim/articulation.py
 *
 * Layout (public, NOT environment-major): articulation a = world * nt_model.na + k; L = the widest articulation in joints (max over k
 * of art_start[k + 1] - art_start[k]), D = nt_model.max_art_dofs.
 *   J         [env_count * na][6 L][D]   row block i of articulation a: the child body of joint art_start[k] + i; column c: the dof
 *                                        joint_qd_start[art_start[k]] + c of that world
 *   joint_S_s [env_count * nd][6]        the column of each dof (optional)
 *   H         [env_count * na][D][D]     joint-space inertia, both triangles
 *   body_I_s  [env_count * nb][6][6]     each link's world-frame spatial inertia about the origin (optional; bodies that are no joint's
 *                                        child are not written)
 * Padding rows / columns (an articulation narrower than L / D) and the entries of dofs that are not on a link's root path are written
 * as zero by every call: no memset is needed.
 *
 * Rows are origin-referenced world twists, linear first.  Columns are with respect to the public joint_qd (a FREE / DISTANCE joint
 * carries its child's COM velocity).  The defining identity, with nt_eval_fk: for link l with world pose (x_l, q_l), COM
 * c_l = x_l + rot(q_l, com_l) and (v, w) = J[a, 6 i : 6 i + 6, :] joint_qd[dofs of a], eval_fk's body_qd[l] = (v + w x c_l, w).
 * Column d of link l is S_d when d belongs to l's joint or to a joint on its joint_parent chain inside the articulation (a FREE child
 * in mid-chain inherits its ancestors' columns), else 0.  With X_wpj = body_q[parent] X_p = (p, R) and p_j the position of
 * X_wcj = X_wpj X_j(joint_q):
 *   PRISMATIC  (R a, 0)                REVOLUTE  (p_j x R a, R a)            BALL  (p_j x R e_k, R e_k)            FIXED  none
 *   D6         linear axes as PRISMATIC; angular axes: eval_fk's successively rotated axes a_0, a_1, a_2 (they depend on the joint's
 *              own joint_q), about p_j
 *   FREE / DISTANCE  linear (R e_k, 0); angular (c_child x R e_k, R e_k) -- about the child's COM
 * H = sum over links of J_l^T I_l J_l, I_l the link's spatial inertia: q'^T H q' / 2 is the articulation's kinetic energy
 * sum m |v_com|^2 / 2 + w^T R I R^T w / 2 with eval_fk's body_qd.  Symmetric bit for bit.  NO armature is added: this is not the matrix
 * nt_featherstone_step factorises (that one carries nt_model's dof armature on its diagonal and the solver's internal FREE-joint
 * velocity convention).  Computed from composite inertias along the tree in a fixed order, without atomics, about the articulation's
 * root link position (H does not depend on the point).
 *
 * Inputs read: in->body_q (parent poses, link COMs) and in->joint_q (the joint's own displacement: D6 pivots and rotated axes) --
 * eval_fk's composition.  After a maximal-coordinate step call nt_eval_ik first, so that joint_q matches body_q.  in->body_qd is not
 * read.
 *
 * art_mask as for nt_eval_ik, with the same contiguity precondition: the slices of unselected articulations in every output are
 * neither computed nor written.  One launch each, no scratch state, no allocation, no synchronisation; recordable by
 * nt_graph_capture_begin / _end.  Errors: null m / in / body_q / joint_q / J / H NT_ERR_INVALID_ARG; nj <= 0, na <= 0, a tile that does
 * not fit the CU's LDS, an envs_per_block other than 0 / 1 / 4 / 8 / 16, a build with NT_DEV_FAST: NT_ERR_UNSUPPORTED.  The _tile
 * forms name the tile as nt_eval_ik_tile does; every tile computes the same bits. */
nt_status nt_eval_jacobian(const nt_model* m, const nt_state* in, float* J, float* joint_S_s /*or NULL*/,
                           const uint8_t* art_mask /*[env_count*na] or NULL*/, void* stream);
nt_status nt_eval_jacobian_tile(const nt_model* m, const nt_state* in, float* J, float* joint_S_s, const uint8_t* art_mask,
                                int32_t envs_per_block, void* stream);
nt_status nt_eval_mass_matrix(const nt_model* m, const nt_state* in, float* H, float* body_I_s /*or NULL*/,
                              const uint8_t* art_mask /*[env_count*na] or NULL*/, void* stream);
nt_status nt_eval_mass_matrix_tile(const nt_model* m, const nt_state* in, float* H, float* body_I_s, const uint8_t* art_mask,
                                   int32_t envs_per_block, void* stream);

/* Inverse dynamics: joint torques for a given joint acceleration, and with it the bias forces h(q, q') = C(q, q') q' + g(q)
 * (joint_qdd NULL) -- the capability of the tensor APIs' generalized gravity / Coriolis-and-centrifugal force getters, in the
 * convention of nt_eval_jacobian / nt_eval_mass_matrix above:
 *   nt_eval_inverse_dynamics   (newton_amd.eval_inverse_dynamics; the reference has no single call for it)
 * With S_d the column of dof d (joint_S_s), J_l the 6 x D block of link l, I_l its world-frame spatial inertia (body_I_s), q' the public
 * joint_qd (a FREE / DISTANCE joint carries the COM velocity), q'' = joint_qdd and g this world's row of nt_model.gravity:
 *   v_l = J_l q'                        (origin-referenced world twist, linear first)
 *   a_l = J_l q'' + J'_l q'             J'_l q' = sum over the dofs d on l's root path of S'_d q'_d
 *   f_l = I_l a_l + v_l x* (I_l v_l) - (m_l g, c_l x m_l g)
 *   tau = sum_l J_l^T f_l               tau . q' is power; tau(q'') - tau(0) = H q'' with nt_eval_mass_matrix's H
 * S'_d is the time derivative of the closed form of S_d above along the motion q'.  A linear direction a carried by a frame of angular
 * velocity w_F gives (w_F x a, 0); an axis w through a pivot p gives (p' x w + p x (w_F x w), w_F x w).  The frames:
 *   PRISMATIC, REVOLUTE, BALL   axes carried by the parent link; the pivot is the parent anchor and moves with the parent
 *   FREE, DISTANCE              axes carried by the parent anchor frame; the pivot is the child's COM and moves with the child
 *   D6                          linear axes carried by the parent; angular axis k by the parent plus the joint's earlier angular dofs
 *                               (w_F = w_parent + sum_{m<k} a_m q'_m); the pivot p_j moves with the parent plus the joint's linear dofs
 * The rigid-body term only, like H: no armature, no joint limits, no drives, no friction.  This is not the bias force
 * nt_featherstone_step forms (that one is in the solver's internal FREE-joint convention); for chains of 1-dof joints the two coincide.
 *
 * flags: NT_ID_GRAVITY includes g(q); NT_ID_VELOCITY includes the terms in joint_qd (Coriolis / centrifugal), clear = joint_qd is taken
 * as 0.  Both clear and joint_qdd NULL: tau = 0 exactly.
 * joint_qdd and tau: the PUBLIC layout [env_count * na][D], D = nt_model.max_art_dofs -- the rows and columns of H.  The padding of tau
 * (an articulation narrower than D) is written as zero by every call.  joint_qdd is read through the pointer at launch time: an in-place
 * update followed by a graph replay takes effect.
 * Inputs read: in->body_q, in->joint_q (as nt_eval_jacobian) and in->joint_qd; in->body_qd is not read.  After a maximal-coordinate
 * step call nt_eval_ik first.  Multi-axis D6 joints as for nt_eval_ik (the caller vouches).  The joints of an articulation must come
 * parent before child (what the model builder makes).
 * One launch of eval_inverse_dynamics_kernel on eval_mass_matrix_kernel's tile: one lane per (environment, link) accumulates v_l and
 * a_l over the dofs on the link's root path in ascending dof order and forms f_l; one lane per (environment, dof) sums S_d . f_l over
 * the links below it in ascending joint order.  Gravity enters as the root acceleration -g, which is the definition above term by
 * term.  Twists, accelerations and wrenches are referenced to the articulation's root link position (tau does not depend on the point;
 * world coordinates of a far-away world would cost the m |c|^2 and c x f terms their digits).  No atomics, a fixed summation order,
 * IEEE arithmetic: every tile computes the same bits, replicated worlds in equal states give equal bits.
 * art_mask as for nt_eval_jacobian, with the same contiguity precondition: the slices of unselected articulations are neither computed
 * nor written.  No scratch state, no allocation, no synchronisation; recordable by nt_graph_capture_begin / _end.  Errors: those of
 * nt_eval_mass_matrix (null m / in / body_q / joint_q / joint_qd / tau NT_ERR_INVALID_ARG), and NT_ERR_INVALID_ARG for unknown flag
 * bits.  The _tile form names the tile as nt_eval_ik_tile does. */
#define NT_ID_GRAVITY  1   /* include g(q) */
#define NT_ID_VELOCITY 2   /* include the terms in joint_qd (Coriolis / centrifugal); clear = treat joint_qd as 0 */
nt_status nt_eval_inverse_dynamics(const nt_model* m, const nt_state* in, const float* joint_qdd /* [env_count*na][D] or NULL = 0 */,
                                   int32_t flags, float* tau /* [env_count*na][D] */, const uint8_t* art_mask, void* stream);
nt_status nt_eval_inverse_dynamics_tile(const nt_model* m, const nt_state* in, const float* joint_qdd, int32_t flags, float* tau,
                                        const uint8_t* art_mask, int32_t envs_per_block, void* stream);

/* Forward dynamics: the joint accelerations that joint forces and external link wrenches produce -- the inverse of the map above:
 *   nt_eval_forward_dynamics   (newton_amd.eval_forward_dynamics; the reference has no single call for it)
 *   H(q) joint_qdd = joint_f + sum_l J_l^T w_l - h(q, q')
 * H, J_l and h are exactly those of nt_eval_mass_matrix, nt_eval_jacobian and nt_eval_inverse_dynamics (joint_qdd NULL): the public
 * convention -- a FREE / DISTANCE joint carries the COM velocity -- the rigid-body terms only: no armature, no joint limits, no drives,
 * no friction.  This is not the acceleration nt_featherstone_step integrates (armature, the solver's internal FREE-joint convention);
 * for fixed-base chains of 1-dof joints without armature the two coincide.
 * w_l is the external wrench on link l, read from in->body_f ([6][nb][ES]: force rows 0..2, torque rows 3..5) in the convention the
 * steppers consume (integrate_bodies, the Featherstone step's body_f_ext): the world-frame force acting at the link's COM and the
 * world-frame torque about the link's COM.  With c_l the world COM, J_l^T w_l = J_l^T (F, T + c_l x F) for the origin-referenced J_l.
 *
 * flags: NT_FD_GRAVITY and NT_FD_VELOCITY as NT_ID_GRAVITY / NT_ID_VELOCITY select the parts of h; NT_FD_BODY_F adds J^T body_f, clear
 * = in->body_f is not read and may be NULL.  All clear and joint_f NULL: joint_qdd = 0 exactly.
 * joint_f and joint_qdd: the PUBLIC layout [env_count * na][D] of nt_eval_inverse_dynamics's tau and joint_qdd -- a round trip needs no
 * reshuffle.  The padding of joint_qdd (an articulation narrower than D) is written as zero by every call; what the padding of joint_f
 * holds does not matter.  joint_f is read through the pointer at launch time: an in-place update followed by a graph replay takes
 * effect.  Inputs read: in->body_q, in->joint_q, in->joint_qd (as nt_eval_inverse_dynamics) and, with NT_FD_BODY_F, in->body_f;
 * nothing is written but joint_qdd and info.
 * Not positive definite (a Cholesky pivot that is not > 0: a massless leaf link, a non-finite input): that articulation's nda entries
 * of joint_qdd are written as NaN and its entry of info ([env_count * na] or NULL) is the 1-based local column of the first failing
 * pivot; every other articulation's entry is 0.  No other articulation is affected in any way, the ones of the same world and
 * workgroup included: H is factored block by block, a failing pivot is replaced inside its own block only.
 * One launch of eval_forward_dynamics_kernel on eval_inverse_dynamics_kernel's tile and launch path: that kernel's walk at q'' = 0
 * gives the link wrenches (the external wrench, carried from the COM to the root link position, is subtracted in the same lane),
 * its per-dof sum the right-hand side; eval_mass_matrix_kernel's composite inertias and entry items give H in LDS; the Cholesky runs
 * column by column, column j of every articulation wider than j between two barriers (D barriers), each entry produced by one lane;
 * L y = rhs and L^T q'' = y by one lane per (environment, articulation).  H never leaves the workgroup.  No atomics, a fixed summation
 * order, IEEE arithmetic (correctly rounded division and square root, no contraction): every tile computes the same bits, replicated
 * worlds in equal states give equal bits.
 * art_mask as for nt_eval_jacobian: the slices of unselected articulations are neither read nor written, in info too.  No scratch
 * state, no allocation, no synchronisation; recordable by nt_graph_capture_begin / _end.  Errors: those of nt_eval_inverse_dynamics
 * (null m / in / body_q / joint_q / joint_qd / joint_qdd NT_ERR_INVALID_ARG), NT_ERR_INVALID_ARG for unknown flag bits and for
 * NT_FD_BODY_F with a null in->body_f, NT_ERR_UNSUPPORTED when not even one environment per workgroup fits the LDS.  The _tile form
 * names the tile as nt_eval_ik_tile does. */
#define NT_FD_GRAVITY  1   /* as NT_ID_GRAVITY */
#define NT_FD_VELOCITY 2   /* as NT_ID_VELOCITY */
#define NT_FD_BODY_F   4   /* add J^T body_f; clear = body_f is not read and may be NULL */
nt_status nt_eval_forward_dynamics(const nt_model* m, const nt_state* in, const float* joint_f /* [env_count*na][D] or NULL = 0 */,
                                   int32_t flags, float* joint_qdd /* out [env_count*na][D] */, int32_t* info /* [env_count*na] or NULL */,
                                   const uint8_t* art_mask, void* stream);
nt_status nt_eval_forward_dynamics_tile(const nt_model* m, const nt_state* in, const float* joint_f, int32_t flags, float* joint_qdd,
                                        int32_t* info, const uint8_t* art_mask, int32_t envs_per_block, void* stream);

/* Batched inverse kinematics (the capability of the reference's newton.ik.IKSolver: position / rotation / joint-limit objectives,
 * Levenberg-Marquardt):
 *   nt_ik_solve           <- newton.ik.IKSolver.step(joint_q_in, joint_q_out, iterations, step_size)     newton/_src/sim/ik/
 * One problem is one world of the replicated model (the reference takes n_problems beside a single-articulation model).  The variables
 * are all nd dofs of the world.  All `iterations` run inside ONE launch; between the iterations nothing is read from or written to
 * device memory.  Everything below is per problem; (p, q) is a link's world pose from nt_eval_fk's composition at the current joint_q.
 *
 * Residuals r, stacked in objective order (weight w):
 *   NT_IK_POSITION     w (p + rot(q, offset.xyz) - target)                                   3 rows, target [env_count][3]
 *   NT_IK_ROTATION     w 2 vec(q_err), q_err = (q * offset) * conj(target); with NT_IK_CANONICALIZE q_err is negated when its
 *                      w < 0                                                                 3 rows, target [env_count][4] (xyzw)
 *   NT_IK_JOINT_LIMIT  one row per dof d of a PRISMATIC / REVOLUTE / D6 joint with lower < upper, both of magnitude below 1e10:
 *                      w (max(0, q_d - upper) - max(0, lower - q_d))                         target [env_count][2 nd] (lower, upper)
 *   cost C = |r|^2 / 2.
 * Jacobian rows, from nt_eval_jacobian's columns (v, omega) of the link (zero off its root path):
 *   position  w (v + omega x (p + rot(q, offset)))     rotation  w omega (the Gauss-Newton approximation: exact at zero rotation error)
 *   limit     w on the dof's own column while violated, else 0.
 * Retraction joint_q (+) delta, consistent with those columns to first order: PRISMATIC / REVOLUTE / D6 coordinates add delta;
 * BALL q_j <- normalize(exp(delta) q_j) (delta in the parent anchor frame); FREE / DISTANCE: in the parent anchor frame the child's
 * COM translates by delta_lin and the child rotates by exp(delta_ang) about its COM, joint_q becomes what nt_eval_ik returns for that
 * pose.  exp(d) = (d sin(|d| / 2) / |d|, cos(|d| / 2)), (d / 2, 1) for d = 0.
 * One iteration: A = J^T J + lambda I, g = J^T r, A delta = -g by Cholesky, q' = q (+) s delta (s = step_size), C' = C(q'),
 *   pred = s (s lambda delta.delta - (2 - s) g.delta) / 2     (the reduction of the quadratic model for the scaled step;
 *                                                               s = 1: delta . (lambda delta - g) / 2)
 *   rho = (C - C') / pred.  Accepted when pred > 0, C' < C and rho > rho_min: q <- q', lambda <- max(lambda / lambda_factor,
 *   lambda_min); otherwise q stays bit for bit and lambda <- min(lambda lambda_factor, lambda_max).  A non-positive pivot is a rejection.
 * joint_q_in / joint_q_out: the PUBLIC layout [env_count][nc] (not environment-major); they may be the same array.  lambda
 * [env_count] is read and written (it persists across calls), cost [env_count] receives the cost at joint_q_out.  iterations = 0
 * copies joint_q and evaluates cost.  The targets are read through the pointers at launch time: an in-place update followed by a
 * graph replay takes effect.  Needs worlds whose bodies are all some joint's child and whose joints all belong to articulations;
 * multi-axis D6 joints as for nt_eval_ik (the caller vouches).  IEEE arithmetic in a fixed order: every tile gives the same bits,
 * identical worlds give identical rows.  Errors: null pointers, iterations < 0 NT_ERR_INVALID_ARG; more than NT_IK_MAX_OBJECTIVES
 * objectives, an unknown objective type, a link outside 0 .. nb - 1, nj <= 0, na <= 0, nd <= 0, a tile that does not fit the CU's LDS,
 * an envs_per_block other than 0 / 1 / 4 / 8 / 16, a build with NT_DEV_FAST: NT_ERR_UNSUPPORTED.  No allocation, no synchronisation;
 * recordable by nt_graph_capture_begin / _end. */
#define NT_IK_MAX_OBJECTIVES 8
enum { NT_IK_POSITION = 0, NT_IK_ROTATION = 1, NT_IK_JOINT_LIMIT = 2 };
enum { NT_IK_CANONICALIZE = 1 };
typedef struct nt_ik_objective {
    int32_t type;        /* NT_IK_POSITION / _ROTATION / _JOINT_LIMIT */
    int32_t link;        /* world-local body index (position, rotation) */
    int32_t flags;       /* NT_IK_CANONICALIZE (rotation) */
    float weight;
    float offset[4];     /* position: the point in the link frame (xyz); rotation: the offset rotation (xyzw) */
    const float* target; /* device pointer, layout by type (above) */
} nt_ik_objective;
typedef struct nt_ik_problem {
    int32_t count;
    float lambda_factor, lambda_min, lambda_max, rho_min;
    nt_ik_objective obj[NT_IK_MAX_OBJECTIVES];
} nt_ik_problem;

nt_status nt_ik_solve(const nt_model* m, const nt_ik_problem* p, const float* joint_q_in, float* joint_q_out, float* lambda, float* cost,
                      int32_t iterations, float step_size, void* stream);
/* the tile named as for nt_eval_ik_tile */
nt_status nt_ik_solve_tile(const nt_model* m, const nt_ik_problem* p, const float* joint_q_in, float* joint_q_out, float* lambda, float* cost,
                           int32_t iterations, float step_size, int32_t envs_per_block, void* stream);

/* Frame sensors (the capability of the reference's newton.sensors.SensorFrameTransform and newton.sensors.SensorIMU;
 * newton_amd.sensors.SensorFrameTransform / SensorIMU):
 *   nt_frame_sensor       <- SensorFrameTransform.update(state) / SensorIMU.update(state)               newton/_src/sensors/
 * A frame is owned by the caller, not by the model: an env-local body (or -1: fixed in the world) and a transform (p_l, q_l xyzw) in
 * that body.  The table of M frames is the same in every world; each of the N output rows of a world names the frame it measures
 * (out_frame) and the frame it is expressed in (out_ref, -1: the world).  One launch of frame_sensor_kernel straight from the env-major
 * state: no staging, no LDS, no scratch state.
 *
 * For a frame on body b with body pose (p, q) = s->body_q[b], COM c = rows 0..2 of nt_model.body_param (body frame) and
 * (v_com, w) = s->body_qd[b] (the linear part is the COM velocity, newton_hip.h):
 *   x = p + rot(q, p_l),  q_f = q * q_l,  r = rot(q, p_l - c),  v = v_com + w x r;
 * for body -1:  x = p_l,  q_f = q_l,  v = w = r = 0.  g is this world's row of nt_model.gravity ([3][ES]; a run-time change of the
 * model's gravity is seen by the next call).  Outputs, per (world, row); every pointer may be NULL, not all of them:
 *   transform   [env_count][N][7]  (rot_inv(q_ref, x - x_ref), q_ref^-1 * q_f) = X_ref^-1 X_frame; out_ref = -1: (x, q_f)
 *   velocity    [env_count][N][6]  (rot_inv(q_f, v), rot_inv(q_f, w)): the velocity of the frame origin and the angular velocity in
 *                                  the frame's own axes.  Absolute: out_ref plays no part
 *   gravity_dir [env_count][N][3]  rot_inv(q_f, g / |g|), zeros when the world's gravity is zero
 *   accel       [env_count][N][3]  the specific force an accelerometer at the frame origin reads, in the frame's axes:
 *                                  rot_inv(q_f, (v_com - v_com_prev) / dt + ((w - w_prev) / dt) x r + w x (w x r) - g).
 *                                  q, r and w are those of `s`; v_com_prev and w_prev = prev->body_qd[b] are all that is read from
 *                                  `prev`, which comes as a whole nt_state so that the caller hands over the previous state's
 *                                  descriptor unchanged.  dt is the time between the two states; the reading is the MEAN acceleration
 *                                  over that interval (the model carries no body_qdd).  prev == s is allowed: the centripetal term
 *                                  minus gravity.  A frame fixed in the world reads rot_inv(q_l, -g).
 * Plain float32 IEEE arithmetic (no contraction, correctly rounded division and square root) in one fixed expression per output
 * element: replicated worlds in equal states give equal bits.  Every selected world's whole row of every non-NULL output is written
 * by every call; world_mask ([env_count] bytes or NULL): the rows of unselected worlds are neither computed nor written.
 *
 * The tables are read on the device through frame_body / frame_xform / out_frame / out_ref; the *_host pointers are host copies of the
 * same arrays, and they are what this call validates (it does not synchronise, so it cannot look at device memory).  Same conventions
 * as above: no allocation, no synchronisation, no atomics, the launch shape depends on env_count and N alone -- recordable by
 * nt_graph_capture_begin / _end.  Errors, all NT_ERR_INVALID_ARG and all before any launch: a null m / s / a, a model without bodies,
 * a null table (device or host copy) or a null state array an output needs (body_q; body_qd for velocity and accel); M <= 0 or N <= 0;
 * every output pointer null; a frame_body outside -1 .. nb-1; an out_frame outside 0 .. M-1 or an out_ref outside -1 .. M-1; a
 * frame_xform entry that is not finite or a quaternion whose norm differs from 1 by more than 1e-4; accel with a null prev (or a prev
 * without body_qd), with dt <= 0 or with a dt that is not finite.  Nothing is answered NT_ERR_UNSUPPORTED. */
typedef struct nt_frame_sensor_args {
    int32_t frame_count;            /* M >= 1 frames in the table */
    const int32_t* frame_body;      /* [M] device: env-local body 0..nb-1, or -1 = fixed in the world */
    const float*   frame_xform;     /* [M][7] device: (p, q xyzw) of the frame in its body (in the world for body -1) */
    int32_t out_count;              /* N >= 1 output rows per world */
    const int32_t* out_frame;       /* [N] device: table index measured */
    const int32_t* out_ref;         /* [N] device: table index it is expressed in, -1 = the world */
    const int32_t* frame_body_host; const float* frame_xform_host;   /* host copies: what the entry point validates */
    const int32_t* out_frame_host;  const int32_t* out_ref_host;
    const uint8_t* world_mask;      /* [env_count] device or NULL */
    float* transform;               /* [env_count][N][7] or NULL: X_ref^-1 X_frame */
    float* velocity;                /* [env_count][N][6] or NULL: (linear velocity of the frame origin, angular velocity), in the frame's own axes */
    float* gravity_dir;             /* [env_count][N][3] or NULL: unit gravity direction in the frame's axes (0 when the world's gravity is 0) */
    float* accel;                   /* [env_count][N][3] or NULL: specific force in the frame's axes; needs `prev` */
} nt_frame_sensor_args;

nt_status nt_frame_sensor(const nt_model* m, const nt_state* s, const nt_state* prev /* NULL unless accel */, float dt,
                          const nt_frame_sensor_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
