// nt_featherstone.hip -- SolverFeatherstone (step / fused rollout), eval_fk and eval_ik: launch code + C ABI.  The solver's kernels are
// nt_featherstone_kernels.hpp, their phases nt_featherstone.hpp (namespace ieee); this unit exists so that they are compiled with the
// default scheduler (see nt_step_preamble.hpp).  eval_ik, eval_jacobian, eval_mass_matrix, eval_inverse_dynamics, eval_forward_dynamics, ik_solve and frame_sensor (kernels and entry
// points, include/newton_hip_kinematics.h) live here whole: the headers the stepping unit shares stay as they are.
// Launch code: the solver's tile choice is fs_launch (a measured rule of its own); every kinematics entry point -- nt_eval_fk and the
// six _tile entry points -- chooses its tile and launches through ONE function, kin_launch, below the kernels.
#include "nt_step_preamble.hpp"
#ifndef NT_EMULATED_GRID
#include "../../include/newton_hip_kinematics.h"
#else  // (the CPU emulator compiles a copy of this file from tests/emu/_build)
#include "../../../include/newton_hip_kinematics.h"
#endif

namespace {
namespace ieee {

// ------------------------------------------------------------------------------------------------
// newton.eval_ik(model, state, joint_q, joint_qd) (newton/_src/sim/articulation.py): joint coordinates from body state, the algebraic
// inverse of eval_fk_kernel / fs_fk_vel_item<PUBLIC>.  The joints of an environment do not depend on each other (a joint reads the
// two bodies it connects), so there is no level loop: one (environment, joint) item per slot-lane between two barriers.
// Tile: the persistent block of the XPBD layout without its body-derived tile (body state, parameters), then joint_q [nc] and
// joint_qd [nd] rows that unstage_rows writes out.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline int ik_rows(const nt_model& m, const bool uni) {
    return make_layout(m, false, false, uni, false).bd.off + m.nc + m.nd;
}

// twist angle of q about `axis`, in (-pi, pi]
NT_DI float ik_twist_angle(vec3 axis, quat q) {
    const float pi = 3.14159265358979323846f;
    float t = 2.0f * atan2f(dot(axis, vec3(q.x, q.y, q.z)), q.w);
    if (t > pi) t -= 2.0f * pi;
    if (t <= -pi) t += 2.0f * pi;
    return t;
}

template <int EPB>
NT_DI void ik_joint_item(const Ctx<EPB>& c, int j, int oq, int oqd, const float* joint_q, const float* joint_qd) {
    const nt_model& m = c.a.m;
    const int parent = c.T.joint_parent[j], child = c.T.joint_child[j], type = c.T.joint_type[j];
    const int qs = c.T.joint_q_start[j], ds = c.T.joint_qd_start[j];
    const int lin = c.T.joint_lin_count[j], ang = c.T.joint_ang_count[j];
    auto Q = [&](int i) -> float& { return c.lds[(oq + i) * Ctx<EPB>::N + c.e]; };
    auto QD = [&](int i) -> float& { return c.lds[(oqd + i) * Ctx<EPB>::N + c.e]; };
    const bool is_free = type == JT_FREE || type == JT_DISTANCE;
    if (type != JT_PRISMATIC && type != JT_REVOLUTE && type != JT_BALL && type != JT_D6 && !is_free) {
        // FIXED has no coordinates; a type eval_fk skips too keeps what the arrays hold
        const int qe = j + 1 < m.nj ? c.T.joint_q_start[j + 1] : m.nc, de = j + 1 < m.nj ? c.T.joint_qd_start[j + 1] : m.nd;
        for (int i = qs; i < qe; ++i) Q(i) = joint_q[(size_t)i * c.ES + c.env];
        for (int i = ds; i < de; ++i) QD(i) = joint_qd[(size_t)i * c.ES + c.env];
        return;
    }
    xform X_wpj = c.plxf(c.L.jp, 0, m.nj, j);
    xform X_wp;
    if (parent >= 0) {
        X_wp = c.body_q(parent);
        X_wpj = X_wp * X_wpj;
    }
    const xform X_wc = c.body_q(child);
    const xform X_wcj = X_wc * c.plxf(c.L.jp, 7, m.nj, j);
    // X_j = X_wpj^-1 X_wcj
    const vec3 x_j = quat_rotate_inv(X_wpj.q, X_wcj.p - X_wpj.p);
    const quat q_j = quat_inverse(X_wpj.q) * X_wcj.q;
    // the joint's velocity in the parent anchor frame: fs_fk_vel_item<PUBLIC> undone term by term (body_qd carries the COM velocity)
    const vec3 w_o = c.body_w(child), com_w = quat_rotate(X_wc.q, c.com(child));
    const vec3 v_o = c.body_v(child) - cross(w_o, com_w);
    vec3 w_parent, v_parent;
    if (parent >= 0) {
        w_parent = c.body_w(parent);
        v_parent = cross(w_parent, X_wc.p - xform_point(X_wp, c.com(parent))) + c.body_v(parent);
    }
    const vec3 ang_w = w_o - w_parent, lin_origin = v_o - v_parent;
    const vec3 lin_w = is_free ? lin_origin + cross(ang_w, com_w) : lin_origin - cross(ang_w, X_wc.p - X_wcj.p);
    const vec3 v_lin = quat_rotate_inv(X_wpj.q, lin_w), v_ang = quat_rotate_inv(X_wpj.q, ang_w);

    if (type == JT_PRISMATIC) {
        Q(qs) = dot(c.dof_axis(ds), x_j);
        QD(ds) = dot(c.dof_axis(ds), v_lin);
    } else if (type == JT_REVOLUTE) {
        Q(qs) = ik_twist_angle(c.dof_axis(ds), q_j);
        QD(ds) = dot(c.dof_axis(ds), v_ang);
    } else if (type == JT_BALL) {
        Q(qs) = q_j.x; Q(qs + 1) = q_j.y; Q(qs + 2) = q_j.z; Q(qs + 3) = q_j.w;
        QD(ds) = v_ang.x; QD(ds + 1) = v_ang.y; QD(ds + 2) = v_ang.z;
    } else if (is_free) {
        Q(qs) = x_j.x; Q(qs + 1) = x_j.y; Q(qs + 2) = x_j.z;
        Q(qs + 3) = q_j.x; Q(qs + 4) = q_j.y; Q(qs + 5) = q_j.z; Q(qs + 6) = q_j.w;
        QD(ds) = v_lin.x; QD(ds + 1) = v_lin.y; QD(ds + 2) = v_lin.z;
        QD(ds + 3) = v_ang.x; QD(ds + 4) = v_ang.y; QD(ds + 5) = v_ang.z;
    } else {  // D6
        for (int k = 0; k < lin; ++k) {
            Q(qs + k) = dot(c.dof_axis(ds + k), x_j);
            QD(ds + k) = dot(c.dof_axis(ds + k), v_lin);
        }
        const int iq = qs + lin, id = ds + lin;
        if (ang == 1) {
            Q(iq) = ik_twist_angle(c.dof_axis(id), q_j);
            QD(id) = dot(c.dof_axis(id), v_ang);
        }
        if (ang >= 2) {
            // eval_fk composes q_2 q_1 q_0 about successively rotated axes = r_0 r_1 r_2 about the fixed (mutually orthogonal) axes:
            // the angles are the intrinsic x-y-z Euler angles of M = B^T R(q_j) B, B = [e0 e1 e2] (a left-handed triple flips
            // their signs); two axes: r_2 = 1 and both angles keep their full range
            const vec3 e0 = c.dof_axis(id), e1 = c.dof_axis(id + 1);
            const vec3 e2 = ang == 3 ? c.dof_axis(id + 2) : cross(e0, e1);
            const vec3 r0 = quat_rotate(q_j, e0), r1 = quat_rotate(q_j, e1), r2 = quat_rotate(q_j, e2);
            float t0, t1, t2 = 0.0f;
            if (ang == 2) {
                t0 = atan2f(dot(e2, r1), dot(e1, r1));
                t1 = atan2f(dot(e0, r2), dot(e0, r0));
            } else {
                const float s = dot(cross(e0, e1), e2) < 0.0f ? -1.0f : 1.0f;
                const float m00 = dot(e0, r0), m01 = dot(e0, r1), m02 = dot(e0, r2);
                t0 = s * atan2f(-dot(e1, r2), dot(e2, r2));
                t1 = s * atan2f(m02, sqrtf(m00 * m00 + m01 * m01));
                t2 = s * atan2f(-m01, m00);
            }
            // rates: v_ang = a_0 qd_0 + a_1 qd_1 (+ a_2 qd_2) over eval_fk's transported axes at the recovered angles (Cramer)
            vec3 a0, a1, a2;
            d6_multi_angular(ang, e0, e1, ang == 3 ? e2 : vec3(), t0, t1, t2, a0, a1, a2);
            Q(iq) = t0; Q(iq + 1) = t1;
            if (ang == 2) {
                const float g00 = dot(a0, a0), g01 = dot(a0, a1), g11 = dot(a1, a1), b0 = dot(a0, v_ang), b1 = dot(a1, v_ang);
                const float det = g00 * g11 - g01 * g01;
                QD(id) = (b0 * g11 - b1 * g01) / det;
                QD(id + 1) = (g00 * b1 - g01 * b0) / det;
            } else {
                const vec3 a12 = cross(a1, a2);
                const float det = dot(a0, a12);
                Q(iq + 2) = t2;
                QD(id) = dot(v_ang, a12) / det;
                QD(id + 1) = dot(a0, cross(v_ang, a2)) / det;
                QD(id + 2) = dot(a0, cross(a1, v_ang)) / det;
            }
        }
    }
}

// art_mask: [env_count * na] or NULL (every joint).  A joint the mask leaves out is neither computed nor written.
template <int EPB>
__global__ void __launch_bounds__(256) eval_ik_kernel(KArgs a, float* joint_q, float* joint_qd, const uint8_t* art_mask) {
    extern __shared__ __align__(16) float lds[];
    const nt_model& m = a.m;
    Ctx<EPB> c(a, lds, ik_rows(m, Ctx<EPB>::UNI));
    load_state(c, a.s_in);
    load_params(c, false);
    __syncthreads();  // (topology ints, tile)
    const int oq = c.L.bd.off, oqd = oq + m.nc;
    if (c.valid) {
        if (!art_mask) {
            for (int j = c.slot; j < m.nj; j += c.nslot) ik_joint_item(c, j, oq, oqd, joint_q, joint_qd);
        } else {  // the joints of the selected articulations; joints outside any articulation never are
            for (int k = 0; k < m.na; ++k)
                if (art_mask[(size_t)c.env * m.na + k])
                    for (int j = m.art_start[k] + c.slot; j < m.art_start[k + 1]; j += c.nslot)
                        ik_joint_item(c, j, oq, oqd, joint_q, joint_qd);
        }
    }
    __syncthreads();
    if (!c.valid) return;
    if (!art_mask) {
        unstage_rows(c, oq, joint_q, m.nc);
        unstage_rows(c, oqd, joint_qd, m.nd);
        return;
    }
    for (int k = 0; k < m.na; ++k) {  // the coordinates of an articulation are one row range
        const int j0 = m.art_start[k], j1 = m.art_start[k + 1];
        if (j0 >= j1 || !art_mask[(size_t)c.env * m.na + k]) continue;
        const int q0 = c.T.joint_q_start[j0], q1 = j1 < m.nj ? c.T.joint_q_start[j1] : m.nc;
        const int d0 = c.T.joint_qd_start[j0], d1 = j1 < m.nj ? c.T.joint_qd_start[j1] : m.nd;
        unstage_rows(c, oq + q0, joint_q + (size_t)q0 * c.ES, q1 - q0);
        unstage_rows(c, oqd + d0, joint_qd + (size_t)d0 * c.ES, d1 - d0);
    }
}

// ------------------------------------------------------------------------------------------------
// nt_frame_sensor (newton_amd.sensors.SensorFrameTransform / SensorIMU; contract: include/newton_hip_kinematics.h): pose, velocity,
// gravity direction and specific force of caller-owned frames, straight from the env-major state.  One lane per (output row, world)
// with the world the fastest index: a workgroup is ONE wave that takes one row for 64 consecutive worlds, so every body_q / body_qd /
// body_param / gravity read is a run of 64 consecutive floats, and the row's table entries (frames, bodies, local transforms) are the
// same in every lane -- they come in through scalar loads.  The (row, 64 worlds) items are handed out grid-stride.  No LDS, no barrier,
// no atomics; the outputs are the public [world][row][comp] arrays, each lane writing the 3 / 6 / 7 consecutive floats of its row.
// ------------------------------------------------------------------------------------------------
constexpr int FR_THREADS = 64;     // lanes of a workgroup: one wave, 64 consecutive worlds of one output row
constexpr int FR_MAX_GRID = 8192;  // workgroups at most (32 waves for each of 256 CUs); what is left is taken grid-stride

struct FrFrame {
    vec3 x, r, vc, v, w;  // origin, origin - COM (world axes), COM velocity, velocity of the origin, angular velocity
    quat q;
    int body;
};

NT_DI vec3 fr_load3(const float* base, int c0, int n, int slot, size_t ES, int e) {
    return vec3(base[((size_t)(c0 + 0) * n + slot) * ES + e], base[((size_t)(c0 + 1) * n + slot) * ES + e],
                base[((size_t)(c0 + 2) * n + slot) * ES + e]);
}
NT_DI int fr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// pose of table frame f in world e; with `vel` its r, v and w too
NT_DI FrFrame fr_frame(const nt_model& m, const float* body_q, const float* body_qd, const nt_frame_sensor_args& a, int f, int e, bool vel) {
    const size_t ES = (size_t)m.env_stride;
    const float* X = a.frame_xform + 7 * (size_t)f;
    const vec3 pl(X[0], X[1], X[2]);
    const quat ql(X[3], X[4], X[5], X[6]);
    FrFrame F;
    F.body = fr_clamp(a.frame_body[f], -1, m.nb - 1);  // (the entry point refuses other values in the host copy)
    if (F.body < 0) {
        F.x = pl;
        F.q = ql;
        return F;
    }
    const vec3 p = fr_load3(body_q, 0, m.nb, F.body, ES, e);
    const quat q(body_q[((size_t)3 * m.nb + F.body) * ES + e], body_q[((size_t)4 * m.nb + F.body) * ES + e],
                 body_q[((size_t)5 * m.nb + F.body) * ES + e], body_q[((size_t)6 * m.nb + F.body) * ES + e]);
    F.x = p + quat_rotate(q, pl);
    F.q = q * ql;
    if (vel) {
        F.r = quat_rotate(q, pl - fr_load3(m.body_param, BP_COM, m.nb, F.body, ES, e));
        F.w = fr_load3(body_qd, 3, m.nb, F.body, ES, e);
        F.vc = fr_load3(body_qd, 0, m.nb, F.body, ES, e);
        F.v = F.vc + cross(F.w, F.r);
    }
    return F;
}

__global__ void __launch_bounds__(FR_THREADS) frame_sensor_kernel(nt_model m, const float* body_q, const float* body_qd, const float* prev_qd,
                                                                  float dt, nt_frame_sensor_args a) {
    const int E = m.env_count, N = a.out_count, M = a.frame_count;
    const size_t ES = (size_t)m.env_stride;
    const int chunks = (E + FR_THREADS - 1) / FR_THREADS, items = chunks * N;
    const bool vel = a.velocity || a.accel;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int n = item / chunks, e = (item - n * chunks) * FR_THREADS + (int)threadIdx.x;
        if (e >= E || (a.world_mask && !a.world_mask[e])) continue;
        const int f = fr_clamp(a.out_frame[n], 0, M - 1), ref = fr_clamp(a.out_ref[n], -1, M - 1);
        const FrFrame F = fr_frame(m, body_q, body_qd, a, f, e, vel);
        const size_t row = (size_t)e * N + n;
        if (a.transform) {
            vec3 x = F.x;
            quat q = F.q;
            if (ref >= 0) {
                const FrFrame R = fr_frame(m, body_q, body_qd, a, ref, e, false);
                x = quat_rotate_inv(R.q, F.x - R.x);
                q = quat_inverse(R.q) * F.q;
            }
            float* out = a.transform + 7 * row;
            out[0] = x.x; out[1] = x.y; out[2] = x.z;
            out[3] = q.x; out[4] = q.y; out[5] = q.z; out[6] = q.w;
        }
        if (a.velocity) {
            const vec3 v = quat_rotate_inv(F.q, F.v), w = quat_rotate_inv(F.q, F.w);
            float* out = a.velocity + 6 * row;
            out[0] = v.x; out[1] = v.y; out[2] = v.z;
            out[3] = w.x; out[4] = w.y; out[5] = w.z;
        }
        if (a.gravity_dir || a.accel) {
            const vec3 g(m.gravity[e], m.gravity[ES + e], m.gravity[2 * ES + e]);
            if (a.gravity_dir) {
                const vec3 d = quat_rotate_inv(F.q, normalize(g));
                float* out = a.gravity_dir + 3 * row;
                out[0] = d.x; out[1] = d.y; out[2] = d.z;
            }
            if (a.accel) {
                vec3 acc = -g;
                if (F.body >= 0) {
                    const vec3 dv = F.vc - fr_load3(prev_qd, 0, m.nb, F.body, ES, e);
                    const vec3 dw = F.w - fr_load3(prev_qd, 3, m.nb, F.body, ES, e);
                    acc = dv / dt + cross(dw / dt, F.r) + cross(F.w, cross(F.w, F.r)) - g;
                }
                acc = quat_rotate_inv(F.q, acc);
                float* out = a.accel + 3 * row;
                out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// newton.eval_jacobian / eval_mass_matrix (newton/_src/sim/articulation.py; contract: include/newton_hip_kinematics.h).  Both kernels
// build the motion-subspace column S_d of every (environment, dof) from the parent pose in body_q and the joint's own joint_q -- eval_fk's
// composition -- and keep it in LDS.  Tile: the persistent block of the XPBD layout without its body-derived tile, then joint_q [nc],
// S (ENV-MAJOR: [e][6][nd], odd stride -- the streaming phase reads it with consecutive lanes on consecutive dofs), and for the mass
// matrix the composite inertias [10][nj] and H (env-major [e][nd][D]).  Block-shared ints behind the topology: the joint's ancestor
// joint, depth and articulation, the joint of each dof, and per joint the bit mask of the joints on its root path (itself included).
// ------------------------------------------------------------------------------------------------
struct JmLayout {
    int jq, S, SW, Ic, H, HW, rows;
};
__host__ __device__ inline JmLayout jm_layout(const nt_model& m, const bool uni, const bool mass) {
    JmLayout F;
    int o = make_layout(m, false, false, uni, false).bd.off;
    F.jq = o; o += m.nc;
    F.SW = (6 * m.nd) | 1;
    F.S = o; o += F.SW;
    F.Ic = o; o += mass ? 10 * m.nj : 0;
    F.HW = (m.nd * m.max_art_dofs) | 1;
    F.H = o; o += mass ? F.HW : 0;
    F.rows = o;
    return F;
}
__host__ __device__ inline int jm_table_ints(const nt_model& m) { return 3 * m.nj + m.nd + m.nj * fs_mask_words(m); }

template <int EPB>
struct JmCtx {
    const Ctx<EPB>& c;
    JmLayout F;
    const int *anc, *depth, *art, *dof_joint;
    const unsigned* pathmask;
    int words;
    static constexpr int N = Ctx<EPB>::N;
    NT_DI JmCtx(const Ctx<EPB>& c_, const JmLayout& F_, const int* extra) : c(c_), F(F_) {
        const int nj = c.a.m.nj;
        anc = extra; depth = extra + nj; art = extra + 2 * nj; dof_joint = extra + 3 * nj;
        pathmask = reinterpret_cast<const unsigned*>(extra + 3 * nj + c.a.m.nd);
        words = fs_mask_words(c.a.m);
    }
    // is joint `a` on the root path of joint `l` (or `l` itself)?
    NT_DI bool on_path(int a, int l) const { return (pathmask[l * words + (a >> 5)] >> (a & 31)) & 1u; }
    NT_DI float& S(int e, int comp, int d) const { return c.lds[F.S * N + e * F.SW + comp * c.a.m.nd + d]; }
    NT_DI float& H(int e, int i, int lj) const { return c.lds[F.H * N + e * F.HW + i * c.a.m.max_art_dofs + lj]; }
    NT_DI float& Ic(int comp, int j) const { return c.lds[(F.Ic + comp * c.a.m.nj + j) * N + c.e]; }
    NT_DI float jq(int i) const { return c.lds[(F.jq + i) * N + c.e]; }
    NT_DI int qd_end(int j) const { return j + 1 < c.a.m.nj ? c.T.joint_qd_start[j + 1] : c.a.m.nd; }
    NT_DI int max_depth() const {
        int d = 0;
        for (int j = 0; j < c.a.m.nj; ++j) d = imax(d, depth[j]);
        return d;
    }
};

// the tables (every thread of the workgroup; the staged topology must be published: one barrier after Ctx's constructor)
template <int EPB>
NT_DI void jm_build_tables(const Ctx<EPB>& c, int* extra) {
    const nt_model& m = c.a.m;
    const int nj = m.nj, words = fs_mask_words(m);
    for (int j = threadIdx.x; j < nj; j += blockDim.x) {
        int p = c.T.joint_parent[j], anc = -1, art = 0;
        for (int k = 0; k < m.na; ++k)
            if (m.art_start[k] <= j) art = k;
        if (p >= 0)  // the joint of the same articulation whose child is this joint's parent body
            for (int k = m.art_start[art]; k < m.art_start[art + 1]; ++k)
                if (c.T.joint_child[k] == p) anc = k;
        extra[j] = anc;
        extra[2 * nj + j] = art;
    }
    for (int d = threadIdx.x; d < m.nd; d += blockDim.x) {
        int j = 0;
        for (int k = 1; k < nj; ++k)
            if (c.T.joint_qd_start[k] <= d) j = k;
        extra[3 * nj + d] = j;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nj; j += blockDim.x) {
        int d = 0, k = extra[j];
        unsigned* mask = reinterpret_cast<unsigned*>(extra + 3 * nj + m.nd) + j * words;
        for (int w = 0; w < words; ++w) mask[w] = 0u;
        mask[j >> 5] |= 1u << (j & 31);
        while (k >= 0 && d < nj) {
            d += 1;
            mask[k >> 5] |= 1u << (k & 31);
            k = extra[k];
        }
        extra[nj + j] = d;
    }
    __syncthreads();
}

// S_d of dof d as an origin-referenced world twist (linear, angular) about the point `ref` (the closed forms of the header)
template <int EPB>
NT_DI void jm_S_item(const JmCtx<EPB>& f, int d, vec3 ref) {
    const Ctx<EPB>& c = f.c;
    const nt_model& m = c.a.m;
    const int j = f.dof_joint[d];
    const int parent = c.T.joint_parent[j], child = c.T.joint_child[j], type = c.T.joint_type[j];
    const int ds = c.T.joint_qd_start[j], cs = c.T.joint_q_start[j], k = d - ds;
    const int lin = c.T.joint_lin_count[j], ang = c.T.joint_ang_count[j];
    xform X_wpj = c.plxf(c.L.jp, 0, m.nj, j);
    if (parent >= 0) X_wpj = c.body_q(parent) * X_wpj;
    const vec3 unit(k % 3 == 0 ? 1.0f : 0.0f, k % 3 == 1 ? 1.0f : 0.0f, k % 3 == 2 ? 1.0f : 0.0f);
    vec3 a_lin, a_ang, pivot = X_wpj.p;  // (axes in the parent anchor frame)
    bool angular = false;
    if (type == JT_PRISMATIC) {
        a_lin = c.dof_axis(d);
    } else if (type == JT_REVOLUTE) {
        a_ang = c.dof_axis(d);
        angular = true;
    } else if (type == JT_BALL) {
        a_ang = unit;
        angular = true;
    } else if (type == JT_FREE || type == JT_DISTANCE) {
        if (k < 3) {
            a_lin = unit;
        } else {  // about the child's COM: joint_qd's linear part is the COM velocity
            a_ang = unit;
            angular = true;
            pivot = xform_point(c.body_q(child), c.com(child));
        }
    } else if (type == JT_D6) {
        if (k < lin) {
            a_lin = c.dof_axis(d);
        } else {
            angular = true;
            vec3 pos(0.0f);
            for (int i = 0; i < lin; ++i) pos += c.dof_axis(ds + i) * f.jq(cs + i);
            pivot = xform_point(X_wpj, pos);
            if (ang == 1) {
                a_ang = c.dof_axis(d);
            } else {
                vec3 a0, a1, a2;
                d6_multi_angular(ang, c.dof_axis(ds + lin), c.dof_axis(ds + lin + 1), ang == 3 ? c.dof_axis(ds + lin + 2) : vec3(),
                                 f.jq(cs + lin), f.jq(cs + lin + 1), ang == 3 ? f.jq(cs + lin + 2) : 0.0f, a0, a1, a2);
                a_ang = k - lin == 0 ? a0 : (k - lin == 1 ? a1 : a2);
            }
        }
    }
    vec3 top, bottom;
    if (angular) {
        bottom = quat_rotate(X_wpj.q, a_ang);
        top = cross(pivot - ref, bottom);
    } else {
        top = quat_rotate(X_wpj.q, a_lin);
    }
    f.S(c.e, 0, d) = top.x; f.S(c.e, 1, d) = top.y; f.S(c.e, 2, d) = top.z;
    f.S(c.e, 3, d) = bottom.x; f.S(c.e, 4, d) = bottom.y; f.S(c.e, 5, d) = bottom.z;
}

// the widest articulation in joints (the row blocks of J)
NT_DI int jm_max_joints(const nt_model& m) {
    int L = 0;
    for (int k = 0; k < m.na; ++k) L = imax(L, m.art_start[k + 1] - m.art_start[k]);
    return L;
}

// staging shared by both kernels: body poses, parameters, joint_q
template <int EPB>
NT_DI void jm_load(const Ctx<EPB>& c, const JmLayout& F) {
    const nt_model& m = c.a.m;
    if (c.valid) stage_rows(c, c.L.bq, c.a.s_in.body_q, 7, m.nb, c.slot);
    load_params(c, false);
    if (c.valid) stage_rows(c, F.jq, c.a.s_in.joint_q, m.nc);
}

// J [env_count * na][6 L][D] and (optional) joint_S_s [env_count * nd][6], both in the public layout.  art_mask as for eval_ik_kernel.
template <int EPB>
__global__ void __launch_bounds__(256) eval_jacobian_kernel(KArgs a, float* J, float* joint_S_s, const uint8_t* art_mask) {
    extern __shared__ __align__(16) float lds[];
    const nt_model& m = a.m;
    constexpr int N = Ctx<EPB>::N;
    const JmLayout F = jm_layout(m, Ctx<EPB>::UNI, false);
    Ctx<EPB> c(a, lds, F.rows);
    int* extra = c.own_tables(jm_table_ints(m));
    __syncthreads();
    jm_build_tables(c, extra);
    const JmCtx<EPB> f(c, F, extra);
    jm_load(c, F);
    __syncthreads();
    if (c.valid)
        for (int d = c.slot; d < m.nd; d += c.nslot)
            if (!art_mask || art_mask[(size_t)c.env * m.na + f.art[f.dof_joint[d]]]) jm_S_item(f, d, vec3());
    __syncthreads();
    // stream the tile's articulations: lanes over the flattened [6 L][D] block, zeros from the ancestor test
    const int L = jm_max_joints(m), D = m.max_art_dofs, block = 6 * L * D;
    for (int t = 0; t < N * m.na; ++t) {
        const int e = t / m.na, k = t - e * m.na, env = blockIdx.x * N + e;
        if (env >= m.env_count) break;
        if (art_mask && !art_mask[(size_t)env * m.na + k]) continue;
        const int j0 = m.art_start[k], nja = m.art_start[k + 1] - j0;
        const int d0 = nja > 0 ? c.T.joint_qd_start[j0] : 0, nda = nja > 0 ? f.qd_end(j0 + nja - 1) - d0 : 0;
        float* out = J + (size_t)((size_t)env * m.na + k) * block;
        for (int i = threadIdx.x; i < block; i += blockDim.x) {
            const int row = i / D, col = i - row * D, jl = row / 6, comp = row - jl * 6;
            float v = 0.0f;
            if (jl < nja && col < nda && f.on_path(f.dof_joint[d0 + col], j0 + jl)) v = f.S(e, comp, d0 + col);
            out[i] = v;
        }
    }
    if (!joint_S_s) return;
    for (int e = 0; e < N; ++e) {
        const int env = blockIdx.x * N + e;
        if (env >= m.env_count) break;
        float* out = joint_S_s + (size_t)env * m.nd * 6;
        for (int i = threadIdx.x; i < 6 * m.nd; i += blockDim.x) {
            const int d = i / 6, comp = i - d * 6;
            if (!art_mask || art_mask[(size_t)env * m.na + f.art[f.dof_joint[d]]]) out[i] = f.S(e, comp, d);
        }
    }
}

// link j's spatial inertia about `ref` as {mass, first moment h = m c, rotational inertia about ref (xx xy xz yy yz zz)}: ten numbers
// that add under composition.  body_I_s (optional): the dense 6 x 6 about the world origin, [env * nb + body][6][6].
template <int EPB>
NT_DI void jm_inertia_item(const JmCtx<EPB>& f, int j, vec3 ref, float* body_I_s) {
    const Ctx<EPB>& c = f.c;
    const nt_model& m = c.a.m;
    const int b = c.T.joint_child[j];
    const xform X = c.body_q(b);
    const float mass = c.pl(c.L.bp, BP_MASS, m.nb, b);
    const mat33 R = quat_to_matrix(X.q);
    const mat33 Ib = c.inertia(b);
    const vec3 r0(R.m00, R.m01, R.m02), r1(R.m10, R.m11, R.m12), r2(R.m20, R.m21, R.m22);
    const vec3 t0 = Ib * r0, t1 = Ib * r1, t2 = Ib * r2;  // R I R^T, entry (i, j) = r_i . (I r_j)
    const float wxx = dot(r0, t0), wxy = dot(r0, t1), wxz = dot(r0, t2), wyy = dot(r1, t1), wyz = dot(r1, t2), wzz = dot(r2, t2);
    const vec3 cw = xform_point(X, c.com(b));
    auto rotational = [&](vec3 r, float (&o)[6]) {  // R I R^T - m [r]x [r]x
        o[0] = wxx + mass * (r.y * r.y + r.z * r.z); o[1] = wxy - mass * (r.x * r.y); o[2] = wxz - mass * (r.x * r.z);
        o[3] = wyy + mass * (r.x * r.x + r.z * r.z); o[4] = wyz - mass * (r.y * r.z); o[5] = wzz + mass * (r.x * r.x + r.y * r.y);
    };
    const vec3 r = cw - ref;
    float io[6];
    rotational(r, io);
    f.Ic(0, j) = mass;
    f.Ic(1, j) = mass * r.x; f.Ic(2, j) = mass * r.y; f.Ic(3, j) = mass * r.z;
#pragma unroll
    for (int k = 0; k < 6; ++k) f.Ic(4 + k, j) = io[k];
    if (body_I_s) {
        rotational(cw, io);
        const vec3 h = cw * mass;
        const float M[6][6] = {{mass, 0.0f, 0.0f, 0.0f, h.z, -h.y},  {0.0f, mass, 0.0f, -h.z, 0.0f, h.x},  {0.0f, 0.0f, mass, h.y, -h.x, 0.0f},
                               {0.0f, -h.z, h.y, io[0], io[1], io[2]}, {h.z, 0.0f, -h.x, io[1], io[3], io[4]}, {-h.y, h.x, 0.0f, io[2], io[4], io[5]}};
        float* out = body_I_s + ((size_t)c.env * m.nb + b) * 36;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int k = 0; k < 6; ++k) out[i * 6 + k] = M[i][k];
    }
}

// H [env_count * na][D][D] and (optional) body_I_s.  Twists and inertias are referenced to the position of the articulation's root
// link (H does not depend on the point; world coordinates of a far-away world would cost the m |c|^2 terms their digits).
template <int EPB>
__global__ void __launch_bounds__(256) eval_mass_matrix_kernel(KArgs a, float* H, float* body_I_s, const uint8_t* art_mask) {
    extern __shared__ __align__(16) float lds[];
    const nt_model& m = a.m;
    constexpr int N = Ctx<EPB>::N;
    const JmLayout F = jm_layout(m, Ctx<EPB>::UNI, true);
    Ctx<EPB> c(a, lds, F.rows);
    int* extra = c.own_tables(jm_table_ints(m));
    __syncthreads();
    jm_build_tables(c, extra);
    const JmCtx<EPB> f(c, F, extra);
    const int max_depth = f.max_depth(), D = m.max_art_dofs;
    jm_load(c, F);
    __syncthreads();
    auto selected = [&](int j) { return !art_mask || art_mask[(size_t)c.env * m.na + f.art[j]]; };
    auto root_pos = [&](int j) { return c.body_q(c.T.joint_child[m.art_start[f.art[j]]]).p; };
    if (c.valid) {
        for (int d = c.slot; d < m.nd; d += c.nslot)
            if (selected(f.dof_joint[d])) jm_S_item(f, d, root_pos(f.dof_joint[d]));
        for (int j = c.slot; j < m.nj; j += c.nslot)
            if (selected(j)) jm_inertia_item(f, j, root_pos(j), body_I_s);
    }
    __syncthreads();
    // composite inertias up the tree: a joint adds its children's (complete since the previous interval) in ascending joint order
    for (int lvl = max_depth - 1; lvl >= 0; --lvl) {
        if (c.valid)
            for (int j = c.slot; j < m.nj; j += c.nslot) {
                if (f.depth[j] != lvl || !selected(j)) continue;
                float acc[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) acc[k] = f.Ic(k, j);
                for (int ch = m.art_start[f.art[j]]; ch < m.art_start[f.art[j] + 1]; ++ch) {
                    if (f.anc[ch] != j) continue;
#pragma unroll
                    for (int k = 0; k < 10; ++k) acc[k] += f.Ic(k, ch);
                }
#pragma unroll
                for (int k = 0; k < 10; ++k) f.Ic(k, j) = acc[k];
            }
        __syncthreads();
    }
    // H_ij = S_i . (I^c_deeper S_j) for ancestor-related dofs i >= j of one articulation, both triangles from one lane
    if (c.valid)
        for (int item = c.slot; item < m.nd * D; item += c.nslot) {
            const int i = item / D, lj = item - i * D, ji = f.dof_joint[i];
            if (!selected(ji)) continue;
            const int d0 = c.T.joint_qd_start[m.art_start[f.art[ji]]], j = d0 + lj;
            if (j > i) continue;
            const int jj = f.dof_joint[j];
            const int deep = f.on_path(jj, ji) ? ji : (f.on_path(ji, jj) ? jj : -1);
            float h = 0.0f;
            if (deep >= 0) {
                const vec3 vi(f.S(c.e, 0, i), f.S(c.e, 1, i), f.S(c.e, 2, i)), wi(f.S(c.e, 3, i), f.S(c.e, 4, i), f.S(c.e, 5, i));
                const vec3 vj(f.S(c.e, 0, j), f.S(c.e, 1, j), f.S(c.e, 2, j)), wj(f.S(c.e, 3, j), f.S(c.e, 4, j), f.S(c.e, 5, j));
                const float mass = f.Ic(0, deep);
                const vec3 hm(f.Ic(1, deep), f.Ic(2, deep), f.Ic(3, deep));
                const float xx = f.Ic(4, deep), xy = f.Ic(5, deep), xz = f.Ic(6, deep), yy = f.Ic(7, deep), yz = f.Ic(8, deep), zz = f.Ic(9, deep);
                const vec3 top = vj * mass + cross(wj, hm);
                const vec3 bottom = cross(hm, vj) + vec3(xx * wj.x + xy * wj.y + xz * wj.z, xy * wj.x + yy * wj.y + yz * wj.z,
                                                        xz * wj.x + yz * wj.y + zz * wj.z);
                h = dot(vi, top) + dot(wi, bottom);
            }
            f.H(c.e, i, lj) = h;
            f.H(c.e, j, i - d0) = h;
        }
    __syncthreads();
    const int block = D * D;
    for (int t = 0; t < N * m.na; ++t) {
        const int e = t / m.na, k = t - e * m.na, env = blockIdx.x * N + e;
        if (env >= m.env_count) break;
        if (art_mask && !art_mask[(size_t)env * m.na + k]) continue;
        const int j0 = m.art_start[k], nja = m.art_start[k + 1] - j0;
        const int d0 = nja > 0 ? c.T.joint_qd_start[j0] : 0, nda = nja > 0 ? f.qd_end(j0 + nja - 1) - d0 : 0;
        float* out = H + (size_t)((size_t)env * m.na + k) * block;
        for (int i = threadIdx.x; i < block; i += blockDim.x) {
            const int li = i / D, lj = i - li * D;
            out[i] = li < nda && lj < nda ? f.H(e, d0 + li, lj) : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// nt_eval_inverse_dynamics (contract: include/newton_hip_kinematics.h): tau = sum_l J_l^T f_l, f_l = I_l a_l + v_l x* (I_l v_l) with
// gravity entering as the root acceleration -g.  Tile: eval_jacobian_kernel's (poses, parameters, joint_q, S), then the link inertias
// [10][nj] (NOT composed), joint_qd [nd], joint_qdd [nd] (gathered from the public layout), the joint pivots [3][nj], the link wrenches
// [6][nj] and tau (env-major [e][nd], odd stride).  Twists, accelerations and wrenches are spatial (the body-fixed point that passes
// through the reference point), referenced to the articulation's root link position; tau does not depend on the point.
// One lane per (environment, link) walks the dofs on the link's root path in ascending order -- the ancestors' dofs come first, the
// model builder's order -- and carries the running twist: at dof d it IS the twist of the frame that carries d's pivot (the parent
// link plus the joint's earlier dofs; those act through the pivot or are linear), and its angular part the rate of the frame that
// carries d's axis for a D6 (parent plus the earlier angular dofs); every other type's axes ride on the parent: the angular rate
// when the walk entered the joint.  The link's wrench follows in the same lane: v, a and f never leave registers between the two.
// ------------------------------------------------------------------------------------------------
struct IdLayout {
    JmLayout F;
    int qd, qdd, piv, f, tau, TW;
};
__host__ __device__ inline IdLayout id_layout(const nt_model& m, const bool uni) {
    IdLayout I;
    I.F = jm_layout(m, uni, false);
    int o = I.F.rows;
    I.F.Ic = o; o += 10 * m.nj;
    I.qd = o; o += m.nd;
    I.qdd = o; o += m.nd;
    I.piv = o; o += 3 * m.nj;
    I.f = o; o += 6 * m.nj;
    I.TW = m.nd | 1;
    I.tau = o; o += I.TW;
    I.F.rows = o;
    return I;
}

// the pivot of joint j's angular dofs (jm_S_item's)
template <int EPB>
NT_DI vec3 id_pivot(const JmCtx<EPB>& f, int j) {
    const Ctx<EPB>& c = f.c;
    const nt_model& m = c.a.m;
    const int parent = c.T.joint_parent[j], child = c.T.joint_child[j], type = c.T.joint_type[j];
    if (type == JT_FREE || type == JT_DISTANCE) return xform_point(c.body_q(child), c.com(child));
    xform X_wpj = c.plxf(c.L.jp, 0, m.nj, j);
    if (parent >= 0) X_wpj = c.body_q(parent) * X_wpj;
    if (type != JT_D6) return X_wpj.p;
    const int ds = c.T.joint_qd_start[j], cs = c.T.joint_q_start[j], lin = c.T.joint_lin_count[j];
    vec3 pos(0.0f);
    for (int i = 0; i < lin; ++i) pos += c.dof_axis(ds + i) * f.jq(cs + i);
    return xform_point(X_wpj, pos);
}

// tau [env_count * na][D] in the public layout; joint_qdd the same layout or NULL (zero).  art_mask as for eval_ik_kernel.
template <int EPB>
__global__ void __launch_bounds__(256) eval_inverse_dynamics_kernel(KArgs a, const float* joint_qdd, int flags, float* tau,
                                                                    const uint8_t* art_mask) {
    extern __shared__ __align__(16) float lds[];
    const nt_model& m = a.m;
    constexpr int N = Ctx<EPB>::N;
    const IdLayout I = id_layout(m, Ctx<EPB>::UNI);
    Ctx<EPB> c(a, lds, I.F.rows);
    int* extra = c.own_tables(jm_table_ints(m));
    __syncthreads();
    jm_build_tables(c, extra);
    const JmCtx<EPB> f(c, I.F, extra);
    const int D = m.max_art_dofs;
    jm_load(c, I.F);
    const bool with_velocity = (flags & NT_ID_VELOCITY) != 0;
    if (c.valid) {
        if (with_velocity) stage_rows(c, I.qd, a.s_in.joint_qd, m.nd);
        else
            for (int d = c.slot; d < m.nd; d += c.nslot) lds[(I.qd + d) * N + c.e] = 0.0f;
    }
    // joint_qdd: the tile's articulations out of the public layout, consecutive lanes on consecutive dofs
    for (int t = 0; t < N * m.na; ++t) {
        const int e = t / m.na, k = t - e * m.na, env = blockIdx.x * N + e;
        if (env >= m.env_count) break;
        if (art_mask && !art_mask[(size_t)env * m.na + k]) continue;
        const int j0 = m.art_start[k], nja = m.art_start[k + 1] - j0;
        const int d0 = nja > 0 ? c.T.joint_qd_start[j0] : 0, nda = nja > 0 ? f.qd_end(j0 + nja - 1) - d0 : 0;
        const float* in = joint_qdd ? joint_qdd + (size_t)((size_t)env * m.na + k) * D : nullptr;
        for (int i = threadIdx.x; i < nda; i += blockDim.x) lds[(I.qdd + d0 + i) * N + e] = in ? in[i] : 0.0f;
    }
    __syncthreads();
    auto selected = [&](int j) { return !art_mask || art_mask[(size_t)c.env * m.na + f.art[j]]; };
    auto root_pos = [&](int j) { return c.body_q(c.T.joint_child[m.art_start[f.art[j]]]).p; };
    auto row3 = [&](int off, int j) { return vec3(lds[(off + j) * N + c.e], lds[(off + m.nj + j) * N + c.e], lds[(off + 2 * m.nj + j) * N + c.e]); };
    auto S_lin = [&](int d) { return vec3(f.S(c.e, 0, d), f.S(c.e, 1, d), f.S(c.e, 2, d)); };
    auto S_ang = [&](int d) { return vec3(f.S(c.e, 3, d), f.S(c.e, 4, d), f.S(c.e, 5, d)); };
    // (1) S_d, the link inertias and the pivots, about the root link position
    if (c.valid) {
        for (int d = c.slot; d < m.nd; d += c.nslot)
            if (selected(f.dof_joint[d])) jm_S_item(f, d, root_pos(f.dof_joint[d]));
        for (int j = c.slot; j < m.nj; j += c.nslot) {
            if (!selected(j)) continue;
            jm_inertia_item(f, j, root_pos(j), nullptr);
            const vec3 p = id_pivot(f, j) - root_pos(j);
            lds[(I.piv + j) * N + c.e] = p.x; lds[(I.piv + m.nj + j) * N + c.e] = p.y; lds[(I.piv + 2 * m.nj + j) * N + c.e] = p.z;
        }
    }
    __syncthreads();
    // (2) + (3) per (environment, link): v_l and a_l over the dofs on the root path, then f_l
    if (c.valid)
        for (int j = c.slot; j < m.nj; j += c.nslot) {
            if (!selected(j)) continue;
            const int d0 = c.T.joint_qd_start[m.art_start[f.art[j]]], d1 = f.qd_end(j);
            vec3 v, w, al, aw, w_parent;
            if (flags & NT_ID_GRAVITY) al = -c.gravity();
            for (int d = d0; d < d1; ++d) {
                const int jd = f.dof_joint[d];
                if (!f.on_path(jd, j)) continue;
                const int ds = c.T.joint_qd_start[jd], type = c.T.joint_type[jd], k = d - ds;
                if (k == 0) w_parent = w;
                const bool angular = type == JT_REVOLUTE || type == JT_BALL || ((type == JT_FREE || type == JT_DISTANCE) && k >= 3) ||
                                     (type == JT_D6 && k >= c.T.joint_lin_count[jd]);
                const vec3 sv = S_lin(d), sw = S_ang(d), w_frame = type == JT_D6 ? w : w_parent;
                const float qd = lds[(I.qd + d) * N + c.e], qdd = lds[(I.qdd + d) * N + c.e];
                vec3 dtop, dbottom;
                if (angular) {
                    const vec3 r = row3(I.piv, jd), p_dot = v + cross(w, r);
                    dbottom = cross(w_frame, sw);
                    dtop = cross(p_dot, sw) + cross(r, dbottom);
                } else {
                    dtop = cross(w_frame, sv);
                }
                al += sv * qdd + dtop * qd;
                aw += sw * qdd + dbottom * qd;
                v += sv * qd;
                w += sw * qd;
            }
            const float mass = f.Ic(0, j);
            const vec3 hm(f.Ic(1, j), f.Ic(2, j), f.Ic(3, j));
            const float xx = f.Ic(4, j), xy = f.Ic(5, j), xz = f.Ic(6, j), yy = f.Ic(7, j), yz = f.Ic(8, j), zz = f.Ic(9, j);
            auto rot = [&](vec3 u) { return vec3(xx * u.x + xy * u.y + xz * u.z, xy * u.x + yy * u.y + yz * u.z, xz * u.x + yz * u.y + zz * u.z); };
            const vec3 p_lin = v * mass + cross(w, hm), p_ang = cross(hm, v) + rot(w);  // I v
            const vec3 f_lin = (al * mass + cross(aw, hm)) + cross(w, p_lin);
            const vec3 f_ang = (cross(hm, al) + rot(aw)) + (cross(w, p_ang) + cross(v, p_lin));
            lds[(I.f + j) * N + c.e] = f_lin.x; lds[(I.f + m.nj + j) * N + c.e] = f_lin.y; lds[(I.f + 2 * m.nj + j) * N + c.e] = f_lin.z;
            lds[(I.f + 3 * m.nj + j) * N + c.e] = f_ang.x; lds[(I.f + 4 * m.nj + j) * N + c.e] = f_ang.y; lds[(I.f + 5 * m.nj + j) * N + c.e] = f_ang.z;
        }
    __syncthreads();
    // (4) per (environment, dof): S_d . f_l over the links whose root path holds the dof, in ascending joint order
    if (c.valid)
        for (int d = c.slot; d < m.nd; d += c.nslot) {
            const int jd = f.dof_joint[d];
            if (!selected(jd)) continue;
            const vec3 sv = S_lin(d), sw = S_ang(d);
            float acc = 0.0f;
            for (int l = jd; l < m.art_start[f.art[jd] + 1]; ++l)
                if (f.on_path(jd, l)) acc += dot(sv, row3(I.f, l)) + dot(sw, row3(I.f + 3 * m.nj, l));
            lds[I.tau * N + c.e * I.TW + d] = acc;
        }
    __syncthreads();
    for (int t = 0; t < N * m.na; ++t) {
        const int e = t / m.na, k = t - e * m.na, env = blockIdx.x * N + e;
        if (env >= m.env_count) break;
        if (art_mask && !art_mask[(size_t)env * m.na + k]) continue;
        const int j0 = m.art_start[k], nja = m.art_start[k + 1] - j0;
        const int d0 = nja > 0 ? c.T.joint_qd_start[j0] : 0, nda = nja > 0 ? f.qd_end(j0 + nja - 1) - d0 : 0;
        float* out = tau + (size_t)((size_t)env * m.na + k) * D;
        for (int i = threadIdx.x; i < D; i += blockDim.x) out[i] = i < nda ? lds[I.tau * N + e * I.TW + d0 + i] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------
// nt_eval_forward_dynamics (contract: include/newton_hip_kinematics.h): H qdd = joint_f + sum_l J_l^T w_l - h.  The two kernels above
// composed without a trip through HBM: eval_inverse_dynamics_kernel's walk at qdd = 0 gives the link wrenches f_l (the external wrench
// w_l, carried from the link's COM to the root link position, is subtracted in the same lane), the per-dof sum gives
// rhs_d = joint_f_d - sum_l S_d . f_l; eval_mass_matrix_kernel's composite inertias and entry items give H; then a Cholesky per
// articulation, column by column as in ik_solve_kernel, and the two triangular solves.  Tile: id_layout (its joint_qdd rows hold joint_f,
// then rhs, then y; its tau block receives qdd), then the composite inertias [10][nj] (the link inertias stay: the wrench phase reads
// them), H (env-major [e][nd][D], factored in place: the strict lower triangle becomes L), the factor's diagonal [nd], the first failing
// column per articulation [na] and, with NT_FD_BODY_F, the staged body_f [6][nb].
// H is block diagonal: column j = 0 .. D - 1 of EVERY articulation wider than j is one barrier interval (D intervals, not nd), and a
// pivot that is not > 0 stays in its own block: it is replaced by 1 so that the interval's arithmetic goes on, the column is recorded,
// and the articulation's result is NaN.  Every lane of a column forms the pivot of its articulation from the same entries in the same
// order (the same bits); the lane of the diagonal row stores it.
// ------------------------------------------------------------------------------------------------
struct FdLayout {
    IdLayout I;
    int Icc, Dg, info, bf;
};
__host__ __device__ inline FdLayout fd_layout(const nt_model& m, const bool uni, const bool body_f) {
    FdLayout X;
    X.I = id_layout(m, uni);
    int o = X.I.F.rows;
    X.Icc = o; o += 10 * m.nj;
    X.I.F.HW = (m.nd * m.max_art_dofs) | 1;
    X.I.F.H = o; o += X.I.F.HW;
    X.Dg = o; o += m.nd;
    X.info = o; o += m.na;
    X.bf = o; o += body_f ? 6 * m.nb : 0;
    X.I.F.rows = o;
    return X;
}

// joint_qdd [env_count * na][D] and info [env_count * na] (or NULL); joint_f the layout of joint_qdd or NULL (zero).  art_mask as for
// eval_ik_kernel.
template <int EPB>
__global__ void __launch_bounds__(256) eval_forward_dynamics_kernel(KArgs a, const float* joint_f, int flags, float* joint_qdd, int* info,
                                                                    const uint8_t* art_mask) {
    extern __shared__ __align__(16) float lds[];
    const nt_model& m = a.m;
    constexpr int N = Ctx<EPB>::N;
    const bool with_body_f = (flags & NT_FD_BODY_F) != 0;
    const FdLayout X = fd_layout(m, Ctx<EPB>::UNI, with_body_f);
    const IdLayout& I = X.I;
    Ctx<EPB> c(a, lds, I.F.rows);
    int* extra = c.own_tables(jm_table_ints(m));
    __syncthreads();
    jm_build_tables(c, extra);
    const JmCtx<EPB> f(c, I.F, extra);
    const int max_depth = f.max_depth(), D = m.max_art_dofs;
    jm_load(c, I.F);
    if (c.valid) {
        if (flags & NT_FD_VELOCITY) stage_rows(c, I.qd, a.s_in.joint_qd, m.nd);
        else
            for (int d = c.slot; d < m.nd; d += c.nslot) lds[(I.qd + d) * N + c.e] = 0.0f;
        if (with_body_f) stage_rows(c, X.bf, a.s_in.body_f, 6 * m.nb);
        for (int k = c.slot; k < m.na; k += c.nslot) lds[(X.info + k) * N + c.e] = 0.0f;
    }
    // joint_f: the tile's articulations out of the public layout, consecutive lanes on consecutive dofs
    for (int t = 0; t < N * m.na; ++t) {
        const int e = t / m.na, k = t - e * m.na, env = blockIdx.x * N + e;
        if (env >= m.env_count) break;
        if (art_mask && !art_mask[(size_t)env * m.na + k]) continue;
        const int j0 = m.art_start[k], nja = m.art_start[k + 1] - j0;
        const int d0 = nja > 0 ? c.T.joint_qd_start[j0] : 0, nda = nja > 0 ? f.qd_end(j0 + nja - 1) - d0 : 0;
        const float* in = joint_f ? joint_f + (size_t)((size_t)env * m.na + k) * D : nullptr;
        for (int i = threadIdx.x; i < nda; i += blockDim.x) lds[(I.qdd + d0 + i) * N + e] = in ? in[i] : 0.0f;
    }
    __syncthreads();
    auto selected = [&](int j) { return !art_mask || art_mask[(size_t)c.env * m.na + f.art[j]]; };
    auto root_pos = [&](int j) { return c.body_q(c.T.joint_child[m.art_start[f.art[j]]]).p; };
    auto row3 = [&](int off, int j) { return vec3(lds[(off + j) * N + c.e], lds[(off + m.nj + j) * N + c.e], lds[(off + 2 * m.nj + j) * N + c.e]); };
    auto S_lin = [&](int d) { return vec3(f.S(c.e, 0, d), f.S(c.e, 1, d), f.S(c.e, 2, d)); };
    auto S_ang = [&](int d) { return vec3(f.S(c.e, 3, d), f.S(c.e, 4, d), f.S(c.e, 5, d)); };
    auto Icc = [&](int comp, int j) -> float& { return lds[(X.Icc + comp * m.nj + j) * N + c.e]; };
    auto rhs = [&](int d) -> float& { return lds[(I.qdd + d) * N + c.e]; };
    auto Dg = [&](int d) -> float& { return lds[(X.Dg + d) * N + c.e]; };
    auto first_dof = [&](int k) { return c.T.joint_qd_start[m.art_start[k]]; };
    // (1) S_d, the link inertias and the pivots, about the root link position: eval_inverse_dynamics_kernel's interval (1)
    if (c.valid) {
        for (int d = c.slot; d < m.nd; d += c.nslot)
            if (selected(f.dof_joint[d])) jm_S_item(f, d, root_pos(f.dof_joint[d]));
        for (int j = c.slot; j < m.nj; j += c.nslot) {
            if (!selected(j)) continue;
            jm_inertia_item(f, j, root_pos(j), nullptr);
            const vec3 p = id_pivot(f, j) - root_pos(j);
            lds[(I.piv + j) * N + c.e] = p.x; lds[(I.piv + m.nj + j) * N + c.e] = p.y; lds[(I.piv + 2 * m.nj + j) * N + c.e] = p.z;
        }
    }
    __syncthreads();
    // (2) per (environment, link): eval_inverse_dynamics_kernel's walk with qdd = 0, f_l minus the external wrench about the root link
    // position; the link's own inertia seeds its composite row
    if (c.valid)
        for (int j = c.slot; j < m.nj; j += c.nslot) {
            if (!selected(j)) continue;
            const int d0 = first_dof(f.art[j]), d1 = f.qd_end(j);
            vec3 v, w, al, aw, w_parent;
            if (flags & NT_FD_GRAVITY) al = -c.gravity();
            for (int d = d0; d < d1; ++d) {
                const int jd = f.dof_joint[d];
                if (!f.on_path(jd, j)) continue;
                const int ds = c.T.joint_qd_start[jd], type = c.T.joint_type[jd], k = d - ds;
                if (k == 0) w_parent = w;
                const bool angular = type == JT_REVOLUTE || type == JT_BALL || ((type == JT_FREE || type == JT_DISTANCE) && k >= 3) ||
                                     (type == JT_D6 && k >= c.T.joint_lin_count[jd]);
                const vec3 sv = S_lin(d), sw = S_ang(d), w_frame = type == JT_D6 ? w : w_parent;
                const float qd = lds[(I.qd + d) * N + c.e];
                vec3 dtop, dbottom;
                if (angular) {
                    const vec3 r = row3(I.piv, jd), p_dot = v + cross(w, r);
                    dbottom = cross(w_frame, sw);
                    dtop = cross(p_dot, sw) + cross(r, dbottom);
                } else {
                    dtop = cross(w_frame, sv);
                }
                al += dtop * qd;
                aw += dbottom * qd;
                v += sv * qd;
                w += sw * qd;
            }
            const float mass = f.Ic(0, j);
            const vec3 hm(f.Ic(1, j), f.Ic(2, j), f.Ic(3, j));
            const float xx = f.Ic(4, j), xy = f.Ic(5, j), xz = f.Ic(6, j), yy = f.Ic(7, j), yz = f.Ic(8, j), zz = f.Ic(9, j);
            auto rot = [&](vec3 u) { return vec3(xx * u.x + xy * u.y + xz * u.z, xy * u.x + yy * u.y + yz * u.z, xz * u.x + yz * u.y + zz * u.z); };
            const vec3 p_lin = v * mass + cross(w, hm), p_ang = cross(hm, v) + rot(w);  // I v
            vec3 f_lin = (al * mass + cross(aw, hm)) + cross(w, p_lin);
            vec3 f_ang = (cross(hm, al) + rot(aw)) + (cross(w, p_ang) + cross(v, p_lin));
            if (with_body_f) {  // body_f: world-frame force and torque about the link's COM
                const int b = c.T.joint_child[j];
                const vec3 F = c.lv3(X.bf, 0, m.nb, b), T = c.lv3(X.bf, 3, m.nb, b);
                const vec3 r = xform_point(c.body_q(b), c.com(b)) - root_pos(j);
                f_lin = f_lin - F;
                f_ang = f_ang - (T + cross(r, F));
            }
            lds[(I.f + j) * N + c.e] = f_lin.x; lds[(I.f + m.nj + j) * N + c.e] = f_lin.y; lds[(I.f + 2 * m.nj + j) * N + c.e] = f_lin.z;
            lds[(I.f + 3 * m.nj + j) * N + c.e] = f_ang.x; lds[(I.f + 4 * m.nj + j) * N + c.e] = f_ang.y; lds[(I.f + 5 * m.nj + j) * N + c.e] = f_ang.z;
            Icc(0, j) = mass;
            Icc(1, j) = hm.x; Icc(2, j) = hm.y; Icc(3, j) = hm.z;
            Icc(4, j) = xx; Icc(5, j) = xy; Icc(6, j) = xz; Icc(7, j) = yy; Icc(8, j) = yz; Icc(9, j) = zz;
        }
    __syncthreads();
    // (3) rhs_d = joint_f_d - sum_l S_d . f_l (eval_inverse_dynamics_kernel's interval (4)) shares the first interval of the composite
    // inertia level loop -- or, on a tree of depth 0, the interval of the H entries: they meet only in the solve
    if (c.valid)
        for (int d = c.slot; d < m.nd; d += c.nslot) {
            const int jd = f.dof_joint[d];
            if (!selected(jd)) continue;
            const vec3 sv = S_lin(d), sw = S_ang(d);
            float acc = 0.0f;
            for (int l = jd; l < m.art_start[f.art[jd] + 1]; ++l)
                if (f.on_path(jd, l)) acc += dot(sv, row3(I.f, l)) + dot(sw, row3(I.f + 3 * m.nj, l));
            rhs(d) = rhs(d) - acc;
        }
    for (int lvl = max_depth - 1; lvl >= 0; --lvl) {  // (eval_mass_matrix_kernel's level loop on the composite rows)
        if (c.valid)
            for (int j = c.slot; j < m.nj; j += c.nslot) {
                if (f.depth[j] != lvl || !selected(j)) continue;
                float acc[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) acc[k] = Icc(k, j);
                for (int ch = m.art_start[f.art[j]]; ch < m.art_start[f.art[j] + 1]; ++ch) {
                    if (f.anc[ch] != j) continue;
#pragma unroll
                    for (int k = 0; k < 10; ++k) acc[k] += Icc(k, ch);
                }
#pragma unroll
                for (int k = 0; k < 10; ++k) Icc(k, j) = acc[k];
            }
        __syncthreads();
    }
    // H_ij = S_i . (I^c_deeper S_j): eval_mass_matrix_kernel's entry items, both triangles from one lane
    if (c.valid)
        for (int item = c.slot; item < m.nd * D; item += c.nslot) {
            const int i = item / D, lj = item - i * D, ji = f.dof_joint[i];
            if (!selected(ji)) continue;
            const int d0 = first_dof(f.art[ji]), j = d0 + lj;
            if (j > i) continue;
            const int jj = f.dof_joint[j];
            const int deep = f.on_path(jj, ji) ? ji : (f.on_path(ji, jj) ? jj : -1);
            float h = 0.0f;
            if (deep >= 0) {
                const vec3 vi = S_lin(i), wi = S_ang(i), vj = S_lin(j), wj = S_ang(j);
                const float mass = Icc(0, deep);
                const vec3 hm(Icc(1, deep), Icc(2, deep), Icc(3, deep));
                const float xx = Icc(4, deep), xy = Icc(5, deep), xz = Icc(6, deep), yy = Icc(7, deep), yz = Icc(8, deep), zz = Icc(9, deep);
                const vec3 top = vj * mass + cross(wj, hm);
                const vec3 bottom = cross(hm, vj) + vec3(xx * wj.x + xy * wj.y + xz * wj.z, xy * wj.x + yy * wj.y + yz * wj.z,
                                                        xz * wj.x + yz * wj.y + zz * wj.z);
                h = dot(vi, top) + dot(wi, bottom);
            }
            f.H(c.e, i, lj) = h;
            f.H(c.e, j, i - d0) = h;
        }
    __syncthreads();
    // (4) Cholesky in place, per articulation: in interval j the lane of dof row i = d0 + li (li >= j) of an articulation forms the
    // pivot of column j, stores it (li == j) or divides its own entry L(li, j) by it; rows above the column rest
    for (int j = 0; j < D; ++j) {
        if (c.valid)
            for (int i = c.slot; i < m.nd; i += c.nslot) {
                const int ji = f.dof_joint[i], k = f.art[ji], d0 = first_dof(k), li = i - d0;
                if (li < j || !selected(ji)) continue;
                const int dj = d0 + j;
                // row dj of L is read once for both sums (on the diagonal lane t repeats p); the loads of four terms leave together
                float p = f.H(c.e, dj, j), t = f.H(c.e, i, j);
#pragma unroll 4
                for (int q = 0; q < j; ++q) {
                    const float l = f.H(c.e, dj, q);
                    p -= l * l;
                    t -= f.H(c.e, i, q) * l;
                }
                const bool bad = !(p > 0.0f);
                if (bad) p = 1.0f;
                p = sqrtf(p);
                if (li == j) {
                    Dg(dj) = p;
                    float& first_bad = lds[(X.info + k) * N + c.e];
                    if (bad && first_bad == 0.0f) first_bad = (float)(j + 1);
                } else {
                    f.H(c.e, i, j) = t / p;
                }
            }
        __syncthreads();
    }
    // (5) L y = rhs, L^T qdd = y: one lane per (environment, articulation), each sum in ascending order
    if (c.valid)
        for (int k = c.slot; k < m.na; k += c.nslot) {
            const int j0 = m.art_start[k], nja = m.art_start[k + 1] - j0;
            if (nja <= 0 || !selected(j0)) continue;
            const int d0 = c.T.joint_qd_start[j0], nda = f.qd_end(j0 + nja - 1) - d0;
            float* out = lds + I.tau * N + c.e * I.TW + d0;
            if (lds[(X.info + k) * N + c.e] != 0.0f) {
                for (int i = 0; i < nda; ++i) out[i] = __builtin_nanf("");
                continue;
            }
            for (int i = 0; i < nda; ++i) {
                float t = rhs(d0 + i);
#pragma unroll 4
                for (int q = 0; q < i; ++q) t -= f.H(c.e, d0 + i, q) * rhs(d0 + q);
                rhs(d0 + i) = t / Dg(d0 + i);
            }
            for (int i = nda - 1; i >= 0; --i) {
                float t = rhs(d0 + i);
#pragma unroll 4
                for (int q = i + 1; q < nda; ++q) t -= f.H(c.e, d0 + q, i) * out[q];
                out[i] = t / Dg(d0 + i);
            }
        }
    __syncthreads();
    for (int t = 0; t < N * m.na; ++t) {
        const int e = t / m.na, k = t - e * m.na, env = blockIdx.x * N + e;
        if (env >= m.env_count) break;
        if (art_mask && !art_mask[(size_t)env * m.na + k]) continue;
        const int j0 = m.art_start[k], nja = m.art_start[k + 1] - j0;
        const int d0 = nja > 0 ? c.T.joint_qd_start[j0] : 0, nda = nja > 0 ? f.qd_end(j0 + nja - 1) - d0 : 0;
        float* out = joint_qdd + (size_t)((size_t)env * m.na + k) * D;
        for (int i = threadIdx.x; i < D; i += blockDim.x) out[i] = i < nda ? lds[I.tau * N + e * I.TW + d0 + i] : 0.0f;
        if (info && threadIdx.x == 0) info[(size_t)env * m.na + k] = (int)lds[(X.info + k) * N + e];
    }
}

// ------------------------------------------------------------------------------------------------
// nt_ik_solve (newton.ik.IKSolver.step; contract: include/newton_hip_kinematics.h): batched Levenberg-Marquardt IK, one problem per
// environment, all iterations in one launch.  Tile: eval_jacobian_kernel's (poses, parameters, joint_q, S), then the candidate's
// joint_q' [nc] and poses [7 nb], the residual blocks of the accepted point and of the candidate (position: residual + world point, 6
// rows; rotation 3; joint limit nd), the staged targets, the packed lower triangle of J^T J [nd (nd + 1) / 2] (factored in place, the
// factor's diagonal beside it), g, delta.  Block-shared behind eval_jacobian's tables: the objective table, IKS_WORDS words each.
// Every entry of A, g, the factor and every residual row is produced by ONE lane in a fixed order, the scalars (cost, predicted
// reduction, decision, lambda) by every lane of the environment from the same LDS values: no atomics, no broadcast, the same bits for
// every tile width.  Barriers are workgroup-wide: every loop bound is block-uniform.
// ------------------------------------------------------------------------------------------------
constexpr int IKS_WORDS = 12;  // type, link, flags, weight, offset[4], the link's joint, first residual row, first target row, spare
__host__ __device__ inline int iks_res_rows(int type, int nd) { return type == NT_IK_POSITION ? 6 : (type == NT_IK_ROTATION ? 3 : nd); }
__host__ __device__ inline int iks_tgt_rows(int type, int nd) { return type == NT_IK_POSITION ? 3 : (type == NT_IK_ROTATION ? 4 : 2 * nd); }
struct IksLayout {
    JmLayout J;
    int jq2, bq2, R, R2, T, A, Dg, g, X, nR, nT, nA, rows;
};
__host__ __device__ inline IksLayout iks_layout(const nt_model& m, const nt_ik_problem& P, const bool uni) {
    IksLayout F;
    F.J = jm_layout(m, uni, false);
    F.nR = F.nT = 0;
    for (int k = 0; k < P.count; ++k) {
        F.nR += iks_res_rows(P.obj[k].type, m.nd);
        F.nT += iks_tgt_rows(P.obj[k].type, m.nd);
    }
    F.nA = m.nd * (m.nd + 1) / 2;
    int o = F.J.rows;
    F.jq2 = o; o += m.nc;
    F.bq2 = o; o += 7 * m.nb;
    F.R = o; o += F.nR;
    F.R2 = o; o += F.nR;
    F.T = o; o += F.nT;
    F.A = o; o += F.nA;
    F.Dg = o; o += m.nd;
    F.g = o; o += m.nd;
    F.X = o; o += m.nd;
    F.rows = o;
    return F;
}
__host__ __device__ inline int iks_table_ints(const nt_model& m) { return jm_table_ints(m) + NT_IK_MAX_OBJECTIVES * IKS_WORDS; }

NT_DI quat iks_exp(vec3 d) {
    const float a = length(d);
    if (a > 0.0f) {
        const float h = 0.5f * a, s = sinf(h) / a;
        return quat(d.x * s, d.y * s, d.z * s, cosf(h));
    }
    return quat(0.5f * d.x, 0.5f * d.y, 0.5f * d.z, 1.0f);
}

template <int EPB>
struct IksCtx {
    const JmCtx<EPB>& f;
    const Ctx<EPB>& c;
    IksLayout F;
    const int* tab;
    int count;
    static constexpr int N = Ctx<EPB>::N;
    NT_DI IksCtx(const JmCtx<EPB>& f_, const IksLayout& F_, const int* tab_, int count_) : f(f_), c(f_.c), F(F_), tab(tab_), count(count_) {}
    NT_DI float& row(int r) const { return c.lds[r * N + c.e]; }
    NT_DI int type(int k) const { return tab[k * IKS_WORDS]; }
    NT_DI int link(int k) const { return tab[k * IKS_WORDS + 1]; }
    NT_DI int flags(int k) const { return tab[k * IKS_WORDS + 2]; }
    NT_DI float weight(int k) const { return reinterpret_cast<const float*>(tab)[k * IKS_WORDS + 3]; }
    NT_DI float offset(int k, int i) const { return reinterpret_cast<const float*>(tab)[k * IKS_WORDS + 4 + i]; }
    NT_DI int link_joint(int k) const { return tab[k * IKS_WORDS + 8]; }
    NT_DI int roff(int k) const { return tab[k * IKS_WORDS + 9]; }
    NT_DI int toff(int k) const { return tab[k * IKS_WORDS + 10]; }
    NT_DI xform pose(int bq, int b) const { return c.lxf(Fld<7>{bq}, 0, c.a.m.nb, b); }
    NT_DI vec3 S_lin(int d) const { return vec3(f.S(c.e, 0, d), f.S(c.e, 1, d), f.S(c.e, 2, d)); }
    NT_DI vec3 S_ang(int d) const { return vec3(f.S(c.e, 3, d), f.S(c.e, 4, d), f.S(c.e, 5, d)); }
    NT_DI float& A(int i, int j) const { return row(F.A + i * (i + 1) / 2 + j); }
};

// eval_fk's X_j of joint j from the coordinates in rows jq
template <int EPB>
NT_DI xform iks_joint_transform(const IksCtx<EPB>& s, int j, int jq) {
    const Ctx<EPB>& c = s.c;
    const int type = c.T.joint_type[j], ds = c.T.joint_qd_start[j], qs = c.T.joint_q_start[j];
    const int lin = c.T.joint_lin_count[j], ang = c.T.joint_ang_count[j];
    auto Q = [&](int i) { return s.row(jq + qs + i); };
    if (type == JT_PRISMATIC) return xform(c.dof_axis(ds) * Q(0), quat_identity());
    if (type == JT_REVOLUTE) return xform(vec3(), quat_from_axis_angle(c.dof_axis(ds), Q(0)));
    if (type == JT_BALL) return xform(vec3(), quat(Q(0), Q(1), Q(2), Q(3)));
    if (type == JT_FREE || type == JT_DISTANCE) return xform(vec3(Q(0), Q(1), Q(2)), quat(Q(3), Q(4), Q(5), Q(6)));
    if (type == JT_D6) {
        vec3 pos(0.0f);
        quat rot = quat_identity();
        for (int k = 0; k < lin; ++k) pos += c.dof_axis(ds + k) * Q(k);
        if (ang == 1) rot = quat_from_axis_angle(c.dof_axis(ds + lin), Q(lin));
        if (ang >= 2) {
            vec3 a0, a1, a2;
            rot = d6_multi_angular(ang, c.dof_axis(ds + lin), c.dof_axis(ds + lin + 1), ang == 3 ? c.dof_axis(ds + lin + 2) : vec3(), Q(lin),
                                   Q(lin + 1), ang == 3 ? Q(lin + 2) : 0.0f, a0, a1, a2);
        }
        return xform(pos, rot);
    }
    return xform(vec3(), quat_identity());
}

// body_q[child] of joint j (rows bq) from its parent's pose in the same rows and the coordinates in rows jq
template <int EPB>
NT_DI void iks_fk_item(const IksCtx<EPB>& s, int j, int jq, int bq) {
    const Ctx<EPB>& c = s.c;
    const nt_model& m = c.a.m;
    const int parent = c.T.joint_parent[j], child = c.T.joint_child[j];
    xform X_wpj = c.plxf(c.L.jp, 0, m.nj, j);
    if (parent >= 0) X_wpj = s.pose(bq, parent) * X_wpj;
    const xform X_wc = (X_wpj * iks_joint_transform(s, j, jq)) * xform_inverse(c.plxf(c.L.jp, 7, m.nj, j));
    c.st_lxf(Fld<7>{bq}, m.nb, child, X_wc);
}

template <int EPB>
NT_DI void iks_fk(const IksCtx<EPB>& s, int max_depth, int jq, int bq) {
    for (int lvl = 0; lvl <= max_depth; ++lvl) {
        if (s.c.valid)
            for (int j = s.c.slot; j < s.c.a.m.nj; j += s.c.nslot)
                if (s.f.depth[j] == lvl) iks_fk_item(s, j, jq, bq);
        __syncthreads();
    }
}

// the residual blocks (rows R) at the poses in rows bq / coordinates in rows jq: an objective per slot-lane, a limit row per slot-lane
template <int EPB>
NT_DI void iks_residuals(const IksCtx<EPB>& s, int jq, int bq, int R) {
    const Ctx<EPB>& c = s.c;
    const nt_model& m = c.a.m;
    for (int k = 0; k < s.count; ++k) {
        const int type = s.type(k), ro = R + s.roff(k), to = s.F.T + s.toff(k);
        const float w = s.weight(k);
        if (type == NT_IK_JOINT_LIMIT) {
            for (int d = c.slot; d < m.nd; d += c.nslot) {
                const int j = s.f.dof_joint[d], jt = c.T.joint_type[j];
                const float lo = s.row(to + d), hi = s.row(to + m.nd + d);
                float r = 0.0f;
                if ((jt == JT_PRISMATIC || jt == JT_REVOLUTE || jt == JT_D6) && lo < hi && fabsf(lo) < NT_MAXVAL && fabsf(hi) < NT_MAXVAL) {
                    const float q = s.row(jq + c.T.joint_q_start[j] + d - c.T.joint_qd_start[j]);
                    r = w * (fmaxw(0.0f, q - hi) - fmaxw(0.0f, lo - q));
                }
                s.row(ro + d) = r;
            }
            continue;
        }
        if (c.slot != k % c.nslot) continue;
        const xform X = s.pose(bq, s.link(k));
        if (type == NT_IK_POSITION) {
            const vec3 P = xform_point(X, vec3(s.offset(k, 0), s.offset(k, 1), s.offset(k, 2)));
            const vec3 r = (P - vec3(s.row(to), s.row(to + 1), s.row(to + 2))) * w;
            s.row(ro) = r.x; s.row(ro + 1) = r.y; s.row(ro + 2) = r.z;
            s.row(ro + 3) = P.x; s.row(ro + 4) = P.y; s.row(ro + 5) = P.z;
        } else {
            const quat target(s.row(to), s.row(to + 1), s.row(to + 2), s.row(to + 3));
            quat qe = (X.q * quat(s.offset(k, 0), s.offset(k, 1), s.offset(k, 2), s.offset(k, 3))) * quat_inverse(target);
            if ((s.flags(k) & NT_IK_CANONICALIZE) && qe.w < 0.0f) qe = quat(-qe.x, -qe.y, -qe.z, -qe.w);
            const float w2 = w * 2.0f;
            s.row(ro) = w2 * qe.x; s.row(ro + 1) = w2 * qe.y; s.row(ro + 2) = w2 * qe.z;
        }
    }
}

// C = |r|^2 / 2 over the residual rows of block R, in row order (every lane of the environment: the same sum)
template <int EPB>
NT_DI float iks_cost(const IksCtx<EPB>& s, int R) {
    float acc = 0.0f;
    for (int k = 0; k < s.count; ++k) {
        const int n = s.type(k) == NT_IK_JOINT_LIMIT ? s.c.a.m.nd : 3, ro = R + s.roff(k);
        for (int i = 0; i < n; ++i) {
            const float r = s.row(ro + i);
            acc += r * r;
        }
    }
    return 0.5f * acc;
}

// the Jacobian rows of objective k (position / rotation) in column d, without the weight
template <int EPB>
NT_DI vec3 iks_col(const IksCtx<EPB>& s, int k, int d) {
    if (s.type(k) == NT_IK_ROTATION) return s.S_ang(d);
    const int ro = s.F.R + s.roff(k);
    return s.S_lin(d) + cross(s.S_ang(d), vec3(s.row(ro + 3), s.row(ro + 4), s.row(ro + 5)));
}

// one entry of the lower triangle of J^T J (item < nA) or of g = J^T r: the objectives in order
template <int EPB>
NT_DI void iks_normal_item(const IksCtx<EPB>& s, int item) {
    const bool is_g = item >= s.F.nA;
    int i = 0, j = 0;
    if (is_g) {
        i = j = item - s.F.nA;
    } else {
        while ((i + 1) * (i + 2) / 2 <= item) ++i;
        j = item - i * (i + 1) / 2;
    }
    const int ji = s.f.dof_joint[i], jj = s.f.dof_joint[j];
    float acc = 0.0f;
    for (int k = 0; k < s.count; ++k) {
        const int type = s.type(k), ro = s.F.R + s.roff(k);
        const float w = s.weight(k);
        if (type == NT_IK_JOINT_LIMIT) {
            const float r = s.row(ro + i);
            if (i == j && r != 0.0f) acc += is_g ? w * r : w * w;
            continue;
        }
        const int lj = s.link_joint(k);
        if (!s.f.on_path(ji, lj) || !s.f.on_path(jj, lj)) continue;
        const vec3 ci = iks_col(s, k, i) * w;
        acc += is_g ? dot(ci, vec3(s.row(ro), s.row(ro + 1), s.row(ro + 2))) : dot(ci, iks_col(s, k, j) * w);
    }
    if (is_g) s.row(s.F.g + i) = acc;
    else s.row(s.F.A + item) = acc;
}

// joint_q (+) step * delta of joint j: rows jq -> rows jq2
template <int EPB>
NT_DI void iks_retract_item(const IksCtx<EPB>& s, int j, float step) {
    const Ctx<EPB>& c = s.c;
    const nt_model& m = c.a.m;
    const int type = c.T.joint_type[j], qs = c.T.joint_q_start[j], ds = c.T.joint_qd_start[j];
    const int qe = j + 1 < m.nj ? c.T.joint_q_start[j + 1] : m.nc;
    auto Q = [&](int i) { return s.row(s.F.J.jq + qs + i); };
    auto Q2 = [&](int i) -> float& { return s.row(s.F.jq2 + qs + i); };
    auto D = [&](int i) { return step * s.row(s.F.X + ds + i); };
    if (type == JT_PRISMATIC || type == JT_REVOLUTE || type == JT_D6) {
        for (int i = 0; i < qe - qs; ++i) Q2(i) = Q(i) + D(i);
    } else if (type == JT_BALL) {
        const quat q = normalize(iks_exp(vec3(D(0), D(1), D(2))) * quat(Q(0), Q(1), Q(2), Q(3)));
        Q2(0) = q.x; Q2(1) = q.y; Q2(2) = q.z; Q2(3) = q.w;
    } else if (type == JT_FREE || type == JT_DISTANCE) {
        // the child pose in the parent anchor frame Y = X_j X_c^-1: its COM translates, it rotates about the COM; X_j' = Y' X_c
        const xform X_c = c.plxf(c.L.jp, 7, m.nj, j);
        const vec3 com = c.com(c.T.joint_child[j]);
        const xform Y = xform(vec3(Q(0), Q(1), Q(2)), quat(Q(3), Q(4), Q(5), Q(6))) * xform_inverse(X_c);
        const quat qy = normalize(iks_exp(vec3(D(3), D(4), D(5))) * Y.q);
        const vec3 cy = xform_point(Y, com) + vec3(D(0), D(1), D(2));
        const xform Xn = xform(cy - quat_rotate(qy, com), qy) * X_c;
        Q2(0) = Xn.p.x; Q2(1) = Xn.p.y; Q2(2) = Xn.p.z;
        Q2(3) = Xn.q.x; Q2(4) = Xn.q.y; Q2(5) = Xn.q.z; Q2(6) = Xn.q.w;
    } else {
        for (int i = 0; i < qe - qs; ++i) Q2(i) = Q(i);
    }
}

template <int EPB>
__global__ void __launch_bounds__(256) ik_solve_kernel(KArgs a, nt_ik_problem P, const float* joint_q_in, float* joint_q_out, float* lambda,
                                                       float* cost, int iterations, float step) {
    extern __shared__ __align__(16) float lds[];
    const nt_model& m = a.m;
    const IksLayout F = iks_layout(m, P, Ctx<EPB>::UNI);
    Ctx<EPB> c(a, lds, F.rows);
    int* extra = c.own_tables(iks_table_ints(m));
    int* tab = extra + jm_table_ints(m);
    __syncthreads();
    jm_build_tables(c, extra);
    const JmCtx<EPB> f(c, F.J, extra);
    const IksCtx<EPB> s(f, F, tab, P.count);
    const int max_depth = f.max_depth(), nd = m.nd;
    // the objective table (one thread; the loop index is uniform: the kernel arguments are read with scalar loads)
    {
        int roff = 0, toff = 0;
        for (int k = 0; k < P.count; ++k) {
            const nt_ik_objective& o = P.obj[k];
            if (threadIdx.x == 0) {
                int lj = 0;
                for (int j = 0; j < m.nj; ++j)
                    if (c.T.joint_child[j] == o.link) lj = j;
                int* t = tab + k * IKS_WORDS;
                float* tf = reinterpret_cast<float*>(t);
                t[0] = o.type; t[1] = o.link; t[2] = o.flags; tf[3] = o.weight;
                tf[4] = o.offset[0]; tf[5] = o.offset[1]; tf[6] = o.offset[2]; tf[7] = o.offset[3];
                t[8] = lj; t[9] = roff; t[10] = toff; t[11] = 0;
            }
            const int nt = iks_tgt_rows(o.type, nd);
            if (c.valid)
                for (int r = c.slot; r < nt; r += c.nslot) s.row(F.T + toff + r) = o.target[(size_t)c.env * nt + r];
            roff += iks_res_rows(o.type, nd);
            toff += nt;
        }
    }
    load_params(c, false);
    if (c.valid)
        for (int i = c.slot; i < m.nc; i += c.nslot) s.row(F.J.jq + i) = joint_q_in[(size_t)c.env * m.nc + i];
    float lam = c.valid ? lambda[c.env] : 1.0f;
    __syncthreads();
    iks_fk(s, max_depth, F.J.jq, c.L.bq.off);
    if (c.valid) iks_residuals(s, F.J.jq, c.L.bq.off, F.R);
    __syncthreads();
    float C = c.valid ? iks_cost(s, F.R) : 0.0f;
    for (int it = 0; it < iterations; ++it) {
        if (c.valid)
            for (int d = c.slot; d < nd; d += c.nslot) jm_S_item(f, d, vec3());
        __syncthreads();
        if (c.valid)
            for (int item = c.slot; item < F.nA + nd; item += c.nslot) iks_normal_item(s, item);
        __syncthreads();
        // Cholesky of A + lambda I in place, column by column: the pivot by every lane, the column's rows dealt to the slot-lanes
        bool bad = false;
        for (int j = 0; j < nd; ++j) {
            if (c.valid) {
                float p = s.A(j, j) + lam;
                for (int k = 0; k < j; ++k) {
                    const float l = s.A(j, k);
                    p -= l * l;
                }
                if (!(p > 0.0f)) {
                    bad = true;
                    p = 1.0f;
                }
                p = sqrtf(p);
                if (c.slot == 0) s.row(F.Dg + j) = p;
                for (int i = j + 1 + c.slot; i < nd; i += c.nslot) {
                    float t = s.A(i, j);
                    for (int k = 0; k < j; ++k) t -= s.A(i, k) * s.A(j, k);
                    s.A(i, j) = t / p;
                }
            }
            __syncthreads();
        }
        // L y = -g, L^T delta = y (one lane: each sum in ascending order)
        if (c.valid && c.slot == 0) {
            for (int i = 0; i < nd; ++i) {
                float t = -s.row(F.g + i);
                for (int k = 0; k < i; ++k) t -= s.A(i, k) * s.row(F.X + k);
                s.row(F.X + i) = t / s.row(F.Dg + i);
            }
            for (int i = nd - 1; i >= 0; --i) {
                float t = s.row(F.X + i);
                for (int k = i + 1; k < nd; ++k) t -= s.A(k, i) * s.row(F.X + k);
                s.row(F.X + i) = t / s.row(F.Dg + i);
            }
        }
        __syncthreads();
        if (c.valid)
            for (int j = c.slot; j < m.nj; j += c.nslot) iks_retract_item(s, j, step);
        __syncthreads();
        iks_fk(s, max_depth, F.jq2, F.bq2);
        if (c.valid) iks_residuals(s, F.jq2, F.bq2, F.R2);
        __syncthreads();
        bool accept = false;
        float C2 = 0.0f;
        if (c.valid) {
            C2 = iks_cost(s, F.R2);
            float dd = 0.0f, gd = 0.0f;
            for (int i = 0; i < nd; ++i) {
                const float x = s.row(F.X + i);
                dd += x * x;
                gd += s.row(F.g + i) * x;
            }
            const float pred = 0.5f * step * (step * lam * dd - (2.0f - step) * gd);
            accept = !bad && pred > 0.0f && C2 < C && (C - C2) / pred > P.rho_min;
        }
        __syncthreads();  // (every lane has read delta, g and the candidate's residuals)
        if (accept) {
            for (int i = c.slot; i < m.nc; i += c.nslot) s.row(F.J.jq + i) = s.row(F.jq2 + i);
            for (int i = c.slot; i < 7 * m.nb; i += c.nslot) s.row(c.L.bq.off + i) = s.row(F.bq2 + i);
            for (int i = c.slot; i < F.nR; i += c.nslot) s.row(F.R + i) = s.row(F.R2 + i);
            C = C2;
            lam = fmaxw(lam / P.lambda_factor, P.lambda_min);
        } else {
            lam = fminw(lam * P.lambda_factor, P.lambda_max);
        }
        __syncthreads();
    }
    if (!c.valid) return;
    for (int i = c.slot; i < m.nc; i += c.nslot) joint_q_out[(size_t)c.env * m.nc + i] = s.row(F.J.jq + i);
    if (c.slot == 0) {
        lambda[c.env] = lam;
        cost[c.env] = C;
    }
}

}  // namespace ieee
}  // namespace

// ------------------------------------------------------------------------------------------------
// kin_launch: the tile rule and the launch of every kinematics entry point (nt_eval_fk, nt_eval_ik_tile, nt_eval_jacobian_tile,
// nt_eval_mass_matrix_tile, nt_eval_inverse_dynamics_tile, nt_eval_forward_dynamics_tile, nt_ik_solve_tile).  envs_per_block 0: on replicated worlds (nt_model.params_uniform, UNI_OK) the
// uniform-parameter tile of 16 -- ONE block-shared parameter copy, the parameters are four fifths of what the per-environment tile of
// eval_ik reads -- if it fits the LDS, otherwise the widest per-environment-parameter tile of 16 / 8 / 4 / 1 that fits.  A named width:
// that per-environment-parameter tile, if it is one of 1 / 4 / 8 / 16 and fits.  Nothing chosen: NT_ERR_UNSUPPORTED, nothing launched.
// An entry point brings what differs: rows(uni), the floats per environment of its layout; shared_ints, its block-shared tables;
// want, the slot-lanes of its widest phase (KArgs::nslot = min(want, 256 / epb)); launch(T, epb, lds_bytes), which returns
// launch_tile(kernel<T>, a, epb, lds_bytes, stream, ...) for T = std::integral_constant of E or of 16 + NT_UNI.  UNI_OK is a template
// argument: without it (nt_eval_fk) launch is never instantiated for 16 + NT_UNI, a kernel that entry point does not have.
// ------------------------------------------------------------------------------------------------
template <bool UNI_OK, typename Rows, typename Launch>
static nt_status kin_launch(const nt_model* m, KArgs& a, int32_t envs_per_block, size_t shared_ints, int want, Rows&& rows, Launch&& launch) {
    auto bytes = [&](int epb, bool uni) {
        return tile_bytes(rows(uni), epb, shared_ints, uni ? make_layout(*m, false, false, true, false).uni_floats : 0);
    };
    const bool uni = UNI_OK && envs_per_block == 0 && m->params_uniform && bytes(16, true) <= LDS_BYTES_PER_CU;
    int epb = 0;
    if (uni) {
        epb = 16;
    } else if (envs_per_block == 0) {
        const int cands[4] = {16, 8, 4, 1};
        for (int i = 0; i < 4 && !epb; ++i)
            if (bytes(cands[i], false) <= LDS_BYTES_PER_CU) epb = cands[i];
    } else if ((envs_per_block == 1 || envs_per_block == 4 || envs_per_block == 8 || envs_per_block == 16) &&
               bytes(envs_per_block, false) <= LDS_BYTES_PER_CU) {
        epb = envs_per_block;
    }
    if (!epb) return NT_ERR_UNSUPPORTED;
    const int cap = 256 / epb;
    a.nslot = want < cap ? want : cap;
    if constexpr (UNI_OK)
        if (uni) return launch(std::integral_constant<int, 16 + NT_UNI>{}, 16, bytes(16, true));
    return dispatch_epb(Epbs<16, 8, 4, 1>{}, epb, [&](auto E) { return launch(E, (int)E, bytes(E, false)); });
}

// nt_eval_jacobian_tile / nt_eval_mass_matrix_tile: argument checks and what they bring to kin_launch
template <bool MASS>
static nt_status jm_launch(const nt_model* m, const nt_state* in, float* out, float* aux, const uint8_t* art_mask, int32_t envs_per_block,
                           hipStream_t stream) {
    if (!model_ok(m) || !in || !in->body_q || !in->joint_q || !out) return NT_ERR_INVALID_ARG;
    if (m->nj <= 0 || m->na <= 0 || !m->art_start || m->max_art_dofs < 0) return NT_ERR_UNSUPPORTED;
#ifdef NT_DEV_FAST
    return NT_ERR_UNSUPPORTED;
#else
    if (m->max_art_dofs == 0) return NT_OK;  // (no dofs: J and H have no entries)
    KArgs a = {};
    a.m = *m;
    a.s_in = *in;
    // slot-lanes: one per dof / joint / body (mass matrix: per entry of a dof's H row block); the streaming phase runs workgroup-wide
    const int want = imax(imax(m->nb, m->nj), MASS ? m->nd * m->max_art_dofs : m->nd);
    return kin_launch<true>(
        m, a, envs_per_block, (size_t)topo_ints(*m) + jm_table_ints(*m), want, [&](bool uni) { return jm_layout(*m, uni, MASS).rows; },
        [&](auto T, int epb, size_t lds_bytes) {
            if constexpr (MASS) return launch_tile(eval_mass_matrix_kernel<T>, a, epb, lds_bytes, stream, out, aux, art_mask);
            else return launch_tile(eval_jacobian_kernel<T>, a, epb, lds_bytes, stream, out, aux, art_mask);
        });
#endif
}

// nt_eval_inverse_dynamics_tile: argument checks and what it brings to kin_launch
static nt_status id_launch(const nt_model* m, const nt_state* in, const float* joint_qdd, int32_t flags, float* tau, const uint8_t* art_mask,
                           int32_t envs_per_block, hipStream_t stream) {
    if (!model_ok(m) || !in || !in->body_q || !in->joint_q || !in->joint_qd || !tau) return NT_ERR_INVALID_ARG;
    if (flags & ~(NT_ID_GRAVITY | NT_ID_VELOCITY)) return NT_ERR_INVALID_ARG;
    if (m->nj <= 0 || m->na <= 0 || !m->art_start || m->max_art_dofs < 0) return NT_ERR_UNSUPPORTED;
#ifdef NT_DEV_FAST
    return NT_ERR_UNSUPPORTED;
#else
    if (m->max_art_dofs == 0) return NT_OK;  // (no dofs: tau has no entries)
    KArgs a = {};
    a.m = *m;
    a.s_in = *in;
    // slot-lanes: one per dof / joint / body; the gather of joint_qdd and the streaming phase run workgroup-wide
    return kin_launch<true>(
        m, a, envs_per_block, (size_t)topo_ints(*m) + jm_table_ints(*m), imax(imax(m->nb, m->nj), m->nd),
        [&](bool uni) { return id_layout(*m, uni).F.rows; },
        [&](auto T, int epb, size_t lds_bytes) {
            return launch_tile(eval_inverse_dynamics_kernel<T>, a, epb, lds_bytes, stream, joint_qdd, (int)flags, tau, art_mask);
        });
#endif
}

// nt_eval_forward_dynamics_tile: argument checks and what it brings to kin_launch
static nt_status fd_launch(const nt_model* m, const nt_state* in, const float* joint_f, int32_t flags, float* joint_qdd, int32_t* info,
                           const uint8_t* art_mask, int32_t envs_per_block, hipStream_t stream) {
    if (!model_ok(m) || !in || !in->body_q || !in->joint_q || !in->joint_qd || !joint_qdd) return NT_ERR_INVALID_ARG;
    if (flags & ~(NT_FD_GRAVITY | NT_FD_VELOCITY | NT_FD_BODY_F)) return NT_ERR_INVALID_ARG;
    if ((flags & NT_FD_BODY_F) && !in->body_f) return NT_ERR_INVALID_ARG;
    if (m->nj <= 0 || m->na <= 0 || !m->art_start || m->max_art_dofs < 0) return NT_ERR_UNSUPPORTED;
#ifdef NT_DEV_FAST
    return NT_ERR_UNSUPPORTED;
#else
    if (m->max_art_dofs == 0) return NT_OK;  // (no dofs: joint_qdd has no entries)
    KArgs a = {};
    a.m = *m;
    a.s_in = *in;
    // slot-lanes: one per dof / joint / body, per entry of a dof's H row block; the gather of joint_f and the streaming phase run
    // workgroup-wide
    return kin_launch<true>(
        m, a, envs_per_block, (size_t)topo_ints(*m) + jm_table_ints(*m), imax(imax(m->nb, m->nj), m->nd * m->max_art_dofs),
        [&](bool uni) { return fd_layout(*m, uni, (flags & NT_FD_BODY_F) != 0).I.F.rows; },
        [&](auto T, int epb, size_t lds_bytes) {
            return launch_tile(eval_forward_dynamics_kernel<T>, a, epb, lds_bytes, stream, joint_f, (int)flags, joint_qdd, (int*)info, art_mask);
        });
#endif
}

extern "C" {

// shared launch logic of the Featherstone kernels (step / rollout)
static nt_status fs_launch(const nt_model* m, KArgs& a, int32_t envs_per_block, bool rollout, hipStream_t stream) {
    if (m->contact_scratch_in_hbm) return NT_ERR_UNSUPPORTED;  // XPBD / collide only
#ifdef NT_DEV_FAST
    return NT_ERR_UNSUPPORTED;
#else
    const bool tree = fs_tree_mode(a);  // (a.fp is set by the caller: the layout of the launch follows the mass-matrix mode)
    FsLayout F = make_fs_layout(*m, make_layout(*m, false, false, false, false), tree);
    const size_t shared_ints = (size_t)topo_ints(*m) + fs_topo_ints(*m);
    auto fits = [&](int epb) { return tile_bytes(F.rows, epb, shared_ints) <= LDS_BYTES_PER_CU; };
    const bool cvx = m->np_analytic < m->np;
    // Uniform-parameter tile of 16 (round 6): the level-synchronous phases of this solver keep a handful of lanes per environment busy
    // and wait on LDS round trips and barriers, so what a CU delivers is the number of environments it holds.  With ONE block-shared
    // parameter copy and the tree-structured solve region (make_fs_layout) an Anymal-class environment needs 9.3 KB instead of 17 KB:
    // 16 per CU in one 512-lane workgroup -- 4 096 environments in ONE round of 256 workgroups instead of two rounds of 1 024 x 4.
    const LdsLayout Lu = make_layout(*m, false, false, true, false);
    const FsLayout Fu = make_fs_layout(*m, Lu, tree);
    // (automatic from 2 049 environments: up to 2 048 the tiles of 4 are ONE round of 512 workgroups already and keep all 64 lanes per
    // environment -- 37.6 vs 32.6 M env-steps/s, profiles/r06H_ab_workloads.txt; envs_per_block = 16 asks for it at any size)
    const bool uni16 = rollout && !cvx && m->params_uniform && (envs_per_block == 16 || (envs_per_block == 0 && m->env_count > 2048)) &&
                       tile_bytes(Fu.rows, 16, shared_ints, Lu.uni_floats) <= LDS_BYTES_PER_CU;
    int epb = 0;
    if (uni16) {
        epb = 16;
    } else if (envs_per_block == 1 || envs_per_block == 4 || envs_per_block == 8 || envs_per_block == 16) {
        epb = fits(envs_per_block) ? envs_per_block : 0;
    } else {
        // measured on MI355X (4096 quadrupeds): 4 envs per workgroup (16 cooperating lanes per env in the Cholesky wave,
        // two resident workgroups per CU) beats 8; 16 rarely fits; articulations too large for 4 (P + H alone are
        // (6 nj + nd) x max_art_dofs floats per environment) run one environment per workgroup, 64 lanes in the Cholesky wave
        const int cands[4] = {4, 8, 16, 1};
        for (int i = 0; i < 4 && !epb; ++i)
            if (fits(cands[i])) epb = cands[i];
    }
    if (!epb) return NT_ERR_UNSUPPORTED;
    if (rollout && cvx && epb == 16) epb = 8;  // the convex rollout is only instantiated for 4 / 8 envs per workgroup
    int want = imax(imax(m->nb, m->nj), imax(m->np * m->cpp, imax(m->nj, m->nd) * m->max_art_dofs));
    const int max_threads = uni16 ? 512 : 256;
    int cap = max_threads / epb;
    a.nslot = want < cap ? want : cap;
    const size_t lds_bytes = uni16 ? tile_bytes(Fu.rows, 16, shared_ints, Lu.uni_floats) : tile_bytes(F.rows, epb, shared_ints);
    if (uni16) return launch_tile(featherstone_rollout_kernel<16 + NT_UNI, false, 512>, a, 16, lds_bytes, stream);
    if (!rollout)
        return dispatch_epb(Epbs<16, 8, 4, 1>{}, epb, [&](auto E) { return launch_tile(featherstone_step_kernel<E>, a, E, lds_bytes, stream); });
    if (cvx)
        return dispatch_epb(Epbs<8, 4, 1>{}, epb,
                            [&](auto E) { return launch_tile(featherstone_rollout_kernel<E, true>, a, E, lds_bytes, stream); });
    return dispatch_epb(Epbs<16, 8, 4, 1>{}, epb,
                        [&](auto E) { return launch_tile(featherstone_rollout_kernel<E, false>, a, E, lds_bytes, stream); });
#endif
}

static bool fs_state_ok(const nt_state* s) { return s && s->joint_q && s->joint_qd && s->body_q && s->body_qd; }

// what nt_featherstone_step and nt_featherstone_rollout fill alike (contacts, has_contacts and substeps: the callers')
static KArgs fs_args(const nt_model* m, const nt_featherstone_params* p, const nt_state* s_in, const nt_state* s_out, const nt_control* ctrl,
                     float dt) {
    KArgs a = {};
    a.m = *m;
    a.s_in = *s_in;
    a.s_out = *s_out;
    a.c = *ctrl;
    a.sp.friction_smoothing = p->friction_smoothing;
    a.fp = *p;
    a.angular_damping = p->angular_damping;
    a.dt = dt;
    return a;
}

nt_status nt_featherstone_step(const nt_model* m, const nt_featherstone_params* p, nt_state* s_in, nt_state* s_out,
                                const nt_control* ctrl, const nt_contacts* c, float dt, int32_t envs_per_block, void* stream) {
    if (!model_ok(m) || !p || !ctrl || !fs_state_ok(s_in) || !fs_state_ok(s_out)) return NT_ERR_INVALID_ARG;
    if (m->nj <= 0 || m->na <= 0 || m->max_art_dofs < 0 || !m->art_start) return NT_ERR_UNSUPPORTED;
    KArgs a = fs_args(m, p, s_in, s_out, ctrl, dt);
    if (c) a.ct = *c;
    a.has_contacts = (c != nullptr && m->np > 0) ? 1 : 0;
    return fs_launch(m, a, envs_per_block, false, (hipStream_t)stream);
}

nt_status nt_featherstone_rollout(const nt_model* m, const nt_featherstone_params* p, const nt_collide_params* cp, nt_state* s0,
                                   nt_state* s1, const nt_control* ctrl, nt_contacts* c, float dt, int32_t substeps,
                                   void* stream) {
    if (!model_ok(m) || !p || !ctrl || !c || !fs_state_ok(s0) || !fs_state_ok(s1) || !s0->body_f || !s1->body_f || substeps <= 0)
        return NT_ERR_INVALID_ARG;
    if (m->nj <= 0 || m->na <= 0 || m->max_art_dofs < 0 || !m->art_start) return NT_ERR_UNSUPPORTED;
    KArgs a = fs_args(m, p, s0, s1, ctrl, dt);
    a.ct = *c;
    a.has_contacts = m->np > 0 ? 1 : 0;
    a.substeps = substeps;
    return fs_launch(m, a, cp ? cp->envs_per_block : 0, true, (hipStream_t)stream);
}

int32_t nt_featherstone_lds_bytes_per_env(const nt_model* m) {
    if (!m) return -1;
    return make_fs_layout(*m, make_layout(*m, false, false, false, false)).rows * 4;  // (dense mass-matrix region, per-environment parameters: the largest form)
}

// the widest per-environment-parameter tile that fits (kin_launch without the uniform tile, no named width)
nt_status nt_eval_fk(const nt_model* m, const float* joint_q, const float* joint_qd, nt_state* out, void* stream) {
    if (!model_ok(m) || !joint_q || !joint_qd || !out || !out->body_q || !out->body_qd) return NT_ERR_INVALID_ARG;
    if (m->nj <= 0) return NT_ERR_UNSUPPORTED;
#ifdef NT_DEV_FAST
    return NT_ERR_UNSUPPORTED;
#else
    KArgs a = {};
    a.m = *m;
    a.s_out = *out;
    const FsLayout F = make_fs_layout(*m, make_layout(*m, false, false, false, false), fs_tree_mode(a));  // (the kernel's own rule)
    return kin_launch<false>(
        m, a, 0, (size_t)topo_ints(*m) + fs_topo_ints(*m), imax(m->nb, m->nj), [&](bool) { return F.rows; },
        [&](auto T, int epb, size_t lds_bytes) {
            return launch_tile(eval_fk_kernel<T>, a, epb, lds_bytes, (hipStream_t)stream, joint_q, joint_qd);
        });
#endif
}

// envs_per_block: the tile, by kin_launch's rule (0: the widest that fits; 1 / 4 / 8 / 16: that per-environment-parameter tile)
nt_status nt_eval_ik_tile(const nt_model* m, const nt_state* in, float* joint_q, float* joint_qd, const uint8_t* art_mask,
                          int32_t envs_per_block, void* stream) {
    if (!model_ok(m) || !in || !in->body_q || !in->body_qd || !joint_q || !joint_qd) return NT_ERR_INVALID_ARG;
    if (m->nj <= 0) return NT_ERR_UNSUPPORTED;
#ifdef NT_DEV_FAST
    return NT_ERR_UNSUPPORTED;
#else
    KArgs a = {};
    a.m = *m;
    a.s_in = *in;
    return kin_launch<true>(
        m, a, envs_per_block, (size_t)topo_ints(*m), imax(m->nb, m->nj), [&](bool uni) { return ik_rows(*m, uni); },
        [&](auto T, int epb, size_t lds_bytes) {
            return launch_tile(eval_ik_kernel<T>, a, epb, lds_bytes, (hipStream_t)stream, joint_q, joint_qd, art_mask);
        });
#endif
}

nt_status nt_eval_ik(const nt_model* m, const nt_state* in, float* joint_q, float* joint_qd, const uint8_t* art_mask, void* stream) {
    return nt_eval_ik_tile(m, in, joint_q, joint_qd, art_mask, 0, stream);
}

nt_status nt_frame_sensor(const nt_model* m, const nt_state* s, const nt_state* prev, float dt, const nt_frame_sensor_args* a, void* stream) {
    if (!model_ok(m) || !s || !a || !s->body_q) return NT_ERR_INVALID_ARG;
    if (a->frame_count <= 0 || a->out_count <= 0 || !a->frame_body || !a->frame_xform || !a->out_frame || !a->out_ref ||
        !a->frame_body_host || !a->frame_xform_host || !a->out_frame_host || !a->out_ref_host)
        return NT_ERR_INVALID_ARG;
    if (!a->transform && !a->velocity && !a->gravity_dir && !a->accel) return NT_ERR_INVALID_ARG;
    if ((a->velocity || a->accel) && (!s->body_qd || !m->body_param)) return NT_ERR_INVALID_ARG;
    if ((a->gravity_dir || a->accel) && !m->gravity) return NT_ERR_INVALID_ARG;
    if (a->accel && (!prev || !prev->body_qd || !(dt > 0.0f) || !(dt <= 3.0e38f))) return NT_ERR_INVALID_ARG;
    const int M = a->frame_count, N = a->out_count;
    for (int f = 0; f < M; ++f) {
        if (a->frame_body_host[f] < -1 || a->frame_body_host[f] >= m->nb) return NT_ERR_INVALID_ARG;
        const float* X = a->frame_xform_host + 7 * (size_t)f;
        double qq = 0.0;
        for (int k = 0; k < 7; ++k) {
            if (!(X[k] >= -3.0e38f && X[k] <= 3.0e38f)) return NT_ERR_INVALID_ARG;  // (NaN fails both comparisons)
            if (k >= 3) qq += (double)X[k] * (double)X[k];
        }
        const double norm_err = sqrt(qq) - 1.0;
        if (!(norm_err >= -1.0e-4 && norm_err <= 1.0e-4)) return NT_ERR_INVALID_ARG;
    }
    for (int n = 0; n < N; ++n)
        if (a->out_frame_host[n] < 0 || a->out_frame_host[n] >= M || a->out_ref_host[n] < -1 || a->out_ref_host[n] >= M)
            return NT_ERR_INVALID_ARG;
    // one wave per (row, 64 worlds); the item index stays an int
    const long long chunks = ((long long)m->env_count + FR_THREADS - 1) / FR_THREADS, items = chunks * N;
    if (items > 0x7fffffffLL) return NT_ERR_INVALID_ARG;
#ifdef NT_EMULATED_GRID
    const long long grid_cap = NT_EMULATED_GRID;
#else
    const long long grid_cap = FR_MAX_GRID;
#endif
    hipLaunchKernelGGL(frame_sensor_kernel, dim3((unsigned)(items < grid_cap ? items : grid_cap)), dim3(FR_THREADS), 0, (hipStream_t)stream,
                       *m, (const float*)s->body_q, (const float*)s->body_qd, a->accel ? (const float*)prev->body_qd : (const float*)nullptr,
                       dt, *a);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

// envs_per_block: the tile, by kin_launch's rule (jm_launch)
nt_status nt_eval_jacobian_tile(const nt_model* m, const nt_state* in, float* J, float* joint_S_s, const uint8_t* art_mask,
                                int32_t envs_per_block, void* stream) {
    return jm_launch<false>(m, in, J, joint_S_s, art_mask, envs_per_block, (hipStream_t)stream);
}

nt_status nt_eval_jacobian(const nt_model* m, const nt_state* in, float* J, float* joint_S_s, const uint8_t* art_mask, void* stream) {
    return nt_eval_jacobian_tile(m, in, J, joint_S_s, art_mask, 0, stream);
}

// envs_per_block: the tile, by kin_launch's rule (jm_launch)
nt_status nt_eval_mass_matrix_tile(const nt_model* m, const nt_state* in, float* H, float* body_I_s, const uint8_t* art_mask,
                                   int32_t envs_per_block, void* stream) {
    return jm_launch<true>(m, in, H, body_I_s, art_mask, envs_per_block, (hipStream_t)stream);
}

nt_status nt_eval_mass_matrix(const nt_model* m, const nt_state* in, float* H, float* body_I_s, const uint8_t* art_mask, void* stream) {
    return nt_eval_mass_matrix_tile(m, in, H, body_I_s, art_mask, 0, stream);
}

// envs_per_block: the tile, by kin_launch's rule (id_launch)
nt_status nt_eval_inverse_dynamics_tile(const nt_model* m, const nt_state* in, const float* joint_qdd, int32_t flags, float* tau,
                                        const uint8_t* art_mask, int32_t envs_per_block, void* stream) {
    return id_launch(m, in, joint_qdd, flags, tau, art_mask, envs_per_block, (hipStream_t)stream);
}

nt_status nt_eval_inverse_dynamics(const nt_model* m, const nt_state* in, const float* joint_qdd, int32_t flags, float* tau,
                                   const uint8_t* art_mask, void* stream) {
    return nt_eval_inverse_dynamics_tile(m, in, joint_qdd, flags, tau, art_mask, 0, stream);
}

// envs_per_block: the tile, by kin_launch's rule (fd_launch)
nt_status nt_eval_forward_dynamics_tile(const nt_model* m, const nt_state* in, const float* joint_f, int32_t flags, float* joint_qdd,
                                        int32_t* info, const uint8_t* art_mask, int32_t envs_per_block, void* stream) {
    return fd_launch(m, in, joint_f, flags, joint_qdd, info, art_mask, envs_per_block, (hipStream_t)stream);
}

nt_status nt_eval_forward_dynamics(const nt_model* m, const nt_state* in, const float* joint_f, int32_t flags, float* joint_qdd,
                                   int32_t* info, const uint8_t* art_mask, void* stream) {
    return nt_eval_forward_dynamics_tile(m, in, joint_f, flags, joint_qdd, info, art_mask, 0, stream);
}

// envs_per_block: the tile, by kin_launch's rule
nt_status nt_ik_solve_tile(const nt_model* m, const nt_ik_problem* p, const float* joint_q_in, float* joint_q_out, float* lambda, float* cost,
                           int32_t iterations, float step_size, int32_t envs_per_block, void* stream) {
    if (!model_ok(m) || !p || !joint_q_in || !joint_q_out || !lambda || !cost || iterations < 0 || p->count < 0) return NT_ERR_INVALID_ARG;
    if (m->nj <= 0 || m->na <= 0 || m->nd <= 0 || !m->art_start || p->count > NT_IK_MAX_OBJECTIVES) return NT_ERR_UNSUPPORTED;
    for (int k = 0; k < p->count; ++k) {
        const nt_ik_objective& o = p->obj[k];
        if (!o.target) return NT_ERR_INVALID_ARG;
        if (o.type != NT_IK_POSITION && o.type != NT_IK_ROTATION && o.type != NT_IK_JOINT_LIMIT) return NT_ERR_UNSUPPORTED;
        if (o.type != NT_IK_JOINT_LIMIT && (o.link < 0 || o.link >= m->nb)) return NT_ERR_UNSUPPORTED;
    }
#ifdef NT_DEV_FAST
    return NT_ERR_UNSUPPORTED;
#else
    KArgs a = {};
    a.m = *m;
    // slot-lanes: one per entry of the normal equations (the widest phase)
    const int want = imax(imax(m->nb, m->nj), m->nd * (m->nd + 1) / 2 + m->nd);
    return kin_launch<true>(
        m, a, envs_per_block, (size_t)topo_ints(*m) + iks_table_ints(*m), want, [&](bool uni) { return iks_layout(*m, *p, uni).rows; },
        [&](auto T, int epb, size_t lds_bytes) {
            return launch_tile(ik_solve_kernel<T>, a, epb, lds_bytes, (hipStream_t)stream, *p, joint_q_in, joint_q_out, lambda, cost,
                               (int)iterations, step_size);
        });
#endif
}

nt_status nt_ik_solve(const nt_model* m, const nt_ik_problem* p, const float* joint_q_in, float* joint_q_out, float* lambda, float* cost,
                      int32_t iterations, float step_size, void* stream) {
    return nt_ik_solve_tile(m, p, joint_q_in, joint_q_out, lambda, cost, iterations, step_size, 0, stream);
}

#ifdef NT_PHASE_TIMING
// debug build only: read and reset this unit's phase cycle counters (the counters are per translation unit)
int nt_debug_phase_clocks_fs(unsigned long long* out) {
    unsigned long long zero[32] = {};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nt_phase_clock), sizeof(zero)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(nt_phase_clock), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
