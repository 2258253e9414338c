// nt_match.hip -- frame-to-frame contact matching (newton/_src/geometry/contact_match.py:266-391,442-480) on the fixed-slot
// contact layout.
//
// The reference sorts the flat contact list by (shape0, shape1, sub-key), binary-searches the previous frame's sorted keys for
// the pair's range and lets the new contacts of a pair race for their closest previous contact with a packed atomic_min.  Here
// a pair's contacts of one environment always live in the same `cpp` slots, so the pair range IS the slot group: one lane per
// (env, slot) scans the <= 5 saved midpoints of its own pair, and the race is resolved without atomics -- every lane re-derives
// the claims of its (<= 4) siblings and the winner is the reference's: smallest distance, ties by the smaller sub-contact index
// (the low bits of the sort key, contact_data.py:60-90).  Results per slot: index of the matched previous SLOT, -1 (pair had no
// contacts last frame), -2 (no candidate within the thresholds, or lost the race).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/newton_hip.h"
#ifndef NT_EMULATED_GRID
#include "../../include/newton_hip_contacts.h"
#else  // (the CPU emulator compiles a copy of this file from tests/emu/_build)
#include "../../../include/newton_hip_contacts.h"
#endif
#include "nt_math.hpp"

using namespace nt;

namespace {

constexpr int MATCH_NOT_FOUND = -1, MATCH_BROKEN = -2;

struct MatchArgs {
    nt_model m;
    nt_state s;
    nt_contacts c;
    nt_contact_history h;
    float pos_threshold_sq, normal_dot_threshold;
    const uint8_t* reset_world_mask;
    int32_t* match_index;
};

__device__ inline vec3 ld3(const float* base, int comp0, int n, int slot, int ES, int env) {
    return vec3(base[((size_t)(comp0 + 0) * n + slot) * ES + env], base[((size_t)(comp0 + 1) * n + slot) * ES + env],
                base[((size_t)(comp0 + 2) * n + slot) * ES + env]);
}
__device__ inline xform body_xform(const nt_state& s, int nb, int b, int ES, int env) {
    const float* q = s.body_q;
    auto g = [&](int comp) { return q[((size_t)comp * nb + b) * ES + env]; };
    return xform(vec3(g(0), g(1), g(2)), quat(g(3), g(4), g(5), g(6)));
}
// world-space midpoint of the two contact points of a slot (the quantity the reference persists and compares)
__device__ inline vec3 midpoint(const MatchArgs& a, int slot, int env, int p) {
    const int ES = a.m.env_stride, ncs = a.m.np * a.m.cpp;
    int sa = a.m.pair_a[p], sb = a.m.pair_b[p];
    if (a.m.shape_type[sa] > a.m.shape_type[sb]) { int t = sa; sa = sb; sb = t; }  // contacts are written type-sorted
    const int ba = a.m.shape_body[sa], bb = a.m.shape_body[sb];
    vec3 p0 = ld3(a.c.data, 0, ncs, slot, ES, env), p1 = ld3(a.c.data, 3, ncs, slot, ES, env);
    if (ba >= 0) p0 = xform_point(body_xform(a.s, a.m.nb, ba, ES, env), p0);
    if (bb >= 0) p1 = xform_point(body_xform(a.s, a.m.nb, bb, ES, env), p1);
    return 0.5f * (p0 + p1);
}

// best previous slot of new contact (p, k): closest saved midpoint within the position threshold whose normal agrees
__device__ inline int best_candidate(const MatchArgs& a, int p, int k, int env, float& best_dist_sq, bool& any_prev) {
    const int ES = a.m.env_stride, cpp = a.m.cpp, ncs = a.m.np * cpp;
    const int slot = p * cpp + k;
    const vec3 pos = midpoint(a, slot, env, p);
    const vec3 n = ld3(a.c.data, 12, ncs, slot, ES, env);
    int best = -1;
    best_dist_sq = a.pos_threshold_sq;
    any_prev = false;
    for (int j = 0; j < cpp; ++j) {
        const int ps = p * cpp + j;
        if (!a.h.prev_live[(size_t)ps * ES + env]) continue;
        any_prev = true;
        const vec3 d = pos - ld3(a.h.prev_pos_world, 0, ncs, ps, ES, env);
        const float dist_sq = dot(d, d);
        if (dist_sq <= best_dist_sq) {
            if (dot(n, ld3(a.h.prev_normal, 0, ncs, ps, ES, env)) >= a.normal_dot_threshold) {
                best_dist_sq = dist_sq;
                best = ps;
            }
        }
    }
    return best;
}

__global__ void __launch_bounds__(256) contacts_match_kernel(MatchArgs a) {
    const int ES = a.m.env_stride, cpp = a.m.cpp, ncs = a.m.np * cpp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ncs * ES) return;
    const int env = (int)(i % ES), slot = (int)(i / ES);
    if (env >= a.m.env_count) return;
    const size_t gi = (size_t)slot * ES + env;
    if (a.c.shape0[gi] < 0 || a.c.shape0[gi] == a.c.shape1[gi]) {  // dead slot: not a contact of this frame
        a.match_index[gi] = MATCH_NOT_FOUND;
        return;
    }
    if (a.reset_world_mask && a.reset_world_mask[env]) {  // contacts of a world that was just reset never match
        a.match_index[gi] = MATCH_NOT_FOUND;
        return;
    }
    const int p = slot / cpp, k = slot - p * cpp;
    float my_dist;
    bool any_prev;
    const int cand = best_candidate(a, p, k, env, my_dist, any_prev);
    if (!any_prev) { a.match_index[gi] = MATCH_NOT_FOUND; return; }
    if (cand < 0) { a.match_index[gi] = MATCH_BROKEN; return; }
    // the race for prev[cand]: a sibling wins with a smaller distance, or the same distance and a smaller sub-contact index
    bool lost = false;
    for (int k2 = 0; k2 < cpp && !lost; ++k2) {
        if (k2 == k) continue;
        const size_t g2 = (size_t)(p * cpp + k2) * ES + env;
        if (a.c.shape0[g2] < 0 || a.c.shape0[g2] == a.c.shape1[g2]) continue;
        float d2;
        bool ap;
        if (best_candidate(a, p, k2, env, d2, ap) != cand) continue;
        if (d2 < my_dist || (d2 == my_dist && k2 < k)) lost = true;
    }
    a.match_index[gi] = lost ? MATCH_BROKEN : cand;
}

// _save_sorted_state_kernel: persist this frame's midpoints, normals and live flags for the next match
__global__ void __launch_bounds__(256) contacts_save_kernel(MatchArgs a) {
    const int ES = a.m.env_stride, cpp = a.m.cpp, ncs = a.m.np * cpp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ncs * ES) return;
    const int env = (int)(i % ES), slot = (int)(i / ES);
    const size_t gi = (size_t)slot * ES + env;
    const bool live = env < a.m.env_count && a.c.shape0[gi] >= 0 && a.c.shape0[gi] != a.c.shape1[gi];
    a.h.prev_live[gi] = live ? 1 : 0;
    if (!live) return;
    const vec3 pos = midpoint(a, slot, env, slot / cpp);
    const vec3 n = ld3(a.c.data, 12, ncs, slot, ES, env);
    if (a.h.prev_body_frame) {  // sticky mode: the body-frame points and offsets of the record actually used this frame
        float* B = a.h.prev_body_frame;
        for (int comp = 0; comp < 12; ++comp) B[((size_t)comp * ncs + slot) * ES + env] = a.c.data[((size_t)comp * ncs + slot) * ES + env];
    }
    float* P = a.h.prev_pos_world;
    float* N = a.h.prev_normal;
    P[((size_t)0 * ncs + slot) * ES + env] = pos.x; P[((size_t)1 * ncs + slot) * ES + env] = pos.y; P[((size_t)2 * ncs + slot) * ES + env] = pos.z;
    N[((size_t)0 * ncs + slot) * ES + env] = n.x; N[((size_t)1 * ncs + slot) * ES + env] = n.y; N[((size_t)2 * ncs + slot) * ES + env] = n.z;
}

// _replay_matched_kernel (contact_match.py:530-562): a matched contact that still touches (fresh gap <= 0) keeps last
// frame's body-frame points / offsets and normal; everything else of the row is key-derived or a per-shape constant
__global__ void __launch_bounds__(256) contacts_replay_kernel(MatchArgs a) {
    const int ES = a.m.env_stride, cpp = a.m.cpp, ncs = a.m.np * cpp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ncs * ES) return;
    const int env = (int)(i % ES), slot = (int)(i / ES);
    if (env >= a.m.env_count) return;
    const size_t gi = (size_t)slot * ES + env;
    if (a.c.shape0[gi] < 0 || a.c.shape0[gi] == a.c.shape1[gi]) return;
    const int idx = a.match_index[gi];
    if (idx < 0) return;  // MATCH_NOT_FOUND or MATCH_BROKEN: keep the new frame's data
    const int p = slot / cpp;
    int sa = a.m.pair_a[p], sb = a.m.pair_b[p];
    if (a.m.shape_type[sa] > a.m.shape_type[sb]) { int t = sa; sa = sb; sb = t; }
    const int ba = a.m.shape_body[sa], bb = a.m.shape_body[sb];
    float* D = a.c.data;
    vec3 p0 = ld3(D, 0, ncs, slot, ES, env), p1 = ld3(D, 3, ncs, slot, ES, env);
    if (ba >= 0) p0 = xform_point(body_xform(a.s, a.m.nb, ba, ES, env), p0);
    if (bb >= 0) p1 = xform_point(body_xform(a.s, a.m.nb, bb, ES, env), p1);
    const vec3 n = ld3(D, 12, ncs, slot, ES, env);
    const float margins = D[((size_t)15 * ncs + slot) * ES + env] + D[((size_t)16 * ncs + slot) * ES + env];
    const float fresh_gap = dot(p1 - p0, n) - margins;
    if (fresh_gap > 0.0f) return;
    const float* B = a.h.prev_body_frame;
    for (int comp = 0; comp < 12; ++comp) D[((size_t)comp * ncs + slot) * ES + env] = B[((size_t)comp * ncs + idx) * ES + env];
    for (int comp = 0; comp < 3; ++comp) D[((size_t)(12 + comp) * ncs + slot) * ES + env] = a.h.prev_normal[((size_t)comp * ncs + idx) * ES + env];
}

bool args_ok(const nt_model* m, const nt_state* s, const nt_contacts* c, const nt_contact_history* h) {
    return m && s && c && h && m->env_count > 0 && m->np > 0 && s->body_q && c->shape0 && c->shape1 && c->data && h->prev_pos_world &&
           h->prev_normal && h->prev_live;
}

}  // namespace

extern "C" {

nt_status nt_contacts_match(const nt_model* m, const nt_state* s, const nt_contacts* c, const nt_contact_history* h,
                            float pos_threshold, float normal_dot_threshold, const uint8_t* reset_world_mask, int32_t* match_index,
                            void* stream) {
    if (!args_ok(m, s, c, h) || !match_index || !(pos_threshold >= 0.0f)) return NT_ERR_INVALID_ARG;
    MatchArgs a = {*m, *s, *c, *h, pos_threshold * pos_threshold, normal_dot_threshold, reset_world_mask, match_index};
    const size_t n = (size_t)m->np * m->cpp * m->env_stride;
    hipLaunchKernelGGL(contacts_match_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

nt_status nt_contacts_replay_matched(const nt_model* m, const nt_state* s, nt_contacts* c, const nt_contact_history* h,
                                     const int32_t* match_index, void* stream) {
    if (!args_ok(m, s, c, h) || !match_index || !h->prev_body_frame) return NT_ERR_INVALID_ARG;
    MatchArgs a = {*m, *s, *c, *h, 0.0f, 0.0f, nullptr, const_cast<int32_t*>(match_index)};
    const size_t n = (size_t)m->np * m->cpp * m->env_stride;
    hipLaunchKernelGGL(contacts_replay_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

nt_status nt_contacts_save_history(const nt_model* m, const nt_state* s, const nt_contacts* c, nt_contact_history* h, void* stream) {
    if (!args_ok(m, s, c, h)) return NT_ERR_INVALID_ARG;
    MatchArgs a = {*m, *s, *c, *h, 0.0f, 0.0f, nullptr, nullptr};
    const size_t n = (size_t)m->np * m->cpp * m->env_stride;
    hipLaunchKernelGGL(contacts_save_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

}  // extern "C"

// ---- key-ordered export and matching report (include/newton_hip_contacts.h) -----------------------------------------------------
// The order is a counting sort over buckets whose key rank is fixed at pipeline construction: per export the live contacts of
// every bucket are counted (tile buckets: one lane per (pair, env) over its <= 5 slots; row buckets: one wave per world walking
// its rows in order, the per-bucket fill in LDS), the counts are scanned in rank order (three-kernel multi-block scan, integer
// sums: the same result whatever the schedule), and every live slot / row is written to bucket_start[rank] + its position inside
// the bucket.  Streaming, one lane per slot / row / output entry, no atomics on the data path.
namespace {

// components of nt_contacts.data (nt_layout.hpp CD_*)
constexpr int CD_POINT0 = 0, CD_POINT1 = 3, CD_OFFSET0 = 6, CD_OFFSET1 = 9, CD_NORMAL = 12, CD_MARGIN0 = 15, CD_MARGIN1 = 16;
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;

unsigned grid_for(size_t n, unsigned threads) {
    size_t b = (n + threads - 1) / threads;
#ifdef NT_EMULATED_GRID
    if (b > NT_EMULATED_GRID) b = NT_EMULATED_GRID;
#else
    if (b > 16384) b = 16384;  // (grid-stride loops cover the rest)
#endif
    return b < 1 ? 1u : (unsigned)b;
}
__host__ __device__ inline int scan_chunks(int n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK; }

// exclusive scan of in[0, n) into out, chunk totals through block_sum ([chunks + 1]); *total (nullable) = the sum
__global__ void __launch_bounds__(SCAN_THREADS) scan_partial_kernel(const int32_t* in, int n, int32_t* block_sum) {
    __shared__ int32_t part[SCAN_THREADS];
    const int chunks = scan_chunks(n), t = threadIdx.x;
    for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        int s = 0;
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            const int i = ch * SCAN_CHUNK + t * SCAN_ITEMS + k;
            if (i < n) s += in[i];
        }
        part[t] = s;
        __syncthreads();
        for (int w = SCAN_THREADS / 2; w > 0; w >>= 1) {
            if (t < w) part[t] += part[t + w];
            __syncthreads();
        }
        if (t == 0) block_sum[ch] = part[0];
        __syncthreads();
    }
}
__global__ void __launch_bounds__(SCAN_THREADS) scan_top_kernel(int32_t* block_sum, int chunks, int32_t* total) {
    __shared__ int32_t part[SCAN_THREADS];
    const int t = threadIdx.x, per = (chunks + SCAN_THREADS - 1) / SCAN_THREADS;
    const int beg = t * per, end = beg + per < chunks ? beg + per : chunks;
    int s = 0;
    for (int i = beg; i < end; ++i) s += block_sum[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int i = 0; i < SCAN_THREADS; ++i) { const int v = part[i]; part[i] = acc; acc += v; }
        block_sum[chunks] = acc;
        if (total) total[0] = acc;
    }
    __syncthreads();
    int acc = part[t];
    for (int i = beg; i < end; ++i) { const int v = block_sum[i]; block_sum[i] = acc; acc += v; }
}
__global__ void __launch_bounds__(SCAN_THREADS) scan_apply_kernel(const int32_t* in, int n, const int32_t* block_sum, int32_t* out) {
    __shared__ int32_t part[SCAN_THREADS];
    const int chunks = scan_chunks(n), t = threadIdx.x;
    for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        int v[SCAN_ITEMS], s = 0;
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            const int i = ch * SCAN_CHUNK + t * SCAN_ITEMS + k;
            v[k] = i < n ? in[i] : 0;
            s += v[k];
        }
        part[t] = s;
        __syncthreads();
        if (t == 0) {
            int acc = block_sum[ch];
            for (int i = 0; i < SCAN_THREADS; ++i) { const int x = part[i]; part[i] = acc; acc += x; }
        }
        __syncthreads();
        int acc = part[t];
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            const int i = ch * SCAN_CHUNK + t * SCAN_ITEMS + k;
            if (i < n) out[i] = acc;
            acc += v[k];
        }
        __syncthreads();
    }
}
void launch_scan(const int32_t* in, int n, int32_t* block_sum, int32_t* out, int32_t* total, hipStream_t st) {
    const int chunks = scan_chunks(n);
    const unsigned g = grid_for((size_t)chunks, 1);
    hipLaunchKernelGGL(scan_partial_kernel, dim3(g), dim3(SCAN_THREADS), 0, st, in, n, block_sum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, block_sum, chunks, total);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(g), dim3(SCAN_THREADS), 0, st, in, n, block_sum, out);
}

// live slot contacts of every tile bucket (pair p, env e, orientation o)
__global__ void __launch_bounds__(256) order_tile_count_kernel(nt_model m, nt_contacts c, nt_contact_order o) {
    const int E = m.env_count, ES = m.env_stride, cpp = m.cpp;
    const size_t n = (size_t)m.np * E;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(i / E), env = (int)(i % E);
        const int want0 = o.tile_shape0[i];
        int cnt[2] = {0, 0};
        for (int k = 0; k < cpp; ++k) {
            const int s0 = c.shape0[(size_t)(p * cpp + k) * ES + env];
            if (s0 < 0) continue;
            cnt[s0 == want0 ? 0 : 1] += 1;
        }
        o.bucket_fill[o.tile_rank[2 * i]] = cnt[0];
        o.bucket_fill[o.tile_rank[2 * i + 1]] = cnt[1];
    }
}

// the rows of one world, 64 at a time in row order: bucket by binary search of the row's key in the world's table, position inside
// the bucket = the bucket's fill so far + the lanes of this round before it with the same bucket
constexpr int ROW_WAVE = 64;
__global__ void __launch_bounds__(ROW_WAVE) order_row_bucket_kernel(nt_model m, nt_flat_rows f, int row_capacity, nt_contact_order o) {
    extern __shared__ __align__(16) float lds[];
    const int K = o.row_keys, E = m.env_count, t = threadIdx.x;
    int32_t* fill = (int32_t*)lds;  // [K]
    int32_t* lane_bucket = fill + K;  // [ROW_WAVE]
    const int nf = f.row_start[E] < row_capacity ? f.row_start[E] : row_capacity;
    for (int w = blockIdx.x; w < E; w += gridDim.x) {
        for (int j = t; j < K; j += ROW_WAVE) fill[j] = 0;
        __syncthreads();
        const int r0 = f.row_start[w] < nf ? f.row_start[w] : nf, r1 = f.row_start[w + 1] < nf ? f.row_start[w + 1] : nf;
        const int64_t* keys = o.row_key + (size_t)w * K;
        for (int base = r0; base < r1; base += ROW_WAVE) {  // (uniform trip count over the block)
            const int i = base + t;
            int b = -1;
            if (i < r1) {
                const int s0 = f.shape0[i], s1 = f.shape1[i];
                if (s0 != s1) {
                    const int64_t key = (int64_t)s0 * ((int64_t)1 << 32) + (int64_t)s1;
                    int lo = 0, hi = K;  // lower bound
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (keys[mid] < key) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo < K && keys[lo] == key) b = lo;
                    else atomicAdd(o.row_unmatched, 1);
                }
            }
            lane_bucket[t] = b;
            __syncthreads();
            int sub = 0;
            bool last = b >= 0;
            if (b >= 0) {
                int before = 0;
                for (int u = 0; u < ROW_WAVE; ++u) {
                    if (lane_bucket[u] != b) continue;
                    if (u < t) before += 1;
                    else if (u > t) last = false;
                }
                sub = fill[b] + before;
            }
            if (i < r1) {
                o.row_bucket[i] = b >= 0 ? o.row_rank[(size_t)w * K + b] : -1;
                o.row_sub[i] = sub;
            }
            __syncthreads();
            if (last) fill[b] = sub + 1;
            __syncthreads();
        }
        for (int j = t; j < K; j += ROW_WAVE) o.bucket_fill[o.row_rank[(size_t)w * K + j]] = fill[j];
        __syncthreads();
    }
}

__device__ inline int32_t global_id(const int32_t* gid, int32_t local) { return local >= 0 ? gid[local] : local; }
__device__ inline void st3v(float* p, size_t i, float x, float y, float z) { p[3 * i] = x; p[3 * i + 1] = y; p[3 * i + 2] = z; }

// (GLOBAL_IDS: a world group's contacts written into the arrays of the whole heterogeneous model, shape ids through `gid`)
template <bool GLOBAL_IDS>
__global__ void __launch_bounds__(256) order_slot_scatter_kernel(nt_model m, nt_contacts c, nt_contact_order o, nt_sorted_contacts s,
                                                                 const int32_t* gid) {
    const int E = m.env_count, ES = m.env_stride, cpp = m.cpp, ncs = m.np * cpp;
    const size_t n = (size_t)ncs * ES;
    for (size_t gi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gi < n; gi += (size_t)gridDim.x * blockDim.x) {
        const int slot = (int)(gi / ES), env = (int)(gi % ES);
        const int s0 = env < E ? c.shape0[gi] : -1;
        if (s0 < 0) { s.slot_flat[gi] = -1; continue; }
        const int p = slot / cpp, k = slot - p * cpp;
        const size_t pe = (size_t)p * E + env;
        const int want0 = o.tile_shape0[pe], orient = s0 == want0 ? 0 : 1;
        int sub = 0;
        for (int k2 = 0; k2 < k; ++k2) {
            const int x = c.shape0[(size_t)(p * cpp + k2) * ES + env];
            if (x >= 0 && (x == want0 ? 0 : 1) == orient) sub += 1;
        }
        const int idx = o.bucket_start[o.tile_rank[2 * pe + orient]] + sub;
        s.slot_flat[gi] = idx;
        if (idx >= s.cap) continue;
        const float* D = c.data;
        auto ld = [&](int comp) { return D[((size_t)comp * ncs + slot) * ES + env]; };
        s.shape0[idx] = GLOBAL_IDS ? gid[s0] : s0;
        s.shape1[idx] = GLOBAL_IDS ? global_id(gid, c.shape1[gi]) : c.shape1[gi];
        st3v(s.point0, idx, ld(CD_POINT0), ld(CD_POINT0 + 1), ld(CD_POINT0 + 2));
        st3v(s.point1, idx, ld(CD_POINT1), ld(CD_POINT1 + 1), ld(CD_POINT1 + 2));
        st3v(s.offset0, idx, ld(CD_OFFSET0), ld(CD_OFFSET0 + 1), ld(CD_OFFSET0 + 2));
        st3v(s.offset1, idx, ld(CD_OFFSET1), ld(CD_OFFSET1 + 1), ld(CD_OFFSET1 + 2));
        st3v(s.normal, idx, ld(CD_NORMAL), ld(CD_NORMAL + 1), ld(CD_NORMAL + 2));
        s.margin0[idx] = ld(CD_MARGIN0);
        s.margin1[idx] = ld(CD_MARGIN1);
        if (s.stiffness) {
            const float* P = c.prop;
            s.stiffness[idx] = P ? P[((size_t)0 * ncs + slot) * ES + env] : 0.0f;
            s.damping[idx] = P ? P[((size_t)1 * ncs + slot) * ES + env] : 0.0f;
            s.friction[idx] = P ? P[((size_t)2 * ncs + slot) * ES + env] : 0.0f;
        }
    }
}

template <bool GLOBAL_IDS>
__global__ void __launch_bounds__(256) order_row_scatter_kernel(nt_model m, nt_flat_rows f, nt_contact_order o, nt_sorted_contacts s,
                                                                const int32_t* gid) {
    const int E = m.env_count;
    const int nf = f.row_start[E] < s.row_capacity ? f.row_start[E] : s.row_capacity;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.row_capacity; i += gridDim.x * blockDim.x) {
        const int b = i < nf ? o.row_bucket[i] : -1;
        if (b < 0) { s.row_flat[i] = -1; continue; }
        const int idx = o.bucket_start[b] + o.row_sub[i];
        s.row_flat[i] = idx;
        if (idx >= s.cap) continue;
        s.shape0[idx] = GLOBAL_IDS ? global_id(gid, f.shape0[i]) : f.shape0[i];
        s.shape1[idx] = GLOBAL_IDS ? global_id(gid, f.shape1[i]) : f.shape1[i];
        for (int k = 0; k < 3; ++k) {
            s.point0[3 * (size_t)idx + k] = f.point0[3 * (size_t)i + k];
            s.point1[3 * (size_t)idx + k] = f.point1[3 * (size_t)i + k];
            s.offset0[3 * (size_t)idx + k] = f.offset0[3 * (size_t)i + k];
            s.offset1[3 * (size_t)idx + k] = f.offset1[3 * (size_t)i + k];
            s.normal[3 * (size_t)idx + k] = f.normal[3 * (size_t)i + k];
        }
        s.margin0[idx] = f.margin0[i];
        s.margin1[idx] = f.margin1[i];
        if (s.stiffness) {
            s.stiffness[idx] = f.stiffness ? f.stiffness[i] : 0.0f;
            s.damping[idx] = f.stiffness ? f.damping[i] : 0.0f;
            s.friction[idx] = f.stiffness ? f.friction_scale[i] : 0.0f;
        }
    }
}

// entries at or beyond the count: what a freshly filled export holds (-1 ids, 0 floats)
__global__ void __launch_bounds__(256) order_tail_kernel(nt_sorted_contacts s) {
    const int n = s.count[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.cap; i += gridDim.x * blockDim.x) {
        if (i < n) continue;
        s.shape0[i] = -1;
        s.shape1[i] = -1;
        st3v(s.point0, i, 0.0f, 0.0f, 0.0f);
        st3v(s.point1, i, 0.0f, 0.0f, 0.0f);
        st3v(s.offset0, i, 0.0f, 0.0f, 0.0f);
        st3v(s.offset1, i, 0.0f, 0.0f, 0.0f);
        st3v(s.normal, i, 0.0f, 0.0f, 0.0f);
        s.margin0[i] = 0.0f;
        s.margin1[i] = 0.0f;
        if (s.stiffness) { s.stiffness[i] = 0.0f; s.damping[i] = 0.0f; s.friction[i] = 0.0f; }
    }
}

// match_index: the previous slot / row each contact matched, as its position in the previous frame's arrays
__global__ void __launch_bounds__(256) report_map_slots_kernel(nt_model m, nt_sorted_contacts s, nt_contact_report r) {
    const int E = m.env_count, ES = m.env_stride;
    const size_t n = (size_t)m.np * m.cpp * ES;
    for (size_t gi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gi < n; gi += (size_t)gridDim.x * blockDim.x) {
        const int env = (int)(gi % ES), idx = s.slot_flat[gi];
        if (env >= E || idx < 0 || idx >= s.cap) continue;
        int v = r.slot_match[gi];
        if (v >= 0) v = r.prev_slot_flat[(size_t)v * ES + env];
        r.match_index[idx] = v;
    }
}
__global__ void __launch_bounds__(256) report_map_rows_kernel(nt_sorted_contacts s, nt_contact_report r) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.row_capacity; i += gridDim.x * blockDim.x) {
        const int idx = s.row_flat[i];
        if (idx < 0 || idx >= s.cap) continue;
        int v = r.row_match[i];
        if (v >= 0) v = r.prev_row_flat[v];
        r.match_index[idx] = v;
    }
}
// tail of match_index (-1) + the flags of the new list
__global__ void __launch_bounds__(256) report_new_flags_kernel(nt_sorted_contacts s, nt_contact_report r, int with_report) {
    const int n = s.count[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.cap; i += gridDim.x * blockDim.x) {
        if (i >= n) r.match_index[i] = -1;
        if (with_report) r.flag[i] = i < n && r.match_index[i] < 0 ? 1 : 0;
    }
}
__global__ void __launch_bounds__(256) report_compact_kernel(int cap, const int32_t* flag, const int32_t* offset, int32_t* out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x)
        if (flag[i]) out[offset[i]] = i;
}
// broken list, step 1: clear the flags
__global__ void __launch_bounds__(256) report_clear_kernel(int cap, int32_t* flag) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x) flag[i] = 0;
}
// step 2: the previous frame's contacts whose history is still alive (slots: prev_live, cleared by a world reset)
__global__ void __launch_bounds__(256) report_alive_slots_kernel(nt_model m, nt_sorted_contacts s, nt_contact_report r) {
    const int E = m.env_count, ES = m.env_stride;
    const size_t n = (size_t)m.np * m.cpp * ES;
    const int pc = r.prev_count[0];
    for (size_t gi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; gi < n; gi += (size_t)gridDim.x * blockDim.x) {
        const int env = (int)(gi % ES), idx = r.prev_slot_flat[gi];
        if (env < E && idx >= 0 && idx < pc && idx < s.cap && r.prev_slot_live[gi]) r.flag[idx] = 1;
    }
}
// (rows: prev_live, and the row's world still has its previous pairs)
__global__ void __launch_bounds__(256) report_alive_rows_kernel(nt_model m, nt_sorted_contacts s, nt_contact_report r) {
    const int E = m.env_count, pc = r.prev_count[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.row_capacity; i += gridDim.x * blockDim.x) {
        const int idx = r.prev_row_flat[i];
        if (idx < 0 || idx >= pc || idx >= s.cap || !r.prev_row_live[i]) continue;
        int lo = 0, hi = E;  // world = number of w with prev_row_start[w + 1] <= i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (r.prev_row_start[mid + 1] <= i) lo = mid + 1;
            else hi = mid;
        }
        if (lo < E && r.prev_pair_count[lo] > 0) r.flag[idx] = 1;
    }
}
// step 3: the ones this frame matched are not broken
__global__ void __launch_bounds__(256) report_hit_kernel(nt_sorted_contacts s, nt_contact_report r) {
    const int n = s.count[0] < s.cap ? s.count[0] : s.cap, pc = r.prev_count[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int v = r.match_index[i];
        if (v >= 0 && v < pc && v < s.cap) r.flag[v] = 0;
    }
}

__global__ void __launch_bounds__(256) order_save_kernel(nt_model m, nt_sorted_contacts s, nt_contact_report r) {
    const size_t ns = (size_t)m.np * m.cpp * m.env_stride;
    size_t n = ns > (size_t)s.row_capacity ? ns : (size_t)s.row_capacity;
    if (n < (size_t)m.env_count) n = (size_t)m.env_count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (i < ns) r.prev_slot_flat[i] = s.slot_flat[i];
        if (i < (size_t)s.row_capacity && r.prev_row_flat) r.prev_row_flat[i] = s.row_flat[i];
        if (i == 0) r.prev_count[0] = s.count[0];
        if (r.reset_world_mask && i < (size_t)m.env_count) r.reset_world_mask[i] = 0;
    }
}

bool sorted_ok(const nt_model* m, const nt_sorted_contacts* s) {
    return m && s && m->env_count > 0 && s->cap > 0 && s->row_capacity >= 0 && s->count && s->shape0 && s->shape1 && s->point0 &&
           s->point1 && s->offset0 && s->offset1 && s->normal && s->margin0 && s->margin1 && (m->np == 0 || s->slot_flat) &&
           (s->row_capacity == 0 || s->row_flat) && (!s->stiffness || (s->damping && s->friction));
}

}  // namespace

extern "C" {

nt_status nt_contacts_export_sorted(const nt_model* m, const nt_contacts* c, const nt_contact_order* o, nt_sorted_contacts* out,
                                    void* stream) {
    if (!c || !o || !sorted_ok(m, out) || o->bucket_count < 0 || !o->bucket_fill || !o->bucket_start || !o->block_sum)
        return NT_ERR_INVALID_ARG;
    const int E = m->env_count;
    const bool slots = m->np > 0, rows = out->row_capacity > 0;
    if (slots && (!c->shape0 || !c->shape1 || !c->data || !o->tile_shape0 || !o->tile_rank)) return NT_ERR_INVALID_ARG;
    if (rows && (!c->flat.row_start || !c->flat.shape0 || o->row_keys <= 0 || !o->row_key || !o->row_rank || !o->row_bucket ||
                 !o->row_sub || !o->row_unmatched))
        return NT_ERR_INVALID_ARG;
    if (o->bucket_count != 2 * E * m->np + (rows ? E * o->row_keys : 0)) return NT_ERR_INVALID_ARG;
    const size_t row_lds = rows ? sizeof(int32_t) * ((size_t)o->row_keys + ROW_WAVE) : 0;
    if (row_lds > 64 * 1024) return NT_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (slots)
        hipLaunchKernelGGL(order_tile_count_kernel, dim3(grid_for((size_t)m->np * E, 256)), dim3(256), 0, st, *m, *c, *o);
    if (rows)
        hipLaunchKernelGGL(order_row_bucket_kernel, dim3(grid_for((size_t)E, 1)), dim3(ROW_WAVE), row_lds, st, *m, c->flat,
                           out->row_capacity, *o);
    if (o->bucket_count > 0) {
        launch_scan(o->bucket_fill, o->bucket_count, o->block_sum, o->bucket_start, out->count, st);
    } else if (hipMemsetAsync(out->count, 0, sizeof(int32_t), st) != hipSuccess) {
        return NT_ERR_LAUNCH;
    }
    if (slots)
        hipLaunchKernelGGL(order_slot_scatter_kernel<false>, dim3(grid_for((size_t)m->np * m->cpp * m->env_stride, 256)), dim3(256), 0,
                           st, *m, *c, *o, *out, (const int32_t*)nullptr);
    if (rows)
        hipLaunchKernelGGL(order_row_scatter_kernel<false>, dim3(grid_for((size_t)out->row_capacity, 256)), dim3(256), 0, st, *m,
                           c->flat, *o, *out, (const int32_t*)nullptr);
    hipLaunchKernelGGL(order_tail_kernel, dim3(grid_for((size_t)out->cap, 256)), dim3(256), 0, st, *out);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

nt_status nt_contacts_match_report(const nt_model* m, const nt_sorted_contacts* s, const nt_contact_report* r, void* stream) {
    if (!sorted_ok(m, s) || !r || !r->prev_count || !r->match_index) return NT_ERR_INVALID_ARG;
    const bool slots = m->np > 0, rows = s->row_capacity > 0, report = r->new_indices != nullptr;
    if (slots && (!r->prev_slot_flat || !r->slot_match || !r->prev_slot_live)) return NT_ERR_INVALID_ARG;
    if (rows && (!r->prev_row_flat || !r->row_match || !r->prev_row_live || !r->prev_row_start || !r->prev_pair_count))
        return NT_ERR_INVALID_ARG;
    if (report && (!r->new_count || !r->broken_indices || !r->broken_count || !r->flag || !r->offset || !r->block_sum))
        return NT_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t nslot = (size_t)m->np * m->cpp * m->env_stride;
    const unsigned gc = grid_for((size_t)s->cap, 256);
    if (slots) hipLaunchKernelGGL(report_map_slots_kernel, dim3(grid_for(nslot, 256)), dim3(256), 0, st, *m, *s, *r);
    if (rows) hipLaunchKernelGGL(report_map_rows_kernel, dim3(grid_for((size_t)s->row_capacity, 256)), dim3(256), 0, st, *s, *r);
    hipLaunchKernelGGL(report_new_flags_kernel, dim3(gc), dim3(256), 0, st, *s, *r, report ? 1 : 0);
    if (report) {
        launch_scan(r->flag, s->cap, r->block_sum, r->offset, r->new_count, st);
        hipLaunchKernelGGL(report_compact_kernel, dim3(gc), dim3(256), 0, st, s->cap, (const int32_t*)r->flag, (const int32_t*)r->offset,
                           r->new_indices);
        hipLaunchKernelGGL(report_clear_kernel, dim3(gc), dim3(256), 0, st, s->cap, r->flag);
        if (slots) hipLaunchKernelGGL(report_alive_slots_kernel, dim3(grid_for(nslot, 256)), dim3(256), 0, st, *m, *s, *r);
        if (rows)
            hipLaunchKernelGGL(report_alive_rows_kernel, dim3(grid_for((size_t)s->row_capacity, 256)), dim3(256), 0, st, *m, *s, *r);
        hipLaunchKernelGGL(report_hit_kernel, dim3(gc), dim3(256), 0, st, *s, *r);
        launch_scan(r->flag, s->cap, r->block_sum, r->offset, r->broken_count, st);
        hipLaunchKernelGGL(report_compact_kernel, dim3(gc), dim3(256), 0, st, s->cap, (const int32_t*)r->flag, (const int32_t*)r->offset,
                           r->broken_indices);
    }
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

nt_status nt_contacts_order_save(const nt_model* m, const nt_sorted_contacts* s, const nt_contact_report* r, void* stream) {
    if (!sorted_ok(m, s) || !r || !r->prev_count || (m->np > 0 && !r->prev_slot_flat) || (s->row_capacity > 0 && !r->prev_row_flat))
        return NT_ERR_INVALID_ARG;
    const size_t nslot = (size_t)m->np * m->cpp * m->env_stride;
    size_t n = nslot > (size_t)s->row_capacity ? nslot : (size_t)s->row_capacity;
    if (n < (size_t)m->env_count) n = (size_t)m->env_count;
    hipLaunchKernelGGL(order_save_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *m, *s, *r);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

}  // extern "C"

// ---- the same over the world groups of a heterogeneous model (nt_contact_group) -------------------------------------------------
// Every per-group pass of the export indexes bucket_fill / bucket_start by rank only: with global ranks and the global scan arrays
// the groups' count passes fill disjoint entries of one bucket_fill, one scan runs over all buckets and the groups' scatters write
// disjoint ranges of one set of arrays.  The report / save passes that walk a group's slots or rows run per group; the ones over the
// arrays (new flags, compaction, hit, scans) run once.
namespace {

// what the per-group passes see: the group's table on the global scan, the global arrays with the group's positions, the group's
// matching state with the global outputs
nt_contact_order group_order(const nt_contact_group& g, const nt_contact_order* o) {
    nt_contact_order x = *g.o;
    x.bucket_fill = o->bucket_fill;
    x.bucket_start = o->bucket_start;
    x.block_sum = o->block_sum;
    return x;
}
nt_sorted_contacts group_sorted(const nt_contact_group& g, const nt_sorted_contacts* s) {
    nt_sorted_contacts x = *s;
    x.row_capacity = g.row_capacity;
    x.slot_flat = g.slot_flat;
    x.row_flat = g.row_flat;
    return x;
}
nt_contact_report group_report(const nt_contact_group& g, const nt_contact_report* r) {
    nt_contact_report x = *g.r;
    x.prev_count = r->prev_count;
    x.match_index = r->match_index;
    x.new_indices = r->new_indices;
    x.new_count = r->new_count;
    x.broken_indices = r->broken_indices;
    x.broken_count = r->broken_count;
    x.flag = r->flag;
    x.offset = r->offset;
    x.block_sum = r->block_sum;
    return x;
}

bool arrays_ok(const nt_sorted_contacts* s) {
    return s && s->cap > 0 && s->count && s->shape0 && s->shape1 && s->point0 && s->point1 && s->offset0 && s->offset1 && s->normal &&
           s->margin0 && s->margin1 && (!s->stiffness || (s->damping && s->friction));
}
bool group_ok(const nt_contact_group& g) {
    const nt_model* m = g.m;
    return m && g.c && g.o && m->env_count > 0 && g.row_capacity >= 0 && (m->np == 0 || g.slot_flat) &&
           (g.row_capacity == 0 || g.row_flat);
}
// the group's matching state (report / save)
bool group_report_ok(const nt_contact_group& g) {
    const nt_contact_report* r = g.r;
    if (!group_ok(g) || !r) return false;
    if (g.m->np > 0 && (!r->prev_slot_flat || !r->slot_match || !r->prev_slot_live)) return false;
    return g.row_capacity == 0 || (r->prev_row_flat && r->row_match && r->prev_row_live && r->prev_row_start && r->prev_pair_count);
}

}  // namespace

extern "C" {

nt_status nt_contacts_export_sorted_groups(int32_t group_count, const nt_contact_group* groups, const nt_contact_order* o,
                                           nt_sorted_contacts* out, void* stream) {
    if (group_count <= 0 || !groups || !o || !arrays_ok(out) || o->bucket_count < 0 || !o->bucket_fill || !o->bucket_start ||
        !o->block_sum)
        return NT_ERR_INVALID_ARG;
    long long buckets = 0;
    size_t row_lds_max = 0;
    for (int i = 0; i < group_count; ++i) {
        const nt_contact_group& g = groups[i];
        if (!group_ok(g)) return NT_ERR_INVALID_ARG;
        const nt_model* m = g.m;
        const nt_contacts* c = g.c;
        const nt_contact_order* go = g.o;
        const int E = m->env_count;
        const bool slots = m->np > 0, rows = g.row_capacity > 0;
        if (slots && (!c->shape0 || !c->shape1 || !c->data || !go->tile_shape0 || !go->tile_rank || !g.shape_id)) return NT_ERR_INVALID_ARG;
        if (rows && (!c->flat.row_start || !c->flat.shape0 || go->row_keys <= 0 || !go->row_key || !go->row_rank || !go->row_bucket ||
                     !go->row_sub || !go->row_unmatched || !g.shape_id))
            return NT_ERR_INVALID_ARG;
        if (go->bucket_count != 2 * E * m->np + (rows ? E * go->row_keys : 0)) return NT_ERR_INVALID_ARG;
        buckets += go->bucket_count;
        const size_t row_lds = rows ? sizeof(int32_t) * ((size_t)go->row_keys + ROW_WAVE) : 0;
        if (row_lds > row_lds_max) row_lds_max = row_lds;
    }
    if (buckets != o->bucket_count) return NT_ERR_INVALID_ARG;
    if (row_lds_max > 64 * 1024) return NT_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < group_count; ++i) {  // counts: disjoint entries of the global bucket_fill
        const nt_contact_group& g = groups[i];
        const nt_model* m = g.m;
        const nt_contact_order go = group_order(g, o);
        const int E = m->env_count;
        if (m->np > 0)
            hipLaunchKernelGGL(order_tile_count_kernel, dim3(grid_for((size_t)m->np * E, 256)), dim3(256), 0, st, *m, *g.c, go);
        if (g.row_capacity > 0)
            hipLaunchKernelGGL(order_row_bucket_kernel, dim3(grid_for((size_t)E, 1)), dim3(ROW_WAVE),
                               sizeof(int32_t) * ((size_t)go.row_keys + ROW_WAVE), st, *m, g.c->flat, g.row_capacity, go);
    }
    if (o->bucket_count > 0) {
        launch_scan(o->bucket_fill, o->bucket_count, o->block_sum, o->bucket_start, out->count, st);
    } else if (hipMemsetAsync(out->count, 0, sizeof(int32_t), st) != hipSuccess) {
        return NT_ERR_LAUNCH;
    }
    for (int i = 0; i < group_count; ++i) {  // scatters: disjoint ranges of the global arrays
        const nt_contact_group& g = groups[i];
        const nt_model* m = g.m;
        const nt_contact_order go = group_order(g, o);
        const nt_sorted_contacts gs = group_sorted(g, out);
        if (m->np > 0)
            hipLaunchKernelGGL(order_slot_scatter_kernel<true>, dim3(grid_for((size_t)m->np * m->cpp * m->env_stride, 256)), dim3(256), 0,
                               st, *m, *g.c, go, gs, g.shape_id);
        if (g.row_capacity > 0)
            hipLaunchKernelGGL(order_row_scatter_kernel<true>, dim3(grid_for((size_t)g.row_capacity, 256)), dim3(256), 0, st, *m,
                               g.c->flat, go, gs, g.shape_id);
    }
    hipLaunchKernelGGL(order_tail_kernel, dim3(grid_for((size_t)out->cap, 256)), dim3(256), 0, st, *out);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

nt_status nt_contacts_match_report_groups(int32_t group_count, const nt_contact_group* groups, const nt_sorted_contacts* s,
                                          const nt_contact_report* r, void* stream) {
    if (group_count <= 0 || !groups || !arrays_ok(s) || !r || !r->prev_count || !r->match_index) return NT_ERR_INVALID_ARG;
    const bool report = r->new_indices != nullptr;
    if (report && (!r->new_count || !r->broken_indices || !r->broken_count || !r->flag || !r->offset || !r->block_sum))
        return NT_ERR_INVALID_ARG;
    for (int i = 0; i < group_count; ++i)
        if (!group_report_ok(groups[i])) return NT_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned gc = grid_for((size_t)s->cap, 256);
    for (int i = 0; i < group_count; ++i) {  // each group's matches, through its previous positions (global) to global positions
        const nt_contact_group& g = groups[i];
        const nt_sorted_contacts gs = group_sorted(g, s);
        const nt_contact_report gr = group_report(g, r);
        if (g.m->np > 0)
            hipLaunchKernelGGL(report_map_slots_kernel, dim3(grid_for((size_t)g.m->np * g.m->cpp * g.m->env_stride, 256)), dim3(256), 0,
                               st, *g.m, gs, gr);
        if (g.row_capacity > 0)
            hipLaunchKernelGGL(report_map_rows_kernel, dim3(grid_for((size_t)g.row_capacity, 256)), dim3(256), 0, st, gs, gr);
    }
    hipLaunchKernelGGL(report_new_flags_kernel, dim3(gc), dim3(256), 0, st, *s, *r, report ? 1 : 0);
    if (report) {
        launch_scan(r->flag, s->cap, r->block_sum, r->offset, r->new_count, st);
        hipLaunchKernelGGL(report_compact_kernel, dim3(gc), dim3(256), 0, st, s->cap, (const int32_t*)r->flag, (const int32_t*)r->offset,
                           r->new_indices);
        hipLaunchKernelGGL(report_clear_kernel, dim3(gc), dim3(256), 0, st, s->cap, r->flag);
        for (int i = 0; i < group_count; ++i) {
            const nt_contact_group& g = groups[i];
            const nt_sorted_contacts gs = group_sorted(g, s);
            const nt_contact_report gr = group_report(g, r);
            if (g.m->np > 0)
                hipLaunchKernelGGL(report_alive_slots_kernel, dim3(grid_for((size_t)g.m->np * g.m->cpp * g.m->env_stride, 256)), dim3(256),
                                   0, st, *g.m, gs, gr);
            if (g.row_capacity > 0)
                hipLaunchKernelGGL(report_alive_rows_kernel, dim3(grid_for((size_t)g.row_capacity, 256)), dim3(256), 0, st, *g.m, gs, gr);
        }
        hipLaunchKernelGGL(report_hit_kernel, dim3(gc), dim3(256), 0, st, *s, *r);
        launch_scan(r->flag, s->cap, r->block_sum, r->offset, r->broken_count, st);
        hipLaunchKernelGGL(report_compact_kernel, dim3(gc), dim3(256), 0, st, s->cap, (const int32_t*)r->flag, (const int32_t*)r->offset,
                           r->broken_indices);
    }
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

nt_status nt_contacts_order_save_groups(int32_t group_count, const nt_contact_group* groups, const nt_sorted_contacts* s,
                                        const nt_contact_report* r, void* stream) {
    if (group_count <= 0 || !groups || !arrays_ok(s) || !r || !r->prev_count) return NT_ERR_INVALID_ARG;
    for (int i = 0; i < group_count; ++i)
        if (!group_report_ok(groups[i])) return NT_ERR_INVALID_ARG;
    for (int i = 0; i < group_count; ++i) {  // (every group's pass also writes the global count into r->prev_count)
        const nt_contact_group& g = groups[i];
        const nt_model* m = g.m;
        const size_t nslot = (size_t)m->np * m->cpp * m->env_stride;
        size_t n = nslot > (size_t)g.row_capacity ? nslot : (size_t)g.row_capacity;
        if (n < (size_t)m->env_count) n = (size_t)m->env_count;
        hipLaunchKernelGGL(order_save_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *m, group_sorted(g, s),
                           group_report(g, r));
    }
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

}  // extern "C"

// ---- nt_contact_sensor (newton_amd.sensors.SensorContact; contract: include/newton_hip_contacts.h) -----------------------------------
// Net contact force per world on S sets of shapes, split by C counterparts, straight from the slot-major contacts and the rows.
// A workgroup of CS_THREADS lanes serves wpb worlds (CS_THREADS / wpb lanes each; wpb shrinks from CS_MAX_WPB while a world has more
// output cells than lanes).  The entries of a world -- its slots in ascending index, then its rows -- pass through a fixed staging
// buffer of CS_ITEMS records in rounds of CS_ITEMS / wpb entries per world: one (entry, world) per lane with the world the fastest index
// (the env-major [slot][ES] arrays are read in runs of wpb consecutive floats), resolved to (sensing object and counterpart of either
// shape, f[3]) once.  After the barrier one lane per output cell walks the round's records of its world in entry order and adds in
// registers: the lanes of a world read the same record (LDS broadcast), different worlds neighbouring words (the records are SoA with
// the world innermost: no bank conflict).  A cell is owned by one lane from the first entry to the last, so the sum is the contract's
// sequential one whatever wpb is; worlds with more cells than lanes take further passes over the same entries.
namespace {

constexpr int CS_THREADS = 256;  // lanes of a workgroup
constexpr int CS_MAX_WPB = 16;   // worlds per workgroup, at most (a power of two)
constexpr int CS_ITEMS = 512;    // staged records per round, over the workgroup's worlds: 7 words each, 14 KB of LDS

// shape slot of a world (env-local slots, then the global shapes) that carries Newton shape id `id`, -1: none of this world's
__device__ inline int cs_slot_of(const nt_model& m, int e, int id) {
    const int l = id - m.shape_local0 - e * m.ns;
    if (id >= 0 && l >= 0 && l < m.ns) return l;
    for (int k = 0; k < m.ng; ++k)
        if (m.gshape_id[k] == id) return m.ns + k;
    return -1;
}
__device__ inline int cs_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ void __launch_bounds__(CS_THREADS) contact_sensor_kernel(nt_model m, nt_contacts c, const float* __restrict__ impulse, float inv_dt,
                                                                    nt_contact_sensor_args a, int wpb) {
    __shared__ int32_t cs_side[2][CS_ITEMS];   // sensing object of shape0 / shape1 (-1: none; both -1: nothing to add)
    __shared__ int32_t cs_other[2][CS_ITEMS];  // counterpart of shape0 / shape1
    __shared__ float cs_f[3][CS_ITEMS];
    const int tid = threadIdx.x, E = m.env_count, nslot = m.np * m.cpp;
    const size_t ES = (size_t)m.env_stride;
    const int rl = CS_THREADS / wpb, chunk = CS_ITEMS / wpb;
    const int S = a.sensing_count, cols = a.include_total + a.counterpart_count, cells = S * cols;
    const nt_flat_rows& fr = c.flat;
    const bool rows = a.row_capacity > 0 && fr.impulse != nullptr;
    const int nf = rows ? cs_clamp(fr.row_start[E], a.row_capacity) : 0;
    const int groups = (E + wpb - 1) / wpb;
    const int wl = tid / rl, ln = tid - wl * rl;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        // the longest entry list of the group's selected worlds: the trip count of the rounds, uniform over the workgroup
        int longest = nslot;
        if (rows)
            for (int u = 0; u < wpb; ++u) {
                const int eu = g * wpb + u;
                if (eu >= E || (a.world_mask && !a.world_mask[eu])) continue;
                const int n = nslot + cs_clamp(fr.row_start[eu + 1], nf) - cs_clamp(fr.row_start[eu], nf);
                longest = n > longest ? n : longest;
            }
        const int e = g * wpb + wl;
        const bool live = e < E && !(a.world_mask && !a.world_mask[e]);
        int n_e = nslot;
        if (live && rows) {
            const int n = nslot + cs_clamp(fr.row_start[e + 1], nf) - cs_clamp(fr.row_start[e], nf);
            n_e = n > n_e ? n : n_e;
        }
        for (int cell0 = 0; cell0 < cells; cell0 += rl) {
            const int cell = cell0 + ln;
            const bool active = live && cell < cells;
            const int s = cell / cols, col = cell - s * cols, cp = col - a.include_total;  // cp < 0: the total column
            float ax = 0.0f, ay = 0.0f, az = 0.0f;
            for (int base = 0; base < longest; base += chunk) {
                __syncthreads();  // the previous round's records are no longer read
                for (int item = tid; item < CS_ITEMS; item += CS_THREADS) {
                    const int j = item / wpb, u = item - j * wpb, eu = g * wpb + u, n = base + j;
                    int k0 = -1, k1 = -1;
                    if (eu < E && !(a.world_mask && !a.world_mask[eu])) {
                        int s0 = -1, s1 = -1;
                        const float* f = nullptr;
                        size_t stride = 1;
                        if (n < nslot) {
                            const size_t gi = (size_t)n * ES + eu;
                            s0 = c.shape0[gi];
                            if (s0 >= 0) {
                                s1 = c.shape1[gi];
                                f = impulse + gi;
                                stride = (size_t)nslot * ES;
                            }
                        } else if (rows) {
                            const int r0 = cs_clamp(fr.row_start[eu], nf), r1 = cs_clamp(fr.row_start[eu + 1], nf), r = r0 + (n - nslot);
                            if (r < r1) {
                                s0 = fr.shape0[r];
                                s1 = fr.shape1[r];
                                if (s0 != s1) f = fr.impulse + 6 * (size_t)r;
                            }
                        }
                        if (f) {
                            const int a0 = cs_slot_of(m, eu, s0), a1 = cs_slot_of(m, eu, s1);
                            k0 = a0 >= 0 ? a.slot_sensing[a0] : -1;
                            k1 = a1 >= 0 ? a.slot_sensing[a1] : -1;
                            if (k0 >= 0 || k1 >= 0) {
                                const bool cps = a.counterpart_count > 0;
                                cs_other[0][item] = cps && a0 >= 0 ? a.slot_counterpart[a0] : -1;
                                cs_other[1][item] = cps && a1 >= 0 ? a.slot_counterpart[a1] : -1;
                                cs_f[0][item] = f[0] * inv_dt;
                                cs_f[1][item] = f[stride] * inv_dt;
                                cs_f[2][item] = f[2 * stride] * inv_dt;
                            }
                        }
                    }
                    cs_side[0][item] = k0;
                    cs_side[1][item] = k1;
                }
                __syncthreads();
                if (active) {
                    const int left = n_e - base, jn = left < chunk ? left : chunk;
                    for (int j = 0; j < jn; ++j) {  // entry order
                        const int item = j * wpb + wl;
                        const int k0 = cs_side[0][item], k1 = cs_side[1][item];
                        if (k0 == s && (cp < 0 || cs_other[1][item] == cp)) {  // on the sensing object as shape0: +f
                            ax = ax + cs_f[0][item];
                            ay = ay + cs_f[1][item];
                            az = az + cs_f[2][item];
                        }
                        if (k1 == s && (cp < 0 || cs_other[0][item] == cp)) {  // as shape1: -f
                            ax = ax - cs_f[0][item];
                            ay = ay - cs_f[1][item];
                            az = az - cs_f[2][item];
                        }
                    }
                }
            }
            if (active) {
                float* out = a.net_force + 3 * ((size_t)e * cells + cell);
                out[0] = ax; out[1] = ay; out[2] = az;
            }
        }
    }
}

}  // namespace

extern "C" nt_status nt_contact_sensor(const nt_model* m, const nt_contacts* c, const float* contact_impulse, float dt,
                                       const nt_contact_sensor_args* a, void* stream) {
    if (!m || !c || !a || !a->slot_sensing || !a->slot_sensing_host || !a->net_force || a->sensing_count <= 0 || a->counterpart_count < 0 ||
        (a->include_total != 0 && a->include_total != 1) || a->include_total + a->counterpart_count <= 0 || a->row_capacity < 0 ||
        !(dt > 0.0f) || !(dt <= 3.0e38f) || m->env_count <= 0 || m->env_stride < m->env_count || m->ns < 0 || m->ng < 0 || m->np < 0 ||
        m->cpp < 0 || m->ns + m->ng <= 0 || (m->ng > 0 && !m->gshape_id))
        return NT_ERR_INVALID_ARG;
    if (a->counterpart_count > 0 && (!a->slot_counterpart || !a->slot_counterpart_host)) return NT_ERR_INVALID_ARG;
    if ((long long)m->np * m->cpp > 0 && (!c->shape0 || !c->shape1 || !contact_impulse)) return NT_ERR_INVALID_ARG;
    if (a->row_capacity > 0 && c->flat.impulse && (!c->flat.row_start || !c->flat.shape0 || !c->flat.shape1)) return NT_ERR_INVALID_ARG;
    for (int k = 0; k < m->ns + m->ng; ++k) {
        if (a->slot_sensing_host[k] < -1 || a->slot_sensing_host[k] >= a->sensing_count) return NT_ERR_INVALID_ARG;
        if (a->counterpart_count > 0 && (a->slot_counterpart_host[k] < -1 || a->slot_counterpart_host[k] >= a->counterpart_count))
            return NT_ERR_INVALID_ARG;
    }
    const long long cells = (long long)a->sensing_count * (a->include_total + a->counterpart_count);
    if (cells > 0x7fffffffLL / 4 / m->env_count) return NT_ERR_INVALID_ARG;  // (the cell index of a world stays an int)
    // worlds per workgroup: as many as still leave every output cell of a world a lane of its own
    int wpb = CS_MAX_WPB;
    while (wpb > 1 && wpb * cells > CS_THREADS) wpb /= 2;
    hipLaunchKernelGGL(contact_sensor_kernel, dim3(grid_for(((size_t)m->env_count + wpb - 1) / wpb, 1)), dim3(CS_THREADS), 0,
                       (hipStream_t)stream, *m, *c, contact_impulse, 1.0f / dt, *a, wpb);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}
