// nt_mesh_plane.hip -- MESH vs infinite plane for gfx950: the vertex leg of CollisionPipeline.collide (include/newton_hip_mesh.h).
// Also home of raycast_kernel / nt_raycast (further down): a unit of the mesh legs with the default scheduler, nt_math.hpp and the mesh tables' header.
//
// Reference behaviour (paths under /root/reference/newton/_src/geometry):
//   routing      narrow_phase.py:618-631     (infinite plane, mesh) pairs -> shape_pairs_mesh_plane, stored (mesh, plane)
//   contacts     narrow_phase.py:1866-1990   one lane per vertex: world point, projection through the plane's frame, distance,
//                                            admission distance < gap sum + margin sum, centre = midpoint, normal = -n
//   reduction    contact_reduction_global.py:2059-2096 (write_contact_to_reducer: position, depth, octahedral normal code),
//                :1246-1346 (reduce_contact_in_hashtable, beta = 1e-4), :2098-2290 (export: roundoff twins, every contact once)
//
// MI355X design.  The reference spreads a pair's vertices over several blocks, buffers every admitted contact in global memory,
// registers the buffer in a device-wide hashtable in a second launch and exports in a third.  Here one workgroup owns a pair: its
// 256 lanes stride over the vertices (12 B each, shared by every world of a replicated scene -> L2 hits after the first world),
// an admitted contact goes straight into the pair's reduction table in LDS (245 x ds_max_u64, nt_contact_reduce.hpp), and the
// <= 245 winners recompute their record from the vertex index after the barrier (same instructions, same bits) -- no contact
// buffer, no hashtable, one launch.  The packed value carries the fingerprint (vertex index, < 2^22), which is unique inside a
// pair.  Rows leave as one contiguous block per pair in ascending vertex order, the order `deterministic=True` sorts into.
// HBM-bound integer / float streaming: vertices in, <= a few dozen 44-byte rows out per pair.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/newton_hip.h"
#include "../../include/newton_hip_mesh.h"
#include "nt_math.hpp"

using namespace nt;

namespace {

#include "nt_contact_reduce.hpp"

constexpr int GEO_PLANE = 1;
constexpr float RED_BETA = 0.0001f;  // contact_reduction_global.py:89 BETA_THRESHOLD

NT_DI xform ld_xform(const float* p) { return xform(vec3(p[0], p[1], p[2]), quat(p[3], p[4], p[5], p[6])); }

NT_DI int mp_live_pairs(const nt_mesh_plane_args& a) { return a.pair_world_prefix ? a.pair_world_prefix[a.worlds] : a.pair_count; }
NT_DI int mp_pair_slot(const nt_mesh_plane_args& a, int f) {  // flat live index -> position w * pairs_per_world + k
    if (!a.pair_world_prefix) return f;
    int lo = 0, hi = a.worlds;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.pair_world_prefix[mid] <= f) lo = mid;
        else hi = mid;
    }
    return lo * a.pairs_per_world + (f - a.pair_world_prefix[lo]);
}

struct PairCtx {  // what every vertex of the pair shares
    xform X_mesh, X_plane, X_plane_sw;
    vec3 plane_normal, scale;
    float threshold, margin_mesh, margin_plane;
    int mesh, plane, v0, nv;
};

NT_DI void pair_setup(const nt_mesh_plane_args& a, int s0, int s1, PairCtx& c) {
    const bool plane_first = a.shape_type[s0] == GEO_PLANE;
    c.mesh = plane_first ? s1 : s0;
    c.plane = plane_first ? s0 : s1;
    c.X_mesh = ld_xform(a.shape_transform + 7 * (size_t)c.mesh);
    c.X_plane = ld_xform(a.shape_transform + 7 * (size_t)c.plane);
    c.X_plane_sw = xform_inverse(c.X_plane);
    c.plane_normal = xform_vector(c.X_plane, vec3(0.0f, 0.0f, 1.0f));
    const float* dm = a.shape_data + 4 * (size_t)c.mesh;
    c.scale = vec3(dm[0], dm[1], dm[2]);
    c.margin_mesh = dm[3];
    c.margin_plane = a.shape_data[4 * (size_t)c.plane + 3];
    const float gap_sum = a.shape_gap[c.mesh] + a.shape_gap[c.plane];
    c.threshold = gap_sum + (c.margin_mesh + c.margin_plane);
    c.v0 = a.shape_vertex_range[2 * (size_t)c.mesh];
    c.nv = a.shape_vertex_range[2 * (size_t)c.mesh + 1];
}

// the contact of vertex vi, if it is within margin + gap of the plane
NT_DI bool vertex_contact(const nt_mesh_plane_args& a, const PairCtx& c, int vi, vec3& centre, float& distance) {
    const float* p = a.vertices + 3 * (size_t)(c.v0 + vi);
    const vec3 local(p[0] * c.scale.x, p[1] * c.scale.y, p[2] * c.scale.z);  // wp.cw_mul
    const vec3 world = xform_point(c.X_mesh, local);
    const vec3 in_plane = xform_point(c.X_plane_sw, world);
    const vec3 on_plane = xform_point(c.X_plane, vec3(in_plane.x, in_plane.y, 0.0f));
    distance = dot(world - on_plane, c.plane_normal);
    if (!(distance < c.threshold)) return false;
    centre = (world + on_plane) * 0.5f;
    return true;
}

// reduce_contact_in_hashtable for one buffered contact (position, octahedral-coded normal, depth) of the pair
NT_DI void red_offer_buffered(unsigned long long* tbl, vec3 normal_decoded, vec3 position, float depth, const xform& X_a_inv,
                              const float* lo, const float* hi, const int* res, int fp) {
    const int b = red_get_slot(normal_decoded);
    vec3 u, v;
    red_face_frame(b, u, v);
    const float px = dot(position, u), py = dot(position, v);
    const vec3 diag(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]);
    if (depth < RED_BETA * length(diag)) {
        for (int d = 0; d < RED_DIRS; ++d) {
            const float score = px * RED_DIR[d][0] + py * RED_DIR[d][1];
            atomicMax(&tbl[b * RED_VALUES + d], red_value_depth(score, fp));
        }
    }
    const unsigned long long dv = red_value_depth(-depth, fp);
    atomicMax(&tbl[b * RED_VALUES + RED_DIRS], dv);
    int vox = red_voxel_index(xform_point(X_a_inv, position), lo, hi, res);
    vox = vox < 0 ? 0 : (vox > RED_VOXELS - 1 ? RED_VOXELS - 1 : vox);
    atomicMax(&tbl[(RED_BINS + vox / RED_VALUES) * RED_VALUES + vox % RED_VALUES], dv);
}

NT_DI void write_row(const nt_mesh_plane_args& a, const PairCtx& c, int slot, int pair_idx, int vi, vec3 centre, vec3 normal, float dist) {
    a.out_pair[slot] = pair_idx;
    a.out_key[slot] = vi;
    float* o = a.out_data + 9 * (size_t)slot;
    o[0] = centre.x; o[1] = centre.y; o[2] = centre.z;
    o[3] = normal.x; o[4] = normal.y; o[5] = normal.z;
    o[6] = dist;
    o[7] = c.margin_mesh;
    o[8] = c.margin_plane;
}

__global__ void __launch_bounds__(256) mesh_plane_pairs_kernel(nt_mesh_plane_args a) {
    __shared__ RedLds L;
    __shared__ int wave_hits[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int live = mp_live_pairs(a);
    for (int f = blockIdx.x; f < live; f += gridDim.x) {
        const int pair_idx = mp_pair_slot(a, f);
        if (a.pair_kind && a.pair_kind[pair_idx] != NT_PAIR_KIND_MESH_PLANE) continue;  // another leg's pair (uniform)
        const int s0 = a.pairs[2 * (size_t)pair_idx], s1 = a.pairs[2 * (size_t)pair_idx + 1];
        PairCtx c;
        pair_setup(a, s0, s1, c);
        __syncthreads();  // every lane has read the pair before it is rewritten as (mesh, plane)
        if (t == 0) { a.pairs[2 * (size_t)pair_idx] = c.mesh; a.pairs[2 * (size_t)pair_idx + 1] = c.plane; }
        const vec3 normal = -c.plane_normal;
        if (!a.reduce) {
            // every admitted vertex is a row, ascending vertex order: rounds of 256 vertices, ballot-compacted
            if (t == 0) L.total = 0;
            __syncthreads();
            int counted = 0;
            for (int pass = 0; pass < 2; ++pass) {  // pass 0 counts, pass 1 writes behind the pair's base
                int run = 0;
                for (int v0 = 0; v0 < c.nv; v0 += 256) {
                    const int vi = v0 + t;
                    vec3 centre;
                    float dist = 0.0f;
                    const bool hit = vi < c.nv && vertex_contact(a, c, vi, centre, dist);
                    const unsigned long long m = __ballot(hit);
                    if (lane == 0) wave_hits[wave] = __popcll(m);
                    __syncthreads();
                    int off = run;
                    for (int k = 0; k < wave; ++k) off += wave_hits[k];
                    if (pass == 1 && hit) {
                        const int slot = L.base + off + __popcll(m & ((1ull << lane) - 1ull));
                        if (slot < a.capacity) write_row(a, c, slot, pair_idx, vi, centre, normal, dist);
                    }
                    run += wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
                    __syncthreads();
                }
                if (pass == 0) {
                    counted = run;
                    if (t == 0) {
                        L.base = counted > 0 ? atomicAdd(a.out_count, counted) : 0;
                        const int room = a.capacity - L.base;
                        a.out_blk[2 * (size_t)pair_idx] = L.base;
                        a.out_blk[2 * (size_t)pair_idx + 1] = counted < room ? counted : (room > 0 ? room : 0);
                    }
                    __syncthreads();
                    if (counted == 0) break;
                }
            }
            continue;
        }
        for (int k = t; k < RED_SLOTS; k += blockDim.x) { L.tbl[k] = 0ull; L.fp[k] = -1; L.keep[k] = 0; }
        __syncthreads();
        // what the buffer would hold of the normal: its octahedral code, decoded again (every contact of the pair shares it)
        float ox, oy;
        red_encode_oct(normal, ox, oy);
        const vec3 normal_buffered = red_decode_oct(ox, oy);
        const xform X_mesh_inv = xform_inverse(c.X_mesh);
        const float* lo = a.shape_aabb_lower + 3 * (size_t)c.mesh;
        const float* hi = a.shape_aabb_upper + 3 * (size_t)c.mesh;
        const int* res = a.shape_voxel_res + 3 * (size_t)c.mesh;
        for (int vi = t; vi < c.nv; vi += blockDim.x) {
            vec3 centre;
            float dist;
            if (vertex_contact(a, c, vi, centre, dist)) red_offer_buffered(L.tbl, normal_buffered, centre, dist, X_mesh_inv, lo, hi, res, vi);
        }
        __syncthreads();
        for (int k = t; k < RED_SLOTS; k += blockDim.x) {  // the winner of slot k: its record recomputed from the vertex index
            if (L.tbl[k] == 0ull) continue;
            const int vi = (int)(L.tbl[k] & RED_FP_MASK);
            vec3 centre;
            float dist;
            vertex_contact(a, c, vi, centre, dist);
            L.pos[k][0] = centre.x; L.pos[k][1] = centre.y; L.pos[k][2] = centre.z; L.pos[k][3] = dist;
            L.oct[k][0] = ox; L.oct[k][1] = oy;
            L.fp[k] = vi;
        }
        __syncthreads();
        red_finish(L, RedLdsRec{L});
        if (t == 0) {
            L.base = L.total > 0 ? atomicAdd(a.out_count, L.total) : 0;
            const int room = a.capacity - L.base;
            a.out_blk[2 * (size_t)pair_idx] = L.base;
            a.out_blk[2 * (size_t)pair_idx + 1] = L.total < room ? L.total : (room > 0 ? room : 0);
        }
        __syncthreads();
        for (int k = t; k < RED_SLOTS; k += blockDim.x) {
            const int slot = L.base + L.keep[k];
            if (L.keep[k] < 0 || slot >= a.capacity) continue;
            write_row(a, c, slot, pair_idx, L.fp[k], vec3(L.pos[k][0], L.pos[k][1], L.pos[k][2]), normal_buffered, L.pos[k][3]);
        }
        __syncthreads();
    }
}


// ------------------------------------------------------------------------------------------------------------------------------
// nt_raycast (newton_amd.sensors.SensorRaycast; contract: include/newton_hip_mesh.h): R rays per world against the selected shapes.
//
// MI355X mapping.  A workgroup of 256 lanes serves `wpb` worlds (4 / 2 / 1 for R <= 64 / 128 / more) with `rl` = 256 / wpb lanes each.
// It stages the selected targets of its worlds once in LDS -- world pose (body_q * shape xform), scale, type, Newton id: RC_REC = 12
// words per (world, target), read from the env-major tables with one (world, target) per lane -- and after one barrier every lane
// owns one ray (rays r, r + rl, ... when R > rl): it loads its ray, puts it into the world frame from body_q, and walks the staged
// records in ascending slot order.  All lanes of a world read the SAME record at the same time: an LDS broadcast, no bank conflicts.
// Meshes and heightfields follow in a second pass over the records; their vertices, indices, block bounds and elevations come from
// HBM / L2 (shared by every world of a replicated scene).  One lane produces every value of a ray: no atomics, no cross-lane
// reduction, so the launch geometry cannot change a bit.  What bounds it: LDS only for thousands of targets (48 B each per world);
// the primitive pass is ALU work on broadcast records, the mesh pass is divergent L2 latency (every lane walks its own blocks).
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int RC_REC = 12;  // staged words per (world, target): p[3] q[4] scale[3] type id
constexpr int RC_THREADS = 256;
constexpr size_t RC_LDS_BYTES_PER_CU = 160 * 1024;
constexpr int RC_PLANE = 1, RC_HFIELD = 2, RC_SPHERE = 3, RC_CAPSULE = 4, RC_ELLIPSOID = 5, RC_CYLINDER = 6, RC_BOX = 7, RC_MESH = 8, RC_CONE = 9;
constexpr float RC_INF = 3.0e38f;

struct RcBest {  // the nearest hit so far: t, Newton shape id, staged record, unnormalised normal in the shape frame
    float t;
    int id, k;
    vec3 n;
};

NT_DI void rc_offer(RcBest& b, float max_distance, float t, int id, int k, vec3 n) {
    if (!(t >= 0.0f) || !(t <= max_distance)) return;
    if (t < b.t || (t == b.t && id < b.id)) { b.t = t; b.id = id; b.k = k; b.n = n; }
}

// entering root of |o + t d| = radius, from the ray's point nearest the centre; p = hit point relative to the centre
NT_DI bool rc_sphere(vec3 o, vec3 d, float radius, float& t, vec3& p) {
    const float a = dot(d, d);
    const float t0 = -dot(o, d) / a;
    const vec3 c = o + d * t0;
    const float disc = radius * radius - dot(c, c);
    if (!(disc > 0.0f)) return false;
    const float h = sqrtf(disc / a);
    t = t0 - h;
    p = c - d * h;
    return true;
}

// entering root on the infinite cylinder x^2 + y^2 = r^2 (2-D, from the point nearest the axis).  0: miss, 1: root, 2: parallel inside
NT_DI int rc_lateral(vec3 o, vec3 d, float r, float& t) {
    const float a = d.x * d.x + d.y * d.y;
    if (!(a > 0.0f)) return (o.x * o.x + o.y * o.y < r * r) ? 2 : 0;
    const float t0 = -(o.x * d.x + o.y * d.y) / a;
    const float cx = o.x + d.x * t0, cy = o.y + d.y * t0;
    const float disc = r * r - (cx * cx + cy * cy);
    if (!(disc > 0.0f)) return 0;
    t = t0 - sqrtf(disc / a);
    return 1;
}

NT_DI bool rc_capsule(vec3 o, vec3 d, float r, float hh, float& t, vec3& n) {
    float tl = 0.0f;
    const int lat = rc_lateral(o, d, r, tl);
    if (lat == 0) return false;
    float end;  // which hemisphere
    if (lat == 1) {
        const float z = o.z + d.z * tl;
        if (fabsf(z) <= hh) { t = tl; n = vec3(o.x + d.x * tl, o.y + d.y * tl, 0.0f); return true; }
        end = z > 0.0f ? hh : -hh;
    } else {
        end = d.z < 0.0f ? hh : -hh;
    }
    vec3 p;
    if (!rc_sphere(vec3(o.x, o.y, o.z - end), d, r, t, p)) return false;
    if (p.z * end < 0.0f) return false;  // (the inner half of the end sphere: not the capsule's surface)
    n = p;
    return true;
}

NT_DI bool rc_cylinder(vec3 o, vec3 d, float r, float hh, float& t, vec3& n) {
    float tl = 0.0f;
    const int lat = rc_lateral(o, d, r, tl);
    if (lat == 0) return false;
    float end;
    if (lat == 1) {
        const float z = o.z + d.z * tl;
        if (fabsf(z) <= hh) { t = tl; n = vec3(o.x + d.x * tl, o.y + d.y * tl, 0.0f); return true; }
        end = z > 0.0f ? hh : -hh;
    } else {
        end = d.z < 0.0f ? hh : -hh;
    }
    if (!(d.z * end < 0.0f)) return false;  // the cap has to face the ray
    t = (end - o.z) / d.z;
    const float x = o.x + d.x * t, y = o.y + d.y * t;
    if (!(x * x + y * y <= r * r)) return false;
    n = vec3(0.0f, 0.0f, end);
    return true;
}

// (a ray that only touches the box misses it, like a tangent to the sphere: t_in < t_out, and |c| < half on an axis it does not move along)
NT_DI bool rc_box(vec3 o, vec3 d, vec3 half, float& t, vec3& n) {
    const float t0 = -dot(o, d) / dot(d, d);
    const vec3 c = o + d * t0;
    float t_in = -RC_INF, t_out = RC_INF;
    int axis = 0;
#define RC_SLAB(I, C, D, H)                                   \
    if ((D) != 0.0f) {                                        \
        const float ta = (-(H) - (C)) / (D), tb = ((H) - (C)) / (D); \
        const float tn = fminw(ta, tb), tf = fmaxw(ta, tb);   \
        if (tn > t_in) { t_in = tn; axis = (I); }             \
        t_out = fminw(t_out, tf);                             \
    } else if (fabsf(C) >= (H)) {                             \
        return false;                                         \
    }
    RC_SLAB(0, c.x, d.x, half.x)
    RC_SLAB(1, c.y, d.y, half.y)
    RC_SLAB(2, c.z, d.z, half.z)
#undef RC_SLAB
    if (!(t_in < t_out)) return false;
    t = t0 + t_in;
    const float da = vget(d, axis);
    n = vec3();
    vset(n, axis, da > 0.0f ? -1.0f : 1.0f);
    return true;
}

NT_DI bool rc_cone(vec3 o, vec3 d, float r, float hh, float& t, vec3& n) {
    const float t0 = -dot(o, d) / dot(d, d);
    const vec3 c = o + d * t0;
    const float k = hh > 0.0f ? r / (2.0f * hh) : 0.0f, k2 = k * k;
    const float w0 = hh - c.z;
    const float A = d.x * d.x + d.y * d.y - k2 * d.z * d.z;
    const float B = c.x * d.x + c.y * d.y + k2 * w0 * d.z;
    const float C = c.x * c.x + c.y * c.y - k2 * w0 * w0;
    float best = RC_INF;
    vec3 bn;
    const float disc = B * B - A * C;
    if (disc >= 0.0f) {
        const float q = -(B + (B < 0.0f ? -1.0f : 1.0f) * sqrtf(disc));
        for (int i = 0; i < 2; ++i) {
            if ((i == 0 ? A : q) == 0.0f) continue;
            const float tr = i == 0 ? q / A : C / q;
            const float w = w0 - tr * d.z;
            if (!(w > 0.0f) || !(w <= 2.0f * hh)) continue;
            const vec3 nn(c.x + d.x * tr, c.y + d.y * tr, k2 * w);
            if (!(dot(nn, d) < 0.0f)) continue;
            if (tr < best) { best = tr; bn = nn; }
        }
    }
    if (d.z > 0.0f) {  // the base disc, facing -z
        const float tr = (-hh - c.z) / d.z;
        const float x = c.x + d.x * tr, y = c.y + d.y * tr;
        if (x * x + y * y <= r * r && tr < best) { best = tr; bn = vec3(0.0f, 0.0f, -1.0f); }
    }
    if (!(best < RC_INF)) return false;
    t = t0 + best;
    n = bn;
    return true;
}

// one primitive in its own frame
NT_DI bool rc_primitive(int type, vec3 s, vec3 o, vec3 d, float& t, vec3& n) {
    if (type == RC_PLANE) {
        if (!(d.z < 0.0f)) return false;
        t = -o.z / d.z;
        if (s.x != 0.0f || s.y != 0.0f) {
            const float x = o.x + d.x * t, y = o.y + d.y * t;
            if (!(fabsf(x) <= s.x) || !(fabsf(y) <= s.y)) return false;
        }
        n = vec3(0.0f, 0.0f, 1.0f);
        return true;
    }
    if (type == RC_SPHERE || type == RC_ELLIPSOID) {
        const vec3 rad = type == RC_SPHERE ? vec3(s.x, s.x, s.x) : s;
        vec3 p;
        if (!rc_sphere(vec3(o.x / rad.x, o.y / rad.y, o.z / rad.z), vec3(d.x / rad.x, d.y / rad.y, d.z / rad.z), 1.0f, t, p)) return false;
        n = vec3(p.x / rad.x, p.y / rad.y, p.z / rad.z);
        return true;
    }
    if (type == RC_BOX) return rc_box(o, d, s, t, n);
    if (type == RC_CAPSULE) return rc_capsule(o, d, s.x, s.y, t, n);
    if (type == RC_CYLINDER) return rc_cylinder(o, d, s.x, s.y, t, n);
    if (type == RC_CONE) return rc_cone(o, d, s.x, s.y, t, n);
    return false;
}

// Moeller-Trumbore, front faces only (det > 0 <=> n . d < 0 for n = e1 x e2), edges inclusive
NT_DI bool rc_triangle(vec3 o, vec3 d, vec3 v0, vec3 v1, vec3 v2, float& t, vec3& n) {
    const vec3 e1 = v1 - v0, e2 = v2 - v0;
    const vec3 pvec = cross(d, e2);
    const float det = dot(e1, pvec);
    if (!(det > 0.0f)) return false;
    const vec3 tvec = o - v0;
    const float u = dot(tvec, pvec);
    if (u < 0.0f || u > det) return false;
    const vec3 qvec = cross(tvec, e1);
    const float v = dot(d, qvec);
    if (v < 0.0f || u + v > det) return false;
    t = dot(e2, qvec) / det;
    n = cross(e1, e2);
    return true;
}

// the t range of the ray inside the box [lo, hi]; false: it misses the box
NT_DI bool rc_clip(vec3 o, vec3 d, vec3 lo, vec3 hi, float& t_in, float& t_out) {
#define RC_CLIP(O, D, LO, HI)                                              \
    if ((D) != 0.0f) {                                                     \
        const float ta = ((LO) - (O)) / (D), tb = ((HI) - (O)) / (D);       \
        t_in = fmaxw(t_in, fminw(ta, tb));                                 \
        t_out = fminw(t_out, fmaxw(ta, tb));                               \
    } else if ((O) < (LO) || (O) > (HI)) {                                 \
        return false;                                                      \
    }
    RC_CLIP(o.x, d.x, lo.x, hi.x)
    RC_CLIP(o.y, d.y, lo.y, hi.y)
    RC_CLIP(o.z, d.z, lo.z, hi.z)
#undef RC_CLIP
    return t_in <= t_out;
}

NT_DI vec3 rc_ld3(const float* p) { return vec3(p[0], p[1], p[2]); }

// every triangle of mesh shape `id` in ascending index (ties keep the lower index); blocks whose padded box the ray misses are skipped
NT_DI void rc_mesh(const nt_raycast_args& a, int id, int k, vec3 s, vec3 o, vec3 d, float max_distance, RcBest& best) {
    const int v0 = a.shape_vertex_range[2 * (size_t)id], nv = a.shape_vertex_range[2 * (size_t)id + 1];
    const int t0 = a.shape_triangle_range[2 * (size_t)id], ntri = a.shape_triangle_range[2 * (size_t)id + 1];
    const bool blocks = a.block_bounds != nullptr && a.shape_block_start != nullptr;
    float bt = RC_INF;
    vec3 bn;
    for (int b0 = 0; b0 < ntri; b0 += NT_MESH_TRIANGLE_BLOCK) {
        if (blocks) {
            const float* bb = a.block_bounds + 6 * (size_t)(a.shape_block_start[id] + b0 / NT_MESH_TRIANGLE_BLOCK);
            const vec3 c0 = cw_mul(rc_ld3(bb), s), c1 = cw_mul(rc_ld3(bb + 3), s);
            vec3 lo = vmin(c0, c1), hi = vmax(c0, c1);
            // padded far beyond the rounding of the triangle test (1e-7 relative): the skip never removes a hit
            const vec3 ao = vabs(o);
            const float pad = 1.0e-4f * (fmaxw(fmaxw(ao.x, ao.y), ao.z) + length(hi - lo)) + 1.0e-6f;
            lo = lo - vec3(pad);
            hi = hi + vec3(pad);
            float t_in = -pad, t_out = max_distance + pad;
            if (!rc_clip(o, d, lo, hi, t_in, t_out)) continue;
        }
        const int b1 = b0 + NT_MESH_TRIANGLE_BLOCK < ntri ? b0 + NT_MESH_TRIANGLE_BLOCK : ntri;
        for (int ti = b0; ti < b1; ++ti) {
            const int* idx = a.indices + 3 * (size_t)(t0 + ti);
            const int i0 = idx[0], i1 = idx[1], i2 = idx[2];
            if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) continue;
            float t;
            vec3 n;
            if (rc_triangle(o, d, cw_mul(rc_ld3(a.vertices + 3 * (size_t)(v0 + i0)), s), cw_mul(rc_ld3(a.vertices + 3 * (size_t)(v0 + i1)), s),
                            cw_mul(rc_ld3(a.vertices + 3 * (size_t)(v0 + i2)), s), t, n) &&
                t >= 0.0f && t <= max_distance && t < bt) {
                bt = t;
                bn = n;
            }
        }
    }
    if (bt < RC_INF) rc_offer(best, max_distance, bt, id, k, bn);
}

NT_DI int rc_cell(float x, int n) {  // floor, clamped to the cells 0 .. n - 1
    const float f = floorf(x);
    return f < 0.0f ? 0 : (f > (float)(n - 1) ? n - 1 : (int)f);
}

// heightfield shape `id`: the ray clipped to the field's box, then one slab of the faster grid axis after the other
NT_DI void rc_hfield(const nt_raycast_args& a, int id, int k, vec3 o, vec3 d, float max_distance, RcBest& best) {
    const int hi_ = a.shape_heightfield_index[id];
    if (hi_ < 0) return;
    const nt_heightfield hd = a.heightfields[hi_];
    const int ncx = hd.ncol - 1, ncy = hd.nrow - 1;
    if (ncx <= 0 || ncy <= 0) return;
    const float dx = 2.0f * hd.hx / (float)ncx, dy = 2.0f * hd.hy / (float)ncy, z_range = hd.max_z - hd.min_z;
    const float* e = a.elevations + hd.data_offset;
    const float eps = 1.0e-3f;  // in cells: far beyond the rounding of the cell coordinates, so that the walk never leaves out a hit
    const float pad_z = eps * fabsf(z_range) + 1.0e-6f;
    float t_a = 0.0f, t_b = max_distance;
    if (!rc_clip(o, d, vec3(-hd.hx - eps * dx, -hd.hy - eps * dy, fminw(hd.min_z, hd.max_z) - pad_z),
                 vec3(hd.hx + eps * dx, hd.hy + eps * dy, fmaxw(hd.min_z, hd.max_z) + pad_z), t_a, t_b))
        return;
    // cell coordinates along the ray: u(t) = u0 + du t (columns), v(t) = v0 + dv t (rows)
    const float u0 = (o.x + hd.hx) / dx, du = d.x / dx, v0 = (o.y + hd.hy) / dy, dv = d.y / dy;
    const bool major_u = fabsf(du) >= fabsf(dv);
    const float m0 = major_u ? u0 : v0, dm = major_u ? du : dv, n0 = major_u ? v0 : u0, dn = major_u ? dv : du;
    const int nm = major_u ? ncx : ncy, nn = major_u ? ncy : ncx;
    float bt = RC_INF;
    int btri = 0;
    vec3 bn;
    // (a ray that does not move along the grid, dm = 0: the one or two slabs it stands in)
    const int i_first = rc_cell(m0 + dm * t_a - (dm < 0.0f ? -eps : eps), nm), i_last = rc_cell(m0 + dm * t_b + (dm < 0.0f ? -eps : eps), nm);
    const int step = dm < 0.0f ? -1 : 1;
    for (int i = i_first; step > 0 ? i <= i_last : i >= i_last; i += step) {
        // the part of the ray inside slab i of the major axis
        float s_in = t_a, s_out = t_b;
        if (dm != 0.0f) {
            const float ta = ((float)i - eps - m0) / dm, tb = ((float)(i + 1) + eps - m0) / dm;
            s_in = fmaxw(s_in, fminw(ta, tb));
            s_out = fminw(s_out, fmaxw(ta, tb));
        }
        if (s_in <= s_out) {
            const float na = n0 + dn * s_in, nb = n0 + dn * s_out;
            const int j0 = rc_cell(fminw(na, nb) - eps, nn), j1 = rc_cell(fmaxw(na, nb) + eps, nn);
            for (int j = j0; j <= j1; ++j) {
                const int col = major_u ? i : j, row = major_u ? j : i;
                // get_triangle_shape_from_heightfield, as nt_mesh_triangle.hip builds the cell
                const float x0 = -hd.hx + (float)col * dx, x1 = x0 + dx, y0 = -hd.hy + (float)row * dy, y1 = y0 + dy;
                const float h00 = e[row * hd.ncol + col], h10 = e[row * hd.ncol + (col + 1)], h01 = e[(row + 1) * hd.ncol + col],
                            h11 = e[(row + 1) * hd.ncol + (col + 1)];
                const vec3 p00(x0, y0, hd.min_z + h00 * z_range), p10(x1, y0, hd.min_z + h10 * z_range), p01(x0, y1, hd.min_z + h01 * z_range),
                    p11(x1, y1, hd.min_z + h11 * z_range);
                for (int sub = 0; sub < 2; ++sub) {
                    const int tri = (row * ncx + col) * 2 + sub;
                    float t;
                    vec3 n;
                    if (rc_triangle(o, d, p00, sub == 0 ? p10 : p11, sub == 0 ? p11 : p01, t, n) && t >= 0.0f && t <= max_distance &&
                        (t < bt || (t == bt && tri < btri))) {
                        bt = t;
                        btri = tri;
                        bn = n;
                    }
                }
            }
            // a hit clearly before the end of this slab: no later slab holds a nearer one
            if (dm != 0.0f && bt + 1.0e-4f * (1.0f + fabsf(s_out)) < s_out) break;
        }
    }
    if (bt < RC_INF) rc_offer(best, max_distance, bt, id, k, bn);
}

__global__ void __launch_bounds__(RC_THREADS) raycast_kernel(nt_model m, const float* body_q, nt_raycast_args a, int wpb, int rl) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, K = a.target_count, R = a.ray_count;
    const size_t ES = (size_t)m.env_stride;
    const int groups = (m.env_count + wpb - 1) / wpb;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        __syncthreads();  // the previous group's records are no longer read
        // stage: one (world, target) per lane
        for (int item = tid; item < wpb * K; item += RC_THREADS) {
            const int wl = item / K, k = item - wl * K, e = g * wpb + wl;
            if (e >= m.env_count || (a.world_mask && !a.world_mask[e])) continue;
            const int slot = a.targets[2 * k], type = a.targets[2 * k + 1];
            float* rec = lds + (size_t)item * RC_REC;
            int* irec = reinterpret_cast<int*>(rec);  // words 10, 11: type, Newton shape id
            if (slot < 0 || slot >= m.ns + m.ng) { irec[10] = 0; irec[11] = -1; continue; }
            float sp[10];
            int id;
            if (slot < m.ns) {
                for (int c = 0; c < 10; ++c) sp[c] = m.shape_param[((size_t)c * m.ns + slot) * ES + e];
                id = m.shape_local0 + e * m.ns + slot;
            } else {
                for (int c = 0; c < 10; ++c) sp[c] = m.gshape_param[(size_t)(slot - m.ns) * NT_SHAPE_PARAM_FLOATS + c];
                id = m.gshape_id[slot - m.ns];
            }
            xform X(vec3(sp[0], sp[1], sp[2]), quat(sp[3], sp[4], sp[5], sp[6]));
            const int body = m.shape_body[slot];
            if (body >= 0 && body < m.nb) {
                const float* q = body_q + (size_t)body * ES + e;
                const size_t cs = (size_t)m.nb * ES;
                X = xform(vec3(q[0], q[cs], q[2 * cs]), quat(q[3 * cs], q[4 * cs], q[5 * cs], q[6 * cs])) * X;
            }
            rec[0] = X.p.x; rec[1] = X.p.y; rec[2] = X.p.z;
            rec[3] = X.q.x; rec[4] = X.q.y; rec[5] = X.q.z; rec[6] = X.q.w;
            rec[7] = sp[7]; rec[8] = sp[8]; rec[9] = sp[9];
            irec[10] = type;
            irec[11] = id;
        }
        __syncthreads();
        const int wl = tid / rl, e = g * wpb + wl;
        if (e >= m.env_count || (a.world_mask && !a.world_mask[e])) continue;
        const float* recs = lds + (size_t)wl * K * RC_REC;
        for (int r = tid - wl * rl; r < R; r += rl) {
            const size_t ray = a.rays_per_world ? (size_t)e * R + r : (size_t)r;
            vec3 O = rc_ld3(a.origins + 3 * ray), D = rc_ld3(a.directions + 3 * ray);
            const int rb = a.ray_body[r];
            bool live = rb >= -1 && rb < m.nb;
            if (rb >= 0 && live) {
                const float* q = body_q + (size_t)rb * ES + e;
                const size_t cs = (size_t)m.nb * ES;
                const xform X(vec3(q[0], q[cs], q[2 * cs]), quat(q[3 * cs], q[4 * cs], q[5 * cs], q[6 * cs]));
                O = xform_point(X, O);
                D = quat_rotate(X.q, D);
            }
            const float len = length(D);
            live = live && len > 0.0f;
            RcBest best;
            best.t = RC_INF; best.id = 0x7fffffff; best.k = -1;
            if (live) {
                D = D / len;
                for (int k = 0; k < K; ++k) {  // primitives, ascending slot
                    const float* rec = recs + (size_t)k * RC_REC;
                    const int type = reinterpret_cast<const int*>(rec)[10];
                    if (type == RC_MESH || type == RC_HFIELD || type == 0) continue;
                    const quat q(rec[3], rec[4], rec[5], rec[6]);
                    const vec3 o = quat_rotate_inv(q, O - vec3(rec[0], rec[1], rec[2])), d = quat_rotate_inv(q, D);
                    float t;
                    vec3 n;
                    if (rc_primitive(type, vec3(rec[7], rec[8], rec[9]), o, d, t, n)) rc_offer(best, a.max_distance, t, reinterpret_cast<const int*>(rec)[11], k, n);
                }
                for (int k = 0; k < K; ++k) {  // meshes and heightfields, ascending slot
                    const float* rec = recs + (size_t)k * RC_REC;
                    const int type = reinterpret_cast<const int*>(rec)[10];
                    if (type != RC_MESH && type != RC_HFIELD) continue;
                    const quat q(rec[3], rec[4], rec[5], rec[6]);
                    const vec3 o = quat_rotate_inv(q, O - vec3(rec[0], rec[1], rec[2])), d = quat_rotate_inv(q, D);
                    if (type == RC_MESH) rc_mesh(a, reinterpret_cast<const int*>(rec)[11], k, vec3(rec[7], rec[8], rec[9]), o, d, a.max_distance, best);
                    else rc_hfield(a, reinterpret_cast<const int*>(rec)[11], k, o, d, a.max_distance, best);
                }
            }
            const size_t out = (size_t)e * R + r;
            const bool hit = best.k >= 0;
            a.distance[out] = hit ? best.t : -1.0f;
            if (a.shape) a.shape[out] = hit ? best.id : -1;
            if (a.normal) {
                vec3 n;
                if (hit) {
                    const float* rec = recs + (size_t)best.k * RC_REC;
                    n = quat_rotate(quat(rec[3], rec[4], rec[5], rec[6]), normalize(best.n));
                }
                a.normal[3 * out] = n.x; a.normal[3 * out + 1] = n.y; a.normal[3 * out + 2] = n.z;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// nt_camera_render (newton_amd.sensors.SensorTiledCamera; contract: include/newton_hip_mesh.h): C cameras of W x H pixels per world.
//
// MI355X mapping.  A pixel is a ray of raycast_kernel -- the same rc_* functions called in the same order, so the same bits -- but
// the launch is shaped for images: one WAVE owns a block of 8 x 8 pixels (lane l at column l % 8, row l / 8), whose rays run through
// the same mesh blocks and heightfield cells together.  The 4 wave slots of a workgroup serve `wpb` = 4 / 2 / 1 worlds (B = 1 / 2 / more
// blocks per world) with spw = 4 / wpb slots each; a workgroup item is (group of wpb worlds, group of bpg * spw consecutive blocks):
// it stages the targets of its worlds once (raycast_kernel's 12-word records), then slot s of a world takes the blocks s, s + spw, ...
// of the group.  Origin, body and optical axis are one per camera: read and transformed once per block, not per ray.  With
// NT_CAMERA_CULL the wave first tests target lane, lane + 64, ... against the block's cone and ballots a wave-uniform survivor mask
// (one register pair for K <= 64, else 64-bit words per slot in LDS behind the records); both passes visit the set bits in ascending
// order, i.e. the survivors in raycast_kernel's order.  One lane produces every value of a pixel; no atomics, no cross-lane arithmetic.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int CAM_SLOTS = RC_THREADS / 64;  // wave slots per workgroup
constexpr int CAM_CONE = 5;                 // floats per block cone: axis[3], cos h, sin h
// The items the entry point aims for when it chooses blocks_per_group: 4 workgroups on each of the 256 CUs.
constexpr long long CAM_TARGET_ITEMS = 1024;
// Margin of the cone test, in metres: CAM_CULL_REL * (|centre - eye| + r) + CAM_CULL_ABS.  The test adds a handful of fp32 products
// of magnitude |centre - eye| (a cross product, two dot products, cos h and sin h rounded to fp32, the axis and the rays turned by
// the same body rotation): its rounding is a few 1e-7 of that distance, and so is the difference between the bounding radius taken
// here and the surface rc_primitive tests.  1e-3 relative sits three decades above that at every scene scale, and 1e-5 m keeps it
// there for a target at the eye.  It only ever keeps a target that a sharper test would drop.
constexpr float CAM_CULL_REL = 1.0e-3f, CAM_CULL_ABS = 1.0e-5f;

// the radius of a sphere about the staged origin that holds the primitive; false: unbounded (an infinite plane), never culled
NT_DI bool cam_bound(int type, vec3 s, float& r) {
    const vec3 a = vabs(s);
    if (type == RC_PLANE) {
        if (s.x == 0.0f && s.y == 0.0f) return false;
        r = sqrtf(a.x * a.x + a.y * a.y);
    } else if (type == RC_SPHERE) r = a.x;
    else if (type == RC_ELLIPSOID) r = fmaxw(fmaxw(a.x, a.y), a.z);
    else if (type == RC_BOX) r = length(a);
    else if (type == RC_CAPSULE) r = a.x + a.y;
    else if (type == RC_CYLINDER || type == RC_CONE) r = sqrtf(a.x * a.x + a.y * a.y);
    else return false;
    return true;
}

__global__ void __launch_bounds__(RC_THREADS) camera_kernel(nt_model m, const float* body_q, nt_camera_args a, nt_raycast_args tab, int wpb, int bpg) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, slot = tid >> 6, K = a.target_count;
    const size_t ES = (size_t)m.env_stride, cs = (size_t)m.nb * ES;
    const int W = a.width, H = a.height, bx = (W + NT_CAMERA_TILE - 1) / NT_CAMERA_TILE, per_cam = bx * ((H + NT_CAMERA_TILE - 1) / NT_CAMERA_TILE);
    const int B = a.camera_count * per_cam, spw = CAM_SLOTS / wpb, span = bpg * spw;
    const int block_groups = (B + span - 1) / span, world_groups = (m.env_count + wpb - 1) / wpb, words = (K + 63) / 64;
    // (K > 64 only) this slot's survivor words, behind the records: wpb * K * 48 bytes, a multiple of 16
    unsigned long long* mask_lds = reinterpret_cast<unsigned long long*>(lds + (size_t)wpb * K * RC_REC) + (size_t)slot * words;
    for (long long item = blockIdx.x; item < (long long)world_groups * block_groups; item += gridDim.x) {
        const int g = (int)(item / block_groups), bg = (int)(item - (long long)g * block_groups);
        __syncthreads();  // the previous item's records are no longer read
        // stage: one (world, target) per lane, as raycast_kernel does
        for (int it = tid; it < wpb * K; it += RC_THREADS) {
            const int wl = it / K, k = it - wl * K, e = g * wpb + wl;
            if (e >= m.env_count || (a.world_mask && !a.world_mask[e])) continue;
            const int tslot = a.targets[2 * k], type = a.targets[2 * k + 1];
            float* rec = lds + (size_t)it * RC_REC;
            int* irec = reinterpret_cast<int*>(rec);  // words 10, 11: type, Newton shape id
            if (tslot < 0 || tslot >= m.ns + m.ng) { irec[10] = 0; irec[11] = -1; continue; }
            float sp[10];
            int id;
            if (tslot < m.ns) {
                for (int c = 0; c < 10; ++c) sp[c] = m.shape_param[((size_t)c * m.ns + tslot) * ES + e];
                id = m.shape_local0 + e * m.ns + tslot;
            } else {
                for (int c = 0; c < 10; ++c) sp[c] = m.gshape_param[(size_t)(tslot - m.ns) * NT_SHAPE_PARAM_FLOATS + c];
                id = m.gshape_id[tslot - m.ns];
            }
            xform X(vec3(sp[0], sp[1], sp[2]), quat(sp[3], sp[4], sp[5], sp[6]));
            const int body = m.shape_body[tslot];
            if (body >= 0 && body < m.nb) {
                const float* q = body_q + (size_t)body * ES + e;
                X = xform(vec3(q[0], q[cs], q[2 * cs]), quat(q[3 * cs], q[4 * cs], q[5 * cs], q[6 * cs])) * X;
            }
            rec[0] = X.p.x; rec[1] = X.p.y; rec[2] = X.p.z;
            rec[3] = X.q.x; rec[4] = X.q.y; rec[5] = X.q.z; rec[6] = X.q.w;
            rec[7] = sp[7]; rec[8] = sp[8]; rec[9] = sp[9];
            irec[10] = type;
            irec[11] = id;
        }
        __syncthreads();
        const int wl = slot / spw, e = g * wpb + wl;  // (wave-uniform from here on)
        if (e >= m.env_count || (a.world_mask && !a.world_mask[e])) continue;
        const float* recs = lds + (size_t)wl * K * RC_REC;
        const int b_end = (bg + 1) * span < B ? (bg + 1) * span : B;
        for (int b = bg * span + (slot - wl * spw); b < b_end; b += spw) {
            const int cam = b / per_cam, bc = b - cam * per_cam, brow = bc / bx, bcol = bc - brow * bx;
            const int px = bcol * NT_CAMERA_TILE + (lane & (NT_CAMERA_TILE - 1)), py = brow * NT_CAMERA_TILE + lane / NT_CAMERA_TILE;
            const bool pixel = px < W && py < H;
            // the camera: one origin, body and optical axis for every ray of the block
            const int rb = a.ray_bodies[cam];
            const bool frame = rb >= -1 && rb < m.nb, attached = frame && rb >= 0;
            vec3 O = rc_ld3(a.ray_origins + 3 * (size_t)cam);
            xform X;
            if (attached) {
                const float* q = body_q + (size_t)rb * ES + e;
                X = xform(vec3(q[0], q[cs], q[2 * cs]), quat(q[3 * cs], q[4 * cs], q[5 * cs], q[6 * cs]));
                O = xform_point(X, O);
            }
            // survivors of the block: target lane, lane + 64, ... against the cone turned into the world
            const float* cone = a.block_cones + CAM_CONE * (size_t)b;
            const bool cull = (a.flags & NT_CAMERA_CULL) && cone[3] > 0.0f;
            vec3 A;
            float cos_h = 0.0f, sin_h = 0.0f;
            if (cull) {
                A = rc_ld3(cone);
                if (attached) A = quat_rotate(X.q, A);
                cos_h = cone[3];
                sin_h = cone[4];
            }
            unsigned long long mask0 = 0ull;
            int count = 0;
            for (int w = 0; w < words; ++w) {
                const int k = w * 64 + lane;
                bool keep = false;
                if (k < K) {
                    const float* rec = recs + (size_t)k * RC_REC;
                    const int type = reinterpret_cast<const int*>(rec)[10];
                    keep = type != 0;
                    float r;
                    if (keep && cull && cam_bound(type, vec3(rec[7], rec[8], rec[9]), r)) {
                        // distance from the centre to the cone's mantle line (never more than to the cone itself) against r + margin
                        const vec3 v = vec3(rec[0], rec[1], rec[2]) - O;
                        keep = !(length(cross(v, A)) * cos_h - dot(v, A) * sin_h > r + (CAM_CULL_REL * (length(v) + r) + CAM_CULL_ABS));
                    }
                }
                const unsigned long long mw = __ballot(keep);
                if (K <= 64) mask0 = mw;
                else mask_lds[w] = mw;  // (every lane of the wave stores the same word and reads its own store)
                count += __popcll(mw);
            }
            if (a.survivors && lane == 0) a.survivors[(size_t)e * B + b] = count;
            if (!pixel) continue;  // (no wave-level operation below)
            vec3 D = rc_ld3(a.ray_directions + 3 * ((size_t)cam * H * W + (size_t)py * W + px));
            if (attached) D = quat_rotate(X.q, D);
            const float len = length(D);
            const bool live = frame && len > 0.0f;
            RcBest best;
            best.t = RC_INF; best.id = 0x7fffffff; best.k = -1;
            if (live) {
                D = D / len;
                for (int w = 0; w < words; ++w) {  // primitives, ascending slot
                    for (unsigned long long mm = K <= 64 ? mask0 : mask_lds[w]; mm; mm &= mm - 1) {
                        const int k = w * 64 + __ffsll((long long)mm) - 1;
                        const float* rec = recs + (size_t)k * RC_REC;
                        const int type = reinterpret_cast<const int*>(rec)[10];
                        if (type == RC_MESH || type == RC_HFIELD || type == 0) continue;
                        const quat q(rec[3], rec[4], rec[5], rec[6]);
                        const vec3 o = quat_rotate_inv(q, O - vec3(rec[0], rec[1], rec[2])), d = quat_rotate_inv(q, D);
                        float t;
                        vec3 n;
                        if (rc_primitive(type, vec3(rec[7], rec[8], rec[9]), o, d, t, n)) rc_offer(best, a.max_distance, t, reinterpret_cast<const int*>(rec)[11], k, n);
                    }
                }
                for (int w = 0; w < words; ++w) {  // meshes and heightfields, ascending slot
                    for (unsigned long long mm = K <= 64 ? mask0 : mask_lds[w]; mm; mm &= mm - 1) {
                        const int k = w * 64 + __ffsll((long long)mm) - 1;
                        const float* rec = recs + (size_t)k * RC_REC;
                        const int type = reinterpret_cast<const int*>(rec)[10];
                        if (type != RC_MESH && type != RC_HFIELD) continue;
                        const quat q(rec[3], rec[4], rec[5], rec[6]);
                        const vec3 o = quat_rotate_inv(q, O - vec3(rec[0], rec[1], rec[2])), d = quat_rotate_inv(q, D);
                        if (type == RC_MESH) rc_mesh(tab, reinterpret_cast<const int*>(rec)[11], k, vec3(rec[7], rec[8], rec[9]), o, d, a.max_distance, best);
                        else rc_hfield(tab, reinterpret_cast<const int*>(rec)[11], k, o, d, a.max_distance, best);
                    }
                }
            }
            const size_t out = (((size_t)e * a.camera_count + cam) * H + py) * W + px;
            const bool hit = best.k >= 0;
            a.distance[out] = hit ? best.t : -1.0f;
            if (a.depth) {
                vec3 F = rc_ld3(a.forward + 3 * (size_t)cam);
                if (attached) F = quat_rotate(X.q, F);
                a.depth[out] = hit ? best.t * dot(D, F) : -1.0f;
            }
            if (a.shape) a.shape[out] = hit ? best.id : -1;
            if (a.normal) {
                vec3 n;
                if (hit) {
                    const float* rec = recs + (size_t)best.k * RC_REC;
                    n = quat_rotate(quat(rec[3], rec[4], rec[5], rec[6]), normalize(best.n));
                }
                a.normal[3 * out] = n.x; a.normal[3 * out + 1] = n.y; a.normal[3 * out + 2] = n.z;
            }
        }
    }
}

}  // namespace

extern "C" nt_status nt_mesh_plane_pairs(const nt_mesh_plane_args* a, void* stream) {
    if (!a || !a->pairs || !a->shape_type || !a->shape_transform || !a->shape_data || !a->shape_gap || !a->shape_vertex_range ||
        !a->vertices || !a->out_count || !a->out_pair || !a->out_key || !a->out_data || !a->out_blk || a->capacity < 0)
        return NT_ERR_INVALID_ARG;
    if (a->reduce && (!a->shape_aabb_lower || !a->shape_aabb_upper || !a->shape_voxel_res)) return NT_ERR_INVALID_ARG;
    if (a->pair_world_prefix ? (a->worlds <= 0 || a->pairs_per_world <= 0) : a->pair_count < 0) return NT_ERR_INVALID_ARG;
    long long blocks = a->pair_world_prefix ? (long long)a->worlds * a->pairs_per_world : (long long)a->pair_count;
    if (blocks == 0) return NT_OK;
#ifdef NT_EMULATED_GRID
    const long long grid_cap = NT_EMULATED_GRID;
#else
    const long long grid_cap = 8192;
#endif
    if (blocks > grid_cap) blocks = grid_cap;
    hipLaunchKernelGGL(mesh_plane_pairs_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

extern "C" nt_status nt_raycast(const nt_model* m, const nt_state* s, const nt_raycast_args* a, void* stream) {
    if (!m || !s || !a || !s->body_q || !a->origins || !a->directions || !a->ray_body || !a->distance || a->ray_count <= 0 ||
        a->target_count < 0 || !(a->max_distance >= 0.0f) || m->env_count <= 0 || m->env_stride < m->env_count || m->nb <= 0 || m->ns < 0 || m->ng < 0)
        return NT_ERR_INVALID_ARG;
    const int K = a->target_count;
    if (K > 0 && (!a->targets || !a->targets_host || !m->shape_body || (m->ns > 0 && !m->shape_param) || (m->ng > 0 && (!m->gshape_param || !m->gshape_id))))
        return NT_ERR_INVALID_ARG;
    bool mesh = false, hfield = false, unsupported = false;
    for (int k = 0, prev = -1; k < K; ++k) {
        const int slot = a->targets_host[2 * k], type = a->targets_host[2 * k + 1];
        if (slot <= prev || slot >= m->ns + m->ng) return NT_ERR_INVALID_ARG;
        prev = slot;
        mesh = mesh || type == RC_MESH;
        hfield = hfield || type == RC_HFIELD;
        unsupported = unsupported || !(type == RC_PLANE || type == RC_HFIELD || type == RC_SPHERE || type == RC_CAPSULE || type == RC_ELLIPSOID ||
                                       type == RC_CYLINDER || type == RC_BOX || type == RC_MESH || type == RC_CONE);
    }
    if (mesh && (!a->shape_vertex_range || !a->shape_triangle_range || !a->vertices || !a->indices)) return NT_ERR_INVALID_ARG;
    if ((a->block_bounds != nullptr) != (a->shape_block_start != nullptr)) return NT_ERR_INVALID_ARG;
    if (hfield && (!a->shape_heightfield_index || !a->heightfields || !a->elevations)) return NT_ERR_INVALID_ARG;
    if (unsupported) return NT_ERR_UNSUPPORTED;
    // worlds per workgroup: four / two while the rays of a world leave lanes idle and the staged targets still fit the CU
    int wpb = a->ray_count <= 64 ? 4 : (a->ray_count <= 128 ? 2 : 1);
    const size_t per_world = (size_t)K * RC_REC * sizeof(float);
    while (wpb > 1 && wpb * per_world > RC_LDS_BYTES_PER_CU) wpb /= 2;
    if (per_world > RC_LDS_BYTES_PER_CU) return NT_ERR_UNSUPPORTED;
    const size_t lds_bytes = wpb * per_world > 16 ? wpb * per_world : 16;
#ifdef NT_EMULATED_GRID
    const long long grid_cap = NT_EMULATED_GRID;
#else
    const long long grid_cap = 8192;
#endif
    long long blocks = ((long long)m->env_count + wpb - 1) / wpb;
    if (blocks > grid_cap) blocks = grid_cap;
    if (lds_bytes > 48 * 1024 &&
        hipFuncSetAttribute((const void*)raycast_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return NT_ERR_LAUNCH;
    hipLaunchKernelGGL(raycast_kernel, dim3((unsigned)blocks), dim3(RC_THREADS), lds_bytes, (hipStream_t)stream, *m, (const float*)s->body_q, *a, wpb,
                       RC_THREADS / wpb);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}

extern "C" nt_status nt_camera_render(const nt_model* m, const nt_state* s, const nt_camera_args* a, void* stream) {
    if (!m || !s || !a || !s->body_q || !a->ray_origins || !a->ray_bodies || !a->ray_directions || !a->forward || !a->distance ||
        a->camera_count <= 0 || a->width <= 0 || a->height <= 0 || a->target_count < 0 || !(a->max_distance >= 0.0f) || a->blocks_per_group < 0 ||
        ((a->flags & NT_CAMERA_CULL) && !a->block_cones) || m->env_count <= 0 || m->env_stride < m->env_count || m->nb <= 0 || m->ns < 0 || m->ng < 0)
        return NT_ERR_INVALID_ARG;
    const int K = a->target_count;
    if (K > 0 && (!a->targets || !a->targets_host || !m->shape_body || (m->ns > 0 && !m->shape_param) || (m->ng > 0 && (!m->gshape_param || !m->gshape_id))))
        return NT_ERR_INVALID_ARG;
    bool mesh = false, hfield = false, unsupported = false;
    for (int k = 0, prev = -1; k < K; ++k) {
        const int slot = a->targets_host[2 * k], type = a->targets_host[2 * k + 1];
        if (slot <= prev || slot >= m->ns + m->ng) return NT_ERR_INVALID_ARG;
        prev = slot;
        mesh = mesh || type == RC_MESH;
        hfield = hfield || type == RC_HFIELD;
        unsupported = unsupported || !(type == RC_PLANE || type == RC_HFIELD || type == RC_SPHERE || type == RC_CAPSULE || type == RC_ELLIPSOID ||
                                       type == RC_CYLINDER || type == RC_BOX || type == RC_MESH || type == RC_CONE);
    }
    if (mesh && (!a->shape_vertex_range || !a->shape_triangle_range || !a->vertices || !a->indices)) return NT_ERR_INVALID_ARG;
    if ((a->block_bounds != nullptr) != (a->shape_block_start != nullptr)) return NT_ERR_INVALID_ARG;
    if (hfield && (!a->shape_heightfield_index || !a->heightfields || !a->elevations)) return NT_ERR_INVALID_ARG;
    if (unsupported) return NT_ERR_UNSUPPORTED;
    const long long B = (long long)a->camera_count * ((a->width + NT_CAMERA_TILE - 1) / NT_CAMERA_TILE) * ((a->height + NT_CAMERA_TILE - 1) / NT_CAMERA_TILE);
    if (B > 0x7fffffffLL / 64) return NT_ERR_INVALID_ARG;
    // worlds per workgroup: a world with one / two blocks needs one / two of the four wave slots, while the staged targets fit the CU
    int wpb = B == 1 ? 4 : (B == 2 ? 2 : 1);
    const size_t per_world = (size_t)K * RC_REC * sizeof(float), mask_bytes = K > 64 ? (size_t)CAM_SLOTS * ((K + 63) / 64) * 8 : 0;
    while (wpb > 1 && wpb * per_world + mask_bytes > RC_LDS_BYTES_PER_CU) wpb /= 2;
    if (per_world + mask_bytes > RC_LDS_BYTES_PER_CU) return NT_ERR_UNSUPPORTED;
    const size_t lds_bytes = wpb * per_world + mask_bytes > 16 ? wpb * per_world + mask_bytes : 16;
    // blocks per slot and item: a world's blocks are cut into as many groups as it takes to reach CAM_TARGET_ITEMS items (few worlds
    // with large images fill the machine), and into ONE group once the worlds alone reach it (many worlds stage their targets once)
    const int spw = CAM_SLOTS / wpb;
    const long long world_groups = ((long long)m->env_count + wpb - 1) / wpb, per_slot = (B + spw - 1) / spw;
    int bpg = a->blocks_per_group;
    if (bpg == 0) {
        long long cuts = (CAM_TARGET_ITEMS + world_groups - 1) / world_groups;
        cuts = cuts < 1 ? 1 : (cuts > per_slot ? per_slot : cuts);
        bpg = (int)((per_slot + cuts - 1) / cuts);
    }
    if (bpg > per_slot) bpg = (int)per_slot;
#ifdef NT_EMULATED_GRID
    const long long grid_cap = NT_EMULATED_GRID;
#else
    const long long grid_cap = 8192;
#endif
    long long blocks = world_groups * ((B + (long long)bpg * spw - 1) / ((long long)bpg * spw));
    if (blocks > grid_cap) blocks = grid_cap;
    if (lds_bytes > 48 * 1024 &&
        hipFuncSetAttribute((const void*)camera_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return NT_ERR_LAUNCH;
    nt_raycast_args tab = {};  // the mesh / heightfield tables in the shape rc_mesh / rc_hfield read them
    tab.shape_vertex_range = a->shape_vertex_range; tab.shape_triangle_range = a->shape_triangle_range;
    tab.vertices = a->vertices; tab.indices = a->indices;
    tab.block_bounds = a->block_bounds; tab.shape_block_start = a->shape_block_start;
    tab.shape_heightfield_index = a->shape_heightfield_index; tab.heightfields = a->heightfields; tab.elevations = a->elevations;
    hipLaunchKernelGGL(camera_kernel, dim3((unsigned)blocks), dim3(RC_THREADS), lds_bytes, (hipStream_t)stream, *m, (const float*)s->body_q, *a, tab, wpb, bpg);
    return hipGetLastError() == hipSuccess ? NT_OK : NT_ERR_LAUNCH;
}
