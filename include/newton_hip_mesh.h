/* newton_hip_mesh.h -- mesh legs of CollisionPipeline.collide that work on mesh VERTICES (extension of newton_hip.h).
 *
 * Reference interface replaced (paths relative to /root/reference/newton/_src/geometry):
 *   pair routing        narrow_phase.py:618-631   a MESH against an INFINITE plane (scale x = y = 0) leaves the primitive / GJK
 *                                                 path for `shape_pairs_mesh_plane`, stored as (mesh, plane)
 *   contact generation  narrow_phase.py:1744-1992 narrow_phase_process_mesh_plane_contacts(_reduce)_kernel: one lane per mesh
 *                                                 vertex -- world position, projection on the plane through the plane's frame,
 *                                                 distance = (v - proj) . n, admitted when distance < gap sum + margin sum,
 *                                                 contact centre = midpoint, normal = -n (mesh -> plane), sort_sub_key = vertex
 *   reduction           contact_reduction_global.py:2059-2096 write_contact_to_reducer, :1246-1346 reduce_contact_in_hashtable
 *                                                 (the BUFFERED variant: uncentred projection, directional slots only for
 *                                                 depth < 1e-4 |aabb(mesh)|, max-depth and voxel slots for every contact),
 *                                                 :2098-2290 export_reduced_contacts_kernel
 * Output = ContactData rows in the form nt_mesh_sdf_collide_reduced emits them (newton_hip.h): one contiguous block per pair,
 * rows in ascending vertex order -- what nt_sdf_rows_finalize / nt_contact_rows_write turn into Newton's contact arrays.
 * Same conventions as newton_hip.h: device pointers owned by the caller, work enqueued on `stream`, no allocation. */
#ifndef NEWTON_HIP_MESH_H
#define NEWTON_HIP_MESH_H

#include "newton_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t* pairs;                    /* [pair_count][2] shape ids, or the per-world candidate regions [worlds * pairs_per_world][2]
                                          of nt_sdf_candidate_pairs; rewritten in place as (mesh, plane) for the pairs processed */
    int32_t pair_count;                /* plain list: number of pairs (pair_world_prefix == NULL) */
    const int32_t* pair_world_prefix;  /* [worlds + 1] exclusive prefix of the live pairs per world, or NULL for a plain list */
    int32_t worlds, pairs_per_world;
    const uint8_t* pair_kind;          /* [pairs] or NULL: when given only pairs of kind NT_PAIR_KIND_MESH_PLANE are processed */
    const int32_t* shape_type;         /* [S] GeoType (PLANE = 1, MESH = 8): which shape of a pair is the plane */
    const float* shape_transform;      /* [S][7] world transforms */
    const float* shape_data;           /* [S][4] scale xyz, margin */
    const float* shape_gap;            /* [S] */
    const int32_t* shape_vertex_range; /* [S][2] (first vertex, vertex count) of a mesh shape in `vertices` */
    const float* vertices;             /* [V][3] mesh-local, unscaled (wp.Mesh.points) */
    const float* shape_aabb_lower;     /* [S][3] Model.shape_collision_aabb_lower / _upper: the mesh's scaled local AABB */
    const float* shape_aabb_upper;
    const int32_t* shape_voxel_res;    /* [S][3] Model.shape_voxel_resolution */
    int32_t reduce;                    /* 1: the global contact reduction (CollisionPipeline default); 0: every admitted vertex */
    int32_t* out_count;                /* [1] rows appended so far (the caller sets the start; keeps counting past capacity) */
    int32_t* out_pair;                 /* [capacity] pair position of the row */
    int32_t* out_key;                  /* [capacity] vertex index (ContactData.sort_sub_key) */
    float* out_data;                   /* [capacity][9] centre, normal mesh -> plane, distance, margin mesh, margin plane */
    int32_t capacity;
    int32_t* out_blk;                  /* [pairs][2] (first row, row count) of the pair's block; written for every processed pair */
} nt_mesh_plane_args;
#define NT_PAIR_KIND_MESH_PLANE 2      /* nt_sdf_scene.template_kind / world_pair_kind: 0 mesh-SDF edges, 1 hydroelastic */
nt_status nt_mesh_plane_pairs(const nt_mesh_plane_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * The triangle leg: a MESH that does not take the SDF route against a convex primitive (sphere, capsule, ellipsoid, cylinder, box,
 * cone) or a convex hull (CONVEX_MESH).  Reference interface replaced (paths relative to /root/reference/newton/_src/geometry):
 *   pair routing        narrow_phase.py:633-638    `shape_pairs_mesh`: a mesh against a non-mesh shape that took no earlier route
 *   midphase            narrow_phase.py:1455-1568 narrow_phase_find_mesh_triangle_overlaps_kernel -> collision_core.py:996-1180
 *                                                 (query AABB from the convex shape's support function in the unscaled mesh frame,
 *                                                 widened by (margin + gap) / |scale|; mesh BVH query; front-face test)
 *   contact generation  contact_reduction_global.py:2299-2403 mesh_triangle_contacts_to_reducer_kernel (reduce_contacts=True) and
 *                                                 narrow_phase.py:1571-1665 (reduce_contacts=False): world-space triangle, back-face
 *                                                 culling, GJK / MPR + manifold with GeoTypeEx.TRIANGLE as shape A,
 *                                                 sort_sub_key = (((triangle << 1) | 1) << 3) | manifold index
 *   reduction           contact_reduction_global.py:2059-2096, :1246-1346, :2098-2290 (the buffered variant, as nt_mesh_plane_pairs)
 * The BVH is replaced by a scan over the mesh's triangles (same candidate set: every triangle whose float32 bounds touch the query
 * box).  Output = ContactData rows like nt_mesh_plane_pairs: one contiguous block per pair, rows in ascending sort_sub_key order;
 * under `reduce` they are the reducer's survivors BEFORE the writer's gap test (nt_sdf_rows_finalize / nt_contact_rows_write apply
 * it, with the effective radii of `out_radius`), without it every generated contact.
 * --------------------------------------------------------------------------------------------------------------------------- */
/* HeightfieldData (newton/_src/utils/heightfield.py:141-156): a grid of nrow x ncol normalised elevations in [0, 1] at
 * `elevations[data_offset + row * ncol + col]`, spanning [-hx, hx] x [-hy, hy], world z = min_z + h (max_z - min_z). */
typedef struct {
    int32_t data_offset, nrow, ncol;
    float hx, hy, min_z, max_z;
} nt_heightfield;
typedef struct {
    int32_t* pairs;                    /* as nt_mesh_plane_args.pairs; rewritten in place as (mesh, convex) for the pairs processed */
    int32_t pair_count;
    const int32_t* pair_world_prefix;  /* [worlds + 1] or NULL for a plain list */
    int32_t worlds, pairs_per_world;
    const uint8_t* pair_kind;          /* [pairs] or NULL: when given only pairs of kind NT_PAIR_KIND_MESH_TRIANGLE are processed */
    const int32_t* shape_type;         /* [S] GeoType (MESH = 8; the partner: SPHERE 3, CAPSULE 4, ELLIPSOID 5, CYLINDER 6, BOX 7, CONE 9,
                                          CONVEX_MESH 10 with `hull_points`) */
    const float* shape_transform;      /* [S][7] world transforms */
    const float* shape_data;           /* [S][4] scale xyz, margin */
    const float* shape_gap;            /* [S] */
    const int32_t* shape_vertex_range; /* [S][2] (first vertex, vertex count) of a mesh shape in `vertices` */
    const int32_t* shape_triangle_range; /* [S][2] (first triangle, triangle count < 2^18) of a mesh shape in `indices` */
    const float* vertices;             /* [V][3] mesh-local, unscaled (wp.Mesh.points) */
    const int32_t* indices;            /* [T][3] vertex ids relative to the shape's first vertex (wp.Mesh.indices) */
    const float* shape_aabb_lower;     /* [S][3] Model.shape_collision_aabb_lower / _upper (reduce: the mesh's scaled local AABB) */
    const float* shape_aabb_upper;
    const int32_t* shape_voxel_res;    /* [S][3] Model.shape_voxel_resolution (reduce) */
    int32_t reduce;                    /* 1: the global contact reduction (CollisionPipeline default); 0: every generated contact */
    int32_t* out_count;                /* [1] rows appended so far (the caller sets the start; keeps counting past capacity) */
    int32_t* out_pair;                 /* [capacity] pair position of the row */
    int32_t* out_key;                  /* [capacity] sort_sub_key of the contact */
    float* out_data;                   /* [capacity][9] centre, normal mesh -> convex, distance, margin mesh, margin convex */
    float* out_radius;                 /* [capacity][2] or NULL: effective radii (0, sphere / capsule radius) of the export */
    int32_t capacity;
    int32_t* out_blk;                  /* [pairs][2] (first row, row count) of the pair's block; written for every processed pair */
    const float* block_bounds;         /* [blocks][6] or NULL: (lower xyz, upper xyz) of the unscaled vertices of every block of
                                          NT_MESH_TRIANGLE_BLOCK consecutive triangles of a mesh (the last block of a mesh is short);
                                          the scan skips blocks that miss the query box -- same candidate set, fewer rounds */
    const int32_t* shape_block_start;  /* [S] or NULL (both or neither): first block of a mesh shape in `block_bounds` */
    const float* hull_points;          /* [H][3] or NULL: vertex tables of the CONVEX_MESH partners (wp.Mesh.points of a hull, unscaled;
                                          Model.mesh_points); without it pairs with a CONVEX_MESH are skipped */
    const int32_t* shape_hull_range;   /* [S][2] or NULL (both or neither): (first vertex, vertex count) of a CONVEX_MESH shape */
    /* heightfields (GeoType.HFIELD = 2) as the mesh-like shape of a pair: narrow_phase.py:553-583 routes (heightfield, convex) pairs to
     * the same triangle kernels -- heightfield_vs_convex_midphase (utils/heightfield.py:366-462: the partner's LOCAL AABB
     * `shape_aabb_lower / _upper` as an oriented box in the heightfield frame -> a cell range, two triangles per cell) and
     * get_triangle_shape_from_heightfield (:280-363: GeoTypeEx.TRIANGLE_PRISM, the triangle extruded 1 m along the field's -Z, MPR /
     * GJK in the heightfield frame; penetrating contacts move to the physical face, collision_core.py:280-322).
     * sort_sub_key = ((((row * (ncol - 1) + col) * 2 + tri_sub) << 1 | 1) << 3) | manifold index; 2 (nrow - 1)(ncol - 1) < 2^18.
     * All three NULL: no heightfield pairs (they are skipped); the mesh tables may be NULL when only heightfields collide. */
    const int32_t* shape_heightfield_index; /* [S] index into `heightfields`, -1 for other shapes (Model.shape_heightfield_index) */
    const nt_heightfield* heightfields;     /* [H] */
    const float* elevations;                /* concatenated normalised elevation grids */
} nt_mesh_triangle_args;
#define NT_MESH_TRIANGLE_BLOCK 64
#define NT_PAIR_KIND_MESH_TRIANGLE 3
nt_status nt_mesh_triangle_pairs(const nt_mesh_triangle_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * nt_raycast: R rays per world against the shapes of that world, one launch (newton_amd.sensors.SensorRaycast; the capability of
 * the reference's newton.sensors.SensorRaycast, which is ONE camera -- here one sensor per world of the batched layout).
 *
 * Rays.  Ray r is an origin o_r, a direction d_r and a frame ray_body[r]: an env-local body index, or -1 for the world frame.  With
 * (p, q) = body_q[ray_body[r]] of the world: O = p + rot(q, o_r), D = normalize(rot(q, d_r)) (world frame: O = o_r, D = normalize(d_r)).
 * A direction of length 0 is a miss, and so is a ray_body outside -1 .. nb - 1.  Only nt_state.body_q is read.  origins / directions
 * are one [R][3] pattern shared by every world (rays_per_world = 0) or [env_count][R][3] (rays_per_world = 1); they are read through
 * the pointers at launch time, so an in-place update followed by a graph replay takes effect (the convention of nt_ik_solve's targets).
 *
 * Targets.  An env-uniform selection of the ns + ng shape slots (env-local shapes, then global shapes).  The byte mask of the Python
 * interface arrives as the ascending list of the selected slots with their GeoType: `targets` [target_count][2] = (slot, type) in
 * device memory, and `targets_host`, the same table in host memory -- the entry point does not synchronise, so what it checks before
 * the launch (slots ascending and inside 0 .. ns + ng - 1, supported types, the LDS fit) it checks on the host copy.  The type is
 * Model.shape_type: MESH and HFIELD are named as such (nt_model.shape_type folds both into CONVEX_MESH for the tiles).  The pose of a
 * shape is body_q[shape_body] * shape xform (shape_param rows 0..6; global shapes: gshape_param), its scale comes from the same tables.
 *
 * Only surfaces that FACE the ray count: with the outward unit normal n at the hit, a hit needs n . D < 0 and 0 <= t <= max_distance.
 * An origin inside a closed shape does not hit that shape; mesh triangles are back-face culled by winding; a heightfield is hit on
 * its top surface only; a plane from its front side only.  In the shape frame (o, d):
 *   PLANE      z = 0, n = +z.  Infinite when scale x = y = 0 (the routing rule above), else |x| <= scale x, |y| <= scale y.
 *   SPHERE, ELLIPSOID   radii scale xyz (sphere: scale x three times).  Cast in the space scaled to the unit sphere: o / radii, d / radii
 *              (t is unchanged), the ray moved to its point nearest the centre first, disc = 1 - |c|^2 > 0 (a tangent ray misses);
 *              n = normalize(p_unit / radii), the inverse-transpose scale.
 *   BOX        half extents scale xyz: slab test from the ray's point nearest the centre, n = the entered face (first axis on a tie);
 *              needs t_enter < t_exit, and |c| < half extent on an axis with a zero direction component: a ray that only touches
 *              the box (through an edge, or inside a face plane) misses, like the tangent to a sphere.
 *   CAPSULE    radius scale x, half height scale y along z (nt_primitives.hpp / nt_convex.hpp): the entering root on the infinite
 *              cylinder (2-D, from the point nearest the axis); |z| <= half height there: the lateral surface, else the hemisphere
 *              of that end.  A ray parallel to the axis takes the hemisphere it runs towards.
 *   CYLINDER   the same lateral surface; beyond the ends the cap disc z = +-half height, x^2 + y^2 <= r^2.  Straight cylinders only
 *              (scale z, the barrel radius, = 0): the scale is per-world device data the entry point cannot see, the caller vouches
 *              (SensorRaycast checks the host model and refuses a barrel).
 *   CONE       apex at z = +half height, base radius scale x at z = -half height: x^2 + y^2 = (k w)^2, k = r / (2 h), w = h - z in
 *              (0, 2 h], n = (x, y, k^2 w), roots by the cancellation-free form q = -(B + sign(B) sqrt(B^2 - A C)), t = q / A, C / q;
 *              and the base disc.  The nearest facing candidate.
 *   MESH       every triangle of shape_triangle_range, vertices times shape scale, Moeller-Trumbore in fp32 in the mesh frame,
 *              det = e1 . (d x e2) > 0 (front face by winding), 0 <= u, 0 <= v, u + v <= det.  With block_bounds, blocks of
 *              NT_MESH_TRIANGLE_BLOCK triangles whose (padded) box the ray misses are skipped: the same hit set.
 *   HFIELD     the two triangles per cell of the triangle leg (tri_sub 0 = (p00, p10, p11), 1 = (p00, p11, p01); index
 *              (row (ncol - 1) + col) 2 + tri_sub), the same test.  The ray is clipped to the field's box and the cells are visited
 *              by a 2-D walk along the ray: one slab of the faster grid axis after the other, the one to three cells the ray can touch
 *              in it; the walk ends once a hit lies before the end of the slab.  The shape scale is not applied (as in the triangle leg).
 * CONVEX_MESH (the model stores vertices only), GAUSSIAN and barrel cylinders are no ray targets: NT_ERR_UNSUPPORTED.
 *
 * Result per (world, ray): the nearest hit; a tie in t goes to the lower Newton shape id, within one mesh / heightfield to the lower
 * triangle index.  distance [env_count][R]: t, or -1 for a miss; normal [env_count][R][3] (or NULL): unit, world frame, zeros on a
 * miss; shape [env_count][R] (or NULL): the Newton shape id, or -1.  world_mask ([env_count] bytes or NULL): rows of unselected worlds
 * are neither computed nor written.  Every value is produced by ONE lane, which visits the targets in ascending slot order
 * (primitives, then meshes and heightfields) and the triangles of a mesh in ascending index; IEEE arithmetic, no atomics: identical
 * worlds give identical bits, and the result does not depend on the launch geometry.
 *
 * Same conventions as newton_hip.h: device pointers owned by the caller, no allocation, no synchronisation, recordable by
 * nt_graph_capture_begin / _end.  Errors: null model / state / args / body_q / rays / distance / target tables, ray_count <= 0,
 * target_count < 0, a MESH or HFIELD target without its tables: NT_ERR_INVALID_ARG; a target list that is not ascending or leaves the
 * slots: NT_ERR_INVALID_ARG; an unsupported target type, or staged targets (48 bytes each per world) beyond the CU's LDS:
 * NT_ERR_UNSUPPORTED.
 * --------------------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t ray_count;                 /* R, rays per world */
    int32_t rays_per_world;            /* 0: origins / directions are [R][3], shared; 1: [env_count][R][3] */
    const float* origins;
    const float* directions;
    const int32_t* ray_body;           /* [R] env-local body index or -1 (world frame) */
    float max_distance;
    int32_t target_count;              /* K selected shape slots */
    const int32_t* targets;            /* DEVICE [K][2] (slot, GeoType), ascending slot */
    const int32_t* targets_host;       /* HOST   [K][2] the same table (checked before the launch) */
    const uint8_t* world_mask;         /* [env_count] or NULL */
    float* distance;                   /* [env_count][R] */
    float* normal;                     /* [env_count][R][3] or NULL */
    int32_t* shape;                    /* [env_count][R] or NULL */
    /* mesh / heightfield tables, indexed by Newton shape id, field meanings of nt_mesh_triangle_args; NULL when no target needs them */
    const int32_t* shape_vertex_range;
    const int32_t* shape_triangle_range;
    const float* vertices;
    const int32_t* indices;
    const float* block_bounds;         /* or NULL: no block skipping */
    const int32_t* shape_block_start;  /* (both or neither) */
    const int32_t* shape_heightfield_index;
    const nt_heightfield* heightfields;
    const float* elevations;
} nt_raycast_args;
nt_status nt_raycast(const nt_model* m, const nt_state* s, const nt_raycast_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * nt_camera_render: C cameras of width x height pixels in every world, one launch (newton_amd.sensors.SensorTiledCamera; the
 * capability of the reference's newton.sensors.SensorTiledCamera without its colour image -- the model carries no shape colours).
 *
 * A pixel is a ray of nt_raycast, and everything that comment says about rays, targets, the per-type surfaces, the facing and tie
 * rules and the error codes holds here word for word; only how the rays are stored differs.  Camera c has ONE origin ray_origins[c]
 * and ONE frame ray_bodies[c] (env-local body or -1, the same in every world) and a table ray_directions[c][H * W][3] in that frame,
 * row-major with row 0 at the top of the image; the directions need not be unit.  distance / normal / shape of pixel (c, i, j) of a
 * world are, BIT FOR BIT, what nt_raycast gives for origin ray_origins[c], direction ray_directions[c][i * W + j] and ray_body
 * ray_bodies[c] against the same targets and max_distance: the same per-ray instructions in the same order, one lane per pixel.
 * depth (or NULL) = t * (D . F), D the unit world direction of the pixel and F = forward[c] turned by the body's rotation (forward:
 * the unit optical axis in the frame of ray_bodies[c]); -1 on a miss.  Outputs are [env_count][C][H][W] (normal: ...[3]).
 *
 * Launch shape.  The unit of work is a block of 8 x 8 pixels on one wave (lane l at column l % 8, row l / 8 of the block); the blocks
 * of a world are numbered over camera, block row, block column: B = C * ceil(H / 8) * ceil(W / 8).  A workgroup has four wave slots
 * and serves 4 / 2 / 1 worlds for B = 1 / 2 / more (halved while the staged targets do not fit the LDS), i.e. 1 / 2 / 4 slots per
 * world.  blocks_per_group > 0: every slot takes that many blocks per workgroup item (an item stages its worlds' targets once);
 * 0: the entry point chooses.  No output bit depends on it.
 *
 * Culling (flags bit 0).  block_cones [C][ceil(H / 8) * ceil(W / 8)][5] = (unit axis in the frame of ray_bodies[c], cos h, sin h): a
 * cone about every ray of the block, h rounded outward; cos h <= 0 switches the block's cull off.  Before a wave walks the targets
 * it drops the bounded primitives whose bounding sphere (about the staged origin) no ray inside the cone can reach, with a margin far
 * above the rounding of that test; infinite planes, meshes and heightfields always stay.  The survivors are visited in ascending
 * slot, so culling changes no output bit; its one observable effect is survivors ([env_count][B] int32 or NULL): the number of
 * targets the block's wave walked (target_count with the cull off).
 *
 * Errors as nt_raycast, plus NT_ERR_INVALID_ARG for camera_count / width / height <= 0, a null table, flags bit 0 without
 * block_cones, blocks_per_group < 0.  The LDS holds 48 bytes per (world, target) and, above 64 targets, 32 * ceil(K / 64) bytes of
 * survivor masks.
 * --------------------------------------------------------------------------------------------------------------------------- */
#define NT_CAMERA_CULL 1
#define NT_CAMERA_TILE 8
typedef struct {
    int32_t camera_count, width, height; /* C, W, H */
    const float* ray_origins;          /* [C][3] in the frame of ray_bodies[c] */
    const int32_t* ray_bodies;         /* [C] env-local body index or -1 (world frame) */
    const float* ray_directions;       /* [C][H * W][3] in the same frame */
    const float* forward;              /* [C][3] unit optical axis in the same frame */
    float max_distance;
    int32_t target_count;              /* K selected shape slots */
    const int32_t* targets;            /* DEVICE [K][2] (slot, GeoType), ascending slot */
    const int32_t* targets_host;       /* HOST   [K][2] the same table (checked before the launch) */
    const uint8_t* world_mask;         /* [env_count] or NULL */
    float* distance;                   /* [env_count][C][H][W] */
    float* depth;                      /* the same shape, or NULL */
    float* normal;                     /* [env_count][C][H][W][3] or NULL */
    int32_t* shape;                    /* [env_count][C][H][W] or NULL */
    /* mesh / heightfield tables, as in nt_raycast_args */
    const int32_t* shape_vertex_range;
    const int32_t* shape_triangle_range;
    const float* vertices;
    const int32_t* indices;
    const float* block_bounds;
    const int32_t* shape_block_start;
    const int32_t* shape_heightfield_index;
    const nt_heightfield* heightfields;
    const float* elevations;
    const float* block_cones;          /* DEVICE [C][blocks per camera][5], or NULL without NT_CAMERA_CULL */
    int32_t* survivors;                /* [env_count][B] or NULL */
    int32_t flags;                     /* NT_CAMERA_CULL */
    int32_t blocks_per_group;          /* 0: chosen by the entry point */
} nt_camera_args;
nt_status nt_camera_render(const nt_model* m, const nt_state* s, const nt_camera_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
