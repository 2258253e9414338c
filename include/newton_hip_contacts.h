/* newton_hip_contacts.h -- the key-ordered contact export and the frame-to-frame matching report of libnewton_hip.so on the device
 * (extension of newton_hip.h).
 *
 * Reference interface replaced (paths relative to the Newton source tree):
 *   ContactSorter             newton/_src/geometry/contact_sort.py:194-440   the deterministic mode of CollisionPipeline.collide: the
 *                                                                            flat contact arrays ordered by the contact sort key
 *   ContactMatcher report     newton/_src/geometry/contact_match.py:602-1055 rigid_contact_match_index in the sorted order, the
 *                                                                            new / broken lists (collide.py:1126-1129,2033-2135)
 *
 * The order is a stable sort on the 64-bit key (shape0 << 32 | shape1) over the raw export order of nt_contacts_export followed by
 * the live rows of nt_contacts.flat (every env's analytic slots, every env's convex slots, then the rows).  No comparison sort runs:
 * the (shape0, shape1) pairs that can carry a contact are fixed when the pipeline is built, so every (pair, orientation) gets a
 * BUCKET whose rank in key order is computed once on the host (nt_contact_order).  Per export: live contacts per bucket -> a
 * multi-block exclusive scan over the ranked buckets (no atomics on the counts, no host read) -> every live slot / row scattered to
 * its position; inside a bucket the raw order is kept.
 *
 * Same conventions as newton_hip.h: device pointers owned by the caller, work enqueued on `stream`, no allocation, no
 * synchronisation -- every entry point can be recorded by nt_graph_capture_begin / _end. */
#ifndef NEWTON_HIP_CONTACTS_H
#define NEWTON_HIP_CONTACTS_H

#include "newton_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The order table.  Buckets: tile bucket (pair p, env e, orientation o) for every device pair of every env, o = 0 when the slot
 * carries shape0 == tile_shape0[p][e], else 1 (the pair written the other way round); row bucket (world w, j) for the K keys a
 * world's rows may carry (both orientations of every pair the SDF legs may route in that world; row_key ascending per world).
 * Ranks: enumerate the buckets in raw order -- tile buckets of the analytic pairs (env-major, then pair, then orientation), those of
 * the convex pairs likewise, then the row buckets world-major -- and take the inverse of a STABLE argsort of their keys (buckets
 * of equal keys then keep the raw order of their contacts).  Scratch sizes: B = 2 * env_count * np + env_count * K buckets. */
typedef struct {
    int32_t bucket_count;         /* B */
    const int32_t* tile_shape0;   /* [np][env_count] Newton id that orientation 0 of (pair, env) writes as shape0 */
    const int32_t* tile_rank;     /* [np][env_count][2] rank of the tile bucket */
    int32_t row_keys;             /* K (0: no row buckets) */
    const int64_t* row_key;       /* [env_count][K] shape0 << 32 | shape1, ascending inside a world */
    const int32_t* row_rank;      /* [env_count][K] rank of the row bucket */
    int32_t* bucket_fill;         /* [B] scratch: live contacts per bucket, indexed by rank */
    int32_t* bucket_start;        /* [B] scratch: exclusive scan of bucket_fill */
    int32_t* block_sum;           /* [B / 1024 + 2] scratch of the scan */
    int32_t* row_bucket;          /* [row_capacity] scratch: rank of the row's bucket, -1 inert */
    int32_t* row_sub;             /* [row_capacity] scratch: position of the row inside its bucket */
    int32_t* row_unmatched;       /* [1]: rows whose (shape0, shape1) is in no bucket of their world (never set by this project's
                                   * legs; such rows are left out of the export), accumulated -- zero it to re-arm */
} nt_contact_order;

/* Key-ordered flat arrays (Newton's Contacts layout, AoS).  Entries at or beyond count: shape ids -1, floats 0. */
typedef struct {
    int32_t cap;                  /* capacity of the flat arrays (Contacts.rigid_contact_max) */
    int32_t row_capacity;         /* capacity of nt_contacts.flat (0: no rows) */
    int32_t* count;               /* [1] rigid_contact_count */
    int32_t* shape0;              /* [cap] */
    int32_t* shape1;
    float* point0;                /* [cap][3] */
    float* point1;
    float* offset0;
    float* offset1;
    float* normal;
    float* margin0;               /* [cap] */
    float* margin1;
    float* stiffness;             /* [cap] or NULL: nt_contacts.prop of the slots, nt_flat_rows.stiffness of the rows (0 when the */
    float* damping;               /* source has none) -- Contacts.rigid_contact_stiffness / _damping / _friction */
    float* friction;
    int32_t* slot_flat;           /* [np*cpp][ES] out: position of every live slot in the arrays, -1 otherwise */
    int32_t* row_flat;            /* [row_capacity] out: position of every live row, -1 otherwise */
} nt_sorted_contacts;

/* counts -> scan -> scatter -> tail fill; writes every entry of `out` */
nt_status nt_contacts_export_sorted(const nt_model* m, const nt_contacts* c, const nt_contact_order* o, nt_sorted_contacts* out,
                                    void* stream);

/* The matching report in the sorted order.  The previous frame is described by what nt_contacts_order_save left (positions of its
 * slots and rows, its count) and by the matchers' histories (nt_contact_history / nt_flat_history, before their save). */
typedef struct {
    int32_t* prev_slot_flat;        /* [np*cpp][ES] positions of the previous frame's slots (initialise to -1) */
    int32_t* prev_row_flat;         /* [row_capacity] or NULL without rows (initialise to -1) */
    int32_t* prev_count;            /* [1] the previous frame's count (0 = no previous frame) */
    const int32_t* slot_match;      /* [np*cpp][ES] nt_contacts_match: previous SLOT, -1 or -2 */
    const int32_t* row_match;       /* [row_capacity] nt_flat_rows_match: previous ROW, -1 or -2; NULL without rows */
    const uint8_t* prev_slot_live;  /* nt_contact_history.prev_live (zeroed for reset worlds) */
    const uint8_t* prev_row_live;   /* nt_flat_history.prev_live, prev_row_start, prev_pair_count (a world with */
    const int32_t* prev_row_start;  /* prev_pair_count 0 was reset); NULL without rows */
    const int32_t* prev_pair_count;
    uint8_t* reset_world_mask;      /* [env_count] or NULL: the mask nt_contacts_match consumed; cleared by nt_contacts_order_save */
    int32_t* match_index;           /* [cap] out: rigid_contact_match_index (-1 beyond the count) */
    int32_t* new_indices;           /* [cap] out or NULL (no report): ascending positions i < count with match_index[i] < 0 */
    int32_t* new_count;             /* [1] */
    int32_t* broken_indices;        /* [cap] out: ascending positions of the previous frame's live contacts that no contact matched */
    int32_t* broken_count;          /* [1] */
    int32_t* flag;                  /* [cap] scratch */
    int32_t* offset;                /* [cap] scratch */
    int32_t* block_sum;             /* [cap / 1024 + 2] scratch */
} nt_contact_report;

/* match_index (+ the new / broken lists when new_indices is set) of the frame `sorted` holds; call after nt_contacts_match /
 * nt_flat_rows_match (and the sticky replay) and nt_contacts_export_sorted, before the histories are saved */
nt_status nt_contacts_match_report(const nt_model* m, const nt_sorted_contacts* sorted, const nt_contact_report* r, void* stream);
/* the frame as the next frame's previous one: positions, count; clears reset_world_mask */
nt_status nt_contacts_order_save(const nt_model* m, const nt_sorted_contacts* sorted, const nt_contact_report* r, void* stream);

/* ---- heterogeneous models: one key-ordered export over several world groups ----------------------------------------------------
 * A model whose worlds differ in topology runs as world groups, each a homogeneous model of its own (group-local shape ids).  The
 * export over all of them is the same counting sort: every group's buckets get GLOBAL ranks (one stable argsort of all groups'
 * bucket keys, in global shape ids, enumerated in the raw heterogeneous order: every group's analytic tile buckets in group order,
 * then per group its convex tile buckets and its row buckets), the per-group count passes fill disjoint entries of one
 * bucket_fill, one scan runs over all of them and the per-group scatters write one set of arrays, translating shape ids. */
typedef struct {
    const nt_model* m;              /* the group's model */
    const nt_contacts* c;           /* its contacts (group-local shape ids) */
    const nt_contact_order* o;      /* its table: bucket_count = the group's own B, ranks GLOBAL (0 <= rank < the global bucket
                                     * count), row scratch of its own; its bucket_fill / bucket_start / block_sum are not used */
    const int32_t* shape_id;        /* [group shape count] global id of every shape of the group (increasing) */
    int32_t row_capacity;           /* capacity of c->flat (0: no rows) */
    int32_t* slot_flat;             /* [np*cpp][ES] out: global position of every live slot, -1 otherwise */
    int32_t* row_flat;              /* [row_capacity] out: global position of every live row, -1 otherwise */
    const nt_contact_report* r;     /* the group's matching state, or NULL without matching: prev_slot_flat / prev_row_flat (GLOBAL
                                     * positions), slot_match, row_match, prev_slot_live, prev_row_live, prev_row_start,
                                     * prev_pair_count, reset_world_mask; its other fields are not used */
} nt_contact_group;

/* `o`: the global scan (bucket_count = sum of the groups' B, bucket_fill / bucket_start [bucket_count], block_sum
 * [bucket_count / 1024 + 2]; its other fields are not used).  `out`: the global arrays (cap, count, shape0 ...), its row_capacity /
 * slot_flat / row_flat are not used.  Writes every entry of `out`, the groups' slot_flat / row_flat, shape ids global. */
nt_status nt_contacts_export_sorted_groups(int32_t group_count, const nt_contact_group* groups, const nt_contact_order* o,
                                           nt_sorted_contacts* out, void* stream);
/* nt_contacts_match_report over the groups: match_index in global positions, the new / broken lists over the global arrays.  `r`:
 * prev_count, match_index, new_indices ... block_sum of the global arrays (its per-group fields are not used); every group
 * carries its own `r` */
nt_status nt_contacts_match_report_groups(int32_t group_count, const nt_contact_group* groups, const nt_sorted_contacts* sorted,
                                          const nt_contact_report* r, void* stream);
/* nt_contacts_order_save over the groups: every group's positions, the global count into r->prev_count, clears every group's
 * reset_world_mask */
nt_status nt_contacts_order_save_groups(int32_t group_count, const nt_contact_group* groups, const nt_sorted_contacts* sorted,
                                        const nt_contact_report* r, void* stream);

/* ---- contact sensor: net contact force per world on chosen sets of shapes, split by counterpart -------------------------------------
 * (newton_amd.sensors.SensorContact; reference capability: newton.sensors.SensorContact.)  One launch of contact_sensor_kernel straight
 * from the slot-major contacts and the rows of nt_contacts.flat, after an nt_xpbd_step that reported its impulses
 * (nt_xpbd_report.contact_impulse, nt_flat_rows.impulse): no export, no allocation, no synchronisation, no host read.
 *
 * Sensing objects and counterparts.  Per world there are S sensing objects and C counterparts, each a set of shape slots of a world
 * (ns env-local slots, then ng global shapes): slot_sensing[slot] in -1 .. S-1, slot_counterpart[slot] in -1 .. C-1.  A slot belongs to
 * at most one sensing object and at most one counterpart (that is what a table per slot can say); it may be both.
 *
 * Output.  net_force [env_count][S][include_total + C][3]: column 0 (with include_total) is the sum over every contact of the sensing
 * object, column include_total + c the part exchanged with counterpart c; the value is the force ON the sensing object.
 *
 * One contact contributes f = impulse[0:3] * (1.0f / dt), the expression of nt_contacts_export_force (a contribution equals the linear
 * part of that contact's Contacts.force row bit for bit): +f to the sensing object of shape0 (Contacts.force is the force on shape0's
 * body), -f to the sensing object of shape1; a counterpart column takes it when the OTHER shape of the contact is in that counterpart.
 * Both shapes may be sensing objects: each side gets its contribution, and when both lie in the same sensing object the cell takes +f,
 * then -f.  Skipped: slots with shape0 < 0 (unused), rows with shape0 == shape1 (inert, both -1), shape ids that are no shape of the
 * world (no env-local id of that world, no global id).
 *
 * Summation order, fixed: every cell is a float32 sequential sum from 0.0f over the world's slots in ascending slot index, then (when
 * nt_contacts.flat carries row_start / shape0 / shape1 / impulse and row_capacity > 0) over the world's rows
 * [row_start[w], row_start[w + 1]), clamped to min(row_start[env_count], row_capacity), in ascending row index.  No float atomics, no
 * grouping that depends on the launch shape (one lane owns a cell from its first contact to its last).  Hence:
 *   - replicated worlds give equal bits;
 *   - with the raw (non-deterministic) export order, a cell equals the float32 sequential sum over that world's entries of the flat
 *     Contacts.force / rigid_contact_shape0 / _shape1 in their order: the flat order restricted to one world is its analytic slots, its
 *     convex slots (= ascending slot index), then its live rows.
 *
 * world_mask ([env_count] uint8, nullable): rows of unselected worlds are neither computed nor written.  Every selected world's whole
 * output row is written on every call, zeros included.
 *
 * The tables are validated on the host copies (slot_sensing_host / slot_counterpart_host, [ns + ng] each; slot_counterpart_host may
 * be NULL when C == 0).  NT_ERR_INVALID_ARG before any launch: NULL arguments, S <= 0, C < 0, no column at all (include_total + C
 * == 0), an entry outside its range, dt <= 0 or not finite, a flat.impulse without row_start / shape0 / shape1.  The mapping has no
 * LDS bound (the contacts of a world pass through a fixed staging buffer in chunks), so no argument is answered
 * NT_ERR_UNSUPPORTED. */
typedef struct {
    int32_t sensing_count;                /* S >= 1 */
    int32_t counterpart_count;            /* C >= 0 */
    int32_t include_total;                /* 0 / 1 */
    int32_t row_capacity;                 /* capacity of nt_contacts.flat (0: its rows are not read) */
    const int32_t* slot_sensing;          /* [ns + ng] device */
    const int32_t* slot_counterpart;      /* [ns + ng] device (NULL allowed when C == 0) */
    const int32_t* slot_sensing_host;     /* the same tables on the host: what the entry point validates */
    const int32_t* slot_counterpart_host;
    const uint8_t* world_mask;            /* [env_count] device or NULL */
    float* net_force;                     /* [env_count][S][include_total + C][3] device, out */
} nt_contact_sensor_args;

/* contact_impulse: [6][np*cpp][ES], what nt_xpbd_step wrote through the contact_impulse member of its report; NULL allowed only when
 * the model has no slots */
nt_status nt_contact_sensor(const nt_model* m, const nt_contacts* c, const float* contact_impulse, float dt,
                            const nt_contact_sensor_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
