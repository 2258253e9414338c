"""Host logic of the key-ordered export over the world groups (newton_amd/hetero.py grouped_contact_order_tables): the global rank
table of a mixed model is a permutation of its buckets, ranks follow the global keys, the ground plane's buckets of all groups form
one block, and every group's own bucket order is kept."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_global_rank_table_of_a_mixed_model():
    from test_heterogeneous_worlds import LAYOUT, mixed_model

    from newton_amd.collide import contact_order_tables
    from newton_amd.hetero import grouped_contact_order_tables

    model = mixed_model(LAYOUT)
    parts = model.world_groups.parts
    tab = grouped_contact_order_tables(model, [False] * len(parts))
    assert grouped_contact_order_tables(model, [False] * len(parts)) is tab  # (built once per model)
    B, key = tab["bucket_count"], tab["bucket_key"]
    rank = np.concatenate([np.concatenate([t.reshape(-1), r.reshape(-1)]) for t, r, _k in tab["groups"]])
    assert B == len(rank) == len(key) == sum(2 * p.env.env_count * p.env.np for p in parts) > 0
    assert np.array_equal(np.sort(rank), np.arange(B))  # a permutation
    by_rank = np.empty(B, np.int64)
    by_rank[rank] = key
    assert np.all(np.diff(by_rank) >= 0)  # non-decreasing global keys
    plane = int(np.flatnonzero(np.asarray(model.shape_world) == -1)[0])
    on_plane = np.flatnonzero((by_rank >> 32) == plane)  # ranks of the buckets whose shape0 is the ground plane
    assert len(on_plane) > 0 and np.array_equal(on_plane, np.arange(on_plane[0], on_plane[-1] + 1))
    off, groups_on_plane = 0, 0
    for p, (tile_rank, _r, _k) in zip(parts, tab["groups"]):
        n = len(tile_rank)
        groups_on_plane += bool(np.any((key[off:off + n] >> 32) == plane))
        # a group's own buckets keep their relative order: its local ranks sorted == its global ranks sorted
        local = contact_order_tables(p)["tile_rank"]
        assert np.array_equal(np.argsort(local, kind="stable"), np.argsort(tile_rank, kind="stable"))
        off += n
    assert groups_on_plane >= 2  # (one block across groups, not one per group)
