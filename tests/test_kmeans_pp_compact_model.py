"""The NumPy model of k-means++'s per-wave split lists (tools/km_pp_compact_sim.py) against the model the pinned
GPU test uses (tools/km_pp_gain_sim.py attempts_split), on two small key sets, no GPU: the lists change when a
cube is walked, not which cubes are split, so the split set, its colours and its undecided trials are equal
attempt by attempt at threshold 8, and the model's walk counts obey what the device's must:

    lanes == split_cubes + und2 + 2 und3
    ceil(lanes / 64) <= walks[W] <= lanes // 64 + W x rounds + min(2 (lanes // 64 + W x rounds), und2 + 2 und3)
    partial[W] <= walks[W], mixed[W] <= walks[W], partial[W] <= 3 W x rounds
    batches_split <= old_walks <= batches_split + und2 + 2 und3      (walking per batch, before)

and, where the split batches hold fewer than 32 cubes on average, fewer walks than split batches.

Inputs: a two-rod colour set on the cells path (8 x 8 cubes per red quarter, 8 192 cubes: whole batches of
owned undecided cubes beside sparse ones) and a small cubes-only set, which lists nothing.
"""
import numpy as np

from tools import km_pp_compact_sim as csim
from tools import km_pp_gain_sim as sim

K = 5
ROUNDS = K - 1
RNG_STATES = (0x9E3779B97F4A7C15, 12345)


def _rods_keys():
    rs = np.random.RandomState(5)
    blk = np.stack(np.meshgrid(np.arange(256), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)
    corner = ((blk & 3) == 0).all(1)
    out = []
    for o in (32, 192):
        rest = blk[~corner][rs.permutation(int((~corner).sum()))[: len(blk) // 12]]
        out.append(np.concatenate([blk[corner], rest]) + np.array([0, o, o]))
    p = np.concatenate(out)
    return np.unique((p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2])


def _small_keys():
    rs = np.random.RandomState(7)
    p = rs.randint(0, 256, (6000, 3))
    return np.unique((p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2])


def _check(keys, st, cells):
    old = sim.attempts_split(keys, K, st, 4, 8)
    new = csim.attempts_compact(keys, K, st, 4, 8)
    total = 0
    for (ch_o, o), (ch_n, n) in zip(old, new):
        assert np.array_equal(ch_o, ch_n)
        assert sorted(o["split_idx"]) == sorted(n["split_idx"])
        assert (o["split_cubes"], o["split_pts"], o["batches_split"]) == (n["split_cubes"], n["split_pts"], n["batches_split"])
        assert np.array_equal(o["und_split"], n["und_split"])
        assert sum(n["round_cubes"]) == n["split_cubes"] and len(n["round_cubes"]) == ROUNDS
        u = n["und_split"]
        extra = int(u[2] + 2 * u[3])
        assert n["lanes"] == n["split_cubes"] + extra
        assert n["batches_split"] <= n["old_walks"] <= n["batches_split"] + extra
        for w in csim.WAVES:
            drains = n["lanes"] // 64 + w * ROUNDS
            assert -(-n["lanes"] // 64) <= n["walks"][w] <= drains + min(2 * drains, extra), (w, n["walks"][w], n["lanes"])
            assert n["partial"][w] <= n["walks"][w] and n["mixed"][w] <= n["walks"][w]
            assert n["partial"][w] <= 3 * w * ROUNDS
        total += n["split_cubes"]
    assert (total > 0) == cells
    return new


def test_rods_split_set_and_walk_invariants():
    keys = _rods_keys()
    assert len(sim.CubeTable(np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1)).n) >= sim.CELL_MIN
    for st in RNG_STATES:
        new = _check(keys, st, True)
        # sparse batches (fewer than 32 cubes on average): the lists need fewer walks than one per batch
        cubes, batches = sum(n["split_cubes"] for _, n in new), sum(n["batches_split"] for _, n in new)
        if cubes < 32 * batches:
            for w in csim.WAVES:
                assert sum(n["walks"][w] for _, n in new) < batches, (w, batches)


def test_cubes_only_set_lists_nothing():
    keys = _small_keys()
    assert len(sim.CubeTable(np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1)).n) < sim.CELL_MIN
    for st in RNG_STATES:
        for _, n in _check(keys, st, False):
            assert n["lanes"] == 0 and not any(n["walks"].values()) and not any(n["mixed"].values())
