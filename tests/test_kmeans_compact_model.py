"""The NumPy model of the Lloyd sweep's cube batches and per-wave pending lists
(tools/km_lloyd_compact_sim.py) on a 160 x 160 photo: its own counts satisfy the identities the device's
trace counters are held to (tests/test_gpu_kmeans_compact.py).  The model is float64 and the device's
margins float32, so the two are never compared with each other."""
import numpy as np

from low_level_feature_extraction_amd import synth
from tools import km_lloyd_compact_sim as sim


def test_model_counts_satisfy_the_walk_identities(orc):
    host = synth.synth_numpy(1, 160, 160, seed=2025)
    keys = orc.color_unique(host, orc.device_noise(160 * 160, 2027, 0))
    attempts = sim.attempt_counts(keys, 5, orc.image_rng_state(2027, 0), attempts=3)
    assert len(attempts) == 3
    two_total = 0
    for a, sweeps in enumerate(attempts):
        assert 1 <= len(sweeps) <= 100, (a, len(sweeps))
        for j, s in enumerate(sweeps):
            two_total += s["two"]
            assert s["old_live"] + s["old_below"] == s["two"], (a, j, s)
            assert sim.OLD_SPLIT_MIN * s["old_walks"] <= s["old_live"] <= 64 * s["old_walks"], (a, j, s)
            assert s["two"] + s["multi"] <= 64 * s["batches"], (a, j, s)
            for w in sim.WAVES:
                walks, part = s["walks"][w], s["partial"][w]
                assert 0 <= part <= min(w, walks), (a, j, w, s)          # at most one flush per wave and sweep
                assert 64 * (walks - part) <= s["two"] <= 64 * walks, (a, j, w, s)
                assert part >= (1 if s["two"] % 64 else 0), (a, j, w, s)
    print(f"photo160: {sum(len(s) for s in attempts)} sweeps, {two_total} two-centre cubes")
    assert two_total > 0  # (8 192 cubes or more: the cells path, with cubes on a bisector)
    assert len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63))) >= sim.CELL_MIN
