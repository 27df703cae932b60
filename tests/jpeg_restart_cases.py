"""Shared by test_jpeg_restart_parse.py (CPU) and test_gpu_jpeg_restart.py: baseline JPEGs with
restart intervals for the device entropy decode (csrc/jpeg_huff.hip, its host twin
llfe_jpeg_entropy_reference) -- every interval length against the MCU grid, markers on the seams
of the subsequence size, flat images that never self-synchronise, and files whose markers are
wrong.  Built on tests/jpeg_restate.py and tests/jpeg_huff_cases.py; everything is found by
deterministic searches on the CPU.
"""
import functools

import numpy as np

from low_level_feature_extraction_amd import decode, synth
from tests import jpeg_huff_cases as H
from tests import jpeg_restate as R


def scan_bytes(blob):
    """The scan of a blob as the parser stages it with LLFE_JPEG_PARSE_RESTARTS, markers included."""
    sb = decode.stage_bytes([blob], workers=1, restarts=True)
    assert sb.status == [0]
    s = sb.scans[0]
    return sb.records[0, s.scan_offset:s.scan_offset + s.scan_bytes].copy()


def markers(blob):
    """Raw offsets in the scan of the FF of every restart marker."""
    d = scan_bytes(blob)
    return [int(k) for k in np.flatnonzero(d[:-1] == 0xFF) if 0xD0 <= d[k + 1] <= 0xD7]


@functools.lru_cache(maxsize=None)
def small(**kw):
    """40 x 56 noise at 4:2:0 (3 x 4 = 12 MCUs of 6 blocks) unless kw says otherwise."""
    kw = dict(dict(quality=85, subsampling=2), **kw)
    gray = kw.pop("gray", False)
    a = np.random.default_rng(77).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    return R.jpeg(a[:, :, 1].copy() if gray else a, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> blobs of one size: the interval lengths, samplings, tables and qualities."""
    out = {
        "ri_1": [small(restart_marker_blocks=1)],  # 11 markers: the index wraps past D7
        "last_interval_short": [small(restart_marker_blocks=5)],
        "dri_without_marker": [small(restart_marker_blocks=12), small(restart_marker_blocks=40)],
        "one_mcu_row": [small(restart_marker_rows=1)],
        "samplings": [small(gray=True, restart_marker_blocks=2), small(subsampling=0, restart_marker_blocks=3),
                      small(subsampling=1, restart_marker_blocks=2)],
        "optimised_tables": [small(optimize=True, restart_marker_blocks=2), small(optimize=True, restart_marker_rows=2)],
        "quality_1_and_100": [small(quality=1, restart_marker_blocks=1), small(quality=100, restart_marker_blocks=1),
                              small(quality=100, subsampling=0, restart_marker_rows=1)],
    }
    assert len(markers(out["ri_1"][0])) == 11 and len(markers(out["last_interval_short"][0])) == 2
    assert [len(markers(b)) for b in out["dri_without_marker"]] == [0, 0]
    return out


@functools.lru_cache(maxsize=None)
def sized(h, w, ri):
    """The case list's sizes at 4:2:0 with an interval of ri MCUs (synth images where large enough)."""
    if min(h, w) < 32:
        a = np.random.default_rng(900 + 17 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        a = synth.synth_numpy(3, h, w, seed=3)[:, :, ::-1].copy()
    return R.jpeg(a, quality=85, subsampling=2, restart_marker_blocks=ri)


@functools.lru_cache(maxsize=None)
def striped(ri=3):
    """H.flat's recipe (512 x 512 flat colour with a noise stripe, 1024 MCUs) with restarts: k_huff_dc's
    lanes hold four MCUs each, so its sums restart inside and between lanes."""
    a = np.empty((512, 512, 3), np.uint8)
    a[:] = (200, 120, 40)
    a[240:272] = np.random.default_rng(1).integers(0, 256, (32, 512, 3), dtype=np.uint8)
    return R.jpeg(a, quality=85, subsampling=2, restart_marker_blocks=ri)


@functools.lru_cache(maxsize=None)
def flat(rows, size=2048):
    """Flat colour at 4:2:0, restart markers every `rows` MCU rows: between two markers no lane
    finds the true state by itself."""
    a = np.empty((size, size, 3), np.uint8)
    a[:] = (200, 120, 40)
    return R.jpeg(a, quality=85, subsampling=2, restart_marker_rows=rows)


@functools.lru_cache(maxsize=None)
def seam(residue):
    """(blob, offset): 16 x 32 grey noise, a marker per block, with a marker's FF at a raw offset
    of the scan that is `residue` mod the subsequence size, at 126 or later."""
    for seed in range(2):
        a = np.random.default_rng(seed).integers(0, 256, (16, 32), dtype=np.uint8)
        for q in range(5, 100, 3):
            b = R.jpeg(a, quality=q, restart_marker_blocks=1)
            hits = [k for k in markers(b) if k >= H.SUB - 2 and k % H.SUB == residue]
            if hits:
                return b, hits[0]
    raise AssertionError(f"no marker at offset {residue} mod {H.SUB}")


SEAMS = (H.SUB - 1, 0, H.SUB - 2, 1)  # the boundary on the Dn, on the FF, just behind the marker, one byte in front


# ------------------------------------------------------------------ files whose markers are wrong
def _span(blob):
    b = bytes(blob)
    sos = b.index(b"\xff\xda")
    return sos + 2 + ((b[sos + 2] << 8) | b[sos + 3]), b.rindex(b"\xff\xd9")


def _first_marker(blob):
    begin, _ = _span(blob)
    return begin + markers(blob)[0]


def wrong_index(blob):
    p = _first_marker(blob)
    assert blob[p:p + 2] == b"\xff\xd0"
    return blob[:p + 1] + b"\xd1" + blob[p + 2:]


def marker_deleted(blob):
    p = _first_marker(blob)
    return blob[:p] + blob[p + 2:]


def dri_edited(blob):
    p = blob.index(b"\xff\xdd\x00\x04\x00\x05")
    return blob[:p + 5] + b"\x04" + blob[p + 6:]


def marker_doubled(blob):
    p = _first_marker(blob)
    return blob[:p + 2] + b"\xff\xd1" + blob[p + 2:]


def marker_mid_interval(blob):
    begin, _ = _span(blob)
    p = begin + markers(blob)[0] // 2
    while 0xFF in blob[p - 2:p + 2]:
        p += 1
    return blob[:p] + b"\xff\xd0" + blob[p:]


def marker_before_eoi(blob):
    _, end = _span(blob)
    return blob[:end] + b"\xff\xd2" + blob[end:]


DAMAGES = (wrong_index, marker_deleted, dri_edited, marker_doubled, marker_mid_interval, marker_before_eoi)


def damaged_source():
    """40 x 56 at 4:2:0 with an interval of 5 MCUs: two markers."""
    b = small(restart_marker_blocks=5)
    assert len(markers(b)) == 2
    return b
