"""Shared by test_jpeg_parse.py (CPU) and test_gpu_jpeg_huff.py: the inputs of the device entropy
decode (csrc/jpeg_huff.hip, its host twin llfe_jpeg_entropy_reference) beyond the case list of
tests/jpeg_restate.py -- phase-locked flat images, scans of chosen lengths around the
subsequence size, a stuffed FF 00 pair on a subsequence boundary, corrupt scans -- and the
comparison of coefficient slots.  Everything is found by deterministic searches on the CPU.
"""
import functools

import numpy as np

from low_level_feature_extraction_amd import _lib, decode
from tests import jpeg_restate as R

SUB = _lib.JPEG_SUBSEQUENCE_BYTES
# SETTINGS of jpeg_restate that are baseline, single-scan and without restart markers
ACCEPTED = (0, 1, 2, 3, 4, 5, 6, 9, 11, 12)
REFUSED = (7, 8, 10, 13)  # progressive (7, 8, 13), restart intervals (10)
UNSUPPORTED, INVALID = -5, -1


def extents(d):
    """[(start, end)] of the bytes of a slot that the image of descriptor d occupies."""
    out = []
    for c in range(d.n_comp):
        k = d.comp[c]
        out += [(k.quant_offset, k.quant_offset + 128), (k.coef_offset, k.coef_offset + k.blocks_w * k.blocks_h * 128)]
    return out


def slots_equal(got, want, d):
    """got / want: one slot each (uint8 arrays); equal over the extents of d."""
    return d.n_comp > 0 and all(np.array_equal(got[a:b], want[a:b]) for a, b in extents(d))


def scan_bytes(blob):
    """The entropy-coded bytes of an eligible blob as llfe_jpeg_parse_batch stages them."""
    sb = decode.stage_bytes([blob], workers=1)
    assert sb.status == [0]
    s = sb.scans[0]
    return sb.records[0, s.scan_offset:s.scan_offset + s.scan_bytes].copy()


@functools.lru_cache(maxsize=None)
def flat(sub, stripe, size=512):
    """A flat colour image (its MCUs are bit-identical: at 4:2:0 a lane that starts one block out
    of phase never synchronises), optionally with a 32-row noise stripe."""
    a = np.empty((size, size, 3), np.uint8)
    a[:] = (200, 120, 40)
    if stripe:
        a[240:272] = np.random.default_rng(1).integers(0, 256, (32, size, 3), dtype=np.uint8)
    return R.jpeg(a, quality=85, subsampling=sub)


@functools.lru_cache(maxsize=None)
def scan_of_length(target):
    """A 16 x 16 grey noise image whose scan is exactly `target` bytes long (searched over seeds
    and qualities)."""
    for seed in range(60):
        a = np.random.default_rng(seed).integers(0, 256, (16, 16), dtype=np.uint8)
        for q in range(5, 100, 3):
            b = R.jpeg(a, quality=q)
            if len(scan_bytes(b)) == target:
                return b
    raise AssertionError(f"no encoding with a scan of {target} bytes")


@functools.lru_cache(maxsize=None)
def stuffed_boundary():
    """(blob, boundaries): quality-100 noise whose scan has the 00 of a stuffed FF 00 pair on a
    subsequence boundary."""
    for seed in range(40):
        a = np.random.default_rng(100 + seed).integers(0, 256, (128, 128, 3), dtype=np.uint8)
        b = R.jpeg(a, quality=100, subsampling=0)
        d = scan_bytes(b)
        hits = [k for k in range(SUB, len(d), SUB) if d[k] == 0 and d[k - 1] == 0xFF]
        if hits:
            return b, hits
    raise AssertionError("no stuffed pair on a subsequence boundary")


def _scan_span(blob):
    b = bytes(blob)
    sos = b.index(b"\xff\xda")
    begin = sos + 2 + ((b[sos + 2] << 8) | b[sos + 3])
    return begin, b.rindex(b"\xff\xd9")


def flipped(blob):
    """One byte of the scan changed mid-stream, without making or breaking an FF."""
    b = bytearray(blob)
    begin, end = _scan_span(blob)
    p = (begin + end) // 2
    while b[p - 1] == 0xFF or b[p] in (0xFF, 0xEF) or b[p + 1] == 0x00:
        p += 1
    b[p] ^= 0x10
    return bytes(b)


def cut(blob, n=10):
    """The scan's last n bytes removed in front of the EOI."""
    b = bytes(blob)
    _, end = _scan_span(blob)
    return b[:end - n] + b[end:]


def host_result(blob):
    """What decode_batch gives for this one blob: its image, or the DecodeError's text."""
    try:
        return decode.decode_batch([blob], workers=1)[0]
    except decode.DecodeError as e:
        return str(e)
