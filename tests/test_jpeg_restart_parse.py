"""Restart intervals in the host half of the device entropy decode (llfe_jpeg_parse_batch_flags
with LLFE_JPEG_PARSE_RESTARTS, csrc/jpeg_decode.cpp) and in the plain C++ twin of the kernels
(llfe_jpeg_entropy_reference: the csrc/jpeg_huff_core.h the kernels compile), CPU only.

Without the flag nothing changes: restart files stay refused.  With it the parser stages their
scans raw, markers included, and the twin -- chunked into subsequences as the kernels are, and in
one piece -- reproduces the coefficient slots of decode.stage_coefs (libjpeg-turbo's
jpeg_read_coefficients) bit for bit: every interval length against the MCU grid, markers on the
seams of the subsequence size, flat images that never self-synchronise between two markers, DC
sums that restart inside and between the lanes of k_huff_dc.  Files whose markers are not where
the interval says are handed back, alone.
"""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib, decode
from tests import jpeg_huff_cases as H
from tests import jpeg_restart_cases as X
from tests import jpeg_restate as R


def _parse(blobs, h, w, flags, fill=0xA5, threads=1, entry="llfe_jpeg_parse_batch_flags"):
    """The parser into pre-filled records, so a write shows."""
    n = len(blobs)
    stride = _lib.JPEG_RECORD_HEADER + ((max(len(b) for b in blobs) + 15) & ~15) + 16
    rec = np.full((n, stride), fill, np.uint8)
    descs, scans = (_lib.LlfeJpegDesc * n)(), (_lib.LlfeJpegScan * n)()
    keep = [C.c_char_p(b) for b in blobs]
    ptrs = (C.c_void_p * n)(*[C.cast(k, C.c_void_p) for k in keep])
    sizes = (C.c_uint64 * n)(*[len(b) for b in blobs])
    status = (C.c_int32 * n)()
    args = [ptrs, sizes, n, h, w, rec.ctypes.data, stride, decode.coef_slot_bytes(h, w), descs, scans, status, threads]
    rc = getattr(_lib.lib(), entry)(*args, *([flags] if entry.endswith("_flags") else []))
    return rc, list(status), rec, descs, scans


def _twin_equals_stage_coefs(blobs, one_piece=False):
    sb = decode.stage_bytes(blobs, workers=2, restarts=True)
    st = decode.stage_coefs(blobs, workers=2)
    assert sb.status == [0] * len(blobs) and st.status == [0] * len(blobs)
    slots, status = decode.entropy_reference(sb, one_piece)
    assert status == [0] * len(blobs)
    for i in range(len(blobs)):
        assert bytes(sb.descs[i]) == bytes(st.descs[i])
        assert H.slots_equal(slots[i], st.slots[i], st.descs[i]), f"image {i}"
    return sb


@pytest.mark.parametrize("h,w", R.SIZES)
def test_defaults_refuse_and_the_flag_takes_restart_files(h, w):
    blob = R.blob(h, w, 10)  # restart_marker_blocks=3
    for entry, flags in (("llfe_jpeg_parse_batch", 0), ("llfe_jpeg_parse_batch_flags", 0)):
        rc, status, rec, descs, scans = _parse([blob], h, w, flags, entry=entry)
        assert rc == H.UNSUPPORTED and status == [H.UNSUPPORTED]
        assert (rec == 0xA5).all() and descs[0].n_comp == 0 and scans[0].blocks_in_mcu == 0
    assert decode.stage_bytes([blob], workers=1).status == [H.UNSUPPORTED]
    assert _parse([blob], h, w, 2)[0] == H.INVALID and _parse([blob], h, w, 3)[0] == H.INVALID  # unknown flag bits
    rc, status, rec, descs, scans = _parse([blob, R.blob(h, w, 0)], h, w, _lib.JPEG_PARSE_RESTARTS, threads=2)
    assert rc == 0 and status == [0, 0]
    assert scans[0].restart_interval == 3 and scans[1].restart_interval == 0
    st = decode.stage_coefs([blob], workers=1)
    assert bytes(descs[0]) == bytes(st.descs[0])
    s = scans[0]
    end = blob.rindex(b"\xff\xd9")
    assert bytes(rec[0, s.scan_offset:s.scan_offset + s.scan_bytes]) == blob[end - s.scan_bytes:end]
    assert not rec[0, s.scan_offset + s.scan_bytes:s.scan_offset + ((s.scan_bytes + 15) & ~15) + 16].any()
    mcus = s.mcus_w * s.mcus_h
    assert len(X.markers(blob)) == (mcus - 1) // 3
    # the restart-free neighbour is staged as the unflagged parser stages it
    rc1, status1, rec1, descs1, scans1 = _parse([R.blob(h, w, 0)], h, w, 0, entry="llfe_jpeg_parse_batch")
    used = _lib.JPEG_RECORD_HEADER + ((scans1[0].scan_bytes + 15) & ~15) + 16
    assert np.array_equal(rec1[0, :used], rec[1, :used])
    assert bytes(descs1[0]) == bytes(descs[1]) and scans1[0].scan_bytes == scans[1].scan_bytes


def test_progressive_arithmetic_and_stray_markers_stay_refused():
    h, w = 40, 56
    a = np.random.default_rng(4).integers(0, 256, (h, w, 3), dtype=np.uint8)
    progressive = R.jpeg(a, quality=85, progressive=True, restart_marker_blocks=2)
    ok = X.small(restart_marker_blocks=5)
    sof = ok.index(b"\xff\xc0")
    arithmetic = ok[:sof + 1] + b"\xc9" + ok[sof + 2:]  # SOF9: the frame of an arithmetic-coded file
    p = X._first_marker(ok)
    fill = ok[:p] + b"\xff" + ok[p:]  # FF FF D0: a fill byte in front of the marker
    other = ok[:p + 1] + b"\xc4" + ok[p + 2:]  # another marker inside the scan
    plain = X.small()
    begin, end = X._span(plain)
    stray = plain[:end] + b"\xff\xd0" + plain[end:]  # a restart marker in a file without a DRI
    blobs = [ok, progressive, arithmetic, fill, other, stray, plain]
    rc, status, rec, descs, scans = _parse(blobs, h, w, _lib.JPEG_PARSE_RESTARTS, threads=3)
    assert status[0] == 0 and status[6] == 0 and all(s in (H.UNSUPPORTED, H.INVALID) for s in status[1:6])
    assert status[1] == status[3] == status[4] == status[5] == H.UNSUPPORTED
    for i in range(1, 6):
        assert (rec[i] == 0xA5).all() and descs[i].n_comp == 0 and scans[i].blocks_in_mcu == 0
    assert scans[0].restart_interval == 5 and scans[6].restart_interval == 0


@pytest.mark.parametrize("one_piece", [False, True])
@pytest.mark.parametrize("name", ["ri_1", "last_interval_short", "dri_without_marker", "one_mcu_row", "samplings",
                                  "optimised_tables", "quality_1_and_100"])
def test_twin_reproduces_the_coefficient_slots(name, one_piece):
    for blob in X.cases()[name]:  # (the samplings differ in their descriptors: one image per batch)
        _twin_equals_stage_coefs([blob], one_piece)


@pytest.mark.parametrize("one_piece", [False, True])
@pytest.mark.parametrize("h,w", R.SIZES)
def test_twin_at_the_case_list_sizes(h, w, one_piece):
    """Intervals of 1, 3 and 5 MCUs at every size of the case list, the restart-free setting 0 in
    the same batch; at 240 x 321 (315 MCUs) the DC sums restart inside every lane of k_huff_dc."""
    _twin_equals_stage_coefs([X.sized(h, w, 1), X.sized(h, w, 3), R.blob(h, w, 0), X.sized(h, w, 5)], one_piece)


@pytest.mark.parametrize("one_piece", [False, True])
def test_twin_restarts_the_dc_sums_inside_and_between_lanes(one_piece):
    sb = _twin_equals_stage_coefs([X.striped(3), X.striped(7)], one_piece)
    assert sb.scans[0].mcus_w * sb.scans[0].mcus_h == 1024 and [s.restart_interval for s in sb.scans] == [3, 7]


@pytest.mark.parametrize("residue", X.SEAMS)
def test_twin_with_a_marker_on_a_subsequence_seam(residue):
    blob, at = X.seam(residue)
    d = X.scan_bytes(blob)
    assert at >= H.SUB - 2 and at % H.SUB == residue and d[at] == 0xFF and 0xD0 <= d[at + 1] <= 0xD7
    _twin_equals_stage_coefs([blob])
    _twin_equals_stage_coefs([blob], one_piece=True)


@pytest.mark.parametrize("rows", [8, 64])
def test_twin_on_flat_images_between_markers(rows):
    """2048 x 2048 flat colour at 4:2:0: lanes in three workgroups, none of which finds the true
    state by itself; 8 MCU rows make intervals of some 4 KB, 64 rows one marker mid-scan and
    intervals longer than a workgroup of lanes."""
    blob = X.flat(rows)
    m = X.markers(blob)
    lanes = -(-len(X.scan_bytes(blob)) // H.SUB)
    assert lanes > 2 * 256 and len(m) == 128 // rows - 1
    if rows == 64:
        assert m[0] > 256 * H.SUB and len(X.scan_bytes(blob)) - m[0] > 256 * H.SUB
    _twin_equals_stage_coefs([blob])


def test_twin_hands_files_with_wrong_markers_back():
    good = X.damaged_source()
    blobs = [good] + [f(good) for f in X.DAMAGES] + [X.small(restart_marker_blocks=1)]
    n = len(blobs)
    sb = decode.stage_bytes(blobs, workers=2, restarts=True)
    assert sb.status == [0] * n  # the headers and the marker walk are fine: the places are what is wrong
    assert [s.restart_interval for s in sb.scans] == [5, 5, 5, 4, 5, 5, 5, 1]
    st = decode.stage_coefs([blobs[0], blobs[-1]], workers=1)
    for one_piece in (False, True):
        slots, status = decode.entropy_reference(sb, one_piece)
        assert status == [0] + [H.UNSUPPORTED] * len(X.DAMAGES) + [0]
        assert H.slots_equal(slots[0], st.slots[0], st.descs[0]) and H.slots_equal(slots[-1], st.slots[1], st.descs[1])


def test_host_check_refuses_a_restart_interval_no_dri_can_hold():
    blobs = [X.small(restart_marker_blocks=5), X.small()]
    sb = decode.stage_bytes(blobs, workers=1, restarts=True)
    for i, value in ((0, -1), (0, 65536), (1, -1), (1, 65536)):
        scans = (_lib.LlfeJpegScan * 2).from_buffer_copy(sb.scans)
        scans[i].restart_interval = value
        slots = np.full((2, sb.slot_bytes), 77, np.uint8)
        status = (C.c_int32 * 2)()
        rc = _lib.lib().llfe_jpeg_entropy_reference(sb.records.ctypes.data, sb.records.size, scans, sb.descs, 2, sb.h, sb.w,
                                                    slots.ctypes.data, sb.slot_bytes, status, 0)
        assert rc == H.INVALID and (slots == 77).all()
    scans = (_lib.LlfeJpegScan * 2).from_buffer_copy(sb.scans)
    scans[0].restart_interval = 65535  # the largest a DRI holds: a valid record of a file whose markers are wrong
    slots, status = decode.entropy_reference(decode.StagedBytes(sb.blobs, sb.h, sb.w, sb.records, sb.descs, scans,
                                                                sb.status, sb.slot_bytes))
    assert status == [H.UNSUPPORTED, 0]
