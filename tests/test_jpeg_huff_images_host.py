"""The host half of the device entropy decode of a mixed-size batch (llfe_jpeg_records_layout and
llfe_jpeg_parse_images behind decode.stage_bytes_images) and the kernels' host twin over tight
slots (llfe_jpeg_entropy_reference_images), CPU only: every baseline case of
tests/jpeg_restate.py, all sizes and sampling classes, in one ragged call against the host's
extraction (decode.stage_coefs_images: libjpeg-turbo's jpeg_read_coefficients); restart files
beside restart-free ones; the record layout and the statuses of what the path hands back; the
refusals that come before any work; damaged files beside good neighbours.  The slots of every
twin call carry a sentinel guard behind their end."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from tests import jpeg_huff_cases as H
from tests import jpeg_restart_cases as RC
from tests import jpeg_restate as R

OK, INVALID, CAPACITY, UNSUPPORTED = 0, _lib.LLFE_ERR_INVALID, -3, -5
GUARD = 4096


def _up16(v):
    return (v + 15) & ~15


def _twin(st, one_piece=False, images=None, slot_bytes=None, used_bytes=None, fill=0):
    """llfe_jpeg_entropy_reference_images into slots with a sentinel guard behind their end:
    -> (rc, the slots without the guard, status list); the guard is checked here."""
    n = len(st.blobs)
    total = st.slot_bytes if slot_bytes is None else slot_bytes
    buf = np.full(total + GUARD, fill, np.uint8)
    buf[total:] = 0xC3
    status = (C.c_int32 * max(n, 1))(*([99] * max(n, 1)))
    rc = _lib.lib().llfe_jpeg_entropy_reference_images(
        st.records.ctypes.data, st.used_bytes if used_bytes is None else used_bytes, st.scans, st.descs,
        st.images if images is None else images, n, buf.ctypes.data, total, status, int(one_piece))
    assert (buf[total:] == 0xC3).all(), "the guard behind the slots was written"
    return rc, buf[:total], list(status)[:n]


def _slot(buf, m):
    return buf[m.slot_offset: m.slot_offset + m.slot_bytes]


def _equal_host(st, slots, status, host, take=None):
    """Every image the twin took equals the host's extraction; -> the places it took."""
    took = []
    for i, rc in enumerate(status):
        if rc != 0 or (take is not None and i not in take):
            continue
        assert host.status[i] == 0 and bytes(st.descs[i]) == bytes(host.descs[i]), i
        assert (st.images[i].slot_offset, st.images[i].slot_bytes) == (host.images[i].slot_offset, host.images[i].slot_bytes)
        assert H.slots_equal(_slot(slots, st.images[i]), _slot(host.slots, host.images[i]), host.descs[i]), f"slot {i} differs"
        took.append(i)
    return took


@pytest.fixture(scope="module")
def case_list():
    cases = [c for c in R.CASES if c[2] in H.ACCEPTED]
    return cases, [R.blob(*c) for c in cases]


def test_all_sizes_in_one_ragged_call(case_list):
    cases, blobs = case_list
    assert {c[:2] for c in cases} == set(R.SIZES) and len(cases) == len(R.SIZES) * len(H.ACCEPTED)
    st = decode.stage_bytes_images(blobs, workers=3)
    host = decode.stage_coefs_images(blobs, workers=3)
    assert st.layout_status == [OK] * len(blobs) and st.status == [OK] * len(blobs) == host.status
    for i in range(len(blobs)):  # the descriptors of the host's extraction, byte for byte
        assert bytes(st.descs[i]) == bytes(host.descs[i]), cases[i]
        assert st.scans[i].restart_interval == 0 and st.scans[i].blocks_in_mcu in (1, 3, 4, 6)
    assert {d.sampling for d in st.descs} == {R.GRAY, R.S444, R.S422, R.S420}
    per_image = {}
    for one_piece in (False, True):
        rc, slots, status = _twin(st, one_piece)
        assert rc == OK and status == [OK] * len(blobs)
        assert _equal_host(st, slots, status, host) == list(range(len(blobs)))
        per_image = {i: _slot(slots, st.images[i]).copy() for i in range(len(blobs))}
    # the same batch shuffled: other offsets, the same slot contents per image
    order = [int(i) for i in np.random.default_rng(11).permutation(len(blobs))]
    sh = decode.stage_bytes_images([blobs[i] for i in order], workers=2)
    assert sh.status == [OK] * len(blobs)
    rc, slots, status = _twin(sh, False, fill=0)
    assert rc == OK and status == [OK] * len(blobs)
    moved = 0
    for k, i in enumerate(order):
        assert bytes(sh.descs[k]) == bytes(st.descs[i])
        assert np.array_equal(_slot(slots, sh.images[k]), per_image[i]), cases[i]
        moved += sh.images[k].slot_offset != st.images[i].slot_offset
    assert moved > len(blobs) // 2


def test_restart_files_beside_restart_free_ones():
    blobs = [R.blob(h, w, k) for (h, w) in ((17, 33), (37, 53), (240, 321)) for k in H.REFUSED + (0, 11)]
    blobs += [b for group in RC.cases().values() for b in group]
    n = len(blobs)
    host = decode.stage_coefs_images(blobs, workers=3)
    assert host.status == [OK] * n
    st = decode.stage_bytes_images(blobs, workers=3, restarts=True)
    progressive = [i for i in range(18) if (H.REFUSED + (0, 11))[i % 6] in (7, 8, 13)]
    assert [rc != OK for rc in st.status] == [i in progressive for i in range(n)]
    assert all(st.status[i] == UNSUPPORTED and st.descs[i].n_comp == 0 and st.scans[i].blocks_in_mcu == 0 for i in progressive)
    with_ri = [i for i in range(n) if st.scans[i].restart_interval != 0]
    assert len(with_ri) == 3 + sum(len(g) for g in RC.cases().values())
    for one_piece in (False, True):
        rc, slots, status = _twin(st, one_piece)
        assert rc == OK and [s != OK for s in status] == [i in progressive for i in range(n)]
        _equal_host(st, slots, status, host)
    # without the flag the restart files are handed back and the others are unaffected
    plain = decode.stage_bytes_images(blobs, workers=3)
    assert [rc != OK for rc in plain.status] == [i in progressive or i in with_ri for i in range(n)]
    assert all(plain.status[i] == UNSUPPORTED for i in with_ri)
    rc, slots, status = _twin(plain)
    assert rc == OK and [s == OK for s in status] == [rc == OK for rc in plain.status]
    assert len(_equal_host(plain, slots, status, host)) == n - len(progressive) - len(with_ri)


def _odd_files():
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    ex = Image.Exif()
    ex[0x0112] = 6
    rot = io.BytesIO()
    Image.fromarray(arr).save(rot, "JPEG", exif=ex.tobytes())
    cmyk = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (20, 30, 4), dtype=np.uint8), "CMYK").save(cmyk, "JPEG")
    good = R.blob(37, 53, 0)
    return {"png": synth.encode_png(arr[:18, :26].copy()), "cmyk": cmyk.getvalue(), "exif6": rot.getvalue(),
            "truncated": good[:len(good) // 2], "empty": b""}


def test_record_layout_and_statuses():
    odd = _odd_files()
    good = [R.blob(17, 33, 0), R.blob(240, 321, 2), R.blob(1, 1, 11), R.blob(37, 53, 9)]
    blobs = [good[0], odd["png"], good[1], odd["cmyk"], odd["exif6"], good[2], odd["truncated"], odd["empty"], good[3]]
    n = len(blobs)
    images, layout_status, total = decode.images_layout(blobs, workers=2)
    ptrs, sizes, status, keep = decode._blob_table(blobs)
    offsets, used = (C.c_int64 * n)(*([-7] * n)), C.c_int64(-1)
    assert _lib.lib().llfe_jpeg_records_layout(sizes, images, n, offsets, C.byref(used)) == OK
    run = 0
    for i, b in enumerate(blobs):  # the running sum, 16-byte aligned; slot_bytes == 0 takes no room
        assert offsets[i] == run and run % 16 == 0
        if images[i].slot_bytes:
            run += _lib.JPEG_RECORD_HEADER + _up16(len(b)) + 16
    assert used.value == run
    assert [m.slot_bytes == 0 for m in images] == [i in (1, 3, 4, 7) for i in range(n)]
    st = decode.stage_bytes_images(blobs, workers=2)
    assert st.used_bytes == run
    # each odd file has the status the header stage or llfe_jpeg_parse_batch gives it, and zeroed records
    alone = decode.stage_bytes([odd["truncated"]], workers=1, size=(37, 53))
    assert alone.status == [UNSUPPORTED] and layout_status[6] == OK
    want = [OK, layout_status[1], OK, layout_status[3], layout_status[4], OK, alone.status[0], layout_status[7], OK]
    assert st.status == want and all(s != OK for i, s in enumerate(want) if i in (1, 3, 4, 6, 7))
    for i in (1, 3, 4, 6, 7):
        assert bytes(st.descs[i]) == bytes(_lib.LlfeJpegDesc()) and bytes(st.scans[i]) == bytes(_lib.LlfeJpegScan())
    for i in (0, 2, 5, 8):
        assert st.scans[i].record_offset == offsets[i]
    host = decode.stage_coefs_images(blobs, workers=2)
    for one_piece in (False, True):
        rc, slots, status = _twin(st, one_piece)
        assert rc == OK and [s == OK for s in status] == [i in (0, 2, 5, 8) for i in range(n)]
        assert _equal_host(st, slots, status, host) == [0, 2, 5, 8]
    # NULL arguments and a negative count
    assert _lib.lib().llfe_jpeg_records_layout(sizes, images, n, offsets, None) == INVALID
    assert _lib.lib().llfe_jpeg_records_layout(sizes, images, -1, offsets, C.byref(used)) == INVALID
    assert _lib.lib().llfe_jpeg_records_layout(None, None, 0, None, C.byref(used)) == OK and used.value == 0


def _parse(blobs, images, offsets, staging, staging_bytes, flags=0, fill=0x5A):
    """llfe_jpeg_parse_images with prefilled outputs: -> (rc, descs, scans, status list)."""
    n = len(blobs)
    descs, scans = (_lib.LlfeJpegDesc * n)(), (_lib.LlfeJpegScan * n)()
    C.memset(descs, fill, C.sizeof(descs))
    C.memset(scans, fill, C.sizeof(scans))
    ptrs, sizes, status, keep = decode._blob_table(blobs)
    for i in range(n):
        status[i] = 99
    rc = _lib.lib().llfe_jpeg_parse_images(ptrs, sizes, n, images, offsets, staging.ctypes.data, staging_bytes, descs, scans,
                                           status, 2, flags)
    return rc, descs, scans, list(status)


def test_refusals_before_any_work():
    blobs = [R.blob(37, 53, 0), R.blob(17, 33, 2), R.blob(240, 321, 11)]
    n = len(blobs)
    st = decode.stage_bytes_images(blobs, workers=1)
    assert st.status == [OK] * n
    offsets = (C.c_int64 * n)(*[s.record_offset for s in st.scans])
    used = st.used_bytes

    def refused_parse(offs=None, staging_bytes=used, flags=0):
        staging = np.full(used + GUARD, 0x5A, np.uint8)
        rc, descs, scans, status = _parse(blobs, st.images, offs or offsets, staging, staging_bytes, flags)
        assert rc == INVALID and status == [99] * n and (staging == 0x5A).all()
        assert bytes(descs) == b"\x5a" * C.sizeof(descs) and bytes(scans) == b"\x5a" * C.sizeof(scans)

    refused_parse((C.c_int64 * n)(offsets[0], offsets[1], used - 16))  # a record outside
    refused_parse((C.c_int64 * n)(offsets[0], offsets[1], -16))
    refused_parse((C.c_int64 * n)(offsets[0], offsets[1] + 8, offsets[2]))  # misaligned
    refused_parse(staging_bytes=used - 1)  # one byte short
    refused_parse(flags=2)  # an unknown flag bit
    refused_parse(flags=_lib.JPEG_PARSE_RESTARTS | 0x80)
    staging = np.full(used + GUARD, 0x5A, np.uint8)
    rc, descs, scans, status = _parse(blobs, st.images, offsets, staging, used)
    assert rc == OK and status == [OK] * n and (staging[used:] == 0x5A).all()
    assert bytes(descs) == bytes(st.descs) and bytes(scans) == bytes(st.scans)
    for s in scans:  # what a record holds: its header and its scan, zero padded
        a, b = s.record_offset, s.record_offset + _lib.JPEG_RECORD_HEADER + _up16(s.scan_bytes) + 16
        assert np.array_equal(staging[a:b], st.records[a:b])

    def refused_twin(edit=None, **kw):
        images = (_lib.LlfeJpegImage * n).from_buffer_copy(st.images)
        if edit:
            edit(images)
        rc, slots, status = _twin(st, images=images, fill=77, **kw)
        assert rc == INVALID and (slots == 77).all() and status == [99] * n

    def slot_outside(m):
        m[2].slot_offset = st.slot_bytes - m[2].slot_bytes + 16

    def slot_negative(m):
        m[0].slot_offset = -16

    def slot_misaligned(m):
        m[1].slot_offset += 8

    def slots_overlap(m):
        m[1].slot_offset = m[0].slot_offset + m[0].slot_bytes - 16

    def slots_same(m):
        m[0].slot_offset = m[2].slot_offset

    def wrong_size(m):
        m[0].height += 8

    for edit in (slot_outside, slot_negative, slot_misaligned, slots_overlap, slots_same, wrong_size):
        refused_twin(edit)
    refused_twin(slot_bytes=st.slot_bytes - 16)  # the last slot past slots_bytes
    last = st.scans[n - 1]  # the last record's scan and its padding past staging_bytes
    refused_twin(used_bytes=last.record_offset + _lib.JPEG_RECORD_HEADER + _up16(last.scan_bytes) + 16 - 1)
    rc, slots, status = _twin(st, fill=77)
    assert rc == OK and status == [OK] * n


def _noise_tail(good):
    noise = bytearray(good)  # the second half of the scan replaced by noise without FF bytes
    begin, end = H._scan_span(good)
    noise[(begin + end) // 2:end] = np.random.default_rng(8).integers(0, 255, end - (begin + end) // 2,
                                                                      dtype=np.uint8).tobytes()
    return bytes(noise)


def test_damaged_files_beside_good_neighbours():
    good = R.blob(240, 321, 0)
    src = RC.damaged_source()
    damaged = [H.flipped(good), H.cut(good), _noise_tail(good)] + [f(src) for f in RC.DAMAGES]
    neighbours = [R.blob(17, 33, 2), good, src, R.blob(37, 53, 11), RC.small(restart_marker_blocks=1)]
    blobs, bad = [], []
    for k, d in enumerate(damaged):  # every damaged file between two good ones
        blobs += [neighbours[k % len(neighbours)], d]
        bad.append(len(blobs) - 1)
    blobs.append(neighbours[-1])
    n = len(blobs)
    st = decode.stage_bytes_images(blobs, workers=3, restarts=True)
    host = decode.stage_coefs_images(blobs, workers=3)
    assert all(st.status[i] == OK for i in range(n) if i not in bad)
    for one_piece in (False, True):
        rc, slots, status = _twin(st, one_piece)
        assert rc == OK
        for i in range(n):
            if i not in bad:
                assert status[i] == OK, i
            elif i != bad[0]:  # handed back, by the parser or by the twin
                assert status[i] == UNSUPPORTED, i
            # (a flipped byte may leave a valid file of another image: then the slot is the host's)
        took = _equal_host(st, slots, status, host)
        assert set(range(n)) - set(bad) <= set(took)
