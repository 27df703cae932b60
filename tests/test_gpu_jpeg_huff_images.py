"""JPEG entropy decode of a batch of images of any sizes on the device (csrc/jpeg_huff.hip behind
decode.decode_images_device(entropy="device")): the tight coefficient slots the kernels write
equal the ones the host stages (decode.stage_coefs_images: libjpeg-turbo's
jpeg_read_coefficients) over every byte an image occupies, and every decoded image equals
decode.decode_bgr -- for the whole case list of tests/jpeg_restate.py in one call, for a batch
whose images have one to many workgroups of subsequences (the per-image offsets into the
workspace, more passes than the small images have workgroups, the launch of the undecided suffix
only), for both kernel instances in one batch, for damaged files between good ones, for every
fallback, and in chunks.  Records that point outside their buffers are refused by the host check
before any launch.  tests/test_jpeg_huff_images_host.py checks the same inputs against the
kernels' host twin on the CPU."""
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from low_level_feature_extraction_amd.image_processor import ImageProcessor
from tests import jpeg_huff_cases as H
from tests import jpeg_restart_cases as RC
from tests import jpeg_restate as R

pytestmark = pytest.mark.gpu
GUARD = 4096


def _device_slots(blobs, restarts=False):
    """The device's status per image, after checking every slot it took against the host's."""
    import torch

    sb = decode.stage_bytes_images(blobs, workers=2, restarts=restarts)
    buf = torch.full((sb.slot_bytes + GUARD,), 0xC3, dtype=torch.uint8, device="cuda:0")
    d_slots, descs, status = decode.entropy_decode_staged_images(sb, slots=buf[:sb.slot_bytes])
    st = decode.stage_coefs_images(blobs, workers=2)
    got = buf.cpu().numpy()
    assert (got[sb.slot_bytes:] == 0xC3).all(), "the guard behind the coefficient tensor was written"
    for i, rc in enumerate(status):
        if rc == 0:
            m, want = sb.images[i], st.images[i]
            assert st.status[i] == 0 and bytes(sb.descs[i]) == bytes(st.descs[i])
            assert (m.slot_offset, m.slot_bytes) == (want.slot_offset, want.slot_bytes)
            a, b = m.slot_offset, m.slot_offset + m.slot_bytes
            assert H.slots_equal(got[a:b], st.slots[a:b], st.descs[i]), f"slot {i} differs"
            assert descs[i].n_comp == st.descs[i].n_comp
        else:
            assert descs[i].n_comp == 0
    return status


def _want(b):
    try:
        return decode.decode_bgr(b)
    except decode.DecodeError as e:
        return e


def _same(blobs, **kw):
    got = decode.decode_images_device(blobs, workers=2, entropy="device", **kw)
    assert len(got) == len(blobs)
    for i, b in enumerate(blobs):
        want = _want(b)
        if isinstance(want, Exception):
            assert isinstance(got[i], decode.DecodeError), i
        else:
            assert not isinstance(got[i], Exception) and got[i].is_cuda and tuple(got[i].shape) == want.shape, i
            assert np.array_equal(got[i].cpu().numpy(), want), f"image {i} differs"
    return got


def _lanes(b, restarts=False):
    return -(-len((RC if restarts else H).scan_bytes(b)) // H.SUB)


def _case_list():
    return [R.blob(h, w, k) for (h, w, k) in R.CASES if k in H.ACCEPTED]


def test_case_list_in_one_call(backend):
    """All seven sizes and every baseline setting in one ragged call: all taken by the device."""
    blobs = _case_list()
    assert len(blobs) == len(R.SIZES) * len(H.ACCEPTED)
    assert _device_slots(blobs) == [0] * len(blobs)
    _same(blobs)


@pytest.mark.parametrize("reverse", [False, True])
def test_workgroup_bookkeeping(backend, reverse):
    """One lane up to many workgroups of lanes in one batch: the images' offsets into the
    workspace, passes that outnumber the small images' workgroups, and the suffix launch; the
    flat 2048 x 2048 files are phase-locked and need the true state carried across launches."""
    tiny = R.jpeg(np.random.default_rng(3).integers(0, 256, (8, 8), dtype=np.uint8), quality=1)
    lengths = (H.SUB - 2, H.SUB - 1, H.SUB, H.SUB + 1, H.SUB + 3, 2 * H.SUB - 2, 2 * H.SUB, 2 * H.SUB + 1, 2 * H.SUB + 3)
    seams = [H.scan_of_length(t) for t in lengths]
    boundary, hits = H.stuffed_boundary()
    one_wg = R.blob(240, 321, 0)
    two_wg = R.jpeg(np.random.default_rng(5).integers(0, 256, (96, 160, 3), dtype=np.uint8), quality=95, subsampling=0)
    flats = [H.flat(2, False, 2048), H.flat(2, True, 2048)]
    assert _lanes(tiny) == 1 and [len(H.scan_bytes(b)) for b in seams] == list(lengths) and hits
    assert 1 < _lanes(one_wg) <= 256 < _lanes(two_wg) <= 512 and min(_lanes(b) for b in flats) > 2 * 256
    blobs = [tiny] + seams + [boundary, one_wg, two_wg] + flats
    if reverse:
        blobs = blobs[::-1]
    assert _device_slots(blobs) == [0] * len(blobs)
    _same(blobs)


def test_both_kernel_instances_in_one_batch(backend):
    """Files with and without restart intervals, of several sizes, in one call."""
    seams = [RC.seam(r) for r in RC.SEAMS]
    assert all(off % H.SUB == r for (b, off), r in zip(seams, RC.SEAMS))
    blobs = [R.blob(17, 33, 0), RC.flat(8), R.blob(240, 321, 2), RC.striped()] + [b for b, _ in seams] + \
            [H.flat(2, True, 512), R.blob(37, 53, 10), R.blob(1, 1, 11)]
    assert _lanes(blobs[1], True) > 2 * 256
    assert _device_slots(blobs, restarts=True) == [0] * len(blobs)
    _same(blobs, restarts=True)
    # without the flag the restart files take the host coefficient path: the same bytes
    status = _device_slots(blobs)
    assert [rc == 0 for rc in status] == [i in (0, 2, 8, 10) for i in range(len(blobs))]
    _same(blobs)


def _noise_tail(good):
    noise = bytearray(good)  # the second half of the scan replaced by noise without FF bytes
    begin, end = H._scan_span(good)
    noise[(begin + end) // 2:end] = np.random.default_rng(8).integers(0, 255, end - (begin + end) // 2,
                                                                      dtype=np.uint8).tobytes()
    return bytes(noise)


def test_damaged_files_between_good_ones(backend):
    """Handed back by the device, decoded by the fallback chain; the neighbours are the device's."""
    good, src = R.blob(240, 321, 0), RC.damaged_source()
    damaged = [H.flipped(good), H.cut(good), _noise_tail(good)] + [f(src) for f in RC.DAMAGES]
    neighbours = [R.blob(17, 33, 2), good, src, R.blob(37, 53, 11), RC.small(restart_marker_blocks=1)]
    blobs, bad = [], []
    for k, d in enumerate(damaged):
        blobs += [neighbours[k % len(neighbours)], d]
        bad.append(len(blobs) - 1)
    blobs.append(neighbours[-1])
    status = _device_slots(blobs, restarts=True)
    for i, rc in enumerate(status):
        if i not in bad:
            assert rc == 0, i
        elif i != bad[0]:  # (a flipped byte may leave a valid file of another image)
            assert rc == H.UNSUPPORTED, i
    _same(blobs, restarts=True)


def _fallback_batch():
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    ex = Image.Exif()
    ex[0x0112] = 6
    rot = io.BytesIO()
    Image.fromarray(arr).save(rot, "JPEG", exif=ex.tobytes())
    cmyk = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (20, 30, 4), dtype=np.uint8), "CMYK").save(cmyk, "JPEG")
    good = R.blob(37, 53, 0)
    return [R.blob(17, 33, 0), synth.encode_png(arr[:18, :26].copy()), R.blob(37, 53, 7), cmyk.getvalue(), good,
            rot.getvalue(), good[:len(good) // 2], b"\xff\xd8\xff\xe0 not a jpeg", R.blob(240, 321, 13), R.blob(16, 16, 11)]


def test_fallbacks_in_one_batch(backend):
    """A PNG, progressive files (the host coefficient path), a CMYK file, an EXIF-6 file (its
    decoded size is the transposed one), a truncated file and bytes nothing decodes."""
    blobs = _fallback_batch()
    status = _device_slots(blobs)
    assert [rc == 0 for rc in status] == [i in (0, 4, 9) for i in range(len(blobs))]
    st = decode.stage_coefs_images(blobs, workers=2)
    assert st.status[2] == st.status[8] == 0  # the progressive files: coefficients from the host
    got = _same(blobs)
    want = decode.decode_many(blobs, workers=2)
    for g, w in zip(got, want):
        assert isinstance(g, Exception) == isinstance(w, Exception)
        if not isinstance(w, Exception):
            assert np.array_equal(g.cpu().numpy(), w)
    assert isinstance(got[7], decode.DecodeError) and tuple(got[5].shape) == (40, 24, 3)


def test_chunking(backend, monkeypatch):
    blobs = _case_list() + _fallback_batch()
    whole = [g if isinstance(g, Exception) else g.cpu().numpy() for g in _same(blobs)]
    images, _, total = decode.images_layout(blobs, workers=2)
    cap = 400000
    assert max(m.slot_bytes for m in images) > cap and total > 3 * cap  # three or more chunks, one image alone above it
    monkeypatch.setenv("LLFE_JPEG_STAGE_BYTES", str(cap))
    got = _same(blobs)
    for g, w in zip(got, whole):
        assert isinstance(g, Exception) == isinstance(w, Exception)
        if not isinstance(w, Exception):
            assert np.array_equal(g.cpu().numpy(), w)


def test_refusals_by_the_device_entry(backend):
    """Host checks: nothing reaches the device, the coefficient tensor stays as it was."""
    import torch

    blobs = [R.blob(37, 53, 0), R.blob(17, 33, 2), R.blob(240, 321, 11)]
    sb = decode.stage_bytes_images(blobs, workers=1)
    assert sb.status == [0, 0, 0]
    records = torch.from_numpy(sb.records[:sb.used_bytes].copy()).cuda()

    def refused(edit, slot_bytes=sb.slot_bytes):
        images = (_lib.LlfeJpegImage * 3).from_buffer_copy(sb.images)
        scans = (_lib.LlfeJpegScan * 3).from_buffer_copy(sb.scans)
        edit(images, scans)
        slots = torch.full((slot_bytes,), 77, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(_lib.LlfeError) as e:
            backend.jpeg_entropy_decode_images(records, scans, sb.descs, images, slots)
        assert e.value.code == _lib.LLFE_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((slots == 77).all())  # no kernel ran: not even the valid images were written

    def slots_overlap(m, s):
        m[1].slot_offset = m[0].slot_offset + m[0].slot_bytes - 16

    def slot_past_tensor(m, s):
        m[2].slot_offset += 16

    def slot_misaligned(m, s):
        m[0].slot_offset += 8

    def record_outside(m, s):
        s[2].record_offset = sb.used_bytes - 16

    def wrong_size(m, s):
        m[1].width += 16

    for edit in (slots_overlap, slot_past_tensor, slot_misaligned, record_outside, wrong_size):
        refused(edit)
    refused(lambda m, s: None, sb.slot_bytes - 16)
    slots = torch.full((sb.slot_bytes,), 77, dtype=torch.uint8, device="cuda:0")
    for bad in (lambda: backend.jpeg_entropy_decode_images(records.cpu(), sb.scans, sb.descs, sb.images, slots),
                lambda: backend.jpeg_entropy_decode_images(records, sb.scans, sb.descs, sb.images, slots.cpu()),
                lambda: backend.jpeg_entropy_decode_images(records, sb.scans, sb.descs, sb.images, slots.view(-1, 16)),
                lambda: backend.jpeg_entropy_decode_images(records, sb.scans[:2], sb.descs, sb.images, slots)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert bool((slots == 77).all())
    assert backend.jpeg_entropy_decode_images(records, sb.scans, sb.descs, sb.images, slots) == [0, 0, 0]


def test_auto_process_images_with_device_entropy(backend):
    blobs = [R.blob(240, 321, 0), R.blob(37, 53, 2), R.blob(240, 321, 10), R.blob(17, 33, 7), b"junk"]
    want = ImageProcessor.auto_process_images(blobs, 50, 40)  # the default route: two of them are resized
    assert np.asarray(want[0]).shape[:2] != (240, 321) and np.asarray(want[3]).shape[:2] == (17, 33)
    for kw in (dict(entropy="device"), dict(entropy="device", restarts=True)):
        got = ImageProcessor.auto_process_images(blobs, 50, 40, device=True, decode="device", **kw)
        assert len(got) == len(want) == 5
        for g, w in zip(got[:4], want[:4]):
            assert g.is_cuda and np.array_equal(g.cpu().numpy(), np.asarray(w))
        assert isinstance(got[4], ValueError) and isinstance(want[4], ValueError) and str(got[4]) == str(want[4])
    for kw in (dict(entropy="device"), dict(device=True, entropy="device"), dict(device=True, decode="device", restarts=True),
               dict(device=True, decode="device", entropy="gpu")):
        with pytest.raises(ValueError):
            ImageProcessor.auto_process_images(blobs, 50, 40, **kw)
