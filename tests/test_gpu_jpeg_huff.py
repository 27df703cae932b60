"""JPEG entropy decode on the device (csrc/jpeg_huff.hip behind
decode.decode_batch_device(entropy="device")): the coefficient slots the kernels write equal the
ones the host stages (decode.stage_coefs: libjpeg-turbo's jpeg_read_coefficients) over every
byte an image occupies, and the decoded batch equals decode.decode_batch, for the case list of
tests/jpeg_restate.py, for flat images that never self-synchronise (in one workgroup of
subsequences and across several), on the seams of the subsequence size, for mixed batches with
both fallbacks, and for corrupt scans, which are handed back rather than trusted.  A scan record
that points outside the staging buffer is refused by the host check before any launch.
tests/test_jpeg_parse.py checks the same inputs against the kernels' host twin on the CPU."""
import dataclasses
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from tests import jpeg_huff_cases as H
from tests import jpeg_restate as R

pytestmark = pytest.mark.gpu


def _device_slots(blobs):
    """The device's status per image, after checking every slot it took against the host's."""
    sb = decode.stage_bytes(blobs, workers=2)
    d_slots, descs, status = decode.entropy_decode_staged(sb)
    st = decode.stage_coefs(blobs, workers=2)
    got = d_slots.cpu().numpy()
    for i, rc in enumerate(status):
        if rc == 0:
            assert st.status[i] == 0 and bytes(sb.descs[i]) == bytes(st.descs[i])
            assert H.slots_equal(got[i], st.slots[i], st.descs[i]), f"slot {i} differs"
            assert descs[i].n_comp == st.descs[i].n_comp
        else:
            assert descs[i].n_comp == 0
    return status


def _same(blobs):
    want = decode.decode_batch(blobs, workers=2)
    got = decode.decode_batch_device(blobs, workers=2, entropy="device")
    assert tuple(got.shape) == want.shape and got.is_cuda
    got = got.cpu().numpy()
    for i in range(len(blobs)):
        assert np.array_equal(got[i], want[i]), f"image {i} differs at {np.argwhere(got[i] != want[i])[:4].tolist()}"
    return got


@pytest.mark.parametrize("h,w", R.SIZES)
def test_case_list_equals_host(backend, h, w):
    """Every baseline setting (4:4:4 / 4:2:2 / 4:2:0 / grey, quality 1..100, optimised tables) at
    one size per call: all taken by the device, none by a fallback."""
    blobs = [R.blob(h, w, k) for k in H.ACCEPTED]
    assert _device_slots(blobs) == [0] * len(blobs)
    _same(blobs)


@pytest.mark.parametrize("size", [512, 2048])
@pytest.mark.parametrize("sub", [2, 1, 0])
def test_phase_locked_images(backend, sub, size):
    """Flat colour, with and without a noise stripe: at 4:2:0 the 512 x 512 one is 33
    subsequences none of which finds the true state by itself; the 2048 x 2048 ones span three
    and more workgroups of subsequences, so the true state also has to cross the launches."""
    blobs = [H.flat(sub, False, size), H.flat(sub, True, size)]
    lanes = [-(-len(H.scan_bytes(b)) // H.SUB) for b in blobs]
    assert lanes[0] == 33 if (sub, size) == (2, 512) else True
    assert min(lanes) > 2 * 256 if size == 2048 else True
    assert _device_slots(blobs) == [0, 0]
    _same(blobs)


def test_seams_of_the_subsequence_size(backend):
    tiny = R.jpeg(np.random.default_rng(3).integers(0, 256, (8, 8), dtype=np.uint8), quality=1)
    assert len(H.scan_bytes(tiny)) < H.SUB
    assert _device_slots([tiny]) == [0]
    _same([tiny])
    # scans a few bytes either side of one and of two subsequences (one batch: 16 x 16 grey)
    lengths = (H.SUB - 2, H.SUB - 1, H.SUB, H.SUB + 1, H.SUB + 3, 2 * H.SUB - 2, 2 * H.SUB, 2 * H.SUB + 1, 2 * H.SUB + 3)
    blobs = [H.scan_of_length(t) for t in lengths]
    assert [len(H.scan_bytes(b)) for b in blobs] == list(lengths)
    assert _device_slots(blobs) == [0] * len(blobs)
    _same(blobs)
    # quality-100 noise: long codes, many FF 00 pairs, one of them across a subsequence boundary
    blob, hits = H.stuffed_boundary()
    d = H.scan_bytes(blob)
    assert hits and all(d[k] == 0 and d[k - 1] == 0xFF and k % H.SUB == 0 for k in hits)
    assert _device_slots([blob]) == [0]
    _same([blob])


@pytest.mark.parametrize("h,w", [(17, 33), (9, 260)])
def test_odd_block_grids_and_optimised_tables(backend, h, w):
    """MCU padding in both directions at 4:2:0; optimize=True tables."""
    rng = np.random.default_rng(8)
    blobs = [R.jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality=q, subsampling=2, optimize=o)
             for q, o in ((85, False), (100, False), (60, True), (30, True))]
    assert _device_slots(blobs) == [0] * len(blobs)
    _same(blobs)


def test_mixed_batch_with_both_fallbacks(backend):
    h, w = 72, 100
    imgs = [synth.synth_numpy(i, h, w, seed=9) for i in range(12)]
    rgb = [im[:, :, ::-1].copy() for im in imgs]
    ex = Image.Exif()
    ex[0x0112] = 3  # rotate 180: the same size after exif_transpose
    rot = io.BytesIO()
    Image.fromarray(rgb[10]).save(rot, "JPEG", exif=ex.tobytes())
    blobs = [R.jpeg(rgb[0], quality=90, subsampling=0), R.jpeg(rgb[1], quality=80, subsampling=1),
             R.jpeg(rgb[2], quality=70, subsampling=2), R.jpeg(rgb[3][:, :, 1].copy(), quality=85),
             R.jpeg(rgb[4], quality=88, progressive=True), synth.encode_png(imgs[5]),
             R.jpeg(rgb[6], quality=30, subsampling=2, optimize=True), R.jpeg(rgb[7], quality=95, subsampling=1),
             R.jpeg(rgb[8], quality=75, restart_marker_blocks=2), synth.encode_png(imgs[9]), rot.getvalue(),
             R.jpeg(rgb[11], quality=1, subsampling=0)]
    # the device takes the baseline files, the host coefficient path the progressive and the
    # restart-interval one, the host decoders the PNGs and the rotated file
    assert [rc == 0 for rc in _device_slots(blobs)] == [i in (0, 1, 2, 3, 6, 7, 11) for i in range(12)]
    st = decode.stage_coefs(blobs, workers=3)
    assert [rc != 0 for rc in st.status] == [i in (5, 9, 10) for i in range(12)]
    got = _same(blobs)
    assert np.array_equal(got[5], imgs[5]) and np.array_equal(got[9], imgs[9])
    assert np.array_equal(got[10], decode.decode_bgr(blobs[10]))


@pytest.mark.parametrize("damage", [H.flipped, H.cut])
def test_corrupt_scans_are_handed_back(backend, damage):
    """One byte flipped mid-stream; the last ten bytes of the scan missing.  Ordinary malformed
    files: the device decodes them inside its bounds and its verification (or the block count,
    or the end of the scan) hands them back, so the batch is what decode_batch makes of it and
    the neighbours are the device's own."""
    good = [R.blob(240, 321, 0), R.blob(240, 321, 9)]
    bad = damage(good[0])
    blobs = [good[0], bad, good[1]]
    status = _device_slots(blobs)
    assert status[0] == status[2] == 0
    if damage is H.cut:
        assert status[1] == H.UNSUPPORTED
    try:
        want = decode.decode_batch(blobs, workers=2)
    except decode.DecodeError as e:
        with pytest.raises(decode.DecodeError) as got:
            decode.decode_batch_device(blobs, workers=2, entropy="device")
        assert str(got.value) == str(e)
        return
    got = decode.decode_batch_device(blobs, workers=2, entropy="device").cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[1], H.host_result(bad))


@pytest.mark.parametrize("odd", [R.blob(16, 16, 0), b"\xff\xd8\xff\xe0 not a jpeg", R.blob(16, 16, 7)])
def test_errors_name_the_image_as_decode_batch_does(backend, odd):
    """An image of another size, or one nothing decodes, behind images the device took: the
    error is decode_batch's, with the image's place in the whole batch."""
    blobs = [R.blob(37, 53, 0), R.blob(37, 53, 2), odd, R.blob(37, 53, 11)]
    with pytest.raises(decode.DecodeError) as want:
        decode.decode_batch(blobs, workers=2)
    assert str(want.value).startswith("image 2:")
    with pytest.raises(decode.DecodeError) as got:
        decode.decode_batch_device(blobs, workers=2, entropy="device")
    assert str(got.value) == str(want.value)


def test_record_outside_the_staging_buffer_is_refused_on_the_host(backend):
    import torch

    blobs = [R.blob(37, 53, k) for k in (0, 2, 11)]
    sb = decode.stage_bytes(blobs, workers=1)
    assert sb.status == [0, 0, 0]
    records = torch.from_numpy(sb.records).cuda()

    def refused(edit):
        scans = (_lib.LlfeJpegScan * 3).from_buffer_copy(sb.scans)
        descs = (_lib.LlfeJpegDesc * 3).from_buffer_copy(sb.descs)
        edit(scans, descs)
        slots = torch.full((3, sb.slot_bytes), 77, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(_lib.LlfeError) as e:
            backend.jpeg_entropy_decode(records, scans, descs, 37, 53, slots)
        assert e.value.code == _lib.LLFE_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((slots == 77).all())  # no kernel ran: not even the valid images were written

    def scan_too_long(s, d):
        s[2].scan_bytes = sb.records.shape[1]

    def scan_negative(s, d):
        s[0].scan_offset = -16

    def table_outside(s, d):
        s[1].table_offset = sb.records.size

    def record_outside(s, d):
        s[2].record_offset = sb.records.size - 16

    def selector(s, d):
        s[0].blk_dc[0] = 2

    def grid_too_small(s, d):
        s[0].mcus_h -= 1

    def coef_outside(s, d):
        d[1].comp[2].coef_offset = sb.slot_bytes - 64

    for edit in (scan_too_long, scan_negative, table_outside, record_outside, selector, grid_too_small, coef_outside):
        refused(edit)
    slots = torch.full((3, sb.slot_bytes), 77, dtype=torch.uint8, device="cuda:0")
    assert backend.jpeg_entropy_decode(records, sb.scans, sb.descs, 37, 53, slots) == [0, 0, 0]


def test_out_tensor_and_process_equal_host_path(backend):
    import torch

    imgs = [synth.synth_numpy(i, 128, 160, seed=21) for i in range(4)]
    blobs = [R.jpeg(im[:, :, ::-1].copy(), quality=85, subsampling=(2, 1, 0, 2)[i]) for i, im in enumerate(imgs)]
    out = torch.zeros((4, 128, 160, 3), dtype=torch.uint8, device="cuda:0")
    dev = decode.decode_batch_device(blobs, out=out, entropy="device")
    assert dev.data_ptr() == out.data_ptr()
    host = decode.decode_batch(blobs)
    feats = ("colors", "shapes", "shadows")
    a = backend.process(dev, feats, seed=5)
    b = backend.process(host, feats, seed=5)
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        for f in dataclasses.fields(x):
            u, v = getattr(x, f.name), getattr(y, f.name)
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v, f.name
