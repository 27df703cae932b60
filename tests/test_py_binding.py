"""The shared helpers of the Python binding, CPU only: backend._image_descs (the descriptor
builder of process_images and submit_images), decode's one staging ring seen through the public
stage_* functions, and decode._renumber."""
import numpy as np
import pytest
import torch

from low_level_feature_extraction_amd import decode, synth
from low_level_feature_extraction_amd.backend import _image_descs
from tests import jpeg_restate as R

H, W = 6, 10


def _pixels(h=H, w=W, c=3):
    return np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, c), dtype=np.uint8)


def _np(a):
    return a, a.ctypes.data, a.strides[0]


def _pt(a):
    """The torch twin of a numpy case (from_numpy shares the memory, so the pointers agree)."""
    t = torch.from_numpy(a)
    return t, t.data_ptr(), t.stride(0)


def _one(im):
    """_image_descs of one image -> (its record, the array / tensor the record points into)."""
    descs, keep, hs, ws, first = _image_descs([im], 0)
    assert len(descs) == len(keep) == 1 and first is None
    assert (hs, ws) == ([im.shape[0]], [im.shape[1]])
    d = descs[0]
    assert (d["height"], d["width"], d["on_device"]) == (im.shape[0], im.shape[1], 0)
    assert (d["noise"], d["noise_on_device"]) == (0, 0)
    return d, keep[0]


def _packed_copy(d, kept, want):
    """The record points at one packed copy of `want`, not at the input."""
    ptr = kept.data_ptr() if isinstance(kept, torch.Tensor) else kept.ctypes.data
    assert d["data"] == ptr and d["row_stride"] == 3 * want.shape[1]
    assert np.array_equal(np.asarray(kept), want) and np.asarray(kept).flags.c_contiguous


@pytest.mark.parametrize("wrap", [_np, _pt], ids=["numpy", "torch"])
def test_image_descs_reads_packed_and_row_strided_images_in_place(wrap):
    im, ptr, _ = wrap(_pixels())
    d, kept = _one(im)
    assert kept is im and (d["data"], d["row_stride"]) == (ptr, 3 * W)
    buf = wrap(_pixels(H, 16))[0]
    view = buf[:, 3:3 + W]  # rows 48 bytes apart, pixels packed: no copy
    d, kept = _one(view)
    vptr = view.data_ptr() if wrap is _pt else view.ctypes.data
    assert kept is view and (d["data"], d["row_stride"]) == (vptr, 48)
    col, ptr, _ = wrap(_pixels(H, 1))  # a 1-column image
    d, kept = _one(col)
    assert kept is col and (d["data"], d["row_stride"], d["width"]) == (ptr, 3, 1)


@pytest.mark.parametrize("wrap", [_np, _pt], ids=["numpy", "torch"])
def test_image_descs_copies_unpacked_pixels_and_overlapping_rows_once(wrap):
    a = _pixels()
    if wrap is _np:  # channel-reversed: pixel stride -1 (torch has no negative strides)
        rev = a[:, :, ::-1]
        d, kept = _one(rev)
        assert d["data"] != rev.ctypes.data
        _packed_copy(d, kept, a[:, :, ::-1])
    four = wrap(_pixels(H, W, 4))[0]  # three of four channels: pixels 4 bytes apart
    d, kept = _one(four[:, :, :3])
    _packed_copy(d, kept, np.asarray(four)[:, :, :3])
    row = wrap(a[:1])[0]
    bcast = np.broadcast_to(row, (H, W, 3)) if wrap is _np else row.expand(H, W, 3)  # row stride 0
    d, kept = _one(bcast)
    assert d["data"] != (row.ctypes.data if wrap is _np else row.data_ptr())
    _packed_copy(d, kept, np.broadcast_to(a[:1], (H, W, 3)))


@pytest.mark.parametrize("wrap", [_np, _pt], ids=["numpy", "torch"])
def test_image_descs_names_the_image_it_refuses(wrap):
    good = wrap(_pixels())[0]
    for bad in (_pixels().astype(np.int16), _pixels()[:, :, 0], _pixels(H, W, 2)):
        with pytest.raises(ValueError, match=r"^image 1: expected H x W x 3 uint8"):
            _image_descs([good, wrap(np.ascontiguousarray(bad))[0]], 0)


def test_image_descs_fills_one_record_per_image_in_order():
    ims = [_pixels(4, 5), torch.from_numpy(_pixels(7, 3)), _pixels(H, 16)[:, :W]]
    descs, keep, hs, ws, first = _image_descs(ims, 0)
    assert (hs, ws, first) == ([4, 7, H], [5, 3, W], None)
    assert descs["data"].tolist() == [ims[0].ctypes.data, ims[1].data_ptr(), ims[2].ctypes.data]
    assert descs["row_stride"].tolist() == [15, 9, 48] and descs["on_device"].tolist() == [0, 0, 0]
    assert descs["height"].tolist() == hs and descs["width"].tolist() == ws
    assert len(_image_descs([], 0)[0]) == 0


def _png16(i):
    return synth.encode_png(synth.synth_numpy(i, 16, 16, seed=6))


def _jpeg16(i):
    return R.jpeg(synth.synth_numpy(i, 16, 16, seed=6)[:, :, ::-1].copy(), quality=85)


def test_stage_png_ring():
    blobs = [_png16(0), _jpeg16(1), _png16(2)]
    seen = []
    for _ in range(4):
        sp = decode.stage_png(blobs, workers=2)
        assert sp.status == [0, -5, 0] and (sp.h, sp.w) == (16, 16)
        assert sp.used_bytes <= sp.records.shape[1] and sp.records.shape[1] % 16 == 0
        seen.append(sp.records.ctypes.data)
    assert len(set(seen[:3])) == 3 and seen[3] == seen[0]  # a ring of three staging buffers


def test_fifth_batch_shape_drops_a_familys_other_rings_and_no_other_familys():
    """A family keeps the rings of four (count, stride) keys; the fifth key drops the others, so
    a batch shape staged again after that gets new buffers.  The rings of another family stay.
    The slot size is one no other test stages with, so the five keys are new to the family
    whatever ran before; the staged batches are kept, so a new buffer cannot take a dropped
    one's address."""
    jpeg, png = _jpeg16(3), _png16(4)
    slot = decode.coef_slot_bytes(16, 16) + 48
    other = decode.stage_png([png] * 7, workers=1).records.ctypes.data
    held = [decode.stage_coefs([jpeg], workers=1, slot_bytes=slot) for _ in range(4)]
    assert all(st.status == [0] for st in held)
    old = [st.slots.ctypes.data for st in held]
    assert len(set(old[:3])) == 3 and old[3] == old[0]
    for n in (2, 3, 4, 5):
        assert decode.stage_coefs([jpeg] * n, workers=1, slot_bytes=slot).slots.shape == (n, slot)
    again = [decode.stage_coefs([jpeg], workers=1, slot_bytes=slot) for _ in range(4)]
    new = [st.slots.ctypes.data for st in again]
    assert not set(new) & set(old)
    assert len(set(new[:3])) == 3 and new[3] == new[0]
    assert [decode.stage_png([png] * 7, workers=1).records.ctypes.data for _ in range(3)][2] == other


def test_renumber_names_the_image_by_its_place_in_the_whole_batch():
    def renumbered(msg):
        e = decode._renumber(decode.DecodeError(msg), [4, 7])
        assert isinstance(e, decode.DecodeError)
        return str(e)

    assert renumbered("image 1: x") == "image 7: x"
    assert renumbered("Failed to decode image") == "Failed to decode image"
    assert renumbered("imagine 1: x") == "imagine 1: x"
