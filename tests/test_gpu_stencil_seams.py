"""The row-streaming stencil at the seams of tests/stencil_cases.py: every stage entry point
bit-exact against the oracle -- edge_classes (k_stencil_stream<true, false>), shadow_stats
(<false, true>) and shape_mask -- and process() (<true, true>) on the marked shapes.
tests/test_stencil_seam_inputs.py proves on the CPU what each shape and image reaches."""
import numpy as np
import pytest

from tests import stencil_cases as SC

pytestmark = pytest.mark.gpu


def _check_stages(backend, h, w):
    x = np.array(SC.images(h, w))  # (the shared batch is read-only)
    cls, shadow, mask = SC.expected(h, w)
    got = backend.edge_classes(x).cpu().numpy()
    for i in range(len(x)):
        assert np.array_equal(got[i], cls[i]), f"classes, image {i}: {(got[i] != cls[i]).sum()} px differ"
    sums, cnts = backend.shadow_stats(x)
    assert [(int(s), int(c)) for s, c in zip(sums, cnts)] == shadow
    got = backend.shape_mask(x).cpu().numpy()
    for i in range(len(x)):
        assert np.array_equal(got[i], mask[i]), f"mask, image {i}: {(got[i] != mask[i]).sum()} px differ"


def _check_process(backend, orc, h, w):
    x = SC.images(h, w)
    _, shadow, mask = SC.expected(h, w)
    res = backend.process(np.array(x), ("shapes", "shadows"))
    for i, r in enumerate(res):
        assert (r.shadow_sum, r.shadow_count) == shadow[i], i
        assert r.n_contours == len(orc.find_contours_external(mask[i])), i
        assert r.shapes == orc.analyze_shapes(x[i])["shapes"], i


@pytest.mark.parametrize("h", sorted({h for h, _ in SC.G1}))
def test_narrow_images(backend, h):
    for hh, w in SC.G1:
        if hh == h:
            _check_stages(backend, h, w)


@pytest.mark.parametrize("h,w", SC.G2 + SC.G3 + SC.G4)
def test_strip_and_segment_seams(backend, orc, h, w):
    _check_stages(backend, h, w)
    if (h, w) in SC.PROCESS:
        _check_process(backend, orc, h, w)


def _at_offset(torch, arr, off):
    """A contiguous device copy of arr at a 16-byte-aligned address + off."""
    buf = torch.zeros(arr.size + 32, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 16
    t = buf[base + off: base + off + arr.size].view(arr.shape)
    t.copy_(torch.from_numpy(np.array(arr)))
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t, buf


@pytest.mark.parametrize("h,w", SC.G5)
def test_misaligned_pointers_take_the_byte_path(backend, h, w):
    """W % 4 == 0 with bgr (or the class map) off the 4-byte grid: every strip, interior
    ones included, loads and stores bytes.  Same results as the aligned run and the oracle."""
    import torch

    x = SC.images(h, w)
    n = len(x)
    cls, shadow, _ = SC.expected(h, w)
    assert np.array_equal(backend.edge_classes(np.array(x)).cpu().numpy(), cls)  # the aligned run
    for off in (1, 2, 3):
        xd, keep = _at_offset(torch, x, off)
        out = torch.empty((n, h, w), dtype=torch.uint8, device=xd.device)
        backend._call("llfe_edge_classes", xd.data_ptr(), out.data_ptr(), n, h, w, backend._stream(xd))
        assert np.array_equal(out.cpu().numpy(), cls), f"classes, bgr at +{off}"
        sums, cnts = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        backend._call("llfe_shadow_stats", xd.data_ptr(), sums.ctypes.data, cnts.ctypes.data, n, h, w,
                      backend._stream(xd))
        assert [(int(s), int(c)) for s, c in zip(sums, cnts)] == shadow, f"shadow stats, bgr at +{off}"
    xd, keep = _at_offset(torch, x, 0)
    out, keep2 = _at_offset(torch, np.zeros((n, h, w), np.uint8), 1)
    backend._call("llfe_edge_classes", xd.data_ptr(), out.data_ptr(), n, h, w, backend._stream(xd))
    assert np.array_equal(out.cpu().numpy(), cls), "classes at +1"
    assert not keep2[: out.storage_offset()].any() and not keep2[out.storage_offset() + out.numel():].any()
