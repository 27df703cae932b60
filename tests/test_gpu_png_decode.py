"""PNG decode on the device (csrc/png_inflate.hip behind decode.decode_batch_device(png="device")):
over the hand-made files of tests/png_cases.py the batch equals decode.decode_batch, the device's
status equals the host twin's image by image (zero for every eligible well-formed file, non-zero
for every anomaly), and the inflated rows equal the twin's; anomalous files behave through the
public door exactly as they do in decode_batch; mixed batches of PNG and JPEG land in one tensor;
png="host" stays the path it was.  tests/test_png_inflate.py checks the same inputs against the
twin on the CPU, tests/test_png_inflate_sanitized.py under the sanitizers."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from tests import png_cases as P

pytestmark = pytest.mark.gpu
SIZES = list(P.by_size())


def _host(blobs):
    """decode_batch's result: the batch, or the text of its DecodeError."""
    try:
        return decode.decode_batch(blobs, workers=2)
    except decode.DecodeError as e:
        return str(e)


def _device(blobs, **kw):
    try:
        return decode.decode_batch_device(blobs, workers=2, png="device", **kw).cpu().numpy()
    except decode.DecodeError as e:
        return str(e)


def _same(blobs, **kw):
    want, got = _host(blobs), _device(blobs, **kw)
    if isinstance(want, str):
        assert got == want
    else:
        assert not isinstance(got, str), got
        for i in range(len(blobs)):
            assert np.array_equal(got[i], want[i]), f"image {i} differs at {np.argwhere(got[i] != want[i])[:4].tolist()}"
    return got


@pytest.mark.parametrize("h,w", SIZES)
def test_case_list_equals_twin_and_host(backend, h, w):
    """One batch per size: status and inflated rows against the twin, pixels against the twin for
    what the device took, then the public door against decode_batch file by file (a file whose
    error decode_batch raises would hide the others of its batch) and as one batch."""
    cases = P.by_size()[(h, w)]
    blobs = [c["blob"] for c in cases]
    sp = decode.stage_png(blobs, workers=2, size=(h, w))
    t_raw, t_bgr, t_status = decode.png_reference(sp)
    raw = torch.zeros((len(blobs), sp.raw_stride), dtype=torch.uint8, device="cuda")
    out, status = decode.png_decode_staged(sp, raw=raw)
    assert status == t_status
    for c, rc in zip(cases, status):
        assert (rc == 0) == (c["kind"] == "ok"), c["name"]
    assert np.array_equal(raw.cpu().numpy(), t_raw)
    got = out.cpu().numpy()
    for i, rc in enumerate(status):
        if rc == 0:
            assert np.array_equal(got[i], t_bgr[i]), cases[i]["name"]
    for c in cases:
        if c["kind"] != "ok":
            _same([c["blob"]])
    _same(blobs)


def test_mixed_batch_in_one_tensor(backend):
    """PNG RGB, RGBA and palette, an anomalous PNG, a baseline JPEG (entropy decode on the device)
    and a progressive one: every image by its own path, the places kept."""
    h, w = 10, 12
    name = {c["name"]: c["blob"] for c in P.CASES}
    rgb = P.smooth(h, w, seed=70)
    rgba = P.smooth(h, w, 4, seed=71)
    jpgs = []
    for kw in ({}, {"progressive": True}):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, "JPEG", quality=85, **kw)
        jpgs.append(buf.getvalue())
    blobs = [jpgs[0], P.png(h, w, 2, P.deflate(P.filter_rows(rgb, [4, 1]))), name["palette"], jpgs[1],
             P.png(h, w, 6, P.deflate(P.filter_rows(rgba, [3]))), name["filter_byte_5"], name["good_10x12"]]
    want = _host(blobs)
    for entropy in ("host", "device"):
        got = _device(blobs, entropy=entropy)
        assert type(got) is type(want)
        assert np.array_equal(got, want) if not isinstance(want, str) else got == want
    # without the file the host refuses, the batch decodes: equal bytes by both JPEG paths
    blobs = [b for b in blobs if b is not name["filter_byte_5"]] + [name["wrong_adler"]]
    for entropy in ("host", "device"):
        _same(blobs, entropy=entropy)


def test_errors_name_the_image_of_the_whole_batch(backend):
    name = {c["name"]: c["blob"] for c in P.CASES}
    buf = io.BytesIO()
    Image.fromarray(P.smooth(10, 12, seed=72)).save(buf, "JPEG")
    blobs = [buf.getvalue(), name["good_10x12"], buf.getvalue(), name["other_size"], name["good_10x12"]]
    want = _host(blobs)
    assert isinstance(want, str) and want.startswith("image 3:")
    assert _device(blobs) == want and _device(blobs, entropy="device") == want


def test_png_host_stays_the_host_path(backend, monkeypatch):
    blobs = [c["blob"] for c in P.by_size()[(48, 64)]]

    def never(*a, **k):
        raise AssertionError("the PNG device path ran")

    monkeypatch.setattr(decode, "stage_png", never)
    want = decode.decode_batch(blobs, workers=2)
    assert np.array_equal(decode.decode_batch_device(blobs, workers=2).cpu().numpy(), want)
    assert np.array_equal(decode.decode_batch_device(blobs, workers=2, png="host").cpu().numpy(), want)
    with pytest.raises(ValueError):
        decode.decode_batch_device(blobs, png="both")


def test_out_is_honoured_and_checked(backend):
    blobs = [c["blob"] for c in P.by_size()[(48, 64)]]
    want = decode.decode_batch(blobs, workers=2)
    out = torch.zeros((len(blobs), 48, 64, 3), dtype=torch.uint8, device="cuda")
    got = decode.decode_batch_device(blobs, workers=2, png="device", out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    for bad in (torch.zeros((len(blobs), 48, 64, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((len(blobs), 48, 64, 3), dtype=torch.int8, device="cuda"),
                torch.zeros((len(blobs), 48, 64, 3), dtype=torch.uint8),
                torch.zeros((len(blobs), 48, 128, 3), dtype=torch.uint8, device="cuda")[:, :, ::2]):
        with pytest.raises(ValueError):
            decode.decode_batch_device(blobs, workers=2, png="device", out=bad)


def test_doctored_descriptor_is_refused_before_any_launch(backend):
    blobs = [c["blob"] for c in P.by_size()[(10, 12)] if c["kind"] == "ok"]
    sp = decode.stage_png(blobs, workers=1)
    descs = (_lib.LlfePngDesc * len(blobs)).from_buffer_copy(sp.descs)
    descs[0].record_offset = sp.records.size  # past the staging buffer
    rec = torch.from_numpy(sp.records).cuda()
    out = torch.zeros((len(blobs), 10, 12, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.LlfeError):
        backend.png_decode(rec, descs, 10, 12, out)
    assert not out.any()
    assert backend.png_decode(rec, sp.descs, 10, 12, out) == [0] * len(blobs)


def test_pillow_encoded_synth_batch(backend):
    """Real encoder output with more than one block: 64 synth images of 200 x 300 as Pillow
    writes them, RGB and RGBA alternating; none falls back."""
    blobs = []
    for i in range(64):
        im = Image.fromarray(np.ascontiguousarray(synth.synth_numpy(i, 200, 300)[:, :, ::-1]))
        buf = io.BytesIO()
        (im.convert("RGBA") if i % 2 else im).save(buf, "PNG")
        blobs.append(buf.getvalue())
    sp = decode.stage_png(blobs, workers=2)
    assert decode.png_decode_staged(sp)[1] == [0] * 64
    _same(blobs)
