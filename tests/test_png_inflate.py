"""The host half of the device PNG decode, CPU only: llfe_png_parse_batch and the kernels' host
twin llfe_png_decode_reference (csrc/png_inflate_core.h is the code the kernels compile) over
the hand-made files of tests/png_cases.py.  The oracle for the inflated rows is zlib.decompress
on the concatenated IDAT payloads, the oracle for the pixels decode.decode_batch.  Everything is
compared exactly."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import decode as D
from tests import png_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -5


def _host_pixels(case):
    """decode_batch's pixels for one case, or the text of its DecodeError."""
    try:
        return D.decode_batch([case["blob"]])[0]
    except D.DecodeError as e:
        return str(e)


@pytest.fixture(scope="module")
def staged():
    """(cases, StagedPng, twin raw, twin pixels, twin status) per size."""
    out = {}
    for (h, w), cases in P.by_size().items():
        sp = D.stage_png([c["blob"] for c in cases], workers=2, size=(h, w))
        # (a staging buffer is one of a ring of three: keep a copy past the next batches)
        sp = D.StagedPng(sp.blobs, h, w, sp.records.copy(), _descs(sp), sp.status)
        out[(h, w)] = (cases, sp) + D.png_reference(sp)
    return out


def test_case_list_covers_every_length_and_distance_code():
    got = {"len": set(), "dist": set(), "cl": set(), "types": set(), "maxlen": 0, "crossing": False}
    for c in P.CASES:
        if c["walk"]:
            r = P.walk(P.idat_payload(c["blob"])[2:-4])
            assert r["out"] == c["h"] * (c["w"] * 3 + 1), c["name"]
            for k in ("len", "dist", "cl"):
                got[k] |= r[k]
            got["types"] |= set(r["types"])
            got["maxlen"] = max(got["maxlen"], r["maxlen"])
            got["crossing"] |= r["crossing"]
    assert got["len"] == set(range(257, 286))
    assert got["dist"] == set(range(30))
    assert {16, 17, 18} <= got["cl"]
    assert got["maxlen"] == 15 and got["crossing"] and got["types"] == {0, 1, 2}


def test_parse_status_and_descriptors(staged):
    for (h, w), (cases, sp, _, _, _) in staged.items():
        for c, rc, d in zip(cases, sp.status, sp.descs):
            if c["kind"] == "parse":
                assert rc == UNSUPPORTED and d.deflate_bytes == 0 and d.raw_bytes == 0, c["name"]
                continue
            assert rc == 0, c["name"]
            payload = P.idat_payload(c["blob"])
            assert d.deflate_bytes == len(payload) - 6 and d.bpp in (3, 4) and d.row_bytes == w * d.bpp
            assert d.raw_bytes == h * (d.row_bytes + 1) and d.adler == int.from_bytes(payload[-4:], "big")
            assert d.record_offset % 16 == 0
            rec = sp.records.reshape(-1)[d.record_offset:]
            pad = (d.deflate_bytes + 15) & ~15
            assert rec[:d.deflate_bytes].tobytes() == payload[2:-4]
            assert not rec[d.deflate_bytes:pad + 16].any()
            assert int.from_bytes(rec[pad + 16:pad + 20].tobytes(), "little") == d.adler


def test_twin_inflates_what_zlib_inflates(staged):
    for (h, w), (cases, sp, raw, _, status) in staged.items():
        for i, c in enumerate(cases):
            if c["kind"] == "ok":
                want = zlib.decompress(P.idat_payload(c["blob"]))
                assert status[i] == 0, c["name"]  # (no eligible case is rescued by the fallback)
                assert raw[i, :len(want)].tobytes() == want, c["name"]
            else:
                assert status[i] == UNSUPPORTED, c["name"]


def test_twin_pixels_are_decode_batch_pixels(staged):
    for (h, w), (cases, sp, _, bgr, status) in staged.items():
        for i, c in enumerate(cases):
            if status[i] == 0:
                assert np.array_equal(bgr[i], _host_pixels(c)), c["name"]


def test_corrupt_container_stays_invalid():
    good = next(c for c in P.CASES if c["name"] == "good_10x12")["blob"]
    bad = bytearray(good)
    bad[40] ^= 1  # inside IDAT: the chunk's CRC no longer matches
    sp = D.stage_png([good, bytes(bad), b"", b"not an image"], workers=1, size=(10, 12))
    assert sp.status == [0, -1, UNSUPPORTED, UNSUPPORTED]


def _descs(sp):
    return (L.LlfePngDesc * len(sp.blobs)).from_buffer_copy(sp.descs)


@pytest.mark.parametrize("field,value", [("record_offset", -16), ("record_offset", 8), ("record_offset", 1 << 40),
                                         ("deflate_bytes", 1 << 30), ("deflate_bytes", -1), ("bpp", 2), ("bpp", 5),
                                         ("row_bytes", 35), ("raw_bytes", 369), ("raw_bytes", 1 << 33)])
def test_doctored_descriptors_are_refused(field, value):
    good = next(c for c in P.CASES if c["name"] == "good_10x12")["blob"]
    sp = D.stage_png([good, good], workers=1)
    raw = np.zeros((2, sp.raw_stride), np.uint8)
    out = np.zeros((2, 10, 12, 3), np.uint8)
    status = (C.c_int32 * 2)()

    def call(descs, h=10, w=12, stride=None):
        return L.lib().llfe_png_decode_reference(sp.records.ctypes.data, sp.records.size, descs, 2, h, w, raw.ctypes.data,
                                                 stride or raw.shape[1], out.ctypes.data, status)

    assert call(_descs(sp)) == 0 and list(status) == [0, 0]
    assert call(_descs(sp), h=11) == L.LLFE_ERR_INVALID and call(_descs(sp), w=13) == L.LLFE_ERR_INVALID
    assert call(_descs(sp), stride=368) == L.LLFE_ERR_INVALID
    d = _descs(sp)
    setattr(d[1], field, value)
    out[:] = 0
    assert call(d) == L.LLFE_ERR_INVALID and not out.any()


def test_last_record_must_fit_the_staging_buffer():
    good = next(c for c in P.CASES if c["name"] == "good_10x12")["blob"]
    sp = D.stage_png([good], workers=1)
    d = _descs(sp)
    need = ((d[0].deflate_bytes + 15) & ~15) + 16
    raw, out, status = np.zeros((1, sp.raw_stride), np.uint8), np.zeros((1, 10, 12, 3), np.uint8), (C.c_int32 * 1)()
    f = L.lib().llfe_png_decode_reference
    assert f(sp.records.ctypes.data, need, d, 1, 10, 12, raw.ctypes.data, raw.shape[1], out.ctypes.data, status) == 0
    assert f(sp.records.ctypes.data, need - 1, d, 1, 10, 12, raw.ctypes.data, raw.shape[1], out.ctypes.data, status) == -1


def test_abi_symbols_and_struct():
    lib = L.lib()
    for name in ("llfe_png_parse_batch", "llfe_png_decode_reference", "llfe_png_decode_device"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert C.sizeof(L.LlfePngDesc) == 32
    assert [(f, getattr(L.LlfePngDesc, f).offset) for f, _ in L.LlfePngDesc._fields_] == [
        ("record_offset", 0), ("raw_bytes", 8), ("deflate_bytes", 16), ("bpp", 20), ("row_bytes", 24), ("adler", 28)]
    assert lib.llfe_png_decode_device(None, None, 0, None, 0, 1, 1, None, 16, None, None, None) == L.LLFE_ERR_INVALID


def test_struct_layout_matches_header_via_compiler(tmp_path):
    fields = [f for f, _ in L.LlfePngDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "llfe.h"', "int main(void){",
             'printf("sizeof %zu\\n", sizeof(llfe_png_desc));']
    lines += [f'printf("{f} %zu\\n", offsetof(llfe_png_desc, {f}));' for f in fields]
    lines.append("return 0;}")
    src = tmp_path / "lay.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(L.LlfePngDesc)
    for f in fields:
        assert int(got[f]) == getattr(L.LlfePngDesc, f).offset, f


def test_png_argument_is_checked():
    with pytest.raises(ValueError):
        D.decode_batch_device([b""], png="gpu")
