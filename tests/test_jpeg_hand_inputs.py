"""The hand-made baseline JPEG files of tests/jpeg_hand_cases.py against the host half of the
device entropy decode, CPU only: the parser (llfe_jpeg_parse_batch_flags) takes or refuses every
file as its kind says and writes nothing for a refused one; the kernels' host twin
(llfe_jpeg_entropy_reference, the csrc/jpeg_huff_core.h the kernels compile) reproduces the
coefficient slots of decode.stage_coefs (libjpeg-turbo's jpeg_read_coefficients) for every "ok"
file, in lanes and in one piece, per size and in one ragged batch, and hands every "handed_back"
file back; the NumPy restatement of the reconstruction equals the library's pixels for the files
whose tables and coefficients no encoder produces; the host decoder agrees with Pillow; and the
walker shows that the list holds the symbols, code lengths and block lengths it is there for.
tests/test_gpu_jpeg_hand.py runs the same list through the kernels."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode
from tests import jpeg_hand_cases as J
from tests import jpeg_huff_cases as H
from tests import jpeg_restart_cases as RC
from tests import jpeg_restate as R

SIZES = sorted(J.by_size())
OK = [c["name"] for c in J.CASES if c["kind"] == "ok"]
# the rows of the case list and their kinds, so that a row cannot leave or change unnoticed
ROWS = {
    "ok": """skew16 extremes only_63 eob_alias zrl_then_eob zrl_lands_on_64 densest long_blocks long_blocks_3wg dc_wrap
             dc_wrap_colour grey_hv22 grey_hv22_odd sel_swapped_420 sel_shared_444 dht_layouts_one_segment dht_layouts_redefined
             dht_layouts_before_sof ids_012 adobe_t1 dqt16_ones dqt16_300 dqt16_1000 dqt16_40000 dqt16_65535 dqt16_mixed
             q255_big q1_big colour_extremes_420 colour_extremes_422 rst_ri1_skew rst_after_stuffed
             rst_ri_larger_than_scan rst_dc_wrap rst_dc_wrap_ri20 rst_long_blocks""",
    "handed_back": "zrl_x4 run_overflow no_such_code dc_cat12 ac_size11 zero_padding extra_byte rst_wrong_index rst_missing",
    "parse": "fill_ff all_ones_code ids_rgb adobe_t0 s440 s411 all_2x2",
}


def _parse(cases, h, w, restarts, fill=0xA5):
    """llfe_jpeg_parse_batch_flags into pre-filled records, so a write shows."""
    blobs = [c["blob"] for c in cases]
    n = len(blobs)
    stride = _lib.JPEG_RECORD_HEADER + ((max(len(b) for b in blobs) + 15) & ~15) + 16
    rec = np.full((n, stride), fill, np.uint8)
    descs, scans = (_lib.LlfeJpegDesc * n)(), (_lib.LlfeJpegScan * n)()
    keep = [C.c_char_p(b) for b in blobs]
    ptrs = (C.c_void_p * n)(*[C.cast(k, C.c_void_p) for k in keep])
    sizes = (C.c_uint64 * n)(*[len(b) for b in blobs])
    status = (C.c_int32 * n)()
    _lib.lib().llfe_jpeg_parse_batch_flags(ptrs, sizes, n, h, w, rec.ctypes.data, stride, decode.coef_slot_bytes(h, w), descs,
                                           scans, status, 2, _lib.JPEG_PARSE_RESTARTS if restarts else 0)
    return list(status), rec, descs, scans


def test_every_row_is_present_with_its_kind():
    listed = {k: sorted(c["name"] for c in J.CASES if c["kind"] == k) for k in ROWS}
    assert listed == {k: sorted(v.split()) for k, v in ROWS.items()}
    for c in J.CASES:
        assert c["restarts"] == c["name"].startswith("rst_") and decode._image_size(c["blob"]) == (c["h"], c["w"])
        assert c["blob"][:2] == b"\xff\xd8" and c["blob"][-2:] == b"\xff\xd9"


@pytest.mark.parametrize("h,w,restarts", SIZES)
def test_parser_and_twin_per_size(h, w, restarts):
    cases = J.by_size()[h, w, restarts]
    blobs = [c["blob"] for c in cases]
    status, rec, descs, scans = _parse(cases, h, w, restarts)
    for i, c in enumerate(cases):
        if c["kind"] == "parse":  # refused, and nothing written
            assert status[i] == H.UNSUPPORTED, c["name"]
            assert (rec[i] == 0xA5).all() and descs[i].n_comp == 0 and scans[i].blocks_in_mcu == 0, c["name"]
        else:
            assert status[i] == 0, c["name"]
            assert scans[i].restart_interval == (J.walk_dri(c["blob"]) if restarts else 0)
    sb = decode.stage_bytes(blobs, workers=2, restarts=restarts, size=(h, w))
    assert sb.status == status
    if not any(rc == 0 for rc in status):
        return
    st = decode.stage_coefs(blobs, workers=2, size=(h, w))
    for one_piece in (False, True):
        slots, twin = decode.entropy_reference(sb, one_piece)
        for i, c in enumerate(cases):
            if c["kind"] == "ok":
                assert twin[i] == 0 and st.status[i] == 0, c["name"]
                assert bytes(sb.descs[i]) == bytes(st.descs[i]), c["name"]
                assert H.slots_equal(slots[i], st.slots[i], st.descs[i]), c["name"]
            else:
                assert twin[i] != 0, c["name"]


@pytest.mark.parametrize("one_piece", [False, True])
def test_twin_on_one_shuffled_ragged_batch(one_piece):
    order = np.random.default_rng(11).permutation(len(J.CASES))
    cases = [J.CASES[k] for k in order]
    blobs = [c["blob"] for c in cases]
    sb = decode.stage_bytes_images(blobs, workers=2, restarts=True)
    st = decode.stage_coefs_images(blobs, workers=2)
    slots, twin = decode.entropy_reference_images(sb, one_piece)
    for i, c in enumerate(cases):
        assert (sb.status[i] == 0) == (c["kind"] != "parse"), c["name"]
        assert (twin[i] == 0) == (c["kind"] == "ok"), c["name"]
        if c["kind"] == "ok":
            m, want = sb.images[i], st.images[i]
            assert st.status[i] == 0 and bytes(sb.descs[i]) == bytes(st.descs[i]), c["name"]
            assert (m.slot_offset, m.slot_bytes) == (want.slot_offset, want.slot_bytes), c["name"]
            a, b = m.slot_offset, m.slot_offset + m.slot_bytes
            assert H.slots_equal(slots[a:b], st.slots[a:b], st.descs[i]), c["name"]


def test_without_the_flag_the_restart_files_are_refused():
    for (h, w, restarts), cases in J.by_size().items():
        if restarts:
            status, rec, descs, scans = _parse(cases, h, w, False)
            dri = [J.walk_dri(c["blob"]) for c in cases]
            assert all(dri) and status == [H.UNSUPPORTED] * len(cases) and (rec == 0xA5).all()


@pytest.mark.parametrize("name", [n for n in OK if n in J.RECON or J.BY_NAME[n]["blob"].count(b"\xff\xc0\x00\x11")])
def test_restatement_equals_the_library_pixels(name):
    """The colour and quantisation cases: 16-bit table entries whose products wrap, samples far
    outside 0..255, saturated chroma through the upsampling and the colour clamp."""
    blob = J.BY_NAME[name]["blob"]
    st = decode.stage_coefs([blob], workers=1)
    assert st.status == [0]
    stats = {}
    assert np.array_equal(R.restate(st, 0, stats), decode.decode_bgr(blob))
    if name.startswith(("q255", "q1_", "dqt16_300", "dqt16_1000", "dqt16_mixed", "colour_extremes")):
        assert stats["idct_out_of_range"] > 0
    if name.startswith("colour_extremes"):
        assert stats["colour_out_of_range"] > 0


def test_quantisation_tables_reach_the_slots():
    for name, want in (("dqt16_ones", 1), ("dqt16_300", 300), ("dqt16_40000", 40000), ("dqt16_65535", 65535), ("q255_big", 255)):
        sb = decode.stage_bytes([J.BY_NAME[name]["blob"]], workers=1)
        slots, status = decode.entropy_reference(sb)
        assert status == [0] and (slots[0, :128].view(np.uint16) == want).all()
    sb = decode.stage_bytes([J.BY_NAME["dqt16_mixed"]["blob"]], workers=1)
    mixed = decode.entropy_reference(sb)[0][0, :128].view(np.uint16)
    assert sorted(mixed.tolist()) == sorted(J.mixed_table(1)) and mixed.max() > 32767


@pytest.mark.parametrize("case", J.CASES, ids=lambda c: c["name"])
def test_host_decoder_agrees_with_pillow(case):
    try:
        im = Image.open(io.BytesIO(case["blob"]))
        im.load()
    except Exception:
        with pytest.raises(decode.DecodeError):  # what the library refuses nobody decodes
            decode.decode_bgr(case["blob"])
        assert case["name"] in ("all_ones_code", "all_2x2")
        return
    want = np.asarray(im.convert("RGB"))[:, :, ::-1]
    assert np.array_equal(decode.decode_bgr(case["blob"]), want)


# ---------------------------------------------------------------- what the walker shows
def _walked(name):
    return J.walk(J.BY_NAME[name]["blob"])


def test_walker_symbols_and_code_lengths():
    a, b = _walked("skew16"), _walked("extremes")
    assert a["ac"] | b["ac"] == set(J.AC_SYMS) and len(J.AC_SYMS) == 162
    assert a["dc"] == set(range(12)) and b["dc"] == {10, 11}
    assert a["lengths"] == set(range(1, 9)) | {16} and 16 in b["lengths"]
    assert a["blocks"] == 12 and b["blocks"] == 25
    # each without the other misses symbols: both carry the claim
    assert a["ac"] != set(J.AC_SYMS) and not set(J.AC_SYMS) - {0x00, 0xF0} - b["ac"]
    assert 0x50 in _walked("eob_alias")["ac"] and 0x00 not in _walked("eob_alias")["ac"]
    assert _walked("only_63")["ac"] == {0xF0, 0xE2, 0xEA, 0x00}
    assert _walked("zrl_then_eob")["ac"] == {0xF0, 0x00, 0x01}
    for name in ("sel_swapped_420", "sel_shared_444", "ids_012", "adobe_t1", "grey_hv22_odd", "colour_extremes_420"):
        assert 16 in _walked(name)["lengths"]


def test_walker_block_lengths_and_subsequences():
    d = _walked("densest")
    assert d["blocks"] == 4096 and d["longest"] == d["shortest"] == 0.25 and d["lengths"] == {1}
    assert d["scan_bytes"] == 1024 and H.SUB // 0.25 == 512  # 512 blocks to a subsequence, eight subsequences
    for name in ("long_blocks", "rst_long_blocks"):
        r = _walked(name)
        assert r["blocks"] == 64 and r["shortest"] > H.SUB  # no block fits a subsequence
        assert 100 <= -(-r["scan_bytes"] // H.SUB) <= 120
    assert _walked("rst_long_blocks")["markers"] == [k & 7 for k in range(63)]
    c = J.BY_NAME["long_blocks_3wg"]
    r = J.walk(c["blob"])
    lanes = -(-len(H.scan_bytes(c["blob"])) // H.SUB)
    assert r["scan_bytes"] == len(H.scan_bytes(c["blob"])) and 2 * 256 < lanes <= 3 * 256 and r["shortest"] > H.SUB
    # the smallest such size: a block row less stays within two workgroups of lanes
    fewer = J.jpeg(c["h"] - 8, c["w"], blocks=J.long_block_list(16 * (c["h"] // 8 - 1)))
    assert c["w"] == 128 and -(-J.walk_scan_bytes(fewer) // H.SUB) <= 2 * 256
    assert len(c["blob"]) < 80000


def test_walker_restart_markers_and_dc_sums():
    assert _walked("rst_ri1_skew")["markers"] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3]
    assert _walked("rst_ri_larger_than_scan")["markers"] == []
    assert J.walk_dri(J.BY_NAME["rst_ri_larger_than_scan"]["blob"]) == 1000
    assert _walked("rst_dc_wrap")["markers"] == [k & 7 for k in range(12)]
    assert _walked("rst_dc_wrap_ri20")["markers"] == [0, 1, 2]
    scan = bytes(RC.scan_bytes(J.BY_NAME["rst_after_stuffed"]["blob"]))
    assert any(scan[k:k + 3] == b"\xff\x00\xff" and 0xD0 <= scan[k + 3] <= 0xD7 for k in range(len(scan) - 3))
    # the DC sums leave 16 bits and the library stores them truncated
    for name, ri in (("dc_wrap", 64), ("rst_dc_wrap", 5), ("rst_dc_wrap_ri20", 20)):
        st = decode.stage_coefs([J.BY_NAME[name]["blob"]], workers=1)
        d = st.descs[0]
        dc = st.slots[0][d.comp[0].coef_offset:d.comp[0].coef_offset + 64 * 128].view(np.int16)[::64]
        true = np.array([2047 * (k % ri + 1) for k in range(64)])
        assert np.array_equal(dc, true.astype(np.int16)) and (np.abs(true).max() > 32767) == (ri > 5)
    st = decode.stage_coefs([J.BY_NAME["dc_wrap_colour"]["blob"]], workers=1)
    sb = decode.stage_bytes([J.BY_NAME["dc_wrap_colour"]["blob"]], workers=1)
    assert 256 < sb.scans[0].mcus_w * sb.scans[0].mcus_h < 512
    for c in range(3):
        k = st.descs[0].comp[c]
        dc = st.slots[0][k.coef_offset:k.coef_offset + k.blocks_w * k.blocks_h * 128].view(np.int16)[::64]
        assert len(np.unique(dc)) > 256 and dc.min() < -30000 and dc.max() > 30000
