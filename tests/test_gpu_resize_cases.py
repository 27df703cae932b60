"""The preprocessing kernels on the directed cases of tests/resize_cases.py, bit-exact:
cvresize.hip against the oracle's cv_resize, resize.hip against Pillow itself (LANCZOS with and
without a box, reduce, thumbnail and its batch form) and text.hip against the oracle's
text_binary.  tests/test_resize_case_inputs.py proves on the CPU which branch each case reaches
and checks the expected values themselves (oracle against Pillow and against NumPy)."""
import numpy as np
import pytest

from tests import resize_cases as RC

pytestmark = pytest.mark.gpu


def _same(got, exp, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    exp = np.asarray(exp)
    assert got.shape == exp.shape, f"{what}: shape {got.shape}, expected {exp.shape}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        where = [(tuple(int(v) for v in p), int(got[tuple(p)]), int(exp[tuple(p)])) for p in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {exp.size} bytes differ; (index, got, expected): {where}")


@pytest.mark.parametrize("case", RC.CV_CASES, ids=lambda c: c.id)
def test_cv_resize_cases(backend, case):
    exp = RC.cv_expected(case)
    for kind, x, e in zip(RC.IMAGE_KINDS, RC.cv_images(case), exp):
        _same(backend.resize_cv(np.array(x), case.ow, case.oh, case.interp), e, f"{case.id} {kind}")


@pytest.mark.parametrize("case", RC.LANCZOS_CASES, ids=lambda c: c.id)
def test_lanczos_cases(backend, case):
    exp = RC.lanczos_expected(case)
    for kind, x, e in zip(RC.IMAGE_KINDS, RC.images(case.h, case.w, case.ch), exp):
        _same(backend.resize_lanczos_pil(np.array(x), case.ow, case.oh, box=case.box), e, f"{case.id} {kind}")


@pytest.mark.parametrize("case", RC.REDUCE_CASES, ids=lambda c: c.id)
def test_reduce_cases(backend, case):
    exp = RC.reduce_expected(case)
    for kind, x, e in zip(RC.IMAGE_KINDS, RC.images(case.h, case.w, case.ch), exp):
        _same(backend.reduce_pil(np.array(x), case.fx, case.fy), e, f"{case.id} {kind}")


@pytest.mark.parametrize("case", RC.THUMB_CASES, ids=lambda c: c.id)
def test_thumbnail_cases(backend, case):
    x = np.array(RC.thumb_image(case.h, case.w, case.ch, case.seed))
    _same(backend.thumbnail_pil(x, case.max_w, case.max_h), RC.thumb_expected(case), case.id)


def test_thumbnail_batch_case(backend):
    h, w, max_w, max_h, seeds = RC.BATCH_CASE
    x = np.stack([RC.thumb_image(h, w, 3, s) for s in seeds])
    got = backend.thumbnail_pil_batch(x, max_w, max_h).cpu().numpy()
    assert len(got) == len(seeds)
    for i, s in enumerate(seeds):
        _same(got[i], RC.thumb_expected(RC.ThumbCase(h, w, 3, max_w, max_h, s, True)), f"batch image {i}")


@pytest.mark.parametrize("name", RC.TEXT_NAMES)
def test_text_binary_cases(backend, name):
    exp, t = RC.text_expected(name)
    got, gt = backend.text_binary(np.array(RC.text_cases()[name]))
    assert gt == t, f"{name}: threshold {gt}, expected {t}"
    _same(got, exp, name)
