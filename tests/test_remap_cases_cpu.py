"""The cases of tests/remap_model.py, without a device: the table is what tests/test_gpu_remap.py needs it to be; every case keeps the margins that
make the comparison with the device exact at every pixel AND at every validity byte; every case's invalid share says that it tests something;
and the model's resampling is the lens model's where the two overlap."""
import numpy as np
import pytest

import lens_model as lm
import remap_model as rm
from line3d_amd import capi

assert (rm.BROWN, rm.FISHEYE) == (capi.LENS_BROWN, capi.LENS_FISHEYE)

MARGIN = 1e-7      # the margins of tests/test_lens_cases_cpu.py: tie_margin in units of 1/32 pixel, limit_distance in pixels


@pytest.fixture(scope="module")
def models():
    return [(c, rm.case_model(c)) for c in rm.CASES]


def test_table_covers_what_the_device_test_needs():
    cs = rm.CASES
    assert len(cs) == len(lm.SIZES) * len(rm.LENSES)
    assert {c["size"][:2] for c in cs} == {(8, 8), (37, 29), (96, 80), (161, 41), (257, 8)} and {c["size"][2] for c in cs} == {1, 3}
    assert any(c["size"][3] for c in cs)                                                             # padded rows
    for name, _, _ in rm.LENSES:
        mine = [c for c in cs if "_%s_" % name in c["name"]]
        assert len(mine) == len(lm.SIZES)
        assert {c["kind"] for c in mine} == set(rm.OUT_KINDS), name                                   # every lens at every kind of output size
        if name != "pinhole":
            assert {c["alpha"] for c in mine} == set(rm.ALPHAS), name                                 # ... and at every alpha
    assert {(c["kind"], c["alpha"]) for c in cs if c["alpha"] is not None} == {(k, a) for k in rm.OUT_KINDS for a in rm.ALPHAS}
    sizes = [(c["size"][:2], c["out_size"]) for c in cs]
    assert any(o == s for s, o in sizes) and any(o[0] < s[0] and o[1] < s[1] for s, o in sizes)
    assert any(o[0] > s[0] and o[1] == s[1] for s, o in sizes) and any(o == (37, 29) and s != o for s, o in sizes)
    assert any(o[0] > s[0] and o[1] > s[1] for s, o in sizes)                                        # (8 x 8 onto 37 x 29: larger on both)
    assert sum(c["masked"] for c in cs) >= 8 and all(not c["masked"] for c in cs if c["alpha"] == 0.0)
    for c in cs:
        if c["model"] == 0:                                                                           # the pinhole: a differing camera
            assert tuple(c["out_cam"]) != tuple(c["src_cam"]) and rm.is_pinhole(c["model"], c["coeffs"])
        else:                                                                                         # the others: the planner's camera for the size
            K, wh = rm.plan(c["model"], c["src_cam"], c["coeffs"], c["size"][:2], c["alpha"], c["out_size"])
            assert wh == c["out_size"] and (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) == tuple(c["out_cam"])


def test_the_mask_has_holes_at_the_edge_and_in_the_middle():
    for w, h in {c["size"][:2] for c in rm.CASES if c["masked"]}:
        m = rm.case_mask(w, h)
        assert m[0, 0] == 0 and m[h - 1, w - 1] == 0 and m[h // 2, w // 2 - 1] == 0                   # corner, last row, middle
        assert m[h // 2 - 2, w // 2 - 1] == 1 and m[h // 2 + 2, w // 2 - 1] == 1 and 0.5 < m.mean() < 1.0


def test_margins(models):
    """A CONDITION on the cases (see tests/test_lens_cases_cpu.py::test_fisheye_margins for the reasoning): with every pixel of a FISHEYE case at
    least 1e-7 (in 32 u) from a rounding tie and 1e-7 pixels from the limits of the inside test, a device atan that differs by a few ulp flips
    neither a rounding nor an inside decision.  A validity byte depends on the inside test, on WHICH taps carry weight and on where they lie:
    a weight is zero iff rint(32 u) is a multiple of 32, which changes only where 32 u crosses a rounding tie -- held explicitly below as the
    distance of 32 u from the two ties next to every multiple of 32 -- and the taps' positions are floor(rint(32 u) / 32), the same ties."""
    n = 0
    for c, m in models:
        if c["model"] != rm.FISHEYE:
            continue
        assert np.isfinite(m["u"]).all() and np.isfinite(m["v"]).all()
        assert m["tie_margin"].min() >= MARGIN, (c["name"], m["tie_margin"].min())
        assert m["limit_distance"].min() >= MARGIN, (c["name"], m["limit_distance"].min())
        for q in (32.0 * m["u"], 32.0 * m["v"]):
            near = np.rint(q / 32.0) * 32.0                               # the multiple of 32 nearest to 32 u: the weight is zero within 1/2 of it
            assert np.abs(np.abs(q - near) - 0.5).min() >= MARGIN, c["name"]
        n += 1
    assert n == 2 * len(lm.SIZES)


def test_every_case_tests_something(models):
    for c, m in models:
        share = float((m["valid"] == 0).mean())
        assert m["resampled"] and m["image"].shape[:2] == c["out_size"][::-1] == m["valid"].shape
        assert set(np.unique(m["valid"])) <= {0, 255}
        if c["alpha"] == 0.0:
            assert share == 0.0, (c["name"], share)
        else:
            assert 0.05 <= share <= 0.60, (c["name"], share)
        assert not m["image"][~m["inside"]].any()                                                     # an outside pixel is written 0
        if c["masked"]:                                                                               # the mask takes pixels the border rule leaves
            _, img, mask = rm.case_image(c)
            plain = rm.remap(img, c["out_size"], c["out_cam"], c["model"], c["src_cam"], c["coeffs"])
            only = rm.remap(img, c["out_size"], c["out_cam"], c["model"], c["src_cam"], c["coeffs"], mask=mask, border_mask=False)
            assert np.array_equal(plain["image"], m["image"]) and np.array_equal(only["image"], m["image"])
            assert ((plain["valid"] == 255) & (m["valid"] == 0)).sum() >= 3, c["name"]
            assert np.array_equal(m["valid"], np.minimum(plain["valid"], only["valid"]))
    partial = sum(1 for c, m in models if ((m["valid"] == 0) & m["inside"]).any() and not c["masked"])
    assert partial >= 5                                             # inside pixels made invalid by a tap off the source


def test_resampling_is_the_lens_models_at_equal_sizes():
    """at the source size and without a mask the pixels are tests/lens_model.py's, and the validity plane is its inside and partial masks"""
    for c in lm.CASES:
        _, img = lm.case_image(c)
        want = lm.case_model(c)
        got = rm.remap(img, None, c["out_cam"], c["model"], c["src_cam"], c["coeffs"])
        assert np.array_equal(got["image"], want["image"]), c["name"]
        if got["resampled"]:
            assert np.array_equal(got["valid"] == 255, want["inside"] & ~want["partial"]), c["name"]
        else:
            assert c["claim"] == "identity" and got["valid"].min() == 255


def test_pass_through():
    img = np.arange(8 * 9, dtype=np.uint8).reshape(8, 9)
    mask = rm.case_mask(9, 8)
    cam = (7.0, 7.0, 4.0, 3.5)
    for model, co in ((None, ()), (0, ()), (rm.BROWN, (0.0,) * 8)):
        m = rm.remap(img, None, cam, model, cam if model is not None else None, co, mask=mask)
        assert not m["resampled"] and np.array_equal(m["image"], img) and np.array_equal(m["valid"], np.where(mask, 255, 0))
    assert rm.remap(img, (10, 8), cam, 0, cam, ())["resampled"]           # a pinhole camera, another size: resampled (a crop or a frame)
