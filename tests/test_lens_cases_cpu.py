"""The cases of tests/lens_model.py, without a device: every case is what its name claims; every FISHEYE case keeps the margins that make the
comparison with the device exact at every pixel; and the model's formulas are checked against a forward projection written separately from them,
per COLMAP's definitions of its camera models, inverted numerically."""
import os

import numpy as np
import pytest

import lens_model as lm
from line3d_amd import capi, sfm

assert (lm.BROWN, lm.FISHEYE) == (capi.LENS_BROWN, capi.LENS_FISHEYE)      # the model's numbers are the library's

MARGIN = 1e-7      # tie_margin in units of 1/32 pixel, limit_distance in pixels (see test_fisheye_margins)


@pytest.fixture(scope="module")
def models():
    return [(c, lm.case_model(c)) for c in lm.CASES]


def test_table_is_the_cross_product():
    assert len(lm.CASES) == len(lm.SIZES) * len(lm.LENSES) * 2 + 1
    assert {c["size"][:2] for c in lm.CASES} == {(8, 8), (37, 29), (96, 80), (161, 41), (257, 8)}
    assert {c["size"][2] for c in lm.CASES} == {1, 3} and any(c["size"][3] for c in lm.CASES)
    assert any(c["other"] and abs(c["out_cam"][0] - 0.6 * c["src_cam"][0]) < 1e-12 for c in lm.CASES)


def test_cases_are_what_they_claim(models):
    seen = set()
    for c, m in models:
        w, h = c["size"][:2]
        k = list(c["coeffs"]) + [0.0] * (8 - len(c["coeffs"]))
        _, img = lm.case_image(c)
        lens = c["name"].split("_", 1)[1]
        if c["other"]:
            assert c["src_cam"] is not None and tuple(c["src_cam"]) != tuple(c["out_cam"]), c["name"]
        if c["claim"] == "identity":
            assert not any(k) and c["src_cam"] is None and np.array_equal(m["image"], img)
            continue
        assert not np.array_equal(m["image"], img), c["name"]
        if lens.startswith("tangential"):
            assert k[2] and k[3] and not any(k[:2] + k[4:])
        if lens.startswith("k3"):
            assert k[4] and not any(k[:4] + k[5:])
        if c["model"] == lm.FISHEYE:
            assert not any(k[4:]) and (all(k[:4]) if "fisheye4" in lens else not any(k[:4]))
        if lens.startswith("all_eight"):
            assert all(k)
        if c["claim"] == "den_not_one":
            den = lm.denominator(w, h, c["out_cam"], k)
            assert np.abs(den - 1.0).max() > 0.02 and den.min() > 0.0, c["name"]
        if c["claim"] == "den_changes_sign":
            den = lm.denominator(w, h, c["out_cam"], k)
            assert den.min() < 0.0 < den.max() and (den == 0.0).any(), c["name"]
            bad = ~np.isfinite(m["u"]) | ~np.isfinite(m["v"])
            assert np.isinf(m["u"]).any() and np.isnan(m["v"]).any(), c["name"]
            assert not m["image"][bad].any() and not m["inside"][bad].any()        # inf and NaN come out 0
            seen.add("nonfinite")
        if (~m["inside"]).any():
            seen.add("outside")
        if m["partial"].any():
            seen.add("partial")
    assert seen == {"nonfinite", "outside", "partial"}


def test_fisheye_margins(models):
    """A CONDITION on the cases, not a measurement: atan is the one operation whose bits the device does not share with numpy.  A device atan within a
    few ulp moves theta by about 1e-16 relative, u and v by under 1e-13 pixels and 32 u by under 1e-11 at these sizes (coordinates below 2^9): with
    every pixel at least 1e-7 from a rounding tie and from the four limits of the inside test, no rounding and no inside decision can flip, and
    the comparison with the device leaves out no pixel.  A case that misses the margin gets other numbers, not another bound."""
    n = 0
    for c, m in models:
        if c["model"] != lm.FISHEYE:
            continue
        assert np.isfinite(m["u"]).all() and np.isfinite(m["v"]).all()
        assert m["tie_margin"].min() >= MARGIN, (c["name"], m["tie_margin"].min())
        assert m["limit_distance"].min() >= MARGIN, (c["name"], m["limit_distance"].min())
        n += 1
    assert n == 4 * len(lm.SIZES)


# ---- an independent check of the formulas: the FORWARD projection (an ideal point to the pixel it is seen at in the distorted image), written from
# COLMAP's model definitions per model and with none of lens_model's code; inverted by Newton with a numeric Jacobian
def _project(model, p, x, y):
    """normalised ideal coordinates -> pixel of the distorted image (COLMAP's pixel coordinates)"""
    r2 = x * x + y * y
    if model == "SIMPLE_PINHOLE":
        return p[0] * x + p[1], p[0] * y + p[2]
    if model == "PINHOLE":
        return p[0] * x + p[2], p[1] * y + p[3]
    if model == "SIMPLE_RADIAL":
        d = p[3] * r2
        return p[0] * (x + x * d) + p[1], p[0] * (y + y * d) + p[2]
    if model == "RADIAL":
        d = p[3] * r2 + p[4] * r2 * r2
        return p[0] * (x + x * d) + p[1], p[0] * (y + y * d) + p[2]
    if model in ("OPENCV", "FULL_OPENCV"):
        k1, k2, p1, p2 = p[4:8]
        k3, k4, k5, k6 = p[8:12] if model == "FULL_OPENCV" else (0.0, 0.0, 0.0, 0.0)
        radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
        return p[0] * (x * radial + dx) + p[2], p[1] * (y * radial + dy) + p[3]
    # the fisheye models: the equidistant angle theta = atan(r), distorted by a polynomial in theta^2
    r = np.sqrt(r2)
    theta = np.arctan2(r, 1.0)
    if model == "OPENCV_FISHEYE":
        fx, fy, cx, cy = p[:4]
        poly = 1 + p[4] * theta ** 2 + p[5] * theta ** 4 + p[6] * theta ** 6 + p[7] * theta ** 8
    elif model == "SIMPLE_RADIAL_FISHEYE":
        fx, fy, cx, cy = p[0], p[0], p[1], p[2]
        poly = 1 + p[3] * theta ** 2
    elif model == "RADIAL_FISHEYE":
        fx, fy, cx, cy = p[0], p[0], p[1], p[2]
        poly = 1 + p[3] * theta ** 2 + p[4] * theta ** 4
    else:
        raise ValueError(model)
    scale = np.where(r > 1e-12, theta * poly / np.where(r > 1e-12, r, 1.0), 1.0)
    return fx * x * scale + cx, fy * y * scale + cy


def _invert(model, p, u, v):
    """the ideal (x, y) that _project sends to (u, v): Newton from the pinhole guess, numeric Jacobian"""
    f = p[0]
    c = (p[1], p[2]) if model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE") else (p[2], p[3])
    x, y = (u - c[0]) / f, (v - c[1]) / f
    e = 1e-7
    for _ in range(50):
        pu, pv = _project(model, p, x, y)
        ax, av = _project(model, p, x + e, y)
        bx, bv = _project(model, p, x, y + e)
        j11, j21, j12, j22 = (ax - pu) / e, (av - pv) / e, (bx - pu) / e, (bv - pv) / e
        det = j11 * j22 - j12 * j21
        du, dv = u - pu, v - pv
        x, y = x + (j22 * du - j12 * dv) / det, y + (-j21 * du + j11 * dv) / det
    return x, y


def test_formulas_against_an_independent_projection():
    """Through the reader on the fixture: for each of the nine models with a lens, random pixels of the distorted image (COLMAP coordinates, inside the
    part of the image where the model is one-to-one) are taken back to the ideal position by inverting the forward projection; the model's
    source_coordinates, evaluated at that ideal position through an output camera of its own, must return the starting pixel within 1e-9.
    This holds the parameter order, the formulas and the half-pixel shift together."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden_colmap", os.path.join(here, "golden", "make_golden_colmap.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    import ctypes as C
    from line3d_amd import capi
    # every camera of the fixture through the reader: an image file that names each camera once, beside the fixture's camera file
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(os.path.join(here, "golden", "colmap_small", "txt", "cameras.txt"), d)
        with open(os.path.join(d, "images.txt"), "w") as f:
            for k, cam in enumerate(gen.CAMERAS):
                f.write("%d 1 0 0 0 0 0 0 %d im%d.jpg\n\n" % (k + 1, cam[0], k))
        scene = sfm.read_colmap(d)
    rng = np.random.default_rng(7)
    checked = 0
    for cam, (_, _, name, params) in zip(scene.cameras, gen.CAMERAS):
        if cam["lens"] is None:
            continue
        lens = cam["lens"]
        w, h = cam["size"]
        u = rng.uniform(0.2 * w, 0.8 * w, 200)
        v = rng.uniform(0.2 * h, 0.8 * h, 200)
        x, y = _invert(name, list(params), u, v)
        pu, pv = _project(name, list(params), x, y)
        assert np.abs(pu - u).max() < 1e-9 and np.abs(pv - v).max() < 1e-9, name          # the inversion converged
        # an output camera whose pixel (j, i) = (3, 2) looks along (x, y): fx' = fy' = 1, cx' = 3 - x, cy' = 2 - y
        for n in range(len(u)):
            uu, vv = lm.source_coordinates(4, 3, (1.0, 1.0, 3.0 - x[n], 2.0 - y[n]), lens.model, (lens.fx, lens.fy, lens.cx, lens.cy), list(lens.k))
            # the library's pixel (0, 0) is COLMAP's (0.5, 0.5)
            assert abs(uu[2, 3] + 0.5 - u[n]) < 1e-9 and abs(vv[2, 3] + 0.5 - v[n]) < 1e-9, (name, n, uu[2, 3] + 0.5, u[n], vv[2, 3] + 0.5, v[n])
        checked += 1
    assert checked == 9
