"""The undistortion planner (l3d_undistort_plan, host code: no device) against tests/remap_model.py, which shares no code with it: the nine COLMAP
models with a lens read from tests/golden/colmap_small, a strong fisheye and a strong barrel BROWN lens; the properties the header promises; and
every refusal."""
import json
import os
import shutil
import tempfile

import numpy as np
import pytest

import lens_model as lm
import remap_model as rm
from line3d_amd import capi, sfm

HERE = os.path.dirname(os.path.abspath(__file__))
# The bound on |K' - model K'| / fx': TEN TIMES the largest difference measured on this table ("measured" in the file; 0 counts as one ulp of 1).
# The factor: the host libm and numpy may differ in atan / tan by ulps, and a Newton iteration that has converged amplifies that little.
TOLERANCE = json.load(open(os.path.join(HERE, "golden", "remap_plan_tolerance.json")))
BOUND = 10.0 * max(TOLERANCE["measured"], 2.0 ** -52)
INVALID = 1
ALPHAS = (0.0, 0.25, 0.5, 1.0)
MODES = (None, "keep_focal", (37, 29), (200, 90))


def _colmap_lenses():
    """(name, model, source camera, coefficients, size) of every camera of the fixture that has a lens"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_colmap", os.path.join(HERE, "golden", "make_golden_colmap.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(os.path.join(HERE, "golden", "colmap_small", "txt", "cameras.txt"), d)
        with open(os.path.join(d, "images.txt"), "w") as f:
            for k, cam in enumerate(gen.CAMERAS):
                f.write("%d 1 0 0 0 0 0 0 %d im%d.jpg\n\n" % (k + 1, cam[0], k))
        scene = sfm.read_colmap(d)
    out = []
    for cam, (_, _, name, _) in zip(scene.cameras, gen.CAMERAS):
        if cam["lens"] is not None:
            L = cam["lens"]
            out.append((name, int(L.model), (L.fx, L.fy, L.cx, L.cy), tuple(L.k), tuple(cam["size"])))
    return out


def _table():
    t = _colmap_lenses()
    assert len(t) == 9
    # of the test's own: a fisheye whose corners lie past 120 degrees (clamped border points), and a barrel lens whose radial function turns over
    # inside the image (border points that cannot be inverted)
    t.append(("strong_fisheye", rm.FISHEYE, (150.0, 152.0, 161.3, 118.6), (-0.02, 0.004, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (320, 240)))
    t.append(("strong_barrel", rm.BROWN, (200.0, 200.0, 158.7, 121.4), (-0.25, 0.0, 0.001, -0.002, 0.0, 0.0, 0.0, 0.0), (320, 240)))
    return t


TABLE = _table()


def _lens(model, cam, k):
    return capi.lens(model, list(k), camera=cam)


def _diff(K, Km):
    return max(abs(K[0, 0] - Km[0, 0]), abs(K[1, 1] - Km[1, 1]), abs(K[0, 2] - Km[0, 2]), abs(K[1, 2] - Km[1, 2])) / abs(Km[0, 0])


def measure():
    """the largest relative difference over the table (what tests/golden/remap_plan_tolerance.json records)"""
    worst = 0.0
    for name, model, cam, k, size in TABLE:
        for alpha in ALPHAS:
            for mode in MODES:
                for max_dim in ((0, 100) if mode == "keep_focal" else (0,)):
                    K, _ = capi.undistort_plan(_lens(model, cam, k), size, alpha, mode, max_dim)
                    Km, _ = rm.plan(model, cam, k, size, alpha, mode, max_dim)
                    worst = max(worst, _diff(K, Km))
    return worst


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r[0])
def test_planner_equals_model(row):
    name, model, cam, k, size = row
    for alpha in ALPHAS:
        for mode in MODES:
            for max_dim in ((0, 100) if mode == "keep_focal" else (0,)):
                K, wh = capi.undistort_plan(_lens(model, cam, k), size, alpha, mode, max_dim)
                Km, whm = rm.plan(model, cam, k, size, alpha, mode, max_dim)
                print(name, alpha, mode, max_dim, wh, _diff(K, Km))
                assert wh == whm, (name, alpha, mode, wh, whm)
                assert _diff(K, Km) <= BOUND, (name, alpha, mode, _diff(K, Km), BOUND)
                assert K[0, 1] == 0.0 and K[1, 0] == 0.0 and K[2].tolist() == [0.0, 0.0, 1.0]
                assert abs(K[1, 1] / K[0, 0] - cam[1] / cam[0]) <= 1e-12 * cam[1] / cam[0]          # the pixel aspect is kept
                if mode == "keep_focal" and (max_dim == 0 or max(wh) <= max_dim and K[0, 0] == cam[0]):
                    assert K[0, 0] == cam[0]
                if mode == "keep_focal" and max_dim:
                    assert max(wh) <= max_dim + 1
                if mode not in (None, "keep_focal"):
                    assert wh == mode


def test_the_table_exercises_the_clamps():
    seen = {}
    for name, model, cam, k, size in TABLE:
        seen[name] = rm.border_points(model, cam, k, *size)["clamped"]
    assert seen["strong_fisheye"].any() and not seen["strong_fisheye"].all()
    assert seen["strong_barrel"].any() and not seen["strong_barrel"].all()
    assert sum(1 for v in seen.values() if not v.any()) >= 5


def test_no_distortion_gives_the_camera_back():
    cam, size = (310.0, 305.5, 161.25, 117.5), (320, 240)
    for alpha in (0.0, 0.3, 1.0):
        for lens in (capi.lens("brown", [0.0] * 8, camera=cam), capi.lens(0, [], camera=cam)):
            K, wh = capi.undistort_plan(lens, size, alpha)
            assert wh == size
            assert _diff(K, np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]])) <= BOUND
            K, wh = capi.undistort_plan(lens, size, alpha, "keep_focal")
            assert wh == size and K[0, 0] == cam[0]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r[0])
def test_focal_length_falls_with_alpha(row):
    name, model, cam, k, size = row
    fx = [capi.undistort_plan(_lens(model, cam, k), size, a)[0][0, 0] for a in np.linspace(0.0, 1.0, 11)]
    assert all(b <= a * (1.0 + 1e-15) for a, b in zip(fx, fx[1:])), fx
    assert fx[-1] < fx[0] or name in ("PINHOLE", "SIMPLE_PINHOLE")


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r[0])
def test_alpha_0_leaves_no_blank_pixel_and_alpha_1_keeps_every_border_point(row):
    name, model, cam, k, size = row
    w, h = size
    src = np.zeros((h, w), np.uint8)
    for mode in (None, "keep_focal", (200, 90)):
        max_dim = 400 if mode == "keep_focal" else 0              # (keeps the model's planes small)
        K, wh = capi.undistort_plan(_lens(model, cam, k), size, 0.0, mode, max_dim)
        m = rm.remap(src, wh, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), model, cam, k)
        assert m["valid"].min() == 255, (name, mode, int((m["valid"] == 0).sum()))
        K, wh = capi.undistort_plan(_lens(model, cam, k), size, 1.0, mode, max_dim)
        p = rm.border_points(model, cam, k, w, h)
        keep = ~p["clamped"]
        uu, vv = K[0, 0] * p["x"][keep] + K[0, 2], K[1, 1] * p["y"][keep] + K[1, 2]
        assert keep.any() and uu.min() >= -0.5 and uu.max() <= wh[0] - 0.5 and vv.min() >= -0.5 and vv.max() <= wh[1] - 0.5, (name, mode)


def test_refusals():
    cam, size = (300.0, 300.0, 160.0, 120.0), (320, 240)
    good = capi.lens("fisheye", [-0.01], camera=cam)
    nan = float("nan")

    def refused(*a, **kw):
        with pytest.raises(capi.L3DError) as e:
            capi.undistort_plan(*a, **kw)
        assert e.value.code == INVALID and "undistort_plan" in str(e.value), str(e.value)
        return str(e.value)
    for alpha in (-1e-9, 1.0 + 1e-9, nan):
        assert "alpha" in refused(good, size, alpha)
    # a degenerate rectangle: a fisheye that looks far past the image (principal point 1000 rows above it), every border point beyond 90 degrees and
    # clamped onto the circle of radius r_max -- the top edge's largest y (straight down) lies below the bottom edge's smallest (at its corners)
    assert "degenerate" in refused(capi.lens("fisheye", [], camera=(100.0, 100.0, 160.0, -1000.0)), size, 0.0)
    with pytest.raises(ValueError, match="degenerate"):
        rm.plan(rm.FISHEYE, (100.0, 100.0, 160.0, -1000.0), (), size, 0.0)
    # sizes below 8 and above the detector's limits, source and output
    for bad in ((7, 240), (320, 7), ((1 << 24) + 1, 8), (40000, 40000)):
        assert "size" in refused(good, bad, 0.0)
        assert "size" in refused(good, size, 0.0, bad)
    assert "size" in refused(capi.lens("brown", [0.0] * 8, camera=(3.0, 3.0, 160.0, 120.0)), size, 0.0, "keep_focal")       # plans 2 x 2
    assert "out size" in refused(good, size, 0.0, (0, 100))
    assert "out size" in refused(good, size, 0.0, (-1, 0))
    assert "max_dim" in refused(good, size, 0.0, "keep_focal", -1)
    for fov in (0.0, 180.0, -5.0, nan):
        assert "fov" in refused(good, size, 0.0, fov_max_deg=fov)
    # the lens: what A LENS refuses, and a lens without its source camera
    for lens in (capi.lens(3, [0.1], camera=cam), capi.lens("brown", [nan], camera=cam), capi.lens("fisheye", [0, 0, 0, 0, 0.1], camera=cam),
                 capi.lens("brown", [0.1]), capi.lens("brown", [0.1], camera=(300.0, 0.0, 160.0, 120.0)), capi.lens("brown", [0.1], camera=(-300.0, 300.0, 160.0, 120.0))):
        refused(lens, size, 0.0)
    with pytest.raises(ValueError):
        rm.plan(rm.FISHEYE, cam, (-0.01,), size, 1.5)


def test_planner_under_sanitizers(tmp_path):
    """tests/cpp/remap_plan_asan.cpp: the planner's source and a main of its own, built with AddressSanitizer and UBSan as a plain host program, over a
    grid of weak, strong and absurd lenses at several sizes, alphas and size modes, and the refusals"""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "plan_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "remap_plan_asan.cpp"),
                           os.path.join(root, "line3d_amd", "csrc", "l3d_remap_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 bad" in run.stdout, run.stdout + run.stderr
