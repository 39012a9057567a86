"""The undistortion contract (include/line3d_amd.h) as tests/undistort_model.py states it in numpy, checked without a device: identities, hand-computed
values, the fixed-point quantisation against unquantised bilinear interpolation, the inverse map, the margins that make the device test
(tests/test_gpu_undistort.py) exact, the sign conventions of the SfM readers, and that the facade additions and the example compile."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import undistort_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(shape, seed=5):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _smooth(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.rint(127.5 + 80.0 * np.sin(xx / 5.0) * np.cos(yy / 7.0) + 40.0 * np.sin((xx + yy) / 11.0)).astype(np.uint8)


def _formulas(img, fx, fy, cx, cy, k1, k2):
    """the model's arithmetic with the pass-through switched off: k1 = k2 = 0 goes through the formulas"""
    saved = um.EPS
    um.EPS = -1.0
    try:
        return um.undistort(img, fx, fy, cx, cy, k1, k2)
    finally:
        um.EPS = saved


@pytest.mark.parametrize("shape", [(29, 37), (30, 36), (29, 37, 3), (8, 8), (1, 1), (5, 2, 3)])
def test_identity_without_distortion(shape):
    img = _noise(shape)
    h, w = shape[:2]
    for fx, fy, cx, cy in ((30.0, 30.0, w / 2.0, h / 2.0), (28.0, 31.0, 16.25, 15.75), (7.3, 1e3, -4.1, 900.7)):
        r = _formulas(img, fx, fy, cx, cy, 0.0, 0.0)            # the formulas themselves are the identity ...
        assert np.array_equal(r["image"], img) and r["inside"].all() and not r["partial"].any()
        assert np.array_equal(um.undistort(img, fx, fy, cx, cy, 0.0, 0.0)["image"], img)     # ... and so is the pass-through
        assert np.array_equal(um.undistort(img, fx, fy, cx, cy, 1e-12, -1e-12)["image"], img)


def test_hand_computed_3x3():
    """fx = fy = 2, cx = cy = 1, k1 = 0.25, k2 = 0.  Corner (j, i) = (0, 0): x = y = -0.5, r2 = 0.5, kr = 1.125, u = v = 2 (-0.5625) + 1 = -0.125:
    iu = iv = -4, x0 = y0 = -1, a = b = 28: only the tap (0, 0) is on the image, out = (28 28 p00 + 512) >> 10.  Edge (1, 0): x = 0, y = -0.5,
    r2 = 0.25, kr = 1.0625, u = 1, v = 2 (-0.53125) + 1 = -0.0625: iv = -2, y0 = -1, b = 30, a = 0: out = (32 30 p(0,1) + 512) >> 10.
    Centre: itself."""
    img = np.array([[200, 100, 40], [90, 255, 10], [30, 60, 120]], np.uint8)
    r = um.undistort(img, 2.0, 2.0, 1.0, 1.0, 0.25, 0.0)
    assert r["u"][0, 0] == -0.125 and r["v"][0, 0] == -0.125 and r["v"][0, 1] == -0.0625 and r["u"][0, 1] == 1.0
    expect = np.array([[(784 * 200 + 512) >> 10, (960 * 100 + 512) >> 10, (784 * 40 + 512) >> 10],
                       [(960 * 90 + 512) >> 10, 255, (960 * 10 + 512) >> 10],
                       [(784 * 30 + 512) >> 10, (960 * 60 + 512) >> 10, (784 * 120 + 512) >> 10]], np.uint8)
    assert expect.tolist() == [[153, 94, 31], [84, 255, 9], [23, 56, 92]]
    assert np.array_equal(r["image"], expect)
    assert r["inside"].all() and r["partial"].sum() == 8 and r["x0_negative"].sum() == 3


def test_negative_fixed_point_coordinate():
    """iu = -1 gives x0 = -1, a = 31 (floor, not truncation)"""
    x0, a, y0, b = um.quantise(np.array([[-1.0 / 32.0]]), np.array([[-33.0 / 32.0 + 1.0 / 16.0]]), np.array([[True]]))
    assert (x0[0, 0], a[0, 0]) == (-1, 31)
    assert (y0[0, 0], b[0, 0]) == (-1, 1)
    # through the image: fx = 32, cx = 0, k1 chosen so that column 1 reads u = -1/32: x = 1/32, r2 = 1/1024, kr = -1/32 = 1 + k1 / 1024
    img = np.array([[64, 128]], np.uint8)
    r = um.undistort(img, 32.0, 1.0, 0.0, 0.0, -1056.0, 0.0)
    assert r["u"][0, 1] == -1.0 / 32.0 and r["x0_negative"][0, 1]
    assert r["image"][0, 1] == (31 * 32 * 64 + 512) >> 10          # weight a = 31 on column 0, the tap at column -1 is black


def test_last_column_gives_the_pixel_itself():
    """u exactly width - 1: a = 0, the tap at column `width` has weight 0"""
    img = _noise((4, 5))
    # column 3 of 5 reads u = 4: fx = 1, cx = 0, x = 3, kr = 4 / 3 = 1 + k1 9 -> k1 = 1 / 27 in row 0 (y = 0)
    r = um.undistort(img, 1.0, 1.0, 0.0, 0.0, 1.0 / 27.0, 0.0)
    assert abs(r["u"][0, 3] - 4.0) < 1e-12 and r["inside"][0, 3] and not r["partial"][0, 3]
    assert r["image"][0, 3] == img[0, 4]


def _newton_inverse(u, v, fx, fy, cx, cy, k1, k2):
    """(u, v) source pixel -> (j, i) with distort(j, i) = (u, v): Newton on the radius, r_d = r (1 + k1 r^2 + k2 r^4)"""
    xd, yd = (u - cx) / fx, (v - cy) / fy
    rd = np.hypot(xd, yd)
    r = rd.copy()
    for _ in range(60):
        f = r * (1.0 + (k2 * r * r + k1) * r * r) - rd
        df = 1.0 + 3.0 * k1 * r * r + 5.0 * k2 * r ** 4
        r = r - f / df
    s = np.where(rd > 0, r / np.where(rd > 0, rd, 1.0), 1.0)
    return fx * (xd * s) + cx, fy * (yd * s) + cy


@pytest.mark.parametrize("case", um.CASES, ids=lambda c: "%dx%dx%d_k%g_%g" % (c[0], c[1], c[2], c[8], c[9]))
def test_case_margins_and_inverse(case):
    """every case of the device test: no pixel within 1e-6 of a rounding tie or of an inside / outside limit (doubles on the device differ from
    numpy's by rounding errors ten orders of magnitude smaller, so no decision can move), and Newton's inverse leads back to the pixel"""
    w, h, ch = case[:3]
    _, img = um.case_image(case)
    r = um.undistort(img, *case[4:])
    tie, lim = float(r["tie_margin"].min()), float(r["limit_distance"].min())
    print("%s: outside %d, partial %d, x0 < 0: %d; smallest tie margin %.3g, smallest limit distance %.3g"
          % (case, (~r["inside"]).sum(), r["partial"].sum(), r["x0_negative"].sum(), tie, lim))
    assert tie >= 1e-6 and lim >= 1e-6
    ins = r["inside"]
    jj, ii = _newton_inverse(r["u"][ins], r["v"][ins], *case[4:])
    i0, j0 = np.nonzero(ins)
    assert np.abs(jj - j0).max() <= 1e-9 and np.abs(ii - i0).max() <= 1e-9


@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("case", [um.CASES[1], um.CASES[2], um.CASES[3][:2] + (1,) + um.CASES[3][3:], um.CASES[5]], ids=lambda c: "%dx%d_k%g" % (c[0], c[1], c[8]))
def test_against_unquantised_bilinear(kind, case):
    """scipy's bilinear interpolation at the unquantised (u, v), zero outside: each coordinate moves by at most 1/64 px when it is rounded to
    1/32 px, which changes a bilinear value by at most Dx / 64 (Dy / 64) -- D the largest neighbour difference of the zero-padded source --,
    and the final rounding adds 1/2"""
    from scipy.ndimage import map_coordinates
    w, h = case[:2]
    img = _smooth(h, w) if kind == "smooth" else _noise((h, w), seed=9)
    r = um.undistort(img, *case[4:])
    pad = np.zeros((h + 4, w + 4))
    pad[2:-2, 2:-2] = img
    Dx, Dy = np.abs(np.diff(pad, axis=1)).max(), np.abs(np.diff(pad, axis=0)).max()
    ins = r["inside"]
    ref = map_coordinates(pad, [r["v"][ins] + 2.0, r["u"][ins] + 2.0], order=1, mode="constant", cval=0.0)
    diff = np.abs(r["image"][ins].astype(np.float64) - ref)
    bound = 0.5 + (Dx + Dy) / 64.0 + 1e-9
    print("%s %s: largest difference %.4f, bound %.4f" % (kind, case, diff.max(), bound))
    assert diff.max() <= bound
    assert not r["image"][~ins].any()


def test_extreme_coefficients():
    _, img = um.case_image(um.CASES[3])
    r = um.undistort(img, 70.0, 70.0, 48.0, 40.0, 1e6, 0.0)
    nz = np.argwhere(r["image"].any(axis=-1))
    assert nz.tolist() == [[40, 48]] and np.array_equal(r["image"][40, 48], img[40, 48])
    assert not um.undistort(img, 70.0, 70.0, 48.0, 40.0, float("nan"), 0.0)["image"].any()
    assert not um.undistort(img, 70.0, 70.0, 48.0, 40.0, 0.1, float("nan"))["image"].any()


# ---- the SfM readers' sign conventions
NVM = """NVM_V3

2
a.jpg 500.5 1 0 0 0 0 0 0 0.125 0
b.jpg 600 1 0 0 0 1 0 0 -0.0625 0

1
0 0 5 255 255 255 2 0 0 1.0 2.0 1 0 3.0 4.0
"""
BUNDLER = """# Bundle file v0.3
2 1
500 0.125 -0.03125
1 0 0
0 1 0
0 0 1
0 0 0
600 0 0.25
1 0 0
0 1 0
0 0 1
1 0 0
0 0 5
255 255 255
2 0 0 1.0 2.0 1 0 3.0 4.0
"""


def test_sfm_cv_distortion_signs(tmp_path):
    from line3d_amd import sfm
    (tmp_path / "s.nvm").write_text(NVM)
    (tmp_path / "bundle.rd.out").write_text(BUNDLER)
    nvm = sfm.read_nvm(str(tmp_path / "s.nvm"))
    assert [c["dist"].tolist() for c in nvm.cameras] == [[0.125, 0.0], [-0.0625, 0.0]]
    assert [c["cv_dist"].tolist() for c in nvm.cameras] == [[-0.125, 0.0], [0.0625, 0.0]]          # main_vsfm.cpp:259: k1 = -d
    bun = sfm.read_bundler(str(tmp_path / "bundle.rd.out"))
    assert [c["dist"].tolist() for c in bun.cameras] == [[0.125, -0.03125], [0.0, 0.25]]
    assert [c["cv_dist"].tolist() for c in bun.cameras] == [[0.125, -0.03125], [0.0, 0.25]]         # main_bundler.cpp:273-274: as they are
    from line3d_amd.capi import load_library
    lib = load_library()
    k = (C.c_double * 2)()
    assert lib.l3d_sfm_camera_cv_distortion(None, C.c_int(0), k) != 0


# ---- the facade additions compile against an image type with pixels and one with a size only
FACADE_SRC = r'''
#include "line3D_amd.hpp"
struct Mat3 { double m[9]; double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct PixelImage { int cols, rows; unsigned char* data; size_t step; int channels() const { return 3; } };
struct SizeImage { int cols, rows; };
int main() {
    L3D::Line3D l("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false);
    std::list<unsigned int> wps{ 1, 2, 3 };
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    Mat3 Km{ { 500, 0, 32, 0, 500, 24, 0, 0, 1 } };
    Vec3 tm{ { 0, 0, 0 } };
    std::vector<unsigned char> px(64 * 48 * 3, 128);
    PixelImage img{ 64, 48, px.data(), 64 * 3 };
    SizeImage size_only{ 64, 48 };
    l.addImageDistorted(0, img, Km, Km, tm, -0.1, 0.01, wps);
    l.addImageDistorted(1, img, Km, Km, tm, -0.1, 0.01, wps, 800, false);
    l.addImage_fixed_simDistorted(2, img, Km, Km, tm, -0.1, 0.0, sim);
    l.addImage_fixed_simDistorted(3, img, Km, Km, tm, -0.1, 0.0, sim, 1920, false);
    l.addImageDistorted(4, size_only, Km, Km, tm, -0.1, 0.01, wps, 1920, false);            // the cache path: the coefficients are ignored
    l.addImage_fixed_simDistorted(5, size_only, Km, Km, tm, -0.1, 0.0, sim, 1920, false);
    const bool done = l.undistortImage(img, Km, -0.1, 0.01);                                 // the drivers' structure: undistort, then addImage
    l.addImage(6, img, Km, Km, tm, wps, 1920, false);
    return (l.numCameras() == 0 && !done) || l.valid() ? 0 : 1;      // (without a GPU every call reports and returns)
}
'''


def test_facade_additions_compile_and_link():
    lib = os.path.join(ROOT, "line3d_amd")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.cpp")
        with open(src, "w") as f:
            f.write(FACADE_SRC)
        exe = os.path.join(td, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
        assert subprocess.run([exe], stderr=subprocess.DEVNULL, cwd=td).returncode == 0


def test_example_compiles_and_links():
    lib = os.path.join(ROOT, "line3d_amd")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "main_vsfm_amd")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "main_vsfm_amd.cpp"),
                               "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
        assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 2            # (usage: no arguments)
