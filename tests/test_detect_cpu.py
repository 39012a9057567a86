"""CPU side of the line segment detector's checks: the agreement measure on the committed reference results
(tests/golden/detect_ref.npz), the stored floor, and which facade overload an image type selects."""
import os
import subprocess

import numpy as np
import pytest

import detect_metric as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "detect_ref.npz")))


def _noisy(g, key):
    return [g["%s_noisy%02d" % (key, i)] for i in range(int(g["n_noisy"]))]


def test_metric_on_the_golden(golden):
    refs = _noisy(golden, "ref")
    assert len(refs) == 12 and all(len(r) > 0 and r.shape[1] == 7 for r in refs)
    for r in refs:
        assert dm.cover(r, r) == 1.0
        assert dm.cover(r, np.zeros((0, 4))) == 0.0 and dm.cover(np.zeros((0, 4)), r) == 0.0
    halves = [np.concatenate([r[:, :2], 0.5 * (r[:, :2] + r[:, 2:4])], axis=1) for r in refs]
    recall = dm.pooled(zip(refs, halves))
    assert 0.4 < recall < 0.6, recall                        # a detector returning half of every segment
    assert dm.pooled(zip(halves, refs)) == 1.0               # ... is still precise
    # a segment 3 px aside, or turned by 10 degrees, covers nothing
    a = np.array([[10.0, 10.0, 110.0, 10.0]])
    assert dm.cover(a, a + [0, 3, 0, 3]) == 0.0 and dm.cover(a, a + [0, 1, 0, 1]) == 1.0
    t = np.deg2rad(10.0)
    assert dm.cover(a, np.array([[10.0, 10.0, 10 + 100 * np.cos(t), 10 + 100 * np.sin(t)]])) == 0.0


def test_stored_floor_is_the_recomputed_one(golden):
    a, b = _noisy(golden, "ref"), _noisy(golden, "refB")
    floor = dm.reference_floor(a, b)
    assert floor == float(golden["floor"])
    assert 0.9 < floor < 1.0
    assert dm.pooled(zip(a, b)) >= floor and dm.pooled(zip(b, a)) >= floor      # pooled >= minimum: the reference itself passes
    assert len(golden["ref_flat"]) == 0 and all(len(golden["ref_" + k]) >= 1 for k in ("edge0", "edge90", "edge45", "edge7", "diag", "tiny"))


def test_rescale_and_grey_formulas():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    assert np.array_equal(dm.rescale_u8(img, 64, 48), img)
    flat = np.full((48, 64, 3), 77, np.uint8)
    assert np.all(dm.rescale_u8(flat, 32, 24) == 77) and np.all(dm.grey_u8(flat) == 77)
    half = dm.rescale_u8(img[..., 0], 32, 24)                # exact halving: the mean of each 2x2 block, rounded half up
    blocks = img[..., 0].astype(np.int64).reshape(24, 2, 32, 2).sum(axis=(1, 3))
    assert np.array_equal(half, ((blocks * 16384 + 32768) >> 16).astype(np.uint8))
    assert dm.grey_u8(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)).tolist() == [[76, 150, 29]]
    assert float(dm.upscale_factor(640, 480, 320, 240)) == 2.0 and float(dm.upscale_factor(640, 480, 640, 480)) == 1.0


STUBS = r'''
#include "line3D_amd.hpp"
struct Mat3 { double m[9]; double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Step { size_t s; operator size_t() const { return s; } };
struct PixelMat { int rows, cols; unsigned char* data; Step step; int channels() const { return 3; } };     // the members of cv::Mat the facade reads
struct SizeMat { int rows, cols; };
void use(L3D::Line3D& l, const IMAGE& img)
{
    Mat3 K{ { 1, 0, 0, 0, 1, 0, 0, 0, 1 } };
    Vec3 t{ { 0, 0, 0 } };
    std::list<unsigned int> wps{ 1, 2, 3 };
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    l.addImage(0, img, K, K, t, wps);
    l.addImage(1, img, K, K, t, wps, 800, false);
    l.addImage_fixed_sim(2, img, K, K, t, sim);
    l.addImage_fixed_sim(3, img, K, K, t, sim, 800, false);
}
'''


def _undefined_symbols(tmp_path, image_type):
    src = tmp_path / (image_type + ".cpp")
    src.write_text(STUBS)
    obj = str(tmp_path / (image_type + ".o"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-DIMAGE=" + image_type, "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])
    out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


def test_facade_overload_selection(tmp_path):
    """compile only: an image type with pixels (.data, .step, .channels()) reaches the pixel calls, a size-only type the cache calls"""
    pix, size = _undefined_symbols(tmp_path, "PixelMat"), _undefined_symbols(tmp_path, "SizeMat")
    assert {"l3d_line3d_add_image_pixels", "l3d_line3d_add_image_pixels_fixed_sim"} <= pix
    assert not ({"l3d_line3d_add_image_ex", "l3d_line3d_add_image_fixed_sim_ex"} & pix)
    assert {"l3d_line3d_add_image_ex", "l3d_line3d_add_image_fixed_sim_ex"} <= size
    assert not ({"l3d_line3d_add_image_pixels", "l3d_line3d_add_image_pixels_fixed_sim"} & size)


def test_image_arguments():
    from line3d_amd import capi
    img = np.zeros((20, 30), np.uint8)
    _, w, h, ch, stride = capi.image_arguments(img)
    assert (w, h, ch, stride) == (30, 20, 1, 30)
    _, w, h, ch, stride = capi.image_arguments(np.zeros((20, 50, 3), np.uint8)[:, :30])
    assert (w, h, ch, stride) == (30, 20, 3, 150)
    _, w, h, ch, stride = capi.image_arguments(np.zeros((20, 60), np.uint8)[:, ::2])          # pixels not contiguous: copied
    assert (w, h, ch, stride) == (30, 20, 1, 30)
    with pytest.raises(TypeError):
        capi.image_arguments(np.zeros((20, 30), np.float32))
