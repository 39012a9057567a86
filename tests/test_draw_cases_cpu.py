"""The drawing's case table (tests/draw_cases.py) on a machine without a GPU: every case is what its name claims (asserted with the key plane of
tests/draw_model.py, the rules of include/line3d_amd.h "PROJECTION AND OVERLAYS" in numpy), the host entry point l3d_test_draw_segments_host -- the
very functions the kernels run -- gives the model's bytes on all of them, padding bytes and a fourth channel stay untouched, every refusal comes
with its code and cause, and the host code of both layers is clean under AddressSanitizer and UBSan (tests/cpp/project_draw_asan.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import draw_cases as dc
import draw_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [c["name"] for c in dc.CASES]


def host(case):
    from line3d_amd import capi
    return capi.draw_segments_host(case["image"], case["segments"], case["colors"], case["color_index"], case["width_px"], case["opacity"])


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(name):
    case = dc.BY_NAME[name]
    img = np.asarray(case["image"])
    h, w = img.shape[:2]
    plane = dm.key_plane((h, w), case["segments"], case["width_px"])
    q, k = plane >> 24, plane & 0xFFFFFF
    claim = case["claim"]
    want = dc.model_of(case)
    if claim[0] in ("q_rows", "q_cols"):
        qq = q if claim[0] == "q_rows" else q.T
        lines, (a, b) = claim[1], claim[2]
        for line, value in lines.items():
            assert np.all(qq[line, a:b + 1] == value), (line, qq[line, a:b + 1])
        for line in (min(lines) - 1, max(lines) + 1):
            assert np.all(qq[line, :] == 0)
    elif claim[0] == "span":
        major = np.flatnonzero((q > 0).any(axis=0 if w >= h else 1))
        assert len(major) == claim[1] and major[-1] - major[0] + 1 == claim[1]
    elif claim[0] == "covered":
        assert claim[1] <= int((q > 0).sum()) <= claim[2], int((q > 0).sum())
    elif claim[0] == "unchanged":
        assert np.array_equal(want, img)
    elif claim[0] == "winner":
        assert (q > 0).any() and np.all(k[q > 0] == claim[1])
    elif claim[0] == "generic":
        assert (q > 0).any() and not np.array_equal(want, img)
    else:
        raise AssertionError(claim)
    if img.ndim == 3 and img.shape[2] == 4:
        assert np.array_equal(want[..., 3], img[..., 3])


def test_the_fan_meets_in_one_pixel():
    """4097 segments through (32, 24): every one of them covers that pixel fully, and the last one wins it"""
    case = dc.BY_NAME["fan_4097"]
    assert len(case["segments"]) == 4097
    for k in (0, 1000, 4096):
        assert dm.key_plane((48, 64), case["segments"][k:k + 1], 1.0)[24, 32] >> 24 == 255
    plane = dm.key_plane((48, 64), case["segments"], 1.0)
    assert plane[24, 32] == (255 << 24) | 4096


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model_byte_for_byte(name):
    case = dc.BY_NAME[name]
    got = host(case)
    assert got.dtype == np.uint8 and got.shape == np.asarray(case["image"]).shape
    assert np.array_equal(got, dc.model_of(case)), name
    if got.base is not None and got.base.ndim == 2 and got.base.shape[1] > got.shape[1]:      # rows with padding: every padding byte as it was
        assert np.all(got.base[:, got.shape[1]:] == 0xA5)


def test_the_padded_case_has_padding():
    from line3d_amd import capi
    out = capi._draw_image_copy(dc.B)
    assert out.strides[0] == 40 and out.shape == (17, 33) and out.base.shape == (17, 40)


@pytest.mark.parametrize("name", [r[0] for r in dc.REFUSALS])
def test_refusals(name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in dc.REFUSALS if r[0] == name)
    kw = dc.refusal_arguments(overrides)
    with pytest.raises(capi.L3DError) as e:
        capi.draw_segments_host(kw["image"], kw["segments"], kw["colors"], kw["color_index"], kw["width_px"], kw["opacity"])
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_raw_refusals():
    """null pointers, counts and sizes out of range, a short row stride: L3D_ERR_INVALID; what the rules cannot hold: L3D_ERR_UNSUPPORTED (5)"""
    from line3d_amd import capi
    lib = capi.load_library()
    px = np.zeros((8, 8, 3), np.uint8)
    segs = np.array([[1, 1, 6, 6]], np.float32)
    col = np.array([[255, 0, 0, 255]], np.uint8)
    good = [capi._p(px), C.c_int(8), C.c_int(8), C.c_int(3), C.c_size_t(24), capi._p(segs), C.c_int(1), capi._p(col), C.c_int(1), None, C.c_double(1.0), C.c_int(255)]
    assert lib.l3d_test_draw_segments_host(*good) == 0
    for i, bad, code in ((0, None, 1), (5, None, 1), (7, None, 1), (6, C.c_int(-1), 1), (1, C.c_int(0), 1), (2, C.c_int(-2), 1), (3, C.c_int(5), 1),
                         (4, C.c_size_t(23), 1), (8, C.c_int(0), 1), (6, C.c_int((1 << 24) + 1), 5), (1, C.c_int(32769), 5)):
        args = list(good)
        args[i] = bad
        assert lib.l3d_test_draw_segments_host(*args) == code, (i, code)


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/project_draw_asan.cpp: l3d_project.hpp and l3d_draw.hpp -- the argument checks, the pair function, the clip, the pieces, the walk and
    the blend -- and a main of its own, built with AddressSanitizer and UBSan"""
    exe = str(tmp_path / "project_draw_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "project_draw_asan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout, r.stdout
