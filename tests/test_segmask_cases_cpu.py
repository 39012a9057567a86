"""The segment mask's case table (tests/segmask_cases.py) on a machine without a GPU: every case is what its name claims (asserted with the samples
of tests/segmask_model.py, the contract of include/line3d_amd.h "A SEGMENT MASK" in numpy), the lens cases keep every sample away from a pixel's
edge, the model's lens formulas are tests/lens_model.py's on the pixel grid, the host entry point l3d_test_mask_segments_host -- the very functions
the kernels run, with 64 lanes one after the other -- equals the model bit for bit in segments and in src_index on every case, every refusal comes
with its code and cause, the host code is clean under AddressSanitizer and UBSan (tests/cpp/segmask_asan.cpp), and the C++ facade compiles."""
import os
import subprocess

import numpy as np
import pytest

import lens_model as lm
import segmask_cases as sc
import segmask_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = [c["name"] for c in sc.CASES]


def _host(case):
    from line3d_amd import capi
    return capi.mask_segments_host(case["segments"], sc.capi_mask(case))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _valid(case, i, bridged=False):
    n, v = sm.validity(case["segments"][i], case["mask"], case["kw"]["threshold"], case["lens"])
    return n, (sm.bridge(v, case["kw"]["max_gap"]) if bridged else v)


def _gaps(v):
    """lengths of the runs of invalid samples strictly between two valid samples"""
    idx = np.flatnonzero(v)
    return [int(b - a - 1) for a, b in zip(idx[:-1], idx[1:]) if b - a > 1]


def test_the_table_covers_every_kind_of_case():
    kinds = {c["claim"][0] for c in sc.CASES}
    assert kinds >= {"samples", "direction", "half", "outside", "gap", "gap_at_end", "tie", "min_length", "all_valid", "all_invalid", "threshold", "permille",
                     "permille_tie", "always_dropped", "grows", "count", "stride", "lens", "lens_inactive"}
    assert sorted({c["claim"][1] for c in sc.CASES if c["claim"][0] == "samples"}) == [2, 63, 64, 65, 128, 129]
    assert sorted({c["claim"][1] for c in sc.CASES if c["claim"][0] == "count"}) == [0, 1, 3, 4, 5, 4095, 4096, 4097]
    assert sorted({c["claim"][1] for c in sc.CASES if c["claim"][0] == "threshold"}) == [0, 1, 128, 255]
    shapes = [c["mask"].shape for c in sc.CASES]
    assert min(s[1] for s in shapes) == 16 and min(s[0] for s in shapes) == 12 and max(s[1] for s in shapes) == 96 and max(s[0] for s in shapes) == 64
    assert {c["lens"]["model"] for c in sc.CASES if c["claim"][0] == "lens"} == {sm.BROWN, sm.FISHEYE}
    assert {c["kw"]["mode"] for c in sc.CASES} == {sm.DROP, sm.CLIP, sm.SPLIT}


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(name):
    case = sc.BY_NAME[name]
    claim, kw, segs = case["claim"], case["kw"], case["segments"]
    out, src = sc.model_of(case)
    kind = claim[0]
    if kind == "samples":
        n, v = _valid(case, 0)
        assert n + 1 == claim[1] == len(v)
        assert v.any() and not v.all()
    elif kind == "direction":
        _, _, _, dx, dy = sm.samples(segs[0])
        assert {"h": dy == 0 and dx != 0, "v": dx == 0 and dy != 0, "d": dx != 0 and dy != 0}[claim[1]]
        assert (min(dx, dy) < 0) == claim[2] or claim[1] == "d"
        assert len(out) >= len(segs)
    elif kind == "half":
        assert all(float(v) % 1.0 == 0.5 for v in segs[:, [0, 2]].ravel())
        m = case["mask"]
        assert m[4, 4] == 255 and m[4, 3] == 0 and m[4, 11] == 255 and m[4, 12] == 0 and m[3].max() == 0 and m[5].max() == 0
        v = _valid(case, 0)[1]
        assert v[0] and not v[-1]                       # x = 3.5 reads pixel 4 (valid), x = 11.5 pixel 12 (invalid)
        v = _valid(case, 1)[1]
        assert not v[0] and v[-1]                       # y = 3.5 reads row 4; the segment runs down from x = 11.5
    elif kind == "outside":
        if claim[1] == "ends":
            for i in range(len(segs)):
                n, v = _valid(case, i)
                assert not v[0] and not v[-1] and v.any()
            assert len(out) == len(segs) and not np.array_equal(_bits(out), _bits(segs))
        else:
            assert not _valid(case, 0)[1].any() and not _valid(case, 1)[1].any() and _valid(case, 2)[1].all()
            assert src.tolist() == [2]
    elif kind == "gap":
        g, nruns = claim[1], claim[2]
        n, v = _valid(case, 0)
        assert kw["max_gap"] == g and (g if nruns == 1 else g + 1) in _gaps(v)
        assert len(sm.runs(sm.bridge(v, g))) == nruns
        assert len(out) == (nruns if kw["mode"] == sm.SPLIT else 1)
    elif kind == "gap_at_end":
        n, v = _valid(case, 0)
        edge = v[:kw["max_gap"]] if claim[1] == "start" else v[-kw["max_gap"]:]
        assert not edge[0 if claim[1] == "start" else -1] and 0 < np.count_nonzero(~edge) <= kw["max_gap"]
        assert len(out) == 1
        same_start, same_end = np.array_equal(_bits(out[0, :2]), _bits(segs[0, :2])), np.array_equal(_bits(out[0, 2:]), _bits(segs[0, 2:]))
        assert (same_start, same_end) == ((False, True) if claim[1] == "start" else (True, False))
    elif kind == "tie":
        n, v = _valid(case, 0)
        rr = sm.runs(v)
        longest = max(b - a for a, b in rr)
        tied = [r for r in rr if r[1] - r[0] == longest]
        assert len(tied) >= 2 and len(out) == 1
        _, px, py, _, _ = sm.samples(segs[0])
        a, b = tied[0]
        assert np.array_equal(_bits(out[0]), _bits(np.array([px[a], py[a], px[b], py[b]]).astype(np.float32)))
    elif kind == "min_length":
        n, v = _valid(case, 0)
        _, _, _, dx, dy = sm.samples(segs[0])
        a, b = max(sm.runs(v), key=lambda r: r[1] - r[0])
        s = np.float64(b - a) / np.float64(n)
        lhs, rhs = (s * s) * (dx * dx + dy * dy), np.float64(kw["min_length"]) ** 2
        if claim[1]:
            assert b - a == 8 and lhs == rhs and len(out) == 1
        else:
            assert b - a == 7 and lhs < rhs and len(out) == 0
    elif kind == "all_valid":
        assert case["mask"].min() == 255 and np.array_equal(_bits(out), _bits(segs)) and src.tolist() == list(range(len(segs)))
    elif kind == "all_invalid":
        assert case["mask"].max() == 0 and len(out) == 0 and len(src) == 0
    elif kind == "threshold":
        others = {t: sc.model_of(sc.BY_NAME["threshold_%d" % t])[0] for t in (0, 1, 128, 255)}
        assert np.array_equal(_bits(others[0]), _bits(others[1]))
        assert len({_bits(others[t]).tobytes() for t in (1, 128, 255)}) == 3
        n, v = _valid(case, 0)
        first = int(np.flatnonzero(v)[0])
        assert case["mask"][7, first] >= max(1, claim[1]) and (first == 0 or case["mask"][7, first - 1] < max(1, claim[1]))
    elif kind == "permille":
        assert src.tolist() == ([0, 1] if claim[1] == "all" else [0])
        if claim[1] == "all":
            assert kw["keep_permille"] == 0 and not any(_valid(case, i)[1].any() for i in range(2))
        else:
            assert kw["keep_permille"] == 1000 and _valid(case, 0)[1].all() and np.count_nonzero(~_valid(case, 1)[1]) == 1
    elif kind == "permille_tie":
        n, v = _valid(case, 0)
        diff = int(np.count_nonzero(v)) * 1000 - kw["keep_permille"] * (n + 1)
        if claim[1] == 0:
            assert diff == 0 and len(out) == 1
        else:
            assert diff in (-1000, -(n + 1)) and len(out) == 0
    elif kind == "always_dropped":
        kept = list(claim[1])
        assert [i for i in range(len(segs)) if sm.samples(segs[i]) is not None] == kept and sorted(set(src.tolist())) == kept
        assert np.isnan(segs).any() and np.isinf(segs).any() and (segs[:, :2] == segs[:, 2:]).all(1).any() and (np.abs(segs[:, 2:] - segs[:, :2]) >= 65536).any()
    elif kind == "grows":
        assert len(out) > len(segs) and kw["mode"] == sm.SPLIT
    elif kind == "count":
        assert len(segs) == claim[1]
        if claim[1] > 100:
            assert 0 < len(set(src.tolist())) < len(segs)             # some are dropped whole, some survive
            if kw["mode"] == sm.SPLIT:
                assert len(set(src.tolist())) < len(src)             # and some are split
    elif kind == "stride":
        assert case["mask"].strides[0] > case["mask"].shape[1] and 0 < len(out)
    elif kind == "lens":
        L = case["lens"]
        assert lm.is_active(L["out_cam"], L["model"], L["src_cam"], L["coeffs"]) and case["mask"].shape != (48, 64)
        plain = sm.filter_segments(segs, case["mask"], lens=None, **kw)
        assert not np.array_equal(_bits(plain[0]), _bits(out)) or not np.array_equal(plain[1], src)        # the lens matters
        assert 0 < len(out)
    elif kind == "lens_inactive":
        L = case["lens"]
        assert not lm.is_active(L["out_cam"], L["model"], L["src_cam"], L["coeffs"])
        plain = sm.filter_segments(segs, case["mask"], lens=None, **kw)
        assert np.array_equal(_bits(plain[0]), _bits(out)) and np.array_equal(plain[1], src) and len(out)
    else:
        raise AssertionError("no check for claim %r" % (kind,))


@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES if c["claim"][0] == "lens"])
def test_lens_cases_keep_their_samples_off_the_pixel_edges(name):
    """atan is the one operation whose bits a device does not share with a host libm: no sample's u + 0.5 or v + 0.5 may lie within 1e-6 of an integer"""
    case = sc.BY_NAME[name]
    for seg in case["segments"]:
        smp = sm.samples(seg)
        if smp is None:
            continue
        u, v = sm.mask_positions(smp[1], smp[2], case["lens"])
        for w in (u, v):
            w = w[np.isfinite(w)] + 0.5
            assert np.all(np.abs(w - np.rint(w)) > 1e-6), name


def test_the_models_lens_is_lens_models_on_the_pixel_grid():
    for case in (c for c in sc.CASES if c["claim"][0] == "lens" and c["kw"]["mode"] == sm.DROP):
        L = case["lens"]
        u, v = lm.source_coordinates(64, 48, L["out_cam"], L["model"], L["src_cam"], L["coeffs"])
        j, i = np.meshgrid(np.arange(64, dtype=np.float64), np.arange(48, dtype=np.float64))
        u2, v2 = sm.lens_point(j, i, L["out_cam"], L["model"], L["src_cam"], L["coeffs"])
        assert np.array_equal(u.view(np.uint64), u2.view(np.uint64)) and np.array_equal(v.view(np.uint64), v2.view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model_bit_for_bit(name):
    case = sc.BY_NAME[name]
    segs, src = _host(case)
    want, wsrc = sc.model_of(case)
    assert segs.dtype == np.float32 and src.dtype == np.int32
    assert np.array_equal(src, wsrc), name
    assert np.array_equal(_bits(segs), _bits(want)), name


def test_refusals_come_with_their_code_and_cause():
    from line3d_amd import capi
    segs = np.array([[1.0, 1.0, 9.0, 6.0]], np.float32)
    mask = np.full((12, 16), 255, np.uint8)

    def refused(m, cause, s=segs):
        with pytest.raises(capi.L3DError) as e:
            capi.mask_segments_host(s, m)
        assert e.value.code == 1 and cause in str(e.value), str(e.value)

    refused(None, "mask is null")
    m = capi.segment_mask(mask)
    m.mask = None
    refused(m, "mask is null")
    for w, h in ((0, 12), (16, 0), (-1, 12)):
        m = capi.segment_mask(mask)
        m.mask_width, m.mask_height = w, h
        refused(m, "extent")
    m = capi.segment_mask(mask)
    m.mask_row_stride = 15
    refused(m, "row stride")
    for mode in (-1, 3):
        refused(capi.segment_mask(mask, mode=mode), "mode")
    for thr in (-1, 256):
        refused(capi.segment_mask(mask, threshold=thr), "threshold")
    for kp in (-1, 1001):
        refused(capi.segment_mask(mask, keep_permille=kp), "keep_permille")
    refused(capi.segment_mask(mask, mode="clip", max_gap=-1), "max_gap")
    for ml in (-0.5, float("nan"), float("inf")):
        refused(capi.segment_mask(mask, mode="split", min_length=ml), "min_length")
    # the lens: A LENS's checks and causes
    cam = (20.0, 20.0, 8.0, 6.0)
    refused(capi.segment_mask(mask, lens=capi.lens(3, [0.1], camera=cam), camera=cam), "unknown model")
    refused(capi.segment_mask(mask, lens=capi.lens("brown", [float("nan")], camera=cam), camera=cam), "not finite")
    refused(capi.segment_mask(mask, lens=capi.lens("fisheye", [0, 0, 0, 0, 0.1], camera=cam), camera=cam), "k[4..7]")
    refused(capi.segment_mask(mask, lens=capi.lens("brown", [0.1], camera=(20.0, 0.0, 8.0, 6.0)), camera=cam), "exactly one")
    refused(capi.segment_mask(mask, lens=capi.lens("brown", [0.1], camera=cam), camera=(0.0, 20.0, 8.0, 6.0)), "fx and fy")
    # the host entry point reads host memory
    m = capi.segment_mask(mask)
    m.mask_on_device = 1
    refused(m, "host memory")
    # a refusal hands nothing out; a good call after it works, and no segments give none
    out, src = capi.mask_segments_host(segs, capi.segment_mask(mask))
    assert np.array_equal(_bits(out), _bits(segs)) and src.tolist() == [0]
    out, src = capi.mask_segments_host(segs[:0], capi.segment_mask(mask))
    assert out.shape == (0, 4) and src.shape == (0,)
    with pytest.raises(TypeError):
        capi.mask_segments_host(segs, capi.segment_mask(mask), mode="clip")
    out, src = capi.mask_segments_host(segs, mask, mode="clip")
    assert src.tolist() == [0]


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/segmask_asan.cpp: l3d_segmask.hpp -- the argument checks, the samples, the run search, the host's wave -- and a main of its own, built
    with AddressSanitizer and UBSan as a plain host program, over masks of every extent from 1 x 1, segments through, beside and far outside them,
    every mode, gaps and thresholds, with and without lenses, and the refusals"""
    exe = str(tmp_path / "segmask_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "segmask_asan.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 bad" in run.stdout, run.stdout + run.stderr


def test_facade_compiles(tmp_path):
    """SegmentMask and Line3D::addImageMasked of include/line3D_amd.hpp, for world point ids and for view similarities"""
    src = tmp_path / "facade_segmask.cpp"
    src.write_text('''#include "line3D_amd.hpp"
int use(L3D::Line3D& l, const std::vector<L3D::float4>& segs, const unsigned char* mask, const double* K, const double* R, const double* t)
{
    std::list<unsigned int> wps;
    std::map<unsigned int, float> sims;
    l3d_lens lens = l3d_lens();
    L3D::SegmentMask a(mask, 64, 48);
    L3D::SegmentMask b(mask, 96, 64, 128);
    b.withLens(lens, 50.0, 50.0, 32.0, 24.0).threshold(128).split(4.0, 2).onDevice(false);
    a.clip(2.0).drop(750);
    const bool x = l.addImageMasked(0, 64, 48, segs, K, R, t, wps, a);
    const bool y = l.addImageMasked(1, 64, 48, segs, K, R, t, sims, b);
    return (x ? 1 : 0) + (y ? 2 : 0) + (b.get()->lens ? 4 : 0);
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
