"""CPU side of the line segment detector's checks: the agreement measure on the committed reference results
(tests/golden/detect_ref.npz), the stored floor, which facade overload an image type selects, and the float64 model of the detector's
stages (tests/detect_model.py) against the reference's own numbers (tests/golden/detect_stages.npz) under the comparisons of
tests/test_gpu_detect_stages.py: the reference and the model stay inside every tolerance on their own."""
import os
import subprocess

import numpy as np
import pytest

import detect_metric as dm
import detect_model as model
import detect_stage_cases as cases

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


# ---- the stage model against the reference's stage outputs (the same comparisons as tests/test_gpu_detect_stages.py)
@pytest.fixture(scope="module")
def stages():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "detect_stages.npz")))


@pytest.mark.parametrize("name", list(cases.PIXEL_NOISE) + list(cases.PIXEL_FIXED))
def test_model_pixel_stage_against_the_reference(stages, name):
    img = stages["px_" + name]
    new_size = cases.PIXEL_NOISE[name][3] if name in cases.PIXEL_NOISE else None
    if name in cases.PIXEL_NOISE:
        w, h, ch, _ = cases.PIXEL_NOISE[name]
        assert np.array_equal(img, cases.noise_image(int(stages["seed_" + name]), w, h, ch))
    else:
        assert np.array_equal(img, cases.fixed_image(name))
    ps = model.pixel_stage(img, new_size)
    ref_img, ref_mod, ref_ang = stages["ref_img_" + name], stages["ref_mod_" + name], stages["ref_ang_" + name]
    assert ps["img"].shape == ref_img.shape == tuple(reversed(model.scaled_size(*(new_size or (img.shape[1], img.shape[0])))))
    assert np.abs(ps["img"] - ref_img).max() <= 4e-12
    assert np.abs(ps["mod"] - ref_mod).max() <= 2e-11
    both = (ps["ang"] != model.NOTDEF) & (ref_ang != model.NOTDEF)
    assert np.abs(ps["ang"] - ref_ang)[both].max(initial=0.0) <= 2e-11
    sure = ps["margin_rho"] > cases.MARGIN
    assert np.array_equal((ps["ang"] != model.NOTDEF)[sure], (ref_ang != model.NOTDEF)[sure])
    ref_bucket, _ = model.buckets(ref_ang)
    for p in range(2):
        clear = sure & (ps["margin_bucket"][..., p] > cases.MARGIN)
        assert np.array_equal(ps["bucket"][..., p][clear], ref_bucket[..., p][clear])
        if name != "checker" or p == 1:
            assert clear.all()                      # the condition on the share left out: nothing, but partition 0 of the checkerboard
    if name == "const255":
        assert np.abs(ps["img"] - 255.0).max() <= 4e-12 and not (ps["ang"] != model.NOTDEF).any()


def test_model_labelling_on_known_maps():
    for M, N in cases.LABEL_SIZES:
        got = {name: model.label(b, a) for name, b, a in cases.label_cases(M, N)}
        np_ = M * N
        parent, size, key = got["one bucket"]
        assert np.all(parent == 0) and np.all(size == np_) and np.all(key == 0)                       # tie: partition 0
        parent, size, key = got["all neighbours differ"]
        assert np.array_equal(parent[0].ravel(), np.arange(np_)) and np.all(size == 1)
        parent, size, key = got["partition 1 larger"]
        assert np.all(key == np_)
        parent, size, key = got["spiral, gaps inactive"]
        assert len(np.unique(parent[0][parent[0] >= 0])) == 1 and np.all(key[parent[0] < 0] == 2 * np_)      # one long arm
        parent, size, key = got["row ends do not join"]
        assert size.max() == 3
        parent, size, key = got["diagonals only"]
        assert size.max() >= min(M, N // 2) - 1 and size[0][parent[0] >= 0].min() >= 1


def test_model_nfa_against_the_exact_tail_and_the_reference(stages):
    n, k, p = cases.nfa_table()
    exact, ref = stages["nfa_exact"], stages["nfa_ref"]
    assert len(n) == len(exact) == len(ref) and len(n) > 300
    small = np.flatnonzero(n <= 1000)[::7]                     # the stored exact values are the model's: a sample is recomputed
    assert np.allclose([model.nfa_exact(n[i], k[i], p[i], cases.NFA_LOGNT) for i in small], exact[small], rtol=0, atol=1e-12)
    E = float(np.abs(ref - exact).max())
    print("reference's largest error on the table: E = %.6g" % E)
    assert 0.0 < E < 1.0
    for zero, what in ((model.FIRST_TERM_ZERO, "the reference's rule"), (100.0 * 2.2250738585072014e-308, "100 DBL_MIN (the device's)")):
        fl = np.array([model.nfa_float(a, b, c, cases.NFA_LOGNT, zero) for a, b, c in zip(n, k, p)])
        err = np.abs(fl - exact)
        print("the recipe with a first term counted as zero by %s: largest error %.6g" % (what, err.max()))
        assert err.max() <= 2 * E + 1e-9
        clear = np.abs(exact) > E
        assert np.array_equal(np.sign(fl[clear]), np.sign(exact[clear]))
        if zero == model.FIRST_TERM_ZERO:
            assert np.abs(fl - ref).max() <= 1e-9              # the recipe as the reference evaluates it
    window = [(a, b, c) for a, b, c in zip(n, k, p) if model.nfa_float(a, b, c, 0.0) != model.nfa_float(a, b, c, 0.0, 100.0 * 2.2250738585072014e-308)]
    assert len(window) >= 6                                    # the table reaches the window in which the two rules differ


@pytest.mark.parametrize("name", cases.REGION_SCENES)
def test_model_regions_against_the_reference(stages, name):
    """the regions region_grow formed: the model's rectangle against region2rect, its search against rect_improve and the iterator's counts"""
    label, rows, mod, ang = stages["rg_label_" + name], stages["rg_rows_" + name], stages["rg_mod_" + name], stages["rg_ang_" + name]
    M, N = label.shape
    ps = model.pixel_stage(stages["rg_img_" + name])
    assert np.abs(ps["mod"] - mod).max() <= 2e-11 and np.array_equal(ps["ang"] != model.NOTDEF, ang != model.NOTDEF)
    logNT, min_reg = model.log_nt(N, M), model.min_region(N, M)
    assert len(rows) >= 1 and np.all(rows[:, 0] >= min_reg)
    for i, row in enumerate(rows):
        px = np.flatnonzero(label.ravel() == i + 1)
        assert len(px) == int(row[0])
        r = model.rect_from_pixels(mod, ang, px)
        for f, v in zip(("reg_angle", "cx", "cy", "x1", "y1", "x2", "y2", "width", "density"), (row[1], row[2], row[3], row[5], row[6], row[7], row[8], row[9], row[10])):
            assert abs(r[f] - v) <= 1e-9, (i, f, r[f], v)
        d = (r["theta"] - row[4]) % (2 * np.pi)
        assert min(d, 2 * np.pi - d) <= 1e-9
        if abs(row[10] - model.DENSITY_TH) <= cases.MARGIN or not row[11]:
            continue
        w = model.region(mod, ang, px, min_reg, logNT)
        dev = model.region(mod, ang, px, min_reg, logNT, model.DEVICE_ZERO)         # the device's first-term rule changes no outcome here
        assert (w["pts"], w["alg"], w["accepted"], w["final"]["p"], w["final"]["width"]) == (dev["pts"], dev["alg"], dev["accepted"], dev["final"]["p"], dev["final"]["width"])
        how = model.search_rule(w)
        if how == "exact":
            assert (w["pts"], w["alg"], w["accepted"], w["final"]["p"]) == (int(row[19]), int(row[20]), row[12] > 0, row[18])
            assert abs(w["final"]["width"] - row[17]) <= 1e-9 and abs(w["nfa"] - row[12]) <= 1e-9 * max(1.0, abs(row[12]))
        elif how == "first":
            plo, phi, alo, ahi = w["first_counts"]
            assert row[12] > 0 and row[18] == model.P0 and abs(row[17] - row[9]) <= 1e-9
            assert plo <= row[19] <= phi and alo <= row[20] <= ahi
            assert w["first_lo"] - 1e-9 * abs(w["first_lo"]) <= row[12] <= w["first_hi"] + 1e-9 * abs(w["first_hi"])


def test_share_of_reference_regions_left_out(stages):
    """every scored region has a pixel centre on its rectangle's border (region2rect puts the end sides through the two extreme pixels), so
    the comparison is made under model.search_rule; that rule leaves out at most a tenth of the scored regions of the fixture"""
    total = literal = left_out = 0
    for name in cases.REGION_SCENES:
        label, rows, mod, ang = stages["rg_label_" + name], stages["rg_rows_" + name], stages["rg_mod_" + name], stages["rg_ang_" + name]
        M, N = label.shape
        for i, row in enumerate(rows):
            if row[11]:
                w = model.region(mod, ang, np.flatnonzero(label.ravel() == i + 1), model.min_region(N, M), model.log_nt(N, M))
                total += 1
                literal += w["margins"]["border"] <= model.BORDER
                left_out += model.search_rule(w) is None
    print("scored regions %d, with a pixel on a border %d, left out by the rule %d" % (total, literal, left_out))
    assert total >= 20 and left_out <= 0.1 * total


def test_model_rectangle_search_against_the_reference(stages):
    """shaped regions with no pixel centre on a border of any rectangle visited: the model's whole search against the reference's
    rect_improve and rectangle iterator, exactly; acceptance at the first score, after every retry stage, and never"""
    M, N = cases.BAND_SHAPE
    rows = stages["band_rows"]
    assert len(rows) == len(cases.band_list()) + 1
    exact, stage_seen = 0, set()
    for (kind, seed), row in zip(cases.band_list() + [("exactly min_reg", None)], rows):
        mod, ang, _, px = cases.tilted_band(seed) if seed is not None else cases.min_reg_bar()
        M, N = mod.shape
        assert len(px) == int(row[0])
        for zero in (model.FIRST_TERM_ZERO, model.DEVICE_ZERO):
            w = model.region(mod, ang, px, model.min_region(N, M), model.log_nt(N, M), zero)
            assert model.search_rule(w) == "exact" and w["steps"] == 0 and (seed is None or cases.band_kind(w) == kind), (kind, seed)
            r, f = w["rect"], w["final"]
            for name, v in zip(("reg_angle", "cx", "cy", "x1", "y1", "x2", "y2", "width", "density"), (row[1], row[2], row[3], row[5], row[6], row[7], row[8], row[9], row[10])):
                assert abs(r[name] - v) <= 1e-9, (kind, seed, name)
            cases.check_search_against_row(w["pts"], w["alg"], w["accepted"], f["p"], f["width"], (f["x1"], f["y1"], f["x2"], f["y2"]), row)
            assert abs(w["nfa"] - row[12]) <= 1e-9 * max(1.0, abs(row[12]))
        exact += 1
        stage_seen.add(w["stage"])
        if w["stage"] is None or w["stage"] >= 0:
            assert len(w["visited"]) > 5                        # the reference went through a whole retry stage at least
        if w["stage"] in (1, 2, 3):
            assert f["width"] < r["width"]
        if w["stage"] in (0, 4):
            assert f["p"] < model.P0
    assert exact >= cases.BANDS_AT_LEAST and stage_seen == {-1, 0, 1, 2, 3, 4, None}


def test_shaped_region_cases_on_the_model():
    mod, ang, _, px = cases.corner_band()
    w = model.region(mod, ang, px, model.min_region(30, 20), model.log_nt(30, 20), model.DEVICE_ZERO)
    assert model.search_rule(w) == "first" and w["steps"] == 0
    mod, ang, _, px = cases.density_exactly_at_the_threshold()
    w = model.region(mod, ang, px, model.min_region(40, 12), model.log_nt(40, 12), model.DEVICE_ZERO)
    assert w["rect"]["density"] == model.DENSITY_TH and w["rect"]["length"] == 20.0 and w["scored"] and w["steps"] == 0


@pytest.mark.parametrize("name", list(cases.COMPOSITION))
def test_composition_scenes_are_decided(stages, name):
    segs, margins = model.detect(stages["cmp_img_" + name], zero=model.DEVICE_ZERO)
    ref_rule, _ = model.detect(stages["cmp_img_" + name])
    assert len(segs) >= 2 and np.array_equal(segs, ref_rule)
    assert margins["undecided"] == 0 and min(v for k, v in margins.items() if k != "undecided") > cases.COMPOSITION_MARGIN, margins
