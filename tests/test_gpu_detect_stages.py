"""The stages of the device line segment detector (l3d_detect.hip), each on its own through the l3d_test_detect_* entry points (the same
kernels and launch shapes as l3d_detect_segments), against the float64 model (tests/detect_model.py) and the reference detector's own
numbers (tests/golden/detect_stages.npz, made by tests/golden/make_golden_detect_stages.py).

  A  pixel stage: grey exact; the sampled image within 4e-12 (values <= 255, two passes of 7 products and 6 sums: 26 roundings of at most
     255 x 2^-53 < 8e-13, the weights' exp < 1e-12, doubled); modulus and angle within 2e-11; definedness and buckets equal wherever the
     model's margin exceeds 1e-9.  Every call follows a call on a larger, different image: a skipped write shows as stale data.
  B  labelling and vote: exact against scipy's connected components.
  C  regions: the rectangle from the moments (centre, angle, end points, width, density) within 1e-9 of the model and of the reference's
     region2rect on regions the reference grew; the pixels kept at every radius of the shrink; the rectangle search (counts, value,
     probability, width, end points, acceptance) equal to the model's and to the reference's rect_improve / rectangle iterator on shaped
     regions that are accepted at the first score, after each of the five retry stages, or never (no pixel centre on a border of any
     rectangle visited); on the grown regions, whose extreme pixels lie ON the end sides, under model.search_rule; the release of
     everything a region did not consume.
  E  the whole detector against model.detect on three scenes whose every decision is clearer than 1e-6: count, order, end points 1e-4.
  D  NFA: within 2 E + 1e-9 of the exact binomial tail, E = the reference's own largest error on the table (0.2217 when the fixture was
     made; the device's largest error measured on an MI355X: 0.3054, printed by the test)."""
import os

import numpy as np
import pytest

import detect_metric as dm
import detect_model as model
import detect_stage_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_stages.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ---------------------------------------------------------------------------------------------------------------- A
def _padded(img):
    """the same pixels in a buffer whose rows are 13 bytes longer"""
    if img.ndim == 2:
        buf = np.full((img.shape[0], img.shape[1] + 13), 201, np.uint8)
    else:
        buf = np.full((img.shape[0], img.shape[1] + 5, img.shape[2]), 201, np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


@pytest.mark.parametrize("name", list(cases.PIXEL_NOISE) + list(cases.PIXEL_FIXED))
def test_pixel_stage(gpu_ctx, golden, name):
    img = golden["px_" + name]
    new_size = cases.PIXEL_NOISE[name][3] if name in cases.PIXEL_NOISE else None
    want = model.pixel_stage(img, new_size)
    gpu_ctx.test_detect_pixel_stage(cases.primer_image(len(name)))              # leaves other data in every buffer
    got = gpu_ctx.test_detect_pixel_stage(_padded(img) if new_size else img, new_size)
    M, N = want["img"].shape
    assert got["img"].shape == (M, N)
    assert np.array_equal(got["grey"], want["grey"])
    for ref_img, what in ((want["img"], "model"), (golden["ref_img_" + name], "reference")):
        err = np.abs(got["img"] - ref_img).max()
        print("%s: sampled image against the %s: %.3g" % (name, what, err))
        assert err <= 4e-12, (what, err)
    for ref_mod, ref_ang, what in ((want["mod"], want["ang"], "model"), (golden["ref_mod_" + name], golden["ref_ang_" + name], "reference")):
        assert np.abs(got["mod"] - ref_mod).max() <= 2e-11, what
        both = (got["ang"] != model.NOTDEF) & (ref_ang != model.NOTDEF)
        assert np.abs(got["ang"] - ref_ang)[both].max(initial=0.0) <= 2e-11, what
    assert np.all(got["mod"][-1, :] == 0) and np.all(got["mod"][:, -1] == 0)
    assert np.all(got["ang"][-1, :] == model.NOTDEF) and np.all(got["ang"][:, -1] == model.NOTDEF)
    # decisions: equal outside the margins; inside, either neighbouring value
    sure = want["margin_rho"] > cases.MARGIN
    defined = got["ang"] != model.NOTDEF
    assert np.array_equal(defined[sure], (want["ang"] != model.NOTDEF)[sure])
    assert np.array_equal(got["bucket"][~defined], np.full((int((~defined).sum()), 2), 255, np.uint8))
    for p in range(2):
        clear = sure & (want["margin_bucket"][..., p] > cases.MARGIN)
        assert np.array_equal(got["bucket"][..., p][clear], want["bucket"][..., p][clear]), "partition %d" % p
        near = sure & ~clear & defined
        step = (got["bucket"][..., p].astype(np.int64) - want["bucket"][..., p].astype(np.int64)) % 8
        assert np.all(np.isin(step[near], (0, 1, 7)))
        if name in cases.PIXEL_NOISE or name == "const255" or p == 1:
            assert clear.all(), "a pixel of %s sits inside a margin" % name
    if name == "const255":
        assert np.abs(got["img"] - 255.0).max() <= 4e-12 and not defined.any()


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("shape", cases.LABEL_SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_labelling_and_vote(gpu_ctx, shape):
    M, N = shape
    for name, bucket, active in cases.label_cases(M, N):
        want_parent, _, want_key = model.label(bucket, active)
        parent, key = gpu_ctx.test_detect_label(bucket, active)
        assert np.array_equal(parent, want_parent), name
        assert np.array_equal(key, want_key), name
        again = gpu_ctx.test_detect_label(bucket, active)
        assert again[0].tobytes() == parent.tobytes() and again[1].tobytes() == key.tobytes(), name


# ---------------------------------------------------------------------------------------------------------------- C
def _bars(N=96, M=80):
    """Straight bars of given pixel counts on an empty field: level-line angle along the bar with a small seeded jitter, modulus seeded.
    -> (mod, ang, key, list of (key, pixels))"""
    rng = np.random.default_rng(77)
    np_ = N * M
    mod = np.zeros((M, N))
    ang = np.full((M, N), model.NOTDEF)
    key = np.full((M, N), 2 * np_, np.uint32)
    min_reg = model.min_region(N, M)
    regions = []

    def put(ys, xs, angle, partition):
        yy, xx = np.meshgrid(ys, xs, indexing="ij")
        px = np.sort((yy * N + xx).ravel())
        k = partition * np_ + int(px[0])
        key.ravel()[px] = k
        mod.ravel()[px] = rng.uniform(6.0, 20.0, len(px))
        ang.ravel()[px] = angle + rng.uniform(-0.05, 0.05, len(px))
        regions.append((k, px))

    m0, a0, _, px0 = cases.min_reg_bar(N, M)                        # exactly min_reg, no pixel centre on its rectangle's border
    key.ravel()[px0], mod.ravel()[px0], ang.ravel()[px0] = int(px0[0]), m0.ravel()[px0], a0.ravel()[px0]
    regions.append((int(px0[0]), px0))
    put([3], range(2, 2 + min_reg - 1), 0.0, 0)                     # one fewer: no record
    for row, n in ((5, 63), (7, 64), (9, 65)):
        put([row], range(1, 1 + n), 0.0, row % 2)
    put(range(12, 52), range(10, 85), 0.0, 1)                       # 3000 pixels
    put(range(56, 79), [0, 1], np.pi / 2, 0)                        # upright, along the left edge
    put([M - 1], range(N - 30, N), np.pi, 1)                        # the bottom right corner, angle turned by pi
    # an L: two arms of one region; density far under 0.7, so it shrinks about its strongest pixel.  Two pixels tie for the strongest, one
    # on each arm: the smaller index (on the horizontal arm) is the seed, and the pixels kept at each radius tell which one was taken
    arm = np.concatenate([(54 * N + np.arange(30, 70)), (np.arange(55, 78) * N + 30)])
    k = int(arm.min())
    key.ravel()[arm] = k
    mod.ravel()[arm] = rng.uniform(6.0, 20.0, len(arm))
    ang.ravel()[arm] = np.where(arm // N == 54, 0.0, np.pi / 2) + rng.uniform(-0.05, 0.05, len(arm))
    mod.ravel()[[54 * N + 60, 70 * N + 30]] = 30.0
    regions.append((k, np.sort(arm)))
    k_tie = k
    # a second L with the strongest pixel at its corner: every radius keeps both arms, the density never reaches 0.7, and the region
    # shrinks step by step until fewer than min_reg pixels are left: no score, all its pixels stay active
    arm = np.concatenate([(56 * N + np.arange(74, 95)), (np.arange(57, 78) * N + 74)])
    k = int(arm.min())
    key.ravel()[arm] = k
    mod.ravel()[arm] = rng.uniform(6.0, 20.0, len(arm))
    ang.ravel()[arm] = np.where(arm // N == 56, 0.0, np.pi / 2) + rng.uniform(-0.05, 0.05, len(arm))
    mod.ravel()[56 * N + 75] = 30.0
    regions.append((k, np.sort(arm)))
    return mod, ang, key, sorted(regions, key=lambda t: t[0]), min_reg, k_tie


def _same_angle(a, b, tol=1e-9):
    d = (a - b) % (2 * np.pi)
    return min(d, 2 * np.pi - d) <= tol


def _check_record(got, w, k):
    """one device record against the model's record of the same region (model.region with the device's first-term rule)"""
    assert (got["steps"], got["n_used"]) == (w["steps"], w["n_used"]), k
    want_hist = dict((step, n) for step, n, _ in w["history"])
    want_hist[w["steps"]] = w["n_used"]
    assert got["hist_n"].tolist() == [want_hist.get(step, 0) for step in range(8)], k          # the pixels kept at every radius
    if "rect" not in w:
        assert not got["scored"] and not got["accepted"], k
        return None
    r = w["rect"]                               # (of the last radius at which the region still had min_reg pixels)
    assert got["minpix"] == w["minpix"], k
    for f in ("cx", "cy", "x1", "y1", "x2", "y2", "width", "density"):
        assert abs(got[f] - r[f]) <= 1e-9, (k, f, got[f], r[f])
    assert _same_angle(got["theta"], r["theta"]), k
    assert w["margins"]["density"] > cases.MARGIN and w["margins"]["radius"] > cases.MARGIN and w["margins"]["flip"] > cases.MARGIN, k
    assert bool(got["scored"]) == w["scored"], k
    if not w["scored"]:
        assert not got["accepted"], k
        return None
    how = model.search_rule(w)
    if how == "exact":                          # the whole rectangle search: counts, value, the stage that accepted, the rectangle it left
        f = w["final"]
        assert (got["pts"], got["alg"], bool(got["accepted"])) == (w["pts"], w["alg"], w["accepted"]), (k, got, w["pts"], w["alg"], w["nfa"])
        assert got["p"] == f["p"] and abs(got["fwidth"] - f["width"]) <= 1e-9, k
        for a, b in (("fx1", "x1"), ("fy1", "y1"), ("fx2", "x2"), ("fy2", "y2")):
            assert abs(got[a] - f[b]) <= 1e-9, (k, a)
        assert abs(got["nfa"] - w["nfa"]) <= 1e-8 * max(1.0, abs(w["nfa"])), (k, got["nfa"], w["nfa"])
    elif how == "first":                        # pixels on the border, but accepted at the first score whichever way they fall
        plo, phi, alo, ahi = w["first_counts"]
        assert got["accepted"] and got["p"] == model.P0 and abs(got["fwidth"] - r["width"]) <= 1e-9, k
        assert plo <= got["pts"] <= phi and alo <= got["alg"] <= ahi, (k, got["pts"], got["alg"], w["first_counts"])
        assert w["first_lo"] - 1e-8 * abs(w["first_lo"]) <= got["nfa"] <= w["first_hi"] + 1e-8 * abs(w["first_hi"]), k
        for a, b in (("fx1", "x1"), ("fy1", "y1"), ("fx2", "x2"), ("fy2", "y2")):
            assert abs(got[a] - r[b]) <= 1e-9, (k, a)
    return how


def _run_regions(gpu_ctx, mod, ang, key, regions):
    """the region stage on a labelling, every record and the active map against the model -> (records, model records, rules)"""
    M, N = mod.shape
    min_reg, logNT = model.min_region(N, M), model.log_nt(N, M)
    rec, active = gpu_ctx.test_detect_regions(mod, ang, key, min_reg)
    want = [(k, model.region(mod, ang, px, min_reg, logNT, model.DEVICE_ZERO)) for k, px in sorted(regions, key=lambda t: t[0])]
    want = [(k, w) for k, w in want if w is not None]
    assert len(rec) == len(want)
    again, active2 = gpu_ctx.test_detect_regions(mod, ang, key, min_reg)
    assert again.tobytes() == rec.tobytes() and active2.tobytes() == active.tobytes()
    expect_active = np.ones(M * N, np.uint8)
    rules = []
    for got, (k, w) in zip(rec, want):
        rules.append(_check_record(got, w, k))
        if w["accepted"] and rules[-1]:
            expect_active[w["used"]] = 0        # consumed: the pixels used go inactive; shed pixels, failed and small regions, the field stay
        elif w["scored"] and rules[-1] is None and got["accepted"]:
            expect_active[w["used"]] = 0        # (a region the rule leaves open: the map follows the device's decision)
    assert np.array_equal(active.ravel(), expect_active)
    return rec, [w for _, w in want], rules


def test_regions_against_the_model(gpu_ctx):
    mod, ang, key, regions, min_reg, k_tie = _bars()
    # the tie: were the larger index taken as the seed, the L would keep other pixels as it shrinks (the model with that pixel raised)
    px = dict(regions)[k_tie]
    tied = px[mod.ravel()[px] == mod.ravel()[px].max()]
    assert len(tied) == 2
    other = mod.copy()
    other.ravel()[tied[1]] += 1.0
    logNT = model.log_nt(mod.shape[1], mod.shape[0])
    mine, theirs = (model.region(m, ang, px, min_reg, logNT, model.DEVICE_ZERO) for m in (mod, other))
    assert (mine["seed"], theirs["seed"]) == (tied[0], tied[1]) and mine["steps"] >= 1
    assert [n for _, n, _ in mine["history"]][1:] != [n for _, n, _ in theirs["history"]][1:] and mine["n_used"] != theirs["n_used"]
    rec, want, rules = _run_regions(gpu_ctx, mod, ang, key, regions)
    assert len(rec) == len(regions) - 1                                 # the region of min_reg - 1 pixels yields none
    assert want[0]["n_used"] == min_reg and want[0]["steps"] == 0 and rules[0] == "exact"      # the region of exactly min_reg pixels
    assert sum(w["steps"] > 0 for w in want) >= 1, "no region of the scene shrinks"
    assert sum(len(w["history"]) >= 3 for w in want) >= 1, "no region is measured at three radii"
    assert [i for i, (h, w) in enumerate(zip(rules, want)) if w["scored"] and h is None] == []      # the rule leaves no region's search open
    assert sum(w["steps"] >= 3 and not w["scored"] for w in want) == 1, "the second L does not shrink to nothing"
    assert sum(w["accepted"] for w in want) >= 6 and rec["accepted"].sum() == sum(w["accepted"] for w in want)


def _check_search_against_reference(got, row):
    cases.check_search_against_row(got["pts"], got["alg"], got["accepted"], got["p"], got["fwidth"], (got["fx1"], got["fy1"], got["fx2"], got["fy2"]), row)


@pytest.mark.parametrize("band", range(len(cases.band_list())), ids=lambda i: "%s, seed %d" % cases.band_list()[i])
def test_rectangle_search_on_a_shaped_region(gpu_ctx, golden, band):
    """regions whose rectangles keep every pixel centre off their borders: accepted at the first score, rejected there and accepted after
    each of the five retry stages, failing every stage (the pixels stay active).  The whole search -- counts, acceptance, the final
    probability, width and end points -- against the model and against the reference's rect_improve and rectangle iterator"""
    kind, seed = cases.band_list()[band]
    mod, ang, key, px = cases.tilted_band(seed)
    rec, want, rules = _run_regions(gpu_ctx, mod, ang, key, [(int(px[0]), px)])
    assert cases.band_kind(want[0]) == kind and rules == ["exact"]
    assert bool(rec[0]["accepted"]) == (kind != "fails every stage")
    assert len(golden["band_rows"]) == len(cases.band_list()) + 1 >= cases.BANDS_AT_LEAST
    _check_search_against_reference(rec[0], golden["band_rows"][band])


def test_rectangle_search_on_a_region_of_exactly_min_reg_pixels(gpu_ctx, golden):
    mod, ang, key, px = cases.min_reg_bar()
    rec, want, rules = _run_regions(gpu_ctx, mod, ang, key, [(int(px[0]), px)])
    assert rules == ["exact"] and rec[0]["n_used"] == model.min_region(mod.shape[1], mod.shape[0])
    _check_search_against_reference(rec[0], golden["band_rows"][-1])


def test_region_clipped_at_all_four_image_sides(gpu_ctx):
    mod, ang, key, px = cases.corner_band()
    M, N = mod.shape
    assert px[0] == 0 and px[-1] == M * N - 1
    rec, want, rules = _run_regions(gpu_ctx, mod, ang, key, [(0, px)])
    assert rules == ["first"] and rec[0]["accepted"]


def test_density_exactly_at_the_threshold_is_scored(gpu_ctx):
    mod, ang, key, px = cases.density_exactly_at_the_threshold()
    M, N = mod.shape
    w = model.region(mod, ang, px, model.min_region(N, M), model.log_nt(N, M), model.DEVICE_ZERO)
    assert w["rect"]["density"] == model.DENSITY_TH and w["scored"] and w["steps"] == 0
    rec, _ = gpu_ctx.test_detect_regions(mod, ang, key, model.min_region(N, M))
    assert len(rec) == 1 and rec[0]["density"] == model.DENSITY_TH and rec[0]["scored"] and rec[0]["steps"] == 0 and rec[0]["n_used"] == 14


@pytest.mark.parametrize("name", cases.REGION_SCENES)
def test_regions_grown_by_the_reference(gpu_ctx, golden, name):
    """the reference's own regions (region_grow in its seed order), fed with its own modulus and angles: the rectangle against region2rect,
    the search against rect_improve and the rectangle iterator's counts, and both against the model"""
    label, rows, mod, ang = golden["rg_label_" + name], golden["rg_rows_" + name], golden["rg_mod_" + name], golden["rg_ang_" + name]
    M, N = label.shape
    flat = label.ravel().astype(np.int64)
    regions = [(int(np.flatnonzero(flat == i + 1)[0]), np.flatnonzero(flat == i + 1)) for i in range(len(rows))]
    key = np.full(M * N, 2 * M * N, np.uint32)
    for k, px in regions:
        key[px] = k
    rec, want, rules = _run_regions(gpu_ctx, mod, ang, key.reshape(M, N), regions)
    assert len(want) == len(rows)
    for got, how, i in zip(rec, rules, sorted(range(len(rows)), key=lambda i: regions[i][0])):
        row = rows[i]
        if abs(row[10] - model.DENSITY_TH) <= cases.MARGIN or got["steps"] != 0:
            continue                            # (a region the device shrinks is held to the model above; region2rect saw the whole region)
        assert got["n_used"] == int(row[0])
        for f, v in zip(("cx", "cy", "x1", "y1", "x2", "y2", "width", "density"), (row[2], row[3], row[5], row[6], row[7], row[8], row[9], row[10])):
            assert abs(got[f] - v) <= 1e-9, (f, got[f], v)
        assert _same_angle(got["theta"], row[4])
        assert bool(got["scored"]) == bool(row[11])
        if how == "exact":                      # (none on these scenes: the end sides of a grown region's rectangle pass through its extreme
            _check_search_against_reference(got, row)                       # pixels.  The shaped regions above take this comparison)
        elif how == "first":
            assert got["accepted"] and row[12] > 0 and got["p"] == row[18] and abs(got["fwidth"] - row[17]) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("name", list(cases.COMPOSITION))
def test_composition_against_the_model(gpu_ctx, golden, name):
    """the whole detector against model.detect: three rounds with release, heads and starts in production, the selection.  The scenes were
    drawn (seeds in the fixture) so that every decision of the model's run is clearer than 1e-6."""
    img = golden["cmp_img_" + name]
    want, margins = model.detect(img, zero=model.DEVICE_ZERO)
    assert margins["undecided"] == 0 and min(v for k, v in margins.items() if k != "undecided") > cases.COMPOSITION_MARGIN
    got = gpu_ctx.detect_segments(img)
    print("%s: %d segments (model %d)" % (name, len(got), len(want)))
    assert len(got) == len(want) and len(want) >= 2
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-4          # same order, end points within 1e-4 px
    capped = gpu_ctx.detect_segments(img, max_segments=2)
    assert np.array_equal(capped, got[:2])


# ---------------------------------------------------------------------------------------------------------------- D
def test_nfa_against_the_exact_tail(gpu_ctx, golden):
    n, k, p = cases.nfa_table()
    exact, ref = golden["nfa_exact"], golden["nfa_ref"]
    assert len(exact) == len(n) == len(ref)
    E = float(np.abs(ref - exact).max())
    got = gpu_ctx.test_detect_nfa(n, k, p, cases.NFA_LOGNT)
    err = np.abs(got - exact)
    i = int(err.argmax())
    print("NFA table, %d rows: reference's largest error E = %.6g; device's largest error %.6g at n=%d k=%d p=1/%d (bound %.6g)"
          % (len(n), E, err[i], n[i], k[i], round(1 / p[i]), 2 * E + 1e-9))
    assert np.all(np.isfinite(got))
    assert err.max() <= 2 * E + 1e-9, (n[i], k[i], p[i], got[i], exact[i])
    clear = np.abs(exact) > E
    assert np.array_equal(np.sign(got[clear]), np.sign(exact[clear]))
