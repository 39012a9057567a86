"""The cases of the detector's stage tests, shared by the fixture generator (tests/golden/make_golden_detect_stages.py), the CPU
checks (tests/test_detect_cpu.py) and the GPU tests (tests/test_gpu_detect_stages.py): image lists, the NFA table, synthetic bucket maps and the margins under which a decision is compared."""
import math

import numpy as np

import detect_model as model

MARGIN = 1e-9               # threshold decisions of the pixel stage and the density are compared when the model's margin exceeds this

# ---- A: pixel stage.  name -> (width, height, channels, new_size)
PIXEL_NOISE = {
    "n8x8": (8, 8, 1, None),                    # N = M = 7, the minimum
    "n37x29": (37, 29, 1, None),                # small and odd
    "n80x20": (80, 20, 1, None),                # N = 64, M = 16: exactly one tile each way
    "n81x21": (81, 21, 1, None),                # N = 65, M = 17: a second block of one column / one row
    "n161x41": (161, 41, 1, None),              # N = 129, M = 33
    "rs50x38": (50, 38, 3, (41, 29)),           # a non-integer shrink
    "rs20x16": (20, 16, 3, (33, 27)),           # an enlargement: the last-sample clamp
    "rs64x48": (64, 48, 3, (32, 24)),
}
PIXEL_FIXED = ("const255", "checker")
PIXEL_SEED0 = 7100
PRIMER_SHAPE = (67, 211)                        # the larger, different image every pixel-stage call is preceded by


def noise_image(seed, w, h, ch):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)


def fixed_image(name):
    if name == "const255":
        return np.full((29, 37), 255, np.uint8)
    yy, xx = np.mgrid[0:29, 0:37]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


def primer_image(k):
    return noise_image(99000 + k, PRIMER_SHAPE[1], PRIMER_SHAPE[0], 1)


# ---- C: the scenes whose reference-grown regions the fixture stores; E: the composition scenes, name -> (width, height)
REGION_SEED0 = 4242
REGION_SCENES = ("tiny", "rects", "rects_noisy", "edge0", "edge7", "edge45", "edge90")
COMPOSITION = {"c37x29": (37, 29), "c96x80": (96, 80), "c161x41": (161, 41)}
COMPOSITION_SEED0 = 5100
COMPOSITION_MARGIN = 1e-6       # every decision of the model's whole run on a composition scene is clearer than this


# ---- D: the NFA table
NFA_LOGNT = 5.0 * (math.log10(512.0) + math.log10(384.0)) / 2.0 + math.log10(11.0)


def nfa_table():
    """n in {1, 2, 15, 16, 64, 1000, 20000} x p in {1/8 .. 1/256} x about 12 values of k (0, 1, n p rounded both ways, n - 1, n, an even
    spread); then first terms that underflow, and first terms between the reference's zero (4.9e-322) and 100 DBL_MIN"""
    rows = set()
    for n in (1, 2, 15, 16, 64, 1000, 20000):
        for e in range(3, 9):
            p = 1.0 / (1 << e)
            ks = {0, 1, int(math.floor(n * p)), int(math.ceil(n * p)), n - 1, n} | {int(round(t)) for t in np.linspace(0, n, 8)}
            for k in ks:
                if 0 <= k <= n:
                    rows.add((n, k, p))
    for n, k, p in ((20000, 15000, 1.0 / 8), (20000, 19999, 1.0 / 8), (20000, 10000, 1.0 / 256), (1000, 999, 1.0 / 256), (20000, 1, 1.0 / 256)):
        rows.add((n, k, p))
    lo, hi = math.log(model.FIRST_TERM_ZERO), math.log(100.0 * 2.2250738585072014e-308)
    for n in (1000, 20000):
        for e in (3, 5, 8):
            p = 1.0 / (1 << e)
            found = 0
            for k in range(int(n * p) + 1, n):
                log1 = (model._log_gamma(n + 1.0) - model._log_gamma(k + 1.0) - model._log_gamma(n - k + 1.0) + k * math.log(p) + (n - k) * math.log(1.0 - p))
                if lo + 1.0 < log1 < hi - 1.0:
                    rows.add((n, k, p))
                    found += 1
                    if found == 3:
                        break
                if log1 < lo:
                    break
    rows = sorted(rows)
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.float64))


# ---- B: synthetic bucket / active maps
LABEL_SIZES = ((80, 96), (7, 7), (5, 257))         # (M, N)


def _spiral(M, N):
    """a one-pixel-wide arm winding inwards: the even rings, each cut below its top-left corner and bridged to the next even ring"""
    yy, xx = np.mgrid[0:M, 0:N]
    ring = np.minimum(np.minimum(xx, yy), np.minimum(N - 1 - xx, M - 1 - yy))
    on = ring % 2 == 0
    for r in range(0, min(M, N) // 2, 2):
        if r + 1 < M - r - 1:
            on[r + 1, r] = False
        if r + 2 < M and r + 1 < N and ring[min(r + 2, M - 1), min(r + 2, N - 1)] == r + 2:
            on[r + 2, r + 1] = True
    return on


def _comb(M, N):
    on = np.zeros((M, N), bool)
    on[0::2, :] = True
    for y in range(1, M, 2):
        on[y, N - 1 if (y // 2) % 2 == 0 else 0] = True
    return on


def label_cases(M, N):
    """-> list of (name, bucket (M, N, 2) uint8, active (M, N) uint8)"""
    yy, xx = np.mgrid[0:M, 0:N]
    ones = np.ones((M, N), np.uint8)
    rng = np.random.default_rng(1000 * M + N)
    out = []

    def add(name, b0, b1, active=ones):
        out.append((name, np.stack([b0, b1], axis=-1).astype(np.uint8), np.asarray(active, np.uint8)))

    sp = _spiral(M, N)
    # partition 0: the spiral; partition 1: the same spiral transposed (square sizes) or turned by 180 degrees.  (The gaps between the arms
    # form a second long spiral in each partition.  Only 96x80 has a long chain, about 3800 pixels; 7x7 and 257x5 have two or three rings.)
    add("spiral", np.where(sp, 0, 1), np.where(sp.T if M == N else sp[::-1, ::-1], 2, 3))
    add("spiral, gaps inactive", np.zeros((M, N)), np.ones((M, N)), sp)
    cb = _comb(M, N)
    add("comb", np.where(cb, 4, 5), np.where(cb[::-1], 6, 7))
    diag = ((xx - yy) % 4 == 0) & (xx < N // 2) | ((xx + yy) % 4 == 0) & (xx >= N // 2)
    add("diagonals only", np.full((M, N), 2), np.full((M, N), 3), diag)
    wrap = np.zeros((M, N), bool)
    for y in range(0, M - 1, 2):
        wrap[y, max(0, N - 3):] = True
        wrap[y + 1, :min(3, N - 4)] = True
    add("row ends do not join", np.full((M, N), 3), np.full((M, N), 3), wrap)
    add("one bucket", np.full((M, N), 5), np.full((M, N), 6))
    four = (xx % 2) + 2 * (yy % 2)
    add("all neighbours differ", four, four + 4)
    add("partition 1 larger", four, np.full((M, N), 1))
    add("ties go to partition 0", np.where(cb, 4, 5), np.where(cb, 1, 2))
    holes = rng.random((M, N)) > 0.2
    add("inactive holes", rng.integers(0, 2, (M, N)), rng.integers(0, 2, (M, N)), holes)
    add("random 8", rng.integers(0, 8, (M, N)), rng.integers(0, 8, (M, N)))
    add("random 2", rng.integers(0, 2, (M, N)), rng.integers(0, 3, (M, N)))
    add("random 2 with holes", rng.integers(0, 2, (M, N)), rng.integers(0, 2, (M, N)), rng.random((M, N)) > 0.45)
    return out


# ---- C: shaped regions for the rectangle search.  A tilted band of pixels with a light spur beyond each end on one side: the spurs are
# the extreme pixels along the axis but lie outside the rectangle sideways, so no pixel centre sits on a border and the whole search
# (counts, values, the stage that accepts) can be compared exactly.  The seeds were found by search_band_seeds() on the CPU.
BAND_SHAPE = (48, 64)           # (M, N)
# kind (band_kind) -> seeds: acceptance at the first score, after each of the five retry stages (0 and 4 halve the precision, 1 cuts the
# width, 2 and 3 move one side in), and no acceptance
BAND_SEEDS = {"accepted at the first score": (8,), "accepted in stage 0": (3,), "accepted in stage 1": (41, 52), "accepted in stage 2": (31, 73),
              "accepted in stage 3": (41225,), "accepted in stage 4": (126,), "fails every stage": (57, 61)}
BANDS_AT_LEAST = 10             # so many regions are compared exactly with the reference's rect_improve (fixture rows 'band_rows')


def band_list():
    """-> [(kind, seed)] in the order of the fixture's band_rows"""
    return [(kind, seed) for kind, seeds in BAND_SEEDS.items() for seed in seeds]


def tilted_band(seed):
    """-> (mod, ang, key (M, N) uint32, pixels of the region)"""
    M, N = BAND_SHAPE
    rng = np.random.default_rng(seed)
    th, length, width = rng.uniform(0.15, 0.65), rng.uniform(14.0, 30.0), rng.uniform(1.2, 2.5)
    cx, cy = N / 2 + rng.uniform(-3, 3), M / 2 + rng.uniform(-3, 3)
    yy, xx = np.mgrid[0:M, 0:N]
    u = (xx - cx) * math.cos(th) + (yy - cy) * math.sin(th)
    v = -(xx - cx) * math.sin(th) + (yy - cy) * math.cos(th)
    light = v > width / 2 - 0.8
    region = (np.abs(u) <= length / 2) & (np.abs(v) <= width / 2) | (np.abs(u) > length / 2) & (np.abs(u) <= length / 2 + 1.5) & light & (v <= width / 2 + 0.5)
    px = np.flatnonzero(region.ravel())
    aligned = rng.random(len(px)) < rng.uniform(0.3, 1.0)
    spread = rng.choice([0.02, 0.1, 0.3])
    mod, ang = np.zeros((M, N)), np.full((M, N), model.NOTDEF)
    mod.ravel()[px] = np.where(light.ravel()[px], rng.uniform(3.0, 5.0, len(px)), rng.uniform(15.0, 30.0, len(px)))
    ang.ravel()[px] = th + np.where(aligned, rng.uniform(-spread, spread, len(px)), rng.uniform(0.6, 2.5, len(px)) * rng.choice([-1.0, 1.0], len(px)))
    key = np.full((M, N), 2 * M * N, np.uint32)
    key.ravel()[px] = px[0]
    return mod, ang, key, px


def band_kind(rec):
    """which of BAND_SEEDS' cases the model's record of a band is, or None"""
    if rec is None or not rec["scored"] or model.search_rule(rec) != "exact" or rec["steps"] != 0 or min(rec["margins"][k] for k in ("density", "flip")) <= MARGIN:
        return None
    if not rec["accepted"]:
        return "fails every stage"
    return "accepted at the first score" if rec["stage"] < 0 else "accepted in stage %d" % rec["stage"]


def search_band_seeds(limit=60000, each=2):
    """-> kind -> the first `each` seeds of that kind under both first-term rules (stages 3 and 4 are rare: one in tens of thousands)"""
    M, N = BAND_SHAPE
    found = {}
    for seed in range(limit):
        mod, ang, _, px = tilted_band(seed)
        kind = band_kind(model.region(mod, ang, px, model.min_region(N, M), model.log_nt(N, M), model.DEVICE_ZERO))
        if kind and len(found.get(kind, ())) < each and kind == band_kind(model.region(mod, ang, px, model.min_region(N, M), model.log_nt(N, M))):
            found.setdefault(kind, []).append(seed)
    return found


def min_reg_bar(N=96, M=80):
    """A region of exactly min_reg pixels that can be compared exactly: a bar in row 1 and, one row lower, a light pixel beyond each end.
    The two light pixels are the extremes along the axis and lie outside the rectangle sideways (width 1 about the bar), so the end
    sides pass through no pixel centre -> (mod, ang, key, pixels)"""
    n = model.min_region(N, M) - 2
    rng = np.random.default_rng(5)
    px = np.sort(np.concatenate([N + 3 + np.arange(n), [2 * N + 2, 2 * N + 3 + n]]))
    strong = px // N == 1
    mod, ang = np.zeros((M, N)), np.full((M, N), model.NOTDEF)
    mod.ravel()[px] = np.where(strong, rng.uniform(6.0, 20.0, len(px)), rng.uniform(3.0, 4.0, len(px)))
    ang.ravel()[px] = rng.uniform(-0.05, 0.05, len(px))
    key = np.full((M, N), 2 * M * N, np.uint32)
    key.ravel()[px] = px[0]
    return mod, ang, key, px


def check_search_against_row(pts, alg, accepted, p, width, ends, row):
    """the outcome of a rectangle search against a fixture row of the reference (rect_improve, the iterator's counts on the rectangle it
    left): counts, acceptance and probability equal; width and end points within 1e-9"""
    assert row[11] == 1.0
    assert (int(pts), int(alg), bool(accepted), float(p)) == (int(row[19]), int(row[20]), bool(row[12] > 0), float(row[18])), (pts, alg, accepted, p, row[11:])
    assert abs(width - row[17]) <= 1e-9, (width, row[17])
    for v, r in zip(ends, row[13:17]):
        assert abs(v - r) <= 1e-9, (ends, row[13:17])


def corner_band():
    """a band along the whole diagonal of a 30x20 field: its bounding box touches column 0 and N - 1 and row 0 and M - 1, and the
    rectangle's own box reaches past all four -> (mod, ang, key, pixels)"""
    M, N = 20, 30
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:M, 0:N]
    th = math.atan2(M - 1, N - 1)
    v = -xx * math.sin(th) + yy * math.cos(th)
    px = np.flatnonzero((np.abs(v) <= 1.3).ravel())
    mod, ang = np.zeros((M, N)), np.full((M, N), model.NOTDEF)
    mod.ravel()[px] = rng.uniform(6.0, 20.0, len(px))
    ang.ravel()[px] = th + rng.uniform(-0.05, 0.05, len(px))
    key = np.full((M, N), 2 * M * N, np.uint32)
    key.ravel()[px] = px[0]
    return mod, ang, key, px


def density_exactly_at_the_threshold():
    """14 equal pixels of row 0 spread symmetrically over 21 columns of a 40x12 field: centre, axis and extents come out exact, the
    rectangle is 20 x 1 and the density is the double 14 / 20 == 0.7 -> (mod, ang, key, pixels)"""
    M, N = 12, 40
    xs = np.array([5, 6, 7, 9, 10, 12, 14, 16, 18, 20, 21, 23, 24, 25])
    assert len(xs) == 14 and xs.sum() == 14 * 15 and np.array_equal(np.sort(30 - xs), xs)
    mod, ang = np.zeros((M, N)), np.full((M, N), model.NOTDEF)
    mod[0, xs], ang[0, xs] = 8.0, math.pi - 0.01
    key = np.full((M, N), 2 * M * N, np.uint32)
    key[0, xs] = xs[0]
    return mod, ang, key, xs.astype(np.int64)
