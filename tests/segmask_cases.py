"""Crafted masks and segments for the segment mask (l3d_mask_segments / l3d_test_mask_segments_host; include/line3d_amd.h, "A SEGMENT MASK"), each
named for what it exercises.  A case is a dict: name; mask (uint8, H x W, possibly a view into wider rows); segments (n, 4) float32; kw: the mode and
its parameters as capi.segment_mask and segmask_model.filter_segments both take them; lens: None or dict(out_cam, model, src_cam, coeffs) as
segmask_model takes it; claim: (kind, ...) -- what tests/test_segmask_cases_cpu.py holds the case to, by the model's samples.

Masks run from 16 x 12 to 96 x 64.  hseg(x0, y, n) is a horizontal segment of n + 1 samples whose sample k reads pixel (x0 + k, y): it starts at
x0 + 0.25 and is n - 0.02 long, so the samples lie 1 - 0.02 / n apart and never drift across a pixel's edge."""
import numpy as np

import segmask_model as sm

DROP, CLIP, SPLIT = sm.DROP, sm.CLIP, sm.SPLIT


def hseg(x0, y, n, reverse=False):
    s = [x0 + 0.25, float(y), x0 + 0.25 + n - 0.02, float(y)]
    return s[2:] + s[:2] if reverse else s


def vseg(x, y0, n, reverse=False):
    s = [float(x), y0 + 0.25, float(x), y0 + 0.25 + n - 0.02]
    return s[2:] + s[:2] if reverse else s


def row_mask(w, h, y, x0, pattern, fill=0):
    """w x h of `fill` with row y set from column x0 by the pattern's characters: '1' = 255, '0' = 0"""
    m = np.full((h, w), fill, np.uint8)
    for k, c in enumerate(pattern):
        if 0 <= x0 + k < w:
            m[y, x0 + k] = 255 if c == "1" else 0
    return m


def stripes(w, h, period, on, axis=1):
    """columns (axis 1) or rows (axis 0) valid where index % period < on"""
    idx = np.arange(w if axis == 1 else h)
    line = np.where(idx % period < on, 255, 0).astype(np.uint8)
    return np.tile(line[None, :], (h, 1)) if axis == 1 else np.tile(line[:, None], (1, w))


def blocks(w, h, seed, cell=6, p=0.7):
    """cells of cell x cell pixels, each valid with probability p"""
    rng = np.random.default_rng(seed)
    g = rng.random(((h + cell - 1) // cell, (w + cell - 1) // cell)) < p
    return (np.kron(g, np.ones((cell, cell))) * 255).astype(np.uint8)[:h, :w].copy()


def random_segments(n, w, h, seed, max_len):
    """n segments with both ends within (or just outside) w x h, no longer than max_len, no coordinate near a half-integer grid by construction of
    the draw (floats of 24 bits: the chance of a sample on a pixel edge is nil, and a miss there would show as a host / model difference)"""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(-2.0, w + 1.0, n), rng.uniform(-2.0, h + 1.0, n)], 1)
    ang, ln = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.6, max_len, n)
    b = a + np.stack([np.cos(ang), np.sin(ang)], 1) * ln[:, None]
    return np.concatenate([a, b], 1).astype(np.float32)


def _kw(mode, threshold=1, keep_permille=500, max_gap=0, min_length=0.0):
    return dict(mode=mode, threshold=threshold, keep_permille=keep_permille, max_gap=max_gap, min_length=min_length)


def _case(name, mask, segments, kw, claim, lens=None):
    return dict(name=name, mask=mask, segments=np.asarray(segments, np.float32).reshape(-1, 4), kw=kw, lens=lens, claim=claim)


COUNT_SEGMENTS = random_segments(4097, 96, 64, 11, 14.0)
COUNT_MASK = blocks(96, 64, 12)


def _cases():
    c = []
    full = np.full((12, 16), 255, np.uint8)
    # ---- sample counts n + 1 at the ends of the ballot words: a 96-wide mask whose valid columns come in stripes of 5 of 7, the segment on one row,
    # starting left of the mask for the counts that do not fit in it.  (n + 1 = 2: a segment shorter than a pixel)
    st = stripes(96, 16, 7, 5)
    for n1 in (2, 63, 64, 65, 128, 129):
        x0 = 1 if n1 <= 65 else -18
        seg = [4.25, 3.0, 4.75, 3.0] if n1 == 2 else hseg(x0, 3, n1 - 1)
        for mode in (DROP, CLIP, SPLIT):
            c.append(_case("samples_%d_%s" % (n1, ("drop", "clip", "split")[mode]), st, [seg], _kw(mode, keep_permille=600), ("samples", n1)))
    # ---- directions
    grid = stripes(48, 40, 9, 6) & stripes(48, 40, 11, 8, axis=0)
    c.append(_case("horizontal", grid, [hseg(2, 4, 40)], _kw(SPLIT), ("direction", "h", False)))
    c.append(_case("horizontal_reversed", grid, [hseg(2, 4, 40, True)], _kw(SPLIT), ("direction", "h", True)))
    c.append(_case("vertical", grid, [vseg(3, 1, 36)], _kw(SPLIT), ("direction", "v", False)))
    c.append(_case("vertical_reversed", grid, [vseg(3, 1, 36, True)], _kw(SPLIT), ("direction", "v", True)))
    c.append(_case("diagonal", grid, [[1.3, 2.1, 44.9, 37.2], [45.2, 3.3, 2.4, 36.8]], _kw(SPLIT), ("direction", "d", False)))
    c.append(_case("diagonal_clip", grid, [[1.3, 2.1, 44.9, 37.2], [45.2, 3.3, 2.4, 36.8]], _kw(CLIP), ("direction", "d", False)))
    # ---- end points at .5: floor(x + 0.5) takes the pixel above
    half = row_mask(24, 12, 4, 0, "000011111111000000000000")
    c.append(_case("ends_at_half", half, [[3.5, 4.0, 11.5, 4.0], [11.5, 3.5, 3.5, 3.5]], _kw(SPLIT), ("half",)))
    # ---- ends outside the mask, and a segment wholly outside it
    c.append(_case("ends_outside", full, [[-6.3, 5.0, 21.8, 5.2], [7.0, -4.4, 7.5, 16.1]], _kw(SPLIT), ("outside", "ends")))
    c.append(_case("ends_outside_clip", full, [[-6.3, 5.0, 21.8, 5.2], [7.0, -4.4, 7.5, 16.1]], _kw(CLIP), ("outside", "ends")))
    c.append(_case("wholly_outside", full, [[20.4, 3.0, 30.2, 9.0], [2.0, -9.0, 12.0, -3.1], [3.0, 3.0, 9.0, 5.5]], _kw(SPLIT), ("outside", "whole")))
    c.append(_case("wholly_outside_drop", full, [[20.4, 3.0, 30.2, 9.0], [2.0, -9.0, 12.0, -3.1], [3.0, 3.0, 9.0, 5.5]], _kw(DROP, keep_permille=1), ("outside", "whole")))
    # ---- gaps of max_gap and max_gap + 1, and a gap that touches an end
    for g in (1, 3):
        c.append(_case("gap_%d_bridged" % g, row_mask(32, 12, 6, 2, "11111" + "0" * g + "111111"), [hseg(2, 6, 10 + g)], _kw(SPLIT, max_gap=g), ("gap", g, 1)))
        c.append(_case("gap_%d_not_bridged" % (g + 1), row_mask(32, 12, 6, 2, "11111" + "0" * (g + 1) + "11111"), [hseg(2, 6, 10 + g)], _kw(SPLIT, max_gap=g), ("gap", g, 2)))
        c.append(_case("gap_%d_bridged_clip" % g, row_mask(32, 12, 6, 2, "11111" + "0" * g + "111111"), [hseg(2, 6, 10 + g)], _kw(CLIP, max_gap=g), ("gap", g, 1)))
    c.append(_case("gap_touches_start", row_mask(32, 12, 6, 2, "0011111111111"), [hseg(2, 6, 12)], _kw(SPLIT, max_gap=3), ("gap_at_end", "start")))
    c.append(_case("gap_touches_end", row_mask(32, 12, 6, 2, "1111111111100"), [hseg(2, 6, 12)], _kw(SPLIT, max_gap=3), ("gap_at_end", "end")))
    c.append(_case("isolated_samples_bridged", row_mask(32, 12, 6, 2, "0101010000100"), [hseg(2, 6, 12)], _kw(SPLIT, max_gap=1), ("gap", 1, 1)))
    # ---- tied longest runs: CLIP takes the first
    c.append(_case("tied_runs", row_mask(32, 12, 6, 2, "011110011110011100"), [hseg(2, 6, 17)], _kw(CLIP), ("tie",)))
    c.append(_case("tied_runs_reversed", row_mask(32, 12, 6, 2, "011110011110011100"), [hseg(2, 6, 17, True)], _kw(CLIP), ("tie",)))
    # ---- min_length met exactly, and a sample short of it: dx = 15.5, n = 16; a run of 8 sample steps has s = 1/2, (s s) L2 = 240.25 / 4 = 7.75^2
    exact = row_mask(24, 12, 5, 0, "000011111111100000000000")          # pixels 4..12 <-> samples 4..12
    short = row_mask(24, 12, 5, 0, "000011111111000000000000")          # pixels 4..11 <-> samples 4..11
    for mode, tag in ((CLIP, "clip"), (SPLIT, "split")):
        c.append(_case("min_length_exact_" + tag, exact, [[0.5, 5.0, 16.0, 5.0]], _kw(mode, min_length=7.75), ("min_length", True)))
        c.append(_case("min_length_short_" + tag, short, [[0.5, 5.0, 16.0, 5.0]], _kw(mode, min_length=7.75), ("min_length", False)))
    # ---- all-valid and all-invalid masks
    inside = [[1.0, 1.0, 14.0, 10.0], [14.2, 0.3, 0.4, 10.9], [3.0, 2.0, 3.4, 2.2], [0.0, 11.0, 15.0, 11.0]]
    for mode, tag in ((DROP, "drop"), (CLIP, "clip"), (SPLIT, "split")):
        c.append(_case("all_valid_" + tag, full, inside, _kw(mode, keep_permille=1000, min_length=0.1), ("all_valid",)))
        c.append(_case("all_invalid_" + tag, np.zeros((12, 16), np.uint8), inside, _kw(mode, keep_permille=1), ("all_invalid",)))
    # ---- thresholds on a graded mask: column x holds min(255, 3 x)
    graded = np.tile(np.minimum(255, 3 * np.arange(96)).astype(np.uint8)[None, :], (16, 1))
    for thr in (1, 128, 255, 0):
        c.append(_case("threshold_%d" % thr, graded, [hseg(0, 7, 94), [90.2, 2.0, 20.7, 13.0]], _kw(CLIP, threshold=thr), ("threshold", thr)))
    # ---- keep_permille: 0 keeps what is not always dropped, 1000 wants every sample; an exact tie, a sample below it, a permille above it
    twenty = row_mask(32, 12, 6, 2, "11111111110000000000")              # 20 samples, 10 valid
    nineteen = row_mask(32, 12, 6, 2, "11111111100000000000")            # 9 valid
    c.append(_case("permille_0", np.zeros((12, 32), np.uint8), [hseg(2, 6, 19), [40.0, 3.0, 50.0, 4.0]], _kw(DROP, keep_permille=0), ("permille", "all")))
    c.append(_case("permille_1000", row_mask(32, 12, 6, 2, "1" * 20), [hseg(2, 6, 19), hseg(2, 6, 20)], _kw(DROP, keep_permille=1000), ("permille", "first")))
    c.append(_case("permille_tie_kept", twenty, [hseg(2, 6, 19)], _kw(DROP, keep_permille=500), ("permille_tie", 0)))
    c.append(_case("permille_tie_one_sample_less", nineteen, [hseg(2, 6, 19)], _kw(DROP, keep_permille=500), ("permille_tie", -1)))
    c.append(_case("permille_tie_one_permille_more", twenty, [hseg(2, 6, 19)], _kw(DROP, keep_permille=501), ("permille_tie", -1)))
    # ---- segments that are always dropped, between segments that are not
    nan, inf = float("nan"), float("inf")
    bad = [[2.0, 2.0, 9.0, 7.0], [5.0, 5.0, 5.0, 5.0], [nan, 1.0, 4.0, 4.0], [1.0, 1.0, inf, 4.0], [0.0, 3.0, 70000.0, 3.0], [3.0, 65540.0, 3.0, 2.0], [4.0, 9.0, 12.0, 3.0]]
    for mode, tag in ((DROP, "drop"), (CLIP, "clip"), (SPLIT, "split")):
        c.append(_case("always_dropped_" + tag, full, bad, _kw(mode, keep_permille=0), ("always_dropped", (0, 6))))
    # ---- a SPLIT that emits more segments than it was given
    c.append(_case("split_grows", stripes(64, 16, 8, 5), [hseg(1, 3, 60), hseg(2, 9, 58, True)], _kw(SPLIT), ("grows",)))
    # ---- segment counts at the ends of the workgroups (4 segments) and of the scan's tiles (4096 ints): prefixes of one set
    for n in (0, 1, 3, 4, 5, 4095, 4096, 4097):
        c.append(_case("count_%d" % n, COUNT_MASK, COUNT_SEGMENTS[:n], _kw(SPLIT, max_gap=1, min_length=1.5), ("count", n)))
    c.append(_case("count_4097_drop", COUNT_MASK, COUNT_SEGMENTS, _kw(DROP, keep_permille=800), ("count", 4097)))
    # ---- a row stride above the width: the mask is a view into wider rows whose other bytes are all valid
    wide = np.full((24, 56), 255, np.uint8)
    wide[:, :40] = blocks(40, 24, 5)
    c.append(_case("row_stride", wide[:, :40], random_segments(24, 40, 24, 6, 30.0), _kw(SPLIT), ("stride",)))
    # ---- lenses: the mask lies in the distorted image's grid at another size (96 x 64) than the grid the segments lie in (64 x 48)
    out_cam, src_cam = (50.0, 51.5, 31.7, 24.2), (70.0, 72.1875, 48.3, 31.8)
    lens_segs = random_segments(16, 64, 48, 7, 60.0)
    lens_mask = blocks(96, 64, 8, cell=7)
    for tag, model, coeffs in (("brown", sm.BROWN, (-0.21, 0.06, 0.0012, -0.0017, 0.01)), ("fisheye", sm.FISHEYE, (-0.04, 0.012, -0.005, 0.0015))):
        for mode, mtag in ((DROP, "drop"), (CLIP, "clip"), (SPLIT, "split")):
            c.append(_case("lens_%s_%s" % (tag, mtag), lens_mask, lens_segs, _kw(mode, max_gap=1, min_length=2.0), ("lens",),
                           lens=dict(out_cam=out_cam, model=model, src_cam=src_cam, coeffs=coeffs)))
    # a lens that is not active: the mask is in the segments' grid
    c.append(_case("lens_inactive", blocks(64, 48, 9), lens_segs, _kw(SPLIT), ("lens_inactive",), lens=dict(out_cam=out_cam, model=sm.BROWN, src_cam=None, coeffs=(0.0,) * 8)))
    return c


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_MODEL = {}


def model_of(case):
    """the model's (segments, src_index) for a case, computed once; the count cases are prefixes of the largest and share its run"""
    name = case["name"]
    if name in _MODEL:
        return _MODEL[name]
    if case["claim"][0] == "count" and name != "count_4097" and case["kw"]["mode"] == SPLIT:
        segs, src = model_of(BY_NAME["count_4097"])
        keep = src < case["claim"][1]
        _MODEL[name] = (segs[keep].copy(), src[keep].copy())
    else:
        _MODEL[name] = sm.filter_segments(case["segments"], case["mask"], lens=case["lens"], **case["kw"])
    return _MODEL[name]


def capi_mask(case, mask=None):
    """the case's capi.segment_mask (mask: a stand-in for the case's plane, e.g. a device tensor of the same content)"""
    from line3d_amd import capi
    lens, camera = None, None
    if case["lens"] is not None:
        L = case["lens"]
        lens, camera = capi.lens(L["model"], L["coeffs"], camera=L["src_cam"]), L["out_cam"]
    return capi.segment_mask(case["mask"] if mask is None else mask, lens=lens, camera=camera, **case["kw"])
