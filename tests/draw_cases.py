"""Crafted images and segments for the drawing (l3d_draw_segments / l3d_test_draw_segments_host; include/line3d_amd.h, "PROJECTION AND OVERLAYS", 2),
each built to be the case its name claims.  CASES: dict(name, image (uint8, H x W or H x W x C; a view with padded rows where the name says so),
segments (n, 4) float32, colors (n_colors, 4) uint8, color_index (None or n int32), width_px, opacity, claim) -- claim: (kind, ...) that
tests/test_draw_cases_cpu.py holds the case to, by the key plane of tests/draw_model.py:
  ("q_rows", {row: q}, (j0, j1))   on columns j0..j1 the winning coverage is q on the rows named and 0 on their neighbours
  ("q_cols", {col: q}, (i0, i1))   the same for columns
  ("span", n)                      the pixels covered span n columns (rows for a y-major line) -- the steps along the major axis
  ("covered", lo, hi)              between lo and hi pixels are covered
  ("unchanged",)                   the image comes back as it was
  ("winner", k)                    every covered pixel is won by segment k
  ("generic",)                     some pixel changes
REFUSALS: (name, keyword overrides of a good call, status, a word of the message)."""
import numpy as np

import draw_model as dm


def _image(h, w, c, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if c == 0 else (h, w, c), dtype=np.uint8)


A = _image(48, 64, 3, 1)                         # 64 x 48 x 3
_B_wide = _image(17, 40, 0, 2)
B = _B_wide[:, :33]                              # 33 x 17 x 1, rows 40 bytes apart
C4 = _image(30, 40, 4, 3)                        # 40 x 30 x 4: the fourth channel stays
D = _image(20, 140, 3, 4)                        # 140 x 20 x 3: long horizontal lines
E = _image(80, 20, 3, 5)                         # 20 x 80 x 3: long vertical lines

RED = [[255, 0, 0, 255]]
PAL = [[255, 0, 0, 255], [0, 255, 0, 128], [0, 0, 255, 0], [10, 200, 90, 255]]


def _case(name, image, segments, claim, colors=RED, color_index=None, width_px=1.0, opacity=255):
    return dict(name=name, image=image, segments=np.array(segments, np.float32).reshape(-1, 4), colors=np.array(colors, np.uint8).reshape(-1, 4),
                color_index=None if color_index is None else np.array(color_index, np.int32), width_px=width_px, opacity=opacity, claim=claim)


def _fan(n, cx, cy, r):
    a = np.arange(n) * (np.pi / n)
    return np.stack([cx - r * np.cos(a), cy - r * np.sin(a), cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


SLANT = [[10.3, 5.7, 50.2, 40.1]]

CASES = [_case("width_%s" % str(w).replace(".", "_"), A, SLANT, ("generic",), width_px=w) for w in (0.5, 1.0, 2.5, 9.0, 64.0)] + [
    # ---- directions and positions
    _case("horizontal_integer_y", A, [[5, 10, 40, 10]], ("q_rows", {10: 255}, (5, 40))),
    _case("horizontal_half_y", A, [[5, 10.5, 40, 10.5]], ("q_rows", {10: 128, 11: 128}, (5, 40))),
    _case("vertical_integer_x", A, [[20, 4, 20, 40]], ("q_cols", {20: 255}, (4, 40))),
    _case("vertical_half_x", A, [[20.5, 4, 20.5, 40]], ("q_cols", {20: 128, 21: 128}, (4, 40))),
    _case("diagonal_45", A, [[5, 5, 35, 35]], ("generic",), width_px=2.5),
    _case("y_major", A, [[10, 2, 20, 45]], ("generic",), width_px=2.5),
    _case("y_major_reversed", A, [[22.25, 44.5, 9.75, 1.5]], ("generic",), width_px=9.0),
    # ---- lengths
    _case("shorter_than_a_pixel", A, [[10.2, 10.3, 10.6, 10.4]], ("covered", 1, 9)),
    _case("zero_length_disc", A, [[20, 20, 20, 20]], ("covered", 60, 90), width_px=9.0),
    _case("steps_63", D, [[3, 9, 63, 9]], ("span", 63), width_px=1.5),
    _case("steps_64", D, [[3, 9, 64, 9]], ("span", 64), width_px=1.5),
    _case("steps_65", D, [[3, 9, 65, 9]], ("span", 65), width_px=1.5),
    _case("steps_129", D, [[3, 9.25, 129, 10.75]], ("span", 129), width_px=1.5),
    _case("steps_65_y_major", E, [[9, 3, 10.5, 65]], ("span", 65), width_px=1.5),
    # ---- outside the image
    _case("wholly_outside", A, [[-50, -50, -10, -20], [70, 10, 90, 30]], ("unchanged",), width_px=2.5),
    _case("crosses_every_border", A, [[-20, -15, 90, 70], [-20, 70, 90, -15]], ("generic",), width_px=2.5),
    _case("ends_at_1e7", A, [[32 - 1e7, 24 - 7e6, 32 + 1e7, 24 + 7e6]], ("generic",)),
    _case("nan_is_dropped", A, [[np.nan, 5, 40, 30], [5, 5, 40, 30], [5, 5, np.inf, 30]], ("winner", 1)),
    # ---- overlap
    _case("index_tie", A, [[5, 20, 50, 20], [5, 20, 50, 20]], ("winner", 1), colors=PAL),
    _case("fan_4097", A, _fan(4097, 32.0, 24.0, 20.0), ("generic",), colors=PAL),
    # ---- colour
    _case("alpha_modulo", A, [[5, 5, 55, 5], [5, 15, 55, 15], [5, 25, 55, 25], [5, 35, 55, 35], [5, 42, 55, 42]], ("generic",), colors=PAL, width_px=2.5),
    _case("alpha_0", A, [[5, 5, 55, 40]], ("unchanged",), colors=[[255, 255, 255, 0]], width_px=2.5),
    _case("opacity_0", A, [[5, 5, 55, 40]], ("unchanged",), colors=PAL, width_px=2.5, opacity=0),
    _case("opacity_200", A, [[5, 5, 55, 40], [5, 40, 55, 5]], ("generic",), colors=PAL, width_px=2.5, opacity=200),
    _case("color_index", A, [[5, 5, 55, 5], [5, 15, 55, 15], [5, 25, 55, 25]], ("generic",), colors=PAL, color_index=[3, 3, 1], width_px=2.5),
    _case("no_segments", A, np.zeros((0, 4)), ("unchanged",)),
    # ---- the other image shapes
    _case("one_channel_padded", B, [[2, 2, 30, 14], [0, 16, 32, 0], [16, 8, 16, 8]], ("generic",), colors=PAL, width_px=2.5),
    _case("one_channel_padded_wide", B, [[-5, 8.5, 40, 8.5]], ("generic",), colors=[[200, 0, 0, 255]], width_px=64.0),
    _case("four_channels", C4, [[2, 2, 38, 27], [38, 3, 1, 28]], ("generic",), colors=PAL, width_px=2.5, opacity=200),
    _case("four_channels_index", C4, [[2, 15, 38, 15.5]], ("generic",), colors=PAL, color_index=[3], width_px=9.0),
]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_MODEL = {}


def model_of(case):
    """the model's image for a case, computed once"""
    if case["name"] not in _MODEL:
        _MODEL[case["name"]] = dm.draw(case["image"], case["segments"], case["colors"], case["color_index"], case["width_px"], case["opacity"])
    return _MODEL[case["name"]]


_GOOD = dict(image=A, segments=np.array([[5, 5, 40, 30]], np.float32), colors=np.array(RED, np.uint8), color_index=None, width_px=1.0, opacity=255)

REFUSALS = [
    ("width_below", dict(width_px=0.49), 1, "width_px"),
    ("width_above", dict(width_px=64.5), 1, "width_px"),
    ("width_nan", dict(width_px=float("nan")), 1, "width_px"),
    ("opacity_above", dict(opacity=256), 1, "opacity"),
    ("opacity_negative", dict(opacity=-1), 1, "opacity"),
    ("no_colours", dict(colors=np.zeros((0, 4), np.uint8)), 1, "null"),
    ("index_out_of_range", dict(color_index=np.array([1], np.int32)), 1, "color_index"),
    ("index_negative", dict(color_index=np.array([-1], np.int32)), 1, "color_index"),
    ("two_channels", dict(image=np.zeros((8, 8, 2), np.uint8)), 1, "channels"),
]


def refusal_arguments(overrides):
    kw = dict(_GOOD)
    kw.update(overrides)
    return kw
