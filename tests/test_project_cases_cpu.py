"""The projection's case table (tests/project_cases.py) on a machine without a GPU: every case is what its name claims (asserted with the model of
tests/project_model.py, the rules of include/line3d_amd.h "PROJECTION AND OVERLAYS" in numpy), the host entry point l3d_test_project_lines_host --
the very functions the kernels run -- equals the model bit for bit on all of them, every refusal comes with its code and cause, and two
convention checks that the model cannot share a mistake with: a hand-computed projection, and the synthetic scene generator's own segments."""
import ctypes as C

import numpy as np
import pytest

import project_cases as pc
import project_model as pm

NAMES = [c["name"] for c in pc.CASES]


same = pc.same


def host(case):
    from line3d_amd import capi
    return capi.project_lines_host(case["seg3d"], case["cams"], case["near"], case["margin"])


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(name):
    case = pc.BY_NAME[name]
    segs, src, flags, start = pc.model_of(case)
    counts = np.diff(start).tolist()
    assert len(start) == len(case["cams"]) + 1 and start[0] == 0 and start[-1] == len(src) == len(flags) == len(segs)
    claim = case["claim"]
    if claim[0] == "counts":
        assert counts == claim[1]
    elif claim[0] == "flags":
        assert flags.tolist() == claim[1]
    elif claim[0] == "exact":
        assert segs.tolist() == [[float(v) for v in row] for row in claim[1]] and flags.tolist() == [0] * len(claim[1])
    elif claim[0] == "touch":
        assert counts == [0]
        assert pm.pair(case["cams"][0], case["seg3d"][0], case["near"], case["margin"]) is None
        t0, t1 = pm.clip.trace                     # the rule ran through its four edges and ended on t0 == t1
        assert t0 == t1 and 0.0 < t0 < 1.0
    elif claim[0] == "empty_row":
        assert counts[claim[1]] == 0 and all(c > 0 for k, c in enumerate(counts) if k != claim[1])
    elif claim[0] == "mixed":
        n = len(case["seg3d"])
        assert all(0 < c < n for c in counts), counts
        assert {0, 3} <= set(flags.tolist()) and ({1, 2} & set(flags.tolist()))
        for c in range(len(counts)):                # input order within a camera
            assert np.all(np.diff(src[start[c]:start[c + 1]]) > 0)
    else:
        raise AssertionError(claim)


def test_the_named_rectangle_cases_meet_p_zero():
    """the segment on the line u = -0.5 has p == 0 at the left and right edges, with q == 0 at the left one; its neighbour q < 0"""
    for name, q_sign in (("rect_on_the_left_border", 0), ("rect_left_of_the_border", -1)):
        case = pc.BY_NAME[name]
        s = case["seg3d"][0]
        uP, uQ = s[0] / s[2], s[3] / s[5]
        assert uP == uQ and np.sign(uP - (-0.5)) == q_sign


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model_bit_for_bit(name):
    case = pc.BY_NAME[name]
    got = host(case)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.uint8 and got[3].dtype == np.int64
    assert same(got, pc.model_of(case)), name


@pytest.mark.parametrize("name", [r[0] for r in pc.REFUSALS])
def test_refusals(name):
    from line3d_amd import capi
    _, overrides, code, word = next(r for r in pc.REFUSALS if r[0] == name)
    kw = pc.refusal_arguments(overrides)
    with pytest.raises(capi.L3DError) as e:
        capi.project_lines_host(kw["seg3d"], kw["cams"], kw["near"], kw["margin"])
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_null_pointers_and_negative_counts_are_refused():
    from line3d_amd import capi
    lib = capi.load_library()
    seg = np.array([[0, 0, 2, 0.1, 0.1, 2]], np.float64)
    cams = capi.cameras([pc.cam()])
    start = np.zeros(2, np.int64)
    o, s, f = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_ubyte)()
    good = [capi._p(seg), C.c_int(1), cams, C.c_int(1), C.c_double(1e-3), C.c_double(0.0), C.byref(o), C.byref(s), C.byref(f), capi._p(start)]
    assert lib.l3d_test_project_lines_host(*good) == 0
    for p in (o, s, f):
        lib.l3d_free(p)
    for i, bad in ((0, None), (2, None), (6, None), (7, None), (8, None), (9, None), (1, C.c_int(-1)), (3, C.c_int(-1))):
        args = list(good)
        args[i] = bad
        assert lib.l3d_test_project_lines_host(*args) == 1, i


def test_convention_hand_computed():
    """K = [[100, 0, 32], [0, 100, 24], [0, 0, 1]], R = I, t = 0: P = (0, 0, 2), Q = (0.5, 0, 2) is (32, 24)-(57, 24), exactly"""
    from line3d_amd import capi
    segs, src, flags, start = capi.project_lines_host([[0, 0, 2, 0.5, 0, 2]], [pc.cam()], near=1e-6, margin=0.0)
    assert segs.tolist() == [[32.0, 24.0, 57.0, 24.0]] and src.tolist() == [0] and flags.tolist() == [0] and start.tolist() == [0, 1]


def test_convention_the_scene_generator():
    """synth.make_scene without noise: every 3-D segment projects into every view as the generator's own 2-D segment, within two f32 roundings at
    coordinates below 2048 (2 x 2048 x 2^-24 = 2.44e-4 px)"""
    from line3d_amd import capi
    from line3d_amd.synth import make_scene
    scene = make_scene(4, 60, 3, seed=5, noise_px=0.0, width=640, height=480, f=500.0)
    cams = [(v["K"], v["R"], v["t"], v["width"], v["height"]) for v in scene.views]
    segs, src, flags, start = capi.project_lines_host(scene.segs3d, cams)
    assert np.diff(start).tolist() == [60] * 4 and not flags.any()
    for c, v in enumerate(scene.views):
        mine = segs[start[c]:start[c + 1]]
        assert src[start[c]:start[c + 1]].tolist() == list(range(60))
        for k, g in enumerate(v["gt"]):
            err = np.abs(mine[g].astype(np.float64) - v["segments"][k].astype(np.float64)).max()
            print("view %d segment %d: %.3g px" % (c, k, err))
            assert err <= 2.5e-4
