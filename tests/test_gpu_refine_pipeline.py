"""The refinement in the pipeline (Line3D.set_refinement) on the small scene: lines, their order and their 2-D segments stay, every refined line's 3-D
segments are collinear, the result is l3d_refine_lines on the same clusters byte for byte, an object without the option gives the bytes it gave before,
a node object gives the ordinary object's refined bytes, and the TXT writer writes the refined segments.

rms_after <= rms_before is asserted for every line of this scene and holds on it (145 lines, 164 with diffusion); it is not a property of the method -- the
Huber cost is what falls, the unweighted rms may rise: on the 64 x 2000 x 12 scene one line of 8028 does (profiles/refine_times.txt)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(scene, refine=None, diffusion=False, devices=None, clear=False):
    from line3d_amd.pipeline import Line3D, load_scene
    l3d = Line3D("", matchingNeighbors=6, devices=devices) if devices is not None else Line3D("", matchingNeighbors=6)
    if refine is not None:
        l3d.set_refinement(True, *refine)
    if clear:
        l3d.set_refinement(False)
    load_scene(l3d, scene)
    l3d.compute3Dmodel(diffusion)
    return l3d


def _bytes(result):
    return [(tuple(s2), b"".join(a.tobytes() + b.tobytes() for a, b in s3)) for s2, s3 in result]


def _inverse_transform(inp, P):
    """Line3D::inverseTransform in the library's order of operations: Rinv (P scale_inv + tneg), every product and sum rounded once"""
    R, s, t = inp["Rinv"], inp["scale_inv"], inp["tneg"]
    v = [P[0] * s + t[0], P[1] * s + t[1], P[2] * s + t[2]]
    return np.array([R[i, 0] * v[0] + R[i, 1] * v[1] + R[i, 2] * v[2] for i in range(3)])


def _check_refined(l3d, plain_result, gpu_ctx, params):
    result, ref = l3d.getResult(), l3d.refinement()
    assert len(result) > 0 and len(result) == len(plain_result)
    assert [s2 for s2, _ in result] == [s2 for s2, _ in plain_result], "lines, order and 2-D segments as in the unrefined run"
    assert set(ref["status"].tolist()) <= {0, 1, 2, 3} and len(ref["status"]) == len(result)
    print("status counts", np.bincount(ref["status"], minlength=4), "rms before/after (pooled)", np.sqrt(np.mean(ref["rms_before"] ** 2)), np.sqrt(np.mean(ref["rms_after"] ** 2)),
          "lines with rms_after > rms_before:", int((ref["rms_after"] > ref["rms_before"]).sum()))
    assert np.all(ref["rms_after"] <= ref["rms_before"])
    inp = l3d.refinement_input()
    assert inp["group_start"][-1] == sum(len(s2) for s2, _ in result)
    direct = gpu_ctx.refine_lines(inp["group_start"], inp["member_cam"], inp["member_seg"], inp["member_pts"], inp["cameras"], *params)
    assert direct["rms_before"].tobytes() == ref["rms_before"].tobytes() and direct["rms_after"].tobytes() == ref["rms_after"].tobytes()
    assert direct["iterations"].tobytes() == ref["iterations"].tobytes()
    k = 0
    for li, ((_, s3), (_, p3)) in enumerate(zip(result, plain_result)):
        n = int(direct["seg_count"][li])
        if n == 0:
            assert ref["status"][li] in (2, 3) and _bytes([((), s3)]) == _bytes([((), p3)]), "nothing emitted: the unrefined segments stay"
            continue
        assert ref["status"][li] == direct["status"][li] and len(s3) == n
        pts = []
        for i, (a, b) in enumerate(s3):
            q = direct["segs"][k + i]
            assert a.tobytes() == _inverse_transform(inp, q[:3]).tobytes() and b.tobytes() == _inverse_transform(inp, q[3:]).tobytes(), "line %d segment %d" % (li, i)
            pts += [a, b]
        k += n
        pts = np.array(pts)
        far = np.linalg.norm(pts - pts[0], axis=1)
        j = int(np.argmax(far))
        d = (pts[j] - pts[0]) / far[j]
        assert np.linalg.norm(np.cross(pts - pts[0], d), axis=1).max() <= 1e-9 * far[j], "line %d: refined segments are collinear" % li
    assert (ref["status"] <= 1).sum() > 0


@pytest.fixture(scope="module")
def plain(small_scene):
    l3d = _run(small_scene)
    out = l3d.getResult()
    from line3d_amd.capi import L3DError
    with pytest.raises(L3DError):
        l3d.refinement()
    l3d.close()
    return out


@pytest.fixture(scope="module")
def refined(small_scene):
    l3d = _run(small_scene, refine=(20, 2.0))
    yield l3d
    l3d.close()


def test_refined_result(refined, plain, gpu_ctx):
    _check_refined(refined, plain, gpu_ctx, (20, 2.0))
    assert _bytes(refined.getResult()) != _bytes(plain)


def test_option_cleared_gives_the_unrefined_bytes(small_scene, plain):
    l3d = _run(small_scene, refine=(20, 2.0), clear=True)
    assert _bytes(l3d.getResult()) == _bytes(plain)
    l3d.close()


def test_reset_keeps_the_setting(small_scene, refined):
    from line3d_amd.pipeline import load_scene
    want = _bytes(refined.getResult())
    refined.reset()
    load_scene(refined, small_scene)
    refined.compute3Dmodel(False)
    assert _bytes(refined.getResult()) == want


def test_node_object_gives_the_refined_bytes(small_scene, refined):
    node = _run(small_scene, refine=(20, 2.0), devices=[0, 0])
    assert _bytes(node.getResult()) == _bytes(refined.getResult())
    assert node.refinement()["status"].tobytes() == refined.refinement()["status"].tobytes()
    node.close()


def test_txt_writer_writes_the_refined_segments(refined, tmp_path):
    path = str(tmp_path / "lines.txt")
    refined.save3DLinesAsTXT(path)
    rows = [ln.split() for ln in open(path).read().splitlines()]
    result = [r for r in refined.getResult() if len(r[1])]
    assert len(rows) == len(result)
    for row, (_, s3) in zip(rows, result):
        n = int(row[0])
        assert n == len(s3)
        want = ["%g" % x for a, b in s3 for x in list(a) + list(b)]
        assert row[1:1 + 6 * n] == want


def test_with_diffusion(small_scene, gpu_ctx):
    p = _run(small_scene, diffusion=True)
    plain_result = p.getResult()
    p.close()
    l3d = _run(small_scene, refine=(20, 2.0), diffusion=True)
    _check_refined(l3d, plain_result, gpu_ctx, (20, 2.0))
    l3d.close()
