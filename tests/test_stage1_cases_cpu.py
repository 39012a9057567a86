"""tests/stage1_cases.py without a GPU: each crafted segment set is the case its name claims -- the rows, tiles, chunks, blocks and pairs that
tests/test_gpu_stage1_paths.py relies on are there, by the contract oracle's dense buffers."""
import numpy as np
import pytest

import stage1_cases as sc
from helpers import sector_rejected


def exp(name, seg_range="case"):
    return sc.expected(sc.get_case(name), seg_range=seg_range)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_shape_and_candidates(name):
    case = sc.get_case(name)
    e = exp(name)
    S, N = len(case["src_segs"]), len(case["offsets"])
    assert case["tgt_segs"].shape == (int(case["offsets"][:, 1].sum()), 4) and case["F"].shape == (N, 3, 3) and np.all(np.diff(case["tbm"]) > 0)
    assert e["count"].sum() > 0 and e["upper"].sum() > e["count"].sum(), name           # candidates, and pairs only the depth test drops
    assert int(case["offsets"][:, 1].max()) * S <= 2.5e5                                  # (about 2e5 pairs per camera at the most)
    count = e["count"].reshape(S, N)
    for cam in case["tbm"]:
        if cam in case.get("empty_cams", ()):
            assert e["upper"].reshape(S, N)[:, cam].sum() == 0, (name, cam)                # (meant to have none: the oracle says so)
        elif case["offsets"][cam, 1] >= 3:
            assert count[:, cam].sum() > 0, (name, "camera %d has no candidate" % cam)
    others = np.setdiff1d(np.arange(N), case["tbm"])
    assert count[:, others].sum() == 0


def test_src_per_block_rule():
    """the launcher's rule (mirrored in stage1_cases.src_per_block; the GPU test holds the mirror to the hook's report): 64 where that fills the
    GPU, halved down to 8 for small grids -- what the cases get, and a partial last workgroup in every case under the rule and under spb 64"""
    seen = {name: sc.case_spb(sc.get_case(name)) for name in sc.CASES}
    assert seen["tiles"] == 8 and seen["wide"] == 8 and seen["many_rows"] == 8 and seen["cams_96"] == 16 and seen["cams_97"] == 16, seen
    assert sc.src_per_block(4000, 4000, 24) == 64 and sc.src_per_block(10, 10, 1) == 8
    assert sc.src_per_block(600, 40, 7) == 8 and sc.src_per_block(600, 1300, 7) == 32 and sc.src_per_block(130, 600, 97) == 64
    assert sc.src_per_block(100, 100, 1, forced=64) == 64 and sc.src_per_block(100, 100, 1, forced=8) == 8 and sc.src_per_block(100, 100, 1, forced=100) == 64
    partial = 0
    for name in sc.CASES:
        case = sc.get_case(name)
        n = [len(case["src_segs"])] + ([case["seg_range"][1] - case["seg_range"][0]] if case["seg_range"] else [])
        assert any(v % 64 != 0 for v in n), name                                        # a partial last workgroup under spb 64 ...
        partial += any(v % seen[name] != 0 for v in n)                                  # ... and under the rule (adversarial: 120 = 15 x 8)
    assert partial >= len(sc.CASES) - 1


def test_tiles():
    case = sc.get_case("tiles")
    w = case["offsets"][:, 1].tolist()
    assert w == [0, 1, 63, 64, 65, 0, 255, 256, 257, 513] and len(case["src_segs"]) == 70
    e = exp("tiles")
    for cam in (2, 3, 4, 6, 7, 8, 9):           # candidates in the last wave / word of the camera
        k = e["kept"][cam]
        assert k[:, (w[cam] - 1) // 64 * 64:].any(), cam
    assert e["kept"][9][:, 512].any() or e["passed"][9][:, 512].any()                   # the lone target of the third tile passes the overlap test


def test_dense_rows():
    e = exp("dense_rows")
    bits, cands = set(e["upper"].tolist()), set(e["count"].tolist())
    for what, have in (("set bits", bits), ("candidates", cands)):
        assert {63, 64, 65, 128, 129} <= have, (what, sorted(have)[-40:])              # both sides of the batch of 64 and of two batches
        assert max(have) > 129, what
    assert e["upper"].sum() - e["count"].sum() >= 200                                   # pairs that pass the overlap test without four positive depths
    assert ((e["upper"] > 0) & (e["count"] == 0)).any()                                 # a row whose every bit is dropped
    carried = 0
    for cam, p in e["passed"].items():
        k = e["kept"][cam]
        for y in range(len(p)):
            x = np.flatnonzero(p[y])                                                     # rank of a pair = its position among the row's set bits
            if len(x) > 64:
                kk = k[y, x]
                carried += bool((~kk[:64]).any() and kk[64:].any())
    assert carried >= 1                                                                 # the packing carries `written` across batches of 64


def test_wide():
    case = sc.get_case("wide")
    assert case["offsets"][:, 1].tolist() == [4100, 16384] and len(case["src_segs"]) == 9
    e = exp("wide")
    assert e["kept"][0][:, 4096:].any() and e["kept"][1][:, 16320:].any() and e["kept"][0][:, :64].any() and e["kept"][1][:, :64].any()
    p = e["passed"][0]
    assert (p[:, :4096].any(1) & p[:, 4096:].any(1)).any()                              # one row's prefix spans both chunks of 64 words
    assert (e["kept"][0][:, :4096].any(1) & e["kept"][0][:, 4096:].any(1)).any()


def test_many_rows():
    case = sc.get_case("many_rows")
    S, N = len(case["src_segs"]), len(case["offsets"])
    s0, s1 = case["seg_range"]
    assert (S, N, s0, s1) == (600, 7, 37, 411) and S * N > 4096 and (s0 * N) % 4 != 0 and ((s1 - s0) * N) % 4096 != 0
    full = exp("many_rows", seg_range=None)["count"]
    assert full[:4096].any() and full[4096:].any() and full[:s0 * N].any() and full[s1 * N:].any()
    ranged = exp("many_rows")["count"]
    assert ranged[s0 * N:s0 * N + 64].any() and ranged[s1 * N - 64:s1 * N].any() and not ranged[:s0 * N].any() and not ranged[s1 * N:].any()
    blocks = np.add.reduceat(exp("many_rows", seg_range=None)["upper"], np.arange(0, S * N, 256))
    assert len(blocks) == 17 and (blocks == 0).sum() >= 1 and (blocks > 0).sum() >= 10
    assert (blocks[1:-1] == 0).any() and blocks[-1] > 0                                  # an empty block with full ones on both sides


@pytest.mark.parametrize("N", [96, 97])
def test_many_cameras(N):
    case = sc.get_case("cams_%d" % N)
    S = len(case["src_segs"])
    assert len(case["offsets"]) == N and S == 130 and case["spb"] == 64 and set(case["offsets"][:, 1].tolist()) == {3, 4, 5} and case["seg_range"] == (1, 130)
    # a workgroup of 64 sources, rows 96 apart: 24 blocks of 256 rows when it starts at a multiple of 64 segments (64 * 96 = 24 * 256), 25 -- the
    # most there can be; the LDS table holds 26 -- from segment 1 on, where the case's range starts
    span = lambda y0, c: (((y0 + 63) * 96 + c) >> 8) - ((y0 * 96 + c) >> 8) + 1
    assert max(span(y0, c) for y0 in (0, 64) for c in range(96)) == 24 and max(span(y0, c) for y0 in (1, 65) for c in range(96)) == 25
    assert max(span(y0, c) for y0 in range(130) for c in range(96)) == 25 <= 64 * 96 // 256 + 2
    up = exp("cams_%d" % N)["upper"].reshape(S, N)
    blocks = np.add.reduceat(up.reshape(-1), np.arange(0, S * N, 256))
    assert (blocks > 0).sum() >= 24                                                     # candidates in (nearly) every block a workgroup spans


def test_subset():
    case = sc.get_case("subset")
    assert case["tbm"].tolist() == [1, 2, 4] and len(case["offsets"]) == 6
    e = exp("subset")
    count = e["count"].reshape(-1, 6)
    assert all(count[:, c].sum() > 0 for c in (1, 2, 4)) and count[:, [0, 3, 5]].sum() == 0


def test_facing():
    case = sc.get_case("facing")
    e = exp("facing")
    S = len(case["src_segs"])
    assert 140 <= S <= 160
    wrapped = sum(sector_rejected(dict(offsets=case["offsets"], src_segs=case["src_segs"], tgt_segs=case["tgt_segs"], F=case["F"]), cam, e["kept"][cam])
                  for cam in case["tbm"])
    assert wrapped >= 20, wrapped
    # e_d = e1 - e2 against the bounding box of a tile of 256 targets, as k_pair_mask forms it (float64 here): crossing switches the sector test off
    crossing = 0
    one = lambda a: np.concatenate([a, np.ones((len(a), 1))], 1)
    s = case["src_segs"].astype(np.float64)
    for cam in case["tbm"]:
        o0, n = case["offsets"][cam]
        F = case["F"][cam].astype(np.float64)
        e1, e2 = one(s[:, :2]) @ F.T, one(s[:, 2:]) @ F.T
        ed = e1 - e2
        for t0 in range(0, n, 256):
            t = case["tgt_segs"][o0 + t0:o0 + min(n, t0 + 256)].astype(np.float64)
            bx0, bx1, by0, by1 = t[:, [0, 2]].min(), t[:, [0, 2]].max(), t[:, [1, 3]].min(), t[:, [1, 3]].max()
            ext0, ext1 = max(abs(bx0), abs(bx1)), max(abs(by0), abs(by1))
            m = sum(1e-4 * (np.abs(e[:, 0]) * ext0 + np.abs(e[:, 1]) * ext1 + np.abs(e[:, 2])) for e in (e1, e2))     # the margins of the two lines
            lo = ed[:, 2] + np.minimum(ed[:, 0] * bx0, ed[:, 0] * bx1) + np.minimum(ed[:, 1] * by0, ed[:, 1] * by1)
            hi = ed[:, 2] + np.maximum(ed[:, 0] * bx0, ed[:, 0] * bx1) + np.maximum(ed[:, 1] * by0, ed[:, 1] * by1)
            crossing += int((~((lo > m) | (hi < -m))).sum())
    assert crossing >= 1


def test_adversarial():
    case = sc.get_case("adversarial")
    e = exp("adversarial")
    fam = lambda k: "end" if k.startswith("end") else "iou" if k.startswith("iou") else k
    for cam in case["tbm"]:
        kinds = np.array([fam(k) for k in case["kinds"][cam]])
        assert len(kinds) == case["offsets"][cam, 1] >= 120 * 15
        for f in ("end", "iou", "tiny", "span"):
            col = kinds == f
            assert col.sum() >= 300, (cam, f)
            # per family: pairs of a target with the source it was built from on both sides of the decision
            own = np.zeros_like(e["kept"][cam])
            own[case["owner"][cam], np.arange(len(kinds))] = True
            assert e["kept"][cam][:, col].any() and (e["passed"][cam] & ~e["kept"][cam])[:, col].any() and (~e["passed"][cam] & own)[:, col].any(), (cam, f)
            if f != "span":     # (a target that spans the image overlaps its own source's pair by a few per cent: never accepted with it)
                assert (e["kept"][cam] & own)[:, col].any() and (e["passed"][cam] & own)[:, col].any(), (cam, f)


def test_degenerate():
    case = sc.get_case("degenerate")
    e = exp("degenerate")
    assert not case["F"][3].any() and np.array_equal(case["centers"][3], case["C_src"])
    assert e["upper"].reshape(-1, 4)[:, 3].sum() == 0                                    # F = 0: the oracle lets no pair pass
    far = case["tgt_segs"][case["offsets"][1, 0] + 256:case["offsets"][1, 0] + 300]
    assert np.abs(far).max() > 32768 and np.abs(case["tgt_segs"][case["offsets"][1, 0]:case["offsets"][1, 0] + 256]).max() < 32768
    assert e["passed"][1][:, 256:300].any()                                             # pairs of the far tile reach the exact test and pass it
    s = case["src_segs"]
    assert np.array_equal(s[5, :2], s[5, 2:]) and np.hypot(*(s[6, 2:] - s[6, :2])) < 1 and np.isfinite(case["tgt_segs"]).all()
