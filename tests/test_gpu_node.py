"""One Line3D object over several GPUs of one process (l3d_line3d_create_node) and its in-process all-gather (l3d_exchange_node, k_node_gather),
with virtual ranks on the one GPU of the test box (a device may repeat in the list): the gather itself, then compute3Dmodel on a node against the
single-device object -- lines, affinity list, per-view kept counts --, the config-2 golden, a C++ driver built against the facade, and a failing
exchange that must end the run on every rank, name the rank, and leave the object usable after reset."""
import hashlib
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

from helpers import assert_lines_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_node_exchange_gathers_every_rank_in_order():
    """W = 3 ranks on threads of this process, send pointers off 16-byte alignment, slots of 1 .. 2^20 + 3 bytes; 50 exchanges in a row per size,
    every send slot rewritten before each one: every rank's recv_block is the concatenation in rank order, and nothing behind it is touched."""
    import torch
    from line3d_amd.capi import NodeComm
    W, reps, guard = 3, 50, 64
    sizes = [1, 15, 16, 4097, (1 << 20) + 3]
    comm = NodeComm([0] * W)
    streams = [torch.cuda.Stream(device=0) for _ in range(W)]
    for r in range(W):
        comm.bind(r, streams[r].cuda_stream)
    offs = [(5 * r + 3) % 16 or 7 for r in range(W)]
    send = [torch.zeros(sizes[-1] + 32, dtype=torch.uint8, device="cuda:0") for _ in range(W)]
    recv = [torch.zeros(W * sizes[-1] + guard, dtype=torch.uint8, device="cuda:0") for _ in range(W)]
    torch.cuda.synchronize()

    def payload(i, r, n):
        return np.random.default_rng(1000003 * i + 7919 * r + n).integers(0, 256, n, dtype=np.uint8)

    errors = []

    def rank(r):
        try:
            with torch.cuda.stream(streams[r]):
                for n in sizes:
                    recv[r].fill_(0xA5)
                    for i in range(reps):
                        send[r][offs[r]:offs[r] + n].copy_(torch.from_numpy(payload(i, r, n)))
                        rc = comm.exchange(i, send[r].data_ptr() + offs[r], recv[r].data_ptr(), n, streams[r].cuda_stream)
                        if rc != 0:
                            errors.append((r, n, i, "rc %d" % rc))
                            return
                        got = recv[r].cpu().numpy()
                        exp = np.concatenate([payload(i, q, n) for q in range(W)])
                        if not np.array_equal(got[:W * n], exp):
                            bad = int(np.flatnonzero(got[:W * n] != exp)[0])
                            errors.append((r, n, i, "first wrong byte %d (slot of rank %d)" % (bad, bad // n)))
                            comm.abort()
                            return
                        if not (got[W * n:W * n + guard] == 0xA5).all():
                            errors.append((r, n, i, "wrote past the block"))
                            comm.abort()
                            return
        except Exception as e:      # noqa: BLE001
            errors.append((r, repr(e)))
            comm.abort()
    th = [threading.Thread(target=rank, args=(r,)) for r in range(W)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in th), "a rank hangs"
    torch.cuda.synchronize()
    comm.close()
    assert not errors, errors


def _single(scene, N, diffusion, loader=None):
    from line3d_amd.pipeline import Line3D, load_scene
    l = Line3D("", matchingNeighbors=N, device=0)
    (loader or load_scene)(l, scene)
    l.compute3Dmodel(diffusion)
    A, n_nodes = l.affinity()
    out = dict(lines=l.getResult(), A=_sha(A), n_A=len(A), n_nodes=n_nodes, kept=l.chain_summary()["n_kept"].copy(), cams=l.numCameras())
    l.close()
    return out


def _node(scene, N, devices, diffusion, loader=None, mode=None):
    from line3d_amd.pipeline import Line3D, load_scene
    l = Line3D("", matchingNeighbors=N, devices=devices)
    assert l.num_ranks() == len(devices)
    if mode is not None:
        l.set_node_mode(mode)
    (loader or load_scene)(l, scene)
    l.compute3Dmodel(diffusion)
    A, n_nodes = l.affinity()
    out = dict(lines=l.getResult(), A=_sha(A), n_A=len(A), n_nodes=n_nodes, kept=l.chain_summary()["n_kept"].copy(), cams=l.numCameras())
    l.close()
    return out


def _assert_same(got, ref):
    assert got["cams"] == ref["cams"]
    assert got["n_nodes"] == ref["n_nodes"] and got["n_A"] == ref["n_A"] and got["A"] == ref["A"], "affinity list differs from the single device's"
    assert np.array_equal(got["kept"], ref["kept"]), "per-view kept counts differ from the single device's"
    assert_lines_equal(got["lines"], ref["lines"], 0.0)


@pytest.mark.parametrize("diffusion", [False, True], ids=["no diffusion", "diffusion"])
def test_node_equals_one_device_on_a_helix(diffusion):
    from line3d_amd.synth import make_scene
    N = 8
    scene = make_scene(48, 800, N, seed=31)
    ref = _single(scene, N, diffusion)
    assert len(ref["lines"]) > 20
    for devices in ([0, 0], [0, 0, 0, 0]):
        _assert_same(_node(scene, N, devices, diffusion), ref)


@pytest.mark.parametrize("mode", [0, 1], ids=["segments of every view", "blocks of views"])
def test_node_equals_one_device_on_scattered_non_mutual_neighbourhoods(mode):
    from line3d_amd.pipeline import load_scene_worldpoints
    from line3d_amd.synth import make_scene_scattered
    N = 8
    scene = make_scene_scattered(36, 260, seed=77)
    ref = _single(scene, N, False, loader=load_scene_worldpoints)
    assert len(ref["lines"]) > 5
    _assert_same(_node(scene, N, [0, 0, 0], False, loader=load_scene_worldpoints, mode=mode), ref)


def test_node_blocks_mode_equals_one_device_on_a_helix():
    from line3d_amd.synth import make_scene
    N = 8
    scene = make_scene(48, 800, N, seed=31)
    _assert_same(_node(scene, N, [0, 0], True, mode=1), _single(scene, N, True))


def test_node_reproduces_the_config2_golden():
    """devices = [0, 0] on BASELINE configs[1] / configs[3]: the lines the ORACLE alone produced (tests/golden/config2_full.npz)"""
    from line3d_amd.pipeline import Line3D, load_scene
    from line3d_amd.synth import make_scene
    g = np.load(os.path.join(ROOT, "tests", "golden", "config2_full.npz"))
    V, S, N, seed = (int(x) for x in g["shape"])
    scene = make_scene(V, S, N, seed=seed)
    l = Line3D("", matchingNeighbors=N, devices=[0, 0])
    try:
        for diffusion, tag in ((False, "plain"), (True, "rdd")):
            l.reset()
            load_scene(l, scene)
            l.compute3Dmodel(diffusion)
            if not diffusion:
                edges, n_nodes = l.affinity()
                assert len(edges) == int(g["affinity_n"]) and n_nodes == int(g["n_nodes"])
                assert _sha(edges) == str(g["affinity_sha256"]), "affinity list differs from the oracle's"
                assert int(np.sum(l.chain_summary()["n_kept"], dtype=np.int64)) == int(g["kept_n"].sum())
            ids, id_off, pts, pt_off = g[tag + "_ids"], g[tag + "_id_off"], g[tag + "_pts"], g[tag + "_pt_off"]
            exp = [([(int(c), int(s)) for c, s in ids[id_off[k]:id_off[k + 1]]], [(p[:3], p[3:]) for p in pts[pt_off[k]:pt_off[k + 1]]])
                   for k in range(len(id_off) - 1)]
            assert len(exp) > 2000
            assert assert_lines_equal(l.getResult(), exp, tol=1e-4) <= 1e-4
    finally:
        l.close()


DRIVER = r'''
// a reference-style driver: the scene from a flat file, one construction line chooses one GPU or a list of them
#include <cstdio>
#include <cstdlib>
#include "line3D_amd.hpp"
int main(int argc, char** argv) {
    if (argc < 5) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int V = 0, N = 0;
    if (fread(&V, 4, 1, f) != 1 || fread(&N, 4, 1, f) != 1) return 3;
    std::vector<int> devices;
    for (int a = 4; a < argc; ++a) devices.push_back(atoi(argv[a]));
    L3D::Line3D* line3D = devices.size() == 1 ? new L3D::Line3D(argv[3], N, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false, devices[0])
                                              : new L3D::Line3D(argv[3], N, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false, devices);
    for (int v = 0; v < V; ++v) {
        unsigned id = 0, w = 0, h = 0; int S = 0, M = 0;
        if (fread(&id, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1 || fread(&S, 4, 1, f) != 1) return 3;
        std::vector<L3D::float4> segs((size_t)S);
        double K[9], R[9], t[3];
        if (fread(segs.data(), 16, (size_t)S, f) != (size_t)S || fread(K, 8, 9, f) != 9 || fread(R, 8, 9, f) != 9 || fread(t, 8, 3, f) != 3) return 3;
        if (fread(&M, 4, 1, f) != 1) return 3;
        std::map<unsigned int, float> sim;
        for (int k = 0; k < M; ++k) { unsigned o = 0; float s = 0; if (fread(&o, 4, 1, f) != 1 || fread(&s, 4, 1, f) != 1) return 3; sim[o] = s; }
        line3D->addImage_fixed_sim(id, w, h, segs, K, R, t, sim, 1920, false);
    }
    fclose(f);
    line3D->compute3Dmodel(false);
    std::list<L3D::L3DFinalLine3D> result;
    line3D->getResult(result);
    line3D->save3DLinesAsTXT(result, argv[2]);
    delete line3D;
    return result.empty() ? 4 : 0;
}
'''


def test_cpp_driver_with_a_device_list_writes_the_one_device_txt():
    from line3d_amd.synth import make_scene
    N = 8
    scene = make_scene(24, 300, N, seed=5)
    lib = os.path.join(ROOT, "line3d_amd")
    with tempfile.TemporaryDirectory() as td:
        src, exe, data = os.path.join(td, "drv.cpp"), os.path.join(td, "drv"), os.path.join(td, "scene.bin")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
        with open(data, "wb") as f:
            f.write(np.array([len(scene.views), N], np.int32).tobytes())
            for v in scene.views:
                segs = np.ascontiguousarray(v["segments"], np.float32)
                f.write(np.array([v["id"], v["width"], v["height"], len(segs)], np.uint32).tobytes())
                f.write(segs.tobytes())
                for a in (v["K"], v["R"], v["t"]):
                    f.write(np.ascontiguousarray(a, np.float64).tobytes())
                f.write(np.array([len(v["sims"])], np.int32).tobytes())
                for o, s in sorted(v["sims"].items()):
                    f.write(np.array([o], np.uint32).tobytes() + np.array([s], np.float32).tobytes())
        outs = {}
        for devs in (["0"], ["0", "0"]):
            out = os.path.join(td, "lines_%d.txt" % len(devs))
            r = subprocess.run([exe, data, out, td + "/"] + devs, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (devs, r.returncode, r.stderr[-2000:])
            outs[len(devs)] = open(out).read().splitlines()
        assert len(outs[1]) > 10
        assert sorted(outs[2]) == sorted(outs[1])


FAILURE_SCRIPT = r'''
import sys
from helpers import assert_lines_equal
from line3d_amd.capi import L3DError
from line3d_amd.pipeline import Line3D, load_scene
from line3d_amd.synth import make_scene
N = 8
scene = make_scene(32, 300, N, seed=9)
ref = Line3D("", matchingNeighbors=N, device=0)
load_scene(ref, scene)
ref.compute3Dmodel(False)
l = Line3D("", matchingNeighbors=N, devices=[0, 0])
load_scene(l, scene)
try:
    l.compute3Dmodel(False)
    sys.exit("the injected exchange failure did not fail compute3Dmodel")
except L3DError as e:
    msg = str(e)
assert "rank 1 (device 0)" in msg, msg
l.reset()
load_scene(l, scene)
l.compute3Dmodel(False)
assert_lines_equal(l.getResult(), ref.getResult(), 0.0)
print("node failure ok:", msg)
'''


@pytest.mark.parametrize("k", [1, 6], ids=["first exchange", "a view's exchange mid-chain"])
def test_node_exchange_failure_fails_every_rank_and_reset_recovers(k):
    """L3D_NODE_FAIL_AT=k (test-only option, read from rank 1's context): rank 1's k-th exchange returns 1 on the host -- a failing call, no device
    fault.  compute3Dmodel must return an error that names rank 1, within the time limit (nothing waits for ever); after reset the same object
    computes the scene as one device does."""
    env = dict(os.environ, L3D_NODE_FAIL_AT=str(k), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", FAILURE_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "node failure ok" in r.stdout
