"""Node mode 2 (l3d_line3d_set_node_mode 2: the ranks of a device take turns on it) on a machine without a GPU: the header declares and the library
exports the new calls, the C++ facade's setNodeMode compiles and links, a null handle is refused, and scripts/memory_plan.py --mode turns plans a
turn within the one-GPU share's plan (--mode segpart --chain-world 1) plus the W - 1 shares of rows the other turns leave on the device."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["l3d_line3d_node_turn_records", "l3d_chain_release_records", "l3d_chain_records_digest"]

FACADE_SRC = r'''
#include "line3D_amd.hpp"
int main() {
    std::vector<int> devices{ 0, 0 };
    L3D::Line3D line3D("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false, devices);
    const bool ok = line3D.setNodeMode(2);
    const bool bad = line3D.setNodeMode(3);
    // (without a GPU there is no object: every call reports and returns false)
    return line3D.valid() ? ((ok && !bad) ? 0 : 1) : ((!ok && !bad) ? 0 : 1);
}
'''


def _lib():
    return C.CDLL(os.path.join(ROOT, "line3d_amd", "libline3d_amd.so"))


def test_header_declares_and_library_exports_the_new_calls():
    header = open(os.path.join(ROOT, "include", "line3d_amd.h")).read()
    lib = _lib()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in header, name
        assert getattr(lib, name) is not None
    assert "2 = the ranks that share a device TAKE TURNS" in header


def test_null_handles_are_refused():
    lib = _lib()
    n = C.c_int64(7)
    assert lib.l3d_line3d_node_turn_records(None, C.c_int(0), C.byref(n)) == 1
    assert lib.l3d_chain_release_records(None) == 1
    assert lib.l3d_chain_records_digest(None, None, None, C.c_int(0)) == 1
    assert lib.l3d_line3d_set_node_mode(None, C.c_int(2)) == 1


def test_facade_set_node_mode_compiles_and_links():
    import torch
    lib = os.path.join(ROOT, "line3d_amd")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
        open(src, "w").write(FACADE_SRC)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
        if not torch.cuda.is_available():
            assert subprocess.run([exe], stderr=subprocess.DEVNULL, timeout=120).returncode == 0


def _plan(*args):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "scripts", "memory_plan.py")] + [str(x) for x in args] + ["--json"], timeout=120)
    return json.loads(out.decode())


def test_memory_plan_turns_runs_and_stays_within_the_share_plus_the_other_shares_of_rows():
    for V, S, N, W, kept in ((512, 2000, 12, 8, 0.1), (2048, 4000, 24, 8, 0.25), (256, 4000, 24, 4, 0.48)):
        common = ["--views", V, "--segments", S, "--neighbors", N, "--world", W, "--kept", kept]
        t = _plan("--mode", "turns", *common)
        s = _plan("--mode", "segpart", "--chain-world", 1, *common)
        assert t["mode"] == "turns" and t["world"] == W
        for key in ("scene", "arena_of_the_keep_set", "chain_scratch"):
            assert t["per_turn_gb"][key] > 0, key
        for key in ("shares_of_rows_and_hypotheses", "one_fill_block"):
            assert t["across_turns_gb"][key] > 0, key
        # (two decimals of a GB in either plan)
        assert t["turn_peak_gb"] <= s["peak_gb"] + (W - 1) * t["share_rows_gb"] + 0.02, (t["turn_peak_gb"], s["peak_gb"], t["share_rows_gb"])
        # the arena and the chain's scratch of a turn are gone before the fill: the turn's arena is no part of the fill's phase
        assert t["peak_gb"] >= t["turn_peak_gb"]
        assert t["peak_gb"] == max(t["phases_gb"].values())


def test_memory_plan_turns_prints_its_table():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "scripts", "memory_plan.py"), "--mode", "turns", "--views", "512", "--segments", "2000", "--neighbors", "12",
                                   "--world", "8", "--kept", "0.1"], timeout=120).decode()
    assert "[turn] kept arena" in out and "[others]" in out and "peak over the phases" in out
