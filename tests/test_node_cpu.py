"""A node object (l3d_line3d_create_node) and its in-process all-gather (l3d_node_comm_*, l3d_exchange_node) on a machine without a GPU: the
C++ facade's device-list constructor compiles and links, bad arguments are refused before any device is touched, no GPU is reported as such, and
k_node_gather compiles for gfx950 to 16-byte vector loads and stores without scratch."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FACADE_SRC = r'''
#include "line3D_amd.hpp"
int main() {
    // a reference driver's construction line with the device list appended (main_vsfm.cpp:116-119)
    std::vector<int> devices{ 0, 0 };
    L3D::Line3D* line3D = new L3D::Line3D("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false, devices);
    L3D::Line3D braced("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false, { 0, 0, 0 });
    std::list<L3D::L3DFinalLine3D> r;
    line3D->compute3Dmodel(false);
    line3D->getResult(r);
    std::vector<L3D::float4> segs(3, L3D::float4{ 0.f, 0.f, 10.f, 10.f });
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    const double K[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t[3] = { 0, 0, 0 };
    line3D->addImage_fixed_sim(0, 640, 480, segs, K, K, t, sim, 1920, false);
    const bool no_gpu = !line3D->valid() && !braced.valid();
    const unsigned n = line3D->numCameras();
    delete line3D;
    return (r.empty() && (no_gpu ? n == 0 : n == 1)) ? 0 : 1;   // (without a GPU every call reports and returns)
}
'''


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def test_facade_device_list_constructor_compiles_and_links():
    lib = os.path.join(ROOT, "line3d_amd")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.cpp")
        open(src, "w").write(FACADE_SRC)
        exe = os.path.join(td, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lline3d_amd",
                               "-Wl,-rpath," + lib, "-o", exe])
        if not _gpu_present():
            assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 0


def _create_node(lib, devices, n):
    h = C.c_void_p()
    rc = lib.l3d_line3d_create_node(devices, C.c_int(n), C.c_int(10), C.c_float(5.0), C.c_float(1.0), C.c_float(3.5), C.c_float(10.0),
                                    C.c_float(0.25), C.c_int(1), C.c_int(0), C.byref(h))
    return rc, h


def test_node_creation_refuses_bad_arguments_and_reports_no_device():
    from line3d_amd import capi
    lib = capi.load_library()
    lib.l3d_line3d_destroy.argtypes = [C.c_void_p]
    lib.l3d_node_comm_destroy.argtypes = [C.c_void_p]
    ok = np.array([0, 0], np.int32)
    neg = np.array([0, -1], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    bad = [(None, 2), (p(ok), 0), (p(ok), -3), (p(neg), 2)]
    for devs, n in bad:
        rc, h = _create_node(lib, devs, n)
        assert rc == 1 and not h.value, (n, rc)                  # L3D_ERR_INVALID
        hc = C.c_void_p()
        assert lib.l3d_node_comm_create(devs, C.c_int(n), C.byref(hc)) == 1 and not hc.value
    assert lib.l3d_node_comm_create(p(ok), C.c_int(2), None) == 1
    # (out == NULL)
    assert lib.l3d_line3d_create_node(p(ok), C.c_int(2), C.c_int(10), C.c_float(5.0), C.c_float(1.0), C.c_float(3.5), C.c_float(10.0),
                                      C.c_float(0.25), C.c_int(1), C.c_int(0), None) == 1
    for n in (1, 2):
        rc, h = _create_node(lib, p(ok), n)
        hc = C.c_void_p()
        rcc = lib.l3d_node_comm_create(p(ok), C.c_int(n), C.byref(hc))
        if _gpu_present():
            assert rc == 0 and rcc == 0
            assert lib.l3d_line3d_num_ranks(h) == n
            lib.l3d_line3d_destroy(h)
            lib.l3d_node_comm_destroy(hc)
        else:
            assert rc == 4 and rcc == 4 and not h.value and not hc.value     # L3D_ERR_NODEVICE, like l3d_line3d_create
    assert lib.l3d_line3d_num_ranks(None) == 0
    assert lib.l3d_line3d_set_node_mode(None, 0) == 1


def test_python_refuses_device_and_devices_together():
    import pytest
    from line3d_amd import capi
    from line3d_amd.pipeline import Line3D
    with pytest.raises(ValueError):
        Line3D("", device=0, devices=[0, 0])
    if not _gpu_present():
        with pytest.raises(capi.L3DError):
            Line3D("", devices=[0, 0])
        with pytest.raises(capi.L3DError):
            capi.NodeComm([0, 0])


def _kernel_blocks(asm, name):
    """the function body and the metadata entry of the one kernel whose mangled name contains `name`"""
    m = re.search(r"^(_Z\S*%s\S*):" % name, asm, flags=re.M)
    assert m, "no kernel %s in the listing" % name
    sym = m.group(1)
    body = asm[m.end():asm.index(".Lfunc_end", m.end())]
    meta_at = asm.index(".name:           " + sym)
    meta = asm[asm.rindex("  - .", 0, meta_at):asm.find("\n  - ", meta_at) if asm.find("\n  - ", meta_at) > 0 else len(asm)]
    return body, meta


def test_node_gather_is_vector_code_without_scratch(tmp_path):
    src = os.path.join(ROOT, "line3d_amd", "csrc", "l3d_node.hip")
    out = str(tmp_path / "node.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-x", "hip", "-S",
                           "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
    asm = open(out).read()
    body, meta = _kernel_blocks(asm, "k_node_gather")
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
    assert "scratch_" not in body
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(r"\.%s:\s+(\d+)" % key, meta)
        assert vals == ["0"], (key, vals)
    # nothing but ordinary loads and stores: no atomics, no waits on memory written by another rank
    assert "atomic" not in body and "s_sleep" not in body
