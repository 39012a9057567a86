"""The drivers' overlays: sfm.reconstruct_from_images(overlay_dir=...) and examples/main_vsfm_amd.cpp --overlays write one binary P6 file per view, of the
view's size, holding Line3D.overlay of the view's (undistorted) image -- a grey canvas in the C++ driver's flow over segment caches."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ref.npz")
DIST = (-0.2, 0.03)


def read_ppm(path):
    data = open(path, "rb").read()
    magic, size, maxval, rest = data.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert magic == b"P6" and maxval == b"255" and len(rest) == w * h * 3
    return np.frombuffer(rest, np.uint8).reshape(h, w, 3)


def test_reconstruct_from_images_writes_an_overlay_per_view(gpu_ctx, tmp_path):
    """the six-view wiring scene of the JPEG tests (tests/golden/jpeg_ref.npz), files and decoded arrays in turn, every camera with distortion"""
    from line3d_amd import sfm
    from line3d_amd.synth import make_scene
    g = np.load(GOLDEN)
    scene = make_scene(6, 30, 6, seed=11, noise_px=0.0, width=320, height=200, f=250.0, seg_len=(0.3, 0.8))
    files = [g["view%d/bytes" % k].tobytes() for k in range(6)]
    images = [gpu_ctx.decode_jpeg(d) for d in files]
    cams = [dict(name="img%d.jpg" % k, focal=250.0, dist=np.array([-DIST[0], 0.0]), cv_dist=np.array(DIST), R=v["R"], t=v["t"], worldpoints=np.arange(10, dtype=np.uint32))
            for k, v in enumerate(scene.views)]
    out = str(tmp_path / "overlays")
    l3d = sfm.reconstruct_from_images(sfm.SfmScene(cams, 10), lambda i, name: files[i] if i % 2 else images[i], str(tmp_path) + os.sep, neighbors=6,
                                      load_and_store_segments=False, overlay_dir=out)
    try:
        assert l3d.numCameras() == 6 and len(l3d.getResult()) > 0
        assert sorted(os.listdir(out)) == ["overlay_%d.ppm" % i for i in range(6)]
        changed = 0
        for i in range(6):
            got = read_ppm(os.path.join(out, "overlay_%d.ppm" % i))
            K = sfm.intrinsics(250.0, 320, 200)
            und = gpu_ctx.undistort(images[i], K, k1=DIST[0], k2=DIST[1])
            und = np.repeat(und[:, :, None], 3, axis=2) if und.ndim == 2 else und
            assert got.shape == (200, 320, 3)
            assert np.array_equal(got, l3d.overlay(i, und))
            changed += int((got != und).any())
        assert changed > 0
    finally:
        l3d.close()


def test_cpp_driver_writes_an_overlay_per_view(tmp_path):
    """main_vsfm_amd --overlays over segment caches (no image folder): grey canvases of the views' size with the overlays, on the scene of tests/test_sfm_readers.py
    (10 views x 300 segments, neighbours from 400 world points: it is known to give lines)"""
    import l3d_oracle_sfm as osfm
    from helpers import synth_worldpoints, write_nvm
    from line3d_amd.io import segment_cache_filename
    from line3d_amd.synth import make_scene
    sc = make_scene(10, 300, 6, seed=77)
    pts = synth_worldpoints(sc, 400, seed=5)
    nvm = str(tmp_path / "scene.nvm")
    write_nvm(nvm, sc, pts)
    data_dir = str(tmp_path / "L3D_data")
    os.makedirs(data_dir)
    for i, v in enumerate(sc.views):
        osfm.write_segment_cache(data_dir + segment_cache_filename(i, v["width"], v["height"], True), v["segments"], {})
    exe = str(tmp_path / "main_vsfm_amd")
    lib = os.path.join(ROOT, "line3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "main_vsfm_amd.cpp"), "-L" + lib, "-lline3d_amd",
                           "-Wl,-rpath," + lib, "-o", exe])
    out_dir, ov_dir = str(tmp_path / "out"), str(tmp_path / "overlays")
    os.makedirs(out_dir)
    os.makedirs(ov_dir)
    r = subprocess.run([exe, "--overlays", ov_dir, nvm, data_dir, "6", "0", out_dir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "10 overlays written" in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(ov_dir)) == sorted("overlay_%d.ppm" % i for i in range(10))
    overlays = [read_ppm(os.path.join(ov_dir, "overlay_%d.ppm" % i)) for i in range(10)]
    assert {o.shape for o in overlays} == {(1080, 1920, 3)}
    assert any((o != 128).any() for o in overlays), "no overlay shows a line"
