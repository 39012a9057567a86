"""The COLMAP model reader (l3d_sfm_read_colmap, line3d_amd/csrc/l3d_sfm.cpp; sfm.read_colmap) on tests/golden/colmap_small (written by
tests/golden/make_golden_colmap.py from its table): text and binary read to the same scene, R from the quaternion, the parameter order of every
model, the half-pixel shift, the models without a lens, and files that are cut short or name a model that does not exist.  No device."""
import importlib.util
import os
import shutil
import struct

import numpy as np
import pytest

from line3d_amd import capi, sfm

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "colmap_small")

_spec = importlib.util.spec_from_file_location("make_golden_colmap", os.path.join(HERE, "golden", "make_golden_colmap.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# what l3d_sfm_camera_lens must make of a model's parameters: (lens model, fx, fy, cx, cy, coefficients), written from the header's table
EXPECT = {
    "SIMPLE_PINHOLE": lambda p: (capi.LENS_BROWN, p[0], p[0], p[1], p[2], []),
    "PINHOLE": lambda p: (capi.LENS_BROWN, p[0], p[1], p[2], p[3], []),
    "SIMPLE_RADIAL": lambda p: (capi.LENS_BROWN, p[0], p[0], p[1], p[2], [p[3]]),
    "RADIAL": lambda p: (capi.LENS_BROWN, p[0], p[0], p[1], p[2], [p[3], p[4]]),
    "OPENCV": lambda p: (capi.LENS_BROWN, p[0], p[1], p[2], p[3], p[4:8]),
    "FULL_OPENCV": lambda p: (capi.LENS_BROWN, p[0], p[1], p[2], p[3], p[4:12]),
    "OPENCV_FISHEYE": lambda p: (capi.LENS_FISHEYE, p[0], p[1], p[2], p[3], p[4:8]),
    "SIMPLE_RADIAL_FISHEYE": lambda p: (capi.LENS_FISHEYE, p[0], p[0], p[1], p[2], [p[3]]),
    "RADIAL_FISHEYE": lambda p: (capi.LENS_FISHEYE, p[0], p[0], p[1], p[2], [p[3], p[4]]),
}
NO_LENS = {"FOV", "THIN_PRISM_FISHEYE"}


def _rotation(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _check_camera(cam, model_name, params):
    assert cam["model"] == model_name and cam["params"].tolist() == list(params)        # the raw accessor: the file's numbers
    if model_name in NO_LENS:
        assert cam["lens"] is None and cam["K"] is None and model_name in cam["lens_error"]
        return
    model, fx, fy, cx, cy, k = EXPECT[model_name](list(params))
    lens = cam["lens"]
    assert lens.model == model
    assert (lens.fx, lens.fy, lens.cx, lens.cy) == (fx, fy, cx - 0.5, cy - 0.5)          # COLMAP's pixel centre (0.5, 0.5) is (0, 0) here
    assert list(lens.k) == list(k) + [0.0] * (8 - len(k))
    assert np.array_equal(cam["K"], np.array([[fx, 0.0, cx - 0.5], [0.0, fy, cy - 0.5], [0.0, 0.0, 1.0]]))
    assert cam["size"] == gen.SIZE


def test_fixture_is_what_the_generator_writes(tmp_path):
    gen.write_txt(str(tmp_path / "txt"))
    gen.write_bin(str(tmp_path / "bin"))
    total = 0
    for sub, names in (("txt", ("cameras.txt", "images.txt")), ("bin", ("cameras.bin", "images.bin"))):
        for n in names:
            with open(os.path.join(FIXTURE, sub, n), "rb") as a, open(tmp_path / sub / n, "rb") as b:
                data = a.read()
                assert data == b.read()
                total += len(data)
    assert total < 8192
    assert {m[1] for m in gen.MODELS} == set(EXPECT) | NO_LENS and len(gen.IMAGES) == 5
    assert any(" " in im[4] for im in gen.IMAGES)
    assert any(p < 0 for im in gen.IMAGES for _, _, p in im[5]) and any(p >= 0 for im in gen.IMAGES for _, _, p in im[5])


@pytest.mark.parametrize("form", ["txt", "bin"])
def test_scene(form):
    scene = sfm.read_colmap(os.path.join(FIXTURE, form))
    assert len(scene.cameras) == len(gen.IMAGES)
    by_id = {c[0]: c for c in gen.CAMERAS}
    for cam, (iid, q, t, cid, name, obs) in zip(scene.cameras, gen.IMAGES):
        assert cam["name"] == name and cam["camera_id"] == cid
        assert np.abs(cam["R"] - _rotation(q)).max() < 1e-15
        assert cam["t"].tolist() == list(t)
        assert cam["worldpoints"].tolist() == [p for _, _, p in obs if p >= 0]
        _check_camera(cam, by_id[cid][2], by_id[cid][3])
        assert cam["focal"] == by_id[cid][3][0]
    assert scene.n_points == 1 + max(p for im in gen.IMAGES for _, _, p in im[5])
    # (k1, k2) exists for the pinhole and radial models only
    assert scene.cameras[4]["model"] == "SIMPLE_PINHOLE" and scene.cameras[4]["cv_dist"].tolist() == [0.0, 0.0]
    assert scene.cameras[0]["model"] == "OPENCV" and scene.cameras[0]["cv_dist"] is None


def test_text_and_binary_read_to_the_same_scene():
    a, b = (sfm.read_colmap(os.path.join(FIXTURE, f)) for f in ("txt", "bin"))
    assert a.n_points == b.n_points and len(a.cameras) == len(b.cameras)
    for x, y in zip(a.cameras, b.cameras):
        assert set(x) == set(y)
        for key in x:
            if key == "lens":
                assert (x[key] is None) == (y[key] is None) and (x[key] is None or bytes(x[key]) == bytes(y[key]))
            elif isinstance(x[key], np.ndarray):
                assert x[key].tobytes() == y[key].tobytes(), key
            else:
                assert x[key] == y[key], key


@pytest.mark.parametrize("form", ["txt", "bin"])
def test_parameter_order_of_every_model(tmp_path, form):
    """the fixture's camera file with an image file in which the five images are repeated until every camera has been named: the scene's cameras
    are its images, so this is how all eleven cameras of the fixture are reached"""
    d = tmp_path / form
    os.makedirs(d)
    shutil.copy(os.path.join(FIXTURE, form, "cameras." + form), d)
    images = [(k + 1,) + gen.IMAGES[k % 5][1:3] + (gen.CAMERAS[k][0],) + gen.IMAGES[k % 5][4:] for k in range(len(gen.CAMERAS))]
    keep = gen.IMAGES
    try:
        gen.IMAGES = images
        if form == "txt":
            gen.write_txt(str(tmp_path / "scratch"))
            shutil.copy(tmp_path / "scratch" / "images.txt", d)
        else:
            with open(d / "images.bin", "wb") as f:
                f.write(gen.bin_bytes()[1])
    finally:
        gen.IMAGES = keep
    scene = sfm.read_colmap(str(d))
    assert [c["model"] for c in scene.cameras] == [c[2] for c in gen.CAMERAS]
    for cam, (_, _, name, params) in zip(scene.cameras, gen.CAMERAS):
        _check_camera(cam, name, params)
    # the (k1, k2) accessor: the pinhole and radial models with fx == fy
    for cam, (_, _, name, params) in zip(scene.cameras, gen.CAMERAS):
        expect = {"SIMPLE_PINHOLE": [0.0, 0.0], "SIMPLE_RADIAL": [params[-1], 0.0], "RADIAL": list(params[-2:])}.get(name)
        assert (cam["cv_dist"] is None) if expect is None else (cam["cv_dist"].tolist() == expect), name     # (the fixture's PINHOLE has fx != fy)


def test_accessors_on_other_scenes(tmp_path):
    """an NVM scene: BROWN with the cv_distortion coefficients, a zero source camera, size 0; the model accessor does not apply"""
    import ctypes as C
    p = tmp_path / "s.nvm"
    p.write_text("NVM_V3\n\n1\na.jpg 500 1 0 0 0 0 0 0 0.07 0\n\n0\n")
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.l3d_sfm_read_nvm(str(p).encode(), C.byref(h)) == 0
    try:
        lens, K, w, hh = capi.Lens(), (C.c_double * 9)(*([1.0] * 9)), C.c_int(5), C.c_int(5)
        assert lib.l3d_sfm_camera_lens(h, C.c_int(0), C.byref(lens), K, C.byref(w), C.byref(hh)) == 0
        assert lens.model == capi.LENS_BROWN and (lens.fx, lens.fy, lens.cx, lens.cy) == (0.0, 0.0, 0.0, 0.0)
        assert list(lens.k) == [float(-np.float32(0.07)), 0.0] + [0.0] * 6 and (w.value, hh.value) == (0, 0) and list(K) == [0.0] * 9
        assert lib.l3d_sfm_camera_model(h, C.c_int(0), None, None, None) == 1
        lib.l3d_sfm_camera_id.restype = C.c_int
        assert lib.l3d_sfm_camera_id(h, C.c_int(0)) == -1
    finally:
        lib.l3d_sfm_free.argtypes = [C.c_void_p]
        lib.l3d_sfm_free(h)


def test_refusals(tmp_path):
    with pytest.raises(RuntimeError, match="cameras"):
        sfm.read_colmap(str(tmp_path / "nothing"))
    cams, ims = gen.bin_bytes()
    # every truncation of the two binary files is a message on the scene object, never a crash or a scene
    for which, data in (("cameras.bin", cams), ("images.bin", ims)):
        for cut in sorted(set(list(range(0, 40)) + list(range(40, len(data), 7)))):
            d = tmp_path / ("%s_%d" % (which, cut))
            os.makedirs(d)
            (d / "cameras.bin").write_bytes(cams[:cut] if which == "cameras.bin" else cams)
            (d / "images.bin").write_bytes(ims[:cut] if which == "images.bin" else ims)
            with pytest.raises(RuntimeError, match="truncated|no images"):
                sfm.read_colmap(str(d))
    # an unknown model id, an impossible count
    d = tmp_path / "model99"
    os.makedirs(d)
    (d / "cameras.bin").write_bytes(cams[:12] + struct.pack("<i", 99) + cams[16:])
    (d / "images.bin").write_bytes(ims)
    with pytest.raises(RuntimeError, match="unknown model id 99"):
        sfm.read_colmap(str(d))
    d = tmp_path / "count"
    os.makedirs(d)
    (d / "cameras.bin").write_bytes(struct.pack("<Q", 1 << 60) + cams[8:])
    (d / "images.bin").write_bytes(ims)
    with pytest.raises(RuntimeError, match="truncated"):
        sfm.read_colmap(str(d))
    # text: an unknown model name, too few parameters, an image that names a camera the file does not have
    for name, cameras, images, match in (
            ("name", "1 PINHOLE_X 640 480 1 2 3 4\n", "1 1 0 0 0 0 0 0 1 a.jpg\n\n", "unknown model 'PINHOLE_X'"),
            ("few", "1 OPENCV 640 480 1 2 3 4 5 6 7\n", "1 1 0 0 0 0 0 0 1 a.jpg\n\n", "too few parameters"),
            ("camera", "1 PINHOLE 640 480 1 2 3 4\n", "1 1 0 0 0 0 0 0 2 a.jpg\n\n", "names camera 2")):
        d = tmp_path / name
        os.makedirs(d)
        (d / "cameras.txt").write_text(cameras)
        (d / "images.txt").write_text(images)
        with pytest.raises(RuntimeError, match=match):
            sfm.read_colmap(str(d))



def test_reader_under_sanitizers(tmp_path):
    """tests/cpp/colmap_reader_asan.cpp: the reader's source and a main of its own, built with AddressSanitizer and UBSan as a plain host program, over
    the fixture, every truncation of its four files and damaged bytes"""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "colmap_asan")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "colmap_reader_asan.cpp"),
                           os.path.join(root, "line3d_amd", "csrc", "l3d_sfm.cpp"), "-o", exe])
    run = subprocess.run([exe, FIXTURE, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
