"""Images in device memory (include/line3d_amd.h, "Images in DEVICE memory"): k_det_ingest and k_det_egress against the numpy model of the conversion
rule (tests/device_image_model.py), byte for byte; then the detector, the undistortion and the add family on torch tensors against the host calls on
the same pixels, byte for byte; the refusals (through l3d_test_device_image_pointer and the field checks only: no bad pointer ever reaches a call
that could launch); and stream order.

Which ingest case reaches which path of k_det_ingest (l3d_device_image.hip):
  rows as bytes, the image one run, 16-byte loads      "hwc1", "hwc3" (8-bit, contiguous; source and slot are both aligned), "image 1 of N" where
                                                       H x W x 3 is a multiple of 16
  rows as bytes, row by row, 16-byte loads             "pitch+16 at 0": rows 16 bytes further apart than they are long, so every row's source is as
                                                       far off 16-byte alignment as its slot row
  rows as bytes, four 4-byte loads                     "pitch+16 at 4": the same with the base 4 bytes on
  rows as bytes, byte loads                            "crop at 1 / 2 / 3" (odd pitch: the rows' alignments differ), "flipped" at most sizes
  rows as bytes, partial chunks                        every row end; whole rows at widths 1 and 3
  pixel groups, vector loads of a plane                "chw", "broadcast", "grey crop", the dtype cases with stride_x 1 -- at widths that are multiples of 4
                                                       every group, otherwise the groups that happen to be aligned
  pixel groups, element loads (the generic path)       "reversed", "hwc4", "hwc4 bgr" (stride_x is not 1), the unaligned groups and the last group of a
                                                       row of the planar cases, the dtype cases at an odd base
  dword stores / byte stores                           3 channels: rows whose slot offset y x W x 3 is a multiple of 4 / the others (odd widths)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import device_image_model as dm
from line3d_amd import capi
from test_gpu_jpeg import DIST, SCENE, _caches, _check, _run, golden, wiring          # noqa: F401  (the fixtures and helpers of the wiring scene)

pytestmark = pytest.mark.gpu

INVALID = 1
ES = {dm.U8: 1, dm.U16: 2, dm.F16: 2, dm.F32: 4}
WIDTHS, HEIGHTS = (1, 3, 15, 16, 17, 63, 64, 65, 257), (1, 2, 9)


def _to_device(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


class Buf:
    """a flat buffer of elements on the device and its host copy; images are described inside it by element offsets"""
    def __init__(self, host, dtype):
        assert host.ndim == 1 and host.dtype == dm.NUMPY_DTYPE[dtype]
        self.host, self.dtype, self.dev = host, dtype, _to_device(host)
        torch.cuda.synchronize()

    def desc(self, base, w, h, channels, sy, sx, sc, chan=(0, 1, 2), scale=1.0):
        lo, hi = _span(w, h, channels, sy, sx, sc, chan)
        assert 0 <= base + lo and base + hi <= len(self.host), "the test's own image leaves its buffer"
        d = capi.DeviceImage()
        d.ptr = self.dev.data_ptr() + base * ES[self.dtype]
        d.width, d.height, d.channels, d.dtype = w, h, channels, self.dtype
        d.stride_y, d.stride_x, d.stride_c = sy, sx, sc
        d.chan[0], d.chan[1], d.chan[2] = chan
        d.scale = scale
        d._keep = self.dev
        return d

    def want(self, base, w, h, channels, sy, sx, sc, chan=(0, 1, 2), scale=1.0):
        return dm.ingest(self.host, base, w, h, channels, sy, sx, sc, chan, scale)


def _span(w, h, channels, sy, sx, sc, chan):
    lo = min(0, (h - 1) * sy) + min(0, (w - 1) * sx)
    hi = max(0, (h - 1) * sy) + max(0, (w - 1) * sx)
    cs = [0] if channels == 1 else [c * sc for c in chan]
    return lo + min(cs), hi + max(cs) + 1


def _layouts(w, h):
    """name -> (base, w, h, channels, sy, sx, sc, chan) inside a buffer of _room(w, h) elements"""
    p3, p1 = w * 3 + 7, w + 7                   # odd pitches: no multiple of 16, and the rows' alignments differ
    L = {
        "hwc1": (0, w, h, 1, w, 1, 0, (0, 1, 2)),
        "hwc3": (0, w, h, 3, w * 3, 3, 1, (0, 1, 2)),
        "hwc4": (0, w, h, 4, w * 4, 4, 1, (0, 1, 2)),
        "hwc4 bgr": (0, w, h, 4, w * 4, 4, 1, (2, 1, 0)),
        "reversed": (0, w, h, 3, w * 3, 3, 1, (2, 1, 0)),
        "chw": (0, w, h, 3, w, 1, w * h, (0, 1, 2)),
        "chw reversed": (0, w, h, 3, w, 1, w * h, (2, 1, 0)),
        "broadcast": (0, w, h, 3, w, 1, 0, (0, 1, 2)),
        "flipped": ((h - 1) * w * 3, w, h, 3, -w * 3, 3, 1, (0, 1, 2)),
        "image 1 of N": (h * w * 3, w, h, 3, w * 3, 3, 1, (0, 1, 2)),
        "image 2 of N": (2 * h * w * 3, w, h, 3, w * 3, 3, 1, (0, 1, 2)),
        "pitch+16 at 0": (0, w, h, 3, w * 3 + 16, 3, 1, (0, 1, 2)),
        "pitch+16 at 4": (4, w, h, 3, w * 3 + 16, 3, 1, (0, 1, 2)),
        "grey crop": (5, w, h, 1, p1, 1, 0, (0, 1, 2)),
    }
    for k in (1, 2, 3):
        L["crop at %d" % k] = (k, w, h, 3, p3, 3, 1, (0, 1, 2))
    return L


def _room(w, h):
    return 4 * (h + 1) * (w * 4 + 16) + 64


@pytest.fixture(scope="module")
def noise():
    return Buf(np.random.default_rng(11).integers(0, 256, size=_room(max(WIDTHS), max(HEIGHTS)), dtype=np.uint8), dm.U8)


@pytest.mark.parametrize("h", HEIGHTS)
def test_ingest_layouts_of_8_bit_images(gpu_ctx, noise, h):
    for w in WIDTHS:
        for name, args in _layouts(w, h).items():
            got = gpu_ctx.test_device_ingest([noise.desc(*args)])
            want = noise.want(*args)
            assert got.shape == (1,) + want.shape, (name, w, h)
            assert got[0].tobytes() == want.tobytes(), "%s at %dx%d: %d bytes differ" % (name, w, h, int((got[0] != want).sum()))


def test_ingest_five_layouts_in_one_chunk(gpu_ctx, noise):
    for w, h in ((17, 9), (64, 2), (257, 9), (3, 1)):
        L = _layouts(w, h)
        names = ["hwc3", "chw", "reversed", "hwc4 bgr", "flipped"]
        got = gpu_ctx.test_device_ingest([noise.desc(*L[n]) for n in names])
        for k, n in enumerate(names):
            assert got[k].tobytes() == noise.want(*L[n]).tobytes(), (n, w, h)
        grey = ["hwc1", "grey crop", "hwc1", "grey crop", "hwc1"]
        got = gpu_ctx.test_device_ingest([noise.desc(*L[n]) for n in grey])
        for k, n in enumerate(grey):
            assert got[k].tobytes() == noise.want(*L[n]).tobytes(), (n, w, h)


def test_ingest_corner_table(gpu_ctx):
    """every row of the model's corner table as a one-row grey image: at base 0 (vector loads for the whole groups, element loads for the tail) and at
    an odd base (element loads throughout) -- against the table's hand-written bytes and against the model"""
    for dtype, raw, scale, want in dm.CORNERS:
        buf = Buf(np.concatenate([raw[:1], raw, raw[:3]]), dtype)
        for base in (0, 1):
            w = len(raw) if base else len(raw) + 1
            expect = want if base else want[:1] + want
            args = (base, w, 1, 1, w, 1, 0)
            got = gpu_ctx.test_device_ingest([buf.desc(*args, scale=scale)])
            assert got.reshape(-1).tolist() == expect, (dtype, scale, base)
            assert got[0].tobytes() == buf.want(*args, scale=scale).tobytes()


@pytest.mark.parametrize("dtype", [dm.U16, dm.F16, dm.F32])
def test_ingest_dtypes_on_noise(gpu_ctx, dtype):
    rng = np.random.default_rng(20 + dtype)
    n = _room(65, 9)
    if dtype == dm.U16:
        host, scales = rng.integers(0, 65536, size=n, dtype=np.uint16), (1.0 / 257.0, 0.01)
    else:       # around [0, 1] with values outside it, halves after the scale, and a few specials
        host = (rng.integers(-80, 600, size=n) / 510.0).astype(dm.NUMPY_DTYPE[dtype])
        host[::97] = np.nan
        host[5::101] = np.inf
        host[7::103] = -np.inf
        scales = (255.0, 1.0)
    buf = Buf(host, dtype)
    for w, h in ((1, 1), (15, 2), (16, 9), (65, 9)):
        L = _layouts(w, h)
        for name in ("hwc1", "hwc3", "hwc4 bgr", "chw", "broadcast", "grey crop", "crop at 1", "flipped", "image 1 of N"):
            for scale in scales:
                got = gpu_ctx.test_device_ingest([buf.desc(*L[name], scale=scale)])
                assert got[0].tobytes() == buf.want(*L[name], scale=scale).tobytes(), (name, w, h, scale)
    L = _layouts(17, 9)
    names = ["hwc3", "chw", "reversed", "hwc4", "flipped"]
    got = gpu_ctx.test_device_ingest([buf.desc(*L[n], scale=scales[0]) for n in names])
    for k, n in enumerate(names):
        assert got[k].tobytes() == buf.want(*L[n], scale=scales[0]).tobytes(), n


# ---- egress
def test_decode_jpeg_on_the_device_equals_the_host_decode(gpu_ctx, golden):
    cases, _ = golden
    for n in ("17x9_420", "37x29_grey", "264x24_444"):
        data, pixels = cases[n]
        host = gpu_ctx.decode_jpeg(data)
        _check(host, pixels, n)
        got = gpu_ctx.decode_jpeg(data, device=True)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == host.shape
        _check(got.cpu().numpy(), host, n + " on the device")


def test_decode_jpeg_into_dtypes_layouts_and_crops(gpu_ctx, golden):
    """l3d_decode_jpeg_device into f32, f16, u16, planar and a strided crop: the whole buffer equals the model's egress applied to the host decode, so
    the elements outside the described image are untouched (the buffers are pre-filled with a pattern)"""
    cases, _ = golden
    for n in ("17x9_420", "37x29_grey", "264x24_444"):
        data = cases[n][0]
        host = gpu_ctx.decode_jpeg(data)
        h, w = host.shape[:2]
        grey = host.ndim == 2
        C3 = 1 if grey else 3
        outs = [("f32", dm.F32, 1.0 / 255.0), ("f16", dm.F16, 1.0 / 255.0), ("u16", dm.U16, 257.0), ("u16 clamped", dm.U16, 1000.0), ("u8", dm.U8, 1.0)]
        for name, dtype, scale in outs:
            npdt = dm.NUMPY_DTYPE[dtype]
            pitch = w * 4 + 5                       # a crop inside rows of 4-channel pixels, 2 rows and 1 pixel in
            fill = (np.arange((h + 3) * pitch) % 251).astype(npdt)
            layouts = [("hwc", 0, C3, w * C3, C3, 1, (0, 1, 2))]
            if not grey:
                layouts += [("planar", 0, 3, w, 1, w * h, (0, 1, 2)), ("crop of 4 channels, bgr", 2 * pitch + 4, 4, pitch, 4, 1, (2, 1, 0)),
                            ("flipped", (h - 1) * w * 3, 3, -w * 3, 3, 1, (0, 1, 2))]
            else:
                layouts += [("grey crop", 2 * pitch + 3, 1, pitch, 1, 0, (0, 1, 2)), ("grey, every second column", 1, 1, 2 * w + 3, 2, 0, (0, 1, 2))]
            for lname, base, channels, sy, sx, sc, chan in layouts:
                buf = Buf(fill.copy(), dtype)
                gpu_ctx.decode_jpeg_into(data, buf.desc(base, w, h, channels, sy, sx, sc, chan, scale))
                want = dm.egress(fill.copy(), base, host, channels, sy, sx, sc, chan, scale, dtype)
                got = buf.dev.cpu().numpy().view(npdt)
                assert got.tobytes() == want.tobytes(), "%s into %s, %s: %d elements differ" % (n, name, lname, int((got.view(np.uint8) != want.view(np.uint8)).sum()))


# ---- detector
@pytest.fixture(scope="module")
def views(gpu_ctx, golden):
    """view0..view3 of the fixture (320 x 200 x 3, the pixels stored in it), what the host call finds in each, and the images as device tensors"""
    images = [golden[0]["view%d" % k][1] for k in range(4)]
    assert images[0].shape == (200, 320, 3)
    single = [gpu_ctx.detect_segments(img) for img in images]
    assert min(len(s) for s in single) > 0
    return images, single, [torch.from_numpy(img).cuda() for img in images]


def test_detect_segments_on_device_tensors(gpu_ctx, views):
    images, single, tensors = views
    cam = (250.0, 250.0, 160.0, 100.0) + DIST
    for img, one, t in zip(images, single, tensors):
        assert gpu_ctx.detect_segments(t).tobytes() == one.tobytes()
        a, b = gpu_ctx.detect_segments(t, new_size=(240, 150), min_length=2.0, max_segments=50), gpu_ctx.detect_segments(img, new_size=(240, 150), min_length=2.0, max_segments=50)
        assert len(b) > 0 and a.tobytes() == b.tobytes()
        a, b = gpu_ctx.detect_segments(t, camera=cam), gpu_ctx.detect_segments(img, camera=cam)
        assert len(b) > 0 and a.tobytes() == b.tobytes() and b.tobytes() != one.tobytes()
    # the f32 C x H x W version of the same image ingests to the same bytes: x / 255 at scale 255 (asserted on the model first)
    img = images[0]
    planar = np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    assert dm.ingest(planar, 0, 320, 200, 3, 320, 1, 320 * 200, scale=255.0).tobytes() == img.tobytes()
    d = capi.device_image(torch.from_numpy(planar).cuda(), layout="CHW")
    assert d.scale == 255.0 and d.dtype == capi.F32
    assert gpu_ctx.test_device_ingest([d])[0].tobytes() == img.tobytes()
    assert gpu_ctx.detect_segments(d).tobytes() == single[0].tobytes()
    # a grey view of it (a strided H x W tensor: the green channel) and an 8x8 image
    green = tensors[0][:, :, 1]
    assert gpu_ctx.detect_segments(green).tobytes() == gpu_ctx.detect_segments(np.ascontiguousarray(img[:, :, 1])).tobytes()
    small = np.kron(np.array([[30, 220], [220, 30]], np.uint8), np.ones((4, 4), np.uint8))
    assert gpu_ctx.detect_segments(torch.from_numpy(small).cuda(), min_length=0.0).tobytes() == gpu_ctx.detect_segments(small, min_length=0.0).tobytes()


def test_detect_segments_batch_on_device_tensors(gpu_ctx, views):
    images, single, tensors = views
    flipped_host = [np.ascontiguousarray(img[:, :, ::-1]) for img in images]
    flipped_single = [gpu_ctx.detect_segments(img) for img in flipped_host]
    assert flipped_single[0].tobytes() != single[0].tobytes()                       # (the channel order matters to the grey weights)
    batch = list(tensors) + [capi.device_image(t, chan=(2, 1, 0)) for t in tensors]
    want = single + flipped_single
    gpu_ctx.profile_enable(True)
    gpu_ctx.set_option("L3D_DET_BATCH_IMAGES", 2)
    try:
        gpu_ctx.profile_reset()
        got = gpu_ctx.detect_segments_batch(batch)
        assert gpu_ctx.profile_get("k_det_ingest")[0] == 4                           # eight images of one plan in chunks of 2: one launch per chunk
        gpu_ctx.profile_reset()
        host = gpu_ctx.detect_segments_batch(images + flipped_host)
        assert gpu_ctx.profile_get("k_det_ingest")[0] == 0                           # a host-only batch ingests nothing
        gpu_ctx.set_option("L3D_DET_BATCH_IMAGES", 0)
        gpu_ctx.profile_reset()
        whole = gpu_ctx.detect_segments_batch(batch[::-1], cameras=[None, (250.0, 250.0, 160.0, 100.0) + DIST] * 4)
        assert gpu_ctx.profile_get("k_det_ingest")[0] == 1
    finally:
        gpu_ctx.profile_enable(False)
        gpu_ctx.set_option("L3D_DET_BATCH_IMAGES", 0)
    for k in range(8):
        assert got[k].tobytes() == want[k].tobytes() == host[k].tobytes(), k
    alone = [gpu_ctx.detect_segments(b, camera=c) for b, c in zip(batch[::-1], [None, (250.0, 250.0, 160.0, 100.0) + DIST] * 4)]
    for k in range(8):
        assert whole[k].tobytes() == alone[k].tobytes(), k
    assert gpu_ctx.detect_segments_batch([]) == []


# ---- undistortion
def test_undistort_on_device_tensors(gpu_ctx, views):
    images, _, tensors = views
    K = np.array([[250.0, 0, 160], [0, 250.0, 100], [0, 0, 1]])
    for img, t in ((images[0], tensors[0]), (np.ascontiguousarray(images[1][:, :, 2]), tensors[1][:, :, 2])):
        want = gpu_ctx.undistort(img, K, *DIST)
        assert not np.array_equal(want, img)
        got = gpu_ctx.undistort(t, K, *DIST)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.device == t.device and tuple(got.shape) == img.shape
        _check(got.cpu().numpy(), want, "undistort on the device")
        _check(gpu_ctx.undistort(t, K, 0.0, 0.0).cpu().numpy(), img, "zero coefficients")
    # in place: in and out describe the same memory
    work = tensors[2].clone()
    d = capi.device_image(work)
    gpu_ctx._chk(gpu_ctx.lib.l3d_undistort_image_device(gpu_ctx.h, C.byref(d), C.c_double(250.0), C.c_double(250.0), C.c_double(160.0), C.c_double(100.0),
                                                        C.c_double(DIST[0]), C.c_double(DIST[1]), C.byref(d)))
    _check(work.cpu().numpy(), gpu_ctx.undistort(images[2], K, *DIST), "undistort in place")
    # planar float in, the same layout in 8 bits out
    planar = torch.from_numpy(np.ascontiguousarray(images[0].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)).cuda()
    got = gpu_ctx.undistort(capi.device_image(planar, layout="CHW"), K, *DIST)
    assert tuple(got.shape) == (3, 200, 320)
    _check(got.cpu().numpy().transpose(1, 2, 0), gpu_ctx.undistort(images[0], K, *DIST), "planar")


# ---- the add family on the wiring scene
def _adders(images, dist, store=False, worldpoints=False):
    if worldpoints:
        return lambda l, v: l.add_image_pixels(v["id"], images[v["id"]], v["K"], v["R"], v["t"], list(range(10)), loadAndStoreSegments=store, dist=dist)
    return lambda l, v: l.add_image_pixels_fixed_sim(v["id"], images[v["id"]], v["K"], v["R"], v["t"], v["sims"], loadAndStoreSegments=store, dist=dist)


@pytest.fixture(scope="module")
def on_device(wiring):
    return {i: torch.from_numpy(img).cuda() for i, img in wiring[2].items()}


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in _caches(d)}


def test_add_image_pixels_takes_device_tensors(gpu_ctx, wiring, on_device, tmp_path):
    scene, files, images, n_segs = wiring
    host_dir, dev_dir = tmp_path / "host", tmp_path / "dev"
    host_dir.mkdir(), dev_dir.mkdir()
    for dist in (None, DIST):
        ref = _run(scene, n_segs, dist, _adders(images, dist), host_dir)
        assert ref[1] > 0
        assert _run(scene, n_segs, dist, _adders(on_device, dist), dev_dir) == ref
        assert _run(scene, n_segs, dist, _adders(on_device, dist, worldpoints=True), dev_dir) == _run(scene, n_segs, dist, _adders(images, dist, worldpoints=True), host_dir)
        assert _caches(host_dir) == _caches(dev_dir) == []
    # the caches the two forms write are the same files
    assert _run(scene, n_segs, DIST, _adders(images, DIST, store=True), host_dir) == _run(scene, n_segs, DIST, _adders(on_device, DIST, store=True), dev_dir)
    written = _files(dev_dir)
    assert len(written) == len(scene.views) and written == _files(host_dir)


def test_add_device_images_on_a_node_object_and_in_one_call(gpu_ctx, wiring, on_device, tmp_path):
    from line3d_amd.pipeline import Line3D
    from test_gpu_undistort import _model_bytes
    scene, files, images, n_segs = wiring
    for dist in (None, DIST):
        assert _run(scene, n_segs, dist, _adders(on_device, dist), tmp_path, devices=[0, 0]) == _run(scene, n_segs, dist, _adders(images, dist), tmp_path, devices=[0, 0])
        ref = _run(scene, n_segs, dist, _adders(on_device, dist), tmp_path)
        for src in (on_device, images):
            l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
            try:
                l3d.keep_view_matches(True)
                entries = [dict(imageID=v["id"], img=src[v["id"]], K=v["K"], R=v["R"], t=v["t"], viewSimilarity=v["sims"], dist=dist) for v in scene.views]
                assert l3d.add_images(entries, loadAndStoreSegments=False) == [0] * len(entries)
                assert l3d.numCameras() == len(scene.views)
                l3d.compute3Dmodel(False)
                assert _model_bytes(l3d, scene, {v["id"]: n_segs[(v["id"], dist)] for v in scene.views}) == ref
            finally:
                l3d.close()


class _HostAddress:
    """a numpy array's address dressed as a device object: what a confused caller would pass"""
    def __init__(self, a):
        self.a = a
        self.__cuda_array_interface__ = dict(shape=a.shape, typestr="|u1", data=(a.ctypes.data, False), version=3, strides=None)


def test_a_wanted_cache_stands_in_for_the_device_image(gpu_ctx, wiring, on_device, tmp_path):
    """with a cache present and wanted the image's memory is never touched and never checked: an entry whose ptr is a HOST address adds its view.
    Nothing is launched on it, so nothing can fault; where the detector would have to run the same entry is refused before any launch"""
    from line3d_amd.pipeline import Line3D
    scene, files, images, n_segs = wiring
    ref = _run(scene, n_segs, None, _adders(on_device, None, store=True), tmp_path)
    written = _files(tmp_path)
    assert len(written) == len(scene.views)
    hollow = {i: _HostAddress(img) for i, img in images.items()}
    assert _run(scene, n_segs, None, _adders(hollow, None, store=True), tmp_path) == ref
    assert _files(tmp_path) == written
    l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
    try:
        v = scene.views[0]
        assert not _adders(hollow, None, store=False)(l3d, v)                       # cache unwanted: the detector has to run, and the check refuses
        assert l3d.last_rc == INVALID and l3d.numCameras() == 0
        assert "not device memory" in l3d.lib.l3d_line3d_last_error(l3d.h).decode()
        assert _adders(on_device, None, store=False)(l3d, v) and l3d.numCameras() == 1
    finally:
        l3d.close()


def test_guards_speak_as_for_host_pixels(gpu_ctx, wiring, on_device, tmp_path):
    from line3d_amd.pipeline import Line3D
    scene, files, images, n_segs = wiring
    said = {}
    for kind, src in (("host", images), ("device", on_device)):
        l3d = Line3D(str(tmp_path) + os.sep, matchingNeighbors=6)
        try:
            v, u = scene.views[0], scene.views[1]
            err = lambda: (l3d.last_rc, l3d.lib.l3d_line3d_last_error(l3d.h).decode())
            assert _adders(src, None)(l3d, v)
            assert not _adders(src, None)(l3d, v)                                   # the id is in use
            said[kind] = [err()]
            assert not l3d.add_image_pixels(u["id"], src[u["id"]], u["K"], u["R"], u["t"], [], loadAndStoreSegments=False)      # no links
            said[kind].append(err())
            assert l3d.add_images([dict(imageID=v["id"], img=src[v["id"]], K=v["K"], R=v["R"], t=v["t"], worldpointIDs=[1, 2]),
                                   dict(imageID=u["id"], img=src[u["id"]], K=u["K"], R=u["R"], t=u["t"], worldpointIDs=[])], loadAndStoreSegments=False) == [1, 1]
            said[kind].append(l3d.lib.l3d_line3d_last_error(l3d.h).decode())
            assert l3d.numCameras() == 1
        finally:
            l3d.close()
    assert said["device"] == said["host"]
    assert "already in use" in said["host"][0][1] and "unlinked" in said["host"][1][1]


def test_reconstruct_from_images_takes_tensors(gpu_ctx, wiring, on_device, tmp_path):
    from line3d_amd import sfm
    scene, files, images, n_segs = wiring
    ids = [v["id"] for v in scene.views]
    cams = [dict(name="img%d.jpg" % v["id"], focal=250.0, dist=np.array([-DIST[0], 0.0]), cv_dist=np.array(DIST), R=v["R"], t=v["t"],
                 worldpoints=np.arange(10, dtype=np.uint32)) for v in scene.views]
    got = {}
    loaders = (("arrays", lambda i, name: images[ids[i]]), ("tensors", lambda i, name: on_device[ids[i]]),
               ("both", lambda i, name: (on_device if i % 3 else images)[ids[i]]))
    for kind, load in loaders:
        l3d = sfm.reconstruct_from_images(sfm.SfmScene(cams, 10), load, str(tmp_path) + os.sep, neighbors=6, load_and_store_segments=False)
        try:
            assert l3d.numCameras() == len(ids)
            got[kind] = b"".join(np.array([l3d.getSegment2D(k, s) for s in range(n_segs[(i, DIST)])], np.float32).tobytes() for k, i in enumerate(ids))
        finally:
            l3d.close()
    assert got["tensors"] == got["arrays"] == got["both"] and len(got["arrays"]) > 0


# ---- refusals: the pointer check's hook and the field checks of the public calls only
def test_refusals_leave_the_context_usable(gpu_ctx, golden, views):
    images, single, tensors = views
    good = lambda: gpu_ctx.detect_segments(tensors[0]).tobytes() == single[0].tobytes()
    host = np.zeros((64, 64, 3), np.uint8)
    rc, msg = gpu_ctx.test_device_image_pointer(capi.device_image(_HostAddress(host)))
    assert rc == INVALID and "not device memory" in msg and good()
    # a dedicated allocation: past everything the caching allocator keeps in one block, after the cache was emptied
    torch.cuda.empty_cache()
    big = torch.zeros(48 << 20, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    inside = capi.DeviceImage()
    inside.ptr, inside.width, inside.height, inside.channels, inside.dtype = big.data_ptr(), 4096, 4096, 3, capi.U8
    inside.stride_y, inside.stride_x, inside.stride_c = 4096 * 3, 3, 1
    inside.chan[0], inside.chan[1], inside.chan[2] = 0, 1, 2
    assert gpu_ctx.test_device_image_pointer(inside) == (0, "")                     # 48 MiB exactly
    past = capi.DeviceImage.from_buffer_copy(inside)
    past.height = 3 * 4096                                                          # three times the allocation
    rc, msg = gpu_ctx.test_device_image_pointer(past)
    assert rc == INVALID and "allocation" in msg and str(3 * (48 << 20)) in msg and good()
    before = capi.DeviceImage.from_buffer_copy(inside)
    before.stride_y = -4096 * 3                                                     # rows going down from the first: they start before the allocation
    rc, msg = gpu_ctx.test_device_image_pointer(before)
    assert rc == INVALID and "allocation" in msg and "-" in msg and good()
    del big
    # fields, through the public calls (refused before the memory is looked at)
    t = tensors[0]
    bad = []
    for field, value, word in (("dtype", 7, "dtype"), ("channels", 2, "channels"), ("scale", float("nan"), "scale")):
        d = capi.device_image(t.float() if field == "scale" else t)
        setattr(d, field, value)
        bad.append((d, word))
    d = capi.device_image(t)
    d.chan[1] = 3
    bad.append((d, "chan"))
    for d, word in bad:
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.detect_segments(d)
        assert e.value.code == INVALID and word in str(e.value), (word, str(e.value))
        segs, statuses = gpu_ctx.detect_segments_batch([tensors[1], d, tensors[0]], return_status=True)
        assert statuses == [0, INVALID, 0] and segs[0].tobytes() == single[1].tobytes() and segs[2].tobytes() == single[0].tobytes() and len(segs[1]) == 0
        assert "entry 1: " in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode() and word in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode()
        assert good()
    # a host address inside a batch fails alone (the pointer check comes before the chunk's launch)
    segs, statuses = gpu_ctx.detect_segments_batch([tensors[1], _HostAddress(np.zeros((200, 320, 3), np.uint8)), tensors[0]], return_status=True)
    assert statuses == [0, INVALID, 0] and segs[0].tobytes() == single[1].tobytes() and segs[2].tobytes() == single[0].tobytes()
    assert "not device memory" in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode()
    # below 8x8: the detector's own words
    with pytest.raises(capi.L3DError) as e1:
        gpu_ctx.detect_segments(t[:7, :23])
    with pytest.raises(capi.L3DError) as e2:
        gpu_ctx.detect_segments(np.ascontiguousarray(images[0][:7, :23]))
    assert e1.value.code == e2.value.code == INVALID and str(e1.value) == str(e2.value) and good()
    # l3d_decode_jpeg_device with a size that is not the file's
    data = golden[0]["17x9_420"][0]
    for shape in ((9, 16, 3), (8, 17, 3), (9, 17)):
        with pytest.raises(capi.L3DError) as e:
            gpu_ctx.decode_jpeg_into(data, torch.zeros(shape, dtype=torch.uint8, device="cuda:0"))
        assert e.value.code == INVALID and "17x9" in str(e.value)
    _check(gpu_ctx.decode_jpeg(data, device=True).cpu().numpy(), golden[0]["17x9_420"][1], "after the refusals")
    assert good()


# ---- stream order
def test_stream_order(gpu_ctx, golden, views):
    """the pixels are written on a side stream that is still busy when the call is made: four 8192^3 f32 matrix products (4.4 TFLOP together, some
    tens of milliseconds on an MI355X) are enqueued in front of the copy, and detect_segments is called at once, without a synchronise.  The
    library's event wait on the image's stream makes it see the pixels.  (A correct implementation passes every time; without the wait the test
    fails only when the stream is in fact still busy -- accepted.)  Then the reverse: an output is readable from another stream on return"""
    images, single, tensors = views
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(8192, 8192, device="cuda:0")
    target = torch.zeros_like(tensors[0])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            a = (a @ a) * 1e-3
        target.copy_(tensors[0], non_blocking=True)
        d = capi.device_image(target)
        assert d.stream == side.cuda_stream
        got = gpu_ctx.detect_segments(d)
    assert got.tobytes() == single[0].tobytes()
    torch.cuda.synchronize()
    data, pixels = golden[0]["264x24_444"]
    out = gpu_ctx.decode_jpeg(data, device=True)
    with torch.cuda.stream(other):
        seen = out.clone()
    other.synchronize()
    _check(seen.cpu().numpy(), pixels, "read on another stream")
