"""Images in device memory, the parts that need no device: the structs against the header, l3d_device_image_check and l3d_device_image_extent
(pure host functions of the library), capi.device_image on fake objects with a hand-written __cuda_array_interface__ (any integer as pointer:
nothing dereferences it), the mixed-list refusals, and the numpy model of the conversion rule on its own corner table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import device_image_model as dm
from line3d_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5


def _desc(width=16, height=8, channels=3, dtype=capi.U8, sy=None, sx=None, sc=1, chan=(0, 1, 2), scale=1.0, ptr=0x10000):
    d = capi.DeviceImage()
    d.ptr, d.width, d.height, d.channels, d.dtype = ptr, width, height, channels, dtype
    d.stride_x = channels if sx is None else sx
    d.stride_y = width * d.stride_x if sy is None else sy
    d.stride_c = sc
    d.chan[0], d.chan[1], d.chan[2] = chan
    d.scale = scale
    return d


class Fake:
    """an object with __cuda_array_interface__ and nothing else"""
    def __init__(self, shape, typestr="|u1", strides=None, ptr=0x7000, stream=None):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), version=3, strides=strides)
        if stream is not None:
            self.__cuda_array_interface__["stream"] = stream


def test_struct_layouts_of_the_device_forms(tmp_path):
    names = [("l3d_device_image", capi.DeviceImage, ("ptr", "width", "height", "channels", "dtype", "stride_y", "stride_x", "stride_c", "chan", "scale", "stream")),
             ("l3d_detect_device_entry", capi.DetectDeviceEntry, ("image", "new_width", "new_height", "min_length", "max_segments", "camera")),
             ("l3d_device_entry", capi.DeviceEntry, ("image_id", "image", "K", "R", "t", "dist", "link_ids", "sims", "n_links"))]
    lines = []
    for cname, _, fields in names:
        lines.append('printf("%%zu ", sizeof(%s));' % cname)
        lines += ['printf("%%zu ", offsetof(%s, %s));' % (cname, f) for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\nint main(void) { %s printf("%%d %%d %%d %%d\\n", L3D_U8, L3D_U16, L3D_F16, L3D_F32); return 0; }\n'
                   % " ".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    want = []
    for _, cls, fields in names:
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f).offset for f in fields]
    assert got == want + [capi.U8, capi.U16, capi.F16, capi.F32], (got, want)
    assert (dm.U8, dm.U16, dm.F16, dm.F32) == (capi.U8, capi.U16, capi.F16, capi.F32)


def test_check_refusals_and_accepted_corners():
    for d, word in ((_desc(width=0), "1x1"), (_desc(height=0), "1x1"), (_desc(width=-3), "1x1"),
                    (_desc(channels=2), "channels"), (_desc(channels=5), "channels"), (_desc(channels=0), "channels"),
                    (_desc(dtype=4), "dtype"), (_desc(dtype=-1), "dtype"),
                    (_desc(chan=(0, 1, 3)), "chan"), (_desc(chan=(-1, 1, 2)), "chan"), (_desc(channels=4, chan=(4, 1, 0)), "chan"),
                    (_desc(dtype=capi.F32, scale=float("nan")), "scale"), (_desc(dtype=capi.F16, scale=float("inf")), "scale"),
                    (_desc(dtype=capi.U16, scale=float("-inf")), "scale")):
        rc, msg = capi.device_image_check(d)
        assert rc == INVALID and word in msg, (rc, msg, word)
    for d in (_desc(width=1, height=1), _desc(width=1, height=1, channels=1), _desc(channels=4, chan=(2, 1, 0)), _desc(channels=4, chan=(3, 3, 3)),
              _desc(sc=0), _desc(channels=1, chan=(9, 9, 9)),                     # chan is ignored for one channel
              _desc(scale=float("nan")),                                         # scale is ignored for U8
              _desc(dtype=capi.F32, scale=0.0), _desc(sy=-48), _desc(sy=0, sx=0, sc=0)):
        assert capi.device_image_check(d) == (0, "")
    assert capi.load_library().l3d_device_image_check(None, None, ctypes.c_size_t(0)) == INVALID


def _extent(width, height, channels, es, sy, sx, sc, chan):
    """the lowest and one past the highest byte offset, in Python integers"""
    lo = hi = 0
    for n, s in ((height - 1, sy), (width - 1, sx)):
        lo += min(0, n * s)
        hi += max(0, n * s)
    cs = [0] if channels == 1 else [c * sc for c in chan]
    return (lo + min(cs)) * es, (hi + max(cs) + 1) * es


@pytest.mark.parametrize("name,kw,es", [
    ("hwc", dict(width=17, height=9, channels=3), 1),
    ("hwc 4 channels, reversed", dict(width=17, height=9, channels=4, chan=(2, 1, 0)), 1),
    ("chw f32", dict(width=64, height=5, channels=3, dtype=capi.F32, sy=64, sx=1, sc=64 * 5), 4),
    ("crop", dict(width=15, height=7, channels=3, sy=3 * 100), 1),
    ("negative stride_y", dict(width=16, height=8, channels=3, sy=-48), 1),
    ("negative stride_x and stride_c", dict(width=16, height=8, channels=3, dtype=capi.U16, sy=64, sx=-3, sc=-1), 2),
    ("zero channel stride", dict(width=16, height=8, channels=3, sy=16, sx=1, sc=0), 1),
    ("all strides zero", dict(width=16, height=8, channels=3, sy=0, sx=0, sc=0, dtype=capi.F16), 2),
    ("grey", dict(width=33, height=2, channels=1, sy=40, sx=1), 1),
    ("1x1", dict(width=1, height=1, channels=3), 1),
    ("past 2^31", dict(width=1000, height=1000, channels=3, dtype=capi.F32, sy=3 * 1000 * 300), 4),
    ("past 2^40", dict(width=100, height=100, channels=1, dtype=capi.F32, sy=1 << 34, sx=1), 4),
    ("past 2^40, downwards", dict(width=100, height=100, channels=1, dtype=capi.U16, sy=-(1 << 35), sx=7), 2),
    ("just inside 2^62", dict(width=2, height=2, channels=1, sy=(1 << 62) - 2, sx=1), 1),
])
def test_extent_against_python_integers(name, kw, es):
    d = _desc(**kw)
    rc, lo, hi = capi.device_image_extent(d)
    assert rc == 0, name
    assert (lo, hi) == _extent(d.width, d.height, d.channels, es, d.stride_y, d.stride_x, d.stride_c, tuple(d.chan)), name
    if name == "negative stride_y":
        assert lo == -7 * 48 and hi == 48            # the first row is the highest address
    if name == "past 2^31":
        assert hi > 1 << 31
    if name.startswith("past 2^40"):
        assert max(hi, -lo) > 1 << 40


def test_extent_refusals():
    # a product that leaves 2^62, the sum that leaves it in bytes, an image past the detector's 2^31 values, fields the check refuses
    assert capi.device_image_extent(_desc(width=2, height=3, channels=1, sy=1 << 62, sx=1))[0] == UNSUPPORTED
    assert capi.device_image_extent(_desc(width=2, height=3, channels=1, sy=-(1 << 62), sx=1))[0] == UNSUPPORTED
    assert capi.device_image_extent(_desc(width=2, height=2, channels=1, dtype=capi.F32, sy=(1 << 61), sx=1))[0] == UNSUPPORTED
    assert capi.device_image_extent(_desc(width=1 << 20, height=1 << 10, channels=1, sy=0, sx=0))[0] == UNSUPPORTED      # 2^30 x 3 > 2^31
    assert capi.device_image_extent(_desc(width=26754, height=26754, channels=1, sy=0, sx=0))[0] == 0                     # 715776516 x 3 <= 2^31
    assert capi.device_image_extent(_desc(channels=2))[0] == INVALID


def test_device_image_strides_dtypes_and_layouts():
    d = capi.device_image(Fake((9, 17, 3)))
    assert (d.width, d.height, d.channels, d.dtype) == (17, 9, 3, capi.U8)
    assert (d.stride_y, d.stride_x, d.stride_c) == (51, 3, 1) and tuple(d.chan) == (0, 1, 2) and d.scale == 1.0 and d.ptr == 0x7000 and d.stream is None
    d = capi.device_image(Fake((9, 17), "<f4", strides=(17 * 4 * 2, 8)))            # every second element of every second row
    assert (d.width, d.height, d.channels, d.dtype) == (17, 9, 1, capi.F32) and (d.stride_y, d.stride_x) == (34, 2) and d.scale == 255.0
    d = capi.device_image(Fake((3, 9, 17), "<f2"), layout="CHW")
    assert (d.width, d.height, d.channels, d.dtype) == (17, 9, 3, capi.F16) and (d.stride_y, d.stride_x, d.stride_c) == (17, 1, 9 * 17) and d.scale == 255.0
    d = capi.device_image(Fake((9, 17, 4), "<u2"), chan=(2, 1, 0))
    assert d.channels == 4 and d.dtype == capi.U16 and tuple(d.chan) == (2, 1, 0) and d.scale == np.float32(1.0 / 257.0)
    assert (d.stride_y, d.stride_x, d.stride_c) == (68, 4, 1)
    # ambiguous: H x W x C unless told otherwise
    d = capi.device_image(Fake((3, 5, 3)))
    assert (d.width, d.height, d.channels) == (5, 3, 3) and (d.stride_y, d.stride_x, d.stride_c) == (15, 3, 1)
    d = capi.device_image(Fake((3, 5, 3)), layout="CHW")
    assert (d.width, d.height, d.channels) == (3, 5, 3) and (d.stride_y, d.stride_x, d.stride_c) == (3, 1, 15)
    d = capi.device_image(Fake((9, 17, 1)))
    assert d.channels == 1
    # a negative byte stride (a flipped view), an explicit scale, a stream from the interface and one given
    d = capi.device_image(Fake((9, 17), "<u2", strides=(-34, 2), stream=0x55), scale=0.25)
    assert (d.stride_y, d.stride_x) == (-17, 1) and d.scale == 0.25 and d.stream == 0x55
    assert capi.device_image(Fake((9, 17), stream=1)).stream is None                # the interface's legacy default stream
    assert capi.device_image(Fake((9, 17)), stream=0x66).stream == 0x66
    obj = Fake((9, 17))
    assert capi.device_image(obj)._keep is obj                                       # kept alive on the descriptor
    assert capi.device_image(d) is d
    with pytest.raises(TypeError):
        capi.device_image(Fake((9, 17), "<f8"))
    with pytest.raises(TypeError):
        capi.device_image(Fake((9, 17), "<i4"))
    with pytest.raises(ValueError):
        capi.device_image(Fake((9, 17), "<f4", strides=(70, 4)))                     # 70 bytes are no whole floats
    with pytest.raises(ValueError):
        capi.device_image(Fake((9, 17), "<u2", strides=(34, 1)))
    with pytest.raises(ValueError):
        capi.device_image(Fake((3, 9, 17)))                                          # planar needs layout="CHW"
    with pytest.raises(ValueError):
        capi.device_image(Fake((2, 3, 9, 17)))
    # the library accepts what the binding builds
    assert capi.device_image_check(capi.device_image(Fake((9, 17, 4), "<f4"), chan=(2, 1, 0))) == (0, "")


def test_mixed_lists_are_refused_before_any_library_call():
    from line3d_amd.pipeline import Line3D
    host, dev = np.zeros((8, 8), np.uint8), Fake((8, 8))
    assert capi.is_device_object(dev) and not capi.is_device_object(host) and not capi.is_device_object(b"\xff\xd8")
    # no context and no object exist here: the refusal has to come before either is touched
    with pytest.raises(ValueError, match="mixes"):
        capi.Context.detect_segments_batch(None, [host, dev])
    with pytest.raises(ValueError, match="mixes"):
        capi.Context.detect_segments_batch(None, [dev, b"\xff\xd8\xff"])
    entry = lambda img, **kw: dict(imageID=1, img=img, K=np.eye(3), R=np.eye(3), t=np.zeros(3), worldpointIDs=[1, 2], **kw)
    with pytest.raises(ValueError, match="mixes"):
        Line3D.add_images(None, [entry(dev), entry(host)])
    with pytest.raises(ValueError, match="mixes"):
        Line3D.add_images(None, [dict(imageID=2, data=b"\xff\xd8", K=np.eye(3), R=np.eye(3), t=np.zeros(3), worldpointIDs=[1]), entry(dev)])
    assert capi.all_device_objects([dev, dev], "x") and not capi.all_device_objects([host, host], "x") and not capi.all_device_objects([], "x")


def test_model_on_its_corner_table():
    for dtype, raw, scale, want in dm.CORNERS:
        assert raw.dtype == dm.NUMPY_DTYPE[dtype]
        got = dm.to_u8(raw, scale)
        assert got.dtype == np.uint8 and got.tolist() == want, (dtype, scale, got.tolist(), want)
    # x / 255 at scale 255 gives x back for every byte (what lets a float tensor stand for an 8-bit image), in f32 and -- 8-bit values exceed its
    # 11 bits of precision only after the division -- not in f16
    b = np.arange(256, dtype=np.uint8)
    assert dm.to_u8(b.astype(np.float32) / np.float32(255), 255.0).tolist() == b.tolist()
    assert dm.to_u8(dm.from_u8(b, dm.F32, 1.0 / 255.0), 255.0).tolist() == b.tolist()
    assert dm.to_u8(dm.from_u8(b, dm.U16, 257.0), 1.0 / 257.0).tolist() == b.tolist()
    # egress corners
    assert dm.from_u8([0, 1, 255], dm.U16, 257.0).tolist() == [0, 257, 65535]
    assert dm.from_u8([0, 1, 255], dm.U16, 1000.0).tolist() == [0, 1000, 65535]
    assert dm.from_u8([0, 3, 255], dm.U16, -1.0).tolist() == [0, 0, 0]
    assert dm.from_u8([1, 3], dm.U16, 0.5).tolist() == [0, 2]                        # ties to even
    assert dm.from_u8([255], dm.F16, 1000.0).tolist() == [np.inf]
    assert dm.from_u8([255], dm.F16, 1.0 / 255.0).view(np.uint16).tolist() == [0x3c00]
    assert dm.from_u8([7], dm.F32, 0.1).view(np.uint32).tolist() == (np.float32(7) * np.float32(0.1)).reshape(1).view(np.uint32).tolist()


def test_model_layouts():
    rng = np.random.default_rng(5)
    hwc = rng.integers(0, 256, size=(6, 7, 3), dtype=np.uint8)
    assert np.array_equal(dm.ingest(hwc, 0, 7, 6, 3, 21, 3, 1), hwc)
    assert np.array_equal(dm.ingest(hwc, 0, 7, 6, 3, 21, 3, 1, chan=(2, 1, 0)), hwc[:, :, ::-1])
    chw = np.ascontiguousarray(hwc.transpose(2, 0, 1))
    assert np.array_equal(dm.ingest(chw, 0, 7, 6, 3, 7, 1, 42), hwc)
    assert np.array_equal(dm.ingest(hwc, 5 * 21, 7, 6, 3, -21, 3, 1), hwc[::-1])                              # flipped
    assert np.array_equal(dm.ingest(hwc, 21 + 3, 4, 3, 3, 21, 3, 1), hwc[1:4, 1:5])                           # a crop
    assert np.array_equal(dm.ingest(hwc[:, :, 0].copy(), 0, 7, 6, 3, 7, 1, 0), np.repeat(hwc[:, :, :1], 3, axis=2))      # one channel broadcast
    assert dm.ingest(hwc[:, :, 0].copy(), 0, 7, 6, 1, 7, 1, 0).shape == (6, 7, 1)
    out = np.full((6, 7, 4), 9, np.uint16)
    dm.egress(out, 0, hwc, 4, 28, 4, 1, chan=(2, 1, 0), scale=257.0, dtype=dm.U16)
    assert np.array_equal(out[:, :, :3], hwc[:, :, ::-1].astype(np.uint16) * 257) and np.all(out[:, :, 3] == 9)
