"""Writes tests/golden/jpeg_ref.npz: per case the bytes of a JPEG file and the pixels Pillow (libjpeg-turbo, JDCT_ISLOW, fancy upsampling) decodes
from them, stored B, G, R.  Needs Pillow; the tests that read the file do not.  Run from anywhere: python tests/golden/make_golden_jpeg.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from test_gpu_jpeg import SCENE  # noqa: E402  (the wiring scene the device tests rebuild)


def content(w, h, seed, grey=False):
    """gradients, a band of noise and saturated patches: every clamp and both rounding offsets are met"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255) // max(1, w - 1), (yy * 255) // max(1, h - 1), ((xx + yy) * 255) // max(1, w + h - 2)], axis=-1).astype(np.uint8)
    band = slice(h // 3, max(h // 3 + 1, h // 2))
    img[band] = rng.integers(0, 256, size=img[band].shape, dtype=np.uint8)
    patches = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 255, 255), (0, 0, 0)]
    pw, y0 = max(1, w // len(patches)), (2 * h) // 3
    for k, col in enumerate(patches):
        img[y0:, k * pw:(k + 1) * pw] = col
    return img[..., 1].copy() if grey else img


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def encode(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_pixels(data):
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    assert im.mode in ("L", "RGB"), im.mode
    return np.ascontiguousarray(a if a.ndim == 2 else a[..., ::-1])


def dqt16(data):
    """the first DQT segment (one 8-bit table) rewritten in 16-bit form"""
    at = data.index(b"\xff\xdb")
    ln = (data[at + 2] << 8) | data[at + 3]
    assert ln == 67 and data[at + 4] >> 4 == 0
    tq = data[at + 4] & 15
    body = b"".join(bytes([0, v]) for v in data[at + 5:at + 69])
    return data[:at] + b"\xff\xdb" + (2 + 1 + 128).to_bytes(2, "big") + bytes([0x10 | tq]) + body + data[at + 2 + ln:]


def scene_images():
    """the 320 x 200 views of a small synthetic scene (SCENE), drawn as tests/test_gpu_undistort.py draws them, tinted so that the three channels differ"""
    from line3d_amd.synth import make_scene
    from test_gpu_undistort import _draw
    scene = make_scene(SCENE["n_views"], SCENE["n_segments"], SCENE["n_neighbors"], **{k: v for k, v in SCENE.items() if k not in ("n_views", "n_segments", "n_neighbors")})
    out = []
    for v in scene.views:
        g = _draw(SCENE["width"], SCENE["height"], v["segments"]).astype(np.int32)
        out.append(np.stack([g, (g * 9) // 10, 255 - g // 2], axis=-1).astype(np.uint8))
    return scene, out


def cases():
    c = {}
    c["8x8_grey"] = encode(content(8, 8, 1, grey=True), quality=85)
    c["16x16_420"] = encode(content(16, 16, 2), quality=85, subsampling=2)
    c["1x1_420"] = encode(content(1, 1, 3), quality=85, subsampling=2)
    c["17x9_420"] = encode(content(17, 9, 4), quality=85, subsampling=2)
    c["7x23_422"] = encode(content(7, 23, 5), quality=85, subsampling=1)
    c["37x29_444"] = encode(content(37, 29, 6), quality=85, subsampling=0)
    c["37x29_422"] = encode(content(37, 29, 6), quality=85, subsampling=1)
    c["37x29_420"] = encode(content(37, 29, 6), quality=85, subsampling=2)
    c["37x29_grey"] = encode(content(37, 29, 6, grey=True), quality=85)
    c["50x33_420"] = encode(content(50, 33, 7), quality=85, subsampling=2)
    c["264x24_444"] = encode(content(264, 24, 8), quality=85, subsampling=0)
    c["noise_q100"] = encode(noise(40, 24, 9), quality=100, subsampling=2)
    c["noise_q5"] = encode(noise(40, 24, 10), quality=5, subsampling=2)
    c["const0"] = encode(np.zeros((19, 21, 3), np.uint8), quality=85, subsampling=2)
    c["const255"] = encode(np.full((19, 21, 3), 255, np.uint8), quality=85, subsampling=2)
    c["optimize"] = encode(content(37, 29, 11), quality=85, subsampling=2, optimize=True)
    c["restart_blocks1"] = encode(content(50, 33, 12), quality=85, subsampling=2, restart_marker_blocks=1)
    c["restart_rows1"] = encode(content(50, 33, 13), quality=85, subsampling=2, restart_marker_rows=1)
    c["keep_rgb"] = encode(content(37, 29, 14), quality=85, keep_rgb=True)
    d16 = dqt16(c["37x29_420"])
    if np.array_equal(pillow_pixels(d16), pillow_pixels(c["37x29_420"])):
        c["dqt16"] = d16
    else:
        print("Pillow decodes the 16-bit DQT variant differently: left out")
    for k, img in enumerate(scene_images()[1]):
        c["view%d" % k] = encode(img, quality=95)
    refusals = {"progressive": encode(content(37, 29, 15), quality=85, progressive=True),
                "cmyk": encode_cmyk(np.concatenate([content(16, 16, 16), content(16, 16, 17)[..., :1]], axis=-1))}
    return c, refusals


def encode_cmyk(img):
    buf = io.BytesIO()
    Image.fromarray(img, "CMYK").save(buf, "JPEG", quality=85)
    return buf.getvalue()


def build():
    c, refusals = cases()
    out = {"names": np.array(sorted(c)), "refusals": np.array(sorted(refusals))}
    for name, data in c.items():
        out[name + "/bytes"] = np.frombuffer(data, np.uint8)
        out[name + "/pixels"] = pillow_pixels(data)
    for name, data in refusals.items():
        out[name + "/bytes"] = np.frombuffer(data, np.uint8)
    return out


if __name__ == "__main__":
    out = build()
    path = os.path.join(HERE, "jpeg_ref.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d refusals, %d bytes" % (path, len(out["names"]), len(out["refusals"]), os.path.getsize(path)))
