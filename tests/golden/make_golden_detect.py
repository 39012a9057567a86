"""Generates tests/golden/detect_ref.npz: seeded synthetic images (uint8) and what the REFERENCE's own line segment detector
(lsd/lsd.cpp, the von Gioi code) returns for them -- its 7-tuples (x1, y1, x2, y2, width, p, -log10 NFA).  Run in the build
container (needs the reference sources and g++): the detector is compiled from where it lies into a temporary directory and called
through ctypes; nothing of it is copied.  Data only goes into the npz.

    python tests/golden/make_golden_detect.py

For every noisy image the reference also runs on the same scene with the noise redrawn; `floor` is the worst single-image
agreement (tests/detect_metric.py) of the reference with itself over those pairs, both directions: the bar the GPU detector's pooled
recall and precision are held to."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import detect_metric as dm  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SS = 4                      # supersampling of the renderer


def build_reference(tmp):
    so = os.path.join(tmp, "liblsd_ref.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, os.path.join(REF, "lsd", "lsd.cpp")])
    lib = C.CDLL(so)
    fn = lib._Z3lsdPiPdii                                   # double* lsd(int* n_out, double* img, int X, int Y)
    fn.restype = C.POINTER(C.c_double)
    fn.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_int]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]

    def lsd(img_u8):
        img = np.ascontiguousarray(img_u8, dtype=np.float64)
        n = C.c_int(0)
        p = fn(C.byref(n), img.ctypes.data_as(C.POINTER(C.c_double)), img.shape[1], img.shape[0])
        out = np.ctypeslib.as_array(p, shape=(n.value, 7)).copy() if n.value else np.zeros((0, 7))
        libc.free(p)
        return out
    return lsd


def render_rects(rng, w, h, n_rect):
    """filled, rotated rectangles of random grey on a mid-grey ground, SS x supersampled -> float image"""
    W, H = w * SS, h * SS
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.full((H, W), 128.0, np.float32)
    for _ in range(n_rect):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        hw, hh = rng.uniform(W / 16, W / 4), rng.uniform(H / 16, H / 4)
        th = rng.uniform(0, np.pi)
        g = rng.uniform(20, 235)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img[(np.abs(u) <= hw) & (np.abs(v) <= hh)] = g
    return img.reshape(h, SS, w, SS).mean(axis=(1, 3))


def render_edge(w, h, deg, through=None):
    """one step edge (60 | 190) at `deg` degrees through the image centre (or the two corners: the full diagonal)"""
    W, H = w * SS, h * SS
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    if through == "diagonal":
        s = (xx + 0.5) * H - (yy + 0.5) * W
    else:
        t = np.deg2rad(deg)
        s = -(xx - W / 2 + 0.5) * np.sin(t) + (yy - H / 2 + 0.5) * np.cos(t)
    img = np.where(s > 0, 190.0, 60.0).astype(np.float32)
    return img.reshape(h, SS, w, SS).mean(axis=(1, 3))


def noisy(clean, rng, sigma):
    return np.clip(np.rint(clean + rng.normal(0.0, sigma, clean.shape)), 0, 255).astype(np.uint8)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lsd = build_reference(tmp)
        rng = np.random.default_rng(20240517)
        # ---- twelve noisy rectangle scenes: ten 320x240, two 640x480; sigma 2 (eight) and 4 (four)
        shapes = [(320, 240, 10)] * 10 + [(640, 480, 20)] * 2
        sigmas = [2, 2, 2, 2, 2, 2, 2, 4, 4, 4, 2, 4]
        refs_a, refs_b = [], []
        for i, ((w, h, n), s) in enumerate(zip(shapes, sigmas)):
            clean = render_rects(rng, w, h, n)
            a, b = noisy(clean, rng, s), noisy(clean, rng, s)
            out["img_noisy%02d" % i] = a
            out["ref_noisy%02d" % i] = lsd(a)
            out["refB_noisy%02d" % i] = lsd(b)                  # the same scene, noise redrawn (the image itself is not kept)
            refs_a.append(out["ref_noisy%02d" % i])
            refs_b.append(out["refB_noisy%02d" % i])
        out["n_noisy"] = np.int32(len(shapes))
        out["sigma"] = np.array(sigmas, np.int32)
        per_image = [(dm.cover(a, b), dm.cover(b, a)) for a, b in zip(refs_a, refs_b)]
        out["floor"] = np.float64(dm.reference_floor(refs_a, refs_b))
        out["repeatability"] = np.array(per_image)
        print("reference vs itself, per image:", np.round(np.array(per_image), 4).tolist())
        print("floor (worst single image) %.4f   pooled %.4f / %.4f" % (out["floor"], dm.pooled(zip(refs_a, refs_b)), dm.pooled(zip(refs_b, refs_a))))
        # ---- single edges, the full diagonal, an odd small image, a flat one (noise-free: they compress to nothing)
        for deg in (0, 90, 45, 7):
            out["img_edge%d" % deg] = np.rint(render_edge(200, 120, deg)).astype(np.uint8)
        out["img_diag"] = np.rint(render_edge(640, 480, 0, "diagonal")).astype(np.uint8)
        out["img_tiny"] = noisy(render_rects(rng, 37, 29, 2), rng, 2)
        out["img_flat"] = np.full((120, 200), 128, np.uint8)
        for k in ("edge0", "edge90", "edge45", "edge7", "diag", "tiny", "flat"):
            out["ref_" + k] = lsd(out["img_" + k])
            print(k, len(out["ref_" + k]), "segments")
        # ---- noisy11 as a 3-channel buffer: channel 0 / 2 = grey + a smooth signed offset (kept as int8: the test rebuilds the buffer),
        # and the same buffer rescaled to 320x240.  The stated integer formulas (detect_metric.rescale_u8 / grey_u8) make the reference's input.
        g = out["img_noisy11"].astype(np.int16)
        yy, xx = np.mgrid[0:480, 0:640]
        d0 = (24 * np.sin(xx / 97.0) * np.cos(yy / 61.0)).astype(np.int8)
        d2 = (-18 * np.cos(xx / 53.0 + yy / 89.0)).astype(np.int8)
        rgb = np.stack([np.clip(g + d0, 0, 255), g, np.clip(g + d2, 0, 255)], axis=-1).astype(np.uint8)
        out["rgb_d0"], out["rgb_d2"] = d0, d2
        out["ref_rgb"] = lsd(dm.grey_u8(rgb))
        out["ref_rescaled"] = lsd(dm.grey_u8(dm.rescale_u8(rgb, 320, 240)))       # coordinates of the 320x240 image
        print("rgb", len(out["ref_rgb"]), "rescaled", len(out["ref_rescaled"]))
        # ---- the reference's CPU time for one sparse 1920x1080 scene, on the machine that made this file
        big = noisy(render_rects(rng, 1920, 1080, 20), rng, 2)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            n_big = len(lsd(big))
            ts.append(time.perf_counter() - t0)
        out["ref_cpu_seconds_1080p"] = np.float64(sorted(ts)[1])
        print("reference, 1920x1080, %d segments: %.3f s (median of 3, this machine)" % (n_big, out["ref_cpu_seconds_1080p"]))
    path = os.path.join(HERE, "detect_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
