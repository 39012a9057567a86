#!/usr/bin/env python3
"""Where the time of a JPEG image goes: host parse + entropy decode, upload, k_jpg_idct, k_jpg_assemble, and the whole l3d_detect_segments_jpeg call
beside l3d_detect_segments on the already decoded pixels.  Writes profiles/jpeg_times.txt.

    python scripts/time_jpeg.py a_640x480.jpg b_1920x1080.jpg [--out F]

The files are the caller's (any baseline JPEG; the recorded run used scenes of scripts/time_undistort.py at 640x480 and 1920x1080, quality 90,
4:2:0).  Protocol of scripts/time_undistort.py: warm-up first, then the two variants alternate image by image, so both see the same machine; each
timed call ends with the segments on the host; median and p10 / p90 are reported.  The host part is timed on its own through
l3d_test_jpeg_coefficients (parser and entropy decoder, no device); the upload and the two kernels come from a pass of their own with the library's
event brackets on, never from the timed pass."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = np.array(ms)
    return "median %7.2f ms   p10 %7.2f  p90 %7.2f   min %7.2f  max %7.2f" % (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90), ms.min(), ms.max())


def host_decode_ms(capi, data, warmup, images):
    """parser + entropy decoder alone, the C call only"""
    lib = capi.load_library()
    ptr, n = capi._bytes_arguments(data)
    qt, layout = np.zeros((3, 64), np.uint16), np.zeros(27, np.int32)
    ms = []
    for k in range(warmup + images):
        coef, nb = C.POINTER(C.c_int16)(), C.c_size_t(0)
        t0 = time.perf_counter()
        rc = lib.l3d_test_jpeg_coefficients(ptr, n, C.byref(coef), C.byref(nb), capi._p(qt), capi._p(layout))
        dt = (time.perf_counter() - t0) * 1e3
        lib.l3d_free(coef)
        if rc != 0:
            raise RuntimeError("not a file the decoder takes: %s" % lib.l3d_jpeg_last_error())
        if k >= warmup:
            ms.append(dt)
    return ms, nb.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_times.txt"))
    a = ap.parse_args()
    from line3d_amd import capi
    capi.load_library().l3d_jpeg_last_error.restype = C.c_char_p
    ctx = capi.Context(0)
    lines = ["baseline JPEG input, ms per image, warm-up %d, %d timed images per variant, variants alternating" % (a.warmup, a.images)]
    for path in a.files:
        data = open(path, "rb").read()
        w, h, ch = capi.jpeg_info(data)
        tag = "%dx%dx%d (%d bytes)" % (w, h, ch, len(data))
        img = ctx.decode_jpeg(data)
        variants = [("jpeg", lambda: ctx.detect_segments_jpeg(data)), ("pixels", lambda: ctx.detect_segments(img))]
        for _ in range(a.warmup):
            for _, f in variants:
                f()
        ms = {name: [] for name, _ in variants}
        for _ in range(a.images):
            for name, f in variants:
                t0 = time.perf_counter()
                f()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        lines.append("%s" % tag)
        lines.append("  detect_segments_jpeg (file bytes in)        %s" % stats(ms["jpeg"]))
        lines.append("  detect_segments (decoded pixels in)        %s" % stats(ms["pixels"]))
        host, n_blocks = host_decode_ms(capi, data, a.warmup, a.images)
        lines.append("  host parse + entropy decode, %6d blocks  %s" % (n_blocks, stats(host)))
        ctx.profile_enable(True)
        ctx.profile_only(None)
        ctx.detect_segments_jpeg(data)
        ctx.profile_reset()
        for _ in range(a.images):
            ctx.detect_segments_jpeg(data)
        for name, nbytes in (("jpg_upload", 512 + n_blocks * 128), ("k_jpg_idct", n_blocks * 192), ("k_jpg_assemble", n_blocks * 64 + w * h * ch)):
            n, total = ctx.profile_get(name)
            us = 1e3 * total / max(n, 1)
            lines.append("  %-15s %d brackets, %8.1f us each; %.2f MB moved: %.0f GB/s" % (name, n, us, nbytes * 1e-6, nbytes / (us * 1e-6) / 1e9 if us > 0 else 0.0))
        ctx.profile_enable(False)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        lines.append("  the JPEG call costs %.2f ms more than the pixel call; the host's parse + entropy decode is %.2f ms of that"
                     % (med["jpeg"] - med["pixels"], float(np.median(host))))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
