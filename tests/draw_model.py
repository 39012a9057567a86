"""The drawing rules of include/line3d_amd.h ("PROJECTION AND OVERLAYS", 2) in numpy: float64 for the clip, the distance and the coverage, int64 /
Python ints for the sixteenths and the blend.  Every pixel of a generous band around a segment is tested, 32 rows at a time (no walk, no pieces), the
winner of a pixel is the largest key (q << 24) | k.  Shares no code with the product."""
import numpy as np

import project_model as pm

F = np.float64


def stroke16(width_px):
    return int(np.rint(F(width_px) * F(16.0)))


def quantised(seg, W16, width, height):
    """the clipped segment in sixteenths (Python ints px, py, qx, qy), or None when it is dropped"""
    s = np.asarray(seg, np.float32)
    if not np.all(np.isfinite(s)):
        return None
    xP, yP, xQ, yQ = (F(v) for v in s)
    dx, dy = xQ - xP, yQ - yP
    margin = (W16 + 31) // 32 + 1
    tt = pm.clip(xP, yP, dx, dy, pm.rect(width, height, margin))
    if tt is None:
        return None
    t0, t1 = tt
    x0, y0 = (xP, yP) if t0 == 0 else (xP + t0 * dx, yP + t0 * dy)
    x1, y1 = (xQ, yQ) if t1 == 1 else (xP + t1 * dx, yP + t1 * dy)
    return tuple(int(np.rint(v * F(16.0))) for v in (x0, y0, x1, y1))


def coverage_box(g, W16, j0, j1, i0, i1):
    """q (int64 array, rows i0..i1, columns j0..j1) of the pixel centres against the quantised segment g"""
    px, py, qx, qy = g
    cx = (np.arange(j0, j1 + 1, dtype=np.int64) * 16)[None, :]
    cy = (np.arange(i0, i1 + 1, dtype=np.int64) * 16)[:, None]
    ax, ay, bx, by = cx - px, cy - py, qx - px, qy - py
    L2 = bx * bx + by * by
    dot = ax * bx + ay * by
    with np.errstate(all="ignore"):
        d_p = np.sqrt((ax * ax + ay * ay).astype(F))
        ex, ey = cx - qx, cy - qy
        d_q = np.sqrt((ex * ex + ey * ey).astype(F))
        rinv = F(1.0) / np.sqrt(F(L2)) if L2 > 0 else F(0.0)
        d_l = np.abs(ax * by - ay * bx).astype(F) * rinv
    d = np.where(dot <= 0, d_p, np.where(dot >= L2, d_q, d_l))
    R16 = F(W16) / F(2.0) + F(8.0)
    cov = np.clip((R16 - d) / F(16.0), 0.0, 1.0)
    return np.floor(cov * F(255.0) + F(0.5)).astype(np.int64)


def key_plane(shape, segments, width_px):
    """(h, w) int64: the winning key of every pixel, 0 where no segment covers it"""
    h, w = shape
    W16 = stroke16(width_px)
    plane = np.zeros((h, w), np.int64)
    reach = W16 // 32 + 3                       # pixels: more than R16 / 16 = W16 / 32 + 0.5
    for k, seg in enumerate(np.asarray(segments, np.float32).reshape(-1, 4)):
        g = quantised(seg, W16, w, h)
        if g is None:
            continue
        i0, i1 = max(0, min(g[1], g[3]) // 16 - reach), min(h - 1, max(g[1], g[3]) // 16 + reach + 1)
        # bands of 32 rows: within a band every pixel of the columns that the segment's part in the band (widened by the reach) spans
        for ia in range(i0, i1 + 1, 32):
            ib = min(i1, ia + 31)
            ylo, yhi = 16 * (ia - reach), 16 * (ib + reach)
            if g[1] == g[3]:
                xs = (g[0], g[2])
            else:
                ta, tb = sorted(((ylo - g[1]) / (g[3] - g[1]), (yhi - g[1]) / (g[3] - g[1])))
                ta, tb = max(0.0, ta), min(1.0, tb)
                if ta > tb:
                    continue
                xs = (g[0] + ta * (g[2] - g[0]), g[0] + tb * (g[2] - g[0]))
            j0, j1 = max(0, int(np.floor(min(xs) / 16)) - reach - 1), min(w - 1, int(np.ceil(max(xs) / 16)) + reach + 1)
            if j1 < j0:
                continue
            q = coverage_box(g, W16, j0, j1, ia, ib)
            key = np.where(q > 0, (q << 24) | k, 0)
            plane[ia:ib + 1, j0:j1 + 1] = np.maximum(plane[ia:ib + 1, j0:j1 + 1], key)
    return plane


def draw(image, segments, colors, color_index=None, width_px=1.0, opacity=255):
    """a new image: `image` (H x W or H x W x C uint8) with the segments drawn over it"""
    img = np.array(image, np.uint8, copy=True)
    h, w = img.shape[:2]
    px = img.reshape(h, w, -1)                   # a view: H x W x channels
    colors = np.asarray(colors, np.uint8).reshape(-1, 4).astype(np.int64)
    if len(np.asarray(segments).reshape(-1, 4)) == 0:
        return img
    plane = key_plane((h, w), segments, width_px)
    hit = plane > 0
    q, k = plane >> 24, plane & 0xFFFFFF
    ci = k % len(colors) if color_index is None else np.asarray(color_index, np.int64)[np.minimum(k, max(0, len(color_index) - 1))]
    col = colors[ci]                            # H x W x 4
    A = (col[..., 3] * int(opacity) + 127) // 255
    a = (q * A + 127) // 255
    for c in range(min(px.shape[2], 3)):
        src = px[..., c].astype(np.int64)
        out = (src * (255 - a) + col[..., c] * a + 127) // 255
        px[..., c] = np.where(hit, out, src).astype(np.uint8)
    return img
