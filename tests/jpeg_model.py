"""The baseline JPEG contract of include/line3d_amd.h in numpy: marker parser, Huffman decoder, dequantisation + inverse DCT (IJG's jidctint in
64-bit integers), fancy chroma upsampling, YCbCr -> RGB, output B, G, R.  Written from the contract, independent of the library's decoder; the tests hold
it to Pillow's (libjpeg-turbo's) pixels byte for byte (tests/golden/jpeg_ref.npz) and hold the library to it."""
import numpy as np

OK, INVALID, UNSUPPORTED = 0, 1, 5

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
                   50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _ceil_div(a, b):
    return -(-a // b)


def parse(data):
    """headers up to SOS -> dict(width, height, ncomp, comps[(id, h, v, tq, td, ta)], qt (ncomp, 64) natural order, huff, restart_interval, rgb,
    scan_offset, and the layout: hmax, vmax, mcux, mcuy, per component bw, bh, cw, chh)"""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegError(INVALID, "no SOI")
    pos = 2
    qtab, huff = {}, {}
    frame = None
    jfif = adobe = False
    transform = 0
    restart = 0
    while True:
        if pos + 2 > n:
            raise JpegError(INVALID, "truncated before the scan")
        if data[pos] != 0xFF:
            raise JpegError(INVALID, "marker expected")
        pos += 1
        while True:
            if pos >= n:
                raise JpegError(INVALID, "truncated in a marker")
            m = data[pos]
            pos += 1
            if m != 0xFF:
                break
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9, 0x00):
            raise JpegError(INVALID, "misplaced marker %02x" % m)
        if pos + 2 > n:
            raise JpegError(INVALID, "truncated segment header")
        ln = (data[pos] << 8) | data[pos + 1]
        if ln < 2 or pos + ln > n:
            raise JpegError(INVALID, "segment past the end")
        d = data[pos + 2:pos + ln]
        pos += ln
        if m == 0xC2:
            raise JpegError(UNSUPPORTED, "progressive")
        if m in (0xC3, 0xC5, 0xC6, 0xC7):
            raise JpegError(UNSUPPORTED, "lossless / differential")
        if m in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise JpegError(UNSUPPORTED, "arithmetic coding")
        if m in (0xC0, 0xC1):
            if frame is not None or len(d) < 6:
                raise JpegError(INVALID, "frame header")
            prec, height, width, nc = d[0], (d[1] << 8) | d[2], (d[3] << 8) | d[4], d[5]
            if prec in (12, 16):
                raise JpegError(UNSUPPORTED, "12-bit")
            if prec != 8:
                raise JpegError(INVALID, "precision")
            if width == 0 or height == 0:
                raise JpegError(INVALID, "zero dimensions")
            if nc in (2, 4):
                raise JpegError(UNSUPPORTED, "components")
            if nc not in (1, 3) or len(d) != 6 + 3 * nc:
                raise JpegError(INVALID, "components")
            comps = []
            for i in range(nc):
                cid, hv, tq = d[6 + 3 * i:9 + 3 * i]
                h, v = hv >> 4, hv & 15
                if not (1 <= h <= 4 and 1 <= v <= 4 and tq <= 3):
                    raise JpegError(INVALID, "sampling")
                comps.append([cid, h, v, tq, 0, 0])
            if nc == 1:
                comps[0][1] = comps[0][2] = 1
            elif [c[1:3] for c in comps[1:]] != [[1, 1], [1, 1]] or comps[0][1:3] not in ([1, 1], [2, 1], [2, 2]):
                raise JpegError(UNSUPPORTED, "sampling")
            frame = dict(width=width, height=height, ncomp=nc, comps=comps)
        elif m == 0xDB:
            o = 0
            while o < len(d):
                pq, tq = d[o] >> 4, d[o] & 15
                o += 1
                if pq > 1 or tq > 3 or len(d) - o < 64 * (pq + 1):
                    raise JpegError(INVALID, "DQT")
                t = np.zeros(64, np.uint16)
                for k in range(64):
                    t[ZIGZAG[k]] = ((d[o] << 8) | d[o + 1]) if pq else d[o]
                    o += pq + 1
                qtab[tq] = t
        elif m == 0xC4:
            o = 0
            while o < len(d):
                tc, th = d[o] >> 4, d[o] & 15
                o += 1
                if tc > 1 or th > 3 or len(d) - o < 16:
                    raise JpegError(INVALID, "DHT")
                bits = list(d[o:o + 16])
                o += 16
                total = sum(bits)
                if total > 256 or len(d) - o < total:
                    raise JpegError(INVALID, "DHT symbols")
                vals = list(d[o:o + total])
                o += total
                codes, code, k = {}, 0, 0
                for ln_ in range(1, 17):
                    for _ in range(bits[ln_ - 1]):
                        if code >= (1 << ln_):
                            raise JpegError(INVALID, "DHT oversubscribed")
                        codes[(ln_, code)] = vals[k]
                        code += 1
                        k += 1
                    code <<= 1
                if tc == 0 and any(v > 15 for v in vals):
                    raise JpegError(INVALID, "DC symbol")
                huff[(tc, th)] = codes
        elif m == 0xDD:
            if len(d) != 2:
                raise JpegError(INVALID, "DRI")
            restart = (d[0] << 8) | d[1]
        elif m == 0xE0:
            if len(d) >= 14 and d[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(d) >= 12 and d[:5] == b"Adobe":
                adobe, transform = True, d[11]
        elif m == 0xDA:
            if frame is None or len(d) < 1:
                raise JpegError(INVALID, "scan before frame")
            ns = d[0]
            if ns < 1 or ns > 4 or len(d) != 4 + 2 * ns:
                raise JpegError(INVALID, "scan header")
            if ns != frame["ncomp"]:
                raise JpegError(UNSUPPORTED, "more than one scan")
            ids = [c[0] for c in frame["comps"]]
            qt = np.zeros((ns, 64), np.uint16)
            hf = []
            for i, c in enumerate(frame["comps"]):
                cs, tt = d[1 + 2 * i], d[2 + 2 * i]
                if cs not in ids:
                    raise JpegError(INVALID, "unknown scan component")
                if cs != c[0]:
                    raise JpegError(UNSUPPORTED, "scan order")
                c[4], c[5] = tt >> 4, tt & 15
                if c[4] > 3 or c[5] > 3 or c[3] not in qtab or (0, c[4]) not in huff or (1, c[5]) not in huff:
                    raise JpegError(INVALID, "missing table")
                qt[i] = qtab[c[3]]
                hf.append((huff[(0, c[4])], huff[(1, c[5])]))
            W, H = frame["width"], frame["height"]
            hmax, vmax = frame["comps"][0][1], frame["comps"][0][2]
            mcux, mcuy = _ceil_div(W, 8 * hmax), _ceil_div(H, 8 * vmax)
            layout = [(mcux * c[1], mcuy * c[2], _ceil_div(W * c[1], hmax), _ceil_div(H * c[2], vmax)) for c in frame["comps"]]
            if sum(bw * bh for bw, bh, _, _ in layout) > 1 << 24:
                raise JpegError(UNSUPPORTED, "image too large")
            rgb = 0
            if ns == 3:
                if jfif:
                    rgb = 0
                elif adobe:
                    rgb = int(transform == 0)
                else:
                    rgb = int(ids == [ord("R"), ord("G"), ord("B")])
            frame.update(qt=qt, huff=hf, restart_interval=restart, rgb=rgb, scan_offset=pos, hmax=hmax, vmax=vmax, mcux=mcux, mcuy=mcuy, layout=layout)
            return frame


class _Bits:
    """bits of the entropy-coded segment; running out of data (a marker or the end of the file) raises"""

    def __init__(self, data, pos):
        self.d, self.pos, self.acc, self.n = data, pos, 0, 0

    def _byte(self):
        d = self.d
        while True:
            if self.pos >= len(d):
                raise JpegError(INVALID, "truncated entropy data")
            b = d[self.pos]
            if b != 0xFF:
                self.pos += 1
                return b
            if self.pos + 1 >= len(d):
                raise JpegError(INVALID, "truncated entropy data")
            b2 = d[self.pos + 1]
            if b2 == 0:
                self.pos += 2
                return 0xFF
            if b2 == 0xFF:
                self.pos += 1
                continue
            raise JpegError(INVALID, "marker inside entropy data")

    def bit(self):
        if self.n == 0:
            self.acc, self.n = self._byte(), 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, codes):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.bit()
            s = codes.get((ln, code))
            if s is not None:
                return s
        raise JpegError(INVALID, "code not in the table")

    def restart(self, m):
        self.n = 0
        d = self.d
        if self.pos + 1 >= len(d) or d[self.pos] != 0xFF:
            raise JpegError(INVALID, "restart marker expected")
        while self.pos + 1 < len(d) and d[self.pos + 1] == 0xFF:
            self.pos += 1
        if self.pos + 1 >= len(d) or d[self.pos + 1] != 0xD0 + (m & 7):
            raise JpegError(INVALID, "wrong restart marker")
        self.pos += 2


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def coefficients(data, f=None):
    """-> (frame, int16 (n_blocks, 64)): quantised coefficients in natural order, per component, per block row, per block column"""
    data = bytes(data)
    f = f or parse(data)
    comps, layout = f["comps"], f["layout"]
    starts, at = [], 0
    for bw, bh, _, _ in layout:
        starts.append(at)
        at += bw * bh
    coef = np.zeros((at, 64), np.int16)
    b = _Bits(data, f["scan_offset"])
    pred = [0] * len(comps)
    ri, to_go, restarts = f["restart_interval"], f["restart_interval"], 0
    for my in range(f["mcuy"]):
        for mx in range(f["mcux"]):
            if ri and to_go == 0:
                b.restart(restarts)
                restarts += 1
                pred = [0] * len(comps)
                to_go = ri
            for ci, c in enumerate(comps):
                dc, ac = f["huff"][ci]
                for by in range(c[2]):
                    for bx in range(c[1]):
                        out = coef[starts[ci] + (my * c[2] + by) * layout[ci][0] + mx * c[1] + bx]
                        s = b.symbol(dc)
                        if s:
                            pred[ci] += _extend(b.bits(s), s)
                        if not -32768 <= pred[ci] <= 32767:
                            raise JpegError(INVALID, "DC predictor range")
                        out[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = b.symbol(ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise JpegError(INVALID, "coefficient index past 63")
                            out[ZIGZAG[k]] = _extend(b.bits(s), s)
                            k += 1
            to_go -= 1
    return f, coef


def _pass(v):
    """one 1-D pass of jidctint on v[..., 0..7] (int64), before the descale"""
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., i] for i in range(8))
    z1 = (v2 + v6) * 4433
    t2 = z1 - v6 * 15137
    t3 = z1 + v2 * 6270
    t0 = (v0 + v4) << 13
    t1 = (v0 - v4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v7, v5, v3, v1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], axis=-1)


def idct_blocks(coef, q):
    """coef (n, 64) int16, q (64,) -> (n, 8, 8) uint8"""
    c = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    ws = (_pass(np.swapaxes(c, 1, 2)) + 1024) >> 11            # columns: [n, column, row-out]
    ws = np.swapaxes(ws, 1, 2)                                  # [n, row, column]
    out = ((_pass(ws) + 131072) >> 18) + 128
    return np.clip(out, 0, 255).astype(np.uint8)


def planes(f, coef):
    """uint8 component planes over whole MCUs"""
    out, at = [], 0
    for ci, (bw, bh, _, _) in enumerate(f["layout"]):
        blk = idct_blocks(coef[at:at + bw * bh], f["qt"][ci]).reshape(bh, bw, 8, 8)
        out.append(blk.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
        at += bw * bh
    return out


def _h2(t, r1, r2, shift):
    """the horizontal step on rows t (int64) of width cw: out[2i] = (3 t[i] + t[i-1] + r1) >> shift, out[2i+1] = (3 t[i] + t[i+1] + r2) >> shift, ends replicated"""
    left = np.concatenate([t[:, :1], t[:, :-1]], axis=1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int64)
    out[:, 0::2] = (3 * t + left + r1) >> shift
    out[:, 1::2] = (3 * t + right + r2) >> shift
    return out


def upsample(s, hf, vf):
    """s: the component at its real size (chh, cw), int64 -> (chh vf, cw hf)"""
    if hf == 1 and vf == 1:
        return s
    if vf == 1:
        return _h2(4 * s, 4, 8, 4)          # 3 s + nb over 4 with offsets 1 / 2: the same numbers on 4 s over 16
    up = np.concatenate([s[:1], s[:-1]], axis=0)
    down = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), np.int64)
    out[0::2] = _h2(3 * s + up, 8, 7, 4)
    out[1::2] = _h2(3 * s + down, 8, 7, 4)
    return out


def assemble(f, pl):
    W, H = f["width"], f["height"]
    if f["ncomp"] == 1:
        return pl[0][:H, :W].copy()
    full = []
    for ci, c in enumerate(f["comps"]):
        _, _, cw, chh = f["layout"][ci]
        full.append(upsample(pl[ci][:chh, :cw].astype(np.int64), f["hmax"] // c[1], f["vmax"] // c[2])[:H, :W])
    if f["rgb"]:
        r, g, b = full
    else:
        y, cb, cr = full[0], full[1] - 128, full[2] - 128
        r = y + ((91881 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """JPEG file bytes -> H x W (grey) or H x W x 3 (B, G, R) uint8"""
    f, coef = coefficients(data)
    return assemble(f, planes(f, coef))
