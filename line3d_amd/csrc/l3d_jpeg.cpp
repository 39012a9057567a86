// l3d_jpeg.cpp -- baseline JPEG on the host: the marker parser and the entropy decoder, the inherently serial part (contract: include/line3d_amd.h).
// Quantised coefficients leave this file as int16 in natural order; dequantisation, inverse DCT, upsampling and colour run on the device
// (k_jpg_idct, k_jpg_assemble in l3d_jpeg_device.hip).  No HIP include: the file compiles alone with g++ (tests/cpp/jpeg_mutate_main.cpp runs it under
// the address and undefined-behaviour sanitizers).  Every read is checked against the end of the file and every write against the block count.
#include "l3d_jpeg.hpp"

#include <cstdlib>
#include <cstring>

#include "../../include/line3d_amd.h"

namespace l3d {

namespace {

const unsigned char kZigzag[64] = { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

int bad(std::string& err, int code, const std::string& msg)
{
    err = "jpeg: " + msg;
    return code;
}

struct Reader {
    const unsigned char* p;
    size_t n, pos = 0;
    bool have(size_t k) const { return pos <= n && k <= n - pos; }
    int u8() { return p[pos++]; }
    int u16() { const int v = (p[pos] << 8) | p[pos + 1]; pos += 2; return v; }
};

const char* sof_refusal(int m)
{
    switch (m) {
    case 0xC2: return "progressive JPEG (SOF2) is not supported";
    case 0xC3: return "lossless JPEG (SOF3) is not supported";
    case 0xC5: case 0xC6: case 0xC7: return "differential (hierarchical) JPEG is not supported";
    case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: return "arithmetic coding is not supported";
    }
    return nullptr;
}

}  // namespace

int jpeg_parse(const unsigned char* bytes, size_t n, JpegFrame& f, std::string& err)
{
    f = JpegFrame();
    if (!bytes || n < 4 || bytes[0] != 0xFF || bytes[1] != 0xD8) return bad(err, kJpgInvalid, "not a JPEG file (no SOI marker)");
    Reader r{ bytes, n, 2 };
    uint16_t qtab[4][64];
    bool q_defined[4] = { false, false, false, false };
    JpegHuff huff[2][4];
    bool saw_sof = false, saw_jfif = false, saw_adobe = false;
    int adobe_transform = 0;
    for (;;) {
        // a marker: FF, any number of fill FFs, the code
        if (!r.have(2)) return bad(err, kJpgInvalid, "truncated: the file ends before the scan");
        if (r.u8() != 0xFF) return bad(err, kJpgInvalid, "corrupt: marker expected at byte " + std::to_string(r.pos - 1));
        int m = 0xFF;
        while (m == 0xFF) {
            if (!r.have(1)) return bad(err, kJpgInvalid, "truncated: the file ends inside a marker");
            m = r.u8();
        }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                 // TEM, RSTn: no length
        if (m == 0xD8) return bad(err, kJpgInvalid, "corrupt: a second SOI marker");
        if (m == 0xD9) return bad(err, kJpgInvalid, "corrupt: EOI before any scan");
        if (m == 0x00) return bad(err, kJpgInvalid, "corrupt: marker expected at byte " + std::to_string(r.pos - 2));
        if (!r.have(2)) return bad(err, kJpgInvalid, "truncated: the file ends inside a segment header");
        const int len = r.u16();
        if (len < 2 || !r.have((size_t)len - 2)) return bad(err, kJpgInvalid, "truncated: a segment runs past the end of the file");
        const size_t seg_end = r.pos + (size_t)len - 2;
        const unsigned char* d = bytes + r.pos;
        const int dl = len - 2;
        if (const char* why = sof_refusal(m)) return bad(err, kJpgUnsupported, why);
        if (m == 0xCC) return bad(err, kJpgUnsupported, "arithmetic coding is not supported");
        if (m == 0xC0 || m == 0xC1) {
            if (saw_sof) return bad(err, kJpgInvalid, "corrupt: a second frame header");
            if (dl < 6) return bad(err, kJpgInvalid, "corrupt: frame header too short");
            const int prec = d[0], nc = d[5];
            f.height = (d[1] << 8) | d[2];
            f.width = (d[3] << 8) | d[4];
            if (prec == 12 || prec == 16) return bad(err, kJpgUnsupported, std::to_string(prec) + "-bit samples are not supported");
            if (prec != 8) return bad(err, kJpgInvalid, "corrupt: sample precision " + std::to_string(prec));
            if (f.width == 0 || f.height == 0) return bad(err, kJpgInvalid, "zero dimensions");
            if (nc == 2 || nc == 4) return bad(err, kJpgUnsupported, std::to_string(nc) + " components (CMYK / YCCK) are not supported");
            if (nc != 1 && nc != 3) return bad(err, kJpgInvalid, "corrupt: " + std::to_string(nc) + " components");
            if (dl != 6 + 3 * nc) return bad(err, kJpgInvalid, "corrupt: frame header length");
            f.ncomp = nc;
            for (int i = 0; i < nc; ++i) {
                JpegComp& c = f.comp[i];
                c.id = d[6 + 3 * i];
                c.h = d[7 + 3 * i] >> 4;
                c.v = d[7 + 3 * i] & 15;
                c.tq = d[8 + 3 * i];
                if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4 || c.tq > 3) return bad(err, kJpgInvalid, "corrupt: component sampling or table number");
            }
            if (nc == 1) f.comp[0].h = f.comp[0].v = 1;          // a single component is never interleaved: its factors mean nothing
            else {
                const bool chroma1 = f.comp[1].h == 1 && f.comp[1].v == 1 && f.comp[2].h == 1 && f.comp[2].v == 1;
                const int yh = f.comp[0].h, yv = f.comp[0].v;
                if (!chroma1 || !((yh == 1 && yv == 1) || (yh == 2 && yv == 1) || (yh == 2 && yv == 2)))
                    return bad(err, kJpgUnsupported, "sampling " + std::to_string(yh) + "x" + std::to_string(yv) + "," + std::to_string(f.comp[1].h) + "x" +
                                                         std::to_string(f.comp[1].v) + "," + std::to_string(f.comp[2].h) + "x" + std::to_string(f.comp[2].v) +
                                                         " is not supported (4:4:4, 4:2:2 and 4:2:0 are)");
            }
            saw_sof = true;
        } else if (m == 0xDB) {
            int o = 0;
            while (o < dl) {
                const int pq = d[o] >> 4, tq = d[o] & 15;
                ++o;
                if (pq > 1 || tq > 3) return bad(err, kJpgInvalid, "corrupt: quantisation table header");
                if (dl - o < 64 * (pq + 1)) return bad(err, kJpgInvalid, "truncated: quantisation table");
                for (int k = 0; k < 64; ++k) {
                    qtab[tq][kZigzag[k]] = pq ? (uint16_t)((d[o] << 8) | d[o + 1]) : d[o];
                    o += pq + 1;
                }
                q_defined[tq] = true;
            }
        } else if (m == 0xC4) {
            int o = 0;
            while (o < dl) {
                const int tc = d[o] >> 4, th = d[o] & 15;
                ++o;
                if (tc > 1 || th > 3) return bad(err, kJpgInvalid, "corrupt: Huffman table header");
                if (dl - o < 16) return bad(err, kJpgInvalid, "truncated: Huffman table");
                JpegHuff& h = huff[tc][th];
                int total = 0, code = 0;
                h.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) {
                    h.bits[l] = d[o + l - 1];
                    total += h.bits[l];
                    code += h.bits[l];
                    if (code > (1 << l)) return bad(err, kJpgInvalid, "corrupt: Huffman table with more codes than its lengths allow");
                    code <<= 1;
                }
                o += 16;
                if (total > 256 || dl - o < total) return bad(err, kJpgInvalid, "truncated: Huffman table symbols");
                memset(h.vals, 0, sizeof(h.vals));
                for (int k = 0; k < total; ++k) {
                    h.vals[k] = d[o + k];
                    if (tc == 0 && h.vals[k] > 15) return bad(err, kJpgInvalid, "corrupt: DC Huffman symbol above 15");
                }
                o += total;
                h.defined = true;
            }
        } else if (m == 0xDD) {
            if (dl != 2) return bad(err, kJpgInvalid, "corrupt: restart interval length");
            f.restart_interval = (d[0] << 8) | d[1];
        } else if (m == 0xE0) {
            if (dl >= 14 && d[0] == 'J' && d[1] == 'F' && d[2] == 'I' && d[3] == 'F' && d[4] == 0) saw_jfif = true;
        } else if (m == 0xEE) {
            if (dl >= 12 && d[0] == 'A' && d[1] == 'd' && d[2] == 'o' && d[3] == 'b' && d[4] == 'e') { saw_adobe = true; adobe_transform = d[11]; }
        } else if (m == 0xDA) {
            if (!saw_sof) return bad(err, kJpgInvalid, "corrupt: scan before the frame header");
            if (dl < 1) return bad(err, kJpgInvalid, "corrupt: scan header too short");
            const int ns = d[0];
            if (ns < 1 || ns > 4 || dl != 4 + 2 * ns) return bad(err, kJpgInvalid, "corrupt: scan header");
            if (ns != f.ncomp) return bad(err, kJpgUnsupported, "more than one scan for a baseline frame is not supported");
            for (int i = 0; i < ns; ++i) {
                JpegComp& c = f.comp[i];
                const int cs = d[1 + 2 * i];
                bool known = false;
                for (int j = 0; j < f.ncomp; ++j) known = known || f.comp[j].id == cs;
                if (!known) return bad(err, kJpgInvalid, "corrupt: the scan names a component the frame does not have");
                if (cs != c.id) return bad(err, kJpgUnsupported, "a scan whose components are not in frame order is not supported");
                c.td = d[2 + 2 * i] >> 4;
                c.ta = d[2 + 2 * i] & 15;
                if (c.td > 3 || c.ta > 3) return bad(err, kJpgInvalid, "corrupt: Huffman table number in the scan header");
                if (!q_defined[c.tq]) return bad(err, kJpgInvalid, "missing table: quantisation table " + std::to_string(c.tq));
                if (!huff[0][c.td].defined) return bad(err, kJpgInvalid, "missing table: DC Huffman table " + std::to_string(c.td));
                if (!huff[1][c.ta].defined) return bad(err, kJpgInvalid, "missing table: AC Huffman table " + std::to_string(c.ta));
                memcpy(f.qt[i], qtab[c.tq], sizeof(f.qt[i]));
            }
            for (int i = ns; i < 3; ++i) memset(f.qt[i], 0, sizeof(f.qt[i]));
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 4; ++b) f.huff[a][b] = huff[a][b];
            // layout
            f.hmax = f.comp[0].h;
            f.vmax = f.comp[0].v;
            f.mcux = (f.width + 8 * f.hmax - 1) / (8 * f.hmax);
            f.mcuy = (f.height + 8 * f.vmax - 1) / (8 * f.vmax);
            size_t at = 0;
            for (int i = 0; i < f.ncomp; ++i) {
                JpegComp& c = f.comp[i];
                c.bw = f.mcux * c.h;
                c.bh = f.mcuy * c.v;
                c.cw = (f.width * c.h + f.hmax - 1) / f.hmax;
                c.chh = (f.height * c.v + f.vmax - 1) / f.vmax;
                c.block0 = at;
                at += (size_t)c.bw * c.bh;
            }
            // the host-only callers size their coefficient buffers from the headers alone: the bound is here, for every caller
            if (at > kJpgMaxBlocks) return bad(err, kJpgUnsupported, "image too large: " + std::to_string(at) + " blocks (at most " + std::to_string(kJpgMaxBlocks) + ")");
            f.n_blocks = at;
            // colour: libjpeg's rule
            f.rgb = 0;
            if (f.ncomp == 3) {
                if (saw_jfif) f.rgb = 0;
                else if (saw_adobe) f.rgb = adobe_transform == 0;
                else f.rgb = f.comp[0].id == 'R' && f.comp[1].id == 'G' && f.comp[2].id == 'B';
            }
            f.scan_offset = seg_end;
            return kJpgOk;
        }
        // APPn, COM and everything else with a length: skipped
        r.pos = seg_end;
    }
}

namespace {

// the next 9 bits decide codes of up to 9 bits; longer ones walk the canonical code's per-length limits
constexpr int kLook = 9;
struct HuffDec {
    uint16_t look[1 << kLook];      // length << 8 | symbol; 0: longer than kLook bits (or no such code)
    int32_t maxcode[18];            // largest code of each length, -1: none
    int32_t valoff[17];             // index of the length's first symbol minus its first code
    const uint8_t* vals;
};

void build(const JpegHuff& h, HuffDec& t)
{
    memset(t.look, 0, sizeof(t.look));
    t.vals = h.vals;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        if (h.bits[l]) {
            for (int i = 0; i < h.bits[l]; ++i, ++k, ++code)
                if (l <= kLook) {
                    const int first = code << (kLook - l), count = 1 << (kLook - l);
                    for (int j = 0; j < count; ++j) t.look[first + j] = (uint16_t)((l << 8) | h.vals[k]);
                }
            t.maxcode[l] = code - 1;
        } else
            t.maxcode[l] = -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
}

// bits of the entropy-coded segment, most significant first.  FF 00 is a data byte FF, FF FF a fill byte; at a marker or at the end of the file
// the reader stops and feeds zeros that do not count: taking more bits than the data holds is an error the caller sees in `real`
struct Bits {
    const unsigned char* p;
    size_t n, pos;
    uint64_t acc = 0;
    int nbits = 0;
    long long real = 0;            // bits in `acc` that came from the file
    bool stopped = false;
    void fill()
    {
        while (nbits <= 56) {
            unsigned b = 0;
            bool got = false;
            while (!stopped && !got) {
                if (pos >= n) { stopped = true; break; }
                b = p[pos];
                if (b != 0xFF) { ++pos; got = true; break; }
                if (pos + 1 >= n) { stopped = true; break; }
                const unsigned b2 = p[pos + 1];
                if (b2 == 0x00) { pos += 2; got = true; }
                else if (b2 == 0xFF) ++pos;
                else stopped = true;
            }
            if (!got) b = 0;
            acc |= (uint64_t)b << (56 - nbits);
            nbits += 8;
            if (got) real += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(acc >> (64 - k)); }
    void skip(int k) { acc <<= k; nbits -= k; real -= k; }
    void align_and_reset() { acc = 0; nbits = 0; real = 0; stopped = false; }
};

// a symbol, or -1: no such code
inline int decode_symbol(Bits& b, const HuffDec& t)
{
    if (b.nbits < 16) b.fill();
    const unsigned e = t.look[b.peek(kLook)];
    if (e) { b.skip((int)(e >> 8)); return (int)(e & 255); }
    const int code16 = (int)b.peek(16);
    for (int l = kLook + 1; l <= 16; ++l) {
        const int code = code16 >> (16 - l);
        if (code <= t.maxcode[l]) { b.skip(l); return t.vals[(t.valoff[l] + code) & 255]; }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s)
{
    if (b.nbits < s) b.fill();
    const int v = (int)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace

int jpeg_decode_coefficients(const unsigned char* bytes, size_t n, const JpegFrame& f, int16_t* coef, std::string& err)
{
    if (!bytes || !coef || f.n_blocks == 0 || f.scan_offset > n) return bad(err, kJpgInvalid, "no parsed frame");
    memset(coef, 0, f.n_blocks * 64 * sizeof(int16_t));
    HuffDec* tabs = static_cast<HuffDec*>(malloc(sizeof(HuffDec) * 6));
    if (!tabs) return bad(err, kJpgInvalid, "out of memory");
    for (int i = 0; i < f.ncomp; ++i) {
        build(f.huff[0][f.comp[i].td], tabs[2 * i]);
        build(f.huff[1][f.comp[i].ta], tabs[2 * i + 1]);
    }
    Bits b{ bytes, n, f.scan_offset };
    int pred[3] = { 0, 0, 0 };
    int rc = kJpgOk, restarts = 0;
    long long to_go = f.restart_interval;
    const long long n_mcu = (long long)f.mcux * f.mcuy;
    long long mcu = 0;
    for (int my = 0; my < f.mcuy && rc == kJpgOk; ++my)
        for (int mx = 0; mx < f.mcux && rc == kJpgOk; ++mx, ++mcu) {
            if (f.restart_interval && to_go == 0) {
                // byte-align, the marker RST (m mod 8), predictors to zero
                b.align_and_reset();
                size_t& pos = b.pos;
                if (pos + 1 >= n || bytes[pos] != 0xFF) { rc = bad(err, kJpgInvalid, "corrupt or truncated: restart marker expected in MCU " + std::to_string(mcu)); break; }
                while (pos + 1 < n && bytes[pos + 1] == 0xFF) ++pos;
                if (pos + 1 >= n || bytes[pos + 1] != 0xD0 + (restarts & 7)) { rc = bad(err, kJpgInvalid, "corrupt: wrong restart marker in MCU " + std::to_string(mcu)); break; }
                pos += 2;
                ++restarts;
                pred[0] = pred[1] = pred[2] = 0;
                to_go = f.restart_interval;
            }
            for (int ci = 0; ci < f.ncomp && rc == kJpgOk; ++ci) {
                const JpegComp& c = f.comp[ci];
                const HuffDec &dc = tabs[2 * ci], &ac = tabs[2 * ci + 1];
                for (int by = 0; by < c.v && rc == kJpgOk; ++by)
                    for (int bx = 0; bx < c.h; ++bx) {
                        const size_t blk = c.block0 + (size_t)(my * c.v + by) * c.bw + (size_t)(mx * c.h + bx);
                        if (blk >= f.n_blocks) { rc = bad(err, kJpgInvalid, "block outside the frame"); break; }
                        int16_t* out = coef + blk * 64;
                        int s = decode_symbol(b, dc);
                        if (s < 0) { rc = bad(err, kJpgInvalid, "corrupt: a Huffman code that is not in the table (DC, MCU " + std::to_string(mcu) + ")"); break; }
                        if (s) pred[ci] += receive_extend(b, s);
                        if (pred[ci] < -32768 || pred[ci] > 32767) { rc = bad(err, kJpgInvalid, "corrupt: a DC predictor leaves the 16-bit range (MCU " + std::to_string(mcu) + ")"); break; }
                        out[0] = (int16_t)pred[ci];
                        for (int k = 1; k < 64;) {
                            const int rs = decode_symbol(b, ac);
                            if (rs < 0) { rc = bad(err, kJpgInvalid, "corrupt: a Huffman code that is not in the table (AC, MCU " + std::to_string(mcu) + ")"); break; }
                            const int run = rs >> 4;
                            s = rs & 15;
                            if (!s) {
                                if (run != 15) break;
                                k += 16;
                                continue;
                            }
                            k += run;
                            if (k > 63) { rc = bad(err, kJpgInvalid, "corrupt: a coefficient index past 63 (MCU " + std::to_string(mcu) + ")"); break; }
                            out[kZigzag[k]] = (int16_t)receive_extend(b, s);
                            ++k;
                        }
                        if (rc == kJpgOk && b.real < 0) rc = bad(err, kJpgInvalid, "truncated: the entropy-coded data ends in MCU " + std::to_string(mcu) + " of " + std::to_string(n_mcu));
                        if (rc != kJpgOk) break;
                    }
            }
            --to_go;
        }
    free(tabs);
    return rc;
}

}  // namespace l3d

// ---- C ABI without a context or a device: the size from the headers, and the entropy decoder's output for the tests
namespace {
thread_local std::string g_jpeg_err;
}

extern "C" {

const char* l3d_jpeg_last_error(void) { return g_jpeg_err.c_str(); }

int l3d_jpeg_info(const unsigned char* bytes, size_t n, int* width, int* height, int* channels)
{
    g_jpeg_err.clear();
    l3d::JpegFrame f;
    const int rc = l3d::jpeg_parse(bytes, n, f, g_jpeg_err);
    if (rc != L3D_OK) return rc;
    if (width) *width = f.width;
    if (height) *height = f.height;
    if (channels) *channels = f.ncomp;
    return L3D_OK;
}

int l3d_test_jpeg_coefficients(const unsigned char* bytes, size_t n, int16_t** coef, size_t* n_blocks, uint16_t* qt, int32_t* layout)
{
    g_jpeg_err.clear();
    if (!coef || !n_blocks || !qt || !layout) { g_jpeg_err = "jpeg: null argument"; return L3D_ERR_INVALID; }
    *coef = nullptr;
    *n_blocks = 0;
    l3d::JpegFrame f;
    int rc = l3d::jpeg_parse(bytes, n, f, g_jpeg_err);
    if (rc != L3D_OK) return rc;
    int16_t* c = static_cast<int16_t*>(malloc(f.n_blocks * 64 * sizeof(int16_t)));
    if (!c) { g_jpeg_err = "jpeg: out of memory"; return L3D_ERR_NOMEM; }
    rc = l3d::jpeg_decode_coefficients(bytes, n, f, c, g_jpeg_err);
    if (rc != L3D_OK) { free(c); return rc; }
    memcpy(qt, f.qt, sizeof(f.qt));
    const int32_t head[9] = { f.width, f.height, f.ncomp, f.hmax, f.vmax, f.mcux, f.mcuy, f.restart_interval, f.rgb };
    memcpy(layout, head, sizeof(head));
    for (int i = 0; i < 3; ++i) {
        const l3d::JpegComp& k = f.comp[i];
        const int32_t per[6] = { k.h, k.v, k.bw, k.bh, k.cw, k.chh }, none[6] = { 0, 0, 0, 0, 0, 0 };
        memcpy(layout + 9 + 6 * i, i < f.ncomp ? per : none, sizeof(per));
    }
    *coef = c;
    *n_blocks = f.n_blocks;
    return L3D_OK;
}

}  // extern "C"
