// l3d_draw.hpp -- 2-D segments drawn over 8-bit pixels ("PROJECTION AND OVERLAYS", 2, in include/line3d_amd.h states every rule; tests/draw_model.py
// holds the same in numpy): the clip, the quantisation to sixteenths of a pixel, the distance and coverage of a pixel centre, the pieces of 64 steps
// a segment is cut into, the walk of one lane across the stroke, the key of a (coverage, segment) pair and the blend -- written once for the device
// (l3d_draw.hip: one wave per piece, atomicMax into a key plane, one thread per pixel for the blend) and for the host (l3d_test_draw_segments_host:
// the same functions, piece after piece, lane after lane).  Floating point is f64, every operation rounded on its own (-ffp-contract=off); integers
// are int64.  The file is plain C++ as well: tests/cpp/project_draw_asan.cpp builds it into a host program of its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/line3d_amd.h"
#include "l3d_project.hpp"

namespace l3d {
namespace draw {

constexpr int kMaxSide = 32768;
constexpr int kMaxSegments = 1 << 24;

// a clipped and quantised segment, and the pieces it is cut into.  Sixteenths of a pixel; `lo`: the first column (ymajor: row) whose centre the
// stroke can reach, `ncol` of them (0: the segment draws nothing)
struct Seg {
    long long px, py, qx, qy;
    double rinv;                    // 1 / sqrt(L2); unread when L2 == 0
    int lo, ncol, ymajor;
    int rlo, rhi, pad;              // the rows the walk of its lanes can touch (rlo > rhi: none)
};

// where the pixels lie: element (i, j, component k) at base + i sy + j sx + off[k] bytes
struct Target {
    unsigned char* base;
    long long sy, sx, off[3];
    int width, height, ncomp;       // ncomp: colour components written, min(channels, 3)
};

L3D_PJ_HD int stroke16(double width_px) { return (int)rint(width_px * 16.0); }
L3D_PJ_HD double radius16(int W16) { return (double)W16 / 2.0 + 8.0; }
L3D_PJ_HD bool finf(float x) { return fabsf(x) <= 3.402823466e38f; }          // (NaN compares false)
L3D_PJ_HD long long floor16(long long a) { return a >= 0 ? a / 16 : -((-a + 15) / 16); }
L3D_PJ_HD long long ceil16(long long a) { return -floor16(-a); }

// half the height of a lane's walk across the stroke, in sixteenths (walk_lane)
L3D_PJ_HD long long walk_half(int W16) { return (long long)ceil(1.4143 * radius16(W16)) + 2; }

// clip, quantise, choose the major axis, bound the columns.  false: the segment is dropped
L3D_PJ_HD bool seg_setup(const float* s, int W16, int width, int height, Seg& g)
{
    g.ncol = 0; g.rlo = 2147483647; g.rhi = -1; g.pad = 0;
    if (!(finf(s[0]) && finf(s[1]) && finf(s[2]) && finf(s[3]))) return false;
    const double xP = (double)s[0], yP = (double)s[1], dx = (double)s[2] - xP, dy = (double)s[3] - yP;
    if (!(project::fin(dx) && project::fin(dy))) return false;
    const double margin = (double)((W16 + 31) / 32 + 1);
    double t0, t1;
    if (!project::clip_rect(project::image_rect(width, height, margin), xP, yP, dx, dy, t0, t1)) return false;
    const double x0 = t0 == 0.0 ? xP : xP + t0 * dx, y0 = t0 == 0.0 ? yP : yP + t0 * dy;
    const double x1 = t1 == 1.0 ? (double)s[2] : xP + t1 * dx, y1 = t1 == 1.0 ? (double)s[3] : yP + t1 * dy;
    g.px = (long long)rint(x0 * 16.0); g.py = (long long)rint(y0 * 16.0);
    g.qx = (long long)rint(x1 * 16.0); g.qy = (long long)rint(y1 * 16.0);
    const long long bx = g.qx - g.px, by = g.qy - g.py, L2 = bx * bx + by * by;
    g.rinv = L2 > 0 ? 1.0 / sqrt((double)L2) : 0.0;
    g.ymajor = (bx < 0 ? -bx : bx) >= (by < 0 ? -by : by) ? 0 : 1;
    // the columns (rows) whose centres lie within the stroke's reach of the segment's extent along the major axis
    const long long mP = g.ymajor ? g.py : g.px, mQ = g.ymajor ? g.qy : g.qx, reach = (long long)ceil(radius16(W16));
    const long long lim = g.ymajor ? height : width;
    long long lo = ceil16((mP < mQ ? mP : mQ) - reach), hi = floor16((mP > mQ ? mP : mQ) + reach);
    if (lo < 0) lo = 0;
    if (hi > lim - 1) hi = lim - 1;
    g.lo = (int)lo; g.ncol = hi >= lo ? (int)(hi - lo + 1) : 0;
    if (g.ncol > 0) {
        if (g.ymajor) { g.rlo = g.lo; g.rhi = g.lo + g.ncol - 1; }
        else {          // (walk_lane's centre line lies between the ends' rows, a rounding apart at the most)
            const long long H = walk_half(W16) + 1;
            long long a = ceil16((g.py < g.qy ? g.py : g.qy) - H), b = floor16((g.py > g.qy ? g.py : g.qy) + H);
            if (a < 0) a = 0;
            if (b > height - 1) b = height - 1;
            g.rlo = (int)a; g.rhi = (int)b;
        }
    }
    return true;
}

L3D_PJ_HD int pieces_of(const Seg& g) { return (g.ncol + 63) / 64; }

// q of the pixel centre (cx, cy), in sixteenths
L3D_PJ_HD int coverage(const Seg& g, double R16, long long cx, long long cy)
{
    const long long ax = cx - g.px, ay = cy - g.py, bx = g.qx - g.px, by = g.qy - g.py;
    const long long L2 = bx * bx + by * by, dot = ax * bx + ay * by;
    double d;
    if (dot <= 0) d = sqrt((double)(ax * ax + ay * ay));
    else if (dot >= L2) { const long long ex = cx - g.qx, ey = cy - g.qy; d = sqrt((double)(ex * ex + ey * ey)); }
    else { const long long cr = ax * by - ay * bx; d = (double)(cr < 0 ? -cr : cr) * g.rinv; }
    double cov = (R16 - d) / 16.0;
    cov = cov < 0.0 ? 0.0 : (cov > 1.0 ? 1.0 : cov);
    return (int)floor(cov * 255.0 + 0.5);
}

// One lane of a piece: column (ymajor: row) `col` of segment k.  Every pixel of the column the stroke can reach is tested -- the centre line at the
// column, clamped to the segment's extent, and sqrt(2) R16 either side of it bound them (a point within R16 of the segment lies within R16 of a point of
// it in both coordinates, and the centre line's slope along the major axis is at most 1) -- and put(pixel index i width + j, key) gets those with q > 0
template <class Put> L3D_PJ_HD void walk_lane(const Seg& g, int W16, int width, int height, int col, unsigned k, Put& put)
{
    const double R16 = radius16(W16);
    const long long mP = g.ymajor ? g.py : g.px, mQ = g.ymajor ? g.qy : g.qx, sP = g.ymajor ? g.px : g.py, sQ = g.ymajor ? g.qx : g.qy;
    const long long mlo = mP < mQ ? mP : mQ, mhi = mP > mQ ? mP : mQ;
    long long mc = 16ll * col;
    mc = mc < mlo ? mlo : (mc > mhi ? mhi : mc);
    const double sc = mQ == mP ? (double)sP : (double)sP + ((double)(mc - mP) * (double)(sQ - sP)) / (double)(mQ - mP);
    const long long H = walk_half(W16);
    const long long lim = g.ymajor ? width : height;
    long long lo = ceil16((long long)floor(sc) - H), hi = floor16((long long)ceil(sc) + H);
    if (lo < 0) lo = 0;
    if (hi > lim - 1) hi = lim - 1;
    for (long long r = lo; r <= hi; ++r) {
        const long long j = g.ymajor ? r : col, i = g.ymajor ? col : r;
        const int q = coverage(g, R16, 16 * j, 16 * i);
        if (q > 0) put((size_t)i * (size_t)width + (size_t)j, ((unsigned)q << 24) | k);
    }
}

// the blend of one pixel whose key is not 0
L3D_PJ_HD void blend_pixel(const Target& t, int i, int j, unsigned key, const unsigned char* colors, int n_colors, const int32_t* color_index, int opacity)
{
    const int q = (int)(key >> 24);
    const unsigned k = key & 0xffffffu;
    const unsigned char* col = colors + 4 * (size_t)(color_index ? color_index[k] : (int)(k % (unsigned)n_colors));
    const int A = ((int)col[3] * opacity + 127) / 255, a = (q * A + 127) / 255;
    unsigned char* p = t.base + (long long)i * t.sy + (long long)j * t.sx;
    for (int c = 0; c < t.ncomp; ++c) {
        const int src = p[t.off[c]];
        p[t.off[c]] = (unsigned char)((src * (255 - a) + (int)col[c] * a + 127) / 255);
    }
}

// the refusals that need no device, in the header's order (the pixels themselves are checked by the caller: host pointer or device image)
inline int check_arguments(int width, int height, int channels, const float* segments, int n, const unsigned char* colors, int n_colors, const int32_t* color_index,
                           double width_px, int opacity, std::string& err)
{
    if (n < 0) { err = "draw segments: a negative count"; return L3D_ERR_INVALID; }
    if ((n > 0 && !segments) || !colors) { err = "draw segments: a null pointer"; return L3D_ERR_INVALID; }
    if (width < 1 || height < 1) { err = "draw segments: a size below 1 x 1"; return L3D_ERR_INVALID; }
    if (channels != 1 && channels != 3 && channels != 4) { err = "draw segments: channels must be 1, 3 or 4"; return L3D_ERR_INVALID; }
    if (n_colors < 1) { err = "draw segments: at least one colour is needed"; return L3D_ERR_INVALID; }
    if (!(width_px >= 0.5 && width_px <= 64.0)) { err = "draw segments: width_px must lie in [0.5, 64]"; return L3D_ERR_INVALID; }
    if (opacity < 0 || opacity > 255) { err = "draw segments: opacity outside 0..255"; return L3D_ERR_INVALID; }
    if (n > kMaxSegments) { err = "draw segments: more than 2^24 segments"; return L3D_ERR_UNSUPPORTED; }
    if (width > kMaxSide || height > kMaxSide) { err = "draw segments: an image side above 32768"; return L3D_ERR_UNSUPPORTED; }
    if (color_index)
        for (int k = 0; k < n; ++k)
            if (color_index[k] < 0 || color_index[k] >= n_colors) { err = "draw segments: color_index[" + std::to_string(k) + "] is no colour"; return L3D_ERR_INVALID; }
    return L3D_OK;
}

// the whole call on the host: the pieces of every segment, lane after lane, into a key plane; then the blend of every pixel with a key
struct HostPut {
    std::vector<unsigned>& plane;
    void operator()(size_t at, unsigned key) { if (key > plane[at]) plane[at] = key; }
};
inline void run_host(const Target& t, const float* segments, int n, const unsigned char* colors, int n_colors, const int32_t* color_index, int W16, int opacity)
{
    std::vector<unsigned> plane((size_t)t.width * (size_t)t.height, 0u);
    HostPut put{ plane };
    for (int k = 0; k < n; ++k) {
        Seg g;
        if (!seg_setup(segments + 4 * (size_t)k, W16, t.width, t.height, g)) continue;
        for (int piece = 0; piece < pieces_of(g); ++piece)
            for (int lane = 0; lane < 64; ++lane) {
                const int c = piece * 64 + lane;
                if (c < g.ncol) walk_lane(g, W16, t.width, t.height, g.lo + c, (unsigned)k, put);
            }
    }
    for (int i = 0; i < t.height; ++i)
        for (int j = 0; j < t.width; ++j) {
            const unsigned key = plane[(size_t)i * t.width + j];
            if (key) blend_pixel(t, i, j, key, colors, n_colors, color_index, opacity);
        }
}

}  // namespace draw
}  // namespace l3d
