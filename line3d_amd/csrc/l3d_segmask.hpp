// l3d_segmask.hpp -- a mask applied to line segments ("A SEGMENT MASK" in include/line3d_amd.h states every rule; tests/segmask_model.py holds the
// same in numpy): the samples of a segment, their validity, the bridging of short gaps and the search for runs, written once for the device
// (l3d_segmask.hip: one wave per segment) and for the host (l3d_test_mask_segments_host: the same functions, lane after lane).  Everything is f64
// and int64, every product and sum rounded on its own (-ffp-contract=off).  The file is plain C++ as well: tests/cpp/segmask_asan.cpp builds it
// into a host program of its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/line3d_amd.h"
#include "l3d_undistort.hpp"

#if defined(__HIPCC__)
#define L3D_SM_HD __host__ __device__ __forceinline__
#else
#define L3D_SM_HD inline
#endif

namespace l3d {
namespace segmask {

constexpr double kMaxExtent = 65536.0;          // a segment whose longer extent reaches this is dropped: at most 65537 samples

// a checked l3d_segment_mask: all that the samples need.  mask: host memory for the host, device memory for the kernels
struct Plan {
    const unsigned char* mask;
    size_t stride;
    int mw, mh;
    int lens_on;                                // 0: the mask lies in the segments' grid
    DetLens L;                                  // the lens, source camera resolved; ofx, ofy, ocx, ocy: the segments' camera
    int mode, threshold, keep_permille, max_gap;
    double min_length;
};

// the refusals that need neither a lens check nor a device, in the header's order: L3D_OK with the plan filled (no lens), or L3D_ERR_INVALID and why
inline int check_fields(const l3d_segment_mask* m, Plan& p, std::string& err)
{
    if (!m || !m->mask) { err = "segment mask: the mask is null"; return L3D_ERR_INVALID; }
    if (m->mask_width < 1 || m->mask_height < 1) { err = "segment mask: an extent below 1 x 1"; return L3D_ERR_INVALID; }
    if (m->mask_row_stride < (size_t)m->mask_width) { err = "segment mask: the row stride is below the width"; return L3D_ERR_INVALID; }
    if (m->mode != L3D_SEGMASK_DROP && m->mode != L3D_SEGMASK_CLIP && m->mode != L3D_SEGMASK_SPLIT) { err = "segment mask: unknown mode " + std::to_string(m->mode); return L3D_ERR_INVALID; }
    if (m->threshold < 0 || m->threshold > 255) { err = "segment mask: threshold outside 0..255"; return L3D_ERR_INVALID; }
    if (m->keep_permille < 0 || m->keep_permille > 1000) { err = "segment mask: keep_permille outside 0..1000"; return L3D_ERR_INVALID; }
    if (m->max_gap < 0) { err = "segment mask: max_gap is negative"; return L3D_ERR_INVALID; }
    if (!(m->min_length >= 0.0) || !(m->min_length <= 1.7976931348623157e308)) { err = "segment mask: min_length must be a finite number >= 0"; return L3D_ERR_INVALID; }
    p.mask = static_cast<const unsigned char*>(m->mask);
    p.stride = m->mask_row_stride; p.mw = m->mask_width; p.mh = m->mask_height;
    p.lens_on = 0; p.L = DetLens{};
    p.mode = m->mode; p.threshold = m->threshold == 0 ? 1 : m->threshold; p.keep_permille = m->keep_permille; p.max_gap = m->max_gap;
    p.min_length = m->min_length;
    return L3D_OK;
}

// ---- the segment and its samples
struct Seg { double x1, y1, dx, dy; int n; };

L3D_SM_HD bool fin(float x) { return fabsf(x) <= 3.402823466e38f; }          // (NaN compares false)

// false: the segment is dropped in every mode (a coordinate that is not finite, no extent, too long)
L3D_SM_HD bool seg_setup(const float* s, Seg& g)
{
    if (!(fin(s[0]) && fin(s[1]) && fin(s[2]) && fin(s[3]))) return false;
    g.x1 = (double)s[0]; g.y1 = (double)s[1];
    g.dx = (double)s[2] - g.x1; g.dy = (double)s[3] - g.y1;
    const double m = fmax(fabs(g.dx), fabs(g.dy));
    if (m == 0.0 || m >= kMaxExtent) return false;
    g.n = (int)floor(m) + 1;
    return true;
}

L3D_SM_HD void sample_pos(const Seg& g, int k, double& px, double& py)
{
    const double t = (double)k / (double)g.n;
    px = g.x1 + t * g.dx; py = g.y1 + t * g.dy;
}

// the map of "A LENS" at a position (j, i) that need not be a pixel centre
L3D_SM_HD void lens_map(const DetLens& L, double j, double i, double& u, double& v)
{
    const double x = (j - L.ocx) / L.ofx, y = (i - L.ocy) / L.ofy;
    const double r2 = x * x + y * y;
    double xd, yd;
    if (L.model == L3D_LENS_BROWN) {
        const double k1 = L.k[0], k2 = L.k[1], p1 = L.k[2], p2 = L.k[3], k3 = L.k[4], k4 = L.k[5], k5 = L.k[6], k6 = L.k[7];
        const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2, den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
        const double kr = num / den;
        xd = x * kr + ((2.0 * p1) * x * y + p2 * (r2 + 2.0 * (x * x)));
        yd = y * kr + (p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * x * y);
    } else {
        const double r = sqrt(r2), th = atan(r), t2 = th * th;
        const double td = th * (1.0 + (((L.k[3] * t2 + L.k[2]) * t2 + L.k[1]) * t2 + L.k[0]) * t2);
        const double s = r > 1e-8 ? td / r : 1.0;
        xd = x * s; yd = y * s;
    }
    u = L.fx * xd + L.cx; v = L.fy * yd + L.cy;
}

// the mask byte a sample reads, against the threshold.  The comparisons are made in double, before any conversion to an integer: a position that is
// not finite, or outside the mask, is invalid and no address is formed from it
L3D_SM_HD bool sample_valid(const Plan& p, const Seg& g, int k)
{
    double u, v;
    sample_pos(g, k, u, v);
    if (p.lens_on) { const double px = u, py = v; lens_map(p.L, px, py, u, v); }
    const double fu = floor(u + 0.5), fv = floor(v + 0.5);
    if (!(fu >= 0.0 && fu < (double)p.mw && fv >= 0.0 && fv < (double)p.mh)) return false;
    return (int)p.mask[(size_t)(int)fv * p.stride + (size_t)(int)fu] >= p.threshold;
}

// ---- runs, on the validity words (bit j of a word: sample base + j).  The open run [a, last] grows over a gap of at most max_gap invalid samples;
// a wider gap closes it.  Closed runs go to `on_run` in ascending order, single samples (a == last) included
struct Runs { int a, last, max_gap; };

template <class F> L3D_SM_HD void runs_word(Runs& r, uint64_t w, int base, F& on_run)
{
    while (w) {
        const int s = __builtin_ctzll(w);
        const uint64_t inv = ~(w >> s);
        const int len = inv ? __builtin_ctzll(inv) : 64;          // (inv == 0: the word is all ones)
        const int lo = base + s, hi = lo + len - 1;
        if (r.a >= 0 && lo - r.last - 1 <= r.max_gap) r.last = hi;
        else {
            if (r.a >= 0) on_run(r.a, r.last);
            r.a = lo; r.last = hi;
        }
        w = s + len >= 64 ? 0 : (w >> (s + len)) << (s + len);
    }
}
template <class F> L3D_SM_HD void runs_end(Runs& r, F& on_run)
{
    if (r.a >= 0) on_run(r.a, r.last);
    r.a = -1;
}

// the length test of a run
L3D_SM_HD bool run_passes(const Plan& p, const Seg& g, int a, int b)
{
    const double s = (double)(b - a) / (double)g.n, L2 = g.dx * g.dx + g.dy * g.dy;
    return (s * s) * L2 >= p.min_length * p.min_length;
}

// the run [a, b] as a segment: the samples rounded to f32, the input's own bits at the input's ends
L3D_SM_HD void run_segment(const Seg& g, const float* s, int a, int b, float* o)
{
    double px, py;
    if (a == 0) { o[0] = s[0]; o[1] = s[1]; }
    else { sample_pos(g, a, px, py); o[0] = (float)px; o[1] = (float)py; }
    if (b == g.n) { o[2] = s[2]; o[3] = s[3]; }
    else { sample_pos(g, b, px, py); o[2] = (float)px; o[3] = (float)py; }
}

// what happens to the runs of one segment: SPLIT hands every passing run on, CLIP remembers the longest (the first on a tie)
template <class Out> struct RunSink {
    const Plan& p; const Seg& g; const float* s; Out& out;
    int best_a, best_b;
    L3D_SM_HD RunSink(const Plan& p_, const Seg& g_, const float* s_, Out& out_) : p(p_), g(g_), s(s_), out(out_), best_a(0), best_b(0) {}
    L3D_SM_HD void operator()(int a, int b)
    {
        if (a >= b) return;
        if (p.mode == L3D_SEGMASK_SPLIT) {
            if (run_passes(p, g, a, b)) { float o[4]; run_segment(g, s, a, b, o); out.put(o); }
        } else if (b - a > best_b - best_a) { best_a = a; best_b = b; }
    }
};

// One segment through the mask.  wv.ballot(f): the 64-bit word whose bit `lane` is f(lane), the same value in every lane -- so everything behind it is
// uniform across the wave and every lane takes the same decisions.  out.put(4 floats): an output segment, in order along the input
template <class Wave, class Out> L3D_SM_HD void mask_segment(Wave& wv, const Plan& p, const float* s, Out& out)
{
    Seg g;
    if (!seg_setup(s, g)) return;
    const int ns = g.n + 1;
    if (p.mode == L3D_SEGMASK_DROP) {
        long long V = 0;
        for (int base = 0; base < ns; base += 64) {
            const uint64_t w = wv.ballot([&](int lane) { const int k = base + lane; return k < ns && sample_valid(p, g, k); });
            V += (long long)__builtin_popcountll(w);
        }
        if (V * 1000ll >= (long long)p.keep_permille * (long long)ns) out.put(s);
        return;
    }
    Runs r{ -1, 0, p.max_gap };
    RunSink<Out> sink(p, g, s, out);
    for (int base = 0; base < ns; base += 64) {
        const uint64_t w = wv.ballot([&](int lane) { const int k = base + lane; return k < ns && sample_valid(p, g, k); });
        runs_word(r, w, base, sink);
    }
    runs_end(r, sink);
    if (p.mode == L3D_SEGMASK_CLIP && sink.best_b > sink.best_a && run_passes(p, g, sink.best_a, sink.best_b)) {
        float o[4];
        run_segment(g, s, sink.best_a, sink.best_b, o);
        out.put(o);
    }
}

// ---- the host's wave and the whole call on the host
struct HostWave {
    template <class F> uint64_t ballot(F f)
    {
        uint64_t w = 0;
        for (int lane = 0; lane < 64; ++lane) if (f(lane)) w |= (uint64_t)1 << lane;
        return w;
    }
};
struct HostOut {
    std::vector<float>& segs; std::vector<int32_t>& src; int32_t index;
    void put(const float* o) { segs.insert(segs.end(), o, o + 4); src.push_back(index); }
};
inline void run_host(const Plan& p, const float* segments, int n, std::vector<float>& segs, std::vector<int32_t>& src)
{
    HostWave wv;
    for (int i = 0; i < n; ++i) {
        HostOut out{ segs, src, (int32_t)i };
        mask_segment(wv, p, segments + 4 * (size_t)i, out);
    }
}

}  // namespace segmask
}  // namespace l3d
