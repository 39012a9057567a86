// l3d_detect.hip -- line segment detection on the device: what Line3D::detectLineSegments (line3D.cc:1789-1871) does with the
// LSD detector (scale 0.8, sigma_scale 0.6, quant 2, ang_th 22.5 deg, log_eps 0, density_th 0.7), for gfx950.
//
// The pixel stage (rescale, grey, Gaussian sub-sampling, 2x2 gradient, level-line angle) and the rectangle / NFA arithmetic follow the
// detector's definitions.  Its region growing is a sequential greedy loop over a seed order and has no parallel equivalent, so the
// support regions are formed WITHOUT a seed order (Burns' scheme):
//   * level-line angles fall in buckets of 45 deg (= 2 ang_th), in two partitions shifted by 22.5 deg;
//   * the 8-connected components of equal bucket are labelled in each partition (hook by atomicMin + compress, to a fixed point);
//   * every pixel joins the larger of its two components (tie: partition 0).  A region is the set of pixels that chose it.
// Per region (one wave, pixels in ascending index order): gradient-weighted centre, inertia axis flipped towards the mean angle,
// extents -> rectangle, density; below 0.7 the region shrinks about its strongest pixel (radius x 0.75 per step from the farther end
// point, rectangle recomputed); NFA by the binomial tail with the log-gamma shortcut, and the rectangle variations of the detector for a
// region that fails it.  Pixels shed by the shrink, and regions that fail, are RELEASED and go through labelling again: three rounds.
// The result therefore AGREES with the reference detector (tests/detect_metric.py) and is not identical to it.  It is deterministic:
// labels are component minima, sizes and votes are integer atomics, every floating-point sum runs in a fixed order (no float atomics),
// and the final order is (length descending, smallest pixel index).
#include "l3d_detect.hpp"

#include <cmath>

#include "l3d_ctx.hpp"
#include "l3d_sort.hpp"

namespace l3d {
namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kNotDef = -1024.0;
constexpr double kScale = 0.8, kSigmaScale = 0.6, kQuant = 2.0, kAngTh = 22.5, kDensityTh = 0.7;
constexpr int kTaps = 7, kHalf = 3;         // sigma = 0.6 / 0.8: h = ceil(sigma sqrt(6 ln 10)) = 3
constexpr int kRounds = 3;

struct DetCand { double x1, y1, x2, y2; unsigned minpix, pad; };

// ---- rescale (bilinear, half-pixel centres, 8-bit weights) + grey: the integer formulas stated in include/line3d_amd.h
__device__ inline void axis_taps(int i, int n_out, int n_in, int& i0, int& i1, int& a)
{
    long long num = (2ll * i + 1) * n_in - n_out;
    if (num < 0) num = 0;
    const long long den = 2ll * n_out;
    i0 = (int)(num / den);
    a = (int)(((num % den) * 256 + den / 2) / den);
    if (i0 >= n_in - 1) { i0 = n_in - 1; a = 0; }
    i1 = min(i0 + 1, n_in - 1);
}
__global__ void k_det_grey(const unsigned char* __restrict__ px, int w, int h, int ch, int nw, int nh, float* __restrict__ grey)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= nw || y >= nh) return;
    int v[3] = { 0, 0, 0 };
    if (nw == w && nh == h) {
        for (int k = 0; k < ch; ++k) v[k] = px[((size_t)y * w + x) * ch + k];
    } else {
        int x0, x1, a, y0, y1, b;
        axis_taps(x, nw, w, x0, x1, a);
        axis_taps(y, nh, h, y0, y1, b);
        for (int k = 0; k < ch; ++k) {
            const int p00 = px[((size_t)y0 * w + x0) * ch + k], p01 = px[((size_t)y0 * w + x1) * ch + k];
            const int p10 = px[((size_t)y1 * w + x0) * ch + k], p11 = px[((size_t)y1 * w + x1) * ch + k];
            v[k] = ((256 - a) * (256 - b) * p00 + a * (256 - b) * p01 + (256 - a) * b * p10 + a * b * p11 + 32768) >> 16;
        }
    }
    const int g = ch == 1 ? v[0] : (299 * v[0] + 587 * v[1] + 114 * v[2] + 500) / 1000;
    grey[(size_t)y * nw + x] = (float)g;
}

// ---- Gaussian sub-sampling, separable, 7 taps; centres and weights per output column / row come from the host (computed as the
// detector computes them); symmetric boundary
__device__ inline int sym_index(int j, int n)
{
    const int d = 2 * n;
    j %= d;
    if (j < 0) j += d;
    return j >= n ? d - 1 - j : j;
}
constexpr int kXSpan = 96, kYRows = 16, kYSpan = 28;
__global__ __launch_bounds__(256) void k_det_gauss_x(const float* __restrict__ grey, int W, int H, double* __restrict__ aux, int N,
                                                      const int* __restrict__ xc, const double* __restrict__ kw)
{
    __shared__ float tile[4][kXSpan];
    const int x0 = blockIdx.x * 64, y = blockIdx.y * 4 + threadIdx.y, xl = min(x0 + 63, N - 1);
    const int lo = xc[x0] - kHalf, span = min(xc[xl] + kHalf - lo + 1, kXSpan);
    if (y < H)
        for (int t = threadIdx.x; t < span; t += 64) tile[threadIdx.y][t] = grey[(size_t)y * W + sym_index(lo + t, W)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= N || y >= H) return;
    const int base = xc[x] - kHalf - lo;
    if (base < 0 || base + kTaps > kXSpan) return;
    double sum = 0.0;
    for (int i = 0; i < kTaps; ++i) sum += (double)tile[threadIdx.y][base + i] * kw[(size_t)x * kTaps + i];
    aux[(size_t)y * N + x] = sum;
}
__global__ __launch_bounds__(256) void k_det_gauss_y(const double* __restrict__ aux, int N, int H, double* __restrict__ img, int M,
                                                      const int* __restrict__ yc, const double* __restrict__ kw)
{
    __shared__ double tile[kYSpan][64];
    const int x = blockIdx.x * 64 + threadIdx.x, y0 = blockIdx.y * kYRows, yl = min(y0 + kYRows - 1, M - 1);
    const int lo = yc[y0] - kHalf, span = min(yc[yl] + kHalf - lo + 1, kYSpan);
    for (int r = threadIdx.y; r < span; r += 4) tile[r][threadIdx.x] = x < N ? aux[(size_t)sym_index(lo + r, H) * N + x] : 0.0;
    __syncthreads();
    if (x >= N) return;
    for (int k = threadIdx.y; k < kYRows; k += 4) {
        const int y = y0 + k;
        if (y >= M) break;
        const int base = yc[y] - kHalf - lo;
        if (base < 0 || base + kTaps > kYSpan) continue;
        double sum = 0.0;
        for (int i = 0; i < kTaps; ++i) sum += tile[base + i][threadIdx.x] * kw[(size_t)y * kTaps + i];
        img[(size_t)y * N + x] = sum;
    }
}

// ---- 2x2 gradient, level-line angle, the two buckets; a pixel with a defined angle starts active
__global__ void k_det_grad(const double* __restrict__ img, int N, int M, double rho, double* __restrict__ mod, double* __restrict__ ang,
                           uchar2* __restrict__ bucket, unsigned char* __restrict__ active)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= N || y >= M) return;
    const size_t i = (size_t)y * N + x;
    double m = 0.0, a = kNotDef;
    if (x < N - 1 && y < M - 1) {
        const double com1 = img[i + N + 1] - img[i], com2 = img[i + 1] - img[i + N];
        const double gx = com1 + com2, gy = com1 - com2;
        m = sqrt((gx * gx + gy * gy) / 4.0);
        if (m > rho) a = atan2(gx, -gy);
    }
    mod[i] = m;
    ang[i] = a;
    uchar2 b = make_uchar2(255, 255);
    if (a != kNotDef) {
        const double t = (a + kPi) / (kPi / 4.0);
        b.x = (unsigned char)(((int)floor(t)) & 7);
        b.y = (unsigned char)(((int)floor(t + 0.5)) & 7);
    }
    bucket[i] = b;
    active[i] = a != kNotDef;
}

// ---- labelling: both partitions in one grid (blockIdx.y); another workgroup's parents are touched through atomics only
__global__ void k_det_label_init(const unsigned char* __restrict__ active, int np, int* __restrict__ parent)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const int v = active[i] ? i : -1;
    parent[i] = v;
    parent[np + i] = v;
}
__device__ inline int det_root(int* par, int a)
{
    int r = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (r != a) { a = r; r = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return a;
}
__global__ void k_det_label_hook(const uchar2* __restrict__ bucket, const unsigned char* __restrict__ active, int N, int M, int* __restrict__ parent,
                                 int* __restrict__ changed)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= N || y >= M) return;
    const int i = y * N + x;
    if (!active[i]) return;
    int* par = parent + (size_t)p * N * M;
    const unsigned char bi = p ? bucket[i].y : bucket[i].x;
    const int nx[4] = { x + 1, x - 1, x, x + 1 }, ny[4] = { y, y + 1, y + 1, y + 1 };
    for (int k = 0; k < 4; ++k) {
        if (nx[k] < 0 || nx[k] >= N || ny[k] >= M) continue;
        const int j = ny[k] * N + nx[k];
        if (!active[j]) continue;
        const unsigned char bj = p ? bucket[j].y : bucket[j].x;
        if (bj != bi) continue;
        const int a = det_root(par, i), b = det_root(par, j);      // (labels only decrease: a stale read costs another round)
        if (a != b) { atomicMin(&par[max(a, b)], min(a, b)); *changed = 1; }
    }
}
__global__ void k_det_label_compress(int* __restrict__ parent, int n2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2) return;
    int r = parent[i];
    if (r < 0) return;
    const int base = i - (i % (n2 / 2));
    while (true) { const int q = parent[base + r]; if (q == r) break; r = q; }
    parent[i] = r;
}

// ---- component sizes, then the vote: region key = partition * np + root; inactive pixels get the key 2 np (sorted last)
__global__ void k_det_sizes(const int* __restrict__ parent, int np, int* __restrict__ size)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * np) return;
    const int r = parent[i];
    if (r >= 0) atomicAdd(&size[(i >= np ? np : 0) + r], 1);
}
__global__ void k_det_vote(const int* __restrict__ parent, const int* __restrict__ size, int np, unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                           int* __restrict__ count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    vals[i] = (unsigned)i;
    const int r0 = parent[i], r1 = parent[np + i];
    if (r0 < 0) { keys[i] = 2u * (unsigned)np; return; }
    const unsigned key = size[np + r1] > size[r0] ? (unsigned)np + (unsigned)r1 : (unsigned)r0;
    keys[i] = key;
    atomicAdd(&count[key], 1);
}
// after the stable sort by key (pixels of a region are contiguous, ascending index): flag the first pixel of every region large enough
__global__ void k_det_heads(const unsigned* __restrict__ keys, const int* __restrict__ count, int np, int min_reg, int* __restrict__ flag)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > np) return;
    int f = 0;
    if (j < np) {
        const unsigned k = keys[j];
        f = k < 2u * (unsigned)np && (j == 0 || keys[j - 1] != k) && count[k] >= min_reg;
    }
    flag[j] = f;
}
__global__ void k_det_starts(const int* __restrict__ flag, const int* __restrict__ pos, int np, int* __restrict__ start)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < np && flag[j]) start[pos[j]] = j;
}

// ---- the region kernel
__device__ inline double wsum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ inline int wsumi(int v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ inline double wmin(double v) { for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o)); return v; }
__device__ inline double wmax(double v) { for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o)); return v; }
__device__ inline unsigned wminu(unsigned v) { for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o)); return v; }

__device__ inline double angle_dist(double a, double b)
{
    a -= b;
    while (a <= -kPi) a += 2.0 * kPi;
    while (a > kPi) a -= 2.0 * kPi;
    return fabs(a);
}
__device__ inline double lgamma_short(double x)
{
    if (x > 15.0)       // Windschitl
        return 0.918938533204673 + (x - 0.5) * log(x) - x + 0.5 * x * log(x * sinh(1.0 / x) + 1.0 / (810.0 * pow(x, 6.0)));
    const double q[7] = { 75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424, 2.50662827511 };     // Lanczos
    double a = (x + 0.5) * log(x + 5.5) - (x + 5.5), b = 0.0, xn = 1.0;
    for (int n = 0; n < 7; ++n) { a -= log(x + (double)n); b += q[n] * xn; xn *= x; }
    return a + log(b);
}
// -log10(number of false alarms) of k aligned among n points, probability p
__device__ double det_nfa(int n, int k, double p, double logNT)
{
    if (n == 0 || k == 0) return -logNT;
    if (n == k) return -logNT - (double)n * log10(p);
    const double p_term = p / (1.0 - p);
    const double log1 = lgamma_short((double)n + 1.0) - lgamma_short((double)k + 1.0) - lgamma_short((double)(n - k) + 1.0) + (double)k * log(p) +
                        (double)(n - k) * log(1.0 - p);
    double term = exp(log1);
    if (fabs(term) <= 2.2250738585072014e-308 * 100.0 || term == 0.0)
        return (double)k > (double)n * p ? -log1 / 2.30258509299404568402 - logNT : -logNT;
    double tail = term;
    for (int i = k + 1; i <= n; ++i) {
        const double bin = (double)(n - i + 1) * (1.0 / (double)i), mult = bin * p_term;
        term *= mult;
        tail += term;
        if (bin < 1.0) {
            const double err = term * ((1.0 - pow(mult, (double)(n - i + 1))) / (1.0 - mult) - 1.0);
            if (err < 0.1 * fabs(-log10(tail) - logNT) * tail) break;
        }
    }
    return -log10(tail) - logNT;
}

struct DetRect { double x1, y1, x2, y2, width, dx, dy, theta, prec, p; };

// pixels whose centre lies in the rectangle / those aligned with it within prec: lanes over the bounding box
__device__ double rect_score(const DetRect& r, const double* __restrict__ ang, int N, int M, double logNT, int lane)
{
    const double hx = -r.dy * r.width * 0.5, hy = r.dx * r.width * 0.5;
    const double minx = fmin(fmin(r.x1 - hx, r.x1 + hx), fmin(r.x2 - hx, r.x2 + hx)), maxx = fmax(fmax(r.x1 - hx, r.x1 + hx), fmax(r.x2 - hx, r.x2 + hx));
    const double miny = fmin(fmin(r.y1 - hy, r.y1 + hy), fmin(r.y2 - hy, r.y2 + hy)), maxy = fmax(fmax(r.y1 - hy, r.y1 + hy), fmax(r.y2 - hy, r.y2 + hy));
    const int ix0 = max(0, (int)floor(minx)), ix1 = min(N - 1, (int)ceil(maxx)), iy0 = max(0, (int)floor(miny)), iy1 = min(M - 1, (int)ceil(maxy));
    const int bw = ix1 - ix0 + 1, bh = iy1 - iy0 + 1;
    int pts = 0, alg = 0;
    if (bw > 0 && bh > 0) {
        const double len = sqrt((r.x2 - r.x1) * (r.x2 - r.x1) + (r.y2 - r.y1) * (r.y2 - r.y1)), hw = r.width * 0.5;
        const long long tot = (long long)bw * bh;
        for (long long k = lane; k < tot; k += 64) {
            const int x = ix0 + (int)(k % bw), y = iy0 + (int)(k / bw);
            const double ux = (double)x - r.x1, uy = (double)y - r.y1;
            const double a = ux * r.dx + uy * r.dy, b = -ux * r.dy + uy * r.dx;
            if (a < 0.0 || a > len || fabs(b) > hw) continue;
            ++pts;
            const double t = ang[(size_t)y * N + x];
            if (t == kNotDef) continue;
            double d = fabs(r.theta - t);
            if (d > 1.5 * kPi) d = fabs(d - 2.0 * kPi);
            alg += d <= r.prec;
        }
    }
    pts = wsumi(pts);
    alg = wsumi(alg);
    return det_nfa(pts, alg, r.p, logNT);
}

// the rectangle variations tried for a region that fails the NFA: finer precision, narrower, one side in, the other side in, finer again
__device__ double rect_retry(DetRect& rec, const double* __restrict__ ang, int N, int M, double logNT, int lane)
{
    double best = rect_score(rec, ang, N, M, logNT, lane);
    if (best > 0.0) return best;
    for (int stage = 0; stage < 5; ++stage) {
        DetRect r = rec;
        for (int n = 0; n < 5; ++n) {
            if (stage == 0 || stage == 4) { r.p *= 0.5; r.prec = r.p * kPi; }
            else {
                if (r.width - 0.5 < 0.5) continue;
                const double s = stage == 1 ? 0.0 : stage == 2 ? 0.25 : -0.25;
                r.x1 += -r.dy * s; r.y1 += r.dx * s; r.x2 += -r.dy * s; r.y2 += r.dx * s;
                r.width -= 0.5;
            }
            const double v = rect_score(r, ang, N, M, logNT, lane);
            if (v > best) { best = v; rec = r; }
        }
        if (best > 0.0) return best;
    }
    return best;
}

__global__ __launch_bounds__(256) void k_det_region(int N, int M, double logNT, int min_reg, const double* __restrict__ mod, const double* __restrict__ ang,
                                                     const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, const int* __restrict__ count,
                                                     const int* __restrict__ start, const int* __restrict__ n_regions, unsigned char* __restrict__ active,
                                                     DetCand* __restrict__ cand, int* __restrict__ n_cand, int cand_cap)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const int n_reg = *n_regions;
    const double prec = kPi * kAngTh / 180.0, p = kAngTh / 180.0;
    for (int reg = wave; reg < n_reg; reg += n_waves) {
        const int s0 = start[reg], n_all = count[keys[s0]];
        const unsigned* px = vals + s0;
        // the strongest pixel (tie: the smallest index): the centre the region shrinks about
        double best_m = -1.0;
        unsigned best_i = 0xffffffffu;
        for (int i = lane; i < n_all; i += 64) {
            const double m = mod[px[i]];
            if (m > best_m) { best_m = m; best_i = px[i]; }
        }
        const double top = wmax(best_m);
        const unsigned seed = wminu(best_m == top ? best_i : 0xffffffffu);
        const double sx = (double)(seed % (unsigned)N), sy = (double)(seed / (unsigned)N);
        double rad = -1.0;                      // < 0: the whole region
        DetRect rec;
        for (int step = 0; step < 64; ++step) {
            double w = 0, wx = 0, wy = 0, cdx = 0, cdy = 0;
            int n = 0;
            unsigned first = 0xffffffffu;
            for (int i = lane; i < n_all; i += 64) {
                const unsigned q = px[i];
                const double x = (double)(q % (unsigned)N), y = (double)(q / (unsigned)N);
                if (rad >= 0.0 && sqrt((x - sx) * (x - sx) + (y - sy) * (y - sy)) > rad) continue;
                const double m = mod[q], t = ang[q];
                w += m; wx += x * m; wy += y * m; cdx += cos(t); cdy += sin(t);
                ++n;
                first = min(first, q);
            }
            n = wsumi(n);
            if (n < min_reg || n < 2) break;
            w = wsum(w); wx = wsum(wx); wy = wsum(wy); cdx = wsum(cdx); cdy = wsum(cdy);
            first = wminu(first);
            if (!(w > 0.0)) break;
            const double cx = wx / w, cy = wy / w;
            double ixx = 0, iyy = 0, ixy = 0;
            for (int i = lane; i < n_all; i += 64) {
                const unsigned q = px[i];
                const double x = (double)(q % (unsigned)N), y = (double)(q / (unsigned)N);
                if (rad >= 0.0 && sqrt((x - sx) * (x - sx) + (y - sy) * (y - sy)) > rad) continue;
                const double m = mod[q];
                ixx += (y - cy) * (y - cy) * m; iyy += (x - cx) * (x - cx) * m; ixy -= (x - cx) * (y - cy) * m;
            }
            ixx = wsum(ixx); iyy = wsum(iyy); ixy = wsum(ixy);
            const double lambda = 0.5 * (ixx + iyy - sqrt((ixx - iyy) * (ixx - iyy) + 4.0 * ixy * ixy));
            double theta = fabs(ixx) > fabs(iyy) ? atan2(lambda - ixx, ixy) : atan2(ixy, lambda - iyy);
            if (angle_dist(theta, atan2(cdy, cdx)) > prec) theta += kPi;
            const double dx = cos(theta), dy = sin(theta);
            double lmin = 0, lmax = 0, wmn = 0, wmx = 0;
            for (int i = lane; i < n_all; i += 64) {
                const unsigned q = px[i];
                const double x = (double)(q % (unsigned)N), y = (double)(q / (unsigned)N);
                if (rad >= 0.0 && sqrt((x - sx) * (x - sx) + (y - sy) * (y - sy)) > rad) continue;
                const double l = (x - cx) * dx + (y - cy) * dy, ww = -(x - cx) * dy + (y - cy) * dx;
                lmin = fmin(lmin, l); lmax = fmax(lmax, l); wmn = fmin(wmn, ww); wmx = fmax(wmx, ww);
            }
            lmin = wmin(lmin); lmax = wmax(lmax); wmn = wmin(wmn); wmx = wmax(wmx);
            rec.x1 = cx + lmin * dx; rec.y1 = cy + lmin * dy; rec.x2 = cx + lmax * dx; rec.y2 = cy + lmax * dy;
            rec.width = fmax(wmx - wmn, 1.0);
            rec.dx = dx; rec.dy = dy; rec.theta = theta; rec.prec = prec; rec.p = p;
            const double len = sqrt((rec.x2 - rec.x1) * (rec.x2 - rec.x1) + (rec.y2 - rec.y1) * (rec.y2 - rec.y1));
            if ((double)n / (len * rec.width) >= kDensityTh) {
                if (rect_retry(rec, ang, N, M, logNT, lane) > 0.0) {
                    if (lane == 0) {
                        const int slot = atomicAdd(n_cand, 1);
                        if (slot < cand_cap) {
                            DetCand c;
                            c.x1 = (rec.x1 + 0.5) / kScale; c.y1 = (rec.y1 + 0.5) / kScale; c.x2 = (rec.x2 + 0.5) / kScale; c.y2 = (rec.y2 + 0.5) / kScale;
                            c.minpix = first; c.pad = 0;
                            cand[slot] = c;
                        }
                    }
                    for (int i = lane; i < n_all; i += 64) {            // consumed: everything else of the region is released
                        const unsigned q = px[i];
                        const double x = (double)(q % (unsigned)N), y = (double)(q / (unsigned)N);
                        if (rad >= 0.0 && sqrt((x - sx) * (x - sx) + (y - sy) * (y - sy)) > rad) continue;
                        active[q] = 0;
                    }
                }
                break;
            }
            if (rad < 0.0) {
                const double r1 = sqrt((sx - rec.x1) * (sx - rec.x1) + (sy - rec.y1) * (sy - rec.y1)), r2 = sqrt((sx - rec.x2) * (sx - rec.x2) + (sy - rec.y2) * (sy - rec.y2));
                rad = fmax(r1, r2);
            }
            rad *= 0.75;
        }
    }
}

// ---- selection: float coordinates x upscale, length filter, (length descending, smallest pixel index), cap
__device__ inline float4 cand_coords(const DetCand& c, float up)
{
    return make_float4((float)c.x1 * up, (float)c.y1 * up, (float)c.x2 * up, (float)c.y2 * up);
}
__global__ void k_det_select_keys(const DetCand* __restrict__ cand, int n, float up, float min_length, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 s = cand_coords(cand[i], up);
    const float dx = s.x - s.z, dy = s.y - s.w, len = sqrtf(dx * dx + dy * dy);
    vals[i] = (unsigned)i;
    keys[i] = len > min_length ? ((unsigned long long)(~__float_as_uint(len)) << 32) | cand[i].minpix : ~0ull;
}
__global__ void k_det_select_gather(const DetCand* __restrict__ cand, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals, int n, int limit,
                                    float up, float4* __restrict__ out, int* __restrict__ n_out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || j >= limit || keys[j] == ~0ull) return;
    out[j] = cand_coords(cand[vals[j]], up);
    if (j + 1 == n || j + 1 == limit || keys[j + 1] == ~0ull) *n_out = j + 1;
}

// the Gaussian sampler's centre and weights of every output column (or row), as the detector computes them, on the host
void sampler_table(int n_out, double sigma, int* centre, double* weights)
{
    for (int x = 0; x < n_out; ++x) {
        const double xx = (double)x / kScale;
        const int xc = (int)floor(xx + 0.5);
        const double mean = (double)kHalf + xx - (double)xc;
        double sum = 0.0, *k = weights + (size_t)x * kTaps;
        for (int i = 0; i < kTaps; ++i) { const double v = ((double)i - mean) / sigma; k[i] = exp(-0.5 * v * v); sum += k[i]; }
        if (sum >= 0.0) for (int i = 0; i < kTaps; ++i) k[i] /= sum;
        centre[x] = xc;
    }
}

}  // namespace

int detect_segments(l3d_ctx* c, const unsigned char* pixels, int w, int h, int ch, size_t stride, int nw, int nh, float min_length, int max_segments,
                    std::vector<float>& out)
{
    out.clear();
    if (!c) return L3D_ERR_INVALID;
    if (!pixels || w < 8 || h < 8 || (ch != 1 && ch != 3) || stride < (size_t)w * ch) return fail(c, L3D_ERR_INVALID, "detect_segments: needs an image of at least 8x8 with 1 or 3 channels and a row stride of at least width x channels");
    if (nw <= 0 || nh <= 0) { nw = w; nh = h; }
    if (nw < 8 || nh < 8 || max_segments < 0) return fail(c, L3D_ERR_INVALID, "detect_segments: rescaled size below 8x8 or a negative cap");
    const int N = (int)ceil(nw * kScale), M = (int)ceil(nh * kScale);
    const long long np_ll = (long long)N * M;
    if (np_ll > (1ll << 30) || (long long)w * h * ch > (1ll << 31)) return fail(c, L3D_ERR_UNSUPPORTED, "detect_segments: image too large");
    const int np = (int)np_ll;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DetectBufs& d = c->det;
    const double prec = kPi * kAngTh / 180.0, rho = kQuant / sin(prec);
    const double logNT = 5.0 * (log10((double)N) + log10((double)M)) / 2.0 + log10(11.0);
    const int min_reg = std::max(2, (int)(-logNT / log10(kAngTh / 180.0)));
    const int cand_cap = np / min_reg + 16;
    float up = 1.0f;
    if (nw != w || nh != h) up = 1.0f / (0.5f * (float(nw) / float(w) + float(nh) / float(h)));

    // ---- scratch
    size_t sort_bytes = 0, sort2_bytes = 0, scan_bytes = 0;
    int key_bits = 1;
    while ((1ull << key_bits) <= 2ull * (unsigned long long)np) ++key_bits;
    HIPCHK(c, sort_pairs_u32_u32(nullptr, sort_bytes, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, np, 0, key_bits, st));
    HIPCHK(c, sort_pairs_u64_u32(nullptr, sort2_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, cand_cap, 0, 64, st));
    HIPCHK(c, exclusive_sum_int(nullptr, scan_bytes, (const int*)nullptr, (int*)nullptr, np + 1, st));
    HIPCHK(c, d.pixels.reserve((size_t)w * h * ch));
    HIPCHK(c, d.grey.reserve((size_t)nw * nh * 4));
    HIPCHK(c, d.aux.reserve((size_t)N * nh * 8));
    HIPCHK(c, d.img.reserve((size_t)np * 8));
    HIPCHK(c, d.mod.reserve((size_t)np * 8));
    HIPCHK(c, d.ang.reserve((size_t)np * 8));
    HIPCHK(c, d.bucket.reserve((size_t)np * 2));
    HIPCHK(c, d.active.reserve((size_t)np));
    HIPCHK(c, d.parent.reserve((size_t)np * 8));
    HIPCHK(c, d.size.reserve((size_t)np * 8));
    HIPCHK(c, d.count.reserve((size_t)np * 8 + 8));
    HIPCHK(c, d.keys.reserve((size_t)np * 4));
    HIPCHK(c, d.keys2.reserve((size_t)np * 4));
    HIPCHK(c, d.vals.reserve((size_t)np * 4));
    HIPCHK(c, d.vals2.reserve((size_t)np * 4));
    HIPCHK(c, d.flag.reserve((size_t)(np + 1) * 4));
    HIPCHK(c, d.pos.reserve((size_t)(np + 1) * 4));
    HIPCHK(c, d.start.reserve((size_t)cand_cap * 4 + (size_t)np / 2 * 4));
    HIPCHK(c, d.tmp.reserve(std::max(std::max(sort_bytes, sort2_bytes), scan_bytes)));
    HIPCHK(c, d.cand.reserve((size_t)cand_cap * sizeof(DetCand)));
    HIPCHK(c, d.ckeys.reserve((size_t)cand_cap * 8));
    HIPCHK(c, d.ckeys2.reserve((size_t)cand_cap * 8));
    HIPCHK(c, d.cvals.reserve((size_t)cand_cap * 4));
    HIPCHK(c, d.cvals2.reserve((size_t)cand_cap * 4));
    HIPCHK(c, d.out.reserve((size_t)std::max(1, std::min(max_segments, cand_cap)) * 16));
    HIPCHK(c, d.scal.reserve(64));
    int* scal = d.scal.as<int>();               // [0] changed, [1] changed (ignored rounds), [2] candidates, [3] selected
    if (d.tab_w != nw || d.tab_h != nh) {
        std::vector<int> centre((size_t)N + M);
        std::vector<double> weights(((size_t)N + M) * kTaps);
        sampler_table(N, kSigmaScale / kScale, centre.data(), weights.data());
        sampler_table(M, kSigmaScale / kScale, centre.data() + N, weights.data() + (size_t)N * kTaps);
        const size_t wb = weights.size() * 8, cb = centre.size() * 4;
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, d.ktab.reserve(wb + cb));
        HIPCHK(c, hipMemcpy(d.ktab.p, weights.data(), wb, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(static_cast<char*>(d.ktab.p) + wb, centre.data(), cb, hipMemcpyHostToDevice));
        d.tab_w = nw; d.tab_h = nh;
    }
    const double* kw = d.ktab.as<double>();
    const int* kc = reinterpret_cast<const int*>(static_cast<const char*>(d.ktab.p) + ((size_t)N + M) * kTaps * 8);

    // ---- pixel stage
    HIPCHK(c, hipMemcpy2DAsync(d.pixels.p, (size_t)w * ch, pixels, stride, (size_t)w * ch, (size_t)h, hipMemcpyHostToDevice, st));
    const dim3 b256(256);
    { ProfScope ps(c, "k_det_grey"); hipLaunchKernelGGL(k_det_grey, dim3((nw + 255) / 256, nh), b256, 0, st, d.pixels.as<unsigned char>(), w, h, ch, nw, nh, d.grey.as<float>()); }
    { ProfScope ps(c, "k_det_gauss_x"); hipLaunchKernelGGL(k_det_gauss_x, dim3((N + 63) / 64, (nh + 3) / 4), dim3(64, 4), 0, st, d.grey.as<float>(), nw, nh, d.aux.as<double>(), N, kc, kw); }
    { ProfScope ps(c, "k_det_gauss_y"); hipLaunchKernelGGL(k_det_gauss_y, dim3((N + 63) / 64, (M + kYRows - 1) / kYRows), dim3(64, 4), 0, st, d.aux.as<double>(), N, nh, d.img.as<double>(), M, kc + N, kw + (size_t)N * kTaps); }
    { ProfScope ps(c, "k_det_grad"); hipLaunchKernelGGL(k_det_grad, dim3((N + 255) / 256, M), b256, 0, st, d.img.as<double>(), N, M, rho, d.mod.as<double>(), d.ang.as<double>(), d.bucket.as<uchar2>(), d.active.as<unsigned char>()); }
    HIPCHK(c, hipMemsetAsync(scal, 0, 64, st));

    // ---- rounds: label, vote, sort, regions
    const dim3 gnp((np + 255) / 256), gnp1((np + 256) / 256), g2np((2 * np + 255) / 256);
    for (int round = 0; round < kRounds; ++round) {
        { ProfScope ps(c, "k_det_label_init"); hipLaunchKernelGGL(k_det_label_init, gnp, b256, 0, st, d.active.as<unsigned char>(), np, d.parent.as<int>()); }
        for (int it = 0; it < 64; ++it) {
            HIPCHK(c, hipMemsetAsync(scal, 0, 4, st));
            for (int r = 0; r < 3; ++r) {                       // a few hooking rounds per look at the flag
                { ProfScope ps(c, "k_det_label_hook"); hipLaunchKernelGGL(k_det_label_hook, dim3((N + 255) / 256, M, 2), b256, 0, st, d.bucket.as<uchar2>(), d.active.as<unsigned char>(), N, M, d.parent.as<int>(), scal + (r == 2 ? 0 : 1)); }
                { ProfScope ps(c, "k_det_label_compress"); hipLaunchKernelGGL(k_det_label_compress, g2np, b256, 0, st, d.parent.as<int>(), 2 * np); }
            }
            int changed = 0;
            HIPCHK(c, hipMemcpyAsync(&changed, scal, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (!changed) break;
            if (it == 63) return fail(c, L3D_ERR_UNSUPPORTED, "detect_segments: labelling did not converge");
        }
        HIPCHK(c, hipMemsetAsync(d.size.p, 0, (size_t)np * 8, st));
        HIPCHK(c, hipMemsetAsync(d.count.p, 0, (size_t)np * 8 + 8, st));
        { ProfScope ps(c, "k_det_sizes"); hipLaunchKernelGGL(k_det_sizes, g2np, b256, 0, st, d.parent.as<int>(), np, d.size.as<int>()); }
        { ProfScope ps(c, "k_det_vote"); hipLaunchKernelGGL(k_det_vote, gnp, b256, 0, st, d.parent.as<int>(), d.size.as<int>(), np, d.keys.as<unsigned>(), d.vals.as<unsigned>(), d.count.as<int>()); }
        { ProfScope ps(c, "det_sort_pixels"); size_t tb = d.tmp.cap; HIPCHK(c, sort_pairs_u32_u32(d.tmp.p, tb, d.keys.as<unsigned>(), d.keys2.as<unsigned>(), d.vals.as<unsigned>(), d.vals2.as<unsigned>(), np, 0, key_bits, st)); }
        { ProfScope ps(c, "k_det_heads"); hipLaunchKernelGGL(k_det_heads, gnp1, b256, 0, st, d.keys2.as<unsigned>(), d.count.as<int>(), np, min_reg, d.flag.as<int>()); }
        { size_t tb = d.tmp.cap; HIPCHK(c, exclusive_sum_int(d.tmp.p, tb, d.flag.as<int>(), d.pos.as<int>(), np + 1, st)); }
        { ProfScope ps(c, "k_det_starts"); hipLaunchKernelGGL(k_det_starts, gnp, b256, 0, st, d.flag.as<int>(), d.pos.as<int>(), np, d.start.as<int>()); }
        { ProfScope ps(c, "k_det_region"); hipLaunchKernelGGL(k_det_region, dim3(1024), b256, 0, st, N, M, logNT, min_reg, d.mod.as<double>(), d.ang.as<double>(), d.keys2.as<unsigned>(), d.vals2.as<unsigned>(), d.count.as<int>(), d.start.as<int>(), d.pos.as<int>() + np, d.active.as<unsigned char>(), d.cand.as<DetCand>(), scal + 2, cand_cap); }
    }

    // ---- selection
    int n_cand = 0;
    HIPCHK(c, hipMemcpyAsync(&n_cand, scal + 2, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    n_cand = std::min(n_cand, cand_cap);
    if (n_cand <= 0 || max_segments == 0) return L3D_OK;
    const dim3 gc((n_cand + 255) / 256);
    { ProfScope ps(c, "k_det_select_keys"); hipLaunchKernelGGL(k_det_select_keys, gc, b256, 0, st, d.cand.as<DetCand>(), n_cand, up, min_length, d.ckeys.as<unsigned long long>(), d.cvals.as<unsigned>()); }
    { size_t tb = d.tmp.cap; HIPCHK(c, sort_pairs_u64_u32(d.tmp.p, tb, d.ckeys.as<unsigned long long>(), d.ckeys2.as<unsigned long long>(), d.cvals.as<unsigned>(), d.cvals2.as<unsigned>(), n_cand, 0, 64, st)); }
    { ProfScope ps(c, "k_det_select_gather"); hipLaunchKernelGGL(k_det_select_gather, gc, b256, 0, st, d.cand.as<DetCand>(), d.ckeys2.as<unsigned long long>(), d.cvals2.as<unsigned>(), n_cand, max_segments, up, d.out.as<float4>(), scal + 3); }
    int n_out = 0;
    HIPCHK(c, hipMemcpyAsync(&n_out, scal + 3, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    n_out = std::max(0, std::min(n_out, std::min(n_cand, max_segments)));
    out.resize((size_t)n_out * 4);
    if (n_out) HIPCHK(c, hipMemcpy(out.data(), d.out.p, (size_t)n_out * 16, hipMemcpyDeviceToHost));
    return L3D_OK;
}

}  // namespace l3d

int l3d_detect_segments(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                        float min_length, int max_segments, float** segments, int* n)
{
    if (!c || !segments || !n) return L3D_ERR_INVALID;
    *segments = nullptr;
    *n = 0;
    std::vector<float> out;
    const int rc = l3d::detect_segments(c, pixels, width, height, channels, row_stride, new_width, new_height, min_length, max_segments, out);
    if (rc != L3D_OK) return rc;
    *n = (int)(out.size() / 4);
    float* p = static_cast<float*>(malloc(std::max<size_t>(16, out.size() * 4)));
    if (!p) return l3d::fail(c, L3D_ERR_INVALID, "detect_segments: out of memory");
    if (!out.empty()) memcpy(p, out.data(), out.size() * 4);
    *segments = p;
    return L3D_OK;
}
