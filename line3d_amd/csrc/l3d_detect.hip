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
//
// A BATCH: images with the same plan (w, h, ch, nw, nh) run B at a time through these kernels.  Every per-pixel array holds the B images one after the
// other (image b at b * np), the pixel kernels take the image from blockIdx.z, and from the labelling on the stack is ONE set of NP = B * np pixels:
// parents, region keys (partition * NP + root) and the pixel sort range over the stack, a region never leaves its image (the hook kernel links
// inside an image only), and the region kernel works in the image's own coordinates (pixel index minus b * np).  One image is a batch of one.
#include "l3d_detect.hpp"

#include <cmath>

#include "l3d_ctx.hpp"
#include "l3d_jpeg.hpp"
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
    px += (size_t)blockIdx.z * w * h * ch;
    grey += (size_t)blockIdx.z * nw * nh;
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
// the tap windows of a block's 64 columns / 16 rows fit its tile (the kernels skip an output whose window does not): the centres of outputs
// j apart lie at most floor(j / kScale) + 1 apart: 63 columns 79, + 7 taps = 86 <= 96; 15 rows 19, + 7 = 26 <= 28
static_assert((int)(63 / kScale) + 1 + kTaps <= kXSpan && (int)((kYRows - 1) / kScale) + 1 + kTaps <= kYSpan, "a block's taps exceed its tile");
__global__ __launch_bounds__(256) void k_det_gauss_x(const float* __restrict__ grey, int W, int H, double* __restrict__ aux, int N,
                                                      const int* __restrict__ xc, const double* __restrict__ kw)
{
    __shared__ float tile[4][kXSpan];
    grey += (size_t)blockIdx.z * W * H;
    aux += (size_t)blockIdx.z * N * H;
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
    aux += (size_t)blockIdx.z * N * H;
    img += (size_t)blockIdx.z * N * M;
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
    const size_t at = (size_t)blockIdx.z * N * M;       // the last row and column of EACH image have no gradient
    img += at; mod += at; ang += at; bucket += at; active += at;
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

// ---- the validity plane beside the pixel stages ("A REMAP" in include/line3d_amd.h): a gradient pixel is UNDEFINED if any pixel that contributed to
// its value is invalid.  Byte planes (non-zero = valid), one AND-pass per stage over that stage's taps, the image in blockIdx.z; then one kernel
// behind k_det_grad, which is left as it is.  A chunk without a plane launches none of these
// k_det_grey's taps: the pixel itself, or where it rescales the taps of axis_taps whose weight is not zero
__global__ void k_det_valid_grey(const unsigned char* __restrict__ v0, int w, int h, int nw, int nh, unsigned char* __restrict__ v1)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= nw || y >= nh) return;
    v0 += (size_t)blockIdx.z * w * h;
    v1 += (size_t)blockIdx.z * nw * nh;
    int x0, x1, a, y0, y1, b;
    axis_taps(x, nw, w, x0, x1, a);
    axis_taps(y, nh, h, y0, y1, b);
    bool ok = true;
    if ((256 - a) && (256 - b)) ok = ok && v0[(size_t)y0 * w + x0];
    if (a && (256 - b)) ok = ok && v0[(size_t)y0 * w + x1];
    if ((256 - a) && b) ok = ok && v0[(size_t)y1 * w + x0];
    if (a && b) ok = ok && v0[(size_t)y1 * w + x1];
    v1[(size_t)y * nw + x] = ok ? 255 : 0;
}
// k_det_gauss_x's seven taps about xc[x], symmetric boundary: v1 (W x H) -> v2 (N x H)
__global__ void k_det_valid_x(const unsigned char* __restrict__ v1, int W, int H, unsigned char* __restrict__ v2, int N, const int* __restrict__ xc)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= N || y >= H) return;
    v1 += (size_t)blockIdx.z * W * H + (size_t)y * W;
    v2 += (size_t)blockIdx.z * N * H;
    const int lo = xc[x] - kHalf;
    bool ok = true;
    for (int i = 0; i < kTaps; ++i) ok = ok && v1[sym_index(lo + i, W)];
    v2[(size_t)y * N + x] = ok ? 255 : 0;
}
// k_det_gauss_y's seven taps about yc[y]: v2 (N x H) -> v3 (N x M)
__global__ void k_det_valid_y(const unsigned char* __restrict__ v2, int N, int H, unsigned char* __restrict__ v3, int M, const int* __restrict__ yc)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= N || y >= M) return;
    v2 += (size_t)blockIdx.z * N * H;
    v3 += (size_t)blockIdx.z * N * M;
    const int lo = yc[y] - kHalf;
    bool ok = true;
    for (int i = 0; i < kTaps; ++i) ok = ok && v2[(size_t)sym_index(lo + i, H) * N + x];
    v3[(size_t)y * N + x] = ok ? 255 : 0;
}
// k_det_grad's 2 x 2 stencil (clipped at the last row and column, which have no gradient anyway); an undefined pixel gets what k_det_grad gives a
// pixel below the gradient threshold -- no magnitude, no angle, no bucket, inactive.  defined: 255 / 0, read by the tests' hook
__global__ void k_det_valid_apply(const unsigned char* __restrict__ v3, int N, int M, double* __restrict__ mod, double* __restrict__ ang, uchar2* __restrict__ bucket,
                                  unsigned char* __restrict__ active, unsigned char* __restrict__ defined)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= N || y >= M) return;
    const size_t at = (size_t)blockIdx.z * N * M;
    v3 += at;
    const int x1 = min(x + 1, N - 1), y1 = min(y + 1, M - 1);
    const bool ok = v3[(size_t)y * N + x] && v3[(size_t)y * N + x1] && v3[(size_t)y1 * N + x] && v3[(size_t)y1 * N + x1];
    const size_t i = at + (size_t)y * N + x;
    defined[i] = ok ? 255 : 0;
    if (ok) return;
    mod[i] = 0.0;
    ang[i] = kNotDef;
    bucket[i] = make_uchar2(255, 255);
    active[i] = 0;
}

// ---- labelling: both partitions of every image in one grid (blockIdx.z = 2 image + partition); another workgroup's parents are touched through
// atomics only.  np here and below, where no image size goes with it: the pixels of the whole stack; parents are indices into the stack
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
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, p = blockIdx.z & 1;
    if (x >= N || y >= M) return;
    const int at = (int)(blockIdx.z >> 1) * N * M;          // neighbours are sought within the image: x, y are its own
    const int i = at + y * N + x;
    if (!active[i]) return;
    int* par = parent + (size_t)p * (gridDim.z >> 1) * N * M;
    const unsigned char bi = p ? bucket[i].y : bucket[i].x;
    const int nx[4] = { x + 1, x - 1, x, x + 1 }, ny[4] = { y, y + 1, y + 1, y + 1 };
    for (int k = 0; k < 4; ++k) {
        if (nx[k] < 0 || nx[k] >= N || ny[k] >= M) continue;
        const int j = at + ny[k] * N + nx[k];
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
__device__ __forceinline__ double det_nfa(int n, int k, double p, double logNT)     // (inlined: the tests' kernel is a third caller)
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
struct DetScore { double v; int pts, alg; };      // the value; the counts it came from (read by the tests' trace only)
__device__ DetScore rect_score(const DetRect& r, const double* __restrict__ ang, int N, int M, double logNT, int lane)
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
    return DetScore{ det_nfa(pts, alg, r.p, logNT), pts, alg };
}

// the rectangle variations tried for a region that fails the NFA: finer precision, narrower, one side in, the other side in, finer again
__device__ DetScore rect_retry(DetRect& rec, const double* __restrict__ ang, int N, int M, double logNT, int lane)
{
    DetScore best = rect_score(rec, ang, N, M, logNT, lane);
    if (best.v > 0.0) return best;
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
            const DetScore v = rect_score(r, ang, N, M, logNT, lane);
            if (v.v > best.v) { best = v; rec = r; }
        }
        if (best.v > 0.0) return best;
    }
    return best;
}

// the waves range over the regions of all images of the stack.  A region lies in one image (vals / (N M)); its pixels are taken relative to that image,
// so coordinates, sums, the rectangle scan's clipping and minpix are what the image alone gives.  cand / n_cand: cand_cap slots and a counter per image
__global__ __launch_bounds__(256) void k_det_region(int N, int M, double logNT, int min_reg, const double* __restrict__ mod_all, const double* __restrict__ ang_all,
                                                     const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, const int* __restrict__ count,
                                                     const int* __restrict__ start, const int* __restrict__ n_regions, unsigned char* __restrict__ active_all,
                                                     DetCand* __restrict__ cand_all, int* __restrict__ n_cand_all, int cand_cap, l3d_detect_region_record* __restrict__ trace)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const int n_reg = *n_regions;
    const double prec = kPi * kAngTh / 180.0, p = kAngTh / 180.0;
    for (int reg = wave; reg < n_reg; reg += n_waves) {
        const int s0 = start[reg], n_all = count[keys[s0]];
        const unsigned* px = vals + s0;
        const unsigned image = px[0] / (unsigned)(N * M), at = image * (unsigned)(N * M);
        const double* mod = mod_all + at;
        const double* ang = ang_all + at;
        unsigned char* active = active_all + at;
        // the strongest pixel (tie: the smallest index): the centre the region shrinks about
        double best_m = -1.0;
        unsigned best_i = 0xffffffffu;
        for (int i = lane; i < n_all; i += 64) {
            const double m = mod[px[i] - at];
            if (m > best_m) { best_m = m; best_i = px[i] - at; }
        }
        const double top = wmax(best_m);
        const unsigned seed = wminu(best_m == top ? best_i : 0xffffffffu);
        const double sx = (double)(seed % (unsigned)N), sy = (double)(seed / (unsigned)N);
        double rad = -1.0;                      // < 0: the whole region
        DetRect rec;
        l3d_detect_region_record* tr = trace && lane == 0 ? trace + reg : nullptr;      // (tests only: what this wave decides; the caller zeroes it)
        if (tr) tr->minpix = px[0] - at;
        for (int step = 0; step < 64; ++step) {
            double w = 0, wx = 0, wy = 0, cdx = 0, cdy = 0;
            int n = 0;
            unsigned first = 0xffffffffu;
            for (int i = lane; i < n_all; i += 64) {
                const unsigned q = px[i] - at;
                const double x = (double)(q % (unsigned)N), y = (double)(q / (unsigned)N);
                if (rad >= 0.0 && sqrt((x - sx) * (x - sx) + (y - sy) * (y - sy)) > rad) continue;
                const double m = mod[q], t = ang[q];
                w += m; wx += x * m; wy += y * m; cdx += cos(t); cdy += sin(t);
                ++n;
                first = min(first, q);
            }
            n = wsumi(n);
            if (tr) { tr->steps = step; tr->n_used = n; if (step < 8) tr->hist_n[step] = n; }
            if (n < min_reg || n < 2) break;
            w = wsum(w); wx = wsum(wx); wy = wsum(wy); cdx = wsum(cdx); cdy = wsum(cdy);
            first = wminu(first);
            if (!(w > 0.0)) break;
            const double cx = wx / w, cy = wy / w;
            double ixx = 0, iyy = 0, ixy = 0;
            for (int i = lane; i < n_all; i += 64) {
                const unsigned q = px[i] - at;
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
                const unsigned q = px[i] - at;
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
            if (tr) {
                tr->minpix = first; tr->cx = cx; tr->cy = cy; tr->density = (double)n / (len * rec.width);
                tr->x1 = rec.x1; tr->y1 = rec.y1; tr->x2 = rec.x2; tr->y2 = rec.y2; tr->width = rec.width; tr->theta = theta;
            }
            if ((double)n / (len * rec.width) >= kDensityTh) {
                const DetScore score = rect_retry(rec, ang, N, M, logNT, lane);
                const double best = score.v;
                if (tr) {
                    tr->pts = score.pts; tr->alg = score.alg; tr->scored = 1; tr->accepted = best > 0.0;
                    tr->fx1 = rec.x1; tr->fy1 = rec.y1; tr->fx2 = rec.x2; tr->fy2 = rec.y2; tr->fwidth = rec.width; tr->p = rec.p; tr->nfa = best;
                }
                if (best > 0.0) {
                    if (lane == 0) {
                        const int slot = atomicAdd(n_cand_all + image, 1);
                        if (slot < cand_cap) {
                            DetCand c;
                            c.x1 = (rec.x1 + 0.5) / kScale; c.y1 = (rec.y1 + 0.5) / kScale; c.x2 = (rec.x2 + 0.5) / kScale; c.y2 = (rec.y2 + 0.5) / kScale;
                            c.minpix = first; c.pad = 0;
                            cand_all[(size_t)image * cand_cap + slot] = c;
                        }
                    }
                    for (int i = lane; i < n_all; i += 64) {            // consumed: everything else of the region is released
                        const unsigned q = px[i] - at;
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
// per image: its candidates (at most cand_cap) and the slots its segments can take (at most max_segments of them), as running sums over the chunk;
// the counts the gather will write start at zero
__global__ void k_det_select_plan(const int* __restrict__ n_cand, const DetImgParam* __restrict__ prm, int B, int cand_cap, int* __restrict__ coff, int* __restrict__ ooff,
                                  int* __restrict__ n_out)
{
    if (blockIdx.x || threadIdx.x) return;
    int c = 0, o = 0;
    for (int b = 0; b < B; ++b) {
        const int n = max(0, min(n_cand[b], cand_cap));
        coff[b] = c; ooff[b] = o; n_out[b] = 0;
        c += n; o += min(n, max(0, prm[b].max_segments));
    }
    coff[B] = c; ooff[B] = o;
}
// the candidates of all images, packed in image order (blockIdx.y: the image).  The key has no room for the image: the order of one image's
// candidates comes from the sort by this key, the images are put apart again by a stable sort on imgs (k_det_select_image)
__global__ void k_det_select_keys(const DetCand* __restrict__ cand, const int* __restrict__ coff, int cand_cap, float up, const DetImgParam* __restrict__ prm,
                                  unsigned long long* __restrict__ keys, unsigned* __restrict__ vals, unsigned* __restrict__ imgs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= coff[b + 1] - coff[b]) return;
    const DetCand& c = cand[(size_t)b * cand_cap + i];
    const float4 s = cand_coords(c, up);
    const float dx = s.x - s.z, dy = s.y - s.w, len = sqrtf(dx * dx + dy * dy);
    const int at = coff[b] + i;
    vals[at] = (unsigned)at;
    imgs[at] = (unsigned)b;
    keys[at] = len > prm[b].min_length ? ((unsigned long long)(~__float_as_uint(len)) << 32) | c.minpix : ~0ull;
}
__global__ void k_det_select_image(const unsigned* __restrict__ vals, const unsigned* __restrict__ imgs, int n, unsigned* __restrict__ img_sorted)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) img_sorted[j] = imgs[vals[j]];
}
// vals: the packed candidates, images apart, each image's by key.  keys, imgs: by packed index.  The image's r-th is its r-th segment
__global__ void k_det_select_gather(const DetCand* __restrict__ cand, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                    const unsigned* __restrict__ imgs, const int* __restrict__ coff, const int* __restrict__ ooff, int B, int cand_cap, float up,
                                    const DetImgParam* __restrict__ prm, float4* __restrict__ out, int* __restrict__ n_out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= coff[B]) return;
    const unsigned v = vals[j], b = imgs[v];
    const int r = j - coff[b], n = coff[b + 1] - coff[b], limit = prm[b].max_segments;
    if (r >= limit || keys[v] == ~0ull) return;
    out[ooff[b] + r] = cand_coords(cand[(size_t)b * cand_cap + (v - coff[b])], up);
    if (r + 1 == n || r + 1 == limit || keys[vals[j + 1]] == ~0ull) n_out[b] = r + 1;
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

namespace {

// what one chunk's run works at: sizes of an image and of its scaled image, thresholds, capacities (per image), and the images in the chunk
struct DetPlan {
    int w = 0, h = 0, ch = 1, nw = 0, nh = 0, N = 0, M = 0, np = 0, min_reg = 2, cand_cap = 0, key_bits = 1, B = 1;
    int sw = 0, sh = 0;                         // the size of the images as they arrive (a remap resamples them to w x h; otherwise w x h)
    double rho = 0.0, logNT = 0.0;
    float up = 1.0f;
    int stack() const { return B * np; }        // pixels of the chunk's stack (at most 2^30)
    bool same_group(const DetPlan& o) const { return w == o.w && h == o.h && ch == o.ch && nw == o.nw && nh == o.nh && sw == o.sw && sh == o.sh; }
};
// the pixel sort's keys reach 2 x the stack
void plan_chunk(DetPlan& p, int B)
{
    p.B = B;
    p.key_bits = 1;
    while ((1ull << p.key_bits) <= 2ull * (unsigned long long)B * (unsigned long long)p.np) ++p.key_bits;
}
// the part of the plan that follows from the scaled size alone
void plan_scaled(DetPlan& p, int N, int M)
{
    p.N = N; p.M = M; p.np = N * M;
    p.rho = kQuant / sin(kPi * kAngTh / 180.0);
    p.logNT = 5.0 * (log10((double)N) + log10((double)M)) / 2.0 + log10(11.0);
    p.min_reg = std::max(2, (int)(-p.logNT / log10(kAngTh / 180.0)));
    p.cand_cap = p.np / p.min_reg + 16;
    plan_chunk(p, 1);
}

// the scalars, ints: [0] changed, [1] changed (ignored rounds); from [16] per image: candidates | first packed candidate (B + 1) | first output slot (B + 1)
constexpr int kScalHead = 16;
inline int* det_n_cand(DetectBufs& d) { return d.scal.as<int>() + kScalHead; }
inline size_t det_out_head(int B) { return ((size_t)B * 4 + 15) & ~(size_t)15; }      // d.out: the images' segment counts, then the segments

// bytes of the device buffers one image of a chunk takes (what det_reserve sums up, with the buffers' slack): the chunk rule's memory term
size_t det_image_bytes(const DetPlan& p, WarpRoute route, size_t jpeg_blocks, bool valid)
{
    const bool undist = route != WarpRoute::None;
    const size_t np = (size_t)p.np, cc = (size_t)p.cand_cap;
    size_t b = (size_t)p.sw * p.sh * p.ch + (undist ? (size_t)p.w * p.h * p.ch : 0) + (size_t)p.nw * p.nh * 4 + (size_t)p.N * p.nh * 8;
    if (valid) b += (size_t)p.sw * p.sh + (size_t)p.w * p.h + (size_t)p.nw * p.nh + (size_t)p.N * p.nh + 2 * np;
    b += np * (8 + 8 + 8 + 2 + 1 + 8 + 8 + 8 + 4 * 4 + 4 + 4 + 2) + np * 16 /* the sorts' scratch */ + cc * (sizeof(DetCand) + 8 + 8 + 4 * 4 + 4 + 16);
    b += jpeg_blocks * (128 + 128 + 64);
    return b + b / 4;
}

// route, valid: the chunk's kernel and whether it carries validity planes (detect_chunk)
int det_reserve(l3d_ctx* c, const DetPlan& p, size_t out_slots, WarpRoute route = WarpRoute::None, bool valid = false)
{
    const bool undist = route != WarpRoute::None;
    hipStream_t st = c->stream;
    DetectBufs& d = c->det;
    const size_t B = (size_t)p.B, np = (size_t)p.stack(), cand_cap = (size_t)p.cand_cap * B;
    size_t sort_bytes = 0, sort2_bytes = 0, sort3_bytes = 0, scan_bytes = 0;
    HIPCHK(c, sort_pairs_u32_u32(nullptr, sort_bytes, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, (int)np, 0, p.key_bits, st));
    HIPCHK(c, sort_pairs_u64_u32(nullptr, sort2_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, (int)cand_cap, 0, 64, st));
    HIPCHK(c, sort_pairs_u32_u32(nullptr, sort3_bytes, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, (int)cand_cap, 0, 32, st));
    HIPCHK(c, exclusive_sum_int(nullptr, scan_bytes, (const int*)nullptr, (int*)nullptr, (int)np + 1, st));
    HIPCHK(c, d.pixels.reserve(B * p.sw * p.sh * p.ch));
    if (undist) HIPCHK(c, d.undist.reserve(B * p.w * p.h * p.ch));
    if (valid) {
        HIPCHK(c, d.valid.reserve(B * p.w * p.h));
        HIPCHK(c, d.vgrey.reserve(B * p.nw * p.nh));
        HIPCHK(c, d.vaux.reserve(B * p.N * p.nh));
        HIPCHK(c, d.vimg.reserve(np));
        HIPCHK(c, d.vdef.reserve(np));
    }
    HIPCHK(c, d.grey.reserve(B * p.nw * p.nh * 4));
    HIPCHK(c, d.aux.reserve(B * p.N * p.nh * 8));
    HIPCHK(c, d.img.reserve(np * 8));
    HIPCHK(c, d.mod.reserve(np * 8));
    HIPCHK(c, d.ang.reserve(np * 8));
    HIPCHK(c, d.bucket.reserve(np * 2));
    HIPCHK(c, d.active.reserve(np));
    HIPCHK(c, d.parent.reserve(np * 8));
    HIPCHK(c, d.size.reserve(np * 8));
    HIPCHK(c, d.count.reserve(np * 8 + 8));
    HIPCHK(c, d.keys.reserve(np * 4));
    HIPCHK(c, d.keys2.reserve(np * 4));
    HIPCHK(c, d.vals.reserve(np * 4));
    HIPCHK(c, d.vals2.reserve(np * 4));
    HIPCHK(c, d.flag.reserve((np + 1) * 4));
    HIPCHK(c, d.pos.reserve((np + 1) * 4));
    HIPCHK(c, d.start.reserve(cand_cap * 4 + np / 2 * 4));
    HIPCHK(c, d.tmp.reserve(std::max(std::max(sort_bytes, sort2_bytes), std::max(sort3_bytes, scan_bytes))));
    HIPCHK(c, d.cand.reserve(cand_cap * sizeof(DetCand)));
    HIPCHK(c, d.ckeys.reserve(cand_cap * 8));
    HIPCHK(c, d.ckeys2.reserve(cand_cap * 8));
    HIPCHK(c, d.cvals.reserve(cand_cap * 4));
    HIPCHK(c, d.cvals2.reserve(cand_cap * 4));
    HIPCHK(c, d.cimg.reserve(cand_cap * 4));
    HIPCHK(c, d.cimg2.reserve(cand_cap * 4));
    HIPCHK(c, d.out.reserve(det_out_head(p.B) + std::max<size_t>(1, out_slots) * 16));
    HIPCHK(c, d.prm.reserve(B * sizeof(DetImgParam)));
    HIPCHK(c, d.scal.reserve(((size_t)kScalHead + 3 * B + 2) * 4));
    return L3D_OK;
}
// the flags and the images' candidate counters
hipError_t det_zero_scalars(l3d_ctx* c, int B) { return hipMemsetAsync(c->det.scal.p, 0, ((size_t)kScalHead + B) * 4, c->stream); }

// image b of the chunk: host pixels into its slot of d.pixels
hipError_t det_upload(l3d_ctx* c, const DetPlan& p, int b, const unsigned char* pixels, size_t stride)
{
    const size_t row = (size_t)p.sw * p.ch;
    return hipMemcpy2DAsync(c->det.pixels.as<unsigned char>() + (size_t)b * row * p.sh, row, pixels, stride, row, (size_t)p.sh, hipMemcpyHostToDevice, c->stream);
}

// ---- pixel stage on the chunk's images in d.pixels (uploaded, or decoded JPEG): the chunk's undistortion kernel, rescale + grey, the two sampler passes,
// gradient -- one launch each, the image in blockIdx.z; leaves the scalars zeroed.  route: the strongest any image needs -- Radial reads the cameras
// in d.prm, Lens and Resample take every image's entry of lens_tab (host) and Resample every image's flags as well, and writes d.valid.  valid: d.valid
// holds the chunk's validity planes (w x h each) and is carried beside the stages
int det_pixel_stage(l3d_ctx* c, const DetPlan& p, WarpRoute route = WarpRoute::None, bool valid = false, const DetLens* lens_tab = nullptr, const int* remap_flags = nullptr)
{
    hipStream_t st = c->stream;
    DetectBufs& d = c->det;
    const int w = p.w, h = p.h, ch = p.ch, nw = p.nw, nh = p.nh, N = p.N, M = p.M, B = p.B;
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
    const dim3 b256(256);
    const unsigned char* image = d.pixels.as<unsigned char>();          // whichever buffer holds the images k_det_grey reads
    if (route == WarpRoute::Resample) { if (int rc = launch_undistort_remap(c, p.sw, p.sh, ch, w, h, B, lens_tab, remap_flags)) return rc; }
    else if (route == WarpRoute::Lens) { if (int rc = launch_undistort_lens(c, w, h, ch, B, lens_tab)) return rc; }
    else if (route == WarpRoute::Radial) launch_undistort(c, w, h, ch, B, DetCamera{ 1.0, 1.0, 0.0, 0.0, 0.0, 0.0 }, d.prm.as<DetImgParam>());
    if (route != WarpRoute::None) image = d.undist.as<unsigned char>();
    { ProfScope ps(c, "k_det_grey"); hipLaunchKernelGGL(k_det_grey, dim3((nw + 255) / 256, nh, B), b256, 0, st, image, w, h, ch, nw, nh, d.grey.as<float>()); }
    { ProfScope ps(c, "k_det_gauss_x"); hipLaunchKernelGGL(k_det_gauss_x, dim3((N + 63) / 64, (nh + 3) / 4, B), dim3(64, 4), 0, st, d.grey.as<float>(), nw, nh, d.aux.as<double>(), N, kc, kw); }
    { ProfScope ps(c, "k_det_gauss_y"); hipLaunchKernelGGL(k_det_gauss_y, dim3((N + 63) / 64, (M + kYRows - 1) / kYRows, B), dim3(64, 4), 0, st, d.aux.as<double>(), N, nh, d.img.as<double>(), M, kc + N, kw + (size_t)N * kTaps); }
    { ProfScope ps(c, "k_det_grad"); hipLaunchKernelGGL(k_det_grad, dim3((N + 255) / 256, M, B), b256, 0, st, d.img.as<double>(), N, M, p.rho, d.mod.as<double>(), d.ang.as<double>(), d.bucket.as<uchar2>(), d.active.as<unsigned char>()); }
    d.vdef_n = valid ? N : 0; d.vdef_m = valid ? M : 0;
    if (valid) {
        const bool rescaled = nw != w || nh != h;
        const unsigned char* v1 = rescaled ? d.vgrey.as<unsigned char>() : d.valid.as<unsigned char>();
        if (rescaled) { ProfScope ps(c, "k_det_valid_grey"); hipLaunchKernelGGL(k_det_valid_grey, dim3((nw + 255) / 256, nh, B), b256, 0, st, d.valid.as<unsigned char>(), w, h, nw, nh, d.vgrey.as<unsigned char>()); }
        { ProfScope ps(c, "k_det_valid_x"); hipLaunchKernelGGL(k_det_valid_x, dim3((N + 255) / 256, nh, B), b256, 0, st, v1, nw, nh, d.vaux.as<unsigned char>(), N, kc); }
        { ProfScope ps(c, "k_det_valid_y"); hipLaunchKernelGGL(k_det_valid_y, dim3((N + 255) / 256, M, B), b256, 0, st, d.vaux.as<unsigned char>(), N, nh, d.vimg.as<unsigned char>(), M, kc + N); }
        { ProfScope ps(c, "k_det_valid_apply"); hipLaunchKernelGGL(k_det_valid_apply, dim3((N + 255) / 256, M, B), b256, 0, st, d.vimg.as<unsigned char>(), N, M, d.mod.as<double>(), d.ang.as<double>(), d.bucket.as<uchar2>(), d.active.as<unsigned char>(), d.vdef.as<unsigned char>()); }
    }
    HIPCHK(c, det_zero_scalars(c, B));
    return L3D_OK;
}

// ---- labelling of the active pixels to the fixed point, component sizes, vote.  Between two compressions every tree is a star, and a
// hooking round that changes anything turns at least one root into a child: at most np - 1 rounds change something, three rounds a look.
// All images of the chunk share the grids and the flag: an image that has reached its fixed point sees further rounds, which change nothing in it
// (its labels are component minima already); the flag only ends the loop, after as many looks as the slowest image needs.
int det_label(l3d_ctx* c, const DetPlan& p)
{
    hipStream_t st = c->stream;
    DetectBufs& d = c->det;
    const int N = p.N, M = p.M, np = p.stack();
    int* scal = d.scal.as<int>();
    const dim3 b256(256), gnp((np + 255) / 256), g2np((unsigned)((2ll * np + 255) / 256));
    { ProfScope ps(c, "k_det_label_init"); hipLaunchKernelGGL(k_det_label_init, gnp, b256, 0, st, d.active.as<unsigned char>(), np, d.parent.as<int>()); }
    const int max_looks = p.np / 3 + 2;
    for (int it = 0; ; ++it) {
        HIPCHK(c, hipMemsetAsync(scal, 0, 4, st));
        for (int r = 0; r < 3; ++r) {                       // a few hooking rounds per look at the flag
            { ProfScope ps(c, "k_det_label_hook"); hipLaunchKernelGGL(k_det_label_hook, dim3((N + 255) / 256, M, 2 * p.B), b256, 0, st, d.bucket.as<uchar2>(), d.active.as<unsigned char>(), N, M, d.parent.as<int>(), scal + (r == 2 ? 0 : 1)); }
            { ProfScope ps(c, "k_det_label_compress"); hipLaunchKernelGGL(k_det_label_compress, g2np, b256, 0, st, d.parent.as<int>(), 2 * np); }
        }
        int changed = 0;
        HIPCHK(c, hipMemcpyAsync(&changed, scal, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (!changed) break;
        if (it + 1 >= max_looks) return fail(c, L3D_ERR_UNSUPPORTED, "detect_segments: labelling did not converge");
    }
    HIPCHK(c, hipMemsetAsync(d.size.p, 0, (size_t)np * 8, st));
    HIPCHK(c, hipMemsetAsync(d.count.p, 0, (size_t)np * 8 + 8, st));
    { ProfScope ps(c, "k_det_sizes"); hipLaunchKernelGGL(k_det_sizes, g2np, b256, 0, st, d.parent.as<int>(), np, d.size.as<int>()); }
    { ProfScope ps(c, "k_det_vote"); hipLaunchKernelGGL(k_det_vote, gnp, b256, 0, st, d.parent.as<int>(), d.size.as<int>(), np, d.keys.as<unsigned>(), d.vals.as<unsigned>(), d.count.as<int>()); }
    return L3D_OK;
}

// ---- regions of the labelling in keys / vals / count: sort, heads, scan, starts, the region kernel.  trace: null outside the tests
int det_regions(l3d_ctx* c, const DetPlan& p, l3d_detect_region_record* trace)
{
    hipStream_t st = c->stream;
    DetectBufs& d = c->det;
    const int N = p.N, M = p.M, np = p.stack();
    const dim3 b256(256), gnp((np + 255) / 256), gnp1((np + 256) / 256);
    { ProfScope ps(c, "det_sort_pixels"); size_t tb = d.tmp.cap; HIPCHK(c, sort_pairs_u32_u32(d.tmp.p, tb, d.keys.as<unsigned>(), d.keys2.as<unsigned>(), d.vals.as<unsigned>(), d.vals2.as<unsigned>(), np, 0, p.key_bits, st)); }
    { ProfScope ps(c, "k_det_heads"); hipLaunchKernelGGL(k_det_heads, gnp1, b256, 0, st, d.keys2.as<unsigned>(), d.count.as<int>(), np, p.min_reg, d.flag.as<int>()); }
    { size_t tb = d.tmp.cap; HIPCHK(c, exclusive_sum_int(d.tmp.p, tb, d.flag.as<int>(), d.pos.as<int>(), np + 1, st)); }
    { ProfScope ps(c, "k_det_starts"); hipLaunchKernelGGL(k_det_starts, gnp, b256, 0, st, d.flag.as<int>(), d.pos.as<int>(), np, d.start.as<int>()); }
    { ProfScope ps(c, "k_det_region"); hipLaunchKernelGGL(k_det_region, dim3(1024), b256, 0, st, N, M, p.logNT, p.min_reg, d.mod.as<double>(), d.ang.as<double>(), d.keys2.as<unsigned>(), d.vals2.as<unsigned>(), d.count.as<int>(), d.start.as<int>(), d.pos.as<int>() + np, d.active.as<unsigned char>(), d.cand.as<DetCand>(), det_n_cand(d), p.cand_cap, trace); }
    return L3D_OK;
}

__global__ void k_det_nfa_test(const int* __restrict__ n, const int* __restrict__ k, const double* __restrict__ p, double logNT, int count, double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = det_nfa(n[i], k[i], p[i], logNT);
}

// have_image: host pixels were given, or the image will be decoded on the device
int plan_image(DetPlan& p, bool have_image, int w, int h, int ch, size_t stride, int nw, int nh, std::string& err)
{
    if (!have_image || w < 8 || h < 8 || (ch != 1 && ch != 3) || stride < (size_t)w * ch) {
        err = "detect_segments: needs an image of at least 8x8 with 1 or 3 channels and a row stride of at least width x channels";
        return L3D_ERR_INVALID;
    }
    if (nw <= 0 || nh <= 0) { nw = w; nh = h; }
    if (nw < 8 || nh < 8) { err = "detect_segments: rescaled size below 8x8"; return L3D_ERR_INVALID; }
    const int N = (int)ceil(nw * kScale), M = (int)ceil(nh * kScale);
    const long long np_ll = (long long)N * M;
    if (np_ll > (1ll << 30) || (long long)w * h * ch > (1ll << 31)) { err = "detect_segments: image too large"; return L3D_ERR_UNSUPPORTED; }
    p.w = w; p.h = h; p.ch = ch; p.nw = nw; p.nh = nh; p.sw = w; p.sh = h;
    plan_scaled(p, N, M);
    p.up = 1.0f;
    if (nw != w || nh != h) p.up = 1.0f / (0.5f * (float(nw) / float(w) + float(nh) / float(h)));
    return L3D_OK;
}

// one image of a chunk: where it comes from, what varies inside a chunk, where its segments go
struct DetItem {
    const unsigned char* pixels = nullptr;      // host pixels, or with null the file `jpeg` staged at jpeg->stage_at
    size_t stride = 0;
    const JpegStaged* jpeg = nullptr;
    const l3d_device_image* dev = nullptr;      // an image in device memory (pixels and jpeg null), checked by device_image_pointer
    DetImgParam prm;                            // (cam_on: the image's route is Radial)
    WarpPlan warp;                              // checked (warp_check)
    std::vector<float>* out = nullptr;
};

// the detector on the B images of one chunk (p.B): every stage enqueued once; the host waits for the labelling's flag, for the candidate counts
// and for the segments
int detect_chunk(l3d_ctx* c, const DetPlan& p, const DetItem* items)
{
    hipStream_t st = c->stream;
    DetectBufs& d = c->det;
    const int B = p.B, cand_cap = p.cand_cap;
    // the chunk's kernel is the strongest route any of its images needs (a weaker image rides along as WarpPlan::L); it carries planes if an image does
    WarpRoute route = WarpRoute::None;
    bool jpeg = false, dev = false, valid = false, masks = false;
    size_t out_slots = 0;
    std::vector<DetImgParam> prm((size_t)B);
    for (int b = 0; b < B; ++b) {
        prm[b] = items[b].prm;
        route = std::max(route, items[b].warp.route);
        valid = valid || items[b].warp.plane;
        masks = masks || (items[b].warp.flags & kRemapMask);
        jpeg = jpeg || (!items[b].pixels && !items[b].dev);
        dev = dev || items[b].dev;
        out_slots += (size_t)std::min(prm[b].max_segments, cand_cap);
    }
    if (int rc = det_reserve(c, p, out_slots, route, valid)) return rc;
    if (masks) {            // the callers' masks, each into its image's slot (a device mask is checked first)
        HIPCHK(c, d.smask.reserve((size_t)B * p.sw * p.sh));
        for (int b = 0; b < B; ++b)
            if (items[b].warp.flags & kRemapMask) { if (int rc = remap_mask_upload(c, items[b].warp, p.sw, p.sh, b)) return rc; }
    }
    if (jpeg) {
        std::vector<const JpegStaged*> files((size_t)B, nullptr);
        for (int b = 0; b < B; ++b) if (!items[b].pixels && !items[b].dev) files[b] = items[b].jpeg;
        if (int rc = jpeg_staged_to_pixels(c, files.data(), B)) return rc;
    }
    if (dev) {              // the chunk's device images: one launch gathers them into their slots
        std::vector<const l3d_device_image*> images((size_t)B, nullptr);
        for (int b = 0; b < B; ++b) images[b] = items[b].dev;
        if (int rc = device_ingest(c, images.data(), B, p.sw, p.sh, p.ch, d.pixels.as<unsigned char>())) return rc;
    }
    for (int b = 0; b < B; ++b) if (items[b].pixels) HIPCHK(c, det_upload(c, p, b, items[b].pixels, items[b].stride));
    // (from pageable memory on purpose: a few dozen bytes go faster through the runtime's staging than as a DMA from pinned memory -- measured, 0.03 ms per call)
    HIPCHK(c, hipMemcpyAsync(d.prm.p, prm.data(), (size_t)B * sizeof(DetImgParam), hipMemcpyHostToDevice, st));
    // Lens and Resample: the chunk's table and, for Resample, the flags (a plain lens and a k1, k2 camera have none: every byte of their plane comes
    // out valid).  A chunk that carries planes and resamples nothing takes them from the masks alone, at the source size
    std::vector<DetLens> lens_tab;
    std::vector<int> rflags;
    if (route >= WarpRoute::Lens)
        for (int b = 0; b < B; ++b) { lens_tab.push_back(items[b].warp.L); rflags.push_back(items[b].warp.flags); }
    if (valid && route != WarpRoute::Resample) {
        for (int b = 0; b < B; ++b)
            if (int rc = plane_without_resample(c, items[b].warp.flags & kRemapMask, (size_t)p.w * p.h, b)) return rc;
    }
    if (int rc = det_pixel_stage(c, p, route, valid, lens_tab.data(), rflags.data())) return rc;

    // ---- rounds: label, vote, sort, regions
    for (int round = 0; round < kRounds; ++round) {
        if (int rc = det_label(c, p)) return rc;
        if (int rc = det_regions(c, p, nullptr)) return rc;
    }

    // ---- selection
    int* n_cand_d = det_n_cand(d);
    int *coff = n_cand_d + B, *ooff = coff + B + 1, *n_out_d = d.out.as<int>();
    const DetImgParam* prm_d = d.prm.as<DetImgParam>();
    float4* out_d = reinterpret_cast<float4*>(static_cast<char*>(d.out.p) + det_out_head(B));
    const dim3 b256(256);
    { ProfScope ps(c, "k_det_select_plan"); hipLaunchKernelGGL(k_det_select_plan, dim3(1), dim3(64), 0, st, n_cand_d, prm_d, B, cand_cap, coff, ooff, n_out_d); }
    std::vector<int> n_cand((size_t)B, 0);
    HIPCHK(c, hipMemcpyAsync(n_cand.data(), n_cand_d, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    int total = 0, most = 0;
    size_t slots = 0;
    std::vector<size_t> slot0((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) {
        n_cand[b] = std::max(0, std::min(n_cand[b], cand_cap));
        total += n_cand[b]; most = std::max(most, n_cand[b]);
        slot0[b] = slots;
        slots += (size_t)std::min(n_cand[b], std::max(0, prm[b].max_segments));
    }
    slot0[B] = slots;
    if (total <= 0 || slots == 0) return L3D_OK;
    const dim3 gc((total + 255) / 256);
    { ProfScope ps(c, "k_det_select_keys"); hipLaunchKernelGGL(k_det_select_keys, dim3((most + 255) / 256, B), b256, 0, st, d.cand.as<DetCand>(), coff, cand_cap, p.up, prm_d, d.ckeys.as<unsigned long long>(), d.cvals.as<unsigned>(), d.cimg.as<unsigned>()); }
    { size_t tb = d.tmp.cap; HIPCHK(c, sort_pairs_u64_u32(d.tmp.p, tb, d.ckeys.as<unsigned long long>(), d.ckeys2.as<unsigned long long>(), d.cvals.as<unsigned>(), d.cvals2.as<unsigned>(), total, 0, 64, st)); }
    const unsigned* order = d.cvals2.as<unsigned>();
    if (B > 1) {            // the images apart again, each keeping the order of its keys (ckeys2 and cvals are free: scratch of the second sort)
        int bits = 1;
        while ((1 << bits) < B) ++bits;
        { ProfScope ps(c, "k_det_select_image"); hipLaunchKernelGGL(k_det_select_image, gc, b256, 0, st, d.cvals2.as<unsigned>(), d.cimg.as<unsigned>(), total, d.cimg2.as<unsigned>()); }
        { size_t tb = d.tmp.cap; HIPCHK(c, sort_pairs_u32_u32(d.tmp.p, tb, d.cimg2.as<unsigned>(), d.ckeys2.as<unsigned>(), d.cvals2.as<unsigned>(), d.cvals.as<unsigned>(), total, 0, bits, st)); }
        order = d.cvals.as<unsigned>();
    }
    { ProfScope ps(c, "k_det_select_gather"); hipLaunchKernelGGL(k_det_select_gather, gc, b256, 0, st, d.cand.as<DetCand>(), d.ckeys.as<unsigned long long>(), order, d.cimg.as<unsigned>(), coff, ooff, B, cand_cap, p.up, prm_d, out_d, n_out_d); }
    const size_t head = det_out_head(B);
    std::vector<unsigned char> host(head + slots * 16);
    HIPCHK(c, hipMemcpyAsync(host.data(), d.out.p, host.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int* n_out = reinterpret_cast<const int*>(host.data());
    for (int b = 0; b < B; ++b) {
        const int n = std::max(0, std::min(n_out[b], (int)(slot0[b + 1] - slot0[b])));
        items[b].out->resize((size_t)n * 4);
        if (n) memcpy(items[b].out->data(), host.data() + head + slot0[b] * 16, (size_t)n * 16);
    }
    return L3D_OK;
}

// images per chunk of a group of n: the option, the index widths (the stack within 2^30 pixels), and half of the HBM that is free or held by the
// detector's own buffers already
int chunk_images(l3d_ctx* c, const DetPlan& p, int n, WarpRoute route, size_t jpeg_blocks, bool valid)
{
    long long lim = std::min<long long>(n, 1024);
    lim = std::min(lim, std::max(1ll, (1ll << 30) / p.np));
    if (c->opt.det_batch_images > 0) lim = std::min<long long>(lim, c->opt.det_batch_images);
    if (lim > 1) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 1; }
        const size_t budget = (free_b + c->det.held()) / 2;
        lim = std::min<long long>(lim, std::max<size_t>(1, budget / det_image_bytes(p, route, jpeg_blocks, valid)));
    }
    return (int)lim;
}
}  // namespace

int detect_segments_batch(l3d_ctx* c, const DetEntry* e, int n, std::vector<std::vector<float>>& out, std::vector<int>& status, std::vector<std::string>& message)
{
    out.assign((size_t)std::max(0, n), std::vector<float>());
    status.assign((size_t)std::max(0, n), L3D_OK);
    message.assign((size_t)std::max(0, n), std::string());
    if (!c) return L3D_ERR_INVALID;
    if (n < 0 || (n > 0 && !e)) return fail(c, L3D_ERR_INVALID, "detect_segments_batch: null argument");
    // ---- per entry, in order, on the caller's thread: headers, plan, warp.  An entry refused here fails alone
    struct Work { DetPlan plan; DetImgParam prm; WarpPlan warp; JpegStaged file; bool todo = false, done = false; };
    std::vector<Work> work((size_t)n);
    std::vector<JpegFrame> frames((size_t)n);
    for (int i = 0; i < n; ++i) {
        Work& k = work[i];
        const DetEntry& en = e[i];
        int w = en.width, h = en.height, ch = en.channels;
        size_t stride = en.row_stride;
        const bool dev = !en.pixels && !en.jpeg && en.dev;
        if (dev) {
            if ((status[i] = device_image_check(*en.dev, message[i])) != L3D_OK) continue;
            w = en.dev->width; h = en.dev->height; ch = device_image_det_channels(en.dev->channels); stride = (size_t)w * ch;
        }
        if (!en.pixels && en.jpeg) {
            if ((status[i] = jpeg_parse(en.jpeg, en.jpeg_bytes, frames[i], message[i])) != L3D_OK) continue;
            w = frames[i].width; h = frames[i].height; ch = frames[i].ncomp; stride = (size_t)w * ch;
            k.file.bytes = en.jpeg; k.file.n = en.jpeg_bytes; k.file.f = &frames[i];
        }
        if (en.max_segments < 0) { status[i] = L3D_ERR_INVALID; message[i] = "detect_segments: negative max_segments"; continue; }
        // a remap is checked before the plan, at the source size: the detector's image is its output (plan_image), and the plan remembers the source
        // size.  Everything else is checked behind the plan
        const bool has_image = en.pixels != nullptr || en.jpeg != nullptr || dev, remap = en.warp.has_remap;
        if (remap) {
            // (plan_image below sees the remap's output: what it asks of an image is asked of the source here -- behind the remap's first refusal,
            // of coefficients or a lens beside it, which is warp_check's first as well)
            if (!(en.warp.has_cam || en.warp.has_lens) && (!has_image || w < 8 || h < 8 || (ch != 1 && ch != 3) || stride < (size_t)w * ch)) {
                status[i] = L3D_ERR_INVALID; message[i] = "detect_segments: needs an image of at least 8x8 with 1 or 3 channels and a row stride of at least width x channels"; continue;
            }
            if ((status[i] = warp_check(en.warp, w, h, ch, k.warp, message[i])) != L3D_OK) continue;
        }
        const int ow = remap ? k.warp.out_w : w, oh = remap ? k.warp.out_h : h;
        if ((status[i] = plan_image(k.plan, has_image, ow, oh, ch, ow == w ? stride : (size_t)ow * ch, en.new_width, en.new_height, message[i])) != L3D_OK) continue;
        k.plan.sw = w; k.plan.sh = h;
        if (!remap && (status[i] = warp_check(en.warp, w, h, ch, k.warp, message[i])) != L3D_OK) continue;
        const bool radial = k.warp.route == WarpRoute::Radial;
        k.prm.cam = k.warp.cam;                 // (the identity camera unless the route is Radial)
        k.prm.cam_on = radial; k.prm.min_length = en.min_length; k.prm.max_segments = en.max_segments; k.prm.pad = 0;
        k.todo = true;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // ---- groups of equal plans in the order of their first entries; a group in chunks
    int rc = L3D_OK;
    for (int first = 0; first < n && rc == L3D_OK; ++first) {
        if (!work[first].todo) continue;
        std::vector<int> group;
        WarpRoute route = WarpRoute::None;
        bool valid = false;
        size_t blocks = 0;
        for (int i = first; i < n; ++i)
            if (work[i].todo && work[i].plan.same_group(work[first].plan)) {
                group.push_back(i); work[i].todo = false;
                route = std::max(route, work[i].warp.route);
                valid = valid || work[i].warp.plane;
                if (work[i].file.f) blocks = std::max(blocks, work[i].file.f->n_blocks);
            }
        const int per = chunk_images(c, work[first].plan, (int)group.size(), route, blocks, valid);
        for (size_t at = 0; at < group.size() && rc == L3D_OK; at += (size_t)per) {
            const size_t end = std::min(group.size(), at + (size_t)per);
            // the chunk's files: entropy decoding on the host threads, each into its own slice of the staging buffer; a file that fails leaves the chunk
            std::vector<JpegStaged*> files;
            for (size_t g = at; g < end; ++g) if (work[group[g]].file.f) files.push_back(&work[group[g]].file);
            if (!files.empty()) rc = jpeg_stage_files(c, files.data(), (int)files.size());
            if (rc != L3D_OK) break;
            std::vector<DetItem> items;
            std::vector<int> entry;
            for (size_t g = at; g < end; ++g) {
                const int i = group[g];
                Work& k = work[i];
                if (k.file.f && k.file.status != L3D_OK) { status[i] = k.file.status; message[i] = k.file.err; continue; }
                DetItem it;
                if (!e[i].pixels && !k.file.f && e[i].dev) {          // a device image: its memory is looked at here, before the chunk's launch; refused, it leaves the chunk
                    if ((status[i] = device_image_pointer(c, *e[i].dev, message[i])) != L3D_OK) continue;
                    it.dev = e[i].dev;
                }
                it.pixels = k.file.f ? nullptr : e[i].pixels; it.stride = e[i].row_stride; it.jpeg = k.file.f ? &k.file : nullptr; it.prm = k.prm; it.warp = k.warp; it.out = &out[i];
                items.push_back(it);
                entry.push_back(i);
            }
            if (items.empty()) continue;
            DetPlan plan = work[first].plan;
            plan_chunk(plan, (int)items.size());
            rc = detect_chunk(c, plan, items.data());
            if (rc == L3D_OK) for (int i : entry) work[i].done = true;
        }
        if (rc != L3D_OK) {         // a device failure ends the call: what was not finished carries its code
            std::string why;
            { std::lock_guard<std::mutex> lk(c->err_mu); why = c->err; }
            for (int i : group) if (status[i] == L3D_OK && !work[i].done) { out[i].clear(); status[i] = rc; message[i] = why; }
            for (int i = 0; i < n; ++i) if (work[i].todo) { status[i] = rc; message[i] = why; }
        }
    }
    return rc;
}

// one image: a batch of one, its outcome the call's
int detect_one(l3d_ctx* c, const DetEntry& en, std::vector<float>& out)
{
    out.clear();
    std::vector<std::vector<float>> outs;
    std::vector<int> status;
    std::vector<std::string> message;
    if (int rc = detect_segments_batch(c, &en, 1, outs, status, message)) return rc;
    if (status[0] != L3D_OK) return fail(c, status[0], message[0]);
    out.swap(outs[0]);
    return L3D_OK;
}

}  // namespace l3d

// ---- the C calls.  An entry of either kind as the detector's (its warp: warp_of_entry on its camera and the lens or remap that comes beside it)
static l3d::DetEntry det_entry(const l3d_detect_entry& e)
{
    l3d::DetEntry d;
    d.pixels = e.pixels; d.width = e.width; d.height = e.height; d.channels = e.channels; d.row_stride = e.row_stride;
    d.jpeg = e.jpeg; d.jpeg_bytes = e.jpeg_bytes;
    d.new_width = e.new_width; d.new_height = e.new_height; d.min_length = e.min_length; d.max_segments = e.max_segments;
    return d;
}
static l3d::DetEntry det_entry(const l3d_detect_device_entry& e)
{
    l3d::DetEntry d;
    d.dev = &e.image;
    d.new_width = e.new_width; d.new_height = e.new_height; d.min_length = e.min_length; d.max_segments = e.max_segments;
    return d;
}
static l3d::DetWarp entry_warp(const double* camera, const l3d_lens* lens) { return l3d::warp_of_entry(camera, lens, nullptr); }
static l3d::DetWarp entry_warp(const double* camera, const l3d_remap* remap) { return l3d::warp_of_entry(camera, nullptr, remap); }

// the segments as the C ABI hands them out: callee-allocated (l3d_free), 4 floats each
static int segments_to_c(l3d_ctx* c, const std::vector<float>& out, float** segments, int* n)
{
    float* p = static_cast<float*>(malloc(std::max<size_t>(16, out.size() * 4)));
    if (!p) return l3d::fail(c, L3D_ERR_INVALID, "detect_segments: out of memory");
    if (!out.empty()) memcpy(p, out.data(), out.size() * 4);
    *segments = p;
    *n = (int)(out.size() / 4);
    return L3D_OK;
}

// one entry (null: the message names the missing argument) through the detector
template <class E>
static int one_to_c(l3d_ctx* c, const E& e, const char* missing, float** segments, int* n)
{
    if (!c || !segments || !n) return L3D_ERR_INVALID;
    *segments = nullptr;
    *n = 0;
    if (missing) return l3d::fail(c, L3D_ERR_INVALID, missing);
    l3d::DetEntry d = det_entry(e);
    d.warp = entry_warp(e.camera, (const l3d_lens*)nullptr);
    std::vector<float> out;
    const int rc = l3d::detect_one(c, d, out);
    return rc != L3D_OK ? rc : segments_to_c(c, out, segments, n);
}

int l3d_detect_segments_distorted(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                                  float min_length, int max_segments, double fx, double fy, double cx, double cy, double k1, double k2, float** segments, int* n)
{
    const double cam[6] = { fx, fy, cx, cy, k1, k2 };
    const l3d_detect_entry e{ pixels, width, height, channels, row_stride, nullptr, 0, new_width, new_height, min_length, max_segments, cam };
    return one_to_c(c, e, nullptr, segments, n);
}

int l3d_detect_segments(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                        float min_length, int max_segments, float** segments, int* n)
{
    const l3d_detect_entry e{ pixels, width, height, channels, row_stride, nullptr, 0, new_width, new_height, min_length, max_segments, nullptr };
    return one_to_c(c, e, nullptr, segments, n);
}

int l3d_detect_segments_jpeg(l3d_ctx* c, const unsigned char* bytes, size_t n, int new_width, int new_height, float min_length, int max_segments,
                             const double* camera, float** segments, int* n_segments)
{
    const l3d_detect_entry e{ nullptr, 0, 0, 0, 0, bytes, n, new_width, new_height, min_length, max_segments, camera };
    return one_to_c(c, e, bytes ? nullptr : "detect_segments_jpeg: null argument", segments, n_segments);
}

int l3d_detect_segments_device(l3d_ctx* c, const l3d_device_image* image, int new_width, int new_height, float min_length, int max_segments, const double* camera,
                               float** segments, int* n)
{
    l3d_detect_device_entry e{};
    if (image) e.image = *image;
    e.new_width = new_width; e.new_height = new_height; e.min_length = min_length; e.max_segments = max_segments; e.camera = camera;
    return one_to_c(c, e, image ? nullptr : "detect_segments: null argument", segments, n);
}

// the batch detector's outcome as the C ABI hands it out: the segments of all entries one after the other, one line per failed entry
static int batch_to_c(l3d_ctx* c, const std::vector<l3d::DetEntry>& entries, float** segments, int* offsets, int* status)
{
    const int n = (int)entries.size();
    std::vector<std::vector<float>> out;
    std::vector<int> st;
    std::vector<std::string> msg;
    const int rc = l3d::detect_segments_batch(c, entries.data(), n, out, st, msg);
    std::string lines;
    std::vector<float> all;
    offsets[0] = 0;
    for (int i = 0; i < n; ++i) {
        status[i] = st[i];
        if (st[i] != L3D_OK) { out[i].clear(); lines += (lines.empty() ? "entry " : "\nentry ") + std::to_string(i) + ": " + msg[i]; }
        all.insert(all.end(), out[i].begin(), out[i].end());
        offsets[i + 1] = (int)(all.size() / 4);
    }
    if (!lines.empty()) l3d::fail(c, rc, lines);
    int total = 0;
    const int rc2 = segments_to_c(c, all, segments, &total);
    return rc != L3D_OK ? rc : rc2;
}

// n entries of either kind, each with the lens or the remap of `with` (the array or an element may be null: the entry's own camera rule)
template <class E, class X>
static int entries_to_c(l3d_ctx* c, const E* e, const X* const* with, int n, float** segments, int* offsets, int* status)
{
    if (!c || !segments || !offsets || !status || n < 0 || (n > 0 && !e)) return L3D_ERR_INVALID;
    *segments = nullptr;
    std::vector<l3d::DetEntry> entries((size_t)n);
    for (int i = 0; i < n; ++i) {
        entries[i] = det_entry(e[i]);
        entries[i].warp = entry_warp(e[i].camera, with ? with[i] : nullptr);
    }
    return batch_to_c(c, entries, segments, offsets, status);
}

int l3d_detect_segments_batch_lens(l3d_ctx* c, const l3d_detect_entry* e, const l3d_lens* const* lens, int n, float** segments, int* offsets, int* status)
{
    return entries_to_c(c, e, lens, n, segments, offsets, status);
}
int l3d_detect_segments_batch_remap(l3d_ctx* c, const l3d_detect_entry* e, const l3d_remap* const* remap, int n, float** segments, int* offsets, int* status)
{
    return entries_to_c(c, e, remap, n, segments, offsets, status);
}
int l3d_detect_segments_batch(l3d_ctx* c, const l3d_detect_entry* e, int n, float** segments, int* offsets, int* status)
{
    return l3d_detect_segments_batch_lens(c, e, nullptr, n, segments, offsets, status);
}
int l3d_detect_segments_device_batch_lens(l3d_ctx* c, const l3d_detect_device_entry* e, const l3d_lens* const* lens, int n, float** segments, int* offsets, int* status)
{
    return entries_to_c(c, e, lens, n, segments, offsets, status);
}
int l3d_detect_segments_device_batch_remap(l3d_ctx* c, const l3d_detect_device_entry* e, const l3d_remap* const* remap, int n, float** segments, int* offsets, int* status)
{
    return entries_to_c(c, e, remap, n, segments, offsets, status);
}
int l3d_detect_segments_device_batch(l3d_ctx* c, const l3d_detect_device_entry* e, int n, float** segments, int* offsets, int* status)
{
    return l3d_detect_segments_device_batch_lens(c, e, nullptr, n, segments, offsets, status);
}

// (tests) the defined / undefined plane, N x M bytes (255 / 0), that the LAST detector call of this context left for the first image of its last chunk;
// 0 x 0 when that chunk carried no validity plane
int l3d_test_detect_defined_plane(l3d_ctx* c, unsigned char* defined, size_t capacity, int* N, int* M)
{
    using namespace l3d;
    if (!c || !N || !M) return L3D_ERR_INVALID;
    DetectBufs& d = c->det;
    *N = d.vdef_n; *M = d.vdef_m;
    const size_t n = (size_t)d.vdef_n * d.vdef_m;
    if (n == 0 || !defined) return L3D_OK;          // (defined NULL: the size alone)
    if (capacity < n) return fail(c, L3D_ERR_INVALID, "test_detect_defined_plane: the buffer is too small");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(defined, d.vdef.p, n, hipMemcpyDeviceToHost));
    return L3D_OK;
}

// ---- the stages on their own, for the tests: the functions above (the same kernels and launch shapes as l3d_detect_segments), results copied out
int l3d_test_detect_pixel_stage(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                                float* grey, double* img, double* mod, double* ang, unsigned char* bucket, int* N, int* M)
{
    using namespace l3d;
    if (!c || !grey || !img || !mod || !ang || !bucket || !N || !M) return L3D_ERR_INVALID;
    DetPlan p;
    { std::string err; if (int rc = plan_image(p, pixels != nullptr, width, height, channels, row_stride, new_width, new_height, err)) return fail(c, rc, err); }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = det_reserve(c, p, 0)) return rc;
    HIPCHK(c, det_upload(c, p, 0, pixels, row_stride));
    if (int rc = det_pixel_stage(c, p)) return rc;
    DetectBufs& d = c->det;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(grey, d.grey.p, (size_t)p.nw * p.nh * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(img, d.img.p, (size_t)p.np * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(mod, d.mod.p, (size_t)p.np * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ang, d.ang.p, (size_t)p.np * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(bucket, d.bucket.p, (size_t)p.np * 2, hipMemcpyDeviceToHost));
    *N = p.N; *M = p.M;
    return L3D_OK;
}

int l3d_test_detect_label(l3d_ctx* c, const unsigned char* bucket, const unsigned char* active, int N, int M, int32_t* parent, uint32_t* key)
{
    using namespace l3d;
    if (!c || !bucket || !active || !parent || !key) return L3D_ERR_INVALID;
    if (N < 1 || M < 1 || (long long)N * M > (1ll << 30)) return fail(c, L3D_ERR_INVALID, "test_detect_label: size");
    DetPlan p;
    plan_scaled(p, N, M);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = det_reserve(c, p, 0)) return rc;
    DetectBufs& d = c->det;
    HIPCHK(c, hipMemcpy(d.bucket.p, bucket, (size_t)p.np * 2, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d.active.p, active, (size_t)p.np, hipMemcpyHostToDevice));
    HIPCHK(c, det_zero_scalars(c, 1));
    if (int rc = det_label(c, p)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(parent, d.parent.p, (size_t)p.np * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(key, d.keys.p, (size_t)p.np * 4, hipMemcpyDeviceToHost));
    return L3D_OK;
}

int l3d_test_detect_regions(l3d_ctx* c, int N, int M, const double* mod, const double* ang, const uint32_t* key, int min_reg,
                            l3d_detect_region_record** rec, int* n_rec, unsigned char* active_out)
{
    using namespace l3d;
    if (!c || !mod || !ang || !key || !rec || !n_rec || !active_out) return L3D_ERR_INVALID;
    *rec = nullptr;
    *n_rec = 0;
    if (N < 1 || M < 1 || (long long)N * M > (1ll << 30) || min_reg < 2) return fail(c, L3D_ERR_INVALID, "test_detect_regions: size or min_reg");
    DetPlan p;
    plan_scaled(p, N, M);
    p.min_reg = min_reg;
    p.cand_cap = p.np / min_reg + 16;
    const int np = p.np;
    // the vote's other outputs, from the keys: pixel indices in order, pixels per key
    std::vector<unsigned> vals((size_t)np);
    std::vector<int> count(2 * (size_t)np + 2, 0);
    for (int i = 0; i < np; ++i) {
        vals[i] = (unsigned)i;
        if (key[i] > 2u * (unsigned)np) return fail(c, L3D_ERR_INVALID, "test_detect_regions: key out of range");
        if (key[i] < 2u * (unsigned)np) ++count[key[i]];
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = det_reserve(c, p, 0)) return rc;
    DetectBufs& d = c->det;
    DevBuf trace;
    const size_t trace_bytes = (size_t)p.cand_cap * sizeof(l3d_detect_region_record);
    HIPCHK(c, trace.reserve(trace_bytes));
    int rc = L3D_OK, n = 0;
    auto step = [&](hipError_t e) { if (rc == L3D_OK && e != hipSuccess) rc = fail(c, L3D_ERR_HIP, hipGetErrorString(e)); };
    step(hipMemcpy(d.mod.p, mod, (size_t)np * 8, hipMemcpyHostToDevice));
    step(hipMemcpy(d.ang.p, ang, (size_t)np * 8, hipMemcpyHostToDevice));
    step(hipMemcpy(d.keys.p, key, (size_t)np * 4, hipMemcpyHostToDevice));
    step(hipMemcpy(d.vals.p, vals.data(), (size_t)np * 4, hipMemcpyHostToDevice));
    step(hipMemcpy(d.count.p, count.data(), (size_t)np * 8 + 8, hipMemcpyHostToDevice));
    step(hipMemset(d.active.p, 1, (size_t)np));
    step(hipMemset(trace.p, 0, trace_bytes));
    step(det_zero_scalars(c, 1));
    if (rc == L3D_OK) rc = det_regions(c, p, trace.as<l3d_detect_region_record>());
    if (rc == L3D_OK) step(hipStreamSynchronize(c->stream));
    if (rc == L3D_OK) step(hipMemcpy(&n, d.pos.as<int>() + np, 4, hipMemcpyDeviceToHost));
    if (rc == L3D_OK && n > p.cand_cap) rc = fail(c, L3D_ERR_INVALID, "test_detect_regions: more regions than np / min_reg");
    if (rc == L3D_OK) {
        l3d_detect_region_record* out = static_cast<l3d_detect_region_record*>(malloc(std::max<size_t>(16, (size_t)n * sizeof(l3d_detect_region_record))));
        if (!out) rc = fail(c, L3D_ERR_INVALID, "test_detect_regions: out of memory");
        else {
            if (n) step(hipMemcpy(out, trace.p, (size_t)n * sizeof(l3d_detect_region_record), hipMemcpyDeviceToHost));
            step(hipMemcpy(active_out, d.active.p, (size_t)np, hipMemcpyDeviceToHost));
            if (rc == L3D_OK) { *rec = out; *n_rec = n; } else free(out);
        }
    }
    trace.release();
    return rc;
}

int l3d_test_detect_nfa(l3d_ctx* c, const int32_t* n, const int32_t* k, const double* p, double logNT, int count, double* out)
{
    using namespace l3d;
    if (!c || !n || !k || !p || !out || count < 0) return L3D_ERR_INVALID;
    if (count == 0) return L3D_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf buf;
    const size_t cnt = (size_t)count;
    HIPCHK(c, buf.reserve(cnt * 24));
    int* dn = buf.as<int>();
    int* dk = dn + cnt;
    double* dp = reinterpret_cast<double*>(dk + cnt);
    double* dout = dp + cnt;
    int rc = L3D_OK;
    auto step = [&](hipError_t e) { if (rc == L3D_OK && e != hipSuccess) rc = fail(c, L3D_ERR_HIP, hipGetErrorString(e)); };
    step(hipMemcpy(dn, n, cnt * 4, hipMemcpyHostToDevice));
    step(hipMemcpy(dk, k, cnt * 4, hipMemcpyHostToDevice));
    step(hipMemcpy(dp, p, cnt * 8, hipMemcpyHostToDevice));
    if (rc == L3D_OK) {
        hipLaunchKernelGGL(k_det_nfa_test, dim3((count + 255) / 256), dim3(256), 0, c->stream, dn, dk, dp, logNT, count, dout);
        step(hipGetLastError());
        step(hipStreamSynchronize(c->stream));
        step(hipMemcpy(out, dout, cnt * 8, hipMemcpyDeviceToHost));
    }
    buf.release();
    return rc;
}
