// l3d_undistort.hip -- undistortion on the device, in front of the detector's rescale: the formulas stated in include/line3d_amd.h ("Undistortion on
// the device", "A LENS", "A REMAP"), every operation in the order stated there.  Three kernels, one per route (WarpRoute, l3d_undistort.hpp), built
// from shared pieces: ONE lens map (the lens and the remap kernel), ONE inside test and ONE four-tap sampler (the k1, k2 and the remap kernel).  The lens
// kernel alone spells the inside test and the taps out, in the words of und_inside and und_sample: through the helpers the compiler gave it three
// more instructions per wave and it measured 0.5 to 1.2 % slower; spelled out, its instruction stream is what it was before the pieces were shared.
// One thread per output pixel, the map in doubles (none is stored), 5 fractional bits per coordinate, the four taps weighted in 1/1024 with black
// outside the image.  Blocks are 32 x 8: the taps of a wave lie within a few source rows.  The image of a chunk is blockIdx.z.
#include "l3d_undistort.hpp"

#include <cmath>

#include "l3d_ctx.hpp"
#include "l3d_detect.hpp"

namespace l3d {
namespace {

constexpr int kUndBx = 32, kUndBy = 8;

// u, v inside the source w x h; NaN and inf fail.  Tested before any conversion to an integer
__device__ __forceinline__ bool und_inside(double u, double v, int w, int h) { return u > -1.0 && u < (double)w && v > -1.0 && v < (double)h; }

// the four taps of a sampled pixel: weights in 1/1024, whether each lies in the source, and the source indices (row offsets q in pixels, columns e)
struct UndTaps { int w00, w01, w10, w11; bool i00, i01, i10, i11; size_t q0, q1, e0, e1; };
// the pixel at (u, v) of src (w x h, inside by und_inside) into o, all channels.  Returns the taps: k_det_undistort_remap's validity byte needs them
__device__ __forceinline__ UndTaps und_sample(const unsigned char* __restrict__ src, int w, int h, int ch, double u, double v, unsigned char* __restrict__ o)
{
    const int iu = (int)rint(32.0 * u), iv = (int)rint(32.0 * v);             // in [-32, 32 w] x [-32, 32 h]
    const int x0 = iu >> 5, a = iu & 31, y0 = iv >> 5, b = iv & 31;           // floor and remainder, for negative values as well
    const bool cx0 = x0 >= 0 && x0 < w, cx1 = x0 + 1 >= 0 && x0 + 1 < w, ry0 = y0 >= 0 && y0 < h, ry1 = y0 + 1 >= 0 && y0 + 1 < h;
    const int w00 = (32 - a) * (32 - b), w01 = a * (32 - b), w10 = (32 - a) * b, w11 = a * b;
    const unsigned char* r0 = src + (size_t)(ry0 ? y0 : 0) * w * ch;           // (an index that is off the image is never formed: row and column 0 stand in)
    const unsigned char* r1 = src + (size_t)(ry1 ? y0 + 1 : 0) * w * ch;
    const size_t c0 = (size_t)(cx0 ? x0 : 0) * ch, c1 = (size_t)(cx1 ? x0 + 1 : 0) * ch;
    for (int k = 0; k < ch; ++k) {
        const int p00 = ry0 && cx0 ? r0[c0 + k] : 0, p01 = ry0 && cx1 ? r0[c1 + k] : 0;
        const int p10 = ry1 && cx0 ? r1[c0 + k] : 0, p11 = ry1 && cx1 ? r1[c1 + k] : 0;
        o[k] = (unsigned char)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10);
    }
    UndTaps t;
    t.w00 = w00; t.w01 = w01; t.w10 = w10; t.w11 = w11;
    t.i00 = ry0 && cx0; t.i01 = ry0 && cx1; t.i10 = ry1 && cx0; t.i11 = ry1 && cx1;
    t.q0 = (size_t)(ry0 ? y0 : 0) * w; t.q1 = (size_t)(ry1 ? y0 + 1 : 0) * w;
    t.e0 = (size_t)(cx0 ? x0 : 0); t.e1 = (size_t)(cx1 ? x0 + 1 : 0);
    return t;
}

// the lens map of "A LENS": output pixel (column j, row i) -> source position (u, v).  The model is uniform across a block
__device__ __forceinline__ void und_lens_map(const DetLens& L, int j, int i, double& u, double& v)
{
    const double x = ((double)j - L.ocx) / L.ofx, y = ((double)i - L.ocy) / L.ofy;
    const double r2 = x * x + y * y;
    double xd, yd;
    if (L.model == L3D_LENS_BROWN) {
        const double k1 = L.k[0], k2 = L.k[1], p1 = L.k[2], p2 = L.k[3], k3 = L.k[4], k4 = L.k[5], k5 = L.k[6], k6 = L.k[7];
        const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2, den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
        const double kr = num / den;
        xd = x * kr + ((2.0 * p1) * x * y + p2 * (r2 + 2.0 * (x * x)));
        yd = y * kr + (p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * x * y);
    } else {
        const double r = __builtin_sqrt(r2), th = atan(r), t2 = th * th;
        const double td = th * (1.0 + (((L.k[3] * t2 + L.k[2]) * t2 + L.k[1]) * t2 + L.k[0]) * t2);
        const double s = r > 1e-8 ? td / r : 1.0;
        xd = x * s; yd = y * s;
    }
    u = L.fx * xd + L.cx; v = L.fy * yd + L.cy;
}

// ---- Radial: k1, k2 onto the same camera.  Its own two-line map: fewer doubles than BROWN's, which is the point of keeping the kernel.
// prm: the cameras of a chunk's images, an image without one is copied; null: `one` for the single image
__global__ __launch_bounds__(256) void k_det_undistort(const unsigned char* __restrict__ src, int w, int h, int ch, DetCamera one, const DetImgParam* __restrict__ prm,
                                                        unsigned char* __restrict__ dst)
{
    const int j = blockIdx.x * kUndBx + threadIdx.x, i = blockIdx.y * kUndBy + threadIdx.y;
    if (j >= w || i >= h) return;
    src += (size_t)blockIdx.z * w * h * ch;
    dst += (size_t)blockIdx.z * w * h * ch;
    if (prm && !prm[blockIdx.z].cam_on) {
        const size_t at = ((size_t)i * w + j) * ch;
        for (int k = 0; k < ch; ++k) dst[at + k] = src[at + k];
        return;
    }
    const DetCamera cam = prm ? prm[blockIdx.z].cam : one;
    const double x = ((double)j - cam.cx) / cam.fx, y = ((double)i - cam.cy) / cam.fy;
    const double r2 = x * x + y * y, kr = 1.0 + (cam.k2 * r2 + cam.k1) * r2;
    const double u = cam.fx * (x * kr) + cam.cx, v = cam.fy * (y * kr) + cam.cy;
    unsigned char* o = dst + ((size_t)i * w + j) * ch;
    if (!und_inside(u, v, w, h)) {
        for (int k = 0; k < ch; ++k) o[k] = 0;
        return;
    }
    und_sample(src, w, h, ch, u, v, o);
}

// ---- Lens: BROWN or FISHEYE onto an output camera.  Behind the map: und_inside and und_sample, word for word (see the head of the file).
// The lens comes per image from the chunk's table, so the load is scalar.  tab: the chunk's lenses
// (model 0: the image is copied); a single image comes with a table of one (a choice between the table and a by-value argument made the compiler read
// the lens with per-lane loads)
__global__ __launch_bounds__(256) void k_det_undistort_lens(const unsigned char* __restrict__ src, int w, int h, int ch, const DetLens* __restrict__ tab,
                                                             unsigned char* __restrict__ dst)
{
    const int j = blockIdx.x * kUndBx + threadIdx.x, i = blockIdx.y * kUndBy + threadIdx.y;
    if (j >= w || i >= h) return;
    src += (size_t)blockIdx.z * w * h * ch;
    dst += (size_t)blockIdx.z * w * h * ch;
    const DetLens L = tab[blockIdx.z];
    unsigned char* o = dst + ((size_t)i * w + j) * ch;
    if (L.model == 0) {
        const unsigned char* s = src + ((size_t)i * w + j) * ch;
        for (int k = 0; k < ch; ++k) o[k] = s[k];
        return;
    }
    double u, v;
    und_lens_map(L, j, i, u, v);
    if (!(u > -1.0 && u < (double)w && v > -1.0 && v < (double)h)) {
        for (int k = 0; k < ch; ++k) o[k] = 0;
        return;
    }
    const int iu = (int)rint(32.0 * u), iv = (int)rint(32.0 * v);
    const int x0 = iu >> 5, a = iu & 31, y0 = iv >> 5, b = iv & 31;
    const bool cx0 = x0 >= 0 && x0 < w, cx1 = x0 + 1 >= 0 && x0 + 1 < w, ry0 = y0 >= 0 && y0 < h, ry1 = y0 + 1 >= 0 && y0 + 1 < h;
    const int w00 = (32 - a) * (32 - b), w01 = a * (32 - b), w10 = (32 - a) * b, w11 = a * b;
    const unsigned char* r0 = src + (size_t)(ry0 ? y0 : 0) * w * ch;
    const unsigned char* r1 = src + (size_t)(ry1 ? y0 + 1 : 0) * w * ch;
    const size_t c0 = (size_t)(cx0 ? x0 : 0) * ch, c1 = (size_t)(cx1 ? x0 + 1 : 0) * ch;
    for (int k = 0; k < ch; ++k) {
        const int p00 = ry0 && cx0 ? r0[c0 + k] : 0, p01 = ry0 && cx1 ? r0[c1 + k] : 0;
        const int p10 = ry1 && cx0 ? r1[c0 + k] : 0, p11 = ry1 && cx1 ? r1[c1 + k] : 0;
        o[k] = (unsigned char)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10);
    }
}

// ---- Resample: onto another size, with a validity plane.  One thread per pixel of the OUTPUT (ow x oh), the source stack is w x h.
// tab: the chunk's lenses -- model 0: the image is copied, which the host allows only where the two sizes are equal.  flags, per image:
// kRemapMask: smask holds a plane of the caller's for this image (w x h bytes per image, non-zero = valid; smask may be null when no image has the
// flag); kRemapBorder: a pixel outside, or with a weighted tap off the source, is invalid.  valid: ow x oh bytes per image, 255 or 0
__global__ __launch_bounds__(256) void k_det_undistort_remap(const unsigned char* __restrict__ src, int w, int h, int ch, const DetLens* __restrict__ tab,
                                                              const int* __restrict__ flags, const unsigned char* __restrict__ smask, unsigned char* __restrict__ dst,
                                                              int ow, int oh, unsigned char* __restrict__ valid)
{
    const int j = blockIdx.x * kUndBx + threadIdx.x, i = blockIdx.y * kUndBy + threadIdx.y;
    if (j >= ow || i >= oh) return;
    src += (size_t)blockIdx.z * w * h * ch;
    dst += (size_t)blockIdx.z * ow * oh * ch;
    valid += (size_t)blockIdx.z * ow * oh;
    const DetLens L = tab[blockIdx.z];
    const int fl = flags[blockIdx.z];
    const unsigned char* mk = (fl & kRemapMask) ? smask + (size_t)blockIdx.z * w * h : nullptr;
    unsigned char* o = dst + ((size_t)i * ow + j) * ch;
    unsigned char* vo = valid + (size_t)i * ow + j;
    if (L.model == 0) {
        if (j >= w || i >= h) { for (int k = 0; k < ch; ++k) o[k] = 0; *vo = 0; return; }       // (not reached: the host keeps ow == w, oh == h here)
        const unsigned char* s = src + ((size_t)i * w + j) * ch;
        for (int k = 0; k < ch; ++k) o[k] = s[k];
        *vo = !mk || mk[(size_t)i * w + j] ? 255 : 0;
        return;
    }
    double u, v;
    und_lens_map(L, j, i, u, v);
    if (!und_inside(u, v, w, h)) {
        for (int k = 0; k < ch; ++k) o[k] = 0;
        *vo = (fl & kRemapBorder) ? 0 : 255;
        return;
    }
    const UndTaps t = und_sample(src, w, h, ch, u, v, o);
    // a tap counts iff its weight is not zero: it must lie inside the source (the border rule) and be valid in the caller's plane (a tap off the
    // source has no entry there and is left to the border rule)
    bool ok = true;
    if (fl & kRemapBorder) ok = (!t.w00 || t.i00) && (!t.w01 || t.i01) && (!t.w10 || t.i10) && (!t.w11 || t.i11);
    if (mk) {
        if (t.w00 && t.i00) ok = ok && mk[t.q0 + t.e0];
        if (t.w01 && t.i01) ok = ok && mk[t.q0 + t.e1];
        if (t.w10 && t.i10) ok = ok && mk[t.q1 + t.e0];
        if (t.w11 && t.i11) ok = ok && mk[t.q1 + t.e1];
    }
    *vo = ok ? 255 : 0;
}

// a caller's mask as a validity plane: 255 / 0
__global__ void k_det_valid_from_mask(const unsigned char* __restrict__ smask, size_t n, unsigned char* __restrict__ valid)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) valid[i] = smask[i] ? 255 : 0;
}

// ---- the checks behind warp_check, one per thing a caller can give
// the camera of an undistortion: fx, fy finite and not zero; *active: a coefficient above L3D_EPS (commons.h:66, the drivers' condition) -- otherwise
// nothing is launched and the pixels pass through
constexpr double kDistEps = 1e-12;
int check_camera(const DetCamera& cam, int w, int h, bool* active, std::string& err)
{
    if (w > (1 << 24) || h > (1 << 24)) { err = "undistort: image too large"; return L3D_ERR_UNSUPPORTED; }      // 32 x a coordinate stays an int
    if (!std::isfinite(cam.fx) || !std::isfinite(cam.fy) || cam.fx == 0.0 || cam.fy == 0.0) { err = "undistort: fx and fy must be finite and not zero"; return L3D_ERR_INVALID; }
    *active = !(fabs(cam.k1) <= kDistEps && fabs(cam.k2) <= kDistEps);
    return L3D_OK;
}
// a lens: the source camera resolved; *active false: the pixels pass through
int lens_check(DetLens& l, int w, int h, bool* active, std::string& err)
{
    *active = false;
    if (w > (1 << 24) || h > (1 << 24)) { err = "undistort: image too large"; return L3D_ERR_UNSUPPORTED; }      // 32 x a coordinate stays an int
    if (l.model != L3D_LENS_BROWN && l.model != L3D_LENS_FISHEYE) { err = "lens: unknown model " + std::to_string(l.model) + " (L3D_LENS_BROWN or L3D_LENS_FISHEYE)"; return L3D_ERR_INVALID; }
    bool finite = std::isfinite(l.fx) && std::isfinite(l.fy) && std::isfinite(l.cx) && std::isfinite(l.cy);
    for (int k = 0; k < 8; ++k) finite = finite && std::isfinite(l.k[k]);
    if (!finite) { err = "lens: a field is not finite"; return L3D_ERR_INVALID; }
    if ((l.fx == 0.0) != (l.fy == 0.0)) { err = "lens: exactly one of fx, fy is zero (both zero: the output camera)"; return L3D_ERR_INVALID; }
    if (l.model == L3D_LENS_FISHEYE && (l.k[4] != 0.0 || l.k[5] != 0.0 || l.k[6] != 0.0 || l.k[7] != 0.0)) { err = "lens: a fisheye lens has four coefficients, k[4..7] must be 0"; return L3D_ERR_INVALID; }
    if (!std::isfinite(l.ofx) || !std::isfinite(l.ofy) || !std::isfinite(l.ocx) || !std::isfinite(l.ocy) || l.ofx == 0.0 || l.ofy == 0.0) {
        err = "undistort: fx and fy must be finite and not zero"; return L3D_ERR_INVALID;
    }
    if (l.fx == 0.0) { l.fx = l.ofx; l.fy = l.ofy; l.cx = l.ocx; l.cy = l.ocy; }
    bool small = true;
    for (int k = 0; k < 8; ++k) small = small && fabs(l.k[k]) <= kDistEps;
    *active = l.model == L3D_LENS_FISHEYE || !small || l.fx != l.ofx || l.fy != l.ofy || l.cx != l.ocx || l.cy != l.ocy;
    return L3D_OK;
}
// a remap: the output size and the lens resolved; *active false: nothing is resampled
int remap_check(DetRemap& r, int w, int h, int ch, bool* active, std::string& err)
{
    *active = false;
    if ((r.out_w == 0) != (r.out_h == 0) || r.out_w < 0 || r.out_h < 0) { err = "remap: the output size is (width, height), or (0, 0) for the source's"; return L3D_ERR_INVALID; }
    if (r.out_w == 0) { r.out_w = w; r.out_h = h; }
    if (r.out_w > (1 << 24) || r.out_h > (1 << 24) || (long long)r.out_w * r.out_h * ch > (1ll << 31)) { err = "remap: output image too large"; return L3D_ERR_UNSUPPORTED; }
    if (r.mask && (r.mask_w != w || r.mask_h != h)) {
        err = "remap: the mask is " + std::to_string(r.mask_w) + " x " + std::to_string(r.mask_h) + ", the source image " + std::to_string(w) + " x " + std::to_string(h);
        return L3D_ERR_INVALID;
    }
    if (r.mask && r.mask_stride < (size_t)w) { err = "remap: the mask's row stride is below the source width"; return L3D_ERR_INVALID; }
    const bool resized = r.out_w != w || r.out_h != h;
    if (!r.has_lens) {
        if (resized) { err = "remap: an output size that differs from the source's needs a lens (model 0: a pinhole camera) to resample with"; return L3D_ERR_INVALID; }
        return L3D_OK;
    }
    if (r.lens.model == 0) { r.lens.model = L3D_LENS_BROWN; for (double& k : r.lens.k) k = 0.0; }       // a pinhole camera
    if (int rc = lens_check(r.lens, w, h, active, err)) return rc;
    *active = *active || resized;
    return L3D_OK;
}

}  // namespace

DetLens make_lens(const l3d_lens& lens, double ofx, double ofy, double ocx, double ocy)
{
    DetLens l{};
    l.model = lens.model;
    l.fx = lens.fx; l.fy = lens.fy; l.cx = lens.cx; l.cy = lens.cy;
    l.ofx = ofx; l.ofy = ofy; l.ocx = ocx; l.ocy = ocy;
    for (int k = 0; k < 8; ++k) l.k[k] = lens.k[k];
    return l;
}

DetLens lens_of_camera(const DetCamera& cam)
{
    DetLens l{};
    l.model = L3D_LENS_BROWN;
    l.fx = l.ofx = cam.fx; l.fy = l.ofy = cam.fy; l.cx = l.ocx = cam.cx; l.cy = l.ocy = cam.cy;
    l.k[0] = cam.k1; l.k[1] = cam.k2;
    return l;
}

DetRemap remap_of(const l3d_remap& m, double fx, double fy, double cx, double cy)
{
    DetRemap r;
    r.has_lens = m.lens != nullptr;
    if (m.lens) r.lens = make_lens(*m.lens, fx, fy, cx, cy);
    r.out_w = m.out_width; r.out_h = m.out_height;
    r.mask = m.mask; r.mask_stride = m.mask_row_stride; r.mask_w = m.mask_width; r.mask_h = m.mask_height; r.mask_on_device = m.mask_on_device != 0; r.border_mask = m.border_mask != 0;
    return r;
}

DetWarp warp_of_entry(const double* k, const l3d_lens* lens, const l3d_remap* remap)
{
    DetWarp w;
    const double none[4] = { 0.0, 0.0, 0.0, 0.0 };
    const double* o = k ? k : none;             // the output camera
    if (k && ((!lens && !remap) || k[4] != 0.0 || k[5] != 0.0)) { w.has_cam = true; w.cam = DetCamera{ k[0], k[1], k[2], k[3], k[4], k[5] }; }
    if (lens) { w.has_lens = true; w.lens = make_lens(*lens, o[0], o[1], o[2], o[3]); }
    if (remap) { w.has_remap = true; w.remap = remap_of(*remap, o[0], o[1], o[2], o[3]); }
    return w;
}

int warp_check(const DetWarp& wp, int w, int h, int ch, WarpPlan& pl, std::string& err)
{
    pl = WarpPlan();
    pl.out_w = w; pl.out_h = h;
    if (wp.has_remap && (wp.has_cam || wp.has_lens)) { err = "remap: an image carries a remap beside distortion coefficients or a lens of its own"; return L3D_ERR_INVALID; }
    if (wp.has_cam && wp.has_lens) { err = "undistort: an image carries both distortion coefficients (k1, k2) and a lens"; return L3D_ERR_INVALID; }
    bool active = false;
    if (wp.has_cam) {
        if (int rc = check_camera(wp.cam, w, h, &active, err)) return rc;
        if (active) { pl.route = WarpRoute::Radial; pl.cam = wp.cam; pl.L = lens_of_camera(wp.cam); }
    } else if (wp.has_lens) {
        DetLens l = wp.lens;
        if (int rc = lens_check(l, w, h, &active, err)) return rc;
        if (active) { pl.route = WarpRoute::Lens; pl.L = l; }
    } else if (wp.has_remap) {
        DetRemap r = wp.remap;
        if (int rc = remap_check(r, w, h, ch, &active, err)) return rc;
        pl.out_w = r.out_w; pl.out_h = r.out_h;
        const bool lens_alone = !r.mask && !r.border_mask && r.out_w == w && r.out_h == h;       // the remap asks for nothing else: the ..._lens call
        if (active) { pl.route = lens_alone ? WarpRoute::Lens : WarpRoute::Resample; pl.L = r.lens; }
        pl.flags = (r.mask ? kRemapMask : 0) | (pl.route == WarpRoute::Resample && r.border_mask ? kRemapBorder : 0);
        pl.plane = r.mask || pl.route == WarpRoute::Resample;
        pl.mask = r.mask; pl.mask_stride = r.mask_stride; pl.mask_on_device = r.mask_on_device;
    }
    return L3D_OK;
}

void launch_undistort(l3d_ctx* c, int w, int h, int ch, int B, const DetCamera& one, const DetImgParam* prm)
{
    DetectBufs& d = c->det;
    ProfScope ps(c, "k_det_undistort");
    hipLaunchKernelGGL(k_det_undistort, dim3((w + kUndBx - 1) / kUndBx, (h + kUndBy - 1) / kUndBy, B), dim3(kUndBx, kUndBy), 0, c->stream, d.pixels.as<unsigned char>(), w, h, ch, one, prm,
                       d.undist.as<unsigned char>());
}

int launch_undistort_lens(l3d_ctx* c, int w, int h, int ch, int B, const DetLens* tab)
{
    DetectBufs& d = c->det;
    HIPCHK(c, d.lens.reserve((size_t)B * sizeof(DetLens)));
    HIPCHK(c, hipMemcpyAsync(d.lens.p, tab, (size_t)B * sizeof(DetLens), hipMemcpyHostToDevice, c->stream));
    ProfScope ps(c, "k_det_undistort_lens");
    hipLaunchKernelGGL(k_det_undistort_lens, dim3((w + kUndBx - 1) / kUndBx, (h + kUndBy - 1) / kUndBy, B), dim3(kUndBx, kUndBy), 0, c->stream, d.pixels.as<unsigned char>(), w, h,
                       ch, d.lens.as<DetLens>(), d.undist.as<unsigned char>());
    return L3D_OK;
}

int launch_undistort_remap(l3d_ctx* c, int w, int h, int ch, int ow, int oh, int B, const DetLens* tab, const int* flags)
{
    DetectBufs& d = c->det;
    HIPCHK(c, d.lens.reserve((size_t)B * sizeof(DetLens)));
    HIPCHK(c, d.rflags.reserve((size_t)B * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(d.lens.p, tab, (size_t)B * sizeof(DetLens), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.rflags.p, flags, (size_t)B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    ProfScope ps(c, "k_det_undistort_remap");
    hipLaunchKernelGGL(k_det_undistort_remap, dim3((ow + kUndBx - 1) / kUndBx, (oh + kUndBy - 1) / kUndBy, B), dim3(kUndBx, kUndBy), 0, c->stream, d.pixels.as<unsigned char>(), w, h,
                       ch, d.lens.as<DetLens>(), d.rflags.as<int>(), d.smask.as<unsigned char>(), d.undist.as<unsigned char>(), ow, oh, d.valid.as<unsigned char>());
    return L3D_OK;
}

int remap_mask_upload(l3d_ctx* c, const WarpPlan& r, int w, int h, int b)
{
    if (r.mask_on_device) {
        l3d_device_image im{};
        im.ptr = r.mask; im.width = w; im.height = h; im.channels = 1; im.dtype = L3D_U8; im.stride_y = (long long)r.mask_stride; im.stride_x = 1; im.stride_c = 0;
        std::string err;
        if (int rc = device_image_pointer(c, im, err)) return fail(c, rc, "remap mask: " + err);
    }
    HIPCHK(c, hipMemcpy2DAsync(c->det.smask.as<unsigned char>() + (size_t)b * w * h, (size_t)w, r.mask, r.mask_stride, (size_t)w, (size_t)h,
                               r.mask_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    return L3D_OK;
}

int plane_without_resample(l3d_ctx* c, bool has_mask, size_t n, int b)
{
    DetectBufs& d = c->det;
    unsigned char* v = d.valid.as<unsigned char>() + (size_t)b * n;
    if (!has_mask) { HIPCHK(c, hipMemsetAsync(v, 255, n, c->stream)); return L3D_OK; }
    ProfScope ps(c, "k_det_valid_from_mask");
    hipLaunchKernelGGL(k_det_valid_from_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d.smask.as<unsigned char>() + (size_t)b * n, n, v);
    return L3D_OK;
}

// the order of the refusals is the calls': fields, sizes and the warp first, device pointers after them, and nothing is launched before the last
int undistort_one(l3d_ctx* c, const WarpIo& io, const DetWarp& warp)
{
    if (!c) return L3D_ERR_INVALID;
    const bool dev = io.in != nullptr, remap = warp.has_remap;
    WarpPlan wp;                                // (lives until the stream has been synchronised: the launches read its lens and flags)
    std::string err;
    int w = io.width, h = io.height, ch = io.channels;
    if (dev) {
        if (int rc = device_image_check(*io.in, err)) return fail(c, rc, err);
        if (int rc = device_image_check(*io.dout, err)) return fail(c, rc, err);
        if (io.dvalid) { if (int rc = device_image_check(*io.dvalid, err)) return fail(c, rc, err); }
        w = io.in->width; h = io.in->height; ch = device_image_det_channels(io.in->channels);
        if (!remap && (io.dout->width != w || io.dout->height != h || device_image_det_channels(io.dout->channels) != ch))
            return fail(c, L3D_ERR_INVALID, "undistort: the output's size and channels must be the input's");
    } else if (!io.pixels || !io.out || w < 1 || h < 1 || (ch != 1 && ch != 3) || io.row_stride < (size_t)w * ch || (!remap && io.out_row_stride < (size_t)w * ch))
        return fail(c, L3D_ERR_INVALID, "undistort: needs an image of at least 1x1 with 1 or 3 channels and row strides of at least width x channels");
    if ((long long)w * h * ch > (1ll << 31)) return fail(c, L3D_ERR_UNSUPPORTED, "undistort: image too large");
    if (int rc = warp_check(warp, w, h, ch, wp, err)) return fail(c, rc, err);
    const int ow = wp.out_w, oh = wp.out_h;
    if (remap && dev) {
        if (io.dout->width != ow || io.dout->height != oh || device_image_det_channels(io.dout->channels) != ch)
            return fail(c, L3D_ERR_INVALID, "undistort: the output's size must be the remap's output size and its channels the input's");
        if (io.dvalid && (io.dvalid->width != ow || io.dvalid->height != oh || io.dvalid->channels != 1 || io.dvalid->dtype != L3D_U8))
            return fail(c, L3D_ERR_INVALID, "undistort: the validity plane is a one-channel L3D_U8 image of the output size");
    } else if (remap && (io.out_row_stride < (size_t)ow * ch || (io.valid && io.valid_row_stride < (size_t)ow)))
        return fail(c, L3D_ERR_INVALID, "undistort: an output row stride is below the output width");
    if (dev) {
        if (int rc = device_image_pointer(c, *io.in, err)) return fail(c, rc, err);
        if (int rc = device_image_pointer(c, *io.dout, err)) return fail(c, rc, err);
        if (io.dvalid) { if (int rc = device_image_pointer(c, *io.dvalid, err)) return fail(c, rc, err); }
    }
    // a remap's own call keeps its kernel for a lens alone: the caller may ask for the plane, which that kernel writes
    const WarpRoute route = remap && wp.route == WarpRoute::Lens ? WarpRoute::Resample : wp.route;
    const bool active = route != WarpRoute::None, want_valid = dev ? io.dvalid != nullptr : io.valid != nullptr;
    const size_t row = (size_t)w * ch, orow = (size_t)ow * ch;
    if (!dev && !active) {                      // the pixels pass through
        if (io.out != io.pixels || io.out_row_stride != io.row_stride)
            for (int i = 0; i < h; ++i) memmove(io.out + (size_t)i * io.out_row_stride, io.pixels + (size_t)i * io.row_stride, row);
        if (!want_valid) return L3D_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    DetectBufs& d = c->det;
    if (dev || active) HIPCHK(c, d.pixels.reserve(row * h));
    if (active) HIPCHK(c, d.undist.reserve(orow * oh));
    if (remap) HIPCHK(c, d.valid.reserve((size_t)ow * oh));
    if (wp.flags & kRemapMask) {
        HIPCHK(c, d.smask.reserve((size_t)w * h));
        if (int rc = remap_mask_upload(c, wp, w, h, 0)) return rc;
    }
    if (dev) {                                  // (the ingest is complete before the egress starts: in and out may be the same memory)
        const l3d_device_image* one[1] = { io.in };
        if (int rc = device_ingest(c, one, 1, w, h, ch, d.pixels.as<unsigned char>())) return rc;
    } else if (active) HIPCHK(c, hipMemcpy2DAsync(d.pixels.p, row, io.pixels, io.row_stride, row, (size_t)h, hipMemcpyHostToDevice, c->stream));
    if (route == WarpRoute::Resample) { if (int rc = launch_undistort_remap(c, w, h, ch, ow, oh, 1, &wp.L, &wp.flags)) return rc; }
    else if (route == WarpRoute::Lens) { if (int rc = launch_undistort_lens(c, w, h, ch, 1, &wp.L)) return rc; }
    else if (route == WarpRoute::Radial) launch_undistort(c, w, h, ch, 1, wp.cam, nullptr);
    else if (remap && want_valid) { if (int rc = plane_without_resample(c, wp.mask != nullptr, (size_t)w * h, 0)) return rc; }      // the mask is the plane
    const unsigned char* res = active ? d.undist.as<unsigned char>() : d.pixels.as<unsigned char>();
    if (dev) {
        if (int rc = device_egress(c, res, *io.dout)) return rc;
        if (io.dvalid) { if (int rc = device_egress(c, d.valid.as<unsigned char>(), *io.dvalid)) return rc; }
    } else {
        if (active) HIPCHK(c, hipMemcpy2DAsync(io.out, io.out_row_stride, res, orow, orow, (size_t)oh, hipMemcpyDeviceToHost, c->stream));
        if (io.valid) HIPCHK(c, hipMemcpy2DAsync(io.valid, io.valid_row_stride, d.valid.p, (size_t)ow, (size_t)ow, (size_t)oh, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return L3D_OK;
}

}  // namespace l3d

// ---- the C calls: argument translators over undistort_one
using l3d::WarpIo;
static WarpIo host_io(const unsigned char* pixels, int width, int height, int channels, size_t row_stride, unsigned char* out, size_t out_row_stride,
                      unsigned char* valid = nullptr, size_t valid_row_stride = 0)
{
    WarpIo io;
    io.pixels = pixels; io.width = width; io.height = height; io.channels = channels; io.row_stride = row_stride;
    io.out = out; io.out_row_stride = out_row_stride; io.valid = valid; io.valid_row_stride = valid_row_stride;
    return io;
}
static WarpIo device_io(const l3d_device_image* in, const l3d_device_image* out, const l3d_device_image* valid = nullptr)
{
    WarpIo io;
    io.in = in; io.dout = out; io.dvalid = valid;
    return io;
}

int l3d_undistort_image(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, double fx, double fy, double cx, double cy,
                        double k1, double k2, unsigned char* out, size_t out_row_stride)
{
    const double cam[6] = { fx, fy, cx, cy, k1, k2 };
    return l3d::undistort_one(c, host_io(pixels, width, height, channels, row_stride, out, out_row_stride), l3d::warp_of_entry(cam, nullptr, nullptr));
}

int l3d_undistort_image_lens(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, double fx, double fy, double cx, double cy,
                             const l3d_lens* lens, unsigned char* out, size_t out_row_stride)
{
    if (!c) return L3D_ERR_INVALID;
    if (!lens) return l3d::fail(c, L3D_ERR_INVALID, "undistort: null argument");
    const double cam[6] = { fx, fy, cx, cy, 0.0, 0.0 };
    return l3d::undistort_one(c, host_io(pixels, width, height, channels, row_stride, out, out_row_stride), l3d::warp_of_entry(cam, lens, nullptr));
}

int l3d_undistort_image_remap(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, double fx, double fy, double cx, double cy,
                              const l3d_remap* remap, unsigned char* out, size_t out_row_stride, unsigned char* valid, size_t valid_row_stride)
{
    if (!c) return L3D_ERR_INVALID;
    if (!remap) return l3d::fail(c, L3D_ERR_INVALID, "undistort: null argument");
    const double cam[6] = { fx, fy, cx, cy, 0.0, 0.0 };
    return l3d::undistort_one(c, host_io(pixels, width, height, channels, row_stride, out, out_row_stride, valid, valid_row_stride), l3d::warp_of_entry(cam, nullptr, remap));
}

int l3d_undistort_image_device(l3d_ctx* c, const l3d_device_image* in, double fx, double fy, double cx, double cy, double k1, double k2, const l3d_device_image* out)
{
    if (!c) return L3D_ERR_INVALID;
    if (!in || !out) return l3d::fail(c, L3D_ERR_INVALID, "undistort: null argument");
    const double cam[6] = { fx, fy, cx, cy, k1, k2 };
    return l3d::undistort_one(c, device_io(in, out), l3d::warp_of_entry(cam, nullptr, nullptr));
}

int l3d_undistort_image_device_lens(l3d_ctx* c, const l3d_device_image* in, double fx, double fy, double cx, double cy, const l3d_lens* lens, const l3d_device_image* out)
{
    if (!c) return L3D_ERR_INVALID;
    if (!in || !out || !lens) return l3d::fail(c, L3D_ERR_INVALID, "undistort: null argument");
    const double cam[6] = { fx, fy, cx, cy, 0.0, 0.0 };
    return l3d::undistort_one(c, device_io(in, out), l3d::warp_of_entry(cam, lens, nullptr));
}

int l3d_undistort_image_device_remap(l3d_ctx* c, const l3d_device_image* in, double fx, double fy, double cx, double cy, const l3d_remap* remap, const l3d_device_image* out,
                                     const l3d_device_image* valid)
{
    if (!c) return L3D_ERR_INVALID;
    if (!in || !out || !remap) return l3d::fail(c, L3D_ERR_INVALID, "undistort: null argument");
    const double cam[6] = { fx, fy, cx, cy, 0.0, 0.0 };
    return l3d::undistort_one(c, device_io(in, out, valid), l3d::warp_of_entry(cam, nullptr, remap));
}

// (tests) host only: warp_check on what a batch entry with this camera, lens and remap carries
int l3d_test_undistort_route(const double* camera, const l3d_lens* lens, const l3d_remap* remap, int width, int height, int channels, int* route, int* plane, int* out_width,
                             int* out_height, char* msg, size_t n)
{
    if (!route || !plane || !out_width || !out_height) return L3D_ERR_INVALID;
    l3d::WarpPlan w;
    std::string err;
    const int rc = l3d::warp_check(l3d::warp_of_entry(camera, lens, remap), width, height, channels, w, err);
    *route = (int)w.route; *plane = w.plane ? 1 : 0; *out_width = w.out_w; *out_height = w.out_h;
    if (msg && n) snprintf(msg, n, "%s", err.c_str());
    return rc;
}
