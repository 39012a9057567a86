// l3d_draw.hip -- 2-D segments drawn over 8-bit pixels on the device ("PROJECTION AND OVERLAYS", 2, in include/line3d_amd.h).  k_draw_pieces: one
// thread per segment runs draw::seg_setup (clip, quantise, major axis, columns) and counts the segment's pieces of 64 columns; k_draw_scan (one
// workgroup, wg_scan_excl) turns the counts into positions and reduces the rows the segments touch.  k_draw_cover: one wave per piece, found by a
// search of the positions, so a long line and many short ones keep the same number of waves busy; a lane takes one column (row) and walks the
// pixels across the stroke (draw::walk_lane), the wave's lanes at neighbouring pixels, and a 32-bit atomicMax whose result is not read files the
// key (coverage << 24 | segment) in the context's key plane.  The winner of a pixel is the largest key, whatever the schedule.  k_draw_resolve:
// one thread per pixel of the rows touched blends where the key is not 0 and writes the 0 back, so the plane is all zeros between calls and is
// cleared only when it is allocated or grown.  The host entry point l3d_test_draw_segments_host runs the header's functions in a loop.
#include "l3d_ctx.hpp"
#include "l3d_detect.hpp"
#include "l3d_draw.hpp"
#include "l3d_scan.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

__global__ __launch_bounds__(256) void k_draw_pieces(const float* __restrict__ segs, int n, int W16, int width, int height, draw::Seg* __restrict__ out,
                                                     int* __restrict__ cnt)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float4 s4 = reinterpret_cast<const float4*>(segs)[k];
    const float s[4] = { s4.x, s4.y, s4.z, s4.w };
    draw::Seg g;
    g.px = g.py = g.qx = g.qy = 0; g.rinv = 0.0; g.lo = 0; g.ymajor = 0;
    draw::seg_setup(s, W16, width, height, g);          // (a dropped segment: ncol 0, no rows)
    out[k] = g;
    cnt[k] = draw::pieces_of(g);
}

// pos[0..n]: the exclusive prefix sums of cnt; res[0]: the total without the int's limit, res[1], res[2]: the first and last row touched
__global__ __launch_bounds__(kScanThreads) void k_draw_scan(const int* __restrict__ cnt, const draw::Seg* __restrict__ segs, int* __restrict__ pos, int n,
                                                            long long* __restrict__ res)
{
    __shared__ int s_w[kScanThreads / 64];
    __shared__ long long s_t[kScanThreads / 64];
    __shared__ int s_lo[kScanThreads / 64], s_hi[kScanThreads / 64];
    long long t = 0;
    int lo = INT_MAX, hi = -1;
    for (int i = threadIdx.x; i < n; i += kScanThreads) {
        t += (long long)cnt[i];
        lo = min(lo, segs[i].rlo); hi = max(hi, segs[i].rhi);
    }
    for (int o = 32; o > 0; o >>= 1) { t += __shfl_down(t, o); lo = min(lo, __shfl_down(lo, o)); hi = max(hi, __shfl_down(hi, o)); }
    if ((threadIdx.x & 63) == 0) { s_t[threadIdx.x >> 6] = t; s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    wg_scan_excl<kScanThreads>(cnt, pos, n, nullptr, s_w);           // (its barriers also order s_t, s_lo, s_hi; n >= 1)
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        int a = INT_MAX, b = -1;
        for (int w = 0; w < kScanThreads / 64; ++w) { sum += s_t[w]; a = min(a, s_lo[w]); b = max(b, s_hi[w]); }
        res[0] = sum; res[1] = a; res[2] = b;
    }
}

struct DrawDevPut {
    unsigned* plane;
    __device__ void operator()(size_t at, unsigned key) { atomicMax(plane + at, key); }          // (result unread: a no-return atomic)
};

__global__ __launch_bounds__(256) void k_draw_cover(const draw::Seg* __restrict__ segs, int n, const int* __restrict__ pos, int total, int W16, int width, int height,
                                                    unsigned* __restrict__ plane)
{
    const int piece = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (piece >= total) return;                                         // (wave-uniform)
    // the segment of the piece: the last k with pos[k] <= piece (segments without pieces share their successor's position and are passed over)
    int a = 0, b = n;                                                   // pos[a] <= piece < pos[b]
    while (b - a > 1) { const int mid = a + ((b - a) >> 1); if (pos[mid] <= piece) a = mid; else b = mid; }
    const draw::Seg g = segs[a];
    const int c = (piece - pos[a]) * 64 + lane;
    if (c >= g.ncol) return;
    DrawDevPut put{ plane };
    draw::walk_lane(g, W16, width, height, g.lo + c, (unsigned)a, put);
}

__global__ __launch_bounds__(256) void k_draw_resolve(draw::Target t, unsigned* __restrict__ plane, int row0, int nrows, const unsigned char* __restrict__ colors,
                                                      int n_colors, const int32_t* __restrict__ color_index, int opacity)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)nrows * (size_t)t.width) return;
    const int i = row0 + (int)(idx / (size_t)t.width), j = (int)(idx % (size_t)t.width);
    const size_t at = (size_t)i * (size_t)t.width + (size_t)j;
    const unsigned key = plane[at];
    if (!key) return;
    plane[at] = 0u;
    draw::blend_pixel(t, i, j, key, colors, n_colors, color_index, opacity);
}

}  // namespace l3d

namespace {

thread_local std::string t_draw_err;

// pixels: the host's (image == nullptr) or a device image's
int draw_run(l3d_ctx* c, unsigned char* pixels, int width, int height, int channels, size_t row_stride, const l3d_device_image* image, const float* segments, int n,
             const unsigned char* colors, int n_colors, const int32_t* color_index, double width_px, int opacity)
{
    if (!c) return L3D_ERR_INVALID;
    std::string msg;
    if (image) {
        if (int rc = device_image_check(*image, msg)) return fail(c, rc, "draw segments: " + msg);
        width = image->width; height = image->height; channels = image->channels;
    } else {
        if (!pixels) return fail(c, L3D_ERR_INVALID, "draw segments: a null pointer");
    }
    if (int rc = draw::check_arguments(width, height, channels, segments, n, colors, n_colors, color_index, width_px, opacity, msg)) return fail(c, rc, msg);
    if (image) {
        if (image->dtype != L3D_U8) return fail(c, L3D_ERR_UNSUPPORTED, "draw segments: a device image must be L3D_U8");
        if (int rc = device_image_pointer(c, *image, msg)) return fail(c, rc, "draw segments: " + msg);
    } else if (row_stride < (size_t)width * (size_t)channels) return fail(c, L3D_ERR_INVALID, "draw segments: the row stride is below width x channels");
    if (n == 0) return L3D_OK;
    const int W16 = draw::stroke16(width_px);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // the key plane: zeroed when it is allocated or grown (or when a failed call may have left keys in it)
    const size_t plane_bytes = (size_t)width * (size_t)height * 4;
    const size_t cap_before = c->draw_plane.cap;
    HIPCHK(c, c->draw_plane.reserve(plane_bytes));
    if (c->draw_plane.cap != cap_before || c->draw_plane_dirty) {
        HIPCHK(c, hipMemsetAsync(c->draw_plane.p, 0, c->draw_plane.cap, st));
        c->draw_plane_dirty = false;
    }
    // segments (g0); per-segment records, counts, positions, totals (g1); colours and colour indices (g3)
    HIPCHK(c, c->g0.reserve((size_t)n * 16));
    HIPCHK(c, hipMemcpyAsync(c->g0.p, segments, (size_t)n * 16, hipMemcpyHostToDevice, st));
    const size_t o_cnt = al((size_t)n * sizeof(draw::Seg)), o_pos = o_cnt + al((size_t)n * 4), o_res = o_pos + al(((size_t)n + 1) * 4);
    HIPCHK(c, c->g1.reserve(o_res + 24));
    char* sb = c->g1.as<char>();
    draw::Seg* d_seg = reinterpret_cast<draw::Seg*>(sb);
    int* d_cnt = reinterpret_cast<int*>(sb + o_cnt);
    int* d_pos = reinterpret_cast<int*>(sb + o_pos);
    long long* d_res = reinterpret_cast<long long*>(sb + o_res);
    const size_t o_idx = al((size_t)n_colors * 4);
    HIPCHK(c, c->g3.reserve(o_idx + (color_index ? (size_t)n * 4 : 0)));
    HIPCHK(c, hipMemcpyAsync(c->g3.p, colors, (size_t)n_colors * 4, hipMemcpyHostToDevice, st));
    const int32_t* d_idx = nullptr;
    if (color_index) {
        HIPCHK(c, hipMemcpyAsync(c->g3.as<char>() + o_idx, color_index, (size_t)n * 4, hipMemcpyHostToDevice, st));
        d_idx = reinterpret_cast<const int32_t*>(c->g3.as<char>() + o_idx);
    }
    { ProfScope ps(c, "draw_pieces", st); hipLaunchKernelGGL(k_draw_pieces, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c->g0.as<float>(), n, W16, width, height, d_seg, d_cnt); }
    { ProfScope ps(c, "draw_scan", st); hipLaunchKernelGGL(k_draw_scan, dim3(1), dim3(kScanThreads), 0, st, d_cnt, d_seg, d_pos, n, d_res); }
    long long res[3] = { 0, 0, 0 };
    HIPCHK(c, hipMemcpyAsync(res, d_res, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (res[0] < 0 || res[0] > (long long)INT_MAX) return fail(c, L3D_ERR_UNSUPPORTED, "draw segments: more than 2^31 - 1 pieces");
    if (res[0] == 0 || res[2] < res[1]) return L3D_OK;                  // nothing reaches the image
    if (res[1] < 0 || res[2] > (long long)height - 1) return fail(c, L3D_ERR_HIP, "draw segments: the rows touched leave the image");
    const int total = (int)res[0], row0 = (int)res[1], nrows = (int)(res[2] - res[1] + 1);
    // the pixels
    draw::Target t{};
    t.width = width; t.height = height; t.ncomp = channels < 3 ? channels : 3;
    if (image) {
        if (!c->det.dev_event) HIPCHK(c, hipEventCreateWithFlags(&c->det.dev_event, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->det.dev_event, static_cast<hipStream_t>(image->stream)));
        HIPCHK(c, hipStreamWaitEvent(st, c->det.dev_event, 0));
        t.base = static_cast<unsigned char*>(const_cast<void*>(image->ptr));
        t.sy = image->stride_y; t.sx = image->stride_x;
        for (int k = 0; k < 3; ++k) t.off[k] = channels == 1 ? 0 : (long long)image->chan[k] * image->stride_c;
    } else {
        const size_t rb = (size_t)width * (size_t)channels;
        HIPCHK(c, c->g2.reserve(rb * (size_t)height));
        HIPCHK(c, hipMemcpy2DAsync(c->g2.p, rb, pixels, row_stride, rb, (size_t)height, hipMemcpyHostToDevice, st));
        t.base = c->g2.as<unsigned char>();
        t.sy = (long long)rb; t.sx = channels;
        for (int k = 0; k < 3; ++k) t.off[k] = k;
    }
    c->draw_plane_dirty = true;
    { ProfScope ps(c, "draw_cover", st); hipLaunchKernelGGL(k_draw_cover, dim3((unsigned)(((size_t)total + 3) / 4)), dim3(256), 0, st, d_seg, n, d_pos, total, W16, width, height, c->draw_plane.as<unsigned>()); }
    {
        ProfScope ps(c, "draw_resolve", st);
        hipLaunchKernelGGL(k_draw_resolve, dim3((unsigned)(((size_t)nrows * (size_t)width + 255) / 256)), dim3(256), 0, st, t, c->draw_plane.as<unsigned>(), row0, nrows,
                           c->g3.as<unsigned char>(), n_colors, d_idx, opacity);
    }
    if (!image) {
        const size_t rb = (size_t)width * (size_t)channels;
        HIPCHK(c, hipMemcpy2DAsync(pixels, row_stride, c->g2.p, rb, rb, (size_t)height, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    c->draw_plane_dirty = false;
    return L3D_OK;
}

}  // namespace

extern "C" const char* l3d_draw_last_error(void) { return t_draw_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_draw_segments_host(unsigned char* pixels, int width, int height, int channels, size_t row_stride, const float* segments, int n,
                                           const unsigned char* colors, int n_colors, const int32_t* color_index, double width_px, int opacity)
{
    std::string msg;
    if (!pixels) { t_draw_err = "draw segments: a null pointer"; return L3D_ERR_INVALID; }
    if (int rc = draw::check_arguments(width, height, channels, segments, n, colors, n_colors, color_index, width_px, opacity, msg)) { t_draw_err = msg; return rc; }
    if (row_stride < (size_t)width * (size_t)channels) { t_draw_err = "draw segments: the row stride is below width x channels"; return L3D_ERR_INVALID; }
    draw::Target t{};
    t.base = pixels; t.sy = (long long)row_stride; t.sx = channels; t.width = width; t.height = height; t.ncomp = channels < 3 ? channels : 3;
    for (int k = 0; k < 3; ++k) t.off[k] = k;
    draw::run_host(t, segments, n, colors, n_colors, color_index, draw::stroke16(width_px), opacity);
    return L3D_OK;
}

extern "C" int l3d_draw_segments(l3d_ctx* c, unsigned char* pixels, int width, int height, int channels, size_t row_stride, const float* segments, int n,
                                 const unsigned char* colors, int n_colors, const int32_t* color_index, double width_px, int opacity)
{
    return draw_run(c, pixels, width, height, channels, row_stride, nullptr, segments, n, colors, n_colors, color_index, width_px, opacity);
}

extern "C" int l3d_draw_segments_device(l3d_ctx* c, const l3d_device_image* image, const float* segments, int n, const unsigned char* colors, int n_colors,
                                        const int32_t* color_index, double width_px, int opacity)
{
    if (!c) return L3D_ERR_INVALID;
    if (!image) return fail(c, L3D_ERR_INVALID, "draw segments: a null pointer");
    return draw_run(c, nullptr, 0, 0, 0, 0, image, segments, n, colors, n_colors, color_index, width_px, opacity);
}
