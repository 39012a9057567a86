// l3d_segmask.hip -- a mask applied to line segments on the device ("A SEGMENT MASK" in include/line3d_amd.h): one wave per segment, four waves per
// workgroup (the launch shape of k_refine_lines).  Lanes stride over the samples of the segment, a ballot turns 64 validities into one word that
// every lane holds, and the bridging of gaps, the run search and the length test of l3d_segmask.hpp work on those words -- uniformly across the wave,
// computed redundantly by every lane, lane 0 writing.  k_segmask_count counts a segment's outputs, k_segmask_scan turns the counts into positions
// (wg_scan_excl: one workgroup), k_segmask_write runs the same function again and writes at those positions: the order comes from the scan, there
// is no atomic anywhere, and the launches are three whatever n is.  The host entry point l3d_test_mask_segments_host runs the header's functions
// with the host's wave.
#include "l3d_ctx.hpp"
#include "l3d_detect.hpp"
#include "l3d_scan.hpp"
#include "l3d_segmask.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

struct SegmaskDevWave {
    int lane;
    template <class F> __device__ uint64_t ballot(F f) { return (uint64_t)__ballot(f(lane) ? 1 : 0); }
};
struct SegmaskCountOut {
    int n;
    __device__ void put(const float*) { ++n; }
};
struct SegmaskWriteOut {
    int lane, at, src;
    float4* out; int* src_index;
    __device__ void put(const float* o)
    {
        if (lane == 0) { out[at] = make_float4(o[0], o[1], o[2], o[3]); src_index[at] = src; }
        ++at;
    }
};

// cnt[g]: the segments that input segment g becomes
__global__ __launch_bounds__(256) void k_segmask_count(segmask::Plan p, const float* __restrict__ segs, int n, int* __restrict__ cnt)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= n) return;
    const float4 s4 = reinterpret_cast<const float4*>(segs)[g];
    const float s[4] = { s4.x, s4.y, s4.z, s4.w };
    SegmaskDevWave wv{ lane };
    SegmaskCountOut out{ 0 };
    segmask::mask_segment(wv, p, s, out);
    if (lane == 0) cnt[g] = out.n;
}

// pos[0..n]: the exclusive prefix sums of cnt (pos[n]: the total as an int); total64: the total without the int's limit
__global__ __launch_bounds__(kScanThreads) void k_segmask_scan(const int* __restrict__ cnt, int* __restrict__ pos, int n, long long* __restrict__ total64)
{
    __shared__ int s_w[kScanThreads / 64];
    __shared__ long long s_t[kScanThreads / 64];
    long long t = 0;
    for (int i = threadIdx.x; i < n; i += kScanThreads) t += (long long)cnt[i];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
    if ((threadIdx.x & 63) == 0) s_t[threadIdx.x >> 6] = t;
    wg_scan_excl<kScanThreads>(cnt, pos, n, nullptr, s_w);           // (its barriers also order s_t; n >= 1)
    __syncthreads();
    if (threadIdx.x == 0) {
        long long sum = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) sum += s_t[w];
        *total64 = sum;
    }
}

// the segments of input segment g at pos[g] ..., with src_index = g
__global__ __launch_bounds__(256) void k_segmask_write(segmask::Plan p, const float* __restrict__ segs, int n, const int* __restrict__ pos, float4* __restrict__ out,
                                                       int* __restrict__ src_index)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= n) return;
    const float4 s4 = reinterpret_cast<const float4*>(segs)[g];
    const float s[4] = { s4.x, s4.y, s4.z, s4.w };
    SegmaskDevWave wv{ lane };
    SegmaskWriteOut o{ lane, pos[g], g, out, src_index };
    segmask::mask_segment(wv, p, s, o);
}

}  // namespace l3d

namespace {

thread_local std::string t_segmask_err;

// everything that needs no device: the fields, then the lens as A LENS checks it (warp_check, with the mask's extent in the place of the image's)
int segmask_validate(const float* segments, int n, const l3d_segment_mask* m, float** out, int32_t** src_index, int* n_out, segmask::Plan& p, std::string& msg)
{
    if (!out || !src_index || !n_out || n < 0 || (n > 0 && !segments)) { msg = "segment mask: bad argument"; return L3D_ERR_INVALID; }
    *out = nullptr; *src_index = nullptr; *n_out = 0;
    if (int rc = segmask::check_fields(m, p, msg)) return rc;
    if (m->lens) {
        DetWarp w;
        w.has_lens = true;
        w.lens = make_lens(*m->lens, m->fx, m->fy, m->cx, m->cy);
        WarpPlan plan;
        if (int rc = warp_check(w, p.mw, p.mh, 1, plan, msg)) return rc;
        if (plan.route != WarpRoute::None) { p.lens_on = 1; p.L = plan.L; }
    }
    return L3D_OK;
}

// the outputs as callee-allocated arrays (one spare element: n_out == 0 still hands out pointers that l3d_free takes)
int segmask_pack(const float* segs, const int32_t* src, size_t total, float** out, int32_t** src_index, int* n_out)
{
    float* o = static_cast<float*>(malloc((total * 4 + 1) * sizeof(float)));
    int32_t* s = static_cast<int32_t*>(malloc((total + 1) * sizeof(int32_t)));
    if (!o || !s) { free(o); free(s); return L3D_ERR_NOMEM; }
    if (total) { memcpy(o, segs, total * 16); memcpy(s, src, total * 4); }
    *out = o; *src_index = s; *n_out = (int)total;
    return L3D_OK;
}

int segmask_run(l3d_ctx* c, const float* segments, bool segs_on_device, int n, const l3d_segment_mask* m, float** out, int32_t** src_index, int* n_out)
{
    if (!c) return L3D_ERR_INVALID;
    segmask::Plan p{};
    std::string msg;
    if (int rc = segmask_validate(segments, n, m, out, src_index, n_out, p, msg)) return fail(c, rc, msg);
    // device memory of the caller's: the check an l3d_device_image gets, before anything is launched or read
    if (m->mask_on_device) {
        l3d_device_image im{};
        im.ptr = m->mask; im.width = p.mw; im.height = p.mh; im.channels = 1; im.dtype = L3D_U8; im.stride_y = (long long)p.stride; im.stride_x = 1; im.stride_c = 0;
        if (int rc = device_image_pointer(c, im, msg)) return fail(c, rc, "segment mask: " + msg);
    }
    if (segs_on_device && n > 0) {
        if (reinterpret_cast<uintptr_t>(segments) & 15) return fail(c, L3D_ERR_INVALID, "segment mask: a device segment array is aligned to 16 bytes");
        l3d_device_image im{};
        im.ptr = segments; im.width = 4; im.height = n; im.channels = 1; im.dtype = L3D_F32; im.stride_y = 4; im.stride_x = 1; im.stride_c = 0;
        if (int rc = device_image_pointer(c, im, msg)) return fail(c, rc, "segment mask: segments: " + msg);
    }
    if (n == 0) { const int rp = segmask_pack(nullptr, nullptr, 0, out, src_index, n_out); return rp ? fail(c, rp, "malloc") : L3D_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // the mask (g2): a host plane is uploaded once, rows packed; a device plane is read where it lies
    if (!m->mask_on_device) {
        HIPCHK(c, c->g2.reserve((size_t)p.mw * p.mh));
        HIPCHK(c, hipMemcpy2DAsync(c->g2.p, (size_t)p.mw, m->mask, p.stride, (size_t)p.mw, (size_t)p.mh, hipMemcpyHostToDevice, st));
        p.mask = c->g2.as<unsigned char>(); p.stride = (size_t)p.mw;
    }
    // the segments (g0)
    const float* d_segs = segments;
    if (!segs_on_device) {
        HIPCHK(c, c->g0.reserve((size_t)n * 16));
        HIPCHK(c, hipMemcpyAsync(c->g0.p, segments, (size_t)n * 16, hipMemcpyHostToDevice, st));
        d_segs = c->g0.as<float>();
    }
    // counts, positions, total (g1)
    const size_t o_cnt = 0, o_pos = al((size_t)n * 4), o_tot = o_pos + al(((size_t)n + 1) * 4);
    HIPCHK(c, c->g1.reserve(o_tot + 8));
    char* sb = c->g1.as<char>();
    int* d_cnt = reinterpret_cast<int*>(sb + o_cnt);
    int* d_pos = reinterpret_cast<int*>(sb + o_pos);
    long long* d_tot = reinterpret_cast<long long*>(sb + o_tot);
    const unsigned blocks = (unsigned)(((size_t)n + 3) / 4);
    { ProfScope ps(c, "segmask_count", st); hipLaunchKernelGGL(k_segmask_count, dim3(blocks), dim3(256), 0, st, p, d_segs, n, d_cnt); }
    { ProfScope ps(c, "segmask_scan", st); hipLaunchKernelGGL(k_segmask_scan, dim3(1), dim3(kScanThreads), 0, st, d_cnt, d_pos, n, d_tot); }
    long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_tot, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (total < 0 || total > (long long)INT_MAX) return fail(c, L3D_ERR_UNSUPPORTED, "segment mask: more than 2^31 - 1 output segments");
    if (total == 0) { const int rp = segmask_pack(nullptr, nullptr, 0, out, src_index, n_out); return rp ? fail(c, rp, "malloc") : L3D_OK; }
    // the outputs (g3): segments | src_index
    const size_t o_src = al((size_t)total * 16);
    HIPCHK(c, c->g3.reserve(o_src + (size_t)total * 4));
    char* ob = c->g3.as<char>();
    { ProfScope ps(c, "segmask_write", st); hipLaunchKernelGGL(k_segmask_write, dim3(blocks), dim3(256), 0, st, p, d_segs, n, d_pos, reinterpret_cast<float4*>(ob), reinterpret_cast<int*>(ob + o_src)); }
    std::vector<float> h_segs((size_t)total * 4);
    std::vector<int32_t> h_src((size_t)total);
    HIPCHK(c, hipMemcpyAsync(h_segs.data(), ob, (size_t)total * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_src.data(), ob + o_src, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const int rp = segmask_pack(h_segs.data(), h_src.data(), (size_t)total, out, src_index, n_out);
    return rp ? fail(c, rp, "malloc") : L3D_OK;
}

}  // namespace

extern "C" const char* l3d_segmask_last_error(void) { return t_segmask_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_mask_segments_host(const float* segments, int n, const l3d_segment_mask* m, float** out, int32_t** src_index, int* n_out)
{
    segmask::Plan p{};
    std::string msg;
    if (int rc = segmask_validate(segments, n, m, out, src_index, n_out, p, msg)) { t_segmask_err = msg; return rc; }
    if (m->mask_on_device) { t_segmask_err = "segment mask: the host entry point reads a mask in host memory"; return L3D_ERR_INVALID; }
    std::vector<float> segs;
    std::vector<int32_t> src;
    segmask::run_host(p, segments, n, segs, src);
    if (src.size() > (size_t)INT_MAX) { t_segmask_err = "segment mask: more than 2^31 - 1 output segments"; return L3D_ERR_UNSUPPORTED; }
    const int rp = segmask_pack(segs.data(), src.data(), src.size(), out, src_index, n_out);
    if (rp) t_segmask_err = "malloc";
    return rp;
}

extern "C" int l3d_mask_segments(l3d_ctx* c, const float* segments, int n, const l3d_segment_mask* m, float** out, int32_t** src_index, int* n_out)
{
    return segmask_run(c, segments, false, n, m, out, src_index, n_out);
}

extern "C" int l3d_mask_segments_device(l3d_ctx* c, const float* segments, int n, const l3d_segment_mask* m, float** out, int32_t** src_index, int* n_out)
{
    return segmask_run(c, segments, true, n, m, out, src_index, n_out);
}
