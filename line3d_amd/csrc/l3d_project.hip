// l3d_project.hip -- 3-D segments projected into cameras on the device ("PROJECTION AND OVERLAYS", 1, in include/line3d_amd.h): one (camera, segment)
// pair per lane, four waves per workgroup, the camera a dimension of the grid, so a wave never spans two cameras.  k_proj_count runs
// project::project_pair and a ballot turns the wave's 64 decisions into one word; k_proj_scan (wg_scan_excl: one workgroup) turns the words' bit
// counts into positions; k_proj_write runs the same function again and writes at the word's position plus the kept lanes below its own: the order
// comes from the scan, there is no atomic anywhere, and the launches are three per chunk of cameras whatever n is.  The host entry point
// l3d_test_project_lines_host runs the header's functions in a loop.
#include "l3d_ctx.hpp"
#include "l3d_detect.hpp"
#include "l3d_project.hpp"
#include "l3d_scan.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

// words[c * nw + w]: bit l set iff pair (camera c of the chunk, segment 64 w + l) is kept; cnt: its number of bits
__global__ __launch_bounds__(256) void k_proj_count(const double* __restrict__ seg3d, int n, const l3d_camera* __restrict__ cams, int nw, double near_z, double margin,
                                                    unsigned long long* __restrict__ words, int* __restrict__ cnt)
{
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, c = blockIdx.y;
    if (w >= nw) return;                                                // (wave-uniform)
    const int i = w * 64 + lane;
    bool keep = false;
    if (i < n) {
        double s[6];
        for (int k = 0; k < 6; ++k) s[k] = seg3d[6 * (size_t)i + k];
        float o[4]; unsigned char fl;
        keep = project::project_pair(cams[c], s, near_z, margin, o, fl);
    }
    const unsigned long long b = (unsigned long long)__ballot(keep ? 1 : 0);
    if (lane == 0) { words[(size_t)c * nw + w] = b; cnt[(size_t)c * nw + w] = __popcll(b); }
}

// pos[0..nwords]: the exclusive prefix sums of cnt (pos[nwords]: the chunk's total; a chunk has fewer than 2^31 pairs)
__global__ __launch_bounds__(kScanThreads) void k_proj_scan(const int* __restrict__ cnt, int* __restrict__ pos, int nwords)
{
    __shared__ int s_w[kScanThreads / 64];
    wg_scan_excl<kScanThreads>(cnt, pos, nwords, nullptr, s_w);
}

__global__ __launch_bounds__(256) void k_proj_write(const double* __restrict__ seg3d, int n, const l3d_camera* __restrict__ cams, int nw, double near_z, double margin,
                                                    const unsigned long long* __restrict__ words, const int* __restrict__ pos, float4* __restrict__ seg2d,
                                                    int* __restrict__ src_index, unsigned char* __restrict__ flags)
{
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, c = blockIdx.y;
    if (w >= nw) return;
    const unsigned long long b = words[(size_t)c * nw + w];
    if (!((b >> lane) & 1ull)) return;                                  // (a set bit implies 64 w + lane < n)
    const int i = w * 64 + lane;
    double s[6];
    for (int k = 0; k < 6; ++k) s[k] = seg3d[6 * (size_t)i + k];
    float o[4]; unsigned char fl = 0;
    project::project_pair(cams[c], s, near_z, margin, o, fl);
    const int at = pos[(size_t)c * nw + w] + __popcll(b & ((1ull << lane) - 1ull));
    seg2d[at] = make_float4(o[0], o[1], o[2], o[3]);
    src_index[at] = i;
    flags[at] = fl;
}

}  // namespace l3d

namespace {

thread_local std::string t_project_err;

// the outputs as callee-allocated arrays (one spare element each: an empty result still hands out pointers that l3d_free takes)
int project_pack(const std::vector<float>& segs, const std::vector<int32_t>& src, const std::vector<unsigned char>& fl, float** seg2d, int32_t** src_index,
                 unsigned char** flags)
{
    const size_t total = src.size();
    float* o = static_cast<float*>(malloc((total * 4 + 1) * sizeof(float)));
    int32_t* s = static_cast<int32_t*>(malloc((total + 1) * sizeof(int32_t)));
    unsigned char* f = static_cast<unsigned char*>(malloc(total + 1));
    if (!o || !s || !f) { free(o); free(s); free(f); return L3D_ERR_NOMEM; }
    if (total) { memcpy(o, segs.data(), total * 16); memcpy(s, src.data(), total * 4); memcpy(f, fl.data(), total); }
    *seg2d = o; *src_index = s; *flags = f;
    return L3D_OK;
}

int project_run(l3d_ctx* c, const double* seg3d, bool on_device, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d,
                int32_t** src_index, unsigned char** flags, int64_t* cam_start)
{
    if (!c) return L3D_ERR_INVALID;
    std::string msg;
    if (int rc = project::check_arguments(seg3d, n, cameras, m, near_z, margin, seg2d, src_index, flags, cam_start, msg)) return fail(c, rc, msg);
    // device memory of the caller's: the check an l3d_device_image gets, before anything is launched or read
    if (on_device && n > 0) {
        if (reinterpret_cast<uintptr_t>(seg3d) & 7) return fail(c, L3D_ERR_INVALID, "project lines: a device segment array is aligned to 8 bytes");
        l3d_device_image im{};
        im.ptr = seg3d; im.width = 12; im.height = n; im.channels = 1; im.dtype = L3D_F32; im.stride_y = 12; im.stride_x = 1; im.stride_c = 0;      // (6 doubles as 12 four-byte elements)
        if (int rc = device_image_pointer(c, im, msg)) return fail(c, rc, "project lines: segments: " + msg);
    }
    std::vector<float> h_segs;
    std::vector<int32_t> h_src;
    std::vector<unsigned char> h_fl;
    for (int k = 0; k <= m; ++k) cam_start[k] = 0;
    if (n > 0 && m > 0) {
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const double* d_segs = seg3d;
        if (!on_device) {
            HIPCHK(c, c->g0.reserve((size_t)n * 48));
            HIPCHK(c, hipMemcpyAsync(c->g0.p, seg3d, (size_t)n * 48, hipMemcpyHostToDevice, st));
            d_segs = c->g0.as<double>();
        }
        const int nw = (int)(((long long)n + 63) / 64);
        const int mc_max = project::chunk_cameras(c->opt.proj_chunk, n, m);
        // scratch (g1): cameras | words | counts | positions
        const size_t nwords_max = (size_t)mc_max * nw;
        const size_t o_cam = 0, o_words = al((size_t)mc_max * sizeof(l3d_camera)), o_cnt = o_words + al(nwords_max * 8), o_pos = o_cnt + al(nwords_max * 4);
        HIPCHK(c, c->g1.reserve(o_pos + al((nwords_max + 1) * 4)));
        char* sb = c->g1.as<char>();
        l3d_camera* d_cam = reinterpret_cast<l3d_camera*>(sb + o_cam);
        unsigned long long* d_words = reinterpret_cast<unsigned long long*>(sb + o_words);
        int* d_cnt = reinterpret_cast<int*>(sb + o_cnt);
        int* d_pos = reinterpret_cast<int*>(sb + o_pos);
        std::vector<int> h_pos;
        for (int c0 = 0; c0 < m; c0 += mc_max) {
            const int mc = std::min(mc_max, m - c0);
            const int nwords = mc * nw;
            HIPCHK(c, hipMemcpyAsync(d_cam, cameras + c0, (size_t)mc * sizeof(l3d_camera), hipMemcpyHostToDevice, st));
            const dim3 grid((unsigned)((nw + 3) / 4), (unsigned)mc);
            { ProfScope ps(c, "proj_count", st); hipLaunchKernelGGL(k_proj_count, grid, dim3(256), 0, st, d_segs, n, d_cam, nw, near_z, margin, d_words, d_cnt); }
            { ProfScope ps(c, "proj_scan", st); hipLaunchKernelGGL(k_proj_scan, dim3(1), dim3(kScanThreads), 0, st, d_cnt, d_pos, nwords); }
            // the outputs (g3), sized for every pair of the chunk: seg2d | src_index | flags
            const size_t pairs = (size_t)mc * (size_t)n;
            const size_t o_src = al(pairs * 16), o_fl = o_src + al(pairs * 4);
            HIPCHK(c, c->g3.reserve(o_fl + pairs));
            char* ob = c->g3.as<char>();
            { ProfScope ps(c, "proj_write", st); hipLaunchKernelGGL(k_proj_write, grid, dim3(256), 0, st, d_segs, n, d_cam, nw, near_z, margin, d_words, d_pos, reinterpret_cast<float4*>(ob), reinterpret_cast<int*>(ob + o_src), reinterpret_cast<unsigned char*>(ob + o_fl)); }
            // the cameras' starts: the positions of their first words
            h_pos.resize((size_t)mc + 1);
            HIPCHK(c, hipMemcpy2DAsync(h_pos.data(), sizeof(int), d_pos, (size_t)nw * sizeof(int), sizeof(int), (size_t)mc, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(h_pos.data() + mc, d_pos + nwords, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            const size_t base = h_src.size(), total = (size_t)h_pos[mc];
            if (total > pairs) return fail(c, L3D_ERR_HIP, "project lines: the scan's total exceeds the chunk's pairs");
            for (int k = 0; k < mc; ++k) cam_start[c0 + k] = (int64_t)(base + (size_t)h_pos[k]);
            if (total) {
                h_segs.resize((base + total) * 4); h_src.resize(base + total); h_fl.resize(base + total);
                HIPCHK(c, hipMemcpyAsync(h_segs.data() + base * 4, ob, total * 16, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipMemcpyAsync(h_src.data() + base, ob + o_src, total * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipMemcpyAsync(h_fl.data() + base, ob + o_fl, total, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
            }
        }
        cam_start[m] = (int64_t)h_src.size();
    }
    const int rp = project_pack(h_segs, h_src, h_fl, seg2d, src_index, flags);
    return rp ? fail(c, rp, "malloc") : L3D_OK;
}

}  // namespace

extern "C" const char* l3d_project_last_error(void) { return t_project_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_project_lines_host(const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d,
                                           int32_t** src_index, unsigned char** flags, int64_t* cam_start)
{
    std::string msg;
    if (int rc = project::check_arguments(seg3d, n, cameras, m, near_z, margin, seg2d, src_index, flags, cam_start, msg)) { t_project_err = msg; return rc; }
    std::vector<float> segs;
    std::vector<int32_t> src;
    std::vector<unsigned char> fl;
    project::run_host(seg3d, n, cameras, m, near_z, margin, segs, src, fl, cam_start);
    const int rp = project_pack(segs, src, fl, seg2d, src_index, flags);
    if (rp) t_project_err = "malloc";
    return rp;
}

extern "C" int l3d_project_lines(l3d_ctx* c, const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d,
                                 int32_t** src_index, unsigned char** flags, int64_t* cam_start)
{
    return project_run(c, seg3d, false, n, cameras, m, near_z, margin, seg2d, src_index, flags, cam_start);
}

extern "C" int l3d_project_lines_device(l3d_ctx* c, const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d,
                                        int32_t** src_index, unsigned char** flags, int64_t* cam_start)
{
    return project_run(c, seg3d, true, n, cameras, m, near_z, margin, seg2d, src_index, flags, cam_start);
}
