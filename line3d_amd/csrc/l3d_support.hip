// l3d_support.hip -- the 2-D segments of every camera that support each 3-D segment, on the device ("SUPPORT OF 3-D LINES" in include/line3d_amd.h; rules:
// l3d_support.hpp).  k_sup_prepare builds the column table of all cameras (support::Col, 64 bytes a column).  The search is count / scan / write over
// chunks of cameras: 256 threads per workgroup, one (camera, 3-D segment) row per lane in registers, the camera the grid's y dimension (a wave never
// spans two cameras), the camera's column tiles of 256 staged in LDS (16 KB; every lane of a wave reads the same column entry: a broadcast) and cut into
// gridDim.z contiguous chunks when the rows alone cannot fill the device.  Each lane counts its own (camera, row, chunk), one scan (wg_scan_excl) over
// the counts in that order gives the starts, and the write pass runs the same functions again, each lane filing its records in ascending j: the list is
// ordered by (camera, k, j) under any schedule and the search is three launches per chunk of cameras.  k_sup_best runs once over the whole list: an
// integer atomicMin per column.  There is no floating-point atomic anywhere.
#include "l3d_ctx.hpp"
#include "l3d_detect.hpp"
#include "l3d_scan.hpp"
#include "l3d_support.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

constexpr int kSupTile = support::kTile;
constexpr int kSupSlack = 16;                      // spare records behind the list: filled with ones before the write pass and checked after it

__global__ __launch_bounds__(256) void k_sup_prepare(const float* __restrict__ seg2d, long long T, support::Col* __restrict__ tab, unsigned long long* __restrict__ n_elig)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (i < T) {
        const float4 g = reinterpret_cast<const float4*>(seg2d)[i];
        const float s[4] = { g.x, g.y, g.z, g.w };
        support::Col o;
        ok = support::make_col(s, o);
        tab[i] = o;
    }
    const unsigned long long b = (unsigned long long)__ballot(ok ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_elig, (unsigned long long)__popcll(b));
}

// The records of this lane's row (camera blockIdx.y of the chunk, 3-D segment blockIdx.x * 256 + threadIdx.x) within the workgroup's column tiles (chunk
// blockIdx.z of the camera's tiles); WRITE: filed from slot `at` on, ascending j.  has_row: the projection and the length rule give the lane a row.  All
// 256 threads of the workgroup must call.
template <bool WRITE>
__device__ __forceinline__ int sup_row(const double* __restrict__ seg3d, int n, const l3d_camera* __restrict__ cams, const long long* __restrict__ seg_start,
                                       const support::Col* __restrict__ tab, l3d_support_params p, long long at, l3d_support_record* __restrict__ rec, bool& has_row)
{
    __shared__ support::Col s_tab[kSupTile];
    const int tid = threadIdx.x, k = blockIdx.x * kSupTile + tid, c = blockIdx.y;
    support::Row me = {};
    has_row = false;
    if (k < n) {
        double s[6];
        for (int q = 0; q < 6; ++q) s[q] = seg3d[6 * (size_t)k + q];
        has_row = support::make_row(cams[c], s, p.near_z, p.margin, me);
    }
    if (!__syncthreads_or(has_row ? 1 : 0)) return 0;                  // (workgroup-uniform: no lane has a row)
    const long long col0 = seg_start[c];
    const int ncols = (int)(seg_start[c + 1] - col0);                  // (at most 2^31 - 1 a camera)
    const int ntiles = (int)(((long long)ncols + kSupTile - 1) / kSupTile), C = (int)gridDim.z;
    const int len = (ntiles + C - 1) / C;
    const int t0 = min(ntiles, (int)blockIdx.z * len), t1 = min(ntiles, t0 + len);
    int cnt = 0;
    for (int t = t0; t < t1; ++t) {
        const long long j0 = (long long)t * kSupTile;
        const int m = (int)min((long long)kSupTile, (long long)ncols - j0);
        __syncthreads();                                               // the previous tile has been read
        const double* g = reinterpret_cast<const double*>(tab + col0 + j0);
        double* s = reinterpret_cast<double*>(s_tab);
        for (int e = tid; e < m * 8; e += kSupTile) s[e] = g[e];
        __syncthreads();
        if (has_row) {
            for (int jj = 0; jj < m; ++jj) {
                const support::Col col = s_tab[jj];
                if (!(col.ok != 0.0)) continue;
                float dist, ov;
                if (!support::pair_test(me, col, p.dist_px, p.cos_min, p.min_overlap, dist, ov)) continue;
                if (WRITE) {
                    l3d_support_record o;
                    o.seg3d = k; o.seg2d = (int)(j0 + jj); o.dist = dist; o.overlap = ov;
                    rec[at + cnt] = o;
                }
                ++cnt;
            }
        }
    }
    return cnt;
}

// cnt[((c n) + k) C + z]: the records of row (c, k) in column chunk z; cam_total[c]: the records of camera c, cam_rows[c]: its rows, both in 64 bits
__global__ __launch_bounds__(256) void k_sup_count(const double* __restrict__ seg3d, int n, const l3d_camera* __restrict__ cams, const long long* __restrict__ seg_start,
                                                   const support::Col* __restrict__ tab, l3d_support_params p, int* __restrict__ cnt,
                                                   unsigned long long* __restrict__ cam_total, unsigned long long* __restrict__ cam_rows)
{
    bool has_row;
    const int v = sup_row<false>(seg3d, n, cams, seg_start, tab, p, 0, nullptr, has_row);
    const int k = blockIdx.x * kSupTile + threadIdx.x, c = blockIdx.y;
    if (k < n) cnt[((size_t)c * n + k) * gridDim.z + blockIdx.z] = v;
    long long w = v;
    for (int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o);
    const unsigned long long b = (unsigned long long)__ballot(has_row ? 1 : 0);
    if ((threadIdx.x & 63) == 0) {
        if (w) atomicAdd(&cam_total[c], (unsigned long long)w);
        if (blockIdx.z == 0 && b) atomicAdd(&cam_rows[c], (unsigned long long)__popcll(b));
    }
}

__global__ __launch_bounds__(kScanThreads) void k_sup_scan(const int* __restrict__ cnt, int* __restrict__ pos, int len)
{
    __shared__ int s_w[kScanThreads / 64];
    wg_scan_excl<kScanThreads>(cnt, pos, len, nullptr, s_w);
}

__global__ __launch_bounds__(256) void k_sup_write(const double* __restrict__ seg3d, int n, const l3d_camera* __restrict__ cams, const long long* __restrict__ seg_start,
                                                   const support::Col* __restrict__ tab, l3d_support_params p, const int* __restrict__ pos,
                                                   l3d_support_record* __restrict__ rec)
{
    const int k = blockIdx.x * kSupTile + threadIdx.x, c = blockIdx.y;
    bool has_row;
    sup_row<true>(seg3d, n, cams, seg_start, tab, p, k < n ? (long long)pos[((size_t)c * n + k) * gridDim.z + blockIdx.z] : 0, rec, has_row);
}

// keys[seg_start[c] + j] = the smallest (bits of dist << 32) | k among camera c's records for j (all ones before): grid-stride over the records of camera
// blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(256) void k_sup_best(const l3d_support_record* __restrict__ rec, const long long* __restrict__ cam_start, const long long* __restrict__ seg_start,
                                                  int m, unsigned long long* __restrict__ keys)
{
    for (int c = blockIdx.y; c < m; c += gridDim.y) {
        const long long r0 = cam_start[c], r1 = cam_start[c + 1], col0 = seg_start[c];
        for (long long r = r0 + (long long)blockIdx.x * 256 + threadIdx.x; r < r1; r += (long long)gridDim.x * 256) {
            const l3d_support_record o = rec[r];
            atomicMin(&keys[col0 + o.seg2d], support::best_key(o.dist, o.seg3d));
        }
    }
}

}  // namespace l3d

namespace {

thread_local std::string t_support_err;

// the record list as a callee-allocated array (one spare record: an empty list still hands out a pointer that l3d_free takes)
l3d_support_record* support_alloc(size_t n_rec)
{
    return static_cast<l3d_support_record*>(malloc((n_rec + 1) * sizeof(l3d_support_record)));
}

int support_run(l3d_ctx* c, const double* seg3d, const float* seg2d, bool on_device, int n, const l3d_camera* cameras, int m, const int64_t* seg_start,
                const l3d_support_params* prm, l3d_support_record** records, int64_t* cam_start, int32_t* best, int64_t* counts)
{
    if (!c) return L3D_ERR_INVALID;
    std::string msg;
    if (int rc = support::check_arguments(seg3d, n, cameras, m, seg2d, seg_start, prm, records, cam_start, best, counts, msg)) return fail(c, rc, msg);
    const long long T = m > 0 ? (long long)seg_start[m] : 0;
    // device memory of the caller's: the check an l3d_device_image gets, before anything is launched or read
    if (on_device) {
        if (n > 0) {
            if (reinterpret_cast<uintptr_t>(seg3d) & 7) return fail(c, L3D_ERR_INVALID, "support lines: a device array of 3-D segments is aligned to 8 bytes");
            l3d_device_image im{};
            im.ptr = seg3d; im.width = 12; im.height = n; im.channels = 1; im.dtype = L3D_F32; im.stride_y = 12; im.stride_x = 1; im.stride_c = 0;      // (6 doubles as 12 four-byte elements)
            if (int rc = device_image_pointer(c, im, msg)) return fail(c, rc, "support lines: 3-D segments: " + msg);
        }
        if (T > 0) {
            if (reinterpret_cast<uintptr_t>(seg2d) & 3) return fail(c, L3D_ERR_INVALID, "support lines: a device array of 2-D segments is aligned to 4 bytes");
            if (T > INT_MAX) return fail(c, L3D_ERR_UNSUPPORTED, "support lines: more than 2^31 - 1 2-D segments in device memory");
            l3d_device_image im{};
            im.ptr = seg2d; im.width = 4; im.height = (int)T; im.channels = 1; im.dtype = L3D_F32; im.stride_y = 4; im.stride_x = 1; im.stride_c = 0;
            if (int rc = device_image_pointer(c, im, msg)) return fail(c, rc, "support lines: 2-D segments: " + msg);
        }
    }
    for (long long i = 0; i < T; ++i) best[i] = -1;
    if (n == 0 || m == 0) {
        *records = support_alloc(0);
        return *records ? L3D_OK : fail(c, L3D_ERR_NOMEM, "malloc");
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const l3d_support_params p = *prm;
    const size_t M = (size_t)m, N = (size_t)n;
    const int mc_max = support::chunk_cameras(c->opt.sup_chunk, n, m);
    // the call's tables in the context's shared scratch: g0: 3-D segments | cameras | seg_start | cam_start | counters; g1: the column table | the keys |
    // the 2-D segments; g2: a chunk's counts | positions; g3: the records of the whole call
    const size_t o_seg = 0, o_cam = o_seg + al(N * 48), o_ss = o_cam + al(M * sizeof(l3d_camera)), o_cs = o_ss + al((M + 1) * 8), o_tot = o_cs + al((M + 1) * 8),
                 o_rows = o_tot + al(M * 8), o_elig = o_rows + al(M * 8), o_end0 = o_elig + 256;
    HIPCHK(c, c->g0.reserve(o_end0));
    char* b0 = c->g0.as<char>();
    const size_t o_tab = 0, o_keys = o_tab + al((size_t)T * sizeof(support::Col)), o_s2 = o_keys + al((size_t)T * 8), o_end1 = o_s2 + al((size_t)T * 16);
    if (c->g1.reserve(o_end1) != hipSuccess) { (void)hipGetLastError(); return fail(c, L3D_ERR_UNSUPPORTED, "support lines: the table of " + std::to_string(T) + " columns cannot be allocated on the device"); }
    char* b1 = c->g1.as<char>();
    const double* d_seg = seg3d;
    if (!on_device) {
        HIPCHK(c, hipMemcpyAsync(b0 + o_seg, seg3d, N * 48, hipMemcpyHostToDevice, st));
        d_seg = reinterpret_cast<const double*>(b0 + o_seg);
    }
    l3d_camera* d_cam = reinterpret_cast<l3d_camera*>(b0 + o_cam);
    long long* d_ss = reinterpret_cast<long long*>(b0 + o_ss);
    long long* d_cs = reinterpret_cast<long long*>(b0 + o_cs);
    unsigned long long* d_tot = reinterpret_cast<unsigned long long*>(b0 + o_tot);
    unsigned long long* d_rows = reinterpret_cast<unsigned long long*>(b0 + o_rows);
    unsigned long long* d_elig = reinterpret_cast<unsigned long long*>(b0 + o_elig);
    support::Col* d_tab = reinterpret_cast<support::Col*>(b1 + o_tab);
    unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(b1 + o_keys);
    HIPCHK(c, hipMemcpyAsync(d_cam, cameras, M * sizeof(l3d_camera), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_ss, seg_start, (M + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_elig, 0, 8, st));
    if (T > 0) {
        const float* d_s2 = seg2d;
        if (!on_device) {
            HIPCHK(c, hipMemcpyAsync(b1 + o_s2, seg2d, (size_t)T * 16, hipMemcpyHostToDevice, st));
            d_s2 = reinterpret_cast<const float*>(b1 + o_s2);
        }
        HIPCHK(c, hipMemsetAsync(d_keys, 0xFF, (size_t)T * 8, st));
        if (reinterpret_cast<uintptr_t>(d_s2) & 15) {                  // (k_sup_prepare reads float4: a device array at an odd offset is copied first)
            HIPCHK(c, hipMemcpyAsync(b1 + o_s2, d_s2, (size_t)T * 16, hipMemcpyDeviceToDevice, st));
            d_s2 = reinterpret_cast<const float*>(b1 + o_s2);
        }
        { ProfScope ps(c, "sup_prepare", st); hipLaunchKernelGGL(k_sup_prepare, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, d_s2, T, d_tab, d_elig); }
    }
    // ---- the search, chunk after chunk: count, scan, write
    std::vector<unsigned long long> h_tot((size_t)mc_max), h_rows((size_t)mc_max);
    std::vector<int64_t> guard((size_t)kSupSlack * 2);
    unsigned long long base = 0, rows = 0;
    for (int c0 = 0; c0 < m;) {
        const int mc = std::min(mc_max, m - c0);
        long long mxc = 0;
        for (int k = 0; k < mc; ++k) mxc = std::max(mxc, (long long)(seg_start[c0 + k + 1] - seg_start[c0 + k]));
        const int C = support::col_chunks(n, mc, mxc);
        const size_t scan_len = N * (size_t)mc * (size_t)C, o_pos = al(scan_len * 4);      // (at most 2^30; the previous chunk has been waited for)
        HIPCHK(c, c->g2.reserve(o_pos + al((scan_len + 1) * 4)));
        int* d_cnt = c->g2.as<int>();
        int* d_pos = reinterpret_cast<int*>(c->g2.as<char>() + o_pos);
        HIPCHK(c, hipMemsetAsync(d_tot + c0, 0, (size_t)mc * 8, st));
        HIPCHK(c, hipMemsetAsync(d_rows + c0, 0, (size_t)mc * 8, st));
        const dim3 grid((unsigned)((n + kSupTile - 1) / kSupTile), (unsigned)mc, (unsigned)C);
        { ProfScope ps(c, "sup_count", st); hipLaunchKernelGGL(k_sup_count, grid, dim3(256), 0, st, d_seg, n, d_cam + c0, d_ss + c0, d_tab, p, d_cnt, d_tot + c0, d_rows + c0); }
        HIPCHK(c, hipMemcpyAsync(h_tot.data(), d_tot + c0, (size_t)mc * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(h_rows.data(), d_rows + c0, (size_t)mc * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        const int use = support::cut_chunk(h_tot.data(), mc);
        if (use == 0) for (int k = 0; k <= m; ++k) cam_start[k] = 0;
        if (use == 0) return fail(c, L3D_ERR_UNSUPPORTED, "support lines: camera " + std::to_string(c0) + " alone yields " + std::to_string(h_tot[0]) + " records, more than 2^31 - 1");
        unsigned long long total = 0;
        for (int k = 0; k < use; ++k) { cam_start[c0 + k] = (int64_t)(base + total); total += h_tot[(size_t)k]; rows += h_rows[(size_t)k]; }
        const size_t need = (size_t)(base + total + kSupSlack) * sizeof(l3d_support_record);
        if (need > c->g3.cap) {
            hipError_t e = c->g3.grow_keep(std::max(need, 2 * c->g3.cap), (size_t)base * sizeof(l3d_support_record), st);
            if (e != hipSuccess) { (void)hipGetLastError(); e = c->g3.grow_keep(need, (size_t)base * sizeof(l3d_support_record), st); }
            if (e != hipSuccess) {
                (void)hipGetLastError();
                for (int k = 0; k <= m; ++k) cam_start[k] = 0;
                return fail(c, L3D_ERR_UNSUPPORTED, "support lines: the list of " + std::to_string(base + total) + " records cannot be allocated on the device");
            }
        }
        l3d_support_record* d_rec = c->g3.as<l3d_support_record>() + base;
        HIPCHK(c, hipMemsetAsync(d_rec + total, 0xFF, kSupSlack * sizeof(l3d_support_record), st));
        const int len = (int)(N * (size_t)use * (size_t)C);
        { ProfScope ps(c, "sup_scan", st); hipLaunchKernelGGL(k_sup_scan, dim3(1), dim3(kScanThreads), 0, st, d_cnt, d_pos, len); }
        const dim3 wgrid(grid.x, (unsigned)use, (unsigned)C);
        { ProfScope ps(c, "sup_write", st); hipLaunchKernelGGL(k_sup_write, wgrid, dim3(256), 0, st, d_seg, n, d_cam + c0, d_ss + c0, d_tab, p, d_pos, d_rec); }
        int h_scan_total = 0;
        HIPCHK(c, hipMemcpyAsync(guard.data(), d_rec + total, kSupSlack * sizeof(l3d_support_record), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&h_scan_total, d_pos + len, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        if ((unsigned long long)(long long)h_scan_total != total) return fail(c, L3D_ERR_HIP, "support lines: the scan's total differs from the counted records");
        for (int64_t g : guard)
            if (g != -1) return fail(c, L3D_ERR_HIP, "support lines: the write pass wrote beyond the records it had counted");
        base += total;
        c0 += use;
    }
    cam_start[m] = (int64_t)base;
    // ---- the best rows, once over the whole list
    std::vector<unsigned long long> h_keys((size_t)T);
    unsigned long long h_elig = 0;
    if (T > 0) {
        if (base) {
            HIPCHK(c, hipMemcpyAsync(d_cs, cam_start, (M + 1) * 8, hipMemcpyHostToDevice, st));
            unsigned long long most = 0;
            for (int k = 0; k < m; ++k) most = std::max(most, (unsigned long long)(cam_start[k + 1] - cam_start[k]));
            const dim3 bgrid((unsigned)std::min<unsigned long long>((most + 255) / 256, 4096ull), (unsigned)std::min(m, 65535));
            { ProfScope ps(c, "sup_best", st); hipLaunchKernelGGL(k_sup_best, bgrid, dim3(256), 0, st, c->g3.as<l3d_support_record>(), d_cs, d_ss, m, d_keys); }
        }
        HIPCHK(c, hipMemcpyAsync(h_keys.data(), d_keys, (size_t)T * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&h_elig, d_elig, 8, hipMemcpyDeviceToHost, st));
    }
    l3d_support_record* out = support_alloc((size_t)base);
    if (!out) return fail(c, L3D_ERR_NOMEM, "malloc");
    if (base) {
        const hipError_t e = hipMemcpyAsync(out, c->g3.p, (size_t)base * sizeof(l3d_support_record), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) { free(out); return fail(c, L3D_ERR_HIP, std::string("support lines: download: ") + hipGetErrorString(e)); }
    }
    {
        hipError_t e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) { free(out); return fail(c, L3D_ERR_HIP, std::string("support lines: ") + hipGetErrorString(e)); }
    }
    counts[0] = (int64_t)rows; counts[1] = (int64_t)h_elig; counts[2] = (int64_t)base; counts[3] = 0;
    if (T > 0) support::best_from_keys(h_keys.data(), T, best, counts);
    *records = out;
    return L3D_OK;
}

}  // namespace

extern "C" const char* l3d_support_last_error(void) { return t_support_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_support_lines_host(const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start,
                                           const l3d_support_params* prm, l3d_support_record** records, int64_t* cam_start, int32_t* best, int64_t* counts)
{
    std::string msg;
    if (int rc = support::check_arguments(seg3d, n, cameras, m, seg2d, seg_start, prm, records, cam_start, best, counts, msg)) { t_support_err = msg; return rc; }
    const int64_t T = m > 0 ? seg_start[m] : 0;
    for (int64_t i = 0; i < T; ++i) best[i] = -1;
    std::vector<l3d_support_record> rec;
    if (n > 0 && m > 0 && !support::run_host(seg3d, n, cameras, m, seg2d, seg_start, *prm, rec, cam_start, best, counts)) {
        for (int k = 0; k <= m; ++k) cam_start[k] = 0;
        for (int k = 0; k < 4; ++k) counts[k] = 0;
        t_support_err = "support lines: a camera alone yields more than 2^31 - 1 records";
        return L3D_ERR_UNSUPPORTED;
    }
    l3d_support_record* out = support_alloc(rec.size());
    if (!out) { t_support_err = "malloc"; return L3D_ERR_NOMEM; }
    if (!rec.empty()) memcpy(out, rec.data(), rec.size() * sizeof(l3d_support_record));
    *records = out;
    return L3D_OK;
}

extern "C" int l3d_support_lines(l3d_ctx* c, const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start,
                                 const l3d_support_params* prm, l3d_support_record** records, int64_t* cam_start, int32_t* best, int64_t* counts)
{
    const int rc = support_run(c, seg3d, seg2d, false, n, cameras, m, seg_start, prm, records, cam_start, best, counts);
    if (rc && c) t_support_err = l3d_last_error(c);
    return rc;
}

extern "C" int l3d_support_lines_device(l3d_ctx* c, const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start,
                                        const l3d_support_params* prm, l3d_support_record** records, int64_t* cam_start, int32_t* best, int64_t* counts)
{
    const int rc = support_run(c, seg3d, seg2d, true, n, cameras, m, seg_start, prm, records, cam_start, best, counts);
    if (rc && c) t_support_err = l3d_last_error(c);
    return rc;
}
