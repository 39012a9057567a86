// l3d_merge.hip -- duplicate 3-D lines found and grouped on the device ("MERGING DUPLICATE LINES" in include/line3d_amd.h; rules: l3d_merge.hpp).
// k_merge_prepare builds the table (P, d, L, tol: 64 bytes a line, and a flag).  The pair search is count / scan / write: 256 threads per workgroup, one
// row line i per lane in registers, column tiles of 256 lines staged in LDS (16 KB; every lane of a wave reads the same column entry: a broadcast),
// only j > i tested and the tiles in front of the row block skipped.  The tiles of a row block are cut into C contiguous chunks, the grid's y dimension
// (merge::chunks: a table of a few thousand lines has only a few dozen row blocks and would leave most of the device idle).  Each lane counts its own
// (row, chunk), one scan (wg_scan_excl) over the counts in (row, chunk) order gives the starts, and the write pass runs the same function again, each
// lane writing its pairs in ascending j: the list is ordered by (i, j) under any schedule and the search is three launches for any n.  The components
// come from the kernels of l3d_cc.hpp; k_merge_rep finds every component's longest line (atomicMax on the bits of L, which order as the value of a
// positive double, then atomicMin on the index among the lines that hold the maximum); k_merge_star tests every line against its representative and
// k_merge_group writes the groups.  The integer atomics make all of it independent of the schedule.
#include "l3d_cc.hpp"
#include "l3d_ctx.hpp"
#include "l3d_merge.hpp"
#include "l3d_scan.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

constexpr int kMergeTile = 256;
constexpr int kMergeSlack = 16;                    // spare (i, j) slots behind the list: filled with ones before the write pass and checked after it

__global__ __launch_bounds__(256) void k_merge_prepare(const double* __restrict__ lines, const double* __restrict__ tol, int n, merge::Line* __restrict__ tab,
                                                       unsigned char* __restrict__ elig)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s[6];
    for (int k = 0; k < 6; ++k) s[k] = lines[6 * (size_t)i + k];
    merge::Line o;
    elig[i] = merge::prepare(s, tol[i], o) ? 1 : 0;
    tab[i] = o;
}

// the column tiles [t0, t1) of chunk blockIdx.y of row block blockIdx.x: the tiles from the row block's own on, cut into gridDim.y contiguous parts
__device__ __forceinline__ void merge_chunk_tiles(int n, int& t0, int& t1)
{
    const int ntiles = (n + kMergeTile - 1) / kMergeTile, b = (int)blockIdx.x, C = (int)gridDim.y;
    const int len = (ntiles - b + C - 1) / C;
    t0 = min(ntiles, b + (int)blockIdx.y * len);
    t1 = min(ntiles, t0 + len);
}

// the pairs (i, j), j > i, of this lane's row line i within the workgroup's column tiles; WRITE: filed from slot `at` on, ascending j.  All 256 threads
// of the workgroup must call.
template <bool WRITE>
__device__ __forceinline__ int merge_row(const merge::Line* __restrict__ tab, const unsigned char* __restrict__ elig, const double* __restrict__ lines, int n,
                                         double cos_min, double max_gap, int at, l3d_edge* __restrict__ E, int2* __restrict__ pairs)
{
    __shared__ merge::Line s_tab[kMergeTile];
    __shared__ unsigned char s_el[kMergeTile];
    const int tid = threadIdx.x, i = blockIdx.x * kMergeTile + tid;
    const bool row = i < n && elig[i];
    merge::Line me = {};
    if (row) me = tab[i];
    int cnt = 0;
    int t0, t1;
    merge_chunk_tiles(n, t0, t1);                                      // (workgroup-uniform; the tiles in front of the row block hold only j < i)
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * kMergeTile, m = min(kMergeTile, n - j0);
        __syncthreads();                                               // the previous tile has been read
        const double* g = reinterpret_cast<const double*>(tab + j0);
        double* s = reinterpret_cast<double*>(s_tab);
        for (int e = tid; e < m * 8; e += kMergeTile) s[e] = g[e];
        if (tid < m) s_el[tid] = elig[j0 + tid];
        __syncthreads();
        if (row) {
            for (int jj = 0; jj < m; ++jj) {
                const int j = j0 + jj;
                if (j <= i || !s_el[jj]) continue;
                if (!merge::pair_test_ij(me, s_tab[jj], lines, i, j, cos_min, max_gap)) continue;
                if (WRITE) { l3d_edge e; e.i = i; e.j = j; e.w = 1.0f; E[(size_t)at + cnt] = e; pairs[(size_t)at + cnt] = make_int2(i, j); }
                ++cnt;
            }
        }
    }
    return cnt;
}

// cnt[i * C + c]: the pairs of row i in chunk c; total: their sum, in 64 bits (the scan's int total wraps beyond 2^31 - 1 and is not used then)
__global__ __launch_bounds__(256) void k_merge_count(const merge::Line* __restrict__ tab, const unsigned char* __restrict__ elig, const double* __restrict__ lines, int n,
                                                     double cos_min, double max_gap, int* __restrict__ cnt, unsigned long long* __restrict__ total)
{
    const int c = merge_row<false>(tab, elig, lines, n, cos_min, max_gap, 0, nullptr, nullptr);
    const int i = blockIdx.x * kMergeTile + threadIdx.x;
    if (i < n) cnt[(size_t)i * gridDim.y + blockIdx.y] = c;
    long long w = c;
    for (int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(total, (unsigned long long)w);
}

__global__ __launch_bounds__(kScanThreads) void k_merge_scan(const int* __restrict__ cnt, int* __restrict__ pos, int n)
{
    __shared__ int s_w[kScanThreads / 64];
    wg_scan_excl<kScanThreads>(cnt, pos, n, nullptr, s_w);
}

__global__ __launch_bounds__(256) void k_merge_write(const merge::Line* __restrict__ tab, const unsigned char* __restrict__ elig, const double* __restrict__ lines, int n,
                                                     double cos_min, double max_gap, const int* __restrict__ pos, l3d_edge* __restrict__ E, int2* __restrict__ pairs)
{
    const int i = blockIdx.x * kMergeTile + threadIdx.x;
    merge_row<true>(tab, elig, lines, n, cos_min, max_gap, i < n ? pos[(size_t)i * gridDim.y + blockIdx.y] : 0, E, pairs);
}

// phase 0: max_l[c] = the bits of the largest L of component c; phase 1: rep[c] = the lowest index among the lines that hold it
__global__ __launch_bounds__(256) void k_merge_rep(const merge::Line* __restrict__ tab, const unsigned char* __restrict__ elig, const int* __restrict__ comp, int n,
                                                   unsigned long long* __restrict__ max_l, int* __restrict__ rep, int phase)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !elig[i]) return;
    const unsigned long long b = (unsigned long long)__double_as_longlong(tab[i].L);       // (L > 0: the bits order as the values)
    const int c = comp[i];
    if (phase == 0) atomicMax(&max_l[c], b);
    else if (max_l[c] == b) atomicMin(&rep[c], i);
}

// THE STAR RULE: stay[i] iff line i is its component's representative or passes the pair test against it; low[c]: the lowest staying index
__global__ __launch_bounds__(256) void k_merge_star(const merge::Line* __restrict__ tab, const unsigned char* __restrict__ elig, const double* __restrict__ lines,
                                                    const int* __restrict__ comp, const int* __restrict__ rep, int n, double cos_min, double max_gap,
                                                    unsigned char* __restrict__ stay, int* __restrict__ low)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool s = false;
    if (elig[i]) {
        const int c = comp[i], r = rep[c];
        if (r == i) s = true;
        else if (r >= 0 && r < n) s = i < r ? merge::pair_test_ij(tab[i], tab[r], lines, i, r, cos_min, max_gap) : merge::pair_test_ij(tab[r], tab[i], lines, r, i, cos_min, max_gap);
        if (s) atomicMin(&low[c], i);
    }
    stay[i] = s ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_merge_group(const int* __restrict__ comp, const unsigned char* __restrict__ stay, const int* __restrict__ low, int n, int* __restrict__ group)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) group[i] = stay[i] ? low[comp[i]] : i;
}

}  // namespace l3d

namespace {

thread_local std::string t_merge_err;

// the pair list as a callee-allocated array (one spare pair: an empty list still hands out a pointer that l3d_free takes)
int32_t* merge_pack(const int32_t* src, size_t n_pairs)
{
    int32_t* o = static_cast<int32_t*>(malloc((n_pairs + 1) * 8));
    if (o && n_pairs) memcpy(o, src, n_pairs * 8);
    return o;
}

int merge_run(l3d_ctx* c, const double* lines, const double* tol, int n, const l3d_merge_params* prm, int32_t* group, int32_t** pairs, int* n_pairs, int32_t* counts)
{
    if (!c) return L3D_ERR_INVALID;
    std::string msg;
    if (int rc = merge::check_arguments(lines, tol, n, prm, group, pairs, n_pairs, counts, msg)) return fail(c, rc, msg);
    if (n == 0) {
        *pairs = merge_pack(nullptr, 0);
        return *pairs ? L3D_OK : fail(c, L3D_ERR_NOMEM, "malloc");
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const double cos_min = prm->cos_min, max_gap = prm->max_gap;
    const size_t N = (size_t)n;
    const size_t C = (size_t)merge::chunks(n);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // the table and the per-line arrays (merge_tab)
    const size_t o_lines = 0, o_tol = o_lines + al(N * 48), o_tab = o_tol + al(N * 8), o_maxl = o_tab + al(N * 64), o_total = o_maxl + al(N * 8), o_cnt = o_total + 256,
                 o_pos = o_cnt + al(N * C * 4), o_comp = o_pos + al((N * C + 1) * 4), o_changed = o_comp + al(N * 4), o_rep = o_changed + 256, o_low = o_rep + al(N * 4),
                 o_group = o_low + al(N * 4), o_elig = o_group + al(N * 4), o_stay = o_elig + al(N), o_end = o_stay + al(N);
    HIPCHK(c, c->merge_tab.reserve(o_end));
    char* b = c->merge_tab.as<char>();
    double* d_lines = reinterpret_cast<double*>(b + o_lines);
    double* d_tol = reinterpret_cast<double*>(b + o_tol);
    merge::Line* d_tab = reinterpret_cast<merge::Line*>(b + o_tab);
    unsigned long long* d_maxl = reinterpret_cast<unsigned long long*>(b + o_maxl);
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(b + o_total);
    int* d_cnt = reinterpret_cast<int*>(b + o_cnt);
    int* d_pos = reinterpret_cast<int*>(b + o_pos);
    int* d_comp = reinterpret_cast<int*>(b + o_comp);
    int* d_changed = reinterpret_cast<int*>(b + o_changed);
    int* d_rep = reinterpret_cast<int*>(b + o_rep);
    int* d_low = reinterpret_cast<int*>(b + o_low);
    int* d_group = reinterpret_cast<int*>(b + o_group);
    unsigned char* d_elig = reinterpret_cast<unsigned char*>(b + o_elig);
    unsigned char* d_stay = reinterpret_cast<unsigned char*>(b + o_stay);
    HIPCHK(c, hipMemcpyAsync(d_lines, lines, N * 48, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_tol, tol, N * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_total, 0, 8, st));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    { ProfScope ps(c, "merge_prepare", st); hipLaunchKernelGGL(k_merge_prepare, grid, block, 0, st, d_lines, d_tol, n, d_tab, d_elig); }
    // ---- the pair search: count, scan, write
    const dim3 sgrid(grid.x, (unsigned)C);
    { ProfScope ps(c, "merge_count", st); hipLaunchKernelGGL(k_merge_count, sgrid, block, 0, st, d_tab, d_elig, d_lines, n, cos_min, max_gap, d_cnt, d_total); }
    { ProfScope ps(c, "merge_scan", st); hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(kScanThreads), 0, st, d_cnt, d_pos, (int)(N * C)); }
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (total > (unsigned long long)merge::kMaxPairs) return fail(c, L3D_ERR_UNSUPPORTED, "merge lines: " + std::to_string(total) + " pairs, more than 2^31 - 1");
    const size_t np = (size_t)total;
    const size_t o_pairs = al(np * sizeof(l3d_edge));
    if (c->merge_pairs.reserve(o_pairs + (np + kMergeSlack) * 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, L3D_ERR_UNSUPPORTED, "merge lines: the list of " + std::to_string(total) + " pairs cannot be allocated on the device");
    }
    l3d_edge* d_E = c->merge_pairs.as<l3d_edge>();
    int2* d_pairs = reinterpret_cast<int2*>(c->merge_pairs.as<char>() + o_pairs);
    HIPCHK(c, hipMemsetAsync(d_pairs + np, 0xFF, kMergeSlack * 8, st));
    { ProfScope ps(c, "merge_cc_init", st); hipLaunchKernelGGL(k_cc_init, grid, block, 0, st, d_comp, n); }
    if (np) {
        { ProfScope ps(c, "merge_write", st); hipLaunchKernelGGL(k_merge_write, sgrid, block, 0, st, d_tab, d_elig, d_lines, n, cos_min, max_gap, d_pos, d_E, d_pairs); }
        // ---- the components: a few hooking rounds per look at the flag
        const dim3 egrid((unsigned)((np + 255) / 256));
        for (int round = 0;; ++round) {
            if (round == 64) return fail(c, L3D_ERR_HIP, "merge lines: the components did not converge");
            HIPCHK(c, hipMemsetAsync(d_changed, 0, 8, st));
            for (int r = 0; r < 3; ++r) {
                { ProfScope ps(c, "merge_cc_hook", st); hipLaunchKernelGGL(k_cc_hook, egrid, block, 0, st, d_E, (int)np, d_comp, d_changed + (r == 2 ? 0 : 1)); }
                { ProfScope ps(c, "merge_cc_compress", st); hipLaunchKernelGGL(k_cc_compress, grid, block, 0, st, d_comp, n); }
            }
            int h_changed = 0;
            HIPCHK(c, hipMemcpyAsync(&h_changed, d_changed, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (!h_changed) break;
        }
    }
    // ---- representatives, the star rule, the groups
    HIPCHK(c, hipMemsetAsync(d_maxl, 0, N * 8, st));
    HIPCHK(c, hipMemsetAsync(d_rep, 0x7F, N * 4, st));
    HIPCHK(c, hipMemsetAsync(d_low, 0x7F, N * 4, st));
    { ProfScope ps(c, "merge_rep", st); hipLaunchKernelGGL(k_merge_rep, grid, block, 0, st, d_tab, d_elig, d_comp, n, d_maxl, d_rep, 0); }
    { ProfScope ps(c, "merge_rep", st); hipLaunchKernelGGL(k_merge_rep, grid, block, 0, st, d_tab, d_elig, d_comp, n, d_maxl, d_rep, 1); }
    { ProfScope ps(c, "merge_star", st); hipLaunchKernelGGL(k_merge_star, grid, block, 0, st, d_tab, d_elig, d_lines, d_comp, d_rep, n, cos_min, max_gap, d_stay, d_low); }
    { ProfScope ps(c, "merge_group", st); hipLaunchKernelGGL(k_merge_group, grid, block, 0, st, d_comp, d_stay, d_low, n, d_group); }
    std::vector<int32_t> h_comp(N), h_pairs((np + kMergeSlack) * 2);
    std::vector<unsigned char> h_elig(N), h_stay(N);
    HIPCHK(c, hipMemcpyAsync(group, d_group, N * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_comp.data(), d_comp, N * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_elig.data(), d_elig, N, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_stay.data(), d_stay, N, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_pairs.data(), d_pairs, (np + kMergeSlack) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (size_t k = 2 * np; k < h_pairs.size(); ++k)
        if (h_pairs[k] != -1) return fail(c, L3D_ERR_HIP, "merge lines: the write pass wrote beyond the pairs it had counted");
    merge::tally(n, h_elig.data(), h_comp.data(), h_stay.data(), group, counts);
    *pairs = merge_pack(h_pairs.data(), np);
    if (!*pairs) return fail(c, L3D_ERR_NOMEM, "malloc");
    *n_pairs = (int)np;
    return L3D_OK;
}

}  // namespace

extern "C" const char* l3d_merge_last_error(void) { return t_merge_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_merge_lines_host(const double* lines, const double* tol, int n, const l3d_merge_params* prm, int32_t* group, int32_t** pairs, int* n_pairs,
                                         int32_t* counts)
{
    std::string msg;
    if (int rc = merge::check_arguments(lines, tol, n, prm, group, pairs, n_pairs, counts, msg)) { t_merge_err = msg; return rc; }
    std::vector<int32_t> pr;
    if (!merge::run_host(lines, tol, n, prm->cos_min, prm->max_gap, group, pr, counts)) { t_merge_err = "merge lines: more than 2^31 - 1 pairs"; return L3D_ERR_UNSUPPORTED; }
    *pairs = merge_pack(pr.data(), pr.size() / 2);
    if (!*pairs) { t_merge_err = "malloc"; return L3D_ERR_NOMEM; }
    *n_pairs = (int)(pr.size() / 2);
    return L3D_OK;
}

extern "C" int l3d_merge_lines(l3d_ctx* c, const double* lines, const double* tol, int n, const l3d_merge_params* prm, int32_t* group, int32_t** pairs, int* n_pairs,
                               int32_t* counts)
{
    const int rc = merge_run(c, lines, tol, n, prm, group, pairs, n_pairs, counts);
    if (rc && c) t_merge_err = l3d_last_error(c);
    return rc;
}
