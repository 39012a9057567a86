// l3d_junction.hip -- the junctions of 3-D lines on the device ("JUNCTIONS OF 3-D LINES" in include/line3d_amd.h; rules: l3d_junction.hpp).
// k_junc_prepare builds the table (P, d, L, tol, ext and the eligibility: 80 bytes a line).  The search is count / scan / write, shaped like the merging's:
// 256 threads per workgroup, one row line i per lane in registers, column tiles of 256 lines staged in LDS (20 KB; every lane of a wave reads the same
// column entry: a broadcast), only j > i tested and the tiles in front of the row block skipped, the tiles of a row block cut into C contiguous chunks
// along the grid's y dimension (junction::chunks).  Each lane counts its own (row, chunk), one scan over the counts in (row, chunk) order gives the
// starts, and the write pass runs the same function again, each lane writing its records in ascending j: the list is ordered by (i, j) under any
// schedule and the search is three launches for any n.  The write pass files one edge per record (an L pair: its two nodes; any other: node 0 with
// itself, which hooks nothing), so the components of the 2 n line ends come from the kernels of l3d_cc.hpp.  k_junc_rep finds every component's
// representative (atomicMax on the bits of L, then atomicMin on the node among those that hold the maximum), k_junc_star decides who stays, counts the
// staying nodes and finds the lowest of them; k_junc_flag / k_junc_vscan number the vertices in the order of their lowest staying nodes.  The position
// of a vertex is a sum in ascending node order: k_junc_keys writes the key (lowest staying node, node) of every staying node that is not the
// representative, a radix sort orders the keys, and k_junc_vertex -- one lane per vertex -- walks its run of keys.  k_junc_attach picks per free end
// its T record by two integer atomicMin phases (bits of gap, then record index).  Integer atomics only: nothing depends on the schedule.
#include "l3d_cc.hpp"
#include "l3d_ctx.hpp"
#include "l3d_junction.hpp"
#include "l3d_scan.hpp"
#include "l3d_sort.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

constexpr int kJuncTile = 256;
constexpr int kJuncSlack = 16;                     // spare records behind the list: filled with ones before the write pass and checked after it
constexpr unsigned long long kJuncNoKey = ~0ull;

static_assert(sizeof(junction::Line) == 80, "a line of the junction table is 80 bytes");
static_assert(sizeof(l3d_junction_record) == 64 && sizeof(l3d_junction_vertex) == 32 && sizeof(l3d_junction_params) == 16, "the junction structs of the header");

__global__ __launch_bounds__(256) void k_junc_prepare(const double* __restrict__ lines, const double* __restrict__ tol, const double* __restrict__ ext, int n,
                                                      junction::Line* __restrict__ tab)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s[6];
    for (int k = 0; k < 6; ++k) s[k] = lines[6 * (size_t)i + k];
    junction::Line o;
    junction::prepare(s, tol[i], ext[i], o);
    tab[i] = o;
}

// the column tiles [t0, t1) of chunk blockIdx.y of row block blockIdx.x: the tiles from the row block's own on, cut into gridDim.y contiguous parts
__device__ __forceinline__ void junc_chunk_tiles(int n, int& t0, int& t1)
{
    const int ntiles = (n + kJuncTile - 1) / kJuncTile, b = (int)blockIdx.x, C = (int)gridDim.y;
    const int len = (ntiles - b + C - 1) / C;
    t0 = min(ntiles, b + (int)blockIdx.y * len);
    t1 = min(ntiles, t0 + len);
}

// the listed pairs (i, j), j > i, of this lane's row line i within the workgroup's column tiles; WRITE: filed from slot `at` on, ascending j (at + cnt
// stays below the next (row, chunk)'s start: both passes run the same function on the same table).  All 256 threads of the workgroup must call.
template <bool WRITE>
__device__ __forceinline__ int junc_row(const junction::Line* __restrict__ tab, int n, double cos_max, int crossings, int at, l3d_edge* __restrict__ E,
                                        l3d_junction_record* __restrict__ rec)
{
    __shared__ junction::Line s_tab[kJuncTile];
    const int tid = threadIdx.x, i = blockIdx.x * kJuncTile + tid;
    junction::Line me = {};
    if (i < n) me = tab[i];
    const bool row = me.elig != 0;
    int cnt = 0;
    int t0, t1;
    junc_chunk_tiles(n, t0, t1);                                       // (workgroup-uniform; the tiles in front of the row block hold only j < i)
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * kJuncTile, m = min(kJuncTile, n - j0);
        __syncthreads();                                               // the previous tile has been read
        const double* g = reinterpret_cast<const double*>(tab + j0);
        double* s = reinterpret_cast<double*>(s_tab);
        for (int e = tid; e < m * 10; e += kJuncTile) s[e] = g[e];
        __syncthreads();
        if (row) {
            for (int jj = 0; jj < m; ++jj) {
                const int j = j0 + jj;
                if (j <= i || !s_tab[jj].elig) continue;
                junction::Eval ev;
                if (!junction::pair_listed(me, s_tab[jj], cos_max, crossings, ev)) continue;
                if (WRITE) {
                    l3d_junction_record r;
                    junction::fill_record(i, j, ev, r);
                    rec[(size_t)at + cnt] = r;
                    const bool l = junction::kind_of(ev) == junction::kKindL;
                    l3d_edge e; e.i = l ? 2 * i + ev.wi : 0; e.j = l ? 2 * j + ev.wj : 0; e.w = 1.0f;
                    E[(size_t)at + cnt] = e;
                }
                ++cnt;
            }
        }
    }
    return cnt;
}

// cnt[i * C + c]: the records of row i in chunk c; total: their sum, in 64 bits (the scan's int total wraps beyond 2^31 - 1 and is not used then)
__global__ __launch_bounds__(256) void k_junc_count(const junction::Line* __restrict__ tab, int n, double cos_max, int crossings, int* __restrict__ cnt,
                                                    unsigned long long* __restrict__ total)
{
    const int c = junc_row<false>(tab, n, cos_max, crossings, 0, nullptr, nullptr);
    const int i = blockIdx.x * kJuncTile + threadIdx.x;
    if (i < n) cnt[(size_t)i * gridDim.y + blockIdx.y] = c;
    long long w = c;
    for (int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(total, (unsigned long long)w);
}

__global__ __launch_bounds__(kScanThreads) void k_junc_scan(const int* __restrict__ cnt, int* __restrict__ pos, int n)
{
    __shared__ int s_w[kScanThreads / 64];
    wg_scan_excl<kScanThreads>(cnt, pos, n, nullptr, s_w);
}

__global__ __launch_bounds__(256) void k_junc_write(const junction::Line* __restrict__ tab, int n, double cos_max, int crossings, const int* __restrict__ pos,
                                                    l3d_edge* __restrict__ E, l3d_junction_record* __restrict__ rec)
{
    const int i = blockIdx.x * kJuncTile + threadIdx.x;
    junc_row<true>(tab, n, cos_max, crossings, i < n ? pos[(size_t)i * gridDim.y + blockIdx.y] : 0, E, rec);
}

// per node v of an eligible line.  phase 0: max_l[c] = the bits of the largest L of component c; phase 1: rep[c] = the lowest node among those that hold it
__global__ __launch_bounds__(256) void k_junc_rep(const junction::Line* __restrict__ tab, const int* __restrict__ comp, int nn, unsigned long long* __restrict__ max_l,
                                                  int* __restrict__ rep, int phase)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nn || !tab[v >> 1].elig) return;
    const unsigned long long b = (unsigned long long)__double_as_longlong(tab[v >> 1].L);      // (L > 0: the bits order as the values)
    const int c = comp[v];
    if (phase == 0) atomicMax(&max_l[c], b);
    else if (max_l[c] == b) atomicMin(&rep[c], v);
}

// THE STAR RULE: stay[v]; low[c]: the lowest staying node, kept[c]: the staying nodes of component c
__global__ __launch_bounds__(256) void k_junc_star(const junction::Line* __restrict__ tab, const int* __restrict__ comp, const int* __restrict__ rep, int nn, double cos_max,
                                                   unsigned char* __restrict__ stay, int* __restrict__ low, int* __restrict__ kept)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nn) return;
    bool s = false;
    if (tab[v >> 1].elig) {
        const int c = comp[v], r = rep[c];
        junction::Eval e;
        if (r == v) s = true;
        else if (r >= 0 && r < nn) s = junction::spoke(tab, v, r, cos_max, e);
        if (s) { atomicMin(&low[c], v); atomicAdd(&kept[c], 1); }
    }
    stay[v] = s ? 1 : 0;
}

// flag[v] = 1 iff v is the lowest staying node of a vertex
__global__ __launch_bounds__(256) void k_junc_flag(const int* __restrict__ comp, const int* __restrict__ low, const int* __restrict__ kept, int nn, int* __restrict__ flag)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < nn) { const int c = comp[v]; flag[v] = (low[c] == v && kept[c] >= 2) ? 1 : 0; }
}

// key[v] = (lowest staying node of v's vertex, v) for a staying node of a vertex that is not the representative; all ones otherwise
__global__ __launch_bounds__(256) void k_junc_keys(const int* __restrict__ comp, const int* __restrict__ rep, const unsigned char* __restrict__ stay,
                                                   const int* __restrict__ low, const int* __restrict__ kept, int nn, unsigned long long* __restrict__ key)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nn) return;
    const int c = comp[v];
    key[v] = (stay[v] && kept[c] >= 2 && rep[c] != v) ? (((unsigned long long)(unsigned)low[c] << 32) | (unsigned)v) : kJuncNoKey;
}

// one lane per vertex: the lane at the first key of a run walks the run, ascending nodes.  vpos: the scan of the flags (the number of the vertex at its
// lowest staying node)
__global__ __launch_bounds__(256) void k_junc_vertex(const junction::Line* __restrict__ tab, const unsigned long long* __restrict__ key, const int* __restrict__ comp,
                                                     const int* __restrict__ rep, const int* __restrict__ vpos, int nn, double cos_max,
                                                     l3d_junction_vertex* __restrict__ vert)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nn) return;
    const unsigned long long k0 = key[p];
    if (k0 == kJuncNoKey) return;
    const unsigned lo = (unsigned)(k0 >> 32);
    if (p > 0 && (unsigned)(key[p - 1] >> 32) == lo) return;
    const int r = rep[comp[lo]];
    double S[3] = { 0.0, 0.0, 0.0 };
    int m = 0;
    for (int q = p; q < nn; ++q) {
        const unsigned long long k = key[q];
        if (k == kJuncNoKey || (unsigned)(k >> 32) != lo) break;
        junction::Eval e;
        if (!junction::spoke(tab, (int)(unsigned)k, r, cos_max, e)) continue;          // (a staying node: it passes)
        for (int c = 0; c < 3; ++c) S[c] = S[c] + e.X[c];
        ++m;
    }
    l3d_junction_vertex o;
    const double dm = (double)m;
    for (int c = 0; c < 3; ++c) o.X[c] = S[c] / dm;
    o.first_node = (int)lo; o.degree = m + 1;
    vert[vpos[lo]] = o;
}

// per T record whose end node is in no vertex.  phase 0: gmin[v] = the bits of the smallest gap (gap >= +0: the bits order as the values); phase 1:
// att[v] = the lowest record index among those that hold it
__global__ __launch_bounds__(256) void k_junc_attach(const l3d_junction_record* __restrict__ rec, int np, const int* __restrict__ comp, const unsigned char* __restrict__ stay,
                                                     const int* __restrict__ kept, unsigned long long* __restrict__ gmin, int* __restrict__ att, int phase)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= np) return;
    const l3d_junction_record r = rec[k];
    if (junction::kind_of(r) != junction::kKindT) return;
    const int v = junction::t_end_node(r);
    if (stay[v] && kept[comp[v]] >= 2) return;
    const unsigned long long b = (unsigned long long)__double_as_longlong(r.gap);
    if (phase == 0) atomicMin(&gmin[v], b);
    else if (gmin[v] == b) atomicMin(&att[v], k);
}

// node_vertex and node_attach
__global__ __launch_bounds__(256) void k_junc_finish(const int* __restrict__ comp, const unsigned char* __restrict__ stay, const int* __restrict__ low,
                                                     const int* __restrict__ kept, const int* __restrict__ vpos, const int* __restrict__ att, int nn,
                                                     int* __restrict__ node_vertex, int* __restrict__ node_attach)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nn) return;
    const int c = comp[v];
    const bool in = stay[v] && kept[c] >= 2;
    node_vertex[v] = in ? vpos[low[c]] : -1;
    node_attach[v] = (!in && att[v] != 0x7F7F7F7F) ? att[v] : -1;
}

}  // namespace l3d

namespace {

thread_local std::string t_junc_err;

// a list as a callee-allocated array (one spare element: an empty list still hands out a pointer that l3d_free takes)
template <typename T>
T* junc_pack(const T* src, size_t count)
{
    T* o = static_cast<T*>(malloc((count + 1) * sizeof(T)));
    if (o && count) memcpy(o, src, count * sizeof(T));
    return o;
}

int junc_run(l3d_ctx* c, const double* lines, const double* tol, const double* ext, int n, const l3d_junction_params* prm, l3d_junction_record** records,
             int* n_records, int32_t* node_vertex, l3d_junction_vertex** vertices, int* n_vertices, int32_t* node_attach, int32_t* counts)
{
    if (!c) return L3D_ERR_INVALID;
    std::string msg;
    if (int rc = junction::check_arguments(lines, tol, ext, n, prm, records, n_records, node_vertex, vertices, n_vertices, node_attach, counts, msg)) return fail(c, rc, msg);
    if (n == junction::kMaxLines) return fail(c, L3D_ERR_UNSUPPORTED, "junction lines: 2^30 lines have 2^31 nodes, more than the device numbers");
    if (n == 0) {
        *records = junc_pack<l3d_junction_record>(nullptr, 0);
        *vertices = junc_pack<l3d_junction_vertex>(nullptr, 0);
        if (!*records || !*vertices) { free(*records); free(*vertices); *records = nullptr; *vertices = nullptr; return fail(c, L3D_ERR_NOMEM, "malloc"); }
        return L3D_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const double cos_max = prm->cos_max;
    const int crossings = prm->crossings;
    const size_t N = (size_t)n, NN = 2 * N;
    const int nn = (int)NN;
    const size_t C = (size_t)junction::chunks(n);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t sort_bytes = 0;
    HIPCHK(c, sort_keys_u64(nullptr, sort_bytes, nullptr, nullptr, nn, 0, 64, st));
    // the table, the per-line and the per-node arrays (junc_tab)
    const size_t o_lines = 0, o_tol = o_lines + al(N * 48), o_ext = o_tol + al(N * 8), o_tab = o_ext + al(N * 8), o_total = o_tab + al(N * 80), o_cnt = o_total + 256,
                 o_pos = o_cnt + al(N * C * 4), o_comp = o_pos + al((N * C + 1) * 4), o_changed = o_comp + al(NN * 4), o_maxl = o_changed + 256, o_rep = o_maxl + al(NN * 8),
                 o_low = o_rep + al(NN * 4), o_kept = o_low + al(NN * 4), o_flag = o_kept + al(NN * 4), o_vpos = o_flag + al(NN * 4), o_key = o_vpos + al((NN + 1) * 4),
                 o_key2 = o_key + al(NN * 8), o_gmin = o_key2 + al(NN * 8), o_att = o_gmin + al(NN * 8), o_nv = o_att + al(NN * 4), o_na = o_nv + al(NN * 4),
                 o_stay = o_na + al(NN * 4), o_vert = o_stay + al(NN), o_sort = o_vert + al(N * 32), o_end = o_sort + al(sort_bytes);
    if (c->junc_tab.reserve(o_end) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, L3D_ERR_UNSUPPORTED, "junction lines: the table of " + std::to_string(n) + " lines cannot be allocated on the device");
    }
    char* b = c->junc_tab.as<char>();
    double* d_lines = reinterpret_cast<double*>(b + o_lines);
    double* d_tol = reinterpret_cast<double*>(b + o_tol);
    double* d_ext = reinterpret_cast<double*>(b + o_ext);
    junction::Line* d_tab = reinterpret_cast<junction::Line*>(b + o_tab);
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(b + o_total);
    int* d_cnt = reinterpret_cast<int*>(b + o_cnt);
    int* d_pos = reinterpret_cast<int*>(b + o_pos);
    int* d_comp = reinterpret_cast<int*>(b + o_comp);
    int* d_changed = reinterpret_cast<int*>(b + o_changed);
    unsigned long long* d_maxl = reinterpret_cast<unsigned long long*>(b + o_maxl);
    int* d_rep = reinterpret_cast<int*>(b + o_rep);
    int* d_low = reinterpret_cast<int*>(b + o_low);
    int* d_kept = reinterpret_cast<int*>(b + o_kept);
    int* d_flag = reinterpret_cast<int*>(b + o_flag);
    int* d_vpos = reinterpret_cast<int*>(b + o_vpos);
    unsigned long long* d_key = reinterpret_cast<unsigned long long*>(b + o_key);
    unsigned long long* d_key2 = reinterpret_cast<unsigned long long*>(b + o_key2);
    unsigned long long* d_gmin = reinterpret_cast<unsigned long long*>(b + o_gmin);
    int* d_att = reinterpret_cast<int*>(b + o_att);
    int* d_nv = reinterpret_cast<int*>(b + o_nv);
    int* d_na = reinterpret_cast<int*>(b + o_na);
    unsigned char* d_stay = reinterpret_cast<unsigned char*>(b + o_stay);
    l3d_junction_vertex* d_vert = reinterpret_cast<l3d_junction_vertex*>(b + o_vert);
    void* d_sort = b + o_sort;
    HIPCHK(c, hipMemcpyAsync(d_lines, lines, N * 48, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_tol, tol, N * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_ext, ext, N * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_total, 0, 8, st));
    const dim3 grid((unsigned)((n + 255) / 256)), ngrid((unsigned)((NN + 255) / 256)), block(256);
    { ProfScope ps(c, "junc_prepare", st); hipLaunchKernelGGL(k_junc_prepare, grid, block, 0, st, d_lines, d_tol, d_ext, n, d_tab); }
    // ---- the search: count, scan, write
    const dim3 sgrid(grid.x, (unsigned)C);
    { ProfScope ps(c, "junc_count", st); hipLaunchKernelGGL(k_junc_count, sgrid, block, 0, st, d_tab, n, cos_max, crossings, d_cnt, d_total); }
    { ProfScope ps(c, "junc_scan", st); hipLaunchKernelGGL(k_junc_scan, dim3(1), dim3(kScanThreads), 0, st, d_cnt, d_pos, (int)(N * C)); }
    unsigned long long total = 0;
    std::vector<junction::Line> h_tab(N);
    HIPCHK(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_tab.data(), d_tab, N * 80, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (total > (unsigned long long)junction::kMaxRecords)
        return fail(c, L3D_ERR_UNSUPPORTED, "junction lines: " + std::to_string(total) + " records, more than 2^31 - 1");
    const size_t np = (size_t)total;
    std::vector<l3d_junction_record> h_rec(np + kJuncSlack);
    std::vector<l3d_junction_vertex> h_vert;
    std::vector<int32_t> h_comp(NN);
    std::vector<unsigned char> h_stay(NN, 0);
    int nv = 0;
    if (np == 0) {
        // no record: no edge, no vertex, no attachment -- nothing more is launched
        for (size_t v = 0; v < NN; ++v) { node_vertex[v] = -1; node_attach[v] = -1; h_comp[v] = (int32_t)v; }
    } else {
        const size_t o_edges = al((np + kJuncSlack) * sizeof(l3d_junction_record));
        if (c->junc_rec.reserve(o_edges + np * sizeof(l3d_edge)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, L3D_ERR_UNSUPPORTED, "junction lines: the list of " + std::to_string(total) + " records cannot be allocated on the device");
        }
        l3d_junction_record* d_rec = c->junc_rec.as<l3d_junction_record>();
        l3d_edge* d_E = reinterpret_cast<l3d_edge*>(c->junc_rec.as<char>() + o_edges);
        HIPCHK(c, hipMemsetAsync(d_rec + np, 0xFF, kJuncSlack * sizeof(l3d_junction_record), st));
        { ProfScope ps(c, "junc_write", st); hipLaunchKernelGGL(k_junc_write, sgrid, block, 0, st, d_tab, n, cos_max, crossings, d_pos, d_E, d_rec); }
        // ---- the components of the line ends: a few hooking rounds per look at the flag
        { ProfScope ps(c, "junc_cc_init", st); hipLaunchKernelGGL(k_cc_init, ngrid, block, 0, st, d_comp, nn); }
        const dim3 egrid((unsigned)((np + 255) / 256));
        for (int round = 0;; ++round) {
            if (round == 64) return fail(c, L3D_ERR_HIP, "junction lines: the components did not converge");
            HIPCHK(c, hipMemsetAsync(d_changed, 0, 8, st));
            for (int r = 0; r < 3; ++r) {
                { ProfScope ps(c, "junc_cc_hook", st); hipLaunchKernelGGL(k_cc_hook, egrid, block, 0, st, d_E, (int)np, d_comp, d_changed + (r == 2 ? 0 : 1)); }
                { ProfScope ps(c, "junc_cc_compress", st); hipLaunchKernelGGL(k_cc_compress, ngrid, block, 0, st, d_comp, nn); }
            }
            int h_changed = 0;
            HIPCHK(c, hipMemcpyAsync(&h_changed, d_changed, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (!h_changed) break;
        }
        // ---- representatives, the star rule, the vertices in order, their positions, the attachments
        HIPCHK(c, hipMemsetAsync(d_maxl, 0, NN * 8, st));
        HIPCHK(c, hipMemsetAsync(d_rep, 0x7F, NN * 4, st));
        HIPCHK(c, hipMemsetAsync(d_low, 0x7F, NN * 4, st));
        HIPCHK(c, hipMemsetAsync(d_kept, 0, NN * 4, st));
        HIPCHK(c, hipMemsetAsync(d_gmin, 0xFF, NN * 8, st));
        HIPCHK(c, hipMemsetAsync(d_att, 0x7F, NN * 4, st));
        { ProfScope ps(c, "junc_rep", st); hipLaunchKernelGGL(k_junc_rep, ngrid, block, 0, st, d_tab, d_comp, nn, d_maxl, d_rep, 0); }
        { ProfScope ps(c, "junc_rep", st); hipLaunchKernelGGL(k_junc_rep, ngrid, block, 0, st, d_tab, d_comp, nn, d_maxl, d_rep, 1); }
        { ProfScope ps(c, "junc_star", st); hipLaunchKernelGGL(k_junc_star, ngrid, block, 0, st, d_tab, d_comp, d_rep, nn, cos_max, d_stay, d_low, d_kept); }
        { ProfScope ps(c, "junc_flag", st); hipLaunchKernelGGL(k_junc_flag, ngrid, block, 0, st, d_comp, d_low, d_kept, nn, d_flag); }
        { ProfScope ps(c, "junc_vscan", st); hipLaunchKernelGGL(k_junc_scan, dim3(1), dim3(kScanThreads), 0, st, d_flag, d_vpos, nn); }
        { ProfScope ps(c, "junc_keys", st); hipLaunchKernelGGL(k_junc_keys, ngrid, block, 0, st, d_comp, d_rep, d_stay, d_low, d_kept, nn, d_key); }
        { ProfScope ps(c, "junc_sort", st); HIPCHK(c, sort_keys_u64(d_sort, sort_bytes, d_key, d_key2, nn, 0, 64, st)); }
        { ProfScope ps(c, "junc_vertex", st); hipLaunchKernelGGL(k_junc_vertex, ngrid, block, 0, st, d_tab, d_key2, d_comp, d_rep, d_vpos, nn, cos_max, d_vert); }
        { ProfScope ps(c, "junc_attach", st); hipLaunchKernelGGL(k_junc_attach, egrid, block, 0, st, d_rec, (int)np, d_comp, d_stay, d_kept, d_gmin, d_att, 0); }
        { ProfScope ps(c, "junc_attach", st); hipLaunchKernelGGL(k_junc_attach, egrid, block, 0, st, d_rec, (int)np, d_comp, d_stay, d_kept, d_gmin, d_att, 1); }
        { ProfScope ps(c, "junc_finish", st); hipLaunchKernelGGL(k_junc_finish, ngrid, block, 0, st, d_comp, d_stay, d_low, d_kept, d_vpos, d_att, nn, d_nv, d_na); }
        HIPCHK(c, hipMemcpyAsync(&nv, d_vpos + NN, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(node_vertex, d_nv, NN * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(node_attach, d_na, NN * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(h_comp.data(), d_comp, NN * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(h_stay.data(), d_stay, NN, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(h_rec.data(), d_rec, (np + kJuncSlack) * sizeof(l3d_junction_record), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        if (nv < 0 || (size_t)nv > N) return fail(c, L3D_ERR_HIP, "junction lines: the number of vertices is out of range");
        h_vert.resize((size_t)nv);
        if (nv) HIPCHK(c, hipMemcpy(h_vert.data(), d_vert, (size_t)nv * sizeof(l3d_junction_vertex), hipMemcpyDeviceToHost));
        const unsigned char* guard = reinterpret_cast<const unsigned char*>(h_rec.data() + np);
        for (size_t k = 0; k < kJuncSlack * sizeof(l3d_junction_record); ++k)
            if (guard[k] != 0xFF) return fail(c, L3D_ERR_HIP, "junction lines: the write pass wrote beyond the records it had counted");
    }
    junction::tally(n, h_tab.data(), h_rec.data(), np, h_comp.data(), h_stay.data(), nv, node_attach, counts);
    *records = junc_pack(h_rec.data(), np);
    *vertices = junc_pack(h_vert.data(), (size_t)nv);
    if (!*records || !*vertices) { free(*records); free(*vertices); *records = nullptr; *vertices = nullptr; return fail(c, L3D_ERR_NOMEM, "malloc"); }
    *n_records = (int)np;
    *n_vertices = nv;
    return L3D_OK;
}

}  // namespace

extern "C" const char* l3d_junction_last_error(void) { return t_junc_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_junction_lines_host(const double* lines, const double* tol, const double* ext, int n, const l3d_junction_params* prm,
                                            l3d_junction_record** records, int* n_records, int32_t* node_vertex, l3d_junction_vertex** vertices, int* n_vertices,
                                            int32_t* node_attach, int32_t* counts)
{
    std::string msg;
    if (int rc = junction::check_arguments(lines, tol, ext, n, prm, records, n_records, node_vertex, vertices, n_vertices, node_attach, counts, msg)) { t_junc_err = msg; return rc; }
    std::vector<l3d_junction_record> rec;
    std::vector<l3d_junction_vertex> vert;
    if (!junction::run_host(lines, tol, ext, n, prm->cos_max, prm->crossings, rec, node_vertex, vert, node_attach, counts)) {
        t_junc_err = "junction lines: more than 2^31 - 1 records";
        return L3D_ERR_UNSUPPORTED;
    }
    *records = junc_pack(rec.data(), rec.size());
    *vertices = junc_pack(vert.data(), vert.size());
    if (!*records || !*vertices) { free(*records); free(*vertices); *records = nullptr; *vertices = nullptr; t_junc_err = "malloc"; return L3D_ERR_NOMEM; }
    *n_records = (int)rec.size();
    *n_vertices = (int)vert.size();
    return L3D_OK;
}

extern "C" int l3d_junction_lines(l3d_ctx* c, const double* lines, const double* tol, const double* ext, int n, const l3d_junction_params* prm,
                                  l3d_junction_record** records, int* n_records, int32_t* node_vertex, l3d_junction_vertex** vertices, int* n_vertices,
                                  int32_t* node_attach, int32_t* counts)
{
    const int rc = junc_run(c, lines, tol, ext, n, prm, records, n_records, node_vertex, vertices, n_vertices, node_attach, counts);
    if (rc && c) t_junc_err = l3d_last_error(c);
    return rc;
}
