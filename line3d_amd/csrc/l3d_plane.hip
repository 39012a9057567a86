// l3d_plane.hip -- the planes of 3-D lines on the device ("PLANES OF 3-D LINES" in include/line3d_amd.h; rules: l3d_plane.hpp).
// k_plane_prepare builds the line table (96 bytes a line), k_plane_hyp the hypothesis table, one lane per seed: what the pair search reads (the plane,
// the two lines' ends and tolerances: 160 bytes) and, apart from it, the point and the weight (32 bytes).  The hypothesis search is count / scan /
// write, shaped like the junctions': 256 threads per workgroup, one row hypothesis h per lane in registers, column tiles of 256 hypotheses staged in
// LDS (40 KB: four workgroups a CU; every lane of a wave reads the same column entry: a broadcast), only g > h tested and the tiles in front of the row
// block skipped, the tiles of a row block cut into C contiguous chunks along the grid's y dimension (plane::chunks).  Each lane counts its own (row,
// chunk), one scan gives the starts, the write pass runs the same function again: three launches for any m.  The components come from the kernels of
// l3d_cc.hpp.  k_plane_rep finds the representatives (atomicMax on the bits of A, then atomicMin on the index), k_plane_star decides who stays and
// finds the lowest staying hypothesis, k_plane_flag and a scan number the candidates in that order.  The parameters are sums in ascending hypothesis
// order: k_plane_keys writes (lowest staying hypothesis, hypothesis) per staying hypothesis, a radix sort orders the keys, and k_plane_param -- one
// lane per candidate -- walks its run.  Membership is one (candidate, line) pair per lane and a ballot word per wave, every wave within one candidate:
// k_plane_mcount counts, k_plane_keep decides which candidates are planes and sums their members in 64 bits, a scan numbers the planes,
// k_plane_mmask clears the words of the dropped candidates, one scan gives every wave its start and k_plane_mwrite files the records, ascending by
// (plane, line) under any schedule.  k_plane_seed finds a staying hypothesis's two lines in its plane's run by bisection and sets their SEED flags
// (atomicOr), k_plane_extent -- one lane per plane over its records -- folds the extents, k_plane_finish writes hyp_plane.  Integer atomics only.
#include "l3d_cc.hpp"
#include "l3d_ctx.hpp"
#include "l3d_plane.hpp"
#include "l3d_scan.hpp"
#include "l3d_sort.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

constexpr int kPlaneTile = 256;
constexpr int kPlaneSlack = 16;                    // spare records behind a list: filled with ones before the write pass and checked after it
constexpr unsigned long long kPlaneNoKey = ~0ull;
constexpr long long kPlaneMaxWaves = 1ll << 30;    // the membership pass's wave words: one scan's length

static_assert(sizeof(plane::Line) == 96 && sizeof(plane::Hyp) == 160 && sizeof(plane::HypAux) == 32, "the tables of the planes");
static_assert(sizeof(l3d_plane) == 128 && sizeof(l3d_plane_member) == 16 && sizeof(l3d_plane_params) == 24, "the plane structs of the header");

// cnt[0] += the eligible lines
__global__ __launch_bounds__(256) void k_plane_prepare(const double* __restrict__ lines, const double* __restrict__ tol, int n, plane::Line* __restrict__ tab,
                                                       int* __restrict__ cnt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (i < n) {
        double s[6];
        for (int k = 0; k < 6; ++k) s[k] = lines[6 * (size_t)i + k];
        plane::Line o;
        ok = plane::prepare(s, tol[i], o);
        tab[i] = o;
    }
    const int w = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&cnt[0], w);
}

// one lane per seed; cnt[1] += the eligible hypotheses
__global__ __launch_bounds__(256) void k_plane_hyp(const plane::Line* __restrict__ tab, int n, const int* __restrict__ seeds, int m, double cos_max,
                                                   plane::Hyp* __restrict__ hyp, plane::HypAux* __restrict__ aux, int* __restrict__ cnt)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (h < m) {
        plane::Hyp o; plane::HypAux a;
        ok = plane::hypothesis(tab, n, seeds[2 * (size_t)h], seeds[2 * (size_t)h + 1], cos_max, o, a);
        hyp[h] = o; aux[h] = a;
    }
    const int w = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&cnt[1], w);
}

// the column tiles [t0, t1) of chunk blockIdx.y of row block blockIdx.x: the tiles from the row block's own on, cut into gridDim.y contiguous parts
__device__ __forceinline__ void plane_chunk_tiles(int m, int& t0, int& t1)
{
    const int ntiles = (m + kPlaneTile - 1) / kPlaneTile, b = (int)blockIdx.x, C = (int)gridDim.y;
    const int len = (ntiles - b + C - 1) / C;
    t0 = min(ntiles, b + (int)blockIdx.y * len);
    t1 = min(ntiles, t0 + len);
}

// the passing pairs (h, g), g > h, of this lane's row hypothesis h within the workgroup's column tiles; WRITE: filed from slot `at` on, ascending g
// (at + cnt stays below the next (row, chunk)'s start: both passes run the same function on the same table).  All 256 threads must call.
template <bool WRITE>
__device__ __forceinline__ int plane_row(const plane::Hyp* __restrict__ hyp, int m, double cos_min, int at, l3d_edge* __restrict__ E)
{
    __shared__ plane::Hyp s_hyp[kPlaneTile];
    const int tid = threadIdx.x, h = blockIdx.x * kPlaneTile + tid;
    plane::Hyp me = {};
    if (h < m) me = hyp[h];
    const bool row = me.elig != 0;
    int cnt = 0;
    int t0, t1;
    plane_chunk_tiles(m, t0, t1);                                      // (workgroup-uniform; the tiles in front of the row block hold only g < h)
    for (int t = t0; t < t1; ++t) {
        const int g0 = t * kPlaneTile, mt = min(kPlaneTile, m - g0);
        __syncthreads();                                               // the previous tile has been read
        const double* src = reinterpret_cast<const double*>(hyp + g0);
        double* s = reinterpret_cast<double*>(s_hyp);
        for (int e = tid; e < mt * 20; e += kPlaneTile) s[e] = src[e];
        __syncthreads();
        if (row) {
            for (int gg = 0; gg < mt; ++gg) {
                const int g = g0 + gg;
                if (g <= h || !s_hyp[gg].elig) continue;
                if (!plane::pair_test(me, s_hyp[gg], cos_min)) continue;
                if (WRITE) { l3d_edge e; e.i = h; e.j = g; e.w = 1.0f; E[(size_t)at + cnt] = e; }
                ++cnt;
            }
        }
    }
    return cnt;
}

// cnt[h * C + c]: the edges of row h in chunk c; total: their sum, in 64 bits (the scan's int total wraps beyond 2^31 - 1 and is not used then)
__global__ __launch_bounds__(256) void k_plane_count(const plane::Hyp* __restrict__ hyp, int m, double cos_min, int* __restrict__ cnt, unsigned long long* __restrict__ total)
{
    const int c = plane_row<false>(hyp, m, cos_min, 0, nullptr);
    const int h = blockIdx.x * kPlaneTile + threadIdx.x;
    if (h < m) cnt[(size_t)h * gridDim.y + blockIdx.y] = c;
    long long w = c;
    for (int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(total, (unsigned long long)w);
}

__global__ __launch_bounds__(kScanThreads) void k_plane_scan(const int* __restrict__ cnt, int* __restrict__ pos, int n)
{
    __shared__ int s_w[kScanThreads / 64];
    wg_scan_excl<kScanThreads>(cnt, pos, n, nullptr, s_w);
}

__global__ __launch_bounds__(256) void k_plane_write(const plane::Hyp* __restrict__ hyp, int m, double cos_min, const int* __restrict__ pos, l3d_edge* __restrict__ E)
{
    const int h = blockIdx.x * kPlaneTile + threadIdx.x;
    plane_row<true>(hyp, m, cos_min, h < m ? pos[(size_t)h * gridDim.y + blockIdx.y] : 0, E);
}

// per eligible hypothesis.  phase 0: max_a[c] = the bits of the largest A of component c (A >= +0: the bits order as the values); phase 1: rep[c] = the
// lowest index among those that hold it
__global__ __launch_bounds__(256) void k_plane_rep(const plane::Hyp* __restrict__ hyp, const plane::HypAux* __restrict__ aux, const int* __restrict__ comp, int m,
                                                   unsigned long long* __restrict__ max_a, int* __restrict__ rep, int phase)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= m || !hyp[h].elig) return;
    const unsigned long long b = (unsigned long long)__double_as_longlong(aux[h].A);
    const int c = comp[h];
    if (phase == 0) atomicMax(&max_a[c], b);
    else if (max_a[c] == b) atomicMin(&rep[c], h);
}

// THE STAR RULE: stay[h]; low[c]: the lowest staying hypothesis of component c; cnt[4] += the released
__global__ __launch_bounds__(256) void k_plane_star(const plane::Hyp* __restrict__ hyp, const int* __restrict__ comp, const int* __restrict__ rep, int m, double cos_min,
                                                    unsigned char* __restrict__ stay, int* __restrict__ low, int* __restrict__ cnt)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= m) return;
    bool s = false;
    if (hyp[h].elig) {
        const int c = comp[h], r = rep[c];
        if (r == h) s = true;
        else if (r >= 0 && r < m) s = plane::pair_test(hyp[h], hyp[r], cos_min);
        if (s) atomicMin(&low[c], h);
        else atomicAdd(&cnt[4], 1);
    }
    stay[h] = s ? 1 : 0;
}

// flag[h] = 1 iff h is the lowest staying hypothesis of its component: a candidate
__global__ __launch_bounds__(256) void k_plane_flag(const int* __restrict__ comp, const unsigned char* __restrict__ stay, const int* __restrict__ low, int m,
                                                    int* __restrict__ flag)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h < m) flag[h] = (stay[h] && low[comp[h]] == h) ? 1 : 0;
}

// key[h] = (lowest staying hypothesis of h's candidate, h) for a staying hypothesis; all ones otherwise
__global__ __launch_bounds__(256) void k_plane_keys(const int* __restrict__ comp, const unsigned char* __restrict__ stay, const int* __restrict__ low, int m,
                                                    unsigned long long* __restrict__ key)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= m) return;
    key[h] = stay[h] ? (((unsigned long long)(unsigned)low[comp[h]] << 32) | (unsigned)h) : kPlaneNoKey;
}

// one lane per candidate: the lane at the first key of a run walks the run, ascending hypotheses.  cpos: the scan of the flags (the number of the
// candidate at its lowest staying hypothesis).  cand[k]: N, c, u, v, rep, first_hyp, n_hyp; ok[k]: its sums and its frame are usable
__global__ __launch_bounds__(256) void k_plane_param(const plane::Line* __restrict__ tab, const plane::Hyp* __restrict__ hyp, const plane::HypAux* __restrict__ aux,
                                                     const unsigned long long* __restrict__ key, const int* __restrict__ comp, const int* __restrict__ rep,
                                                     const int* __restrict__ cpos, int m, l3d_plane* __restrict__ cand, int* __restrict__ ok)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    const unsigned long long k0 = key[p];
    if (k0 == kPlaneNoKey) return;
    const unsigned lo = (unsigned)(k0 >> 32);
    if (p > 0 && (unsigned)(key[p - 1] >> 32) == lo) return;
    int count = 1;
    while (p + count < m && key[p + count] != kPlaneNoKey && (unsigned)(key[p + count] >> 32) == lo) ++count;
    const int r = rep[comp[lo]];
    l3d_plane o = {};
    const bool good = plane::parameters(hyp, aux, key + p, count, r, tab[hyp[r].li].d, o);
    o.rep = r; o.first_hyp = (int)lo; o.n_hyp = count; o.n_lines = 0;
    const int k = cpos[lo];
    cand[k] = o;
    ok[k] = good ? 1 : 0;
}

// this lane's (candidate, line) pair: wave w of the grid tests the 64 lines from (w % wpc) 64 on against candidate w / wpc
__device__ __forceinline__ bool plane_member(const plane::Line* __restrict__ tab, int n, const l3d_plane* __restrict__ cand, const int* __restrict__ use, int wpc,
                                             long long waves, long long& w, int& c, int& line)
{
    w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    c = 0; line = 0;
    if (w >= waves) return false;
    c = (int)(w / wpc);
    line = (int)(w % wpc) * 64 + (int)(threadIdx.x & 63);
    if (line >= n || !use[c] || !tab[line].elig) return false;
    return plane::lies_in(tab[line].P, tab[line].Q, tab[line].tol, cand[c].N, cand[c].c);
}

// wcnt[w]: the members in wave w's ballot word; nl[c] += them
__global__ __launch_bounds__(256) void k_plane_mcount(const plane::Line* __restrict__ tab, int n, const l3d_plane* __restrict__ cand, const int* __restrict__ ok, int wpc,
                                                      long long waves, int* __restrict__ wcnt, int* __restrict__ nl)
{
    long long w; int c, line;
    const bool in = plane_member(tab, n, cand, ok, wpc, waves, w, c, line);
    const int k = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0 && w < waves) { wcnt[w] = k; if (k) atomicAdd(&nl[c], k); }
}

// keep[c]: candidate c is a plane; total += its members
__global__ __launch_bounds__(256) void k_plane_keep(const int* __restrict__ ok, const int* __restrict__ nl, int ncand, int min_lines, int* __restrict__ keep,
                                                    unsigned long long* __restrict__ total)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncand) return;
    const bool k = ok[c] && nl[c] >= min_lines;
    keep[c] = k ? 1 : 0;
    if (k) atomicAdd(total, (unsigned long long)nl[c]);
}

// the ballot words of the dropped candidates count nothing
__global__ __launch_bounds__(256) void k_plane_mmask(const int* __restrict__ keep, int wpc, long long waves, int* __restrict__ wcnt)
{
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w < waves && !keep[w / wpc]) wcnt[w] = 0;
}

// the records of the kept candidates: wave w's from mpos[w] on, ascending lines
__global__ __launch_bounds__(256) void k_plane_mwrite(const plane::Line* __restrict__ tab, int n, const l3d_plane* __restrict__ cand, const int* __restrict__ keep,
                                                      const int* __restrict__ ppos, int wpc, long long waves, const int* __restrict__ mpos,
                                                      l3d_plane_member* __restrict__ rec)
{
    long long w; int c, line;
    const bool in = plane_member(tab, n, cand, keep, wpc, waves, w, c, line);
    const unsigned long long word = __ballot(in);
    if (!in) return;
    const int lane = threadIdx.x & 63;
    l3d_plane_member r; r.plane = ppos[c]; r.line = line; r.flags = 0; r.pad = 0;
    rec[(size_t)mpos[w] + __popcll(word & ((1ull << lane) - 1ull))] = r;
}

// per staying hypothesis of a plane: its two lines, where they are members, carry the SEED flag (the plane's records are ascending by line: bisection)
__global__ __launch_bounds__(256) void k_plane_seed(const plane::Hyp* __restrict__ hyp, const unsigned char* __restrict__ stay, const int* __restrict__ comp,
                                                    const int* __restrict__ low, const int* __restrict__ cpos, const int* __restrict__ keep, int wpc,
                                                    const int* __restrict__ mpos, int m, l3d_plane_member* __restrict__ rec)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= m || !stay[h]) return;
    const int c = cpos[low[comp[h]]];
    if (!keep[c]) return;
    const int r0 = mpos[(size_t)c * wpc], r1 = mpos[(size_t)(c + 1) * wpc];
    for (int e = 0; e < 2; ++e) {
        const int line = e == 0 ? hyp[h].li : hyp[h].lj;
        int a = r0, b = r1;
        while (a < b) { const int mid = a + (b - a) / 2; if (rec[mid].line < line) a = mid + 1; else b = mid; }
        if (a < r1 && rec[a].line == line) atomicOr(&rec[a].flags, plane::kSeed);
    }
}

// one lane per candidate that is a plane: the extent over its records, in their order; the plane's record
__global__ __launch_bounds__(256) void k_plane_extent(const plane::Line* __restrict__ tab, const l3d_plane* __restrict__ cand, const int* __restrict__ nl,
                                                      const int* __restrict__ keep, const int* __restrict__ ppos, int wpc, const int* __restrict__ mpos, int ncand,
                                                      const l3d_plane_member* __restrict__ rec, l3d_plane* __restrict__ planes)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncand || !keep[c]) return;
    l3d_plane o = cand[c];
    const int r0 = mpos[(size_t)c * wpc], r1 = mpos[(size_t)(c + 1) * wpc];
    for (int k = r0; k < r1; ++k) {
        const int line = rec[k].line;
        plane::extend(o, tab[line].P, k == r0, o.rect);
        plane::extend(o, tab[line].Q, false, o.rect);
    }
    o.n_lines = nl[c];
    planes[ppos[c]] = o;
}

// hyp_plane
__global__ __launch_bounds__(256) void k_plane_finish(const unsigned char* __restrict__ stay, const int* __restrict__ comp, const int* __restrict__ low,
                                                      const int* __restrict__ cpos, const int* __restrict__ keep, const int* __restrict__ ppos, int m,
                                                      int* __restrict__ hyp_plane)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= m) return;
    int p = -1;
    if (stay[h]) { const int c = cpos[low[comp[h]]]; if (keep[c]) p = ppos[c]; }
    hyp_plane[h] = p;
}

}  // namespace l3d

namespace {

thread_local std::string t_plane_err;

// a list as a callee-allocated array (one spare element: an empty list still hands out a pointer that l3d_free takes)
template <typename T>
T* plane_pack(const T* src, size_t count)
{
    T* o = static_cast<T*>(malloc((count + 1) * sizeof(T)));
    if (o && count) memcpy(o, src, count * sizeof(T));
    return o;
}

template <typename T>
bool guard_intact(const T* behind)
{
    const unsigned char* g = reinterpret_cast<const unsigned char*>(behind);
    for (size_t k = 0; k < kPlaneSlack * sizeof(T); ++k) if (g[k] != 0xFF) return false;
    return true;
}

int plane_hand_out(const std::vector<l3d_plane>& pl, size_t np, const std::vector<l3d_plane_member>& mem, size_t nm, l3d_plane** planes, int* n_planes,
                   l3d_plane_member** members, int* n_members)
{
    *planes = plane_pack(pl.data(), np);
    *members = plane_pack(mem.data(), nm);
    if (!*planes || !*members) { free(*planes); free(*members); *planes = nullptr; *members = nullptr; return L3D_ERR_NOMEM; }
    *n_planes = (int)np;
    *n_members = (int)nm;
    return L3D_OK;
}

int plane_run(l3d_ctx* c, const double* lines, const double* tol, int n, const int32_t* seeds, int m, const l3d_plane_params* prm, l3d_plane** planes, int* n_planes,
              l3d_plane_member** members, int* n_members, int32_t* hyp_plane, int32_t* counts)
{
    if (!c) return L3D_ERR_INVALID;
    std::string msg;
    if (int rc = plane::check_arguments(lines, tol, n, seeds, m, prm, planes, n_planes, members, n_members, hyp_plane, counts, msg)) return fail(c, rc, msg);
    std::vector<l3d_plane> h_planes;
    std::vector<l3d_plane_member> h_mem;
    if (n == 0 || m == 0) {
        for (int h = 0; h < m; ++h) hyp_plane[h] = -1;
        if (plane_hand_out(h_planes, 0, h_mem, 0, planes, n_planes, members, n_members)) return fail(c, L3D_ERR_NOMEM, "malloc");
        return L3D_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const double cos_max = prm->cos_max, cos_min = prm->cos_min;
    const int min_lines = prm->min_lines;
    const size_t N = (size_t)n, M = (size_t)m;
    const size_t C = (size_t)plane::chunks(m);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t sort_bytes = 0;
    HIPCHK(c, sort_keys_u64(nullptr, sort_bytes, nullptr, nullptr, m, 0, 64, st));
    // the tables, the per-hypothesis and the per-candidate arrays (plane_tab)
    const size_t o_lines = 0, o_tol = o_lines + al(N * 48), o_seeds = o_tol + al(N * 8), o_tab = o_seeds + al(M * 8), o_hyp = o_tab + al(N * 96), o_aux = o_hyp + al(M * 160),
                 o_total = o_aux + al(M * 32), o_cnt = o_total + 256, o_pos = o_cnt + al(M * C * 4), o_comp = o_pos + al((M * C + 1) * 4), o_changed = o_comp + al(M * 4),
                 o_maxa = o_changed + 256, o_rep = o_maxa + al(M * 8), o_low = o_rep + al(M * 4), o_flag = o_low + al(M * 4), o_cpos = o_flag + al(M * 4),
                 o_key = o_cpos + al((M + 1) * 4), o_key2 = o_key + al(M * 8), o_stay = o_key2 + al(M * 8), o_cand = o_stay + al(M), o_ok = o_cand + al(M * 128),
                 o_nl = o_ok + al(M * 4), o_keep = o_nl + al(M * 4), o_ppos = o_keep + al(M * 4), o_hp = o_ppos + al((M + 1) * 4), o_sort = o_hp + al(M * 4),
                 o_end = o_sort + al(sort_bytes);
    if (c->plane_tab.reserve(o_end) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, L3D_ERR_UNSUPPORTED, "plane lines: the tables of " + std::to_string(n) + " lines and " + std::to_string(m) + " seeds cannot be allocated on the device");
    }
    char* b = c->plane_tab.as<char>();
    double* d_lines = reinterpret_cast<double*>(b + o_lines);
    double* d_tol = reinterpret_cast<double*>(b + o_tol);
    int* d_seeds = reinterpret_cast<int*>(b + o_seeds);
    plane::Line* d_tab = reinterpret_cast<plane::Line*>(b + o_tab);
    plane::Hyp* d_hyp = reinterpret_cast<plane::Hyp*>(b + o_hyp);
    plane::HypAux* d_aux = reinterpret_cast<plane::HypAux*>(b + o_aux);
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(b + o_total);      // [0]: the edges, [1]: the member records; the counters behind them
    int* d_counts = reinterpret_cast<int*>(b + o_total + 64);
    int* d_cnt = reinterpret_cast<int*>(b + o_cnt);
    int* d_pos = reinterpret_cast<int*>(b + o_pos);
    int* d_comp = reinterpret_cast<int*>(b + o_comp);
    int* d_changed = reinterpret_cast<int*>(b + o_changed);
    unsigned long long* d_maxa = reinterpret_cast<unsigned long long*>(b + o_maxa);
    int* d_rep = reinterpret_cast<int*>(b + o_rep);
    int* d_low = reinterpret_cast<int*>(b + o_low);
    int* d_flag = reinterpret_cast<int*>(b + o_flag);
    int* d_cpos = reinterpret_cast<int*>(b + o_cpos);
    unsigned long long* d_key = reinterpret_cast<unsigned long long*>(b + o_key);
    unsigned long long* d_key2 = reinterpret_cast<unsigned long long*>(b + o_key2);
    unsigned char* d_stay = reinterpret_cast<unsigned char*>(b + o_stay);
    l3d_plane* d_cand = reinterpret_cast<l3d_plane*>(b + o_cand);
    int* d_ok = reinterpret_cast<int*>(b + o_ok);
    int* d_nl = reinterpret_cast<int*>(b + o_nl);
    int* d_keep = reinterpret_cast<int*>(b + o_keep);
    int* d_ppos = reinterpret_cast<int*>(b + o_ppos);
    int* d_hp = reinterpret_cast<int*>(b + o_hp);
    void* d_sort = b + o_sort;
    HIPCHK(c, hipMemcpyAsync(d_lines, lines, N * 48, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_tol, tol, N * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_seeds, seeds, M * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_total, 0, 256, st));
    const dim3 lgrid((unsigned)((n + 255) / 256)), hgrid((unsigned)((m + 255) / 256)), block(256);
    { ProfScope ps(c, "plane_prepare", st); hipLaunchKernelGGL(k_plane_prepare, lgrid, block, 0, st, d_lines, d_tol, n, d_tab, d_counts); }
    { ProfScope ps(c, "plane_hyp", st); hipLaunchKernelGGL(k_plane_hyp, hgrid, block, 0, st, d_tab, n, d_seeds, m, cos_max, d_hyp, d_aux, d_counts); }
    // ---- the hypothesis search: count, scan, write
    const dim3 sgrid(hgrid.x, (unsigned)C);
    { ProfScope ps(c, "plane_count", st); hipLaunchKernelGGL(k_plane_count, sgrid, block, 0, st, d_hyp, m, cos_min, d_cnt, d_total); }
    { ProfScope ps(c, "plane_scan", st); hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(kScanThreads), 0, st, d_cnt, d_pos, (int)(M * C)); }
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (total > (unsigned long long)plane::kMaxRecords) return fail(c, L3D_ERR_UNSUPPORTED, "plane lines: " + std::to_string(total) + " edges, more than 2^31 - 1");
    const size_t ne = (size_t)total;
    { ProfScope ps(c, "plane_cc_init", st); hipLaunchKernelGGL(k_cc_init, hgrid, block, 0, st, d_comp, m); }
    if (ne) {
        if (c->plane_rec.reserve((ne + kPlaneSlack) * sizeof(l3d_edge)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, L3D_ERR_UNSUPPORTED, "plane lines: the list of " + std::to_string(total) + " edges cannot be allocated on the device");
        }
        l3d_edge* d_E = c->plane_rec.as<l3d_edge>();
        HIPCHK(c, hipMemsetAsync(d_E + ne, 0xFF, kPlaneSlack * sizeof(l3d_edge), st));
        { ProfScope ps(c, "plane_write", st); hipLaunchKernelGGL(k_plane_write, sgrid, block, 0, st, d_hyp, m, cos_min, d_pos, d_E); }
        // ---- the components of the hypotheses: a few hooking rounds per look at the flag
        const dim3 egrid((unsigned)((ne + 255) / 256));
        for (int round = 0;; ++round) {
            if (round == 64) return fail(c, L3D_ERR_HIP, "plane lines: the components did not converge");
            HIPCHK(c, hipMemsetAsync(d_changed, 0, 8, st));
            for (int r = 0; r < 3; ++r) {
                { ProfScope ps(c, "plane_cc_hook", st); hipLaunchKernelGGL(k_cc_hook, egrid, block, 0, st, d_E, (int)ne, d_comp, d_changed + (r == 2 ? 0 : 1)); }
                { ProfScope ps(c, "plane_cc_compress", st); hipLaunchKernelGGL(k_cc_compress, hgrid, block, 0, st, d_comp, m); }
            }
            int h_changed = 0;
            HIPCHK(c, hipMemcpyAsync(&h_changed, d_changed, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (!h_changed) break;
        }
        l3d_edge h_guard[kPlaneSlack];
        HIPCHK(c, hipMemcpy(h_guard, d_E + ne, sizeof(h_guard), hipMemcpyDeviceToHost));
        if (!guard_intact(h_guard)) return fail(c, L3D_ERR_HIP, "plane lines: the write pass wrote beyond the edges it had counted");
    }
    // ---- representatives, the star rule, the candidates in order, their parameters
    HIPCHK(c, hipMemsetAsync(d_maxa, 0, M * 8, st));
    HIPCHK(c, hipMemsetAsync(d_rep, 0x7F, M * 4, st));
    HIPCHK(c, hipMemsetAsync(d_low, 0x7F, M * 4, st));
    { ProfScope ps(c, "plane_rep", st); hipLaunchKernelGGL(k_plane_rep, hgrid, block, 0, st, d_hyp, d_aux, d_comp, m, d_maxa, d_rep, 0); }
    { ProfScope ps(c, "plane_rep", st); hipLaunchKernelGGL(k_plane_rep, hgrid, block, 0, st, d_hyp, d_aux, d_comp, m, d_maxa, d_rep, 1); }
    { ProfScope ps(c, "plane_star", st); hipLaunchKernelGGL(k_plane_star, hgrid, block, 0, st, d_hyp, d_comp, d_rep, m, cos_min, d_stay, d_low, d_counts); }
    { ProfScope ps(c, "plane_flag", st); hipLaunchKernelGGL(k_plane_flag, hgrid, block, 0, st, d_comp, d_stay, d_low, m, d_flag); }
    { ProfScope ps(c, "plane_cscan", st); hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(kScanThreads), 0, st, d_flag, d_cpos, m); }
    { ProfScope ps(c, "plane_keys", st); hipLaunchKernelGGL(k_plane_keys, hgrid, block, 0, st, d_comp, d_stay, d_low, m, d_key); }
    { ProfScope ps(c, "plane_sort", st); HIPCHK(c, sort_keys_u64(d_sort, sort_bytes, d_key, d_key2, m, 0, 64, st)); }
    { ProfScope ps(c, "plane_param", st); hipLaunchKernelGGL(k_plane_param, hgrid, block, 0, st, d_tab, d_hyp, d_aux, d_key2, d_comp, d_rep, d_cpos, m, d_cand, d_ok); }
    int ncand = 0;
    HIPCHK(c, hipMemcpyAsync(&ncand, d_cpos + M, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (ncand < 0 || (size_t)ncand > M) return fail(c, L3D_ERR_HIP, "plane lines: the number of candidates is out of range");
    int np = 0;
    size_t nm = 0;
    if (ncand) {
        // ---- membership: every (candidate, line) pair; count, keep, mask, scan, write
        const int wpc = (n + 63) / 64;
        const long long waves = (long long)ncand * wpc;
        if (waves > kPlaneMaxWaves)
            return fail(c, L3D_ERR_UNSUPPORTED, "plane lines: " + std::to_string(ncand) + " candidates x " + std::to_string(n) + " lines, more than 2^30 wave words");
        const size_t Wt = (size_t)waves;
        if (c->plane_waves.reserve(al(Wt * 4) + al((Wt + 1) * 4)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, L3D_ERR_UNSUPPORTED, "plane lines: the membership words of " + std::to_string(ncand) + " candidates cannot be allocated on the device");
        }
        int* d_wcnt = c->plane_waves.as<int>();
        int* d_mpos = reinterpret_cast<int*>(c->plane_waves.as<char>() + al(Wt * 4));
        const dim3 mgrid((unsigned)((Wt + 3) / 4)), wgrid((unsigned)((Wt + 255) / 256)), cgrid((unsigned)((ncand + 255) / 256));
        HIPCHK(c, hipMemsetAsync(d_nl, 0, (size_t)ncand * 4, st));
        { ProfScope ps(c, "plane_mcount", st); hipLaunchKernelGGL(k_plane_mcount, mgrid, block, 0, st, d_tab, n, d_cand, d_ok, wpc, waves, d_wcnt, d_nl); }
        { ProfScope ps(c, "plane_keep", st); hipLaunchKernelGGL(k_plane_keep, cgrid, block, 0, st, d_ok, d_nl, ncand, min_lines, d_keep, d_total + 1); }
        { ProfScope ps(c, "plane_pscan", st); hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(kScanThreads), 0, st, d_keep, d_ppos, ncand); }
        { ProfScope ps(c, "plane_mmask", st); hipLaunchKernelGGL(k_plane_mmask, wgrid, block, 0, st, d_keep, wpc, waves, d_wcnt); }
        { ProfScope ps(c, "plane_mscan", st); hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(kScanThreads), 0, st, d_wcnt, d_mpos, (int)Wt); }
        unsigned long long mtotal = 0;
        HIPCHK(c, hipMemcpyAsync(&mtotal, d_total + 1, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&np, d_ppos + ncand, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        if (mtotal > (unsigned long long)plane::kMaxRecords)
            return fail(c, L3D_ERR_UNSUPPORTED, "plane lines: " + std::to_string(mtotal) + " member records, more than 2^31 - 1");
        if (np < 0 || np > ncand) return fail(c, L3D_ERR_HIP, "plane lines: the number of planes is out of range");
        nm = (size_t)mtotal;
        if (np) {
            // (the edges are done with: their buffer takes the member records and the planes)
            const size_t o_planes = al((nm + kPlaneSlack) * sizeof(l3d_plane_member));
            if (c->plane_rec.reserve(o_planes + (size_t)np * sizeof(l3d_plane)) != hipSuccess) {
                (void)hipGetLastError();
                return fail(c, L3D_ERR_UNSUPPORTED, "plane lines: the list of " + std::to_string(mtotal) + " member records cannot be allocated on the device");
            }
            l3d_plane_member* d_mem = c->plane_rec.as<l3d_plane_member>();
            l3d_plane* d_planes = reinterpret_cast<l3d_plane*>(c->plane_rec.as<char>() + o_planes);
            HIPCHK(c, hipMemsetAsync(d_mem + nm, 0xFF, kPlaneSlack * sizeof(l3d_plane_member), st));
            { ProfScope ps(c, "plane_mwrite", st); hipLaunchKernelGGL(k_plane_mwrite, mgrid, block, 0, st, d_tab, n, d_cand, d_keep, d_ppos, wpc, waves, d_mpos, d_mem); }
            { ProfScope ps(c, "plane_seed", st); hipLaunchKernelGGL(k_plane_seed, hgrid, block, 0, st, d_hyp, d_stay, d_comp, d_low, d_cpos, d_keep, wpc, d_mpos, m, d_mem); }
            { ProfScope ps(c, "plane_extent", st); hipLaunchKernelGGL(k_plane_extent, cgrid, block, 0, st, d_tab, d_cand, d_nl, d_keep, d_ppos, wpc, d_mpos, ncand, d_mem, d_planes); }
            { ProfScope ps(c, "plane_finish", st); hipLaunchKernelGGL(k_plane_finish, hgrid, block, 0, st, d_stay, d_comp, d_low, d_cpos, d_keep, d_ppos, m, d_hp); }
            h_planes.resize((size_t)np);
            h_mem.resize(nm + kPlaneSlack);
            HIPCHK(c, hipMemcpyAsync(h_planes.data(), d_planes, (size_t)np * sizeof(l3d_plane), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(h_mem.data(), d_mem, (nm + kPlaneSlack) * sizeof(l3d_plane_member), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(hyp_plane, d_hp, M * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            if (!guard_intact(h_mem.data() + nm)) return fail(c, L3D_ERR_HIP, "plane lines: the write pass wrote beyond the member records it had counted");
        }
    }
    if (!np) { nm = 0; for (int h = 0; h < m; ++h) hyp_plane[h] = -1; }
    int h_counts[8];
    HIPCHK(c, hipMemcpy(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost));
    counts[0] = h_counts[0]; counts[1] = h_counts[1]; counts[2] = (int32_t)ne; counts[3] = ncand; counts[4] = h_counts[4]; counts[5] = ncand - np; counts[6] = np;
    counts[7] = (int32_t)nm;
    if (plane_hand_out(h_planes, (size_t)np, h_mem, nm, planes, n_planes, members, n_members)) return fail(c, L3D_ERR_NOMEM, "malloc");
    return L3D_OK;
}

}  // namespace

extern "C" const char* l3d_plane_last_error(void) { return t_plane_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_plane_lines_host(const double* lines, const double* tol, int n, const int32_t* seeds, int m, const l3d_plane_params* prm, l3d_plane** planes,
                                         int* n_planes, l3d_plane_member** members, int* n_members, int32_t* hyp_plane, int32_t* counts)
{
    std::string msg;
    if (int rc = plane::check_arguments(lines, tol, n, seeds, m, prm, planes, n_planes, members, n_members, hyp_plane, counts, msg)) { t_plane_err = msg; return rc; }
    std::vector<l3d_plane> pl;
    std::vector<l3d_plane_member> mem;
    if (const int over = plane::run_host(lines, tol, n, seeds, m, prm->cos_max, prm->cos_min, prm->min_lines, pl, mem, hyp_plane, counts)) {
        for (int k = 0; k < 8; ++k) counts[k] = 0;
        t_plane_err = over == 1 ? "plane lines: more than 2^31 - 1 edges" : "plane lines: more than 2^31 - 1 member records";
        return L3D_ERR_UNSUPPORTED;
    }
    if (plane_hand_out(pl, pl.size(), mem, mem.size(), planes, n_planes, members, n_members)) { t_plane_err = "malloc"; return L3D_ERR_NOMEM; }
    return L3D_OK;
}

extern "C" int l3d_plane_lines(l3d_ctx* c, const double* lines, const double* tol, int n, const int32_t* seeds, int m, const l3d_plane_params* prm, l3d_plane** planes,
                               int* n_planes, l3d_plane_member** members, int* n_members, int32_t* hyp_plane, int32_t* counts)
{
    const int rc = plane_run(c, lines, tol, n, seeds, m, prm, planes, n_planes, members, n_members, hyp_plane, counts);
    if (rc && c) t_plane_err = l3d_last_error(c);
    return rc;
}
