// l3d_covis.hip -- co-visibility counting on the device ("CO-VISIBILITY" in include/line3d_amd.h; the closed form and its derivation: l3d_covis.hpp).
// The observations become keys (point << vb | view index, vb the bits a view index takes) that one radix sort orders: a point's track is then a run
// of the sorted keys, its views ascending.  k_covis_runs gives every observation its run (two bounded binary searches: a run is at most n_lists long
// when no list names an id twice) and sees a repeated id as two equal neighbours.  k_covis_count / k_covis_write: one workgroup per (view, column tile)
// walks the view's observations; every track of three or more views adds 1 per member into an LDS histogram over the tile's view indices -- a lane
// walks a track of up to kCovisSerial views alone, the lanes of the wave share a longer one -- and the histogram's non-zeros are counted, then (after
// k_covis_scan) written in ascending column order.  No atomics on global memory, no V x V table; the launches are six whatever the sizes.
#include "l3d_ctx.hpp"
#include "l3d_covis.hpp"
#include "l3d_scan.hpp"
#include "l3d_sort.hpp"

#include <climits>

using namespace l3d;

namespace l3d {

typedef unsigned long long u64;

// keys[i] = point << vb | view index of observation i, vals[i] = i.  The view: the last list that starts at or before i (empty lists own nothing)
__global__ __launch_bounds__(256) void k_covis_keys(const unsigned* __restrict__ ids, const long long* __restrict__ list_start, int n_lists, int n, int vb,
                                                    u64* __restrict__ keys, unsigned* __restrict__ vals)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int lo = 0, hi = n_lists;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (list_start[mid] <= i) lo = mid; else hi = mid;
        }
        keys[i] = ((u64)ids[i] << vb) | (u64)lo;
        vals[i] = (unsigned)i;
    }
}

// sorted position j: the run of its point [start, start + len) -- searched within n_lists - 1 positions either side, which holds every run when no
// list names an id twice (otherwise *dup is set and the runs are not used; they stay inside [0, n) either way) -- filed under the observation's own
// position vals[j]; sview[j]: the view index of position j
__global__ __launch_bounds__(256) void k_covis_runs(const u64* __restrict__ keys, const unsigned* __restrict__ vals, int n, int vb, int n_lists,
                                                    int* __restrict__ run_start, int* __restrict__ run_len, unsigned* __restrict__ sview, int* __restrict__ dup)
{
    for (long long jj = (long long)blockIdx.x * 256 + threadIdx.x; jj < n; jj += (long long)gridDim.x * 256) {
        const int j = (int)jj;
        const u64 k = keys[j], p = k >> vb;
        if (j > 0 && keys[j - 1] == k) *dup = 1;
        int lo = max(0, j - (n_lists - 1)), hi = j;             // keys[hi] >> vb == p throughout
        int start = lo;
        if ((keys[lo] >> vb) != p) {
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((keys[mid] >> vb) == p) hi = mid; else lo = mid;
            }
            start = hi;
        }
        lo = j; hi = (int)min((long long)n - 1, (long long)j + (n_lists - 1));   // keys[lo] >> vb == p throughout
        int end = hi;
        if ((keys[hi] >> vb) != p) {
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((keys[mid] >> vb) == p) lo = mid; else hi = mid;
            }
            end = lo;
        }
        const unsigned i = vals[j];
        run_start[i] = start;
        run_len[i] = end - start + 1;
        sview[j] = (unsigned)(k & ((1ull << vb) - 1ull));
    }
}

// The walk of view `row` over the columns [c0, c1) of tile blockIdx.y.  WRITE false: nnz[row * n_tiles + tile] = the non-zero counts of the tile,
// and from tile 0 num_wps[row] = the view's observations in tracks of three or more views.  WRITE true: those counts and their columns at
// pos[row * n_tiles + tile] ..., ascending
template <bool WRITE>
__global__ __launch_bounds__(256) void k_covis_walk(const long long* __restrict__ list_start, const int* __restrict__ run_start, const int* __restrict__ run_len,
                                                    const unsigned* __restrict__ sview, int n_lists, int tile, int n_tiles, unsigned* __restrict__ num_wps,
                                                    int* __restrict__ nnz, const int* __restrict__ pos, int* __restrict__ col, unsigned* __restrict__ count)
{
    __shared__ unsigned s_hist[kCovisTileMax];
    __shared__ int s_w[8];
    const int row = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = t * tile, c1 = min(n_lists, c0 + tile), w = c1 - c0;
    for (int c = tid; c < w; c += 256) s_hist[c] = 0u;
    __syncthreads();
    const long long b = list_start[row], e = list_start[row + 1];
    auto add = [&](unsigned c) { if ((int)c >= c0 && (int)c < c1 && (int)c != row) atomicAdd(&s_hist[(int)c - c0], 1u); };
    int mine = 0;
    for (long long base = b + wave * 64; base < e; base += 256) {        // (uniform across the wave)
        const long long i = base + lane;
        int s = 0, l = 0;
        if (i < e) { l = run_len[i]; s = run_start[i]; }
        if (l < 3) l = 0;
        mine += l > 0 ? 1 : 0;
        if (l > 0 && l <= kCovisSerial)
            for (int k = 0; k < l; ++k) add(sview[s + k]);
        u64 m = __ballot(l > kCovisSerial ? 1 : 0);
        while (m) {                                                      // a long track: its members over the lanes
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int ss = __shfl(s, src), ll = __shfl(l, src);
            for (int k = lane; k < ll; k += 64) add(sview[ss + k]);
        }
    }
    __syncthreads();
    if (!WRITE) {
        int nz = 0;
        for (int c = tid; c < w; c += 256) nz += s_hist[c] != 0u ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) { nz += __shfl_down(nz, o); mine += __shfl_down(mine, o); }
        if (lane == 0) { s_w[wave] = nz; s_w[4 + wave] = mine; }
        __syncthreads();
        if (tid == 0) {
            nnz[(long long)row * n_tiles + t] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
            if (t == 0) num_wps[row] = (unsigned)(s_w[4] + s_w[5] + s_w[6] + s_w[7]);
        }
    } else {
        int at = pos[(long long)row * n_tiles + t];
        for (int cb = 0; cb < w; cb += 256) {
            const int c = cb + tid;
            const unsigned v = c < w ? s_hist[c] : 0u;
            const u64 bal = __ballot(v != 0u ? 1 : 0);
            if (lane == 0) s_w[wave] = __popcll(bal);
            __syncthreads();
            int off = __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
            for (int q = 0; q < 4; ++q) { const int x = s_w[q]; tot += x; if (q < wave) off += x; }
            if (v != 0u) { col[at + off] = c0 + c; count[at + off] = v; }
            at += tot;
            __syncthreads();                                             // s_w is rewritten by the next chunk
        }
    }
}

// pos[0..n]: the exclusive prefix sums of cnt; total64: the total without the int's limit
__global__ __launch_bounds__(kScanThreads) void k_covis_scan(const int* __restrict__ cnt, int* __restrict__ pos, int n, long long* __restrict__ total64)
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

}  // namespace l3d

namespace {

thread_local std::string t_covis_err;

int covis_validate(const uint32_t* ids, const int64_t* list_start, int n_lists, uint32_t** num_wps, int32_t** row_start, int32_t** col, uint32_t** count, int* path,
                   std::string& msg)
{
    if (!num_wps || !row_start || !col || !count || !path || !list_start || n_lists < 0) { msg = "covisibility: bad argument"; return L3D_ERR_INVALID; }
    *num_wps = nullptr; *row_start = nullptr; *col = nullptr; *count = nullptr; *path = 0;
    if (n_lists >= INT_MAX) { msg = "covisibility: 2^31 - 1 views or more"; return L3D_ERR_UNSUPPORTED; }
    if (list_start[0] != 0) { msg = "covisibility: list_start[0] is not 0"; return L3D_ERR_INVALID; }
    for (int i = 0; i < n_lists; ++i)
        if (list_start[i + 1] < list_start[i]) { msg = "covisibility: list_start descends"; return L3D_ERR_INVALID; }
    if (list_start[n_lists] >= (int64_t)INT_MAX) { msg = "covisibility: 2^31 - 1 observations or more"; return L3D_ERR_UNSUPPORTED; }
    if (list_start[n_lists] > 0 && !ids) { msg = "covisibility: point_ids is null"; return L3D_ERR_INVALID; }
    return L3D_OK;
}

// the outputs as callee-allocated arrays (one spare element each: an empty result still hands out pointers that l3d_free takes)
int covis_pack(const uint32_t* num, const int32_t* rs, const int32_t* cl, const uint32_t* cn, int n_lists, size_t nnz, uint32_t** num_wps, int32_t** row_start,
               int32_t** col, uint32_t** count)
{
    uint32_t* a = static_cast<uint32_t*>(malloc(((size_t)n_lists + 1) * 4));
    int32_t* b = static_cast<int32_t*>(malloc(((size_t)n_lists + 2) * 4));
    int32_t* c = static_cast<int32_t*>(malloc((nnz + 1) * 4));
    uint32_t* d = static_cast<uint32_t*>(malloc((nnz + 1) * 4));
    if (!a || !b || !c || !d) { free(a); free(b); free(c); free(d); return L3D_ERR_NOMEM; }
    if (n_lists) memcpy(a, num, (size_t)n_lists * 4);
    memcpy(b, rs, ((size_t)n_lists + 1) * 4);
    if (nnz) { memcpy(c, cl, nnz * 4); memcpy(d, cn, nnz * 4); }
    *num_wps = a; *row_start = b; *col = c; *count = d;
    return L3D_OK;
}

// the lists through Line3D::processWorldpointList itself, in add order, on tables of its own; the view ids are the list indices
int covis_replay(const uint32_t* ids, const int64_t* list_start, int n_lists, uint32_t** num_wps, int32_t** row_start, int32_t** col, uint32_t** count, std::string& msg)
{
    std::vector<uint32_t> num, cn;
    std::vector<int32_t> rs, cl;
    if (!replay_csr(ids, list_start, n_lists, num, rs, cl, cn)) { msg = "covisibility: more than 2^31 - 1 non-zero counts"; return L3D_ERR_UNSUPPORTED; }
    const int rp = covis_pack(num.data(), rs.data(), cl.data(), cn.data(), n_lists, cl.size(), num_wps, row_start, col, count);
    if (rp) msg = "malloc";
    return rp;
}

// the device memory of one call: released when the call returns, whichever way
struct CovisScratch {
    DevBuf ids, ls, keys_a, keys_b, vals_a, vals_b, tmp, small, nnz, pos, out;
    ~CovisScratch()
    {
        DevBuf* b[] = { &ids, &ls, &keys_a, &keys_b, &vals_a, &vals_b, &tmp, &small, &nnz, &pos, &out };
        for (DevBuf* x : b) x->release();
    }
};

int covis_device(l3d_ctx* c, const uint32_t* ids, const int64_t* list_start, int n_lists, uint32_t** num_wps, int32_t** row_start, int32_t** col, uint32_t** count, int* path)
{
    const int n = (int)list_start[n_lists];
    if (n == 0) {                           // no observation: nothing to count (and nothing to launch)
        std::vector<uint32_t> num((size_t)n_lists + 1, 0);
        std::vector<int32_t> rs((size_t)n_lists + 1, 0);
        const int rp = covis_pack(num.data(), rs.data(), nullptr, nullptr, n_lists, 0, num_wps, row_start, col, count);
        return rp ? fail(c, rp, "malloc") : L3D_OK;
    }
    int tile = c->opt.covis_tile > 0 ? std::min(c->opt.covis_tile, kCovisTileMax) : kCovisTileMax;
    tile = std::min(tile, n_lists);
    const long long n_tiles_ll = ((long long)n_lists + tile - 1) / tile;
    if (n_tiles_ll > 65535 || (long long)n_lists * n_tiles_ll >= (long long)INT_MAX)
        return fail(c, L3D_ERR_UNSUPPORTED, "covisibility: too many column tiles (option covis_tile is too small for this many views)");
    const int n_tiles = (int)n_tiles_ll, n_cells = n_lists * n_tiles;
    int vb = 1;
    while ((1ll << vb) < (long long)n_lists) ++vb;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    CovisScratch S;
    HIPCHK(c, S.ids.reserve_exact((size_t)n * 4));
    HIPCHK(c, S.ls.reserve_exact(((size_t)n_lists + 1) * 8));
    HIPCHK(c, S.keys_a.reserve_exact((size_t)n * 8));
    HIPCHK(c, S.keys_b.reserve_exact((size_t)n * 8));
    HIPCHK(c, S.vals_a.reserve_exact((size_t)n * 4));
    HIPCHK(c, S.vals_b.reserve_exact((size_t)n * 4));
    size_t tmp_bytes = 0;
    HIPCHK(c, sort_pairs_u64_u32(nullptr, tmp_bytes, S.keys_a.as<u64>(), S.keys_b.as<u64>(), S.vals_a.as<unsigned>(), S.vals_b.as<unsigned>(), n, 0, 32 + vb, st));
    HIPCHK(c, S.tmp.reserve_exact(tmp_bytes ? tmp_bytes : 16));
    HIPCHK(c, S.small.reserve_exact(16 + (size_t)n_lists * 4));         // dup flag | total | num_wps
    HIPCHK(c, S.nnz.reserve_exact((size_t)n_cells * 4));
    HIPCHK(c, S.pos.reserve_exact(((size_t)n_cells + 1) * 4));
    int* d_dup = S.small.as<int>();
    long long* d_total = reinterpret_cast<long long*>(S.small.as<char>() + 8);
    unsigned* d_num = reinterpret_cast<unsigned*>(S.small.as<char>() + 16);
    HIPCHK(c, hipMemsetAsync(S.small.p, 0, 16, st));
    HIPCHK(c, hipMemcpyAsync(S.ids.p, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S.ls.p, list_start, ((size_t)n_lists + 1) * 8, hipMemcpyHostToDevice, st));
    const long long* d_ls = S.ls.as<long long>();
    const unsigned blocks = (unsigned)std::min<long long>(((long long)n + 255) / 256, 16384);
    { ProfScope ps(c, "covis_keys", st); hipLaunchKernelGGL(k_covis_keys, dim3(blocks), dim3(256), 0, st, S.ids.as<unsigned>(), d_ls, n_lists, n, vb, S.keys_a.as<u64>(), S.vals_a.as<unsigned>()); }
    {
        ProfScope ps(c, "covis_sort", st);
        HIPCHK(c, sort_pairs_u64_u32(S.tmp.p, tmp_bytes, S.keys_a.as<u64>(), S.keys_b.as<u64>(), S.vals_a.as<unsigned>(), S.vals_b.as<unsigned>(), n, 0, 32 + vb, st));
    }
    // behind the sort its inputs are free: the runs take the place of keys_a (start | length), the sorted view indices that of vals_a
    int* d_rstart = S.keys_a.as<int>();
    int* d_rlen = d_rstart + n;
    unsigned* d_sview = S.vals_a.as<unsigned>();
    { ProfScope ps(c, "covis_runs", st); hipLaunchKernelGGL(k_covis_runs, dim3(blocks), dim3(256), 0, st, S.keys_b.as<u64>(), S.vals_b.as<unsigned>(), n, vb, n_lists, d_rstart, d_rlen, d_sview, d_dup); }
    const dim3 grid((unsigned)n_lists, (unsigned)n_tiles);
    { ProfScope ps(c, "covis_count", st); hipLaunchKernelGGL(k_covis_walk<false>, grid, dim3(256), 0, st, d_ls, d_rstart, d_rlen, d_sview, n_lists, tile, n_tiles, d_num, S.nnz.as<int>(), (const int*)nullptr, (int*)nullptr, (unsigned*)nullptr); }
    { ProfScope ps(c, "covis_scan", st); hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(kScanThreads), 0, st, S.nnz.as<int>(), S.pos.as<int>(), n_cells, d_total); }
    int dup = 0;
    long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&dup, d_dup, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (dup) { *path = 1; return L3D_OK; }          // (the caller replays)
    if (total < 0 || total > (long long)INT_MAX) return fail(c, L3D_ERR_UNSUPPORTED, "covisibility: more than 2^31 - 1 non-zero counts");
    const size_t o_cnt = (((size_t)total * 4) + 255) & ~(size_t)255;
    HIPCHK(c, S.out.reserve_exact(o_cnt + (size_t)total * 4 + 16));
    int* d_col = S.out.as<int>();
    unsigned* d_count = reinterpret_cast<unsigned*>(S.out.as<char>() + o_cnt);
    { ProfScope ps(c, "covis_write", st); hipLaunchKernelGGL(k_covis_walk<true>, grid, dim3(256), 0, st, d_ls, d_rstart, d_rlen, d_sview, n_lists, tile, n_tiles, (unsigned*)nullptr, (int*)nullptr, (const int*)S.pos.as<int>(), d_col, d_count); }
    std::vector<uint32_t> h_num((size_t)n_lists), h_cnt((size_t)total + 1);
    std::vector<int32_t> h_pos((size_t)n_cells + 1), h_col((size_t)total + 1), h_rs((size_t)n_lists + 1);
    HIPCHK(c, hipMemcpyAsync(h_num.data(), d_num, (size_t)n_lists * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_pos.data(), S.pos.p, ((size_t)n_cells + 1) * 4, hipMemcpyDeviceToHost, st));
    if (total) {
        HIPCHK(c, hipMemcpyAsync(h_col.data(), d_col, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(h_cnt.data(), d_count, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (int r = 0; r <= n_lists; ++r) h_rs[(size_t)r] = h_pos[(size_t)r * n_tiles];
    const int rp = covis_pack(h_num.data(), h_rs.data(), h_col.data(), h_cnt.data(), n_lists, (size_t)total, num_wps, row_start, col, count);
    return rp ? fail(c, rp, "malloc") : L3D_OK;
}

}  // namespace

extern "C" const char* l3d_covis_last_error(void) { return t_covis_err.c_str(); }

extern "C" int l3d_test_covisibility_host(const uint32_t* point_ids, const int64_t* list_start, int n_lists, uint32_t** num_wps, int32_t** row_start, int32_t** col,
                                          uint32_t** count, int* path)
{
    std::string msg;
    int rc = covis_validate(point_ids, list_start, n_lists, num_wps, row_start, col, count, path, msg);
    if (!rc) { *path = 1; rc = covis_replay(point_ids, list_start, n_lists, num_wps, row_start, col, count, msg); }
    if (rc) t_covis_err = msg;
    return rc;
}

extern "C" int l3d_covisibility(l3d_ctx* c, const uint32_t* point_ids, const int64_t* list_start, int n_lists, uint32_t** num_wps, int32_t** row_start, int32_t** col,
                                uint32_t** count, int* path)
{
    if (!c) return L3D_ERR_INVALID;
    std::string msg;
    if (int rc = covis_validate(point_ids, list_start, n_lists, num_wps, row_start, col, count, path, msg)) return fail(c, rc, msg);
    if (int rc = covis_device(c, point_ids, list_start, n_lists, num_wps, row_start, col, count, path)) return rc;
    if (*path == 0) return L3D_OK;
    const int rc = covis_replay(point_ids, list_start, n_lists, num_wps, row_start, col, count, msg);
    return rc ? fail(c, rc, msg) : L3D_OK;
}
