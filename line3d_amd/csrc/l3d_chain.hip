// l3d_chain.hip -- Line3D::matchViews (line3D.cc:620-648) as ONE device-resident chain.
//
// The reference processes views strictly one after the other and crosses the host<->device boundary several
// times per view (uploads, a dense download per neighbour, host sort, download of confidences, and the
// verified matches of a view travel through the host -- a file! -- to become candidates of later views,
// line3D.cc:838-872, view.cc:162-224).  Here the whole schedule is static: which neighbours a view still has to
// match (toBeMatched) and which earlier views feed it with reverse matches depends only on the neighbour graph
// and the processing order, not on data.  So the host enqueues everything without ever waiting:
//
//   phase 1  stage 1 (pair test -> bit rows -> row counts) of ALL views: independent, back to back
//   phase 2  per view, in order: reverse matches are pulled on the device out of the kept lists of the earlier
//            views (they never leave HBM), prefix sums, depth records, verification, per-segment best/filter,
//            ordered compaction of the kept matches into one arena
//
// and only trails behind the GPU to hand each view's kept list to the caller's bookkeeping (a callback), which
// overlaps with the GPU working on later views.  Results are identical to the per-view entry point
// (l3d_compute_pairwise_matches): same kernels, same candidate order.
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "l3d_ctx.hpp"
#include "l3d_scan.hpp"
#include "l3d_kept.hpp"
#include "l3d_products.hpp"
#include "l3d_chain_common.hpp"
#include "l3d_chain_partition.hpp"
#include "l3d_runtable.hpp"

#ifndef L3D_AHEAD
#define L3D_AHEAD 4
#define L3D_S1AHEAD 8
#endif

using namespace l3d;

namespace l3d {

// reverse matches for view `view_id` out of the kept lists of earlier views (blockIdx.y = source): count per
// (segment, camera) row.  (seg, tgt) swap roles and the depth pairs swap, line3D.cc:847-856.
// Short lists -- config 2 keeps 36 k matches per view, 1.2 MB -- are scanned record by record: one pass over cache-resident data beats the run tables' extra
// level of dependent loads (12.2 vs 12.9 ms per config-2 pass).  Once the views keep more than chain_long_list() records each on average (2^18; option
// long_list), the following views read their sources' runs instead (k_exist_count_rt, k_place_rt), and the chain transposes the products' pairs itself (L3D_PROD_EARLY=1).
__global__ void k_exist_count(const Match* __restrict__ arena, const ChainResult* __restrict__ res, const int* __restrict__ src_index,
                              const int* __restrict__ src_cam, unsigned view_id, int N, int S, int* __restrict__ rowcnt)
{
    const ChainResult* src = res + src_index[blockIdx.y];
    const int cam = src_cam[blockIdx.y];
    const int n = src->n_kept;
    const Match* kept = arena + src->kept_base;
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Match r = kept[i];
        if (r.camID2 == view_id && (int)r.segID2 < S) atomicAdd(&rowcnt[r.segID2 * N + cam], 1);
    }
}
// Round 6, run tables (l3d_runtable.hpp): the records of source w that point at this view are the runs rt_w[slot][s] .. rt_w[slot + 1][s] of its list
// (slot = this view's local camera number in w's neighbour list) -- read directly, through the packed side array (4 bytes per record: the target
// segment is all the count needs), instead of scanning the source's whole list for them: 1/N of it is touched, twelve sources' lists are not.
// g (a power of two) lanes share a run.
// (round 6, late) NO GLOBAL ATOMICS: 2 M scattered atomicAdds per view -- every one on its own 64-byte line, the rows being N x 4 bytes apart -- ran at
// 14 G/s whatever fed them (144 us per view at 40 x 4000 x 24, with or without the run tables).  A source's segments are cut into kExistChunks chunks; a
// workgroup per (chunk, source) counts its runs' targets in LDS and leaves its S counters in `part`; k_exist_combine sums every (source, target segment)'s
// chunk counts into the row count (and leaves the chunk bases, exclusive sums, in `part`).
static thread_local unsigned t_collect_launched = 0;      // L3D_CK_*: the kernels the launchers below started on this host thread since the last reset (one OR per launch: l3d_test_collect_candidates reports it)
constexpr int kExistChunks = 16;
constexpr int kExistThreads = 1024;         // (sixteen waves per (chunk, source): a workgroup's critical path is its runs / waves dependent load pairs)
__global__ __launch_bounds__(kExistThreads) void k_exist_count_rt(const unsigned* __restrict__ qt_arena, const RtInfo* __restrict__ info, const ChainResult* __restrict__ res,
                                                        const int* __restrict__ src_index, const int* __restrict__ src_slot, int g, int S, int* __restrict__ part)
{
    extern __shared__ int s_hist[];
    const int j = blockIdx.y, ch = blockIdx.x;
    const int si = src_index[j], slot = src_slot[j];
    const RtInfo w = info[si];
    int* out = part + ((size_t)j * kExistChunks + ch) * S;
    for (int u = threadIdx.x; u < S; u += kExistThreads) s_hist[u] = 0;
    __syncthreads();
    if (w.rt && slot >= 0 && res[si].n_kept > 0) {
        const unsigned* qt = qt_arena + res[si].kept_base;
        const int* r0 = w.rt + (size_t)slot * w.S;
        const int* r1 = r0 + w.S;
        const int s_lo = (int)(((long long)w.S * ch) / kExistChunks), s_hi = (int)(((long long)w.S * (ch + 1)) / kExistChunks);
        const int grp = threadIdx.x / g, gl = threadIdx.x - grp * g, ngrp = kExistThreads / g;
        for (int s = s_lo + grp; s < s_hi; s += ngrp) {
            const int a = r0[s], b = r1[s];
            for (int i = a + gl; i < b; i += g) { const int u = (int)(qt[i] & 0xffffu); if (u < S) atomicAdd(&s_hist[u], 1); }
        }
    }
    __syncthreads();
    for (int u = threadIdx.x; u < S; u += kExistThreads) out[u] = s_hist[u];
}
__global__ __launch_bounds__(256) void k_exist_combine(int* __restrict__ part, const int* __restrict__ src_cam, int N, int S, int* __restrict__ rowcnt)
{
    const int j = blockIdx.y, u = blockIdx.x * 256 + threadIdx.x;
    if (u >= S) return;
    int* p = part + (size_t)j * kExistChunks * S + u;
    int run = 0;
#pragma unroll
    for (int ch = 0; ch < kExistChunks; ++ch) { const int t = p[(size_t)ch * S]; p[(size_t)ch * S] = run; run += t; }
    if (run) atomicAdd(&rowcnt[u * N + src_cam[j]], run);           // (one thread per cell: the atomic only keeps the add whole beside stage 1's rows of other cameras)
}
// The scatter order inside a (segment, camera) run is arbitrary.  One wave per run restores the (segment, camera,
// target) order of the reference's list sort: every lane holds up to four entries in registers, ranks them by
// counting (keys are broadcast with shuffles, target ids inside a run are distinct) and writes them to their place.
__global__ __launch_bounds__(256) void k_exist_sort_runs(const int* __restrict__ cams, int n_cams, int N, int S, int seg_begin, int seg_end,
                                                         const int* __restrict__ row_start, uint2* __restrict__ meta,
                                                         float4* __restrict__ depths, int cap, float* stage, long long stage_stride, unsigned* stage_key)
{
    if (row_start[(size_t)S * N] > cap) return;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= (seg_end - seg_begin) * n_cams) return;
    const int seg = seg_begin + t / n_cams, cam = cams[t % n_cams];
    const int b = row_start[seg * N + cam], n = row_start[seg * N + cam + 1] - b;
    sort_exist_run(lane, b, n, cam, meta, depths, stage, stage_stride, stage_key);      // (stage: the verification's scratch + confidence slots, unused until it runs)
}

// Both writers of the combined candidate arrays in one launch (independent: stage-1 candidates go to the rows of the cameras
// to be matched, reverse matches to the rows of the source cameras): the first `blocks_move` workgroups move the stage-1 rows
// (move_stage1_row), the others scatter the reverse matches of short lists (bps workgroups per source view).
__global__ __launch_bounds__(256) void k_place(int blocks_move, int bps, const int* __restrict__ tbm, int n_tbm, const int* __restrict__ rowA,
                                               const uint2* __restrict__ metaA, const float4* __restrict__ depthsA,
                                               const Match* __restrict__ arena, const ChainResult* __restrict__ res, const int* __restrict__ src_index,
                                               const int* __restrict__ src_cam, unsigned view_id, int N, int S,
                                               const int* __restrict__ row_start, int* __restrict__ cursor,
                                               uint2* __restrict__ meta, float4* __restrict__ depths, int cap)
{
    if (row_start[(size_t)S * N] > cap) return;                  // overflow: the chain is re-run with more room
    if ((int)blockIdx.x < blocks_move) { move_stage1_row(0, S, tbm, n_tbm, N, rowA, metaA, depthsA, row_start, meta, depths); return; }
    const int e = (int)blockIdx.x - blocks_move, si = e / bps, bx = e % bps;         // bps workgroups per source view
    const ChainResult* src = res + src_index[si];
    const int cam = src_cam[si];
    const int n = src->n_kept;
    const Match* kept = arena + src->kept_base;
    for (int i = bx * 256 + (int)threadIdx.x; i < n; i += bps * 256) {
        const Match r = kept[i];
        if (r.camID2 == view_id && (int)r.segID2 < S) place_reverse_match(r, N, cam, row_start, cursor, meta, depths);
    }
}
// k_place for long lists: the stage-1 rows are moved as in k_place, the reverse matches come from the sources' runs towards this view through the
// global row cursors -- 6000 small workgroups in one launch with the move: faster than 192 (or 768) big ones with LDS cursors in a launch of their own
// (cand_move 12.0 against 17.1 / 13.2 ms at 40 x 4000 x 24, NOTEBOOK 12.f; the LDS-cursor variant is retired)
__global__ __launch_bounds__(256) void k_place_rt(int blocks_move, int bps, const int* __restrict__ tbm, int n_tbm, const int* __restrict__ rowA,
                                                  const uint2* __restrict__ metaA, const float4* __restrict__ depthsA,
                                                  const Match* __restrict__ arena, const ChainResult* __restrict__ res, const int* __restrict__ src_index,
                                                  const int* __restrict__ src_cam, int N, int S, const int* __restrict__ row_start, int* __restrict__ cursor,
                                                  uint2* __restrict__ meta, float4* __restrict__ depths, int cap,
                                                  const RtInfo* __restrict__ info, const int* __restrict__ src_slot, int g)
{
    if (row_start[(size_t)S * N] > cap) return;
    if ((int)blockIdx.x < blocks_move) { move_stage1_row(0, S, tbm, n_tbm, N, rowA, metaA, depthsA, row_start, meta, depths); return; }
    const int e = (int)blockIdx.x - blocks_move, sj = e / bps, bx = e % bps;
    const int si = src_index[sj], cam = src_cam[sj], slot = src_slot[sj];
    const RtInfo w = info[si];
    if (!w.rt || slot < 0 || res[si].n_kept == 0) return;
    const Match* kept = arena + res[si].kept_base;
    const int* r0 = w.rt + (size_t)slot * w.S;
    const int* r1 = r0 + w.S;
    const int grp = threadIdx.x / g, gl = threadIdx.x - grp * g, ngrp = 256 / g;
    for (int sg = bx * ngrp + grp; sg < w.S; sg += bps * ngrp) {
        const int a = r0[sg], b = r1[sg];
        for (int i = a + gl; i < b; i += g) {
            const Match r = kept[i];
            if ((int)r.segID2 < S) place_reverse_match(r, N, cam, row_start, cursor, meta, depths);
        }
    }
}
// Kept records of a view into its slice of the arena, in ONE launch behind the verification: each workgroup (one segment) sums
// the kept counts in front of its segment itself (kept_before_total), and the slice starts where the previous verified view's
// ended (its result record) -- no cursor, no atomics.
// Workgroup 0 also writes the view's result record (device copy for later views, host-mapped copy for the host).
__global__ __launch_bounds__(256) void k_kept_write_chain(VerifyArgs a, const int* __restrict__ kept_cnt, int nrow, const ChainResult* __restrict__ prev,
                                                          unsigned long long arena_cap, ChainResult* __restrict__ res, ChainResult* __restrict__ res_host,
                                                          const unsigned* __restrict__ local2global, Match* __restrict__ arena, int* __restrict__ best_pos, unsigned* __restrict__ cams,
                                                          int* __restrict__ rt, int rt_stride)
{
    __shared__ int s_red[8];
    __shared__ int s_cnt[32];
    __shared__ int s_qcnt[256];
    __shared__ unsigned long long s_best[4];
    const int tid = threadIdx.x;
    const int nseg = a.seg_end - a.seg_begin;
    const int yl = blockIdx.x;
    int before, total;
    kept_before_total(kept_cnt + a.seg_begin, nseg, yl, s_red, before, total);
    ChainResult r;
    r.R = a.row_start[nrow];
    r.overflow = r.R > a.cand_cap ? 1 : 0;
    r.n_kept = r.overflow ? 0 : total;
    r.n_want = 0;
    r.kept_base = prev ? prev->kept_base + (uint64_t)prev->n_kept : 0;
    if (r.kept_base + (uint64_t)r.n_kept > arena_cap) { r.overflow |= 2; r.n_want = r.n_kept; r.n_kept = 0; }     // (the regrow must hold this view too)
    if (blockIdx.x == 0 && tid == 0) { *res = r; *res_host = r; }
    if (yl >= nseg || r.overflow) return;
    write_kept_segment_wg(a, a.seg_begin + yl, before, local2global, arena + r.kept_base, s_cnt, best_pos ? best_pos + a.seg_begin + yl : nullptr, s_best, cams ? cams + r.kept_base : nullptr,
                          rt, rt_stride, s_qcnt);
}

void launch_exist_count(const Match* arena, const ChainResult* res, const int* src_index, const int* src_cam, int n_src, unsigned view_id,
                        int N, int S, int* rowcnt, hipStream_t st, int bps)
{
    if (n_src > 0) { hipLaunchKernelGGL(k_exist_count, dim3(std::max(1, bps), n_src), dim3(256), 0, st, arena, res, src_index, src_cam, view_id, N, S, rowcnt); t_collect_launched |= L3D_CK_EXIST_COUNT; }
}
void launch_exist_sort_runs(const int* cams, int n_cams, int N, int S, const int* row_start, uint2* meta, float4* depths, int cap, hipStream_t st,
                            int seg_begin, int seg_end, float* stage, long long stage_stride, unsigned* stage_key)
{
    if (seg_end < 0) seg_end = S;
    const int runs = (seg_end - seg_begin) * n_cams;
    if (runs > 0) { hipLaunchKernelGGL(k_exist_sort_runs, dim3((runs + 3) / 4), dim3(256), 0, st, cams, n_cams, N, S, seg_begin, seg_end, row_start, meta, depths, cap, stage, stage_stride, stage_key); t_collect_launched |= L3D_CK_SORT_RUNS; }
}
void launch_place(const int* tbm, int n_tbm, int N, int S, const int* rowA, const uint2* metaA, const float4* depthsA,
                  const Match* arena, const ChainResult* res, const int* src_index, const int* src_cam, int n_src, unsigned view_id,
                  const int* row_start, int* cursor, int cand_cap, uint2* meta, float4* depths, hipStream_t st, int bps,
                  const RtInfo* info, const int* src_slot, int g)
{
    bps = std::max(1, bps);
    const int blocks_move = (S * n_tbm + 3) / 4;
    const int blocks = blocks_move + bps * n_src;
    if (info) { if (blocks > 0) hipLaunchKernelGGL(k_place_rt, dim3(blocks), dim3(256), 0, st, blocks_move, bps, tbm, n_tbm, rowA, metaA, depthsA, arena, res, src_index, src_cam,
                                                         N, S, row_start, cursor, meta, depths, cand_cap, info, src_slot, std::max(1, g)); }
    else if (blocks > 0) hipLaunchKernelGGL(k_place, dim3(blocks), dim3(256), 0, st, blocks_move, bps, tbm, n_tbm, rowA, metaA, depthsA, arena, res, src_index, src_cam,
                                            view_id, N, S, row_start, cursor, meta, depths, cand_cap);
    if (blocks > 0) t_collect_launched |= info ? L3D_CK_PLACE_RT : L3D_CK_PLACE;
}
void launch_exist_count_rt(const unsigned* qt_arena, const RtInfo* info, const ChainResult* res, const int* src_index, const int* src_cam, const int* src_slot, int n_src, int g,
                           int N, int S, int* rowcnt, int* part, hipStream_t st)
{
    if (n_src <= 0 || S <= 0) return;
    hipLaunchKernelGGL(k_exist_count_rt, dim3(kExistChunks, n_src), dim3(kExistThreads), (size_t)S * 4, st, qt_arena, info, res, src_index, src_slot, std::max(1, g), S, part);
    hipLaunchKernelGGL(k_exist_combine, dim3((S + 255) / 256, n_src), dim3(256), 0, st, part, src_cam, N, S, rowcnt);
    t_collect_launched |= L3D_CK_EXIST_COUNT_RT;
}
int exist_chunks() { return kExistChunks; }
void launch_kept_write_chain(const VerifyArgs& a, const int* kept_cnt, int nrow, const ChainResult* prev, unsigned long long arena_cap, ChainResult* res,
                             ChainResult* res_host, const unsigned* l2g, Match* arena, hipStream_t st, int* best_pos, unsigned* cams, int* rt, int rt_stride)
{
    hipLaunchKernelGGL(k_kept_write_chain, dim3(std::max(1, a.seg_end - a.seg_begin)), dim3(256), 0, st, a, kept_cnt, nrow, prev, arena_cap, res, res_host, l2g, arena, best_pos, cams, rt, rt_stride);
}

}  // namespace l3d

namespace {

typedef l3d::ChainViewDev ViewDev;

// Side words and run tables of lists that did not come out of the chain's kept writer, rebuilt from their records (l3d_runtable.hpp): jobs[i] names
// the records, the outputs and the sizes, l2g[i] the list's neighbours (N global ids).  The neighbours sorted by id, their local numbers, the key
// scratch and the error counter go into ch_rtjobs behind the job array; *bad = records whose camera is no neighbour + descents of the (segment,
// camera) order, over all jobs.  Returns with the stream idle.
int rebuild_run_tables(l3d_ctx* c, std::vector<RtJob>& jobs, const std::vector<const unsigned*>& l2g, hipStream_t st, int* bad, int* max_n_out = nullptr)
{
    *bad = 0;
    if (max_n_out) *max_n_out = 0;
    if (jobs.empty()) return L3D_OK;
    std::vector<unsigned> ids;
    std::vector<int> qs;
    std::vector<size_t> at;
    for (size_t i = 0; i < jobs.size(); ++i) {
        std::vector<std::pair<unsigned, int>> byid;
        for (int q = 0; q < jobs[i].N; ++q) byid.push_back({ l2g[i][q], q });
        std::sort(byid.begin(), byid.end());
        at.push_back(ids.size());
        for (auto& e : byid) { ids.push_back(e.first); qs.push_back(e.second); }
    }
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_ids = al(jobs.size() * sizeof(RtJob)), o_qs = o_ids + al(ids.size() * 4), o_err = o_qs + al(qs.size() * 4), o_key = o_err + 256;
    size_t n_keys = 0;
    for (const RtJob& j : jobs) n_keys += (size_t)j.n;
    HIPCHK(c, c->ch_rtjobs.reserve(o_key + n_keys * 4 + 256));       // (not ch_stage: the taken-over records may live there)
    unsigned char* sb = c->ch_rtjobs.as<unsigned char>();
    int max_n = 0, max_cells = 0;
    size_t ko = 0;
    for (size_t i = 0; i < jobs.size(); ++i) {
        jobs[i].ids = reinterpret_cast<const unsigned*>(sb + o_ids) + at[i]; jobs[i].qs = reinterpret_cast<const int*>(sb + o_qs) + at[i];
        jobs[i].skey = reinterpret_cast<unsigned*>(sb + o_key) + ko; ko += (size_t)jobs[i].n;
        max_n = std::max(max_n, jobs[i].n); max_cells = std::max(max_cells, (jobs[i].N + 1) * jobs[i].S);
    }
    HIPCHK(c, hipMemcpyAsync(sb, jobs.data(), jobs.size() * sizeof(RtJob), hipMemcpyHostToDevice, st));
    if (!ids.empty()) {
        HIPCHK(c, hipMemcpyAsync(sb + o_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(sb + o_qs, qs.data(), qs.size() * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipMemsetAsync(sb + o_err, 0, 4, st));
    launch_qt_from_records(reinterpret_cast<const RtJob*>(sb), (int)jobs.size(), max_n, reinterpret_cast<int*>(sb + o_err), st);
    launch_rt_from_qt(reinterpret_cast<const RtJob*>(sb), (int)jobs.size(), max_cells, st);
    HIPCHK(c, hipMemcpyAsync(bad, sb + o_err, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (max_n_out) *max_n_out = max_n;
    return L3D_OK;
}

// One view's candidates collected on the chain's stream (run_chain per view; l3d_test_collect_candidates on crafted lists): its reverse matches counted
// out of its sources' kept lists into the row counts stage 1 left (records scanned, or the sources' runs towards this view read through their run
// tables), the combined row starts (+ zeroed scatter cursors, + the segments ordered longest first for the verification launch), stage-1 rows moved
// and reverse matches scattered in one launch, and -- unless the window kernel orders them itself -- the runs put into target order.
struct CollectIn {
    const Match* arena; const ChainResult* dres; const unsigned* cams; const RtInfo* info;
    const int *d_sc, *d_si, *d_ss, *d_tbm;          // source cameras, source views, this view's slot in each source's neighbour list, cameras to be matched (device)
    int n_sources, n_tbm; unsigned view_id; int S, N;
    int* rowcnt; const int* rowA; const uint2* metaA; const float4* depthsA;
    size_t cand_cap; bool sort_apart;
};
void enqueue_collect(l3d_ctx* c, const CollectIn& in, const CollectRule& r, hipStream_t st)
{
    const int S = in.S, N = in.N;
    if (r.rt) {
        ProfScope p(c, "exist");
        launch_exist_count_rt(in.cams, in.info, in.dres, in.d_si, in.d_sc, in.d_ss, in.n_sources, r.rt_g, N, S, in.rowcnt, c->ch_existpart.as<int>(), st);
    } else {
        ProfScope p(c, "exist");
        launch_exist_count(in.arena, in.dres, in.d_si, in.d_sc, in.n_sources, in.view_id, N, S, in.rowcnt, st, r.bps);
    }
    { ProfScope p(c, "scan"); launch_scan(in.rowcnt, c->row_start.as<int>(), S * N, c->ch_cursor.as<int>(), st, c->ch_segorder.as<int>(), N, 0, S); t_collect_launched |= L3D_CK_SCAN; }
    {
        ProfScope p(c, "cand_move");
        launch_place(in.d_tbm, in.n_tbm, N, S, in.rowA, in.metaA, in.depthsA, in.arena, in.dres, in.d_si, in.d_sc, in.n_sources, in.view_id,
                     c->row_start.as<int>(), c->ch_cursor.as<int>(), (int)in.cand_cap, c->cand_meta.as<uint2>(), c->cand_depths.as<float4>(), st, r.rt ? r.rt_bps : r.bps,
                     r.rt ? in.info : nullptr, in.d_ss, r.rt_g);
    }
    if (in.n_sources && in.sort_apart) {
        ProfScope p(c, "exist");
        launch_exist_sort_runs(in.d_sc, in.n_sources, N, S, c->row_start.as<int>(), c->cand_meta.as<uint2>(), c->cand_depths.as<float4>(), (int)in.cand_cap, st, 0, -1,
                               c->vw_scratch.as<float>(), (long long)in.cand_cap + kVWSlack, c->cand_conf.as<unsigned>());
    }
}
// the run tables' descriptors of every view of a schedule (rt[k]: null = none) and the room for the chunk counts of a view's sources, on `st`
int upload_rtinfo(l3d_ctx* c, const l3d_chain_view* views, int n_views, const std::vector<const int*>& rt, int maxS, int maxN, hipStream_t st)
{
    std::vector<RtInfo>& info = c->rtinfo_host;     // (lives in the context: the upload is asynchronous)
    info.resize((size_t)n_views);
    for (int k = 0; k < n_views; ++k) info[(size_t)k] = RtInfo{ rt[(size_t)k], views[k].S_src, views[k].N };
    HIPCHK(c, c->ch_rtinfo.reserve((size_t)n_views * sizeof(RtInfo) + 64));
    HIPCHK(c, c->ch_existpart.reserve((size_t)std::max(1, maxN) * exist_chunks() * (size_t)std::max(1, maxS) * 4 + 256));     // chunk counts / bases of a view's sources
    HIPCHK(c, hipMemcpyAsync(c->ch_rtinfo.p, info.data(), info.size() * sizeof(RtInfo), hipMemcpyHostToDevice, st));
    return L3D_OK;
}

}  // namespace

namespace {

// run-ahead depths, A/B measured on one box (ms per config-2 pass): (12, 24) 19.1, (6, 12) 18.7, (4, 8) 18.4, (2, 4) 18.3,
// (24, 40) 20.0 -- a shallow queue keeps the stage-1 candidates of a view cache-warm until its chain consumes them
// the ring covers every view that can be in flight between the one being collected and the newest stage 1: after an
// overflow ALL of them are refilled before any of their chains runs again (bit rows and stage-1 candidates alike)
constexpr int kAhead = L3D_AHEAD, kStage1Ahead = L3D_S1AHEAD, kRing = kAhead + kStage1Ahead + 3;

// The delivery thread of a chain with a callback: finished views are handed to it in order (push); it copies a view's kept slice and depth pairs to
// the host (copy stream, SDMA) and runs the caller's bookkeeping -- so the ~13 launches per view of the enqueueing thread are never held up by host
// work.  A resident run (no callback) hands nothing to the host: no thread, push only counts the kept records.
class Delivery {
public:
    Delivery(l3d_ctx* c_, const l3d_chain_view* views_, const std::vector<ViewDev>& vd_, l3d_chain_callback cb_, void* user_)
        : c(c_), views(views_), vd(vd_), cb(cb_), user(user_) { if (cb) th = std::thread([this]() { run(); }); }
    ~Delivery() { finish(); }
    void push(int k, int verified, const ChainResult& r)
    {
        if (!cb) { if (verified) kept_total += r.n_kept; return; }
        { std::lock_guard<std::mutex> lk(mu); work.push_back(Item{ k, verified, r }); }
        cv_work.notify_one();
    }
    void wait_idle()                                    // every handed-over view has left the device arena
    {
        if (!cb) return;
        std::unique_lock<std::mutex> lk(mu);
        cv_idle.wait(lk, [&]() { return work.empty() && !busy; });
    }
    bool failed() { std::lock_guard<std::mutex> lk(mu); return rc != L3D_OK; }
    // the queue drained and the thread joined: the first delivery's error (text: its message), or L3D_OK
    int finish(std::string* text = nullptr)
    {
        if (th.joinable()) {
            { std::lock_guard<std::mutex> lk(mu); done = true; }
            cv_work.notify_one();
            th.join();
        }
        if (text) *text = err;
        return rc;
    }
    double kept_total = 0, t_cb = 0, t_d2h = 0;

private:
    struct Item { int k; int verified; ChainResult r; };
    void run()
    {
        (void)hipSetDevice(c->device);
        for (;;) {
            Item it;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&]() { return done || !work.empty(); });
                if (work.empty()) return;
                it = work.front();
                work.pop_front();
                busy = true;
            }
            int it_rc = L3D_OK;
            std::string it_err;
            if (rc == L3D_OK) deliver(it, it_rc, it_err);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (it_rc && rc == L3D_OK) { rc = it_rc; err = it_err; }
                busy = false;
            }
            cv_idle.notify_all();
        }
    }
    void deliver(const Item& it, int& it_rc, std::string& it_err)
    {
        const l3d_chain_view& v = views[it.k];
        const ViewDev& d = vd[(size_t)it.k];
        if (!it.verified) {                     // cudawrapper.cu:877-878: nothing to match, the caller keeps its list
            if (cb(user, it.k, 0, nullptr, 0, nullptr, 0, 0)) { it_rc = L3D_ERR_INVALID; it_err = "callback failed"; }
            return;
        }
        const double td0 = now_s();
        // the kept list lands in the pinned arena, where it stays valid for the caller until the next chain starts
        hipError_t e = hipSuccess;
        l3d_match* kept_host = static_cast<l3d_match*>(c->pin_arena.alloc((size_t)it.r.n_kept * sizeof(Match) + 16, &e));
        if (e == hipSuccess) e = c->ch_pin_best.reserve((size_t)v.S_src * 8 + 16);
        if (e == hipSuccess && it.r.n_kept)
            e = hipMemcpyAsync(kept_host, c->ch_kept.as<Match>() + it.r.kept_base, (size_t)it.r.n_kept * sizeof(Match), hipMemcpyDeviceToHost, c->copy_stream);
        if (e == hipSuccess && v.S_src) e = hipMemcpyAsync(c->ch_pin_best.p, d.best, (size_t)v.S_src * 8, hipMemcpyDeviceToHost, c->copy_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->copy_stream);
        if (e != hipSuccess) { it_rc = L3D_ERR_HIP; it_err = std::string("chain delivery, view ") + std::to_string(it.k) + ": " + hipGetErrorString(e); return; }
        float* best = c->ch_pin_best.as<float>();
        int nb = 0;
        if (it.r.R > 0)
            for (int s = 0; s < v.S_src; ++s)
                if (best[2 * s] != -1.0f) { best[2 * nb] = best[2 * s]; best[2 * nb + 1] = best[2 * s + 1]; ++nb; }   // in place: nb <= s
        kept_total += it.r.n_kept;
        const double tc0 = now_s();
        t_d2h += tc0 - td0;
        if (cb(user, it.k, 1, kept_host, it.r.n_kept, best, nb, it.r.R)) { it_rc = L3D_ERR_INVALID; it_err = "callback failed"; }
        t_cb += now_s() - tc0;
    }

    l3d_ctx* c; const l3d_chain_view* views; const std::vector<ViewDev>& vd; l3d_chain_callback cb; void* user;
    std::mutex mu;
    std::condition_variable cv_work, cv_idle;
    std::deque<Item> work;
    bool done = false, busy = false;
    int rc = L3D_OK;
    std::string err;
    std::thread th;
};

// One call of run_chain: what its phases share.  The phases run in the order run_chain names them; every HIP call keeps its stream and its place.
struct ChainRun {
    l3d_ctx* c; const l3d_chain_view* views; int n_views; l3d_chain_callback cb; const l3d_dense_map* map; int k_begin, k_end; const ChainPreload* pre; bool ranged;
    hipStream_t st = nullptr, s1 = nullptr, sp = nullptr;   // phase 2 (the chain proper) | stage 1, running ahead | the early transposes' side stream
    std::vector<ViewDev> vd;
    ChainLayout L;
    const unsigned char* dtab = nullptr;
    int maxN = 0;
    bool fused_rows = false;
    // per-view results are written by the kernels straight into host-mapped pinned memory (no copy operations on the streams)
    ChainResult *hres = nullptr, *hres_dev = nullptr;
    int *hstats = nullptr, *hstats_dev = nullptr;
    std::vector<hipEvent_t> ev1, ev;    // a view's stage 1 / its chain is through
    int k_p1 = 0, k_enq = 0;            // next view whose stage 1 / whose phase 2 is enqueued
    double pairs = 0;
    size_t cand_cap = 0, arena_cap = 0, turn_room = 0;
    bool same_scene = false;
    std::vector<char> has_rec;          // views that own a slice of the arena: the range's verified views and the preloaded ones (a view's slice starts where the previous such view's ended)
    long long pre_records = 0;
    Products& PE;
    bool early = false;
    int early_batch = 1, early_next = 0, early_maxSt = 1;   // views [0, early_next) have their transposes launched
    double t_ev1 = 0, t_wait = 0;       // host time spent waiting for stage-1 statistics / for view results
    double kept_seen = 0;               // kept records / views whose result record the host has read (sizes the source scans)
    int views_seen = 0;
    double raw_sum = 0;
    int rc_final = L3D_OK;
    double t_enter = 0, t_setup0 = 0, t_loop0 = 0;

    ChainRun(l3d_ctx* c_, const l3d_chain_view* views_, int n_views_, l3d_chain_callback cb_, const l3d_dense_map* map_, int k_begin_, int k_end_, const ChainPreload* pre_, bool ranged_)
        : c(c_), views(views_), n_views(n_views_), cb(cb_), map(map_), k_begin(k_begin_), k_end(k_end_), pre(pre_), ranged(ranged_),
          ev1((size_t)n_views_, nullptr), ev((size_t)n_views_, nullptr), has_rec((size_t)n_views_, 0), PE(c_->products) {}

    bool hip_ok(hipError_t e, const char* what)
    {
        if (e == hipSuccess) return true;
        rc_final = fail(c, L3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        return false;
    }
    // (the four depths of a stage-1 pair are triangulated once, by k_pair_fill: it runs ahead on the stage-1 stream, its true row counts are in place
    // before the chain counts the view's reverse matches on top)
    PairArgs pair_args(int k) const { return chain_pair_args(c, views[k], vd[(size_t)k], dtab); }
    uint2* ringA_meta(int k) const { return c->ch_ringA_meta.as<uint2>() + (size_t)(k % kRing) * cand_cap; }
    float4* ringA_depths(int k) const { return c->ch_ringA_depths.as<float4>() + (size_t)(k % kRing) * cand_cap; }
    bool early_fits() const { return early && arena_cap < 0x7ffffff0ull; }      // (beyond 2^31 records the end transposes block by block)

    int setup();
    void restrict_to_range();
    int plan_capacities();
    int plan_early();
    int reserve_caps();
    int take_over_preload();
    void enqueue_fillA(int k, hipStream_t s);
    int enqueue_stage1(int k);
    int enqueue_view(int k);
    void launch_early(int k0, int n, double avg_run, hipStream_t s);
    bool grow_buffer(DevBuf& b, size_t bytes, size_t used, const char* what);
    bool grow_arena(int k, const ChainResult& r);
    bool restart_at(int k, const ChainResult& r, Delivery& dl);
    int products_tail(l3d_chain_summary* summary, int64_t* n_pot);
    int finish(const Delivery& dl, double t_prod0);
};

// ---- streams, validation, table layout and upload, per-view slices of the whole-run arenas (l3d_chain_common.hip: shared with the sharded chain),
// the result records and the event that lets stage 1 start
int ChainRun::setup()
{
    c->pin_arena.reset();
    st = c->stream;
    s1 = c->stage1_stream;              // stage 1 runs ahead here, concurrently with the latency-bound kernels of phase 2
    if (c->opt.chain_serial != 0) s1 = st;      // diagnostic: one stream, kernels one at a time (isolated durations)
    (void)hipGetLastError();            // errors of earlier, already reported calls are not ours
    if (int rc = chain_plan_views(c, views, n_views, 0, 1, vd, L, "l3d_match_chain")) return rc;
    if (int rc = chain_upload_tables(c, views, n_views, vd, L, st)) return rc;
    // run tables (round 6): the kept writer fills one per view and leaves a (local camera << 16 | target) word per record in the side array
    // (ch_keptcam); later views and the products read runs instead of scanning lists
    if (int rc = chain_assign_arenas(c, views, n_views, vd, L, true, true, kRing, st, true)) return rc;
    {
        std::vector<const int*> rts((size_t)n_views);
        for (int k = 0; k < n_views; ++k) rts[(size_t)k] = vd[(size_t)k].rt;
        if (int rc = upload_rtinfo(c, views, n_views, rts, L.maxS, L.maxN, st)) return rc;
    }
    dtab = L.dtab;
    maxN = L.maxN;
    // the row starts of the stage-1 candidates are formed inside k_pair_fill from k_pair_mask's counters and their block sums: no
    // scan launch on the stage-1 stream (the longer of the two), no statistics for the host to wait for -- up to 96 neighbours
    fused_rows = chain_fused_rows(maxN);
    if (ranged) restrict_to_range();    // (after the arenas are laid out for all views: a view keeps its slices whatever the range is)
    HIPCHK(c, c->ch_res.reserve((size_t)n_views * sizeof(ChainResult) + 16));
    HIPCHK(c, c->ch_flags.reserve(64));
    HIPCHK(c, c->ch_pin_res.reserve((size_t)n_views * (sizeof(ChainResult) + 8) + 64));
    HIPCHK(c, hipMemsetAsync(c->ch_res.p, 0, (size_t)n_views * sizeof(ChainResult), st));
    HIPCHK(c, hipMemsetAsync(c->ch_flags.p, 0, 64, st));
    {   // stage 1 starts after the tables and the zeroed row counts are in place
        hipEvent_t ready = get_local_event(c);
        HIPCHK(c, hipEventRecord(ready, st));
        HIPCHK(c, hipStreamWaitEvent(s1, ready, 0));
        put_local_event(c, ready);
    }
    hres = c->ch_pin_res.as<ChainResult>();
    hstats = reinterpret_cast<int*>(c->ch_pin_res.as<unsigned char>() + (size_t)n_views * sizeof(ChainResult));
    if (ranged) memset(hres, 0, (size_t)n_views * sizeof(ChainResult));          // (views outside the range: no records, whatever an earlier chain left here)
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&hres_dev), hres, 0));
    hstats_dev = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(hres_dev) + (size_t)n_views * sizeof(ChainResult));
    { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(c, L3D_ERR_HIP, std::string("chain setup: ") + hipGetErrorString(e_)); }
    return L3D_OK;
}

// views outside [k_begin, k_end) launch nothing; the pair counts that size the capacities are the range's
void ChainRun::restrict_to_range()
{
    double p_range = 0, p_max = 0;
    for (int k = 0; k < n_views; ++k) {
        if (k < k_begin || k >= k_end) { vd[(size_t)k].verified = false; continue; }
        if (!vd[(size_t)k].verified) continue;
        double p = 0;
        for (int j = 0; j < views[k].n_tbm; ++j) p += (double)views[k].S_src * views[k].offsets[2 * views[k].to_be_matched[j] + 1];
        p_range += p; p_max = std::max(p_max, p);
    }
    L.pairs = p_range; L.max_pairs = p_max;
}

// ---- capacities (guarded on the device; an overflow restarts the chain at that view with more room): first guesses, what the last pass over the
// same scene ended with, option arena_guess, the tests' caps, the records of a preload, a turn's room
int ChainRun::plan_capacities()
{
    pairs = L.pairs;
    c->stats[0] = pairs;
    // first guess from the pair counts (raw density ~6 %, kept ~0.2 % of the pairs on the synthetic scenes)
    cand_cap = chain_first_cand_cap(L.max_pairs);
    // The kept arena's first guess is GENEROUS (5 % of the pairs: the densest synthetic scene keeps 4.5 %, config 2 0.16 %) within 35 % of the free HBM: memory that is
    // never written costs an allocation of a millisecond when it is the process's first big one, while growing later means a hipMalloc of tens of GB in a process that
    // has freed big buffers before -- measured at 256 x 4000 x 24: 0.5 ms for the first 59 GB, 1.8-2.2 s for 75 GB at the second regrow, 25 ms per GB at 40 views in one
    // run of three (profiles/r6_first_pass_allocations.txt).  A job sized by memory gives its capacities (l3d_set_chain_capacities) or the old guess (L3D_ARENA_GUESS=4)
    arena_cap = (size_t)(pairs * 0.004) + 1048576;
    // a pass over the same scene (same number of views, same pair count) starts with what the previous one ended up needing: no
    // overflow, no restart, no allocation after the first pass
    same_scene = c->chain_seen_views == n_views && c->chain_seen_pairs == pairs;
    if (same_scene) { cand_cap = std::max(cand_cap, c->chain_seen_cand_cap); arena_cap = std::max(arena_cap, c->chain_seen_arena_cap); }
    else if (c->opt.arena_guess > 4 && !ranged && !pre) {      // (a block of views of a partitioned job is sized by memory: it keeps the small guess and grows)
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            const size_t want = (size_t)(pairs * 0.001 * c->opt.arena_guess) + 1048576, fits = (size_t)((double)fr * 0.35 / 40.0);
            arena_cap = std::max(arena_cap, std::min(want, fits));
        }
        (void)hipGetLastError();
    }
    if (c->test_cand_cap) cand_cap = c->test_cand_cap;      // tests: force the overflow / restart path
    if (c->test_arena_cap) arena_cap = c->test_arena_cap;
    for (int k = 0; k < n_views; ++k) has_rec[(size_t)k] = vd[(size_t)k].verified ? 1 : 0;
    if (pre) {
        if (pre->k1 != k_begin || pre->k0 < 0 || pre->k0 > pre->k1 || (int)pre->n_kept.size() != pre->k1 - pre->k0 || (int)pre->R.size() != pre->k1 - pre->k0) return fail(c, L3D_ERR_INVALID, "match_chain: bad preload");
        for (int k = pre->k0; k < pre->k1; ++k) { pre_records += pre->n_kept[(size_t)(k - pre->k0)]; has_rec[(size_t)k] = views[k].n_tbm > 0 ? 1 : 0; }
        arena_cap += (size_t)pre_records;
        kept_seen = (double)pre_records;
        views_seen = pre->k1 - pre->k0;
    }
    // a turn of a node object that hands the chain over (match_chain_turn) under option regrow_free_mb: the room binds on everything the turn's arena
    // takes -- this first guess, the regrow below, the slices its share puts behind the records -- as it does on the compact arena of a plain turn
    turn_room = c->turn_arena_room;
    if (turn_room) {
        if ((size_t)pre_records + 65536 > turn_room)
            return fail(c, L3D_ERR_NOMEM, "match_chain: the " + std::to_string(pre_records) + " records taken over from the turn before need more than the room for " + std::to_string(turn_room) + " records (" +
                                          std::to_string(c->opt.regrow_free_mb) + " MB at " + std::to_string(sizeof(Match) + 4) + " B per record)");
        arena_cap = std::min(arena_cap, turn_room);
    }
    return L3D_OK;
}

// early pair transposes (round 6, l3d_products.hip): a (view, camera) pair of the potential-correspondence build depends on that view's kept list alone, so
// it is transposed on a side stream right behind the view's kept writer -- next to the following views' chains -- and the end of matchViews finds only the rows
// left.  Entries live in an array aligned with the kept arena (a view's pairs hold exactly its records).  L3D_PROD_EARLY=0: all transposes at the end (A/B)
// Long lists only (> 2^18 records per view: what the last pass over this scene kept, or the arena's first guess), view by view.  At config 2 (36 k records per view)
// two launches and an event per view cost more than the 0.2 ms of transposes they take off the end (12.60 vs 12.41 ms per pass); eight views per launch still lose
// (12.52 vs 12.41; the first pass pays 5 ms for the side stream and its buffers).  Option values 2 / 3 force a view / eight views per launch (tests)
int ChainRun::plan_early()
{
    early = map && !ranged && !pre && !cb && c->opt.prod_early != 0 && c->opt.prod_transpose != 0 && maxN > 0;
    early_batch = c->opt.prod_early == 3 ? 8 : 1;
    if (early && c->opt.prod_early == 1) {
        const double per_view = (same_scene && c->chain_seen_kept > 0 ? c->chain_seen_kept : pairs * 0.004) / std::max(1, n_views);
        early = per_view > (double)chain_long_list(c->opt);
    }
    if (!early) return L3D_OK;
    std::vector<int> tab((size_t)n_views * maxN * 2 + (size_t)n_views * (sizeof(EarlyView) / 4), 0);       // [St | boff_off], n_views x maxN each; the views' descriptors behind them
    PE.e_boff_off.assign((size_t)n_views * maxN, 0);
    long long nb = 0;
    for (int k = 0; k < n_views && early; ++k) {
        if (!vd[(size_t)k].verified) continue;
        for (int q = 0; q < views[k].N; ++q) {
            const uint32_t* it = std::lower_bound(map->view_ids, map->view_ids + map->n_views, views[k].local2global[q]);
            if (it == map->view_ids + map->n_views || *it != views[k].local2global[q]) continue;
            const int t = (int)(it - map->view_ids), St = map->seg_base[t + 1] - map->seg_base[t];
            if (St <= 0) continue;
            tab[(size_t)k * maxN + q] = St;
            tab[(size_t)n_views * maxN + (size_t)k * maxN + q] = (int)nb;
            PE.e_boff_off[(size_t)k * maxN + q] = (int)nb;
            nb += St + 1;
            early_maxSt = std::max(early_maxSt, St);
            if (nb > 0x7ffffff0ll) early = false;
        }
    }
    if (!early) return L3D_OK;
    if (!c->prod_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->prod_stream, hipStreamNonBlocking));
    sp = c->prod_stream;
    HIPCHK(c, PE.e_tab.reserve(tab.size() * 4 + 64));
    static_assert(sizeof(EarlyView) % 8 == 0, "descriptor size");
    {
        const int* dt = PE.e_tab.as<int>();
        EarlyView* hv = reinterpret_cast<EarlyView*>(tab.data() + (size_t)n_views * maxN * 2);       // (n_views * maxN * 2 ints: 8-byte aligned)
        for (int k = 0; k < n_views; ++k) {
            EarlyView e;
            e.rt = vd[(size_t)k].verified ? vd[(size_t)k].rt : nullptr;
            e.St = dt + (size_t)k * maxN; e.boff_off = dt + (size_t)n_views * maxN + (size_t)k * maxN;
            e.k = k; e.S = views[k].S_src; e.N = views[k].N; e.pad = 0;
            hv[k] = e;
        }
    }
    HIPCHK(c, PE.e_cnt.reserve((size_t)n_views * maxN * 4 + 64));
    HIPCHK(c, PE.e_poff.reserve((size_t)n_views * maxN * 4 + 64));
    HIPCHK(c, PE.e_boff.reserve((size_t)nb * 4 + 64));
    HIPCHK(c, hipMemcpyAsync(PE.e_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));                    // (`tab` is pageable and leaves scope)
    return L3D_OK;
}

// the buffers sized by the capacities (at the start, and again after an overflow)
int ChainRun::reserve_caps()
{
    if (int rc = chain_reserve_candidates(c, L, cand_cap, kRing)) return rc;
    HIPCHK(c, c->ch_kept.reserve(arena_cap * sizeof(Match)));
    HIPCHK(c, c->ch_keptcam.reserve(arena_cap * 4 + 64));
    if (early_fits()) { HIPCHK(c, PE.e_E.reserve(arena_cap * 4 + 64)); HIPCHK(c, PE.e_T.reserve(arena_cap * 4 + 64)); }
    return L3D_OK;
}

// the views [pre->k0, pre->k1) taken over from another rank: their records at the head of the arena with their result records, their best depth pairs
// and positions in their own slices, their side words and run tables rebuilt
int ChainRun::take_over_preload()
{
    if (!pre || pre->k1 <= pre->k0) return L3D_OK;
    long long base = 0;
    size_t so = 0;
    for (int k = pre->k0; k < pre->k1; ++k) {
        ChainResult r;
        r.kept_base = (uint64_t)base; r.n_want = 0; r.n_kept = has_rec[(size_t)k] ? pre->n_kept[(size_t)(k - pre->k0)] : 0; r.R = pre->R[(size_t)(k - pre->k0)]; r.overflow = 0;
        hres[k] = r;
        base += r.n_kept;
        if (views[k].n_tbm > 0) {
            // (chain_assign_arenas gave every verified view of the schedule its slices, whatever the range)
            ChainViewDev& d = vd[(size_t)k];
            if (views[k].S_src > 0 && d.best && pre->best) HIPCHK(c, hipMemcpyAsync(d.best, pre->best + so, (size_t)views[k].S_src * 8, hipMemcpyDeviceToDevice, st));
            if (views[k].S_src > 0 && d.bestpos && pre->bestpos) HIPCHK(c, hipMemcpyAsync(d.bestpos, pre->bestpos + so, (size_t)views[k].S_src * 4, hipMemcpyDeviceToDevice, st));
            so += (size_t)views[k].S_src;
        }
    }
    if (base > 0) HIPCHK(c, hipMemcpyAsync(c->ch_kept.p, pre->records, (size_t)base * sizeof(Match), hipMemcpyDeviceToDevice, st));
    if (base > 0) {
        // the taken-over lists did not come out of this chain's kept writer: their side array and run tables are rebuilt from the records
        std::vector<RtJob> jobs;
        std::vector<const unsigned*> l2g;
        for (int k = pre->k0; k < pre->k1; ++k) {
            if (!has_rec[(size_t)k] || hres[k].n_kept == 0) continue;
            if (!vd[(size_t)k].rt) return fail(c, L3D_ERR_INVALID, "match_chain: view " + std::to_string(k) + " was taken over with records but has no run table");
            RtJob j;
            j.recs = c->ch_kept.as<Match>() + hres[k].kept_base; j.qt = c->ch_keptcam.as<unsigned>() + hres[k].kept_base; j.rt = vd[(size_t)k].rt;
            j.ids = nullptr; j.qs = nullptr; j.n = hres[k].n_kept; j.S = views[k].S_src; j.N = views[k].N; j.pad = 0;
            jobs.push_back(j);
            l2g.push_back(views[k].local2global);
        }
        if (!jobs.empty()) {
            int bad = 0;
            if (int rc = rebuild_run_tables(c, jobs, l2g, st, &bad)) return rc;
            if (bad) return fail(c, L3D_ERR_INVALID, "match_chain: the lists taken over from another rank are not ordered (segment, camera) -- no run tables");
        }
    }
    HIPCHK(c, hipMemcpyAsync(c->ch_res.as<ChainResult>() + pre->k0, hres + pre->k0, (size_t)(pre->k1 - pre->k0) * sizeof(ChainResult), hipMemcpyHostToDevice, st));
    return L3D_OK;
}

// ---- phase 1 (stage 1 of a view: pair test -> bit rows -> row counts -> statistics) is independent of the
// chain; it is enqueued a window ahead of phase 2 so that the GPU always has work while the host trails behind
// row starts + depth records of a view's stage-1 candidates alone (its reverse matches are not known yet), into the view's ring slot; k_place
// later moves them into the combined order on the chain stream, which stays short.  (Measured: triangulating on the chain stream instead was 5 %
// slower on config 2; letting the verification read the stage-1 candidates in place instead of copying them 20 % SLOWER -- the copy is a streaming
// pass that leaves the candidates cache-hot for the latency-bound kernels that follow.)
void ChainRun::enqueue_fillA(int k, hipStream_t s)
{
    const ViewDev& d = vd[(size_t)k];
    const PairArgs pa = chain_fill_args(pair_args(k), d, fused_rows, cand_cap);
    { ProfScope p(c, "pair_fill", s); launch_pair_fill(pa, d.rowA, ringA_meta(k), ringA_depths(k), s); }
}
int ChainRun::enqueue_stage1(int k)
{
    if (!vd[(size_t)k].verified) return L3D_OK;
    hstats[2 * k] = hstats[2 * k + 1] = 0;
    if (views[k].S_src > 0) {
        const PairArgs pa = pair_args(k);
        {   // bit rows + row counts (added into the rows zeroed at chain start) in one launch
            const PairArgs pm = chain_mask_args(pa, vd[(size_t)k], fused_rows);
            ProfScope p(c, "pair_mask", s1);
            launch_pair_mask(pm, vd[(size_t)k].maxW, s1, c->opt.pair_spb);
        }
        // (unfused) row starts of the stage-1 candidates + their statistics straight into host-mapped memory (one launch)
        if (!fused_rows) { ProfScope p(c, "scan", s1); launch_scan(vd[(size_t)k].rowcnt, vd[(size_t)k].rowA, views[k].S_src * views[k].N, nullptr, s1, nullptr, views[k].N, 0, views[k].S_src, hstats_dev + 2 * k); }
        // the ring slot was last used by view k - kRing: wait until its chain has consumed it
        for (int j = k - kRing; j >= 0; j -= kRing) if (ev[(size_t)j]) { HIPCHK(c, hipStreamWaitEvent(s1, ev[(size_t)j], 0)); break; }
        enqueue_fillA(k, s1);
    }
    ev1[(size_t)k] = get_local_event(c);
    HIPCHK(c, hipEventRecord(ev1[(size_t)k], s1));
    return L3D_OK;
}

// ---- phase 2 of view k on the chain stream (behind the stage 1 of the views up to kStage1Ahead in front of it): its candidates collected, verified, its
// kept records written behind the previous view's, the event the host trails on -- and the early transposes of the views that are due
int ChainRun::enqueue_view(int k)
{
    const l3d_chain_view& v = views[k];
    const ViewDev& d = vd[(size_t)k];
    while (k_p1 < n_views && k_p1 <= k + kStage1Ahead) { int rc = enqueue_stage1(k_p1); if (rc) return rc; ++k_p1; }
    if (!d.verified) return L3D_OK;
    const double te0 = now_s();
    if (!fused_rows) HIPCHK(c, hipEventSynchronize(ev1[(size_t)k]));          // its stage-1 statistics (enqueued a window earlier)
    t_ev1 += now_s() - te0;
    HIPCHK(c, hipStreamWaitEvent(st, ev1[(size_t)k], 0));
    PairArgs pa = pair_args(k);
    pa.cand_cap = (int)cand_cap;
    const int S = v.S_src, N = v.N;
    const size_t nrow = (size_t)S * N;
    Match* arena = c->ch_kept.as<Match>();
    ChainResult* dres = c->ch_res.as<ChainResult>();
    const int* d_sc = reinterpret_cast<const int*>(dtab + d.o_sc);
    (void)hipGetLastError();
    const int* d_si = reinterpret_cast<const int*>(dtab + d.o_si);
    unsigned* cams = c->ch_keptcam.as<unsigned>();
    // sized from the lists the chain has seen so far (the host trails a few views behind); short lists (config 2 keeps 36 k matches per view) are
    // scanned record by record
    const CollectRule rule = chain_collect_rule(c->opt, views_seen > 0, views_seen > 0 ? kept_seen / views_seen : 0.0, S, N, L.maxS);
    ++c->chain_routes[rule.rt ? 1 : 0];
    CollectIn ci;
    ci.arena = arena; ci.dres = dres; ci.cams = cams; ci.info = c->ch_rtinfo.as<RtInfo>(); ci.d_sc = d_sc; ci.d_si = d_si;
    ci.d_ss = reinterpret_cast<const int*>(dtab + d.o_ss); ci.d_tbm = pa.tbm; ci.n_sources = v.n_sources; ci.n_tbm = v.n_tbm; ci.view_id = v.view_id; ci.S = S; ci.N = N;
    ci.rowcnt = d.rowcnt; ci.rowA = d.rowA; ci.metaA = ringA_meta(k); ci.depthsA = ringA_depths(k); ci.cand_cap = cand_cap;
    ci.sort_apart = !(c->verify_mode == 0 && verify_window_supported(N));     // (the window kernel orders the runs itself)
    enqueue_collect(c, ci, rule, st);
    VerifyArgs va = chain_verify_args(c, v, d, dtab, cand_cap);
    va.res = dres + k;
    // (fused row starts: no statistics -- the largest LDS image the budget allows)
    chain_launch_verify(c, va, d, d_sc, v.n_sources, fused_rows ? -1 : hstats[2 * k + 1], cand_cap, st);
    {
        ProfScope p(c, "kept_write");
        int pv = k - 1;
        while (pv >= 0 && !has_rec[(size_t)pv]) --pv;                    // the arena slice starts where the previous verified (or preloaded) view's ended
        launch_kept_write_chain(va, c->kept_cnt.as<int>(), (int)nrow, pv >= 0 ? dres + pv : nullptr, (unsigned long long)arena_cap, dres + k, hres_dev + k,
                                reinterpret_cast<const unsigned*>(dtab + d.o_l2g), arena, st, (map || ranged) ? d.bestpos : nullptr, cams, d.rt, S);
    }
    { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(c, L3D_ERR_HIP, std::string("chain launch, view ") + std::to_string(k) + ": " + hipGetErrorString(e_)); }
    // (with a delivery callback the host starts D2H copies of device memory once it has seen this event: a default, fenced event then)
    if (!ev[(size_t)k]) ev[(size_t)k] = cb ? get_event(c) : get_local_event(c);
    HIPCHK(c, hipEventRecord(ev[(size_t)k], st));
    if (early_fits() && k + 1 - early_next >= early_batch) {
        HIPCHK(c, hipStreamWaitEvent(sp, ev[(size_t)k], 0));
        launch_early(early_next, k + 1 - early_next, rule.avg_run, sp);
        early_next = k + 1;
    }
    return L3D_OK;
}
// the transposes of the views [k0, k0 + n) on stream s
void ChainRun::launch_early(int k0, int n, double avg_run, hipStream_t s)
{
    launch_early_transposes(c, reinterpret_cast<const EarlyView*>(PE.e_tab.as<int>() + (size_t)n_views * maxN * 2), k0, n, maxN, early_maxSt, c->ch_res.as<ChainResult>(), c->ch_keptcam.as<unsigned>(),
                            PE.e_cnt.as<int>(), PE.e_poff.as<unsigned>(), PE.e_boff.as<int>(), PE.e_E.as<unsigned>(), PE.e_T.as<unsigned>(), avg_run, s);
}

// ---- an overflow.  The arena cannot be reallocated without losing earlier lists that later views still read: its used part is copied over
// (DevBuf::grow_keep), and so are the side words and -- the earlier views' transposed entries move with their records -- the early transposes' entries.
bool ChainRun::grow_buffer(DevBuf& b, size_t bytes, size_t used, const char* what)
{
    const hipError_t e = b.grow_keep(bytes, used, st);
    return hip_ok(e, e == hipErrorOutOfMemory ? what : "hipMemcpy");
}
bool ChainRun::grow_arena(int k, const ChainResult& r)
{
    const int n_pre = pre ? pre->k1 - pre->k0 : 0;
    size_t fr = 0, tot = 0;
    const bool known = hipMemGetInfo(&fr, &tot) == hipSuccess;
    if (known && c->opt.regrow_free_mb > 0) fr = std::min(fr, (size_t)c->opt.regrow_free_mb << 20);     // (tests: a card with less room)
    (void)hipGetLastError();
    const ArenaRegrow g = chain_arena_regrow(arena_cap, r.kept_base, r.n_want, k - k_begin + n_pre, k_end - k_begin + n_pre, known ? fr : kRegrowFreeUnknown, turn_room, early, map != nullptr);
    if (!g.ok) {
        rc_final = fail(c, L3D_ERR_NOMEM, "match_chain: the kept arena of " + std::to_string(arena_cap) + " records is full at view " + std::to_string(k) + " of " + std::to_string(n_views) + " (" +
                                              std::to_string((size_t)r.kept_base) + " records in use, the view keeps " + std::to_string(r.n_want) + ") and an arena of " +
                                              std::to_string(g.need) + " records does not fit beside it (room for " + std::to_string(g.fits) + " at " + std::to_string(g.per_rec) + " B per record, " +
                                              std::to_string(g.reserve >> 20) + " MB kept back; " + std::to_string(fr >> 20) + " of " + std::to_string(tot >> 20) +
                                              " MB free): l3d_set_chain_capacities sizes the arena up front");
        return false;
    }
    const size_t new_cap = g.new_cap, used = (size_t)r.kept_base;
    double ms[3] = { 0, 0, 0 };
    const hipError_t e = c->ch_kept.grow_keep(new_cap * sizeof(Match), used * sizeof(Match), st, ms);
    if (e == hipErrorOutOfMemory) {
        (void)hipMemGetInfo(&fr, &tot);
        rc_final = fail(c, L3D_ERR_NOMEM, "match_chain: growing the kept arena to " + std::to_string(new_cap * sizeof(Match) >> 20) + " MB at view " + std::to_string(k) + " of " + std::to_string(n_views) +
                                          " (" + std::to_string(used * sizeof(Match) >> 20) + " MB in use, " + std::to_string(fr >> 20) + " of " + std::to_string(tot >> 20) + " MB free): " + hipGetErrorString(e));
        return false;
    }
    if (!hip_ok(e, "hipMemcpy")) return false;
    if (c->opt.timing) fprintf(stderr, "[l3d match_chain]   arena of %zu MB: hipMalloc %.2f ms, copy of %zu MB %.2f ms, hipFree of the old one %.2f ms\n", new_cap * sizeof(Match) >> 20, ms[0],
                               used * sizeof(Match) >> 20, ms[1], ms[2]);
    if (!grow_buffer(c->ch_keptcam, new_cap * 4 + 64, used * 4, "hipMalloc (side words of the kept arena)")) return false;
    if (early && new_cap < 0x7ffffff0ull && !grow_buffer(PE.e_E, new_cap * 4 + 64, used * 4, "hipMalloc (transposed entries of the kept arena)")) return false;
    arena_cap = new_cap;
    return true;
}
// View k came back without room for its candidates (1) / its kept matches (2): everything before it is valid and stays in the arena.  The queue and
// the delivery of earlier views drain, the buffers grow, the ring is refilled and the enqueueing rewinds to k.  false: rc_final says why not
bool ChainRun::restart_at(int k, const ChainResult& r, Delivery& dl)
{
    if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize") || !hip_ok(hipStreamSynchronize(s1), "hipStreamSynchronize")) return false;
    if (sp && !hip_ok(hipStreamSynchronize(sp), "hipStreamSynchronize")) return false;
    const double t_restart0 = now_s();
    dl.wait_idle();
    if (r.overflow & 1) cand_cap = (size_t)r.R + (size_t)r.R / 4 + 65536;
    if ((r.overflow & 2) && !grow_arena(k, r)) return false;
    { int rc = reserve_caps(); if (rc) { rc_final = rc; return false; } }
    if (c->opt.timing) fprintf(stderr, "[l3d match_chain] view %d of %d overflowed (%d): candidates %zu, arena %zu records; regrown in %.2f ms, %.2f ms into the loop\n", k, n_views, r.overflow, cand_cap, arena_cap,
                               (now_s() - t_restart0) * 1e3, (now_s() - t_loop0) * 1e3);
    // the row counts of the views enqueued after k were already incremented by their reverse matches: rebuild
    // and the stage-1 candidate buffers of every view in flight live in the (re-sized) ring: refill them
    for (int j = k; j < k_p1; ++j) {
        if (!vd[(size_t)j].verified || views[j].S_src == 0) continue;
        if (j < k_enq) {
            if (!hip_ok(hipMemsetAsync(vd[(size_t)j].rowcnt, 0, (size_t)views[j].S_src * views[j].N * 4, st), "hipMemsetAsync")) return false;
            if (!fused_rows) launch_row_count(pair_args(j), vd[(size_t)j].rowcnt, st);      // (fused: the upper bounds live in rowub, untouched)
        }
        enqueue_fillA(j, st);
    }
    k_enq = k;
    early_next = std::min(early_next, k);           // (the views run again are transposed again)
    return true;
}

// ---- the products of matchViews, on the device, from the arena (l3d_products.hip); enqueued behind the last view
int ChainRun::products_tail(l3d_chain_summary* summary, int64_t* n_pot)
{
    std::vector<ProdChainView> pv((size_t)n_views);
    for (int k = 0; k < n_views; ++k) pv[(size_t)k] = ProdChainView{ vd[(size_t)k].verified ? vd[(size_t)k].best : nullptr, vd[(size_t)k].verified ? vd[(size_t)k].bestpos : nullptr, vd[(size_t)k].verified ? 1 : 0,
                                                                     vd[(size_t)k].verified ? vd[(size_t)k].rt : nullptr };
    ProdEarly pe;
    const bool early_done = early_fits();
    if (early_done) {
        if (early_next < n_views) {                     // the last batch's remainder: on the chain's stream, behind the last view
            launch_early(early_next, n_views - early_next, views_seen > 0 ? kept_seen / views_seen / std::max(1.0, (double)L.maxS * std::max(1, maxN)) : 1.0, st);
            early_next = n_views;
        }
        hipEvent_t e = get_local_event(c);
        (void)hipEventRecord(e, sp);
        (void)hipStreamWaitEvent(st, e, 0);
        put_local_event(c, e);
        pe.pcnt_kq = PE.e_cnt.as<int>(); pe.poff_kq = PE.e_poff.as<unsigned>(); pe.boff = PE.e_boff.as<int>(); pe.E = PE.e_E.as<unsigned>();
        pe.boff_off_host = PE.e_boff_off.data(); pe.maxN = maxN;
    }
    return build_products(c, views, n_views, pv.data(), hres, map, summary, n_pot, 0, -1, nullptr, c->ch_keptcam.as<unsigned>(), early_done ? &pe : nullptr);
}

// the timing lines, the streams idle, the events back in their pools, the counters and -- after a pass that succeeded without the tests' caps -- what
// the next pass over the same scene starts with
int ChainRun::finish(const Delivery& dl, double t_prod0)
{
    if (c->opt.timing)
        fprintf(stderr, "[l3d match_chain] setup %.2f ms | enqueue + watch loop %.2f ms (waiting: view results %.2f, stage-1 statistics %.2f) | delivery thread: d2h %.2f, callback %.2f\n",
                (t_loop0 - t_setup0) * 1e3, (t_prod0 - t_loop0) * 1e3, t_wait * 1e3, t_ev1 * 1e3, dl.t_d2h * 1e3, dl.t_cb * 1e3);
    if (c->opt.timing && map) fprintf(stderr, "[l3d match_chain] products on the device %.2f ms\n", (now_s() - t_prod0) * 1e3);
    const double t_tail0 = now_s();
    (void)hipStreamSynchronize(s1);
    if (sp) (void)hipStreamSynchronize(sp);
    (void)hipStreamSynchronize(st);
    if (c->opt.timing) fprintf(stderr, "[l3d match_chain] hipSetDevice %.3f ms, final syncs %.3f ms\n", (t_setup0 - t_enter) * 1e3, (now_s() - t_tail0) * 1e3);
    for (hipEvent_t e : ev) { if (cb) put_event(c, e); else put_local_event(c, e); }
    for (hipEvent_t e : ev1) put_local_event(c, e);
    c->stats[1] = raw_sum;
    c->stats[3] = dl.kept_total;
    if (rc_final == L3D_OK && !c->test_cand_cap && !c->test_arena_cap) {
        c->chain_seen_views = n_views; c->chain_seen_pairs = pairs; c->chain_seen_cand_cap = cand_cap; c->chain_seen_arena_cap = arena_cap; c->chain_seen_kept = kept_seen;
    }
    return rc_final;
}

}  // namespace

// cb: per-view delivery of the kept lists to the host (l3d_match_chain); map: products built on the device at the end of the chain
// (l3d_match_chain_resident) -- either or both
// [k_begin, k_end): the views this call computes (k_end < 0: all).  Views outside the range are treated as if they had never run: they
// launch nothing and their result records stay zero, so a view inside the range finds no kept matches of a source in front of it
// (l3d_match_chain_blocks: a block of views started cold).  With a range and neither cb nor map the call only fills the kept arena and
// the per-view result records (c->ch_pin_res).
// pre: the views [pre->k0, pre->k1 = k_begin) taken over from another rank (their kept lists, best depth pairs and positions): they are put at
// the head of the arena with their result records, so the range's views find their TRUE sources -- a block of views re-run warm after its
// cold-started speculation failed, or a turn that its predecessor handed the chain over to (l3d_chain_partition.hip).
int l3d::run_chain(l3d_ctx* c, const l3d_chain_view* views, int n_views, l3d_chain_callback cb, void* user, const l3d_dense_map* map,
                   l3d_chain_summary* summary, int64_t* n_pot, int k_begin, int k_end, const ChainPreload* pre)
{
    if (!c) return L3D_ERR_INVALID;
    const bool ranged = k_end >= 0;
    if (!ranged) { k_begin = 0; k_end = n_views; }
    if (n_views < 0 || (n_views > 0 && (!views || (!cb && !map && !ranged))) || k_begin < 0 || k_end > n_views || k_begin > k_end) return fail(c, L3D_ERR_INVALID, "l3d_match_chain: bad argument");
    c->products.valid = false;
    c->chain_routes[0] = c->chain_routes[1] = 0;
    if (n_views == 0) return L3D_OK;
    ChainRun R(c, views, n_views, cb, map, k_begin, k_end, pre, ranged);
    R.t_enter = now_s();
    HIPCHK(c, hipSetDevice(c->device));
    R.t_setup0 = now_s();
    if (int rc = R.setup()) return rc;
    if (int rc = R.plan_capacities()) return rc;
    if (int rc = R.plan_early()) return rc;
    if (int rc = R.reserve_caps()) return rc;
    if (int rc = R.take_over_preload()) return rc;

    // ---- phase 2 + trailing result loop.  This thread enqueues (phase 2 of a view kAhead in front of the one it waits for, stage 1 kStage1Ahead in
    // front of that) and watches the per-view result records: an overflow grows the buffers and restarts at that view, a finished view goes, in
    // order, to the delivery thread.
    R.t_loop0 = now_s();
    Delivery dl(c, views, R.vd, cb, user);
    for (int k = 0; k < n_views && R.rc_final == L3D_OK; ++k) {
        while (R.k_enq < n_views && R.k_enq <= k + kAhead) { int rc = R.enqueue_view(R.k_enq); if (rc) { R.rc_final = rc; break; } ++R.k_enq; }
        if (R.rc_final || dl.failed()) break;
        if (!R.vd[(size_t)k].verified) { dl.push(k, 0, ChainResult()); continue; }
        const double tw0 = now_s();
        if (!R.hip_ok(hipEventSynchronize(R.ev[(size_t)k]), "hipEventSynchronize")) break;
        R.t_wait += now_s() - tw0;
        const ChainResult r = R.hres[k];
        if (r.overflow) {
            if (!R.restart_at(k, r, dl)) break;
            --k;
            continue;
        }
        R.raw_sum += r.R;                   // candidates verified (stage-1 + existing), counted when the view is final (a restart enqueues views twice)
        R.kept_seen += r.n_kept; R.views_seen += 1;
        dl.push(k, 1, r);
    }
    std::string deliver_err;
    const int deliver_rc = dl.finish(&deliver_err);
    if (R.rc_final == L3D_OK && deliver_rc) R.rc_final = fail(c, deliver_rc, deliver_err);
    const double t_prod0 = now_s();
    if (R.rc_final == L3D_OK && map) R.rc_final = R.products_tail(summary, n_pot);
    return R.finish(dl, t_prod0);
}

extern "C" int l3d_match_chain(l3d_ctx* c, const l3d_chain_view* views, int n_views, l3d_chain_callback cb, void* user)
{
    if (c && n_views > 0 && !cb) return fail(c, L3D_ERR_INVALID, "l3d_match_chain: bad argument");
    return run_chain(c, views, n_views, cb, user, nullptr, nullptr, nullptr);
}

extern "C" int l3d_match_chain_resident(l3d_ctx* c, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot)
{
    if (!c) return L3D_ERR_INVALID;
    if (!map || !map->view_ids || !map->seg_base || map->n_views < 0 || (n_views > 0 && !summary)) return fail(c, L3D_ERR_INVALID, "l3d_match_chain_resident: bad argument");
    if (n_pot) *n_pot = 0;
    return run_chain(c, views, n_views, nullptr, nullptr, map, summary, n_pot);
}

extern "C" int l3d_last_chain_routes(l3d_ctx* c, int* n_scanned, int* n_run_tables)
{
    if (!c || !n_scanned || !n_run_tables) return L3D_ERR_INVALID;
    *n_scanned = c->chain_routes[0]; *n_run_tables = c->chain_routes[1];
    return L3D_OK;
}

// host only: no context, no device
extern "C" int l3d_test_rt_lanes(int opt, double avg_run) { return rt_lanes_per_run(opt, avg_run); }
extern "C" int l3d_test_arena_regrow(uint64_t arena_cap, uint64_t kept_base, int n_want, int done, int span, uint64_t free_bytes, uint64_t turn_room, int early, int products, uint64_t out[5])
{
    if (!out) return L3D_ERR_INVALID;
    const ArenaRegrow g = chain_arena_regrow((size_t)arena_cap, kept_base, n_want, done, span, free_bytes == UINT64_MAX ? kRegrowFreeUnknown : (size_t)free_bytes, (size_t)turn_room, early != 0, products != 0);
    out[0] = g.new_cap; out[1] = g.need; out[2] = g.fits; out[3] = g.per_rec; out[4] = g.reserve;
    return g.ok ? L3D_OK : L3D_ERR_NOMEM;
}

// One view's collect step on kept lists of the caller's (tests/test_gpu_collect_paths.py): everything is validated on the host, the lists go into the
// arena with result records, side words and run tables (rebuild_run_tables), the outputs are filled with 0xff bytes, then enqueue_collect runs under
// chain_collect_rule's numbers -- what run_chain does per view.
extern "C" int l3d_test_collect_candidates(l3d_ctx* c, const l3d_chain_view* views, int n_views, int k, const l3d_match* kept, const int32_t* n_kept,
                                           const int32_t* rowA, const uint32_t* metaA, const float* depthsA, int n_A, const int32_t* rowcnt,
                                           l3d_test_collect_path* sel, int32_t* row_start, uint32_t* cand_meta, float* cand_depths, int32_t* cursor, int32_t* seg_order)
{
    if (!c) return L3D_ERR_INVALID;
    if (!sel || !views || n_views < 1 || k < 0 || k >= n_views || !n_kept || !row_start || n_A < 0 || sel->cand_cap < 0 || (sel->route != 0 && sel->route != 1) ||
        !(sel->avg_kept >= 0.0) || (sel->cand_cap > 0 && (!cand_meta || !cand_depths)) || (n_A > 0 && (!metaA || !depthsA)))
        return fail(c, L3D_ERR_INVALID, "collect_candidates: bad argument");
    const l3d_chain_view& v = views[k];
    const int S = v.S_src, N = v.N;
    if (S < 0 || S > 16384 || N < 1 || N > 255 || v.n_tbm < 1 || v.n_tbm > N || !v.to_be_matched || !v.local2global || v.n_sources < 0 ||
        (v.n_sources && (!v.source_cam || !v.source_index)) || (S > 0 && (!rowA || !rowcnt || !cursor || !seg_order)))
        return fail(c, L3D_ERR_INVALID, "collect_candidates: the view under test is not a verified view of at most 16384 segments and 255 neighbours");
    std::vector<char> is_tbm((size_t)N, 0), is_src((size_t)N, 0);
    for (int j = 0; j < v.n_tbm; ++j) {
        const int cam = v.to_be_matched[j];
        if (cam < 0 || cam >= N || is_tbm[(size_t)cam]) return fail(c, L3D_ERR_INVALID, "collect_candidates: to_be_matched out of range or repeated");
        is_tbm[(size_t)cam] = 1;
    }
    for (int q = 0; q < v.n_sources; ++q) {
        const int cam = v.source_cam[q], si = v.source_index[q];
        if (si < 0 || si >= k || cam < 0 || cam >= N || is_tbm[(size_t)cam] || is_src[(size_t)cam])
            return fail(c, L3D_ERR_INVALID, "collect_candidates: a source must be an earlier view, its camera a neighbour that is not to be matched, named once");
        is_src[(size_t)cam] = 1;
    }
    size_t n_rec = 0, rt_ints = 0;
    int maxS = S, maxN = std::max(N, v.n_sources);
    for (int j = 0; j < k; ++j) {
        const l3d_chain_view& w = views[j];
        if (w.S_src < 0 || w.S_src > 65536 || w.N < 0 || w.N > 255 || n_kept[j] < 0 || (w.N > 0 && !w.local2global) || (w.n_tbm <= 0 && n_kept[j] != 0) || (n_kept[j] > 0 && (!kept || w.N < 1)))
            return fail(c, L3D_ERR_INVALID, "collect_candidates: an earlier view's sizes are out of range, or a view that was never verified has records");
        for (int i = 0; i < n_kept[j]; ++i)
            if (kept[n_rec + (size_t)i].segID1 >= (unsigned)w.S_src) return fail(c, L3D_ERR_INVALID, "collect_candidates: a record's segment is past its view's");
        n_rec += (size_t)n_kept[j];
        if (w.n_tbm > 0) rt_ints += (((size_t)w.N + 1) * w.S_src + 3) & ~(size_t)3;
        maxS = std::max(maxS, w.S_src); maxN = std::max(maxN, w.N);
    }
    if (n_rec >= (1u << 30)) return fail(c, L3D_ERR_INVALID, "collect_candidates: too many records");
    const size_t nrow = (size_t)S * N;
    for (size_t row = 0; row < nrow; ++row) {
        const bool tbm = is_tbm[row % (size_t)N] != 0;
        if (rowcnt[row] < 0 || (!tbm && rowcnt[row] != 0)) return fail(c, L3D_ERR_INVALID, "collect_candidates: a stage-1 count below 0, or above 0 for a camera that is not to be matched");
        if (tbm && (rowA[row] < 0 || (long long)rowA[row] + rowcnt[row] > n_A)) return fail(c, L3D_ERR_INVALID, "collect_candidates: a stage-1 row outside the stage-1 candidates");
    }
    sel->kernels = 0; sel->g = sel->bps = sel->blocks_move = sel->R = 0;

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipGetLastError();
    struct OptionsBack { l3d_ctx* c; Options o; ~OptionsBack() { c->opt = o; } } back{ c, c->opt };
    c->opt.rt_g = sel->rt_g;
    const size_t cap = (size_t)sel->cand_cap, ccap = std::max<size_t>(cap, 1);
    // ---- the earlier views' lists where a chain leaves them
    HIPCHK(c, c->ch_kept.reserve(n_rec * sizeof(Match) + 64)); HIPCHK(c, c->ch_keptcam.reserve(n_rec * 4 + 64));
    HIPCHK(c, c->ch_rt.reserve(rt_ints * 4 + 64)); HIPCHK(c, c->ch_res.reserve((size_t)n_views * sizeof(ChainResult) + 16));
    if (n_rec) HIPCHK(c, hipMemcpyAsync(c->ch_kept.p, kept, n_rec * sizeof(Match), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(c->ch_keptcam.p, 0xff, n_rec * 4 + 64, st));
    HIPCHK(c, hipMemsetAsync(c->ch_rt.p, 0xff, rt_ints * 4 + 64, st));
    std::vector<ChainResult> res((size_t)n_views);
    std::vector<const int*> rts((size_t)n_views, nullptr);
    std::vector<RtJob> jobs;
    std::vector<const unsigned*> l2g;
    {
        size_t ro = 0, to = 0;
        for (int j = 0; j < n_views; ++j) {
            ChainResult& r = res[(size_t)j];
            memset(&r, 0, sizeof(r));
            if (j >= k) continue;
            const l3d_chain_view& w = views[j];
            const bool over = sel->overflowed && sel->overflowed[j];
            r.kept_base = ro; r.n_kept = over ? 0 : n_kept[j]; r.overflow = over ? 2 : 0; r.n_want = over ? n_kept[j] : 0;
            if (w.n_tbm > 0) {
                rts[(size_t)j] = c->ch_rt.as<int>() + to;
                if (n_kept[j] > 0) {        // (an overflowed view's tables too: stale ones are what a chain would hold -- its n_kept = 0 must keep every reader out)
                    RtJob jb;
                    memset(&jb, 0, sizeof(jb));
                    jb.recs = c->ch_kept.as<Match>() + ro; jb.qt = c->ch_keptcam.as<unsigned>() + ro; jb.rt = c->ch_rt.as<int>() + to; jb.n = n_kept[j]; jb.S = w.S_src; jb.N = w.N;
                    jobs.push_back(jb); l2g.push_back(w.local2global);
                } else if (w.S_src > 0) HIPCHK(c, hipMemsetAsync(c->ch_rt.as<int>() + to, 0, ((size_t)w.N + 1) * w.S_src * 4, st));     // (an empty list: every run starts and ends at 0)
                to += (((size_t)w.N + 1) * w.S_src + 3) & ~(size_t)3;
            }
            ro += (size_t)n_kept[j];
        }
    }
    int bad = 0;
    if (int rc = rebuild_run_tables(c, jobs, l2g, st, &bad)) return rc;
    if (bad) return fail(c, L3D_ERR_INVALID, "collect_candidates: a list is not in (segment, camera) order or names a camera that is no neighbour");
    HIPCHK(c, hipMemcpyAsync(c->ch_res.p, res.data(), res.size() * sizeof(ChainResult), hipMemcpyHostToDevice, st));
    if (int rc = upload_rtinfo(c, views, n_views, rts, maxS, maxN, st)) return rc;
    // ---- view k: its tables (cameras to be matched | source cameras | source views | its slot in each source's list), stage-1 rows and counts
    std::vector<int> tab;
    tab.insert(tab.end(), v.to_be_matched, v.to_be_matched + v.n_tbm);
    const size_t o_sc = tab.size();
    if (v.n_sources) tab.insert(tab.end(), v.source_cam, v.source_cam + v.n_sources);
    const size_t o_si = tab.size();
    if (v.n_sources) tab.insert(tab.end(), v.source_index, v.source_index + v.n_sources);
    const size_t o_ss = tab.size();
    for (int q = 0; q < v.n_sources; ++q) tab.push_back(chain_source_slot(views, v, q));
    HIPCHK(c, c->tables.reserve(tab.size() * 4 + 16));
    HIPCHK(c, hipMemcpyAsync(c->tables.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    const int* dt = c->tables.as<int>();
    ChainLayout L;
    L.maxS = S; L.maxN = N;
    if (int rc = chain_reserve_candidates(c, L, ccap, 0)) return rc;
    HIPCHK(c, c->rowcnt.reserve(nrow * 4 + 16)); HIPCHK(c, c->ch_rowA.reserve(nrow * 4 + 16));
    HIPCHK(c, c->ch_ringA_meta.reserve((size_t)std::max(n_A, 1) * 8)); HIPCHK(c, c->ch_ringA_depths.reserve((size_t)std::max(n_A, 1) * 16));
    HIPCHK(c, c->row_start.reserve((nrow + 1) * 4)); HIPCHK(c, c->ch_cursor.reserve(nrow * 4 + 16)); HIPCHK(c, c->ch_segorder.reserve((size_t)S * 4 + 16));
    if (nrow) {
        HIPCHK(c, hipMemcpyAsync(c->rowcnt.p, rowcnt, nrow * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->ch_rowA.p, rowA, nrow * 4, hipMemcpyHostToDevice, st));
    }
    if (n_A) {
        HIPCHK(c, hipMemcpyAsync(c->ch_ringA_meta.p, metaA, (size_t)n_A * 8, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->ch_ringA_depths.p, depthsA, (size_t)n_A * 16, hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipMemsetAsync(c->row_start.p, 0xff, (nrow + 1) * 4, st));
    HIPCHK(c, hipMemsetAsync(c->ch_cursor.p, 0xff, nrow * 4 + 16, st));
    HIPCHK(c, hipMemsetAsync(c->ch_segorder.p, 0xff, (size_t)S * 4 + 16, st));
    HIPCHK(c, hipMemsetAsync(c->cand_meta.p, 0xff, ccap * 8, st));
    HIPCHK(c, hipMemsetAsync(c->cand_depths.p, 0xff, ccap * 16, st));

    CollectRule rule = chain_collect_rule(c->opt, true, sel->avg_kept, S, N, maxS);
    rule.rt = sel->route == 1;                          // (the route is the caller's; everything else the chain's rule)
    CollectIn ci;
    ci.arena = c->ch_kept.as<Match>(); ci.dres = c->ch_res.as<ChainResult>(); ci.cams = c->ch_keptcam.as<unsigned>(); ci.info = c->ch_rtinfo.as<RtInfo>();
    ci.d_tbm = dt; ci.d_sc = dt + o_sc; ci.d_si = dt + o_si; ci.d_ss = dt + o_ss; ci.n_sources = v.n_sources; ci.n_tbm = v.n_tbm; ci.view_id = v.view_id; ci.S = S; ci.N = N;
    ci.rowcnt = c->rowcnt.as<int>(); ci.rowA = c->ch_rowA.as<int>(); ci.metaA = c->ch_ringA_meta.as<uint2>(); ci.depthsA = c->ch_ringA_depths.as<float4>();
    ci.cand_cap = cap; ci.sort_apart = sel->sort_apart != 0;
    t_collect_launched = 0;
    enqueue_collect(c, ci, rule, st);
    sel->kernels = t_collect_launched; sel->g = rule.rt_g; sel->bps = rule.rt ? rule.rt_bps : rule.bps; sel->blocks_move = (S * v.n_tbm + 3) / 4;
    HIPCHK(c, hipMemcpyAsync(row_start, c->row_start.p, (nrow + 1) * 4, hipMemcpyDeviceToHost, st));
    if (nrow) HIPCHK(c, hipMemcpyAsync(cursor, c->ch_cursor.p, nrow * 4, hipMemcpyDeviceToHost, st));
    if (S) HIPCHK(c, hipMemcpyAsync(seg_order, c->ch_segorder.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    if (cap) {
        HIPCHK(c, hipMemcpyAsync(cand_meta, c->cand_meta.p, cap * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(cand_depths, c->cand_depths.p, cap * 16, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    sel->R = row_start[nrow];
    return L3D_OK;
}

// The kept writers and the rebuild of side words and run tables on one view's candidates of the caller's (tests/test_gpu_kept_write.py): everything is
// validated on the host, the arena and every output are filled with 0xff bytes, then the product's launchers run -- launch_kept_write_chain, or
// launch_scan + launch_kept_write, and rebuild_run_tables (what run_chain calls for lists taken over).
extern "C" int l3d_test_kept_write(l3d_ctx* c, int S, int N, const int32_t* row_start, const uint32_t* cand_meta, const float* cand_depths, const float* cand_conf,
                                   const int32_t* kept_cnt, const uint32_t* local2global, l3d_test_kept_path* sel, l3d_match* records, uint32_t* side, int32_t* rt,
                                   int32_t* best_pos)
{
    if (!c) return L3D_ERR_INVALID;
    if (!sel || S < 0 || N < 1 || N > 255 || !row_start || !local2global || (S > 0 && !kept_cnt) || (sel->writer != 0 && sel->writer != 1) || sel->n_jobs < 0 ||
        (sel->n_jobs > 0 && !sel->jobs) || sel->cand_cap < 0 || (sel->has_prev && sel->prev_n_kept < 0))
        return fail(c, L3D_ERR_INVALID, "kept_write: bad argument");
    if ((long long)S * (N + 1) >= 0x7fffffffll || sel->arena_cap >= (1ull << 31) || (sel->has_prev && sel->prev_base >= (1ull << 40))) return fail(c, L3D_ERR_INVALID, "kept_write: too many rows or records");
    const size_t nrow = (size_t)S * N, acap = (size_t)sel->arena_cap;
    if (sel->writer == 0 && S > 0 && (!side || !rt || !best_pos)) return fail(c, L3D_ERR_INVALID, "kept_write: the chain's writer needs side, rt and best_pos");
    if (acap > 0 && (!records || (sel->writer == 0 && !side))) return fail(c, L3D_ERR_INVALID, "kept_write: no room for the arena");
    if (row_start[0] != 0) return fail(c, L3D_ERR_INVALID, "kept_write: row_start must start at 0");
    for (size_t i = 0; i < nrow; ++i) if (row_start[i + 1] < row_start[i]) return fail(c, L3D_ERR_INVALID, "kept_write: row_start does not ascend");
    const int R = row_start[nrow];
    if (R > 0 && (!cand_meta || !cand_depths || !cand_conf)) return fail(c, L3D_ERR_INVALID, "kept_write: candidates missing");
    long long total = 0;
    for (int y = 0; y < S; ++y) {
        int kept = 0;
        for (int q = 0; q < N; ++q)
            for (int r = row_start[(size_t)y * N + q]; r < row_start[(size_t)y * N + q + 1]; ++r) {
                if (cand_meta[2 * (size_t)r + 1] != (unsigned)q) return fail(c, L3D_ERR_INVALID, "kept_write: a candidate's camera is not its row's");
                if (cand_meta[2 * (size_t)r] >= 65536u) return fail(c, L3D_ERR_INVALID, "kept_write: a target id does not fit 16 bits");
                kept += cand_conf[r] > 1.0f ? 1 : 0;
            }
        if (kept_cnt[y] != kept) return fail(c, L3D_ERR_INVALID, "kept_write: kept_cnt of segment " + std::to_string(y) + " is not its count of confidences above 1");
        total += kept;
    }
    if (sel->writer == 1 && (unsigned long long)total > sel->arena_cap) return fail(c, L3D_ERR_INVALID, "kept_write: the seam writer needs room for " + std::to_string(total) + " records");
    size_t job_recs = 0, job_cells = 0;
    for (int i = 0; i < sel->n_jobs; ++i) {
        const l3d_test_kept_job& j = sel->jobs[i];
        if (!j.records) { if (sel->writer != 0) return fail(c, L3D_ERR_INVALID, "kept_write: only the chain's writer leaves a list to rebuild"); job_recs += (size_t)total; job_cells += (size_t)(N + 1) * S; continue; }
        if (j.n < 0 || j.S < 0 || j.N < 1 || j.N > 255 || !j.local2global || (long long)j.S * (j.N + 1) >= 0x7fffffffll || (j.n > 0 && !j.qt) || (j.S > 0 && !j.rt))
            return fail(c, L3D_ERR_INVALID, "kept_write: bad rebuild job");
        job_recs += (size_t)j.n; job_cells += (size_t)(j.N + 1) * j.S;
    }
    sel->n_kept = sel->R = sel->overflow = sel->n_want = sel->rebuild_err = sel->rebuild_blocks = 0; sel->kept_base = 0;

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipGetLastError();
    const size_t rcap = (size_t)std::max(R, 1);
    HIPCHK(c, c->row_start.reserve((nrow + 1) * 4));
    HIPCHK(c, c->cand_meta.reserve(rcap * 8)); HIPCHK(c, c->cand_depths.reserve(rcap * 16)); HIPCHK(c, c->cand_conf.reserve(rcap * 4));
    HIPCHK(c, c->kept_cnt.reserve((size_t)S * 4 + 4)); HIPCHK(c, c->kept_start.reserve((size_t)S * 4 + 8));
    HIPCHK(c, c->l2g.reserve((size_t)N * 4));
    HIPCHK(c, c->ch_kept.reserve(acap * sizeof(Match) + 64)); HIPCHK(c, c->ch_keptcam.reserve(acap * 4 + 64));
    HIPCHK(c, c->ch_rt.reserve((size_t)(N + 1) * S * 4 + 64)); HIPCHK(c, c->ch_bestpos.reserve((size_t)S * 4 + 64));
    HIPCHK(c, c->ch_res.reserve(2 * sizeof(ChainResult))); HIPCHK(c, c->ch_pin_res.reserve(sizeof(ChainResult)));
    HIPCHK(c, hipMemcpyAsync(c->row_start.p, row_start, (nrow + 1) * 4, hipMemcpyHostToDevice, st));
    if (R) {
        HIPCHK(c, hipMemcpyAsync(c->cand_meta.p, cand_meta, (size_t)R * 8, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->cand_depths.p, cand_depths, (size_t)R * 16, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->cand_conf.p, cand_conf, (size_t)R * 4, hipMemcpyHostToDevice, st));
    }
    if (S) HIPCHK(c, hipMemcpyAsync(c->kept_cnt.p, kept_cnt, (size_t)S * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->l2g.p, local2global, (size_t)N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(c->ch_kept.p, 0xff, acap * sizeof(Match) + 64, st));
    HIPCHK(c, hipMemsetAsync(c->ch_keptcam.p, 0xff, acap * 4 + 64, st));
    HIPCHK(c, hipMemsetAsync(c->ch_rt.p, 0xff, (size_t)(N + 1) * S * 4 + 64, st));
    HIPCHK(c, hipMemsetAsync(c->ch_bestpos.p, 0x7f, (size_t)S * 4 + 64, st));          // (-1 is an answer of the writer's: no kept match)
    ChainResult* dres = c->ch_res.as<ChainResult>();
    ChainResult* hres = c->ch_pin_res.as<ChainResult>();
    ChainResult prev;
    prev.kept_base = sel->prev_base; prev.n_kept = sel->prev_n_kept; prev.R = 0; prev.overflow = 0; prev.n_want = 0;
    HIPCHK(c, hipMemsetAsync(dres, 0xff, 2 * sizeof(ChainResult), st));
    if (sel->has_prev) HIPCHK(c, hipMemcpyAsync(dres, &prev, sizeof(ChainResult), hipMemcpyHostToDevice, st));
    memset(hres, 0xff, sizeof(ChainResult));
    ChainResult* hres_dev = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&hres_dev), hres, 0));

    VerifyArgs va;
    memset(&va, 0, sizeof(va));
    va.row_start = c->row_start.as<int>(); va.cand_meta = c->cand_meta.as<uint2>(); va.cand_depths = c->cand_depths.as<float4>(); va.cand_conf = c->cand_conf.as<float>();
    va.N = N; va.seg_begin = 0; va.seg_end = S; va.nrow_total = (int)nrow; va.cand_cap = sel->cand_cap; va.only_above = -1;
    ChainResult got;
    memset(&got, 0, sizeof(got));
    if (sel->writer == 0) {
        ProfScope p(c, "kept_write");
        launch_kept_write_chain(va, c->kept_cnt.as<int>(), (int)nrow, sel->has_prev ? dres : nullptr, (unsigned long long)sel->arena_cap, dres + 1, hres_dev, c->l2g.as<unsigned>(),
                                c->ch_kept.as<Match>(), st, c->ch_bestpos.as<int>(), c->ch_keptcam.as<unsigned>(), c->ch_rt.as<int>(), S);
    } else {
        { ProfScope p(c, "scan"); launch_scan(c->kept_cnt.as<int>(), c->kept_start.as<int>(), S, nullptr, st); }
        { ProfScope p(c, "kept_write"); launch_kept_write(va, c->kept_start.as<int>(), c->l2g.as<unsigned>(), c->ch_kept.as<Match>(), st); }
    }
    if (sel->writer == 0) HIPCHK(c, hipMemcpyAsync(&got, dres + 1, sizeof(ChainResult), hipMemcpyDeviceToHost, st));
    else HIPCHK(c, hipMemcpyAsync(&got.n_kept, c->kept_start.as<int>() + S, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (sel->writer == 0 && memcmp(&got, hres, sizeof(ChainResult)) != 0) return fail(c, L3D_ERR_INVALID, "kept_write: the device and the host-mapped result record differ");
    if (sel->writer == 1) got.R = R;
    sel->kept_base = got.kept_base; sel->n_kept = got.n_kept; sel->R = got.R; sel->overflow = got.overflow; sel->n_want = got.n_want;
    if (acap) HIPCHK(c, hipMemcpyAsync(records, c->ch_kept.p, acap * sizeof(Match), hipMemcpyDeviceToHost, st));
    if (acap && side) HIPCHK(c, hipMemcpyAsync(side, c->ch_keptcam.p, acap * 4, hipMemcpyDeviceToHost, st));
    if (S && rt) HIPCHK(c, hipMemcpyAsync(rt, c->ch_rt.p, (size_t)(N + 1) * S * 4, hipMemcpyDeviceToHost, st));
    if (S && best_pos) HIPCHK(c, hipMemcpyAsync(best_pos, c->ch_bestpos.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));

    if (sel->n_jobs > 0) {
        // crafted records | every job's side words | every job's run table: apart from what the writer left
        HIPCHK(c, c->g0.reserve(job_recs * sizeof(Match) + 64)); HIPCHK(c, c->g1.reserve(job_recs * 4 + 64)); HIPCHK(c, c->g2.reserve(job_cells * 4 + 64));
        HIPCHK(c, hipMemsetAsync(c->g1.p, 0xff, job_recs * 4 + 64, st));
        HIPCHK(c, hipMemsetAsync(c->g2.p, 0xff, job_cells * 4 + 64, st));
        std::vector<RtJob> jobs((size_t)sel->n_jobs);
        std::vector<const unsigned*> l2g((size_t)sel->n_jobs);
        size_t ro = 0, co = 0;
        for (int i = 0; i < sel->n_jobs; ++i) {
            l3d_test_kept_job& tj = sel->jobs[i];
            RtJob& j = jobs[(size_t)i];
            memset(&j, 0, sizeof(j));
            if (!tj.records) {
                tj.n = got.n_kept; tj.S = S; tj.N = N;
                j.recs = c->ch_kept.as<Match>() + got.kept_base; l2g[(size_t)i] = local2global;
            } else {
                j.recs = c->g0.as<Match>() + ro; l2g[(size_t)i] = tj.local2global;
                if (tj.n) HIPCHK(c, hipMemcpyAsync(c->g0.as<Match>() + ro, tj.records, (size_t)tj.n * sizeof(Match), hipMemcpyHostToDevice, st));
            }
            j.qt = c->g1.as<unsigned>() + ro; j.rt = c->g2.as<int>() + co; j.n = tj.n; j.S = tj.S; j.N = tj.N;
            ro += (size_t)tj.n; co += (size_t)(tj.N + 1) * tj.S;
        }
        int bad = 0, max_n = 0;
        if (int rc = rebuild_run_tables(c, jobs, l2g, st, &bad, &max_n)) return rc;
        HIPCHK(c, hipGetLastError());
        sel->rebuild_err = bad; sel->rebuild_blocks = max_n > 0 ? qt_from_records_blocks(max_n) : 0;
        for (int i = 0; i < sel->n_jobs; ++i) {
            const l3d_test_kept_job& tj = sel->jobs[i];
            const RtJob& j = jobs[(size_t)i];
            if (tj.n && tj.qt) HIPCHK(c, hipMemcpyAsync(tj.qt, j.qt, (size_t)tj.n * 4, hipMemcpyDeviceToHost, st));
            if (tj.S && tj.rt) HIPCHK(c, hipMemcpyAsync(tj.rt, j.rt, (size_t)(tj.N + 1) * tj.S * 4, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(c, hipStreamSynchronize(st));
    }
    HIPCHK(c, hipGetLastError());
    return L3D_OK;
}

void l3d::warm_chain() { touch_kernel(reinterpret_cast<const void*>(&k_exist_count)); }
