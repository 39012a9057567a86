// l3d_chain_sharded.hip -- the resident matchViews chain (l3d_chain.hip) with every view's SOURCE segments sharded over
// the GPUs of one node.
//
// matchViews is a dependency chain over views, so views are not distributed.  Each rank (one process per GPU) runs the
// chain on its source-segment range [S*r/W, S*(r+1)/W) of every view: stage 1 and the verification of a source segment
// only touch that segment's rows, so the ranges are independent and need no exchange.  The single exchange per view
// is its kept list: a later view pulls its reverse matches (line3D.cc:838-872) from ALL ranks' kept records, so after a
// view's kept records are written into this rank's fixed-size SLOT the caller all-gathers the slots of that view
// (RCCL over xGMI, `torch.distributed.all_gather_into_tensor` on this context's stream, see
// line3d_amd/distributed.py).  Nothing waits for the host: the library only enqueues (l3d_shard_chain_enqueue), the
// framework enqueues the collective on the same stream, the host trails behind on events (l3d_shard_chain_fetch).
// The concatenation of the ranks' kept lists in rank order is the sorted list of the unsharded run, bit for bit.
//
// slot layout: [SlotHeader 32 B][best depth pairs float2 x seg_cap][position of every segment's best kept match int x seg_cap][kept records
// l3d_match x slot_records]
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "l3d_ctx.hpp"
#include "l3d_scan.hpp"
#include "l3d_kept.hpp"
#include "l3d_chain_common.hpp"
#include "l3d_products.hpp"
#include "l3d_shard_rule.hpp"

using namespace l3d;

// Host-side waits of the enqueue threads: yield for a while, then sleep -- a thread that is far ahead (the stage-1 thread
// almost always is) must not burn a core of a CPU-quota'd container shared by eight ranks.
template <class Pred>
static inline void wait_until(Pred pred, int spins_before_sleep)
{
    int spins = 0;
    while (!pred()) {
        if (++spins < spins_before_sleep) std::this_thread::yield();
        else { const int us = tunables().wait_sleep_us.load(std::memory_order_relaxed); if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us)); else std::this_thread::yield(); }
    }
}

namespace l3d {

struct SlotHeader { int n_kept, R, overflow, s0, s1, pad[3]; };
static_assert(sizeof(SlotHeader) == kShardSlotHeaderBytes && sizeof(Match) == kShardRecordBytes, "slot header, kept record (SlotGeom: l3d_shard_rule.hpp)");

// reverse matches for view `view_id`, source-segment range [s0,s1), out of the gathered slots of earlier views
// (blockIdx.y = source * world + rank)
__global__ void k_exist_count_slots(const unsigned char* __restrict__ G, SlotGeom g, const int* __restrict__ src_index,
                                    const int* __restrict__ src_cam, const int* __restrict__ src_slot, unsigned view_id, int N, int s0, int s1, int* __restrict__ rowcnt)
{
    const int src = blockIdx.y / g.world, r = blockIdx.y % g.world;
    const unsigned char* slot = G + ((size_t)(src_index[src] % g.ring) * g.world + r) * g.slot_bytes;
    const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(slot);
    const int n = hd->overflow ? 0 : hd->n_kept;
    const Match* kept = reinterpret_cast<const Match*>(slot + g.rec_off);
    // side array (dense scenes): (the record's LOCAL camera << 16 | its target segment) -- camera and segment range are decided on 4 bytes, the count reads no
    // record (round 5: the global camera id; the 1 record in N that matched was read, 7 in 8 of those for another rank's range)
    const unsigned* side = g.cam_off ? reinterpret_cast<const unsigned*>(slot + g.cam_off) : nullptr;
    const int cam = src_cam[src];
    if (src_slot[src] < 0) return;                              // (this view is not among the source's neighbours: no record of it points here)
    const unsigned want = (unsigned)src_slot[src];
    const int stride = gridDim.x * blockDim.x;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (side) {                                                 // (a slot with side words has a run table, and a neighbour's local number is a row of it: slot_geometry)
        if (n <= 0) return;                                     // (an overflowed slot holds no records and no run table)
        // run tables: the runs of this view's camera in the rank's slot, sixteen lanes per run
        const int* rt = reinterpret_cast<const int*>(slot + g.rt_off);
        const int* r0 = rt + (size_t)want * g.seg_cap;
        const int* r1 = r0 + g.seg_cap;
        const int nsl = hd->s1 - hd->s0;
        const int grp = i >> 4, gl = i & 15, ngrp = stride >> 4;
        for (int sl = grp; sl < nsl; sl += ngrp) {
            const int a = r0[sl], b = r1[sl];
            for (int k = a + gl; k < b; k += 16) { const unsigned w = side[k]; const int u = (int)(w & 0xffffu); if (u >= s0 && u < s1) atomicAdd(&rowcnt[u * N + cam], 1); }
        }
        return;
    }
    for (; i < n; i += stride) {
        const Match m = kept[i];
        if (m.camID2 == view_id && (int)m.segID2 >= s0 && (int)m.segID2 < s1) atomicAdd(&rowcnt[m.segID2 * N + cam], 1);
    }
}

// Both writers of the combined candidate arrays in one launch (they are independent: stage-1 candidates go to the rows of the
// cameras to be matched, reverse matches to the rows of the source cameras): the first `blocks_move` workgroups copy the
// stage-1 candidates of the rank's rows (a wave per row), the others scatter the reverse matches
// (k_exist_scatter_slots, wps workgroups per (source view, rank) list).
__global__ __launch_bounds__(256) void k_place_slots(int blocks_move, int wps, const int* __restrict__ tbm, int n_tbm, const int* __restrict__ rowA,
                                                     const uint2* __restrict__ metaA, const float4* __restrict__ depthsA,
                                                     const unsigned char* __restrict__ G, SlotGeom g, const int* __restrict__ src_index,
                                                     const int* __restrict__ src_cam, const int* __restrict__ src_slot, unsigned view_id, int N, int S, int s0, int s1,
                                                     const int* __restrict__ row_start, int* __restrict__ cursor,
                                                     uint2* __restrict__ meta, float4* __restrict__ depths, int cap)
{
    if (row_start[(size_t)S * N] > cap) return;                  // overflow: the chain is re-run with more room
    if ((int)blockIdx.x < blocks_move) { move_stage1_row(s0, s1, tbm, n_tbm, N, rowA, metaA, depthsA, row_start, meta, depths); return; }
    const int e = (int)blockIdx.x - blocks_move, list = e / wps, bx = e % wps;
    const int src = list / g.world, r = list % g.world;
    const unsigned char* slot = G + ((size_t)(src_index[src] % g.ring) * g.world + r) * g.slot_bytes;
    const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(slot);
    const int n = hd->overflow ? 0 : hd->n_kept;
    const Match* kept = reinterpret_cast<const Match*>(slot + g.rec_off);
    const unsigned* side = g.cam_off ? reinterpret_cast<const unsigned*>(slot + g.cam_off) : nullptr;     // (local camera << 16 | target segment): k_exist_count_slots
    const int cam = src_cam[src];
    if (src_slot[src] < 0) return;                              // (this view is not among the source's neighbours: no record of it points here)
    const unsigned want = (unsigned)src_slot[src];
    auto place = [&](int i) {
        const Match m = kept[i];
        if (m.camID2 == view_id && (int)m.segID2 >= s0 && (int)m.segID2 < s1) place_reverse_match(m, N, cam, row_start, cursor, meta, depths);
    };
    const int stride = wps * 256;
    int i = bx * 256 + (int)threadIdx.x;
    if (side) {     // run tables: k_exist_count_slots
        if (n <= 0) return;
        const int* rt = reinterpret_cast<const int*>(slot + g.rt_off);
        const int* r0 = rt + (size_t)want * g.seg_cap;
        const int* r1 = r0 + g.seg_cap;
        const int nsl = hd->s1 - hd->s0;
        const int grp = i >> 4, gl = i & 15, ngrp = stride >> 4;
        for (int sl = grp; sl < nsl; sl += ngrp) {
            const int a = r0[sl], b = r1[sl];
            for (int k = a + gl; k < b; k += 16) { const unsigned w = side[k]; const int u = (int)(w & 0xffffu); if (u >= s0 && u < s1) place(k); }
        }
        return;
    }
    for (; i < n; i += stride) place(i);
}

// Kept records of this rank's source-segment range [s0,s1) into its slot, in ONE launch behind the verification (every
// launch of the sharded chain sits on the per-view critical path): each workgroup (one segment) sums the kept counts in
// front of its segment itself -- a few hundred to 2000 ints out of L2 -- instead of waiting for a scan launch;
// workgroup 0 also writes the slot header (count, #candidates, overflow).  kept_cnt points at the range's first segment.
__global__ __launch_bounds__(256) void k_slot_write(VerifyArgs a, const int* __restrict__ kept_cnt, int nrow, int slot_records,
                                                    const unsigned* __restrict__ local2global, const float2* __restrict__ best, SlotGeom g,
                                                    unsigned char* __restrict__ slot)
{
    __shared__ int s_red[8];
    __shared__ int s_cnt[32];
    __shared__ int s_qcnt[256];
    __shared__ unsigned long long s_best[4];
    const int tid = threadIdx.x;
    const int nseg = a.seg_end - a.seg_begin;
    const int yl = blockIdx.x;
    int before, total;
    kept_before_total(kept_cnt, nseg, yl, s_red, before, total);
    SlotHeader h;
    h.R = a.row_start[nrow];
    h.overflow = h.R > a.cand_cap ? 1 : 0;
    h.n_kept = h.overflow ? 0 : total;
    if (h.n_kept > slot_records) { h.overflow |= 2; h.n_kept = 0; }
    h.s0 = a.seg_begin; h.s1 = a.seg_end; h.pad[0] = total; h.pad[1] = h.pad[2] = 0;      // pad[0]: the kept count even when it did not fit
    if (blockIdx.x == 0 && tid == 0) *reinterpret_cast<SlotHeader*>(slot) = h;
    if (yl >= nseg) return;                                  // (an empty range still launches workgroup 0 for the header)
    const int y = a.seg_begin + yl;
    if (tid == 0) reinterpret_cast<float2*>(slot + g.best_off)[yl] = best[y];
    int* bpos = reinterpret_cast<int*>(slot + g.bpos_off) + yl;              // (position in this slot's records; -1: the segment kept nothing)
    if (h.overflow) { if (tid == 0) *bpos = -1; return; }
    // (round 6) the side array holds (local camera << 16 | target segment): a reader decides camera AND segment range on 4 bytes -- the count reads no record at all
    // the run table's rows are seg_cap apart and indexed by the segment's position in the rank's range (the writer indexes by the segment: the base is shifted)
    int* rt = g.rt_off ? reinterpret_cast<int*>(slot + g.rt_off) - a.seg_begin : nullptr;
    write_kept_segment_wg(a, y, before, local2global, reinterpret_cast<Match*>(slot + g.rec_off), s_cnt, bpos, s_best, g.cam_off ? reinterpret_cast<unsigned*>(slot + g.cam_off) : nullptr,
                          rt, g.seg_cap, s_qcnt);
}

// Hand-over of one finished view on a committing rank: the ranks' kept records, concatenated in rank (= segment) order
// behind the raw depth-pair arrays, are packed into a contiguous device staging buffer (one SDMA copy of the exact size
// brings them to the host); the summary goes straight into host-mapped pinned memory.
struct PackHeader { long long R; int n_kept, overflow, pad[4]; };
static_assert(sizeof(PackHeader) == 32, "pack header");
__global__ __launch_bounds__(256) void k_pack_view(const unsigned char* __restrict__ block, SlotGeom g, unsigned char* __restrict__ out,
                                                   PackHeader* __restrict__ hdr_host)
{
    const int r = blockIdx.y;
    int base = 0, bad = 0;
    long long R = 0;
    for (int q = 0; q < g.world; ++q) {
        const SlotHeader* hq = reinterpret_cast<const SlotHeader*>(block + (size_t)q * g.slot_bytes);
        const bool ok = !hq->overflow && hq->n_kept >= 0 && hq->n_kept <= g.slot_records;
        bad |= !ok;
        if (q < r && ok) base += hq->n_kept;
        R += hq->R;
    }
    const unsigned char* slot = block + (size_t)r * g.slot_bytes;
    const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(slot);
    const size_t best_bytes = (size_t)g.seg_cap * 8;
    unsigned char* o_best = out + (size_t)r * best_bytes;
    unsigned char* o_rec = out + (size_t)g.world * best_bytes;
    const int n = bad ? 0 : hd->n_kept;
    if (r == g.world - 1 && blockIdx.x == 0 && threadIdx.x == 0) {
        PackHeader ph;
        ph.R = R; ph.n_kept = bad ? 0 : base + n; ph.overflow = bad; ph.pad[0] = ph.pad[1] = ph.pad[2] = ph.pad[3] = 0;
        *hdr_host = ph;
    }
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    // depth pairs of this rank's segment range (fixed stride seg_cap; the host skips the -1 markers)
    const int nb = (hd->s1 - hd->s0);
    for (int i = tid; i < nb; i += nt)
        reinterpret_cast<float2*>(o_best)[i] = reinterpret_cast<const float2*>(slot + g.best_off)[i];
    const float4* src = reinterpret_cast<const float4*>(slot + g.rec_off);
    float4* dst = reinterpret_cast<float4*>(o_rec + (size_t)base * sizeof(Match));
    for (int i = tid; i < 2 * n; i += nt) dst[i] = src[i];
}

// ---- matchViews' products from the gathered slots (l3d_shard_chain_products): every rank holds every view's kept records, so every
// rank can build what the single-GPU chain builds from its kept arena -- no rank hands lists to the host.
// per view: kept matches and candidates summed over the ranks' slots
// (hdr, hdr_stride: the slot headers where they are -- in front of every slot of the gathered blocks, or the compact header table the ring
// mode keeps)
__global__ void k_shard_totals(const unsigned char* __restrict__ hdr, size_t hdr_stride, SlotGeom g, const unsigned char* __restrict__ verified, int n_views, int2* __restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_views) return;
    int n = 0; long long R = 0;
    if (verified[k])
        for (int r = 0; r < g.world; ++r) {
            const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(hdr + ((size_t)k * g.world + r) * hdr_stride);
            n += hd->overflow ? 0 : hd->n_kept; R += hd->R;
        }
    out[k] = make_int2(n, (int)min(R, 0x7fffffffll));
}
// all views' slots -> ONE kept arena (views back to back, ranks in segment order: the sorted list of the unsharded run) + the whole
// view's best depth pairs and best positions (relative to the view's slice).  grid (x, rank, view).
__global__ __launch_bounds__(256) void k_shard_pack_all(const unsigned char* __restrict__ G, SlotGeom g, const unsigned char* __restrict__ verified,
                                                        const unsigned long long* __restrict__ kept_base, const long long* __restrict__ best_off, Match* __restrict__ arena,
                                                        float2* __restrict__ best_all, int* __restrict__ bestpos_all)
{
    const int k = blockIdx.z, r = blockIdx.y;
    if (!verified[k]) return;
    const unsigned char* block = G + (size_t)k * g.world * g.slot_bytes;
    int base = 0;
    for (int q = 0; q < r; ++q) { const SlotHeader* hq = reinterpret_cast<const SlotHeader*>(block + (size_t)q * g.slot_bytes); base += hq->overflow ? 0 : hq->n_kept; }
    const unsigned char* slot = block + (size_t)r * g.slot_bytes;
    const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(slot);
    const int n = hd->overflow ? 0 : hd->n_kept;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    const float4* src = reinterpret_cast<const float4*>(slot + g.rec_off);
    float4* dst = reinterpret_cast<float4*>(arena + kept_base[k] + base);
    for (int i = tid; i < 2 * n; i += nt) dst[i] = src[i];
    const float2* sb = reinterpret_cast<const float2*>(slot + g.best_off);
    const int* sp = reinterpret_cast<const int*>(slot + g.bpos_off);
    for (int i = tid; i < hd->s1 - hd->s0; i += nt) {
        const long long o = best_off[k] + hd->s0 + i;
        best_all[o] = sb[i];
        const int p = sp[i];
        bestpos_all[o] = p < 0 || n == 0 ? -1 : base + p;
    }
}

// Ring mode (l3d_shard_chain_run when the gathered blocks of all views would not fit a budget: 2048 views x 8 ranks x 3.8 MB slots = 63 GB at
// 4000 segments x 24 neighbours): the gathered buffer holds only the views later views still read (the neighbour window of the schedule);
// older blocks are RETIRED a batch at a time -- their used records into the compact kept arena in the order of the unsharded run (what
// k_shard_pack_all does for all views at the end), their headers into a small table for the shared verdict -- before their ring block is
// overwritten.  grid (x, rank, view of the batch).  base_dev[k]: the arena offset of view k (running sum kept on the device: the host never
// learns a count on the way); the block of the batch's last view publishes the offset of the next batch.
// keep (partitioned job, l3d_shard_chain_partition; null: every view): a view that is not flagged leaves its headers in the table (the shared
// verdict reads them) and nothing in this rank's arena.
__global__ __launch_bounds__(256) void k_shard_retire(const unsigned char* __restrict__ G, SlotGeom g, const unsigned char* __restrict__ verified, const unsigned char* __restrict__ keep, int k0, int n_batch,
                                                      long long* __restrict__ base_dev, long long arena_cap, const long long* __restrict__ best_off, Match* __restrict__ arena,
                                                      float2* __restrict__ best_all, int* __restrict__ bestpos_all, SlotHeader* __restrict__ hdr_all, int* __restrict__ overflow,
                                                      unsigned* __restrict__ qt_arena, int* __restrict__ rt_all, const long long* __restrict__ rt_off, const int2* __restrict__ view_sn)
{
    const int k = k0 + blockIdx.z, r = blockIdx.y;
    long long base = base_dev[k0];
    for (int q = k0; q < k; ++q) {
        if (!verified[q] || (keep && !keep[q])) continue;
        const unsigned char* bq = G + (size_t)(q % g.ring) * g.world * g.slot_bytes;
        for (int w = 0; w < g.world; ++w) { const SlotHeader* hq = reinterpret_cast<const SlotHeader*>(bq + (size_t)w * g.slot_bytes); base += hq->overflow ? 0 : hq->n_kept; }
    }
    const unsigned char* block = G + (size_t)(k % g.ring) * g.world * g.slot_bytes;
    const bool kept_here = !keep || keep[k];
    int in_front = 0, all = 0;
    if (verified[k] && kept_here)
        for (int w = 0; w < g.world; ++w) {
            const SlotHeader* hq = reinterpret_cast<const SlotHeader*>(block + (size_t)w * g.slot_bytes);
            const int n = hq->overflow ? 0 : hq->n_kept;
            if (w < r) in_front += n;
            all += n;
        }
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first && r == 0) base_dev[k] = base;                                          // (k0 itself: rewritten with the same value)
    if (first && r == 0 && (int)blockIdx.z == n_batch - 1) base_dev[k + 1] = base + all;
    SlotHeader* ho = hdr_all + (size_t)k * g.world + r;
    if (!verified[k]) { if (first) { SlotHeader z; z.n_kept = z.R = z.overflow = z.s0 = z.s1 = 0; z.pad[0] = z.pad[1] = z.pad[2] = 0; *ho = z; } return; }
    const unsigned char* slot = block + (size_t)r * g.slot_bytes;
    const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(slot);
    if (first) *ho = *hd;
    if (!kept_here) return;
    const int n = hd->overflow ? 0 : hd->n_kept;
    if (base + all > arena_cap) { if (first) atomicMax(overflow, 1); return; }      // the arena's first guess was too small: the run ends with a capacity verdict
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    const float4* src = reinterpret_cast<const float4*>(slot + g.rec_off);
    float4* dst = reinterpret_cast<float4*>(arena + base + in_front);
    for (int i = tid; i < 2 * n; i += nt) dst[i] = src[i];
    const float2* sb = reinterpret_cast<const float2*>(slot + g.best_off);
    const int* sp = reinterpret_cast<const int*>(slot + g.bpos_off);
    for (int i = tid; i < hd->s1 - hd->s0; i += nt) {
        const long long o = best_off[k] + hd->s0 + i;
        best_all[o] = sb[i];
        const int p = sp[i];
        bestpos_all[o] = p < 0 || n == 0 ? -1 : in_front + p;
    }
    // (round 6) the slot's side words and run table travel with its records: the view's (local camera << 16 | target) array and its run table, (N + 1) x S with
    // positions counted from the view's first record -- what the single-GPU chain's kept writer leaves, so the products transpose without rebuilding either
    if (qt_arena) {
        const unsigned* sq = reinterpret_cast<const unsigned*>(slot + g.cam_off);
        unsigned* dq = qt_arena + base + in_front;
        for (int i = tid; i < n; i += nt) dq[i] = sq[i];
        const int S = view_sn[k].x, N = view_sn[k].y, ns = hd->s1 - hd->s0;
        int* rt = rt_all + rt_off[k];
        const int* srt = reinterpret_cast<const int*>(slot + g.rt_off);
        for (int i = tid; i < (N + 1) * ns; i += nt) {
            const int q = i / ns, j = i - q * ns;
            rt[(size_t)q * S + hd->s0 + j] = in_front + (n > 0 ? srt[(size_t)q * g.seg_cap + j] : 0);
        }
    }
}

// After the last exchange: the OR of the overflow bits of every gathered slot header (1 candidate capacity, 2 slot records,
// 4 a rank gave up) and, for sizing a retry, the largest candidate / kept count any rank reported.  Every rank holds the same
// gathered blocks, so every rank computes the same answer: the ranks agree on the outcome without another collective.
__global__ void k_check_slots(const unsigned char* __restrict__ hdr, size_t hdr_stride, SlotGeom g, const unsigned char* __restrict__ verified, int n_views, int* __restrict__ out3)
{
    int bits = 0, maxR = 0, maxK = 0;
    const int n = n_views * g.world;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (!verified[i / g.world]) continue;
        const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(hdr + (size_t)i * hdr_stride);
        bits |= hd->overflow & 7;
        maxR = max(maxR, hd->R);
        maxK = max(maxK, hd->pad[0]);
    }
    for (int o = 32; o > 0; o >>= 1) { bits |= __shfl_down(bits, o); maxR = max(maxR, __shfl_down(maxR, o)); maxK = max(maxK, __shfl_down(maxK, o)); }
    if ((threadIdx.x & 63) == 0) { if (bits) atomicOr(&out3[0], bits); atomicMax(&out3[1], maxR); atomicMax(&out3[2], maxK); }
}

}  // namespace l3d

namespace {

typedef l3d::ChainViewDev SViewDev;           // (s0, s1: this rank's source-segment range)

}  // namespace

struct l3d_shard_chain {
    l3d_ctx* c = nullptr;
    const l3d_chain_view* views = nullptr;
    int n_views = 0, rank = 0, world = 1;
    SlotGeom geom;
    std::vector<SViewDev> vd;
    const unsigned char* dtab = nullptr;
    int* hstats = nullptr;
    int* hstats_dev = nullptr;
    std::vector<hipEvent_t> ev1, ev2;
    int k_p1 = 0;
    size_t cand_cap = 0;
    static constexpr int kStage1Ahead = 8, kRingA = kStage1Ahead + 2;   // ring of stage-1 candidate buffers
    int maxS = 0, maxN = 0;
    const unsigned char* gathered = nullptr;
    double pairs = 0, raw_sum = 0, kept_total = 0;
    std::vector<float> best_scratch;
    // hand-over (k_pack_view): a ring of device staging buffers, per-view summaries in host-mapped pinned memory
    static constexpr int kRing = 16;
    size_t stage_bytes = 0;
    PackHeader* hdr_host = nullptr;
    PackHeader* hdr_dev = nullptr;
    bool eager_pack = false;                 // l3d_shard_chain_run on a committing rank: pack at mark time, on the chain's stream
    std::vector<char> packed;                // per view: its pack kernel is enqueued (and covered by ev2)
    hipEvent_t ev3 = nullptr;                // lazy pack (step-wise protocol): enqueued by fetch
    std::atomic<int> marked{0};              // views [0, marked) carry their completion event
    std::atomic<int> s1_done{0};             // l3d_shard_chain_run with a stage-1 thread: views [0, s1_done) have their stage 1 enqueued
    bool s1_thread = false;
    std::atomic<int> fetched{0};             // views [0, fetched) have left their staging buffer
    int copy_issued = -1;                    // view whose D2H copy the previous fetch has already issued (fetch thread only)
    l3d_match* copy_dst = nullptr;           // ... and where its records go (pinned arena)
    double t_wait = 0, t_copy = 0, t_cb = 0, t_enq = 0, t_ex = 0;   // host-side phase timers (L3D_TIMING=1)
    int outcome[3] = { 0, 0, 0 };            // after l3d_shard_chain_run: OR of the ranks' overflow bits (8: the compact arena of the ring mode), largest candidate / kept count of a slot
    // ring mode of l3d_shard_chain_run (commit on the device only): the gathered buffer holds `geom.ring` view blocks, older ones are retired.  Set by the
    // run (ShardRun::plan_ring, setup_ring_tables, shared_verdict), read by the products; `window` alone is the schedule's, set when the chain is opened
    struct Ring {
        bool on = false;
        int window = 0;                      // max over views of (index - smallest source index): how far back a view reads
        long long arena_cap = 0, arena_needed = 0;
        long long* base_dev = nullptr;       // arena offset of every view (+ the total behind the last), kept on the device
        SlotHeader* hdr_all = nullptr;       // the headers of all slots of all views (32 B each)
        const long long* best_off_dev = nullptr;
        const unsigned char* ver_dev = nullptr;
        bool retire_tables = false;          // the retire kernel also files the slots' side words and run tables (ch_keptcam, ch_rt): the products need not rebuild them
        std::vector<long long> rt_off;       // where view k's run table starts in ch_rt (ints)
    } ring;
    // partitioned retirement (l3d_shard_chain_partition): only the views flagged in `keep` go to this rank's compact arena
    struct Part {
        bool on = false;
        int own0 = 0, own1 = 0, reach = 0;
        std::vector<unsigned char> keep;
        const unsigned char* keep_dev = nullptr;
        l3d_exchange_fn exchange = nullptr;  // the run's exchange: l3d_shard_chain_products' one status exchange
        void* user = nullptr;
        unsigned char* status = nullptr;     // [own word | the ranks' words], 256 B each (RingTables::status)
    } part;
};

extern "C" {

void* l3d_ctx_stream(l3d_ctx* c) { return c ? (void*)c->stream : nullptr; }

int l3d_shard_chain_open(l3d_ctx* c, const l3d_chain_view* views, int n_views, int rank, int world, int slot_records,
                         l3d_shard_chain** out, size_t* slot_bytes)
{
    if (!c) return L3D_ERR_INVALID;
    if (!out || !slot_bytes || n_views < 0 || world < 1 || rank < 0 || rank >= world || (n_views > 0 && !views) || slot_records < 1)
        return fail(c, L3D_ERR_INVALID, "l3d_shard_chain_open: bad argument");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipGetLastError();
    std::unique_ptr<l3d_shard_chain> h(new l3d_shard_chain());       // (the caller's once *out is set: every return before that frees it)
    h->c = c; h->views = views; h->n_views = n_views; h->rank = rank; h->world = world;
    ChainLayout L;
    if (int rc = chain_plan_views(c, views, n_views, rank, world, h->vd, L, "l3d_shard_chain_open")) return rc;
    h->maxS = L.maxS; h->maxN = L.maxN; h->pairs = L.pairs;
    for (int k = 0; k < n_views; ++k)
        for (int q = 0; q < views[k].n_sources; ++q) h->ring.window = std::max(h->ring.window, k - views[k].source_index[q]);
    // the slot (l3d_shard_rule.hpp).  The side array of dense scenes was measured on one emulated rank of eight at 64 x 4000 x 24
    // (profiles/r5_emulated_rank_64x4000x24_w8_partition.txt); the run table saves 188 MB of scans per view and rank there
    const SlotPlan plan = slot_geometry(h->maxS, h->maxN, world, slot_records, c->opt.slot_cams_min, n_views);
    h->geom = plan.geom;
    h->stage_bytes = plan.stage_bytes;
    *slot_bytes = h->geom.slot_bytes;

    // tables, target rays, per-view slices of the whole-run arenas (l3d_chain_common.hip: shared with the single-GPU chain)
    if (int rc = chain_upload_tables(c, views, n_views, h->vd, L, st)) return rc;
    if (int rc = chain_assign_arenas(c, views, n_views, h->vd, L, false, true, l3d_shard_chain::kRingA, st)) return rc;   // (+ best positions: l3d_shard_chain_products)
    h->dtab = L.dtab;
    // (the run's statistics words; a partitioned run's products leave the per-view result records in the same buffer afterwards: sized for both)
    HIPCHK(c, c->ch_pin_res.reserve((size_t)n_views * std::max<size_t>(8, sizeof(ChainResult)) + 64));
    h->hstats = c->ch_pin_res.as<int>();
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->hstats_dev), h->hstats, 0));
    {   // stage 1 (own stream) starts after the tables and the zeroed row counts are in place
        hipEvent_t ready = get_event(c);
        HIPCHK(c, hipEventRecord(ready, st));
        HIPCHK(c, hipStreamWaitEvent(c->stage1_stream, ready, 0));
        put_event(c, ready);
    }
    h->cand_cap = c->test_cand_cap ? c->test_cand_cap : chain_first_cand_cap(L.max_pairs);     // (l3d_set_chain_capacities: tests, retries with more room)
    if (int rc = chain_reserve_candidates(c, L, h->cand_cap, l3d_shard_chain::kRingA)) return rc;
    HIPCHK(c, c->ch_pin_kept.reserve(2 * ((size_t)world * (size_t)h->geom.seg_cap * 8 + 64) + 64));
    c->pin_arena.reset();
    HIPCHK(c, c->ch_pin_best.reserve((size_t)n_views * sizeof(PackHeader) + 64));
    h->hdr_host = c->ch_pin_best.as<PackHeader>();
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->hdr_dev), h->hdr_host, 0));
    h->packed.assign((size_t)n_views, 0);
    h->ev1.assign((size_t)n_views, nullptr);
    h->ev2.assign((size_t)n_views, nullptr);
    for (int k = 0; k < n_views; ++k) { h->ev2[(size_t)k] = get_event(c); h->ev1[(size_t)k] = get_event(c); }
    h->ev3 = get_event(c);
    c->stats[0] = h->pairs;
    *out = h.release();
    return L3D_OK;
}

static PairArgs shard_pair_args(l3d_shard_chain* h, int k) { return chain_pair_args(h->c, h->views[k], h->vd[(size_t)k], h->dtab); }

static int shard_stage1(l3d_shard_chain* h, int k)
{
    l3d_ctx* c = h->c;
    hipStream_t s1 = c->stage1_stream;
    const SViewDev& d = h->vd[(size_t)k];
    if (!d.verified) return L3D_OK;
    h->hstats[2 * k] = h->hstats[2 * k + 1] = 0;
    if (d.s1 > d.s0) {
        const PairArgs pa = shard_pair_args(h, k);
        {   // bit rows + row counts (added into the rows zeroed when the chain was opened) in one launch
            const PairArgs pm = chain_mask_args(pa, d, false);
            ProfScope p(c, "pair_mask", s1);
            launch_pair_mask(pm, d.maxW, s1, c->opt.pair_spb);
        }
        // row starts of the stage-1 candidates of the rank's rows + their statistics straight into host-mapped memory (one launch)
        { ProfScope p(c, "scan", s1); launch_scan_range(d.rowcnt, d.rowA, h->views[k].N, d.s0, d.s1, h->views[k].S_src * h->views[k].N, nullptr, nullptr, s1, h->hstats_dev + 2 * k); }
        // depth records of the stage-1 candidates, in their own row order, into the ring slot last used by view k - kRingA
        // (its completion event is recorded by l3d_shard_chain_mark before this view's stage 1 is enqueued)
        if (k - l3d_shard_chain::kRingA >= 0) HIPCHK(c, hipStreamWaitEvent(s1, h->ev2[(size_t)(k - l3d_shard_chain::kRingA)], 0));
        const PairArgs pf = chain_fill_args(pa, d, false, h->cand_cap);
        { ProfScope p(c, "pair_fill", s1); launch_pair_fill(pf, d.rowA, c->ch_ringA_meta.as<uint2>() + (size_t)(k % l3d_shard_chain::kRingA) * h->cand_cap,
                                                             c->ch_ringA_depths.as<float4>() + (size_t)(k % l3d_shard_chain::kRingA) * h->cand_cap, s1); }
    }
    HIPCHK(c, hipEventRecord(h->ev1[(size_t)k], s1));
    return L3D_OK;
}

// workgroups per (source view, rank) list of the two scans of the sources' slots: 16 for the lists of a sparse scene (a few thousand records: 5 steps
// per thread), one per 4096 records of the slot's capacity on a dense one -- 650 k records per slot at 4000 segments x 24 neighbours were 160
// dependent loads per thread (measured on one emulated rank of eight, 64 x 4000 x 24: exist + cand_move 47 -> see profiles/r5_emulated_rank_*).
// A scan wants them by the slot's records; with run tables a list is seg_cap runs of sixteen lanes
static int slot_scan_workgroups(const SlotGeom& g, int slot_scan_grain)
{
    return g.rt_off ? std::max(1, std::min(256, (g.seg_cap * 16 + 255) / 256)) : std::max(16, std::min(256, g.slot_records / (slot_scan_grain > 0 ? slot_scan_grain : 4096)));
}
// whether a view with sources orders its runs of reverse matches in a launch of its own (option exist_sort_apart: 0 never, > 0 always).  The window
// kernel orders the runs itself -- except on a rank's small launch of a dense scene: a segment's workgroup ranks its 12 runs three per wave, one after
// the other, and the launch waits for the heaviest segment; a launch of one wave per run is balanced.  Same rule as the split verification
static bool sorts_runs_apart(const Options& o, int range_segments, size_t cand_cap)
{
    return o.exist_sort_apart != 0 && (o.exist_sort_apart > 0 || (range_segments <= o.vw_wide_max && cand_cap / (size_t)std::max(1, range_segments) >= (size_t)o.vw_split_avg));
}

// Enqueue view k up to (and including) the write of this rank's slot.  send_slot: device buffer of slot_bytes that the
// caller all-gathers into gathered_base + (k*world + r)*slot_bytes for r = 0..world-1 (stream ordered, same stream).
int l3d_shard_chain_enqueue(l3d_shard_chain* h, int k, void* send_slot, const void* gathered_base)
{
    if (!h || k < 0 || k >= h->n_views || !gathered_base) return L3D_ERR_INVALID;
    l3d_ctx* c = h->c;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipGetLastError();            // the framework shares this thread: its (benign) sticky errors are not ours
    if (!h->s1_thread)
        while (h->k_p1 < h->n_views && h->k_p1 <= k + l3d_shard_chain::kStage1Ahead) { int rc = shard_stage1(h, h->k_p1); if (rc) return rc; ++h->k_p1; }
    else
        wait_until([&]() { return h->s1_done.load(std::memory_order_acquire) > k; }, 4000);     // the stage-1 thread enqueues it (normally long done)
    const l3d_chain_view& v = h->views[k];
    const SViewDev& d = h->vd[(size_t)k];
    h->gathered = reinterpret_cast<const unsigned char*>(gathered_base);
    if (!d.verified) return L3D_OK;
    if (!send_slot) return fail(c, L3D_ERR_INVALID, "l3d_shard_chain_enqueue: null slot");
    // its stage-1 statistics: the candidate total, and the largest count per segment that sizes the verification's LDS image
    HIPCHK(c, hipEventSynchronize(h->ev1[(size_t)k]));
    h->raw_sum += h->hstats[2 * k];
    HIPCHK(c, hipStreamWaitEvent(st, h->ev1[(size_t)k], 0));
    PairArgs pa = shard_pair_args(h, k);
    pa.cand_cap = (int)h->cand_cap;
    const int S = v.S_src, N = v.N;
    const size_t nrow = (size_t)S * N;
    const unsigned char* dtab = h->dtab;
    const int* d_sc = reinterpret_cast<const int*>(dtab + d.o_sc);
    const int* d_si = reinterpret_cast<const int*>(dtab + d.o_si);
    unsigned char* slot = reinterpret_cast<unsigned char*>(send_slot);
    const int wps = slot_scan_workgroups(h->geom, c->opt.slot_scan_grain);
    if (v.n_sources) {
        ProfScope p(c, "exist");
        hipLaunchKernelGGL(k_exist_count_slots, dim3(wps, v.n_sources * h->world), dim3(256), 0, st, h->gathered, h->geom, d_si, d_sc, reinterpret_cast<const int*>(h->dtab + d.o_ss), v.view_id, N, d.s0, d.s1, d.rowcnt);
    }
    // row starts of this rank's rows only (+ zeroed scatter cursors, segment order); row_start[nrow] = their total
    { ProfScope p(c, "scan"); launch_scan_range(d.rowcnt, c->row_start.as<int>(), N, d.s0, d.s1, (int)nrow, c->ch_cursor.as<int>(), c->ch_segorder.as<int>(), st); }
    {
        ProfScope p(c, "cand_move");
        const int blocks_move = ((d.s1 - d.s0) * v.n_tbm + 3) / 4;
        const int blocks = blocks_move + wps * v.n_sources * h->world;
        if (blocks > 0)
            hipLaunchKernelGGL(k_place_slots, dim3(blocks), dim3(256), 0, st, blocks_move, wps, pa.tbm, v.n_tbm, d.rowA,
                               c->ch_ringA_meta.as<uint2>() + (size_t)(k % l3d_shard_chain::kRingA) * h->cand_cap,
                               c->ch_ringA_depths.as<float4>() + (size_t)(k % l3d_shard_chain::kRingA) * h->cand_cap,
                               h->gathered, h->geom, d_si, d_sc, reinterpret_cast<const int*>(h->dtab + d.o_ss), v.view_id, N, S, d.s0, d.s1, c->row_start.as<int>(), c->ch_cursor.as<int>(),
                               c->cand_meta.as<uint2>(), c->cand_depths.as<float4>(), (int)h->cand_cap);
    }
    const bool sort_apart = v.n_sources && sorts_runs_apart(c->opt, d.s1 - d.s0, h->cand_cap);
    if (v.n_sources && (!(c->verify_mode == 0 && verify_window_supported(N)) || sort_apart)) {
        ProfScope p(c, "exist");
        launch_exist_sort_runs(d_sc, v.n_sources, N, S, c->row_start.as<int>(), c->cand_meta.as<uint2>(), c->cand_depths.as<float4>(), (int)h->cand_cap, st, d.s0, d.s1,
                               c->vw_scratch.as<float>(), (long long)h->cand_cap + kVWSlack, c->cand_conf.as<unsigned>());
    }
    VerifyArgs va = chain_verify_args(c, v, d, dtab, h->cand_cap);
    chain_launch_verify(c, va, d, d_sc, sort_apart ? 0 : v.n_sources, h->hstats[2 * k + 1], h->cand_cap, st);
    const int mmax = va.mmax;
    {
        ProfScope p(c, "kept_write");
        hipLaunchKernelGGL(k_slot_write, dim3(std::max(1, d.s1 - d.s0)), dim3(256), 0, st, va, c->kept_cnt.as<int>() + d.s0, (int)nrow,
                           h->geom.slot_records, reinterpret_cast<const unsigned*>(dtab + d.o_l2g), d.best, h->geom, slot);
    }
    { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(c, L3D_ERR_HIP, std::string("shard enqueue view ") + std::to_string(k) + " (mmax " + std::to_string(mmax) + ", lds " + std::to_string(verify_window_lds_bytes(mmax, N)) + ", range " + std::to_string(d.s0) + "-" + std::to_string(d.s1) + "): " + hipGetErrorString(e_)); }
    return L3D_OK;
}

// Enqueue the hand-over of view k (k_pack_view) into staging buffer k % kRing.
static int shard_pack(l3d_shard_chain* h, int k, hipStream_t st)
{
    l3d_ctx* c = h->c;
    const size_t block = (size_t)h->world * h->geom.slot_bytes;
    // the staging ring of the host hand-over: 16 views x the ranks' slots -- only a rank that commits on the host ever packs (13 GB at 4000 segments x
    // 24 neighbours: a rank that builds the products on its device never pays it)
    HIPCHK(c, c->ch_stage.reserve((size_t)l3d_shard_chain::kRing * h->stage_bytes + 64));
    hipLaunchKernelGGL(k_pack_view, dim3(8, h->world), dim3(256), 0, st, h->gathered + (size_t)k * block, h->geom,
                       c->ch_stage.as<unsigned char>() + (size_t)(k % l3d_shard_chain::kRing) * h->stage_bytes, h->hdr_dev + k);
    h->packed[(size_t)k] = 1;
    return L3D_OK;
}

// Record "view k is complete" on the stream -- call after the all-gather of view k has been enqueued.
int l3d_shard_chain_mark(l3d_shard_chain* h, int k)
{
    if (!h || k < 0 || k >= h->n_views) return L3D_ERR_INVALID;
    l3d_ctx* c = h->c;
    if (h->eager_pack && h->vd[(size_t)k].verified) { int rc = shard_pack(h, k, c->stream); if (rc) return rc; }
    HIPCHK(c, hipEventRecord(h->ev2[(size_t)k], c->stream));
    h->marked.store(k + 1, std::memory_order_release);
    return L3D_OK;
}

// Wait for view k (host side only) and hand the ranks' kept lists, concatenated in rank (= segment) order, and the depth
// pairs to the callback.  Views must be fetched in ascending order.
int l3d_shard_chain_fetch(l3d_shard_chain* h, int k, l3d_chain_callback cb, void* user)
{
    if (!h || k < 0 || k >= h->n_views || !cb) return L3D_ERR_INVALID;
    l3d_ctx* c = h->c;
    if (!h->vd[(size_t)k].verified) {
        h->fetched.store(k + 1, std::memory_order_release);
        return cb(user, k, 0, nullptr, 0, nullptr, 0, 0) ? fail(c, L3D_ERR_INVALID, "callback failed") : L3D_OK;
    }
    if (h->marked.load(std::memory_order_acquire) <= k) return fail(c, L3D_ERR_INVALID, "l3d_shard_chain_fetch: view not marked");
    HIPCHK(c, hipSetDevice(c->device));
    const double tf0 = now_s();
    if (h->packed[(size_t)k]) {
        HIPCHK(c, hipEventSynchronize(h->ev2[(size_t)k]));
    } else {                                        // step-wise protocol: pack now, behind whatever the stream has queued
        int rc = shard_pack(h, k, c->stream); if (rc) return rc;
        HIPCHK(c, hipEventRecord(h->ev3, c->stream));
        HIPCHK(c, hipEventSynchronize(h->ev3));
    }
    const double tf1 = now_s();
    const PackHeader ph = h->hdr_host[k];
    if (ph.overflow) return fail(c, L3D_ERR_NOMEM, "l3d_shard_chain: view " + std::to_string(k) + ": a rank ran out of candidate or slot capacity, or gave up (l3d_shard_chain_info tells which)");
    const size_t best_bytes = (size_t)h->geom.seg_cap * 8;
    const size_t pin_bytes = (size_t)h->world * best_bytes + 64;
    unsigned char* host = c->ch_pin_kept.as<unsigned char>() + (size_t)(k & 1) * pin_bytes;      // depth pairs: two small pinned buffers
    // the records go straight into the pinned arena (valid for the caller until the next chain), the depth pairs to staging
    auto issue_copy = [&](int v, const PackHeader& hd, l3d_match** dst) -> int {
        const unsigned char* stage = c->ch_stage.as<unsigned char>() + (size_t)(v % l3d_shard_chain::kRing) * h->stage_bytes;
        hipError_t ae = hipSuccess;
        *dst = static_cast<l3d_match*>(c->pin_arena.alloc((size_t)hd.n_kept * sizeof(Match) + 16, &ae));
        HIPCHK(c, ae);
        HIPCHK(c, hipMemcpyAsync(c->ch_pin_kept.as<unsigned char>() + (size_t)(v & 1) * pin_bytes, stage, (size_t)h->world * best_bytes,
                                 hipMemcpyDeviceToHost, c->copy_stream));
        if (hd.n_kept) HIPCHK(c, hipMemcpyAsync(*dst, stage + (size_t)h->world * best_bytes, (size_t)hd.n_kept * sizeof(Match), hipMemcpyDeviceToHost, c->copy_stream));
        return L3D_OK;
    };
    l3d_match* kept_dst = h->copy_dst;
    if (h->copy_issued != k) { int rc = issue_copy(k, ph, &kept_dst); if (rc) return rc; }       // (otherwise the previous fetch has issued it already)
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    h->fetched.store(k + 1, std::memory_order_release);          // the staging buffer of view k may be reused
    // the next view's copy travels while this view's bookkeeping runs, if the GPU is already done with it
    if (k + 1 < h->n_views && h->vd[(size_t)(k + 1)].verified && h->marked.load(std::memory_order_acquire) > k + 1 && h->packed[(size_t)(k + 1)] &&
        hipEventQuery(h->ev2[(size_t)(k + 1)]) == hipSuccess && !h->hdr_host[k + 1].overflow) {
        int rc = issue_copy(k + 1, h->hdr_host[k + 1], &h->copy_dst); if (rc) return rc;
        h->copy_issued = k + 1;
    } else {
        (void)hipGetLastError();                                 // hipEventQuery reports "not ready" as an error
    }
    const l3d_match* kept = kept_dst;
    std::vector<float>& best = h->best_scratch;
    best.clear();
    if (ph.R > 0)
        for (int r = 0; r < h->world; ++r) {
            const int s0 = (int)(((long long)h->views[k].S_src * r) / h->world), s1 = (int)(((long long)h->views[k].S_src * (r + 1)) / h->world);
            const float* b = reinterpret_cast<const float*>(host + (size_t)r * best_bytes);
            for (int s = 0; s < s1 - s0; ++s)
                if (b[2 * s] != -1.0f) { best.push_back(b[2 * s]); best.push_back(b[2 * s + 1]); }
        }
    const double tf2 = now_s();
    h->kept_total += (double)ph.n_kept;
    if (cb(user, k, 1, kept, ph.n_kept, best.data(), (int)(best.size() / 2), (int)std::min<long long>(ph.R, 0x7fffffff)))
        return fail(c, L3D_ERR_INVALID, "callback failed");
    h->t_wait += tf1 - tf0; h->t_copy += tf2 - tf1; h->t_cb += now_s() - tf2;
    return L3D_OK;
}

}  // extern "C"

// ---- the whole sharded chain as ONE native call -------------------------------------------------------------------
// The calling thread only enqueues: this rank's kernels of view k, then the exchange of the ranks' slots on the same
// stream (RCCL all-gather over xGMI through l3d_exchange_rccl), then the "view complete" event.  A second host thread
// trails behind on those events and does the host bookkeeping (fetch -> callback) of the ranks that commit.  No
// interpreter, no host synchronisation on the enqueue path: per view the stream sees ~9 kernels + one collective.
namespace {

// THE HELPER THREADS.  Each of the two classes owns its thread and its flags, and its destructor stops and joins.  A std::thread destroyed while
// joinable terminates the process -- and would leave the peers waiting in their collectives: with the threads owned here, no return between their
// start and the end of the run can skip the join, wherever a line is moved.

// A second enqueue thread feeds the stage-1 stream (7 of the ~17 calls per view): with small per-rank slices the host launch rate, not the GPU, limits
// the chain otherwise.  It stays kStage1Ahead views ahead of the chain thread (h->marked); the ring slot it writes was released by view k - kRingA,
// whose completion event the chain thread has recorded by then.
class Stage1Feeder {
public:
    explicit Stage1Feeder(l3d_shard_chain* h_) : h(h_)
    {
        h->s1_thread = true;
        h->s1_done.store(0);
        th = std::thread([this]() { run(); });
    }
    ~Stage1Feeder() { finish(); }
    int failed() const { return rc.load(); }
    void finish() { if (!th.joinable()) return; stop.store(true); th.join(); h->s1_thread = false; }

private:
    void run()
    {
        (void)hipSetDevice(h->c->device);
        for (int k = 0; k < h->n_views && !stop.load(); ++k) {
            wait_until([&]() { return stop.load() || h->marked.load(std::memory_order_acquire) >= k - l3d_shard_chain::kStage1Ahead; }, 64);
            if (stop.load()) break;
            const int r = shard_stage1(h, k);
            if (r) { rc.store(r); break; }
            h->s1_done.store(k + 1, std::memory_order_release);
        }
        h->s1_done.store(h->n_views + 1, std::memory_order_release);      // (never leave the chain thread waiting)
    }
    l3d_shard_chain* const h;
    std::atomic<int> rc{L3D_OK};
    std::atomic<bool> stop{false};
    std::thread th;
};

// The bookkeeping thread of a committing rank: it trails the "view complete" events (h->marked, the one count of marked views -- the condition
// variable only carries the wake-up) and hands every view to the callback (l3d_shard_chain_fetch).  A run without a callback starts no thread.
class Fetcher {
public:
    Fetcher(l3d_shard_chain* h_, l3d_chain_callback cb_, void* user_) : h(h_), cb(cb_), user(user_) { if (cb) th = std::thread([this]() { run(); }); }
    ~Fetcher() { finish(); }
    void wake() { if (!cb) return; { std::lock_guard<std::mutex> lk(mu); } cv.notify_one(); }       // h->marked has advanced (under the lock: no wake-up is lost)
    bool failed() { std::lock_guard<std::mutex> lk(mu); return rc != L3D_OK; }
    // stopped (views that are not marked are left out) and joined: the first fetch's error (text: its message), or L3D_OK
    int finish(std::string* text = nullptr)
    {
        if (th.joinable()) {
            { std::lock_guard<std::mutex> lk(mu); stop = true; }
            cv.notify_one();
            th.join();
        }
        if (text) *text = err;
        return rc;
    }

private:
    void run()
    {
        (void)hipSetDevice(h->c->device);
        for (int k = 0; k < h->n_views; ++k) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&]() { return h->marked.load(std::memory_order_acquire) > k || stop; });
                if (h->marked.load(std::memory_order_acquire) <= k) return;
            }
            const int r = l3d_shard_chain_fetch(h, k, cb, user);
            if (r) {
                std::string m;
                { std::lock_guard<std::mutex> lk(h->c->err_mu); m = h->c->err; }
                std::lock_guard<std::mutex> lk(mu);
                rc = r; err = m;
                return;
            }
        }
    }
    l3d_shard_chain* const h;
    const l3d_chain_callback cb;
    void* const user;
    std::mutex mu;
    std::condition_variable cv;
    bool stop = false;
    int rc = L3D_OK;
    std::string err;
    std::thread th;
};

// One call of l3d_shard_chain_run as its phases.
//   THE FAILURE PROTOCOL.  A rank that fails -- its own enqueue, its stage-1 thread, or (committing rank) the bookkeeping thread reading a slot that
// overflowed -- must NOT stop calling the exchange: the other ranks keep enqueueing one collective per verified view and would wait for it forever.
// From the failure on (drain) it sends a header that says "gave up" for every remaining view (no kernels) and keeps exchanging; k_check_slots then
// gives every rank the same verdict.  Only a failing exchange call itself ends the loop (exchange_broken).
struct ShardRun {
    l3d_shard_chain* const h; l3d_ctx* const c;
    const l3d_exchange_fn exchange; void* const exchange_user; const l3d_chain_callback cb;
    const size_t slot, block;                   // bytes of a slot, of a view's gathered block
    std::vector<unsigned char> verified;        // per view (uploaded for the retire kernel and for k_check_slots)
    std::vector<long long> best_off_h;          // per view: where its best depth pairs start in ch_best
    int send_ring = 0;                          // slots this rank sends from
    unsigned char *send = nullptr, *gathered = nullptr;
    RingTables T = RingTables();                // ring mode: the header block's layout, the block itself
    unsigned char* hb = nullptr;
    RetireSchedule sched;                       // ring mode: what is retired and waited for
    hipStream_t rs = nullptr;                   // ... the stream the retirement runs on
    hipEvent_t retire_done = nullptr;           // ... the outstanding batch's retirement on the side stream (sched.outstanding())
    SlotHeader* abort_hdr = nullptr;            // the "gave up" header (pinned)
    int rc = L3D_OK; std::string rc_msg;        // the run's first failure
    bool draining = false, exchange_broken = false;
    double t_run0 = 0;

    ShardRun(l3d_shard_chain* h_, l3d_exchange_fn exchange_, void* exchange_user_, l3d_chain_callback cb_)
        : h(h_), c(h_->c), exchange(exchange_), exchange_user(exchange_user_), cb(cb_), slot(h_->geom.slot_bytes), block(h_->geom.slot_bytes * (size_t)h_->world),
          verified((size_t)h_->n_views), best_off_h((size_t)h_->n_views, 0)
    {
        for (int k = 0; k < h->n_views; ++k) verified[(size_t)k] = h->vd[(size_t)k].verified ? 1 : 0;
    }

    void drain(int code, const std::string& msg) { rc = code; rc_msg = msg; draining = true; }

    int plan_ring();
    void guess_arena();
    int setup_ring_tables();
    int setup_retire_tables();
    int alloc_abort_header();
    void retire_wait();
    void retire_to(int upto);
    void throttle(int k, Stage1Feeder& feeder, Fetcher& fetcher);
    bool step(int k, Stage1Feeder& feeder, Fetcher& fetcher);
    void finish_threads(Stage1Feeder& feeder, Fetcher& fetcher);
    void shared_verdict();
    hipError_t arena_verdict_exchange(hipError_t e, int& arena_overflow);
    void settle_retirement();
};

// ---- the ring plan (shard_ring_plan) and the rings of slots and gathered blocks; where the retirement runs
int ShardRun::plan_ring()
{
    const ShardRingPlan p = shard_ring_plan(h->n_views, h->ring.window, block, c->opt.slot_ring, h->part.on, cb != nullptr);
    h->ring.on = p.ring_mode;
    h->geom.ring = p.ring_views;
    send_ring = p.send_ring;
    if (h->ring.on) {      // (rings of whole slots: GBs whose size is exact)
        HIPCHK(c, c->ch_send.reserve_exact((size_t)send_ring * slot + 256));
        HIPCHK(c, c->ch_gathered.reserve_exact((size_t)h->geom.ring * block + 256));
    } else {
        HIPCHK(c, c->ch_send.reserve((size_t)send_ring * slot + 256));
        HIPCHK(c, c->ch_gathered.reserve((size_t)h->geom.ring * block + 256));
    }
    h->eager_pack = cb != nullptr;
    send = c->ch_send.as<unsigned char>();
    gathered = c->ch_gathered.as<unsigned char>();
    // every verified view's block is fully written by its exchange before anything reads it; only the blocks of views
    // that are never verified (nothing to match) must read as "no kept records"
    if (!h->ring.on)
        for (int k = 0; k < h->n_views; ++k)
            if (!verified[(size_t)k]) HIPCHK(c, hipMemsetAsync(gathered + (size_t)k * block, 0, block, c->stream));
    h->ring.retire_tables = false;
    // The retirement copies a batch's records out of the ring (9.6 GB of traffic per pass of an emulated rank of eight at 64 x 4000 x 24: 4.7 of its 63 ms) and
    // nothing of the chain reads what it writes: it runs on a side stream behind the batch's exchanges (round 6; L3D_RETIRE_APART=0: on the chain's stream)
    sched = RetireSchedule();
    sched.window = h->ring.window; sched.ring = h->geom.ring; sched.apart = h->ring.on && c->opt.retire_apart != 0;
    rs = c->stream;
    if (sched.apart) {
        if (!c->prod_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->prod_stream, hipStreamNonBlocking));
        rs = c->prod_stream;
    }
    return L3D_OK;
}

// the compact arena's first guess (shard_arena_first_guess; the free HBM is asked for only where the rule reads it)
void ShardRun::guess_arena()
{
    size_t fr = kShardFreeUnknown, tot = 0;
    if (shard_guess_reads_free(h->part.on, c->test_arena_cap, c->opt.arena_guess)) {
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = kShardFreeUnknown;
        (void)hipGetLastError();
    }
    long long kept_views = 0;
    for (unsigned char x : h->part.keep) kept_views += x;
    h->ring.arena_cap = shard_arena_first_guess(h->pairs, h->world, c->test_arena_cap, c->chain_seen_arena_cap, c->opt.arena_guess, fr, shard_room_records(c->opt.regrow_free_mb),
                                                h->part.on, kept_views, h->n_views, c->part_arena_seen);
}

// ---- ring mode: the compact arena, the header block (RingTables) with the per-view offsets, the header table and the flags the retire kernel reads
int ShardRun::setup_ring_tables()
{
    if (!h->ring.on) return L3D_OK;
    l3d_shard_chain::Ring& R = h->ring;
    const size_t nvs = (size_t)h->n_views;
    guess_arena();
    if (!h->part.on) HIPCHK(c, c->ch_kept.reserve(((size_t)R.arena_cap + 64) * sizeof(Match)));
    T = ring_tables(nvs, h->world);
    HIPCHK(c, c->ch_hdr.reserve(T.total));
    hb = c->ch_hdr.as<unsigned char>();
    R.base_dev = reinterpret_cast<long long*>(hb + T.base);
    R.hdr_all = reinterpret_cast<SlotHeader*>(hb + T.hdr);
    for (int k = 0; k < h->n_views; ++k) best_off_h[(size_t)k] = verified[(size_t)k] ? (long long)(h->vd[(size_t)k].best - c->ch_best.as<float2>()) : 0;
    HIPCHK(c, hipMemsetAsync(hb, 0, T.best_off, c->stream));
    HIPCHK(c, hipMemsetAsync(hb + T.overflow, 0, 256, c->stream));
    HIPCHK(c, hipMemcpyAsync(hb + T.best_off, best_off_h.data(), nvs * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(hb + T.verified, verified.data(), nvs, hipMemcpyHostToDevice, c->stream));
    R.best_off_dev = reinterpret_cast<const long long*>(hb + T.best_off);
    R.ver_dev = hb + T.verified;
    h->part.keep_dev = nullptr;
    if (h->part.on) {
        HIPCHK(c, hipMemcpyAsync(hb + T.keep, h->part.keep.data(), nvs, hipMemcpyHostToDevice, c->stream));
        h->part.keep_dev = hb + T.keep;
        HIPCHK(c, c->ch_kept.reserve_exact(((size_t)R.arena_cap + 64) * sizeof(Match)));
    }
    if (int r = setup_retire_tables()) return r;
    h->part.status = hb + T.status; h->part.exchange = exchange; h->part.user = exchange_user;
    return L3D_OK;
}

// the retired views' side words and run tables (slots that carry a side array carry both)
int ShardRun::setup_retire_tables()
{
    l3d_shard_chain::Ring& R = h->ring;
    const size_t nvs = (size_t)h->n_views;
    R.retire_tables = h->geom.rt_off != 0 && h->geom.cam_off != 0 && c->opt.prod_transpose != 0 && c->opt.retire_tables != 0;
    if (!R.retire_tables) return L3D_OK;
    R.rt_off.assign(nvs, 0);
    std::vector<int2> sn(nvs);
    long long rt_ints = 0;
    for (int k = 0; k < h->n_views; ++k) {
        sn[(size_t)k] = make_int2(h->views[k].S_src, h->views[k].N);
        R.rt_off[(size_t)k] = rt_ints;
        if (verified[(size_t)k] && (!h->part.on || h->part.keep[(size_t)k])) rt_ints += ((long long)h->views[k].N + 1) * h->views[k].S_src;
    }
    HIPCHK(c, c->ch_rt.reserve((size_t)rt_ints * 4 + 256));
    HIPCHK(c, c->ch_keptcam.reserve(((size_t)R.arena_cap + 64) * 4));
    HIPCHK(c, hipMemcpyAsync(hb + T.rt_off, R.rt_off.data(), nvs * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(hb + T.view_sn, sn.data(), nvs * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (`sn` leaves scope)
    return L3D_OK;
}

// the "gave up" header of the failure protocol
int ShardRun::alloc_abort_header()
{
    hipError_t ae = hipSuccess;
    abort_hdr = static_cast<SlotHeader*>(c->pin_arena.alloc(sizeof(SlotHeader), &ae));
    HIPCHK(c, ae);
    memset(abort_hdr, 0, sizeof(SlotHeader));
    abort_hdr->overflow = kShardBitGaveUp;
    return L3D_OK;
}

// ---- the retirement: RetireSchedule decides, these two perform.  The chain's stream waits for the outstanding batch ...
void ShardRun::retire_wait()
{
    if (!retire_done) return;
    (void)hipStreamWaitEvent(c->stream, retire_done, 0);
    put_local_event(c, retire_done);
    retire_done = nullptr;
}
// ... and the retirement of views [retired, upto) is enqueued behind their exchanges, a batch at a time
void ShardRun::retire_to(int upto)
{
    const l3d_shard_chain::Ring& R = h->ring;
    for (RetireBatch b = sched.next(upto); b.count; b = sched.next(upto)) {
        if (sched.apart) {
            if (b.wait_before) retire_wait();
            hipEvent_t e = get_local_event(c);
            (void)hipEventRecord(e, c->stream);
            (void)hipStreamWaitEvent(rs, e, 0);
            put_local_event(c, e);
        }
        ProfScope p(c, "retire", rs);
        hipLaunchKernelGGL(k_shard_retire, dim3(8, h->world, b.count), dim3(256), 0, rs, gathered, h->geom, R.ver_dev, h->part.keep_dev, b.first, b.count, R.base_dev, R.arena_cap,
                           R.best_off_dev, c->ch_kept.as<Match>(), c->ch_best.as<float2>(), c->ch_bestpos.as<int>(), R.hdr_all, reinterpret_cast<int*>(hb + T.overflow),
                           R.retire_tables ? c->ch_keptcam.as<unsigned>() : nullptr, R.retire_tables ? c->ch_rt.as<int>() : nullptr,
                           reinterpret_cast<const long long*>(hb + T.rt_off), reinterpret_cast<const int2*>(hb + T.view_sn));
        if (sched.apart) {
            retire_done = get_local_event(c);
            (void)hipEventRecord(retire_done, rs);
        }
    }
}

// ---- one view: throttle -> retire what is due -> enqueue (draining: the "gave up" header) -> exchange -> mark
// a committing rank stays less than a staging ring ahead of its bookkeeping thread (which trails the GPU closely)
void ShardRun::throttle(int k, Stage1Feeder& feeder, Fetcher& fetcher)
{
    if (feeder.failed()) drain(feeder.failed(), "l3d_shard_chain_run: stage 1 failed: " + c->err);
    while (!draining && cb && h->fetched.load(std::memory_order_acquire) < k - (l3d_shard_chain::kRing - 2)) {
        if (fetcher.failed()) { draining = true; break; }
        std::this_thread::yield();
    }
    if (fetcher.failed()) draining = true;
}

// false: the exchange call itself failed -- the loop ends
bool ShardRun::step(int k, Stage1Feeder& feeder, Fetcher& fetcher)
{
    if (!draining) throttle(k, feeder, fetcher);
    const bool ver = verified[(size_t)k] != 0;
    unsigned char* const send_slot = send + (size_t)(k % send_ring) * slot;
    unsigned char* const recv_block = gathered + (size_t)(k % h->geom.ring) * block;
    if (!draining) {
        const double te0 = now_s();
        // ring mode: block k % ring is about to be overwritten by this view's exchange -- whatever lived there (view k - ring) and every older view must
        // be in the arena first (RetireSchedule, l3d_shard_rule.hpp: a batch at a time; no later view reads them: they are further back than the window)
        if (h->ring.on) {
            retire_to(sched.due(k));
            if (sched.wait_due(k)) retire_wait();
        }
        const int r = l3d_shard_chain_enqueue(h, k, send_slot, gathered);
        h->t_enq += now_s() - te0;
        if (r) drain(r, c->err);
    }
    if (h->ring.on && !ver && !draining)          // (a view that is never verified must read as "no kept records", whatever lived in its ring block)
        if (hipMemsetAsync(recv_block, 0, block, c->stream) != hipSuccess) { (void)hipGetLastError(); }
    if (draining && ver)
        if (hipMemcpyAsync(send_slot, abort_hdr, sizeof(SlotHeader), hipMemcpyHostToDevice, c->stream) != hipSuccess) { (void)hipGetLastError(); }
    if (ver) {
        const double te1 = now_s();
        if (const int exr = exchange(exchange_user, k, send_slot, recv_block, slot, h->world, (void*)c->stream)) {
            if (rc == L3D_OK) { rc = L3D_ERR_HIP; rc_msg = "l3d_shard_chain_run: the exchange of view " + std::to_string(k) + " failed (code " + std::to_string(exr) + ", last HIP error: " + hipGetErrorString(hipGetLastError()) + ")"; }
            exchange_broken = true;
            return false;
        }
        h->t_ex += now_s() - te1;
    }
    if (!draining) {
        const int r = l3d_shard_chain_mark(h, k);
        if (r) drain(r, c->err);
        else fetcher.wake();
    }
    return true;
}

// ---- both threads joined, the stream drained
void ShardRun::finish_threads(Stage1Feeder& feeder, Fetcher& fetcher)
{
    feeder.finish();
    if (rc == L3D_OK && feeder.failed()) { rc = feeder.failed(); rc_msg = "l3d_shard_chain_run: stage 1 failed"; }
    const double t_run1 = now_s();
    (void)hipStreamSynchronize(c->stream);
    const double t_run2 = now_s();
    // (l3d_shard_chain_enqueue has added these totals already: the native run's "raw" statistic counts every candidate twice -- left as it is here, a fix of its own)
    for (int k = 0; k < h->n_views; ++k) if (verified[(size_t)k]) h->raw_sum += h->hstats[2 * k];
    std::string fetch_err;
    const int fetch_rc = fetcher.finish(&fetch_err);
    if (c->opt.timing)
        fprintf(stderr, "[l3d shard chain run] enqueue loop %.2f ms, stream drained after %.2f ms, bookkeeping thread done after %.2f ms\n",
                (t_run1 - t_run0) * 1e3, (t_run2 - t_run0) * 1e3, (now_s() - t_run0) * 1e3);
    if (rc == L3D_OK && fetch_rc) { rc = fetch_rc; rc_msg = fetch_err; }
}

// ---- the verdict every rank shares: the overflow bits of all gathered headers (k_check_slots: same blocks, same answer on every rank)
void ShardRun::shared_verdict()
{
    const int nv = h->n_views;
    int host3[3] = { 0, 0, 0 }, arena_overflow = 0;
    long long arena_total = 0;
    bool checked = false;                           // k_check_slots ran over every view's headers
    hipError_t e = c->ch_flags.reserve((size_t)nv + 64);
    if (e == hipSuccess) e = hipMemsetAsync(c->ch_flags.p, 0, 16, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->ch_flags.as<unsigned char>() + 16, verified.data(), (size_t)nv, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && h->ring.on) {
        if (!draining) retire_to(nv);               // the views still in the ring
        sched.wait_all();
        retire_wait();
        checked = sched.retired == nv;
        if (checked) {
            hipLaunchKernelGGL(k_check_slots, dim3(8), dim3(256), 0, c->stream, reinterpret_cast<const unsigned char*>(h->ring.hdr_all), sizeof(SlotHeader), h->geom,
                               c->ch_flags.as<unsigned char>() + 16, nv, c->ch_flags.as<int>());
            e = hipMemcpyAsync(&arena_overflow, hb + T.overflow, 4, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&arena_total, h->ring.base_dev + nv, 8, hipMemcpyDeviceToHost, c->stream);
        } else {
            host3[0] = kShardBitGaveUp;             // this rank gave up before every view was exchanged: so did the verdict
        }
    } else if (e == hipSuccess) {
        hipLaunchKernelGGL(k_check_slots, dim3(8), dim3(256), 0, c->stream, gathered, slot, h->geom, c->ch_flags.as<unsigned char>() + 16, nv, c->ch_flags.as<int>());
        checked = true;
    }
    if (e == hipSuccess && checked) e = hipMemcpyAsync(host3, c->ch_flags.p, 12, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (h->part.on && h->part.status) e = arena_verdict_exchange(e, arena_overflow);
    if (e != hipSuccess) {
        if (rc == L3D_OK) { rc = L3D_ERR_HIP; rc_msg = std::string("l3d_shard_chain_run: reading the slot headers: ") + hipGetErrorString(e); }
        return;
    }
    if (arena_overflow) host3[0] |= kShardBitArena;     // the compact arena's first guess was too small (same data, same verdict on every rank)
    h->ring.arena_needed = arena_total;
    h->outcome[0] = host3[0]; h->outcome[1] = host3[1]; h->outcome[2] = host3[2];
    const ShardVerdict v = shard_verdict(host3[0], host3[1], host3[2], arena_total);
    if (v.rc && (rc == L3D_OK || rc == L3D_ERR_NOMEM)) { rc = v.rc; rc_msg = v.text; }
}

// partitioned: every rank's arena is its own, "too small" is no shared verdict by itself -- one more exchange makes it one (entered by every rank,
// whatever happened to it: the status words of the block modes).  e: what reading this rank's own headers gave; returns the first error of the two
hipError_t ShardRun::arena_verdict_exchange(hipError_t e, int& arena_overflow)
{
    std::vector<long long> words;
    const StatusWords s = exchange_status_words(exchange, exchange_user, h->world, e == hipSuccess ? (long long)arena_overflow : 1, h->part.status, h->part.status + 256, c->stream, words);
    if (!s.exchanged) {
        if (rc == L3D_OK) { rc = L3D_ERR_HIP; rc_msg = "l3d_shard_chain_run: the exchange of the arena verdicts failed"; }
        return e == hipSuccess ? s.publish : e;
    }
    const hipError_t e2 = s.publish != hipSuccess ? s.publish : s.read;
    if (e2 == hipSuccess)
        for (long long x : words) if (x) arena_overflow = 1;
    return e == hipSuccess ? e2 : e;
}

// (a run that ended early: nothing of the retirement stays in flight)
void ShardRun::settle_retirement()
{
    if (!retire_done) return;
    (void)hipStreamSynchronize(rs);
    put_local_event(c, retire_done);
    retire_done = nullptr;
}

}  // namespace

extern "C" {

int l3d_shard_chain_run(l3d_shard_chain* h, l3d_exchange_fn exchange, void* exchange_user, l3d_chain_callback cb, void* cb_user)
{
    if (!h || !exchange) return L3D_ERR_INVALID;
    l3d_ctx* c = h->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (h->part.on && cb) return fail(c, L3D_ERR_UNSUPPORTED, "l3d_shard_chain_run: a partitioned run hands nothing to the host (cb must be NULL)");
    ShardRun R(h, exchange, exchange_user, cb);
    if (int rc = R.plan_ring()) return rc;
    if (int rc = R.setup_ring_tables()) return rc;
    if (int rc = R.alloc_abort_header()) return rc;
    {   // (the threads live in this scope: whatever leaves it joins them)
        Fetcher fetcher(h, cb, cb_user);
        Stage1Feeder feeder(h);
        R.t_run0 = now_s();
        for (int k = 0; k < h->n_views; ++k)
            if (!R.step(k, feeder, fetcher)) break;
        R.finish_threads(feeder, fetcher);
    }
    if (!R.exchange_broken) R.shared_verdict();
    R.settle_retirement();
    return R.rc ? fail(c, R.rc, R.rc_msg) : L3D_OK;
}

// exchange adapters.  RCCL: user = l3d_rccl_link {communicator, address of ncclAllGather}; the library does not link
// against RCCL, the caller hands over what its process already has loaded (line3d_amd/distributed.py).
int l3d_exchange_rccl(void* user, int, const void* send_slot, void* recv_block, size_t slot_bytes, int, void* stream)
{
    const l3d_rccl_link* L = static_cast<const l3d_rccl_link*>(user);
    if (!L || !L->comm || !L->all_gather) return 1;
    typedef int (*all_gather_t)(const void*, void*, size_t, int, void*, void*);       // ncclAllGather(send, recv, count, dtype, comm, stream)
    return reinterpret_cast<all_gather_t>(L->all_gather)(send_slot, recv_block, slot_bytes, 1 /* ncclUint8 */, L->comm, stream);
}
// a single rank: the gathered block is the slot itself
int l3d_exchange_local(void*, int, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream)
{
    if (world != 1) return 1;
    return (int)hipMemcpyAsync(recv_block, send_slot, slot_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}
// replay of a recorded run (user = device address of its gathered blocks): one rank of a world-W job measured on one GPU
int l3d_exchange_replay(void* user, int view, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream)
{
    const size_t block = slot_bytes * (size_t)world;
    //  the only negative tag a replay can answer is -3, the status words of a partitioned run, whose readers ask "did anybody report something"
    // and "how much in all": the replayed rank's words land in slot 0, its peers' stay zero.  Any other collective of the block modes indexes the block by
    // rank and would read the wrong slot: refused
    if (view < 0 && view != -3) { fprintf(stderr, "[l3d exchange_replay] tag %d: a replay holds gathered slots of views and answers status exchanges (-3) only\n", view); return 1; }
    if (view < 0) {      // a status-word exchange of a partitioned run (tag -3): the replayed rank alone, its peers report "nothing to report"
        hipError_t e0 = hipMemsetAsync(recv_block, 0, block, (hipStream_t)stream);
        if (e0 == hipSuccess) e0 = hipMemcpyAsync(recv_block, send_slot, slot_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        return (int)e0;
    }
    const hipError_t e = hipMemcpyAsync(recv_block, static_cast<const unsigned char*>(user) + (size_t)view * block, block, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) fprintf(stderr, "[l3d exchange_replay] view %d: hipMemcpyAsync(dst %p, src %p + %zu, %zu bytes): %s\n", view, recv_block, user, (size_t)view * block, block, hipGetErrorString(e));
    return (int)e;
}
const void* l3d_shard_chain_gathered(l3d_shard_chain* h) { return h && !h->ring.on ? h->c->ch_gathered.p : nullptr; }     // (ring mode: most blocks are gone)
long long l3d_shard_chain_arena_needed(l3d_shard_chain* h) { return h ? h->ring.arena_needed : 0; }
int l3d_shard_chain_info(l3d_shard_chain* h, size_t* cand_cap, int* slot_records, int* overflow_bits, int* max_candidates, int* max_kept)
{
    if (!h) return L3D_ERR_INVALID;
    if (cand_cap) *cand_cap = h->cand_cap;
    if (slot_records) *slot_records = h->geom.slot_records;
    if (overflow_bits) *overflow_bits = h->outcome[0];
    if (max_candidates) *max_candidates = h->outcome[1];
    if (max_kept) *max_kept = h->outcome[2];
    return L3D_OK;
}

// What matchViews leaves behind (l3d_match_chain_resident's products: potential correspondences, best matches, medians), built on THIS
// rank's device from the gathered slots of a finished, successful l3d_shard_chain_run: all views' kept records go into one arena in the
// order of the unsharded run, then the very builder of the single-GPU chain runs on it.  Every rank may call it (each then holds the
// full products and can run greedy selection / affinity fill / clustering); none hands a kept list to the host.
static int shard_products_local(l3d_shard_chain* h, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot, ProductsPart* part_out);

int l3d_shard_chain_products(l3d_shard_chain* h, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot)
{
    if (!h) return L3D_ERR_INVALID;
    l3d_ctx* c = h->c;
    if (!map || !summary) return fail(c, L3D_ERR_INVALID, "l3d_shard_chain_products: bad argument");
    if (!h->gathered || h->outcome[0]) return fail(c, L3D_ERR_INVALID, "l3d_shard_chain_products: no finished run without overflow on this chain");     // (a verdict every rank shares)
    if (!h->part.on) return shard_products_local(h, map, summary, n_pot, nullptr);
    // partitioned: whatever this rank fails in on its own travels with ONE status exchange (tag -3) that every rank enters -- the ranks go on to the
    // collective finish together or not at all
    ProductsPart part;
    int64_t n_local = 0;
    const int rc = shard_products_local(h, map, summary, &n_local, &part);
    std::string err_local;
    if (rc) { std::lock_guard<std::mutex> lk(c->err_mu); err_local = c->err; }
    hipStream_t st = c->stream;
    std::vector<long long> words;
    const StatusWords s = exchange_status_words(h->part.exchange, h->part.user, h->world, rc ? -(long long)std::abs(rc) : (long long)n_local, h->part.status, h->part.status + 256, st, words);
    if (!s.exchanged) return fail(c, L3D_ERR_HIP, "l3d_shard_chain_products: the exchange of the status words failed");
    if (rc) return fail(c, rc, err_local);
    if (s.read != hipSuccess) return fail(c, L3D_ERR_HIP, std::string("l3d_shard_chain_products: reading the status words: ") + hipGetErrorString(s.read));
    part.n_pot_all = 0;
    for (int r = 0; r < h->world; ++r) {
        const long long x = words[(size_t)r];
        if (x < 0) return fail(c, L3D_ERR_HIP, "l3d_shard_chain_products: rank " + std::to_string(r) + " failed (code " + std::to_string(-x) + ") while building its rows of the products");
        part.n_pot_all += x;
    }
    c->products.part = part;
    c->products.n_pot = n_local;
    c->products.valid = true;
    if (n_pot) *n_pot = n_local;
    return L3D_OK;
}

// a partitioned rank's share from its compact arena: rows of the views within reach of its block, best matches / medians of every view it kept
static int shard_products_share(l3d_shard_chain* h, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot, ProductsPart* part_out,
                                const std::vector<ProdChainView>& pvh, const std::vector<ChainResult>& hres, long long total, const unsigned* qt_arena)
{
    l3d_ctx* c = h->c;
    const int nv = h->n_views, own0 = h->part.own0, own1 = h->part.own1, reach = h->part.reach;
    ProductsPart part = products_part(h->views, nv, map, h->rank, h->world, own0, own1, std::max(0, own0 - reach), std::min(nv, own1 + reach), std::max(0, own0 - 2 * reach), std::min(nv, own1 + 2 * reach));
    // (a turn of a node object whose ranks share a device: the share was computed alone -- world 1 -- and joins the collective finish as the rank it stands for)
    if (c->turn_share && h->world == 1 && c->opt.part_vworld > 0) { part.world = c->opt.part_vworld; part.rank = std::max(0, std::min(c->opt.part_vrank, part.world - 1)); }
    int64_t n_local = 0;
    if (c->opt.part_release != 0) {
        // the job is sized by memory: the chain's scratch and the rings of slots are given back before the products are built (as l3d_match_chain_partition does)
        if (int rc = release_chain_scratch(c, { &c->ch_gathered, &c->ch_send })) return rc;
        h->gathered = nullptr;
    }
    const int rc = build_products(c, h->views, nv, pvh.data(), hres.data(), map, summary, &n_local, part.row_dv0, part.row_dv1, reinterpret_cast<const char*>(h->part.keep.data()), qt_arena);
    if (rc) return rc;
    c->part_arena_seen = std::max(c->part_arena_seen, (size_t)total + (size_t)total / 8 + 65536);
    if (n_pot) *n_pot = n_local;
    if (part_out) *part_out = part;
    memcpy(c->ch_pin_res.as<ChainResult>(), hres.data(), (size_t)nv * sizeof(ChainResult));      // (what l3d_chain_kept_list reads)
    return L3D_OK;
}

// the rank-local part: totals, (partitioned: release of the chain's scratch,) the builder of the single-GPU chain on this rank's arena
static int shard_products_local(l3d_shard_chain* h, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot, ProductsPart* part_out)
{
    l3d_ctx* c = h->c;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int nv = h->n_views;
    const size_t nvs = (size_t)nv;
    // scratch: verified flags | totals int2 | kept_base u64 | best_off i64
    const size_t o_ver = 0, o_tot = align256(nvs), o_kb = o_tot + align256(nvs * 8), o_bo = o_kb + align256(nvs * 8), bytes = o_bo + align256(nvs * 8);
    HIPCHK(c, c->g7.reserve(bytes + 64));
    unsigned char* sc = c->g7.as<unsigned char>();
    std::vector<unsigned char> ver(nvs);
    for (int k = 0; k < nv; ++k) ver[(size_t)k] = h->vd[(size_t)k].verified ? 1 : 0;
    HIPCHK(c, hipMemcpyAsync(sc + o_ver, ver.data(), nvs, hipMemcpyHostToDevice, st));
    if (h->ring.on) hipLaunchKernelGGL(k_shard_totals, dim3((nv + 255) / 256), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(h->ring.hdr_all), sizeof(SlotHeader), h->geom, sc + o_ver, nv, reinterpret_cast<int2*>(sc + o_tot));
    else hipLaunchKernelGGL(k_shard_totals, dim3((nv + 255) / 256), dim3(256), 0, st, h->gathered, h->geom.slot_bytes, h->geom, sc + o_ver, nv, reinterpret_cast<int2*>(sc + o_tot));
    std::vector<int2> tot(nvs);
    HIPCHK(c, hipMemcpyAsync(tot.data(), sc + o_tot, nvs * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->shard_view_kept.assign(nvs, 0);
    for (int k = 0; k < nv; ++k) c->shard_view_kept[(size_t)k] = h->vd[(size_t)k].verified ? tot[(size_t)k].x : 0;
    std::vector<ChainResult> hres(nvs);
    std::vector<ProdChainView> pvh(nvs);
    std::vector<unsigned long long> kept_base(nvs, 0);
    std::vector<long long> best_off(nvs, 0);
    long long total = 0;
    for (int k = 0; k < nv; ++k) {
        const SViewDev& d = h->vd[(size_t)k];
        ChainResult& r = hres[(size_t)k];
        const bool here = !h->part.on || h->part.keep[(size_t)k];            // (partitioned: the views this rank retired)
        r.kept_base = (uint64_t)total; r.n_want = 0; r.n_kept = d.verified && here ? tot[(size_t)k].x : 0; r.R = d.verified && here ? tot[(size_t)k].y : 0; r.overflow = 0;
        kept_base[(size_t)k] = (unsigned long long)total;
        total += r.n_kept;
        best_off[(size_t)k] = d.verified ? (long long)(d.best - c->ch_best.as<float2>()) : 0;
        pvh[(size_t)k].verified = d.verified ? 1 : 0;
        pvh[(size_t)k].best = d.verified && here ? d.best : nullptr;
        pvh[(size_t)k].bestpos = d.verified && here ? d.bestpos : nullptr;
        pvh[(size_t)k].rt = h->ring.on && h->ring.retire_tables && d.verified && here ? c->ch_rt.as<int>() + h->ring.rt_off[(size_t)k] : nullptr;
    }
    const unsigned* qt_arena = h->ring.on && h->ring.retire_tables ? c->ch_keptcam.as<unsigned>() : nullptr;
    if (h->ring.on) {
        // the records are in the arena already (k_shard_retire, view by view in this very order)
        if (total != h->ring.arena_needed) return fail(c, L3D_ERR_INVALID, "l3d_shard_chain_products: the retired records do not add up to the slot headers");
        h->kept_total = (double)total;
        if (h->part.on) return shard_products_share(h, map, summary, n_pot, part_out, pvh, hres, total, qt_arena);
        c->chain_seen_arena_cap = std::max(c->chain_seen_arena_cap, (size_t)total + (size_t)total / 8 + 65536);
        return build_products(c, h->views, nv, pvh.data(), hres.data(), map, summary, n_pot, 0, -1, nullptr, qt_arena);
    }
    HIPCHK(c, c->ch_kept.reserve(((size_t)total + 64) * sizeof(Match)));
    HIPCHK(c, hipMemcpyAsync(sc + o_kb, kept_base.data(), nvs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(sc + o_bo, best_off.data(), nvs * 8, hipMemcpyHostToDevice, st));
    if (nv > 0)
        hipLaunchKernelGGL(k_shard_pack_all, dim3(8, h->world, nv), dim3(256), 0, st, h->gathered, h->geom, sc + o_ver, reinterpret_cast<const unsigned long long*>(sc + o_kb),
                           reinterpret_cast<const long long*>(sc + o_bo), c->ch_kept.as<Match>(), c->ch_best.as<float2>(), c->ch_bestpos.as<int>());
    HIPCHK(c, hipStreamSynchronize(st));                                 // (the upload sources above are locals)
    HIPCHK(c, hipGetLastError());
    h->kept_total = (double)total;
    return build_products(c, h->views, nv, pvh.data(), hres.data(), map, summary, n_pot);
}

// A partitioned job on top of the segment-sharded run (round 5): every rank sees every view's gathered slots go by, so WHAT IT KEEPS is its own
// choice -- with this call: the views its block [own_begin, own_end) of the chain needs (2 x reach either side: DESIGN.md section 6 iii), the sources
// of the early-return views and the views their local camera numbers name (cudawrapper.cu:877-878, line3D.cc:861-865: whole lists, a few views).
// The run then retires only those into this rank's arena; l3d_shard_chain_products builds the rows of the block and its neighbours, the best
// matches and medians of the kept views -- the state l3d_match_chain_partition leaves, computed WITHOUT speculation (a scene whose chain never
// forgets a cold start -- the box scene at 4000 segments x 24 neighbours keeps half of its candidates and does not within 120 views -- gets the
// segment-sharded run's speed and the partition's memory).  l3d_affinity_fill_sharded follows as there.
int l3d_partition_keep_views(const l3d_chain_view* views, int nv, int own_begin, int own_end, unsigned char* keep, int* reach_out)
{
    // (host logic only: no context, no device -- tests/test_partition_keep_cpu.py runs it without a GPU)
    if (!views || !keep || nv < 0 || own_begin < 0 || own_end > nv || own_begin > own_end) return L3D_ERR_INVALID;
    const ScheduleIndex index(views, nv);
    const int reach = std::max(1, index.neighbour_reach());
    std::fill(keep, keep + nv, (unsigned char)0);
    for (int k = std::max(0, own_begin - 2 * reach); k < std::min(nv, own_end + 2 * reach); ++k) keep[k] = 1;
    for (int k = 0; k < nv; ++k) {
        if (views[k].n_tbm != 0 || views[k].n_sources == 0) continue;          // an early-return view (cudawrapper.cu:877-878) ...
        keep[k] = 1;
        for (int q = 0; q < views[k].n_sources; ++q) {
            const int si = views[k].source_index[q];                            // ... its sources, whose lists hold the records that point at it ...
            if (si >= 0 && si < nv) keep[si] = 1;
            const int av = index.find((unsigned)views[k].source_cam[q]);        // ... and the view its LOCAL camera number names (line3D.cc:861-865)
            if (av >= 0) keep[av] = 1;
        }
    }
    if (reach_out) *reach_out = reach;
    return L3D_OK;
}

int l3d_shard_chain_partition(l3d_shard_chain* h, int own_begin, int own_end)
{
    if (!h) return L3D_ERR_INVALID;
    l3d_ctx* c = h->c;
    const int nv = h->n_views;
    if (own_begin < 0 || own_end > nv || own_begin > own_end) return fail(c, L3D_ERR_INVALID, "l3d_shard_chain_partition: bad view range");
    h->part.keep.assign((size_t)nv, 0);
    int reach = 1;
    if (int rc = l3d_partition_keep_views(h->views, nv, own_begin, own_end, h->part.keep.data(), &reach)) return fail(c, rc, "l3d_shard_chain_partition: bad schedule");
    h->part.on = true; h->part.own0 = own_begin; h->part.own1 = own_end; h->part.reach = reach;
    return L3D_OK;
}

int l3d_shard_chain_close(l3d_shard_chain* h)
{
    if (!h) return L3D_ERR_INVALID;
    l3d_ctx* c = h->c;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stage1_stream);
    (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : h->ev1) put_event(c, e);
    for (hipEvent_t e : h->ev2) put_event(c, e);
    put_event(c, h->ev3);
    c->stats[1] = h->raw_sum; c->stats[3] = h->kept_total;
    if (c->opt.timing)
        fprintf(stderr, "[l3d shard chain rank %d/%d] enqueue %.2f  exchange-call %.2f | fetch: wait %.2f  d2h %.2f  callback %.2f ms\n",
                h->rank, h->world, h->t_enq * 1e3, h->t_ex * 1e3, h->t_wait * 1e3, h->t_copy * 1e3, h->t_cb * 1e3);
    delete h;
    return L3D_OK;
}

// the rules of l3d_shard_rule.hpp on plain numbers (tests/test_shard_plan_cases_cpu.py): no context, no device.  A section whose input is null is skipped
int l3d_test_shard_plan(const int64_t geom_in[6], int64_t geom_out[10], const int64_t ring_in[6], int32_t ring_out[3], double pairs, const int64_t guess_in[10],
                        int64_t* guess_out, const int64_t verdict_in[4], int32_t* verdict_rc, char* text, int text_cap, const int64_t retry_in[8], int64_t retry_out[5])
{
    if (geom_in) {
        if (!geom_out || geom_in[2] < 1 || geom_in[3] < 1) return L3D_ERR_INVALID;
        const SlotPlan p = slot_geometry((int)geom_in[0], (int)geom_in[1], (int)geom_in[2], (int)geom_in[3], (int)geom_in[4], (int)geom_in[5]);
        const SlotGeom& g = p.geom;
        const int64_t v[10] = { g.seg_cap, (int64_t)g.best_off, (int64_t)g.bpos_off, (int64_t)g.rec_off, (int64_t)g.cam_off, (int64_t)g.rt_off, (int64_t)g.slot_bytes, (int64_t)p.stage_bytes, g.ring, g.max_n };
        memcpy(geom_out, v, sizeof(v));
    }
    if (ring_in) {
        if (!ring_out) return L3D_ERR_INVALID;
        const ShardRingPlan p = shard_ring_plan((int)ring_in[0], (int)ring_in[1], (size_t)ring_in[2], (int)ring_in[3], ring_in[4] != 0, ring_in[5] != 0);
        ring_out[0] = p.ring_mode ? 1 : 0; ring_out[1] = p.ring_views; ring_out[2] = p.send_ring;
    }
    if (guess_in) {      // world, test cap, seen cap, arena_guess, free bytes (-1: unknown), regrow_free_mb, partition, kept views, n_views, part seen
        if (!guess_out) return L3D_ERR_INVALID;
        guess_out[1] = shard_room_records((int)guess_in[5]);
        guess_out[0] = shard_arena_first_guess(pairs, (int)guess_in[0], (size_t)guess_in[1], (size_t)guess_in[2], (int)guess_in[3], guess_in[4] < 0 ? kShardFreeUnknown : (size_t)guess_in[4],
                                               guess_out[1], guess_in[6] != 0, guess_in[7], (int)guess_in[8], (size_t)guess_in[9]);
    }
    if (verdict_in) {    // bits, largest candidate count, largest kept count, arena total
        if (!verdict_rc || !text || text_cap < 1) return L3D_ERR_INVALID;
        const ShardVerdict v = shard_verdict((int)verdict_in[0], (int)verdict_in[1], (int)verdict_in[2], verdict_in[3]);
        *verdict_rc = v.rc;
        snprintf(text, (size_t)text_cap, "%s", v.text.c_str());
    }
    if (retry_in) {      // bits, cand_cap, largest candidate count, slot_records, largest kept count, arena needed, room, replay
        if (!retry_out) return L3D_ERR_INVALID;
        const ShardRetry r = shard_retry((int)retry_in[0], (size_t)retry_in[1], (int)retry_in[2], (int)retry_in[3], (int)retry_in[4], retry_in[5], retry_in[6], retry_in[7] != 0);
        const int64_t v[5] = { r.retry ? 1 : 0, (int64_t)r.cand_cap_next, r.slot_records_next, (int64_t)r.arena_cap_next, r.refuse_for_room ? 1 : 0 };
        memcpy(retry_out, v, sizeof(v));
    }
    return L3D_OK;
}

// RetireSchedule as l3d_shard_chain_run drives it, over all views of a run whose ring is planned by shard_ring_plan (tests/test_shard_retire_cases_cpu.py): for
// every view the views retired / waited for when its exchange is enqueued, every batch as (first, count, the view it was enqueued at -- n_views: the final
// flush --, waited before), and summary = { ring mode, ring, batches, retired and waited for after the flush, 1 when a batch is still outstanding }
int l3d_test_shard_retire(int n_views, int window, int slot_ring, int partition, int apart, int32_t* retired_at, int32_t* waited_at, int32_t* batches, int max_batches, int32_t summary[6])
{
    if (n_views < 0 || window < 0 || (n_views > 0 && (!retired_at || !waited_at)) || !batches || max_batches < 0 || !summary) return L3D_ERR_INVALID;
    const ShardRingPlan p = shard_ring_plan(n_views, window, 1, slot_ring, partition != 0, false);
    RetireSchedule s;
    s.window = window; s.ring = p.ring_views; s.apart = p.ring_mode && apart != 0;
    int nb = 0;
    auto retire_to = [&](int upto, int at) {
        for (RetireBatch b = s.next(upto); b.count; b = s.next(upto), ++nb)
            if (nb < max_batches) { int32_t* o = batches + 4 * (size_t)nb; o[0] = b.first; o[1] = b.count; o[2] = at; o[3] = b.wait_before ? 1 : 0; }
    };
    for (int k = 0; k < n_views && p.ring_mode; ++k) {
        retire_to(s.due(k), k);
        s.wait_due(k);
        retired_at[k] = s.retired; waited_at[k] = s.waited();
    }
    if (p.ring_mode) { retire_to(n_views, n_views); s.wait_all(); }
    const int32_t v[6] = { p.ring_mode ? 1 : 0, p.ring_views, nb, s.retired, s.waited(), s.outstanding() ? 1 : 0 };
    memcpy(summary, v, sizeof(v));
    return nb <= max_batches ? L3D_OK : L3D_ERR_INVALID;
}

}  // extern "C"

// ---- the slot kernels on slots handed in (tests/test_gpu_shard_slots.py): l3d_test_shard_slot_write, l3d_test_shard_collect, l3d_test_shard_pack.
// Everything a kernel uses as an index or a count is checked here, on the host, before anything is launched.
namespace {

int test_shard_geom(l3d_ctx* c, const l3d_test_shard_geom* gi, SlotPlan& p, const char* what)
{
    if (!gi || gi->maxS < 0 || gi->maxS > 16384 || gi->maxN < 1 || gi->maxN > 255 || gi->world < 1 || gi->world > 64 || gi->slot_records < 1 || gi->slot_records > (1 << 20) ||
        gi->n_views < 0 || gi->n_views > 4096 || gi->ring < 0 || gi->ring > 4096)
        return fail(c, L3D_ERR_INVALID, std::string(what) + ": geometry out of range");
    p = slot_geometry(gi->maxS, gi->maxN, gi->world, gi->slot_records, gi->slot_cams_min, gi->n_views);
    if (gi->ring > 0) p.geom.ring = gi->ring;
    return L3D_OK;
}

// the header of a slot whose view has S segments: empty text = fine
std::string test_slot_header(const SlotHeader& h, const SlotGeom& g, int S)
{
    if (h.R < 0 || h.overflow < 0 || h.overflow > 7) return "a header with R < 0 or overflow outside [0, 7]";
    if (h.s0 < 0 || h.s1 < h.s0 || h.s1 > S || h.s1 - h.s0 > g.seg_cap - 1) return "a header whose range is not 0 <= s0 <= s1 <= S with s1 - s0 <= seg_cap - 1";
    if (!h.overflow && (h.n_kept < 0 || h.n_kept > g.slot_records)) return "a header whose n_kept is outside [0, slot_records]";
    return std::string();
}

// the body of a slot of view w that holds records (header checked): records, side words, run table
std::string test_slot_body(const unsigned char* slot, const SlotGeom& g, const l3d_chain_view& w)
{
    const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(slot);
    const int n = hd->n_kept, ns = hd->s1 - hd->s0;
    const Match* rec = reinterpret_cast<const Match*>(slot + g.rec_off);
    const unsigned* side = g.cam_off ? reinterpret_cast<const unsigned*>(slot + g.cam_off) : nullptr;
    std::vector<std::pair<unsigned, int>> cams;
    for (int q = w.N - 1; q >= 0; --q) cams.push_back(std::make_pair(w.local2global[q], q));
    std::stable_sort(cams.begin(), cams.end(), [](const std::pair<unsigned, int>& a, const std::pair<unsigned, int>& b) { return a.first < b.first; });
    std::vector<int> key((size_t)n);
    for (int i = 0; i < n; ++i) {
        const Match& m = rec[i];
        auto it = std::lower_bound(cams.begin(), cams.end(), std::make_pair(m.camID2, -1));
        if (it == cams.end() || it->first != m.camID2) return "a record whose camera is no neighbour of its view";
        if ((long long)m.segID1 < hd->s0 || (long long)m.segID1 >= hd->s1) return "a record whose segment is outside its header's range";
        if (m.segID2 >= 65536u) return "a record whose target does not fit 16 bits";
        // (several neighbours with one id: the lowest local number, as chain_source_slot finds it)
        int q = it->second;
        for (auto jt = it; jt != cams.end() && jt->first == m.camID2; ++jt) q = std::min(q, jt->second);
        key[(size_t)i] = ((int)m.segID1 - hd->s0) * 256 + q;
        if (i > 0 && key[(size_t)i] < key[(size_t)i - 1]) return "records out of (segment, local camera) order";
        if (side && side[i] != (((unsigned)q << 16) | m.segID2)) return "a side word that is not (local camera << 16 | target) of its record";
    }
    if (g.rt_off) {
        const int* rt = reinterpret_cast<const int*>(slot + g.rt_off);
        for (int q = 0; q <= w.N; ++q)
            for (int j = 0; j < ns; ++j) {
                const int want = q < w.N ? j * 256 + q : (j + 1) * 256;
                if (rt[(size_t)q * g.seg_cap + j] != (int)(std::lower_bound(key.begin(), key.end(), want) - key.begin())) return "a run-table entry that is not the position of the first record at or behind (segment, camera)";
            }
    }
    return std::string();
}

}  // namespace

extern "C" {

// k_slot_write on one view's verified candidates of the caller's, for one rank's range: validated on the host, the slot filled with 0xff bytes (0x7f in the
// best positions), 256 guard bytes behind it, then the launch l3d_shard_chain_enqueue makes.
int l3d_test_shard_slot_write(l3d_ctx* c, int S, int N, const int32_t* row_start, const uint32_t* cand_meta, const float* cand_depths, const float* cand_conf,
                              const int32_t* kept_cnt, const uint32_t* local2global, const float* best, int s0, int s1, const l3d_test_shard_geom* geom,
                              int cand_cap, unsigned char* slot)
{
    if (!c) return L3D_ERR_INVALID;
    SlotPlan plan;
    if (int rc = test_shard_geom(c, geom, plan, "shard_slot_write")) return rc;
    const SlotGeom g = plan.geom;
    if (S < 0 || N < 1 || N > 255 || !row_start || !local2global || !slot || cand_cap < 0 || (S > 0 && (!kept_cnt || !best))) return fail(c, L3D_ERR_INVALID, "shard_slot_write: bad argument");
    if (N > geom->maxN || S > geom->maxS) return fail(c, L3D_ERR_INVALID, "shard_slot_write: the view is larger than the geometry's largest");
    if (s0 < 0 || s1 < s0 || s1 > S || s1 - s0 > g.seg_cap - 1) return fail(c, L3D_ERR_INVALID, "shard_slot_write: the range is outside [0, S] or longer than seg_cap - 1");
    const size_t nrow = (size_t)S * N;
    if (row_start[0] != 0) return fail(c, L3D_ERR_INVALID, "shard_slot_write: row_start must start at 0");
    for (size_t i = 0; i < nrow; ++i) if (row_start[i + 1] < row_start[i]) return fail(c, L3D_ERR_INVALID, "shard_slot_write: row_start does not ascend");
    const int R = row_start[nrow];
    if (R > 0 && (!cand_meta || !cand_depths || !cand_conf)) return fail(c, L3D_ERR_INVALID, "shard_slot_write: candidates missing");
    for (int y = 0; y < S; ++y) {
        int kept = 0;
        for (int q = 0; q < N; ++q)
            for (int r = row_start[(size_t)y * N + q]; r < row_start[(size_t)y * N + q + 1]; ++r) {
                if (cand_meta[2 * (size_t)r + 1] != (unsigned)q) return fail(c, L3D_ERR_INVALID, "shard_slot_write: a candidate's camera is not its row's");
                if (cand_meta[2 * (size_t)r] >= 65536u) return fail(c, L3D_ERR_INVALID, "shard_slot_write: a target id does not fit 16 bits");
                kept += cand_conf[r] > 1.0f ? 1 : 0;
            }
        if (kept_cnt[y] != kept) return fail(c, L3D_ERR_INVALID, "shard_slot_write: kept_cnt of segment " + std::to_string(y) + " is not its count of confidences above 1");
    }

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipGetLastError();
    const size_t rcap = (size_t)std::max(R, 1), guard = 256;
    HIPCHK(c, c->row_start.reserve((nrow + 1) * 4));
    HIPCHK(c, c->cand_meta.reserve(rcap * 8)); HIPCHK(c, c->cand_depths.reserve(rcap * 16)); HIPCHK(c, c->cand_conf.reserve(rcap * 4));
    HIPCHK(c, c->kept_cnt.reserve((size_t)S * 4 + 4)); HIPCHK(c, c->l2g.reserve((size_t)N * 4)); HIPCHK(c, c->best.reserve((size_t)S * 8 + 8));
    HIPCHK(c, c->ch_send.reserve(g.slot_bytes + guard));
    HIPCHK(c, hipMemcpyAsync(c->row_start.p, row_start, (nrow + 1) * 4, hipMemcpyHostToDevice, st));
    if (R) {
        HIPCHK(c, hipMemcpyAsync(c->cand_meta.p, cand_meta, (size_t)R * 8, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->cand_depths.p, cand_depths, (size_t)R * 16, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->cand_conf.p, cand_conf, (size_t)R * 4, hipMemcpyHostToDevice, st));
    }
    if (S) {
        HIPCHK(c, hipMemcpyAsync(c->kept_cnt.p, kept_cnt, (size_t)S * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->best.p, best, (size_t)S * 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipMemcpyAsync(c->l2g.p, local2global, (size_t)N * 4, hipMemcpyHostToDevice, st));
    unsigned char* dslot = c->ch_send.as<unsigned char>();
    HIPCHK(c, hipMemsetAsync(dslot, 0xff, g.slot_bytes + guard, st));
    HIPCHK(c, hipMemsetAsync(dslot + g.bpos_off, 0x7f, (size_t)g.seg_cap * 4, st));          // (-1 is an answer of the writer's: no kept match)
    VerifyArgs va;
    memset(&va, 0, sizeof(va));
    va.row_start = c->row_start.as<int>(); va.cand_meta = c->cand_meta.as<uint2>(); va.cand_depths = c->cand_depths.as<float4>(); va.cand_conf = c->cand_conf.as<float>();
    va.N = N; va.seg_begin = s0; va.seg_end = s1; va.nrow_total = (int)nrow; va.cand_cap = cand_cap; va.only_above = -1;
    {
        ProfScope p(c, "kept_write");
        hipLaunchKernelGGL(k_slot_write, dim3(std::max(1, s1 - s0)), dim3(256), 0, st, va, c->kept_cnt.as<int>() + s0, (int)nrow, g.slot_records, c->l2g.as<unsigned>(),
                           c->best.as<float2>(), g, dslot);
    }
    std::vector<unsigned char> back(g.slot_bytes + guard);
    HIPCHK(c, hipMemcpyAsync(back.data(), dslot, back.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (size_t i = g.slot_bytes; i < back.size(); ++i) if (back[i] != 0xff) return fail(c, L3D_ERR_INVALID, "shard_slot_write: the kernel wrote behind the slot");
    memcpy(slot, back.data(), g.slot_bytes);
    return L3D_OK;
}

// The collect step of l3d_shard_chain_enqueue for view k and one range over a gathered buffer of the caller's: every slot a kernel will read is validated
// on the host, the outputs are filled with 0xff bytes, then the chain's launches run with its grid rules.
int l3d_test_shard_collect(l3d_ctx* c, const l3d_chain_view* views, int n_views, int k, const unsigned char* gathered, const l3d_test_shard_geom* geom,
                           const int32_t* rowA, const uint32_t* metaA, const float* depthsA, int n_A, const int32_t* rowcnt,
                           l3d_test_shard_collect_path* sel, int32_t* row_start, uint32_t* cand_meta, float* cand_depths, int32_t* cursor, int32_t* seg_order)
{
    if (!c) return L3D_ERR_INVALID;
    SlotPlan plan;
    if (int rc = test_shard_geom(c, geom, plan, "shard_collect")) return rc;
    const SlotGeom g = plan.geom;
    if (!sel || !views || !gathered || n_views < 1 || n_views != geom->n_views || k < 0 || k >= n_views || !row_start || n_A < 0 || sel->cand_cap < 0 ||
        (sel->cand_cap > 0 && (!cand_meta || !cand_depths)) || (n_A > 0 && (!metaA || !depthsA)))
        return fail(c, L3D_ERR_INVALID, "shard_collect: bad argument");
    const l3d_chain_view& v = views[k];
    const int S = v.S_src, N = v.N, s0 = sel->s0, s1 = sel->s1;
    if (S < 0 || S > geom->maxS || N < 1 || N > geom->maxN || v.n_tbm < 1 || v.n_tbm > N || !v.to_be_matched || !v.local2global || v.n_sources < 0 ||
        (v.n_sources && (!v.source_cam || !v.source_index)) || (S > 0 && (!rowA || !rowcnt || !cursor || !seg_order)))
        return fail(c, L3D_ERR_INVALID, "shard_collect: the view under test is not a verified view within the geometry");
    if (s0 < 0 || s1 < s0 || s1 > S || s1 - s0 > g.seg_cap - 1) return fail(c, L3D_ERR_INVALID, "shard_collect: the range is outside [0, S] or longer than seg_cap - 1");
    std::vector<char> is_tbm((size_t)N, 0), is_src((size_t)N, 0);
    for (int j = 0; j < v.n_tbm; ++j) {
        const int cam = v.to_be_matched[j];
        if (cam < 0 || cam >= N || is_tbm[(size_t)cam]) return fail(c, L3D_ERR_INVALID, "shard_collect: to_be_matched out of range or repeated");
        is_tbm[(size_t)cam] = 1;
    }
    for (int j = 0; j < k; ++j)
        if (views[j].S_src < 0 || views[j].S_src > geom->maxS || views[j].N < 0 || views[j].N > geom->maxN || (views[j].N > 0 && !views[j].local2global))
            return fail(c, L3D_ERR_INVALID, "shard_collect: an earlier view's sizes are outside the geometry");
    long long reverse = 0;
    std::vector<int> src_slot((size_t)v.n_sources, -1);
    for (int q = 0; q < v.n_sources; ++q) {
        const int cam = v.source_cam[q], si = v.source_index[q];
        if (si < 0 || si >= k || cam < 0 || cam >= N || is_tbm[(size_t)cam] || is_src[(size_t)cam])
            return fail(c, L3D_ERR_INVALID, "shard_collect: a source must be an earlier view, its camera a neighbour that is not to be matched, named once");
        is_src[(size_t)cam] = 1;
        if ((long long)si + g.ring < k) return fail(c, L3D_ERR_INVALID, "shard_collect: the ring block of source view " + std::to_string(si) + " was overwritten before view " + std::to_string(k));
        const l3d_chain_view& w = views[si];
        src_slot[(size_t)q] = chain_source_slot(views, v, q);
        if (src_slot[(size_t)q] < 0) continue;                  // (no kernel reads behind the header of such a source's slots)
        for (int r = 0; r < g.world; ++r) {
            const unsigned char* slot = gathered + ((size_t)(si % g.ring) * g.world + r) * g.slot_bytes;
            const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(slot);
            std::string bad = test_slot_header(*hd, g, 65536);
            if (bad.empty() && !hd->overflow && hd->n_kept > 0) {
                bad = hd->s1 > w.S_src ? std::string("a header whose range ends past its view's segments") : test_slot_body(slot, g, w);
                const Match* rec = reinterpret_cast<const Match*>(slot + g.rec_off);
                for (int i = 0; i < hd->n_kept && bad.empty(); ++i) reverse += rec[i].camID2 == v.view_id && (int)rec[i].segID2 >= s0 && (int)rec[i].segID2 < s1 ? 1 : 0;
            }
            if (!bad.empty()) return fail(c, L3D_ERR_INVALID, "shard_collect: source view " + std::to_string(si) + ", rank " + std::to_string(r) + ": " + bad);
        }
    }
    const size_t nrow = (size_t)S * N;
    long long stage1 = 0;
    for (size_t row = 0; row < nrow; ++row) {
        const bool tbm = is_tbm[row % (size_t)N] != 0;
        if (rowcnt[row] < 0 || (!tbm && rowcnt[row] != 0)) return fail(c, L3D_ERR_INVALID, "shard_collect: a stage-1 count below 0, or above 0 for a camera that is not to be matched");
        if (tbm && (rowA[row] < 0 || (long long)rowA[row] + rowcnt[row] > n_A)) return fail(c, L3D_ERR_INVALID, "shard_collect: a stage-1 row outside the stage-1 candidates");
        if ((int)(row / (size_t)N) >= s0 && (int)(row / (size_t)N) < s1) stage1 += rowcnt[row];
    }
    if (stage1 + reverse > sel->cand_cap) return fail(c, L3D_ERR_INVALID, "shard_collect: cand_cap does not hold the range's " + std::to_string(stage1 + reverse) + " candidates");
    sel->wps = sel->blocks_move = sel->R = 0;

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipGetLastError();
    const size_t cap = (size_t)sel->cand_cap, ccap = std::max<size_t>(cap, 1), gbytes = (size_t)g.ring * g.world * g.slot_bytes;
    std::vector<int> tab;
    tab.insert(tab.end(), v.to_be_matched, v.to_be_matched + v.n_tbm);
    const size_t o_sc = tab.size();
    if (v.n_sources) tab.insert(tab.end(), v.source_cam, v.source_cam + v.n_sources);
    const size_t o_si = tab.size();
    if (v.n_sources) tab.insert(tab.end(), v.source_index, v.source_index + v.n_sources);
    const size_t o_ss = tab.size();
    tab.insert(tab.end(), src_slot.begin(), src_slot.end());
    HIPCHK(c, c->tables.reserve(tab.size() * 4 + 16));
    HIPCHK(c, hipMemcpyAsync(c->tables.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    const int* dt = c->tables.as<int>();
    ChainLayout L;
    L.maxS = S; L.maxN = N;
    if (int rc = chain_reserve_candidates(c, L, ccap, 0)) return rc;
    HIPCHK(c, c->ch_gathered.reserve(gbytes + 256));
    HIPCHK(c, c->rowcnt.reserve(nrow * 4 + 16)); HIPCHK(c, c->ch_rowA.reserve(nrow * 4 + 16));
    HIPCHK(c, c->ch_ringA_meta.reserve((size_t)std::max(n_A, 1) * 8)); HIPCHK(c, c->ch_ringA_depths.reserve((size_t)std::max(n_A, 1) * 16));
    HIPCHK(c, c->row_start.reserve((nrow + 1) * 4)); HIPCHK(c, c->ch_cursor.reserve(nrow * 4 + 16)); HIPCHK(c, c->ch_segorder.reserve((size_t)S * 4 + 16));
    HIPCHK(c, hipMemsetAsync(c->ch_gathered.p, 0xee, c->ch_gathered.cap, st));          // (behind the ring: headers that carry every overflow bit -- no records)
    HIPCHK(c, hipMemcpyAsync(c->ch_gathered.p, gathered, gbytes, hipMemcpyHostToDevice, st));
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

    const unsigned char* G = c->ch_gathered.as<unsigned char>();
    const int wps = slot_scan_workgroups(g, sel->slot_scan_grain);
    if (v.n_sources) {
        ProfScope p(c, "exist");
        hipLaunchKernelGGL(k_exist_count_slots, dim3(wps, v.n_sources * g.world), dim3(256), 0, st, G, g, dt + o_si, dt + o_sc, dt + o_ss, v.view_id, N, s0, s1, c->rowcnt.as<int>());
    }
    { ProfScope p(c, "scan"); launch_scan_range(c->rowcnt.as<int>(), c->row_start.as<int>(), N, s0, s1, (int)nrow, c->ch_cursor.as<int>(), c->ch_segorder.as<int>(), st); }
    const int blocks_move = ((s1 - s0) * v.n_tbm + 3) / 4;
    {
        ProfScope p(c, "cand_move");
        const int blocks = blocks_move + wps * v.n_sources * g.world;
        if (blocks > 0)
            hipLaunchKernelGGL(k_place_slots, dim3(blocks), dim3(256), 0, st, blocks_move, wps, dt, v.n_tbm, c->ch_rowA.as<int>(), c->ch_ringA_meta.as<uint2>(), c->ch_ringA_depths.as<float4>(),
                               G, g, dt + o_si, dt + o_sc, dt + o_ss, v.view_id, N, S, s0, s1, c->row_start.as<int>(), c->ch_cursor.as<int>(), c->cand_meta.as<uint2>(),
                               c->cand_depths.as<float4>(), (int)cap);
    }
    if (v.n_sources && sel->sort_apart) {
        ProfScope p(c, "exist");
        launch_exist_sort_runs(dt + o_sc, v.n_sources, N, S, c->row_start.as<int>(), c->cand_meta.as<uint2>(), c->cand_depths.as<float4>(), (int)cap, st, s0, s1,
                               c->vw_scratch.as<float>(), (long long)ccap + kVWSlack, c->cand_conf.as<unsigned>());
    }
    sel->wps = wps; sel->blocks_move = blocks_move;
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

// The consumers of the gathered blocks over all views' slots of the caller's: headers and ranges validated on the host (nothing else of a slot is an
// index to these kernels), every output filled with 0xff bytes, then the launches of shared_verdict, shard_pack, shard_products_local and retire_to.
int l3d_test_shard_pack(l3d_ctx* c, const unsigned char* gathered, const l3d_test_shard_geom* geom, l3d_test_shard_pack_io* io)
{
    if (!c) return L3D_ERR_INVALID;
    SlotPlan plan;
    if (int rc = test_shard_geom(c, geom, plan, "shard_pack")) return rc;
    const SlotGeom g = plan.geom;
    const int nv = geom ? geom->n_views : 0, W = g.world;
    if (!gathered || !io || nv < 1 || !io->verified || !io->best_off || !io->view_sn || io->n_batches < 0 || (io->n_batches > 0 && !io->batches) || io->arena_cap < 0 ||
        io->arena_cap > (1 << 26) || io->pack_cap < 0 || io->pack_cap > (1 << 26) || io->best_cap < 0 || io->best_cap > (1 << 26) || io->rt_cap < 0 || io->rt_cap > (1 << 28) ||
        !io->stage || !io->pack_hdr || !io->totals || !io->check || !io->base_dev || !io->hdr_all || !io->overflow ||
        (io->pack_cap > 0 && !io->pa_arena) || (io->arena_cap > 0 && !io->rt_arena) || (io->best_cap > 0 && (!io->pa_best || !io->pa_bestpos || !io->rt_best || !io->rt_bestpos)))
        return fail(c, L3D_ERR_INVALID, "shard_pack: bad argument");
    const bool tables = io->retire_tables != 0;
    if (tables && (!g.rt_off || !g.cam_off || !io->rt_off || (io->arena_cap > 0 && !io->qt_arena) || (io->rt_cap > 0 && !io->rt_all)))
        return fail(c, L3D_ERR_INVALID, "shard_pack: retire tables need a geometry with side words and run tables, rt_off, qt_arena and rt_all");
    const size_t nvs = (size_t)nv, block = (size_t)W * g.slot_bytes;
    long long pack_total = 0, all_records = 0;
    std::vector<unsigned long long> kept_base(nvs, 0);
    std::vector<int2> want_tot(nvs);
    for (int k = 0; k < nv; ++k) {
        const int S = io->view_sn[2 * k], N = io->view_sn[2 * k + 1];
        if (io->verified[k] > 1 || (io->keep && io->keep[k] > 1)) return fail(c, L3D_ERR_INVALID, "shard_pack: a flag that is not 0 or 1");
        if (S < 0 || S > geom->maxS || N < 1 || N > geom->maxN) return fail(c, L3D_ERR_INVALID, "shard_pack: a view larger than the geometry's largest");
        if (io->best_off[k] < 0 || io->best_off[k] + S > io->best_cap) return fail(c, L3D_ERR_INVALID, "shard_pack: a view's best pairs end past best_cap");
        if (tables && io->verified[k] && (!io->keep || io->keep[k]) && (io->rt_off[k] < 0 || io->rt_off[k] + ((long long)N + 1) * S > io->rt_cap))
            return fail(c, L3D_ERR_INVALID, "shard_pack: a view's run table ends past rt_cap");
        kept_base[(size_t)k] = (unsigned long long)pack_total;
        long long n = 0, R = 0;
        if (io->verified[k])
            for (int r = 0; r < W; ++r) {
                const SlotHeader* hd = reinterpret_cast<const SlotHeader*>(gathered + (size_t)k * block + (size_t)r * g.slot_bytes);
                const std::string bad = test_slot_header(*hd, g, S);
                if (!bad.empty()) return fail(c, L3D_ERR_INVALID, "shard_pack: view " + std::to_string(k) + ", rank " + std::to_string(r) + ": " + bad);
                n += hd->overflow ? 0 : hd->n_kept; R += hd->R;
            }
        want_tot[(size_t)k] = make_int2((int)n, (int)std::min(R, 0x7fffffffll));
        pack_total += n; all_records += n;
    }
    if (pack_total > io->pack_cap) return fail(c, L3D_ERR_INVALID, "shard_pack: the verified views keep " + std::to_string(pack_total) + " records: more than pack_cap");
    {
        int next = 0, at_before = 0;
        for (int b = 0; b < io->n_batches; ++b) {
            const int first = io->batches[3 * b], count = io->batches[3 * b + 1], at = io->batches[3 * b + 2];
            if (first != next || count < 1 || first + count > nv || at < at_before || at > nv) return fail(c, L3D_ERR_INVALID, "shard_pack: the batches are not contiguous and ascending from view 0");
            if (first + count > at) return fail(c, L3D_ERR_INVALID, "shard_pack: batch " + std::to_string(b) + " retires a view that is not exchanged yet");
            if ((long long)first + g.ring < at) return fail(c, L3D_ERR_INVALID, "shard_pack: batch " + std::to_string(b) + " reads a ring block that is already overwritten");
            next = first + count; at_before = at;
        }
    }

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipGetLastError();
    // (room behind every arena for all the records there are: a record filed at a wrong offset still lands in the buffer, and shows)
    const size_t slack = (size_t)all_records + 64, pcap = (size_t)io->pack_cap, acap = (size_t)io->arena_cap, bcap = (size_t)io->best_cap, rcap = (size_t)io->rt_cap;
    // small tables: verified | keep | best_off | kept_base | rt_off | view_sn | totals x 2 | check x 2 | pack headers | base_dev | hdr_all | overflow
    const size_t o_ver = 0, o_keep = align256(nvs), o_bo = o_keep + align256(nvs), o_kb = o_bo + align256(nvs * 8), o_ro = o_kb + align256(nvs * 8), o_sn = o_ro + align256(nvs * 8),
                 o_tot = o_sn + align256(nvs * 8), o_chk = o_tot + align256(2 * nvs * 8), o_ph = o_chk + 256, o_base = o_ph + align256(nvs * 32), o_hdr = o_base + align256((nvs + 2) * 8),
                 o_ovf = o_hdr + align256(nvs * W * 32), small = o_ovf + 256;
    HIPCHK(c, c->g0.reserve((size_t)nv * block + 256)); HIPCHK(c, c->g1.reserve((size_t)g.ring * block + 256)); HIPCHK(c, c->g2.reserve((nvs + 1) * plan.stage_bytes + 256));
    HIPCHK(c, c->g3.reserve(small)); HIPCHK(c, c->g4.reserve((pcap + acap + 2 * slack) * sizeof(Match))); HIPCHK(c, c->g5.reserve(2 * (bcap + 64) * 12));
    HIPCHK(c, c->g6.reserve((acap + slack) * 4)); HIPCHK(c, c->g7.reserve((rcap + 64) * 4));
    unsigned char* sm = c->g3.as<unsigned char>();
    unsigned char* full = c->g0.as<unsigned char>();
    unsigned char* ring = c->g1.as<unsigned char>();
    unsigned char* stage = c->g2.as<unsigned char>();
    Match* pa_arena = c->g4.as<Match>();
    Match* rt_arena = pa_arena + pcap + slack;
    float2* pa_best = c->g5.as<float2>();
    float2* rt_best = pa_best + bcap + 64;
    int* pa_bpos = reinterpret_cast<int*>(rt_best + bcap + 64);
    int* rt_bpos = pa_bpos + bcap + 64;
    HIPCHK(c, hipMemcpyAsync(full, gathered, (size_t)nv * block, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(ring, 0xff, (size_t)g.ring * block, st));
    HIPCHK(c, hipMemsetAsync(stage, 0xff, nvs * plan.stage_bytes, st));
    HIPCHK(c, hipMemsetAsync(sm, 0xff, small, st));
    HIPCHK(c, hipMemsetAsync(c->g4.p, 0xff, (pcap + acap + 2 * slack) * sizeof(Match), st));
    HIPCHK(c, hipMemsetAsync(c->g5.p, 0xff, 2 * (bcap + 64) * 8, st));
    HIPCHK(c, hipMemsetAsync(pa_bpos, 0x7f, 2 * (bcap + 64) * 4, st));
    HIPCHK(c, hipMemsetAsync(c->g6.p, 0xff, (acap + slack) * 4, st));
    HIPCHK(c, hipMemsetAsync(c->g7.p, 0xff, (rcap + 64) * 4, st));
    HIPCHK(c, hipMemcpyAsync(sm + o_ver, io->verified, nvs, hipMemcpyHostToDevice, st));
    if (io->keep) HIPCHK(c, hipMemcpyAsync(sm + o_keep, io->keep, nvs, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(sm + o_bo, io->best_off, nvs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(sm + o_kb, kept_base.data(), nvs * 8, hipMemcpyHostToDevice, st));
    if (tables) HIPCHK(c, hipMemcpyAsync(sm + o_ro, io->rt_off, nvs * 8, hipMemcpyHostToDevice, st));
    else HIPCHK(c, hipMemsetAsync(sm + o_ro, 0, nvs * 8, st));
    HIPCHK(c, hipMemcpyAsync(sm + o_sn, io->view_sn, nvs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(sm + o_chk, 0, 256, st));                                   // (both kernels' answers are ORs and maxima into zeroed words)
    HIPCHK(c, hipMemsetAsync(sm + o_base, 0, (nvs + 2) * 8, st));                        // (the run starts the offsets at zero: setup_ring_tables)
    HIPCHK(c, hipMemsetAsync(sm + o_ovf, 0, 4, st));
    const unsigned char* ver = sm + o_ver;
    int2* tot = reinterpret_cast<int2*>(sm + o_tot);
    int* chk = reinterpret_cast<int*>(sm + o_chk);
    SlotHeader* hdr_all = reinterpret_cast<SlotHeader*>(sm + o_hdr);

    // ---- the headers in front of the slots: totals, verdict; the hand-over of every verified view; all views into one arena
    hipLaunchKernelGGL(k_shard_totals, dim3((nv + 255) / 256), dim3(256), 0, st, full, g.slot_bytes, g, ver, nv, tot);
    hipLaunchKernelGGL(k_check_slots, dim3(8), dim3(256), 0, st, full, g.slot_bytes, g, ver, nv, chk);
    std::vector<int2> got_tot(nvs);
    HIPCHK(c, hipMemcpyAsync(got_tot.data(), tot, nvs * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    // (the products lay the arena out from these totals: a kernel that counts differently than the host did must not place a record)
    for (int k = 0; k < nv; ++k)
        if (got_tot[(size_t)k].x != want_tot[(size_t)k].x) return fail(c, L3D_ERR_INVALID, "shard_pack: k_shard_totals counts " + std::to_string(got_tot[(size_t)k].x) + " kept records in view " + std::to_string(k) + ", the headers add up to " + std::to_string(want_tot[(size_t)k].x));
    for (int k = 0; k < nv; ++k)
        if (io->verified[k])
            hipLaunchKernelGGL(k_pack_view, dim3(8, W), dim3(256), 0, st, full + (size_t)k * block, g, stage + (size_t)k * plan.stage_bytes, reinterpret_cast<PackHeader*>(sm + o_ph) + k);
    hipLaunchKernelGGL(k_shard_pack_all, dim3(8, W, nv), dim3(256), 0, st, full, g, ver, reinterpret_cast<const unsigned long long*>(sm + o_kb), reinterpret_cast<const long long*>(sm + o_bo),
                       pa_arena, pa_best, pa_bpos);
    // ---- the ring: blocks arrive as the exchanges bring them, batches leave as listed
    int exchanged = 0;
    for (int b = 0; b < io->n_batches; ++b) {
        const int first = io->batches[3 * b], count = io->batches[3 * b + 1], at = io->batches[3 * b + 2];
        for (; exchanged < at; ++exchanged) {
            unsigned char* dst = ring + (size_t)(exchanged % g.ring) * block;
            if (io->verified[exchanged]) HIPCHK(c, hipMemcpyAsync(dst, full + (size_t)exchanged * block, block, hipMemcpyDeviceToDevice, st));
            else HIPCHK(c, hipMemsetAsync(dst, 0, block, st));
        }
        ProfScope p(c, "retire", st);
        hipLaunchKernelGGL(k_shard_retire, dim3(8, W, count), dim3(256), 0, st, ring, g, ver, io->keep ? sm + o_keep : nullptr, first, count, reinterpret_cast<long long*>(sm + o_base),
                           (long long)io->arena_cap, reinterpret_cast<const long long*>(sm + o_bo), rt_arena, rt_best, rt_bpos, hdr_all, reinterpret_cast<int*>(sm + o_ovf),
                           tables ? c->g6.as<unsigned>() : nullptr, tables ? c->g7.as<int>() : nullptr, reinterpret_cast<const long long*>(sm + o_ro), reinterpret_cast<const int2*>(sm + o_sn));
    }
    // ---- the compact header table the retire run left: totals and verdict again
    hipLaunchKernelGGL(k_shard_totals, dim3((nv + 255) / 256), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(hdr_all), sizeof(SlotHeader), g, ver, nv, tot + nvs);
    hipLaunchKernelGGL(k_check_slots, dim3(8), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(hdr_all), sizeof(SlotHeader), g, ver, nv, chk + 3);

    HIPCHK(c, hipMemcpyAsync(io->stage, stage, nvs * plan.stage_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(io->pack_hdr, sm + o_ph, nvs * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(io->totals, tot, 2 * nvs * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(io->check, chk, 24, hipMemcpyDeviceToHost, st));
    if (pcap) HIPCHK(c, hipMemcpyAsync(io->pa_arena, pa_arena, pcap * sizeof(Match), hipMemcpyDeviceToHost, st));
    if (acap) HIPCHK(c, hipMemcpyAsync(io->rt_arena, rt_arena, acap * sizeof(Match), hipMemcpyDeviceToHost, st));
    if (bcap) {
        HIPCHK(c, hipMemcpyAsync(io->pa_best, pa_best, bcap * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(io->rt_best, rt_best, bcap * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(io->pa_bestpos, pa_bpos, bcap * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(io->rt_bestpos, rt_bpos, bcap * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipMemcpyAsync(io->base_dev, sm + o_base, (nvs + 2) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(io->hdr_all, hdr_all, nvs * W * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(io->overflow, sm + o_ovf, 4, hipMemcpyDeviceToHost, st));
    if (acap && io->qt_arena) HIPCHK(c, hipMemcpyAsync(io->qt_arena, c->g6.p, acap * 4, hipMemcpyDeviceToHost, st));
    if (rcap && io->rt_all) HIPCHK(c, hipMemcpyAsync(io->rt_all, c->g7.p, rcap * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    // the room behind the arenas must be as it was
    {
        std::vector<unsigned char> tail(slack * sizeof(Match));
        for (const Match* a : { pa_arena + pcap, rt_arena + acap }) {
            HIPCHK(c, hipMemcpy(tail.data(), a, tail.size(), hipMemcpyDeviceToHost));
            for (unsigned char x : tail) if (x != 0xff) return fail(c, L3D_ERR_INVALID, "shard_pack: a kernel wrote behind its arena");
        }
    }
    return L3D_OK;
}

}  // extern "C"

void l3d::warm_chain_sharded() { touch_kernel(reinterpret_cast<const void*>(&l3d::k_exist_count_slots)); }
