// l3d_chain_partition.hip -- matchViews over the ranks of a job by BLOCKS OF VIEWS: every rank runs the single-GPU chain (l3d_chain.hip:
// run_chain) on its block.  Two ways to give a block its sources: all ranks at once, speculatively, with collectives (l3d_match_chain_blocks,
// l3d_match_chain_partition), or one after the other on one device, each handed its predecessor's tail (match_chain_turn).  What a rank's
// share of the products needs from views it does not hold -- the early-return quirk -- is packed, ingested and built by ONE set of functions
// (below the kernels); the two callers differ in how the pieces travel: through exchanges, or through a store on the device.
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "l3d_ctx.hpp"
#include "l3d_products.hpp"
#include "l3d_chain_common.hpp"
#include "l3d_blocks_rule.hpp"
#include "l3d_chain_partition.hpp"
#include "l3d_turns.hpp"

using namespace l3d;

// =================================================================================================================================
// matchViews sharded by BLOCKS OF VIEWS, speculatively, with exact verification (round 4).
//
// The chain over views has a short memory: started cold at view B - L (nothing known about earlier views), its kept lists become
// bit-identical to the true chain's after about three neighbour windows (measured: scripts/speculate_blocks.py).  So rank r of `world`
// runs the ordinary single-GPU chain -- full-width kernels, no per-view collective -- on views [B_r - warmup, B_{r+1}) only, and the ranks
// then CHECK the speculation: every rank publishes a 64-bit digest of every kept list it computed; rank r's block is exact if rank r-1's is
// and the `window` views in front of B_r came out of rank r's warm-up exactly as rank r-1 (whose block they belong to) computed them --
// from B_r on every view then has the same inputs as in the one chain, and the same arithmetic.  All ranks read the same gathered table,
// so all reach the same verdict without another collective.  When it holds, the ranks all-gather their blocks' kept records (+ best depth
// pairs / positions), lay them out as the one chain's arena and build matchViews' products from it (l3d_products.hip, unchanged).  When it
// does not, nothing is committed and the caller takes the segment-sharded run (l3d_shard_chain_run), whose result needs no speculation.
// The rules -- block_begin, blocks_reach, blocks_verdict, blocks_handover_plan -- are pure functions of l3d_blocks_rule.hpp.
namespace l3d {

// order-sensitive 64-bit digest of a view's kept records: sum over records of a mix of (index, the record's eight words)
__global__ __launch_bounds__(256) void k_block_digest(const Match* __restrict__ arena, const ChainResult* __restrict__ res, int k_begin, BlockDigest* __restrict__ out)
{
    const int k = k_begin + blockIdx.y;
    const ChainResult r = res[k];
    unsigned long long h = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < r.n_kept; i += gridDim.x * 256) {
        const uint4* w = reinterpret_cast<const uint4*>(arena + r.kept_base + i);
        const uint4 a = w[0], b = w[1];
        unsigned long long x = 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
        const unsigned v[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
        for (int q = 0; q < 8; ++q) { x ^= v[q]; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 29; }
        h += x;
    }
    for (int o = 32; o > 0; o >>= 1) h += __shfl_down(h, o);
    if ((threadIdx.x & 63) == 0 && h) atomicAdd(&out[k].hash, h);
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[k].n_kept = r.n_kept; out[k].R = r.R; }
}

}  // namespace l3d

// k_block_digest over the kept lists of the resident products, whoever built them: hash[k] / n_kept[k] of every chain view (0 / 0: nothing of
// the view is held here).  What two ranks that took turns on one device compare of the views both held, before the records are released.
extern "C" int l3d_chain_records_digest(l3d_ctx* c, uint64_t* hash, int32_t* n_kept, int n)
{
    if (!c) return L3D_ERR_INVALID;
    Products& P = c->products;
    if (!hash || !n_kept || n < 0) return fail(c, L3D_ERR_INVALID, "l3d_chain_records_digest: bad argument");
    if (!P.valid || n != P.n_chain || (int)P.res.size() != n) return fail(c, L3D_ERR_INVALID, "l3d_chain_records_digest: no resident products of that many chain views");
    if (c->records_released) return fail(c, L3D_ERR_INVALID, "l3d_chain_records_digest: the kept records of this chain were released (l3d_chain_release_records)");
    if (n == 0) return L3D_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // every list must lie inside the arena: the kernel trusts the records' table
    for (int k = 0; k < n; ++k) {
        const ChainResult& r = P.res[(size_t)k];
        if (r.n_kept < 0 || (r.n_kept > 0 && ((size_t)r.kept_base + (size_t)r.n_kept) * sizeof(Match) > c->ch_kept.cap))
            return fail(c, L3D_ERR_INVALID, "l3d_chain_records_digest: a kept list lies outside the arena");
    }
    const size_t o_dig = ((size_t)n * sizeof(ChainResult) + 255) & ~(size_t)255;
    HIPCHK(c, c->g7.reserve(o_dig + (size_t)n * sizeof(BlockDigest) + 64));
    ChainResult* dres = c->g7.as<ChainResult>();
    BlockDigest* dd = reinterpret_cast<BlockDigest*>(c->g7.as<unsigned char>() + o_dig);
    HIPCHK(c, hipMemcpyAsync(dres, P.res.data(), (size_t)n * sizeof(ChainResult), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(dd, 0, (size_t)n * sizeof(BlockDigest), st));
    for (int k0 = 0; k0 < n; k0 += 32768)        // (a launch's second grid dimension holds 65 535 blocks)
        hipLaunchKernelGGL(k_block_digest, dim3(16, (unsigned)std::min(32768, n - k0)), dim3(256), 0, st, c->ch_kept.as<Match>(), dres, k0, dd);
    std::vector<BlockDigest> hd((size_t)n);
    HIPCHK(c, hipMemcpyAsync(hd.data(), dd, (size_t)n * sizeof(BlockDigest), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (int k = 0; k < n; ++k) { hash[k] = hd[(size_t)k].hash; n_kept[k] = hd[(size_t)k].n_kept; }
    return L3D_OK;
}

namespace l3d {

// one source's records that point at an early-return view, in list order (stable): out == nullptr counts only
__global__ __launch_bounds__(256) void k_early_pack(const Match* __restrict__ arena, const ChainResult* __restrict__ res, const int* __restrict__ group_src,
                                                    const unsigned* __restrict__ early_ids, int n_early, const long long* __restrict__ out_off, Match* __restrict__ out, int* __restrict__ counts)
{
    __shared__ int s_w[4];
    const ChainResult r = res[group_src[blockIdx.x]];
    const Match* kept = arena + r.kept_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long off = out ? out_off[blockIdx.x] : 0;
    int total = 0;
    for (int b = 0; b < r.n_kept; b += 256) {
        const int i = b + tid;
        Match m;
        bool on = false;
        if (i < r.n_kept) { m = kept[i]; for (int e = 0; e < n_early; ++e) on = on || m.camID2 == early_ids[e]; }
        const unsigned long long bal = __ballot(on);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; ++w) { if (w < wave) before += s_w[w]; all += s_w[w]; }
        if (on && out) out[off + before + __popcll(bal & ((1ull << lane) - 1ull))] = m;
        off += all; total += all;
        __syncthreads();
    }
    if (tid == 0 && !out) counts[blockIdx.x] = total;
}

// one view's best matches as a package other ranks can build its hypotheses from: [view, R, n, S | position of every segment's best match in the
// compact list or -1 | best depth pairs | the best records, compact, in segment order (room for S)]
__global__ __launch_bounds__(256) void k_alias_pack(const Match* __restrict__ arena, const ChainResult* __restrict__ res, const int* __restrict__ pk_view, const int* __restrict__ pk_S,
                                                    const long long* __restrict__ pk_best_off, const long long* __restrict__ pk_out_off, const float2* __restrict__ best_all,
                                                    const int* __restrict__ bestpos_all, unsigned char* __restrict__ out)
{
    __shared__ int s_w[4];
    const int k = pk_view[blockIdx.x], S = pk_S[blockIdx.x];
    const ChainResult r = res[k];
    const float2* best = best_all + pk_best_off[blockIdx.x];
    const int* bestpos = bestpos_all + pk_best_off[blockIdx.x];
    unsigned char* o = out + pk_out_off[blockIdx.x];
    int* o_pos = reinterpret_cast<int*>(o + 16);
    float2* o_best = reinterpret_cast<float2*>(o + 16 + (size_t)S * 4);
    Match* o_rec = reinterpret_cast<Match*>(o + 16 + (size_t)S * 12);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int off = 0;
    for (int b = 0; b < S; b += 256) {
        const int s = b + tid;
        const int p = s < S ? bestpos[s] : -1;
        const bool on = p >= 0 && r.n_kept > 0;
        const unsigned long long bal = __ballot(on);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; ++w) { if (w < wave) before += s_w[w]; all += s_w[w]; }
        if (s < S) {
            const int q = on ? off + before + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
            o_pos[s] = q; o_best[s] = best[s];
            if (on) o_rec[q] = arena[r.kept_base + p];
        }
        off += all;
        __syncthreads();
    }
    if (tid == 0) { int* h = reinterpret_cast<int*>(o); h[0] = k; h[1] = r.R; h[2] = off; h[3] = S; }
}

}  // namespace l3d

// =================================================================================================================================
// What the partition and the turns share.  Every function returns a code with the message set (fail); none knows who calls it: `who` is only
// the prefix of its messages, `grow` the caller's way to make room in the kept arena.
namespace {

// useful work of a rank = the stage-1 pairs of its own block
double block_pairs(const l3d_chain_view* views, int own0, int own1)
{
    double p = 0;
    for (int k = own0; k < own1; ++k)
        for (int j = 0; j < views[k].n_tbm; ++j) p += (double)views[k].S_src * views[k].offsets[2 * views[k].to_be_matched[j] + 1];
    return p;
}
// offsets of the views' slices in the whole-run arrays of best pairs / positions (chain_assign_arenas: verified views back to back)
std::vector<long long> best_offsets(const l3d_chain_view* views, int n_views)
{
    std::vector<long long> best_off((size_t)n_views + 1, 0);
    for (int k = 0; k < n_views; ++k) best_off[(size_t)k + 1] = best_off[(size_t)k] + (views[k].n_tbm > 0 ? views[k].S_src : 0);
    return best_off;
}

// a run of views as one byte stream [records | best depth pairs | best positions]
struct TailLayout {
    size_t o_best, o_bpos, bytes;
    TailLayout(long long records, long long segments)
        : o_best(align256((size_t)records * sizeof(Match))), o_bpos(o_best + align256((size_t)segments * 8)), bytes(o_bpos + align256((size_t)segments * 4)) {}
};
// such a stream at `base` on the device, holding the views [k0, k1), as what a chain that starts at k1 takes over
ChainPreload tail_preload(const void* base, size_t o_best, size_t o_bpos, int k0, int k1, std::vector<int> n_kept, std::vector<int> R)
{
    ChainPreload pre;
    pre.k0 = k0; pre.k1 = k1;
    const unsigned char* G = static_cast<const unsigned char*>(base);
    pre.records = reinterpret_cast<const Match*>(G);
    pre.best = reinterpret_cast<const float2*>(G + o_best);
    pre.bestpos = reinterpret_cast<const int*>(G + o_bpos);
    pre.n_kept = std::move(n_kept); pre.R = std::move(R);
    return pre;
}
// what build_products reads per chain view: a verified view's slices of the whole-run arrays of best pairs / positions (here: per view, whether this
// rank has them; nullptr: every view's)
std::vector<ProdChainView> prod_chain_views(l3d_ctx* c, const l3d_chain_view* views, int n_views, const long long* best_off, const char* here)
{
    std::vector<ProdChainView> pvh((size_t)n_views);
    for (int k = 0; k < n_views; ++k) {
        const bool ver = views[k].n_tbm > 0, on = ver && (!here || here[k]);
        pvh[(size_t)k].verified = ver ? 1 : 0;
        pvh[(size_t)k].best = on ? c->ch_best.as<float2>() + best_off[(size_t)k] : nullptr;
        pvh[(size_t)k].bestpos = on ? c->ch_bestpos.as<int>() + best_off[(size_t)k] : nullptr;
    }
    return pvh;
}

// ---- the early-return views of a schedule with what the quirk couples them to (cudawrapper.cu:877-878, line3D.cc:861-865)
struct TurnEarly {
    int view = 0;
    std::vector<int> src;           // verified earlier views whose records point at it (ProdSrc of l3d_products.hip)
    std::vector<int> alias_rows;    // the views those sources' LOCAL camera numbers name: their rows get entries that name this view's segments
    std::vector<int> alias_best;    // the verified views any of its local camera numbers names: k_alias_pack packages
};
// the only early-return analysis of a schedule
struct EarlyReturns {
    std::vector<TurnEarly> views;   // in chain order
    std::vector<unsigned> ids;      // their view ids
    std::vector<int> groups;        // every source of one, ascending, unique: k_early_pack groups
    std::vector<int> alias;         // every verified view a local camera number of one names, ascending, unique: k_alias_pack packages
    // what k_early_pack's control block holds: a schedule with more is refused
    static constexpr size_t kMaxViews = 64, kMaxGroups = 480;
    bool fits() const { return views.size() <= kMaxViews && groups.size() <= kMaxGroups; }
};
EarlyReturns turn_early_views(const l3d_chain_view* views, int n, const ScheduleIndex& index)
{
    EarlyReturns E;
    for (int k = 0; k < n; ++k) {
        if (views[k].n_tbm != 0 || views[k].n_sources == 0) continue;
        TurnEarly e;
        e.view = k;
        for (int q = 0; q < views[k].n_sources; ++q) {
            const int si = views[k].source_index[q], b = index.find((unsigned)views[k].source_cam[q]);
            const bool valid = si >= 0 && si < k && views[si].n_tbm > 0;
            if (valid) { e.src.push_back(si); E.groups.push_back(si); if (b >= 0) e.alias_rows.push_back(b); }
            if (b >= 0 && views[b].n_tbm > 0) e.alias_best.push_back(b);
        }
        E.alias.insert(E.alias.end(), e.alias_best.begin(), e.alias_best.end());
        E.ids.push_back(views[k].view_id);
        E.views.push_back(e);
    }
    for (std::vector<int>* v : { &E.groups, &E.alias }) { std::sort(v->begin(), v->end()); v->erase(std::unique(v->begin(), v->end()), v->end()); }
    return E;
}

// ---- k_early_pack: the records of a rank's sources (`groups`) that point at an early-return view, in two passes.  Its control block in ch_send, which
// the caller reserves (EarlyPackCtl::bytes + 256) and leaves alone between the passes:
// [ids of the early-return views | the groups | where each group's records go | each group's count]
struct EarlyPackCtl { static constexpr size_t o_ids = 0, o_grp = 256, o_off = o_grp + 2048, o_cnt = o_off + 4096, bytes = o_cnt + 2048; };
static_assert(EarlyReturns::kMaxViews * 4 <= 256 && EarlyReturns::kMaxGroups * 4 <= 2048 && EarlyReturns::kMaxGroups * 8 <= 4096, "control block of k_early_pack");

void launch_early_pack(l3d_ctx* c, size_t n_groups, size_t n_early, Match* dst, hipStream_t st)      // dst == nullptr: count
{
    unsigned char* S0 = c->ch_send.as<unsigned char>();
    hipLaunchKernelGGL(k_early_pack, dim3((unsigned)n_groups), dim3(256), 0, st, c->ch_kept.as<Match>(), c->ch_res.as<ChainResult>(), reinterpret_cast<const int*>(S0 + EarlyPackCtl::o_grp),
                       reinterpret_cast<const unsigned*>(S0 + EarlyPackCtl::o_ids), (int)n_early, dst ? reinterpret_cast<const long long*>(S0 + EarlyPackCtl::o_off) : nullptr, dst,
                       dst ? nullptr : reinterpret_cast<int*>(S0 + EarlyPackCtl::o_cnt));
}
// pass 1: cnt[g] = the records of groups[g] that point at one of early_ids
int count_early_records(l3d_ctx* c, const std::vector<unsigned>& early_ids, const std::vector<int>& groups, std::vector<int>& cnt, hipStream_t st)
{
    cnt.assign(groups.size(), 0);
    if (groups.empty()) return L3D_OK;
    unsigned char* S0 = c->ch_send.as<unsigned char>();
    HIPCHK(c, hipMemcpyAsync(S0 + EarlyPackCtl::o_ids, early_ids.data(), early_ids.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S0 + EarlyPackCtl::o_grp, groups.data(), groups.size() * 4, hipMemcpyHostToDevice, st));
    launch_early_pack(c, groups.size(), early_ids.size(), nullptr, st);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), S0 + EarlyPackCtl::o_cnt, groups.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return L3D_OK;
}
// pass 2: the groups' records to dst, back to back in the order of the groups (room for the sum of cnt); returns with the stream idle
int pack_early_records(l3d_ctx* c, const char* who, size_t n_early, const std::vector<int>& cnt, Match* dst, hipStream_t st)
{
    std::vector<long long> offs(cnt.size(), 0);
    long long total = 0;
    for (size_t g = 0; g < cnt.size(); ++g) { offs[g] = total; total += cnt[g]; }
    if (total > 0) {
        HIPCHK(c, hipMemcpyAsync(c->ch_send.as<unsigned char>() + EarlyPackCtl::o_off, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, st));
        launch_early_pack(c, cnt.size(), n_early, dst, st);
    }
    const hipError_t e = hipStreamSynchronize(st);      // (offs is a stack vector)
    if (e != hipSuccess) return fail(c, L3D_ERR_HIP, std::string(who) + ": packing the early-return records: " + hipGetErrorString(e));
    return L3D_OK;
}

// ---- k_alias_pack: the best matches of the views in pk_view as packages, back to back in dst (alias_package_bytes each).  The control vectors go
// through ch_send, which the caller reserves (alias_ctl_bytes); returns with the stream idle
size_t alias_package_bytes(int S) { return align256(16 + (size_t)S * (12 + sizeof(Match))); }
size_t alias_ctl_bytes(size_t n) { return align256(n * 4) * 2 + align256(n * 8) * 2 + 256; }
int pack_alias_packages(l3d_ctx* c, const char* who, const l3d_chain_view* views, const std::vector<int>& pk_view, const long long* best_off, unsigned char* dst, hipStream_t st)
{
    const size_t n = pk_view.size();
    if (n == 0) return L3D_OK;
    std::vector<int> pk_S;
    std::vector<long long> pk_bo, pk_oo;
    size_t o = 0;
    for (int b : pk_view) { pk_S.push_back(views[b].S_src); pk_bo.push_back(best_off[(size_t)b]); pk_oo.push_back((long long)o); o += alias_package_bytes(views[b].S_src); }
    unsigned char* S0 = c->ch_send.as<unsigned char>();
    const size_t o1 = align256(n * 4), o2 = 2 * align256(n * 4), o3 = o2 + align256(n * 8);
    hipError_t e = hipMemcpyAsync(S0, pk_view.data(), n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(S0 + o1, pk_S.data(), n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(S0 + o2, pk_bo.data(), n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(S0 + o3, pk_oo.data(), n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_alias_pack, dim3((unsigned)n), dim3(256), 0, st, c->ch_kept.as<Match>(), c->ch_res.as<ChainResult>(), reinterpret_cast<const int*>(S0), reinterpret_cast<const int*>(S0 + o1),
                           reinterpret_cast<const long long*>(S0 + o2), reinterpret_cast<const long long*>(S0 + o3), c->ch_best.as<float2>(), c->ch_bestpos.as<int>(), dst);
        e = hipStreamSynchronize(st);                   // (the control vectors are on the stack)
    }
    if (e != hipSuccess) return fail(c, L3D_ERR_HIP, std::string(who) + ": packing the alias views' best matches: " + hipGetErrorString(e));
    return L3D_OK;
}

// ---- a rank's share: the one chain's records of the views [held0, held1) it holds, and behind them in its arena what it ingests of views it does not hold
struct ShareState {
    std::vector<ChainResult> hloc;          // per chain view: its list in this rank's arena (zero: nothing of it is here)
    long long used = 0;                     // records of the arena in use
    std::vector<char> alias_known;          // per chain view: its best matches came in a package
    const long long* best_off;
    ShareState(const ChainResult* hres, int n_views, int held0, int held1, const long long* best_off_) : hloc((size_t)n_views), alias_known((size_t)n_views, 0), best_off(best_off_)
    {
        for (int k = 0; k < n_views; ++k) { hloc[(size_t)k] = ChainResult(); if (k >= held0 && k < held1) { hloc[(size_t)k] = hres[k]; used = std::max(used, (long long)hres[k].kept_base + hres[k].n_kept); } }
    }
};
// the kept arena grown with an eighth on top, its first used_records kept (DevBuf::grow_keep: behind the copies the ingests queued on the stream)
int arena_grow_keep(l3d_ctx* c, size_t records, size_t used_records)
{
    if (records * sizeof(Match) <= c->ch_kept.cap) return L3D_OK;
    const size_t want = records * sizeof(Match) + records * sizeof(Match) / 8 + 4096;
    const hipError_t e = c->ch_kept.grow_keep(want, used_records * sizeof(Match), c->stream);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(c, L3D_ERR_NOMEM, "growing the kept arena to " + std::to_string(want >> 20) + " MB"); }
    if (e != hipSuccess) return fail(c, L3D_ERR_HIP, std::string("copying the kept arena over: ") + hipGetErrorString(e));
    return L3D_OK;
}
// a share's way to make room for `records` records in the kept arena, the first `used_records` of them kept.  room: what a turn's arena may hold
// under option regrow_free_mb (match_chain_turn; 0: no cap -- the partition)
struct ArenaGrow {
    l3d_ctx* c; size_t room; int rank;
    int operator()(long long records, long long used_records) const
    {
        if (room && (size_t)records > room)
            return fail(c, L3D_ERR_NOMEM, "match_chain_turn: the arena of rank " + std::to_string(rank) + " needs " + std::to_string(records) + " records with the slices of the views it does not hold, there is room for " +
                                          std::to_string(room) + " (" + std::to_string(c->opt.regrow_free_mb) + " MB at " + std::to_string(sizeof(Match) + 4) + " B per record)");
        return arena_grow_keep(c, (size_t)records + 64, (size_t)used_records);
    }
};
// a source this rank does not hold gets a list of its own: just its n records (at src, on the device) that point at early-return views, in list order
int ingest_early_slice(l3d_ctx* c, ShareState& sh, int si, const Match* src, int n, const ArenaGrow& grow, hipStream_t st)
{
    if (int rc = grow(sh.used + n, sh.used)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ch_kept.as<Match>() + sh.used, src, (size_t)n * sizeof(Match), hipMemcpyDeviceToDevice, st));
    ChainResult& x = sh.hloc[(size_t)si];
    x.kept_base = (uint64_t)sh.used; x.n_kept = n; x.R = n; x.overflow = 0;
    sh.used += n;
    return L3D_OK;
}
// view b, which this rank does not hold, gets its best matches from the package pk (on the device): the compact list of the best records behind
// `used`, positions and depth pairs in the view's slices of the whole-run arrays
int ingest_alias_package(l3d_ctx* c, const char* who, ShareState& sh, const l3d_chain_view* views, int b, const unsigned char* pk, const ArenaGrow& grow, hipStream_t st)
{
    int h[4] = { 0, 0, 0, 0 };
    HIPCHK(c, hipMemcpyAsync(h, pk, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int S = views[b].S_src;
    if (h[0] != b || h[3] != S || h[2] < 0 || h[2] > S) return fail(c, L3D_ERR_INVALID, std::string(who) + ": a package of best matches does not name the view it should");
    //  a view this rank does not hold can be BOTH a source of an early-return view -- its list here is then the sliver of
    // records that point at that view -- and a view an early return's local numbers name: one list cannot be both, and the best matches
    // would replace the sliver silently.  No scene of the tests does this; a job that does is refused here, on every rank alike
    if (sh.hloc[(size_t)b].n_kept > 0) return fail(c, L3D_ERR_UNSUPPORTED, std::string(who) + ": view " + std::to_string(views[b].view_id) + " is a source of an early-return view and named by an early return's local camera number");
    if (int rc = grow(sh.used + h[2], sh.used)) return rc;
    if (h[2] > 0) HIPCHK(c, hipMemcpyAsync(c->ch_kept.as<Match>() + sh.used, pk + 16 + (size_t)S * 12, (size_t)h[2] * sizeof(Match), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ch_bestpos.as<int>() + sh.best_off[(size_t)b], pk + 16, (size_t)S * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ch_best.as<float2>() + sh.best_off[(size_t)b], pk + 16 + (size_t)S * 4, (size_t)S * 8, hipMemcpyDeviceToDevice, st));
    ChainResult& x = sh.hloc[(size_t)b];
    x.kept_base = (uint64_t)sh.used; x.n_kept = h[2]; x.R = h[1]; x.overflow = 0;
    sh.used += h[2];
    sh.alias_known[(size_t)b] = 1;
    return L3D_OK;
}

// the local products of a rank with the ranges t (l3d_turns.hpp: it holds [pre0, run1), builds the rows of [row0, row1), owns [own0, own1)): the rows of
// the table, best matches and medians for every view it holds.  part, n_local: what share_file files once the caller knows the entries over all ranks
int share_build(l3d_ctx* c, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int rank, int world, const TurnRange& t,
                const ShareState& sh, ProductsPart& part, int64_t& n_local)
{
    std::vector<char> held((size_t)n_views, 0), here((size_t)n_views, 0);
    for (int k = 0; k < n_views; ++k) {
        held[(size_t)k] = k >= t.pre0 && k < t.run1 ? 1 : 0;
        here[(size_t)k] = held[(size_t)k] || sh.alias_known[(size_t)k] ? 1 : 0;
    }
    const std::vector<ProdChainView> pvh = prod_chain_views(c, views, n_views, sh.best_off, here.data());
    part = products_part(views, n_views, map, rank, world, t.own0, t.own1, t.row0, t.row1, t.pre0, t.run1);
    n_local = 0;
    return build_products(c, views, n_views, pvh.data(), sh.hloc.data(), map, summary, &n_local, part.row_dv0, part.row_dv1, held.data());
}
void share_file(l3d_ctx* c, int n_views, const TurnRange& t, const ShareState& sh, ProductsPart part, int64_t n_local, long long n_pot_all)
{
    part.n_pot_all = n_pot_all;
    c->products.part = part;
    c->products.n_pot = n_local;
    c->products.valid = true;
    memcpy(c->ch_pin_res.as<ChainResult>(), sh.hloc.data(), (size_t)n_views * sizeof(ChainResult));       // (what l3d_chain_kept_list reads)
    double kept = 0, raw = 0;
    for (int k = t.own0; k < t.own1; ++k) { kept += sh.hloc[(size_t)k].n_kept; raw += sh.hloc[(size_t)k].R; }      // (this rank's block)
    c->stats[3] = kept; c->stats[1] = raw;
}

}  // namespace

// =================================================================================================================================
// One call of l3d_match_chain_blocks (partition = false: every rank ends up with the whole arena and the whole table, replicas for the finishing
// stages) or of l3d_match_chain_partition (true: nothing is replicated, include/line3d_amd.h), as its phases: run() below.
//   THE FAILURE PROTOCOL.  Everything a rank can fail in ON ITS OWN between two collectives (an allocation, a copy, a launch, its chain) is collected in
// local_rc -- note(rc), soft(hip error) -- and travels with the next exchange of status words, all_gather_word: a failed rank still enters it, with a
// mark every rank reads, and then all of them return -- nobody is left waiting.  So from the first collective to the last a phase returns non-zero
// only out of an exchange that failed (every rank's does) or out of all_gather_word (every rank's does); whatever else goes wrong is noted.
namespace {

struct BlocksRun {
    l3d_ctx* const c; const l3d_chain_view* const views; const int n_views; const l3d_dense_map* const map; l3d_chain_summary* const summary; int64_t* const n_pot;
    const int rank, world, warmup_views, window; const l3d_exchange_fn exchange; void* const exchange_user; int* const verdict; const bool partition;
    const ScheduleIndex index;
    const std::vector<long long> best_off;
    hipStream_t st = nullptr;
    int reach = 0, tail = 0, check = 0;                 // blocks_reach
    int own0 = 0, own1 = 0, first = 0, last = 0;        // this rank's block; the views its chain runs over
    bool releases = false;                              // partitioned: what only a running chain needs is given back before the products are built
    std::vector<char> verified; std::vector<int> S_src; // per view, for blocks_handover_plan
    int local_rc = L3D_OK; std::string local_err;       // the first failure of this rank alone, with its message
    size_t tab_bytes = 0;
    BlockDigest *dtab_own = nullptr, *dtab_all = nullptr;       // device: this rank's digest table, everybody's
    long long *st_own = nullptr, *st_all = nullptr;             // device: this rank's status word, everybody's (256 bytes apart)
    std::vector<BlockDigest> tab;                       // everybody's digest tables, world x n_views
    std::vector<long long> words;                       // everybody's status words of the last all_gather_word
    std::vector<int> comp_from;                         // per rank: the first view it computed (or took over); every rank keeps the same table
    const ChainResult* hres = nullptr;
    int arena_first = 0;                                // first view whose records sit in this rank's arena
    int exact_from = 0;                                 // first view from which this rank's lists are the one chain's (once nobody misses)
    int rounds = 0, blocks_rerun = 0;
    double t0 = 0, t1 = 0, t2 = 0;

    BlocksRun(l3d_ctx* c_, const l3d_chain_view* views_, int n_views_, const l3d_dense_map* map_, l3d_chain_summary* summary_, int64_t* n_pot_, int rank_, int world_, int warmup_views_,
              int window_, l3d_exchange_fn exchange_, void* exchange_user_, int* verdict_, bool partition_)
        : c(c_), views(views_), n_views(n_views_), map(map_), summary(summary_), n_pot(n_pot_), rank(rank_), world(world_), warmup_views(warmup_views_), window(window_), exchange(exchange_),
          exchange_user(exchange_user_), verdict(verdict_), partition(partition_), index(views_, n_views_), best_off(best_offsets(views_, n_views_)) {}

    // ---- the failure protocol
    void note(int rc) { if (rc && !local_rc) { local_rc = rc; std::lock_guard<std::mutex> lk(c->err_mu); local_err = c->err; } }
    void soft(hipError_t e, const char* what) { if (e != hipSuccess) note(fail(c, L3D_ERR_HIP, std::string("l3d_match_chain_blocks: ") + what + ": " + hipGetErrorString(e))); }
    // publishes `mine` (negative = this rank failed with code -mine), reads everybody's into `words`; non-zero return: somebody failed (this rank's own message is kept)
    int all_gather_word(long long mine, const char* what)
    {
        if (local_rc && mine >= 0) mine = -(long long)local_rc;
        const StatusWords s = exchange_status_words(exchange, exchange_user, world, mine, st_own, st_all, st, words);
        if (s.publish != hipSuccess) note(fail(c, L3D_ERR_HIP, std::string("l3d_match_chain_blocks: status word: ") + hipGetErrorString(s.publish)));      // (it sent -1: failed)
        if (!s.exchanged) return fail(c, L3D_ERR_HIP, std::string("l3d_match_chain_blocks: the exchange of the status words failed (") + what + ")");
        if (s.read != hipSuccess) return fail(c, L3D_ERR_HIP, std::string("l3d_match_chain_blocks: status word: ") + hipGetErrorString(s.read));     // (after the collective: nobody waits for this rank any more)
        if (local_rc) return fail(c, local_rc, local_err);
        for (int r = 0; r < world; ++r)
            if (words[(size_t)r] < 0) return fail(c, L3D_ERR_HIP, "l3d_match_chain_blocks: rank " + std::to_string(r) + " failed (code " + std::to_string(-words[(size_t)r]) + ") while " + what);
        return L3D_OK;
    }

    bool held(int k) const { return k >= exact_from && k < last; }
    ArenaGrow grow() const { return ArenaGrow{ c, 0, rank }; }

    int setup();
    void run_cold();
    int reserve_tables();
    int exchange_digests();
    void report_round(const BlocksVerdict& v) const;
    void stage_tail_chunk(const BlocksHandoverPlan& plan, const TailLayout& tl, size_t off, size_t n);
    int hand_over(const std::vector<char>& miss, const BlocksHandoverPlan& plan, const TailLayout& tl);
    void rerun_warm(const TailLayout& tl);
    int run();

    // nothing replicated
    int finish_partitioned();
    int gather_early_slices(const EarlyReturns& E, ShareState& sh);
    void ingest_early_slots(ShareState& sh, size_t eslot, size_t hdr);
    int gather_alias_packages(const EarlyReturns& E, ShareState& sh);
    int build_share(ShareState& sh);

    // replicas
    struct Replicas {
        std::vector<long long> rec_of, seg_of;          // per rank: records / best-pair segments of its block
        long long total = 0;
        size_t o_best = 0, o_bpos = 0, slot = 0;        // a block's slot: [records | best depth pairs | best positions]
        std::vector<int> dvb;                           // the blocks' first views in the dense map
        std::vector<ChainResult> hres_all;              // the one chain's result records
        int64_t n_local = 0;
        double t3 = 0;
    };
    int finish_replicated();
    int gather_blocks(Replicas& R);
    int assemble_and_build(Replicas& R);
    int gather_pieces(Replicas& R);
};

// ---- the ranges of this rank (no collective yet: every rank of the job is configured alike, so a failure here is every rank's)
int BlocksRun::setup()
{
    *verdict = 1;
    if (n_pot) *n_pot = 0;
    c->products.valid = false;
    c->products.part = ProductsPart();
    HIPCHK(c, hipSetDevice(c->device));
    st = c->stream;
    const BlocksReach b = blocks_reach(window, index.neighbour_reach(), partition);
    reach = b.reach; tail = b.tail; check = b.check;
    own0 = block_begin(rank, n_views, world); own1 = block_begin(rank + 1, n_views, world);
    first = rank == 0 ? 0 : std::max(0, own0 - warmup_views);
    last = std::min(n_views, own1 + tail);
    arena_first = first;
    comp_from.assign((size_t)world, 0);
    for (int r = 1; r < world; ++r) comp_from[(size_t)r] = std::max(0, block_begin(r, n_views, world) - warmup_views);
    // partitioned: the job is sized by memory, not by the time of a second pass
    releases = partition && c->opt.part_release != 0;
    verified.assign((size_t)n_views, 0); S_src.assign((size_t)n_views, 0);
    for (int k = 0; k < n_views; ++k) { verified[(size_t)k] = views[k].n_tbm > 0 ? 1 : 0; S_src[(size_t)k] = views[k].S_src; }
    return L3D_OK;
}

// ---- this rank's chain: its block and the warm-up views in front of it, started cold
// (a rank whose chain fails must not leave the others waiting in the first collective: it still publishes its table, with a mark that every rank
// reads -- they all return an error then, without entering another collective)
void BlocksRun::run_cold()
{
    t0 = now_s();
    note(run_chain(c, views, n_views, nullptr, nullptr, nullptr, nullptr, nullptr, first, last));
    if (releases) note(release_chain_scratch(c));
    hres = c->ch_pin_res.as<ChainResult>();
    t1 = t2 = now_s();
    c->stats[0] = block_pairs(views, own0, own1);       // (the warm-up is the price of the speculation)
}

// the digest tables AND the status words, sized once: no reallocation between collectives
int BlocksRun::reserve_tables()
{
    tab_bytes = align256((size_t)n_views * sizeof(BlockDigest));
    if (c->ch_hdr.reserve(tab_bytes * (size_t)(world + 1) + 512 * (size_t)(world + 2) + 256) != hipSuccess)
        return fail(c, L3D_ERR_NOMEM, "l3d_match_chain_blocks: digest tables");     // (before the first collective of this call: every rank of the job is configured alike)
    unsigned char* H = c->ch_hdr.as<unsigned char>();
    dtab_own = reinterpret_cast<BlockDigest*>(H);
    dtab_all = reinterpret_cast<BlockDigest*>(H + tab_bytes);
    st_own = reinterpret_cast<long long*>(H + tab_bytes * (size_t)(world + 1));
    st_all = reinterpret_cast<long long*>(H + tab_bytes * (size_t)(world + 1) + 256);
    tab.assign((size_t)world * (size_t)n_views, BlockDigest());
    words.assign((size_t)world, 0);
    return L3D_OK;
}

// ---- digests of every list this rank computed (or the failure mark), all-gathered and read back; then the status words
int BlocksRun::exchange_digests()
{
    soft(hipMemsetAsync(dtab_own, 0, tab_bytes, st), "clearing the digest table");
    if (local_rc) {
        const BlockDigest mark = digest_failure_mark(local_rc);
        (void)hipMemcpyAsync(dtab_own, &mark, sizeof(mark), hipMemcpyHostToDevice, st);
        (void)hipStreamSynchronize(st);
    } else if (last > arena_first) {
        soft(hipMemcpyAsync(c->ch_res.p, hres, (size_t)n_views * sizeof(ChainResult), hipMemcpyHostToDevice, st), "uploading the result records");     // (the final records: a restart rewrites them)
        hipLaunchKernelGGL(k_block_digest, dim3(16, last - arena_first), dim3(256), 0, st, c->ch_kept.as<Match>(), c->ch_res.as<ChainResult>(), arena_first, dtab_own);
    }
    if (exchange(exchange_user, -1, dtab_own, dtab_all, tab_bytes, world, (void*)st)) return fail(c, L3D_ERR_HIP, "l3d_match_chain_blocks: the exchange of the digests failed");
    hipError_t e = hipSuccess;
    for (int r = 0; r < world && e == hipSuccess; ++r)
        e = hipMemcpyAsync(tab.data() + (size_t)r * n_views, reinterpret_cast<const unsigned char*>(dtab_all) + (size_t)r * tab_bytes, (size_t)n_views * sizeof(BlockDigest), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // a rank that cannot read the table cannot know the verdict the others reach: the status words below (entered by every rank after every digest
    // exchange) carry the failure to them
    if (e != hipSuccess) note(fail(c, L3D_ERR_HIP, std::string("l3d_match_chain_blocks: reading the digest tables: ") + hipGetErrorString(e)));
    t2 = now_s();
    const int failed = local_rc == L3D_OK ? blocks_failed_rank(tab.data(), n_views, world) : -1;
    if (failed >= 0) note(fail(c, L3D_ERR_HIP, "l3d_match_chain_blocks: the chain of rank " + std::to_string(failed) + " failed (code " + std::to_string(tab[(size_t)failed * n_views].R) + ")"));
    return all_gather_word(0, "computing its block");
}

void BlocksRun::report_round(const BlocksVerdict& v) const
{
    if (!c->opt.timing) return;
    for (int r = 1; r < world; ++r) {
        const int k = v.first_diff[(size_t)r];
        if (k >= 0 && k < block_begin(r, n_views, world))
            fprintf(stderr, "[l3d chain_blocks] rank %d's warm-up view %d differs from rank %d's (%d vs %d kept)\n", r, k, r - 1, tab[(size_t)r * n_views + k].n_kept, tab[(size_t)(r - 1) * n_views + k].n_kept);
    }
    fprintf(stderr, "[l3d chain_blocks rank %d/%d] round %d: views %d..%d (block from %d): chain %.2f ms, digests + exchange %.2f ms, %d rank(s) missed\n",
            rank, world, rounds, arena_first, last - 1, own0, (t1 - t0) * 1e3, (t2 - t1) * 1e3, v.n_miss);
}

// the part of this rank's tail -- one contiguous run of records, of best depth pairs, of best positions -- that falls into the chunk [off, off + n) of its slot
void BlocksRun::stage_tail_chunk(const BlocksHandoverPlan& plan, const TailLayout& tl, size_t off, size_t n)
{
    const int k0 = std::max(0, block_begin(rank + 1, n_views, world) - check), kf = plan.t_first[(size_t)rank];
    const size_t n_rec = (size_t)plan.t_rec[(size_t)rank], n_seg = (size_t)plan.t_seg[(size_t)rank];
    struct Piece { size_t at, len; const unsigned char* src; } pieces[3] = {
        { 0, n_rec * sizeof(Match), kf >= 0 ? reinterpret_cast<const unsigned char*>(c->ch_kept.as<Match>() + hres[kf].kept_base) : nullptr },
        { tl.o_best, n_seg * 8, reinterpret_cast<const unsigned char*>(c->ch_best.as<float2>() + best_off[(size_t)k0]) },
        { tl.o_bpos, n_seg * 4, reinterpret_cast<const unsigned char*>(c->ch_bestpos.as<int>() + best_off[(size_t)k0]) } };
    for (const Piece& q : pieces) {
        const size_t lo = std::max(q.at, off), hi = std::min(q.at + q.len, off + n);
        if (q.src && hi > lo) soft(hipMemcpyAsync(c->ch_send.as<unsigned char>() + (lo - off), q.src + (lo - q.at), hi - lo, hipMemcpyDeviceToDevice, st), "staging a chunk of the hand-over");
    }
}

// ---- recovery, all missed blocks at once: every rank that missed takes over its predecessor's last `check` views (records, best depth pairs, best
// positions: one all-gather, the one primitive of the protocol).  A predecessor that missed too hands over what its cold start produced -- usually
// already the one chain's by the end of a block; if not, the next round's digests show it and that rank runs again.  After round j rank j is exact
// whatever happened (it took over from rank j-1, exact since round j-1).
//   A tail is one byte stream (TailLayout), the same offsets on every rank; it travels in CHUNKS (option handover_chunk_kb, 256 MB): an all-gather hands
// every rank every slot, and a whole tail per slot would cost world x tail bytes on every rank (52 GB at 4000 x 24 x 8 ranks) for the one slot a rank
// reads -- a chunk per slot costs world x 256 MB
int BlocksRun::hand_over(const std::vector<char>& miss, const BlocksHandoverPlan& plan, const TailLayout& tl)
{
    const size_t slot = tl.bytes + 256;
    const size_t chunk = std::min(slot, align256((size_t)std::max(1, c->opt.handover_chunk_kb) << 10));
    const bool sends = rank + 1 < world && miss[(size_t)rank + 1], takes = miss[(size_t)rank] != 0;
    hipError_t e = c->ch_send.reserve(chunk + 256);
    if (e == hipSuccess) e = c->ch_gathered.reserve(chunk * (size_t)world + 256);
    if (e == hipSuccess && takes) e = c->ch_stage.reserve(slot + 256);
    if (e != hipSuccess) note(fail(c, L3D_ERR_NOMEM, "l3d_match_chain_blocks: the hand-over of a block's sources"));
    if (int rc = all_gather_word(0, "staging the hand-over of a block's sources")) return rc;
    for (size_t off = 0; off < slot; off += chunk) {
        const size_t n = std::min(chunk, slot - off);
        if (sends && !local_rc) stage_tail_chunk(plan, tl, off, n);
        if (exchange(exchange_user, -5, c->ch_send.p, c->ch_gathered.p, n, world, (void*)st)) return fail(c, L3D_ERR_HIP, "l3d_match_chain_blocks: the hand-over exchange failed");
        if (takes && !local_rc) soft(hipMemcpyAsync(c->ch_stage.as<unsigned char>() + off, c->ch_gathered.as<unsigned char>() + (size_t)(rank - 1) * n, n, hipMemcpyDeviceToDevice, st), "keeping a chunk of the hand-over");
        if (off + chunk < slot) soft(hipStreamSynchronize(st), "waiting for a chunk of the hand-over");       // (the next chunk reuses the send and gathered buffers)
    }
    for (int r = 1; r < world; ++r) if (miss[(size_t)r]) comp_from[(size_t)r] = std::max(0, block_begin(r, n_views, world) - check);
    return L3D_OK;
}

// this rank's block again, WARM from the tail its predecessor handed over (in ch_stage)
void BlocksRun::rerun_warm(const TailLayout& tl)
{
    const int k0 = std::max(0, own0 - check);
    const BlockDigest* src = tab.data() + (size_t)(rank - 1) * n_views;
    std::vector<int> n_kept, R;
    for (int k = k0; k < own0; ++k) { n_kept.push_back(src[k].n_kept); R.push_back(src[k].R); }
    const ChainPreload pre = tail_preload(c->ch_stage.p, tl.o_best, tl.o_bpos, k0, own0, std::move(n_kept), std::move(R));
    const double tr0 = now_s();
    note(run_chain(c, views, n_views, nullptr, nullptr, nullptr, nullptr, nullptr, own0, last, &pre));
    if (releases) note(release_chain_scratch(c));
    hres = c->ch_pin_res.as<ChainResult>();
    arena_first = k0;
    t1 += now_s() - tr0;
    if (c->opt.timing) fprintf(stderr, "[l3d chain_blocks rank %d/%d] block re-run warm from rank %d's last %d views: %.2f ms\n", rank, world, rank - 1, own0 - k0, (now_s() - tr0) * 1e3);
}

// ---- the chain, cold; then rounds of digests and verdict: a block whose speculation failed is re-run WARM from its predecessor's true lists (the first
// one that failed: everything in front of it is exact), and the digests are exchanged again -- a miss costs one block, not the pass
int BlocksRun::run()
{
    if (int rc = setup()) return rc;
    run_cold();
    if (int rc = reserve_tables()) return rc;
    for (;; ++rounds) {
        if (int rc = exchange_digests()) return rc;
        const BlocksVerdict v = blocks_verdict(tab.data(), n_views, world, check, tail, partition, comp_from.data());
        report_round(v);
        if (v.n_miss == 0) break;
        // option block_recover = 0 (A/B, tests of the fall-through): the round-4 behaviour -- any miss sends the pass to the caller's other mode
        if (v.hopeless || c->opt.block_recover == 0 || rounds >= world) return L3D_OK;                  // *verdict = 1: nothing committed
        blocks_rerun += v.n_miss;
        const BlocksHandoverPlan plan = blocks_handover_plan(tab.data(), n_views, world, check, v.miss.data(), verified.data(), S_src.data());
        const TailLayout tl(plan.max_rec, plan.max_seg);
        if (int rc = hand_over(v.miss, plan, tl)) return rc;
        if (v.miss[(size_t)rank]) rerun_warm(tl);
    }
    c->products.part.recovery_rounds = rounds; c->products.part.blocks_rerun = blocks_rerun;
    exact_from = rank == 0 ? 0 : std::max(arena_first, own0 - check);
    return partition ? finish_partitioned() : finish_replicated();
}

// =================================================================================================================================
// Nothing is replicated.  This rank holds the exact records of the views [exact_from, last) and builds from them, locally: the rows of the table
// for the views within `reach` of its block, best matches and medians for every view it holds.  What the early-return quirk (cudawrapper.cu:877-878)
// files under LOCAL camera numbers read as view ids can name any view of the scene: the pieces below are all-gathered, each by the rank that owns it.
int BlocksRun::finish_partitioned()
{
    ShareState sh(hres, n_views, exact_from, last, best_off.data());
    const EarlyReturns E = turn_early_views(views, n_views, index);
    if (!E.fits()) return L3D_OK;    // (a schedule full of early returns: the replicated mode takes it; the same on every rank)
    if (world > 1) {
        if (int rc = gather_early_slices(E, sh)) return rc;
        if (int rc = gather_alias_packages(E, sh)) return rc;
    }
    return build_share(sh);
}

// ---- the records that point at an early-return view -- a sliver of their sources' lists: groups = the sources; sender = the owner of the source.
// slot: [int n_groups | (int source, int count) x n_groups] [records of the groups, back to back]; staged in ch_stage (ch_send holds the control block)
int BlocksRun::gather_early_slices(const EarlyReturns& E, ShareState& sh)
{
    if (E.groups.empty()) return L3D_OK;
    const char* who = "l3d_match_chain_partition";
    std::vector<int> mine;
    for (int si : E.groups) if (block_owner(si, n_views, world) == rank) mine.push_back(si);
    std::vector<int> cnt(mine.size(), 0);
    long long total = 0;
    if (c->ch_send.reserve(EarlyPackCtl::bytes + 256) != hipSuccess) note(fail(c, L3D_ERR_NOMEM, "l3d_match_chain_partition: early-return control block"));
    else { note(count_early_records(c, E.ids, mine, cnt, st)); for (int x : cnt) total += x; }
    if (int rc = all_gather_word(total, "counting the records that point at early-return views")) return rc;
    long long max_total = 0;
    for (int r = 0; r < world; ++r) max_total = std::max(max_total, words[(size_t)r]);
    const size_t hdr = 4096, eslot = hdr + align256((size_t)max_total * sizeof(Match)) + 256;
    hipError_t e = c->ch_stage.reserve(eslot + 256);
    if (e == hipSuccess) e = c->ch_gathered.reserve(eslot * (size_t)world + 256);
    if (e != hipSuccess) note(fail(c, L3D_ERR_NOMEM, "l3d_match_chain_partition: early-return slots"));
    else {
        std::vector<int> h((size_t)1 + 2 * mine.size(), 0);
        h[0] = (int)mine.size();
        for (size_t g = 0; g < mine.size(); ++g) { h[1 + 2 * g] = mine[g]; h[2 + 2 * g] = cnt[g]; }
        unsigned char* E0 = c->ch_stage.as<unsigned char>();
        soft(hipMemcpyAsync(E0, h.data(), h.size() * 4, hipMemcpyHostToDevice, st), "uploading the header of the early-return slot");
        note(pack_early_records(c, who, E.ids.size(), cnt, reinterpret_cast<Match*>(E0 + hdr), st));       // (it leaves the stream idle: h is a stack vector)
    }
    if (int rc = all_gather_word(0, "staging the records that point at early-return views")) return rc;
    if (exchange(exchange_user, -6, c->ch_stage.p, c->ch_gathered.p, eslot, world, (void*)st)) return fail(c, L3D_ERR_HIP, "l3d_match_chain_partition: the exchange of the early-return records failed");
    ingest_early_slots(sh, eslot, hdr);
    return L3D_OK;
}
// every other rank's slot: the slices of the sources this rank does not hold go behind its records
void BlocksRun::ingest_early_slots(ShareState& sh, size_t eslot, size_t hdr)
{
    const unsigned char* G = c->ch_gathered.as<unsigned char>();
    std::vector<int> hh(1024);
    for (int r = 0; r < world && !local_rc; ++r) {
        if (r == rank) continue;
        soft(hipMemcpyAsync(hh.data(), G + (size_t)r * eslot, hdr, hipMemcpyDeviceToHost, st), "reading the header of an early-return slot");
        soft(hipStreamSynchronize(st), "reading the header of an early-return slot");
        if (local_rc) break;
        long long o = 0;
        for (int g = 0; g < hh[0] && g < (int)EarlyReturns::kMaxGroups; ++g) {
            const int si = hh[1 + 2 * g], n = hh[2 + 2 * g];
            if (si >= 0 && si < n_views && n > 0 && !held(si))
                if (int rc = ingest_early_slice(c, sh, si, reinterpret_cast<const Match*>(G + (size_t)r * eslot + hdr) + o, n, grow(), st)) { note(rc); break; }
            o += n;
        }
    }
}

// ---- the views an early return's LOCAL camera numbers name (cudawrapper.cu:877-878 hands the list back with local numbers, line3D.cc:861-865
// files the entries under them read as view ids): rows of an early-return view point at their segments, whoever holds them.  The affinity fill
// only asks whether such a segment has a hypothesis and where it stands in the order -- the views' best matches (one record per segment:
// a few hundred KB per view) are all-gathered, each view's by the rank that owns it
int BlocksRun::gather_alias_packages(const EarlyReturns& E, ShareState& sh)
{
    const std::vector<int>& alias = E.alias;
    if (alias.empty()) return L3D_OK;
    const char* who = "l3d_match_chain_partition";
    std::vector<size_t> slot_of((size_t)world, 0);
    for (int b : alias) slot_of[(size_t)block_owner(b, n_views, world)] += alias_package_bytes(views[b].S_src);
    size_t aslot = 256;
    for (int r = 0; r < world; ++r) aslot = std::max(aslot, slot_of[(size_t)r] + 256);
    std::vector<int> mine;
    for (int b : alias) if (block_owner(b, n_views, world) == rank) mine.push_back(b);
    hipError_t e = c->ch_stage.reserve(aslot + 256);
    if (e == hipSuccess) e = c->ch_gathered.reserve(aslot * (size_t)world + 256);
    if (e == hipSuccess) e = c->ch_send.reserve(alias_ctl_bytes(mine.size()));
    if (e != hipSuccess) note(fail(c, L3D_ERR_NOMEM, "l3d_match_chain_partition: alias-view packages"));
    else note(pack_alias_packages(c, who, views, mine, best_off.data(), c->ch_stage.as<unsigned char>(), st));
    if (int rc = all_gather_word(0, "packing the best matches of the views early returns name")) return rc;
    if (exchange(exchange_user, -11, c->ch_stage.p, c->ch_gathered.p, aslot, world, (void*)st)) return fail(c, L3D_ERR_HIP, "l3d_match_chain_partition: the exchange of the alias views' best matches failed");
    const unsigned char* G = c->ch_gathered.as<unsigned char>();
    std::vector<size_t> at((size_t)world, 0);
    for (int b : alias) {
        const int r = block_owner(b, n_views, world);
        const unsigned char* pk = G + (size_t)r * aslot + at[(size_t)r];
        at[(size_t)r] += alias_package_bytes(views[b].S_src);
        if (local_rc || held(b)) continue;              // (held: its own records say it all)
        if (int rc = ingest_alias_package(c, who, sh, views, b, pk, grow(), st)) {
            // (refused on every rank alike -- the status words carry it: such a job takes l3d_shard_chain_partition, which keeps such views whole)
            if (rc == L3D_ERR_UNSUPPORTED) rc = fail(c, rc, std::string(l3d_last_error(c)) + ": use the segment-sharded partition");
            note(rc);
            break;
        }
    }
    return L3D_OK;
}

// ---- the local products; the counts of all ranks travel with the last status words
int BlocksRun::build_share(ShareState& sh)
{
    TurnRange t;
    t.pre0 = exact_from; t.run1 = last; t.own0 = own0; t.own1 = own1;
    t.row0 = std::max(rank == 0 ? 0 : exact_from, own0 - reach); t.row1 = std::min(last, own1 + reach);
    ProductsPart part;
    int64_t n_local = 0;
    const double t3 = now_s();
    if (!local_rc) note(share_build(c, views, n_views, map, summary, rank, world, t, sh, part, n_local));
    if (int rc = all_gather_word(n_local, "building its rows of the products")) return rc;
    long long n_pot_all = 0;
    for (int r = 0; r < world; ++r) n_pot_all += words[(size_t)r];
    part.recovery_rounds = rounds; part.blocks_rerun = blocks_rerun;
    share_file(c, n_views, t, sh, part, n_local, n_pot_all);
    if (n_pot) *n_pot = n_local;
    if (c->opt.timing) fprintf(stderr, "[l3d chain_partition rank %d/%d] exact from view %d, chain to view %d, rows of views %d..%d, %lld potential correspondences here of %lld: products %.2f ms\n",
                               rank, world, exact_from, last - 1, t.row0, t.row1 - 1, (long long)n_local, n_pot_all, (now_s() - t3) * 1e3);
    *verdict = 0;
    return L3D_OK;
}

// =================================================================================================================================
// Replicas: the blocks are all-gathered and laid out as the one chain's arena; then matchViews' products: every rank builds the rows of its OWN block
// of views (sort + unique of the keys whose source lies in the block: its views' records and their neighbours', all of them in the arena now), the
// pieces are all-gathered and put together -- 1/world of the sort per rank instead of all of it on every rank
int BlocksRun::finish_replicated()
{
    Replicas R;
    if (int rc = gather_blocks(R)) return rc;
    const int nvd = map->n_views;
    R.dvb.assign((size_t)world + 1, 0);
    for (int r = 0; r <= world; ++r) R.dvb[(size_t)r] = r == 0 ? 0 : (r == world ? nvd : chain_dense_view(views, n_views, map, block_begin(r, n_views, world)));
    for (int r = 1; r <= world; ++r) if (R.dvb[(size_t)r] < R.dvb[(size_t)r - 1]) return fail(c, L3D_ERR_INVALID, "l3d_match_chain_blocks: the chain's views do not ascend with the dense map");     // (the same on every rank)
    // counts first (a piece is padded to the largest; a negative count = this rank failed), then the pieces
    note(assemble_and_build(R));
    if (int rc = all_gather_word((long long)R.n_local, "building its rows of the products")) return rc;
    return gather_pieces(R);
}

// ---- all-gather of the blocks: [records of the block's views][best depth pairs][best positions], padded to the largest block
int BlocksRun::gather_blocks(Replicas& R)
{
    R.rec_of.assign((size_t)world, 0); R.seg_of.assign((size_t)world, 0);
    for (int k = 0; k < n_views; ++k) {
        const int r = block_owner(k, n_views, world);
        R.rec_of[(size_t)r] += tab[(size_t)r * n_views + k].n_kept;
        if (views[k].n_tbm > 0) R.seg_of[(size_t)r] += views[k].S_src;
    }
    long long max_rec = 0, max_seg = 0;
    for (int r = 0; r < world; ++r) { max_rec = std::max(max_rec, R.rec_of[(size_t)r]); max_seg = std::max(max_seg, R.seg_of[(size_t)r]); R.total += R.rec_of[(size_t)r]; }
    const TailLayout tl(max_rec, max_seg);
    R.o_best = tl.o_best; R.o_bpos = tl.o_bpos; R.slot = tl.bytes;
    hipError_t e = c->ch_send.reserve(R.slot + 256);
    if (e == hipSuccess) e = c->ch_gathered.reserve(R.slot * (size_t)world + 256);
    if (e != hipSuccess) { (void)hipGetLastError(); note(fail(c, L3D_ERR_NOMEM, "l3d_match_chain_blocks: the blocks' slots (" + std::to_string(world) + " x " + std::to_string(R.slot >> 20) + " MB: " + std::to_string(max_rec) + " kept matches in the largest block)")); }
    else {
        unsigned char* send = c->ch_send.as<unsigned char>();
        const size_t n_rec = (size_t)R.rec_of[(size_t)rank], n_seg = (size_t)R.seg_of[(size_t)rank];
        long long own_start = 0;                                    // (this rank's arena: the views it holds, back to back from arena_first)
        for (int k = arena_first; k < own0; ++k) own_start += hres[k].n_kept;
        if (n_rec > 0) soft(hipMemcpyAsync(send, c->ch_kept.as<Match>() + own_start, n_rec * sizeof(Match), hipMemcpyDeviceToDevice, st), "staging the block's records");
        if (n_seg > 0) {
            soft(hipMemcpyAsync(send + R.o_best, c->ch_best.as<float2>() + best_off[(size_t)own0], n_seg * 8, hipMemcpyDeviceToDevice, st), "staging the block's best depth pairs");
            soft(hipMemcpyAsync(send + R.o_bpos, c->ch_bestpos.as<int>() + best_off[(size_t)own0], n_seg * 4, hipMemcpyDeviceToDevice, st), "staging the block's best positions");
        }
    }
    if (int rc = all_gather_word(0, "staging its block")) return rc;
    if (exchange(exchange_user, -2, c->ch_send.p, c->ch_gathered.p, R.slot, world, (void*)st)) return fail(c, L3D_ERR_HIP, "l3d_match_chain_blocks: the exchange of the kept lists failed");
    return L3D_OK;
}

// ---- the one chain's arena: blocks in rank order = views in order; then this rank's rows of the products
int BlocksRun::assemble_and_build(Replicas& R)
{
    const std::vector<long long>&rec_of = R.rec_of, &seg_of = R.seg_of;
    const long long total = R.total;
    const size_t o_best = R.o_best, o_bpos = R.o_bpos, slot = R.slot;
    HIPCHK(c, hipStreamSynchronize(st));            // (the arena below may be reallocated: everything that reads the old one is done)
    if (c->ch_kept.reserve(((size_t)total + 64) * sizeof(Match)) != hipSuccess) {
        (void)hipGetLastError();
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        return fail(c, L3D_ERR_NOMEM, "l3d_match_chain_blocks: the one chain's arena of " + std::to_string(total) + " kept matches (" + std::to_string(((size_t)total * sizeof(Match)) >> 20) +
                                          " MB) does not fit (" + std::to_string(fr >> 20) + " of " + std::to_string(tot >> 20) + " MB free; l3d_match_chain_partition keeps every rank's records where they are)");
    }
    R.hres_all.assign((size_t)n_views, ChainResult());
    long long base = 0;
    for (int k = 0; k < n_views; ++k) {
        const BlockDigest& e = tab[(size_t)block_owner(k, n_views, world) * n_views + k];
        ChainResult& r = R.hres_all[(size_t)k];
        r.kept_base = (uint64_t)base; r.n_kept = e.n_kept; r.R = e.R; r.overflow = 0;
        base += e.n_kept;
    }
    const std::vector<ProdChainView> pvh = prod_chain_views(c, views, n_views, best_off.data(), nullptr);
    long long at = 0;
    const unsigned char* G = c->ch_gathered.as<unsigned char>();
    for (int r = 0; r < world; ++r) {
        const int b0 = block_begin(r, n_views, world);
        if (rec_of[(size_t)r]) HIPCHK(c, hipMemcpyAsync(c->ch_kept.as<Match>() + at, G + (size_t)r * slot, (size_t)rec_of[(size_t)r] * sizeof(Match), hipMemcpyDeviceToDevice, st));
        if (seg_of[(size_t)r]) {
            HIPCHK(c, hipMemcpyAsync(c->ch_best.as<float2>() + best_off[(size_t)b0], G + (size_t)r * slot + o_best, (size_t)seg_of[(size_t)r] * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(c->ch_bestpos.as<int>() + best_off[(size_t)b0], G + (size_t)r * slot + o_bpos, (size_t)seg_of[(size_t)r] * 4, hipMemcpyDeviceToDevice, st));
        }
        at += rec_of[(size_t)r];
    }
    R.t3 = now_s();
    return build_products(c, views, n_views, pvh.data(), R.hres_all.data(), map, summary, &R.n_local, R.dvb[(size_t)rank], R.dvb[(size_t)rank + 1]);
}

// ---- all-gather of the pieces of the table, [row starts of the block, numbered from 0 | entries] padded to the largest, and the one table put together
int BlocksRun::gather_pieces(Replicas& R)
{
    Products& P = c->products;
    const std::vector<int>& dvb = R.dvb;
    const int nvd = map->n_views;
    const int64_t n_local = R.n_local;
    const std::vector<long long> cnts = words;
    long long max_cnt = 0, max_rows = 0, n_pot_all = 0;
    for (int r = 0; r < world; ++r) {
        max_cnt = std::max(max_cnt, cnts[(size_t)r]); n_pot_all += cnts[(size_t)r];
        max_rows = std::max(max_rows, (long long)map->seg_base[dvb[(size_t)r + 1]] - map->seg_base[dvb[(size_t)r]]);
    }
    const size_t o_ent = align256((size_t)max_rows * 8), pslot = o_ent + align256((size_t)max_cnt * 4 + 4);
    hipError_t e = c->ch_send.reserve(pslot + 256);
    if (e == hipSuccess) e = c->ch_gathered.reserve(pslot * (size_t)world + 256);
    if (e != hipSuccess) note(fail(c, L3D_ERR_NOMEM, "l3d_match_chain_blocks: the pieces' slots"));
    else {
        const long long r0 = map->seg_base[dvb[(size_t)rank]], nr = (long long)map->seg_base[dvb[(size_t)rank + 1]] - r0;
        unsigned char* sp = c->ch_send.as<unsigned char>();
        if (nr > 0) soft(hipMemcpyAsync(sp, P.pot_start.as<long long>() + r0, (size_t)nr * 8, hipMemcpyDeviceToDevice, st), "staging the piece's row starts");
        if (n_local > 0) soft(hipMemcpyAsync(sp + o_ent, P.pot_tgt.p, (size_t)n_local * 4, hipMemcpyDeviceToDevice, st), "staging the piece's entries");
    }
    if (int rc = all_gather_word(0, "staging its piece of the products")) return rc;
    if (exchange(exchange_user, -4, c->ch_send.p, c->ch_gathered.p, pslot, world, (void*)st)) return fail(c, L3D_ERR_HIP, "l3d_match_chain_blocks: the exchange of the table pieces failed");
    // (past the last collective: a failure from here on is this rank's alone)
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, P.pot_tgt.reserve(((size_t)n_pot_all + 2) * 4));
    const unsigned char* G = c->ch_gathered.as<unsigned char>();
    long long base = 0;
    for (int r = 0; r < world; ++r) {
        const long long r0 = map->seg_base[dvb[(size_t)r]], nr = (long long)map->seg_base[dvb[(size_t)r + 1]] - r0;
        launch_prod_shift_rows(reinterpret_cast<const long long*>(G + (size_t)r * pslot), nr, base, P.pot_start.as<long long>() + r0, st);
        if (cnts[(size_t)r]) HIPCHK(c, hipMemcpyAsync(P.pot_tgt.as<int>() + base, G + (size_t)r * pslot + o_ent, (size_t)cnts[(size_t)r] * 4, hipMemcpyDeviceToDevice, st));
        base += cnts[(size_t)r];
    }
    HIPCHK(c, hipMemcpyAsync(P.pot_start.as<long long>() + map->seg_base[nvd], &n_pot_all, 8, hipMemcpyHostToDevice, st));     // the closing row start
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    P.n_pot = n_pot_all;
    P.valid = true;
    if (n_pot) *n_pot = n_pot_all;
    memcpy(c->ch_pin_res.as<ChainResult>(), R.hres_all.data(), (size_t)n_views * sizeof(ChainResult));       // (what l3d_chain_kept_list reads)
    c->stats[3] = (double)R.total;
    { double raw = 0; for (int k = own0; k < own1; ++k) raw += tab[(size_t)rank * n_views + k].R; c->stats[1] = raw; }      // (this rank's useful share)
    if (c->opt.timing) fprintf(stderr, "[l3d chain_blocks rank %d/%d] gather of the blocks %.2f ms, products (own rows + gather of the pieces) %.2f ms\n", rank, world, (R.t3 - t2) * 1e3, (now_s() - R.t3) * 1e3);
    *verdict = 0;
    return L3D_OK;
}

}  // namespace

static int chain_blocks_impl(l3d_ctx* c, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot,
                             int rank, int world, int warmup_views, int window, l3d_exchange_fn exchange, void* exchange_user, int* verdict, bool partition)
{
    if (!c) return L3D_ERR_INVALID;
    if (!views || n_views <= 0 || !map || !summary || !exchange || !verdict || world < 1 || rank < 0 || rank >= world || warmup_views < 0 || window < 0)
        return fail(c, L3D_ERR_INVALID, "l3d_match_chain_blocks: bad argument");
    return BlocksRun(c, views, n_views, map, summary, n_pot, rank, world, warmup_views, window, exchange, exchange_user, verdict, partition).run();
}

extern "C" int l3d_match_chain_blocks(l3d_ctx* c, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot,
                                      int rank, int world, int warmup_views, int window, l3d_exchange_fn exchange, void* exchange_user, int* verdict)
{
    return chain_blocks_impl(c, views, n_views, map, summary, n_pot, rank, world, warmup_views, window, exchange, exchange_user, verdict, 0);
}

extern "C" int l3d_match_chain_partition(l3d_ctx* c, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot,
                                         int rank, int world, int warmup_views, int window, l3d_exchange_fn exchange, void* exchange_user, int* verdict)
{
    return chain_blocks_impl(c, views, n_views, map, summary, n_pot, rank, world, warmup_views, window, exchange, exchange_user, verdict, 1);
}

// the rules of l3d_blocks_rule.hpp on a table given as plain arrays (tests/test_blocks_verdict_cases_cpu.py): no context, no device
extern "C" int l3d_test_blocks_verdict(int n_views, int world, int window, int neighbour_reach, int check, int tail, int partition, const uint64_t* hash, const int32_t* n_kept,
                                       const int32_t* comp_from, const int32_t* verified, const int32_t* S_src, int32_t* begin, int32_t* owner, int32_t reach_out[3], int32_t* miss, int32_t* first_diff,
                                       int32_t summary[3], int64_t* t_rec, int64_t* t_seg, int32_t* t_first, int64_t maxima[2])
{
    if (n_views <= 0 || world < 1 || check < 0 || tail < 0 || !hash || !n_kept || !comp_from || !verified || !S_src || !begin || !owner || !reach_out || !miss || !first_diff || !summary || !t_rec || !t_seg ||
        !t_first || !maxima) return L3D_ERR_INVALID;
    const BlocksReach b = blocks_reach(window, neighbour_reach, partition != 0);
    reach_out[0] = b.reach; reach_out[1] = b.tail; reach_out[2] = b.check;
    for (int r = 0; r <= world; ++r) begin[r] = block_begin(r, n_views, world);
    for (int k = 0; k < n_views; ++k) owner[k] = block_owner(k, n_views, world);
    std::vector<BlockDigest> tab((size_t)world * n_views);
    std::vector<char> ver((size_t)n_views);
    for (size_t i = 0; i < tab.size(); ++i) { tab[i].hash = hash[i]; tab[i].n_kept = n_kept[i]; tab[i].R = 0; }
    for (int k = 0; k < n_views; ++k) ver[(size_t)k] = verified[k] != 0;
    const BlocksVerdict v = blocks_verdict(tab.data(), n_views, world, check, tail, partition != 0, comp_from);
    const BlocksHandoverPlan p = blocks_handover_plan(tab.data(), n_views, world, check, v.miss.data(), ver.data(), S_src);
    for (int r = 0; r < world; ++r) {
        miss[r] = v.miss[(size_t)r]; first_diff[r] = v.first_diff[(size_t)r];
        t_rec[r] = p.t_rec[(size_t)r]; t_seg[r] = p.t_seg[(size_t)r]; t_first[r] = p.t_first[(size_t)r];
    }
    summary[0] = v.n_miss; summary[1] = v.hopeless ? 1 : 0; summary[2] = blocks_failed_rank(tab.data(), n_views, world);
    maxima[0] = p.max_rec; maxima[1] = p.max_seg;
    return L3D_OK;
}

extern "C" int l3d_partition_info(l3d_ctx* c, int info[10], int64_t* n_pot_all)
{
    if (!c) return L3D_ERR_INVALID;
    const ProductsPart& q = c->products.part;
    if (info) { const int v[10] = { q.rank, q.world, q.own_dv0, q.own_dv1, q.row_dv0, q.row_dv1, q.held_dv0, q.held_dv1, q.recovery_rounds, q.blocks_rerun }; memcpy(info, v, sizeof(v)); }
    if (n_pot_all) *n_pot_all = q.active ? q.n_pot_all : c->products.n_pot;
    return L3D_OK;                      // (info[1] = world of the partition; not partitioned: the defaults, world 1)
}

// =================================================================================================================================
// Turns that hand the chain over (l3d_turns.hpp; line3d_host.cpp: node mode 2 with l3d_line3d_set_turn_handover).  The parts of the
// blocks-of-views partition above that involve no collective, composed SEQUENTIALLY: the ranks of one device run one after the other, so a
// successor needs no speculation -- it is given its predecessor's tail (ChainPreload, as the recovery path gives it after a miss).
namespace {

struct TurnNeeds { std::vector<char> in_E; std::vector<int> src, alias_req, alias_opt; };

// what the share of a turn with these ranges ingests.  in_E: the early-return views it builds hypotheses and entries of -- the ones it holds and the
// ones whose entries land in its rows; every other one is left out of its products (a partial list of sources would give it hypotheses its owner
// does not have)
void turn_needs(const std::vector<TurnEarly>& early, const l3d::TurnRange& t, TurnNeeds& o)
{
    auto held = [&](int k) { return k >= t.pre0 && k < t.run1; };
    auto in_rows = [&](int k) { return k >= t.row0 && k < t.row1; };
    o.in_E.assign(early.size(), 0);
    for (size_t i = 0; i < early.size(); ++i) {
        const TurnEarly& e = early[i];
        bool in = held(e.view);
        for (int b : e.alias_rows) in = in || in_rows(b);
        if (!in) continue;
        o.in_E[i] = 1;
        for (int si : e.src) if (!held(si)) o.src.push_back(si);
        for (int b : e.alias_best) if (!held(b)) { o.alias_opt.push_back(b); if (in_rows(e.view)) o.alias_req.push_back(b); }
    }
    for (std::vector<int>* v : { &o.src, &o.alias_req, &o.alias_opt }) { std::sort(v->begin(), v->end()); v->erase(std::unique(v->begin(), v->end()), v->end()); }
}

}  // namespace

int l3d::turn_handover_schedule(const l3d_chain_view* views, int n_views, int world, int window, TurnSchedule* out)
{
    if (!views || n_views <= 0 || world < 1 || !out) return L3D_ERR_INVALID;
    for (int k = 0; k < n_views; ++k) {
        if (views[k].N < 0 || views[k].n_sources < 0 || (views[k].N > 0 && !views[k].local2global) || (views[k].n_sources > 0 && (!views[k].source_cam || !views[k].source_index))) return L3D_ERR_INVALID;
        for (int q = 0; q < views[k].n_sources; ++q) if (views[k].source_index[q] >= n_views) return L3D_ERR_INVALID;
    }
    if (window <= 0) {
        window = 1;
        for (int k = 0; k < n_views; ++k) for (int q = 0; q < views[k].n_sources; ++q) if (views[k].source_index[q] >= 0) window = std::max(window, k - views[k].source_index[q]);
    }
    const ScheduleIndex index(views, n_views);
    const BlocksReach b = blocks_reach(window, index.neighbour_reach(), true);
    const int reach = b.reach;
    TurnSchedule& S = *out;
    S.reach = reach; S.tail = b.tail; S.check = b.check; S.supported = true;
    S.turns.assign((size_t)world, TurnRange());
    for (int r = 0; r < world; ++r) {
        TurnRange& t = S.turns[(size_t)r];
        t.own0 = block_begin(r, n_views, world); t.own1 = block_begin(r + 1, n_views, world);
        t.run1 = std::min(n_views, t.own1 + S.tail);
        t.pre0 = r == 0 ? 0 : std::max(0, t.own0 - S.check);
        t.run0 = r == 0 ? 0 : t.own0;
        t.row0 = std::max(t.pre0, t.own0 - reach); t.row1 = std::min(t.run1, t.own1 + reach);
        t.deferred = 0;
    }
    const EarlyReturns E = turn_early_views(views, n_views, index);
    if (!E.fits()) S.supported = false;
    for (int r = 0; r < world && world > 1; ++r) {
        TurnNeeds need;
        turn_needs(E.views, S.turns[(size_t)r], need);
        for (int si : need.src) if (block_owner(si, n_views, world) > r) S.turns[(size_t)r].deferred = 1;
        for (int b : need.alias_req) if (block_owner(b, n_views, world) > r) S.turns[(size_t)r].deferred = 1;
        // (chain_blocks_impl: one list cannot be both the sliver of records that point at an early-return view and the view's best matches)
        for (int b : need.alias_opt) if (std::binary_search(need.src.begin(), need.src.end(), b)) S.supported = false;
    }
    return L3D_OK;
}

extern "C" int l3d_turn_handover_plan(const l3d_chain_view* views, int n_views, int world, int32_t* out, int32_t* info)
{
    if (!out) return L3D_ERR_INVALID;
    l3d::TurnSchedule S;
    if (const int rc = l3d::turn_handover_schedule(views, n_views, world, 0, &S)) return rc;
    for (int r = 0; r < world; ++r) {
        const l3d::TurnRange& t = S.turns[(size_t)r];
        const int v[8] = { t.pre0, t.run0, t.run1, t.row0, t.row1, t.own0, t.own1, t.deferred };
        memcpy(out + 8 * r, v, sizeof(v));
    }
    if (info) { info[0] = S.reach; info[1] = S.check; info[2] = S.tail; info[3] = S.supported ? 1 : 0; }
    return L3D_OK;
}

void l3d::turn_handover_release(TurnHandover* p)
{
    if (!p) return;
    if (p->dev) { if (p->device >= 0) (void)hipSetDevice(p->device); (void)hipFree(p->dev); }
    *p = TurnHandover();
}
void l3d::turn_store_release(TurnStore* s)
{
    if (!s) return;
    if (s->device >= 0) (void)hipSetDevice(s->device);
    for (auto& x : s->early) if (x.owns && x.base) (void)hipFree(x.base);
    for (auto& x : s->alias) if (x.owns && x.base) (void)hipFree(x.base);
    *s = TurnStore();
}

namespace {

// one visit of a turn (match_chain_turn) as its four numbered steps; each returns a code with the message set
struct TurnVisit {
    l3d_ctx* c; const l3d_chain_view* views; int n_views; const l3d_dense_map* map; l3d_chain_summary* summary; int rank, world;
    TurnStore* store; TurnReport* report;
    TurnSchedule S;
    TurnRange T;
    hipStream_t st = nullptr;
    std::vector<long long> best_off;
    const char* who = "match_chain_turn";

    int chain_piece(const TurnHandover* in);
    int digest_held(const ShareState& sh);
    int leave_tail(const ShareState& sh, TurnHandover* out);
    int file_early_slices(const EarlyReturns& E);
    int file_alias_packages(const EarlyReturns& E);
    int build_share(const EarlyReturns& E, ShareState& sh, double chain_ms);
};

// ---- 1. the chain piece: cold from view 0 (turn 0), else warm from the predecessor's tail
int TurnVisit::chain_piece(const TurnHandover* in)
{
    const int last = T.run1;
    if (T.run0 > T.pre0) {
        if (!in || !in->dev || in->device != c->device || in->k0 != T.pre0 || in->k1 != T.run0 || (int)in->n_kept.size() != T.run0 - T.pre0 || (int)in->R.size() != T.run0 - T.pre0)
            return fail(c, L3D_ERR_INVALID, "match_chain_turn: rank " + std::to_string(rank) + " was not handed the views " + std::to_string(T.pre0) + ".." + std::to_string(T.run0 - 1) + " of its predecessor");
        const ChainPreload pre = tail_preload(in->dev, in->o_best, in->o_bpos, T.pre0, T.run0, in->n_kept, in->R);
        if (int rc = run_chain(c, views, n_views, nullptr, nullptr, nullptr, nullptr, nullptr, T.run0, last, &pre)) return rc;
    } else if (int rc = run_chain(c, views, n_views, nullptr, nullptr, nullptr, nullptr, nullptr, T.run0, last)) return rc;
    report->views_computed = last - T.run0;
    // (a job sized by memory: what only a running chain needs goes back before anything else is allocated -- as the partition does)
    if (c->opt.part_release != 0) if (int rc = release_chain_scratch(c)) return rc;
    return L3D_OK;
}

// the final records on the device (a restart rewrites them) and the digests of every view held
int TurnVisit::digest_held(const ShareState& sh)
{
    const std::vector<ChainResult>& hloc = sh.hloc;
    const int exact_from = T.pre0, last = T.run1;
    if ((size_t)sh.used * sizeof(Match) > c->ch_kept.cap) return fail(c, L3D_ERR_INVALID, "match_chain_turn: the chain's result records point outside its arena");
    HIPCHK(c, hipMemcpyAsync(c->ch_res.p, hloc.data(), (size_t)n_views * sizeof(ChainResult), hipMemcpyHostToDevice, st));
    report->hash.assign((size_t)n_views, 0); report->n_kept.assign((size_t)n_views, 0); report->held.assign((size_t)n_views, 0);
    for (int k = exact_from; k < last; ++k) report->held[(size_t)k] = 1;
    const size_t tab_bytes = align256((size_t)n_views * sizeof(BlockDigest));
    HIPCHK(c, c->ch_hdr.reserve(tab_bytes + 256));
    BlockDigest* dd = c->ch_hdr.as<BlockDigest>();
    HIPCHK(c, hipMemsetAsync(dd, 0, tab_bytes, st));
    for (int k0 = exact_from; k0 < last; k0 += 32768)
        hipLaunchKernelGGL(k_block_digest, dim3(16, (unsigned)std::min(32768, last - k0)), dim3(256), 0, st, c->ch_kept.as<Match>(), c->ch_res.as<ChainResult>(), k0, dd);
    std::vector<BlockDigest> hd((size_t)n_views);
    HIPCHK(c, hipMemcpyAsync(hd.data(), dd, (size_t)n_views * sizeof(BlockDigest), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (int k = exact_from; k < last; ++k) { report->hash[(size_t)k] = hd[(size_t)k].hash; report->n_kept[(size_t)k] = hd[(size_t)k].n_kept; }
    report->arena_records = sh.used;
    return L3D_OK;
}

// ---- 2. the tail for the successor, before the records go: [records | best depth pairs | best positions] of the last `check` views of the block, in an
// allocation of its own.  The records are copied view by view (the recovery path of the partition copies one contiguous run in chunks: stage_tail_chunk)
int TurnVisit::leave_tail(const ShareState& sh, TurnHandover* out)
{
    const std::vector<ChainResult>& hloc = sh.hloc;
    turn_handover_release(out);
    const TurnRange& N = S.turns[(size_t)rank + 1];
    const int k0 = N.pre0, k1 = N.run0;
    if (k0 < T.pre0 || k1 > T.run1 || k1 < k0) return fail(c, L3D_ERR_INVALID, "match_chain_turn: the successor's preload is not covered by what this rank holds");
    long long t_rec = 0, t_seg = 0;
    for (int k = k0; k < k1; ++k) { t_rec += hloc[(size_t)k].n_kept; if (views[k].n_tbm > 0) t_seg += views[k].S_src; }
    out->device = c->device; out->k0 = k0; out->k1 = k1;
    const TailLayout tl(t_rec, t_seg);
    out->o_best = tl.o_best; out->o_bpos = tl.o_bpos; out->bytes = tl.bytes + 256;
    if (hipMalloc(&out->dev, out->bytes) != hipSuccess) { (void)hipGetLastError(); out->dev = nullptr; return fail(c, L3D_ERR_NOMEM, "match_chain_turn: the hand-over package of " + std::to_string(out->bytes >> 20) + " MB"); }
    unsigned char* G = static_cast<unsigned char*>(out->dev);
    long long at = 0;
    for (int k = k0; k < k1; ++k) {
        const ChainResult& r = hloc[(size_t)k];
        out->n_kept.push_back(r.n_kept); out->R.push_back(r.R);
        if (r.n_kept > 0) HIPCHK(c, hipMemcpyAsync(G + (size_t)at * sizeof(Match), c->ch_kept.as<Match>() + r.kept_base, (size_t)r.n_kept * sizeof(Match), hipMemcpyDeviceToDevice, st));
        at += r.n_kept;
    }
    if (t_seg > 0) {
        HIPCHK(c, hipMemcpyAsync(G + out->o_best, c->ch_best.as<float2>() + best_off[(size_t)k0], (size_t)t_seg * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(G + out->o_bpos, c->ch_bestpos.as<int>() + best_off[(size_t)k0], (size_t)t_seg * 4, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return L3D_OK;
}

// ---- 3. the quirk store: what this rank's block owes the other turns (filed once: a second visit finds its pieces there).  Per source of an
// early-return view the records that point at one: one allocation for this rank's sources (the first piece owns it), a slice per source
int TurnVisit::file_early_slices(const EarlyReturns& E)
{
    std::vector<int> mine;
    for (int si : E.groups) if (block_owner(si, n_views, world) == rank && !store->has_early[(size_t)si]) mine.push_back(si);
    if (mine.empty()) return L3D_OK;
    HIPCHK(c, c->ch_send.reserve(EarlyPackCtl::bytes + 256));
    std::vector<int> cnt;
    if (int rc = count_early_records(c, E.ids, mine, cnt, st)) return rc;
    long long total = 0;
    for (int x : cnt) total += x;
    void* buf = nullptr;
    if (hipMalloc(&buf, (size_t)std::max<long long>(total, 1) * sizeof(Match)) != hipSuccess) { (void)hipGetLastError(); return fail(c, L3D_ERR_NOMEM, "match_chain_turn: the records that point at early-return views"); }
    // (filed at once: whatever fails below, the store owns the allocation)
    long long at = 0;
    for (size_t g = 0; g < mine.size(); ++g) {
        TurnStore::Piece& x = store->early[(size_t)mine[g]];
        x.base = buf; x.off = (size_t)at * sizeof(Match); x.n = cnt[g]; x.owns = g == 0;
        at += cnt[g];
    }
    if (int rc = pack_early_records(c, who, E.ids.size(), cnt, static_cast<Match*>(buf), st)) return rc;
    for (int si : mine) store->has_early[(size_t)si] = 1;
    return L3D_OK;
}
// ... and per view an early return's local camera numbers name, its best matches as a package
int TurnVisit::file_alias_packages(const EarlyReturns& E)
{
    std::vector<int> mine;
    size_t bytes = 0;
    for (int b : E.alias) if (block_owner(b, n_views, world) == rank && !store->has_alias[(size_t)b]) { mine.push_back(b); bytes += alias_package_bytes(views[b].S_src); }
    if (mine.empty()) return L3D_OK;
    HIPCHK(c, c->ch_send.reserve(alias_ctl_bytes(mine.size())));
    void* buf = nullptr;
    if (hipMalloc(&buf, bytes + 256) != hipSuccess) { (void)hipGetLastError(); return fail(c, L3D_ERR_NOMEM, "match_chain_turn: alias-view packages"); }
    if (int rc = pack_alias_packages(c, who, views, mine, best_off.data(), static_cast<unsigned char*>(buf), st)) { (void)hipFree(buf); return rc; }
    size_t at = 0;
    for (size_t i = 0; i < mine.size(); ++i) {
        TurnStore::Piece& x = store->alias[(size_t)mine[i]];
        x.base = buf; x.off = at; x.n = views[mine[i]].S_src; x.owns = i == 0;
        store->has_alias[(size_t)mine[i]] = 1;
        at += alias_package_bytes(views[mine[i]].S_src);
    }
    return L3D_OK;
}

// ---- 4. the share: the slices of the views this rank does not hold come out of the store (the partition reads them from the gathered buffers)
int TurnVisit::build_share(const EarlyReturns& E, ShareState& sh, double chain_ms)
{
    const std::vector<TurnEarly>& early = E.views;
    // option regrow_free_mb: the slices stay within the room of the turn's arena
    const ArenaGrow grow_within_room{ c, c->turn_arena_room, rank };
    TurnNeeds need;
    turn_needs(early, T, need);
    for (int si : need.src) {
        if (!store->has_early[(size_t)si]) return fail(c, L3D_ERR_INVALID, "match_chain_turn: rank " + std::to_string(rank) + " builds its share before the records of view " + std::to_string(views[si].view_id) + " that point at early-return views are filed");
        const TurnStore::Piece& x = store->early[(size_t)si];
        if (x.n <= 0) continue;
        if (!x.base) return fail(c, L3D_ERR_INVALID, "match_chain_turn: a filed slice has no allocation");
        if (int rc = ingest_early_slice(c, sh, si, reinterpret_cast<const Match*>(static_cast<const unsigned char*>(x.base) + x.off), x.n, grow_within_room, st)) return rc;
    }
    for (int b : need.alias_opt) {
        if (!store->has_alias[(size_t)b]) {
            if (std::binary_search(need.alias_req.begin(), need.alias_req.end(), b)) return fail(c, L3D_ERR_INVALID, "match_chain_turn: rank " + std::to_string(rank) + " builds its share before the best matches of view " + std::to_string(views[b].view_id) + " are filed");
            continue;
        }
        const TurnStore::Piece& x = store->alias[(size_t)b];
        if (!x.base) return fail(c, L3D_ERR_INVALID, "match_chain_turn: a filed package has no allocation");
        if (int rc = ingest_alias_package(c, who, sh, views, b, static_cast<const unsigned char*>(x.base) + x.off, grow_within_room, st)) return rc;
    }
    report->arena_records = sh.used;
    // an early-return view outside the set this share is about contributes nothing here: its entries land in other ranks' rows, and a partial list of
    // its sources would give it hypotheses its owner does not have
    std::vector<l3d_chain_view> vloc(views, views + n_views);
    for (size_t i = 0; i < early.size(); ++i) if (!need.in_E[i]) vloc[(size_t)early[i].view].n_sources = 0;
    ProductsPart part;
    int64_t n_local = 0;
    const double t3 = now_s();
    if (int rc = share_build(c, vloc.data(), n_views, map, summary, rank, world, T, sh, part, n_local)) return rc;
    // (no collective here: the node object adds the other turns' counts when all of them are through -- ctx_part_total)
    share_file(c, n_views, T, sh, part, n_local, n_local);
    report->n_pot = n_local;
    if (c->opt.timing) fprintf(stderr, "[l3d chain_turn rank %d/%d] views %d..%d warm from %d: chain %.2f ms, rows of views %d..%d, %lld potential correspondences: products %.2f ms\n",
                               rank, world, T.run0, T.run1 - 1, T.pre0, chain_ms, T.row0, T.row1 - 1, (long long)n_local, (now_s() - t3) * 1e3);
    return L3D_OK;
}

}  // namespace

int l3d::match_chain_turn(l3d_ctx* c, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int rank, int world, int window,
                          const TurnHandover* in, TurnHandover* out, TurnStore* store, bool build_share, TurnReport* report)
{
    if (!c) return L3D_ERR_INVALID;
    if (!views || n_views <= 0 || !map || !summary || !store || !report || world < 1 || rank < 0 || rank >= world || window < 0) return fail(c, L3D_ERR_INVALID, "match_chain_turn: bad argument");
    TurnVisit v{ c, views, n_views, map, summary, rank, world, store, report };
    if (turn_handover_schedule(views, n_views, world, window, &v.S)) return fail(c, L3D_ERR_INVALID, "match_chain_turn: bad schedule");
    if (!v.S.supported) return fail(c, L3D_ERR_UNSUPPORTED, "match_chain_turn: a schedule the blocks-of-views partition refuses (early returns)");
    const TurnRange T = v.T = v.S.turns[(size_t)rank];
    // option regrow_free_mb (tests: a card with less room): what the turn's arena may hold, records with their side words -- run_chain's first guess
    // and regrow and the slices of step 4 all stay within it (the compact arena of a plain turn: l3d_line3d_shard_run)
    struct RoomGuard { l3d_ctx* c; ~RoomGuard() { c->turn_arena_room = 0; } } room_guard{ c };
    c->turn_arena_room = c->opt.regrow_free_mb > 0 ? ((size_t)c->opt.regrow_free_mb << 20) / (sizeof(Match) + 4) : 0;
    c->products.valid = false;
    c->products.part = ProductsPart();
    HIPCHK(c, hipSetDevice(c->device));
    v.st = c->stream;
    if (store->device < 0) { store->device = c->device; store->early.assign((size_t)n_views, TurnStore::Piece()); store->alias.assign((size_t)n_views, TurnStore::Piece()); store->has_early.assign((size_t)n_views, 0); store->has_alias.assign((size_t)n_views, 0); }
    if (store->device != c->device || (int)store->early.size() != n_views) return fail(c, L3D_ERR_INVALID, "match_chain_turn: the store belongs to another device or scene");
    v.best_off = best_offsets(views, n_views);

    const double t0 = now_s();
    if (int rc = v.chain_piece(in)) return rc;                                                  // 1
    const double t1 = now_s();
    c->stats[0] = block_pairs(views, T.own0, T.own1);
    ShareState sh(c->ch_pin_res.as<ChainResult>(), n_views, T.pre0, T.run1, v.best_off.data());
    if (int rc = v.digest_held(sh)) return rc;
    if (out && rank + 1 < world) if (int rc = v.leave_tail(sh, out)) return rc;                 // 2
    const EarlyReturns E = turn_early_views(views, n_views, ScheduleIndex(views, n_views));
    if (world > 1) {                                                                            // 3
        if (int rc = v.file_early_slices(E)) return rc;
        if (int rc = v.file_alias_packages(E)) return rc;
    }
    if (!build_share) {
        if (c->opt.timing) fprintf(stderr, "[l3d chain_turn rank %d/%d] views %d..%d warm from %d: chain %.2f ms, tail and store %.2f ms; the share is deferred\n", rank, world, T.run0, T.run1 - 1, T.pre0, (t1 - t0) * 1e3, (now_s() - t1) * 1e3);
        return L3D_OK;
    }
    return v.build_share(E, sh, (t1 - t0) * 1e3);                                                // 4
}
