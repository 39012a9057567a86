// l3d_chain_common.hpp -- what the single-GPU resident chain (l3d_chain.hip) and the sharded one (l3d_chain_sharded.hip) share: the
// validation of the caller's view descriptions, the layout and upload of the static tables, the per-view slices of the whole-run
// arenas, the argument blocks of the kernels and the sizing rules (first capacity guesses, LDS image of the window kernel).  One copy
// of every rule; the two files differ in what happens BETWEEN the views (an arena slice vs. a slot and an exchange).
// Behind those: what the partitioned jobs on top of either chain share (l3d_chain_partition.hip, l3d_shard_chain_partition) -- the index of a
// schedule's view ids, the release of the chain's scratch, a rank's ranges as views of the dense map.
#pragma once

#include <algorithm>
#include <initializer_list>
#include <utility>
#include <vector>

#include "l3d_ctx.hpp"

namespace l3d {

struct ChainViewDev {               // device addresses of one view's static tables and its slices of the whole-run arenas
    const float4 *src = nullptr, *tgt = nullptr;
    size_t o_off = 0, o_F = 0, o_R = 0, o_C = 0, o_P = 0, o_Rs = 0, o_Cs = 0, o_tbm = 0, o_l2g = 0, o_sc = 0, o_si = 0, o_ss = 0;   // offsets into the table block
    unsigned long long* mask = nullptr;
    int* rowcnt = nullptr;
    int* rowA = nullptr;            // row starts of the stage-1 candidates alone (S*N + 1)
    int* rowub = nullptr;           // fused row starts: k_pair_mask's (upper-bound) counts, S*N, and their 256-row block sums (never rewritten)
    int* rowblk = nullptr;
    int* stats = nullptr;           // {raw total, raw max per segment}
    float2* best = nullptr;
    int* bestpos = nullptr;         // per segment: position (in the view's kept slice) of its best kept match or -1 (k_kept_write_chain)
    int* rt = nullptr;              // run table of the view's kept list, (N + 1) x S (l3d_runtable.hpp; the single-GPU chain's verified views)
    float4* rays = nullptr;         // unit viewing rays of the target endpoints (2 per target entry), k_tgt_rays
    float4* src_rays = nullptr;     // ... of the view's own end points (2 per source segment)
    int W64 = 0, maxW = 0;
    int s0 = 0, s1 = 0;             // this rank's source-segment range ([0, S) in the single-GPU chain)
    bool verified = false;
};

struct ChainLayout {
    size_t tab_bytes = 0, mask_bytes = 0, max_mask_bytes = 0, rowcnt_ints = 0, best_elems = 0;
    size_t rowA_ints = 0, rowub_ints = 0, rowblk_ints = 0;
    int maxS = 0, maxN = 0;
    double pairs = 0, max_pairs = 0;        // stage-1 pairs of this rank's ranges: all views / the largest view
    const unsigned char* dtab = nullptr;    // the table block on the device
};

// Validates the views, makes their segment arrays resident, lays out the table block (rank, world: the source-segment ranges).
int chain_plan_views(l3d_ctx* c, const l3d_chain_view* views, int n_views, int rank, int world, std::vector<ChainViewDev>& vd, ChainLayout& L, const char* what);
// Packs the tables into the pinned block, uploads them, fills the target-ray table (one launch) -- all on `st`.
int chain_upload_tables(l3d_ctx* c, const l3d_chain_view* views, int n_views, std::vector<ChainViewDev>& vd, ChainLayout& L, hipStream_t st);
// Reserves the whole-run arenas (bit rows, row counts, row starts [+ upper-bound counts and block sums], best depths [+ positions]) and
// hands every view its slices; zeroes what the kernels add into.
// mask_ring: slots of the bit-row arena (a view's bit rows live from its k_pair_mask to its k_pair_fill, both on the stage-1 stream in order:
// two slots instead of one slice per view -- 24.6 MB x 2048 views = 50 GB at 4000 segments x 24 neighbours); 0: one slice per view.
int chain_assign_arenas(l3d_ctx* c, const l3d_chain_view* views, int n_views, std::vector<ChainViewDev>& vd, ChainLayout& L, bool fused_rows, bool best_positions, int mask_ring, hipStream_t st, bool with_rt = false);
// Per-launch scratch that depends on the candidate capacity (candidate store, window scratch, stage-1 ring of `ring` slots).
int chain_reserve_candidates(l3d_ctx* c, const ChainLayout& L, size_t cand_cap, int ring);

PairArgs chain_pair_args(const l3d_ctx* c, const l3d_chain_view& v, const ChainViewDev& d, const unsigned char* dtab);
// Stage 1 of a chain view, from chain_pair_args(): the arguments of its k_pair_mask launch and of its k_pair_fill launch (the chains and
// l3d_test_pair_candidates).  fused_rows: no scan launch in between -- k_pair_mask adds its (upper-bound) counts into rowub and their 256-row
// block sums into rowblk, k_pair_fill forms a row's start from them, writes it to rowA and the row's true count to rowcnt; else k_pair_mask
// adds into rowcnt, a scan launch turns that into rowA, and k_pair_fill replaces the row's count by the true one.
// (k_pair_mask sums the blocks of one workgroup's rows -- up to 64, N apart -- in an LDS table of 26 entries: up to 96 neighbours)
inline bool chain_fused_rows(int maxN) { return maxN <= 96; }
PairArgs chain_mask_args(const PairArgs& pa, const ChainViewDev& d, bool fused_rows);
PairArgs chain_fill_args(const PairArgs& pa, const ChainViewDev& d, bool fused_rows, size_t cand_cap);
// One view's two jobs of k_tgt_rays (its targets under their cameras, its own segments under its own) appended to `jobs`, the view's slices of the
// ray table at rbase + 2 * ro handed to it (ro advances by the entries taken).
void chain_view_ray_jobs(const l3d_chain_view& v, ChainViewDev& d, const unsigned char* dtab, float4* rbase, size_t& ro, std::vector<RayJob>& jobs);
// everything of VerifyArgs that does not depend on the chain flavour (candidate arrays of the context, tables, range, parameters)
VerifyArgs chain_verify_args(l3d_ctx* c, const l3d_chain_view& v, const ChainViewDev& d, const unsigned char* dtab, size_t cand_cap);
// the window kernel's launch on those arguments (LDS image from the raw maximum per segment, or the largest the budget allows), or the
// all-pairs kernel + per-segment epilogue beyond ~50 neighbours / in all-pairs mode
void chain_launch_verify(l3d_ctx* c, VerifyArgs& va, const ChainViewDev& d, const int* exist_cams, int n_exist_cams, int raw_max_per_segment, size_t cand_cap, hipStream_t st, int mmax_given = 0);

// first guess of the candidate capacity from the largest view's pair count (raw density ~6 % + reverse matches; guarded on the device)
inline size_t chain_first_cand_cap(double max_pairs) { return (size_t)(max_pairs * 0.12) + 65536; }
// The size (records) the single-GPU chain grows its kept arena to when a view overflowed it -- run_chain, and l3d_test_arena_regrow for
// tests/test_regrow_cases_cpu.py.  arena_cap: the arena that overflowed; kept_base: the records in use; n_want: what the view keeps; done of span:
// views of THIS call finished, preloaded ones included (a ranged chain -- a block of views -- must not size its arena for the whole scene);
// free_bytes: the free HBM (kRegrowFreeUnknown: not known -- no cut, no NOMEM); turn_room: the room of a turn under option regrow_free_mb (records;
// the room is the arena's, nothing is kept back from it); early: the chain transposes early; products: it builds the products (a dense map was given).
//   The doubling, or the projection from the views done when there are enough of them (dense scenes keep 10x the first guess).  The first views of a
// chain have few sources yet and keep less than the later ones (40 x 4000 x 24: the projection at view 8 x 1.3 fell 2 % short, the arena overflowed
// again at view 38 and DOUBLED to 9.8 GB -- an allocation that took 3 to 250 ms): 1.5 early on; past the middle the projection is good and replaces
// the doubling.
//   Records are indexed with 64 bits: memory is the only bound.  The new arena must hold the records in use AND the view that overflowed (n_want: its
// true count), so that its re-run cannot overflow again: `need`.  The old arena and side array stay allocated until the used part is copied over, so
// near the top of HBM the new ones must fit BESIDE them (per_rec bytes a record: the record, its side word, an early-transpose entry below 2^31
// records, 8 B of the products' table), next to what the products will take (`reserve`: their smallest transient blocks, 6.4 GB, + 1 GB): a size above
// what fits is cut down to it -- and when what fits cannot hold that view or is no larger than the arena that just overflowed, the answer is !ok
// (NOMEM and the sizes).  Every regrow grows the arena and lets the view through: the restarts are bounded.
constexpr size_t kRegrowFreeUnknown = ~(size_t)0;
struct ArenaRegrow { size_t new_cap, need, fits, per_rec, reserve; bool ok; };
inline ArenaRegrow chain_arena_regrow(size_t arena_cap, uint64_t kept_base, int n_want, int done, int span, size_t free_bytes, size_t turn_room, bool early, bool products)
{
    ArenaRegrow g;
    g.new_cap = arena_cap * 2;
    if (done >= 4) {
        const size_t proj = (size_t)((double)kept_base / done * span * (2 * done < span ? 1.5 : 1.15)) + 1048576;
        g.new_cap = 2 * done < span ? std::max(g.new_cap, proj) : std::max(proj, arena_cap + arena_cap / 8);
    }
    g.need = (size_t)kept_base + (size_t)std::max(0, n_want) + 65536;
    g.new_cap = std::max(g.new_cap, g.need);
    const bool known = free_bytes != kRegrowFreeUnknown;
    g.per_rec = sizeof(Match) + 4 + (early && g.new_cap < 0x7ffffff0ull ? 4 : 0) + (products ? 8 : 0);
    g.reserve = turn_room ? 0 : products ? (size_t)((1ll << 28) * 24) + ((size_t)1 << 30) : (size_t)512 << 20;
    g.fits = turn_room ? turn_room : known && free_bytes > g.reserve ? (free_bytes - g.reserve) / g.per_rec : 0;
    g.ok = true;
    if (known && g.new_cap > g.fits) {
        if (g.fits < g.need || g.fits <= arena_cap) g.ok = false;
        else g.new_cap = g.fits;
    }
    return g;
}
// Lanes that share a run when a view collects its reverse matches through the run tables (k_exist_count_rt, k_place_rt): always a power of two in
// [1, 64] -- both kernels cut their workgroup into groups of g lanes (256 / g and 1024 / g of them) and step their segment loops by the number of
// groups, so a g above the workgroup would make that step 0 (the loop never ends) and a g that does not divide it would let the last, partial group
// take the next workgroup's first segments a second time.  opt (option rt_g) < 0: the average run of the lists seen so far rounded up to a power of
// two; 0: a run per thread; > 0: that many, rounded DOWN to a power of two and clamped to 64.
inline int rt_lanes_per_run(int opt, double avg_run)
{
    if (opt == 0) return 1;
    int g = 1;
    if (opt < 0) { while (g < 64 && g < avg_run) g <<= 1; return g; }
    while (g < 64 && 2 * g <= opt) g <<= 1;
    return g;
}
// Views keep more than this many records each on average (option long_list; 0: 2^18): the following views read their sources' runs instead of
// scanning their lists (k_exist_count_rt / k_place_rt), and the chain transposes the products' pairs itself (prod_early = 1).
inline int chain_long_list(const Options& o) { return o.long_list > 0 ? o.long_list : 262144; }
// How a view of the resident chain collects its reverse matches, from the lists seen so far (avg_kept records per view; any_seen: the host has read a
// result record yet) -- shared by run_chain and l3d_test_collect_candidates:
//   bps     workgroups per source view of the two scans of the sources' lists: a thread walks its stride of a list with dependent loads, so the list must
//           be spread over enough of them -- 32 x 256 threads take config 2's 36 k records in 5 steps, but 3.5 M records (4000 x 24) in 430
//   rt      the run-table route (long lists); rt_g lanes per run, rt_bps workgroups per source to cover its segments
struct CollectRule { int bps, rt_g, rt_bps; bool rt; double avg_run; };
inline CollectRule chain_collect_rule(const Options& o, bool any_seen, double avg_kept, int S, int N, int maxS)
{
    CollectRule r;
    if (!any_seen) avg_kept = 0.0;
    r.bps = (int)std::min(512.0, std::max(32.0, avg_kept / 4096.0));
    r.avg_run = any_seen ? avg_kept / std::max(1.0, (double)S * std::max(1, N)) : 1.0;
    r.rt_g = rt_lanes_per_run(o.rt_g, r.avg_run);
    r.rt_bps = std::max(1, std::min(512, (maxS * std::max(1, r.rt_g) + 255) / 256));
    r.rt = any_seen && avg_kept > (double)chain_long_list(o);
    return r;
}
// the LOCAL camera number view v has in the neighbour list of its q-th source (run tables: which runs of the source's list point at v); -1: not listed
inline int chain_source_slot(const l3d_chain_view* views, const l3d_chain_view& v, int q)
{
    const l3d_chain_view& w = views[v.source_index[q]];
    for (int j = 0; j < w.N && w.local2global; ++j) if (w.local2global[j] == v.view_id) return j;
    return -1;
}
inline size_t chain_align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// internal to the library: not among its dynamic symbols
#define L3D_HIDDEN __attribute__((visibility("hidden")))

// The chain position of a view id, over one schedule.  Host only: no context, no device.
struct L3D_HIDDEN ScheduleIndex {
    ScheduleIndex(const l3d_chain_view* views, int n_views);
    int find(unsigned view_id) const;       // chain position, or -1
    // the largest distance, in chain positions, between a view and one of its neighbours (0: no neighbour is in the schedule)
    int neighbour_reach() const;
private:
    const l3d_chain_view* views;
    int n;
    std::vector<std::pair<unsigned, int>> idx;      // (view_id, position), sorted
};

// What only a running chain needs (candidate store and its ring, window scratch, bit rows, viewing rays, row counters: 10-15 GB at 4000 segments x 24
// neighbours), given back once both streams are idle -- a job sized by memory does this before it builds its products.  extra: the caller's own.
L3D_HIDDEN int release_chain_scratch(l3d_ctx* c, std::initializer_list<DevBuf*> extra = {});

// The status words of the partitioned jobs: every rank publishes ONE word (`own`: device, 256 B; negative by convention = this rank failed), the words
// are exchanged with tag -3 (`all`: device, world x 256 B) and read back with one synchronisation.  A rank that cannot publish sends -1 and still
// enters the exchange: nobody is left waiting.  Each caller words its own messages: publish / read are the HIP errors of the two halves, !exchanged the
// failure of the exchange itself (every rank's does; `words` is then not filled).
struct StatusWords { hipError_t publish = hipSuccess, read = hipSuccess; bool exchanged = false; };
L3D_HIDDEN StatusWords exchange_status_words(l3d_exchange_fn exchange, void* user, int world, long long mine, void* own, void* all, hipStream_t st, std::vector<long long>& words);

// the dense view a chain view is (ids ascend in both; k >= n_views: one past the last)
L3D_HIDDEN int chain_dense_view(const l3d_chain_view* views, int n_views, const l3d_dense_map* map, int k);
// a rank's share of partitioned products from its ranges in chain positions: its block, the views whose rows it builds, the views it holds
L3D_HIDDEN ProductsPart products_part(const l3d_chain_view* views, int n_views, const l3d_dense_map* map, int rank, int world,
                                      int own0, int own1, int row0, int row1, int held0, int held1);

}  // namespace l3d
