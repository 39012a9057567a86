// l3d_blocks_rule.hpp -- the pure rules of matchViews sharded by BLOCKS OF VIEWS (l3d_chain_partition.hip; DESIGN.md section 6 ii, iii): which views a
// rank owns, how far it runs and is checked, what the gathered table of digests says about every rank's speculation, and what a predecessor hands a
// rank that missed.  Arithmetic on small host arrays: no context, no device, no HIP header.  l3d_test_blocks_verdict exports them for
// tests/test_blocks_verdict_cases_cpu.py, which holds them to tests/blocks_verdict_model.py.
#pragma once

#include <algorithm>
#include <vector>

namespace l3d {

// blocks of views: rank r owns the chain positions [block_begin(r), block_begin(r + 1))
inline int block_begin(int r, int n, int world) { return (int)(((long long)n * r) / world); }
inline int block_owner(int k, int n, int world)
{
    int r = (int)(((long long)k * world) / n);
    while (r + 1 < world && block_begin(r + 1, n, world) <= k) ++r;
    while (r > 0 && block_begin(r, n, world) > k) --r;
    return r;
}

// reach: the largest distance, in chain positions, between a view and one of its neighbours or sources (every rank computes the same number).
// partitioned: a rank runs its chain `tail` = 2 x reach views PAST its block and must be exact `check` = max(window, 2 x reach) views in front of it --
// everything the rows of its block, their flags and the hypotheses they name can depend on is then computed locally (DESIGN.md section 6 iii).
// replicas: no tail, and the `window` views in front of the block are checked.
struct BlocksReach { int reach, tail, check; };
inline BlocksReach blocks_reach(int window, int neighbour_reach, bool partition)
{
    BlocksReach b;
    b.reach = std::max(window, neighbour_reach);
    b.tail = partition ? 2 * b.reach : 0;
    b.check = partition ? std::max(window, 2 * b.reach) : window;
    return b;
}

// per view of the chain: the digest of its kept list as one rank computed it (k_block_digest); zero = not computed by this rank.  The ranks' tables
// are gathered into one of world x n_views entries, rank by rank.
struct BlockDigest { unsigned long long hash; int n_kept, R; };
static_assert(sizeof(BlockDigest) == 16, "digest entry");
// (the kept LIST must be the same; R, the number of candidates it was chosen from, may differ while a warm-up converges)
inline bool digest_differs(const BlockDigest& x, const BlockDigest& y) { return x.hash != y.hash || x.n_kept != y.n_kept; }

// a rank whose chain failed publishes a table whose entry 0 is this mark (R: its error code); the first rank that did, or -1
inline BlockDigest digest_failure_mark(int code) { BlockDigest m; m.hash = ~0ull; m.n_kept = -1; m.R = code; return m; }
inline int blocks_failed_rank(const BlockDigest* tab, int n_views, int world)
{
    for (int r = 0; r < world; ++r)
        if (tab[(size_t)r * n_views].n_kept == -1 && tab[(size_t)r * n_views].hash == ~0ull) return r;
    return -1;
}

// ---- the verdict (the same on every rank: same table).  miss[r]: the `check` views in front of rank r's block did not come out of its warm-up as its
// predecessor computed them.  No miss anywhere = every rank exact (rank 0 is; rank r's check views equal rank r-1's, which are then the one chain's, and
// from them on rank r's chain had the one chain's inputs).  comp_from[r]: the first view rank r computed or took over.  first_diff[r]: the first view
// at which rank r's table differs from its predecessor's among the views compared, or -1.
struct BlocksVerdict { std::vector<char> miss; std::vector<int> first_diff; int n_miss = 0; bool hopeless = false; };
inline BlocksVerdict blocks_verdict(const BlockDigest* tab, int n_views, int world, int check, int tail, bool partition, const int* comp_from)
{
    BlocksVerdict v;
    v.miss.assign((size_t)world, 0);
    v.first_diff.assign((size_t)world, -1);
    for (int r = 1; r < world; ++r) {
        const int b = block_begin(r, n_views, world), lo = std::max(0, b - check);
        const BlockDigest *x = tab + (size_t)r * n_views, *y = tab + (size_t)(r - 1) * n_views;
        // a warm-up shorter than the check leaves views the rank never computed: a miss (the warm re-run takes them over)
        bool ok = lo >= comp_from[r];
        // (replicas: a block shorter than the window cannot vouch for its successor's sources -- the blocks are what gets gathered; partitioned: the
        // predecessor's exact range reaches back as far as this rank's check)
        if (!partition && b - check < block_begin(r - 1, n_views, world)) { ok = false; v.hopeless = true; }
        // partitioned, behind the check: the predecessor's tail against this rank's block -- both are the one chain's, or something is wrong
        const int e = partition ? std::min(std::min(n_views, b + tail), block_begin(r + 1, n_views, world)) : b;
        for (int k = lo; k < e && ok; ++k)
            if (digest_differs(x[k], y[k])) { ok = false; v.first_diff[(size_t)r] = k; }
        v.miss[(size_t)r] = ok ? 0 : 1;
        v.n_miss += ok ? 0 : 1;
    }
    return v;
}

// ---- what the sender r - 1 of every rank r that missed hands over: its last `check` views in front of block r -- t_rec records (by ITS table), t_seg
// segments of best depth pairs / positions (the verified views'; S_src each), t_first the first verified view among them (a tail's records are
// contiguous in the sender's arena from there on; -1: none) -- and the largest of each, which size the slot every rank sends
struct BlocksHandoverPlan { std::vector<long long> t_rec, t_seg; std::vector<int> t_first; long long max_rec = 0, max_seg = 0; };
inline BlocksHandoverPlan blocks_handover_plan(const BlockDigest* tab, int n_views, int world, int check, const char* miss, const char* verified, const int* S_src)
{
    BlocksHandoverPlan p;
    p.t_rec.assign((size_t)world, 0); p.t_seg.assign((size_t)world, 0); p.t_first.assign((size_t)world, -1);
    for (int r = 1; r < world; ++r) {
        if (!miss[r]) continue;
        const size_t s = (size_t)r - 1;
        const int fb = block_begin(r, n_views, world);
        for (int k = std::max(0, fb - check); k < fb; ++k) {
            p.t_rec[s] += tab[s * n_views + k].n_kept;
            if (verified[k]) { p.t_seg[s] += S_src[k]; if (p.t_first[s] < 0) p.t_first[s] = k; }
        }
        p.max_rec = std::max(p.max_rec, p.t_rec[s]); p.max_seg = std::max(p.max_seg, p.t_seg[s]);
    }
    return p;
}

}  // namespace l3d
