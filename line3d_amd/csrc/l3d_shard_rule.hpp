// l3d_shard_rule.hpp -- the pure rules of matchViews with every view's SOURCE SEGMENTS sharded over the ranks (l3d_chain_sharded.hip; DESIGN.md
// section 6 i, iv): the layout of a slot, whether the gathered blocks live in a ring and how long it is, the first guess of the compact kept arena, when
// the ring's blocks are retired and when the chain waits for that, the layout of the ring's header block, what the gathered overflow bits say and
// what a retry is sized to.  Arithmetic on scalars: no context, no device, no HIP header.  l3d_test_shard_plan and l3d_test_shard_retire export them for
// tests/test_shard_plan_cases_cpu.py and tests/test_shard_retire_cases_cpu.py, which hold them to tests/shard_rule_model.py.
#pragma once

#include <algorithm>
#include <cstddef>
#include <string>

#include "../../include/line3d_amd.h"

namespace l3d {

constexpr size_t kShardRecordBytes = 32;            // a kept record (Match = l3d_match)
constexpr size_t kShardSlotHeaderBytes = 32;        // SlotHeader (l3d_chain_sharded.hip)
static_assert(sizeof(l3d_match) == kShardRecordBytes, "kept record");
inline size_t shard_align(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- a slot: [SlotHeader 32 B][best depth pairs float2 x seg_cap][position of every segment's best kept match int x seg_cap][kept records x slot_records]
// [side words unsigned x slot_records][run table int x (max_n + 1) x seg_cap].  Offsets are 32-aligned, the slot 256.
//   cam_off (0: none): dense scenes (slots of slot_cams_min records and more) carry a side array of (the record's local camera << 16 | its target
// segment) -- the two scans every later neighbour makes of the slot read 4 bytes per record instead of 32; + 12.5 % on the all-gather.
//   rt_off (0: none): ... and the slot's RUN TABLE (l3d_runtable.hpp; positions in the slot's records): a later neighbour reads the runs of its camera --
// 1/N of the slot -- instead of scanning the side array.
//   ring: view blocks the gathered buffer holds (view k lives in block k % ring); n_views when every block is kept
struct SlotGeom { size_t slot_bytes, best_off, bpos_off, rec_off, cam_off, rt_off; int seg_cap, slot_records, world, ring, max_n; };
// stage_bytes: a staging buffer of the host hand-over (k_pack_view): the ranks' depth pairs, then their records back to back
struct SlotPlan { SlotGeom geom; size_t stage_bytes; };
inline SlotPlan slot_geometry(int maxS, int maxN, int world, int slot_records, int slot_cams_min, int n_views)
{
    SlotPlan p;
    SlotGeom& g = p.geom;
    g.world = world;
    g.ring = std::max(1, n_views);
    g.seg_cap = (maxS + world - 1) / world + 1;
    g.slot_records = slot_records;
    g.max_n = maxN;
    g.best_off = kShardSlotHeaderBytes;
    g.bpos_off = g.best_off + (size_t)g.seg_cap * 8;
    g.rec_off = shard_align(g.bpos_off + (size_t)g.seg_cap * 4, 32);
    const size_t rec_end = g.rec_off + (size_t)slot_records * kShardRecordBytes;
    g.cam_off = slot_records >= slot_cams_min ? shard_align(rec_end, 32) : 0;
    g.rt_off = g.cam_off ? shard_align(g.cam_off + (size_t)slot_records * 4, 32) : 0;
    g.slot_bytes = shard_align(g.rt_off ? g.rt_off + ((size_t)maxN + 1) * g.seg_cap * 4 : rec_end, 256);       // (a slot with side words has a run table)
    p.stage_bytes = shard_align((size_t)world * ((size_t)g.seg_cap * 8 + (size_t)slot_records * kShardRecordBytes), 256);
    return p;
}

// ---- ring mode: when the gathered blocks of all views exceed the budget (or option slot_ring = 1) and nobody commits on the host, the buffer holds
// window + batch + 2 view blocks; a batch of older views is retired into the compact kept arena (k_shard_retire) before its blocks are reused.
// slot_ring = 0 keeps every block (what the recording tests read back through l3d_shard_chain_gathered).  A partitioned job retires by definition: what
// a rank does not keep is gone when its ring block is reused (a schedule that reads further back than it has views -- scattered neighbourhoods -- gets a
// ring that never wraps: all retired at the end).  send_ring: the slots this rank sends from (a slot is read by its exchange only).
constexpr int kRetireBatch = 16;
constexpr size_t kGatheredBudget = (size_t)8 << 30;
struct ShardRingPlan { bool ring_mode; int ring_views, send_ring; };
inline ShardRingPlan shard_ring_plan(int n_views, int window, size_t block_bytes, int slot_ring, bool partition, bool host_commit)
{
    const int ring = std::min(window + kRetireBatch + 2, std::max(1, n_views));
    ShardRingPlan p;
    p.ring_mode = partition || (!host_commit && slot_ring != 0 && ring < n_views && (slot_ring > 0 || (size_t)n_views * block_bytes > kGatheredBudget));
    p.ring_views = p.ring_mode ? ring : std::max(1, n_views);
    p.send_ring = p.ring_mode ? ring : n_views;
    return p;
}

// ---- the compact arena's room under option regrow_free_mb (tests: a card with less room; records): the arena and its side words may take that much
// and no more -- a first guess above it is cut to it, a run that needs more ends with the capacity verdict and l3d_line3d_shard_run's NOMEM.  0: no limit
inline long long shard_room_records(int regrow_free_mb) { return regrow_free_mb > 0 ? (long long)(((size_t)regrow_free_mb << 20) / (kShardRecordBytes + 4)) : 0; }

// ---- the first guess of the compact kept arena (records): like the single-GPU chain's, or what an earlier pass / a capacity verdict taught
// (seen_cap), or the test's cap; with option arena_guess > 4 a generous guess within 35 % of the free HBM (here a guess that is too small costs a
// capacity verdict and the whole chain again); a partitioned rank takes its share of the scene's by the views it keeps, or what an earlier pass of its
// own taught (part_seen).  free_bytes = kShardFreeUnknown: not known (or not asked: shard_guess_reads_free).
constexpr size_t kShardFreeUnknown = ~(size_t)0;
inline bool shard_guess_reads_free(bool partition, size_t test_cap, int arena_guess) { return !partition && !test_cap && arena_guess > 4; }
inline long long shard_arena_first_guess(double pairs, int world, size_t test_cap, size_t seen_cap, int arena_guess, size_t free_bytes, long long room,
                                         bool partition, long long kept_views, int n_views, size_t part_seen)
{
    long long cap = test_cap ? (long long)test_cap : std::max((long long)(pairs * world * 0.004) + 1048576, (long long)seen_cap);
    if (shard_guess_reads_free(partition, test_cap, arena_guess) && free_bytes != kShardFreeUnknown) {
        const long long want = (long long)(pairs * world * 0.001 * arena_guess) + 1048576, fits = (long long)((double)free_bytes * 0.35 / 40.0);
        cap = std::max(cap, std::min(want, fits));
    }
    if (partition && !test_cap) cap = std::max<long long>((long long)part_seen, cap * kept_views / std::max(1, n_views) + 1048576);
    if (room > 0) cap = std::min(cap, room);
    return cap;
}

// ---- when the ring's blocks are retired.  Views [0, retired) are in the compact arena (or on their way: enqueued).  The retirement copies a batch's
// records out of the ring and nothing of the chain reads what it writes: with `apart` it runs on a side stream behind the batch's exchanges, and the
// chain waits for it only before the first exchange that overwrites a block of the batch (view a + ring for a batch that starts at view a).
//   THE INVARIANT (tests/test_shard_retire_cases_cpu.py).  Block k % ring is overwritten by view k's exchange: whatever lived there (view k - ring) must
// be retired, and that retirement waited for, first.  Views in front of k - window are read by nobody from view k on; a batch goes once 16 of them
// have gathered, so retired >= k - window - 15 > k - ring with ring = window + batch + 2, and never more than k - window views are retired.
// The schedule only decides; the driver performs the HIP calls: for view k, enqueue every batch of next(due(k)), then wait if wait_due(k).
struct RetireBatch { int first, count; bool wait_before; };      // wait_before: the batch before it is still outstanding -- the chain waits for it first
struct RetireSchedule {
    int window = 0, ring = 1;
    bool apart = false;
    int retired = 0;
    int pending_first = -1;                 // the first view of the last batch on the side stream, not yet waited for; -1: nothing outstanding
    bool outstanding() const { return pending_first >= 0; }
    int waited() const { return outstanding() ? pending_first : retired; }      // views [0, waited) are retired as far as the chain's stream is concerned
    int due(int k) const { return (k - window) - retired >= kRetireBatch ? k - window : retired; }       // retire up to here before view k is enqueued
    RetireBatch next(int upto)              // the next batch of the retirement of [retired, upto); count 0: done
    {
        RetireBatch b = { retired, std::max(0, std::min(kRetireBatch, upto - retired)), false };
        if (!b.count) return b;
        b.wait_before = apart && outstanding();
        if (apart) pending_first = retired;
        retired += b.count;
        return b;
    }
    bool wait_due(int k) { return outstanding() && k >= pending_first + ring ? wait_all() : false; }     // view k's exchange needs the outstanding batch done
    bool wait_all() { const bool w = outstanding(); pending_first = -1; return w; }
};

// ---- the header block of a ring-mode run (one device allocation): every table 256-aligned
//   base      long long x (n_views + 2): arena offset of every view (+ the total behind the last), kept on the device
//   hdr       SlotHeader x n_views x world: the retired slots' headers (the shared verdict and the products read them)
//   best_off, verified, keep: per view -- where its best depth pairs go, whether it is verified, (partitioned) whether this rank keeps it
//   overflow  one int: the compact arena was too small
//   status    (world + 1) x 256 B: this rank's status word, then every rank's (exchange tag -3)
//   rt_off, view_sn: per view -- where its run table starts in ch_rt, its (S, N)
struct RingTables { size_t base, hdr, best_off, verified, overflow, keep, status, rt_off, view_sn, total; };
inline RingTables ring_tables(size_t n_views, int world)
{
    auto al = [](size_t b) { return shard_align(b, 256); };
    RingTables t;
    t.base = 0;
    t.hdr = al((n_views + 2) * 8);
    t.best_off = t.hdr + al(n_views * world * kShardSlotHeaderBytes);
    t.verified = t.best_off + al(n_views * 8);
    t.overflow = t.verified + al(n_views);
    t.keep = t.overflow + 256;
    t.status = t.keep + al(n_views);
    t.rt_off = t.status + 256 * ((size_t)world + 1);
    t.view_sn = t.rt_off + al(n_views * 8);
    t.total = t.view_sn + al(n_views * 8);
    return t;
}

// ---- the verdict every rank shares: the OR of the overflow bits of all gathered slot headers
enum : int { kShardBitCandidates = 1, kShardBitSlot = 2, kShardBitGaveUp = 4, kShardBitArena = 8, kShardBitsCapacity = 1 | 2 | 8 };
struct ShardVerdict { int rc; std::string text; };
inline ShardVerdict shard_verdict(int bits, int max_cand, int max_kept, long long arena_total)
{
    ShardVerdict v = { L3D_OK, std::string() };
    if (!bits) return v;
    v.rc = L3D_ERR_NOMEM;
    v.text = std::string("l3d_shard_chain_run:") +
             ((bits & kShardBitCandidates) ? " candidate capacity exceeded on a rank (" + std::to_string(max_cand) + " candidates in one view's range; l3d_set_chain_capacities);" : "") +
             ((bits & kShardBitSlot) ? " slot_records too small (" + std::to_string(max_kept) + " kept matches in one view's range);" : "") +
             ((bits & kShardBitArena) ? " the compact kept arena of the slot ring is too small (" + std::to_string(arena_total) + " kept matches);" : "") +
             ((bits & kShardBitGaveUp) ? " a rank gave up;" : "");
    return v;
}

// ---- what l3d_line3d_shard_run does with a NOMEM verdict: every rank reopens with the same, larger capacities and runs again (0: as it was).  No
// capacity bit: nothing a retry would change.  refuse_for_room: the compact arena needs more than option regrow_free_mb leaves -- a run that needs
// more has its answer, no re-run.  replay: recorded blocks have the recorded slot size -- the caller records again with more room.
struct ShardRetry { bool retry, refuse_for_room; size_t cand_cap_next; int slot_records_next; size_t arena_cap_next; };
inline ShardRetry shard_retry(int bits, size_t cand_cap, int max_cand, int slot_records, int max_kept, long long arena_needed, long long room, bool replay)
{
    ShardRetry r = { false, false, 0, 0, 0 };
    if (!(bits & kShardBitsCapacity)) return r;
    if (bits & kShardBitArena) {
        if (room > 0 && arena_needed > room) { r.refuse_for_room = true; return r; }
        r.arena_cap_next = (size_t)arena_needed + (size_t)arena_needed / 4 + 65536;
    }
    if ((bits & kShardBitSlot) && replay) { r.arena_cap_next = 0; return r; }
    r.retry = true;
    if (bits & kShardBitCandidates) r.cand_cap_next = std::max(cand_cap * 2, (size_t)max_cand + (size_t)max_cand / 4 + 65536);
    if (bits & kShardBitSlot) r.slot_records_next = std::max(slot_records * 2, max_kept + max_kept / 4 + 1024);
    return r;
}

}  // namespace l3d
