// l3d_turns.hpp -- what the node handle (line3d_host.cpp) sets on a rank's context when the ranks of a node object take turns on one device
// (l3d_line3d_set_node_mode 2) beyond the C ABI.  Internal flags: none of them is an option, none is read from the environment.
#pragma once

#include <vector>

#include "../../include/line3d_amd.h"

namespace l3d {
// on: a world-1 partitioned run with the options part_vrank / part_vworld files its products as rank part_vrank of part_vworld ranks
// (ProductsPart.rank / .world) -- the collective finish of that many ranks follows; off: the standalone share (scripts/run_rank_share.py)
void ctx_turn_share(l3d_ctx* c, int on);
// l3d_affinity_fill_sharded calls gate(user, 1) before and gate(user, 0) after this rank's candidate enumeration (null: no gate)
void ctx_fill_gate(l3d_ctx* c, void (*gate)(void* user, int acquire), void* user);
// on: past the last collective of l3d_affinity_fill_sharded this rank forms no numbering and no edge list and returns an empty one
void ctx_fill_collective_only(l3d_ctx* c, int on);
// the last sharded run's kept count of every chain view, from the slot headers (every rank sees every header, whatever it retired)
const std::vector<int>& ctx_shard_view_kept(const l3d_ctx* c);
// a rank whose result nobody reads gives back what the collective finish left on its device: its share of the products, the fill's tables and slots
void ctx_release_share(l3d_ctx* c);
// the entries of the table over ALL ranks, once the node object knows them (ProductsPart.n_pot_all of a share built without a collective)
void ctx_part_total(l3d_ctx* c, long long n_pot_all);

// ---- turns that hand the chain over (l3d_line3d_set_turn_handover): turn r computes its own piece of the chain, warm from the tail turn r - 1 left ----
// What the static schedule says about one turn (every range in chain positions).  The turn takes over [pre0, run0) from its predecessor, computes
// [run0, run1), holds the one chain's records of [pre0, run1), builds the rows of [row0, row1) and owns [own0, own1).  deferred: something its share
// ingests -- the records of a source that point at an early-return view, the best matches of a view an early return's local camera numbers name --
// belongs to a LATER turn's block: the turn runs its piece in order (the successor needs the tail), builds nothing and comes back after the last turn.
struct TurnRange { int pre0 = 0, run0 = 0, run1 = 0, row0 = 0, row1 = 0, own0 = 0, own1 = 0, deferred = 0; };
// the schedule of all W turns; supported = false: a scene the blocks-of-views partition refuses (more than 64 early returns or 480 of their sources,
// or a view that a turn would ingest both as such a source and as a named view) -- such a compute3Dmodel runs as plain mode 2
struct TurnSchedule { int reach = 0, check = 0, tail = 0; bool supported = true; std::vector<TurnRange> turns; };
// no context, no device: the same role as l3d_partition_keep_views.  window: the largest distance of a view to one of its sources (<= 0: from the schedule)
int turn_handover_schedule(const l3d_chain_view* views, int n_views, int world, int window, TurnSchedule* out);

// the tail a turn leaves its successor: records, best depth pairs, best positions and the result words of the views [k0, k1), in one device
// allocation [records | best depth pairs | best positions] (the layout of the recovery path of l3d_match_chain_partition).  Owned by the node
// object: it outlives l3d_chain_release_records of the sender.
struct TurnHandover {
    int device = -1, k0 = 0, k1 = 0;
    void* dev = nullptr;
    size_t bytes = 0, o_best = 0, o_bpos = 0;
    std::vector<int> n_kept, R;
};
void turn_handover_release(TurnHandover* p);
// what leaves a rank through exchanges in the partition and is filed here instead, once, by the turn that owns the view: per source of an
// early-return view its records that point at one (k_early_pack), per view an early return's local numbers name its best matches (k_alias_pack)
struct TurnStore {
    struct Piece { void* base = nullptr; size_t off = 0; int n = 0; bool owns = false; };      // a slice of its rank's allocation (one piece owns it)
    int device = -1;
    std::vector<Piece> early, alias;        // per chain view
    std::vector<char> has_early, has_alias;
};
void turn_store_release(TurnStore* s);
// what a visit reports to the node object
struct TurnReport {
    int views_computed = 0;
    long long n_pot = 0;                    // entries of this rank's rows of the table (a visit that built its share)
    long long arena_records = 0;            // records in the arena when the share was built (or when the chain ended: a deferred first visit)
    std::vector<uint64_t> hash;             // per chain view: k_block_digest of the views held, 0 elsewhere
    std::vector<int32_t> n_kept;
    std::vector<unsigned char> held;
};
// One visit of turn `rank` of `world`: chain piece, hand-over out, quirk store, and -- build_share -- this rank's share of the products as
// l3d_match_chain_partition leaves it (ProductsPart rank / world), by the same code (l3d_chain_partition.hip).  No collective.  L3D_ERR_UNSUPPORTED: a scene turn_handover_schedule refuses.
int match_chain_turn(l3d_ctx* c, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int rank, int world, int window,
                     const TurnHandover* in, TurnHandover* out, TurnStore* store, bool build_share, TurnReport* report);
}  // namespace l3d
// (l3d_turn_handover_plan, include/line3d_amd.h: turn_handover_schedule as plain words)
