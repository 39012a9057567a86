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
}  // namespace l3d
