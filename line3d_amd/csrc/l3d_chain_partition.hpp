// l3d_chain_partition.hpp -- what the blocks-of-views partition and the turns that hand the chain over (l3d_chain_partition.hip) take from the
// single-GPU chain (l3d_chain.hip): the chain over a range of views, cold or warm from views another rank computed.
#pragma once

#include <vector>

#include "l3d_chain_common.hpp"

namespace l3d {

// the views [k0, k1) taken over from another rank, as run_chain puts them at the head of its arena
struct L3D_HIDDEN ChainPreload {
    int k0 = 0, k1 = 0;
    const Match* records = nullptr;        // device: the views' kept lists, back to back
    const float2* best = nullptr;          // device: best depth pairs of the verified views among them, back to back (S_src each)
    const int* bestpos = nullptr;          // device: ... and the positions of the best kept matches
    std::vector<int> n_kept, R;            // per view
};

// (l3d_chain.hip describes the arguments)
L3D_HIDDEN int run_chain(l3d_ctx* c, const l3d_chain_view* views, int n_views, l3d_chain_callback cb, void* user, const l3d_dense_map* map,
                         l3d_chain_summary* summary, int64_t* n_pot, int k_begin = 0, int k_end = -1, const ChainPreload* pre = nullptr);

}  // namespace l3d
