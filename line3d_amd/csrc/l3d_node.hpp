// l3d_node.hpp -- what the node handle (line3d_host.cpp) calls in the in-process communicator (l3d_node.hip) beyond the C ABI.
#pragma once

#include "../../include/line3d_amd.h"

namespace l3d {
// every rank is out of its exchanges (between two runs of a node handle): a broken barrier is whole again
void node_comm_rearm(l3d_node_comm* c);
// the rank whose exchange broke the barrier since the last rearm (-1: none, or l3d_node_comm_abort from outside)
int node_comm_culprit(l3d_node_comm* c);
// tests (option node_fail_at): rank `rank`'s k-th exchange from now returns 1 and breaks the barrier, once; k <= 0: never
void node_comm_fail_at(l3d_node_comm* c, int rank, long long k);
}  // namespace l3d
