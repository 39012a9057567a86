// l3d_cc.hpp -- connected components of an edge list on the device (defined in l3d_rdd.hip; used there and by l3d_merge.hip): labels = smallest node
// id of the component.  Hooking by atomicMin on the roots + full path compression, repeated until a hooking round changes nothing:
//   k_cc_init(comp, n);  then rounds of { k_cc_hook(E, nnz, comp, changed); k_cc_compress(comp, n); } until `changed` stays 0.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/line3d_amd.h"

namespace l3d {

__global__ void k_cc_init(int* __restrict__ comp, int n);
__global__ void k_cc_hook(const l3d_edge* __restrict__ E, int nnz, int* __restrict__ comp, int* __restrict__ changed);
__global__ void k_cc_compress(int* __restrict__ comp, int n);

}  // namespace l3d
