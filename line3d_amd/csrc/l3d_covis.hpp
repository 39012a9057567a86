// l3d_covis.hpp -- co-visibility counting ("CO-VISIBILITY" in include/line3d_amd.h): what Line3D::processWorldpointList (line3D.cc:1874-1935) files
// per observation, as a closed form counted on the device, and the literal function on a scratch state for the lists the closed form does not cover.
//
// THE CLOSED FORM.  A world point seen by the views v1 ... vL in add order, each naming it once: v1 and v2 file nothing; when v3 arrives the
// `size() == 2` branch counts the pair (v1, v2) and 1 for v1 and for v2, and from the third view on the `size() >= 2` branch counts (vi, vk) for every
// i < k and 1 for vk.  So a track of fewer than three views counts nothing, and a track of L >= 3 adds 1 to common_wps[a][b] for every ordered pair
// a != b of its views and 1 to num_wps[v] of each -- whatever the add order.  A list that names an id twice leaves the closed form (self pairs, the
// `size() == 2` branch taken again): such lists are replayed through the function itself.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <unordered_map>
#include <vector>

namespace l3d {

// the three tables the function works on (l3d_line3d holds the same three)
struct CovisLinks {
    std::map<uint32_t, unsigned> num_wps;
    std::map<uint32_t, std::map<uint32_t, unsigned>> common_wps;
    std::unordered_map<uint32_t, std::vector<uint32_t>> worldpoints2views;
};

// Line3D::processWorldpointList, line3D.cc:1874-1935 -- on the tables handed in: the object's own (process_worldpoints(L*, ...) in line3d_host_views.cpp),
// or a scratch state (replay_csr below)
inline void process_worldpoints(std::map<uint32_t, unsigned>& num_wps, std::map<uint32_t, std::map<uint32_t, unsigned>>& common_wps,
                                std::unordered_map<uint32_t, std::vector<uint32_t>>& worldpoints2views, uint32_t viewID, const uint32_t* wps, int n)
{
    num_wps[viewID] = 0;
    for (int i = 0; i < n; ++i) {
        std::vector<uint32_t>& w2v = worldpoints2views[wps[i]];
        std::sort(w2v.begin(), w2v.end());
        if (w2v.size() == 2) {
            const uint32_t v1 = w2v[0], v2 = w2v[1];
            common_wps[v1][v2] += 1;
            common_wps[v2][v1] += 1;
            ++num_wps[v1];
            ++num_wps[v2];
        }
        if (w2v.size() >= 2) {
            for (uint32_t v : w2v) {
                common_wps[v][viewID] += 1;
                common_wps[viewID][v] += 1;
            }
            ++num_wps[viewID];
        }
        if (std::find(w2v.begin(), w2v.end(), viewID) == w2v.end()) w2v.push_back(viewID);
    }
}

// the lists through the function itself, in add order, on tables of its own (the view ids are the list indices) -> num_wps per list and the non-zero
// common_wps as a CSR, columns ascending.  false: more than 2^31 - 1 non-zero counts
inline bool replay_csr(const uint32_t* ids, const int64_t* list_start, int n_lists, std::vector<uint32_t>& num, std::vector<int32_t>& row_start,
                       std::vector<int32_t>& col, std::vector<uint32_t>& count)
{
    CovisLinks L;
    for (int i = 0; i < n_lists; ++i)
        process_worldpoints(L.num_wps, L.common_wps, L.worldpoints2views, (uint32_t)i, ids + list_start[i], (int)(list_start[i + 1] - list_start[i]));
    num.assign((size_t)n_lists, 0);
    row_start.assign((size_t)n_lists + 1, 0);
    col.clear(); count.clear();
    for (auto& kv : L.num_wps) num[kv.first] = kv.second;
    for (int i = 0; i < n_lists; ++i) {
        auto it = L.common_wps.find((uint32_t)i);
        if (it != L.common_wps.end())
            for (auto& e : it->second) { col.push_back((int32_t)e.first); count.push_back(e.second); }
        if (col.size() > (size_t)INT32_MAX) return false;
        row_start[(size_t)i + 1] = (int32_t)col.size();
    }
    return true;
}

// columns of the LDS histogram of k_covis_count / k_covis_write: the most one pass takes (option covis_tile: fewer)
constexpr int kCovisTileMax = 8192;
// a lane walks a track of up to this many views alone; the lanes of the wave share the walk of a longer one
constexpr int kCovisSerial = 16;

}  // namespace l3d
