// covis_asan.cpp -- the host side of the co-visibility counting (l3d_covis.hpp: Line3D::processWorldpointList on given tables and the replay of
// whole lists into a CSR) as a plain host program with a main of its own, for AddressSanitizer and UBSan (tests/test_covis_cases_cpu.py builds and
// runs it).  Random lists -- empty ones, ids at both ends of uint32, tracks of every length up to the number of views -- go through replay_csr and are
// compared with the closed form counted here by brute force; lists with a repeated id are replayed for the sanitizers' sake and checked for the
// self counts that make them leave the closed form.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/covis_asan.cpp -o covis_asan && ./covis_asan
#include "../../line3d_amd/csrc/l3d_covis.hpp"

#include <cstdio>
#include <random>
#include <set>

namespace {

struct Lists {
    std::vector<uint32_t> ids;
    std::vector<int64_t> start{ 0 };
    int n() const { return (int)start.size() - 1; }
    void add(const std::vector<uint32_t>& l) { ids.insert(ids.end(), l.begin(), l.end()); start.push_back((int64_t)ids.size()); }
};

// the closed form by brute force: per point the set of its views; tracks of three or more views count every ordered pair and every view once
void closed_form(const Lists& L, std::vector<uint32_t>& num, std::vector<std::map<uint32_t, unsigned>>& common)
{
    std::map<uint32_t, std::set<uint32_t>> tracks;
    for (int v = 0; v < L.n(); ++v)
        for (int64_t q = L.start[(size_t)v]; q < L.start[(size_t)v + 1]; ++q) tracks[L.ids[(size_t)q]].insert((uint32_t)v);
    num.assign((size_t)L.n(), 0);
    common.assign((size_t)L.n(), {});
    for (auto& t : tracks) {
        if (t.second.size() < 3) continue;
        for (uint32_t a : t.second) {
            ++num[a];
            for (uint32_t b : t.second) if (a != b) ++common[a][b];
        }
    }
}

bool equal_to_closed_form(const Lists& L)
{
    std::vector<uint32_t> num, cnt, enum_;
    std::vector<int32_t> rs, col;
    if (!l3d::replay_csr(L.ids.data(), L.start.data(), L.n(), num, rs, col, cnt)) return false;
    std::vector<std::map<uint32_t, unsigned>> common;
    closed_form(L, enum_, common);
    if (num != enum_ || (int)rs.size() != L.n() + 1 || rs[0] != 0) return false;
    for (int v = 0; v < L.n(); ++v) {
        if ((size_t)(rs[(size_t)v + 1] - rs[(size_t)v]) != common[(size_t)v].size()) return false;
        int q = rs[(size_t)v];
        for (auto& e : common[(size_t)v]) {
            if (col[(size_t)q] != (int32_t)e.first || cnt[(size_t)q] != e.second) return false;
            ++q;
        }
    }
    return true;
}

}  // namespace

int main()
{
    int cases = 0, bad = 0;
    std::mt19937 rng(12345);
    const uint32_t special[] = { 0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0x00010001u, 0x80010001u };
    for (int round = 0; round < 300; ++round) {
        const int V = 1 + (int)(rng() % 12), P = (int)(rng() % 40);
        std::vector<std::vector<uint32_t>> lists((size_t)V);
        for (int p = 0; p < P; ++p) {
            const uint32_t id = (rng() % 3 == 0) ? special[rng() % 9] + (uint32_t)(p << 8) * (rng() % 2) : (uint32_t)rng();
            const int len = 1 + (int)(rng() % (unsigned)V);
            std::vector<int> views((size_t)V);
            for (int v = 0; v < V; ++v) views[(size_t)v] = v;
            std::shuffle(views.begin(), views.end(), rng);
            for (int k = 0; k < len; ++k) {
                std::vector<uint32_t>& l = lists[(size_t)views[(size_t)k]];
                if (std::find(l.begin(), l.end(), id) == l.end()) l.push_back(id);
            }
        }
        Lists L;
        for (auto& l : lists) { std::shuffle(l.begin(), l.end(), rng); L.add(l); }
        ++cases;
        if (!equal_to_closed_form(L)) { ++bad; printf("round %d: the replay differs from the closed form\n", round); }
        // the same lists with one id named twice by a view that is not the first to see it: the function counts that view with itself
        int v = -1;
        for (int q = 1; q < V && v < 0; ++q)
            for (uint32_t id : lists[(size_t)q]) {
                bool earlier = false;
                for (int r = 0; r < q; ++r) earlier = earlier || std::find(lists[(size_t)r].begin(), lists[(size_t)r].end(), id) != lists[(size_t)r].end();
                if (earlier) { v = q; lists[(size_t)q].push_back(id); break; }
            }
        if (v < 0) continue;
        Lists R;
        for (auto& l : lists) R.add(l);
        std::vector<uint32_t> num, cnt;
        std::vector<int32_t> rs, col;
        ++cases;
        bool self = false;
        if (l3d::replay_csr(R.ids.data(), R.start.data(), R.n(), num, rs, col, cnt))
            for (int q = rs[(size_t)v]; q < rs[(size_t)v + 1]; ++q) self = self || col[(size_t)q] == v;
        if (!self) { ++bad; printf("round %d: a repeated id left no self count\n", round); }
    }
    // no lists at all, and lists without observations
    {
        Lists L;
        ++cases;
        if (!equal_to_closed_form(L)) ++bad;
        L.add({}); L.add({}); L.add({});
        ++cases;
        if (!equal_to_closed_form(L)) ++bad;
    }
    printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
