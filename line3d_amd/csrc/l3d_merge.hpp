// l3d_merge.hpp -- duplicate 3-D lines found and grouped ("MERGING DUPLICATE LINES" in include/line3d_amd.h states every rule; tests/merge_model.py
// holds the same in numpy): a line of the table, the pair test, and the grouping with its star rule, written once for the device (l3d_merge.hip: one
// row line per lane against column tiles in LDS) and for the host (l3d_test_merge_lines_host: the same functions in loops).  Everything is f64,
// every product, sum and quotient rounded on its own (-ffp-contract=off), dot products as ((x x) + (y y)) + (z z).  The file is plain C++ as well:
// tests/cpp/merge_asan.cpp builds it into a host program of its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/line3d_amd.h"

#if defined(__HIPCC__)
#define L3D_MG_HD __host__ __device__ __forceinline__
#else
#define L3D_MG_HD inline
#endif

namespace l3d {
namespace merge {

constexpr double kMaxFinite = 1.7976931348623157e308;
constexpr long long kMaxPairs = 2147483647ll;

L3D_MG_HD bool fin(double x) { return fabs(x) <= kMaxFinite; }          // (NaN compares false)
L3D_MG_HD double dot3(const double* a, const double* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }
L3D_MG_HD double mx(double a, double b) { return a < b ? b : a; }
L3D_MG_HD double mn(double a, double b) { return b < a ? b : a; }

// A LINE OF THE TABLE: 64 bytes (its Q stays in the caller's array: the pair test reads it there)
struct Line { double P[3], d[3], L, tol; };

// s: P then Q.  false: not eligible (a number that is not finite, or a length that is not a finite number above 0); the entry is then all zeros
L3D_MG_HD bool prepare(const double* s, double tol, Line& o)
{
    const double v[3] = { s[3] - s[0], s[4] - s[1], s[5] - s[2] };
    const double L = sqrt(dot3(v, v));
    const bool ok = fin(s[0]) && fin(s[1]) && fin(s[2]) && fin(s[3]) && fin(s[4]) && fin(s[5]) && fin(tol) && fin(L) && L > 0.0;
    for (int k = 0; k < 3; ++k) { o.P[k] = ok ? s[k] : 0.0; o.d[k] = ok ? v[k] / L : 0.0; }
    o.L = ok ? L : 0.0; o.tol = ok ? tol : 0.0;
    return ok;
}

// a is the longer of two eligible lines: at equal L the one with the lower index
L3D_MG_HD bool first_is_a(const Line& i, const Line& j) { return i.L >= j.L; }            // (for i < j)

// offset along a's axis and distance from it of the point X
L3D_MG_HD void along_across(const Line& a, const double* X, double& s, double& e)
{
    const double v[3] = { X[0] - a.P[0], X[1] - a.P[1], X[2] - a.P[2] };
    s = dot3(v, a.d);
    const double r[3] = { v[0] - s * a.d[0], v[1] - s * a.d[1], v[2] - s * a.d[2] };
    e = sqrt(dot3(r, r));
}

// THE PAIR TEST of a (the longer) and b, both eligible; Qb: the end of b
L3D_MG_HD bool pair_test(const Line& a, const Line& b, const double* Qb, double cos_min, double max_gap)
{
    if (!(fabs(dot3(a.d, b.d)) >= cos_min)) return false;
    const double tol = mx(a.tol, b.tol);
    double sP, eP, sQ, eQ;
    along_across(a, b.P, sP, eP);
    along_across(a, Qb, sQ, eQ);
    if (!(eP <= tol) || !(eQ <= tol)) return false;
    const double overlap = mn(mx(sP, sQ), a.L) - mx(mn(sP, sQ), 0.0);
    return overlap >= -(max_gap * b.L);
}

// lines i < j of the table
L3D_MG_HD bool pair_test_ij(const Line& li, const Line& lj, const double* lines, int i, int j, double cos_min, double max_gap)
{
    return first_is_a(li, lj) ? pair_test(li, lj, lines + 6 * (size_t)j + 3, cos_min, max_gap) : pair_test(lj, li, lines + 6 * (size_t)i + 3, cos_min, max_gap);
}

// the refusals that need no device, in the header's order: L3D_OK, or L3D_ERR_INVALID and why
inline int check_arguments(const double* lines, const double* tol, int n, const l3d_merge_params* prm, int32_t* group, int32_t** pairs, int* n_pairs, int32_t* counts,
                           std::string& err)
{
    if (!pairs || !n_pairs || !counts) { err = "merge lines: a null output pointer"; return L3D_ERR_INVALID; }
    *pairs = nullptr; *n_pairs = 0;
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (n < 0) { err = "merge lines: a negative count"; return L3D_ERR_INVALID; }
    if (n > 0 && (!lines || !tol || !group)) { err = "merge lines: a null array"; return L3D_ERR_INVALID; }
    if (!prm) { err = "merge lines: null parameters"; return L3D_ERR_INVALID; }
    if (!(prm->cos_min >= 0.0 && prm->cos_min <= 1.0)) { err = "merge lines: cos_min must lie in [0, 1]"; return L3D_ERR_INVALID; }
    if (!(prm->max_gap >= 0.0 && prm->max_gap <= kMaxFinite)) { err = "merge lines: max_gap must be a finite number, not negative"; return L3D_ERR_INVALID; }
    for (int i = 0; i < n; ++i)
        if (!(tol[i] >= 0.0)) { err = "merge lines: tol[" + std::to_string(i) + "] is negative or not a number"; return L3D_ERR_INVALID; }
    return L3D_OK;
}

// chunks of column tiles per row block of the device search (the grid's y dimension): 1 from 512 row blocks on; below, enough for about 1024
// workgroups, at most one per tile and at most 64, and n x chunks stays below 2^30 (the scan's length)
inline int chunks(int n)
{
    const long long tiles = ((long long)n + 255) / 256;
    if (tiles >= 512) return 1;
    long long c = (1024 + tiles - 1) / (tiles > 0 ? tiles : 1);
    if (c > tiles) c = tiles;
    if (c > 64) c = 64;
    if (n > 0 && c > (1ll << 30) / n) c = (1ll << 30) / n;
    return (int)(c < 1 ? 1 : c);
}

// counts[4] = eligible lines, components with a pair, lines released, groups of two or more lines
inline void tally(int n, const unsigned char* elig, const int32_t* comp, const unsigned char* stay, const int32_t* group, int32_t* counts)
{
    std::vector<int32_t> size((size_t)n, 0), kept((size_t)n, 0);
    for (int i = 0; i < n; ++i) if (elig[i]) { ++size[(size_t)comp[i]]; kept[(size_t)comp[i]] += stay[i] ? 1 : 0; }
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int i = 0; i < n; ++i) {
        counts[0] += elig[i] ? 1 : 0;
        if (size[(size_t)i] >= 2) { ++counts[1]; counts[2] += size[(size_t)i] - kept[(size_t)i]; counts[3] += kept[(size_t)i] >= 2 ? 1 : 0; }
    }
    (void)group;
}

// the whole call on the host.  pairs: (i, j) in ascending order; comp: smallest index of the component; false: more than kMaxPairs pairs
inline bool run_host(const double* lines, const double* tol, int n, double cos_min, double max_gap, int32_t* group, std::vector<int32_t>& pairs, int32_t* counts)
{
    std::vector<Line> tab((size_t)n);
    std::vector<unsigned char> elig((size_t)n), stay((size_t)n, 0);
    for (int i = 0; i < n; ++i) elig[(size_t)i] = prepare(lines + 6 * (size_t)i, tol[i], tab[(size_t)i]) ? 1 : 0;
    std::vector<int32_t> comp((size_t)n);
    for (int i = 0; i < n; ++i) comp[(size_t)i] = i;
    auto root = [&](int x) { while (comp[(size_t)x] != x) { comp[(size_t)x] = comp[(size_t)comp[(size_t)x]]; x = comp[(size_t)x]; } return x; };
    for (int i = 0; i < n; ++i) {
        if (!elig[(size_t)i]) continue;
        for (int j = i + 1; j < n; ++j) {
            if (!elig[(size_t)j] || !pair_test_ij(tab[(size_t)i], tab[(size_t)j], lines, i, j, cos_min, max_gap)) continue;
            if ((long long)(pairs.size() / 2) >= kMaxPairs) return false;
            pairs.push_back(i); pairs.push_back(j);
            const int a = root(i), b = root(j);
            if (a != b) comp[(size_t)(a < b ? b : a)] = a < b ? a : b;            // (the smaller index stays the root)
        }
    }
    for (int i = 0; i < n; ++i) comp[(size_t)i] = root(i);
    // the representative: the longest line, at equal L the lowest index (ascending i: the first that holds the maximum)
    std::vector<int32_t> rep((size_t)n, -1), low((size_t)n, -1);
    for (int i = 0; i < n; ++i) {
        if (!elig[(size_t)i]) continue;
        int32_t& r = rep[(size_t)comp[(size_t)i]];
        if (r < 0 || tab[(size_t)i].L > tab[(size_t)r].L) r = i;
    }
    // the star rule, and the lowest staying index of every component
    for (int i = 0; i < n; ++i) {
        if (!elig[(size_t)i]) continue;
        const int r = rep[(size_t)comp[(size_t)i]];
        const bool s = i == r || (i < r ? pair_test_ij(tab[(size_t)i], tab[(size_t)r], lines, i, r, cos_min, max_gap)
                                        : pair_test_ij(tab[(size_t)r], tab[(size_t)i], lines, r, i, cos_min, max_gap));
        stay[(size_t)i] = s ? 1 : 0;
        if (s && low[(size_t)comp[(size_t)i]] < 0) low[(size_t)comp[(size_t)i]] = i;
    }
    for (int i = 0; i < n; ++i) group[i] = stay[(size_t)i] ? low[(size_t)comp[(size_t)i]] : i;
    tally(n, elig.data(), comp.data(), stay.data(), group, counts);
    return true;
}

}  // namespace merge
}  // namespace l3d
