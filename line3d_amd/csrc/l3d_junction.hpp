// l3d_junction.hpp -- the junctions of 3-D lines ("JUNCTIONS OF 3-D LINES" in include/line3d_amd.h states every rule; tests/junction_model.py holds the
// same in numpy): a line of the table, the pair test with its closest points, where on a line a junction lies, the vertices with their star rule and
// the attachments, written once for the device (l3d_junction.hip: one row line per lane against column tiles in LDS) and for the host
// (l3d_test_junction_lines_host: the same functions in loops).  Everything is f64, every product, sum, quotient and root rounded on its own
// (-ffp-contract=off), dot products as ((x x) + (y y)) + (z z).  The file is plain C++ as well: tests/cpp/junction_asan.cpp builds it into a host
// program of its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/line3d_amd.h"

#if defined(__HIPCC__)
#define L3D_JN_HD __host__ __device__ __forceinline__
#else
#define L3D_JN_HD inline
#endif

namespace l3d {
namespace junction {

constexpr double kMaxFinite = 1.7976931348623157e308;
constexpr long long kMaxRecords = 2147483647ll;
constexpr int kMaxLines = 1 << 30;
constexpr int kEndP = 0, kEndQ = 1, kInterior = 2;
constexpr int kKindL = 0, kKindT = 1, kKindX = 2;

L3D_JN_HD bool fin(double x) { return fabs(x) <= kMaxFinite; }          // (NaN compares false)
L3D_JN_HD double dot3(const double* a, const double* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }
L3D_JN_HD double mx(double a, double b) { return a < b ? b : a; }
L3D_JN_HD double mn(double a, double b) { return b < a ? b : a; }

// A LINE OF THE TABLE: 80 bytes
struct Line { double P[3], d[3], L, tol, ext; int32_t elig, pad; };

// s: P then Q.  false: not eligible (one of the eight numbers or the length is not finite, or the length is not above 0); the entry is then all zeros
L3D_JN_HD bool prepare(const double* s, double tol, double ext, Line& o)
{
    const double v[3] = { s[3] - s[0], s[4] - s[1], s[5] - s[2] };
    const double L = sqrt(dot3(v, v));
    const bool ok = fin(s[0]) && fin(s[1]) && fin(s[2]) && fin(s[3]) && fin(s[4]) && fin(s[5]) && fin(tol) && fin(ext) && fin(L) && L > 0.0;
    for (int k = 0; k < 3; ++k) { o.P[k] = ok ? s[k] : 0.0; o.d[k] = ok ? v[k] / L : 0.0; }
    o.L = ok ? L : 0.0; o.tol = ok ? tol : 0.0; o.ext = ok ? ext : 0.0;
    o.elig = ok ? 1 : 0; o.pad = 0;
    return ok;
}

// WHERE ON A LINE the parameter s of a closest point lies
L3D_JN_HD int where_on(double s, double L, double ext)
{
    if (s + s <= L) return s <= ext ? kEndP : kInterior;
    return L - s <= ext ? kEndQ : kInterior;
}

// what the pair test of lines i < j leaves behind when it passes
struct Eval { double s, t, g, X[3]; int wi, wj; };

L3D_JN_HD int kind_of(const Eval& e) { return e.wi != kInterior ? (e.wj != kInterior ? kKindL : kKindT) : (e.wj != kInterior ? kKindT : kKindX); }

// THE PAIR TEST of the eligible lines i < j
L3D_JN_HD bool pair_eval(const Line& li, const Line& lj, double cos_max, Eval& e)
{
    const double b = dot3(li.d, lj.d);
    if (!(fabs(b) <= cos_max)) return false;
    const double w[3] = { li.P[0] - lj.P[0], li.P[1] - lj.P[1], li.P[2] - lj.P[2] };
    const double p = dot3(li.d, w), q = dot3(lj.d, w), den = 1.0 - (b * b);
    if (!(den > 0.0)) return false;
    const double s = ((b * q) - p) / den, t = (q - (b * p)) / den;
    if (!(-li.ext <= s && s <= li.L + li.ext)) return false;
    if (!(-lj.ext <= t && t <= lj.L + lj.ext)) return false;
    double r[3], X[3];
    for (int k = 0; k < 3; ++k) {
        const double ci = li.P[k] + (s * li.d[k]), cj = lj.P[k] + (t * lj.d[k]);
        r[k] = ci - cj;
        X[k] = (ci + cj) * 0.5;
    }
    const double g = sqrt(dot3(r, r));
    if (!(g <= mx(li.tol, lj.tol))) return false;
    e.s = s; e.t = t; e.g = g;
    e.X[0] = X[0]; e.X[1] = X[1]; e.X[2] = X[2];
    e.wi = where_on(s, li.L, li.ext);
    e.wj = where_on(t, lj.L, lj.ext);
    return true;
}

// a pair that is listed: it passes, and it is no X pair unless crossings are asked for
L3D_JN_HD bool pair_listed(const Line& li, const Line& lj, double cos_max, int crossings, Eval& e)
{
    return pair_eval(li, lj, cos_max, e) && (crossings != 0 || kind_of(e) != kKindX);
}

L3D_JN_HD void fill_record(int i, int j, const Eval& e, l3d_junction_record& r)
{
    r.i = i; r.j = j; r.where_i = e.wi; r.where_j = e.wj;
    r.s = e.s; r.t = e.t; r.gap = e.g;
    r.X[0] = e.X[0]; r.X[1] = e.X[1]; r.X[2] = e.X[2];
}

// THE STAR RULE for a node that is not its component's representative `rep`: the pair test between the two lines passes as an L pair at exactly
// these two ends.  e: that pair's values (its X is the record's X)
L3D_JN_HD bool spoke(const Line* tab, int node, int rep, double cos_max, Eval& e)
{
    const int a = node >> 1, r = rep >> 1;
    if (a == r) return false;
    const bool lo = a < r;
    if (!pair_eval(tab[lo ? a : r], tab[lo ? r : a], cos_max, e)) return false;
    return (lo ? e.wi : e.wj) == (node & 1) && (lo ? e.wj : e.wi) == (rep & 1);
}

// the end node of a T record
L3D_JN_HD int t_end_node(const l3d_junction_record& r) { return r.where_i != kInterior ? 2 * r.i + r.where_i : 2 * r.j + r.where_j; }
L3D_JN_HD int kind_of(const l3d_junction_record& r)
{
    return r.where_i != kInterior ? (r.where_j != kInterior ? kKindL : kKindT) : (r.where_j != kInterior ? kKindT : kKindX);
}

// the refusals that need no device, in the header's order: L3D_OK, L3D_ERR_INVALID or L3D_ERR_UNSUPPORTED, and why
inline int check_arguments(const double* lines, const double* tol, const double* ext, int n, const l3d_junction_params* prm, l3d_junction_record** records,
                           int* n_records, int32_t* node_vertex, l3d_junction_vertex** vertices, int* n_vertices, int32_t* node_attach, int32_t* counts, std::string& err)
{
    if (!records || !n_records || !vertices || !n_vertices || !counts) { err = "junction lines: a null output pointer"; return L3D_ERR_INVALID; }
    *records = nullptr; *n_records = 0; *vertices = nullptr; *n_vertices = 0;
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    if (n < 0) { err = "junction lines: a negative count"; return L3D_ERR_INVALID; }
    if (n > kMaxLines) { err = "junction lines: " + std::to_string(n) + " lines, more than 2^30"; return L3D_ERR_UNSUPPORTED; }
    if (n > 0 && (!lines || !tol || !ext || !node_vertex || !node_attach)) { err = "junction lines: a null array"; return L3D_ERR_INVALID; }
    if (!prm) { err = "junction lines: null parameters"; return L3D_ERR_INVALID; }
    if (!(prm->cos_max >= 0.0 && prm->cos_max < 1.0)) { err = "junction lines: cos_max must lie in [0, 1)"; return L3D_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {
        if (!(tol[i] >= 0.0)) { err = "junction lines: tol[" + std::to_string(i) + "] is negative or not a number"; return L3D_ERR_INVALID; }
        if (!(ext[i] >= 0.0)) { err = "junction lines: ext[" + std::to_string(i) + "] is negative or not a number"; return L3D_ERR_INVALID; }
    }
    return L3D_OK;
}

// chunks of column tiles per row block of the device search (the grid's y dimension), by the rule of merge::chunks: 1 from 512 row blocks on; below,
// enough for about 1024 workgroups, at most one per tile and at most 64, and n x chunks stays below 2^30 (the scan's length)
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

// counts[8] = eligible lines, L records, T records, X records, components with an edge, vertices, nodes released, nodes attached.  comp: per node the
// label of its component (a node index); stay: per node
inline void tally(int n, const Line* tab, const l3d_junction_record* rec, size_t n_rec, const int32_t* comp, const unsigned char* stay, int n_vertices,
                  const int32_t* node_attach, int32_t* counts)
{
    const size_t nn = 2 * (size_t)n;
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    for (int i = 0; i < n; ++i) counts[0] += tab[i].elig ? 1 : 0;
    for (size_t k = 0; k < n_rec; ++k) ++counts[1 + kind_of(rec[k])];
    std::vector<int32_t> size(nn, 0), kept(nn, 0);
    for (size_t v = 0; v < nn; ++v) { ++size[(size_t)comp[v]]; kept[(size_t)comp[v]] += stay[v] ? 1 : 0; }
    for (size_t v = 0; v < nn; ++v) {
        if (size[v] >= 2) { ++counts[4]; counts[6] += size[v] - kept[v]; }
        counts[7] += node_attach[v] >= 0 ? 1 : 0;
    }
    counts[5] = n_vertices;
}

// the whole call on the host.  rec: ascending by (i, j); false: more than kMaxRecords records
inline bool run_host(const double* lines, const double* tol, const double* ext, int n, double cos_max, int crossings, std::vector<l3d_junction_record>& rec,
                     int32_t* node_vertex, std::vector<l3d_junction_vertex>& vert, int32_t* node_attach, int32_t* counts)
{
    const size_t nn = 2 * (size_t)n;
    std::vector<Line> tab((size_t)n);
    for (int i = 0; i < n; ++i) prepare(lines + 6 * (size_t)i, tol[i], ext[i], tab[(size_t)i]);
    std::vector<int32_t> comp(nn);
    for (size_t v = 0; v < nn; ++v) comp[v] = (int32_t)v;
    auto root = [&](int x) { while (comp[(size_t)x] != x) { comp[(size_t)x] = comp[(size_t)comp[(size_t)x]]; x = comp[(size_t)x]; } return x; };
    Eval e;
    for (int i = 0; i < n; ++i) {
        if (!tab[(size_t)i].elig) continue;
        for (int j = i + 1; j < n; ++j) {
            if (!tab[(size_t)j].elig || !pair_listed(tab[(size_t)i], tab[(size_t)j], cos_max, crossings, e)) continue;
            if ((long long)rec.size() >= kMaxRecords) return false;
            l3d_junction_record r;
            fill_record(i, j, e, r);
            rec.push_back(r);
            if (kind_of(e) != kKindL) continue;
            const int a = root(2 * i + e.wi), b = root(2 * j + e.wj);
            if (a != b) comp[(size_t)(a < b ? b : a)] = a < b ? a : b;            // (the smaller index stays the root)
        }
    }
    for (size_t v = 0; v < nn; ++v) comp[v] = root((int)v);
    // the representative: the node of the longest line, at equal L the lowest node (ascending nodes: the first that holds the maximum)
    std::vector<int32_t> rep(nn, -1), low(nn, -1), kept(nn, 0), vidx(nn, -1);
    for (size_t v = 0; v < nn; ++v) {
        if (!tab[v >> 1].elig) continue;
        int32_t& r = rep[(size_t)comp[v]];
        if (r < 0 || tab[v >> 1].L > tab[(size_t)r >> 1].L) r = (int32_t)v;
    }
    // the star rule, the lowest staying node and the staying nodes of every component
    std::vector<unsigned char> stay(nn, 0);
    for (size_t v = 0; v < nn; ++v) {
        if (!tab[v >> 1].elig) continue;
        const int c = comp[v], r = rep[(size_t)c];
        const bool s = (int)v == r || spoke(tab.data(), (int)v, r, cos_max, e);
        stay[v] = s ? 1 : 0;
        if (s) { if (low[(size_t)c] < 0) low[(size_t)c] = (int32_t)v; ++kept[(size_t)c]; }
    }
    // the vertices in the order of their lowest staying nodes; positions: the sum in ascending node order, then one division per coordinate
    for (size_t v = 0; v < nn; ++v) {
        const int c = comp[v];
        if (!stay[v] || kept[(size_t)c] < 2 || low[(size_t)c] != (int32_t)v) continue;
        vidx[(size_t)c] = (int32_t)vert.size();
        l3d_junction_vertex o;
        o.X[0] = o.X[1] = o.X[2] = 0.0; o.first_node = (int32_t)v; o.degree = kept[(size_t)c];
        vert.push_back(o);
    }
    for (size_t v = 0; v < nn; ++v) {
        const int c = comp[v];
        const bool in = stay[v] && kept[(size_t)c] >= 2;
        node_vertex[v] = in ? vidx[(size_t)c] : -1;
        node_attach[v] = -1;
        if (!in || (int)v == rep[(size_t)c]) continue;
        spoke(tab.data(), (int)v, rep[(size_t)c], cos_max, e);
        l3d_junction_vertex& o = vert[(size_t)vidx[(size_t)c]];
        for (int k = 0; k < 3; ++k) o.X[k] = o.X[k] + e.X[k];
    }
    for (l3d_junction_vertex& o : vert) { const double m = (double)(o.degree - 1); for (int k = 0; k < 3; ++k) o.X[k] = o.X[k] / m; }
    // the attachments: per free end the T record with the smallest (gap, index)
    for (size_t k = 0; k < rec.size(); ++k) {
        if (kind_of(rec[k]) != kKindT) continue;
        const int v = t_end_node(rec[k]);
        if (node_vertex[v] >= 0) continue;
        if (node_attach[v] < 0 || rec[k].gap < rec[(size_t)node_attach[v]].gap) node_attach[v] = (int32_t)k;
    }
    tally(n, tab.data(), rec.data(), rec.size(), comp.data(), stay.data(), (int)vert.size(), node_attach, counts);
    return true;
}

}  // namespace junction
}  // namespace l3d
