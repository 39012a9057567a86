// l3d_plane.hpp -- the planes of 3-D lines ("PLANES OF 3-D LINES" in include/line3d_amd.h states every rule; tests/plane_model.py holds the same in
// numpy): a line of the table, a hypothesis from a seed pair, the lies-in test, the hypothesis pair test, the parameters of a candidate with its frame,
// the members and the extent, written once for the device (l3d_plane.hip) and for the host (l3d_test_plane_lines_host: the same functions in loops).
// Everything is f64, every product, sum, quotient and root rounded on its own (-ffp-contract=off), dot products as ((x x) + (y y)) + (z z), cross
// products as ((a1 b2) - (a2 b1), (a2 b0) - (a0 b2), (a0 b1) - (a1 b0)).  The file is plain C++ as well: tests/cpp/plane_asan.cpp builds it into a host
// program of its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/line3d_amd.h"

#if defined(__HIPCC__)
#define L3D_PL_HD __host__ __device__ __forceinline__
#else
#define L3D_PL_HD inline
#endif

namespace l3d {
namespace plane {

constexpr double kMaxFinite = 1.7976931348623157e308;
constexpr long long kMaxRecords = 2147483647ll;
constexpr int kMaxItems = 1 << 30;
constexpr int kSeed = 1;

L3D_PL_HD bool fin(double x) { return fabs(x) <= kMaxFinite; }          // (NaN compares false)
L3D_PL_HD double dot3(const double* a, const double* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }
L3D_PL_HD void cross3(const double* a, const double* b, double* o)
{
    o[0] = (a[1] * b[2]) - (a[2] * b[1]); o[1] = (a[2] * b[0]) - (a[0] * b[2]); o[2] = (a[0] * b[1]) - (a[1] * b[0]);
}
L3D_PL_HD double mx(double a, double b) { return a < b ? b : a; }
L3D_PL_HD double mn(double a, double b) { return b < a ? b : a; }

// A LINE OF THE TABLE: 96 bytes
struct Line { double P[3], Q[3], d[3], L, tol; int32_t elig, pad; };

// s: P then Q.  false: not eligible (one of the seven numbers or the length is not finite, or the length is not above 0); the entry is then all zeros
L3D_PL_HD bool prepare(const double* s, double tol, Line& o)
{
    const double v[3] = { s[3] - s[0], s[4] - s[1], s[5] - s[2] };
    const double L = sqrt(dot3(v, v));
    const bool ok = fin(s[0]) && fin(s[1]) && fin(s[2]) && fin(s[3]) && fin(s[4]) && fin(s[5]) && fin(tol) && fin(L) && L > 0.0;
    for (int k = 0; k < 3; ++k) { o.P[k] = ok ? s[k] : 0.0; o.Q[k] = ok ? s[3 + k] : 0.0; o.d[k] = ok ? v[k] / L : 0.0; }
    o.L = ok ? L : 0.0; o.tol = ok ? tol : 0.0;
    o.elig = ok ? 1 : 0; o.pad = 0;
    return ok;
}

// LIES IN: both ends of a line within its own tolerance of the plane (N, c)
L3D_PL_HD bool lies_in(const double* P, const double* Q, double tol, const double* N, double c)
{
    return fabs(dot3(N, P) - c) <= tol && fabs(dot3(N, Q) - c) <= tol;
}

// A HYPOTHESIS as the pair search reads it (a column entry of the LDS tile): its plane, its two lines' ends and tolerances.  160 bytes
struct Hyp { double N[3], c, Pi[3], Qi[3], Pj[3], Qj[3], toli, tolj; int32_t li, lj, elig, pad; };
// and what only the parameters need: the point and the weight.  32 bytes
struct HypAux { double X[3], A; };

// the hypothesis of the seed (i, j) over the table; false: not eligible, both entries all zeros
L3D_PL_HD bool hypothesis(const Line* tab, int n, int i, int j, double cos_max, Hyp& h, HypAux& a)
{
    Hyp z = {}; HypAux za = {};
    h = z; a = za;
    h.li = i; h.lj = j;
    if (i == j || i < 0 || j < 0 || i >= n || j >= n) return false;
    const Line li = tab[i], lj = tab[j];
    if (!li.elig || !lj.elig) return false;
    const double b = dot3(li.d, lj.d);
    if (!(fabs(b) <= cos_max)) return false;
    const double den = 1.0 - (b * b);
    if (!(den > 0.0)) return false;
    double cr[3];
    cross3(li.d, lj.d, cr);
    const double mm = sqrt(dot3(cr, cr));
    if (!(mm > 0.0)) return false;
    const double w[3] = { li.P[0] - lj.P[0], li.P[1] - lj.P[1], li.P[2] - lj.P[2] };
    const double p = dot3(li.d, w), q = dot3(lj.d, w);
    const double s = ((b * q) - p) / den, t = (q - (b * p)) / den;
    for (int k = 0; k < 3; ++k) {
        const double ci = li.P[k] + (s * li.d[k]), cj = lj.P[k] + (t * lj.d[k]);
        a.X[k] = (ci + cj) * 0.5;
        h.N[k] = cr[k] / mm;
        h.Pi[k] = li.P[k]; h.Qi[k] = li.Q[k]; h.Pj[k] = lj.P[k]; h.Qj[k] = lj.Q[k];
    }
    h.c = dot3(h.N, a.X);
    h.toli = li.tol; h.tolj = lj.tol;
    a.A = (li.L * lj.L) * mm;
    h.elig = 1;
    return true;
}

// THE HYPOTHESIS PAIR TEST of two eligible hypotheses (symmetric in its arguments)
L3D_PL_HD bool pair_test(const Hyp& h, const Hyp& g, double cos_min)
{
    if (!(fabs(dot3(h.N, g.N)) >= cos_min)) return false;
    if (!lies_in(g.Pi, g.Qi, g.toli, h.N, h.c) || !lies_in(g.Pj, g.Qj, g.tolj, h.N, h.c)) return false;
    return lies_in(h.Pi, h.Qi, h.toli, g.N, g.c) && lies_in(h.Pj, h.Qj, h.tolj, g.N, g.c);
}

// THE PARAMETERS OF A CANDIDATE from its staying hypotheses stay[0 .. count) (ascending indices), rep among them; di: d of line i of the
// representative's seed.  o: N, c, u, v (rect and the integers are left alone).  false: sqrt(S . S), W or lu is not finite or not above 0
template <typename Index>
L3D_PL_HD bool parameters(const Hyp* hyp, const HypAux* aux, const Index* stay, int count, int rep, const double* di, l3d_plane& o)
{
    double S[3] = { 0.0, 0.0, 0.0 }, W = 0.0;
    for (int k = 0; k < count; ++k) {
        const int h = (int)(unsigned)stay[k];
        const double sg = dot3(hyp[h].N, hyp[rep].N) < 0.0 ? -1.0 : 1.0, as = aux[h].A * sg;
        for (int e = 0; e < 3; ++e) S[e] = S[e] + (as * hyp[h].N[e]);
        W = W + aux[h].A;
    }
    const double ns = sqrt(dot3(S, S));
    for (int e = 0; e < 3; ++e) o.N[e] = S[e] / ns;
    double T = 0.0;
    for (int k = 0; k < count; ++k) {
        const int h = (int)(unsigned)stay[k];
        T = T + (aux[h].A * dot3(o.N, aux[h].X));
    }
    o.c = T / W;
    const double dn = dot3(di, o.N);
    double up[3];
    for (int e = 0; e < 3; ++e) up[e] = di[e] - (dn * o.N[e]);
    const double lu = sqrt(dot3(up, up));
    for (int e = 0; e < 3; ++e) o.u[e] = up[e] / lu;
    cross3(o.N, o.u, o.v);
    return fin(ns) && ns > 0.0 && fin(W) && W > 0.0 && fin(lu) && lu > 0.0;
}

// the frame coordinates (a, b) of a point X folded into rect = (min a, max a, min b, max b); first: rect is set, not folded
L3D_PL_HD void extend(const l3d_plane& p, const double* X, bool first, double* rect)
{
    const double r[3] = { X[0] - (p.c * p.N[0]), X[1] - (p.c * p.N[1]), X[2] - (p.c * p.N[2]) };
    const double a = dot3(p.u, r), b = dot3(p.v, r);
    rect[0] = first ? a : mn(rect[0], a); rect[1] = first ? a : mx(rect[1], a);
    rect[2] = first ? b : mn(rect[2], b); rect[3] = first ? b : mx(rect[3], b);
}

// the refusals that need no device, in the header's order: L3D_OK, L3D_ERR_INVALID or L3D_ERR_UNSUPPORTED, and why
inline int check_arguments(const double* lines, const double* tol, int n, const int32_t* seeds, int m, const l3d_plane_params* prm, l3d_plane** planes, int* n_planes,
                           l3d_plane_member** members, int* n_members, int32_t* hyp_plane, int32_t* counts, std::string& err)
{
    if (!planes || !n_planes || !members || !n_members || !counts) { err = "plane lines: a null output pointer"; return L3D_ERR_INVALID; }
    *planes = nullptr; *n_planes = 0; *members = nullptr; *n_members = 0;
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    if (n < 0 || m < 0) { err = "plane lines: a negative count"; return L3D_ERR_INVALID; }
    if (n > kMaxItems) { err = "plane lines: " + std::to_string(n) + " lines, more than 2^30"; return L3D_ERR_UNSUPPORTED; }
    if (m > kMaxItems) { err = "plane lines: " + std::to_string(m) + " seeds, more than 2^30"; return L3D_ERR_UNSUPPORTED; }
    if ((n > 0 && (!lines || !tol)) || (m > 0 && (!seeds || !hyp_plane))) { err = "plane lines: a null array"; return L3D_ERR_INVALID; }
    if (!prm) { err = "plane lines: null parameters"; return L3D_ERR_INVALID; }
    if (!(prm->cos_max >= 0.0 && prm->cos_max < 1.0)) { err = "plane lines: cos_max must lie in [0, 1)"; return L3D_ERR_INVALID; }
    if (!(prm->cos_min > 0.0 && prm->cos_min <= 1.0)) { err = "plane lines: cos_min must lie in (0, 1]"; return L3D_ERR_INVALID; }
    if (prm->min_lines < 2) { err = "plane lines: min_lines must be at least 2"; return L3D_ERR_INVALID; }
    for (int i = 0; i < n; ++i)
        if (!(tol[i] >= 0.0)) { err = "plane lines: tol[" + std::to_string(i) + "] is negative or not a number"; return L3D_ERR_INVALID; }
    for (int k = 0; k < m; ++k)
        for (int e = 0; e < 2; ++e)
            if (seeds[2 * (size_t)k + e] < 0 || seeds[2 * (size_t)k + e] >= n) {
                err = "plane lines: seed " + std::to_string(k) + " names line " + std::to_string(seeds[2 * (size_t)k + e]) + ", outside the table";
                return L3D_ERR_INVALID;
            }
    return L3D_OK;
}

// chunks of column tiles per row block of the device's hypothesis search (the grid's y dimension), by the rule of merge::chunks: 1 from 512 row blocks
// on; below, enough for about 1024 workgroups, at most one per tile and at most 64, and m x chunks stays below 2^30 (the scan's length)
inline int chunks(int m)
{
    const long long tiles = ((long long)m + 255) / 256;
    if (tiles >= 512) return 1;
    long long c = (1024 + tiles - 1) / (tiles > 0 ? tiles : 1);
    if (c > tiles) c = tiles;
    if (c > 64) c = 64;
    if (m > 0 && c > (1ll << 30) / m) c = (1ll << 30) / m;
    return (int)(c < 1 ? 1 : c);
}

// the whole call on the host.  0: done; 1: more than kMaxRecords edges; 2: more than kMaxRecords member records
inline int run_host(const double* lines, const double* tol, int n, const int32_t* seeds, int m, double cos_max, double cos_min, int min_lines,
                    std::vector<l3d_plane>& planes, std::vector<l3d_plane_member>& members, int32_t* hyp_plane, int32_t* counts)
{
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    for (int h = 0; h < m; ++h) hyp_plane[h] = -1;
    if (n == 0 || m == 0) return 0;
    const size_t N = (size_t)n, M = (size_t)m;
    std::vector<Line> tab(N);
    for (size_t i = 0; i < N; ++i) counts[0] += prepare(lines + 6 * i, tol[i], tab[i]) ? 1 : 0;
    std::vector<Hyp> hyp(M);
    std::vector<HypAux> aux(M);
    for (size_t h = 0; h < M; ++h) counts[1] += hypothesis(tab.data(), n, seeds[2 * h], seeds[2 * h + 1], cos_max, hyp[h], aux[h]) ? 1 : 0;
    // the components of the pair graph (the smaller index stays the root)
    std::vector<int32_t> comp(M);
    for (size_t h = 0; h < M; ++h) comp[h] = (int32_t)h;
    auto root = [&](int x) { while (comp[(size_t)x] != x) { comp[(size_t)x] = comp[(size_t)comp[(size_t)x]]; x = comp[(size_t)x]; } return x; };
    long long edges = 0;
    for (int h = 0; h < m; ++h) {
        if (!hyp[(size_t)h].elig) continue;
        for (int g = h + 1; g < m; ++g) {
            if (!hyp[(size_t)g].elig || !pair_test(hyp[(size_t)h], hyp[(size_t)g], cos_min)) continue;
            if (++edges > kMaxRecords) return 1;
            const int a = root(h), b = root(g);
            if (a != b) comp[(size_t)(a < b ? b : a)] = a < b ? a : b;
        }
    }
    counts[2] = (int32_t)edges;
    for (size_t h = 0; h < M; ++h) comp[h] = root((int)h);
    // the representative: the largest A, at equal A the lowest index (ascending: the first that holds the maximum)
    std::vector<int32_t> rep(M, -1);
    for (size_t h = 0; h < M; ++h) {
        if (!hyp[h].elig) continue;
        int32_t& r = rep[(size_t)comp[h]];
        if (r < 0 || aux[h].A > aux[(size_t)r].A) r = (int32_t)h;
    }
    // the star rule; the staying hypotheses of every component, ascending
    std::vector<std::vector<int32_t>> stay(M);
    for (size_t h = 0; h < M; ++h) {
        if (!hyp[h].elig) continue;
        const int c = comp[h], r = rep[(size_t)c];
        if ((int)h == r || pair_test(hyp[h], hyp[(size_t)r], cos_min)) stay[(size_t)c].push_back((int32_t)h);
        else ++counts[4];
    }
    // the candidates in the order of their lowest staying hypotheses
    std::vector<std::pair<int32_t, int32_t>> cand;                     // (lowest staying hypothesis, component)
    for (size_t c = 0; c < M; ++c) if (!stay[c].empty()) cand.push_back({ stay[c][0], (int32_t)c });
    std::sort(cand.begin(), cand.end());
    counts[3] = (int32_t)cand.size();
    std::vector<unsigned char> seed(N);
    for (const auto& lc : cand) {
        const std::vector<int32_t>& s = stay[(size_t)lc.second];
        const int r = rep[(size_t)lc.second];
        l3d_plane o = {};
        const bool ok = parameters(hyp.data(), aux.data(), s.data(), (int)s.size(), r, tab[(size_t)hyp[(size_t)r].li].d, o);
        int nl = 0;
        if (ok) {
            std::fill(seed.begin(), seed.end(), 0);
            for (int32_t h : s) { seed[(size_t)hyp[(size_t)h].li] = 1; seed[(size_t)hyp[(size_t)h].lj] = 1; }
            for (size_t k = 0; k < N; ++k) nl += (tab[k].elig && lies_in(tab[k].P, tab[k].Q, tab[k].tol, o.N, o.c)) ? 1 : 0;
        }
        if (!ok || nl < min_lines) { ++counts[5]; continue; }
        if ((long long)members.size() + nl > kMaxRecords) return 2;
        bool first = true;
        for (size_t k = 0; k < N; ++k) {
            if (!tab[k].elig || !lies_in(tab[k].P, tab[k].Q, tab[k].tol, o.N, o.c)) continue;
            l3d_plane_member r2;
            r2.plane = (int32_t)planes.size(); r2.line = (int32_t)k; r2.flags = seed[k] ? kSeed : 0; r2.pad = 0;
            members.push_back(r2);
            extend(o, tab[k].P, first, o.rect);
            extend(o, tab[k].Q, false, o.rect);
            first = false;
        }
        o.rep = r; o.first_hyp = s[0]; o.n_hyp = (int32_t)s.size(); o.n_lines = nl;
        for (int32_t h : s) hyp_plane[h] = (int32_t)planes.size();
        planes.push_back(o);
    }
    counts[6] = (int32_t)planes.size();
    counts[7] = (int32_t)members.size();
    return 0;
}

}  // namespace plane
}  // namespace l3d
