// The host side of the planes of 3-D lines (line3d_amd/csrc/l3d_plane.hpp: the argument checks, the line table, the hypotheses, the pair test, the
// components, the star rule, the parameters, the members, the extents, the counts) as a program of its own, for AddressSanitizer and UBSan:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/plane_asan.cpp -o plane_asan
//     ./plane_asan
// Random boxes at the sizes of the case tables (wave and tile ends of lines and seeds), a cube with exactly representable corners, lines and seeds that
// are not eligible, and every refusal; the arrays are allocated to the element, so a read or write past one is an error the sanitizer reports.  Exit
// status 0 and "0 bad" on its last line: nothing was reported and every invariant held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../line3d_amd/csrc/l3d_plane.hpp"

using namespace l3d;

struct Out {
    std::vector<l3d_plane> planes;
    std::vector<l3d_plane_member> members;
    std::vector<int32_t> hp;
    int32_t counts[8];
};

static int run(const std::vector<double>& lines, const std::vector<double>& tol, const std::vector<int32_t>& seeds, double cos_max, double cos_min, int min_lines, Out& o)
{
    const int n = (int)tol.size(), m = (int)(seeds.size() / 2);
    o.planes.clear(); o.members.clear();
    o.hp.assign((size_t)m, -7);
    return plane::run_host(lines.data(), tol.data(), n, seeds.data(), m, cos_max, cos_min, min_lines, o.planes, o.members, o.hp.data(), o.counts);
}

// what holds for every result
static int invariants(int n, int m, int min_lines, const Out& o)
{
    int bad = 0;
    const int np = (int)o.planes.size();
    bad += o.counts[6] != np;
    bad += o.counts[7] != (int)o.members.size();
    bad += o.counts[3] - o.counts[5] != np;
    bad += !(o.counts[0] <= n && o.counts[1] <= m && o.counts[4] <= o.counts[1]);
    std::vector<int> nl((size_t)np, 0), nh((size_t)np, 0);
    for (size_t k = 0; k < o.members.size(); ++k) {
        const l3d_plane_member& r = o.members[k];
        bad += !(0 <= r.plane && r.plane < np && 0 <= r.line && r.line < n && (r.flags & ~1) == 0 && r.pad == 0);
        if (k) bad += !(o.members[k - 1].plane < r.plane || (o.members[k - 1].plane == r.plane && o.members[k - 1].line < r.line));
        if (0 <= r.plane && r.plane < np) ++nl[(size_t)r.plane];
    }
    for (int h = 0; h < m; ++h) {
        bad += !(-1 <= o.hp[(size_t)h] && o.hp[(size_t)h] < np);
        if (o.hp[(size_t)h] >= 0) { if (!nh[(size_t)o.hp[(size_t)h]]) bad += o.planes[(size_t)o.hp[(size_t)h]].first_hyp != h; ++nh[(size_t)o.hp[(size_t)h]]; }
    }
    for (int k = 0; k < np; ++k) {
        const l3d_plane& p = o.planes[(size_t)k];
        bad += !(nl[(size_t)k] == p.n_lines && p.n_lines >= min_lines && nh[(size_t)k] == p.n_hyp && p.n_hyp >= 1);
        bad += !(0 <= p.rep && p.rep < m && o.hp[(size_t)p.rep] == k);
        bad += !(std::fabs(plane::dot3(p.N, p.N) - 1.0) < 1e-12 && std::fabs(plane::dot3(p.u, p.u) - 1.0) < 1e-12 && std::fabs(plane::dot3(p.N, p.u)) < 1e-9);
        bad += !(p.rect[0] <= p.rect[1] && p.rect[2] <= p.rect[3]);
        if (k) bad += !(o.planes[(size_t)k - 1].first_hyp < p.first_hyp);
    }
    return bad;
}

// nb boxes with random frames: 12 edges each, a little beside and short of their corners; the 24 corner pairs of every box as seeds, cut to m
static void boxes(int n, int m, unsigned seed, std::vector<double>& lines, std::vector<double>& tol, std::vector<int32_t>& seeds)
{
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const int nb = (n + 11) / 12;
    lines.clear(); tol.clear(); seeds.clear();
    for (int b = 0; b < nb; ++b) {
        double c[3], R[3][3], h[3];
        for (int k = 0; k < 3; ++k) { c[k] = 5.0 * U(rng); h[k] = 1.0 + 0.5 * U(rng); }
        // a frame: Gram-Schmidt of two random vectors
        double a[3] = { U(rng), U(rng), U(rng) + 2.0 }, q[3] = { U(rng) + 2.0, U(rng), U(rng) };
        const double la = std::sqrt(plane::dot3(a, a));
        for (int k = 0; k < 3; ++k) a[k] /= la;
        const double aq = plane::dot3(a, q);
        for (int k = 0; k < 3; ++k) q[k] -= aq * a[k];
        const double lq = std::sqrt(plane::dot3(q, q));
        for (int k = 0; k < 3; ++k) q[k] /= lq;
        double w[3];
        plane::cross3(a, q, w);
        for (int k = 0; k < 3; ++k) { R[k][0] = a[k]; R[k][1] = q[k]; R[k][2] = w[k]; }
        for (int ax = 0; ax < 3; ++ax) {
            const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2;
            for (int s1 = -1; s1 <= 1; s1 += 2)
                for (int s2 = -1; s2 <= 1; s2 += 2) {
                    double P[3], Q[3];
                    for (int k = 0; k < 3; ++k) {
                        const double mid = c[k] + R[k][o0] * (s1 * h[o0]) + R[k][o1] * (s2 * h[o1]);
                        P[k] = mid - R[k][ax] * (h[ax] - 0.03 * U(rng)) + 0.003 * U(rng);
                        Q[k] = mid + R[k][ax] * (h[ax] - 0.03 * U(rng)) + 0.003 * U(rng);
                    }
                    for (int k = 0; k < 3; ++k) lines.push_back(P[k]);
                    for (int k = 0; k < 3; ++k) lines.push_back(Q[k]);
                    tol.push_back(0.03);
                }
        }
    }
    lines.resize(6 * (size_t)n); tol.resize((size_t)n);
    // corner (s0, s1, s2): its edge along axis ax sits at the signs of the two other axes
    std::vector<int32_t> all;
    for (int cs = 0; cs < 8; ++cs) {
        const int s[3] = { cs & 1, (cs >> 1) & 1, (cs >> 2) & 1 };
        int e[3];
        for (int ax = 0; ax < 3; ++ax) { const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2; e[ax] = 4 * ax + 2 * s[o0] + s[o1]; }
        const int pr[3][2] = { { 0, 1 }, { 0, 2 }, { 1, 2 } };
        for (int p = 0; p < 3; ++p)
            for (int b = 0; b < nb; ++b) { all.push_back(12 * b + e[pr[p][0]]); all.push_back(12 * b + e[pr[p][1]]); }
    }
    std::vector<int32_t> ok;
    for (size_t k = 0; k + 1 < all.size(); k += 2) if (all[k] < n && all[k + 1] < n) { ok.push_back(all[k]); ok.push_back(all[k + 1]); }
    for (int k = 0; k < m && !ok.empty(); ++k) { seeds.push_back(ok[(2 * (size_t)k) % ok.size()]); seeds.push_back(ok[(2 * (size_t)k + 1) % ok.size()]); }
}

int main()
{
    int bad = 0, checks = 0;
    const double cos10 = std::cos(10.0 * 3.14159265358979323846 / 180.0);
    Out o;
    std::vector<double> lines, tol;
    std::vector<int32_t> seeds;
    const int sizes[][2] = { { 12, 1 }, { 64, 63 }, { 65, 64 }, { 256, 255 }, { 257, 256 }, { 300, 257 }, { 300, 513 }, { 600, 1200 } };
    for (const auto& s : sizes) {
        boxes(s[0], s[1], 100u + (unsigned)s[1], lines, tol, seeds);
        bad += run(lines, tol, seeds, cos10, cos10, 3, o) != 0;
        bad += invariants(s[0], (int)(seeds.size() / 2), 3, o);
        bad += o.counts[0] != s[0] || o.counts[6] < 1;
        bad += plane::chunks(s[1]) < 1 || plane::chunks(s[1]) > 64;
        ++checks;
    }
    // a cube with corners at +-2: six planes of four lines, every line in two, 36 edges
    {
        lines.clear(); tol.assign(12, 0.0); seeds.clear();
        for (int ax = 0; ax < 3; ++ax) {
            const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2;
            for (int s1 = -1; s1 <= 1; s1 += 2)
                for (int s2 = -1; s2 <= 1; s2 += 2) {
                    double P[3], Q[3];
                    P[ax] = -2.0; Q[ax] = 2.0; P[o0] = Q[o0] = 2.0 * s1; P[o1] = Q[o1] = 2.0 * s2;
                    for (int k = 0; k < 3; ++k) lines.push_back(P[k]);
                    for (int k = 0; k < 3; ++k) lines.push_back(Q[k]);
                }
        }
        for (int cs = 0; cs < 8; ++cs) {
            const int s[3] = { cs & 1, (cs >> 1) & 1, (cs >> 2) & 1 };
            int e[3];
            for (int ax = 0; ax < 3; ++ax) { const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2; e[ax] = 4 * ax + 2 * s[o0] + s[o1]; }
            const int pr[3][2] = { { 0, 1 }, { 0, 2 }, { 1, 2 } };
            for (int p = 0; p < 3; ++p) { seeds.push_back(e[pr[p][0]]); seeds.push_back(e[pr[p][1]]); }
        }
        bad += run(lines, tol, seeds, cos10, cos10, 3, o) != 0;
        bad += invariants(12, 24, 3, o);
        const int32_t want[8] = { 12, 24, 36, 6, 0, 0, 6, 24 };
        for (int k = 0; k < 8; ++k) bad += o.counts[k] != want[k];
        std::vector<int> per(12, 0);
        for (const l3d_plane_member& r : o.members) { ++per[(size_t)r.line]; bad += r.flags != 1; }
        for (int k = 0; k < 12; ++k) bad += per[(size_t)k] != 2;
        ++checks;
        // lines and seeds that are not eligible: no length, a NaN, an infinite tolerance, a line paired with itself
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        for (int k = 0; k < 3; ++k) lines[6 * 3 + 3 + k] = lines[6 * 3 + k];
        lines[6 * 5] = nan;
        tol[7] = inf;
        seeds.push_back(2); seeds.push_back(2);
        bad += run(lines, tol, seeds, cos10, cos10, 3, o) != 0;
        bad += invariants(12, 25, 3, o);
        bad += o.counts[0] != 9 || o.hp[24] != -1;
        for (const l3d_plane_member& r : o.members) bad += r.line == 3 || r.line == 5 || r.line == 7;
        ++checks;
        // min_lines above what any plane has: every candidate is dropped
        bad += run(lines, tol, seeds, cos10, cos10, 13, o) != 0;
        bad += !(o.planes.empty() && o.members.empty() && o.counts[5] == o.counts[3] && o.counts[3] > 0);
        for (int32_t h : o.hp) bad += h != -1;
        ++checks;
    }
    // empty tables
    {
        std::vector<double> none;
        std::vector<int32_t> nos;
        bad += run(none, none, nos, cos10, cos10, 3, o) != 0 || !o.planes.empty();
        for (int k = 0; k < 8; ++k) bad += o.counts[k] != 0;
        ++checks;
    }
    // the refusals
    {
        boxes(12, 24, 5u, lines, tol, seeds);
        l3d_plane_params prm = { cos10, cos10, 3, 0 };
        l3d_plane* pl = nullptr; l3d_plane_member* mem = nullptr; int npl = 0, nm = 0;
        std::vector<int32_t> hp(24);
        int32_t counts[8];
        std::string err;
        auto chk = [&](const double* l, const double* t, int n, const int32_t* s, int m, const l3d_plane_params* p, l3d_plane** a, int* na, l3d_plane_member** b2, int* nb2, int32_t* h,
                       int32_t* c, int want) {
            err.clear();
            const int rc = plane::check_arguments(l, t, n, s, m, p, a, na, b2, nb2, h, c, err);
            bad += rc != want || (want != L3D_OK && err.empty());
            ++checks;
        };
        const double* L = lines.data(); const double* T = tol.data(); const int32_t* S = seeds.data();
        chk(L, T, 12, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_OK);
        chk(L, T, 12, S, 24, &prm, nullptr, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, 12, S, 24, &prm, &pl, nullptr, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, 12, S, 24, &prm, &pl, &npl, nullptr, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, 12, S, 24, &prm, &pl, &npl, &mem, nullptr, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, 12, S, 24, &prm, &pl, &npl, &mem, &nm, nullptr, counts, L3D_ERR_INVALID);
        chk(L, T, 12, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), nullptr, L3D_ERR_INVALID);
        chk(nullptr, T, 12, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, nullptr, 12, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, 12, nullptr, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, 12, S, 24, nullptr, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, -1, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(L, T, 12, S, -1, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        chk(nullptr, nullptr, plane::kMaxItems + 1, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_UNSUPPORTED);
        chk(L, T, 12, nullptr, plane::kMaxItems + 1, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_UNSUPPORTED);
        chk(L, T, 11, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);            // a seed names line 11
        const double bad_cos[] = { -0.1, 1.0, std::numeric_limits<double>::quiet_NaN() };
        for (double x : bad_cos) { l3d_plane_params p = prm; p.cos_max = x; chk(L, T, 12, S, 24, &p, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID); }
        const double bad_min[] = { 0.0, 1.5, std::numeric_limits<double>::quiet_NaN() };
        for (double x : bad_min) { l3d_plane_params p = prm; p.cos_min = x; chk(L, T, 12, S, 24, &p, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID); }
        { l3d_plane_params p = prm; p.min_lines = 1; chk(L, T, 12, S, 24, &p, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID); }
        std::vector<double> t2 = tol;
        t2[4] = -1e-300;
        chk(L, t2.data(), 12, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        t2[4] = std::numeric_limits<double>::quiet_NaN();
        chk(L, t2.data(), 12, S, 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
        std::vector<int32_t> s2 = seeds;
        s2[5] = -1;
        chk(L, T, 12, s2.data(), 24, &prm, &pl, &npl, &mem, &nm, hp.data(), counts, L3D_ERR_INVALID);
    }
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
