// The host side of the grouping of duplicate 3-D lines (line3d_amd/csrc/l3d_merge.hpp: the argument checks, the table, the pair test, the components,
// the star rule, the counts) as a program of its own, for AddressSanitizer and UBSan:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/merge_asan.cpp -o merge_asan
//     ./merge_asan
// The sizes of the case tables (wave and tile ends), every refusal, the decision points built from exactly representable numbers, and lines that are
// not eligible; the arrays are allocated to the element, so a read or write past one is an error the sanitizer reports.  Exit status 0 and "0 bad"
// on its last line: nothing was reported and every invariant held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../line3d_amd/csrc/l3d_merge.hpp"

using namespace l3d;

static int run(const std::vector<double>& lines, const std::vector<double>& tol, double cos_min, double max_gap, std::vector<int32_t>& group,
               std::vector<int32_t>& pairs, int32_t* counts)
{
    const int n = (int)tol.size();
    group.assign((size_t)n, -7);
    pairs.clear();
    return merge::run_host(lines.data(), tol.data(), n, cos_min, max_gap, group.data(), pairs, counts) ? 0 : 1;
}

int main()
{
    std::mt19937_64 rng(4711);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double cos5 = std::cos(5.0 * M_PI / 180.0);
    int bad = 0, runs = 0, refusals = 0;
    std::vector<int32_t> group, pairs;
    int32_t counts[4];

    // ---- the sizes: near-copies of n / 4 base lines, with lines that are not eligible in between
    for (int n : { 0, 1, 2, 63, 64, 65, 255, 256, 257, 513 }) {
        const int m = n / 4 > 0 ? n / 4 : 1;
        std::vector<double> base((size_t)m * 6), lines((size_t)n * 6), tol((size_t)n, 0.05);
        for (auto& v : base) v = U(rng) * 5.0;
        for (int k = 0; k < n; ++k) for (int c = 0; c < 6; ++c) lines[(size_t)k * 6 + c] = base[(size_t)(k % m) * 6 + c] + U(rng) * 0.01;
        if (n > 70) { lines[6 * 40 + 1] = nan; lines[6 * 41 + 5] = inf; for (int c = 0; c < 3; ++c) lines[6 * 42 + 3 + c] = lines[6 * 42 + c]; lines[6 * 43] = 1e300; lines[6 * 43 + 3] = -1e300; }
        bad += run(lines, tol, cos5, 0.0, group, pairs, counts);
        ++runs;
        const size_t np = pairs.size() / 2;
        for (size_t k = 0; k < np; ++k) {
            bad += !(0 <= pairs[2 * k] && pairs[2 * k] < pairs[2 * k + 1] && pairs[2 * k + 1] < n);
            if (k) bad += !(pairs[2 * k - 2] < pairs[2 * k] || (pairs[2 * k - 2] == pairs[2 * k] && pairs[2 * k - 1] < pairs[2 * k + 1]));
        }
        for (int k = 0; k < n; ++k) bad += !(0 <= group[(size_t)k] && group[(size_t)k] <= k && group[(size_t)group[(size_t)k]] == group[(size_t)k]);
        if (n > 70) { bad += counts[0] != n - 4; for (int k = 40; k < 44; ++k) bad += group[(size_t)k] != k; }
        else bad += counts[0] != n;
        if (n >= 8) bad += !(np > 0 && counts[1] > 0 && counts[3] > 0);
    }

    // ---- the decision points (a: (0,0,0)-(4,0,0))
    struct D { double b[6]; double tol_a, tol_b, cos_min, max_gap; int expect; };
    const double h = 0.5, h1 = std::nextafter(0.5, 1.0), c45 = 4.0 / 5.0;
    const D points[] = {
        { { 1, h, 0, 3, h, 0 }, 0.5, 0.5, cos5, 0, 1 },  { { 1, h1, 0, 3, h, 0 }, 0.5, 0.5, cos5, 0, 0 },
        { { 1, h, 0, 3, h, 0 }, 0.5, 0.0, cos5, 0, 1 },  { { 1, h, 0, 3, h, 0 }, 0.0, 0.5, cos5, 0, 1 },  { { 1, h, 0, 3, h, 0 }, 0.25, 0.25, cos5, 0, 0 },
        { { 0, 0, 0, 1.6, 1.2, 0 }, 10, 10, c45, 0, -1 }, { { 3, 0, 0, 1, 0, 0 }, 0, 0, cos5, 0, 1 },
        { { 4, 0, 0, 6, 0, 0 }, 0, 0, cos5, 0, 1 },      { { std::nextafter(4.0, 5.0), 0, 0, 6, 0, 0 }, 0, 0, cos5, 0, 0 },
        { { 5, 0, 0, 7, 0, 0 }, 0, 0, cos5, 0.5, 1 },    { { std::nextafter(5.0, 6.0), 0, 0, 7, 0, 0 }, 0, 0, cos5, 0.5, 0 },
        { { 0, 0, 0, 4, 0, 0 }, 0, 0, 1.0, 0, 1 },
    };
    for (const D& p : points) {
        std::vector<double> lines = { 0, 0, 0, 4, 0, 0 };
        lines.insert(lines.end(), p.b, p.b + 6);
        bad += run(lines, { p.tol_a, p.tol_b }, p.cos_min, p.max_gap, group, pairs, counts);
        ++runs;
        if (p.expect >= 0) bad += (int)(pairs.size() / 2) != p.expect;
        bad += !(counts[0] == 2 && counts[3] == (int)(pairs.size() / 2));
    }
    // 3-4-5: |dot| == cos_min passes, the next number above fails
    {
        std::vector<double> lines = { 0, 0, 0, 10, 0, 0, 0, 0, 0, 4, 3, 0 };
        bad += run(lines, { 10, 10 }, c45, 0.0, group, pairs, counts) || pairs.size() != 2;
        bad += run(lines, { 10, 10 }, std::nextafter(c45, 1.0), 0.0, group, pairs, counts) || pairs.size() != 0;
        runs += 2;
    }
    // a chain A ~ B ~ C with A unlike C: C is released
    {
        auto ang = [](double deg, double L) { return std::vector<double>{ 0, 0, 0, L * std::cos(deg * M_PI / 180.0), L * std::sin(deg * M_PI / 180.0), 0 }; };
        std::vector<double> lines;
        for (auto v : { ang(0, 10), ang(4, 5), ang(8, 4) }) lines.insert(lines.end(), v.begin(), v.end());
        bad += run(lines, { 10, 10, 10 }, cos5, 0.0, group, pairs, counts);
        bad += !(pairs.size() == 4 && group[0] == 0 && group[1] == 0 && group[2] == 2 && counts[1] == 1 && counts[2] == 1 && counts[3] == 1);
        ++runs;
    }

    // ---- the chunks of the device search: at least 1, at most one per tile and 64, 1 from 512 row blocks on, n x chunks below 2^30
    for (int n : { 0, 1, 256, 257, 513, 8209, 100000, 131072, 131073, 20000000, 2147483647 }) {
        const long long tiles = ((long long)n + 255) / 256, c = merge::chunks(n);
        bad += !(c >= 1 && c <= 64 && (c <= tiles || tiles == 0) && (tiles < 512 || c == 1) && (long long)n * c <= (1ll << 30) + (c == 1 ? (1ll << 31) : 0));
        ++runs;
    }
    bad += !(merge::chunks(257) == 2 && merge::chunks(513) == 3 && merge::chunks(8209) == 32 && merge::chunks(100000) == 3);

    // ---- the refusals
    {
        const double lines[12] = { 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0 };
        double tol[2] = { 0.1, 0.1 };
        int32_t g[2]; int32_t* pr = nullptr; int np = 0;
        std::string msg;
        l3d_merge_params ok = { 0.9, 0.0 };
        bad += merge::check_arguments(lines, tol, 2, &ok, g, &pr, &np, counts, msg) != L3D_OK;
        bad += merge::check_arguments(nullptr, nullptr, 0, &ok, nullptr, &pr, &np, counts, msg) != L3D_OK;
        auto refused = [&](const double* l, const double* t, int n, const l3d_merge_params* p, int32_t* gg, int32_t** pp, int* nn, int32_t* cc) {
            ++refusals;
            msg.clear();
            return merge::check_arguments(l, t, n, p, gg, pp, nn, cc, msg) == L3D_ERR_INVALID && !msg.empty() ? 0 : 1;
        };
        bad += refused(lines, tol, -1, &ok, g, &pr, &np, counts);
        bad += refused(nullptr, tol, 2, &ok, g, &pr, &np, counts);
        bad += refused(lines, nullptr, 2, &ok, g, &pr, &np, counts);
        bad += refused(lines, tol, 2, &ok, nullptr, &pr, &np, counts);
        bad += refused(lines, tol, 2, nullptr, g, &pr, &np, counts);
        bad += refused(lines, tol, 2, &ok, g, nullptr, &np, counts);
        bad += refused(lines, tol, 2, &ok, g, &pr, nullptr, counts);
        bad += refused(lines, tol, 2, &ok, g, &pr, &np, nullptr);
        for (double cm : { -0.1, 1.5, nan, inf }) { l3d_merge_params p = { cm, 0.0 }; bad += refused(lines, tol, 2, &p, g, &pr, &np, counts); }
        for (double mg : { -1.0, nan, inf }) { l3d_merge_params p = { 0.9, mg }; bad += refused(lines, tol, 2, &p, g, &pr, &np, counts); }
        for (double t : { -0.1, nan }) { tol[1] = t; bad += refused(lines, tol, 2, &ok, g, &pr, &np, counts); }
    }
    printf("merge: %d runs, %d refusals, %d bad\n", runs, refusals, bad);
    return bad ? 1 : 0;
}
