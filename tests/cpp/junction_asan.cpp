// The host side of the junctions of 3-D lines (line3d_amd/csrc/l3d_junction.hpp: the argument checks, the table, the pair test, the components, the
// star rule, the vertices, the attachments, the counts) as a program of its own, for AddressSanitizer and UBSan:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/junction_asan.cpp -o junction_asan
//     ./junction_asan
// The sizes of the case tables (wave and tile ends), every refusal, the decision points built from exactly representable numbers, and lines that are
// not eligible; the arrays are allocated to the element, so a read or write past one is an error the sanitizer reports.  Exit status 0 and "0 bad"
// on its last line: nothing was reported and every invariant held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../line3d_amd/csrc/l3d_junction.hpp"

using namespace l3d;

struct Out {
    std::vector<l3d_junction_record> rec;
    std::vector<l3d_junction_vertex> vert;
    std::vector<int32_t> nv, na;
    int32_t counts[8];
};

static int run(const std::vector<double>& lines, const std::vector<double>& tol, const std::vector<double>& ext, double cos_max, int crossings, Out& o)
{
    const int n = (int)tol.size();
    o.rec.clear(); o.vert.clear();
    o.nv.assign(2 * (size_t)n, -7); o.na.assign(2 * (size_t)n, -7);
    return junction::run_host(lines.data(), tol.data(), ext.data(), n, cos_max, crossings, o.rec, o.nv.data(), o.vert, o.na.data(), o.counts) ? 0 : 1;
}

// what holds for every result
static int invariants(int n, const Out& o)
{
    int bad = 0;
    const size_t np = o.rec.size();
    for (size_t k = 0; k < np; ++k) {
        const l3d_junction_record& r = o.rec[k];
        bad += !(0 <= r.i && r.i < r.j && r.j < n && 0 <= r.where_i && r.where_i <= 2 && 0 <= r.where_j && r.where_j <= 2 && r.gap >= 0.0);
        if (k) bad += !(o.rec[k - 1].i < r.i || (o.rec[k - 1].i == r.i && o.rec[k - 1].j < r.j));
    }
    bad += o.counts[1] + o.counts[2] + o.counts[3] != (int)np;
    bad += o.counts[5] != (int)o.vert.size();
    std::vector<int> deg(o.vert.size(), 0);
    for (int v = 0; v < 2 * n; ++v) {
        bad += !(-1 <= o.nv[(size_t)v] && o.nv[(size_t)v] < (int)o.vert.size());
        bad += !(-1 <= o.na[(size_t)v] && o.na[(size_t)v] < (int)np);
        bad += o.nv[(size_t)v] >= 0 && o.na[(size_t)v] >= 0;
        if (o.nv[(size_t)v] >= 0) { if (!deg[(size_t)o.nv[(size_t)v]]) bad += o.vert[(size_t)o.nv[(size_t)v]].first_node != v; ++deg[(size_t)o.nv[(size_t)v]]; }
        if (o.na[(size_t)v] >= 0) bad += !(junction::kind_of(o.rec[(size_t)o.na[(size_t)v]]) == junction::kKindT && junction::t_end_node(o.rec[(size_t)o.na[(size_t)v]]) == v);
    }
    for (size_t k = 0; k < o.vert.size(); ++k) {
        bad += !(deg[k] == o.vert[k].degree && deg[k] >= 2);
        if (k) bad += !(o.vert[k - 1].first_node < o.vert[k].first_node);
    }
    return bad;
}

int main()
{
    std::mt19937_64 rng(4711);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double cos10 = std::cos(10.0 * M_PI / 180.0);
    int bad = 0, runs = 0, refusals = 0;
    Out o;

    // ---- the sizes: three edges per corner along the coordinate axes, the edges of one corner n / 3 apart, with lines that are not eligible in between
    for (int n : { 0, 1, 2, 63, 64, 65, 255, 256, 257, 513 }) {
        const int m = n / 3 > 0 ? n / 3 : 1;
        std::vector<double> corner((size_t)m * 3), lines((size_t)n * 6), tol((size_t)n, 0.05), ext((size_t)n, 0.1);
        for (auto& v : corner) v = U(rng) * 5.0;
        for (int k = 0; k < n; ++k) {
            const int a = (k / m) % 3;
            for (int c = 0; c < 3; ++c) {
                const double p = corner[(size_t)(k % m) * 3 + c] + U(rng) * 0.005 + (c == a ? 0.03 * U(rng) : 0.0);
                lines[(size_t)k * 6 + c] = p;
                lines[(size_t)k * 6 + 3 + c] = p + (c == a ? 1.0 + (k % 5) * 0.5 : 0.0);
            }
        }
        if (n > 70) {
            lines[6 * 40 + 1] = nan; lines[6 * 41 + 5] = inf; for (int c = 0; c < 3; ++c) lines[6 * 42 + 3 + c] = lines[6 * 42 + c];
            lines[6 * 43] = 1e300; lines[6 * 43 + 3] = -1e300; tol[44] = inf; ext[45] = inf;
        }
        for (int crossings : { 0, 1 }) {
            bad += run(lines, tol, ext, cos10, crossings, o);
            ++runs;
            bad += invariants(n, o);
            if (n > 70) { bad += o.counts[0] != n - 6; for (int k = 40; k < 46; ++k) bad += !(o.nv[2 * (size_t)k] == -1 && o.nv[2 * (size_t)k + 1] == -1); }
            else bad += o.counts[0] != n;
            if (n >= 8) bad += !(o.counts[1] > 0 && o.counts[4] > 0 && o.counts[5] > 0);
        }
    }

    // ---- the decision points: the probe (0,0,0)-(4,0,0) and a line from (x0, 0, h) along y
    struct D { double x0, h, ext_probe, tol; int records, where; };
    const double h = 0.5;
    const D points[] = {
        { -0.5, 0, h, 0.05, 1, 0 }, { std::nextafter(-0.5, -1.0), 0, h, 0.05, 0, 0 }, { 0.5, 0, h, 0.05, 1, 0 }, { std::nextafter(0.5, 1.0), 0, h, 0.05, 1, 2 },
        { 2.0, 0, h, 0.05, 1, 2 }, { std::nextafter(2.0, 3.0), 0, h, 0.05, 1, 2 }, { 3.5, 0, h, 0.05, 1, 1 }, { std::nextafter(3.5, 0.0), 0, h, 0.05, 1, 2 },
        { 4.5, 0, h, 0.05, 1, 1 }, { std::nextafter(4.5, 5.0), 0, h, 0.05, 0, 0 }, { 2.0, 0, 2.5, 0.05, 1, 0 }, { std::nextafter(2.0, 3.0), 0, 2.5, 0.05, 1, 1 },
        { 2.0, 0.5, h, 0.5, 1, 2 }, { 2.0, std::nextafter(0.5, 1.0), h, 0.5, 0, 0 },
    };
    for (const D& p : points) {
        for (int probe_first : { 1, 0 }) {
            const std::vector<double> probe = { 0, 0, 0, 4, 0, 0 }, other = { p.x0, 0, p.h, p.x0, 3, p.h };
            std::vector<double> lines = probe_first ? probe : other;
            lines.insert(lines.end(), probe_first ? other.begin() : probe.begin(), probe_first ? other.end() : probe.end());
            const std::vector<double> ext = probe_first ? std::vector<double>{ p.ext_probe, 0.5 } : std::vector<double>{ 0.5, p.ext_probe };
            bad += run(lines, { p.tol, p.tol }, ext, cos10, 1, o);
            ++runs;
            bad += invariants(2, o);
            bad += (int)o.rec.size() != p.records;
            if (p.records == 1 && o.rec.size() == 1) {
                bad += (probe_first ? o.rec[0].where_i : o.rec[0].where_j) != p.where;
                bad += (probe_first ? o.rec[0].s : o.rec[0].t) != p.x0;
                bad += o.rec[0].gap != p.h;
            }
        }
    }
    // 3-4-5: |b| == cos_max passes, the next number below fails
    {
        const double c45 = 4.0 / 5.0;
        std::vector<double> lines = { 0, 0, 0, 10, 0, 0, 0, 0, 0, 4, 3, 0 };
        bad += run(lines, { 0.05, 0.05 }, { 0.1, 0.1 }, c45, 0, o) || o.rec.size() != 1 || o.vert.size() != 1;
        bad += run(lines, { 0.05, 0.05 }, { 0.1, 0.1 }, std::nextafter(c45, 0.0), 0, o) || o.rec.size() != 0 || o.vert.size() != 0;
        runs += 2;
    }
    // a row of five P ends 0.08 apart: one component, the representative (the long line 0) keeps only its neighbour
    {
        std::vector<double> lines;
        for (int k = 0; k < 5; ++k) {
            const double L = k == 0 ? 3.0 : 1.0, a = 20.0 * k * M_PI / 180.0;
            for (double v : { 0.08 * k, 0.0, 0.0, 0.08 * k, L * std::cos(a), L * std::sin(a) }) lines.push_back(v);
        }
        bad += run(lines, std::vector<double>(5, 0.1), std::vector<double>(5, 0.05), cos10, 0, o);
        bad += invariants(5, o);
        bad += !(o.rec.size() == 4 && o.counts[4] == 1 && o.counts[5] == 1 && o.counts[6] == 3 && o.nv[0] == 0 && o.nv[2] == 0 && o.nv[4] == -1 && o.nv[8] == -1);
        ++runs;
    }
    // an end on the inside of two lines: the T record with the smaller gap, at equal gaps the lower record
    {
        std::vector<double> lines = { 0, 0, 0, 4, 0, 0, 2, 0, -2, 2, 0, 2, 2, 0.01, 0, 2, 3, 0 };
        bad += run(lines, std::vector<double>(3, 0.05), std::vector<double>(3, 0.1), cos10, 0, o) || o.na[4] != 0 || o.counts[7] != 1;
        lines[14] = lines[17] = 0.001;
        bad += run(lines, std::vector<double>(3, 0.05), std::vector<double>(3, 0.1), cos10, 0, o) || o.na[4] != 1 || o.counts[7] != 1;
        bad += invariants(3, o);
        runs += 2;
    }

    // ---- the chunks of the device search: at least 1, at most one per tile and 64, 1 from 512 row blocks on, n x chunks below 2^30
    for (int n : { 0, 1, 256, 257, 513, 8209, 100000, 131072, 131073, 20000000, 1 << 30 }) {
        const long long tiles = ((long long)n + 255) / 256, c = junction::chunks(n);
        bad += !(c >= 1 && c <= 64 && (c <= tiles || tiles == 0) && (tiles < 512 || c == 1) && ((long long)n * c <= (1ll << 30)));
        ++runs;
    }
    bad += !(junction::chunks(257) == 2 && junction::chunks(513) == 3 && junction::chunks(8209) == 32 && junction::chunks(100000) == 3);

    // ---- the refusals
    {
        const double lines[12] = { 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0 };
        double tol[2] = { 0.1, 0.1 }, ext[2] = { 0.1, 0.1 };
        int32_t nv[4], na[4], counts[8];
        l3d_junction_record* rec = nullptr; l3d_junction_vertex* vert = nullptr; int nr = 0, nvert = 0;
        std::string msg;
        l3d_junction_params ok = { 0.9, 0, 0 };
        bad += junction::check_arguments(lines, tol, ext, 2, &ok, &rec, &nr, nv, &vert, &nvert, na, counts, msg) != L3D_OK;
        bad += junction::check_arguments(nullptr, nullptr, nullptr, 0, &ok, &rec, &nr, nullptr, &vert, &nvert, nullptr, counts, msg) != L3D_OK;
        auto refused = [&](int code, const double* l, const double* t, const double* e, int n, const l3d_junction_params* p, l3d_junction_record** rr, int* nn, int32_t* v,
                           l3d_junction_vertex** vv, int* nvv, int32_t* a, int32_t* cc) {
            ++refusals;
            msg.clear();
            return junction::check_arguments(l, t, e, n, p, rr, nn, v, vv, nvv, a, cc, msg) == code && !msg.empty() ? 0 : 1;
        };
        const int I = L3D_ERR_INVALID;
        bad += refused(I, lines, tol, ext, -1, &ok, &rec, &nr, nv, &vert, &nvert, na, counts);
        bad += refused(L3D_ERR_UNSUPPORTED, lines, tol, ext, (1 << 30) + 1, &ok, &rec, &nr, nv, &vert, &nvert, na, counts);
        bad += refused(I, nullptr, tol, ext, 2, &ok, &rec, &nr, nv, &vert, &nvert, na, counts);
        bad += refused(I, lines, nullptr, ext, 2, &ok, &rec, &nr, nv, &vert, &nvert, na, counts);
        bad += refused(I, lines, tol, nullptr, 2, &ok, &rec, &nr, nv, &vert, &nvert, na, counts);
        bad += refused(I, lines, tol, ext, 2, nullptr, &rec, &nr, nv, &vert, &nvert, na, counts);
        bad += refused(I, lines, tol, ext, 2, &ok, nullptr, &nr, nv, &vert, &nvert, na, counts);
        bad += refused(I, lines, tol, ext, 2, &ok, &rec, nullptr, nv, &vert, &nvert, na, counts);
        bad += refused(I, lines, tol, ext, 2, &ok, &rec, &nr, nullptr, &vert, &nvert, na, counts);
        bad += refused(I, lines, tol, ext, 2, &ok, &rec, &nr, nv, nullptr, &nvert, na, counts);
        bad += refused(I, lines, tol, ext, 2, &ok, &rec, &nr, nv, &vert, nullptr, na, counts);
        bad += refused(I, lines, tol, ext, 2, &ok, &rec, &nr, nv, &vert, &nvert, nullptr, counts);
        bad += refused(I, lines, tol, ext, 2, &ok, &rec, &nr, nv, &vert, &nvert, na, nullptr);
        for (double cm : { -0.1, 1.0, 1.5, nan, inf }) { l3d_junction_params p = { cm, 0, 0 }; bad += refused(I, lines, tol, ext, 2, &p, &rec, &nr, nv, &vert, &nvert, na, counts); }
        for (double t : { -0.1, nan }) { tol[1] = t; bad += refused(I, lines, tol, ext, 2, &ok, &rec, &nr, nv, &vert, &nvert, na, counts); }
        tol[1] = 0.1;
        for (double e : { -0.1, nan }) { ext[0] = e; bad += refused(I, lines, tol, ext, 2, &ok, &rec, &nr, nv, &vert, &nvert, na, counts); }
    }
    printf("junction: %d runs, %d refusals, %d bad\n", runs, refusals, bad);
    return bad ? 1 : 0;
}
