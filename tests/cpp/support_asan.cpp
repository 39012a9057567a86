// The host side of the support search (line3d_amd/csrc/l3d_support.hpp: the argument checks, the rows, the column table, the pair test, the best rows,
// the counts, and the sizing rules of the device call) as a program of its own, for AddressSanitizer and UBSan:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/support_asan.cpp -o support_asan
//     ./support_asan
// The sizes of the case tables (wave and tile ends), cameras without segments and without rows, the decision points built from exactly representable
// numbers, columns that are not eligible, every refusal, and the cut of a chunk from 64-bit totals; the arrays are allocated to the element, so a read
// or write past one is an error the sanitizer reports.  Exit status 0 and "0 bad" on its last line: nothing was reported and every invariant held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../line3d_amd/csrc/l3d_support.hpp"

using namespace l3d;

static l3d_camera unit_camera(int w = 64, int h = 48)
{
    l3d_camera c{};
    c.K[0] = c.K[4] = c.K[8] = 1.0;
    c.R[0] = c.R[4] = c.R[8] = 1.0;
    c.width = w; c.height = h;
    return c;
}

struct Out { std::vector<l3d_support_record> rec; std::vector<int64_t> cam_start; std::vector<int32_t> best; int64_t counts[4]; };

static int run(const std::vector<double>& s3, const std::vector<l3d_camera>& cams, const std::vector<float>& s2, const std::vector<int64_t>& start,
               const l3d_support_params& p, Out& o)
{
    const int n = (int)(s3.size() / 6), m = (int)cams.size();
    o.rec.clear();
    o.cam_start.assign((size_t)m + 1, -7);
    o.best.assign((size_t)start[(size_t)m], -7);
    return support::run_host(s3.data(), n, cams.data(), m, s2.data(), start.data(), p, o.rec, o.cam_start.data(), o.best.data(), o.counts) ? 0 : 1;
}

// the invariants of any result
static int check(const Out& o, int n, const std::vector<int64_t>& start)
{
    int bad = 0;
    const int m = (int)start.size() - 1;
    bad += !(o.cam_start[0] == 0 && o.cam_start[(size_t)m] == (int64_t)o.rec.size() && o.counts[2] == (int64_t)o.rec.size());
    int64_t with_best = 0;
    for (int c = 0; c < m; ++c) {
        const int64_t nj = start[(size_t)c + 1] - start[(size_t)c];
        bad += !(o.cam_start[(size_t)c] <= o.cam_start[(size_t)c + 1]);
        std::vector<unsigned long long> key((size_t)nj, ~0ull);
        for (int64_t r = o.cam_start[(size_t)c]; r < o.cam_start[(size_t)c + 1]; ++r) {
            const l3d_support_record& x = o.rec[(size_t)r];
            bad += !(0 <= x.seg3d && x.seg3d < n && 0 <= x.seg2d && x.seg2d < nj && x.dist >= 0.0f && x.overlap <= 1.0f);
            if (r > o.cam_start[(size_t)c]) { const l3d_support_record& y = o.rec[(size_t)r - 1]; bad += !(y.seg3d < x.seg3d || (y.seg3d == x.seg3d && y.seg2d < x.seg2d)); }
            const unsigned long long k = support::best_key(x.dist, x.seg3d);
            if (k < key[(size_t)x.seg2d]) key[(size_t)x.seg2d] = k;
        }
        for (int64_t j = 0; j < nj; ++j) {
            const int32_t b = o.best[(size_t)(start[(size_t)c] + j)];
            bad += b != (key[(size_t)j] == ~0ull ? -1 : (int32_t)(key[(size_t)j] & 0xFFFFFFFFull));
            with_best += b >= 0;
        }
    }
    bad += o.counts[3] != with_best;
    return bad;
}

int main()
{
    std::mt19937_64 rng(4711);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
    const double cos5 = std::cos(5.0 * M_PI / 180.0);
    const l3d_support_params P0 = { 3.0, cos5, 0.5, 1e-3, 0.0 };
    int bad = 0, runs = 0, refusals = 0;
    Out o;

    // ---- the sizes: n segments in the plane z = 1 of three cameras (the second has no segments, the third looks away: no rows), k columns in the others
    for (int n : { 0, 1, 63, 64, 65, 257 })
        for (int k : { 0, 1, 255, 256, 257, 513 }) {
            if (n > 65 && k > 257) continue;
            std::vector<double> s3((size_t)n * 6);
            for (int i = 0; i < n; ++i) {
                const double x = U(rng) * 40.0, y = U(rng) * 40.0, a = U(rng) * 6.28;
                const double v[6] = { x, y, 1.0, x + 20.0 * std::cos(a), y + 20.0 * std::sin(a), 1.0 };
                for (int c = 0; c < 6; ++c) s3[(size_t)i * 6 + c] = v[c];
            }
            std::vector<l3d_camera> cams = { unit_camera(), unit_camera(), unit_camera() };
            cams[2].R[0] = -1.0; cams[2].R[8] = -1.0;                  // (a half turn about y)
            std::vector<int64_t> start = { 0, k, k, 2 * (int64_t)k };
            std::vector<float> s2((size_t)k * 8);
            for (int j = 0; j < 2 * k; ++j) {
                const int i = n ? (int)(U(rng) * n) % n : 0;
                const double a = 0.1 + 0.3 * U(rng), b = a + 0.4;
                for (int e = 0; e < 2; ++e) {
                    const double t = e ? b : a;
                    s2[(size_t)j * 4 + 2 * e] = n ? (float)(s3[(size_t)i * 6] + t * (s3[(size_t)i * 6 + 3] - s3[(size_t)i * 6]) + U(rng)) : 1.0f;
                    s2[(size_t)j * 4 + 2 * e + 1] = n ? (float)(s3[(size_t)i * 6 + 1] + t * (s3[(size_t)i * 6 + 4] - s3[(size_t)i * 6 + 1]) + U(rng)) : (float)e;
                }
            }
            if (k > 200) { s2[4 * 100] = fnan; s2[4 * 101 + 2] = finf; s2[4 * 102 + 2] = s2[4 * 102]; s2[4 * 102 + 3] = s2[4 * 102 + 1]; }
            if (n == 0) { o.rec.clear(); continue; }                  // (the entry points answer n == 0 themselves)
            bad += run(s3, cams, s2, start, P0, o);
            ++runs;
            bad += check(o, n, start);
            bad += !(o.cam_start[1] == o.cam_start[2] && o.cam_start[2] == o.cam_start[3]);      // no segments; no rows
            bad += o.counts[1] != 2 * k - (k > 200 ? 3 : 0);
            bad += !(o.counts[0] <= 2 * n && o.counts[0] % 2 == 0 && (n < 63 || o.counts[0] > 0));      // (the first two cameras are the same)
            if (n >= 63 && k >= 255) bad += o.rec.empty();
        }

    // ---- the decision points: the row (0, 0) -> (16, 0) of the unit camera against one column
    struct D { float col[4]; double dist_px, cos_min, min_overlap; int expect; float dist, overlap; };
    const double c35 = 3.0 / 5.0;
    const D points[] = {
        { { 2, 3, 10, 3 }, 3.0, cos5, 0.5, 1, 3.0f, 1.0f },            { { 2, 3, 10, 3 }, std::nextafter(3.0, 0.0), cos5, 0.5, 0, 0, 0 },
        { { 2, 1, 10, 3 }, std::nextafter(3.0, 0.0), 0.5, 0.5, 0, 0, 0 },
        { { 4, 0, 7, 4 }, 5.0, c35, 0.5, 1, 4.0f, 0.6f },              { { 4, 0, 7, 4 }, 5.0, std::nextafter(c35, 1.0), 0.5, 0, 0, 0 },
        { { 7, 4, 4, 0 }, 5.0, c35, 0.5, 1, 4.0f, 0.6f },
        { { 12, 1, 20, 1 }, 3.0, cos5, 0.5, 1, 1.0f, 0.5f },           { { 12, 1, 20, 1 }, 3.0, cos5, std::nextafter(0.5, 1.0), 0, 0, 0 },
        { { 2, 0, 10, 0 }, 0.0, cos5, 0.5, 1, 0.0f, 1.0f },            { { 2, 9.5367431640625e-07f, 10, 0 }, 0.0, cos5, 0.5, 0, 0, 0 },
        { { 16, 0, 20, 0 }, 3.0, cos5, 0.0, 1, 0.0f, 0.0f },           { { 18, 0, 22, 0 }, 3.0, cos5, 0.0, 0, 0, 0 },
        { { 8, -1, 8, 1 }, 3.0, 0.0, 0.0, 1, 1.0f, 0.0f },             { { 5, 0, 5, 0 }, 3.0, 0.0, 0.0, 0, 0, 0 },
    };
    for (const D& d : points) {
        const l3d_support_params p = { d.dist_px, d.cos_min, d.min_overlap, 1e-3, 0.0 };
        bad += run({ 0, 0, 1, 16, 0, 1 }, { unit_camera() }, std::vector<float>(d.col, d.col + 4), { 0, 1 }, p, o);
        ++runs;
        bad += check(o, 1, { 0, 1 });
        bad += (int)o.rec.size() != d.expect;
        if (d.expect == 1 && o.rec.size() == 1) bad += !(o.rec[0].dist == d.dist && o.rec[0].overlap == d.overlap && o.best[0] == 0);
        if (d.expect == 0) bad += o.best[0] != -1;
    }
    // a 2-D segment longer than the projected line; two rows tied for a column; a clipped row
    {
        bad += run({ 4, 0, 1, 8, 0, 1 }, { unit_camera() }, { 0, 0.5f, 16, 0.5f }, { 0, 1 }, P0, o) || !(o.rec.size() == 1 && o.rec[0].overlap == 1.0f);
        bad += run({ 0, 0, 1, 16, 0, 1, 0, 0, 1, 16, 0, 1, 0, 2, 1, 16, 2, 1 }, { unit_camera() }, { 2, 1, 10, 1, 2, 2.5f, 10, 2.5f }, { 0, 2 }, P0, o)
               || !(o.rec.size() == 6 && o.best[0] == 0 && o.best[1] == 2);
        bad += run({ -20.5, 10, 1, 40, 10, 1 }, { unit_camera() }, { 5, 10, 30, 10, -18, 10, -4, 10 }, { 0, 2 }, P0, o) || !(o.rec.size() == 1 && o.rec[0].seg2d == 0);
        runs += 3;
    }

    // ---- the sizing rules of the device call
    for (int n : { 1, 255, 256, 257, 8209, 100000, 1 << 20, 1 << 30 })
        for (int opt : { 0, 1, 2, 64, 70000 })
            for (int m : { 1, 3, 64, 1000 }) {
                const int mc = support::chunk_cameras(opt, n, m);
                bad += !(mc >= 1 && mc <= m && mc <= 65535 && (mc == 1 || (long long)mc * n <= support::kMaxScan) && (opt == 0 ? mc <= 64 : mc <= opt));
                for (long long cols : { 0ll, 1ll, 256ll, 257ll, 2000ll, 1000000ll }) {
                    const int C = support::col_chunks(n, mc, cols);
                    const long long tiles = (cols + 255) / 256;
                    bad += !(C >= 1 && C <= 64 && (C <= tiles || C == 1) && (C == 1 || (long long)n * mc * C <= support::kMaxScan));
                    ++runs;
                }
            }
    bad += !(support::chunk_cameras(0, 8209, 64) == 64 && support::col_chunks(8209, 64, 2000) == 1 && support::col_chunks(189, 1, 2000) == 8 && support::col_chunks(20, 1, 513) == 3);
    // the cut of a chunk: the leading cameras whose records stay within 2^31 - 1, decided in 64 bits; 0: the first camera alone has more
    {
        const unsigned long long big = 2147483647ull;
        const unsigned long long a[4] = { 5, 7, 0, 9 }, b[3] = { big, 0, 1 }, c[2] = { big + 1, 1 }, d[3] = { 1ull << 40, 1, 1 }, e[3] = { big - 1, 1, 1 }, f[2] = { 1, ~0ull };
        bad += !(support::cut_chunk(a, 4) == 4 && support::cut_chunk(b, 3) == 2 && support::cut_chunk(c, 2) == 0 && support::cut_chunk(d, 3) == 0
                 && support::cut_chunk(e, 3) == 2 && support::cut_chunk(f, 2) == 1 && support::cut_chunk(a, 0) == 0);
        runs += 7;
    }

    // ---- the refusals
    {
        const double s3[6] = { 0, 0, 1, 16, 0, 1 };
        const float s2[4] = { 2, 1, 10, 1 };
        l3d_camera cam = unit_camera();
        int64_t start[2] = { 0, 1 }, cs[2], counts[4];
        int32_t best[1];
        l3d_support_record* rec = nullptr;
        std::string msg;
        bad += support::check_arguments(s3, 1, &cam, 1, s2, start, &P0, &rec, cs, best, counts, msg) != L3D_OK;
        bad += support::check_arguments(nullptr, 0, nullptr, 0, nullptr, nullptr, &P0, &rec, cs, nullptr, counts, msg) != L3D_OK;
        auto refused = [&](const double* a, int n, const l3d_camera* c, int m, const float* b, const int64_t* st, const l3d_support_params* p, l3d_support_record** r, int64_t* s,
                           int32_t* be, int64_t* co, int code = L3D_ERR_INVALID) {
            ++refusals;
            msg.clear();
            return support::check_arguments(a, n, c, m, b, st, p, r, s, be, co, msg) == code && !msg.empty() ? 0 : 1;
        };
        bad += refused(s3, 1, &cam, 1, s2, start, &P0, nullptr, cs, best, counts);
        bad += refused(s3, 1, &cam, 1, s2, start, &P0, &rec, nullptr, best, counts);
        bad += refused(s3, 1, &cam, 1, s2, start, &P0, &rec, cs, best, nullptr);
        bad += refused(s3, -1, &cam, 1, s2, start, &P0, &rec, cs, best, counts);
        bad += refused(s3, 1, &cam, -1, s2, start, &P0, &rec, cs, best, counts);
        bad += refused(nullptr, 1, &cam, 1, s2, start, &P0, &rec, cs, best, counts);
        bad += refused(s3, 1, nullptr, 1, s2, start, &P0, &rec, cs, best, counts);
        bad += refused(s3, 1, &cam, 1, s2, nullptr, &P0, &rec, cs, best, counts);
        bad += refused(s3, 1, &cam, 1, nullptr, start, &P0, &rec, cs, best, counts);
        bad += refused(s3, 1, &cam, 1, s2, start, &P0, &rec, cs, nullptr, counts);
        bad += refused(s3, 1, &cam, 1, s2, start, nullptr, &rec, cs, best, counts);
        { int64_t st[2] = { 1, 2 }; bad += refused(s3, 1, &cam, 1, s2, st, &P0, &rec, cs, best, counts); }
        { int64_t st[2] = { 0, -1 }; bad += refused(s3, 1, &cam, 1, s2, st, &P0, &rec, cs, best, counts); }
        { int64_t st[2] = { 0, 1ll << 31 }; bad += refused(s3, 1, &cam, 1, s2, st, &P0, &rec, cs, best, counts); }
        for (double v : { -1.0, nan, inf }) { l3d_support_params p = P0; p.dist_px = v; bad += refused(s3, 1, &cam, 1, s2, start, &p, &rec, cs, best, counts); }
        for (double v : { -0.1, 1.5, nan }) { l3d_support_params p = P0; p.cos_min = v; bad += refused(s3, 1, &cam, 1, s2, start, &p, &rec, cs, best, counts); }
        for (double v : { -0.1, 1.5, nan }) { l3d_support_params p = P0; p.min_overlap = v; bad += refused(s3, 1, &cam, 1, s2, start, &p, &rec, cs, best, counts); }
        for (double v : { 0.0, -1.0, nan, inf }) { l3d_support_params p = P0; p.near_z = v; bad += refused(s3, 1, &cam, 1, s2, start, &p, &rec, cs, best, counts); }
        for (double v : { -0.5, nan, 2147483648.0 }) { l3d_support_params p = P0; p.margin = v; bad += refused(s3, 1, &cam, 1, s2, start, &p, &rec, cs, best, counts); }
        { l3d_camera c2 = cam; c2.K[8] = 2.0; bad += refused(s3, 1, &c2, 1, s2, start, &P0, &rec, cs, best, counts); }
        { l3d_camera c2 = cam; c2.width = 0; bad += refused(s3, 1, &c2, 1, s2, start, &P0, &rec, cs, best, counts); }
        bad += refused(s3, (1 << 30) + 1, &cam, 1, s2, start, &P0, &rec, cs, best, counts, L3D_ERR_UNSUPPORTED);
    }
    printf("support: %d runs, %d refusals, %d bad\n", runs, refusals, bad);
    return bad ? 1 : 0;
}
