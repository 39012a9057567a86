// l3d_support.hpp -- the 2-D segments of every camera that support each 3-D segment ("SUPPORT OF 3-D LINES" in include/line3d_amd.h states every rule;
// tests/support_model.py holds the same in numpy): a row (one 3-D segment projected into one camera by project::project_ends, its ends in f64), a column
// (one 2-D segment of that camera) and the pair test, written once for the device (l3d_support.hip: one row per lane against column tiles in LDS) and for
// the host (l3d_test_support_lines_host: the same functions in loops).  Everything is f64, every product, sum, quotient and square root rounded on its
// own (-ffp-contract=off).  The file is plain C++ as well: tests/cpp/support_asan.cpp builds it into a host program of its own.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "l3d_project.hpp"

namespace l3d {
namespace support {

constexpr double kMaxFinite = 1.7976931348623157e308;
constexpr long long kMaxRecords = 2147483647ll;     // of one camera, and of one chunk of cameras on the device
constexpr long long kMaxScan = 1ll << 30;           // entries of the device's one scan per chunk (rows x cameras x column chunks)
constexpr int kTile = 256;                          // columns per LDS tile of the device search

L3D_PJ_HD bool fin(double x) { return fabs(x) <= kMaxFinite; }          // (NaN compares false)
L3D_PJ_HD double mx(double a, double b) { return a < b ? b : a; }
L3D_PJ_HD double mn(double a, double b) { return b < a ? b : a; }

// A ROW: the first end A, the unit direction da and the length La of the projected, clipped 3-D segment
struct Row { double Ax, Ay, dax, day, La; };

// A COLUMN OF THE TABLE: 64 bytes; ok is 1.0 for an eligible column, and the entry of any other is all zeros
struct Col { double Ux, Uy, Vx, Vy, dbx, dby, Lb, ok; };

// s: P then Q.  false: no row (the projection drops the pair, or the clipped length is not a finite number above 0)
L3D_PJ_HD bool make_row(const l3d_camera& c, const double* s, double near_z, double margin, Row& r)
{
    project::Ends e;
    if (!project::project_ends(c, s, near_z, margin, e)) return false;
    double Ax = e.uP, Ay = e.vP, Bx = e.uQ, By = e.vQ;
    if (!(e.t0 == 0.0)) { Ax = e.uP + e.t0 * e.du; Ay = e.vP + e.t0 * e.dv; }
    if (!(e.t1 == 1.0)) { Bx = e.uP + e.t1 * e.du; By = e.vP + e.t1 * e.dv; }
    const double ax = Bx - Ax, ay = By - Ay;
    const double La = sqrt((ax * ax) + (ay * ay));
    if (!(fin(La) && La > 0.0)) return false;
    r.Ax = Ax; r.Ay = Ay; r.dax = ax / La; r.day = ay / La; r.La = La;
    return true;
}

// g: x1, y1, x2, y2.  false: not eligible
L3D_PJ_HD bool make_col(const float* g, Col& o)
{
    const double Ux = (double)g[0], Uy = (double)g[1], Vx = (double)g[2], Vy = (double)g[3];
    const double bx = Vx - Ux, by = Vy - Uy;
    const double Lb = sqrt((bx * bx) + (by * by));
    const bool ok = fin(Ux) && fin(Uy) && fin(Vx) && fin(Vy) && fin(Lb) && Lb > 0.0;
    o.Ux = ok ? Ux : 0.0; o.Uy = ok ? Uy : 0.0; o.Vx = ok ? Vx : 0.0; o.Vy = ok ? Vy : 0.0;
    o.dbx = ok ? bx / Lb : 0.0; o.dby = ok ? by / Lb : 0.0; o.Lb = ok ? Lb : 0.0; o.ok = ok ? 1.0 : 0.0;
    return ok;
}

// THE PAIR TEST of a row and an eligible column.  true: a record, with its dist and overlap
L3D_PJ_HD bool pair_test(const Row& r, const Col& c, double dist_px, double cos_min, double min_overlap, float& dist, float& overlap)
{
    if (!(fabs((r.dax * c.dbx) + (r.day * c.dby)) >= cos_min)) return false;
    const double wUx = c.Ux - r.Ax, wUy = c.Uy - r.Ay;
    const double eU = fabs((wUx * r.day) - (wUy * r.dax));
    if (!(eU <= dist_px)) return false;
    const double wVx = c.Vx - r.Ax, wVy = c.Vy - r.Ay;
    const double eV = fabs((wVx * r.day) - (wVy * r.dax));
    if (!(eV <= dist_px)) return false;
    const double sU = (wUx * r.dax) + (wUy * r.day), sV = (wVx * r.dax) + (wVy * r.day);
    const double ov = mn(mx(sU, sV), r.La) - mx(mn(sU, sV), 0.0);
    const double Lm = mn(r.La, c.Lb);
    if (!(ov >= min_overlap * Lm)) return false;
    dist = (float)mx(eU, eV);
    overlap = (float)(ov / Lm);
    return true;
}

// the key of a record in the race for its column's best row: a non-negative float's bits order as its value; the smallest key wins
L3D_PJ_HD unsigned long long best_key(float dist, int k)
{
    uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = __float_as_uint(dist);
#else
    memcpy(&b, &dist, 4);
#endif
    return ((unsigned long long)b << 32) | (unsigned long long)(uint32_t)k;
}

// the refusals that need no device, in the header's order: L3D_OK, or a code and why
inline int check_arguments(const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start, const l3d_support_params* prm,
                           l3d_support_record** records, int64_t* cam_start, int32_t* best, int64_t* counts, std::string& err)
{
    if (!records || !cam_start || !counts) { err = "support lines: a null output pointer"; return L3D_ERR_INVALID; }
    *records = nullptr;
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (n < 0 || m < 0) { err = "support lines: a negative count"; return L3D_ERR_INVALID; }
    for (int k = 0; k <= m; ++k) cam_start[k] = 0;
    if ((n > 0 && !seg3d) || (m > 0 && !cameras)) { err = "support lines: a null input pointer"; return L3D_ERR_INVALID; }
    if (m > 0 && !seg_start) { err = "support lines: a null seg_start"; return L3D_ERR_INVALID; }
    if (m > 0 && seg_start[0] != 0) { err = "support lines: seg_start does not begin at 0"; return L3D_ERR_INVALID; }
    for (int c = 0; c < m; ++c) {
        if (seg_start[c + 1] < seg_start[c]) { err = "support lines: seg_start descends at camera " + std::to_string(c); return L3D_ERR_INVALID; }
        if (seg_start[c + 1] - seg_start[c] > 2147483647ll) { err = "support lines: camera " + std::to_string(c) + " has more than 2^31 - 1 segments"; return L3D_ERR_INVALID; }
    }
    if (m > 0 && seg_start[m] > 0 && (!seg2d || !best)) { err = "support lines: a null array of 2-D segments or of best rows"; return L3D_ERR_INVALID; }
    if (!prm) { err = "support lines: null parameters"; return L3D_ERR_INVALID; }
    if (!(prm->dist_px >= 0.0 && prm->dist_px <= kMaxFinite)) { err = "support lines: dist_px must be a finite number, not negative"; return L3D_ERR_INVALID; }
    if (!(prm->cos_min >= 0.0 && prm->cos_min <= 1.0)) { err = "support lines: cos_min must lie in [0, 1]"; return L3D_ERR_INVALID; }
    if (!(prm->min_overlap >= 0.0 && prm->min_overlap <= 1.0)) { err = "support lines: min_overlap must lie in [0, 1]"; return L3D_ERR_INVALID; }
    for (int c = 0; c < m; ++c) {
        const l3d_camera& k = cameras[c];
        if (!(k.K[6] == 0.0 && k.K[7] == 0.0 && k.K[8] == 1.0)) { err = "support lines: camera " + std::to_string(c) + ": the third row of K is not (0, 0, 1)"; return L3D_ERR_INVALID; }
        if (k.width < 1 || k.height < 1) { err = "support lines: camera " + std::to_string(c) + ": a size below 1 x 1"; return L3D_ERR_INVALID; }
    }
    if (!(prm->near_z > 0.0 && prm->near_z <= kMaxFinite)) { err = "support lines: near must be a finite number above 0"; return L3D_ERR_INVALID; }
    if (!(prm->margin >= 0.0 && prm->margin <= project::kMaxMargin)) { err = "support lines: margin must lie in [0, 2^30]"; return L3D_ERR_INVALID; }
    if ((long long)n > kMaxScan) { err = "support lines: more than 2^30 3-D segments"; return L3D_ERR_UNSUPPORTED; }
    return L3D_OK;
}

// cameras per chunk of the device call: `opt` (0: 64), cut down so that the chunk's rows stay within the scan's length; at least 1
inline int chunk_cameras(int opt, int n, int m)
{
    long long mc = opt > 0 ? (opt < 65535 ? opt : 65535) : 64;          // (the cameras are the grid's y dimension)
    if (n > 0) mc = mc < kMaxScan / n ? mc : kMaxScan / n;
    if (mc > m) mc = m;
    return (int)(mc < 1 ? 1 : mc);
}

// chunks of column tiles per row block of the device search (the grid's z dimension): enough for about 1024 workgroups, at most one per tile of the
// chunk's camera with the most columns and at most 64, and rows x cameras x chunks stays within the scan's length
inline int col_chunks(int n, int mc, long long max_cols)
{
    const long long blocks = (((long long)n + kTile - 1) / kTile) * (mc > 0 ? mc : 1);
    const long long tiles = (max_cols + kTile - 1) / kTile;
    long long c = (1024 + blocks - 1) / (blocks > 0 ? blocks : 1);
    if (c > tiles) c = tiles;
    if (c > 64) c = 64;
    const long long rows = (long long)n * (mc > 0 ? mc : 1);
    if (rows > 0 && c > kMaxScan / rows) c = kMaxScan / rows;
    return (int)(c < 1 ? 1 : c);
}

// THE CUT of a chunk after its count pass, from the 64-bit totals of its cameras: the number of leading cameras whose records together stay within
// 2^31 - 1 (the rest is counted again with the next chunk); 0: the first camera alone has more, which the call refuses
inline int cut_chunk(const unsigned long long* cam_total, int mc)
{
    unsigned long long sum = 0;
    int k = 0;
    for (; k < mc; ++k) {
        if (cam_total[k] > (unsigned long long)kMaxRecords || sum + cam_total[k] > (unsigned long long)kMaxRecords) break;
        sum += cam_total[k];
    }
    return k;
}

// best[] and counts[3] from the keys of all columns (all ones: no record)
inline void best_from_keys(const unsigned long long* keys, int64_t n_cols, int32_t* best, int64_t* counts)
{
    counts[3] = 0;
    for (int64_t i = 0; i < n_cols; ++i) {
        const bool any = keys[i] != ~0ull;
        best[i] = any ? (int32_t)(uint32_t)(keys[i] & 0xFFFFFFFFull) : -1;
        counts[3] += any ? 1 : 0;
    }
}

// the whole call on the host: camera-major, ascending k, ascending j.  false: a camera with more than kMaxRecords records
inline bool run_host(const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start, const l3d_support_params& p,
                     std::vector<l3d_support_record>& rec, int64_t* cam_start, int32_t* best, int64_t* counts)
{
    const int64_t T = seg_start[m];
    std::vector<Col> tab((size_t)T);
    std::vector<unsigned long long> keys((size_t)T, ~0ull);
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int64_t i = 0; i < T; ++i) counts[1] += make_col(seg2d + 4 * (size_t)i, tab[(size_t)i]) ? 1 : 0;
    for (int c = 0; c < m; ++c) {
        cam_start[c] = (int64_t)rec.size();
        const int64_t j0 = seg_start[c], nj = seg_start[c + 1] - j0;
        for (int k = 0; k < n; ++k) {
            Row r;
            if (!make_row(cameras[c], seg3d + 6 * (size_t)k, p.near_z, p.margin, r)) continue;
            ++counts[0];
            for (int64_t j = 0; j < nj; ++j) {
                const Col& col = tab[(size_t)(j0 + j)];
                l3d_support_record o;
                if (!(col.ok != 0.0) || !pair_test(r, col, p.dist_px, p.cos_min, p.min_overlap, o.dist, o.overlap)) continue;
                if ((long long)((int64_t)rec.size() - cam_start[c]) >= kMaxRecords) return false;
                o.seg3d = k; o.seg2d = (int32_t)j;
                rec.push_back(o);
                const unsigned long long key = best_key(o.dist, k);
                if (key < keys[(size_t)(j0 + j)]) keys[(size_t)(j0 + j)] = key;
            }
        }
    }
    cam_start[m] = (int64_t)rec.size();
    counts[2] = (int64_t)rec.size();
    if (T) best_from_keys(keys.data(), T, best, counts);
    return true;
}

}  // namespace support
}  // namespace l3d
