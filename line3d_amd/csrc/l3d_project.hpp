// l3d_project.hpp -- 3-D segments projected into cameras and clipped to their images ("PROJECTION AND OVERLAYS", 1, in include/line3d_amd.h states
// every rule; tests/project_model.py holds the same in numpy): the camera frame, the near plane, the pixel map and the rectangle rule, written once
// for the device (l3d_project.hip: one (camera, segment) pair per lane) and for the host (l3d_test_project_lines_host: the same functions, lane
// after lane).  Everything is f64, every product, sum and quotient rounded on its own (-ffp-contract=off).  The rectangle rule is also the clip of
// l3d_draw.hpp.  The file is plain C++ as well: tests/cpp/project_draw_asan.cpp builds it into a host program of its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/line3d_amd.h"

#if defined(__HIPCC__)
#define L3D_PJ_HD __host__ __device__ __forceinline__
#else
#define L3D_PJ_HD inline
#endif

namespace l3d {
namespace project {

constexpr double kMaxMargin = 1073741824.0;         // 2^30
constexpr double kMaxFinite = 1.7976931348623157e308;

L3D_PJ_HD bool fin(double x) { return fabs(x) <= kMaxFinite; }          // (NaN compares false)

struct Rect { double xmin, xmax, ymin, ymax; };

L3D_PJ_HD Rect image_rect(int width, int height, double margin)
{
    Rect r;
    r.xmin = -0.5 - margin; r.xmax = ((double)width - 0.5) + margin;
    r.ymin = -0.5 - margin; r.ymax = ((double)height - 0.5) + margin;
    return r;
}

// one edge of Liang-Barsky: false = dropped
L3D_PJ_HD bool clip_edge(double p, double q, double& t0, double& t1)
{
    if (p == 0.0) return !(q < 0.0);
    const double r = q / p;
    if (p < 0.0) { if (r > t1) return false; t0 = fmax(t0, r); }
    else { if (r < t0) return false; t1 = fmin(t1, r); }
    return true;
}

// THE RECTANGLE RULE on the segment (uP, vP) + t (du, dv): kept iff true, with t0 < t1.  All inputs finite.
L3D_PJ_HD bool clip_rect(const Rect& rc, double uP, double vP, double du, double dv, double& t0, double& t1)
{
    t0 = 0.0; t1 = 1.0;
    if (!clip_edge(-du, uP - rc.xmin, t0, t1)) return false;
    if (!clip_edge(du, rc.xmax - uP, t0, t1)) return false;
    if (!clip_edge(-dv, vP - rc.ymin, t0, t1)) return false;
    if (!clip_edge(dv, rc.ymax - vP, t0, t1)) return false;
    return t0 < t1;
}

L3D_PJ_HD void camera_frame(const l3d_camera& c, const double* X, double* o)
{
    for (int r = 0; r < 3; ++r) o[r] = ((c.R[3 * r] * X[0] + c.R[3 * r + 1] * X[1]) + c.R[3 * r + 2] * X[2]) + c.t[r];
}

L3D_PJ_HD void pixel(const l3d_camera& c, const double* p, double& u, double& v)
{
    const double xn = p[0] / p[2], yn = p[1] / p[2];
    u = (c.K[0] * xn + c.K[1] * yn) + c.K[2];
    v = (c.K[3] * xn + c.K[4] * yn) + c.K[5];
}

// One (camera, segment) pair through THE RECTANGLE RULE.  s: P then Q, 6 doubles.  true: kept, with the pixels of both ends, (du, dv), the rule's t0 < t1
// and whether the near plane moved an end (l3d_support.hpp takes its rows from here, in f64)
struct Ends { double uP, vP, uQ, vQ, du, dv, t0, t1; bool movedP, movedQ; };

L3D_PJ_HD bool project_ends(const l3d_camera& c, const double* s, double near_z, double margin, Ends& e)
{
    double P[3], Q[3];
    camera_frame(c, s, P);
    camera_frame(c, s + 3, Q);
    if (!(fin(P[0]) && fin(P[1]) && fin(P[2]) && fin(Q[0]) && fin(Q[1]) && fin(Q[2]))) return false;
    bool movedP = false, movedQ = false;
    if (P[2] < near_z && Q[2] < near_z) return false;
    if (P[2] < near_z) {
        const double t = (near_z - P[2]) / (Q[2] - P[2]);
        P[0] = P[0] + t * (Q[0] - P[0]); P[1] = P[1] + t * (Q[1] - P[1]); P[2] = near_z;
        movedP = true;
    } else if (Q[2] < near_z) {
        const double t = (near_z - Q[2]) / (P[2] - Q[2]);
        Q[0] = Q[0] + t * (P[0] - Q[0]); Q[1] = Q[1] + t * (P[1] - Q[1]); Q[2] = near_z;
        movedQ = true;
    }
    double uP, vP, uQ, vQ;
    pixel(c, P, uP, vP);
    pixel(c, Q, uQ, vQ);
    const double du = uQ - uP, dv = vQ - vP;
    if (!(fin(uP) && fin(vP) && fin(uQ) && fin(vQ) && fin(du) && fin(dv))) return false;
    if (du == 0.0 && dv == 0.0) return false;
    double t0, t1;
    if (!clip_rect(image_rect(c.width, c.height, margin), uP, vP, du, dv, t0, t1)) return false;
    e.uP = uP; e.vP = vP; e.uQ = uQ; e.vQ = vQ; e.du = du; e.dv = dv; e.t0 = t0; e.t1 = t1; e.movedP = movedP; e.movedQ = movedQ;
    return true;
}

// One (camera, segment) pair.  s: P then Q, 6 doubles.  true: kept, with the 2-D segment in o and the flags in fl
L3D_PJ_HD bool project_pair(const l3d_camera& c, const double* s, double near_z, double margin, float* o, unsigned char& fl)
{
    Ends e;
    if (!project_ends(c, s, near_z, margin, e)) return false;
    const double uP = e.uP, vP = e.vP, uQ = e.uQ, vQ = e.vQ, du = e.du, dv = e.dv, t0 = e.t0, t1 = e.t1;
    const bool movedP = e.movedP, movedQ = e.movedQ;
    if (t0 == 0.0) { o[0] = (float)uP; o[1] = (float)vP; }
    else { o[0] = (float)(uP + t0 * du); o[1] = (float)(vP + t0 * dv); }
    if (t1 == 1.0) { o[2] = (float)uQ; o[3] = (float)vQ; }
    else { o[2] = (float)(uP + t1 * du); o[3] = (float)(vP + t1 * dv); }
    fl = (unsigned char)(((movedP || t0 > 0.0) ? 1 : 0) | ((movedQ || t1 < 1.0) ? 2 : 0));
    return true;
}

// the refusals that need no device, in the header's order: L3D_OK, or L3D_ERR_INVALID and why
inline int check_arguments(const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d, int32_t** src_index,
                           unsigned char** flags, int64_t* cam_start, std::string& err)
{
    if (!seg2d || !src_index || !flags || !cam_start) { err = "project lines: a null output pointer"; return L3D_ERR_INVALID; }
    *seg2d = nullptr; *src_index = nullptr; *flags = nullptr;
    if (n < 0 || m < 0) { err = "project lines: a negative count"; return L3D_ERR_INVALID; }
    if ((n > 0 && !seg3d) || (m > 0 && !cameras)) { err = "project lines: a null input pointer"; return L3D_ERR_INVALID; }
    for (int c = 0; c < m; ++c) {
        const l3d_camera& k = cameras[c];
        if (!(k.K[6] == 0.0 && k.K[7] == 0.0 && k.K[8] == 1.0)) { err = "project lines: camera " + std::to_string(c) + ": the third row of K is not (0, 0, 1)"; return L3D_ERR_INVALID; }
        if (k.width < 1 || k.height < 1) { err = "project lines: camera " + std::to_string(c) + ": a size below 1 x 1"; return L3D_ERR_INVALID; }
    }
    if (!(near_z > 0.0 && near_z <= kMaxFinite)) { err = "project lines: near must be a finite number above 0"; return L3D_ERR_INVALID; }
    if (!(margin >= 0.0 && margin <= kMaxMargin)) { err = "project lines: margin must lie in [0, 2^30]"; return L3D_ERR_INVALID; }
    return L3D_OK;
}

// the whole call on the host: camera-major, input order within a camera
inline void run_host(const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, std::vector<float>& seg2d,
                     std::vector<int32_t>& src, std::vector<unsigned char>& flags, int64_t* cam_start)
{
    for (int c = 0; c < m; ++c) {
        cam_start[c] = (int64_t)src.size();
        for (int i = 0; i < n; ++i) {
            float o[4]; unsigned char fl = 0;
            if (!project_pair(cameras[c], seg3d + 6 * (size_t)i, near_z, margin, o, fl)) continue;
            seg2d.insert(seg2d.end(), o, o + 4); src.push_back((int32_t)i); flags.push_back(fl);
        }
    }
    cam_start[m] = (int64_t)src.size();
}

// cameras per chunk of the device call: `opt` (0: 64), cut down so that the chunk's ballot words stay below 2^20 and its pairs below 2^31; at least 1
inline int chunk_cameras(int opt, int n, int m)
{
    long long mc = opt > 0 ? (opt < 65535 ? opt : 65535) : 64;          // (the cameras are the grid's y dimension)
    const long long words = ((long long)n + 63) / 64;
    if (words > 0) mc = mc < (1ll << 20) / words ? mc : (1ll << 20) / words;
    if (n > 0) mc = mc < 2147483647ll / n ? mc : 2147483647ll / n;
    if (mc > m) mc = m;
    return (int)(mc < 1 ? 1 : mc);
}

}  // namespace project
}  // namespace l3d
