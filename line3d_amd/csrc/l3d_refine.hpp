// l3d_refine.hpp -- non-linear refinement of a cluster's 3-D line against the 2-D segments of its members, as functions the host and the
// device share (the idiom of l3d_linefit.hpp): the arithmetic is written once, uses only + - * / sqrt and comparisons, and the build
// has -ffp-contract=off, so the two give the same bits.  The reference has no such step (its successor, Line3D++, added one); this
// comment is its specification, and tests/refine_model.py is written from it.
//
// INPUT per cluster ("group"): members in key order.  Member m has a camera index c into a table of 3x4 matrices P = [M | p4] (f64,
// row-major), a 2-D segment (x1, y1, x2, y2) (f32, widened to f64) and the two 3-D end points X of its hypothesis (f64), in P's frame.
// Points are numbered 2*m + {0, 1}.  Per camera, once: Minv = la::inverse(M) (cofactor inverse), C = -(Minv p4).
//
// NOT FINITE: if any end-point coordinate or segment coordinate of the group is not finite (x - x != 0), or the group has no member, nothing is computed: status 2,
// iterations 0, no segments, and line[0..5], rms_before, rms_after are the quiet NaN with the bits 0x7ff8000000000000.
//
// START: (Pc, dir) = fit::line_of_points over the 2n points.  State: A = Pc, d = dir (unit), Pc0 = Pc.
//
// EVALUATION of a state (A, d) with huber scale c:
//   basis: k = index of the smallest |d_k| (first on ties), u = (d x e_k) / |d x e_k|, v = d x u.
//   member m, camera (M, p4):  p = M A + p4,  g = M d,  l = p x g,  n2 = l0^2 + l1^2.
//     n2 not finite or n2 < 1e-300: the member is DROPPED from this evaluation (both end points; counted in `dropped`).
//     else n = sqrt(n2), dl_1..4 = (M u) x g, (M v) x g, p x (M u), p x (M v)         (derivatives of l by the local parameters at 0)
//     end point j = 0, 1 with x = (x_j, y_j, 1):
//       s = l0 x_j + l1 y_j + l2,  r = s / n                                            (pixels)
//       J_i = (dl_i0 x_j + dl_i1 y_j + dl_i2) / n - s (l0 dl_i0 + l1 dl_i1) / (n2 n)    (i = 1..4)
//       |r| <= c or c == 0:  w = 1, rho = r^2;   else  w = c / |r|, rho = 2 c |r| - c^2
//       H_ab += w J_a J_b (a <= b: 10 sums),  b_a += w J_a r (4 sums),  cost += rho,  sumsq += r^2,  count += 1
//   ORDER OF EVERY SUM (part of the result): lane L of 64 sums the members m = L, L + 64, ... in ascending m, end point 0 before 1, from 0.0;
//   the 64 partial sums are combined by s = s + other(L xor off) for off = 32, 16, 8, 4, 2, 1 -- addition commutes, so every lane ends with
//   the same bits.  The host runs the same 64 partial sums and the same tree.
//   rms = sqrt(sumsq / count), 0 when count == 0 (unweighted, over the end points that were not dropped).
//
// LEVENBERG-MARQUARDT: lambda = 1e-3, iterations = 0.  S = evaluation of the start; rms_before from S.  If n - dropped < 2: status 2 (the
// start is returned).  Otherwise, while iterations < max_iterations and S.cost != 0:
//   solve (H + lambda diag(H)) delta = -b by a 4x4 Cholesky factorisation (L L^T, column by column; a pivot that is not > 0 or not finite,
//   or a delta that is not finite, fails the trial);  iterations += 1 (every trial counts, failed ones too)
//   trial state: A' = A + a u + b v,  d' = (d + c' u + e' v) / |d + c' u + e' v|,  then A' is RE-CENTRED: A' <- A' + ((Pc0 - A') . d') d'
//   (re-centring BEFORE the trial is evaluated: the cost that decides is the cost of exactly the state that is kept, so the recorded cost
//   never rises);  S' = evaluation of (A', d')
//   accepted (solve ok and S'.cost < S.cost):  dec = S.cost - S'.cost;  small = dec <= 1e-14 * S.cost;  (A, d, S) <- (A', d', S');
//       lambda <- max(lambda / 10, 1e-12);  stop if small
//   not accepted:  lambda <- min(10 lambda, 1e12);  stop if lambda >= 1e12
// status 0 if a trial was accepted, else 1.  rms_after from the final S.  DIRECTION SIGN at the end: d <- -d if its component of largest
// magnitude (first on ties: the rule of line_of_points) is negative.
//
// SEGMENTS of the line (A, d): end point i of member m, x = (x_j, y_j, 1), hypothesis point X:
//   q = Minv x,  w = C - A,  den = (q.q) - (d.q)^2;   den > 1e-12 (q.q) and status != 2:  t = [(q.q)(d.w) - (d.q)(q.w)] / den   (the point of
//   the line closest to the viewing ray);  otherwise (ray parallel to the line, or status 2):  t = d . (X - A).
//   The points are ranked by (t, point index) -- rank = number of points (t_j, j) below (t_i, i), the stable order as in k_fit_clusters; a t that is not
//   a number ranks as +infinity -- and swept by fit::sweep_line with the point A + t d: a stretch exists while segments of >= 3 cameras are open.
#pragma once

#include "l3d_linefit.hpp"

namespace l3d {
namespace refine {

using la::M3;
using la::V3;

struct Cam { double P[12]; double Minv[9]; double C[3]; };           // the table the device reads: 24 doubles per camera

// sums of an evaluation: 0..9 H (00 01 02 03 11 12 13 22 23 33), 10..13 b, 14 cost, 15 sumsq, 16 count, 17 dropped members
constexpr int kSums = 18;
constexpr double kLambda0 = 1e-3, kLambdaMin = 1e-12, kLambdaMax = 1e12, kN2Min = 1e-300, kDecRel = 1e-14, kParallel = 1e-12;

L3D_LA_HD inline bool fin(double x) { return x - x == 0.0; }
L3D_LA_HD inline double quiet_nan() { const unsigned long long b = 0x7ff8000000000000ull; double x; memcpy(&x, &b, 8); return x; }
L3D_LA_HD inline V3 mulM(const double* P, V3 x) { return { P[0] * x.x + P[1] * x.y + P[2] * x.z, P[4] * x.x + P[5] * x.y + P[6] * x.z, P[8] * x.x + P[9] * x.y + P[10] * x.z }; }

inline void make_cam(const double* P, Cam& c)
{
    memcpy(c.P, P, 96);
    M3 M;
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) M(r, k) = P[r * 4 + k];
    const M3 Mi = la::inverse(M);
    memcpy(c.Minv, Mi.m, 72);
    const V3 q = la::mul(Mi, V3{ P[3], P[7], P[11] });
    c.C[0] = -q.x; c.C[1] = -q.y; c.C[2] = -q.z;
}

L3D_LA_HD inline void basis(V3 d, V3& u, V3& v)
{
    const double a[3] = { fabs(d.x), fabs(d.y), fabs(d.z) };
    int k = 0; if (a[1] < a[k]) k = 1; if (a[2] < a[k]) k = 2;
    const V3 e = k == 0 ? V3{ 1, 0, 0 } : (k == 1 ? V3{ 0, 1, 0 } : V3{ 0, 0, 1 });
    u = la::cross(d, e);
    u = u / la::norm(u);
    v = la::cross(d, u);
}

// one member's two end points into a lane's partial sums
L3D_LA_HD inline void add_member(double* s, const Cam& c, const float* sg, V3 A, V3 d, V3 u, V3 v, double hub)
{
    const V3 p = mulM(c.P, A) + V3{ c.P[3], c.P[7], c.P[11] }, g = mulM(c.P, d), l = la::cross(p, g);
    const double n2 = l.x * l.x + l.y * l.y;
    if (!fin(n2) || n2 < kN2Min) { s[17] = s[17] + 1.0; return; }
    const double n = std::sqrt(n2), n3 = n2 * n;
    const V3 Mu = mulM(c.P, u), Mv = mulM(c.P, v);
    const V3 dl[4] = { la::cross(Mu, g), la::cross(Mv, g), la::cross(p, Mu), la::cross(p, Mv) };
    double ln[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ln[i] = l.x * dl[i].x + l.y * dl[i].y;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double x = (double)sg[2 * j], y = (double)sg[2 * j + 1];
        const double sx = l.x * x + l.y * y + l.z, r = sx / n;
        double J[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) J[i] = (dl[i].x * x + dl[i].y * y + dl[i].z) / n - sx * ln[i] / n3;
        const double ar = fabs(r);
        double w = 1.0, rho = r * r;
        if (!(ar <= hub) && hub != 0.0) { w = hub / ar; rho = 2.0 * hub * ar - hub * hub; }
        int q = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = a; b < 4; ++b) { s[q] = s[q] + w * J[a] * J[b]; ++q; }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) s[10 + a] = s[10 + a] + w * J[a] * r;
        s[14] = s[14] + rho; s[15] = s[15] + r * r; s[16] = s[16] + 1.0;
    }
}

// (H + lambda diag(H)) delta = -b, Cholesky; false: a pivot not > 0 or not finite, or delta not finite
L3D_LA_HD inline bool solve4(const double* s, double lambda, double* delta)
{
    const double a00 = s[0] + lambda * s[0], a01 = s[1], a02 = s[2], a03 = s[3], a11 = s[4] + lambda * s[4], a12 = s[5], a13 = s[6], a22 = s[7] + lambda * s[7], a23 = s[8],
                 a33 = s[9] + lambda * s[9];
    if (!(a00 > 0.0) || !fin(a00)) return false;
    const double l00 = std::sqrt(a00), l10 = a01 / l00, l20 = a02 / l00, l30 = a03 / l00;
    const double p1 = a11 - l10 * l10;
    if (!(p1 > 0.0) || !fin(p1)) return false;
    const double l11 = std::sqrt(p1), l21 = (a12 - l20 * l10) / l11, l31 = (a13 - l30 * l10) / l11;
    const double p2 = a22 - l20 * l20 - l21 * l21;
    if (!(p2 > 0.0) || !fin(p2)) return false;
    const double l22 = std::sqrt(p2), l32 = (a23 - l30 * l20 - l31 * l21) / l22;
    const double p3 = a33 - l30 * l30 - l31 * l31 - l32 * l32;
    if (!(p3 > 0.0) || !fin(p3)) return false;
    const double l33 = std::sqrt(p3);
    const double y0 = (0.0 - s[10]) / l00, y1 = ((0.0 - s[11]) - l10 * y0) / l11, y2 = ((0.0 - s[12]) - l20 * y0 - l21 * y1) / l22,
                 y3 = ((0.0 - s[13]) - l30 * y0 - l31 * y1 - l32 * y2) / l33;
    const double x3 = y3 / l33, x2 = (y2 - l32 * x3) / l22, x1 = (y1 - l21 * x2 - l31 * x3) / l11, x0 = (y0 - l10 * x1 - l20 * x2 - l30 * x3) / l00;
    delta[0] = x0; delta[1] = x1; delta[2] = x2; delta[3] = x3;
    return fin(x0) && fin(x1) && fin(x2) && fin(x3);
}

L3D_LA_HD inline double rms_of(const double* s) { return s[16] > 0.0 ? std::sqrt(s[15] / s[16]) : 0.0; }

// the line parameter of an end point (see SEGMENTS)
L3D_LA_HD inline double point_t(const Cam& c, double x, double y, V3 X, V3 A, V3 d, bool by_ray)
{
    const V3 q = { c.Minv[0] * x + c.Minv[1] * y + c.Minv[2], c.Minv[3] * x + c.Minv[4] * y + c.Minv[5], c.Minv[6] * x + c.Minv[7] * y + c.Minv[8] };
    const V3 w = V3{ c.C[0], c.C[1], c.C[2] } - A;
    const double qq = la::dot(q, q), dq = la::dot(d, q), den = qq - dq * dq;
    if (by_ray && den > kParallel * qq) return (qq * la::dot(d, w) - dq * la::dot(q, w)) / den;
    return la::dot(d, X - A);
}

// the members' tables of one group and its scratch (2n: t, order; n: open, cid, ccnt) and outputs
struct Group {
    int n;
    const int* cam; const float* seg; const double* pts;     // n, 4n, 6n
    double* t; int* order; unsigned char* open; unsigned* cid; unsigned* ccnt;
    double* line; double* rms_before; double* rms_after; int* iterations; int* status; double* out; int* out_cnt;
};

// A wave W runs the group: W::sum<N>(o, f) -- f(lane, acc) adds lane's share into acc (zeroed), the 64 shares are combined by the xor tree;
// W::lanes(f) -- f(lane) for every lane; W::first(f) -- once; W::sync() -- memory written by lanes() is visible after it.  On the device W is the
// wave itself (every lane holds the same state), on the host a loop over 64 lanes.  get(i) = 3-D point i (the caller may have staged them).
template <class W, class Get>
L3D_LA_HD inline void refine_group(W& wv, const Group& G, Get get, const Cam* cams, int max_iterations, double hub)
{
    const int n = G.n, n2 = 2 * n;
    double bad[1];
    wv.template sum<1>(bad, [&](int lane, double* a) {
        for (int m = lane; m < n; m += 64) {
            for (int k = 0; k < 6; ++k) if (!fin(G.pts[6 * (size_t)m + k])) a[0] = a[0] + 1.0;
            for (int k = 0; k < 4; ++k) if (!fin((double)G.seg[4 * (size_t)m + k])) a[0] = a[0] + 1.0;
        }
    });
    if (bad[0] != 0.0 || n == 0) {
        wv.first([&]() {
            const double qn = quiet_nan();
            for (int k = 0; k < 6; ++k) G.line[k] = qn;
            *G.rms_before = qn; *G.rms_after = qn; *G.iterations = 0; *G.status = 2; *G.out_cnt = 0;
        });
        return;
    }
    V3 Pc0, d, min_point;
    fit::line_of_points(get, n2, Pc0, d, min_point);
    V3 A = Pc0, u, v;
    double S[kSums], T[kSums];
    basis(d, u, v);
    wv.template sum<kSums>(S, [&](int lane, double* a) { for (int m = lane; m < n; m += 64) add_member(a, cams[G.cam[m]], G.seg + 4 * (size_t)m, A, d, u, v, hub); });
    const double rms0 = rms_of(S);
    int status = 1, it = 0;
    if ((double)n - S[17] < 2.0) status = 2;
    else {
        double lambda = kLambda0;
        while (it < max_iterations && S[14] != 0.0) {
            double dl[4];
            const bool ok = solve4(S, lambda, dl);
            ++it;
            bool accepted = false, small = false;
            if (ok) {
                V3 A1 = A + dl[0] * u + dl[1] * v, d1 = d + dl[2] * u + dl[3] * v;
                d1 = d1 / la::norm(d1);
                A1 = A1 + la::dot(Pc0 - A1, d1) * d1;
                V3 u1, v1;
                basis(d1, u1, v1);
                wv.template sum<kSums>(T, [&](int lane, double* a) { for (int m = lane; m < n; m += 64) add_member(a, cams[G.cam[m]], G.seg + 4 * (size_t)m, A1, d1, u1, v1, hub); });
                if (T[14] < S[14]) {
                    accepted = true;
                    small = S[14] - T[14] <= kDecRel * S[14];
                    A = A1; d = d1; u = u1; v = v1;
                    for (int k = 0; k < kSums; ++k) S[k] = T[k];
                }
            }
            if (accepted) {
                status = 0;
                lambda = lambda / 10.0; if (lambda < kLambdaMin) lambda = kLambdaMin;
                if (small) break;
            } else {
                lambda = 10.0 * lambda; if (lambda > kLambdaMax) lambda = kLambdaMax;
                if (lambda >= kLambdaMax) break;
            }
        }
    }
    {
        const double a[3] = { fabs(d.x), fabs(d.y), fabs(d.z) };
        int k = 0; if (a[1] > a[k]) k = 1; if (a[2] > a[k]) k = 2;
        const double c = k == 0 ? d.x : (k == 1 ? d.y : d.z);
        if (c < 0) d = d * -1.0;
    }
    const bool by_ray = status != 2;
    wv.lanes([&](int lane) {
        for (int i = lane; i < n2; i += 64) {
            const int m = i >> 1;
            const float* sg = G.seg + 4 * (size_t)m + 2 * (i & 1);
            G.t[i] = point_t(cams[G.cam[m]], (double)sg[0], (double)sg[1], get(i), A, d, by_ray);
            G.order[i] = i;
        }
    });
    wv.sync();
    wv.lanes([&](int lane) {
        for (int i = lane; i < n2; i += 64) {
            const double ti = G.t[i], ki = ti == ti ? ti : HUGE_VAL;
            int r = 0;
            for (int j = 0; j < n2; ++j) { const double tj = G.t[j], kj = tj == tj ? tj : HUGE_VAL; r += (kj < ki) || (kj == ki && j < i); }
            G.order[r] = i;
        }
    });
    wv.sync();
    const double rms1 = rms_of(S);
    wv.first([&]() {
        int n_out = 0;
        double* out = G.out;
        fit::sweep_line(G.order, n2, [&](int p) { return A + G.t[p] * d; }, [&](int member) { return (unsigned)G.cam[member]; }, G.open, G.cid, G.ccnt,
                        [&](V3 s0, V3 e0) { double* o = out + 6 * (size_t)n_out++; o[0] = s0.x; o[1] = s0.y; o[2] = s0.z; o[3] = e0.x; o[4] = e0.y; o[5] = e0.z; });
        G.line[0] = A.x; G.line[1] = A.y; G.line[2] = A.z; G.line[3] = d.x; G.line[4] = d.y; G.line[5] = d.z;
        *G.rms_before = rms0; *G.rms_after = rms1; *G.iterations = it; *G.status = status; *G.out_cnt = n_out;
    });
}

// the host's wave: 64 lanes one after the other, the same partial sums and the same tree
struct HostWave {
    template <int N, class F> void sum(double* o, F f)
    {
        double p[64][N], q[64][N];
        for (int l = 0; l < 64; ++l) { for (int k = 0; k < N; ++k) p[l][k] = 0.0; f(l, p[l]); }
        for (int off = 32; off >= 1; off >>= 1) {
            for (int l = 0; l < 64; ++l) for (int k = 0; k < N; ++k) q[l][k] = p[l][k] + p[l ^ off][k];
            memcpy(p, q, sizeof(p));
        }
        for (int k = 0; k < N; ++k) o[k] = p[0][k];
    }
    template <class F> void lanes(F f) { for (int l = 0; l < 64; ++l) f(l); }
    template <class F> void first(F f) { f(); }
    void sync() {}
};

}  // namespace refine
}  // namespace l3d
