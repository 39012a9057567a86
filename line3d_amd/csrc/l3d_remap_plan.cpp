// l3d_remap_plan.cpp -- the undistortion planner: the output camera and size for a lens, chosen from the undistorted positions of the source
// image's border pixels ("A REMAP" in include/line3d_amd.h states every formula; tests/remap_model.py holds the same in numpy).  Host code in
// double precision: no context, no device.
#include <cmath>
#include <string>

#include "../../include/line3d_amd.h"

namespace {

thread_local std::string g_plan_error;

int refuse(const char* why)
{
    g_plan_error = std::string("undistort_plan: ") + why;
    return L3D_ERR_INVALID;
}

constexpr int kPlanIterations = 50;         // the cap of both Newton iterations
constexpr double kPlanConverged = 1e-12;    // a step at or below this (normalised units / radians) ends an iteration
constexpr double kPlanSizeSlack = 1e-6;     // floor(v + slack): an extent within rounding of a whole pixel counts as that pixel
constexpr double kPlanPi = 3.14159265358979323846;

constexpr int kPlanRaySteps = 16;           // the monotonicity test looks at this many points between the optical axis and a solution

// the determinant of BROWN's Jacobian at (x, y)
double brown_det(const double* k, double x, double y)
{
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    const double r2 = x * x + y * y;
    const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2, den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    const double dnum = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1, dden = (3.0 * k6 * r2 + 2.0 * k5) * r2 + k4;
    const double kr = num / den, dkr = (dnum * den - num * dden) / (den * den);
    const double fx = kr + 2.0 * x * x * dkr + 2.0 * p1 * y + 6.0 * p2 * x, fy = 2.0 * x * y * dkr + 2.0 * p1 * x + 2.0 * p2 * y;
    const double gy = kr + 2.0 * y * y * dkr + 6.0 * p1 * y + 2.0 * p2 * x;
    return fx * gy - fy * fy;
}

// the ideal (x, y) whose distorted position is (xd, yd): Newton on BROWN's two forward formulas with their analytic Jacobian, from (xd, yd).
// false: no convergence, a step that is not finite, a solution on the other side of the axis, or a Jacobian whose determinant is not positive at the
// solution or at one of the points that divide the segment from the axis to it into kPlanRaySteps parts (the lens folds over)
bool invert_brown(const double* k, double xd, double yd, double& x, double& y)
{
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    x = xd; y = yd;
    bool converged = false;
    double det = 0.0;
    for (int it = 0; it <= kPlanIterations; ++it) {
        const double r2 = x * x + y * y;
        const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2, den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
        const double dnum = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1, dden = (3.0 * k6 * r2 + 2.0 * k5) * r2 + k4;
        const double kr = num / den, dkr = (dnum * den - num * dden) / (den * den);
        const double f = x * kr + ((2.0 * p1) * x * y + p2 * (r2 + 2.0 * (x * x))) - xd;
        const double g = y * kr + (p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * x * y) - yd;
        const double fx = kr + 2.0 * x * x * dkr + 2.0 * p1 * y + 6.0 * p2 * x, fy = 2.0 * x * y * dkr + 2.0 * p1 * x + 2.0 * p2 * y;
        const double gx = fy, gy = kr + 2.0 * y * y * dkr + 6.0 * p1 * y + 2.0 * p2 * x;
        det = fx * gy - fy * gx;
        if (converged || it == kPlanIterations) break;          // (the Jacobian above is the solution's)
        const double sx = (gy * f - fy * g) / det, sy = (fx * g - gx * f) / det;
        if (!std::isfinite(sx) || !std::isfinite(sy)) return false;
        x -= sx; y -= sy;
        converged = std::fabs(sx) <= kPlanConverged && std::fabs(sy) <= kPlanConverged;
    }
    if (!converged || !(det > 0.0) || !(x * xd + y * yd >= 0.0)) return false;
    for (int q = 1; q < kPlanRaySteps; ++q) {                   // the lens must not fold over anywhere between the axis and the solution
        const double t = (double)q / (double)kPlanRaySteps;
        if (!(brown_det(k, x * t, y * t) > 0.0)) return false;
    }
    return true;
}

// the angle theta with theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = td: Newton from theta = td.
// false: no convergence, theta outside [0, pi/2), or a derivative that is not positive at the solution or at one of the kPlanRaySteps points between 0
// and it (the radial function is not monotone)
bool invert_fisheye(const double* k, double td, double& theta)
{
    theta = td;
    bool converged = false;
    double d = 0.0;
    for (int it = 0; it <= kPlanIterations; ++it) {
        const double t2 = theta * theta;
        const double poly = 1.0 + (((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2;
        d = 1.0 + (((9.0 * k[3] * t2 + 7.0 * k[2]) * t2 + 5.0 * k[1]) * t2 + 3.0 * k[0]) * t2;
        if (converged || it == kPlanIterations) break;
        const double s = (theta * poly - td) / d;
        if (!std::isfinite(s)) return false;
        theta -= s;
        converged = std::fabs(s) <= kPlanConverged;
    }
    if (!converged || !(d > 0.0) || !(theta >= 0.0 && theta < kPlanPi / 2.0)) return false;
    for (int q = 1; q < kPlanRaySteps; ++q) {
        const double t2 = theta * ((double)q / (double)kPlanRaySteps) * (theta * ((double)q / (double)kPlanRaySteps));
        if (!(1.0 + (((9.0 * k[3] * t2 + 7.0 * k[2]) * t2 + 5.0 * k[1]) * t2 + 3.0 * k[0]) * t2 > 0.0)) return false;
    }
    return true;
}

// one border pixel's undistorted position, clamped to radius r_max where it cannot be used as it is
void border_point(const l3d_lens& L, double j, double i, double r_max, double& x, double& y)
{
    const double xd = (j - L.cx) / L.fx, yd = (i - L.cy) / L.fy;
    const double rd = std::sqrt(xd * xd + yd * yd);
    bool ok;
    if (L.model == L3D_LENS_FISHEYE) {
        double theta = 0.0;
        ok = invert_fisheye(L.k, rd, theta);
        const double s = rd > 1e-8 ? std::tan(theta) / rd : 1.0;
        x = xd * s; y = yd * s;
    } else {
        ok = invert_brown(L.k, xd, yd, x, y);
    }
    const double r = std::sqrt(x * x + y * y);
    if (ok && std::isfinite(r) && r <= r_max) return;
    if (ok && std::isfinite(r)) { x = x / r * r_max; y = y / r * r_max; return; }      // beyond the limit: along its own direction
    if (rd > 0.0) { x = xd / rd * r_max; y = yd / rd * r_max; } else { x = 0.0; y = 0.0; }    // not invertible: along the distorted point's direction
}

}  // namespace

extern "C" const char* l3d_undistort_plan_error(void) { return g_plan_error.c_str(); }

extern "C" int l3d_undistort_plan(const l3d_lens* lens, int width, int height, double alpha, int out_width, int out_height, int max_dim, double fov_max_deg,
                                  double K_out[9], int* w_out, int* h_out)
{
    g_plan_error.clear();
    if (!lens || !K_out || !w_out || !h_out) return refuse("null argument");
    l3d_lens L = *lens;
    if (L.model == 0) { L.model = L3D_LENS_BROWN; for (double& v : L.k) v = 0.0; }       // no distortion: a pinhole camera
    if (L.model != L3D_LENS_BROWN && L.model != L3D_LENS_FISHEYE) return refuse("unknown lens model");
    bool finite = std::isfinite(L.fx) && std::isfinite(L.fy) && std::isfinite(L.cx) && std::isfinite(L.cy);
    for (double v : L.k) finite = finite && std::isfinite(v);
    if (!finite) return refuse("a field of the lens is not finite");
    if (!(L.fx > 0.0 && L.fy > 0.0)) return refuse("the lens must carry its source camera, fx and fy positive");
    if (L.model == L3D_LENS_FISHEYE && (L.k[4] != 0.0 || L.k[5] != 0.0 || L.k[6] != 0.0 || L.k[7] != 0.0)) return refuse("a fisheye lens has four coefficients, k[4..7] must be 0");
    const int kMaxSide = 1 << 24;
    const long long kMaxBytes = 1ll << 31;
    if (width < 8 || height < 8 || width > kMaxSide || height > kMaxSide || 3ll * width * height > kMaxBytes) return refuse("source size below 8 or above the detector's limits");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return refuse("alpha outside [0, 1]");
    if (!(fov_max_deg > 0.0 && fov_max_deg < 180.0)) return refuse("fov_max_deg outside (0, 180)");
    if (max_dim < 0) return refuse("negative max_dim");
    const bool given = out_width > 0 && out_height > 0, source = out_width == 0 && out_height == 0, keep_focal = out_width == -1 && out_height == -1;
    if (!given && !source && !keep_focal) return refuse("out size must be (w, h), (0, 0) for the source size or (-1, -1) for the size that keeps the focal length");
    if (given && (out_width < 8 || out_height < 8 || out_width > kMaxSide || out_height > kMaxSide || 3ll * out_width * out_height > kMaxBytes))
        return refuse("output size below 8 or above the detector's limits");

    // ---- the border points and the two rectangles
    const double r_max = std::tan(fov_max_deg * (kPlanPi / 180.0) / 2.0), inf = INFINITY;
    double lo_x = inf, hi_x = -inf, lo_y = inf, hi_y = -inf;            // outer
    double in_l = -inf, in_r = inf, in_t = -inf, in_b = inf;            // inner
    for (int j = 0; j < width; ++j)
        for (int e = 0; e < 2; ++e) {                                   // top and bottom edge
            double x, y;
            border_point(L, (double)j, e ? (double)(height - 1) : 0.0, r_max, x, y);
            lo_x = std::fmin(lo_x, x); hi_x = std::fmax(hi_x, x); lo_y = std::fmin(lo_y, y); hi_y = std::fmax(hi_y, y);
            if (e) in_b = std::fmin(in_b, y); else in_t = std::fmax(in_t, y);
        }
    for (int i = 0; i < height; ++i)
        for (int e = 0; e < 2; ++e) {                                   // left and right edge (the corners belong to both pairs)
            double x, y;
            border_point(L, e ? (double)(width - 1) : 0.0, (double)i, r_max, x, y);
            lo_x = std::fmin(lo_x, x); hi_x = std::fmax(hi_x, x); lo_y = std::fmin(lo_y, y); hi_y = std::fmax(hi_y, y);
            if (e) in_r = std::fmin(in_r, x); else in_l = std::fmax(in_l, x);
        }
    if (!(in_r > in_l && in_b > in_t)) return refuse("degenerate rectangle: the inner bounds cross (no region of the view is seen along whole rows and columns)");
    const double l = in_l + alpha * (lo_x - in_l), r = in_r + alpha * (hi_x - in_r), t = in_t + alpha * (lo_y - in_t), b = in_b + alpha * (hi_y - in_b);
    const double aspect = L.fy / L.fx;

    // ---- size and focal length
    int w2, h2;
    double fx2;
    if (keep_focal) {
        fx2 = L.fx;
        w2 = (int)std::fmin(std::floor(fx2 * (r - l) + kPlanSizeSlack) + 1.0, 2.0 * kMaxSide);
        h2 = (int)std::fmin(std::floor(fx2 * aspect * (b - t) + kPlanSizeSlack) + 1.0, 2.0 * kMaxSide);
        if (max_dim > 0 && (w2 > max_dim || h2 > max_dim)) {
            const double s = (double)max_dim / (double)(w2 > h2 ? w2 : h2);
            fx2 = L.fx * s;
            w2 = (int)std::floor(fx2 * (r - l) + kPlanSizeSlack) + 1;
            h2 = (int)std::floor(fx2 * aspect * (b - t) + kPlanSizeSlack) + 1;
        }
        if (w2 < 8 || h2 < 8 || w2 > kMaxSide || h2 > kMaxSide || 3ll * w2 * h2 > kMaxBytes) return refuse("the planned output size is below 8 or above the detector's limits");
    } else {
        w2 = given ? out_width : width;
        h2 = given ? out_height : height;
        const double f0 = std::fmax((double)(w2 - 1) / (in_r - in_l), (double)(h2 - 1) / (aspect * (in_b - in_t)));
        const double f1 = std::fmin((double)(w2 - 1) / (hi_x - lo_x), (double)(h2 - 1) / (aspect * (hi_y - lo_y)));
        fx2 = f0 + alpha * (f1 - f0);
    }
    const double fy2 = fx2 * aspect;
    if (!std::isfinite(fx2) || !std::isfinite(fy2) || fx2 == 0.0 || fy2 == 0.0) return refuse("the planned focal length is not finite");
    for (int k = 0; k < 9; ++k) K_out[k] = 0.0;
    K_out[0] = fx2; K_out[4] = fy2; K_out[8] = 1.0;
    K_out[2] = 0.5 * (double)(w2 - 1) - fx2 * (0.5 * (l + r));
    K_out[5] = 0.5 * (double)(h2 - 1) - fy2 * (0.5 * (t + b));
    *w_out = w2; *h_out = h2;
    return L3D_OK;
}
