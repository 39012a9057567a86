// The undistortion planner (line3d_amd/csrc/l3d_remap_plan.cpp) under AddressSanitizer and UBSan, as a plain host program: it is compiled together
// with the planner's source (no HIP, no device, no Python) and run on the CPU:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/remap_plan_asan.cpp line3d_amd/csrc/l3d_remap_plan.cpp -o plan_asan
//     ./plan_asan
// It plans a grid of lenses -- weak and strong, BROWN and FISHEYE, principal points inside and far outside the image, coefficients that make the
// Newton iterations diverge or produce inf and NaN -- at several sizes, alphas and size modes, and every refusal.  Exit code 0: every call gave a
// plan or a message, every plan is finite and within the detector's limits, and the sanitizers found nothing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../include/line3d_amd.h"

static int plans = 0, refusals = 0, bad = 0;

static void one(const l3d_lens& L, int w, int h, double alpha, int ow, int oh, int max_dim, double fov)
{
    double K[9];
    int w2 = -7, h2 = -7;
    const int rc = l3d_undistort_plan(&L, w, h, alpha, ow, oh, max_dim, fov, K, &w2, &h2);
    if (rc == L3D_OK) {
        ++plans;
        bool ok = w2 >= 8 && h2 >= 8 && w2 <= (1 << 24) && h2 <= (1 << 24);
        for (int k = 0; k < 9; ++k) ok = ok && std::isfinite(K[k]);
        ok = ok && K[0] > 0.0 && K[4] > 0.0 && K[8] == 1.0 && K[1] == 0.0;
        if (ow > 0) ok = ok && w2 == ow && h2 == oh;
        if (!ok) { ++bad; fprintf(stderr, "bad plan: model %d, %dx%d alpha %g out %dx%d -> %dx%d fx %g\n", L.model, w, h, alpha, ow, oh, w2, h2, K[0]); }
    } else {
        ++refusals;
        if (rc != L3D_ERR_INVALID || strlen(l3d_undistort_plan_error()) < 10) { ++bad; fprintf(stderr, "refusal without a message (rc %d)\n", rc); }
    }
}

int main()
{
    const double ks[][8] = { { 0, 0, 0, 0, 0, 0, 0, 0 }, { -0.1, 0.01, 0, 0, 0, 0, 0, 0 }, { -0.6, 0.2, 0.05, -0.04, 0.1, 0, 0, 0 }, { 0.4, 0, 0, 0, 0, -4.0, 0, 0 },
                             { 30.0, -500.0, 3.0, 3.0, 1e4, 0, 0, 0 }, { -0.04, 0.012, -0.005, 0.0015, 0, 0, 0, 0 }, { -2.0, 5.0, -9.0, 4.0, 0, 0, 0, 0 },
                             { 1e300, 1e300, 0, 0, 0, 0, 0, 0 } };
    const int sizes[][2] = { { 8, 8 }, { 37, 29 }, { 640, 480 }, { 1921, 9 } };
    const double cams[][4] = { { 0.7, 0.7, 0.5, 0.5 }, { 0.2, 0.21, 0.45, 0.55 }, { 3.0, 3.0, -4.0, 0.5 }, { 0.5, 0.5, 0.5, -20.0 }, { 1e-6, 1e-6, 0.5, 0.5 } };   // in units of the width
    for (int model = 0; model <= 2; ++model)
        for (const auto& k : ks)
            for (const auto& s : sizes)
                for (const auto& c : cams) {
                    l3d_lens L;
                    memset(&L, 0, sizeof L);
                    L.model = model;
                    L.fx = c[0] * s[0]; L.fy = c[1] * s[0]; L.cx = c[2] * s[0]; L.cy = c[3] * s[1];
                    for (int i = 0; i < 8; ++i) L.k[i] = (model == L3D_LENS_FISHEYE && i >= 4) ? 0.0 : k[i];
                    for (double alpha : { 0.0, 0.37, 1.0 }) {
                        one(L, s[0], s[1], alpha, 0, 0, 0, 120.0);
                        one(L, s[0], s[1], alpha, -1, -1, 0, 120.0);
                        one(L, s[0], s[1], alpha, -1, -1, 64, 170.0);
                        one(L, s[0], s[1], alpha, 33, 17, 0, 20.0);
                    }
                }
    // the refusals
    l3d_lens good;
    memset(&good, 0, sizeof good);
    good.model = L3D_LENS_FISHEYE; good.fx = good.fy = 300.0; good.cx = 160.0; good.cy = 120.0; good.k[0] = -0.01;
    const int before = plans;
    double K[9]; int w2, h2;
    one(good, 320, 240, -0.1, 0, 0, 0, 120.0); one(good, 320, 240, NAN, 0, 0, 0, 120.0); one(good, 7, 240, 0.0, 0, 0, 0, 120.0);
    one(good, 320, 240, 0.0, 5, 100, 0, 120.0); one(good, 320, 240, 0.0, 0, 100, 0, 120.0); one(good, 320, 240, 0.0, 0, 0, -1, 120.0);
    one(good, 320, 240, 0.0, 0, 0, 0, 180.0); one(good, 320, 240, 0.0, 40000, 40000, 0, 120.0);
    if (l3d_undistort_plan(nullptr, 320, 240, 0.0, 0, 0, 0, 120.0, K, &w2, &h2) != L3D_ERR_INVALID) ++bad;
    if (l3d_undistort_plan(&good, 320, 240, 0.0, 0, 0, 0, 120.0, nullptr, &w2, &h2) != L3D_ERR_INVALID) ++bad;
    if (plans != before) { ++bad; fprintf(stderr, "a call that must be refused gave a plan\n"); }
    one(good, 320, 240, 0.5, 0, 0, 0, 120.0);
    if (plans != before + 1) ++bad;
    printf("%d plans, %d refusals, %d bad\n", plans, refusals, bad);
    return bad ? 1 : 0;
}
