// The host side of the projection and of the drawing (line3d_amd/csrc/l3d_project.hpp, l3d_draw.hpp: the argument checks, the pair function, the
// rectangle rule, the pieces, the walk of a lane, the blend) as a program of its own, for AddressSanitizer and UBSan:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/project_draw_asan.cpp -o project_draw_asan
//     ./project_draw_asan
// Random and crafted inputs, among them coordinates that are not finite, segments far outside the image, every stroke width's extremes and images
// of one pixel; the pixel buffers are allocated to the byte, so a write past a row or a plane is an error the sanitizer reports.  Exit status 0
// and "0 bad" on its last line: nothing was reported and every invariant held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "../../line3d_amd/csrc/l3d_draw.hpp"
#include "../../line3d_amd/csrc/l3d_project.hpp"

using namespace l3d;

int main()
{
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    int bad = 0, runs = 0, refusals = 0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- projection
    for (int round = 0; round < 40; ++round) {
        const int n = round % 7 == 0 ? 0 : 1 + (int)(rng() % 200), m = 1 + (int)(rng() % 4);
        std::vector<double> seg((size_t)n * 6);
        for (auto& v : seg) v = U(rng) * 6.0;
        if (n > 3) { seg[0] = nan; seg[7] = inf; seg[14] = -inf; seg[20] = 1e300; }
        std::vector<l3d_camera> cams((size_t)m);
        for (auto& c : cams) {
            memset(&c, 0, sizeof(c));
            c.K[0] = 100.0 + U(rng); c.K[1] = U(rng); c.K[2] = 32.0; c.K[4] = 90.0; c.K[5] = 24.0; c.K[8] = 1.0;
            c.R[0] = c.R[4] = c.R[8] = 1.0; c.R[1] = U(rng) * 0.1; c.t[2] = U(rng);
            c.width = 1 + (int)(rng() % 100); c.height = 1 + (int)(rng() % 100);
        }
        float* o = nullptr; int32_t* s = nullptr; unsigned char* f = nullptr;
        std::vector<int64_t> start((size_t)m + 1);
        std::string err;
        if (project::check_arguments(seg.data(), n, cams.data(), m, 1e-3, round % 3 ? 0.0 : 5.0, &o, &s, &f, start.data(), err) != L3D_OK) { ++bad; fprintf(stderr, "refused good arguments: %s\n", err.c_str()); continue; }
        std::vector<float> segs; std::vector<int32_t> src; std::vector<unsigned char> fl;
        project::run_host(seg.data(), n, cams.data(), m, 1e-3, round % 3 ? 0.0 : 5.0, segs, src, fl, start.data());
        ++runs;
        if (segs.size() != src.size() * 4 || fl.size() != src.size() || start[(size_t)m] != (int64_t)src.size()) { ++bad; fprintf(stderr, "projection: sizes disagree\n"); }
        for (size_t k = 0; k < src.size(); ++k)
            if (src[k] < 0 || src[k] >= n || fl[k] > 3 || !(segs[4 * k] == segs[4 * k])) { ++bad; fprintf(stderr, "projection: a bad output\n"); break; }
        if (project::chunk_cameras(0, n, m) < 1 || project::chunk_cameras(1, n, m) != 1) { ++bad; fprintf(stderr, "projection: chunk rule\n"); }
    }
    {
        float* o; int32_t* s; unsigned char* f; int64_t start[2]; std::string err;
        l3d_camera c; memset(&c, 0, sizeof(c)); c.K[0] = c.K[4] = c.K[8] = 1.0; c.R[0] = c.R[4] = c.R[8] = 1.0; c.width = c.height = 4;
        double seg[6] = { 0, 0, 1, 1, 1, 1 };
        auto refused = [&](const double* sg, int n, const l3d_camera* cm, int m, double nr, double mg, float** po) {
            if (project::check_arguments(sg, n, cm, m, nr, mg, po, &s, &f, start, err) == L3D_ERR_INVALID) ++refusals; else { ++bad; fprintf(stderr, "projection: a refusal is missing\n"); }
        };
        refused(nullptr, 1, &c, 1, 1e-3, 0, &o); refused(seg, 1, nullptr, 1, 1e-3, 0, &o); refused(seg, -1, &c, 1, 1e-3, 0, &o); refused(seg, 1, &c, -1, 1e-3, 0, &o);
        refused(seg, 1, &c, 1, 0.0, 0, &o); refused(seg, 1, &c, 1, nan, 0, &o); refused(seg, 1, &c, 1, 1e-3, -1.0, &o); refused(seg, 1, &c, 1, 1e-3, nan, &o);
        refused(seg, 1, &c, 1, 1e-3, 0, nullptr);
        l3d_camera k2 = c; k2.K[8] = 2.0; refused(seg, 1, &k2, 1, 1e-3, 0, &o);
        l3d_camera w0 = c; w0.width = 0; refused(seg, 1, &w0, 1, 1e-3, 0, &o);
    }

    // ---- drawing
    const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
    const double widths[] = { 0.5, 1.0, 2.5, 9.0, 64.0 };
    for (int round = 0; round < 60; ++round) {
        const int w = round % 9 == 0 ? 1 : 1 + (int)(rng() % 90), h = round % 11 == 0 ? 1 : 1 + (int)(rng() % 70), ch = round % 3 == 0 ? 1 : (round % 3 == 1 ? 3 : 4);
        const size_t stride = (size_t)w * ch + (round % 2 ? 0 : 5);
        std::vector<unsigned char> px((size_t)(h - 1) * stride + (size_t)w * ch, 77);          // (to the byte: the last row has no padding)
        const int n = round % 13 == 0 ? 0 : 1 + (int)(rng() % 40);
        std::vector<float> segs((size_t)n * 4);
        for (int k = 0; k < n; ++k) {
            const double scale = k % 5 == 0 ? 1e7 : (k % 5 == 1 ? 3.0 : 1.0);
            segs[4 * k] = (float)((U(rng) * 0.7 + 0.5) * w * scale); segs[4 * k + 1] = (float)((U(rng) * 0.7 + 0.5) * h * scale);
            segs[4 * k + 2] = (float)((U(rng) * 0.7 + 0.5) * w * scale); segs[4 * k + 3] = (float)((U(rng) * 0.7 + 0.5) * h * scale);
            if (k % 7 == 3) { segs[4 * k + 2] = segs[4 * k]; segs[4 * k + 3] = segs[4 * k + 1]; }
        }
        if (n > 2) { segs[1] = fnan; segs[6] = finf; }
        std::vector<unsigned char> colors = { 255, 0, 0, 255, 0, 255, 0, 128, 0, 0, 255, 0 };
        std::vector<int32_t> idx((size_t)n);
        for (int k = 0; k < n; ++k) idx[k] = (int32_t)(rng() % 3);
        const double width_px = widths[round % 5];
        std::string err;
        if (draw::check_arguments(w, h, ch, segs.data(), n, colors.data(), 3, round % 2 ? idx.data() : nullptr, width_px, 200, err) != L3D_OK) { ++bad; fprintf(stderr, "refused a good draw: %s\n", err.c_str()); continue; }
        draw::Target t{};
        t.base = px.data(); t.sy = (long long)stride; t.sx = ch; t.width = w; t.height = h; t.ncomp = ch < 3 ? ch : 3;
        for (int k = 0; k < 3; ++k) t.off[k] = k;
        draw::run_host(t, segs.data(), n, colors.data(), 3, round % 2 ? idx.data() : nullptr, draw::stroke16(width_px), 200);
        ++runs;
        for (int i = 0; i + 1 < h && stride > (size_t)w * ch; ++i)
            for (size_t b = (size_t)w * ch; b < stride; ++b)
                if (px[(size_t)i * stride + b] != 77) { ++bad; fprintf(stderr, "drawing: a padding byte changed\n"); i = h; break; }
        if (ch == 4)
            for (int i = 0; i < h; ++i)
                for (int j = 0; j < w; ++j)
                    if (px[(size_t)i * stride + (size_t)j * 4 + 3] != 77) { ++bad; fprintf(stderr, "drawing: the fourth channel changed\n"); i = h; break; }
    }
    {
        std::string err;
        unsigned char col[4] = { 1, 2, 3, 4 };
        float seg[4] = { 0, 0, 1, 1 };
        int32_t bad_idx[1] = { 1 };
        auto refused = [&](int w, int h, int ch, const float* s, int n, const unsigned char* c, int nc, const int32_t* ix, double wp, int op, int code) {
            if (draw::check_arguments(w, h, ch, s, n, c, nc, ix, wp, op, err) == code) ++refusals; else { ++bad; fprintf(stderr, "drawing: a refusal is missing\n"); }
        };
        refused(0, 4, 3, seg, 1, col, 1, nullptr, 1.0, 255, L3D_ERR_INVALID); refused(4, 4, 2, seg, 1, col, 1, nullptr, 1.0, 255, L3D_ERR_INVALID);
        refused(4, 4, 3, nullptr, 1, col, 1, nullptr, 1.0, 255, L3D_ERR_INVALID); refused(4, 4, 3, seg, 1, nullptr, 1, nullptr, 1.0, 255, L3D_ERR_INVALID);
        refused(4, 4, 3, seg, 1, col, 0, nullptr, 1.0, 255, L3D_ERR_INVALID); refused(4, 4, 3, seg, 1, col, 1, bad_idx, 1.0, 255, L3D_ERR_INVALID);
        refused(4, 4, 3, seg, 1, col, 1, nullptr, 0.25, 255, L3D_ERR_INVALID); refused(4, 4, 3, seg, 1, col, 1, nullptr, 65.0, 255, L3D_ERR_INVALID);
        refused(4, 4, 3, seg, 1, col, 1, nullptr, 1.0, 256, L3D_ERR_INVALID); refused(4, 4, 3, seg, -1, col, 1, nullptr, 1.0, 255, L3D_ERR_INVALID);
        refused(4, 32769, 3, seg, 1, col, 1, nullptr, 1.0, 255, L3D_ERR_UNSUPPORTED); refused(4, 4, 3, seg, (1 << 24) + 1, col, 1, nullptr, 1.0, 255, L3D_ERR_UNSUPPORTED);
    }
    printf("project_draw_asan: %d runs, %d refusals, %d bad\n", runs, refusals, bad);
    return bad ? 1 : 0;
}
