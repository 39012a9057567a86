// The host side of the segment mask (line3d_amd/csrc/l3d_segmask.hpp: the argument checks, the samples, the lens map, the run search on the validity
// words, the host's wave) under AddressSanitizer and UBSan, as a plain host program (no HIP, no device, no Python):
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/segmask_asan.cpp -o segmask_asan
//     ./segmask_asan
// Every mask is a heap block of exactly stride x (height - 1) + width bytes, so a read one byte past the plane is caught.  The segments run through,
// beside and far outside the masks, with coordinates that are huge, infinite and NaN; every mode, thresholds, gaps up to INT_MAX and lengths; with
// BROWN and FISHEYE lenses, one whose denominator crosses zero included; and the refusals.  Exit code 0: every call gave an ordered output with
// finite segments or a refusal with a message, an all-valid mask gave the input back, and the sanitizers found nothing.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../line3d_amd/csrc/l3d_segmask.hpp"

using namespace l3d;

static int runs_ok = 0, refusals = 0, bad = 0;

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static void check_output(const std::vector<float>& in, const std::vector<float>& out, const std::vector<int32_t>& src, const char* what)
{
    bool ok = out.size() == src.size() * 4;
    for (size_t i = 0; ok && i < src.size(); ++i) {
        ok = src[i] >= 0 && (size_t)src[i] < in.size() / 4 && (i == 0 || src[i] >= src[i - 1]);
        for (int k = 0; k < 4; ++k) ok = ok && std::isfinite(out[4 * i + k]);
    }
    if (!ok) { ++bad; fprintf(stderr, "bad output: %s\n", what); }
    ++runs_ok;
}

int main()
{
    const float nan = std::nanf(""), inf = INFINITY;
    const int extents[][3] = { { 1, 1, 1 }, { 16, 12, 16 }, { 16, 12, 21 }, { 37, 5, 40 }, { 96, 64, 96 }, { 3, 70, 3 } };     // width, height, stride
    const int modes[] = { L3D_SEGMASK_DROP, L3D_SEGMASK_CLIP, L3D_SEGMASK_SPLIT };
    const int gaps[] = { 0, 5, INT_MAX };
    const int thresholds[] = { 0, 128 };
    const double lengths[] = { 0.0, 1.0, 7.75, 1e300 };
    l3d_lens lenses[4];
    memset(lenses, 0, sizeof(lenses));
    lenses[1].model = L3D_LENS_BROWN; lenses[1].k[0] = -0.21; lenses[1].k[1] = 0.06; lenses[1].k[2] = 0.001; lenses[1].k[3] = -0.002;
    lenses[2].model = L3D_LENS_FISHEYE; lenses[2].k[0] = -0.04; lenses[2].k[1] = 0.012;
    lenses[3].model = L3D_LENS_BROWN; lenses[3].k[0] = 0.1; lenses[3].k[5] = -4.0;        // den = 1 - 4 r2 crosses zero: inf and NaN positions
    unsigned seed = 7;
    for (const auto& e : extents) {
        const int w = e[0], h = e[1], stride = e[2];
        for (int fill = 0; fill < 3; ++fill) {                 // all valid, all invalid, a pattern of graded bytes
            std::vector<unsigned char> plane((size_t)stride * (h - 1) + w);
            for (size_t i = 0; i < plane.size(); ++i) plane[i] = fill == 0 ? 255 : fill == 1 ? 0 : (unsigned char)(lcg(seed) % 3 ? lcg(seed) & 255 : 0);
            std::vector<float> segs;
            auto add = [&](float a, float b, float c, float d) { segs.push_back(a); segs.push_back(b); segs.push_back(c); segs.push_back(d); };
            add(0.0f, 0.0f, (float)(w - 1), (float)(h - 1));
            add((float)(w - 1), 0.0f, 0.0f, (float)(h - 1));
            add(-0.5f, -0.5f, (float)w - 0.5f, (float)h - 0.5f);
            add(-30.0f, (float)h / 2, (float)w + 200.0f, (float)h / 2 + 0.3f);
            add((float)w / 2, -500.0f, (float)w / 2, 500.0f);
            add(0.25f, 0.25f, 0.25f, 0.25f);
            add(nan, 0.0f, 1.0f, 1.0f); add(0.0f, 0.0f, inf, 1.0f); add(-inf, 0.0f, inf, 0.0f);
            add(0.0f, 0.0f, 65535.9f, 0.0f); add(0.0f, 0.0f, 65536.0f, 3.0f); add(-3e38f, 0.0f, 3e38f, 1.0f); add(3e38f, 3e38f, 3.0000002e38f, 3e38f);
            add(2147483648.0f, 1.0f, 2147483700.0f, 3.0f); add(-2147483904.0f, 1.0f, -2147483648.0f, 3.0f);
            for (int r = 0; r < 24; ++r) {
                const float x = (float)(lcg(seed) % (unsigned)(w + 8)) - 4.0f + 0.37f, y = (float)(lcg(seed) % (unsigned)(h + 8)) - 4.0f + 0.61f;
                add(x, y, x + (float)(lcg(seed) % 140) - 70.0f + 0.13f, y + (float)(lcg(seed) % 140) - 70.0f - 0.29f);
            }
            for (int mode : modes) for (int gap : gaps) for (int thr : thresholds) for (double len : lengths) for (int li = 0; li < 4; ++li) {
                if (li && (gap != 0 || thr == 128)) continue;              // (the lenses on part of the grid)
                l3d_segment_mask m;
                memset(&m, 0, sizeof(m));
                m.mask = plane.data(); m.mask_row_stride = (size_t)stride; m.mask_width = w; m.mask_height = h;
                m.mode = mode; m.threshold = thr; m.keep_permille = (gap % 7) * 160; m.max_gap = gap; m.min_length = len;
                segmask::Plan p;
                std::string err;
                if (segmask::check_fields(&m, p, err) != L3D_OK) { ++bad; fprintf(stderr, "refused a good mask: %s\n", err.c_str()); continue; }
                if (li) {           // (the lens as the library's check resolves it: the segments' camera about the mask's middle, the source camera zoomed in)
                    p.lens_on = 1;
                    p.L.model = lenses[li].model;
                    for (int k = 0; k < 8; ++k) p.L.k[k] = lenses[li].k[k];
                    p.L.ofx = p.L.ofy = 0.5 * w + 2.0; p.L.ocx = 0.5 * w; p.L.ocy = 0.5 * h;
                    p.L.fx = p.L.fy = 0.8 * w + 2.0; p.L.cx = 0.5 * w - 0.3; p.L.cy = 0.5 * h + 0.2;
                }
                std::vector<float> out;
                std::vector<int32_t> src;
                segmask::run_host(p, segs.data(), (int)(segs.size() / 4), out, src);
                check_output(segs, out, src, "grid");
                if (fill == 0 && !li && len == 0.0 && mode != L3D_SEGMASK_DROP && w > 1 && h > 1) {          // all valid: the first two segments lie inside and come back bit for bit
                    if (src.size() < 2 || src[0] != 0 || src[1] != 1 || memcmp(out.data(), segs.data(), 32) != 0) { ++bad; fprintf(stderr, "all-valid mask changed a segment\n"); }
                }
                if (fill == 1 && thr != 0 && !(mode == L3D_SEGMASK_DROP && m.keep_permille == 0) && !out.empty()) { ++bad; fprintf(stderr, "all-invalid mask kept a segment\n"); }
            }
        }
    }
    // the refusals of the argument check, each with a message
    unsigned char one_byte = 255;
    l3d_segment_mask good;
    memset(&good, 0, sizeof(good));
    good.mask = &one_byte; good.mask_row_stride = 1; good.mask_width = 1; good.mask_height = 1;
    auto refuse = [&](l3d_segment_mask m, const l3d_segment_mask* ptr = nullptr, bool null_struct = false) {
        segmask::Plan p;
        std::string err;
        const int rc = segmask::check_fields(null_struct ? nullptr : (ptr ? ptr : &m), p, err);
        if (rc != L3D_ERR_INVALID || err.size() < 10) { ++bad; fprintf(stderr, "a refusal is missing or has no message (rc %d)\n", rc); }
        ++refusals;
    };
    refuse(good, nullptr, true);
    { l3d_segment_mask m = good; m.mask = nullptr; refuse(m); }
    { l3d_segment_mask m = good; m.mask_width = 0; refuse(m); }
    { l3d_segment_mask m = good; m.mask_height = -4; refuse(m); }
    { l3d_segment_mask m = good; m.mask_width = 2; refuse(m); }                 // stride 1 below width 2
    { l3d_segment_mask m = good; m.mode = 3; refuse(m); }
    { l3d_segment_mask m = good; m.mode = -1; refuse(m); }
    { l3d_segment_mask m = good; m.threshold = 256; refuse(m); }
    { l3d_segment_mask m = good; m.threshold = -1; refuse(m); }
    { l3d_segment_mask m = good; m.keep_permille = 1001; refuse(m); }
    { l3d_segment_mask m = good; m.keep_permille = -1; refuse(m); }
    { l3d_segment_mask m = good; m.max_gap = -1; refuse(m); }
    { l3d_segment_mask m = good; m.min_length = -1.0; refuse(m); }
    { l3d_segment_mask m = good; m.min_length = std::nan(""); refuse(m); }
    { l3d_segment_mask m = good; m.min_length = INFINITY; refuse(m); }
    { segmask::Plan p; std::string err; if (segmask::check_fields(&good, p, err) != L3D_OK || p.threshold != 1) { ++bad; fprintf(stderr, "a good mask was refused, or threshold 0 does not read as 1\n"); } }
    printf("segmask_asan: %d runs, %d refusals, %d bad\n", runs_ok, refusals, bad);
    return bad ? 1 : 0;
}
