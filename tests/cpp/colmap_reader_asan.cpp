// The COLMAP reader (line3d_amd/csrc/l3d_sfm.cpp) under AddressSanitizer and UBSan, as a plain host program: it is compiled together with the
// reader's source (no HIP, no device, no Python) and run on the CPU:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/colmap_reader_asan.cpp line3d_amd/csrc/l3d_sfm.cpp -o colmap_asan
//     ./colmap_asan tests/golden/colmap_small
// It reads the fixture in both forms through every accessor, then every truncation of the four files and a few damaged ones.  Exit code 0: every
// read gave a scene or a message, and the sanitizers found nothing.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "../../include/line3d_amd.h"

static std::vector<unsigned char> slurp(const std::string& p)
{
    std::vector<unsigned char> b;
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", p.c_str()); exit(2); }
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}
static void spill(const std::string& p, const std::vector<unsigned char>& b, size_t n)
{
    FILE* f = fopen(p.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", p.c_str()); exit(2); }
    if (n) fwrite(b.data(), 1, n, f);
    fclose(f);
}

// every accessor on every camera of a scene that was read; returns the number of cameras
static int walk(l3d_sfm_scene* s)
{
    const int n = l3d_sfm_num_cameras(s);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        double focal, dist[2], R[9], t[3], K[9], cv[2];
        int nw = 0, w = 0, h = 0, np = 0;
        l3d_sfm_camera(s, i, &focal, dist, R, t, &nw);
        std::vector<uint32_t> ids((size_t)nw + 1);
        l3d_sfm_camera_worldpoints(s, i, ids.data());
        for (int k = 0; k < nw; ++k) sum += ids[(size_t)k];
        l3d_sfm_camera_cv_distortion(s, i, cv);
        const char* name = nullptr;
        const double* params = nullptr;
        if (l3d_sfm_camera_model(s, i, &name, &params, &np) == L3D_OK) for (int k = 0; k < np; ++k) sum += params[k];
        l3d_lens lens;
        if (l3d_sfm_camera_lens(s, i, &lens, K, &w, &h) != L3D_OK) sum += (double)std::string(l3d_sfm_last_error(s)).size();
        sum += (double)std::string(l3d_sfm_camera_name(s, i)).size() + l3d_sfm_camera_id(s, i) + focal + R[8] + t[2] + w + h;
    }
    l3d_sfm_camera_lens(s, n, nullptr, nullptr, nullptr, nullptr);      // out of range, null: refused
    l3d_sfm_camera_model(s, -1, nullptr, nullptr, nullptr);
    return sum == sum ? n : -1;
}

static int read_dir(const std::string& dir, bool must_succeed)
{
    l3d_sfm_scene* s = nullptr;
    const int rc = l3d_sfm_read_colmap(dir.c_str(), &s);
    int bad = 0;
    if (rc == L3D_OK) { if (walk(s) <= 0) bad = 1; }
    else if (must_succeed || !s || !*l3d_sfm_last_error(s)) bad = 1;      // a failed read carries its message
    if (bad) fprintf(stderr, "%s: rc %d, %s\n", dir.c_str(), rc, s ? l3d_sfm_last_error(s) : "no scene");
    l3d_sfm_free(s);
    return bad;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <tests/golden/colmap_small> [scratch directory]\n", argv[0]); return 2; }
    const std::string fixture = argv[1], scratch = std::string(argc > 2 ? argv[2] : "/tmp") + "/colmap_asan_scratch";
    mkdir(scratch.c_str(), 0700);
    int bad = read_dir(fixture + "/txt", true) + read_dir(fixture + "/bin", true) + read_dir(fixture + "/none", false);
    int reads = 3;
    for (const char* form : { "bin", "txt" }) {
        const std::string ext = form;
        const std::vector<unsigned char> cams = slurp(fixture + "/" + ext + "/cameras." + ext), ims = slurp(fixture + "/" + ext + "/images." + ext);
        for (int which = 0; which < 2; ++which) {
            const std::vector<unsigned char>& cut = which ? ims : cams;
            for (size_t n = 0; n < cut.size(); ++n) {           // every truncation: a message or, for text cut at a line's end, a smaller scene
                spill(scratch + "/cameras." + ext, cams, which ? cams.size() : n);
                spill(scratch + "/images." + ext, ims, which ? n : ims.size());
                bad += read_dir(scratch, false);
                ++reads;
            }
        }
        // single bytes damaged: model ids, counts, name bytes
        for (size_t at = 0; at < cams.size(); at += 3) {
            std::vector<unsigned char> d = cams;
            d[at] ^= 0xff;
            spill(scratch + "/cameras." + ext, d, d.size());
            spill(scratch + "/images." + ext, ims, ims.size());
            bad += read_dir(scratch, false);
            ++reads;
        }
        remove((scratch + "/cameras." + ext).c_str());
        remove((scratch + "/images." + ext).c_str());
    }
    rmdir(scratch.c_str());
    printf("%d reads, %d bad\n", reads, bad);
    return bad ? 1 : 0;
}
