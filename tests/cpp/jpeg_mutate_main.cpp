// jpeg_mutate_main.cpp -- the JPEG parser and entropy decoder (line3d_amd/csrc/l3d_jpeg.cpp) over damaged files, built with
// -fsanitize=address,undefined -fno-sanitize-recover by tests/test_jpeg_cpu.py: every truncation length of the files given as "trunc:<path>", and 2000
// seeded single- and double-byte mutations of each file given as "mut:<path>".  Every run must return a status (0, 1 or 5) and touch nothing outside its
// buffers -- the input is copied into a heap block of exactly its length, the coefficients into one of exactly n_blocks x 64, so that the sanitizer
// sees a read or write one byte past either.  Exit 0: all runs returned; the counts are printed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../line3d_amd/csrc/l3d_jpeg.hpp"

namespace {

int counts[6] = { 0, 0, 0, 0, 0, 0 };

bool run(const std::vector<unsigned char>& file, size_t n)
{
    unsigned char* exact = static_cast<unsigned char*>(malloc(n ? n : 1));
    if (n) memcpy(exact, file.data(), n);
    l3d::JpegFrame f;
    std::string err;
    int rc = l3d::jpeg_parse(exact, n, f, err);
    if (rc == l3d::kJpgOk) {
        int16_t* coef = static_cast<int16_t*>(malloc(f.n_blocks * 64 * sizeof(int16_t)));
        rc = l3d::jpeg_decode_coefficients(exact, n, f, coef, err);
        free(coef);
    }
    free(exact);
    if (rc != l3d::kJpgOk && rc != l3d::kJpgInvalid && rc != l3d::kJpgUnsupported) { fprintf(stderr, "status %d is none of 0, 1, 5\n", rc); return false; }
    if (rc != l3d::kJpgOk && err.empty()) { fprintf(stderr, "status %d without a message\n", rc); return false; }
    ++counts[rc];
    return true;
}

bool read_file(const char* path, std::vector<unsigned char>& out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return !out.empty();
}

uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next()      // splitmix64
{
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

}  // namespace

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a) {
        const bool trunc = strncmp(argv[a], "trunc:", 6) == 0, mut = strncmp(argv[a], "mut:", 4) == 0;
        if (!trunc && !mut) { fprintf(stderr, "usage: %s trunc:<file> ... mut:<file> ...\n", argv[0]); return 2; }
        std::vector<unsigned char> file;
        if (!read_file(argv[a] + (trunc ? 6 : 4), file)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        const int ok_before = counts[0];
        if (!run(file, file.size()) || counts[0] == ok_before) { fprintf(stderr, "%s: the intact file does not decode\n", argv[a]); return 1; }
        if (trunc) {
            for (size_t n = 0; n < file.size(); ++n)
                if (!run(file, n)) return 1;
        } else {
            state = 0x9e3779b97f4a7c15ull + (uint64_t)a;
            for (int k = 0; k < 2000; ++k) {
                std::vector<unsigned char> m = file;
                const int changes = 1 + (int)(next() & 1);
                for (int c = 0; c < changes; ++c) {
                    // half of the mutations in the headers (the first 700 bytes hold every table), where a byte decides more
                    const size_t at = (size_t)(next() % ((next() & 1) ? std::min<size_t>(700, m.size()) : m.size()));
                    m[at] = (unsigned char)(next() & 255);
                }
                if (!run(m, m.size())) return 1;
            }
        }
    }
    printf("ok %d invalid %d unsupported %d\n", counts[0], counts[1], counts[5]);
    return 0;
}
