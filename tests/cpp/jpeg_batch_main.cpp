// jpeg_batch_main.cpp -- the entropy decoder over several files at once (line3d_amd/csrc/l3d_jpeg_batch.cpp: jpeg_decode_many on the host threads)
// against the serial decode, built from the host-only sources with -fsanitize=address,undefined -fno-sanitize-recover (and once with
// -fsanitize=thread) by tests/test_add_images_cpu.py.  The files given on the command line -- intact ones, truncated ones and files the parser
// refuses -- are decoded one after the other, then together on 1, 2 and 8 threads, several rounds each so that the pool's threads are reused:
// every status, every message and every coefficient buffer must equal the serial decode's.  The buffers are heap blocks of exactly
// n_blocks x 64 values, so that a write one past a file's slice is seen.  Exit 0: all equal; the counts are printed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../line3d_amd/csrc/l3d_jpeg.hpp"

namespace {

struct File {
    std::vector<unsigned char> bytes;
    l3d::JpegFrame frame;
    int parse_status = 0, status = 0;
    std::string err;
    std::vector<int16_t> coef;          // the serial decode's
};

bool read_file(const char* path, std::vector<unsigned char>& out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return !out.empty();
}

}  // namespace

int main(int argc, char** argv)
{
    std::vector<File> files((size_t)(argc > 1 ? argc - 1 : 0));
    int decoded = 0, failed = 0, refused = 0;
    for (int a = 1; a < argc; ++a) {
        File& f = files[(size_t)a - 1];
        if (!read_file(argv[a], f.bytes)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        f.parse_status = l3d::jpeg_parse(f.bytes.data(), f.bytes.size(), f.frame, f.err);
        if (f.parse_status != l3d::kJpgOk) { f.status = f.parse_status; ++refused; continue; }
        f.coef.assign(f.frame.n_blocks * 64, 0);
        f.status = l3d::jpeg_decode_coefficients(f.bytes.data(), f.bytes.size(), f.frame, f.coef.data(), f.err);
        ++(f.status == l3d::kJpgOk ? decoded : failed);
    }
    if (files.empty()) { fprintf(stderr, "usage: %s <file> ...\n", argv[0]); return 2; }
    const unsigned threads[3] = { 1, 2, 8 };
    for (unsigned nt : threads)
        for (int round = 0; round < 4; ++round) {
            std::vector<l3d::JpegDecodeJob> jobs;
            std::vector<int16_t*> bufs;
            std::vector<size_t> of;
            for (size_t i = 0; i < files.size(); ++i) {
                const File& f = files[(i + (size_t)round) % files.size()];      // another order every round
                if (f.parse_status != l3d::kJpgOk) continue;                     // a refused file never reaches the decoder: its status is the parser's
                l3d::JpegDecodeJob j;
                j.bytes = f.bytes.data(); j.n = f.bytes.size(); j.f = &f.frame;
                j.coef = static_cast<int16_t*>(malloc(f.frame.n_blocks * 64 * sizeof(int16_t)));
                j.status = -1; j.err = "stale";
                jobs.push_back(j); bufs.push_back(j.coef); of.push_back((i + (size_t)round) % files.size());
            }
            l3d::jpeg_decode_many(jobs.data(), (int)jobs.size(), nt);
            bool same = true;
            for (size_t k = 0; k < jobs.size(); ++k) {
                const File& f = files[of[k]];
                if (jobs[k].status != f.status || jobs[k].err != f.err) { fprintf(stderr, "%u threads, file %zu: status %d \"%s\", serial %d \"%s\"\n", nt, of[k], jobs[k].status, jobs[k].err.c_str(), f.status, f.err.c_str()); same = false; }
                else if (memcmp(bufs[k], f.coef.data(), f.coef.size() * sizeof(int16_t)) != 0) { fprintf(stderr, "%u threads, file %zu: coefficients differ from the serial decode\n", nt, of[k]); same = false; }
                free(bufs[k]);
            }
            if (!same) return 1;
        }
    printf("files %zu decoded %d failed %d refused %d\n", files.size(), decoded, failed, refused);
    return 0;
}
