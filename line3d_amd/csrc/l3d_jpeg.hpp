// l3d_jpeg.hpp -- the host half of the baseline JPEG decoder (l3d_jpeg.cpp): marker parser and Huffman decoder.  Plain C++17, no HIP: it
// compiles alone with g++ (tests/cpp/jpeg_mutate_main.cpp).  The device half (k_jpg_idct, k_jpg_assemble) is in l3d_jpeg_device.hip; the contract
// is stated in include/line3d_amd.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace l3d {

// status codes of include/line3d_amd.h (kept apart so that this file needs no other header)
constexpr int kJpgOk = 0, kJpgInvalid = 1, kJpgUnsupported = 5;
// the largest frame jpeg_parse accepts, in 8x8 blocks of all components (2^24: a gigabyte of component planes, whose byte offsets stay ints on the
// device; 128 bytes of coefficients per block on the host).  Beyond: kJpgUnsupported
constexpr size_t kJpgMaxBlocks = (size_t)1 << 24;

struct JpegComp {
    int id = 0, h = 1, v = 1, tq = 0;      // component id, sampling factors, quantisation table
    int td = 0, ta = 0;                    // Huffman tables of the scan
    int bw = 0, bh = 0;                    // blocks per row / rows of blocks, over whole MCUs
    int cw = 0, chh = 0;                   // the component's real size: ceil(W h / hmax), ceil(H v / vmax)
    size_t block0 = 0;                     // first block of the component in the coefficient buffer
};

// a Huffman table as DHT states it: codes per length 1..16, then the symbols in code order
struct JpegHuff {
    uint8_t bits[17] = { 0 }, vals[256] = { 0 };
    bool defined = false;
};

// what the headers say (everything in front of the entropy-coded data)
struct JpegFrame {
    JpegHuff huff[2][4];                   // [0]: DC, [1]: AC -- as they stand at SOS
    int width = 0, height = 0, ncomp = 0;  // ncomp: 1 or 3 -- the output's channels
    int hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
    int restart_interval = 0;
    int rgb = 0;                           // 3 components that are R, G, B already (libjpeg's rule: JFIF, Adobe transform, component ids)
    JpegComp comp[3];
    uint16_t qt[3][64];                    // per COMPONENT, natural (row-major) order
    size_t n_blocks = 0;                   // blocks of all components: the coefficient buffer holds 64 int16 each
    size_t scan_offset = 0;                // first byte of the entropy-coded data
};

// headers only: up to and including SOS.  kJpgOk, or the status with `err` naming the cause
int jpeg_parse(const unsigned char* bytes, size_t n, JpegFrame& f, std::string& err);
// entropy decoding into `coef` (f.n_blocks x 64 int16, natural order; per component, per block row, per block column).  The buffer is
// written in full (absent coefficients are zero)
int jpeg_decode_coefficients(const unsigned char* bytes, size_t n, const JpegFrame& f, int16_t* coef, std::string& err);

// several files at once (l3d_jpeg_batch.cpp): jpeg_decode_coefficients of every job on up to `threads` host threads.  Each job has its own buffer,
// status and message; the outcome of a job does not depend on the others or on the number of threads
struct JpegDecodeJob {
    const unsigned char* bytes = nullptr;
    size_t n = 0;
    const JpegFrame* f = nullptr;
    int16_t* coef = nullptr;
    int status = 0;
    std::string err;
};
void jpeg_decode_many(JpegDecodeJob* jobs, int n, unsigned threads);

}  // namespace l3d
