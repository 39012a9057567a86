// l3d_jpeg_device.hip -- the device half of the baseline JPEG decoder (contract: include/line3d_amd.h; host half: l3d_jpeg.cpp).  The host parses the file
// and entropy-decodes into a pinned staging buffer; from there everything is per sample and runs here:
//   k_jpg_idct      dequantisation and IJG's jidctint in 64-bit integers, 8 lanes per 8x8 block (a lane does one column, then one row; the
//                   transpose goes through LDS), writing uint8 component planes padded to whole MCUs
//   k_jpg_assemble  one thread per output pixel: Y, the chroma samples up-sampled on the fly (nothing up-sampled is stored), YCbCr -> RGB,
//                   written B, G, R (or the grey sample) at tight stride into DetectBufs::pixels -- where an uploaded image would be
// Integers only, no atomics: the same file gives the same bytes.
#include "l3d_detect.hpp"

#include "l3d_ctx.hpp"
#include "l3d_hostsort.hpp"
#include "l3d_jpeg.hpp"

namespace l3d {
namespace {

// what the kernels need of a frame; block and plane offsets per component
struct JpgLayout {
    int n_blocks, ncomp, width, height, hs, vs, rgb;
    int block0[3], bw[3];           // first block, blocks per block row
    int plane0[3], pw[3];           // first byte of the plane, bytes per plane row (8 bw)
    int cw[3], chh[3];              // the component's real size
};

constexpr int kQtBytes = 512;       // the staging buffer: 3 x 64 uint16 quantisation values, then the coefficients
constexpr int kIdctThreads = 256, kIdctBlocks = kIdctThreads / 8;
constexpr int kRowPad = 9;          // a tile row of 8 values takes 9 slots: lanes that walk a column of the tile do not meet in one bank

// one 1-D pass of jidctint on v[0..7], before the descale
__device__ inline void idct_pass(const long long v[8], long long o[8])
{
    long long z1 = (v[2] + v[6]) * 4433;
    const long long t2 = z1 - v[6] * 15137, t3 = z1 + v[2] * 6270;
    const long long t0 = (v[0] + v[4]) << 13, t1 = (v[0] - v[4]) << 13;
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    long long a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
    z1 = a0 + a3;
    long long z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const long long z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    o[0] = t10 + a3; o[1] = t11 + a2; o[2] = t12 + a1; o[3] = t13 + a0;
    o[4] = t13 - a0; o[5] = t12 - a1; o[6] = t11 - a2; o[7] = t10 - a3;
}

__global__ __launch_bounds__(kIdctThreads) void k_jpg_idct(const short* __restrict__ coef, const unsigned short* __restrict__ qt, JpgLayout L,
                                                           unsigned char* __restrict__ planes)
{
    __shared__ long long tile[kIdctBlocks][8 * kRowPad];
    const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int blk = blockIdx.x * kIdctBlocks + lb;
    const bool live = blk < L.n_blocks;
    int ci = 0;
    if (live) {
        if (L.ncomp == 3 && blk >= L.block0[1]) ci = blk >= L.block0[2] ? 2 : 1;
        const short* c = coef + (size_t)blk * 64;
        const unsigned short* q = qt + ci * 64;
        long long v[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = (long long)c[r * 8 + j] * (long long)q[r * 8 + j];          // column j
        idct_pass(v, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) tile[lb][r * kRowPad + j] = (o[r] + 1024) >> 11;
    }
    __syncthreads();
    if (!live) return;
    long long v[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[lb][j * kRowPad + k];                                        // row j
    idct_pass(v, o);
    unsigned px[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long s = ((o[k] + 131072) >> 18) + 128;
        px[k] = (unsigned)(s < 0 ? 0 : s > 255 ? 255 : s);
    }
    const int rel = blk - (ci == 0 ? L.block0[0] : ci == 1 ? L.block0[1] : L.block0[2]);
    const int bw = ci == 0 ? L.bw[0] : ci == 1 ? L.bw[1] : L.bw[2];
    const int pw = ci == 0 ? L.pw[0] : ci == 1 ? L.pw[1] : L.pw[2];
    const int p0 = ci == 0 ? L.plane0[0] : ci == 1 ? L.plane0[1] : L.plane0[2];
    const int brow = rel / bw, bcol = rel - brow * bw;
    // 8 bytes at a multiple of 8: the planes start at multiples of 64 and their rows are 8 bw long
    uint2 w;
    w.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    w.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    *reinterpret_cast<uint2*>(planes + (size_t)p0 + (size_t)(brow * 8 + j) * pw + (size_t)bcol * 8) = w;
}

// a chroma sample at output pixel (x, y): the contract's fancy upsampling, edges replicated at the component's real size
__device__ inline int chroma_at(const unsigned char* __restrict__ p, int pw, int cw, int chh, int hs, int vs, int x, int y)
{
    if (hs == 1) return p[(size_t)y * pw + x];
    const int i = x >> 1, odd = x & 1;
    const int in = odd ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (vs == 1) {
        const unsigned char* row = p + (size_t)y * pw;
        return (3 * row[i] + row[in] + (odd ? 2 : 1)) >> 2;
    }
    const int r = y >> 1, rn = (y & 1) ? min(r + 1, chh - 1) : max(r - 1, 0);
    const unsigned char *row = p + (size_t)r * pw, *nb = p + (size_t)rn * pw;
    const int ti = 3 * row[i] + nb[i], tn = 3 * row[in] + nb[in];
    return (3 * ti + tn + (odd ? 7 : 8)) >> 4;
}

__device__ inline unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void k_jpg_assemble(const unsigned char* __restrict__ planes, JpgLayout L, unsigned char* __restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= L.width || y >= L.height) return;
    const int c0 = planes[(size_t)L.plane0[0] + (size_t)y * L.pw[0] + x];
    if (L.ncomp == 1) { out[(size_t)y * L.width + x] = (unsigned char)c0; return; }
    const int c1 = chroma_at(planes + L.plane0[1], L.pw[1], L.cw[1], L.chh[1], L.hs, L.vs, x, y);
    const int c2 = chroma_at(planes + L.plane0[2], L.pw[2], L.cw[2], L.chh[2], L.hs, L.vs, x, y);
    int r, g, b;
    if (L.rgb) { r = c0; g = c1; b = c2; }
    else {
        const int cb = c1 - 128, cr = c2 - 128;
        r = c0 + ((91881 * cr + 32768) >> 16);
        b = c0 + ((116130 * cb + 32768) >> 16);
        g = c0 + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    }
    unsigned char* o = out + ((size_t)y * L.width + x) * 3;
    o[0] = clamp255(b); o[1] = clamp255(g); o[2] = clamp255(r);
}

}  // namespace

// entropy decoding of the files on the host threads, each into its own slice of the pinned staging buffer (its quantisation tables, then its
// coefficients).  The per-file outcome goes into the file's status and message -- nothing is read from a thread's last-error string
int jpeg_stage_files(l3d_ctx* c, JpegStaged* const* files, int n)
{
    DetectBufs& d = c->det;
    size_t stage_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const JpegFrame& f = *files[i]->f;
        if (f.n_blocks == 0 || f.n_blocks > kJpgMaxBlocks) return fail(c, L3D_ERR_INVALID, "jpeg: no parsed frame");       // (jpeg_parse's bound: byte offsets of the planes stay ints)
        files[i]->stage_at = stage_bytes;
        stage_bytes += kQtBytes + f.n_blocks * 64 * sizeof(int16_t);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));            // (the staging buffer is about to be rewritten)
    HIPCHK(c, d.jstage.reserve(stage_bytes));
    unsigned char* stage = d.jstage.as<unsigned char>();
    std::vector<JpegDecodeJob> jobs((size_t)n);
    for (int i = 0; i < n; ++i) {
        unsigned char* at = stage + files[i]->stage_at;
        memset(at, 0, kQtBytes);
        memcpy(at, files[i]->f->qt, sizeof(files[i]->f->qt));
        jobs[i].bytes = files[i]->bytes; jobs[i].n = files[i]->n; jobs[i].f = files[i]->f; jobs[i].coef = reinterpret_cast<int16_t*>(at + kQtBytes);
    }
    jpeg_decode_many(jobs.data(), n, host_threads());
    for (int i = 0; i < n; ++i) { files[i]->status = jobs[i].status; files[i]->err = jobs[i].err; }
    return L3D_OK;
}

// the staged files into their slots of DetectBufs::pixels (tight stride, f.ncomp channels), which the caller has reserved: one upload of the staged
// range, the two kernels per file (a file's layout is a kernel argument).  Returns with the work enqueued on the context's stream
int jpeg_staged_to_pixels(l3d_ctx* c, const JpegStaged* const* files, int B)
{
    DetectBufs& d = c->det;
    hipStream_t st = c->stream;
    size_t lo = ~(size_t)0, hi = 0, plane_bytes = 0, slot = 0;
    for (int b = 0; b < B; ++b) {
        if (!files[b]) continue;
        const JpegFrame& f = *files[b]->f;
        lo = std::min(lo, files[b]->stage_at);
        hi = std::max(hi, files[b]->stage_at + kQtBytes + f.n_blocks * 64 * sizeof(int16_t));
        plane_bytes += f.n_blocks * 64;
        slot = (size_t)f.width * f.height * f.ncomp;
    }
    if (hi == 0) return L3D_OK;
    if (d.jstage.cap < hi) return fail(c, L3D_ERR_INVALID, "jpeg: the files were not staged");
    if (d.pixels.cap < slot * B) return fail(c, L3D_ERR_INVALID, "jpeg: the pixel buffer was not reserved");
    HIPCHK(c, d.jcoef.reserve(hi));
    HIPCHK(c, d.jplanes.reserve(plane_bytes));
    { ProfScope ps(c, "jpg_upload"); HIPCHK(c, hipMemcpyAsync(static_cast<char*>(d.jcoef.p) + lo, d.jstage.as<unsigned char>() + lo, hi - lo, hipMemcpyHostToDevice, st)); }
    size_t plane_at = 0;
    for (int b = 0; b < B; ++b) {
        if (!files[b]) continue;
        const JpegFrame& f = *files[b]->f;
        if ((size_t)f.width * f.height * f.ncomp != slot) return fail(c, L3D_ERR_INVALID, "jpeg: files of different sizes in one chunk");
        JpgLayout L;
        L.n_blocks = (int)f.n_blocks; L.ncomp = f.ncomp; L.width = f.width; L.height = f.height; L.hs = f.hmax; L.vs = f.vmax; L.rgb = f.rgb;
        int comp_at = 0;
        for (int i = 0; i < 3; ++i) {
            const JpegComp& k = f.comp[i < f.ncomp ? i : 0];
            L.block0[i] = i < f.ncomp ? (int)k.block0 : L.n_blocks;
            L.bw[i] = k.bw; L.pw[i] = k.bw * 8; L.cw[i] = k.cw; L.chh[i] = k.chh;
            L.plane0[i] = i < f.ncomp ? comp_at : 0;
            if (i < f.ncomp) comp_at += k.bw * k.bh * 64;
        }
        const char* staged = static_cast<const char*>(d.jcoef.p) + files[b]->stage_at;
        const unsigned short* qt = reinterpret_cast<const unsigned short*>(staged);
        const short* coef = reinterpret_cast<const short*>(staged + kQtBytes);
        unsigned char* planes = d.jplanes.as<unsigned char>() + plane_at;
        { ProfScope ps(c, "k_jpg_idct"); hipLaunchKernelGGL(k_jpg_idct, dim3((L.n_blocks + kIdctBlocks - 1) / kIdctBlocks), dim3(kIdctThreads), 0, st, coef, qt, L, planes); }
        { ProfScope ps(c, "k_jpg_assemble"); hipLaunchKernelGGL(k_jpg_assemble, dim3((f.width + 255) / 256, f.height), dim3(256), 0, st, planes, L, d.pixels.as<unsigned char>() + slot * b); }
        plane_at += f.n_blocks * 64;
    }
    HIPCHK(c, hipGetLastError());
    return L3D_OK;
}

// one file into DetectBufs::pixels
static int jpeg_decode_to_pixels(l3d_ctx* c, const unsigned char* bytes, size_t n, const JpegFrame& f)
{
    JpegStaged file;
    file.bytes = bytes; file.n = n; file.f = &f;
    JpegStaged* files[1] = { &file };
    if (int rc = jpeg_stage_files(c, files, 1)) return rc;
    if (file.status != L3D_OK) return fail(c, file.status, file.err);
    return jpeg_staged_to_pixels(c, files, 1);
}

// host bytes in, host pixels out, device in between
int decode_jpeg(l3d_ctx* c, const unsigned char* bytes, size_t n, unsigned char* out, size_t out_stride)
{
    if (!c) return L3D_ERR_INVALID;
    if (!bytes || !out) return fail(c, L3D_ERR_INVALID, "decode_jpeg: null argument");
    JpegFrame f;
    std::string err;
    if (int rc = jpeg_parse(bytes, n, f, err)) return fail(c, rc, err);
    const size_t row = (size_t)f.width * f.ncomp;
    if (out_stride < row) return fail(c, L3D_ERR_INVALID, "decode_jpeg: the output's row stride is below width x channels");
    HIPCHK(c, hipSetDevice(c->device));
    DetectBufs& d = c->det;
    HIPCHK(c, d.pixels.reserve(row * f.height));
    if (int rc = jpeg_decode_to_pixels(c, bytes, n, f)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(out, out_stride, d.pixels.p, row, row, (size_t)f.height, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return L3D_OK;
}

}  // namespace l3d

int l3d_decode_jpeg(l3d_ctx* c, const unsigned char* bytes, size_t n, unsigned char* out, size_t out_row_stride)
{
    return l3d::decode_jpeg(c, bytes, n, out, out_row_stride);
}
