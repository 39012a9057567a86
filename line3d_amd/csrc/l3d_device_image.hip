// l3d_device_image.hip -- images in device memory: the descriptor's checks, the gather into the detector's pixel buffer (k_det_ingest) and the way
// back (k_det_egress).  The descriptor, the conversion rule and the contract are stated in include/line3d_amd.h ("Images in DEVICE memory").
//
// Both kernels compute ONE function per output byte -- out(y, x, k) = convert(source element (y, x, chan[k])) -- and differ only in how many bytes a
// lane moves at a time.  Two work shapes, chosen per image on the host (DevDesc::rows_as_bytes):
//   rows as bytes   an 8-bit image whose rows are runs of width x channels bytes in the detector's own order (stride_c 1, stride_x = channels = the
//                   detector's, chan the identity): a row is copied in 16-byte chunks aligned on the DESTINATION; the source chunk is read as one
//                   16-byte load, as four 4-byte loads or as bytes, whichever its address allows (per row: a crop's rows differ), the chunks at a
//                   row's two ends go byte by byte.  Rows that follow one another without a gap on both sides are ONE row (per image)
//   pixel groups    everything else: a lane takes four pixels of a row, reads each detector channel's four elements -- with one vector load where
//                   the elements are adjacent (stride_x 1: planar layouts and grey images, each plane coalesced along x) and the address is aligned
//                   to the four, else element by element (the generic path) -- converts, and stores the 4 x ch bytes as dwords where the
//                   destination is aligned to 4 bytes, else as bytes.  The last group of a row takes the pixels that exist, element by element
// No atomics, no LDS, no scratch (every small array below is unrolled into registers).
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "l3d_ctx.hpp"
#include "l3d_detect.hpp"
#include "l3d_jpeg.hpp"

namespace l3d {
namespace {

constexpr long long kExtentLimit = 1ll << 62;

inline int elem_bytes(int dtype) { return dtype == L3D_U8 ? 1 : dtype == L3D_F32 ? 4 : 2; }

// one image of a chunk as the kernels see it.  off[k]: element offset of detector channel k (chan[k] * stride_c); ptr null: the slot is left alone
struct DevDesc {
    unsigned char* ptr;
    long long sy, sx, off[3];
    int dtype, rows_as_bytes;
    float scale;
    int pad;
};

// ---- the conversion rule, both directions
__device__ inline unsigned to_u8(float x, float scale)
{
    const float y = x * scale;
    float r = rintf(y);
    if (!(r >= 0.0f)) r = 0.0f;             // NaN and everything below 0
    if (r > 255.0f) r = 255.0f;
    return (unsigned)(int)r;
}
__device__ inline unsigned ingest_elem(const unsigned char* p, long long at, int dtype, float scale)
{
    switch (dtype) {
    case L3D_U8: return p[at];
    case L3D_U16: return to_u8((float)reinterpret_cast<const unsigned short*>(p)[at], scale);
    case L3D_F16: return to_u8((float)reinterpret_cast<const _Float16*>(p)[at], scale);
    default: return to_u8(reinterpret_cast<const float*>(p)[at], scale);
    }
}
__device__ inline void egress_elem(unsigned char* p, long long at, int dtype, float scale, unsigned v)
{
    const float y = (float)v * scale;
    switch (dtype) {
    case L3D_U8: p[at] = (unsigned char)v; break;
    case L3D_U16: {
        float r = rintf(y);
        if (!(r >= 0.0f)) r = 0.0f;
        if (r > 65535.0f) r = 65535.0f;
        reinterpret_cast<unsigned short*>(p)[at] = (unsigned short)(int)r;
        break;
    }
    case L3D_F16: reinterpret_cast<_Float16*>(p)[at] = (_Float16)y; break;
    default: reinterpret_cast<float*>(p)[at] = y;
    }
}

// ---- rows as bytes: `rows` runs of L bytes, src_stride / dst_stride bytes apart; work item `id` is chunk id % nchunk of row id / nchunk, the chunks
// 16 bytes wide and aligned on the destination (the first and the last of a row are partial)
__device__ inline void copy_row_chunk(const unsigned char* src, long long src_stride, unsigned char* dst, long long dst_stride, long long L, long long rows, long long id)
{
    if (src_stride == L && dst_stride == L) { L *= rows; rows = 1; }          // no gaps on either side: one run
    const long long nchunk = (L + 15) / 16 + 1;
    const long long row = id / nchunk, c = id % nchunk;
    if (row >= rows) return;
    const unsigned char* s = src + row * src_stride;
    unsigned char* d = dst + row * dst_stride;
    const long long start = c * 16 - (long long)(reinterpret_cast<uintptr_t>(d) & 15);
    const long long b = start < 0 ? 0 : start, e = start + 16 < L ? start + 16 : L;
    if (b >= e) return;
    if (e - b == 16) {
        const unsigned char* sp = s + start;
        const uintptr_t a = reinterpret_cast<uintptr_t>(sp);
        uint4 v;
        if ((a & 15) == 0) v = *reinterpret_cast<const uint4*>(sp);
        else if ((a & 3) == 0) {
            const unsigned* q = reinterpret_cast<const unsigned*>(sp);
            v = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
            unsigned w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = (unsigned)sp[4 * i] | (unsigned)sp[4 * i + 1] << 8 | (unsigned)sp[4 * i + 2] << 16 | (unsigned)sp[4 * i + 3] << 24;
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(d + start) = v;
    } else {
        for (long long i = b; i < e; ++i) d[i] = s[i];
    }
}

// ---- pixel groups, ingest: four elements of one detector channel from x0 on, converted, packed low byte first; n: how many exist (4: all)
__device__ inline unsigned load_group(const DevDesc& d, long long at, int n)
{
    const unsigned char* p = d.ptr;
    if (n == 4 && d.sx == 1) {
        const int es = d.dtype == L3D_U8 ? 1 : d.dtype == L3D_F32 ? 4 : 2;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p) + (uintptr_t)(at * es);
        if ((a & (uintptr_t)(4 * es - 1)) == 0) {
            if (d.dtype == L3D_U8) return *reinterpret_cast<const unsigned*>(a);
            if (d.dtype == L3D_F32) {
                const float4 v = *reinterpret_cast<const float4*>(a);
                return to_u8(v.x, d.scale) | to_u8(v.y, d.scale) << 8 | to_u8(v.z, d.scale) << 16 | to_u8(v.w, d.scale) << 24;
            }
            const uint2 v = *reinterpret_cast<const uint2*>(a);
            const unsigned short h0 = (unsigned short)(v.x & 0xffffu), h1 = (unsigned short)(v.x >> 16), h2 = (unsigned short)(v.y & 0xffffu), h3 = (unsigned short)(v.y >> 16);
            if (d.dtype == L3D_U16)
                return to_u8((float)h0, d.scale) | to_u8((float)h1, d.scale) << 8 | to_u8((float)h2, d.scale) << 16 | to_u8((float)h3, d.scale) << 24;
            return to_u8((float)__builtin_bit_cast(_Float16, h0), d.scale) | to_u8((float)__builtin_bit_cast(_Float16, h1), d.scale) << 8 |
                   to_u8((float)__builtin_bit_cast(_Float16, h2), d.scale) << 16 | to_u8((float)__builtin_bit_cast(_Float16, h3), d.scale) << 24;
        }
    }
    unsigned r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) r |= ingest_elem(p, at + j * d.sx, d.dtype, d.scale) << (8 * j);
    return r;
}

template <int CH>
__device__ inline void ingest_group(const DevDesc& d, int w, int h, unsigned char* dst, long long id)
{
    const int G = (w + 3) / 4;
    const long long y = id / G;
    if (y >= h) return;
    const int x0 = (int)(id % G) * 4, n = min(4, w - x0);
    unsigned c[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) c[k] = load_group(d, y * d.sy + (long long)x0 * d.sx + d.off[k], n);
    unsigned char* o = dst + (y * w + x0) * CH;
    if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        if (CH == 1) o4[0] = c[0];
        else {          // p0c0 p0c1 p0c2 p1c0 | p1c1 p1c2 p2c0 p2c1 | p2c2 p3c0 p3c1 p3c2
            const unsigned a = c[0], b = c[CH > 1 ? 1 : 0], g = c[CH > 2 ? 2 : 0];
            o4[0] = (a & 0xffu) | (b & 0xffu) << 8 | (g & 0xffu) << 16 | (a >> 8 & 0xffu) << 24;
            o4[1] = (b >> 8 & 0xffu) | (g >> 8 & 0xffu) << 8 | (a >> 16 & 0xffu) << 16 | (b >> 16 & 0xffu) << 24;
            o4[2] = (g >> 16 & 0xffu) | (a >> 24) << 8 | (b >> 24) << 16 | (g >> 24) << 24;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
#pragma unroll
                for (int k = 0; k < CH; ++k) o[j * CH + k] = (unsigned char)(c[k] >> (8 * j) & 0xffu);
            }
    }
}

// the chunk's images (blockIdx.y) into their tight slots of `out`: w x h pixels of ch (1 or 3) bytes each
__global__ __launch_bounds__(256) void k_det_ingest(const DevDesc* __restrict__ tab, int w, int h, int ch, unsigned char* __restrict__ out)
{
    const DevDesc d = tab[blockIdx.y];
    if (!d.ptr) return;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned char* dst = out + (size_t)blockIdx.y * w * h * ch;
    if (d.rows_as_bytes) copy_row_chunk(d.ptr, d.sy, dst, (long long)w * ch, (long long)w * ch, h, id);
    else if (ch == 1) ingest_group<1>(d, w, h, dst, id);
    else ingest_group<3>(d, w, h, dst, id);
}

// one image: tight w x h x ch bytes at src into the memory d describes.  A lane takes one pixel (its channels' elements lie wherever the strides say)
__global__ __launch_bounds__(256) void k_det_egress(const unsigned char* __restrict__ src, int w, int h, int ch, DevDesc d)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d.rows_as_bytes) { copy_row_chunk(src, (long long)w * ch, d.ptr, d.sy, (long long)w * ch, h, id); return; }
    const long long y = id / w;
    if (y >= h) return;
    const int x = (int)(id % w);
    const unsigned char* s = src + (y * w + x) * ch;
    const long long at = y * d.sy + (long long)x * d.sx;
    egress_elem(d.ptr, at + d.off[0], d.dtype, d.scale, s[0]);
    if (ch == 3) {
        egress_elem(d.ptr, at + d.off[1], d.dtype, d.scale, s[1]);
        egress_elem(d.ptr, at + d.off[2], d.dtype, d.scale, s[2]);
    }
}

DevDesc make_desc(const l3d_device_image& im)
{
    DevDesc d;
    const int ch = device_image_det_channels(im.channels);
    d.ptr = static_cast<unsigned char*>(const_cast<void*>(im.ptr));
    d.sy = im.stride_y; d.sx = im.stride_x;
    for (int k = 0; k < 3; ++k) d.off[k] = im.channels == 1 ? 0 : (long long)im.chan[k] * im.stride_c;
    d.dtype = im.dtype;
    d.scale = im.scale;
    d.pad = 0;
    const bool identity = im.channels == 1 || (im.chan[0] == 0 && im.chan[1] == 1 && im.chan[2] == 2 && im.stride_c == 1);
    d.rows_as_bytes = im.dtype == L3D_U8 && im.channels == ch && identity && im.stride_x == ch;
    return d;
}

// work items per image: the larger of the two shapes' counts
long long work_items(int w, int h, int ch)
{
    const long long groups = (long long)h * ((w + 3) / 4), chunks = (long long)h * (((long long)w * ch + 15) / 16 + 1);
    return std::max(groups, chunks);
}

// the context's stream behind whatever `stream` holds now
int wait_for_stream(l3d_ctx* c, void* stream)
{
    DetectBufs& d = c->det;
    if (!d.dev_event) HIPCHK(c, hipEventCreateWithFlags(&d.dev_event, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(d.dev_event, static_cast<hipStream_t>(stream)));
    HIPCHK(c, hipStreamWaitEvent(c->stream, d.dev_event, 0));
    return L3D_OK;
}

const char* memory_kind(hipMemoryType t)
{
    switch (t) {
    case hipMemoryTypeHost: return "pinned host memory";
    case hipMemoryTypeManaged: return "managed memory";
    case hipMemoryTypeArray: return "an array";
    case hipMemoryTypeUnified: return "unified memory";
    default: return "unregistered host memory";
    }
}

int extent_of(const l3d_device_image& im, long long* lo_out, long long* hi_out)
{
    using i128 = __int128;
    const i128 lim = (i128)kExtentLimit;
    i128 lo = 0, hi = 0;
    auto span = [&](long long n, long long stride) {        // offsets 0 .. n * stride
        const i128 p = (i128)n * stride;
        if (p > lim || p < -lim) return false;
        if (p < 0) lo += p; else hi += p;
        return true;
    };
    if (!span(im.height - 1, im.stride_y) || !span(im.width - 1, im.stride_x)) return L3D_ERR_UNSUPPORTED;
    i128 cmin = 0, cmax = 0;
    if (im.channels != 1)
        for (int k = 0; k < 3; ++k) {
            const i128 p = (i128)im.chan[k] * im.stride_c;
            if (p > lim || p < -lim) return L3D_ERR_UNSUPPORTED;
            if (k == 0 || p < cmin) cmin = p;
            if (k == 0 || p > cmax) cmax = p;
        }
    const int es = elem_bytes(im.dtype);
    lo = (lo + cmin) * es;
    hi = (hi + cmax + 1) * es;
    if (lo < -lim || hi > lim) return L3D_ERR_UNSUPPORTED;
    if ((long long)im.width * im.height * 3 > (1ll << 31)) return L3D_ERR_UNSUPPORTED;
    *lo_out = (long long)lo; *hi_out = (long long)hi;
    return L3D_OK;
}

}  // namespace

int device_image_check(const l3d_device_image& im, std::string& err)
{
    if (im.width < 1 || im.height < 1) { err = "device image: needs a size of at least 1x1"; return L3D_ERR_INVALID; }
    if (im.channels != 1 && im.channels != 3 && im.channels != 4) { err = "device image: channels must be 1, 3 or 4"; return L3D_ERR_INVALID; }
    if (im.dtype != L3D_U8 && im.dtype != L3D_U16 && im.dtype != L3D_F16 && im.dtype != L3D_F32) { err = "device image: unknown dtype (L3D_U8, L3D_U16, L3D_F16, L3D_F32)"; return L3D_ERR_INVALID; }
    if (im.channels != 1)
        for (int k = 0; k < 3; ++k)
            if (im.chan[k] < 0 || im.chan[k] >= im.channels) { err = "device image: every chan entry must be a channel of the source"; return L3D_ERR_INVALID; }
    if (im.dtype != L3D_U8 && !std::isfinite(im.scale)) { err = "device image: scale must be finite"; return L3D_ERR_INVALID; }
    return L3D_OK;
}

int device_image_pointer(l3d_ctx* c, const l3d_device_image& im, std::string& err)
{
    if (int rc = device_image_check(im, err)) return rc;
    long long lo = 0, hi = 0;
    if (int rc = extent_of(im, &lo, &hi)) { err = "device image: the strides or the size leave the supported range"; return rc; }
    if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); err = "device image: the context's device cannot be selected"; return L3D_ERR_HIP; }
    hipPointerAttribute_t attr;
    if (!im.ptr || hipPointerGetAttributes(&attr, im.ptr) != hipSuccess) {
        (void)hipGetLastError();
        err = "device image: not device memory (the runtime does not know the pointer)";
        return L3D_ERR_INVALID;
    }
    if (attr.type != hipMemoryTypeDevice) { err = std::string("device image: not device memory (") + memory_kind(attr.type) + ")"; return L3D_ERR_INVALID; }
    if (attr.device != c->device) {
        err = "device image: the memory is on device " + std::to_string(attr.device) + ", the context runs on device " + std::to_string(c->device);
        return L3D_ERR_INVALID;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(im.ptr)) != hipSuccess || !base) { (void)hipGetLastError(); return L3D_OK; }      // no range known: skipped
    const long long before = (long long)(static_cast<const char*>(im.ptr) - static_cast<const char*>(base));
    if (before + lo < 0 || (unsigned long long)(before + hi) > size) {
        err = "device image: addresses bytes " + std::to_string(before + lo) + " .. " + std::to_string(before + hi) + " of an allocation of " + std::to_string(size) + " bytes";
        return L3D_ERR_INVALID;
    }
    return L3D_OK;
}

int device_ingest(l3d_ctx* c, const l3d_device_image* const* images, int B, int w, int h, int ch, unsigned char* dst)
{
    DetectBufs& d = c->det;
    d.ingest_host.resize((size_t)B * sizeof(DevDesc));
    DevDesc* tab = reinterpret_cast<DevDesc*>(d.ingest_host.data());
    void* waited = nullptr;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (!images[b]) { tab[b] = DevDesc{}; continue; }
        tab[b] = make_desc(*images[b]);
        if (!any || images[b]->stream != waited) { if (int rc = wait_for_stream(c, images[b]->stream)) return rc; }
        waited = images[b]->stream; any = true;
    }
    if (!any) return L3D_OK;
    HIPCHK(c, d.ingest.reserve((size_t)B * sizeof(DevDesc)));
    HIPCHK(c, hipMemcpyAsync(d.ingest.p, tab, (size_t)B * sizeof(DevDesc), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "k_det_ingest");
        hipLaunchKernelGGL(k_det_ingest, dim3((unsigned)((work_items(w, h, ch) + 255) / 256), B), dim3(256), 0, c->stream, d.ingest.as<DevDesc>(), w, h, ch, dst);
    }
    HIPCHK(c, hipGetLastError());
    return L3D_OK;
}

int device_egress(l3d_ctx* c, const unsigned char* src, const l3d_device_image& out)
{
    const int ch = device_image_det_channels(out.channels);
    if (int rc = wait_for_stream(c, out.stream)) return rc;
    {
        ProfScope ps(c, "k_det_egress");
        hipLaunchKernelGGL(k_det_egress, dim3((unsigned)((std::max((long long)out.width * out.height, work_items(out.width, out.height, ch)) + 255) / 256)), dim3(256), 0, c->stream, src, out.width, out.height, ch, make_desc(out));
    }
    HIPCHK(c, hipGetLastError());
    return L3D_OK;
}

}  // namespace l3d

int l3d_device_image_check(const l3d_device_image* image, char* msg, size_t n)
{
    std::string err;
    const int rc = image ? l3d::device_image_check(*image, err) : L3D_ERR_INVALID;
    if (!image) err = "device image: null argument";
    if (msg && n) snprintf(msg, n, "%s", err.c_str());
    return rc;
}

int l3d_device_image_extent(const l3d_device_image* image, long long* lo, long long* hi)
{
    if (!image || !lo || !hi) return L3D_ERR_INVALID;
    std::string err;
    if (int rc = l3d::device_image_check(*image, err)) return rc;
    return l3d::extent_of(*image, lo, hi);
}

int l3d_test_device_image_pointer(l3d_ctx* c, const l3d_device_image* image)
{
    if (!c) return L3D_ERR_INVALID;
    if (!image) return l3d::fail(c, L3D_ERR_INVALID, "device image: null argument");
    std::string err;
    const int rc = l3d::device_image_pointer(c, *image, err);
    return rc == L3D_OK ? rc : l3d::fail(c, rc, err);
}

int l3d_test_device_ingest(l3d_ctx* c, const l3d_device_image* images, int n, unsigned char* out)
{
    using namespace l3d;
    if (!c) return L3D_ERR_INVALID;
    if (!images || !out || n < 1) return fail(c, L3D_ERR_INVALID, "test_device_ingest: null argument");
    const int w = images[0].width, h = images[0].height, ch = device_image_det_channels(images[0].channels);
    std::vector<const l3d_device_image*> list((size_t)n);
    for (int i = 0; i < n; ++i) {
        std::string err;
        if (int rc = device_image_pointer(c, images[i], err)) return fail(c, rc, "image " + std::to_string(i) + ": " + err);
        if (images[i].width != w || images[i].height != h || device_image_det_channels(images[i].channels) != ch)
            return fail(c, L3D_ERR_INVALID, "test_device_ingest: the images of a chunk have one size and one detector channel count");
        list[i] = &images[i];
    }
    const size_t bytes = (size_t)n * w * h * ch;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->det.pixels.reserve(bytes));
    if (int rc = device_ingest(c, list.data(), n, w, h, ch, c->det.pixels.as<unsigned char>())) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->det.pixels.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return L3D_OK;
}

int l3d_decode_jpeg_device(l3d_ctx* c, const unsigned char* bytes, size_t n, const l3d_device_image* out)
{
    using namespace l3d;
    if (!c) return L3D_ERR_INVALID;
    if (!bytes || !out) return fail(c, L3D_ERR_INVALID, "decode_jpeg: null argument");
    JpegFrame f;
    std::string err;
    if (int rc = jpeg_parse(bytes, n, f, err)) return fail(c, rc, err);
    if (int rc = device_image_check(*out, err)) return fail(c, rc, err);
    if (out->width != f.width || out->height != f.height || device_image_det_channels(out->channels) != f.ncomp)
        return fail(c, L3D_ERR_INVALID, "decode_jpeg: the output is " + std::to_string(out->width) + "x" + std::to_string(out->height) + " with " +
                                            std::to_string(device_image_det_channels(out->channels)) + " channels, the file " + std::to_string(f.width) + "x" +
                                            std::to_string(f.height) + " with " + std::to_string(f.ncomp));
    if (int rc = device_image_pointer(c, *out, err)) return fail(c, rc, err);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->det.pixels.reserve((size_t)f.width * f.ncomp * f.height));
    JpegStaged file;
    file.bytes = bytes; file.n = n; file.f = &f;
    JpegStaged* files[1] = { &file };
    if (int rc = jpeg_stage_files(c, files, 1)) return rc;
    if (file.status != L3D_OK) return fail(c, file.status, file.err);
    if (int rc = jpeg_staged_to_pixels(c, files, 1)) return rc;
    if (int rc = device_egress(c, c->det.pixels.as<unsigned char>(), *out)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return L3D_OK;
}
