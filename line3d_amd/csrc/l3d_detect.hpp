// l3d_detect.hpp -- the line segment detector in front of addImage (l3d_detect.hip): 8-bit pixels in, the segments
// Line3D::detectLineSegments would hand to the view out (length filter, longest first, capped), in original-image pixels.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

struct l3d_ctx;
struct l3d_device_image;
struct l3d_lens;

namespace l3d {

// ---- images in device memory (l3d_device_image.hip; the descriptor and its conversion rule: include/line3d_amd.h)
// the detector's channel count for a source: 1, or 3 for 3 and 4 channels
inline int device_image_det_channels(int source_channels) { return source_channels == 1 ? 1 : 3; }
// the fields (no device): L3D_OK, or the code with the cause in err
int device_image_check(const l3d_device_image& im, std::string& err);
// what comes before the first launch that touches im.ptr: device memory of the context's device, the extent inside its allocation.  Launches nothing
int device_image_pointer(l3d_ctx* c, const l3d_device_image& im, std::string& err);
// B images (checked by the two above, all w x h with ch detector channels; a null entry's slot is left alone) into B tight slots at dst (device):
// per image the context's stream waits for the image's stream, then ONE launch of k_det_ingest.  Returns with the work enqueued
int device_ingest(l3d_ctx* c, const l3d_device_image* const* images, int B, int w, int h, int ch, unsigned char* dst);
// the inverse for one image: tight 8-bit pixels at src (device) into the memory `out` describes (checked as above), after the context's stream
// waits for out's stream.  Returns with the work enqueued
int device_egress(l3d_ctx* c, const unsigned char* src, const l3d_device_image& out);

// the camera of an undistortion (include/line3d_amd.h): focal lengths, principal point, OpenCV-convention radial coefficients
struct DetCamera { double fx, fy, cx, cy, k1, k2; };
// a lens (include/line3d_amd.h, "A LENS": l3d_lens) together with the output camera it is resampled onto; model 0 in a chunk's table: no camera, the
// image is copied.  As make_lens leaves it the source camera may still be zero ("the output camera"); lens_check resolves that
struct DetLens { int model, pad; double fx, fy, cx, cy, ofx, ofy, ocx, ocy, k[8]; };
DetLens make_lens(const l3d_lens& lens, double ofx, double ofy, double ocx, double ocy);
// the refusals of the header (no device): L3D_OK with the source camera resolved and *active set (false: the pixels pass through), or the code with
// the cause in err
int lens_check(DetLens& lens, int width, int height, bool* active, std::string& err);

// ---- a remap (include/line3d_amd.h, "A REMAP"): the lens as make_lens gives it (has_lens false: none; model 0: a pinhole camera), the output size
// (0, 0: the source's), the caller's mask in the source grid
struct DetRemap {
    bool has_lens = false;
    DetLens lens{};
    int out_w = 0, out_h = 0;
    const void* mask = nullptr;
    size_t mask_stride = 0;
    int mask_w = 0, mask_h = 0;                 // the extent the caller states for the mask: it must be the source's
    bool mask_on_device = false, border_mask = true;
};

// pixels: host, `channels` (1 or 3) interleaved bytes per pixel, rows `row_stride` bytes apart.  out: 4 floats per segment.
int detect_segments(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                    float min_length, int max_segments, std::vector<float>& out, const DetCamera* cam = nullptr, const DetLens* lens = nullptr);
// cam, lens: both null = the pixels as they are; otherwise they are undistorted on the device between the upload and the rescale (both given: refused)

// ---- many images in one call.  An entry is host pixels, or (pixels null) a baseline JPEG file; cam as above
struct DetEntry {
    const unsigned char* pixels = nullptr;
    int width = 0, height = 0, channels = 0;
    size_t row_stride = 0;
    const unsigned char* jpeg = nullptr;
    size_t jpeg_bytes = 0;
    int new_width = 0, new_height = 0;
    float min_length = 0.0f;
    int max_segments = 0;
    const DetCamera* cam = nullptr;
    const DetLens* lens = nullptr;              // as make_lens gives it; checked per entry (lens_check)
    const l3d_device_image* dev = nullptr;      // a third source (pixels and jpeg null): an image in device memory (l3d_device_image.hip)
    const DetRemap* remap = nullptr;            // a remap (then cam and lens are null): the lens as make_lens gives it, checked per entry (remap_check)
};
// out[i]: the segments detect_segments / detect_segments_jpeg gives for entry i alone, byte for byte.  Entries with the same sizes run together, in
// chunks (option det_batch_images, the index widths, half of the free HBM).  status[i] / message[i]: what the single call would have returned and
// said -- a refused entry fails alone.  The return value is L3D_OK, or a device failure's code (entries not finished by then carry it)
int detect_segments_batch(l3d_ctx* c, const DetEntry* e, int n, std::vector<std::vector<float>>& out, std::vector<int>& status, std::vector<std::string>& message);

// detect_segments on an image in device memory (checked, ingested by k_det_ingest); an image below 8x8 is refused as detect_segments refuses it
int detect_segments_device(l3d_ctx* c, const l3d_device_image& image, int new_width, int new_height, float min_length, int max_segments, std::vector<float>& out,
                           const DetCamera* cam = nullptr, const DetLens* lens = nullptr);
// device in, device out (may be the same memory), same size and detector channels; coefficients at or below 1e-12: ingest and egress only.
// lens given: it stands in for cam, which is not looked at
int undistort_image_device(l3d_ctx* c, const l3d_device_image& in, const DetCamera& cam, const l3d_device_image& out, const DetLens* lens = nullptr);

// host in, host out, same size and channels; coefficients at or below 1e-12: the pixels are copied.  lens given: it stands in for cam
int undistort_image(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const DetCamera& cam, unsigned char* out,
                    size_t out_row_stride, const DetLens* lens = nullptr);

// ---- a remap's calls
// the refusals of the header that need no device: L3D_OK with the output size and the lens resolved and *active set (false: nothing is resampled)
int remap_check(DetRemap& r, int width, int height, int channels, bool* active, std::string& err);
// host in, host out (out_w x out_h); valid: null, or out_w x out_h bytes, 255 / 0
int undistort_image_remap(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const DetRemap& remap, unsigned char* out,
                          size_t out_row_stride, unsigned char* valid, size_t valid_row_stride);
// device in, device out; valid: null, or a one-channel image of the output size
int undistort_image_device_remap(l3d_ctx* c, const l3d_device_image& in, const DetRemap& remap, const l3d_device_image& out, const l3d_device_image* valid);

// ---- JPEG input (l3d_jpeg.cpp, l3d_jpeg_device.hip): baseline files decoded into the detector's pixel buffer; three components come out B, G, R
struct JpegFrame;
// a file on its way into DetectBufs::pixels: bytes and parsed headers in; where its quantisation tables and coefficients stand in the pinned
// staging buffer, and how its entropy decoding went, out
struct JpegStaged {
    const unsigned char* bytes = nullptr;
    size_t n = 0;
    const JpegFrame* f = nullptr;
    size_t stage_at = 0;
    int status = 0;
    std::string err;
};
// entropy decoding of n files on the host threads, each into its own slice of the staging buffer.  A file that fails says so in its status; the
// return value is a device failure's
int jpeg_stage_files(l3d_ctx* c, JpegStaged* const* files, int n);
// the staged files into their slots of DetectBufs::pixels (reserved by the caller; slot b = entry b of `files`, null: not a file, the slot is left
// alone; all of one size): one upload, then inverse DCT, upsampling and colour per file.  Returns with the work enqueued on the context's stream
int jpeg_staged_to_pixels(l3d_ctx* c, const JpegStaged* const* files, int B);
// host bytes in, host pixels out (height rows of width x channels bytes), any size from 1x1
int decode_jpeg(l3d_ctx* c, const unsigned char* bytes, size_t n, unsigned char* out, size_t out_row_stride);
// detect_segments on the decoded image, which never crosses the host; images below 8x8 are refused as detect_segments refuses them
int detect_segments_jpeg(l3d_ctx* c, const unsigned char* bytes, size_t n, int new_width, int new_height, float min_length, int max_segments,
                         std::vector<float>& out, const DetCamera* cam = nullptr, const DetLens* lens = nullptr);

}  // namespace l3d
