// l3d_detect.hpp -- the line segment detector in front of addImage (l3d_detect.hip): 8-bit pixels in, the segments
// Line3D::detectLineSegments would hand to the view out (length filter, longest first, capped), in original-image pixels.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include "l3d_undistort.hpp"

struct l3d_ctx;
struct l3d_device_image;

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

// ---- many images in one call.  An entry is host pixels, or (pixels null) a baseline JPEG file, or (both null) an image in device memory
struct DetEntry {
    const unsigned char* pixels = nullptr;
    int width = 0, height = 0, channels = 0;
    size_t row_stride = 0;
    const unsigned char* jpeg = nullptr;
    size_t jpeg_bytes = 0;
    int new_width = 0, new_height = 0;
    float min_length = 0.0f;
    int max_segments = 0;
    const l3d_device_image* dev = nullptr;      // a third source (pixels and jpeg null): an image in device memory (l3d_device_image.hip)
    DetWarp warp;                               // nothing: the pixels as they are; otherwise they are undistorted on the device between the upload and the
                                                // rescale.  Checked per entry (warp_check)
};
// out[i]: the segments entry i gives alone, byte for byte.  Entries with the same sizes run together, in chunks (option det_batch_images, the index
// widths, half of the free HBM).  status[i] / message[i]: what the single call would have returned and said -- a refused entry fails alone.  The
// return value is L3D_OK, or a device failure's code (entries not finished by then carry it)
int detect_segments_batch(l3d_ctx* c, const DetEntry* e, int n, std::vector<std::vector<float>>& out, std::vector<int>& status, std::vector<std::string>& message);
// one image: a batch of one, its outcome the call's (a refusal's message is the context's last error).  out: 4 floats per segment.  An image below 8x8
// is refused whatever its source
int detect_one(l3d_ctx* c, const DetEntry& e, std::vector<float>& out);

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

}  // namespace l3d
