// l3d_detect.hpp -- the line segment detector in front of addImage (l3d_detect.hip): 8-bit pixels in, the segments
// Line3D::detectLineSegments would hand to the view out (length filter, longest first, capped), in original-image pixels.
#pragma once

#include <cstddef>
#include <vector>

struct l3d_ctx;

namespace l3d {

// the camera of an undistortion (include/line3d_amd.h): focal lengths, principal point, OpenCV-convention radial coefficients
struct DetCamera { double fx, fy, cx, cy, k1, k2; };

// pixels: host, `channels` (1 or 3) interleaved bytes per pixel, rows `row_stride` bytes apart.  out: 4 floats per segment.
int detect_segments(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                    float min_length, int max_segments, std::vector<float>& out, const DetCamera* cam = nullptr);
// cam: null = the pixels as they are; otherwise they are undistorted on the device between the upload and the rescale

// host in, host out, same size and channels; coefficients at or below 1e-12: the pixels are copied
int undistort_image(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const DetCamera& cam, unsigned char* out,
                    size_t out_row_stride);

// ---- JPEG input (l3d_jpeg.cpp, l3d_jpeg_device.hip): baseline files decoded into the detector's pixel buffer; three components come out B, G, R
struct JpegFrame;
// f: the parsed headers of `bytes`.  Entropy decoding on the host, inverse DCT, upsampling and colour on the device, into DetectBufs::pixels
// (reserved by the caller); returns with the work enqueued on the context's stream
int jpeg_decode_to_pixels(l3d_ctx* c, const unsigned char* bytes, size_t n, const JpegFrame& f);
// host bytes in, host pixels out (height rows of width x channels bytes), any size from 1x1
int decode_jpeg(l3d_ctx* c, const unsigned char* bytes, size_t n, unsigned char* out, size_t out_row_stride);
// detect_segments on the decoded image, which never crosses the host; images below 8x8 are refused as detect_segments refuses them
int detect_segments_jpeg(l3d_ctx* c, const unsigned char* bytes, size_t n, int new_width, int new_height, float min_length, int max_segments,
                         std::vector<float>& out, const DetCamera* cam = nullptr);

}  // namespace l3d
