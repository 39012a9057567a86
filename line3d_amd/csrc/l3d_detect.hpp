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

}  // namespace l3d
