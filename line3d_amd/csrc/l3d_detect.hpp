// l3d_detect.hpp -- the line segment detector in front of addImage (l3d_detect.hip): 8-bit pixels in, the segments
// Line3D::detectLineSegments would hand to the view out (length filter, longest first, capped), in original-image pixels.
#pragma once

#include <cstddef>
#include <vector>

struct l3d_ctx;

namespace l3d {

// pixels: host, `channels` (1 or 3) interleaved bytes per pixel, rows `row_stride` bytes apart.  out: 4 floats per segment.
int detect_segments(l3d_ctx* c, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                    float min_length, int max_segments, std::vector<float>& out);

}  // namespace l3d
