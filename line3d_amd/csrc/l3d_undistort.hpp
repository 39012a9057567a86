// l3d_undistort.hpp -- what happens to an image's pixels before the detector sees them (l3d_undistort.hip): radial k1, k2 coefficients, a lens, or a
// remap onto another camera and size with a validity plane (include/line3d_amd.h: "Undistortion on the device", "A LENS", "A REMAP").  One descriptor
// says what the caller gave, one check says which of the three kernels an image needs, and one body serves every single-image call.
#pragma once

#include <cstddef>
#include <string>

struct l3d_ctx;
struct l3d_device_image;
struct l3d_lens;
struct l3d_remap;

namespace l3d {

// the camera of an undistortion (include/line3d_amd.h): focal lengths, principal point, OpenCV-convention radial coefficients
struct DetCamera { double fx, fy, cx, cy, k1, k2; };
// a lens (include/line3d_amd.h, "A LENS": l3d_lens) together with the output camera it is resampled onto; model 0 in a chunk's table: no camera, the
// image is copied.  As make_lens leaves it the source camera may still be zero ("the output camera"); warp_check resolves that
struct DetLens { int model, pad; double fx, fy, cx, cy, ofx, ofy, ocx, ocy, k[8]; };
DetLens make_lens(const l3d_lens& lens, double ofx, double ofy, double ocx, double ocy);
// a k1, k2 camera as the lens that performs its operations (BROWN, the cameras equal): the place of such an image in a chunk that has lenses
DetLens lens_of_camera(const DetCamera& cam);

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
// an l3d_remap and the output camera as a DetRemap
DetRemap remap_of(const l3d_remap& m, double fx, double fy, double cx, double cy);

// what differs between the images of one chunk, on the device: the camera of k_det_undistort (on: the image is undistorted by it), the selection's
// filter and cap
struct DetImgParam { DetCamera cam; int cam_on; float min_length; int max_segments; int pad; };

// ---- the descriptor (DetWarp: what the caller gave) and what the check makes of it (WarpPlan).  The kernel an image needs, weakest first: a chunk
// runs the STRONGEST route any of its images needs, and a weaker image rides along with the same bytes -- Radial in a Lens or Resample chunk as
// lens_of_camera, None as model 0 (a copy).  That is WarpPlan::L
enum class WarpRoute { None = 0, Radial = 1, Lens = 2, Resample = 3 };     // nothing | k_det_undistort | k_det_undistort_lens | k_det_undistort_remap
constexpr int kRemapMask = 1, kRemapBorder = 2;                             // k_det_undistort_remap's flags per image
struct DetWarp {
    // what the caller gave: nothing, a k1, k2 camera, a lens, or a remap (more than one: refused by warp_check in the header's words)
    bool has_cam = false, has_lens = false, has_remap = false;
    DetCamera cam{ 1.0, 1.0, 0.0, 0.0, 0.0, 0.0 };
    DetLens lens{};                             // as make_lens gives it
    DetRemap remap;                             // its lens: as make_lens gives it
};
// a checked descriptor: all that the launches need
struct WarpPlan {
    WarpRoute route = WarpRoute::None;
    bool plane = false;                         // the image carries a validity plane: a mask, or a remap that resamples
    int flags = 0;                              // kRemapMask: `mask` holds a plane of the caller's; kRemapBorder: resampled with the border rule
    int out_w = 0, out_h = 0;                   // the size the detector sees
    DetCamera cam{ 1.0, 1.0, 0.0, 0.0, 0.0, 0.0 };      // Radial: k_det_undistort's camera
    DetLens L{};                                // the image's entry in a chunk's lens table, source camera resolved
    const void* mask = nullptr;                 // kRemapMask: the caller's mask in the source grid, its row stride, host or device memory
    size_t mask_stride = 0;
    bool mask_on_device = false;
};
// the refusals of the header that need no device, with its codes and strings, for an image of width x height x channels: L3D_OK with the plan, or
// the code with the cause in err (the plan then says None, no plane, the source's size).  Reclassified here: a remap that asks for nothing but its
// lens (no mask, border_mask 0, the source's size) is that lens alone -- its own kernel, no plane; coefficients or a lens that change nothing: None
int warp_check(const DetWarp& w, int width, int height, int channels, WarpPlan& plan, std::string& err);
// the descriptor of a batch entry: `camera` (NULL, or fx, fy, cx, cy, k1, k2) alone is the k1, k2 camera; beside a lens or a remap it is the output
// camera, and coefficients there leave both set, which warp_check refuses; a lens without a camera has no output camera (fx' = fy' = 0): refused too
DetWarp warp_of_entry(const double* camera, const l3d_lens* lens, const l3d_remap* remap);

// ---- the launches: d.pixels (B images, one after the other) -> d.undist, both reserved by the caller
// each image with its camera of `prm` (device; an image without one is copied), or all (B = 1) with `one` when prm is null
void launch_undistort(l3d_ctx* c, int w, int h, int ch, int B, const DetCamera& one, const DetImgParam* prm);
// with lenses: the B entries of `tab` (host; it has to live until the stream has been synchronised) go to d.lens, one launch follows
int launch_undistort_lens(l3d_ctx* c, int w, int h, int ch, int B, const DetLens* tab);
// w x h -> ow x oh and d.valid: `tab` and `flags` (host; they live until the stream has been synchronised) go to d.lens and d.rflags, one launch
// follows.  d.smask holds the masks of the images whose flag says so
int launch_undistort_remap(l3d_ctx* c, int w, int h, int ch, int ow, int oh, int B, const DetLens* tab, const int* flags);
// the caller's mask (kRemapMask) into slot b of d.smask (reserved by the caller for the chunk): a device mask is checked as an l3d_device_image is,
// before the copy
int remap_mask_upload(l3d_ctx* c, const WarpPlan& r, int w, int h, int b);
// the validity plane of an image that is NOT resampled, into slot b of d.valid (n = w x h bytes per slot, reserved by the caller): the caller's mask
// (already in slot b of d.smask) as 255 / 0, or all valid
int plane_without_resample(l3d_ctx* c, bool has_mask, size_t n, int b);

// ---- one image through its warp: the body of every l3d_undistort_image* call.  Host: pixels (width x height x channels, rows row_stride apart) to
// out and, where the caller wants the plane, valid.  Device (in set): in to dout and dvalid, which may be the memory of in.  Without a remap the
// output has the input's size; with one, the remap's output size.  A warp that changes nothing passes the pixels through: a host copy (in place:
// nothing), or ingest and egress alone
struct WarpIo {
    const unsigned char* pixels = nullptr;
    int width = 0, height = 0, channels = 0;
    size_t row_stride = 0;
    unsigned char* out = nullptr;
    size_t out_row_stride = 0;
    unsigned char* valid = nullptr;
    size_t valid_row_stride = 0;
    const l3d_device_image *in = nullptr, *dout = nullptr, *dvalid = nullptr;
};
int undistort_one(l3d_ctx* c, const WarpIo& io, const DetWarp& warp);

}  // namespace l3d
