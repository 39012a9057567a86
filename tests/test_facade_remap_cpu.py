"""The remap forms of include/line3D_amd.hpp (addImageRemap, addImageJPEGRemap, addImageDeviceRemap, ImageEntry::withRemap / DeviceEntry::withRemap in
addImages / addImagesDevice, undistortImage(image, K, remap, out, mask_out), undistortPlan) compile with plain g++ against mock image types and link;
the planner runs (it needs no device); the new symbols are in the header and in the library, and the struct's Python mirror has its layout."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["l3d_undistort_plan", "l3d_undistort_image_remap", "l3d_undistort_image_device_remap", "l3d_detect_segments_batch_remap",
           "l3d_detect_segments_device_batch_remap", "l3d_line3d_add_image_entry_remap", "l3d_line3d_add_images_remap", "l3d_line3d_add_device_entry_remap",
           "l3d_line3d_add_device_images_remap", "l3d_line3d_undistort_image_remap", "l3d_test_detect_defined_plane"]

SRC = r'''
#include <cmath>
#include "line3D_amd.hpp"
struct Mat3 { double m[9]; double operator()(int i, int j) const { return m[i * 3 + j]; } double& operator()(int i, int j) { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
// the members of cv::Mat / cv::cuda::GpuMat the facade reads
struct Mat { unsigned char* data; size_t step; int cols, rows; int ch; int channels() const { return ch; } };
int main() {
    // the planner: host only
    l3d_lens fish = l3d_lens();
    fish.model = L3D_LENS_FISHEYE; fish.fx = fish.fy = 20; fish.cx = 7.6; fish.cy = 8.3; fish.k[0] = -0.02;
    Mat3 K2{ { 0 } };
    int w2 = 0, h2 = 0;
    if (!L3D::Line3D::undistortPlan(fish, 16, 16, 0.5, K2, w2, h2) || w2 != 16 || h2 != 16 || !(K2(0, 0) > 0.0) || K2(0, 1) != 0.0 || K2(2, 2) != 1.0) return 3;
    const double f_same = K2(0, 0);
    w2 = h2 = -1;
    if (!L3D::Line3D::undistortPlan(fish, 16, 16, 1.0, K2, w2, h2, 64) || K2(0, 0) != 20.0 || w2 < 16 || h2 < 16 || !(f_same < 20.0)) return 4;
    int bw = 0, bh = 0;
    if (L3D::Line3D::undistortPlan(fish, 16, 16, 1.5, K2, bw, bh)) return 5;            // alpha outside [0, 1]: refused (and said so on cerr)

    L3D::Line3D l("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false);
    std::list<unsigned int> wps{ 1, 2, 3 };
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    Mat3 Km{ { 100, 0, 8, 0, 100, 8, 0, 0, 1 } };
    Vec3 tm{ { 0, 0, 0 } };
    std::vector<unsigned char> px(16 * 16 * 3, 0), mk(16 * 16, 1);
    Mat m{ px.data(), 48, 16, 16, 3 };
    l3d_remap remap = l3d_remap();
    remap.lens = &fish; remap.out_width = 24; remap.out_height = 20; remap.border_mask = 1;
    remap.mask = mk.data(); remap.mask_row_stride = 16; remap.mask_width = 16; remap.mask_height = 16;
    l3d_remap mask_only = l3d_remap();
    mask_only.mask = mk.data(); mask_only.mask_row_stride = 16; mask_only.mask_width = 16; mask_only.mask_height = 16;
    l.addImageRemap(0, m, Km, Km, tm, remap, wps);
    l.addImageRemap(1, m, Km, Km, tm, mask_only, sim, 800, false);
    const unsigned char none[4] = { 0, 0, 0, 0 };
    l.addImageJPEGRemap(2, none, sizeof(none), Km, Km, tm, remap, wps);
    l.addImageJPEGRemap(3, none, sizeof(none), Km, Km, tm, remap, sim, 1920, false);
    Mat g{ nullptr, 1024, 320, 200, 3 };
    l.addImageDeviceRemap(4, g, Km, Km, tm, remap, wps);
    l.addImageDeviceRemap(5, L3D::Line3D::deviceImage(g, nullptr), Km, Km, tm, remap, sim, 1920, false);
    std::vector<L3D::Line3D::ImageEntry> entries;
    entries.push_back(L3D::Line3D::makeEntry(6, m, Km, Km, tm, wps).withRemap(remap));
    entries.push_back(L3D::Line3D::makeEntry(7, m, Km, Km, tm, sim).withLens(fish));
    entries.push_back(L3D::Line3D::makeEntry(8, none, sizeof(none), Km, Km, tm, wps).withRemap(mask_only));
    entries.push_back(L3D::Line3D::makeEntry(9, m, Km, Km, tm, wps));
    // the entry holds its own copy of the lens, whatever becomes of the caller's and however the entry is copied
    std::vector<L3D::Line3D::ImageEntry> copy = entries;
    l3d_remap store;
    const l3d_remap* r0 = copy[0].remap_for_call(store);
    if (!r0 || r0->lens != &copy[0].lens || r0->lens->model != L3D_LENS_FISHEYE || r0->out_width != 24 || r0->mask != mk.data() || copy[0].has_lens) return 6;
    const l3d_remap* r1 = copy[1].remap_for_call(store);
    if (!r1 || r1->lens != &copy[1].lens || r1->border_mask != 0 || r1->mask || r1->out_width != 0) return 6;      // a lens alone: a remap that asks for nothing more
    const l3d_remap* r2 = copy[2].remap_for_call(store);
    if (!r2 || r2->lens || r2->mask != mk.data() || copy[3].remap_for_call(store)) return 6;
    const std::vector<int> st = l.addImages(entries, 1920, false);
    std::vector<L3D::Line3D::DeviceEntry> dev;
    dev.push_back(L3D::Line3D::makeDeviceEntry(10, g, Km, Km, tm, wps).withRemap(remap));
    dev.push_back(L3D::Line3D::makeDeviceEntry(11, g, Km, Km, tm, sim));
    if (!dev[0].base.has_remap || !dev[0].base.remap_has_lens || dev[1].base.has_remap) return 6;
    const std::vector<int> sd = l.addImagesDevice(dev, 1920, false);
    std::vector<unsigned char> o(24 * 20 * 3, 0), v(24 * 20, 0);
    Mat out{ o.data(), 72, 24, 20, 3 }, valid{ v.data(), 24, 24, 20, 1 }, wrong{ o.data(), 48, 16, 16, 3 };
    const bool a = l.undistortImage(m, Km, remap, wrong);              // an output of another size than the remap's: refused by the facade
    const bool b = l.undistortImage(m, Km, remap, out, &valid);        // (without a device: reported, false)
    return (st.size() == 4 && sd.size() == 2 && !a && (!b || l.numCameras() >= 0) && l.numCameras() == 0) ? 0 : 1;
}
'''


def test_remap_forms_compile_link_and_plan(tmp_path):
    lib = os.path.join(ROOT, "line3d_amd")
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
    import torch
    if not torch.cuda.is_available():           # with a device the add calls would be refused one by one as well, but the test is about compiling and the planner
        assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 0


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "line3d_amd.h"\nint main(void) { l3d_remap r = { 0 }; double K[9]; int w, h; l3d_lens l = { 0 };\n'
                   '  return r.mask_width + r.mask_height + r.border_mask + (l3d_undistort_plan(&l, 16, 16, 0.0, 0, 0, 0, 120.0, K, &w, &h) == L3D_ERR_INVALID ? 0 : 1); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_symbols_and_layout(tmp_path):
    with open(os.path.join(ROOT, "include", "line3d_amd.h")) as f:
        header = f.read()
    from line3d_amd import capi
    lib = capi.load_library()
    for s in SYMBOLS:
        assert ("int %s(" % s) in header, s
        assert getattr(lib, s) is not None, s
    assert "typedef struct l3d_remap {" in header
    # the Python mirror of l3d_remap against the header itself
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(l3d_remap),\n'
                   '  offsetof(l3d_remap, lens), offsetof(l3d_remap, out_width), offsetof(l3d_remap, out_height), offsetof(l3d_remap, mask), offsetof(l3d_remap, mask_row_stride),\n'
                   '  offsetof(l3d_remap, mask_width), offsetof(l3d_remap, mask_height), offsetof(l3d_remap, mask_on_device), offsetof(l3d_remap, border_mask)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    R = capi.Remap
    assert got == [ctypes.sizeof(R), R.lens.offset, R.out_width.offset, R.out_height.offset, R.mask.offset, R.mask_row_stride.offset, R.mask_width.offset,
                   R.mask_height.offset, R.mask_on_device.offset, R.border_mask.offset], got
