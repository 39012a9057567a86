"""The lens forms of include/line3D_amd.hpp (addImageLens, addImage_fixed_simLens, addImageJPEGLens, addImageDeviceLens, the lens member of ImageEntry
and DeviceEntry, undistortImage(image, K, lens)) compile with plain g++ against mock image types and link; the new symbols are in the header and in
the library.  Nothing here needs a device: without one every call reports and returns."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["l3d_undistort_image_lens", "l3d_undistort_image_device_lens", "l3d_detect_segments_batch_lens", "l3d_detect_segments_device_batch_lens",
           "l3d_line3d_add_image_entry_lens", "l3d_line3d_add_images_lens", "l3d_line3d_add_device_entry_lens", "l3d_line3d_add_device_images_lens",
           "l3d_line3d_undistort_image_lens", "l3d_sfm_read_colmap", "l3d_sfm_camera_lens", "l3d_sfm_camera_model", "l3d_sfm_camera_id"]

SRC = r'''
#include "line3D_amd.hpp"
struct Mat3 { double m[9]; double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
// the members of cv::Mat / cv::cuda::GpuMat the facade reads
struct Mat { unsigned char* data; size_t step; int cols, rows; int ch; int channels() const { return ch; } };
int main() {
    static_assert(L3D_LENS_BROWN == 1 && L3D_LENS_FISHEYE == 2, "lens models");
    L3D::Line3D l("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false);
    std::list<unsigned int> wps{ 1, 2, 3 };
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    Mat3 Km{ { 100, 0, 8, 0, 100, 8, 0, 0, 1 } };
    Vec3 tm{ { 0, 0, 0 } };
    std::vector<unsigned char> px(16 * 16 * 3, 0);
    Mat m{ px.data(), 48, 16, 16, 3 };
    l3d_lens brown = l3d_lens();
    brown.model = L3D_LENS_BROWN; brown.k[0] = -0.2; brown.k[2] = 0.01;
    l3d_lens fish = l3d_lens();
    fish.model = L3D_LENS_FISHEYE; fish.fx = fish.fy = 160; fish.cx = fish.cy = 8;
    l3d_lens zero = l3d_lens();                     // model 0: refused
    l.addImageLens(0, m, Km, Km, tm, brown, wps);
    l.addImage_fixed_simLens(1, m, Km, Km, tm, fish, sim, 800, false);
    const unsigned char none[4] = { 0, 0, 0, 0 };
    l.addImageJPEGLens(2, none, sizeof(none), Km, Km, tm, brown, wps);
    l.addImageJPEGLens(3, none, sizeof(none), Km, Km, tm, fish, sim, 1920, false);
    Mat g{ nullptr, 1024, 320, 200, 3 };
    l.addImageDeviceLens(4, g, Km, Km, tm, fish, wps);
    l.addImageDeviceLens(5, L3D::Line3D::deviceImage(g, nullptr), Km, Km, tm, brown, sim, 1920, false);
    std::vector<L3D::Line3D::ImageEntry> entries;
    entries.push_back(L3D::Line3D::makeEntry(6, m, Km, Km, tm, wps).withLens(brown));
    entries.push_back(L3D::Line3D::makeEntry(7, m, Km, Km, tm, sim));
    entries.push_back(L3D::Line3D::makeEntry(8, none, sizeof(none), Km, Km, tm, wps).withLens(fish).distorted(-0.1, 0.0));
    if (!entries[0].has_lens || entries[0].lens.model != L3D_LENS_BROWN || entries[1].has_lens) return 2;
    const std::vector<int> st = l.addImages(entries, 1920, false);
    std::vector<L3D::Line3D::DeviceEntry> dev;
    dev.push_back(L3D::Line3D::makeDeviceEntry(9, g, Km, Km, tm, wps).withLens(fish));
    dev.push_back(L3D::Line3D::makeDeviceEntry(10, g, Km, Km, tm, sim));
    if (!dev[0].base.has_lens || dev[0].base.lens.model != L3D_LENS_FISHEYE) return 2;
    const std::vector<int> sd = l.addImagesDevice(dev, 1920, false);
    const bool a = l.undistortImage(m, Km, zero);
    return (st.size() == 3 && sd.size() == 2 && !a && l.numCameras() == 0) ? 0 : 1;
}
'''


def test_lens_forms_compile_and_link(tmp_path):
    lib = os.path.join(ROOT, "line3d_amd")
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
    import torch
    if not torch.cuda.is_available():           # with a device the calls above would be refused one by one as well, but the test is about compiling
        assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 0


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "line3d_amd.h"\nint main(void) { l3d_lens l = { 0 }; return l.model + (int)sizeof(l.k) - 64 + L3D_LENS_BROWN - 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_symbols():
    with open(os.path.join(ROOT, "include", "line3d_amd.h")) as f:
        header = f.read()
    from line3d_amd import capi
    lib = capi.load_library()
    for s in SYMBOLS:
        assert ("int %s(" % s) in header, s
        assert getattr(lib, s) is not None, s
    assert "typedef struct l3d_lens {" in header and "L3D_LENS_BROWN = 1" in header and "L3D_LENS_FISHEYE = 2" in header
    assert ctypes.sizeof(capi.Lens) == 8 + 4 * 8 + 8 * 8
