"""The device forms of include/line3D_amd.hpp (addImageDevice ..., makeDeviceEntry, addImagesDevice, decodeJPEGDevice, undistortImageDevice) compile
with plain g++ against a GpuMat-shaped type and an l3d_device_image, and link.  Nothing here needs a device: without one every call reports and
returns, and no pointer is ever followed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "line3D_amd.hpp"
struct Mat3 { double m[9]; double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
// the members of cv::cuda::GpuMat the facade reads
struct GpuMat { unsigned char* data; size_t step; int cols, rows; int ch; int channels() const { return ch; } };
int main() {
    L3D::Line3D l("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false);
    std::list<unsigned int> wps{ 1, 2, 3 };
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    Mat3 Km{ { 1, 0, 0, 0, 1, 0, 0, 0, 1 } };
    Vec3 tm{ { 0, 0, 0 } };
    GpuMat g{ nullptr, 1024, 320, 200, 3 };
    const l3d_device_image d = L3D::Line3D::deviceImage(g, nullptr);
    if (d.width != 320 || d.height != 200 || d.channels != 3 || d.dtype != L3D_U8 || d.stride_y != 1024 || d.stride_x != 3 || d.stride_c != 1 || d.scale != 1.0f) return 2;
    l3d_device_image planar = d;
    planar.dtype = L3D_F32; planar.stride_y = 320; planar.stride_x = 1; planar.stride_c = 64000; planar.scale = 255.0f;
    l.addImageDevice(0, g, Km, Km, tm, wps);
    l.addImageDevice(1, planar, Km, Km, tm, wps, 1920, false);
    l.addImageDeviceDistorted(2, g, Km, Km, tm, -0.2, 0.03, wps);
    l.addImage_fixed_simDevice(3, g, Km, Km, tm, sim);
    l.addImage_fixed_simDeviceDistorted(4, planar, Km, Km, tm, -0.2, 0.03, sim, 800, false);
    std::vector<L3D::Line3D::DeviceEntry> entries;
    entries.push_back(L3D::Line3D::makeDeviceEntry(5, g, Km, Km, tm, wps));
    entries.push_back(L3D::Line3D::makeDeviceEntry(6, g, Km, Km, tm, sim, (void*)nullptr).distorted(-0.2, 0.03));
    entries.push_back(L3D::Line3D::makeDeviceEntry(7, planar, Km, Km, tm, wps));
    const std::vector<int> st = l.addImagesDevice(entries, 1920, false);
    const unsigned char none[4] = { 0, 0, 0, 0 };
    const bool a = l.decodeJPEGDevice(none, sizeof(none), d), b = l.undistortImageDevice(d, Km, -0.2, 0.03, d);
    return (st.size() == 3 && !a && !b && l.numCameras() == 0) ? 0 : 1;
}
'''


def test_device_forms_compile_and_link(tmp_path):
    lib = os.path.join(ROOT, "line3d_amd")
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", exe])
    import torch
    if not torch.cuda.is_available():           # with a device the null pointers above would be refused one by one as well, but the test is about compiling
        assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 0
