"""The C++ facade's overlay methods (include/line3D_amd.hpp: Line3D::projectResult, overlayView, overlayViewDevice, drawSegments, L3D::OverlayStyle)
compile against a dummy image type with a cv::Mat's members, the plain-C header compiles as C with the new structs, the library exports the new
symbols, and the Python mirror of l3d_overlay_style and l3d_camera has the header's layout."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("l3d_project_lines", "l3d_project_lines_device", "l3d_test_project_lines_host", "l3d_project_last_error", "l3d_draw_segments",
               "l3d_draw_segments_device", "l3d_test_draw_segments_host", "l3d_draw_last_error", "l3d_default_palette", "l3d_line3d_project_result",
               "l3d_line3d_overlay", "l3d_line3d_overlay_device")


def test_facade_compiles(tmp_path):
    src = tmp_path / "facade_overlay.cpp"
    src.write_text('''#include "line3D_amd.hpp"
struct Mat { unsigned char* data; size_t step; int cols, rows; int channels() const { return 3; } };
int use(L3D::Line3D& l, Mat& image, const l3d_device_image& dev)
{
    L3D::OverlayStyle style;
    style.width_model = 3.0; style.select = L3D_SELECT_ALL; style.layers = L3D_LAYER_MODEL;
    const bool a = l.overlayView(7u, image, style);
    const bool b = l.overlayViewDevice(7u, dev, L3D::OverlayStyle());
    std::vector<unsigned int> ids = { 1u, 2u };
    L3D::Line3D::Projection p = l.projectResult(ids);
    L3D::Line3D::Projection q = l.projectResult(ids, L3D_SELECT_OBSERVED, 1e-3, 2.0);
    std::vector<L3D::float4> segs = p.segments;
    std::vector<std::array<unsigned char, 4> > colours = { { { 255, 0, 0, 255 } }, { { 0, 255, 0, 128 } } };
    const bool c = l.drawSegments(image, segs, colours, 2.5);
    const bool d = l.drawSegments(image, segs, colours);
    return (a ? 1 : 0) + (b ? 2 : 0) + (c ? 4 : 0) + (d ? 8 : 0) + (int)q.camStart.size() + (int)q.flags.size() + (int)q.lineIndex.size() + (int)q.segIndex.size();
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_symbols_are_exported():
    from line3d_amd import capi
    lib = capi.load_library()
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    names = lib.l3d_profile_names().decode().split(";")
    for k in ("proj_count", "proj_scan", "proj_write", "draw_pieces", "draw_scan", "draw_cover", "draw_resolve"):
        assert k in names, k


def test_struct_layouts_and_the_palette(tmp_path):
    from line3d_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "line3d_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(l3d_camera), offsetof(l3d_camera, t), offsetof(l3d_camera, width),\n'
                   '  sizeof(l3d_overlay_style), offsetof(l3d_overlay_style, width_members), offsetof(l3d_overlay_style, near_z),\n'
                   '  offsetof(l3d_overlay_style, color_model), offsetof(l3d_overlay_style, palette), offsetof(l3d_overlay_style, n_palette)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    S, K = capi.OverlayStyle, capi.Camera
    assert got == [C.sizeof(K), K.t.offset, K.width.offset, C.sizeof(S), S.width_members.offset, S.near_z.offset, S.color_model.offset, S.palette.offset, S.n_palette.offset], got
    pal = capi.default_palette()
    assert pal.shape == (12, 4) and pal[0].tolist() == [230, 25, 75, 255] and pal[11].tolist() == [170, 110, 40, 255] and (pal[:, 3] == 255).all()
    assert len({tuple(p) for p in pal.tolist()}) == 12
