"""Images in batches, the parts that need no GPU: the new symbols, the facade's addImages / makeEntry against stand-in image and matrix types, the
refusal of malformed entries before any device call, and the host's concurrent entropy decode (l3d_jpeg_batch.cpp) against the serial one under the
address and undefined-behaviour sanitizers -- a stand-alone program; nothing loaded into Python runs under a sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest

from line3d_amd import capi
from line3d_amd import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line3d_amd", "csrc")
SYMBOLS = ["l3d_detect_segments_batch", "l3d_line3d_add_images"]


@pytest.fixture(scope="module")
def jpeg():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "jpeg_ref.npz")))


def test_header_declares_and_library_exports_the_calls():
    header = open(os.path.join(ROOT, "include", "line3d_amd.h")).read()
    lib = capi.load_library()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert hasattr(lib, s), s
    for phrase in ("typedef struct l3d_detect_entry", "typedef struct l3d_image_entry", "L3D_DET_BATCH_IMAGES", "image <id>: <message>"):
        assert phrase in header, phrase
    assert "L3D_DET_BATCH_IMAGES" in open(os.path.join(CSRC, "l3d_options.hpp")).read()
    # the structures of capi.py are the header's: same fields in the same order
    for struct, cls in (("l3d_detect_entry", capi.DetectEntry), ("l3d_image_entry", capi.ImageEntry)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)\s*[,;]", body)
        fields = [f[0] for f in cls._fields_]
        assert names == fields, (names, fields)


FACADE_SRC = r'''
#include "line3D_amd.hpp"
struct Mat3 { double m[9]; double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Image { int cols, rows; unsigned char* data; size_t step; int channels() const { return 1; } };
int main() {
    std::vector<unsigned char> px(64 * 48, 128), file{ 0xFF, 0xD8, 0xFF, 0xD9 };
    Image img{ 64, 48, px.data(), 64 };
    L3D::Line3D l("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false);
    std::list<unsigned int> wps{ 1, 2, 3 };
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    Mat3 Km{ { 500, 0, 32, 0, 500, 24, 0, 0, 1 } };
    Vec3 tm{ { 0, 0, 0 } };
    std::vector<L3D::Line3D::ImageEntry> entries;
    entries.push_back(L3D::Line3D::makeEntry(0, img, Km, Km, tm, wps));
    entries.push_back(L3D::Line3D::makeEntry(1, img, Km, Km, tm, sim).distorted(-0.1, 0.01));
    entries.push_back(L3D::Line3D::makeEntry(2, file.data(), file.size(), Km, Km, tm, wps));
    entries.push_back(L3D::Line3D::makeEntry(3, file.data(), file.size(), Km, Km, tm, sim).distorted(-0.1, 0.0));
    if (entries[0].link_ids.size() != 3 || entries[0].fixed_sim || !entries[1].fixed_sim || entries[1].sims.size() != 2 || !entries[1].has_dist) return 1;
    if (entries[2].jpeg != file.data() || entries[2].pixels || entries[0].step != 64 || entries[0].K[2] != 32) return 1;
    const std::vector<int> status = l.addImages(entries);
    const std::vector<int> none = l.addImages(std::vector<L3D::Line3D::ImageEntry>(), 800, false);
    if (status.size() != 4 || !none.empty()) return 1;
    if (status[2] == 0 || status[3] == 0) return 1;          // four bytes are no JPEG file: refused from the headers, with or without a device
    return l.numCameras() == 0 ? 0 : 1;                      // (a flat image has no segments; without a GPU every entry reports and returns)
}
'''


def test_facade_add_images_compiles_and_links(tmp_path):
    lib = os.path.join(ROOT, "line3d_amd")
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(FACADE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    if "no usable HIP device" not in r.stderr:
        assert "image 2: jpeg" in r.stderr and "image 3: jpeg" in r.stderr


def test_malformed_entries_are_refused_before_any_device_call(jpeg):
    img, data = np.zeros((48, 64), np.uint8), jpeg["17x9_420/bytes"].tobytes()
    K, R, t = np.eye(3), np.eye(3), np.zeros(3)
    good = dict(imageID=0, img=img, K=K, R=R, t=t, worldpointIDs=[1, 2])
    arr, keep = pipeline.image_entries([good, dict(imageID=1, data=data, K=K, R=R, t=t, viewSimilarity={3: 0.5, 2: 0.25}, dist=(-0.1, 0.0))])
    assert (arr[0].width, arr[0].height, arr[0].channels, arr[0].row_stride, arr[0].n_links, arr[0].sims, arr[0].jpeg) == (64, 48, 1, 64, 2, None, None)
    assert arr[1].pixels is None and arr[1].jpeg_bytes == len(data) and arr[1].n_links == 2 and arr[1].sims and arr[1].dist
    for bad, exc in ((dict(good, data=data), ValueError), ({k: v for k, v in good.items() if k != "img"}, ValueError),
                     (dict(good, img=img.astype(np.float32)), TypeError), (dict(good, viewSimilarity={1: 0.5}), ValueError),
                     ({k: v for k, v in good.items() if k != "worldpointIDs"}, ValueError), (dict(good, img=None, data="a.jpg"), TypeError),
                     (dict(good, worldpointIDs=[[1, 2], [3, 4]]), ValueError), (dict(good, n_links=3), ValueError)):
        with pytest.raises(exc):
            pipeline.image_entries([good, bad])
    entries, keep = capi.detect_entries([img, data], new_sizes=[(32, 24), None], cameras=[None, (1, 1, 0, 0, -0.1, 0)])
    assert (entries[0].new_width, entries[0].new_height, entries[1].new_width, entries[1].new_height) == (32, 24, 17, 9)
    assert entries[0].camera is None and entries[1].camera and entries[1].pixels is None and entries[1].jpeg_bytes == len(data)
    assert abs(entries[0].min_length - 0.005 * np.hypot(64, 48)) < 1e-5
    for args, exc in ((([img.astype(np.int16)],), TypeError), ((["a.jpg"],), TypeError), (([img], [(8, 8), (9, 9)]), ValueError),
                      (([img], None, None, 3000, [(1, 2, 3)]), ValueError), (([img, img], None, [1.0]), ValueError), (([img], None, None, [1, 2]), ValueError)):
        with pytest.raises(exc):
            capi.detect_entries(*args)


def _batch_program(tmp_path, sanitize, jpeg):
    exe = tmp_path / ("jpeg_batch_" + sanitize[0].split("=")[1].split(",")[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror"] + sanitize +
                          [os.path.join(ROOT, "tests", "cpp", "jpeg_batch_main.cpp"), os.path.join(CSRC, "l3d_jpeg.cpp"), os.path.join(CSRC, "l3d_jpeg_batch.cpp"), "-o", str(exe)])
    paths = []
    names = [str(n) for n in jpeg["names"]] + [str(n) for n in jpeg["refusals"]]
    for n in names:
        p = tmp_path / (n.replace("/", "_") + ".jpg")
        p.write_bytes(jpeg[n + "/bytes"].tobytes())
        paths.append(str(p))
    for n, part in (("view2", 0.5), ("restart_blocks1", 0.8), ("37x29_420", 0.9)):          # whole headers, the entropy-coded data cut short
        b = jpeg[n + "/bytes"].tobytes()
        p = tmp_path / ("cut_%s.jpg" % n)
        p.write_bytes(b[:int(len(b) * part)])
        paths.append(str(p))
    return exe, paths, len(names)


def test_concurrent_decode_equals_serial_under_sanitizers(tmp_path, jpeg):
    """tests/cpp/jpeg_batch_main.cpp from the host-only sources with the address and undefined-behaviour sanitizers (runtimes linked into the program):
    the fixture's files, its two refusals and three truncated files on 1, 2 and 8 threads; every coefficient buffer, status and message equals the
    serial decode's"""
    exe, paths, n_fixture = _batch_program(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover", "-static-libasan", "-static-libubsan"], jpeg)
    r = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.match(r"files (\d+) decoded (\d+) failed (\d+) refused (\d+)", r.stdout)
    assert m and [int(g) for g in m.groups()] == [n_fixture + 3, n_fixture - 2, 3, 2]


def test_host_batch_decoder_compiles_alone(tmp_path):
    """plain C++17, no HIP header"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", os.path.join(CSRC, "l3d_jpeg_batch.cpp"), "-o", str(tmp_path / "b.o")])
    text = open(os.path.join(CSRC, "l3d_jpeg_batch.cpp")).read()
    assert "hip/" not in text and "l3d_ctx.hpp" not in text
