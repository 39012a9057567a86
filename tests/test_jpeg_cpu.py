"""The baseline JPEG decoder without a device: the numpy statement of the contract (tests/jpeg_model.py) against Pillow's pixels (tests/golden/jpeg_ref.npz),
the library's host half (l3d_jpeg.cpp: parser and entropy decoder) against the model, the refusals, the header / library / facade additions, and the
parser and entropy decoder over truncated and mutated files under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import jpeg_model as jm
from line3d_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_ref.npz")

_z = np.load(GOLDEN)
NAMES = [str(n) for n in _z["names"]]
REFUSALS = [str(n) for n in _z["refusals"]]
# every case of the issue's table is in the fixture (dqt16: Pillow decodes the rewritten file to the same pixels, so it is kept)
EXPECTED = {"8x8_grey", "16x16_420", "1x1_420", "17x9_420", "7x23_422", "37x29_444", "37x29_422", "37x29_420", "37x29_grey", "50x33_420", "264x24_444",
            "noise_q100", "noise_q5", "const0", "const255", "optimize", "restart_blocks1", "restart_rows1", "keep_rgb", "dqt16", "view0", "view1", "view2", "view3", "view4", "view5"}


def _case(name):
    return _z[name + "/bytes"].tobytes(), _z[name + "/pixels"]


def test_fixture_holds_every_case():
    assert set(NAMES) == EXPECTED and set(REFUSALS) == {"progressive", "cmyk"}
    assert os.path.getsize(GOLDEN) < 1 << 20
    lay = {n: jm.parse(_case(n)[0]) for n in NAMES}
    assert lay["restart_blocks1"]["restart_interval"] == 1 and lay["restart_rows1"]["restart_interval"] == lay["restart_rows1"]["mcux"]
    assert lay["keep_rgb"]["rgb"] == 1 and all(lay[n]["rgb"] == 0 for n in NAMES if n != "keep_rgb")
    assert (lay["37x29_444"]["hmax"], lay["37x29_444"]["vmax"]) == (1, 1) and (lay["37x29_422"]["hmax"], lay["37x29_422"]["vmax"]) == (2, 1)
    assert (lay["37x29_420"]["hmax"], lay["37x29_420"]["vmax"]) == (2, 2) and lay["37x29_grey"]["ncomp"] == 1
    assert sum(bw * bh for bw, bh, _, _ in lay["264x24_444"]["layout"]) == 3 * 99
    data = _case("dqt16")[0]
    at = data.index(b"\xff\xdb")
    assert data[at + 4] >> 4 == 1                                  # the first table is in 16-bit form
    assert _case("optimize")[0].count(b"\xff\xc4") >= 1 and len(_case("optimize")[0]) < len(_case("37x29_420")[0])


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_pillow(name):
    data, pixels = _case(name)
    got = jm.decode(data)
    assert got.shape == pixels.shape and got.dtype == np.uint8
    assert np.array_equal(got, pixels), "%d samples differ" % np.count_nonzero(got != pixels)


def test_fixture_rederived_where_pillow_is():
    """the fixture is what tests/golden/make_golden_jpeg.py writes with the Pillow that is here; a machine without Pillow has nothing to re-derive"""
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_jpeg as mg
    out = mg.build()
    assert sorted(str(n) for n in out["names"]) == sorted(NAMES)
    for key in _z.files:
        assert np.array_equal(out[key], _z[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_library_coefficients_and_info_equal_the_model(name):
    data, pixels = _case(name)
    f, coef = jm.coefficients(data)
    got, qt, layout = capi.test_jpeg_coefficients(data)
    assert got.shape == coef.shape and np.array_equal(got, coef)
    assert np.array_equal(qt[:f["ncomp"]], f["qt"]) and not qt[f["ncomp"]:].any()
    head = [f["width"], f["height"], f["ncomp"], f["hmax"], f["vmax"], f["mcux"], f["mcuy"], f["restart_interval"], f["rgb"]]
    assert layout[:9].tolist() == head
    for i, c in enumerate(f["comps"]):
        assert layout[9 + 6 * i:15 + 6 * i].tolist() == [c[1], c[2]] + list(f["layout"][i])
    assert capi.jpeg_info(data) == (pixels.shape[1], pixels.shape[0], 1 if pixels.ndim == 2 else 3)


def _sof_at(data):
    m = re.search(b"\xff[\xc0\xc1\xc2]", data)
    return m.start()


def _variants():
    """(name, bytes, status, a word of the message): the fixture's refusals and files made from good ones by rewriting header bytes"""
    good = _case("37x29_420")[0]
    sof = _sof_at(good)
    sos = good.index(b"\xff\xda")
    scan = jm.parse(good)["scan_offset"]

    def patch(at, value, src=good):
        b = bytearray(src)
        b[at] = value
        return bytes(b)
    out = [("progressive", _z["progressive/bytes"].tobytes(), 5, "progressive"), ("cmyk", _z["cmyk/bytes"].tobytes(), 5, "components"),
           ("lossless", patch(sof + 1, 0xC3), 5, "lossless"), ("arithmetic", patch(sof + 1, 0xC9), 5, "arithmetic"),
           ("12-bit", patch(sof + 4, 12), 5, "12-bit"), ("sampling 1x2", patch(sof + 11, 0x12), 5, "sampling"),
           ("sampling 4x1", patch(sof + 11, 0x41), 5, "sampling"), ("chroma 2x1", patch(sof + 14, 0x21), 5, "sampling"),
           ("zero width", patch(sof + 7, 0, patch(sof + 8, 0)), 1, "zero dimensions"), ("zero height", patch(sof + 5, 0, patch(sof + 6, 0)), 1, "zero dimensions"),
           ("no SOI", b"\x89PNG" + good[4:], 1, "SOI"), ("headers only", good[:scan - 20], 1, "truncated"),
           ("missing quantisation table", patch(sof + 12, 3), 1, "missing table"), ("missing Huffman table", patch(sos + 6, 0x33), 1, "missing table"),
           ("two components", patch(sof + 9, 2), 5, "components"),
           ("65535 x 65535", patch(sof + 5, 255, patch(sof + 6, 255, patch(sof + 7, 255, patch(sof + 8, 255)))), 5, "too large")]
    # a frame of 3 components whose scan carries one: more than one scan
    b = bytearray(good)
    b[sos + 2:sos + 4] = (8).to_bytes(2, "big")
    b[sos + 4] = 1
    del b[sos + 7:sos + 11]
    out.append(("several scans", bytes(b), 5, "scan"))
    return out


@pytest.mark.parametrize("case", _variants(), ids=lambda c: c[0])
def test_refusals_name_their_cause(case):
    name, data, code, word = case
    lib = capi.load_library()
    lib.l3d_jpeg_last_error.restype = C.c_char_p
    ptr, n = capi._bytes_arguments(data)
    w, h, ch = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.l3d_jpeg_info(ptr, n, C.byref(w), C.byref(h), C.byref(ch)) == code
    msg = lib.l3d_jpeg_last_error().decode()
    assert word in msg and msg.startswith("jpeg: "), msg
    with pytest.raises(capi.L3DError) as e:
        capi.test_jpeg_coefficients(data)
    assert e.value.code == code and word in str(e.value)
    with pytest.raises(jm.JpegError) as e:
        jm.coefficients(data)
    assert e.value.code == code
    good = _case("16x16_420")[0]                      # the next call is not affected, and clears the message
    assert capi.jpeg_info(good) == (16, 16, 3) and lib.l3d_jpeg_last_error() == b""


def _handmade(width, dc_symbol, ac_symbol, bits):
    """a grey baseline JPEG of `width` x 8 (one block per 8 columns, quantisation all ones) whose DC and AC Huffman tables hold ONE code each, the
    1-bit code "0", for `dc_symbol` and `ac_symbol`; `bits` (a string of 0 / 1, padded with ones to whole bytes, FF stuffed) is its
    entropy-coded data.  With it a stream can say exactly what a test wants it to say."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    dht = lambda cls, sym: seg(0xC4, bytes([cls << 4, 1] + [0] * 15 + [sym]))
    bits = bits + "1" * (-len(bits) % 8)
    data = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    return (b"\xff\xd8" + seg(0xDB, bytes([0] + [1] * 64)) + seg(0xC0, bytes([8, 0, 8]) + width.to_bytes(2, "big") + bytes([1, 1, 0x11, 0]))
            + dht(0, dc_symbol) + dht(1, ac_symbol) + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + data + b"\xff\xd9")


def _entropy_cases():
    data = _case("37x29_420")[0]
    scan = jm.parse(data)["scan_offset"]
    return [("cut in the scan", data[:scan + 40], "truncated"),
            ("a marker inside the scan", data[:scan + 40] + b"\xff\xd9" + data[scan + 42:], "truncated"),
            ("restart marker missing", _case("restart_blocks1")[0].replace(b"\xff\xd1", b"\x12\x34", 1), "restart"),
            # the standard tables have no code of sixteen ones
            ("all ones", data[:scan] + b"\xff\x00" * 200, "not in the table"),
            # the only DC code is "0": a first bit of 1 is no code
            ("handmade: a code that is not in the table", _handmade(8, 0, 0, "1" * 16), "not in the table"),
            # DC 0, then the AC symbol F1 (run 15, size 1) four times: indices 16, 32, 48 are written, the fourth lands on 64
            ("handmade: a coefficient index past 63", _handmade(8, 0, 0xF1, "0" + "01" * 4), "index past 63"),
            # two blocks whose DC differences are +32767 each (category 15, fifteen ones): the predictor reaches 65534
            ("handmade: a DC predictor past int16", _handmade(16, 15, 0x00, ("0" + "1" * 15 + "0") * 2), "DC predictor")]


@pytest.mark.parametrize("case", _entropy_cases(), ids=lambda c: c[0])
def test_entropy_errors(case):
    """damage behind the headers: the parser accepts, the entropy decoder returns L3D_ERR_INVALID and names the cause"""
    what, bad, word = case
    assert len(capi.jpeg_info(bad)) == 3                 # the headers are fine
    with pytest.raises(capi.L3DError) as e:
        capi.test_jpeg_coefficients(bad)
    assert e.value.code == 1 and word in str(e.value), (what, str(e.value))
    with pytest.raises(jm.JpegError) as e2:
        jm.coefficients(bad)
    assert e2.value.code == 1


def test_handmade_streams_are_streams():
    """the controls of the handmade cases: the same builder, one step short of each error, decodes -- in the library and in the model alike"""
    for data, expect in ((_handmade(8, 0, 0, "00"), {}),                                              # DC 0, end of block
                         (_handmade(8, 0, 0xF1, "0" + "01" * 3), None),                                 # three AC symbols (indices 16, 32, 48), then a bit that is no code
                         (_handmade(8, 15, 0x00, "0" + "1" * 15 + "0"), {0: 32767}),                    # one block: the predictor stays in range
                         (_handmade(16, 15, 0x00, "0" + "1" * 15 + "0" + "0" + "0" * 15 + "0"), {0: 32767, 64: 0})):   # +32767, then -32767
        if expect is None:
            with pytest.raises(capi.L3DError) as e:
                capi.test_jpeg_coefficients(data)
            assert e.value.code == 1 and "index past 63" not in str(e.value)
            continue
        got = capi.test_jpeg_coefficients(data)[0]
        assert np.array_equal(got, jm.coefficients(data)[1])
        want = np.zeros(got.size, np.int16)
        for k, v in expect.items():
            want[k] = v
        assert np.array_equal(got.ravel(), want)


def test_accepted_oddities():
    """fill bytes in front of a marker, a missing EOI and bytes after EOI are all accepted"""
    data = _case("37x29_420")[0]
    f, coef = jm.coefficients(data)
    sos = data.index(b"\xff\xda")
    for ok in (data[:sos] + b"\xff\xff\xff" + data[sos:], data[:-2], data + b"trailing bytes \xff\xd8\xff"):
        assert np.array_equal(capi.test_jpeg_coefficients(ok)[0], coef)
        assert np.array_equal(jm.coefficients(ok)[1], coef)


# ---- header, library, facade, example
SYMBOLS = ["l3d_jpeg_info", "l3d_jpeg_last_error", "l3d_decode_jpeg", "l3d_detect_segments_jpeg", "l3d_line3d_add_image_jpeg", "l3d_line3d_add_image_jpeg_fixed_sim",
           "l3d_line3d_decode_jpeg", "l3d_test_jpeg_coefficients"]


def test_header_declares_and_library_exports_the_calls():
    header = open(os.path.join(ROOT, "include", "line3d_amd.h")).read()
    lib = capi.load_library()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert hasattr(lib, s), s
    for phrase in ("B, G, R INTERLEAVED", "JDCT_ISLOW", "(x + 1024) >> 11", "131072", "91881", "116130", "-22554", "46802", "L3D_ERR_UNSUPPORTED"):
        assert phrase in header, phrase
    for text in (header, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "image decoding (jpeg / png)" not in text.lower()


FACADE_SRC = r'''
#include "line3D_amd.hpp"
struct Mat3 { double m[9]; double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
int main(int argc, char** argv) {
    std::vector<unsigned char> file;
    if (FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr) { unsigned char b[4096]; for (size_t n; (n = fread(b, 1, sizeof(b), f)) > 0;) file.insert(file.end(), b, b + n); fclose(f); }
    unsigned int w = 0, h = 0, ch = 0;
    if (!L3D::Line3D::jpegSize(file.data(), file.size(), w, h, ch) || w != 17 || h != 9 || ch != 3) return 1;      // no device needed
    if (L3D::Line3D::jpegSize(file.data(), 10, w, h, ch)) return 1;
    L3D::Line3D l("dir", 10, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, false);
    std::list<unsigned int> wps{ 1, 2, 3 };
    std::map<unsigned int, float> sim{ { 1u, 0.5f } };
    Mat3 Km{ { 500, 0, 32, 0, 500, 24, 0, 0, 1 } };
    Vec3 tm{ { 0, 0, 0 } };
    l.addImageJPEG(0, file.data(), file.size(), Km, Km, tm, wps);
    l.addImageJPEG(1, file.data(), file.size(), Km, Km, tm, wps, 800, false);
    l.addImageJPEGDistorted(2, file.data(), file.size(), Km, Km, tm, -0.1, 0.01, wps);
    l.addImageJPEGDistorted(3, file.data(), file.size(), Km, Km, tm, -0.1, 0.01, wps, 1920, false);
    l.addImage_fixed_simJPEG(4, file.data(), file.size(), Km, Km, tm, sim);
    l.addImage_fixed_simJPEG(5, file.data(), file.size(), Km, Km, tm, sim, 1920, false);
    l.addImage_fixed_simJPEGDistorted(6, file.data(), file.size(), Km, Km, tm, -0.1, 0.0, sim);
    l.addImage_fixed_simJPEGDistorted(7, file.data(), file.size(), Km, Km, tm, -0.1, 0.0, sim, 1920, false);
    std::vector<unsigned char> px;
    const bool done = l.decodeJPEG(file.data(), file.size(), px, w, h, ch);
    return (l.numCameras() == 0 && !done) || l.valid() ? 0 : 1;      // (without a GPU every call reports and returns)
}
'''


def test_facade_additions_compile_and_link(tmp_path):
    lib = os.path.join(ROOT, "line3d_amd")
    src, exe, jpg = tmp_path / "t.cpp", tmp_path / "t", tmp_path / "a.jpg"
    src.write_text(FACADE_SRC)
    jpg.write_bytes(_case("17x9_420")[0])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.run([str(exe), str(jpg)], stderr=subprocess.DEVNULL, cwd=tmp_path).returncode == 0


def test_example_mentions_jpeg_and_still_builds(tmp_path):
    text = open(os.path.join(ROOT, "examples", "main_vsfm_amd.cpp")).read()
    assert "addImageJPEGDistorted" in text and "convert\n// JPEG" not in text and "convert JPEG" not in text
    lib = os.path.join(ROOT, "line3d_amd")
    exe = tmp_path / "main_vsfm_amd"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "main_vsfm_amd.cpp"),
                           "-L" + lib, "-lline3d_amd", "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.run([str(exe)], stderr=subprocess.DEVNULL).returncode == 2


def test_host_decoder_compiles_alone():
    """plain C++17, no HIP header"""
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", os.path.join(ROOT, "line3d_amd", "csrc", "l3d_jpeg.cpp"), "-o", os.path.join(td, "j.o")])
    text = open(os.path.join(ROOT, "line3d_amd", "csrc", "l3d_jpeg.cpp")).read() + open(os.path.join(ROOT, "line3d_amd", "csrc", "l3d_jpeg.hpp")).read()
    assert "hip/" not in text and "l3d_ctx.hpp" not in text


def test_truncations_and_mutations_under_sanitizers(tmp_path):
    """tests/cpp/jpeg_mutate_main.cpp, built from l3d_jpeg.cpp alone with the address and undefined-behaviour sanitizers: every truncation length of two
    files and 2000 seeded mutations of each of three; every run returns a status, the program exits 0"""
    exe = tmp_path / "jpeg_mutate"
    # the sanitizers' runtimes are linked into the program itself: nothing is preloaded, and the environment is passed on as it is
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "jpeg_mutate_main.cpp"), os.path.join(ROOT, "line3d_amd", "csrc", "l3d_jpeg.cpp"), "-o", str(exe)])
    args = []
    for kind, names in (("trunc", ("16x16_420", "17x9_420")), ("mut", ("37x29_420", "restart_blocks1", "optimize"))):
        for n in names:
            p = tmp_path / (n + ".jpg")
            p.write_bytes(_case(n)[0])
            args.append("%s:%s" % (kind, p))
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.match(r"ok (\d+) invalid (\d+) unsupported (\d+)", r.stdout)
    total = len(_case("16x16_420")[0]) + len(_case("17x9_420")[0]) + 3 * 2000 + 5
    assert m and sum(int(g) for g in m.groups()) == total
    assert int(m.group(1)) >= 5 and int(m.group(2)) > 1000 and int(m.group(3)) > 0
