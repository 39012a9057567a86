"""Writes tests/golden/colmap_small/: one small COLMAP model in both of its forms (cameras.txt + images.txt under txt/, cameras.bin + images.bin under
bin/), from the table below.  The layouts are COLMAP's documented output format:
    cameras.txt   CAMERA_ID MODEL WIDTH HEIGHT PARAMS[]
    images.txt    IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME  /  X Y POINT3D_ID ... (a second line per image, possibly empty; -1: no point)
    cameras.bin   uint64 count, then per camera uint32 id, int32 model id, uint64 width, uint64 height, float64 params[]
    images.bin    uint64 count, then per image uint32 id, float64 q[4], float64 t[3], uint32 camera id, the name with a terminating 0, uint64 count of
                  observations, then per observation float64 x, float64 y, uint64 point id (all ones: no point)
all little endian; lines that start with # are comments.  One camera of each of the eleven models, five images (two models are used by the images
that tests/test_colmap_reader.py expects to have no lens), observations with and without a point, one name with a space.

    python tests/golden/make_golden_colmap.py
"""
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))

# model id, name, parameters -- every number distinct, so that a wrong order shows
MODELS = [
    (0, "SIMPLE_PINHOLE", [500.5, 320.25, 240.75]),
    (1, "PINHOLE", [510.5, 511.5, 321.25, 241.75]),
    (2, "SIMPLE_RADIAL", [520.5, 322.25, 242.75, -0.11]),
    (3, "RADIAL", [530.5, 323.25, 243.75, -0.12, 0.013]),
    (4, "OPENCV", [540.5, 541.5, 324.25, 244.75, -0.13, 0.014, 0.0015, -0.0016]),
    (5, "OPENCV_FISHEYE", [550.5, 551.5, 325.25, 245.75, -0.014, 0.0015, -0.0016, 0.00017]),
    (6, "FULL_OPENCV", [560.5, 561.5, 326.25, 246.75, -0.15, 0.016, 0.0017, -0.0018, 0.019, 0.02, -0.021, 0.0022]),
    (7, "FOV", [570.5, 571.5, 327.25, 247.75, 0.93]),
    (8, "SIMPLE_RADIAL_FISHEYE", [580.5, 328.25, 248.75, -0.023]),
    (9, "RADIAL_FISHEYE", [590.5, 329.25, 249.75, -0.024, 0.0025]),
    (10, "THIN_PRISM_FISHEYE", [600.5, 601.5, 330.25, 250.75, -0.026, 0.0027, 0.0028, -0.0029, 0.003, 0.0031, 0.0032, -0.0033]),
]
SIZE = (640, 480)
# the camera ids are the model ids + 1, written in descending order: the reader must go by id, not by position
CAMERAS = [(m + 1, m, name, params) for m, name, params in reversed(MODELS)]
# image id, quaternion (w, x, y, z: not normalised in the file's digits beyond what is printed), t, camera id, name, observations (x, y, point id)
IMAGES = [
    (1, (0.9238795325112867, 0.0, 0.3826834323650898, 0.0), (0.1, -0.2, 1.5), 5, "frame_000.jpg", [(10.5, 20.25, 3), (11.5, 21.25, -1), (300.0, 200.0, 7), (12.0, 13.0, 12)]),
    (2, (0.5, 0.5, -0.5, 0.5), (-1.25, 0.5, 2.0), 6, "sub dir/frame 001.jpg", [(1.0, 2.0, -1), (3.0, 4.0, -1)]),
    (4, (0.8, 0.0, 0.0, 0.6), (0.0, 0.0, 0.0), 7, "frame_003.jpg", []),
    (7, (0.7071067811865476, -0.7071067811865476, 0.0, 0.0), (3.0, 2.0, 1.0), 8, "frame_004.jpg", [(5.0, 6.0, 0), (7.0, 8.0, 3), (9.0, 10.0, 41)]),
    (9, (1.0, 0.0, 0.0, 0.0), (0.25, 0.5, 0.75), 1, "frame_005.jpg", [(100.0, 50.0, 12)]),
]


def write_txt(d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n# Number of cameras: %d\n" % len(CAMERAS))
        for cid, _, name, params in CAMERAS:
            f.write("%d %s %d %d %s\n" % (cid, name, SIZE[0], SIZE[1], " ".join(repr(p) for p in params)))
    with open(os.path.join(d, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        f.write("# Number of images: %d\n" % len(IMAGES))
        for iid, q, t, cid, name, obs in IMAGES:
            f.write("%d %s %s %d %s\n" % (iid, " ".join(repr(v) for v in q), " ".join(repr(v) for v in t), cid, name))
            f.write(" ".join("%r %r %d" % o for o in obs) + "\n")


def bin_bytes():
    cams = struct.pack("<Q", len(CAMERAS))
    for cid, mid, _, params in CAMERAS:
        cams += struct.pack("<IiQQ", cid, mid, SIZE[0], SIZE[1]) + struct.pack("<%dd" % len(params), *params)
    ims = struct.pack("<Q", len(IMAGES))
    for iid, q, t, cid, name, obs in IMAGES:
        ims += struct.pack("<I4d3dI", iid, *q, *t, cid) + name.encode() + b"\0" + struct.pack("<Q", len(obs))
        for x, y, p in obs:
            ims += struct.pack("<ddQ", x, y, p if p >= 0 else 0xFFFFFFFFFFFFFFFF)
    return cams, ims


def write_bin(d):
    os.makedirs(d, exist_ok=True)
    cams, ims = bin_bytes()
    with open(os.path.join(d, "cameras.bin"), "wb") as f:
        f.write(cams)
    with open(os.path.join(d, "images.bin"), "wb") as f:
        f.write(ims)


if __name__ == "__main__":
    root = os.path.join(HERE, "colmap_small")
    write_txt(os.path.join(root, "txt"))
    write_bin(os.path.join(root, "bin"))
    print("wrote", root)
