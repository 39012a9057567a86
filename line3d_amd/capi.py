"""ctypes binding of the C ABI (include/line3d_amd.h).  Plumbing only: every compute call lands in the
HIP library; if the library or a GPU is missing the constructor raises (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libline3d_amd.so")
if os.environ.get("L3D_LIBRARY"):      # A/B measurements: an alternative build of the library
    LIB_PATH = os.environ["L3D_LIBRARY"]

MATCH_DTYPE = np.dtype([("segID1", "<u4"), ("camID2", "<u4"), ("segID2", "<u4"),
                        ("depths", "<f4", (4,)), ("confidence", "<f4")])
EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("w", "<f4")])
HYP_DTYPE = np.dtype([("P1", "<f8", (3,)), ("P2", "<f8", (3,)), ("dir", "<f8", (3,)),
                      ("depth_p1", "<f4"), ("depth_p2", "<f4"),
                      ("k_lower", "<f4"), ("k_upper", "<f4"), ("median_depth", "<f4"), ("pad", "<u4")])
REGION_DTYPE = np.dtype([("minpix", "<u4"), ("n_used", "<i4"), ("steps", "<i4"), ("pts", "<i4"), ("alg", "<i4"), ("scored", "<i4"), ("accepted", "<i4"),
                         ("pad", "<i4"), ("hist_n", "<i4", (8,))] + [(k, "<f8") for k in ("cx", "cy", "x1", "y1", "x2", "y2", "width", "theta", "density",
                                                                "fx1", "fy1", "fx2", "fy2", "fwidth", "p", "nfa")])
assert MATCH_DTYPE.itemsize == 32 and EDGE_DTYPE.itemsize == 12 and HYP_DTYPE.itemsize == 96 and REGION_DTYPE.itemsize == 192

_lib = None
_lib_check = None
CHECK_LIB_PATH = os.path.join(_HERE, "libline3d_amd_check.so")


def load_library(crosschecks: bool = False):
    """dlopen libline3d_amd.so (built in-tree by __graft_entry__.build() / make -C line3d_amd/csrc).
    crosschecks=True (tests only): libline3d_amd_check.so, the same sources built with -DL3D_CROSSCHECKS -- the only build in which
    L3D_HOST_BOOKKEEPING / L3D_HOST_CLUSTERING / L3D_MATCH_SYNC force a host-side stage where the device stage would run."""
    global _lib, _lib_check
    if crosschecks:
        if _lib_check is None:
            load_library()
            if not os.path.exists(CHECK_LIB_PATH):
                raise RuntimeError("cross-check library not built: %s (make -C line3d_amd/csrc check)" % CHECK_LIB_PATH)
            lib = C.CDLL(CHECK_LIB_PATH)
            lib.l3d_last_error.restype = C.c_char_p
            lib.l3d_last_error.argtypes = [C.c_void_p]
            lib.l3d_profile_names.restype = C.c_char_p
            lib.l3d_free.argtypes = [C.c_void_p]
            lib.l3d_ctx_destroy.argtypes = [C.c_void_p]
            _lib_check = lib
        return _lib_check
    if _lib is None:
        try:
            # PyTorch-ROCm ships its own HIP runtime; when both live in one process (multi-GPU driver, tests) the
            # framework's copy has to be loaded first or torch.cuda reports no devices.  Plumbing only.
            import torch  # noqa: F401
        except Exception:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("HIP library not built: %s (run `python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.l3d_last_error.restype = C.c_char_p
        lib.l3d_last_error.argtypes = [C.c_void_p]
        lib.l3d_profile_names.restype = C.c_char_p
        lib.l3d_free.argtypes = [C.c_void_p]
        lib.l3d_ctx_destroy.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


class L3DError(RuntimeError):
    pass


def _p(a, t=C.c_void_p):
    return a.ctypes.data_as(t)


def image_arguments(img):
    """uint8 array H x W or H x W x C -> (pointer, width, height, channels, row stride in bytes) for the pixel-taking calls; an array whose
    pixels are not contiguous within a row is copied.  The pointer refers to `img` (or the copy, kept alive on the returned object)."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise TypeError("image must be a uint8 array H x W or H x W x C")
    ch = 1 if a.ndim == 2 else a.shape[2]
    inner_ok = a.strides[1] == ch and (a.ndim == 2 or a.strides[2] == 1)
    if not inner_ok or a.strides[0] < a.shape[1] * ch:
        a = np.ascontiguousarray(a)
    ptr = C.c_void_p(a.ctypes.data)
    ptr._keep = a
    return ptr, int(a.shape[1]), int(a.shape[0]), int(ch), int(a.strides[0])


def _bytes_arguments(data):
    """bytes-like (or a uint8 array) -> (pointer, length); the buffer is kept alive on the pointer"""
    a = np.frombuffer(bytes(data) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).tobytes(), dtype=np.uint8)
    ptr = C.c_void_p(a.ctypes.data if len(a) else None)
    ptr._keep = a
    return ptr, C.c_size_t(len(a))


def jpeg_info(data):
    """l3d_jpeg_info: (width, height, channels) of a baseline JPEG file from its headers alone -- no context, no device.  A file the decoder
    refuses raises L3DError carrying the status in .code (5: unsupported, 1: invalid) and the cause in its text."""
    lib = load_library()
    lib.l3d_jpeg_last_error.restype = C.c_char_p
    ptr, n = _bytes_arguments(data)
    w, h, ch = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib.l3d_jpeg_info(ptr, n, C.byref(w), C.byref(h), C.byref(ch))
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_jpeg_last_error().decode()))
        e.code = rc
        raise e
    return w.value, h.value, ch.value


def test_jpeg_coefficients(data):
    """l3d_test_jpeg_coefficients (host only): (coef int16 (n_blocks, 64), qt uint16 (3, 64), layout int32 (27,)) as include/line3d_amd.h lists them"""
    lib = load_library()
    lib.l3d_jpeg_last_error.restype = C.c_char_p
    ptr, n = _bytes_arguments(data)
    coef, nb = C.POINTER(C.c_int16)(), C.c_size_t(0)
    qt, layout = np.zeros((3, 64), np.uint16), np.zeros(27, np.int32)
    rc = lib.l3d_test_jpeg_coefficients(ptr, n, C.byref(coef), C.byref(nb), _p(qt), _p(layout))
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_jpeg_last_error().decode()))
        e.code = rc
        raise e
    out = np.ctypeslib.as_array(coef, (nb.value, 64)).copy()
    lib.l3d_free(coef)
    return out, qt, layout


test_jpeg_coefficients.__test__ = False


class RefineParams(C.Structure):
    """l3d_refine_params"""
    _fields_ = [("max_iterations", C.c_int32), ("pad", C.c_int32), ("huber_px", C.c_double)]


def _refine_call(fn, head, group_start, member_cam, member_seg, member_pts, cameras, max_iterations, huber_px):
    """the argument list l3d_refine_lines and l3d_test_refine_host share (head: the context, or nothing) -> (rc, result dict)"""
    gs = np.ascontiguousarray(group_start, np.int32)
    mc = np.ascontiguousarray(member_cam, np.int32)
    ms = np.ascontiguousarray(member_seg, np.float32).reshape(-1, 4)
    mp = np.ascontiguousarray(member_pts, np.float64).reshape(-1, 6)
    cams = np.ascontiguousarray(cameras, np.float64).reshape(-1, 12)
    ng = max(len(gs) - 1, 0)
    if not (len(mc) == len(ms) == len(mp)) or (ng and gs[-1] > len(mc)):
        raise ValueError("refine_lines: the member arrays do not match the group table")
    prm = None if max_iterations is None and huber_px is None else RefineParams(20 if max_iterations is None else int(max_iterations), 0, 2.0 if huber_px is None else float(huber_px))
    line, rb, ra = np.zeros((ng, 6)), np.zeros(ng), np.zeros(ng)
    it, st = np.zeros(ng, np.int32), np.zeros(ng, np.int32)
    cnt, segs, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(), C.c_int(0)
    rc = fn(*head, _p(gs), C.c_int(ng), _p(mc), _p(ms), _p(mp), _p(cams), C.c_int(len(cams)), C.byref(prm) if prm is not None else None, _p(line), _p(rb), _p(ra), _p(it), _p(st),
            C.byref(cnt), C.byref(segs), C.byref(n))
    if rc != 0:
        return rc, None
    counts = np.ctypeslib.as_array(cnt, (ng,)).copy() if ng else np.zeros(0, np.int32)
    flat = np.ctypeslib.as_array(segs, (n.value * 6,)).copy().reshape(-1, 6) if n.value else np.zeros((0, 6))
    lib = load_library()
    lib.l3d_free(cnt)
    lib.l3d_free(segs)
    return 0, {"line": line, "rms_before": rb, "rms_after": ra, "iterations": it, "status": st, "seg_count": counts, "segs": flat}


def refine_lines_host(group_start, member_cam, member_seg, member_pts, cameras, max_iterations=None, huber_px=None):
    """l3d_test_refine_host: the refinement's arithmetic on the host -- no context, no device.  Arguments and result as Context.refine_lines."""
    lib = load_library()
    lib.l3d_refine_last_error.restype = C.c_char_p
    rc, out = _refine_call(lib.l3d_test_refine_host, (), group_start, member_cam, member_seg, member_pts, cameras, max_iterations, huber_px)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_refine_last_error().decode()))
        e.code = rc
        raise e
    return out


class DetectEntry(C.Structure):
    """l3d_detect_entry (include/line3d_amd.h)"""
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("row_stride", C.c_size_t),
                ("jpeg", C.c_void_p), ("jpeg_bytes", C.c_size_t), ("new_width", C.c_int), ("new_height", C.c_int), ("min_length", C.c_float),
                ("max_segments", C.c_int), ("camera", C.c_void_p)]


class ImageEntry(C.Structure):
    """l3d_image_entry (include/line3d_amd.h)"""
    _fields_ = [("image_id", C.c_uint32), ("pixels", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int),
                ("row_stride", C.c_size_t), ("jpeg", C.c_void_p), ("jpeg_bytes", C.c_size_t), ("K", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p),
                ("dist", C.c_void_p), ("link_ids", C.c_void_p), ("sims", C.c_void_p), ("n_links", C.c_int)]


# l3d_lens (include/line3d_amd.h, "A LENS")
LENS_BROWN, LENS_FISHEYE = 1, 2


class Lens(C.Structure):
    """l3d_lens: model, the source camera fx, fy, cx, cy (all zero: the output camera), k[8]"""
    _fields_ = [("model", C.c_int), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k", C.c_double * 8)]


def lens(model, coeffs, camera=None):
    """An l3d_lens.  model: LENS_BROWN / "brown" (coeffs k1 k2 p1 p2 k3 k4 k5 k6, OpenCV's order) or LENS_FISHEYE / "fisheye" (k1 k2 k3 k4); fewer
    coefficients are filled up with zeros.  camera = (fx, fy, cx, cy) of the distorted image; None: the camera the image is undistorted onto.
    What the library refuses (an unknown model number, values that are not finite, ...) is left to it; only the shapes are checked here."""
    m = {"brown": LENS_BROWN, "fisheye": LENS_FISHEYE}.get(model.lower() if isinstance(model, str) else None, model)
    if isinstance(m, str):
        raise ValueError("lens model must be 'brown', 'fisheye' or a model number")
    k = [float(v) for v in coeffs]
    if len(k) > 8:
        raise ValueError("a lens has at most 8 coefficients")
    out = Lens()
    out.model = int(m)
    if camera is not None:
        if len(camera) != 4:
            raise ValueError("camera must be (fx, fy, cx, cy)")
        out.fx, out.fy, out.cx, out.cy = (float(v) for v in camera)
    for i, v in enumerate(k):
        out.k[i] = v
    return out


def _lens_camera(lens_, camera):
    """The camera entry (6 doubles) that goes with a lens: the output camera (4 numbers, or 6 of which the library wants k1 = k2 = 0); None: the
    lens's own source camera"""
    if camera is None:
        if lens_.fx == 0.0 and lens_.fy == 0.0:
            raise ValueError("a lens without a source camera needs camera = (fx, fy, cx, cy), the camera to undistort onto")
        camera = (lens_.fx, lens_.fy, lens_.cx, lens_.cy)
    if len(camera) not in (4, 6):
        raise ValueError("camera must be (fx, fy, cx, cy) beside a lens")
    return (C.c_double * 6)(*([float(v) for v in camera] + [0.0, 0.0])[:6])


def lens_pointers(lenses, n):
    """the `const l3d_lens* const*` argument of the ..._lens calls for a list with one Lens or None per entry (None: a null array), and what keeps it alive"""
    if lenses is None or all(l is None for l in lenses):
        return None, []
    lenses = list(lenses)
    if len(lenses) != n:
        raise ValueError("lenses: %d entries for %d images" % (len(lenses), n))
    arr = (C.c_void_p * max(1, n))()
    for i, l in enumerate(lenses):
        if l is not None:
            if not isinstance(l, Lens):
                raise TypeError("lens %d must come from capi.lens()" % i)
            arr[i] = C.addressof(l)
    return arr, lenses


# l3d_remap (include/line3d_amd.h, "A REMAP")
class Remap(C.Structure):
    """l3d_remap: the lens, the output size (0, 0: the source's), the caller's mask in the source grid, and whether blank pixels are invalid"""
    _fields_ = [("lens", C.c_void_p), ("out_width", C.c_int32), ("out_height", C.c_int32), ("mask", C.c_void_p), ("mask_row_stride", C.c_size_t), ("mask_width", C.c_int32), ("mask_height", C.c_int32),
                ("mask_on_device", C.c_int32), ("border_mask", C.c_int32)]


def remap(lens=None, out_size=None, mask=None, border_mask=True):
    """An l3d_remap.  lens: capi.lens(...) or None; out_size = (width, height), None: the source's; mask: None, a uint8 / bool array H x W in the
    SOURCE grid (non-zero = valid), or a device object of that shape (a torch uint8 device tensor, anything with __cuda_array_interface__);
    border_mask: pixels the resampling leaves blank are invalid.  What it points at is kept alive on the returned object."""
    r = Remap()
    r._keep = []
    if lens is not None:
        if not isinstance(lens, Lens):
            raise TypeError("lens must come from capi.lens()")
        r.lens = C.addressof(lens)
        r._keep.append(lens)
    if out_size is not None:
        r.out_width, r.out_height = int(out_size[0]), int(out_size[1])
    if mask is not None:
        if hasattr(mask, "__cuda_array_interface__"):
            iface = mask.__cuda_array_interface__
            shape, strides = tuple(iface["shape"]), iface.get("strides")
            if len(shape) != 2 or str(iface["typestr"]) not in ("|u1", "|b1") or (strides is not None and int(strides[1]) != 1):
                raise TypeError("a device mask must be an H x W array of bytes whose rows are contiguous")
            r.mask, r.mask_row_stride, r.mask_on_device = int(iface["data"][0]), int(shape[1] if strides is None else strides[0]), 1
            r._keep.append(mask)
            r._mask_shape = (int(shape[0]), int(shape[1]))
            r.mask_height, r.mask_width = r._mask_shape
        else:
            m = np.asarray(mask)
            if m.ndim != 2 or m.dtype not in (np.uint8, np.bool_):
                raise TypeError("mask must be a uint8 or bool array H x W")
            m = np.ascontiguousarray(m).view(np.uint8)
            r.mask, r.mask_row_stride, r.mask_on_device = m.ctypes.data, m.strides[0], 0
            r._keep.append(m)
            r._mask_shape = m.shape
            r.mask_height, r.mask_width = m.shape
    r.border_mask = 1 if border_mask else 0
    return r


def remap_of(lens, out_size, mask, border_mask, source_size):
    """The Remap of the lens=, out_size=, mask=, border_mask= keywords (None when only a lens, or nothing, was given: the call as it was);
    source_size = (width, height) of the image the mask must match"""
    if out_size is None and mask is None and border_mask is None:
        return None
    r = remap(lens, out_size, mask, True if border_mask is None else border_mask)
    if mask is not None and tuple(r._mask_shape) != (int(source_size[1]), int(source_size[0])):
        raise ValueError("mask: shape %s, the source image is %d x %d (H x W)" % (tuple(r._mask_shape), source_size[1], source_size[0]))
    return r


def undistort_plan(lens_, size, alpha=0.0, out_size=None, max_dim=0, fov_max_deg=120.0):
    """l3d_undistort_plan (host, no context and no device): the output camera and size for a lens that carries its source camera.
    size = (width, height) of the source image; alpha in [0, 1]: 0 = no blank pixel in the output, 1 = every source pixel inside fov_max_deg is
    kept; out_size: (width, height), None for the source size, or "keep_focal" / (-1, -1) for the size at which fx' = fx, scaled down to max_dim
    when that is positive.  -> (K 3 x 3 float64, (width, height)).  A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_undistort_plan_error.restype = C.c_char_p
    if not isinstance(lens_, Lens):
        raise TypeError("lens must come from capi.lens()")
    ow, oh = (0, 0) if out_size is None else (-1, -1) if isinstance(out_size, str) and out_size == "keep_focal" else (int(out_size[0]), int(out_size[1]))
    K = np.zeros(9, np.float64)
    w, h = C.c_int(0), C.c_int(0)
    rc = lib.l3d_undistort_plan(C.byref(lens_), C.c_int(int(size[0])), C.c_int(int(size[1])), C.c_double(float(alpha)), C.c_int(ow), C.c_int(oh),
                                C.c_int(int(max_dim)), C.c_double(float(fov_max_deg)), _p(K), C.byref(w), C.byref(h))
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_undistort_plan_error().decode()))
        e.code = rc
        raise e
    return K.reshape(3, 3), (w.value, h.value)


def undistort_route(camera, lens_, remap_, size, channels=1):
    """l3d_test_undistort_route (host only, no context and no device): what a batch entry with this camera (None or fx, fy, cx, cy, k1, k2), lens
    and remap (capi.lens / capi.remap or None) makes of an image of size = (width, height) -> (code, message, route, plane, (out_width, out_height));
    route: 0 none, 1 k_det_undistort, 2 k_det_undistort_lens, 3 k_det_undistort_remap.  A refusal is returned, not raised."""
    lib = load_library()
    cam = None if camera is None else np.ascontiguousarray(camera, np.float64)
    route, plane, ow, oh = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    msg = C.create_string_buffer(256)
    rc = lib.l3d_test_undistort_route(None if cam is None else _p(cam), None if lens_ is None else C.byref(lens_), None if remap_ is None else C.byref(remap_),
                                      C.c_int(int(size[0])), C.c_int(int(size[1])), C.c_int(int(channels)), C.byref(route), C.byref(plane), C.byref(ow), C.byref(oh),
                                      msg, C.c_size_t(len(msg)))
    return rc, msg.value.decode(), route.value, plane.value, (ow.value, oh.value)




def remap_pointers(lenses, out_sizes, masks, border_masks, n):
    """the `const l3d_remap* const*` argument of the ..._remap calls, or None when no image asks for another size, a mask or a border rule (then
    the ..._lens call, or the plain one, is the call to make), and what keeps it alive.  An image with only a lens gets a remap that says nothing more
    (border_mask 0): the library treats it as the lens alone"""
    lenses, out_sizes, masks, border_masks = (_per_image(v, n, what) for v, what in ((lenses, "lenses"), (out_sizes, "out_sizes"), (masks, "masks"),
                                                                                     (border_masks, "border_masks")))
    if all(o is None and m is None and b is None for o, m, b in zip(out_sizes, masks, border_masks)):
        return None, []
    arr, keep = (C.c_void_p * max(1, n))(), [None] * n             # (keep: one entry per image)
    for i in range(n):
        asks = out_sizes[i] is not None or masks[i] is not None or border_masks[i] is not None
        if not asks and lenses[i] is None:
            continue
        r = remap(lenses[i], out_sizes[i], masks[i], (True if border_masks[i] is None else border_masks[i]) if asks else False)
        arr[i] = C.addressof(r)
        keep[i] = r
    return arr, keep


# l3d_segment_mask (include/line3d_amd.h, "A SEGMENT MASK")
SEGMASK_DROP, SEGMASK_CLIP, SEGMASK_SPLIT = 0, 1, 2


class SegmentMask(C.Structure):
    """l3d_segment_mask: the plane, the lens and the segments' camera, the mode and its parameters"""
    _fields_ = [("mask", C.c_void_p), ("mask_row_stride", C.c_size_t), ("mask_width", C.c_int32), ("mask_height", C.c_int32), ("mask_on_device", C.c_int32),
                ("lens", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("mode", C.c_int32), ("threshold", C.c_int32),
                ("keep_permille", C.c_int32), ("max_gap", C.c_int32), ("min_length", C.c_double)]


def segment_mask(mask, lens=None, camera=None, mode="drop", threshold=1, keep_permille=500, max_gap=0, min_length=0.0):
    """An l3d_segment_mask.  mask: a uint8 / bool array H x W whose rows are contiguous (they may lie further apart than W: a view into a wider
    array is taken as it is), or a device object of that shape (a torch uint8 device tensor, anything with __cuda_array_interface__); a byte
    >= threshold is valid.  lens: capi.lens(...) when the mask lies in the distorted image's grid, with camera = (fx, fy, cx, cy) of the grid the
    segments lie in; None: the mask is in the segments' grid.  mode: "drop" (keep a segment when at least keep_permille of its samples are valid),
    "clip" (the longest valid stretch) or "split" (every valid stretch), the latter two bridging gaps of up to max_gap samples and keeping
    stretches of at least min_length pixels; or a mode number.  What the library refuses is left to it.  What the struct points at is kept alive
    on the returned object."""
    m = SegmentMask()
    m._keep = []
    if hasattr(mask, "__cuda_array_interface__"):
        iface = mask.__cuda_array_interface__
        shape, strides = tuple(iface["shape"]), iface.get("strides")
        if len(shape) != 2 or str(iface["typestr"]) not in ("|u1", "|b1") or (strides is not None and int(strides[1]) != 1):
            raise TypeError("a device mask must be an H x W array of bytes whose rows are contiguous")
        m.mask, m.mask_row_stride, m.mask_on_device = int(iface["data"][0]), int(shape[1] if strides is None else strides[0]), 1
        m.mask_height, m.mask_width = int(shape[0]), int(shape[1])
        m._keep.append(mask)
    elif mask is not None:
        a = np.asarray(mask)
        if a.ndim != 2 or a.dtype not in (np.uint8, np.bool_):
            raise TypeError("mask must be a uint8 or bool array H x W")
        if a.shape[0] > 1 and a.shape[1] > 0 and (a.strides[1] != 1 or a.strides[0] < a.shape[1]):
            a = np.ascontiguousarray(a)
        a = a.view(np.uint8)
        m.mask = a.ctypes.data if a.size else None
        m.mask_row_stride = max(int(a.strides[0]), int(a.shape[1]))
        m.mask_height, m.mask_width = int(a.shape[0]), int(a.shape[1])
        m._keep.append(a)
    if lens is not None:
        if not isinstance(lens, Lens):
            raise TypeError("lens must come from capi.lens()")
        m.lens = C.addressof(lens)
        m._keep.append(lens)
    if camera is not None:
        if len(camera) != 4:
            raise ValueError("camera must be (fx, fy, cx, cy)")
        m.fx, m.fy, m.cx, m.cy = (float(v) for v in camera)
    mode_ = {"drop": SEGMASK_DROP, "clip": SEGMASK_CLIP, "split": SEGMASK_SPLIT}.get(mode.lower() if isinstance(mode, str) else None, mode)
    if isinstance(mode_, str):
        raise ValueError("mode must be 'drop', 'clip', 'split' or a mode number")
    m.mode, m.threshold, m.keep_permille, m.max_gap, m.min_length = int(mode_), int(threshold), int(keep_permille), int(max_gap), float(min_length)
    return m


def _as_segment_mask(mask, kw):
    if isinstance(mask, SegmentMask):
        if kw:
            raise TypeError("a capi.segment_mask() carries its parameters: %s given beside it" % sorted(kw))
        return mask
    return segment_mask(mask, **kw)


def _mask_segments_call(fn, head, seg_ptr, n, m):
    """the argument list the segment-mask calls share (head: the context, or nothing) -> (rc, segments (k, 4) float32, src_index (k,) int32)"""
    out, src, n_out = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)(), C.c_int(0)
    rc = fn(*head, seg_ptr, C.c_int(n), C.byref(m) if m is not None else None, C.byref(out), C.byref(src), C.byref(n_out))
    if rc != 0:
        return rc, None, None
    k = n_out.value
    segs = np.ctypeslib.as_array(out, (k * 4,)).copy().reshape(-1, 4) if k else np.zeros((0, 4), np.float32)
    idx = np.ctypeslib.as_array(src, (k,)).copy() if k else np.zeros(0, np.int32)
    lib = load_library()
    lib.l3d_free(out)
    lib.l3d_free(src)
    return 0, segs, idx


def mask_segments_host(segments, mask, **kw):
    """l3d_test_mask_segments_host: the segment mask's arithmetic on the host -- no context, no device.  Arguments and result as
    Context.mask_segments (host arrays only).  A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_segmask_last_error.restype = C.c_char_p
    m = None if mask is None else _as_segment_mask(mask, kw)
    s = np.ascontiguousarray(segments, np.float32).reshape(-1, 4)
    rc, segs, idx = _mask_segments_call(lib.l3d_test_mask_segments_host, (), _p(s) if len(s) else None, len(s), m)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_segmask_last_error().decode()))
        e.code = rc
        raise e
    return segs, idx


class Camera(C.Structure):
    """l3d_camera: K, R, t (row-major, x = K (R X + t)) and the image size"""
    _fields_ = [("K", C.c_double * 9), ("R", C.c_double * 9), ("t", C.c_double * 3), ("width", C.c_int32), ("height", C.c_int32)]


def cameras(cams):
    """An l3d_camera array from a list of (K, R, t, width, height) tuples or of dicts with those keys (an array made here passes through)"""
    if isinstance(cams, C.Array) and cams._type_ is Camera:
        return cams
    arr = (Camera * max(1, len(cams)))()
    for i, cam in enumerate(cams):
        K, R, t, w, h = (cam[k] for k in ("K", "R", "t", "width", "height")) if isinstance(cam, dict) else cam
        arr[i].K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
        arr[i].R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
        arr[i].t[:] = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
        arr[i].width, arr[i].height = int(w), int(h)
    arr._n = len(cams)
    return arr


def _project_call(fn, head, seg_ptr, n, cams, m, near, margin):
    """the argument list the projection calls share (head: the context, or nothing) -> (rc, seg2d (k, 4) float32, src_index (k,) int32,
    flags (k,) uint8, cam_start (m + 1,) int64)"""
    seg2d, src, flags = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_ubyte)()
    start = np.zeros(max(0, m) + 1, np.int64)
    rc = fn(*head, seg_ptr, C.c_int(n), cams, C.c_int(m), C.c_double(near), C.c_double(margin), C.byref(seg2d), C.byref(src), C.byref(flags), _p(start))
    if rc != 0:
        return rc, None, None, None, None
    k = int(start[-1])
    segs = np.ctypeslib.as_array(seg2d, (k * 4,)).copy().reshape(-1, 4) if k else np.zeros((0, 4), np.float32)
    idx = np.ctypeslib.as_array(src, (k,)).copy() if k else np.zeros(0, np.int32)
    fl = np.ctypeslib.as_array(flags, (k,)).copy() if k else np.zeros(0, np.uint8)
    lib = load_library()
    for p in (seg2d, src, flags):
        lib.l3d_free(p)
    return 0, segs, idx, fl, start


def _project_arguments(seg3d, cams):
    s = np.ascontiguousarray(seg3d, np.float64).reshape(-1, 6)
    arr = cameras(cams)
    m = getattr(arr, "_n", len(arr))
    return s, arr, m


def project_lines_host(seg3d, cams, near=1e-6, margin=0.0):
    """l3d_test_project_lines_host: the projection's arithmetic on the host -- no context, no device.  Arguments and result as
    Context.project_lines (host arrays only).  A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_project_last_error.restype = C.c_char_p
    s, arr, m = _project_arguments(seg3d, cams)
    rc, segs, idx, fl, start = _project_call(lib.l3d_test_project_lines_host, (), _p(s) if len(s) else None, len(s), arr if m else None, m, near, margin)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_project_last_error().decode()))
        e.code = rc
        raise e
    return segs, idx, fl, start


class MergeParams(C.Structure):
    """l3d_merge_params (include/line3d_amd.h)"""
    _fields_ = [("cos_min", C.c_double), ("max_gap", C.c_double)]


def merge_params(cos_min=None, max_gap=0.0, angle_deg=5.0):
    """An l3d_merge_params.  cos_min None: cos(angle_deg pi / 180), in double"""
    import math
    p = MergeParams()
    p.cos_min = math.cos(angle_deg * math.pi / 180.0) if cos_min is None else float(cos_min)
    p.max_gap = float(max_gap)
    return p


def _merge_call(fn, head, lines, tol, prm):
    """the argument list the merge calls share (head: the context, or nothing) -> (rc, dict(group (n,) int32, pairs (k, 2) int32, counts (4,) int32)).
    lines / tol None: passed as NULL with the count in `lines` (an int), for the refusals"""
    if lines is None or isinstance(lines, int):
        n, lp, tp = int(lines or 0), None, (None if tol is None else _p(np.ascontiguousarray(tol, np.float64)))
    else:
        lines = np.ascontiguousarray(lines, np.float64).reshape(-1, 6)
        n, lp = len(lines), (_p(lines) if len(lines) else None)
        tol = None if tol is None else np.ascontiguousarray(tol, np.float64).reshape(-1)
        if tol is not None and len(tol) != n:
            raise ValueError("merge lines: one tolerance per line")
        tp = None if tol is None or n == 0 else _p(tol)
    group = np.zeros(max(1, n), np.int32)
    counts = np.zeros(4, np.int32)
    pairs, k = C.POINTER(C.c_int32)(), C.c_int(0)
    rc = fn(*head, lp, tp, C.c_int(n), None if prm is None else C.byref(prm), _p(group), C.byref(pairs), C.byref(k), _p(counts))
    if rc != 0:
        return rc, None
    pr = np.ctypeslib.as_array(pairs, (k.value * 2,)).copy().reshape(-1, 2) if k.value else np.zeros((0, 2), np.int32)
    load_library().l3d_free(pairs)
    return 0, dict(group=group[:max(0, n)].copy(), pairs=pr, counts=counts)


def merge_lines_host(lines, tol, cos_min=None, max_gap=0.0, params=None):
    """l3d_test_merge_lines_host: the grouping of duplicate 3-D lines on the host -- no context, no device.  Arguments and result as
    Context.merge_lines.  A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_merge_last_error.restype = C.c_char_p
    rc, out = _merge_call(lib.l3d_test_merge_lines_host, (), lines, tol, merge_params(cos_min, max_gap) if params is None else params)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_merge_last_error().decode()))
        e.code = rc
        raise e
    return out


class JunctionParams(C.Structure):
    """l3d_junction_params (include/line3d_amd.h)"""
    _fields_ = [("cos_max", C.c_double), ("crossings", C.c_int32), ("pad", C.c_int32)]


class JunctionRecord(C.Structure):
    """l3d_junction_record: 64 bytes"""
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("where_i", C.c_int32), ("where_j", C.c_int32), ("s", C.c_double), ("t", C.c_double), ("gap", C.c_double),
                ("X", C.c_double * 3)]


class JunctionVertex(C.Structure):
    """l3d_junction_vertex: 32 bytes"""
    _fields_ = [("X", C.c_double * 3), ("first_node", C.c_int32), ("degree", C.c_int32)]


JUNCTION_RECORD = np.dtype([("i", np.int32), ("j", np.int32), ("where_i", np.int32), ("where_j", np.int32), ("s", np.float64), ("t", np.float64),
                            ("gap", np.float64), ("X", np.float64, (3,))])
JUNCTION_VERTEX = np.dtype([("X", np.float64, (3,)), ("first_node", np.int32), ("degree", np.int32)])
JUNCTION_END_P, JUNCTION_END_Q, JUNCTION_INTERIOR = 0, 1, 2


def junction_params(cos_max=None, crossings=0, angle_min_deg=10.0):
    """An l3d_junction_params.  cos_max None: cos(angle_min_deg pi / 180), in double"""
    import math
    p = JunctionParams()
    p.cos_max = math.cos(angle_min_deg * math.pi / 180.0) if cos_max is None else float(cos_max)
    p.crossings = int(crossings)
    p.pad = 0
    return p


def _junction_call(fn, head, lines, tol, ext, prm):
    """the argument list the junction calls share (head: the context, or nothing) -> (rc, dict(records: JUNCTION_RECORD array, node_vertex (2 n,) int32,
    vertices: JUNCTION_VERTEX array, node_attach (2 n,) int32, counts (8,) int32)).  lines None or an int: passed as NULL with that count, for the
    refusals"""
    dbl = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).reshape(-1)
    if lines is None or isinstance(lines, int):
        n, lp, tol, ext = int(lines or 0), None, dbl(tol), dbl(ext)
    else:
        lines = np.ascontiguousarray(lines, np.float64).reshape(-1, 6)
        n, lp, tol, ext = len(lines), (_p(lines) if len(lines) else None), dbl(tol), dbl(ext)
        if (tol is not None and len(tol) != n) or (ext is not None and len(ext) != n):
            raise ValueError("junction lines: one tolerance and one extension per line")
    tp = None if tol is None or len(tol) == 0 else _p(tol)
    ep = None if ext is None or len(ext) == 0 else _p(ext)
    node_vertex = np.zeros(max(2, 2 * n), np.int32)
    node_attach = np.zeros(max(2, 2 * n), np.int32)
    counts = np.zeros(8, np.int32)
    rec, vert, nr, nv = C.POINTER(JunctionRecord)(), C.POINTER(JunctionVertex)(), C.c_int(0), C.c_int(0)
    rc = fn(*head, lp, tp, ep, C.c_int(n), None if prm is None else C.byref(prm), C.byref(rec), C.byref(nr), _p(node_vertex), C.byref(vert), C.byref(nv),
            _p(node_attach), _p(counts))
    if rc != 0:
        return rc, None
    records = np.frombuffer(C.string_at(rec, nr.value * 64), JUNCTION_RECORD).copy() if nr.value else np.zeros(0, JUNCTION_RECORD)
    vertices = np.frombuffer(C.string_at(vert, nv.value * 32), JUNCTION_VERTEX).copy() if nv.value else np.zeros(0, JUNCTION_VERTEX)
    lib = load_library()
    lib.l3d_free(rec)
    lib.l3d_free(vert)
    m = 2 * max(0, n)
    return 0, dict(records=records, node_vertex=node_vertex[:m].copy(), vertices=vertices, node_attach=node_attach[:m].copy(), counts=counts)


def junction_lines_host(lines, tol, ext, cos_max=None, crossings=0, params=None):
    """l3d_test_junction_lines_host: the junctions of 3-D lines on the host -- no context, no device.  Arguments and result as Context.junction_lines.
    A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_junction_last_error.restype = C.c_char_p
    rc, out = _junction_call(lib.l3d_test_junction_lines_host, (), lines, tol, ext, junction_params(cos_max, crossings) if params is None else params)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_junction_last_error().decode()))
        e.code = rc
        raise e
    return out


class PlaneParams(C.Structure):
    """l3d_plane_params (include/line3d_amd.h)"""
    _fields_ = [("cos_max", C.c_double), ("cos_min", C.c_double), ("min_lines", C.c_int32), ("pad", C.c_int32)]


class Plane(C.Structure):
    """l3d_plane: 128 bytes"""
    _fields_ = [("N", C.c_double * 3), ("c", C.c_double), ("u", C.c_double * 3), ("v", C.c_double * 3), ("rect", C.c_double * 4), ("rep", C.c_int32),
                ("first_hyp", C.c_int32), ("n_hyp", C.c_int32), ("n_lines", C.c_int32)]


class PlaneMember(C.Structure):
    """l3d_plane_member: 16 bytes"""
    _fields_ = [("plane", C.c_int32), ("line", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32)]


PLANE = np.dtype([("N", np.float64, (3,)), ("c", np.float64), ("u", np.float64, (3,)), ("v", np.float64, (3,)), ("rect", np.float64, (4,)), ("rep", np.int32),
                  ("first_hyp", np.int32), ("n_hyp", np.int32), ("n_lines", np.int32)])
PLANE_MEMBER = np.dtype([("plane", np.int32), ("line", np.int32), ("flags", np.int32), ("pad", np.int32)])
PLANE_SEED = 1


def plane_params(cos_max=None, cos_min=None, min_lines=3, angle_min_deg=10.0, angle_deg=10.0):
    """An l3d_plane_params.  cos_max None: cos(angle_min_deg pi / 180), the junctions' own; cos_min None: cos(angle_deg pi / 180); both in double"""
    import math
    p = PlaneParams()
    p.cos_max = math.cos(angle_min_deg * math.pi / 180.0) if cos_max is None else float(cos_max)
    p.cos_min = math.cos(angle_deg * math.pi / 180.0) if cos_min is None else float(cos_min)
    p.min_lines = int(min_lines)
    p.pad = 0
    return p


def _plane_call(fn, head, lines, tol, seeds, prm):
    """the argument list the plane calls share (head: the context, or nothing) -> (rc, dict(planes: PLANE array, members: PLANE_MEMBER array,
    hyp_plane (m,) int32, counts (8,) int32)).  lines or seeds None or an int: passed as NULL with that count, for the refusals"""
    if lines is None or isinstance(lines, int):
        n, lp = int(lines or 0), None
        tol = None if tol is None else np.ascontiguousarray(tol, np.float64).reshape(-1)
    else:
        lines = np.ascontiguousarray(lines, np.float64).reshape(-1, 6)
        n, lp = len(lines), (_p(lines) if len(lines) else None)
        tol = None if tol is None else np.ascontiguousarray(tol, np.float64).reshape(-1)
        if tol is not None and len(tol) != n:
            raise ValueError("plane lines: one tolerance per line")
    if seeds is None or isinstance(seeds, int):
        m, sp = int(seeds or 0), None
    else:
        seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1, 2)
        m, sp = len(seeds), (_p(seeds) if len(seeds) else None)
    tp = None if tol is None or len(tol) == 0 else _p(tol)
    hyp_plane = np.zeros(max(1, m) if sp is not None else 1, np.int32)
    counts = np.zeros(8, np.int32)
    pl, mem, npl, nm = C.POINTER(Plane)(), C.POINTER(PlaneMember)(), C.c_int(0), C.c_int(0)
    rc = fn(*head, lp, tp, C.c_int(n), sp, C.c_int(m), None if prm is None else C.byref(prm), C.byref(pl), C.byref(npl), C.byref(mem), C.byref(nm), _p(hyp_plane),
            _p(counts))
    if rc != 0:
        return rc, None
    planes = np.frombuffer(C.string_at(pl, npl.value * 128), PLANE).copy() if npl.value else np.zeros(0, PLANE)
    members = np.frombuffer(C.string_at(mem, nm.value * 16), PLANE_MEMBER).copy() if nm.value else np.zeros(0, PLANE_MEMBER)
    lib = load_library()
    lib.l3d_free(pl)
    lib.l3d_free(mem)
    return 0, dict(planes=planes, members=members, hyp_plane=hyp_plane[:max(0, m)].copy(), counts=counts)


def plane_lines_host(lines, tol, seeds, cos_max=None, cos_min=None, min_lines=3, params=None):
    """l3d_test_plane_lines_host: the planes of 3-D lines on the host -- no context, no device.  Arguments and result as Context.plane_lines.
    A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_plane_last_error.restype = C.c_char_p
    rc, out = _plane_call(lib.l3d_test_plane_lines_host, (), lines, tol, seeds, plane_params(cos_max, cos_min, min_lines) if params is None else params)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_plane_last_error().decode()))
        e.code = rc
        raise e
    return out


class SupportParams(C.Structure):
    """l3d_support_params (include/line3d_amd.h)"""
    _fields_ = [("dist_px", C.c_double), ("cos_min", C.c_double), ("min_overlap", C.c_double), ("near_z", C.c_double), ("margin", C.c_double)]


class SupportRecord(C.Structure):
    """l3d_support_record: 16 bytes"""
    _fields_ = [("seg3d", C.c_int32), ("seg2d", C.c_int32), ("dist", C.c_float), ("overlap", C.c_float)]


class LineSupport(C.Structure):
    """l3d_line_support: 24 bytes"""
    _fields_ = [("view_id", C.c_uint32), ("seg", C.c_uint32), ("seg3d", C.c_int32), ("dist", C.c_float), ("overlap", C.c_float), ("flags", C.c_uint32)]


LINE_SUPPORT = np.dtype([("view_id", np.uint32), ("seg", np.uint32), ("seg3d", np.int32), ("dist", np.float32), ("overlap", np.float32), ("flags", np.uint32)])
SUPPORT_MEMBER, SUPPORT_MEMBER_ELSEWHERE, SUPPORT_BEST = 1, 2, 4
SUPPORT_RECORD = np.dtype([("seg3d", np.int32), ("seg2d", np.int32), ("dist", np.float32), ("overlap", np.float32)])


def support_params(dist_px=3.0, cos_min=None, min_overlap=0.5, near_z=1e-6, margin=None, angle_deg=5.0):
    """An l3d_support_params.  cos_min None: cos(angle_deg pi / 180), in double; margin None: dist_px"""
    import math
    p = SupportParams()
    p.dist_px = float(dist_px)
    p.cos_min = math.cos(angle_deg * math.pi / 180.0) if cos_min is None else float(cos_min)
    p.min_overlap = float(min_overlap)
    p.near_z = float(near_z)
    p.margin = float(dist_px) if margin is None else float(margin)
    return p


def support_columns(segments_per_camera):
    """a list of (k, 4) float32 arrays, one per camera -> (all of them one after the other (T, 4), seg_start (m + 1,) int64)"""
    per = [np.ascontiguousarray(s, np.float32).reshape(-1, 4) for s in segments_per_camera]
    start = np.zeros(len(per) + 1, np.int64)
    if per:
        start[1:] = np.cumsum([len(s) for s in per])
    return (np.concatenate(per) if per else np.zeros((0, 4), np.float32)), start


def _support_call(fn, head, seg_ptr, n, cams, m, seg2d_ptr, start, prm):
    """the argument list the support calls share (head: the context, or nothing) -> (rc, dict(records: SUPPORT_RECORD array, cam_start (m + 1,) int64,
    best (seg_start[m],) int32, counts (4,) int64: rows, eligible columns, records, columns with a best row))"""
    rec = C.POINTER(SupportRecord)()
    cam_start = np.zeros(max(0, m) + 1, np.int64)
    T = int(start[-1]) if start is not None and len(start) and m > 0 else 0
    best = np.zeros(max(1, T), np.int32)
    counts = np.zeros(4, np.int64)
    rc = fn(*head, seg_ptr, C.c_int(n), cams, C.c_int(m), seg2d_ptr, None if start is None else _p(start), None if prm is None else C.byref(prm),
            C.byref(rec), _p(cam_start), _p(best), _p(counts))
    if rc != 0:
        return rc, None
    k = int(counts[2])
    records = np.frombuffer(C.string_at(rec, k * 16), SUPPORT_RECORD).copy() if k else np.zeros(0, SUPPORT_RECORD)
    load_library().l3d_free(rec)
    return 0, dict(records=records, cam_start=cam_start, best=best[:max(0, T)].copy(), counts=counts)


def support_lines_host(seg3d, cams, segments_per_camera, params=None):
    """l3d_test_support_lines_host: the support search on the host -- no context, no device.  Arguments and result as Context.support_lines (host arrays
    only).  A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_support_last_error.restype = C.c_char_p
    s, arr, m = _project_arguments(seg3d, cams)
    cols, start = support_columns(segments_per_camera)
    if len(start) != m + 1:
        raise ValueError("support lines: one array of 2-D segments per camera")
    rc, out = _support_call(lib.l3d_test_support_lines_host, (), _p(s) if len(s) else None, len(s), arr if m else None, m, _p(cols) if len(cols) else None, start,
                            support_params() if params is None else params)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_support_last_error().decode()))
        e.code = rc
        raise e
    return out


SELECT_ALL, SELECT_OBSERVED = 0, 1
LAYER_MEMBERS, LAYER_MODEL = 1, 2


class OverlayStyle(C.Structure):
    """l3d_overlay_style (include/line3d_amd.h)"""
    _fields_ = [("layers", C.c_int32), ("select", C.c_int32), ("by_line", C.c_int32), ("opacity", C.c_int32), ("width_members", C.c_double),
                ("width_model", C.c_double), ("near_z", C.c_double), ("color_members", C.c_ubyte * 4), ("color_model", C.c_ubyte * 4), ("palette", C.c_void_p),
                ("n_palette", C.c_int32), ("pad", C.c_int32)]


def default_palette():
    """l3d_default_palette: (12, 4) uint8"""
    lib = load_library()
    lib.l3d_default_palette.restype = C.POINTER(C.c_ubyte)
    return np.ctypeslib.as_array(lib.l3d_default_palette(), (12, 4)).copy()


def overlay_style(layers=("members", "model"), select="observed", by_line=True, opacity=255, width_members=1.0, width_model=2.0, near=1e-6,
                  color_members=(0, 255, 0, 255), color_model=(255, 0, 0, 255), palette=None):
    """An l3d_overlay_style.  layers: names out of "members", "model" (or a bit mask); select: "all", "observed" (or a number); palette: None (the
    default of 12 colours) or (n, 4) uint8, kept alive on the returned object"""
    st = OverlayStyle()
    names = {"members": LAYER_MEMBERS, "model": LAYER_MODEL}
    st.layers = int(layers) if isinstance(layers, (int, np.integer)) else sum(names[str(v).lower()] for v in layers)
    st.select = {"all": SELECT_ALL, "observed": SELECT_OBSERVED}[select.lower()] if isinstance(select, str) else int(select)
    st.by_line, st.opacity = int(bool(by_line)), int(opacity)
    st.width_members, st.width_model, st.near_z = float(width_members), float(width_model), float(near)
    st.color_members[:] = [int(v) for v in color_members]
    st.color_model[:] = [int(v) for v in color_model]
    if palette is not None:
        pal = np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
        st.palette, st.n_palette = pal.ctypes.data if len(pal) else None, len(pal)
        st._keep = pal
    return st


def _draw_image_copy(image):
    """A copy of a uint8 image to draw on.  Rows that lie further apart than their pixels (a view into a wider array) keep their stride: the copy
    is a view into a buffer of its own whose padding bytes are 0xa5 (out.base), so that a test can see them untouched"""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise TypeError("image must be a uint8 array H x W or H x W x C")
    ch = 1 if a.ndim == 2 else a.shape[2]
    row = a.shape[1] * ch
    if a.shape[0] > 1 and a.strides[1] == ch and (a.ndim == 2 or a.strides[2] == 1) and a.strides[0] > row:
        buf = np.full((a.shape[0], a.strides[0]), 0xA5, np.uint8)
        out = buf[:, :row].reshape(a.shape)
        out[...] = a
        return out
    return np.array(a, dtype=np.uint8, order="C", copy=True)


def _draw_arguments(segments, colors, color_index):
    s = np.ascontiguousarray(segments, np.float32).reshape(-1, 4)
    col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
    idx = None if color_index is None else np.ascontiguousarray(color_index, np.int32).reshape(-1)
    if idx is not None and len(idx) != len(s):
        raise ValueError("color_index has one entry per segment")
    return s, col, idx


def draw_segments_host(image, segments, colors, color_index=None, width_px=1.0, opacity=255):
    """l3d_test_draw_segments_host: the drawing's arithmetic on the host -- no context, no device.  Arguments and result as
    Context.draw_segments with a numpy image.  A refusal raises L3DError carrying the status in .code."""
    lib = load_library()
    lib.l3d_draw_last_error.restype = C.c_char_p
    out = _draw_image_copy(image)
    ptr, w, h, ch, stride = image_arguments(out)
    s, col, idx = _draw_arguments(segments, colors, color_index)
    rc = lib.l3d_test_draw_segments_host(ptr, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), _p(s) if len(s) else None, C.c_int(len(s)),
                                         _p(col) if len(col) else None, C.c_int(len(col)), None if idx is None else _p(idx), C.c_double(width_px), C.c_int(opacity))
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_draw_last_error().decode()))
        e.code = rc
        raise e
    return out


def covisibility_arguments(lists):
    """The views' world point lists -> (point_ids uint32, list_start int64 of len(lists) + 1): the lists one after the other, in add order"""
    arrs = [np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in lists]
    start = np.zeros(len(arrs) + 1, np.int64)
    if arrs:
        start[1:] = np.cumsum([len(a) for a in arrs])
    ids = np.concatenate(arrs + [np.zeros(1, np.uint32)])           # (one spare element: never a null pointer)
    return ids, start


def _covisibility_call(fn, head, ids, start, n_lists):
    """the argument list the co-visibility calls share (head: the context, or nothing) -> (rc, (num_wps, row_start, col, count, path))"""
    num, rs = C.POINTER(C.c_uint32)(), C.POINTER(C.c_int32)()
    col, cnt, path = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_int(-1)
    rc = fn(*head, ids, start, C.c_int(n_lists), C.byref(num), C.byref(rs), C.byref(col), C.byref(cnt), C.byref(path))
    if rc != 0:
        return rc, None
    n = max(0, n_lists)
    row_start = np.ctypeslib.as_array(rs, (n + 1,)).copy()
    nnz = int(row_start[n])
    out = (np.ctypeslib.as_array(num, (n,)).copy() if n else np.zeros(0, np.uint32), row_start,
           np.ctypeslib.as_array(col, (nnz,)).copy() if nnz else np.zeros(0, np.int32),
           np.ctypeslib.as_array(cnt, (nnz,)).copy() if nnz else np.zeros(0, np.uint32), path.value)
    lib = load_library()
    for q in (num, rs, col, cnt):
        lib.l3d_free(q)
    return 0, out


def covisibility_host(lists):
    """l3d_test_covisibility_host: the views' world point lists through Line3D::processWorldpointList itself, in add order -- no context, no device.
    -> (num_wps (V,) uint32, row_start (V + 1,) int32, col int32, count uint32, path): the non-zero common_wps as a CSR over list indices"""
    lib = load_library()
    lib.l3d_covis_last_error.restype = C.c_char_p
    ids, start = covisibility_arguments(lists)
    rc, out = _covisibility_call(lib.l3d_test_covisibility_host, (), _p(ids), _p(start), len(start) - 1)
    if rc != 0:
        e = L3DError("line3d_amd error %d: %s" % (rc, lib.l3d_covis_last_error().decode()))
        e.code = rc
        raise e
    return out


def rt_lanes(opt: int, avg_run: float) -> int:
    """l3d_test_rt_lanes: the lanes that share a run on the chain's run-table route for option rt_g = opt -- host only, no context, no device"""
    return int(load_library().l3d_test_rt_lanes(C.c_int(int(opt)), C.c_double(float(avg_run))))


def arena_regrow(arena_cap, kept_base, n_want, done, span, free_bytes, turn_room, early, products) -> dict:
    """l3d_test_arena_regrow: the size the chain grows its kept arena to after an overflow (free_bytes 2**64 - 1: not known) -- host only, no
    context, no device.  -> dict(ok, new_cap, need, fits, per_rec, reserve); ok False: the chain would fail with L3D_ERR_NOMEM"""
    out = (C.c_uint64 * 5)()
    rc = load_library().l3d_test_arena_regrow(C.c_uint64(arena_cap), C.c_uint64(kept_base), C.c_int(n_want), C.c_int(done), C.c_int(span),
                                              C.c_uint64(free_bytes), C.c_uint64(turn_room), C.c_int(bool(early)), C.c_int(bool(products)), out)
    if rc not in (0, 3):
        raise L3DError("l3d_test_arena_regrow: error %d" % rc)
    return dict(ok=rc == 0, new_cap=int(out[0]), need=int(out[1]), fits=int(out[2]), per_rec=int(out[3]), reserve=int(out[4]))


def blocks_verdict(n_views, world, check, tail, partition, hash, n_kept, comp_from, verified, S_src, window=0, neighbour_reach=0) -> dict:
    """l3d_test_blocks_verdict: the rules of matchViews sharded by blocks of views on a table of digests (hash, n_kept: world x n_views) -- host only,
    no context, no device.  -> dict(begin, owner, reach, miss, first_diff, n_miss, hopeless, failed_rank, t_rec, t_seg, t_first, max_rec, max_seg)"""
    h = np.ascontiguousarray(hash, dtype=np.uint64).reshape(world, n_views)
    nk = np.ascontiguousarray(n_kept, dtype=np.int32).reshape(world, n_views)
    cf, ver, ss = (np.ascontiguousarray(a, dtype=np.int32) for a in (comp_from, verified, S_src))
    assert len(cf) == world and len(ver) == n_views and len(ss) == n_views
    begin, owner, reach = np.zeros(world + 1, np.int32), np.zeros(n_views, np.int32), np.zeros(3, np.int32)
    miss, first_diff, summary, t_first = np.zeros(world, np.int32), np.zeros(world, np.int32), np.zeros(3, np.int32), np.zeros(world, np.int32)
    t_rec, t_seg, maxima = np.zeros(world, np.int64), np.zeros(world, np.int64), np.zeros(2, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = load_library().l3d_test_blocks_verdict(C.c_int(n_views), C.c_int(world), C.c_int(window), C.c_int(neighbour_reach), C.c_int(check), C.c_int(tail), C.c_int(bool(partition)),
                                                p(h), p(nk), p(cf), p(ver), p(ss), p(begin), p(owner), p(reach), p(miss), p(first_diff), p(summary), p(t_rec), p(t_seg), p(t_first), p(maxima))
    if rc:
        raise L3DError("l3d_test_blocks_verdict: error %d" % rc)
    return dict(begin=begin.tolist(), owner=owner.tolist(), reach=tuple(reach.tolist()), miss=miss.tolist(), first_diff=first_diff.tolist(), n_miss=int(summary[0]),
                hopeless=bool(summary[1]), failed_rank=int(summary[2]), t_rec=t_rec.tolist(), t_seg=t_seg.tolist(), t_first=t_first.tolist(), max_rec=int(maxima[0]), max_seg=int(maxima[1]))


def _i64(values):
    return (C.c_int64 * len(values))(*[int(v) for v in values])


def _shard_plan(geom=None, ring=None, pairs=0.0, guess=None, verdict=None, retry=None):
    """l3d_test_shard_plan on the sections given -> (geom_out, ring_out, guess_out, verdict rc, text, retry_out)"""
    geom_out, ring_out, guess_out, retry_out = (C.c_int64 * 10)(), (C.c_int32 * 3)(), (C.c_int64 * 2)(), (C.c_int64 * 5)()
    vrc, text = C.c_int32(0), C.create_string_buffer(1024)
    rc = load_library().l3d_test_shard_plan(_i64(geom) if geom else None, geom_out, _i64(ring) if ring else None, ring_out, C.c_double(float(pairs)),
                                            _i64(guess) if guess else None, guess_out, _i64(verdict) if verdict else None, C.byref(vrc), text, C.c_int(len(text)),
                                            _i64(retry) if retry else None, retry_out)
    if rc:
        raise L3DError("l3d_test_shard_plan: error %d" % rc)
    return list(geom_out), list(ring_out), list(guess_out), int(vrc.value), text.value.decode(), list(retry_out)


def shard_slot_geometry(maxS, maxN, world, slot_records, slot_cams_min, n_views) -> dict:
    """l3d_test_shard_plan, geometry: the layout of a slot of the segment-sharded run -- host only, no context, no device"""
    keys = ("seg_cap", "best_off", "bpos_off", "rec_off", "cam_off", "rt_off", "slot_bytes", "stage_bytes", "ring", "max_n")
    return dict(zip(keys, _shard_plan(geom=(maxS, maxN, world, slot_records, slot_cams_min, n_views))[0]))


def shard_ring_plan(n_views, window, block_bytes, slot_ring, partition, host_commit) -> dict:
    """l3d_test_shard_plan, ring plan: whether the gathered blocks of a run live in a ring, and how long it is"""
    out = _shard_plan(ring=(n_views, window, block_bytes, slot_ring, bool(partition), bool(host_commit)))[1]
    return dict(ring_mode=bool(out[0]), ring_views=out[1], send_ring=out[2])


def shard_arena_first_guess(pairs, world, test_cap, seen_cap, arena_guess, free_bytes, regrow_free_mb, partition, kept_views, n_views, part_seen):
    """l3d_test_shard_plan, first guess: (records of the compact kept arena's first guess, room in records under regrow_free_mb); free_bytes -1: not known"""
    out = _shard_plan(pairs=pairs, guess=(world, test_cap, seen_cap, arena_guess, free_bytes, regrow_free_mb, bool(partition), kept_views, n_views, part_seen))[2]
    return out[0], out[1]


def shard_verdict(bits, max_cand, max_kept, arena_total):
    """l3d_test_shard_plan, verdict: (return code, error text) of a run whose gathered overflow bits are `bits`"""
    out = _shard_plan(verdict=(bits, max_cand, max_kept, arena_total))
    return out[3], out[4]


def shard_retry(bits, cand_cap, max_cand, slot_records, max_kept, arena_needed, room, replay) -> dict:
    """l3d_test_shard_plan, retry: what l3d_line3d_shard_run does with a capacity verdict"""
    out = _shard_plan(retry=(bits, cand_cap, max_cand, slot_records, max_kept, arena_needed, room, bool(replay)))[5]
    return dict(retry=bool(out[0]), cand_cap_next=out[1], slot_records_next=out[2], arena_cap_next=out[3], refuse_for_room=bool(out[4]))


def shard_retire(n_views, window, slot_ring, partition, apart) -> dict:
    """l3d_test_shard_retire: the retirement schedule of a ring-mode run over all its views -- host only, no context, no device.
    -> dict(ring_mode, ring, retired_at, waited_at, batches [(first, count, enqueued at view, waited before)], retired, waited, outstanding)"""
    n = max(0, n_views)
    max_batches = n // 16 + n + 2
    retired_at, waited_at = np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.int32)
    batches, summary = np.zeros((max_batches, 4), np.int32), np.zeros(6, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = load_library().l3d_test_shard_retire(C.c_int(n_views), C.c_int(window), C.c_int(slot_ring), C.c_int(bool(partition)), C.c_int(bool(apart)), p(retired_at), p(waited_at),
                                              p(batches), C.c_int(max_batches), p(summary))
    if rc:
        raise L3DError("l3d_test_shard_retire: error %d" % rc)
    return dict(ring_mode=bool(summary[0]), ring=int(summary[1]), retired_at=retired_at[:n].tolist(), waited_at=waited_at[:n].tolist(),
                batches=[tuple(int(x) for x in b) for b in batches[:int(summary[2])]], retired=int(summary[3]), waited=int(summary[4]), outstanding=bool(summary[5]))


# dtype codes of l3d_device_image (L3D_U8 ...)
U8, U16, F16, F32 = 0, 1, 2, 3
_TYPESTR = {"|u1": U8, "<u2": U16, "<f2": F16, "<f4": F32}
_ELEMENT_BYTES = {U8: 1, U16: 2, F16: 2, F32: 4}


class DeviceImage(C.Structure):
    """l3d_device_image (include/line3d_amd.h): an image in device memory, where it lies and how it converts to the detector's 8 bits"""
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("dtype", C.c_int),
                ("stride_y", C.c_longlong), ("stride_x", C.c_longlong), ("stride_c", C.c_longlong), ("chan", C.c_int * 3), ("scale", C.c_float),
                ("stream", C.c_void_p)]


class DetectDeviceEntry(C.Structure):
    """l3d_detect_device_entry (include/line3d_amd.h)"""
    _fields_ = [("image", DeviceImage), ("new_width", C.c_int), ("new_height", C.c_int), ("min_length", C.c_float), ("max_segments", C.c_int),
                ("camera", C.c_void_p)]


class DeviceEntry(C.Structure):
    """l3d_device_entry (include/line3d_amd.h)"""
    _fields_ = [("image_id", C.c_uint32), ("image", DeviceImage), ("K", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p), ("dist", C.c_void_p),
                ("link_ids", C.c_void_p), ("sims", C.c_void_p), ("n_links", C.c_int)]


def is_device_object(obj):
    """a DeviceImage, or anything that carries __cuda_array_interface__ (torch device tensors do, on ROCm builds as well; a host tensor does not)"""
    return isinstance(obj, DeviceImage) or hasattr(obj, "__cuda_array_interface__")


def all_device_objects(images, what):
    """True: every image of the list is a device object; False: none is.  A list that mixes the two raises ValueError -- before any library call"""
    kinds = [is_device_object(im) for im in images]
    if any(kinds) and not all(kinds):
        raise ValueError("%s: a list mixes images in device memory with host images or files; give them in separate calls" % what)
    return bool(kinds) and all(kinds)


def device_image(obj, layout=None, chan=None, scale=None, stream=None):
    """The l3d_device_image of anything with __cuda_array_interface__ (a DeviceImage passes through).  Layout: 2-D is H x W; 3-D with a last
    dimension of 1, 3 or 4 is H x W x C (an ambiguous 3 x 5 x 3 too) unless layout="CHW" says planar.  Strides come from the interface's
    bytes (ValueError when they are no whole elements); typestr |u1, <u2, <f2, <f4 (TypeError otherwise).  chan defaults to (0, 1, 2),
    scale to 255 for the float types, 1 / 257 for 16-bit integers and 1 for 8-bit.  stream: an integer handle or an object with .cuda_stream;
    None: the current stream of a torch tensor's device, else the interface's `stream` entry, else the null stream.  The object is kept
    alive on the descriptor."""
    if isinstance(obj, DeviceImage):
        return obj
    iface = obj.__cuda_array_interface__
    typestr = str(iface["typestr"])
    if typestr not in _TYPESTR:
        raise TypeError("device image: typestr %r is not one of |u1, <u2, <f2, <f4" % typestr)
    dtype = _TYPESTR[typestr]
    es = _ELEMENT_BYTES[dtype]
    shape = tuple(int(v) for v in iface["shape"])
    strides = iface.get("strides")
    if strides is None:                 # contiguous, C order
        strides, acc = [], es
        for dim in reversed(shape):
            strides.insert(0, acc)
            acc *= dim
    strides = [int(v) for v in strides]
    if any(v % es for v in strides):
        raise ValueError("device image: byte strides %s are no whole elements of %d bytes" % (strides, es))
    strides = [v // es for v in strides]
    if layout not in (None, "HWC", "CHW", "HW"):
        raise ValueError("device image: layout must be None, 'HW', 'HWC' or 'CHW'")
    if len(shape) == 2 and layout in (None, "HW"):
        layout, (h, w), ch = "HW", shape, 1
        sy, sx, sc = strides[0], strides[1], 0
    elif len(shape) == 3 and layout == "CHW":
        ch, h, w = shape
        sc, sy, sx = strides
    elif len(shape) == 3 and layout in (None, "HWC"):
        if layout is None and shape[2] not in (1, 3, 4):
            raise ValueError("device image: a shape of %s is no H x W x C image of 1, 3 or 4 channels; planar images pass layout='CHW'" % (shape,))
        layout, (h, w, ch) = "HWC", shape
        sy, sx, sc = strides
    else:
        raise ValueError("device image: a shape of %s does not fit layout %r" % (shape, layout))
    d = DeviceImage()
    d.ptr = int(iface["data"][0]) or None
    d.width, d.height, d.channels, d.dtype = w, h, ch, dtype
    d.stride_y, d.stride_x, d.stride_c = sy, sx, sc
    chan = (0, 1, 2) if chan is None else tuple(int(v) for v in chan)
    if len(chan) != 3:
        raise ValueError("device image: chan has three entries")
    d.chan[0], d.chan[1], d.chan[2] = chan
    d.scale = float(scale) if scale is not None else {U8: 1.0, U16: 1.0 / 257.0}.get(dtype, 255.0)
    if stream is None:
        if type(obj).__module__.split(".")[0] == "torch":
            import torch
            stream = torch.cuda.current_stream(obj.device).cuda_stream
        else:
            stream = iface.get("stream")
            stream = 0 if stream in (None, 1) else int(stream)         # (the interface's 1 is the legacy default stream)
    elif hasattr(stream, "cuda_stream"):
        stream = stream.cuda_stream
    d.stream = int(stream) or None
    d._keep, d._layout, d._shape = obj, layout, shape
    return d


def device_image_check(d):
    """l3d_device_image_check (no device): (status, message) for a descriptor's fields"""
    msg = C.create_string_buffer(256)
    rc = load_library().l3d_device_image_check(C.byref(d), msg, C.c_size_t(256))
    return int(rc), msg.value.decode()


def device_image_extent(d):
    """l3d_device_image_extent (no device): (status, lo, hi) -- the lowest and one past the highest byte offset from ptr the image addresses"""
    lo, hi = C.c_longlong(0), C.c_longlong(0)
    rc = load_library().l3d_device_image_extent(C.byref(d), C.byref(lo), C.byref(hi))
    return int(rc), int(lo.value), int(hi.value)


def detect_device_entries(images, new_sizes=None, min_lengths=None, max_segments=3000, cameras=None, lenses=None, out_sizes=None):
    """The l3d_detect_device_entry array of Context.detect_segments_batch for a list of device objects, and what keeps its pointers alive"""
    images = [device_image(im) for im in images]
    n = len(images)
    new_sizes, min_lengths, cameras = _per_image(new_sizes, n, "new_sizes"), _per_image(min_lengths, n, "min_lengths"), _per_image(cameras, n, "cameras")
    lenses, out_sizes = _per_image(lenses, n, "lenses"), _per_image(out_sizes, n, "out_sizes")
    caps = [int(max_segments)] * n if np.isscalar(max_segments) else [int(v) for v in _per_image(max_segments, n, "max_segments")]
    entries, keep = (DetectDeviceEntry * max(1, n))(), list(images)
    for i, im in enumerate(images):
        e = entries[i]
        e.image = im
        w, h = (im.width, im.height) if out_sizes[i] is None else (int(out_sizes[i][0]), int(out_sizes[i][1]))       # (a remap's output: what the detector sees)
        e.new_width, e.new_height = (w, h) if new_sizes[i] is None else (int(new_sizes[i][0]), int(new_sizes[i][1]))
        e.min_length = float(np.float32(0.005) * np.sqrt(np.float32(h * h + w * w))) if min_lengths[i] is None else float(min_lengths[i])
        e.max_segments = caps[i]
        if lenses[i] is not None:
            cam = _lens_camera(lenses[i], cameras[i])
            keep.append(cam)
            e.camera = C.addressof(cam)
        elif cameras[i] is not None:
            if len(cameras[i]) != 6:
                raise ValueError("camera must be (fx, fy, cx, cy, k1, k2)")
            cam = (C.c_double * 6)(*[float(v) for v in cameras[i]])
            keep.append(cam)
            e.camera = C.addressof(cam)
    return entries, keep


def device_output_like(d, device_index=0):
    """A zero-filled torch uint8 tensor of the shape the descriptor `d` was made from (an H x W[x 3] one for a hand-made descriptor) on its
    device, and its descriptor: same layout and chan, on the same stream -- where the ..._device output calls write"""
    import torch
    src = getattr(d, "_keep", None)
    shape = getattr(d, "_shape", None) or ((d.height, d.width) if d.channels == 1 else (d.height, d.width, 3))
    layout = getattr(d, "_layout", None)
    dev = src.device if src is not None and type(src).__module__.split(".")[0] == "torch" else "cuda:%d" % device_index
    out = torch.zeros(shape, dtype=torch.uint8, device=dev)
    o = device_image(out, layout=layout, chan=tuple(d.chan) if len(shape) == 3 else None, scale=1.0, stream=d.stream or 0)
    return out, o


class VerifyPath(C.Structure):
    """l3d_test_verify_path (include/line3d_amd.h)"""
    _fields_ = [("path", C.c_int32), ("gb", C.c_int32), ("split_unit", C.c_int32), ("mmax", C.c_int32), ("wide_max", C.c_int32),
                ("mmax_used", C.c_int32), ("kernels", C.c_uint32), ("pad", C.c_int32), ("seg_order", C.c_void_p),
                ("exist_cams", C.c_void_p), ("n_exist_cams", C.c_int32), ("pad2", C.c_int32), ("cand_meta_out", C.c_void_p), ("cand_depths_out", C.c_void_p)]


class PairPath(C.Structure):
    """l3d_test_pair_path (include/line3d_amd.h)"""
    _fields_ = [(n, C.c_int32) for n in ("path", "pretest", "spb", "seg_begin", "seg_end", "ray_tables", "cand_cap", "capacity",
                                          "needed", "total", "largest", "spb_used", "overflow", "pad")]


class ChainView(C.Structure):
    """l3d_chain_view (include/line3d_amd.h)"""
    _fields_ = [("view_id", C.c_uint32), ("src_segs", C.c_void_p), ("S_src", C.c_int32), ("RtKinv_src", C.c_void_p), ("C_src", C.c_void_p),
                ("tgt_segs", C.c_void_p), ("n_tgt", C.c_int32), ("offsets", C.c_void_p), ("N", C.c_int32), ("F", C.c_void_p), ("RtKinv", C.c_void_p),
                ("centers", C.c_void_p), ("P", C.c_void_p), ("to_be_matched", C.c_void_p), ("n_tbm", C.c_int32), ("local2global", C.c_void_p),
                ("source_cam", C.c_void_p), ("source_index", C.c_void_p), ("n_sources", C.c_int32),
                ("sigma_p", C.c_float), ("sigma_a", C.c_float), ("spatial_k", C.c_float)]


class DenseMap(C.Structure):
    """l3d_dense_map (include/line3d_amd.h)"""
    _fields_ = [("n_views", C.c_int32), ("view_ids", C.c_void_p), ("seg_base", C.c_void_p)]


SUMMARY_DTYPE = np.dtype([("verified", "<i4"), ("n_kept", "<i4"), ("n_candidates", "<i8"), ("median_depth", "<f4"), ("pad", "<i4")])   # l3d_chain_summary


class ProductsPath(C.Structure):
    """l3d_test_products_path (include/line3d_amd.h)"""
    _fields_ = [("side_arrays", C.c_int32), ("early_pairs", C.c_int32), ("dv0", C.c_int32), ("dv1", C.c_int32), ("held", C.c_void_p),
                ("block_capacity", C.c_int32), ("side_arrays_used", C.c_int32), ("build", C.c_int32), ("refused", C.c_int32), ("n_blocks", C.c_int32),
                ("max_touch", C.c_int32), ("early_cap", C.c_int32), ("early_g", C.c_int32),
                ("block_cap", C.c_void_p), ("block_staged", C.c_void_p), ("block_g", C.c_void_p)]


class CollectPath(C.Structure):
    """l3d_test_collect_path (include/line3d_amd.h)"""
    _fields_ = [("route", C.c_int32), ("rt_g", C.c_int32), ("sort_apart", C.c_int32), ("cand_cap", C.c_int32), ("avg_kept", C.c_double),
                ("overflowed", C.c_void_p), ("kernels", C.c_uint32), ("g", C.c_int32), ("bps", C.c_int32), ("blocks_move", C.c_int32),
                ("R", C.c_int32), ("pad", C.c_int32)]


# L3D_CK_*: the kernels a test_collect_candidates call launched
CK_EXIST_COUNT, CK_EXIST_COUNT_RT, CK_SCAN, CK_PLACE, CK_PLACE_RT, CK_SORT_RUNS = 1, 2, 4, 8, 16, 32


class KeptJob(C.Structure):
    """l3d_test_kept_job (include/line3d_amd.h)"""
    _fields_ = [("records", C.c_void_p), ("local2global", C.c_void_p), ("qt", C.c_void_p), ("rt", C.c_void_p),
                ("n", C.c_int32), ("S", C.c_int32), ("N", C.c_int32), ("pad", C.c_int32)]


class KeptPath(C.Structure):
    """l3d_test_kept_path (include/line3d_amd.h)"""
    _fields_ = [("writer", C.c_int32), ("has_prev", C.c_int32), ("prev_base", C.c_uint64), ("prev_n_kept", C.c_int32), ("cand_cap", C.c_int32),
                ("arena_cap", C.c_uint64), ("jobs", C.c_void_p), ("n_jobs", C.c_int32),
                ("n_kept", C.c_int32), ("R", C.c_int32), ("overflow", C.c_int32), ("n_want", C.c_int32), ("rebuild_err", C.c_int32),
                ("rebuild_blocks", C.c_int32), ("pad", C.c_int32), ("kept_base", C.c_uint64)]


class ShardGeom(C.Structure):
    """l3d_test_shard_geom (include/line3d_amd.h)"""
    _fields_ = [("maxS", C.c_int32), ("maxN", C.c_int32), ("world", C.c_int32), ("slot_records", C.c_int32), ("slot_cams_min", C.c_int32),
                ("n_views", C.c_int32), ("ring", C.c_int32), ("pad", C.c_int32)]


class ShardCollectPath(C.Structure):
    """l3d_test_shard_collect_path (include/line3d_amd.h)"""
    _fields_ = [("s0", C.c_int32), ("s1", C.c_int32), ("cand_cap", C.c_int32), ("sort_apart", C.c_int32), ("slot_scan_grain", C.c_int32),
                ("wps", C.c_int32), ("blocks_move", C.c_int32), ("R", C.c_int32)]


class ShardPackIO(C.Structure):
    """l3d_test_shard_pack_io (include/line3d_amd.h)"""
    _fields_ = [("verified", C.c_void_p), ("keep", C.c_void_p), ("best_off", C.c_void_p), ("view_sn", C.c_void_p), ("rt_off", C.c_void_p),
                ("batches", C.c_void_p), ("n_batches", C.c_int32), ("retire_tables", C.c_int32), ("arena_cap", C.c_int64), ("pack_cap", C.c_int64),
                ("best_cap", C.c_int64), ("rt_cap", C.c_int64), ("stage", C.c_void_p), ("pack_hdr", C.c_void_p), ("totals", C.c_void_p),
                ("check", C.c_void_p), ("pa_arena", C.c_void_p), ("pa_best", C.c_void_p), ("pa_bestpos", C.c_void_p), ("rt_arena", C.c_void_p),
                ("rt_best", C.c_void_p), ("rt_bestpos", C.c_void_p), ("base_dev", C.c_void_p), ("hdr_all", C.c_void_p), ("overflow", C.c_void_p),
                ("qt_arena", C.c_void_p), ("rt_all", C.c_void_p)]


def shard_geom(geom) -> "ShardGeom":
    """the geometry inputs of the sharded chain's test hooks from a dict: maxS, maxN, world, slot_records, slot_cams_min, n_views and (optional) ring"""
    return ShardGeom(int(geom["maxS"]), int(geom["maxN"]), int(geom["world"]), int(geom["slot_records"]), int(geom["slot_cams_min"]), int(geom["n_views"]),
                     int(geom.get("ring", 0)), 0)


# l3d_test_products_path: build / refused
PROD_TRANSPOSED, PROD_SORTED = 1, 2
PROD_REFUSED_WIDE_VIEW, PROD_REFUSED_UNORDERED = 1, 2


# L3D_VK_*: the stage-2 kernels a test_verify_candidates call launched
VK_ALL_PAIRS, VK_SEG_POST, VK_WINDOW_256, VK_WINDOW_512, VK_WINDOW_GB, VK_BUILD, VK_WALK, VK_WALK_GB = 1, 2, 4, 8, 16, 32, 64, 128


def _per_image(value, n, what):
    """None, or one entry per image"""
    if value is None:
        return [None] * n
    value = list(value)
    if len(value) != n:
        raise ValueError("%s: %d entries for %d images" % (what, len(value), n))
    return value


def detect_entries(images, new_sizes=None, min_lengths=None, max_segments=3000, cameras=None, lenses=None, out_sizes=None):
    """The l3d_detect_entry array of Context.detect_segments_batch, and what keeps its pointers alive.  Everything malformed is refused here,
    before any device call: an image that is neither a uint8 array nor bytes, a camera that is not six numbers, lists of the wrong length."""
    images = list(images)
    n = len(images)
    new_sizes, min_lengths, cameras = _per_image(new_sizes, n, "new_sizes"), _per_image(min_lengths, n, "min_lengths"), _per_image(cameras, n, "cameras")
    lenses, out_sizes = _per_image(lenses, n, "lenses"), _per_image(out_sizes, n, "out_sizes")
    caps = [int(max_segments)] * n if np.isscalar(max_segments) else [int(v) for v in _per_image(max_segments, n, "max_segments")]
    entries, keep = (DetectEntry * max(1, n))(), []
    for i, img in enumerate(images):
        e = entries[i]
        if isinstance(img, (bytes, bytearray, memoryview)):
            ptr, nbytes = _bytes_arguments(img)
            try:
                w, h, _ = jpeg_info(img)
            except L3DError:                # the library refuses the entry with its own status and message
                w, h = 0, 0
            e.jpeg, e.jpeg_bytes = ptr.value, nbytes.value
        elif isinstance(img, np.ndarray):
            ptr, w, h, ch, stride = image_arguments(img)
            e.pixels, e.width, e.height, e.channels, e.row_stride = ptr.value, w, h, ch, stride
        else:
            raise TypeError("image %d must be a uint8 array or the bytes of a JPEG file" % i)
        keep.append(ptr)
        if out_sizes[i] is not None:            # a remap's output: what the detector sees
            w, h = int(out_sizes[i][0]), int(out_sizes[i][1])
        e.new_width, e.new_height = (w, h) if new_sizes[i] is None else (int(new_sizes[i][0]), int(new_sizes[i][1]))
        e.min_length = float(np.float32(0.005) * np.sqrt(np.float32(h * h + w * w))) if min_lengths[i] is None else float(min_lengths[i])
        e.max_segments = caps[i]
        if lenses[i] is not None:
            cam = _lens_camera(lenses[i], cameras[i])
            keep.append(cam)
            e.camera = C.addressof(cam)
        elif cameras[i] is not None:
            if len(cameras[i]) != 6:
                raise ValueError("camera must be (fx, fy, cx, cy, k1, k2)")
            cam = (C.c_double * 6)(*[float(v) for v in cameras[i]])
            keep.append(cam)
            e.camera = C.addressof(cam)
    return entries, keep


class AffinityInput(C.Structure):
    """l3d_affinity_input (include/line3d_amd.h)"""
    _fields_ = [("n_views", C.c_int32), ("seg_base", C.c_void_p), ("view_hyp_begin", C.c_void_p), ("n_hyp", C.c_int32),
                ("hyp", C.c_void_p), ("score", C.c_void_p), ("hyp_dense", C.c_void_p), ("best", C.c_void_p),
                ("pot_start", C.c_void_p), ("pot_tgt", C.c_void_p), ("coll_start", C.c_void_p), ("coll_other", C.c_void_p),
                ("coll_w", C.c_void_p), ("sigma_a", C.c_float)]


class AffinityPart(C.Structure):
    """l3d_test_affinity_part (include/line3d_amd.h)"""
    _fields_ = [("h0", C.c_int32), ("h1", C.c_int32), ("pos_base", C.c_uint64), ("loc2glob", C.c_void_p), ("assume_symmetric", C.c_int32),
                ("n_launches", C.c_int32), ("coll_sym", C.c_int32), ("pad", C.c_int32), ("n_candidates", C.c_int64), ("n_passed", C.c_int64)]


class Context:
    """One GPU, one stream, grow-only device arenas (l3d_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.l3d_ctx_create(C.c_int(device), C.byref(h))
        if rc != 0:
            raise L3DError("l3d_ctx_create failed (code %d): no usable MI355X / HIP device -- this package has no CPU fallback" % rc)
        self.h = h
        self.device = int(device)
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.lib.l3d_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            e = L3DError("line3d_amd error %d: %s" % (rc, self.lib.l3d_last_error(self.h).decode()))
            e.code = rc
            raise e

    # -- measurement --------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self.lib.l3d_profile_enable(self.h, C.c_int(1 if on else 0)))

    def profile_only(self, name: str | None):
        """Bracket only this kernel with HIP events (None: all)."""
        self._chk(self.lib.l3d_profile_only(self.h, (name or "").encode()))

    def profile_reset(self):
        self._chk(self.lib.l3d_profile_reset(self.h))

    def profile_get(self, name: str):
        n = C.c_int64(0)
        ms = C.c_double(0)
        self._chk(self.lib.l3d_profile_get(self.h, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_all(self):
        return {k: self.profile_get(k) for k in self.lib.l3d_profile_names().decode().split(";")}

    def test_sq_threshold(self, u: np.ndarray):
        u = np.ascontiguousarray(u, dtype=np.float32)
        a, b = np.zeros_like(u), np.zeros_like(u)
        self._chk(self.lib.l3d_test_sq_threshold(self.h, _p(u), C.c_int(len(u)), _p(a), _p(b)))
        return a, b

    def set_chain_capacities(self, cand_cap: int, arena_cap: int):
        self._chk(self.lib.l3d_set_chain_capacities(self.h, C.c_size_t(cand_cap), C.c_size_t(arena_cap)))

    def set_verify_lds_budget(self, nbytes: int):
        self._chk(self.lib.l3d_set_verify_lds_budget(C.c_size_t(nbytes)))

    def set_pair_pretest(self, on: bool):
        self._chk(self.lib.l3d_set_pair_pretest(self.h, C.c_int(3 if on is True else int(on))))

    def set_verify_mode(self, mode: int):
        self._chk(self.lib.l3d_set_verify_mode(self.h, C.c_int(mode)))

    def set_option(self, name: str, value: int):
        """A diagnostic / A-B switch of the context (l3d_options.hpp); the environment is read once, at context creation."""
        self._chk(self.lib.l3d_set_option(self.h, name.encode(), C.c_int(int(value))))

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        self._chk(self.lib.l3d_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def last_chain_routes(self):
        """l3d_last_chain_routes: (views that scanned their sources' records, views that read their sources' run tables) of the last resident chain"""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.lib.l3d_last_chain_routes(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_stats(self):
        s = (C.c_double * 4)()
        self._chk(self.lib.l3d_last_stats(self.h, s))
        return list(s)

    def register_segments(self, segs: np.ndarray):
        assert segs.dtype == np.float32 and segs.flags.c_contiguous
        self._keep.append(segs)
        self._chk(self.lib.l3d_register_segments(self.h, _p(segs), C.c_int(len(segs))))

    # -- line segment detection (l3d_detect.hip) --------------------------------------------------
    def undistort(self, img, K, k1=None, k2=None, lens=None, in_place=False, out_size=None, mask=None, border_mask=None, return_mask=False):
        """l3d_undistort_image: uint8 image H x W or H x W x 3 -> the undistorted image, same shape (initUndistortRectifyMap + remap of the drivers,
        the formulas of include/line3d_amd.h).  K: 3 x 3, its fx, fy, cx, cy are used; k1, k2: OpenCV-convention radial coefficients.
        A device object (device_image) stays on the device (l3d_undistort_image_device): the result is a torch uint8 tensor of the input's
        shape on its device.
        lens (capi.lens(...)) in the place of k1, k2: l3d_undistort_image[_device]_lens -- tangential, rational and fisheye models, resampled from
        the lens's source camera onto K.  in_place (with a lens): a host array is overwritten and returned, a device object is its own output.
        out_size, mask, border_mask, return_mask (any of them: l3d_undistort_image[_device]_remap, "A REMAP"): the output has out_size =
        (width, height); mask (capi.remap's) is the caller's validity in the source grid; return_mask: -> (image, validity plane), the plane
        H' x W' uint8 with 255 = valid -- a torch tensor where the image is one."""
        K = np.asarray(K, dtype=np.float64).reshape(3, 3)
        if out_size is not None or mask is not None or border_mask is not None or return_mask:
            if k1 is not None or k2 is not None or in_place:
                raise ValueError("out_size, mask, border_mask and return_mask go with a lens (or none), not with k1, k2 or in_place")
            return self._undistort_remap(img, K, lens, out_size, mask, border_mask, return_mask)
        if lens is not None:
            if k1 is not None or k2 is not None:
                raise ValueError("undistort takes k1, k2 or a lens, not both")
            return self._undistort_lens(img, K, lens, in_place)
        if k1 is None or k2 is None or in_place:
            raise ValueError("undistort needs k1 and k2, or a lens (in_place goes with a lens)")
        if is_device_object(img):
            d = device_image(img)
            out, o = device_output_like(d, getattr(self, "device", 0))
            self._chk(self.lib.l3d_undistort_image_device(self.h, C.byref(d), C.c_double(K[0, 0]), C.c_double(K[1, 1]), C.c_double(K[0, 2]), C.c_double(K[1, 2]),
                                                          C.c_double(float(k1)), C.c_double(float(k2)), C.byref(o)))
            return out
        pix, w, h, ch, stride = image_arguments(img)
        out = np.zeros(np.asarray(img).shape, np.uint8)
        self._chk(self.lib.l3d_undistort_image(self.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), C.c_double(K[0, 0]), C.c_double(K[1, 1]),
                                               C.c_double(K[0, 2]), C.c_double(K[1, 2]), C.c_double(float(k1)), C.c_double(float(k2)), _p(out),
                                               C.c_size_t(w * ch)))
        return out

    def _undistort_remap(self, img, K, lens_, out_size, mask, border_mask, return_mask):
        cam = [C.c_double(K[0, 0]), C.c_double(K[1, 1]), C.c_double(K[0, 2]), C.c_double(K[1, 2])]
        if is_device_object(img):
            import torch
            d = device_image(img)
            r = remap(lens_, out_size, mask, True if border_mask is None else border_mask)
            ow, oh = (d.width, d.height) if out_size is None else (int(out_size[0]), int(out_size[1]))
            src = getattr(d, "_keep", None)
            dev = src.device if src is not None and type(src).__module__.split(".")[0] == "torch" else "cuda:%d" % getattr(self, "device", 0)
            out = torch.zeros((max(oh, 0), max(ow, 0)) if d.channels == 1 else (max(oh, 0), max(ow, 0), 3), dtype=torch.uint8, device=dev)
            valid = torch.zeros((max(oh, 0), max(ow, 0)), dtype=torch.uint8, device=dev)
            o = device_image(out, chan=tuple(d.chan) if d.channels != 1 else None, scale=1.0, stream=d.stream or 0) if out.numel() else DeviceImage()
            v = device_image(valid, scale=1.0, stream=d.stream or 0) if valid.numel() else DeviceImage()
            self._chk(self.lib.l3d_undistort_image_device_remap(self.h, C.byref(d), *cam, C.byref(r), C.byref(o), C.byref(v) if return_mask else None))
            return (out, valid) if return_mask else out
        pix, w, h, ch, stride = image_arguments(img)
        r = remap_of(lens_, out_size, mask, border_mask, (w, h)) or remap(lens_)
        ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
        out = np.zeros((max(oh, 0), max(ow, 0)) + np.asarray(img).shape[2:], np.uint8)
        valid = np.zeros((max(oh, 0), max(ow, 0)), np.uint8)
        self._chk(self.lib.l3d_undistort_image_remap(self.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), *cam, C.byref(r), _p(out),
                                                     C.c_size_t(max(ow, 0) * ch), _p(valid) if return_mask else None, C.c_size_t(max(ow, 0))))
        return (out, valid) if return_mask else out

    def _undistort_lens(self, img, K, lens_, in_place):
        cam = [C.c_double(K[0, 0]), C.c_double(K[1, 1]), C.c_double(K[0, 2]), C.c_double(K[1, 2])]
        if is_device_object(img):
            d = device_image(img)
            out, o = (img, d) if in_place else device_output_like(d, getattr(self, "device", 0))
            self._chk(self.lib.l3d_undistort_image_device_lens(self.h, C.byref(d), *cam, C.byref(lens_), C.byref(o)))
            return out
        if in_place:
            a = np.asarray(img)
            pix, w, h, ch, stride = image_arguments(a)
            if pix._keep is not a:
                raise ValueError("in_place needs an array whose pixels are contiguous within a row")
            self._chk(self.lib.l3d_undistort_image_lens(self.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), *cam, C.byref(lens_), pix, C.c_size_t(stride)))
            return a
        pix, w, h, ch, stride = image_arguments(img)
        out = np.zeros(np.asarray(img).shape, np.uint8)
        self._chk(self.lib.l3d_undistort_image_lens(self.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), *cam, C.byref(lens_), _p(out), C.c_size_t(w * ch)))
        return out

    def detect_segments(self, img, new_size=None, min_length=None, max_segments=3000, camera=None, lens=None, out_size=None, mask=None, border_mask=None):
        """l3d_detect_segments: uint8 image H x W or H x W x 3 (contiguous pixels, rows contiguous or strided) -> (n, 4) float32 segments
        (x1, y1, x2, y2) in pixels of `img`, longest first.  new_size = (width, height) the detector works at (None: the image's own);
        min_length None: the reference's 0.005 x the image diagonal.  camera = (fx, fy, cx, cy, k1, k2): the image is undistorted on the device
        first (l3d_detect_segments_distorted) and the segments are in pixels of the undistorted image.
        A device object (a torch device tensor, anything with __cuda_array_interface__, a device_image descriptor) is read where it lies
        (l3d_detect_segments_device): the segments are those of the host call on the converted pixels.
        lens (capi.lens(...)): the image is undistorted with it first, onto camera = (fx, fy, cx, cy) (None: the lens's own source camera) -- a
        batch of one through l3d_detect_segments[_device]_batch_lens.  out_size, mask, border_mask: as detect_segments_batch's out_sizes, masks,
        border_masks -- a batch of one through l3d_detect_segments[_device]_batch_remap."""
        if out_size is not None or mask is not None or border_mask is not None:
            return self.detect_segments_batch([img], None if new_size is None else [new_size], None if min_length is None else [min_length], max_segments, [camera],
                                              lenses=[lens], out_sizes=[out_size], masks=[mask], border_masks=[border_mask])[0]
        if lens is not None:
            return self.detect_segments_batch([img], None if new_size is None else [new_size], None if min_length is None else [min_length], max_segments, [camera], lenses=[lens])[0]
        if is_device_object(img):
            d = device_image(img)
            w, h = d.width, d.height
            nw, nh = (w, h) if new_size is None else (int(new_size[0]), int(new_size[1]))
            if min_length is None:
                min_length = float(np.float32(0.005) * np.sqrt(np.float32(h * h + w * w)))
            cam = None
            if camera is not None:
                if len(camera) != 6:
                    raise ValueError("camera must be (fx, fy, cx, cy, k1, k2)")
                cam = (C.c_double * 6)(*[float(v) for v in camera])
            out, n = C.POINTER(C.c_float)(), C.c_int(0)
            self._chk(self.lib.l3d_detect_segments_device(self.h, C.byref(d), C.c_int(nw), C.c_int(nh), C.c_float(min_length), C.c_int(int(max_segments)), cam,
                                                          C.byref(out), C.byref(n)))
            segs = np.ctypeslib.as_array(out, (n.value, 4)).copy() if n.value else np.zeros((0, 4), np.float32)
            self.lib.l3d_free(out)
            return segs
        pix, w, h, ch, stride = image_arguments(img)
        nw, nh = (w, h) if new_size is None else (int(new_size[0]), int(new_size[1]))
        if min_length is None:
            min_length = float(np.float32(0.005) * np.sqrt(np.float32(h * h + w * w)))
        out, n = C.POINTER(C.c_float)(), C.c_int(0)
        if camera is not None:
            cam = [C.c_double(float(v)) for v in camera]
            if len(cam) != 6:
                raise ValueError("camera must be (fx, fy, cx, cy, k1, k2)")
            self._chk(self.lib.l3d_detect_segments_distorted(self.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), C.c_int(nw), C.c_int(nh),
                                                             C.c_float(min_length), C.c_int(int(max_segments)), *cam, C.byref(out), C.byref(n)))
        else:
            self._chk(self.lib.l3d_detect_segments(self.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), C.c_int(nw), C.c_int(nh),
                                                   C.c_float(min_length), C.c_int(int(max_segments)), C.byref(out), C.byref(n)))
        segs = np.ctypeslib.as_array(out, (n.value, 4)).copy() if n.value else np.zeros((0, 4), np.float32)
        self.lib.l3d_free(out)
        return segs

    # -- baseline JPEG input (l3d_jpeg.cpp, l3d_jpeg_device.hip) ------------------------------------
    def decode_jpeg(self, data, device=False):
        """l3d_decode_jpeg: the bytes of a baseline JPEG file -> uint8 H x W (grey) or H x W x 3 (B, G, R, as cv::imread gives them),
        byte-identical to libjpeg's default decoder.  device=True: the same pixels as a torch uint8 tensor on the context's device
        (l3d_decode_jpeg_device), readable from any stream when the call returns."""
        w, h, ch = jpeg_info(data)
        ptr, n = _bytes_arguments(data)
        if device:
            import torch
            out = torch.zeros((h, w) if ch == 1 else (h, w, ch), dtype=torch.uint8, device="cuda:%d" % getattr(self, "device", 0))
            o = device_image(out)
            self._chk(self.lib.l3d_decode_jpeg_device(self.h, ptr, n, C.byref(o)))
            return out
        out = np.zeros((h, w) if ch == 1 else (h, w, ch), np.uint8)
        self._chk(self.lib.l3d_decode_jpeg(self.h, ptr, n, _p(out), C.c_size_t(w * ch)))
        return out

    def detect_segments_jpeg(self, data, new_size=None, min_length=None, max_segments=3000, camera=None, lens=None, out_size=None, mask=None, border_mask=None):
        """l3d_detect_segments_jpeg: detect_segments on the image of a baseline JPEG file, decoded on the device (arguments as detect_segments)"""
        if out_size is not None or mask is not None or border_mask is not None:
            return self.detect_segments_batch([bytes(data)], None if new_size is None else [new_size], None if min_length is None else [min_length], max_segments, [camera],
                                              lenses=[lens], out_sizes=[out_size], masks=[mask], border_masks=[border_mask])[0]
        if lens is not None:
            return self.detect_segments_batch([bytes(data)], None if new_size is None else [new_size], None if min_length is None else [min_length], max_segments, [camera], lenses=[lens])[0]
        w, h, _ = jpeg_info(data)
        ptr, n = _bytes_arguments(data)
        nw, nh = (w, h) if new_size is None else (int(new_size[0]), int(new_size[1]))
        if min_length is None:
            min_length = float(np.float32(0.005) * np.sqrt(np.float32(h * h + w * w)))
        cam = None
        if camera is not None:
            if len(camera) != 6:
                raise ValueError("camera must be (fx, fy, cx, cy, k1, k2)")
            cam = (C.c_double * 6)(*[float(v) for v in camera])
        out, cnt = C.POINTER(C.c_float)(), C.c_int(0)
        self._chk(self.lib.l3d_detect_segments_jpeg(self.h, ptr, n, C.c_int(nw), C.c_int(nh), C.c_float(min_length), C.c_int(int(max_segments)), cam,
                                                    C.byref(out), C.byref(cnt)))
        segs = np.ctypeslib.as_array(out, (cnt.value, 4)).copy() if cnt.value else np.zeros((0, 4), np.float32)
        self.lib.l3d_free(out)
        return segs

    # -- images in batches: one pass of the detector over many images ---------------------------------
    def detect_segments_batch(self, images, new_sizes=None, min_lengths=None, max_segments=3000, cameras=None, return_status=False, lenses=None,
                              out_sizes=None, masks=None, border_masks=None):
        """l3d_detect_segments_batch: a list of images -- uint8 arrays (as detect_segments takes them) or `bytes` of baseline JPEG files (as
        detect_segments_jpeg takes them) -> a list of (n, 4) float32 arrays, each byte for byte what the single call gives for that image.
        new_sizes, min_lengths, max_segments, cameras: None, one value for all (max_segments), or a list with one entry (possibly None) per image,
        with the single calls' meanings and defaults.  An entry the single call would refuse raises L3DError (its .code the first such entry's
        status, .statuses all of them); return_status=True: no raise, the result is (segments, statuses).
        A list of device objects (as detect_segments takes them) goes through l3d_detect_segments_device_batch; a list that mixes them with
        host images or files raises ValueError before any call.
        lenses: None, or a list with one capi.lens(...) or None per image (l3d_detect_segments[_device]_batch_lens); an image with a lens is
        undistorted onto its entry of cameras, (fx, fy, cx, cy) -- None: the lens's own source camera.
        out_sizes, masks, border_masks (lists with one entry or None per image; l3d_detect_segments[_device]_batch_remap, "A REMAP"): the image is
        resampled onto out_size = (width, height) -- which new_size and min_length then default from --, mask (capi.remap's) is the caller's
        validity plane in the source grid, and border_mask (default true where one of the three is given) makes the blank pixels of the
        resampling invalid: no line-support region starts where an invalid pixel contributed to the gradient."""
        images = list(images)
        on_device = all_device_objects(images, "detect_segments_batch")
        entries, keep = (detect_device_entries if on_device else detect_entries)(images, new_sizes, min_lengths, max_segments, cameras, lenses, out_sizes)
        n = len(images)
        out, offsets, status = C.POINTER(C.c_float)(), (C.c_int * (n + 1))(), (C.c_int * max(1, n))()
        remap_arr, remap_keep = remap_pointers(lenses, out_sizes, masks, border_masks, n)
        # a mask is in the grid of the image as it arrives: an early ValueError where the size is at hand (the library refuses a mask whose stated
        # extent, l3d_remap.mask_width x mask_height, is not the source's on every path -- a file's size it reads from the headers)
        for i, r in enumerate(remap_keep):
            src = (entries[i].image.height, entries[i].image.width) if on_device else (entries[i].height, entries[i].width)
            if remap_arr is not None and getattr(r, "_mask_shape", None) is not None and src[0] > 0 and tuple(r._mask_shape) != src:
                raise ValueError("mask: shape %s, the source image is %d x %d (H x W)" % (tuple(r._mask_shape), src[0], src[1]))
        lens_arr, lens_keep = lens_pointers(lenses, n)
        if remap_arr is not None:
            call = self.lib.l3d_detect_segments_device_batch_remap if on_device else self.lib.l3d_detect_segments_batch_remap
            rc = call(self.h, entries, remap_arr, C.c_int(n), C.byref(out), offsets, status)
        elif lens_arr is not None:
            call = self.lib.l3d_detect_segments_device_batch_lens if on_device else self.lib.l3d_detect_segments_batch_lens
            rc = call(self.h, entries, lens_arr, C.c_int(n), C.byref(out), offsets, status)
        else:
            call = self.lib.l3d_detect_segments_device_batch if on_device else self.lib.l3d_detect_segments_batch
            rc = call(self.h, entries, C.c_int(n), C.byref(out), offsets, status)
        statuses = [int(status[i]) for i in range(n)]
        segs = []
        if rc == 0:
            total = int(offsets[n])
            flat = np.ctypeslib.as_array(out, (total, 4)).copy() if total else np.zeros((0, 4), np.float32)
            segs = [flat[offsets[i]:offsets[i + 1]].copy() for i in range(n)]
        self.lib.l3d_free(out)
        self._chk(rc)
        if return_status:
            return segs, statuses
        bad = [st for st in statuses if st != 0]
        if bad:
            e = L3DError("line3d_amd error %d: %s" % (bad[0], self.lib.l3d_last_error(self.h).decode()))
            e.code, e.statuses = bad[0], statuses
            raise e
        return segs

    # -- images in device memory (l3d_device_image.hip), the pieces on their own (tests)
    def test_device_image_pointer(self, d):
        """l3d_test_device_image_pointer: what the library establishes about a descriptor's memory before a launch -> (status, message); launches nothing"""
        rc = int(self.lib.l3d_test_device_image_pointer(self.h, C.byref(d)))
        return rc, (self.lib.l3d_last_error(self.h).decode() if rc else "")

    def test_device_ingest(self, descriptors):
        """l3d_test_device_ingest: check, stream wait and ONE k_det_ingest launch for a chunk of same-size descriptors -> uint8 (n, H, W, 1 or 3)"""
        n = len(descriptors)
        arr = (DeviceImage * n)(*descriptors)
        ch = 1 if descriptors[0].channels == 1 else 3
        out = np.zeros((n, descriptors[0].height, descriptors[0].width, ch), np.uint8)
        self._chk(self.lib.l3d_test_device_ingest(self.h, arr, C.c_int(n), _p(out)))
        return out

    def decode_jpeg_into(self, data, out):
        """l3d_decode_jpeg_device into the memory the descriptor (or device object) `out` describes"""
        ptr, n = _bytes_arguments(data)
        o = device_image(out)
        self._chk(self.lib.l3d_decode_jpeg_device(self.h, ptr, n, C.byref(o)))

    # -- the detector's stages on their own (tests): the same kernels and launch shapes as detect_segments
    def test_detect_defined_plane(self):
        """l3d_test_detect_defined_plane: the defined / undefined plane (M, N) uint8, 255 = defined, that the last detector call left for the first
        image of its last chunk; None when that chunk carried no validity plane"""
        n, m = C.c_int(0), C.c_int(0)
        self._chk(self.lib.l3d_test_detect_defined_plane(self.h, None, C.c_size_t(0), C.byref(n), C.byref(m)))
        if n.value == 0 or m.value == 0:
            return None
        out = np.zeros((m.value, n.value), np.uint8)
        self._chk(self.lib.l3d_test_detect_defined_plane(self.h, _p(out), C.c_size_t(out.size), C.byref(n), C.byref(m)))
        return out

    def test_detect_pixel_stage(self, img, new_size=None):
        """l3d_test_detect_pixel_stage -> dict: grey (nh, nw) float32; img, mod, ang (M, N) float64; bucket (M, N, 2) uint8"""
        pix, w, h, ch, stride = image_arguments(img)
        nw, nh = (w, h) if new_size is None else (int(new_size[0]), int(new_size[1]))
        N, M = int(np.ceil(nw * 0.8)), int(np.ceil(nh * 0.8))
        out = {"grey": np.zeros((nh, nw), np.float32), "img": np.zeros((M, N)), "mod": np.zeros((M, N)), "ang": np.zeros((M, N)),
               "bucket": np.zeros((M, N, 2), np.uint8)}
        n, m = C.c_int(0), C.c_int(0)
        self._chk(self.lib.l3d_test_detect_pixel_stage(self.h, pix, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), C.c_int(nw), C.c_int(nh),
                                                       _p(out["grey"]), _p(out["img"]), _p(out["mod"]), _p(out["ang"]), _p(out["bucket"]),
                                                       C.byref(n), C.byref(m)))
        if (n.value, m.value) != (N, M):
            raise L3DError("scaled size (%d, %d), expected (%d, %d)" % (n.value, m.value, N, M))
        return out

    def test_detect_label(self, bucket, active):
        """l3d_test_detect_label: bucket (M, N, 2) uint8, active (M, N) -> parent (2, M, N) int32, key (M, N) uint32"""
        bucket = np.ascontiguousarray(bucket, dtype=np.uint8)
        active = np.ascontiguousarray(active, dtype=np.uint8)
        M, N = active.shape
        assert bucket.shape == (M, N, 2)
        parent, key = np.zeros((2, M, N), np.int32), np.zeros((M, N), np.uint32)
        self._chk(self.lib.l3d_test_detect_label(self.h, _p(bucket), _p(active), C.c_int(N), C.c_int(M), _p(parent), _p(key)))
        return parent, key

    def test_detect_regions(self, mod, ang, key, min_reg):
        """l3d_test_detect_regions: mod, ang (M, N) float64, key (M, N) uint32 -> (records REGION_DTYPE, active_out (M, N) uint8)"""
        mod, ang = np.ascontiguousarray(mod, dtype=np.float64), np.ascontiguousarray(ang, dtype=np.float64)
        key = np.ascontiguousarray(key, dtype=np.uint32)
        M, N = key.shape
        assert mod.shape == (M, N) and ang.shape == (M, N)
        rec, n = C.c_void_p(), C.c_int(0)
        active = np.zeros((M, N), np.uint8)
        self._chk(self.lib.l3d_test_detect_regions(self.h, C.c_int(N), C.c_int(M), _p(mod), _p(ang), _p(key), C.c_int(int(min_reg)),
                                                   C.byref(rec), C.byref(n), _p(active)))
        out = np.zeros(n.value, dtype=REGION_DTYPE)
        if n.value:
            C.memmove(out.ctypes.data, rec, n.value * REGION_DTYPE.itemsize)
        self.lib.l3d_free(rec)
        return out, active

    def test_detect_nfa(self, n, k, p, logNT):
        """l3d_test_detect_nfa: -log10 NFA per (n, k, p)"""
        n, k = np.ascontiguousarray(n, dtype=np.int32), np.ascontiguousarray(k, dtype=np.int32)
        p = np.ascontiguousarray(p, dtype=np.float64)
        out = np.zeros(len(n))
        self._chk(self.lib.l3d_test_detect_nfa(self.h, _p(n), _p(k), _p(p), C.c_double(float(logNT)), C.c_int(len(n)), _p(out)))
        return out

    def test_verify_candidates(self, src_segs, tgt_segs, offsets, P, RtKinv_src, C_src, row_start, cand_meta, cand_depths, sigma_p, sigma_a, spatial_k,
                               path=0, gb=0, split_unit=0, mmax=0, wide_max=0, seg_order=None, exist_cams=None):
        """l3d_test_verify_candidates: stage 2 on a packed candidate list -> (conf (R,), kept_cnt (S,), best_depths (S, 2), mmax_used, kernels).
        exist_cams (path 2): the local cameras whose rows are handed in unordered; the result then ends with cand_meta (R, 2) and cand_depths (R, 4)
        as the kernels left them.  Nothing is checked here: a broken table is the library's to refuse."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        src_segs, tgt_segs, P, RtKinv_src, C_src, cand_depths = f(src_segs), f(tgt_segs), f(P), f(RtKinv_src), f(C_src), f(cand_depths)
        offsets, row_start = np.ascontiguousarray(offsets, dtype=np.int32), np.ascontiguousarray(row_start, dtype=np.int32)
        cand_meta = np.ascontiguousarray(cand_meta, dtype=np.uint32)
        S, N, R, n_tgt = len(src_segs), len(offsets), len(cand_meta), len(tgt_segs.reshape(-1, 4))
        assert row_start.shape == (S * N + 1,) and cand_meta.shape == (R, 2) and cand_depths.shape == (R, 4) and P.size == N * 12
        sel = VerifyPath(int(path), int(gb), int(split_unit), int(mmax), int(wide_max), 0, 0, 0, None)
        if seg_order is not None:
            seg_order = np.ascontiguousarray(seg_order, dtype=np.int32)
            assert seg_order.shape == (S,)
            sel.seg_order = seg_order.ctypes.data
        conf, kept, best = np.zeros(R, np.float32), np.zeros(S, np.int32), np.zeros((S, 2), np.float32)
        if exist_cams is not None:
            exist_cams = np.ascontiguousarray(exist_cams, dtype=np.int32)
            meta_out, depths_out = np.zeros((R, 2), np.uint32), np.zeros((R, 4), np.float32)
            sel.exist_cams, sel.n_exist_cams = exist_cams.ctypes.data, len(exist_cams)
            sel.cand_meta_out, sel.cand_depths_out = meta_out.ctypes.data, depths_out.ctypes.data
        self._chk(self.lib.l3d_test_verify_candidates(self.h, C.c_int(S), C.c_int(N), _p(src_segs), _p(tgt_segs), C.c_int(n_tgt), _p(offsets), _p(P),
                                                      _p(RtKinv_src), _p(C_src), _p(row_start), _p(cand_meta), _p(cand_depths), C.c_int(R),
                                                      C.c_float(float(sigma_p)), C.c_float(float(sigma_a)), C.c_float(float(spatial_k)), C.byref(sel),
                                                      _p(conf), _p(kept), _p(best)))
        if exist_cams is not None:
            return conf, kept, best, int(sel.mmax_used), int(sel.kernels), meta_out, depths_out
        return conf, kept, best, int(sel.mmax_used), int(sel.kernels)

    def test_pair_candidates(self, src_segs, tgt_segs, offsets, F, RtKinv, centers, RtKinv_src, C_src, to_be_matched, path=0, pretest=3, spb=0,
                             seg_range=None, ray_tables=None, cand_cap=0, capacity=0):
        """l3d_test_pair_candidates: stage 1 of one source view on one launch sequence -> dict(row_upper (S*N,), row_count (S*N,), row_start (S*N + 1,),
        cand_meta (capacity, 2), cand_depths (capacity, 4), total, largest, spb_used, overflow, needed).  ray_tables None: 1 on paths 1 and 2.
        Nothing is checked here: a broken table is the library's to refuse (the L3DError then carries the slots needed in .needed)."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        src_segs, tgt_segs, F, RtKinv, centers, RtKinv_src, C_src = f(src_segs), f(tgt_segs), f(F), f(RtKinv), f(centers), f(RtKinv_src), f(C_src)
        offsets, tbm = np.ascontiguousarray(offsets, dtype=np.int32), np.ascontiguousarray(to_be_matched, dtype=np.int32)
        S, N, n_tgt = len(src_segs.reshape(-1, 4)), len(offsets), len(tgt_segs.reshape(-1, 4))
        assert F.size == N * 9 and RtKinv.size == N * 9 and centers.size == N * 3 and RtKinv_src.size == 9 and C_src.size == 3
        s0, s1 = (0, S) if seg_range is None else seg_range
        if ray_tables is None:
            ray_tables = 1 if path in (1, 2) else 0
        sel = PairPath(int(path), int(pretest), int(spb), int(s0), int(s1), int(ray_tables), int(cand_cap), int(capacity))
        out = dict(row_upper=np.zeros(S * N, np.int32), row_count=np.zeros(S * N, np.int32), row_start=np.zeros(S * N + 1, np.int32),
                   cand_meta=np.zeros((int(capacity), 2), np.uint32), cand_depths=np.zeros((int(capacity), 4), np.float32))
        try:
            self._chk(self.lib.l3d_test_pair_candidates(self.h, C.c_int(S), C.c_int(N), _p(src_segs), _p(tgt_segs), C.c_int(n_tgt), _p(offsets), _p(F), _p(RtKinv),
                                                        _p(centers), _p(RtKinv_src), _p(C_src), _p(tbm), C.c_int(len(tbm)), C.byref(sel), _p(out["row_upper"]),
                                                        _p(out["row_count"]), _p(out["row_start"]), _p(out["cand_meta"]), _p(out["cand_depths"])))
        except L3DError as e:
            e.needed = int(sel.needed)
            raise
        out.update(total=int(sel.total), largest=int(sel.largest), spb_used=int(sel.spb_used), overflow=int(sel.overflow), needed=int(sel.needed))
        return out

    def test_collect_candidates(self, views, k, rowA, metaA, depthsA, rowcnt, route=0, rt_g=-1, sort_apart=0, cand_cap=0, avg_kept=0.0, overflowed=None):
        """l3d_test_collect_candidates: the collect step of the resident chain for view k of a schedule.  views: one dict per chain view, in chain
        order -- id, S, l2g, n_tbm, tbm (cameras to be matched), source_cam, source_index, kept (MATCH_DTYPE, global camera ids; read for the views
        in front of k).  -> dict(row_start, cand_meta (cand_cap, 2), cand_depths (cand_cap, 4), cursor, seg_order, kernels, g, bps, blocks_move, R).
        Nothing is checked here: a broken table is the library's to refuse."""
        n = len(views)
        arr, keep = (ChainView * max(1, n))(), []
        for j, v in enumerate(views):
            l2g, tbm = np.ascontiguousarray(v["l2g"], dtype=np.uint32), np.ascontiguousarray(v["tbm"], dtype=np.int32)
            sc, si = np.ascontiguousarray(v["source_cam"], dtype=np.int32), np.ascontiguousarray(v["source_index"], dtype=np.int32)
            keep += [l2g, tbm, sc, si]
            e = arr[j]
            e.view_id, e.S_src, e.N, e.n_tbm, e.n_sources = int(v["id"]), int(v["S"]), len(l2g), int(v["n_tbm"]), len(sc)
            e.local2global, e.to_be_matched, e.source_cam, e.source_index = l2g.ctypes.data, tbm.ctypes.data, sc.ctypes.data, si.ctypes.data
        lists = [np.ascontiguousarray(v["kept"], dtype=MATCH_DTYPE) for v in views[:k]]
        n_kept = np.array([len(a) for a in lists] + [0] * (n - k), np.int32)
        kept_all = np.concatenate(lists) if lists else np.zeros(0, MATCH_DTYPE)
        S, N = int(views[k]["S"]), len(views[k]["l2g"])
        rowA, rowcnt = np.ascontiguousarray(rowA, dtype=np.int32), np.ascontiguousarray(rowcnt, dtype=np.int32)
        metaA, depthsA = np.ascontiguousarray(metaA, dtype=np.uint32).reshape(-1, 2), np.ascontiguousarray(depthsA, dtype=np.float32).reshape(-1, 4)
        assert rowA.shape == rowcnt.shape == (S * N,) and len(metaA) == len(depthsA)
        sel = CollectPath()
        sel.route, sel.rt_g, sel.sort_apart, sel.cand_cap, sel.avg_kept = int(route), int(rt_g), int(sort_apart), int(cand_cap), float(avg_kept)
        ov = None if overflowed is None else np.ascontiguousarray(overflowed, dtype=np.uint8)
        assert ov is None or len(ov) == n
        sel.overflowed = None if ov is None else ov.ctypes.data
        out = dict(row_start=np.zeros(S * N + 1, np.int32), cand_meta=np.zeros((int(cand_cap), 2), np.uint32), cand_depths=np.zeros((int(cand_cap), 4), np.float32),
                   cursor=np.zeros(S * N, np.int32), seg_order=np.zeros(S, np.int32))
        nz = lambda a: _p(a) if a.size else None
        self._chk(self.lib.l3d_test_collect_candidates(self.h, arr, C.c_int(n), C.c_int(int(k)), nz(kept_all), _p(n_kept), nz(rowA), nz(metaA), nz(depthsA),
                                                       C.c_int(len(metaA)), nz(rowcnt), C.byref(sel), _p(out["row_start"]), nz(out["cand_meta"]),
                                                       nz(out["cand_depths"]), nz(out["cursor"]), nz(out["seg_order"])))
        out.update(kernels=int(sel.kernels), g=int(sel.g), bps=int(sel.bps), blocks_move=int(sel.blocks_move), R=int(sel.R))
        return out

    def test_kept_write(self, N, row_start, cand_meta, cand_depths, cand_conf, kept_cnt, l2g, writer=0, prev=None, cand_cap=None, arena_cap=0, jobs=()):
        """l3d_test_kept_write: the kept writer on one view's verified candidates, then (jobs) the rebuild of side words and run tables.
        prev: None or (kept_base, n_kept) of the view before; cand_cap None: exactly R.  jobs: None = the list the writer just left, or a dict
        records (MATCH_DTYPE, global camera ids), S, l2g.  -> dict(records (arena_cap,) MATCH_DTYPE, side (arena_cap,) uint32, rt (N + 1, S),
        best_pos (S,), kept_base, n_kept, R, overflow, n_want, rebuild_err, rebuild_blocks, jobs = [dict(n, qt, rt)]); what no kernel wrote is
        0xff bytes.  Nothing is checked here: a broken table is the library's to refuse."""
        row_start = np.ascontiguousarray(row_start, dtype=np.int32)
        cand_meta = np.ascontiguousarray(cand_meta, dtype=np.uint32).reshape(-1, 2)
        cand_depths = np.ascontiguousarray(cand_depths, dtype=np.float32).reshape(-1, 4)
        cand_conf = np.ascontiguousarray(cand_conf, dtype=np.float32)
        kept_cnt, l2g = np.ascontiguousarray(kept_cnt, dtype=np.int32), np.ascontiguousarray(l2g, dtype=np.uint32)
        S, R = len(kept_cnt), len(cand_conf)
        assert row_start.shape == (S * N + 1,) and len(cand_meta) == R and len(cand_depths) == R and l2g.shape == (N,)
        sel = KeptPath()
        sel.writer, sel.has_prev = int(writer), 0 if prev is None else 1
        if prev is not None:
            sel.prev_base, sel.prev_n_kept = int(prev[0]), int(prev[1])
        sel.cand_cap, sel.arena_cap = R if cand_cap is None else int(cand_cap), int(arena_cap)
        cj = (KeptJob * max(1, len(jobs)))()
        keep, outs = [], []
        for i, j in enumerate(jobs):
            if j is None:
                n, jS, jN = int(kept_cnt.sum()), S, N
            else:
                recs = np.ascontiguousarray(j["records"], dtype=MATCH_DTYPE)
                jl = np.ascontiguousarray(j["l2g"], dtype=np.uint32)
                n, jS, jN = len(recs), int(j["S"]), len(jl)
                keep += [recs, jl]
                cj[i].records, cj[i].local2global = recs.ctypes.data, jl.ctypes.data
            qt, rt = np.full(max(1, n), 0xffffffff, np.uint32), np.full((jN + 1, jS), -1, np.int32)
            cj[i].qt, cj[i].rt, cj[i].n, cj[i].S, cj[i].N = qt.ctypes.data, rt.ctypes.data if rt.size else None, n, jS, jN
            outs.append((qt, rt))
        sel.jobs, sel.n_jobs = C.addressof(cj), len(jobs)
        records = np.zeros(int(arena_cap), dtype=MATCH_DTYPE)
        side = np.zeros(int(arena_cap), np.uint32)
        rt, best_pos = np.zeros((N + 1, S), np.int32), np.zeros(S, np.int32)
        nz = lambda a: _p(a) if a.size else None
        self._chk(self.lib.l3d_test_kept_write(self.h, C.c_int(S), C.c_int(N), _p(row_start), nz(cand_meta), nz(cand_depths), nz(cand_conf), nz(kept_cnt), _p(l2g),
                                               C.byref(sel), nz(records), nz(side), nz(rt), nz(best_pos)))
        return dict(records=records, side=side, rt=rt, best_pos=best_pos, kept_base=int(sel.kept_base), n_kept=int(sel.n_kept), R=int(sel.R),
                    overflow=int(sel.overflow), n_want=int(sel.n_want), rebuild_err=int(sel.rebuild_err), rebuild_blocks=int(sel.rebuild_blocks),
                    jobs=[dict(n=int(cj[i].n), qt=outs[i][0][:int(cj[i].n)], rt=outs[i][1]) for i in range(len(jobs))])

    def test_shard_slot_write(self, N, row_start, cand_meta, cand_depths, cand_conf, kept_cnt, l2g, best, s0, s1, geom, cand_cap=None):
        """l3d_test_shard_slot_write: k_slot_write for one view's verified candidates and the range [s0, s1) -> the slot's bytes (uint8, slot_bytes of
        the geometry; 0xff where the kernel did not write, 0x7f in the best positions).  geom: the dict shard_geom takes; cand_cap None: exactly R.
        Nothing is checked here: a broken table is the library's to refuse."""
        row_start = np.ascontiguousarray(row_start, dtype=np.int32)
        cand_meta = np.ascontiguousarray(cand_meta, dtype=np.uint32).reshape(-1, 2)
        cand_depths = np.ascontiguousarray(cand_depths, dtype=np.float32).reshape(-1, 4)
        cand_conf = np.ascontiguousarray(cand_conf, dtype=np.float32)
        kept_cnt, l2g = np.ascontiguousarray(kept_cnt, dtype=np.int32), np.ascontiguousarray(l2g, dtype=np.uint32)
        best = np.ascontiguousarray(best, dtype=np.float32).reshape(-1, 2)
        S, R = len(kept_cnt), len(cand_conf)
        assert row_start.shape == (S * N + 1,) and len(cand_meta) == R and len(cand_depths) == R and l2g.shape == (N,) and len(best) == S
        g = shard_geom(geom)
        try:
            n_bytes = shard_slot_geometry(g.maxS, g.maxN, g.world, g.slot_records, g.slot_cams_min, g.n_views)["slot_bytes"]
        except L3DError:
            n_bytes = 0                 # (a geometry the library refuses: the call below says so)
        slot = np.zeros(max(1, n_bytes), np.uint8)
        nz = lambda a: _p(a) if a.size else None
        self._chk(self.lib.l3d_test_shard_slot_write(self.h, C.c_int(S), C.c_int(N), _p(row_start), nz(cand_meta), nz(cand_depths), nz(cand_conf), nz(kept_cnt), _p(l2g),
                                                     nz(best), C.c_int(int(s0)), C.c_int(int(s1)), C.byref(g), C.c_int(R if cand_cap is None else int(cand_cap)), _p(slot)))
        return slot[:n_bytes]

    def test_shard_collect(self, views, k, gathered, geom, s0, s1, rowA, metaA, depthsA, rowcnt, cand_cap, sort_apart=0, slot_scan_grain=0):
        """l3d_test_shard_collect: the collect step of the sharded chain for view k and the range [s0, s1) over the gathered bytes (uint8, ring x world
        x slot_bytes).  views: as test_collect_candidates takes them (kept is not read).  -> dict(row_start, cand_meta (cand_cap, 2), cand_depths
        (cand_cap, 4), cursor, seg_order, wps, blocks_move, R); 0xff bytes where no kernel wrote.  Nothing is checked here."""
        n = len(views)
        arr, keep = (ChainView * max(1, n))(), []
        for j, v in enumerate(views):
            l2g, tbm = np.ascontiguousarray(v["l2g"], dtype=np.uint32), np.ascontiguousarray(v["tbm"], dtype=np.int32)
            sc, si = np.ascontiguousarray(v["source_cam"], dtype=np.int32), np.ascontiguousarray(v["source_index"], dtype=np.int32)
            keep += [l2g, tbm, sc, si]
            e = arr[j]
            e.view_id, e.S_src, e.N, e.n_tbm, e.n_sources = int(v["id"]), int(v["S"]), len(l2g), int(v["n_tbm"]), len(sc)
            e.local2global, e.to_be_matched, e.source_cam, e.source_index = l2g.ctypes.data, tbm.ctypes.data, sc.ctypes.data, si.ctypes.data
        S, N = int(views[k]["S"]), len(views[k]["l2g"])
        gathered = np.ascontiguousarray(gathered, dtype=np.uint8)
        rowA, rowcnt = np.ascontiguousarray(rowA, dtype=np.int32), np.ascontiguousarray(rowcnt, dtype=np.int32)
        metaA, depthsA = np.ascontiguousarray(metaA, dtype=np.uint32).reshape(-1, 2), np.ascontiguousarray(depthsA, dtype=np.float32).reshape(-1, 4)
        assert rowA.shape == rowcnt.shape == (S * N,) and len(metaA) == len(depthsA)
        g = shard_geom(geom)
        sel = ShardCollectPath(int(s0), int(s1), int(cand_cap), int(sort_apart), int(slot_scan_grain), 0, 0, 0)
        out = dict(row_start=np.zeros(S * N + 1, np.int32), cand_meta=np.zeros((int(cand_cap), 2), np.uint32), cand_depths=np.zeros((int(cand_cap), 4), np.float32),
                   cursor=np.zeros(S * N, np.int32), seg_order=np.zeros(S, np.int32))
        nz = lambda a: _p(a) if a.size else None
        self._chk(self.lib.l3d_test_shard_collect(self.h, arr, C.c_int(n), C.c_int(int(k)), nz(gathered), C.byref(g), nz(rowA), nz(metaA), nz(depthsA), C.c_int(len(metaA)),
                                                  nz(rowcnt), C.byref(sel), _p(out["row_start"]), nz(out["cand_meta"]), nz(out["cand_depths"]), nz(out["cursor"]),
                                                  nz(out["seg_order"])))
        out.update(wps=int(sel.wps), blocks_move=int(sel.blocks_move), R=int(sel.R))
        return out

    def test_shard_pack(self, gathered, geom, verified, best_off, view_sn, batches, arena_cap, pack_cap, best_cap, keep=None, rt_off=None, rt_cap=0,
                        retire_tables=0):
        """l3d_test_shard_pack: the consumers of the gathered blocks over all views' slots (uint8, n_views x world x slot_bytes).  batches: (first, count,
        enqueued at view) triples.  -> dict(stage (n_views, stage_bytes) uint8, pack_hdr (n_views, 32) uint8, totals (2, n_views, 2), check (2, 3),
        pa_arena / rt_arena (MATCH_DTYPE), pa_best / rt_best (best_cap, 2), pa_bestpos / rt_bestpos, base_dev (n_views + 2) int64, hdr_all (n_views,
        world, 8) int32, overflow, qt_arena (arena_cap) uint32, rt_all (rt_cap) int32).  Nothing is checked here."""
        g = shard_geom(geom)
        nv, W = g.n_views, g.world
        try:
            stage_bytes = shard_slot_geometry(g.maxS, g.maxN, g.world, g.slot_records, g.slot_cams_min, g.n_views)["stage_bytes"]
        except L3DError:
            stage_bytes = 0
        gathered = np.ascontiguousarray(gathered, dtype=np.uint8)
        ver, bo = np.ascontiguousarray(verified, dtype=np.uint8), np.ascontiguousarray(best_off, dtype=np.int64)
        sn = np.ascontiguousarray(view_sn, dtype=np.int32).reshape(-1, 2)
        bt = np.ascontiguousarray(batches, dtype=np.int32).reshape(-1, 3)
        kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
        ro = None if rt_off is None else np.ascontiguousarray(rt_off, dtype=np.int64)
        assert len(ver) == len(bo) == len(sn) == nv and (kp is None or len(kp) == nv) and (ro is None or len(ro) == nv)
        one = lambda n: max(1, int(n))
        out = dict(stage=np.zeros((nv, one(stage_bytes)), np.uint8), pack_hdr=np.zeros((nv, 32), np.uint8), totals=np.zeros((2, nv, 2), np.int32),
                   check=np.zeros((2, 3), np.int32), pa_arena=np.zeros(one(pack_cap), MATCH_DTYPE), pa_best=np.zeros((one(best_cap), 2), np.float32),
                   pa_bestpos=np.zeros(one(best_cap), np.int32), rt_arena=np.zeros(one(arena_cap), MATCH_DTYPE), rt_best=np.zeros((one(best_cap), 2), np.float32),
                   rt_bestpos=np.zeros(one(best_cap), np.int32), base_dev=np.zeros(nv + 2, np.int64), hdr_all=np.zeros((nv, W, 8), np.int32),
                   overflow=np.zeros(1, np.int32), qt_arena=np.zeros(one(arena_cap), np.uint32), rt_all=np.zeros(one(rt_cap), np.int32))
        io = ShardPackIO()
        io.verified, io.keep, io.best_off, io.view_sn = ver.ctypes.data, None if kp is None else kp.ctypes.data, bo.ctypes.data, sn.ctypes.data
        io.rt_off, io.batches, io.n_batches, io.retire_tables = None if ro is None else ro.ctypes.data, bt.ctypes.data if len(bt) else None, len(bt), int(retire_tables)
        io.arena_cap, io.pack_cap, io.best_cap, io.rt_cap = int(arena_cap), int(pack_cap), int(best_cap), int(rt_cap)
        for name in ("stage", "pack_hdr", "totals", "check", "pa_arena", "pa_best", "pa_bestpos", "rt_arena", "rt_best", "rt_bestpos", "base_dev", "hdr_all", "overflow",
                     "qt_arena", "rt_all"):
            setattr(io, name, out[name].ctypes.data)
        self._chk(self.lib.l3d_test_shard_pack(self.h, _p(gathered) if gathered.size else None, C.byref(g), C.byref(io)))
        for name, n in (("pa_arena", pack_cap), ("rt_arena", arena_cap), ("qt_arena", arena_cap), ("pa_best", best_cap), ("rt_best", best_cap), ("pa_bestpos", best_cap),
                        ("rt_bestpos", best_cap), ("rt_all", rt_cap)):
            out[name] = out[name][:int(n)]
        out["stage"] = out["stage"][:, :stage_bytes]
        out["overflow"] = int(out["overflow"][0])
        return out

    def chain_products_get(self, n_dense: int, n_pot: int, slack: int = 0):
        """l3d_chain_products_get: (pot_start int64 (n_dense + 1,), pot_tgt int32 (n_pot + slack,), best MATCH_DTYPE (n_dense,)).  The slots of
        pot_tgt behind n_pot are filled with -1 (0xffffffff) before the call: the library must leave them alone."""
        pot_start = np.zeros(n_dense + 1, np.int64)
        pot_tgt = np.full(n_pot + slack, -1, np.int32)
        best = np.zeros(n_dense, dtype=MATCH_DTYPE)
        self._chk(self.lib.l3d_chain_products_get(self.h, _p(pot_start), _p(pot_tgt), _p(best)))
        return pot_start, pot_tgt, best

    def test_products(self, views, view_ids, seg_base, side_arrays=0, early_pairs=0, rows=None, held=None, slack=64, max_blocks=1024):
        """l3d_test_products: the products of matchViews from kept lists handed in.  views: one dict per chain view, in chain order -- id, S, l2g
        (global ids of its N neighbours), n_tbm (0: early return), source_cam, source_index, kept (MATCH_DTYPE, GLOBAL camera ids), R, best (S, 2)
        float32, bestpos (S,) int32.  view_ids / seg_base: the dense map.  rows: None or (dv0, dv1); held: None or one flag per chain view.
        -> dict(pot_start, pot_tgt (n_pot + slack entries, -1 behind n_pot), best, n_pot, summary (SUMMARY_DTYPE), report)."""
        n = len(views)
        arr, keep = (ChainView * max(1, n))(), []
        for k, v in enumerate(views):
            l2g = np.ascontiguousarray(v["l2g"], dtype=np.uint32)
            sc, si = np.ascontiguousarray(v["source_cam"], dtype=np.int32), np.ascontiguousarray(v["source_index"], dtype=np.int32)
            assert len(sc) == len(si)
            keep += [l2g, sc, si]
            e = arr[k]
            e.view_id, e.S_src, e.N, e.n_tbm, e.n_sources = int(v["id"]), int(v["S"]), len(l2g), int(v["n_tbm"]), len(sc)
            e.local2global, e.source_cam, e.source_index = l2g.ctypes.data, sc.ctypes.data, si.ctypes.data
        kept = [np.ascontiguousarray(v["kept"], dtype=MATCH_DTYPE) for v in views]
        n_kept = np.array([len(a) for a in kept], np.int32)
        kept_all = np.concatenate(kept) if n else np.zeros(0, MATCH_DTYPE)
        R = np.array([int(v["R"]) for v in views], np.int64)
        best = np.ascontiguousarray(np.concatenate([np.asarray(v["best"], np.float32).reshape(-1, 2) for v in views]), dtype=np.float32)
        bestpos = np.ascontiguousarray(np.concatenate([np.asarray(v["bestpos"], np.int32).reshape(-1) for v in views]), dtype=np.int32)
        assert len(best) == len(bestpos) == sum(int(v["S"]) for v in views)
        ids, sb = np.ascontiguousarray(view_ids, dtype=np.uint32), np.ascontiguousarray(seg_base, dtype=np.int32)
        assert len(sb) == len(ids) + 1
        dm = DenseMap(len(ids), ids.ctypes.data, sb.ctypes.data)
        blk = [np.full(max_blocks, -9, np.int32) for _ in range(3)]
        sel = ProductsPath()
        sel.side_arrays, sel.early_pairs = int(side_arrays), int(early_pairs)
        sel.dv0, sel.dv1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
        hb = None if held is None else np.ascontiguousarray(held, dtype=np.uint8)
        assert hb is None or len(hb) == n
        sel.held = None if hb is None else hb.ctypes.data
        sel.block_capacity = max_blocks
        sel.block_cap, sel.block_staged, sel.block_g = (b.ctypes.data for b in blk)
        summary = np.zeros(max(1, n), dtype=SUMMARY_DTYPE)
        n_pot = C.c_int64(0)
        self._chk(self.lib.l3d_test_products(self.h, arr, C.c_int(n), C.byref(dm), _p(kept_all), _p(n_kept), _p(R), _p(best), _p(bestpos), C.byref(sel),
                                             _p(summary), C.byref(n_pot)))
        nd = int(sb[-1])
        pot_start, pot_tgt, bm = self.chain_products_get(nd, n_pot.value, slack)
        nb = min(max_blocks, int(sel.n_blocks)) if sel.build == PROD_TRANSPOSED else 0
        report = dict(side_arrays_used=int(sel.side_arrays_used), build=int(sel.build), refused=int(sel.refused), n_blocks=int(sel.n_blocks),
                      max_touch=int(sel.max_touch), early_cap=int(sel.early_cap), early_g=int(sel.early_g),
                      block_cap=blk[0][:nb].tolist(), block_staged=blk[1][:nb].tolist(), block_g=blk[2][:nb].tolist())
        return dict(pot_start=pot_start, pot_tgt=pot_tgt, best=bm, n_pot=int(n_pot.value), summary=summary[:n], report=report)

    # -- the three seam functions ---------------------------------------------------------------
    def compute_collinearity(self, segs, collin_s=2.0):
        segs = np.ascontiguousarray(segs, dtype=np.float32)
        oi, oj, ow = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
        n = C.c_int(0)
        self._chk(self.lib.l3d_compute_collinearity(self.h, _p(segs), C.c_int(len(segs)), C.c_float(collin_s),
                                                    C.byref(oi), C.byref(oj), C.byref(ow), C.byref(n)))
        k = n.value
        i = np.ctypeslib.as_array(oi, (k,)).copy() if k else np.zeros(0, np.int32)
        j = np.ctypeslib.as_array(oj, (k,)).copy() if k else np.zeros(0, np.int32)
        w = np.ctypeslib.as_array(ow, (k,)).copy() if k else np.zeros(0, np.float32)
        for p in (oi, oj, ow):
            self.lib.l3d_free(p)
        return i, j, w

    def compute_collinearity_batch(self, seg_sets, collin_s=2.0):
        """l3d_compute_collinearity_batch: list of (S_v, 4) arrays -> list of (i, j, w) triplet arrays, one per set."""
        sets = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 4) for s in seg_sets]
        n = len(sets)
        ptrs = (C.c_void_p * max(n, 1))(*[s.ctypes.data for s in sets])
        ns = np.array([len(s) for s in sets], np.int32)
        start = np.zeros(n + 1, np.int32)
        oi, oj, ow = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
        self._chk(self.lib.l3d_compute_collinearity_batch(self.h, ptrs, _p(ns), C.c_int(n), C.c_float(collin_s),
                                                          C.byref(oi), C.byref(oj), C.byref(ow), _p(start)))
        total = int(start[n])
        i = np.ctypeslib.as_array(oi, (total,)).copy() if total else np.zeros(0, np.int32)
        j = np.ctypeslib.as_array(oj, (total,)).copy() if total else np.zeros(0, np.int32)
        w = np.ctypeslib.as_array(ow, (total,)).copy() if total else np.zeros(0, np.float32)
        for p in (oi, oj, ow):
            self.lib.l3d_free(p)
        return [(i[start[v]:start[v + 1]], j[start[v]:start[v + 1]], w[start[v]:start[v + 1]]) for v in range(n)]

    def compute_pairwise_matches(self, src_segs, RtKinv_src, C_src, tgt_segs, offsets, F, RtKinv, centers, P,
                                 to_be_matched, in_matches, local2global, k_upper, k_lower, sigma_p, sigma_a,
                                 spatial_k, median_depth=1.0, seg_range=None, want_best=False):
        def f32(a):
            return a if (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous) else np.ascontiguousarray(a, dtype=np.float32)
        src_segs, tgt_segs = f32(src_segs), f32(tgt_segs)
        RtKinv_src, C_src, F, RtKinv, centers, P = f32(RtKinv_src), f32(C_src), f32(F), f32(RtKinv), f32(centers), f32(P)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        tbm = np.ascontiguousarray(to_be_matched, dtype=np.int32)
        inm = np.ascontiguousarray(in_matches, dtype=MATCH_DTYPE)
        l2g = np.ascontiguousarray(local2global, dtype=np.uint32)
        S = len(src_segs)
        s0, s1 = (0, S) if seg_range is None else seg_range
        out = C.c_void_p()
        n_out = C.c_int(0)
        med = C.c_float(median_depth)
        bd = C.POINTER(C.c_float)()
        nb = C.c_int(0)
        self._chk(self.lib.l3d_compute_pairwise_matches(
            self.h, _p(src_segs), C.c_int(S), _p(RtKinv_src), _p(C_src), _p(tgt_segs), _p(offsets), C.c_int(len(offsets)),
            _p(F), _p(RtKinv), _p(centers), _p(P), _p(tbm), C.c_int(len(tbm)), _p(inm), C.c_int(len(inm)), _p(l2g),
            C.c_float(k_upper), C.c_float(k_lower), C.c_float(sigma_p), C.c_float(sigma_a), C.c_float(spatial_k),
            C.c_int(s0), C.c_int(s1), C.byref(out), C.byref(n_out), C.byref(med), C.byref(bd), C.byref(nb)))
        n = n_out.value
        res = np.zeros(n, dtype=MATCH_DTYPE)
        if n:
            C.memmove(res.ctypes.data, out, n * 32)
        self.lib.l3d_free(out)
        best = np.ctypeslib.as_array(bd, (nb.value * 2,)).copy() if nb.value else np.zeros(0, np.float32)
        if bd:
            self.lib.l3d_free(bd)
        if want_best:
            return res, med.value, best
        return res, med.value

    def replicator_dynamics_diffusion(self, edges, n, iters=10):
        edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        out = np.zeros(len(edges), dtype=EDGE_DTYPE)
        self._chk(self.lib.l3d_replicator_dynamics_diffusion(self.h, _p(edges), C.c_int(len(edges)), C.c_int(n),
                                                             C.c_int(iters), _p(out)))
        return out

    def similarity_coll3D_batch(self, hyp, pairs, sigma_a):
        hyp = np.ascontiguousarray(hyp, dtype=HYP_DTYPE)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        sim = np.zeros(len(pairs), dtype=np.float32)
        self._chk(self.lib.l3d_similarity_coll3D_batch(self.h, _p(hyp), C.c_int(len(hyp)), _p(pairs), C.c_int(len(pairs)),
                                                       C.c_float(sigma_a), _p(sim)))
        return sim

    @staticmethod
    def _affinity_input(seg_base, view_hyp_begin, hyp, score, hyp_dense, best, pot_start, pot_tgt, coll_start, coll_other, coll_w, sigma_a):
        """-> (l3d_affinity_input, the arrays it points into)"""
        arrs = [np.ascontiguousarray(seg_base, np.int32), np.ascontiguousarray(view_hyp_begin, np.int32), np.ascontiguousarray(hyp, HYP_DTYPE),
                np.ascontiguousarray(score, np.float32), np.ascontiguousarray(hyp_dense, np.int32), np.ascontiguousarray(best, np.int32),
                np.ascontiguousarray(pot_start, np.int64), np.ascontiguousarray(pot_tgt, np.int32), np.ascontiguousarray(coll_start, np.int64),
                np.ascontiguousarray(coll_other, np.int32), np.ascontiguousarray(coll_w, np.float32)]
        ptr = [a.ctypes.data_as(C.c_void_p) for a in arrs]
        return AffinityInput(len(arrs[0]) - 1, ptr[0], ptr[1], len(arrs[2]), ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], ptr[7], ptr[8], ptr[9], ptr[10], float(sigma_a)), arrs

    def test_affinity_fill(self, tables, h0=0, h1=None, pos_base=0, loc2glob=None, assume_symmetric=False):
        """l3d_test_affinity_fill: the fill's core as one part of a sharded fill.  tables: the arguments of affinity_fill, in order.  -> dict(flags uint8 per
        potential correspondence, needs_prev int32 per view, n_launches, coll_sym, n_candidates, n_passed, pairs int32 (n_passed, 2), w float32, first uint64
        per hypothesis)"""
        inp, arrs = self._affinity_input(*tables)
        nh, V, n_pot = len(arrs[2]), len(arrs[0]) - 1, len(arrs[7])
        l2g = None if loc2glob is None else np.ascontiguousarray(loc2glob, np.int32)
        if l2g is not None and len(l2g) != nh:
            raise ValueError("loc2glob: one number per hypothesis")
        part = AffinityPart(int(h0), nh if h1 is None else int(h1), int(pos_base), None if l2g is None else l2g.ctypes.data_as(C.c_void_p), int(bool(assume_symmetric)))
        flags, needs_prev = np.zeros(n_pot + 1, np.uint8), np.zeros(V + 1, np.int32)
        first = np.zeros(nh + 1, np.uint64)
        pairs, w = C.c_void_p(), C.c_void_p()
        self._chk(self.lib.l3d_test_affinity_fill(self.h, C.byref(inp), C.byref(part), _p(flags), _p(needs_prev), C.byref(pairs), C.byref(w), _p(first)))
        n = int(part.n_passed)
        out_pairs, out_w = np.zeros((n, 2), np.int32), np.zeros(n, np.float32)
        if n:
            C.memmove(out_pairs.ctypes.data, pairs, n * 8)
            C.memmove(out_w.ctypes.data, w, n * 4)
        self.lib.l3d_free(pairs)
        self.lib.l3d_free(w)
        return dict(flags=flags[:n_pot], needs_prev=needs_prev[:V], n_launches=int(part.n_launches), coll_sym=int(part.coll_sym),
                    n_candidates=int(part.n_candidates), n_passed=n, pairs=out_pairs, w=out_w, first=first[:nh])

    def affinity_fill(self, seg_base, view_hyp_begin, hyp, score, hyp_dense, best, pot_start, pot_tgt, coll_start, coll_other, coll_w, sigma_a):
        """l3d_affinity_fill: flat tables -> (edges EDGE_DTYPE, node_hyp int32, number of enumerated candidate pairs)."""
        inp, arrs = self._affinity_input(seg_base, view_hyp_begin, hyp, score, hyp_dense, best, pot_start, pot_tgt, coll_start, coll_other, coll_w, sigma_a)
        edges, nodes = C.c_void_p(), C.c_void_p()
        ne, nn, nc = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.lib.l3d_affinity_fill(self.h, C.byref(inp), C.byref(edges), C.byref(ne), C.byref(nodes), C.byref(nn), C.byref(nc)))
        A = np.zeros(ne.value, dtype=EDGE_DTYPE)
        node_hyp = np.zeros(nn.value, dtype=np.int32)
        if ne.value:
            C.memmove(A.ctypes.data, edges, ne.value * 12)
        if nn.value:
            C.memmove(node_hyp.ctypes.data, nodes, nn.value * 4)
        self.lib.l3d_free(edges)
        self.lib.l3d_free(nodes)
        return A, node_hyp, nc.value

    def chain_release_records(self):
        """l3d_chain_release_records: the kept arena, its side words and run tables, the early transposes and the chain's scratch go back to the
        device; the products stay.  chain_kept_list raises afterwards, until the next chain."""
        self._chk(self.lib.l3d_chain_release_records(self.h))

    def chain_records_digest(self, n: int):
        """l3d_chain_records_digest: (uint64 digests, int32 lengths) of the kept lists of the n chain views of the resident products"""
        hsh, cnt = np.zeros(n, np.uint64), np.zeros(n, np.int32)
        self._chk(self.lib.l3d_chain_records_digest(self.h, hsh.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.c_int(n)))
        return hsh, cnt

    def chain_kept_list(self, index: int):
        """l3d_chain_kept_list: the kept list of chain view `index` out of the resident arena (MATCH_DTYPE array); partitioned products: the
        views this rank holds, empty for the others"""
        p, n = C.c_void_p(), C.c_int(0)
        self._chk(self.lib.l3d_chain_kept_list(self.h, C.c_int(index), C.byref(p), C.byref(n)))
        out = np.zeros(n.value, dtype=MATCH_DTYPE)
        if n.value:
            C.memmove(out.ctypes.data, p, n.value * 32)
        self.lib.l3d_free(p)
        return out

    def last_fill_counts(self):
        """(candidate pairs enumerated, candidates that passed their threshold) of the last affinity fill on this context, as 64-bit counts"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.l3d_last_fill_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def clustering_edges(self, edges, n_nodes, perform_diffusion=False, iters=10):
        """l3d_clustering_edges: (diffused, symmetrised) edge list in performClustering's stable ascending weight order."""
        edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        out = np.zeros(len(edges), dtype=EDGE_DTYPE)
        self._chk(self.lib.l3d_clustering_edges(self.h, _p(edges), C.c_int(len(edges)), C.c_int(n_nodes), C.c_int(int(perform_diffusion)),
                                                C.c_int(iters), _p(out)))
        return out

    def clustering_edges_grouped(self, edges, n_nodes, perform_diffusion=False, iters=10):
        """l3d_clustering_edges_grouped: -> (edges grouped by connected component, stable ascending weight inside a group; group_start)."""
        edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        out = np.zeros(len(edges), dtype=EDGE_DTYPE)
        gs = C.POINTER(C.c_int32)()
        ng = C.c_int(0)
        self._chk(self.lib.l3d_clustering_edges_grouped(self.h, _p(edges), C.c_int(len(edges)), C.c_int(n_nodes), C.c_int(int(perform_diffusion)),
                                                        C.c_int(iters), _p(out), C.byref(gs), C.byref(ng)))
        start = np.ctypeslib.as_array(gs, (ng.value + 1,)).copy() if ng.value else np.zeros(1, np.int32)
        self.lib.l3d_free(gs)
        return out, start

    def perform_clustering_device(self, edges, n_nodes, c=1.0, perform_diffusion=False, iters=10):
        """l3d_perform_clustering_device: [diffusion +] performClustering's merge loop on the device -> (labels (n_nodes,), components with an edge)."""
        edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        labels = np.full(max(n_nodes, 1), -1, dtype=np.int32)
        nc = C.c_int(0)
        self._chk(self.lib.l3d_perform_clustering_device(self.h, _p(edges), C.c_int(len(edges)), C.c_int(n_nodes), C.c_int(int(perform_diffusion)),
                                                         C.c_int(iters), C.c_float(c), _p(labels), C.byref(nc)))
        return labels[:n_nodes], nc.value

    def fit_clusters(self, group_start, member_hyp, hyp, hyp_cam, Rinv, scale_inv, tneg):
        """l3d_fit_clusters: -> list (one per cluster) of lists of (start (3,), end (3,)) float64."""
        gs = np.ascontiguousarray(group_start, np.int32)
        mh = np.ascontiguousarray(member_hyp, np.int32)
        hy = np.ascontiguousarray(hyp, HYP_DTYPE)
        hc = np.ascontiguousarray(hyp_cam, np.uint32)
        R = np.ascontiguousarray(Rinv, np.float64).reshape(9)
        t = np.ascontiguousarray(tneg, np.float64).reshape(3)
        cnt, segs = C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()
        n = C.c_int(0)
        ng = len(gs) - 1
        self._chk(self.lib.l3d_fit_clusters(self.h, _p(gs), C.c_int(ng), _p(mh), _p(hy), _p(hc), C.c_int(len(hy)), _p(R), C.c_double(scale_inv), _p(t),
                                            C.byref(cnt), C.byref(segs), C.byref(n)))
        counts = np.ctypeslib.as_array(cnt, (ng,)).copy() if ng else np.zeros(0, np.int32)
        flat = np.ctypeslib.as_array(segs, (n.value * 6,)).copy().reshape(-1, 6) if n.value else np.zeros((0, 6))
        self.lib.l3d_free(cnt)
        self.lib.l3d_free(segs)
        out, k = [], 0
        for c in counts:
            out.append([(flat[k + i, :3].copy(), flat[k + i, 3:].copy()) for i in range(c)])
            k += int(c)
        return out

    def refine_lines(self, group_start, member_cam, member_seg, member_pts, cameras, max_iterations=None, huber_px=None):
        """l3d_refine_lines: clusters as group_start (n_groups + 1) into member_cam (n,), member_seg (n, 4) float32, member_pts (n, 6) float64; cameras
        (n_cameras, 3, 4).  max_iterations and huber_px both None: the defaults (20, 2.0).  -> dict of line (n_groups, 6), rms_before, rms_after,
        iterations, status, seg_count (n_groups,) and segs (n_segs, 6), the clusters' segments back to back."""
        rc, out = _refine_call(self.lib.l3d_refine_lines, (self.h,), group_start, member_cam, member_seg, member_pts, cameras, max_iterations, huber_px)
        self._chk(rc)
        return out

    def mask_segments(self, segments, mask, **kw):
        """l3d_mask_segments: segments (n, 4) float32 through a segment mask ("A SEGMENT MASK") -> (segments (k, 4) float32, src_index (k,) int32),
        the input segment every output came from.  mask: a capi.segment_mask(...), or a mask array / device object with segment_mask's keywords
        (lens=, camera=, mode=, threshold=, keep_permille=, max_gap=, min_length=).  segments may be a device object (a float32 (n, 4) device
        tensor, contiguous and 16-byte aligned): it is read in place (l3d_mask_segments_device), like a device mask; the caller has synchronised
        whatever wrote them.  The result is host memory either way."""
        m = None if mask is None else _as_segment_mask(mask, kw)
        if hasattr(segments, "__cuda_array_interface__"):
            iface = segments.__cuda_array_interface__
            shape, strides = tuple(int(v) for v in iface["shape"]), iface.get("strides")
            if len(shape) != 2 or shape[1] != 4 or str(iface["typestr"]) != "<f4" or (strides is not None and tuple(int(v) for v in strides) != (16, 4)):
                raise TypeError("device segments must be a contiguous float32 array n x 4")
            rc, segs, idx = _mask_segments_call(self.lib.l3d_mask_segments_device, (self.h,), C.c_void_p(int(iface["data"][0]) or None), shape[0], m)
        else:
            s = np.ascontiguousarray(segments, np.float32).reshape(-1, 4)
            rc, segs, idx = _mask_segments_call(self.lib.l3d_mask_segments, (self.h,), _p(s) if len(s) else None, len(s), m)
        self._chk(rc)
        return segs, idx

    def project_lines(self, seg3d, cams, near=1e-6, margin=0.0):
        """l3d_project_lines: 3-D segments (n, 6) float64 (P then Q) into the cameras (capi.cameras(...), or a list of (K, R, t, width, height))
        ("PROJECTION AND OVERLAYS") -> (seg2d (k, 4) float32, src_index (k,) int32, flags (k,) uint8, cam_start (m + 1,) int64): camera-major,
        input order within a camera; flags bit 0 / 1: the P / Q end was moved by the near plane or the image's border.  seg3d may be a device
        object (a contiguous float64 (n, 6) device tensor): it is read in place (l3d_project_lines_device); the caller has synchronised whatever
        wrote it.  The result is host memory either way."""
        if hasattr(seg3d, "__cuda_array_interface__"):
            iface = seg3d.__cuda_array_interface__
            shape, strides = tuple(int(v) for v in iface["shape"]), iface.get("strides")
            if len(shape) != 2 or shape[1] != 6 or str(iface["typestr"]) != "<f8" or (strides is not None and tuple(int(v) for v in strides) != (48, 8)):
                raise TypeError("device segments must be a contiguous float64 array n x 6")
            arr = cameras(cams)
            m = getattr(arr, "_n", len(arr))
            rc, segs, idx, fl, start = _project_call(self.lib.l3d_project_lines_device, (self.h,), C.c_void_p(int(iface["data"][0]) or None), shape[0],
                                                     arr if m else None, m, near, margin)
        else:
            s, arr, m = _project_arguments(seg3d, cams)
            rc, segs, idx, fl, start = _project_call(self.lib.l3d_project_lines, (self.h,), _p(s) if len(s) else None, len(s), arr if m else None, m, near, margin)
        self._chk(rc)
        return segs, idx, fl, start

    def support_lines(self, seg3d, cams, segments_per_camera, params=None):
        """l3d_support_lines: the 2-D segments of every camera that support each 3-D segment ("SUPPORT OF 3-D LINES").  seg3d (n, 6) float64 (P then
        Q); cams as project_lines takes them; segments_per_camera: one (k, 4) float32 array per camera; params: capi.support_params(...) (None: 3 px,
        5 degrees, overlap 0.5, near 1e-6, margin 3) -> dict(records: SUPPORT_RECORD array (seg3d, seg2d within the camera, dist, overlap), ordered by
        (camera, seg3d, seg2d); cam_start (m + 1,) int64; best (all 2-D segments,) int32: the 3-D segment nearest to each, -1 for none; counts (4,)
        int64: rows, eligible columns, records, columns with a best row).  With seg3d a device object (a contiguous float64 (n, 6) device tensor),
        segments_per_camera is (a contiguous float32 (T, 4) device tensor, seg_start (m + 1,)): both are read in place (l3d_support_lines_device);
        the caller has synchronised whatever wrote them.  The result is host memory either way."""
        prm = support_params() if params is None else params
        if hasattr(seg3d, "__cuda_array_interface__"):
            cols, start = segments_per_camera
            start = np.ascontiguousarray(start, np.int64).reshape(-1)
            ptrs = []
            for obj, width, typestr, what in ((seg3d, 6, "<f8", "float64 array n x 6"), (cols, 4, "<f4", "float32 array T x 4")):
                if not hasattr(obj, "__cuda_array_interface__"):
                    raise TypeError("support lines: with device 3-D segments the 2-D segments are a device object too")
                iface = obj.__cuda_array_interface__
                shape, strides = tuple(int(v) for v in iface["shape"]), iface.get("strides")
                item = 8 if width == 6 else 4
                if len(shape) != 2 or shape[1] != width or str(iface["typestr"]) != typestr or (strides is not None and tuple(int(v) for v in strides) != (width * item, item)):
                    raise TypeError("device segments must be a contiguous " + what)
                ptrs.append((C.c_void_p(int(iface["data"][0]) or None), shape[0]))
            arr = cameras(cams)
            m = getattr(arr, "_n", len(arr))
            if len(start) != m + 1 or (m > 0 and int(start[-1]) != ptrs[1][1]):
                raise ValueError("support lines: seg_start has one entry per camera and one more, the last the number of 2-D segments")
            rc, out = _support_call(self.lib.l3d_support_lines_device, (self.h,), ptrs[0][0], ptrs[0][1], arr if m else None, m, ptrs[1][0], start, prm)
        else:
            s, arr, m = _project_arguments(seg3d, cams)
            cols, start = support_columns(segments_per_camera)
            if len(start) != m + 1:
                raise ValueError("support lines: one array of 2-D segments per camera")
            rc, out = _support_call(self.lib.l3d_support_lines, (self.h,), _p(s) if len(s) else None, len(s), arr if m else None, m, _p(cols) if len(cols) else None,
                                    start, prm)
        self._chk(rc)
        return out

    def merge_lines(self, lines, tol, cos_min=None, max_gap=0.0, params=None):
        """l3d_merge_lines: duplicate 3-D lines grouped on the device ("MERGING DUPLICATE LINES").  lines (n, 6) float64 (P then Q), tol (n,) float64
        in scene units; cos_min None: cos(5 degrees) -> dict(group (n,) int32: the lowest index of the line's group, pairs (k, 2) int32 ascending
        by (i, j), counts (4,) int32: eligible lines, components with a pair, lines released, groups of two or more)."""
        rc, out = _merge_call(self.lib.l3d_merge_lines, (self.h,), lines, tol, merge_params(cos_min, max_gap) if params is None else params)
        self._chk(rc)
        return out

    def junction_lines(self, lines, tol, ext, cos_max=None, crossings=0, params=None):
        """l3d_junction_lines: where 3-D lines meet, on the device ("JUNCTIONS OF 3-D LINES").  lines (n, 6) float64 (P then Q), tol and ext (n,) float64
        in scene units; cos_max None: cos(10 degrees) -> dict(records: JUNCTION_RECORD array ascending by (i, j), node_vertex (2 n,) int32: per line
        end 2 k + e its vertex or -1, vertices: JUNCTION_VERTEX array, node_attach (2 n,) int32: per free end its T record or -1, counts (8,) int32:
        eligible lines, L, T and X records, components with an edge, vertices, nodes released, nodes attached)."""
        rc, out = _junction_call(self.lib.l3d_junction_lines, (self.h,), lines, tol, ext, junction_params(cos_max, crossings) if params is None else params)
        self._chk(rc)
        return out

    def plane_lines(self, lines, tol, seeds, cos_max=None, cos_min=None, min_lines=3, params=None):
        """l3d_plane_lines: which 3-D lines lie in one plane, on the device ("PLANES OF 3-D LINES").  lines (n, 6) float64 (P then Q), tol (n,) float64
        in scene units, seeds (m, 2) int32: pairs of lines that meet; cos_max None: cos(10 degrees), cos_min None: cos(10 degrees) ->
        dict(planes: PLANE array in the order of their lowest staying seeds, members: PLANE_MEMBER array ascending by (plane, line), hyp_plane (m,)
        int32: per seed the plane it stays in or -1, counts (8,) int32: eligible lines, eligible hypotheses, hypothesis edges, components, hypotheses
        released, candidates dropped, planes, member records)."""
        rc, out = _plane_call(self.lib.l3d_plane_lines, (self.h,), lines, tol, seeds, plane_params(cos_max, cos_min, min_lines) if params is None else params)
        self._chk(rc)
        return out

    def draw_segments(self, image, segments, colors, color_index=None, width_px=1.0, opacity=255, layout=None, chan=None):
        """l3d_draw_segments: segments (n, 4) float32 in the image's grid drawn over 8-bit pixels ("PROJECTION AND OVERLAYS").  colors: (n_colors, 4)
        uint8, (c0, c1, c2, alpha) in the image's channel order; segment k takes colors[color_index[k]], or colors[k % n_colors] without
        color_index.  A numpy image H x W or H x W x C gives a NEW array; a device object (a uint8 device tensor, a capi.device_image(...)
        descriptor; layout and chan as device_image takes them) is drawn in place and returned (l3d_draw_segments_device)."""
        s, col, idx = _draw_arguments(segments, colors, color_index)
        tail = (_p(s) if len(s) else None, C.c_int(len(s)), _p(col) if len(col) else None, C.c_int(len(col)), None if idx is None else _p(idx),
                C.c_double(width_px), C.c_int(opacity))
        if is_device_object(image):
            d = device_image(image, layout=layout, chan=chan)
            self._chk(self.lib.l3d_draw_segments_device(self.h, C.byref(d), *tail))
            return image
        out = _draw_image_copy(image)
        ptr, w, h, ch, stride = image_arguments(out)
        self._chk(self.lib.l3d_draw_segments(self.h, ptr, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), *tail))
        return out

    def covisibility(self, lists):
        """l3d_covisibility: what Line3D::processWorldpointList files for the views' world point lists (one array of uint32 ids per view, in add
        order), counted on the device ("CO-VISIBILITY") -> (num_wps (V,) uint32, row_start (V + 1,) int32, col int32, count uint32, path): the
        non-zero common_wps as a CSR over list indices, columns ascending; path 1: a list named an id twice and the lists were replayed on the host"""
        ids, start = covisibility_arguments(lists)
        rc, out = _covisibility_call(self.lib.l3d_covisibility, (self.h,), _p(ids), _p(start), len(start) - 1)
        self._chk(rc)
        return out

    def fit_labelled_clusters(self, labels, node_hyp, hyp, hyp_cam, Rinv, scale_inv, tneg):
        """l3d_fit_labelled_clusters: -> (group_start, member_hyp, list per fitted cluster of (start, end))."""
        lab = np.ascontiguousarray(labels, np.int32)
        nh = np.ascontiguousarray(node_hyp, np.int32)
        hy = np.ascontiguousarray(hyp, HYP_DTYPE)
        hc = np.ascontiguousarray(hyp_cam, np.uint32)
        R = np.ascontiguousarray(Rinv, np.float64).reshape(9)
        t = np.ascontiguousarray(tneg, np.float64).reshape(3)
        gs, mh, cnt, segs = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()
        ng, n = C.c_int(0), C.c_int(0)
        self._chk(self.lib.l3d_fit_labelled_clusters(self.h, _p(lab), _p(nh), C.c_int(len(lab)), _p(hy), _p(hc), C.c_int(len(hy)), _p(R), C.c_double(scale_inv), _p(t),
                                                     C.byref(gs), C.byref(mh), C.byref(ng), C.byref(cnt), C.byref(segs), C.byref(n)))
        g = ng.value
        group_start = np.ctypeslib.as_array(gs, (g + 1,)).copy() if g else np.zeros(1, np.int32)
        members = np.ctypeslib.as_array(mh, (int(group_start[-1]),)).copy() if g and group_start[-1] else np.zeros(0, np.int32)
        counts = np.ctypeslib.as_array(cnt, (g,)).copy() if g else np.zeros(0, np.int32)
        flat = np.ctypeslib.as_array(segs, (n.value * 6,)).copy().reshape(-1, 6) if n.value else np.zeros((0, 6))
        for q in (gs, mh, cnt, segs):
            self.lib.l3d_free(q)
        out, k = [], 0
        for c in counts:
            out.append([(flat[k + i, :3].copy(), flat[k + i, 3:].copy()) for i in range(c)])
            k += int(c)
        return group_start, members, out

    def test_contract_math(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        e = np.zeros(len(x), np.float32)
        ac = np.zeros(len(x), np.float32)
        acd = np.zeros(len(x), np.float64)
        self._chk(self.lib.l3d_test_contract_math(self.h, _p(x), C.c_int(len(x)), _p(e), _p(ac), _p(acd)))
        return e, ac, acd

    def test_exclusive_sum(self, x):
        """l3d_test_exclusive_sum: int32 (n,) -> its exclusive prefix sums, int32 (n,)"""
        x = np.ascontiguousarray(x, dtype=np.int32)
        out = np.zeros(len(x), np.int32)
        self._chk(self.lib.l3d_test_exclusive_sum(self.h, _p(x), C.c_int(len(x)), _p(out)))
        return out


class NodeComm:
    """The in-process all-gather of the ranks of one process (l3d_node_comm_*, the adapter l3d_exchange_node): rank r on devices[r], a device may
    repeat.  Bind each rank's stream (the stream its exchanges arrive on), then hand `h.value` as exchange_user with exchange "node" to
    Line3D.shard_run / partition_run, or call `exchange` directly.  A broken communicator (abort(), a failed exchange) fails every later exchange."""

    def __init__(self, devices):
        self.lib = load_library()
        self.lib.l3d_node_comm_destroy.argtypes = [C.c_void_p]
        self.lib.l3d_node_comm_abort.argtypes = [C.c_void_p]
        self.lib.l3d_node_comm_bind.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.lib.l3d_exchange_node.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.devices = [int(d) for d in devices]
        devs = np.ascontiguousarray(self.devices, dtype=np.int32)
        h = C.c_void_p()
        rc = self.lib.l3d_node_comm_create(_p(devs) if len(devs) else None, C.c_int(len(devs)), C.byref(h))
        if rc != 0:
            raise L3DError("l3d_node_comm_create(%s) failed (code %d)" % (self.devices, rc))
        self.h = h

    def bind(self, rank: int, stream: int):
        rc = self.lib.l3d_node_comm_bind(self.h, C.c_int(rank), C.c_void_p(stream))
        if rc != 0:
            raise L3DError("l3d_node_comm_bind(rank %d) failed (code %d)" % (rank, rc))

    def exchange(self, view: int, send_ptr: int, recv_ptr: int, slot_bytes: int, stream: int) -> int:
        """rank (of `stream`)'s all-gather of one slot: 0 = enqueued"""
        return int(self.lib.l3d_exchange_node(self.h, C.c_int(view), C.c_void_p(send_ptr), C.c_void_p(recv_ptr), C.c_size_t(slot_bytes),
                                              C.c_int(len(self.devices)), C.c_void_p(stream)))

    def abort(self):
        self.lib.l3d_node_comm_abort(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.l3d_node_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
