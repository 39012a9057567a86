"""SfM front ends over the C ABI: VisualSfM NVM and bundler files -> what Line3D::addImage needs, and the
drivers' flow (main_vsfm.cpp / main_bundler.cpp) with segments supplied instead of images."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import load_library


class SfmScene:
    """cameras: list of dicts {name, focal, dist (2,), cv_dist (2,), R (3,3), t (3,), worldpoints (uint32 array)}.  dist: the file's own numbers;
    cv_dist: (k1, k2) in OpenCV's convention, as the drivers use them (l3d_sfm_camera_cv_distortion) -- what add_image_pixels(dist=...) takes.
    A camera of a COLMAP model (read_colmap) has in addition: camera_id, model and params (the file's own numbers), size = (width, height), and --
    unless the model has no lens in this library (FOV, THIN_PRISM_FISHEYE: lens_error says so) -- lens (capi.lens: what add_image_pixels(lens=...)
    takes) and K (3 x 3), both with the principal point moved by half a pixel (include/line3d_amd.h).  cv_dist is None where the model has no
    (k1, k2) form."""

    def __init__(self, cameras, n_points):
        self.cameras = cameras
        self.n_points = n_points


def _read(path: str, fn_name: str) -> SfmScene:
    lib = load_library()
    lib.l3d_sfm_last_error.restype = C.c_char_p
    lib.l3d_sfm_last_error.argtypes = [C.c_void_p]
    lib.l3d_sfm_camera_name.restype = C.c_char_p
    lib.l3d_sfm_camera_name.argtypes = [C.c_void_p, C.c_int]
    lib.l3d_sfm_free.argtypes = [C.c_void_p]
    h = C.c_void_p()
    rc = getattr(lib, fn_name)(path.encode(), C.byref(h))
    try:
        if rc != 0:
            raise RuntimeError(lib.l3d_sfm_last_error(h).decode() if h else "cannot read %s" % path)
        cams = []
        for i in range(lib.l3d_sfm_num_cameras(h)):
            focal = C.c_double(0)
            dist = (C.c_double * 2)()
            R = (C.c_double * 9)()
            t = (C.c_double * 3)()
            nw = C.c_int(0)
            lib.l3d_sfm_camera(h, C.c_int(i), C.byref(focal), dist, R, t, C.byref(nw))
            cv = (C.c_double * 2)()
            has_cv = lib.l3d_sfm_camera_cv_distortion(h, C.c_int(i), cv) == 0
            w = np.zeros(nw.value, dtype=np.uint32)
            if nw.value:
                lib.l3d_sfm_camera_worldpoints(h, C.c_int(i), w.ctypes.data_as(C.c_void_p))
            cams.append(dict(name=lib.l3d_sfm_camera_name(h, C.c_int(i)).decode(), focal=focal.value, dist=np.array(list(dist)),
                             cv_dist=np.array(list(cv)) if has_cv else None, R=np.array(list(R)).reshape(3, 3), t=np.array(list(t)), worldpoints=w))
            if fn_name == "l3d_sfm_read_colmap":
                name, params, n = C.c_char_p(), C.POINTER(C.c_double)(), C.c_int(0)
                lib.l3d_sfm_camera_model(h, C.c_int(i), C.byref(name), C.byref(params), C.byref(n))
                lens, K, width, height = capi.Lens(), (C.c_double * 9)(), C.c_int(0), C.c_int(0)
                lib.l3d_sfm_camera_id.restype = C.c_int
                cams[-1].update(camera_id=int(lib.l3d_sfm_camera_id(h, C.c_int(i))), model=name.value.decode(), params=np.array([params[k] for k in range(n.value)]))
                if lib.l3d_sfm_camera_lens(h, C.c_int(i), C.byref(lens), K, C.byref(width), C.byref(height)) == 0:
                    cams[-1].update(lens=lens, K=np.array(list(K)).reshape(3, 3), size=(width.value, height.value))
                else:
                    cams[-1].update(lens=None, K=None, size=None, lens_error=lib.l3d_sfm_last_error(h).decode())
        return SfmScene(cams, lib.l3d_sfm_num_points(h))
    finally:
        if h:
            lib.l3d_sfm_free(h)


def read_nvm(path: str) -> SfmScene:
    """main_vsfm.cpp:121-223"""
    return _read(path, "l3d_sfm_read_nvm")


def read_bundler(path: str) -> SfmScene:
    """main_bundler.cpp:110-204 (bundle.rd.out)"""
    return _read(path, "l3d_sfm_read_bundler")


def read_colmap(model_dir: str) -> SfmScene:
    """A COLMAP model folder: cameras.bin + images.bin, else cameras.txt + images.txt (l3d_sfm_read_colmap); one camera of the scene per image"""
    return _read(model_dir, "l3d_sfm_read_colmap")


def _lens_active(cam) -> bool:
    """the camera has a lens that changes the image (a fisheye always does)"""
    lens = cam.get("lens")
    return lens is not None and (lens.model != capi.LENS_BROWN or any(abs(v) > 1e-12 for v in lens.k))


def intrinsics(focal: float, width: int, height: int) -> np.ndarray:
    """main_vsfm.cpp:232-241"""
    K = (C.c_double * 9)()
    load_library().l3d_sfm_intrinsics(C.c_double(focal), C.c_uint(width), C.c_uint(height), K)
    return np.array(list(K)).reshape(3, 3)


def result_basename(max_width=-1, neighbors=10, min_uncertainty=1.0, max_uncertainty=5.0, sigma_p=3.5, sigma_a=10.0,
                    collinearity=True, diffusion=False) -> str:
    """The drivers' output name (main_vsfm.cpp:289-313), numbers in stream-default formatting."""
    n = "N_ALL__" if neighbors < 0 else "N_%d__" % neighbors
    return ("line3D_result__W_%d__%stL_%g__tU_%g__sigmaP_%g__sigmaA_%g__%s__%s"
            % (max_width, n, min_uncertainty, max_uncertainty, sigma_p, sigma_a,
               "COLLIN" if collinearity else "NO_COLLIN", "DIFFUSION" if diffusion else "NO_DIFFUSION"))


def reconstruct(scene: SfmScene, segments, image_sizes, out_dir=None, neighbors=10, diffusion=False, device=0, masks=None, mask_mode="split", mask_threshold=1,
                mask_keep_permille=500, mask_max_gap=0, mask_min_length=0.0, covisibility="host", merge=False, support=False, junctions=False, planes=False, **line3d_kwargs):
    """The drivers' flow (main_vsfm.cpp:226-325) with detected segments in place of images: K from focal and image size,
    addImage with the world point lists, compute3Dmodel, optional STL + TXT output under the drivers' file name.
    segments[i]: (S,4) float32 of camera i (undistorted image coordinates); image_sizes[i]: (width, height).
    segments may also be a DIRECTORY: the reference's data directory (main_vsfm.cpp:108-116, "<image folder>/L3D_data"),
    whose segment caches "segments_<id>_<w>x<h>_coll<0|1>.bin" of an earlier run are replayed (line3D.cc:143-168).
    masks: None, or a callable image name -> mask (a uint8 / bool array H x W of the image's size, or a device object; a byte >= mask_threshold is
    valid) or None for an image without one (COLMAP's mask_path read by the caller).  The image's segments -- given, or replayed from a cache, whose
    collinearities are then computed anew -- go through the mask on the device first ("A SEGMENT MASK", capi.segment_mask): mask_mode "drop",
    "clip" or "split" with mask_keep_permille, mask_max_gap and mask_min_length beside it.  An image whose segments all fall to its mask adds no view.
    covisibility: "host" files the world point links as the views are added, "device" counts them on the GPU in compute3Dmodel
    (Line3D.set_covisibility: the same neighbours and lines).
    merge: the duplicate 3-D lines of the result are merged on the device (Line3D.set_merging, defaults) before it is written.
    support: every line's 2-D segments are extended by the segments of ALL views that lie on it (Line3D.set_support, defaults), as the last step.
    junctions: where the lines meet is found on the device (Line3D.set_junctions, defaults; Line3D.junctions() and save3DLinesAsOBJ then hold the
    wireframe).
    planes: which lines lie in one plane is found on the device (Line3D.set_planes, defaults; Line3D.planes() and save3DPlanesAsOBJ then hold the faces)."""
    import os
    from . import capi
    from .pipeline import Line3D
    from .io import segment_cache_filename
    l3d = Line3D("", matchingNeighbors=neighbors, device=device, **line3d_kwargs)
    if merge:
        l3d.set_merging(True)
    if support:
        l3d.set_support(True)
    if junctions:
        l3d.set_junctions(True)
    if planes:
        l3d.set_planes(True)
    if covisibility != "host":
        l3d.set_covisibility(covisibility)

    def mask_of(cam):
        m = masks(cam["name"]) if masks is not None else None
        return None if m is None else capi.segment_mask(m, mode=mask_mode, threshold=mask_threshold, keep_permille=mask_keep_permille, max_gap=mask_max_gap,
                                                        min_length=mask_min_length)
    for i, cam in enumerate(scene.cameras):
        if np.any(np.abs(cam["dist"]) > 1e-12) or _lens_active(cam):
            raise RuntimeError("camera %d has lens distortion: segments of the undistorted image cannot be made from it here -- "
                               "reconstruct_from_images undistorts and detects from the pixels" % i)
        w, h = image_sizes[i]
        if isinstance(segments, (str, os.PathLike)):
            path = os.fspath(segments) + segment_cache_filename(i, w, h, line3d_kwargs.get("useCollinearity", True))
            if not os.path.exists(path):
                raise RuntimeError("no segment cache %s (this flow reads no image files: segments come from a cache or the caller; pixels go through Line3D.add_image_pixels)" % path)
            m = mask_of(cam)
            if not l3d.addImage_cached(i, w, h, path, intrinsics(cam["focal"], w, h), cam["R"], cam["t"], cam["worldpoints"], segment_mask=m) and m is not None:
                raise RuntimeError("camera %d: %s" % (i, l3d.lib.l3d_line3d_last_error(l3d.h).decode()))      # (a mask of another size than the image, ...)
            continue
        m = mask_of(cam)
        if not l3d.addImage(i, w, h, segments[i], intrinsics(cam["focal"], w, h), cam["R"], cam["t"], cam["worldpoints"], segment_mask=m) and m is not None:
            raise RuntimeError("camera %d: %s" % (i, l3d.lib.l3d_line3d_last_error(l3d.h).decode()))
    l3d.compute3Dmodel(diffusion)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        base = os.path.join(out_dir, result_basename(neighbors=neighbors, diffusion=diffusion))
        l3d.save3DLinesAsSTL(base + ".stl")
        l3d.save3DLinesAsTXT(base + ".txt")
    return l3d


def undistorted_for_view(ctx, img, en):
    """The image of an entry of reconstruct_from_images in its view's grid, as a host array H x W x 3: undistorted as the add undistorts it (k1, k2;
    a lens; a lens onto a planned size), a grey image repeated over three channels"""
    if en.get("out_size") is not None:
        out = ctx.undistort(img, en["K"], lens=en["lens"], out_size=en["out_size"])
    elif en.get("lens") is not None:
        out = ctx.undistort(img, en["K"], lens=en["lens"])
    elif en.get("dist") is not None and any(abs(float(c)) > 1e-12 for c in en["dist"]):
        out = ctx.undistort(img, en["K"], k1=float(en["dist"][0]), k2=float(en["dist"][1]))
    else:
        out = img
    if capi.is_device_object(out):
        out = out.cpu().numpy() if hasattr(out, "cpu") else out
    out = np.asarray(out, np.uint8)
    return np.ascontiguousarray(np.repeat(out[:, :, None], 3, axis=2) if out.ndim == 2 else out[:, :, :3])


def write_ppm(path, image):
    """A uint8 image H x W x 3 as a binary P6 file"""
    image = np.ascontiguousarray(image, np.uint8)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("write_ppm takes an H x W x 3 uint8 image")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (image.shape[1], image.shape[0]))
        f.write(image.tobytes())


def reconstruct_from_images(scene: SfmScene, load_image, data_directory, out_dir=None, neighbors=10, diffusion=False, max_width=1920,
                            load_and_store_segments=True, device=0, batch=16, refine=False, alpha=None, out_size=None, covisibility="host", overlay_dir=None,
                            merge=False, support=False, junctions=False, planes=False, **line3d_kwargs):
    """The drivers' flow (main_vsfm.cpp:226-325) from pixels: per camera the image load_image(i, name) returns -- `bytes`: the contents of a
    baseline JPEG file, decoded on the device (Line3D.add_image_jpeg); or a uint8 array H x W or H x W x 3, decoded by the caller; or an image
    in device memory (a torch device tensor, a capi.device_image descriptor), read where it lies --, K from the focal length and the image size, the image undistorted with the camera's coefficients and its
    segments detected on the device (Line3D.add_image_pixels(..., dist=cam["cv_dist"])); a camera that has `lens` and `K` (read_colmap) is added with
    those instead (Line3D.add_image_pixels(..., lens=cam["lens"]) with its own K); then compute3Dmodel, optional STL + TXT output under the
    drivers' file name.  data_directory: the drivers' "<image folder>/L3D_data/" -- with load_and_store_segments (the drivers' default) the segment
    caches are written there, and a cache of an earlier run stands in for the image (line3D.cc:143-168).  The images go to the library `batch`
    at a time (Line3D.add_images): the same views as one call per image, with the detector run once per batch.
    merge: the duplicate 3-D lines of the result are merged on the device (Line3D.set_merging, defaults), before the refinement.
    refine: the 3-D lines are refined against the 2-D segments of their clusters (Line3D.set_refinement, defaults) before they are written.
    support: every line's 2-D segments are extended by the segments of ALL views that lie on it (Line3D.set_support, defaults), after the refinement;
    the TXT file and the overlays then show them.
    junctions: where the lines meet is found on the device (Line3D.set_junctions, defaults), after the refinement and before the support.
    planes: which lines lie in one plane is found on the device (Line3D.set_planes, defaults), after the junctions and before the support.
    alpha, out_size (either given; "A REMAP" in include/line3d_amd.h): a camera with an active lens -- a COLMAP camera's, or an NVM / bundler camera's
    k1, k2 as a BROWN lens -- is PLANNED (capi.undistort_plan(lens, size, alpha or 0, out_size), once per distinct camera) and the view is added
    with the planned K and size, the blank pixels of the resampling invalid for the detector.  Neither given: what it did before.
    covisibility: as in reconstruct.
    overlay_dir: after compute3Dmodel every view's image is loaded once more, undistorted into the view's grid (Context.undistort with the entry's
    coefficients, lens or planned size) and written with the view's overlay (Line3D.overlay: its member segments and the projected lines it
    observes) as overlay_<imageID>.ppm, binary P6, into this directory."""
    import os
    from .pipeline import Line3D
    l3d = Line3D(data_directory, matchingNeighbors=neighbors, device=device, **line3d_kwargs)
    if merge:
        l3d.set_merging(True)
    if refine:
        l3d.set_refinement(True)
    if support:
        l3d.set_support(True)
    if junctions:
        l3d.set_junctions(True)
    if planes:
        l3d.set_planes(True)
    if covisibility != "host":
        l3d.set_covisibility(covisibility)
    entries = []
    added = []              # overlay_dir: what undistorts an entry's image into its view's grid
    planned = {}            # (lens, source size) -> (K, size): one plan per distinct camera

    def flush():
        for en, st in zip(entries, l3d.add_images(entries, maxImgWidth=max_width, loadAndStoreSegments=load_and_store_segments)):
            if st != 0:
                raise RuntimeError("camera %d: %s" % (en["imageID"], l3d.lib.l3d_line3d_last_error(l3d.h).decode()))
        del entries[:]

    for i, cam in enumerate(scene.cameras):         # `batch` images per add_images call: the detector runs over them together
        img = load_image(i, cam["name"])
        en = dict(imageID=i, R=cam["R"], t=cam["t"], worldpointIDs=cam["worldpoints"])
        if cam.get("lens") is not None and cam.get("K") is not None:       # a COLMAP camera: its own lens and K
            en["lens"] = cam["lens"]
        elif "lens_error" in cam:
            raise RuntimeError(cam["lens_error"])
        else:
            en["dist"] = cam["cv_dist"]
        if isinstance(img, (bytes, bytearray, memoryview)):
            from .capi import jpeg_info
            w, h, _ = jpeg_info(img)
            en["data"] = bytes(img)
            if entries and capi.is_device_object(entries[-1].get("img")):
                flush()
        elif capi.is_device_object(img):
            d = capi.device_image(img)
            w, h = d.width, d.height
            en["img"] = d
            if entries and not capi.is_device_object(entries[-1].get("img")):      # (a call takes device images or host images and files, not both)
                flush()
        else:
            img = np.asarray(img)
            h, w = img.shape[:2]
            en["img"] = img
            if entries and capi.is_device_object(entries[-1].get("img")):
                flush()
        en["K"] = cam["K"] if "lens" in en else intrinsics(cam["focal"], w, h)
        if alpha is not None or out_size is not None:
            K = np.asarray(en["K"], dtype=np.float64).reshape(3, 3)
            lens = en.get("lens")
            if lens is None and en.get("dist") is not None and any(abs(float(c)) > 1e-12 for c in en["dist"]):
                lens = capi.lens("brown", [float(c) for c in en["dist"]], camera=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
            active = lens is not None and (lens.model == capi.LENS_FISHEYE or any(abs(c) > 1e-12 for c in lens.k))
            if active and K[0, 1] == 0.0:
                if lens.fx == 0.0 and lens.fy == 0.0:           # a lens without a camera of its own: the entry's K is its source camera
                    lens = capi.lens(lens.model, list(lens.k), camera=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
                key = (lens.model, lens.fx, lens.fy, lens.cx, lens.cy, tuple(lens.k), w, h)
                if key not in planned:
                    planned[key] = capi.undistort_plan(lens, (w, h), 0.0 if alpha is None else alpha, out_size)
                en.pop("dist", None)
                en["lens"], en["K"], en["out_size"] = lens, planned[key][0], planned[key][1]
        entries.append(en)
        if overlay_dir is not None:
            added.append({k: en.get(k) for k in ("imageID", "K", "dist", "lens", "out_size")})
        if len(entries) >= batch:
            flush()
    if entries:
        flush()
    l3d.compute3Dmodel(diffusion)
    if overlay_dir is not None:
        os.makedirs(overlay_dir, exist_ok=True)
        from .capi import L3DError
        ctx = l3d.context()
        for i, (cam, en) in enumerate(zip(scene.cameras, added)):
            try:
                l3d.project_result([en["imageID"]], select="observed")
            except L3DError as e:                       # (an image in which nothing was detected is no view)
                if "unknown view" in str(e):
                    continue
                raise
            img = load_image(i, cam["name"])
            if isinstance(img, (bytes, bytearray, memoryview)):
                img = l3d.decode_jpeg(bytes(img))
            write_ppm(os.path.join(overlay_dir, "overlay_%d.ppm" % en["imageID"]), l3d.overlay(en["imageID"], undistorted_for_view(ctx, img, en)))
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        base = os.path.join(out_dir, result_basename(max_width=max_width, neighbors=neighbors, diffusion=diffusion))
        l3d.save3DLinesAsSTL(base + ".stl")
        l3d.save3DLinesAsTXT(base + ".txt")
    return l3d
