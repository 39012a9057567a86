"""Python mirror of the reference's operator interface, class L3D::Line3D (line3D.h:61-101), over the
C ABI (l3d_line3d_* in include/line3d_amd.h).  Same calls, argument meaning and defaults
(commons.h:42-61); images are replaced by their detected segments."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import MATCH_DTYPE, EDGE_DTYPE, L3DError, _p

# l3d_chain_summary (include/line3d_amd.h)
SUMMARY_DTYPE = np.dtype([("verified", np.int32), ("n_kept", np.int32), ("n_candidates", np.int64), ("median_depth", np.float32), ("pad", np.int32)])


def image_entries(entries):
    """The l3d_image_entry array of Line3D.add_images and what keeps its pointers alive.  Everything malformed is refused here, before any
    library call: neither or both of img and data, an image that is not uint8, neither or both kinds of links, links without ids."""
    entries = list(entries)
    arr, keep = (capi.ImageEntry * max(1, len(entries)))(), []

    def pointer(a):
        keep.append(a)
        return a.ctypes.data

    for i, en in enumerate(entries):
        e = arr[i]
        unknown = set(en) - {"imageID", "img", "data", "K", "R", "t", "dist", "lens", "out_size", "mask", "border_mask", "worldpointIDs", "viewSimilarity"}
        if unknown:
            raise ValueError("entry %d: unknown keys %s" % (i, sorted(unknown)))
        if (en.get("img") is None) == (en.get("data") is None):
            raise ValueError("entry %d needs either img (pixels) or data (a JPEG file), not both" % i)
        if (en.get("worldpointIDs") is None) == (en.get("viewSimilarity") is None):
            raise ValueError("entry %d needs either worldpointIDs or viewSimilarity, not both" % i)
        e.image_id = int(en["imageID"])
        if en.get("img") is not None:
            pix, w, h, ch, stride = capi.image_arguments(en["img"])
            keep.append(pix)
            e.pixels, e.width, e.height, e.channels, e.row_stride = pix.value, w, h, ch, stride
        else:
            if not isinstance(en["data"], (bytes, bytearray, memoryview, np.ndarray)):
                raise TypeError("entry %d: data must be the bytes of a JPEG file" % i)
            ptr, nbytes = capi._bytes_arguments(en["data"])
            keep.append(ptr)
            e.jpeg, e.jpeg_bytes = ptr.value, nbytes.value
        e.K, e.R, e.t = (pointer(np.ascontiguousarray(en[k], dtype=np.float64)) for k in ("K", "R", "t"))
        if en.get("dist") is not None:
            e.dist = pointer(np.ascontiguousarray(en["dist"], dtype=np.float64).reshape(2))
        if en.get("viewSimilarity") is not None:
            sim = en["viewSimilarity"]
            ids = np.ascontiguousarray(sorted(sim), dtype=np.uint32)
            e.sims = pointer(np.ascontiguousarray([sim[int(k)] for k in ids] + [0.0], dtype=np.float32))      # (never a null pointer: it says which kind of links)
        else:
            ids = np.ascontiguousarray(list(en["worldpointIDs"]), dtype=np.uint32)
        if ids.ndim != 1:
            raise ValueError("entry %d: link ids must be a flat list" % i)
        e.link_ids, e.n_links = pointer(np.concatenate([ids, np.zeros(1, np.uint32)])), len(ids)
    return arr, keep


def device_entries(entries):
    """The l3d_device_entry array of Line3D.add_images for entries whose img is a device object (capi.device_image), and what keeps its pointers
    alive; refusals as image_entries"""
    entries = list(entries)
    arr, keep = (capi.DeviceEntry * max(1, len(entries)))(), []

    def pointer(a):
        keep.append(a)
        return a.ctypes.data

    for i, en in enumerate(entries):
        e = arr[i]
        unknown = set(en) - {"imageID", "img", "data", "K", "R", "t", "dist", "lens", "out_size", "mask", "border_mask", "worldpointIDs", "viewSimilarity"}
        if unknown:
            raise ValueError("entry %d: unknown keys %s" % (i, sorted(unknown)))
        if en.get("img") is None or en.get("data") is not None:
            raise ValueError("entry %d needs img (an image in device memory) and no data" % i)
        if (en.get("worldpointIDs") is None) == (en.get("viewSimilarity") is None):
            raise ValueError("entry %d needs either worldpointIDs or viewSimilarity, not both" % i)
        e.image_id = int(en["imageID"])
        d = capi.device_image(en["img"])
        e.image = d
        keep.append(d)                  # (the descriptor keeps the object it was made from alive)
        e.K, e.R, e.t = (pointer(np.ascontiguousarray(en[k], dtype=np.float64)) for k in ("K", "R", "t"))
        if en.get("dist") is not None:
            e.dist = pointer(np.ascontiguousarray(en["dist"], dtype=np.float64).reshape(2))
        if en.get("viewSimilarity") is not None:
            sim = en["viewSimilarity"]
            ids = np.ascontiguousarray(sorted(sim), dtype=np.uint32)
            e.sims = pointer(np.ascontiguousarray([sim[int(k)] for k in ids] + [0.0], dtype=np.float32))      # (never a null pointer: it says which kind of links)
        else:
            ids = np.ascontiguousarray(list(en["worldpointIDs"]), dtype=np.uint32)
        if ids.ndim != 1:
            raise ValueError("entry %d: link ids must be a flat list" % i)
        e.link_ids, e.n_links = pointer(np.concatenate([ids, np.zeros(1, np.uint32)])), len(ids)
    return arr, keep


def _entries_on_device(entries, what):
    """True when every entry's img is a device object, False when none is; a mixed list raises ValueError before any library call"""
    return capi.all_device_objects([en.get("img") for en in entries], what)


def _camera_and_links(K, R, t, links, fixed_sim):
    """The K, R, t and link arguments of the segment-taking calls, and the arrays behind them.  links: world point ids, or {view id: similarity}
    with fixed_sim"""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (K, R, t)]
    if fixed_sim:
        ids = np.ascontiguousarray(sorted(links), dtype=np.uint32)
        arrays += [ids, np.ascontiguousarray([links[int(i)] for i in ids], dtype=np.float32)]
    else:
        ids = np.ascontiguousarray(list(links), dtype=np.uint32)
        arrays.append(ids)
    return [_p(a) for a in arrays] + [C.c_int(len(ids))], arrays


class Line3D:
    def __init__(self, data_directory: str = "", matchingNeighbors: int = 10, uncertainty_t_upper_2D: float = 5.0,
                 uncertainty_t_lower_2D: float = 1.0, sigma_p: float = 3.5, sigma_a: float = 10.0,
                 min_baseline: float = 0.25, useCollinearity: bool = True, verbose: bool = False, device: int | None = None, crosschecks: bool = False,
                 devices=None):
        """devices: a list of HIP device ids -- one object over several GPUs of this process (l3d_line3d_create_node: rank r on devices[r], a
        device may repeat); compute3Dmodel runs matchViews partitioned over the ranks.  device: the one GPU of an ordinary object."""
        if device is not None and devices is not None:
            raise ValueError("Line3D: give device or devices, not both")
        self.lib = capi.load_library(crosschecks)        # (crosschecks: the test-only build in which the L3D_HOST_* switches exist)
        self.lib.l3d_line3d_last_error.restype = C.c_char_p
        self.lib.l3d_line3d_last_error.argtypes = [C.c_void_p]
        self.lib.l3d_line3d_context.restype = C.c_void_p
        self.lib.l3d_line3d_context.argtypes = [C.c_void_p]
        self.lib.l3d_line3d_destroy.argtypes = [C.c_void_p]
        self.data_directory = data_directory          # kept for signature parity; nothing is written to disk
        h = C.c_void_p()
        params = (C.c_int(matchingNeighbors), C.c_float(uncertainty_t_upper_2D), C.c_float(uncertainty_t_lower_2D), C.c_float(sigma_p),
                  C.c_float(sigma_a), C.c_float(min_baseline), C.c_int(int(useCollinearity)), C.c_int(int(verbose)), C.byref(h))
        if devices is not None:
            devs = np.ascontiguousarray(list(devices), dtype=np.int32)
            rc = self.lib.l3d_line3d_create_node(_p(devs) if len(devs) else None, C.c_int(len(devs)), *params)
            if rc != 0:
                raise L3DError("l3d_line3d_create_node(%s) failed (code %d): no usable set of MI355X / HIP devices -- no CPU fallback"
                               % (list(devices), rc))
        else:
            rc = self.lib.l3d_line3d_create(C.c_int(0 if device is None else device), *params)
            if rc != 0:
                raise L3DError("l3d_line3d_create failed (code %d): no usable MI355X / HIP device -- no CPU fallback" % rc)
        self.h = h
        self._device = int(devices[0]) if devices is not None and len(devices) else int(device or 0)      # where the detector runs (a node object: rank 0's)
        self._keep = []
        self.last_rc = 0          # status of the last add_image_pixels* / add_image_jpeg* (they return a bool, as the other adders do)

    def close(self):
        if getattr(self, "h", None):
            self.lib.l3d_line3d_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise L3DError("line3d_amd error %d: %s" % (rc, self.lib.l3d_line3d_last_error(self.h).decode()))

    def num_ranks(self) -> int:
        """ranks of the object: len(devices) of a node object, 1 otherwise"""
        return int(self.lib.l3d_line3d_num_ranks(self.h))

    def set_node_mode(self, mode: int):
        """how compute3Dmodel shards matchViews over the ranks of a node object: 0 = segments of every view (default), 1 = blocks of views
        (falls back to 0 where its verdict says the speculation cannot hold), 2 = the ranks of a device take turns on it (a scene whose kept records do
        not fit the device at once; every turn computes the whole chain: matchViews costs about len(devices) single passes)"""
        self._chk(self.lib.l3d_line3d_set_node_mode(self.h, C.c_int(int(mode))))

    def node_turn_records(self, rank: int) -> int:
        """after compute3Dmodel in node mode 2: the kept records rank `rank` retired in its turn (l3d_line3d_node_turn_records)"""
        n = C.c_int64(0)
        self._chk(self.lib.l3d_line3d_node_turn_records(self.h, C.c_int(int(rank)), C.byref(n)))
        return int(n.value)

    def set_turn_handover(self, on=True):
        """node mode 2 with a warm hand-over between the turns (l3d_line3d_set_turn_handover): a turn computes its own piece of the chain from the
        tail its predecessor left, so matchViews costs between one and two passes instead of len(devices).  No effect unless the node mode is 2;
        `on` is True / False (or 1 / 0)"""
        self._chk(self.lib.l3d_line3d_set_turn_handover(self.h, C.c_int(int(on))))

    def node_turn_views(self, rank: int):
        """after compute3Dmodel in node mode 2: (chain views rank `rank` computed over all its visits, its visits) (l3d_line3d_node_turn_views)"""
        n, v = C.c_int64(0), C.c_int(0)
        self._chk(self.lib.l3d_line3d_node_turn_views(self.h, C.c_int(int(rank)), C.byref(n), C.byref(v)))
        return int(n.value), int(v.value)

    def context(self) -> capi.Context:
        """The pipeline's l3d_ctx as a (non-owning) Context, for profiling (refused on a node object: one context per rank)."""
        c = capi.Context.__new__(capi.Context)
        c.lib = self.lib
        ptr = self.lib.l3d_line3d_context(self.h)
        if not ptr:
            raise L3DError("line3d_amd: %s" % self.lib.l3d_line3d_last_error(self.h).decode())
        c.h = C.c_void_p(ptr)
        c._keep = []
        c.close = lambda: None
        return c

    # -- reference interface ------------------------------------------------------------------
    def _add_masked(self, imageID, width, height, segments, cache, K, R, t, links, fixed_sim, segment_mask):
        """the segment-taking adds behind a segment mask (l3d_line3d_add_image_masked / ..._cached_masked); the status stays in last_rc"""
        if not isinstance(segment_mask, capi.SegmentMask):
            raise TypeError("segment_mask must come from capi.segment_mask()")
        args, keep = _camera_and_links(K, R, t, links, fixed_sim)
        links_args = args[3:] if fixed_sim else [args[3], None, args[4]]           # link_ids, sims (None: world point ids), n_links
        head = [self.h, C.c_uint32(imageID), C.c_uint(width), C.c_uint(height)]
        if cache is not None:
            rc = self.lib.l3d_line3d_add_image_cached_masked(*head, cache, *args[:3], *links_args, C.byref(segment_mask))
        else:
            segs = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 4)
            rc = self.lib.l3d_line3d_add_image_masked(*head, _p(segs) if len(segs) else None, C.c_int(len(segs)), *args[:3], *links_args, C.byref(segment_mask))
        self.last_rc = int(rc)
        return rc == 0

    def addImage(self, imageID, width, height, segments, K, R, t, worldpointIDs, segment_mask=None):
        """segment_mask: None, or a capi.segment_mask(...) the segments go through first ("A SEGMENT MASK": dropped, clipped or split on the device;
        without a lens the mask has the view's size; segments that all fall to it add no view and the call is still True)"""
        if segment_mask is not None:
            return self._add_masked(imageID, width, height, segments, None, K, R, t, worldpointIDs, False, segment_mask)
        segs = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 4)
        args, keep = _camera_and_links(K, R, t, worldpointIDs, False)
        rc = self.lib.l3d_line3d_add_image(self.h, C.c_uint32(imageID), C.c_uint(width), C.c_uint(height), _p(segs), C.c_int(len(segs)), *args)
        return rc == 0          # the reference prints to cerr and returns (line3D.cc:101-127)

    def addImage_fixed_sim(self, imageID, width, height, segments, K, R, t, viewSimilarity, segment_mask=None):
        if segment_mask is not None:
            return self._add_masked(imageID, width, height, segments, None, K, R, t, viewSimilarity, True, segment_mask)
        segs = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 4)
        args, keep = _camera_and_links(K, R, t, viewSimilarity, True)
        rc = self.lib.l3d_line3d_add_image_fixed_sim(self.h, C.c_uint32(imageID), C.c_uint(width), C.c_uint(height), _p(segs), C.c_int(len(segs)), *args)
        return rc == 0

    def addImage_cached(self, imageID, width, height, cache_path, K, R, t, worldpointIDs, segment_mask=None):
        """addImage when the segment cache file exists (line3D.cc:160-168): segments and collinearities from the file.  With a segment_mask the
        file's segments go through the mask and the view computes its own collinearities; the file is not changed (there the links may also be
        {view id: similarity}, as addImage_fixed_sim takes them)."""
        from .io import open_segment_cache, close_segment_cache
        cache = open_segment_cache(cache_path)
        try:
            if segment_mask is not None:        # (the masked form also takes {view id: similarity} in the place of the world point ids)
                return self._add_masked(imageID, width, height, None, cache, K, R, t, worldpointIDs, isinstance(worldpointIDs, dict), segment_mask)
            args, keep = _camera_and_links(K, R, t, worldpointIDs, False)
            rc = self.lib.l3d_line3d_add_image_cached(self.h, C.c_uint32(imageID), C.c_uint(width), C.c_uint(height), cache, *args)
        finally:
            close_segment_cache(cache)
        return rc == 0

    def addImage_ex(self, imageID, width, height, segments, K, R, t, links, maxImgWidth=1920, loadAndStoreSegments=True, fixed_sim=False):
        """addImage / addImage_fixed_sim with the reference's segment-cache behaviour in `data_directory` (line3D.cc:128-199): the cache
        file is removed, read instead of `segments`, or written.  links: world point ids, or {view id: similarity} with fixed_sim."""
        segs = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 4)
        args, keep = _camera_and_links(K, R, t, links, fixed_sim)
        add = self.lib.l3d_line3d_add_image_fixed_sim_ex if fixed_sim else self.lib.l3d_line3d_add_image_ex
        rc = add(self.h, C.c_uint32(imageID), C.c_uint(width), C.c_uint(height), _p(segs), C.c_int(len(segs)), *args,
                 C.c_char_p(self.data_directory.encode()), C.c_int(maxImgWidth), C.c_int(int(loadAndStoreSegments)))
        return rc == 0

    def _add_entry(self, en, maxImgWidth, loadAndStoreSegments):
        """one image entry (as add_images takes them) through l3d_line3d_add_image_entry: True when it was taken; the status stays in last_rc.
        What is no image or no file raises TypeError, as image_arguments and bytes() do; image_entries speaks of "entry 0" in what it refuses.
        An entry with a lens goes through the ..._entry_lens form of the same call"""
        if en.get("lens") is None:
            en.pop("lens", None)
        lens = en.get("lens")
        if lens is not None and not isinstance(lens, capi.Lens):
            raise TypeError("lens must come from capi.lens()")
        tail = (C.c_char_p(self.data_directory.encode()), C.c_int(int(maxImgWidth)), C.c_int(int(loadAndStoreSegments)))
        remap_arr, remap_keep = capi.remap_pointers([lens], [en.get("out_size")], [en.get("mask")], [en.get("border_mask")], 1)
        if remap_arr is not None:           # another size, a mask or a border rule: the ..._entry_remap form
            if "data" in en and not isinstance(en["data"], (bytes, bytearray, memoryview, np.ndarray)):
                en["data"] = bytes(en["data"])
            on_device = capi.is_device_object(en.get("img"))
            arr, keep = (device_entries if on_device else image_entries)([en])
            call = self.lib.l3d_line3d_add_device_entry_remap if on_device else self.lib.l3d_line3d_add_image_entry_remap
            self.last_rc = call(self.h, arr, C.byref(remap_keep[0]), *tail)
            return self.last_rc == 0
        if capi.is_device_object(en.get("img")):
            arr, keep = device_entries([en])
            self.last_rc = self.lib.l3d_line3d_add_device_entry(self.h, arr, *tail) if lens is None else self.lib.l3d_line3d_add_device_entry_lens(self.h, arr, C.byref(lens), *tail)
            return self.last_rc == 0
        if "data" in en and not isinstance(en["data"], (bytes, bytearray, memoryview, np.ndarray)):
            en["data"] = bytes(en["data"])            # (whatever bytes() takes, as before; None or a str: TypeError)
        arr, keep = image_entries([en])
        self.last_rc = self.lib.l3d_line3d_add_image_entry(self.h, arr, *tail) if lens is None else self.lib.l3d_line3d_add_image_entry_lens(self.h, arr, C.byref(lens), *tail)
        return self.last_rc == 0

    def add_image_pixels(self, imageID, img, K, R, t, worldpointIDs, maxImgWidth=1920, loadAndStoreSegments=True, dist=None, lens=None, out_size=None, mask=None, border_mask=None):
        """Line3D::addImage from pixels (an image entry with img, include/line3d_amd.h): uint8 image H x W or H x W x 3.  The segment cache in
        `data_directory` is loaded when present (and loadAndStoreSegments); otherwise the segments are detected on the device, and the cache written
        or a stale one removed.  An image without segments adds no view and is no error (line3D.cc:186-190).  dist = (k1, k2), OpenCV-convention
        radial coefficients: the image is undistorted on the device with K before the detector sees it.
        img may be a device object (a torch device tensor, a capi.device_image descriptor): it is read where it lies (l3d_line3d_add_device_entry).
        lens (capi.lens(...)) in the place of dist: tangential, rational and fisheye models, the image resampled from the lens's source camera onto
        K, which the view keeps (l3d_line3d_add_image_entry_lens).  dist and lens together are refused by the library.
        out_size = (width, height), mask, border_mask ("A REMAP", l3d_line3d_add_image_entry_remap; also on the other image-taking add calls and as
        keys of add_images' entries): the image is resampled onto out_size -- the view's size, which names the cache file and which maxImgWidth
        acts on --, K is the output camera (capi.undistort_plan chooses one), mask (capi.remap's) is the caller's validity plane in the source
        grid, and no segment starts where a blank or masked pixel contributed to the gradient (border_mask, default true)."""
        return self._add_entry(dict(imageID=imageID, img=img if capi.is_device_object(img) else np.asarray(img), K=K, R=R, t=t, worldpointIDs=list(worldpointIDs), dist=dist, lens=lens, out_size=out_size, mask=mask, border_mask=border_mask), maxImgWidth, loadAndStoreSegments)

    def add_image_pixels_fixed_sim(self, imageID, img, K, R, t, viewSimilarity, maxImgWidth=1920, loadAndStoreSegments=True, dist=None, lens=None, out_size=None, mask=None, border_mask=None):
        """Line3D::addImage_fixed_sim from pixels; dist and device objects as in add_image_pixels"""
        return self._add_entry(dict(imageID=imageID, img=img if capi.is_device_object(img) else np.asarray(img), K=K, R=R, t=t, viewSimilarity=dict(viewSimilarity), dist=dist, lens=lens, out_size=out_size, mask=mask, border_mask=border_mask), maxImgWidth, loadAndStoreSegments)

    def add_image_jpeg(self, imageID, data, K, R, t, worldpointIDs, maxImgWidth=1920, loadAndStoreSegments=True, dist=None, lens=None, out_size=None, mask=None, border_mask=None):
        """Line3D::addImage from the bytes of a baseline JPEG file (an image entry with data): decoded, undistorted (dist = (k1, k2), None: not)
        and its segments detected on the device.  Cache rules as add_image_pixels; a cache that is present and wanted is loaded without decoding
        the file.  A file the decoder refuses adds no view and returns False (the cause: l3d_line3d_last_error)."""
        return self._add_entry(dict(imageID=imageID, data=data, K=K, R=R, t=t, worldpointIDs=list(worldpointIDs), dist=dist, lens=lens, out_size=out_size, mask=mask, border_mask=border_mask), maxImgWidth, loadAndStoreSegments)

    def add_image_jpeg_fixed_sim(self, imageID, data, K, R, t, viewSimilarity, maxImgWidth=1920, loadAndStoreSegments=True, dist=None, lens=None, out_size=None, mask=None, border_mask=None):
        """Line3D::addImage_fixed_sim from the bytes of a baseline JPEG file; as add_image_jpeg"""
        return self._add_entry(dict(imageID=imageID, data=data, K=K, R=R, t=t, viewSimilarity=dict(viewSimilarity), dist=dist, lens=lens, out_size=out_size, mask=mask, border_mask=border_mask), maxImgWidth, loadAndStoreSegments)

    def add_images(self, entries, maxImgWidth=1920, loadAndStoreSegments=True):
        """l3d_line3d_add_images: many images in one call -- exactly the add_image_pixels[_fixed_sim] / add_image_jpeg[_fixed_sim] calls in entry order,
        with the detector run once over all entries whose cache does not stand in for them.  An entry is a dict with the single calls' argument
        names: imageID, K, R, t; img (a uint8 array) or data (the bytes of a baseline JPEG file); worldpointIDs or viewSimilarity ({view id:
        similarity}); optionally dist = (k1, k2) or lens = capi.lens(...) (l3d_line3d_add_images_lens).  Returns the list of statuses, one per entry: 0, or the code the single call would have failed
        with (the causes: l3d_line3d_last_error, one line per failed entry).  A malformed entry raises before anything is added.
        The img of every entry may be a device object instead (l3d_line3d_add_device_images); a list that mixes device objects with host
        images or files raises ValueError before any call."""
        entries = list(entries)
        on_device = _entries_on_device(entries, "add_images")
        arr, keep = (device_entries if on_device else image_entries)(entries)
        n = len(entries)
        status = (C.c_int * max(1, n))()
        lens_arr, lens_keep = capi.lens_pointers([en.get("lens") for en in entries], n)
        remap_arr, remap_keep = capi.remap_pointers(*([en.get(k) for en in entries] for k in ("lens", "out_size", "mask", "border_mask")), n)
        tail = (C.c_int(n), C.c_char_p(self.data_directory.encode()), C.c_int(int(maxImgWidth)), C.c_int(int(loadAndStoreSegments)), status)
        if remap_arr is not None:
            call = self.lib.l3d_line3d_add_device_images_remap if on_device else self.lib.l3d_line3d_add_images_remap
            self._chk(call(self.h, arr, remap_arr, *tail))
        elif lens_arr is not None:
            call = self.lib.l3d_line3d_add_device_images_lens if on_device else self.lib.l3d_line3d_add_images_lens
            self._chk(call(self.h, arr, lens_arr, *tail))
        else:
            call = self.lib.l3d_line3d_add_device_images if on_device else self.lib.l3d_line3d_add_images
            self._chk(call(self.h, arr, *tail))
        return [int(status[i]) for i in range(n)]

    def decode_jpeg(self, data, device=False):
        """l3d_line3d_decode_jpeg: Context.decode_jpeg with the object's device (a node object: rank 0's); device=True: a torch uint8 tensor there"""
        w, h, ch = capi.jpeg_info(data)
        ptr, n = capi._bytes_arguments(data)
        if device:
            import torch
            out = torch.zeros((h, w) if ch == 1 else (h, w, ch), dtype=torch.uint8, device="cuda:%d" % self._device)
            o = capi.device_image(out)
            self._chk(self.lib.l3d_line3d_decode_jpeg_device(self.h, ptr, n, C.byref(o)))
            return out
        out = np.zeros((h, w) if ch == 1 else (h, w, ch), np.uint8)
        self._chk(self.lib.l3d_line3d_decode_jpeg(self.h, ptr, n, _p(out), C.c_size_t(w * ch)))
        return out

    def compute3Dmodel(self, perform_diffusion: bool = False):
        self._chk(self.lib.l3d_line3d_compute3Dmodel(self.h, C.c_int(int(perform_diffusion))))

    def getResult(self):
        """list of (segments2D [(camID, segID)...], segments3D [(P1, P2)...]) -- L3DFinalLine3D (commons.h:215-238)."""
        nl, n3, n2 = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.lib.l3d_line3d_result_sizes(self.h, C.byref(nl), C.byref(n3), C.byref(n2)))
        l3 = np.zeros(nl.value, np.int32)
        l2 = np.zeros(nl.value, np.int32)
        s3 = np.zeros((n3.value, 6), np.float64)
        s2 = np.zeros((n2.value, 2), np.uint32)
        if nl.value:
            self._chk(self.lib.l3d_line3d_get_result(self.h, _p(l3), _p(l2), _p(s3), _p(s2)))
        out, a, b = [], 0, 0
        for k in range(nl.value):
            seg3 = [(s3[a + i, :3].copy(), s3[a + i, 3:].copy()) for i in range(l3[k])]
            seg2 = [(int(s2[b + i, 0]), int(s2[b + i, 1])) for i in range(l2[k])]
            a += l3[k]
            b += l2[k]
            out.append((seg2, seg3))
        return out

    def project_result(self, view_ids=None, cameras=None, select="all", near=1e-6, margin=0.0):
        """l3d_line3d_project_result: the result's 3-D segments (getResult's order) projected into views ("PROJECTION AND OVERLAYS", 3) ->
        (seg2d (k, 4) float32, seg_index (k,) int32 into the flat list of getResult's 3-D segments, line_index (k,) int32, flags (k,) uint8,
        cam_start (m + 1,) int64), camera-major.  cameras None: each view's own camera as it was added (view_ids needed); else a list of
        (K, R, t, width, height), and view_ids may be None.  select "observed": only lines with a 2-D member in the view (needs view_ids)."""
        ids = None if view_ids is None else np.ascontiguousarray(view_ids, np.uint32).reshape(-1)
        cams = None if cameras is None else capi.cameras(cameras)
        m = len(ids) if ids is not None else (getattr(cams, "_n", len(cams)) if cams is not None else 0)
        if ids is not None and cams is not None and getattr(cams, "_n", len(cams)) != m:
            raise ValueError("project_result: one camera per view id")
        sel = {"all": capi.SELECT_ALL, "observed": capi.SELECT_OBSERVED}[select.lower()] if isinstance(select, str) else int(select)
        seg2d, si, li, fl = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_ubyte)()
        start = np.zeros(m + 1, np.int64)
        self._chk(self.lib.l3d_line3d_project_result(self.h, None if ids is None or not len(ids) else _p(ids), C.c_int(m), cams if cams is not None and m else None, C.c_int(sel),
                                                     C.c_double(near), C.c_double(margin), C.byref(seg2d), C.byref(si), C.byref(li), C.byref(fl), _p(start)))
        k = int(start[-1])
        out = (np.ctypeslib.as_array(seg2d, (k * 4,)).copy().reshape(-1, 4) if k else np.zeros((0, 4), np.float32),
               np.ctypeslib.as_array(si, (k,)).copy() if k else np.zeros(0, np.int32), np.ctypeslib.as_array(li, (k,)).copy() if k else np.zeros(0, np.int32),
               np.ctypeslib.as_array(fl, (k,)).copy() if k else np.zeros(0, np.uint8), start)
        for p in (seg2d, si, li, fl):
            self.lib.l3d_free(p)
        return out

    def overlay(self, view_id, image, layers=("members", "model"), select="observed", by_line=True, style=None, layout=None, chan=None, **kw):
        """l3d_line3d_overlay: the view's member segments and the projected result drawn over an image of the view's size ("PROJECTION AND
        OVERLAYS", 3).  A numpy image gives a NEW array; a device object (a uint8 device tensor or a capi.device_image descriptor; layout, chan
        as capi.device_image takes them) is drawn in place and returned.  style: a capi.overlay_style(...), or its keywords (opacity=,
        width_members=, width_model=, near=, color_members=, color_model=, palette=) beside layers, select and by_line."""
        st = style if style is not None else capi.overlay_style(layers=layers, select=select, by_line=by_line, **kw)
        if capi.is_device_object(image):
            d = capi.device_image(image, layout=layout, chan=chan)
            self._chk(self.lib.l3d_line3d_overlay_device(self.h, C.c_uint32(view_id), C.byref(d), C.byref(st)))
            return image
        out = capi._draw_image_copy(image)
        ptr, w, h, ch, stride = capi.image_arguments(out)
        self._chk(self.lib.l3d_line3d_overlay(self.h, C.c_uint32(view_id), ptr, C.c_int(w), C.c_int(h), C.c_int(ch), C.c_size_t(stride), C.byref(st)))
        return out

    def getSegment2D(self, camID, segID):
        o = (C.c_float * 4)()
        self.lib.l3d_line3d_get_segment2D(self.h, C.c_uint32(camID), C.c_uint32(segID), o)
        return tuple(o)

    # line3D.h:91-95 -- result writers (formats: line3D.cc:384-473, README.txt:177-185)
    def save3DLinesAsSTL(self, filename: str):
        self._chk(self.lib.l3d_line3d_save_result(self.h, filename.encode(), C.c_int(0)))

    def save3DLinesAsTXT(self, filename: str):
        self._chk(self.lib.l3d_line3d_save_result(self.h, filename.encode(), C.c_int(1)))

    # -- refinement of the result against the clusters' 2-D segments (no counterpart in the reference) --------------------
    def set_refinement(self, on=True, max_iterations=20, huber_px=2.0):
        """l3d_line3d_set_refinement: with it on, finish / compute3Dmodel refine every line of the result (Levenberg-Marquardt on the members' 2-D end
        points, Huber loss of scale huber_px, 0 = least squares) and replace its 3-D segments by collinear ones; off by default; reset keeps it."""
        self._chk(self.lib.l3d_line3d_set_refinement(self.h, C.c_int(int(bool(on))), C.c_int(int(max_iterations)), C.c_double(float(huber_px))))

    def refinement(self):
        """l3d_line3d_get_refinement: dict of rms_before, rms_after (pixels), iterations, status -- one entry per line of getResult().  status 0 refined,
        1 starting line (no trial lowered the cost), 2 degenerate, 3 the refined sweep emitted nothing: unrefined segments kept."""
        nl = C.c_int(0)
        self._chk(self.lib.l3d_line3d_result_sizes(self.h, C.byref(nl), None, None))
        n = nl.value
        rb, ra, it, st = np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._chk(self.lib.l3d_line3d_get_refinement(self.h, _p(rb), _p(ra), _p(it), _p(st)))
        return {"rms_before": rb, "rms_after": ra, "iterations": it, "status": st}

    # -- merging of the result's duplicate lines (no counterpart in the reference) -------------------------------------------
    def set_merging(self, on=True, dist_px=4.0, angle_deg=5.0, max_gap=0.0, max_rounds=3):
        """l3d_line3d_set_merging: with it on, finish / compute3Dmodel group the near-copies of a 3-D line on the device (capi.Context.merge_lines: ends
        within dist_px pixel footprints of the longer line's axis, directions within angle_deg, a gap of at most max_gap times the shorter length),
        refit every group from all of its 2-D segments and repeat, max_rounds times at the most, before the refinement; off by default; reset keeps it."""
        self._chk(self.lib.l3d_line3d_set_merging(self.h, C.c_int(int(bool(on))), C.c_double(float(dist_px)), C.c_double(float(angle_deg)), C.c_double(float(max_gap)),
                                                  C.c_int(int(max_rounds))))

    def merging(self):
        """l3d_line3d_get_merging: dict of lines_before, lines_after, rounds, pairs_first_round, groups_merged, lines_released, empty_refits, final_index
        (one per line before merging: its index in getResult()) and n_sources (one per line of getResult())."""
        cnt = np.zeros(8, np.int32)
        self._chk(self.lib.l3d_line3d_get_merging(self.h, _p(cnt), None, None))
        fi, ns = np.zeros(max(1, int(cnt[0])), np.int32), np.zeros(max(1, int(cnt[1])), np.int32)
        self._chk(self.lib.l3d_line3d_get_merging(self.h, _p(cnt), _p(fi), _p(ns)))
        keys = ("lines_before", "lines_after", "rounds", "pairs_first_round", "groups_merged", "lines_released", "empty_refits")
        out = {k: int(cnt[i]) for i, k in enumerate(keys)}
        out["final_index"], out["n_sources"] = fi[:int(cnt[0])].copy(), ns[:int(cnt[1])].copy()
        return out

    # -- support of the result's lines over all views (no counterpart in the reference) ----------------------------------------------
    def gather_support(self, params=None, **kw):
        """l3d_line3d_gather_support: which 2-D segments of which views lie on each line of the current result ("SUPPORT OF 3-D LINES", on the
        object).  params: a capi.support_params(...), or its keywords (dist_px=, cos_min= or angle_deg=, min_overlap=, near_z=, margin=); neither: 3 px,
        5 degrees, overlap 0.5, near 1e-6, margin 3 -> dict(records: capi.LINE_SUPPORT array (view_id, seg, seg3d into the flat list of getResult's 3-D
        segments, dist, overlap, flags: 1 member of this line, 2 member of another line, 4 this line holds the segment's best row), ordered by (line,
        view id, segment); line_start (lines + 1,) int64; line_views (lines, 2) int32: views with a member, views with a record; counts (4,) int64:
        records, members found again, members not found, segments on a line that are members of none)."""
        prm = params if params is not None else (capi.support_params(**kw) if kw else None)
        nl = C.c_int(0)
        self._chk(self.lib.l3d_line3d_result_sizes(self.h, C.byref(nl), None, None))
        n = nl.value
        rec = C.POINTER(capi.LineSupport)()
        start, views, counts = np.zeros(n + 1, np.int64), np.zeros((max(1, n), 2), np.int32), np.zeros(4, np.int64)
        self._chk(self.lib.l3d_line3d_gather_support(self.h, None if prm is None else C.byref(prm), C.byref(rec), _p(start), _p(views), _p(counts)))
        k = int(counts[0])
        records = np.frombuffer(C.string_at(rec, k * 24), capi.LINE_SUPPORT).copy() if k else np.zeros(0, capi.LINE_SUPPORT)
        self.lib.l3d_free(rec)
        return {"records": records, "line_start": start, "line_views": views[:n].copy(), "counts": counts}

    def set_support(self, on=True, dist_px=3.0, angle_deg=5.0, min_overlap=0.5):
        """l3d_line3d_set_support: with it on, finish / compute3Dmodel end with gather_support (after the line fit, the merging and the refinement) and
        extend every line's 2-D segments by the segments of all views for which it holds the best row and that are members of no line, behind the old
        members in (view id, segment) order; the 3-D segments are untouched; off by default; reset keeps it."""
        self._chk(self.lib.l3d_line3d_set_support(self.h, C.c_int(int(bool(on))), C.c_double(float(dist_px)), C.c_double(float(angle_deg)), C.c_double(float(min_overlap))))

    def support(self):
        """l3d_line3d_get_support: what the last finish with the support on recorded -- dict of records, members_found, members_not_found,
        segments_unclaimed (gather_support's counts, before the lists were extended) and, one per line of getResult(), members_before, members_added,
        views_before, views_after."""
        nl = C.c_int(0)
        self._chk(self.lib.l3d_line3d_result_sizes(self.h, C.byref(nl), None, None))
        n = nl.value
        cnt, per = np.zeros(4, np.int64), np.zeros((max(1, n), 4), np.int32)
        self._chk(self.lib.l3d_line3d_get_support(self.h, _p(cnt), _p(per)))
        out = {k: int(cnt[i]) for i, k in enumerate(("records", "members_found", "members_not_found", "segments_unclaimed"))}
        for i, k in enumerate(("members_before", "members_added", "views_before", "views_after")):
            out[k] = per[:n, i].copy()
        return out

    # -- junctions of the result's lines: a wireframe (no counterpart in the reference) --------------------------------------------
    def set_junctions(self, on=True, dist_px=4.0, ext_px=12.0, angle_min_deg=10.0, max_ext_rel=0.25, snap=False):
        """l3d_line3d_set_junctions: with it on, finish / compute3Dmodel find where the lines of the result meet (capi.Context.junction_lines: axes that
        pass within dist_px pixel footprints of each other, at least angle_min_deg apart, each line prolonged by at most ext_px footprints and
        max_ext_rel of its length), after the merging and the refinement and before the support gather.  snap: the ends that stay in a vertex or rest
        on another line move there along their own axes; off by default; reset keeps it."""
        self._chk(self.lib.l3d_line3d_set_junctions(self.h, C.c_int(int(bool(on))), C.c_double(float(dist_px)), C.c_double(float(ext_px)), C.c_double(float(angle_min_deg)),
                                                    C.c_double(float(max_ext_rel)), C.c_int(int(bool(snap)))))

    def junctions(self):
        """l3d_line3d_get_junctions: what the last finish with the junctions on recorded -- dict of vertices (capi.JUNCTION_VERTEX array: X, first_node,
        degree), per line of getResult() vertex_P, vertex_Q (the vertex an end stays in, or -1) and attach_line_P, attach_line_Q (the line an end rests
        on, or -1), and the counts: eligible_lines, l_records, t_records, x_records, components, vertices_found, nodes_released, nodes_attached, ends_moved,
        moves_skipped."""
        nl = C.c_int(0)
        self._chk(self.lib.l3d_line3d_result_sizes(self.h, C.byref(nl), None, None))
        n = nl.value
        vert, nv = C.POINTER(capi.JunctionVertex)(), C.c_int(0)
        per, cnt = np.zeros((max(1, n), 4), np.int32), np.zeros(10, np.int32)
        self._chk(self.lib.l3d_line3d_get_junctions(self.h, C.byref(vert), C.byref(nv), _p(per), _p(cnt)))
        vertices = np.frombuffer(C.string_at(vert, nv.value * 32), capi.JUNCTION_VERTEX).copy() if nv.value else np.zeros(0, capi.JUNCTION_VERTEX)
        self.lib.l3d_free(vert)
        out = {"vertices": vertices}
        for i, k in enumerate(("vertex_P", "vertex_Q", "attach_line_P", "attach_line_Q")):
            out[k] = per[:n, i].copy()
        for i, k in enumerate(("eligible_lines", "l_records", "t_records", "x_records", "components", "vertices_found", "nodes_released", "nodes_attached", "ends_moved",
                               "moves_skipped")):
            out[k] = int(cnt[i])
        return out

    def save3DLinesAsOBJ(self, filename):
        """l3d_line3d_save_wireframe: the result as a Wavefront OBJ wireframe -- the vertices of the last finish's junctions, then every line as a group of
        its own; an end that stays in a vertex uses the shared index; coordinates as %.17g.  Works without the junctions too (no shared vertices)."""
        self._chk(self.lib.l3d_line3d_save_wireframe(self.h, str(filename).encode()))

    # -- planes of the result's lines: faces for the wireframe (no counterpart in the reference) ------------------------------------
    def set_planes(self, on=True, dist_px=4.0, angle_deg=10.0, min_lines=3):
        """l3d_line3d_set_planes: with it on, finish / compute3Dmodel find which lines of the result lie in one plane (capi.Context.plane_lines: every
        pair of lines that meet spans a hypothesis, hypotheses within angle_deg whose lines lie within dist_px pixel footprints of each other's planes
        are grouped, a plane needs min_lines member lines), after the junctions -- whose search runs for the seeds even when that option is off -- and
        before the support gather.  Off by default; reset keeps it."""
        self._chk(self.lib.l3d_line3d_set_planes(self.h, C.c_int(int(bool(on))), C.c_double(float(dist_px)), C.c_double(float(angle_deg)), C.c_int(int(min_lines))))

    def planes(self):
        """l3d_line3d_get_planes: what the last finish with the planes on recorded -- dict of planes (capi.PLANE array: N, c, u, v, rect, rep, first_hyp,
        n_hyp, n_lines), members (capi.PLANE_MEMBER array ascending by (plane, line)), planes_per_line (per line of getResult() the number of planes it
        lies in), and the counts: eligible_lines, eligible_hypotheses, hypothesis_edges, components, hypotheses_released, candidates_dropped,
        planes_found, member_records."""
        nl = C.c_int(0)
        self._chk(self.lib.l3d_line3d_result_sizes(self.h, C.byref(nl), None, None))
        n = nl.value
        pl, mem, npl, nm = C.POINTER(capi.Plane)(), C.POINTER(capi.PlaneMember)(), C.c_int(0), C.c_int(0)
        per, cnt = np.zeros(max(1, n), np.int32), np.zeros(8, np.int32)
        self._chk(self.lib.l3d_line3d_get_planes(self.h, C.byref(pl), C.byref(npl), C.byref(mem), C.byref(nm), _p(per), _p(cnt)))
        out = {"planes": np.frombuffer(C.string_at(pl, npl.value * 128), capi.PLANE).copy() if npl.value else np.zeros(0, capi.PLANE),
               "members": np.frombuffer(C.string_at(mem, nm.value * 16), capi.PLANE_MEMBER).copy() if nm.value else np.zeros(0, capi.PLANE_MEMBER),
               "planes_per_line": per[:n].copy()}
        self.lib.l3d_free(pl)
        self.lib.l3d_free(mem)
        for i, k in enumerate(("eligible_lines", "eligible_hypotheses", "hypothesis_edges", "components", "hypotheses_released", "candidates_dropped", "planes_found",
                               "member_records")):
            out[k] = int(cnt[i])
        return out

    def save3DPlanesAsOBJ(self, filename):
        """l3d_line3d_save_planes: the planes of the last finish as a Wavefront OBJ -- per plane a group of the four corners of its rectangle and one face;
        coordinates as %.17g."""
        self._chk(self.lib.l3d_line3d_save_planes(self.h, str(filename).encode()))

    def refinement_input(self):
        """l3d_line3d_refinement_input (inspection): what a refinement of the current result is fed with -- dict of group_start, member_cam, member_seg,
        member_pts, cameras (normalised frame) and Rinv (3, 3), scale_inv, tneg (3,) of Line3D::inverseTransform."""
        cnt = np.zeros(3, np.int32)
        self._chk(self.lib.l3d_line3d_refinement_input(self.h, _p(cnt), None, None, None, None, None, None))
        nl, nm, nv = (int(x) for x in cnt)
        gs, mc, ms, mp = np.zeros(nl + 1, np.int32), np.zeros(nm, np.int32), np.zeros((nm, 4), np.float32), np.zeros((nm, 6))
        cams, tr = np.zeros((nv, 3, 4)), np.zeros(13)
        self._chk(self.lib.l3d_line3d_refinement_input(self.h, _p(cnt), _p(gs), _p(mc), _p(ms), _p(mp), _p(cams), _p(tr)))
        return {"group_start": gs, "member_cam": mc, "member_seg": ms, "member_pts": mp, "cameras": cams, "Rinv": tr[:9].reshape(3, 3).copy(), "scale_inv": float(tr[9]),
                "tneg": tr[10:13].copy()}

    # -- co-visibility: where the world point links are filed, and what prepare() chose from them -----------------------
    def set_covisibility(self, mode="device"):
        """l3d_line3d_set_covisibility: "host" (default) files a view's world point links as it is added; "device" stores the list and has prepare()
        count all lists on the GPU.  Refused while the object holds views; reset keeps the setting."""
        m = {"host": 0, "device": 1}.get(mode, mode)
        if m not in (0, 1):
            raise ValueError('set_covisibility: "host" or "device"')
        self._chk(self.lib.l3d_line3d_set_covisibility(self.h, C.c_int(int(m))))

    def covisibility_path(self):
        """l3d_line3d_covisibility_path: 0 the closed form on the device, 1 the host replay (a list named an id twice) -- of the last count"""
        return int(self.lib.l3d_line3d_covisibility_path(self.h))

    def neighbors(self, view_id):
        """l3d_line3d_get_neighbors: the view's visual neighbours after prepare, ascending ids (uint32)"""
        n = C.c_int(0)
        self._chk(self.lib.l3d_line3d_get_neighbors(self.h, C.c_uint32(view_id), None, C.c_int(0), C.byref(n)))
        ids = np.zeros(n.value, np.uint32)
        self._chk(self.lib.l3d_line3d_get_neighbors(self.h, C.c_uint32(view_id), _p(ids), C.c_int(len(ids)), C.byref(n)))
        return ids

    def view_similarities(self, view_id):
        """l3d_line3d_get_view_similarities: (ids uint32, similarities float32) of the view after prepare, ascending by the other view's id"""
        n = C.c_int(0)
        self._chk(self.lib.l3d_line3d_get_view_similarities(self.h, C.c_uint32(view_id), None, None, C.c_int(0), C.byref(n)))
        ids, sims = np.zeros(n.value, np.uint32), np.zeros(n.value, np.float32)
        self._chk(self.lib.l3d_line3d_get_view_similarities(self.h, C.c_uint32(view_id), _p(ids), _p(sims), C.c_int(len(ids)), C.byref(n)))
        return ids, sims

    def numCameras(self):
        return self.lib.l3d_line3d_num_cameras(self.h)

    def reset(self):
        self._chk(self.lib.l3d_line3d_reset(self.h))

    # -- stages ----------------------------------------------------------------------------------
    def prepare(self):
        self._chk(self.lib.l3d_line3d_prepare(self.h))

    def match_views(self):
        self._chk(self.lib.l3d_line3d_match_views(self.h))

    def finish(self, perform_diffusion=False):
        self._chk(self.lib.l3d_line3d_finish(self.h, C.c_int(int(perform_diffusion))))

    def match_begin(self):
        n = C.c_int(0)
        self._chk(self.lib.l3d_line3d_match_begin(self.h, C.byref(n)))
        ids = np.zeros(n.value, np.uint32)
        ns = np.zeros(n.value, np.int32)
        self._chk(self.lib.l3d_line3d_match_order(self.h, _p(ids), _p(ns)))
        return ids, ns

    def view_num_to_be_matched(self, view_id):
        return self.lib.l3d_line3d_view_num_to_be_matched(self.h, C.c_uint32(view_id))

    def match_view_compute(self, view_id, seg_begin, seg_end):
        out = C.c_void_p()
        n = C.c_int(0)
        med = C.c_float(1.0)
        bd = C.POINTER(C.c_float)()
        nb = C.c_int(0)
        self._chk(self.lib.l3d_line3d_match_view_compute(self.h, C.c_uint32(view_id), C.c_int(seg_begin), C.c_int(seg_end),
                                                         C.byref(out), C.byref(n), C.byref(med), C.byref(bd), C.byref(nb)))
        res = np.zeros(n.value, dtype=MATCH_DTYPE)
        if n.value:
            C.memmove(res.ctypes.data, out, n.value * 32)
        self.lib.l3d_free(out)
        best = np.ctypeslib.as_array(bd, (nb.value * 2,)).copy() if nb.value else np.zeros(0, np.float32)
        if bd:
            self.lib.l3d_free(bd)
        return res, med.value, best

    def match_view_commit(self, view_id, matches, best_depths=None, median=1.0):
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        if best_depths is None:
            self._chk(self.lib.l3d_line3d_match_view_commit(self.h, C.c_uint32(view_id), _p(m), C.c_int(len(m)), None,
                                                            C.c_int(-1), C.c_float(median)))
        else:
            b = np.ascontiguousarray(best_depths, dtype=np.float32)
            self._chk(self.lib.l3d_line3d_match_view_commit(self.h, C.c_uint32(view_id), _p(m), C.c_int(len(m)), _p(b),
                                                            C.c_int(len(b) // 2), C.c_float(median)))

    # -- resident chain sharded over ranks (line3d_amd/distributed.py drives it) -------------------
    def stream_ptr(self) -> int:
        self.lib.l3d_ctx_stream.restype = C.c_void_p
        self.lib.l3d_ctx_stream.argtypes = [C.c_void_p]
        return int(self.lib.l3d_ctx_stream(C.c_void_p(self.lib.l3d_line3d_context(self.h))) or 0)

    def shard_open(self, rank: int, world: int, slot_records: int):
        n = C.c_int(0)
        sb = C.c_size_t(0)
        self._chk(self.lib.l3d_line3d_shard_open(self.h, C.c_int(rank), C.c_int(world), C.c_int(slot_records), C.byref(n), C.byref(sb)))
        return n.value, sb.value

    def shard_view_verified(self, k: int) -> bool:
        return self.lib.l3d_line3d_shard_view_verified(self.h, C.c_int(k)) == 1

    def shard_enqueue(self, k: int, send_slot_ptr: int, gathered_ptr: int):
        self._chk(self.lib.l3d_line3d_shard_enqueue(self.h, C.c_int(k), C.c_void_p(send_slot_ptr), C.c_void_p(gathered_ptr)))

    def shard_mark(self, k: int):
        self._chk(self.lib.l3d_line3d_shard_mark(self.h, C.c_int(k)))

    def shard_fetch(self, k: int):
        self._chk(self.lib.l3d_line3d_shard_fetch(self.h, C.c_int(k)))

    def shard_run(self, rank: int, world: int, slot_records: int, exchange: str = "local", exchange_user=None, commit: bool = True):
        """The whole sharded chain as one native call (l3d_shard_chain_run).  exchange: "rccl" (exchange_user = a ctypes
        l3d_rccl_link), "local" (world 1), "replay" (exchange_user = device address of recorded gathered blocks) or "node" (exchange_user =
        capi.NodeComm.h of the ranks of this process, this object's stream bound to its rank).
        commit: False / 0 = compute and exchange only, True / 1 = host bookkeeping on this rank, 2 (or "device") = matchViews' products built on
        this rank's device from the gathered slots, 3 (or "partition") = as 2, but this rank keeps the records and builds the rows of its block of
        views only (l3d_shard_chain_partition: exact without speculation; finish_sharded() follows on every rank).
        Returns (device address of the gathered blocks, slot_bytes)."""
        if commit == "device":
            commit = 2
        if commit == "partition":
            commit = 3
        if callable(exchange):       # tests: a Python exchange (called on this thread by the enqueue loop), e.g. to inject a failure
            proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
            fn = self._exchange_keepalive = proto(exchange)
        else:
            fn = {"rccl": self.lib.l3d_exchange_rccl, "local": self.lib.l3d_exchange_local, "replay": self.lib.l3d_exchange_replay,
                  "node": self.lib.l3d_exchange_node}[exchange]
        user = C.c_void_p(exchange_user) if isinstance(exchange_user, int) else (C.c_void_p(C.addressof(exchange_user)) if exchange_user is not None else None)
        g = C.c_void_p(0)
        sb = C.c_size_t(0)
        self._chk(self.lib.l3d_line3d_shard_run(self.h, C.c_int(rank), C.c_int(world), C.c_int(slot_records), C.cast(fn, C.c_void_p), user,
                                                C.c_int(int(commit)), C.byref(g), C.byref(sb)))
        return g.value, sb.value

    def block_run(self, rank: int, world: int, exchange="local", exchange_user=None, warmup_views: int = -1) -> bool:
        """matchViews with the views sharded over the ranks in blocks (l3d_line3d_block_run): True = the speculation was exact and this object
        holds matchViews' products; False = it was not (same answer on every rank): run shard_run instead.  exchange as for shard_run."""
        if callable(exchange):
            proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
            fn = self._exchange_keepalive = proto(exchange)
        else:
            fn = {"rccl": self.lib.l3d_exchange_rccl, "local": self.lib.l3d_exchange_local, "node": self.lib.l3d_exchange_node}[exchange]
        user = C.c_void_p(exchange_user) if isinstance(exchange_user, int) else (C.c_void_p(C.addressof(exchange_user)) if exchange_user is not None else None)
        verdict = C.c_int(1)
        self._chk(self.lib.l3d_line3d_block_run(self.h, C.c_int(rank), C.c_int(world), C.c_int(warmup_views), C.cast(fn, C.c_void_p), user, C.byref(verdict)))
        return verdict.value == 0

    def partition_run(self, rank: int, world: int, exchange="local", exchange_user=None, warmup_views: int = -1) -> bool:
        """matchViews sharded by blocks of views with nothing replicated (l3d_line3d_partition_run): this object then holds its block's share of the
        kept records and of matchViews' products; finish_sharded() -- on every rank -- completes compute3Dmodel.  exchange as for block_run."""
        if callable(exchange):
            proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
            fn = self._exchange_keepalive = proto(exchange)
        else:
            fn = {"rccl": self.lib.l3d_exchange_rccl, "local": self.lib.l3d_exchange_local, "node": self.lib.l3d_exchange_node}[exchange]
        user = C.c_void_p(exchange_user) if isinstance(exchange_user, int) else (C.c_void_p(C.addressof(exchange_user)) if exchange_user is not None else None)
        verdict = C.c_int(1)
        self._chk(self.lib.l3d_line3d_partition_run(self.h, C.c_int(rank), C.c_int(world), C.c_int(warmup_views), C.cast(fn, C.c_void_p), user, C.byref(verdict)))
        return verdict.value == 0

    def finish_sharded(self, perform_diffusion=False):
        """the rest of compute3Dmodel after partition_run, on every rank (collective; the exchange of the run)"""
        self._chk(self.lib.l3d_line3d_finish_sharded(self.h, C.c_int(int(perform_diffusion)), None, None))

    def partition_info(self):
        """what this rank's share covers (views of the dense map): dict(rank, world, own, rows, held, n_pot_all, recovery_rounds, blocks_rerun)"""
        info = (C.c_int * 10)()
        npot = C.c_int64(0)
        self._chk(self.lib.l3d_partition_info(C.c_void_p(self.lib.l3d_line3d_context(self.h)), info, C.byref(npot)))
        return dict(rank=info[0], world=info[1], own=(info[2], info[3]), rows=(info[4], info[5]), held=(info[6], info[7]), n_pot_all=npot.value, recovery_rounds=info[8],
                    blocks_rerun=info[9])

    def shard_close(self, committed: bool):
        self._chk(self.lib.l3d_line3d_shard_close(self.h, C.c_int(int(committed))))

    def match_end(self):
        self._chk(self.lib.l3d_line3d_match_end(self.h))

    # -- inspection ------------------------------------------------------------------------------
    def set_sync_matching(self, on=True):
        self._chk(self.lib.l3d_line3d_set_sync_matching(self.h, C.c_int(int(on))))

    def match_path(self) -> int:
        """l3d_line3d_match_path: 0 resident chain, 1 chain + host bookkeeping, 2 per-view seam calls on request, 3 per-view because the schedule is not static"""
        return int(self.lib.l3d_line3d_match_path(self.h))

    def keep_view_matches(self, on=True):
        self._chk(self.lib.l3d_line3d_keep_view_matches(self.h, C.c_int(int(on))))

    def view_matches(self, view_id):
        p = C.c_void_p()
        n = C.c_int(0)
        med = C.c_float(0)
        self._chk(self.lib.l3d_line3d_view_matches(self.h, C.c_uint32(view_id), C.byref(p), C.byref(n), C.byref(med)))
        res = np.zeros(n.value, dtype=MATCH_DTYPE)
        if n.value:
            C.memmove(res.ctypes.data, p, n.value * 32)
        return res, med.value

    def affinity(self):
        p = C.c_void_p()
        nnz, nn = C.c_int(0), C.c_int(0)
        self._chk(self.lib.l3d_line3d_affinity(self.h, C.byref(p), C.byref(nnz), C.byref(nn)))
        res = np.zeros(nnz.value, dtype=EDGE_DTYPE)
        if nnz.value:
            C.memmove(res.ctypes.data, p, nnz.value * 12)
        return res, nn.value

    def resident_products(self):
        """The device-resident products of the last match_views (and, after finish, the hypothesis table), copied to the host:
        None when matchViews ran with host bookkeeping.  dict(seg_base, pot_start, pot_tgt, best, hyp, score)."""
        nv, nd, nh = C.c_int(0), C.c_int(0), C.c_int(0)
        npot = C.c_int64(0)
        self._chk(self.lib.l3d_line3d_products_sizes(self.h, C.byref(nv), C.byref(nd), C.byref(npot), C.byref(nh)))
        if nv.value == 0:
            return None
        seg_base = np.zeros(nv.value + 1, np.int32)
        pot_start = np.zeros(nd.value + 1, np.int64)
        pot_tgt = np.zeros(max(1, npot.value), np.int32)
        best = np.zeros(nd.value, MATCH_DTYPE)
        hyp = np.zeros(max(1, nh.value), capi.HYP_DTYPE)
        score = np.zeros(max(1, nh.value), np.float32)
        self._chk(self.lib.l3d_line3d_products_get(self.h, _p(seg_base), _p(pot_start), _p(pot_tgt), _p(best), _p(hyp) if nh.value else None,
                                                   _p(score) if nh.value else None))
        return dict(seg_base=seg_base, pot_start=pot_start, pot_tgt=pot_tgt[:npot.value], best=best, hyp=hyp[:nh.value], score=score[:nh.value])

    def chain_summary(self):
        """Per chain view of the last match_views with resident products (the index of Context.chain_kept_list): structured array of
        (verified, n_kept, n_candidates, median_depth); empty without resident products"""
        p, n = C.c_void_p(), C.c_int(0)
        self._chk(self.lib.l3d_line3d_chain_summary(self.h, C.byref(p), C.byref(n)))
        out = np.zeros(n.value, dtype=SUMMARY_DTYPE)
        if n.value:
            C.memmove(out.ctypes.data, p, n.value * SUMMARY_DTYPE.itemsize)
        return out

    def stats(self):
        s = (C.c_double * 12)()
        self._chk(self.lib.l3d_line3d_stats(self.h, s))
        keys = ["pairs", "raw", "kept", "hypotheses", "t_match", "t_gpu_call", "t_commit", "t_finalize", "t_affinity",
                "t_cluster", "edges", "lines"]
        return dict(zip(keys, list(s)))


def load_scene(l3d: Line3D, scene):
    for v in scene.views:
        ok = l3d.addImage_fixed_sim(v["id"], v["width"], v["height"], v["segments"], v["K"], v["R"], v["t"], v["sims"])
        assert ok


def load_scene_worldpoints(l3d: Line3D, scene):
    """views that carry the world points they see (synth.make_scene_scattered): Line3D::addImage, neighbours chosen by the library"""
    for v in scene.views:
        ok = l3d.addImage(v["id"], v["width"], v["height"], v["segments"], v["K"], v["R"], v["t"], v["worldpoints"])
        assert ok
