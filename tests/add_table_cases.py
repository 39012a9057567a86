"""The add family's behaviour as a table: forms (the exported l3d_line3d_add_image* calls, l3d_line3d_add_images with one and with three entries)
by causes (added, the cache rules, every refusal, and coincidences of two causes that pin the order in which they are tested).  CASES is the list;
Runner replays a case on a Line3D object and returns what scripts/record_add_table.py stored in tests/golden/add_table.json and
tests/test_gpu_add_table.py compares: return code, message, number of cameras, the data directory's listing, a batch's status list.

A case: name, c (the content, below), setup (steps before the call), las (load_and_store), via (how the content is handed over), causes (tags of
CAUSES it stands for), and optionally prepare (fill up to four views and run prepare(): the listing then shows which caches were to be written),
maxw (max_img_width) and node (a node object of two ranks on one device).
Content: src = pixels | jpeg | both | neither (an image entry), segs | segs_ex | size_ex | cached (the segment-taking calls); img = view | flat |
w0 | null0 (a null pointer, 0 x 0, three channels: a default-constructed image); bytes = view | progressive | four | hollow (headers intact, the
entropy-coded data zeroed) | null (no bytes at all); links = wps | sims; n_links = 0; dist (key present: the _distorted call; None: a null
pointer); null = K | R | t; skew.  The subject is view 2 of the six-view scene; views 0 and 1 surround it in a batch of three; views 3 to 5 fill up."""
import ctypes as C
import os
import tempfile

import numpy as np

# the wiring scenes of tests/test_gpu_add_images.py, which are 320 x 200 (tests/golden/jpeg_ref.npz: view0..view5); the suite has no 64 x 48 scene that is
# known to yield segments, with and without DIST, from pixels and from its JPEG file.  Only the flat image, in which nothing is to be found, is 64 x 48
SCENE = dict(n_views=6, n_segments=30, n_neighbors=6, seed=11, noise_px=0.0, width=320, height=200, f=250.0, seg_len=(0.3, 0.8))
DIST = (-0.2, 0.03)
TINY = (1e-13, -1e-13)
WORLDPOINTS = list(range(10))
SUBJECT, BEFORE, AFTER, FILL = 2, 0, 1, (3, 4, 5)

ENTRY_POINTS = ["add_image", "add_image_fixed_sim", "add_image_cached", "add_image_ex", "add_image_fixed_sim_ex", "add_image_pixels",
                "add_image_pixels_fixed_sim", "add_image_pixels_distorted", "add_image_pixels_fixed_sim_distorted", "add_image_jpeg",
                "add_image_jpeg_fixed_sim", "add_images", "add_image_entry"]
CAUSES = ["added_store", "added_nostore", "cache_wanted", "cache_wanted_refused_jpeg", "cache_unwanted", "cache_truncated", "flat", "flat_stale", "dup",
          "zero_links_wps", "zero_links_sims", "width0", "computed", "null_K", "null_R", "null_t", "null_dist", "skew", "tiny_dist", "progressive",
          "four_byte", "both", "neither", "null_image", "hollow_jpeg", "progressive+cache", "dup+flat", "dup+refused_jpeg", "zero_links+skew",
          "width0+dup", "dup+cache_wanted", "node_added", "node_cache", "node_refused"]

CASES = []


def _case(name, c, causes, via=("named",), setup=(), las=0, **kw):
    CASES.append(dict(name=name, c=c, causes=tuple(causes), via=tuple(via), setup=tuple(setup), las=las, **kw))


P, PS = dict(src="pixels"), dict(src="pixels", links="sims")
J, JS = dict(src="jpeg"), dict(src="jpeg", links="sims")
PD, PSD = dict(P, dist=DIST), dict(PS, dist=DIST)
ALL3 = ("named", "batch1", "batch3")

# added, no cache
_case("added_store_pixels", P, ["added_store"], ALL3, las=1, prepare=True)
_case("added_store_pixels_sims", PS, ["added_store"], ("named", "batch1"), las=1)
_case("added_store_pixels_distorted", PD, ["added_store"], ("named", "batch1"), las=1)
_case("added_store_pixels_sims_distorted", PSD, ["added_store"], ("named",), las=1)
_case("added_store_jpeg", J, ["added_store"], ("named", "batch1"), las=1)
_case("added_store_jpeg_sims_distorted", dict(JS, dist=DIST), ["added_store"], ALL3, las=1, prepare=True)
_case("added_store_scaled", P, ["added_store"], ("named", "batch1"), las=1, prepare=True, maxw=160)
_case("added_nostore_pixels", P, ["added_nostore"], ALL3)
_case("added_nostore_jpeg", J, ["added_nostore"], ("named",))
_case("added_segs", dict(src="segs"), ["added_nostore"])
_case("added_segs_sims", dict(src="segs", links="sims"), ["added_nostore"])
_case("added_cached", dict(src="cached"), ["added_nostore"])
_case("added_store_ex", dict(src="segs_ex"), ["added_store"], las=1, prepare=True)
_case("added_nostore_ex_sims", dict(src="segs_ex", links="sims"), ["added_nostore"])
_case("size_only_without_cache", dict(src="size_ex"), ["added_store"], las=1)
# the cache rules
_case("cache_wanted_pixels", P, ["cache_wanted"], ALL3, setup=["cache"], las=1)
_case("cache_wanted_hollow_jpeg", dict(J, bytes="hollow"), ["cache_wanted", "cache_wanted_refused_jpeg"], ALL3, setup=["cache"], las=1)
_case("cache_wanted_hollow_jpeg_sims_distorted", dict(JS, bytes="hollow", dist=DIST), ["cache_wanted_refused_jpeg"], ("named", "batch1"), setup=["cache"], las=1)
_case("hollow_jpeg_without_cache", dict(JS, bytes="hollow"), ["hollow_jpeg"], ("named", "batch1"), las=1)
_case("hollow_jpeg_cache_unwanted", dict(J, bytes="hollow"), ["hollow_jpeg", "cache_unwanted"], ("named", "batch1"), setup=["cache"])
_case("cache_wanted_refused_jpeg", dict(J, bytes="progressive"), ["progressive+cache"], ("named", "batch1"), setup=["cache"], las=1)
_case("cache_wanted_ex", dict(src="segs_ex"), ["cache_wanted"], setup=["cache"], las=1)
_case("cache_wanted_size_only_sims", dict(src="size_ex", links="sims"), ["cache_wanted"], setup=["cache"], las=1)
_case("cache_unwanted_pixels", P, ["cache_unwanted"], ("named", "batch1"), setup=["cache"])
_case("cache_unwanted_ex", dict(src="segs_ex"), ["cache_unwanted"], setup=["cache"])
_case("cache_truncated_pixels", P, ["cache_truncated"], ("named", "batch1"), setup=["cache_cut"], las=1)
_case("cache_truncated_jpeg_sims", JS, ["cache_truncated"], setup=["cache_cut"], las=1)
_case("cache_truncated_ex", dict(src="segs_ex"), ["cache_truncated"], setup=["cache_cut"], las=1)
_case("cache_truncated_unwanted", P, ["cache_truncated", "cache_unwanted"], setup=["cache_cut"])
# nothing detected
_case("flat", dict(P, img="flat"), ["flat"], ALL3)
_case("flat_store", dict(PS, img="flat"), ["flat"], ("named", "batch1"), las=1)
_case("flat_stale_cache", dict(P, img="flat"), ["flat_stale"], ("named", "batch1"), setup=["cache"])
_case("flat_wanted_cache", dict(P, img="flat"), ["flat", "cache_wanted"], setup=["cache"], las=1)
# the guards
_case("dup_pixels", P, ["dup"], ALL3, setup=["dup"])
_case("dup_segs", dict(src="segs"), ["dup"], setup=["dup"])
_case("dup_cached", dict(src="cached"), ["dup"], setup=["dup"])
_case("dup_ex", dict(src="segs_ex"), ["dup"], setup=["dup"])
_case("zero_wps_pixels", dict(P, n_links=0), ["zero_links_wps"], ("named", "batch1"))
_case("zero_sims_pixels", dict(PS, n_links=0), ["zero_links_sims"], ("named", "batch1"))
_case("zero_sims_jpeg", dict(JS, n_links=0), ["zero_links_sims"])
_case("zero_wps_segs", dict(src="segs", n_links=0), ["zero_links_wps"])
_case("zero_sims_segs", dict(src="segs", links="sims", n_links=0), ["zero_links_sims"])
_case("zero_wps_ex", dict(src="segs_ex", n_links=0), ["zero_links_wps"], setup=["cache"])
_case("zero_sims_ex", dict(src="segs_ex", links="sims", n_links=0), ["zero_links_sims"])
_case("zero_wps_cached", dict(src="cached", n_links=0), ["zero_links_wps"])
_case("width0_pixels", dict(P, img="w0"), ["width0"], ("named", "batch1"))
_case("width0_segs", dict(src="segs", img="w0"), ["width0"])
_case("width0_ex", dict(src="segs_ex", img="w0"), ["width0"])
_case("width0_cached", dict(src="cached", img="w0"), ["width0"])
_case("computed_pixels", P, ["computed"], ("named", "batch1"), setup=["computed"])
_case("computed_jpeg", J, ["computed"], setup=["computed"])
_case("computed_segs", dict(src="segs"), ["computed"], setup=["computed"])
_case("computed_ex", dict(src="segs_ex"), ["computed"], setup=["computed"])
_case("computed_cached", dict(src="cached"), ["computed"], setup=["computed"])
# null pointers, where the form admits one
_case("null_K_pixels", dict(P, null="K"), ["null_K"], ("named", "batch1"))
_case("null_K_pixels_distorted", dict(PD, null="K"), ["null_K"], ("named", "batch1"))
_case("null_dist_pixels_distorted", dict(P, dist=None), ["null_dist"])
_case("null_K_and_dist_pixels_distorted", dict(PS, dist=None, null="K"), ["null_K", "null_dist"])
_case("null_R_jpeg", dict(J, null="R"), ["null_R"], ("named", "batch1"))
_case("null_K_jpeg_distorted", dict(JS, dist=DIST, null="K"), ["null_K"])
_case("null_t_ex", dict(src="segs_ex", null="t"), ["null_t"])
_case("null_K_segs", dict(src="segs", null="K"), ["null_K"])
_case("null_R_cached", dict(src="cached", null="R"), ["null_R"])
_case("null_t_pixels_sims", dict(PS, null="t"), ["null_t"], ("named", "batch1"), las=1)
# the camera of the undistortion
_case("skew_pixels", dict(PD, skew=True), ["skew"], ("named", "batch1"))
_case("skew_jpeg", dict(J, dist=DIST, skew=True), ["skew"], ("named", "batch3"))
_case("tiny_dist_pixels", dict(P, dist=TINY), ["tiny_dist"], ("named", "batch1"))
_case("tiny_dist_skew_jpeg_sims", dict(JS, dist=TINY, skew=True), ["tiny_dist"])
# files the decoder refuses; entries that are no image
_case("progressive", dict(J, bytes="progressive"), ["progressive"], ALL3)
_case("progressive_sims", dict(JS, bytes="progressive"), ["progressive"])
_case("four_byte", dict(J, bytes="four"), ["four_byte"], ("named", "batch1"))
_case("both", dict(src="both"), ["both"], ("batch1", "batch3"))
_case("neither", dict(src="neither"), ["neither"], ("batch1", "batch3"))
# no image at all: a default-constructed image, no bytes
_case("null_pixels_empty", dict(P, img="null0"), ["null_image"], ("named", "batch1"))
_case("null_pixels_empty_sims_distorted", dict(PSD, img="null0"), ["null_image"], ("named",), setup=["dup"])
_case("null_bytes_jpeg", dict(J, bytes="null"), ["null_image"], ("named", "batch1"))
_case("null_bytes_jpeg_sims_distorted", dict(JS, bytes="null", dist=DIST), ["null_image"], ("named",), setup=["cache"], las=1)
# two causes at once: which one is reported pins the order
_case("dup_flat", dict(P, img="flat"), ["dup+flat"], ("named", "batch1"), setup=["dup"])
_case("dup_flat_stale_cache", dict(P, img="flat"), ["dup+flat", "flat_stale"], ("named", "batch1"), setup=["dup", "cache"])
_case("dup_refused_jpeg", dict(J, bytes="progressive"), ["dup+refused_jpeg"], ("named", "batch1"), setup=["dup"])
_case("zero_links_skew", dict(PD, skew=True, n_links=0), ["zero_links+skew"], ("named", "batch1"))
_case("width0_dup_pixels", dict(P, img="w0"), ["width0+dup"], ("named", "batch1"), setup=["dup"])
_case("width0_dup_ex", dict(src="segs_ex", img="w0"), ["width0+dup"], setup=["dup"])
_case("dup_cache_wanted_pixels", P, ["dup+cache_wanted"], ("named", "batch1"), setup=["dup", "cache"], las=1)
_case("dup_cache_wanted_ex", dict(src="segs_ex"), ["dup+cache_wanted"], setup=["dup", "cache"], las=1)
_case("dup_cache_unwanted_pixels", P, ["dup", "cache_unwanted"], setup=["dup", "cache"])
# a node object of two ranks on one device
_case("node_added_pixels", P, ["node_added"], ("named", "batch3"), las=1, prepare=True, node=True)
_case("node_added_ex_sims", dict(src="segs_ex", links="sims"), ["node_added"], las=1, prepare=True, node=True)
_case("node_cache_loaded_pixels", P, ["node_cache"], ("named", "batch1"), setup=["cache"], las=1, prepare=True, node=True)
_case("node_cache_loaded_hollow_jpeg_sims", dict(JS, bytes="hollow"), ["node_cache"], ("named", "batch3"), setup=["cache"], las=1, node=True)
_case("node_cache_jpeg", dict(J, bytes="progressive"), ["node_refused", "progressive+cache"], ("named", "batch1"), setup=["cache"], las=1, node=True)
_case("node_cache_unwanted", PS, ["node_added", "cache_unwanted"], setup=["cache"], node=True)
_case("node_refused_jpeg", dict(J, bytes="progressive"), ["node_refused"], ("named", "batch3"), node=True)
_case("node_refused_dup", PD, ["node_refused"], ("named", "batch1"), setup=["dup"], node=True)


def named_form(c):
    """the exported call (without its l3d_line3d_ prefix) that takes this content on its own; None: only an image entry can carry it"""
    s = "_fixed_sim" if c.get("links") == "sims" else ""
    return {"segs": "add_image" + s, "cached": "add_image_cached", "segs_ex": "add_image" + s + "_ex", "size_ex": "add_image" + s + "_ex",
            "pixels": "add_image_pixels" + s + ("_distorted" if "dist" in c else ""), "jpeg": "add_image_jpeg" + s}.get(c["src"])


def entry_expressible(c):
    """an l3d_image_entry says the same as the named call: an image, and not the _distorted call with a null dist (a null dist of an entry means none).
    (An entry with neither pixels nor a file is, in the single call, a null image of the kind its fields state: the null_image cases.)"""
    return c["src"] in ("pixels", "jpeg", "both") and not ("dist" in c and c["dist"] is None and c["src"] == "pixels")


def runs(case, with_entry):
    """the (case name, via) pairs of a case; with_entry: also through l3d_line3d_add_image_entry"""
    out = [(case["name"], v) for v in case["via"]]
    if with_entry and entry_expressible(case["c"]):
        out.append((case["name"], "entry"))
    return out


def entry_point_of(case, via):
    return {"named": named_form(case["c"]), "batch1": "add_images", "batch3": "add_images", "entry": "add_image_entry"}[via]


def expected_for_entry(case, table):
    """what l3d_line3d_add_image_entry has to give: the named call's record; where no named call takes the content, the one-entry batch's with the
    entry's status as the code and the message without its "image <id>: " prefix"""
    key = case["name"] + "/named"
    if key in table:
        return table[key]
    b = dict(table[case["name"] + "/batch1"])
    status = b.pop("status")
    b["rc"] = status[0]
    b["error"] = b["error"].split(": ", 1)[1] if b["error"] else ""
    return b


def check_properties(case, rec):
    """what a record has to show for the case to BE the cause it is tagged with (the tags alone would pass whatever the case does)"""
    causes, subject_ok = case["causes"], rec["rc"] == 0 and rec.get("status", [0])[len(rec.get("status", [0])) // 2] == 0
    if {"cache_wanted", "cache_wanted_refused_jpeg", "node_cache", "added_nostore", "node_added"} & set(causes) or (causes == ("added_store",) and case["c"]["src"] != "size_ex"):
        assert subject_ok and rec["cameras"] >= 1 and rec["error"] == "", (case["name"], rec)        # the view is there
    if {"cache_wanted", "cache_wanted_refused_jpeg", "node_cache", "progressive+cache", "dup+cache_wanted"} & set(causes):
        assert any(f.startswith("segments_2_") for f in rec["listing"]), (case["name"], rec)         # ... and the cache file untouched
    if {"cache_unwanted", "flat_stale"} & set(causes) and "dup" not in causes and "hollow_jpeg" not in causes:
        assert rec["listing"] == [], (case["name"], rec)                                              # the stale file is gone
    if {"dup", "zero_links_wps", "zero_links_sims", "width0", "computed", "skew", "progressive", "four_byte", "both", "neither", "null_image", "hollow_jpeg",
        "cache_truncated", "node_refused", "progressive+cache", "dup+refused_jpeg", "zero_links+skew", "width0+dup", "dup+cache_wanted"} & set(causes) \
            and "cache_unwanted" not in causes:
        assert not subject_ok and rec["error"], (case["name"], rec)                                  # refused, with a message
    if {"flat", "dup+flat"} & set(causes) and "cache_wanted" not in causes:
        assert subject_ok and rec["cameras"] == (1 if "dup" in case["setup"] else 2 if "status" in rec and len(rec["status"]) == 3 else 0), (case["name"], rec)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Runner:
    """replays cases on one ordinary and one node object (reset between cases), each case in a data directory of its own"""

    def __init__(self, golden_jpeg, base_dir):
        from line3d_amd.pipeline import Line3D
        from line3d_amd.synth import make_scene
        g = np.load(golden_jpeg)
        self.scene = make_scene(SCENE["n_views"], SCENE["n_segments"], SCENE["n_neighbors"],
                                **{k: v for k, v in SCENE.items() if k not in ("n_views", "n_segments", "n_neighbors")})
        self.base = str(base_dir)
        self.objects = {False: Line3D("", matchingNeighbors=6), True: None}
        one = self.objects[False]
        self.files = [g["view%d/bytes" % k].tobytes() for k in range(len(self.scene.views))]
        self.images = [np.ascontiguousarray(one.decode_jpeg(d)) for d in self.files]
        self.progressive = g["progressive/bytes"].tobytes()
        import jpeg_model as jm
        self.hollow = [d[:jm.parse(d)["scan_offset"]] + bytes(len(d) - jm.parse(d)["scan_offset"]) for d in self.files]
        self.flat = np.full((48, 64), 128, np.uint8)
        self.side = tempfile.mkdtemp(dir=self.base)        # the file behind the explicit cache handle: not in any data directory

    def close(self):
        for o in self.objects.values():
            if o is not None:
                o.close()

    def _object(self, node):
        from line3d_amd.pipeline import Line3D
        if self.objects[node] is None:
            self.objects[node] = Line3D("", matchingNeighbors=6, devices=[0, 0])
        l3d = self.objects[node]
        l3d.reset()
        return l3d

    # -- what a content becomes ------------------------------------------------------------------------------------------------------------
    def _arguments(self, c, k=SUBJECT):
        """the arrays of a content for view k (kept alive by the returned dict)"""
        v = self.scene.views[k]
        a = dict(id=int(v["id"]))
        K = np.ascontiguousarray(v["K"], dtype=np.float64).copy()
        if c.get("skew"):
            K[0, 1] = 0.5
        a["K"], a["R"], a["t"] = K, np.ascontiguousarray(v["R"], dtype=np.float64), np.ascontiguousarray(v["t"], dtype=np.float64)
        if c.get("null"):
            a[c["null"]] = None
        a["dist"] = None if c.get("dist") is None else np.ascontiguousarray(c["dist"], dtype=np.float64)
        if c.get("links") == "sims":
            ids = [] if c.get("n_links") == 0 else sorted(v["sims"])
            a["sims"] = np.ascontiguousarray([v["sims"][i] for i in ids] + [0.0], dtype=np.float32)
        else:
            ids = [] if c.get("n_links") == 0 else WORLDPOINTS
            a["sims"] = None
        a["link_ids"], a["n_links"] = np.ascontiguousarray(list(ids) + [0], dtype=np.uint32), len(ids)
        img = self.flat if c.get("img") == "flat" else self.images[k]
        a["img"], a["height"], a["width"] = img, img.shape[0], 0 if c.get("img") == "w0" else img.shape[1]
        a["channels"], a["stride"] = (1 if img.ndim == 2 else img.shape[2]), img.strides[0]
        a["pixels"] = img
        if c.get("img") == "null0":
            a["pixels"], a["width"], a["height"], a["stride"] = None, 0, 0, 0
        data = {"progressive": self.progressive, "four": self.files[k][:4], "hollow": self.hollow[k]}.get(c.get("bytes"), self.files[k])
        a["bytes"] = None if c.get("bytes") == "null" else np.frombuffer(data, dtype=np.uint8)
        a["segs"] = np.ascontiguousarray(v["segments"], dtype=np.float32).reshape(-1, 4)
        return a

    def _entry(self, c, k, keep):
        from line3d_amd import capi
        a = self._arguments(c, k)
        keep.append(a)
        e = capi.ImageEntry()
        e.image_id = a["id"]
        if c["src"] in ("pixels", "both"):
            e.pixels, e.width, e.height, e.channels, e.row_stride = (None if a["pixels"] is None else a["pixels"].ctypes.data), a["width"], a["height"], a["channels"], a["stride"]
        if c["src"] in ("jpeg", "both"):
            e.jpeg, e.jpeg_bytes = (None, 0) if a["bytes"] is None else (a["bytes"].ctypes.data, len(a["bytes"]))
        for f in ("K", "R", "t", "dist", "link_ids", "sims"):
            if a[f] is not None:
                setattr(e, f, a[f].ctypes.data)
        e.n_links = a["n_links"]
        return e

    def _cache_path(self, directory, c):
        from line3d_amd.io import segment_cache_filename
        a = self._arguments(c)
        w, h = a["img"].shape[1], a["img"].shape[0]
        return directory + segment_cache_filename(a["id"], w, h, True)       # (the name starts with the separator)

    def _write_cache(self, path):
        from line3d_amd.io import write_segment_cache
        segs = np.ascontiguousarray(self.scene.views[SUBJECT]["segments"], dtype=np.float32).reshape(-1, 4)[:10]
        write_segment_cache(path, segs, [0, 1], [1, 0], [0.5, 0.5])

    def _fill(self, l3d, views, sims):
        for k in views:
            v = self.scene.views[k]
            ok = l3d.addImage_fixed_sim(v["id"], v["width"], v["height"], v["segments"], v["K"], v["R"], v["t"], v["sims"]) if sims else \
                l3d.addImage(v["id"], v["width"], v["height"], v["segments"], v["K"], v["R"], v["t"], WORLDPOINTS)
            assert ok, "filling view %d" % k

    # -- the calls -------------------------------------------------------------------------------------------------------------------------
    def _named(self, l3d, form, a, directory, maxw, las, cache):
        h, I = l3d.h, C.c_uint32(a["id"])
        size = (C.c_uint(a["width"]), C.c_uint(a["height"]))
        cam = (_ptr(a["K"]), _ptr(a["R"]), _ptr(a["t"]))
        links = (_ptr(a["link_ids"]), C.c_int(a["n_links"])) if a["sims"] is None else (_ptr(a["link_ids"]), _ptr(a["sims"]), C.c_int(a["n_links"]))
        tail = (C.c_char_p(directory), C.c_int(maxw), C.c_int(las))
        img = (_ptr(a["pixels"]), C.c_int(a["width"]), C.c_int(a["height"]), C.c_int(a["channels"]), C.c_size_t(a["stride"]))
        segs = (_ptr(a["segs"]), C.c_int(len(a["segs"])))
        data = (_ptr(a["bytes"]), C.c_size_t(0 if a["bytes"] is None else len(a["bytes"])))
        args = {"add_image": size + segs + cam + links, "add_image_fixed_sim": size + segs + cam + links,
                "add_image_cached": size + (cache,) + cam + links,
                "add_image_ex": size + segs + cam + links + tail, "add_image_fixed_sim_ex": size + segs + cam + links + tail,
                "add_image_pixels": img + cam + links + tail, "add_image_pixels_fixed_sim": img + cam + links + tail,
                "add_image_pixels_distorted": img + cam + (_ptr(a["dist"]),) + links + tail,
                "add_image_pixels_fixed_sim_distorted": img + cam + (_ptr(a["dist"]),) + links + tail,
                "add_image_jpeg": data + cam + (_ptr(a["dist"]),) + links + tail,
                "add_image_jpeg_fixed_sim": data + cam + (_ptr(a["dist"]),) + links + tail}[form]
        return int(getattr(l3d.lib, "l3d_line3d_" + form)(h, I, *args))

    def run(self, case, via):
        """-> the record of one (case, via)"""
        from line3d_amd.io import open_segment_cache, close_segment_cache
        c, las, maxw = case["c"], int(case["las"]), int(case.get("maxw", 1920))
        l3d = self._object(bool(case.get("node")))
        lib = l3d.lib
        directory = tempfile.mkdtemp(dir=self.base)
        d = (directory + os.sep).encode()
        sims = c.get("links") == "sims"
        for step in case["setup"]:
            if step == "dup":
                self._fill(l3d, [SUBJECT], sims)
            elif step in ("cache", "cache_cut"):
                path = self._cache_path(directory, c)
                self._write_cache(path)
                if step == "cache_cut":
                    with open(path, "r+b") as f:
                        f.truncate(40)
            elif step == "computed":
                self._fill(l3d, FILL + (BEFORE,), sims)
                l3d.compute3Dmodel(False)
        cache = None
        rec = {}
        try:
            if via == "named":
                a = self._arguments(c)
                if c["src"] == "size_ex":
                    a["segs"] = a["segs"][:0]
                if c["src"] == "cached":
                    path = os.path.join(self.side, "cache.bin")
                    self._write_cache(path)
                    cache = open_segment_cache(path)
                rc = self._named(l3d, named_form(c), a, d, maxw, las, cache)
            else:
                keep = []
                good = dict(src="pixels", links=c.get("links", "wps")), dict(src="jpeg", links=c.get("links", "wps"))
                es = [self._entry(c, SUBJECT, keep)] if via in ("batch1", "entry") else \
                    [self._entry(good[0], BEFORE, keep), self._entry(c, SUBJECT, keep), self._entry(good[1], AFTER, keep)]
                from line3d_amd import capi
                arr = (capi.ImageEntry * len(es))(*es)
                if via == "entry":
                    rc = int(lib.l3d_line3d_add_image_entry(l3d.h, arr, C.c_char_p(d), C.c_int(maxw), C.c_int(las)))
                else:
                    status = (C.c_int * len(es))()
                    rc = int(lib.l3d_line3d_add_images(l3d.h, arr, C.c_int(len(es)), C.c_char_p(d), C.c_int(maxw), C.c_int(las), status))
                    rec["status"] = [int(s) for s in status]
            failed = rc != 0 or any(rec.get("status", []))
            rec["rc"] = rc
            rec["error"] = lib.l3d_line3d_last_error(l3d.h).decode().replace(directory + os.sep, "<dir>/").replace(directory, "<dir>") if failed else ""
            rec["cameras"] = int(l3d.numCameras())
            rec["listing"] = sorted(os.listdir(directory))
            if case.get("prepare"):
                self._fill(l3d, FILL, sims)
                rec["prepare_rc"] = int(lib.l3d_line3d_prepare(l3d.h))
                rec["listing_prepared"] = sorted(os.listdir(directory))
        finally:
            if cache is not None:
                close_segment_cache(cache)
        return rec
