"""The detector over a batch (l3d_detect_segments_batch) against the single calls on the same device: for every image of a batch the bytes are those
of l3d_detect_segments / _distorted / _jpeg for that image alone, whatever else is in the batch and in whatever order.  The single call is the
oracle everywhere; where a case needs segments to mean anything, the single call is asserted to find some."""
import os

import numpy as np
import pytest

from detect_stage_cases import _spiral
from line3d_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROGRESSIVE_OR_CMYK, INVALID = 5, 1        # L3D_ERR_UNSUPPORTED, L3D_ERR_INVALID


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "detect_ref.npz")))


@pytest.fixture(scope="module")
def stages():
    return dict(np.load(os.path.join(GOLDEN, "detect_stages.npz")))


@pytest.fixture(scope="module")
def jpeg():
    return dict(np.load(os.path.join(GOLDEN, "jpeg_ref.npz")))


@pytest.fixture(scope="module")
def noisy(gpu_ctx, ref):
    """the ten 320x240 noisy images and what the single call gives for each (computed once)"""
    images = [ref["img_noisy%02d" % i] for i in range(10)]
    single = [gpu_ctx.detect_segments(img) for img in images]
    assert min(len(s) for s in single) > 0
    return images, single


def _same(batch, single):
    assert len(batch) == len(single)
    for k, (b, s) in enumerate(zip(batch, single)):
        assert b.dtype == np.float32 and b.shape == s.shape and b.tobytes() == s.tobytes(), "image %d: %d segments in the batch, %d alone" % (k, len(b), len(s))


def test_batch_of_one_and_of_ten_in_both_orders(gpu_ctx, noisy):
    images, single = noisy
    _same(gpu_ctx.detect_segments_batch(images[:1]), single[:1])
    _same(gpu_ctx.detect_segments_batch(images), single)
    _same(gpu_ctx.detect_segments_batch(images[::-1]), single[::-1])
    assert gpu_ctx.detect_segments_batch([]) == []


def test_image_borders_inside_a_chunk(gpu_ctx, ref):
    """an edge a few rows above the bottom of one image, a flat image, an edge a few rows below the top of the next: a link or a rectangle scan across
    a border would change the first or the third"""
    edge = ref["img_edge0"]
    rows = np.flatnonzero(np.abs(np.diff(edge.astype(np.int32), axis=0)).max(axis=1) > 0)
    assert len(rows) > 0
    at = int(rows[0])                                   # the edge lies between rows `at` and `at + 1`
    low, high = np.roll(edge, (edge.shape[0] - 5) - at, axis=0), np.roll(edge, 4 - at, axis=0)
    # the roll moves the image's wrap-around seam as well: keep only one transition, the edge itself
    low[:edge.shape[0] - 5 - 30] = low[edge.shape[0] - 5 - 30]
    high[4 + 30:] = high[4 + 30]
    images = [low, ref["img_flat"], high]
    single = [gpu_ctx.detect_segments(img, min_length=0.0) for img in images]
    assert len(single[0]) >= 1 and len(single[1]) == 0 and len(single[2]) >= 1
    assert single[0][:, [1, 3]].min() > edge.shape[0] - 12 and single[2][:, [1, 3]].max() < 12
    _same(gpu_ctx.detect_segments_batch(images, min_lengths=[0.0] * 3), single)
    _same(gpu_ctx.detect_segments_batch(images[::-1], min_lengths=[0.0] * 3), single[::-1])


def test_convergence_is_shared_without_effect(gpu_ctx, ref, stages):
    rects = stages["rg_img_rects"]
    one = gpu_ctx.detect_segments(rects, min_length=0.0)
    assert len(one) > 0
    _same(gpu_ctx.detect_segments_batch([rects, rects.copy()], min_lengths=[0.0, 0.0]), [one, one])
    # a one-pixel arm winding inwards (the labelling needs many looks) beside a flat image (it needs one)
    spiral = np.where(_spiral(80, 96), 220, 40).astype(np.uint8)
    flat = np.ascontiguousarray(ref["img_flat"][:80, :96])
    single = [gpu_ctx.detect_segments(img, min_length=0.0) for img in (spiral, flat, rects)]
    assert len(single[0]) > 0 and len(single[1]) == 0
    _same(gpu_ctx.detect_segments_batch([spiral, flat, rects], min_lengths=[0.0] * 3), single)
    _same(gpu_ctx.detect_segments_batch([flat, rects, spiral], min_lengths=[0.0] * 3), [single[1], single[2], single[0]])


def test_cap_and_ties_are_per_image(gpu_ctx, noisy):
    images, single = noisy
    assert min(len(s) for s in single[:4]) > 2
    caps = [2, 0, 1 << 20, 2]
    got = gpu_ctx.detect_segments_batch(images[:4], max_segments=caps)
    alone = [gpu_ctx.detect_segments(img, max_segments=c) for img, c in zip(images[:4], caps)]
    assert [len(a) for a in alone] == [2, 0, len(single[2]), 2]
    _same(got, alone)
    # the same image four times: every candidate ties with its copies in the other images
    _same(gpu_ctx.detect_segments_batch([images[0]] * 4, max_segments=[2, 3000, 1, 3000]), [single[0][:2], single[0], single[0][:1], single[0]])
    lengths = [0.0, 40.0, None, 15.0]
    alone = [gpu_ctx.detect_segments(img, min_length=m) for img, m in zip(images[:4], lengths)]
    assert len(alone[0]) > len(alone[1]) > 0
    _same(gpu_ctx.detect_segments_batch(images[:4], min_lengths=lengths), alone)


def test_mixed_plans_in_one_call(gpu_ctx, stages, noisy):
    images, _ = noisy
    padded = np.full((240, 320 + 37), 77, np.uint8)
    padded[:, :320] = images[3]
    view = padded[:, :320]
    assert view.strides[0] == 357
    batch = [stages["px_n37x29"], images[0], stages["px_n161x41"], stages["px_rs64x48"], view, stages["px_n37x29"][::-1].copy(), images[1]]
    sizes = [None, None, None, (26, 20), None, None, (200, 150)]
    single = [gpu_ctx.detect_segments(img, new_size=s, min_length=0.0) for img, s in zip(batch, sizes)]
    assert sum(len(s) for s in single) > 0 and len(single[4]) > 0 and len(single[6]) > 0
    _same(gpu_ctx.detect_segments_batch(batch, new_sizes=sizes, min_lengths=[0.0] * len(batch)), single)


def test_chunks_of_two(gpu_ctx, noisy):
    images, single = noisy
    gpu_ctx.set_option("L3D_DET_BATCH_IMAGES", 2)
    try:
        gpu_ctx.profile_enable(True)
        gpu_ctx.profile_reset()
        _same(gpu_ctx.detect_segments_batch(images[:5]), single[:5])
        assert gpu_ctx.profile_get("k_det_region")[0] == 3 * 3              # chunks of 2, 2 and 1
    finally:
        gpu_ctx.profile_enable(False)
        gpu_ctx.set_option("L3D_DET_BATCH_IMAGES", 0)


def test_cameras_vary_inside_a_chunk(gpu_ctx, noisy):
    images, single = noisy
    cams = [(300.0, 300.0, 160.0, 120.0, -0.12, 0.03), (300.0, 300.0, 160.0, 120.0, 0.0, 0.0), None]
    alone = [gpu_ctx.detect_segments(img, camera=c) for img, c in zip(images[:3], cams)]
    assert len(alone[0]) > 0 and alone[0].tobytes() != single[0].tobytes()
    assert alone[1].tobytes() == single[1].tobytes()
    _same(gpu_ctx.detect_segments_batch(images[:3], cameras=cams), alone)
    _same(gpu_ctx.detect_segments_batch(images[2::-1], cameras=cams[::-1]), alone[::-1])


def test_jpeg_entries(gpu_ctx, jpeg):
    files = [jpeg["view%d/bytes" % i].tobytes() for i in range(6)]
    single = [gpu_ctx.detect_segments_jpeg(f) for f in files]
    assert min(len(s) for s in single) > 0
    _same(gpu_ctx.detect_segments_batch(files), single)
    # files and pixels of one size share a chunk
    pixels = jpeg["view2/pixels"]
    mixed = gpu_ctx.detect_segments_batch([files[0], pixels, files[5]])
    _same(mixed, [single[0], gpu_ctx.detect_segments(pixels), single[5]])
    for name in ("progressive", "cmyk"):
        refused = jpeg[name + "/bytes"].tobytes()
        got, status = gpu_ctx.detect_segments_batch(files[:3] + [refused] + files[3:], return_status=True)
        assert status == [0, 0, 0, PROGRESSIVE_OR_CMYK, 0, 0, 0] and len(got[3]) == 0
        assert b"entry 3: jpeg" in gpu_ctx.lib.l3d_last_error(gpu_ctx.h)
        _same(got[:3] + got[4:], single)
    cut = files[4][:len(files[4]) * 2 // 3]              # the headers are whole, the entropy-coded data ends early
    with pytest.raises(capi.L3DError) as alone:
        gpu_ctx.detect_segments_jpeg(cut)
    assert alone.value.code == INVALID
    got, status = gpu_ctx.detect_segments_batch(files[:2] + [cut] + files[2:4], return_status=True)
    assert status == [0, 0, INVALID, 0, 0] and len(got[2]) == 0
    assert str(alone.value).split(": ", 1)[1] in gpu_ctx.lib.l3d_last_error(gpu_ctx.h).decode()
    _same(got[:2] + got[3:], single[:4])
    with pytest.raises(capi.L3DError) as err:
        gpu_ctx.detect_segments_batch(files[:2] + [cut])
    assert err.value.code == INVALID and err.value.statuses == [0, 0, INVALID]


def test_launches_do_not_depend_on_the_batch(gpu_ctx, noisy):
    images, single = noisy
    names = ("k_det_region", "det_sort_pixels", "k_det_label_hook", "k_det_label_compress", "k_det_grey", "k_det_grad", "k_det_select_gather")

    def count(batch):
        gpu_ctx.profile_reset()
        got = gpu_ctx.detect_segments_batch(batch)
        return got, {k: gpu_ctx.profile_get(k)[0] for k in names}

    gpu_ctx.profile_enable(True)
    try:
        got1, one = count([images[0]])
        got8, eight = count([images[0]] * 8)                   # the same labelling eight times: the same looks
        _, mixed = count(images[:8])
    finally:
        gpu_ctx.profile_enable(False)
    print("launches for one image %s, for eight copies %s, for eight images %s" % (one, eight, mixed))
    _same(got1, single[:1])
    _same(got8, [single[0]] * 8)
    assert one["k_det_region"] == 3 and one["det_sort_pixels"] == 3 and one["k_det_grey"] == 1 and one["k_det_label_hook"] % 3 == 0
    assert eight == one
    for k in ("k_det_region", "det_sort_pixels", "k_det_grey", "k_det_grad", "k_det_select_gather"):
        assert mixed[k] == one[k]
    assert mixed["k_det_label_hook"] % 3 == 0 and mixed["k_det_label_hook"] < 8 * one["k_det_label_hook"]


def test_deterministic(gpu_ctx, noisy, jpeg):
    images, single = noisy
    batch = images[:4] + [jpeg["view1/bytes"].tobytes(), jpeg["view3/bytes"].tobytes()]
    a = gpu_ctx.detect_segments_batch(batch)
    b = gpu_ctx.detect_segments_batch(batch)
    _same(a, b)
    _same(a[:4], single[:4])
    other = capi.Context(0)
    try:
        _same(other.detect_segments_batch(batch), a)
    finally:
        other.close()
