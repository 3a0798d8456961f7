"""Frame geometry beyond 256 x 256 (tests/frame_geometry_cases.py): pitches that carry the byte offset inside an image past 2^16,
2^24 and up to and over 2^31, frames of 65 535 and 65 600 rows and of 70 000 columns, frames of one set more than 2^32 bytes apart,
the converter on frames of many workgroups, and the crops, the tracker and its motion search on the same sets.  Every frame is a view into ONE device
buffer of 255s, so a read of padding differs from the black canvas; the same pixels as dense host arrays go through the CPU
references: the oracle (integer decisions bit for bit, feature rows within the bound of test_gpu_packing.py), align_ref and
align_tensor_ref (bit for bit), track_ref (the lost mask), orc.bgr2gray (bit for bit).

What keeps a case from passing by accident (frame_geometry_cases.conditions, asserted per case on the oracle's decisions): a patch
wholly inside the frame, a patch across each border the case is about, and a patch with pixels beyond the boundary the case names.
test_case_table (no GPU) recomputes every named quantity and runs the CPU references on the arrays."""
import contextlib

import numpy as np
import pytest

import align_ref as A
import align_tensor_ref as T
import frame_geometry_cases as G
import track_motion_ref as R
import track_ref as TR
from oracle import sdm_oracle as orc
from superviseddescent_amd import HoGParam, LinearRegressor, SupervisedDescentOptimiser, alignment_template, detection_model, ibug
from superviseddescent_amd.engine import hog_plan
from superviseddescent_amd._lib import SDM_HOG_COLUMNS

gpu = pytest.mark.gpu
L, IDS, MEAN, RE, LE = G.L, G.IDS, G.MEAN, G.RE, G.LE
PARAMS = [HoGParam(*p) for p in G.HOG]
LMS = np.array([3, 6, 9, 12, 15, 18, 21]) % L
CROP = 24
SPECS = [dict(dtype="float16", layout="nchw", channels=3, order="rgb", scale=np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], np.float32),
              bias=np.array([-2.1179, -2.0357, -1.8044], np.float32)),
         dict(dtype="uint8", layout="nhwc", channels=1)]
FMT = {"gray": T.GRAY, "nv12": T.NV12, "bgr": T.BGR, "rgb": T.RGB, "bgra": T.BGRA, "rgba": T.RGBA}


# ---- no GPU: the table, the layout, the CPU references on the arrays -------------------------------------------------------------------
def row_intervals(f):
    """(first, last + 1) byte of every row of a frame inside the buffer, chroma rows included"""
    rows = f["h"] + ((f["h"] + 1) // 2 if f["fmt"] == "nv12" else 0)
    start = f["off"] + np.arange(rows, dtype=np.int64) * f["pitch"]
    return np.stack([start, start + max(f["w"] * G.BPP[f["fmt"]], 2 * ((f["w"] + 1) // 2) if f["fmt"] == "nv12" else 0)], 1)


def disjoint(frames):
    iv = np.concatenate([row_intervals(f) for f in frames])
    iv = iv[np.argsort(iv[:, 0])]
    return bool((iv[1:, 0] >= iv[:-1, 1]).all())


def test_case_table():
    for case, what, value, lo, hi in G.table():
        assert lo < value <= hi, (case, what, value, lo, hi)
    assert {t[0] for t in G.table()} == set("1234567")                 # (case 8 runs on the frames of 3 and 4)
    for f in G.all_frames():
        assert f["off"] >= 4096 and f["off"] + G.extent(f) + 4096 <= G.BUF_BYTES, f
        assert f["pitch"] >= f["w"] * G.BPP[f["fmt"]]
    # frames that are on the device at the same time share no byte
    for together in (G.FAR, G.STACK, G.conv_frames(), [G.NV12_24, G.NV12_31] + G.NV12_TWINS):
        assert disjoint(together)
    # the stack is what sdm_set_images_device(n = 3) addresses
    assert [f["off"] - G.STACK[0]["off"] for f in G.STACK] == [i * G.FH * G.STACK_PITCH for i in range(3)]
    # every detect case meets its conditions on the oracle's decisions; the oracle runs on these arrays
    for name in G.detect_cases():
        x0, feat, dec = G.level0(name)
        assert np.isfinite(feat).all() and (dec[:, 0] > 0).all(), name
        assert G.unmet(name) == [], (name, G.unmet(name))
    # every patch of the largest-stride case keeps (rows outside) * stride inside the documented limit
    x0_, y0_, x1_, y1_ = G.patches(G.level0("1 largest fused stride")[2])
    assert (np.maximum(-y0_, y1_ - G.MAXP_H).max() + 1) * G.MAX_STRIDE < 2 ** 31
    # the tracker's streams: the conditions, and track_ref on these rows (a stream beyond 2^16 inside, the last one outside)
    for which in TRACK:
        img, f, boxes, far_stream, borders, beyond = tracker_case(which)
        rows = G.aligned(boxes)
        dec = G.oracle_level([img], np.zeros(len(boxes), np.int32), rows, 0)[1]
        assert G.conditions(dec, [(f["w"], f["h"])] * len(boxes), borders, beyond) == [], which
        lost = TR.lost_mask(rows, rows, f["w"], f["h"], 8.0, 1.5, RE, LE)
        assert lost[far_stream] == 0 and lost[-1] == TR.OUTSIDE and not lost[:-1].any(), (which, lost)
    # the motion cases: their conditions on the restatement, the streams' first rows standing in for the device's
    for name, (images, boxes, idx, frames, borders, beyond, far) in G.motion_cases().items():
        rows = G.aligned(boxes)
        sizes = np.array([(frames[i]["w"], frames[i]["h"]) for i in idx])
        lost = TR.lost_mask(rows, rows, sizes[:, 0], sizes[:, 1], 8.0, 1.5, RE, LE)
        assert (lost == 0).sum() >= 3, name
        assert G.motion_plan(name, rows, lost)[5] == [], (name, G.motion_plan(name, rows, lost)[5])
        assert all(f in G.all_frames() for f in frames) and len(images) == len(frames)
    # ... and one that lacks the interior stream is caught: nothing on the far frame takes a shift
    grids = {1: (2, -40, -30), 0: (3, 2, 1)}                           # (stream 1 on the far frame, stream 0 on another)
    assert G.motion_unmet("far apart", grids, {1: (0, 0), 0: (6, -3)}) == ["a stream of the far frame that takes a non-zero shift"]
    # case 7's rows
    assert case7_unmet(G.oracle_level([nv12_pixels(k)[0] for k in (0, 0, 1, 1)], CASE7_IDX, G.aligned(case7_boxes()), 0)[1]) == []
    # ... and a case that lacks one is caught: without its last three boxes the wide frame has no patch beyond column 65 536
    images, boxes, idx, frames, borders, beyond, far = G.detect_cases()["4 width 70000"]
    assert "a patch beyond the boundary" in G.conditions(G.level0("4 width 70000")[2][:3], [(G.WIDE_W, G.WIDE_H)] * 3, borders, beyond)
    # the crop references on a tall and a wide frame and on an NV12 surface, the converter's reference on its frames
    M = np.array([[1.5, 0.2, 69980.0], [-0.2, 1.5, 20.0]], np.float32)
    assert A.warp(G.wide()[0], M, CROP, CROP).any() and A.partial(M, CROP, CROP, G.WIDE_W, G.WIDE_H)
    M = np.array([[1.5, 0.2, 10.0], [-0.2, 1.5, 65500.0]], np.float32)
    assert A.warp(G.tall(65535)[0], M, CROP, CROP).any()
    y, uv = nv12_pixels(0)
    M = np.array([[2.0, 0.0, 20.0], [0.0, 2.0, 10.0]], np.float32)
    assert T.tensor(T.Frame(T.NV12, y, uv), M, CROP, CROP, **SPECS[0]).shape == (3, CROP, CROP)
    for f, pix in zip(G.conv_frames(), conv_pixels()):
        assert orc.bgr2gray(to_bgr(pix, f["fmt"]), 15).shape == (f["h"], f["w"])


def to_bgr(pix, fmt):
    return np.ascontiguousarray(pix[..., 2::-1] if fmt in ("rgb", "rgba") else pix[..., :3])


def conv_pixels():
    rng = np.random.default_rng(66)
    return [rng.integers(0, 256, (f["h"], f["w"], G.BPP[f["fmt"]]), dtype=np.uint8) for f in G.conv_frames()]


def nv12_pixels(k):
    """(luma 80 x 96: a face cut; chroma 40 x 48 x 2: noise)"""
    return G.faces()[0][k % 3], np.random.default_rng(40 + k).integers(0, 256, (G.FH // 2, G.FW // 2, 2), dtype=np.uint8)


CASE7_FRAMES = [G.NV12_24, G.NV12_TWINS[0], G.NV12_31, G.NV12_TWINS[1]]
CASE7_IDX = np.array([0, 1, 2, 3] * 5, np.int32)


def case7_boxes():
    return np.repeat(G.faces()[1], 4, 0)                                   # box k on all four frames: rows 4 k ... 4 k + 3


def case7_unmet(dec):
    """case 7's conditions: all borders; a patch with luma rows more than 2^24 bytes into its plane (the far chroma lies behind them)"""
    pitch = np.array([CASE7_FRAMES[i]["pitch"] for i in CASE7_IDX], np.int64)[:, None]
    return G.conditions(dec, [(G.FW, G.FH)] * len(CASE7_IDX), "left right top bottom", lambda x0, y0, x1, y1, w, h: (y1 - 1) * pitch > 2 ** 24)


TRACK = ["tall 65535", "tall 65600", "wide"]


def tracker_case(which):
    """(image, frame, boxes of the streams -- the last one centred just outside the image --, the stream beyond 2^16 or at the last
    rows, the borders and the boundary of the case)"""
    if which == "wide":
        (img, boxes), f = G.wide(), G.WIDE
        boxes = list(boxes[:5]) + [(f["w"] - 25, 12, 60, 60)]              # (4: around column 69 950; last: centre 5 columns outside)
        return img, f, np.array(boxes, np.int32), 4, "left right", lambda x0, y0, x1, y1, w, h: x1 - 1 >= 65536
    hh = int(which.split()[1])
    (img, boxes), f = G.tall(hh), G.TALL[hh]
    near = (-6, 65470, 60, 60) if hh == 65535 else (4, 65535, 56, 56)        # centre around row 65 500 | beyond row 65 536
    boxes = list(boxes[:4]) + [near, (2, hh - 25, 60, 60)]                 # (last: centre 5 rows below the image)
    return img, f, np.array(boxes, np.int32), 4, "top bottom", lambda x0, y0, x1, y1, w, h: y1 - 1 >= min(hh - 1, 65536)


# ---- the device buffer and the model -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(built):
    import torch
    buf = torch.full((G.BUF_BYTES,), 255, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def model(gpu_ctx):
    """the two-level RCR-22 model of test_gpu_frames_device.py: small random regressors, a level moves a landmark by about a pixel"""
    rng = np.random.default_rng(77)
    regs = []
    for p in PARAMS:
        r = LinearRegressor()
        r.x = rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32)
        regs.append(r)
    sdo = SupervisedDescentOptimiser(regs, ctx=gpu_ctx)
    yield detection_model(sdo, MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    gpu_ctx.align_set_source_frames(None)
    gpu_ctx.upload_images([np.zeros((4, 4), np.uint8)])                # (the session's context keeps no pointer into this module's buffer)
    gpu_ctx.set_sample_image_index(None)


def views_of(big, f):
    import torch
    c = G.BPP[f["fmt"]]
    if c > 1:
        return [torch.as_strided(big, (f["h"], f["w"], c), (f["pitch"], c, 1), f["off"])]
    v = [torch.as_strided(big, (f["h"], f["w"]), (f["pitch"], 1), f["off"])]
    if f["fmt"] == "nv12":
        v.append(torch.as_strided(big, ((f["h"] + 1) // 2, (f["w"] + 1) // 2, 2), (f["pitch"], 2, 1), f["off"] + f["h"] * f["pitch"]))
    return v


@contextlib.contextmanager
def placed(big, frames, pixels):
    """the pixels written into their views (only the viewed bytes are copied); the buffer is all 255 again afterwards.  Yields the
    (ptr, w, h, pitch, format) tuples.  pixels: one array per frame, NV12: (luma, chroma)."""
    import torch
    views = []
    try:
        for f, p in zip(frames, pixels):
            vs = views_of(big, f)
            for v, a in zip(vs, p if isinstance(p, tuple) else (p,)):
                v.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
            views += vs
        torch.cuda.synchronize()                                        # (the library runs on a stream of its own)
        yield [(big.data_ptr() + f["off"], f["w"], f["h"], f["pitch"], f["fmt"]) for f in frames]
    finally:
        for v in views:
            v.fill_(255)
        torch.cuda.synchronize()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def bind(model):
    ctx = model.optimised_model.ctx
    ctx.set_model_geometry(L, RE, LE, PARAMS)
    model.optimised_model._load_regressors()
    model.optimised_model._bound = None
    ctx.set_templates(None)
    ctx.set_hog_mode(SDM_HOG_COLUMNS)
    ctx.set_hog_packing(True)
    ctx.align_set_source_frames(None)
    # both levels HAVE the fused kernels: what runs then depends on the image set alone (a set that qualifies runs hog_packed_kernel
    # and, with packing off, the one-patch-per-wave kernel; any other the generic one)
    for level, p in enumerate(PARAMS):
        info = ctx.hog_info(level)
        assert info["fast_kernel"] is True and info["fast_bins"] == 2 and hog_plan(p.num_cells, p.cell_size, p.num_bins, L) is not None
    return ctx


def cascade(ctx, idx, x0):
    """Both launches of every level from the level's own input rows, then the cascade in one call.  Returns ([(x, packed features,
    its decisions, one-patch-per-wave features, its decisions)] per level, the rows after detect_batch)."""
    ctx.set_sample_image_index(idx)
    levels, x = [], x0
    for level in range(len(PARAMS)):
        ctx.set_x(x)
        packed, pidx = ctx.hog_features(level, fetch=True), ctx.patch_indices()
        ctx.set_hog_packing(False)
        plain, qidx = ctx.hog_features(level, fetch=True), ctx.patch_indices()
        ctx.set_hog_packing(True)
        levels.append((x, packed, pidx, plain, qidx))
        ctx.detect_level(level)
        x = ctx.get_x()
    ctx.set_x(x0)
    final = ctx.detect_batch()
    assert np.array_equal(bits(final), bits(x))                        # (the levels one by one are the cascade)
    return levels, final


def check_oracle(name, levels, images, idx):
    """integer decisions bit for bit, feature rows within the bound of test_packed_equals_plain_and_oracle, at every level"""
    for level, (x, packed, pidx, plain, qidx) in enumerate(levels):
        ofeat, odec = G.level0(name)[1:] if level == 0 else G.oracle_level(images, idx, x, level)
        if level == 0:
            assert G.unmet(name, odec) == [], (name, G.unmet(name, odec))
        print("%s level %d: packed - oracle %.3g (rel %.3g), packed - plain %.3g, decisions differ in %d / %d" % (
            name, level, np.abs(packed - ofeat).max(), rel_l2(packed, ofeat), np.abs(packed - plain).max(),
            int((pidx != odec).sum()), int((qidx != odec).sum())))
        assert np.array_equal(pidx, odec) and np.array_equal(qidx, odec), (name, level)
        assert np.isfinite(packed).all() and (packed[:, -1] == 1.0).all()
        assert np.abs(packed - plain).max() <= 2e-7
        assert np.abs(packed - ofeat).max() <= 1e-6 and rel_l2(packed, ofeat) <= 5e-7
        assert np.abs(plain - ofeat).max() <= 1e-6 and rel_l2(plain, ofeat) <= 5e-7


def check_crops(ctx, lst, host, idx, rows):
    """case 7 on the current rows: the gray crops of the context's images against align_ref, the tensor crops of the frame list
    against align_tensor_ref, through the device's own matrices"""
    tmpl = alignment_template(MEAN, LMS, CROP, CROP, 0.2)
    ctx.align_set_source(None)
    crops, mats, flags = ctx.align_crops(LMS, tmpl, CROP, CROP)
    assert crops.any() and np.isfinite(mats).all() and not (flags & A.DEGENERATE).any()
    for r, im in enumerate(idx):
        assert np.array_equal(crops[r, ..., 0], A.warp(host[im].pix, mats[r], CROP, CROP)), r
        assert flags[r] == (A.PARTIAL if A.partial(mats[r], CROP, CROP, host[im].w, host[im].h) else 0), r
    ctx.align_set_source_frames(lst)
    out = []
    for spec in SPECS:
        got, m2, f2 = ctx.align_crops_tensor(LMS, tmpl, CROP, CROP, **spec)
        assert np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
        got = got.cpu().numpy()
        for r, im in enumerate(idx):
            assert np.array_equal(bits(got[r]), bits(T.tensor(host[im], m2[r], CROP, CROP, **spec))), (r, spec["dtype"])
        out.append(got)
    ctx.align_set_source_frames(None)
    return crops, out


def run_case(model, big, name, entry, fmt="gray", crops=False):
    """one detect case through one entry point: the oracle at every level, the host upload of the same pixels (an extra), the crops"""
    images, boxes, idx, frames, borders, beyond, far = G.detect_cases()[name]
    ctx = bind(model)
    x0 = G.level0(name)[0]
    frames = [dict(f, fmt=fmt) for f in frames]
    pixels = [(im, nv12_pixels(k)[1]) if fmt == "nv12" else im for k, im in enumerate(images)]
    with placed(big, frames, pixels) as lst:
        if entry == "frames":
            ctx.set_frames_device(lst)
        elif entry == "images":
            f = frames[0]
            ctx.set_images_device(lst[0][0], len(frames), f["w"], f["h"], f["pitch"])
        else:
            ctx.upload_images(images)
        levels, final = cascade(ctx, idx, x0)
        assert all(np.array_equal(ctx.download_image(i), im) for i, im in enumerate(images))
        check_oracle(name, levels, images, idx)
        if crops:
            host = [T.Frame(FMT[fmt], *(p if isinstance(p, tuple) else (p,))) for p in pixels]
            check_crops(ctx, lst, host, idx, final)
        ctx.upload_images([np.zeros((4, 4), np.uint8)])
    return final


def host_upload(model, name):
    images, boxes, idx, frames, borders, beyond, far = G.detect_cases()[name]
    ctx = bind(model)
    ctx.upload_images(images)
    ctx.set_sample_image_index(idx)
    ctx.set_x(G.level0(name)[0])
    return ctx.detect_batch()


# ---- case 1: the byte offset inside the image crosses 2^16, 2^24 and approaches 2^31 (crops: case 7) ----------------------------------------
@gpu
@pytest.mark.parametrize("fmt", ["gray", "nv12"])
@pytest.mark.parametrize("name", list(G.CASE1))
def test_case1_offsets_inside_an_image(model, big, name, fmt):
    final = run_case(model, big, "1 " + name, "frames", fmt, crops=True)
    if G.CASE1[name]["pitch"] <= G.MAX_STRIDE:                          # the fused kernels both times: the same bits as the host upload
        assert np.array_equal(bits(final), bits(host_upload(model, "1 " + name)))      # (beyond: the generic kernel here, the fused one there)


@gpu
def test_case1_faces_far_above_and_below_the_largest_pitch(model, big):
    """rows so far outside the image that a 32-bit (row * pitch) wraps back into the plane: black, as for the oracle (such a pitch
    is served by the generic kernel: image_needs_generic)"""
    run_case(model, big, "1 rows far outside", "frames")


@gpu
@pytest.mark.parametrize("entry", ["frames", "images"])
def test_case1_largest_stride_of_the_fused_kernels(model, big, entry):
    """the largest stride image_needs_generic leaves to the fused kernels, h * stride up to INT_MAX - 2^20 + 1, faces 2 000 rows
    above and below the image: the documented limit (rows outside) * stride < 2^31 from the inside"""
    final = run_case(model, big, "1 largest fused stride", entry, crops=entry == "frames")
    assert np.array_equal(bits(final), bits(host_upload(model, "1 largest fused stride")))


# ---- case 2: h * pitch just above INT_MAX, through the routed and through the older entry --------------------------------------------------
@gpu
@pytest.mark.parametrize("entry", ["frames", "images"])
def test_case2_plane_over_int_max(model, big, entry):
    run_case(model, big, "2 over INT_MAX", entry)


# ---- case 3: the row index at and beyond 16 bits (crops: case 7) ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("entry", ["upload", "images", "frames"])
@pytest.mark.parametrize("h", [65535, 65600])
def test_case3_tall_frames(model, big, h, entry):
    name = "3 height %d" % h
    final = run_case(model, big, name, entry, crops=entry == "frames")
    if entry != "upload":
        assert np.array_equal(bits(final), bits(host_upload(model, name)))


# ---- case 4: the column index beyond 16 bits (crops: case 7) --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("entry", ["upload", "images", "frames"])
def test_case4_wide_frame(model, big, entry):
    final = run_case(model, big, "4 width 70000", entry, crops=entry == "frames")
    if entry != "upload":
        assert np.array_equal(bits(final), bits(host_upload(model, "4 width 70000")))


# ---- case 5: frames of one set more than 2^32 bytes apart, the first one the highest; the stack's offset[2] above 2^31 -------------------------
@gpu
def test_case5_frames_far_apart(model, big):
    final = run_case(model, big, "5 far apart", "frames", crops=True)
    assert np.array_equal(bits(final), bits(host_upload(model, "5 far apart")))


@gpu
def test_case5_stack_offsets(model, big):
    run_case(model, big, "5 stack", "images")                              # (a stride of 2^24: the generic kernel, no bits shared with an upload)


# ---- case 6: the converter on frames of many workgroups, small frames between them, a row beyond 2^32 -----------------------------------------
@gpu
@pytest.mark.parametrize("shift", [14, 15])
def test_case6_converter(gpu_ctx, big, shift):
    frames, pixels = G.conv_frames(), conv_pixels()
    want = [orc.bgr2gray(to_bgr(p, f["fmt"]), shift) for f, p in zip(frames, pixels)]
    with placed(big, frames, pixels) as lst:
        gpu_ctx.set_frames_device(lst, gray_shift=shift)                   # ONE call
        bad = [(i, frames[i]) for i in range(len(frames)) if not np.array_equal(gpu_ctx.download_image(i), want[i])]
        assert not bad, bad
        for f, p in zip(frames, pixels):                                   # the source is only read
            assert np.array_equal(views_of(big, f)[0].cpu().numpy(), p)
        gpu_ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- case 7: NV12 surfaces with a far chroma plane and with a plane that needs 64-bit offsets, each beside a twin at a small pitch ---------------
@gpu
def test_case7_nv12_crops_and_twins(model, big):
    ctx = bind(model)
    frames = CASE7_FRAMES
    pixels = [nv12_pixels(0), nv12_pixels(0), nv12_pixels(1), nv12_pixels(1)]
    host = [T.Frame(T.NV12, *p) for p in pixels]
    idx = CASE7_IDX
    x0 = G.aligned(case7_boxes())
    with placed(big, frames, pixels) as lst:
        ctx.set_frames_device(lst)
        levels, final = cascade(ctx, idx, x0)
        images = [p[0] for p in pixels]
        for level, (x, packed, pidx, plain, qidx) in enumerate(levels):
            ofeat, odec = G.oracle_level(images, idx, x, level)
            assert level > 0 or case7_unmet(odec) == []
            assert np.array_equal(pidx, odec) and np.array_equal(qidx, odec)
            assert np.abs(packed - ofeat).max() <= 1e-6 and rel_l2(packed, ofeat) <= 5e-7
        gray, tensors = check_crops(ctx, lst, host, idx, final)
        # twins: the same pixels, the same rows, the same crops
        assert np.array_equal(bits(final[0::4]), bits(final[1::4])) and np.array_equal(bits(final[2::4]), bits(final[3::4]))
        for got in [gray] + tensors:
            assert np.array_equal(bits(got[0::4]), bits(got[1::4])) and np.array_equal(bits(got[2::4]), bits(got[3::4]))
        assert tensors[0].any()
        ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- case 8: the tracker on the tall and on the wide frame, several streams on one image ---------------------------------------------------
@gpu
@pytest.mark.parametrize("which", TRACK)
def test_case8_tracker(model, big, which):
    img, f, boxes, far, borders, beyond = tracker_case(which)
    dec = G.oracle_level([img], np.zeros(len(boxes), np.int32), G.aligned(boxes), 0)[1]
    assert G.conditions(dec, [(f["w"], f["h"])] * len(boxes), borders, beyond) == []
    n = len(boxes)
    ids, zeros = np.arange(n), np.zeros(n, np.int32)
    MIN_SIZE, MAX_SCALE = 8.0, 1.5
    runs = []
    with placed(big, [f], [img]) as lst:
        for frames in (lst, [img]):
            tr = model.tracker(n, init="previous", min_size=MIN_SIZE, max_scale_change=MAX_SCALE)
            tr.start(ids, boxes)
            r1, l1 = tr.step(ids, frames, image_index=zeros)
            keep = ids[l1 == 0]
            r2, l2 = tr.step(keep, frames, image_index=zeros[:len(keep)])
            runs.append((r1, l1, r2, l2, tr.get(ids)))
        model.optimised_model.ctx.upload_images([np.zeros((4, 4), np.uint8)])
    (r1, l1, r2, l2, (state, status)), host = runs
    assert np.array_equal(bits(r1), bits(host[0])) and np.array_equal(l1, host[1])
    assert np.array_equal(bits(r2), bits(host[2])) and np.array_equal(l2, host[3])
    assert np.array_equal(bits(state), bits(host[4][0])) and np.array_equal(status, host[4][1])
    assert np.array_equal(l1, TR.lost_mask(G.aligned(boxes), r1, f["w"], f["h"], MIN_SIZE, MAX_SCALE, RE, LE))
    keep = ids[l1 == 0]
    assert np.array_equal(l2, TR.lost_mask(r1[keep], r2, f["w"], f["h"], MIN_SIZE, MAX_SCALE, RE, LE))
    centre = (r1[far, :L].min() + r1[far, :L].max()) / 2 if which == "wide" else (r1[far, L:].min() + r1[far, L:].max()) / 2
    assert 65400 < centre < (f["w"] if which == "wide" else f["h"]) and l1[far] == 0 and far in keep and l2[list(keep).index(far)] == 0
    if which != "tall 65535":
        assert centre > 65536
    assert l1[n - 1] & TR.OUTSIDE and np.isfinite(r1).all()


# ---- case 9: the tracker's motion-compensated initialisation on the tall, the wide, the far and the stacked frames ---------------------------
MOTION_CASES = [("tall 65600", "gray"), ("wide", "gray"), ("over INT_MAX", "gray"), ("over INT_MAX", "nv12"), ("pitch to 2^31", "gray"),
                ("far apart", "gray"), ("stack", "gray")]


@gpu
@pytest.mark.parametrize("name,fmt", MOTION_CASES, ids=["%s-%s" % c for c in MOTION_CASES])
def test_case9_tracker_motion(model, big, name, fmt):
    """step 1 on the case's pixels; step 2 on the same frames rewritten, every image's content moved by whole cells of the streams on
    it.  Chips, grids, last results and the stepped rows against tests/track_motion_ref.py, the stepped rows against detect from the
    shifted initialisation on the dense host arrays, and every device result against the same tracker on those arrays."""
    import torch
    images, boxes, idx, frames, borders, beyond, far = G.motion_cases()[name]
    n = len(boxes)
    ids = np.arange(n)
    MIN_SIZE, MAX_SCALE = 8.0, 1.5
    frames = [dict(f, fmt=fmt) for f in frames]
    pixels = [(im, nv12_pixels(k)[1]) if fmt == "nv12" else im for k, im in enumerate(images)]
    sizes = np.array([(frames[i]["w"], frames[i]["h"]) for i in idx])
    ctx = model.optimised_model.ctx
    # a pitch beyond the fused kernels' is served by the generic pixel kernel, which shares no bits with them: where the case's frames
    # need it, a one-column image at the end of the host set makes that set take it too (image_needs_generic: w < 2)
    generic = any(f["pitch"] > G.MAX_STRIDE or f["pitch"] * f["h"] > G.INT_MAX for f in frames)
    extra = [np.zeros((4, 1), np.uint8)] if generic else []
    runs, plan = [], None
    with placed(big, frames, pixels) as lst:
        for on_device in (True, False):
            tr = model.tracker(n, init="previous", min_size=MIN_SIZE, max_scale_change=MAX_SCALE, motion=G.MOTION)
            tr.start(ids, boxes)
            r1, l1 = tr.step(ids, lst if on_device else images + extra, image_index=idx)
            m1 = tr.motion(ids)
            if plan is None:
                plan = G.motion_plan(name, r1, l1)
            ref, stored, keep, moved, shifts, unmet = plan
            if on_device:
                for f, a in zip(frames, moved):                        # the luma rewritten in place, the pitch bytes untouched
                    views_of(big, f)[0].copy_(torch.from_numpy(a).cuda())
                torch.cuda.synchronize()
            r2, l2 = tr.step(keep, lst if on_device else moved + extra, image_index=idx[keep])
            runs.append((r1, l1, m1, r2, l2, tr.motion(ids)))
        ref, stored, keep, moved, shifts, unmet = plan
        # detect from the shifted initialisation on the dense host arrays
        init = R.shifted(runs[0][0][keep], shifts)
        ctx.upload_images(moved + extra)
        ctx.set_sample_image_index(idx[keep])
        ctx.set_x(init)
        detected = ctx.detect_batch()
        ctx.set_sample_image_index(None)
        ctx.upload_images([np.zeros((4, 4), np.uint8)])
    dev, host = runs
    for a, b in zip(dev[:2] + dev[2] + dev[3:5] + dev[5], host[:2] + host[2] + host[3:5] + host[5]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    r1, l1, m1, r2, l2, m2 = dev
    assert unmet == [], (name, unmet)
    assert np.array_equal(l1, TR.lost_mask(G.aligned(boxes), r1, sizes[:, 0], sizes[:, 1], MIN_SIZE, MAX_SCALE, RE, LE))
    for got, want in zip(m1, stored):
        assert np.array_equal(got, want)
    print("%s %s: cell sizes %s, shifts %s" % (name, fmt, ref.grid[keep, 0].tolist(), shifts.tolist()))
    assert np.array_equal(bits(r2), bits(detected))
    assert np.array_equal(l2, TR.lost_mask(init, r2, sizes[keep, 0], sizes[keep, 1], MIN_SIZE, MAX_SCALE, RE, LE))
    ref.store_step(keep, r2, l2, moved, idx[keep])
    for got, want in zip(m2, ref.get(ids)):
        assert np.array_equal(got, want)
