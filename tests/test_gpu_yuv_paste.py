"""Crop tensors and warped face tensors pasted into NV12 frames that carry a colour description (include/sdm.h, "YUV colour description
and 10-bit surfaces"; csrc/sdm_yuv_device.h through the block path of csrc/sdm_paste_device.h): rigid and piecewise-affine, plain and
area-averaged, into NV12 under each of the six descriptions beside a plain "nv12" and a BGR frame in the same list.  Of the six names,
"nv12:bt601" -- BT.601, limited range -- IS value 5 by the bit layout (matrix bits 0, range bit 0): it is plain NV12 a second time, with
OpenCV's constants, so five descriptions run the derived encode and two frames the one that always was.  Luma and chroma
are bit for bit those of tests/paste_nv12_ref.py, warp_paste_nv12_ref.py and warp_paste_area_ref.py with the encode substituted
(tests/yuv_ref.py, `substituted`) -- the plain "nv12" and the BGR frame those of the references as they are --, compared on the WHOLE
buffer: every byte outside the footprints keeps its noise.  Then the round trip on the device, and the refusal of a P010 destination."""
import contextlib
import ctypes

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import paste_area_ref as PA
import paste_cases as PCS
import paste_nv12_ref as N
import paste_ref as P
import warp_cases as W
import warp_paste_area_ref as WPA
import warp_paste_nv12_ref as WN
import warp_paste_ref as WP
import warp_ref as WR
import yuv_cases as C
import yuv_ref as Y
from superviseddescent_amd import Context, HoGParam, _lib, align_filter, ibug

pytestmark = pytest.mark.gpu
f32 = np.float32
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
LM = np.array([3, 6, 9, 12, 15])
AREA = (PA.AREA, 16, 1.0)
COMBOS = [("uint8", "nhwc", 3, "bgr"), ("float16", "nchw", 3, "rgb"), ("float32", "nhwc", 1, "bgr"), ("float32", "nchw", 3, "rgb")]
# NV12 under each of the six names (module docstring: the first is value 5), a plain "nv12" and a BGR frame
FRAMES = [(37, 29, C.NAMES8[1], 1, False), (64, 48, C.NAMES8[2], 3, True), (5, 4, C.NAMES8[3], 0, True), (2, 2, C.NAMES8[4], 5, False),
          (1, 1, C.NAMES8[5], 0, True), (38, 34, C.NAMES8[0], 1, True), (37, 29, "nv12", 2, True), (37, 29, "bgr", 2, False)]


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


def spec_of(layout, order):
    return dict(layout=layout, order=order, scale=PCS.SCALES, bias=PCS.BIASES, gray_shift=14 if order == "bgr" else 15)


class Dest:
    """one destination frame inside a host copy of the buffer, as views the references write through"""

    def __init__(self, buf, f):
        st = np.lib.stride_tricks.as_strided
        h, w, s = f["h"], f["w"], f["stride"]
        self.f = f
        if f["fmt"] == T.NV12:
            self.Y, self.UV = st(buf[f["off"]:], (h, w), (s, 1)), st(buf[f["uv_off"]:], ((h + 1) // 2, (w + 1) // 2, 2), (s, 2, 1))
        else:
            self.pix = st(buf[f["off"]:], (h, w, 3), (s, 3, 1))

    def encode(self):
        """the frame's encode in place of the references' for the duration of a row"""
        d = self.f["desc"]
        return Y.substituted(d) if d is not None else contextlib.nullcontext()


def expect(buf, frames, idx, row):
    want = buf.copy()
    dest = {}
    for r, im in enumerate(idx):
        if im not in dest:
            dest[im] = Dest(want, frames[im])
        with dest[im].encode():
            row(dest[im], r)
    return want


def alpha_of(alpha, r):
    return None if alpha is None else alpha if alpha.ndim == 2 else alpha[r]


def maps(k, n, w, h):
    return (None, PCS.alpha_maps(1, w, h, 50 + k)[0], PCS.alpha_maps(n, w, h, 60 + k, zero_band=True))[k % 3]


def rigid_row(mats, x, alpha, filt, channels, spec):
    def row(d, r):
        S = 1 if filt is None or P.inverse(mats[r])[1] else PA.samples(mats[r], *filt)
        if d.f["fmt"] == T.NV12:
            N.paste_row(d.Y, d.UV, mats[r], x[r], alpha_of(alpha, r), S, channels=channels, **spec)
        else:
            PA.paste_row(d.pix, T.BGR, mats[r], x[r], alpha_of(alpha, r), S, channels=channels, **spec)
    return row


def mesh_row(points, tri, mats, lab, x, alpha, filt, channels, spec, frames, idx):
    def row(d, r):
        a, f = alpha_of(alpha, r), frames[idx[r]]
        if filt is None:
            if f["fmt"] == T.NV12:
                WN.paste_row(d.Y, d.UV, points[r], tri, mats[r], lab, x[r], a, channels=channels, **spec)
            else:
                WP.paste_row(d.pix, T.BGR, points[r], tri, mats[r], lab, x[r], a, channels=channels, **spec)
            return
        cnt = WPA.counts(points[r], tri, mats[r], f["w"], f["h"], *filt)
        if f["fmt"] == T.NV12:
            WPA.paste_row_nv12(d.Y, d.UV, points[r], tri, mats[r], lab, x[r], a, cnt, channels=channels, **spec)
        else:
            WPA.paste_row(d.pix, T.BGR, points[r], tri, mats[r], lab, x[r], a, cnt, channels=channels, **spec)
    return row


def filter_of(filt):
    return None if filt is None else align_filter("area", filt[1], filt[2])


def touched(want, buf, frames):
    """bytes changed per frame: the case cannot pass on frames nothing was pasted into"""
    return [int((want[C.owned(f)] != buf[C.owned(f)]).sum()) for f in frames]


RIGID_ROWS = [0, 1, 2, 3, 4, 5, 6, 7, 1, 5, 1]                       # row -> frame: three rows share frame 1, two (overlapping) frame 5


def rigid_case(frames, w, h, filt):
    mats = np.stack([S.astype(f32) for S in K.similarities(frames, RIGID_ROWS, w, h, 70 + w)])
    if filt:                                                       # (filtered: the crop outsizes the face, S > 1)
        mats[:, :, :2] /= f32(2.6)
        c = np.array([(w - 1) / 2, (h - 1) / 2], f32)
        for r, im in enumerate(RIGID_ROWS):
            mats[r][:, 2] = np.array([(frames[im]["w"] - 1) / 2, (frames[im]["h"] - 1) / 2], f32) - mats[r][:, :2] @ c
    mats[9] = mats[5].copy()
    mats[9][:, 2] += (3.5, -2.25)
    return mats


# ---- 9: the pastes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, AREA])
def test_rigid_paste_every_description(ctx, filt):
    import torch
    buf, frames = C.place(FRAMES, seed=29)
    w, h = K.CROPS[2]
    mats = rigid_case(frames, w, h, filt)
    for k, (dtype, layout, channels, order) in enumerate(COMBOS):
        x, alpha, spec = PCS.tensor(len(RIGID_ROWS), w, h, dtype, layout, channels, 80 + k), maps(k + 1, len(RIGID_ROWS), w, h), spec_of(layout, order)
        dev = torch.from_numpy(buf).cuda()
        lst, chroma = C.device_frames(dev, frames)
        got = ctx.align_paste_tensor_at(mats, torch.from_numpy(x).cuda(), lst, image_index=RIGID_ROWS, mask=alpha, chroma=chroma,
                                        filter=filter_of(filt), **spec)
        want = expect(buf, frames, RIGID_ROWS, rigid_row(mats, x, alpha, filt, channels, spec))
        assert np.array_equal(dev.cpu().numpy(), want), (dtype, layout, channels, order)
        assert all(n > 0 for n in touched(want, buf, frames)), touched(want, buf, frames)
        if filt:
            assert got[1].tolist() == [1 if P.inverse(m)[1] else PA.samples(m, *filt) for m in mats] and got[1].max() > 1
        if channels == 3:
            # the description matters: under the plain encode the described frames would hold other bytes
            plain = buf.copy()
            for r, im in enumerate(RIGID_ROWS):
                rigid_row(mats, x, alpha, filt, channels, spec)(Dest(plain, frames[im]), r)
            assert not np.array_equal(plain, want)


MESH_ROWS = [0, 1, 5, 6, 7, 2, 1, 5, 3, 4]                           # rows 1 and 6 on frame 1, rows 2 and 7 on frame 5 overlap


@pytest.mark.parametrize("filt", [None, AREA])
def test_mesh_paste_every_description(ctx, filt):
    import torch
    buf, frames = C.place(FRAMES, seed=29)
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    rows = W.rows_for(frames, MESH_ROWS, idx, t, w, h, 40)
    lab = WR.labels(t, tri, w, h)
    points = WP.points_of(rows, idx)
    mats = WP.matrices(points, t, tri)
    for k, (dtype, layout, channels, order) in enumerate(COMBOS):
        x, alpha, spec = PCS.tensor(len(MESH_ROWS), w, h, dtype, layout, channels, 90 + k), maps(k, len(MESH_ROWS), w, h), spec_of(layout, order)
        dev = torch.from_numpy(buf).cuda()
        lst, chroma = C.device_frames(dev, frames)
        got = ctx.warp_paste_tensor_at(points, torch.from_numpy(x).cuda(), lst, image_index=MESH_ROWS, mask=alpha, chroma=chroma,
                                       filter=filter_of(filt), **spec)
        want = expect(buf, frames, MESH_ROWS, mesh_row(points, tri, mats, lab, x, alpha, filt, channels, spec, frames, MESH_ROWS))
        assert np.array_equal(dev.cpu().numpy(), want), (dtype, layout, channels, order)
        assert (want != buf).sum() > 500
        if filt:
            cnt = np.stack([WPA.counts(points[r], tri, mats[r], frames[im]["w"], frames[im]["h"], *filt) for r, im in enumerate(MESH_ROWS)])
            assert np.array_equal(got[1], cnt)


# ---- 10: the round trip on the device --------------------------------------------------------------------------------------------
def test_round_trip_crop_then_paste(ctx):
    """Per description, frames of 8 x 8 blocks -- 16 x 16 pixels -- of one in-gamut colour each: the identity crop of the 12 x 12 pixels
    at the origin, pasted back with opacity 255, leaves every Y, U and V of the frame within +-1 of where it started (half a unit in,
    times coefficients whose absolute values sum to at most 1, plus half a unit out).  The crop ends inside the frame: a pixel of the
    frame's last column takes half its chroma from the fill of 128 outside the plane (the existing siting, position / 2), which no
    description can undo."""
    import torch
    colours = [(200, 120, 60), (30, 90, 220), (128, 128, 128), (250, 250, 5)]          # (R, G, B)
    specs = [(16, 16, name, 1 + i % 3, bool(i % 2)) for i, name in enumerate(C.NAMES8) for _ in colours]
    buf, frames = C.place(specs, seed=3)
    start = []
    for k, f in enumerate(frames):
        r, g, b = colours[k % len(colours)]
        bgr = np.array([b, g, r], np.int64)
        y = int(Y.luma_of(f["desc"])(bgr))
        u, v = (int(c) for c in Y.chroma_of(f["desc"])(bgr))
        d = Dest(buf, f)
        d.Y[...] = y
        d.UV[...] = (u, v)
        start.append((y, u, v))
    dev = torch.from_numpy(buf).cuda()
    lst, chroma = C.device_frames(dev, frames)
    idx = list(range(len(frames)))
    w = h = 12
    tmpl = (np.array([[0.2, 0.2], [0.8, 0.25], [0.5, 0.5], [0.3, 0.8], [0.75, 0.7]]) * (w - 1, h - 1)).astype(f32)
    ctx.set_frames_device(lst, chroma=chroma)
    ctx.set_sample_image_index(idx)
    ctx.set_x(K.landmark_rows([np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])] * len(frames), tmpl, LM, L))
    ctx.align_set_source_frames(lst, chroma=chroma)
    out, mats, flags = ctx.align_crops_tensor(LM, tmpl, w, h, dtype="uint8", layout="nhwc", channels=3, order="bgr")
    assert not flags.any()
    crops = out.cpu().numpy()
    for k, f in enumerate(frames):                                  # the crop is the decoded colour, and near the colour encoded
        want = Y.decode(f["desc"])(*start[k])
        assert (crops[k] == want).all(), f["name"]
        assert np.abs(want[::-1] - np.array(colours[k % len(colours)])).max() <= 2
    ctx.align_paste_tensor_at(mats, out, lst, image_index=idx, chroma=chroma, layout="nhwc", order="bgr")
    after = dev.cpu().numpy()
    worst = 0
    for k, f in enumerate(frames):
        d = Dest(after, f)
        for plane, v0 in ((d.Y, start[k][0]), (d.UV[..., 0], start[k][1]), (d.UV[..., 1], start[k][2])):
            worst = max(worst, int(np.abs(plane.astype(np.int64) - v0).max()))
    print("round trip: worst |difference| of a Y, U or V:", worst)
    assert worst <= 1
    untouched = np.ones(len(buf), bool)
    for f in frames:
        untouched[C.owned(f)] = False
    assert np.array_equal(after[untouched], buf[untouched])
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


BLOCK_COLOURS = [(200, 120, 60), (30, 90, 220), (128, 128, 128), (225, 225, 30), (60, 200, 90), (90, 40, 160), (210, 60, 140), (40, 160, 200)]


def block_frame(buf, f, seed):
    """the frame filled with 8 x 8-pixel blocks of differing in-gamut colours, encoded with its description: (Y, UV) as they start"""
    d = Dest(buf, f)
    rng = np.random.default_rng(seed)
    nb = (f["h"] + 7) // 8, (f["w"] + 7) // 8
    pick = rng.permutation(nb[0] * nb[1]) % len(BLOCK_COLOURS)
    for by in range(nb[0]):
        for bx in range(nb[1]):
            r, g, b = BLOCK_COLOURS[pick[by * nb[1] + bx]]
            bgr = np.array([b, g, r], np.int64)
            u, v = (int(c) for c in Y.chroma_of(f["desc"])(bgr))
            d.Y[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = int(Y.luma_of(f["desc"])(bgr))
            d.UV[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = (u, v)
    return d.Y.astype(np.int64), d.UV.astype(np.int64)


def interior(n, period):
    """positions 0 ... n - 1 whose bilinear chroma taps stay inside one block: not the last of a period (a pixel at an odd position
    reads the chroma sample at position / 2 and the next one; the last pixel of a block reads the next block's)"""
    return np.arange(n) % period != period - 1


def check_block_round_trip(f, before, after, crop):
    """+-1 on every luma pixel and chroma sample under the crop whose taps stay inside one block; everything outside the crop as it was"""
    (y0, uv0), (y1, uv1) = before, after
    w, h = crop
    ly, lx = interior(h, 8), interior(w, 8)
    cy, cx = interior(h // 2, 4), interior(w // 2, 4)
    dy = np.abs(y1[:h, :w] - y0[:h, :w])[np.ix_(ly, lx)]
    duv = np.abs(uv1[:h // 2, :w // 2] - uv0[:h // 2, :w // 2])[np.ix_(cy, cx)]
    assert np.array_equal(y1[h:], y0[h:]) and np.array_equal(y1[:, w:], y0[:, w:])
    assert np.array_equal(uv1[h // 2:], uv0[h // 2:]) and np.array_equal(uv1[:, w // 2:], uv0[:, w // 2:])
    return int(dy.max()), int(duv.max()), int(np.abs(uv1 - uv0).max())


def test_round_trip_on_blocks_of_differing_colours(ctx):
    """Per name, a 40 x 40 frame of 8 x 8-pixel blocks of differing in-gamut colours; the identity crop of the 32 x 32 pixels at the
    origin, pasted back with opacity 255.  +-1 is asserted where it can hold: on every luma pixel and chroma sample under the crop
    whose chroma taps stay inside one block.  At a block's last column or row the existing siting (position / 2) reads half the next
    block's chroma, which no description gives back; those samples are left out, and what lies outside the crop is as it was."""
    import torch
    specs = [(40, 40, name, 1 + i % 3, bool(i % 2)) for i, name in enumerate(C.NAMES8)]
    buf, frames = C.place(specs, seed=8)
    before = [block_frame(buf, f, 20 + k) for k, f in enumerate(frames)]
    dev = torch.from_numpy(buf).cuda()
    lst, chroma = C.device_frames(dev, frames)
    idx = list(range(len(frames)))
    w = h = 32
    tmpl = (np.array([[0.2, 0.2], [0.8, 0.25], [0.5, 0.5], [0.3, 0.8], [0.75, 0.7]]) * (w - 1, h - 1)).astype(f32)
    ctx.set_frames_device(lst, chroma=chroma)
    ctx.set_sample_image_index(idx)
    ctx.set_x(K.landmark_rows([np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])] * len(frames), tmpl, LM, L))
    ctx.align_set_source_frames(lst, chroma=chroma)
    out, mats, flags = ctx.align_crops_tensor(LM, tmpl, w, h, dtype="uint8", layout="nhwc", channels=3, order="bgr")
    assert not flags.any()
    ctx.align_paste_tensor_at(mats, out, lst, image_index=idx, chroma=chroma, layout="nhwc", order="bgr")
    after = dev.cpu().numpy()
    for k, f in enumerate(frames):
        d = Dest(after, f)
        worst_y, worst_uv, at_edges = check_block_round_trip(f, before[k], (d.Y.astype(np.int64), d.UV.astype(np.int64)), (w, h))
        print("%s: worst |difference| inside the blocks Y %d, UV %d; over all samples UV %d" % (f["name"], worst_y, worst_uv, at_edges))
        assert worst_y <= 1 and worst_uv <= 1, f["name"]
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- 11: a P010 destination is refused -------------------------------------------------------------------------------------------
def test_p010_destination_is_refused(ctx):
    import torch
    buf, frames = C.place([(16, 16, "p010:bt709", 2, False), (16, 16, "nv12:bt709", 1, False)], seed=4)
    dev = torch.from_numpy(buf).cuda()
    lst, chroma = C.device_frames(dev, frames)
    w = h = 7
    mats = np.stack([S.astype(f32) for S in K.similarities(frames, [0, 1], w, h, 5)])
    x = torch.from_numpy(PCS.tensor(2, w, h, "uint8", "nhwc", 3, 6)).cuda()
    spec = _lib.paste_tensor_spec("uint8", "nhwc", 3, "bgr")
    paste = _lib.SdmAlignPaste(None, 0)
    flags = np.zeros(2, np.int32)
    lib = _lib.lib()
    wtri = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(*wtri)
    ctx.warp_set_mesh(idx, t, tri, *wtri)
    points = WP.points_of(W.rows_for(frames, [0, 1], idx, t, wtri[0], wtri[1], 40), idx)
    xw = torch.from_numpy(PCS.tensor(2, wtri[0], wtri[1], "uint8", "nhwc", 3, 7)).cuda()
    # an image set of its own, read by a detect before and after every refusal: it stays the one in use
    rng = np.random.default_rng(13)
    gray = torch.from_numpy(rng.integers(0, 256, (64, 72), dtype=np.uint8)).cuda()
    ctx.set_frames_device([gray])
    for lvl, p in enumerate(PARAMS):
        ctx.set_regressor(lvl, rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32))
    boxes = np.array([[10, 8, 40, 40], [20, 12, 36, 36]], np.int32)

    def detect():
        ctx.set_sample_image_index([0, 0])
        ctx.init_from_boxes(ibug.select_mean(IDS), boxes)
        return ctx.detect_batch()

    found = detect()
    assert np.isfinite(found).all()

    def same_image_set():
        return np.array_equal(detect().view(np.uint32), found.view(np.uint32)) and np.array_equal(ctx.download_image(0), gray.cpu().numpy())

    def arr(fs):
        return (_lib.SdmFrame * len(fs))(*[_lib.SdmFrame(p, fw, fh, st, _lib._frame_format(name)) for p, fw, fh, st, name in fs])

    cases = {
        "rigid, nv12 form": lambda: lib.sdm_align_paste_tensor_at_nv12(ctx._h, mats.ctypes.data, None, 2, w, h, ctypes.byref(spec), None,
                                                                       ctypes.c_void_p(x.data_ptr()), ctypes.byref(paste), arr(lst), None, 2,
                                                                       flags.ctypes.data, None),
        "rigid, plain form": lambda: lib.sdm_align_paste_tensor_at(ctx._h, mats.ctypes.data, None, 2, w, h, ctypes.byref(spec),
                                                                   ctypes.c_void_p(x.data_ptr()), ctypes.byref(paste), arr(lst[:1]), 1,
                                                                   flags.ctypes.data),
    }
    for name, fn in cases.items():
        assert fn() == _lib.SDM_ERR_INVALID, name
        assert np.array_equal(dev.cpu().numpy(), buf), name
        assert same_image_set(), name
    from superviseddescent_amd import SdmError
    with pytest.raises(SdmError, match="P010") as e:
        ctx.warp_paste_tensor_at(points, xw, lst, image_index=[0, 1], chroma=chroma, layout="nhwc", order="bgr")
    assert e.value.code == _lib.SDM_ERR_INVALID
    with pytest.raises(SdmError, match="P010"):
        ctx.align_paste_tensor_at(mats, x, lst, image_index=[0, 1], chroma=chroma, filter=align_filter("area"), layout="nhwc", order="bgr")
    assert np.array_equal(dev.cpu().numpy(), buf) and same_image_set()
    # the NV12 frame beside it is a valid destination on its own
    ctx.align_paste_tensor_at(mats[1:], x[1:].clone(), lst[1:], image_index=[0], chroma=chroma[1:], layout="nhwc", order="bgr")
    assert not np.array_equal(dev.cpu().numpy(), buf)
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])
