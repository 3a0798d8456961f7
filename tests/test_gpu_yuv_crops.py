"""YUV frames with a colour description, and P010 surfaces, as the crop source and as the image set (include/sdm.h, "YUV colour
description and 10-bit surfaces"; csrc/sdm_yuv_device.h, the P010 taps of csrc/sdm_align_tensor_device.h and the area sums,
csrc/sdm_frames.hip): the identity crop, the four crop calls on one mixed list, the image set with detect and the tracker, the refusals
and the 64-bit offsets.  Every comparison is bit for bit: NV12 frames against the existing references with the conversion substituted
(tests/yuv_ref.py, `substituted`), BGR and plain "nv12" frames against the references as they are, P010 frames against yuv_ref's 10-bit
fetches, always on the device's own matrices."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest

import align_area_cases as AC
import align_area_ref as AR
import align_tensor_cases as K
import align_tensor_ref as T
import warp_area_cases as WAC
import warp_area_ref as WA
import warp_cases as W
import warp_ref as WR
import yuv_cases as C
import yuv_ref as Y
from superviseddescent_amd import (Context, HoGParam, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, align_filter,
                                   detection_model, ibug, synth)

pytestmark = pytest.mark.gpu
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
MEAN = ibug.select_mean(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
LM = AC.LM
SCALES = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], np.float32)
BIASES = np.array([-2.1179, -2.0357, -1.8044], np.float32)
# both layouts and the three dtypes at 3 channels; one dtype at 1 channel
COMBOS = [(d, l, 3, o) for (d, l), o in zip(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw")), ("bgr", "rgb") * 3)] + \
    [("float32", "nchw", 1, "bgr")]
# the mixed list: BGR, plain "nv12", two described NV12 and two P010 frames, and the 1 x 1 and 2 x 2 frames
MIXED = [(37, 29, "bgr", 2, False), (38, 34, "nv12", 1, True), (5, 4, "nv12:bt709", 0, False), (64, 48, "nv12:bt2020:full", 3, True),
         (37, 29, "p010:bt709", 2, False), (38, 34, "p010:bt2020:full", 6, True), (1, 1, "p010:bt709", 0, True), (2, 2, "nv12:bt709", 5, True)]


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def placed():
    buf, frames = C.place(MIXED)
    return buf, frames, [C.host_frame(buf, f) for f in frames]


def template(w, h):
    return (np.array([[0.2, 0.2], [0.8, 0.25], [0.5, 0.5], [0.3, 0.8], [0.75, 0.7]]) * (w - 1 + 1e-3, h - 1 + 1e-3)).astype(np.float32) + 0.125


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def spec_of(dtype, layout, channels, order):
    return dict(dtype=dtype, layout=layout, channels=channels, order=order, scale=SCALES, bias=BIASES, gray_shift=14 if order == "bgr" else 15)


def want(call, f, hf, *args):
    """(kind, bgr, y) of one row: `call` in rigid | area | warp | warp_area on frame f (its host copy hf)"""
    if f["fmt"] == "p010":
        return {"rigid": Y.rigid, "area": Y.area, "warp": Y.warp, "warp_area": Y.warp_area}[call](hf, *args)
    with (Y.substituted(f["desc"]) if f["desc"] is not None else contextlib.nullcontext()):
        if call == "rigid":
            kind, bgr = T.warped(hf, *args)
            return kind, bgr, (T.luma(hf, *args) if kind == "nv12" else None)
        return {"area": AR.warped, "warp": WR.warped, "warp_area": WA.warped}[call](hf, *args)


def compare(got, want_of_row, rows, frames, spec):
    got = got.cpu().numpy()
    for r, im in enumerate(rows):
        w = T.finish(*want_of_row[r], **spec)
        assert got[r].dtype == w.dtype and got[r].shape == w.shape
        assert np.array_equal(bits(got[r]), bits(w)), (r, im, frames[im]["name"], spec["dtype"], spec["layout"], spec["channels"])


def install(ctx, dev, frames, idx, x):
    lst, chroma = C.device_frames(dev, frames)
    ctx.set_frames_device(lst, chroma=chroma)
    ctx.set_sample_image_index(idx)
    ctx.set_x(x)
    ctx.align_set_source_frames(lst, chroma=chroma)
    return lst, chroma


def restore(ctx):
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- 6: the identity crop --------------------------------------------------------------------------------------------------------
def test_identity_crop_every_description(ctx):
    """one NV12 and one P010 frame under each of the six descriptions; the row's landmarks equal the template, so every luma tap weight
    is 1024 and a pixel at even coordinates is the frame's own (Y, U, V) through the description's decode"""
    import torch
    sizes = [(37, 29), (38, 34), (64, 48)]
    pads = {"nv12": (1, 2, 3, 5, 0, 4), "p010": (0, 2, 6, 4, 2, 0)}           # (odd pitches; even ones for P010)
    specs = [sizes[i % 3] + (name, pads[name[:4]][i % 6], bool(i % 2)) for i, name in enumerate(C.NAMES8 + C.NAMES10)]
    buf, frames = C.place(specs, seed=41)
    host = [C.host_frame(buf, f) for f in frames]
    dev = torch.from_numpy(buf).cuda()
    w = h = 16
    idx = list(range(len(frames)))
    ident = [np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])] * len(frames)
    install(ctx, dev, frames, idx, K.landmark_rows(ident, template(w, h), LM, L))
    spec = dict(dtype="uint8", layout="nhwc", channels=3, order="bgr")
    out, mats, flags = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
    assert not flags.any()
    compare(out, [want("rigid", f, hf, mats[r], w, h) for r, (f, hf) in enumerate(zip(frames, host))], idx, frames, spec)
    got = out.cpu().numpy()
    for r, (f, hf) in enumerate(zip(frames, host)):
        if f["fmt"] == "p010":
            y, uv = hf.y.astype(np.int64), hf.uv.astype(np.int64)
        else:
            y, uv = hf.pix.astype(np.int64), hf.uv.astype(np.int64)
        direct = Y.decode(f["desc"])(y[:h:2, :w:2], uv[:h // 2, :w // 2, 0], uv[:h // 2, :w // 2, 1])
        assert np.array_equal(got[r][::2, ::2], direct), f["name"]
    assert np.array_equal(dev.cpu().numpy(), buf)
    restore(ctx)


# ---- 7: the four crop calls on the mixed list ------------------------------------------------------------------------------------
def test_rigid_crops_mixed_list(ctx, placed):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    idx = [5, 3, 1, 0, 2, 4, 6, 7, 4, 5]
    w, h = K.CROPS[2]
    x = K.landmark_rows(K.similarities(frames, idx, w, h, 30 + w), template(w, h), LM, L)
    x[8, :L] += 700.0                                              # row 8: wholly outside its frame
    install(ctx, dev, frames, idx, x)
    cache = None
    for combo in COMBOS:
        spec = spec_of(*combo)
        out, mats, flags = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
        if cache is None:
            cache = [want("rigid", frames[im], host[im], mats[r], w, h) for r, im in enumerate(idx)]
            assert not cache[8][1].any() and sum(int(c[1].any()) for c in cache) >= 8
        compare(out, cache, idx, frames, spec)
    assert np.array_equal(dev.cpu().numpy(), buf)                  # the in-place source is only read
    restore(ctx)


def test_area_crops_mixed_list_at_every_s(ctx, placed):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    w, h = K.CROPS[1]
    seen = set()
    for idx, sims, want_S in AC.mixed_rows(frames, w, h, 70 + w):
        install(ctx, dev, frames, idx, K.landmark_rows(sims, template(w, h), LM, L))
        cache = None
        for combo in COMBOS:
            spec = spec_of(*combo)
            out, mats, flags, samples = ctx.align_crops_tensor(LM, template(w, h), w, h, filter="area", **spec)
            assert list(samples) == want_S
            if cache is None:
                cache = [want("area", frames[im], host[im], mats[r], w, h, int(samples[r])) for r, im in enumerate(idx)]
            compare(out, cache, idx, frames, spec)
        seen |= {(im, S) for im, S in zip(idx, want_S)}
    assert seen == {(im, S) for im in range(len(frames)) for _, S in AC.CLASSES}      # every frame at every S
    assert np.array_equal(dev.cpu().numpy(), buf)
    restore(ctx)


WARP_ROWS = [0, 1, 3, 4, 5, 2, 7, 6]                                # row -> frame


@pytest.mark.parametrize("filtered", [False, True])
def test_warps_mixed_list(ctx, placed, filtered):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    filt = align_filter("area")
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    x = WAC.rows_for(frames, WARP_ROWS, idx, t, w, h, WAC.SEED, scales=[0.6, 2.6, 1.7, 4.2, 3.3, 0.9, 2.1, 1.4]) if filtered else \
        W.rows_for(frames, WARP_ROWS, idx, t, w, h, 40)
    install(ctx, dev, frames, WARP_ROWS, x)
    cache = None
    for combo in COMBOS:
        spec = spec_of(*combo)
        if filtered:
            out, mats, flags, smp = ctx.warp_crops_tensor(filter=filt, **spec)
            if cache is None:
                assert smp.max() > 1
                cache = [want("warp_area", frames[im], host[im], mats[r].reshape(-1, 6), lab, smp[r]) for r, im in enumerate(WARP_ROWS)]
        else:
            out, mats, flags = ctx.warp_crops_tensor(**spec)
            if cache is None:
                cache = [want("warp", frames[im], host[im], mats[r].reshape(-1, 6), lab) for r, im in enumerate(WARP_ROWS)]
        compare(out, cache, WARP_ROWS, frames, spec)
    assert sum(int(c[1].any()) for c in cache) >= 6
    assert np.array_equal(dev.cpu().numpy(), buf)
    restore(ctx)


# ---- 8: the image set ------------------------------------------------------------------------------------------------------------
def test_image_set_bytes(ctx, placed):
    import torch
    buf, frames, host = placed
    full = C.place([(37, 29, "nv12:bt709:full", 3, True), (33, 16, "p010:bt601", 4, False), (16, 5, "p010", 0, True), (70, 9, "p010:bt2020:full", 2, True)], 43)
    buf2, frames2 = full
    dev, dev2 = torch.from_numpy(buf).cuda(), torch.from_numpy(buf2).cuda()
    for d, b, fs in ((dev, buf, frames), (dev2, buf2, frames2)):
        lst, chroma = C.device_frames(d, fs)
        ctx.set_frames_device(lst, chroma=chroma)
        for i, f in enumerate(fs):
            hf = C.host_frame(b, f)
            if f["fmt"] == "p010":
                expect = Y.luma8(hf.y).astype(np.uint8)                                  # min(255, ((word >> 6) + 2) >> 2)
            elif f["fmt"] == T.BGR:
                continue
            else:
                expect = hf.pix                                                          # Y as it is, whatever the description
            assert np.array_equal(ctx.download_image(i), expect), f["name"]
        assert np.array_equal(d.cpu().numpy(), b)                                        # the source is only read
    restore(ctx)


def random_model():
    rng = np.random.default_rng(77)
    regs = []
    for p in PARAMS:
        r = LinearRegressor()
        r.x = rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32)
        regs.append(r)
    return detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def test_detect_and_tracker_on_p010_equal_the_gray_frames(built):
    """P010 frames whose gray formula gives exactly the bytes of a gray u8 frame: detect_batch and three tracker steps, bit for bit"""
    import torch
    model = random_model()
    tracks, _, boxes = synth.make_tracks(2, 3, seed=31)            # frames x streams x H x W
    rng = np.random.default_rng(9)
    cut = ((slice(0, 200), slice(10, 250)), (slice(20, 256), slice(0, 220)))      # two sizes
    shift = np.array([[10, 0], [0, 20]])
    grays, p010, keep = [], [], []
    for t in range(3):
        grays.append([]), p010.append([])
        for s in range(2):
            g = np.ascontiguousarray(tracks[t, s][cut[s]])
            h, w = g.shape
            stride = 2 * w + (6 if s else 0)
            # Y10 = 4 g + d with d in {0, 1}: (Y10 + 2) >> 2 == g; noise in the six low bits, in the pitch padding and in the UV plane
            y10 = 4 * g.astype(np.uint16) + rng.integers(0, 2, g.shape, dtype=np.uint16)
            words = (y10 << 6) | rng.integers(0, 64, g.shape, dtype=np.uint16)
            raw = rng.integers(0, 256, (h + (h + 1) // 2, stride), dtype=np.uint8)
            raw[:h, :2 * w] = words.view(np.uint8).reshape(h, 2 * w)
            d = torch.from_numpy(raw).cuda()
            keep.append((d, raw))
            p010[t].append((d.data_ptr(), w, h, stride, "p010:bt709" if s else "p010"))
            grays[t].append(torch.from_numpy(g).cuda())
    b0 = boxes[0].copy()
    b0[:, 0] -= shift[:, 0]
    b0[:, 1] -= shift[:, 1]
    bx = np.array([b0[0], b0[1], b0[0] + [6, -4, 0, 0], b0[1] + [-5, 7, 0, 0], b0[0] + [-40, -60, 0, 0]], np.int32)
    idx = np.array([0, 1, 0, 1, 0], np.int32)
    a = model.detect_batch(grays[0], bx, idx)
    b = model.detect_batch(p010[0], bx, idx)
    assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b))
    ids = np.arange(2)
    runs = []
    for frames in (p010, grays):
        tr = model.tracker(2)
        tr.start(ids, b0)
        out = [tr.step(ids, frames[t]) for t in (0, 1, 2)]
        out.append(tr.get(ids))
        runs.append(out)
    for u, v in zip(*runs):
        assert np.array_equal(bits(u[0]), bits(v[0])) and np.array_equal(u[1], v[1])
    assert np.isfinite(runs[0][2][0]).all()
    for d, raw in keep:
        assert np.array_equal(d.cpu().numpy(), raw)                # the source is only read


# ---- 11: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(ctx, placed):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    idx = [0, 1, 4]
    w = h = 7
    x = K.landmark_rows(K.similarities(frames, idx, w, h, 5), template(w, h), LM, L)
    lst, chroma = install(ctx, dev, frames, idx, x)
    rng = np.random.default_rng(12)
    for lvl, p in enumerate(PARAMS):
        ctx.set_regressor(lvl, rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32))
    spec = spec_of("float32", "nchw", 3, "rgb")

    boxes = np.array([[4, 2, 24, 24], [6, 5, 26, 26], [3, 1, 22, 22]], np.int32)

    def state():
        ctx.init_from_boxes(MEAN, boxes)
        found = ctx.detect_batch()                                 # (the image set, read by a detect)
        ctx.set_x(x)
        return (found,) + tuple(ctx.align_crops_tensor(LM, template(w, h), w, h, **spec))

    before = state()
    assert np.isfinite(before[0]).all()
    images = [ctx.download_image(i) for i in range(len(frames))]
    lib = _lib.lib()
    big = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = big.data_ptr()
    assert p % 4 == 0
    NV12, P010, B709, FULL = _lib.SDM_FRAME_NV12, _lib.SDM_FRAME_P010, _lib.SDM_FRAME_YUV_BT709, _lib.SDM_FRAME_YUV_FULL

    def arr(fs):
        return (_lib.SdmFrame * len(fs))(*[_lib.SdmFrame(*f) for f in fs])

    def image_set(f):
        return lib.sdm_set_frames_device(ctx._h, arr([f]), 1, 14)

    def source(f, uv=None):
        return lib.sdm_align_set_source_frames(ctx._h, arr([f]), None if uv is None else (ctypes.c_void_p * 1)(uv), 1)

    bad = {
        "a flag on BGR": (p, 8, 8, 40, _lib.SDM_FRAME_BGR | B709),
        "a flag on GRAY": (p, 8, 8, 40, _lib.SDM_FRAME_GRAY | FULL),
        "a flag on planar": (p, 8, 8, 40, _lib.SDM_FRAME_BGR_PLANAR | B709),
        "matrix 0x300": (p, 8, 8, 40, NV12 | 0x300),
        "bit 13": (p, 8, 8, 40, NV12 | 0x2000),
        "bit 13 on P010": (p, 8, 8, 40, P010 | 0x2000),
        "P010, an odd pointer": (p + 1, 8, 8, 40, P010),
        "P010, an odd stride": (p, 8, 8, 41, P010 | B709),
        "P010, stride < 2 * width": (p, 8, 8, 14, P010),
    }
    cases = {}
    for name, f in bad.items():
        cases["image set: " + name] = lambda f=f: image_set(f)
        cases["crop source: " + name] = lambda f=f: source(f)
    cases["crop source: P010, an odd UV pointer"] = lambda: source((p, 8, 8, 40, P010), p + 8 * 40 + 1)
    cases["crop source: P010, a UV row that does not fit"] = lambda: source((p, 9, 8, 18, P010))
    for name, fn in cases.items():
        assert fn() == _lib.SDM_ERR_INVALID, name
        after = state()
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(after, before)), name
        assert all(np.array_equal(ctx.download_image(i), im) for i, im in enumerate(images)), name
    # the valid neighbours of the cases above are accepted
    assert source((p, 8, 8, 40, P010 | B709 | FULL), p + 8 * 40 + 2) == 0 and source((p, 8, 8, 40, NV12 | 0x200 | FULL)) == 0
    # sdm_align_crops, the interleaved u8 form, refuses P010 as it refuses NV12, naming the tensor call
    ctx.align_set_source_frames(lst[4:5], chroma=chroma[4:5])
    ctx.set_frames_device(lst[4:5], chroma=chroma[4:5])
    ctx.set_sample_image_index([0])
    ctx.set_x(x[2:3])
    with pytest.raises(SdmError, match="sdm_align_crops_tensor") as e:
        ctx.align_crops(LM, template(w, h), w, h)
    assert e.value.code == _lib.SDM_ERR_INVALID
    out = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
    assert np.array_equal(bits(out[0]), bits(before[1][2:3]))
    assert np.array_equal(dev.cpu().numpy(), buf)
    restore(ctx)


# ---- 12: offsets -----------------------------------------------------------------------------------------------------------------
def test_p010_plane_beyond_int_max_takes_64_bit_offsets(ctx):
    """a 96 x 80 P010 frame whose height * stride_bytes exceeds INT_MAX, its UV rows in the gaps between the luma rows, inside ONE
    untouched allocation of which only the frame's rows are written; the same pixels at a small pitch give the same bits"""
    import torch
    w, h = 96, 80
    cw2, ch2 = (w + 1) // 2, (h + 1) // 2
    stride = ((2 ** 31 - 1) // h + 2) // 2 * 2 + 2
    assert h * stride > 2 ** 31 - 1 and stride % 2 == 0
    rng = np.random.default_rng(90)
    yw = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    uvw = rng.integers(0, 65536, (ch2, 2 * cw2), dtype=np.uint16)
    off, uv_gap = 64, 4096                                          # the UV plane starts 4096 bytes behind the luma's first row
    big = torch.empty(off + (h - 1) * stride + 2 * w + 64, dtype=torch.uint8, device="cuda")
    torch.as_strided(big, (h, 2 * w), (stride, 1), off).copy_(torch.from_numpy(yw.view(np.uint8).reshape(h, 2 * w)).cuda())
    torch.as_strided(big, (ch2, 4 * cw2), (stride, 1), off + uv_gap).copy_(torch.from_numpy(uvw.view(np.uint8).reshape(ch2, 4 * cw2)).cuda())
    small = np.zeros((h + ch2, 2 * w + 6), np.uint8)
    small[:h, :2 * w] = yw.view(np.uint8).reshape(h, 2 * w)
    small[h:, :4 * cw2] = uvw.view(np.uint8).reshape(ch2, 4 * cw2)
    twin = torch.from_numpy(small).cuda()
    name = "p010:bt2020"
    lst = [(big.data_ptr() + off, w, h, stride, name), (twin.data_ptr(), w, h, 2 * w + 6, name)]
    chroma = [big.data_ptr() + off + uv_gap, None]
    f = dict(w=w, h=h)
    cw, ch = 16, 16
    rows = K.landmark_rows(K.similarities([f], [0, 0, 0, 0], cw, ch, 9), template(cw, ch), LM, L)
    ctx.set_frames_device(lst, chroma=chroma)
    assert np.array_equal(ctx.download_image(0), ctx.download_image(1)) and np.array_equal(ctx.download_image(0), Y.luma8(yw >> 6))
    ctx.set_sample_image_index([0, 0, 0, 0, 1, 1, 1, 1])
    ctx.set_x(np.concatenate([rows, rows]))
    ctx.align_set_source_frames(lst, chroma=chroma)
    hf = Y.Frame10(Y.Desc(name), yw, uvw.reshape(ch2, cw2, 2))
    for combo, filt in ((("uint8", "nhwc", 3, "rgb"), None), (("float32", "nchw", 3, "bgr"), "area"), (("float16", "nchw", 1, "bgr"), None)):
        spec = spec_of(*combo)
        got = ctx.align_crops_tensor(LM, template(cw, ch), cw, ch, filter=filt, **spec)
        out, mats = got[0].cpu().numpy(), got[1]
        assert np.array_equal(bits(mats[:4]), bits(mats[4:])) and np.array_equal(bits(out[:4]), bits(out[4:]))
        ws = [Y.rigid(hf, mats[r], cw, ch) if filt is None else Y.area(hf, mats[r], cw, ch, int(got[3][r])) for r in range(4)]
        assert any(wn[1].any() for wn in ws)
        compare(got[0][:4], ws, [0, 0, 0, 0], [dict(name=name)], spec)
    restore(ctx)
    del big
