"""Planar colour frames, 3 x H x W, as the image set and as the crop source (include/sdm.h, "Planar colour frames";
csrc/sdm_frames.hip, csrc/sdm_align_tensor_device.h and the area sums): the converted gray bytes against the formula of
sdm_upload_images_bgr_u8 for every width class, pitch, plane distance and pointer alignment of the conversion kernel; detect and the
tracker against the same pixels given interleaved; the rigid crop, the area crop, the warp and the area warp bit for bit against the
references of the interleaved formats (tests/align_tensor_ref.py, align_area_ref.py, warp_ref.py, warp_area_ref.py) applied to the
interleaved view of the same pixels and to the device's own matrices; the 64-bit plane distance; the refusals."""
import ctypes
import itertools

import numpy as np
import pytest

import align_area_cases as AC
import align_area_ref as AR
import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import planar_cases as PC
import warp_area_cases as WAC
import warp_area_ref as WA
import warp_cases as W
import warp_ref as WR
from oracle import sdm_oracle as orc
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
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
BP, RP = PC.BGR_PLANAR, PC.RGB_PLANAR


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def placed():
    buf, frames = PC.place()
    return buf, frames, [PC.host_frame(buf, f) for f in frames]


def template(w, h):
    return (np.array([[0.2, 0.2], [0.8, 0.25], [0.5, 0.5], [0.3, 0.8], [0.75, 0.7]]) * (w - 1 + 1e-3, h - 1 + 1e-3)).astype(np.float32) + 0.125


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def spec_of(dtype, layout, channels, order):
    return dict(dtype=dtype, layout=layout, channels=channels, order=order, scale=SCALES, bias=BIASES, gray_shift=14 if order == "bgr" else 15)


def gray_of(planes, fmt, shift):
    """the formula of sdm_upload_images_bgr_u8 on the planes (3, h, w) of a planar frame"""
    b, g, r = (planes[0], planes[1], planes[2]) if fmt == BP else (planes[2], planes[1], planes[0])
    wb, wg, wr = T.WEIGHTS[shift]
    return ((b.astype(np.int64) * wb + g.astype(np.int64) * wg + r.astype(np.int64) * wr + (1 << (shift - 1))) >> shift).astype(np.uint8)


# ---- the gray conversion ---------------------------------------------------------------------------------------------------------
# Not checked here: the bytes behind the last pixel of a row of the OWNED gray image (the conversion stores whole 16-byte words; the
# interleaved path leaves zeros there).  No entry point reads them back -- download_image copies width bytes per row, and the pixel
# kernels take the width from the image table --, so no test of the interleaved formats checks them either.  The planar branch of
# frames_to_gray_kernel forms its word as the interleaved one does: it starts as 0 and only pixels k < npx are ORed in.
@pytest.mark.parametrize("shift", [14, 15])
def test_converted_bytes_equal_the_formula(ctx, shift):
    import torch
    plan, at = [], 0
    for w, h, pad, kind, mis, fmt in itertools.product((1, 15, 16, 17, 33, 70), (1, 9), (0, 5), ("default", "odd", "far", "negative"),
                                                       range(4), (BP, RP)):
        stride = w + pad
        gap = h * stride + {"default": 0, "odd": 3, "far": 64, "negative": 0}[kind]
        start = (at + 3) // 4 * 4 + mis                            # the lowest plane starts `mis` bytes behind a 4-byte boundary
        D = -gap if kind == "negative" else gap
        plan.append(dict(fmt=fmt, w=w, h=h, stride=stride, off=start + (2 * gap if kind == "negative" else 0), D=D, kind=kind))
        at = start + 2 * gap + h * stride
    assert len(plan) == 768
    host = np.random.default_rng(50 + shift).integers(0, 256, at + 64, dtype=np.uint8)      # (noise everywhere: pitch padding, gaps)
    big = torch.from_numpy(host).cuda()
    assert big.data_ptr() % 4 == 0
    base = big.data_ptr()
    frames = [(base + f["off"], f["w"], f["h"], f["stride"], PC.NAMES[f["fmt"]]) for f in plan]
    chroma = [None if f["kind"] == "default" else base + f["off"] + f["D"] for f in plan]
    want = [gray_of(PC.planes(host, f), f["fmt"], shift) for f in plan]
    # the formula is the oracle's cvtColor on the interleaved view of the same pixels
    for f, g in list(zip(plan, want))[::97]:
        assert np.array_equal(g, orc.bgr2gray(_bgr(PC.host_frame(host, f)), shift))
    ctx.set_frames_device(frames, gray_shift=shift, chroma=chroma)                         # ONE call: the multi-frame grid
    bad = [(i, {k: plan[i][k] for k in ("fmt", "w", "h", "stride", "D")}) for i in range(len(plan))
           if not np.array_equal(ctx.download_image(i), want[i])]
    assert not bad, bad[:8]
    assert np.array_equal(big.cpu().numpy(), host)                                          # the source is only read
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


def _bgr(frame):
    """B, G, R in this order of an interleaved align_tensor_ref.Frame"""
    return np.ascontiguousarray(frame.pix[..., ::-1] if frame.fmt == T.RGB else frame.pix)


def test_mixed_list_gray_bgr_nv12_planar(ctx, placed):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    rng = np.random.default_rng(3)
    gray = torch.from_numpy(rng.integers(0, 256, (13, 21), dtype=np.uint8)).cuda()
    lst, formats, chroma = PC.device_frames(dev, frames)
    ctx.set_frames_device([gray] + lst, [None] + formats, chroma=[None] + chroma)
    assert np.array_equal(ctx.download_image(0), gray.cpu().numpy())
    for i, (f, hf) in enumerate(zip(frames, host)):
        want = hf.pix if f["fmt"] == T.NV12 else orc.bgr2gray(_bgr(hf), 14)
        assert np.array_equal(ctx.download_image(i + 1), want), (i, f["fmt"], f["kind"])
    assert np.array_equal(dev.cpu().numpy(), buf)
    # the stacked form: one n x 3 x H x W batch (its frames at the default distance), and a channel-sliced view of a 4-plane batch
    batch = torch.from_numpy(rng.integers(0, 256, (3, 4, 9, 17), dtype=np.uint8)).cuda()
    for view in (batch[:, :3], batch[:, 1:]):
        ctx.set_frames_device(view, "rgb_planar", gray_shift=15)
        v = view.cpu().numpy()
        assert all(np.array_equal(ctx.download_image(i), gray_of(v[i], RP, 15)) for i in range(3))
    # one bare 3 x H x W tensor is one frame, with its name alone or in a list of one
    for name in ("bgr_planar", ["bgr_planar"]):
        ctx.set_frames_device(batch[2, 1:], name)
        assert np.array_equal(ctx.download_image(0), gray_of(batch[2, 1:].cpu().numpy(), BP, 14))
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- detect and the tracker ------------------------------------------------------------------------------------------------------
def random_model(ctx=None):
    rng = np.random.default_rng(77)
    regs = []
    for p in PARAMS:
        r = LinearRegressor()
        r.x = rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32)
        regs.append(r)
    return detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def test_detect_and_tracker_equal_the_interleaved_frames(built):
    import torch
    model = random_model()
    tracks, _, boxes = synth.make_tracks(2, 3, seed=31)           # frames x streams x H x W
    rng = np.random.default_rng(8)
    cut = ((slice(0, 200), slice(10, 250)), (slice(20, 256), slice(0, 220)))      # two sizes
    shift = np.array([[10, 0], [0, 20]])

    def colour(t, s):
        g = tracks[t, s][cut[s]]
        c = rng.integers(0, 256, g.shape + (3,), dtype=np.uint8)
        c[..., 1] = g
        return c

    hwc = [[torch.from_numpy(colour(t, s)).cuda() for s in range(2)] for t in range(3)]
    # the planar frames: stream 0 a contiguous 3 x H x W tensor, stream 1 a region of a larger one (pitched, planes further apart)
    def planar(t, s):
        p = hwc[t][s].permute(2, 0, 1)
        if s == 0:
            return p.contiguous()
        big = torch.full((3, p.shape[1] + 7, p.shape[2] + 13), 255, dtype=torch.uint8, device="cuda")
        big[:, 3:3 + p.shape[1], 5:5 + p.shape[2]] = p
        return big[:, 3:3 + p.shape[1], 5:5 + p.shape[2]]

    chw = [[planar(t, s) for s in range(2)] for t in range(3)]
    assert not chw[0][1].is_contiguous()
    b0 = boxes[0].copy()
    b0[:, 0] -= shift[:, 0]
    b0[:, 1] -= shift[:, 1]
    # detect: a handful of faces on the two frames
    bx = np.array([b0[0], b0[1], b0[0] + [6, -4, 0, 0], b0[1] + [-5, 7, 0, 0], b0[0] + [-40, -60, 0, 0]], np.int32)
    idx = np.array([0, 1, 0, 1, 0], np.int32)
    want = model.detect_batch(hwc[0], bx, idx, formats="rgb")
    got = model.detect_batch(chw[0], bx, idx, formats="rgb_planar")
    assert np.isfinite(want).all() and np.array_equal(bits(got), bits(want))
    ids = np.arange(2)
    runs = []
    for frames, fmt in ((chw, "bgr_planar"), (hwc, "bgr")):
        tr = model.tracker(2)
        tr.start(ids, b0)
        out = [tr.step(ids, frames[t], formats=fmt) for t in (1, 2)]
        out.append(tr.get(ids))
        runs.append(out)
    for a, b in zip(*runs):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    assert np.isfinite(runs[0][1][0]).all()


# ---- crops -----------------------------------------------------------------------------------------------------------------------
def install(ctx, dev, frames, idx, x):
    lst, formats, chroma = PC.device_frames(dev, frames)
    ctx.set_frames_device(lst, formats, chroma=chroma)
    ctx.set_sample_image_index(idx)
    ctx.set_x(x)
    ctx.align_set_source_frames(lst, formats, chroma=chroma)
    return lst


def restore(ctx):
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


def compare(got, want_of_row, rows, host, spec):
    got = got.cpu().numpy()
    for r, im in enumerate(rows):
        want = T.finish(*want_of_row[r], **spec)
        assert got[r].dtype == want.dtype and got[r].shape == want.shape
        assert np.array_equal(bits(got[r]), bits(want)), (r, im, host[im].fmt, spec)


def test_rigid_crops_every_combination(ctx, placed):
    """rows over every frame of the set -- planar at every plane distance, the region view, BGR and NV12 in the same list --, among them
    a row wholly outside its frame and a degenerate row"""
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    idx = [5, 3, 1, 0, 2, 4, 6, 7, 0, 1]
    seen = 0
    for (w, h) in K.CROPS:
        x = K.landmark_rows(K.similarities(frames, idx, w, h, 30 + w), template(w, h), LM, L)
        x[8, :L] += 700.0                                          # row 8: wholly outside frame 0
        x[9, LM[2]] = np.nan                                       # row 9: degenerate
        install(ctx, dev, frames, idx, x)
        cache = None
        for combo in COMBOS:
            spec = spec_of(*combo)
            out, mats, flags = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
            assert flags[9] == A.DEGENERATE and np.isnan(mats[9]).all() and flags[8] == A.PARTIAL
            if cache is None:
                cache = []
                for r, im in enumerate(idx[:9]):
                    kind, bgr = T.warped(host[im], mats[r], w, h)
                    cache.append((kind, bgr, T.luma(host[im], mats[r], w, h) if kind == "nv12" else None))
                assert not cache[8][1].any()
                cache.append((cache[8][0], np.zeros_like(cache[8][1]), None))      # degenerate: (0, 0, 0) before scale and bias
            compare(out, cache, idx, host, spec)
            seen |= int(flags.max())
        assert np.array_equal(dev.cpu().numpy(), buf)              # the in-place source is only read
    assert seen & A.PARTIAL
    restore(ctx)


def test_area_crops_every_combination_at_every_s(ctx, placed):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    seen = set()
    for (w, h) in K.CROPS:
        for idx, sims, want_S in AC.mixed_rows(frames, w, h, 70 + w):
            install(ctx, dev, frames, idx, K.landmark_rows(sims, template(w, h), LM, L))
            cache = None
            for combo in COMBOS:
                spec = spec_of(*combo)
                out, mats, flags, samples = ctx.align_crops_tensor(LM, template(w, h), w, h, filter="area", **spec)
                assert list(samples) == want_S
                if cache is None:
                    cache = [AR.warped(host[im], mats[r], w, h, int(samples[r])) for r, im in enumerate(idx)]
                compare(out, cache, idx, host, spec)
            seen |= {(im, S) for im, S in zip(idx, want_S)}
    assert seen == {(im, S) for im in range(len(frames)) for _, S in AC.CLASSES}      # every frame at every S
    assert np.array_equal(dev.cpu().numpy(), buf)
    restore(ctx)


WARP_ROWS = [0, 1, 5, 6, 7, 2, 1]                                  # row -> frame: planar frames, the region view, BGR, NV12, the 5 x 4 frame


@pytest.mark.parametrize("filtered", [False, True])
def test_warps_every_combination(ctx, placed, filtered):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    filt = align_filter("area")
    for (w, h) in W.CROPS:
        idx, t, tri = W.mesh_rcr22(w, h)
        ctx.warp_set_mesh(idx, t, tri, w, h)
        lab = ctx.warp_labels()
        x = WAC.rows_for(frames, WARP_ROWS, idx, t, w, h, WAC.SEED, scales=[0.6, 2.6, 1.7, 4.2, 3.3, 0.9, 2.1]) if filtered else \
            W.rows_for(frames, WARP_ROWS, idx, t, w, h, 40)
        x[5, :L] += 900.0                                          # row 5: wholly outside its frame
        install(ctx, dev, frames, WARP_ROWS, x)
        cache = None
        for combo in COMBOS:
            spec = spec_of(*combo)
            if filtered:
                out, mats, flags, smp = ctx.warp_crops_tensor(filter=filt, **spec)
                want_s = np.stack([WA.samples(m.reshape(-1, 6), bool(f & WR.DEGENERATE), filt.mode, filt.max_samples, filt.min_scale)
                                   for m, f in zip(mats, flags)])
                assert np.array_equal(smp, want_s)
                if cache is None:
                    assert smp.max() > 1
                    cache = [WA.warped(host[im], mats[r].reshape(-1, 6), lab, smp[r]) for r, im in enumerate(WARP_ROWS)]
            else:
                out, mats, flags = ctx.warp_crops_tensor(**spec)
                if cache is None:
                    cache = [WR.warped(host[im], mats[r].reshape(-1, 6), lab) for r, im in enumerate(WARP_ROWS)]
            assert not cache[5][1].any()
            compare(out, cache, WARP_ROWS, host, spec)
        assert np.array_equal(dev.cpu().numpy(), buf)
    restore(ctx)


# ---- the 64-bit plane distance ---------------------------------------------------------------------------------------------------
def test_planes_more_than_2_32_bytes_apart(ctx):
    """one untouched allocation of 2 * (2^32 + 2^26) + 2^20 bytes; only the three planes of a 33 x 21 frame are written"""
    import torch
    D = (1 << 32) + (1 << 26) + 3
    w, h, stride = 33, 21, 40
    big = torch.empty(2 * D + (1 << 20), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(64)
    pl = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    for c in range(3):
        torch.as_strided(big, (h, w), (stride, 1), 5 + c * D).copy_(torch.from_numpy(pl[c]).cuda())
    frame = torch.as_strided(big, (3, h, w), (D, stride, 1), 5)
    host = T.Frame(T.RGB, np.ascontiguousarray(np.transpose(pl, (1, 2, 0))), None)
    f = dict(w=w, h=h)
    cw, ch = 16, 16
    x = K.landmark_rows(K.similarities([f], [0, 0], cw, ch, 9), template(cw, ch), LM, L)
    ctx.set_frames_device([frame], "rgb_planar")
    assert np.array_equal(ctx.download_image(0), gray_of(pl, RP, 14))
    ctx.set_sample_image_index([0, 0])
    ctx.set_x(x)
    ctx.align_set_source_frames([frame], "rgb_planar")
    spec = spec_of("uint8", "nhwc", 3, "rgb")
    out, mats, flags = ctx.align_crops_tensor(LM, template(cw, ch), cw, ch, **spec)
    want = [T.warped(host, mats[r], cw, ch) + (None,) for r in range(2)]
    assert any(wn[1].any() for wn in want)
    compare(out, want, [0, 0], [host], spec)
    # the reversed view of the same memory: data is the highest plane, the second plane D bytes BELOW it
    top = (big.data_ptr() + 5 + 2 * D, w, h, stride, "bgr_planar")
    ctx.align_set_source_frames([top], chroma=[big.data_ptr() + 5 + D])
    out2, m2, _ = ctx.align_crops_tensor(LM, template(cw, ch), cw, ch, **spec)
    assert np.array_equal(bits(m2), bits(mats)) and np.array_equal(out2.cpu().numpy(), out.cpu().numpy())      # (R G B up = B G R down)
    restore(ctx)
    del big


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(ctx, placed):
    import torch
    buf, frames, host = placed
    dev = torch.from_numpy(buf).cuda()
    idx = [0, 1, 5]
    w = h = 7
    x = K.landmark_rows(K.similarities(frames, idx, w, h, 5), template(w, h), LM, L)
    lst = install(ctx, dev, frames, idx, x)
    spec = spec_of("float32", "nchw", 3, "rgb")
    before = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
    images = [ctx.download_image(i) for i in range(len(frames))]
    p = dev.data_ptr() + frames[0]["off"]
    lib = _lib.lib()

    def arr(fs):
        return (_lib.SdmFrame * len(fs))(*[_lib.SdmFrame(*f) for f in fs])

    def planes(ps):
        return (ctypes.c_void_p * len(ps))(*ps)

    ok = (p, 8, 8, 40, BP)
    cases = {
        "image set, D == 0": lambda: lib.sdm_set_frames_device_planes(ctx._h, arr([ok]), planes([p]), 1, 14),
        "image set, stride < width": lambda: lib.sdm_set_frames_device_planes(ctx._h, arr([(p, 8, 8, 7, RP)]), None, 1, 14),
        "image set, stride < width, plain call": lambda: lib.sdm_set_frames_device(ctx._h, arr([ok, (p, 8, 8, 7, BP)]), 2, 14),
        "image set, null data": lambda: lib.sdm_set_frames_device_planes(ctx._h, arr([(None, 8, 8, 8, BP)]), None, 1, 14),
        "image set, short list": lambda: lib.sdm_set_frames_device_planes(ctx._h, arr([ok]), None, 0, 14),
        "image set, null list": lambda: lib.sdm_set_frames_device_planes(ctx._h, None, None, 1, 14),
        "image set, gray_shift": lambda: lib.sdm_set_frames_device_planes(ctx._h, arr([ok]), None, 1, 13),
        "crop source, D == 0": lambda: lib.sdm_align_set_source_frames(ctx._h, arr([ok]), planes([p]), 1),
        "crop source, stride < width": lambda: lib.sdm_align_set_source_frames(ctx._h, arr([ok, (p, 8, 8, 7, RP)]), None, 2),
    }
    for name, fn in cases.items():
        assert fn() == _lib.SDM_ERR_INVALID, name
        after = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(after, before)), name
        assert all(np.array_equal(ctx.download_image(i), im) for i, im in enumerate(images)), name
    # a crop source shorter than the rows' images: refused by the crop call
    ctx.align_set_source_frames(lst[:2], ["bgr_planar", "rgb_planar"])
    with pytest.raises(SdmError) as e:
        ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
    assert e.value.code == _lib.SDM_ERR_INVALID
    # sdm_align_crops, the interleaved u8 form, on a planar list: refused as NV12 is, naming the tensor call
    lst2, formats, chroma = PC.device_frames(dev, frames)
    assert ctx.align_set_source_frames(lst2[:1], formats[:1]) is None
    ctx.set_sample_image_index([0])
    ctx.set_x(x[:1])
    with pytest.raises(SdmError, match="sdm_align_crops_tensor") as e:
        ctx.align_crops(LM, template(w, h), w, h)
    assert e.value.code == _lib.SDM_ERR_INVALID
    out = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
    assert np.array_equal(bits(out[0]), bits(before[0][:1]))
    # Python: D == 0 reaches the library (an expanded plane), and a planar name needs stride(2) == 1
    flat = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda").expand(3, 8, 8)
    with pytest.raises(SdmError):
        ctx.set_frames_device([flat], "bgr_planar")
    with pytest.raises(ValueError):
        ctx.set_frames_device([torch.zeros((3, 8, 16), dtype=torch.uint8, device="cuda")[:, :, ::2]], "bgr_planar")
    assert np.array_equal(dev.cpu().numpy(), buf)
    restore(ctx)
