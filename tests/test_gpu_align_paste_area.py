"""The filtered paste on the device (csrc/sdm_align_paste.hip: paste_kernel_t<false, true>; include/sdm.h "Pasting crops back, filtered";
detection_model.paste_crops_tensor(filter="area")).  Every comparison is bit for bit against the host restatement
(tests/paste_area_ref.py) and on the WHOLE destination buffer: the frames, their pitch padding and the 16 guard bytes around each
(tests/paste_cases.py)."""
import ctypes

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import paste_area_cases as D
import paste_area_ref as Q
import paste_cases as C
import paste_ref as P
from test_gpu_align_tensor import IDS, L, LE, LM, MEAN, PARAMS, RE, bits, code, template
from test_gpu_align_paste import on_device
from superviseddescent_amd import (Context, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, detection_model, feather_mask, ibug)

pytestmark = pytest.mark.gpu
f32 = np.float32
# eight rows over the frames of paste_cases.FRAMES: frame 0 (BGR 37 x 29) and frame 1 (RGBA 64 x 48) take several overlapping rows
IDX = [0, 1, 0, 6, 1, 4, 0, 1]


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


def matrices(frames, idx, cw, ch, seed):
    """one minifying matrix per row, the W scales of paste_area_cases in turn: S = 1, 3, 2 on frame 0, S = 2, 16, 3 on frame 1"""
    return np.stack([D.minifying(frames[im], cw, ch, seed + r, 1, D.W_SCALES[r % 5:] + D.W_SCALES[:r % 5])[0] for r, im in enumerate(idx)])


def expect(buf, frames, idx, mats, x, alpha, filt=(Q.AREA, 16, 1.0), **spec):
    """(the restatement on a copy of buf: the rows of every frame in row order, S of every row)"""
    want, S = buf.copy(), []
    for r, im in enumerate(idx):
        a = None if alpha is None else alpha if alpha.ndim == 2 else alpha[r]
        S.append(1 if P.inverse(mats[r])[1] else Q.samples(mats[r], *filt))
        if not P.inverse(mats[r])[1]:
            Q.paste_row(C.view(want, frames[im]), frames[im]["fmt"], mats[r], x[r], a, S[-1], **spec)
    return want, S


def paste_at(ctx, buf, frames, idx, mats, x, alpha, filter="area", **kw):
    import torch
    dev, lst = on_device(buf, frames)
    xd = torch.from_numpy(x).cuda()
    ad = None if alpha is None else torch.from_numpy(alpha).cuda()
    got = ctx.align_paste_tensor_at(mats, xd, lst, image_index=idx, mask=ad, filter=filter, **kw)
    assert np.array_equal(xd.cpu().numpy().view(np.uint8), x.view(np.uint8))                   # the tensor and the opacity are only read
    assert alpha is None or np.array_equal(ad.cpu().numpy(), alpha)
    return dev.cpu().numpy(), got


def test_at_form_overlapping_rows_of_mixed_S(ctx):
    buf, frames = C.place(C.FRAMES, 5)
    seen = set()
    combos = [("uint8", "nhwc", 3, "bgr"), ("float16", "nchw", 3, "rgb"), ("float32", "nhwc", 1, "bgr"), ("float16", "nhwc", 3, "bgr"),
              ("float32", "nchw", 3, "rgb"), ("uint8", "nchw", 1, "rgb")]
    for k, (dtype, layout, channels, order) in enumerate(combos):
        cw, ch = D.CROPS[k % 3]
        mats = matrices(frames, IDX, cw, ch, 700 + 10 * k)
        mats[5] = np.array([[1, 0, np.nan], [0, 1, 0]], f32) if k % 2 else mats[5]
        x = C.tensor(len(IDX), cw, ch, dtype, layout, channels, 40 + k)
        alpha = [None, C.alpha_maps(1, cw, ch, 50 + k)[0], C.alpha_maps(len(IDX), cw, ch, 60 + k, zero_band=True)][k % 3]
        spec = dict(layout=layout, order=order, scale=C.SCALES, bias=C.BIASES, gray_shift=14 if order == "bgr" else 15)
        got, (flags, S) = paste_at(ctx, buf, frames, IDX, mats, x, alpha, **spec)
        want, wS = expect(buf, frames, IDX, mats, x, alpha, channels=channels, **spec)
        assert S.tolist() == wS, (k, S, wS)
        assert flags.tolist() == [P.flags_at(mats[r], cw, ch, frames[im]["w"], frames[im]["h"]) for r, im in enumerate(IDX)]
        assert np.array_equal(got, want), (cw, ch, dtype, layout, channels, order)
        assert (want != buf).sum() > 300
        seen |= set(wS)
    assert seen >= {1, 2, 3, 5, 16}
    # the case cannot pass by accident: in the first pass the three rows of frame 0 have three different S, and pixels under two of them
    mats, x = matrices(frames, IDX, 16, 16, 700), C.tensor(len(IDX), 16, 16, "uint8", "nhwc", 3, 40)
    S = [Q.samples(m) for m in mats]
    cover = sum((Q.paste_row(C.view(buf.copy(), frames[0]), T.BGR, mats[r], x[r], None, S[r], layout="nhwc", order="bgr") > 0).astype(int)
                for r in (0, 2, 6))
    assert len({S[r] for r in (0, 2, 6)}) == 3 and (cover >= 2).sum() > 20


def test_cap_gate_bilinear_and_rows_at_one(ctx):
    buf, frames = C.place(C.FRAMES, 5)
    cw, ch = 33, 20
    mats = matrices(frames, IDX, cw, ch, 800)
    x = C.tensor(len(IDX), cw, ch, "float16", "nchw", 3, 81)
    alpha = C.alpha_maps(len(IDX), cw, ch, 82)
    spec = dict(layout="nchw", order="rgb", scale=C.SCALES, bias=C.BIASES, gray_shift=14)
    for filt in ((Q.AREA, 4, 1.0), (Q.AREA, 16, 2.0)):
        got, (flags, S) = paste_at(ctx, buf, frames, IDX, mats, x, alpha, max_samples=filt[1], min_scale=filt[2], **spec)
        want, wS = expect(buf, frames, IDX, mats, x, alpha, filt, channels=3, **spec)
        assert S.tolist() == wS and np.array_equal(got, want), filt
    # mode BILINEAR, and mode AREA on rows that all take S = 1: the unfiltered call's buffer, byte for byte
    plain, f0 = paste_at(ctx, buf, frames, IDX, mats, x, alpha, filter=None, **spec)
    got, (flags, S) = paste_at(ctx, buf, frames, IDX, mats, x, alpha, filter="bilinear", **spec)
    assert (S == 1).all() and np.array_equal(flags, f0) and np.array_equal(got, plain) and (plain != buf).any()
    big = np.stack([A.similarity(1.3, 10.0 * r - 30, 4 + r, 2 + r).astype(f32) for r in range(len(IDX))])       # magnifying rows
    plain, f0 = paste_at(ctx, buf, frames, IDX, big, x, alpha, filter=None, **spec)
    got, (flags, S) = paste_at(ctx, buf, frames, IDX, big, x, alpha, **spec)
    assert (S == 1).all() and np.array_equal(flags, f0) and np.array_equal(got, plain) and (plain != buf).any()


def test_known_answer_and_checkerboard(ctx):
    import torch
    M, crop, S, want = D.known_answer()
    dst = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(crop[None, :, :, None].copy()).cuda()
    flags, s = ctx.align_paste_tensor_at(M[None], x, [dst], layout="nhwc", order="bgr", filter="area")
    assert s.tolist() == [S] and not flags.any() and np.array_equal(dst.cpu().numpy(), want)
    for theta in (0.0, 0.3):
        M, crop, frame, win = D.checkerboard(theta)
        plain, area = frame.copy(), frame.copy()
        P.paste_row(plain, T.BGR, M, crop[None], None, layout="nchw", channels=1)
        Q.paste_row(area, T.BGR, M, crop[None], None, Q.samples(M), layout="nchw", channels=1)
        x = torch.from_numpy(crop[None, :, :, None].copy()).cuda()
        d0, d1 = torch.from_numpy(frame).cuda(), torch.from_numpy(frame).cuda()
        ctx.align_paste_tensor_at(M[None], x, [d0], layout="nhwc", order="bgr")
        _, s = ctx.align_paste_tensor_at(M[None], x, [d1], layout="nhwc", order="bgr", filter="area")
        got0, got1 = d0.cpu().numpy(), d1.cpu().numpy()
        print("theta", theta, "unfiltered", np.abs(got0[win].astype(int) - 128).max(), "area", np.abs(got1[win].astype(int) - 128).max())
        assert s.tolist() == [4] and np.array_equal(got0, plain) and np.array_equal(got1, area)
        assert np.abs(got0[win].astype(int) - 128).max() > 100 and np.abs(got1[win].astype(int) - 128).max() <= 4


def small_model():
    rng = np.random.default_rng(77)
    R = [rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(f32) for p in PARAMS]
    regs = [LinearRegressor() for _ in PARAMS]
    for reg, r in zip(regs, R):
        reg.x = r
    return detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS), rng


def test_fit_form_behind_detect_batch(built):
    import torch
    model, rng = small_model()
    colour = [rng.integers(0, 256, (48, 131, 3), dtype=np.uint8), rng.integers(0, 256, (29, 37, 3), dtype=np.uint8)]
    dev = [torch.from_numpy(c).cuda() for c in colour]
    model.detect_batch(dev, np.array([[50, 8, 30, 30], [6, 3, 24, 24]]))
    size = 96                                                                # a crop three to four times the face: S about 3
    x, m0, f0 = model.aligned_crops_tensor(size, frames=dev, dtype="uint8")
    y = (255 - x).contiguous()                                               # the "network"
    c = model.optimised_model.ctx
    before = c.get_x()
    for m in (None, feather_mask(size, 12)):
        dst = [torch.from_numpy(cc).cuda() for cc in colour]
        mats, flags, S = model.paste_crops_tensor(y, frames=dst, mask=m, filter="area")
        assert np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0)
        assert S.tolist() == [Q.samples(m0[s]) for s in range(2)] and (S > 1).all(), S
        low = [torch.from_numpy(cc).cuda() for cc in colour]
        fl, s1 = c.align_paste_tensor_at(m0, y, low, mask=m, filter="area")
        again = [torch.from_numpy(cc).cuda() for cc in colour]
        m1, f1, s2 = model.paste_crops_tensor(y, frames=again, mask=m, matrices=m0, filter="area")
        assert np.array_equal(fl, flags) and np.array_equal(f1, flags) and np.array_equal(bits(m1), bits(m0))
        assert np.array_equal(s1, S) and np.array_equal(s2, S)
        for s in range(2):
            want = colour[s].copy()
            Q.paste_row(want, T.BGR, m0[s], y[s].cpu().numpy(), m, int(S[s]))
            assert (want != colour[s]).any()
            for got in (dst, low, again):
                assert np.array_equal(got[s].cpu().numpy(), want), (s, m is None)
        # filter=None is the call as it was: two values, the unfiltered bytes
        plain = [torch.from_numpy(cc).cuda() for cc in colour]
        two = model.paste_crops_tensor(y, frames=plain, mask=m)
        assert len(two) == 2
        for s in range(2):
            want = colour[s].copy()
            P.paste_row(want, T.BGR, m0[s], y[s].cpu().numpy(), m)
            assert np.array_equal(plain[s].cpu().numpy(), want) and not np.array_equal(want, dst[s].cpu().numpy())
    assert np.array_equal(bits(c.get_x()), bits(before))                     # the landmark state is only read
    c.close()


def test_tracker_slots_and_state_stay(built):
    import torch
    from superviseddescent_amd import synth
    from test_gpu_warp import random_model
    model = random_model()
    frames, _, boxes = synth.make_tracks(2, 2, seed=58)
    colour = [np.repeat(frames[1, s][..., None], 3, -1).copy() for s in range(2)]
    ids = np.arange(2)
    tr = model.tracker(2)
    tr.start(ids, boxes[0])
    tr.step(ids, [torch.from_numpy(f).cuda() for f in frames[0]])
    dev = [torch.from_numpy(c).cuda() for c in colour]
    tr.step(ids, dev)
    c = model.optimised_model.ctx
    before = (c.get_x(), tr.get(ids))
    x, m0, f0 = model.aligned_crops_tensor(64, frames=dev, dtype="uint8")
    y = (255 - x).contiguous()
    mats, flags, S = model.paste_crops_tensor(y, frames=dev, filter="area")
    assert np.array_equal(bits(mats), bits(m0)) and S.tolist() == [Q.samples(m0[s]) for s in range(2)]
    for s in range(2):
        want = colour[s].copy()
        if not flags[s] & A.DEGENERATE:
            Q.paste_row(want, T.BGR, m0[s], y[s].cpu().numpy(), None, int(S[s]))
        assert np.array_equal(dev[s].cpu().numpy(), want)
    after = (c.get_x(), tr.get(ids))
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert np.array_equal(bits(before[1][0]), bits(after[1][0])) and np.array_equal(before[1][1], after[1][1])


def test_refusals(ctx):
    import torch
    buf, frames = C.place(C.FRAMES[:4], 5)
    idx = [0, 1, 2, 3]
    w, h = 16, 16
    src, lst = on_device(buf, frames)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(idx)
    t = template(w, h)
    ctx.set_x(K.landmark_rows(K.similarities(frames, idx, w, h, 31), t, LM, L))
    ctx.align_set_source_frames(None)
    x = torch.from_numpy(C.tensor(4, w, h, "float16", "nchw", 3, 32)).cuda()
    amap = torch.from_numpy(C.alpha_maps(1, w, h, 33)[0]).cuda()
    spec = dict(layout="nchw", order="rgb", scale=C.SCALES, bias=C.BIASES)
    dst, dlst = on_device(buf, frames)
    mats, flags, S = ctx.align_paste_tensor(LM, t, x, dlst, mask=amap, filter="area", **spec)
    good = dst.cpu().numpy()
    assert (good != buf).any()

    dst, dlst = on_device(buf, frames)
    lib, hnd = ctx._lib, ctx._h
    idx32, t32, m32 = np.ascontiguousarray(LM, np.int32), np.ascontiguousarray(t), np.ascontiguousarray(mats.reshape(-1, 6))
    ii32 = np.array(idx, np.int32)
    sp = _lib.paste_tensor_spec("float16", "nchw", 3, **{k: v for k, v in spec.items() if k != "layout"})
    pa = _lib.SdmAlignPaste(amap.data_ptr(), 0)
    ok = _lib.align_filter("area")

    def arr(lst_):
        d = _lib.frame_descriptors(lst_, None)
        return (_lib.SdmFrame * len(d))(*[_lib.SdmFrame(ctypes.c_void_p(p), fw, fh, st, f) for p, fw, fh, st, f in d]), len(d)

    fr, nf = arr(dlst)
    p2, fw2, fh2, st2, _ = dlst[2]
    nv12 = arr(dlst[:2] + [(p2, fw2, fh2, st2, "nv12")] + dlst[3:])[0]

    def fit(fl=ok, f=fr, s=sp, x_=x.data_ptr()):
        rc = lib.sdm_align_paste_tensor_filtered(hnd, idx32.ctypes.data, t32.ctypes.data, LM.size, w, h, None if s is None else ctypes.byref(s),
                                                 None if fl is None else ctypes.byref(fl), ctypes.c_void_p(x_), ctypes.byref(pa), f, nf,
                                                 None, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def at(fl=ok, f=fr, s=sp, x_=x.data_ptr()):
        rc = lib.sdm_align_paste_tensor_at_filtered(hnd, m32.ctypes.data, ii32.ctypes.data, 4, w, h, None if s is None else ctypes.byref(s),
                                                    None if fl is None else ctypes.byref(fl), ctypes.c_void_p(x_), ctypes.byref(pa), f, nf,
                                                    None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    F = _lib.SdmAlignFilter
    for call in (fit, at):
        for bad in (dict(fl=None), dict(fl=F(2, 16, 1.0)), dict(fl=F(-1, 16, 1.0)), dict(fl=F(1, 0, 1.0)), dict(fl=F(1, 17, 1.0)),
                    dict(fl=F(1, 16, 0.5)), dict(fl=F(1, 16, float("nan"))), dict(fl=F(1, 16, float("inf"))), dict(fl=F(0, 16, -1.0)),
                    dict(f=nv12), dict(s=None), dict(x_=0)):
            assert code(call, **bad) == -1, bad
    assert np.array_equal(dst.cpu().numpy(), buf)                                   # nothing was launched
    # a valid call behind the refusals, with no output pointer at all, gives what the call gave before them
    fit()
    assert np.array_equal(dst.cpu().numpy(), good)
    dst, dlst = on_device(buf, frames)
    m2, f2, S2 = ctx.align_paste_tensor(LM, t, x, dlst, mask=amap, filter="area", **spec)
    assert np.array_equal(dst.cpu().numpy(), good) and np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
    assert np.array_equal(S2, S)
    ctx.set_sample_image_index(None)
