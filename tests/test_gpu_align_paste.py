"""Crop tensors pasted back into frames on the device (csrc/sdm_align_paste.hip, include/sdm.h "Pasting crops back",
detection_model.paste_crops_tensor).  Every comparison is bit for bit against the host restatement (tests/paste_ref.py) and on the WHOLE
destination buffer: the frames, their pitch padding and the 16 guard bytes around each (tests/paste_cases.py)."""
import ctypes

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import paste_cases as C
import paste_ref as P
from test_gpu_align_tensor import COMBOS, IDS, L, LE, LM, MEAN, PARAMS, RE, bits, code, template
from superviseddescent_amd import (Context, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, detection_model, feather_mask, ibug)

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


def on_device(buf, frames):
    """(the buffer on the device, the frame list of the Python layer): views into the one buffer"""
    import torch
    dev = torch.from_numpy(buf).cuda()
    return dev, [(dev.data_ptr() + f["off"], f["w"], f["h"], f["stride"], K.NAMES[f["fmt"]]) for f in frames]


def expect(buf, frames, idx, mats, x, alpha, **spec):
    """the restatement on a copy of buf: the rows of every frame in row order"""
    want = buf.copy()
    for r, im in enumerate(idx):
        a = None if alpha is None else alpha if alpha.ndim == 2 else alpha[r]
        P.paste_row(C.view(want, frames[im]), frames[im]["fmt"], mats[r], x[r], a, **spec)
    return want


def paste_at(ctx, buf, frames, idx, mats, x, alpha, **spec):
    import torch
    dev, lst = on_device(buf, frames)
    flags = ctx.align_paste_tensor_at(mats, torch.from_numpy(x).cuda(), lst, image_index=idx, mask=alpha, **spec)
    return dev.cpu().numpy(), flags


def test_integer_translation_identity(ctx):
    """cut with M = [1 0 tx; 0 1 ty], pasted with that M and no opacity map into a zeroed frame: the source rectangle, nothing else"""
    import torch
    t = np.array([[2, 2], [12, 3], [7, 8], [4, 12], [10, 10]], f32)          # both coordinate sums are 35: the fit's means are exact
    w, h, tx, ty = 16, 14, 5, 3
    specs = [(24, 20, fmt) for fmt in (T.GRAY, T.BGR, T.RGB, T.BGRA, T.RGBA)]
    buf, frames = C.place(specs, 3)
    dev, lst = on_device(buf, frames)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(None)
    ctx.set_x(K.landmark_rows([A.similarity(1, 0, tx, ty)] * 5, t, LM, L))
    ctx.align_set_source_frames(lst)
    M = np.array([[1, 0, tx], [0, 1, ty]], f32)
    for channels in (3, 1):
        rows = list(range(5)) if channels == 3 else [0]                        # (one channel: the gray frame)
        crops, mats, flags = ctx.align_crops_tensor(LM, t, w, h, dtype="uint8", layout="nhwc", channels=channels, order="bgr")
        assert all(np.array_equal(mats[r], M) for r in range(5)) and not flags.any()          # (as values: the fit's -b / d is -0.0)
        zero = np.zeros_like(buf)
        dst, dlst = on_device(zero, frames)
        f2 = ctx.align_paste_tensor_at(mats[rows], crops[rows].contiguous(), dlst, image_index=rows, layout="nhwc", order="bgr")
        assert not f2.any()
        want = zero.copy()
        for r in rows:
            src, out = C.view(buf, frames[r]), C.view(want, frames[r])
            out[ty:ty + h, tx:tx + w, :min(3, src.shape[2])] = src[ty:ty + h, tx:tx + w, :3]
        assert want.any() and np.array_equal(dst.cpu().numpy(), want)
    ctx.align_set_source_frames(None)


def test_ragged_frame_list_all_formats_in_one_call(ctx):
    buf, frames = C.place(C.FRAMES, 5)
    idx = [0, 1, 2, 3, 4, 5, 6, 1]
    seen, formats = 0, {frames[i]["fmt"] for i in idx}
    assert formats == {T.GRAY, T.BGR, T.RGB, T.BGRA, T.RGBA}
    for (w, h) in K.CROPS:
        mats = np.stack([S.astype(f32) for S in K.similarities(frames, idx, w, h, 30 + w)])
        for k, (dtype, layout, channels, order) in enumerate(COMBOS):
            x = C.tensor(len(idx), w, h, dtype, layout, channels, 40 + k)
            alpha = C.alpha_maps(len(idx), w, h, 50 + k) if k % 2 else None
            spec = dict(layout=layout, order=order, scale=C.SCALES, bias=C.BIASES, gray_shift=14 if order == "bgr" else 15)
            got, flags = paste_at(ctx, buf, frames, idx, mats, x, alpha, **spec)
            want = expect(buf, frames, idx, mats, x, alpha, channels=channels, **spec)
            assert np.array_equal(got, want), (w, h, dtype, layout, channels, order)
            assert flags.tolist() == [P.flags_at(mats[r], w, h, frames[im]["w"], frames[im]["h"]) for r, im in enumerate(idx)]
            assert (want != buf).sum() > 500
            seen |= int(flags.max())
    assert seen == A.PARTIAL


def test_overlapping_rows_paste_in_row_order(ctx):
    buf, frames = C.place([(37, 29, T.BGR)], 7)
    w = h = 16
    mats = np.stack([A.similarity(1.2, a, 9 + 2 * r, 4 + r).astype(f32) for r, a in enumerate((10.0, -20.0, 35.0))])
    idx = [0, 0, 0]
    x = C.tensor(3, w, h, "float16", "nchw", 3, 8)
    alpha = C.alpha_maps(3, w, h, 9)
    spec = dict(layout="nchw", order="rgb", scale=C.SCALES, bias=C.BIASES, gray_shift=14)
    # the case cannot pass by accident: a pixel under all three rows with 0 < a < 255, and the reverse order gives other bytes
    probe = buf.copy()
    res = P.paste(C.view(probe, frames[0]), T.BGR, [(mats[r], x[r], alpha[r]) for r in range(3)], channels=3, **spec)
    assert np.logical_and.reduce([foot & (a > 0) & (a < 255) for foot, a in res]).any()
    want = expect(buf, frames, idx, mats, x, alpha, channels=3, **spec)
    back = expect(buf, frames, idx, mats[::-1], x[::-1], alpha[::-1], channels=3, **spec)
    assert np.array_equal(probe, want) and not np.array_equal(want, back)
    got, flags = paste_at(ctx, buf, frames, idx, mats, x, alpha, **spec)
    assert np.array_equal(got, want)
    # the rows of one frame need not be neighbours in the call
    buf2, frames2 = C.place([(37, 29, T.BGR), (33, 21, T.GRAY)], 7)
    idx2, m2 = [0, 1, 0, 1, 0], np.stack([mats[0], mats[1], mats[1], mats[0], mats[2]])
    x2, a2 = C.tensor(5, w, h, "float32", "nhwc", 3, 10), C.alpha_maps(5, w, h, 11)
    spec2 = dict(layout="nhwc", order="bgr", scale=C.SCALES, bias=C.BIASES, gray_shift=15)
    got, _ = paste_at(ctx, buf2, frames2, idx2, m2, x2, a2, **spec2)
    assert np.array_equal(got, expect(buf2, frames2, idx2, m2, x2, a2, channels=3, **spec2))


def test_shared_null_and_per_row_opacity(ctx):
    buf, frames = C.place([(37, 29, T.RGBA), (64, 48, T.GRAY)], 12)
    idx = [0, 1, 1]
    w, h = 7, 7
    mats = np.stack([S.astype(f32) for S in K.similarities(frames, idx, w, h, 13)])
    mats[0] = A.similarity(3.0, 0.0, 6.0, 4.0).astype(f32)                    # row 0 magnified, inside its frame
    x = C.tensor(3, w, h, "uint8", "nhwc", 3, 14)
    spec = dict(layout="nhwc", order="rgb", gray_shift=14)
    results = {}
    for name, alpha in (("null", None), ("shared", C.alpha_maps(1, w, h, 15)[0]), ("rows", C.alpha_maps(3, w, h, 16, zero_band=True))):
        got, _ = paste_at(ctx, buf, frames, idx, mats, x, alpha, **spec)
        assert np.array_equal(got, expect(buf, frames, idx, mats, x, alpha, channels=3, **spec)), name
        results[name] = got
    assert not np.array_equal(results["null"], results["shared"]) and not np.array_equal(results["shared"], results["rows"])
    # where a row's map is zero the old bytes stay: pixels of row 0's footprint that the NULL map changes and the banded map does not
    px = lambda b: C.view(b, frames[0])[..., :3].astype(int)
    kept = (px(results["rows"]) == px(buf)).all(-1) & (px(results["null"]) != px(buf)).any(-1)
    assert kept.sum() > 50
    assert np.array_equal(C.view(results["null"], frames[0])[..., 3], C.view(buf, frames[0])[..., 3])       # alpha bytes stay


def test_fit_form(ctx):
    import torch
    buf, frames = C.place(C.FRAMES, 5)
    idx = [0, 1, 6, 4, 1, 0]
    w, h = 16, 16
    src, lst = on_device(buf, frames)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(idx)
    t = template(w, h)
    rows = K.landmark_rows(K.similarities(frames, idx, w, h, 21), t, LM, L)
    rows[3, LM[1]] = np.nan                                                  # a DEGENERATE row
    ctx.set_x(rows)
    ctx.align_set_source_frames(lst)
    _, m0, f0 = ctx.align_crops_tensor(LM, t, w, h, dtype="uint8", layout="nhwc", channels=3)
    x = C.tensor(len(idx), w, h, "float16", "nchw", 3, 22)
    alpha = feather_mask(w, 3)
    spec = dict(layout="nchw", order="rgb", scale=C.SCALES, bias=C.BIASES, gray_shift=14)
    dst, dlst = on_device(buf, frames)
    mats, flags = ctx.align_paste_tensor(LM, t, torch.from_numpy(x).cuda(), dlst, mask=alpha, **spec)
    assert np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0)
    assert flags[3] == A.DEGENERATE and np.isnan(mats[3]).all() and (flags[[0, 1, 2, 4, 5]] & A.DEGENERATE == 0).all()
    assert (flags & A.PARTIAL).any()
    got = dst.cpu().numpy()
    at, f_at = paste_at(ctx, buf, frames, idx, mats, x, alpha, **spec)
    assert np.array_equal(got, at) and np.array_equal(f_at, flags)
    assert np.array_equal(got, expect(buf, frames, idx, mats, x, alpha, channels=3, **spec))
    # the degenerate row pastes nothing: frame 4 (BGRA 131 x 7) is its alone; a PARTIAL row pastes its inside part
    assert np.array_equal(C.view(got, frames[4]), C.view(buf, frames[4]))
    part = int(np.nonzero(flags & A.PARTIAL)[0][0])
    alone = expect(buf, frames, [idx[part]], mats[part:part + 1], x[part:part + 1], alpha, channels=3, **spec)
    assert (alone != buf).any()
    assert np.array_equal(src.cpu().numpy(), buf)                             # the context's frames and the crop source are only read
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


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
    mats, flags = ctx.align_paste_tensor(LM, t, x, dlst, mask=amap, **spec)
    good = dst.cpu().numpy()
    assert (good != buf).any()

    dst, dlst = on_device(buf, frames)
    lib, hnd = ctx._lib, ctx._h
    idx32, t32, m32 = np.ascontiguousarray(LM, np.int32), np.ascontiguousarray(t), np.ascontiguousarray(mats.reshape(-1, 6))
    ii32 = np.array(idx, np.int32)
    sp = _lib.paste_tensor_spec("float16", "nchw", 3, **{k: v for k, v in spec.items() if k != "layout"})
    pa = _lib.SdmAlignPaste(amap.data_ptr(), 0)
    mis = torch.zeros(4 * 3 * w * h + 4, dtype=torch.float16, device="cuda")[4:]                       # 8 bytes off

    def arr(lst_):
        d = _lib.frame_descriptors(lst_, None)
        return (_lib.SdmFrame * len(d))(*[_lib.SdmFrame(ctypes.c_void_p(p), fw, fh, st, f) for p, fw, fh, st, f in d]), len(d)

    fr, nf = arr(dlst)

    def fit(lm=idx32, tm=t32, k=LM.size, cw=w, chh=h, s=sp, x_=x.data_ptr(), p=pa, f=fr, n=nf):
        rc = lib.sdm_align_paste_tensor(hnd, None if lm is None else lm.ctypes.data, tm.ctypes.data, k, cw, chh, None if s is None else ctypes.byref(s),
                                        ctypes.c_void_p(x_), None if p is None else ctypes.byref(p), f, n, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def at(m=m32, ii=ii32, n_rows=4, cw=w, chh=h, s=sp, x_=x.data_ptr(), p=pa, f=fr, n=nf):
        rc = lib.sdm_align_paste_tensor_at(hnd, None if m is None else m.ctypes.data, None if ii is None else ii.ctypes.data, n_rows, cw, chh,
                                           None if s is None else ctypes.byref(s), ctypes.c_void_p(x_), None if p is None else ctypes.byref(p),
                                           f, n, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def S(**kw):
        s = _lib.paste_tensor_spec("float16", "nchw", 3, "rgb", **{k: v for k, v in dict(spec, **kw).items() if k in ("scale", "bias")})
        for k, v in kw.items():
            if k not in ("scale", "bias"):
                setattr(s, k, v)
        return s

    def with_frame(i, **kw):
        """the frame list with entry i changed"""
        p, fw, fh, st, fmt = dlst[i]
        e = dict(p=p, w=fw, h=fh, stride=st, fmt=fmt)
        e.update(kw)
        return arr(dlst[:i] + [(e["p"], e["w"], e["h"], e["stride"], e["fmt"])] + dlst[i + 1:])[0]

    both = []
    for call in (fit, at):
        both += [
            lambda call=call: call(s=None), lambda call=call: call(s=S(dtype=3)), lambda call=call: call(s=S(layout=2)),
            lambda call=call: call(s=S(order=2)), lambda call=call: call(s=S(channels=2)), lambda call=call: call(s=S(gray_shift=13)),
            lambda call=call: call(s=S(scale=[1, np.nan, 1])), lambda call=call: call(s=S(bias=[0, 0, np.inf])),
            lambda call=call: call(x_=0), lambda call=call: call(x_=mis.data_ptr()),                         # in_dev NULL, misaligned
            lambda call=call: call(p=None), lambda call=call: call(p=_lib.SdmAlignPaste(amap.data_ptr(), 2)),
            lambda call=call: call(p=_lib.SdmAlignPaste(amap.data_ptr(), -1)),
            lambda call=call: call(f=None), lambda call=call: call(n=0), lambda call=call: call(n=-1),
            lambda call=call: call(n=3),                                                                # row 3's image index is outside
            lambda call=call: call(f=with_frame(0, p=0)), lambda call=call: call(f=with_frame(1, w=0)), lambda call=call: call(f=with_frame(1, h=0)),
            lambda call=call: call(f=with_frame(0, stride=37 * 3 - 1)), lambda call=call: call(f=with_frame(1, stride=64 * 4 - 1)),
            lambda call=call: call(f=with_frame(2, fmt=6)), lambda call=call: call(f=with_frame(2, fmt=-1)),
            lambda call=call: call(f=with_frame(2, fmt="nv12")),                                         # an NV12 destination
            lambda call=call: call(cw=0), lambda call=call: call(chh=1025),
        ]
    cases = both + [
        # the fit form: what sdm_align_crops_tensor refuses of the landmarks and the template, and the size rule
        lambda: fit(k=1), lambda: fit(k=L + 1), lambda: fit(lm=None), lambda: fit(lm=np.array([3, 3, 9, 12, 15], np.int32)),
        lambda: fit(lm=np.array([3, L, 9, 12, 15], np.int32)), lambda: fit(tm=np.full_like(t32, 2.0)),
        lambda: fit(tm=np.where(np.arange(5)[:, None] == 1, np.nan, t32).astype(f32)),
        lambda: fit(f=with_frame(1, w=63)), lambda: fit(f=with_frame(0, h=30, stride=200)),
        # the _at form
        lambda: at(m=None), lambda: at(n_rows=0), lambda: at(n_rows=-2), lambda: at(ii=np.array([0, 1, 2, 4], np.int32)),
        lambda: at(ii=np.array([0, -1, 2, 3], np.int32)), lambda: at(ii=None, n=3),
    ]
    for f in cases:
        assert code(f) == -1
    assert np.array_equal(dst.cpu().numpy(), buf)                                   # nothing was launched
    fresh = Context(0)
    try:
        assert code(fresh.align_paste_tensor, LM, t, x, dlst, **spec) == -1         # no geometry, no rows
        fl = fresh.align_paste_tensor_at(mats, x, dlst, image_index=idx, mask=amap, **spec)      # the _at form needs neither
        assert np.array_equal(fl, flags) and np.array_equal(dst.cpu().numpy(), good)
    finally:
        fresh.close()
    # a valid call behind the refusals gives what it gave before them
    dst, dlst = on_device(buf, frames)
    m2, f2 = ctx.align_paste_tensor(LM, t, x, dlst, mask=amap, **spec)
    assert np.array_equal(dst.cpu().numpy(), good) and np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
    ctx.set_sample_image_index(None)


def test_detection_model_paste_crops_tensor(built):
    import torch
    rng = np.random.default_rng(77)
    R = [rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(f32) for p in PARAMS]
    regs = [LinearRegressor() for _ in PARAMS]
    for reg, r in zip(regs, R):
        reg.x = r
    model = detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    colour = [rng.integers(0, 256, (48, 131, 3), dtype=np.uint8), rng.integers(0, 256, (29, 37, 3), dtype=np.uint8)]
    dev = [torch.from_numpy(c).cuda() for c in colour]
    model.detect_batch(dev, np.array([[50, 8, 30, 30], [6, 3, 24, 24]]))
    x, m0, f0 = model.aligned_crops_tensor(16, frames=dev, dtype="uint8")
    assert tuple(x.shape) == (2, 3, 16, 16)
    y = (255 - x).contiguous()                                               # the "network"
    c = model.optimised_model.ctx
    mask = feather_mask(16, 4)
    for m in (None, mask):
        dst = [torch.from_numpy(cc).cuda() for cc in colour]
        mats, flags = model.paste_crops_tensor(y, frames=dst, mask=m)
        assert np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0)
        low = [torch.from_numpy(cc).cuda() for cc in colour]
        fl = c.align_paste_tensor_at(m0, y, low, mask=m)
        again = [torch.from_numpy(cc).cuda() for cc in colour]
        m1, _ = model.paste_crops_tensor(y, frames=again, mask=m, matrices=m0)
        assert np.array_equal(fl, flags) and np.array_equal(bits(m1), bits(m0))
        for s in range(2):
            want = colour[s].copy()
            P.paste_row(want, T.BGR, m0[s], y[s].cpu().numpy(), m)
            assert (want != colour[s]).any()
            for got in (dst, low, again):
                assert np.array_equal(got[s].cpu().numpy(), want), (s, m is None)
    c.close()
