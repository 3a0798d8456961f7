"""Crop tensors pasted back into NV12 frames on the device (csrc/sdm_align_paste.hip: paste_kernel_t<true, AREA>; include/sdm.h "Pasting crops
back into NV12 frames"; detection_model.paste_crops_tensor on "nv12" frames).  Every comparison is bit for bit against the host
restatement (tests/paste_nv12_ref.py) and on the WHOLE destination buffer: both planes of every frame, their pitch padding and the 16
guard bytes around each plane (tests/paste_nv12_cases.py)."""
import ctypes

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import paste_area_ref as Q
import paste_cases as C
import paste_nv12_cases as V
import paste_nv12_ref as N
import paste_ref as P
from test_gpu_align_tensor import IDS, L, LE, LM, MEAN, PARAMS, RE, bits, code, template
from superviseddescent_amd import (Context, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, detection_model, ibug)

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def calls():
    """the cases and their restatement, computed once: [(case, expected buffer, expected S)]"""
    return [(c,) + V.expect(c) for c in V.calls()]


def on_device(buf, frames):
    """(the buffer on the device, the frame list of the Python layer, the chroma list): views into the one buffer; a UV plane directly
    behind its Y plane is passed as None"""
    import torch
    dev = torch.from_numpy(buf).cuda()
    lst = [(dev.data_ptr() + f["off"], f["w"], f["h"], f["stride"], K.NAMES[f["fmt"]]) for f in frames]
    chroma = [dev.data_ptr() + f["uv_off"] if f["fmt"] == T.NV12 and f["separate"] else None for f in frames]
    return dev, lst, chroma


def filter_args(filt):
    if filt is None:
        return {}
    return dict(filter="area" if filt[0] == Q.AREA else "bilinear", max_samples=filt[1], min_scale=filt[2])


def paste_at(ctx, c, frames=None, idx=None, rows=None, **over):
    import torch
    frames = c["frames"] if frames is None else frames
    rows = list(range(len(c["idx"]))) if rows is None else rows
    dev, lst, chroma = on_device(c["buf"], frames)
    xd = torch.from_numpy(np.ascontiguousarray(c["x"][rows])).cuda()
    alpha = c["alpha"] if c["alpha"] is None or c["alpha"].ndim == 2 else np.ascontiguousarray(c["alpha"][rows])
    ad = None if alpha is None else torch.from_numpy(alpha).cuda()
    kw = dict(filter_args(c["filter"]), **V.spec_of(c))
    kw.update(over)
    if any(f["fmt"] == T.NV12 for f in frames):
        kw.setdefault("chroma", chroma)
    got = ctx.align_paste_tensor_at(c["mats"][rows], xd, lst, image_index=[c["idx"][r] for r in rows] if idx is None else idx, mask=ad, **kw)
    return dev.cpu().numpy(), got


def test_at_form_both_planes_bit_equal(ctx, calls):
    seen = set()
    for k, (c, want, wS) in enumerate(calls):
        got, res = paste_at(ctx, c)
        flags, S = (res, None) if c["filter"] is None else res
        what = (k, c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"], c["filter"])
        assert flags.tolist() == [P.flags_at(c["mats"][r], c["cw"], c["ch"], c["frames"][im]["w"], c["frames"][im]["h"])
                                  for r, im in enumerate(c["idx"])], what
        assert S is None or S.tolist() == wS, what
        for f in c["frames"]:                                                  # plane by plane first: a failure names its frame
            if f["fmt"] == T.NV12:
                for a, b in zip(V.planes(got, f), V.planes(want, f)):
                    assert np.array_equal(a, b), (what, f["w"], f["h"])
        assert np.array_equal(got, want), what                                 # ... then padding, guards and the other formats
        assert (want != c["buf"]).sum() > 2000
        if c["channels"] == 1:                                                 # the UV plane is neither read nor written
            for f in c["frames"][:V.NV12_FRAMES]:
                assert np.array_equal(V.planes(got, f)[1], V.planes(c["buf"], f)[1])
        seen |= set(wS)
    assert seen >= {1, 2, 3}


def test_bilinear_filter_equals_null_filter(ctx, calls):
    c = calls[0][0]
    assert c["filter"] is None
    got, flags = paste_at(ctx, c)
    same, (f2, S) = paste_at(ctx, c, filter="bilinear")
    assert np.array_equal(got, same) and np.array_equal(got, calls[0][1]) and np.array_equal(flags, f2) and (S == 1).all()


def test_other_formats_in_the_list_and_twins_on_bgr_frames(ctx, calls):
    """the BGR and the GRAY frame of the mixed list hold what the existing calls write on them alone; matrices / flags / S are those of the
    existing calls on BGR frames of the NV12 frames' sizes"""
    for k in (1, 3):
        c, want, wS = calls[k]
        mixed, (flags, S) = paste_at(ctx, c)
        rows = [r for r, im in enumerate(c["idx"]) if im >= V.NV12_FRAMES]
        others = c["frames"][V.NV12_FRAMES:]
        alone, (fl, s1) = paste_at(ctx, c, frames=others, idx=[c["idx"][r] - V.NV12_FRAMES for r in rows], rows=rows)
        for f in others:
            assert np.array_equal(C.view(mixed, f), C.view(alone, f)) and (C.view(alone, f) != C.view(c["buf"], f)).any()
        assert np.array_equal(fl, flags[rows]) and np.array_equal(s1, S[rows])
        buf2, placed = C.place([(f["w"], f["h"], T.BGR) for f in c["frames"]], 3)
        _, (f3, s3) = paste_at(ctx, dict(c, buf=buf2), frames=placed)
        assert np.array_equal(f3, flags) and np.array_equal(s3, S)


def test_fit_form_on_nv12_context_frames(ctx, calls):
    import torch
    c = calls[3][0]                                                            # float16 NHWC BGR, "area", no opacity map
    frames, idx, w, h = c["frames"], c["idx"], c["cw"], c["ch"]
    src, lst, chroma = on_device(c["buf"], frames)
    ctx.set_frames_device(lst)                                                 # an NV12 frame is its own luma
    ctx.set_sample_image_index(idx)
    t = template(w, h)
    sims = [np.where(np.isfinite(m), m, 1.0) if P.inverse(m)[1] else m for m in c["mats"]]
    ctx.set_x(K.landmark_rows(sims, t, LM, L))
    ctx.align_set_source_frames(None)
    xd, ad = torch.from_numpy(c["x"]).cuda(), None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
    kw = dict(filter_args(c["filter"]), **V.spec_of(c))
    dst, dlst, dchroma = on_device(c["buf"], frames)
    mats, flags, S = ctx.align_paste_tensor(LM, t, xd, dlst, mask=ad, chroma=dchroma, **kw)
    got = dst.cpu().numpy()
    fitted = dict(c, mats=mats)
    want, wS = V.expect(fitted)
    assert S.tolist() == wS and np.array_equal(got, want) and (want != c["buf"]).sum() > 2000
    at, (f_at, s_at) = paste_at(ctx, fitted)
    assert np.array_equal(at, got) and np.array_equal(s_at, S)
    assert np.array_equal(flags & A.DEGENERATE, f_at & A.DEGENERATE)
    # the same fit, flags and S as the filtered call on BGR twins of the frames
    buf2, twins = C.place([(f["w"], f["h"], T.BGR) for f in frames], 3)
    d2 = torch.from_numpy(buf2).cuda()
    l2 = [(d2.data_ptr() + f["off"], f["w"], f["h"], f["stride"], "bgr") for f in twins]
    m2, f2, s2 = ctx.align_paste_tensor(LM, t, xd, l2, mask=ad, **kw)
    assert np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags) and np.array_equal(s2, S)
    assert np.array_equal(src.cpu().numpy(), c["buf"])                        # the context's frames are only read
    ctx.set_sample_image_index(None)


def test_refusals(ctx, calls):
    import torch
    c = calls[1][0]
    frames, idx, w, h = c["frames"], c["idx"], c["cw"], c["ch"]
    src, lst, _ = on_device(c["buf"], frames)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(idx)
    t = template(w, h)
    ctx.set_x(K.landmark_rows([np.where(np.isfinite(m), m, 1.0) if P.inverse(m)[1] else m for m in c["mats"]], t, LM, L))
    ctx.align_set_source_frames(None)
    x, amap = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["alpha"]).cuda()
    kw = dict(filter_args(c["filter"]), **V.spec_of(c))
    dst, dlst, dchroma = on_device(c["buf"], frames)
    mats, flags, S = ctx.align_paste_tensor(LM, t, x, dlst, mask=amap, chroma=dchroma, **kw)
    good = dst.cpu().numpy()
    assert (good != c["buf"]).any()

    dst, dlst, dchroma = on_device(c["buf"], frames)
    lib, hnd = ctx._lib, ctx._h
    idx32, t32, m32 = np.ascontiguousarray(LM, np.int32), np.ascontiguousarray(t), np.ascontiguousarray(mats.reshape(-1, 6))
    ii32 = np.array(idx, np.int32)
    sp = _lib.paste_tensor_spec(c["dtype"], c["layout"], c["channels"], **{k: v for k, v in V.spec_of(c).items() if k != "layout"})
    pa = _lib.SdmAlignPaste(amap.data_ptr(), 0)
    ok = _lib.align_filter("area")
    uv = (ctypes.c_void_p * len(dlst))(*dchroma)

    def arr(lst_):
        d = _lib.frame_descriptors(lst_, None)
        return (_lib.SdmFrame * len(d))(*[_lib.SdmFrame(ctypes.c_void_p(p), fw, fh, st, f) for p, fw, fh, st, f in d]), len(d)

    fr, nf = arr(dlst)

    def with_frame(i, **kw_):
        p, fw, fh, st, fmt = dlst[i]
        e = dict(p=p, w=fw, h=fh, stride=st, fmt=fmt)
        e.update(kw_)
        return arr(dlst[:i] + [(e["p"], e["w"], e["h"], e["stride"], e["fmt"])] + dlst[i + 1:])[0]

    def fit(fl=ok, f=fr, s=sp, x_=x.data_ptr(), p=pa, n=nf):
        rc = lib.sdm_align_paste_tensor_nv12(hnd, idx32.ctypes.data, t32.ctypes.data, LM.size, w, h, None if s is None else ctypes.byref(s),
                                             None if fl is None else ctypes.byref(fl), ctypes.c_void_p(x_),
                                             None if p is None else ctypes.byref(p), f, uv, n, None, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def at(fl=ok, f=fr, s=sp, x_=x.data_ptr(), p=pa, n=nf, ii=ii32, n_rows=len(idx)):
        rc = lib.sdm_align_paste_tensor_at_nv12(hnd, m32.ctypes.data, ii.ctypes.data, n_rows, w, h, None if s is None else ctypes.byref(s),
                                                None if fl is None else ctypes.byref(fl), ctypes.c_void_p(x_),
                                                None if p is None else ctypes.byref(p), f, uv, n, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    F = _lib.SdmAlignFilter
    for call in (fit, at):
        for bad in (dict(fl=F(2, 16, 1.0)), dict(fl=F(-1, 16, 1.0)), dict(fl=F(1, 0, 1.0)), dict(fl=F(1, 17, 1.0)), dict(fl=F(1, 16, 0.5)),
                    dict(fl=F(1, 16, float("nan"))), dict(fl=F(1, 16, float("inf"))), dict(fl=F(0, 16, -1.0)),
                    dict(s=None), dict(x_=0), dict(x_=x.data_ptr() + 8), dict(p=None), dict(p=_lib.SdmAlignPaste(amap.data_ptr(), 2)),
                    dict(f=None), dict(n=0), dict(n=len(dlst) - 1),
                    dict(f=with_frame(0, p=0)), dict(f=with_frame(1, w=0)), dict(f=with_frame(1, h=0)), dict(f=with_frame(2, fmt=6)),
                    dict(f=with_frame(0, stride=36)),                                             # below the luma row of 37 bytes
                    dict(f=with_frame(0, stride=37)),                                             # the luma fits, 19 UV pairs do not
                    dict(f=with_frame(7, stride=37 * 3 - 1))):
            assert code(call, **bad) == -1, bad
    assert code(fit, f=with_frame(1, w=63)) == -1 and code(fit, f=with_frame(0, h=30, stride=200)) == -1      # the size rule
    assert code(at, ii=np.array([len(dlst)] * len(idx), np.int32)) == -1 and code(at, n_rows=0) == -1
    assert np.array_equal(dst.cpu().numpy(), c["buf"])                              # nothing was launched
    # the existing entry points keep refusing an NV12 frame
    for name, args in (("sdm_align_paste_tensor_at", ()), ("sdm_align_paste_tensor_at_filtered", (ctypes.byref(ok),))):
        tail = (None,) if not args else (None, None)
        rc = getattr(lib, name)(hnd, m32.ctypes.data, ii32.ctypes.data, len(idx), w, h, ctypes.byref(sp), *args, ctypes.c_void_p(x.data_ptr()),
                                ctypes.byref(pa), fr, nf, *tail)
        assert rc == -1
    assert np.array_equal(dst.cpu().numpy(), c["buf"])
    # a valid call behind the refusals, with no output pointer at all, gives what the call gave before them
    fit()
    assert np.array_equal(dst.cpu().numpy(), good)
    dst, dlst, dchroma = on_device(c["buf"], frames)
    m2, f2, S2 = ctx.align_paste_tensor(LM, t, x, dlst, mask=amap, chroma=dchroma, **kw)
    assert np.array_equal(dst.cpu().numpy(), good) and np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
    assert np.array_equal(S2, S)
    ctx.set_sample_image_index(None)


def small_model():
    rng = np.random.default_rng(77)
    R = [rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(f32) for p in PARAMS]
    regs = [LinearRegressor() for _ in PARAMS]
    for reg, r in zip(regs, R):
        reg.x = r
    return detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS), rng


def nv12_surface(rng, w, h, smooth):
    """an NV12 surface as one uint8 buffer, the UV plane directly behind Y at pitch w + 3 (noise in the padding).  smooth: ramps inside
    the limited range and the BGR gamut -- what a resampling reproduces, so that a round trip's deviation is the conversion pair's"""
    stride = 2 * ((w + 1) // 2) + 3
    rows = h + (h + 1) // 2
    buf = rng.integers(0, 256, rows * stride, dtype=np.uint8)
    f = dict(fmt=T.NV12, w=w, h=h, stride=stride, off=0, uv_off=h * stride, separate=False)
    if smooth:
        Y, UV = V.planes(buf, f)
        yy, xx = np.mgrid[:h, :w]
        Y[...] = 40 + (0.6 * xx + 0.9 * yy).astype(int)
        cy, cx = np.mgrid[:(h + 1) // 2, :(w + 1) // 2]
        UV[..., 0] = 112 + cx // 4
        UV[..., 1] = 140 - cy // 2
    return buf, f


def test_detection_model_pastes_into_the_frames_it_detected_on_and_round_trip(built):
    """detect on NV12 surfaces, cut the crops from them, paste the "network's" output back into them; then the round trip: the crops
    themselves pasted back at full opacity give the bytes of the restatement's own round trip, whose deviation from the surface is a
    property of the integer conversion pair (printed; DESIGN 4.20 records it)"""
    import torch
    model, rng = small_model()
    surf = [nv12_surface(rng, 161, 97, True), nv12_surface(rng, 97, 81, True)]             # odd sizes; the faces well inside
    dev = [torch.from_numpy(b).cuda() for b, _ in surf]
    lst = [(d.data_ptr(), f["w"], f["h"], f["stride"], "nv12") for d, (_, f) in zip(dev, surf)]
    model.detect_batch(lst, np.array([[64, 32, 30, 30], [36, 28, 24, 24]]))
    x, m0, f0 = model.aligned_crops_tensor(16, frames=lst, dtype="uint8")
    assert tuple(x.shape) == (2, 3, 16, 16) and not (f0 & A.DEGENERATE).any()
    c = model.optimised_model.ctx
    before = c.get_x()
    xh = x.cpu().numpy()
    for s, (b, f) in enumerate(surf):                                          # the crops are the restatement's: the round trip below is its own
        Y0, UV0 = V.planes(b, f)
        assert np.array_equal(xh[s], T.tensor(T.Frame(T.NV12, Y0.copy(), UV0.copy()), m0[s], 16, 16, dtype="uint8", layout="nchw", channels=3,
                                              order="rgb"))
    for name, y in (("inverted", (255 - x).contiguous()), ("round trip", x)):
        yh = y.cpu().numpy()
        dst = [torch.from_numpy(b).cuda() for b, _ in surf]
        dl = [(d.data_ptr(), f["w"], f["h"], f["stride"], "nv12") for d, (_, f) in zip(dst, surf)]
        mats, flags = model.paste_crops_tensor(y, frames=dl)
        assert np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0)
        again = [torch.from_numpy(b).cuda() for b, _ in surf]
        al = [(d.data_ptr(), f["w"], f["h"], f["stride"], "nv12") for d, (_, f) in zip(again, surf)]
        m1, f1, s1 = model.paste_crops_tensor(y, frames=al, matrices=m0, filter="area", chroma=[None, None])
        assert np.array_equal(f1, flags) and s1.tolist() == [Q.samples(m0[s]) for s in range(2)]
        for s, (b, f) in enumerate(surf):
            want = b.copy()
            Y, UV = V.planes(want, f)
            a = N.paste_row(Y, UV, m0[s], yh[s], None, 1)
            assert (want != b).any() or name == "round trip"
            assert np.array_equal(dst[s].cpu().numpy(), want), (name, s)
            if int(s1[s]) == 1:
                assert np.array_equal(again[s].cpu().numpy(), want), (name, s)
            if name == "round trip":
                Y0, UV0 = V.planes(b, f)
                full = a == 255
                whole = N.blocks(full.astype(np.int64)) == 4
                dy = int(np.abs(Y.astype(int) - Y0)[full].max())
                duv = int(np.abs(UV.astype(int) - UV0)[whole].max())
                print("round trip, surface", s, "flags", int(f0[s]), "scale", float(np.hypot(m0[s][0, 0], m0[s][1, 0])), ": luma deviates by at most", dy,
                      "chroma by at most", duv, "over", int(full.sum()), "pixels and", int(whole.sum()), "samples at full opacity")
                assert full.sum() > 20
    assert np.array_equal(bits(c.get_x()), bits(before))                     # the landmark state is only read
    c.close()
