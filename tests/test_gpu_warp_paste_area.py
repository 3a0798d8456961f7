"""The filtered piecewise-affine paste on the device (csrc/sdm_warp_paste.hip: warp_paste_kernel_t<true, true>; include/sdm.h "Pasting warped
faces back, filtered"; Context.warp_paste_tensor[_at](filter=...), detection_model.paste_warped_tensor(filter=...)).  Every comparison is
bit for bit against the host restatement (tests/warp_paste_area_ref.py) and on the WHOLE destination buffer: every frame and plane, their
pitch padding and the 16 guard bytes around each (tests/warp_paste_area_cases.py); the geometry case on a window around every row inside
the buffer of tests/test_gpu_frame_geometry.py, and then on the whole buffer for stray stores."""
import ctypes

import numpy as np
import pytest

import align_tensor_ref as T
import frame_geometry_cases as G
import paste_nv12_cases as V
import warp_cases as WC
import warp_paste_area_cases as M
import warp_paste_area_ref as WA
import warp_paste_ref as WP
from test_gpu_align_paste_nv12 import on_device, small_model
from test_gpu_frame_geometry import big, bind, model, views_of  # noqa: F401
from test_gpu_frame_geometry_paste import checked
from test_gpu_warp import L, LE, PARAMS, RE, bits, code
from superviseddescent_amd import Context, SdmError, _lib, synth

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
    """the cases and their restatement, computed once: [(case, expected buffer, per-row results, counts)]"""
    return [(c,) + M.expect(c) for c in M.calls()]


def set_mesh(ctx, c):
    ctx.warp_set_mesh(c["lm"], c["t"], c["tri"], c["cw"], c["ch"])
    assert np.array_equal(ctx.warp_labels(), c["lab"])


def rows_x(c):
    """the points as N x 2L landmark rows"""
    x = np.zeros((len(c["idx"]), 2 * L), f32)
    x[:, c["lm"]], x[:, L + c["lm"]] = c["pts"][..., 0], c["pts"][..., 1]
    return x


def filter_args(filt):
    return dict(filter="area" if filt[0] == WA.AREA else "bilinear", max_samples=filt[1], min_scale=filt[2])


def paste_at(ctx, c, filt="case", **over):
    """the _at form on a fresh copy of the case's buffer: (the buffer afterwards, what the call returned).  filt None: the unfiltered
    call, with the chroma list only where the list holds an NV12 frame"""
    import torch
    dev, lst, chroma = on_device(c["buf"], c["frames"])
    xd = torch.from_numpy(np.ascontiguousarray(c["x"])).cuda()
    ad = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
    kw = dict(M.spec_of(c))
    filt = c["filter"] if filt == "case" else filt
    if filt is not None:
        kw.update(filter_args(filt))
    if any(f["fmt"] == T.NV12 for f in c["frames"]):
        kw["chroma"] = chroma
    kw.update(over)
    got = ctx.warp_paste_tensor_at(c["pts"], xd, lst, image_index=c["idx"], mask=ad, **kw)
    return dev.cpu().numpy(), got


def compare(c, got, want, what):
    for i, f in enumerate(c["frames"]):                                        # frame by frame first: a failure names its frame
        for a, b in zip(M.owned(c, got, f), M.owned(c, want, f)):
            assert np.array_equal(a, b), (what, i, f["fmt"], f["w"], f["h"], int((a != b).sum()))
    assert np.array_equal(got, want), what                                     # ... then the guards between the frames


@pytest.mark.parametrize("k", range(12))
def test_at_form_bit_equal_three_meshes(ctx, calls, k):
    c, want, res, cnt = calls[k]
    what = (k, c["mesh"], c["list"], c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"], c["filter"])
    set_mesh(ctx, c)
    got, (flags, samples) = paste_at(ctx, c)
    assert np.array_equal(flags, M.flags(c)), what
    assert samples.shape == cnt.shape and np.array_equal(samples, cnt), what
    compare(c, got, want, what)
    assert (want != c["buf"]).sum() > 2000 and (cnt > 1).any()
    # the hull's border is antialiased from the inside; pixels zeroed by the 2^20 rule are left alone
    assert sum(int((o[5] & (o[1] > 0)).sum()) for o in res.values()) > 100 and sum(int((o[4] & o[3]).sum()) for o in res.values()) > 0
    if c["channels"] == 1 and c["list"] == "nv12":                             # the UV plane is neither read nor written
        for f in c["frames"][:V.NV12_FRAMES]:
            assert np.array_equal(V.planes(got, f)[1], V.planes(c["buf"], f)[1])


@pytest.mark.parametrize("channels", (3, 1))
def test_mixed_list_in_one_call(ctx, channels):
    """a BGR frame, a GRAY frame at an odd pitch and an NV12 surface with its UV plane apart in ONE call, under a shared opacity map with a
    zero band; a 1-channel tensor leaves the UV plane alone"""
    c = M.mixed(channels)
    set_mesh(ctx, c)
    want, res, cnt = M.expect(c)
    got, (flags, samples) = paste_at(ctx, c)
    assert np.array_equal(flags, M.flags(c)) and np.array_equal(samples, cnt)
    compare(c, got, want, ("mixed", channels))
    for f in c["frames"]:
        assert any((a != b).any() for a, b in zip(M.owned(c, want, f)[:1], M.owned(c, c["buf"], f)[:1]))
    uv = V.planes(got, c["frames"][2])[1]
    assert np.array_equal(uv, V.planes(c["buf"], c["frames"][2])[1]) == (channels == 1)


@pytest.mark.parametrize("k", (0, 3, 5, 10))
def test_mode_bilinear_writes_the_unfiltered_bytes(ctx, calls, k):
    c = calls[k][0]
    set_mesh(ctx, c)
    plain, f0 = paste_at(ctx, c, filt=None)
    got, (f1, samples) = paste_at(ctx, c, filt=(WA.BILINEAR, 16, 1.0))
    assert np.array_equal(got, plain) and (plain != c["buf"]).sum() > 1000
    assert np.array_equal(f0, f1) and (samples == 1).all()


@pytest.mark.parametrize("k", (1, 6))
def test_magnifying_placements_write_the_unfiltered_bytes_under_area(ctx, calls, k):
    c = M.magnified(calls[k][0])
    set_mesh(ctx, c)
    assert (M.counts(c, filt=(WA.AREA, 16, 1.0)) == 1).all()
    plain, f0 = paste_at(ctx, c, filt=None)
    got, (f1, samples) = paste_at(ctx, c, filt=(WA.AREA, 16, 1.0))
    assert np.array_equal(got, plain) and (plain != c["buf"]).sum() > 1000
    assert np.array_equal(f0, f1) and (samples == 1).all()


@pytest.mark.parametrize("name", ("pixel", "nv12"))
def test_eight_overlapping_rows_of_different_counts(ctx, name):
    """eight rows over one another on ONE frame, their largest counts between 3 and 16: the bytes are those of the restatement's row
    order whatever order the workgroups ran in; the same rows given in reverse order give other bytes; guards and pitch padding stay"""
    c = M.stacked(name)
    set_mesh(ctx, c)
    want, res, cnt = M.expect(c)
    assert len({int(cnt[r].max()) for r in range(8)}) >= 5
    covered = np.sum([res[r][3] for r in range(8)], 0)
    assert (covered >= 6).sum() > 50
    got, (flags, samples) = paste_at(ctx, c)
    assert np.array_equal(samples, cnt)
    compare(c, got, want, name)
    order = list(range(7, -1, -1))
    d = dict(c, pts=c["pts"][order], x=np.ascontiguousarray(c["x"][order]), alpha=np.ascontiguousarray(c["alpha"][order]))
    rev, _, _ = M.expect(d)
    got2, _ = paste_at(ctx, d)
    compare(d, got2, rev, name + " reversed")
    assert not np.array_equal(rev, want)


@pytest.mark.parametrize("k", (2, 7, 9))
def test_fit_form_equals_the_at_form(ctx, calls, k):
    import torch
    c, want, res, cnt = calls[k]
    set_mesh(ctx, c)
    src, lst, chroma = on_device(c["buf"], c["frames"])
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(c["idx"])
    ctx.set_x(rows_x(c))
    xd = torch.from_numpy(c["x"]).cuda()
    ad = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
    dst, dlst, dchroma = on_device(c["buf"], c["frames"])
    kw = dict(M.spec_of(c), **filter_args(c["filter"]))
    if c["list"] == "nv12":
        kw["chroma"] = dchroma
    mats, flags, samples = ctx.warp_paste_tensor(xd, dlst, mask=ad, **kw)
    got_at, (f_at, s_at) = paste_at(ctx, c)
    assert np.array_equal(flags, f_at) and np.array_equal(samples, s_at) and np.array_equal(samples, cnt)
    finite = np.isfinite(c["pts"]).all((1, 2))
    assert np.array_equal(bits(mats.reshape(len(c["idx"]), -1, 6)[finite]), bits(M.matrices(c)[finite]))
    assert np.array_equal(dst.cpu().numpy(), got_at)
    compare(c, got_at, want, ("fit", k))
    assert np.array_equal(src.cpu().numpy(), c["buf"])                        # the context's frames are only read
    ctx.set_sample_image_index(None)


def test_refusals(ctx, calls):
    import torch
    c, want, res, cnt = calls[4]
    assert c["list"] == "nv12"
    set_mesh(ctx, c)
    frames, idx = c["frames"], c["idx"]
    src, lst, chroma = on_device(c["buf"], frames)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(idx)
    ctx.set_x(rows_x(c))
    x = torch.from_numpy(c["x"]).cuda()
    amap = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
    dst, dlst, dchroma = on_device(c["buf"], frames)
    lib, hnd = ctx._lib, ctx._h
    pts, ii32 = np.ascontiguousarray(c["pts"], f32), np.array(idx, np.int32)
    opts = {k: v for k, v in M.spec_of(c).items() if k != "layout"}
    sp = _lib.paste_tensor_spec(c["dtype"], c["layout"], c["channels"], **opts)
    pa = _lib.SdmAlignPaste(None if amap is None else amap.data_ptr(), int(amap is not None and amap.dim() == 3))
    uv = (ctypes.c_void_p * len(dlst))(*dchroma)
    fl = _lib.SdmAlignFilter(*c["filter"])

    def arr(lst_):
        d = _lib.frame_descriptors(lst_, None)
        return (_lib.SdmFrame * len(d))(*[_lib.SdmFrame(ctypes.c_void_p(p), fw, fh, st, f) for p, fw, fh, st, f in d]), len(d)

    fr, nf = arr(dlst)

    def with_frame(i, **kw_):
        p, fw, fh, st, fmt = dlst[i]
        e = dict(p=p, w=fw, h=fh, stride=st, fmt=fmt)
        e.update(kw_)
        return arr(dlst[:i] + [(e["p"], e["w"], e["h"], e["stride"], e["fmt"])] + dlst[i + 1:])[0]

    def fit(f=fr, s=sp, x_=x.data_ptr(), p=pa, n=nf, handle=hnd, flt=fl, u=uv):
        rc = lib.sdm_warp_paste_tensor_filtered(handle, None if s is None else ctypes.byref(s), None if flt is None else ctypes.byref(flt),
                                                ctypes.c_void_p(x_), None if p is None else ctypes.byref(p), f, u, n, None, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def at(f=fr, s=sp, x_=x.data_ptr(), p=pa, n=nf, ii=ii32, n_rows=len(idx), points=pts, handle=hnd, flt=fl, u=uv):
        rc = lib.sdm_warp_paste_tensor_at_filtered(handle, None if points is None else points.ctypes.data, ii.ctypes.data, n_rows,
                                                   None if s is None else ctypes.byref(s), None if flt is None else ctypes.byref(flt),
                                                   ctypes.c_void_p(x_), None if p is None else ctypes.byref(p), f, u, n, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def bad_spec(**kw):
        s = _lib.paste_tensor_spec(c["dtype"], c["layout"], c["channels"], **opts)
        for k_, v in kw.items():
            setattr(s, k_, v)
        return s

    def refused(call, **bad):
        """the call is refused and has launched nothing; the same form's good call right behind it, on a fresh copy of the buffer,
        gives the bytes it gave before"""
        assert code(call, **bad) == -1, bad
        assert np.array_equal(dst.cpu().numpy(), c["buf"]), bad
        scratch, slst, schroma = on_device(c["buf"], frames)
        call(f=arr(slst)[0], u=(ctypes.c_void_p * len(slst))(*schroma))
        assert np.array_equal(scratch.cpu().numpy(), want), ("the call behind the refusal", bad)

    bgr = next(i for i, f in enumerate(frames) if f["fmt"] == T.BGR)
    for call in (fit, at):
        for bad in (dict(s=None), dict(s=bad_spec(dtype=3)), dict(s=bad_spec(channels=2)), dict(s=bad_spec(gray_shift=13)),
                    dict(x_=0), dict(x_=x.data_ptr() + 8), dict(p=None), dict(p=_lib.SdmAlignPaste(x.data_ptr(), 2)),
                    dict(f=None), dict(n=0), dict(n=len(dlst) - 1),
                    dict(f=with_frame(0, p=0)), dict(f=with_frame(1, w=0)), dict(f=with_frame(1, h=0)), dict(f=with_frame(2, fmt=6)),
                    dict(f=with_frame(0, stride=36)),                                             # below the luma row of 37 bytes
                    dict(f=with_frame(0, stride=37)),                                             # the luma fits, 19 UV pairs do not
                    dict(f=with_frame(bgr, stride=37 * 3 - 1)),
                    # the filter
                    dict(flt=None), dict(flt=_lib.SdmAlignFilter(2, 16, 1.0)), dict(flt=_lib.SdmAlignFilter(-1, 16, 1.0)),
                    dict(flt=_lib.SdmAlignFilter(1, 0, 1.0)), dict(flt=_lib.SdmAlignFilter(1, 17, 1.0)),
                    dict(flt=_lib.SdmAlignFilter(1, 16, 0.5)), dict(flt=_lib.SdmAlignFilter(1, 16, float("nan"))),
                    dict(flt=_lib.SdmAlignFilter(1, 16, float("inf")))):
            refused(call, **bad)
    refused(fit, f=with_frame(1, w=63))                                                           # the fit form's size rule
    for bad in (dict(ii=np.array([len(dlst)] * len(idx), np.int32)), dict(n_rows=0), dict(points=None)):
        refused(at, **bad)
    fresh = Context(0)                                                              # no mesh; no rows
    try:
        fresh.set_model_geometry(L, RE, LE, PARAMS)
        refused(at, handle=fresh._h)
        refused(fit, handle=fresh._h)
        fresh.warp_set_mesh(c["lm"], c["t"], c["tri"], c["cw"], c["ch"])
        refused(fit, handle=fresh._h)
    finally:
        fresh.close()
    # the buffer the refusals were aimed at is still as it was; a valid call on it, with no output pointer at all, gives the same bytes
    at()
    compare(c, dst.cpu().numpy(), want, "behind the refusals")
    ctx.set_sample_image_index(None)


def test_detection_model_behind_tracker_step_and_detect_batch(built):
    """detection_model.paste_warped_tensor(filter="area") on the tracker's and on detect_batch's rows, with and without points=: the
    restatement's bytes from the device's own matrices' points, the counts, and the landmark state only read"""
    import torch
    model_, rng = small_model()
    frames, _, boxes = synth.make_tracks(2, 2, seed=58)
    ids = np.arange(2)
    tr = model_.tracker(2)
    tr.start(ids, boxes[0])
    c = model_.optimised_model.ctx
    w, h = 224, 200                                                            # larger than the faces: the way back minifies
    _, t, tri = WC.mesh_rcr22(w, h)
    y = torch.from_numpy(rng.integers(0, 256, (2, 1, h, w), dtype=np.uint8)).cuda()
    yh = y.cpu().numpy()

    def check(what):
        before = c.get_x()
        dst = [torch.from_numpy(f.copy()).cuda() for f in frames[1]]
        mats, flags, samples = model_.paste_warped_tensor(y, frames=dst, filter="area")
        pts, lab = model_.warp_points(), c.warp_labels()
        again = [torch.from_numpy(f.copy()).cuda() for f in frames[1]]
        none, f1, s1 = model_.paste_warped_tensor(y, frames=again, points=pts, filter="area")
        assert none is None and np.array_equal(f1, flags) and np.array_equal(s1, samples)
        capped = model_.paste_warped_tensor(y, frames=[torch.from_numpy(f.copy()).cuda() for f in frames[1]], filter="area", max_samples=1)
        assert (capped[2] == 1).all()
        assert samples.shape == (2, len(tri), 2) and (samples > 1).any(), what
        for s in range(2):
            m = WP.matrices(pts[s], t, tri)[0]
            assert np.array_equal(bits(mats[s].reshape(-1, 6)), bits(m))
            cnt = WA.counts(pts[s], tri, m, 256, 256)
            assert np.array_equal(samples[s], cnt), (what, s)
            want = frames[1][s].copy()
            WA.paste_row(want[..., None], T.GRAY, pts[s], tri, m, lab, yh[s], None, cnt, channels=1)
            assert (want != frames[1][s]).sum() > 1000
            assert np.array_equal(dst[s].cpu().numpy(), want), (what, s)
            assert np.array_equal(again[s].cpu().numpy(), want), (what, s)
        assert np.array_equal(bits(c.get_x()), bits(before))

    for step in range(2):
        tr.step(ids, [torch.from_numpy(f).cuda() for f in frames[step]])
    check("tracker")
    model_.detect_batch(list(frames[1]), boxes[1])
    c = model_.optimised_model.ctx
    check("detect_batch")
    c.close()


# ---- frame geometry: a luma row more than 2^24 bytes into its plane, an odd surface --------------------------------------------------
def geometry_case():
    cw, ch = 66, 40
    c = G.paste_case(70, "7", "nv12", [G.NV12_ODD], [0] * 5, [(47, 40), (3, 4), (93, 77), (92, 20), (30, 77)], cw, ch,
                     "left right top bottom", None, scales=[1.7, 2.6, 4.5, 1.3, 0.8])
    c["points"] = G.mesh_points(c["mats"], cw, ch, 4070)
    return c


def geometry_reference(c, pixels):
    """the restatement on copies of the planes, every row on a window of whole 2 x 2 blocks around it"""
    want = [tuple(p.copy() for p in q) for q in pixels]
    idx, t, tri, lab = G.mesh(c["cw"], c["ch"])
    mats = WP.matrices(c["points"], t, tri)
    f = c["frames"][0]
    cnt = np.stack([WA.counts(c["points"][r], tri, mats[r], f["w"], f["h"]) for r in range(5)])
    changed = far = last = 0
    for r in range(5):
        x0, y0, x1, y1 = G.paste_window(f, c["points"][r], True)
        alpha = None if c["alpha"] is None else c["alpha"] if c["alpha"].ndim == 2 else c["alpha"][r]
        Y, UV = want[0][0][y0:y1, x0:x1], want[0][1][y0 // 2:(y1 + 1) // 2, x0 // 2:(x1 + 1) // 2]
        q, a, tmap, foot, refused, hull, written = WA.paste_row_nv12(Y, UV, c["points"][r], tri, mats[r], lab, c["x"][r], alpha, cnt[r],
                                                                     channels=3, origin=(x0, y0), **G.paste_spec(c))
        touched = foot | (a > 0)
        for edge, is_frame_edge in ((touched[:, 0], x0 == 0), (touched[:, -1], x1 == f["w"]), (touched[0], y0 == 0), (touched[-1], y1 == f["h"])):
            assert is_frame_edge or not edge.any(), ("the footprint touches the window's edge", r)
        changed += int((a > 0).sum())
        far += int(((a > 0).any(1) & ((np.arange(y0, y1) * f["pitch"]) > 2 ** 24)).sum())
        if x1 == f["w"] and y1 == f["h"]:
            last += int((a[-1] > 0).sum()) + int((a[:, -1] > 0).sum())
    return want, cnt, changed, far, last


def test_frame_geometry(model, big):
    import torch
    c = geometry_case()
    pixels = G.paste_pixels(c)
    want, cnt, changed, far, last = geometry_reference(c, pixels)
    # luma rows more than 2^24 bytes into their plane; pixels of the frame's last row and column; triangles at (1, 1) and well above
    assert changed > 500 and far > 10 and last > 4 and cnt.max() >= 4 and (cnt == 1).all(-1).any(), (changed, far, last, cnt.max())
    idx, t, tri, lab = G.mesh(c["cw"], c["ch"])
    f = c["frames"][0]
    wc = bind(model)
    frames, ppix = G.paste_placement(c, pixels)
    with checked(big, frames, ppix):
        base = big.data_ptr()
        lst = [(base + g["off"], g["w"], g["h"], g["pitch"], g["fmt"]) for g in c["frames"]]
        chroma = [base + g["uv_off"] if "uv_off" in g else None for g in c["frames"]]
        wc.warp_set_mesh(idx, t, tri, c["cw"], c["ch"])
        y = torch.from_numpy(c["x"]).cuda()
        mask = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
        flags, samples = wc.warp_paste_tensor_at(c["points"], y, lst, image_index=c["idx"], mask=mask, chroma=chroma, filter="area",
                                                 **G.paste_spec(c))
        wc.synchronize()
        assert np.array_equal(flags, WP.flags(c["points"], t, tri, [(f["w"], f["h"])] * 5)) and np.array_equal(samples, cnt)
        wframes, wpix = G.paste_placement(c, want)
        for i, (g, w) in enumerate(zip(wframes, wpix)):
            for plane, (v, a) in enumerate(zip(views_of(big, g), w if isinstance(w, tuple) else (w,))):
                got = v.cpu().numpy()
                assert np.array_equal(got, a), ("frame %d plane %d" % (i, plane), "%d bytes differ" % int((got != a).sum()))
