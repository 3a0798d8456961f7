"""Warped face tensors pasted back into NV12 frames on the device (csrc/sdm_warp_paste.hip: warp_paste_kernel_t<true, false>; include/sdm.h
"Pasting warped faces back into NV12 frames"; detection_model.paste_warped_tensor on "nv12" frames).  Every comparison is bit for bit
against the host restatement (tests/warp_paste_nv12_ref.py) and on the WHOLE destination buffer: both planes of every frame, their
pitch padding and the 16 guard bytes around each plane (tests/warp_paste_nv12_cases.py); the two geometry cases on a window around
every row inside the 4.5 GiB buffer of tests/test_gpu_frame_geometry.py, and then on the whole buffer for stray stores."""
import ctypes

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import frame_geometry_cases as G
import paste_cases as C
import paste_nv12_cases as V
import paste_nv12_ref as N
import warp_cases as WC
import warp_paste_nv12_cases as M
import warp_paste_nv12_ref as WN
import warp_paste_ref as WP
import warp_ref as R
from test_gpu_align_paste_nv12 import nv12_surface, on_device, small_model
from test_gpu_frame_geometry import big, bind, model, views_of  # noqa: F401
from test_gpu_frame_geometry_paste import checked
from test_gpu_warp import L, LE, PARAMS, RE, bits, code
from superviseddescent_amd import Context, SdmError, _lib

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
    """the cases and their restatement, computed once: [(case, expected buffer, per-row results)]"""
    return [(c,) + M.expect(c) for c in M.calls()]


def set_mesh(ctx, c):
    ctx.warp_set_mesh(c["lm"], c["t"], c["tri"], c["cw"], c["ch"])
    assert np.array_equal(ctx.warp_labels(), c["lab"])


def rows_x(c):
    """the points as N x 2L landmark rows"""
    x = np.zeros((len(c["idx"]), 2 * L), f32)
    x[:, c["lm"]], x[:, L + c["lm"]] = c["pts"][..., 0], c["pts"][..., 1]
    return x


def paste_at(ctx, c, frames=None, idx=None, rows=None, old=False, **over):
    import torch
    frames = c["frames"] if frames is None else frames
    rows = list(range(len(c["idx"]))) if rows is None else rows
    dev, lst, chroma = on_device(c["buf"], frames)
    xd = torch.from_numpy(np.ascontiguousarray(c["x"][rows])).cuda()
    alpha = c["alpha"] if c["alpha"] is None or c["alpha"].ndim == 2 else np.ascontiguousarray(c["alpha"][rows])
    ad = None if alpha is None else torch.from_numpy(alpha).cuda()
    kw = dict(M.spec_of(c))
    kw.update(over)
    if not old:
        kw.setdefault("chroma", chroma)
    flags = ctx.warp_paste_tensor_at(c["pts"][rows], xd, lst, image_index=[c["idx"][r] for r in rows] if idx is None else idx, mask=ad, **kw)
    return dev.cpu().numpy(), flags


def compare(c, got, want, what):
    for f in c["frames"]:                                                      # plane by plane first: a failure names its frame
        if f["fmt"] == T.NV12:
            for name, a, b in zip("Y UV".split(), V.planes(got, f), V.planes(want, f)):
                assert np.array_equal(a, b), (what, f["w"], f["h"], name, int((a != b).sum()))
    assert np.array_equal(got, want), what                                     # ... then padding, guards and the other formats


@pytest.mark.parametrize("k", range(6))
def test_at_form_both_planes_bit_equal(ctx, calls, k):
    c, want, res = calls[k]
    what = (k, c["mesh"], c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"])
    set_mesh(ctx, c)
    got, flags = paste_at(ctx, c)
    assert np.array_equal(flags, M.flags(c)), what
    compare(c, got, want, what)
    assert (want != c["buf"]).sum() > 2000
    if c["channels"] == 1:                                                     # the UV plane is neither read nor written
        for f in c["frames"][:M.NV12_FRAMES]:
            assert np.array_equal(V.planes(got, f)[1], V.planes(c["buf"], f)[1])


def test_chroma_behind_y_and_apart(ctx, calls):
    """chroma=None: every UV plane directly behind its Y plane -- a buffer laid out so; and the planes apart through chroma="""
    import torch
    c, _, _ = calls[1]
    set_mesh(ctx, c)
    specs = [(w, h, fmt, False) for w, h, fmt, _ in V.FRAMES]
    buf, frames = V.place(specs, 12)
    d = dict(c, buf=buf, frames=frames)
    want, _ = M.expect(d)
    dev, lst, chroma = on_device(buf, frames)
    assert chroma == [None] * len(frames)
    xd, ad = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["alpha"]).cuda()
    flags = ctx.warp_paste_tensor_at(c["pts"], xd, lst, image_index=c["idx"], mask=ad, **M.spec_of(c))      # (no chroma at all: "nv12" in the list)
    compare(d, dev.cpu().numpy(), want, "behind Y")
    assert np.array_equal(flags, M.flags(c))
    specs = [(w, h, fmt, True) for w, h, fmt, _ in V.FRAMES]
    buf, frames = V.place(specs, 13)
    d = dict(c, buf=buf, frames=frames)
    want, _ = M.expect(d)
    got, _ = paste_at(ctx, d)
    compare(d, got, want, "apart")


def test_other_formats_in_the_list_equal_the_existing_call(ctx, calls):
    """the BGR and the GRAY frame of the mixed list hold what sdm_warp_paste_tensor_at writes on them alone, byte for byte; the flags are
    those of the existing call on BGR frames of the NV12 frames' sizes"""
    for k in (0, 3, 5):
        c, want, _ = calls[k]
        set_mesh(ctx, c)
        mixed, flags = paste_at(ctx, c)
        rows = [r for r, im in enumerate(c["idx"]) if im >= M.NV12_FRAMES]
        others = c["frames"][M.NV12_FRAMES:]
        alone, fl = paste_at(ctx, c, frames=others, idx=[c["idx"][r] - M.NV12_FRAMES for r in rows], rows=rows, old=True)
        for f in others:
            assert np.array_equal(C.view(mixed, f), C.view(alone, f)) and (C.view(alone, f) != C.view(c["buf"], f)).any()
        assert np.array_equal(fl, flags[rows])
        buf2, twins = C.place([(f["w"], f["h"], T.BGR) for f in c["frames"]], 3)
        _, f3 = paste_at(ctx, dict(c, buf=buf2), frames=twins, old=True)
        assert np.array_equal(f3, flags)


@pytest.mark.parametrize("k", range(6))
def test_fit_form_on_nv12_context_frames(ctx, calls, k):
    """the current rows on NV12 frames that are the context's images and its crop source: the A_t bits of sdm_warp_crops_tensor, the
    bytes of the restatement and of the _at form"""
    import torch
    c, want, _ = calls[k]
    set_mesh(ctx, c)
    src, lst, chroma = on_device(c["buf"], c["frames"])
    ctx.set_frames_device(lst)                                                 # an NV12 frame is its own luma
    ctx.set_sample_image_index(c["idx"])
    ctx.set_x(rows_x(c))
    ctx.align_set_source_frames(lst, chroma=chroma)
    _, m0, f0 = ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=3)
    xd = torch.from_numpy(c["x"]).cuda()
    ad = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
    dst, dlst, dchroma = on_device(c["buf"], c["frames"])
    mats, flags = ctx.warp_paste_tensor(xd, dlst, mask=ad, chroma=dchroma, **M.spec_of(c))
    assert np.array_equal(bits(mats), bits(m0))
    assert np.array_equal(flags, M.flags(c)) and np.array_equal(flags & ~R.PARTIAL, f0 & ~R.PARTIAL)
    finite = np.isfinite(c["pts"]).all((1, 2))
    assert np.array_equal(bits(mats.reshape(len(c["idx"]), -1, 6)[finite]), bits(M.matrices(c)[finite]))
    got = dst.cpu().numpy()
    compare(c, got, want, ("fit", k))
    assert np.array_equal(src.cpu().numpy(), c["buf"])                        # the context's frames are only read
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def test_rows_in_reverse_order_give_other_bytes(ctx, calls):
    c, want, _ = calls[0]
    set_mesh(ctx, c)
    order = list(range(len(c["idx"]) - 1, -1, -1))
    d = dict(c, pts=c["pts"][order], idx=[c["idx"][r] for r in order], x=np.ascontiguousarray(c["x"][order]),
             alpha=c["alpha"] if c["alpha"] is None or c["alpha"].ndim == 2 else np.ascontiguousarray(c["alpha"][order]))
    rev, _ = M.expect(d)
    got, _ = paste_at(ctx, d)
    compare(d, got, rev, "reversed")
    f = c["frames"][0]
    assert not np.array_equal(V.planes(rev, f)[0], V.planes(want, f)[0]) and not np.array_equal(V.planes(rev, f)[1], V.planes(want, f)[1])


def test_refusals(ctx, calls):
    import torch
    c, want, _ = calls[1]
    set_mesh(ctx, c)
    frames, idx = c["frames"], c["idx"]
    src, lst, chroma = on_device(c["buf"], frames)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(idx)
    ctx.set_x(rows_x(c))
    ctx.align_set_source_frames(lst, chroma=chroma)
    x, amap = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["alpha"]).cuda()
    dst, dlst, dchroma = on_device(c["buf"], frames)
    lib, hnd = ctx._lib, ctx._h
    pts, ii32 = np.ascontiguousarray(c["pts"], f32), np.array(idx, np.int32)
    sp = _lib.paste_tensor_spec(c["dtype"], c["layout"], c["channels"], **{k: v for k, v in M.spec_of(c).items() if k != "layout"})
    pa = _lib.SdmAlignPaste(amap.data_ptr(), 0)
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

    def fit(f=fr, s=sp, x_=x.data_ptr(), p=pa, n=nf, handle=hnd):
        rc = lib.sdm_warp_paste_tensor_nv12(handle, None if s is None else ctypes.byref(s), ctypes.c_void_p(x_),
                                            None if p is None else ctypes.byref(p), f, uv, n, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def at(f=fr, s=sp, x_=x.data_ptr(), p=pa, n=nf, ii=ii32, n_rows=len(idx), points=pts, handle=hnd):
        rc = lib.sdm_warp_paste_tensor_at_nv12(handle, None if points is None else points.ctypes.data, ii.ctypes.data, n_rows,
                                               None if s is None else ctypes.byref(s), ctypes.c_void_p(x_),
                                               None if p is None else ctypes.byref(p), f, uv, n, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def bad_spec(**kw):
        s = _lib.paste_tensor_spec(c["dtype"], c["layout"], c["channels"], **{k: v for k, v in M.spec_of(c).items() if k != "layout"})
        for k_, v in kw.items():
            setattr(s, k_, v)
        return s

    for call in (fit, at):
        for bad in (dict(s=None), dict(s=bad_spec(dtype=3)), dict(s=bad_spec(channels=2)), dict(s=bad_spec(gray_shift=13)),
                    dict(x_=0), dict(x_=x.data_ptr() + 8), dict(p=None), dict(p=_lib.SdmAlignPaste(amap.data_ptr(), 2)),
                    dict(f=None), dict(n=0), dict(n=len(dlst) - 1),
                    dict(f=with_frame(0, p=0)), dict(f=with_frame(1, w=0)), dict(f=with_frame(1, h=0)), dict(f=with_frame(2, fmt=6)),
                    dict(f=with_frame(0, stride=36)),                                             # below the luma row of 37 bytes
                    dict(f=with_frame(0, stride=37)),                                             # the luma fits, 19 UV pairs do not
                    dict(f=with_frame(7, stride=37 * 3 - 1))):
            assert code(call, **bad) == -1, bad
    assert code(fit, f=with_frame(1, w=63)) == -1                                                 # the fit form's size rule
    assert code(at, ii=np.array([len(dlst)] * len(idx), np.int32)) == -1 and code(at, n_rows=0) == -1 and code(at, points=None) == -1
    assert np.array_equal(dst.cpu().numpy(), c["buf"])                              # nothing was launched
    # the existing entry points keep refusing an NV12 frame
    assert lib.sdm_warp_paste_tensor_at(hnd, pts.ctypes.data, ii32.ctypes.data, len(idx), ctypes.byref(sp), ctypes.c_void_p(x.data_ptr()),
                                        ctypes.byref(pa), fr, nf, None) == -1
    assert lib.sdm_warp_paste_tensor(hnd, ctypes.byref(sp), ctypes.c_void_p(x.data_ptr()), ctypes.byref(pa), fr, nf, None, None) == -1
    assert np.array_equal(dst.cpu().numpy(), c["buf"])
    # no mesh
    fresh = Context(0)
    try:
        fresh.set_model_geometry(L, RE, LE, PARAMS)
        assert code(at, handle=fresh._h) == -1 and code(fit, handle=fresh._h) == -1
        fresh.warp_set_mesh(c["lm"], c["t"], c["tri"], c["cw"], c["ch"])
        assert code(fit, handle=fresh._h) == -1                                                   # no rows
        assert np.array_equal(dst.cpu().numpy(), c["buf"])
    finally:
        fresh.close()
    # a valid call behind the refusals, with no output pointer at all, gives the restatement's bytes
    at()
    compare(c, dst.cpu().numpy(), want, "behind the refusals")
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


ROUND_TRIP = {0: (1, 1, 151, 30), 1: (1, 1, 101, 20)}        # surface: (luma, chroma, pixels, samples) -- DESIGN 4.21


def test_detection_model_on_nv12_frames_and_round_trip(built):
    """detect on NV12 surfaces, cut the warped faces from them, paste the "network's" output back into them, with and without points=;
    then the round trip: the warped crops themselves pasted back with the same points at full opacity give the bytes of the
    restatement's own round trip, whose deviation from the surface inside the hull is asserted (DESIGN 4.21 records it)"""
    import torch
    model_, rng = small_model()
    surf = [nv12_surface(rng, 161, 97, True), nv12_surface(rng, 97, 81, True)]             # odd sizes; the faces well inside
    dev = [torch.from_numpy(b).cuda() for b, _ in surf]
    lst = [(d.data_ptr(), f["w"], f["h"], f["stride"], "nv12") for d, (_, f) in zip(dev, surf)]
    model_.detect_batch(lst, np.array([[64, 32, 30, 30], [36, 28, 24, 24]]))
    w, h = WC.CROPS[0]
    x, m0, f0 = model_.warped_crops_tensor((w, h), frames=lst, dtype="uint8")
    assert tuple(x.shape) == (2, 3, h, w) and not (f0 & R.DEGENERATE).any()
    c = model_.optimised_model.ctx
    before = c.get_x()
    pts, lab = model_.warp_points(), c.warp_labels()
    _, t, tri = WC.mesh_rcr22(w, h)
    seen = {}
    for name, y in (("inverted", (255 - x).contiguous()), ("round trip", x)):
        yh = y.cpu().numpy()
        dst = [torch.from_numpy(b).cuda() for b, _ in surf]
        dl = [(d.data_ptr(), f["w"], f["h"], f["stride"], "nv12") for d, (_, f) in zip(dst, surf)]
        mats, flags = model_.paste_warped_tensor(y, frames=dl)
        assert np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0)
        again = [torch.from_numpy(b).cuda() for b, _ in surf]
        al = [(d.data_ptr(), f["w"], f["h"], f["stride"], "nv12") for d, (_, f) in zip(again, surf)]
        none, f1 = model_.paste_warped_tensor(y, frames=al, points=pts, chroma=[None, None])
        assert none is None and np.array_equal(f1, flags)
        for s, (b, f) in enumerate(surf):
            want = b.copy()
            Y, UV = V.planes(want, f)
            a, tmap, foot, written = WN.paste_row(Y, UV, pts[s], tri, m0[s].reshape(-1, 6), lab, yh[s], None)
            assert (want != b).any() or name == "round trip"
            assert np.array_equal(dst[s].cpu().numpy(), want), (name, s)
            assert np.array_equal(again[s].cpu().numpy(), want), (name, s)
            if name == "round trip":
                Y0, UV0 = V.planes(b, f)
                full = a == 255
                whole = N.blocks(full.astype(np.int64)) == 4
                dy = int(np.abs(Y.astype(int) - Y0)[full].max())
                duv = int(np.abs(UV.astype(int) - UV0)[whole].max())
                print("round trip, surface", s, ": luma deviates by at most", dy, "chroma by at most", duv, "over", int(full.sum()),
                      "pixels and", int(whole.sum()), "samples at full opacity inside the hull")
                seen[s] = (dy, duv, int(full.sum()), int(whole.sum()))
    assert seen == ROUND_TRIP, seen
    assert np.array_equal(bits(c.get_x()), bits(before))                     # the landmark state is only read
    c.close()


# ---- frame geometry: offsets beyond 2^24, the chroma plane 2^28 bytes BEFORE its luma --------------------------------------------------
GEOMETRY = {"odd surface": (G.NV12_ODD, [(47, 40), (3, 4), (93, 77), (92, 20), (30, 77)], (33, 20)),
            "chroma before luma": (G.NV12_UV_BEFORE, G.FACE_CENTRES, (24, 24))}


def geometry_case(name):
    f, places, (cw, ch) = GEOMETRY[name]
    k = 60 + sorted(GEOMETRY).index(name)
    c = G.paste_case(k, "7", "nv12", [f], [0] * 5, places, cw, ch, "left right top bottom", None)
    c["points"] = G.mesh_points(c["mats"], cw, ch, 4000 + k)
    return c


def geometry_reference(c, pixels):
    """the restatement on copies of the planes, every row on a window of whole 2 x 2 blocks around it, as
    frame_geometry_cases.paste_reference does it for the other families"""
    want = [tuple(p.copy() for p in q) for q in pixels]
    idx, t, tri, lab = G.mesh(c["cw"], c["ch"])
    mats = WP.matrices(c["points"], t, tri)
    f = c["frames"][0]
    changed = far = last = 0
    for r in range(len(c["idx"])):
        x0, y0, x1, y1 = G.paste_window(f, c["points"][r], True)
        alpha = None if c["alpha"] is None else c["alpha"] if c["alpha"].ndim == 2 else c["alpha"][r]
        Y, UV = want[0][0][y0:y1, x0:x1], want[0][1][y0 // 2:(y1 + 1) // 2, x0 // 2:(x1 + 1) // 2]
        a, tmap, foot, written = WN.paste_row(Y, UV, c["points"][r], tri, mats[r], lab, c["x"][r], alpha, channels=3, origin=(x0, y0),
                                              **G.paste_spec(c))
        touched = foot | (a > 0)
        for edge, is_frame_edge in ((touched[:, 0], x0 == 0), (touched[:, -1], x1 == f["w"]), (touched[0], y0 == 0), (touched[-1], y1 == f["h"])):
            assert is_frame_edge or not edge.any(), ("the footprint touches the window's edge", r)
        changed += int((a > 0).sum())
        far += int(((a > 0).any(1) & ((np.arange(y0, y1) * f["pitch"]) > 2 ** 24)).sum())
        if x1 == f["w"] and y1 == f["h"]:
            last += int((a[-1] > 0).sum()) + int((a[:, -1] > 0).sum())
    return want, changed, far, last


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_frame_geometry(model, big, name):
    import torch
    c = geometry_case(name)
    pixels = G.paste_pixels(c)
    want, changed, far, last = geometry_reference(c, pixels)
    # luma rows more than 2^24 bytes into their plane; pixels of the frame's last row and column (odd surface: blocks of 2 x 1, 1 x 2, 1)
    assert changed > 1000 and far > 20 and last > 4, (changed, far, last)
    wc = bind(model)
    frames, ppix = G.paste_placement(c, pixels)
    with checked(big, frames, ppix):
        base = big.data_ptr()
        lst = [(base + f["off"], f["w"], f["h"], f["pitch"], f["fmt"]) for f in c["frames"]]
        chroma = [base + f["uv_off"] if "uv_off" in f else None for f in c["frames"]]
        idx, t, tri, lab = G.mesh(c["cw"], c["ch"])
        wc.warp_set_mesh(idx, t, tri, c["cw"], c["ch"])
        y = torch.from_numpy(c["x"]).cuda()
        mask = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
        flags = wc.warp_paste_tensor_at(c["points"], y, lst, image_index=c["idx"], mask=mask, chroma=chroma, **G.paste_spec(c))
        wc.synchronize()
        assert np.array_equal(flags, WP.flags(c["points"], t, tri, [(c["frames"][0]["w"], c["frames"][0]["h"])] * 5))
        wframes, wpix = G.paste_placement(c, want)
        for i, (f, w) in enumerate(zip(wframes, wpix)):
            for plane, (v, a) in enumerate(zip(views_of(big, f), w if isinstance(w, tuple) else (w,))):
                got = v.cpu().numpy()
                assert np.array_equal(got, a), (name, "frame %d plane %d" % (i, plane), "%d bytes differ" % int((got != a).sum()))
