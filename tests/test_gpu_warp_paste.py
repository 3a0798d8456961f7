"""Warped face tensors pasted back into frames on the device (csrc/sdm_warp_paste.hip, include/sdm.h "Pasting warped faces back",
detection_model.paste_warped_tensor).  Every comparison is bit for bit and on the WHOLE destination buffer -- the frames of
tests/warp_cases.py (gray 40 x 36 at pitch 41, BGR 37 x 33 at pitch 113, RGBA 48 x 40, cut from one buffer at misalignments 0 to 3),
their pitch padding and the bytes around them -- against the host restatement (tests/warp_paste_ref.py) on the device's own matrices."""
import ctypes
import itertools

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import paste_cases as C
import warp_cases as W
import warp_paste_ref as WP
import warp_ref as R
from test_warp_paste_host import spanning_rows
from test_gpu_warp import IDS, L, LE, MEAN, MESHES, PARAMS, RE, bits, code, identity_mesh, random_model
from superviseddescent_amd import Context, SdmError, _lib, feather_warp_mask, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
ROWS = [0, 1, 2, 1, 2, 1]                                        # six rows over the three frames a paste can write
SWAPPED = {**K.NAMES, T.BGR: "rgb", T.RGBA: "bgra"}              # the same bytes read as RGB and BGRA: the five formats
SWAP_FMT = {T.BGR: T.RGB, T.RGBA: T.BGRA}


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def placed():
    buf, frames = W.place()
    return buf, frames[:3]


def on_device(buf, frames, names=K.NAMES):
    import torch
    dev = torch.from_numpy(buf).cuda()
    return dev, [(dev.data_ptr() + f["off"], f["w"], f["h"], f["stride"], names[f["fmt"]]) for f in frames]


def install(ctx, buf, frames, rows, x, names=K.NAMES):
    """the frames as the context's images, as the crop source (in colour) and as the destination, the rows"""
    dev, lst = on_device(buf, frames, names)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(rows)
    ctx.set_x(x)
    ctx.align_set_source_frames(lst)
    return dev, lst


def spec_of(combo, k=0):
    dtype, layout, channels, order = combo
    return dict(layout=layout, channels=channels, order=order, scale=C.SCALES, bias=C.BIASES, gray_shift=14 + k % 2)


def expect(buf, frames, rows, pts, tri, mats, lab, y, alpha, swapped=False, **spec):
    """the restatement on a copy of buf: the rows in row order; returns (bytes, per-row (footprint, opacity, triangle map))"""
    want, res = buf.copy(), []
    for r, im in enumerate(rows):
        a = None if alpha is None else alpha if alpha.ndim == 2 else alpha[r]
        fmt = SWAP_FMT.get(frames[im]["fmt"], frames[im]["fmt"]) if swapped else frames[im]["fmt"]
        res.append(WP.paste_row(C.view(want, frames[im]), fmt, pts[r], tri, np.asarray(mats[r]).reshape(-1, 6), lab, y[r], a, **spec))
    return want, res


def paste_call(spec):
    return {k: v for k, v in spec.items() if k != "channels"}


def test_identity(ctx, placed):
    """landmarks = template + an integer translation, the tensor cut by the warp itself, a whole-crop opacity of 255: the paste leaves
    every byte; the complemented tensor changes exactly the pixels of warp_mask() shifted, each to its complement"""
    buf, frames = placed
    w, h = W.CROPS[0]
    idx, t, tri = identity_mesh(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    on = ctx.warp_labels() != R.NONE
    shifts = [(5, 7), (11, 3), (0, 0), (13, 12)]
    rows = [0, 1, 2, 1]
    x = np.zeros((4, 2 * L), f32)
    for r, (tx, ty) in enumerate(shifts):
        x[r, idx], x[r, L + idx] = t[:, 0] + tx, t[:, 1] + ty
    dev, lst = install(ctx, buf, frames, rows, x)
    crops, mats, flags = ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=3, order="bgr")
    assert not flags.any()
    full = np.full((h, w), 255, np.uint8)
    m2, f2 = ctx.warp_paste_tensor(crops, lst, layout="nhwc", mask=full, order="bgr")
    assert not f2.any() and np.array_equal(bits(m2), bits(mats))
    assert np.array_equal(dev.cpu().numpy(), buf)
    ctx.warp_paste_tensor(255 - crops, lst, layout="nhwc", mask=full, order="bgr")
    want = buf.copy()
    for r, (tx, ty) in enumerate(shifts):
        f = frames[rows[r]]
        src, out = C.view(buf, f), C.view(want, f)
        nb = min(3, src.shape[2])
        out[ty:ty + h, tx:tx + w, :nb][on] = 255 - src[ty:ty + h, tx:tx + w, :nb][on]
    got = dev.cpu().numpy()
    assert (want != buf).sum() > 3 * on.sum() and np.array_equal(got, want)


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_against_the_restatement(ctx, placed, mesh):
    buf, frames = placed
    import torch
    # run k of the 24 (three meshes x two crops x two format sets x two) takes combination 5 k mod 24: every one of dtype x layout x
    # channels x order exactly once over the three meshes, and both orders under every mesh
    k = sorted(MESHES).index(mesh) * 8
    assert len(MESHES) == 3 and {COMBOS[(5 * j) % len(COMBOS)] for j in range(24)} == set(COMBOS)
    seen = set()
    for (w, h), swapped in itertools.product(W.CROPS, (False, True)):
        idx, t, tri = MESHES[mesh](w, h)
        ctx.warp_set_mesh(idx, t, tri, w, h)
        lab = ctx.warp_labels()
        x = W.rows_for(frames, ROWS, idx, t, w, h, 60 + k)
        pts = WP.points_of(x, idx)
        for rep in range(2):
            combo = COMBOS[(5 * k) % len(COMBOS)]
            seen.add(combo)
            spec = spec_of(combo, k)
            y = C.tensor(len(ROWS), w, h, combo[0], combo[1], combo[2], 70 + k)
            alpha = [None, C.alpha_maps(1, w, h, 80 + k)[0], C.alpha_maps(len(ROWS), w, h, 81 + k)][(k + rep) % 3]
            dev, lst = install(ctx, buf, frames, ROWS, x, SWAPPED if swapped else K.NAMES)
            mats, flags = ctx.warp_paste_tensor(torch.from_numpy(y).cuda(), lst, mask=alpha, **paste_call(spec))
            assert np.array_equal(bits(mats.reshape(len(ROWS), -1, 6)), bits(R.matrices(x, idx, t, tri)))
            assert np.array_equal(flags, R.flags(x, idx, t, tri, [(frames[i]["w"], frames[i]["h"]) for i in ROWS]))
            want, _ = expect(buf, frames, ROWS, pts, tri, mats, lab, y, alpha, swapped, **spec)
            assert (want != buf).sum() > 200
            assert np.array_equal(dev.cpu().numpy(), want), (mesh, w, h, swapped, combo)
            k += 1
    assert len(seen) == 8 and {c[3] for c in seen} == {"bgr", "rgb"} and {c[0] for c in seen} == {"uint8", "float16", "float32"}


def test_rows_overlap_in_row_order(ctx, placed):
    """six rows on ONE frame, each a little beside the other: the result is that of the rows one after another, and the same call
    with the rows reversed gives the other result"""
    buf, frames = placed
    import torch
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    rows = [2] * 6
    x = W.rows_for(frames, rows, idx, t, w, h, 91)
    pts = WP.points_of(x, idx)
    y = C.tensor(6, w, h, "uint8", "nchw", 3, 92)
    alpha = C.alpha_maps(6, w, h, 93)
    spec = spec_of(("uint8", "nchw", 3, "rgb"))
    out = []
    for order in (np.arange(6), np.arange(6)[::-1]):
        dev, lst = install(ctx, buf, frames, rows, x[order])
        mats, _ = ctx.warp_paste_tensor(torch.from_numpy(y[order].copy()).cuda(), lst, mask=alpha[order].copy(), **paste_call(spec))
        want, res = expect(buf, frames, rows, pts[order], tri, mats, lab, y[order], alpha[order], **spec)
        assert sum((a > 0).astype(int) for _, a, _ in res).max() >= 2            # rows meet on a pixel
        out.append(dev.cpu().numpy())
        assert np.array_equal(out[-1], want)
    assert not np.array_equal(out[0], out[1])


def test_opacity_maps_and_the_zero_band(ctx, placed):
    buf, frames = placed
    import torch
    w, h = W.CROPS[1]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    x = W.rows_for(frames, ROWS, idx, t, w, h, 95)
    pts = WP.points_of(x, idx)
    pattern = np.tile(np.arange(251, dtype=np.uint8), buf.size // 251 + 1)[:buf.size].copy()      # (frames pre-filled with a pattern)
    y = C.tensor(len(ROWS), w, h, "float16", "nhwc", 3, 96)
    spec = spec_of(("float16", "nhwc", 3, "bgr"))
    for alpha in (None, C.alpha_maps(1, w, h, 97)[0], C.alpha_maps(len(ROWS), w, h, 98), C.alpha_maps(len(ROWS), w, h, 99, zero_band=True)):
        dev, lst = install(ctx, pattern, frames, ROWS, x)
        mats, _ = ctx.warp_paste_tensor(torch.from_numpy(y).cuda(), lst, mask=alpha, **paste_call(spec))
        want, res = expect(pattern, frames, ROWS, pts, tri, mats, lab, y, alpha, **spec)
        got = dev.cpu().numpy()
        assert np.array_equal(got, want) and (want != pattern).sum() > 300
    # under the zero band (the last map): pixels inside a footprint whose every opacity is 0 keep the pattern
    kept = 0
    for im in range(3):
        foot = np.any([res[r][0] for r in range(len(ROWS)) if ROWS[r] == im], 0)
        none = foot & ~np.any([res[r][1] > 0 for r in range(len(ROWS)) if ROWS[r] == im], 0)
        kept += int(none.sum())
        assert np.array_equal(C.view(got, frames[im])[none], C.view(pattern, frames[im])[none])
    assert kept > 20


def test_the_hull_fades_by_itself(ctx, placed):
    buf, frames = placed
    import torch
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    x = W.rows_for(frames, ROWS, idx, t, w, h, 101)
    pts = WP.points_of(x, idx)
    y = C.tensor(len(ROWS), w, h, "uint8", "nchw", 1, 102)
    spec = spec_of(("uint8", "nchw", 1, "rgb"))
    dev, lst = install(ctx, buf, frames, ROWS, x)
    mats, _ = ctx.warp_paste_tensor(torch.from_numpy(y).cuda(), lst, **paste_call(spec))
    want, res = expect(buf, frames, ROWS, pts, tri, mats, lab, y, None, **spec)
    assert np.array_equal(dev.cpu().numpy(), want)
    seen = 0
    for foot, a, tmap in res:
        if foot.sum() < 100:                                                   # (a face minified to a few pixels)
            continue
        part = (a > 0) & (a < 255)
        assert 4 <= part.sum() < foot.sum() // 2 and (a == 255).any()          # the border fades, the interior has full weight
        seen += 1
    assert seen >= 4


def test_fit_form_against_at_form(ctx, placed):
    buf, frames = placed
    import torch
    w, h = W.CROPS[1]
    idx, t, tri = W.mesh_254(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    x = W.rows_for(frames, ROWS, idx, t, w, h, 105)
    y = torch.from_numpy(C.tensor(len(ROWS), w, h, "float32", "nchw", 3, 106)).cuda()
    alpha = C.alpha_maps(1, w, h, 107)[0]
    spec = paste_call(spec_of(("float32", "nchw", 3, "rgb")))
    dev, lst = install(ctx, buf, frames, ROWS, x)
    crops, mats, flags = ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=3)
    before = (ctx.get_x(), crops.cpu().numpy())
    assert np.array_equal(dev.cpu().numpy(), buf)
    m2, f2 = ctx.warp_paste_tensor(y, lst, mask=alpha, **spec)
    assert np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
    fit = dev.cpu().numpy()
    assert np.array_equal(bits(ctx.get_x()), bits(before[0]))
    # the crop source is untouched: the warp of the ORIGINAL bytes gives the crops again
    dev0, lst0 = install(ctx, buf, frames, ROWS, x)
    assert np.array_equal(ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=3)[0].cpu().numpy(), before[1])
    # the _at form: no rows, no images -- a fresh context with the mesh alone
    fresh = Context(0)
    try:
        fresh.set_model_geometry(L, RE, LE, PARAMS)
        fresh.warp_set_mesh(idx, t, tri, w, h)
        dev1, lst1 = on_device(buf, frames)
        f3 = fresh.warp_paste_tensor_at(WP.points_of(x, idx), y, lst1, image_index=ROWS, mask=alpha, **spec)
        assert np.array_equal(f3, flags) and np.array_equal(dev1.cpu().numpy(), fit) and not np.array_equal(fit, buf)
    finally:
        fresh.close()


def test_every_flag_alone(ctx, placed):
    buf, frames = placed
    import torch
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    rows = [2, 2, 2, 2]                                                    # the 48 x 40 frame holds the whole template at (12, 10)
    x = np.zeros((4, 2 * L), f32)
    x[:, idx], x[:, L + idx] = t[:, 0] + 12, t[:, 1] + 10
    a, b, c = tri[0]
    x[0, idx[4]] = np.nan                                                   # DEGENERATE
    x[1, idx] = t[:, 0] - t[:, 0].min() - 0.5                               # PARTIAL alone: half a pixel past the left edge
    x[2, [idx[b], idx[c]]], x[2, [L + idx[b], L + idx[c]]] = x[2, [idx[c], idx[b]]], x[2, [L + idx[c], L + idx[b]]]      # FOLDED alone
    pts = WP.points_of(x, idx)
    y = C.tensor(4, w, h, "uint8", "nhwc", 3, 111)
    spec = spec_of(("uint8", "nhwc", 3, "bgr"))
    dev, lst = install(ctx, buf, frames, rows, x)
    mats, flags = ctx.warp_paste_tensor(torch.from_numpy(y).cuda(), lst, **paste_call(spec))
    assert flags.tolist() == [R.DEGENERATE, R.PARTIAL, R.FOLDED, 0] and np.isnan(mats[0]).all()
    want, res = expect(buf, frames, rows, pts, tri, mats, lab, y, None, **spec)
    assert not res[0][0].any() and all(r[0].sum() > 50 for r in res[1:])    # the degenerate row pastes nothing, its neighbours do
    assert np.array_equal(dev.cpu().numpy(), want)
    # the degenerate row alone: no byte changes
    dev, lst = install(ctx, buf, frames, rows[:1], x[:1])
    assert ctx.warp_paste_tensor(torch.from_numpy(y[:1]).cuda(), lst, **paste_call(spec))[1].tolist() == [R.DEGENERATE]
    assert np.array_equal(dev.cpu().numpy(), buf)


def test_far_landmarks_are_decided_by_the_triangle_box(ctx, placed):
    """six rows that all span the 48 x 40 frame, five of them with one landmark at 1e9 ... 1e18 (test_warp_paste_host.FAR): the needle triangles at that landmark
    have rounded edge functions >= 0 many pixels beyond their corners, where only the triangle's box decides -- the same in the
    owner's walk behind the wave's cull and in the ownership path, or a pixel would have two owners"""
    buf, frames = placed
    import torch
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    rows = [2] * 6
    p = spanning_rows(t, 48, 40, w, h, 6, np.random.default_rng(131))
    x = np.zeros((6, 2 * L), f32)
    x[:, idx], x[:, L + idx] = p[..., 0], p[..., 1]
    pts = WP.points_of(x, idx)
    y = C.tensor(6, w, h, "float32", "nhwc", 3, 132)
    spec = spec_of(("float32", "nhwc", 3, "rgb"))
    alpha = np.full((h, w), 128, np.uint8)
    dev, lst = install(ctx, buf, frames, rows, x)
    mats, flags = ctx.warp_paste_tensor(torch.from_numpy(y).cuda(), lst, mask=alpha, **paste_call(spec))
    assert not (flags & R.DEGENERATE).any()
    want, res = expect(buf, frames, rows, pts, tri, mats, lab, y, alpha, **spec)
    boxed = sum(int((res[r][2] != WP.triangle_map(pts[r], tri, np.asarray(mats[r]).reshape(-1, 6), 48, 40, tri_box=False)).sum())
                for r in range(6))
    assert boxed > 100 and sum((a > 0).astype(int) for _, a, _ in res).max() >= 2
    assert np.array_equal(dev.cpu().numpy(), want)


def test_refusals(ctx, placed):
    import torch
    buf, frames = placed
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    idx, tri = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(tri, np.int32)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    good_labels = ctx.warp_labels()
    x = W.rows_for(frames, ROWS, idx, t, w, h, 9)
    dev, lst = install(ctx, buf, frames, ROWS, x)
    n = len(ROWS)
    y = torch.from_numpy(C.tensor(n, w, h, "float16", "nchw", 3, 12)).cuda()
    mis = torch.zeros(y.numel() + 4, dtype=torch.float16, device="cuda")[4:]                                      # 8 bytes off
    pts = WP.points_of(x, idx)
    rows = np.asarray(ROWS, np.int32)
    lib, hnd = ctx._lib, ctx._h
    base = dict(dtype="float16", layout="nchw", channels=3, scale=C.SCALES, bias=C.BIASES)

    def S(**kw):
        s = _lib.paste_tensor_spec(**dict(base, **{k: v for k, v in kw.items() if k in ("scale", "bias")}))
        for k, v in kw.items():
            if k not in ("scale", "bias"):
                setattr(s, k, v)
        return ctypes.byref(s)

    def frame_array(lst):
        desc = _lib.frame_descriptors(lst, None)
        return (_lib.SdmFrame * len(desc))(*[_lib.SdmFrame(ctypes.c_void_p(p), fw, fh, st, f) for p, fw, fh, st, f in desc])

    arr = frame_array(lst)
    paste = _lib.SdmAlignPaste(None, 0)

    def raw(spec_ptr=None, in_ptr=None, paste_ptr=ctypes.byref(paste), fr=arr, nf=3, at=False, points=pts, index=rows, nr=n, handle=hnd):
        spec_ptr = S() if spec_ptr is None else spec_ptr
        in_ptr = y.data_ptr() if in_ptr is None else in_ptr
        if at:
            rc = lib.sdm_warp_paste_tensor_at(handle, None if points is None else points.ctypes.data, None if index is None else index.ctypes.data,
                                              nr, spec_ptr, ctypes.c_void_p(in_ptr), paste_ptr, fr, nf, None)
        else:
            rc = lib.sdm_warp_paste_tensor(handle, spec_ptr, ctypes.c_void_p(in_ptr), paste_ptr, fr, nf, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def with_frame(i, **kw):
        """the frame array with fields of entry i replaced"""
        out = (_lib.SdmFrame * 3)(*[_lib.SdmFrame(ctypes.c_void_p(a.data), a.width, a.height, a.stride_bytes, a.format) for a in arr])
        for name, v in kw.items():
            setattr(out[i], name, v)
        return out

    bad_paste = _lib.SdmAlignPaste(None, 2)
    nv12 = with_frame(1, format=T.NV12)
    for at in (False, True):
        calls = [
            lambda: raw(S(dtype=3), at=at), lambda: raw(S(layout=2), at=at), lambda: raw(S(order=-1), at=at), lambda: raw(S(channels=2), at=at),
            lambda: raw(S(gray_shift=13), at=at), lambda: raw(S(scale=[1, np.nan, 1]), at=at), lambda: raw(S(bias=[0, 0, np.inf]), at=at),
            lambda: raw(in_ptr=mis.data_ptr(), at=at), lambda: raw(paste_ptr=None, at=at), lambda: raw(paste_ptr=ctypes.byref(bad_paste), at=at),
            lambda: raw(fr=None, at=at), lambda: raw(nf=0, at=at), lambda: raw(fr=nv12, at=at),
            lambda: raw(fr=with_frame(0, width=0), at=at), lambda: raw(fr=with_frame(1, stride_bytes=3 * lst[1][1] - 1), at=at),
            lambda: raw(fr=with_frame(2, data=None), at=at), lambda: raw(fr=with_frame(2, format=77), at=at),
            lambda: raw(nf=2, at=at),                                            # a row's image index beyond the frames
        ]
        for f in calls:
            assert code(f) == -1
            assert np.array_equal(dev.cpu().numpy(), buf) and np.array_equal(ctx.warp_labels(), good_labels)
    assert lib.sdm_warp_paste_tensor(hnd, None, ctypes.c_void_p(y.data_ptr()), ctypes.byref(paste), arr, 3, None, None) == -1       # no spec
    assert lib.sdm_warp_paste_tensor(hnd, S(), None, ctypes.byref(paste), arr, 3, None, None) == -1                                  # no tensor
    # fit form: a frame that differs in size from the context's image
    assert code(lambda: raw(fr=with_frame(1, width=lst[1][1] - 1))) == -1
    # _at form: no points, no rows, an index outside the list
    assert code(lambda: raw(at=True, points=None)) == -1 and code(lambda: raw(at=True, nr=0)) == -1
    assert code(lambda: raw(at=True, index=np.array([0, 1, 2, 3, 1, 1], np.int32))) == -1
    assert code(lambda: raw(at=True, index=np.array([0, 1, -1, 2, 1, 1], np.int32))) == -1
    assert np.array_equal(dev.cpu().numpy(), buf) and np.array_equal(ctx.warp_labels(), good_labels)
    # fit form: the warp call's rules on the rows' source -- a crop source that does not cover the rows, or differs in size
    ctx.align_set_source_frames(lst[:2])
    assert code(lambda: raw()) == -1
    ctx.align_set_source_frames([lst[0], (lst[1][0], lst[1][1] - 1, lst[1][2], lst[1][3], lst[1][4]), lst[2]])
    assert code(lambda: raw()) == -1
    ctx.align_set_source_frames(lst)
    assert np.array_equal(dev.cpu().numpy(), buf) and np.array_equal(ctx.warp_labels(), good_labels)
    raw()                                                                        # the good call pastes
    assert not np.array_equal(dev.cpu().numpy(), buf)
    # no mesh, no rows; another L drops the mesh
    fresh = Context(0)
    try:
        dev1, lst1 = on_device(buf, frames)
        arr1 = frame_array(lst1)
        fresh.set_model_geometry(L, RE, LE, PARAMS)
        assert code(lambda: raw(fr=arr1, handle=fresh._h)) == -1 and code(lambda: raw(fr=arr1, at=True, handle=fresh._h)) == -1      # no mesh
        fresh.warp_set_mesh(idx, t, tri, w, h)
        assert code(lambda: raw(fr=arr1, handle=fresh._h)) == -1                                                                 # no rows
        fresh.set_model_geometry(L + 1, RE, LE, PARAMS)
        assert code(lambda: raw(fr=arr1, at=True, handle=fresh._h)) == -1                                                        # L changed
        assert np.array_equal(dev1.cpu().numpy(), buf)
    finally:
        fresh.close()


def test_behind_tracker_step_and_detect_batch(built):
    import torch
    model = random_model()
    frames, _, boxes = synth.make_tracks(2, 2, seed=58)
    rng = np.random.default_rng(5)
    colour = [np.repeat(frames[1, s][..., None], 3, -1) + rng.integers(0, 2, frames[1, s].shape + (3,), dtype=np.uint8) for s in range(2)]
    ids = np.arange(2)
    tr = model.tracker(2)
    tr.start(ids, boxes[0])
    tr.step(ids, [torch.from_numpy(f).cuda() for f in frames[0]])
    dev = [torch.from_numpy(c).cuda() for c in colour]
    tr.step(ids, dev)
    c = model.optimised_model.ctx
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
    before = (c.get_x(), tr.get(ids))
    out, mats, flags = model.warped_crops_tensor((24, 20), frames=dev, **norm)
    pts = model.warp_points()
    assert pts.shape == (2, len(IDS), 2) and pts.dtype == f32
    y = -out                                                                   # "a network": the negated texture
    m2, f2 = model.paste_warped_tensor(y, frames=dev, **norm)
    assert np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
    lab, (T_, w, h) = c.warp_labels(), c.warp_mesh
    idx, t, tri = W.mesh_rcr22(w, h)
    spec = _lib.paste_tensor_spec("float16", **norm)
    ynp = y.cpu().numpy()
    for s in range(2):
        want = colour[s].copy()
        WP.paste_row(want, T.BGR, pts[s], tri, m2[s].reshape(-1, 6), lab, ynp[s], None, scale=np.array(spec.scale, f32), bias=np.array(spec.bias, f32))
        assert np.array_equal(dev[s].cpu().numpy(), want) and (want != colour[s]).sum() > 100
    after = (c.get_x(), tr.get(ids))
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert np.array_equal(bits(before[1][0]), bits(after[1][0])) and np.array_equal(before[1][1], after[1][1])
    # later, with the points kept: the tracker has stepped on, the paste lands where the faces were
    dev2 = [torch.from_numpy(c_).cuda() for c_ in colour]
    tr.step(ids, [torch.from_numpy(f).cuda() for f in frames[1]])
    none, f3 = model.paste_warped_tensor(y, frames=dev2, points=pts, **norm)
    assert none is None and np.array_equal(f3, flags)
    assert all(np.array_equal(dev2[s].cpu().numpy(), dev[s].cpu().numpy()) for s in range(2))
    # behind detect_batch, with a feathered map
    rows = model.detect_batch(list(frames[1]), boxes[1])
    c = model.optimised_model.ctx
    gray = [torch.from_numpy(f.copy()).cuda() for f in frames[1]]
    out, mats, flags = model.warped_crops_tensor((33, 17), frames=gray, dtype="float32", channels=1)
    mask = feather_warp_mask(model.warp_mask(), 2)
    m2, f2 = model.paste_warped_tensor(out * 0.5, frames=gray, mask=mask)
    assert np.array_equal(bits(c.get_x()), bits(rows)) and np.array_equal(bits(m2), bits(mats))
    pts, lab = model.warp_points(), c.warp_labels()
    _, t, tri = W.mesh_rcr22(33, 17)
    for s in range(2):
        want = frames[1][s].copy()[..., None]
        WP.paste_row(want, T.GRAY, pts[s], tri, m2[s].reshape(-1, 6), lab, (out * 0.5)[s].cpu().numpy(), mask, channels=1)
        assert np.array_equal(gray[s].cpu().numpy(), want[..., 0]) and (want[..., 0] != frames[1][s]).sum() > 50
    c.close()
