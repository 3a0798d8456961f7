"""Crop tensors and warped face tensors pasted into planar colour frames, 3 x H x W (include/sdm.h, "Planar colour frames";
csrc/sdm_paste_device.h: paste_load / paste_apply / paste_store): rigid and piecewise-affine, plain and area-averaged, the `_at` form and
the fit form; destinations at the default plane distance through the plain calls, at a padded, a negative and a region view's distance
through the `_nv12` forms, with a BGR and an NV12 frame in the same list.  Every comparison is bit for bit against the references of the
interleaved formats (tests/paste_ref.py, paste_area_ref.py, paste_nv12_ref.py, warp_paste_ref.py, warp_paste_area_ref.py,
warp_paste_nv12_ref.py) applied to the interleaved view of the same pixels, and on the WHOLE destination buffer: pitch padding, the gaps
between the planes and the untouched pixels keep the noise they held."""
import ctypes

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import paste_area_ref as PA
import paste_cases as C
import paste_nv12_ref as N
import paste_ref as P
import planar_cases as PC
import warp_cases as W
import warp_paste_area_ref as WPA
import warp_paste_nv12_ref as WN
import warp_paste_ref as WP
import warp_ref as WR
from superviseddescent_amd import Context, HoGParam, SdmError, _lib, align_filter, ibug

pytestmark = pytest.mark.gpu
f32 = np.float32
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
LM = np.array([3, 6, 9, 12, 15])
BP, RP = PC.BGR_PLANAR, PC.RGB_PLANAR
AREA = (PA.AREA, 16, 1.0)
# (dtype, layout, channels, order): every dtype, both layouts and orders, 1 and 3 channels
COMBOS = [("uint8", "nhwc", 3, "bgr"), ("float16", "nchw", 3, "rgb"), ("float32", "nhwc", 1, "bgr"), ("float16", "nhwc", 3, "bgr"),
          ("uint8", "nchw", 1, "rgb"), ("float32", "nchw", 3, "rgb")]
DEFAULT = [(37, 29, BP, 1, "default"), (64, 48, RP, 3, "default"), (2, 2, RP, 5, "default"), (1, 1, BP, 0, "default"), (5, 4, BP, 0, "default")]


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


def template(w, h):
    return (np.array([[0.2, 0.2], [0.8, 0.25], [0.5, 0.5], [0.3, 0.8], [0.75, 0.7]]) * (w - 1 + 1e-3, h - 1 + 1e-3)).astype(f32) + 0.125


def bits(a):
    return np.asarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[np.asarray(a).dtype.itemsize])


def spec_of(layout, order):
    return dict(layout=layout, order=order, scale=C.SCALES, bias=C.BIASES, gray_shift=14 if order == "bgr" else 15)


class Dest:
    """one destination frame inside a host copy of the buffer, as the references write it: a planar frame as the interleaved array of
    the same pixels (scattered back into the planes by done()), the other formats as views"""

    def __init__(self, buf, f):
        st = np.lib.stride_tricks.as_strided
        self.f, self.buf = f, buf
        if PC.is_planar(f):
            self.fmt, self.pix = PC.PACKED[f["fmt"]], np.ascontiguousarray(np.transpose(PC.planes(buf, f), (1, 2, 0)))
        elif f["fmt"] == T.NV12:
            h, w, s = f["h"], f["w"], f["stride"]
            self.fmt, self.Y, self.UV = T.NV12, st(buf[f["off"]:], (h, w), (s, 1)), st(buf[f["uv_off"]:], ((h + 1) // 2, (w + 1) // 2, 2), (s, 2, 1))
        else:
            bpp = P.BPP[f["fmt"]]
            self.fmt, self.pix = f["fmt"], st(buf[f["off"]:], (f["h"], f["w"], bpp), (f["stride"], bpp, 1))

    def done(self):
        f = self.f
        if PC.is_planar(f):
            st = np.lib.stride_tricks.as_strided
            for c in range(3):
                st(self.buf[f["off"] + c * f["D"]:], (f["h"], f["w"]), (f["stride"], 1))[...] = self.pix[..., c]


def expect(buf, frames, idx, row):
    """the references on a copy of buf: row(dest, r) pastes row r into its frame, the rows in row order"""
    want = buf.copy()
    dest = {}
    for r, im in enumerate(idx):
        if im not in dest:
            dest[im] = Dest(want, frames[im])
        row(dest[im], r)
    for d in dest.values():
        d.done()
    return want


def alpha_of(alpha, r):
    return None if alpha is None else alpha if alpha.ndim == 2 else alpha[r]


def rigid_row(mats, x, alpha, filt, channels, spec):
    def row(d, r):
        S = 1 if filt is None or P.inverse(mats[r])[1] else PA.samples(mats[r], *filt)
        if d.fmt == T.NV12:
            N.paste_row(d.Y, d.UV, mats[r], x[r], alpha_of(alpha, r), S, channels=channels, **spec)
        else:
            PA.paste_row(d.pix, d.fmt, mats[r], x[r], alpha_of(alpha, r), S, channels=channels, **spec)
    return row


def mesh_row(points, tri, mats, lab, x, alpha, filt, channels, spec, frames, idx):
    def row(d, r):
        a = alpha_of(alpha, r)
        f = frames[idx[r]]
        if filt is None:
            if d.fmt == T.NV12:
                WN.paste_row(d.Y, d.UV, points[r], tri, mats[r], lab, x[r], a, channels=channels, **spec)
            else:
                WP.paste_row(d.pix, d.fmt, points[r], tri, mats[r], lab, x[r], a, channels=channels, **spec)
            return
        cnt = WPA.counts(points[r], tri, mats[r], f["w"], f["h"], *filt)
        if d.fmt == T.NV12:
            WPA.paste_row_nv12(d.Y, d.UV, points[r], tri, mats[r], lab, x[r], a, cnt, channels=channels, **spec)
        else:
            WPA.paste_row(d.pix, d.fmt, points[r], tri, mats[r], lab, x[r], a, cnt, channels=channels, **spec)
    return row


def maps(k, n, w, h):
    """no map, one for all rows, one per row (its left half 0), by turns"""
    return (None, C.alpha_maps(1, w, h, 50 + k)[0], C.alpha_maps(n, w, h, 60 + k, zero_band=True))[k % 3]


def tuples(dev, frames):
    """the frames as (ptr, w, h, stride, name) tuples WITHOUT second planes: the default plane distance, the plain calls"""
    return [(dev.data_ptr() + f["off"], f["w"], f["h"], f["stride"], PC.NAMES[f["fmt"]]) for f in frames]


def filter_of(filt):
    return None if filt is None else align_filter("area", filt[1], filt[2])


# ---- the rigid paste -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, AREA])
def test_rigid_at_form_default_distance_plain_calls(ctx, filt):
    import torch
    buf, frames = PC.place(DEFAULT, 23)
    idx = [0, 1, 2, 3, 4, 1, 0]
    for (w, h) in K.CROPS[1:]:
        mats = np.stack([S.astype(f32) for S in K.similarities(frames, idx, w, h, 30 + w)])
        for k, (dtype, layout, channels, order) in enumerate(COMBOS):
            x, alpha, spec = C.tensor(len(idx), w, h, dtype, layout, channels, 40 + k), maps(k, len(idx), w, h), spec_of(layout, order)
            dev = torch.from_numpy(buf).cuda()
            lst = tuples(dev, frames)
            assert all(p is None for p in _lib.frame_planes(lst)[1])          # no second plane: sdm_align_paste_tensor_at[_filtered]
            got = ctx.align_paste_tensor_at(mats, torch.from_numpy(x).cuda(), lst, image_index=idx, mask=alpha, filter=filter_of(filt), **spec)
            flags = got if filt is None else got[0]
            want = expect(buf, frames, idx, rigid_row(mats, x, alpha, filt, channels, spec))
            assert np.array_equal(dev.cpu().numpy(), want), (w, h, dtype, layout, channels, order)
            assert flags.tolist() == [P.flags_at(mats[r], w, h, frames[im]["w"], frames[im]["h"]) for r, im in enumerate(idx)]
            assert (want != buf).sum() > 500


@pytest.mark.parametrize("filt", [None, AREA])
def test_rigid_at_form_mixed_list_every_plane_distance(ctx, filt):
    """planar at the odd, the negative, the far and the region view's distance, BGR and NV12 in one list: the _nv12 forms; two rows on
    frame 5 and three on frame 1 overlap"""
    import torch
    buf, frames = PC.place()
    idx = [0, 1, 2, 3, 4, 5, 6, 7, 1, 5, 1]
    seen = 0
    for (w, h) in K.CROPS[1:]:
        mats = np.stack([S.astype(f32) for S in K.similarities(frames, idx, w, h, 70 + w)])
        scale = 2.6 if filt else 1.0                               # (filtered: the crop outsizes the face, S > 1)
        mats[8] = A.similarity(1.3 / scale * 64 / w, 20.0, 9, 4).astype(f32)
        mats[10] = A.similarity(1.1 / scale * 64 / w, -15.0, 14, 8).astype(f32)
        mats[1] = A.similarity(1.2 / scale * 64 / w, 5.0, 4, 6).astype(f32)
        mats[9] = mats[5].copy()
        mats[9][:, 2] += (3.5, -2.25)
        for k, (dtype, layout, channels, order) in enumerate(COMBOS):
            x, alpha, spec = C.tensor(len(idx), w, h, dtype, layout, channels, 80 + k), maps(k + 1, len(idx), w, h), spec_of(layout, order)
            dev = torch.from_numpy(buf).cuda()
            lst, formats, chroma = PC.device_frames(dev, frames)
            got = ctx.align_paste_tensor_at(mats, torch.from_numpy(x).cuda(), lst, formats, image_index=idx, mask=alpha, chroma=chroma,
                                            filter=filter_of(filt), **spec)
            want = expect(buf, frames, idx, rigid_row(mats, x, alpha, filt, channels, spec))
            assert np.array_equal(dev.cpu().numpy(), want), (w, h, dtype, layout, channels, order)
            if filt:
                assert got[1].tolist() == [1 if P.inverse(m)[1] else PA.samples(m, *filt) for m in mats] and got[1].max() > 1
            seen += 1
        # the case cannot pass by accident: rows 1, 8 and 10 share pixels of frame 1, and the reverse order gives other bytes
        order3 = [1, 8, 10]
        back = expect(buf, frames, [1, 1, 1], rigid_row(mats[order3[::-1]], x[order3[::-1]], None, filt, channels, spec))
        fwd = expect(buf, frames, [1, 1, 1], rigid_row(mats[order3], x[order3], None, filt, channels, spec))
        assert not np.array_equal(fwd, back)
    assert seen == 2 * len(COMBOS)


@pytest.mark.parametrize("filt", [None, AREA])
def test_rigid_fit_form(ctx, filt):
    import torch
    buf, frames = PC.place()
    idx = [0, 1, 5, 6, 7, 2, 1]
    w, h = 16, 16
    src = torch.from_numpy(buf).cuda()
    lst, formats, chroma = PC.device_frames(src, frames)
    ctx.set_frames_device(lst, formats, chroma=chroma)
    ctx.set_sample_image_index(idx)
    t = template(w, h)
    rows = K.landmark_rows(K.similarities(frames, idx, w, h, 21), t, LM, L)
    rows[3, LM[1]] = np.nan                                        # a DEGENERATE row
    ctx.set_x(rows)
    for k, (dtype, layout, channels, order) in enumerate(COMBOS[:3]):
        x, alpha, spec = C.tensor(len(idx), w, h, dtype, layout, channels, 22 + k), maps(k + 2, len(idx), w, h), spec_of(layout, order)
        dev = torch.from_numpy(buf).cuda()
        dl, df, dc = PC.device_frames(dev, frames)
        got = ctx.align_paste_tensor(LM, t, torch.from_numpy(x).cuda(), dl, df, mask=alpha, chroma=dc, filter=filter_of(filt), **spec)
        mats, flags = got[0], got[1]
        assert flags[3] == A.DEGENERATE and np.isnan(mats[3]).all()
        want = expect(buf, frames, idx, rigid_row(mats, x, alpha, filt, channels, spec))
        assert np.array_equal(dev.cpu().numpy(), want), (dtype, layout, channels, order)
        assert (want != buf).sum() > 500
    assert np.array_equal(src.cpu().numpy(), buf)                  # the context's frames are only read
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


def test_rigid_fit_form_default_distance_plain_call(ctx):
    import torch
    buf, frames = PC.place(DEFAULT, 23)
    idx = [0, 1, 4, 1]
    w, h = 16, 16
    src = torch.from_numpy(buf).cuda()
    ctx.set_frames_device(tuples(src, frames))
    ctx.set_sample_image_index(idx)
    t = template(w, h)
    ctx.set_x(K.landmark_rows(K.similarities(frames, idx, w, h, 27), t, LM, L))
    for k, (dtype, layout, channels, order) in enumerate(COMBOS[1:3]):
        for filt in (None, AREA):
            x, alpha, spec = C.tensor(len(idx), w, h, dtype, layout, channels, 31 + k), maps(k, len(idx), w, h), spec_of(layout, order)
            dev = torch.from_numpy(buf).cuda()
            got = ctx.align_paste_tensor(LM, t, torch.from_numpy(x).cuda(), tuples(dev, frames), mask=alpha, filter=filter_of(filt), **spec)
            want = expect(buf, frames, idx, rigid_row(got[0], x, alpha, filt, channels, spec))
            assert np.array_equal(dev.cpu().numpy(), want) and (want != buf).sum() > 500
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- the piecewise-affine paste --------------------------------------------------------------------------------------------------
MESH_ROWS = [0, 1, 5, 6, 7, 2, 1, 5]                               # row -> frame; rows 1 and 6 on frame 1, rows 2 and 7 on frame 5 overlap


def mesh_case(ctx, frames, rows, w, h, seed):
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    x = W.rows_for(frames, rows, idx, t, w, h, seed)
    return idx, t, tri, x, WR.labels(t, tri, w, h)


@pytest.mark.parametrize("filt", [None, AREA])
def test_mesh_at_form_mixed_list(ctx, filt):
    import torch
    buf, frames = PC.place()
    w, h = W.CROPS[0]
    idx, t, tri, rows, lab = mesh_case(ctx, frames, MESH_ROWS, w, h, 40)
    points = WP.points_of(rows, idx)
    mats = WP.matrices(points, t, tri)
    for k, (dtype, layout, channels, order) in enumerate(COMBOS):
        x, alpha, spec = C.tensor(len(MESH_ROWS), w, h, dtype, layout, channels, 90 + k), maps(k, len(MESH_ROWS), w, h), spec_of(layout, order)
        dev = torch.from_numpy(buf).cuda()
        lst, formats, chroma = PC.device_frames(dev, frames)
        got = ctx.warp_paste_tensor_at(points, torch.from_numpy(x).cuda(), lst, formats, image_index=MESH_ROWS, mask=alpha, chroma=chroma,
                                       filter=filter_of(filt), **spec)
        want = expect(buf, frames, MESH_ROWS, mesh_row(points, tri, mats, lab, x, alpha, filt, channels, spec, frames, MESH_ROWS))
        assert np.array_equal(dev.cpu().numpy(), want), (dtype, layout, channels, order)
        assert (want != buf).sum() > 500
        if filt:
            cnt = np.stack([WPA.counts(points[r], tri, mats[r], frames[im]["w"], frames[im]["h"], *filt) for r, im in enumerate(MESH_ROWS)])
            assert np.array_equal(got[1], cnt) and cnt.max() > 1


@pytest.mark.parametrize("filt", [None, AREA])
def test_mesh_fit_form_mixed_list(ctx, filt):
    import torch
    buf, frames = PC.place()
    w, h = W.CROPS[1]
    idx, t, tri, rows, lab = mesh_case(ctx, frames, MESH_ROWS, w, h, 41)
    src = torch.from_numpy(buf).cuda()
    lst, formats, chroma = PC.device_frames(src, frames)
    ctx.set_frames_device(lst, formats, chroma=chroma)
    ctx.set_sample_image_index(MESH_ROWS)
    ctx.set_x(rows)
    points = WP.points_of(rows, idx)
    for k, (dtype, layout, channels, order) in enumerate(COMBOS[:3]):
        x, alpha, spec = C.tensor(len(MESH_ROWS), w, h, dtype, layout, channels, 95 + k), maps(k + 1, len(MESH_ROWS), w, h), spec_of(layout, order)
        dev = torch.from_numpy(buf).cuda()
        dl, df, dc = PC.device_frames(dev, frames)
        got = ctx.warp_paste_tensor(torch.from_numpy(x).cuda(), dl, df, mask=alpha, chroma=dc, filter=filter_of(filt), **spec)
        mats = got[0].reshape(len(MESH_ROWS), -1, 6)
        assert np.array_equal(bits(mats), bits(WP.matrices(points, t, tri)))
        want = expect(buf, frames, MESH_ROWS, mesh_row(points, tri, mats, lab, x, alpha, filt, channels, spec, frames, MESH_ROWS))
        assert np.array_equal(dev.cpu().numpy(), want), (dtype, layout, channels, order)
        assert (want != buf).sum() > 500
    assert np.array_equal(src.cpu().numpy(), buf)
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


def test_mesh_default_distance_plain_calls(ctx):
    """sdm_warp_paste_tensor_at and sdm_warp_paste_tensor on planar destinations without second planes"""
    import torch
    buf, frames = PC.place(DEFAULT, 23)
    rows_to = [0, 1, 4, 1]
    w, h = W.CROPS[0]
    idx, t, tri, rows, lab = mesh_case(ctx, frames, rows_to, w, h, 43)
    points = WP.points_of(rows, idx)
    mats = WP.matrices(points, t, tri)
    src = torch.from_numpy(buf).cuda()
    ctx.set_frames_device(tuples(src, frames))
    ctx.set_sample_image_index(rows_to)
    ctx.set_x(rows)
    for k, (dtype, layout, channels, order) in enumerate(COMBOS[:4]):
        x, alpha, spec = C.tensor(len(rows_to), w, h, dtype, layout, channels, 97 + k), maps(k, len(rows_to), w, h), spec_of(layout, order)
        want = expect(buf, frames, rows_to, mesh_row(points, tri, mats, lab, x, alpha, None, channels, spec, frames, rows_to))
        assert (want != buf).sum() > 500
        for fit in (False, True):
            dev = torch.from_numpy(buf).cuda()
            if fit:
                m, _ = ctx.warp_paste_tensor(torch.from_numpy(x).cuda(), tuples(dev, frames), mask=alpha, **spec)
                assert np.array_equal(bits(m.reshape(len(rows_to), -1, 6)), bits(mats))
            else:
                ctx.warp_paste_tensor_at(points, torch.from_numpy(x).cuda(), tuples(dev, frames), image_index=rows_to, mask=alpha, **spec)
            assert np.array_equal(dev.cpu().numpy(), want), (fit, dtype, layout, channels, order)
    ctx.set_sample_image_index(None)
    ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- the 64-bit plane distance ---------------------------------------------------------------------------------------------------
def test_paste_into_planes_more_than_2_32_bytes_apart(ctx):
    """one untouched allocation of about 8.6 GB; the three planes of a 33 x 21 frame and 64 guard bytes around each are set and read back"""
    import torch
    D = (1 << 32) + (1 << 26) + 3
    w, h, stride, off = 33, 21, 40, 69
    plane = h * stride
    big = torch.empty(2 * D + (1 << 20), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(65)
    small = rng.integers(0, 256, (3, plane + 128), dtype=np.uint8)                   # plane c with its guard bytes, as it lies at off - 64 + c D
    for c in range(3):
        big[off - 64 + c * D:off - 64 + c * D + plane + 128] = torch.from_numpy(small[c]).cuda()
    frame = torch.as_strided(big, (3, h, w), (D, stride, 1), off)
    cw = ch = 16
    f = dict(w=w, h=h)
    mats = np.stack([S.astype(f32) for S in K.similarities([f], [0, 0], cw, ch, 9)])
    x = C.tensor(2, cw, ch, "float16", "nchw", 3, 66)
    alpha = C.alpha_maps(2, cw, ch, 67)
    spec = spec_of("nchw", "rgb")
    ctx.align_paste_tensor_at(mats, torch.from_numpy(x).cuda(), [frame], "rgb_planar", image_index=[0, 0], mask=alpha, **spec)
    st = np.lib.stride_tricks.as_strided
    pix = np.ascontiguousarray(np.stack([st(small[c, 64:], (h, w), (stride, 1)) for c in range(3)], -1))
    for r in range(2):
        P.paste_row(pix, T.RGB, mats[r], x[r], alpha[r], channels=3, **spec)
    want = small.copy()
    for c in range(3):
        st(want[c, 64:], (h, w), (stride, 1))[...] = pix[..., c]
    got = np.stack([big[off - 64 + c * D:off - 64 + c * D + plane + 128].cpu().numpy() for c in range(3)])
    assert (want != small).sum() > 300 and np.array_equal(got, want)
    del big


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_alone(ctx):
    import torch
    buf, frames = PC.place(DEFAULT[:2], 23)
    dev = torch.from_numpy(buf).cuda()
    w = h = 7
    mats = np.stack([S.astype(f32) for S in K.similarities(frames, [0, 1], w, h, 5)])
    x = torch.from_numpy(C.tensor(2, w, h, "uint8", "nhwc", 3, 6)).cuda()
    spec = _lib.paste_tensor_spec("uint8", "nhwc", 3, "bgr")
    paste = _lib.SdmAlignPaste(None, 0)
    flags = np.zeros(2, np.int32)
    lib = _lib.lib()
    p = [dev.data_ptr() + f["off"] for f in frames]
    ok = [(p[0], 37, 29, 38, BP), (p[1], 64, 48, 67, RP)]

    def arr(fs):
        return (_lib.SdmFrame * len(fs))(*[_lib.SdmFrame(*f) for f in fs])

    def at_nv12(fs, planes, n=None):
        uv = None if planes is None else (ctypes.c_void_p * len(planes))(*planes)
        return lib.sdm_align_paste_tensor_at_nv12(ctx._h, mats.ctypes.data, None, 2, w, h, ctypes.byref(spec), None, ctypes.c_void_p(x.data_ptr()),
                                                  ctypes.byref(paste), arr(fs), uv, len(fs) if n is None else n, flags.ctypes.data, None)

    def at_plain(fs, n=None):
        return lib.sdm_align_paste_tensor_at(ctx._h, mats.ctypes.data, None, 2, w, h, ctypes.byref(spec), ctypes.c_void_p(x.data_ptr()),
                                             ctypes.byref(paste), arr(fs), len(fs) if n is None else n, flags.ctypes.data)

    cases = {
        "D == 0": lambda: at_nv12(ok, [None, p[1]]),
        "stride < width": lambda: at_nv12([ok[0], (p[1], 64, 48, 63, RP)], None),
        "stride < width, plain call": lambda: at_plain([ok[0], (p[1], 64, 48, 63, RP)]),
        "null data": lambda: at_plain([(None, 37, 29, 38, BP), ok[1]]),
        "a short list": lambda: at_plain(ok[:1]),
        "a short list, nv12 form": lambda: at_nv12(ok[:1], [None]),
        "no list": lambda: at_nv12(ok, None, 0),
    }
    for name, fn in cases.items():
        assert fn() == _lib.SDM_ERR_INVALID, name
        assert np.array_equal(dev.cpu().numpy(), buf), name
    with pytest.raises(SdmError):
        ctx.align_paste_tensor_at(mats, x, tuples(dev, frames), image_index=[0, 1], layout="nhwc", order="bgr", chroma=[p[0], None])
    assert np.array_equal(dev.cpu().numpy(), buf)
    assert at_plain(ok) == 0 and not np.array_equal(dev.cpu().numpy(), buf)      # (and the valid list of the cases above is accepted)
