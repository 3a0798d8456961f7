"""The piecewise-affine face warp without a device (include/sdm.h, "Warped faces"): sdm_warp_delaunay, the properties of the label map as
tests/warp_ref.py restates it, and the per-triangle and per-pixel code of csrc/sdm_warp_device.h compiled for the host
(tests/cpp/warp_host.cpp, address and undefined-behaviour sanitizers, planes of exactly the frames' bytes) against that restatement, bit
for bit."""
import struct

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import warp_cases as W
import warp_ref as R
from superviseddescent_amd import _lib, delaunay, ibug

f32 = np.float32


def orient(p, a, b, c):
    u, v = p[b] - p[a], p[c] - p[a]
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def hull(p):
    """Andrew's monotone chain, float64: (the hull's vertices without collinear ones, its area, whether three hull points are collinear)"""
    order = sorted(range(len(p)), key=lambda k: (p[k, 0], p[k, 1]))
    collinear = False

    def chain(seq):
        nonlocal collinear
        out = []
        for k in seq:
            while len(out) >= 2:
                o = orient(p, out[-2], out[-1], k)
                if o == 0:
                    collinear = True
                if o > 0:
                    break
                out.pop()
            out.append(k)
        return out[:-1]

    h = chain(order) + chain(order[::-1])
    q = p[h]
    area = 0.5 * abs(np.sum(q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1]))
    return h, area, collinear


def in_circle(p, tri):
    """(T x K in-circle determinants of every point against every triangle, T x K magnitudes: the sum of the absolute values of the
    determinant's six products), float64"""
    a, b, c = (p[tri[:, k]][:, None, :] - p[None, :, :] for k in range(3))          # T x K x 2, relative to the tested point
    a2, b2, c2 = ((v ** 2).sum(-1) for v in (a, b, c))
    terms = [a[..., 0] * b[..., 1] * c2, -a[..., 0] * b2 * c[..., 1], -a[..., 1] * b[..., 0] * c2, a[..., 1] * b2 * c[..., 0],
             a2 * b[..., 0] * c[..., 1], -a2 * b[..., 1] * c[..., 0]]
    return sum(terms), sum(np.abs(t) for t in terms)


def check_delaunay(pts):
    p32 = np.asarray(pts, f32)
    p = p32.astype(np.float64)
    tri = delaunay(p32)
    assert np.array_equal(tri, delaunay(p32))                                       # the same input, the same output
    K_ = len(p)
    assert tri.min() >= 0 and tri.max() < K_ and set(tri.reshape(-1)) == set(range(K_))
    d = orient(p, tri[:, 0], tri[:, 1], tri[:, 2])
    assert (d > 0).all()                                                            # counter-clockwise (D > 0), none without area
    h, area, collinear = hull(p)
    if not collinear:
        assert len(tri) == 2 * K_ - 2 - len(h)
    assert abs(0.5 * d.sum() - area) <= 1e-9 * area
    # No point strictly inside a circumcircle.  The inputs are float32, exact in float64; the determinant is a sum of six products of three
    # factors, each factor a difference (or a sum of two squares of differences) rounded to 2^-53 relative: its float64 value is within a
    # few 2^-53 of `mag`, the sum of the products' magnitudes.  1e-9 mag is 10^6 times that rounding error and 10^3 times the library's
    # own tie threshold (1e-12 mag), so a determinant above it is a point inside beyond any rounding.
    det, mag = in_circle(p, tri)
    for k in range(3):
        det[np.arange(len(tri)), tri[:, k]] = 0.0
    assert (det <= 1e-9 * mag).all(), float((det / np.maximum(mag, 1e-300)).max())
    return tri


def test_delaunay_means(built):
    for ids in (ibug.RCR22_IDS, ibug.IBUG68_IDS):
        m = ibug.select_mean(ids)
        n = len(ids)
        check_delaunay(np.stack([m[:n], m[n:]], 1))
    idx, t, tri = W.mesh_rcr22(24, 20)
    assert np.array_equal(tri, check_delaunay(t))


def test_delaunay_random_sets(built):
    rng = np.random.default_rng(1)
    for k in range(200):
        n = 3 + k % 58
        pts = rng.uniform(0, 112, (n, 2)) if k % 3 else rng.integers(0, 12, (n, 2)).astype(np.float64) + rng.uniform(0, 1e-3, (n, 2))
        check_delaunay(pts)


def test_delaunay_cocircular_grid(built):
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0)), -1).reshape(-1, 2) * 7 + 3
    tri = check_delaunay(g)
    assert len(tri) == 32                                                           # 16 squares, two triangles each


def test_delaunay_refusals(built):
    bad = [np.zeros((2, 2)), np.array([[0, 0], [1, 1], [2, 2], [3, 3.0]]), np.array([[0, 0], [1, 0], [1, 0], [0, 1.0]]),
           np.array([[0, 0], [1, 0], [np.nan, 1]])]
    for pts in bad:
        with pytest.raises(_lib.SdmError) as e:
            delaunay(pts)
        assert e.value.code == _lib.SDM_ERR_INVALID
    import ctypes
    p = np.array([[0, 0], [4, 0], [0, 4], [4, 4.5]], f32)
    out, n = np.zeros((2, 3), np.int32), ctypes.c_int(0)
    assert _lib.lib().sdm_warp_delaunay(p.ctypes.data, 4, out.ctypes.data, 1, ctypes.byref(n)) == _lib.SDM_ERR_INVALID
    assert _lib.lib().sdm_warp_delaunay(p.ctypes.data, 4, out.ctypes.data, 2, ctypes.byref(n)) == 0 and n.value == 2


def test_label_map_properties(built):
    for (w, h) in W.CROPS + [(112, 112)]:
        idx, t, tri = W.mesh_rcr22(w, h)
        lab = R.labels(t, tri, w, h)
        e = R.edge_functions(t, tri, w, h)
        jj, ii = np.meshgrid(np.arange(w), np.arange(h))
        on = lab != R.NONE
        assert on.any() and (~on).any()
        assert (e[lab[on], :, ii[on], jj[on]] >= 0).all()                           # every labelled pixel lies in its triangle
        # a pixel inside the hull is labelled: the hull's edge functions, strictly positive with a margin far above rounding
        q = t.astype(np.float64)
        hv, _, _ = hull(q)
        inside = np.ones((h, w), bool)
        for a, b in zip(hv, hv[1:] + hv[:1]):
            inside &= (q[b, 0] - q[a, 0]) * (ii - q[a, 1]) - (q[b, 1] - q[a, 1]) * (jj - q[a, 0]) > 1e-6
        assert inside.sum() >= 50 and on[inside].all()
    # the lowest index on a shared edge, integer template points: the diagonal of a square belongs to triangle 0 whichever comes first
    sq = np.array([[2, 2], [10, 2], [10, 10], [2, 10]], f32)
    for tri in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 3], [0, 1, 2]], [[0, 2, 1], [0, 3, 2]]):          # (the last: both clockwise as given)
        lab = R.labels(sq, np.array(tri), 13, 13)
        d = np.arange(2, 11)
        assert (lab[d, d] == 0).all()
        assert (lab[2:11, 2:11] != R.NONE).all() and (lab[:2] == R.NONE).all() and (lab[:, 11:] == R.NONE).all()
        assert set(np.unique(lab)) == {0, 1, R.NONE}
    # overlapping triangles: the lowest index wins everywhere
    lab = R.labels(sq, np.array([[0, 1, 2], [0, 1, 2], [0, 2, 3]]), 13, 13)
    assert set(np.unique(lab)) == {0, 2, R.NONE}


def border_matrices(f, w, h, T_):
    """T_ matrices that send taps across every border of frame f: identity-like maps shifted past the left, right, top and bottom edges,
    a large magnification, a position beyond 2^20 and a NaN"""
    out = []
    for k in range(T_):
        dx, dy = [(-3.4, 1.2), (f["w"] - w + 3.7, 0.4), (0.6, -2.3), (1.1, f["h"] - h + 2.8)][k % 4]
        s = [1.0, 0.53, 1.9][k % 3]
        out.append([s, 0.07 * (k % 5), dx, -0.05 * (k % 3), s, dy])
    m = np.array(out, f32)
    if T_ > 6:
        m[5, 2] = 3e6
        m[6, 0] = np.nan
    return m


def test_host_build_of_the_warp_code_under_sanitizers(built, tmp_path):
    exe = B.host_program("warp_host", tmp_path)
    scale, bias = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], f32), np.array([-2.1179, -2.0357, -1.8044], f32)
    # ---- the fit of a triangle: the rows of the device test, one folded and one flat triangle among them
    w, h = W.CROPS[0]
    buf, frames = W.place()
    idx, t, tri = W.mesh_rcr22(w, h)
    x = W.rows_for(frames, W.ROWS, idx, t, w, h, 3)
    x[1, [idx[tri[0, 1]], idx[tri[0, 2]]]] = x[1, [idx[tri[0, 2]], idx[tri[0, 1]]]]
    x[1, [W.L + idx[tri[0, 1]], W.L + idx[tri[0, 2]]]] = x[1, [W.L + idx[tri[0, 2]], W.L + idx[tri[0, 1]]]]
    x[2, idx[tri[1, 1]]], x[2, W.L + idx[tri[1, 1]]] = x[2, idx[tri[1, 0]]], x[2, W.L + idx[tri[1, 0]]]
    G, qa, D = R.constants(t, tri)
    fits = [struct.pack("<i", len(x) * len(tri))]
    for n in range(len(x)):
        for k, (a, b, c) in enumerate(tri):
            fits.append(G[k].tobytes() + qa[k].tobytes() + struct.pack("<d", D[k])
                        + np.array([[x[n, idx[v]], x[n, W.L + idx[v]]] for v in (a, b, c)], f32).tobytes())
    want_m = R.matrices(x, idx, t, tri)
    want_f = R.flags(x, idx, t, tri, [(10 ** 6, 10 ** 6)] * len(x))
    want_f &= R.FOLDED                                                              # (PARTIAL needs the frames: the device test)
    assert want_f[1] and want_f[2] and not want_f[0] and not want_f[3:].any()
    # ---- the pixels: every frame of both sets through fitted matrices and through matrices that cross every border
    cases, blob, seen = [], [b""], set()
    for (w, h) in W.CROPS:
        idx, t, tri = W.mesh_254(w, h) if (w, h) == W.CROPS[1] else W.mesh_rcr22(w, h)
        lab = R.labels(t, tri, w, h)
        assert (lab == R.NONE).any()
        for frames_, buf_, rows in ((frames, buf, W.ROWS),) + tuple((fr, bf, range(len(fr))) for bf, fr in (K.place(K.RAGGED, 11), K.place(K.NV12, 12))):
            xs = W.rows_for(frames_, rows, idx, t, w, h, 7 + w)
            fitted = R.matrices(xs, idx, t, tri)
            for r, im in enumerate(rows):
                f = frames_[im]
                for mats in (fitted[r], border_matrices(f, w, h, len(tri))):
                    b0, b1 = K.plane_bytes(f)
                    blob.append(struct.pack("<8i", f["fmt"], f["w"], f["h"], f["stride"], f["stride"] if b1 else 0, w, h, len(tri))
                                + mats.tobytes() + lab.tobytes() + scale.tobytes() + bias.tobytes()
                                + struct.pack("<i", b0) + buf_[f["off"]:f["off"] + b0].tobytes()
                                + struct.pack("<i", b1) + (buf_[f["uv_off"]:f["uv_off"] + b1].tobytes() if b1 else b""))
                    cases.append((K.host_frame(buf_, f), mats, lab))
                    seen.add(f["fmt"])
    assert seen == set(range(6))
    blob[0] = struct.pack("<i", len(cases))
    (tmp_path / "cases.bin").write_bytes(b"".join(fits) + b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 300, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    nf = want_m.shape[0] * want_m.shape[1]
    rec = got[:nf * 28].reshape(nf, 28)
    assert np.array_equal(rec[:, :24].copy().view(np.uint32), want_m.reshape(nf, 6).view(np.uint32))
    folded = rec[:, 24:].copy().view(np.int32).reshape(want_m.shape[:2])
    assert np.array_equal(np.where(folded.any(1), R.FOLDED, 0), want_f)
    at = nf * 28
    for frame, mats, lab in cases:
        h, w = lab.shape
        kind, bgr, y = R.warped(frame, mats, lab)
        n = w * h
        assert np.array_equal(got[at:at + 3 * n].reshape(h, w, 3), bgr), (frame.fmt, frame.w, frame.h, w, h)
        assert not bgr[lab == R.NONE].any()
        at += 3 * n
        for shift in (14, 15):
            want = T.finish(kind, bgr, y, "uint8", "nhwc", 1, "bgr", gray_shift=shift)[..., 0]
            assert np.array_equal(got[at:at + n].reshape(h, w), want), (frame.fmt, shift)
            at += n
        want = T.finish(kind, bgr, None, "float32", "nchw", 3, "rgb", scale, bias)
        assert np.array_equal(got[at:at + 12 * n].copy().view(np.uint32).reshape(3, h, w), want.view(np.uint32)), frame.fmt
        at += 12 * n
    assert at == got.size
