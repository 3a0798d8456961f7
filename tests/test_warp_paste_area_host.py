"""sdm_warp_paste_tensor_filtered without a device: properties of the numpy restatement alone (tests/warp_paste_area_ref.py); the pixel
code compiled for the host (tests/cpp/warp_paste_area_host.cpp, address and undefined-behaviour sanitizers, every frame or plane, tensor,
label map and opacity map in a heap block of exactly its bytes, run as a child process) against the restatement, bit for bit: the flags,
A_t, W_t, (Sx, Sy) and every byte the frame owns, with the rows in descending and in ascending order and through both shapes; what the
case list holds; the Python argument handling.  The kernel's wave-wide cull, its ballots and its LDS staging run only in
tests/test_gpu_warp_paste_area.py."""
import inspect
import struct

import numpy as np
import pytest

import align_ref as A
import align_tensor_ref as T
import cpp_build as B
import paste_area_ref as Q
import paste_cases as C
import warp_cases as WC
import warp_paste_area_cases as M
import warp_paste_area_ref as WA
import warp_paste_ref as WP
import warp_ref as R
from superviseddescent_amd import _lib

f32 = np.float32


def through(t, S):
    """K x 2 float32: the template seen through the crop -> frame matrix S"""
    return (np.asarray(t, np.float64) @ S[:, :2].T + S[:, 2]).astype(f32)


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def test_counts_of_a_similarity_equal_the_rigid_paste():
    cw, ch = 48, 40
    _, t, tri = WC.mesh_rcr22(cw, ch)
    for scale, deg, S in ((1 / 0.8, 10.0, 1), (1 / 1.7, -25.0, 2), (1 / 2.6, 40.0, 3), (1 / 5.3, 5.0, 6)):
        Mx = np.concatenate([A.similarity(scale, deg, 0.0, 0.0)[:, :2], [[30.0], [28.0]]], 1).astype(f32)
        p = through(t, Mx.astype(np.float64))
        cnt = WA.counts(p, tri, WP.matrices(p, t, tri)[0], 100, 90)
        assert Q.samples(Mx) == S and (cnt == S).all(), (scale, cnt)
        assert (WA.counts(p, tri, WP.matrices(p, t, tri)[0], 100, 90, WA.BILINEAR) == 1).all()


def squeezed(t, cw, ch, fx=4.0, fy=1.5, at=(40.0, 40.0)):
    return ((np.asarray(t, np.float64) - [(cw - 1) / 2, (ch - 1) / 2]) / [fx, fy] + at).astype(f32)


def test_an_anisotropic_placement_gives_other_counts_per_axis():
    cw, ch = 48, 40
    _, t, tri = WC.mesh_rcr22(cw, ch)
    p = squeezed(t, cw, ch)
    mats = WP.matrices(p, t, tri)[0]
    cnt = WA.counts(p, tri, mats, 100, 90)
    assert (cnt[:, 0] != cnt[:, 1]).all() and np.isin(cnt[:, 0], (4, 5)).all() and (cnt[:, 1] == 2).all(), cnt
    capped = WA.counts(p, tri, mats, 100, 90, WA.AREA, 3, 1.0)
    assert (capped[:, 0] == 3).all() and (capped[:, 1] == 2).all()                # max_samples caps
    gated = WA.counts(p, tri, mats, 100, 90, WA.AREA, 16, 2.0)
    assert np.array_equal(gated[:, 0], cnt[:, 0]) and (gated[:, 1] == 1).all()    # min_scale suppresses: 1.5^2 < 2^2 <= 4^2
    assert (WA.counts(p, tri, mats, 100, 90, WA.AREA, 16, 8.0) == 1).all()
    # a row that pastes nothing has no counts above 1: a NaN landmark, a box outside the frame
    bad = p.copy(); bad[3, 0] = np.nan
    assert (WA.counts(bad, tri, WP.matrices(bad, t, tri)[0], 100, 90) == 1).all()
    assert (WA.counts(p + f32(500), tri, WP.matrices(p + f32(500), t, tri)[0], 100, 90) == 1).all()


def test_a_constant_tensor_pastes_to_that_constant():
    cw, ch = 48, 40
    _, t, tri = WC.mesh_rcr22(cw, ch)
    lab = R.labels(t, tri, cw, ch)
    p = squeezed(t, cw, ch, 3.0, 2.2, (20.0, 14.0))
    mats = WP.matrices(p, t, tri)[0]
    cnt = WA.counts(p, tri, mats, 40, 30)
    assert cnt.min() > 1
    pix = np.random.default_rng(1).integers(0, 256, (30, 40, 3), dtype=np.uint8)
    x = np.broadcast_to(np.array([200, 100, 40], np.uint8), (ch, cw, 3)).copy()
    q, a, tmap, foot, refused, hull = WA.paste_row(pix, T.BGR, p, tri, mats, lab, x, None, cnt, layout="nhwc", order="bgr")
    full = a == 255
    assert full.sum() > 40 and (pix[full] == [200, 100, 40]).all() and not refused.any()
    assert ((a > 0) & (a < 255)).sum() > 10 and hull.sum() > 10                  # the hull's border, antialiased from the inside


# the largest deviation from 127.5 of the filtered restatement on the stripes, where a == 255: observed 0.5, the bound is the next integer
STRIPE_BOUND = 1


def test_stripes_come_out_flat_under_the_filter_and_alias_without():
    cw, ch = 96, 80
    _, t, tri = WC.mesh_rcr22(cw, ch)
    lab = R.labels(t, tri, cw, ch)
    p = squeezed(t, cw, ch, 4.0, 4.0, (15.3, 12.2))                           # (a phase at which four taps do not happen to straddle a stripe)
    mats = WP.matrices(p, t, tri)[0]
    x = np.zeros((1, ch, cw), np.uint8)
    x[:, :, 1::2] = 255                                                        # period 2 along a crop row
    out = {}
    for name, filt in (("area", (WA.AREA, 16, 1.0)), ("bilinear", (WA.BILINEAR, 16, 1.0))):
        pix = np.zeros((26, 32, 1), np.uint8)
        cnt = WA.counts(p, tri, mats, 32, 26, *filt)
        q, a, *_ = WA.paste_row(pix, T.GRAY, p, tri, mats, lab, x, None, cnt, channels=1)
        full = a == 255
        assert full.sum() > 60
        out[name] = float(np.abs(pix[..., 0][full].astype(np.float64) - 127.5).max())
    print("stripes: the largest deviation from 127.5 where a == 255:", out)
    assert out["area"] <= STRIPE_BOUND and out["bilinear"] > STRIPE_BOUND, out


# ---- the host build of the pixel code ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calls():
    """the cases and their restatement, computed once: [(case, expected buffer, per-row results, counts)]"""
    return [(c,) + M.expect(c) for c in M.calls()]


def host_cases(calls):
    """one case per (call, frame): the frame's rows in row order, its bytes as blocks of exactly their size"""
    out = []
    for c, want, res, cnt in calls:
        fl = M.flags(c)
        for i, f in enumerate(c["frames"]):
            rows = [r for r, im in enumerate(c["idx"]) if im == i]
            alpha = c["alpha"] if c["alpha"] is None or c["alpha"].ndim == 2 else c["alpha"][rows]
            out.append(dict(c, f=f, rows=rows, pts=c["pts"][rows], x=np.ascontiguousarray(c["x"][rows]), alpha=alpha,
                            mode=0 if alpha is None else 1 if alpha.ndim == 2 else 2, want_flags=fl[rows], want_counts=cnt[rows],
                            have=[b.copy() for b in M.owned(c, c["buf"], f)], want=M.owned(c, want, f)))
    return out


def test_host_build_bit_equal_under_sanitizers_in_both_orders(tmp_path, calls):
    exe = B.host_program("warp_paste_area_host", tmp_path)
    cases = host_cases(calls)
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        f = c["f"]
        a = b"" if c["alpha"] is None else c["alpha"].tobytes()
        G, qa, D = R.constants(c["t"], c["tri"])
        consts = np.concatenate([G.reshape(-1, 4), qa, D[:, None]], 1).astype(np.float64)
        mode, max_samples, min_scale = c["filter"]
        blob.append(struct.pack("<17if", f["fmt"], f["w"], f["h"], f["stride"], c["cw"], c["ch"], _lib.ALIGN_DTYPES[c["dtype"]],
                                _lib.ALIGN_LAYOUTS[c["layout"]], c["channels"], _lib.ALIGN_ORDERS[c["order"]], c["gray_shift"], len(c["rows"]),
                                c["mode"], c["t"].shape[0], c["tri"].shape[0], mode, max_samples, min_scale)
                    + C.SCALES.tobytes() + C.BIASES.tobytes() + c["tri"].tobytes() + consts.tobytes() + c["pts"].astype(f32).tobytes()
                    + struct.pack("<i", c["lab"].size) + c["lab"].tobytes()
                    + struct.pack("<i", c["x"].nbytes) + c["x"].tobytes() + struct.pack("<i", len(a)) + a
                    + b"".join(struct.pack("<i", b.size) + b.tobytes() for b in c["have"]))
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 600, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at, touched, formats, sizes = 0, 0, set(), set()

    def take(nbytes, view=np.uint8):
        nonlocal at
        at += nbytes
        return got[at - nbytes:at].view(view)

    for k, c in enumerate(cases):
        f, n, Tn = c["f"], len(c["rows"]), c["tri"].shape[0]
        what = (k, c["mesh"], c["list"], f["fmt"], f["w"], f["h"], c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"], c["filter"])
        flags = take(4 * n, np.int32)
        At = take(24 * n * Tn, f32).reshape(n, Tn, 6)
        Wt = take(24 * n * Tn, f32).reshape(n, Tn, 6)
        cnt = take(8 * n * Tn, np.int32).reshape(n, Tn, 2)
        mats = WP.matrices(c["pts"], c["t"], c["tri"])
        assert np.array_equal(flags, c["want_flags"]), what
        assert np.array_equal(cnt, c["want_counts"]), what
        for r in range(n):
            if flags[r] & WP.DEGENERATE:
                assert np.isnan(At[r]).all() and np.isnan(mats[r]).all(), (what, r)
                continue
            assert np.array_equal(At[r].view(np.uint32), mats[r].view(np.uint32)), (what, r)
            W_ref, skipped = WP.inverses(mats[r])
            assert np.array_equal(Wt[r][~skipped].view(np.uint32), W_ref[~skipped].view(np.uint32)), (what, r)
        for name in ("descending, PasteMeshArea", "ascending, PasteMeshAreaOwn"):
            for have, want in zip(c["have"], c["want"]):
                assert np.array_equal(take(have.size), want), (what, name)     # (pitch padding is part of the block)
        touched += sum(int((w != h).sum()) for w, h in zip(c["want"], c["have"]))
        formats.add(f["fmt"])
        sizes.add((f["w"], f["h"]))
    assert at == got.size
    assert touched > 30000 and formats == {T.GRAY, T.BGR, T.RGB, T.BGRA, T.RGBA, T.NV12}, (touched, formats)
    assert sizes >= {(w, h) for w, h, _ in C.FRAMES}


def test_the_case_list_holds_what_it_must(calls):
    """counted on the restatement, so that the list cannot silently lose them"""
    n = dict(aniso=0, mixed=0, cap=0, hull=0, refused=0, flags=0, overlap=0)
    for c, want, res, cnt in calls:
        fl = M.flags(c)
        n["flags"] |= int(np.bitwise_or.reduce(fl))
        n["aniso"] += int((cnt[..., 0] != cnt[..., 1]).sum())                  # triangles with Sx != Sy
        n["cap"] += int((cnt == 16).sum())                                     # a count at the cap of 16
        for r, out in res.items():
            q, a, tmap, foot, refused, hull = out[:6]
            used = np.unique(tmap[foot])
            one = (cnt[r][used] == 1).all(1)
            n["mixed"] += int(one.any() and not one.all())                     # (1, 1) beside counts above 1 among one row's pixels
            n["hull"] += int((hull & (a > 0)).sum())                           # a pixel with a sub-sample on label 255
            n["refused"] += int((refused & foot).sum())                        # a pixel zeroed by the 2^20 rule
        for i in range(len(c["frames"])):
            rows = [r for r in res if c["idx"][r] == i]
            for r, s in zip(rows, rows[1:]):
                both = res[r][3] & res[s][3]
                if both.any() and cnt[r][np.unique(res[r][2][both])].max() != cnt[s][np.unique(res[s][2][both])].max():
                    n["overlap"] += 1                                          # overlapping rows with different counts on one frame
    # every kind of opacity map: none, one for all rows, one per row; and a zero band
    kinds = {None if c["alpha"] is None else c["alpha"].ndim for c, *_ in calls}
    assert kinds == {None, 2, 3}
    assert any(c["alpha"] is not None and c["alpha"].ndim == 2 and (c["alpha"][..., :4] == 0).all() for c, *_ in calls)
    assert any(c["alpha"] is not None and c["alpha"].ndim == 3 and (c["alpha"][..., :4] == 0).all() for c, *_ in calls)
    print(n)
    assert n["flags"] == WP.DEGENERATE | WP.PARTIAL | WP.FOLDED
    assert all(v > 0 for v in n.values()), n


def test_symbols_and_python_arguments():
    from superviseddescent_amd import Context, detection_model
    assert {"sdm_warp_paste_tensor_filtered", "sdm_warp_paste_tensor_at_filtered"} <= set(_lib.EXPORTED)
    for fn in (Context.warp_paste_tensor, Context.warp_paste_tensor_at, detection_model.paste_warped_tensor):
        par = inspect.signature(fn).parameters
        assert par["filter"].default is None and par["max_samples"].default == 16 and par["min_scale"].default == 1.0
