"""sdm_align_paste_tensor_nv12 without a device: the block ownership rule and the luma / chroma arithmetic compiled for the host
(tests/cpp/align_paste_nv12_host.cpp, address and undefined-behaviour sanitizers, every plane, tensor and opacity map in a heap block of
exactly its bytes, every (row, block) in a shuffled order) against the numpy restatement (tests/paste_nv12_ref.py), bit for bit in both
planes, pitch padding included; which bytes are stored; the restatement against the two it is built on and against a block worked by
hand; the round trip's deviation; the Python argument handling."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

import align_ref as A
import align_tensor_ref as T
import cpp_build as B
import paste_area_ref as Q
import paste_cases as C
import paste_nv12_cases as V
import paste_nv12_ref as N
import paste_ref as P
from superviseddescent_amd import _lib

f32 = np.float32


def host_cases():
    """one case per (call, NV12 frame): the frame's rows in row order, its planes as blocks of exactly their bytes"""
    out = []
    for k, c in enumerate(V.calls()):
        for i, f in enumerate(c["frames"][:V.NV12_FRAMES]):
            rows = [r for r, im in enumerate(c["idx"]) if im == i]
            yb, ub = V.owned_bytes(f)
            alpha = c["alpha"] if c["alpha"] is None or c["alpha"].ndim == 2 else c["alpha"][rows]
            out.append(dict(c, f=f, mats=c["mats"][rows], x=np.ascontiguousarray(c["x"][rows]), alpha=alpha,
                            mode=0 if alpha is None else 1 if alpha.ndim == 2 else 2, seed=17 * k + i,
                            Y=c["buf"][f["off"]:f["off"] + yb].copy(), UV=c["buf"][f["uv_off"]:f["uv_off"] + ub].copy()))
    return out


def plane_views(c, Y, UV):
    return V.planes(np.concatenate([Y, UV]), dict(c["f"], off=0, uv_off=Y.size))


def restate(c):
    """(Y bytes, UV bytes, S per row, luma pixels some row stores, chroma samples some row stores) of the restatement"""
    f = c["f"]
    both = np.concatenate([c["Y"], c["UV"]])
    Y, UV = V.planes(both, dict(f, off=0, uv_off=c["Y"].size))
    spec = V.spec_of(c)
    S, sy, suv = [], np.zeros(Y.shape, bool), np.zeros(UV.shape[:2], bool)
    for r, m in enumerate(c["mats"]):
        degenerate = P.inverse(m)[1]
        S.append(1 if c["filter"] is None or degenerate else Q.samples(m, *c["filter"]))
        a = N.paste_row(Y, UV, m, c["x"][r], None if c["alpha"] is None else c["alpha"][r] if c["mode"] == 2 else c["alpha"], S[-1],
                        channels=c["channels"], **spec)
        sy |= a > 0
        if c["channels"] == 3:
            blk = N.blocks(a)
            suv |= (blk > 0) & ((blk + N.blocks(np.ones_like(a)) // 2) // N.blocks(np.ones_like(a)) > 0)
    return both[:c["Y"].size], both[c["Y"].size:], S, sy, suv


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    """the host program built under the sanitizers and run ONCE, as a child process, on every case: [(case, its output)]"""
    tmp = tmp_path_factory.mktemp("paste_nv12")
    exe = B.host_program("align_paste_nv12_host", tmp)
    cases = host_cases()
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        f = c["f"]
        a = b"" if c["alpha"] is None else c["alpha"].tobytes()
        mode, cap, gate = c["filter"] or (0, 16, 1.0)
        blob.append(struct.pack("<16if", f["w"], f["h"], f["stride"], c["cw"], c["ch"], _lib.ALIGN_DTYPES[c["dtype"]],
                                _lib.ALIGN_LAYOUTS[c["layout"]], c["channels"], _lib.ALIGN_ORDERS[c["order"]], c["gray_shift"], len(c["mats"]),
                                c["mode"], int(c["filter"] is not None), mode, cap, c["seed"], gate)
                    + C.SCALES.tobytes() + C.BIASES.tobytes() + c["mats"].tobytes()
                    + struct.pack("<i", c["x"].nbytes) + c["x"].tobytes() + struct.pack("<i", len(a)) + a
                    + struct.pack("<i", c["Y"].size) + c["Y"].tobytes() + struct.pack("<i", c["UV"].size) + c["UV"].tobytes())
    (tmp / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp / "cases.bin", tmp / "out.bin"], 300, sanitized=True)
    got = np.fromfile(str(tmp / "out.bin"), np.uint8)
    at, out = 0, []
    for c in cases:
        n, w, h = len(c["mats"]), c["f"]["w"], c["f"]["h"]
        bw, bh = (w + 1) // 2, (h + 1) // 2
        o = {}
        for name, size, view, shape in (("flags", 4 * n, np.int32, (n,)), ("S", 4 * n, np.int32, (n,)), ("stored_y", w * h, np.uint8, (h, w)),
                                        ("stored_uv", bw * bh, np.uint8, (bh, bw)), ("twice", 4, np.int32, ()),
                                        ("Y", c["Y"].size, np.uint8, (-1,)), ("UV", c["UV"].size, np.uint8, (-1,))):
            o[name] = got[at:at + size].view(view).reshape(shape)
            at += size
        out.append((c, o, restate(c)))
    assert at == got.size
    return out


def test_both_planes_bit_equal_under_sanitizers_in_shuffled_order(ran):
    touched_y = touched_uv = 0
    sizes, samples, seen = set(), set(), 0
    for k, (c, o, (wy, wuv, S, _, _)) in enumerate(ran):
        f = c["f"]
        what = (k, f["w"], f["h"], c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"], c["filter"])
        for r, m in enumerate(c["mats"]):
            assert o["flags"][r] == P.flags_at(m, c["cw"], c["ch"], f["w"], f["h"]), (what, r)
        assert o["S"].tolist() == S, what
        assert int(o["twice"]) == 0, what                                        # a block has one owner
        assert np.array_equal(o["Y"], wy), what                                  # (pitch padding is part of the block)
        assert np.array_equal(o["UV"], wuv), what
        touched_y += int((wy != c["Y"]).sum())
        touched_uv += int((wuv != c["UV"]).sum())
        sizes.add((f["w"], f["h"]))
        samples |= set(S)
        seen |= int(o["flags"].max())
    assert touched_y > 5000 and touched_uv > 2000 and samples >= {1, 2, 3} and seen == A.DEGENERATE | A.PARTIAL
    assert sizes == {(w, h) for w, h, _, _ in V.FRAMES[:V.NV12_FRAMES]}


def test_stores_only_where_an_opacity_is_not_zero(ran):
    """never stored to, not even with the old value: luma pixels whose every a is 0 -- even in a block whose chroma is written --, chroma
    samples whose every a_c is 0, the whole UV plane for a 1-channel tensor"""
    lone = mono = 0
    for k, (c, o, (_, _, _, sy, suv)) in enumerate(ran):
        assert np.array_equal(o["stored_y"].astype(bool), sy), k
        assert np.array_equal(o["stored_uv"].astype(bool), suv), k
        if c["channels"] == 1:
            assert not o["stored_uv"].any() and np.array_equal(o["UV"], c["UV"]) and sy.any()
            mono += 1
        else:
            some = N.blocks(sy.astype(np.int64))
            lone += int((suv & (some < N.blocks(np.ones(sy.shape, np.int64)))).sum())     # a written sample with an unwritten luma pixel
    assert lone > 50 and mono >= 7


def test_overlap_order_and_half_cut_blocks_are_in_the_cases(ran):
    """the cases cannot pass by accident: on frame 0 of the first call rows overlap with partial opacity so that the reverse order gives
    other bytes in BOTH planes, and a footprint edge cuts blocks in half"""
    c = ran[V.NV12_FRAMES][0]                                                     # the second call (one opacity map for all rows), frame 0
    assert c["channels"] == 3 and c["mode"] == 1 and c["f"]["w"] == 37
    spec = V.spec_of(c)
    both = np.concatenate([c["Y"], c["UV"]])

    def run(order):
        b = both.copy()
        Y, UV = V.planes(b, dict(c["f"], off=0, uv_off=c["Y"].size))
        return b, [N.paste_row(Y, UV, c["mats"][r], c["x"][r], c["alpha"], 1, channels=3, **spec) for r in order]
    fwd, a = run(range(len(c["mats"])))
    back, _ = run(range(len(c["mats"]) - 1, -1, -1))
    edge = N.paste_row(*V.planes(both.copy(), dict(c["f"], off=0, uv_off=c["Y"].size)), c["mats"][3], c["x"][3], None, 1, channels=3, **spec)
    ny = c["Y"].size
    assert not np.array_equal(fwd[:ny], back[:ny]) and not np.array_equal(fwd[ny:], back[ny:])
    partial = [(x > 0) & (x < 255) for x in a[:3]]
    assert (partial[0] & partial[1] & partial[2]).any()                           # a pixel under three rows, none of them opaque
    held = N.blocks((edge > 0).astype(np.int64))                                 # the translation to odd coordinates
    assert ((held > 0) & (held < 4)).sum() >= (c["cw"] + c["ch"]) // 2           # one edge across and one down, in blocks


def test_restatement_agrees_with_the_ones_it_is_built_on():
    """sample() is what paste_ref.paste_row and paste_area_ref.paste_row blend: their BGR frames from its q and a"""
    rng = np.random.default_rng(5)
    for S, M in ((1, A.similarity(1.3, 20.0, 3.0, 2.0)), (1, A.similarity(0.4, -30.0, 9.0, 5.0)), (3, A.similarity(0.4, -30.0, 9.0, 5.0))):
        M = M.astype(f32)
        for channels, order in ((3, "rgb"), (3, "bgr"), (1, "bgr")):
            x = C.tensor(1, 16, 12, "float16", "nchw", channels, 3)[0]
            alpha = C.alpha_maps(1, 16, 12, 4)[0]
            spec = dict(layout="nchw", channels=channels, order=order, scale=C.SCALES, bias=C.BIASES)
            pix = rng.integers(0, 256, (21, 33, 3), dtype=np.uint8)
            want = pix.copy()
            a0 = Q.paste_row(want, T.BGR, M, x, alpha, S, **spec)
            q, a = N.sample(M, x, alpha, S, 21, 33, **spec)
            assert np.array_equal(a, a0) and a.any()
            got = np.where((a > 0)[..., None], N.blend(a[..., None], np.broadcast_to(q, (21, 33, 3)), pix.astype(np.int64)), pix)
            assert np.array_equal(got, want)


def test_one_block_by_hand():
    """a 3 x 3 frame, M the identity, a 2 x 2 crop of one colour with opacity 255, 255, 128, 0: block (0, 0) by the section's formulas"""
    Y, UV = np.full((3, 3), 50, np.uint8), np.full((2, 2, 2), 90, np.uint8)
    x = np.broadcast_to(np.array([200, 100, 40], np.uint8), (2, 2, 3)).copy()          # B, G, R
    alpha = np.array([[255, 255], [128, 0]], np.uint8)
    a = N.paste_row(Y, UV, np.array([[1, 0, 0], [0, 1, 0]], f32), x, alpha, 1, layout="nhwc", order="bgr")
    assert a[:2, :2].tolist() == [[255, 255], [128, 0]] and not a[2].any() and not a[:, 2].any()
    yq = (269484 * 40 + 528482 * 100 + 102760 * 200 + (16 << 20) + (1 << 19)) >> 20
    assert yq == 96 and Y.tolist() == [[96, 96, 50], [(128 * 96 + 127 * 50 + 127) // 255, 50, 50], [50, 50, 50]]
    uq = (460324 * 200 - 305135 * 100 - 155188 * 40 + (128 << 20) + (1 << 19)) >> 20
    vq = (460324 * 40 - 385875 * 100 - 74448 * 200 + (128 << 20) + (1 << 19)) >> 20
    ac = (638 + 2) // 4                                                                  # A = 638 over cnt = 4 pixels
    assert UV[0, 0].tolist() == [(ac * uq + (255 - ac) * 90 + 127) // 255, (ac * vq + (255 - ac) * 90 + 127) // 255]
    assert (UV[0, 1] == 90).all() and (UV[1] == 90).all()
    # the edge sample (1, 1) of the 3 x 3 frame belongs to ONE pixel: cnt = 1, so a = 255 there replaces the sample
    Y2, UV2 = np.full((3, 3), 50, np.uint8), np.full((2, 2, 2), 90, np.uint8)
    N.paste_row(Y2, UV2, np.array([[1, 0, 2], [0, 1, 2]], f32), x, None, 1, layout="nhwc", order="bgr")
    assert Y2[2, 2] == 96 and UV2[1, 1].tolist() == [uq, vq] and (UV2[0] == 90).all() and (UV2[1, 0] == 90).all()


def round_trip_deviation():
    """(largest luma deviation, largest chroma deviation) of decode-then-paste on whole frames: every pixel of an NV12 frame through the
    crop call's BT.601 decode, pasted back with M the identity at full opacity, the planes compared with what they were"""
    dy = duv = pixels = samples = 0
    buf, frames = V.place()
    for f in frames[:V.NV12_FRAMES]:
        Y, UV = (p.copy() for p in V.planes(buf, f))
        bgr = N.bgr_of(Y, UV).astype(np.uint8)
        y2, uv2 = Y.copy(), UV.copy()
        a = N.paste_row(y2, uv2, np.array([[1, 0, 0], [0, 1, 0]], f32), bgr, None, 1, layout="nhwc", order="bgr")
        assert (a == 255).all()
        # noise planes hold values outside the limited range (Y < 16 or > 235, colours that clip): only in-range pixels are comparable
        terms = T.nv12_terms(Y, np.repeat(np.repeat(UV[..., 0], 2, 0), 2, 1)[:f["h"], :f["w"]],
                               np.repeat(np.repeat(UV[..., 1], 2, 0), 2, 1)[:f["h"], :f["w"]])[1]
        unclipped = (Y >= 16) & (Y <= 235)
        for s in (terms[0], terms[3], terms[4]):
            unclipped &= (s >> 20 >= 0) & (s >> 20 <= 255)
        if unclipped.any():
            dy = max(dy, int(np.abs(y2.astype(int) - Y)[unclipped].max()))
        whole = N.blocks(unclipped.astype(np.int64)) == N.blocks(np.ones(Y.shape, np.int64))
        if whole.any():
            duv = max(duv, int(np.abs(uv2.astype(int) - UV)[whole].max()))
        pixels, samples = pixels + int(unclipped.sum()), samples + int(whole.sum())
    return dy, duv, pixels, samples


def test_round_trip_deviation_of_the_conversion_pair():
    dy, duv, pixels, samples = round_trip_deviation()
    print("round trip of the integer conversion pair: luma deviates by at most", dy, "chroma by at most", duv, "over", pixels, "pixels and",
          samples, "whole blocks inside the limited range and the BGR gamut")
    # the restatement's own figures (DESIGN 4.20 records them): the Q20 encode constants invert the Q20 decode constants exactly there
    assert pixels > 500 and samples > 20 and (dy, duv) == (0, 0)


def test_symbols_and_python_arguments():
    from superviseddescent_amd import Context, detection_model
    assert {"sdm_align_paste_tensor_nv12", "sdm_align_paste_tensor_at_nv12"} <= set(_lib.EXPORTED)
    for fn in (Context.align_paste_tensor, Context.align_paste_tensor_at, detection_model.paste_crops_tensor):
        assert inspect.signature(fn).parameters["chroma"].default is None
    F = _lib.SdmFrame
    bgr = (F * 1)(F(ctypes.c_void_p(64), 4, 4, 12, _lib.SDM_FRAME_BGR))
    nv = (F * 2)(F(ctypes.c_void_p(64), 4, 4, 12, _lib.SDM_FRAME_BGR), F(ctypes.c_void_p(640), 4, 4, 4, _lib.SDM_FRAME_NV12))
    assert Context._paste_chroma(None, bgr, ()) is None                        # no NV12, no chroma: the calls as they were
    assert Context._paste_chroma(None, nv, ())[0] is None
    uv = Context._paste_chroma([None, 4096], nv, ())[0]
    assert uv[0] is None and uv[1] == 4096
    assert Context._paste_chroma([None], bgr, ())[0][0] is None                # chroma given: the NV12 entry point
    with pytest.raises(ValueError):
        Context._paste_chroma([None], nv, ())
