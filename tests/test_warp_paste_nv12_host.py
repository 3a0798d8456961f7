"""sdm_warp_paste_tensor_nv12 without a device: the block ownership rule on the mesh's two shapes compiled for the host
(tests/cpp/warp_paste_nv12_host.cpp, address and undefined-behaviour sanitizers, every plane, tensor, label map and opacity map in a
heap block of exactly its bytes, every (row, block) in a shuffled order: once through PasteMesh, once through the adaptor PasteMeshOwn
with the owner's winners from a plain loop) against the numpy restatement (tests/warp_paste_nv12_ref.py), bit for bit in both planes,
pitch padding included; which bytes are stored; the restatement against the one it is built on and against a block worked by hand; what
the cases hold; the Python argument handling.  The kernel's wave-wide cull and its ballots run only in
tests/test_gpu_warp_paste_nv12.py."""
import inspect
import struct

import numpy as np
import pytest

import align_tensor_ref as T
import cpp_build as B
import paste_cases as C
import paste_nv12_cases as V
import paste_nv12_ref as N
import warp_cases as WC
import warp_paste_nv12_cases as M
import warp_paste_nv12_ref as WN
import warp_paste_ref as WP
import warp_ref as R
from superviseddescent_amd import _lib

f32 = np.float32


@pytest.fixture(scope="module")
def calls():
    """the cases and their restatement, computed once: [(case, expected buffer, per-row results)]"""
    return [(c,) + M.expect(c) for c in M.calls()]


def host_cases(calls):
    """one case per (call, NV12 frame): the frame's rows in row order, its planes as blocks of exactly their bytes"""
    out = []
    for k, (c, want, _) in enumerate(calls):
        flags = M.flags(c)
        for i, f in enumerate(c["frames"][:M.NV12_FRAMES]):
            rows = [r for r, im in enumerate(c["idx"]) if im == i]
            yb, ub = V.owned_bytes(f)
            alpha = c["alpha"] if c["alpha"] is None or c["alpha"].ndim == 2 else c["alpha"][rows]
            out.append(dict(c, f=f, rows=rows, pts=c["pts"][rows], x=np.ascontiguousarray(c["x"][rows]), alpha=alpha,
                            mode=0 if alpha is None else 1 if alpha.ndim == 2 else 2, seed=17 * k + i, want_flags=flags[rows],
                            Y=c["buf"][f["off"]:f["off"] + yb].copy(), UV=c["buf"][f["uv_off"]:f["uv_off"] + ub].copy(),
                            want_Y=want[f["off"]:f["off"] + yb], want_UV=want[f["uv_off"]:f["uv_off"] + ub]))
    return out


@pytest.fixture(scope="module")
def ran(tmp_path_factory, calls):
    """the host program built under the sanitizers and run ONCE, as a child process, on every case: [(case, its output per pass)]"""
    tmp = tmp_path_factory.mktemp("warp_paste_nv12")
    exe = B.host_program("warp_paste_nv12_host", tmp)
    cases = host_cases(calls)
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        f = c["f"]
        a = b"" if c["alpha"] is None else c["alpha"].tobytes()
        G, qa, D = R.constants(c["t"], c["tri"])
        consts = np.concatenate([G.reshape(-1, 4), qa, D[:, None]], 1).astype(np.float64)
        blob.append(struct.pack("<15i", f["w"], f["h"], f["stride"], c["cw"], c["ch"], _lib.ALIGN_DTYPES[c["dtype"]],
                                _lib.ALIGN_LAYOUTS[c["layout"]], c["channels"], _lib.ALIGN_ORDERS[c["order"]], c["gray_shift"], len(c["rows"]),
                                c["mode"], c["t"].shape[0], c["tri"].shape[0], c["seed"])
                    + C.SCALES.tobytes() + C.BIASES.tobytes() + c["tri"].tobytes() + consts.tobytes() + c["pts"].astype(f32).tobytes()
                    + struct.pack("<i", c["lab"].size) + c["lab"].tobytes()
                    + struct.pack("<i", c["x"].nbytes) + c["x"].tobytes() + struct.pack("<i", len(a)) + a
                    + struct.pack("<i", c["Y"].size) + c["Y"].tobytes() + struct.pack("<i", c["UV"].size) + c["UV"].tobytes())
    (tmp / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp / "cases.bin", tmp / "out.bin"], 300, sanitized=True)
    got = np.fromfile(str(tmp / "out.bin"), np.uint8)
    at, out = 0, []
    for c in cases:
        n, w, h = len(c["rows"]), c["f"]["w"], c["f"]["h"]
        bw, bh = (w + 1) // 2, (h + 1) // 2
        flags = got[at:at + 4 * n].view(np.int32)
        at += 4 * n
        passes = []
        for _ in range(2):
            o = {}
            for name, size, view, shape in (("stored_y", w * h, np.uint8, (h, w)), ("stored_uv", bw * bh, np.uint8, (bh, bw)),
                                            ("twice", 4, np.int32, ()), ("Y", c["Y"].size, np.uint8, (-1,)), ("UV", c["UV"].size, np.uint8, (-1,))):
                o[name] = got[at:at + size].view(view).reshape(shape)
                at += size
            passes.append(o)
        out.append((c, flags, passes))
    assert at == got.size
    return out


def test_both_shapes_bit_equal_under_sanitizers_in_shuffled_order(ran, calls):
    touched_y = touched_uv = seen = 0
    sizes = set()
    for k, (c, flags, passes) in enumerate(ran):
        f = c["f"]
        what = (k, c["mesh"], f["w"], f["h"], c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"])
        assert np.array_equal(flags, c["want_flags"]), what
        for name, o in zip(("PasteMesh", "PasteMeshOwn"), passes):
            assert int(o["twice"]) == 0, (what, name)                            # a block has one owner
            assert np.array_equal(o["Y"], c["want_Y"]), (what, name)             # (pitch padding is part of the block)
            assert np.array_equal(o["UV"], c["want_UV"]), (what, name)
        touched_y += int((c["want_Y"] != c["Y"]).sum())
        touched_uv += int((c["want_UV"] != c["UV"]).sum())
        sizes.add((f["w"], f["h"]))
        seen |= int(np.bitwise_or.reduce(flags))
    assert touched_y > 5000 and touched_uv > 2000 and seen == WP.DEGENERATE | WP.PARTIAL | WP.FOLDED, (touched_y, touched_uv, seen)
    assert sizes == {(w, h) for w, h, _, _ in V.FRAMES[:V.NV12_FRAMES]}


def test_stores_only_where_an_opacity_is_not_zero(ran, calls):
    """never stored to, not even with the old value: luma pixels whose every a is 0 -- even in a block whose chroma is written --, chroma
    samples whose every a_c is 0, the whole UV plane for a 1-channel tensor"""
    lone = mono = 0
    for k, (c, _, passes) in enumerate(ran):
        res = calls[k // M.NV12_FRAMES][2]
        sy = np.any([res[r][0] > 0 for r in c["rows"]], 0)
        suv = np.any([res[r][3] for r in c["rows"]], 0)
        for o in passes:
            assert np.array_equal(o["stored_y"].astype(bool), sy), k
            assert np.array_equal(o["stored_uv"].astype(bool), suv), k
            if c["channels"] == 1:
                assert not o["stored_uv"].any() and np.array_equal(o["UV"], c["UV"])
        if c["channels"] == 1:
            mono += int(sy.any())
        else:
            some = N.blocks(sy.astype(np.int64))
            lone += int((suv & (some < N.blocks(np.ones(sy.shape, np.int64)))).sum())
    assert lone > 50 and mono >= 7, (lone, mono)


def test_the_cases_meet_their_conditions(calls):
    """what the cases must hold for their own inputs, counted on the restatement (DESIGN 4.21 records the counts)"""
    total = {}
    for c, want, res in calls:
        n = M.conditions(c, want, res)
        print(c["mesh"], (c["cw"], c["ch"]), c["dtype"], c["layout"], c["channels"], c["order"], n)
        for key, v in n.items():
            total[key] = (total.get(key, set()) | v) if isinstance(v, set) else (total.get(key, 0) | v) if key == "flags" else total.get(key, 0) + v
        if c["mesh"] == "words":
            assert n["words"] == {0, 1, 2, 3}, n["words"]                      # winners in each of the four candidate words
        if c["mesh"] != "single":
            assert n["boxed"] > 0                                               # pixels decided by a triangle's box
        if c["channels"] == 3:
            assert n["chroma_without_luma"] > 0 and n["reversed_uv"] > 0
            assert n["disjoint_blocks_uv_order"] > 0 or c["mesh"] == "single"   # (three one-triangle rows seldom share a block so)
        assert n["edge_blocks"] > 0 and n["reversed_y"] > 0
        assert n["two_triangle_blocks"] > 0 or c["mesh"] == "single"
        assert n["flags"] == WP.DEGENERATE | WP.PARTIAL | WP.FOLDED
    print("all calls:", total)
    assert all((v > 0 if not isinstance(v, set) else v == {0, 1, 2, 3}) for v in total.values())


def test_restatement_agrees_with_the_one_it_is_built_on():
    """sample() is what warp_paste_ref.paste_row blends: a BGR, an RGBA and a GRAY frame from its q and a, with 1-channel and "bgr" order
    tensors among them"""
    rng = np.random.default_rng(5)
    w, h = WC.CROPS[0]
    _, t, tri = WC.mesh_rcr22(w, h)
    lab = R.labels(t, tri, w, h)
    S = np.array([[1.1, 0.3, 4.0], [-0.3, 1.2, 6.0]])
    p = (np.asarray(t, np.float64) @ S[:, :2].T + S[:, 2] + rng.uniform(-0.4, 0.4, t.shape)).astype(f32)
    mats = WP.matrices(p, t, tri)[0]
    for (channels, order), (fmt, bpp) in zip(((3, "rgb"), (3, "bgr"), (1, "bgr")), ((T.BGR, 3), (T.RGBA, 4), (T.GRAY, 1))):
        x = C.tensor(1, w, h, "float16", "nchw", channels, 3)[0]
        alpha = C.alpha_maps(1, w, h, 4)[0]
        spec = dict(layout="nchw", channels=channels, order=order, scale=C.SCALES, bias=C.BIASES, gray_shift=15)
        pix = rng.integers(0, 256, (33, 37, bpp), dtype=np.uint8)
        want = pix.copy()
        foot0, a0, tmap0 = WP.paste_row(want, fmt, p, tri, mats, lab, x, alpha, **spec)
        q, a, tmap, foot = WN.sample(p, tri, mats, lab, x, alpha, 33, 37, **spec)
        assert np.array_equal(a, a0) and np.array_equal(tmap, tmap0) and np.array_equal(foot, foot0) and (a > 0).sum() > 100
        got = pix.copy()
        WN.blend_bgr(got, fmt, q, a, channels, 15)
        assert np.array_equal(got, want) and (want != pix).any()


def test_one_block_crossed_by_a_hull_edge_by_hand():
    """a 4 x 4 frame under ONE triangle with corners (0, 0), (3, 0), (0, 3), the template the same points: A_t and W_t are the identity.
    The hull edge x + y = 3 crosses block (1, 0) -- pixels (2, 0), (3, 0), (2, 1), (3, 1): the first three lie on or inside it, (3, 1)
    outside.  By the header's formulas: pixel (3, 1) has a_i = 0 and still counts in cnt."""
    t = np.array([[0, 0], [3, 0], [0, 3]], f32)
    tri = np.array([[0, 1, 2]], np.int32)
    lab = R.labels(t, tri, 4, 4)
    assert lab[0, 2] == 0 and lab[0, 3] == 0 and lab[1, 2] == 0 and lab[1, 3] == R.NONE
    mats = WP.matrices(t, t, tri)[0]
    assert mats.reshape(6).tolist() == [1, 0, 0, 0, 1, 0]
    Y, UV = np.full((4, 4), 50, np.uint8), np.full((2, 2, 2), 90, np.uint8)
    x = np.broadcast_to(np.array([200, 100, 40], np.uint8), (4, 4, 3)).copy()          # B, G, R
    a, tmap, foot, written = WN.paste_row(Y, UV, t, tri, mats, lab, x, None, layout="nhwc", order="bgr")
    # integer positions: one tap of weight 1024 each, opacity 255 on a labelled crop pixel and 0 on label 255
    assert a[0, 2] == 255 and a[0, 3] == 255 and a[1, 2] == 255 and a[1, 3] == 0 and tmap[1, 3] == -1
    yq = (269484 * 40 + 528482 * 100 + 102760 * 200 + (16 << 20) + (1 << 19)) >> 20
    assert yq == 96 and Y[0, 2] == 96 and Y[0, 3] == 96 and Y[1, 2] == 96 and Y[1, 3] == 50
    uq = (460324 * 200 - 305135 * 100 - 155188 * 40 + (128 << 20) + (1 << 19)) >> 20
    vq = (460324 * 40 - 385875 * 100 - 74448 * 200 + (128 << 20) + (1 << 19)) >> 20
    ac = (3 * 255 + 2) // 4                                                              # A = 765 over cnt = 4: the outside pixel counts
    assert ac == 191 and written[0, 1]
    assert UV[0, 1].tolist() == [(ac * uq + (255 - ac) * 90 + 127) // 255, (ac * vq + (255 - ac) * 90 + 127) // 255]
    # block (1, 1) -- pixels (2, 2) ... (3, 3) -- lies wholly outside the hull: neither plane changes there
    assert (Y[2:, 2:] == 50).all() and (UV[1, 1] == 90).all() and not written[1, 1]


def test_symbols_and_python_arguments():
    from superviseddescent_amd import Context, detection_model
    assert {"sdm_warp_paste_tensor_nv12", "sdm_warp_paste_tensor_at_nv12"} <= set(_lib.EXPORTED)
    for fn in (Context.warp_paste_tensor, Context.warp_paste_tensor_at, detection_model.paste_warped_tensor):
        assert inspect.signature(fn).parameters["chroma"].default is None
