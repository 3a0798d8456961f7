"""The destination frames, meshes, rows, tensors and opacity maps of the piecewise-affine paste into NV12 frames (include/sdm.h, "Pasting
warped faces back into NV12 frames") that tests/test_warp_paste_nv12_host.py runs through the host build of the block code and
tests/test_gpu_warp_paste_nv12.py on the device: the smallest shapes at which the kernel can still go wrong.

  frames   those of tests/paste_nv12_cases.py, cut from ONE noise buffer with 16 guard bytes around each plane: NV12 37 x 29, 64 x 48,
           5 x 4, 2 x 2, 1 x 1, 131 x 7 (wider than one wave's strip of 128 pixels, an odd last block row) and 33 x 21 at odd pitches,
           the UV plane behind Y or apart at a misalignment of its own; one BGR and one GRAY frame in the same list
  crops    24 x 20 and 33 x 17 (tests/warp_cases.py)
  meshes   warp_cases.mesh_single (T = 1), warp_cases.mesh_rcr22 (35 triangles), and mesh_words: 254 triangles with Delaunay triangle i
           at position 3 + 7 i and copies of triangle 0 elsewhere, so that the winners lie in all four 64-bit candidate words
           (warp_cases.mesh_254 cycles the list: its winners are always below 35)
  rows     frame 0: scale 0.3 at 45 degrees, 3 at -45 degrees and 1 (overlapping), then wholly outside, a NaN, a flat triangle, a folded
           one and a landmark of 1e30 -- eight rows; frame 1: the eight far-landmark rows of tests/test_warp_paste_host.py that all span
           the frame (the one-triangle mesh: three similarities); two rows on 131 x 7 and on 33 x 21; one on every other frame
  tensors  one of the six dtype / layout / channel / order combinations of tests/paste_nv12_cases.py per call; no opacity map, one for
           all rows, one per row in turn
"""
import itertools

import numpy as np

import align_tensor_cases as K
import align_tensor_ref as T
import paste_cases as C
import paste_nv12_cases as V
import paste_nv12_ref as N
import warp_cases as WC
import warp_paste_nv12_ref as WN
import warp_paste_ref as WP
import warp_ref as R
from test_warp_paste_host import FAR, placed, spanning_rows, special_rows

f32 = np.float32
CROPS = WC.CROPS
COMBOS = V.COMBOS
NV12_FRAMES = V.NV12_FRAMES


def mesh_words(w, h):
    """254 triangles over the RCR-22 landmarks: Delaunay triangle i at position 3 + 7 i, every other position a copy of triangle 0 (which
    can only ever win at position 0)"""
    idx, t, tri = WC.mesh_rcr22(w, h)
    assert 3 + 7 * (len(tri) - 1) < 254
    out = np.repeat(np.asarray(tri[:1], np.int32), 254, 0)
    out[3 + 7 * np.arange(len(tri))] = tri
    return idx, t, out


MESHES = {"single": WC.mesh_single, "rcr22": WC.mesh_rcr22, "words": mesh_words}


def rows_of(frames, t, tri, cw, ch, seed):
    """(points N x K x 2 float32, frame of every row)"""
    rng = np.random.default_rng(seed)
    pts = [placed(t, S, rng) for S in K.similarities(frames, [0] * 3, cw, ch, seed)]
    pts += special_rows(pts[2], tri, frames[0])
    idx = [0] * len(pts)
    if t.shape[0] == WC.L:
        f = frames[1]
        assert (f["w"], f["h"]) in FAR
        pts += list(spanning_rows(t, f["w"], f["h"], cw, ch, 8, rng))
        idx += [1] * 8
    else:
        pts += [placed(t, S, rng) for S in K.similarities(frames, [1] * 3, cw, ch, seed + 1)]
        idx += [1] * 3
    for i in (2, 3, 4, 5, 5, 6, 6, 7, 8):
        r = sum(1 for j in idx if j == i)
        pts.append(placed(t, K.similarities(frames, [i] * 3, cw, ch, seed + 10 + i)[2 - r], rng))
        idx.append(i)
    return np.stack(pts).astype(f32), idx


def calls():
    """one call per (mesh, crop): the frame list of paste_nv12_cases.place(), a combination, a tensor and an opacity map"""
    buf, frames = V.place()
    out = []
    for k, (mesh, (cw, ch)) in enumerate(itertools.product(sorted(MESHES), CROPS)):
        dtype, layout, channels, order = COMBOS[k]
        lm, t, tri = MESHES[mesh](cw, ch)
        tri = np.ascontiguousarray(tri, np.int32)
        pts, idx = rows_of(frames, t, tri, cw, ch, 700 + 10 * k)
        x = C.tensor(len(idx), cw, ch, dtype, layout, channels, 40 + k)
        alpha = [None, C.alpha_maps(1, cw, ch, 50 + k)[0], C.alpha_maps(len(idx), cw, ch, 60 + k, zero_band=k == 5)][k % 3]
        out.append(dict(buf=buf, frames=frames, mesh=mesh, lm=np.asarray(lm), t=np.asarray(t, f32), tri=tri, lab=R.labels(t, tri, cw, ch),
                        cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order, gray_shift=14 if order == "bgr" else 15,
                        pts=pts, idx=idx, x=x, alpha=alpha))
    return out


def spec_of(c):
    return dict(layout=c["layout"], order=c["order"], scale=C.SCALES, bias=C.BIASES, gray_shift=c["gray_shift"])


def alpha_of(c, r):
    return None if c["alpha"] is None else c["alpha"] if c["alpha"].ndim == 2 else c["alpha"][r]


def matrices(c):
    return WP.matrices(c["pts"], c["t"], c["tri"])


def flags(c):
    return WP.flags(c["pts"], c["t"], c["tri"], [(c["frames"][i]["w"], c["frames"][i]["h"]) for i in c["idx"]])


def expect(c, mats=None, order=None):
    """(the restatement on a copy of the buffer: the rows in `order` -- default: row order --, per row of an NV12 frame what
    warp_paste_nv12_ref.paste_row returns)"""
    want, res = c["buf"].copy(), {}
    mats = matrices(c) if mats is None else np.asarray(mats, f32).reshape(len(c["idx"]), -1, 6)
    spec = spec_of(c)
    for r in range(len(c["idx"])) if order is None else order:
        f = c["frames"][c["idx"][r]]
        if f["fmt"] == T.NV12:
            Y, UV = V.planes(want, f)
            res[r] = WN.paste_row(Y, UV, c["pts"][r], c["tri"], mats[r], c["lab"], c["x"][r], alpha_of(c, r), channels=c["channels"], **spec)
        else:
            WP.paste_row(C.view(want, f), f["fmt"], c["pts"][r], c["tri"], mats[r], c["lab"], c["x"][r], alpha_of(c, r), channels=c["channels"],
                         **spec)
    return want, res


def per_block(v, fill):
    """v (H x W) as ceil(H/2) x ceil(W/2) x 4: the pixels of every 2 x 2 block, a pixel outside the frame reading `fill`"""
    H, Wd = v.shape
    pad = np.full(((H + 1) // 2 * 2, (Wd + 1) // 2 * 2), fill, v.dtype)
    pad[:H, :Wd] = v
    return pad.reshape(pad.shape[0] // 2, 2, pad.shape[1] // 2, 2).transpose(0, 2, 1, 3).reshape(pad.shape[0] // 2, pad.shape[1] // 2, 4)


def conditions(c, want, res):
    """what the issue asks the cases to meet, counted on the restatement of one call"""
    n = dict(edge_blocks=0, two_triangle_blocks=0, disjoint_blocks=0, disjoint_blocks_uv_order=0, chroma_without_luma=0, boxed=0,
             words=set(), flags=0, reversed_y=0, reversed_uv=0)
    mats = matrices(c)
    n["flags"] = int(np.bitwise_or.reduce(flags(c)))
    rev, _ = expect(c, order=range(len(c["idx"]) - 1, -1, -1))
    for i, f in enumerate(c["frames"][:NV12_FRAMES]):
        rows = [r for r in res if c["idx"][r] == i]
        if not rows:
            continue
        cnt = N.blocks(np.ones((f["h"], f["w"]), np.int64))
        held = {r: per_block(res[r][2], False) for r in rows}
        for r in rows:
            a, tmap, foot, written = res[r]
            k = held[r].sum(-1)
            n["edge_blocks"] += int(((k > 0) & (k < cnt)).sum())
            tb = per_block(np.where(foot, tmap, -1), -1)
            lo = np.where(tb >= 0, tb, 1 << 20).min(-1)
            n["two_triangle_blocks"] += int(((tb.max(-1) > lo) & (lo < (1 << 20))).sum())
            n["words"] |= set((np.unique(tmap[foot]) // 64).tolist())
            if not np.isfinite(c["pts"][r]).all() or np.abs(c["pts"][r]).max() < 1e8:
                continue
            free = WP.triangle_map(c["pts"][r], c["tri"], mats[r], f["w"], f["h"], tri_box=False)
            n["boxed"] += int((free != tmap).sum())
        (Yw, UVw), (Yr, UVr) = V.planes(want, f), V.planes(rev, f)
        n["reversed_y"] += int((Yw != Yr).sum())
        n["reversed_uv"] += int((UVw != UVr).any(-1).sum())
        for r, s in itertools.combinations(rows, 2):
            apart = held[r].any(-1) & held[s].any(-1) & ~(held[r] & held[s]).any(-1)
            n["disjoint_blocks"] += int(apart.sum())
            n["disjoint_blocks_uv_order"] += int((apart & (UVw != UVr).any(-1)).sum())
        luma = per_block(np.any([res[r][0] > 0 for r in rows], 0), True)       # (a pixel outside the frame is no unwritten pixel)
        chroma = np.any([res[r][3] for r in rows], 0)
        n["chroma_without_luma"] += int((chroma & ~luma.all(-1)).sum())
    return n
