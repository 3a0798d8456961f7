"""The destination frames, meshes, rows, tensors, opacity maps and filters of the filtered piecewise-affine paste (include/sdm.h,
"Pasting warped faces back, filtered") that tests/test_warp_paste_area_host.py runs through the host build of the pixel code and
tests/test_gpu_warp_paste_area.py on the device: the smallest shapes at which the filter really acts.

  lists    "pixel": the seven frames of tests/paste_cases.py (1 x 1 up to 131 x 7, the five per-pixel formats); "nv12": the list of
           tests/paste_nv12_cases.py (seven NV12 surfaces, odd sizes, the UV plane behind Y or apart, then one BGR and one GRAY frame)
  crops    48 x 40 and 96 x 80: crops that really minify on placements a few to 35 frame pixels wide
  meshes   warp_cases.mesh_rcr22 (35 triangles), mesh_single (T = 1), mesh_254 (the LDS bound, four candidate words)
  rows     on every frame five rows that lie over one another (core_rows): a minifying near-similarity; the template squeezed 4 x in x and
           1.5 x in y (Sx = 4, Sy = 2); a face whose x map stretches from 0.15 to 1.3 frame pixels per crop pixel and whose y map
           magnifies, so that triangles at (1, 1) stand beside triangles above 1 in one row; a face 1 / 18 of its crop (the cap of 16);
           and a face squeezed to 2^-22 in x around frame column 0, whose pixels have sub-samples beyond 2^20 crop pixels (refused).  On
           frames 0 and 1 in addition the special rows of tests/test_warp_paste_host.py: wholly outside, a NaN, a flat triangle, a
           folded one, a landmark of 1e30.
  filters  area at 16 sub-samples, area capped at 4, area with min_scale 1.5, in turn
"""
import itertools

import numpy as np

import align_tensor_ref as T
import paste_cases as C
import paste_nv12_cases as V
import warp_cases as WC
import warp_paste_area_ref as WA
import warp_paste_ref as WP
import warp_ref as R
from test_warp_paste_host import special_rows

f32 = np.float32
CROPS = [(48, 40), (96, 80)]
MESHES = {"rcr22": WC.mesh_rcr22, "single": WC.mesh_single, "254": WC.mesh_254}
COMBOS = V.COMBOS
FILTERS = [(WA.AREA, 16, 1.0), (WA.AREA, 4, 1.0), (WA.AREA, 16, 1.5)]
CORE = 5


def core_rows(t, cw, ch, f, rng):
    """the five rows every frame gets, K x 2 float32 each"""
    t = np.asarray(t, np.float64)
    c = np.array([(cw - 1) / 2.0, (ch - 1) / 2.0])
    fc = np.array([(f["w"] - 1) / 2.0, (f["h"] - 1) / 2.0])
    d = t - c
    s = min(30.0, max(8.0, 0.6 * f["w"])) / cw
    co, si = np.cos(np.radians(20.0)), np.sin(np.radians(20.0))
    near = d @ (s * np.array([[co, -si], [si, co]])).T + fc + rng.uniform(-0.2, 0.2, d.shape)
    squeezed = d * np.array([1 / 4.0, 1 / 1.5]) + fc + np.array([1.0, -1.0])
    g = 0.15 * t[:, 0] + 0.575 * t[:, 0] ** 2 / cw                         # dx'/dx from 0.15 to 1.3
    stretched = np.stack([g - 0.3625 * cw + fc[0], 1.1 * d[:, 1] + fc[1]], 1)
    tiny = d / 18.0 + fc + np.array([3.0, 2.0])
    refused = np.stack([d[:, 0] * 2.0 ** -22, 0.5 * d[:, 1] + fc[1]], 1)
    return [np.asarray(p, f32) for p in (near, squeezed, stretched, tiny, refused)]


def rows_of(frames, t, tri, cw, ch, seed):
    """(points N x K x 2 float32, frame of every row)"""
    rng = np.random.default_rng(seed)
    pts, idx = [], []
    for i, f in enumerate(frames):
        rows = core_rows(t, cw, ch, f, rng)
        if i < 2:
            rows += special_rows(rows[0], tri, f)
        pts += rows
        idx += [i] * len(rows)
    return np.stack(pts).astype(f32), idx


def frame_lists():
    bufp, fp = C.place(C.FRAMES, 5)
    for f in fp:
        f["uv_off"] = None
    bufn, fn = V.place()
    return {"pixel": (bufp, fp), "nv12": (bufn, fn)}


def calls():
    """one call per (mesh, crop, list): a combination, a tensor, an opacity map (none, shared, per row; a zero band in turn) and a filter"""
    lists = frame_lists()
    out = []
    for k, (mesh, (cw, ch), name) in enumerate(itertools.product(sorted(MESHES), CROPS, sorted(lists))):
        buf, frames = lists[name]
        dtype, layout, channels, order = COMBOS[(k + k // 6) % len(COMBOS)]
        lm, t, tri = MESHES[mesh](cw, ch)
        tri = np.ascontiguousarray(tri, np.int32)
        pts, idx = rows_of(frames, t, tri, cw, ch, 800 + 10 * k)
        x = C.tensor(len(idx), cw, ch, dtype, layout, channels, 140 + k)
        alpha = [None, C.alpha_maps(1, cw, ch, 150 + k, zero_band=k % 2 == 1)[0], C.alpha_maps(len(idx), cw, ch, 160 + k, zero_band=k == 5)][k % 3]
        out.append(dict(buf=buf, frames=frames, list=name, mesh=mesh, lm=np.asarray(lm), t=np.asarray(t, f32), tri=tri,
                        lab=R.labels(t, tri, cw, ch), cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order,
                        gray_shift=14 if order == "bgr" else 15, pts=pts, idx=idx, x=x, alpha=alpha, filter=FILTERS[k % len(FILTERS)]))
    return out


def spec_of(c):
    return dict(layout=c["layout"], order=c["order"], scale=C.SCALES, bias=C.BIASES, gray_shift=c["gray_shift"])


def alpha_of(c, r):
    return None if c["alpha"] is None else c["alpha"] if c["alpha"].ndim == 2 else c["alpha"][r]


def matrices(c):
    return WP.matrices(c["pts"], c["t"], c["tri"])


def flags(c):
    return WP.flags(c["pts"], c["t"], c["tri"], [(c["frames"][i]["w"], c["frames"][i]["h"]) for i in c["idx"]])


def counts(c, mats=None, filt=None):
    """N x T x 2 int32"""
    mats = matrices(c) if mats is None else mats
    filt = c["filter"] if filt is None else filt
    return np.stack([WA.counts(c["pts"][r], c["tri"], mats[r], c["frames"][i]["w"], c["frames"][i]["h"], *filt) for r, i in enumerate(c["idx"])])


def expect(c, filt=None, order=None, cnt=None):
    """(the restatement on a copy of the buffer: the rows in `order` -- default: row order --, per row what warp_paste_area_ref's paste_row /
    paste_row_nv12 return, the counts N x T x 2)"""
    want, res = c["buf"].copy(), {}
    mats = matrices(c)
    cnt = counts(c, mats, filt) if cnt is None else cnt
    spec = spec_of(c)
    for r in range(len(c["idx"])) if order is None else order:
        f = c["frames"][c["idx"][r]]
        args = (c["pts"][r], c["tri"], mats[r], c["lab"], c["x"][r], alpha_of(c, r), cnt[r])
        if f["fmt"] == T.NV12:
            Y, UV = V.planes(want, f)
            res[r] = WA.paste_row_nv12(Y, UV, *args, channels=c["channels"], **spec)
        else:
            res[r] = WA.paste_row(C.view(want, f), f["fmt"], *args, channels=c["channels"], **spec)
    return want, res, cnt


def owned(c, buf, f):
    """the bytes of frame f inside buf as the host program's blocks: (the frame or its Y plane, the UV plane or nothing)"""
    if f["fmt"] == T.NV12:
        yb, ub = V.owned_bytes(f)
        return buf[f["off"]:f["off"] + yb], buf[f["uv_off"]:f["uv_off"] + ub]
    return buf[f["off"]:f["off"] + C.owned_bytes(f)], buf[:0]


def magnified(c):
    """the call with every row's face LARGER in the frame than in the crop (scale 1.3 about the frame's centre): every count is 1"""
    centre = np.array([(c["cw"] - 1) / 2.0, (c["ch"] - 1) / 2.0])
    pts = []
    for r, i in enumerate(c["idx"]):
        f = c["frames"][i]
        d = (np.asarray(c["t"], np.float64) - centre) * 1.3 + [(f["w"] - 1) / 2.0 + r % 3, (f["h"] - 1) / 2.0 - r % 2]
        pts.append(d)                                                      # (no noise: a sliver's map would minify under it)
    return dict(c, pts=np.stack(pts).astype(f32))


def stacked(name):
    """eight rows of the RCR-22 mesh over one another on the 64 x 48 frame of list `name` alone: a 96 x 80 crop at 1 / 1.2 ... 1 / 6 of its
    size, turned a little more from row to row; one opacity map per row"""
    buf, frames = frame_lists()[name]
    i = next(j for j, f in enumerate(frames) if (f["w"], f["h"]) == (64, 48))
    cw, ch = CROPS[1]
    lm, t, tri = WC.mesh_rcr22(cw, ch)
    tri = np.ascontiguousarray(tri, np.int32)
    rng = np.random.default_rng(21)
    d = np.asarray(t, np.float64) - [(cw - 1) / 2.0, (ch - 1) / 2.0]
    pts = []
    for r, div in enumerate((1.2, 1.8, 2.4, 3.0, 3.6, 4.4, 5.2, 6.0)):
        co, si = np.cos(np.radians(9.0 * r)), np.sin(np.radians(9.0 * r))
        pts.append(d @ (np.array([[co, -si], [si, co]]) / div).T + [31.0 + r, 23.0 - 0.5 * r] + rng.uniform(-0.2, 0.2, d.shape))
    dtype, layout, channels, order = COMBOS[3]
    return dict(buf=buf, frames=frames, list=name, mesh="rcr22", lm=np.asarray(lm), t=np.asarray(t, f32), tri=tri, lab=R.labels(t, tri, cw, ch),
                cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order, gray_shift=14, pts=np.stack(pts).astype(f32),
                idx=[i] * 8, x=C.tensor(8, cw, ch, dtype, layout, channels, 240), alpha=C.alpha_maps(8, cw, ch, 250), filter=FILTERS[0])


def mixed(channels):
    """ONE call on a BGR frame, a GRAY frame at an odd pitch and an NV12 surface whose UV plane lies apart: the core rows on each"""
    buf, frames = V.place([(37, 29, T.BGR, False), (34, 21, T.GRAY, False), (64, 48, T.NV12, True)], 31)
    assert frames[1]["stride"] % 2 == 1 and frames[2]["separate"]
    cw, ch = CROPS[0]
    lm, t, tri = WC.mesh_rcr22(cw, ch)
    tri = np.ascontiguousarray(tri, np.int32)
    pts, idx = rows_of(frames, t, tri, cw, ch, 33)
    dtype, layout, _, order = COMBOS[1]
    return dict(buf=buf, frames=frames, list="mixed", mesh="rcr22", lm=np.asarray(lm), t=np.asarray(t, f32), tri=tri, lab=R.labels(t, tri, cw, ch),
                cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order, gray_shift=15, pts=pts, idx=idx,
                x=C.tensor(len(idx), cw, ch, dtype, layout, channels, 260), alpha=C.alpha_maps(1, cw, ch, 270, zero_band=True)[0],
                filter=FILTERS[0])
