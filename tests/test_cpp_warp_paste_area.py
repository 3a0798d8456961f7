"""The rcr::paste_warped_tensor overloads that take an rcr::AlignFilter (superviseddescent_amd/include/rcr/warp.hpp,
tests/cpp/warp_paste_area_gpu.cpp): landmark rows on NV12 DeviceFrames -- the UV plane behind Y or in an allocation of its own -- and a
BGR one in one list give, through the fit and through explicit points, the bytes, flags and counts of the Python call
(Context.warp_paste_tensor_at(filter="area")) and of the restatement (tests/warp_paste_area_ref.py); the tracker's overload, behind one
step on the same frames, gives the bytes of the Python call on the tracker's own rows."""
import os

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import paste_cases as C
import paste_nv12_cases as V
import warp_paste_area_ref as WA
import warp_paste_ref as WP
import warp_ref as R


def test_cpp_driver_compiles(tmp_path):
    """the new overloads and their driver build against the headers without a device"""
    B.gpu_driver("warp_paste_area_gpu", tmp_path, link=False)


@pytest.mark.gpu
def test_cpp_filtered_warp_paste_matches_the_python_call(built, tmp_path):
    from superviseddescent_amd import HoGParam, alignment_template, delaunay
    from test_gpu_align_tensor import IDS as ids, L, MEAN as mean
    LM = np.arange(L)                                          # the RCR-22 mesh: every landmark
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    buf, frames = V.place([V.FRAMES[0], V.FRAMES[1], V.FRAMES[7], V.FRAMES[6]], 17)
    w, h, S = 48, 40, 4                                        # larger than the faces: the way back minifies
    tmpl = alignment_template(mean, LM, w, h, 0.1)
    tri = delaunay(tmpl)
    lab = R.labels(tmpl, tri, w, h)
    x = K.landmark_rows(K.similarities(frames, range(S), w, h, 18), tmpl, LM, L)
    x[:, :L] = x[:, :L].mean(1, keepdims=True) + np.float32(0.7) * (x[:, :L] - x[:, :L].mean(1, keepdims=True))      # narrower: Sx != Sy
    y = C.tensor(S, w, h, "float16", "nchw", 3, 19)
    alpha = C.alpha_maps(S, w, h, 20, zero_band=True)
    d = str(tmp_path)
    B.write_model(d, L, params, mean, ids)
    meta = [f"{S} {w} {h} {len(LM)} " + " ".join(map(str, LM)) + "\n"]

    def planes_of(b):
        """the frames' bytes as the driver lays them out: plane 0 (h rows of the pitch), then the UV plane"""
        out = []
        for fr in frames:
            out.append(b[fr["off"]:fr["off"] + fr["h"] * fr["stride"]])
            if fr["fmt"] == T.NV12:
                out.append(b[fr["uv_off"]:fr["uv_off"] + (fr["h"] + 1) // 2 * fr["stride"]])
        return np.concatenate(out)

    full = np.concatenate([buf, np.zeros(256, np.uint8)])                        # (whole pitches of the last plane lie inside)
    planes_of(full).tofile(os.path.join(d, "frames.u8"))
    for fr in frames:
        nv = fr["fmt"] == T.NV12
        meta.append(f"{fr['fmt']} {fr['w']} {fr['h']} {fr['stride']} {fr['h'] * fr['stride']} "
                    f"{(fr['h'] + 1) // 2 * fr['stride'] if nv else 0} {int(nv and fr['separate'])}\n")
    x.tofile(os.path.join(d, "rows.f32"))
    tmpl.tofile(os.path.join(d, "tmpl.f32"))
    y.tofile(os.path.join(d, "tensor.f16"))
    alpha.tofile(os.path.join(d, "alpha.u8"))
    side = [int(0.6 * min(fr["w"], fr["h"])) for fr in frames]                  # the tracker's start boxes: centred, smaller than the crop
    np.array([[(fr["w"] - b) // 2, (fr["h"] - b) // 2, b, b] for fr, b in zip(frames, side)], np.int32).tofile(os.path.join(d, "boxes.i32"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("".join(meta))
    B.run(B.gpu_driver("warp_paste_area_gpu", tmp_path), [d], 300)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    pts = WP.points_of(x, LM)
    mats = WP.matrices(pts, tmpl, tri)
    assert rd("mats.f32", np.uint32).tobytes() == mats.tobytes()
    flags = WP.flags(pts, tmpl, tri, [(fr["w"], fr["h"]) for fr in frames])
    assert np.array_equal(rd("flags.i32", np.int32), flags) and np.array_equal(rd("flags_at.i32", np.int32), flags)
    cnt = np.stack([WA.counts(pts[r], tri, mats[r], fr["w"], fr["h"]) for r, fr in enumerate(frames)])
    assert (cnt > 1).any() and (cnt[..., 0] != cnt[..., 1]).any()
    assert np.array_equal(rd("samples.i32", np.int32).reshape(cnt.shape), cnt) and np.array_equal(rd("samples_at.i32", np.int32).reshape(cnt.shape), cnt)
    spec = dict(scale=C.SCALES, bias=C.BIASES)
    want = full.copy()
    for r, fr in enumerate(frames):
        if fr["fmt"] == T.NV12:
            WA.paste_row_nv12(*V.planes(want, fr), pts[r], tri, mats[r], lab, y[r], alpha[r], cnt[r], **spec)
        else:
            WA.paste_row(C.view(want, fr), fr["fmt"], pts[r], tri, mats[r], lab, y[r], alpha[r], cnt[r], **spec)
    assert (want != full).sum() > 500
    # the Python call on the same frames, rows, tensor and maps
    import torch
    from superviseddescent_amd import Context, ibug
    ctx = Context(0)
    try:
        ctx.set_model_geometry(L, *ibug.eye_indices(ids), params)
        ctx.warp_set_mesh(LM, tmpl, tri, w, h)
        dev = torch.from_numpy(full).cuda()
        lst = [(dev.data_ptr() + fr["off"], fr["w"], fr["h"], fr["stride"], K.NAMES[fr["fmt"]]) for fr in frames]
        chroma = [dev.data_ptr() + fr["uv_off"] if fr["fmt"] == T.NV12 and fr["separate"] else None for fr in frames]
        pf, ps = ctx.warp_paste_tensor_at(pts, torch.from_numpy(y).cuda(), lst, mask=torch.from_numpy(alpha).cuda(), chroma=chroma,
                                          filter="area", **spec)
        python = dev.cpu().numpy()
        # the tracker's rows, as the driver's tracker left them, through the same call
        tx = rd("track_rows.f32", np.float32).reshape(S, 2 * L)
        tp = WP.points_of(tx, LM)
        dev2 = torch.from_numpy(full).cuda()
        lst2 = [(dev2.data_ptr() + fr["off"], fr["w"], fr["h"], fr["stride"], K.NAMES[fr["fmt"]]) for fr in frames]
        chroma2 = [dev2.data_ptr() + fr["uv_off"] if fr["fmt"] == T.NV12 and fr["separate"] else None for fr in frames]
        tf, ts = ctx.warp_paste_tensor_at(tp, torch.from_numpy(y).cuda(), lst2, mask=torch.from_numpy(alpha).cuda(), chroma=chroma2,
                                          filter="area", **spec)
        tracked = dev2.cpu().numpy()
    finally:
        ctx.close()
    assert np.array_equal(pf, flags) and np.array_equal(ps, cnt) and np.array_equal(python, want)
    assert np.isfinite(tx).all() and (ts > 1).any() and (tracked != full).sum() > 300, ((ts > 1).sum(), int((tracked != full).sum()))
    assert np.array_equal(rd("track_flags.i32", np.int32), tf) and np.array_equal(rd("track_samples.i32", np.int32).reshape(ts.shape), ts)
    assert np.array_equal(rd("track.u8", np.uint8), planes_of(tracked))
    for name in ("fit.u8", "at.u8", "behind.u8"):                               # (behind: the driver laid every UV plane behind its Y plane)
        assert np.array_equal(rd(name, np.uint8), planes_of(python)), name
