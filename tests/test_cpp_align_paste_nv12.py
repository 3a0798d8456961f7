"""The rcr::paste_crops_tensor overloads that take the frames' UV planes (superviseddescent_amd/include/rcr/alignment.hpp,
tests/cpp/align_paste_nv12_gpu.cpp): landmark rows on NV12 DeviceFrames -- the UV plane behind Y or in an allocation of its own -- and a
BGR one give, through the fit and through explicit matrices, filtered and plain, the bytes and the S of the Python layer on the same
rows, tensor, opacity maps and frames -- the same kernel behind the same C-ABI --, and those are the restatement's."""
import os

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import paste_area_cases as D
import paste_area_ref as Q
import paste_cases as C
import paste_nv12_cases as V
import paste_nv12_ref as N


@pytest.mark.gpu
def test_cpp_nv12_paste_matches_python(built, tmp_path):
    import torch
    from superviseddescent_amd import Context, HoGParam, ibug
    from test_gpu_align_tensor import IDS as ids, L, LM, MEAN as mean, template
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    buf, frames = V.place([V.FRAMES[0], V.FRAMES[1], V.FRAMES[7], V.FRAMES[6]], 17)
    w, h, S = 16, 16, 4
    tmpl = template(w, h)
    sims = [D.minifying(frames[r], w, h, 18 + r, 1, D.W_SCALES[r:] + D.W_SCALES[:r])[0] for r in range(S)]     # W scales 0.8, 1.7, 2.6, 4.5
    x = K.landmark_rows(sims, tmpl, LM, L)
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
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("".join(meta))
    B.run(B.gpu_driver("align_paste_nv12_gpu", tmp_path), [d], 300)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    c = Context(0)
    try:
        re_, le_ = ibug.eye_indices(ids)
        c.set_model_geometry(L, re_, le_, params)

        def fresh():
            dev = torch.from_numpy(full).cuda()
            return dev, B.device_frames(dev, frames), B.device_chroma(dev, frames, only_separate=True)
        dev, lst, chroma = fresh()
        c.set_frames_device(lst)
        c.set_sample_image_index(None)
        c.set_x(x)
        spec = dict(scale=C.SCALES, bias=C.BIASES)
        yd = torch.from_numpy(y).cuda()
        mats, flags, samples = c.align_paste_tensor(LM, tmpl, yd, lst, mask=alpha, filter="area", chroma=chroma, **spec)
        got = dev.cpu().numpy()
        assert rd("mats.f32", np.uint32).tobytes() == mats.tobytes()
        assert np.array_equal(rd("flags.i32", np.int32), flags) and np.array_equal(rd("flags_at.i32", np.int32), flags)
        assert np.array_equal(rd("samples.i32", np.int32), samples) and np.array_equal(rd("samples_at.i32", np.int32), samples)
        assert samples.tolist() == [Q.samples(m) for m in mats] and len(set(samples.tolist())) >= 3
        assert np.array_equal(rd("fit.u8", np.uint8), planes_of(got)) and np.array_equal(rd("at.u8", np.uint8), planes_of(got))
        want = full.copy()
        for r, fr in enumerate(frames):
            if fr["fmt"] == T.NV12:
                N.paste_row(*V.planes(want, fr), mats[r], y[r], alpha[r], int(samples[r]), **spec)
            else:
                Q.paste_row(C.view(want, fr), fr["fmt"], mats[r], y[r], alpha[r], int(samples[r]), **spec)
        assert np.array_equal(got, want) and (want != full).sum() > 100
        dev, lst, chroma = fresh()
        c.align_paste_tensor_at(mats, yd, lst, mask=alpha, chroma=chroma, **spec)
        plain = dev.cpu().numpy()
        assert np.array_equal(rd("plain.u8", np.uint8), planes_of(plain)) and not np.array_equal(plain, got)
    finally:
        c.close()
