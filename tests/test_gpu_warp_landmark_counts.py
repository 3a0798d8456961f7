"""warp_fit_kernel (csrc/sdm_warp.hip) with more than 64 mesh landmarks: its first loop, `for (k = lane; k < K; k += 64)`, looks at the
mesh's K landmarks for DEGENERATE and PARTIAL, and every mesh of tests/test_gpu_warp.py is built on 22.  Here the model has all 68
ibug landmarks and the meshes hold K = 68 of them (their Delaunay triangulation: more than 64 real triangles, none repeated), K = 64
and K = 65.  Labels, the N x T x 6 matrices, the flags and the tensor against tests/warp_ref.py as tests/test_gpu_warp.py compares them;
then every flag from the far end of its loop alone: DEGENERATE from mesh position 66, PARTIAL from mesh position 67 one pixel past
the frame, FOLDED from triangles of index >= 64 -- and the same rows without it carry no flag."""
import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import warp_cases as W
import warp_ref as R
from superviseddescent_amd import Context, HoGParam, alignment_template, delaunay, ibug

pytestmark = pytest.mark.gpu
IDS = ibug.IBUG68_IDS
L = len(IDS)
MEAN = ibug.select_mean(IDS)
RE, LE = ibug.eye_indices(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6)]
SCALES = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], np.float32)
BIASES = np.array([-2.1179, -2.0357, -1.8044], np.float32)
CHIN, NOSE_TIP = 8, 30


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def placed():
    buf, frames = W.place()
    return buf, frames, [K.host_frame(buf, f) for f in frames]


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def mesh(k, w, h, last_triangles_at=None):
    """(landmark indices, template, triangles): the first k of the 68 landmarks -- at k = 68 with the chin as mesh position 67, so that
    the last landmark the fit looks at lies on the hull -- the default template and its Delaunay triangulation.  With
    ``last_triangles_at`` the triangles that touch that mesh position come last."""
    idx = np.arange(k)
    if k == L:
        idx[[CHIN, L - 1]] = [L - 1, CHIN]
    t = alignment_template(MEAN, idx, w, h, 0.1)
    tri = np.asarray(delaunay(t), np.int32)
    if last_triangles_at is not None:
        touch = (tri == last_triangles_at).any(1)
        tri = np.ascontiguousarray(np.concatenate([tri[~touch], tri[touch]]))
    return idx, t, tri


def install(ctx, buf, frames, rows, x):
    import torch
    dev = torch.from_numpy(buf).cuda()
    base = dev.data_ptr()
    lst = [(base + f["off"], f["w"], f["h"], f["stride"], K.NAMES[f["fmt"]]) for f in frames]
    chroma = [base + f["uv_off"] if f["fmt"] == T.NV12 else None for f in frames]
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(rows)
    ctx.set_x(x)
    ctx.align_set_source_frames(lst, chroma=chroma)
    return dev, lst, chroma


def restore(ctx):
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def sizes(frames, rows):
    return [(frames[i]["w"], frames[i]["h"]) for i in rows]


@pytest.mark.parametrize("k", [64, 65, 68])
def test_labels_matrices_flags_and_tensor(ctx, placed, k):
    buf, frames, host = placed
    for (w, h) in W.CROPS:
        idx, t, tri = mesh(k, w, h)
        assert len(idx) == k and 64 < len(tri) <= 254 and len(np.unique(np.sort(tri, 1), axis=0)) == len(tri)      # real triangles, none twice
        ctx.warp_set_mesh(idx, t, tri, w, h)
        lab = ctx.warp_labels()
        assert lab.shape == (h, w) and np.array_equal(lab, R.labels(t, tri, w, h))
        assert (lab == R.NONE).any() and (lab != R.NONE).any() and (lab[lab != R.NONE] >= 64).any()
        x = W.rows_for(frames, W.ROWS, idx, t, w, h, 3 + k, L=L)
        keep = install(ctx, buf, frames, W.ROWS, x)
        spec = dict(dtype="float16", layout="nchw", channels=3, order="rgb", scale=SCALES, bias=BIASES)
        out, mats, flags = ctx.warp_crops_tensor(**spec)
        assert mats.shape == (len(W.ROWS), len(tri), 2, 3)
        assert np.array_equal(bits(mats.reshape(len(W.ROWS), -1, 6)), bits(R.matrices(x, idx, t, tri)))
        assert np.array_equal(flags, R.flags(x, idx, t, tri, sizes(frames, W.ROWS)))
        got = out.cpu().numpy()
        for r, im in enumerate(W.ROWS):
            kind, bgr, y = R.warped(host[im], mats[r].reshape(-1, 6), lab)
            want = T.finish(kind, bgr, y, **spec)
            assert got[r].dtype == want.dtype and np.array_equal(bits(got[r]), bits(want)), (k, r)
        assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


@pytest.mark.parametrize("k", [65, 68])
def test_flags_from_the_last_landmarks_and_triangles(ctx, placed, k):
    buf, frames, host = placed
    w, h = W.CROPS[0]
    touched = L - 1 if k == L else k - 1                         # the mesh position whose triangles come last: the chin / landmark 64
    idx, t, tri = mesh(k, w, h, last_triangles_at=touched if k == L else None)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    frame = 2                                                   # the 48 x 40 frame holds the whole template at (12, 10)
    fw, fh = frames[frame]["w"], frames[frame]["h"]
    base = np.random.default_rng(1).uniform(0, 30, (1, 2 * L)).astype(np.float32)
    base[0, idx], base[0, L + idx] = t[:, 0] + 12, t[:, 1] + 10
    rows = [base[0].copy()]                                     # row 0: the template moved: no flag
    last, before = k - 1, k - 2                                  # mesh positions 67 and 66 (64 and 63 at K = 65)
    assert before >= 63 and last >= 64
    r = base[0].copy(); r[idx[last]] = np.nan; rows.append(r)   # row 1: DEGENERATE from the last mesh position alone
    if k == L:
        r = base[0].copy(); r[L + idx[before]] = np.inf; rows.append(r)         # row 2: DEGENERATE from mesh position 66 alone
        r = base[0].copy(); r[L + idx[last]] = np.float32(fh); rows.append(r)     # row 3: the chin one pixel past the last frame row: PARTIAL
        r = base[0].copy(); r[L + idx[last]] = np.float32(fh - 1); rows.append(r)       # row 4: on the last frame row: inside
        # row 5: a vertex all of whose triangles have index >= 64 moved across the mesh: FOLDED from those alone
        v = idx[last]
        r = base[0].copy(); r[L + v] = t[:, 1].min() + 10 - 3.0; rows.append(r)  # (the chin above the brows: still inside the frame)
    x = np.stack(rows)
    n = len(x)
    want = R.flags(x, idx, t, tri, [(fw, fh)] * n)
    keep = install(ctx, buf, frames, [frame] * n, x)
    out, mats, flags = ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=1)
    assert np.array_equal(flags, want)
    assert flags[0] == 0 and flags[1] == R.DEGENERATE
    assert np.isnan(mats[1]).all() and np.isfinite(mats[0]).all()
    assert np.array_equal(bits(mats.reshape(n, -1, 6)), bits(R.matrices(x, idx, t, tri)))
    if k == L:
        assert flags[2] == R.DEGENERATE and flags[3] == R.PARTIAL and flags[4] == 0 and flags[5] == R.FOLDED
        # which triangles of row 5 turned over: all of index >= 64, by the reference's determinants
        _, _, det, D = R._fit(x[5:6], idx, t, tri)
        turned = np.flatnonzero(~(((det[0] > 0) & (D > 0)) | ((det[0] < 0) & (D < 0))))
        assert len(turned) and turned.min() >= 64
        touch = np.flatnonzero((tri == touched).any(1))
        assert touch.min() >= 64 and set(turned) <= set(touch)
    assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)
