"""Deterministic synthetic faces for benchmarks and parity tests.

No dataset can be downloaded here, so the workload is generated: 256x256 single-channel u8 images
made of a smooth random background, per-pixel noise and a small blob at each of the 68 ground-truth
ibug landmark positions (so that HOG patches around the landmarks carry signal and a trained cascade
actually converges).  Ground truth and initialisations follow the reference trainer's recipe:
``x* = align_mean(mean, box) + N(0, 1.5 px)``, ``x0 = align_mean(mean, perturb(box, t~N(0,.04),
t~N(0,.04), s~N(1,.04)))`` (apps/rcr/rcr-train.cpp:130-146, 387-397, 421-431; include/rcr/model.hpp:64-76).

The same bytes are fed to the GPU engine and to the CPU oracle.
"""
from __future__ import annotations

import numpy as np

from . import ibug

SEED = 0x5D2015
IMAGE_SIZE = 256


def align_mean(mean: np.ndarray, box, scaling_x=1.0, scaling_y=1.0, translation_x=0.0,
               translation_y=0.0) -> np.ndarray:
    """rcr::align_mean (include/rcr/model.hpp:64-76), evaluated in float32.  box = (x, y, w, h)."""
    mean = np.asarray(mean, np.float32).reshape(-1)
    L = mean.size // 2
    f = np.float32
    out = np.empty_like(mean)
    out[:L] = (mean[:L] * f(scaling_x) + f(0.5) + f(translation_x)) * f(box[2]) + f(box[0])
    out[L:] = (mean[L:] * f(scaling_y) + f(0.5) + f(translation_y)) * f(box[3]) + f(box[1])
    return out


def perturb(box, tx: float, ty: float, s: float = 1.0):
    """perturb() of apps/rcr/rcr-train.cpp:130-146: float arithmetic, truncated into an int Rect."""
    f = np.float32
    x, y, w, h = (int(v) for v in box)
    pw, ph = f(w) * f(s), f(h) * f(s)
    nx = f(x) + (f(w) - pw) / f(2.0) + f(tx) * f(w)
    ny = f(y) + (f(h) - ph) / f(2.0) + f(ty) * f(h)
    return (int(nx), int(ny), int(pw), int(ph))


def _face_chunk(rng, n: int, size: int):
    """One chunk of make_faces: (images [n,size,size] u8, boxes [n,4], gt68 [n,136]) drawn from ``rng``."""
    wh = rng.integers(160, 209, size=n)
    bx = (rng.random(n) * (size - wh)).astype(np.int32)
    by = (rng.random(n) * (size - wh)).astype(np.int32)
    boxes = np.stack([bx, by, wh, wh], 1).astype(np.int32)
    # smooth background: 6 Gaussians (sigma 12..40 px), amplitude +-48
    gcx = rng.random((n, 6)).astype(np.float32) * size
    gcy = rng.random((n, 6)).astype(np.float32) * size
    gsig = (12 + 28 * rng.random((n, 6))).astype(np.float32)
    gamp = (48 * (2 * rng.random((n, 6)) - 1)).astype(np.float32)
    field = _background(gcx, gcy, gsig, gamp, size)
    # landmark blobs at the ground-truth shape (rigid mean + 1.5 px jitter)
    gt68 = np.empty((n, 136), np.float32)
    for i in range(n):
        gt68[i] = align_mean(ibug.MEAN_IBUG_LFPW_68, boxes[i])
    gt68 += (1.5 * rng.standard_normal((n, 136))).astype(np.float32)
    return _draw_faces(rng, field, gt68, size), boxes, gt68


def _background(gcx, gcy, gsig, gamp, size: int):
    """Smooth background of n faces [n, y, x] from their 6 Gaussians each (centres, sigmas, amplitudes)."""
    coords = np.arange(size, dtype=np.float32)
    ex = np.exp(-0.5 * ((coords[None, None, :] - gcx[:, :, None]) / gsig[:, :, None]) ** 2)
    ey = np.exp(-0.5 * ((coords[None, None, :] - gcy[:, :, None]) / gsig[:, :, None]) ** 2)
    return np.matmul((ey * gamp[:, :, None]).transpose(0, 2, 1), ex)          # [n, y, x]


def _draw_faces(rng, field, gt68, size: int):
    """Landmark blobs at gt68 [n, 136] on the background ``field`` (modified), per-pixel noise drawn from ``rng``, as u8 images."""
    coords = np.arange(size, dtype=np.float32)
    n = field.shape[0]
    lx, ly = gt68[:, :68], gt68[:, 68:]
    lamp = np.where(np.arange(68) % 2 == 0, 70.0, -70.0).astype(np.float32)
    bxk = np.exp(-0.5 * ((coords[None, None, :] - lx[:, :, None]) / 3.0) ** 2).astype(np.float32)
    byk = np.exp(-0.5 * ((coords[None, None, :] - ly[:, :, None]) / 3.0) ** 2).astype(np.float32)
    field += np.matmul((byk * lamp[None, :, None]).transpose(0, 2, 1), bxk)
    noise = (24 * (2 * rng.random((n, size, size), dtype=np.float32) - 1))
    return np.clip(128 + field + noise, 0, 255).astype(np.uint8)


def make_faces(n_images: int, seed: int = SEED, size: int = IMAGE_SIZE, chunk: int = 256, workers: int = 0):
    """Returns (images uint8 [n,size,size], boxes int32 [n,4] (x,y,w,h), gt68 float32 [n,136]).

    ``workers <= 1``: one random stream, chunk after chunk (the stream every fixture and test of this repo uses).
    ``workers > 1``: the chunks are drawn from independent streams ``default_rng([seed, chunk_index])`` in a pool of
    forked worker processes -- a different (equally deterministic) data set, meant for the large training sets of bench.py."""
    images = np.empty((n_images, size, size), np.uint8)
    boxes = np.empty((n_images, 4), np.int32)
    gt68 = np.empty((n_images, 136), np.float32)
    starts = list(range(0, n_images, chunk))
    if workers <= 1:
        rng = np.random.default_rng(seed)
        for c0 in starts:
            n = min(chunk, n_images - c0)
            images[c0:c0 + n], boxes[c0:c0 + n], gt68[c0:c0 + n] = _face_chunk(rng, n, size)
        return images, boxes, gt68
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor

    jobs = [(seed, ci, min(chunk, n_images - c0), size) for ci, c0 in enumerate(starts)]
    # fork: the workers only run numpy.  Call this BEFORE the process initialises HIP / torch.cuda: forking an
    # initialised ROCm process leaves a later torch.cuda initialisation without devices
    with ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("fork")) as pool:
        for (_, ci, n, _), (im, bx, gt) in zip(jobs, pool.map(_face_chunk_job, jobs)):
            c0 = starts[ci]
            images[c0:c0 + n], boxes[c0:c0 + n], gt68[c0:c0 + n] = im, bx, gt
    return images, boxes, gt68


def _face_chunk_job(job):
    seed, ci, n, size = job
    return _face_chunk(np.random.default_rng([seed, ci]), n, size)


def make_samples(boxes: np.ndarray, gt68: np.ndarray, landmark_ids, n_perturb: int = 0,
                 seed: int = SEED + 1):
    """Rows of the training/test matrices.  For every image the unperturbed box, then ``n_perturb``
    perturbed boxes (rcr-train.cpp:421-431).  Returns (x_star [N,2L], x0 [N,2L], img_index [N])."""
    rng = np.random.default_rng(seed)
    pos = [ibug.IBUG68_IDS.index(i) for i in landmark_ids]
    sel = np.array(pos + [68 + p for p in pos])
    mean_sel = ibug.select_mean(landmark_ids)
    n_img = boxes.shape[0]
    per = 1 + n_perturb
    N = n_img * per
    x_star = np.repeat(gt68[:, sel], per, axis=0).astype(np.float32)
    x0 = np.empty((N, sel.size), np.float32)
    img_index = np.repeat(np.arange(n_img, dtype=np.int32), per)
    t = rng.normal(0.0, 0.04, size=(N, 2))
    s = rng.normal(1.0, 0.04, size=N)
    for r in range(N):
        box = boxes[img_index[r]]
        if n_perturb == 0 or r % per != 0:
            box = perturb(box, t[r, 0], t[r, 1], s[r])
        x0[r] = align_mean(mean_sel, box)
    return x_star, x0, img_index


def make_tracks(n_streams: int, n_frames: int, seed: int = SEED + 7, size: int = IMAGE_SIZE, max_step: float = 3.0,
                max_scale: float = 0.03):
    """Synthetic video for the tracker: ``n_streams`` faces, each drawn as ``make_faces`` draws one (its own smooth background,
    landmark blobs, fresh per-pixel noise every frame), whose box moves by up to ``max_step`` pixels (3) in x and in y and scales by
    up to ``max_scale`` (3 %) per frame and
    stays at least 10 pixels inside the frame together with every ground-truth landmark.  The boxes stand in for a face
    detector.  Returns (frames uint8 [n_frames, n_streams, size, size], gt68 float32 [n_frames, n_streams, 136], boxes int32
    [n_frames, n_streams, 4] (x, y, w, h)); stream s of frame t is image s of frames[t]."""
    rng = np.random.default_rng(seed)
    m = np.asarray(ibug.MEAN_IBUG_LFPW_68, np.float32)
    margin = 10
    # a box (x, y, w, w) keeps its landmarks inside [x + (0.5 + min m_x) w, ...] -- the mean reaches below the box (m_y up to 0.6)
    lo_x, hi_x, lo_y, hi_y = (float(v) + 0.5 for v in (m[:68].min(), m[:68].max(), m[68:].min(), m[68:].max()))
    w_max = int((size - 2 * margin - 10) / max(hi_x - lo_x, hi_y - lo_y, 1.0))

    def clamp(x, y, w):
        x = int(min(max(x, margin - lo_x * w), size - margin - hi_x * w))
        y = int(min(max(y, margin - lo_y * w), size - margin - hi_y * w))
        return x, y

    w = rng.integers(136, 177, size=n_streams).astype(np.float64)
    cx, cy = rng.random(n_streams), rng.random(n_streams)
    gcx = rng.random((n_streams, 6)).astype(np.float32) * size
    gcy = rng.random((n_streams, 6)).astype(np.float32) * size
    gsig = (12 + 28 * rng.random((n_streams, 6))).astype(np.float32)
    gamp = (48 * (2 * rng.random((n_streams, 6)) - 1)).astype(np.float32)
    shape = np.clip(1.5 * rng.standard_normal((n_streams, 136)), -4.5, 4.5).astype(np.float32)   # each face's own shape
    background = _background(gcx, gcy, gsig, gamp, size)
    pos = np.empty((n_streams, 2))
    for s in range(n_streams):
        wi = int(w[s])
        pos[s] = clamp(margin + cx[s] * (size - 2 * margin - wi), margin + cy[s] * (size - 2 * margin - wi), wi)
    frames = np.empty((n_frames, n_streams, size, size), np.uint8)
    gt68 = np.empty((n_frames, n_streams, 136), np.float32)
    boxes = np.empty((n_frames, n_streams, 4), np.int32)
    for t in range(n_frames):
        if t > 0:
            step = rng.uniform(-float(max_step), float(max_step), (n_streams, 2))
            scale = rng.uniform(1.0 - float(max_scale), 1.0 + float(max_scale), n_streams)
        for s in range(n_streams):
            if t > 0:
                w[s] = min(max(w[s] * scale[s], 112.0), float(w_max))
                pos[s] = clamp(pos[s, 0] + step[s, 0], pos[s, 1] + step[s, 1], int(w[s]))
            box = (int(pos[s, 0]), int(pos[s, 1]), int(w[s]), int(w[s]))
            boxes[t, s] = box
            gt68[t, s] = align_mean(m, box) + shape[s]
        frames[t] = _draw_faces(rng, background.copy(), gt68[t], size)
    return frames, gt68, boxes
