"""The tracker's temporal landmark filter (include/sdm.h, "Tracking, filtered"; csrc/sdm_track_filter_device.h) restated in numpy
float32, state included: every operation on float32 values, rounded on its own, in the order the header writes it.

    f = OneEuro(S, L, min_cutoff, beta, d_cutoff)
    out = f.step(ids, x, masks, dt)      # x n x 2L raw rows, masks n, dt one value or n -> n x 2L filtered rows; the state moves on
    f.unprime(ids)                       # sdm_track_start
    rows, derivative, primed = f.get(ids)

``guards`` counts the coordinates whose derivative (index 0) or filtered value (index 1) was not finite and was replaced."""
import numpy as np

f32 = np.float32
TWO_PI = f32(6.2831855)
ONE = f32(1.0)


def alpha(fc, dt):
    """1.0f / (1.0f + (1.0f / (6.2831855f * fc)) / dt)"""
    with np.errstate(all="ignore"):
        return ONE / (ONE + (ONE / (TWO_PI * f32(fc))) / f32(dt))


def alpha_exact(fc, dt):
    """the same quantity in double: what the derived figures of the filter's behaviour are stated in"""
    tau = 1.0 / (2.0 * np.pi * fc)
    return 1.0 / (1.0 + tau / dt)


class OneEuro:
    def __init__(self, S, L, min_cutoff, beta, d_cutoff=1.0):
        self.L, self.M = L, 2 * L
        self.min_cutoff, self.beta, self.d_cutoff = f32(min_cutoff), f32(beta), f32(d_cutoff)
        self.r = np.zeros((S, 2 * L), f32)
        self.d = np.zeros((S, 2 * L), f32)
        self.f = np.zeros((S, 2 * L), f32)
        self.primed = np.zeros(S, np.int32)
        self.guards = [0, 0]

    def unprime(self, ids):
        self.primed[np.atleast_1d(ids)] = 0

    def step(self, ids, x, masks, dt):
        ids = np.atleast_1d(np.asarray(ids))
        x = np.ascontiguousarray(x, f32).reshape(ids.size, self.M)
        masks = np.broadcast_to(np.asarray(masks), (ids.size,))
        dt = np.broadcast_to(np.asarray(dt, f32).reshape(-1), (ids.size,))
        out = x.copy()
        for i, sid in enumerate(ids):
            if masks[i] != 0:
                self.primed[sid] = 0
            elif not self.primed[sid]:
                self.r[sid], self.d[sid], self.f[sid] = x[i], 0, x[i]
                self.primed[sid] = 1
            else:
                out[i] = self._row(sid, x[i], f32(dt[i]))
        return out

    def _row(self, sid, x, dt):
        L = self.L
        with np.errstate(all="ignore"):
            s = max(f32(x[:L].max() - x[:L].min()), f32(x[L:].max() - x[L:].min()))
            w = self.beta / s if s > 0 else f32(0)
            ad = alpha(self.d_cutoff, dt)
            v = (x - self.r[sid]) / dt
            dn = (ad * v) + ((ONE - ad) * self.d[sid])
            bad = ~np.isfinite(dn)
            self.guards[0] += int(bad.sum())
            dn[bad] = 0
            a = ONE / (ONE + (ONE / (TWO_PI * (self.min_cutoff + w * np.abs(dn)))) / dt)
            fn = (a * x) + ((ONE - a) * self.f[sid])
            bad = ~np.isfinite(fn)
            self.guards[1] += int(bad.sum())
            fn[bad] = x[bad]
        assert dn.dtype == f32 and fn.dtype == f32 and a.dtype == f32
        self.r[sid], self.d[sid], self.f[sid] = x, dn, fn
        return fn

    def get(self, ids):
        ids = np.atleast_1d(np.asarray(ids))
        on = self.primed[ids] != 0
        return np.where(on[:, None], self.f[ids], f32(0)), np.where(on[:, None], self.d[ids], f32(0)), on.astype(np.int32)
