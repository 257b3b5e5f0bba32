"""Multipath rays of the air interface (include/trxhip.h, "multipath rays per path") restated in numpy on
tests/air_model.py.  Nothing of the arithmetic is imported from the product.

    ray     {gain, delay, hz, phase}; p_r(ts) = phase + (uint32)(ts - ts_set) * (uint32)inc, ts_set the direction's end_ts at
            set_rays; c_r = a path's contribution of the source sample at ts - delay through {p_r(ts), gain * 256}
    path    the integer sum of c_r over its rays while it has any, its plain state's contribution otherwise
"""
import numpy as np

import air_model as A
import ms_nco_model as NM

F = np.float32
MAX_RAYS = 64


class Ray:
    def __init__(self, gain=1.0, delay=0, hz=0.0, phase=0):
        self.gain, self.delay, self.hz, self.phase = F(gain), int(delay), float(hz), int(phase)
        self.inc = NM.inc_of(hz)


class AirRays(A.Air):
    """Air with set_rays / rays: AirChannel's model"""

    def __init__(self, tabs, n_members, max_delay=0, seed=0):
        super().__init__(tabs, n_members, max_delay, seed)
        self.ray = [[[] for _ in range(n_members)] for _ in range(2)]
        self.ray_ts = [[0] * n_members for _ in range(2)]

    def set_rays(self, d, m, rays):
        rays = [] if rays is None else list(rays)
        if len(rays) > MAX_RAYS:
            raise ValueError
        new = []
        for r in rays:
            if not 0.0 <= r.get("gain", 1.0) <= 16.0 or not 0 <= r.get("delay", 0) <= self.max_delay or not 0 <= r.get("phase", 0) < 1 << 32:
                raise ValueError(r)
            new.append(Ray(**r))                                   # inc_of raises for |hz| > 500000 and NaN
        self.ray[d][m], self.ray_ts[d][m] = new, self.end_ts[d]

    def rays(self, d, m):
        """([dict], ts_set), the phases at the direction's end_ts"""
        ts0 = self.ray_ts[d][m]
        return [dict(gain=float(r.gain), delay=r.delay, hz=r.hz, phase=NM.phase(r.phase, ts0, r.inc, self.end_ts[d])) for r in self.ray[d][m]], ts0

    def _contrib(self, d, m, src, first_ts, n):
        rays = self.ray[d][m]
        if not rays:
            return super()._contrib(d, m, src, first_ts, n)
        acc = np.zeros((n, 2), np.int64)
        back = src.shape[0] - n
        for r in rays:
            x = np.zeros((n, 2), np.int16)
            lo = max(0, r.delay - back)
            x[lo:] = src[back + lo - r.delay: back + n - r.delay]
            ph = (np.uint64(NM.phase(r.phase, self.ray_ts[d][m], r.inc, first_ts)) + np.arange(n, dtype=np.uint64) * np.uint64(r.inc & NM.M32)) & A.M32
            rc, rs = NM.phasor(self.tabs, ph)
            xr, xi = x[:, 0].astype(F), x[:, 1].astype(F)
            yr, yi = (xr * rc) - (xi * rs), (xr * rs) + (xi * rc)
            g256 = F(r.gain * F(256.0))
            acc += np.stack([np.rint(yr * g256), np.rint(yi * g256)], axis=1).astype(np.int64)
        return acc
