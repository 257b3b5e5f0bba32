"""The air interface (include/trxhip.h, "the air interface") restated in numpy on tests/ms_nco_model.py's
oscillator (phasor, Nco).  Nothing of the arithmetic is imported from the product; the phasor tables are an argument, as in the
NCO tests (the library's trxhip_ms_nco_tables_host(), compared with numpy's cos / sin there).

    x      the source's int16 sample at ts - delay, 0 in front of the direction's first sample or its last reset
    y      x times the phasor of p(ts), every product and sum rounded to float32
    c      rint(y * (gain * 256)) per component, half-even
    noise  s(seed, lane, ts) = the bytes of fmix32(fmix32(lo) + fmix32(seed ^ fmix32(lane)) + hi * 0x9e3779b9) summed, - 510;
           nq = (scale * s + 128) >> 8, scale = rint(rms * 65536 / sqrt(21845))
    out    clamp((sum of c + nq + 128) >> 8)
"""
import numpy as np

import ms_nco_model as NM

F = np.float32
UL, DL = 0, 1
UL_RX = 4096
SIGMA = 147.80054127099805
MAX_DELAY = 65536
M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """murmur3's finaliser on uint64 arrays holding 32-bit values"""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def noise_s(seed, lane, ts):
    """s of the lane at the timestamps ts (any ints, taken modulo 2^64): int64 array"""
    t = np.array([int(v) % (1 << 64) for v in np.atleast_1d(ts)], dtype=np.uint64) if not isinstance(ts, np.ndarray) else ts.astype(np.uint64)
    lo, hi = t & M32, t >> np.uint64(32)
    key = (fmix32(np.uint64(seed & 0xFFFFFFFF) ^ fmix32(np.uint64(lane))) + hi * np.uint64(0x9E3779B9)) & M32
    w = fmix32((fmix32(lo) + key) & M32)
    b = (w & np.uint64(255)) + ((w >> np.uint64(8)) & np.uint64(255)) + ((w >> np.uint64(16)) & np.uint64(255)) + (w >> np.uint64(24))
    return b.astype(np.int64) - 510


def noise_scale(rms):
    if not 0.0 <= rms <= 8192.0:
        raise ValueError(rms)
    return int(np.rint(np.float64(rms) * 65536.0 / SIGMA))


def nq(scale, s):
    return (np.int64(scale) * s + 128) >> 8


def finish(acc):
    return np.clip((acc + 128) >> 8, -32768, 32767).astype(np.int16)


class Path:
    def __init__(self):
        self.gain, self.delay, self.osc = F(1.0), 0, NM.Nco()


class Air:
    """AirChannel's model: set_path, set_noise, reset, uplink, downlink, path_state.  The source's whole past since the last
    reset is kept (the product keeps max_delay samples; no path reaches further back)"""

    def __init__(self, tabs, n_members, max_delay=0, seed=0):
        if not 1 <= n_members <= 4096 or not 0 <= max_delay <= MAX_DELAY:
            raise ValueError
        self.tabs, self.n, self.max_delay, self.seed = tabs, n_members, max_delay, seed
        self.path = [[Path() for _ in range(n_members)] for _ in range(2)]
        self.scale = [[0], [0] * n_members]
        self.started, self.end_ts = [False, False], [0, 0]
        self.past = [np.zeros((n_members, 0, 2), np.int16), np.zeros((1, 0, 2), np.int16)]

    def set_path(self, d, m, gain=1.0, delay=0, hz=0.0):
        if not 0.0 <= gain <= 16.0 or not 0 <= delay <= self.max_delay:
            raise ValueError
        NM.inc_of(hz)
        p = self.path[d][m]
        p.osc.set(hz != 0.0, hz, self.end_ts[d])
        p.gain, p.delay = F(gain), int(delay)

    def set_noise(self, d, m, rms):
        self.scale[d][0 if d == UL else m] = noise_scale(rms)

    def reset(self, d, ts):
        self.started[d], self.end_ts[d] = True, ts
        self.past[d] = self.past[d][:, :0]

    def path_state(self, d, m):
        p = self.path[d][m]
        return dict(gain=float(p.gain), delay=p.delay, hz=p.osc.hz, inc=p.osc.inc, acc=p.osc.acc, ts_ref=p.osc.ts_ref,
                    noise_scale=self.scale[d][0 if d == UL else m], started=int(self.started[d]), end_ts=self.end_ts[d])

    def _contrib(self, d, m, src, first_ts, n):
        """int64[n, 2]: path (d, m) over the window, src = int16[past + n, 2] ending with the window"""
        p = self.path[d][m]
        back = src.shape[0] - n
        x = np.zeros((n, 2), np.int16)
        lo = max(0, p.delay - back)                                # outputs in front of it read 0
        x[lo:] = src[back + lo - p.delay: back + n - p.delay]
        ph = (np.uint64(p.osc.phase(first_ts)) + np.arange(n, dtype=np.uint64) * np.uint64(p.osc.inc & NM.M32)) & M32
        rc, rs = NM.phasor(self.tabs, ph)
        xr, xi = x[:, 0].astype(F), x[:, 1].astype(F)
        yr, yi = (xr * rc) - (xi * rs), (xr * rs) + (xi * rc)
        g256 = F(p.gain * F(256.0))
        return np.stack([np.rint(yr * g256), np.rint(yi * g256)], axis=1).astype(np.int64)

    def _noise(self, rx, scale, first_ts, n):
        ts = [first_ts + i for i in range(n)]
        return np.stack([nq(scale, noise_s(self.seed, 2 * rx + c, ts)) for c in (0, 1)], axis=1)

    def _window(self, d, src_rows, first_ts):
        if self.started[d] and first_ts != self.end_ts[d]:
            raise ValueError("not contiguous")
        n = src_rows.shape[1]
        assert n > 0
        full = np.concatenate([self.past[d], src_rows], axis=1)
        self.past[d] = full[:, -self.max_delay:] if self.max_delay else full[:, :0]
        self.started[d], self.end_ts[d] = True, first_ts + n
        return full, n

    def uplink(self, rows, first_ts):
        """rows: int16[n_members, n, 2] -> int16[n, 2]"""
        full, n = self._window(UL, np.asarray(rows), first_ts)
        acc = np.zeros((n, 2), np.int64)
        for m in range(self.n):
            acc += self._contrib(UL, m, full[m], first_ts, n)
        return finish(acc + self._noise(UL_RX, self.scale[UL][0], first_ts, n))

    def downlink(self, x, first_ts):
        """x: int16[n, 2] -> int16[n_members, n, 2]"""
        full, n = self._window(DL, np.asarray(x)[None], first_ts)
        return np.stack([finish(self._contrib(DL, m, full[0], first_ts, n) + self._noise(m, self.scale[DL][m], first_ts, n))
                         for m in range(self.n)])
