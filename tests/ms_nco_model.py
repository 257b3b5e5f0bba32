"""The MS-side numerically controlled oscillator (include/trxhip.h, "MS-side frequency correction") restated in numpy, and the
streams the NCO tests share (tests/test_ms_nco_cpu.py, tests/test_gpu_ms_nco.py).  Nothing of the arithmetic is imported from the
product; the byte-exact rotation takes the two phasor tables as an argument, and the tests hand it the library's
(trxhip_ms_nco_tables_host()), which they compare with numpy's cos / sin separately.

    phase      p(ts) = acc + (uint32)(ts - ts_ref) * (uint32)inc  modulo 2^32
    increment  inc = (int32)llrint(hz * (2^32 / (13e6 / 12))), |hz| <= 500000
    phasor     C[p >> 22], F[(p >> 12) & 1023]; r = (Cc Fc - Cs Fs, Cc Fs + Cs Fc), every product and sum rounded to float32
    rotation   (xr rc - xi rs, xr rs + xi rc), the same way; the receiver multiplies by its scale afterwards
"""
import functools
import math

import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
SAMPLE_HZ = 13e6 / 12.0
MAX_HZ = 500000.0
BIAS_HZ = 25.0 / 3.0
SLOT = 625


def inc_of(hz):
    """llrint() in the default rounding mode is round-half-even, as np.rint"""
    if not abs(hz) <= MAX_HZ:                                      # (NaN fails the comparison)
        raise ValueError(hz)
    return int(np.rint(np.float64(hz) * np.float64(4294967296.0 / SAMPLE_HZ)))


def phase(acc, ts_ref, inc, ts):
    return (acc + ((ts - ts_ref) & M32) * (inc & M32)) & M32


def hz_from_fcch(hz):
    return -(float(hz) - BIAS_HZ)


def tables_numpy():
    """(C, F) float32[1024, 2] straight from numpy's double cos / sin: the yardstick of the library's tables, not used to rotate"""
    a = 2 * math.pi * np.arange(1024) / 1024.0
    b = 2 * math.pi * np.arange(1024) / 1048576.0
    return np.stack([np.cos(a), np.sin(a)], axis=1), np.stack([np.cos(b), np.sin(b)], axis=1)


def phasor(tabs, p):
    """p: uint64 array of phases.  Returns (rc, rs) float32"""
    C, Fi = tabs
    a, b = (p >> 22) & 1023, (p >> 12) & 1023
    cc, cs, fc, fs = C[a, 0], C[a, 1], Fi[b, 0], Fi[b, 1]
    assert cc.dtype == F and fc.dtype == F
    return (cc * fc) - (cs * fs), (cc * fs) + (cs * fc)            # float32 arrays: numpy rounds every operation


def parts(x):
    """(xr, xi) float32 of int16[..., 2] or complex64[...] samples"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x[..., 0].astype(F), x[..., 1].astype(F)
    assert x.dtype == np.complex64, x.dtype
    return x.real.astype(F), x.imag.astype(F)


def rotate(tabs, x, phase0, inc):
    """x: int16[n, 2] or complex64[n]; sample i rotated by the phasor of phase0 + i * inc.  Returns complex64[n]"""
    xr, xi = parts(x)
    p = (np.uint64(phase0 & M32) + np.arange(len(xr), dtype=np.uint64) * np.uint64(inc & M32)) & np.uint64(M32)
    rc, rs = phasor(tabs, p)
    out = np.empty(len(xr), dtype=np.complex64)
    out.real = (xr * rc) - (xi * rs)
    out.imag = (xr * rs) + (xi * rc)
    return out


class Nco:
    """a member's oscillator: what trxhip_ms_nco_*_set / _state keep"""

    def __init__(self):
        self.enable, self.inc, self.acc, self.ts_ref, self.hz = False, 0, 0, 0, 0.0

    def set(self, enable, hz, ts_now):
        inc = inc_of(hz)
        self.acc = phase(self.acc, self.ts_ref, self.inc, ts_now) if (self.enable and enable) else 0
        self.ts_ref, self.inc, self.hz, self.enable = ts_now, inc, float(hz), bool(enable)

    def phase(self, ts):
        return phase(self.acc, self.ts_ref, self.inc, ts)

    def state(self):
        return dict(enable=self.enable, inc=self.inc, acc=self.acc, ts_ref=self.ts_ref, hz=self.hz)


# ---- streams ------------------------------------------------------------------------------------------------------------------

def carrier(x, cfo_hz, k0=0):
    """complex128: the samples x (int16[n, 2] or complex) on a carrier cfo_hz off, sample k at the angle 2 pi cfo (k0 + k) / fs"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        x = x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)
    return x * np.exp(2j * math.pi * cfo_hz / SAMPLE_HZ * (k0 + np.arange(len(x))))


def to_i16(y):
    return np.stack([np.round(y.real), np.round(y.imag)], axis=-1).clip(-32768, 32767).astype(np.int16)


# the loop's stream: three frames from (LOOP_FN0, 0) on -- an FCCH slot, an SCH slot one frame later and traffic on TN 1 .. 3 --
# at 25 dB SNR and amplitude 3000, on a carrier LOOP_CFO off, rounded to int16
LOOP_FN0 = 51 * 12
LOOP_BSIC = 0o45
LOOP_TSC = LOOP_BSIC & 7
LOOP_ACTIVE = 0b00001111
LOOP_CFO = 2000.0
LOOP_SEED = 7301
LOOP_FRAMES = 3


@functools.lru_cache(maxsize=None)
def loop_stream(cfo=LOOP_CFO, seed=LOOP_SEED):
    """(int16[24 * 625, 2], sent): sent[(fn, tn)] = the 148 bits of the traffic slots on ACTIVE TNs; the other traffic slots hold
    noise, the FCCH slot ms_afc_model.tone in the same noise, the SCH slot (LOOP_BSIC, fn)"""
    import ms_afc_model as AM
    import ms_rx_cases as K
    import ms_sched_model as SM
    rng = np.random.default_rng(seed)
    slots, sent = [], {}
    for fn in range(LOOP_FN0, LOOP_FN0 + LOOP_FRAMES):
        for tn in range(8):
            if SM.is_fcch(fn, tn):
                slots.append(K.place(rng, AM.tone(0.0, 1.0, 0.0).astype(np.complex64), 0, 25.0, 3000.0))
            elif SM.is_sch(fn, tn):
                slots.append(K.sch_slot(rng, LOOP_BSIC, fn, 0))
            elif (LOOP_ACTIVE >> tn) & 1:
                y, bits = K.nb_slot(rng, LOOP_TSC, 0)
                slots.append(y)
                sent[(fn, tn)] = bits
            else:
                slots.append(K.place(rng, None, None, 25.0, 3000.0))
    x = to_i16(carrier(np.concatenate(slots), cfo))
    x.setflags(write=False)
    return x, sent
