"""The MS-side uplink oscillator (include/trxhip.h, "MS-side uplink frequency correction") restated in numpy on top of the uplink
model (tests/ms_tx_model.py) and the oscillator's model (tests/ms_nco_model.py), for tests/test_ms_tx_nco_cpu.py and
tests/test_gpu_ms_tx_nco.py.  Nothing of the arithmetic is imported from the product; the rotation takes the two phasor tables as
an argument and the tests hand it the library's (trxhip_ms_nco_tables_host()).

    _set     acts at the end of the last rendered window, 0 before the first: ms_nco_model.Nco.set(enable, hz, ts_now)
    sample   x = the modulator's sample times the plan's scale (complex64); y = rotate(x, p(ts)); int16 = trunc(y), C's cast
    zeros    every sample outside a burst is 0
"""
import math

import numpy as np

import ms_nco_model as NM
import ms_tx_model as M


def cast(y):
    """(int16_t)(int)(y * 1.0f) per component of complex64[n]: truncation toward zero; |y| < 32768 is the caller's to show"""
    y = np.asarray(y, dtype=np.complex64)
    return np.stack([np.trunc(y.real), np.trunc(y.imag)], axis=-1).astype(np.int32).astype(np.int16)


def scaled(x, scale):
    """scaleVector() with (scale, 0): Complex<float> operator*, every product and sum a float32"""
    x = np.asarray(x, dtype=np.complex64)
    s, z = np.float32(scale), np.float32(0.0)
    out = np.empty(len(x), dtype=np.complex64)
    out.real = (x.real * s) - (x.imag * z)
    out.imag = (x.real * z) + (x.imag * s)
    return out


class MsTxNco(M.MsTx):
    """MsTx with the member's oscillator"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.nco = NM.Nco()

    def set_nco(self, enable, hz=0.0):
        self.nco.set(enable, hz, self.rendered_end if self.rendered_end is not None else 0)

    def nco_state(self):
        return self.nco.state()

    def render_stream(self, n_samples, first_ts, rows, tabs):
        """rows: {radio_ts: complex64[625], the burst's scaled samples}.  Returns (n_drawn, int16[n_samples, 2]): the render takes
        the oscillator's setting as it is now"""
        nco = self.nco.state()
        nd, pieces = self.render(n_samples, first_ts)
        out = np.zeros((n_samples, 2), dtype=np.int16)
        for off, first, length, ts in pieces:
            x = np.asarray(rows[ts], dtype=np.complex64)[first:first + length]
            if nco["enable"]:
                x = NM.rotate(tabs, x, NM.phase(nco["acc"], nco["ts_ref"], nco["inc"], first_ts + off), nco["inc"])
            out[off:off + length] = cast(x)
        return nd, out


def radio(x, hz, k0=0):
    """a radio whose oscillator is hz off: the int16 stream x[n, 2] rotated by hz in double, truncated like the cast"""
    y = NM.carrier(x, hz, k0)
    return np.stack([np.trunc(y.real), np.trunc(y.imag)], axis=-1).clip(-32768, 32767).astype(np.int16)


# ---- the uplink on the CPU oracle: the BTS's detector and demodulator over bursts on a carrier that is off -------------------

UL_TSC = 5
UL_AMP = 2047.0
UL_NOISE = 20
UL_BURSTS = 64
UL_SEED = 4127


def ul_bursts(n=UL_BURSTS, seed=UL_SEED):
    """(bits uint8[n, 148] with no second correlation peak, complex64[n, 625] of the oracle's modulator times 2047, start phases)"""
    import oracle_lib as O
    from test_gpu_tx_frontend import _unambiguous_bursts
    rng = np.random.default_rng(seed)
    bits = _unambiguous_bursts(np.full(n, UL_TSC), rng)
    x = np.stack([scaled(O.modulate_burst(b, 8, 4), UL_AMP) for b in bits])
    return bits, x, rng.uniform(0, 2 * math.pi, n)


def ul_wrong_bits(x, bits, start, cfo_hz, seed=UL_SEED + 1):
    """x complex64[n, 625] as transmitted, each on a carrier cfo_hz off from a random start phase, +-20 counts of noise, int16;
    the oracle's pull_batch as the BTS.  Returns (bursts detected, fraction of wrong hard bits 3 .. 144)"""
    import oracle_lib as O
    rng = np.random.default_rng(seed)
    n = len(x)
    y = np.stack([NM.carrier(x[i], cfo_hz) * np.exp(1j * start[i]) for i in range(n)])
    iq = np.stack([np.trunc(y.real), np.trunc(y.imag)], axis=-1) + rng.integers(-UL_NOISE, UL_NOISE + 1, (n, 625, 2))
    iq = iq.clip(-32768, 32767).astype(np.int16)
    p = np.zeros(n, dtype=O.PARAMS_DTYPE)
    p["type"], p["tsc"], p["max_toa"] = 1, UL_TSC, 20          # TSC: a normal burst
    res, soft = O.pull_batch(iq, 4, p, threshold=4.0, full_scale=UL_AMP)
    hard = (soft[:, :148] > 0.5).astype(np.uint8)
    return int((res["rc"] > 0).sum()), float((hard[:, 3:145] != bits[:, 3:145]).mean())
