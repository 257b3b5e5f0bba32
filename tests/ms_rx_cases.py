"""Slots for the tests of the MS-side downlink burst receiver (tests/test_ms_rx_cpu.py, tests/test_gpu_ms_rx.py): normal and
synchronisation bursts from the oracle's modulator, `off` samples into a slot of 625 (off < 0: the slot begins inside the burst)."""
import numpy as np

import oracle_lib as O
from osmo_trx_amd import synth

SLOT = 625


def nb_bits(rng, tsc):
    """148 bits of a normal burst: 3 tail | 58 | 26 training | 58 | 3 tail."""
    bits = rng.integers(0, 2, 148, dtype=np.uint8)
    bits[:3] = 0
    bits[-3:] = 0
    bits[61:87] = [int(c) for c in synth.TSC_BITS[tsc]]
    return bits


def place(rng, wave, off, snr_db, amp):
    """SLOT samples of noise (amp / snr below the burst's amplitude) with `wave` starting at sample `off` (None: noise only)."""
    sigma = amp * 10 ** (-snr_db / 20) / np.sqrt(2)
    y = ((rng.normal(size=SLOT) + 1j * rng.normal(size=SLOT)) * sigma).astype(np.complex64)
    if off is not None:
        w = wave * np.complex64(amp * np.exp(1j * rng.uniform(0, 2 * np.pi)))
        lo, hi = max(off, 0), min(off + len(w), SLOT)
        y[lo:hi] += w[lo - off:hi - off]
    return y


def nb_slot(rng, tsc, off, snr_db=25.0, amp=3000.0):
    """(complex64[625], the 148 bits sent)."""
    bits = nb_bits(rng, tsc)
    return place(rng, O.modulate_burst(bits, 8, 4), off, snr_db, amp), bits


def sch_slot(rng, bsic, fn, off, snr_db=25.0, amp=3000.0):
    return place(rng, O.modulate_burst(synth.sch_burst_bits(bsic, fn), 8, 4), off, snr_db, amp)


def to_i16(y):
    """int16[..., 2]: the samples rounded, as a radio would deliver them."""
    return np.stack([np.round(y.real), np.round(y.imag)], axis=-1).clip(-32768, 32767).astype(np.int16)


def hard(bits):
    """The sbits of sent bits: -127 is a one."""
    return np.where(np.asarray(bits) > 0, -127, 127).astype(np.int8)
