"""Streams and rows for the tests of the MS-side FCCH search (tests/test_ms_fsearch_cpu.py, tests/test_gpu_ms_fsearch.py), from the
existing generators: the oracle's modulator through tests/ms_rx_cases.py, tests/ms_nco_model.carrier, tests/ms_afc_model.tone."""
import functools

import numpy as np

import ms_afc_model as AM
import ms_fsearch_model as FM
import ms_nco_model as NM
import ms_rx_cases as K
import ms_sched_model as SM
import oracle_lib as O

SLOT = K.SLOT
FULL = 2047.0
AMP = 3000.0
FN0 = 51 * 12                              # (FN0, 0) is an FCCH slot, (FN0 + 1, 0) the SCH slot behind it
BSIC = 0o45
TSC = BSIC & 7
ACQ_LEN = 60000                            # the buffer length of the acquire tests: 96 slots


@functools.lru_cache(maxsize=None)
def fcch_burst():
    """complex64: the frequency-correction burst, 148 zero bits through the oracle's modulator at unit amplitude"""
    return O.modulate_burst(np.zeros(148, dtype=np.uint8), 8, 4)


@functools.lru_cache(maxsize=None)
def cell(seed, snr_db, cfo, n_frames=12, lead=0, active=0xFF, fcch=True):
    """(int16[lead + n_frames * 5000, 2], fcch_starts, sent): `lead` samples of noise, then the frames FN0 .. of a cell on a
    carrier cfo Hz off: the frequency-correction burst in every FCCH slot (fcch=False: noise), the SCH burst (BSIC, fn) in every SCH
    slot, a normal burst of random bits on every other slot whose TN is in `active` (noise on the others), all at amplitude AMP
    and snr_db.  fcch_starts: the first sample of every FCCH slot; sent[(fn, tn)]: a traffic slot's 148 bits"""
    rng = np.random.default_rng(seed)
    parts, starts, sent = ([K.place(rng, None, None, snr_db, AMP)[:lead]] if lead else []), [], {}
    assert lead <= SLOT
    for fn in range(FN0, FN0 + n_frames):
        for tn in range(8):
            if SM.is_fcch(fn, tn):
                starts.append(lead + ((fn - FN0) * 8 + tn) * SLOT)
                parts.append(K.place(rng, fcch_burst() if fcch else None, 0 if fcch else None, snr_db, AMP))
            elif SM.is_sch(fn, tn):
                parts.append(K.sch_slot(rng, BSIC, fn, 0, snr_db, AMP))
            elif (active >> tn) & 1:
                y, bits = K.nb_slot(rng, TSC, 0, snr_db, AMP)
                parts.append(y)
                sent[(fn, tn)] = bits
            else:
                parts.append(K.place(rng, None, None, snr_db, AMP))
    x = NM.to_i16(NM.carrier(np.concatenate(parts), cfo))
    x.setflags(write=False)
    return x, tuple(starts), sent


def to_c64(x):
    return (x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)).astype(np.complex64)


def tone_row(n, at, cfo=0.0, amp=AMP, seed=1, noise=30.0, length=592):
    """int16[n, 2]: noise `noise` dB below amp with a tone of `length` samples from sample `at` on (clipped to the row)"""
    rng = np.random.default_rng(seed)
    sigma = amp * 10 ** (-noise / 20) / np.sqrt(2)
    y = (rng.normal(size=n) + 1j * rng.normal(size=n)) * sigma
    lo, hi = max(at, 0), min(at + length, n)
    y[lo:hi] += AM.tone(cfo, amp, 0.3, length)[lo - at:hi - at]
    return NM.to_i16(y)


def tie_row(n, amp=1000.0):
    """x[n] = round(A exp(2 pi i n / 16)): every block of 16 repeats exactly, so every window has the same sums and score"""
    k = np.arange(n)
    return NM.to_i16(amp * np.exp(2j * np.pi * (k % 16) / 16.0))


def rails_row(n, kind):
    """full-scale rows for the int64 paths: 'min' every part -32768, 'max' every part 32767, 'alt' samples alternating between
    (-32768, 32767) and (32767, -32768), 'mix' -32768 re against 32767 im"""
    x = np.empty((n, 2), dtype=np.int16)
    if kind == "min":
        x[:] = -32768
    elif kind == "max":
        x[:] = 32767
    elif kind == "alt":
        x[0::2] = (-32768, 32767)
        x[1::2] = (32767, -32768)
    else:
        x[:, 0], x[:, 1] = -32768, 32767
    return x
