"""Cases for the tests of the MS-side FCCH frequency-offset measurement (tests/test_ms_afc_cpu.py, tests/test_gpu_ms_afc.py): the
row set both compare models and device on, and downlink streams whose FCCH slots hold a tone at a known carrier offset."""
import functools
import math

import numpy as np

import ms_afc_model as AM

SLOT = 625
FULL = 2047.0
TONE_AMP = 8000.0
BIAS_HZ = AM.TONE_HZ - 67700           # what the estimator reads on a carrier that is exactly on frequency: +8.33 Hz


def noisy_tone(rng, cfo, snr_db, amp=TONE_AMP):
    sigma = amp * 10 ** (-snr_db / 20) / math.sqrt(2)
    return AM.tone(cfo, amp, rng.uniform(0, 2 * math.pi)) + (rng.normal(size=SLOT) + 1j * rng.normal(size=SLOT)) * sigma


@functools.lru_cache(maxsize=None)
def row_set():
    """(int16[430, 625, 2], n_tones): 10 tones each at 30, 10 and 3 dB SNR, then 400 noise-only rows at amplitudes 3, 100, 5000"""
    rng = np.random.default_rng(20260)
    rows = [noisy_tone(rng, rng.uniform(-80000, 85000), snr) for snr in (30, 10, 3) for _ in range(10)]
    n_tones = len(rows)
    for i in range(400):
        amp = (3.0, 100.0, 5000.0)[i % 3]
        rows.append((rng.normal(size=SLOT) + 1j * rng.normal(size=SLOT)) * amp / math.sqrt(2))
    out = AM.to_i16(np.stack(rows))
    out.setflags(write=False)
    return out, n_tones


@functools.lru_cache(maxsize=None)
def device_row_set():
    """row_set() plus clipped rows (+-32767, -32768: a saturated tone, constant rails, a square wave between the rails) and an
    all-zero row.  Returns (int16[n, 625, 2], n_tones)"""
    rows, n_tones = row_set()
    rng = np.random.default_rng(20261)
    clip = [AM.to_i16(AM.tone(12000.0, 60000.0, 0.4)), np.full((SLOT, 2), 32767, np.int16), np.full((SLOT, 2), -32768, np.int16),
            np.where(rng.integers(0, 2, (SLOT, 2)) > 0, 32767, -32768).astype(np.int16),
            np.repeat(np.where(np.arange(SLOT) // 2 % 2 > 0, 32767, -32768).astype(np.int16)[:, None], 2, axis=1)]
    out = np.concatenate([rows, np.stack(clip), np.zeros((1, SLOT, 2), np.int16)])
    out.setflags(write=False)
    return out, n_tones


@functools.lru_cache(maxsize=None)
def models(which="device"):
    """the float64 model's dict of every row of device_row_set() (or row_set()), computed once"""
    rows = (device_row_set() if which == "device" else row_set())[0]
    return tuple(AM.fcch_offset(x) for x in AM.scaled(rows, FULL))


# ---- streams ----------------------------------------------------------------------------------------------------------

N_FRAMES = 2 * 51
FN0 = 51 * 40                          # the stream's first slot is (FN0, 0): an FCCH slot


def fcch_slots(n_frames=N_FRAMES, fn0=FN0):
    """the indices, among the stream's slots, of its FCCH slots"""
    return [8 * f for f in range(n_frames) if (fn0 + f) % 51 in (0, 10, 20, 30, 40)]


@functools.lru_cache(maxsize=None)
def _base():
    import ms_sched_cases as SC
    x, _ = SC.cell_stream(5150, FN0, N_FRAMES, 0o53, tsc=0o53 & 7)
    x.setflags(write=False)
    return x


def stream(burst, cfo, seed, amp=3000.0):
    """int16[N_FRAMES * 8 * 625, 2]: tests/ms_sched_cases.py's cell (SCH and normal bursts in noise) with, in every FCCH slot,
    `burst` -- complex64 samples of an all-zero-bit GMSK burst at unit amplitude, the FCCH tone -- rotated by cfo Hz, at a random
    phase, rounded to int16.
    The FCCH slots carry no noise.  The tests hold every estimate within 100 Hz of the truth, a bar for a ramped, quantised,
    modulated tone; noise is the model tests' subject.  At an SNR of rho the angle of the lag-L sum over N = 92 samples has a
    variance of about L / (rho N^2): at 25 dB (the cell's other slots) that is 61 Hz on omegal1 and 19 Hz on omegal2, 32 Hz on
    their mean -- 100 Hz would be a 3-sigma event, met once in a few hundred slots."""
    rng = np.random.default_rng(seed)
    x = _base().copy()
    rot = np.exp(2j * math.pi * cfo / AM.GSM_SYM_RATE * np.arange(len(burst)))
    for k in fcch_slots():
        y = np.zeros(SLOT, np.complex128)
        y[:len(burst)] = burst * rot * (amp * np.exp(1j * rng.uniform(0, 2 * math.pi)))
        x[k * SLOT:(k + 1) * SLOT] = AM.to_i16(y)
    return x
