"""CPU tests of the MS-side SCH receiver (trxhip_sch_sync_batch_*): the model the GPU tests compare with
(tests/sch_sync_model.py) is pinned to the C oracle where the oracle covers the same code, the channel coding round-trips
through it, and the chain decodes what was sent.  No GPU is opened."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import sch_sync_model as M
from test_oracle import _va_burst
from osmo_trx_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 1.0 / 2047.0


def _model_va(y, ctype, tsc, max_toa):
    """demodAnyBurst_va (Transceiver.cpp:620-645) through the model's get_chan_imp_resp / detect_burst, with the normal-burst
    (grgsm_vitac.cpp:265-273) or access (:246-255) window and sequence."""
    x = M.scale_samples(y, O.VA_SCALE)
    if ctype == O.TSC:
        center, nbits, ss = 3 + 58 + 5, 148, 3
        seq = M.norm_seq([int(c) for c in synth.TSC_BITS[tsc]])
    else:
        center, nbits, ss = 8 + 5, 88, max_toa
        seq = M.acc_seq()
    pos, cir, _ = M.get_chan_imp_resp(x, (center - 5) * 4 + 1, (center + 5 + 5) * 4, seq)
    start = max(pos - center * 4, 0)
    out = M.detect_burst(x, cir, start, nbits, ss)
    soft = np.zeros(148, dtype=np.float32)
    soft[:nbits] = np.where(out > 0, 127.0, -127.0)
    return start, soft


def test_model_equals_c_oracle_on_normal_bursts():
    rng = np.random.default_rng(101)
    for k in range(32):
        y, _ = _va_burst(rng, k % 8, int(rng.integers(0, 22)), snr_db=rng.uniform(3, 30), amp=10 ** rng.uniform(2.5, 4.2))
        st, ref = O.demod_any_burst_va(y, O.TSC, k % 8, 3)
        mst, msoft = _model_va(y, O.TSC, k % 8, 3)
        assert mst == st, k
        assert np.array_equal(msoft, ref[:148]), k


def test_model_equals_c_oracle_on_access_bursts():
    rng = np.random.default_rng(102)
    for k in range(8):
        bits = np.concatenate([np.array([0, 0, 1, 1, 1, 0, 1, 0], np.uint8), M.ACCESS_BITS, rng.integers(0, 2, 36, dtype=np.uint8),
                               np.zeros(3, np.uint8)])
        x = O.modulate_burst(bits, 8, 4)
        off = int(rng.integers(0, 26))
        y = np.zeros(625, dtype=np.complex64)
        m = min(len(x), 625 - off)
        y[off:off + m] = x[:m] * np.complex64(4000.0 * np.exp(1j * rng.uniform(0, 6.28)))
        y += ((rng.normal(size=625) + 1j * rng.normal(size=625)) * rng.uniform(10, 800)).astype(np.complex64)
        max_toa = [3, 0, 12, 15][k % 4]
        st, ref = O.demod_any_burst_va(y, O.RACH, 0, max_toa)
        mst, msoft = _model_va(y, O.RACH, 0, max_toa)
        assert mst == st, k
        assert np.array_equal(msoft, ref[:148]), k


def test_kernel_training_codes_equal_the_run_time_walk():
    src = open(os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_sch_sync.hip")).read()
    lo = int(re.search(r"#define SS_SCH_CODES_LO (0x[0-9a-f]+)ull", src).group(1), 16)
    hi = int(re.search(r"#define SS_SCH_CODES_HI (0x[0-9a-f]+)ull", src).group(1), 16)
    seq = M.sch_seq()
    assert len(seq) == 54
    assert M.quarter_codes(seq) == lo | (hi << 64)
    assert synth.SCH_SYNC == "".join(str(b) for b in M.SYNC_BITS)


def _sbits(bits):
    return np.where(np.asarray(bits) > 0, -127, 127).astype(np.int8)


def test_coding_round_trip_all_bsic_and_frames():
    """synth.sch_burst_bits -> decoder model gives the fields back.  The last SCH frame of the hyperframe is 2 715 647 - 9 (frame 41
    of the last 51-multiframe); 2 715 647 - 6 is frame 44 and carries no SCH, the encoder refuses it."""
    rng = np.random.default_rng(103)
    fns = [1, 11, 41, 51 * 26 - 10, 2715647 - 9] + [int(f) for f in synth.random_sch_frames(200, rng)]
    assert all(f % 51 in (1, 11, 21, 31, 41) for f in fns)
    with pytest.raises(ValueError):
        synth.sch_burst_bits(0, 2715647 - 6)
    branches = set()
    sent, data = [], []
    for fn in fns:
        for bsic in range(64):
            b = _sbits(synth.sch_burst_bits(bsic, fn))
            data.append(np.concatenate([b[3:42], b[106:145]]))
            sent.append((bsic, fn))
    u = M.conv_decode(np.stack(data))
    for (bsic, fn), ub in zip(sent, u):
        assert np.array_equal(M.crc10(ub[:25]), ub[25:35]) and not ub[35:].any()
        gb, t1, t2, t3p = M.sch_parse(ub[:25])
        gfn, low = M.sch_to_fn(t1, t2, t3p)
        branches.add(bool(low))
        assert (gb, gfn) == (bsic, fn)
        assert (t1, t2, t3p) == (fn // 1326, fn % 26, (fn % 51 - 1) // 10)
    assert branches == {False, True}                               # both branches of gsm_sch_to_fn
    # the whole decode_sch() on a few of them
    for bsic, fn in sent[::997]:
        r = M.decode_sch(_sbits(synth.sch_burst_bits(bsic, fn)))
        assert (r["rc"], r["bsic"], r["fn"]) == (1, bsic, fn)


def test_bit_flips():
    rng = np.random.default_rng(104)
    for _ in range(40):
        bsic, fn = int(rng.integers(0, 64)), int(synth.random_sch_frames(1, rng)[0])
        bits = synth.sch_burst_bits(bsic, fn)
        # one flipped information bit: re-encoded without fixing the parity
        info = synth.sch_info_bits(bsic, fn)
        k = int(rng.integers(0, 25))
        good = M.conv_decode(np.concatenate([_sbits(bits)[3:42], _sbits(bits)[106:145]]))
        bad = good.copy()
        bad[k] ^= 1
        assert np.array_equal(good[:25], info)
        c = M.conv_encode(bad)
        b2 = bits.copy()
        b2[3:42], b2[106:145] = c[:39], c[39:]
        assert M.decode_sch(_sbits(b2))["rc"] == 0
        # three flipped coded bits: the free distance of the code is 7
        b3 = bits.copy()
        pos = rng.choice(np.concatenate([np.arange(3, 42), np.arange(106, 145)]), 3, replace=False)
        b3[pos] ^= 1
        r = M.decode_sch(_sbits(b3))
        assert (r["rc"], r["bsic"], r["fn"]) == (1, bsic, fn)


def _sch_wave(bsic, fn):
    return O.modulate_burst(synth.sch_burst_bits(bsic, fn), 8, 4)


def _buffer(rng, wave, L, off, snr_db, amp=3000.0):
    sigma = amp * 10 ** (-snr_db / 20) / np.sqrt(2)
    y = ((rng.normal(size=L) + 1j * rng.normal(size=L)) * sigma).astype(np.complex64)
    m = max(0, min(len(wave), L - off))
    y[off:off + m] += wave[:m] * np.complex64(amp * np.exp(1j * rng.uniform(0, 2 * np.pi)))
    return y


def test_chain_track():
    rng = np.random.default_rng(105)
    for snr in (25.0, 10.0):
        for off in (0, 1, 4, 10, 20, 30, 39):
            bsic, fn = int(rng.integers(0, 64)), int(synth.random_sch_frames(1, rng)[0])
            y = _buffer(rng, _sch_wave(bsic, fn), 625, off, snr)
            r = M.sch_sync(y, M.TRACK, SCALE)
            assert (r["rc"], r["bsic"], r["fn"]) == (1, bsic, fn), (snr, off, r)
            assert (r["t1"], r["t2"], r["t3p"]) == (fn // 1326, fn % 26, (fn % 51 - 1) // 10)
            assert abs(r["start"] - off) <= 6 and -39 <= r["start"] <= 39


def test_chain_acq():
    rng = np.random.default_rng(106)
    for off in (0, 7, 300, 1250, 2503):
        bsic, fn = int(rng.integers(0, 64)), int(synth.random_sch_frames(1, rng)[0])
        y = _buffer(rng, _sch_wave(bsic, fn), 5000, off, 25.0)
        r = M.sch_sync(y, M.ACQ, SCALE)
        assert (r["rc"], r["bsic"], r["fn"]) == (1, bsic, fn), (off, r)
        assert abs(r["start"] - off) <= 6


def test_library_exports_and_wrapper():
    from osmo_trx_amd import trxhip
    L = trxhip.load_library()
    for name in ("trxhip_sch_sync_batch_cf32", "trxhip_sch_sync_batch_i16"):
        assert hasattr(L, name) and name in trxhip.SYMBOLS
    assert callable(trxhip.TrxHip.sch_sync)
    assert trxhip.SCH_SYNC_DTYPE.itemsize == 24
    assert [trxhip.SCH_SYNC_DTYPE.fields[f][1] for f in ("rc", "start", "corr_max", "fn", "t1", "bsic", "t2", "t3p")] == \
        [0, 4, 8, 12, 16, 18, 19, 20]
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    assert int(re.search(r"#define TRXHIP_SCH_SYNC_MAX_LEN \(1 << (\d+)\)", hdr).group(1)) == 20
    assert trxhip.SCH_SYNC_MAX_LEN == 1 << 20 >= 60000
