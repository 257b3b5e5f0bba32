"""CPU tests of the MS-side downlink burst receiver (trxhip_ms_rx_batch_*): the model the GPU tests compare with
(tests/ms_rx_model.py) is pinned to the C oracle where the oracle covers the same code, it receives what was sent, the slot kinds
are the reference's, and the library and the wrapper carry the new entry points.  No GPU is opened."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ms_rx_cases as K
import ms_rx_model as M
import oracle_lib as O
from osmo_trx_amd import trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_SCALE = 2047.0
EINVAL = -22


def test_model_equals_c_oracle_where_the_start_is_not_negative():
    """demodAnyBurst_va (Transceiver.cpp:620-645) runs the same get_norm_chan_imp_resp and detect_burst_nb but clamps the start to
    >= 0: wherever the model's start is >= 0 the two must give the same start and the same hard decisions (the oracle's soft bits
    are the sbits times -1, Transceiver.cpp:638)."""
    rng = np.random.default_rng(901)
    scale = np.float32(1.0) / np.float32(FULL_SCALE)
    same = 0
    for k in range(32):
        tsc = k % 8
        y, _ = K.nb_slot(rng, tsc, int(rng.integers(-6, 25)), snr_db=float(rng.uniform(3, 30)), amp=float(10 ** rng.uniform(1.5, 3.3)))
        m = M.ms_rx(y, 7, 2, tsc, True, FULL_SCALE)
        assert m["kind"] == M.KIND_NB and m["sent"] == 1
        if m["start"] < 0:
            continue
        st, ref = O.demod_any_burst_va(y, O.TSC, tsc, 0, scale)
        assert st == m["start"], k
        assert np.array_equal(m["bits"], -ref[:148].astype(np.int8)), k
        same += 1
    assert same >= 20


def test_model_equals_c_oracle_on_int16_samples():
    rng = np.random.default_rng(902)
    scale = np.float32(1.0) / np.float32(FULL_SCALE)
    y, _ = K.nb_slot(rng, 5, 9, snr_db=12.0, amp=1500.0)
    q = K.to_i16(y)
    m = M.ms_rx(q, 3, 1, 5, True, FULL_SCALE)
    st, ref = O.demod_any_burst_va((q[:, 0] + 1j * q[:, 1]).astype(np.complex64), O.TSC, 5, 0, scale)
    assert m["start"] == st >= 0 and np.array_equal(m["bits"], -ref[:148].astype(np.int8))


def test_model_receives_what_was_sent():
    """The 59-lag search follows burst offsets on both sides of the slot start; the bits come out without an error where the
    burst's head is still inside the slot."""
    rng = np.random.default_rng(903)
    for snr in (25.0, 10.0):
        for off in range(-24, 25, 4):
            tsc = int(rng.integers(0, 8))
            y, bits = K.nb_slot(rng, tsc, off, snr_db=snr)
            m = M.ms_rx(y, 5, 3, tsc, True, FULL_SCALE)
            assert -39 <= m["start"] <= 39
            if -19 <= off <= 20:
                # the 20-sample energy window is coarse by design: the estimate lies within one window of the true position
                assert abs(m["start"] - off) < 20, (snr, off, m["start"])
            if -12 <= off <= 16:
                assert np.array_equal(m["bits"], K.hard(bits)), (snr, off)
            # :272 divides rxFullScale by the level of the SCALED samples, here 3000 / 2047
            assert m["flags"] == 0 and abs(m["rssi_exact"] - 20 * np.log10(FULL_SCALE / (3000.0 / FULL_SCALE))) < 1.0
            assert m["rssi"] == int(np.floor(m["rssi_exact"])) and m["toa256"] == 0


def test_energy_and_rssi_of_known_slots():
    full = np.full((625, 2), 32767, dtype=np.int16)
    full[::2] = -32767
    m = M.ms_rx(full, 5, 1, 0, True, 32767.0)
    # every scaled sample is (+-1, +-1): norm2 = 2, the mean of 80 of them 2, 20 log10(32767 / sqrt 2) = 87.3
    assert m["pow"] == np.float32(2.0) and m["rssi"] == 87 and m["flags"] == 0
    z = M.ms_rx(np.zeros((625, 2), dtype=np.int16), 5, 1, 0, True, 32767.0)
    assert z["pow"] == 0 and z["rssi"] == 0 and z["flags"] == M.IND_SILENT and z["sent"] == 1 and z["start"] == -19
    # only the samples 0, 4, ..., 316 count
    one = np.zeros(625, dtype=np.complex64)
    one[316] = 3.0 + 4.0j
    one[317:] = 100.0
    one[1:4] = 100.0
    assert M.energy_detect(one) == np.float32(25.0 / 80.0)


def test_slot_kinds_not_demodulated():
    rng = np.random.default_rng(904)
    y, _ = K.nb_slot(rng, 0, 3)
    a = M.ms_rx(y, 10, 0, 0, True)                                   # FCCH
    assert (a["kind"], a["sent"], a["flags"], a["sch_fn"]) == (M.KIND_FCCH, 1, M.IND_TRASH, -1) and not a["bits"].any()
    b = M.ms_rx(y, 10, 0, 0, False)
    assert (b["kind"], b["sent"], b["flags"]) == (M.KIND_FCCH, 0, 0)
    c = M.ms_rx(y, 10, 1, 0, False)                                  # traffic, not active
    assert (c["kind"], c["sent"], c["start"], c["pow"], c["sch_fn"]) == (M.KIND_NB, 0, 0, 0, -1) and not c["bits"].any()
    for fn, tn, tsc in ((10, 8, 0), (10, 1, 8), (12, 0, 200)):
        d = M.ms_rx(y, fn, tn, tsc, True)
        assert (d["kind"], d["sent"], d["flags"], d["sch_fn"]) == (M.KIND_BAD, 0, 0, -1) and not d["bits"].any()
    assert M.ms_rx(y, 11, 0, 200, True)["kind"] == M.KIND_SCH        # the TSC of an SCH slot is not looked at
    s = K.sch_slot(rng, 41, 51 * 300 + 11, 7)
    for active in (True, False):
        e = M.ms_rx(s, 51 * 300 + 11, 0, 0, active)
        assert (e["kind"], e["sent"], e["rssi"], e["toa256"]) == (M.KIND_SCH, int(active), 10, 0)
        assert (e["sch_rc"], e["sch_fn"], e["sch_bsic"]) == (1, 51 * 300 + 11, 41)


def _ref_fcch_check_fn(fn):
    """gsm_fcch_check_fn, sch.c:100-114, statement by statement"""
    fn51 = fn % 51
    if fn51 == 0 or fn51 == 10 or fn51 == 20 or fn51 == 30 or fn51 == 40:
        return 1
    return 0


def _ref_sch_check_fn(fn):
    """gsm_sch_check_fn, sch.c:117-131"""
    fn51 = fn % 51
    if fn51 == 1 or fn51 == 11 or fn51 == 21 or fn51 == 31 or fn51 == 41:
        return 1
    return 0


def test_ms_slot_kind_over_a_multiframe():
    counts = {k: 0 for k in range(4)}
    for base in (0, 51 * 26 * 2047, 2715648 - 51):
        for fn in range(base, base + 51):
            for tn in range(8):
                is_fcch = tn == 0 and _ref_fcch_check_fn(fn)         # gsm_fcch_check_ts, sch.c:133-135
                is_sch = tn == 0 and _ref_sch_check_fn(fn)           # gsm_sch_check_ts, sch.c:137-139
                want = trxhip.MS_KIND_FCCH if is_fcch else trxhip.MS_KIND_SCH if is_sch else trxhip.MS_KIND_NB
                assert trxhip.ms_slot_kind(fn, tn) == want == M.slot_kind(fn, tn), (fn, tn)
                counts[want] += 1
    assert counts == {0: 0, 1: 15, 2: 15, 3: 3 * 408 - 30}
    assert trxhip.ms_slot_kind(5, 8) == trxhip.ms_slot_kind(5, 255) == trxhip.MS_KIND_BAD
    assert trxhip.ms_slot_kind(5, 1, 8) == trxhip.MS_KIND_BAD and trxhip.ms_slot_kind(5, 1, 7) == trxhip.MS_KIND_NB
    assert trxhip.ms_slot_kind(1, 0, 8) == trxhip.MS_KIND_SCH and trxhip.ms_slot_kind(0, 0, 8) == trxhip.MS_KIND_FCCH
    assert (trxhip.MS_KIND_BAD, trxhip.MS_KIND_FCCH, trxhip.MS_KIND_SCH, trxhip.MS_KIND_NB) == \
        (M.KIND_BAD, M.KIND_FCCH, M.KIND_SCH, M.KIND_NB)


def test_library_exports_and_wrapper():
    import torch
    L = trxhip.load_library()
    for name in ("trxhip_ms_rx_batch_i16", "trxhip_ms_rx_batch_cf32"):
        assert hasattr(L, name) and name in trxhip.SYMBOLS
    assert callable(trxhip.TrxHip.ms_rx)
    # the records and the constants are the header's
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    for name in ("MS_KIND_BAD", "MS_KIND_FCCH", "MS_KIND_SCH", "MS_KIND_NB", "MS_SLOT_ACTIVE", "MS_IND_TRASH", "MS_IND_SILENT"):
        assert int(re.search(r"#define TRXHIP_%s\s+(\d+)" % name, hdr).group(1)) == getattr(trxhip, name), name
    assert trxhip.MS_SLOT_DTYPE.itemsize == 8 and trxhip.MS_IND_DTYPE.itemsize == 32
    assert [trxhip.MS_SLOT_DTYPE.fields[f][1] for f in ("fn", "tn", "tsc", "flags", "reserved")] == [0, 4, 5, 6, 7]
    assert [trxhip.MS_IND_DTYPE.fields[f][1] for f in ("fn", "tn", "kind", "sent", "flags", "rssi", "toa256", "start", "corr_max", "pow",
                                                        "sch_fn", "sch_rc", "sch_bsic", "reserved")] == \
        [0, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 28, 29, 30]
    # the C entry points refuse a NULL context before they look for a device
    buf = (C.c_char * 64)()
    for fn in (L.trxhip_ms_rx_batch_i16, L.trxhip_ms_rx_batch_cf32):
        assert fn(None, buf, 625, buf, buf, None, 1, 2047.0, None) == EINVAL
    # ... and the wrapper refuses what the library would, before it touches the GPU
    geo = trxhip.TrxHip.ms_rx_geometry
    slots = np.zeros(3, dtype=trxhip.MS_SLOT_DTYPE)
    i16 = torch.zeros((3, 700, 2), dtype=torch.int16)
    cf = torch.zeros((3, 625), dtype=torch.complex64)
    assert geo(i16, slots, 2047.0) == (3, 700, True) and geo(cf, slots, 32767.0) == (3, 625, False)
    assert geo(cf, torch.zeros((3, 8), dtype=torch.uint8), 1.0) == (3, 625, False)
    bad = [
        (torch.zeros((3, 624, 2), dtype=torch.int16), slots, 2047.0),       # slot_stride < 625
        (torch.zeros((0, 625, 2), dtype=torch.int16), slots[:0], 2047.0),   # no slot
        (torch.zeros((3, 625), dtype=torch.int16), slots, 2047.0),          # int16 without the IQ axis
        (torch.zeros((3, 625), dtype=torch.float32), slots, 2047.0),        # no such sample type
        (cf, slots[:2], 2047.0),                                            # one record per slot
        (cf, np.zeros(3, dtype=np.uint64), 2047.0),
        (cf, torch.zeros((3, 4), dtype=torch.uint8), 2047.0),
        (cf, slots, 0.0), (cf, slots, -1.0), (cf, slots, float("inf")), (cf, slots, float("nan")),
    ]
    for a in bad:
        with pytest.raises(trxhip.TrxHipError):
            geo(*a)
