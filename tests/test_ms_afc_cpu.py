"""CPU tests of the MS-side FCCH frequency-offset measurement: the model (tests/ms_afc_model.py, the literal restatement of
gsm_fcch_offset()) on tones and noise, its float32 form against its float64 form, pinv(), the all-zero slot, and what the header, the
wrapper and the library agree on.  No GPU is opened."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ms_afc_cases as AC
import ms_afc_model as AM
from osmo_trx_amd import trxhip

EINVAL = -22
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- tone recovery ------------------------------------------------------------------------------------------------------

def test_model_recovers_a_tone_to_a_fifth_of_a_hertz():
    """noise-free int16 tones at amplitude 8000, 2.5 kHz steps from -82.5 to +90 kHz around 67 708.33 Hz, random start phase: both
    forms of the model read cfo + 8.33 Hz (expected_fcch_val is built from 67700) to <= 0.2 Hz"""
    rng = np.random.default_rng(7)
    worst = 0.0
    for cfo in np.arange(-82500.0, 90000.0 + 1, 2500.0):
        x = AM.scaled(AM.to_i16(AM.tone(cfo, AC.TONE_AMP, rng.uniform(0, 2 * math.pi))), AC.FULL)
        for acc in (np.float32, np.float64):
            m = AM.fcch_offset(x, acc)
            err = abs(float(m["hz"]) - (cfo + AC.BIAS_HZ))
            worst = max(worst, err)
            assert err <= 0.2, (cfo, acc, err)
            assert float(m["mag_one"]) / float(m["energy"]) > 0.99            # the caller's tone test
    print("worst tone error: %.4f Hz" % worst)


def test_model_aliases_below_minus_85_khz():
    """the estimator's range, documented by a test: a carrier 90 kHz low reads about 17 kHz off (no pair (r, s) has its P)"""
    m = AM.fcch_offset(AM.scaled(AM.to_i16(AM.tone(-90000.0, AC.TONE_AMP, 0.3)), AC.FULL))
    off = float(m["hz"]) - (-90000.0 + AC.BIAS_HZ)
    assert 16000 < off < 18000, off
    assert (m["r"], m["s"]) == (0, 0) and AM.pinv(m["p"]) == (0, 0) and m["p"] != 0


# ---- float32 in the reference's order against float64 -----------------------------------------------------------------------

def test_float32_form_agrees_with_float64_form():
    rows, n_tones = AC.row_set()
    want = AC.models("cpu")
    xs = AM.scaled(rows, AC.FULL)
    worst_tone = 0.0
    for i, (x, b) in enumerate(zip(xs, want)):
        a = AM.fcch_offset(x, np.float32)
        assert (a["p"], a["r"], a["s"]) == (b["p"], b["r"], b["s"]), i
        d = abs(float(a["hz"]) - float(b["hz"]))
        assert d <= AM.hz_bar(b), (i, d, AM.hz_bar(b))
        if i < n_tones:
            worst_tone = max(worst_tone, d)
    print("float32 against float64 on tones: %.4f Hz" % worst_tone)
    assert len(rows) == 430 and n_tones == 30


def test_row_set_is_decided():
    """what the GPU test may leave out of its (p, r, s) comparison: rows whose P_unrounded lies inside the error margin of a
    half-integer -- at most 2 % of the set, and no tone row"""
    want = AC.models("device")
    n_tones = AC.device_row_set()[1]
    inside = [i for i, m in enumerate(want[:-1]) if AM.decision_margin(m) <= 0]          # (the last row is all zero: exact)
    assert len(inside) <= 0.02 * len(want) and all(i >= n_tones for i in inside), inside


# ---- pinv, the all-zero slot ----------------------------------------------------------------------------------------------

def test_pinv_table():
    pairs = {}
    for i in range(3):
        for j in range(32):
            pairs.setdefault(32 * i - 3 * j, (i, j))               # the first pair in the reference's loop order
    assert len(pairs) == 96                                         # 32 and 3 are coprime: no P has two pairs
    for P in range(-120, 121):
        assert AM.pinv(P) == pairs.get(P, (0, 0)), P
    assert AM.pinv(0) == (0, 0) and AM.pinv(32) == (1, 0) and AM.pinv(-3) == (0, 1) and AM.pinv(29) == (1, 1)
    assert AM.pinv(64) == (2, 0) and AM.pinv(-93) == (0, 31) and AM.pinv(1) == (2, 21)
    assert AM.pinv(3) == (0, 0) and AM.pinv(65) == (0, 0) and AM.pinv(-94) == (0, 0)      # no pair: the caller's r = s = 0


def test_all_zero_slot():
    for acc in (np.float32, np.float64):
        m = AM.fcch_offset(np.zeros(625, np.complex64), acc)
        assert (m["alpha_one"], m["alpha_two"], m["p"], m["r"], m["s"]) == (0, 0, 0, 0, 0)
        assert m["mag_one"] == 0 and m["mag_two"] == 0 and m["energy"] == 0
        want = -F(AM.GSM_SYM_RATE / (2 * math.pi) * float(AM.EXPECTED_FCCH_VAL))
        assert m["hz"] == want and abs(float(want) + 67700) < 0.01
    assert AM.FS == F(1083333.375) and (AM.FIRST, AM.LAST) == (52, 175)


# ---- header, wrapper, library -----------------------------------------------------------------------------------------------

def header():
    return open(os.path.join(ROOT, "include", "trxhip.h")).read()


def struct_fields(hdr, name):
    """the field names of `typedef struct [tag] { ... } name;` in declaration order"""
    body = re.search(r"typedef struct\s*\w*\s*\{([^{}]*)\}\s*" + name + r"\s*;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.sub(r"[\s*]|\[.*\]", "", n) for n in decl.strip().split(None, 1)[1].split(",")]
    return names


def test_header_constants_and_struct_layouts():
    hdr = header()
    assert ["%d" % trxhip.MS_AFC_RING] == re.findall(r"#define TRXHIP_MS_AFC_RING\s+(\d+)", hdr) == ["8"]
    assert struct_fields(hdr, "trxhip_ms_fcch") == list(trxhip.MS_FCCH_DTYPE.names)
    assert struct_fields(hdr, "trxhip_ms_afc_entry") == list(trxhip.MS_AFC_ENTRY_DTYPE.names)
    assert struct_fields(hdr, "trxhip_ms_afc_status") == list(trxhip.MS_AFC_STATE_DTYPE.names)
    assert struct_fields(hdr, "trxhip_ms_afc_cfg") == [f[0] for f in trxhip._MsAfcCfg._fields_]
    assert trxhip.MS_FCCH_DTYPE.itemsize == 32 and trxhip.MS_AFC_ENTRY_DTYPE.itemsize == 16
    assert trxhip.MS_AFC_STATE_DTYPE.itemsize == 176 and C.sizeof(trxhip._MsAfcCfg) == 16
    assert [trxhip.MS_FCCH_DTYPE.fields[k][1] for k in ("hz", "energy", "p", "r", "s", "reserved")] == [0, 20, 24, 26, 27, 28]
    assert trxhip.MS_AFC_STATE_DTYPE.fields["last"][1] == 16 and trxhip.MS_AFC_STATE_DTYPE.fields["ring"][1] == 48
    from osmo_trx_amd import MS_FCCH_DTYPE, MS_AFC_STATE_DTYPE
    assert MS_FCCH_DTYPE is trxhip.MS_FCCH_DTYPE and MS_AFC_STATE_DTYPE is trxhip.MS_AFC_STATE_DTYPE
    # the kernel's constants are the reference's, as the model has them
    k = open(os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_ms_afc.h")).read()
    got = {n: int(v) for n, v in re.findall(r"#define TRX_AFC_(START|L1|L2|N)\s+(\d+)", k)}
    assert got == dict(START=AM.START, L1=AM.L1, L2=AM.L2, N=AM.N1) and AM.N1 == AM.N2


def test_symbols_and_abi():
    L = trxhip.load_library()
    hdr = header()
    names = ["trxhip_ms_fcch_batch_i16", "trxhip_ms_fcch_batch_cf32"] + \
        ["trxhip_ms_afc_%s_%s" % (o, f) for o in ("sched", "group") for f in ("set", "state")]
    for name in names:
        assert hasattr(L, name) and name in trxhip.SYMBOLS and name + "(" in hdr, name
    assert L.trxhip_abi_version() == 5 and re.search(r"^#define\s+TRXHIP_ABI_VERSION\s+5\b", hdr, re.M)
    for cls in (trxhip.MsRxScheduler, trxhip.MsRxSchedulerGroup):
        assert hasattr(cls, "set_afc") and hasattr(cls, "afc_state")
    assert hasattr(trxhip.TrxHip, "ms_fcch")


def test_plan_only_objects_refuse():
    """a plan-only object has no samples: _set is EINVAL whatever it asks for; _state reports the empty state; pulls go on"""
    s = trxhip.MsRxScheduler(None, tracking=False)
    s.set_clock(51 * 3, 7, 0)
    for enable in (True, False):
        with pytest.raises(trxhip.TrxHipError):
            s.set_afc(enable)
    cfg = trxhip._MsAfcCfg(1, 0, None)
    assert s.L.trxhip_ms_afc_sched_set(s.h, C.byref(cfg)) == EINVAL and s.L.trxhip_ms_afc_sched_set(s.h, None) == EINVAL
    assert s.pull(n_samples=625 * 100, first_ts=625)[0] == 100
    st = s.afc_state()
    assert st == dict(count=0, enable=False, last=None, ring=[])
    g = trxhip.MsRxSchedulerGroup(None, 3, tracking=False)
    for m in range(3):
        with pytest.raises(trxhip.TrxHipError):
            g.set_afc(m, True)
        assert g.afc_state(m) == dict(count=0, enable=False, last=None, ring=[])
    a = np.zeros(1, dtype=trxhip.MS_AFC_STATE_DTYPE)
    assert g.L.trxhip_ms_afc_group_state(g.h, 3, a.ctypes.data_as(C.c_void_p)) == EINVAL     # no such member
    assert g.L.trxhip_ms_afc_group_state(g.h, 0, None) == EINVAL
    assert g.L.trxhip_ms_afc_group_set(g.h, 3, C.byref(cfg)) == EINVAL
