"""CPU tests of the MS-side NCO: the phasor tables, the increment and the phase against the numpy restatement
(tests/ms_nco_model.py), the bookkeeping of plan-only scheduler objects, the exports and the header, and -- on the CPU models of the
receiver and of the FCCH estimator alone -- the measure-then-correct loop on the very stream the GPU test runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ms_afc_model as AM
import ms_nco_model as NM
import ms_rx_cases as K
import ms_rx_model as RX
from osmo_trx_amd import trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FULL = 2047.0


# ---- the tables -------------------------------------------------------------------------------------------------------------

def test_tables_exact_entries_and_one_ulp():
    c, f = trxhip.ms_nco_tables_host()
    assert c.dtype == np.float32 and c.shape == f.shape == (1024, 2)
    for a, want in ((0, (1, 0)), (256, (0, 1)), (512, (-1, 0)), (768, (0, -1))):
        assert tuple(c[a]) == want and not np.signbit(c[a][np.array(want) == 0]).any(), (a, c[a])
    assert tuple(f[0]) == (1, 0)
    # within one float32 ulp of numpy's double cos / sin.  The double reference itself errs by up to 2^-52: its argument
    # 2 pi a / 1024 is a rounded double (cos(pi / 2) reads 6e-17 there, and is 0 in the table), which is what the bar adds
    for got, ref in zip((c, f), NM.tables_numpy()):
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - ref) <= ulp + 2.0 ** -52).all()
    # the coarse table is its first quadrant turned: (c, s) -> (-s, c)
    assert (c[256:, 0] == -c[:768, 1]).all() and (c[256:, 1] == c[:768, 0]).all()


# ---- increment and phase ------------------------------------------------------------------------------------------------------

HZ = [0.0] + [s * v for v in (0.0003, 2000.0, 67708.33, 270833.0, 500000.0) for s in (1, -1)]


def test_inc_against_restatement_and_refusals():
    L = trxhip.load_library()
    for hz in HZ:
        assert trxhip.ms_nco_inc(hz) == NM.inc_of(hz), hz
        assert -2 ** 31 <= trxhip.ms_nco_inc(hz) < 2 ** 31
    assert trxhip.ms_nco_inc(2000.0) == 7929170 and trxhip.ms_nco_inc(0.0003) == 1 and trxhip.ms_nco_inc(-0.0003) == -1
    inc = C.c_int32(77)
    for hz in (500000.1, -500000.1, float("nan"), float("inf")):
        assert L.trxhip_ms_nco_inc(hz, C.byref(inc)) == EINVAL and inc.value == 77
        with pytest.raises(ValueError):
            NM.inc_of(hz)
    assert L.trxhip_ms_nco_inc(0.0, None) == EINVAL


def test_phase_against_restatement():
    rng = np.random.default_rng(11)
    incs = [0, 1, -1, 2 ** 31 - 1, -2 ** 31] + [NM.inc_of(h) for h in HZ]
    around = [0, 2 ** 31, 2 ** 32, 2 ** 40]
    ts_set = [b + d for b in around for d in (-626, -1, 0, 1, 625)]
    for inc in incs:
        for ts_ref in ts_set:
            acc = int(rng.integers(0, 2 ** 32))
            for ts in ts_set:                                      # (ts - ts_ref is negative in half of the pairs)
                assert trxhip.ms_nco_phase(acc, ts_ref, inc, ts) == NM.phase(acc, ts_ref, inc, ts), (acc, ts_ref, inc, ts)
    # the phase is a function of the absolute timestamp: moving the reference along the ramp changes nothing
    acc, inc = 0x9E3779B9, NM.inc_of(-67708.33)
    moved = NM.phase(acc, 1000, inc, 2 ** 40 + 5)
    assert trxhip.ms_nco_phase(moved, 2 ** 40 + 5, inc, 123) == trxhip.ms_nco_phase(acc, 1000, inc, 123)


def test_model_rotation_identity_and_quarter_turns():
    tabs = trxhip.ms_nco_tables_host()
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, (700, 2)).astype(np.int16)
    same = NM.rotate(tabs, x, 0, 0)
    assert (same.real == x[:, 0]).all() and (same.imag == x[:, 1]).all()
    q = NM.rotate(tabs, x, 1 << 30, 0)                             # a quarter turn: (xr, xi) -> (-xi, xr), exactly
    assert (q.real == -x[:, 1].astype(np.float32)).all() and (q.imag == x[:, 0]).all()
    # against the rotation in double: the phase loses its low 12 bits (< 6e-6 rad) and every step rounds to float32
    inc = NM.inc_of(2000.0)
    got = NM.rotate(tabs, x, 12345, inc)
    p = (12345 + np.arange(700) * inc) % 2 ** 32
    want = (x[:, 0] + 1j * x[:, 1].astype(np.float64)) * np.exp(2j * np.pi * p / 2 ** 32)
    assert np.abs(got - want).max() <= np.abs(want).max() * (6e-6 + 8 * 2.0 ** -24)


# ---- plan-only objects ----------------------------------------------------------------------------------------------------------

SEQ = (("pull", 625 * 20 + 300), ("set", True, 2000.0), ("pull", 1000), ("set", True, -67708.33), ("pull", 625 * 9 - 100),
       ("set", False, 0.0), ("pull", 700), ("set", True, 270833.0), ("pull", 625 * 3), ("set", True, 0.0), ("pull", 55))
T0 = 2 ** 40 - 3000
STARTS = [3, -2, 0, 1, 5]


def run_single(with_nco):
    s = trxhip.MsRxScheduler(None, tracking=True)
    s.set_clock(51 * 4 - 1, 7, T0 - 625)
    s.feed_starts(STARTS)
    nco, plans, at = NM.Nco(), [], T0
    for step in SEQ:
        if step[0] == "pull":
            plans.append((s.pull(n_samples=step[1], first_ts=at), s.plan().tobytes(), s.clock(), s.state().tobytes()))
            at += step[1]
        elif with_nco:
            s.set_nco(step[1], step[2])
            nco.set(step[1], step[2], s.clock()[2])
            assert s.nco_state() == nco.state()
    return plans, s.nco_state(), nco


def test_plan_only_single_object():
    plans_on, st, nco = run_single(True)
    plans_off, st_off, _ = run_single(False)
    assert plans_on == plans_off                                   # the NCO moves nothing of the cutter, the clock or the plan
    assert st == nco.state() and st["enable"] and st["inc"] == 0
    assert st_off == dict(enable=False, inc=0, acc=0, ts_ref=0, hz=0.0)
    # a refused pull and the setters leave the NCO alone
    s = trxhip.MsRxScheduler(None, tracking=False)
    s.set_nco(True, 1234.5)                                        # before a clock is set: at ts 0
    assert s.nco_state() == dict(enable=True, inc=NM.inc_of(1234.5), acc=0, ts_ref=0, hz=1234.5)
    s.set_clock(100, 3, 5000)
    before = s.nco_state()
    with pytest.raises(trxhip.TrxHipError):
        s.pull(n_samples=0, first_ts=5625)
    s.set_tsc(3)
    s.set_active(0x0F)
    s.set_clock(7, 7, 99)
    assert s.nco_state() == before
    s.set_nco(True, -1234.5)                                       # continuous: acc is the old ramp at the new clock
    assert s.nco_state()["acc"] == NM.phase(0, 0, NM.inc_of(1234.5), 99) and s.nco_state()["ts_ref"] == 99


def test_plan_only_group_of_three():
    def run(with_nco):
        g = trxhip.MsRxSchedulerGroup(None, 3, tracking=[True, False, True])
        ncos = [NM.Nco() for _ in range(3)]
        t0 = [T0, 1000, 2 ** 32 - 700]
        for m in range(3):
            g.set_clock(m, 51 * 4 - 1, 7, t0[m] - 625)
            g.feed_starts(m, STARTS)
        at, out = list(t0), []
        for k, step in enumerate(SEQ):
            if step[0] == "pull":
                sizes = [step[1], step[1] + 17, 0 if k % 4 == 2 else step[1] + 625]
                out.append((g.pull(n_samples=sizes, first_ts=at), [g.clock(m) for m in range(3)]))
                at = [a + n for a, n in zip(at, sizes)]
            elif with_nco:
                for m, hz in ((0, step[2]), (2, -step[2] / 2)):    # member 1 never has it
                    g.set_nco(m, step[1], hz)
                    ncos[m].set(step[1], hz, g.clock(m)[2])
                for m in range(3):
                    assert g.nco_state(m) == ncos[m].state(), m
        return out
    assert run(True) == run(False)
    g = trxhip.MsRxSchedulerGroup(None, 3)
    cfg = trxhip._MsNcoCfg(1, 0, 100.0)
    a = np.zeros(1, dtype=trxhip.MS_NCO_STATE_DTYPE)
    assert g.L.trxhip_ms_nco_group_set(g.h, 3, C.byref(cfg)) == EINVAL             # no such member
    assert g.L.trxhip_ms_nco_group_state(g.h, 3, a.ctypes.data_as(C.c_void_p)) == EINVAL
    assert g.L.trxhip_ms_nco_group_set(g.h, 0, None) == EINVAL and g.L.trxhip_ms_nco_group_state(g.h, 0, None) == EINVAL
    for hz in (500000.1, -500000.1, float("nan")):
        with pytest.raises(trxhip.TrxHipError):
            g.set_nco(1, True, hz)
    assert g.nco_state(1) == dict(enable=False, inc=0, acc=0, ts_ref=0, hz=0.0)


# ---- the loop on the CPU models, with the GPU test's stream and seed ------------------------------------------------------------

def receive(x, sent):
    """ms_rx_model over the stream's SCH slots and ACTIVE traffic slots: ([(fn, record)] of SCH slots, [(wrong bits)] per traffic slot)"""
    sch, wrong = [], []
    for k in range(len(x) // NM.SLOT):
        fn, tn = NM.LOOP_FN0 + k // 8, k % 8
        active = bool((NM.LOOP_ACTIVE >> tn) & 1)
        kind = RX.slot_kind(fn, tn, NM.LOOP_TSC)
        if kind == RX.KIND_SCH:
            sch.append((fn, RX.ms_rx(x[k * 625:(k + 1) * 625], fn, tn, NM.LOOP_TSC, active, FULL)))
        elif kind == RX.KIND_NB and active:
            r = RX.ms_rx(x[k * 625:(k + 1) * 625], fn, tn, NM.LOOP_TSC, active, FULL)
            wrong.append(int((r["bits"] != K.hard(sent[(fn, tn)])).sum()))
    return sch, wrong


def test_loop_on_the_models():
    x, sent = NM.loop_stream()
    assert len(x) == 24 * 625 and len(sent) >= 6
    sch, wrong = receive(x, sent)
    assert len(sch) == 1 and all(r["sch_rc"] == 0 for _, r in sch)                 # uncorrected: nothing is received
    assert len(wrong) == len(sent) and all(w > 0 for w in wrong)
    m = AM.fcch_offset(AM.scaled(x[:625], FULL))
    hz = NM.hz_from_fcch(m["hz"])
    assert hz == trxhip.nco_hz_from_fcch(m["hz"]) and abs(hz + NM.LOOP_CFO) <= 100.0
    y = NM.rotate(trxhip.ms_nco_tables_host(), x, 0, NM.inc_of(hz))
    sch, wrong = receive(y, sent)
    assert [(r["sch_rc"], r["sch_fn"], r["sch_bsic"]) for _, r in sch] == [(1, fn, NM.LOOP_BSIC) for fn, _ in sch]
    assert wrong == [0] * len(sent)                                # zero failures is the cap


# ---- exports, header, ABI -----------------------------------------------------------------------------------------------------------

def test_symbols_header_and_abi():
    L = trxhip.load_library()
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    names = ["trxhip_ms_nco_tables_host", "trxhip_ms_nco_inc", "trxhip_ms_nco_phase", "trxhip_ms_nco_batch_i16", "trxhip_ms_nco_batch_cf32"] + \
        ["trxhip_ms_nco_%s_%s" % (o, f) for o in ("sched", "group") for f in ("set", "state")]
    for name in names:
        assert hasattr(L, name) and name in trxhip.SYMBOLS and name + "(" in hdr, name
    assert L.trxhip_abi_version() == 5 and re.search(r"^#define\s+TRXHIP_ABI_VERSION\s+5\b", hdr, re.M)
    assert re.search(r"#define TRXHIP_MS_FCCH_BIAS_HZ \(25\.0 / 3\.0\)", hdr) and trxhip.MS_FCCH_BIAS_HZ == 25.0 / 3.0
    assert trxhip.nco_hz_from_fcch(2008.0) == -(2008.0 - 25.0 / 3.0)
    for cls in (trxhip.MsRxScheduler, trxhip.MsRxSchedulerGroup):
        assert hasattr(cls, "set_nco") and hasattr(cls, "nco_state")
    assert hasattr(trxhip.TrxHip, "ms_nco")
    from test_ms_afc_cpu import struct_fields
    assert struct_fields(hdr, "trxhip_ms_nco_status") == list(trxhip.MS_NCO_STATE_DTYPE.names)
    assert struct_fields(hdr, "trxhip_ms_nco_row") == list(trxhip.MS_NCO_ROW_DTYPE.names)
    assert struct_fields(hdr, "trxhip_ms_nco_cfg") == [f[0] for f in trxhip._MsNcoCfg._fields_]
    assert trxhip.MS_NCO_STATE_DTYPE.itemsize == 32 and C.sizeof(trxhip._MsNcoCfg) == 16
    assert [trxhip.MS_NCO_STATE_DTYPE.fields[k][1] for k in ("enable", "inc", "acc", "ts_ref", "hz")] == [0, 4, 8, 16, 24]
    # the scheduler's records keep their sizes: the NCO rides beside them
    k = open(os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_ms_rx.hip")).read()
    assert 'static_assert(sizeof(trx_mss_member) == 64, "table entry");' in k
