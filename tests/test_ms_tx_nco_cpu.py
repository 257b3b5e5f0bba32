"""CPU tests of the MS-side uplink oscillator (trxhip_ms_nco_tx_*, MsTxScheduler.set_nco / MsTxSchedulerGroup.set_nco): the
bookkeeping of plan-only objects against the model (tests/ms_tx_nco_model.py), the uplink itself left exactly as it was, every
refusal, the bound that keeps the int16 cast defined, and -- on the compiled reference -- what the oscillator is for: an uplink
2 kHz off is detected and decoded as garbage, the same bursts rotated back decode clean.  No GPU is opened."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ms_nco_model as NM
import ms_tx_model as M
import ms_tx_nco_model as T
import osmo_trx_amd
from osmo_trx_amd import trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FS, DELAY = 2047, -60
BITS = (np.arange(148) * 7 % 3 == 0).astype(np.uint8)
OFF = dict(enable=False, inc=0, acc=0, ts_ref=0, hz=0.0)


def reqs_of(triples):
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    return trxhip.ms_tx_requests(t[:, 0], t[:, 1], t[:, 2], np.tile(BITS, (len(t), 1)))


# ---- exports, header, ABI, record sizes ------------------------------------------------------------------------------------------

def test_symbols_header_abi_and_sizes():
    L = trxhip.load_library()
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    for name in ("trxhip_ms_nco_tx_set", "trxhip_ms_nco_tx_state", "trxhip_ms_nco_tx_group_set", "trxhip_ms_nco_tx_group_state"):
        assert hasattr(L, name) and name in trxhip.SYMBOLS and name + "(" in hdr, name
    assert L.trxhip_abi_version() == 5 and re.search(r"^#define\s+TRXHIP_ABI_VERSION\s+5\b", hdr, re.M)
    for cls in (trxhip.MsTxScheduler, trxhip.MsTxSchedulerGroup):
        assert hasattr(cls, "set_nco") and hasattr(cls, "nco_state")
    assert osmo_trx_amd.nco_tx_hz is trxhip.nco_tx_hz and "nco_tx_hz" in osmo_trx_amd.__all__
    # the records the render hands its kernels keep their sizes, and so does the public state record
    k = open(os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_ms_tx.h")).read()
    assert 'static_assert(sizeof(trx_mstx_gmember) == 32, "trx_mstx_gmember layout");' in k
    assert 'static_assert(sizeof(trx_mstx_seg) == 16, "trx_mstx_seg layout");' in k
    assert "typedef struct trxhip_ms_tx_status {  /* 96 bytes */" in hdr and trxhip.MS_TX_STATE_DTYPE.itemsize == 96
    from test_ms_afc_cpu import struct_fields
    assert struct_fields(hdr, "trxhip_ms_tx_status") == list(trxhip.MS_TX_STATE_DTYPE.names)
    buf = np.full(96 + 32, 0xA5, dtype=np.uint8)
    s = trxhip.MsTxScheduler(None)
    s.set_nco(True, 1234.5)
    assert L.trxhip_ms_tx_state(s.h, buf.ctypes.data_as(C.c_void_p)) == 0
    assert (buf[96:] == 0xA5).all()                                 # state() writes 96 bytes with an oscillator on, too
    buf[:] = 0xA5
    assert L.trxhip_ms_nco_tx_state(s.h, buf.ctypes.data_as(C.c_void_p)) == 0
    assert (buf[32:] == 0xA5).all() and trxhip.MS_NCO_STATE_DTYPE.itemsize == 32


def test_nco_tx_hz():
    assert trxhip.nco_tx_hz(-2008.5) == 2008.5 and trxhip.nco_tx_hz(0.0) == 0.0
    dl, ul = 947.4e6, 902.4e6
    assert trxhip.nco_tx_hz(-2000.0, dl, ul) == 2000.0 * (ul / dl)
    assert abs(trxhip.nco_tx_hz(-2000.0, dl, ul) - 1905.0) < 0.01   # 45 MHz below a 947.4 MHz downlink
    with pytest.raises(ValueError):
        trxhip.nco_tx_hz(1.0, dl_hz=dl)


# ---- bookkeeping against the model ----------------------------------------------------------------------------------------------------

# per step: ("set", enable, hz) or ("render", gap in front of the window, n_samples) or ("submit",) or ("ta", val)
STEPS = [("set", True, 2000.0), ("set", True, -270000.0), ("submit",), ("render", 0, 700), ("set", True, 1999.5), ("render", 13, 1),
         ("ta", 7), ("render", 0, 4999), ("set", False, 0.0), ("render", 100000, 625), ("set", False, 77.0), ("set", True, -500000.0),
         ("submit",), ("render", 0, 3), ("set", True, 500000.0), ("render", (1 << 33) + 5, 312), ("set", True, 0.0), ("render", 0, 50),
         ("set", True, 33.25)]


@pytest.mark.parametrize("first_ts", [0, -5000, -(1 << 40) - 3, (1 << 32) - 400, (1 << 40) - 1000, -300])
def test_single_bookkeeping_equals_the_model(first_ts):
    """set, render, change, disable and enable against the model; ts_ref is 0 before the first window, rendered_end after it, and
    the windows leave gaps; next to it an object that never has an oscillator gets the same calls: plans, counters, state()"""
    s, plain = (trxhip.MsTxScheduler(None, tx_full_scale=FS, rxtx_delay=DELAY, max_pending=64) for _ in range(2))
    model = T.MsTxNco(FS, DELAY, 64)
    assert s.nco_state() == OFF == model.nco_state()
    at, fn = first_ts, 100
    for step in STEPS:
        if step[0] == "set":
            s.set_nco(step[1], step[2])
            model.set_nco(step[1], step[2])
            if model.rendered_end is None:
                assert s.nco_state()["ts_ref"] == 0
            else:
                assert s.nco_state()["ts_ref"] == model.rendered_end == at
        elif step[0] == "ta":
            for o in (s, plain, model):
                o.set_ta(step[1])
        elif step[0] == "submit":
            clock = (fn, 0, at + 100)
            tr = [(fn + k // 3, 2 * (k % 3), 3 * k) for k in range(6)]
            fn += 10
            a, b, c = s.submit(reqs_of(tr), clock), plain.submit(reqs_of(tr), clock), model.submit(tr, clock)
            assert a.tobytes() == b.tobytes() and [int(x) for x in a["status"]] == [p["status"] for p in c]
        else:
            at += step[1]
            nd_a, nd_b, nd_c = s.render(step[2], at)[1], plain.render(step[2], at)[1], model.render(step[2], at)[0]
            assert nd_a == nd_b == nd_c
            at += step[2]
        assert s.nco_state() == model.nco_state(), step
        assert s.state().tobytes() == plain.state().tobytes()
        for k, v in model.state().items():
            assert int(s.state()[k]) == v, (k, step)
        assert plain.nco_state() == OFF
    assert s.state()["drawn"] + s.state()["missed"] > 0
    # the phase the next window would start with is the library's own phase of the state
    st = s.nco_state()
    assert trxhip.ms_nco_phase(st["acc"], st["ts_ref"], st["inc"], at + 12345) == NM.phase(st["acc"], st["ts_ref"], st["inc"], at + 12345)


def test_group_of_three_equals_singles_equals_the_model():
    """members with their own windows (first_ts around 0, 2^32 and below -2^40), set at different times; member 1 is rendered in
    some rounds only; the group without any oscillator moves in step"""
    g, plain = (trxhip.MsTxSchedulerGroup(None, n_members=3, tx_full_scale=FS, rxtx_delay=DELAY, max_pending=32) for _ in range(2))
    single = [trxhip.MsTxScheduler(None, tx_full_scale=FS, rxtx_delay=DELAY, max_pending=32) for _ in range(3)]
    model = [T.MsTxNco(FS, DELAY, 32) for _ in range(3)]
    at = [-777, (1 << 32) - 2000, -(1 << 40) - 11]
    settings = [(0, True, 2000.0), (2, True, -270000.0), (1, True, 0.0), (0, True, -1500.25), (2, False, 0.0), (1, False, 5.0),
                (2, True, 499999.0), (0, False, 0.0), (0, True, 10.0)]
    for rnd, (m, en, hz) in enumerate(settings):
        g.set_nco(m, en, hz)
        single[m].set_nco(en, hz)
        model[m].set_nco(en, hz)
        if rnd == 0:
            assert g.nco_state(0)["ts_ref"] == 0 and g.nco_state(0)["acc"] == 0
        if rnd % 3 == 0:
            clocks = [(50 + 10 * rnd, 1, at[k] + 200) for k in range(3)]
            tr = [(50 + 10 * rnd + 1 + k, (3 * k) % 8, 0) for k in range(4)]
            members = [0, 2, 1, 0]
            pa, pb = g.submit(members, reqs_of(tr), clocks), plain.submit(members, reqs_of(tr), clocks)
            assert pa.tobytes() == pb.tobytes()
            for k in range(3):
                mine = [t for t, mm in zip(tr, members) if mm == k]
                single[k].submit(reqs_of(mine), clocks[k])
                model[k].submit(mine, clocks[k])
        sizes = [700 + 625 * rnd, 0 if rnd % 2 else 313, 5000]
        gaps = [0, 17 * rnd, 1 << 20 if rnd == 4 else 0]
        first = [at[k] + gaps[k] for k in range(3)]
        nd_a, nd_b = g.render(sizes, first)[1], plain.render(sizes, first)[1]
        assert nd_a == nd_b
        for k in range(3):
            if sizes[k]:
                assert single[k].render(sizes[k], first[k])[1] == nd_a[k] == model[k].render(sizes[k], first[k])[0]
                at[k] = first[k] + sizes[k]
        for k in range(3):
            assert g.nco_state(k) == single[k].nco_state() == model[k].nco_state(), (rnd, k)
            assert g.state(k).tobytes() == plain.state(k).tobytes() == single[k].state().tobytes(), (rnd, k)
            assert plain.nco_state(k) == OFF
    assert sum(int(g.state(k)["drawn"]) for k in range(3)) > 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_both_states_untouched():
    L = trxhip.load_library()
    s = trxhip.MsTxScheduler(None, tx_full_scale=FS, rxtx_delay=DELAY, max_pending=8)
    g = trxhip.MsTxSchedulerGroup(None, n_members=3, tx_full_scale=FS, rxtx_delay=DELAY, max_pending=8)
    s.submit(reqs_of([(11, 2, 0)]), (10, 0, 1000))
    s.render(100, 900)
    s.set_nco(True, -1234.0)
    g.render([10, 0, 20], [5, 0, -7])
    g.set_nco(2, True, 99.0)
    before = (s.state().tobytes(), s.nco_state(), [g.state(m).tobytes() for m in range(3)], [g.nco_state(m) for m in range(3)])
    out = np.zeros(1, dtype=trxhip.MS_NCO_STATE_DTYPE)
    po = out.ctypes.data_as(C.c_void_p)
    for hz in (500000.1, -500000.1, 1e300, float("nan"), float("inf")):
        for en in (0, 1):
            cfg = trxhip._MsNcoCfg(en, 0, hz)
            assert L.trxhip_ms_nco_tx_set(s.h, C.byref(cfg)) == EINVAL
            assert L.trxhip_ms_nco_tx_group_set(g.h, 2, C.byref(cfg)) == EINVAL
        with pytest.raises(trxhip.TrxHipError):
            s.set_nco(True, hz)
        with pytest.raises(trxhip.TrxHipError):
            g.set_nco(0, True, hz)
    ok = trxhip._MsNcoCfg(1, 0, 100.0)
    assert L.trxhip_ms_nco_tx_set(None, C.byref(ok)) == EINVAL and L.trxhip_ms_nco_tx_set(s.h, None) == EINVAL
    assert L.trxhip_ms_nco_tx_state(None, po) == EINVAL and L.trxhip_ms_nco_tx_state(s.h, None) == EINVAL
    assert L.trxhip_ms_nco_tx_group_set(None, 0, C.byref(ok)) == EINVAL and L.trxhip_ms_nco_tx_group_set(g.h, 0, None) == EINVAL
    assert L.trxhip_ms_nco_tx_group_set(g.h, 3, C.byref(ok)) == EINVAL and L.trxhip_ms_nco_tx_group_set(g.h, 0xFFFFFFFF, C.byref(ok)) == EINVAL
    assert L.trxhip_ms_nco_tx_group_state(None, 0, po) == EINVAL and L.trxhip_ms_nco_tx_group_state(g.h, 0, None) == EINVAL
    assert L.trxhip_ms_nco_tx_group_state(g.h, 3, po) == EINVAL
    assert not out.view(np.uint8).any()
    # a refused render moves nothing of the oscillator either
    with pytest.raises(trxhip.TrxHipError):
        s.render(10, 0)                                             # the window goes backwards
    with pytest.raises(trxhip.TrxHipError):
        g.render([10, 0, 20], [0, 0, 1000])                         # member 0's does
    after = (s.state().tobytes(), s.nco_state(), [g.state(m).tobytes() for m in range(3)], [g.nco_state(m) for m in range(3)])
    assert after == before
    # the limits themselves pass
    s.set_nco(True, 500000.0)
    g.set_nco(1, True, -500000.0)
    assert s.nco_state()["inc"] == NM.inc_of(500000.0) and g.nco_state(1)["inc"] == NM.inc_of(-500000.0)


# ---- the cast stays defined -----------------------------------------------------------------------------------------------------------

def test_the_cast_bound_behind_the_oscillator():
    """include/trxhip.h's argument with the generated tables: |x| <= scale * (per-phase sum of |taps|) * max|symbol|, the
    modulator's roundings below 2^-20, the oscillator's (table entries, the phasor's three, the rotation's three) below 2^-20
    again, and the product stays below 32768 at the largest tx_full_scale create accepts -- so set_nco is accepted there"""
    from test_tx_cpu import TX_TABLES
    t = np.frombuffer(trxhip.generate_tx_tables_host(), dtype=TX_TABLES)[0]
    c0, c1 = t["pulse4_c0"].astype(np.float64), t["pulse4_c1"].astype(np.float64)
    taps = max(np.abs(c0[p::4]).sum() + np.abs(c1[p::4]).sum() for p in range(4))
    assert abs(taps - 1.52568) < 1e-5
    sym = np.abs(t["rot4"][0:4 * 150:4].astype(np.complex128)).max()   # c0 symbols are +-rot4[4m], c1 symbols those times (0, +-1)
    assert abs(sym - 1.0) < 2.0 ** -23
    u = 2.0 ** -24
    C_, F_ = (x.astype(np.float64) for x in trxhip.ms_nco_tables_host())
    assert np.hypot(C_[:, 0], C_[:, 1]).max() <= 1 + u and np.hypot(F_[:, 0], F_[:, 1]).max() <= 1 + u
    r = (1 + u) ** 2 * (1 + 3 * np.sqrt(2) * u)                     # |r|: the entries' moduli, the phasor's three roundings
    assert r < 1 + 6.3 * u and r * (1 + 3 * u) < 1 + 2.0 ** -20      # and the rotation's three
    bound = taps * sym * (1 + 2.0 ** -20) * (1 + 2.0 ** -20)
    assert 21477 * bound < 32768.0 <= 21478 * taps
    for make in (lambda: trxhip.MsTxScheduler(None, tx_full_scale=21477), lambda: trxhip.MsTxSchedulerGroup(None, 2, tx_full_scale=21477)):
        o = make()
        o.set_nco(*((True, 2000.0) if isinstance(o, trxhip.MsTxScheduler) else (1, True, 2000.0)))
        o.close()
    # the model at full scale, every phase of the oscillator's coarse table against the worst sample it could meet
    tabs = trxhip.ms_nco_tables_host()
    worst = np.full(1024, np.complex64(complex(np.float32(21477 * taps * (1 + 2.0 ** -20)), 0.0)))
    for turn in (1, 1j, -1, -1j, np.exp(0.25j * np.pi)):
        y = NM.rotate(tabs, (worst * turn).astype(np.complex64), 0, 1 << 22)
        assert np.abs(T.cast(y).astype(np.int32)).max() <= 32767


# ---- what it is for: the uplink on the compiled reference -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def uplink():
    import oracle_lib as O
    O.lib().orc_setup()
    return T.ul_bursts()


def test_uplink_off_frequency_is_detected_and_decoded_as_garbage(uplink):
    bits, x, start = uplink
    for hz in (0.0, 500.0):
        found, wrong = T.ul_wrong_bits(x, bits, start, hz)
        print(f"uplink at {hz:+.0f} Hz: {found} of {len(x)} detected, {wrong:.4f} of the hard bits wrong")
        assert found == len(x) and wrong == 0.0
    for hz in (2000.0, -2000.0):
        found, wrong = T.ul_wrong_bits(x, bits, start, hz)
        print(f"uplink at {hz:+.0f} Hz: {found} of {len(x)} detected, {wrong:.4f} of the hard bits wrong")
        assert found == len(x) and wrong > 0.25


@pytest.mark.parametrize("hz", [2000.0, -2000.0])
def test_uplink_rotated_back_decodes_clean(uplink, hz):
    """the model's rotation by the opposite frequency in front of the radio's error: no wrong bit, what the oracle gives on
    frequency"""
    bits, x, start = uplink
    tabs = trxhip.ms_nco_tables_host()
    inc = NM.inc_of(-hz)
    y = np.stack([NM.rotate(tabs, x[i], (i * 0x9E3779B1) & NM.M32, inc) for i in range(len(x))])
    found, wrong = T.ul_wrong_bits(y, bits, start, hz)
    print(f"uplink at {hz:+.0f} Hz behind the oscillator at {-hz:+.0f} Hz: {found} detected, {wrong:.4f} wrong")
    assert found == len(x) and wrong == 0.0
