"""The uplink burst scheduler without a GPU: a plan-only object (trxhip_rx_sched_create with no context) against the model of
tests/rx_sched_model.py -- slot types over every combination, the FN offset across the hyperframe wrap, the slot cutter's
strict `>` and the refusals.  The device object shares this code (csrc/trx_rx_sched.h); tests/test_gpu_rx_sched.py runs it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rx_sched_model as M  # noqa: E402
from osmo_trx_amd import trxhip  # noqa: E402

EINVAL = -22
FRAMES = 2652                      # lcm(26, 51, 52, 102): every modulus expectedCorrType() reads comes round


def handover_patterns():
    rng = np.random.default_rng(11)
    return {"none": np.zeros((8, 8), bool), "ss0": np.eye(1, 8, dtype=bool).repeat(8, 0), "all": np.ones((8, 8), bool),
            "random": rng.random((8, 8)) < 0.4}


def plan_of(s, m, n_samples):
    """pull n_samples on both; returns (object's plan, model's plan) per channel"""
    n, carried = s.pull(n_samples=n_samples)
    want = m.cut(n_samples)
    assert n == len(want[0]) and carried == m.carried
    got = [s.plan(c) for c in range(m.chans)]
    return got, want


def assert_plan(got, want):
    w = np.array(want, dtype=np.int64).reshape(-1, 4)
    assert np.array_equal(got["fn"], w[:, 0]) and np.array_equal(got["tn"], w[:, 1])
    assert np.array_equal(got["type"], w[:, 2]), np.flatnonzero(got["type"] != w[:, 2])[:10]
    assert np.array_equal(got["max_toa"], w[:, 3])


@pytest.mark.parametrize("ext_rach", [0, 1])
@pytest.mark.parametrize("egprs", [0, 1])
@pytest.mark.parametrize("pattern", ["none", "ss0", "all", "random"])
def test_types_match_model(ext_rach, egprs, pattern):
    """every combination 0 .. 15 (two objects of 8 channels: channel c has combination 8 * half + c on every TN) over 2652 frames"""
    ho = handover_patterns()[pattern]
    for half in range(2):
        s = trxhip.RxScheduler(None, chans=8, ext_rach=ext_rach, egprs=egprs, max_slots=FRAMES * 8)
        m = M.Model(8, ext_rach=bool(ext_rach), egprs=bool(egprs))
        for o in (s, m):
            o.set_clock(1000, 0)
            o.set_max_toa(21, 47)
            for c in range(8):
                for tn in range(8):
                    o.set_slot(c, tn, 8 * half + c)
            for tn in range(8):
                for ss in range(8):
                    o.set_handover(tn, ss, bool(ho[tn, ss]))
        got, want = plan_of(s, m, FRAMES * 8 * 625 + 1)
        assert len(want[0]) == FRAMES * 8
        for c in range(8):
            assert_plan(got[c], want[c])
        s.close()


@pytest.mark.parametrize("offset", [-3, 0, 5])
def test_fn_offset_and_hyperframe_wrap(offset):
    s = trxhip.RxScheduler(None, chans=1, ul_fn_offset=offset, max_slots=64)
    m = M.Model(1, ul_fn_offset=offset)
    for o in (s, m):
        o.set_clock(2715646, 0)
        for tn in range(8):
            o.set_slot(0, tn, 7)
    got, want = plan_of(s, m, 40 * 625 + 1)
    assert len(want[0]) == 40
    assert_plan(got[0], want[0])
    assert got[0]["fn"][0] == (2715646 + offset) % M.HYPERFRAME and got[0]["fn"][16] == (0 + offset) % M.HYPERFRAME
    assert s.clock() == m.clock == (2715646 + 5 - M.HYPERFRAME, 0)       # the receive clock itself carries no offset


def test_slot_cutting_matches_model():
    rng = np.random.default_rng(3)
    s = trxhip.RxScheduler(None, chans=2, max_slots=16)
    m = M.Model(2)
    s.set_clock(7, 5)
    m.set_clock(7, 5)
    for n in [0, 1, 624, 625, 626, 1250] + [int(x) for x in rng.integers(0, 4001, 200)]:
        assert s.slots(n) == m.slots(n), n
        cut, carried = s.pull(n_samples=n)
        want = m.cut(n)
        assert (cut, carried) == (len(want[0]), m.carried), n
        assert 0 <= carried <= 625
        assert s.clock() == m.clock
        assert s.slots(0) == 0 and s.slots(626 - carried) == 1 and s.slots(625 - carried) == 0      # the strict `>`
    # exactly 625 samples stay in the remainder
    s.set_clock(0, 0)
    assert s.pull(n_samples=625) == (0, 625) and s.pull(n_samples=1) == (1, 1)


def _cfg(**kw):
    d = dict(chans=1, sps=4, tsc=0, ul_fn_offset=0, ext_rach=0, egprs=0, flags=0, threshold=4.0, full_scale=32767.0, reserved=0,
             max_slots=8)
    d.update(kw)
    return trxhip._RxSchedCfg(*[d[k] for k, _ in trxhip._RxSchedCfg._fields_])


def test_refusals_leave_state_untouched():
    L = trxhip.load_library()
    h = C.c_void_p()
    for bad in (dict(chans=0), dict(chans=9), dict(sps=1), dict(sps=2), dict(tsc=8), dict(tsc=-1), dict(ul_fn_offset=M.HYPERFRAME),
                dict(flags=1), dict(full_scale=0.0), dict(max_slots=0), dict(max_slots=(1 << 20) + 1)):
        cfg = _cfg(**bad)
        assert L.trxhip_rx_sched_create(None, C.byref(cfg), C.byref(h)) == EINVAL, bad
        assert h.value is None
    assert L.trxhip_rx_sched_create(None, None, C.byref(h)) == EINVAL
    assert L.trxhip_rx_sched_create(None, C.byref(_cfg()), None) == EINVAL

    s = trxhip.RxScheduler(None, chans=2, max_slots=8)
    ns, nc = C.c_size_t(99), C.c_size_t(99)
    pull = lambda n, buf=None: L.trxhip_rx_sched_pull_s16(s.h, buf, 0, n, None, 0, None, None, None, 0, C.byref(ns), C.byref(nc), None)  # noqa: E731
    assert pull(1000) == EINVAL                                           # before set_clock
    fn, tn = C.c_uint32(), C.c_int()
    assert L.trxhip_rx_sched_clock(s.h, C.byref(fn), C.byref(tn)) == EINVAL
    assert L.trxhip_rx_sched_set_clock(s.h, M.HYPERFRAME, 0) == EINVAL
    assert L.trxhip_rx_sched_set_clock(s.h, 0, 8) == EINVAL
    s.set_clock(100, 6)
    s.set_slot(1, 6, 13)
    s.set_handover(3, 2, True)
    assert s.pull(n_samples=700) == (1, 75)
    before = (s.clock(), s.slots(0), s.slots(551), s.plan(1).tobytes())
    for rc in (L.trxhip_rx_sched_set_slot(s.h, 2, 0, 1), L.trxhip_rx_sched_set_slot(s.h, -1, 0, 1), L.trxhip_rx_sched_set_slot(s.h, 0, 8, 1),
               L.trxhip_rx_sched_set_slot(s.h, 0, 0, 16), L.trxhip_rx_sched_set_slot(s.h, 0, 0, -1),
               L.trxhip_rx_sched_set_handover(s.h, 8, 0, 1), L.trxhip_rx_sched_set_handover(s.h, 0, 8, 1),
               L.trxhip_rx_sched_set_handover(s.h, -1, 0, 1), L.trxhip_rx_sched_set_muted(s.h, 2, 1),
               L.trxhip_rx_sched_set_trxd_version(s.h, 0, 2), L.trxhip_rx_sched_set_trxd_version(s.h, 2, 1),
               L.trxhip_rx_sched_set_rssi_offset(s.h, 2, 1.0), L.trxhip_rx_sched_set_rssi_offset(s.h, 0, float("nan")),
               L.trxhip_rx_sched_set_max_toa(s.h, -1, 63), L.trxhip_rx_sched_set_max_toa(s.h, 30, 65536),
               pull(9 * 625),                                            # 9 slots > max_slots
               pull(10, (C.c_int16 * 20)()),                              # a plan-only object takes no buffers
               L.trxhip_rx_sched_plan(s.h, 0, None, 1), L.trxhip_rx_sched_plan(s.h, 2, None, 0),
               L.trxhip_rx_sched_counters(s.h, 2, (C.c_uint64 * 3)()), L.trxhip_rx_sched_counters(s.h, 0, None),
               L.trxhip_rx_sched_slots(None, 1), L.trxhip_rx_sched_noise_state(s.h, 0, None, None, None)):
        assert rc == EINVAL
    a = np.zeros(2, dtype=trxhip.RX_PLAN_DTYPE)
    assert L.trxhip_rx_sched_plan(s.h, 0, a.ctypes.data_as(C.c_void_p), 2) == EINVAL       # more than the last pull cut
    assert (ns.value, nc.value) == (99, 99)
    assert (s.clock(), s.slots(0), s.slots(551), s.plan(1).tobytes()) == before
    # ... and the settings: the next slots are planned as the model plans them without any of the refused changes
    m = M.Model(2)
    m.set_clock(100, 7)
    m.carried = 75
    m.set_slot(1, 6, 13)
    m.set_handover(3, 2, True)
    got, want = plan_of(s, m, 8 * 625)
    for c in range(2):
        assert_plan(got[c], want[c])
    assert s.counters(0) == dict(rx_empty_burst=0, rx_clipping=0, rx_no_burst_detected=0)
    ring, itr, lev = s.noise_state(1)
    assert not ring.any() and itr == 0 and lev == 0
    L.trxhip_rx_sched_destroy(None)
