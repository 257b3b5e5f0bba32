"""The uplink burst scheduler's Viterbi-equaliser option (cfg->use_va, TRXHIP_FLAG_USE_VA) without a GPU: what create accepts and
refuses, and that a plan-only object with the flag cuts and plans exactly as one without it.  tests/test_gpu_rx_sched_va.py runs
the flow on the device."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rx_sched_model as M  # noqa: E402
from osmo_trx_amd import trxhip  # noqa: E402

EINVAL = -22
USE_VA, EXACT_DEMOD = 8, 2


def _cfg(**kw):
    d = dict(chans=1, sps=4, tsc=0, ul_fn_offset=0, ext_rach=0, egprs=0, flags=USE_VA, threshold=4.0, full_scale=32767.0, reserved=0,
             max_slots=8)
    d.update(kw)
    return trxhip._RxSchedCfg(*[d[k] for k, _ in trxhip._RxSchedCfg._fields_])


def test_header_value():
    import oracle_lib as O
    assert O.header_constant("TRXHIP_FLAG_USE_VA") == USE_VA == trxhip.FLAG_USE_VA
    assert trxhip.load_library().trxhip_abi_version() == 5


def test_flag_accepted_by_a_plan_only_object():
    L = trxhip.load_library()
    for create in (L.trxhip_rx_sched_create, L.trxhip_rx_sched_create_sps):
        h = C.c_void_p()
        assert create(None, C.byref(_cfg(ext_rach=1, chans=3)), C.byref(h)) == 0
        assert h.value
        L.trxhip_rx_sched_destroy(h)
    s = trxhip.RxScheduler(None, chans=2, use_va=True)
    s.set_clock(0, 0)
    assert s.pull(n_samples=626) == (1, 1)
    s.close()


def test_refused_configurations():
    L = trxhip.load_library()
    h = C.c_void_p()
    assert L.trxhip_rx_sched_create_sps(None, C.byref(_cfg(sps=1)), C.byref(h)) == EINVAL and h.value is None
    for create in (L.trxhip_rx_sched_create, L.trxhip_rx_sched_create_sps):
        for bad in (dict(egprs=1), dict(flags=USE_VA | EXACT_DEMOD), dict(flags=USE_VA | 1), dict(flags=USE_VA | 4), dict(flags=USE_VA | 16)):
            assert create(None, C.byref(_cfg(**bad)), C.byref(h)) == EINVAL, bad
            assert h.value is None
    # the same configurations without the flag are what they were
    assert L.trxhip_rx_sched_create_sps(None, C.byref(_cfg(sps=1, flags=0)), C.byref(h)) == 0
    L.trxhip_rx_sched_destroy(h)
    for ok in (dict(egprs=1, flags=0), dict(flags=EXACT_DEMOD)):
        h = C.c_void_p()
        assert L.trxhip_rx_sched_create(None, C.byref(_cfg(**ok)), C.byref(h)) == 0, ok
        L.trxhip_rx_sched_destroy(h)


def test_cuts_and_plans_as_without_the_flag():
    rng = np.random.default_rng(17)
    kw = dict(chans=3, tsc=5, ul_fn_offset=-7, ext_rach=True, max_slots=64)
    a, b = trxhip.RxScheduler(None, use_va=True, **kw), trxhip.RxScheduler(None, **kw)
    m = M.Model(3, tsc=5, ul_fn_offset=-7, ext_rach=True)
    combs = ([1, 4, 5, 7, 13, M.COMB_FILL, M.COMB_NONE, M.COMB_LOOPBACK], [7, 1, 13, 5, 2, 3, 6, M.COMB_FILL], [1] * 8)
    for o in (a, b, m):
        o.set_clock(M.HYPERFRAME - 3, 6)
        o.set_max_toa(17, 50)
        o.set_handover(2, 1, True)
        for c in range(3):
            for tn in range(8):
                o.set_slot(c, tn, combs[c][tn])
    for i, n in enumerate([0, 1, 624, 625, 626, 20, 39 * 625 + 585, 40] + [int(x) for x in rng.integers(0, 12000, 60)]):
        if i == 20:
            for o in (a, b, m):
                o.set_muted(1, True)
        assert a.slots(n) == b.slots(n) == m.slots(n)
        got, ref = a.pull(n_samples=n), b.pull(n_samples=n)
        want = m.cut(n)
        assert got == ref == (len(want[0]), m.carried), (i, n)
        assert a.clock() == b.clock() == m.clock
        for c in range(3):
            pa, pb = a.plan(c), b.plan(c)
            assert pa.tobytes() == pb.tobytes()
            w = np.array(want[c], dtype=np.int64).reshape(-1, 4)
            assert np.array_equal(np.stack([pa[k] for k in ("fn", "tn", "type", "max_toa")], 1), w)
    # refused pulls are refused alike: more than max_slots, buffers handed to a plan-only object
    L = trxhip.load_library()
    ns, nc = C.c_size_t(99), C.c_size_t(99)
    buf = (C.c_int16 * 4)()
    for o in (a, b):
        before = (o.clock(), o.slots(0), o.slots(700))
        assert L.trxhip_rx_sched_pull_s16(o.h, None, 0, 66 * 625, None, 0, None, None, None, 0, C.byref(ns), C.byref(nc), None) == EINVAL
        assert L.trxhip_rx_sched_pull_s16(o.h, buf, 0, 2, None, 0, None, None, None, 0, C.byref(ns), C.byref(nc), None) == EINVAL
        assert (ns.value, nc.value) == (99, 99) and (o.clock(), o.slots(0), o.slots(700)) == before
    a.close()
    b.close()
