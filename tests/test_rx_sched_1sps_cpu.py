"""The uplink burst scheduler at one sample per symbol without a GPU: a plan-only object from trxhip_rx_sched_create_sps()
against tests/rx_sched_model_1sps.py, whose cutter is the literal loop of RadioInterface::driveReceiveRadio() for mSPSRx == 1
(radioInterface.cpp:252-291).  The device object shares this code (csrc/trx_rx_sched.h); tests/test_gpu_rx_sched_1sps.py runs it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rx_sched_model_1sps as M1  # noqa: E402
from osmo_trx_amd import trxhip  # noqa: E402

EINVAL = -22
FRAMES = 2652                      # lcm(26, 51, 52, 102): every modulus expectedCorrType() reads comes round


def pair(tn0, chans=1, max_slots=8192, **kw):
    s = trxhip.RxScheduler(None, chans=chans, sps=1, max_slots=max_slots, **kw)
    m = M1.Model(chans, ext_rach=bool(kw.get("ext_rach", False)))
    for o in (s, m):
        o.set_clock(77, tn0)
    return s, m


def pull_both(s, m, n):
    """one pull on the object and on the model: slots() before it, slots cut, samples carried and the clock"""
    assert s.slots(n) == m.slots(n), (n, m.clock, m.carried)
    cut, carried = s.pull(n_samples=n)
    want = m.cut(n)
    assert (cut, carried) == (len(want[0]), m.carried), (n, m.clock)
    assert 0 <= carried <= 157
    assert s.clock() == m.clock
    return cut


@pytest.mark.parametrize("tn0", range(8))
def test_cutter_matches_the_reference_loop(tn0):
    """chunk sizes 0 .. 3000 in order and shuffled (the carried count and the TN phase they meet differ), then at random up to
    10^6; after every pull the strict `>` against the size of the slot that would be cut next"""
    rng = np.random.default_rng(100 + tn0)
    s, m = pair(tn0)
    sizes = list(range(3001)) + [int(x) for x in rng.permutation(3001)] + [int(x) for x in rng.integers(0, 10**6 + 1, 40)]
    seen = set()
    for n in sizes:
        pull_both(s, m, n)
        size = M1.burst_size(m.clock[1])                                  # the slot that would be cut next
        assert m.carried <= size
        assert s.slots(0) == 0 and s.slots(size - m.carried) == 0 and s.slots(size + 1 - m.carried) == 1
        seen.add((size, m.carried == size))
    # both sizes were met, each with a full slot waiting in the remainder: 156 stay in front of 156, 157 in front of 157
    assert seen == {(156, False), (156, True), (157, False), (157, True)}


@pytest.mark.parametrize("tn0", range(8))
def test_strict_greater_at_both_sizes(tn0):
    """exactly one slot's worth stays in the remainder, whichever size the next slot has; one more sample cuts it"""
    s, m = pair(tn0)
    for _ in range(9):
        size = M1.burst_size(m.clock[1])
        assert size == (157 if m.clock[1] % 4 == 0 else 156)
        assert pull_both(s, m, size - m.carried) == 0 and m.carried == size
        assert pull_both(s, m, 1) == 1 and m.carried == 1
    # eight consecutive slots are 1250 samples
    s, m = pair(tn0)
    assert pull_both(s, m, 1250) == 7 and pull_both(s, m, 1) == 1 and m.carried == 1 and m.clock == (78, tn0)


def test_plan_matches_model_over_2652_frames():
    """every combination 0 .. 15 (two objects of 8 channels: channel c has combination 8 * half + c on every TN), a random handover
    table and EXT_RACH, over 2652 frames of 157 / 156 / 156 / 156 slots"""
    ho = np.random.default_rng(11).random((8, 8)) < 0.4
    for half in range(2):
        s, m = pair(0, chans=8, max_slots=FRAMES * 8, ext_rach=True)
        for o in (s, m):
            o.set_clock(1000, 0)
            o.set_max_toa(21, 47)
            for c in range(8):
                for tn in range(8):
                    o.set_slot(c, tn, 8 * half + c)
            for tn in range(8):
                for ss in range(8):
                    o.set_handover(tn, ss, bool(ho[tn, ss]))
        n, carried = s.pull(n_samples=FRAMES * 1250 + 1)
        want = m.cut(FRAMES * 1250 + 1)
        assert n == len(want[0]) == FRAMES * 8 and carried == m.carried == 1
        for c in range(8):
            got = s.plan(c)
            w = np.array(want[c], dtype=np.int64).reshape(-1, 4)
            for i, k in enumerate(("fn", "tn", "type", "max_toa")):
                assert np.array_equal(got[k], w[:, i]), (half, c, k)
        s.close()


def _cfg(**kw):
    d = dict(chans=1, sps=1, tsc=0, ul_fn_offset=0, ext_rach=0, egprs=0, flags=0, threshold=4.0, full_scale=32767.0, reserved=0,
             max_slots=8)
    d.update(kw)
    return trxhip._RxSchedCfg(*[d[k] for k, _ in trxhip._RxSchedCfg._fields_])


def test_refusals():
    L = trxhip.load_library()
    h = C.c_void_p()
    for bad in (dict(sps=0), dict(sps=2), dict(sps=3), dict(sps=8), dict(egprs=1), dict(chans=0), dict(tsc=8), dict(flags=1),
                dict(max_slots=0)):
        assert L.trxhip_rx_sched_create_sps(None, C.byref(_cfg(**bad)), C.byref(h)) == EINVAL, bad
        assert h.value is None
    assert L.trxhip_rx_sched_create_sps(None, None, C.byref(h)) == EINVAL
    assert L.trxhip_rx_sched_create_sps(None, C.byref(_cfg()), None) == EINVAL
    assert L.trxhip_rx_sched_create(None, C.byref(_cfg()), C.byref(h)) == EINVAL and h.value is None   # the old entry point: 4 only
    # at 4 the new entry point is the old one (EDGE included); TRXHIP_FLAG_EXACT_DEMOD is accepted at 1
    for ok in (dict(sps=4), dict(sps=4, egprs=1), dict(flags=trxhip.FLAG_EXACT_DEMOD)):
        assert L.trxhip_rx_sched_create_sps(None, C.byref(_cfg(**ok)), C.byref(h)) == 0, ok
        L.trxhip_rx_sched_destroy(h)
        h = C.c_void_p()
    s4 = trxhip.RxScheduler(None, sps=4, max_slots=8)
    s4.set_clock(0, 0)
    assert s4.pull(n_samples=625) == (0, 625) and s4.pull(n_samples=1) == (1, 1)

    # int16 and complex64 mixed over a carried remainder, and the other refused pulls: the state stays
    s, m = pair(3, max_slots=8)
    ns, nc = C.c_size_t(99), C.c_size_t(99)

    def pull(fn, n):
        return fn(s.h, None, 0, n, None, 0, None, None, None, 0, C.byref(ns), C.byref(nc), None)

    assert pull(L.trxhip_rx_sched_pull_s16, 200) == 0 and (ns.value, nc.value) == (1, 44)
    m.cut(200)
    ns.value = nc.value = 99
    before = (s.clock(), s.slots(0), s.slots(113), s.slots(114), s.plan(0).tobytes())
    assert before[:4] == (m.clock, 0, 0, 1)
    assert pull(L.trxhip_rx_sched_pull_cf32, 500) == EINVAL                 # complex64 over 44 int16 samples
    assert pull(L.trxhip_rx_sched_pull_s16, 9 * 157) == EINVAL              # 9 slots > max_slots
    assert (ns.value, nc.value) == (99, 99)
    assert (s.clock(), s.slots(0), s.slots(113), s.slots(114), s.plan(0).tobytes()) == before
    assert pull(L.trxhip_rx_sched_pull_cf32, 0) == 0                        # nothing to mix
    assert pull(L.trxhip_rx_sched_pull_s16, 114) == 0 and (ns.value, nc.value) == (1, 1)
    m.cut(114)
    assert s.clock() == m.clock
    s.set_clock(5, 0)                                                       # drops the remainder: either format may follow
    assert pull(L.trxhip_rx_sched_pull_cf32, 158) == 0 and (ns.value, nc.value) == (1, 1)
    assert pull(L.trxhip_rx_sched_pull_s16, 10) == EINVAL
