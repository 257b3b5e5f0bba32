"""CPU tests of the MS-side uplink burst scheduler (trxhip_ms_tx_*, MsTxScheduler): the plan-only object (ctx == NULL) against the
literal restatement of ms_trx::submit_burst(), set_ta() and driveTx()'s scale (tests/ms_tx_model.py) -- every plan record, the
two reference quirks (the unsigned-TN wrap, the integer -RSSI / 10), the queue rules the header defines, and every refusal with
the state untouched.  No GPU is opened."""
import ctypes as C

import numpy as np
import pytest

import ms_tx_model as M
from osmo_trx_amd import trxhip

EINVAL = -22
H = M.HYPERFRAME
BITS = (np.arange(148) * 7 % 3 == 0).astype(np.uint8)


def reqs_of(triples):
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    return trxhip.ms_tx_requests(t[:, 0], t[:, 1], t[:, 2], np.tile(BITS, (len(t), 1)))


class Pair:
    """a plan-only object and the model side by side"""

    def __init__(self, fs=2047, delay=0, max_pending=1024):
        self.obj = trxhip.MsTxScheduler(None, tx_full_scale=fs, rxtx_delay=delay, max_pending=max_pending)
        self.model = M.MsTx(fs, delay, max_pending)

    def set_ta(self, val):
        self.obj.set_ta(val)
        self.model.set_ta(val)

    def submit(self, triples, clock):
        plan = self.obj.submit(reqs_of(triples), clock)
        ref = self.model.submit(triples, clock)
        assert len(plan) == len(ref)
        for p, r, t in zip(plan, ref, triples):
            for k in ("status", "send_ts", "radio_ts", "diff_fn", "diff_tn"):
                assert int(p[k]) == r[k], (k, t, clock, p, r)
            assert p["scale"].tobytes() == r["scale"].tobytes(), (t, p["scale"], r["scale"])
        self.check_state()
        return plan

    def render(self, n, first_ts):
        _, nd = self.obj.render(n, first_ts)
        ref, _ = self.model.render(n, first_ts)
        assert nd == ref
        self.check_state()
        return nd

    def check_state(self):
        st, ref = self.obj.state(), self.model.state()
        for k, v in ref.items():
            assert int(st[k]) == v, (k, st, ref)


def target_for(now_fn, diff_fn, ttn):
    """the request (fn, tn) whose target after incTN(3) is (now_fn + diff_fn, ttn)"""
    t = M.Time((now_fn + diff_fn) % H, ttn).decTN(3)
    return t.fn, t.tn


@pytest.mark.parametrize("delay", [0, -60, -67])
def test_plan_equals_the_model(delay):
    """every (now_tn, target tn) pair x diff_fn in {-1, 0, 1, 2, 51 * 26}, FN wrap both ways, now_ts near 0 and near 2^40, every
    timing advance; a fresh pair per clock so that no burst overlaps another's"""
    n_status = np.zeros(6, dtype=int)
    for now_fn, now_ts in ((1000, 7), (H - 1, (1 << 40) + 311), (0, 5000), (H // 2, 1 << 40)):
        for ta in (-126, -1, 0, 1, 63, 127):
            for now_tn in range(8):
                pair = Pair(delay=delay, max_pending=64)
                pair.set_ta(ta)
                triples = []
                for dfn in (-1, 0, 1, 2, 51 * 26):
                    for ttn in range(8):
                        fn, tn = target_for(now_fn, dfn, ttn)
                        triples.append((fn, tn, 0))
                plan = pair.submit(triples, (now_fn, now_tn, now_ts))
                n_status += np.bincount(plan["status"], minlength=6)
                ok = plan[plan["status"] == M.QUEUED]
                assert (ok["radio_ts"] == ok["send_ts"] + delay).all()
    assert n_status[M.QUEUED] and n_status[M.LATE] and n_status[M.WRAPPED] and not n_status[M.OVERLAP:].any()


def test_fn_wrap_both_directions():
    pair = Pair()
    # the clock at the last frame of the hyperframe, the target in frame 0 ...
    p = pair.submit([(0, 2, 0)], (H - 1, 0, 100))
    assert p["status"][0] == M.QUEUED and p["diff_fn"][0] == 1 and p["send_ts"][0] == 100 + 5000 + 5 * 625
    # ... and the reverse: one frame back across the wrap is late
    pair = Pair()
    p = pair.submit([(H - 1, 2, 0)], (0, 0, 100))
    assert p["status"][0] == M.LATE and p["diff_fn"][0] == -1
    # incTN(3) itself carries across the wrap: (H - 1, 6) -> (0, 1)
    pair = Pair()
    p = pair.submit([(H - 1, 6, 0)], (H - 1, 7, 0))
    assert p["status"][0] == M.QUEUED and p["diff_fn"][0] == 1 and p["diff_tn"][0] == -6 and p["send_ts"][0] == 2 * 625


@pytest.mark.parametrize("k", range(1, 8))
def test_wrapped_reports_the_literal_send_ts(k):
    """diff_fn == 0 and target_tn = now_tn - k: target_tn - TN() wraps, the burst is not 'too late', tosend = Time(0, 0).decTN(k) =
    (H - 1, 8 - k), and the products of ms.cpp:139 are unsigned int.  Nothing is staged."""
    for now_tn in range(k, 8):
        pair = Pair(delay=-60)
        pair.set_ta(3)
        now_fn, now_ts = 4242, 1 << 33
        fn, tn = target_for(now_fn, 0, now_tn - k)
        p = pair.submit([(fn, tn, 0)], (now_fn, now_tn, now_ts))[0]
        literal = now_ts + ((H - 1) * 8 * 625) % (1 << 32) + (8 - k) * 625 - 12
        assert p["status"] == M.WRAPPED and p["diff_tn"] == -k and p["send_ts"] == literal and p["radio_ts"] == literal - 60
        st = pair.obj.state()
        assert st["wrapped"] == 1 and st["pending"] == 0 and st["queued"] == 0


def test_late_exactly_where_the_reference_says():
    for now_tn in range(8):
        for dfn in (-2, -1, 0, 1):
            for ttn in range(8):
                pair = Pair()
                fn, tn = target_for(5000, dfn, ttn)
                p = pair.submit([(fn, tn, 0)], (5000, now_tn, 0))[0]
                late = dfn < 0 or (dfn == 0 and 0 <= ttn - now_tn < 3)
                assert (p["status"] == M.LATE) == late, (now_tn, dfn, ttn)
                if late:
                    assert p["send_ts"] == 0 and p["radio_ts"] == 0


@pytest.mark.parametrize("fs", [2047, 9830])
def test_scale_is_the_integer_division(fs):
    pair = Pair(fs=fs)
    pwrs = (0, 9, 10, 19, 20, 99, 255)
    plan = pair.submit([(100 + 2 * i, 0, pw) for i, pw in enumerate(pwrs)], (50, 0, 0))
    for p, pw in zip(plan, pwrs):
        want = np.float32(float(fs) * 10.0 ** (-(pw // 10)))
        assert p["status"] == M.QUEUED and p["scale"].tobytes() == want.tobytes(), (pw, p["scale"], want)
    assert plan["scale"][0] == plan["scale"][1] == fs and plan["scale"][2] == plan["scale"][3]      # 9 dB is no attenuation


def test_overlap_when_ta_rises_and_not_when_it_falls():
    pair = Pair()
    pair.set_ta(10)
    clock = (200, 0, 10000)
    a = pair.submit([(300, 1, 0)], clock)[0]
    pair.set_ta(11)                      # one symbol more: the next TN's burst starts 4 samples inside the queued one
    b = pair.submit([(300, 2, 0)], clock)[0]
    assert a["status"] == M.QUEUED and b["status"] == M.OVERLAP and b["radio_ts"] == a["radio_ts"] + 621
    pair.set_ta(10)                      # falling back: exactly adjacent
    c = pair.submit([(300, 2, 0)], clock)[0]
    assert c["status"] == M.QUEUED and c["radio_ts"] == a["radio_ts"] + 625
    pair.set_ta(9)                       # falling further: a gap of 4 samples
    d = pair.submit([(300, 3, 0)], clock)[0]
    assert d["status"] == M.QUEUED and d["radio_ts"] == c["radio_ts"] + 629
    # the burst in front of a queued one overlaps as well, and the same slot twice
    pair.set_ta(8)
    e = pair.submit([(300, 0, 0), (300, 3, 0)], clock)
    assert list(e["status"]) == [M.OVERLAP, M.OVERLAP]
    st = pair.obj.state()
    assert st["overlap"] == 3 and st["pending"] == 3 and st["timing_advance"] == 32


def test_full_at_max_pending():
    pair = Pair(max_pending=3)
    plan = pair.submit([(100 + i, 0, 0) for i in range(5)], (50, 0, 0))
    assert list(plan["status"]) == [M.QUEUED] * 3 + [M.FULL] * 2
    assert pair.render(8 * 625, int(plan["radio_ts"][0])) == 1      # one retired: room for one more
    plan = pair.submit([(110, 0, 0), (111, 0, 0)], (50, 0, 0))
    assert list(plan["status"]) == [M.QUEUED, M.FULL]


def test_expired_against_the_rendered_window():
    pair = Pair(delay=-67)
    clock = (50, 0, 1000)
    plan = pair.submit([(60, 0, 0), (60, 4, 0)], clock)
    t0, t1 = (int(t) for t in plan["radio_ts"])
    # a plan-only render advances the window without drawing: the first burst ends in it, the second crosses its end
    assert pair.render(t1 + 100 - (t0 - 10), t0 - 10) == 1
    st = pair.obj.state()
    assert st["window_set"] == 1 and st["rendered_end"] == t1 + 100 and st["pending"] == 1 and st["drawn"] == 1
    plan = pair.submit([(60, 2, 0), (60, 5, 0)], clock)              # TN 2 lies inside what was rendered; TN 5 behind it
    assert list(plan["status"]) == [M.EXPIRED, M.QUEUED]
    # a gap between windows: the burst on TN 5 lies wholly in it
    t5 = int(plan["radio_ts"][1])
    assert pair.render(10, t5 + 10000) == 1                          # the straddler is retired here, as drawn
    st = pair.obj.state()
    assert st["drawn"] == 2 and st["missed"] == 1 and st["pending"] == 0 and st["expired"] == 1


def test_refusals_leave_the_state_untouched():
    L = trxhip.load_library()
    for fs, mp in ((21478, 16), (1 << 31, 16), (2047, 0), (2047, (1 << 22) + 1)):
        with pytest.raises(trxhip.TrxHipError):
            trxhip.MsTxScheduler(None, tx_full_scale=fs, max_pending=mp)
    trxhip.MsTxScheduler(None, tx_full_scale=21477, max_pending=1 << 22).close()       # the bound itself passes
    pair = Pair(max_pending=8)
    pair.set_ta(5)
    pair.submit([(100, 0, 0), (101, 0, 20)], (50, 0, 0))
    pair.render(1000, 0)
    before = pair.obj.state().tobytes()

    def refused(fn, *a):
        assert fn(pair.obj.h, *a) == EINVAL
        assert pair.obj.state().tobytes() == before

    for val in (-127, 128, 1000):
        refused(L.trxhip_ms_tx_set_ta, val)
    good = reqs_of([(102, 0, 0), (103, 0, 0)])
    plan = np.zeros(2, dtype=trxhip.MS_TX_PLAN_DTYPE)
    for bad in ((H, 0), (102, 8), (0xFFFFFFFF, 255)):
        r = good.copy()
        r["fn"][1], r["tn"][1] = bad                   # the second request is bad: the first must not be queued either
        refused(L.trxhip_ms_tx_submit, r.ctypes.data_as(C.c_void_p), 2, 50, 0, 0, plan.ctypes.data_as(C.c_void_p), None)
    refused(L.trxhip_ms_tx_submit, good.ctypes.data_as(C.c_void_p), 2, H, 0, 0, None, None)
    refused(L.trxhip_ms_tx_submit, good.ctypes.data_as(C.c_void_p), 2, 50, 8, 0, None, None)
    refused(L.trxhip_ms_tx_submit, good.ctypes.data_as(C.c_void_p), 2, 50, -1, 0, None, None)
    refused(L.trxhip_ms_tx_submit, None, 2, 50, 0, 0, None, None)
    nd = C.c_size_t()
    refused(L.trxhip_ms_tx_render_s16, None, 100, 999, C.byref(nd), None)              # the window would go backwards
    refused(L.trxhip_ms_tx_render_s16, None, (1 << 31) + 1, 1000, C.byref(nd), None)
    refused(L.trxhip_ms_tx_render_s16, C.c_void_p(64), 100, 1000, C.byref(nd), None)   # a plan-only object takes no buffer
    # and the object still works: a window that starts exactly at the end of the last one, a NULL plan
    assert L.trxhip_ms_tx_submit(pair.obj.h, good.ctypes.data_as(C.c_void_p), 2, 50, 0, 0, None, None) == 0
    pair.model.submit([(102, 0, 0), (103, 0, 0)], (50, 0, 0))
    pair.render(100, 1000)
    assert L.trxhip_ms_tx_state(None, None) == EINVAL
