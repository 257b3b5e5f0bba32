"""The downlink burst scheduler's planner on plan-only objects (trxhip_tx_sched_create with ctx == NULL; no GPU): plan and
counters against tests/tx_sched_model.py, the cited restatement of Transceiver.cpp's transmit path."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from osmo_trx_amd import build as trx_build  # noqa: E402
from osmo_trx_amd import trxhip  # noqa: E402
import tx_sched_model as M  # noqa: E402

SRC = {trxhip.TXS_SRC_ZERO: "zero", trxhip.TXS_SRC_BURST: "burst", trxhip.TXS_SRC_FILLER: "filler"}


@pytest.fixture(scope="module", autouse=True)
def lib():
    trx_build.build_lib()
    return trxhip.load_library()


class Pair:
    """the same calls on a plan-only scheduler and on the model; every render's plan and the counters compared"""

    def __init__(self, chans, sps, filler, max_slots=4096, queue_cap=4096):
        self.s = trxhip.TxScheduler(None, chans=chans, sps=sps, filler=filler, max_slots=max_slots, queue_cap=queue_cap)
        self.m = M.Model(chans, sps, filler)
        self.chans = chans
        self.plans = [[] for _ in range(chans)]

    def set_clock(self, fn, tn):
        self.s.set_clock(fn, tn)
        self.m.set_clock(fn, tn)

    def set_slot(self, c, tn, comb):
        self.s.set_slot(c, tn, comb)
        self.m.set_slot(c, tn, comb)

    def set_muted(self, c, on):
        self.s.set_muted(c, on)
        self.m.set_muted(c, on)

    def submit(self, c, d):
        a, b = self.s.submit(c, d), self.m.submit(c, d)
        assert a == b, (a, b)
        return a

    def render(self, n):
        self.s.render(n)
        want = self.m.render(n)
        for c in range(self.chans):
            p = self.s.plan(c)
            got = [(SRC[int(x["src"])], int(x["id"])) for x in p]
            assert got == want[c], next((k, got[k], want[c][k]) for k in range(n) if got[k] != want[c][k])
            self.plans[c] += got
        assert self.s.clock() == self.m.clock
        self.check_counters()

    def check_counters(self):
        for c in range(self.chans):
            assert self.s.counters(c) == self.m.ch[c].ctr, c


def traffic(rng, pair, fn0, n_frames, chans, sps, p_bad=0.02, chunks=(1, 7, 1000), toggles=True, slot_changes=True, prefill=False):
    """random downlink traffic ahead of the clock: bursts per (chan, TN) submitted a few frames early, some missing, late,
    out of order, repeated, duplicated or malformed; mute toggled and slots reconfigured between renders"""
    pos = 0                                        # slots rendered
    nxt = [[fn0 + 2] * 8 for _ in range(chans)]    # next FN each (chan, TN) stream submits
    total = n_frames * 8
    k = 0
    while pos < total:
        n = min(chunks[k % len(chunks)], total - pos)
        k += 1
        horizon = n_frames + 3 if prefill else (pos + n) // 8 + 3    # frames submitted before this render
        for c in range(chans):
            for tn in range(8):
                while (nxt[c][tn] - fn0) < horizon:
                    fn = nxt[c][tn] % M.HYPERFRAME
                    r = rng.random()
                    bits = rng.integers(0, 2, 148)
                    if r < 0.15:
                        pass                        # missing burst: filler
                    elif r < 0.18:
                        pair.submit(c, M.dgram((fn - rng.integers(3, 9)) % M.HYPERFRAME, tn, bits))       # stale / out of order
                    elif r < 0.20:
                        pair.submit(c, M.dgram(fn, tn, bits))
                        pair.submit(c, M.dgram(fn, tn, bits))                                          # repeated FN
                    elif r < 0.22:
                        pair.submit(c, M.dgram(fn, tn, bits, att=3))
                        pair.submit(c, M.dgram((fn - 1) % M.HYPERFRAME, tn, bits))
                        pair.submit(c, M.dgram(fn, tn, bits, att=5))                                   # duplicate (FN, TN)
                    elif r < 0.22 + p_bad:
                        bad = rng.integers(0, 3)
                        if bad == 0:
                            pair.submit(c, M.dgram(fn, tn, bits)[:100])
                        elif bad == 1:
                            pair.submit(c, M.dgram(fn, tn, bits, version=2))
                        else:
                            pair.submit(c, M.dgram(fn, tn, rng.integers(0, 2, 444)))                    # 8-PSK (refused at 1 SPS)
                    else:
                        if rng.random() < 0.02:
                            nxt[c][tn] += int(rng.integers(1, 4))                                       # skipped FNs
                            fn = nxt[c][tn] % M.HYPERFRAME
                        pair.submit(c, M.dgram(fn, tn, bits, att=int(rng.integers(0, 20))))
                    nxt[c][tn] += 1
        if toggles and rng.random() < 0.1:
            c = int(rng.integers(0, chans))
            pair.set_muted(c, not pair.m.ch[c].muted)
        if slot_changes and rng.random() < 0.05:
            pair.set_slot(int(rng.integers(0, chans)), int(rng.integers(0, 8)), int(rng.choice([1, 4, 7, 13, M.COMB_NONE, 0, 8])))
        pair.render(n)
        pos += n


@pytest.mark.parametrize("filler", [M.FILLER_DUMMY, M.FILLER_ZERO])
@pytest.mark.parametrize("sps", [4, 1])
def test_random_traffic_matches_model(filler, sps):
    rng = np.random.default_rng(7 + filler + sps)
    p = Pair(3, sps, filler)
    fn0 = 1000
    p.set_clock(fn0, 0)
    for c in range(3):
        for tn, comb in enumerate([5, 1, 7, 13, 1, M.COMB_NONE, 4, 1]):
            p.set_slot(c, tn, comb)
    traffic(rng, p, fn0, 3000, 3, sps)
    srcs = [s for s, _ in p.plans[0]]
    assert srcs.count("burst") > 1000 and srcs.count("filler") > 100 and srcs.count("zero") > 100
    ctr = p.s.counters(0)
    assert ctr["tx_stale_bursts"] > 0 and ctr["tx_trxd_fn_repeated"] > 0 and ctr["tx_trxd_fn_outoforder"] > 0 and ctr["refused"] > 0
    if filler == M.FILLER_DUMMY:          # retransmitted bursts come back as fillers
        assert any(s == "filler" and i >= 0 for s, i in p.plans[0])
    else:
        assert ctr["tx_unavailable_bursts"] > 0 and ctr["tx_trxd_fn_skipped"] > 0


def test_chunking_does_not_change_plan():
    plans = []
    for chunks in [(1,), (7,), (1000,), (1, 7, 1000), (3, 333, 5)]:
        rng = np.random.default_rng(11)
        p = Pair(3, 4, M.FILLER_DUMMY)
        p.set_clock(500, 3)
        for c in range(3):
            for tn in range(8):
                p.set_slot(c, tn, [5, 1, 7, 13][tn % 4])
        traffic(rng, p, 500, 400, 3, 4, chunks=chunks, toggles=False, slot_changes=False, prefill=True)
        plans.append((p.plans, [p.s.counters(c) for c in range(3)]))
    assert all(x == plans[0] for x in plans[1:])


def test_retransmitted_burst_reused_in_one_render():
    p = Pair(1, 4, M.FILLER_DUMMY)
    p.set_clock(100, 0)
    p.set_slot(0, 2, 1)                     # modulus 26
    i = p.submit(0, M.dgram(100, 2, [1] * 148, att=4))
    p.render(8 * 60)
    plan = p.plans[0]
    assert plan[2] == ("burst", i)
    assert plan[8 * 26 + 2] == ("filler", i) and plan[8 * 52 + 2] == ("filler", i)
    assert plan[8 * 1 + 2] == ("filler", -1)


def test_fn_wrap():
    p = Pair(2, 4, M.FILLER_ZERO)
    fn0 = M.HYPERFRAME - 20
    p.set_clock(fn0, 5)
    for c in range(2):
        for tn in range(8):
            p.set_slot(c, tn, 1)
    ids = []
    for k in range(40):
        fn = (fn0 + k) % M.HYPERFRAME
        ids.append(p.submit(0, M.dgram(fn, 6, [k & 1] * 148)))
    p.submit(1, M.dgram(M.HYPERFRAME - 1, 1, [0] * 148))
    p.submit(1, M.dgram(0, 1, [0] * 148))
    p.submit(1, M.dgram(M.HYPERFRAME - 2, 1, [0] * 148))      # out of order across the wrap
    p.render(8 * 41)
    got = [i for s, i in p.plans[0] if s == "burst"]
    assert got == ids
    assert p.s.counters(1)["tx_trxd_fn_outoforder"] == 1
    assert p.s.clock()[0] == (fn0 + 41) % M.HYPERFRAME


def test_mute_none_and_moduli():
    p = Pair(1, 4, M.FILLER_DUMMY)
    p.set_clock(0, 0)
    for tn, comb in enumerate([4, 7, 13, 1, M.COMB_NONE, 0, 6, 15]):
        p.set_slot(0, tn, comb)
    for fn in range(0, 120):
        for tn in range(8):
            if (fn + tn) % 3:
                p.submit(0, M.dgram(fn, tn, [(fn >> tn) & 1] * 148))
    p.render(8 * 30)
    p.set_muted(0, True)
    p.render(8 * 10)
    p.set_muted(0, False)
    p.render(8 * 80)
    assert all(s == "zero" for s, _ in p.plans[0][8 * 30:8 * 40])
    assert all(s == "zero" for s, _ in p.plans[0][4::8])


def test_refusals_leave_state_untouched():
    s = trxhip.TxScheduler(None, chans=2, sps=4, max_slots=16, queue_cap=2)
    with pytest.raises(trxhip.TrxHipError):
        s.render(1)                                           # before set_clock
    s.set_clock(10, 0)
    for bad in [lambda: s.set_slot(2, 0, 1), lambda: s.set_slot(0, 8, 1), lambda: s.set_slot(0, 0, 16),
                lambda: s.set_muted(-1, 1), lambda: s.submit(2, M.dgram(10, 0, [0] * 148)), lambda: s.render(17),
                lambda: s.set_clock(M.HYPERFRAME, 0), lambda: s.set_clock(0, 8)]:
        with pytest.raises(trxhip.TrxHipError):
            bad()
    assert s.clock() == (10, 0)
    assert s.submit(0, M.dgram(12, 0, [0] * 148)) == 0 and s.submit(0, M.dgram(13, 0, [0] * 148)) == 1
    with pytest.raises(trxhip.TrxHipError):                   # queue full: ENOMEM, the FN-order state unchanged
        s.submit(0, M.dgram(14, 0, [0] * 148))
    assert s.counters(0) == dict.fromkeys(M.COUNTERS, 0)
    for cfg in [dict(chans=0), dict(chans=9), dict(sps=2), dict(filler=2), dict(queue_cap=0), dict(max_slots=0)]:
        with pytest.raises(trxhip.TrxHipError):
            trxhip.TxScheduler(None, **cfg)
