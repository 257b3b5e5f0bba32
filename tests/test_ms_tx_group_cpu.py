"""CPU tests of the MS-side uplink scheduler group (trxhip_ms_tx_group_*, osmo_trx_amd.MsTxSchedulerGroup): the plan-only group
against N plan-only single objects (MsTxScheduler) and against the literal model (tests/ms_tx_model.py) -- every plan record of
every request, every member's state() after every call --, every refusal with all members untouched and the same call without
the bad item accepted, and the exported names.  No GPU is opened."""
import os

import numpy as np
import pytest

import ms_tx_model as M
import osmo_trx_amd
from osmo_trx_amd import trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = M.HYPERFRAME
BITS = (np.arange(148) * 5 % 3 == 0).astype(np.uint8)
FS, DELAY = 2047, -60
PLAN_KEYS = ("status", "send_ts", "radio_ts", "diff_fn", "diff_tn")
GAPS = {15: 3, 30: 6}                    # round: the member whose window leaves a gap behind the one before


def reqs_of(triples):
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    return trxhip.ms_tx_requests(t[:, 0], t[:, 1], t[:, 2], np.tile(BITS, (len(t), 1)))


def target_for(now_fn, diff_fn, ttn):
    """the request (fn, tn) whose target after incTN(3) is (now_fn + diff_fn, ttn)"""
    t = M.Time((now_fn + diff_fn) % H, ttn).decTN(3)
    return t.fn, t.tn


class Trio:
    """a plan-only group, and per member a plan-only single object and the model"""

    def __init__(self, n, max_pending):
        self.n = n
        self.group = trxhip.MsTxSchedulerGroup(None, n_members=n, tx_full_scale=FS, rxtx_delay=DELAY, max_pending=max_pending)
        self.single = [trxhip.MsTxScheduler(None, tx_full_scale=FS, rxtx_delay=DELAY, max_pending=max_pending) for _ in range(n)]
        self.model = [M.MsTx(FS, DELAY, max_pending) for _ in range(n)]

    def set_ta(self, m, val):
        self.group.set_ta(m, val)
        self.single[m].set_ta(val)
        self.model[m].set_ta(val)
        self.check_states()

    def submit(self, members, triples, clocks):
        """one group submit of requests that mix members; the same requests, per member and in order, to the singles and models"""
        plan = self.group.submit(members, reqs_of(triples), clocks)
        assert len(plan) == len(triples) and self.group.bad == -1
        for m in sorted(set(members)):
            idx = [i for i, x in enumerate(members) if x == m]
            mine = [triples[i] for i in idx]
            ps = self.single[m].submit(reqs_of(mine), clocks[m])
            pm = self.model[m].submit(mine, clocks[m])
            assert plan[idx].tobytes() == ps.tobytes(), (m, plan[idx], ps)
            for p, r, t in zip(plan[idx], pm, mine):
                for k in PLAN_KEYS:
                    assert int(p[k]) == r[k], (k, m, t, clocks[m], p, r)
                assert p["scale"].tobytes() == r["scale"].tobytes()
        self.check_states()
        return plan

    def render(self, sizes, first_ts):
        _, nd = self.group.render(sizes, first_ts)
        assert self.group.bad == -1
        for m in range(self.n):
            if sizes[m]:
                _, nd_s = self.single[m].render(sizes[m], first_ts[m])
                nd_m, _ = self.model[m].render(sizes[m], first_ts[m])
                assert nd[m] == nd_s == nd_m, (m, nd[m], nd_s, nd_m)
            else:
                assert nd[m] == 0
        self.check_states()
        return nd

    def check_states(self):
        for m in range(self.n):
            st = self.group.state(m)
            assert st.tobytes() == self.single[m].state().tobytes(), (m, st, self.single[m].state())
            for k, v in self.model[m].state().items():
                assert int(st[k]) == v, (m, k, st)

    def snapshot(self):
        return [self.group.state(m).tobytes() for m in range(self.n)]


def test_group_equals_singles_equals_the_model():
    """7 members, 45 rounds of one mixed submit and one render each: a clock 20 frames before the hyperframe wrap, now_ts near 0
    and near 2^40, seven timing advances with a rising and a falling change mid-run, requests of several members interleaved
    in one submit, member 4 without a request, member 5 never rendered (its queue fills: FULL), window lengths 0 .. 12998 that
    differ per member and round, two gaps between windows (missed), and every plan status met"""
    n, rounds = 7, 45
    rng = np.random.default_rng(4100)
    trio = Trio(n, max_pending=6)
    start = [(1000, 2, 7), (H - 20, 5, (1 << 40) + 311), (5000, 0, 5000), (H // 2, 7, 1 << 40), (40, 1, 99), (2000, 4, 1 << 33),
             (777, 3, 12345)]
    for m, ta in enumerate((0, 3, 10, -5, 0, 7, 127)):
        trio.set_ta(m, ta)
    lengths = (5000, 4999, 626, 9375, 0, 7000, 1, 5001, 12998)             # 5000 on average: the windows keep up with the clocks
    at = [c[2] for c in start]                                              # where each member's next window begins
    seen = np.zeros(6, dtype=int)
    for r in range(rounds):
        if r == 12:
            trio.set_ta(0, 4)                                               # rising: the next TN's burst overlaps a queued one
        if r == 27:
            trio.set_ta(2, 2)                                               # falling: gaps between adjacent TNs
        clocks = [((fn + r) % H, tn, ts + 5000 * r) for fn, tn, ts in start]
        members, triples = [], []
        for m in rng.permutation([0, 1, 2, 3, 5, 6])[:int(rng.integers(2, 7))]:
            for _ in range(int(rng.integers(1, 4))):
                dfn = int(rng.choice([-1, 0, 0, 1, 1, 1, 2]))
                fn, tn = target_for(clocks[m][0], dfn, int(rng.integers(0, 8)))
                members.append(int(m))
                triples.append((fn, tn, int(rng.integers(0, 40))))
        if r in GAPS:                                                       # six frames ahead of its clock: behind its windows
            members.append(GAPS[r])
            triples.append(target_for(clocks[GAPS[r]][0], 6, 4) + (0,))
        order = rng.permutation(len(members))                             # the members' requests interleave
        members, triples = [members[i] for i in order], [triples[i] for i in order]
        plan = trio.submit(members, triples, clocks)
        seen += np.bincount(plan["status"], minlength=6)
        sizes = [0 if m == 5 else lengths[(r + 2 * m) % len(lengths)] for m in range(n)]
        if r in GAPS:                                                       # a gap over a queued burst no window has touched: missed
            fresh = [b[0] for b in trio.model[GAPS[r]].q if not b[1]]
            assert fresh
            at[GAPS[r]] = max(at[GAPS[r]], min(fresh) + 625 + 7)
        trio.render(sizes, at)
        at = [a + s for a, s in zip(at, sizes)]
    assert seen.all(), seen                                                 # QUEUED, LATE, WRAPPED, EXPIRED, OVERLAP, FULL
    st = [trio.group.state(m) for m in range(n)]
    assert st[4]["submitted"] == 0 and st[4]["window_set"] == 1
    assert st[5]["window_set"] == 0 and st[5]["pending"] == 6 and st[5]["full"] > 0 and st[5]["drawn"] == 0
    assert sum(int(s["missed"]) for s in st) > 0 and sum(int(s["drawn"]) for s in st) > 20
    assert len({int(s["timing_advance"]) for s in st}) >= 6


def busy_trio():
    trio = Trio(4, max_pending=8)
    clocks = [(50, 0, 0), (60, 3, 1 << 20), None, (70, 7, -5000)]
    trio.set_ta(1, 5)
    trio.submit([0, 1, 3, 0], [(100, 0, 0), (101, 1, 20), (75, 2, 0), (102, 3, 0)], clocks)
    trio.render([1000, 0, 700, 625], [0, 0, 10, -5000])
    return trio, clocks


def test_submit_refusals_leave_every_member_untouched():
    trio, clocks = busy_trio()
    before = trio.snapshot()
    good = [(103, 0, 0), (104, 1, 0), (80, 2, 0)]
    for members, triples, cl, bad_at in (
            ([0, 4, 3], good, clocks, 1),                                   # a member index out of range
            ([0, 0xFFFFFFFF, 3], good, clocks, 1),
            ([0, 1, 3], [good[0], good[1], (80, 8, 0)], clocks, 2),         # tn > 7
            ([0, 1, 3], [good[0], (H, 1, 0), good[2]], clocks, 1),          # fn outside the hyperframe
            ([0, 2, 3], good, clocks, 1),                                   # member 2 is named and has no clock
            ([0, 1, 3], good, [clocks[0], (60, 8, 0), None, clocks[3]], 1),  # a named member's clock with tn 8
            ([0, 1, 3], good, [clocks[0], clocks[1], None, (H, 0, 0)], 2)):
        with pytest.raises(trxhip.TrxHipError):
            trio.group.submit(members, reqs_of(triples), cl)
        assert trio.group.bad == bad_at
        assert trio.snapshot() == before
    # a bad clock of a member that no request names is not read
    trio.submit([0, 1, 3], good, [clocks[0], clocks[1], (H, 9, 0), clocks[3]])
    assert trio.snapshot() != before


def test_render_refusals_leave_every_member_untouched():
    trio, clocks = busy_trio()
    before = trio.snapshot()
    ends = [int(trio.group.state(m)["rendered_end"]) for m in range(4)]
    assert ends == [1000, 0, 710, -4375]

    def refused(sizes, first_ts, bad, **kw):
        with pytest.raises(trxhip.TrxHipError):
            trio.group.render(sizes, first_ts, **kw)
        assert trio.group.bad == bad and trio.snapshot() == before

    refused([100, 100, 100, 100], [1000, 0, 709, -4375], 2)                 # member 2's window goes backwards
    refused([100, 100, 100, 100], [1000, 0, 709, -4376], 2)                 # two bad members: the lowest is reported
    refused([100, 100, 100, 100], [999, 0, 709, -4376], 0)
    refused([100, 100, 101, 100], ends, 2, out_stride=100)                  # n_samples > out_stride
    refused([100, 100, 100, (1 << 31) + 1], ends, 3)
    refused([100, 100, 100, 100], [1000, 0, 710, (1 << 62) + 1], 3)
    # a member that is not rendered is not checked: member 2 would go backwards, with n_samples 0 it is left alone
    trio.render([100, 100, 0, 100], [1000, 0, 0, -4375])
    # and the same windows without the bad item pass; out_stride 0 leaves a plan-only group unbounded
    trio.group.render([100, 100, 100, 100], [1100, 100, 710, -4275], out_stride=100)
    for m, s in enumerate(trio.single):
        s.render(100, [1100, 100, 710, -4275][m])
    for m, mod in enumerate(trio.model):
        mod.render(100, [1100, 100, 710, -4275][m])
    trio.check_states()


def test_create_refusals_and_member_calls():
    import ctypes as C
    L = trxhip.load_library()
    for n, fs, mp in ((4, 21478, 16), (4, 1 << 31, 16), (0, 2047, 16), (4097, 2047, 16), (4, 2047, 0), (4, 2047, (1 << 22) + 1),
                      (4096, 2047, 1 << 20)):                               # 2^32 ring rows: one more than a uint32 names
        with pytest.raises(trxhip.TrxHipError):
            trxhip.MsTxSchedulerGroup(None, n_members=n, tx_full_scale=fs, max_pending=mp)
    g = trxhip.MsTxSchedulerGroup(None, n_members=trxhip.MS_TX_GROUP_MAX_MEMBERS, tx_full_scale=21477, max_pending=(1 << 20) - 1)
    assert L.trxhip_ms_tx_group_size(g.h) == 4096 and L.trxhip_ms_tx_group_size(None) == -22
    before = g.state(4095).tobytes()
    for m, val in ((4096, 0), (0, -127), (0, 128)):
        assert L.trxhip_ms_tx_group_set_ta(g.h, m, val) == -22
    assert L.trxhip_ms_tx_group_state(g.h, 4096, C.c_void_p(0)) == -22 and L.trxhip_ms_tx_group_state(g.h, 0, None) == -22
    # a plan-only group takes no buffer
    ts, ns = (C.c_int64 * 4096)(), (C.c_size_t * 4096)()
    ns[7] = 10
    assert L.trxhip_ms_tx_group_render_s16(g.h, C.c_void_p(64), 100, C.cast(ts, C.c_void_p), C.cast(ns, C.c_void_p), None, None, None) == -22
    assert g.state(4095).tobytes() == before and g.state(7)["window_set"] == 0
    assert L.trxhip_ms_tx_group_render_s16(g.h, None, 100, C.cast(ts, C.c_void_p), C.cast(ns, C.c_void_p), None, None, None) == 0
    assert g.state(7)["window_set"] == 1 and g.state(7)["rendered_end"] == 10 and g.state(6)["window_set"] == 0
    g.set_ta(4095, -126)
    assert g.state(4095)["timing_advance"] == -504
    g.close()


def test_every_symbol_is_exported():
    L = trxhip.load_library()
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    names = ("create", "destroy", "size", "set_ta", "submit", "render_s16", "state")
    for name in names:
        full = "trxhip_ms_tx_group_" + name
        assert hasattr(L, full) and full in trxhip.SYMBOLS and full + "(" in hdr
    assert sorted(s for s in trxhip.SYMBOLS if s.startswith("trxhip_ms_tx_group_")) == sorted("trxhip_ms_tx_group_" + x for x in names)
    assert L.trxhip_abi_version() == 5
    assert osmo_trx_amd.MsTxSchedulerGroup is trxhip.MsTxSchedulerGroup and "MsTxSchedulerGroup" in osmo_trx_amd.__all__
