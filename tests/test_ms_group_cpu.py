"""CPU tests of the MS-side scheduler group (trxhip_ms_group_*, osmo_trx_amd.MsRxSchedulerGroup): the plan-only group against N
plan-only single objects and against the literal model (tests/ms_sched_model.py) after every pull; a refused group pull moves
nothing; and the precondition of the GPU loopback test on the CPU models alone.  No GPU is opened.

out_stride: the plan-only single object has no output bound (it takes no buffers); the plan-only group checks the counts
against out_stride when it is not 0, which is how "out_stride too small" is met here without a GPU."""
import ctypes as C

import numpy as np
import pytest

import ms_group_cases as GC
import ms_rx_cases as K
import ms_rx_model as RX
import ms_sched_model as SM
from osmo_trx_amd import trxhip

EINVAL = -22
STARTS = (-39, -2, -1, 0, 1, 2, 39, None)                          # None: decode_sch() failed
NO_SCH = trxhip.MS_SCHED_NO_SCH


def cycle_starts():
    """starts for the SCH slots in the order they are cut, over all members that share it: every value of STARTS comes by"""
    count = [0]

    def starts(fn, tn, ts):
        count[0] += 1
        return STARTS[(count[0] * 3) % len(STARTS)]

    return starts


class Member:
    """one member three times: the model, a plan-only single object, and its index in the group"""

    def __init__(self, idx, tracking=True, tsc=3, active=0b10100101, starts=None):
        self.idx, self.tracking, self.tsc, self.active = idx, tracking, tsc, active
        self.single = trxhip.MsRxScheduler(None, tsc=tsc, active_tns=active, tracking=tracking)
        self.used, self.seen = [], []
        starts = starts or (lambda fn, tn, ts: STARTS[(fn // 10 * 5 + fn // 51 + idx) % len(STARTS)])

        def cb(fn, tn, ts):
            self.used.append(starts(fn, tn, ts))
            return self.used[-1]

        self.model = SM.Cutter(cb, tracking=tracking)
        self.ts = 0

    def snapshot(self, group):
        st = group.state(self.idx)
        return (group.clock(self.idx) if st["clock_set"] else None, st.tobytes())


def model_pull(mem, n):
    """the model's pull; returns (plan or None where it refuses, the feed the pull consumes)"""
    mem.used = []
    try:
        want = mem.model.grab_bursts(mem.ts, n)
    except SM.Refused:
        want = None
    return want, [NO_SCH if s is None else s for s in mem.used]


def same_member(group, mem, want, n_slots, n_carried):
    """group member == single object == model, after a pull in which the member had a chunk"""
    i, s, m = mem.idx, mem.single, mem.model
    assert (n_slots, n_carried) == (len(want), m.partial_rdofs) == (s._last, s.carried)
    got = group.plan(i, n_slots)
    assert got.tobytes() == s.plan().tobytes()
    assert [(int(p["fn"]), int(p["tn"]), int(p["ts"]), int(p["src_off"])) for p in got] == want
    for p in got:
        assert p["kind"] == trxhip.ms_slot_kind(int(p["fn"]), int(p["tn"]), mem.tsc)
        assert p["flags"] == (mem.active >> int(p["tn"])) & 1
    st = group.state(i)
    assert st.tobytes() == s.state().tobytes()                    # to_skip, pending, carried, first_call, every counter
    assert group.clock(i) == s.clock() == (m.tk.fn, m.tk.tn, m.tk.ts)
    assert (st["to_skip"], st["pending"], st["carried"], st["clock_jumps"]) == (m.to_skip, m.temp_ts_corr_offset, m.partial_rdofs,
                                                                             m.tk.jumps)
    assert st["first_call"] == int(m.first_call) and st["tsc"] == mem.tsc and st["tracking"] == int(mem.tracking)


def group_pull(group, mems, sizes, feed_group=True):
    """one group pull, the singles and the models beside it; sizes[m] == 0: no chunk.  feed_group=False: the group's queues hold
    the pull's starts already.  Returns the models' plans."""
    wants = {}
    for mem, n in zip(mems, sizes):
        if not n:
            continue
        want, feed = model_pull(mem, n)
        assert want is not None
        wants[mem.idx] = want
        mem.seen += mem.used
        mem.single.feed_starts(feed)
        if feed_group:
            group.feed_starts(mem.idx, feed)
        assert group.slots(mem.idx, n) == mem.single.slots(n)
        mem.single.pull(n_samples=n, first_ts=mem.ts)
    idle = {mem.idx: (mem.snapshot(group), group.plan(mem.idx, 0).tobytes()) for mem, n in zip(mems, sizes) if not n}
    ns, nc = group.pull(n_samples=sizes, first_ts=[mem.ts for mem in mems])
    assert group.bad_member == -1
    for mem, n in zip(mems, sizes):
        if n:
            same_member(group, mem, wants[mem.idx], ns[mem.idx], nc[mem.idx])
            mem.ts += n
        else:                                                      # no chunk: nothing of the member changes
            assert ns[mem.idx] == 0 and nc[mem.idx] == mem.model.partial_rdofs
            assert (mem.snapshot(group), group.plan(mem.idx, 0).tobytes()) == idle[mem.idx]
            assert group.state(mem.idx).tobytes() == mem.single.state().tobytes()
    return wants


def test_group_equals_singles_equals_the_model():
    """7 members, 40 pulls: different start clocks (one 3 slots in front of the hyperframe wrap), first calls after a batched
    acquire with fracts 0, 1 and 624, chunk sizes 700 .. 6000 that differ per member and per pull (aligned ones included),
    every value of STARTS fed, a tracking-off member among tracking-on ones, a member whose chunks only extend its partial slot
    and that has no chunk in some pulls, and a member whose straddling slot is an SCH slot."""
    rng = np.random.default_rng(5200)
    trk = [True, True, False, True, True, True, True]
    shared = cycle_starts()
    mems = [Member(i, tracking=t, tsc=i, active=0xA5 ^ ((i * 17) & 0xFF), starts=shared) for i, t in enumerate(trk)]
    mems[6] = Member(6, tsc=6, active=0x3C, starts=lambda fn, tn, ts: -7)
    group = trxhip.MsRxSchedulerGroup(None, n=7, tsc=[m.tsc for m in mems], active_tns=[m.active for m in mems], tracking=trk)
    for i, (fn, tn, ts) in {0: (51 * 3, 6, 0), 1: (SM.HYPERFRAME - 1, 4, 99_000), 2: (51 * 7 + 20, 7, -625), 6: (51 * 3, 6, 0)}.items():
        group.set_clock(i, fn, tn, ts)
        mems[i].single.set_clock(fn, tn, ts)
        mems[i].model.set_clock(fn, tn, ts)
        mems[i].ts = ts + 625
    # members 3, 4, 5: one batched acquire; their first chunks begin fracts = 0, 1, 624 samples behind a slot boundary
    recs = np.zeros(3, dtype=trxhip.SCH_SYNC_DTYPE)
    t_acq = [777_000, -40_000, 5]
    for k, i in enumerate((3, 4, 5)):
        recs[k]["rc"], recs[k]["start"], recs[k]["fn"], recs[k]["bsic"] = 1, 30_005 + k, 51 * 40 + 21 + 10 * k, 0o50 + k
    found, _ = group.acquire([3, 4, 5], results=recs, first_ts=t_acq)
    assert found.all()
    for k, (i, fracts) in enumerate(zip((3, 4, 5), (0, 1, 624))):
        f, _ = mems[i].single.acquire(first_ts=t_acq[k], result=recs[k])
        assert f
        mems[i].model.acquired(int(recs[k]["fn"]), int(recs[k]["start"]), t_acq[k])
        mems[i].tsc = int(recs[k]["bsic"]) & 7
        st = group.state(i)
        assert st.tobytes() == mems[i].single.state().tobytes() and st["first_call"] == 1
        mems[i].ts = int(st["first_sch_ts_start"]) + (2 + k) * 625 + fracts

    n_pulls = 40
    sizes = rng.integers(700, 6001, (n_pulls, 7))
    sizes[0, 0], sizes[1, 0] = 1225, 3000                          # member 0: (153, 7) cut, 600 carried; then the SCH slot (154, 0) straddles
    sizes[:6, 2] = [1250, 625, 5000, 700, 1875, 6000]              # member 2, tracking off from an aligned clock: frac == 0 three times
    sizes[:14, 6] = [700, 100, 0, 1, 448, 1, 0, 3000, 800, 0, 0, 5000, 50, 0]   # member 6: extends its partial slot, or has no chunk
    sizes[20:, 6] = np.where(rng.random(20) < 0.4, 0, sizes[20:, 6])
    sizes[rng.random(n_pulls) < 0.2, 4] = 0
    sizes[0, 3:6] = 6000
    aligned = extended = straddled_sch = wrapped = 0
    for k in range(n_pulls):
        before6 = mems[6].model.partial_rdofs
        wants = group_pull(group, mems, [int(v) for v in sizes[k]])
        aligned += mems[2].model.partial_rdofs == 0
        extended += 6 in wants and wants[6] == [] and mems[6].model.partial_rdofs > before6
        if k == 1:
            straddled_sch += wants[0][0][:2] == (51 * 3 + 1, 0) and wants[0][0][3] == -600
        wrapped += 1 in wants and any(w[0] == 0 for w in wants[1])
    assert aligned >= 3 and extended >= 4 and straddled_sch == 1 and wrapped >= 1
    seen = set(s for m in mems for s in m.seen)
    assert seen >= set(STARTS), seen
    for mem in mems:
        st = group.state(mem.idx)
        assert st["pulls"] == np.count_nonzero(sizes[:, mem.idx]) and st["clock_jumps"] == 0
    assert group.state(2)["pending"] == 0 and not mems[2].seen


def _three():
    """members 0 and 2 with a clock one slot in front of an SCH slot, member 1 with 600 samples carried in front of one that
    will report 39; returns (group, members)"""
    mems = [Member(0, starts=lambda fn, tn, ts: 39), Member(1, starts=lambda fn, tn, ts: 39), Member(2, starts=lambda fn, tn, ts: -2)]
    group = trxhip.MsRxSchedulerGroup(None, n=3, tsc=3, active_tns=0b10100101, tracking=True)
    for mem in mems:
        group.set_clock(mem.idx, 51 * 3, 6, 0)
        mem.single.set_clock(51 * 3, 6, 0)
        mem.model.set_clock(51 * 3, 6, 0)
        mem.ts = 625
    group_pull(group, mems, [700, 1225, 5000])
    return group, mems


def _refused(group, mems, sizes, bad, out_stride=0, feeds=True):
    """the pull is refused with `bad` named; state, clock and plan of every member stay.  feeds: every member's queue holds what
    the pull would consume (the models move: the caller puts them back)"""
    if feeds:
        for mem, n in zip(mems, sizes):
            if n:
                _, feed = model_pull(mem, n)
                group.feed_starts(mem.idx, feed)
    before = [(mem.snapshot(group), group.plan(mem.idx).tobytes()) for mem in mems]
    with pytest.raises(trxhip.TrxHipError):
        group.pull(n_samples=sizes, first_ts=[mem.ts for mem in mems], out_stride=out_stride)
    assert group.bad_member == bad
    assert [(mem.snapshot(group), group.plan(mem.idx).tobytes()) for mem in mems] == before


def _model_state(mem):
    m = mem.model
    return (m.tk.fn, m.tk.tn, m.tk.ts, m.tk.jumps, m.partial_rdofs, m.first_call, m.temp_ts_corr_offset, m.to_skip)


def _model_restore(mem, saved):
    m = mem.model
    m.tk.fn, m.tk.tn, m.tk.ts, m.tk.jumps, m.partial_rdofs, m.first_call, m.temp_ts_corr_offset, m.to_skip = saved


@pytest.mark.parametrize("case", ["to_skip", "out_stride", "no_clock", "two_bad"])
def test_a_refused_group_pull_moves_no_member(case):
    """One member's pull is one the single object refuses: the code comes back with the lowest bad index, state(), clock() and
    plan() of EVERY member are unchanged, no feed queue is consumed, and the same pull without the bad member's chunk succeeds
    and equals the single objects'."""
    group, mems = _three()
    sizes, stride, bad = [3000, 3000, 3000], 0, 1
    if case == "to_skip":
        sizes[1] = 30                                              # the SCH slot completes: to_skip = 25 + 39 > 30
    elif case == "out_stride":
        stride = 4                                                 # members 0 and 2 cut 4 slots each, member 1 the completed slot
        sizes = [3000, 3100, 3000]                                 # and (3100 - 25 - 39) // 625 = 4 more
    elif case == "no_clock":
        mems = [Member(i) for i in range(4)]                       # member 3 never gets a clock
        group = trxhip.MsRxSchedulerGroup(None, n=4, tsc=3, active_tns=0b10100101, tracking=True)
        for mem in mems[:3]:
            group.set_clock(mem.idx, 51 * 3, 6, 0)
            mem.single.set_clock(51 * 3, 6, 0)
            mem.model.set_clock(51 * 3, 6, 0)
            mem.ts = 625
        sizes, bad = [3000, 3000, 3000, 3000], 3
    else:                                                          # members 1 and 2 both refuse: the lowest index is named
        sizes = [3000, 30, 0]
    saved = [_model_state(mem) for mem in mems]
    if case == "two_bad":
        group.feed_starts(0, [39, 39])                             # (the pull of 3000 consumes the first)
        group.feed_starts(1, [39])
        before = [(mem.snapshot(group), group.plan(mem.idx).tobytes()) for mem in mems]
        ch = np.zeros(3, dtype=trxhip.MS_GROUP_CHUNK_DTYPE)
        ch["n_samples"], ch["first_ts"] = [3000, 30, 1 << 41], [mem.ts for mem in mems]     # member 2: n_samples above the limit
        bad_m = C.c_int(-7)
        assert group.L.trxhip_ms_group_pull_s16(group.h, ch.ctypes.data_as(C.c_void_p), None, None, 0, None, None, C.byref(bad_m),
                                                None) == EINVAL
        assert bad_m.value == 1 and [(mem.snapshot(group), group.plan(mem.idx).tobytes()) for mem in mems] == before
        sizes = [3000, 0, 0]
    elif case == "no_clock":
        _refused(group, mems[:3] + [mems[3]], sizes, bad, feeds=False)
        assert group.state(3)["clock_set"] == 0
    else:
        _refused(group, mems, sizes, bad, out_stride=stride)
    for mem, s in zip(mems, saved):
        _model_restore(mem, s)
    # the same pull without the bad member's chunk: the feed queues were not consumed by the refused one
    if case != "two_bad":
        sizes[bad] = 0
    wants = group_pull(group, mems, sizes, feed_group=case == "no_clock")
    assert len(wants[0]) >= 4


def test_group_refusals_at_the_edges():
    L = trxhip.load_library()
    vp = C.c_void_p
    h = vp()
    cfgs = (trxhip._MsSchedCfg * 4097)(*[trxhip._MsSchedCfg(2047.0, 0, 0xFF, 1, 0)] * 4097)
    create = lambda full, n, c=cfgs: L.trxhip_ms_group_create(None, full, n, C.cast(c, vp), C.byref(h))     # noqa: E731
    assert create(2047.0, 0) == EINVAL and create(2047.0, trxhip.MS_GROUP_MAX_MEMBERS + 1) == EINVAL
    assert create(0.0, 2) == EINVAL and create(float("nan"), 2) == EINVAL
    assert create(2048.0, 2) == EINVAL                             # cfgs[i].rx_full_scale is not the group's
    odd = (trxhip._MsSchedCfg * 2)(trxhip._MsSchedCfg(2047.0, 0, 0xFF, 1, 0), trxhip._MsSchedCfg(2047.0, 8, 0xFF, 1, 0))
    assert create(2047.0, 2, odd) == EINVAL                        # tsc > 7
    assert L.trxhip_ms_group_create(None, 2047.0, 2, None, C.byref(h)) == EINVAL
    assert L.trxhip_ms_group_create(None, 2047.0, 2, C.cast(cfgs, vp), None) == EINVAL
    assert create(2047.0, trxhip.MS_GROUP_MAX_MEMBERS) == 0 and L.trxhip_ms_group_members(h) == 4096
    L.trxhip_ms_group_destroy(h)
    with pytest.raises(trxhip.TrxHipError):
        trxhip.MsRxSchedulerGroup(None, n=0)

    g = trxhip.MsRxSchedulerGroup(None, n=3, tsc=[1, 2, 3])
    for i in range(3):
        g.set_clock(i, 10, i, 0)
    with pytest.raises(trxhip.TrxHipError):
        g.pull(n_samples=[0, 0, 0], first_ts=625)                  # no member has a chunk
    assert g.bad_member == -1
    with pytest.raises(trxhip.TrxHipError):
        g.set_clock(3, 10, 0, 0)                                   # no such member
    assert L.trxhip_ms_group_set_clock(g.h, 0, 2715648, 0, 0) == EINVAL and L.trxhip_ms_group_set_tsc(g.h, 0, 8) == EINVAL
    assert L.trxhip_ms_group_slots(g.h, 3, 700) == EINVAL and L.trxhip_ms_group_state(g.h, 0, None) == EINVAL
    buf = (C.c_int16 * 8)()
    ch = np.zeros(3, dtype=trxhip.MS_GROUP_CHUNK_DTYPE)
    ch["n_samples"], ch["first_ts"] = 700, 625
    bad = C.c_int(-7)
    pull = lambda d_ind=None, d_bits=None: L.trxhip_ms_group_pull_s16(g.h, ch.ctypes.data_as(vp), d_ind, d_bits, 0, None, None,    # noqa: E731
                                                                      C.byref(bad), None)
    assert pull(d_ind=C.addressof(buf)) == EINVAL and bad.value == 0     # a plan-only group takes no buffers
    assert pull(d_bits=C.addressof(buf)) == EINVAL and bad.value == 0
    ch["d_in"][1] = C.addressof(buf)
    assert pull() == EINVAL and bad.value == 1
    ch["d_in"][1] = 0
    assert L.trxhip_ms_group_pull_cf32(g.h, ch.ctypes.data_as(vp), None, None, 0, None, None, None, None) == 0
    ch["first_ts"] += 700
    assert pull() == EINVAL and bad.value == 0                     # int16 over the complex64 partial slots
    assert L.trxhip_ms_group_pull_s16(g.h, None, None, None, 0, None, None, C.byref(bad), None) == EINVAL and bad.value == -1
    # acquire: a member listed twice, a member that does not exist, n == 0; nothing is touched
    before = [(g.clock(i), g.state(i).tobytes()) for i in range(3)]
    rec = np.zeros(2, dtype=trxhip.SCH_SYNC_DTYPE)
    rec["rc"], rec["fn"], rec["start"] = 1, 77, 1000
    for members in ([1, 1], [0, 3], []):
        with pytest.raises(trxhip.TrxHipError):
            g.acquire(members, results=rec[:len(members)], first_ts=0)
    rec["fn"][1] = 2715648                                         # a found record outside the hyperframe: nothing is assigned
    with pytest.raises(trxhip.TrxHipError):
        g.acquire([0, 1], results=rec, first_ts=0)
    assert [(g.clock(i), g.state(i).tobytes()) for i in range(3)] == before
    rec["fn"][1], rec["rc"][1] = 78, 0                             # member 1 not found: untouched
    found, _ = g.acquire([2, 1], results=rec, first_ts=[500, 600])
    assert list(found) == [True, False] and g.clock(2) == (77, 0, 0) and g.state(2)["first_sch_ts_start"] == 500 + 1000 - 17
    assert (g.clock(1), g.state(1).tobytes()) == before[1] and (g.clock(0), g.state(0).tobytes()) == before[0]


def test_header_wrapper_and_library_agree():
    L = trxhip.load_library()
    names = ("create", "destroy", "members", "set_clock", "clock", "set_tsc", "set_active", "set_tracking", "feed_starts", "slots", "plan",
             "state", "acquire_s16", "acquire_cf32", "pull_s16", "pull_cf32")
    hdr = open(trxhip.os.path.join(trxhip.os.path.dirname(trxhip.PKG), "include", "trxhip.h")).read()
    for name in names:
        full = "trxhip_ms_group_" + name
        assert hasattr(L, full) and full in trxhip.SYMBOLS and full + "(" in hdr
    assert sorted(n for n in trxhip.SYMBOLS if n.startswith("trxhip_ms_group_")) == sorted("trxhip_ms_group_" + n for n in names)
    assert L.trxhip_abi_version() == 5
    assert trxhip.MS_GROUP_CHUNK_DTYPE.itemsize == 24 and "#define TRXHIP_MS_GROUP_MAX_MEMBERS %d" % trxhip.MS_GROUP_MAX_MEMBERS in hdr
    import osmo_trx_amd
    assert osmo_trx_amd.MsRxSchedulerGroup is trxhip.MsRxSchedulerGroup and "MsRxSchedulerGroup" in osmo_trx_amd.__all__


@pytest.mark.parametrize("k", [0, 1, 2])
def test_loopback_precondition_on_the_cpu_models(k):
    """What tests/test_gpu_ms_group.py's batched acquire -> pull loopback relies on, on the models alone, per cell of
    tests/ms_group_cases.py: the ACQ model finds the one SCH burst of the buffer (and none in the noise member's), the model
    receiver recovers all 148 bits of EVERY ACTIVE traffic slot the cutter cuts, and the SCH slot decodes to the frame it is cut as."""
    L = GC.LOOPS[k]
    x, sent = GC.loop_stream(L)
    acq, out = GC.model_loopback(x, L)
    if L.get("noise"):
        assert acq["rc"] == 0 and not out
        return
    assert (acq["rc"], acq["fn"], acq["bsic"]) == (1, L["fn0"] + 7, L["bsic"]) and (L["fn0"] + 7) % 51 == 1
    traffic = [(fn, tn, m) for fn, tn, m in out if m["kind"] == RX.KIND_NB and m["sent"]]
    n_active = sum(1 for fn, tn, m in out if (L["active"] >> tn) & 1 and not SM.is_sch(fn, tn) and not SM.is_fcch(fn, tn))
    assert len(out) == (len(x) - L["acq_len"]) // 625 == 96 and len(traffic) == n_active >= 46
    for fn, tn, m in traffic:
        assert (L["active"] >> tn) & 1 and np.array_equal(m["bits"], K.hard(sent[(fn, tn)])), (fn, tn)
    sch = [(fn, m) for fn, tn, m in out if m["kind"] == RX.KIND_SCH]
    assert len(sch) == 1 and sch[0][1]["sch_rc"] == 1 and sch[0][1]["sch_fn"] == sch[0][0]
