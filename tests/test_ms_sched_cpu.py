"""CPU tests of the MS-side downlink slot scheduler (trxhip_ms_sched_*): the plan-only object (ctx == NULL) against the literal
restatement of the reference's cutter and clock (tests/ms_sched_model.py) -- plan, clock, ts, to_skip, pending correction and
carried count after every pull, with SCH starts fed from outside; every refusal with the state untouched; and the precondition
of the GPU loopback test on the CPU models alone.  No GPU is opened."""
import ctypes as C

import numpy as np
import pytest

import ms_rx_cases as K
import ms_rx_model as RX
import ms_sched_cases as SC
import ms_sched_model as SM
from osmo_trx_amd import trxhip

EINVAL = -22
STARTS = (-39, -2, -1, 0, 1, 2, 39, None)                          # None: decode_sch() failed


def start_of(fn, tn=0, ts=0):
    """the start the SCH slot of frame fn reports: every value of STARTS comes by, in an order that mixes the signs"""
    return STARTS[(fn // 10 * 5 + fn // 51) % len(STARTS)]


class Pair:
    """a plan-only object and the model side by side"""

    def __init__(self, tracking=True, tsc=3, active=0b10100101, starts=start_of):
        self.obj = trxhip.MsRxScheduler(None, tsc=tsc, active_tns=active, tracking=tracking)
        self.used = []

        def cb(fn, tn, ts):
            self.used.append(starts(fn, tn, ts))
            return self.used[-1]

        self.model = SM.Cutter(cb, tracking=tracking)
        self.tsc, self.active = tsc, active

    def set_clock(self, fn, tn, ts):
        self.obj.set_clock(fn, tn, ts)
        self.model.set_clock(fn, tn, ts)

    def acquire(self, fn, start, first_ts, bsic=0o25):
        rec = np.zeros(1, dtype=trxhip.SCH_SYNC_DTYPE)[0]
        rec["rc"], rec["start"], rec["fn"], rec["bsic"] = 1, start, fn, bsic
        found, _ = self.obj.acquire(first_ts=first_ts, result=rec)
        assert found
        self.model.acquired(fn, start, first_ts)
        self.tsc = bsic & 7

    def pull(self, first_ts, n):
        """one pull on both; returns the model's plan, or None where both refuse"""
        self.used = []
        before = self.snapshot()
        try:
            want = self.model.grab_bursts(first_ts, n)
        except SM.Refused:
            want = None
        self.obj.feed_starts([trxhip.MS_SCHED_NO_SCH if s is None else s for s in self.used])
        bound = self.obj.slots(n)
        ns, nc = C.c_size_t(), C.c_size_t()
        rc = self.obj.L.trxhip_ms_sched_pull_s16(self.obj.h, None, n, first_ts, None, None, 0, C.byref(ns), C.byref(nc), None)
        if want is None:
            assert rc == EINVAL and self.snapshot() == before
            return None
        assert rc == 0
        assert (ns.value, nc.value) == (len(want), self.model.partial_rdofs)
        assert ns.value <= bound
        if not self.model.tracking:
            assert ns.value == bound or before[-1]                 # exact, but for the first call after an acquire
        self.obj._last = ns.value
        got = self.obj.plan()
        assert [(int(p["fn"]), int(p["tn"]), int(p["ts"]), int(p["src_off"])) for p in got] == want
        for p in got:
            assert p["kind"] == trxhip.ms_slot_kind(int(p["fn"]), int(p["tn"]), self.tsc)
            assert p["flags"] == (self.active >> int(p["tn"])) & 1 and p["reserved"] == 0 and p["reserved2"] == 0
        self.same_state()
        return want

    def snapshot(self):
        st = self.obj.state()
        clock = self.obj.clock() if st["clock_set"] else None
        return (clock, st.tobytes(), bool(st["first_call"]))

    def same_state(self):
        st, m = self.obj.state(), self.model
        assert self.obj.clock() == (m.tk.fn, m.tk.tn, m.tk.ts)
        assert (st["to_skip"], st["pending"], st["carried"], st["clock_jumps"]) == (m.to_skip, m.temp_ts_corr_offset, m.partial_rdofs,
                                                                                 m.tk.jumps)
        assert st["first_call"] == int(m.first_call) and st["tsc"] == self.tsc


def run_stream(pair, sizes, first_ts):
    cut, applied = 0, set()
    for n in sizes:
        before = pair.model.temp_ts_corr_offset
        want = pair.pull(first_ts, int(n))
        assert want is not None
        if before and pair.model.temp_ts_corr_offset != before:
            applied.add(before)
        cut += len(want)
        first_ts += int(n)
    return cut, applied


SIZES = [700, 6000, 1250, 625, 5000, 4999, 5001, 1875, 3333, 701, 2500, 5999]   # 625, 1250, 1875, 2500, 5000: frac == 0 when aligned


@pytest.mark.parametrize("tracking", [True, False])
def test_chunk_sizes_and_injected_starts(tracking):
    """Chunk sizes from 700 to 6000 against the model, from a clock whose next slot is an SCH slot.  With tracking every value of
    STARTS is met, abs(start) <= 1 and a failed decode move nothing, and both signs of the correction are applied."""
    rng = np.random.default_rng(5100)
    pair = Pair(tracking=tracking)
    pair.set_clock(51 * 3, 7, 10_000 - 625)
    sizes = SIZES * 4 + [int(v) for v in rng.integers(700, 6001, 160)]
    cut, applied = run_stream(pair, sizes, 10_000)
    st = pair.obj.state()
    assert st["slots"] == cut and st["pulls"] == len(sizes) and st["clock_jumps"] == 0
    assert st["sch_slots"] == sum(1 for s in range(cut) if SM.is_sch(51 * 3 + 1 + s // 8, s % 8))
    if tracking:
        assert any(a > 0 for a in applied) and any(a < 0 for a in applied)
    else:
        assert not applied and st["pending"] == 0 and cut == sum(sizes) // 625


def test_aligned_chunks_leave_no_partial_slot_and_the_clamp_keeps_the_offset():
    """Chunks of whole slots from an aligned clock: frac == 0, nothing is carried.  The first SCH slot reports -39: the pending
    +39 exceeds to_skip = 0, so to_skip is clamped to 0 and the offset is kept whole (ms_rx_lower.cpp:403-404), pull after pull."""
    pair = Pair(starts=lambda fn, tn, ts: -39 if fn == 51 * 3 + 1 else 0)
    pair.set_clock(51 * 3, 7, -625)
    ts = 0
    for n in (5000, 1250, 625):
        want = pair.pull(ts, n)
        assert len(want) == n // 625 and pair.model.partial_rdofs == 0
        assert pair.model.temp_ts_corr_offset == 39 and pair.model.to_skip == 0
        ts += n
    # a chunk that leaves a partial slot, and the next one: to_skip = the missing part - 39 >= 0 clears the offset
    pair.pull(ts, 700)
    assert pair.model.partial_rdofs == 75 and pair.model.temp_ts_corr_offset == 39
    pair.pull(ts + 700, 1300)
    assert pair.model.temp_ts_corr_offset == 0 and pair.model.to_skip == 550 - 39


@pytest.mark.parametrize("fracts", [0, 1, 624])
@pytest.mark.parametrize("fullts", [0, 1, 7, 97])
def test_first_call_after_an_acquire(fracts, fullts):
    """ms_rx_lower.cpp:362-383 for fracts in {0, 1, 624}: fracts == 0 skips a whole slot.  The acquire sets the clock (fn, 0), mTSC
    and first_sch_ts_start = first_ts + start - 17."""
    pair = Pair()
    fn, start, t_acq = 51 * 40 + 21, 30_005, 777_000
    pair.acquire(fn, start, t_acq, bsic=0o56)
    st = pair.obj.state()
    assert pair.obj.clock() == (fn, 0, 0) and st["tsc"] == 0o56 & 7 and st["first_sch_ts_start"] == t_acq + start - 17
    assert st["first_call"] == 1 and st["carried"] == 0 and st["pending"] == 0
    first_ts = int(st["first_sch_ts_start"]) + fullts * 625 + fracts
    want = pair.pull(first_ts, 6000)
    assert pair.model.to_skip == 625 - fracts
    assert len(want) == (6000 - (625 - fracts)) // 625
    # the first slot cut, one slot behind first_ts rounded up, is labelled fullts + 1 slots behind the SCH burst's (fn, 0) -- and
    # only fullts with fracts == 0, where inc_both() is left out but a whole slot is skipped all the same (a quirk kept)
    k = fullts + (1 if fracts else 0)
    assert want[0][:3] == ((fn + k // 8) % SM.HYPERFRAME, k % 8, first_ts + 625 - fracts)
    run_stream(pair, [900, 5000, 700], first_ts + 6000)


def test_first_call_before_the_sch_burst():
    """first_ts in front of first_sch_ts_start: C's division truncates toward zero, fracts is negative and to_skip exceeds a slot"""
    pair = Pair()
    pair.acquire(51 * 9 + 1, 20_000, 0)
    first = 20_000 - 17
    assert pair.pull(first - 1000, 300) is None                    # to_skip = 625 + 375 leaves the chunk: refused
    want = pair.pull(first - 1000, 3000)
    assert pair.model.to_skip == 1000 and len(want) == 3


def test_a_chunk_shorter_than_the_missing_part_only_extends_the_partial_slot():
    pair = Pair(starts=lambda fn, tn, ts: -7)
    pair.set_clock(51 * 3, 6, 0)
    ts = 625
    pair.pull(ts, 700)                                             # (153, 7) cut, 75 samples carried
    ts += 700
    for n in (100, 1, 448):                                        # 550 are missing
        assert pair.pull(ts, n) == [] and pair.obj.clock()[:2] == (51 * 3, 7)
        ts += n
    assert pair.model.partial_rdofs == 624
    want = pair.pull(ts, 1)                                        # the last missing sample: the SCH slot (154, 0) is cut
    assert [w[:2] for w in want] == [(51 * 3 + 1, 0)] and want[0][3] == -624
    assert pair.model.temp_ts_corr_offset == 7 and pair.model.to_skip == 0 and pair.obj.state()["carried"] == 1   # 1 - 7 < 0: clamped
    with pytest.raises(trxhip.TrxHipError):
        pair.obj.plan(2)


def test_where_the_arithmetic_leaves_the_chunk_the_pull_is_refused():
    """to_skip > n_samples after the correction: the reference calls read_n with a negative count.  Refused with the state
    untouched; a longer chunk is accepted."""
    pair = Pair(starts=lambda fn, tn, ts: 39)
    pair.set_clock(51 * 3, 6, 0)
    pair.pull(625, 625 + 600)                                      # (153, 7); 600 carried
    ts = 625 + 1225
    assert pair.pull(ts, 30) is None                               # the SCH slot completes, to_skip = 25 + 39 > 30
    assert pair.pull(ts, 63) is None
    want = pair.pull(ts, 64)
    assert len(want) == 1 and pair.model.to_skip == 64 and pair.model.partial_rdofs == 0


def test_clock_jumps_are_counted_not_fatal():
    pair = Pair(tracking=False)
    pair.set_clock(100, 3, 0)
    pair.pull(625 + 400, 1250)                                     # diff = 1025 > 1.5 * 625
    pair.pull(625 + 400 + 1250, 1250)
    pair.pull(625 + 400 + 2500 - 400, 625)                         # diff = 225 < 0.5 * 625
    assert pair.obj.state()["clock_jumps"] == 2 == pair.model.tk.jumps


def test_the_hyperframe_wraps():
    pair = Pair()
    pair.set_clock(SM.HYPERFRAME - 1, 5, 0)
    want = pair.pull(625, 625 * 4)
    assert [w[:2] for w in want] == [(SM.HYPERFRAME - 1, 6), (SM.HYPERFRAME - 1, 7), (0, 0), (0, 1)]


def test_refusals_leave_the_state_untouched():
    L = trxhip.load_library()
    vp, sz = C.c_void_p, C.c_size_t

    def cfg(full=2047.0, tsc=0):
        return trxhip._MsSchedCfg(full, tsc, 0xFF, 1, 0)

    h = vp()
    for bad in (cfg(tsc=8), cfg(full=0.0), cfg(full=-1.0), cfg(full=float("inf")), cfg(full=float("nan"))):
        assert L.trxhip_ms_sched_create(None, C.byref(bad), C.byref(h)) == EINVAL
    assert L.trxhip_ms_sched_create(None, None, C.byref(h)) == EINVAL
    good = cfg()
    assert L.trxhip_ms_sched_create(None, C.byref(good), None) == EINVAL

    s = trxhip.MsRxScheduler(None, tsc=2)
    ns, nc = sz(), sz()
    pull16 = lambda n, ts=0, d_in=None, d_ind=None, d_bits=None: L.trxhip_ms_sched_pull_s16(    # noqa: E731
        s.h, d_in, n, ts, d_ind, d_bits, 0, C.byref(ns), C.byref(nc), None)
    assert pull16(700) == EINVAL                                   # before set_clock or a successful acquire
    fn, tn, ts = C.c_uint32(), C.c_int(), C.c_int64()
    assert L.trxhip_ms_sched_clock(s.h, C.byref(fn), C.byref(tn), C.byref(ts)) == EINVAL
    rec = np.zeros(1, dtype=trxhip.SCH_SYNC_DTYPE)
    assert L.trxhip_ms_sched_acquire_s16(s.h, None, 60000, 0, rec.ctypes.data_as(vp), None) == 0      # rc == 0: not found
    assert pull16(700) == EINVAL and s.state()["clock_set"] == 0
    for a in ((2715648, 0, 0), (5, 8, 0), (5, -1, 0)):
        assert L.trxhip_ms_sched_set_clock(s.h, *a) == EINVAL
    s.set_clock(5, 1, 0)
    s.pull(n_samples=700, first_ts=625)
    before = (s.state().tobytes(), s.clock(), s.plan().tobytes())

    def untouched():
        return (s.state().tobytes(), s.clock(), s.plan().tobytes()) == before

    buf = (C.c_int16 * 8)()
    assert pull16(0) == EINVAL and untouched()                     # n_samples == 0
    assert pull16(700, d_in=C.addressof(buf)) == EINVAL and untouched()     # a plan-only object takes no buffers
    assert pull16(700, d_ind=C.addressof(buf)) == EINVAL and pull16(700, d_bits=C.addressof(buf)) == EINVAL and untouched()
    assert L.trxhip_ms_sched_pull_cf32(s.h, None, 700, 0, None, None, 0, C.byref(ns), C.byref(nc), None) == EINVAL   # formats mixed
    assert untouched()
    assert L.trxhip_ms_sched_set_tsc(s.h, 8) == EINVAL and L.trxhip_ms_sched_set_tsc(s.h, -1) == EINVAL and untouched()
    assert L.trxhip_ms_sched_acquire_s16(s.h, None, 531, 0, rec.ctypes.data_as(vp), None) == EINVAL
    assert L.trxhip_ms_sched_acquire_s16(s.h, None, 60000, 0, None, None) == EINVAL and untouched()
    assert L.trxhip_ms_sched_plan(s.h, None, 1) == EINVAL and L.trxhip_ms_sched_state(s.h, None) == EINVAL
    assert L.trxhip_ms_sched_slots(None, 700) == EINVAL and L.trxhip_ms_sched_pull_s16(None, None, 700, 0, None, None, 0, None, None,
                                                                                      None) == EINVAL
    assert pull16(1300, ts=625 + 700) == 0 and ns.value == 2       # and the stream goes on
    # set_clock drops the carried partial slot and a pending correction
    s.feed_starts([39])
    s.set_clock(51 * 3, 7, 0)
    s.pull(n_samples=700, first_ts=625)
    assert (s.state()["pending"], s.state()["carried"]) == (-39, 75)
    s.set_clock(9, 2, 0)
    assert (s.state()["pending"], s.state()["carried"], s.state()["first_call"]) == (0, 0, 0)


def test_setters_take_effect_with_the_next_pull():
    s = trxhip.MsRxScheduler(None, tsc=1, active_tns=0x01, tracking=True)
    s.set_clock(51 * 3, 7, 0)
    s.pull(n_samples=1250, first_ts=625)
    p = s.plan()
    assert list(p["kind"]) == [trxhip.MS_KIND_SCH, trxhip.MS_KIND_NB] and list(p["flags"]) == [1, 0]
    s.set_active(0x0C)
    s.set_tracking(False)
    s.feed_starts([39] * 8)
    s.pull(n_samples=1250, first_ts=625 + 1250)
    assert list(s.plan()["flags"]) == [1, 1] and list(s.plan()["tn"]) == [2, 3]
    assert list(p["flags"]) == [1, 0] and s.state()["tracking"] == 0 and s.state()["active_tns"] == 0x0C


def test_header_wrapper_and_library_agree():
    L = trxhip.load_library()
    for name in ("create", "destroy", "set_clock", "clock", "set_tsc", "set_active", "set_tracking", "feed_starts", "acquire_s16",
                 "acquire_cf32", "slots", "pull_s16", "pull_cf32", "plan", "state"):
        assert hasattr(L, "trxhip_ms_sched_" + name) and "trxhip_ms_sched_" + name in trxhip.SYMBOLS
    import osmo_trx_amd
    assert osmo_trx_amd.MsRxScheduler is trxhip.MsRxScheduler


def test_loopback_precondition_on_the_cpu_models():
    """What tests/test_gpu_ms_sched.py's acquire -> pull loopback relies on, on the models alone (tests/ms_rx_model.py is pinned to
    the oracle): for LOOP's seed and the defaults of tests/ms_rx_cases.py (25 dB, amplitude 3000) the ACQ model finds the one SCH
    burst of the buffer, and the model receiver recovers all 148 bits of EVERY ACTIVE traffic slot the cutter cuts -- those in
    front of the first tracking correction too; the SCH slot decodes to the frame it is cut as."""
    x, sent = SC.loopback_stream()
    acq, out = SC.model_loopback(x)
    L = SC.LOOP
    assert (acq["fn"], acq["bsic"]) == (L["fn0"] + 7, L["bsic"]) and (L["fn0"] + 7) % 51 == 1
    traffic = [(fn, tn, m) for fn, tn, m in out if m["kind"] == RX.KIND_NB and m["sent"]]
    assert len(out) == (len(x) - L["acq_len"]) // 625 and len(traffic) == len(out) // 2
    for fn, tn, m in traffic:
        assert (L["active"] >> tn) & 1 and np.array_equal(m["bits"], K.hard(sent[(fn, tn)])), (fn, tn)
    sch = [(fn, m) for fn, tn, m in out if m["kind"] == RX.KIND_SCH]
    assert len(sch) == 1 and sch[0][1]["sch_rc"] == 1 and sch[0][1]["sch_fn"] == sch[0][0] and abs(sch[0][1]["start"]) > 1
