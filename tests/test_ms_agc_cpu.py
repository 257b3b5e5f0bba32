"""CPU tests of the MS-side receive gain control (trxhip_ms_agc_*): the model's own quirks (tests/ms_agc_model.py, the literal
restatement of normed_abs_sum(), maybe_update_gain() and the level gate), and the plan-only single object and group, fed levels,
against the model record by record.  Everything is bit-equal; no GPU is opened."""
import ctypes as C
import re

import numpy as np
import pytest

import ms_agc_model as AM
from osmo_trx_amd import trxhip

EINVAL = -22
F = np.float32


def levels_for(seed, n, fs=2047):
    """n slot levels in regimes of 160: near silence (runmean ends below 2: the gain moves), ordinary, above the cutoff"""
    rng = np.random.default_rng(seed)
    out = np.empty(n, dtype=np.float32)
    for w in range(0, n, 160):
        kind = rng.integers(0, 3)
        hi = (0.02, fs / 4, fs)[kind]
        out[w:w + 160] = rng.uniform(0, hi, size=len(out[w:w + 160])).astype(np.float32)
    return out


# ---- the model's own quirks ---------------------------------------------------------------------

def test_model_offset_is_a_bool():
    """gain moves by +1 only when runmean < 2, never down, and never above 60"""
    for level, moved in ((0.0, True), (0.3, True), (1.4, False), (100.0, False), (2000.0, False)):
        a = AM.Agc(2047, 30)
        a.run([level] * 160)
        r = a.records[0]
        assert len(a.records) == 1 and (r["runmean"] < 2) == moved
        assert r["new_gain"] == 30 + moved and r["applied"] == moved and a.rxgain == 30 + moved
        assert a.runmean == 0 and a.gain_check == 0
    a = AM.Agc(2047, 59)
    a.run([0.0] * 480)
    assert [(r["old_gain"], r["new_gain"], r["applied"]) for r in a.records] == [(59, 60, 1), (60, 61, 0), (60, 61, 0)]
    # the recurrence is not a mean: runmean_k = runmean_{k-1} + (sum_k - 1) / (k + 2), up to rounding
    a = AM.Agc(2047, 30)
    a.run([100.0] * 159)
    assert abs(a.runmean - (100 + 99 * sum(1.0 / (k + 2) for k in range(1, 159)))) < 0.05


def test_model_gate_boundary():
    assert AM.gate(255.0, 2047, 30) == (AM.RAISE, 34.0)            # sum == target_val: not above
    assert AM.gate(np.nextafter(F(255), F(256)), 2047, 30) == (AM.SEARCH, 30.0)
    assert AM.gate(256.0, 2047, 30) == (AM.SEARCH, 30.0)
    assert AM.gate(0.0, 2047, 60) == (AM.SEARCH, 60.0) and AM.gate(0.0, 2047, 59.5) == (AM.RAISE, 63.5)
    assert AM.gate(4095.0, 32767, 0) == (AM.RAISE, 4.0) and AM.gate(4096.0, 32767, 0) == (AM.SEARCH, 0.0)


def test_model_sequential_sum_is_the_integer_total_up_to_2_24():
    rng = np.random.default_rng(5)
    for n, amp in ((625, 2047), (625, 13000), (1, 32767), (63, 32767), (255, 32767)):
        for _ in range(8):
            x = rng.integers(-amp, amp + 1, size=(n, 2)).astype(np.int16)
            total = int(np.abs(x.astype(np.int64)).sum())
            assert total <= 1 << 24
            assert AM.normed_abs_sum(x) == F(total) / F(2 * n)
    x = np.full((256, 2), -32768, dtype=np.int16)                  # exactly 2^24; abs(-32768) is 32768
    assert AM.normed_abs_sum(x) == F(32768)
    # ... and not above it: 2^24 + 1 is a tie that rounds to even
    y = np.concatenate([x, np.array([[1, 0]], dtype=np.int16)])
    assert AM.normed_abs_sum(y) == F(1 << 24) / F(514)


# ---- the product's gate ---------------------------------------------------------------------------

def test_gate_equals_model():
    for fs in (2047.0, 32767.0, 1.0, 7.0):
        t = int(fs) // 8
        for level in (0.0, t - 1.0, float(t), float(np.nextafter(F(t), F(1e9))), t + 1.0, 40000.0):
            for gain in (0.0, 30.0, 56.0, 59.9, 60.0, 61.0):
                assert trxhip.ms_agc_gate(level, fs, gain) == AM.gate(level, fs, gain), (fs, level, gain)
    new = C.c_float()
    L = trxhip.load_library()
    assert L.trxhip_ms_agc_gate(1.0, -1.0, 30.0, C.byref(new)) == EINVAL
    assert L.trxhip_ms_agc_gate(float("nan"), 2047.0, 30.0, C.byref(new)) == EINVAL
    assert L.trxhip_ms_agc_gate(1.0, 2047.0, 30.0, None) == EINVAL


# ---- plan-only objects against the model ------------------------------------------------------------

class Single:
    """a plan-only single object with gain control on, and the model, side by side"""

    def __init__(self, rx_gain=30.0, fs=2047.0, seed=1, n_levels=4000):
        self.obj = trxhip.MsRxScheduler(None, rx_full_scale=fs, tracking=False)
        self.obj.set_clock(51 * 3, 7, 0)
        self.obj.set_agc(True, rx_gain)
        self.model = AM.Agc(fs, rx_gain)
        self.levels = levels_for(seed, n_levels, int(fs))
        self.pos, self.ts = 0, 625

    def pull(self, n):
        bound = self.obj.slots(n)
        self.obj.feed_levels(self.levels[self.pos:self.pos + bound])
        ns, _ = self.obj.pull(n_samples=n, first_ts=self.ts)
        assert ns == bound
        self.model.run(self.levels[self.pos:self.pos + ns])
        self.pos += ns
        self.ts += n
        AM.same_state(self.obj.agc_state(), self.model.state())
        return ns


def test_single_object_equals_model():
    s = Single()
    # windows that cross pulls, a chunk that only extends the partial slot, two decisions in one pull (>= 320 slots), one slot
    for n in (625 * 100, 300, 200, 625 * 59 + 125, 625 * 2, 625 * 330 + 7, 618, 625, 625 * 161, 100, 625 * 800):
        s.pull(n)
    st = s.obj.agc_state()
    assert st["enable"] and st["decisions"] == s.pos // 160 >= 9 and len(st["ring"]) == 8 and 0 < st["applied"] < st["decisions"]
    assert [r["slot"] for r in st["ring"]] == [160 * (st["decisions"] - 8 + k) + 159 for k in range(8)]


def test_gain_stops_at_60_and_set_gain():
    s = Single(rx_gain=58.0)
    s.levels[:] = 0.0
    s.pull(625 * 640)
    st = s.obj.agc_state()
    assert st["rx_gain"] == 60.0 and st["applied"] == 2 and st["decisions"] == 4 and st["ring"][-1]["new_gain"] == 61.0
    s.obj.agc_set_gain(12.5)
    s.model.rxgain = F(12.5)
    assert s.obj.agc_state()["rx_gain"] == 12.5
    s.pull(625 * 170)
    assert s.obj.agc_state()["rx_gain"] == 13.5


def test_clock_and_acquire_keep_the_agc_state():
    s = Single()
    s.pull(625 * 100)
    before = s.obj.agc_state()
    assert before["gain_check"] == 100 and before["runmean"] != 0
    s.obj.set_clock(77, 3, 10 ** 6)
    assert s.obj.agc_state() == before
    rec = np.zeros(1, dtype=trxhip.SCH_SYNC_DTYPE)[0]
    rec["rc"], rec["start"], rec["fn"] = 1, 100, 52
    assert s.obj.acquire(first_ts=2 * 10 ** 6, result=rec)[0]
    assert s.obj.agc_state() == before
    s.obj.set_agc(False, before["rx_gain"])                         # off: pulls measure nothing, the state stays
    s.obj.set_clock(51 * 3, 7, 0)
    s.obj.pull(n_samples=625 * 10, first_ts=625)
    after = s.obj.agc_state()
    assert not after["enable"] and {**after, "enable": True} == before


def test_refused_pull_moves_nothing():
    s = Single()
    s.pull(625 * 150 + 3)
    before = (s.obj.agc_state(), s.obj.state().tobytes(), s.obj.clock())
    L, ns, nc = s.obj.L, C.c_size_t(), C.c_size_t()
    # fewer levels fed than slots cut
    s.obj.feed_levels(s.levels[:19])
    assert L.trxhip_ms_sched_pull_s16(s.obj.h, None, 625 * 20, s.ts, None, None, 0, C.byref(ns), C.byref(nc), None) == EINVAL
    assert (s.obj.agc_state(), s.obj.state().tobytes(), s.obj.clock()) == before
    # a complex64 pull with gain control on
    s.obj.feed_levels(s.levels[:40])
    assert L.trxhip_ms_sched_pull_cf32(s.obj.h, None, 625 * 20, s.ts, None, None, 0, C.byref(ns), C.byref(nc), None) == EINVAL
    assert (s.obj.agc_state(), s.obj.state().tobytes(), s.obj.clock()) == before
    # n_samples == 0
    assert L.trxhip_ms_sched_pull_s16(s.obj.h, None, 0, s.ts, None, None, 0, C.byref(ns), C.byref(nc), None) == EINVAL
    assert (s.obj.agc_state(), s.obj.state().tobytes(), s.obj.clock()) == before
    # a plan-only object takes no level array; a bad gain
    cfg = trxhip._MsAgcCfg(1, 30.0, 0x1000)
    assert L.trxhip_ms_agc_sched_set(s.obj.h, C.byref(cfg)) == EINVAL
    assert L.trxhip_ms_agc_sched_set_gain(s.obj.h, float("inf")) == EINVAL
    assert (s.obj.agc_state(), s.obj.state().tobytes(), s.obj.clock()) == before
    s.pull(625 * 20)                                               # and the same pull, fed, goes through


def test_group_equals_single_objects():
    """4 members: different gains and chunk lengths, member 2 with gain control off, member 1 without a chunk in some pulls, two
    decisions in one pull on member 0; a refused pull in between (out_stride too small for member 3) moves no member"""
    n = 4
    g = trxhip.MsRxSchedulerGroup(None, n, tracking=False)
    singles = [Single(rx_gain=30.0 + 7 * m, seed=10 + m) for m in range(n)]
    for m in range(n):
        g.set_clock(m, 51 * 3, 7, 0)
        if m != 2:
            g.set_agc(m, True, 30.0 + 7 * m)
    ts = [625] * n
    pulls = [(625 * 100, 625 * 3 + 9, 625 * 5, 625 * 161), (625 * 330 + 1, 0, 100, 300), (624, 625 * 200, 0, 625 * 40 + 325),
             (625 * 70, 0, 625, 625 * 2), (625 * 200, 616 + 625 * 118, 625 * 4, 10)]
    for k, sizes in enumerate(pulls):
        for m in range(n):
            if sizes[m] and m != 2:
                g.feed_levels(m, singles[m].levels[singles[m].pos:singles[m].pos + g.slots(m, sizes[m])])
        if k == 2:                                                 # refused: nothing moves, no level is consumed
            before = [(g.agc_state(m), g.state(m).tobytes()) for m in range(n)]
            with pytest.raises(trxhip.TrxHipError):
                g.pull(n_samples=list(sizes), first_ts=ts, out_stride=40)
            assert g.bad_member == 1 and [(g.agc_state(m), g.state(m).tobytes()) for m in range(n)] == before
        ns, _ = g.pull(n_samples=list(sizes), first_ts=ts)
        for m in range(n):
            if not sizes[m]:
                assert ns[m] == 0
            elif m != 2:
                assert singles[m].pull(sizes[m]) == ns[m]
            ts[m] += sizes[m]
            if m != 2:
                assert g.agc_state(m) == singles[m].obj.agc_state()
                AM.same_state(g.agc_state(m), singles[m].model.state())
    off = g.agc_state(2)
    assert not off["enable"] and off["slots"] == 0 and off["decisions"] == 0
    assert g.agc_state(0)["decisions"] >= 4 and g.agc_state(3)["decisions"] >= 1


def test_header_wrapper_and_library_agree():
    L = trxhip.load_library()
    hdr = open(trxhip.os.path.join(trxhip.os.path.dirname(trxhip.PKG), "include", "trxhip.h")).read()
    names = ["trxhip_ms_level_batch_i16", "trxhip_ms_agc_gate"] + \
        ["trxhip_ms_agc_%s_%s" % (o, f) for o in ("sched", "group") for f in ("set", "set_gain", "state", "feed_levels")]
    for name in names:
        assert hasattr(L, name) and name in trxhip.SYMBOLS and name + "(" in hdr, name
    assert L.trxhip_abi_version() == 5
    assert ["%d" % trxhip.MS_AGC_RING] == re.findall(r"#define TRXHIP_MS_AGC_RING\s+(\d+)", hdr) and trxhip.MS_AGC_STATE_DTYPE.itemsize == 304
    for cls in (trxhip.MsRxScheduler, trxhip.MsRxSchedulerGroup):
        for f in ("set_agc", "agc_set_gain", "agc_state", "feed_levels", "acquire_gated"):
            assert hasattr(cls, f)
    assert hasattr(trxhip.TrxHip, "ms_level")
