"""GPU tests of the MS-side receive gain control: the level kernel's three forms and the gain kernels against the literal model
(tests/ms_agc_model.py).  Everything is bit-equal: there is no tolerance anywhere in this feature."""
import numpy as np
import pytest

import ms_agc_model as AM
import ms_sched_cases as SC
from osmo_trx_amd import trxhip

pytestmark = pytest.mark.gpu

EINVAL = -22
F = np.float32


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def model_levels(rows):
    return np.array([AM.normed_abs_sum(r) for r in rows], dtype=np.float32)


def check_rows(trx, rows):
    """rows int16[n, len, 2]: the row form against the model, bit for bit"""
    got = trx.ms_level(dev(rows)).cpu().numpy()
    want = model_levels(rows)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    return got


# ---- the row form --------------------------------------------------------------------------------

def test_rows_plain_values(trx):
    rng = np.random.default_rng(11)
    rows = np.stack([np.zeros((625, 2), np.int16), rng.integers(-2047, 2048, (625, 2)).astype(np.int16),
                     np.full((625, 2), 32767, np.int16), np.full((625, 2), -32768, np.int16),
                     rng.integers(-2047, 2048, (625, 2)).astype(np.int16)])
    got = check_rows(trx, rows)
    assert got[0] == 0


def test_rows_around_2_24(trx):
    """total exactly 2^24 (the last exact one), then the first steps of the ordered path: 2^24 + 1 (a tie, to even: 2^24),
    2^24 + 3 in one value (a tie, to even: 2^24 + 4) and as 1 + 1 + 1 (each lost); the crossing at several places of a tile"""
    base = np.zeros((625, 2), np.int16)
    base[:256] = -32768                                            # 512 values of 32768: 2^24
    rows = []
    for extra in ([], [(1, 0)], [(3, 0)], [(1, 1), (1, 0)], [(0, 1)], [(2, 0)], [(1, 1), (1, 1), (5, -7)]):
        for shift in (0, 1, 37, 63, 64, 300):                      # zeros in front: the 2^24 is reached elsewhere in the tiles
            r = np.zeros((625, 2), np.int16)
            r[shift:shift + 256] = -32768
            for k, v in enumerate(extra):
                r[shift + 256 + k] = v
            rows.append(r)
    rows = np.stack(rows)
    got = check_rows(trx, rows)
    assert got[0] == F(1 << 24) / F(1250) and got[6] == got[0] and got[12] == F((1 << 24) + 4) / F(1250) and got[18] == got[0]
    # the small values FIRST: the integer prefix is still exact when the big ones come
    r = np.zeros((625, 2), np.int16)
    r[0] = (1, 1)
    r[1] = (1, 0)
    r[2:258] = -32768
    check_rows(trx, r[None])


def test_rows_full_scale_crosses_mid_row(trx):
    rng = np.random.default_rng(12)
    rows = rng.integers(-32768, 32768, (6, 625, 2)).astype(np.int16)
    tot = np.abs(rows.astype(np.int64)).sum(axis=(1, 2))
    assert (tot > 1 << 24).all()
    rows[5, :400] //= 4                                            # crosses late
    check_rows(trx, rows)


@pytest.mark.parametrize("row_len", [1, 2, 63, 64, 65, 625, 60000])
def test_rows_lengths(trx, row_len):
    rng = np.random.default_rng(100 + row_len)
    rows = np.stack([rng.integers(-32768, 32768, (row_len, 2)), rng.integers(-2047, 2048, (row_len, 2)),
                     rng.integers(-300, 301, (row_len, 2))]).astype(np.int16)
    check_rows(trx, rows)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_rows_any_sample_offset_odd_stride(trx, off):
    """rows are 4-byte aligned only: every head and tail length of the 16-byte loads comes by"""
    rng = np.random.default_rng(20 + off)
    for row_len, stride, amp in ((625, 627, 2047), (65, 67, 32767), (625, 629, 32767), (6, 7, 2047)):
        n = 9
        buf = rng.integers(-amp, amp + 1, (off + n * stride + 8, 2)).astype(np.int16)
        got = trx.ms_level(dev(buf)[off:], row_len=row_len, row_stride=stride, n_rows=n).cpu().numpy()
        want = model_levels([buf[off + r * stride:off + r * stride + row_len] for r in range(n)])
        assert np.array_equal(bits(got), bits(want)), (row_len, stride, off)


def test_rows_refusals(trx):
    import torch
    L = trx.L
    x = torch.zeros((700, 2), dtype=torch.int16, device="cuda:0")
    out = torch.full((4,), 7.0, dtype=torch.float32, device="cuda:0")
    for args in ((x.data_ptr(), 1, 0, 0), (x.data_ptr(), 1, 625, 624), (x.data_ptr() + 2, 1, 625, 625), (0, 1, 625, 625),
                 (x.data_ptr(), 1, (1 << 20) + 1, (1 << 20) + 1)):
        assert L.trxhip_ms_level_batch_i16(trx.h, args[0], args[1], args[2], args[3], out.data_ptr(), None) == EINVAL
    assert L.trxhip_ms_level_batch_i16(trx.h, x.data_ptr(), 0, 625, 625, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()


# ---- the stream form -------------------------------------------------------------------------------

def run_stream(trx, x, chunks, clock=None, acquire_len=0, fs=2047.0, rx_gain=30.0, tracking=True, tsc=0, active=0xFF):
    """the same pulls on an object with gain control on (levels returned) and on one with it off.  After every pull: indications
    and sbits byte-identical; d_level[k] = the row form = the model on the 625 samples plan()'s src_off names; agc_state() = the
    model.  Returns (the object, the model)."""
    import torch
    objs = [trxhip.MsRxScheduler(trx, rx_full_scale=fs, tsc=tsc, active_tns=active, tracking=tracking) for _ in range(2)]
    on, off = objs
    on.set_agc(True, rx_gain, levels=True)
    model = AM.Agc(fs, rx_gain)
    d_x = dev(x)
    at = 0
    if acquire_len:
        for o in objs:
            found, _ = o.acquire(d_x[:acquire_len], first_ts=1000)
            assert found
        at = acquire_len
    else:
        for o in objs:
            o.set_clock(*clock)
    AM.same_state(on.agc_state(), model.state())
    first_ts = 1000 + at if acquire_len else clock[2] + 625
    origin = first_ts - at                                         # the timestamp of x[0]
    for n in chunks:
        ind1, sb1, lv = on.pull(d_x[at:at + n], first_ts=first_ts)
        ind0, sb0 = off.pull(d_x[at:at + n], first_ts=first_ts)
        assert ind1.shape == ind0.shape and torch.equal(ind1, ind0) and torch.equal(sb1, sb0)
        assert on.state().tobytes() == off.state().tobytes() and on.clock() == off.clock()
        plan = on.plan()
        assert len(plan) == lv.shape[0] == ind1.shape[0]
        if len(plan):
            rows = np.stack([x[int(p["ts"]) - origin:int(p["ts"]) - origin + 625] for p in plan])
            assert [int(p["src_off"]) for p in plan] == [int(p["ts"]) - first_ts for p in plan]
            want = model_levels(rows)
            assert np.array_equal(bits(lv.cpu().numpy()), bits(want))
            assert np.array_equal(bits(trx.ms_level(dev(rows)).cpu().numpy()), bits(want))
            model.run(want)
        AM.same_state(on.agc_state(), model.state())
        at += n
        first_ts += n
    assert at <= len(x)
    return on, model


def test_stream_after_acquire(trx):
    """the loopback stream: a first pull after an acquire, straddling slots, a chunk shorter than the missing part, SCH slots the
    cutter follows (tracking on: the pull that demodulates a straddling SCH slot first measures it all the same)"""
    x, _ = SC.loopback_stream()
    L = SC.LOOP
    on, model = run_stream(trx, x, (7000, 3111, 50, 20, 625, 20000, 5001, 24000), acquire_len=L["acq_len"], tsc=L["tsc"],
                           active=L["active"])
    assert model.slots >= 90 and on.state()["sch_slots"] >= 1


def test_stream_windows_and_decisions(trx):
    """quiet slots (runmean ends below 2: the gain moves) and loud ones, windows that cross pulls, a pull of 330 slots (two
    decisions in one pull), a straddling SCH slot with tracking on, a chunk that only extends the partial slot"""
    rng = np.random.default_rng(31)
    n = 625 * 700
    x = rng.integers(-2047, 2048, (n, 2)).astype(np.int16)
    x[:625 * 160] = rng.integers(-1, 2, (625 * 160, 2))           # windows 0 and 2 are quiet, 1 and 3 loud
    x[625 * 320:625 * 480] = rng.integers(0, 2, (625 * 160, 2))
    chunks = (300, 625 * 4, 625 * 100 + 500, 20, 625 * 330, 625 * 60 + 105, 625 * 170, 33)
    on, model = run_stream(trx, x, chunks, clock=(51 * 3, 7, 0), rx_gain=58.0)   # slot 0 is (154, 0): an SCH slot, and it straddles
    st = on.agc_state()
    assert st["decisions"] == 4 and st["applied"] == 2 and st["rx_gain"] == 60.0 and [r["applied"] for r in st["ring"]] == [1, 0, 1, 0]


def test_stream_many_decisions_in_one_pull(trx):
    """one pull of 70 windows and a bit: more decisions than a wave has lanes, quiet windows among them (those move the gain; the
    decide kernel skips over the others), the ring holds the last 8"""
    rng = np.random.default_rng(34)
    n_slots = 160 * 70 + 37
    x = rng.integers(-600, 601, (625 * n_slots + 99, 2)).astype(np.int16)
    for w in (0, 3, 4, 62, 63, 64, 65, 68):
        x[625 * 160 * w:625 * 160 * (w + 1)] = 0                   # a silent window: runmean ends near -4.4, below 2
    on, model = run_stream(trx, x, (625 * 100 + 5, 625 * n_slots - 625 * 100 + 90), clock=(51 * 3 + 2, 5, 0), rx_gain=55.0, tracking=False)
    st = on.agc_state()
    assert st["decisions"] == 70 and len(st["ring"]) == 8 and st["slots"] == n_slots
    assert [r["applied"] for r in model.records] == [int(w in (0, 3, 4, 62, 63)) for w in range(70)] and st["rx_gain"] == 60.0   # 55 -> 60; 61 is refused (windows 64, 65, 68)


def test_stream_full_scale_radio(trx):
    """rxFullScale 32767 near clipping: every slot takes the ordered path"""
    rng = np.random.default_rng(32)
    x = rng.integers(-32768, 32768, (625 * 200, 2)).astype(np.int16)
    on, model = run_stream(trx, x, (625 * 3 + 1, 625 * 150 + 311, 625 * 40), clock=(51 * 3 + 2, 5, 0), fs=32767.0, tracking=False)
    assert on.agc_state()["decisions"] == 1 and model.records[0]["runmean"] > 32767 * 2 // 3


def test_stream_refusals_keep_the_state(trx):
    import torch
    rng = np.random.default_rng(33)
    x = dev(rng.integers(-2047, 2048, (625 * 12, 2)).astype(np.int16))
    s = trxhip.MsRxScheduler(trx, tracking=False)
    s.set_clock(10, 0, 0)
    s.set_agc(True, 30.0, levels=True)
    s.pull(x[:625 * 5 + 100], first_ts=625)
    before = (s.agc_state(), s.state().tobytes(), s.clock())
    xc = torch.zeros(625 * 3, dtype=torch.complex64, device="cuda:0")
    with pytest.raises(trxhip.TrxHipError):                        # a carried int16 partial slot AND gain control: refused either way
        s.pull(xc, first_ts=625 * 6 + 100)
    s2 = trxhip.MsRxScheduler(trx, tracking=False)                 # no partial slot: refused for gain control alone
    s2.set_clock(10, 0, 0)
    s2.set_agc(True, 30.0)
    b2 = (s2.agc_state(), s2.state().tobytes())
    with pytest.raises(trxhip.TrxHipError):
        s2.pull(xc, first_ts=625)
    assert (s2.agc_state(), s2.state().tobytes()) == b2
    ns, nc = trxhip.C.c_size_t(), trxhip.C.c_size_t()
    ind = torch.empty((8, 32), dtype=torch.uint8, device="cuda:0")
    rc = s.L.trxhip_ms_sched_pull_s16(s.h, x.data_ptr(), 625 * 6, 625 * 6 + 100, ind.data_ptr(), None, 2, trxhip.C.byref(ns),
                                      trxhip.C.byref(nc), None)    # out_slots too small
    assert rc == EINVAL and (s.agc_state(), s.state().tobytes(), s.clock()) == before
    s.set_agc(False, 30.0)                                         # off: complex64 pulls are taken again
    s.set_clock(10, 0, 0)
    s.pull(xc, first_ts=625)
    assert {**s.agc_state(), "enable": True} == before[0]


# ---- the group form ----------------------------------------------------------------------------------

def test_group_equals_single_objects(trx):
    """3 members, different chunk lengths and phases; member 1 has gain control off; member 2 has no chunk in one pull; one pull of
    330 slots on member 0; a refused pull (out_stride too small for member 0) leaves all three AGC states untouched"""
    import torch
    rng = np.random.default_rng(41)
    n = 3
    xs = [rng.integers(-2047, 2048, (625 * 560, 2)).astype(np.int16) for _ in range(n)]
    xs[0][:625 * 200] = rng.integers(-1, 2, (625 * 200, 2))
    d_xs = [dev(x) for x in xs]
    clocks = [(51 * 3, 7, 0), (51 * 5 + 9, 2, 0), (51 * 3 + 1, 6, 0)]
    tracking = [True, False, True]
    gains = [30.0, 11.0, 59.0]
    g = trxhip.MsRxSchedulerGroup(trx, n=n, tsc=[1, 2, 3], active_tns=[0xFF, 0x0F, 0xA5], tracking=tracking)
    singles = [trxhip.MsRxScheduler(trx, tsc=m + 1, active_tns=(0xFF, 0x0F, 0xA5)[m], tracking=tracking[m]) for m in range(n)]
    models = [AM.Agc(2047, gains[m]) for m in range(n)]
    for m in range(n):
        g.set_clock(m, *clocks[m])
        singles[m].set_clock(*clocks[m])
        if m != 1:
            g.set_agc(m, True, gains[m], levels=True)
            singles[m].set_agc(True, gains[m], levels=True)
    pulls = [(300, 625 * 2 + 7, 625 * 9 + 600), (625 * 4, 625, 0), (625 * 100 + 500, 40, 30), (625 * 330, 625 * 3, 625 * 165 + 1),
             (625 * 20 + 3, 625 * 200, 625 * 7), (625 * 90, 0, 625 * 150)]
    at = [0] * n
    ts = [625] * n
    for k, sizes in enumerate(pulls):
        chunks = [d_xs[m][at[m]:at[m] + sizes[m]] if sizes[m] else None for m in range(n)]
        if k == 2:                                                 # refused for member 0's 101 slots: nothing moves
            before = [(g.agc_state(m), g.state(m).tobytes(), g.clock(m)) for m in range(n)]
            with pytest.raises(trxhip.TrxHipError):
                g.pull(chunks, first_ts=ts, out_stride=50)
            assert g.bad_member == 0 and [(g.agc_state(m), g.state(m).tobytes(), g.clock(m)) for m in range(n)] == before
        res, ns, lvs = g.pull(chunks, first_ts=ts)
        for m in range(n):
            if not sizes[m]:
                assert ns[m] == 0
                continue
            out = singles[m].pull(chunks[m], first_ts=ts[m])
            assert torch.equal(res[m][0], out[0]) and torch.equal(res[m][1], out[1]), (k, m)
            assert g.state(m).tobytes() == singles[m].state().tobytes() and g.clock(m) == singles[m].clock()
            if m != 1:
                assert torch.equal(lvs[m], out[2]), (k, m)
                models[m].run(out[2].cpu().numpy())
            else:
                assert lvs[m] is None and len(out) == 2
            at[m] += sizes[m]
            ts[m] += sizes[m]
        for m in range(n):
            assert g.agc_state(m) == singles[m].agc_state(), (k, m)
            if m != 1:
                AM.same_state(g.agc_state(m), models[m].state())
    assert g.agc_state(0)["decisions"] >= 3 and g.agc_state(0)["applied"] >= 1 and g.agc_state(2)["decisions"] >= 2
    assert g.agc_state(1)["slots"] == 0 and not g.agc_state(1)["enable"]


# ---- acquire_gated -------------------------------------------------------------------------------------

def test_acquire_gated(trx):
    x, _ = SC.loopback_stream()
    L = SC.LOOP
    buf = x[:L["acq_len"]]
    level = AM.normed_abs_sum(buf)
    assert AM.gate(level, SC.FULL, 30.0)[0] == AM.SEARCH
    quiet = (buf // 16).astype(np.int16)
    assert AM.gate(AM.normed_abs_sum(quiet), SC.FULL, 30.0)[0] == AM.RAISE
    s = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL)
    s.set_agc(True, 30.0)
    before = (s.state().tobytes(), s.agc_state())
    assert s.acquire_gated(dev(quiet), first_ts=500) == (trxhip.RAISE, 34.0)
    assert (s.state().tobytes(), s.agc_state()) == before
    with pytest.raises(trxhip.TrxHipError):                        # no clock yet: nothing was acquired
        s.clock()
    assert s.acquire_gated(dev(quiet), first_ts=500, rx_gain=60.0)[0] in (False, True)     # rxgain >= 60: it searches
    ref = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL)
    s = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL)
    s.set_agc(True, 30.0)
    f0, r0 = ref.acquire(dev(buf), first_ts=500)
    f1, r1 = s.acquire_gated(dev(buf), first_ts=500)
    assert f0 and f1 is True and r0.tobytes() == r1.tobytes() and s.state().tobytes() == ref.state().tobytes() and s.clock() == ref.clock()
    # the group: member 0 below the gate, member 2 above it
    g = trxhip.MsRxSchedulerGroup(trx, n=3, rx_full_scale=SC.FULL)
    gb = (g.state(0).tobytes(), g.agc_state(0))
    found, rec, new = g.acquire_gated([0, 2], dev(np.stack([quiet, buf])), first_ts=[500, 500], rx_gain=30.0)
    assert list(found) == [False, True] and new == [34.0, None] and rec[1].tobytes() == r0.tobytes()
    assert (g.state(0).tobytes(), g.agc_state(0)) == gb and g.clock(2) == ref.clock()
