"""GPU tests of the MS-side NCO: the batch call against the numpy restatement byte for byte (tests/ms_nco_model.py, with the
library's own tables), the receiver's rotating instances against the composition "batch call, then the complex64 receiver" on the
single scheduler and on a group of three, the acquire path, what must not move (AFC, AGC), and the measure-then-correct loop on the
stream tests/test_ms_nco_cpu.py proves on the CPU models."""
import ctypes as C
import functools

import numpy as np
import pytest

import ms_nco_model as NM
import ms_sched_cases as SC
from osmo_trx_amd import trxhip

pytestmark = pytest.mark.gpu

EINVAL = -22
FULL = 2047.0
CANARY = 0xA5


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


@pytest.fixture(scope="module")
def tabs():
    return trxhip.ms_nco_tables_host()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")


def to_c64(x):
    return (x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)).astype(np.complex64)


# ---- 1. the batch call against the model ----------------------------------------------------------------------------------------

INCS = [0, 1, -1, 2 ** 31 - 1, -2 ** 31, NM.inc_of(2000.0), NM.inc_of(-2000.0)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 625, 60000])
def test_batch_equals_model(trx, tabs, n):
    import torch
    rng = np.random.default_rng(100 + n)
    rows = rng.integers(-32768, 32768, (len(INCS) + 1, n, 2)).astype(np.int16)
    rows[0, :min(n, 4)] = [[32767, -32768], [-32768, 32767], [0, 0], [-1, 1]][:min(n, 4)]
    phase0 = [int(p) for p in rng.integers(0, 2 ** 32, len(INCS))] + [0]
    incs = INCS + [0]                                               # the last row: the identity
    want = np.stack([NM.rotate(tabs, rows[r], phase0[r], incs[r]) for r in range(len(incs))])
    got = trx.ms_nco(dev(rows), phase0, incs)
    got_c = trx.ms_nco(dev(to_c64(rows)), phase0, incs)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert got_c.cpu().numpy().tobytes() == want.tobytes()
    # inc = 0 at phase 0 is convert_short_float
    assert want[-1].tobytes() == to_c64(rows[-1]).tobytes()


def test_batch_windows_and_refusals(trx, tabs):
    """rows at strides of their own from an odd sample on, canaries around and between the output rows; bad arguments"""
    import torch
    rng = np.random.default_rng(7)
    n, length, stride, ostride, off = 3, 65, 71, 70, 1
    buf = rng.integers(-32768, 32768, (off + n * stride, 2)).astype(np.int16)
    rec = np.zeros(n, dtype=trxhip.MS_NCO_ROW_DTYPE)
    rec["phase0"], rec["inc"] = [5, 2 ** 31, 77], [INCS[5], -3, 2 ** 31 - 1]
    d_buf, d_rec = dev(buf), dev(rec.view(np.uint8))
    out = torch.full((1 + n * ostride + 1, 8), CANARY, dtype=torch.uint8, device="cuda:0")
    L = trx.L
    assert L.trxhip_ms_nco_batch_i16(trx.h, d_buf.data_ptr() + 4 * off, stride, d_rec.data_ptr(), out.data_ptr() + 8, ostride, n, length, None) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[0] == CANARY).all() and (o[-1] == CANARY).all()
    body = o[1:-1].reshape(n, ostride, 8)
    assert (body[:, length:] == CANARY).all()
    for r in range(n):
        want = NM.rotate(tabs, buf[off + r * stride:off + r * stride + length], int(rec["phase0"][r]), int(rec["inc"][r]))
        assert body[r, :length].tobytes() == want.tobytes(), r
    i16, c32 = L.trxhip_ms_nco_batch_i16, L.trxhip_ms_nco_batch_cf32
    x, r_, o_ = d_buf.data_ptr(), d_rec.data_ptr(), out.data_ptr()
    out.fill_(CANARY)
    for fn, args in ((i16, (x + 2, 65, r_, o_, 65, 1, 65)), (i16, (0, 65, r_, o_, 65, 1, 65)), (i16, (x, 65, 0, o_, 65, 1, 65)),
                     (i16, (x, 65, r_, 0, 65, 1, 65)), (i16, (x, 64, r_, o_, 65, 1, 65)), (i16, (x, 65, r_, o_, 64, 1, 65)),
                     (i16, (x, 65, r_, o_, 65, 0, 65)), (i16, (x, 65, r_, o_, 65, 1, 0)), (i16, (x, 1 << 31, r_, o_, 1 << 31, 1, 1 << 31)),
                     (i16, (x, 65, r_ + 2, o_, 65, 1, 65)), (i16, (x, 65, r_, o_ + 4, 65, 1, 65)), (c32, (x + 4, 65, r_, o_, 65, 1, 65))):
        assert fn(trx.h, *args, None) == EINVAL, args
    assert i16(None, x, 65, r_, o_, 65, 1, 65, None) == EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all()


# ---- the streams of the scheduler tests ---------------------------------------------------------------------------------------------
# three frames of a cell from an FCCH frame on, every burst 6 samples late (the SCH slot's start moves the cut where tracking is on),
# on a carrier -hz off, so that the NCO at +hz is what lets the SCH slot decode

N = 24 * 625
BSIC = (0o53, 0o21, 0o76)
HZ = (2000.0, 2000.0, -270000.0)           # member 0 of the group has the NCO off
T0 = (2 ** 40 - 5000, 123456, 2 ** 32 - 8000)
ACTIVE = (0b01100110, 0xFF, 0b00010001)
# one piece; 625 k + r (a correction lies between a straddling slot and its chunk); pieces shorter than a slot; a straddling SCH slot
CHUNKINGS = ((N,), (625 * 9 + 100, 625 * 6 + 33, 625 * 9 - 133), (300, 200, 125, 625 * 3 + 10, 400, 215, 625 * 19),
             (625 * 8 + 300, 625 * 2, 625 * 14 - 300))


@functools.lru_cache(maxsize=None)
def member_stream(m):
    x, _ = SC.cell_stream(8800 + m, 51 * (30 + m), 3, BSIC[m], tsc=BSIC[m] & 7, late=6)
    x = NM.to_i16(NM.carrier(x, -HZ[m]))
    x.setflags(write=False)
    return x


def start_clock(o, m, member=None):
    args = (51 * (30 + m) - 1, 7, T0[m] - 625)
    o.set_clock(*args) if member is None else o.set_clock(member, *args)


def rotated(trx, x, nco, ts):
    """the batch call over x whose first sample has the timestamp ts: complex64 device tensor"""
    return trx.ms_nco(dev(x)[None], [nco.phase(ts) if nco.enable else 0], [nco.inc if nco.enable else 0])[0]


def st(rec):
    """state() without the format of the carried partial slot: the object under test takes int16 where its yardstick takes complex64"""
    rec = rec.copy()
    rec["carried_cf32"] = 0
    return rec.tobytes()


def same_pull(a, b):
    import torch
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("chunks", CHUNKINGS, ids=["one", "625k+r", "short", "sch-straddle"])
def test_single_pull_equals_composition(trx, chunks):
    assert sum(chunks) == N
    x = member_stream(0)
    decoded = 0
    for tracking in (True, False):
        for c64 in (False, True):
            on, ref = (trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=BSIC[0] & 7, active_tns=ACTIVE[0], tracking=tracking) for _ in range(2))
            nco = NM.Nco()
            for o in (on, ref):
                start_clock(o, 0)
            on.set_nco(True, HZ[0])
            nco.set(True, HZ[0], on.clock()[2])
            assert on.nco_state() == nco.state() and ref.nco_state()["enable"] is False
            d_in = dev(to_c64(x) if c64 else x)
            d_rot = rotated(trx, x, nco, T0[0])
            at = 0
            for n in chunks:
                a = on.pull(d_in[at:at + n], first_ts=T0[0] + at)
                b = ref.pull(d_rot[at:at + n], first_ts=T0[0] + at)
                same_pull(a, b)
                assert on.plan().tobytes() == ref.plan().tobytes() and on.clock() == ref.clock()
                assert st(on.state()) == st(ref.state()) and on.carried == ref.carried
                ind = on.ind_to_numpy(a[0])
                decoded += int(ind["sch_rc"].sum())
                assert (np.abs(ind["start"][ind["sch_rc"] == 1]) > 1).all()    # a start the cutter follows where tracking is on
                at += n
            assert on.nco_state() == nco.state()                   # pulls do not move it
    assert decoded == 4                                            # the stream's one SCH slot, in all four runs


def test_single_set_between_pulls(trx):
    """another frequency between two pulls, where no partial slot is carried: the phase goes on from where it was"""
    x = member_stream(0)
    on, ref = (trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=BSIC[0] & 7, active_tns=0xFF, tracking=False) for _ in range(2))
    nco = NM.Nco()
    for o in (on, ref):
        start_clock(o, 0)
    on.set_nco(True, HZ[0])
    nco.set(True, HZ[0], on.clock()[2])
    d_in, at = dev(x), 0
    for k, n in enumerate((625 * 5, 625 * 7 + 200, 625 * 12 - 200)):
        if k == 1:
            assert on.carried == 0
            on.set_nco(True, -67708.33)
            nco.set(True, -67708.33, on.clock()[2])
            assert on.nco_state() == nco.state() and nco.acc != 0
        d_rot = rotated(trx, x[at:], nco, T0[0] + at)
        same_pull(on.pull(d_in[at:at + n], first_ts=T0[0] + at), ref.pull(d_rot[:n], first_ts=T0[0] + at))
        assert st(on.state()) == st(ref.state()) and on.clock() == ref.clock()
        at += n
    # off again: the receiver is the one it was
    on.set_nco(False)
    for o in (on, ref):
        start_clock(o, 0)
    same_pull(on.pull(d_in[:625 * 4], first_ts=T0[0]), ref.pull(d_in[:625 * 4], first_ts=T0[0]))


GROUP_CHUNKS = (((625 * 9 + 100, 625 * 6 + 33, 625 * 9 - 133), (N, None, None), (300, 625 * 8 + 300, 625 * 15 + 25)),
                ((625 * 8 + 300, 625 * 2, 625 * 14 - 300), (625 * 8 + 300, 625 * 2, 625 * 14 - 300), (None, 625 * 10 + 1, 625 * 14 - 1)))


@pytest.mark.parametrize("chunks", GROUP_CHUNKS, ids=["mixed", "sch-straddle"])
def test_group_pull_equals_composition(trx, chunks):
    xs = [member_stream(m) for m in range(3)]
    for tracking in (True, False):
        for c64 in (False, True):
            mk = lambda: trxhip.MsRxSchedulerGroup(trx, 3, rx_full_scale=FULL, tsc=[b & 7 for b in BSIC], active_tns=list(ACTIVE),
                                                   tracking=tracking)
            on, ref = mk(), mk()
            ncos = [NM.Nco() for _ in range(3)]
            for m in range(3):
                for o in (on, ref):
                    start_clock(o, m, member=m)
                if m:
                    on.set_nco(m, True, HZ[m])
                    ncos[m].set(True, HZ[m], on.clock(m)[2])
                assert on.nco_state(m) == ncos[m].state()
            d_in = [dev(to_c64(x) if c64 else x) for x in xs]
            d_rot = [rotated(trx, xs[m], ncos[m], T0[m]) for m in range(3)]
            at = [0, 0, 0]
            for k in range(3):
                sizes = [chunks[m][k] for m in range(3)]
                cut = lambda d: [d[m][at[m]:at[m] + sizes[m]] if sizes[m] else None for m in range(3)]
                ts = [T0[m] + at[m] for m in range(3)]
                ra, na = on.pull(cut(d_in), first_ts=ts)
                rb, nb = ref.pull(cut(d_rot), first_ts=ts)
                assert na == nb and on.carried == ref.carried
                for m in range(3):
                    same_pull(ra[m], rb[m])
                    assert on.plan(m).tobytes() == ref.plan(m).tobytes() and on.clock(m) == ref.clock(m)
                    assert st(on.state(m)) == st(ref.state(m))
                at = [a + (n or 0) for a, n in zip(at, sizes)]
            assert at == [N, N, N]
            assert [on.nco_state(m) for m in range(3)] == [o.state() for o in ncos]


# ---- 3. on at 0 Hz from creation: the rotating instance is the identity ---------------------------------------------------------------

def test_zero_hz_equals_off(trx):
    x = member_stream(1)
    d_in = dev(x)
    on, off = (trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=BSIC[1] & 7, active_tns=0xFF, tracking=True) for _ in range(2))
    on.set_nco(True, 0.0)
    for o in (on, off):
        start_clock(o, 1)
    at = 0
    for n in CHUNKINGS[1]:
        same_pull(on.pull(d_in[at:at + n], first_ts=T0[1] + at), off.pull(d_in[at:at + n], first_ts=T0[1] + at))
        assert st(on.state()) == st(off.state()) and on.plan().tobytes() == off.plan().tobytes()
        at += n
    assert on.nco_state() == dict(enable=True, inc=0, acc=0, ts_ref=0, hz=0.0)
    mk = lambda: trxhip.MsRxSchedulerGroup(trx, 3, rx_full_scale=FULL, tsc=BSIC[1] & 7, active_tns=0xFF, tracking=True)
    g_on, g_off = mk(), mk()
    for m in range(3):
        g_on.set_nco(m, m != 1, 0.0)                               # (member 1 rides along with it off)
        for g in (g_on, g_off):
            start_clock(g, 1, member=m)
    at = 0
    for n in CHUNKINGS[3]:
        ts = T0[1] + at
        ra, na = g_on.pull([d_in[at:at + n]] * 3, first_ts=ts)
        rb, nb = g_off.pull([d_in[at:at + n]] * 3, first_ts=ts)
        assert na == nb
        for m in range(3):
            same_pull(ra[m], rb[m])
            assert st(g_on.state(m)) == st(g_off.state(m))
        at += n


# ---- 4. AFC and AGC read the stream as received ---------------------------------------------------------------------------------------

def test_afc_and_agc_do_not_see_the_nco(trx):
    import torch
    x = member_stream(0)
    d_in = dev(x)
    objs, fcs = [], []
    for nco_on in (True, False):
        s = trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=BSIC[0] & 7, active_tns=0xFF, tracking=False)
        fc = torch.full((26, 32), CANARY, dtype=torch.uint8, device="cuda:0")
        s.set_afc(True, out=fc)
        s.set_agc(True, 30.0, levels=True)
        start_clock(s, 0)
        if nco_on:
            s.set_nco(True, HZ[0])
        objs.append(s)
        fcs.append(fc)
    at, differs = 0, False
    for n in CHUNKINGS[1]:
        res = [o.pull(d_in[at:at + n], first_ts=T0[0] + at) for o in objs]
        assert torch.equal(res[0][2], res[1][2])                   # the slots' levels
        assert torch.equal(fcs[0], fcs[1])
        differs = differs or not torch.equal(res[0][1], res[1][1])
        a, b = (o.afc_state() for o in objs)
        assert a["count"] == b["count"] and a["ring"] == b["ring"] and a["last"].tobytes() == b["last"].tobytes()
        assert objs[0].agc_state() == objs[1].agc_state()
        at += n
    assert differs and objs[0].afc_state()["count"] == 1           # the receiver did see it


# ---- 5. acquire -------------------------------------------------------------------------------------------------------------------------

def test_acquire_equals_composition(trx):
    import torch
    x, _ = SC.loopback_stream()
    L = SC.LOOP
    buf = NM.to_i16(NM.carrier(x[:L["acq_len"]], -HZ[0]))
    t0 = 2 ** 40 + 17
    nco = NM.Nco()
    nco.set(True, HZ[0], 0)                                        # no clock yet: the setting acts at ts 0
    want = None
    for how in ("s16", "cf32", "gated"):
        on, ref = (trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=0, active_tns=L["active"], tracking=True) for _ in range(2))
        on.set_nco(True, HZ[0])
        assert on.nco_state() == nco.state()
        d_rot = rotated(trx, buf, nco, t0)
        fb, rb = ref.acquire(d_rot, first_ts=t0)
        if how == "gated":
            level = trx.ms_level(dev(buf)[None]).item()
            fa, ra = on.acquire_gated(dev(buf), first_ts=t0, rx_gain=30.0)
            assert level == trx.ms_level(dev(buf)[None]).item()    # the gate's level: the raw int16 buffer, whatever the NCO
        else:
            fa, ra = on.acquire(dev(to_c64(buf) if how == "cf32" else buf), first_ts=t0)
        assert fa is True and fb is True and ra.tobytes() == rb.tobytes()
        assert on.clock() == ref.clock() and st(on.state()) == st(ref.state())
        assert on.nco_state() == nco.state()                       # acquire leaves it alone
        want = rb if want is None else want
        assert rb.tobytes() == want.tobytes()
    quiet = (np.random.default_rng(1).integers(-20, 21, (L["acq_len"], 2))).astype(np.int16)
    assert on.acquire_gated(dev(quiet), first_ts=t0, rx_gain=30.0) == (trxhip.RAISE, 34.0)
    # the group: members 2 and 0 in one call, member 2 with the NCO on, member 0 riding along with it off
    g_on, g_ref = (trxhip.MsRxSchedulerGroup(trx, 3, rx_full_scale=FULL, tracking=True) for _ in range(2))
    g_on.set_nco(2, True, HZ[0])
    bufs = np.stack([buf, buf])
    ts = [t0, 5]
    rot = trx.ms_nco(dev(bufs), [nco.phase(t0), 0], [nco.inc, 0])
    fa, ra = g_on.acquire([2, 0], dev(bufs), first_ts=ts)
    fb, rb = g_ref.acquire([2, 0], rot, first_ts=ts)
    assert list(fa) == list(fb) and fa[0] and ra.tobytes() == rb.tobytes()
    fa, ra, gains = g_on.acquire_gated([2, 0], dev(bufs), first_ts=ts, rx_gain=30.0)
    assert list(fa) == list(fb) and ra.tobytes() == rb.tobytes() and gains == [None, None]
    for m in (0, 2):
        assert st(g_on.state(m)) == st(g_ref.state(m))
    assert g_on.clock(2) == g_ref.clock(2)
    torch.cuda.synchronize()


# ---- 6. the loop --------------------------------------------------------------------------------------------------------------------

def test_measure_then_correct_loop(trx):
    x, sent = NM.loop_stream()
    d_x = dev(x)

    def make():
        s = trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=NM.LOOP_TSC, active_tns=NM.LOOP_ACTIVE, tracking=True)
        s.set_afc(True)
        s.set_clock(NM.LOOP_FN0 - 1, 7, -625)
        return s

    def traffic(ind, sb, fn0_slot):
        """[(signs equal the sent bits)] of the ACTIVE traffic slots of a pull"""
        ind, sb, out = trxhip.MsRxScheduler.ind_to_numpy(ind), sb.cpu().numpy(), []
        for k, r in enumerate(ind):
            key = (int(r["fn"]), int(r["tn"]))
            if r["kind"] == trxhip.MS_KIND_NB and key in sent:
                out.append(bool(((sb[k] < 0) == (sent[key] > 0)).all()))
        return ind, out

    # NCO off: as the model says, nothing is received
    s = make()
    ind, ok = traffic(*s.pull(d_x, first_ts=0), 0)
    sch = ind[ind["kind"] == trxhip.MS_KIND_SCH]
    assert len(sch) == 1 and sch["sch_rc"].sum() == 0 and len(ok) == len(sent) and not any(ok)
    # measure on the first frame, set, receive the rest
    s = make()
    s.pull(d_x[:5000], first_ts=0)
    hz = float(s.afc_state()["last"]["hz"])
    assert abs(hz - trxhip.MS_FCCH_BIAS_HZ - NM.LOOP_CFO) <= 100.0
    s.set_nco(True, trxhip.nco_hz_from_fcch(hz))
    ind, ok = traffic(*s.pull(d_x[5000:], first_ts=5000), 8)
    sch = ind[ind["kind"] == trxhip.MS_KIND_SCH]
    assert [(int(r["sch_rc"]), int(r["sch_fn"]), int(r["sch_bsic"])) for r in sch] == [(1, NM.LOOP_FN0 + 1, NM.LOOP_BSIC)]
    assert len(ok) == sum(1 for fn, _ in sent if fn > NM.LOOP_FN0) >= 6 and all(ok)
    assert s.afc_state()["count"] == 1


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals(trx):
    s = trxhip.MsRxScheduler(trx, rx_full_scale=FULL)
    g = trxhip.MsRxSchedulerGroup(trx, 3, rx_full_scale=FULL)
    s.set_nco(True, 1000.0)
    before = s.nco_state()
    for hz in (500000.1, -500000.1, float("nan"), float("inf")):
        with pytest.raises(trxhip.TrxHipError):
            s.set_nco(True, hz)
        with pytest.raises(trxhip.TrxHipError):
            g.set_nco(1, True, hz)
    s.set_nco(True, 500000.0)
    s.set_nco(True, 1000.0)
    assert {**s.nco_state(), "ts_ref": 0} == {**before, "ts_ref": 0}
    cfg = trxhip._MsNcoCfg(1, 0, 100.0)
    a = np.zeros(1, dtype=trxhip.MS_NCO_STATE_DTYPE)
    L = trx.L
    assert L.trxhip_ms_nco_sched_set(s.h, None) == EINVAL and L.trxhip_ms_nco_group_set(g.h, 0, None) == EINVAL
    assert L.trxhip_ms_nco_sched_state(s.h, None) == EINVAL
    assert L.trxhip_ms_nco_group_set(g.h, 3, C.byref(cfg)) == EINVAL
    assert L.trxhip_ms_nco_group_state(g.h, 3, a.ctypes.data_as(C.c_void_p)) == EINVAL
    assert L.trxhip_ms_nco_sched_set(None, C.byref(cfg)) == EINVAL
    assert [g.nco_state(m)["enable"] for m in range(3)] == [False] * 3
    # a refused group pull names its member and moves no oscillator
    g.set_nco(2, True, 100.0)
    x = dev(member_stream(0)[:1250])
    with pytest.raises(trxhip.TrxHipError):
        g.pull([x, x, x], first_ts=0)                              # no clock is set
    assert g.bad_member == 0 and g.nco_state(2) == dict(enable=True, inc=NM.inc_of(100.0), acc=0, ts_ref=0, hz=100.0)
