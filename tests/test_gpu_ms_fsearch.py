"""GPU tests of the MS-side FCCH search (include/trxhip.h, "MS-side FCCH search"): the batch call against the numpy
restatement (tests/ms_fsearch_model.py) -- int16 rows to the byte, complex64 rows under the derived bar --, the measurement behind it
against trxhip_ms_fcch_batch_*, acquire_afc against the composition of the four public steps on the single object and on a group of
three, the cold start that the parent cannot do, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import ms_fsearch_cases as FC
import ms_fsearch_model as FM
from osmo_trx_amd import trxhip

pytestmark = pytest.mark.gpu

EINVAL = -22
FULL = FC.FULL
CANARY = 0xA5
MIN_SCORE = trxhip.MS_FSEARCH_MIN_SCORE
SEAM = FM.SEG * FM.HOP                     # 4096: the first sample of a row's second segment


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")


def clk(o, *m):
    """the object's (or member m's) clock, None while it has none"""
    try:
        return o.clock(*m)
    except trxhip.TrxHipError:
        return None


def search(trx, rows, **kw):
    return trx.fsearch_to_numpy(*trx.ms_fcch_search(dev(rows), **kw))


def same_hit_i16(got, x, min_score=MIN_SCORE):
    """pos, found and the five sums to the byte, the score within 4 ulp of the model's double"""
    want = FM.search(x, min_score)
    assert got["pos"] == want["pos"] and got["found"] == want["found"] and got["reserved"] == 0, (got, want)
    for k in FM.SUMS:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert abs(float(got["score"]) - float(want["score"])) <= 4 * np.spacing(abs(float(want["score"]))), (got["score"], want["score"])
    return want


def same_fcch(trx, got, x, pos):
    """the measurement: the bytes of trxhip_ms_fcch_batch_* on the slot at pos, zeros where the row ends before pos + 625"""
    want = trx.ms_fcch(dev(FM.slot_at(x, pos))[None], rx_full_scale=FULL)[0]
    assert got.tobytes() == want.tobytes(), (got, want)


def noise(n, amp, seed):
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(size=(n, 2)) * amp).clip(-32768, 32767).astype(np.int16)


# ---- 1. the batch call, int16 -----------------------------------------------------------------------------------------------------

# one window; one window with samples behind the last whole block; two windows; a segment one window short, full, full with ignored
# samples, two segments; the acquire buffer
LENGTHS = [584, 599, 600, SEAM + 560 + 8 - 1, SEAM + 560 + 8, SEAM + 560 + 8 + 15, SEAM + 560 + 8 + 16, 60000]


def rows_of(n):
    """int16[5, n, 2]: a tone somewhere, a tone at 10 dB on another carrier, noise alone, random full-range samples, a piece of a cell"""
    rng = np.random.default_rng(n)
    at = int(rng.integers(0, max(n - 600, 1)))
    cell = FC.cell(21, 25.0, 2000.0, 12, 137)[0]
    lo = int(rng.integers(0, len(cell) - n + 1))
    return np.stack([FC.tone_row(n, at, seed=n), FC.tone_row(n, n // 3, cfo=-40000.0, noise=10.0, seed=n + 1), noise(n, 300.0, n + 2),
                     rng.integers(-32768, 32768, (n, 2)).astype(np.int16), cell[lo:lo + n]])


@pytest.mark.parametrize("n", LENGTHS)
def test_i16_rows_equal_the_model(trx, n):
    rows = rows_of(n)
    hits, fcch = search(trx, rows, rx_full_scale=FULL)
    for r in range(len(rows)):
        want = same_hit_i16(hits[r], rows[r])
        same_fcch(trx, fcch[r], rows[r], int(want["pos"]))


def test_i16_strided_rows_and_canaries(trx):
    """eight rows of 584 at a stride of 640 from an odd sample on: what lies between the rows is a loud clean tone that would win
    every search and move every measurement if it were read; canaries round d_hit and d_fcch"""
    import torch
    n, length, stride, off = 8, 584, 640, 3
    loud = FC.tone_row(off + n * stride + 700, -50, amp=30000.0, noise=60.0, length=10 ** 6)
    buf = loud.copy()
    rows = np.stack([FC.tone_row(length, 0, amp=500.0 + 100 * r, noise=15.0, seed=50 + r) if r % 2 == 0 else noise(length, 200.0, 60 + r)
                     for r in range(n)])
    for r in range(n):
        buf[off + r * stride:off + r * stride + length] = rows[r]
    d_buf = dev(buf)
    d_hit = torch.full((n + 2, 64), CANARY, dtype=torch.uint8, device="cuda:0")
    d_fc = torch.full((n + 2, 32), CANARY, dtype=torch.uint8, device="cuda:0")
    rc = trx.L.trxhip_ms_fcch_search_i16(trx.h, d_buf.data_ptr() + 4 * off, stride, length, n, MIN_SCORE, FULL, d_hit.data_ptr() + 64,
                                         d_fc.data_ptr() + 32, None)
    assert rc == 0
    torch.cuda.synchronize()
    h, f = d_hit.cpu().numpy(), d_fc.cpu().numpy()
    assert (h[0] == CANARY).all() and (h[-1] == CANARY).all() and (f[0] == CANARY).all() and (f[-1] == CANARY).all()
    hits, fcch = h[1:-1].reshape(-1).view(trxhip.MS_FCCH_HIT_DTYPE), f[1:-1].reshape(-1).view(trxhip.MS_FCCH_DTYPE)
    for r in range(n):
        want = same_hit_i16(hits[r], rows[r])
        assert want["pos"] == 0
        same_fcch(trx, fcch[r], rows[r], 0)                        # the row ends at 584: zeros behind it, not the loud tone
    assert torch.equal(d_buf.cpu(), torch.from_numpy(buf))
    # d_fcch == NULL: the hits alone
    d_hit.fill_(CANARY)
    assert trx.L.trxhip_ms_fcch_search_i16(trx.h, d_buf.data_ptr() + 4 * off, stride, length, n, MIN_SCORE, FULL, d_hit.data_ptr() + 64,
                                           None, None) == 0
    torch.cuda.synchronize()
    assert d_hit.cpu().numpy()[1:-1].tobytes() == h[1:-1].tobytes()


def test_i16_seams_first_and_last_window(trx):
    """the burst where its best window is the last of a segment, the first of the next, straddles the seam's sample, is the row's
    first and the row's last grid window"""
    n = 3 * SEAM + 592 + 8                                         # 16 k + 8: the last window ends 8 samples before the row does
    last = FM.HOP * (FM.n_windows(n) - 1)
    ats = [SEAM - 16, SEAM, SEAM - 288, 2 * SEAM - 8, 0, n - 584]
    # a tone of 584 samples holds one grid window whole: which window is the best is not left to the noise
    rows = np.stack([FC.tone_row(n, at, noise=50.0, seed=70 + i, length=584) for i, at in enumerate(ats)])
    hits, fcch = search(trx, rows, rx_full_scale=FULL)
    for r, at in enumerate(ats):
        want = same_hit_i16(hits[r], rows[r])
        same_fcch(trx, fcch[r], rows[r], int(want["pos"]))
        assert want["found"] == 1 and abs(int(want["pos"]) - min(at, last)) <= 16, (at, want["pos"])
    assert hits[0]["pos"] // FM.HOP == FM.SEG - 1 and hits[1]["pos"] // FM.HOP == FM.SEG and hits[2]["pos"] == SEAM - 288
    assert hits[4]["pos"] == 0 and hits[5]["pos"] == last


def test_i16_tie_zero_and_full_scale_rows(trx):
    n = 5000                                                       # two segments: the tie rule carries across them
    rows = np.stack([FC.tie_row(n), np.zeros((n, 2), np.int16)] + [FC.rails_row(n, k) for k in ("min", "max", "alt", "mix")])
    hits, fcch = search(trx, rows, rx_full_scale=FULL)
    for r in range(len(rows)):
        want = same_hit_i16(hits[r], rows[r])
        same_fcch(trx, fcch[r], rows[r], int(want["pos"]))
    assert hits[0]["pos"] == 0 and hits[0]["found"] == 1           # every window of the tie row has the same bits
    z = hits[1]
    assert z["found"] == 0 and z["pos"] == 0 and z["score"] == 0.0 and all(z[k] == 0 for k in FM.SUMS)
    assert hits[2]["energy"] == 576.0 * 2 ** 31 and hits[2]["ra_re"] == 288.0 * 2 ** 31     # past int32 in every term's sum


# ---- 2. the batch call, complex64 -------------------------------------------------------------------------------------------------

def c64_rows():
    """complex64 rows of one length, chosen so that the model's best window beats every other by more than the bar can move it:
    the int16 rows' tones and cell pieces as floats, and the same at other scales"""
    n = SEAM + 560 + 8 + 16 + 300
    base = [FC.tone_row(n, 1000, seed=1), FC.tone_row(n, SEAM - 290, cfo=80000.0, noise=10.0, seed=2), FC.tone_row(n, n - 592, seed=3),
            FC.cell(21, 25.0, 2000.0, 12, 137)[0][:n], FC.cell(22, 10.0, -40000.0, 12, 137)[0][50000 - 2000:50000 - 2000 + n],
            noise(n, 300.0, 5)]
    rows = [FC.to_c64(x) for x in base]
    rows += [(rows[0] * np.float32(1.0 / 2047.0)).astype(np.complex64), (rows[3] * np.float32(1e-4)).astype(np.complex64),
             (rows[1] * np.complex64(3e3 * np.exp(0.7j))).astype(np.complex64)]
    return np.stack(rows)


def test_c64_rows_are_decided_on_the_cpu():
    """the model alone: on every row of the set the best window stands above all others by more than the bar moves a score"""
    for r, x in enumerate(c64_rows()):
        assert FM.score_margin(x) > 0, r


def test_c64_rows_under_the_bar(trx):
    rows = c64_rows()
    hits, fcch = search(trx, rows, rx_full_scale=FULL)
    worst = 0.0
    for r, x in enumerate(rows):
        w = FM.windows(x)
        want = FM.search(x, MIN_SCORE, w)
        assert hits[r]["pos"] == want["pos"] and hits[r]["found"] == want["found"], (r, hits[r], want)
        j, S = int(want["pos"]) // FM.HOP, FM.bars(x)
        for k in FM.SUMS:
            err, bar = abs(float(hits[r][k]) - float(want[k])), FM.BAR * float(S[k][j])
            worst = max(worst, err / bar)
            assert err <= bar, (r, k, err, bar)
        same_fcch(trx, fcch[r], x, int(want["pos"]))
    print(f"complex64 sums: the largest error is {worst:.3f} of the bar")
    assert hits[:3]["found"].all() and not hits[5]["found"]
    # zeros, and a row that is not finite: NaN scores count as 0, so pos 0 and not found
    odd = np.zeros((2, 700), np.complex64)
    odd[1, 100] = np.nan
    hits, _ = search(trx, odd)
    assert (hits["pos"] == 0).all() and (hits["found"] == 0).all() and (hits["score"] == 0).all()


# ---- 3. acquire_afc is the composition of the four public steps -----------------------------------------------------------------

REST = 2 * 8 * FC.SLOT                     # two frames behind the acquire buffer, for the pull that follows


def member_buf(m):
    """(stream, acquire buffer) of member 0: on frequency, 1: +2000 Hz, 2: a cell whose FCCH slots hold noise"""
    x = FC.cell(31 + m, 25.0, (0.0, 2000.0, 0.0)[m], 14, 0, 0xFF, m != 2)[0]
    return x, x[:FC.ACQ_LEN]


def as_input(x, c64):
    return dev(FC.to_c64(x) if c64 else x)


@pytest.mark.parametrize("c64", [False, True], ids=["int16", "complex64"])
def test_single_acquire_afc_equals_composition(trx, c64):
    import torch
    for m in range(3):
        x, buf = member_buf(m)
        on, ref = (trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=FC.TSC, active_tns=0x0F, tracking=True) for _ in range(2))
        fresh = ref.state().tobytes(), clk(ref), ref.nco_state()
        for o in (on, ref):
            o.set_nco(True, 777.0)                                 # already on: the search still reads the buffer as received
        d_buf, t0 = as_input(buf, c64), 2 ** 33 + 5
        found, rec, hit, fc = on.acquire_afc(d_buf, first_ts=t0)
        # the four steps
        hits, fcch = trx.fsearch_to_numpy(*trx.ms_fcch_search(d_buf[None], rx_full_scale=FULL))
        assert hit.tobytes() == hits[0].tobytes() and fc.tobytes() == fcch[0].tobytes()
        if m == 2:
            assert not hits[0]["found"] and (found, rec) == (False, None)
        else:
            assert hits[0]["found"]
            ref.set_nco(True, trxhip.nco_hz_from_fcch(fcch[0]["hz"]))
            f2, r2 = ref.acquire(d_buf, first_ts=t0)
            assert found is True and f2 is True and rec.tobytes() == r2.tobytes() and rec["bsic"] == FC.BSIC
        assert on.nco_state() == ref.nco_state() and on.state().tobytes() == ref.state().tobytes() and clk(on) == clk(ref)
        if m == 2:
            assert (on.state().tobytes(), clk(on)) == fresh[:2] and on.nco_state()["hz"] == 777.0
            continue
        d_rest = as_input(x[FC.ACQ_LEN:FC.ACQ_LEN + REST], c64)
        a, b = (o.pull(d_rest, first_ts=t0 + FC.ACQ_LEN) for o in (on, ref))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert on.state().tobytes() == ref.state().tobytes() and clk(on) == clk(ref)


@pytest.mark.parametrize("c64,order", [(False, (0, 1, 2)), (False, (2, 0, 1)), (False, (0, 2, 1)), (True, (1, 2, 0))],
                         ids=["int16-012", "int16-201", "int16-021", "complex64-120"])
def test_group_acquire_afc_equals_composition(trx, c64, order):
    """members 0 and 1 are found (one run or two, by the order), member 2 is not: untouched, h_found 0"""
    import torch
    streams = [member_buf(m) for m in range(3)]
    on, ref = (trxhip.MsRxSchedulerGroup(trx, 3, rx_full_scale=FULL, tsc=FC.TSC, active_tns=[0x0F, 0xFF, 0x33], tracking=True) for _ in range(2))
    fresh = [(ref.state(m).tobytes(), clk(ref, m), ref.nco_state(m)) for m in range(3)]
    members = list(order)
    bufs = as_input(np.stack([streams[m][1] for m in members]), c64)
    ts = [10 ** 6 * (m + 1) + 7 for m in members]
    found, rec, hit, fc = on.acquire_afc(members, bufs, first_ts=ts)
    hits, fcch = trx.fsearch_to_numpy(*trx.ms_fcch_search(bufs, rx_full_scale=FULL))
    assert hit.tobytes() == hits.tobytes() and fc.tobytes() == fcch.tobytes()
    go = [i for i in range(3) if hits[i]["found"]]
    assert [members[i] for i in go] == [m for m in members if m != 2]
    for i in go:
        ref.set_nco(members[i], True, trxhip.nco_hz_from_fcch(fcch[i]["hz"]))
    f2, r2 = ref.acquire([members[i] for i in go], bufs[go].contiguous(), first_ts=[ts[i] for i in go])
    assert list(found[go]) == list(f2) == [True, True] and rec[go].tobytes() == r2.tobytes()
    assert not found[members.index(2)] and rec[members.index(2)].tobytes() == bytes(24)
    for m in range(3):
        assert on.nco_state(m) == ref.nco_state(m) and on.state(m).tobytes() == ref.state(m).tobytes() and clk(on, m) == clk(ref, m)
    assert (on.state(2).tobytes(), clk(on, 2), on.nco_state(2)) == fresh[2]
    assert abs(on.nco_state(1)["hz"] + 2000.0) <= 100.0 and abs(on.nco_state(0)["hz"]) <= 100.0
    chunks = [as_input(streams[m][0][FC.ACQ_LEN:FC.ACQ_LEN + REST], c64) if m != 2 else None for m in range(3)]
    t1 = [10 ** 6 * (m + 1) + 7 + FC.ACQ_LEN for m in range(3)]
    (ra, na), (rb, nb) = (o.pull(chunks, first_ts=t1) for o in (on, ref))
    assert na == nb
    for m in (0, 1):
        assert torch.equal(ra[m][0], rb[m][0]) and torch.equal(ra[m][1], rb[m][1])
        assert on.state(m).tobytes() == ref.state(m).tobytes() and clk(on, m) == clk(ref, m)


# ---- 4. the cold start ---------------------------------------------------------------------------------------------------------------

COLD_CFO = 2000.0


def cold_stream():
    """24 frames like ms_nco_model.loop_stream -- an FCCH burst, an SCH burst a frame later, traffic on TN 1 .. 3 -- on a carrier
    2000 Hz off: the acquire buffer of 60000 samples and 12 frames behind it"""
    return FC.cell(7301, 25.0, COLD_CFO, 24, 0, 0x0F)


def test_cold_start_cpu_models_say_plain_acquire_finds_nothing():
    import ms_sched_cases as SC
    import sch_sync_model as SS
    x = cold_stream()[0]
    assert SS.sch_sync(x[:FC.ACQ_LEN], SS.ACQ, SC.SCALE)["rc"] == 0
    on = FC.cell(7301, 25.0, 0.0, 24, 0, 0x0F)[0]                  # the same cell on frequency is acquired
    assert SS.sch_sync(on[:FC.ACQ_LEN], SS.ACQ, SC.SCALE)["rc"] == 1


def test_cold_start(trx):
    x, starts, sent = cold_stream()
    d_x = dev(x)
    make = lambda: trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=FC.TSC, active_tns=0x0F, tracking=True)
    # the receiver alone: the carrier is too far off
    found, _ = make().acquire(d_x[:FC.ACQ_LEN], first_ts=0)
    assert found is False
    # search, measure, set, acquire
    s = make()
    found, rec, hit, fc = s.acquire_afc(d_x[:FC.ACQ_LEN], first_ts=0)
    print(f"cold start: pos {int(hit['pos'])} score {float(hit['score']):.4f} fcch hz {float(fc['hz']):.1f} nco {s.nco_state()['hz']:.1f}")
    assert hit["found"] == 1 and min(abs(int(hit["pos"]) - k) for k in starts) <= 32
    assert found is True and rec["rc"] == 1 and rec["bsic"] == FC.BSIC and rec["fn"] in (FC.FN0 + 1, FC.FN0 + 11)
    assert s.nco_state()["enable"] and abs(s.nco_state()["hz"] + COLD_CFO) <= 100.0
    # the rest of the stream through the NCO it set
    ind, sb = s.pull(d_x[FC.ACQ_LEN:], first_ts=FC.ACQ_LEN)[:2]
    ind, sb = trxhip.MsRxScheduler.ind_to_numpy(ind), sb.cpu().numpy()
    sch = ind[ind["kind"] == trxhip.MS_KIND_SCH]
    assert [(int(r["sch_rc"]), int(r["sch_fn"]), int(r["sch_bsic"])) for r in sch] == [(1, FC.FN0 + 21, FC.BSIC)]
    ok = [bool(((sb[k] < 0) == (sent[(int(r["fn"]), int(r["tn"]))] > 0)).all()) for k, r in enumerate(ind)
          if r["kind"] == trxhip.MS_KIND_NB and (int(r["fn"]), int(r["tn"])) in sent]
    assert len(ok) >= 11 * 3 and all(ok)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------

def test_batch_refusals(trx):
    import torch
    n = 600
    d_buf = dev(FC.tone_row(2 * n + 8, 0))
    d_hit = torch.full((4, 64), CANARY, dtype=torch.uint8, device="cuda:0")
    d_fc = torch.full((4, 32), CANARY, dtype=torch.uint8, device="cuda:0")
    x, h, f = d_buf.data_ptr(), d_hit.data_ptr(), d_fc.data_ptr()
    i16, c32 = trx.L.trxhip_ms_fcch_search_i16, trx.L.trxhip_ms_fcch_search_cf32
    good = (x, n, n, 2, MIN_SCORE, FULL, h, f)
    assert i16(trx.h, *good, None) == 0
    torch.cuda.synchronize()
    d_hit.fill_(CANARY)
    d_fc.fill_(CANARY)

    def bad(**kw):
        names = ("iq", "stride", "len", "n", "score", "full", "hit", "fc")
        a = dict(zip(names, good))
        a.update(kw)
        return tuple(a[k] for k in names)

    inf, nan = float("inf"), float("nan")
    for args in (bad(len=583, stride=583), bad(len=1 << 31, stride=1 << 31), bad(stride=n - 1), bad(n=0), bad(score=0.0), bad(score=-0.1),
                 bad(score=1.0000001), bad(score=nan), bad(score=inf), bad(full=0.0), bad(full=-1.0), bad(full=inf), bad(full=nan),
                 bad(iq=0), bad(hit=0), bad(iq=x + 2), bad(hit=h + 4), bad(fc=f + 4)):
        assert i16(trx.h, *args, None) == EINVAL, args
    assert c32(trx.h, *bad(iq=x + 4), None) == EINVAL
    assert i16(None, *good, None) == EINVAL
    assert i16(trx.h, *bad(score=1.0), None) == 0 and i16(trx.h, *bad(score=1.0, fc=0), None) == 0      # the ends of the ranges
    torch.cuda.synchronize()
    hit = d_hit.cpu().numpy()
    assert (hit[2:] == CANARY).all() and (d_fc.cpu().numpy()[2:] == CANARY).all()
    d_hit.fill_(CANARY)
    for args in (bad(score=0.0), bad(iq=x + 2)):
        assert i16(trx.h, *args, None) == EINVAL
    torch.cuda.synchronize()
    assert (d_hit.cpu().numpy() == CANARY).all() and (d_fc.cpu().numpy()[2:] == CANARY).all()


def test_scheduler_refusals_change_nothing(trx):
    bufs = dev(np.stack([member_buf(0)[1], member_buf(1)[1]]))
    g = trxhip.MsRxSchedulerGroup(trx, 3, rx_full_scale=FULL, tracking=True)
    g.set_nco(1, True, 50.0)
    snap = lambda: [(g.state(m).tobytes(), clk(g, m), g.nco_state(m)) for m in range(3)]
    before = snap()
    L, p = trx.L, bufs.data_ptr()
    members = lambda *m: np.array(m, dtype=np.uint32)
    ts = np.array([0, 0, 0], dtype=np.int64)
    out = dict(hit=np.full(3, CANARY, dtype=np.uint8).repeat(64), fc=np.full(3, CANARY, dtype=np.uint8).repeat(32),
               rec=np.full(3, CANARY, dtype=np.uint8).repeat(24), found=np.full(3, -7, dtype=np.int32))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(mem, n, buf, stride, length, score, fn=L.trxhip_ms_afc_group_acquire_s16):
        return fn(g.h, ptr(mem), n, buf, stride, length, ptr(ts), score, ptr(out["hit"]), ptr(out["fc"]), ptr(out["rec"]), ptr(out["found"]), None)

    n = FC.ACQ_LEN
    for args in ((members(0, 0), 2, p, n, n, MIN_SCORE),           # a member listed twice
                 (members(0, 3), 2, p, n, n, MIN_SCORE),           # no such member
                 (members(0, 1), 0, p, n, n, MIN_SCORE), (members(0, 1, 2, 0), 4, p, n, n, MIN_SCORE),
                 (members(0, 1), 2, None, n, n, MIN_SCORE), (members(0, 1), 2, p + 2, n, n, MIN_SCORE), (members(0, 1), 2, p, n - 1, n, MIN_SCORE),
                 (members(0, 1), 2, p, 500, 500, MIN_SCORE),       # acquire's shortest buffer is 532
                 (members(0, 1), 2, p, 560, 560, MIN_SCORE),       # the search's is 584
                 (members(0, 1), 2, p, n, n, 0.0), (members(0, 1), 2, p, n, n, 1.5), (members(0, 1), 2, p, n, n, float("nan"))):
        assert call(*args) == EINVAL, args[1:]
    assert call(members(0, 1), 2, p + 4, n, n, MIN_SCORE, L.trxhip_ms_afc_group_acquire_cf32) == EINVAL
    assert L.trxhip_ms_afc_group_acquire_s16(None, ptr(members(0)), 1, p, n, n, ptr(ts), MIN_SCORE, None, None, None, None, None) == EINVAL
    assert snap() == before
    assert (out["hit"] == CANARY).all() and (out["fc"] == CANARY).all() and (out["rec"] == CANARY).all() and (out["found"] == -7).all()
    s = trxhip.MsRxScheduler(trx, rx_full_scale=FULL)
    one = (s.state().tobytes(), clk(s), s.nco_state())
    for score in (0.0, 2.0):
        with pytest.raises(trxhip.TrxHipError):
            s.acquire_afc(bufs[0], first_ts=0, min_score=score)
    with pytest.raises(trxhip.TrxHipError):
        s.acquire_afc(bufs[0][:560], first_ts=0)
    assert (s.state().tobytes(), clk(s), s.nco_state()) == one
    # every output is optional
    assert L.trxhip_ms_afc_group_acquire_s16(g.h, ptr(members(1, 0)), 2, p, n, n, ptr(ts), MIN_SCORE, None, None, None, None, None) == 2
    assert g.nco_state(0)["enable"] and abs(g.nco_state(0)["hz"] + 2000.0) <= 100.0 and clk(g, 1) != before[1][1]
