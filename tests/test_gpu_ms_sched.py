"""GPU tests of the MS-side downlink slot scheduler (trxhip_ms_sched_*, osmo_trx_amd.MsRxScheduler).

Every comparison is equality.  The stream form of the receiver is the row receiver's body on the same 625 samples, so its
indication records and sbits must equal trxhip_ms_rx_batch_*() byte for byte; the cutter is integer arithmetic, so plan, clock,
to_skip and pending correction must equal the literal model (tests/ms_sched_model.py) fed with the device's own SCH starts."""
import ctypes as C

import numpy as np
import pytest

import ms_rx_cases as K
import ms_sched_cases as SC
import ms_sched_model as SM
from osmo_trx_amd import trxhip

pytestmark = pytest.mark.gpu

EINVAL = -22
FN0 = 51 * 600                                                     # the streams begin with a 51-multiframe
ACTIVE = 0b11011011


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


@pytest.fixture(scope="module")
def stream():
    """2 x 51 frames x 8 slots = 816 slots (int16): SCH, noise-only FCCH, traffic on TSC fn % 8; bursts at their slots' starts"""
    return SC.cell_stream(4000, FN0, 102, bsic=0o31)[0]


@pytest.fixture(scope="module")
def late_stream():
    """the same cell with every burst 3 samples late"""
    return SC.cell_stream(4001, FN0, 102, bsic=0o31, tsc=1, late=3)[0]


def _dev(x, cf32):
    import torch
    if cf32:
        return torch.from_numpy((x[:, 0].astype(np.float32) + 1j * x[:, 1].astype(np.float32)).astype(np.complex64)).to("cuda:0")
    return torch.from_numpy(x).to("cuda:0")


def _chunks(total, sizes):
    """(start, length) over `total` samples, cycling through sizes"""
    at, k, out = 0, 0, []
    while at < total:
        n = min(sizes[k % len(sizes)], total - at)
        out.append((at, n))
        at, k = at + n, k + 1
    return out


def _pull_all(s, d_x, chunks, t0=0, tsc_of=None):
    """Pull the chunks; returns (ind records, sbits, plan records with `pos` = where each slot begins in the stream, per-pull
    (n_slots, state, clock))."""
    ind, bits, plan, pos, tscs, per = [], [], [], [], [], []
    for k, (at, n) in enumerate(chunks):
        if tsc_of is not None:
            s.set_tsc(tsc_of(k))
        i, b = s.pull(d_x[at:at + n], first_ts=t0 + at)
        p = s.plan()
        assert len(p) == i.shape[0] == b.shape[0]
        ind.append(trxhip.MsRxScheduler.ind_to_numpy(i))
        bits.append(b.cpu().numpy())
        plan.append(p)
        pos.append(at + p["src_off"].astype(np.int64))
        tscs.append(np.full(len(p), s.state()["tsc"], dtype=np.uint8))
        per.append((len(p), s.state(), s.clock()))
    return np.concatenate(ind), np.concatenate(bits), np.concatenate(plan), np.concatenate(pos), np.concatenate(tscs), per


def _rows(trx, d_x, pos, plan, tscs):
    """the row receiver on the slots the plan names, gathered into rows, with the plan's records"""
    import torch
    idx = torch.from_numpy(pos).to("cuda:0")[:, None] + torch.arange(625, device="cuda:0")[None, :]
    rows = d_x[idx].contiguous()
    slots = np.zeros(len(plan), dtype=trxhip.MS_SLOT_DTYPE)
    slots["fn"], slots["tn"], slots["tsc"], slots["flags"] = plan["fn"], plan["tn"], tscs, plan["flags"]
    return trx.ms_rx(rows, slots, rx_full_scale=SC.FULL)


IDENTITY_CHUNKINGS = [[510000], [5300], [700, 6000, 625, 1250, 4999], [60000, 100, 200, 400, 64000]]


@pytest.mark.parametrize("cf32", [False, True])
@pytest.mark.parametrize("tracking", [False, True])
def test_identity_with_the_row_receiver(trx, stream, cf32, tracking):
    """Every indication byte and every sbit of a pulled slot equals trxhip_ms_rx_batch_*() on the same 625 samples with the plan's
    {fn, tn, tsc, ACTIVE} -- for the slots read in the chunk, for the straddling slot, with the TSC changed between pulls."""
    d_x = _dev(stream, cf32)
    for sizes in IDENTITY_CHUNKINGS:
        s = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL, tsc=0, active_tns=ACTIVE, tracking=tracking)
        s.set_clock(FN0 - 1, 7, -625)
        ind, bits, plan, pos, tscs, per = _pull_all(s, d_x, _chunks(len(stream), sizes), tsc_of=lambda k: k % 8)
        assert len(plan) >= 815 - 2 and s.state()["clock_jumps"] == 0
        rec, rbits = _rows(trx, d_x, pos, plan, tscs)
        assert ind.tobytes() == rec.tobytes() and np.array_equal(bits, rbits)
        assert np.array_equal(ind["kind"], plan["kind"]) and np.array_equal(ind["sent"] == 1, (plan["flags"] == 1) & (plan["kind"] != 0))
        sch = ind["kind"] == trxhip.MS_KIND_SCH
        assert sch.sum() == 10 and (ind["sch_rc"][sch] == 1).all() and np.array_equal(ind["sch_fn"][sch], plan["fn"][sch])
        if len(sizes) > 1:
            assert (plan["src_off"] < 0).any()                     # straddling slots were among them
        s.close()


@pytest.mark.parametrize("cf32", [False, True])
def test_chunking_invariance_with_tracking_off(trx, late_stream, cf32):
    """Any chunking equals one pull, a chunk that only extends the partial slot included."""
    d_x = _dev(late_stream, cf32)
    one = None
    for sizes in ([510000], [5300], [700, 100, 6000, 50, 1, 625], [99, 1234]):
        s = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL, tsc=1, active_tns=ACTIVE, tracking=False)
        s.set_clock(FN0 - 1, 7, -625)
        ind, bits, plan, pos, _, per = _pull_all(s, d_x, _chunks(len(late_stream), sizes))
        st = s.state()
        assert (st["pending"], st["clock_jumps"]) == (0, 0)
        if len(sizes) > 2:
            assert any(n == 0 for n, _, _ in per)                  # pulls that cut nothing
        if one is None:
            one = (ind.tobytes(), bits.tobytes(), _labels(plan), s.clock())
            # the receiver's zero lies 2 samples behind a burst's first sample: bursts 3 samples late report 5, give or take the noise
            assert len(ind) == 816 and (np.abs(ind["start"][ind["kind"] == trxhip.MS_KIND_SCH] - 5) <= 1).all()
        else:
            assert (ind.tobytes(), bits.tobytes(), _labels(plan), s.clock()) == one
        s.close()


def _labels(plan):
    """what a slot is, without where it lay in its chunk"""
    return np.stack([plan[f].astype(np.int64) for f in ("fn", "tn", "kind", "flags", "ts")]).tobytes()


def _tracked(trx, d_x, total, sizes):
    """Pull with tracking on, the model beside it fed with the device's own starts; plan, to_skip, pending and clock are compared
    after every pull.  Returns [(ts, start, first_ts of the pull)] of the SCH slots, [pending after each pull], the plans."""
    s = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL, tsc=1, active_tns=ACTIVE, tracking=True)
    s.set_clock(FN0 - 1, 7, -625)
    got = {}
    model = SM.Cutter(lambda fn, tn, ts: got[fn], tracking=True)
    model.set_clock(FN0 - 1, 7, -625)
    sch, pend, plans = [], [], []
    for at, n in _chunks(total, sizes):
        bound = s.slots(n)
        i, _ = s.pull(d_x[at:at + n], first_ts=at)
        ind, p = trxhip.MsRxScheduler.ind_to_numpy(i), s.plan()
        assert len(p) <= bound
        for r, q in zip(ind, p):
            if r["kind"] == trxhip.MS_KIND_SCH:
                got[int(r["fn"])] = int(r["start"]) if r["sch_rc"] == 1 else None
                sch.append((int(q["ts"]), int(r["start"]), at))
        want = model.grab_bursts(at, n)
        assert [(int(q["fn"]), int(q["tn"]), int(q["ts"]), int(q["src_off"])) for q in p] == want
        st = s.state()
        assert (st["to_skip"], st["pending"], st["carried"]) == (model.to_skip, model.temp_ts_corr_offset, model.partial_rdofs)
        assert s.clock() == (model.tk.fn, model.tk.tn, model.tk.ts) and st["clock_jumps"] == 0
        pend.append(int(st["pending"]))
        plans.append(p)
    s.close()
    return sch, pend, plans


@pytest.mark.parametrize("cf32", [False, True])
def test_tracking_an_sch_slot_on_the_chunk_boundary(trx, late_stream, cf32):
    """Bursts 3 samples late, chunks of 5300 samples: the first SCH slot (samples 5000 .. 5624) straddles the first boundary, so
    the pull that completes it demodulates it alone, waits for its start and plans the rest with it -- the cut moves in that very
    pull, as in the reference, where the completed slot is handled before to_skip -= temp_ts_corr_offset.  Every SCH slot behind
    this first correction reports abs(start) <= 1."""
    sch, pend, plans = _tracked(trx, _dev(late_stream, cf32), len(late_stream), [5300])
    assert plans[1][0]["kind"] == trxhip.MS_KIND_SCH and plans[1][0]["src_off"] == -300
    v = sch[0][1]
    assert abs(v - 5) <= 1 and pend[0] == 0 and pend[1] == 0       # measured and applied within the second pull
    assert plans[1][1]["src_off"] == 325 + v
    assert len(sch) == 10 and all(abs(start) <= 1 for ts, start, at in sch[1:])


def test_tracking_two_sch_slots_in_one_pull_add_up(trx, late_stream):
    """Chunks of 60000 samples (96 slots): the first holds the SCH slots of frames 1 and 11, which both report the same offset
    before anything is applied, and the pending correction is their sum, as temp_ts_corr_offset is after one reference buffer
    (ms_rx_lower.cpp:199-203 runs once per SCH slot, :399 once per buffer).  The cut therefore overshoots by one offset -- the
    literal reference at this buffer size --, the single SCH slot of the second pull reports the opposite offset, and behind that
    second correction every SCH slot reports abs(start) <= 1."""
    sch, pend, plans = _tracked(trx, _dev(late_stream, False), len(late_stream), [60000])
    first = [start for ts, start, at in sch if at == 0]
    assert len(first) == 2 and all(abs(v - 5) <= 1 for v in first) and pend[0] == -sum(first)
    second = [start for ts, start, at in sch if at == 60000]
    assert len(second) == 1 and abs(second[0] + first[0]) <= 1 and pend[1] == -second[0]
    rest = [start for ts, start, at in sch if at >= 120000]
    assert len(rest) == 7 and all(abs(v) <= 1 for v in rest) and not any(pend[2:])


def test_acquire_then_pull_loopback(trx):
    """A 60000-sample buffer and its continuation (tests/test_ms_sched_cpu.py checks the precondition on the CPU models): the clock
    after the acquire is the FN sent, every ACTIVE traffic slot's hard bits are the bits sent, the SCH slot decodes to the FN sent."""
    L = SC.LOOP
    x, sent = SC.loopback_stream()
    d_x = _dev(x, False)
    s = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL, tsc=0, active_tns=L["active"], tracking=True)
    found, rec = s.acquire(d_x[:L["acq_len"]], first_ts=L["t0"])
    assert found and (rec["rc"], rec["fn"], rec["bsic"]) == (1, L["fn0"] + 7, L["bsic"])
    assert s.clock() == (L["fn0"] + 7, 0, 0)
    st = s.state()
    assert st["tsc"] == L["tsc"] and st["first_call"] == 1 and st["first_sch_ts_start"] == L["t0"] + int(rec["start"]) - 17
    at, n_traffic, n_sch = L["acq_len"], 0, 0
    for n in L["chunks"]:
        chunk = d_x[at:at + n]
        i, b = s.pull(chunk, first_ts=L["t0"] + at)
        ind, bits = trxhip.MsRxScheduler.ind_to_numpy(i), b.cpu().numpy()
        for r, hard in zip(ind, bits):
            key = (int(r["fn"]), int(r["tn"]))
            if r["kind"] == trxhip.MS_KIND_NB and r["sent"]:
                assert np.array_equal(hard, K.hard(sent[key])), key
                n_traffic += 1
            elif r["kind"] == trxhip.MS_KIND_NB:
                assert not hard.any() and not (L["active"] >> key[1]) & 1
            elif r["kind"] == trxhip.MS_KIND_SCH:
                assert (r["sch_rc"], r["sch_fn"], r["sch_bsic"]) == (1, key[0], L["bsic"]) and key[0] % 51 in (1, 11, 21, 31, 41)
                n_sch += 1
        at += chunk.shape[0]
    assert (n_traffic, n_sch) == (48, 1) and s.state()["clock_jumps"] == 0 and s.state()["slots"] == 96
    # the acquire on complex64 samples gives the same record
    s2 = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL)
    found2, rec2 = s2.acquire(_dev(x[:L["acq_len"]], True), first_ts=L["t0"])
    assert found2 and rec2.tobytes() == rec.tobytes()
    # a buffer of noise: nothing found, the object stays without a clock
    s3 = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL)
    rng = np.random.default_rng(1)
    found3, rec3 = s3.acquire(_dev(rng.integers(-50, 51, (3000, 2)).astype(np.int16), False), first_ts=5)
    assert not found3 and rec3["rc"] == 0 and s3.state()["clock_set"] == 0


def test_refusals_leave_the_state_and_the_outputs_untouched(trx):
    import torch
    L = trx.L
    vp, sz = C.c_void_p, C.c_size_t
    P = lambda t: vp(t.data_ptr())                                 # noqa: E731
    x = torch.zeros((4000, 2), dtype=torch.int16, device="cuda:0")
    xf = torch.zeros(4000, dtype=torch.complex64, device="cuda:0")
    ind = torch.full((8, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    bits = torch.full((8, 148), 0x5A, dtype=torch.int8, device="cuda:0")
    st = trx._stream()
    ns, nc = sz(), sz()
    h = vp()
    for cfg in (trxhip._MsSchedCfg(2047.0, 8, 0xFF, 1, 0), trxhip._MsSchedCfg(0.0, 0, 0xFF, 1, 0),
                trxhip._MsSchedCfg(float("nan"), 0, 0xFF, 1, 0), trxhip._MsSchedCfg(float("inf"), 0, 0xFF, 1, 0)):
        assert L.trxhip_ms_sched_create(trx.h, C.byref(cfg), C.byref(h)) == EINVAL
    s = trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL, tsc=2, tracking=False)
    pull = lambda fn, d_in, n, d_ind=P(ind), d_bits=P(bits), out=8: fn(s.h, d_in, n, 0, d_ind, d_bits, out, C.byref(ns),     # noqa: E731
                                                                       C.byref(nc), st)
    p16, pf = L.trxhip_ms_sched_pull_s16, L.trxhip_ms_sched_pull_cf32
    assert pull(p16, P(x), 700) == EINVAL                          # before set_clock or a successful acquire
    assert L.trxhip_ms_sched_acquire_s16(s.h, vp(0), 3000, 0, None, st) == EINVAL
    assert L.trxhip_ms_sched_acquire_s16(s.h, vp(x.data_ptr() + 2), 3000, 0, None, st) == EINVAL
    assert L.trxhip_ms_sched_acquire_s16(s.h, P(x), 531, 0, None, st) == EINVAL
    assert L.trxhip_ms_sched_feed_starts(s.h, None, 0) == EINVAL   # a device object takes its starts from the device
    s.set_clock(7, 7, -625)
    assert pull(p16, P(x), 700) == 0 and ns.value == 1 and nc.value == 75
    torch.cuda.synchronize()
    ind.fill_(0xAB)
    bits.fill_(0x5A)
    before = (s.state().tobytes(), s.clock(), s.plan().tobytes())
    calls = [
        (p16, P(x), 0),                                            # n_samples == 0
        (p16, vp(0), 700),                                         # NULL or misaligned buffers
        (p16, vp(x.data_ptr() + 2), 700),
        (pf, P(xf), 700),                                          # complex64 over an int16 partial slot
    ]
    for fn, d_in, n in calls:
        assert pull(fn, d_in, n) == EINVAL
    assert pull(p16, P(x), 700, d_ind=vp(0)) == EINVAL
    assert pull(p16, P(x), 700, d_ind=vp(ind.data_ptr() + 1)) == EINVAL
    assert pull(p16, P(x), 700, out=0) == EINVAL                   # out_slots too small: 1 slot would be cut
    assert pull(p16, P(x), 4000, out=5) == EINVAL                  # 6 would be cut: the completed slot and 5 in the chunk
    assert L.trxhip_ms_sched_set_tsc(s.h, 8) == EINVAL and L.trxhip_ms_sched_set_clock(s.h, 2715648, 0, 0) == EINVAL
    torch.cuda.synchronize()
    assert (s.state().tobytes(), s.clock(), s.plan().tobytes()) == before
    assert (ind.cpu().numpy() == 0xAB).all() and (bits.cpu().numpy() == 0x5A).all()
    # the complex64 entry point's alignment is 8 bytes
    s.set_clock(7, 7, -625)
    assert pull(pf, vp(xf.data_ptr() + 4), 700) == EINVAL and pull(pf, P(xf), 700) == 0
    # what is accepted goes on from the untouched state, and a NULL d_bits gives the same records
    s.set_clock(7, 7, -625)
    assert pull(p16, P(x), 700) == 0 and pull(p16, P(x), 4000, out=6) == 0 and ns.value == 6
    torch.cuda.synchronize()
    a = ind.cpu().numpy().copy()
    s.set_clock(7, 7, -625)
    assert pull(p16, P(x), 700) == 0 and pull(p16, P(x), 4000, d_bits=vp(0), out=6) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ind.cpu().numpy()[:6], a[:6]) and (a[:6] != 0xAB).any() and (a[6:] == 0xAB).all()
