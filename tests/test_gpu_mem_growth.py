"""Scratch that grows between two calls of one object (pytest -m gpu): a small call, then a larger one whose buffers are freed and
allocated again in between (csrc/trx_mem.h, reserve()).  What the larger call gives is compared byte for byte with an object whose
buffers had the room before the small call.  Only the growth paths no other test reaches: the levels of gain control
(trxhip_ms_group's d_work) grow from one slot to 330 in test_gpu_ms_agc.py (test_stream_windows_and_decisions,
test_group_equals_single_objects), against the model."""
import numpy as np
import pytest

import ms_nco_model as NM
import ms_sched_cases as SC
from osmo_trx_amd import trxhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def trx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = trxhip.TrxHip(0)
    yield t
    t.close()


def rand_i16(rng, shape, amp=2047):
    return torch.from_numpy(rng.integers(-amp, amp + 1, shape).astype(np.int16)).to("cuda:0")


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_rx_frontend_channel_scratch(trx):
    """d_chan: a geometry that fits no tile of the fused kernel (q = 384) runs the channelizer into a scratch buffer; a pull of 1
    block, then one of 4.  The other object had pulled 4 blocks and was reset before."""
    p, q, bl = 65, 384, 384
    rng = np.random.default_rng(501)
    x = rand_i16(rng, (5 * bl * 4, 2), 20000)
    outs = []
    for room in (False, True):
        fe = trxhip.RxFrontEnd(trx, block_len=bl, p=p, q=q, chans=3)
        if room:
            fe.pull(rand_i16(rng, (4 * bl * 4, 2)), 4)
            fe.reset()
        a = fe.pull(x[:bl * 4].contiguous(), 1)
        b = fe.pull(x[bl * 4:].contiguous(), 4)
        torch.cuda.synchronize()
        outs.append((a, b))
        fe.close()
    assert outs[0][1].abs().max().item() > 0
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])


def test_ms_group_acquire_nco_work(trx):
    """d_nco_work: an acquire of two members, one with its NCO on, over buffers of the minimum 532 samples, then of 2048 (a cell's
    stream from an SCH slot on; the NCO member's with the carrier offset its oscillator takes out).  The other group had searched
    2048-sample buffers of zeros before: an acquire that finds nothing moves nothing."""
    rng = np.random.default_rng(502)
    hz = 1234.5
    x, _ = SC.cell_stream(8811, 51 * 30 + 1, 1, 0o53, tsc=3, late=6)
    big = torch.from_numpy(np.stack([NM.to_i16(NM.carrier(x[:2048], -hz)), x[:2048]])).to("cuda:0")
    small = rand_i16(rng, (2, 532, 2))
    nothing = torch.zeros((2, 2048, 2), dtype=torch.int16, device="cuda:0")
    ts = [2 ** 33 + 5, 77]
    res = []
    for room in (False, True):
        g = trxhip.MsRxSchedulerGroup(trx, 2, rx_full_scale=2047.0, tracking=True)
        g.set_nco(1, True, hz)
        if room:
            found, _ = g.acquire([1, 0], nothing, first_ts=ts)
            assert not found.any()
        fa, ra = g.acquire([1, 0], small, first_ts=ts)
        fb, rb = g.acquire([1, 0], big, first_ts=ts)
        res.append((list(fa), ra.tobytes(), list(fb), rb.tobytes(), g.state(0).tobytes(), g.state(1).tobytes()))
    assert res[0] == res[1]


def test_ms_tx_group_tables(trx):
    """d_stage / d_tab and their pinned twins keep a floor of 4096 bytes: a submit of 3 rows and a render of 8 slots, then a submit
    of 597 rows (164 bytes each) and a render of 512 slots with 600 bursts in its table (8 bytes each).  A group has no call that
    sizes its tables without moving its windows, so the yardstick is the three members as single objects, whose segment tables
    take the other path (and grow too: 16 bytes per segment)."""
    rng = np.random.default_rng(503)
    n, per = 3, 200
    bits = rng.integers(0, 2, (n, per, 148)).astype(np.uint8)
    k = np.arange(per)
    reqs = [trxhip.ms_tx_requests(110 + k // 8, k % 8, rng.integers(0, 30, per), bits[m]) for m in range(n)]
    clock = (100, 0, 0)
    g = trxhip.MsTxSchedulerGroup(trx, n_members=n, max_pending=256)
    singles = [trxhip.MsTxScheduler(trx, max_pending=256) for _ in range(n)]
    for m in range(n):
        g.set_ta(m, 3 * m)
        singles[m].set_ta(3 * m)
    pg = g.submit(np.arange(n), np.concatenate([r[:1] for r in reqs]), [clock] * n)
    for m in range(n):
        assert singles[m].submit(reqs[m][:1], clock).tobytes() == pg[m:m + 1].tobytes()
    first = 0
    for w, n_slots in enumerate((8, 512)):
        ns = n_slots * 625
        out, drawn = g.render(ns, first)
        for m in range(n):
            want, nd = singles[m].render(ns, first)
            assert same(out[m, :ns], want) and nd == drawn[m], (w, m)
            assert g.state(m).tobytes() == singles[m].state().tobytes()
        if w == 0:
            pg = g.submit(np.repeat(np.arange(n), per - 1), np.concatenate([r[1:] for r in reqs]), [clock] * n)
            assert (pg["status"] == 0).all()                           # TRXHIP_MS_TX_QUEUED
            for m in range(n):
                assert singles[m].submit(reqs[m][1:], clock).tobytes() == pg[m * (per - 1):(m + 1) * (per - 1)].tobytes()
        first += ns
    torch.cuda.synchronize()
    assert sum(drawn) == n * per and out.abs().max().item() > 0


def test_tx_sched_carry_keeps_its_contents(trx):
    """d_carry, the one growth that keeps contents: a render through a front end of the shortest block (q samples) leaves a
    remainder; the next render goes through a front end of a longer block, so the carry buffer grows while samples are carried.
    The other object's carry buffer was sized for the longer block by an empty render before."""
    p, q = 96, 65
    rng = np.random.default_rng(504)
    dgrams = [(fn, tn, rng.integers(0, 2, 148)) for fn in (77, 78, 79) for tn in range(8)]
    res = []
    for room in (False, True):
        s = trxhip.TxScheduler(trx, chans=1, sps=4, filler=trxhip.FILLER_DUMMY, full_scale=3000.0, queue_cap=64, max_slots=8)
        s.set_clock(77, 3)
        for tn in range(8):
            s.set_slot(0, tn, 1)
        for fn, tn, b in dgrams:
            s.submit(0, bytes([tn]) + int(fn).to_bytes(4, "big") + bytes([0]) + bytes(int(x) for x in b))
        short = trxhip.TxFrontEnd(trx, chans=1, block_len=q, p=p, q=q, mode="resamp")
        long_ = trxhip.TxFrontEnd(trx, chans=1, block_len=10 * q, p=p, q=q, mode="resamp")
        if room:
            assert s.render_frontend(0, long_)[:2] == (0, 0)
        nb1, nc1, o1, _ = s.render_frontend(1, short)
        nb2, nc2, o2, _ = s.render_frontend(8, long_)
        torch.cuda.synchronize()
        assert (nb1, nc1) == (625 // q, 625 % q) and nc1 > 0
        assert (nb2, nc2) == ((nc1 + 5000) // (10 * q), (nc1 + 5000) % (10 * q))
        res.append((o1.clone(), o2.clone()))
        s.close()
    assert res[0][1].abs().max().item() > 0
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])
