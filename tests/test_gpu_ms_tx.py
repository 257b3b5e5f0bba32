"""The MS-side uplink burst scheduler on the MI355X (trxhip_ms_tx_*, MsTxScheduler; ms_tx_render_kernel): the rendered stream
against the row modulator -- a burst's samples are TrxHip.modulate(bits, {148, guard, scale of the plan}, sps=4, s16_scale=1.0)
wherever it lies and however the windows cut it -- against the model's plan and counters (tests/ms_tx_model.py), against the
oracle's modulator with the C cast in numpy, and through the BTS-side uplink receiver."""
import numpy as np
import pytest

import ms_tx_model as M
import oracle_lib as O
from osmo_trx_amd import trxhip
from osmo_trx_amd.trxhip import tx_params_host

pytestmark = pytest.mark.gpu

SENT = 64                       # sentinel samples on each side of a window
MARK = 0x5A5A


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    O.lib().orc_setup()
    t = trxhip.TrxHip(0)
    yield t
    t.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def rows_of(trx, bits, tn, scale):
    """the yardstick: int16[n, 625, 2] of the row modulator"""
    import torch
    bits = np.asarray(bits, dtype=np.uint8).reshape(-1, 148)
    p = tx_params_host(148, 8 + (np.asarray(tn) % 4 == 0), 0, np.asarray(scale, dtype=np.float32), n=len(bits))
    _, s16, lens = trx.modulate(dev(bits), trx.tx_params_tensor(p), sps=4, cf32=False, s16_scale=1.0)
    torch.cuda.synchronize()
    assert (lens.cpu().numpy() == 625).all()
    return s16.cpu().numpy()


def render(tx, n, first_ts, shift=0):
    """one window with a sentinel on each side; shift: samples the window starts behind an aligned address"""
    import torch
    buf = torch.full((SENT + shift + n + SENT, 2), MARK, dtype=torch.int16, device="cuda:0")
    out, nd = tx.render(n, first_ts, out=buf[SENT + shift:])
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:SENT + shift] == MARK).all() and (a[SENT + shift + n:] == MARK).all(), "wrote outside the window"
    return a[SENT + shift:SENT + shift + n], nd


def expected_stream(n, first_ts, bursts):
    """bursts: (radio_ts, int16[625, 2]) pairs"""
    x = np.zeros((n, 2), dtype=np.int16)
    for ts, row in bursts:
        lo, hi = max(ts, first_ts), min(ts + 625, first_ts + n)
        if lo < hi:
            x[lo - first_ts:hi - first_ts] = row[lo - ts:hi - ts]
    return x


def some_bits(rng, n):
    return rng.integers(0, 256, (n, 148)).astype(np.uint8)        # any byte: bit 0 counts


CLOCK = (1000, 2, 123457)


def one_burst(trx, rng, pwr=0, delay=-67, ta=0):
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=9830, rxtx_delay=delay, max_pending=8)
    tx.set_ta(ta)
    bits = some_bits(rng, 1)
    plan = tx.submit(trxhip.ms_tx_requests(1003, 4, pwr, bits), CLOCK)
    assert plan["status"][0] == M.QUEUED
    return tx, int(plan["radio_ts"][0]), rows_of(trx, bits, 4, plan["scale"])[0]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_alignment_classes(trx, lead, shift):
    """the burst starts lead samples into the window, the window shift samples behind a 16-byte boundary: byte offsets 0, 4, 8, 12
    mod 16 of the burst's first sample, from an aligned and from an odd window"""
    rng = np.random.default_rng(100 + 4 * shift + lead)
    tx, ts, row = one_burst(trx, rng)
    n = lead + 625 + 7
    got, nd = render(tx, n, ts - lead, shift)
    assert nd == 1 and row.any()
    assert np.array_equal(got, expected_stream(n, ts - lead, [(ts, row)]))
    assert not got[:lead].any() and not got[lead + 625:].any()
    st = tx.state()
    assert st["drawn"] == 1 and st["pending"] == 0 and st["rendered_end"] == ts - lead + n


@pytest.mark.parametrize("cut", [1, 2, 3, 312, 623, 624])
def test_straddle(trx, cut):
    rng = np.random.default_rng(7)
    whole_tx, ts, row = one_burst(trx, rng, pwr=12)
    whole, _ = render(whole_tx, 40 + 625 + 40, ts - 40)
    rng = np.random.default_rng(7)
    tx, ts2, _ = one_burst(trx, rng, pwr=12)
    assert ts2 == ts
    a, nd_a = render(tx, 40 + cut, ts - 40)
    assert nd_a == 0 and tx.state()["pending"] == 1 and tx.state()["drawn"] == 0
    b, nd_b = render(tx, 625 - cut + 40, ts + cut, shift=1)
    assert nd_b == 1 and tx.state()["pending"] == 0 and tx.state()["drawn"] == 1
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert np.array_equal(whole[40:665], row)


# ---- windows and bursts round the 625-sample pieces a render is cut into (segments here, tiles in a group) ----

@pytest.mark.parametrize("n", [1, 3, 624, 625, 626, 1249, 1251])
def test_window_lengths_round_the_tile(trx, n):
    """windows that start 1 sample before a burst and end inside the first tile, at its end, one sample into the second and round
    the end of the second; the burst is retired once its last sample is drawn, and a second render draws the rest"""
    tx, ts, row = one_burst(trx, np.random.default_rng(40))
    got, nd = render(tx, n, ts - 1, shift=n & 1)
    assert np.array_equal(got, expected_stream(n, ts - 1, [(ts, row)])) and row.any()
    assert nd == (n >= 626) and tx.state()["pending"] == (n < 626)
    rest, nd = render(tx, 700, ts - 1 + n)
    assert np.array_equal(rest, expected_stream(700, ts - 1 + n, [(ts, row)])) and nd == (n < 626)
    assert tx.state()["drawn"] == 1 and tx.state()["pending"] == 0


@pytest.mark.parametrize("lead", [624, 625, 626])
def test_burst_at_the_tile_boundary(trx, lead):
    """the burst begins one sample before the window's second tile, exactly at it and one sample after it; the tiles behind hold
    its tail and then nothing; the last tile is shorter than 625"""
    tx, ts, row = one_burst(trx, np.random.default_rng(41))
    got, nd = render(tx, 2000, ts - lead, shift=lead & 1)
    assert nd == 1 and np.array_equal(got, expected_stream(2000, ts - lead, [(ts, row)]))
    assert np.array_equal(got[lead:lead + 625], row) and row.any()


@pytest.mark.parametrize("lead", [0, 1, 312])
@pytest.mark.parametrize("gap", [0, 4])
def test_two_bursts_in_one_tile(trx, gap, lead):
    """adjacent TNs that touch, and 4 samples apart after a timing advance that fell by 1: a tile of the window holds the first
    burst's tail, the gap (or none) and the second burst's head"""
    rng = np.random.default_rng(42)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=9830, rxtx_delay=0, max_pending=8)
    bits = some_bits(rng, 2)
    tx.set_ta(10)
    a = tx.submit(trxhip.ms_tx_requests(1003, 4, 0, bits[:1]), CLOCK)
    tx.set_ta(10 - gap // 4)
    b = tx.submit(trxhip.ms_tx_requests(1003, 5, 15, bits[1:]), CLOCK)
    ts = [int(a["radio_ts"][0]), int(b["radio_ts"][0])]
    assert a["status"][0] == M.QUEUED and b["status"][0] == M.QUEUED and ts[1] - ts[0] == 625 + gap
    rows = [rows_of(trx, bits[:1], 4, a["scale"])[0], rows_of(trx, bits[1:], 5, b["scale"])[0]]
    got, nd = render(tx, 2400, ts[0] - lead, shift=lead & 1)
    assert nd == 2 and np.array_equal(got, expected_stream(2400, ts[0] - lead, zip(ts, rows)))
    assert rows[0].any() and rows[1].any() and not np.array_equal(rows[0], rows[1])


def traffic(trx, tx_full_scale=2047):
    """8 frames, a burst on 5 of the 8 TNs, mixed pwr, two timing-advance changes (falling, so that nothing overlaps):
    returns the clock, the (ta, requests, the model's plan) steps and the bursts as (radio_ts, row of the row modulator)"""
    rng = np.random.default_rng(2024)
    clock = (2715640, 5, 1 << 35)                       # the FN wraps inside the run
    steps, rows = [], []
    model = M.MsTx(tx_full_scale, -60, 64)
    for ta, frames in ((9, (1, 2, 3)), (4, (4, 5)), (0, (6, 7, 8))):
        fn = [(clock[0] + f) % M.HYPERFRAME for f in frames for _ in range(5)]
        tn = [t for _ in frames for t in (0, 1, 3, 4, 6)]
        pwr = [(7 * i) % 35 for i in range(len(fn))]
        bits = some_bits(rng, len(fn))
        model.set_ta(ta)
        plan = model.submit(zip(fn, tn, pwr), clock)
        assert all(p["status"] == M.QUEUED for p in plan)
        steps.append((ta, trxhip.ms_tx_requests(fn, tn, pwr, bits), plan))
        r = rows_of(trx, bits, tn, [p["scale"] for p in plan])
        rows += [(p["radio_ts"], r[i]) for i, p in enumerate(plan)]
    return clock, steps, rows


@pytest.mark.parametrize("chunk", [40000, 313, 625, 1250, 4999])
def test_chunking_invariance(trx, chunk):
    clock, steps, rows = traffic(trx)
    first_ts = min(ts for ts, _ in rows) - 300
    want = expected_stream(40000, first_ts, rows)
    assert len(rows) == 40 and max(ts for ts, _ in rows) + 625 <= first_ts + 40000      # 8 frames hold them all
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=-60, max_pending=64)
    model = M.MsTx(2047, -60, 64)
    for ta, reqs, ref in steps:
        tx.set_ta(ta)
        model.set_ta(ta)
        plan = tx.submit(reqs, clock)
        model.submit(zip(reqs["fn"], reqs["tn"], reqs["pwr"]), clock)
        assert [int(t) for t in plan["radio_ts"]] == [p["radio_ts"] for p in ref]
        assert plan["scale"].tobytes() == np.array([p["scale"] for p in ref], dtype=np.float32).tobytes()
    got, drawn = [], 0
    for k, at in enumerate(range(0, 40000, chunk)):
        n = min(chunk, 40000 - at)
        x, nd = render(tx, n, first_ts + at, shift=k & 1)
        ref_nd, _ = model.render(n, first_ts + at)
        assert nd == ref_nd
        got.append(x)
        drawn += nd
    got = np.concatenate(got)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:10]
    st, ref = tx.state(), model.state()
    for k, v in ref.items():
        assert int(st[k]) == v, (k, st, ref)
    assert drawn == 40 and st["drawn"] == 40 and st["pending"] == 0


def test_adjacent_empty_and_gap(trx):
    rng = np.random.default_rng(5)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=0, max_pending=8)
    bits = some_bits(rng, 3)
    plan = tx.submit(trxhip.ms_tx_requests([1003, 1003, 1010], [4, 5, 0], 0, bits), CLOCK)
    ts = [int(t) for t in plan["radio_ts"]]
    assert list(plan["status"]) == [M.QUEUED] * 3 and ts[1] == ts[0] + 625
    rows = rows_of(trx, bits, [4, 5, 0], plan["scale"])
    # a window with no burst is all zeros
    got, nd = render(tx, 1000, ts[0] - 1003, shift=1)
    assert nd == 0 and not got.any()
    # adjacent TNs: 625 samples apart, no zero sample and no double write between them -- every sample is one of the two rows'
    got, nd = render(tx, 3 + 1250 + 3, ts[0] - 3)
    assert nd == 2 and np.array_equal(got[3:628], rows[0]) and np.array_equal(got[628:1253], rows[1])
    assert not got[:3].any() and not got[1253:].any()
    # a window gap over the third burst
    got, nd = render(tx, 100, ts[2] + 5000)
    assert nd == 0 and not got.any()
    st = tx.state()
    assert st["missed"] == 1 and st["drawn"] == 2 and st["pending"] == 0


def test_power_255_is_drawn_as_zeros(trx):
    tx, ts, row = one_burst(trx, np.random.default_rng(9), pwr=255)
    assert not row.any()
    got, nd = render(tx, 700, ts - 10)
    assert nd == 1 and not got.any() and tx.state()["drawn"] == 1


def test_pinned_to_the_oracle(trx):
    """16 bursts: the oracle's modulateBurst(), driveTx()'s float scale and C's cast, in numpy"""
    rng = np.random.default_rng(16)
    n = 16
    fn, tn = 1002 + np.arange(n), np.arange(n) % 8
    pwr = (np.arange(n) * 5) % 40
    bits = rng.integers(0, 2, (n, 148)).astype(np.uint8)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=9830, rxtx_delay=-67, max_pending=n)
    plan = tx.submit(trxhip.ms_tx_requests(fn, tn, pwr, bits), CLOCK)
    assert (plan["status"] == M.QUEUED).all()
    first_ts = int(plan["radio_ts"].min()) - 5
    got, nd = render(tx, int(plan["radio_ts"].max()) + 630 - first_ts, first_ts)
    assert nd == n
    for i in range(n):
        x = O.modulate_burst(bits[i], 8 + (tn[i] % 4 == 0), 4)
        assert len(x) == 625
        s = np.float32(plan["scale"][i])
        assert s == M.scale_of(9830, pwr[i])
        z = np.float32(0.0)
        re = (x.real * s - x.imag * z).astype(np.float32)       # scaleVector: Complex<float> operator*, (s, 0)
        im = (x.real * z + x.imag * s).astype(np.float32)
        want = np.stack([np.trunc(re).astype(np.int16), np.trunc(im).astype(np.int16)], axis=1)   # static_cast<int16_t>(x * 1)
        at = int(plan["radio_ts"][i]) - first_ts
        assert np.array_equal(got[at:at + 625], want), i


def _loopback(trx, ta):
    import torch
    from test_gpu_tx_frontend import _unambiguous_bursts
    tsc, frames, tns = 5, 26, (1, 6)
    rng = np.random.default_rng(77)
    ms_rx = trxhip.MsRxScheduler(trx)
    ms_rx.set_clock(5000, 2, 40 * 625)
    clock = ms_rx.clock()
    assert clock == (5000, 2, 40 * 625)
    fn = np.repeat(clock[0] + 2 + np.arange(frames), len(tns))
    tn = np.tile(tns, frames)
    bits = _unambiguous_bursts(np.full(len(fn), tsc), rng)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=0, max_pending=128)
    tx.set_ta(ta)
    plan = tx.submit(trxhip.ms_tx_requests(fn, tn, 0, bits), clock)
    assert (plan["status"] == M.QUEUED).all()
    n_slots = (frames + 4) * 8
    x, nd = tx.render(n_slots * 625 + 1, clock[2])
    assert nd == len(fn)
    noise = torch.from_numpy(rng.integers(-20, 21, tuple(x.shape)).astype(np.int16)).to("cuda:0")
    x = (x.to(torch.int32) + noise).clamp(-32768, 32767).to(torch.int16)
    # the uplink clock at the window's origin: the downlink clock's slot three TNs earlier
    ul = M.Time(clock[0], clock[1]).decTN(3)
    rx = trxhip.RxScheduler(trx, chans=1, tsc=tsc, exact=True, full_scale=2047.0, max_slots=1024)
    rx.set_clock(ul.fn, ul.tn)
    rx.set_max_toa(20, 63)
    rx.set_trxd_version(0, 1)
    for t in range(8):
        rx.set_slot(0, t, 1)
    pkt, plen, ind, _ = rx.pull(x)
    torch.cuda.synchronize()
    assert pkt.shape[1] == n_slots
    pkt, plen, ind = pkt.cpu().numpy()[0], plen.cpu().numpy()[0], rx.ind_to_numpy(ind)[0]
    found = plen == 11 + 148
    sent = np.zeros(n_slots, bool)
    order = []
    for i in range(len(fn)):
        k = np.flatnonzero((ind["fn"] == fn[i]) & (ind["tn"] == tn[i]))
        assert len(k) == 1
        sent[k[0]] = True
        order.append(k[0])
    assert found[sent].all(), np.flatnonzero(sent & ~found)[:10]
    assert found[~sent].mean() < 0.03
    hard = (pkt[order][:, 11:11 + 148] > 127).astype(np.uint8)
    assert (hard[:, 3:145] != bits[:, 3:145]).mean() < 1e-3
    return ind["toa"][order]


def test_loopback_against_the_bts_uplink_receiver(trx):
    """MsRxScheduler's clock -> MsTxScheduler -> +-20 counts of noise -> RxScheduler.pull: every sent slot is found where the BTS
    expects it (uplink TN = downlink TN - 3), with the bars of the existing loopbacks; at TA = 5 the TOA moves by -5 symbols."""
    toa0 = _loopback(trx, 0)
    toa5 = _loopback(trx, 5)
    assert np.abs(toa5 - toa0 + 5.0).max() < 0.1, (toa0[:4], toa5[:4])
