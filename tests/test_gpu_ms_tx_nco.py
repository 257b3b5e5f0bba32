"""The MS-side uplink oscillator on the MI355X (trxhip_ms_nco_tx_*, MsTxScheduler.set_nco / MsTxSchedulerGroup.set_nco; the
rotating instances ms_tx_render_nco_kernel and ms_tx_render_group_nco_kernel): the rendered int16 against the composition of
public calls -- modulate to complex64 with the plan's scale, the NCO batch call, convert_float_short -- wherever a burst lies and
however the windows cut it, against the model (tests/ms_tx_nco_model.py) across a change of frequency and at full scale, the
group against the composition and against single objects, and the loop it closes: an uplink through a radio 2 kHz low into the
BTS-side receiver."""
import ctypes as C

import numpy as np
import pytest

import ms_nco_model as NM
import ms_tx_model as M
import ms_tx_nco_model as T
from osmo_trx_amd import trxhip
from osmo_trx_amd.trxhip import tx_params_host
from test_gpu_ms_tx import CLOCK, MARK, SENT, dev, expected_stream, render, rows_of, some_bits, traffic

pytestmark = pytest.mark.gpu

EINVAL = -22
HZ_INC1 = 1.0 / 3964.0                     # llrint(hz * 2^32 / (13e6 / 12)) = 1: the smallest increment
# inc 0, +-1, +-2000 Hz, -270 kHz and the largest increments _set accepts: +-500 kHz.  (2^31 - 1 and -2^31 lie outside
# |hz| <= 500000 -- |inc| <= 1982292598 -- so no public call brings them into a render.)
HZ_CASES = [0.0, HZ_INC1, -HZ_INC1, 2000.0, -2000.0, -270000.0, 500000.0, -500000.0]


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = trxhip.TrxHip(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def tabs():
    return trxhip.ms_nco_tables_host()


def rows_c64(trx, bits, tn, scale):
    """complex64[n, 625] device tensor of the row modulator with the plans' scales: the x of the contract"""
    import torch
    bits = np.asarray(bits, dtype=np.uint8).reshape(-1, 148)
    p = tx_params_host(148, 8 + (np.asarray(tn) % 4 == 0), 0, np.asarray(scale, dtype=np.float32), n=len(bits))
    out, _, lens = trx.modulate(dev(bits), trx.tx_params_tensor(p), sps=4, cf32=True)
    torch.cuda.synchronize()
    assert (lens.cpu().numpy() == 625).all()
    return out


def composed(trx, x, phase0, inc):
    """the composition of public calls: x complex64[n, 625] (device) -> ms_nco(phase0[r], inc) -> convert_float_short(scale 1).
    Returns int16[n, 625, 2]"""
    import torch
    y = trx.ms_nco(x.contiguous(), phase0, inc)
    out = torch.empty((x.shape[0], 625, 2), dtype=torch.int16, device="cuda:0")
    rc = trx.L.trxhip_convert_float_short(trx.h, C.c_void_p(out.data_ptr()), C.c_void_p(y.data_ptr()), C.c_float(1.0), x.shape[0] * 625 * 2,
                                          trx._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def composed_for(trx, st, x, radio_ts):
    """rows of the composition for bursts at radio_ts under the oscillator state st (nco_state()); off: the identity"""
    if not st["enable"]:
        return composed(trx, x, 0, 0)
    return composed(trx, x, [trxhip.ms_nco_phase(st["acc"], st["ts_ref"], st["inc"], int(t)) for t in radio_ts], st["inc"])


def clock_for(target_ts, fn, tn, delay, ta=0):
    """a clock (1000, 2, now_ts) from which the request (fn, tn) gets radio_ts = target_ts"""
    probe = trxhip.MsTxScheduler(None, rxtx_delay=delay)
    probe.set_ta(ta)
    k = int(probe.submit(trxhip.ms_tx_requests(fn, tn, 0, np.zeros(148, np.uint8)), (1000, 2, 0))["radio_ts"][0])
    return (1000, 2, target_ts - k)


# ---- 1. byte identity with the composition of public calls ---------------------------------------------------------------------------

@pytest.mark.parametrize("hz", HZ_CASES)
def test_equals_the_composition_of_public_calls(trx, hz):
    """two bursts of different pwr; the first begins lead samples into a window that lies shift samples behind a 16-byte boundary
    (byte offsets 0, 4, 8, 12 mod 16, from an aligned and an odd window) and straddles 2^32 or 2^40 on the radio_ts timeline"""
    for k, (lead, shift) in enumerate((l, s) for s in (0, 1) for l in (0, 1, 2, 3)):
        rng = np.random.default_rng(300 + k)
        edge = (1 << 32) if k % 2 == 0 else (1 << 40)
        clock = clock_for(edge - 100 - 37 * k, 1003, 4, -67)
        tx = trxhip.MsTxScheduler(trx, tx_full_scale=9830, rxtx_delay=-67, max_pending=8)
        tx.set_nco(True, hz)
        assert tx.nco_state()["inc"] == NM.inc_of(hz) and tx.nco_state()["ts_ref"] == 0
        bits, tn, pwr = some_bits(rng, 2), [4, 6], [0, 13]
        plan = tx.submit(trxhip.ms_tx_requests([1003, 1003], tn, pwr, bits), clock)
        ts = [int(t) for t in plan["radio_ts"]]
        assert list(plan["status"]) == [M.QUEUED] * 2 and ts[0] < edge < ts[0] + 625 and plan["scale"][0] != plan["scale"][1]
        rows = composed_for(trx, tx.nco_state(), rows_c64(trx, bits, tn, plan["scale"]), ts)
        n = ts[1] + 625 + 7 - (ts[0] - lead)
        got, nd = render(tx, n, ts[0] - lead, shift)
        want = expected_stream(n, ts[0] - lead, zip(ts, rows))
        assert nd == 2 and np.array_equal(got, want), (lead, shift, np.flatnonzero((got != want).any(axis=1))[:8])
        assert rows[0].any() and not got[:lead].any() and not got[lead + 625:ts[1] - ts[0] + lead].any()
        tx.close()


def test_the_rotation_is_there(trx):
    """a guard against a yardstick that rotates nothing: at 2000 Hz the rendered burst is not the unrotated one, its modulus is"""
    rng = np.random.default_rng(5)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=9830, rxtx_delay=0, max_pending=4)
    tx.set_nco(True, 2000.0)
    bits = some_bits(rng, 1)
    plan = tx.submit(trxhip.ms_tx_requests(1003, 4, 0, bits), CLOCK)
    ts = int(plan["radio_ts"][0])
    got, _ = render(tx, 625, ts)
    plain = rows_of(trx, bits, 4, plan["scale"])[0]
    assert (got != plain).any(axis=1).mean() > 0.9
    assert np.abs(np.hypot(*got.astype(np.float64).T) - np.hypot(*plain.astype(np.float64).T)).max() < 2.0
    ang = np.angle((got[:, 0] + 1j * got[:, 1]) * np.conj(plain[:, 0] + 1j * plain[:, 1]))
    k = np.arange(625)
    want = np.angle(np.exp(2j * np.pi * 2000.0 / NM.SAMPLE_HZ * (ts + k)))
    big = np.hypot(*plain.astype(np.float64).T) > 1000
    assert np.abs(np.angle(np.exp(1j * (ang - want))))[big].max() < 0.01       # hz > 0 moves the spectrum up


# ---- 2. chunking -----------------------------------------------------------------------------------------------------------------------

def one_burst(trx, seed, hz, pwr=12):
    rng = np.random.default_rng(seed)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=9830, rxtx_delay=-67, max_pending=8)
    tx.set_nco(True, hz)
    bits = some_bits(rng, 1)
    plan = tx.submit(trxhip.ms_tx_requests(1003, 4, pwr, bits), CLOCK)
    assert plan["status"][0] == M.QUEUED
    return tx, int(plan["radio_ts"][0]), bits, plan


@pytest.mark.parametrize("cut", [1, 2, 3, 312, 623, 624])
def test_straddle(trx, cut):
    whole_tx, ts, bits, plan = one_burst(trx, 7, -270000.0)
    whole, _ = render(whole_tx, 40 + 625 + 40, ts - 40)
    row = composed_for(trx, whole_tx.nco_state(), rows_c64(trx, bits, 4, plan["scale"]), [ts])[0]
    assert np.array_equal(whole[40:665], row) and row.any()
    tx, ts2, _, _ = one_burst(trx, 7, -270000.0)
    assert ts2 == ts
    a, nd_a = render(tx, 40 + cut, ts - 40)
    assert nd_a == 0 and tx.state()["pending"] == 1
    b, nd_b = render(tx, 625 - cut + 40, ts + cut, shift=1)
    assert nd_b == 1 and tx.state()["pending"] == 0 and tx.state()["drawn"] == 1
    assert np.array_equal(np.concatenate([a, b]), whole)


@pytest.fixture(scope="module")
def traffic_2k(trx):
    """test_gpu_ms_tx's 8 frames of 40 bursts (mixed pwr, three timing advances) and their stream under an oscillator at +2000 Hz
    set before the first window: the composition's rows where the bursts lie"""
    clock, steps, rows = traffic(trx)
    first_ts = min(ts for ts, _ in rows) - 300
    bits = np.concatenate([reqs["bits"] for _, reqs, _ in steps])
    tn = np.concatenate([reqs["tn"] for _, reqs, _ in steps])
    plans = [p for _, _, ref in steps for p in ref]
    ts = [p["radio_ts"] for p in plans]
    st = dict(enable=True, acc=0, ts_ref=0, inc=NM.inc_of(2000.0))
    y = composed_for(trx, st, rows_c64(trx, bits, tn, [p["scale"] for p in plans]), ts)
    want = expected_stream(40000, first_ts, zip(ts, y))
    want.setflags(write=False)
    return clock, steps, first_ts, want


@pytest.mark.parametrize("chunk", [40000, 313, 625, 1250, 4999])
def test_chunking_invariance(trx, traffic_2k, chunk):
    clock, steps, first_ts, want = traffic_2k
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=-60, max_pending=64)
    tx.set_nco(True, 2000.0)
    for ta, reqs, _ in steps:
        tx.set_ta(ta)
        assert (tx.submit(reqs, clock)["status"] == M.QUEUED).all()
    got, drawn = [], 0
    for k, at in enumerate(range(0, 40000, chunk)):
        n = min(chunk, 40000 - at)
        x, nd = render(tx, n, first_ts + at, shift=k & 1)
        got.append(x)
        drawn += nd
    got = np.concatenate(got)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:10]
    assert drawn == 40 and tx.state()["drawn"] == 40 and tx.state()["pending"] == 0
    assert tx.nco_state() == dict(enable=True, inc=NM.inc_of(2000.0), acc=0, ts_ref=0, hz=2000.0)      # renders leave it alone


# ---- 3. a change of frequency in the middle of a burst --------------------------------------------------------------------------------

@pytest.mark.parametrize("second", [(True, -1500.0), (False, 0.0), (True, 2000.0)])
def test_change_between_two_renders_inside_a_burst(trx, tabs, second):
    tx, ts, bits, plan = one_burst(trx, 11, 2000.0, pwr=0)
    model = T.MsTxNco(9830, -67, 8)
    model.set_nco(True, 2000.0)
    pm = model.submit([(1003, 4, 0)], CLOCK)
    assert pm[0]["radio_ts"] == ts
    x = {ts: rows_c64(trx, bits, 4, plan["scale"]).cpu().numpy()[0]}
    a, _ = render(tx, 40 + 312, ts - 40)
    _, ma = model.render_stream(40 + 312, ts - 40, x, tabs)
    tx.set_nco(*second)
    model.set_nco(*second)
    assert tx.nco_state() == model.nco_state() and tx.nco_state()["ts_ref"] == ts + 312
    b, nd = render(tx, 313 + 40, ts + 312, shift=1)
    _, mb = model.render_stream(313 + 40, ts + 312, x, tabs)
    assert nd == 1 and np.array_equal(a, ma) and np.array_equal(b, mb)
    assert ma[40:].any() and mb[:313].any()
    if second == (True, 2000.0):                                  # the same frequency again: the burst drawn whole
        whole_tx, _, _, _ = one_burst(trx, 11, 2000.0, pwr=0)
        whole, _ = render(whole_tx, 40 + 625 + 40, ts - 40)
        assert np.array_equal(np.concatenate([a, b]), whole)
    else:
        # phase continuity at rendered_end: the second part's first sample is rotated by exactly p(ts + 312) of the first setting
        first = dict(enable=True, acc=0, ts_ref=0, inc=NM.inc_of(2000.0))
        if second[0]:
            assert tx.nco_state()["acc"] == NM.phase(0, 0, first["inc"], ts + 312)
            y = NM.rotate(tabs, x[ts][312:313], tx.nco_state()["acc"], 0)
            assert np.array_equal(T.cast(y)[0], b[0])
        else:
            assert np.array_equal(b[:313], T.cast(x[ts][312:]))


# ---- 4. off and zero -------------------------------------------------------------------------------------------------------------------

def test_zero_hz_and_off_are_the_plain_render(trx):
    clock, steps, rows = traffic(trx)
    first_ts = min(ts for ts, _ in rows) - 300
    plain = expected_stream(40000, first_ts, rows)                  # the row modulator's int16: the render without an oscillator
    # 0 Hz from creation
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=-60, max_pending=64)
    tx.set_nco(True, 0.0)
    for ta, reqs, _ in steps:
        tx.set_ta(ta)
        tx.submit(reqs, clock)
    got, nd = render(tx, 40000, first_ts)
    assert nd == 40 and np.array_equal(got, plain)
    # on, then off: never-on from there
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=-60, max_pending=64)
    tx.set_nco(True, -270000.0)
    for ta, reqs, _ in steps:
        tx.set_ta(ta)
        tx.submit(reqs, clock)
    a, _ = render(tx, 17000, first_ts)
    assert (a != plain[:17000]).any()
    tx.set_nco(False)
    assert tx.nco_state() == dict(enable=False, inc=0, acc=0, ts_ref=first_ts + 17000, hz=0.0)
    b, _ = render(tx, 23000, first_ts + 17000, shift=1)
    assert np.array_equal(b, plain[17000:]) and b.any()


# ---- 5. full scale ---------------------------------------------------------------------------------------------------------------------

def test_full_scale(trx, tabs):
    """tx_full_scale 21477, pwr 0, 64 bursts at scattered phases (123456.7 Hz: the phase moves 41 degrees a sample)"""
    rng = np.random.default_rng(21477)
    fn, tn = 1002 + np.arange(64) // 8, np.arange(64) % 8
    bits = rng.integers(0, 2, (64, 148)).astype(np.uint8)
    bits[0], bits[1] = 0, 1                                         # the constant bursts reach the largest samples
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=21477, rxtx_delay=0, max_pending=64)
    model = T.MsTxNco(21477, 0, 64)
    tx.set_nco(True, 123456.7)
    model.set_nco(True, 123456.7)
    plan = tx.submit(trxhip.ms_tx_requests(fn, tn, 0, bits), CLOCK)
    pm = model.submit(zip(fn, tn, [0] * 64), CLOCK)
    assert (plan["status"] == M.QUEUED).all() and (plan["scale"] == np.float32(21477.0)).all()
    x = rows_c64(trx, bits, tn, plan["scale"]).cpu().numpy()
    first_ts = int(plan["radio_ts"].min()) - 9
    n = int(plan["radio_ts"].max()) + 625 + 9 - first_ts
    got, nd = render(tx, n, first_ts, shift=1)
    _, want = model.render_stream(n, first_ts, {p["radio_ts"]: x[i] for i, p in enumerate(pm)}, tabs)
    assert nd == 64 and np.array_equal(got, want)
    peak = int(np.abs(got.astype(np.int32)).max())
    print(f"full scale: the largest |int16| is {peak}, the largest |x| {np.abs(x).max():.2f}")
    assert 21477 * 0.9 < peak <= 32767 and np.abs(x).max() < 32767.5


# ---- 6. the group ----------------------------------------------------------------------------------------------------------------------

def group_case(trx, settings):
    """three members with their own timing advance, requests and windows, rendered twice; members[m] = (enable, hz) set before
    the first render, and member 2's frequency halves between the renders.  Every window is the composition's rows (composed_for
    over rows_c64, under the member's oscillator state at that render) where the plan puts them.  Returns (group windows, single
    windows)"""
    import torch
    rng = np.random.default_rng(66)
    g = trxhip.MsTxSchedulerGroup(trx, n_members=3, tx_full_scale=9830, rxtx_delay=-67, max_pending=16)
    single = [trxhip.MsTxScheduler(trx, tx_full_scale=9830, rxtx_delay=-67, max_pending=16) for _ in range(3)]
    clocks = [(1000, 2, 123457), (1000, 2, (1 << 32) - 9000), (2000, 5, -40000)]
    members, fn, tn, pwr = [], [], [], []
    for m in range(3):
        g.set_ta(m, 3 * m)
        single[m].set_ta(3 * m)
        if settings[m] is not None:
            g.set_nco(m, *settings[m])
            single[m].set_nco(*settings[m])
        for k in range(6):
            members.append(m)
            fn.append(clocks[m][0] + 1 + k // 3)
            tn.append((2 * k + m) % 8)
            pwr.append(5 * k)
    bits = some_bits(rng, len(fn))
    reqs = trxhip.ms_tx_requests(fn, tn, pwr, bits)
    plan = g.submit(members, reqs, clocks)
    assert (plan["status"] == M.QUEUED).all()
    for m in range(3):
        idx = [i for i, x in enumerate(members) if x == m]
        assert single[m].submit(reqs[idx], clocks[m]).tobytes() == plan[idx].tobytes()
    x = rows_c64(trx, bits, tn, plan["scale"])
    out = []
    at = [int(plan["radio_ts"][[i for i, x in enumerate(members) if x == m]].min()) - 10 * (m + 1) for m in range(3)]
    for rnd, sizes in enumerate(([3000 + 313, 5000, 5001], [6000, 4999, 4000])):
        stride = max(sizes) + 3
        buf = torch.full((3, stride, 2), MARK, dtype=torch.int16, device="cuda:0")
        states = [g.nco_state(m) for m in range(3)]
        _, nd = g.render(sizes, at, out=buf)
        torch.cuda.synchronize()
        a = buf.cpu().numpy()
        for m in range(3):
            assert (a[m, sizes[m]:] == MARK).all()
            idx = [i for i, y in enumerate(members) if y == m]
            ts = [int(t) for t in plan["radio_ts"][idx]]
            want = expected_stream(sizes[m], at[m], zip(ts, composed_for(trx, states[m], x[idx], ts)))
            assert np.array_equal(a[m, :sizes[m]], want), (rnd, m, np.flatnonzero((a[m, :sizes[m]] != want).any(axis=1))[:8])
            s, nd_s = render(single[m], sizes[m], at[m], shift=m & 1)
            assert nd_s == nd[m]
            out.append((a[m, :sizes[m]], s))
            at[m] += sizes[m]
        if settings[2] is not None:
            g.set_nco(2, settings[2][0], settings[2][1] / 2)
            single[2].set_nco(settings[2][0], settings[2][1] / 2)
        for m in range(3):
            assert g.nco_state(m) == single[m].nco_state()
    assert sum(int(g.state(m)["drawn"]) for m in range(3)) >= 12
    return out


def test_group_equals_three_single_objects(trx):
    out = group_case(trx, [None, (True, 2000.0), (True, -270000.0)])
    for k, (a, s) in enumerate(out):
        assert np.array_equal(a, s) and a.any(), k
    # the oscillators are there: members 1 and 2 differ from the same group without any
    plain = group_case(trx, [None, None, None])
    for k, ((a, _), (p, _)) in enumerate(zip(out, plain)):
        assert np.array_equal(a, p) == (k % 3 == 0), k


def test_group_render_of_the_off_member_alone(trx):
    """a render in which only the member with its oscillator off has a window: the bytes of a group that has none"""
    import torch
    rng = np.random.default_rng(67)
    bits = some_bits(rng, 3)
    outs = []
    for on in (True, False):
        g = trxhip.MsTxSchedulerGroup(trx, n_members=3, tx_full_scale=2047, rxtx_delay=0, max_pending=8)
        if on:
            g.set_nco(1, True, 2000.0)
            g.set_nco(2, True, -270000.0)
        plan = g.submit([0, 0, 0], trxhip.ms_tx_requests([1003, 1003, 1004], [4, 5, 0], [0, 11, 22], bits), [CLOCK, None, None])
        ts = int(plan["radio_ts"][0])
        buf = torch.full((3, 6000, 2), MARK, dtype=torch.int16, device="cuda:0")
        _, nd = g.render([5999, 0, 0], [ts - 5, 0, 0], out=buf)
        torch.cuda.synchronize()
        a = buf.cpu().numpy()
        assert nd == [3, 0, 0] and (a[1:] == MARK).all() and (a[0, 5999:] == MARK).all()
        outs.append(a[0, :5999])
        rows = rows_of(trx, bits, [4, 5, 0], plan["scale"])
        assert np.array_equal(a[0, :5999], expected_stream(5999, ts - 5, zip([int(t) for t in plan["radio_ts"]], rows)))
        rows = composed_for(trx, g.nco_state(0), rows_c64(trx, bits, [4, 5, 0], plan["scale"]), plan["radio_ts"])
        assert np.array_equal(a[0, :5999], expected_stream(5999, ts - 5, zip([int(t) for t in plan["radio_ts"]], rows)))
    assert np.array_equal(outs[0], outs[1])


# ---- 7., 8. the loop: MS uplink -> a radio 2000 Hz low -> the BTS-side uplink receiver --------------------------------------------------

RADIO_HZ = -2000.0


def bts_receives(trx, x, clock, fn, tn, bits, tsc, rng):
    """the int16 uplink stream x (numpy, its first sample at the downlink clock's slot) through the radio's error and +-20 counts of
    noise into RxScheduler, as test_gpu_ms_tx._loopback: returns (sent slots found, fraction of wrong hard bits 3 .. 144)"""
    import torch
    n_slots = (len(x) - 1) // 625
    y = T.radio(x, RADIO_HZ).astype(np.int32) + rng.integers(-20, 21, x.shape)
    y = dev(y.clip(-32768, 32767).astype(np.int16))
    ul = M.Time(clock[0], clock[1]).decTN(3)                        # the uplink clock: the downlink slot three TNs earlier
    rx = trxhip.RxScheduler(trx, chans=1, tsc=tsc, exact=True, full_scale=2047.0, max_slots=1024)
    rx.set_clock(ul.fn, ul.tn)
    rx.set_max_toa(20, 63)
    rx.set_trxd_version(0, 1)
    for t in range(8):
        rx.set_slot(0, t, 1)
    pkt, plen, ind, _ = rx.pull(y)
    torch.cuda.synchronize()
    assert pkt.shape[1] == n_slots
    pkt, plen, ind = pkt.cpu().numpy()[0], plen.cpu().numpy()[0], rx.ind_to_numpy(ind)[0]
    found = plen == 11 + 148
    order = []
    for i in range(len(fn)):
        k = np.flatnonzero((ind["fn"] == fn[i]) & (ind["tn"] == tn[i]))
        assert len(k) == 1
        order.append(k[0])
    hard = (pkt[order][:, 11:11 + 148] > 127).astype(np.uint8)
    return found[order], float((hard[:, 3:145] != bits[:, 3:145])[found[order]].mean())


def uplink_through_the_radio(trx, clock, nco_hz):
    from test_gpu_tx_frontend import _unambiguous_bursts
    import torch
    tsc, frames, tns = 5, 26, (1, 6)
    rng = np.random.default_rng(77)
    fn = np.repeat(clock[0] + 2 + np.arange(frames), len(tns))
    tn = np.tile(tns, frames)
    bits = _unambiguous_bursts(np.full(len(fn), tsc), rng)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=0, max_pending=128)
    if nco_hz is not None:
        tx.set_nco(True, nco_hz)
    plan = tx.submit(trxhip.ms_tx_requests(fn, tn, 0, bits), clock)
    assert (plan["status"] == M.QUEUED).all()
    n_slots = (frames + 4) * 8
    x, nd = tx.render(n_slots * 625 + 1, clock[2])
    torch.cuda.synchronize()
    assert nd == len(fn)
    return bts_receives(trx, x.cpu().numpy(), clock, fn, tn, bits, tsc, rng)


def test_loopback_through_a_radio_2000_hz_low(trx):
    clock = (5000, 2, 40 * 625)
    found, wrong = uplink_through_the_radio(trx, clock, None)
    print(f"uplink oscillator off, radio at {RADIO_HZ:+.0f} Hz: {found.sum()} of {len(found)} slots found, {wrong:.4f} of the hard bits wrong")
    assert found.all() and wrong > 0.25
    found, wrong = uplink_through_the_radio(trx, clock, -RADIO_HZ)
    print(f"uplink oscillator at {-RADIO_HZ:+.0f} Hz: {found.sum()} of {len(found)} slots found, {wrong:.5f} of the hard bits wrong")
    assert found.all() and wrong < 1e-3


def test_the_whole_ms(trx):
    """the cold stream of test_gpu_ms_fsearch at +2000 Hz -> acquire_afc() -> the uplink oscillator from the receive one -> submit
    from the receiver's clock -> render -> the radio's error on the uplink -> RxScheduler.  No frequency is given to the MS."""
    import ms_fsearch_cases as FC
    from test_gpu_ms_fsearch import cold_stream, FULL
    x = cold_stream()[0]
    rx = trxhip.MsRxScheduler(trx, rx_full_scale=FULL, tsc=FC.TSC, active_tns=0x0F, tracking=True)
    found, rec, hit, fc = rx.acquire_afc(dev(x)[:FC.ACQ_LEN], first_ts=0)
    assert found is True and rx.nco_state()["enable"] and abs(rx.nco_state()["hz"] - RADIO_HZ) <= 100.0
    hz = trxhip.nco_tx_hz(rx.nco_state()["hz"])
    clock = rx.clock()
    print(f"whole MS: receive oscillator {rx.nco_state()['hz']:.1f} Hz, uplink oscillator {hz:.1f} Hz, clock {clock}")
    found, wrong = uplink_through_the_radio(trx, clock, hz)
    print(f"whole MS: {found.sum()} of {len(found)} slots found, {wrong:.5f} of the hard bits wrong")
    assert found.all() and wrong < 1e-3


# ---- 9. refusals on device objects -----------------------------------------------------------------------------------------------------

def test_refusals_on_device_objects(trx):
    import torch
    rng = np.random.default_rng(9)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=0, max_pending=8)
    g = trxhip.MsTxSchedulerGroup(trx, n_members=2, tx_full_scale=2047, rxtx_delay=0, max_pending=8)
    tx.set_nco(True, 2000.0)
    g.set_nco(1, True, -2000.0)
    bits = some_bits(rng, 1)
    ts = int(tx.submit(trxhip.ms_tx_requests(1003, 4, 0, bits), CLOCK)["radio_ts"][0])
    g.submit([1], trxhip.ms_tx_requests(1003, 4, 0, bits), [None, CLOCK])
    before = (tx.state().tobytes(), tx.nco_state(), [g.state(m).tobytes() for m in range(2)], [g.nco_state(m) for m in range(2)])
    L = trx.L
    for hz in (500000.5, -1e9, float("nan")):
        cfg = trxhip._MsNcoCfg(1, 0, hz)
        assert L.trxhip_ms_nco_tx_set(tx.h, C.byref(cfg)) == EINVAL and L.trxhip_ms_nco_tx_group_set(g.h, 1, C.byref(cfg)) == EINVAL
    ok = trxhip._MsNcoCfg(1, 0, 1.0)
    assert L.trxhip_ms_nco_tx_group_set(g.h, 2, C.byref(ok)) == EINVAL and L.trxhip_ms_nco_tx_set(tx.h, None) == EINVAL
    assert L.trxhip_ms_nco_tx_state(tx.h, None) == EINVAL and L.trxhip_ms_nco_tx_group_state(g.h, 2, None) == EINVAL
    # refused renders: nothing is written, nothing moves
    buf = torch.full((2, 1000, 2), MARK, dtype=torch.int16, device="cuda:0")
    assert L.trxhip_ms_tx_render_s16(tx.h, C.c_void_p(buf.data_ptr() + 2), 100, ts, None, trx._stream()) == EINVAL      # not 4-byte aligned
    assert L.trxhip_ms_tx_render_s16(tx.h, C.c_void_p(buf.data_ptr()), (1 << 31) + 1, ts, None, trx._stream()) == EINVAL
    with pytest.raises(trxhip.TrxHipError):
        g.render([0, 1001], [0, ts], out=buf)                       # longer than the stride
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == MARK).all()
    after = (tx.state().tobytes(), tx.nco_state(), [g.state(m).tobytes() for m in range(2)], [g.nco_state(m) for m in range(2)])
    assert after == before
    # and the objects work on: both draw the same rotated burst
    a, nd = render(tx, 700, ts - 30)
    _, ndg = g.render([0, 700], [0, ts - 30], out=buf)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert nd == 1 and ndg == [0, 1] and (b[0] == MARK).all() and (b[1, 700:] == MARK).all()
    x = rows_c64(trx, bits, 4, [2047.0])
    up = composed(trx, x, [trxhip.ms_nco_phase(0, 0, NM.inc_of(2000.0), ts)], NM.inc_of(2000.0))[0]
    down = composed(trx, x, [trxhip.ms_nco_phase(0, 0, NM.inc_of(-2000.0), ts)], NM.inc_of(-2000.0))[0]
    assert np.array_equal(a[30:655], up) and np.array_equal(b[1, 30:655], down) and not a[:30].any() and not b[1, 655:700].any()
