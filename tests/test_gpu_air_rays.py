"""The air interface's multipath rays on the MI355X (trxhip_multipath_*, AirChannel.set_rays; air_ul_rays_kernel and
air_dl_rays_kernel in csrc/trx_air.hip): the device object byte-identical to the host object -- the plain loop over the same
inline functions, itself pinned to the numpy model in tests/test_air_rays_cpu.py -- on the CPU cases, across the share split of
the ray list, in the long-window instance and through the ring; and byte-identical to the object as it was with one member per
ray, which pins the new kernels to the existing ones without the host loop; and the two loops of tests/test_gpu_air.py through
a dispersive channel (tests/air_rays_loop.py) into the receivers that equalise."""
import functools

import numpy as np
import pytest

from osmo_trx_amd import trxhip
from test_air_cpu import CHUNKS, FIRST_TS, MAX_DELAY, N, RMS, SEED, rows3
from test_air_rays_cpu import PLAIN0, case1
from test_gpu_air import cuts_of, dev, ul_windows

pytestmark = pytest.mark.gpu

UL, DL = trxhip.AIR_UL, trxhip.AIR_DL


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = trxhip.TrxHip(0)
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def host_ul(first_ts):
    y = case1(trxhip.AirChannel(None, 3, MAX_DELAY, SEED)).uplink(rows3(), first_ts)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def host_dl(first_ts):
    y = case1(trxhip.AirChannel(None, 3, MAX_DELAY, SEED)).downlink(rows3()[0], first_ts)
    y.setflags(write=False)
    return y


def where(y, ref):
    return np.flatnonzero((y != ref).reshape(len(y), -1).any(axis=1))[:8]


# ---- 7. the CPU cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_uplink_equals_the_host_object(trx, first_ts):
    d = case1(trxhip.AirChannel(trx, 3, MAX_DELAY, SEED))
    y = ul_windows(d, rows3(), first_ts, [0, N], True)
    assert np.array_equal(y, host_ul(first_ts)) and y.any(), where(y, host_ul(first_ts))
    assert d.path_state(UL, 0)["end_ts"] == first_ts + N


@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_downlink_equals_the_host_object(trx, first_ts):
    d = case1(trxhip.AirChannel(trx, 3, MAX_DELAY, SEED))
    x = rows3()[0]
    assert np.array_equal(d.downlink(dev(x), first_ts).cpu().numpy(), host_dl(first_ts))
    d2 = case1(trxhip.AirChannel(trx, 3, MAX_DELAY, SEED))
    parts = [d2.downlink(dev(x[k:k + 63]), first_ts + k) for k in range(0, N, 63)]
    assert np.array_equal(np.concatenate([p.cpu().numpy() for p in parts], axis=1), host_dl(first_ts))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_uplink_chunking_changes_no_bit(trx, chunk):
    """every window behind the first runs on the list the first one copied"""
    first_ts = (1 << 32) - 100
    d = case1(trxhip.AirChannel(trx, 3, MAX_DELAY, SEED))
    y = ul_windows(d, rows3(), first_ts, cuts_of(N, chunk), True)
    assert np.array_equal(y, host_ul(first_ts)), where(y, host_ul(first_ts))


def test_set_rays_between_windows(trx):
    """the state round trip, set_path and set_noise under rays, and clearing, on both directions: the device object follows the
    host object window by window, and the states agree"""
    x = rows3()
    d, h = (case1(trxhip.AirChannel(t, 3, MAX_DELAY, SEED)) for t in (trx, None))
    got = [[], []]
    for k, (lo, hi) in enumerate(((0, 200), (200, 333), (333, 450), (450, N))):
        for j, o in enumerate((d, h)):
            if k == 1:
                for dir in (UL, DL):
                    o.set_rays(dir, 1, o.rays(dir, 1)[0])
                    o.set_rays(dir, 2, o.rays(dir, 2)[0])
            if k == 2:
                o.set_rays(DL, 2, o.rays(DL, 2)[0][:40])               # a shorter list on the device
                o.set_path(UL, 1, gain=0.5, delay=31, hz=-1234.5)      # under rays: no byte of the output
                o.set_path(UL, 0, gain=2.0, delay=3, hz=500.0)         # a plain member of a direction with rays
                o.set_noise(UL, 0, 100.0)
                o.set_noise(DL, 1, 55.0)
            if k == 3:
                for dir in (UL, DL):
                    o.set_rays(dir, 1, None)
                    o.set_rays(dir, 2, [])                             # the last rays go: the direction is plain again
            w, v = np.ascontiguousarray(x[:, lo:hi]), np.ascontiguousarray(x[1, lo:hi])
            y, z = o.uplink(dev(w) if j == 0 else w, 1000 + lo), o.downlink(dev(v) if j == 0 else v, 1000 + lo)
            got[j].append((y.cpu().numpy(), z.cpu().numpy()) if j == 0 else (y, z))
        for m in range(3):
            for dir in (UL, DL):
                assert d.path_state(dir, m).tobytes() == h.path_state(dir, m).tobytes()
                assert d.rays(dir, m)[0].tobytes() == h.rays(dir, m)[0].tobytes() and d.rays(dir, m)[1] == h.rays(dir, m)[1]
    for k, (a, b) in enumerate(zip(*got)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
    assert np.array_equal(np.concatenate([g[0] for g in got[0][:2]]), host_ul(1000)[:333])       # the round trip changed no byte


# ---- 8. the share split across the ray list -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def many(n_members, n, max_delay=64):
    """(rows int16[n_members, n, 2], per member None or a list of rays, plain paths): ray counts cycling 0, 1, 2, 7; mostly
    sparse rows and two dense ones"""
    rng = np.random.default_rng(n_members)
    rows = np.zeros((n_members, n, 2), np.int16)
    for m in range(n_members):
        if m % 3 != 2:
            at = int(rng.integers(0, n - 20))
            rows[m, at:at + 100] = rng.integers(-2047, 2048, size=rows[m, at:at + 100].shape)
    rows[5], rows[n_members - 1] = rng.integers(-30000, 30001, size=(2, n, 2))
    rows.setflags(write=False)

    def path():
        return dict(gain=float(rng.choice([0.0, 0.01, 0.25, 1.0, 3.7, 16.0])), delay=int(rng.integers(0, max_delay + 1)),
                    hz=float(rng.choice([0.0, 1.0, -1.0]) * rng.uniform(0.0, 500000.0)))

    plain = [path() for _ in range(n_members)]
    rays = [[dict(path(), phase=int(rng.integers(0, 1 << 32))) for _ in range((0, 1, 2, 7)[m % 4])] for m in range(n_members)]
    return rows, rays, plain


def pair_many(trx, n_members, rays, plain, rms=40.0):
    objs = trxhip.AirChannel(trx, n_members, 64, 9), trxhip.AirChannel(None, n_members, 64, 9)
    for o in objs:
        for d in (UL, DL):
            for m in range(n_members):
                o.set_path(d, m, **plain[m])
                o.set_rays(d, m, rays[m])
        o.set_noise(UL, 0, rms)
    return objs


@pytest.mark.parametrize("n_members, n", [(130, 200), (517, 64)])
def test_share_split(trx, n_members, n):
    """130 members hold 354 entries (a member without rays is one), 517 hold 1420: by ul_shares' rule (at least 8 entries to a share, enough
    shares to fill the chip) both windows split into dozens of shares of 8 or 9 entries, whose boundaries fall inside the members
    with 7 rays"""
    rows, rays, plain = many(n_members, n)
    d, h = pair_many(trx, n_members, rays, plain)
    first_ts = (1 << 32) - n // 2
    ref = h.uplink(rows, first_ts)
    y = ul_windows(d, rows, first_ts, [0, n], True)
    assert np.array_equal(y, ref), where(y, ref)
    assert 0.01 < (np.abs(ref.astype(np.int32)) >= 32767).mean() < 0.99
    d2, _ = pair_many(trx, n_members, rays, plain)
    y = ul_windows(d2, rows, first_ts, [0, 7, 40, n], True)              # other windows, other splits
    assert np.array_equal(y, ref), where(y, ref)
    if n_members == 130:
        x = np.ascontiguousarray(rows[5])
        for m in range(n_members):
            for o in (d, h):
                o.set_noise(DL, m, 7.0 + m)
        assert np.array_equal(d.downlink(dev(x), -3).cpu().numpy(), h.downlink(x, -3))


# ---- 9. the long-window instance ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotating", [True, False])
def test_long_window_without_the_share_split(trx, rotating):
    """as test_gpu_air's: from 262 144 samples on the uplink runs the instance that deals nothing to waves; two members with 2 and
    3 rays are 5 entries, one share; the second window is back in the split instance.  With rotating rays in the list the long
    window takes the instance with the tables in LDS, with none the one that never reads them"""
    rng = np.random.default_rng(262144)
    n = 262144 + 300
    rows = rng.integers(-9000, 9001, size=(2, n + 500, 2)).astype(np.int16)
    rows[1, 1000:200000] = 0
    rays = [[dict(gain=0.75, delay=17, hz=1234.5, phase=99), dict(gain=0.3, delay=0, hz=0.0, phase=1 << 31)],
            [dict(gain=1.0, delay=64, hz=-250000.0, phase=5), dict(gain=0.5, delay=3, hz=0.0), dict(gain=0.25, delay=33, hz=70.0, phase=1 << 20)]]
    if not rotating:
        rays = [[dict(r, hz=0.0) for r in rs] for rs in rays]
    objs = trxhip.AirChannel(trx, 2, 64, 4), trxhip.AirChannel(None, 2, 64, 4)
    for o in objs:
        for m in range(2):
            o.set_rays(UL, m, rays[m])
        o.set_noise(UL, 0, RMS)
    d, h = objs
    ts = (1 << 32) - 1000
    ref = np.concatenate([h.uplink(np.ascontiguousarray(rows[:, :n]), ts), h.uplink(np.ascontiguousarray(rows[:, n:]), ts + n)])
    y = ul_windows(d, rows, ts, [0, n, n + 500], True)
    assert np.array_equal(y, ref), where(y, ref)


# ---- 10. the ring ---------------------------------------------------------------------------------------------------------------------------

def test_two_rays_40000_samples_apart(trx):
    rng = np.random.default_rng(70000)
    rows = rng.integers(-9000, 9001, size=(1, 70000, 2)).astype(np.int16)
    rays = [dict(gain=1.0, delay=0, hz=0.0, phase=0), dict(gain=0.75, delay=40000, hz=-33333.3, phase=1 << 29)]
    objs = trxhip.AirChannel(trx, 1, 65536, 3), trxhip.AirChannel(None, 1, 65536, 3)
    for o in objs:
        for dir in (UL, DL):
            o.set_rays(dir, 0, rays)
            o.set_noise(dir, 0, RMS)
    d, h = objs
    ref = h.uplink(rows, -20000)
    y = ul_windows(d, rows, -20000, [0, 30000, 30001, 45000, 70000], True)    # n < delay, and the ring wraps
    assert np.array_equal(y, ref), where(y, ref)
    x = rows[0]
    parts = [d.downlink(dev(x[a:b]), 5 + a).cpu().numpy() for a, b in ((0, 25000), (25000, 70000))]
    assert np.array_equal(np.concatenate(parts, axis=1), h.downlink(x, 5))


# ---- 11. one member per ray on the object as it was ------------------------------------------------------------------------------------------

def test_rays_equal_one_member_per_ray_on_the_device(trx):
    """40 members x 6 rays at phase 0 set at end_ts = t0, against the existing kernels under 240 members fed
    torch.repeat_interleave rows with set_path at the same end_ts; no host loop takes part"""
    import torch
    rng = np.random.default_rng(240)
    n_m, n_r, n, t0 = 40, 6, 1300, (1 << 32) - 650
    rows = rng.integers(-3000, 3001, size=(n_m, n, 2)).astype(np.int16)
    rows[::3, 200:900] = 0
    rays = [[dict(gain=float(rng.choice([0.1, 0.5, 1.0, 4.0])), delay=int(rng.integers(0, 49)),
                  hz=float(rng.choice([0.0, 0.0, 1.0, -1.0]) * rng.uniform(0.0, 3000.0)), phase=0) for _ in range(n_r)] for _ in range(n_m)]
    a, b = trxhip.AirChannel(trx, n_m, 48, 8), trxhip.AirChannel(trx, n_m * n_r, 48, 8)
    for o in (a, b):
        o.reset(UL, t0)
        o.set_noise(UL, 0, RMS)
    for m in range(n_m):
        a.set_rays(UL, m, rays[m])
        for k, r in enumerate(rays[m]):
            b.set_path(UL, m * n_r + k, r["gain"], r["delay"], r["hz"])
    d_rows = dev(rows)
    out = []
    for lo, hi in ((0, 700), (700, n)):
        w = d_rows[:, lo:hi].contiguous()
        out.append((a.uplink(w, t0 + lo), b.uplink(torch.repeat_interleave(w, n_r, dim=0), t0 + lo)))
    for k, (y, z) in enumerate(out):
        assert torch.equal(y, z) and bool(y.any()), k


# ---- 12. a direction without rays -----------------------------------------------------------------------------------------------------------

def test_a_direction_without_rays_is_untouched(trx):
    x = rows3()[0]
    a, b = trxhip.AirChannel(trx, 3, MAX_DELAY, SEED), trxhip.AirChannel(trx, 3, MAX_DELAY, SEED)
    case1(a, dirs=(UL,))
    for o in (a, b):
        o.set_path(DL, 0, **PLAIN0)
        o.set_path(DL, 2, gain=1.5, delay=40, hz=-67.7)
        for m in range(3):
            o.set_noise(DL, m, RMS)
    a.uplink(dev(rows3()), 0)
    y = [o.downlink(dev(x), -300).cpu().numpy() for o in (a, b)]
    assert np.array_equal(y[0], y[1]) and y[0].any()


# ---- 13. the two loops through a dispersive channel -----------------------------------------------------------------------------------------

def dispersive_uplink(trx, use_va):
    """test_gpu_air's uplink loop -- the same 18 bursts, TNs, delays and TAs -- behind tests/air_rays_loop.py's two rays per member,
    the radio reading 20 samples early.  Returns (found, wrong hard bits 3 .. 144) per sent burst"""
    import torch
    import air_rays_loop as RL
    import ms_tx_model as M
    member, fn, tn, bits = RL.bursts()
    g = trxhip.MsTxSchedulerGroup(trx, n_members=3, tx_full_scale=2047, rxtx_delay=RL.UL_RXTX_DELAY, max_pending=32)
    for m in range(3):
        g.set_ta(m, RL.UL_TA[m])
    plan = g.submit(member, trxhip.ms_tx_requests(fn, tn, 0, bits), [RL.CLOCK] * 3)
    assert (plan["status"] == M.QUEUED).all()
    rows, nd = g.render(RL.N, RL.CLOCK[2])
    assert nd == [RL.FRAMES] * 3
    y = RL.air_of(trx, RL.G2).uplink(rows, RL.CLOCK[2])
    ul = M.Time(RL.CLOCK[0], RL.CLOCK[1]).decTN(3)
    rx = trxhip.RxScheduler(trx, chans=1, tsc=RL.TSC, exact=not use_va, full_scale=2047.0, max_slots=1024, use_va=use_va)
    rx.set_clock(ul.fn, ul.tn)
    rx.set_max_toa(20, 63)
    rx.set_trxd_version(0, 1)
    for t in range(8):
        rx.set_slot(0, t, 1)
    pkt, plen, ind, _ = rx.pull(y)
    torch.cuda.synchronize()
    pkt, plen, ind = pkt.cpu().numpy()[0], plen.cpu().numpy()[0], rx.ind_to_numpy(ind)[0]
    order = []
    for i in range(len(fn)):
        k = np.flatnonzero((ind["fn"] == fn[i]) & (ind["tn"] == tn[i]))
        assert len(k) == 1
        order.append(k[0])
    hard = (pkt[order][:, 11:11 + 148] > 127).astype(np.uint8)
    return (plen == 11 + 148)[order] & (ind["rc"][order] > 0), (hard[:, 3:145] != bits[:, 3:145]).sum(axis=1)


def test_uplink_loop_through_the_echo(trx):
    """MS group -> uplink() under {1, d} + {0.5, d + 8 samples, a quarter turn} per member -> RxScheduler(use_va=True): every
    slot found, no bit wrong; the plain demodulator on the same stream has the oracle's count of wrong bits"""
    import air_rays_loop as RL
    found, wrong = dispersive_uplink(trx, True)
    print("use_va: found", int(found.sum()), "wrong bits", wrong.tolist())
    assert found.all() and not wrong.any()
    found_p, wrong_p = dispersive_uplink(trx, False)
    want = RL.oracle_uplink(RL.G2)[False]
    print("plain: found", int(found_p.sum()), "wrong bits", int(wrong_p.sum()), "the oracle's", int(want[1].sum()))
    assert np.array_equal(found_p, want[0]) and int(wrong_p.sum()) == int(want[1].sum())


DL_G2 = 0.5


def dispersive_downlink(trx, g2):
    """test_gpu_air's downlink loop behind two rays per member and noise rms 20.  Returns per member (acquired, the SCH slot of the
    rest decoded, traffic slots with every bit right, traffic slots judged)"""
    import air_rays_loop as RL
    import ms_fsearch_cases as FC
    x, _, sent = FC.cell(7301, 25.0, 0.0, 24, 0, 0x0F)
    hz, delay = (2000.0, -1500.0), (3, 11)
    air = trxhip.AirChannel(trx, 2, max_delay=32, seed=5)
    for m in range(2):
        air.set_rays(DL, m, RL.two_rays(delay[m], g2, hz[m]))
        air.set_noise(DL, m, 20.0)
    g = trxhip.MsRxSchedulerGroup(trx, 2, rx_full_scale=FC.FULL, tsc=FC.TSC, active_tns=[0x0F, 0x0F], tracking=True)
    d_x = dev(x)
    found, rec, hit, _ = g.acquire_afc([0, 1], air.downlink(d_x[:FC.ACQ_LEN], 0), first_ts=0)
    out = []
    acquired = [bool(found[m]) and hit["found"][m] == 1 and rec[m]["rc"] == 1 and rec[m]["bsic"] == FC.BSIC for m in range(2)]
    if not all(acquired):
        return [(a, False, 0, 0) for a in acquired]
    rest = air.downlink(d_x[FC.ACQ_LEN:], FC.ACQ_LEN)
    res, _ = g.pull([rest[0], rest[1]], first_ts=FC.ACQ_LEN)
    for m in range(2):
        ind, sb = trxhip.MsRxScheduler.ind_to_numpy(res[m][0]), res[m][1].cpu().numpy()
        sch = ind[ind["kind"] == trxhip.MS_KIND_SCH]
        sch_ok = [(int(r["sch_rc"]), int(r["sch_fn"]), int(r["sch_bsic"])) for r in sch] == [(1, FC.FN0 + 21, FC.BSIC)]
        ok = [bool(((sb[i] < 0) == (sent[(int(r["fn"]), int(r["tn"]))] > 0)).all()) for i, r in enumerate(ind)
              if r["kind"] == trxhip.MS_KIND_NB and (int(r["fn"]), int(r["tn"])) in sent]
        out.append((True, sch_ok, sum(ok), len(ok)))
    return out


def test_downlink_loop_through_the_echo(trx):
    """the cell of test_gpu_air's downlink loop through the same two rays per member (at the member's +2000 / -1500 Hz) and noise
    rms 20: acquire_afc() finds both, every SCH slot and every ACTIVE traffic bit decodes through the 16-state MLSE receiver"""
    res = dispersive_downlink(trx, DL_G2)
    print("downlink loop, g2", DL_G2, res)
    for m, (acquired, sch_ok, n_ok, n) in enumerate(res):
        assert acquired and sch_ok and n >= 11 * 3 and n_ok == n, (m, res)
