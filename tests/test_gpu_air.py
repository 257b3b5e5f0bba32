"""The air interface on the MI355X (trxhip_air_*, AirChannel; csrc/trx_air.hip): the device object byte-identical to the host
object -- the plain loop over the same inline functions, itself pinned to the numpy model in tests/test_air_cpu.py -- on the CPU
cases, across the member split of the uplink kernel and over a long single row, and the two loops the object closes on the
device: an MS uplink group through uplink() into the BTS-side receiver, and a cell's downlink through downlink() into a cold-
starting MS group."""
import functools

import numpy as np
import pytest

import ms_tx_model as M
from osmo_trx_amd import trxhip
from test_air_cpu import CHUNKS, FIRST_TS, MAX_DELAY, N, PATHS, RMS, SEED, rows3

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


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")


def pair(trx, n, max_delay, seed, paths, rms=RMS):
    """(device object, host object) with the same paths and noise in both directions"""
    objs = trxhip.AirChannel(trx, n, max_delay, seed), trxhip.AirChannel(None, n, max_delay, seed)
    for o in objs:
        for d in (UL, DL):
            for k, p in enumerate(paths):
                o.set_path(d, k, **p)
                if d == DL or k == 0:
                    o.set_noise(d, k, rms)
    return objs


def ul_windows(o, rows, first_ts, cuts, on_device):
    """the uplink of rows[:, a:b] for consecutive cuts, concatenated: numpy int16[n, 2]"""
    import torch
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        w = np.ascontiguousarray(rows[:, a:b])
        out.append(o.uplink(dev(w) if on_device else w, first_ts + a))
    if on_device:
        y = torch.cat(out).cpu().numpy()                            # the copy waits for the stream
        return y
    return np.concatenate(out)


def cuts_of(n, chunk):
    return list(range(0, n, chunk)) + [n]


@functools.lru_cache(maxsize=None)
def host_ul(first_ts):
    h = trxhip.AirChannel(None, 3, MAX_DELAY, SEED)
    for k, p in enumerate(PATHS):
        h.set_path(UL, k, **p)
    h.set_noise(UL, 0, RMS)
    y = h.uplink(rows3(), first_ts)
    y.setflags(write=False)
    return y


# ---- 1. the CPU cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_uplink_equals_the_host_object(trx, first_ts):
    d, _ = pair(trx, 3, MAX_DELAY, SEED, PATHS)
    y = ul_windows(d, rows3(), first_ts, [0, N], True)
    assert np.array_equal(y, host_ul(first_ts)) and y.any()
    assert d.path_state(UL, 0)["end_ts"] == first_ts + N


@pytest.mark.parametrize("chunk", CHUNKS)
def test_uplink_chunking_changes_no_bit(trx, chunk):
    first_ts = (1 << 32) - 100
    d, _ = pair(trx, 3, MAX_DELAY, SEED, PATHS)
    y = ul_windows(d, rows3(), first_ts, cuts_of(N, chunk), True)
    assert np.array_equal(y, host_ul(first_ts)), np.flatnonzero((y != host_ul(first_ts)).any(axis=1))[:8]


def test_set_path_and_reset_between_windows(trx):
    import torch
    d, h = pair(trx, 3, MAX_DELAY, SEED, PATHS)
    x = rows3()
    got = [[], []]
    for k, (lo, hi) in enumerate(((0, 300), (300, 520), (520, N))):
        for j, o in enumerate((d, h)):
            if k == 1:
                o.set_path(UL, 1, gain=0.5, delay=31, hz=-1234.5)
                o.set_path(UL, 2, gain=2.0, delay=0, hz=0.0)
            if k == 2:
                o.set_path(UL, 2, gain=2.0, delay=48, hz=500000.0)
                o.set_noise(UL, 0, 100.0)
            w = np.ascontiguousarray(x[:, lo:hi])
            y = o.uplink(dev(w) if j == 0 else w, 1000 + lo)
            got[j].append(y.cpu().numpy() if j == 0 else y)
        for m in range(3):
            assert d.path_state(UL, m).tobytes() == h.path_state(UL, m).tobytes()
    for o in (d, h):
        o.reset(UL, -50)
    w = np.ascontiguousarray(x[:, :100])
    got[0].append(d.uplink(dev(w), -50).cpu().numpy())
    got[1].append(h.uplink(w, -50))
    with pytest.raises(trxhip.TrxHipError):
        d.uplink(dev(w), 49)                                        # not contiguous: end_ts is 50
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(*got)):
        assert np.array_equal(a, b), k


@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_downlink_equals_the_host_object(trx, first_ts):
    d, h = pair(trx, 3, MAX_DELAY, SEED, PATHS)
    x = rows3()[0]
    ref = h.downlink(x, first_ts)
    assert np.array_equal(d.downlink(dev(x), first_ts).cpu().numpy(), ref)
    d2, _ = pair(trx, 3, MAX_DELAY, SEED, PATHS)
    parts = [d2.downlink(dev(x[k:k + 63]), first_ts + k) for k in range(0, N, 63)]
    assert np.array_equal(np.concatenate([p.cpu().numpy() for p in parts], axis=1), ref)


def test_identity_rounding_and_clamp(trx):
    x = rows3()[0]
    a = trxhip.AirChannel(trx, 1)
    assert np.array_equal(a.uplink(dev(x[None]), -77).cpu().numpy(), x)
    assert np.array_equal(a.downlink(dev(x), 1 << 40).cpu().numpy()[0], x)
    for acc, out in ((-129, -1), (-128, 0), (127, 0), (128, 1)):
        a = trxhip.AirChannel(trx, 1)
        a.set_path(UL, 0, abs(acc) / 256.0, 0, 0.0)
        a.set_path(DL, 0, abs(acc) / 256.0, 0, 0.0)
        s = np.array([[np.sign(acc), 0], [0, np.sign(acc)]], dtype=np.int16)
        want = np.array([[out, 0], [0, out]], dtype=np.int16)
        assert np.array_equal(a.uplink(dev(s[None]), 0).cpu().numpy(), want) and np.array_equal(a.downlink(dev(s), 0).cpu().numpy()[0], want)
    rails = np.array([[32767, -32768], [-32768, 32767]], dtype=np.int16)
    a = trxhip.AirChannel(trx, 2)
    assert np.array_equal(a.uplink(dev(np.stack([rails, rails])), 0).cpu().numpy(), rails)


# ---- 2. across the member split, and a long row -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def many(n_members, n=1300, max_delay=64):
    """(rows int16[n_members, n, 2], paths): mostly zero rows with a few bursts of 148 * 4 samples, each member on its own path"""
    rng = np.random.default_rng(n_members)
    rows = np.zeros((n_members, n, 2), np.int16)
    for m in range(n_members):
        if m % 3 != 2:
            at = int(rng.integers(0, n - 100))
            rows[m, at:at + 592] = rng.integers(-2047, 2048, size=rows[m, at:at + 592].shape)
    rows[5], rows[n_members - 1] = rng.integers(-30000, 30001, size=(2, n, 2))      # two dense rows, one in the last share
    paths = [dict(gain=float(rng.choice([0.0, 0.01, 0.25, 1.0, 3.7, 16.0])), delay=int(rng.integers(0, max_delay + 1)),
                  hz=float(rng.choice([0.0, 1.0, -1.0]) * rng.uniform(0.0, 500000.0))) for _ in range(n_members)]
    rows.setflags(write=False)
    return rows, paths


@pytest.mark.parametrize("n_members", [130, 517])
def test_member_split(trx, n_members):
    rows, paths = many(n_members)
    d, h = pair(trx, n_members, 64, 9, paths, rms=40.0)
    first_ts = (1 << 32) - 650
    ref = h.uplink(rows, first_ts)
    y = ul_windows(d, rows, first_ts, [0, 1300], True)
    assert np.array_equal(y, ref), np.flatnonzero((y != ref).any(axis=1))[:8]
    assert 0.01 < (np.abs(ref.astype(np.int32)) >= 32767).mean() < 0.99
    d2, _ = pair(trx, n_members, 64, 9, paths, rms=40.0)
    y = ul_windows(d2, rows, first_ts, [0, 7, 64, 700, 1300], True)      # other windows, other splits
    assert np.array_equal(y, ref), np.flatnonzero((y != ref).any(axis=1))[:8]
    if n_members == 130:
        x = np.ascontiguousarray(rows[5])
        assert np.array_equal(d.downlink(dev(x), -3).cpu().numpy(), h.downlink(x, -3))


def test_one_member_over_70000_samples(trx):
    rng = np.random.default_rng(70000)
    rows = rng.integers(-9000, 9001, size=(1, 70000, 2)).astype(np.int16)
    paths = [dict(gain=1.5, delay=40000, hz=-33333.3)]
    d, h = pair(trx, 1, 65536, 3, paths)
    ref = h.uplink(rows, -20000)
    assert np.array_equal(ul_windows(d, rows, -20000, [0, 70000], True), ref) and ref[40000:].any() and np.abs(ref[:40000]).max() < 100
    d2, _ = pair(trx, 1, 65536, 3, paths)
    assert np.array_equal(ul_windows(d2, rows, -20000, [0, 30000, 30001, 70000], True), ref)      # n < d, and the ring wraps
    x = rows[0]
    assert np.array_equal(d.downlink(dev(x), 5).cpu().numpy(), h.downlink(x, 5))


def test_long_window_without_the_member_split(trx):
    """from 4 blocks of 256 samples per CU on (262 144 samples on 256 CUs) the uplink runs the instance that deals no members to
    waves; two members, the second window back in the split instance"""
    rng = np.random.default_rng(262144)
    n = 262144 + 300
    rows = rng.integers(-9000, 9001, size=(2, n + 500, 2)).astype(np.int16)
    rows[1, 1000:200000] = 0
    paths = [dict(gain=0.75, delay=17, hz=1234.5), dict(gain=1.0, delay=64, hz=-250000.0)]
    d, h = pair(trx, 2, 64, 4, paths)
    ts = (1 << 32) - 1000
    ref = np.concatenate([h.uplink(np.ascontiguousarray(rows[:, :n]), ts), h.uplink(np.ascontiguousarray(rows[:, n:]), ts + n)])
    y = ul_windows(d, rows, ts, [0, n, n + 500], True)
    assert np.array_equal(y, ref), np.flatnonzero((y != ref).any(axis=1))[:8]


# ---- 3. the uplink loop: MS group -> uplink() -> RxScheduler -------------------------------------------------------------------------------

UL_TNS, UL_DELAYS, UL_TA = (1, 2, 5), (0, 8, 20), (0, 2, 5)
# the radio's calibration: with rxtx_delay 0 this loop reads a TOA of 4.63 symbols for an MS at no distance (what
# test_gpu_ms_tx's loopback reads too, it compares differences); 18 samples earlier the same MS reads 0.13
UL_RXTX_DELAY = -18


def uplink_loop(trx, ta):
    """three MSs on TNs 1, 2 and 5 behind delays of 0, 8 and 20 samples, noise rms 12 at the BTS.  Returns (found, wrong hard bits
    3 .. 144, toa) per sent slot, and the member of each"""
    import torch
    from test_gpu_tx_frontend import _unambiguous_bursts
    tsc, frames, clock = 5, 6, (5000, 2, 40 * 625)
    rng = np.random.default_rng(77)
    member = np.tile(np.arange(3), frames)
    fn = np.repeat(clock[0] + 2 + np.arange(frames), 3)
    tn = np.asarray(UL_TNS)[member]
    bits = _unambiguous_bursts(np.full(len(fn), tsc), rng)
    g = trxhip.MsTxSchedulerGroup(trx, n_members=3, tx_full_scale=2047, rxtx_delay=UL_RXTX_DELAY, max_pending=32)
    air = trxhip.AirChannel(trx, 3, max_delay=32, seed=1)
    for m in range(3):
        g.set_ta(m, ta[m])
        air.set_path(UL, m, 1.0, UL_DELAYS[m], 0.0)
    air.set_noise(UL, 0, 12.0)
    plan = g.submit(member, trxhip.ms_tx_requests(fn, tn, 0, bits), [clock] * 3)
    assert (plan["status"] == M.QUEUED).all()
    n_slots = (frames + 4) * 8
    n = n_slots * 625 + 1
    rows, nd = g.render(n, clock[2])
    assert nd == [frames] * 3
    y = air.uplink(rows, clock[2])
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
    order = []
    for i in range(len(fn)):
        k = np.flatnonzero((ind["fn"] == fn[i]) & (ind["tn"] == tn[i]))
        assert len(k) == 1
        order.append(k[0])
    hard = (pkt[order][:, 11:11 + 148] > 127).astype(np.uint8)
    return (plen == 11 + 148)[order], (hard[:, 3:145] != bits[:, 3:145]).sum(axis=1), ind["toa"][order], member


def test_uplink_loop(trx):
    found, wrong, toa, member = uplink_loop(trx, UL_TA)
    print("uplink loop, TA set: toa per member", [np.round(toa[member == m], 3).tolist() for m in range(3)])
    assert found.all() and not wrong.any()
    assert np.abs(toa).max() < 1.0
    found0, wrong0, toa0, _ = uplink_loop(trx, (0, 0, 0))
    print("uplink loop, TA left out: toa per member", [np.round(toa0[member == m], 3).tolist() for m in range(3)])
    assert found0.all()
    # a delay of 20 samples is 5 symbols; the estimate of one burst moves by that within a quarter symbol at this noise
    assert np.abs(toa0[member == 2] - toa[member == 2] - 5.0).max() < 0.25
    assert np.abs(toa0[member == 1] - toa[member == 1] - 2.0).max() < 0.25
    assert np.abs(toa0[member == 0] - toa[member == 0]).max() < 0.25


# ---- 4. the downlink loop: a cell -> downlink() -> a cold-starting MS group -------------------------------------------------------------------

def test_downlink_loop(trx):
    """the cell of the cold-start test (ms_fsearch_cases.cell(7301, ...), 24 frames, traffic on TN 0 .. 3) leaves the BTS on
    frequency; the paths put member 0 at +2000 Hz behind 3 samples and member 1 at -1500 Hz behind 11, each receiver adds noise of
    rms 20.  No frequency is given to the MSs"""
    import ms_fsearch_cases as FC
    x, _, sent = FC.cell(7301, 25.0, 0.0, 24, 0, 0x0F)
    hz, delay = (2000.0, -1500.0), (3, 11)
    air = trxhip.AirChannel(trx, 2, max_delay=16, seed=5)
    for m in range(2):
        air.set_path(DL, m, 1.0, delay[m], hz[m])
        air.set_noise(DL, m, 20.0)
    g = trxhip.MsRxSchedulerGroup(trx, 2, rx_full_scale=FC.FULL, tsc=FC.TSC, active_tns=[0x0F, 0x0F], tracking=True)
    d_x = dev(x)
    acq = air.downlink(d_x[:FC.ACQ_LEN], 0)
    found, rec, hit, fc = g.acquire_afc([0, 1], acq, first_ts=0)
    print("downlink loop: nco", [round(g.nco_state(m)["hz"], 1) for m in range(2)], "sch fn", [int(r["fn"]) for r in rec])
    assert list(found) == [True, True] and list(hit["found"]) == [1, 1]
    for m in range(2):
        assert rec[m]["rc"] == 1 and rec[m]["bsic"] == FC.BSIC and rec[m]["fn"] in (FC.FN0 + 1, FC.FN0 + 11)
        assert g.nco_state(m)["enable"] and abs(g.nco_state(m)["hz"] + hz[m]) <= 100.0
    rest = air.downlink(d_x[FC.ACQ_LEN:], FC.ACQ_LEN)
    res, k = g.pull([rest[0], rest[1]], first_ts=FC.ACQ_LEN)
    for m in range(2):
        ind, sb = trxhip.MsRxScheduler.ind_to_numpy(res[m][0]), res[m][1].cpu().numpy()
        sch = ind[ind["kind"] == trxhip.MS_KIND_SCH]
        assert [(int(r["sch_rc"]), int(r["sch_fn"]), int(r["sch_bsic"])) for r in sch] == [(1, FC.FN0 + 21, FC.BSIC)], m
        ok = [bool(((sb[i] < 0) == (sent[(int(r["fn"]), int(r["tn"]))] > 0)).all()) for i, r in enumerate(ind)
              if r["kind"] == trxhip.MS_KIND_NB and (int(r["fn"]), int(r["tn"])) in sent]
        assert len(ok) >= 11 * 3 and all(ok), (m, len(ok), sum(ok))
