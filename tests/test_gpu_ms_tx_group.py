"""The MS-side uplink scheduler group on the MI355X (trxhip_ms_tx_group_*, MsTxSchedulerGroup; ms_tx_stage_kernel,
ms_tx_render_group_kernel): every int16 of every member's window against the row modulator's rows laid where the plans put them
-- wherever the bursts lie in the tiles and however the windows cut them --, and the window, its state() and its n_drawn against a
MsTxScheduler fed the same requests and windows (the same host object as a group of one: the row modulator is the yardstick
that shares nothing with it), nothing written outside a window, and refusals that move nothing."""
import ctypes as C

import numpy as np
import pytest

import ms_tx_model as M
from osmo_trx_amd import trxhip
from test_gpu_ms_tx import expected_stream, rows_of, some_bits

pytestmark = pytest.mark.gpu

MARK = 0x5A5A
CLOCK = (1000, 2, 123457)


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = trxhip.TrxHip(0)
    yield t
    t.close()


class Out:
    """the group's output with a guard row before and after it, all sentinel; shift: samples the output starts behind an aligned
    address"""

    def __init__(self, n, stride, shift=0):
        import torch
        self.n, self.stride, self.shift = n, stride, shift
        self.flat = torch.full(((n + 2) * stride + 2, 2), MARK, dtype=torch.int16, device="cuda:0")
        self.out = self.flat[stride + shift:stride + shift + n * stride].view(n, stride, 2)

    def windows(self, sizes):
        """the members' windows as numpy, after a check that nothing else was written"""
        import torch
        torch.cuda.synchronize()
        a = self.flat.cpu().numpy()
        lo = self.stride + self.shift
        assert (a[:lo] == MARK).all() and (a[lo + self.n * self.stride:] == MARK).all(), "wrote outside the output"
        rows = a[lo:lo + self.n * self.stride].reshape(self.n, self.stride, 2)
        for m, k in enumerate(sizes):
            assert (rows[m, k:] == MARK).all(), "member %d: wrote behind its window" % m
        return [rows[m, :k].copy() for m, k in enumerate(sizes)]

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.flat == MARK).all())


def single_render(tx, n, first_ts):
    import torch
    buf = torch.full((n + 16, 2), MARK, dtype=torch.int16, device="cuda:0")
    _, nd = tx.render(n, first_ts, out=buf[8:])
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:8] == MARK).all() and (a[8 + n:] == MARK).all()
    return a[8:8 + n], nd


class Pair:
    """a group and one MsTxScheduler per member, fed the same; bursts[m]: the (radio_ts, row of the row modulator) of every burst
    member m has queued"""

    def __init__(self, trx, n, fs=9830, delay=-67, max_pending=64):
        self.trx, self.n = trx, n
        self.bursts = [[] for _ in range(n)]
        self.group = trxhip.MsTxSchedulerGroup(trx, n_members=n, tx_full_scale=fs, rxtx_delay=delay, max_pending=max_pending)
        self.single = [trxhip.MsTxScheduler(trx, tx_full_scale=fs, rxtx_delay=delay, max_pending=max_pending) for _ in range(n)]

    def set_ta(self, m, val):
        self.group.set_ta(m, val)
        self.single[m].set_ta(val)

    def submit(self, members, reqs, clocks):
        members = [int(x) for x in np.broadcast_to(members, (len(reqs),))]
        plan = self.group.submit(members, reqs, clocks)
        for m in sorted(set(members)):
            idx = [i for i, x in enumerate(members) if x == m]
            assert plan[idx].tobytes() == self.single[m].submit(reqs[idx], clocks[m]).tobytes(), m
        queued = np.flatnonzero(plan["status"] == M.QUEUED)
        if len(queued):
            rows = rows_of(self.trx, reqs["bits"][queued], reqs["tn"][queued], plan["scale"][queued])
            for i, row in zip(queued, rows):
                self.bursts[members[i]].append((int(plan["radio_ts"][i]), row))
        return plan

    def render(self, sizes, first_ts, stride=None, shift=0):
        """one group render against the row modulator's rows where the plans put them, and against the members' single renders:
        windows, n_drawn, states.  Returns the windows."""
        stride = stride or max(max(sizes), 1) + 3
        o = Out(self.n, stride, shift)
        _, nd = self.group.render(sizes, first_ts, out=o.out)
        got = o.windows(sizes)
        for m, k in enumerate(sizes):
            if k:
                want, nd_s = single_render(self.single[m], k, first_ts[m])
                assert nd[m] == nd_s, (m, nd, nd_s)
                assert np.array_equal(got[m], want), (m, k, np.flatnonzero((got[m] != want).any(axis=1))[:8])
                want = expected_stream(k, first_ts[m], self.bursts[m])
                assert np.array_equal(got[m], want), (m, k, np.flatnonzero((got[m] != want).any(axis=1))[:8])
            else:
                assert nd[m] == 0
            assert self.group.state(m).tobytes() == self.single[m].state().tobytes(), m
        return got


def dense(rng, frames, skip_tn=None, fn0=1003):
    """a burst on every TN (but skip_tn) of `frames` frames"""
    fn = np.repeat(fn0 + np.arange(frames), 8)
    tn = np.tile(np.arange(8), frames)
    keep = tn != skip_tn
    fn, tn = fn[keep], tn[keep]
    return trxhip.ms_tx_requests(fn, tn, (np.arange(len(fn)) * 7) % 35, some_bits(rng, len(fn)))


LENGTHS = (0, 1, 3, 624, 625, 626, 1249, 1251, 4999)


@pytest.mark.parametrize("n", [5, 10])
def test_byte_identity(trx, n):
    """n members with their own clocks, timing advances and traffic, four renders whose window lengths go through LENGTHS (with 10
    members all nine in one render), out_stride larger than any window, from an aligned and from an odd output"""
    rng = np.random.default_rng(300 + n)
    pair = Pair(trx, n)
    clocks = [(1000 + 3 * m, m % 8, 123457 + 1111 * m) for m in range(n)]
    members, reqs = [], []
    for m in range(n):
        pair.set_ta(m, (5 * m) % 23 - 7)
        r = dense(rng, 4, skip_tn=m % 8, fn0=clocks[m][0] + 2)
        members += [m] * len(r)
        reqs.append(r)
    reqs = np.concatenate(reqs)
    # members mixed in one submit, each member's requests in their order: the members of a random permutation, each taking its next
    by_member = {m: iter([i for i in range(len(reqs)) if members[i] == m]) for m in range(n)}
    mixed = [next(by_member[members[i]]) for i in rng.permutation(len(reqs))]
    plan = pair.submit([members[i] for i in mixed], reqs[mixed], clocks)
    assert (plan["status"] == M.QUEUED).all()
    at = [int(plan["radio_ts"][[i for i, j in enumerate(mixed) if members[j] == m]].min()) - 100 - m for m in range(n)]
    drawn = 0
    for k in range(4):
        sizes = [LENGTHS[(m + 5 * k) % len(LENGTHS)] for m in range(n)]
        if n == 10 and k == 0:
            assert set(sizes) == set(LENGTHS)
        got = pair.render(sizes, at, stride=5003, shift=k & 1)
        drawn += sum(int(w.any()) for w in got)
        at = [a + s for a, s in zip(at, sizes)]
    assert drawn >= n                                               # the windows met bursts, not zeros alone


@pytest.mark.parametrize("shift", [0, 1])
def test_alignment_classes(trx, shift):
    """bursts that begin 0, 1, 2 and 3 samples into their windows, rows an odd number of samples apart, from an aligned and an odd
    output: byte offsets 0, 4, 8, 12 mod 16 of a burst's first sample, from even and odd window starts"""
    rng = np.random.default_rng(11)
    pair = Pair(trx, 8)
    plan = pair.submit(np.arange(8), trxhip.ms_tx_requests(1003, 4, 0, some_bits(rng, 8)), [CLOCK] * 8)
    ts = int(plan["radio_ts"][0])
    got = pair.render([m % 4 + 625 + 7 for m in range(8)], [ts - m % 4 for m in range(8)], stride=641, shift=shift)
    for m in range(8):
        assert got[m][m % 4:m % 4 + 625].any() and not got[m][:m % 4].any() and not got[m][m % 4 + 625:].any()


def test_straddle_the_window_ends(trx):
    """a burst crosses the end of one window and the start of the next, split after 1, 2, 3, 312, 623 and 624 samples"""
    cuts = (1, 2, 3, 312, 623, 624)
    rng = np.random.default_rng(12)
    pair = Pair(trx, len(cuts))
    bits = some_bits(rng, 1)
    plan = pair.submit(np.arange(len(cuts)), trxhip.ms_tx_requests(1003, 4, 12, np.repeat(bits, len(cuts), axis=0)), [CLOCK] * len(cuts))
    ts = int(plan["radio_ts"][0])
    row = rows_of(trx, bits, 4, plan["scale"][:1])[0]
    a = pair.render([40 + c for c in cuts], [ts - 40] * len(cuts))
    assert [int(pair.group.state(m)["pending"]) for m in range(len(cuts))] == [1] * len(cuts)
    b = pair.render([625 - c + 40 for c in cuts], [ts + c for c in cuts], shift=1)
    for m in range(len(cuts)):
        whole = np.concatenate([a[m], b[m]])
        assert np.array_equal(whole[40:665], row) and not whole[:40].any() and not whole[665:].any()
        assert pair.group.state(m)["drawn"] == 1


def test_bursts_at_the_tile_boundary(trx):
    """a burst begins one sample before a tile boundary, exactly at it and one sample after it; the tiles behind it hold its tail
    and then nothing; the last tile is shorter than 625"""
    rng = np.random.default_rng(13)
    pair = Pair(trx, 3)
    bits = some_bits(rng, 1)
    plan = pair.submit(np.arange(3), trxhip.ms_tx_requests(1003, 4, 0, np.repeat(bits, 3, axis=0)), [CLOCK] * 3)
    ts = int(plan["radio_ts"][0])
    row = rows_of(trx, bits, 4, plan["scale"][:1])[0]
    got = pair.render([2000] * 3, [ts - 624, ts - 625, ts - 626])
    for m, lead in enumerate((624, 625, 626)):
        assert np.array_equal(got[m], expected_stream(2000, ts - lead, [(ts, row)]))


@pytest.mark.parametrize("lead", [300, 0, 624])
def test_two_bursts_in_one_tile(trx, lead):
    """adjacent TNs that touch, and with a gap of 4 and of 20 samples from a falling timing advance: the tile behind the first
    holds a tail, a gap (or none) and a head; the window's third tile holds the second burst's tail and zeros, the fourth none"""
    rng = np.random.default_rng(14)
    pair = Pair(trx, 3, delay=0)
    bits = some_bits(rng, 6)
    for m in range(3):
        pair.set_ta(m, 10)
    a = pair.submit(np.arange(3), trxhip.ms_tx_requests(1003, 4, 0, bits[:3]), [CLOCK] * 3)
    for m, ta in enumerate((10, 9, 5)):
        pair.set_ta(m, ta)
    b = pair.submit(np.arange(3), trxhip.ms_tx_requests(1003, 5, 15, bits[3:]), [CLOCK] * 3)
    assert [int(y - x) for x, y in zip(a["radio_ts"], b["radio_ts"])] == [625, 629, 645]
    ts = int(a["radio_ts"][0])
    rows_a, rows_b = rows_of(trx, bits[:3], [4] * 3, a["scale"]), rows_of(trx, bits[3:], [5] * 3, b["scale"])
    got = pair.render([2400] * 3, [ts - lead] * 3, shift=lead & 1)
    for m in range(3):
        want = expected_stream(2400, ts - lead, [(ts, rows_a[m]), (int(b["radio_ts"][m]), rows_b[m])])
        assert np.array_equal(got[m], want), m
        assert pair.group.state(m)["drawn"] == 2


def traffic(rng):
    """8 frames, a burst on 5 of the 8 TNs, mixed pwr, two falling timing-advance changes: (ta, requests) steps"""
    clock = (2715640, 5, 1 << 35)                       # the FN wraps inside the run
    steps = []
    for ta, frames in ((9, (1, 2, 3)), (4, (4, 5)), (0, (6, 7, 8))):
        fn = [(clock[0] + f) % M.HYPERFRAME for f in frames for _ in range(5)]
        tn = [t for _ in frames for t in (0, 1, 3, 4, 6)]
        pwr = [(7 * i) % 35 for i in range(len(fn))]
        steps.append((ta, trxhip.ms_tx_requests(fn, tn, pwr, some_bits(rng, len(fn)))))
    return clock, steps


def test_chunking_invariance(trx):
    """five members with the same 40 bursts over 8 frames, rendered whole and in chunks of 313, 625, 1250 and 4999 in the same
    calls: the five streams are identical, and are the single object's"""
    import torch
    total, chunks = 40000, (40000, 313, 625, 1250, 4999)
    n = len(chunks)
    clock, steps = traffic(np.random.default_rng(2024))
    group = trxhip.MsTxSchedulerGroup(trx, n_members=n, tx_full_scale=2047, rxtx_delay=-60, max_pending=64)
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=2047, rxtx_delay=-60, max_pending=64)
    first_ts = None
    for ta, reqs in steps:
        tx.set_ta(ta)
        want_plan = tx.submit(reqs, clock)
        for m in range(n):
            group.set_ta(m, ta)
        plan = group.submit(np.repeat(np.arange(n), len(reqs)), np.tile(reqs, n), [clock] * n)
        assert (plan["status"] == M.QUEUED).all() and plan.reshape(n, -1)[3].tobytes() == want_plan.tobytes()
        first_ts = first_ts if first_ts is not None else int(plan["radio_ts"].min()) - 300
    want, nd = single_render(tx, total, first_ts)
    assert nd == 40
    o = Out(n, total)
    acc = torch.zeros((n, total, 2), dtype=torch.int16, device="cuda:0")
    done, drawn = [0] * n, [0] * n
    while min(done) < total:
        sizes = [min(c, total - d) for c, d in zip(chunks, done)]
        o.flat.fill_(MARK)
        _, nd = group.render(sizes, [first_ts + d for d in done], out=o.out)
        for m, k in enumerate(sizes):
            acc[m, done[m]:done[m] + k] = o.out[m, :k]
            o.out[m, :k] = MARK
            done[m] += k
            drawn[m] += nd[m]
        assert o.untouched(), "wrote outside a window"
    got = acc.cpu().numpy()
    for m in range(n):
        assert np.array_equal(got[m], want), (m, np.flatnonzero((got[m] != want).any(axis=1))[:8])
        assert group.state(m).tobytes() == tx.state().tobytes()
    assert drawn == [40] * n


def test_members_are_independent(trx):
    """member 1's samples, plan and state do not depend on what the other members are asked and on their windows"""
    rng = np.random.default_rng(15)
    mine = dense(rng, 2, skip_tn=3)
    streams = []
    for variant in range(2):
        g = trxhip.MsTxSchedulerGroup(trx, n_members=3, tx_full_scale=9830, rxtx_delay=-67, max_pending=32)
        g.set_ta(1, 6)
        clocks = [(500, 1, 99), CLOCK, (77, 7, 1 << 36)] if variant else [CLOCK] * 3
        if variant:
            g.set_ta(0, 40)
            other = dense(rng, 3, fn0=503)
            members = [0, 0] + [1] * len(mine) + [0] * (len(other) - 2)
            plan = g.submit(members, np.concatenate([other[:2], mine, other[2:]]), clocks)
            plan = plan[2:2 + len(mine)]
        else:
            plan = g.submit(1, mine, clocks)
        at = int(plan["radio_ts"].min()) - 50
        o = Out(3, 6000)
        sizes, first = ([4000, 5999, 17], [99, at, 0]) if variant else ([0, 5999, 0], [0, at, 0])
        g.render(sizes, first, out=o.out)
        w = o.windows(sizes)[1]
        o = Out(3, 6000, shift=1)
        sizes, first = ([0, 4001, 6000], [0, at + 5999, 1 << 36]) if variant else ([1, 4001, 0], [5, at + 5999, 0])
        g.render(sizes, first, out=o.out)
        streams.append((np.concatenate([w, o.windows(sizes)[1]]), plan.tobytes(), g.state(1).tobytes()))
    assert streams[0][0].any() and np.array_equal(streams[0][0], streams[1][0]) and streams[0][1:] == streams[1][1:]


def test_group_of_one_and_ring_rows_reused(trx):
    """a group of one is the single object; and with max_pending 3 the ring rows of three members come round again and again under
    submits that mix the members: still the single objects' streams"""
    rng = np.random.default_rng(16)
    one = Pair(trx, 1)
    plan = one.submit(0, dense(rng, 2), [CLOCK])
    at = int(plan["radio_ts"].min()) - 9
    for k in (700, 4999, 5000):
        one.render([k], [at])
        at += k
    pair = Pair(trx, 3, fs=2047, delay=0, max_pending=3)
    for m in range(3):
        pair.set_ta(m, 3 * m)
    at, statuses = None, set()
    for r in range(10):
        clocks = [(1000 + r, 2, 123457 + 5000 * r)] * 3
        tns = ((0, 3, 5, 6), (1, 4), (2, 7, 0))                     # four requests against three rows: FULL among them
        members = [m for k in range(4) for m in range(3) if k < len(tns[m])]
        tn = [tns[m][k] for k in range(4) for m in range(3) if k < len(tns[m])]
        plan = pair.submit(members, trxhip.ms_tx_requests(1002 + r, tn, (r * 11) % 30, some_bits(rng, len(tn))), clocks)
        statuses |= set(int(s) for s in plan["status"])
        if at is None:
            at = [int(plan["radio_ts"].min()) - 20] * 3
        sizes = [5000, 4999 + (r & 1) * 2, 5000]
        got = pair.render(sizes, at, shift=r & 1)
        assert all(w.any() for w in got)
        at = [a + s for a, s in zip(at, sizes)]
    assert statuses >= {M.QUEUED, M.FULL}
    assert all(int(pair.group.state(m)["drawn"]) >= 15 for m in range(3))      # five times the ring and more


def test_refusals_move_nothing(trx):
    rng = np.random.default_rng(17)
    pair = Pair(trx, 3)
    reqs = dense(rng, 1)
    plan = pair.submit(np.arange(len(reqs)) % 3, reqs, [CLOCK] * 3)
    at = int(plan["radio_ts"].min()) - 10
    pair.render([1000, 0, 300], [at] * 3)
    before = [pair.group.state(m).tobytes() for m in range(3)]
    g, L = pair.group, pair.group.L
    more = trxhip.ms_tx_requests(1010, [0, 1, 2], 0, some_bits(rng, 3))
    bad_tn = more.copy()
    bad_tn["tn"][2] = 8
    for members, r, clocks, bad_at in (([0, 3, 1], more, [CLOCK] * 3, 1), ([0, 1, 2], bad_tn, [CLOCK] * 3, 2),
                                       ([0, 1, 2], more, [CLOCK, (M.HYPERFRAME, 0, 0), CLOCK], 1)):
        with pytest.raises(trxhip.TrxHipError):
            g.submit(members, r, clocks)
        assert g.bad == bad_at and [g.state(m).tobytes() for m in range(3)] == before
    o = Out(3, 2000)
    for sizes, first, bad_at in (([500, 500, 500], [at + 1000, at, at + 299], 2), ([500, 500, 500], [at + 999, at, at + 299], 0),
                                 ([500, 2001, 500], [at + 1000, at, at + 300], 1)):
        with pytest.raises(trxhip.TrxHipError):
            g.render(sizes, first, out=o.out)
        assert g.bad == bad_at and o.untouched() and [g.state(m).tobytes() for m in range(3)] == before
    ts = np.array([at + 1000, at, at + 300], dtype=np.int64)
    ns = np.array([500, 500, 500], dtype=np.uintp)
    vp = C.c_void_p
    for ptr in (o.out.data_ptr() + 2, None):                       # misaligned, NULL
        assert L.trxhip_ms_tx_group_render_s16(g.h, ptr, 2000, ts.ctypes.data_as(vp), ns.ctypes.data_as(vp), None, None, None) == -22
        assert o.untouched() and [g.state(m).tobytes() for m in range(3)] == before
    # what the refused calls left behind draws as the single objects do
    pair.render([500, 500, 500], [at + 1000, at, at + 300], stride=2000)


def test_pinned_to_the_row_modulator(trx):
    """16 bursts of one member among three against trxhip_modulate_batch(..., s16_scale=1) rows, as for the single object"""
    rng = np.random.default_rng(18)
    n = 16
    fn, tn = 1002 + np.arange(n), np.arange(n) % 8
    bits = some_bits(rng, n)
    g = trxhip.MsTxSchedulerGroup(trx, n_members=3, tx_full_scale=9830, rxtx_delay=-67, max_pending=n)
    g.set_ta(2, 17)
    plan = g.submit(2, trxhip.ms_tx_requests(fn, tn, (np.arange(n) * 5) % 40, bits), {2: CLOCK})
    assert (plan["status"] == M.QUEUED).all()
    assert plan["scale"].tobytes() == np.array([M.scale_of(9830, p) for p in (np.arange(n) * 5) % 40], dtype=np.float32).tobytes()
    rows = rows_of(trx, bits, tn, plan["scale"])
    first_ts = int(plan["radio_ts"].min()) - 5
    k = int(plan["radio_ts"].max()) + 630 - first_ts
    o = Out(3, k + 1, shift=1)
    _, nd = g.render([0, 0, k], [0, 0, first_ts], out=o.out)
    got = o.windows([0, 0, k])[2]
    assert nd == [0, 0, n]
    assert np.array_equal(got, expected_stream(k, first_ts, [(int(t), rows[i]) for i, t in enumerate(plan["radio_ts"])]))
