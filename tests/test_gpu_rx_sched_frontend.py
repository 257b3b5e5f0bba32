"""The uplink scheduler behind the receive front end on the GPU (pytest -m gpu): trxhip_rx_sched_pull_frontend() against the
two calls it is defined by, trxhip_rx_frontend_pull() into rows and trxhip_rx_sched_pull_cf32() over them, on a second pair of
fresh objects.  Every comparison is byte for byte -- datagrams, lengths, indication records, soft rows, clock, noise rings,
counters, carried count -- so the feature brings no tolerance of its own.  The wideband input is the project's own transmit
side: a TxScheduler with submitted datagrams through render_frontend to int16, plus a little noise, so that the slots hold normal
bursts, access bursts, dummy bursts and silence, and the receiving scheduler looks for TSC, RACH, IDLE and OFF on different
timeslots of different channels (v0 on one channel, v1 on the others)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rx_sched_model as M  # noqa: E402
import tx_sched_model as TM  # noqa: E402
from osmo_trx_amd import synth, trxhip  # noqa: E402
from test_rx_sched_frontend_cpu import MULTI_SEQ, SPS1_SEQ  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 32767.0
TSC = 5
HEAD = trxhip.RX_SCHED_WORK_HEAD
EINVAL = -22
N_SLOTS = 52 * 8                                         # 416 slots = 1000 blocks of 192 wideband time steps
WB = 192 * 4                                             # wideband samples per block
# the receiving scheduler's combinations per channel and TN: I (TSC), IV (RACH), FILL (IDLE), NONE (OFF)
RX_COMBS = ([1, 1, 1, M.COMB_FILL, 1, 4, 1, 1],
            [1, 1, M.COMB_FILL, 1, 4, 1, M.COMB_NONE, 1],
            [1, M.COMB_NONE, 1, 4, 1, M.COMB_FILL, 1, 1])
RACH_TN = (5, 4, 3)                                      # ... so channel c is sent access bursts on TN RACH_TN[c]
RX_VERSIONS = (1, 0, 1)


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = trxhip.TrxHip(0)
    yield t
    t.close()


def add_noise(wide, rng):
    import torch
    noise = torch.from_numpy(np.round(rng.standard_normal(tuple(wide.shape)) * 20.0).astype(np.int16)).to("cuda:0")
    return (wide.to(torch.int32) + noise).clamp(-32768, 32767).to(torch.int16).contiguous()


def access_bits(n, rng):
    """148-bit datagram payloads that hold an access burst (8 tail | 41 sync | 36 data | 3 tail) from bit 0, zeros behind"""
    import torch
    gen = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    out = np.zeros((n, 148), dtype=np.uint8)
    out[:, :88] = synth.access_burst_bits(n, torch.zeros(n), gen, "cpu").numpy()
    return out


class Air:
    """three channels, 416 slots from (FN 0, TN 0) through the MULTI transmit front end: normal bursts of TSC 5; access bursts
    on TN RACH_TN[c]; channel 0 sends nothing of its own in `idle` slots (the dummy filler goes out in the first 26 frames, the
    burst of 26 frames earlier after that); channel 1's TN 6 is NONE (silence)"""

    def __init__(self, trx):
        import torch
        from test_gpu_tx_frontend import _unambiguous_bursts
        rng = np.random.default_rng(41)
        slot = np.arange(N_SLOTS)
        self.bits = [_unambiguous_bursts(np.full(N_SLOTS, TSC), rng) for _ in range(3)]
        self.rach = [slot % 8 == RACH_TN[c] for c in range(3)]
        for c in range(3):
            self.bits[c][self.rach[c]] = access_bits(int(self.rach[c].sum()), rng)
        self.idle = (slot % 7 == 3) & (slot % 8 != 6) & ~self.rach[0]
        self.dummy = self.idle & (slot < 26 * 8)
        self.retx = self.idle & (slot >= 26 * 8)
        self.none = slot % 8 == 6
        tx = trxhip.TxScheduler(trx, chans=3, sps=4, filler=TM.FILLER_DUMMY, full_scale=6000.0, queue_cap=1024, max_slots=1024)
        tx.set_clock(0, 0)
        for c in range(3):
            for tn in range(8):
                tx.set_slot(c, tn, TM.COMB_NONE if (c == 1 and tn == 6) else 1)
            for i in range(N_SLOTS):
                if c == 0 and self.idle[i]:
                    continue
                assert tx.submit(c, TM.dgram(i // 8, i % 8, self.bits[c][i])) >= 0
        fe = trxhip.TxFrontEnd(trx, chans=3)
        nb, nc, _, wide = tx.render_frontend(N_SLOTS, fe, cf32=False, s16_scale=float(np.float32(1.0 / 3)))
        assert nb == 1000 and nc == 0
        torch.cuda.synchronize()
        self.wide = add_noise(wide, rng)
        assert self.wide.shape == (1000 * WB, 2)
        fe.close()
        tx.close()

    def blocks(self, a, b):
        return self.wide[a * WB:b * WB]


@pytest.fixture(scope="module")
def air(trx):
    return Air(trx)


def new_rx(trx, chans, sps=4, exact=False, max_slots=1024, muted=None, clock=(0, 0), combs=RX_COMBS):
    s = trxhip.RxScheduler(trx, chans=chans, sps=sps, tsc=TSC, exact=exact, full_scale=FULL, max_slots=max_slots)
    s.set_clock(*clock)
    s.set_max_toa(20, 63)
    for c in range(chans):
        for tn in range(8):
            s.set_slot(c, tn, combs[c][tn])
        s.set_trxd_version(c, RX_VERSIONS[c])
    if chans > 1:
        s.set_rssi_offset(1, 9.0)
    if muted is not None:
        s.set_muted(muted, True)
    return s


def new_pair(trx, chans, **kw):
    return trxhip.RxFrontEnd(trx, 192, 65, 48, chans=chans), new_rx(trx, chans, **kw)


def two_calls(fe, s, wide, n_blocks):
    """the form the join is defined by: the front end into rows of its own, then a complex64 pull over them"""
    return s.pull(fe.pull(wide, n_blocks), want_soft=True)


def host(out):
    """(pkt, pkt_len, ind, soft) device tensors -> their bytes on the host"""
    return tuple(t.cpu().numpy().reshape(t.shape[0], int(np.prod(t.shape[1:]))).view(np.uint8) for t in out)


def cat(parts):
    """per-pull host outputs [chans, n_i * bytes] -> the stream's, per channel"""
    return tuple(np.concatenate([p[k] for p in parts], 1) for k in range(4))


def same(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), ("pkt", "pkt_len", "ind", "soft")[k]


def state(s):
    """clock, carried count, and per channel the noise ring and the counters (waits for the pulls)"""
    out = [s.clock(), s.carried, s.slots(0), s.slots(1)]
    for c in range(s.chans):
        ring, itr, lev = s.noise_state(c)
        out += [ring.tobytes(), itr, np.float32(lev).tobytes(), tuple(sorted(s.counters(c).items()))]
    return out


@pytest.mark.parametrize("chans", [1, 2, 3])
def test_one_pull_equals_the_two_calls(trx, air, chans):
    """125 blocks = 32 500 samples per channel = exactly 52 slots: the strict `>` cuts 51 and carries 625.  The 25 blocks behind
    them then begin with a slot that lies in the remainder whole"""
    import torch
    fe, s = new_pair(trx, chans, exact=chans == 2)
    fe2, s2 = new_pair(trx, chans, exact=chans == 2)
    w = air.blocks(0, 125)
    assert s.slots_frontend(fe, 125) == 51 == s2.slots(32500)
    got = s.pull_frontend(fe, w, 125, want_soft=True)
    want = two_calls(fe2, s2, w, 125)
    torch.cuda.synchronize()
    assert got[0].shape == (chans, 51, 160) and got[3].shape == (chans, 51, 148)
    same(host(got), host(want))
    assert s.carried == 625 == s2.carried and s.clock() == (6, 3)
    assert state(s) == state(s2)
    ind = s.ind_to_numpy(got[2])
    if chans == 3:
        assert set(ind["type"].ravel()) == {M.TSC, M.RACH, M.IDLE, M.OFF}
        assert [int(ind[c]["type"][RACH_TN[c]]) for c in range(3)] == [M.RACH] * 3
        assert (ind["rc"] == M.RACH).sum() >= 15            # (one and two channels listen to other carriers' timeslots)
    assert (ind["rc"] == M.TSC).sum() > 15 * chans
    for c in range(chans):
        assert np.array_equal(s.plan(c), s2.plan(c))
    # both front ends carry the same histories, both schedulers the same 625 samples
    w = air.blocks(125, 150)
    got, want = s.pull_frontend(fe, w, 25, want_soft=True), two_calls(fe2, s2, w, 25)
    assert got[0].shape[1] == 11
    same(host(got), host(want))
    assert state(s) == state(s2)


_one_piece = {}


def one_piece(trx, air, muted):
    """the 125 blocks in one pull_frontend of three channels -> (host outputs, state); computed once per `muted`"""
    if muted not in _one_piece:
        fe, s = new_pair(trx, 3, muted=muted)
        out = host(s.pull_frontend(fe, air.blocks(0, 125), 125, want_soft=True))
        _one_piece[muted] = (out, state(s))
    return _one_piece[muted]


@pytest.mark.parametrize("muted", [None, 2])
def test_any_chunking(trx, air, muted):
    """block counts 1, 2, 3, 1, 5, 7, 2, 11, ...: pulls that only carry (260 samples; 310 carried + 260), pulls whose first slot
    begins in the remainder (780 samples behind 155 carried), and the outputs and the state of the one-piece pull"""
    fe, s = new_pair(trx, 3, muted=muted)
    parts, cuts, at, i = [], [], 0, 0
    while at < 125:
        nb = min(MULTI_SEQ[i % len(MULTI_SEQ)], 125 - at)
        carried = s.carried
        out = s.pull_frontend(fe, air.blocks(at, at + nb), nb, want_soft=True)
        cuts.append((carried, out[0].shape[1]))
        parts.append(host(out))
        at += nb
        i += 1
    assert cuts[:5] == [(0, 0), (260, 1), (155, 1), (310, 0), (570, 2)]      # (carried in front of the pull, slots it cut)
    want, want_state = one_piece(trx, air, muted)
    same(cat(parts), want)
    assert state(s) == want_state
    if muted is not None:
        ind = np.ascontiguousarray(want[2][muted]).view(trxhip.UL_IND_DTYPE)
        assert ((ind["flags"] & trxhip.ULIND_MUTED) != 0)[ind["type"] != M.OFF].all()


def test_alternating_with_pull_cf32(trx, air):
    """pull_frontend, pull_cf32 over rows of a second front end, pull_frontend: one object, one carried remainder"""
    fe, s = new_pair(trx, 3)
    parts = [host(s.pull_frontend(fe, air.blocks(0, 40), 40, want_soft=True))]
    assert s.carried == 40 * 260 - 16 * 625
    fe2 = trxhip.RxFrontEnd(trx, 192, 65, 48, chans=3)
    fe2.seed(air.blocks(0, 40), 40)
    parts.append(host(s.pull(fe2.pull(air.blocks(40, 77), 37), want_soft=True)))
    assert s.carried == 77 * 260 - 32 * 625
    fe.seed(air.blocks(40, 77), 37)                        # the first object has not seen these blocks
    parts.append(host(s.pull_frontend(fe, air.blocks(77, 125), 48, want_soft=True)))
    want, want_state = one_piece(trx, air, None)
    same(cat(parts), want)
    assert state(s) == want_state


def resamp_stream(trx, sps, n_slots, p, q, block_len, clock, seed):
    """one channel of normal bursts from `clock` through the RESAMP transmit front end (p, q) -> int16[n, 2] with noise"""
    import torch
    from test_gpu_tx_frontend import _unambiguous_bursts
    rng = np.random.default_rng(seed)
    bits = _unambiguous_bursts(np.full(n_slots, TSC), rng)
    tx = trxhip.TxScheduler(trx, chans=1, sps=sps, filler=TM.FILLER_DUMMY, full_scale=6000.0, queue_cap=256, max_slots=256)
    tx.set_clock(*clock)
    for tn in range(8):
        tx.set_slot(0, tn, 1)
    for i in range(n_slots):
        t = clock[1] + i
        assert tx.submit(0, TM.dgram(clock[0] + t // 8, t % 8, bits[i])) >= 0
    fe = trxhip.TxFrontEnd(trx, chans=1, block_len=block_len, p=p, q=q, mode="resamp")
    nb, _, _, wide = tx.render_frontend(n_slots, fe, cf32=False, s16_scale=1.0)
    torch.cuda.synchronize()
    wide = add_noise(wide, rng)
    fe.close()
    tx.close()
    return wide


ALL_TSC = ([1] * 8,)


@pytest.mark.parametrize("p,q,block_len,tx_block,n_slots", [(65, 96, 1536, 260, 42), (52, 75, 1200, 208, 34)])
def test_resamp_4sps(trx, p, q, block_len, tx_block, n_slots):
    """RadioInterfaceResamp's chunks, 25 of them in pulls of 3, 1, 7, 2 and 12, against the two calls"""
    wide = resamp_stream(trx, 4, n_slots, q, p, tx_block, (0, 0), 7)
    assert wide.shape[0] >= 25 * block_len
    pairs = [(trxhip.RxFrontEnd(trx, block_len, p, q, chans=1, mode="resamp"), new_rx(trx, 1, combs=ALL_TSC)) for _ in range(2)]
    at, found = 0, 0
    for nb in (3, 1, 7, 2, 12):
        w = wide[at * block_len:(at + nb) * block_len]
        got = pairs[0][1].pull_frontend(pairs[0][0], w, nb, want_soft=True)
        want = two_calls(pairs[1][0], pairs[1][1], w, nb)
        same(host(got), host(want))
        assert state(pairs[0][1]) == state(pairs[1][1])
        found += int((pairs[0][1].ind_to_numpy(got[2])["rc"] == M.TSC).sum())
        at += nb
    total = 25 * block_len // q * p
    assert pairs[0][1].carried == total - (total - 1) // 625 * 625
    assert found >= (total - 1) // 625 - 2                 # the bursts are found (all but the stream's first and last slot)


@pytest.mark.parametrize("tn0", [0, 1, 2, 3])
def test_resamp_1sps(trx, tn0):
    """block_len 384 at (65, 96) into a 1-SPS scheduler, from each TN phase, in uneven block counts: slot 0 of a pull begins in
    the remainder both as a slot of 157 and as one of 156 samples"""
    wide = resamp_stream(trx, 1, 72, 96, 65, 260, (7, tn0), 11 + tn0)
    assert wide.shape[0] >= 40 * 384
    pairs = [(trxhip.RxFrontEnd(trx, 384, 65, 96, chans=1, mode="resamp"), new_rx(trx, 1, sps=1, clock=(7, tn0), combs=ALL_TSC))
             for _ in range(2)]
    at, i, found, slots, straddle = 0, 0, 0, 0, set()
    while at < 40:
        nb = min(SPS1_SEQ[i % len(SPS1_SEQ)], 40 - at)
        s = pairs[0][1]
        tn, carried = s.clock()[1], s.carried
        w = wide[at * 384:(at + nb) * 384]
        got = s.pull_frontend(pairs[0][0], w, nb, want_soft=True)
        want = two_calls(pairs[1][0], pairs[1][1], w, nb)
        same(host(got), host(want))
        assert state(s) == state(pairs[1][1])
        if got[0].shape[1] and carried:
            straddle.add(tn % 4 == 0)
        found += int((s.ind_to_numpy(got[2])["rc"] == M.TSC).sum())
        slots += got[0].shape[1]
        at += nb
        i += 1
    assert straddle == {True, False}
    assert slots in (66, 67) and found >= slots - 2


def test_loopback(trx, air):
    """TxScheduler.render_frontend (3 channels) -> wideband int16 -> RxScheduler.pull_frontend: every submitted normal burst
    that the receiver looks for as a normal burst comes back at its FN / TN, with its TSC and 148 soft bytes whose hard
    decisions are its bits; the access bursts come back as RACH.  The front ends' delay is handled as in the loopbacks of
    test_gpu_tx_sched.py and test_gpu_rx_sched.py: it is left to the detector's search window (max_toa 20), the stream's first
    slot, which begins in the front ends' transient, is not judged, and the bits judged are 3 .. 144 with those tests' bar
    (wrong in fewer than 1e-3 of positions) -- the delay pushes the burst's last symbols past the end of its 625-sample slot,
    so the trailing tail bits, which carry no information, are decided from samples the slot does not hold (measured on
    channel 0: 291 bursts, no wrong bit in 3 .. 144, 746 wrong among bits 145 .. 147; an isolated burst gives all 148,
    test_gpu_tx.py).  1000 blocks are 416 slots' worth: 415 are cut, 625 samples wait for one more"""
    import torch
    fe, s = new_pair(trx, 3, exact=True)
    pkt, plen, ind, _ = s.pull_frontend(fe, air.wide, 1000)
    torch.cuda.synchronize()
    n = N_SLOTS - 1
    assert pkt.shape[1] == n and s.carried == 625
    pkt, plen, ind = pkt.cpu().numpy(), plen.cpu().numpy(), s.ind_to_numpy(ind)
    k = np.arange(n)
    body = k > 0
    for c in range(3):
        comb = np.array(RX_COMBS[c])[k % 8]
        assert np.array_equal(ind[c]["fn"], k // 8) and np.array_equal(ind[c]["tn"], k % 8)
        sent = body & (comb == 1)
        if c == 0:
            sent &= ~air.dummy[:n]
        if c == 1:
            sent &= ~air.none[:n]
        want = air.bits[c][:n].copy()
        if c == 0:
            want[air.retx[:n]] = air.bits[0][np.flatnonzero(air.retx[:n]) - 26 * 8]
        assert (ind[c]["rc"][sent] == M.TSC).all(), (c, np.flatnonzero(sent & (ind[c]["rc"] != M.TSC))[:10])
        assert (ind[c]["tsc"][sent] == TSC).all() and (ind[c]["nbits"][sent] == 148).all()
        hdr = 8 if RX_VERSIONS[c] == 0 else 11                # v0 ends with two bytes of padding
        assert (plen[c][sent] == (158 if RX_VERSIONS[c] == 0 else 159)).all()
        d = pkt[c][sent]
        i = np.flatnonzero(sent)
        assert np.array_equal(d[:, 0] & 7, i % 8) and np.array_equal(d[:, 4] | (d[:, 3].astype(np.int64) << 8), i // 8)
        hard = (d[:, hdr:hdr + 148] > 127).astype(np.uint8)
        wrong = hard != want[sent]
        print("channel", c, "bursts", int(sent.sum()), "wrong bits", int(wrong.sum()), "of them in 3..144", int(wrong[:, 3:145].sum()))
        assert wrong[:, 3:145].mean() < 1e-3, (c, np.argwhere(wrong[:, 3:145])[:10])
        rach = body & (comb == 4)
        assert rach.sum() >= 50 and (ind[c]["rc"][rach] == M.RACH).all(), (c, np.flatnonzero(rach & (ind[c]["rc"] != M.RACH))[:10])
        assert ((ind[c]["flags"] & trxhip.ULIND_OFF) != 0)[comb == M.COMB_NONE].all()


def test_larger_pull(trx, air):
    """4096 blocks x 3 channels, 1703 slots per channel: the front end walks several tiles per workgroup and the detector's grid
    is more than one wave of workgroups"""
    import torch
    wide = air.wide.repeat(5, 1)[:4096 * WB].contiguous()
    fe, s = new_pair(trx, 3, max_slots=2048)
    fe2, s2 = new_pair(trx, 3, max_slots=2048)
    assert s.slots_frontend(fe, 4096) == 1703
    got = s.pull_frontend(fe, wide, 4096, want_soft=True)
    want = two_calls(fe2, s2, wide, 4096)
    torch.cuda.synchronize()
    assert got[0].shape[1] == 1703 and s.carried == 4096 * 260 - 1703 * 625
    same(host(got), host(want))
    assert state(s) == state(s2)
    assert (s.ind_to_numpy(got[2])["rc"] == M.TSC).sum() > 2000


def test_refusals(trx, air):
    """every refusal is TRXHIP_EINVAL, launches nothing and leaves the scheduler and the front end -- its history half too --
    where objects that never saw the call are; n_blocks == 0 is OK and changes nothing"""
    import torch
    L = trx.L
    nb = 30
    n_out = nb * 260
    fe, s = new_pair(trx, 3, max_slots=64)
    fe_c, s_c = new_pair(trx, 3, max_slots=64)                               # the clean pair
    first = [o.pull_frontend(f, air.blocks(0, 20), 20, want_soft=True) for f, o in ((fe, s), (fe_c, s_c))]
    k = s.slots_frontend(fe, nb)
    assert k == 12 and s.carried == 200
    w = air.blocks(20, 20 + nb + 1)
    stride = HEAD + n_out
    work = torch.full((3, stride + 8), 7.0, dtype=torch.complex64, device="cuda:0")
    pkt = torch.full((3, k, 160), 0xAB, dtype=torch.uint8, device="cuda:0")
    plen = torch.full((3, k), -1, dtype=torch.int16, device="cuda:0")
    ind = torch.full((3, k, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    soft = torch.full((3, k, 148), -7.0, dtype=torch.float32, device="cuda:0")
    ns, nc = C.c_size_t(99), C.c_size_t(99)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)    # noqa: E731
    st = trx._stream()

    def call(sh=None, feh=None, d_wide=None, n_blocks=nb, d_work=None, work_stride=stride, out_slots=k):
        return L.trxhip_rx_sched_pull_frontend(s.h if sh is None else sh, fe.h if feh is None else feh,
                                               p(w) if d_wide is None else d_wide, n_blocks, p(work) if d_work is None else d_work,
                                               work_stride, p(pkt), 160, p(plen), p(ind), p(soft), out_slots, C.byref(ns),
                                               C.byref(nc), st)

    null = C.c_void_p(None)
    plan_only = trxhip.RxScheduler(None, chans=3)
    plan_only.set_clock(0, 0)
    other = trxhip.TrxHip(0)                                                  # a second context on the same device
    fe_other = trxhip.RxFrontEnd(other, 192, 65, 48, chans=3)
    fe_two = trxhip.RxFrontEnd(trx, 192, 65, 48, chans=2)
    fe_four = trxhip.RxFrontEnd(trx, 192, 65, 48)
    assert fe_four.rows == 4
    no_clock = trxhip.RxScheduler(trx, chans=3, full_scale=FULL, max_slots=64)
    s16_rem = new_rx(trx, 3, max_slots=64)
    s16_rem.pull(torch.zeros((3, 100, 2), dtype=torch.int16, device="cuda:0"))
    assert s16_rem.carried == 100
    refused = {
        "no scheduler": call(sh=null),
        "no front end": call(feh=null),
        "plan-only scheduler": call(sh=plan_only.h),
        "front end of another context": call(feh=fe_other.h),
        "rows != chans": call(feh=fe_two.h),
        "four-row front end": call(feh=fe_four.h),
        "no d_wide": call(d_wide=null),
        "d_wide misaligned": call(d_wide=p(w, 4)),
        "no d_work": call(d_work=null),
        "d_work misaligned": call(d_work=p(work, 8)),
        "work_stride too small": call(work_stride=stride - 2),
        "work_stride odd": call(work_stride=stride + 1),
        "pull before set_clock": call(sh=no_clock.h),
        "more than max_slots": call(n_blocks=200, work_stride=HEAD + 200 * 260),
        "more than out_slots": call(out_slots=k - 1),
        "int16 remainder": call(sh=s16_rem.h),
    }
    for sh, feh in ((plan_only.h, fe.h), (s.h, fe_other.h), (s.h, fe_two.h), (s.h, fe_four.h), (s.h, null), (null, fe.h)):
        assert L.trxhip_rx_sched_slots_frontend(sh, feh, nb) == EINVAL
    assert L.trxhip_rx_sched_slots_frontend(s.h, fe.h, nb) == k
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in refused.values()), {x: rc for x, rc in refused.items() if rc != EINVAL}
    assert (ns.value, nc.value) == (99, 99)
    assert (pkt == 0xAB).all() and (plen == -1).all() and (ind == 0xAB).all() and (soft == -7.0).all()      # nothing was launched
    assert (work == 7.0).all()
    assert state(s) == state(s_c) and s16_rem.slots(0) == 0 and s16_rem.slots(526) == 1
    # n_blocks == 0: OK, nothing cut, nothing changed
    assert call(n_blocks=0) == 0 and (ns.value, nc.value) == (0, 200)
    torch.cuda.synchronize()
    assert (pkt == 0xAB).all() and (work == 7.0).all() and state(s) == state(s_c)
    got = [o.pull_frontend(f, air.blocks(20, 20 + nb), nb, want_soft=True) for f, o in ((fe, s), (fe_c, s_c))]
    torch.cuda.synchronize()
    same(host(first[0]), host(first[1]))
    same(host(got[0]), host(got[1]))
    assert got[0][0].shape[1] == k and state(s) == state(s_c)
    assert (s.ind_to_numpy(got[0][2])["rc"] == M.TSC).sum() > 20
    # a work area of the caller's: rows longer than needed, reused by the next pull
    big = torch.empty((3, HEAD + 40 * 260), dtype=torch.complex64, device="cuda:0")
    for n_b, at in ((7, 50), (40, 57)):
        a = s.pull_frontend(fe, air.blocks(at, at + n_b), n_b, want_soft=True, work=big)
        b = two_calls(fe_c, s_c, air.blocks(at, at + n_b), n_b)
        same(host(a), host(b))
    with pytest.raises(ValueError):
        s.pull_frontend(fe, air.blocks(97, 98), 1, work=big[:2])
    with pytest.raises(ValueError):
        s.pull_frontend(fe, air.blocks(97, 98), 1, work=torch.empty((3, HEAD + 259), dtype=torch.complex64, device="cuda:0"))
    for o in (fe_other, fe_two, fe_four, no_clock, s16_rem, plan_only):
        o.close()
    other.close()


def test_host_classes_forward_to_the_join(trx, air, tmp_path):
    """sigproc_selftest rx_join: MultiArfcnRx::pullScheduled in runs of 1, 2, 3, ... blocks against the two calls, from C++"""
    exe = os.path.join(ROOT, "osmo_trx_amd", "lib", "sigproc_selftest")
    (tmp_path / "wide.s16").write_bytes(air.blocks(0, 45).cpu().numpy().tobytes())
    r = subprocess.run([exe, "rx_join", str(tmp_path / "wide.s16"), "45", "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert r.returncode == 0 and "rx_join identical 18" in r.stdout, r.stdout
