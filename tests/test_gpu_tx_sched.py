"""The downlink burst scheduler on the GPU (pytest -m gpu): trxhip_tx_sched_render / _render_frontend against the model of
tests/tx_sched_model.py, each modelled source turned into samples by the already-pinned modulators (trxhip_modulate_trxd_batch,
the oracle's modulateBurst for the dummy filler)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O  # noqa: E402
import tx_sched_model as M  # noqa: E402
from osmo_trx_amd import trxhip  # noqa: E402

pytestmark = pytest.mark.gpu
FULL = 3000.0


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


def slot_len(tn, sps):
    return 625 if sps == 4 else 156 + (tn % 4 == 0)


class Expect:
    """samples of the modelled sources: bursts through modulate_trxd (pinned to the oracle by test_gpu_tx.py), the initial
    dummy filler from the oracle's modulateBurst scaled by (full_scale, 0) with Complex<float>'s multiply"""

    def __init__(self, trx, sps):
        self.trx, self.sps = trx, sps
        self.dg = {}
        self.rows = {}
        t = np.frombuffer(trxhip.generate_tx_tables_host(), dtype=np.uint8)
        from test_tx_cpu import TX_TABLES                                          # noqa: F401 (layout of the tables)
        self.dummy = np.frombuffer(t.tobytes(), dtype=TX_TABLES)[0]["dummy_burst"]
        self.fill0 = {}

    def add(self, i, d):
        if i >= 0:
            self.dg[i] = d

    def modulate_all(self):
        ids = [i for i in self.dg if i not in self.rows]
        if not ids:
            return
        D = np.zeros((len(ids), 450), dtype=np.uint8)
        L = np.zeros(len(ids), dtype=np.int32)
        for k, i in enumerate(ids):
            D[k, :len(self.dg[i])] = np.frombuffer(self.dg[i], np.uint8)
            L[k] = len(self.dg[i])
        out, _, info = self.trx.modulate_trxd(dev(D), dev(L), FULL, sps=self.sps, out_stride=625)
        assert (self.trx.tx_info_to_numpy(info)["status"] == 0).all()
        out = out.cpu().numpy()
        for k, i in enumerate(ids):
            self.rows[i] = out[k]

    def dummy_fill(self, tn):
        if tn not in self.fill0:
            x = O.modulate_burst(self.dummy, 8 + (tn % 4 == 0), self.sps)
            s = np.float32(FULL)
            re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
            self.fill0[tn] = (re * s - im * np.float32(0.0)) + 1j * (re * np.float32(0.0) + im * s)
        return self.fill0[tn].astype(np.complex64)

    def stream(self, srcs, tn0, chan, filler):
        self.modulate_all()
        parts = []
        for k, (kind, i) in enumerate(srcs):
            tn = (tn0 + k) % 8
            n = slot_len(tn, self.sps)
            if kind == "burst" or (kind == "filler" and i >= 0):
                parts.append(self.rows[i][:n])
            elif kind == "filler" and chan == 0 and filler == M.FILLER_DUMMY:
                parts.append(self.dummy_fill(tn)[:n])
            else:
                parts.append(np.zeros(n, np.complex64))
        return np.concatenate(parts)


def drive(trx, sps, filler, chans, frames, rng, fn0=77, tn0=3, renders=(1, 7, 300, 13), s16=None, queued=False, mute_at=None):
    """random traffic, then renders of the given sizes; returns (per-render outputs, per-render model sources, expect)"""
    s = trxhip.TxScheduler(trx, chans=chans, sps=sps, filler=filler, full_scale=FULL, queue_cap=4096, max_slots=4096)
    m = M.Model(chans, sps, filler)
    ex = Expect(trx, sps)
    for o in (s, m):
        o.set_clock(fn0, tn0)
        for c in range(chans):
            for tn, comb in enumerate([5, 1, 7, 13, 1, M.COMB_NONE, 4, 1]):
                o.set_slot(c, tn, comb)
    for fn in range(fn0, fn0 + frames + 2):
        for c in range(chans):
            for tn in range(8):
                r = rng.random()
                if r < 0.2:
                    continue
                n = 444 if r > 0.9 else 148
                d = M.dgram(fn if r > 0.25 else fn - 4, tn, rng.integers(0, 2, n), att=int(rng.integers(0, 12)))
                i = s.submit(c, d)
                assert i == m.submit(c, d)
                ex.add(i, d)
                if r < 0.22:
                    d2 = M.dgram(fn, tn, rng.integers(0, 2, 148), att=1)              # duplicate time / repeated FN
                    i = s.submit(c, d2)
                    assert i == m.submit(c, d2)
                    ex.add(i, d2)
    outs, srcs = [], []
    total, k, done = frames * 8, 0, 0
    while done < total:
        n = min(renders[k % len(renders)], total - done)
        if mute_at is not None and k == mute_at:
            s.set_muted(0, True)
            m.set_muted(0, True)
        if mute_at is not None and k == mute_at + 1:
            s.set_muted(0, False)
            m.set_muted(0, False)
        _, tn_now = s.clock()
        cf, i16 = s.render(n, s16_scales=s16)
        outs.append((cf.clone() if cf is not None else None, i16.clone() if i16 is not None else None, tn_now))
        srcs.append(m.render(n))
        if not queued:
            import torch
            torch.cuda.synchronize()
        k += 1
        done += n
    for c in range(chans):
        assert s.counters(c) == m.ch[c].ctr
    return s, outs, srcs, ex


@pytest.mark.parametrize("sps,filler", [(4, M.FILLER_DUMMY), (1, M.FILLER_DUMMY), (4, M.FILLER_ZERO)])
@pytest.mark.parametrize("queued", [False, True])
def test_render_matches_model(trx, sps, filler, queued):
    import torch
    rng = np.random.default_rng(5 + sps + 10 * filler)
    s, outs, srcs, ex = drive(trx, sps, filler, 3, 120, rng, queued=queued, mute_at=5)
    torch.cuda.synchronize()
    if sps == 1:
        assert s.counters(1)["refused"] > 0                                          # 8-PSK refused and counted at 1 SPS
    for (cf, _, tn0), src in zip(outs, srcs):
        got = cf.cpu().numpy()
        for c in range(3):
            want = ex.stream(src[c], tn0, c, filler)
            assert got[c].shape == want.shape
            assert np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), c          # bit for bit, sign of zero included
    if sps == 4 and filler == M.FILLER_DUMMY:
        # an 8-PSK burst written into channel 0's filler table comes back in a later render as a device filler descriptor
        sent = {}
        found = False
        for k, src in enumerate(srcs):
            for kind, i in src[0]:
                if kind == "burst":
                    sent.setdefault(i, k)
                elif kind == "filler" and i in sent and sent[i] < k and len(ex.dg[i]) == 6 + 444:
                    found = True
        assert found


def test_staging_rows_recycled_while_renders_are_in_flight(trx):
    """A small ring: queue_cap 6 on 3 channels is 36 staging rows, and each render of 4 slots consumes up to 15.  The device is
    held back by a sleep, so no render completes while the host submits: by the third render every row is taken and submit
    must wait for the first render's event before it rewrites a row (and the fifth render for the first's slot buffer).  A
    row reused before its upload ran would change the samples; every render is compared with the model bit for bit."""
    import torch
    chans, cap, fn0 = 3, 6, 200
    s = trxhip.TxScheduler(trx, chans=chans, sps=4, filler=M.FILLER_DUMMY, full_scale=FULL, queue_cap=cap, max_slots=4)
    m = M.Model(chans, 4, M.FILLER_DUMMY)
    ex = Expect(trx, 4)
    for o in (s, m):
        o.set_clock(fn0, 0)
        for c in range(chans):
            for tn, comb in enumerate([5, 1, 7, 13, 1, M.COMB_NONE, 4, 1]):
                o.set_slot(c, tn, comb)
    rng = np.random.default_rng(17)
    bufs = torch.empty((60, chans, 4 * 625), dtype=torch.complex64, device="cuda:0")    # no allocation while the device sleeps
    torch.cuda.synchronize()
    torch.cuda._sleep(int(5e8))                          # the renders below queue up behind this
    outs, srcs = [], []
    for step in range(60):
        t = 4 * step
        for c in range(chans):
            for k in range(4):
                u = t + k
                r = rng.random()
                if k == 0 and r < 0.1:                   # a late burst: out of order or repeated, stale if queued
                    d = M.dgram(fn0 + (u - 8) // 8, u % 8, rng.integers(0, 2, 148), att=2)
                    i = s.submit(c, d)
                    assert i == m.submit(c, d)
                    ex.add(i, d)
                if r < 0.15:
                    continue
                d = M.dgram(fn0 + u // 8, u % 8, rng.integers(0, 2, 444 if r > 0.9 else 148), att=int(rng.integers(0, 12)))
                i = s.submit(c, d)
                assert i == m.submit(c, d)
                ex.add(i, d)
        _, tn_now = s.clock()
        cf, _ = s.render(4, out=bufs[step])
        outs.append((cf, tn_now))
        srcs.append(m.render(4))
    torch.cuda.synchronize()
    for c in range(chans):
        assert s.counters(c) == m.ch[c].ctr
    for (cf, tn0), src in zip(outs, srcs):
        got = cf.cpu().numpy()
        for c in range(chans):
            assert np.array_equal(got[c].view(np.uint32), ex.stream(src[c], tn0, c, M.FILLER_DUMMY).view(np.uint32)), c


def test_int16_three_scales(trx):
    import torch
    rng = np.random.default_rng(3)
    scales = [0.5, 1.0, 1.7]
    s, outs, srcs, ex = drive(trx, 4, M.FILLER_DUMMY, 3, 40, rng, s16=scales, renders=(37, 100))
    torch.cuda.synchronize()
    for (cf, i16, tn0), src in zip(outs, srcs):
        for c in range(3):
            want = ex.stream(src[c], tn0, c, M.FILLER_DUMMY).view(np.float32)
            q = (want * np.float32(scales[c])).astype(np.int32).astype(np.int16)
            assert np.array_equal(i16[c].cpu().numpy().reshape(-1), q), c
            assert np.array_equal(cf[c].cpu().numpy(), want.view(np.complex64))


@pytest.mark.parametrize("mode,chans,p,q", [("multi", 3, 48, 65), ("resamp", 1, 96, 65)])
def test_render_frontend_equals_push_of_model_stream(trx, mode, chans, p, q):
    import torch
    rng = np.random.default_rng(9)
    frames = 30
    s, outs, srcs, ex = drive(trx, 4, M.FILLER_DUMMY, chans, frames, rng, renders=(frames * 8,))
    torch.cuda.synchronize()
    x = torch.from_numpy(np.stack([ex.stream(srcs[0][c], 3, c, M.FILLER_DUMMY) for c in range(chans)])).to("cuda:0")
    bl = 260
    n_blocks = x.shape[1] // bl
    ref_fe = trxhip.TxFrontEnd(trx, chans=chans, block_len=bl, p=p, q=q, mode=mode)
    want, _ = ref_fe.push(x if chans > 1 else x[0], n_blocks)
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    # the same traffic again, rendered through a front end in random chunks
    rng = np.random.default_rng(9)
    sched = trxhip.TxScheduler(trx, chans=chans, sps=4, filler=M.FILLER_DUMMY, full_scale=FULL, queue_cap=4096, max_slots=4096)
    replay(sched, rng, chans, frames)
    fe = trxhip.TxFrontEnd(trx, chans=chans, block_len=bl, p=p, q=q, mode=mode)
    got, done, carried, blocks = [], 0, 0, 0
    crng = np.random.default_rng(1)
    while done < frames * 8:
        n = int(min(crng.integers(1, 40), frames * 8 - done))
        nb, nc, out, _ = sched.render_frontend(n, fe)
        done += n
        blocks += nb
        assert nb == (carried + 625 * n) // bl and nc == (carried + 625 * n) % bl
        carried = nc
        got.append(out.cpu().numpy())
    got = np.concatenate(got)
    assert blocks == n_blocks
    assert np.array_equal(got.view(np.float32), want.view(np.float32))


def replay(s, rng, chans, frames, fn0=77, tn0=3):
    """the submissions of drive() (same rng draws), on s only"""
    s.set_clock(fn0, tn0)
    for c in range(chans):
        for tn, comb in enumerate([5, 1, 7, 13, 1, M.COMB_NONE, 4, 1]):
            s.set_slot(c, tn, comb)
    for fn in range(fn0, fn0 + frames + 2):
        for c in range(chans):
            for tn in range(8):
                r = rng.random()
                if r < 0.2:
                    continue
                n = 444 if r > 0.9 else 148
                s.submit(c, M.dgram(fn if r > 0.25 else fn - 4, tn, rng.integers(0, 2, n), att=int(rng.integers(0, 12))))
                if r < 0.22:
                    s.submit(c, M.dgram(fn, tn, rng.integers(0, 2, 148), att=1))


def test_loopback_through_multi_front_end_and_receiver(trx):
    """scheduler -> MULTI front end -> RxFrontEnd -> detect_demod: every burst on its own logical channel and TN, with its TSC;
    channel 0's slots without a burst carry the dummy burst (rc IDLE with TRXHIP_FLAG_IDLE_DUMMY) in the first 26 frames and
    the burst sent 26 frames earlier after that (retransmission through the filler table); channel 1's NONE slots and the muted channel 2
    send zeros, which the receiver's noise turns into no more than its false alarms (the samples themselves are zeros bit for
    bit in test_render_matches_model)"""
    import torch
    from test_gpu_tx_frontend import _unambiguous_bursts
    chans, n_slots = 3, 52 * 8
    rng = np.random.default_rng(41)
    slot = np.arange(n_slots)
    tsc = [(slot + 3 * l) % 8 for l in range(chans)]
    bits = [_unambiguous_bursts(tsc[l], rng) for l in range(chans)]
    s = trxhip.TxScheduler(trx, chans=chans, sps=4, filler=M.FILLER_DUMMY, full_scale=6000.0, queue_cap=1024, max_slots=1024)
    idle = (slot % 7 == 3) & (slot % 8 != 6)            # channel 0: no burst submitted
    dummy = idle & (slot < 26 * 8)                         # ... the initial dummy filler goes out
    retx = idle & (slot >= 26 * 8)                         # ... the burst of FN - 26 goes out again (retransmission, modulus 26)
    none = slot % 8 == 6                                   # channel 1: TN 6 is NONE (its bursts are consumed, zeros go out)
    s.set_clock(0, 0)
    for c in range(chans):
        for tn in range(8):
            s.set_slot(c, tn, M.COMB_NONE if (c == 1 and tn == 6) else 1)
        for i in range(n_slots):
            if c == 0 and idle[i]:
                continue
            assert s.submit(c, M.dgram(i // 8, i % 8, bits[c][i])) >= 0
    s.set_muted(2, True)
    fe = trxhip.TxFrontEnd(trx, chans=chans)
    nb, nc, _, wide = s.render_frontend(n_slots, fe, cf32=False, s16_scale=float(np.float32(1.0 / chans)))
    assert nb == 1000 and nc == 0
    torch.cuda.synchronize()
    noise = torch.from_numpy(np.round(rng.standard_normal(tuple(wide.shape)) * 20.0).astype(np.int16)).to("cuda:0")
    wide = (wide.to(torch.int32) + noise).clamp(-32768, 32767).to(torch.int16)   # a receiver's noise floor
    rx = trxhip.RxFrontEnd(trx, 192, 65, 48)
    rs = rx.pull(wide, nb)
    body = np.zeros(n_slots, bool)
    body[1:-1] = True
    for pchan, lchan in ((0, 1), (1, 0), (3, 2)):
        params = np.zeros(n_slots, dtype=O.PARAMS_DTYPE)
        params["type"], params["max_toa"], params["tsc"] = O.TSC, 20, tsc[lchan]
        res, soft = trx.detect_demod(rs[pchan].view(n_slots, 625), trx.params_tensor(params), sps=4, full_scale=32767.0, exact=True)
        r = trx.results_to_numpy(res)
        if lchan == 0:
            # detectAnyBurst(IDLE) at the threshold of test_gpu_parity's dummy-burst test (the dummy midamble repeats every 8
            # bits: its peak-to-neighbourhood ratio stays under BURST_THRESH = 4 even on clean bursts).  Idle slots of the first
            # 26 frames send the initial dummy filler: found as the dummy burst, not as a normal burst
            pi = params.copy()
            pi["type"] = O.IDLE
            ri, _ = trx.detect_demod(rs[pchan].view(n_slots, 625), trx.params_tensor(pi), sps=4, threshold=1.5, full_scale=32767.0,
                                     exact=True, idle_dummy=True)
            ri = trx.results_to_numpy(ri)
            assert (ri["rc"][body & dummy] == O.IDLE).all(), np.flatnonzero(body & dummy & (ri["rc"] != O.IDLE))
            assert (r["rc"][body & dummy] > 0).mean() < 0.03
        # zeros (muted, NONE) carry only the receiver's noise: the noise-only false-alarm bar of test_gpu_tx_frontend's loopback
        if lchan == 2:
            assert (r["rc"] > 0).mean() < 0.03
            continue
        sent = body & ~(dummy if lchan == 0 else none)
        want = bits[lchan].copy()
        if lchan == 0:
            want[retx] = bits[0][np.flatnonzero(retx) - 26 * 8]       # the filler entry of FN - 26: the burst sent then
        else:
            assert (r["rc"][body & none] > 0).mean() < 0.03
        assert (r["rc"][sent] == O.TSC).all(), (pchan, np.flatnonzero(sent & (r["rc"] != O.TSC))[:10])
        hard = (soft.cpu().numpy()[sent] > 0.5).astype(np.uint8)
        assert (hard[:, 3:145] != want[sent][:, 3:145]).mean() < 1e-3


def test_full_size_render(trx):
    """one channel, 2^20 slots in one render (5.2 GB of cf32: offsets past 2^31 bytes), spot-checked against the model"""
    import torch
    n = 1 << 20
    s = trxhip.TxScheduler(trx, chans=1, sps=4, filler=M.FILLER_DUMMY, full_scale=FULL, queue_cap=64, max_slots=n)
    m = M.Model(1, 4, M.FILLER_DUMMY)
    ex = Expect(trx, 4)
    rng = np.random.default_rng(2)
    for o in (s, m):
        o.set_clock(10, 0)
        for tn in range(8):
            o.set_slot(0, tn, [4, 1][tn % 2])
    for k in range(40):                                   # bursts early and late in the render
        fn = 10 + (k if k < 20 else n // 8 - 40 + k)
        d = M.dgram(fn, k % 8, rng.integers(0, 2, 148), att=k % 7)
        i = s.submit(0, d)
        assert i == m.submit(0, d)
        ex.add(i, d)
    out = torch.empty((1, n * 625), dtype=torch.complex64, device="cuda:0")
    s.render(n, out=out)
    src = m.render(n)[0]
    torch.cuda.synchronize()
    for a in list(rng.integers(0, n - 64, 6)) + [0, n - 64, n - 300]:
        a = int(a)
        want = ex.stream(src[a:a + 64], a % 8, 0, M.FILLER_DUMMY)
        got = out[0, a * 625:(a + 64) * 625].cpu().numpy()
        assert np.array_equal(got, want), a


def test_refusals(trx):
    import torch
    s = trxhip.TxScheduler(trx, chans=3, sps=4, max_slots=64)
    with pytest.raises(trxhip.TrxHipError):
        s.render(8)                                                     # before set_clock
    s.set_clock(0, 0)
    with pytest.raises(trxhip.TrxHipError):
        s.render(65)                                                    # more slots than configured
    fe = trxhip.TxFrontEnd(trx, chans=2)
    with pytest.raises(trxhip.TrxHipError):
        s.render_frontend(8, fe)                                        # chans differ
    small = torch.empty((3, 100), dtype=torch.complex64, device="cuda:0")
    with pytest.raises(trxhip.TrxHipError):
        s.render(8, out=small)                                          # output too small
    for bad in [lambda: s.set_slot(3, 0, 1), lambda: s.set_slot(0, 8, 1), lambda: s.set_muted(3, 1),
                lambda: s.submit(-1, M.dgram(0, 0, [0] * 148))]:
        with pytest.raises(trxhip.TrxHipError):
            bad()
    assert s.clock() == (0, 0)
    cf, _ = s.render(8)
    torch.cuda.synchronize()
    assert (cf.cpu().numpy() == 0).all()                                # NONE everywhere: zeros
