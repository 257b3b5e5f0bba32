"""The uplink burst scheduler at one sample per symbol on the GPU (pytest -m gpu): an object from trxhip_rx_sched_create_sps()
against the entry points it stands for.  A 1-SPS stream is slots of 157 / 156 / 156 / 156 samples back to back; the expected
records, soft rows and datagrams are what trxhip_detect_demod_batch(sps = 1) + trxhip_pack_trxd_wire_batch give over the same
slots gathered by length into a batch of 156-sample rows and one of 157-sample rows (both pinned to the reference by
test_gpu_kernel_instances.py and test_gpu_trxd_hostpipe.py), so every comparison is byte for byte.  Slot times, types, the
noise ring and the counters come from tests/rx_sched_model_1sps.py run over the device's own energies and return codes."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_inputs as I  # noqa: E402
import rx_sched_model_1sps as M  # noqa: E402
from osmo_trx_amd import synth, trxhip  # noqa: E402

pytestmark = pytest.mark.gpu
FULL = 32767.0
TSC = 3
FRAMES = 204                                   # twice the longest modulus (102): 1632 slots per channel
N = FRAMES * 8
# I, IV, V, VII, XIII (TSC without EDGE), FILL, NONE, LOOPBACK / VII, I, XIII, V, II, III, VI, FILL / channel 2 is muted
COMBS = ([1, 4, 5, 7, 13, M.COMB_FILL, M.COMB_NONE, M.COMB_LOOPBACK], [7, 1, 13, 5, 2, 3, 6, M.COMB_FILL],
         [1, 4, M.COMB_FILL, M.COMB_NONE, 1, 1, 5, 7])
VERSIONS = (0, 1, 1)
OFFSETS = (0.0, 9.0, 4.0)
MUTED = (False, False, True)
CHANS = 3


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = trxhip.TrxHip(0)
    yield t
    t.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def raw(a):
    """the bytes of an array (a field of a structured array is not contiguous); NaN compares equal to the same NaN"""
    return np.ascontiguousarray(a).view(np.uint8)


def slot_lens(tn0, n):
    return 156 + ((tn0 + np.arange(n)) % 4 == 0).astype(np.int64)


def slot_starts(lens):
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)


def lay_out(rows, lens, extra=1):
    """rows [n, 157, ...] -> the stream: the first lens[k] samples of row k back to back, + `extra` zero samples (so that the
    last slot is cut: the strict `>`)"""
    import torch
    keep = torch.arange(157, device=rows.device)[None, :] < torch.from_numpy(lens).to(rows.device)[:, None]
    x = rows[keep]
    return torch.cat([x, torch.zeros((extra,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)])


def configure(o, tn0):
    o.set_clock(2715648 - 50, tn0)                   # the hyperframe wraps inside the stream
    for c in range(CHANS):
        for tn in range(8):
            o.set_slot(c, tn, COMBS[c][tn])
        o.set_trxd_version(c, VERSIONS[c])
        o.set_muted(c, MUTED[c])
    o.set_handover(2, 1, True)                       # SDCCH/4 subslot 1 of TN 2 (combination V on channel 0)
    o.set_handover(1, 0, True)                       # TCH/F on TN 1 of channel 1


def new_sched(trx, tn0=0, exact=False, max_slots=N):
    s = trxhip.RxScheduler(trx, chans=CHANS, sps=1, tsc=TSC, ul_fn_offset=-2, exact=exact, full_scale=FULL, max_slots=max_slots)
    configure(s, tn0)
    for c in range(CHANS):
        s.set_rssi_offset(c, OFFSETS[c])
    return s


def new_model(tn0=0):
    m = M.Model(CHANS, tsc=TSC, ul_fn_offset=-2)
    configure(m, tn0)
    return m


def clipped_noise(n, seed):
    """int16[n, 157, 2] rows of noise loud enough to pass maxAmplitude() > 30000 (sigProcLib.cpp:1746-1750) in every row"""
    import torch
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal((n, 157, 2)) * 14000.0).clip(-32768, 32767).astype(np.int16)
    assert (np.abs(x.astype(np.int32))[:, :156].max((1, 2)) > 30000).all()
    return torch.from_numpy(x)


@functools.lru_cache(None)
def burst_pools():
    nb, _, truth = synth.make_normal_bursts(CHANS * N, "cpu", 1, seed=201, tsc=TSC, p_noise=0.1, p_clip=0.1, burst_len=157)
    assert truth["clipped"].sum() > 20 and truth["noise_only"].sum() > 20
    ab, _, _ = I.access_bursts_1sps(CHANS * N, 157, False, seed=202)
    return nb, ab, clipped_noise(CHANS * N, 205)


class Scenario:
    """CHANS channels' streams of N slots + 1 sample from a clock at TN tn0: rows placed by the model's slot type (normal bursts
    with clipped and noise-only rows among them on TSC, IDLE and OFF slots, access bursts on RACH slots), every 11th slot loud
    noise whatever its type.  A row is 157 samples; a slot of 156 takes the first 156 (the last lies in the guard period)."""

    def __init__(self, tn0):
        import torch
        self.tn0 = tn0
        m = new_model(tn0)
        self.lens = np.array(m.slot_lens(N * 1250 // 8 + 1), dtype=np.int64)
        assert len(self.lens) == N and np.array_equal(self.lens, slot_lens(tn0, N))
        self.plan = m.cut(N * 1250 // 8 + 1)
        assert len(self.plan[0]) == N and m.carried == 1
        nb, ab, loud = burst_pools()
        chans = []
        for c in range(CHANS):
            typ = np.array([p[2] for p in self.plan[c]])
            rows = nb[c * N:(c + 1) * N].clone()
            idx = torch.from_numpy(np.flatnonzero(typ == M.RACH))
            rows[idx] = ab[c * N + idx]
            rows[5::11] = loud[c * N + 5:(c + 1) * N:11]
            chans.append(lay_out(rows, self.lens))
            assert set(typ) == {M.TSC, M.RACH, M.IDLE, M.OFF} or c == 1, (c, set(typ))
        self.stream = torch.stack(chans).to("cuda:0")
        assert self.stream.shape == (CHANS, N * 1250 // 8 + 1, 2)

    def params_meta(self, c):
        plan = self.plan[c]
        p = np.zeros(len(plan), dtype=trxhip.PARAMS_DTYPE)
        m = np.zeros(len(plan), dtype=trxhip.TRXD_META_DTYPE)
        a = np.array(plan, dtype=np.int64).reshape(-1, 4)
        m["fn"], m["tn"], p["type"], p["max_toa"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        p["tsc"] = TSC
        m["version"] = VERSIONS[c]
        return p, m


@functools.lru_cache(None)
def scenario(tn0):
    return Scenario(tn0)


def batch_calls(trx, x, lens, p, m, rssi_offset, pick=None):
    """The two existing entry points over the slots `pick` (default: all) of one channel's stream x (int16[n, 2] or
    complex64[n], device), gathered by length into rows of 156 and rows of 157 -> (results, pkt, pkt_len, soft) in pick's order"""
    import torch
    starts = slot_starts(lens)
    pick = np.arange(len(lens)) if pick is None else np.asarray(pick)
    k = len(pick)
    res = np.zeros(k, dtype=trxhip.RESULT_DTYPE)
    pkt, plen, soft = np.zeros((k, 160), np.uint8), np.zeros(k, np.int16), np.zeros((k, 148), np.float32)
    for L in (156, 157):
        sel = np.flatnonzero(lens[pick] == L)
        if not len(sel):
            continue
        at = dev(starts[pick[sel]])[:, None] + torch.arange(L, device="cuda:0")[None, :]
        rows = x[at].contiguous()
        pt = trx.params_tensor(p[sel])
        r, so = trx.detect_demod(rows, pt, sps=1, full_scale=FULL, soft_stride=148)
        pk, pl = trx.pack_trxd_wire(r, pt, so, dev(m[sel].view(np.uint8).reshape(-1, 8)), pkt_stride=160, rssi_offset=rssi_offset)
        torch.cuda.synchronize()
        res[sel], pkt[sel], plen[sel], soft[sel] = trx.results_to_numpy(r), pk.cpu().numpy(), pl.cpu().numpy(), so.cpu().numpy()
    return res, pkt, plen, soft


def check_records(ind, res, want):
    """ind: the scheduler's records of one channel; res: the batch call's result records; want: the model's run over res"""
    for k in ("rc", "toa", "ci", "tsc", "rssi"):
        assert np.array_equal(raw(ind[k]), raw(res[k])), (k, np.flatnonzero(ind[k] != res[k])[:10])
    assert np.array_equal(ind["nbits"], 4 * res["nbits_div4"].astype(np.uint16))
    assert np.array_equal(ind["fn"], [w["fn"] for w in want]) and np.array_equal(ind["tn"], [w["tn"] for w in want])
    assert np.array_equal(ind["type"], [w["type"] for w in want])
    assert np.array_equal(ind["flags"], [w["flags"] for w in want])
    lev = np.array([w["noise_lev"] for w in want], dtype=np.float32)
    assert np.array_equal(raw(ind["noise_lev"]), raw(lev)), np.flatnonzero(ind["noise_lev"] != lev)[:10]
    for k in ("rc", "tsc", "nbits"):
        assert np.array_equal(ind[k], [w[k] for w in want]), k
    for k in ("toa", "ci", "rssi"):
        assert np.array_equal(raw(ind[k]), raw(np.array([w[k] for w in want], dtype=np.float32))), k


def as_kind(x, cf32):
    import torch
    return torch.view_as_complex(x.to(torch.float32)) if cf32 else x


def one_piece(trx, scn, cf32):
    """the whole stream in one pull -> (scheduler, ind, pkt, pkt_len, soft)"""
    import torch
    s = new_sched(trx, scn.tn0, exact=cf32)          # TRXHIP_FLAG_EXACT_DEMOD is accepted at 1 SPS and changes nothing
    pkt, plen, ind, soft = s.pull(as_kind(scn.stream, cf32), want_soft=True)
    torch.cuda.synchronize()
    assert pkt.shape == (CHANS, N, 160) and soft.shape == (CHANS, N, 148)
    return s, s.ind_to_numpy(ind), pkt.cpu().numpy(), plen.cpu().numpy(), soft.cpu().numpy()


@pytest.mark.parametrize("kind", ["s16", "cf32"])
def test_pull_equals_batch_calls(trx, kind):
    cf32 = kind == "cf32"
    scn = scenario(0)
    s, ind, pkt, plen, soft = one_piece(trx, scn, cf32)
    m = new_model()
    plan = m.cut(scn.stream.shape[1])
    assert s.clock() == m.clock and s.slots(0) == 0 and s.slots(156) == 0 and s.slots(157) == 1   # a slot of 157 is next
    x = as_kind(scn.stream, cf32)
    for c in range(CHANS):
        got_plan = s.plan(c)
        assert np.array_equal(np.stack([got_plan[k] for k in ("fn", "tn", "type", "max_toa")], 1), np.array(plan[c]))
        p, mt = scn.params_meta(c)
        if MUTED[c]:
            # no DSP runs on a muted slot (Transceiver.cpp:719-721): the detector saw it as OFF; the packer sees the slot's type
            pd = p.copy()
            pd["type"] = M.OFF
            res, _, _, _ = batch_calls(trx, x[c], scn.lens, pd, mt, OFFSETS[c])
            want = m.run(c, plan[c], res)
            assert np.array_equal(ind[c]["flags"], [w["flags"] for w in want])
            off = np.array([r[2] for r in plan[c]]) == M.OFF
            assert off.any() and (~off).any()
            assert (ind[c]["flags"][~off] == (trxhip.ULIND_MUTED | trxhip.ULIND_IDLE)).all()
            assert (ind[c]["rc"] == 0).all() and (ind[c]["rssi"] == 0).all() and (ind[c]["noise_lev"] == 0).all()
            assert (plen[c][off] == 0).all() and (plen[c][~off] == 11).all()         # v1: an idle indication with rssi byte 0
            idle = pkt[c][~off]
            assert (idle[:, 5] == 0).all() and (idle[:, 8] == 0x80).all() and np.array_equal(idle[:, 0], 0x10 | ind[c]["tn"][~off])
            assert not soft[c].any()
            ring, itr, lev = s.noise_state(c)
            assert not ring.any() and itr == 0 and lev == 0
            continue
        res, wpkt, wlen, wsoft = batch_calls(trx, x[c], scn.lens, p, mt, OFFSETS[c])
        assert np.array_equal(plen[c], wlen), np.flatnonzero(plen[c] != wlen)[:10]
        assert np.array_equal(pkt[c], wpkt), np.flatnonzero((pkt[c] != wpkt).any(1))[:10]
        assert np.array_equal(soft[c].view(np.uint32), wsoft.view(np.uint32)), np.flatnonzero((soft[c] != wsoft).any(1))[:10]
        check_records(ind[c], res, m.run(c, plan[c], res))
        assert s.counters(c) == m.ctr[c]
        ring, itr, lev = s.noise_state(c)
        assert np.array_equal(ring.view(np.uint32), m.noise[c].ring.view(np.uint32)) and itr == m.noise[c].itr
        assert lev.view(np.uint32) == m.noise[c].lev.view(np.uint32)
        if VERSIONS[c] == 0:
            assert (plen[c][ind[c]["flags"] != 0] == 0).all()                 # v0 sends no idle indication
        else:
            assert (plen[c][(ind[c]["flags"] & trxhip.ULIND_OFF) == 0] >= 11).all()
    typ0 = ind[0]["type"]
    assert set(typ0) == {M.TSC, M.RACH, M.IDLE, M.OFF}
    for t in (M.TSC, M.RACH):
        assert (ind[0]["rc"][typ0 == t] == t).mean() > 0.5, t                  # the rows are found as what they are
    for L in (156, 157):
        assert (ind[0]["rc"][scn.lens == L] > 0).mean() > 0.25, L              # ... in slots of either length
    assert m.ctr[0]["rx_clipping"] > 0 and m.noise[0].itr > 0 and m.noise[1].lev > 0


def test_ext_rach_object(trx):
    """a second object with cfg.ext_rach: combination IV on every TN, 11-bit access bursts of all three sync sequences"""
    import torch
    n = 256
    rows, _, ts = I.access_bursts_1sps(n, 157, True, seed=211)
    for cf32 in (False, True):
        s = trxhip.RxScheduler(trx, chans=1, sps=1, ext_rach=True, full_scale=FULL, max_slots=n)
        m = M.Model(1, ext_rach=True)
        for o in (s, m):
            o.set_clock(40, 2)
            for tn in range(8):
                o.set_slot(0, tn, 4)
            o.set_trxd_version(0, 1)
        lens = slot_lens(2, n)
        x = as_kind(lay_out(rows, lens).to("cuda:0"), cf32)
        pkt, plen, ind, soft = s.pull(x, want_soft=True)
        torch.cuda.synchronize()
        plan = m.cut(x.shape[0])[0]
        assert len(plan) == n and all(r[2] == M.EXT_RACH for r in plan)
        p = np.zeros(n, dtype=trxhip.PARAMS_DTYPE)
        mt = np.zeros(n, dtype=trxhip.TRXD_META_DTYPE)
        p["type"], p["max_toa"] = M.EXT_RACH, 63
        mt["fn"], mt["tn"], mt["version"] = [r[0] for r in plan], [r[1] for r in plan], 1
        res, wpkt, wlen, wsoft = batch_calls(trx, x, lens, p, mt, 0.0)
        ind = s.ind_to_numpy(ind)[0]
        assert np.array_equal(plen[0].cpu().numpy(), wlen) and np.array_equal(pkt[0].cpu().numpy(), wpkt)
        assert np.array_equal(soft[0].cpu().numpy().view(np.uint32), wsoft.view(np.uint32))
        check_records(ind, res, m.run(0, plan, res))
        det = ind["rc"] == M.EXT_RACH
        assert det.mean() > 0.8 and (np.bincount(ind["tsc"][det], minlength=3)[:3] >= 30).all()


@pytest.mark.parametrize("tn0", range(4))
def test_chunking_never_changes_the_output(trx, tn0):
    """the same streams in uneven chunks, for each of the four TN phases the clock can start in"""
    import torch
    scn = scenario(tn0)
    s1, ind1, pkt1, plen1, soft1 = one_piece(trx, scn, False)
    s = new_sched(trx, tn0)
    total = scn.stream.shape[1]
    rng = np.random.default_rng(60 + tn0)
    sizes = [1, 155, 156, 157, 158, 313, 1250, 1251, 0, 17, 17] + [int(v) for v in rng.integers(1, 4000, 12)]
    sizes.append(total - sum(sizes))
    assert sizes[-1] > 100000
    m = new_model(tn0)
    parts, at = [], 0
    for n in sizes:
        want_n = s.slots(n)
        assert want_n == m.slots(n)
        pkt, plen, ind, soft = s.pull(scn.stream[:, at:at + n].contiguous(), want_soft=True)
        m.cut(n)
        assert pkt.shape[1] == want_n and s.clock() == m.clock
        parts.append((s.ind_to_numpy(ind), pkt, plen, soft))
        at += n
    torch.cuda.synchronize()
    # 1 + 155 samples: 156 stay in front of a slot of 156 (tn0 != 0), they are no slot of 157 either (tn0 == 0): the strict `>`
    assert [p[0].shape[1] for p in parts][:3] == [0, 0, 1]
    ind = np.concatenate([p[0] for p in parts], 1)
    pkt, plen, soft = (torch.cat([p[k] for p in parts], 1).cpu().numpy() for k in (1, 2, 3))
    assert ind.shape == ind1.shape
    assert np.array_equal(ind.view(np.uint8), ind1.view(np.uint8)), np.argwhere(ind != ind1)[:10]
    assert np.array_equal(plen, plen1) and np.array_equal(pkt, pkt1)
    assert np.array_equal(soft.view(np.uint32), soft1.view(np.uint32))
    assert s.clock() == s1.clock()
    assert (ind1[0]["rc"] > 0).mean() > 0.2
    for c in range(CHANS):
        assert s.counters(c) == s1.counters(c)
        a, b = s.noise_state(c), s1.noise_state(c)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1] and a[2].view(np.uint32) == b[2].view(np.uint32)


def test_stale_sample_behind_a_short_slot(trx):
    """One channel, 65536 slots: each of the kernel's 4096 resident waves takes several, slots of 156 behind slots of 157.  The
    kernel's LDS slice holds 157 samples; after a slot of 157 its sample 156 still lies there (delayed and scaled, or raw), and
    the delay filter of a 156-sample burst with TOA >= 1 symbol reads that place, which the row kernel finds zero.  Normal bursts
    of the searched TSC, delays 1.25 .. 4 symbols; every slot against the batch calls.
    What a slot of 157 leaves in that place depends on it: detected with TOA >= 1 symbol, its own delayed sample 156 comes from
    behind the burst and is exactly zero, which would hide a kernel that leaves it there.  So the slots of 157 on TN 4 carry
    noise instead (nothing detected: the raw sample stays, some thousand against the demodulated burst's unit scale); those on
    TN 0 and all slots of 156 are the bursts above.  Run against a build without the zero store, 33 % of the 156-sample rows differ."""
    import torch
    n = 1 << 16
    rows, _, _ = synth.make_normal_bursts(n, "cuda:0", 1, seed=77, tsc=TSC, delay_sym=(1.25, 4.0), p_noise=0.0, p_clip=0.0,
                                          snr_range=(15.0, 30.0), burst_len=157)
    lens = slot_lens(0, n)
    gen = torch.Generator(device="cuda:0").manual_seed(78)
    rows[4::8] = (torch.randn((n // 8, 157, 2), generator=gen, device="cuda:0") * 3000.0).round().clamp(-29000, 29000).to(torch.int16)
    x = lay_out(rows, lens)
    s = trxhip.RxScheduler(trx, chans=1, sps=1, tsc=TSC, full_scale=FULL, max_slots=n)
    s.set_clock(0, 0)
    for tn in range(8):
        s.set_slot(0, tn, 1)
    s.set_trxd_version(0, 1)
    pkt, plen, ind, soft = s.pull(x, want_soft=True)
    torch.cuda.synchronize()
    assert pkt.shape[1] == n
    p = np.zeros(n, dtype=trxhip.PARAMS_DTYPE)
    mt = np.zeros(n, dtype=trxhip.TRXD_META_DTYPE)
    p["type"], p["tsc"], p["max_toa"] = M.TSC, TSC, 30
    k = np.arange(n)
    mt["fn"], mt["tn"], mt["version"] = k // 8, k % 8, 1
    res, wpkt, wlen, wsoft = batch_calls(trx, x, lens, p, mt, 0.0)
    short = lens == 156
    met = short & (res["rc"] == M.TSC) & (res["toa"] >= 1.0)
    assert met.sum() >= 0.9 * short.sum(), (met.sum(), short.sum())           # the case was met
    ind = s.ind_to_numpy(ind)[0]
    soft = soft[0].cpu().numpy()
    bad = np.flatnonzero((soft.view(np.uint32) != wsoft.view(np.uint32)).any(1))
    assert not len(bad), (len(bad), len(bad) / short.sum(), bad[:10], lens[bad[:10]])
    for f in ("rc", "toa", "ci", "tsc", "rssi"):
        assert np.array_equal(raw(ind[f]), raw(res[f])), f
    assert np.array_equal(plen[0].cpu().numpy(), wlen) and np.array_equal(pkt[0].cpu().numpy(), wpkt)


def test_noise_ring_matches_model(trx):
    """channel 0: FILL on every TN; channel 1: combination I, never IDLE.  Pulls of 7, 33, 1, (9 muted), 4096 slots"""
    import torch
    rng = np.random.default_rng(8)
    cuts = [7, 33, 1, 9, 4096]
    total = sum(cuts)
    amp = rng.uniform(5.0, 3000.0, (2, total, 1, 1))
    rows = np.round(rng.standard_normal((2, total, 157, 2)) * amp).clip(-32768, 32767).astype(np.int16)
    lens = slot_lens(5, total)
    x = torch.stack([lay_out(torch.from_numpy(rows[c]), lens) for c in range(2)]).to("cuda:0")
    s = trxhip.RxScheduler(trx, chans=2, sps=1, full_scale=FULL, max_slots=4096)
    m = M.Model(2)
    for o in (s, m):
        o.set_clock(9, 5)
        for tn in range(8):
            o.set_slot(0, tn, M.COMB_FILL)
            o.set_slot(1, tn, 1)
    at = first = 0
    for i, k in enumerate(cuts):
        n = int(lens[first:first + k].sum()) + (1 if i == 0 else 0)          # one sample more: every slot is cut
        for o in (s, m):
            o.set_muted(0, i == 3)
        before = s.noise_state(0)
        _, _, ind, _ = s.pull(x[:, at:at + n].contiguous())
        plan = m.cut(n)
        assert ind.shape[1] == k == len(plan[0]) and m.carried == 1
        ind = s.ind_to_numpy(ind)
        for c in range(2):
            p = np.zeros(total, dtype=trxhip.PARAMS_DTYPE)
            pick = np.arange(first, first + k)
            p["type"][pick] = [r[2] for r in plan[c]]
            p["max_toa"][pick] = [r[3] for r in plan[c]]
            res, _, _, _ = batch_calls(trx, x[c], lens, p[pick], np.zeros(k, dtype=trxhip.TRXD_META_DTYPE), 0.0, pick=pick)
            want = m.run(c, plan[c], res)
            lev = np.array([w["noise_lev"] for w in want], dtype=np.float32)
            assert np.array_equal(raw(ind[c]["noise_lev"]), raw(lev)), (i, c, np.flatnonzero(ind[c]["noise_lev"] != lev)[:10])
            assert np.array_equal(ind[c]["flags"], [w["flags"] for w in want])
            ring, itr, nl = s.noise_state(c)
            assert np.array_equal(ring.view(np.uint32), m.noise[c].ring.view(np.uint32)), (i, c)
            assert itr == m.noise[c].itr and nl.view(np.uint32) == m.noise[c].lev.view(np.uint32)
            assert s.counters(c) == m.ctr[c]
        if i == 3:                                                        # the muted pull: ring, itr and level untouched
            after = s.noise_state(0)
            assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]
            assert (ind[0]["flags"] == (trxhip.ULIND_MUTED | trxhip.ULIND_IDLE)).all() and (ind[0]["rssi"] == 0).all()
        at += n
        first += k
    assert m.noise[0].itr == (7 + 33 + 1 + 4096 - 1) % 20 + 1 and m.noise[0].lev > 0
    ring, itr, lev = s.noise_state(1)
    assert not ring.any() and itr == 0 and lev == 0


def test_loopback_both_schedulers(trx):
    """TxScheduler(sps=1) -> additive noise (sigma 20 at full scale 6000) -> RxScheduler(sps=1), both clocks started at the same
    (FN, TN): the downlink scheduler renders the 157 / 156 / 156 / 156 pattern the uplink scheduler cuts.  The 4-SPS loopback's
    bars: hard bits 3 .. 144 wrong in fewer than 1e-3 of positions, false alarms on empty slots under 3 %.  Channel 0 carries a
    burst in every slot but TN 6 (NONE on the transmit side: zeros); channel 1 is muted on the transmit side."""
    import torch
    import tx_sched_model as TM
    from test_gpu_tx_frontend import _unambiguous_bursts
    chans, n_slots, tsc, fn0, tn0 = 2, 52 * 8, 5, 17, 3
    rng = np.random.default_rng(43)
    slot = np.arange(n_slots)
    tn = (tn0 + slot) % 8
    fn = fn0 + (tn0 + slot) // 8
    bits = _unambiguous_bursts(np.full(n_slots, tsc), rng)
    tx = trxhip.TxScheduler(trx, chans=chans, sps=1, filler=TM.FILLER_ZERO, full_scale=6000.0, queue_cap=1024, max_slots=1024)
    tx.set_clock(fn0, tn0)
    none = tn == 6
    for c in range(chans):
        for t in range(8):
            tx.set_slot(c, t, TM.COMB_NONE if t == 6 else 1)
    for i in range(n_slots):
        if not none[i]:
            assert tx.submit(0, TM.dgram(int(fn[i]), int(tn[i]), bits[i])) >= 0
            assert tx.submit(1, TM.dgram(int(fn[i]), int(tn[i]), bits[i])) >= 0
    tx.set_muted(1, True)
    _, x = tx.render(n_slots, cf32=False, s16_scales=[1.0] * chans)
    torch.cuda.synchronize()
    assert x.shape == (chans, n_slots * 1250 // 8, 2)
    noise = torch.from_numpy(np.round(rng.standard_normal(tuple(x.shape)) * 20.0).astype(np.int16)).to("cuda:0")
    x = (x.to(torch.int32) + noise).clamp(-32768, 32767).to(torch.int16)
    rx = trxhip.RxScheduler(trx, chans=chans, sps=1, tsc=tsc, full_scale=FULL, max_slots=1024)
    rx.set_clock(fn0, tn0)                                 # the transmit clock
    rx.set_max_toa(20, 63)
    for c in range(chans):
        rx.set_trxd_version(c, 1)
        for t in range(8):
            rx.set_slot(c, t, 1)
    pkt, plen, ind, _ = rx.pull(x)
    torch.cuda.synchronize()
    n = n_slots - 1                                        # the last slot waits for one sample more
    assert pkt.shape[1] == n and rx.slots(1) == 1
    pkt, plen, ind = pkt.cpu().numpy(), plen.cpu().numpy(), rx.ind_to_numpy(ind)
    none, tn, fn = none[:n], tn[:n], fn[:n]
    found = plen == 11 + 148
    assert ((plen == 11) | found).all()
    assert found[1].mean() < 0.03                          # the muted channel: the receiver's false alarms only
    assert found[0][none].mean() < 0.03
    sent = ~none
    assert found[0][sent].all(), np.flatnonzero(sent & ~found[0])[:10]
    d = pkt[0][sent]
    assert np.array_equal(d[:, 0], 0x10 | tn[sent]) and np.array_equal(d[:, 4] | (d[:, 3].astype(np.int64) << 8), fn[sent])
    assert (d[:, 8] == tsc).all()                          # not idle, GMSK, its TSC
    assert (ind[0]["rc"][sent] == M.TSC).all() and (ind[0]["tsc"][sent] == tsc).all()
    hard = (d[:, 11:11 + 148] > 127).astype(np.uint8)
    assert (hard[:, 3:145] != bits[:n][sent][:, 3:145]).mean() < 1e-3


def test_full_size_pull(trx):
    """one channel, 262144 slots in one pull (41 M samples), 64 slots checked against the batch calls"""
    import torch
    n = 1 << 18
    rows, _, _ = synth.make_normal_bursts(n, "cuda:0", 1, seed=55, max_toa=30, burst_len=157)
    lens = slot_lens(5, n)
    x = lay_out(rows, lens)
    del rows
    assert x.shape[0] == n * 1250 // 8 + 1
    s = trxhip.RxScheduler(trx, chans=1, sps=1, tsc=TSC, full_scale=FULL, max_slots=n)
    m = M.Model(1, tsc=TSC)
    for o in (s, m):
        o.set_clock(123456, 5)
        for tn in range(8):
            o.set_slot(0, tn, 1)
        o.set_trxd_version(0, 1)
    pkt, plen, ind, _ = s.pull(x)
    torch.cuda.synchronize()
    assert pkt.shape == (1, n, 160)
    plan = m.cut(x.shape[0])[0]
    assert len(plan) == n and s.clock() == m.clock
    fn, tn = np.array([r[0] for r in plan]), np.array([r[1] for r in plan])
    ind = s.ind_to_numpy(ind)[0]
    rng = np.random.default_rng(6)
    pick = np.sort(np.concatenate([rng.choice(np.arange(1, n - 1), 62, replace=False), [0, n - 1]]))
    assert set(lens[pick]) == {156, 157}
    p = np.zeros(len(pick), dtype=trxhip.PARAMS_DTYPE)
    mt = np.zeros(len(pick), dtype=trxhip.TRXD_META_DTYPE)
    p["type"], p["tsc"], p["max_toa"] = M.TSC, TSC, 30
    mt["fn"], mt["tn"], mt["version"] = fn[pick], tn[pick], 1
    res, wpkt, wlen, _ = batch_calls(trx, x, lens, p, mt, 0.0, pick=pick)
    assert np.array_equal(plen[0].cpu().numpy()[pick], wlen) and np.array_equal(pkt[0][dev(pick)].cpu().numpy(), wpkt)
    for k in ("rc", "toa", "ci", "tsc", "rssi"):
        assert np.array_equal(raw(ind[k][pick]), raw(res[k])), k
    assert np.array_equal(ind["fn"], fn) and np.array_equal(ind["tn"], tn)
    assert (ind["rc"] == M.TSC).mean() > 0.1                                  # TSC i % 8: every eighth row carries mTSC
    r = np.zeros(n, dtype=trxhip.RESULT_DTYPE)                                # the counters: the model over the device's records
    r["rc"], r["toa"], r["ci"], r["tsc"], r["rssi"], r["nbits_div4"] = ind["rc"], ind["toa"], ind["ci"], ind["tsc"], ind["rssi"], ind["nbits"] // 4
    m.run(0, plan, r)
    assert s.counters(0) == m.ctr[0] and m.ctr[0]["rx_clipping"] > 100
    assert (ind["noise_lev"] == 0).all()


def test_refused_pulls_on_a_device_object(trx):
    """Every refusal a pull makes only with a context -- outputs too small, a missing or misaligned buffer, a row stride the
    packer does not take, a chunk longer than its stride, complex64 over an int16 remainder -- is TRXHIP_EINVAL, launches nothing
    and leaves the object where an object that never saw the call is."""
    import torch
    EINVAL = -22
    L = trx.L
    n = 24
    rows, _, _ = synth.make_normal_bursts(2 * n, "cpu", 1, seed=31, tsc=TSC, p_noise=0.2, p_clip=0.2, burst_len=157)
    lens = slot_lens(2, n)
    x = torch.stack([lay_out(rows[c * n:(c + 1) * n], lens, extra=64) for c in range(2)])
    x[:, -64:] = 7
    x = x.to("cuda:0")
    xc = torch.view_as_complex(x.to(torch.float32))
    objs = []
    for _ in range(2):
        s = trxhip.RxScheduler(trx, chans=2, sps=1, tsc=TSC, full_scale=FULL, max_slots=n)
        s.set_clock(50, 2)
        for c in range(2):
            for tn in range(8):
                s.set_slot(c, tn, [1, M.COMB_FILL, 7, 1, M.COMB_NONE, 13, 1, 5][tn])
            s.set_trxd_version(c, 1)
        objs.append(s)
    s, clean = objs
    first = int(lens[:10].sum()) + 30                                     # 10 slots, 30 samples stay
    outs = [o.pull(x[:, :first].contiguous()) for o in objs]
    torch.cuda.synchronize()
    assert outs[0][0].shape[1] == 10
    rest = x[:, first:].contiguous()
    nr = rest.shape[1]
    k = s.slots(nr)
    assert k == 14
    pkt = torch.full((2, k, 160), 0xAB, dtype=torch.uint8, device="cuda:0")
    plen = torch.full((2, k), -1, dtype=torch.int16, device="cuda:0")
    ind = torch.full((2, k, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    soft = torch.full((2, k, 148), -7.0, dtype=torch.float32, device="cuda:0")
    restc = xc[:, first:].contiguous()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)    # noqa: E731
    ns, nc = C.c_size_t(99), C.c_size_t(99)
    st = trx._stream()

    def s16(d_in=None, stride=nr, count=nr, d_pkt=None, pkt_stride=160, d_len=None, d_ind=None, d_soft=None, out_slots=k):
        return L.trxhip_rx_sched_pull_s16(s.h, p(rest) if d_in is None else d_in, stride, count, p(pkt) if d_pkt is None else d_pkt,
                                          pkt_stride, p(plen) if d_len is None else d_len, p(ind) if d_ind is None else d_ind,
                                          p(soft) if d_soft is None else d_soft, out_slots, C.byref(ns), C.byref(nc), st)

    null = C.c_void_p(None)
    refused = {
        "out_slots = n - 1": s16(out_slots=k - 1),
        "no d_ind": s16(d_ind=null),
        "no d_pkt": s16(d_pkt=null),
        "no d_pkt_len": s16(d_len=null),
        "no d_in": s16(d_in=null),
        "pkt_stride 158": s16(pkt_stride=158),
        "pkt_stride 162": s16(pkt_stride=162),
        "d_in misaligned": s16(d_in=p(rest, 2), count=nr - 1, stride=nr - 1),
        "d_pkt misaligned": s16(d_pkt=p(pkt, 2)),
        "d_ind misaligned": s16(d_ind=p(ind, 2)),
        "d_pkt_len misaligned": s16(d_len=p(plen.view(torch.uint8), 1)),
        "d_soft misaligned": s16(d_soft=p(soft.view(torch.uint8), 2)),
        "in_stride < n_samples": s16(stride=nr - 1),
        "more than max_slots": s16(count=(n + 1) * 157, stride=(n + 1) * 157),
        "cf32 over an int16 remainder": L.trxhip_rx_sched_pull_cf32(s.h, p(restc), nr, nr, p(pkt), 160, p(plen), p(ind), p(soft), k,
                                                                    C.byref(ns), C.byref(nc), st),
    }
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in refused.values()), {w: rc for w, rc in refused.items() if rc != EINVAL}
    assert (ns.value, nc.value) == (99, 99)
    assert (pkt == 0xAB).all() and (plen == -1).all() and (ind == 0xAB).all() and (soft == -7.0).all()      # nothing was launched
    assert s.clock() == clean.clock() and s.slots(0) == clean.slots(0) == 0 and s.slots(nr) == clean.slots(nr) == k
    for c in range(2):
        assert s.counters(c) == clean.counters(c)
        a, b = s.noise_state(c), clean.noise_state(c)
        assert np.array_equal(raw(a[0]), raw(b[0])) and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
    got = [o.pull(rest, want_soft=True) for o in objs]
    torch.cuda.synchronize()
    for a, b in zip(*got):
        assert a.shape[1] == k and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in zip(*outs):
        if a is not None:
            assert torch.equal(a, b)
    assert (got[0][1] > 0).any() and s.noise_state(0)[1] > 0
    for c in range(2):
        assert s.counters(c) == clean.counters(c)
    assert s.clock() == clean.clock() == (50 + (2 + 24) // 8, (2 + 24) % 8)
