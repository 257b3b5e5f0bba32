"""The burst loop of the normal-burst kernel (csrc/trx_kernel_nb.hip) as a state machine: what a wave carries from one burst
to the next (the deferred soft-bit stores and their masks, the pending miss record, the records parked 64 at a time, "a burst
was left", the next burst's prefetch) across every pair of neighbouring cases, across the record batch boundary inside the
loop, on both sides of the size at which the cross-die pool is switched on, and across two launches into the same buffers.
The comparison is that of tests/test_gpu_nb_window_regs.py: the split path against the general kernel alone
(set_nb_kernel(False)) as bytes, and a seeded sample against the oracle (decisions identical, soft bits within the header's
bar)."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from osmo_trx_amd import TrxHip, synth

pytestmark = pytest.mark.gpu

N_ORACLE = 1024                 # bursts per batch that also go through the CPU oracle
DEV = "cuda:0"
FUSED_SOFT_ATOL = O.header_constant("TRXHIP_FUSED_SOFT_ATOL")
KINDS = ("detected", "noise", "clipped", "foreign", "max_toa_33", "early", "late")


@pytest.fixture(scope="module")
def trx():
    t = TrxHip(0)
    yield t
    t.close()


FILL = 0xa5                     # what the split path's result buffer holds before the launch: a record nobody wrote keeps it


def split_and_general(trx, d_iq, params):
    d_p = trx.params_tensor(params)
    trx.set_nb_kernel(True)
    res_a = torch.full((len(params), 32), FILL, dtype=torch.uint8, device=DEV)
    res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4, results=res_a)
    torch.cuda.synchronize()
    trx.set_nb_kernel(False)
    res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    return res_a, soft_a, res_b, soft_b


def assert_bytes(res_a, soft_a, res_b, soft_b, rows=None):
    if rows is not None:
        res_a, soft_a, res_b, soft_b = res_a[rows], soft_a[rows], res_b[rows], soft_b[rows]
    bad = np.flatnonzero((res_a != res_b).any(dim=1).cpu().numpy())
    assert torch.equal(res_a, res_b), (len(bad), bad[:8])
    assert torch.equal(soft_a.view(torch.int32), soft_b.view(torch.int32)), \
        np.flatnonzero((soft_a != soft_b).any(dim=1).cpu().numpy())[:8]


def assert_oracle(trx, d_iq, params, res, soft, n_oracle=N_ORACLE):
    """decisions identical to the oracle's on the first n_oracle bursts, soft bits within the header's bar"""
    n = min(n_oracle, len(params))
    g = trx.results_to_numpy(res[:n])
    o_res, o_soft = O.pull_batch(d_iq[:n].cpu().numpy(), 4, params[:n])
    for k in ("rc", "tsc", "toa"):
        bad = np.flatnonzero(g[k] != o_res[k])
        assert bad.size == 0, (k, bad[:8], g[k][bad[:8]], o_res[k][bad[:8]])
    # the fused demodulator's statement of include/trxhip.h: |soft - ref| <= TRXHIP_FUSED_SOFT_ATOL * max(1, rms / (4 |amp|))
    amp = np.hypot(o_res["amp_re"], o_res["amp_im"])
    ratio = np.where(amp > 0, np.sqrt(np.maximum(o_res["energy"], 0)) / np.maximum(amp, 1e-30), 1.0)
    bar = (FUSED_SOFT_ATOL * np.maximum(1.0, ratio / 4.0))[:, None]
    err = np.abs(soft[:n].cpu().numpy() - o_soft)
    print("largest soft-bit error against the oracle, in bars:", float((err / bar).max()))
    assert (err <= bar).all(), float((err / bar).max())


def check(trx, d_iq, params, n_oracle=N_ORACLE):
    out = split_and_general(trx, d_iq, params)
    assert_bytes(*out)
    assert_oracle(trx, d_iq, params, out[0], out[1], n_oracle)
    return out


# ---- 1. every pair of neighbouring cases ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds_pool():
    """20 000 bursts of each kind, generated once on the device; a batch picks burst i from the pool of its kind"""
    n = 20000
    kw = dict(p_noise=0.0, p_clip=0.0)
    spec = {
        "detected": dict(max_toa=5, delay_sym=(0.0, 4.0), **kw),
        "noise": dict(max_toa=5, delay_sym=(0.0, 4.0), p_noise=1.0, p_clip=0.0),
        "clipped": dict(max_toa=5, delay_sym=(0.0, 4.0), p_noise=0.0, p_clip=1.0),
        "foreign": dict(max_toa=5, delay_sym=(0.0, 4.0), **kw),
        "max_toa_33": dict(max_toa=33, delay_sym=(0.0, 4.0), **kw),
        "early": dict(max_toa=5, delay_sym=(-3.0, -1.0), snr_range=(15.0, 30.0), **kw),
        "late": dict(max_toa=20, delay_sym=(10.5, 18.0), snr_range=(15.0, 30.0), **kw),
    }
    iqs, prms = [], []
    for k, name in enumerate(KINDS):
        iq, p, _ = synth.make_normal_bursts(n, DEV, 4, seed=9100 + k, **spec[name])
        if name == "foreign":
            p["type"] = O.EDGE
        iqs.append(iq)
        prms.append(p)
    return n, torch.stack(iqs), np.stack(prms)


def mixed_batch(kinds_pool, kinds):
    n, iqs, prms = kinds_pool
    idx = np.arange(n)
    d_iq = iqs[torch.from_numpy(kinds).to(DEV), torch.arange(n, device=DEV)]
    return d_iq, np.ascontiguousarray(prms[kinds, idx])


@pytest.mark.parametrize("last", [None, "foreign", "noise"])
def test_every_pair_of_neighbouring_cases(trx, kinds_pool, last):
    """more than 4096 bursts: every wave takes several (about five), one after the other, by ticket from its workgroup's range --
    which ones is the hardware's choice, so which kinds follow each other in a wave cannot be asserted from outside.  The
    kinds are drawn i.i.d.: the roughly 16 000 pairs of consecutive bursts of the 4096 waves are then i.i.d. pairs too, about
    330 of each of the 49 ordered pairs (none with probability 49 * exp(-330)), whatever the assignment.  `last`: the batch
    ends on a burst that is left behind / on a miss record"""
    n = kinds_pool[0]
    kinds = np.random.default_rng(9200 + (0 if last is None else 1 + KINDS.index(last))).integers(0, len(KINDS), n)
    if last is not None:
        kinds[-1] = KINDS.index(last)
    assert np.bincount(kinds, minlength=len(KINDS)).min() > 2000
    d_iq, params = mixed_batch(kinds_pool, kinds)
    res_a, soft_a, res_b, soft_b = check(trx, d_iq, params)
    r = trx.results_to_numpy(res_a)
    of = {name: kinds == k for k, name in enumerate(KINDS)}
    found = r["rc"] > 0
    # every kind occurred, by the records
    assert found[of["detected"]].mean() > 0.9
    assert (r["rc"][of["noise"]] == 0).mean() > 0.9
    assert (r["clip"][of["clipped"]] == 1).mean() > 0.9
    assert found[of["max_toa_33"]].mean() > 0.9
    # (a slot of another type: the second launch's record is there -- the fill pattern is gone; that it is the general kernel's
    # is the byte comparison below)
    rec = res_a.cpu().numpy()
    assert not (rec[of["foreign"]] == FILL).all(axis=1).any()
    assert ((r["rc"] == 1) & (r["nbits_div4"] == 37))[of["detected"]].mean() > 0.9
    assert (r["toa"][of["early"] & found] < -0.5).sum() > 100
    assert (r["toa"][of["late"] & found] > 9.5).sum() > 100
    # the two kinds that the kernel leaves behind carry the general kernel's bytes
    for name in ("foreign", "max_toa_33"):
        assert_bytes(res_a, soft_a, res_b, soft_b, rows=torch.from_numpy(np.flatnonzero(of[name])).to(DEV))
    if last is not None:
        assert_bytes(res_a, soft_a, res_b, soft_b, rows=slice(n - 64, n))


# ---- 2. the record batch boundary inside the loop ---------------------------------------------------------------------
@pytest.mark.parametrize("n,p_noise", [(327680, 0.0), (327680, 0.5), (655360, 0.5)])
def test_record_batch_boundary_inside_the_loop(trx, n, p_noise):
    """64 x 16 x 256 = 262 144 detected bursts fill every wave's 64 parked records once; 327 680 bursts, about 80 per wave, 95 %
    of them detected: every wave flushes in the loop and again at the end, the pool is on.  The same size with half the slots
    noise-only: about 40 detections per wave, no wave reaches the boundary -- miss records and parked records alternate and
    everything is flushed at the end.  655 360 bursts with half the slots noise-only: about 80 detections per wave again, the
    waves reach the boundary at different bursts, between miss records"""
    d_iq, params, _ = synth.make_normal_bursts(n, DEV, 4, seed=9300 + int(10 * p_noise), p_noise=p_noise, p_clip=0.0)
    res_a, _, _, _ = check(trx, d_iq, params)
    found = trx.results_to_numpy(res_a)["rc"] > 0
    assert abs(found.mean() - (1.0 - p_noise)) < 0.1


# ---- 3. pool on and off at the threshold -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold_batch():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n0 = 128 * n_cu
    d_iq, params, _ = synth.make_normal_bursts(n0 + 17, DEV, 4, seed=9400)
    return n0, d_iq, params


@pytest.mark.parametrize("extra", [-1, 0, 1, 15, 17])
def test_pool_on_and_off_at_the_threshold(trx, threshold_batch, extra):
    """the pool is given to launches of 128 * n_cu bursts and more: the sizes on either side, and ragged last groups behind it"""
    n0, d_iq, params = threshold_batch
    n = n0 + extra
    check(trx, d_iq[:n], params[:n])


# ---- 4. two launches back to back ---------------------------------------------------------------------------------------
def test_two_launches_into_the_same_buffers(trx, kinds_pool):
    """different batches, one stream, the same output buffers, no synchronisation between them: deferred stores and parked
    records are flushed per launch, nothing of the first launch is in the second one's output"""
    n = kinds_pool[0]
    rng = np.random.default_rng(9500)
    first = mixed_batch(kinds_pool, rng.integers(0, len(KINDS), n))
    second = mixed_batch(kinds_pool, rng.permutation(np.arange(n) % len(KINDS)))
    trx.set_nb_kernel(False)
    ref_res, ref_soft = trx.detect_demod(second[0], trx.params_tensor(second[1]), sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    results = torch.full((n, 32), 0xa5, dtype=torch.uint8, device=DEV)
    soft = torch.full((n, 148), -7.0, dtype=torch.float32, device=DEV)
    p1, p2 = trx.params_tensor(first[1]), trx.params_tensor(second[1])
    trx.detect_demod(first[0], p1, sps=4, results=results, soft=soft)
    trx.detect_demod(second[0], p2, sps=4, results=results, soft=soft)
    torch.cuda.synchronize()
    assert_bytes(results, soft, ref_res, ref_soft)
    assert_oracle(trx, second[0], second[1], results, soft)
