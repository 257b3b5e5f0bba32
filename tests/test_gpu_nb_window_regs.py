"""The normal-burst kernel's detection window in registers (tools/gen_nb_asm.py, blocks DEC / CORR: accumulators that move
across the lanes for windows of up to 45 lags, lane = sample / lag with the samples through LDS for wider ones): the split path
against the general kernel alone (trxhip_set_nb_kernel(ctx, 0)), results and soft bits BYTE-identical -- every window width
(both forms, the boundary max_toa 29 / 30 included), all eight training sequences, batch sizes with a ragged last group,
inputs on which the addition-only correlation's guard fails on every burst (the multiplying form), peaks at the first and at
the last lag of the window -- and rc / TSC / TOA equal to the oracle on the same inputs."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from osmo_trx_amd import TrxHip, synth

pytestmark = pytest.mark.gpu

N_ORACLE = 1024                 # bursts per case that also go through the CPU oracle


@pytest.fixture(scope="module")
def trx():
    t = TrxHip(0)
    yield t
    t.close()


def split_and_general(trx, iq, params):
    d_iq, d_p = iq.to("cuda:0"), trx.params_tensor(params)
    trx.set_nb_kernel(True)
    res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(False)
    res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    return res_a, soft_a, res_b, soft_b


def check(trx, iq, params, n_oracle=N_ORACLE):
    res_a, soft_a, res_b, soft_b = split_and_general(trx, iq, params)
    rows = np.flatnonzero((res_a != res_b).any(dim=1).cpu().numpy())
    assert torch.equal(res_a, res_b), (len(rows), rows[:8], trx.results_to_numpy(res_a)[rows[:4]], trx.results_to_numpy(res_b)[rows[:4]])
    assert torch.equal(soft_a.view(torch.int32), soft_b.view(torch.int32)), \
        np.flatnonzero((soft_a != soft_b).any(dim=1).cpu().numpy())[:8]
    g = trx.results_to_numpy(res_a)
    n = min(n_oracle, len(params))
    o_res, _ = O.pull_batch(iq[:n].cpu().numpy(), 4, params[:n])
    for k in ("rc", "tsc", "toa"):
        bad = np.flatnonzero(g[k][:n] != o_res[k])
        assert bad.size == 0, (k, bad[:8], g[k][:n][bad[:8]], o_res[k][bad[:8]])
    return g


@pytest.mark.parametrize("max_toa", list(range(33)))
def test_every_window_width(trx, max_toa):
    """1003 bursts: 62 full groups of 16 and a ragged one; burst i uses training sequence i % 8; delays across the window"""
    iq, params, _ = synth.make_normal_bursts(1003, "cpu", 4, seed=4000 + max_toa, max_toa=max_toa,
                                             delay_sym=(0.0, float(max(max_toa, 1))))
    g = check(trx, iq, params)
    assert (g["rc"] > 0).mean() > 0.85
    assert set(np.unique(g["tsc"][g["rc"] > 0])) == set(range(8))


@pytest.mark.parametrize("n", [1, 15, 17, 33, 1000, 4099])
@pytest.mark.parametrize("max_toa", [3, 29, 30])
def test_ragged_batches(trx, n, max_toa):
    iq, params, _ = synth.make_normal_bursts(n, "cpu", 4, seed=5000 + 40 * max_toa + n, max_toa=max_toa,
                                             delay_sym=(0.0, float(max_toa)))
    check(trx, iq, params, n_oracle=min(n, 64))


@pytest.mark.parametrize("max_toa", [0, 3, 29, 30, 32])
@pytest.mark.parametrize("component", [0, 1])
def test_guard_fails_on_every_burst(trx, max_toa, component):
    """real-only / imaginary-only bursts: every decimated sample has a zero component, the guard fails, the multiplying form runs
    (half the signal is missing: the reference finds no burst in most of them, and the kernels must say the same)"""
    iq, params, _ = synth.make_normal_bursts(2051, "cpu", 4, seed=6000 + 2 * max_toa + component, max_toa=max_toa,
                                             delay_sym=(0.0, float(max(max_toa, 1))), p_noise=0.0, p_clip=0.0)
    iq = iq.clone()
    iq[:, :, 1 - component] = 0
    check(trx, iq, params)


@pytest.mark.parametrize("max_toa", [0, 3, 17, 29, 30, 32])
@pytest.mark.parametrize("edge", ["first", "last"])
def test_peak_at_the_ends_of_the_window(trx, max_toa, edge):
    """the window of a normal burst starts ten symbols in front of the expected peak (head 10, sigProcLib.cpp:1887-1904): delays
    within four symbols of -10 put the correlation's maximum on the first lags, delays around max_toa + 5 on the last ones (the arg-max
    lane at both ends of its range; detectBurst's edge gate then rejects what sits on the outermost three lags)"""
    length = 16 + max_toa
    centre = -10.0 if edge == "first" else float(length - 1 - 10)
    iq, params, _ = synth.make_normal_bursts(2005, "cpu", 4, seed=7000 + 2 * max_toa + (edge == "last"), max_toa=max_toa,
                                             delay_sym=(centre - 4.0, centre + 4.0), p_noise=0.0, p_clip=0.0,
                                             snr_range=(20.0, 30.0))
    g = check(trx, iq, params)
    found = g["rc"] > 0
    assert found.any() and not found.all()                       # both sides of the edge gate are in the batch
