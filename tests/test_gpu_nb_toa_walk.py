"""The normal-burst kernel's TOA search on its position-ordered lane layout (tools/gen_nb_asm.py: walk_rank; DETA / DETB find the
leaf of a certified, monotone round as a first zero and walk every other mask level by level in NB_ASM_COLD): two batches of
4 SPS, 625-sample normal bursts over all eight TSCs, the default path against the general kernel alone as bytes; batch 1 against
the oracle within the bars of tests/parity_checks.py, batch 2's decisions against the oracle's (test_against_the_oracle says why).

Batch 1 (threshold 4, 11 264 bursts):
  * 4096 bursts whose delay sweeps 0 .. 4 symbols: every odd fraction is a final position;
  * 2048 bursts through two rays a fraction of a symbol to 1.5 symbols apart with comparable amplitude: rounds whose certified
    decisions are NOT monotone in position -- the level-by-level walk that ends certified;
  * 4096 noise-only slots: a few pass the gates at the threshold, most do not;
  * 512 bursts each with max_toa 0 and 32 (batch 1's other bursts have max_toa 3).
Batch 2 (threshold 2, 4096 bursts): two rays of nearly equal amplitude about two symbols apart.  Under the default threshold the
peak-ratio gate refuses them (a second peak is one of its eight terms); under this one they reach what no single ray does: the
search ends a whole symbol from the arg-max lag, at round A's outermost leaves.

What a round did is counted by a host-side float64 model of the search (tests/nb_toa_walk_model.py) -- the kernel has no
counter for a level-by-level walk that ends certified (g_trx_fast_stats counts the ones that end unsure).  That the model IS the
kernels' search is asserted first: it gives the TOA the kernels report for every detected burst whose decisions clear twice the
certification margin in both rounds.  With that: all 32 leaves of round A and all 16 of round B are reached; a single ray stays
within half a symbol of its arg-max lag (leaves 8 .. 23 at least); and in both batches rounds that are certified by that
margin and not monotone occur at least eight times (found on the recorded seeds: batch 1 some tens, batch 2 hundreds)."""
import numpy as np
import pytest
import torch

import nb_toa_walk_model as M
import oracle_lib as O
import parity_checks as P
from osmo_trx_amd import TrxHip, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KAPPA = 6e-6                                                            # TRX_FAST_KAPPA (csrc/trx_device.h)
N_SWEEP, N_RAYS, N_NOISE, N_EDGE, N_FAR = 4096, 2048, 4096, 512, 4096
THRESHOLDS = (4.0, 2.0)


@pytest.fixture(scope="module")
def trx():
    t = TrxHip(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def batches():
    """[(iq int16[n, 625, 2] on the CPU, params, threshold)] and the row ranges of batch 1's parts"""
    kw = dict(p_noise=0.0, p_clip=0.0)
    parts = [synth.make_normal_bursts(N_SWEEP, "cpu", 4, seed=17001, max_toa=3, delay_sym=(0.0, 4.0), **kw)[:2],
             M.make_two_ray_bursts(N_RAYS, 17002, gap_sym=(0.3, 1.5), rel_amp=(0.6, 1.5)),
             synth.make_normal_bursts(N_NOISE, "cpu", 4, seed=17003, max_toa=3, p_noise=1.0, p_clip=0.0)[:2],
             synth.make_normal_bursts(N_EDGE, "cpu", 4, seed=17004, max_toa=0, delay_sym=(-0.4, 0.4), **kw)[:2],
             synth.make_normal_bursts(N_EDGE, "cpu", 4, seed=17005, max_toa=32, delay_sym=(0.0, 31.0), **kw)[:2]]
    iq1, p1 = torch.cat([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    edges = np.cumsum([0] + [len(b) for _, b in parts])
    rows = {k: slice(edges[i], edges[i + 1]) for i, k in enumerate(("sweep", "rays", "noise", "toa0", "toa32"))}
    iq2, p2 = M.make_two_ray_bursts(N_FAR, 17006, gap_sym=(1.6, 2.4), rel_amp=(0.95, 1.05))
    assert set(p1["tsc"]) == set(p2["tsc"]) == set(range(8)) and set(p1["max_toa"]) == {0, 3, 32}
    return [(iq1, p1, THRESHOLDS[0]), (iq2, p2, THRESHOLDS[1])], rows


@pytest.fixture(scope="module")
def runs(trx, batches):
    """per batch: default path, general kernel alone, oracle, the model -- computed once"""
    out = []
    for iq, params, thr in batches[0]:
        d_iq, d_p = iq.to(DEV), trx.params_tensor(params)
        trx.set_nb_kernel(True)
        res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4, threshold=thr)
        torch.cuda.synchronize()
        trx.set_nb_kernel(False)
        res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4, threshold=thr)
        torch.cuda.synchronize()
        trx.set_nb_kernel(True)
        o_res, o_soft = O.pull_batch(iq.numpy(), 4, params, threshold=thr)
        out.append(dict(res_a=res_a, soft_a=soft_a, res_b=res_b, soft_b=soft_b, o_res=o_res, o_soft=o_soft,
                        model=M.toa_search(iq.numpy(), params), params=params))
    return out


def test_default_path_is_the_general_kernel_byte_for_byte(runs):
    for r in runs:
        bad = np.flatnonzero((r["res_a"] != r["res_b"]).any(dim=1).cpu().numpy())
        assert torch.equal(r["res_a"], r["res_b"]), (len(bad), bad[:8])
        assert torch.equal(r["soft_a"].view(torch.int32), r["soft_b"].view(torch.int32)), \
            np.flatnonzero((r["soft_a"] != r["soft_b"]).any(dim=1).cpu().numpy())[:8]


def test_against_the_oracle(trx, runs):
    """Batch 1 -- the issue's cases -- through tests/parity_checks.py unchanged.  Batch 2 is NOT held to the oracle's bars: its
    peaks lie between two rays, below the arg-max magnitude, and there the FAST detector's amp leaves TRXHIP_FAST_AMP_RTOL
    (largest found 1.4e-6 of |amp| against 1e-6, in the general kernel and the normal-burst kernel alike -- a matter of
    include/trxhip.h, not of the walks).  Round A's outermost leaves, which only such bursts reach, are therefore covered by the
    byte comparison with the general kernel above, by the decisions below (rc, TSC, flags and TOA identical to the oracle's, as
    check_parity() asks), and by tests/test_nb_toa_walk_cpu.py."""
    r = runs[0]
    P.check_parity(trx.results_to_numpy(r["res_a"]), r["soft_a"].cpu().numpy(), r["o_res"], r["o_soft"], soft_atol=P.FUSED_SOFT_ATOL)
    g, o = trx.results_to_numpy(runs[1]["res_a"]), runs[1]["o_res"]
    for f in ("rc", "tsc", "clip", "idle", "nbits_div4", "toa"):
        assert np.array_equal(g[f], o[f]), f


def searched(trx, r):
    """(detected, certain, final position in 1/512 symbol as the kernel reports it)"""
    g = trx.results_to_numpy(r["res_a"])
    t5 = np.array([int(O.tables()["midamble"][t]["toa"] * 512.0) for t in range(8)])
    det = g["rc"] > 0
    t512 = g["toa"].astype(np.float64) * 512.0
    assert (t512[det] == np.round(t512[det])).all()
    m = r["model"]
    certain = (m["margin_a"] > 2 * KAPPA) & (m["margin_b"] > 2 * KAPPA)
    return det, certain, t512.astype(np.int64) + t5[r["params"]["tsc"]] + M.HEAD * 512


def test_the_model_is_the_kernels_search(trx, runs):
    for r in runs:
        det, certain, pos = searched(trx, r)
        same = pos == r["model"]["pos512"]
        print("detected", int(det.sum()), "of them certain", int((det & certain).sum()), "model's position differs on", int((det & ~same).sum()))
        assert (det & certain).sum() > 0.9 * det.sum()
        assert same[det & certain].all(), np.flatnonzero(det & certain & ~same)[:8]


def test_every_leaf_of_both_rounds_is_reached(trx, runs, batches):
    rows = batches[1]
    la, lb = set(), set()
    for r in runs:
        det, certain, _ = searched(trx, r)
        la |= set(r["model"]["leaf_a"][det & certain].tolist())
        lb |= set(r["model"]["leaf_b"][det & certain].tolist())
    assert la == set(range(32)), sorted(set(range(32)) - la)
    assert lb == set(range(16)), sorted(set(range(16)) - lb)
    # a single ray: the search ends within half a symbol of the arg-max lag, on every odd fraction
    r = runs[0]
    det, certain, pos = searched(trx, r)
    sw = np.zeros(len(det), bool)
    sw[rows["sweep"]] = True
    one = set(r["model"]["leaf_a"][sw & det & certain].tolist())
    print("round A's leaves of the sweep:", sorted(one))
    assert one >= set(range(8, 24)) and one <= set(range(6, 26)), sorted(one)
    assert set(r["model"]["leaf_b"][sw & det & certain].tolist()) == set(range(16))
    assert set((pos[sw & det] & 511).tolist()) == set(range(1, 512, 2))


def test_certified_rounds_that_are_not_monotone(trx, runs, batches):
    """the level-by-level walk that ends certified: in the two-ray parts, of both rounds"""
    rows = batches[1]
    for k, r in enumerate(runs):
        det, certain, _ = searched(trx, r)
        part = np.zeros(len(det), bool)
        part[rows["rays"] if k == 0 else slice(None)] = True
        na = int((part & det & certain & ~r["model"]["mono_a"]).sum())
        nb = int((part & det & certain & ~r["model"]["mono_b"]).sum())
        print("batch", k + 1, "two-ray bursts detected:", int((part & det).sum()), "certified and not monotone: round A", na, "round B", nb)
        assert na >= 8 and nb >= 8, (k, na, nb)


def test_noise_slots_and_windows(trx, runs, batches):
    rows = batches[1]
    det, _, _ = searched(trx, runs[0])
    print("noise slots detected:", int(det[rows["noise"]].sum()), "max_toa 0:", int(det[rows["toa0"]].sum()), "max_toa 32:", int(det[rows["toa32"]].sum()))
    assert 1 <= det[rows["noise"]].sum() < N_NOISE // 10                # at the threshold: a few pass
    assert det[rows["toa0"]].sum() >= N_EDGE // 2 and det[rows["toa32"]].sum() >= N_EDGE // 2
