"""The normal-burst kernel's sinc LUT as row pairs (csrc/trx_kernel_nb.hip, trx_tables.h trx_sincp_idx; block DETB of
tools/gen_nb_asm.py reads the weights of two taps as one 8-byte entry): 8192 normal bursts at 4 SPS over all eight TSCs whose
TOA searches address every column slot of the table that round B of the bisection can reach, from both sides of the peak (496
of the 512 fractions; every odd one as a final position -- see the first test), and whose peaks sit at the first and the last
admissible lag of the windows of max_toa 0, 3 and 32.  The default path against the general kernel alone as bytes, both
against the oracle (decisions identical, soft bits within the header's bar), and the re-run of the TOA search in the
reference's operand order (the cold reader of the new layout) must have run."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from osmo_trx_amd import TrxHip, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FUSED_SOFT_ATOL = O.header_constant("TRXHIP_FUSED_SOFT_ATOL")
N_COVER = 6656                  # bursts 0 .. N_COVER - 1: max_toa 3, delays 0 .. 4 symbols (every fraction the search can reach)
N_EDGE = 256                    # per window edge: 3 windows x {first, last admissible lag}
EDGE_MAX_TOA = (0, 3, 32)
HEAD = 10                       # detectGeneralBurst's head (sigProcLib.cpp:1887-1904): TOA 0 is lag HEAD + sync->toa of the window


@pytest.fixture(scope="module")
def trx():
    t = TrxHip(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def batch():
    """(iq int16[8192, 625, 2] on the CPU, params).  An edge burst's delay puts its correlation peak within a symbol of lag 3
    (TOA 3 - HEAD = -7) or of lag len - 3 = 13 + max_toa (TOA 3 + max_toa): the edge gate passes 3 <= lag <= len - 3 (:1683)"""
    kw = dict(p_noise=0.0, p_clip=0.0, snr_range=(12.0, 30.0))
    iqs, prms = [], []
    iq, p, _ = synth.make_normal_bursts(N_COVER, "cpu", 4, seed=15001, max_toa=3, delay_sym=(0.0, 4.0))
    iqs.append(iq)
    prms.append(p)
    for k, mt in enumerate(EDGE_MAX_TOA):
        for side, centre in enumerate((3.0 - HEAD, 3.0 + mt)):
            iq, p, _ = synth.make_normal_bursts(N_EDGE, "cpu", 4, seed=15100 + 2 * k + side, max_toa=mt,
                                                delay_sym=(centre - 0.9, centre + 0.9), **kw)
            iqs.append(iq)
            prms.append(p)
    iq, params = torch.cat(iqs), np.concatenate(prms)
    assert len(params) == 8192 and set(params["tsc"]) == set(range(8))
    return iq, params


@pytest.fixture(scope="module")
def runs(trx, batch):
    """default path (with the re-run counter of the covering part alone), general kernel alone, oracle: computed once"""
    iq, params = batch
    d_iq, d_p = iq.to(DEV), trx.params_tensor(params)
    trx.set_nb_kernel(True)
    trx.fast_stats(reset=True)
    trx.detect_demod(d_iq[:N_COVER], d_p[:N_COVER], sps=4)
    stats = trx.fast_stats(reset=True)
    res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(False)
    res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    o_res, o_soft = O.pull_batch(iq.numpy(), 4, params)
    return dict(res_a=res_a, soft_a=soft_a, res_b=res_b, soft_b=soft_b, o_res=o_res, o_soft=o_soft, stats=stats)


def positions512(r, params):
    """final position of the TOA search in 1/512 symbol, of the detected bursts: toa = position - sync->toa - head (:1704, :1768),
    exact in 1/512 (the kernels compute it as an integer)"""
    t5 = np.array([int(O.tables()["midamble"][t]["toa"] * 512.0) for t in range(8)])
    det = r["rc"] > 0
    t512 = r["toa"].astype(np.float64) * 512.0
    assert (t512[det] == np.round(t512[det])).all()
    return det, t512.astype(np.int64) + t5[params["tsc"]] + HEAD * 512


def node_offset(n, inc0):
    """trx_device.h node_offset(): earlyIndex offset of heap node n of a bisection subtree whose first step is inc0"""
    lv = (n + 1).bit_length() - 1
    p = n + 1 - (1 << lv)
    return ((4 * p * inc0) >> lv) - (2 * inc0 - ((2 * inc0) >> lv))


# round B's positions by lane, relative to earlyIndex * 512 (trx_device.h peak_const(): offB): lanes 0..29 the early / late
# positions of the 15 nodes of levels 5..8, lanes 32..47 the sixteen possible final positions
OFF_B = [node_offset(l >> 1, 8) + (1024 if l & 1 else 0) for l in range(30)] + [2 * k - 15 + 512 for k in range(16)]


def test_every_fraction_round_b_can_address_occurs(trx, batch, runs):
    """What peakDetect()'s bisection (:1141-1186) can reach: round A leaves earlyIndex at 16 mod 32 (in 1/512 symbol), round B's
    nodes add sums of +-8 +-4 +-2 (even, within +-14) and its final step is +-1, so a FINAL position is always odd -- 256
    fractions -- and the positions round B EVALUATES take every fraction that is no multiple of 32 -- 496 of the 512.  A multiple
    of 32, fraction 0 with its column slot 512 and the zero tail among them, is never addressed by round B on any input; those
    slots are read only by the re-run's tie exit (a tie can stop the search on any node) and are checked entry by entry in
    tests/test_nb_sinc_pairs_cpu.py.  Asserted on the general kernel's TOA: every odd fraction is a final position, and the lanes
    of round B together address all 496 fractions, at and below the peak (column f) and above it (column 512 - f)."""
    _, params = batch
    r = trx.results_to_numpy(runs["res_b"])                         # the general kernel's TOA
    det, pos = positions512(r, params)
    cover = det & (np.arange(len(params)) < N_COVER)
    final = pos[cover]
    f = final & 511
    print("detected bursts of the covering part:", int(cover.sum()), "fewest per odd fraction:", int(np.bincount(f, minlength=512)[1::2].min()))
    assert set(f.tolist()) == set(range(1, 512, 2)), sorted(set(range(1, 512, 2)) - set(f.tolist()))[:8]
    # earlyIndex behind round A: final = E + 512 + (2 p - 15) with E = 16 mod 32, so the last step is (final mod 32) - 16
    early = final - 512 - ((final & 31) - 16)
    assert ((early & 31) == 16).all()
    lanes = (early[:, None] + np.array(OFF_B)[None, :]) & 511
    reachable = {q for q in range(512) if q % 32}
    lo = set(lanes.ravel().tolist())                                # taps at and below the peak: column slot swz(f)
    hi = set((512 - lanes).ravel().tolist())                        # taps above it: column 512 - f
    assert lo == reachable, (sorted(reachable - lo)[:8], sorted(lo - reachable)[:8])
    assert hi == {512 - q for q in reachable}


def test_peaks_at_the_first_and_last_admissible_lag(trx, batch, runs):
    _, params = batch
    r = trx.results_to_numpy(runs["res_b"])
    det, pos = positions512(r, params)
    first = N_COVER
    for mt in EDGE_MAX_TOA:
        length = 16 + mt
        for side in range(2):
            rows = np.arange(first, first + N_EDGE)
            first += N_EDGE
            assert (params["max_toa"][rows] == mt).all()
            p = pos[rows][det[rows]]
            # a position below lag 3 belongs to a peak AT lag 3 (the search stays within a symbol of the peak, and the gate refuses
            # lag 2), one above lag len - 3 to a peak at lag len - 3
            at_edge = (p < 3 * 512) if side == 0 else (p > (length - 3) * 512)
            print("max_toa", mt, "side", side, "detected", int(det[rows].sum()), "at the edge lag", int(at_edge.sum()),
                  "refused", int((~det[rows]).sum()))
            assert at_edge.sum() >= 8, (mt, side, int(at_edge.sum()))
            assert (~det[rows]).sum() >= 8, (mt, side)             # and the gate's other side is in the batch, too


def test_default_path_is_the_general_kernel_byte_for_byte(runs):
    res_a, soft_a, res_b, soft_b = runs["res_a"], runs["soft_a"], runs["res_b"], runs["soft_b"]
    bad = np.flatnonzero((res_a != res_b).any(dim=1).cpu().numpy())
    assert torch.equal(res_a, res_b), (len(bad), bad[:8])
    assert torch.equal(soft_a.view(torch.int32), soft_b.view(torch.int32)), \
        np.flatnonzero((soft_a != soft_b).any(dim=1).cpu().numpy())[:8]


def test_against_the_oracle(trx, runs):
    o_res, o_soft = runs["o_res"], runs["o_soft"]
    g = trx.results_to_numpy(runs["res_a"])
    for k in ("rc", "tsc", "toa"):
        bad = np.flatnonzero(g[k] != o_res[k])
        assert bad.size == 0, (k, bad[:8], g[k][bad[:8]], o_res[k][bad[:8]])
    # the fused demodulator's statement of include/trxhip.h: |soft - ref| <= TRXHIP_FUSED_SOFT_ATOL * max(1, rms / (4 |amp|))
    amp = np.hypot(o_res["amp_re"], o_res["amp_im"])
    ratio = np.where(amp > 0, np.sqrt(np.maximum(o_res["energy"], 0)) / np.maximum(amp, 1e-30), 1.0)
    bar = (FUSED_SOFT_ATOL * np.maximum(1.0, ratio / 4.0))[:, None]
    err = np.abs(runs["soft_a"].cpu().numpy() - o_soft)
    print("largest soft-bit error against the oracle, in bars:", float((err / bar).max()))
    assert (err <= bar).all(), float((err / bar).max())


def test_the_rerun_over_the_new_layout_ran(runs):
    """bursts with an uncertified early / late decision take the TOA search again in the reference's operand order, reading
    the row pairs through trx_sincp_idx (peak_detect_spec<true>): about one detected burst in 200.  The covering part is all
    within the kernel's geometry, so what it leaves to the general kernel (which counts its own re-runs) is next to nothing."""
    st = runs["stats"]
    print(st)
    left = st["left_guard"] + st["left_gate"] + st["left_geometry"]
    assert st["reruns"] > left, st
    assert st["reruns"] >= 4, st
