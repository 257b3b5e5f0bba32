"""The rare sides of the normal-burst kernel's blocks (csrc/trx_kernel_nb.hip, tools/gen_nb_asm.py) lie out of the main path's
instruction stream -- in the shadow of block CORR's computed jump, or in a statement behind the burst loop -- and are entered
from and left for labels inside the blocks.  Here every one of them is entered and left between two ordinary bursts of the same
wave: the kinds below are drawn i.i.d. in one batch of 20 000 bursts (about five per wave, 256 workgroups of sixteen waves), so
every ordered pair of kinds occurs in some wave's sequence whatever the hardware's assignment.  The result is compared byte for
byte, every burst, with the general kernel alone (set_nb_kernel(False)); detected bursts also with the oracle, within the
header's bar.

  window      max_toa 0, 3, 29 (moving forms of DEC / CORR), 30, 32 (NB_ASM_CORR_MAX_LEN = 45 lags: the wide forms)
  zero_q      the quadrature component of samples 220 .. 243 is zero, so that of decimated sample 60 (taps on samples 225 .. 240),
              inside every window, is exactly zero: the addition-only correlation's guard fails and CORR takes the multiplying
              form (narrow and wide window)
  edge        the burst lies so early / late that the correlation's peak is within three lags of the window's edge (DETA's edge exit)
  noise       noise-only slots (the peak-ratio gate's miss)
  early, late TOA outside the straight-line demodulator's geometry (TAIL's exit, the general form of the demodulator)
  foreign     a slot of another type;  clipped: maxAmplitude() above the threshold
The exact re-run of the TOA search (DETA's / DETB's careful walk ending unsure: about 0.5 % of detections) and the general
demodulator are counted by the kernel (fast_stats); the other exits follow from how the inputs are made.  The gate's
too-close-to-call exit occurs about once in 1e5 bursts and is not asserted.
The oracle is a CPU program: it takes the batch's first N_ORACLE = 2048 bursts (1024 of the flush case), which keeps the test at a
few seconds.  The kinds are drawn i.i.d., so that prefix holds about 146 bursts of every kind; all 20 000 bursts are held to
the general kernel's bytes, and the general kernel to the oracle by tests/test_gpu_parity.py."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from osmo_trx_amd import TrxHip, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 20000
N_ORACLE = 2048                 # bursts of the batch that also go through the CPU oracle
FILL = 0xa5
FUSED_SOFT_ATOL = O.header_constant("TRXHIP_FUSED_SOFT_ATOL")
QUIET = dict(p_noise=0.0, p_clip=0.0)
LOUD = dict(snr_range=(15.0, 30.0), **QUIET)
KINDS = {
    "toa0": dict(max_toa=0, delay_sym=(0.0, 2.0), **QUIET),
    "toa3": dict(max_toa=3, delay_sym=(0.0, 3.0), **QUIET),
    "toa29": dict(max_toa=29, delay_sym=(0.0, 4.0), **QUIET),
    "toa30": dict(max_toa=30, delay_sym=(0.0, 4.0), **QUIET),
    "toa32": dict(max_toa=32, delay_sym=(0.0, 4.0), **QUIET),
    "zero_q": dict(max_toa=3, delay_sym=(0.0, 3.0), **LOUD),
    "zero_q_wide": dict(max_toa=32, delay_sym=(0.0, 4.0), **LOUD),
    "edge_lo": dict(max_toa=3, delay_sym=(-10.0, -7.6), **LOUD),      # peak at lag 10 + delay: below 3
    "edge_hi": dict(max_toa=3, delay_sym=(6.6, 8.4), **LOUD),        # above len - 3 = 16
    "noise": dict(max_toa=3, p_noise=1.0, p_clip=0.0),
    "early": dict(max_toa=5, delay_sym=(-3.0, -1.0), **LOUD),
    "late": dict(max_toa=20, delay_sym=(10.5, 18.0), **LOUD),
    "foreign": dict(max_toa=3, **QUIET),
    "clipped": dict(max_toa=3, p_noise=0.0, p_clip=1.0),
}
NAMES = tuple(KINDS)
ZERO_Q = slice(220, 244)        # decimated sample 60 = sum of 16 taps on samples 225 .. 240: window samples are 56 .. 70 + len


@pytest.fixture(scope="module")
def trx():
    t = TrxHip(0)
    yield t
    t.close()


def split_and_general(trx, d_iq, params):
    d_p = trx.params_tensor(params)
    trx.set_nb_kernel(True)
    trx.fast_stats(reset=True)
    res_a = torch.full((len(params), 32), FILL, dtype=torch.uint8, device=DEV)
    res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4, results=res_a)
    torch.cuda.synchronize()
    stats = trx.fast_stats(reset=True)
    trx.set_nb_kernel(False)
    res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    return res_a, soft_a, res_b, soft_b, stats


def assert_bytes(res_a, soft_a, res_b, soft_b):
    """every burst: records as bytes, soft bits as bytes"""
    bad = np.flatnonzero((res_a != res_b).any(dim=1).cpu().numpy())
    assert torch.equal(res_a, res_b), (len(bad), bad[:8])
    assert torch.equal(soft_a.view(torch.int32), soft_b.view(torch.int32)), \
        np.flatnonzero((soft_a != soft_b).any(dim=1).cpu().numpy())[:8]


def assert_oracle(trx, d_iq, params, res, soft, n=N_ORACLE):
    """the first n bursts: decisions identical to the oracle's; the detected ones' soft bits within the header's bar
    (include/trxhip.h: |soft - ref| <= TRXHIP_FUSED_SOFT_ATOL * max(1, rms / (4 |amp|)))"""
    n = min(n, len(params))
    g = trx.results_to_numpy(res[:n])
    o_res, o_soft = O.pull_batch(d_iq[:n].cpu().numpy(), 4, params[:n])
    for k in ("rc", "tsc", "toa"):
        bad = np.flatnonzero(g[k] != o_res[k])
        assert bad.size == 0, (k, bad[:8], g[k][bad[:8]], o_res[k][bad[:8]])
    det = o_res["rc"] > 0
    amp = np.hypot(o_res["amp_re"], o_res["amp_im"])
    ratio = np.where(amp > 0, np.sqrt(np.maximum(o_res["energy"], 0)) / np.maximum(amp, 1e-30), 1.0)
    bar = (FUSED_SOFT_ATOL * np.maximum(1.0, ratio / 4.0))[:, None]
    err = np.abs(soft[:n].cpu().numpy() - o_soft)
    print("detected:", int(det.sum()), "of", n, "-- largest soft-bit error against the oracle, in bars:", float((err / bar)[det].max()))
    assert (err <= bar)[det].all(), float((err / bar)[det].max())


@pytest.fixture(scope="module")
def batch():
    """the kinds drawn i.i.d.; each kind's bursts are generated once, as many as the draw took of it"""
    kinds = np.random.default_rng(9700).integers(0, len(NAMES), N)
    d_iq = torch.empty((N, 625, 2), dtype=torch.int16, device=DEV)
    params = None
    for k, name in enumerate(NAMES):
        rows = np.flatnonzero(kinds == k)
        assert rows.size > 1000
        iq, p, _ = synth.make_normal_bursts(rows.size, DEV, 4, seed=9710 + k, **KINDS[name])
        if name.startswith("zero_q"):
            iq[:, ZERO_Q, 1] = 0
        if name == "foreign":
            p["type"] = O.EDGE
        if params is None:
            params = np.zeros(N, dtype=p.dtype)
        d_iq[torch.from_numpy(rows).to(DEV)] = iq
        params[rows] = p
    return kinds, d_iq, params


def test_every_cold_exit_between_ordinary_bursts(trx, batch):
    kinds, d_iq, params = batch
    res_a, soft_a, res_b, soft_b, stats = split_and_general(trx, d_iq, params)
    assert_bytes(res_a, soft_a, res_b, soft_b)
    assert_oracle(trx, d_iq, params, res_a, soft_a)
    r = trx.results_to_numpy(res_a)
    of = {name: kinds == k for k, name in enumerate(NAMES)}
    found = r["rc"] > 0
    print("fast_stats:", stats, {name: float(found[of[name]].mean()) for name in NAMES})
    # ---- counted by the kernel: the exact re-run (a careful walk that ends unsure), the general demodulator (TAIL's exit)
    assert stats["reruns"] > 0, stats
    assert stats["left_geometry"] > 0, stats
    # ---- by construction: the windows on either side of the change of form are detected
    for name in ("toa0", "toa3", "toa29", "toa30", "toa32"):
        assert found[of[name]].mean() > 0.9, name
    assert set(np.unique(params["max_toa"])) >= {0, 3, 29, 30, 32}
    # the multiplying form: a decimated sample of the window has a component that is exactly zero
    for name in ("zero_q", "zero_q_wide"):
        assert (d_iq[torch.from_numpy(np.flatnonzero(of[name])).to(DEV)][:, ZERO_Q, 1] == 0).all()
    # the edge exit and the gate's miss: no burst is found
    for name in ("edge_lo", "edge_hi", "noise"):
        assert (r["rc"][of[name]] == 0).mean() > 0.9, name
    # the general form of the demodulator, both sides of the geometry
    assert (r["toa"][of["early"] & found] < -0.5).sum() > 100
    assert (r["toa"][of["late"] & found] > 9.5).sum() > 100
    assert (r["clip"][of["clipped"]] == 1).mean() > 0.9
    # a slot of another type: the second launch's record is there
    assert not (res_a.cpu().numpy()[of["foreign"]] == FILL).all(axis=1).any()


def test_cold_exits_with_the_record_flush_inside_the_loop(trx):
    """327 680 bursts, about 80 per wave, 95 % of them detected: every wave's 64 parked records are flushed inside the loop (and
    the rest at its end) among early bursts, misses and re-runs -- the flush is one more path that joins the loop's end"""
    n = 327680
    d_iq, params, _ = synth.make_normal_bursts(n, DEV, 4, seed=9750, delay_sym=(-1.0, 4.0), max_toa=5, p_noise=0.03, p_clip=0.0)
    res_a, soft_a, res_b, soft_b, stats = split_and_general(trx, d_iq, params)
    assert_bytes(res_a, soft_a, res_b, soft_b)
    assert_oracle(trx, d_iq, params, res_a, soft_a, 1024)
    found = trx.results_to_numpy(res_a)["rc"] > 0
    print("fast_stats:", stats, float(found.mean()))
    assert found.mean() > 0.85
    assert stats["left_geometry"] > 0 and stats["reruns"] > 0, stats
