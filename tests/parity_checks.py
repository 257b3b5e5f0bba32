"""What the GPU parity tests share: the launch helper and the comparisons against the oracle, with the bars of
include/trxhip.h (read from there) and of tests/test_gpu_parity.py's module docstring."""
import numpy as np

import oracle_lib as O


def _torch():
    import torch
    return torch


def run_gpu(trx, iq, params, sps, soft_stride=148, slice_bits=True, exact=True, **kw):
    d_iq = iq.to("cuda:0") if not iq.is_cuda else iq
    d_p = trx.params_tensor(params)
    res, soft = trx.detect_demod(d_iq, d_p, sps=sps, soft_stride=soft_stride, slice_bits=slice_bits, exact=exact, **kw)
    _torch().cuda.synchronize()
    return trx.results_to_numpy(res), soft.cpu().numpy()


header_constant = O.header_constant
fast_ci_bar = O.fast_ci_bar
FAST_AMP_RTOL = header_constant("TRXHIP_FAST_AMP_RTOL")                 # fused kernels: amp against the reference's


FUSED_SOFT_ATOL = header_constant("TRXHIP_FUSED_SOFT_ATOL")             # fused demodulator, GMSK soft bits (full scale 1)
FUSED_SOFT_ATOL_8PSK = header_constant("TRXHIP_FUSED_SOFT_ATOL_8PSK")   # 8-PSK rows and the fuzz inputs


def assert_same_detection(r, rx):
    """Result records of the fused kernel (FAST detector) against the bit-exact kernel's (or the oracle's): rc, TSC, flags,
    TOA, energy and RSSI bit for bit; amp and C/I inside the bars of include/trxhip.h."""
    for f in ("rc", "tsc", "clip", "idle", "nbits_div4"):
        assert np.array_equal(r[f], rx[f]), f
    for f in ("toa", "energy", "rssi"):
        assert np.array_equal(r[f], rx[f], equal_nan=True), f
    aref = np.hypot(rx["amp_re"], rx["amp_im"])
    assert (np.hypot(r["amp_re"] - rx["amp_re"], r["amp_im"] - rx["amp_im"]) <= FAST_AMP_RTOL * aref).all()
    O.assert_fast_ci(r["ci"], rx["ci"])


def check_parity(g_res, g_soft, o_res, o_soft, soft_atol=0.0, sliced=None):
    """GPU against oracle.  soft_atol = 0: everything bit-identical (exact demodulator).  Otherwise the fused
    demodulator's statement of include/trxhip.h, both clauses: |soft - ref| <= soft_atol * max(1, rms / (4 |amp|)) with
    rms = sqrt(energy) and amp the amplitude estimate -- the plain bar on every real detection, amplitude-aware on noise
    slots detected far below their samples' level -- and identical hard decisions wherever the reference is not within
    10 bars of the decision threshold."""
    for f in ("rc", "tsc", "clip", "idle", "nbits_div4"):
        assert np.array_equal(g_res[f], o_res[f]), f
    assert np.array_equal(g_res["toa"], o_res["toa"])                   # TOA: identical in both kernels
    if soft_atol == 0.0:
        for f in ("amp_re", "amp_im"):
            assert np.array_equal(g_res[f], o_res[f]), f
    else:
        # fused kernels' FAST detector: the interpolated peak is an FMA sum (include/trxhip.h, TRXHIP_FAST_AMP_RTOL)
        aref = np.hypot(o_res["amp_re"], o_res["amp_im"])
        d = np.hypot(g_res["amp_re"] - o_res["amp_re"], g_res["amp_im"] - o_res["amp_im"])
        assert (d <= FAST_AMP_RTOL * aref).all(), float((d / np.maximum(aref, 1e-30)).max())
    if soft_atol == 0.0:
        assert np.array_equal(g_soft, o_soft)
    else:
        amp = np.hypot(o_res["amp_re"], o_res["amp_im"])
        ratio = np.ones_like(amp)
        np.divide(np.sqrt(np.maximum(o_res["energy"], 0)), amp, out=ratio, where=amp > 0)
        bar = (soft_atol * np.maximum(1.0, ratio / 4.0))[:, None]
        err = np.abs(g_soft - o_soft)
        assert (err <= bar).all(), float((err / bar).max())
        if sliced is None:                                               # (a caller that checks row subsets says which rows it has)
            sliced = o_soft.min() >= 0
        ref_mid = 0.5 if sliced else 0.0
        sure = np.abs(o_soft - ref_mid) > 10 * bar
        assert np.array_equal((g_soft > ref_mid)[sure], (o_soft > ref_mid)[sure])      # same hard decisions
    np.testing.assert_allclose(g_res["energy"], o_res["energy"], rtol=3e-6, atol=0)       # 80-term tree sum vs serial sum
    fin = np.isfinite(o_res["rssi"])
    np.testing.assert_allclose(g_res["rssi"][fin], o_res["rssi"][fin], rtol=0, atol=2e-5)
    assert np.array_equal(np.isfinite(g_res["rssi"]), fin)
    if soft_atol:
        nan = np.isnan(o_res["ci"])                                      # (S < C on a noise slot: log of a negative number, both sides)
        assert np.array_equal(np.isnan(g_res["ci"]), nan)
        assert (np.abs(g_res["ci"] - o_res["ci"])[~nan] <= fast_ci_bar(o_res["ci"][~nan])).all()
    else:
        np.testing.assert_allclose(g_res["ci"], o_res["ci"], rtol=0, atol=2e-5)
