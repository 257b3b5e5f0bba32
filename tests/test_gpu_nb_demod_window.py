"""The normal-burst kernel's demodulator with the filter window sliding across the lanes (tools/gen_nb_asm.py, block DEMOD /
fir_moving: every lane reads its own twelve samples, the three accumulators move two lanes up; the low-edge symbols on three
lanes each): the split path against the general kernel alone (trxhip_set_nb_kernel(ctx, 0)), results and soft bits
BYTE-identical, and within TRXHIP_FUSED_SOFT_ATOL of the oracle, over the whole straight-line geometry.

The geometry: nk = -512 * toa (the reported TOA, a multiple of 1/256 symbol: the bisection ends on even 1/512 steps), shift
w = nk >> 7 in 0 .. -36, fr = nk & 127, delay-filter row fr >> 1 for fr >= 2 and "no fractional delay" (row 64) for fr = 0.
Row 0 does not exist in either kernel (fr >> 1 = 0 only for fr < 2, which selects row 64), so a shift has 64 cells -- rows
1 .. 63 and "none" -- and the geometry 37 * 64 = 2368, each ONE TOA value wide.  The sweep is 65536 bursts with delays uniform
over the geometry and a margin on both sides: 27 bursts per cell on average, and the test asserts that every cell was hit by a
detected burst.  TOAs outside the geometry (earlier than -127/512, later than 9 symbols) must take the general form of the
demodulator inside the kernel (demod_general): counted by the kernel (fast_stats, left_geometry) and compared with the count of
such TOAs in the results."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from osmo_trx_amd import synth

MAX_TOA = 12                    # window of 28 lags: TOAs of -7 .. +14 symbols inside the edge gate
N_SWEEP = 65536
W_ALL = range(0, -37, -1)
ROW_NONE = 64
ROWS_ALL = list(range(1, 64)) + [ROW_NONE]
FUSED_SOFT_ATOL = O.header_constant("TRXHIP_FUSED_SOFT_ATOL")


def detected_only(iq, params):
    """the reference turns down about two in 10^4 of even clean bursts (the peak-ratio gate on the data's own sidelobes); the
    sweep is made of detections, so those are dropped where the inputs are made -> (iq, params, number dropped)"""
    o_res, _ = O.pull_batch(iq.numpy(), 4, params)
    keep = o_res["rc"] > 0
    return iq[torch.from_numpy(keep)].contiguous(), params[keep], int((~keep).sum())


def sweep():
    """delays over the geometry (-0.248 .. 9 symbols) and 0.06 symbol beyond on both sides (the estimate is within 0.05 of the delay)"""
    iq, params, _ = synth.make_normal_bursts(N_SWEEP, "cpu", 4, seed=11000, max_toa=MAX_TOA, delay_sym=(-0.31, 9.06), p_noise=0.0,
                                             p_clip=0.0, snr_range=(22.0, 35.0), amp_range=(1000.0, 16000.0))
    return detected_only(iq, params)


def outside(kind):
    rng = {"early": (-3.0, -0.32), "late": (9.07, 11.5)}[kind]
    iq, params, _ = synth.make_normal_bursts(4099, "cpu", 4, seed=11100 + (kind == "late"), max_toa=MAX_TOA, delay_sym=rng,
                                             p_noise=0.0, p_clip=0.0, snr_range=(22.0, 35.0), amp_range=(1000.0, 16000.0))
    return detected_only(iq, params)


def geometry(toa):
    """-> (nk, w, row, inside) of reported TOAs"""
    nk = -np.round(toa.astype(np.float64) * 512.0).astype(np.int64)
    assert np.array_equal((-nk / 512.0).astype(np.float32), toa)       # (exact in 1/512 symbol)
    w, fr = nk >> 7, nk & 127
    row = np.where(fr >= 2, fr >> 1, ROW_NONE)
    return nk, w, row, (w <= 0) & (w >= -36)


def cells_hit(res):
    det = res["rc"] > 0
    _, w, row, inside = geometry(res["toa"])
    return {(int(a), int(b)) for a, b in zip(w[det & inside], row[det & inside])}, int((det & ~inside).sum())


ALL_CELLS = {(w, r) for w in W_ALL for r in ROWS_ALL}


def test_sweep_inputs_on_the_oracle():
    """the input generator, without a GPU: the oracle alone detects every burst of the sweep, and the detected TOAs hit every
    (shift, row) cell of the geometry and both sides of each of its ends; the outside batches are detected and lie outside"""
    iq, params, dropped = sweep()
    assert dropped < N_SWEEP // 1000 and len(params) == N_SWEEP - dropped
    o_res, _ = O.pull_batch(iq.numpy(), 4, params)
    assert (o_res["rc"] > 0).all()
    hit, n_out = cells_hit(o_res)
    assert hit == ALL_CELLS, sorted(ALL_CELLS - hit)[:8]
    _, w, _, _ = geometry(o_res["toa"])
    assert (w > 0).sum() > 100 and (w < -36).sum() > 100 and n_out == (w > 0).sum() + (w < -36).sum()
    for kind in ("early", "late"):
        iq, params, dropped = outside(kind)
        assert dropped < 40 and len(params) > 4000
        o_res, _ = O.pull_batch(iq.numpy(), 4, params)
        assert (o_res["rc"] > 0).all()
        _, w, _, inside = geometry(o_res["toa"])
        # (a handful lock onto a sidelobe at the far end of the window: outside as well, on the other side)
        assert not inside.any() and ((w > 0) if kind == "early" else (w < -36)).mean() > 0.99


@pytest.fixture(scope="module")
def trx():
    from osmo_trx_amd import TrxHip
    t = TrxHip(0)
    yield t
    t.close()


def check(trx, iq, params):
    """split path == general kernel alone, byte for byte; both against the oracle -> (results, left_geometry, left_gate)"""
    d_iq, d_p = iq.to("cuda:0"), trx.params_tensor(params)
    trx.set_nb_kernel(True)
    trx.fast_stats(reset=True)
    res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    st = trx.fast_stats(reset=True)
    trx.set_nb_kernel(False)
    res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    rows = np.flatnonzero((res_a != res_b).any(dim=1).cpu().numpy())
    assert torch.equal(res_a, res_b), (len(rows), rows[:8])
    bad = np.flatnonzero((soft_a.view(torch.int32) != soft_b.view(torch.int32)).any(dim=1).cpu().numpy())
    g = trx.results_to_numpy(res_a)
    assert bad.size == 0, (bad.size, bad[:8], g["toa"][bad[:8]],
                           np.flatnonzero((soft_a[int(bad[0])] != soft_b[int(bad[0])]).cpu().numpy())[:16])
    # the oracle: decisions and TOA identical, soft bits inside the fused demodulator's bar (include/trxhip.h)
    o_res, o_soft = O.pull_batch(iq.numpy(), 4, params)
    for k in ("rc", "tsc", "toa"):
        assert np.array_equal(g[k], o_res[k]), k
    amp = np.hypot(o_res["amp_re"], o_res["amp_im"])
    ratio = np.where(amp > 0, np.sqrt(np.maximum(o_res["energy"], 0)) / np.maximum(amp, 1e-30), 1.0)
    bar = (FUSED_SOFT_ATOL * np.maximum(1.0, ratio / 4.0))[:, None]
    err = np.abs(soft_a.cpu().numpy() - o_soft)
    print(f"max |soft - oracle| = {float(err.max()):.3e} ({float((err / bar).max()):.3f} of the bar), left_geometry {st['left_geometry']}, "
          f"left_gate {st['left_gate']}")
    assert (err <= bar).all(), float((err / bar).max())
    return g, st


@pytest.mark.gpu
def test_every_shift_and_row_of_the_geometry(trx):
    iq, params, _ = sweep()
    g, st = check(trx, iq, params)
    assert (g["rc"] > 0).all()
    hit, n_out = cells_hit(g)
    assert hit == ALL_CELLS, sorted(ALL_CELLS - hit)[:8]          # no cell of the geometry went untested
    # what left the straight-line form is exactly what lies outside the geometry (a burst whose gate was too close to call never
    # reaches the demodulator: it is left to the general kernel as a whole)
    assert n_out > 200 and n_out - st["left_gate"] <= st["left_geometry"] <= n_out, (n_out, st)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["early", "late"])
def test_outside_the_geometry_takes_the_general_form(trx, kind):
    iq, params, _ = outside(kind)
    g, st = check(trx, iq, params)
    assert (g["rc"] > 0).all()
    _, _, _, inside = geometry(g["toa"])
    assert not inside.any()
    assert len(params) - st["left_gate"] <= st["left_geometry"] <= len(params), st
