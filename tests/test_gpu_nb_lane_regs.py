"""The normal-burst kernel's lane-only registers (csrc/trx_kernel_nb.hip: a_p, a_w, a_l4, a_l4c, a_l16, a_st -- addresses that
depend on the lane and the wave alone, made once in front of the burst loop and carried through it): a value that a cold path
clobbered or a row offset that is off by one shows in the bytes of some LATER burst of the same wave.
  1. every kind of burst the loop knows, every cold path among them, in every order inside a wave;
  2. one wave alone, ragged last groups, and all sixteen waves (sixteen slice bases) of every workgroup;
  3. one sample above the clip threshold at the edges of the conversion's rows -- the tenth row's mask and offsets.
The comparison is that of tests/test_gpu_nb_loop_paths.py: the split path against the general kernel alone
(set_nb_kernel(False)) as bytes, and the first 1024 bursts against the oracle (decisions identical, soft bits within the
header's bar)."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from osmo_trx_amd import TrxHip, synth

N_ORACLE = 1024
DEV = "cuda:0"
FILL = 0xa5                     # what the split path's result buffer holds before the launch: a record nobody wrote keeps it
FUSED_SOFT_ATOL = O.header_constant("TRXHIP_FUSED_SOFT_ATOL")
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def trx():
    t = TrxHip(0)
    yield t
    t.close()


def split_and_general(trx, d_iq, params):
    """-> split path's records and soft bits, the general kernel's, and the split launch's fast_stats()"""
    d_p = trx.params_tensor(params)
    trx.set_nb_kernel(True)
    res_a = torch.full((len(params), 32), FILL, dtype=torch.uint8, device=DEV)
    trx.fast_stats(reset=True)
    res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4, results=res_a)
    torch.cuda.synchronize()
    st = trx.fast_stats(reset=True)
    trx.set_nb_kernel(False)
    res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    return res_a, soft_a, res_b, soft_b, st


def assert_bytes(res_a, soft_a, res_b, soft_b):
    bad = np.flatnonzero((res_a != res_b).any(dim=1).cpu().numpy())
    assert torch.equal(res_a, res_b), (len(bad), bad[:8])
    assert torch.equal(soft_a.view(torch.int32), soft_b.view(torch.int32)), \
        np.flatnonzero((soft_a != soft_b).any(dim=1).cpu().numpy())[:8]


def assert_oracle(trx, res, soft, o_res, o_soft):
    """decisions identical to the oracle's on the bursts it was given, soft bits within the header's bar"""
    n = min(len(o_res), len(res))
    o_res, o_soft = o_res[:n], o_soft[:n]
    g = trx.results_to_numpy(res[:n])
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


# ---- 1. a value carried across a cold path comes back intact ---------------------------------------------------------------
KINDS = ("detected", "max_toa_0", "max_toa_31", "real_only", "early", "late", "foreign", "max_toa_33", "noise", "clipped")


@gpu
def test_value_carried_across_a_cold_path(trx):
    """20 000 bursts, more than 4096: every wave takes about five, one after the other, by ticket -- which ones is the hardware's
    choice.  The kinds are drawn i.i.d., so the roughly 16 000 pairs of consecutive bursts of a wave are i.i.d. pairs too: about
    160 of each of the 100 ordered pairs, whatever the assignment.  The cold paths -- the foreign slot, the burst left behind,
    the multiplying correlation, the TOA search's re-run, the general demodulator, the record flush -- derive their own lane id
    and run between two bursts that read a_p, a_w, a_l4, a_l16 and a_st; max_toa 31 takes the wide DEC / CORR forms, other
    offsets of a_w."""
    n = 20000
    kinds = np.random.default_rng(9600).integers(0, len(KINDS), n)
    assert np.bincount(kinds, minlength=len(KINDS)).min() > 1500
    kw = dict(p_noise=0.0, p_clip=0.0)
    spec = {
        "detected": dict(max_toa=5, delay_sym=(0.0, 4.0), **kw),
        "max_toa_0": dict(max_toa=0, delay_sym=(0.0, 2.0), **kw),
        "max_toa_31": dict(max_toa=31, delay_sym=(0.0, 4.0), **kw),
        "real_only": dict(max_toa=5, delay_sym=(0.0, 4.0), snr_range=(15.0, 30.0), **kw),
        "early": dict(max_toa=5, delay_sym=(-3.0, -1.0), snr_range=(15.0, 30.0), **kw),
        "late": dict(max_toa=20, delay_sym=(10.5, 18.0), snr_range=(15.0, 30.0), **kw),
        "foreign": dict(max_toa=5, delay_sym=(0.0, 4.0), **kw),
        "max_toa_33": dict(max_toa=33, delay_sym=(0.0, 4.0), **kw),
        "noise": dict(max_toa=5, delay_sym=(0.0, 4.0), p_noise=1.0, p_clip=0.0),
        "clipped": dict(max_toa=5, delay_sym=(0.0, 4.0), p_noise=0.0, p_clip=1.0),
    }
    d_iq = torch.empty((n, 625, 2), dtype=torch.int16, device=DEV)
    params = np.zeros(n, dtype=O.PARAMS_DTYPE)
    of = {}
    for k, name in enumerate(KINDS):
        rows = np.flatnonzero(kinds == k)
        of[name] = kinds == k
        iq, p, _ = synth.make_normal_bursts(len(rows), DEV, 4, seed=9610 + k, **spec[name])
        if name == "foreign":
            p["type"] = O.EDGE
        if name == "real_only":
            iq[:, :, 1] = 0         # every decimated sample fails the addition-only correlation's guard: the multiplying form
        d_iq[torch.from_numpy(rows).to(DEV)] = iq
        params[rows] = p
    res_a, soft_a, res_b, soft_b, st = split_and_general(trx, d_iq, params)
    print("fast_stats of the split launch:", st)
    assert_bytes(res_a, soft_a, res_b, soft_b)
    assert_oracle(trx, res_a, soft_a, *O.pull_batch(d_iq[:N_ORACLE].cpu().numpy(), 4, params[:N_ORACLE]))
    # every kind occurred, by the records
    r = trx.results_to_numpy(res_a)
    found = r["rc"] > 0
    for name in ("detected", "max_toa_0", "max_toa_31", "max_toa_33"):
        assert found[of[name]].mean() > 0.9, name
    assert ((r["rc"] == 1) & (r["nbits_div4"] == 37))[of["detected"]].mean() > 0.9
    # (real-only: the image of the burst at the mirrored frequency fails the peak-ratio gate -- the oracle finds none of 600 such
    # bursts -- so what the records show of this kind is a miss behind the multiplying correlation; that Q is zero is the input's)
    assert not d_iq[torch.from_numpy(np.flatnonzero(of["real_only"])).to(DEV), :, 1].any()
    assert (r["rc"][of["real_only"]] == 0).mean() > 0.9 and (r["energy"][of["real_only"]] > 0).all()
    assert (r["rc"][of["noise"]] == 0).mean() > 0.9
    assert (r["clip"][of["clipped"]] == 1).mean() > 0.9
    assert not (res_a.cpu().numpy()[of["foreign"]] == FILL).all(axis=1).any()
    assert (r["toa"][of["early"] & found] < -0.5).sum() > 100
    assert (r["toa"][of["late"] & found] > 9.5).sum() > 100
    # the re-run of the TOA search (0.49 % of detections: about 50 expected) and the general demodulator ran inside the kernel
    assert st["reruns"] >= 1 and st["left_geometry"] >= 1, st


# ---- 2. every wave's slice base and short batches ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized_batch():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    d_iq, params, _ = synth.make_normal_bursts(256 * n_cu + 1, DEV, 4, seed=9700)
    return n_cu, d_iq, params, O.pull_batch(d_iq[:N_ORACLE].cpu().numpy(), 4, params[:N_ORACLE])


SIZES = {"1": lambda n_cu: 1, "15": lambda n_cu: 15, "16": lambda n_cu: 16, "17": lambda n_cu: 17,
         "16*n_cu-1": lambda n_cu: 16 * n_cu - 1, "256*n_cu+1": lambda n_cu: 256 * n_cu + 1}


@gpu
@pytest.mark.parametrize("size", list(SIZES))
def test_every_waves_slice_base_and_short_batches(trx, sized_batch, size):
    """one wave alone; a group short of one burst, a full one, one burst of a second; every compute unit's first group with the
    last one ragged; and sixteen bursts per wave with all sixteen waves -- the sixteen different a_w and a_p -- of every
    workgroup at work"""
    n_cu, d_iq, params, oracle = sized_batch
    n = SIZES[size](n_cu)
    res_a, soft_a, res_b, soft_b, _ = split_and_general(trx, d_iq[:n], params[:n])
    assert_bytes(res_a, soft_a, res_b, soft_b)
    assert_oracle(trx, res_a, soft_a, *oracle)


# ---- 3. the rows' edges --------------------------------------------------------------------------------------------------------
EDGES = (0, 63, 64, 575, 576, 623, 624)
NOISE_SIGMA = 300.0             # the clip threshold, 30000, is 100 sigma away


def edge_noise():
    """64 noise-only bursts, the same for the CPU check and every GPU case"""
    x = np.random.default_rng(9800).normal(0.0, NOISE_SIGMA, (64, 625, 2))
    params = np.zeros(64, dtype=O.PARAMS_DTYPE)
    params["type"] = O.TSC
    params["tsc"] = np.arange(64) % 8
    params["max_toa"] = 5
    return np.round(x).astype(np.int16), params


def test_edge_noise_is_not_clipped_by_itself():
    """the oracle on the noise alone: no record says clipped, so the flag in the GPU cases below comes from the one sample"""
    iq, params = edge_noise()
    assert np.abs(iq.astype(np.int32)).max() < 3000
    o_res, _ = O.pull_batch(iq, 4, params)
    assert not o_res["clip"].any()


@gpu
@pytest.mark.parametrize("sample", EDGES)
def test_one_clipping_sample_at_a_row_edge(trx, sample):
    """sample `sample` of every burst set to 32000 (I in the even bursts, Q in the odd ones: both halves of its word).  The
    conversion's row r holds samples 64 r .. 64 r + 63 at offset 128 r of a_p; the tenth holds 576 .. 624 on lanes 0 .. 48 under
    a constant mask -- sample 624 is the only one of its lane 48.  A row offset or a mask that is off by one loses the sample:
    the clip scan reads what the conversion made."""
    iq, params = edge_noise()
    iq[0::2, sample, 0] = 32000
    iq[1::2, sample, 1] = 32000
    d_iq = torch.from_numpy(iq).to(DEV)
    res_a, soft_a, res_b, soft_b, _ = split_and_general(trx, d_iq, params)
    r = trx.results_to_numpy(res_a)
    assert (r["clip"] == 1).all(), np.flatnonzero(r["clip"] != 1)[:8]
    assert_bytes(res_a, soft_a, res_b, soft_b)
    assert_oracle(trx, res_a, soft_a, *O.pull_batch(iq, 4, params))
