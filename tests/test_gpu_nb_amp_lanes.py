"""Block TAIL's per-lane 1 / amp, DETA's m from the arg-max, and the product-sum chains that start as a product (csrc/
trx_kernel_nb.hip, tools/gen_nb_asm.py: amp_lane, chain_term): 2048 normal bursts at 4 SPS, all eight TSCs, the carrier phase of
amp = peak / gain set to sixteen steps of pi / 8 -- the four axes among them, where amp.re or amp.im is tiny -- so that every
lane variant of the new table multiplies both signs of both components.  Mixed in between the ordinary bursts, in one fixed
shuffle: an all-zero burst, bursts with every fourth sample zeroed (one polyphase row: exact-zero products all along the
chains), bursts whose first 48 samples are zero (the +-0 products at the chains' starts and behind the low-edge rows' leading
zero taps), noise-only slots, clipped bursts, bursts later than 9 symbols and early bursts (the geometry's cold exit, which
forms amp in C++), and the widest window.

Soft bits and records of the default path are compared byte for byte, every burst, with the general kernel alone
(set_nb_kernel(False)), and with the oracle within the header's bars.  The phase is set by rotating each generated burst by
the difference between the step and the phase the oracle finds in it: the rotation turns signal and noise alike, so the
detected phase follows it up to the int16 rounding of the rotated samples."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from osmo_trx_amd import TrxHip, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PER_KIND = 128                  # 8 TSCs x 16 phase steps
STEPS = 16
FUSED_SOFT_ATOL = O.header_constant("TRXHIP_FUSED_SOFT_ATOL")
FAST_AMP_RTOL = O.header_constant("TRXHIP_FAST_AMP_RTOL")
AMPS = dict(amp_range=(500.0, 15000.0))
QUIET = dict(p_noise=0.0, p_clip=0.0, **AMPS)
PLAIN = dict(max_toa=3, delay_sym=(0.0, 4.0), snr_range=(12.0, 30.0), **QUIET)
LOUD = dict(snr_range=(15.0, 30.0), **QUIET)
KINDS = (
    ("plain0", PLAIN), ("plain1", PLAIN), ("plain2", PLAIN), ("plain3", PLAIN), ("plain4", PLAIN), ("plain5", PLAIN),
    ("plain6", PLAIN), ("plain7", PLAIN),
    ("zero", PLAIN),                                               # every sample zero
    ("fourth", dict(max_toa=3, delay_sym=(0.0, 4.0), **LOUD)),     # samples k, k + 4, .. zero (k = 0..3)
    ("head48", dict(max_toa=3, delay_sym=(0.0, 4.0), **LOUD)),     # samples 0..47 zero
    ("noise", dict(max_toa=3, p_noise=1.0, p_clip=0.0, **AMPS)),
    ("clipped", dict(max_toa=3, p_noise=0.0, p_clip=1.0)),
    ("late", dict(max_toa=20, delay_sym=(10.5, 18.0), **LOUD)),
    ("early", dict(max_toa=5, delay_sym=(-3.0, -1.0), **LOUD)),
    ("wide", dict(max_toa=32, delay_sym=(0.0, 4.0), **LOUD)),
)
NAMES = tuple(k for k, _ in KINDS)
N = PER_KIND * len(KINDS)


@pytest.fixture(scope="module")
def trx():
    t = TrxHip(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def batch():
    """(kind index[N], phase step[N], iq int16[N, 625, 2] on the CPU, params)"""
    iqs, prms = [], []
    for k, (name, kw) in enumerate(KINDS):
        iq, p, _ = synth.make_normal_bursts(PER_KIND, "cpu", 4, seed=16100 + k, **kw)
        iqs.append(iq)
        prms.append(p)
    iq, params = torch.cat(iqs).numpy(), np.concatenate(prms)
    kind = np.repeat(np.arange(len(KINDS)), PER_KIND)
    step = (np.arange(N) // 8) % STEPS
    assert (params["tsc"] == np.arange(N) % 8).all()
    # ---- the phase: rotate by (step * pi / 8 - the phase the oracle finds).  Multiples of pi / 2 would be exact; the others round
    base, _ = O.pull_batch(iq, 4, params)
    phi = np.arctan2(base["amp_im"].astype(np.float64), base["amp_re"].astype(np.float64))
    rot = np.where(base["rc"] > 0, np.exp(1j * (step * (np.pi / 8) - phi)), 1.0)
    x = (iq[..., 0].astype(np.float64) + 1j * iq[..., 1]) * rot[:, None]
    # (a rotation keeps |x|: with amplitudes up to 15000 no component of an unclipped kind comes near the clip threshold, and
    # the clipped kind's saturated samples stay above it)
    iq = np.stack([np.clip(np.round(x.real), -32768, 32767), np.clip(np.round(x.imag), -32768, 32767)], -1).astype(np.int16)
    # ---- the zeroed kinds
    iq[kind == NAMES.index("zero")] = 0
    for r in np.flatnonzero(kind == NAMES.index("fourth")):
        iq[r, (r // 8) % 4::4] = 0
    iq[kind == NAMES.index("head48"), :48] = 0
    # ---- one fixed shuffle: every kind between ordinary bursts of the same wave
    perm = np.random.default_rng(16001).permutation(N)
    return kind[perm], step[perm], torch.from_numpy(np.ascontiguousarray(iq[perm])), params[perm]


@pytest.fixture(scope="module")
def runs(trx, batch):
    """default path (with its counters), general kernel alone, oracle: computed once"""
    _, _, iq, params = batch
    d_iq, d_p = iq.to(DEV), trx.params_tensor(params)
    trx.set_nb_kernel(True)
    trx.fast_stats(reset=True)
    res_a, soft_a = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    stats = trx.fast_stats(reset=True)
    trx.set_nb_kernel(False)
    res_b, soft_b = trx.detect_demod(d_iq, d_p, sps=4)
    torch.cuda.synchronize()
    trx.set_nb_kernel(True)
    o_res, o_soft = O.pull_batch(iq.numpy(), 4, params)
    return dict(res_a=res_a, soft_a=soft_a, res_b=res_b, soft_b=soft_b, o_res=o_res, o_soft=o_soft, stats=stats)


def test_default_path_is_the_general_kernel_byte_for_byte(runs):
    res_a, soft_a, res_b, soft_b = runs["res_a"], runs["soft_a"], runs["res_b"], runs["soft_b"]
    assert len(res_a) == N == len(soft_a)                           # every burst: none is left out of the comparison
    bad = np.flatnonzero((res_a != res_b).any(dim=1).cpu().numpy())
    assert torch.equal(res_a, res_b), (len(bad), bad[:8])
    assert torch.equal(soft_a.view(torch.int32), soft_b.view(torch.int32)), \
        np.flatnonzero((soft_a != soft_b).any(dim=1).cpu().numpy())[:8]


def test_every_sign_quadrant_of_amp_and_the_axes(trx, batch, runs):
    kind, step, _, params = batch
    r = trx.results_to_numpy(runs["res_a"])
    det = r["rc"] > 0
    plain = det & (kind < 8)
    quad = (r["amp_re"] > 0).astype(int) * 2 + (r["amp_im"] > 0).astype(int)
    for t in range(8):
        rows = plain & (params["tsc"] == t)
        counts = np.bincount(quad[rows], minlength=4)
        print("tsc", t, "detected ordinary bursts by sign quadrant of amp:", counts.tolist())
        assert (counts >= 8).all(), (t, counts)
        assert set(step[rows]) == set(range(STEPS)), t
    # on the axes one component is tiny: the detected phase is the step's up to the rounding of the rotated samples
    small = np.minimum(np.abs(r["amp_re"]), np.abs(r["amp_im"])) / np.maximum(np.hypot(r["amp_re"], r["amp_im"]), 1e-30)
    axis = plain & (step % 4 == 0)
    print("bursts on an axis:", int(axis.sum()), "smaller / larger component: median", float(np.median(small[axis])),
          "largest", float(small[axis].max()))
    assert axis.sum() >= 200 and np.median(small[axis]) < 1e-2
    for s in (0, 4, 8, 12):                                         # each of the four axes, each side of it
        rows = plain & (step == s)
        minor = r["amp_im"][rows] if s % 8 == 0 else r["amp_re"][rows]
        assert (minor > 0).any() and (minor < 0).any(), s


def test_the_kinds_are_what_they_say(trx, batch, runs):
    kind, _, iq, params = batch
    r = trx.results_to_numpy(runs["res_a"])
    of = {name: kind == k for k, name in enumerate(NAMES)}
    found = r["rc"] > 0
    stats = runs["stats"]
    print("fast_stats:", stats, {name: float(found[of[name]].mean()) for name in NAMES})
    for k in range(8):
        assert found[of[f"plain{k}"]].mean() > 0.9
    assert not found[of["zero"]].any() and not iq.numpy()[of["zero"]].any()
    assert (r["rc"][of["noise"]] == 0).mean() > 0.9
    assert found[of["head48"]].mean() > 0.9 and not iq.numpy()[of["head48"], :48].any()
    assert found[of["fourth"]].mean() > 0.5
    assert (r["clip"][of["clipped"]] == 1).mean() > 0.9 and not r["clip"][~of["clipped"]].any()
    assert found[of["wide"]].mean() > 0.9 and (params["max_toa"][of["wide"]] == 32).all()
    # the geometry's cold exit, both sides (the general form of the demodulator, amp formed in C++)
    assert (r["toa"][of["late"] & found] > 9.5).sum() >= 32
    assert (r["toa"][of["early"] & found] < -0.5).sum() >= 32
    assert stats["left_geometry"] >= 64, stats


def test_against_the_oracle(trx, runs):
    o_res, o_soft = runs["o_res"], runs["o_soft"]
    g = trx.results_to_numpy(runs["res_a"])
    for k in ("rc", "tsc", "clip", "toa"):
        bad = np.flatnonzero(g[k] != o_res[k])
        assert bad.size == 0, (k, bad[:8], g[k][bad[:8]], o_res[k][bad[:8]])
    det = o_res["rc"] > 0
    aref = np.hypot(o_res["amp_re"], o_res["amp_im"])
    aerr = np.hypot(g["amp_re"] - o_res["amp_re"], g["amp_im"] - o_res["amp_im"])
    print("largest amp error / |amp|:", float((aerr[det] / aref[det]).max()), "bar", FAST_AMP_RTOL)
    assert (aerr[det] <= FAST_AMP_RTOL * aref[det]).all()
    O.assert_fast_ci(g["ci"][det], o_res["ci"][det])
    # the fused demodulator's statement of include/trxhip.h: |soft - ref| <= TRXHIP_FUSED_SOFT_ATOL * max(1, rms / (4 |amp|))
    ratio = np.where(aref > 0, np.sqrt(np.maximum(o_res["energy"], 0)) / np.maximum(aref, 1e-30), 1.0)
    bar = (FUSED_SOFT_ATOL * np.maximum(1.0, ratio / 4.0))[:, None]
    err = np.abs(runs["soft_a"].cpu().numpy() - o_soft)
    print("detected:", int(det.sum()), "of", N, "-- largest soft-bit error against the oracle, in bars:", float((err / bar).max()))
    assert (err <= bar).all(), float((err / bar).max())
