"""The kernel-instance matrix of trxhip_detect_demod_batch{,_cf32} (pytest -m gpu): every instance pull_common()
(csrc/trx_capi.cpp) can launch, against the CPU oracle, on the two axes the rest of the suite hardly touches -- 1 SPS and
complex64 input:

  burst_pull_kernel<1, cf32, 3>            1 SPS (always the exact demodulator)
  burst_pull_kernel<4, cf32, 10>           4 SPS, L 629..640 (prefetching)
  burst_pull_kernel<4, cf32, 0>            4 SPS, L 641..1536
  burst_pull4_kernel<cf32, exact, common>  4 SPS, L 624..628: fused + sliced rows of 148 at L = 625 (COMMON), fused otherwise,
                                           exact (12 waves per workgroup with complex64 input)

Bars: the project's existing ones and no other -- exact paths bit-identical to the oracle; fused paths inside
TRXHIP_FAST_AMP_RTOL, TRXHIP_FAST_CI_ATOL_DB and TRXHIP_FUSED_SOFT_ATOL{,_8PSK} (include/trxhip.h); energy / RSSI / C/I as
parity_checks.check_parity states them.  Every condition "on the oracle alone" makes sure a batch exercises what it is meant to
(detections on both sides of a threshold, early and late TOAs, ...) and says nothing about the GPU.  Oracle references are
computed once per (batch, row layout), kept read-only and shared between the tests."""
import functools
import os
import re

import numpy as np
import pytest

import instance_inputs as I
import oracle_lib as O
from parity_checks import run_gpu, check_parity, FUSED_SOFT_ATOL, FUSED_SOFT_ATOL_8PSK

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_TOA_LIMIT = int(O.header_constant("TRXHIP_MAX_TOA"))
LENS_1SPS = (148, 156, 157, 192)                                        # pull_common() accepts 148..192 at 1 SPS
RROT1_LEN = 157                                                         # GMSKReverseRotation1 (sigProcLib.cpp:207)


@pytest.fixture(scope="module")
def trx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_ORACLE = {}


def oracle(key, iq, sps, params, **kw):
    """O.pull_batch / O.pull_batch_cf32 (by dtype) of a named batch, computed once per row layout, read-only."""
    k = (key, str(iq.dtype), tuple(sorted(kw.items())))
    if k not in _ORACLE:
        assert len(params) <= 1024
        fn = O.pull_batch_cf32 if iq.dtype == torch.complex64 else O.pull_batch
        res, soft = fn(iq.numpy(), sps, params, **kw)
        res.setflags(write=False)
        soft.setflags(write=False)
        _ORACLE[k] = (res, soft)
    return _ORACLE[k]


def with_max_toa_rule(o_res, o_soft, params):
    """include/trxhip.h: max_toa > TRXHIP_MAX_TOA is refused with -SIGERR_UNSUPPORTED instead of searched (the rule
    test_gpu_parity.py::test_fuzz_against_oracle applies)."""
    o_res, o_soft = o_res.copy(), o_soft.copy()
    live = (params["max_toa"] > MAX_TOA_LIMIT) & ~np.isin(params["type"], [O.OFF, O.IDLE, O.SCH, 9]) & \
        ~((params["tsc"] > 7) & np.isin(params["type"], [O.TSC, O.EDGE]))
    o_res["rc"][live] = -O.SIGERR_UNSUPPORTED
    for f in ("toa", "amp_re", "amp_im", "ci", "tsc", "nbits_div4"):
        o_res[f][live] = 0
    o_res["idle"][live] = 1
    o_soft[live] = 0
    return o_res, o_soft


def cat(parts):
    return torch.cat([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ------------------------------------------------------------------------------------------------
# 1 SPS, int16 and complex64: burst_pull_kernel<1, *, 3>
# ------------------------------------------------------------------------------------------------
# 33 / 34: on either side of the straight-line branch's limit.  Both branches must give the oracle's bits; the batch does not pin
# WHERE the limit sits (at 34 the straight-line geometry still holds and gives the same bits, see test_1sps_unit_correlation_guard).
MAX_TOA_1SPS = np.array([0, 3, 32, 33, 34, 63, 112], dtype=np.uint16)


@functools.lru_cache(None)
def nb_1sps(L, n=1024):
    """Normal bursts, all eight TSCs (burst i: TSC i % 8), delays -2..28 symbols, max_toa cycling with period 7: straight-line
    and general bursts alternate inside every wave, every (TSC, max_toa) pair occurs."""
    from osmo_trx_amd import synth
    iq, params, _ = synth.make_normal_bursts(n, "cpu", 1, seed=3100 + L, max_toa=30, delay_sym=(-2.0, 28.0), snr_range=(10.0, 30.0),
                                             burst_len=L)
    params["max_toa"] = MAX_TOA_1SPS[np.arange(n) % len(MAX_TOA_1SPS)]
    return iq, params


def nb_1sps_conditions(o_res, params):
    det = o_res["rc"] > 0
    assert det[params["max_toa"] >= 32].mean() >= 0.85
    assert det[params["max_toa"] == 33].sum() >= 50 and det[params["max_toa"] == 34].sum() >= 50
    assert (o_res["toa"][det] < 0).any() and (o_res["toa"][det] > 20).any()
    return int(det.sum())


@pytest.mark.parametrize("L", LENS_1SPS)
def test_1sps_normal_bursts_all_tsc_and_windows(trx, L):
    """burst_pull_kernel<1, false, 3> and <1, true, 3>: the straight-line branch (TSC 0..7, max_toa <= 33, its windows running
    past the burst at L = 148) and detect_any_burst<false, false> (max_toa 34, 63, 112) in one batch; sliced rows of 148, raw rows
    of stride L, and at L = 192 raw rows of stride 200: values for i < 157, zeros behind (the reference's rotation table ends
    there, include/trxhip.h).  int16 against the oracle bit for bit; complex64 of the same bursts bit-identical to the int16
    launch and to O.pull_batch_cf32."""
    iq, params = nb_1sps(L)
    x = I.as_cf32(iq)
    for stride, sl in [(148, True), (L, False)] + ([(200, False)] if L == 192 else []):
        kw = dict(soft_stride=stride, slice_bits=sl)
        o_res, o_soft = oracle(("nb1", L), iq, 1, params, **kw)
        nb_1sps_conditions(o_res, params)
        g_res, g_soft = run_gpu(trx, iq, params, 1, **kw)
        check_parity(g_res, g_soft, o_res, o_soft)
        if not sl:
            det = o_res["rc"] > 0
            assert not g_soft[:, RROT1_LEN:].any() and (g_soft[det][:, min(L, RROT1_LEN) - 1] != 0).any()
        c_res, c_soft = run_gpu(trx, x, params, 1, **kw)
        assert same_bits(c_res, g_res) and same_bits(c_soft, g_soft)
        oc_res, oc_soft = oracle(("nb1", L), x, 1, params, **kw)
        check_parity(c_res, c_soft, oc_res, oc_soft)


def residue_only_burst(tsc, rng, A=8000.0, max_toa=3):
    """The input on which corr_unit() and the multiplying correlation differ most: an ideal rotated burst (every sample +-A or
    +-iA exactly), whose correlation with the unit taps leaves one component of every lag EXACTLY zero.  xs[56] keeps its zero
    component (the one guard-unsafe sample of the window xs[56 .. 56 + 15 + len)); the window's other samples get a small
    perpendicular integer each (safe: ratio <= 8000), chosen by the recurrence below so that their sum cancels exactly at every
    lag.  The multiplying path then leaves the residue A * e, e ~ 4.6e-14, in that component of corr[0]; corr_unit() leaves 0."""
    from osmo_trx_amd import synth
    u = np.round(O.tables()["midamble"][tsc]["seq"].astype(np.complex128))           # the taps' unit structure: +-1 / +-i
    ln = 16 + max_toa
    while True:
        bits = rng.integers(0, 2, 148).astype(np.uint8)
        bits[:3] = 0
        bits[-3:] = 0
        bits[61:87] = [int(c) for c in synth.TSC_BITS[tsc]]
        main = np.round(O.modulate_burst(bits, 8, 1, empty=True).astype(np.complex128))   # 156 samples, exactly +-1 or +-i
        perp = 1j * main
        x = A * main
        x[57:71] += rng.choice([-2.0, -1.0, 1.0, 2.0], size=14) * perp[57:71]
        ok = True
        for j in range(ln):                                                 # corr[j] = sum_k xs[56 + j + k] * u[k]; solve for xs[71 + j]
            c = np.dot(x[56 + j:72 + j], u)
            coef = perp[71 + j] * u[15]
            d = -(c.imag / coef.imag if coef.real == 0 else c.real / coef.real) if (j - 10) % 2 == 0 else \
                -(c.real / coef.real if coef.imag == 0 else c.imag / coef.imag)
            x[71 + j] += d * perp[71 + j]
            ok = ok and d != 0 and abs(d) <= 20000
        if ok:
            iq = torch.zeros((156, 2), dtype=torch.int16)
            iq[:, 0] = torch.from_numpy(x.real.astype(np.int16))
            iq[:, 1] = torch.from_numpy(x.imag.astype(np.int16))
            return iq


@functools.lru_cache(None)
def unit_guard_1sps(n=128):
    """Five sub-batches around the straight-line branch's guard, which inspects xs[56 + lane], lane < 15 + len, len = 16 + max_toa
    (max_toa 3 and 33 alternate): a component that is exactly zero makes a sample "unsafe" for the addition-only correlation."""
    from osmo_trx_amd import synth
    subs = []
    for k, name in enumerate(("whole", "first", "last", "outside", "patterns")):
        iq, params, _ = synth.make_normal_bursts(n, "cpu", 1, seed=4100 + k, delay_sym=(0.0, 3.0), snr_range=(15.0, 30.0), p_noise=0.0,
                                                 p_clip=0.0, burst_len=156)
        iq = iq.clone()
        params["max_toa"] = np.where(np.arange(n) % 2, 33, 3)
        last = 56 + 15 + 16 + params["max_toa"].astype(int) - 1                 # the last sample the ballot inspects
        for b in range(n):
            comp = (b // 2) % 2
            if name == "whole":
                iq[b, :, comp] = 0
            elif name == "first":
                iq[b, 56, comp] = 0
            elif name == "last":
                iq[b, last[b], comp] = 0
            elif name == "outside":
                iq[b, last[b] + 1, comp] = 0                                     # just outside: must not matter
            else:
                # int16 cannot reach a 2^17 ratio between non-zero components: unit patterns and small values instead
                pos = (56, last[b], last[b] + 1)[b % 3]
                iq[b, pos] = torch.tensor([(1, 0), (0, 1), (0, -3), (2, 0), (1, 1), (32767, 1), (0, 0)][b % 7], dtype=torch.int16)
        # a burst with one component zero throughout keeps every other symbol only (pi/2 rotation per symbol): its peak ratio stays
        # below BURST_THRESH = 4, so that sub-batch is searched with a threshold of 2.5 (both sides) to have detections
        subs.append((name, iq, params, 2.5 if name == "whole" else 4.0))
    rng = np.random.default_rng(4200)
    iq = torch.stack([residue_only_burst(b % 8, rng) for b in range(32)])
    params = np.zeros(32, dtype=O.PARAMS_DTYPE)
    params["type"], params["tsc"], params["max_toa"] = O.TSC, np.arange(32) % 8, 3
    subs.append(("residue", iq, params, 4.0))
    return subs


def test_1sps_unit_correlation_guard(trx):
    """burst_pull_kernel<1, false, 3>, straight-line branch: unit_unsafe() over xs[56 .. 56 + 15 + len) decides between
    corr_unit() and the multiplying correlation; BOTH must give the oracle's bits, and that is what this test checks: zero
    components on the whole burst, on the first and the last inspected sample, just outside the inspected range, and the
    residue-only bursts.  It does NOT pin which samples the guard inspects, and no result-comparing test can: the two
    correlations differ by |x| * 4.6e-14 in one component of corr[0] (xs[56]) or corr[len - 1] (the last sample; never read by
    interpolatePoint, sigProcLib.cpp:1105); even where every other term of that component is exactly zero (residue_only_burst)
    the result divides the peak by the sequence's gain, whose imaginary part (3e-3 .. 8e-2 of 15) puts 2e-4 .. 5e-3 of the peak
    into that component of amp and buries the residue 1e9 times over.  A guard reading xs[57 + lane], or a straight-line
    limit of 34 (whose only fault is that 64 lanes no longer cover the 65 samples), passes this test and every other."""
    for name, iq, params, thr in unit_guard_1sps():
        o_res, o_soft = oracle(("unit1", name), iq, 1, params, threshold=thr)
        assert (o_res["rc"] > 0).sum() >= len(params) // 2, name
        g_res, g_soft = run_gpu(trx, iq, params, 1, threshold=thr)
        check_parity(g_res, g_soft, o_res, o_soft)


MAX_TOA_RACH = np.array([3, 63, 112], dtype=np.uint16)


@functools.lru_cache(None)
def access_1sps(L, ext, n=512):
    iq, params, ts = I.access_bursts_1sps(n, L, ext, seed=5100 + 2 * L + int(ext))
    params["max_toa"] = MAX_TOA_RACH[np.arange(n) % 3]
    return iq, params, ts


def access_1sps_conditions(o_res, params, ext):
    det = o_res["rc"] > 0
    assert det[params["max_toa"] >= 63].mean() >= 0.85
    assert (o_res["rc"][det] == (O.EXT_RACH if ext else O.RACH)).all()
    if ext:
        assert (np.bincount(o_res["tsc"][det], minlength=3)[:3] >= 30).all()
    return int(det.sum())


@pytest.mark.parametrize("L", (148, 157, 192))
@pytest.mark.parametrize("ext", [False, True])
def test_1sps_access_bursts(trx, ext, L):
    """burst_pull_kernel<1, false, 3> -> detect_any_burst<false, false>, RACH / EXT_RACH: the three sync sequences (first hit
    wins), max_toa 3 / 63 / 112 per burst -- at L = 148 the two wide windows run past the burst."""
    iq, params, _ = access_1sps(L, ext)
    for kw in (dict(soft_stride=148, slice_bits=True), dict(soft_stride=L, slice_bits=False)):
        o_res, o_soft = oracle(("rach1", L, ext), iq, 1, params, **kw)
        access_1sps_conditions(o_res, params, ext)
        g_res, g_soft = run_gpu(trx, iq, params, 1, **kw)
        check_parity(g_res, g_soft, o_res, o_soft)


MAX_TOA_EDGE = np.array([5, 33, 34], dtype=np.uint16)


@functools.lru_cache(None)
def edge_1sps(L, off, n=256, n_nb=64):
    """n 8-PSK bursts (4-SPS bursts decimated from sample `off`), every 16th slot typed TSC, followed by n_nb GMSK normal bursts
    in slots typed EDGE (detectAnyBurst falls through to TSC, sigProcLib.cpp:1933-1941)."""
    from osmo_trx_amd import synth
    iq, params, bits = I.edge_bursts_1sps(n, L, off, seed=6100 + L)
    params["max_toa"] = MAX_TOA_EDGE[np.arange(n) % 3]
    params["type"][15::16] = O.TSC
    iq_nb, p_nb, _ = synth.make_normal_bursts(n_nb, "cpu", 1, seed=6200 + L, burst_len=L)
    p_nb["type"] = O.EDGE
    p_nb["max_toa"] = MAX_TOA_EDGE[np.arange(n_nb) % 3]
    return torch.cat([iq, iq_nb]), np.concatenate([params, p_nb]), bits


def edge_1sps_conditions(o_res, o_soft, params, bits, sliced):
    n = len(bits)
    slots = params["type"][:n] == O.EDGE
    hit = (o_res["rc"][:n] == O.EDGE) & slots
    assert hit.sum() >= 0.9 * slots.sum()
    assert (o_res["nbits_div4"][:n][hit] == 111).all()
    assert ((o_soft[:n][hit] > (0.5 if sliced else 0.0)).astype(np.uint8) != bits[hit]).mean() < 0.03
    assert (o_res["rc"][n:] == O.TSC).sum() >= 0.8 * (len(params) - n)          # the fall-through finds the normal bursts
    return int(hit.sum())


@pytest.mark.parametrize("L", LENS_1SPS)
def test_1sps_edge_slots(trx, L):
    """burst_pull_kernel<1, false, 3>: EDGE slots at 1 SPS -- detect_any_burst<false, false> with the EDGE midambles, then
    edge_post(xs, L, ...) over the burst itself (n_dec = L, no decimation): equaliser, derotation, C/I, 444 soft bits.  All four
    decimation phases of the 4-SPS generator, max_toa 5 / 33 / 34, rows of 444 sliced and raw; C/I inside check_parity's bar."""
    for off in range(4):
        iq, params, bits = edge_1sps(L, off)
        for sl in (True, False):
            o_res, o_soft = oracle(("edge1", L, off), iq, 1, params, soft_stride=444, slice_bits=sl)
            edge_1sps_conditions(o_res, o_soft, params, bits, sl)
            g_res, g_soft = run_gpu(trx, iq, params, 1, soft_stride=444, slice_bits=sl)
            check_parity(g_res, g_soft, o_res, o_soft)


IDLE_THRESHOLD = 1.5      # the dummy midamble repeats every 8 bits: its peak ratio stays below 4 (see test_gpu_parity.py's dummy test)


@functools.lru_cache(None)
def idle_1sps(L):
    from osmo_trx_amd import synth
    iq_d, p_d = I.dummy_bursts_1sps(128, L, seed=7100 + L)
    iq_n, p_n, _ = synth.make_normal_bursts(64, "cpu", 1, seed=7200 + L, p_noise=1.0, burst_len=L)
    iq_b, p_b, _ = synth.make_normal_bursts(64, "cpu", 1, seed=7300 + L, max_toa=5, burst_len=L)
    iq, params = cat([(iq_d, p_d), (iq_n, p_n), (iq_b, p_b)])
    params["type"] = O.IDLE
    return iq, params


@pytest.mark.parametrize("L", LENS_1SPS)
def test_1sps_idle_slots_with_and_without_dummy_search(trx, L):
    """burst_pull_kernel<1, false, 3>: IDLE slots are skipped (Transceiver.cpp:754-755) unless TRXHIP_FLAG_IDLE_DUMMY asks for
    detectDummyBurst (sigProcLib.cpp:1863-1877).  Dummy bursts, noise and normal bursts; both rc patterns equal the oracle's."""
    iq, params = idle_1sps(L)
    for kw in (dict(soft_stride=148, slice_bits=True), dict(soft_stride=L, slice_bits=False)):
        o_res, o_soft = oracle(("idle1", L), iq, 1, params, threshold=IDLE_THRESHOLD, idle_dummy=True, **kw)
        assert (o_res["rc"][:128] == O.IDLE).sum() >= 64 and (o_res["tsc"] == 0).all()
        assert (o_res["idle"][o_res["rc"] == O.IDLE] == 0).all()
        g_res, g_soft = run_gpu(trx, iq, params, 1, threshold=IDLE_THRESHOLD, idle_dummy=True, **kw)
        check_parity(g_res, g_soft, o_res, o_soft)
        o_res, o_soft = oracle(("idle1", L), iq, 1, params, threshold=IDLE_THRESHOLD, **kw)
        assert (o_res["rc"] == 0).all() and (o_res["idle"] == 1).all() and (o_res["energy"] > 0).all()
        g_res, g_soft = run_gpu(trx, iq, params, 1, threshold=IDLE_THRESHOLD, **kw)
        check_parity(g_res, g_soft, o_res, o_soft)


@functools.lru_cache(None)
def fuzz_1sps(L, n=768):
    """tests/test_gpu_parity.py::_fuzz_batch at 1 SPS: random slot types (invalid ones included), TSC 0..8, every kind of search
    window, over normal / access / 8-PSK bursts with wild timing, silence, +-full-scale saturation and single impulses."""
    from osmo_trx_amd import synth
    rng = np.random.default_rng(8100 + L)
    iq, params, _ = synth.make_normal_bursts(n, "cpu", 1, seed=int(rng.integers(1 << 30)), max_toa=30, delay_sym=(-9.0, 34.0),
                                             p_noise=0.1, p_clip=0.05, burst_len=L)
    iq = iq.clone()
    iq_rb, _, _ = I.access_bursts_1sps(n, L, True, seed=int(rng.integers(1 << 30)))
    iq_eb, _, _ = I.edge_bursts_1sps(n, L, int(rng.integers(4)), seed=int(rng.integers(1 << 30)))
    kind = rng.random(n)
    iq[torch.from_numpy(kind < 0.3)] = iq_rb[torch.from_numpy(kind < 0.3)]
    iq[torch.from_numpy(kind > 0.88)] = iq_eb[torch.from_numpy(kind > 0.88)]
    params["type"] = rng.choice([O.OFF, O.TSC, O.EXT_RACH, O.RACH, O.SCH, O.EDGE, O.IDLE, 9], size=n,
                                p=[0.04, 0.4, 0.12, 0.2, 0.02, 0.15, 0.05, 0.02])
    params["tsc"] = rng.integers(0, 9, size=n)                              # 8 is invalid
    params["max_toa"] = rng.choice([0, 1, 3, 30, 33, 34, 63, 112, 113, 400], size=n)
    special = rng.random(n)
    iq[torch.from_numpy(special < 0.02)] = 0                                # silence: energy 0, rssi inf
    iq[torch.from_numpy((special >= 0.02) & (special < 0.04))] = 32767
    iq[torch.from_numpy((special >= 0.04) & (special < 0.05))] = -32768
    for i in np.where((special >= 0.05) & (special < 0.07))[0]:
        iq[i] = 0
        iq[i, int(rng.integers(0, L)), 0] = 20000
    return iq, params


FUZZ_1SPS = [(148, 148), (157, 1), (157, 444), (192, 100), (192, 200)]


@pytest.mark.parametrize("L,soft_stride", FUZZ_1SPS)
def test_1sps_fuzz_against_oracle(trx, L, soft_stride):
    """burst_pull_kernel<1, false, 3> and <1, true, 3>: every branch of the 1-SPS kernel in one adversarial batch, odd soft
    strides, sliced and raw rows; max_toa > TRXHIP_MAX_TOA by the header's rule.  complex64 of the same bursts: bit-identical to
    the int16 launch, equal to O.pull_batch_cf32."""
    iq, params = fuzz_1sps(L)
    x = I.as_cf32(iq)
    for sl in (True, False):
        kw = dict(soft_stride=soft_stride, slice_bits=sl)
        o_res, o_soft = with_max_toa_rule(*oracle(("fuzz1", L), iq, 1, params, **kw), params)
        assert set(np.unique(o_res["rc"])) >= {-3, 0, O.TSC, O.EXT_RACH, O.RACH}
        g_res, g_soft = run_gpu(trx, iq, params, 1, **kw)
        check_parity(g_res, g_soft, o_res, o_soft)
        c_res, c_soft = run_gpu(trx, x, params, 1, **kw)
        assert same_bits(c_res, g_res) and same_bits(c_soft, g_soft)
        oc_res, oc_soft = with_max_toa_rule(*oracle(("fuzz1", L), x, 1, params, **kw), params)
        check_parity(c_res, c_soft, oc_res, oc_soft)


@pytest.mark.parametrize("cf32", [False, True])
def test_1sps_results_do_not_depend_on_the_batch_size(trx, cf32):
    """burst_pull_kernel<1, *, 3>: 16 waves per workgroup claim bursts in groups of 16 and prefetch one burst ahead.  On the fuzz
    batch (branches alternate inside a wave), L = 192, raw rows of stride 200: every burst alone, and the batch in slices of 1, 15,
    16, 17, 255 and 257, equal the whole-batch launch."""
    iq, params = fuzz_1sps(192)
    d_iq = (I.as_cf32(iq) if cf32 else iq).to("cuda:0")
    d_p = trx.params_tensor(params)
    n = len(params)
    res, soft = trx.detect_demod(d_iq, d_p, sps=1, soft_stride=200, slice_bits=False)
    torch.cuda.synchronize()
    for b in range(n):
        r2, s2 = trx.detect_demod(d_iq[b:b + 1], d_p[b:b + 1], sps=1, soft_stride=200, slice_bits=False)
        assert torch.equal(res[b:b + 1], r2) and torch.equal(soft[b:b + 1].view(torch.int32), s2.view(torch.int32)), b
    off = 0
    for m in (1, 15, 16, 17, 255, 257):
        sl = slice(off, off + m)
        r2, s2 = trx.detect_demod(d_iq[sl].contiguous(), d_p[sl].contiguous(), sps=1, soft_stride=200, slice_bits=False)
        assert torch.equal(res[sl], r2) and torch.equal(soft[sl].view(torch.int32), s2.view(torch.int32)), (m, off)
        off += m
    assert off <= n


# ------------------------------------------------------------------------------------------------
# generic 4 SPS, int16 and complex64: burst_pull_kernel<4, *, 10> and <4, *, 0>
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def generic_4sps(L, n=256):
    from osmo_trx_amd import synth
    iq_nb, p_nb, _ = synth.make_normal_bursts(n, "cpu", 4, seed=9100 + L, max_toa=30, delay_sym=(-2.0, 28.0))
    p_nb["max_toa"] = np.array([3, 30, 63, 112], dtype=np.uint16)[np.arange(n) % 4]
    iq_rb, p_rb, _ = synth.make_access_bursts(n, "cpu", seed=9200 + L, ext=True)
    iq, params = cat([(iq_nb, p_nb), (iq_rb, p_rb)])
    return I._fit(iq, L), params                                        # zero-padded to L, as the existing fuzz does


@pytest.mark.parametrize("L", (629, 640, 641, 1536))
def test_generic_4sps_lengths_int16_and_complex64(trx, L):
    """burst_pull_kernel<4, false / true, 10> (L 629, 640: ten prefetch registers per lane, the last one partly past the burst)
    and <4, false / true, 0> (L 641 and TRXHIP_MAX_BURST_LEN = 1536, where fewer waves fit the LDS): normal and access bursts,
    sliced and raw rows, bit-identical to the oracle; complex64 bit-identical to int16."""
    iq, params = generic_4sps(L)
    x = I.as_cf32(iq)
    for kw in (dict(soft_stride=148, slice_bits=True), dict(soft_stride=156, slice_bits=False)):
        o_res, o_soft = oracle(("gen4", L), iq, 4, params, **kw)
        assert (o_res["rc"] > 0).mean() >= 0.7 and (o_res["rc"] == O.EXT_RACH).sum() >= 200
        g_res, g_soft = run_gpu(trx, iq, params, 4, **kw)
        check_parity(g_res, g_soft, o_res, o_soft)
        c_res, c_soft = run_gpu(trx, x, params, 4, **kw)
        assert same_bits(c_res, g_res) and same_bits(c_soft, g_soft)
        oc_res, oc_soft = oracle(("gen4", L), x, 4, params, **kw)
        check_parity(c_res, c_soft, oc_res, oc_soft)


def test_burst_longer_than_the_limit_is_refused(trx):
    """pull_common(): burst_len = TRXHIP_MAX_BURST_LEN + 1 is TRXHIP_EINVAL on both entry points, nothing is launched."""
    from osmo_trx_amd.trxhip import FLAG_SLICE
    hdr = open(os.path.join(O.ROOT, "include", "trxhip.h")).read()
    einval = int(re.search(r"#define\s+TRXHIP_EINVAL\s+\((-?\d+)\)", hdr).group(1))
    L = int(re.search(r"#define\s+TRXHIP_MAX_BURST_LEN\s+(\d+)", hdr).group(1)) + 1
    assert L == 1537
    p = torch.zeros((2, 8), dtype=torch.uint8, device="cuda:0")
    res = torch.full((2, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    soft = torch.empty((2, 148), dtype=torch.float32, device="cuda:0")
    for fn, iq in ((trx.L.trxhip_detect_demod_batch, torch.zeros((2, L, 2), dtype=torch.int16, device="cuda:0")),
                   (trx.L.trxhip_detect_demod_batch_cf32, torch.zeros((2, L), dtype=torch.complex64, device="cuda:0"))):
        rc = fn(trx.h, trx._dev(iq), trx._dev(p), trx._dev(res), trx._dev(soft), 2, L, 4, 4.0, 32767.0, 148, FLAG_SLICE, trx._stream())
        assert rc == einval
    torch.cuda.synchronize()
    assert (res == 0xA5).all()


# ------------------------------------------------------------------------------------------------
# complex64 into the 4-SPS kernel: burst_pull4_kernel<true, exact, common>, L 624..628
# ------------------------------------------------------------------------------------------------
LENS_K4 = (624, 625, 628)
# name -> (exact, slice_bits, soft_stride).  At L = 625 "fused_148" is the COMMON instance, elsewhere the plain fused one.
K4_INSTANCES = {
    "fused_148": (False, True, 148),
    "fused_raw156": (False, False, 156),
    "fused_444": (False, True, 444),
    "fused_100": (False, True, 100),
    "exact_148": (True, True, 148),          # complex64 + exact: 12 waves per workgroup
    "exact_raw156": (True, False, 156),
}
K4_THREE = ("fused_148", "fused_raw156", "exact_148")                      # fused-common (at 625) / fused / exact
K4_SCALED = K4_THREE + ("fused_444",)                                      # ... and whole 8-PSK rows through the fused demodulator
MAX_TOA_K4 = np.array([3, 30, 63, 64, 65, 112], dtype=np.uint16)           # 64 / 65: the narrow correlation buffer's limit


def check_k4(inst, g_res, g_soft, o_res, o_soft):
    """check_parity with the instance's bars: exact bit-identical; fused TRXHIP_FUSED_SOFT_ATOL, _8PSK on rows detected as EDGE."""
    if K4_INSTANCES[inst][0]:
        check_parity(g_res, g_soft, o_res, o_soft)
        return
    edge = o_res["rc"] == O.EDGE
    for m, atol in ((~edge, FUSED_SOFT_ATOL), (edge, FUSED_SOFT_ATOL_8PSK)):
        if m.any():
            check_parity(g_res[m], g_soft[m], o_res[m], o_soft[m], soft_atol=atol, sliced=K4_INSTANCES[inst][1])


@functools.lru_cache(None)
def nb_access_k4(L):
    """384 normal bursts (all TSCs x max_toa 3 / 30 / 63 / 64 / 65 / 112) + 64 RACH + 64 EXT_RACH."""
    from osmo_trx_amd import synth
    iq_nb, p_nb, _ = synth.make_normal_bursts(384, "cpu", 4, seed=10100, max_toa=30, delay_sym=(-2.0, 28.0))
    p_nb["max_toa"] = MAX_TOA_K4[(np.arange(384) // 8) % 6]                 # burst i: TSC i % 8 -- all 48 pairs
    iq_r, p_r, _ = synth.make_access_bursts(64, "cpu", seed=10200)
    iq_x, p_x, _ = synth.make_access_bursts(64, "cpu", seed=10300, ext=True)
    iq, params = cat([(iq_nb, p_nb), (iq_r, p_r), (iq_x, p_x)])
    return I._fit(iq, L), params


@functools.lru_cache(None)
def mixed_k4(L):
    """1024 bursts: nb_access_k4 + the 7:1 mix with OFF / IDLE slots and invalid TSCs + 8-PSK bursts in EDGE slots."""
    from osmo_trx_amd import synth
    iq_a, p_a = nb_access_k4(L)
    iq_m, p_m = synth.make_mixed_bursts(256, "cpu", seed=10400)
    p_m = synth.make_idle_off_mix(p_m)
    p_m["tsc"][9::32] = 9
    iq_e, p_e, _ = synth.make_edge_bursts(256, "cpu", seed=10500)
    p_e["type"][7::16] = O.TSC
    iq, params = cat([(iq_a, p_a), (I._fit(iq_m, L), p_m), (I._fit(iq_e, L), p_e)])
    return iq, params


@pytest.mark.parametrize("inst", list(K4_INSTANCES))
@pytest.mark.parametrize("L", LENS_K4)
def test_k4_complex64_integer_valued(trx, L, inst):
    """burst_pull4_kernel<true, exact, common>: complex64 samples that are the int16 samples' values.  Records and rows
    bit-identical to the int16 entry point with the normal-burst kernel split off (for the COMMON launch also with the split
    on, the header's own claim), then against the oracle with the instance's bars."""
    exact, sl, stride = K4_INSTANCES[inst]
    iq, params = mixed_k4(L)
    kw = dict(soft_stride=stride, slice_bits=sl)
    o_res, o_soft = oracle(("k4mix", L), iq, 4, params, **kw)
    assert set(np.unique(o_res["rc"])) >= {-3, 0, O.TSC, O.EXT_RACH, O.RACH, O.EDGE} and (o_res["rc"] > 0).sum() >= 800
    c_res, c_soft = run_gpu(trx, I.as_cf32(iq), params, 4, exact=exact, **kw)
    try:
        trx.set_nb_kernel(False)
        g_res, g_soft = run_gpu(trx, iq, params, 4, exact=exact, **kw)
    finally:
        trx.set_nb_kernel(True)
    assert same_bits(c_res, g_res) and same_bits(c_soft, g_soft)
    if inst == "fused_148" and L == 625:
        s_res, s_soft = run_gpu(trx, iq, params, 4, exact=False, **kw)
        assert same_bits(c_res, s_res) and same_bits(c_soft, s_soft)
    check_k4(inst, c_res, c_soft, o_res, o_soft)


# scale -> (float32 factor, full_scale, dither seed).  Powers of two are exact in float32 and keep every intermediate finite and
# normal: samples 1 .. 32768 become 9e-13 .. 3e-8 (squares >= 8e-25, sums <= 1e-12) at 2^-40 and 1e6 .. 3.4e10 (squares and
# their sums <= 1e24) at 2^20, far inside 1.2e-38 .. 3.4e38, so every float operation scales exactly and nothing may change
# but the exponents.  3e-4 with dither is an ordinary non-integer input.
# One thing in the reference is not scale-free: computePeakRatio() adds 1e-5 to the rms it divides by (sigProcLib.cpp:1568).  With
# amplitudes 0.015 .. 1 (2^-15) that changes no decision of this batch; at 2^-30 (5e-7 .. 3e-5) it decides most; at 2^-40 the
# ratio is ~1e-4 and the reference detects nothing at all -- so there "as many detections as unscaled" cannot hold for the
# oracle, and the case checks that the kernels find nothing either (their energy, RSSI and clip flag still against the oracle).
K4_SCALES = {
    "2^-15": (2.0 ** -15, 1.0, None),
    "2^-30": (2.0 ** -30, 32768.0 * 2.0 ** -30, None),
    "2^-40": (2.0 ** -40, 32768.0 * 2.0 ** -40, None),
    "2^20": (2.0 ** 20, 32768.0 * 2.0 ** 20, None),
    "3e-4_dither": (3e-4, 32768.0 * 3e-4, 11),
}


@pytest.mark.parametrize("scale", list(K4_SCALES))
@pytest.mark.parametrize("L", LENS_K4)
def test_k4_complex64_scaled(trx, L, scale, capsys):
    """burst_pull4_kernel<true, exact, common>, fused-common / fused (raw 156, rows of 444) / exact, on inputs only complex64 can
    express: the mixed batch of the integer-valued test (normal, access, 7:1 mix with OFF / IDLE / invalid slots, 8-PSK) times 2^-15 with full_scale 1.0 (what sigProcLib-signature callers present), times 2^-30, 2^-40 and 2^20 (K4_SCALES says
    what the reference's arithmetic makes of them), and times 3e-4 with sub-LSB dither (non-integer values).  Against
    O.pull_batch_cf32 with the same full_scale: rc / TSC / flags / TOA identical everywhere; exact: amp and soft bits bit-identical; fused: the header's bars.  The FAST detector's re-run rate is printed (no
    bar)."""
    factor, full_scale, dither = K4_SCALES[scale]
    iq, params = mixed_k4(L)
    x = I.as_cf32(iq, factor, dither)
    na = len(nb_access_k4(L)[1])                                            # the count conditions: the normal / access part
    for inst in K4_SCALED:
        exact, sl, stride = K4_INSTANCES[inst]
        kw = dict(soft_stride=stride, slice_bits=sl, full_scale=full_scale)
        o_res, o_soft = oracle(("k4scaled", L, scale), x, 4, params, **kw)
        n_det, n_edge = int((o_res["rc"][:na] > 0).sum()), int((o_res["rc"] == O.EDGE).sum())
        u_res, _ = oracle(("k4scaled", L, "1"), I.as_cf32(iq), 4, params, soft_stride=stride, slice_bits=sl)
        u_det = int((u_res["rc"][:na] > 0).sum())
        if scale == "2^-40":
            assert (o_res["rc"] <= 0).all()                                 # sigProcLib.cpp:1568, see K4_SCALES
        elif scale == "2^-30":
            assert 0.2 * na <= n_det < u_det
        else:
            assert n_det >= 0.85 * na and n_edge >= 200                     # EDGE rows reach the fused 8-PSK path
            if dither is None:
                assert n_det == u_det and np.array_equal(o_res["toa"], u_res["toa"]) and np.array_equal(o_res["rc"] > 0, u_res["rc"] > 0)
        trx.fast_stats(reset=True)
        g_res, g_soft = run_gpu(trx, x, params, 4, exact=exact, **kw)
        st = trx.fast_stats(reset=True)
        check_k4(inst, g_res, g_soft, o_res, o_soft)
        with capsys.disabled():
            n_all = int((o_res["rc"] > 0).sum())
            print(f"\n[k4 cf32 x {scale}, L {L}, {inst}] oracle: {n_det}/{na} normal / access bursts, {n_edge} EDGE, {n_all}/{len(params)} "
                  f"in all detected; {st['reruns']} TOA searches re-run ({st['reruns'] / max(1, n_all):.2%} of detected)")


CLIP_TARGETS = (np.float32(30000.0), np.nextafter(np.float32(30000.0), np.float32(np.inf)), np.float32(30000.5), np.float32(29999.99))


@functools.lru_cache(None)
def clip_edge_k4(L, n=64):
    """Per target, n bursts (half normal bursts, half noise that nothing detects) whose largest component is exactly the target:
    maxAmplitude() > 30000 (sigProcLib.cpp:1711-1722, :1746) is a strict compare on float samples."""
    from osmo_trx_amd import synth
    xs, ps = [], []
    for k, target in enumerate(CLIP_TARGETS):
        iq_b, p_b, _ = synth.make_normal_bursts(n // 2, "cpu", 4, seed=11100 + k, p_noise=0.0, p_clip=0.0)
        iq_n, p_n, _ = synth.make_normal_bursts(n // 2, "cpu", 4, seed=11200 + k, p_noise=1.0)
        iq, params = cat([(iq_b, p_b), (iq_n, p_n)])
        x = torch.view_as_real(I.as_cf32(I._fit(iq, L), 1.0, dither=k + 1)).clone()
        for b in range(n):
            flat = x[b].reshape(-1)
            j = int(flat.abs().argmax())
            sign = 1.0 if flat[j] >= 0 else -1.0
            flat *= 0.999 * float(target) / float(flat[j].abs())
            flat[j] = sign * float(target)
        xs.append(torch.view_as_complex(x))
        ps.append(params)
    return torch.cat(xs), np.concatenate(ps)


@pytest.mark.parametrize("L", LENS_K4)
def test_k4_complex64_clip_edge(trx, L):
    """burst_pull4_kernel<true, *, *>: the clip test on float samples.  Largest component exactly 30000.0 and 29999.99 (no clip),
    nextafter(30000) and 30000.5 (clip): the flag, and -SIGERR_CLIP on the undetected ones, equal the oracle's in all instances."""
    x, params = clip_edge_k4(L)
    n = len(params) // len(CLIP_TARGETS)
    for inst in K4_THREE:
        exact, sl, stride = K4_INSTANCES[inst]
        o_res, o_soft = oracle(("k4clip", L), x, 4, params, soft_stride=stride, slice_bits=sl)
        assert np.array_equal(o_res["clip"].reshape(len(CLIP_TARGETS), n).mean(axis=1), [0, 1, 1, 0])
        assert (o_res["rc"] == -O.SIGERR_CLIP).sum() >= n // 2 and (o_res["rc"] == 0).sum() >= n // 2 and (o_res["rc"] > 0).sum() >= n
        g_res, g_soft = run_gpu(trx, x, params, 4, exact=exact, soft_stride=stride, slice_bits=sl)
        check_k4(inst, g_res, g_soft, o_res, o_soft)


UNIT_THRESHOLD = 2.5      # a normal burst with one component zero (or I = Q) keeps half its power: peak ratio below 4, above 2.5
UNIT_RATIOS = (2.0 ** 17, 2.0 ** 17 * (1.0 + 2.0 ** -10))                 # on the guard's threshold and just beyond it


@functools.lru_cache(None)
def unit_guard_k4(L, n=64):
    """Q = 0; I = Q; one component 2^17 and 2^17 (1 + 2^-10) times the other -- on every sample (the decimator's real taps keep a
    power-of-two ratio exact, so the decimated samples sit on the guard's threshold too) and on the 16 input samples behind one
    decimated sample inside the correlation window; normal and access bursts alternate."""
    from osmo_trx_amd import synth
    iq_nb, p_nb, _ = synth.make_normal_bursts(n, "cpu", 4, seed=12100, p_noise=0.0, p_clip=0.0)
    iq_rb, p_rb, _ = synth.make_access_bursts(n, "cpu", seed=12200, p_noise=0.0)
    iq_nb[1::2], p_nb[1::2] = iq_rb[1::2], p_rb[1::2]
    base = torch.view_as_real(I.as_cf32(I._fit(iq_nb, L)))
    xs = []
    q0 = base.clone()
    q0[:, :, 1] = 0.0
    xs.append(q0)
    eq = base.clone()
    eq[:, :, 1] = eq[:, :, 0]
    xs.append(eq)
    for ratio in UNIT_RATIOS:
        every = base.clone()
        every[:, :, 1] = every[:, :, 0] / np.float32(ratio)
        xs.append(every)
        one = base.clone()
        for b in range(n):
            # decimated sample i = sum_k x[4i - 15 + k] g[k]: these 16 input samples put exactly one decimated sample, inside
            # the normal-burst and the access-burst correlation windows, on the ratio
            i = 64 + b % 16
            one[b, 4 * i - 15:4 * i + 1, 1] = one[b, 4 * i - 15:4 * i + 1, 0] / np.float32(ratio)
        xs.append(one)
    x = torch.view_as_complex(torch.cat(xs).contiguous())
    return x, np.concatenate([p_nb] * len(xs))


@pytest.mark.parametrize("L", LENS_K4)
def test_k4_complex64_unit_correlation_guard(trx, L):
    """burst_pull4_kernel<true, *, *>: the addition-only correlation's guard (a component more than 2^17 times the other, on the
    decimated samples) with ratios int16 input cannot reach: exactly 2^17 (safe) and 2^17 (1 + 2^-10) (unsafe), infinite (Q = 0)
    and 1 (I = Q).  Fused and exact against the oracle."""
    x, params = unit_guard_k4(L)
    for inst in K4_THREE:
        exact, sl, stride = K4_INSTANCES[inst]
        o_res, o_soft = oracle(("k4unit", L), x, 4, params, soft_stride=stride, slice_bits=sl, threshold=UNIT_THRESHOLD)
        assert ((o_res["rc"] > 0).reshape(-1, 64).sum(axis=1) >= 32).all()
        assert (o_res["rc"][:64] == O.TSC).sum() >= 8 and (o_res["rc"][:64] == O.RACH).sum() >= 8
        g_res, g_soft = run_gpu(trx, x, params, 4, exact=exact, soft_stride=stride, slice_bits=sl, threshold=UNIT_THRESHOLD)
        check_k4(inst, g_res, g_soft, o_res, o_soft)


@pytest.mark.parametrize("inst", K4_THREE)
def test_k4_complex64_results_do_not_depend_on_the_batch_size(trx, inst):
    """burst_pull4_kernel<true, exact, common> at L = 625: 16 waves per workgroup fused, 12 with complex64 + exact, so the LDS
    carve and the prefetch registers differ per instance.  A 12288-burst mixed complex64 batch in slices of 1, 15, 16, 17, 255,
    257 and 4097 equals the whole-batch launch (no oracle call: the one larger batch of this file)."""
    from osmo_trx_amd import synth
    exact, sl, stride = K4_INSTANCES[inst]
    n = 12288
    iq, params = synth.make_mixed_bursts(n, "cuda:0", seed=13100)
    params["type"][5::64] = O.OFF
    params["type"][9::64] = O.IDLE
    x = torch.view_as_complex(iq.to(torch.float32) * (2.0 ** -15))
    d_p = trx.params_tensor(params)
    kw = dict(sps=4, soft_stride=stride, slice_bits=sl, exact=exact, full_scale=1.0)
    res, soft = trx.detect_demod(x, d_p, **kw)
    torch.cuda.synchronize()
    off = 0
    for m in (1, 15, 16, 17, 255, 257, 4097):
        s = slice(off, off + m)
        r2, s2 = trx.detect_demod(x[s].contiguous(), d_p[s].contiguous(), **kw)
        assert torch.equal(res[s], r2) and torch.equal(soft[s].view(torch.int32), s2.view(torch.int32)), (inst, m, off)
        off += m
    assert off <= n
