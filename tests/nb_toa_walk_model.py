"""Host-side model of the TOA search of detectBurst() (sigProcLib.cpp:1649-1709) for 4-SPS normal bursts, in float64, for
tests/test_gpu_nb_toa_walk.py: the correlation window, its arg-max, the early / late decision of EVERY node of the two rounds of
peakDetect()'s bisection (:1141-1186) -- the masks the normal-burst kernel's blocks DETA / DETB walk, in position order --, the
reference's path through them and the final position.  The model says which leaf each round ends at and whether a round's
decisions are monotone in position (n times "right", then "left": the kernel's first-zero form) or not (its level-by-level
walk); that it is the search the kernels run is checked by the test, on the TOA they report.

Also the test's two-ray bursts: a normal burst through two paths a fraction of a symbol to a few symbols apart."""
import math

import numpy as np
import torch

import oracle_lib as O
from osmo_trx_amd import synth

HEAD, TARGET = 10, 3 + 58 + 16 + 5                                      # analyzeTrafficBurst (:1887-1904)
START = TARGET - HEAD - 1


def node_offset(n, inc0):
    """trx_device.h node_offset(): earlyIndex offset (1/512 symbol) of heap node n of a subtree whose first step is inc0"""
    lv = (n + 1).bit_length() - 1
    p = n + 1 - (1 << lv)
    return ((4 * p * inc0) >> lv) - (2 * inc0 - ((2 * inc0) >> lv))


def correlation(iq, tsc, length):
    """downsampleBurst (:1587-1601) and the correlation with the midamble (:1674): complex128[n, length]"""
    t = O.tables()
    x = iq[:, :624, 0].astype(np.float64) + 1j * iq[:, :624, 1].astype(np.float64)
    g = t["dec_taps"].astype(np.float64)
    xp = np.concatenate([np.zeros((len(x), 15)), x, np.zeros((len(x), 16))], axis=1)      # xp[j + 15] = x[j]
    dec = np.zeros((len(x), 156), np.complex128)
    for k in range(16):
        dec += xp[:, k:k + 4 * 156:4] * g[k]                                            # x[4 i - 15 + k]
    seq = np.stack([np.asarray(t["midamble"][s]["seq"], np.complex128) for s in range(8)])[tsc]      # [n, 16]
    corr = np.zeros((len(x), length), np.complex128)
    for k in range(16):
        corr += dec[:, START - 15 + k:START - 15 + k + length] * seq[:, k:k + 1]
    return corr


def interp_power(corr, pos512):
    """|interpolatePoint(corr, position)|^2 (:1100-1118) at positions in 1/512 symbol: int64[n, m] -> float64[n, m]"""
    sinc = O.tables()["sinc_table"].astype(np.float64)
    n, size = corr.shape
    fl = pos512 >> 9
    acc = np.zeros(pos512.shape, np.complex128)
    rows = np.arange(n)[:, None]
    for d in range(-10, 11):
        i = fl + d
        ok = (i >= np.maximum(fl - 10, 0)) & (i < np.minimum(fl + 11, size - 1))
        dist = np.abs(i * 512 - pos512)                                  # |i - ix| * 512; the LUT's index is floor(|i - ix| * 128)
        w = np.where(ok & (dist < 8 * 512), sinc[np.minimum(dist >> 2, 1024)], 0.0)
        acc += corr[rows, np.clip(i, 0, size - 1)] * w
    return acc.real ** 2 + acc.imag ** 2


def bisection_round(corr, early512, levels, inc0):
    """All nodes of one round: (leaf, monotone, margin) -- the reference's path over the decisions, whether the decisions read in
    position order are n times right then left, and the smallest gap |E - L| / (E + L + 2 m) over the round's nodes, m the
    arg-max power: the kernel certifies a decision when its float32 gap exceeds TRX_FAST_KAPPA = 6e-6 times that sum (trx_device.h)"""
    nodes = (1 << levels) - 1
    off = np.array([node_offset(h, inc0) for h in range(nodes)])
    pe = interp_power(corr, early512[:, None] + off[None, :])
    pl = interp_power(corr, early512[:, None] + off[None, :] + 1024)
    right = pe < pl                                                     # heap order
    p = np.zeros(len(corr), np.int64)
    for k in range(levels):
        p = 2 * p + right[np.arange(len(corr)), p + (1 << k) - 1]
    order = np.argsort(off)                                             # position order
    r = right[:, order]
    ones = r.sum(axis=1)
    monotone = (r == (np.arange(nodes)[None, :] < ones[:, None])).all(axis=1)
    assert (p[monotone] == ones[monotone]).all()                        # the first-zero form's leaf IS the path's
    m = (corr.real ** 2 + corr.imag ** 2).max(axis=1)[:, None]
    margin = (np.abs(pe - pl) / np.maximum(pe + pl + 2 * m, 1e-300)).min(axis=1)
    return p, monotone, margin


def toa_search(iq, params):
    """-> dict of per-burst arrays: bidx (arg-max lag), leaf_a, leaf_b, mono_a, mono_b, margin_a, margin_b (bisection_round),
    pos512 (final position in 1/512 symbol)"""
    n = len(params)
    out = {k: np.zeros(n, np.int64) for k in ("bidx", "leaf_a", "leaf_b", "pos512")}
    out.update({k: np.zeros(n, bool) for k in ("mono_a", "mono_b")})
    out.update({k: np.zeros(n) for k in ("margin_a", "margin_b")})
    for mt in np.unique(params["max_toa"]):
        rows = np.flatnonzero(params["max_toa"] == mt)
        corr = correlation(iq[rows], params["tsc"][rows].astype(np.int64), 16 + int(mt))
        bidx = (corr.real ** 2 + corr.imag ** 2).argmax(axis=1)
        e = (bidx - 1) * 512
        la, ma, ga = bisection_round(corr, e, 5, 256)
        e = e + 32 * la - 496
        lb, mb, gb = bisection_round(corr, e, 4, 8)
        for k, v in (("bidx", bidx), ("leaf_a", la), ("leaf_b", lb), ("mono_a", ma), ("mono_b", mb), ("margin_a", ga), ("margin_b", gb),
                     ("pos512", e + 2 * lb - 15 + 512)):
            out[k][rows] = v
    return out


def make_two_ray_bursts(n, seed, max_toa=3, gap_sym=(0.3, 2.5), rel_amp=(0.6, 1.5), snr_db=35.0, delay_sym=(1.0, 3.0)):
    """Normal bursts (TSC i % 8) through two paths: the first `delay_sym` symbols late with amplitude a, the second a further
    +-gap symbols away with amplitude a * rel_amp and a phase of its own.  -> (iq int16[n, 625, 2] on the CPU, params)"""
    gen = synth._gen(seed, "cpu")
    params = np.zeros(n, dtype=synth.PARAMS_DTYPE)
    params["type"] = synth.T_TSC
    params["max_toa"] = max_toa
    params["tsc"] = (np.arange(n) % 8).astype(np.uint8)
    bits = synth.normal_burst_bits(n, torch.from_numpy(params["tsc"].copy()), gen, "cpu")
    wave = synth.modulate_laurent_4sps(bits)
    u = torch.rand((6, n), generator=gen)
    amp = 2000.0 + 8000.0 * u[0]
    d1 = delay_sym[0] + (delay_sym[1] - delay_sym[0]) * u[1]
    gap = (gap_sym[0] + (gap_sym[1] - gap_sym[0]) * u[2]) * torch.where(u[3] < 0.5, -1.0, 1.0)
    a2 = amp * (rel_amp[0] + (rel_amp[1] - rel_amp[0]) * u[4])
    base = synth.BASE_TOA[4]
    y = synth._frac_delay(wave, (d1 - base) * 4) * torch.polar(amp, 2 * math.pi * u[5])[:, None]
    ph2 = torch.rand(n, generator=gen) * (2 * math.pi)
    y = y + synth._frac_delay(wave, (d1 + gap - base) * 4) * torch.polar(a2, ph2)[:, None]
    sigma = amp * 10.0 ** (-snr_db / 20.0) / math.sqrt(2.0)
    out = torch.view_as_real(y) + torch.randn((n, wave.shape[1], 2), generator=gen) * sigma[:, None, None]
    return torch.round(out).clamp_(-32768, 32767).to(torch.int16).contiguous(), params
