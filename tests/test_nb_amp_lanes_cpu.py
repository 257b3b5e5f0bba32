"""Block TAIL of the normal-burst kernel forms 1 / amp per LANE (tools/gen_nb_asm.py, amp_lane; csrc/trx_tables.h,
trx_amp_lane_coef): lane l takes the pair (A, B) of its variant l & 3 from a table staged per training sequence, forms its own
component comp = fl(fl(xr A) + fl(xi B)) of amp = peak * (1 / gain), the norm n = fl(comp^2) + the quad neighbour's
fl(comp^2), and VP = fl(comp * rcp(n)).  Before, every lane formed the whole wave-uniform amp (Complex.h:74), |amp|^2 =
fl(im^2) + fl(re^2), and picked VP[l & 3] = (sx, sy, -sx, -sy) by two selects.

A float32 numpy model of both forms, on random and edge values of (xr, xi, g0, g1): comp and n are compared as BITS, variant by
variant (rcp is not modelled: its input is what is compared).  One case is not the same bits and is pinned down here as what it
is: where a component of amp cancels to an exact zero, -(a - b) is -0 and (-a) + b is +0.  The output stage multiplies a
zero VP into a product that is a zero of either sign and adds the other product onto it, and the slicer's fma(d, 0.5, 0.5)
takes a zero of either sign to 0.5: the model runs that stage on both forms, zeros among the filter's sums included, and
compares the soft bits as bits.

The staged (A, B) table is checked entry by entry against the blob's header, all eight sequences; the header's function is
compiled for the host and called through ctypes.  The tap at the peak of block DETB's interpolation (its chain now starts as
a product: the argument in the generator wants that weight positive for every fraction) is checked on the blob's sinc LUT.
No GPU."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from osmo_trx_amd import trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "osmo_trx_amd", "csrc")
SRC = """
#include <cstddef>
#include "trx_tables.h"
extern "C" float coef(float g0, float g1, int k) { return trx_amp_lane_coef(g0, g1, k); }
extern "C" int seq_size(void) { return (int)sizeof(trx_seq); }
extern "C" int seq0_off(void) { return (int)(offsetof(trx_tables, seq) + TRX_SEQ_TSC0 * sizeof(trx_seq)); }
extern "C" int gain_inv_off(void) { return (int)offsetof(trx_seq, gain_inv); }
extern "C" int sincv_off(void) { return (int)offsetof(trx_tables, sincv); }
extern "C" int swz(int q) { return trx_sincv_swz(q); }
"""
F = np.float32
# (A, B) by lane & 3 for (g0, g1) = 1 / gain, as the issue of this change states them
PAIRS = (lambda g0, g1: (g0, -g1), lambda g0, g1: (-g1, -g0), lambda g0, g1: (-g0, g1), lambda g0, g1: (g1, g0))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or "g++"                           # (the host compiler of osmo_trx_amd/build.py)
    d = tmp_path_factory.mktemp("amplanes")
    (d / "amplanes.cpp").write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(d / "libamplanes.so"), str(d / "amplanes.cpp")], check=True, capture_output=True)
    so = ctypes.CDLL(str(d / "libamplanes.so"))
    so.coef.restype = ctypes.c_float
    so.coef.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_int]
    return so


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64 (one rounding of the sum to 53 bits in front of the one to 24:
    both forms go through the same function, and the inputs here are far from its double-rounding cases' measure)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


@pytest.fixture(scope="module")
def inputs():
    """(xr, xi, g0, g1) float32 arrays: random values over twelve decades and signs, then every combination of the edge values"""
    rng = np.random.default_rng(1601)
    n = 200000
    mag = lambda: (10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    rnd = [mag(), mag(), mag(), mag()]
    # large ratios between the components
    rnd[1][: n // 4] *= F(1e-9)
    rnd[0][n // 4: n // 2] *= F(1e-9)
    rnd[3][n // 2: 3 * n // 4] *= F(1e-9)
    edge = np.array([0.0, -0.0, 1.0, -1.0, 3.0, -3.0, 0.75, 1e-12, -1e12, 2.5e6, 1.0000001, -0.33333334], dtype=F)
    grid = np.stack(np.meshgrid(edge, edge, edge, edge, indexing="ij"), -1).reshape(-1, 4)
    # exact cancellation of a component: xr g0 == xi g1 (amp.re = 0) and xr g1 == -xi g0 (amp.im = 0), powers of two and not
    canc = np.array([[2, 4, 8, 4], [3, 3, 5, 5], [1, -1, 1, -1], [6, 3, 1, 2], [2, 4, 4, -2], [5, 5, 7, -7], [0, 3, 2, 0], [3, 0, 0, 2]],
                    dtype=F)
    allv = np.concatenate([np.stack(rnd, -1), grid, canc])
    return [np.ascontiguousarray(allv[:, k]) for k in range(4)]


def old_form(xr, xi, g0, g1):
    """every lane: amp = peak * (1 / gain) (Complex.h:74), |amp|^2; what VP[v] multiplies the reciprocal with, by variant"""
    a0, a1, a2, a3 = xr * g0, xr * g1, xi * g1, xi * g0
    re, im = a0 - a2, a1 + a3
    n = im * im + re * re
    return [re, -im, -re, im], n


def new_form(xr, xi, g0, g1):
    comp = []
    for v in range(4):
        a, b = PAIRS[v](g0, g1)
        comp.append(xr * a + xi * b)
    sq = [c * c for c in comp]
    return comp, [sq[v] + sq[v ^ 1] for v in range(4)]


def test_component_and_norm_by_lane_residue(inputs):
    xr, xi, g0, g1 = inputs
    with np.errstate(over="ignore", invalid="ignore"):
        want, n_old = old_form(xr, xi, g0, g1)
        comp, n_new = new_form(xr, xi, g0, g1)
    ok = np.isfinite(n_old)                                         # (an overflow is an overflow in both forms: not compared)
    assert ok.sum() > 200000
    zero_seen = 0
    for v in range(4):
        assert np.array_equal(bits(n_new[v])[ok], bits(n_old)[ok]), v
        same = bits(comp[v]) == bits(want[v])
        # the one case that is not the same bits: a component that cancels to an exact zero keeps +0 where the negated form had -0
        diff = ok & ~same
        assert (comp[v][diff] == 0).all() and (want[v][diff] == 0).all(), (v, np.flatnonzero(diff)[:8])
        assert v in (1, 2) or not diff.any(), v                     # (the variants that are not negated: bits, zeros included)
        zero_seen += int(diff.sum())
    assert zero_seen > 0                                            # (the inputs hold that case)


def test_a_zero_of_either_sign_reaches_no_soft_bit(inputs):
    """the output stage (block DEMOD): d = fma(VP[b], z.y, fl(VP[a] z.x)), soft = clamp(fma(d, 0.5, 0.5)) -- on both forms' VP,
    with one stand-in for the reciprocal (its input has the same bits), for filter sums that hold zeros of both signs"""
    xr, xi, g0, g1 = inputs
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        want, n_old = old_form(xr, xi, g0, g1)
        comp, _ = new_form(xr, xi, g0, g1)
        r = F(1.0) / n_old
        ok = np.isfinite(r) & np.isfinite(n_old)
        rng = np.random.default_rng(1602)
        zs = [F(0.0), F(-0.0), F(1.5), F(-2.25), rng.standard_normal(len(xr)).astype(F)]
        for a in range(4):
            b = (a + 3) & 3                                         # z.x * VP[k] + z.y * VP[k - 1]
            for zx in zs:
                for zy in zs:
                    zx_, zy_ = np.broadcast_to(zx, xr.shape).astype(F), np.broadcast_to(zy, xr.shape).astype(F)
                    out = []
                    for vp in (want, comp):
                        d = fma32(vp[b] * r, zy_, (vp[a] * r) * zx_)
                        out.append(np.clip(fma32(d, np.full_like(d, 0.5), np.full_like(d, 0.5)), 0, 1))
                    fin = ok & np.isfinite(out[0])
                    assert np.array_equal(bits(out[0])[fin], bits(out[1])[fin]), (a, zx, zy)


def test_staged_table_against_the_header(lib):
    """float k of sequence t's row (trx_kernel_nb.hip: lamp[8 t + k] = trx_amp_lane_coef(gain_inv.re, gain_inv.im, k)): A of
    variant k for k < 4, B of variant k - 4 behind -- what a lane reads 16 bytes apart"""
    blob = trxhip.generate_tables_host()
    for t in range(8):
        off = lib.seq0_off() + t * lib.seq_size() + lib.gain_inv_off()
        g0, g1 = np.frombuffer(blob, dtype="<f4", count=2, offset=off)
        assert g0 != 0 or g1 != 0
        row = [F(lib.coef(g0, g1, k)) for k in range(8)]
        for v in range(4):
            a, b = PAIRS[v](g0, g1)
            assert bits(row[v]) == bits(a) and bits(row[4 + v]) == bits(b), (t, v)
    # and on values whose negation shows in the bits of a zero
    for g0, g1 in ((0.0, 2.0), (-0.0, -3.0), (1.5, 0.0)):
        for v in range(4):
            a, b = PAIRS[v](F(g0), F(g1))
            assert bits(F(lib.coef(g0, g1, v))) == bits(a) and bits(F(lib.coef(g0, g1, 4 + v))) == bits(b)


def test_the_tap_at_the_peak_has_a_positive_weight(lib):
    """block DETB, chain p1: tap fl takes sincv[swz(f)], f = 0 .. 511 (row 0 of the LUT)"""
    blob = trxhip.generate_tables_host()
    sincv = np.frombuffer(blob, dtype="<f4", count=4096, offset=lib.sincv_off())
    w = np.array([sincv[lib.swz(f)] for f in range(512)])
    assert w[0] == 1.0 and (w > 0).all(), float(w.min())


def test_the_generator_emits_what_is_committed(tmp_path):
    """osmo_trx_amd/csrc/trx_nb_asm.inc is tools/gen_nb_asm.py's output (its hazard checker passes: it exits otherwise)"""
    spec = importlib.util.spec_from_file_location("gen_nb_asm", os.path.join(ROOT, "tools", "gen_nb_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = tmp_path / "trx_nb_asm.inc"
    m.main(str(out))
    assert out.read_text() == open(os.path.join(CSRC, "trx_nb_asm.inc")).read()
