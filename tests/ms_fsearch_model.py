"""The MS-side FCCH search (include/trxhip.h, "MS-side FCCH search") restated in numpy: the oracle of the feature --
the reference has no such search.  Nothing is imported from the product; the measurement behind the search is
tests/ms_afc_model.py's.

    samples   x[n] = re + i im; int16 rows in int64 (every sum is exact), complex64 rows in float64
    p[n] = x[n + LAG] conj(x[n]),  e[n] = |x[n]|^2
    block b   sums of p and e over samples 16 b .. 16 b + 15; nb = (len - LAG) // 16 whole blocks
    window j  pos = 16 j, j + 36 <= nb:  Ra = blocks j .. j + 17,  Rb = blocks j + 18 .. j + 35 of p,  E = all 36 blocks of e
    score     4 (Ra.re Rb.re + Ra.im Rb.im) / (E E) in float64, in that order; E == 0 (and a NaN) gives 0
    answer    the first window with the largest score (strict >); found = score >= min_score
"""
import numpy as np

import ms_afc_model as AM

HOP, W, LAG = 16, 576, 8
BLOCKS, HALF = W // HOP, W // HOP // 2
MIN_LEN = W + LAG
SEG = 256                                  # windows per segment of the kernel: what the tests place their seams by
SLOT = 625
HIT_DTYPE = np.dtype([("found", "<i4"), ("pos", "<u4"), ("score", "<f8"), ("ra_re", "<f8"), ("ra_im", "<f8"), ("rb_re", "<f8"),
                      ("rb_im", "<f8"), ("energy", "<f8"), ("reserved", "<u8")])
assert HIT_DTYPE.itemsize == 64
SUMS = ("ra_re", "ra_im", "rb_re", "rb_im", "energy")


def parts(x):
    """(re, im) of int16[n, 2] as int64, of complex64[n] as float64"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x[:, 0].astype(np.int64), x[:, 1].astype(np.int64)
    assert x.dtype == np.complex64, x.dtype
    return x.real.astype(np.float64), x.imag.astype(np.float64)


def n_blocks(n):
    return (n - LAG) // HOP


def n_windows(n):
    return n_blocks(n) - BLOCKS + 1


def block_sums(x):
    """(p.re, p.im, e) per whole block"""
    re, im = parts(x)
    nb = n_blocks(len(re))
    a_re, a_im, b_re, b_im = re[LAG:LAG + nb * HOP], im[LAG:LAG + nb * HOP], re[:nb * HOP], im[:nb * HOP]
    p_re = a_re * b_re + a_im * b_im                               # x[n + LAG] conj(x[n])
    p_im = a_im * b_re - a_re * b_im
    e = b_re * b_re + b_im * b_im
    return tuple(v.reshape(nb, HOP).sum(axis=1) for v in (p_re, p_im, e))


def _run(v, first, count, n):
    """sums of `count` consecutive blocks from block j + first on, for the n windows j"""
    c = np.concatenate([np.zeros(1, v.dtype), np.cumsum(v)])
    if v.dtype == np.float64:                                      # (no prefix differences in floating point: sum the blocks)
        return np.array([v[j + first:j + first + count].sum() for j in range(n)])
    return c[first + count:first + count + n] - c[first:first + n]


def windows(x):
    """dict of per-window arrays: the five sums (int64 or float64) and score (float64)"""
    assert len(x) >= MIN_LEN, len(x)
    p_re, p_im, e = block_sums(x)
    n = len(e) - BLOCKS + 1
    w = dict(ra_re=_run(p_re, 0, HALF, n), ra_im=_run(p_im, 0, HALF, n), rb_re=_run(p_re, HALF, HALF, n), rb_im=_run(p_im, HALF, HALF, n),
             energy=_run(e, 0, BLOCKS, n))
    d = {k: w[k].astype(np.float64) for k in SUMS}
    with np.errstate(all="ignore"):
        score = 4.0 * (d["ra_re"] * d["rb_re"] + d["ra_im"] * d["rb_im"]) / (d["energy"] * d["energy"])
    score[(d["energy"] == 0) | np.isnan(score)] = 0.0
    w["score"] = score
    return w


def search(x, min_score, w=None):
    """the row's answer as a HIT_DTYPE record"""
    w = windows(x) if w is None else w
    j = int(np.argmax(w["score"]))                                 # the first of the largest: strict > from window 0 on
    hit = np.zeros((), dtype=HIT_DTYPE)
    hit["pos"], hit["score"], hit["found"] = HOP * j, w["score"][j], int(w["score"][j] >= min_score)
    for k in SUMS:
        hit[k] = float(w[k][j])
    return hit


def slot_at(x, pos):
    """the 625 samples the measurement is defined on, zeros behind the row's end (only pos + 52 .. pos + 175 are read)"""
    x = np.asarray(x)
    s = x[pos:pos + SLOT]
    if len(s) < SLOT:
        s = np.concatenate([s, np.zeros((SLOT - len(s),) + x.shape[1:], x.dtype)])
    return s


def measure(x, pos, rx_full_scale=2047.0, acc=np.float64):
    """ms_afc_model.fcch_offset() on the slot that begins at pos"""
    return AM.fcch_offset(AM.scaled(slot_at(x, pos), rx_full_scale), acc)


# ---- complex64 rows: the bar of the tests, derived ------------------------------------------------------------------------------
# A term of Ra / Rb is a b + c d with float32 factors: two products and a sum, each within 2^-24 relative, and |a b| + |c d| <=
# |x[n + LAG]| |x[n]|, so the term errs by <= 2 * 2^-24 of that (the sum's error applies to a value that is itself bounded by it).
# Adding 576 such terms in float32 in ANY order adds at most one rounding of a partial sum per level of the summation tree the
# kernel happens to have; a balanced tree over 576 terms is 10 levels deep, a chain of length k costs k.  The issue fixes the bar at
# 2^-19 = 32 * 2^-24 of S = sum |x[n + LAG]| |x[n]| over the sum's terms (sum |x[n]|^2 for the energy): room for the 2 of the term
# and 30 levels.  The kernel here adds 4 terms in a lane, 4 lanes by two exchanges (5 roundings), and everything above a block of 16
# in double: 7 * 2^-24 S, a quarter of the bar.

BAR = 2.0 ** -19


def bars(x):
    """per window: dict of S for each of the five sums, in float64"""
    re, im = parts(x)
    mag = np.hypot(re, im)
    nb = n_blocks(len(re))
    s = (mag[LAG:LAG + nb * HOP] * mag[:nb * HOP]).reshape(nb, HOP).sum(axis=1)
    e = (mag[:nb * HOP] ** 2).reshape(nb, HOP).sum(axis=1)
    n = nb - BLOCKS + 1
    sa, sb = _run(s, 0, HALF, n), _run(s, HALF, HALF, n)
    return dict(ra_re=sa, ra_im=sa, rb_re=sb, rb_im=sb, energy=_run(e, 0, BLOCKS, n))


def score_margin(x, w=None):
    """How far the best window's score stands above every other window's once each sum may move by its bar: > 0 means pos is
    decided.  d score <= 4 (|dRa| |Rb| + |Ra| |dRb| + |dRa| |dRb|) / E^2 + 2 score dE / E (first order in dE / E, which is 2^-19),
    with |dR| <= sqrt(2) BAR S for a complex sum whose two parts each move by BAR S."""
    w = windows(x) if w is None else w
    b = bars(x)
    ra, rb = np.hypot(w["ra_re"], w["ra_im"]), np.hypot(w["rb_re"], w["rb_im"])
    da, db = np.sqrt(2) * BAR * b["ra_re"], np.sqrt(2) * BAR * b["rb_re"]
    E = np.where(w["energy"] > 0, w["energy"], np.inf)
    ds = 4 * (da * rb + ra * db + da * db) / (E * E) + 2.5 * np.abs(w["score"]) * BAR
    j = int(np.argmax(w["score"]))
    others = np.delete(w["score"] + ds, j)
    return float(w["score"][j] - ds[j] - (others.max() if len(others) else -np.inf))
