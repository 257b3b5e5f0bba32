"""The reference's FCCH frequency-offset estimator, restated literally in numpy.  Nothing is imported from the product.

    gsm_fcch_offset()      ms/sch.c:282-314
    ac_sum_with_lag()      ms/sch.c:273-279
    pinv()                 ms/sch.c:262-270
    FCCH_TAIL_BITS_LEN, L1, L2, N1, N2, GSM_SYM_RATE   ms/sch.c:206, :255-258, :83

sch.c cannot be compiled on its own (it needs libosmocore's headers) and the oracle does not hold it, so this model is pinned by
reading the source: every line below names the line it restates, with the reference's types -- `float` locals, double wherever
M_PI (a double) enters an expression, fs as a float, expected_fcch_val from 67700 (not 67708.33).

One restatement with the accumulator type of ac_sum_with_lag() as a parameter:
    acc=np.float32   `complex float v`, the 92 products added one after the other in the reference's order, every product and
                     sum rounded to float32 (generic C, FLT_EVAL_METHOD 0, no contraction)
    acc=np.float64   the same sums without their rounding error: the yardstick the device, which adds in another order, is
                     measured against
Not restated, as in the product: the call of org_gsm_fcch_offset() (:305: its value is discarded, and it multiplies the caller's
burst by a reference tone in place) and the len > GSM_MAX_BURST_LEN clamp (:289-290: no effect at 625).
mag_one, mag_two and energy are the product's own fields (the reference has no validity test); they are defined here as the
product defines them."""
import math

import numpy as np

F = np.float32
START = 3 * 4 + 10 * 4                 # FCCH_TAIL_BITS_LEN + 10 * 4, :206, :292
L1, L2, N1, N2 = 3, 32, 92, 92         # :255-258
FIRST, LAST = START, START + L2 + N2 - 1            # the samples read: 52 .. 175
GSM_SYM_RATE = (1625e3 / 6) * 4        # :83
FS = F(13. / 48. * 1e6 * 4)            # const float fs, :286
EXPECTED_FCCH_VAL = F(((2 * math.pi) / float(FS)) * 67700)      # const float, double arithmetic, :287
TONE_HZ = 1625e3 / 6 / 4               # the FCCH tone: 67 708.33 Hz above the carrier


def scaled(iq, rx_full_scale=2047.0):
    """convert_and_scale by 1.f / rxFullScale (ms_upper.cpp:203): int16[..., 2] or complex64[...] -> complex64[...]; complex64
    samples are multiplied by the same factor, as the product's receiver does"""
    scale = F(1.0) / F(rx_full_scale)
    iq = np.asarray(iq)
    if iq.dtype == np.int16:
        return (iq[..., 0].astype(F) * scale + 1j * (iq[..., 1].astype(F) * scale)).astype(np.complex64)
    assert iq.dtype == np.complex64, iq.dtype
    return ((iq.real * scale) + 1j * (iq.imag * scale)).astype(np.complex64)


def pinv(P):
    """:262-270: the first (i, j) with P == L2 * i - L1 * j, or the caller's (0, 0)"""
    for i in range(L1):
        for j in range(L2):
            if P == L2 * i - L1 * j:
                return i, j
    return 0, 0


def roundf(x):
    """C's roundf: halves away from zero"""
    return int(math.copysign(math.floor(abs(float(x)) + 0.5), float(x)))


def ac_sum(x, lag, acc):
    """:273-279: v += in[s + offset + lag] * conjf(in[s + offset]) for s < N, in order.  Returns (re, im) in `acc`, and
    S = sum |a| |b| in float64"""
    a = x[START + lag:START + lag + N1]
    b = x[START:START + N1]
    ar, ai, br, bi = (v.astype(acc) for v in (a.real, a.imag, b.real, b.imag))
    pr = (ar * br).astype(acc) + (ai * bi).astype(acc)             # (ar + i ai) * (br - i bi), every operation rounded to acc
    pi = (ai * br).astype(acc) - (ar * bi).astype(acc)
    re = np.add.accumulate(pr.astype(acc), dtype=acc)[-1]          # accumulate IS the sequential sum
    im = np.add.accumulate(pi.astype(acc), dtype=acc)[-1]
    S = float(np.sum(np.abs(a.astype(np.complex128)) * np.abs(b.astype(np.complex128))))
    return re, im, S


def fcch_offset(x, acc=np.float64):
    """gsm_fcch_offset() on x: complex64[>= 176] scaled samples (scaled()).  Returns a dict: the product's record fields (hz,
    alpha_one, alpha_two, mag_one, mag_two, energy, p, r, s) and, for the tests' bounds, S_one, S_two (sum |a| |b| of each
    autocorrelation), E (the energy sum in float64) and P_unrounded"""
    x = np.asarray(x, dtype=np.complex64)
    re1, im1, S1 = ac_sum(x, L1, acc)
    re2, im2, S2 = ac_sum(x, L2, acc)
    alpha_one = F(np.arctan2(im1, re1))                            # float alpha = cargf(v), :278, :293-294
    alpha_two = F(np.arctan2(im2, re2))
    lin = F(F(F(L1) * alpha_two) - F(F(L2) * alpha_one))           # int * float and float - float are float
    P_unrounded = F(float(lin) / (2 * math.pi))                    # / double, stored to float, :296
    P = roundf(P_unrounded)                                        # :297
    r, s = pinv(P)                                                 # :299-300
    omegal1 = F((float(alpha_one) + 2 * math.pi * r) / L1)         # double, stored to float, :302
    omegal2 = F((float(alpha_two) + 2 * math.pi * s) / L2)         # :303
    mid = F(EXPECTED_FCCH_VAL - F(F(omegal1 + omegal2) / F(2)))    # float arithmetic
    reval = F(GSM_SYM_RATE / (2 * math.pi) * float(mid))           # double * float, stored to float, :308
    w = x[START:START + N1].astype(np.complex128)
    E = float(np.sum(w.real * w.real + w.imag * w.imag))
    return dict(hz=F(-reval), alpha_one=alpha_one, alpha_two=alpha_two,             # return -reval, :313
                mag_one=F(math.hypot(float(re1), float(im1))), mag_two=F(math.hypot(float(re2), float(im2))), energy=F(E),
                p=P, r=r, s=s, S_one=S1, S_two=S2, E=E, P_unrounded=float(P_unrounded))


def tone(cfo_hz, amp, phase, n=625):
    """complex128[n]: the FCCH tone of a carrier cfo_hz off, at 4 samples per symbol"""
    k = np.arange(n)
    return amp * np.exp(1j * (2 * math.pi * (TONE_HZ + cfo_hz) / GSM_SYM_RATE * k + phase))


def to_i16(y):
    """int16[..., 2]: the samples rounded and clipped, as a radio would deliver them"""
    return np.stack([np.round(y.real), np.round(y.imag)], axis=-1).clip(-32768, 32767).astype(np.int16)


# ---- the bounds of the tests, derived (not measured) ------------------------------------------------------------------
# A 92-term float sum in any order errs by <= 92 * 2^-23 * S, so the angle of v_L moves by <= d_alpha_L = 92 * 2^-23 * S_L / |v_L|
# (where that is small; it is meaningless, and the bar wide open, where |v_L| is not well above the error), and
# hz = fs / (4 pi) * (omegal1 + omegal2) + const moves by <= fs / (4 pi) * (d_alpha_1 / 3 + d_alpha_2 / 32): 0.32 and 0.03 Hz per
# unit of S / |v|; a few ulps of hz (0.004 at 45 kHz) make the constant.
EPS_SUM = 92 * 2.0 ** -23


def d_alpha(m, which):
    S, mag = (m["S_one"], float(m["mag_one"])) if which == 1 else (m["S_two"], float(m["mag_two"]))
    return EPS_SUM * S / mag if mag > 0 else math.inf


def hz_bar(m):
    r1 = m["S_one"] / float(m["mag_one"]) if m["mag_one"] > 0 else math.inf
    r2 = m["S_two"] / float(m["mag_two"]) if m["mag_two"] > 0 else math.inf
    return 0.02 + 0.32 * r1 + 0.03 * r2


def decision_margin(m):
    """how far P_unrounded is from a half-integer, minus what the sums' error can move it: > 0 means (p, r, s) is decided"""
    dist = abs(abs(m["P_unrounded"] - math.floor(m["P_unrounded"])) - 0.5)
    return dist - (3 * d_alpha(m, 2) + 32 * d_alpha(m, 1)) / (2 * math.pi)
