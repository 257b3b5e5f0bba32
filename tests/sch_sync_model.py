"""CPU model of the MS-side SCH receiver, the live branch of ms_trx::handle_sch() (Transceiver52M/ms/ms_rx_lower.cpp:157-205):
convert_and_scale, get_sch_chan_imp_resp / get_sch_buffer_chan_imp_resp (grgsm_vitac/grgsm_vitac.cpp:283-309) over
get_chan_imp_resp (:183-235), the clamp (ms_rx_lower.cpp:173-175), detect_burst_nb (:82-119) and decode_sch
(ms_rx_lower.cpp:59-100) over gsm_sch_decode / gsm_sch_parse / gsm_sch_to_fn (ms/sch.c:141-204).

Everything is float32 in the reference's operand order, statement by statement: std::complex's a * b is spelled out as
(ar*br - ai*bi, ar*bi + ai*br), the division by (length, 0) is component-wise, abs() is hypotf and std::pow(float, int) is
pow in double.  Loops whose order decides a result are explicit; the correlation taps are vectorised ACROSS lags and add their
terms in the reference's order.  The 16-state MLSE itself is oracle_lib.va_viterbi (pinned to the reference-compiled
viterbi_detector.cc by tests/test_oracle.py).

Two points where the reference is undefined are defined here, and in the product the same way:
  * a sample in front of the buffer (ACQ with a window in the first 188 lags: burst start < 0) reads as zero;
  * the convolutional decoder's survivor rule on metric ties (libosmocore's osmo_conv_decode is not restated): a candidate
    replaces the survivor only when strictly smaller, candidates visited by ascending predecessor state.
"""
import numpy as np

import oracle_lib as O

F = np.float32
OSR = 4                          # d_OSR, grgsm_vitac.h:63
CIR = 5                          # CHAN_IMP_RESP_LENGTH
FL = CIR * OSR
BURST = 148                      # BURST_SIZE
TRAIN_BEGINNING = 5
SYNC_POS = 3 + 39                # constants.h:53
SYNC_SEARCH_RANGE = 30           # grgsm_vitac.h:62
ONE_TS_BURST_LEN = 625           # ms.h:50
TRACK, ACQ = 0, 1

# 3GPP TS 45.002 5.2.5: the 64 extended training bits of the synchronisation burst (SYNC_BITS, constants.h:70-75)
SYNC_BITS = np.array([int(c) for c in "1011100101100010000001000000111100101101010001010111011000011011"], dtype=np.uint8)
ACCESS_BITS = np.array([int(c) for c in "01001011011111111001100110101010001111000"], dtype=np.uint8)


def gmsk_map(bits, start):
    """gmsk_mapper() (grgsm_vitac.cpp:125-146) followed by conj (:61-62): a walk over {1, j, -1, -j}."""
    out = np.zeros(len(bits), dtype=np.complex64)
    out[0] = start
    prev = 2 * int(bits[0]) - 1
    for i in range(1, len(bits)):
        cur = 2 * int(bits[i]) - 1
        enc = cur * prev
        out[i] = np.complex64(1j) * np.complex64(enc) * out[i - 1]
        prev = cur
    return np.conj(out)


def sch_seq():
    """&d_sch_training_seq[TRAIN_BEGINNING], N_SYNC_BITS - 2 * TRAIN_BEGINNING = 54 elements (:288-289)."""
    return gmsk_map(SYNC_BITS, -1j)[TRAIN_BEGINNING:64 - TRAIN_BEGINNING]


def acc_seq():
    return gmsk_map(ACCESS_BITS, -1j)[TRAIN_BEGINNING:41 - TRAIN_BEGINNING]


def norm_seq(tsc_bits):
    start = 1.0 if int(tsc_bits[0]) == 0 else -1.0
    return gmsk_map(tsc_bits, start)[TRAIN_BEGINNING:26 - TRAIN_BEGINNING]


def quarter_codes(seq):
    """2-bit codes of a {1, j, -1, -j} sequence (0: 1, 1: j, 2: -1, 3: -j), element k at bits 2k, 2k+1."""
    v = 0
    for k, s in enumerate(seq):
        c = {(1, 0): 0, (0, 1): 1, (-1, 0): 2, (0, -1): 3}[(int(round(s.real)), int(round(s.imag)))]
        v |= c << (2 * k)
    return v


def take(x, idx):
    """x[idx] with zeros outside [0, len(x))."""
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < len(x))
    out = np.zeros(idx.shape, dtype=np.complex64)
    out[ok] = x[idx[ok]]
    return out


def _cmul(ar, ai, br, bi):
    """std::complex<float> operator*, all float32"""
    return (ar * br - ai * bi).astype(F), (ar * bi + ai * br).astype(F)


def correlate(seq, x, lags):
    """correlate_sequence() (:148-156) for every lag of `lags` at once; the terms ii = 0 .. len-1 are added in order."""
    lags = np.asarray(lags)
    re = np.zeros(len(lags), dtype=F)
    im = np.zeros(len(lags), dtype=F)
    for ii in range(len(seq)):
        xv = take(x, lags + ii * OSR)
        tr, ti = _cmul(F(seq[ii].real), F(seq[ii].imag), xv.real.astype(F), xv.imag.astype(F))
        re = (re + tr).astype(F)
        im = (im + ti).astype(F)
    # conj(result) / gr_complex(length, 0): the complex division the compiler expands in line, (a + jb) / (c + jd) with |c| >= |d|:
    # ratio = d / c = 0, ((a + b * ratio) / c, (b - a * ratio) / c).  The values are a / c and b / c; the products with zero only
    # decide the sign of an exact zero (an imaginary sum that cancels gives -0.0 where a >= 0 and +0.0 where a < 0)
    n, ratio, b = F(len(seq)), F(0), (-im).astype(F)
    return ((re + b * ratio) / n).astype(F), ((b - re * ratio) / n).astype(F)


def get_chan_imp_resp(x, start_pos, stop_pos, seq):
    """get_chan_imp_resp() (:183-235).  Returns (search_start_pos + strongest_window_nr, cir complex64[20], corr_max)."""
    nw = stop_pos - start_pos
    cre, cim = correlate(seq, x, start_pos + np.arange(nw))
    mag = np.hypot(cre, cim).astype(F)                               # abs(): hypotf
    power = (mag.astype(np.float64) ** 2).astype(F)                  # std::pow(float, int): pow in double (:199)
    ws = F(0)
    for i in range(FL):                                              # :206-208
        ws = F(ws + power[i])
    energy = [ws]
    for i in range(FL, nw):                                          # :212-215
        ws = F(ws + F(power[i] - power[i - FL]))
        energy.append(ws)
    best = 0                                                         # std::max_element: the first largest
    for i in range(1, len(energy)):
        if energy[best] < energy[i]:
            best = i
    corr_max = F(0)
    for ii in range(FL):                                             # :220-226
        if mag[best + ii] > corr_max:
            corr_max = mag[best + ii]
    cir = np.zeros(FL, dtype=np.complex64)                           # part by part: a + 1j * b turns an imaginary -0.0 into +0.0,
    cir.real, cir.imag = cre[best:best + FL], cim[best:best + FL]    # which the reference's conj() of an exact zero sum is
    return start_pos + best, cir, corr_max


def detect_burst(x, cir, burst_start, nbits=BURST, start_state=3):
    """detect_burst_generic() (:82-103) without the final mapping: the Viterbi detector's float outputs."""
    cr, ci = cir.real.astype(F), cir.imag.astype(F)
    rt = np.zeros(FL, dtype=np.complex64)
    for k in range(FL - 1, -1, -1):                                  # autocorrelation() :159-166
        ar, ai = F(0), F(0)
        for i in range(k, FL):
            tr, ti = _cmul(cr[i], ci[i], cr[i - k], F(-ci[i - k]))
            ar, ai = F(ar + tr), F(ai + ti)
        rt[k] = complex(ar, ai)
    rhh = np.conj(rt[::OSR]).astype(np.complex64)                    # :94-95
    n = np.arange(nbits)
    fr = np.zeros(nbits, dtype=F)
    fi = np.zeros(nbits, dtype=F)
    for ii in range(FL):                                             # mafi() :168-181
        live = n * OSR + ii < nbits * OSR                            # "if ((a + ii) >= nitems * d_OSR) break"
        xv = take(x, burst_start + n * OSR + ii)
        tr, ti = _cmul(xv.real.astype(F), xv.imag.astype(F), cr[ii], ci[ii])
        fr = np.where(live, (fr + tr).astype(F), fr)
        fi = np.where(live, (fi + ti).astype(F), fi)
    filt = (fr + 1j * fi).astype(np.complex64)
    return O.va_viterbi(filt, rhh, start_state)


def scale_samples(iq, scale):
    """convert_and_scale(): every component times `scale`.  iq: int16[n, 2] or complex64[n]."""
    iq = np.asarray(iq)
    if iq.dtype == np.int16:
        v = iq.astype(F)
        re, im = v[:, 0], v[:, 1]
    else:
        re, im = iq.real.astype(F), iq.imag.astype(F)
    s = F(scale)
    return ((re * s).astype(F) + 1j * (im * s).astype(F)).astype(np.complex64)


# ---- decode_sch() -------------------------------------------------------------------------------------------------
CONV_INF = 1 << 24


def conv_output(state, u):
    """3GPP TS 45.003 4.7: c(2k) = u(k) + u(k-3) + u(k-4), c(2k+1) = u(k) + u(k-1) + u(k-3) + u(k-4); state bit i = u(k-1-i)
    (the trellis of sch_next_output / sch_next_state, sch.c:60-72)."""
    b0, b2, b3 = state & 1, (state >> 2) & 1, (state >> 3) & 1
    return u ^ b2 ^ b3, u ^ b0 ^ b2 ^ b3


def conv_encode(u):
    out, s = [], 0
    for b in u:
        c0, c1 = conv_output(s, int(b))
        out += [c0, c1]
        s = ((s << 1) | int(b)) & 15
    return np.array(out, dtype=np.uint8)


def conv_decode(sbits):
    """39 steps from state 0, flushed to state 0, for one burst (78 sbits) or a batch [N, 78].  Integer metrics: a coded 0
    expects +127, a coded 1 expects -127, the cost is |x - e| summed.  Survivor of state n: the candidate from predecessor
    n >> 1 first, the one from (n >> 1) + 8 only when strictly smaller.  Steps in an explicit loop; states and bursts vectorised."""
    x = np.atleast_2d(np.asarray(sbits)).astype(np.int64)
    N = x.shape[0]
    n = np.arange(16)
    preds = (n >> 1, (n >> 1) + 8)
    exp = []
    for p in preds:
        c = [conv_output(int(pp), int(nn) & 1) for pp, nn in zip(p, n)]
        exp.append((np.array([-127 if c0 else 127 for c0, _ in c]), np.array([-127 if c1 else 127 for _, c1 in c])))
    pm = np.full((N, 16), CONV_INF, dtype=np.int64)
    pm[:, 0] = 0
    dec = np.zeros((39, N, 16), dtype=np.int64)
    for k in range(39):
        x0, x1 = x[:, 2 * k, None], x[:, 2 * k + 1, None]
        c = [pm[:, preds[j]] + np.abs(x0 - exp[j][0]) + np.abs(x1 - exp[j][1]) for j in (0, 1)]
        d = c[1] < c[0]
        pm = np.where(d, c[1], c[0])
        dec[k] = d
    u = np.zeros((N, 39), dtype=np.uint8)
    s = np.zeros(N, dtype=np.int64)
    rows = np.arange(N)
    for k in range(38, -1, -1):
        u[:, k] = s & 1
        s = (s >> 1) + 8 * dec[k][rows, s]
    return u[0] if np.ndim(sbits) == 1 else u


def crc10(info):
    """The 10 parity bits of gsm0503_sch_crc10: generator D^10 + D^8 + D^6 + D^5 + D^4 + D^2 + 1, remainder inverted, MSB first."""
    reg = 0
    for b in info:
        reg ^= int(b) << 9
        reg = ((reg << 1) ^ 0x175) if reg & 0x200 else (reg << 1)
        reg &= 0x3ff
    reg ^= 0x3ff
    return np.array([(reg >> (9 - i)) & 1 for i in range(10)], dtype=np.uint8)


def sch_parse(info):
    """gsm_sch_parse() (sch.c:162-185) over sch_packed_info (:41-49): t1_hi[2] bsic[6] t1_md[8] t3p_hi[2] t2[5] t1_lo t3p_lo."""
    i = [int(b) for b in info]
    bsic = sum(i[2 + k] << k for k in range(6))
    t1 = i[23] | sum(i[8 + k] << (1 + k) for k in range(8)) | (i[0] << 9) | (i[1] << 10)
    t2 = sum(i[18 + k] << k for k in range(5))
    t3p = i[24] | (i[16] << 1) | (i[17] << 2)
    return bsic, t1, t2, t3p


def sch_to_fn(t1, t2, t3p):
    """gsm_sch_to_fn() (sch.c:142-159).  Returns (fn, whether the t3 < t2 branch was taken)."""
    t3 = t3p * 10 + 1
    if t3 < t2:
        tt = (t3 + 26) - t2
    else:
        tt = (t3 - t2) % 26
    return t1 * 51 * 26 + tt * 51 + t3, t3 < t2


def decode_sch(bits):
    """decode_sch() (ms_rx_lower.cpp:59-100) on the 148 demodulated sbits.  Returns dict(rc, fn, t1, bsic, t2, t3p)."""
    data = np.concatenate([bits[3:42], bits[106:145]])               # :66-67
    u = conv_decode(data)
    if not np.array_equal(crc10(u[:25]), u[25:35]):
        return dict(rc=0, fn=-1, t1=0, bsic=0, t2=0, t3p=0)
    bsic, t1, t2, t3p = sch_parse(u[:25])
    fn, _ = sch_to_fn(t1, t2, t3p)
    return dict(rc=1, fn=fn, t1=t1, bsic=bsic, t2=t2, t3p=t3p)


def sch_sync(iq, mode, scale):
    """handle_sch() (ms_rx_lower.cpp:157-179) for one buffer.  Returns dict(rc, start, corr_max, fn, t1, bsic, t2, t3p, bits)."""
    x = scale_samples(iq, scale)
    seq = sch_seq()
    center = SYNC_POS + TRAIN_BEGINNING
    if mode == TRACK:
        x = x[:ONE_TS_BURST_LEN]                                     # :160, zeros around it (:162, :164)
        pos, cir, cm = get_chan_imp_resp(x, (center - 10) * OSR, (center + SYNC_SEARCH_RANGE) * OSR, seq)
        start = pos - center * OSR
        start = start if start < 39 else 39                          # :174-175
        start = start if start > -39 else -39
    else:
        pos, cir, cm = get_chan_imp_resp(x, 0, len(x) - 64 * 8, seq)
        start = pos - center * OSR
    out = detect_burst(x, cir, start)
    bits = np.where(out > 0, -127, 127).astype(np.int8)              # "pre flip bits!" (:101-102)
    r = decode_sch(bits)
    r.update(start=start, corr_max=cm, bits=bits)
    return r
