"""Inputs for the MLSE receivers and what the reference's compiled code makes of them (test infrastructure).

The inputs are int16 IQ: the int16 entry points take them as they are, the float paths take x.astype(float32) * scale with the
path's own scale (SCALE_BTS: scaleVector's 1 / 16383 of Transceiver.cpp:783; SCALE_MS: convert_and_scale's 1 / rxFullScale).
The records come from oracle_lib.ref_vitac(), the reference's grgsm_vitac.cpp + viterbi_detector.cc compiled unmodified.
tests/golden/make_vitac_vectors.py stores one seeded set in tests/golden/ref_vitac_vectors.npz; tests/test_vitac_ref_cpu.py runs
the restatements against the stored set and, where the compiled reference is present, against freshly seeded ones."""
import numpy as np

import ms_rx_cases as K
import oracle_lib as O
import sch_sync_model as M
import sch_util
from osmo_trx_amd import synth

F = np.float32
SLOT = 625
SCALE_BTS = O.VA_SCALE
MS_FULL_SCALE = 2047.0
SCALE_MS = F(1.0) / F(MS_FULL_SCALE)
TRAIN_POS = 3 + 57 + 1 + 5                                   # constants.h: TRAIN_POS
NB_SEARCH = ((TRAIN_POS - 5) * 4 + 1, (TRAIN_POS + 5 + 5) * 4)   # get_norm_chan_imp_resp's window (grgsm_vitac.cpp:268-269)
NB_DELAYS = (0, 1, 7, 13, 20, 21)                            # samples, as the BTS-side buffer sees a burst (tests/test_oracle.py)
NB_EARLY = (-14, -9)                                         # the slot begins inside the burst: raw starts below 0 (MS side)
NOISE_SCALES = (3.0, 3000.0)
AB_START_STATES = (0, 3, 12, 15)                             # from 16 on the reference stores out of bounds
AB_SYNC = np.array([int(c) for c in "01001011011111111001100110101010001111000"], dtype=np.uint8)
AB_TAIL = np.array([0, 0, 1, 1, 1, 0, 1, 0], dtype=np.uint8)
ACQ_LEN = 64 * 8 + 20                                        # the shortest buffer trxhip_sch_sync_batch_* takes in ACQ mode
SCH_OFFSETS_PLAIN = (0, 3, 10, 17, 25, 33, 39, 45, 60, 100)  # sch_util.sch_burst: random payload
SCH_OFFSETS_CODED = (-44, -20, -5, 12)                       # ms_rx_cases.sch_slot: a decodable BSIC / FN, the slot may begin inside it


def tsc_bits(tsc):
    """The 26 training bits of 3GPP TS 45.002 5.2.3, this project's table."""
    return np.array([int(c) for c in synth.TSC_BITS[tsc]], dtype=np.uint8)


def noise(rng, n, scale):
    return ((rng.normal(size=n) + 1j * rng.normal(size=n)) * scale).astype(np.complex64)


def to_x(iq, scale):
    """int16[n, 2] -> complex64[n]: every component converted, then times scale."""
    return M.scale_samples(np.asarray(iq, dtype=np.int16), scale)


def to_cf(iq):
    """int16[..., 2] -> complex64[...], unscaled: what the complex64 entry points are given."""
    v = np.asarray(iq, dtype=np.int16).astype(F)
    return (v[..., 0] + 1j * v[..., 1]).astype(np.complex64)


def normal_slots(rng, per_tsc_delays=NB_DELAYS, early=()):
    """Per TSC: one noise-only slot per NOISE_SCALES, then one burst per delay (SNR 3 .. 35 dB, amplitude 10^2.5 .. 10^4.2).  The
    delays of `early` replace the first len(early) delays for odd TSCs.  Returns dict(iq int16[n, 625, 2], tsc, kind (0 noise,
    1 burst), delay, bits uint8[n, 148] sent (zero on noise slots))."""
    iq, tsc, kind, delay, bits = [], [], [], [], []
    for t in range(8):
        for s in NOISE_SCALES:
            iq.append(K.to_i16(noise(rng, SLOT, s)))
            tsc.append(t)
            kind.append(0)
            delay.append(0)
            bits.append(np.zeros(148, np.uint8))
        delays = list(per_tsc_delays)
        if t % 2:
            delays[:len(early)] = early
        for d in delays:
            b = K.nb_bits(rng, t)
            y = K.place(rng, O.modulate_burst(b, 8, 4), int(d), float(rng.uniform(3, 35)), float(10 ** rng.uniform(2.5, 4.2)))
            iq.append(K.to_i16(y))
            tsc.append(t)
            kind.append(1)
            delay.append(d)
            bits.append(b)
    return dict(iq=np.stack(iq), tsc=np.array(tsc, np.uint8), kind=np.array(kind, np.uint8), delay=np.array(delay, np.int32),
                bits=np.stack(bits))


def access_slots(rng, n):
    """n access-burst slots, every sixth noise only, start states cycling through AB_START_STATES.
    Returns dict(iq int16[n, 625, 2], ss)."""
    iq, ss = [], []
    for b in range(n):
        if b % 6 == 5:
            y = noise(rng, SLOT, NOISE_SCALES[(b // 6) % 2])
        else:
            bits = np.concatenate([AB_TAIL, AB_SYNC, rng.integers(0, 2, 36, dtype=np.uint8), np.zeros(3, np.uint8)])
            y = K.place(rng, O.modulate_burst(bits, 8, 4), int(rng.integers(0, 26)), float(rng.uniform(3, 35)),
                        float(10 ** rng.uniform(2.5, 4.0)))
        iq.append(K.to_i16(y))
        ss.append(AB_START_STATES[b % 4])
    return dict(iq=np.stack(iq), ss=np.array(ss, np.uint8))


def sch_slots(rng, plain=SCH_OFFSETS_PLAIN, coded=SCH_OFFSETS_CODED):
    """Synchronisation bursts across get_sch_chan_imp_resp's search range (raw starts -40 .. 100, clamped to +-39 behind it),
    then one noise-only slot per NOISE_SCALES.  Returns dict(iq int16[n, 625, 2], off; -1000 on a noise slot, sent int32[n, 2]: the BSIC and
    frame number a coded burst carries, -1 elsewhere)."""
    iq, off, sent = [], [], []
    for o in plain:
        amp = float(10 ** rng.uniform(2.5, 4.0))
        y, _ = sch_util.sch_burst(rng, SLOT, int(o), amp=amp, noise=amp * 10 ** (-float(rng.uniform(3, 35)) / 20) / np.sqrt(2))
        iq.append(K.to_i16(y))
        off.append(o)
        sent.append((-1, -1))
    for o in coded:
        bsic, fn = int(rng.integers(0, 64)), int(synth.random_sch_frames(1, rng)[0])
        y = K.sch_slot(rng, bsic, fn, int(o), float(rng.uniform(10, 35)), float(10 ** rng.uniform(2.5, 4.0)))
        iq.append(K.to_i16(y))
        off.append(o)
        sent.append((bsic, fn))
    for s in NOISE_SCALES:
        iq.append(K.to_i16(noise(rng, SLOT, s)))
        off.append(-1000)
        sent.append((-1, -1))
    return dict(iq=np.stack(iq), off=np.array(off, np.int32), sent=np.array(sent, np.int32))


def acq_buffers(rng, n, length=ACQ_LEN):
    """n buffers for get_sch_buffer_chan_imp_resp: the search covers lags 0 .. length - 513 and a burst at offset o has its
    window near lag o + 188, so the burst begins in front of the buffer.  Returns int16[n, length, 2]."""
    out = []
    for b in range(n):
        amp = float(10 ** rng.uniform(2.5, 4.0))
        y = noise(rng, length, amp * 10 ** (-float(rng.uniform(10, 30)) / 20) / np.sqrt(2))
        w = O.modulate_burst(synth.sch_burst_bits(int(rng.integers(0, 64)), int(synth.random_sch_frames(1, rng)[0])), 8, 4)
        o = -188 + int(rng.integers(0, max(length - 512 - 19, 1)))
        w = w * np.complex64(amp * np.exp(1j * rng.uniform(0, 2 * np.pi)))
        lo, hi = max(o, 0), min(o + len(w), length)
        y[lo:hi] += w[lo - o:hi - o]
        out.append(K.to_i16(y))
    return np.stack(out)


def tie_slots():
    """Slots whose window energies tie exactly at the maximum, so std::max_element's rule (the first largest) decides the burst
    start: an all-zero slot, and single impulses (every fourth lag has the same power, every window five of them) inside the
    normal-burst and the access-burst search.  Returns dict(iq int16[3, 625, 2], tsc)."""
    iq = np.zeros((3, SLOT, 2), dtype=np.int16)
    iq[1, 300] = (1000, 0)
    iq[2, 60] = (0, -1000)
    return dict(iq=iq, tsc=np.array([0, 2, 5], np.uint8))


def clamp_ms(start):
    """ms_upper.cpp:224-225, ms_rx_lower.cpp:174-175"""
    return min(max(int(start), -39), 39)


# ---- what the compiled reference returns ----------------------------------------------------------------------------------------
def ref_normal(R, iq, tsc, scale, ms, seq=None):
    """get_norm_chan_imp_resp + detect_burst_nb(.., 3) on one slot at `scale`; the burst start handed on is max(start, 0) on the
    BTS side (Transceiver.cpp:627-629) and the start clamped to +-39 on the MS side.  With `seq` (16 elements) the same compiled
    get_chan_imp_resp is given that sequence over get_norm_chan_imp_resp's window.  Returns (raw start, cir, corr_max, sbits[148])."""
    x = to_x(iq, scale)
    if seq is None:
        start, cir, cm = R.norm_imp_resp(x, tsc)
    else:
        pos, cir, cm = R.chan_imp_resp(x, NB_SEARCH[0], NB_SEARCH[1], seq)
        start = pos - TRAIN_POS * 4
    return start, cir, cm, R.detect_burst_nb(x, cir, clamp_ms(start) if ms else max(start, 0), 3)


def ref_tsc1_3gpp_seq(R):
    """The compiled gmsk_mapper's mapping of the 3GPP TSC 1 bit string, conjugated, elements 5 .. 20 (initvita's recipe)."""
    b = tsc_bits(1)
    return np.conj(R.gmsk_mapper(b, 1.0 if b[0] == 0 else -1.0))[5:21].astype(np.complex64)


def tsc1_cost(R, rng, n):
    """What row 1 of the reference's table costs: n TSC 1 bursts (delays 0 .. 21 samples, SNR 3 .. 35 dB, amplitude 10^2.5 .. 10^4.2)
    through the BTS-side chain as the reference ships it and with the 3GPP row.  Returns int32[6]: wrong hard bits as shipped, wrong
    hard bits with the 3GPP row, bits sent, bursts whose start differs, bursts whose sbits differ, bursts."""
    seq = ref_tsc1_3gpp_seq(R)
    err_a = err_b = d_start = d_out = 0
    for _ in range(n):
        b = K.nb_bits(rng, 1)
        y = K.place(rng, O.modulate_burst(b, 8, 4), int(rng.integers(0, 22)), float(rng.uniform(3, 35)), float(10 ** rng.uniform(2.5, 4.2)))
        iq = K.to_i16(y)
        sa, _, _, oa = ref_normal(R, iq, 1, SCALE_BTS, False)
        sb, _, _, ob = ref_normal(R, iq, 1, SCALE_BTS, False, seq=seq)
        err_a += int(((oa < 0) != (b > 0)).sum())                    # -127 is a one
        err_b += int(((ob < 0) != (b > 0)).sum())
        d_start += int(sa != sb)
        d_out += int(not np.array_equal(oa, ob))
    return np.array([err_a, err_b, 148 * n, d_start, d_out, n], dtype=np.int32)


def ref_access(R, iq, ss):
    """get_access_imp_resp(.., 0) + max(start, 0) + detect_burst_ab(.., ss) at SCALE_BTS.  Returns (raw start, cir, corr_max, sbits[88])."""
    assert 0 <= int(ss) <= 15
    x = to_x(iq, SCALE_BTS)
    start, cir, cm = R.access_imp_resp(x, 0)
    return start, cir, cm, R.detect_burst_ab(x, cir, max(start, 0), int(ss))[:88]


def ref_sch_track(R, iq):
    """get_sch_chan_imp_resp + the clamp + detect_burst_nb(&ss[start], cir, 0, ..) at SCALE_MS (ms_rx_lower.cpp:171-177).
    corr_max is a local of get_sch_chan_imp_resp: it is taken from the compiled get_chan_imp_resp over the same window with the
    compiled sequence, whose start and taps must agree.  Returns (raw start, cir, corr_max, sbits[148])."""
    x = to_x(iq, SCALE_MS)
    start, cir = R.sch_imp_resp(x)
    c = M.SYNC_POS + M.TRAIN_BEGINNING
    pos, cir2, cm = R.chan_imp_resp(x, (c - 10) * 4, (c + M.SYNC_SEARCH_RANGE) * 4, R.training_seqs()[2][5:59])
    assert pos - c * 4 == start and cir2.tobytes() == cir.tobytes()
    return start, cir, cm, R.detect_burst_nb(x, cir, clamp_ms(start), 3)


def ref_sch_acq(R, iq):
    """get_sch_buffer_chan_imp_resp + detect_burst_nb(&ss[start], cir, 0, ..) at SCALE_MS.  Returns (start, cir, corr_max, sbits)."""
    x = to_x(iq, SCALE_MS)
    start, cir, cm = R.sch_buffer_imp_resp(x)
    return start, cir, cm, R.detect_burst_nb(x, cir, start, 3)


def expected_nb(v, side):
    """(raw start, cir, corr_max, sbits) of the normal slots as the project computes them: the reference's records, the TSC 1
    rows from the 3GPP-row records."""
    rec = [v[f"nb_{side}_{k}"].copy() for k in ("start", "cir", "corr_max", "out")]
    for a, k in zip(rec, ("start", "cir", "corr_max", "out")):
        a[v["tsc1b_rows"]] = v[f"tsc1b_{side}_{k}"]
    return rec


def records(fn, rows):
    """Stack the (start, cir, corr_max, sbits) of fn(row) for every row."""
    r = [fn(*row) for row in rows]
    return (np.array([a[0] for a in r], np.int32), np.stack([a[1] for a in r]).astype(np.complex64),
            np.array([a[2] for a in r], np.float32), np.stack([a[3] for a in r]).astype(np.int8))
