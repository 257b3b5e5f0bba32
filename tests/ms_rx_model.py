"""CPU model of the MS-side downlink burst receiver: upper_trx::pullRadioVector() and the burst indication of driveReceiveFIFO()
(Transceiver52M/ms/ms_upper.cpp:161-304), one slot at a time, on the pieces of tests/sch_sync_model.py (float32 in the reference's
operand order; the MLSE is the oracle's).  An SCH slot is sch_sync_model.sch_sync(TRACK): what ms_trx::handle_sch() demodulates
whether or not the upper layer listens (ms_rx_lower.cpp:130-153).

Where the reference is undefined, the model and the product define the same:
  * an all-zero traffic slot (pow == 0: rxFullScale / 0 at :272) has rssi = 0 and the flag SILENT;
  * an FCCH slot ("return trash", :189-192) is an indication without content: flag TRASH, bits zero;
  * tn > 7, and a traffic slot with tsc > 7 (d_norm_training_seq has 8 rows + dummy), are BAD: nothing is done.
"""
import math

import numpy as np

import sch_sync_model as M
from osmo_trx_amd import synth

F = np.float32
KIND_BAD, KIND_FCCH, KIND_SCH, KIND_NB = 0, 1, 2, 3
IND_TRASH, IND_SILENT = 1, 2
TRAIN_POS = 3 + 57 + 1 + 5       # constants.h: the 16 middle bits of the training sequence start here
SLOT = M.ONE_TS_BURST_LEN


def slot_kind(fn, tn, tsc=0):
    """gsm_fcch_check_ts / gsm_sch_check_ts (ms/sch.c:133-139) as pullRadioVector asks them (:180-181)."""
    if tn > 7:
        return KIND_BAD
    if tn == 0 and fn % 51 in (0, 10, 20, 30, 40):                   # sch.c:100-114
        return KIND_FCCH
    if tn == 0 and fn % 51 in (1, 11, 21, 31, 41):                   # sch.c:117-131
        return KIND_SCH
    return KIND_NB if tsc <= 7 else KIND_BAD


def energy_detect(x, window=80):
    """energyDetect(sv, 20 * 4) (sigProcLib.cpp:1573-1585): energy += norm2() of samples 0, 4, ... one term at a time, / window.
    norm2() is i*i + r*r (Complex.h:113)."""
    energy = F(0.0)
    for i in range(window):
        s = x[4 * i]
        re, im = F(s.real), F(s.imag)
        energy = F(energy + F(F(im * im) + F(re * re)))
    return F(energy / F(window))


def rssi_value(pow_, rx_full_scale):
    """20.0 * log10(rxFullScale / avg) with avg = sqrt(pow) (:211, :272): an unsigned over a float is a float division, log10 and the
    product are double."""
    avg = F(np.sqrt(F(pow_)))
    return 20.0 * math.log10(float(F(F(rx_full_scale) / avg)))


def ms_rx(iq_slot, fn, tn, tsc, active, rx_full_scale=2047.0):
    """One slot: int16[625, 2] or complex64[625].  Returns dict(kind, sent, flags, rssi, rssi_exact, toa256, start, corr_max, pow,
    sch_fn, sch_rc, sch_bsic, bits int8[148])."""
    kind = slot_kind(fn, tn, tsc)
    r = dict(kind=kind, sent=0, flags=0, rssi=0, rssi_exact=None, toa256=0, start=0, corr_max=F(0), pow=F(0), sch_fn=-1, sch_rc=0,
             sch_bsic=0, bits=np.zeros(M.BURST, dtype=np.int8))
    scale = F(1.0) / F(rx_full_scale)                                # 1.f / float(rxFullScale) (:203)
    if kind == KIND_BAD:
        return r
    if kind == KIND_SCH:                                             # ms_rx_lower.cpp:157-205, then ms_upper.cpp:194-200
        s = M.sch_sync(np.asarray(iq_slot)[:SLOT], M.TRACK, scale)
        r.update(sent=1 if active else 0, rssi=10, start=s["start"], corr_max=s["corr_max"], bits=s["bits"], sch_rc=s["rc"],
                 sch_fn=s["fn"], sch_bsic=s["bsic"])
        return r
    if not active:                                                   # :186-187
        return r
    r["sent"] = 1
    if kind == KIND_FCCH:                                            # :189-192
        r["flags"] = IND_TRASH
        return r
    x = M.scale_samples(np.asarray(iq_slot)[:SLOT], scale)           # convert_and_scale (:203); zeros around it (:164-171)
    pow_ = energy_detect(x)                                          # :205
    seq = M.norm_seq([int(c) for c in synth.TSC_BITS[tsc]])
    # get_norm_chan_imp_resp (grgsm_vitac.cpp:265-274)
    pos, cir, cm = M.get_chan_imp_resp(x, (TRAIN_POS - 5) * M.OSR + 1, (TRAIN_POS + 5 + M.CIR) * M.OSR, seq)
    start = pos - TRAIN_POS * M.OSR
    start = start if start < 39 else 39                              # :224-225
    start = start if start > -39 else -39
    out = M.detect_burst(x, cir, start)                              # detect_burst_nb (:230): start state 3
    r.update(start=start, corr_max=cm, pow=pow_, bits=np.where(out > 0, -127, 127).astype(np.int8))
    if pow_ == 0:
        r["flags"] = IND_SILENT
    else:
        r["rssi_exact"] = rssi_value(pow_, rx_full_scale)
        r["rssi"] = int(math.floor(r["rssi_exact"]))                 # :272
    return r
