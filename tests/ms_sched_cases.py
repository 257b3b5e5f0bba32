"""Downlink sample streams of one cell for the tests of the MS-side slot scheduler (tests/test_ms_sched_cpu.py,
tests/test_gpu_ms_sched.py): whole frames of 8 slots of 625 samples from the oracle's modulator through tests/ms_rx_cases.py --
SCH bursts of the cell in the SCH slots, noise alone in the FCCH slots, normal bursts in every other slot."""
import numpy as np

import ms_rx_cases as K
import ms_rx_model as RX
import ms_sched_model as SM
import sch_sync_model as SS

SLOT = K.SLOT
FULL = 2047.0
SCALE = np.float32(1.0) / np.float32(FULL)


def cell_stream(seed, fn0, n_frames, bsic, tsc=None, late=0, lead=0, snr_db=25.0, amp=3000.0):
    """`lead` samples of noise, then the slots (fn0, 0) .. (fn0 + n_frames - 1, 7), every burst `late` samples into its slot.
    tsc: the training sequence of the traffic bursts (None: frame fn uses fn % 8).  Returns (int16[n, 2] samples, sent) with
    sent[(fn, tn)] = the 148 bits of a traffic slot; the SCH slots carry (bsic, fn)."""
    rng = np.random.default_rng(seed)
    parts = [K.place(rng, None, None, snr_db, amp)[:lead]] if lead else []
    sent = {}
    for fn in range(fn0, fn0 + n_frames):
        for tn in range(8):
            if SM.is_sch(fn, tn):
                parts.append(K.sch_slot(rng, bsic, fn, late, snr_db, amp))
            elif SM.is_fcch(fn, tn):
                parts.append(K.place(rng, None, None, snr_db, amp))
            else:
                y, bits = K.nb_slot(rng, fn % 8 if tsc is None else tsc, late, snr_db, amp)
                parts.append(y)
                sent[(fn, tn)] = bits
    return K.to_i16(np.concatenate(parts)), sent


# the acquire -> pull loopback: 12 frames that hold one SCH burst (frame 52 of the multiframe that begins at 51 * 777), and 12 more
LOOP = dict(seed=4100, fn0=51 * 777 + 45, n_frames=24, bsic=0o53, tsc=0o53 & 7, lead=137, t0=1_000_000, acq_len=60000,
            active=0b01100110, chunks=(7000, 3111, 100000))


def loopback_stream():
    return cell_stream(LOOP["seed"], LOOP["fn0"], LOOP["n_frames"], LOOP["bsic"], tsc=LOOP["tsc"], lead=LOOP["lead"])


class _Window:
    """slot samples by timestamp out of the carried partial slot followed by the chunk"""

    def __init__(self, have, base):
        self.have, self.base = have, base

    def __getitem__(self, ts):
        o = ts - self.base
        assert 0 <= o <= len(self.have) - SLOT, (ts, self.base, len(self.have))
        return self.have[o:o + SLOT]


def model_loopback(x):
    """The loopback on the CPU models alone: sch_sync_model's ACQ receiver, ms_sched_model's cutter fed with sch_sync_model's
    TRACK starts, ms_rx_model on every cut slot.  Returns (acq record, [(fn, tn, model record)] for every slot cut)."""
    acq = SS.sch_sync(x[:LOOP["acq_len"]], SS.ACQ, SCALE)
    assert acq["rc"] == 1
    win = [None]

    def starts(fn, tn, ts):
        m = SS.sch_sync(win[0][ts], SS.TRACK, SCALE)
        return int(m["start"]) if m["rc"] == 1 else None

    cut = SM.Cutter(starts)
    cut.acquired(int(acq["fn"]), int(acq["start"]), LOOP["t0"])
    out, at = [], LOOP["acq_len"]
    carry = x[:0]
    for n in LOOP["chunks"]:
        chunk = x[at:at + n]
        first_ts = LOOP["t0"] + at
        have = np.concatenate([carry, chunk])
        win[0] = _Window(have, first_ts - len(carry))
        for fn, tn, ts, off in cut.grab_bursts(first_ts, len(chunk)):
            out.append((fn, tn, RX.ms_rx(win[0][ts], fn, tn, LOOP["tsc"], bool((LOOP["active"] >> tn) & 1), FULL)))
        carry = have[len(have) - cut.partial_rdofs:]
        at += len(chunk)
    return acq, out
