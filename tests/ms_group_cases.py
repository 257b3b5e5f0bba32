"""Streams and CPU models for the tests of the MS-side scheduler group (tests/test_ms_group_cpu.py, tests/test_gpu_ms_group.py):
the acquire -> pull loopback of tests/ms_sched_cases.py for several cells at once, each described by a dict of LOOP's shape."""
import numpy as np

import ms_rx_model as RX
import ms_sched_cases as SC
import ms_sched_model as SM
import sch_sync_model as SS

# Three members of the batched acquire -> pull loopback.  Each cell: 12 frames that hold ONE SCH burst (frame fn0 + 7 has
# fn % 51 == 1, the frames 10 before and after it have not), and 12 more; the last chunk ends with the stream.  "noise": the
# member whose buffer holds no SCH burst.
LOOPS = [
    dict(seed=4200, fn0=51 * 300 + 45, n_frames=24, bsic=0o53, tsc=0o53 & 7, lead=137, t0=1_000_000, acq_len=60000, active=0b01100110,
         chunks=(7000, 3111, 100000)),
    dict(noise=True, seed=4201, t0=2_000_000, acq_len=60000, active=0xFF, chunks=(7000, 3111, 100000)),
    dict(seed=4202, fn0=51 * 1200 + 45, n_frames=24, bsic=0o16, tsc=0o16 & 7, lead=411, t0=-5_000, acq_len=60000, active=0b10011001,
         chunks=(5000, 6222, 100000)),
]


def loop_stream(L):
    """(int16[n, 2] samples, sent bits by (fn, tn)) of one loopback cell; the noise member: amplitude-50 noise, nothing sent"""
    if L.get("noise"):
        rng = np.random.default_rng(L["seed"])
        return rng.integers(-50, 51, (L["acq_len"] + 60137, 2)).astype(np.int16), {}
    return SC.cell_stream(L["seed"], L["fn0"], L["n_frames"], L["bsic"], tsc=L["tsc"], lead=L["lead"])


def model_loopback(x, L):
    """tests/ms_sched_cases.py::model_loopback for the cell L: (acq record, [(fn, tn, model record)] for every slot cut)"""
    acq = SS.sch_sync(x[:L["acq_len"]], SS.ACQ, SC.SCALE)
    if acq["rc"] != 1:
        return acq, []
    win = [None]

    def starts(fn, tn, ts):
        m = SS.sch_sync(win[0][ts], SS.TRACK, SC.SCALE)
        return int(m["start"]) if m["rc"] == 1 else None

    cut = SM.Cutter(starts)
    cut.acquired(int(acq["fn"]), int(acq["start"]), L["t0"])
    out, at = [], L["acq_len"]
    carry = x[:0]
    for n in L["chunks"]:
        chunk = x[at:at + n]
        first_ts = L["t0"] + at
        have = np.concatenate([carry, chunk])
        win[0] = SC._Window(have, first_ts - len(carry))
        for fn, tn, ts, off in cut.grab_bursts(first_ts, len(chunk)):
            out.append((fn, tn, RX.ms_rx(win[0][ts], fn, tn, L["tsc"], bool((L["active"] >> tn) & 1), SC.FULL)))
        carry = have[len(have) - cut.partial_rdofs:]
        at += len(chunk)
    return acq, out
