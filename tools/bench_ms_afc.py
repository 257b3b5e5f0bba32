#!/usr/bin/env python3
"""The cost of the MS-side FCCH frequency-offset measurement on one GPU: the same pulls on scheduler objects with AFC on and off,
HIP-event time, int16, the 51-multiframe mix of tools/bench_ms_group.py, all ACTIVE, tracking on.
  on64 / off64     a group of 64 members, 8 slots (one frame) per member and pull, `frames` pulls in a row; per frame
  on256 / off256   the same with 256 members
  on1 / off1       the single object, 8 slots per pull
  onbig / offbig   the single object, one pull of `slots` slots (set_clock + pull per call)
  batch            trxhip_ms_fcch_batch_i16 over `slots` rows; per call
The members with AFC on write their records to a d_fcch array.  Every round is a fresh process under its own time limit; inside a
round the legs are timed in turns, the order reversed every other turn; every timed region follows one untimed call of the same
leg.  Median per leg over the rounds, spread = max - min over the rounds -> profiles/ms_afc_bench.json; `big_pair_alone`: as many rounds
of onbig / offbig in processes of their own.  The first step that
fails ends the run.

   python3 tools/bench_ms_afc.py [--rounds 5] [--slots N] [--frames F] [--inner I] [--warmup W] [--reps R] [--timeout S] [--trace LEG] [--out FILE]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

FULL_SCALE = 2047.0
BASE_FN = 51 * 4321
FRAME = 8 * 625
PAIRS = (("on64", "off64"), ("on256", "off256"), ("on1", "off1"), ("onbig", "offbig"))
ROW_BYTES = 124 * 4 + 32               # the batch pass reads samples 52 .. 175 of a row and writes a record


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per frame (per pull for the big legs, per call for batch)}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    from workloads import TSC, multiframe
    trx = TrxHip(0)
    base_iq = multiframe(trx, BASE_FN)[0]
    names = br.select_legs([k for pair in PAIRS for k in pair] + ["batch"], a.legs)
    L, st = trx.L, trx._stream()
    vp = C.c_void_p
    frames = a.frames
    assert 1 <= frames <= 51
    iq = base_iq.repeat(3, 1, 1).contiguous()
    stride = 9
    ns1, nc1 = C.c_size_t(), C.c_size_t()
    legs, checks = {}, []

    def group_pair(n):
        gs = [trxhip.MsRxSchedulerGroup(trx, n=n, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True) for _ in range(2)]
        fc = torch.zeros((n * stride, 32), dtype=torch.uint8, device="cuda:0")
        for m in range(n):
            gs[0].set_afc(m, True, out=fc)
        tabs = []
        for k in range(frames):
            ch = np.zeros(n, dtype=trxhip.MS_GROUP_CHUNK_DTYPE)
            ch["d_in"] = [iq.data_ptr() + ((m % 51) + k) * FRAME * 4 for m in range(n)]
            ch["n_samples"], ch["first_ts"] = FRAME, k * FRAME
            tabs.append(ch)
        ind = torch.zeros((2, n, stride, 32), dtype=torch.uint8, device="cuda:0")
        bits = torch.zeros((2, n, stride, 148), dtype=torch.int8, device="cuda:0")
        cnt = (C.c_size_t * n)()

        def leg(i):
            def run():
                for m in range(n):
                    gs[i].set_clock(m, BASE_FN + (m % 51) - 1, 7, -625)
                for ch in tabs:
                    trxhip._check(L.trxhip_ms_group_pull_s16(gs[i].h, ch.ctypes.data_as(vp), vp(ind[i].data_ptr()), vp(bits[i].data_ptr()),
                                                             stride, C.cast(cnt, vp), None, None, st), "group pull")
            return run

        def check():
            before = sum(gs[0].afc_state(m)["count"] for m in range(n))
            ind.zero_()
            bits.zero_()
            leg(0)()
            leg(1)()
            torch.cuda.synchronize()
            assert torch.equal(ind[0], ind[1]) and torch.equal(bits[0], bits[1]), "AFC changed what a pull returns"
            want = sum(((m % 51) + k) % 51 in (0, 10, 20, 30, 40) for m in range(n) for k in range(frames))
            got = sum(gs[0].afc_state(m)["count"] for m in range(n)) - before       # (a cut the SCH bursts moved may end a slot early)
            assert want - n <= got <= want and got > 0 and gs[1].afc_state(0)["count"] == 0, (got, want)

        return leg(0), leg(1), check

    for n, (on, off) in ((64, PAIRS[0]), (256, PAIRS[1])):
        if on in names or off in names:
            legs[on], legs[off], check = group_pair(n)
            legs[on], legs[off] = (legs[on], frames), (legs[off], frames)
            checks.append(check)

    def single_pair(x, n_samples, out_slots, per_call_clock, tabs_ts):
        ss = [trxhip.MsRxScheduler(trx, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True) for _ in range(2)]
        fc = torch.zeros((out_slots, 32), dtype=torch.uint8, device="cuda:0")
        ss[0].set_afc(True, out=fc)
        ind = torch.zeros((2, out_slots, 32), dtype=torch.uint8, device="cuda:0")
        bits = torch.zeros((2, out_slots, 148), dtype=torch.int8, device="cuda:0")

        def leg(i):
            args = [(ss[i].h, vp(x.data_ptr() + k * n_samples * 4), n_samples, ts, vp(ind[i].data_ptr()), vp(bits[i].data_ptr()), out_slots,
                     C.byref(ns1), C.byref(nc1), st) for k, ts in enumerate(tabs_ts)]

            def run():
                ss[i].set_clock(*per_call_clock)
                for arg in args:
                    if L.trxhip_ms_sched_pull_s16(*arg) != 0:
                        raise RuntimeError("trxhip_ms_sched_pull_s16 failed")
            return run

        def check():
            before = ss[0].afc_state()["count"]
            leg(0)()
            leg(1)()
            torch.cuda.synchronize()
            assert torch.equal(ind[0], ind[1]) and torch.equal(bits[0], bits[1]), "AFC changed what a pull returns"
            frames_cut = n_samples // FRAME * len(tabs_ts)
            want = sum(f % 51 in (0, 10, 20, 30, 40) for f in range(frames_cut))
            got = ss[0].afc_state()["count"] - before
            assert want - 1 <= got <= want and got > 0 and ss[1].afc_state()["count"] == 0, (got, want)

        return leg(0), leg(1), check

    if "on1" in names or "off1" in names:
        r0, r1, check = single_pair(iq, FRAME, stride, (BASE_FN - 1, 7, -625), [k * FRAME for k in range(frames)])
        legs["on1"], legs["off1"] = (r0, frames), (r1, frames)
        checks.append(check)
    big = None
    if "onbig" in names or "offbig" in names or "batch" in names:
        big = base_iq.repeat((a.slots + 407) // 408, 1, 1)[:a.slots].contiguous()
    if "onbig" in names or "offbig" in names:
        r0, r1, check = single_pair(big, a.slots * 625, a.slots, (BASE_FN - 1, 7, -625), [0])
        legs["onbig"], legs["offbig"] = (r0, 1), (r1, 1)
        checks.append(check)
    if "batch" in names:
        rec = torch.empty((a.slots, 32), dtype=torch.uint8, device="cuda:0")

        def batch():
            trxhip._check(L.trxhip_ms_fcch_batch_i16(trx.h, vp(big.data_ptr()), 625, vp(rec.data_ptr()), a.slots, FULL_SCALE, st), "fcch batch")

        legs["batch"] = (batch, 1)
    names = [k for k in names if k in legs]
    times = br.time_in_turns(torch, legs, names, a, untimed_first=True)
    if not a.legs:
        for check in checks:
            check()
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "ms_afc", "slots": a.slots, "small_pull_slots": 8, "frames_per_call": a.frames, "slot_len": 625, "input": "int16",
           "tracking": True, "rounds": a.rounds, "inner": a.inner, "reps": a.reps,
           "unit": "ms per frame of all members (onbig / offbig: per pull; batch: per call)",
           "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}, "pairs": {}}
    for x, y in PAIRS:
        if x in res["legs"] and y in res["legs"]:
            res["pairs"][x + "_over_" + y] = br.pair(res["legs"], x, y)
    if "batch" in res["legs"]:
        ms = res["legs"]["batch"]["median_ms"]
        res["batch_pass"] = dict(rows=a.slots, bytes=a.slots * ROW_BYTES, fraction_of_8TBps=round(a.slots * ROW_BYTES / 8e12 / (ms * 1e-3), 4))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--frames", type=int, default=17, help="8-slot pulls in a row per timed call")
    br.add_options(ap, "ms_afc", warmup=2, reps=3, timeout=150, inner=6, even_inner=True, trace="legs")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots), "--frames", str(a.frames)]
    res = summarise(br.run_rounds("ms_afc", me, a), a)
    # the large pair once more in processes that time nothing else: in the full round the large legs follow the small ones, whose
    # pulls leave the GPU idle most of the time, in every other turn
    alone = br.run_rounds("ms_afc_big", me + ["--legs", "onbig,offbig"], a)
    res["big_pair_alone"] = {"legs": {name: br.leg_summary(xs) for name, xs in alone.items()}}
    res["big_pair_alone"]["onbig_over_offbig"] = br.pair(res["big_pair_alone"]["legs"], "onbig", "offbig")
    if a.trace:
        res["kernel_trace_us"] = {}
        for leg in a.trace.split(","):
            rows = br.kernel_trace("ms_afc", me, ["--inner", "1", "--warmup", "1", "--reps", "1"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if re.match(r"ms_rx|ms_join|ms_fcch", k)}
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
