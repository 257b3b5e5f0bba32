#!/usr/bin/env python3
"""The MS-side downlink slot scheduler on one GPU against the path the tree had before it, HIP-event time, over an int16 stream
with the 51-multiframe mix over 8 TNs (per 408 slots: 5 FCCH, 5 SCH, 398 traffic), all ACTIVE, tracking on:
  sched      one trxhip_ms_sched_pull_s16 of `slots` slots (set_clock + pull per call: no slot records exist)
  rows       the same samples the way a caller had to do it: the slot records {fn, tn, tsc, ACTIVE} made on the host (outside the
             timed region: the cut and the clock are the caller's), their upload from pinned memory, trxhip_ms_rx_batch_i16
  sched8     51 consecutive pulls of 8 slots (one multiframe; every pull behind an SCH-carrying pull waits for the correction),
             per pull
  rows8      51 times: upload 8 slot records, trxhip_ms_rx_batch_i16 on 8 slots, per call
The stream is cut at multiples of 625, so the single pull and `rows` read the same slots and must give the same bytes (checked after
the timing; from pull to pull the cut follows the SCH bursts, so the 8-slot pulls need not lie where the rows do).
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; inside a round the legs are timed in turns, in alternating
order, and the round reports each leg's median.  Then one run per leg under rocprofv3 --kernel-trace --stats gives the durations
of the stream instance and of the join kernel.  Medians, spreads (max - min over the rounds) and the trace rows go to
profiles/ms_sched_bench.json.

   python3 tools/bench_ms_sched.py [--rounds 5] [--slots N] [--inner I] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
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


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    from workloads import TSC, multiframe
    trx = TrxHip(0)
    base_iq, base_slots, sent, kinds = multiframe(trx, BASE_FN)
    reps = (a.slots + 407) // 408
    iq = base_iq.repeat(reps, 1, 1)[:a.slots].contiguous()         # [slots, 625, 2]: a stream cut at multiples of 625
    slots_np = np.tile(base_slots, reps)[:a.slots].copy()
    slots_np["fn"] += 51 * (np.arange(a.slots, dtype=np.uint32) // 408)
    h_slots = torch.from_numpy(slots_np.view(np.uint8).reshape(-1, 8).copy()).pin_memory()
    d_slots = torch.empty_like(h_slots, device="cuda:0")
    L, st = trx.L, trx._stream()
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    ind = torch.empty((a.slots, 32), dtype=torch.uint8, device="cuda:0")
    bits = torch.empty((a.slots, 148), dtype=torch.int8, device="cuda:0")
    ind_r, bits_r = torch.empty_like(ind), torch.empty_like(bits)
    s = trxhip.MsRxScheduler(trx, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True)
    ns, nc = C.c_size_t(), C.c_size_t()
    small = 51 * 8

    def sched():
        s.set_clock(BASE_FN - 1, 7, -625)
        trxhip._check(L.trxhip_ms_sched_pull_s16(s.h, ptr(iq), a.slots * 625, 0, ptr(ind), ptr(bits), a.slots, C.byref(ns), C.byref(nc), st),
                      "pull")

    def rows():
        d_slots.copy_(h_slots, non_blocking=True)
        trxhip._check(L.trxhip_ms_rx_batch_i16(trx.h, ptr(iq), 625, ptr(d_slots), ptr(ind_r), ptr(bits_r), a.slots, FULL_SCALE, st), "ms_rx")

    def sched8():
        s.set_clock(BASE_FN - 1, 7, -625)
        for k in range(51):
            trxhip._check(L.trxhip_ms_sched_pull_s16(s.h, ptr(iq, k * 8 * 625 * 4), 8 * 625, k * 8 * 625, ptr(ind, k * 8 * 32),
                                                     ptr(bits, k * 8 * 148), 8, C.byref(ns), C.byref(nc), st), "pull")

    def rows8():
        for k in range(51):
            d_slots[k * 8:k * 8 + 8].copy_(h_slots[k * 8:k * 8 + 8], non_blocking=True)
            trxhip._check(L.trxhip_ms_rx_batch_i16(trx.h, ptr(iq, k * 8 * 625 * 4), 625, ptr(d_slots, k * 8 * 8), ptr(ind_r, k * 8 * 32),
                                                   ptr(bits_r, k * 8 * 148), 8, FULL_SCALE, st), "ms_rx")

    legs = {"sched": (sched, 1), "rows": (rows, 1), "sched8": (sched8, 51), "rows8": (rows8, 51)}
    assert a.slots >= small
    names = br.select_legs(legs, a.legs)
    times = br.time_in_turns(torch, legs, names, a)
    # the two paths gave the same bytes, and the slots received what was sent
    if "sched" in names and "rows" in names:
        sched()
        rows()
        torch.cuda.synchronize()
        assert ns.value == a.slots and nc.value == 0
        assert torch.equal(ind, ind_r) and torch.equal(bits, bits_r), "the scheduler's slots differ from the row receiver's"
        r = ind.cpu().numpy().reshape(-1).view(trxhip.MS_IND_DTYPE)
        sch = r["kind"] == trxhip.MS_KIND_SCH
        assert (r["sch_rc"][sch] == 1).all() and (r["sch_fn"][sch] % 51 == r["fn"][sch] % 51).all(), "SCH slots did not decode"   # (the multiframe repeats)
        dem = kinds != trxhip.MS_KIND_FCCH
        assert np.array_equal(bits[:408].cpu().numpy()[dem], np.where(sent[dem] > 0, -127, 127)), "the bits are not the ones sent"
    if "sched8" in names and "rows8" in names:
        # (with tracking on the cut follows the SCH bursts from pull to pull: the 8-slot pulls need not lie where the rows do)
        before = int(s.state()["slots"])
        sched8()
        torch.cuda.synchronize()
        assert 51 * 7 <= int(s.state()["slots"]) - before <= small, "8-slot pulls cut too few slots"
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "ms_sched", "slots": a.slots, "small_pull_slots": 8, "slot_len": 625, "mix_per_408": {"fcch": 5, "sch": 5, "traffic": 398},
           "input": "int16", "tracking": True, "rounds": a.rounds, "inner": a.inner, "reps": a.reps,
           "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}}
    lg = res["legs"]
    res["sched_over_rows"] = round(lg["sched"]["median_ms"] / lg["rows"]["median_ms"], 4)
    res["sched8_over_rows8"] = round(lg["sched8"]["median_ms"] / lg["rows8"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    br.add_options(ap, "ms_sched", warmup=2, reps=3, timeout=180, inner=5, trace="off")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots)]
    res = summarise(br.run_rounds("ms_sched", me, a), a)
    if not a.no_trace:
        res["kernel_trace_us"] = {}
        for leg in ("sched", "rows", "sched8"):
            rows = br.kernel_trace("ms_sched", me, ["--inner", "1", "--warmup", "1", "--reps", "3"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if re.match(r"ms_rx|ms_join", k)}
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
