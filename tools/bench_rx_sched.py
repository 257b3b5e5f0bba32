#!/usr/bin/env python3
"""The uplink burst scheduler on one GPU, HIP-event time per call: one trxhip_rx_sched_pull_s16 of 262 144 slots (one channel,
int16, normal bursts, combination I on every TN) against what it is built from, trxhip_detect_demod_batch +
trxhip_pack_trxd_wire_batch on the same rows with params / meta already resident.
  two_calls      the two entry points back to back
  pull           steady state: every pull carries one sample over, so slot 0 straddles the remainder and the chunk (one more
                 detect launch over the assembled row)
  pull_aligned   set_clock before every pull (the remainder dropped): every slot lies in the chunk
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; a round times every leg once, in alternating order.
Then one run of its own under rocprofv3 --kernel-trace --stats gives the kernels' own durations.  Medians, each leg's spread
(max - min over the rounds) and the trace rows go to profiles/rx_sched_bench.json.
--sps 1: the same at one sample per symbol -- a stream of 157 / 156 / 156 / 156 slots through an object of
trxhip_rx_sched_create_sps(), against trxhip_detect_demod_batch(sps = 1, burst_len = 156) + the packer over as many resident
rows.  A second trace, over pull_aligned and two_calls, puts burst_pull_stream_kernel<false> next to burst_pull_kernel<1, false, 3>
(in the steady-state pull the row kernel also runs over the one straddling row, which would be averaged in); the result goes
under the key "sps1" of the same file and the 4-SPS entries stay.

   python3 tools/bench_rx_sched.py [--sps 4|1] [--rounds 5] [--slots N] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

TSC = 0


def child(a):
    """One round: every leg once -> one JSON line {leg: ms per call}."""
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, synth, trxhip
    trx = TrxHip(0)
    L, st = trx.L, trx._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    n = a.slots
    if a.sps == 1:
        # rows of 157; the stream takes 157 samples of a row where the slot's TN is a multiple of 4 (the clock starts at TN 0) and
        # 156 elsewhere, the batch leg the first 156 of every row
        iq, params, _ = synth.make_normal_bursts(n, "cuda:0", 1, tsc=TSC, max_toa=30, burst_len=157)
        keep = torch.arange(157, device="cuda:0")[None, :] < (156 + (torch.arange(n, device="cuda:0") % 4 == 0))[:, None]
        total, blen = n * 1250 // 8, 156
        x = torch.zeros((total + 1, 2), dtype=torch.int16, device="cuda:0")
        x[:total] = iq[keep]
        rows = iq[:, :156].contiguous()
        del iq, keep
    else:
        iq, params, _ = synth.make_normal_bursts(n, "cuda:0", 4, tsc=TSC, max_toa=30)
        total, blen = n * 625, 625
        x = torch.zeros((total + 1, 2), dtype=torch.int16, device="cuda:0")
        x[:total] = iq.view(total, 2)
        rows = x
        del iq
    d_params = trx.params_tensor(params)
    meta = np.zeros(n, dtype=trxhip.TRXD_META_DTYPE)
    meta["fn"], meta["tn"], meta["version"] = np.arange(n) // 8, np.arange(n) % 8, 1
    d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1, 8).copy()).to("cuda:0")
    res = torch.empty((n, 32), dtype=torch.uint8, device="cuda:0")
    soft = torch.empty((n, 148), dtype=torch.float32, device="cuda:0")
    pkt = torch.empty((n, 160), dtype=torch.uint8, device="cuda:0")
    plen = torch.empty(n, dtype=torch.int16, device="cuda:0")
    ind = torch.empty((n, 32), dtype=torch.uint8, device="cuda:0")
    s = trxhip.RxScheduler(trx, chans=1, sps=a.sps, tsc=TSC, max_slots=n)
    for tn in range(8):
        s.set_slot(0, tn, 1)
    s.set_trxd_version(0, 1)

    def two_calls():
        trxhip._check(L.trxhip_detect_demod_batch(trx.h, ptr(rows), ptr(d_params), ptr(res), ptr(soft), n, blen, a.sps, 4.0, 32767.0, 148,
                                                  trxhip.FLAG_SLICE, st), "detect")
        trxhip._check(L.trxhip_pack_trxd_wire_batch(trx.h, ptr(res), ptr(d_params), ptr(soft), 148, ptr(d_meta), ptr(pkt), 160,
                                                    ptr(plen), n, 0.0, st), "pack")

    def pull(n_samples):
        trxhip._check(L.trxhip_rx_sched_pull_s16(s.h, ptr(x), n_samples, n_samples, ptr(pkt), 160, ptr(plen), ptr(ind), None, n, None,
                                                 None, st), "pull")

    def pull_steady():
        pull(total)

    def pull_aligned():
        s.set_clock(0, 0)
        pull(total + 1)

    def start_steady():
        s.set_clock(0, 0)
        pull(total + 1)                                                # leaves one sample: the next pulls of `total` cut n slots each

    legs = {"two_calls": (None, two_calls), "pull": (start_steady, pull_steady), "pull_aligned": (None, pull_aligned)}
    names = [k for k in legs if not a.legs or k in a.legs.split(",")]
    if a.round % 2:
        names.reverse()
    out = {}
    for name in names:
        prep, f = legs[name]
        if prep:
            prep()
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(a.reps):
            f()
        ev[1].record()
        torch.cuda.synchronize()
        out[name] = ev[0].elapsed_time(ev[1]) / a.reps
    print(json.dumps(out), flush=True)


def trace_rows(d):
    """{kernel: {calls, avg_us}} of a rocprofv3 --kernel-trace --stats directory"""
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
                rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sps", type=int, default=4, choices=(4, 1))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per round")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rx_sched_bench.json"))
    ap.add_argument("--logs", default=os.path.join(ROOT, "build", "measure"))
    ap.add_argument("--round", type=int, default=None, help=argparse.SUPPRESS)     # child: run one round on the GPU
    ap.add_argument("--legs", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    if a.rounds < 5:
        ap.error("at least five rounds")
    if a.sps == 1 and a.slots % 8:
        ap.error("--sps 1: whole frames (the steady-state pull starts at TN 0 every time)")
    import measure
    os.makedirs(a.logs, exist_ok=True)
    per_leg = {}
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots), "--sps", str(a.sps)]
    tag = "rx_sched" if a.sps == 4 else "rx_sched_sps1"
    for r in range(a.rounds):
        log = os.path.join(a.logs, tag + "_round_%d.log" % (r + 1))
        measure.step("round %d" % (r + 1), me + ["--round", str(r), "--warmup", str(a.warmup), "--reps", str(a.reps)], log, a.timeout)
        for k, v in measure.last_json(log).items():
            per_leg.setdefault(k, []).append(v)
        print("round %d done" % (r + 1), flush=True)
    n = a.slots
    res = {"workload": "rx_sched", "sps": a.sps, "slots": n, "chans": 1, "rounds": a.rounds, "reps": a.reps, "legs": {}}
    if a.sps == 4:
        del res["sps"]
    for name, xs in per_leg.items():
        med = statistics.median(xs)
        res["legs"][name] = dict(median_ms=round(med, 4), spread_ms=round(max(xs) - min(xs), 4), ms=[round(x, 4) for x in xs],
                                 ns_per_slot=round(med * 1e6 / n, 2))
    two = res["legs"]["two_calls"]["median_ms"]
    for name in ("pull", "pull_aligned"):
        res[name + "_minus_two_calls_ms"] = round(res["legs"][name]["median_ms"] - two, 4)
    if not a.no_trace:
        d = os.path.join(a.logs, tag + "_trace")

        def trace(legs):
            shutil.rmtree(d, ignore_errors=True)
            measure.step("kernel trace", ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rx_sched", "--"] +
                         me + ["--round", "0", "--warmup", "1", "--reps", "3", "--legs", legs], os.path.join(a.logs, tag + "_trace.log"),
                         a.timeout)
            return trace_rows(d)

        rows = trace("pull")
        res["kernel_trace_us"] = {k: v for k, v in sorted(rows.items()) if k.startswith(("rx_", "pack_trxd_wire", "nb_pull4", "burst_pull4", "burst_pull_"))}
        new = sum(v["avg_us"] for k, v in rows.items() if k.startswith("rx_"))
        res["new_kernels_us_per_pull"] = round(new, 2)
        res["pull_minus_two_calls_minus_new_kernels_ms"] = round(res["pull_minus_two_calls_ms"] - new / 1e3, 4)
        if a.sps == 1:
            # the yardstick: the pull is done when its excess over the two calls is no more than the three small kernels' own
            # durations plus the larger of the two run-to-run spreads
            spread = max(res["legs"]["pull"]["spread_ms"], res["legs"]["two_calls"]["spread_ms"])
            res["allowed_excess_ms"] = round(new / 1e3 + spread, 4)
            res["within_allowance"] = res["pull_minus_two_calls_ms"] <= res["allowed_excess_ms"]
            both = trace("pull_aligned,two_calls")
            res["stream_vs_row_kernel_us"] = {k: both[k] for k in ("burst_pull_stream_kernel<false>", "burst_pull_kernel<1, false, 3>")}
            res["stream_vs_row_kernel_ns_per_slot"] = [round(v["avg_us"] * 1e3 / n, 3) for v in res["stream_vs_row_kernel_us"].values()]
        shutil.rmtree(d, ignore_errors=True)
    out = res
    if a.sps == 1:                                                         # under a key of its own: the 4-SPS entries stay
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out["sps1"] = res
    elif os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "sps1" in old:
            out = dict(res, sps1=old["sps1"])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
