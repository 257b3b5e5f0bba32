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
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

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
    print(json.dumps(br.time_in_order(torch, legs, br.select_legs(legs, a.legs), a)), flush=True)


def summarise(per_leg, a):
    n = a.slots
    res = {"workload": "rx_sched", "sps": a.sps, "slots": n, "chans": 1, "rounds": a.rounds, "reps": a.reps, "legs": {}}
    if a.sps == 4:
        del res["sps"]
    for name, xs in per_leg.items():
        res["legs"][name] = br.leg_summary(xs, ns_per_slot=round(statistics.median(xs) * 1e6 / n, 2))
    two = res["legs"]["two_calls"]["median_ms"]
    for name in ("pull", "pull_aligned"):
        res[name + "_minus_two_calls_ms"] = round(res["legs"][name]["median_ms"] - two, 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sps", type=int, default=4, choices=(4, 1))
    ap.add_argument("--slots", type=int, default=1 << 18)
    br.add_options(ap, "rx_sched", warmup=3, reps=10, timeout=240, trace="off")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    if a.sps == 1 and a.slots % 8:
        ap.error("--sps 1: whole frames (the steady-state pull starts at TN 0 every time)")
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots), "--sps", str(a.sps)]
    tag = "rx_sched" if a.sps == 4 else "rx_sched_sps1"
    res = summarise(br.run_rounds(tag, me, a), a)
    if not a.no_trace:
        n, small = a.slots, ["--warmup", "1", "--reps", "3"]
        rows = br.kernel_trace(tag, me, small, "pull", a)
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
            both = br.kernel_trace(tag, me, small, "pull_aligned,two_calls", a)
            res["stream_vs_row_kernel_us"] = {k: both[k] for k in ("burst_pull_stream_kernel<false>", "burst_pull_kernel<1, false, 3>")}
            res["stream_vs_row_kernel_ns_per_slot"] = [round(v["avg_us"] * 1e3 / n, 3) for v in res["stream_vs_row_kernel_us"].values()]
    old = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
    if a.sps == 1:                                                         # under a key of its own: the 4-SPS entries stay
        out = dict(old, sps1=res)
    else:
        out = dict(res, sps1=old["sps1"]) if "sps1" in old else res
    br.write_json(a.out, out)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
