#!/usr/bin/env python3
"""The uplink scheduler behind the receive front end on one GPU, HIP-event time per pull: wideband int16 of three ARFCNs
(MULTI, 192-step blocks at 65/48) to TRXD indications, steady state (every pull finds a carried remainder).
  two_calls      trxhip_rx_frontend_pull into resident rows, then trxhip_rx_sched_pull_cf32 over them: the slot that begins
                 in the remainder is assembled (rx_edge_kernel) and detected by a launch of its own over chans rows
  pull_frontend  trxhip_rx_sched_pull_frontend into a resident work area: rx_join_kernel, one detect launch per channel
The method is tools/bench_rx_sched.py's: the driver (no --round) never opens the GPU; every round is a fresh child process
under its own time limit through tools/measure.py's step(), which stops the run at the first failure; a round times both legs
once, in alternating order (the times are also kept by position, first or second in their process: at the large size the leg
that runs first is the slower one, whichever it is).  Then each leg runs once under rocprofv3 --kernel-trace --stats for the kernels' own durations.
Medians, spreads (max - min over the rounds) and the trace rows go to profiles/rx_sched_frontend_bench.json under the key
"blocks_<N>", so that the large pull (262 144 blocks) and the real-time-sized one (8 blocks) sit side by side.

   python3 tools/bench_rx_sched_frontend.py [--blocks N] [--rounds 5] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
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

CHANS, TSC = 3, 0


def child(a):
    """One round: both legs once -> one JSON line {leg: ms per pull}."""
    import torch
    from osmo_trx_amd import TrxHip, synth, trxhip
    trx = TrxHip(0)
    L, st = trx.L, trx._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    nb = a.blocks
    # 1040 slots of three carriers are 2500 blocks; the stream repeats them (the seams are a handful of slots)
    base, base_blocks, _, _ = synth.make_multi_arfcn_wideband(1040, "cuda:0")
    wide = base.repeat((nb + base_blocks - 1) // base_blocks, 1)[:nb * 768].contiguous()
    del base
    n_out = nb * 260
    cap = n_out // 625 + 2                                             # slots a pull can cut
    rows = torch.empty((CHANS, n_out), dtype=torch.complex64, device="cuda:0")
    work = torch.empty((CHANS, trxhip.RX_SCHED_WORK_HEAD + n_out), dtype=torch.complex64, device="cuda:0")
    soft = torch.empty((CHANS * cap, 148), dtype=torch.float32, device="cuda:0")
    pkt = torch.empty((CHANS * cap, 160), dtype=torch.uint8, device="cuda:0")
    plen = torch.empty(CHANS * cap, dtype=torch.int16, device="cuda:0")
    ind = torch.empty((CHANS * cap, 32), dtype=torch.uint8, device="cuda:0")

    def pair():
        fe = trxhip.RxFrontEnd(trx, 192, 65, 48, chans=CHANS)
        s = trxhip.RxScheduler(trx, chans=CHANS, tsc=TSC, max_slots=cap)
        s.set_clock(0, 0)
        for c in range(CHANS):
            for tn in range(8):
                s.set_slot(c, tn, 1)
            s.set_trxd_version(c, 1)
        return fe, s

    fe2, s2 = pair()
    fej, sj = pair()

    def two_calls():
        trxhip._check(L.trxhip_rx_frontend_pull(fe2.h, ptr(wide), nb, ptr(rows), n_out, st), "frontend_pull")
        trxhip._check(L.trxhip_rx_sched_pull_cf32(s2.h, ptr(rows), n_out, n_out, ptr(pkt), 160, ptr(plen), ptr(ind), ptr(soft), cap,
                                                  None, None, st), "pull_cf32")

    def pull_frontend():
        trxhip._check(L.trxhip_rx_sched_pull_frontend(sj.h, fej.h, ptr(wide), nb, ptr(work), work.shape[1], ptr(pkt), 160, ptr(plen),
                                                      ptr(ind), ptr(soft), cap, None, None, st), "pull_frontend")

    legs = {"two_calls": (None, two_calls), "pull_frontend": (None, pull_frontend)}
    a.warmup = max(a.warmup, 1)                                        # the first pull leaves the remainder the others find
    out = br.time_in_order(torch, legs, br.select_legs(legs, a.legs), a)
    out["order"] = list(out)
    print(json.dumps(out), flush=True)


def summarise(per_leg, a):
    per_leg = dict(per_leg)
    by_pos = {}
    for r, order in enumerate(per_leg.pop("order")):                   # the leg a process times first pays for its first touches
        for pos, k in enumerate(order):
            by_pos.setdefault(k, {}).setdefault(("first", "second")[pos], []).append(round(per_leg[k][r], 4))
    res = {"workload": "rx_sched_frontend", "mode": "MULTI", "chans": CHANS, "blocks": a.blocks, "samples_per_chan": a.blocks * 260,
           "rounds": a.rounds, "reps": a.reps, "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}}
    res["pull_frontend_minus_two_calls_ms"] = round(res["legs"]["pull_frontend"]["median_ms"] - res["legs"]["two_calls"]["median_ms"], 4)
    res["larger_spread_ms"] = max(v["spread_ms"] for v in res["legs"].values())
    res["no_slower_beyond_spread"] = res["pull_frontend_minus_two_calls_ms"] <= res["larger_spread_ms"]
    res["by_position_ms"] = by_pos                                     # the legs alternate: compare like with like
    res["by_position_median_ms"] = {k: {w: round(statistics.median(xs), 4) for w, xs in v.items()} for k, v in by_pos.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=1 << 18, help="192-step blocks per pull")
    br.add_options(ap, "rx_sched_frontend", warmup=None, reps=None, timeout=240, trace="off")
    a = ap.parse_args()
    small = a.blocks < 4096
    if a.warmup is None:
        a.warmup = 20 if small else 3
    if a.reps is None:
        a.reps = 500 if small else 10
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--blocks", str(a.blocks)]
    tag = "rx_sched_frontend_%d" % a.blocks
    res = summarise(br.run_rounds(tag, me, a), a)
    if not a.no_trace:
        res["kernel_trace_us"] = {}
        for leg in ("pull_frontend", "two_calls"):
            rows = br.kernel_trace(tag, me, ["--warmup", "1", "--reps", "3"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if k.startswith(
                ("rx_", "frontend_fused", "save_wide_hist", "pack_trxd_wire", "burst_pull4", "burst_pull_"))}
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["blocks_%d" % a.blocks] = res
    br.write_json(a.out, out)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
