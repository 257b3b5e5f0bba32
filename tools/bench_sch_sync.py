#!/usr/bin/env python3
"""The MS-side SCH receiver on one GPU, HIP-event time per call:
  track          trxhip_sch_sync_batch_cf32, TRACK: 262 144 slots of 625 samples
  acq            trxhip_sch_sync_batch_cf32, ACQ: 256 buffers of 60 000 samples (the reference's 12 frames)
and, for context only (they do different work), on the same buffers
  detect_full    trxhip_detect_sch_batch_cf32 FULL over the slots    (detectSCHBurst: stops at a TOA)
  va_demod       trxhip_demod_va_batch_cf32 over the slots           (normal-burst MLSE: 59 lags, no channel decoder)
  detect_buffer  trxhip_detect_sch_batch_cf32 BUFFER over the buffers
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; a round times every leg once, in alternating order.  Then one
run of its own under rocprofv3 --kernel-trace --stats gives the kernels' own durations, and tools/resource_usage.sh the compiler's
resource report of the new kernels (no GPU).  Medians, each leg's spread (max - min over the rounds), the trace rows and the
resource report go to profiles/sch_sync_bench.json.

   python3 tools/bench_sch_sync.py [--rounds 5] [--slots N] [--bufs N] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ACQ_LEN = 60000


def child(a):
    """One round: every leg once -> one JSON line {leg: ms per call}."""
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, synth, trxhip
    trx = TrxHip(0)
    # distinct bursts made once and repeated: no kernel's time depends on the data
    base, truth = synth.make_sch_buffers(min(1024, a.slots), "cuda:0", trxhip.SCH_SYNC_TRACK, trx)
    slots = base.repeat((a.slots + base.shape[0] - 1) // base.shape[0], 1)[:a.slots].contiguous()
    bbase, btruth = synth.make_sch_buffers(min(16, a.bufs), "cuda:0", trxhip.SCH_SYNC_ACQ, trx, buf_len=ACQ_LEN)
    bufs = bbase.repeat((a.bufs + bbase.shape[0] - 1) // bbase.shape[0], 1)[:a.bufs].contiguous()
    params = np.zeros(a.slots, dtype=trxhip.PARAMS_DTYPE)
    params["type"], params["max_toa"] = trxhip.TSC, 3
    d_params = trx.params_tensor(params)
    scale = 1.0 / 2047.0
    # the legs launch into preallocated outputs through the C ABI: no allocation or download inside the timed region
    L, st = trx.L, trx._stream()
    import ctypes as C
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rec_s = torch.empty((a.slots, 24), dtype=torch.uint8, device="cuda:0")
    rec_b = torch.empty((a.bufs, 24), dtype=torch.uint8, device="cuda:0")
    res_s = torch.empty((a.slots, 32), dtype=torch.uint8, device="cuda:0")
    res_b = torch.empty((a.bufs, 32), dtype=torch.uint8, device="cuda:0")
    soft = torch.empty((a.slots, 156), dtype=torch.float32, device="cuda:0")
    starts = torch.empty(a.slots, dtype=torch.int32, device="cuda:0")

    def track():
        trxhip._check(L.trxhip_sch_sync_batch_cf32(trx.h, ptr(slots), 625, ptr(rec_s), None, a.slots, 625, trxhip.SCH_SYNC_TRACK, scale,
                                                   st), "track")

    def acq():
        trxhip._check(L.trxhip_sch_sync_batch_cf32(trx.h, ptr(bufs), ACQ_LEN, ptr(rec_b), None, a.bufs, ACQ_LEN, trxhip.SCH_SYNC_ACQ, scale,
                                                   st), "acq")

    def detect_full():
        trxhip._check(L.trxhip_detect_sch_batch_cf32(trx.h, ptr(slots), ptr(res_s), a.slots, 625, 4, trxhip.SCH_DETECT_FULL, 4.0, st), "full")

    def detect_buffer():
        trxhip._check(L.trxhip_detect_sch_batch_cf32(trx.h, ptr(bufs), ptr(res_b), a.bufs, ACQ_LEN, 4, trxhip.SCH_DETECT_BUFFER, 4.0, st),
                      "buffer")

    def va_demod():
        trxhip._check(L.trxhip_demod_va_batch_cf32(trx.h, ptr(slots), ptr(d_params), None, ptr(soft), ptr(starts), a.slots, 625,
                                                   1.0 / 16383.0, 156, 0, st), "va")

    legs = {"track": track, "acq": acq, "detect_full": detect_full, "detect_buffer": detect_buffer, "va_demod": va_demod}
    names = [k for k in legs if not a.legs or k in a.legs.split(",")]
    if a.round % 2:
        names.reverse()
    out = {}
    for name in names:
        f = legs[name]
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
    # the timed calls decoded what was sent
    r = rec_s.cpu().numpy().reshape(-1).view(trxhip.SCH_SYNC_DTYPE)[:base.shape[0]]
    rb = rec_b.cpu().numpy().reshape(-1).view(trxhip.SCH_SYNC_DTYPE)[:bbase.shape[0]]
    if "track" in names:
        assert (r["rc"] == 1).all() and np.array_equal(r["fn"], truth["fn"]), "TRACK did not decode its bursts"
    if "acq" in names:
        assert (rb["rc"] == 1).all() and np.array_equal(rb["fn"], btruth["fn"]), "ACQ did not decode its bursts"
    print(json.dumps(out), flush=True)


def resource_usage():
    """{kernel: {VGPRs, SGPRs spill, VGPRs spill, scratch bytes/lane, LDS bytes/block, occupancy}} from tools/resource_usage.sh"""
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "resource_usage.sh"), "trx_sch_sync.hip", "sch_"], stdout=subprocess.PIPE,
                         text=True, check=True).stdout
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "lds_bytes_per_block", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for line in txt.splitlines():
        m = re.match(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip() or m.group(1)
            cur = out.setdefault(name.split("(")[0].replace("void ", ""), {})
            continue
        m = re.match(r"\s+([^:]+): (\d+)$", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--bufs", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per round")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sch_sync_bench.json"))
    ap.add_argument("--logs", default=os.path.join(ROOT, "build", "measure"))
    ap.add_argument("--round", type=int, default=None, help=argparse.SUPPRESS)     # child: run one round on the GPU
    ap.add_argument("--legs", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    if a.rounds < 5:
        ap.error("at least five rounds")
    import measure
    from bench_rx_sched import trace_rows
    os.makedirs(a.logs, exist_ok=True)
    per_leg = {}
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots), "--bufs", str(a.bufs)]
    for r in range(a.rounds):
        log = os.path.join(a.logs, "sch_sync_round_%d.log" % (r + 1))
        measure.step("round %d" % (r + 1), me + ["--round", str(r), "--warmup", str(a.warmup), "--reps", str(a.reps)], log, a.timeout)
        for k, v in measure.last_json(log).items():
            per_leg.setdefault(k, []).append(v)
        print("round %d done" % (r + 1), flush=True)
    units = {"track": a.slots, "detect_full": a.slots, "va_demod": a.slots, "acq": a.bufs, "detect_buffer": a.bufs}
    res = {"workload": "sch_sync", "slots": a.slots, "slot_len": 625, "bufs": a.bufs, "buf_len": ACQ_LEN, "rounds": a.rounds,
           "reps": a.reps, "legs": {}}
    for name, xs in per_leg.items():
        med = statistics.median(xs)
        res["legs"][name] = dict(median_ms=round(med, 4), spread_ms=round(max(xs) - min(xs), 4), ms=[round(x, 4) for x in xs],
                                 us_per_unit=round(med * 1e3 / units[name], 4))
    if not a.no_trace:
        d = os.path.join(a.logs, "sch_sync_trace")
        res["kernel_trace_us"] = {}
        for leg in ("track", "acq"):                                       # one trace per mode: both run sch_sync_demod_kernel
            shutil.rmtree(d, ignore_errors=True)
            measure.step("kernel trace " + leg, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o",
                                                 "sch_sync", "--"] + me + ["--round", "0", "--warmup", "1", "--reps", "3", "--legs", leg],
                         os.path.join(a.logs, "sch_sync_trace_%s.log" % leg), a.timeout)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(trace_rows(d).items()) if k.startswith("sch_")}
        shutil.rmtree(d, ignore_errors=True)
    res["resource_usage"] = resource_usage()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
