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
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

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

    legs = {"track": (None, track), "acq": (None, acq), "detect_full": (None, detect_full), "detect_buffer": (None, detect_buffer),
            "va_demod": (None, va_demod)}
    names = br.select_legs(legs, a.legs)
    out = br.time_in_order(torch, legs, names, a)
    # the timed calls decoded what was sent
    r = rec_s.cpu().numpy().reshape(-1).view(trxhip.SCH_SYNC_DTYPE)[:base.shape[0]]
    rb = rec_b.cpu().numpy().reshape(-1).view(trxhip.SCH_SYNC_DTYPE)[:bbase.shape[0]]
    if "track" in names:
        assert (r["rc"] == 1).all() and np.array_equal(r["fn"], truth["fn"]), "TRACK did not decode its bursts"
    if "acq" in names:
        assert (rb["rc"] == 1).all() and np.array_equal(rb["fn"], btruth["fn"]), "ACQ did not decode its bursts"
    print(json.dumps(out), flush=True)


def summarise(per_leg, a):
    units = {"track": a.slots, "detect_full": a.slots, "va_demod": a.slots, "acq": a.bufs, "detect_buffer": a.bufs}
    res = {"workload": "sch_sync", "slots": a.slots, "slot_len": 625, "bufs": a.bufs, "buf_len": ACQ_LEN, "rounds": a.rounds,
           "reps": a.reps, "legs": {}}
    for name, xs in per_leg.items():
        res["legs"][name] = br.leg_summary(xs, us_per_unit=round(statistics.median(xs) * 1e3 / units[name], 4))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--bufs", type=int, default=256)
    br.add_options(ap, "sch_sync", warmup=2, reps=5, timeout=240, trace="off")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots), "--bufs", str(a.bufs)]
    res = summarise(br.run_rounds("sch_sync", me, a), a)
    if not a.no_trace:
        res["kernel_trace_us"] = {}
        for leg in ("track", "acq"):                                       # one trace per mode: both run sch_sync_demod_kernel
            rows = br.kernel_trace("sch_sync", me, ["--warmup", "1", "--reps", "3"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if k.startswith("sch_")}
    res["resource_usage"] = br.resource_usage("trx_sch_sync.hip", "sch_")
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
