#!/usr/bin/env python3
"""The MS-side downlink burst receiver on one GPU, HIP-event time per call, over 262 144 int16 slots with the 51-multiframe mix over
8 TNs (per 408 slots: 5 FCCH, 5 SCH, 398 traffic), all ACTIVE:
  ms_rx   trxhip_ms_rx_batch_i16 over the stream where it lies (slot_stride 625)
  chain   what the tree needed before for the same slots: trxhip_convert_short_float + trxhip_energy_detect_batch_cf32 +
          trxhip_demod_va_batch_cf32 on the traffic slots and trxhip_sch_sync_batch_i16 (TRACK) on the SCH slots, both gathered into
          batches of their own outside the timed region.  Its results differ (the start is clamped to >= 0, there is no RSSI): it is
          context for the time only.
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; inside a round the two legs are timed in turns, `inner` times
each in alternating order, and the round reports each leg's median.  Then one run of its own under rocprofv3 --kernel-trace
--stats gives the kernels' own durations, and tools/resource_usage.sh the compiler's resource report (no GPU).  Medians, each leg's
spread (max - min over the rounds), the trace rows and the resource report go to profiles/ms_rx_bench.json.

   python3 tools/bench_ms_rx.py [--rounds 5] [--slots N] [--inner I] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

FULL_SCALE = 2047.0


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    from workloads import TSC, multiframe
    trx = TrxHip(0)
    base_iq, base_slots, sent, kinds = multiframe(trx, 51 * 4321)
    reps = (a.slots + 407) // 408
    iq = base_iq.repeat(reps, 1, 1)[:a.slots].contiguous()
    slots_np = np.tile(base_slots, reps)[:a.slots].copy()
    slots_np["fn"] += 51 * (np.arange(a.slots, dtype=np.uint32) // 408)        # the multiframes follow one another
    d_slots = trx.ms_slots_tensor(slots_np)
    kind_all = np.tile(kinds, reps)[:a.slots]
    # the chain's inputs: traffic and SCH slots in batches of their own (gathered here, not in the timed region)
    t_idx = torch.from_numpy(np.nonzero(kind_all == trxhip.MS_KIND_NB)[0]).to("cuda:0")
    s_idx = torch.from_numpy(np.nonzero(kind_all == trxhip.MS_KIND_SCH)[0]).to("cuda:0")
    iq_t, iq_s = iq[t_idx].contiguous(), iq[s_idx].contiguous()
    nt, ns = iq_t.shape[0], iq_s.shape[0]
    params = np.zeros(nt, dtype=trxhip.PARAMS_DTYPE)
    params["type"], params["tsc"], params["max_toa"] = trxhip.TSC, TSC, 3
    d_params = trx.params_tensor(params)
    L, st = trx.L, trx._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    # preallocated outputs: no allocation or download inside the timed region
    ind = torch.empty((a.slots, 32), dtype=torch.uint8, device="cuda:0")
    bits = torch.empty((a.slots, 148), dtype=torch.int8, device="cuda:0")
    xf = torch.empty((nt, 625, 2), dtype=torch.float32, device="cuda:0")
    energy = torch.empty(nt, dtype=torch.float32, device="cuda:0")
    soft = torch.empty((nt, 156), dtype=torch.float32, device="cuda:0")
    starts = torch.empty(nt, dtype=torch.int32, device="cuda:0")
    rec_s = torch.empty((ns, 24), dtype=torch.uint8, device="cuda:0")
    bits_s = torch.empty((ns, 148), dtype=torch.int8, device="cuda:0")
    scale = 1.0 / FULL_SCALE

    def ms_rx():
        trxhip._check(L.trxhip_ms_rx_batch_i16(trx.h, ptr(iq), 625, ptr(d_slots), ptr(ind), ptr(bits), a.slots, FULL_SCALE, st), "ms_rx")

    def chain():
        trxhip._check(L.trxhip_convert_short_float(trx.h, ptr(xf), ptr(iq_t), nt * 625 * 2, st), "convert")
        trxhip._check(L.trxhip_energy_detect_batch_cf32(trx.h, ptr(xf), nt, 625, 80, ptr(energy), st), "energy")
        trxhip._check(L.trxhip_demod_va_batch_cf32(trx.h, ptr(xf), ptr(d_params), None, ptr(soft), ptr(starts), nt, 625, scale, 156, 0, st),
                      "va")
        trxhip._check(L.trxhip_sch_sync_batch_i16(trx.h, ptr(iq_s), 625, ptr(rec_s), ptr(bits_s), ns, 625, trxhip.SCH_SYNC_TRACK, scale, st),
                      "sch")

    legs = {"ms_rx": (ms_rx, 1), "chain": (chain, 1)}
    names = br.select_legs(legs, a.legs)
    times = br.time_in_turns(torch, legs, names, a)
    # the timed calls received what was sent
    if "ms_rx" in names:
        r = ind.cpu().numpy().reshape(-1).view(trxhip.MS_IND_DTYPE)
        b = bits.cpu().numpy()
        assert np.array_equal(r["kind"], kind_all) and (r["sent"] == 1).all(), "slot kinds"
        sch = kind_all == trxhip.MS_KIND_SCH
        assert (r["sch_rc"][sch] == 1).all() and (r["sch_fn"][sch] % 51 == slots_np["fn"][sch] % 51).all(), "SCH slots did not decode"
        dem = (kind_all[:408] != trxhip.MS_KIND_FCCH)
        assert np.array_equal(b[:408][dem], np.where(sent[dem] > 0, -127, 127)), "the bits are not the ones sent"
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "ms_rx", "slots": a.slots, "slot_len": 625, "mix_per_408": {"fcch": 5, "sch": 5, "traffic": 398}, "input": "int16",
           "rounds": a.rounds, "inner": a.inner, "reps": a.reps, "legs": {}}
    for name, xs in per_leg.items():
        res["legs"][name] = br.leg_summary(xs, us_per_slot=round(statistics.median(xs) * 1e3 / a.slots, 5))
    res["chain_over_ms_rx"] = round(res["legs"]["chain"]["median_ms"] / res["legs"]["ms_rx"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    br.add_options(ap, "ms_rx", warmup=2, reps=3, timeout=180, inner=5, trace="off")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots)]
    res = summarise(br.run_rounds("ms_rx", me, a), a)
    if not a.no_trace:
        res["kernel_trace_us"] = {}
        for leg in ("ms_rx", "chain"):
            rows = {k: v for k, v in sorted(br.kernel_trace("ms_rx", me, ["--inner", "1", "--warmup", "1", "--reps", "3"], leg, a).items())
                    if re.match(r"ms_rx|sch_sync|va_demod|energy|convert", k)}
            for v in rows.values():
                v["ns_per_slot"] = round(v["avg_us"] * 1e3 / a.slots, 3)
            res["kernel_trace_us"][leg] = rows
    res["resource_usage"] = br.resource_usage("trx_ms_rx.hip", "ms_rx")
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
