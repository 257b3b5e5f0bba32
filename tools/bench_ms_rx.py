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
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FULL_SCALE = 2047.0
TSC = 5
BSIC = 0o52


def multiframe(trx, base_fn, seed=7):
    """One 51-multiframe of a cell as the radio delivers it: (int16[408, 625, 2] on the GPU, MS_SLOT_DTYPE[408], sent bits
    uint8[408, 148], kinds).  SCH and normal bursts come through the product's own modulator; FCCH slots hold a random burst."""
    import numpy as np
    import torch
    from osmo_trx_amd import synth, trxhip
    rng = np.random.default_rng(seed)
    fns = np.repeat(np.arange(base_fn, base_fn + 51), 8)
    tns = np.tile(np.arange(8), 51)
    kinds = np.array([trxhip.ms_slot_kind(int(f), int(t)) for f, t in zip(fns, tns)])
    sent = rng.integers(0, 2, (408, 148), dtype=np.uint8)
    sent[:, :3] = 0
    sent[:, -3:] = 0
    sent[:, 61:87] = [int(c) for c in synth.TSC_BITS[TSC]]
    for b in np.nonzero(kinds == trxhip.MS_KIND_SCH)[0]:
        sent[b] = synth.sch_burst_bits(BSIC, int(fns[b]))
    p = np.zeros(408, dtype=trxhip.TX_PARAMS_DTYPE)
    p["nbits"], p["guard"], p["scale_re"] = 148, 8, 1.0
    _, iq, _ = trx.modulate(torch.from_numpy(sent).to("cuda:0"), trx.tx_params_tensor(p), sps=4, cf32=False, s16_scale=1400.0)
    slots = np.zeros(408, dtype=trxhip.MS_SLOT_DTYPE)
    slots["fn"], slots["tn"], slots["tsc"], slots["flags"] = fns, tns, TSC, trxhip.MS_SLOT_ACTIVE
    return iq, slots, sent, kinds


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
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

    legs = {"ms_rx": ms_rx, "chain": chain}
    names = [k for k in legs if not a.legs or k in a.legs.split(",")]
    times = {k: [] for k in names}
    for name in names:
        for _ in range(a.warmup):
            legs[name]()
    torch.cuda.synchronize()
    for i in range(a.inner):
        for name in (names if (a.round + i) % 2 == 0 else names[::-1]):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(a.reps):
                legs[name]()
            ev[1].record()
            torch.cuda.synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]) / a.reps)
    # the timed calls received what was sent
    if "ms_rx" in names:
        r = ind.cpu().numpy().reshape(-1).view(trxhip.MS_IND_DTYPE)
        b = bits.cpu().numpy()
        assert np.array_equal(r["kind"], kind_all) and (r["sent"] == 1).all(), "slot kinds"
        sch = kind_all == trxhip.MS_KIND_SCH
        assert (r["sch_rc"][sch] == 1).all() and (r["sch_fn"][sch] % 51 == slots_np["fn"][sch] % 51).all(), "SCH slots did not decode"
        dem = (kind_all[:408] != trxhip.MS_KIND_FCCH)
        assert np.array_equal(b[:408][dem], np.where(sent[dem] > 0, -127, 127)), "the bits are not the ones sent"
    print(json.dumps({k: statistics.median(v) for k, v in times.items()}), flush=True)


def resource_usage():
    """{kernel: {...}} from tools/resource_usage.sh"""
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "resource_usage.sh"), "trx_ms_rx.hip", "ms_rx"], stdout=subprocess.PIPE,
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
    ap.add_argument("--inner", type=int, default=5, help="turns per leg inside a round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per round")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_rx_bench.json"))
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
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots)]
    for r in range(a.rounds):
        log = os.path.join(a.logs, "ms_rx_round_%d.log" % (r + 1))
        measure.step("round %d" % (r + 1), me + ["--round", str(r), "--inner", str(a.inner), "--warmup", str(a.warmup), "--reps",
                                                 str(a.reps)], log, a.timeout)
        for k, v in measure.last_json(log).items():
            per_leg.setdefault(k, []).append(v)
        print("round %d done" % (r + 1), flush=True)
    res = {"workload": "ms_rx", "slots": a.slots, "slot_len": 625, "mix_per_408": {"fcch": 5, "sch": 5, "traffic": 398}, "input": "int16",
           "rounds": a.rounds, "inner": a.inner, "reps": a.reps, "legs": {}}
    for name, xs in per_leg.items():
        med = statistics.median(xs)
        res["legs"][name] = dict(median_ms=round(med, 4), spread_ms=round(max(xs) - min(xs), 4), ms=[round(x, 4) for x in xs],
                                 us_per_slot=round(med * 1e3 / a.slots, 5))
    res["chain_over_ms_rx"] = round(res["legs"]["chain"]["median_ms"] / res["legs"]["ms_rx"]["median_ms"], 3)
    if not a.no_trace:
        d = os.path.join(a.logs, "ms_rx_trace")
        res["kernel_trace_us"] = {}
        for leg in ("ms_rx", "chain"):
            shutil.rmtree(d, ignore_errors=True)
            measure.step("kernel trace " + leg, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ms_rx",
                                                 "--"] + me + ["--round", "0", "--inner", "1", "--warmup", "1", "--reps", "3", "--legs", leg],
                         os.path.join(a.logs, "ms_rx_trace_%s.log" % leg), a.timeout)
            rows = {k: v for k, v in sorted(trace_rows(d).items())
                    if re.match(r"ms_rx|sch_sync|va_demod|energy|convert", k)}
            for v in rows.values():
                v["ns_per_slot"] = round(v["avg_us"] * 1e3 / a.slots, 3)
            res["kernel_trace_us"][leg] = rows
        shutil.rmtree(d, ignore_errors=True)
    res["resource_usage"] = resource_usage()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
