#!/usr/bin/env python3
"""The uplink burst scheduler's Viterbi-equaliser flow (RxScheduler(use_va=True)) on one GPU, HIP-event time per call, against
the composition the tree had before it on the same samples -- the host pipe's launch list for cfg->use_va
(csrc/trx_hostpipe.cpp: zero the shift rows, copy every slot into them 20 samples on, trxhip_detect_demod_batch without soft
output, trxhip_convert_short_float, trxhip_energy_detect_batch_cf32, trxhip_demod_va_batch_cf32,
trxhip_apply_diversity_power, trxhip_pack_trxd_wire_batch) with params and meta already resident.  The zeroing and the 2-D copy
are torch's (Tensor.zero_, a strided copy_) in place of hipMemsetAsync / hipMemcpy2DAsync: the same bytes moved.
  composition    those calls back to back over the slots as rows
  pull           steady state: every pull carries one sample over, so slot 0 is the assembled straddling row
Sizes: one pull of --slots slots (262 144) and pulls of 8 slots, one channel, int16 and complex64 input; normal bursts of the
scheduler's TSC 20 samples into their slots, combination I on every TN.
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; a round times every leg once, in alternating order.  Then one
run of the large pulls under rocprofv3 --kernel-trace --stats gives the kernels' own durations and the two new kernels' share
of a pull's kernel time.  Medians, spreads (max - min over the rounds) and the trace rows go to profiles/rx_sched_va_bench.json.

   python3 tools/bench_rx_sched_va.py [--rounds 5] [--slots N] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
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
SMALL = 8


def child(a):
    """One round: every leg of every size and format once -> one JSON line {"<fmt>_<slots>": {leg: ms per call}}."""
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, synth, trxhip
    trx = TrxHip(0)
    L, st = trx.L, trx._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    big = a.slots
    iq, params, _ = synth.make_normal_bursts(big, "cuda:0", 4, tsc=TSC, max_toa=30)
    x16 = torch.zeros((big * 625 + 1, 2), dtype=torch.int16, device="cuda:0")
    x16[:big * 625] = torch.roll(iq, 20, dims=1).view(big * 625, 2)
    del iq
    meta = np.zeros(big, dtype=trxhip.TRXD_META_DTYPE)
    meta["fn"], meta["tn"], meta["version"] = np.arange(big) // 8, np.arange(big) % 8, 1
    d_params = trx.params_tensor(params)
    d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1, 8).copy()).to("cuda:0")
    res = torch.empty((big, 32), dtype=torch.uint8, device="cuda:0")
    soft = torch.empty((big, 148), dtype=torch.float32, device="cuda:0")
    pkt = torch.empty((big, 160), dtype=torch.uint8, device="cuda:0")
    plen = torch.empty(big, dtype=torch.int16, device="cuda:0")
    ind = torch.empty((big, 32), dtype=torch.uint8, device="cuda:0")
    energy = torch.empty(big, dtype=torch.float32, device="cuda:0")
    out = {}
    order = [(f, n) for n in (big, SMALL) for f in ("s16", "cf32") if not a.legs or "%s_%d" % (f, n) in a.legs.split(",")]
    for fmt, n in order:
        cf32 = fmt == "cf32"
        total = n * 625
        x = torch.view_as_complex(x16[:total + 1].to(torch.float32)) if cf32 else x16[:total + 1]
        rows = x[:total].view(n, 625) if cf32 else x[:total].view(n, 625, 2)
        shift = torch.empty_like(rows)
        cf = rows if cf32 else torch.empty((n, 625), dtype=torch.complex64, device="cuda:0")
        detect = L.trxhip_detect_demod_batch_cf32 if cf32 else L.trxhip_detect_demod_batch
        s = trxhip.RxScheduler(trx, chans=1, tsc=TSC, max_slots=n, use_va=True)
        for tn in range(8):
            s.set_slot(0, tn, 1)
        s.set_trxd_version(0, 1)

        def composition():
            shift.zero_()
            shift[:, :585] = rows[:, 20:605]
            trxhip._check(detect(trx.h, ptr(shift), ptr(d_params), ptr(res), None, n, 625, 4, 4.0, 32767.0, 148, 0, st), "detect")
            if not cf32:
                trxhip._check(L.trxhip_convert_short_float(trx.h, ptr(cf), ptr(rows), n * 1250, st), "convert")
            trxhip._check(L.trxhip_energy_detect_batch_cf32(trx.h, ptr(cf), n, 625, 80, ptr(energy), st), "energy")
            trxhip._check(L.trxhip_demod_va_batch_cf32(trx.h, ptr(cf), ptr(d_params), ptr(res), ptr(soft), None, n, 625, 1.0 / 16383.0,
                                                       148, trxhip.FLAG_SLICE, st), "demod_va")
            trxhip._check(L.trxhip_apply_diversity_power(trx.h, ptr(res), ptr(d_params), ptr(energy), n, 32767.0, st), "power")
            trxhip._check(L.trxhip_pack_trxd_wire_batch(trx.h, ptr(res), ptr(d_params), ptr(soft), 148, ptr(d_meta), ptr(pkt), 160,
                                                        ptr(plen), n, 0.0, st), "pack")

        pull_fn = L.trxhip_rx_sched_pull_cf32 if cf32 else L.trxhip_rx_sched_pull_s16

        def pull(n_samples=total):
            trxhip._check(pull_fn(s.h, ptr(x), n_samples, n_samples, ptr(pkt), 160, ptr(plen), ptr(ind), ptr(soft), n, None, None, st),
                          "pull")

        def start_steady():
            s.set_clock(0, 0)
            pull(total + 1)                                            # leaves one sample: the next pulls of `total` cut n slots each

        legs = {"composition": (None, composition), "pull": (start_steady, pull)}
        out["%s_%d" % (fmt, n)] = br.time_in_order(torch, legs, list(legs), a, reps=a.reps if n == big else 20 * a.reps)
        s.close()
        del shift, cf, x, rows
    print(json.dumps(out), flush=True)


def summarise(per, a):
    """per: {"<fmt>_<slots>": [{leg: ms} per round]}"""
    res = {"workload": "rx_sched_va", "chans": 1, "rounds": a.rounds, "reps": a.reps, "cases": {}}
    for case, rounds in per.items():
        n = int(case.split("_")[1])
        c = {"slots": n, "legs": {}}
        for name in rounds[0]:
            xs = [r[name] for r in rounds]
            c["legs"][name] = br.leg_summary(xs, ns_per_slot=round(statistics.median(xs) * 1e6 / n, 2))
        c["pull_minus_composition_ms"] = round(c["legs"]["pull"]["median_ms"] - c["legs"]["composition"]["median_ms"], 4)
        res["cases"][case] = c
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    br.add_options(ap, "rx_sched_va", warmup=2, reps=5, timeout=240, trace="off")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots)]
    res = summarise(br.run_rounds("rx_sched_va", me, a), a)
    if not a.no_trace:
        rows = br.kernel_trace("rx_sched_va", me, ["--warmup", "1", "--reps", "3"], "s16_%d,cf32_%d" % (a.slots, a.slots), a)
        keep = ("rx_", "va_demod", "energy_detect", "convert_short", "diversity_power", "pack_trxd_wire", "nb_pull4", "burst_pull4")
        res["kernel_trace_us"] = {k: v for k, v in sorted(rows.items()) if k.startswith(keep)}
        # the two new kernels' own durations as shares of the large pull of their format (the detect kernels, the packer and the
        # scheduler's small kernels also run in the composition and in the other format's pull: their rows are averages over all)
        shares = {}
        for fmt, t in (("s16", "<unsigned int>"), ("cf32", "<HIP_vector_type<float, 2u>")):
            pull_ms = res["cases"]["%s_%d" % (fmt, a.slots)]["legs"]["pull"]["median_ms"]
            for k, v in rows.items():
                if k.startswith("rx_va_") and t in k:
                    shares[k] = dict(avg_us=v["avg_us"], share_of_pull=round(v["avg_us"] / 1e3 / pull_ms, 4))
        res["new_kernels"] = shares
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
