#!/usr/bin/env python3
"""The cost of the MS-side FCCH search on one GPU, HIP-event time, int16 buffers of 60 000 samples (the reference's 12
frames of an acquire): 96 slots of a cell from the product's own modulator, the frequency-correction burst in the FCCH slots, each
buffer beginning at another frame of the multiframe.
  b256 / b4096     trxhip_ms_fcch_search_i16 over 256 / 4096 buffers, hits and measurements written; per call, no wait inside
  afc256 / acq256  trxhip_ms_afc_group_acquire_s16 against trxhip_ms_group_acquire_s16 on the same 256 buffers at 0 Hz, each on a
                   group of 256 members of its own; per call, waits included (one in acquire, two in acquire_afc)
Every round is a fresh process under its own time limit; inside a round the legs are timed in turns, the order reversed every other
turn; every timed region follows one untimed call of the same leg.  Median per leg over the rounds, spread = max - min over the
rounds -> profiles/ms_fsearch_bench.json, with the bytes the batch call has to read over its time as a fraction of 8 TB/s and, with
--trace, the kernels of the named legs from a kernel trace in a run of its own.  The first step that fails ends the run.

   python3 tools/bench_ms_fsearch.py [--rounds 5] [--inner I] [--warmup W] [--reps R] [--timeout S] [--trace b256,b4096,afc256] [--out FILE]"""
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
ACQ_LEN = 60000
FRAME = 8 * 625
LEGS = ("b256", "b4096", "afc256", "acq256")
BYTES_PER_SAMPLE = 4


def cell(trx, torch, np):
    """int16[2 * 408 * 625, 2] on the GPU: two 51-multiframes of tools/workloads.multiframe()'s cell, with 148 zero bits -- the
    frequency-correction burst -- in the FCCH slots"""
    from osmo_trx_amd import synth, trxhip
    from workloads import BSIC, TSC
    rng = np.random.default_rng(7)
    fns = np.repeat(np.arange(BASE_FN, BASE_FN + 102), 8)
    tns = np.tile(np.arange(8), 102)
    sent = rng.integers(0, 2, (816, 148), dtype=np.uint8)
    sent[:, :3] = 0
    sent[:, -3:] = 0
    sent[:, 61:87] = [int(c) for c in synth.TSC_BITS[TSC]]
    for b, (f, t) in enumerate(zip(fns, tns)):
        kind = trxhip.ms_slot_kind(int(f), int(t))
        if kind == trxhip.MS_KIND_SCH:
            sent[b] = synth.sch_burst_bits(BSIC, int(f))
        elif kind == trxhip.MS_KIND_FCCH:
            sent[b] = 0
    p = np.zeros(816, dtype=trxhip.TX_PARAMS_DTYPE)
    p["nbits"], p["guard"], p["scale_re"] = 148, 8, 1.0
    _, iq, _ = trx.modulate(torch.from_numpy(sent).to("cuda:0"), trx.tx_params_tensor(p), sps=4, cf32=False, s16_scale=1400.0)
    return iq.reshape(-1, 2)


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    from workloads import BSIC, TSC
    trx = TrxHip(0)
    flat = cell(trx, torch, np)
    names = br.select_legs(list(LEGS), a.legs)
    L, st, vp = trx.L, trx._stream(), C.c_void_p
    score = trxhip.MS_FSEARCH_MIN_SCORE

    def buffers(n):
        return torch.stack([flat[(m % 51) * FRAME:(m % 51) * FRAME + ACQ_LEN] for m in range(n)]).contiguous()

    legs, checks = {}, []
    for n in (256, 4096):
        if "b%d" % n in names:
            bufs = buffers(n)
            hit = torch.zeros((n, 64), dtype=torch.uint8, device="cuda:0")
            fc = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")

            def batch(bufs=bufs, hit=hit, fc=fc, n=n):
                trxhip._check(L.trxhip_ms_fcch_search_i16(trx.h, vp(bufs.data_ptr()), ACQ_LEN, ACQ_LEN, n, score, FULL_SCALE, vp(hit.data_ptr()),
                                                          vp(fc.data_ptr()), st), "fcch search")

            def check(hit=hit, fc=fc, n=n):
                h, f = trx.fsearch_to_numpy(hit, fc)
                assert h["found"].all() and (h["score"] > 0.9).all() and (np.abs(f["hz"] - trxhip.MS_FCCH_BIAS_HZ) < 100.0).all(), n
            legs["b%d" % n] = (batch, 1)
            checks.append(check)
    if "afc256" in names or "acq256" in names:
        n = 256
        bufs = buffers(n)
        members = np.arange(n, dtype=np.uint32)
        ts = np.zeros(n, dtype=np.int64)
        gs = [trxhip.MsRxSchedulerGroup(trx, n=n, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True) for _ in range(2)]
        found = np.zeros((2, n), dtype=np.int32)
        rec = np.zeros((2, n), dtype=trxhip.SCH_SYNC_DTYPE)
        got = [0, 0]

        def afc():
            got[0] = L.trxhip_ms_afc_group_acquire_s16(gs[0].h, members.ctypes.data_as(vp), n, vp(bufs.data_ptr()), ACQ_LEN, ACQ_LEN,
                                                       ts.ctypes.data_as(vp), score, None, None, rec[0].ctypes.data_as(vp),
                                                       found[0].ctypes.data_as(vp), st)

        def acq():
            got[1] = L.trxhip_ms_group_acquire_s16(gs[1].h, members.ctypes.data_as(vp), n, vp(bufs.data_ptr()), ACQ_LEN, ACQ_LEN,
                                                   ts.ctypes.data_as(vp), rec[1].ctypes.data_as(vp), found[1].ctypes.data_as(vp), st)

        def check():
            ran = [i for i, k in enumerate(("afc256", "acq256")) if k in names]
            # (a buffer holds two or three SCH bursts of equal strength and no noise: either call may take any of them)
            for i in ran:
                assert got[i] == n and found[i].all() and (rec[i]["bsic"] == BSIC).all() and (rec[i]["fn"] % 51 % 10 == 1).all(), (i, got)
            if 0 in ran:
                assert all(abs(gs[0].nco_state(m)["hz"]) < 100.0 for m in range(n))
            assert not gs[1].nco_state(0)["enable"]

        legs["afc256"], legs["acq256"] = (afc, 1), (acq, 1)
        checks.append(check)
    names = [k for k in names if k in legs]
    times = br.time_in_turns(torch, legs, names, a, untimed_first=True)
    torch.cuda.synchronize()
    for check in checks:
        check()
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "ms_fsearch", "buf_len": ACQ_LEN, "input": "int16", "rounds": a.rounds, "inner": a.inner, "reps": a.reps,
           "unit": "ms per call (b*: no wait inside; afc256 / acq256: waits included)",
           "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}, "batch_pass": {}, "pairs": {}}
    for n in (256, 4096):
        leg = res["legs"].get("b%d" % n)
        if leg:
            nbytes = n * ACQ_LEN * BYTES_PER_SAMPLE
            res["batch_pass"]["b%d" % n] = dict(buffers=n, bytes=nbytes, fraction_of_8TBps=round(nbytes / 8e12 / (leg["median_ms"] * 1e-3), 4))
    if "afc256" in res["legs"] and "acq256" in res["legs"]:
        res["pairs"]["afc256_over_acq256"] = br.pair(res["legs"], "afc256", "acq256")
        if "b256" in res["legs"]:
            res["search_share_of_acquire_afc"] = round(res["legs"]["b256"]["median_ms"] / res["legs"]["afc256"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    br.add_options(ap, "ms_fsearch", warmup=2, reps=3, timeout=200, inner=6, even_inner=True, trace="legs")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__)]
    res = summarise(br.run_rounds("ms_fsearch", me, a), a)
    if a.trace:
        res["kernel_trace_us"] = {}
        for leg in a.trace.split(","):
            rows = br.kernel_trace("ms_fsearch", me, ["--inner", "2", "--warmup", "1", "--reps", "1"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if re.match(r"ms_fsearch|sch_|ms_nco|ms_fcch", k)}
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
