#!/usr/bin/env python3
"""Downlink burst scheduler throughput (trxhip_tx_sched_render, tx_render_kernel) against tx_modulate_kernel on the same bursts.
Every slot of a 4-SPS channel carries a GMSK burst (148 bits), so the render does the modulator's work plus the placement.
  render   : device time of one render of N slots (rows upload + slot words + kernel), timed with events while a device sleep
             covers the host's planning; slots/s and the fraction of 8 TB/s on the bytes moved per slot: 5000 (cf32) or
             2500 (int16) written + 4 (slot word) + 464 (staged datagram row, read)
  modulate : trxhip_modulate_trxd_batch over the same N datagrams into N x 625 rows (the same store volume)
  planner  : host wall time of render() per 1000 slots with N queued bursts (planning, slot words, launch)
Prints one JSON line.  Kernel-only durations: rocprofv3 --kernel-trace --memory-copy-trace --stats -- python3
tools/bench_tx_sched.py --modes cf32 (tx_render_kernel and tx_modulate_kernel<true> then both write cf32 rows; the memory-copy
trace shows the staged-row upload)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from osmo_trx_amd import TrxHip, trxhip

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="cf32,s16", help="render outputs to time: cf32, s16 (the modulator runs cf32 rows)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    n = a.slots
    trx = TrxHip(0)
    dev = "cuda:0"
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, (n, 148)).astype(np.uint8)
    s = trxhip.TxScheduler(trx, chans=1, sps=4, filler=trxhip.FILLER_DUMMY, full_scale=32767.0, queue_cap=n, max_slots=n)
    s.set_clock(0, 0)
    for tn in range(8):
        s.set_slot(0, tn, 1)
    out = torch.empty((1, n * 625), dtype=torch.complex64, device=dev)
    s16 = torch.empty((1, n * 625, 2), dtype=torch.int16, device=dev)
    stream = trx._stream()
    vp = trxhip._VP
    res = {"slots": n, "steps": a.steps}

    def submit_window():
        fn0, tn0 = s.clock()
        assert tn0 == 0
        hdr = np.zeros(6, np.uint8)
        sub = trx.L.trxhip_tx_sched_submit
        buf = np.zeros(154, np.uint8)
        for k in range(n):
            fn = (fn0 + k // 8) % 2715648
            buf[0] = k % 8
            buf[1:5] = np.frombuffer(int(fn).to_bytes(4, "big"), np.uint8)
            buf[5] = 0
            buf[6:] = bits[k]
            assert sub(s.h, 0, buf.ctypes.data_as(vp), 154, None) == 0
        del hdr

    for mode in a.modes.split(","):
        dev_ms, host_ms = [], []
        for step in range(a.warmup + a.steps):
            submit_window()
            torch.cuda.synchronize()
            torch.cuda._sleep(int(2e9))                    # the device waits while the host plans: events time the device work
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            if mode == "cf32":
                rc = trx.L.trxhip_tx_sched_render(s.h, n, vp(out.data_ptr()), n * 625, None, None, stream)
            else:
                sc = (trxhip.C.c_float * 1)(1.0)
                rc = trx.L.trxhip_tx_sched_render(s.h, n, None, n * 625, vp(s16.data_ptr()), sc, stream)
            t1 = time.perf_counter()
            e1.record()
            assert rc == 0, rc
            torch.cuda.synchronize()
            if step >= a.warmup:
                dev_ms.append(e0.elapsed_time(e1))
                host_ms.append((t1 - t0) * 1e3)
        if max(host_ms) > 900:
            res[mode + "_note"] = "host planning may have outlasted the device sleep"
        ms = float(np.median(dev_ms))
        nbytes = (5000 if mode == "cf32" else 2500) + 4 + 464
        res[mode + "_render_ms"] = round(ms, 4)
        res[mode + "_slots_s"] = round(n / (ms * 1e-3), 1)
        res[mode + "_bytes_per_slot"] = nbytes
        res[mode + "_frac_8tbs"] = round(n * nbytes / (ms * 1e-3) / HBM, 4)
        res[mode + "_planner_ms_per_1000_slots"] = round(float(np.median(host_ms)) / n * 1000, 4)

    # the modulator on the same datagrams
    D = np.zeros((n, 154), np.uint8)
    D[:, 0] = np.arange(n) % 8
    D[:, 6:] = bits
    dg = torch.from_numpy(D).to(dev)
    dl = torch.full((n,), 154, dtype=torch.int16, device=dev)
    rows = out.view(n, 625)
    info = torch.empty((n, 16), dtype=torch.uint8, device=dev)

    def mod():
        return trx.L.trxhip_modulate_trxd_batch(trx.h, vp(dg.data_ptr()), 154, vp(dl.data_ptr()), 32767.0, 4, vp(rows.data_ptr()), vp(0),
                                                0.0, 625, vp(info.data_ptr()), n, stream)
    for _ in range(a.warmup):
        assert mod() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        mod()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    res["modulate_ms"] = round(ms, 4)
    res["modulate_bursts_s"] = round(n / (ms * 1e-3), 1)
    if "cf32_render_ms" in res:
        res["render_over_modulate"] = round(res["cf32_render_ms"] / ms, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
