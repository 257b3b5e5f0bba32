#!/usr/bin/env python3
"""The multi-ARFCN transmit front end on one GPU: RadioInterfaceMulti::pushBuffer over 262 144 blocks of 3 logical channels
(260 low-rate samples per channel and block -> 768 wideband samples), fused (trxhip_tx_frontend_push) against the composition of
the separate calls (Resampler(48, 65) per logical channel into the 4 path rows, trxhip_synthesize_batch, then
trxhip_convert_float_short), with int16 and with cf32 output; and RadioInterfaceResamp::pushBuffer (Resampler(96, 65), int16).

   python3 tools/bench_tx_frontend.py [--blocks N] [--warmup W] [--reps R]
   -> one JSON line: per leg ms per call, Mblocks/s, algorithmic bytes per block (low-rate input read once, output written
      once) and the fraction of 8 TB/s those bytes make."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from osmo_trx_amd import TrxHip, trxhip

PEAK = 8e12
ACTIVE3 = {1: 0, 0: 1, 3: 2}                   # pchan <- lchan with 3 chans (radioInterfaceMulti.cpp:92-124)


def timeit(f, warmup, reps):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        f()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=1 << 18)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    nb, chans = a.blocks, 3
    trx = TrxHip(0)
    L = trx.L
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    x = torch.view_as_complex((torch.randn((chans, nb * 260, 2), generator=g, device="cuda:0") * 2000.0).contiguous())
    scale = float(np.float32(1.0 / chans))
    n_wide = nb * 768
    o_cf = torch.empty(n_wide, dtype=torch.complex64, device="cuda:0")
    o_s16 = torch.empty((n_wide, 2), dtype=torch.int16, device="cuda:0")
    rows = torch.zeros((4, nb * 192), dtype=torch.complex64, device="cuda:0")
    st = trx._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    fused = trxhip.TxFrontEnd(trx, chans=chans)
    resamp = [trxhip.TxFrontEnd(trx, chans=1, mode="resamp") for _ in range(chans)]

    def run_fused(cf32):
        trxhip._check(L.trxhip_tx_frontend_push(fused.h, ptr(x), x.shape[1], nb, ptr(o_cf) if cf32 else None,
                                                None if cf32 else ptr(o_s16), scale, st), "push")

    def run_unfused(cf32):
        for pchan, lchan in ACTIVE3.items():
            trxhip._check(L.trxhip_tx_frontend_push(resamp[lchan].h, ptr(x[lchan]), x.shape[1], nb, ptr(rows[pchan]), None, 1.0, st),
                          "push")
        trxhip._check(L.trxhip_synthesize_batch(trx.h, ptr(rows), rows.shape[1], ptr(o_cf), nb, 4, 192, 16, st), "synthesize")
        if not cf32:
            trxhip._check(L.trxhip_convert_float_short(trx.h, ptr(o_s16), ptr(o_cf), scale, 2 * n_wide, st), "convert")

    r96 = trxhip.TxFrontEnd(trx, chans=1, p=96, q=65, bw=0.45, mode="resamp")
    r_s16 = torch.empty((nb * 384, 2), dtype=torch.int16, device="cuda:0")

    def run_resamp():
        trxhip._check(L.trxhip_tx_frontend_push(r96.h, ptr(x[0]), x.shape[1], nb, None, ptr(r_s16), 1.0, st), "push")

    in_b = chans * 260 * 8
    legs = {
        "fused_s16": (lambda: run_fused(False), in_b + 768 * 4),
        "unfused_s16": (lambda: run_unfused(False), in_b + 768 * 4),
        "fused_cf32": (lambda: run_fused(True), in_b + 768 * 8),
        "unfused_cf32": (lambda: run_unfused(True), in_b + 768 * 8),
        "resamp_96_65_s16": (run_resamp, 260 * 8 + 384 * 4),
    }
    res = {"workload": "tx_frontend", "blocks": nb, "chans": chans, "peak_bytes_per_s": PEAK}
    for name, (f, bpb) in legs.items():
        ms = timeit(f, a.warmup, a.reps)
        res[name] = {"ms": round(ms, 4), "mblocks_per_s": round(nb / ms / 1e3, 2), "bytes_per_block": bpb,
                     "frac_of_8tbs": round(nb * bpb / (ms * 1e-3) / PEAK, 3)}
    res["fused_over_unfused_s16"] = round(res["unfused_s16"]["ms"] / res["fused_s16"]["ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
