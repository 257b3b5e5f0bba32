#!/usr/bin/env python3
"""Transmit-side throughput: tx_modulate_kernel over N 4-SPS GMSK bursts (148 bits, out_stride 625) in three modes
  cf32  trxhip_modulate_batch, complex64 rows            s16  the same, int16 rows only
  trxd  trxhip_modulate_trxd_batch over 6 + 148-byte TRXD datagrams, complex64 rows
timed with device events after a warm-up.  Prints one JSON line; per mode: Mbursts/s, the algorithmic bytes per burst
(computed from the shapes: what the launch must read and write at least) and the fraction of 8 TB/s that makes:
  {"n": N, "cf32_mbursts_s": ..., "cf32_bytes_per_burst": ..., "cf32_frac_8tbs": ..., "s16_...": ..., "trxd_...": ...}
Usable under `tools/measure.py ab --field cf32_mbursts_s -- python3 tools/bench_tx.py`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from osmo_trx_amd import TrxHip, trxhip

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="cf32,s16,trxd")
    a = ap.parse_args()
    trx = TrxHip(0)
    dev = "cuda:0"
    n, L = a.n, 625
    gen = torch.Generator(device=dev).manual_seed(7)
    bits = torch.randint(0, 2, (n, 148), generator=gen, device=dev, dtype=torch.uint8)
    tn = np.arange(n) % 8
    params = trx.tx_params_tensor(trxhip.tx_params_host(148, 8 + (tn % 4 == 0)))
    hdr = torch.zeros((n, 6), dtype=torch.uint8, device=dev)
    hdr[:, 0] = torch.from_numpy(tn.astype(np.uint8)).to(dev)
    dgrams = torch.cat([hdr, bits], dim=1).contiguous()
    dlen = torch.full((n,), 154, dtype=torch.int16, device=dev)

    out = torch.empty((n, L), dtype=torch.complex64, device=dev)
    s16 = torch.empty((n, L, 2), dtype=torch.int16, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    stream = trx._stream()
    vp = trxhip._VP

    def cf32():
        return trx.L.trxhip_modulate_batch(trx.h, vp(bits.data_ptr()), 148, vp(params.data_ptr()), vp(out.data_ptr()), vp(0), 0.0, L,
                                           vp(lens.data_ptr()), n, 4, stream)

    def s16_only():
        return trx.L.trxhip_modulate_batch(trx.h, vp(bits.data_ptr()), 148, vp(params.data_ptr()), vp(0), vp(s16.data_ptr()), 8192.0,
                                           L, vp(lens.data_ptr()), n, 4, stream)

    def trxd():
        return trx.L.trxhip_modulate_trxd_batch(trx.h, vp(dgrams.data_ptr()), 154, vp(dlen.data_ptr()), 32767.0, 4,
                                                vp(out.data_ptr()), vp(0), 0.0, L, vp(info.data_ptr()), n, stream)

    # algorithmic bytes per burst: inputs read + outputs written, from the shapes
    modes = {
        "cf32": (cf32, 148 + 16 + L * 8 + 4),
        "s16": (s16_only, 148 + 16 + L * 4 + 4),
        "trxd": (trxd, 154 + 2 + L * 8 + 16),
    }
    res = {"n": n, "steps": a.steps}
    for m in a.modes.split(","):
        fn, nbytes = modes[m]
        for _ in range(a.warmup):
            assert fn() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        rate = n / (ms * 1e-3)
        res[m + "_ms"] = round(ms, 4)
        res[m + "_mbursts_s"] = round(rate / 1e6, 2)
        res[m + "_bytes_per_burst"] = nbytes
        res[m + "_frac_8tbs"] = round(rate * nbytes / HBM, 4)
    assert int((lens[:8] == L).sum()) == 8 or "cf32" not in a.modes
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
