#!/usr/bin/env python3
"""The receive front end per logical channel on one GPU, HIP-event time per pull:
  MULTI   262 144 blocks of 192 wideband steps, (65, 48): the four-row object against chans = 3, 2, 1;
  RESAMP  (65, 96) on 1536-sample chunks and (52, 75) on 1200: the one-pass object against trxhip_convert_short_float +
          trxhip_resample_batch run back to back on the same samples.
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; a round times every leg once, in alternating order.
Medians and each leg's spread (max - min over the rounds) go to profiles/rx_frontend_bench.json, with the fraction of 8 TB/s on
3072 + rows * 260 * 8 B per block (MULTI) and on 4 B in + 8 p / q B out per input sample (RESAMP).

   python3 tools/bench_rx_frontend.py [--rounds 5] [--blocks N] [--warmup W] [--reps R] [--timeout S] [--out FILE]"""
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

PEAK = 8e12
RESAMP = (("65_96", 65, 96, 1536), ("52_75", 52, 75, 1200))


def child(a):
    """One round: every leg once -> one JSON line {leg: ms per call}."""
    import torch
    from osmo_trx_amd import TrxHip, synth, trxhip
    trx = TrxHip(0)
    L, st = trx.L, trx._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    nb = a.blocks
    legs = {}
    wide = synth.make_wideband_stream(nb, "cuda:0")
    n_out = nb * 260
    out = torch.empty((4, n_out), dtype=torch.complex64, device="cuda:0")
    keep = []
    for name, chans in (("four_rows", None), ("chans3", 3), ("chans2", 2), ("chans1", 1)):
        fe = trxhip.RxFrontEnd(trx, 192, 65, 48, chans=chans)
        keep.append(fe)
        legs["multi_" + name] = (None, lambda fe=fe: trxhip._check(
            L.trxhip_rx_frontend_pull(fe.h, ptr(wide), nb, ptr(out), n_out, st), "pull"))
    for tag, p, q, bl in RESAMP:
        n_in = nb * 192 // bl * bl                                     # about as many input samples as one MULTI channel
        g = torch.Generator(device="cuda:0")
        g.manual_seed(p)
        x = torch.randint(-32768, 32768, (n_in, 2), generator=g, device="cuda:0", dtype=torch.int32).to(torch.int16)
        y = torch.empty(n_in // q * p, dtype=torch.complex64, device="cuda:0")
        xf = torch.empty((n_in, 2), dtype=torch.float32, device="cuda:0")
        fe = trxhip.RxFrontEnd(trx, bl, p, q, chans=1, mode="resamp")
        keep.append(fe)
        legs["resamp_%s_one_pass" % tag] = (None, lambda fe=fe, x=x, y=y, n=n_in // bl: trxhip._check(
            L.trxhip_rx_frontend_pull(fe.h, ptr(x), n, ptr(y), y.numel(), st), "pull"))

        def two(x=x, xf=xf, y=y, n_in=n_in, p=p, q=q):
            trxhip._check(L.trxhip_convert_short_float(trx.h, ptr(xf), ptr(x), 2 * n_in, st), "convert")
            trxhip._check(L.trxhip_resample_batch(trx.h, ptr(xf), ptr(y), n_in, p, q, 1, n_in, y.numel(), st), "resample")
        legs["resamp_%s_two_calls" % tag] = (None, two)
    print(json.dumps(br.time_in_order(torch, legs, br.select_legs(legs, a.legs), a)), flush=True)


def summarise(per_leg, a):
    nb = a.blocks
    res = {"workload": "rx_frontend", "blocks": nb, "rounds": a.rounds, "reps": a.reps, "peak_bytes_per_s": PEAK, "legs": {}}

    def leg(name, n_bytes, extra):
        xs = per_leg[name]
        res["legs"][name] = dict(extra, **br.leg_summary(xs, bytes=n_bytes,
                                                         frac_of_8tbs=round(n_bytes / (statistics.median(xs) * 1e-3) / PEAK, 3)))
    for name, rows in (("four_rows", 4), ("chans3", 3), ("chans2", 2), ("chans1", 1)):
        leg("multi_" + name, nb * (3072 + rows * 260 * 8), {"rows": rows, "bytes_per_block": 3072 + rows * 260 * 8})
    for tag, p, q, bl in RESAMP:
        n_in = nb * 192 // bl * bl
        for form in ("one_pass", "two_calls"):                             # both on the one-pass form's algorithmic bytes
            leg("resamp_%s_%s" % (tag, form), n_in * 4 + n_in // q * p * 8, {"p": p, "q": q, "chunk": bl, "samples_in": n_in})
    L = res["legs"]
    res["chans3_minus_four_rows_ms"] = round(L["multi_chans3"]["median_ms"] - L["multi_four_rows"]["median_ms"], 4)
    res["chans3_within_four_rows_spread"] = res["chans3_minus_four_rows_ms"] <= L["multi_four_rows"]["spread_ms"]
    for tag, _, _, _ in RESAMP:
        d = L["resamp_%s_one_pass" % tag]["median_ms"] - L["resamp_%s_two_calls" % tag]["median_ms"]
        res["resamp_%s_one_pass_minus_two_calls_ms" % tag] = round(d, 4)
        res["resamp_%s_within_two_calls_spread" % tag] = d <= L["resamp_%s_two_calls" % tag]["spread_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=1 << 18)
    br.add_options(ap, "rx_frontend", warmup=5, reps=20, timeout=240)
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    res = summarise(br.run_rounds("rx_frontend", [sys.executable, os.path.abspath(__file__), "--blocks", str(a.blocks)], a), a)
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
