#!/usr/bin/env python3
"""The cost of the air interface on one GPU, HIP-event time per call, against what a caller had before it: a
composition of torch ops on the same tensors -- int16 -> float, the per-member shift (one gather with a prepared index), the
phasor (polar of a phase ramp), the complex multiply, the sum over the members, randn noise, round, clamp, int16.  The composition
makes the same kind of stream, not the same bits; the fused call is never its own yardstick.
  shapes   n64 / n256 / n4096: that many members x 8 slots (5000 samples); n8long: 8 members x 32 768 slots
  legs     ul_sparse_S / ul_dense_S: AirChannel.uplink() on rows with one TN in 8 occupied / dense; dl_S: AirChannel.downlink();
           t_ul_sparse_S / t_ul_dense_S / t_dl_S: the torch composition on the same tensors
Every round is a fresh process under its own time limit; inside a round the legs are timed in turns, the order reversed every other
turn.  Median per leg over the rounds, spread = max - min over the rounds -> profiles/air_bench.json, with each fused leg against
its composition (bar: not slower beyond the composition's spread), the bytes the definition must move (N n 4 + n 4) over the
fused time as a fraction of 8 TB/s and, with --trace, the kernels of the named legs from a kernel trace in a run of its own.  The
first step that fails ends the run.

   python3 tools/bench_air.py [--rounds 5] [--inner I] [--warmup W] [--reps R] [--timeout S] [--trace ul_dense_n4096,...] [--out FILE]"""
import argparse
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

SHAPES = {"n64": (64, 5000), "n256": (256, 5000), "n4096": (4096, 5000), "n8long": (8, 32768 * 625)}
KINDS = ("ul_sparse", "ul_dense", "dl")
LEGS = tuple(p + k + "_" + s for s in SHAPES for k in KINDS for p in ("", "t_"))
MAX_DELAY = 64
SAMPLE_HZ = 13e6 / 12.0
RMS = 12.0


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    trx = TrxHip(0)
    names = br.select_legs(list(LEGS), a.legs)
    legs, checks = {}, []
    dev = "cuda:0"
    for s, (n_members, n) in SHAPES.items():
        mine = [k for k in names if k.endswith("_" + s)]
        if not mine:
            continue
        rng = np.random.default_rng(n_members)
        delay = rng.integers(0, MAX_DELAY + 1, n_members)
        hz = rng.uniform(-3000.0, 3000.0, n_members)
        gain = np.full(n_members, 1.0 / math.sqrt(n_members))
        air = trxhip.AirChannel(trx, n_members, MAX_DELAY, 1)
        for d in (trxhip.AIR_UL, trxhip.AIR_DL):
            for m in range(n_members):
                air.set_path(d, m, gain[m] if d == trxhip.AIR_UL else 1.0, int(delay[m]), hz[m])
                air.set_noise(d, m, RMS)
        g = torch.Generator(device=dev).manual_seed(5)
        t = torch.arange(n, device=dev)
        idx = (t[None, :] - torch.from_numpy(delay).to(dev)[:, None]).clamp_(min=0)        # the shift: one gather index, prepared
        w = torch.from_numpy(2 * math.pi * hz / SAMPLE_HZ).to(dev, torch.float32)
        tf = t.to(torch.float32)
        rows = {}
        if any("ul_dense" in k for k in mine):
            rows["ul_dense"] = torch.randint(-2047, 2048, (n_members, n, 2), generator=g, device=dev, dtype=torch.int16)
        if any("ul_sparse" in k for k in mine):
            on = ((t // 625) % 8)[None, :] == (torch.arange(n_members, device=dev) % 8)[:, None]
            rows["ul_sparse"] = torch.randint(-2047, 2048, (n_members, n, 2), generator=g, device=dev, dtype=torch.int16) * on[:, :, None]
            del on
        x_dl = torch.randint(-2047, 2048, (n, 2), generator=g, device=dev, dtype=torch.int16)
        out_ul = torch.empty((n, 2), dtype=torch.int16, device=dev)
        out_dl = torch.empty((n_members, n, 2), dtype=torch.int16, device=dev) if any(k.endswith("dl_" + s) for k in mine) else None
        at = {trxhip.AIR_UL: 0, trxhip.AIR_DL: 0}

        def fused_ul(r, air=air, at=at, n=n, out=out_ul):
            air.uplink(r, at[trxhip.AIR_UL], out=out)
            at[trxhip.AIR_UL] += n

        def fused_dl(air=air, at=at, n=n, x=x_dl, out=out_dl):
            air.downlink(x, at[trxhip.AIR_DL], out=out)
            at[trxhip.AIR_DL] += n

        def finish(y):
            return torch.view_as_real(y).round_().clamp_(-32768, 32767).to(torch.int16)

        def rot(g_, w=w, tf=tf):
            return torch.polar(g_[:, None].expand(-1, tf.shape[0]), w[:, None] * tf[None, :])

        g_ul = torch.from_numpy(gain).to(dev, torch.float32)
        g_dl = torch.ones(n_members, device=dev)

        def torch_ul(r, idx=idx, n=n, rot=rot, g_ul=g_ul):
            z = torch.view_as_complex(r.to(torch.float32))
            y = (torch.gather(z, 1, idx) * rot(g_ul)).sum(0)
            return finish(y + torch.randn(n, dtype=torch.complex64, device=dev) * (RMS * math.sqrt(2.0)))

        def torch_dl(x=x_dl, idx=idx, n=n, n_members=n_members, rot=rot, g_dl=g_dl):
            z = torch.view_as_complex(x.to(torch.float32))
            y = z[idx] * rot(g_dl)
            return finish(y + torch.randn((n_members, n), dtype=torch.complex64, device=dev) * (RMS * math.sqrt(2.0)))

        for k in ("ul_sparse", "ul_dense"):
            if k + "_" + s in mine:
                legs[k + "_" + s] = (lambda r=rows[k], f=fused_ul: f(r), 1)
            if "t_" + k + "_" + s in mine:
                legs["t_" + k + "_" + s] = (lambda r=rows[k], f=torch_ul: f(r), 1)
        if "dl_" + s in mine:
            legs["dl_" + s] = (fused_dl, 1)
        if "t_dl_" + s in mine:
            legs["t_dl_" + s] = (torch_dl, 1)

        def check(out_ul=out_ul, out_dl=out_dl, mine=mine, s=s, torch_dl=torch_dl):
            # the fused outputs are a stream of the composition's kind: about the same power
            if "ul_dense_" + s in mine or "ul_sparse_" + s in mine:
                assert out_ul.any()
            if out_dl is not None and "dl_" + s in mine:
                p = out_dl[:4].to(torch.float32).pow(2).mean().item()
                q = torch_dl()[:4].to(torch.float32).pow(2).mean().item()
                assert 0.8 < p / q < 1.25, (s, p, q)
        checks.append(check)
    names = [k for k in names if k in legs]
    times = br.time_in_turns(torch, legs, names, a)
    torch.cuda.synchronize()
    for check in checks:
        check()
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "air", "shapes": {s: dict(members=m, samples=n) for s, (m, n) in SHAPES.items()}, "max_delay": MAX_DELAY,
           "rounds": a.rounds, "inner": a.inner, "reps": a.reps, "unit": "ms per call, HIP events around the calls of a turn",
           "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}, "pairs": {}, "uplink_bytes": {}}
    for s, (m, n) in SHAPES.items():
        for k in KINDS:
            f, t = k + "_" + s, "t_" + k + "_" + s
            if f in res["legs"] and t in res["legs"]:
                p = br.pair(res["legs"], f, t)
                p["bar_met"] = res["legs"][f]["median_ms"] <= res["legs"][t]["median_ms"] + res["legs"][t]["spread_ms"]
                res["pairs"][f + "_over_torch"] = p
            if k != "dl" and f in res["legs"]:
                nbytes = m * n * 4 + n * 4
                res["uplink_bytes"][f] = dict(bytes=nbytes, fraction_of_8TBps=round(nbytes / 8e12 / (res["legs"][f]["median_ms"] * 1e-3), 4))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    br.add_options(ap, "air", warmup=2, reps=5, timeout=300, inner=4, even_inner=True, trace="legs")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__)]
    res = summarise(br.run_rounds("air", me, a), a)
    if a.trace:
        res["kernel_trace_us"] = {}
        for leg in a.trace.split(","):
            rows = br.kernel_trace("air", me, ["--inner", "2", "--warmup", "1", "--reps", "2"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if re.match(r"air_", k)}
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
