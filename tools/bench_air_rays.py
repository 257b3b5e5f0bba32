#!/usr/bin/env python3
"""The cost of the air interface's multipath rays on one GPU, HIP-event time per call, against what a caller had
before them: torch.repeat_interleave of the rows plus the object as it was with one member per ray (N R <= 4096), and on the
downlink that object's N R rows summed per member in torch.  The composition makes the same bytes on the uplink.
  shapes   s64 / s512: that many members x 6 static rays x 8 slots (5000 samples); s8long: 8 x 6 static x 32 768 slots;
           r64: 64 x 16 rotating rays (air_rays' Jakes set at 200 Hz) x 8 slots; r8long: 8 x 16 rotating x 32 768 slots;
           z64 / z8long: r64 / r8long with the same rays at 0 Hz -- static against rotating rays on one shape
  legs     ul_dense_S / ul_sparse_S: AirChannel.uplink() under rays on dense rows / one TN in 8 occupied; dl_S (s shapes):
           AirChannel.downlink(); c_*: the composition on the same tensors
Every round is a fresh process under its own time limit; inside a round the legs are timed in turns, the order reversed every other
turn.  Median per leg over the rounds, spread = max - min over the rounds -> profiles/air_rays_bench.json, with each rays leg
against its composition (bar: not slower beyond the composition's spread), the bytes the definition must move (N n 4 + n 4) over
the rays time as a fraction of 8 TB/s, rotating over static and, with --trace, the kernels of the named legs from a kernel trace
in a run of its own.  The first step that fails ends the run.

   python3 tools/bench_air_rays.py [--rounds 5] [--inner I] [--warmup W] [--reps R] [--timeout S] [--trace ul_dense_r64,...] [--out FILE]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

LONG = 32768 * 625
# members, rays, samples, Doppler of the rays (None: static rays with spread delays), downlink legs too
SHAPES = {"s64": (64, 6, 5000, None, True), "s512": (512, 6, 5000, None, True), "s8long": (8, 6, LONG, None, True),
          "r64": (64, 16, 5000, 200.0, False), "r8long": (8, 16, LONG, 200.0, False),
          "z64": (64, 16, 5000, 0.0, False), "z8long": (8, 16, LONG, 0.0, False)}
KINDS = ("ul_sparse", "ul_dense", "dl")
LEGS = tuple(p + k + "_" + s for s, v in SHAPES.items() for k in KINDS if k != "dl" or v[4] for p in ("", "c_"))
MAX_DELAY = 64
RMS = 12.0


def rays_of(trxhip, np, m, n_rays, doppler):
    """member m's rays, phase 0 (what set_path at end_ts 0 gives the composition's members)"""
    if doppler is None:
        rng = np.random.default_rng(1000 + m)
        r = np.zeros(n_rays, dtype=trxhip.AIR_RAY_DTYPE)
        r["gain"] = 1.0 / np.sqrt(n_rays)
        r["delay"] = np.sort(rng.integers(0, MAX_DELAY + 1, n_rays))
        return r
    r = trxhip.air_rays([0.0], [0.0], doppler_hz=doppler, sinusoids=n_rays, seed=m)
    r["phase"] = 0
    return r


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    trx = TrxHip(0)
    names = br.select_legs(list(LEGS), a.legs)
    legs, checks = {}, []
    dev = "cuda:0"
    UL, DL = trxhip.AIR_UL, trxhip.AIR_DL
    for s, (n_members, n_rays, n, doppler, _) in SHAPES.items():
        mine = [k for k in names if k.endswith("_" + s)]
        if not mine:
            continue
        dirs = [d for d, tag in ((UL, "ul_"), (DL, "dl_")) if any(tag in k for k in mine)]
        air = trxhip.AirChannel(trx, n_members, MAX_DELAY, 1)
        comp = trxhip.AirChannel(trx, n_members * n_rays, MAX_DELAY, 1) if any(k.startswith("c_") for k in mine) else None
        scale = 1.0 / np.sqrt(n_members)
        for m in range(n_members):
            r = rays_of(trxhip, np, m, n_rays, doppler)
            for d in dirs:
                q = r.copy()
                if d == UL:
                    q["gain"] *= scale
                air.set_rays(d, m, q)
                if comp is not None:
                    for k in range(n_rays):
                        comp.set_path(d, m * n_rays + k, float(q["gain"][k]), int(q["delay"][k]), float(q["hz"][k]))
        for o in (air, comp):
            if o is not None:
                o.set_noise(UL, 0, RMS)
        for m in range(n_members if DL in dirs else 0):
            air.set_noise(DL, m, RMS)
        g = torch.Generator(device=dev).manual_seed(5)
        t = torch.arange(n, device=dev)
        rows = {}
        if any("ul_dense" in k for k in mine):
            rows["ul_dense"] = torch.randint(-2047, 2048, (n_members, n, 2), generator=g, device=dev, dtype=torch.int16)
        if any("ul_sparse" in k for k in mine):
            on = ((t // 625) % 8)[None, :] == (torch.arange(n_members, device=dev) % 8)[:, None]
            rows["ul_sparse"] = torch.randint(-2047, 2048, (n_members, n, 2), generator=g, device=dev, dtype=torch.int16) * on[:, :, None]
            del on
        del t
        x_dl = torch.randint(-2047, 2048, (n, 2), generator=g, device=dev, dtype=torch.int16)
        out = {k: torch.empty((n, 2), dtype=torch.int16, device=dev) for k in ("ul", "c_ul")}
        out_dl = torch.empty((n_members, n, 2), dtype=torch.int16, device=dev) if "dl_" + s in mine else None
        out_cdl = torch.empty((n_members * n_rays, n, 2), dtype=torch.int16, device=dev) if "c_dl_" + s in mine else None
        at = {}

        def rays_ul(r, air=air, at=at, n=n, out=out["ul"]):
            air.uplink(r, at.setdefault("ul", 0), out=out)
            at["ul"] += n

        def comp_ul(r, comp=comp, at=at, n=n, out=out["c_ul"], n_rays=n_rays):
            comp.uplink(torch.repeat_interleave(r, n_rays, dim=0), at.setdefault("c_ul", 0), out=out)
            at["c_ul"] += n

        def rays_dl(air=air, at=at, n=n, x=x_dl, out=out_dl):
            air.downlink(x, at.setdefault("dl", 0), out=out)
            at["dl"] += n

        def comp_dl(comp=comp, at=at, n=n, x=x_dl, out=out_cdl, n_members=n_members, n_rays=n_rays):
            comp.downlink(x, at.setdefault("c_dl", 0), out=out)
            at["c_dl"] += n
            return out.view(n_members, n_rays, n, 2).sum(1, dtype=torch.int32).clamp_(-32768, 32767).to(torch.int16)

        for k in ("ul_sparse", "ul_dense"):
            if k + "_" + s in mine:
                legs[k + "_" + s] = (lambda r=rows[k], f=rays_ul: f(r), 1)
            if "c_" + k + "_" + s in mine:
                legs["c_" + k + "_" + s] = (lambda r=rows[k], f=comp_ul: f(r), 1)
        if "dl_" + s in mine:
            legs["dl_" + s] = (rays_dl, 1)
        if "c_dl_" + s in mine:
            legs["c_dl_" + s] = (comp_dl, 1)

        def check(s=s, mine=mine, rows=rows, n=n, n_rays=n_rays, air=air, comp=comp):
            # from one timestamp on: the composition's uplink bytes are the rays'
            k = next((k for k in ("ul_dense", "ul_sparse") if k + "_" + s in mine and "c_" + k + "_" + s in mine), None)
            if k is not None and n <= 5000:
                for o in (air, comp):
                    o.reset(UL, 0)
                y = air.uplink(rows[k], 0)
                assert torch.equal(y, comp.uplink(torch.repeat_interleave(rows[k], n_rays, dim=0), 0)) and bool(y.any()), s
        checks.append(check)
    names = [k for k in names if k in legs]
    times = br.time_in_turns(torch, legs, names, a)
    torch.cuda.synchronize()
    for check in checks:
        check()
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "air_rays", "shapes": {s: dict(members=v[0], rays=v[1], samples=v[2], doppler_hz=v[3]) for s, v in SHAPES.items()},
           "max_delay": MAX_DELAY, "rounds": a.rounds, "inner": a.inner, "reps": a.reps,
           "unit": "ms per call, HIP events around the calls of a turn", "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()},
           "pairs": {}, "uplink_bytes": {}, "rotating_over_static": {}}
    L = res["legs"]
    for s, v in SHAPES.items():
        for k in KINDS:
            f, c = k + "_" + s, "c_" + k + "_" + s
            if f in L and c in L:
                p = br.pair(L, f, c)
                p["bar_met"] = L[f]["median_ms"] <= L[c]["median_ms"] + L[c]["spread_ms"]
                res["pairs"][f + "_over_composition"] = p
            if k != "dl" and f in L:
                nbytes = v[0] * v[2] * 4 + v[2] * 4
                res["uplink_bytes"][f] = dict(bytes=nbytes, fraction_of_8TBps=round(nbytes / 8e12 / (L[f]["median_ms"] * 1e-3), 4))
            z = k + "_z" + s[1:]
            if s[0] == "r" and f in L and z in L:
                res["rotating_over_static"][f] = br.pair(L, f, z)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    br.add_options(ap, "air_rays", warmup=2, reps=5, timeout=300, inner=4, even_inner=True, trace="legs")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__)]
    if a.legs:
        me += ["--legs", a.legs]
    res = summarise(br.run_rounds("air_rays", me, a), a)
    if a.trace:
        res["kernel_trace_us"] = {}
        for leg in a.trace.split(","):
            rows = br.kernel_trace("air_rays", [sys.executable, os.path.abspath(__file__)], ["--inner", "2", "--warmup", "1", "--reps", "2"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if re.match(r"air_", k)}
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
