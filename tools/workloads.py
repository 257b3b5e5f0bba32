#!/usr/bin/env python3
"""One definition of every measured workload: the synth batches (and seeds) behind the tools' timings and counter passes.

   python tools/workloads.py NAME [--n N] [--warmup W] [--reps R] [--no-split] [--hint]
   -> {"workload", "n", "ms", "mbursts_per_s"}: HIP-event time of one launch after W warm ones (units: bursts; buffers for
      sch_*, 768-sample blocks for frontend).  `tools/measure.py ab --field mbursts_per_s` compares it across builds;
      `tools/measure.py pmc -- python3 tools/workloads.py NAME` profiles it.

Burst workloads (detect + demod, 1 Mi bursts): normal (BASELINE.json configs[1]), rach / ext (configs[2] access bursts),
mixed (configs[4]: 7:1 normal / access), edge (8-PSK, 444 soft bits), 1sps (configs[0] geometry, TSC 0), cf32 (normal
bursts as complex64), exact (normal, exact demodulator), va (normal, Viterbi alternative), nb_toa63 / nb_toa112 (normal
bursts spread over 60 symbols of delay, max_toa 63 / 112: the windowed path), mixed_blocked (mixed, the access bursts moved
to the end of the batch).  Others: sch_full (detectSCHBurst FULL, 16384 x 625 samples), sch_buffer (BUFFER search,
256 x 60000 samples), frontend (configs[3]: channelizer, resampler and the fused front end over 256 Ki blocks), tx_frontend
(the transmit front end: 3 logical channels through trxhip_tx_frontend_push to int16, 256 Ki blocks of 260 samples).
multiframe(): the 51-multiframe of a cell behind the MS-side benches (tools/bench_ms_*.py)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from osmo_trx_amd import TrxHip, synth, trxhip

NAMES = ("normal", "rach", "ext", "mixed", "edge", "1sps", "cf32", "exact", "va", "nb_toa63", "nb_toa112", "mixed_blocked",
         "sch_full", "sch_buffer", "frontend", "tx_frontend")
DEFAULT_N = {"sch_full": 16384, "sch_buffer": 256, "frontend": 1 << 18, "tx_frontend": 1 << 18}
TSC = 5                                 # the cell of multiframe()
BSIC = 0o52


def make(name, n, device="cuda:0", seed=None):
    """(iq, host params or None, keywords of the launch) of workload `name` with n units on `device`; seed=None: synth's own."""
    s = {} if seed is None else {"seed": seed}
    kw = {"sps": 4, "soft_stride": 148}
    if name in ("normal", "exact", "cf32", "va"):
        iq, p, _ = synth.make_normal_bursts(n, device, 4, **s)
        if name in ("cf32", "va"):
            iq = torch.view_as_complex(iq.to(torch.float32)).contiguous()
        if name == "exact":
            kw["exact"] = True
    elif name in ("nb_toa63", "nb_toa112"):
        iq, p, _ = synth.make_normal_bursts(n, device, 4, max_toa=63, delay_sym=(0.0, 60.0), **s)
        p["max_toa"] = int(name[6:])
    elif name in ("rach", "ext"):
        iq, p, _ = synth.make_access_bursts(n, device, ext=name == "ext", **s)
    elif name in ("mixed", "mixed_blocked"):
        iq, p = synth.make_mixed_bursts(n, device, **s)
        if name == "mixed_blocked":
            idx = np.concatenate([np.flatnonzero(np.arange(n) % 8 != 7), np.flatnonzero(np.arange(n) % 8 == 7)])
            iq, p = iq[torch.from_numpy(idx).to(iq.device)].contiguous(), p[idx]
    elif name == "edge":
        iq, p, _ = synth.make_edge_bursts(n, device, **s)
        kw["soft_stride"] = 444
    elif name == "1sps":
        iq, p, _ = synth.make_normal_bursts(n, device, 1, burst_len=156, tsc=0, **s)
        kw["sps"] = 1
    elif name in ("sch_full", "sch_buffer"):
        g = torch.Generator(device=device)
        g.manual_seed(7 if seed is None else seed)
        x = torch.randn((n, 625 if name == "sch_full" else 60000, 2), generator=g, device=device) * 1000.0
        iq, p = torch.view_as_complex(x.contiguous()), None
        kw = {"state": trxhip.SCH_DETECT_FULL if name == "sch_full" else trxhip.SCH_DETECT_BUFFER}
    elif name == "frontend":
        iq, p, kw = synth.make_wideband_stream(n, device, **s), None, {}
    elif name == "tx_frontend":
        g = torch.Generator(device=device)
        g.manual_seed(5 if seed is None else seed)
        x = torch.randn((3, n * 260, 2), generator=g, device=device) * 2000.0
        iq, p, kw = torch.view_as_complex(x.contiguous()), None, {}
    else:
        raise ValueError(f"unknown workload {name!r} (one of {', '.join(NAMES)})")
    return iq, p, kw


def launcher(trx, name, iq, params, kw, hint=False):
    """A callable that runs one launch of the workload (outputs allocated once, outside it)."""
    if name.startswith("sch_"):
        return lambda: trx.detect_sch(iq, **kw)
    if name == "frontend":
        n = iq.shape[0] // 768                                  # 4 channels x 192 samples per block
        ch = trx.channelize(iq, n)
        x = ch[:, :ch.shape[1] // 48 * 48].contiguous()
        fe = trxhip.RxFrontEnd(trx)

        def run():
            trx.channelize(iq, n)
            trx.resample(x, 65, 48)
            return fe.pull(iq, n)
        return run
    if name == "tx_frontend":
        n = iq.shape[1] // 260
        fe = trxhip.TxFrontEnd(trx, chans=3)
        return lambda: fe.push(iq, n, cf32=False, s16_scale=float(np.float32(1.0 / 3)))
    dp = trx.params_tensor(params)
    if name == "va":
        return lambda: trx.demod_va(iq, dp)
    res = torch.empty((iq.shape[0], 32), dtype=torch.uint8, device=iq.device)
    soft = torch.empty((iq.shape[0], kw["soft_stride"]), dtype=torch.float32, device=iq.device)
    h = trxhip.few_nb_hint(params) if hint else None
    return lambda: trx.detect_demod(iq, dp, results=res, soft=soft, hint=h, **kw)


def multiframe(trx, base_fn, seed=7):
    """One 51-multiframe of a cell as the radio delivers it: (int16[408, 625, 2] on the GPU, MS_SLOT_DTYPE[408], sent bits
    uint8[408, 148], kinds).  SCH and normal bursts come through the product's own modulator; FCCH slots hold a random burst."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("name", choices=NAMES)
    ap.add_argument("--n", type=int, default=None, help="units per launch (default 1 Mi bursts; see above)")
    ap.add_argument("--warmup", type=int, default=60, help="untimed launches first (settled clocks)")
    ap.add_argument("--reps", type=int, default=20, help="timed launches")
    ap.add_argument("--no-split", action="store_true", help="the general kernel alone (no normal-burst kernel)")
    ap.add_argument("--hint", action="store_true", help="pass the few-normal-bursts hint worked out from the host params")
    a = ap.parse_args()
    n = a.n or DEFAULT_N.get(a.name, 1 << 20)
    trx = TrxHip(0)
    if a.no_split:
        trx.set_nb_kernel(False)
    iq, params, kw = make(a.name, n)
    f = launcher(trx, a.name, iq, params, kw, a.hint)
    for _ in range(a.warmup):
        f()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(a.reps):
        f()
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / max(1, a.reps)
    print(json.dumps({"workload": a.name, "n": n, "ms": round(ms, 4), "mbursts_per_s": round(n / ms / 1e3, 3)}), flush=True)


if __name__ == "__main__":
    main()
