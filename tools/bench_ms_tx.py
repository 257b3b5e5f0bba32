#!/usr/bin/env python3
"""The MS-side uplink burst scheduler on one GPU against the row modulator the tree had before it, HIP-event time around the
render (the submit that queues the bursts runs before the first event: its copy is not what is compared), int16 out:
  dense      one trxhip_ms_tx_render_s16 of `slots` slots with a burst on all 8 TNs (slots bursts)
  dense_rows trxhip_modulate_batch, int16 rows, over the same bursts (bits and descriptors on the device)
  sparse     one render of `slots` slots with a burst on one TN in 8 (slots / 8 bursts): the MS's usual load
  sparse_rows trxhip_modulate_batch over those slots / 8 bursts (it writes an eighth of the window)
  fill       writing the window once (zero_ of the same tensor)
  dense8     51 consecutive renders of 8 slots, all 8 TNs carrying a burst, per render
  rows8      51 times trxhip_modulate_batch on 8 bursts, per call
With rxtx_delay 0 and timing advance 0 the bursts lie on the slot grid of the window, so the dense stream must equal the rows
byte for byte (checked after the timing).  The render's time includes its host planning (segments, retiring): the device idles
behind the first event while the host plans.
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; inside a round the legs are timed in turns, in alternating
order, and the round reports each leg's median.  Then one run per leg under rocprofv3 --kernel-trace --stats gives the kernels'
durations.  Medians, spreads (max - min over the rounds) and the trace rows go to profiles/ms_tx_bench.json.

   python3 tools/bench_ms_tx.py [--rounds 5] [--slots N] [--inner I] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
import argparse
import json
import os
import re
import shutil
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FULL_SCALE = 2047
BASE_FN = 51 * 4321


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    trx = TrxHip(0)
    n = a.slots
    assert n % 8 == 0 and n >= 51 * 8
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (n, 148)).astype(np.uint8)
    # request k is heard in slot k of the window: its target after incTN(3) is the clock k slots on, the window starts at the clock
    k = np.arange(n)
    fn, tn = BASE_FN + (k - 3) // 8, (k - 3) % 8
    pwr = (k * 3) % 30
    reqs = {"dense": trxhip.ms_tx_requests(fn, tn, pwr, bits), "sparse": trxhip.ms_tx_requests(fn[5::8], tn[5::8], pwr[5::8], bits[5::8])}
    small = 51 * 8
    reqs["dense8"] = reqs["dense"][3:3 + small].copy()               # the first three lie behind the clock: start at slot 3
    L, st = trx.L, trx._stream()
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    window = torch.empty((n * 625, 2), dtype=torch.int16, device="cuda:0")
    rows = torch.empty((n, 625, 2), dtype=torch.int16, device="cuda:0")
    d_bits = torch.from_numpy(bits).to("cuda:0")
    tx = trxhip.MsTxScheduler(trx, tx_full_scale=FULL_SCALE, rxtx_delay=0, max_pending=n)
    scale = np.array([np.float32(float(FULL_SCALE) * 10.0 ** -j) for j in range(3)])[pwr // 10]      # driveTx()'s expression
    d_par = trx.tx_params_tensor(trxhip.tx_params_host(148, 8 + (tn % 4 == 0), 0, scale, n=n))
    d_bits_s, d_par_s = d_bits[5::8].contiguous(), d_par[5::8].contiguous()
    d_len = torch.empty(n, dtype=torch.int32, device="cuda:0")
    nd = C.c_size_t()
    now = [0]                                                       # every window lies behind the last one

    def submit(name):
        now[0] += (n + 16) * 625
        plan = tx.submit(reqs[name], (BASE_FN, 0, now[0]))
        assert (plan["status"][3 if name == "dense" else 0:] == trxhip.MS_TX_QUEUED).all(), np.bincount(plan["status"])

    def render(n_slots, first_slot=0):
        trxhip._check(L.trxhip_ms_tx_render_s16(tx.h, ptr(window, first_slot * 2500), n_slots * 625, now[0] + first_slot * 625,
                                                C.byref(nd), st), "render")

    def modulate(b, p, out, cnt):
        trxhip._check(L.trxhip_modulate_batch(trx.h, b, 148, p, None, out, 1.0, 625, ptr(d_len), cnt, 4, st), "modulate")

    # (prepare, timed call, calls per timed call)
    legs = {
        "dense": (lambda: submit("dense"), lambda: render(n), 1),
        "dense_rows": (None, lambda: modulate(ptr(d_bits), ptr(d_par), ptr(rows), n), 1),
        "sparse": (lambda: submit("sparse"), lambda: render(n), 1),
        "sparse_rows": (None, lambda: modulate(ptr(d_bits_s), ptr(d_par_s), ptr(rows), n // 8), 1),
        "fill": (None, lambda: window.zero_(), 1),
        "dense8": (lambda: submit("dense8"), lambda: [render(8, 3 + 8 * j) for j in range(51)], 51),
        "rows8": (None, lambda: [modulate(ptr(d_bits, (3 + 8 * j) * 148), ptr(d_par, (3 + 8 * j) * 16), ptr(rows, (3 + 8 * j) * 2500), 8)
                                 for j in range(51)], 51),
    }
    names = [x for x in legs if not a.legs or x in a.legs.split(",")]
    times = {x: [] for x in names}

    def run(name, timed):
        prep, call, per = legs[name]
        total = 0.0
        for _ in range(a.reps if timed else a.warmup):
            if prep:
                prep()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            call()
            ev[1].record()
            torch.cuda.synchronize()
            total += ev[0].elapsed_time(ev[1])
        return total / max(a.reps, 1) / per

    for name in names:
        run(name, False)
    for i in range(a.inner):
        for name in (names if (a.round + i) % 2 == 0 else names[::-1]):
            times[name].append(run(name, True))
    # the dense stream is the rows, slot for slot (the first three requests lie behind the clock: zeros)
    if "dense" in names and "dense_rows" in names:
        submit("dense")
        render(n)
        modulate(ptr(d_bits), ptr(d_par), ptr(rows), n)
        torch.cuda.synchronize()
        assert nd.value == n - 3
        w = window.view(n, 625, 2)
        assert torch.equal(w[3:], rows[3:]) and not w[:3].any(), "the rendered stream differs from the row modulator's"
        assert rows[3:].any()
    if "sparse" in names and "dense_rows" in names:
        submit("sparse")
        render(n)
        torch.cuda.synchronize()
        w = window.view(n // 8, 8, 625, 2)
        assert nd.value == n // 8 and torch.equal(w[:, 5], rows.view(n // 8, 8, 625, 2)[:, 5]) and not w[:, :5].any() and not w[:, 6:].any()
    st_ = tx.state()
    assert st_["pending"] == 0 and st_["missed"] == 0 and st_["overlap"] == 0 and st_["expired"] == 0, st_
    print(json.dumps({x: statistics.median(v) for x, v in times.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--inner", type=int, default=5, help="turns per leg inside a round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per round")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_tx_bench.json"))
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
        log = os.path.join(a.logs, "ms_tx_round_%d.log" % (r + 1))
        measure.step("round %d" % (r + 1), me + ["--round", str(r), "--inner", str(a.inner), "--warmup", str(a.warmup), "--reps",
                                                 str(a.reps)], log, a.timeout)
        for k, v in measure.last_json(log).items():
            per_leg.setdefault(k, []).append(v)
        print("round %d done" % (r + 1), flush=True)
    res = {"workload": "ms_tx", "slots": a.slots, "small_render_slots": 8, "slot_len": 625, "output": "int16", "rounds": a.rounds,
           "inner": a.inner, "reps": a.reps, "legs": {}}
    for name, xs in per_leg.items():
        med = statistics.median(xs)
        res["legs"][name] = dict(median_ms=round(med, 4), spread_ms=round(max(xs) - min(xs), 4), ms=[round(x, 4) for x in xs])
    lg = res["legs"]
    res["dense_over_rows"] = round(lg["dense"]["median_ms"] / lg["dense_rows"]["median_ms"], 4)
    res["sparse_over_fill"] = round(lg["sparse"]["median_ms"] / lg["fill"]["median_ms"], 4)
    res["dense8_over_rows8"] = round(lg["dense8"]["median_ms"] / lg["rows8"]["median_ms"], 4)
    if not a.no_trace:
        d = os.path.join(a.logs, "ms_tx_trace")
        res["kernel_trace_us"] = {}
        for leg in ("dense", "dense_rows", "sparse"):
            shutil.rmtree(d, ignore_errors=True)
            measure.step("kernel trace " + leg, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ms_tx",
                                                 "--"] + me + ["--round", "0", "--inner", "1", "--warmup", "1", "--reps", "3", "--legs", leg],
                         os.path.join(a.logs, "ms_tx_trace_%s.log" % leg), a.timeout)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(trace_rows(d).items()) if re.match(r"ms_tx_render|tx_modulate", k)}
        shutil.rmtree(d, ignore_errors=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
