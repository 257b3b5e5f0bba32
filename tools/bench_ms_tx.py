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
--nco times the uplink oscillator instead (results under "ms_tx" in profiles/ms_tx_nco_bench.json): dense / sparse / dense8 as
above on an object with the oscillator off, dense_nco / sparse_nco / dense8_nco the same requests on an object with it on
(+2000 Hz, the rotating instance of the kernel), fill, and
  dense_comp the composition the fused render is defined by, on resident rows: trxhip_modulate_batch to complex64,
             trxhip_ms_nco_batch_cf32, trxhip_convert_float_short over the same `slots` bursts (it moves every sample three times)
The dense_nco stream must equal dense_comp's rows byte for byte (checked after the timing).
With rxtx_delay 0 and timing advance 0 the bursts lie on the slot grid of the window, so the dense stream must equal the rows
byte for byte (checked after the timing).  The render's time includes its host planning (segments, retiring): the device idles
behind the first event while the host plans.
The driver (no arguments) never opens the GPU: every round is a fresh child process under its own time limit through
tools/measure.py's step(), which stops the run at the first failure; inside a round the legs are timed in turns, in alternating
order, and the round reports each leg's median.  Then one run per leg under rocprofv3 --kernel-trace --stats gives the kernels'
durations.  Medians, spreads (max - min over the rounds) and the trace rows go to profiles/ms_tx_bench.json.

   python3 tools/bench_ms_tx.py [--nco] [--rounds 5] [--slots N] [--inner I] [--warmup W] [--reps R] [--timeout S] [--no-trace] [--out FILE]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

FULL_SCALE = 2047
BASE_FN = 51 * 4321
NCO_HZ = 2000.0
DEFAULT_OUT = os.path.join(ROOT, "profiles", "ms_tx_bench.json")
NCO_OUT = os.path.join(ROOT, "profiles", "ms_tx_nco_bench.json")        # --nco: shared with tools/bench_ms_tx_group.py --nco


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per call}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    trx = TrxHip(0)
    n = a.slots
    assert n % 8 == 0 and n >= 51 * 8 + 8                            # dense8 / rows8 write slots 3 .. 3 + 51 * 8 of the window / the rows
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
    tx_nco = None
    if a.nco:
        tx_nco = trxhip.MsTxScheduler(trx, tx_full_scale=FULL_SCALE, rxtx_delay=0, max_pending=n)
        tx_nco.set_nco(True, NCO_HZ)
        inc = tx_nco.nco_state()["inc"]
        c64 = torch.empty((2, n, 625), dtype=torch.complex64, device="cuda:0")
        d_rec = torch.zeros((n, 8), dtype=torch.uint8, device="cuda:0")
    scale = np.array([np.float32(float(FULL_SCALE) * 10.0 ** -j) for j in range(3)])[pwr // 10]      # driveTx()'s expression
    d_par = trx.tx_params_tensor(trxhip.tx_params_host(148, 8 + (tn % 4 == 0), 0, scale, n=n))
    d_bits_s, d_par_s = d_bits[5::8].contiguous(), d_par[5::8].contiguous()
    d_len = torch.empty(n, dtype=torch.int32, device="cuda:0")
    nd = C.c_size_t()
    now = [0]                                                       # every window lies behind the last one

    def submit(name, obj=tx):
        now[0] += (n + 16) * 625
        plan = obj.submit(reqs[name], (BASE_FN, 0, now[0]))
        assert (plan["status"][3 if name == "dense" else 0:] == trxhip.MS_TX_QUEUED).all(), np.bincount(plan["status"])

    def render(n_slots, first_slot=0, obj=tx):
        trxhip._check(L.trxhip_ms_tx_render_s16(obj.h, ptr(window, first_slot * 2500), n_slots * 625, now[0] + first_slot * 625,
                                                C.byref(nd), st), "render")

    def modulate(b, p, out, cnt):
        trxhip._check(L.trxhip_modulate_batch(trx.h, b, 148, p, None, out, 1.0, 625, ptr(d_len), cnt, 4, st), "modulate")

    def compose():
        trxhip._check(L.trxhip_modulate_batch(trx.h, ptr(d_bits), 148, ptr(d_par), ptr(c64[0]), None, 0.0, 625, ptr(d_len), n, 4, st), "modulate")
        trxhip._check(L.trxhip_ms_nco_batch_cf32(trx.h, ptr(c64[0]), 625, ptr(d_rec), ptr(c64[1]), 625, n, 625, st), "ms_nco_batch_cf32")
        trxhip._check(L.trxhip_convert_float_short(trx.h, ptr(rows), ptr(c64[1]), 1.0, n * 625 * 2, st), "convert_float_short")

    alone = lambda: None   # noqa: E731  no preparation, but timed call by call like the legs that have one
    # (prepare, timed call, calls per timed call)
    legs = {
        "dense": (lambda: submit("dense"), lambda: render(n), 1),
        "dense_rows": (alone, lambda: modulate(ptr(d_bits), ptr(d_par), ptr(rows), n), 1),
        "sparse": (lambda: submit("sparse"), lambda: render(n), 1),
        "sparse_rows": (alone, lambda: modulate(ptr(d_bits_s), ptr(d_par_s), ptr(rows), n // 8), 1),
        "fill": (alone, lambda: window.zero_(), 1),
        "dense8": (lambda: submit("dense8"), lambda: [render(8, 3 + 8 * j) for j in range(51)], 51),
        "rows8": (alone, lambda: [modulate(ptr(d_bits, (3 + 8 * j) * 148), ptr(d_par, (3 + 8 * j) * 16), ptr(rows, (3 + 8 * j) * 2500), 8)
                                  for j in range(51)], 51),
    }
    if a.nco:
        legs = {k: legs[k] for k in ("dense", "sparse", "fill", "dense8")}
        legs["dense_nco"] = (lambda: submit("dense", tx_nco), lambda: render(n, obj=tx_nco), 1)
        legs["sparse_nco"] = (lambda: submit("sparse", tx_nco), lambda: render(n, obj=tx_nco), 1)
        legs["dense8_nco"] = (lambda: submit("dense8", tx_nco), lambda: [render(8, 3 + 8 * j, tx_nco) for j in range(51)], 51)
        legs["dense_comp"] = (alone, compose, 1)
    names = br.select_legs(legs, a.legs)
    times = br.time_in_turns(torch, legs, names, a)
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
    # the rotated dense stream is the composition's rows: burst k lies at now + 625 k, its first sample has phase (now + 625 k) * inc
    if "dense_nco" in names and "dense_comp" in names:
        submit("dense", tx_nco)
        rec = np.zeros(n, dtype=trxhip.MS_NCO_ROW_DTYPE)
        rec["phase0"] = ((now[0] + 625 * k).astype(np.uint64) * np.uint64(inc & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)    # modulo 2^64, then 2^32
        rec["inc"] = inc
        d_rec.copy_(torch.from_numpy(rec.view(np.uint8).reshape(n, 8)))
        render(n, obj=tx_nco)
        compose()
        torch.cuda.synchronize()
        w = window.view(n, 625, 2)
        assert nd.value == n - 3 and torch.equal(w[3:], rows[3:]) and not w[:3].any(), "the rotated stream differs from the composition's"
        assert rows[3:].any()
    for obj in (tx, tx_nco):
        st_ = obj.state() if obj is not None else None
        assert st_ is None or (st_["pending"] == 0 and st_["missed"] == 0 and st_["overlap"] == 0 and st_["expired"] == 0), st_
    st_ = tx.state()
    assert st_["pending"] == 0 and st_["missed"] == 0 and st_["overlap"] == 0 and st_["expired"] == 0, st_
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "ms_tx", "slots": a.slots, "small_render_slots": 8, "slot_len": 625, "output": "int16", "rounds": a.rounds,
           "inner": a.inner, "reps": a.reps, "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}}
    lg = res["legs"]
    if getattr(a, "nco", False):
        res["nco_hz"] = NCO_HZ
        for x, y in (("dense_nco", "dense"), ("sparse_nco", "sparse"), ("dense8_nco", "dense8"), ("dense_nco", "dense_comp")):
            res[x + "_over_" + y] = br.pair(lg, x, y)
        return res
    res["dense_over_rows"] = round(lg["dense"]["median_ms"] / lg["dense_rows"]["median_ms"], 4)
    res["sparse_over_fill"] = round(lg["sparse"]["median_ms"] / lg["fill"]["median_ms"], 4)
    res["dense8_over_rows8"] = round(lg["dense8"]["median_ms"] / lg["rows8"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--nco", action="store_true", help="time the uplink oscillator: on against off, fused against the composition")
    br.add_options(ap, "ms_tx", warmup=2, reps=3, timeout=180, inner=5, trace="off")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots)] + (["--nco"] if a.nco else [])
    tag = "ms_tx_nco" if a.nco else "ms_tx"
    res = summarise(br.run_rounds(tag, me, a), a)
    if not a.no_trace:
        res["kernel_trace_us"] = {}
        for leg in (("dense", "dense_nco", "sparse_nco", "dense_comp") if a.nco else ("dense", "dense_rows", "sparse")):
            rows = br.kernel_trace(tag, me, ["--inner", "1", "--warmup", "1", "--reps", "3"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items())
                                           if re.match(r"ms_tx_render|tx_modulate|ms_nco_rows|convert_float_short", k)}
    if a.nco:
        br.merge_json(NCO_OUT if a.out == DEFAULT_OUT else a.out, "ms_tx", res)
    else:
        br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
