#!/usr/bin/env python3
"""The MS-side uplink scheduler group on one GPU against single uplink scheduler objects on the same requests, the same windows
and the same stream, HIP-event time, int16, a burst on every TN unless said.
  g64 / s64        64 members, one frame (8 slots) per member and render, `frames` frames in a row, each with the submit of that
                   frame's requests: one group submit and one group render per frame against 64 trxhip_ms_tx_submit and 64
                   trxhip_ms_tx_render_s16; reported per frame
  g256 / s256      the same with 256 members
  g1 / s1          one member, 8 slots per render, with its submit
  gdense / sdense    one member, one render of `slots` slots with a burst on every TN (the submit before it is not timed)
  gsparse / ssparse  the same window with a burst on one TN in 8
--nco times the uplink oscillator instead (results under "ms_tx_group" in profiles/ms_tx_nco_bench.json): g64 / g256 / gdense /
gsparse as above on groups with every oscillator off, and g64_nco / g256_nco / gdense_nco / gsparse_nco the same requests on
groups whose members all have it on (2000 Hz + the member's index: the rotating instance of the kernel).
Every round is a fresh process under its own time limit; inside a round the legs are timed in turns, the order reversed every
other turn and the number of turns even; every timed region follows one untimed call of the same leg.  Every round ends with a
byte comparison of the group's outputs with the single objects'.  Median per leg over the rounds, spread = max - min over the
rounds -> profiles/ms_tx_group_bench.json.  --trace takes the kernel times of the named legs from rocprofv3 --kernel-trace runs
of their own.  The first step that fails ends the run.

   python3 tools/bench_ms_tx_group.py [--nco] [--rounds 5] [--slots N] [--frames F] [--inner I] [--warmup W] [--reps R] [--timeout S] [--trace LEGS] [--out FILE]"""
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
FRAME = 8 * 625
PAIRS = (("g64", "s64"), ("g256", "s256"), ("g1", "s1"), ("gdense", "sdense"), ("gsparse", "ssparse"))
NCO_PAIRS = (("g64_nco", "g64"), ("g256_nco", "g256"), ("gdense_nco", "gdense"), ("gsparse_nco", "gsparse"))
NCO_HZ = 2000.0
DEFAULT_OUT = os.path.join(ROOT, "profiles", "ms_tx_group_bench.json")
NCO_OUT = os.path.join(ROOT, "profiles", "ms_tx_nco_bench.json")        # --nco: shared with tools/bench_ms_tx.py --nco


def slot_requests(trxhip, np, slots, bits):
    """request k is heard in slot slots[k] of a stream that starts at the clock (BASE_FN, 0): its target after incTN(3)"""
    return trxhip.ms_tx_requests(BASE_FN + (slots - 3) // 8, (slots - 3) % 8, (slots * 3) % 30, bits)


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per frame (per render for the big legs)}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    trx = TrxHip(0)
    pairs = NCO_PAIRS if a.nco else PAIRS
    names = br.select_legs([k for pair in pairs for k in pair], a.legs)
    L, st = trx.L, trx._stream()
    vp = C.c_void_p
    frames = a.frames
    rng = np.random.default_rng(3)
    now = [0]                                                       # every run's windows lie behind the last run's

    def frame_legs(n, nco=False):
        """n members: per run `frames` frames, each the submit of its 8 requests per member and the render of its 5000 samples;
        nco: every member's oscillator on, and the single objects' too"""
        g = trxhip.MsTxSchedulerGroup(trx, n_members=n, tx_full_scale=FULL_SCALE, rxtx_delay=0, max_pending=16)
        ss = [trxhip.MsTxScheduler(trx, tx_full_scale=FULL_SCALE, rxtx_delay=0, max_pending=16) for _ in range(n)]
        if nco:
            for m in range(n):
                g.set_nco(m, True, NCO_HZ + m)
                ss[m].set_nco(True, NCO_HZ + m)
        out = torch.zeros((2, n, FRAME, 2), dtype=torch.int16, device="cuda:0")
        # frame f of a run holds slots 8 (f + 1) .. 8 (f + 1) + 7 behind the run's clock (the first three lie behind the clock)
        reqs = [[slot_requests(trxhip, np, 8 * (f + 1) + np.arange(8), rng.integers(0, 2, (8, 148))) for _ in range(n)] for f in range(frames)]
        greqs = [np.concatenate(r) for r in reqs]
        member = np.repeat(np.arange(n, dtype=np.uint32), 8)
        clocks = np.zeros(n, dtype=trxhip.MS_TX_CLOCK_DTYPE)
        clocks["fn"] = BASE_FN
        first = [np.zeros(n, dtype=np.int64) for _ in range(frames)]
        sizes = np.full(n, FRAME, dtype=np.uintp)
        now_c = C.c_int64()
        first_c = [C.c_int64() for _ in range(frames)]
        nd1, bad, badm = C.c_size_t(), C.c_size_t(), C.c_int()
        g_sub = [(g.h, member.ctypes.data_as(vp), r.ctypes.data_as(vp), len(r), clocks.ctypes.data_as(vp), None, C.byref(bad), st) for r in greqs]
        g_ren = [(g.h, vp(out[0].data_ptr()), FRAME, t.ctypes.data_as(vp), sizes.ctypes.data_as(vp), None, C.byref(badm), st) for t in first]
        s_sub = [[(ss[m].h, reqs[f][m].ctypes.data_as(vp), 8, BASE_FN, 0, now_c, None, st) for m in range(n)] for f in range(frames)]
        s_ren = [[(ss[m].h, vp(out[1, m].data_ptr()), FRAME, first_c[f], C.byref(nd1), st) for m in range(n)] for f in range(frames)]
        gsubmit, grender = L.trxhip_ms_tx_group_submit, L.trxhip_ms_tx_group_render_s16
        ssubmit, srender = L.trxhip_ms_tx_submit, L.trxhip_ms_tx_render_s16

        def advance():
            now[0] += (frames + 4) * FRAME
            return now[0]

        def run():
            t = advance()
            clocks["ts"] = t
            for f in range(frames):
                first[f][:] = t + (f + 1) * FRAME
            for sub, ren in zip(g_sub, g_ren):
                if gsubmit(*sub) != 0 or grender(*ren) != 0:
                    raise RuntimeError("group call failed")

        def run_singles():
            t = advance()
            now_c.value = t
            for f in range(frames):
                first_c[f].value = t + (f + 1) * FRAME
            for subs, rens in zip(s_sub, s_ren):
                for sub in subs:
                    if ssubmit(*sub) != 0:
                        raise RuntimeError("trxhip_ms_tx_submit failed")
                for ren in rens:
                    if srender(*ren) != 0:
                        raise RuntimeError("trxhip_ms_tx_render_s16 failed")

        def check():
            """the last frame of both paths holds the same bytes, member for member, and every burst was drawn"""
            out.zero_()
            run()
            if nco:
                now[0] -= (frames + 4) * FRAME                      # a rotated sample depends on its timestamp: the same windows
            run_singles()
            torch.cuda.synchronize()
            assert torch.equal(out[0], out[1]) and bool(out[0].any(dim=2).any(dim=1).all()), "the group's streams differ from the single objects'"
            for m in (0, n - 1):
                a_, b_ = g.state(m), ss[m].state()
                assert a_["drawn"] == a_["queued"] and b_["drawn"] == b_["queued"] and a_["pending"] == 0 and a_["missed"] == 0, (a_, b_)
                assert a.nco or a_["drawn"] == b_["drawn"]          # (--nco times the groups only: the single objects ran less often)

        return run, run_singles, check

    legs, checks = {}, []
    for n, (gn, sn) in ((64, PAIRS[0]), (256, PAIRS[1]), (1, PAIRS[2])):
        if a.nco and n > 1 and (gn in names or gn + "_nco" in names):
            run, _, check = frame_legs(n)
            run_nco, _, check_nco = frame_legs(n, nco=True)           # its check: the rotating group against rotating single objects
            legs[gn], legs[gn + "_nco"] = (None, run, frames), (None, run_nco, frames)
            checks += [check, check_nco]                              # (the checks also keep the objects alive: the calls hold handles)
        elif not a.nco and (gn in names or sn in names):
            run, run_singles, check = frame_legs(n)
            legs[gn], legs[sn] = (None, run, frames), (None, run_singles, frames)
            checks.append(check)
    if any(k in names for k in ("gdense", "sdense", "gsparse", "ssparse", "gdense_nco", "gsparse_nco")):
        n = a.slots
        assert n % 8 == 0 and n >= 64
        k = np.arange(n)
        dense = slot_requests(trxhip, np, k, rng.integers(0, 2, (n, 148)))
        big = {"dense": dense, "sparse": dense[5::8].copy()}
        gb = trxhip.MsTxSchedulerGroup(trx, n_members=1, tx_full_scale=FULL_SCALE, rxtx_delay=0, max_pending=n)
        sb = trxhip.MsTxScheduler(trx, tx_full_scale=FULL_SCALE, rxtx_delay=0, max_pending=n)
        if a.nco:                                                   # the pair is the group with its oscillator off and the single
            sb.set_nco(True, NCO_HZ)                                # object's place is taken by a second group with it on
            gn_ = trxhip.MsTxSchedulerGroup(trx, n_members=1, tx_full_scale=FULL_SCALE, rxtx_delay=0, max_pending=n)
            gn_.set_nco(0, True, NCO_HZ)
        window = torch.empty((2, n * 625, 2), dtype=torch.int16, device="cuda:0")
        ndb = C.c_size_t()

        def submit_big(obj, name):
            now[0] += (n + 16) * 625
            clock = (BASE_FN, 0, now[0])
            plan = obj.submit(big[name], clock) if obj is sb else obj.submit(0, big[name], [clock])
            assert (plan["status"][3 if name == "dense" else 0:] == trxhip.MS_TX_QUEUED).all(), np.bincount(plan["status"])
            return now[0]

        at = {}

        def gbig():
            _, nd = gb.render([n * 625], [at["g"]], out=window[0:1])
            return nd[0]

        def sbig():
            trxhip._check(L.trxhip_ms_tx_render_s16(sb.h, vp(window[1].data_ptr()), n * 625, at["s"], C.byref(ndb), st), "render")
            return ndb.value

        def gbig_nco():
            _, nd = gn_.render([n * 625], [at["n"]], out=window[0:1])
            return nd[0]

        for name in ("dense", "sparse"):
            legs["g" + name] = (lambda name=name: at.__setitem__("g", submit_big(gb, name)), gbig, 1)
            if a.nco:
                legs["g" + name + "_nco"] = (lambda name=name: at.__setitem__("n", submit_big(gn_, name)), gbig_nco, 1)
            else:
                legs["s" + name] = (lambda name=name: at.__setitem__("s", submit_big(sb, name)), sbig, 1)

        def check_big():
            for name, want in (("dense", n - 3), ("sparse", n // 8)):
                if a.nco:                                           # the rotating group against the rotating single object
                    at["n"] = submit_big(gn_, name)
                    now[0] -= (n + 16) * 625                        # the same window for both: a rotated sample depends on its timestamp
                    at["s"] = submit_big(sb, name)
                    assert gbig_nco() == sbig() == want
                else:
                    legs["g" + name][0]()
                    legs["s" + name][0]()
                    assert gbig() == sbig() == want
                torch.cuda.synchronize()
                assert torch.equal(window[0], window[1]) and bool(window[0].any()), "the group's stream differs from the single object's"

        checks.append(check_big)
    names = [k for k in names if k in legs]
    # (prepare, call, calls per call); without a prepare step the submits are part of the timed region
    times = br.time_in_turns(torch, legs, names, a, untimed_first=True)
    if not a.legs:
        for check in checks:
            check()
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    res = {"workload": "ms_tx_group", "slots": a.slots, "small_render_slots": 8, "frames_per_call": a.frames, "slot_len": 625,
           "output": "int16", "rounds": a.rounds, "inner": a.inner, "reps": a.reps,
           "unit": "ms per frame of all members, submits included (gdense / sdense / gsparse / ssparse: per render)",
           "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}, "pairs": {}}
    for x, y in (NCO_PAIRS if getattr(a, "nco", False) else PAIRS):
        if x in res["legs"] and y in res["legs"]:
            res["pairs"][x + "_over_" + y] = br.pair(res["legs"], x, y)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--frames", type=int, default=17, help="frames in a row per timed call")
    ap.add_argument("--nco", action="store_true", help="time the uplink oscillator: every member's on against every member's off")
    br.add_options(ap, "ms_tx_group", warmup=2, reps=3, timeout=150, inner=6, even_inner=True, trace="legs")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots), "--frames", str(a.frames)] + (["--nco"] if a.nco else [])
    tag = "ms_tx_group_nco" if a.nco else "ms_tx_group"
    res = summarise(br.run_rounds(tag, me, a), a)
    if a.trace:
        res["kernel_trace_us"] = {}
        for leg in a.trace.split(","):
            rows = br.kernel_trace(tag, me, ["--inner", "2", "--warmup", "1", "--reps", "1"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if re.match(r"ms_tx_", k)}
    if a.nco:
        res["nco_hz"] = "2000 + the member's index"
        br.merge_json(NCO_OUT if a.out == DEFAULT_OUT else a.out, "ms_tx_group", res)
    else:
        br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
