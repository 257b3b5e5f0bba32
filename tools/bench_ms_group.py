#!/usr/bin/env python3
"""The MS-side scheduler group on one GPU against single scheduler objects on the same chunks and the same stream, HIP-event
time, int16, the 51-multiframe mix over 8 TNs (per 408 slots: 5 FCCH, 5 SCH, 398 traffic), all ACTIVE, tracking on.  Member m's
stream begins at frame m % 51 of the multiframe, so the members do not meet their SCH slots in the same pull.
  g64 / s64      64 members, 8 slots (one frame) per member and pull, `frames` pulls in a row from fresh clocks: one group pull
                 per frame against 64 trxhip_ms_sched_pull_s16 per frame; reported per frame
  g256 / s256    the same with 256 members
  g1 / s1        one member, 8 slots per pull
  gbig / sbig    one member, one pull of `slots` slots (set_clock + pull per call)
With --nco the singles are left out and every group leg gets a partner with the NCO on (trxhip_ms_nco_group_set, +2000 Hz on every
member: the receiver's rotating instance) -> profiles/ms_nco_bench.json:
  n64 / n256 / n1 / nbig   g64 / g256 / g1 / gbig with the NCO on
  cbig                     the composition the fused pull replaces: trxhip_ms_nco_batch_i16 over the `slots` slots into a complex64
                           buffer, then gbig's pull as trxhip_ms_group_pull_cf32 on it (the same indications, byte for byte)
Every round is a fresh process under its own time limit; inside a round the legs are timed in turns, the order reversed every
other turn and the number of turns even, so that every leg is timed as often in front of its partner as behind it; every timed
region follows one untimed call of the same leg, so that what ran before a leg is that leg, whatever the order.  Median per leg over the rounds, spread = max - min over the rounds -> profiles/ms_group_bench.json.  The first step
that fails ends the run.

   python3 tools/bench_ms_group.py [--nco] [--rounds 5] [--slots N] [--frames F] [--inner I] [--warmup W] [--reps R] [--timeout S] [--trace LEG] [--out FILE]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_rounds as br   # noqa: E402

FULL_SCALE = 2047.0
BASE_FN = 51 * 4321
FRAME = 8 * 625
PAIRS = (("g64", "s64"), ("g256", "s256"), ("g1", "s1"), ("gbig", "sbig"))
NCO_PAIRS = (("n64", "g64"), ("n256", "g256"), ("n1", "g1"), ("nbig", "gbig"), ("nbig", "cbig"))
NCO_HZ = 2000.0


def child(a):
    """One round: the legs in turns -> one JSON line {leg: median ms per frame (per pull for gbig / sbig)}."""
    import ctypes as C
    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, trxhip
    from workloads import TSC, multiframe
    trx = TrxHip(0)
    base_iq = multiframe(trx, BASE_FN)[0]
    pairs = NCO_PAIRS if a.nco else PAIRS
    names = br.select_legs(list(dict.fromkeys(k for pair in pairs for k in pair)), a.legs)
    L, st = trx.L, trx._stream()
    vp = C.c_void_p
    frames = a.frames
    assert 1 <= frames <= 51
    iq = base_iq.repeat(3, 1, 1).contiguous()                      # 153 frames: member m reads the frames m % 51 + k, k < frames
    big = None
    if {"gbig", "sbig", "nbig", "cbig"} & set(names):
        big = base_iq.repeat((a.slots + 407) // 408, 1, 1)[:a.slots].contiguous()
    stride = 9                                                     # 8 slots and the straddling one
    ns1, nc1 = C.c_size_t(), C.c_size_t()

    def members(n):
        """(group, singles, chunk tables per frame, outputs) for n members of 8-slot pulls"""
        g = trxhip.MsRxSchedulerGroup(trx, n=n, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True)
        ss = [trxhip.MsRxScheduler(trx, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True) for _ in range(n)]
        tabs = []
        for k in range(frames):
            ch = np.zeros(n, dtype=trxhip.MS_GROUP_CHUNK_DTYPE)
            ch["d_in"] = [iq.data_ptr() + ((m % 51) + k) * FRAME * 4 for m in range(n)]
            ch["n_samples"], ch["first_ts"] = FRAME, k * FRAME
            tabs.append(ch)
        ind = torch.zeros((2, n, stride, 32), dtype=torch.uint8, device="cuda:0")
        bits = torch.zeros((2, n, stride, 148), dtype=torch.int8, device="cuda:0")
        cnt = (C.c_size_t * n)()
        return g, ss, tabs, ind, bits, cnt

    def group_leg(n):
        g, ss, tabs, ind, bits, cnt = members(n)

        def run():
            for m in range(n):
                g.set_clock(m, BASE_FN + (m % 51) - 1, 7, -625)
            for ch in tabs:
                trxhip._check(L.trxhip_ms_group_pull_s16(g.h, ch.ctypes.data_as(vp), vp(ind[0].data_ptr()), vp(bits[0].data_ptr()), stride,
                                                         C.cast(cnt, vp), None, None, st), "group pull")

        pull16 = L.trxhip_ms_sched_pull_s16
        args = [[(ss[m].h, vp(int(ch["d_in"][m])), FRAME, int(ch["first_ts"][m]), vp(ind[1, m].data_ptr()), vp(bits[1, m].data_ptr()), stride,
                  C.byref(ns1), C.byref(nc1), st) for m in range(n)] for ch in tabs]     # (made once: the loop below only calls)

        def run_singles():
            for m in range(n):
                ss[m].set_clock(BASE_FN + (m % 51) - 1, 7, -625)
            for row in args:
                for arg in row:
                    if pull16(*arg) != 0:
                        raise RuntimeError("trxhip_ms_sched_pull_s16 failed")

        def check():
            """the last frame of both paths holds the same bytes, member for member"""
            ind.zero_()
            bits.zero_()
            run()
            run_singles()
            torch.cuda.synchronize()
            assert torch.equal(ind[0], ind[1]) and torch.equal(bits[0], bits[1]), "the group's slots differ from the single objects'"
            assert all(int(g.state(m)["slots"]) == int(ss[m].state()["slots"]) for m in range(n))
            assert min(list(cnt)) >= 7, "8-slot pulls cut too few slots"

        return run, run_singles, check

    def nco_leg(n):
        """the group leg of n members and its partner with the NCO on; at 0 Hz the two return the same bytes"""
        g, _, tabs, ind, bits, cnt = members(n)
        gn = trxhip.MsRxSchedulerGroup(trx, n=n, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True)

        def leg(grp, i):
            def run():
                for m in range(n):
                    grp.set_clock(m, BASE_FN + (m % 51) - 1, 7, -625)
                for ch in tabs:
                    trxhip._check(L.trxhip_ms_group_pull_s16(grp.h, ch.ctypes.data_as(vp), vp(ind[i].data_ptr()), vp(bits[i].data_ptr()), stride,
                                                             C.cast(cnt, vp), None, None, st), "group pull")
            return run

        def set_all(hz):
            for m in range(n):
                gn.set_nco(m, False)                               # (off and on again: the phase starts at 0)
                gn.set_nco(m, True, hz)

        def check():
            set_all(0.0)
            ind.zero_()
            bits.zero_()
            leg(g, 0)()
            leg(gn, 1)()
            torch.cuda.synchronize()
            assert torch.equal(ind[0], ind[1]) and torch.equal(bits[0], bits[1]), "the NCO at 0 Hz changed what a pull returns"
            set_all(NCO_HZ)

        set_all(NCO_HZ)
        return leg(g, 0), leg(gn, 1), check

    legs, checks = {}, []
    for n, (gn, sn) in ((64, pairs[0]), (256, pairs[1]), (1, pairs[2])):
        if gn in names or sn in names:
            if a.nco:
                run, run_nco, check = nco_leg(n)
                legs[sn], legs[gn] = (run, frames), (run_nco, frames)
            else:
                run, run_singles, check = group_leg(n)
                legs[gn], legs[sn] = (run, frames), (run_singles, frames)
            checks.append(check)
    if big is not None and a.nco:
        gb, nb, cb = (trxhip.MsRxSchedulerGroup(trx, n=1, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True) for _ in range(3))
        nb.set_clock(0, BASE_FN - 1, 7, -625)
        nb.set_nco(0, True, NCO_HZ)
        ind_b = torch.empty((3, a.slots, 32), dtype=torch.uint8, device="cuda:0")
        bits_b = torch.empty((3, a.slots, 148), dtype=torch.int8, device="cuda:0")
        rot = torch.empty((a.slots * 625,), dtype=torch.complex64, device="cuda:0")
        o = nb.nco_state(0)
        rec = np.zeros(1, dtype=trxhip.MS_NCO_ROW_DTYPE)
        rec["phase0"], rec["inc"] = trxhip.ms_nco_phase(o["acc"], o["ts_ref"], o["inc"], 0), o["inc"]
        d_rec = torch.from_numpy(rec.view(np.uint8)).to("cuda:0")
        cntb = (C.c_size_t * 1)()

        def chunk(ptr):
            ch = np.zeros(1, dtype=trxhip.MS_GROUP_CHUNK_DTYPE)
            ch["d_in"], ch["n_samples"], ch["first_ts"] = ptr, a.slots * 625, 0
            return ch

        ch_i16, ch_rot = chunk(big.data_ptr()), chunk(rot.data_ptr())

        def pull(grp, i, ch, fn):
            grp.set_clock(0, BASE_FN - 1, 7, -625)
            trxhip._check(fn(grp.h, ch.ctypes.data_as(vp), vp(ind_b[i].data_ptr()), vp(bits_b[i].data_ptr()), a.slots, C.cast(cntb, vp), None,
                             None, st), "group pull")

        def cbig():
            trxhip._check(L.trxhip_ms_nco_batch_i16(trx.h, vp(big.data_ptr()), a.slots * 625, vp(d_rec.data_ptr()), vp(rot.data_ptr()),
                                                    a.slots * 625, 1, a.slots * 625, st), "nco batch")
            pull(cb, 2, ch_rot, L.trxhip_ms_group_pull_cf32)

        def check_nco_big():
            pull(nb, 1, ch_i16, L.trxhip_ms_group_pull_s16)
            cbig()
            torch.cuda.synchronize()
            assert cntb[0] == a.slots and nb.nco_state(0) == o
            assert torch.equal(ind_b[1], ind_b[2]) and torch.equal(bits_b[1], bits_b[2]), "the fused pull differs from the composition"

        legs["gbig"] = (lambda: pull(gb, 0, ch_i16, L.trxhip_ms_group_pull_s16), 1)
        legs["nbig"] = (lambda: pull(nb, 1, ch_i16, L.trxhip_ms_group_pull_s16), 1)
        legs["cbig"] = (cbig, 1)
        checks.append(check_nco_big)
    elif big is not None:
        gb = trxhip.MsRxSchedulerGroup(trx, n=1, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True)
        sb = trxhip.MsRxScheduler(trx, rx_full_scale=FULL_SCALE, tsc=TSC, active_tns=0xFF, tracking=True)
        ind_b = torch.empty((2, a.slots, 32), dtype=torch.uint8, device="cuda:0")
        bits_b = torch.empty((2, a.slots, 148), dtype=torch.int8, device="cuda:0")
        chb = np.zeros(1, dtype=trxhip.MS_GROUP_CHUNK_DTYPE)
        chb["d_in"], chb["n_samples"], chb["first_ts"] = big.data_ptr(), a.slots * 625, 0
        cntb = (C.c_size_t * 1)()

        def gbig():
            gb.set_clock(0, BASE_FN - 1, 7, -625)
            trxhip._check(L.trxhip_ms_group_pull_s16(gb.h, chb.ctypes.data_as(vp), vp(ind_b[0].data_ptr()), vp(bits_b[0].data_ptr()), a.slots,
                                                     C.cast(cntb, vp), None, None, st), "group pull")

        def sbig():
            sb.set_clock(BASE_FN - 1, 7, -625)
            trxhip._check(L.trxhip_ms_sched_pull_s16(sb.h, vp(big.data_ptr()), a.slots * 625, 0, vp(ind_b[1].data_ptr()), vp(bits_b[1].data_ptr()),
                                                     a.slots, C.byref(ns1), C.byref(nc1), st), "pull")

        def check_big():
            gbig()
            sbig()
            torch.cuda.synchronize()
            assert cntb[0] == ns1.value == a.slots
            assert torch.equal(ind_b[0], ind_b[1]) and torch.equal(bits_b[0], bits_b[1]), "the group's slots differ from the single object's"

        legs["gbig"], legs["sbig"] = (gbig, 1), (sbig, 1)
        checks.append(check_big)
    names = [k for k in names if k in legs]
    times = br.time_in_turns(torch, legs, names, a, untimed_first=True)
    if not a.legs:
        for check in checks:
            check()
    print(json.dumps(times), flush=True)


def summarise(per_leg, a):
    nco = getattr(a, "nco", False)
    res = {"workload": "ms_nco" if nco else "ms_group", "slots": a.slots, "small_pull_slots": 8, "frames_per_call": a.frames, "slot_len": 625,
           "mix_per_408": {"fcch": 5, "sch": 5, "traffic": 398}, "input": "int16", "tracking": True, "rounds": a.rounds, "inner": a.inner,
           "reps": a.reps, "unit": "ms per frame of all members (gbig / sbig: per pull)",
           "legs": {name: br.leg_summary(xs) for name, xs in per_leg.items()}, "pairs": {}}
    if nco:
        res["nco_hz"] = NCO_HZ
    for x, y in (NCO_PAIRS if nco else PAIRS):
        if x in res["legs"] and y in res["legs"]:
            res["pairs"][x + "_over_" + y] = br.pair(res["legs"], x, y)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--frames", type=int, default=17, help="8-slot pulls in a row per timed call")
    ap.add_argument("--nco", action="store_true", help="the NCO legs instead of the single objects -> profiles/ms_nco_bench.json")
    br.add_options(ap, "ms_group", warmup=2, reps=3, timeout=150, inner=6, even_inner=True, trace="legs")
    a = ap.parse_args()
    if a.round is not None:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--slots", str(a.slots), "--frames", str(a.frames)] + (["--nco"] if a.nco else [])
    if a.nco and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "ms_nco_bench.json")
    res = summarise(br.run_rounds("ms_nco" if a.nco else "ms_group", me, a), a)
    if a.trace:
        res["kernel_trace_us"] = {}
        for leg in a.trace.split(","):
            rows = br.kernel_trace("ms_group", me, ["--inner", "1", "--warmup", "1", "--reps", "1"], leg, a)
            res["kernel_trace_us"][leg] = {k: v for k, v in sorted(rows.items()) if re.match(r"ms_rx|ms_join|ms_nco", k)}
    br.write_json(a.out, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
