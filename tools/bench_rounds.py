"""What the scheduler benches (tools/bench_rx_*.py, bench_sch_sync.py, bench_ms_*.py) share.  Imported, never run; it opens no
GPU and imports no torch: the timing loops take the child's own torch as an argument.

Driver side (the parent process): add_options() for the common command line, run_rounds() for one fresh child per round through
tools/measure.py's step() (each under its own `timeout -k 10`; the first failing step ends the run with its exit status),
leg_summary() / pair() for the per-leg and per-pair figures, kernel_trace() for one rocprofv3 --kernel-trace --stats run
(kernel traces only, never counters), resource_usage() for the compiler's report, write_json().
Child side (the per-round process): select_legs(), time_in_order(), time_in_turns()."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

import measure

ROOT = measure.ROOT


def add_options(ap, name, warmup, reps, timeout, inner=None, even_inner=False, trace=None):
    """The options every bench has, with this tool's defaults.  inner: turns per leg inside a round (None: the tool times in
    order and has no --inner); even_inner: run_rounds() refuses an odd --inner (the tools whose legs are compared in pairs, so that
    each is timed as often in front of its partner as behind it); trace: "off" adds --no-trace, "legs" adds --trace LEGS."""
    ap.add_argument("--rounds", type=int, default=5)
    if inner is not None:
        ap.add_argument("--inner", type=int, default=inner, help="turns per leg inside a round" +
                        (" (even: both orders equally often)" if even_inner else ""))
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--timeout", type=int, default=timeout, help="seconds per round")
    if trace == "off":
        ap.add_argument("--no-trace", action="store_true")
    elif trace == "legs":
        ap.add_argument("--trace", default="", help="also take a kernel trace of these legs (comma-separated), each in a run of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", name + "_bench.json"))
    ap.add_argument("--logs", default=os.path.join(ROOT, "build", "measure"))
    ap.add_argument("--round", type=int, default=None, help=argparse.SUPPRESS)     # child: run one round on the GPU
    ap.add_argument("--legs", default="", help=argparse.SUPPRESS)
    ap.set_defaults(even_inner=even_inner)


def run_rounds(tag, child_cmd, a):
    """a.rounds fresh children of `child_cmd --round k [--inner I] --warmup W --reps R`, one after the other, logs in
    <logs>/<tag>_round_<k>.log -> {key of the child's last JSON line: [value per round]}"""
    for bad, why in ((a.rounds < 5, "at least five rounds"), (getattr(a, "even_inner", False) and a.inner % 2, "an even number of turns")):
        if bad:
            print("error: " + why, file=sys.stderr)
            sys.exit(2)
    os.makedirs(a.logs, exist_ok=True)
    sizes = (["--inner", str(a.inner)] if hasattr(a, "inner") else []) + ["--warmup", str(a.warmup), "--reps", str(a.reps)]
    per_leg = {}
    for r in range(a.rounds):
        log = os.path.join(a.logs, "%s_round_%d.log" % (tag, r + 1))
        measure.step("round %d" % (r + 1), child_cmd + ["--round", str(r)] + sizes, log, a.timeout)
        for k, v in measure.last_json(log).items():
            per_leg.setdefault(k, []).append(v)
        print("round %d done" % (r + 1), flush=True)
    return per_leg


def leg_summary(xs, **extra):
    """One leg's per-round values -> its entry under "legs"."""
    return dict(median_ms=round(statistics.median(xs), 4), spread_ms=round(max(xs) - min(xs), 4), ms=[round(x, 4) for x in xs], **extra)


def pair(legs, a, b):
    """Leg a against leg b of a result's "legs"."""
    return dict(ratio=round(legs[a]["median_ms"] / legs[b]["median_ms"], 4), diff_ms=round(legs[a]["median_ms"] - legs[b]["median_ms"], 4),
                larger_spread_ms=max(legs[a]["spread_ms"], legs[b]["spread_ms"]))


def trace_rows(d):
    """{kernel: {calls, avg_us}} of a rocprofv3 --kernel-trace --stats directory"""
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
                rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    return rows


def kernel_trace(tag, child_cmd, child_args, leg, a):
    """One run of `child_cmd --round 0 <child_args> --legs <leg>` under rocprofv3 --kernel-trace --stats -> trace_rows()"""
    d = os.path.join(a.logs, tag + "_trace")
    shutil.rmtree(d, ignore_errors=True)
    measure.step("kernel trace " + leg, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", tag, "--"] +
                 child_cmd + ["--round", "0"] + child_args + ["--legs", leg], os.path.join(a.logs, "%s_trace_%s.log" % (tag, leg)), a.timeout)
    rows = trace_rows(d)
    shutil.rmtree(d, ignore_errors=True)
    return rows


def resource_usage(source_file, pattern):
    """{kernel: {VGPRs, SGPRs spill, VGPRs spill, scratch bytes/lane, LDS bytes/block, occupancy}} from tools/resource_usage.sh"""
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "resource_usage.sh"), source_file, pattern], stdout=subprocess.PIPE,
                         text=True, check=True).stdout
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "lds_bytes_per_block", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for line in txt.splitlines():
        m = re.match(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip() or m.group(1)
            cur = out.setdefault(name.split("(")[0].replace("void ", ""), {})
            continue
        m = re.match(r"\s+([^:]+): (\d+)$", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def write_json(path, res):
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def merge_json(path, key, res):
    """res under `key` of the JSON object in `path`, its other keys kept: the file two tools report into"""
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[key] = res
    write_json(path, doc)


def select_legs(all_names, legs):
    """all_names, or those of them that --legs names"""
    return [k for k in all_names if not legs or k in legs.split(",")]


def _region(torch, call, n):
    """ms of n calls between two event records, synchronised behind them"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def time_in_order(torch, legs, names, a, reps=None):
    """Every leg once, the order reversed on odd rounds: its prepare step (if any), a.warmup calls, then one timed region of
    `reps` (a.reps) calls.  legs[name] = (prepare or None, call) -> {name: ms per call}, in the order timed."""
    reps = a.reps if reps is None else reps
    out = {}
    for name in (names[::-1] if a.round % 2 else names):
        prep, f = legs[name]
        if prep:
            prep()
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        out[name] = _region(torch, f, reps) / reps
    return out


def time_in_turns(torch, legs, names, a, untimed_first=False):
    """All legs warmed, then a.inner turns whose order flips with (a.round + turn) % 2 -> {name: median over the turns of ms per
    call / `per`}.  untimed_first: every timed region follows one untimed call of the same leg.  Two forms of legs:
      legs[name] = (call, per)           a.warmup bare calls per leg, one synchronize; a turn is one region of a.reps calls
      legs[name] = (prepare, call, per)  with a prepare step every call is a region of its own behind its (untimed) prepare, with
                                         None all calls are one region; the warm-up and the untimed call have that form too"""
    prepared = bool(names) and len(legs[names[0]]) == 3
    if prepared:
        def run(name, n):
            prep, call, per = legs[name]
            if prep is None:
                return _region(torch, call, n) / max(n, 1) / per
            total = 0.0
            for _ in range(n):
                prep()
                total += _region(torch, call, 1)
            return total / max(n, 1) / per

        for name in names:
            run(name, a.warmup)
    else:
        def run(name, n):
            f, per = legs[name]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            if untimed_first:
                f()
            ev[0].record()
            for _ in range(n):
                f()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / n / per

        for name in names:
            f = legs[name][0]
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
    times = {k: [] for k in names}
    for i in range(a.inner):
        for name in (names if (a.round + i) % 2 == 0 else names[::-1]):
            if prepared and untimed_first:
                run(name, 1)
            times[name].append(run(name, a.reps))
    return {k: statistics.median(v) for k, v in times.items()}
