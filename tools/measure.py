#!/usr/bin/env python3
"""GPU measurement steps, one fresh child process at a time, each under `timeout -k 10 <seconds>`.  The first step that
exits non-zero (time limit, abort, fault or any other status) ends the run: its log's tail is printed, nothing more is
started, and this exits with that status.  No step is ever retried.  This driver never opens the GPU itself.

Same-box A/B (the boxes of a pool differ by a few percent between sessions, so builds are compared inside one):
   python tools/measure.py ab --rounds 3 --arm old:TRXHIP_LIB=osmo_trx_amd/lib/libtrxhip_old.so --arm new \\
       [--field value --field roofline.kernel_ms] [-- python3 bench.py --main-only --steps 40]
   python tools/measure.py ab --arm split --arm general:TRXHIP_NO_NB_KERNEL=1 --field config.other_configs.configs[2].mbursts_per_s_all_gpus -- python3 bench.py --legs c2
   python tools/measure.py ab --arm a --arm b:TRXHIP_LIB=... --field mbursts_per_s -- python3 tools/workloads.py rach
Counter passes (rocprofv3 --pmc, one run per counter set, no tracing), per-unit means per kernel:
   python tools/measure.py pmc --set insts --set active [--kernels pull4] [--per 1048576] [--tag q] [--arm ...] \\
       [-- python3 bench.py --steps 2 --warmup 1 --main-only]      -> <out>/<tag>_pmc.json
   python tools/measure.py pmc --set mem --set active --set cache --kernels 'channelize|resample|frontend' --per 262144 \\
       -- python3 tools/workloads.py frontend --warmup 2 --reps 2"""
import argparse
import collections
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Counter sets: each is passed to rocprofv3 in a single run as some earlier recipe of this project did.
SETS = {
    "insts": "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES",
    "mix": "SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_BRANCH",
    "mem": "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR",
    "busy": "SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_BUSY_CYCLES GRBM_GUI_ACTIVE",
    "active": "SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_LDS_IDX_ACTIVE SQ_WAIT_ANY "
              "SQ_WAIT_INST_ANY SQ_LDS_BANK_CONFLICT",
    "wait": "SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY "
            "SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT",
    "level": "SQ_INSTS_VALU SQ_IFETCH SQ_INST_LEVEL_LDS SQ_BUSY_CYCLES SQ_WAVES SQ_INSTS_MISC",
    "cache": "GRBM_GUI_ACTIVE TCC_HIT_sum TCC_MISS_sum TCC_EA0_WRREQ_sum TCC_EA0_RDREQ_sum TCP_PENDING_STALL_CYCLES_sum",
    "icache": "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQ_IFETCH SQ_WAVE_CYCLES SQ_INSTS_VALU",
    "icache_wait": "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQ_IFETCH SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_WAIT_INST_ANY",
}


def step(name, cmd, log, seconds, env=None):
    """Run `cmd` under `timeout -k 10 seconds` from the repository root, stdout and stderr into `log`; exit on failure."""
    with open(log, "w") as f:
        rc = subprocess.call(["timeout", "-k", "10", str(seconds)] + cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT,
                             env={**os.environ, **(env or {})})
    if rc != 0:
        rc = 128 - rc if rc < 0 else rc                     # killed by a signal: report it the way a shell does
        print(f"measure.py: step {name} failed with exit status {rc} (log: {log}): {' '.join(cmd)}", file=sys.stderr)
        with open(log, errors="replace") as f:
            sys.stderr.write("".join(f.readlines()[-20:]))
        sys.exit(rc)


def parse_arm(spec):
    """NAME[:VAR=VAL,...] -> (name, env); a TRXHIP_LIB path is made absolute."""
    name, _, rest = spec.partition(":")
    env = dict(kv.split("=", 1) for kv in rest.split(",") if kv)
    if "TRXHIP_LIB" in env:
        env["TRXHIP_LIB"] = os.path.abspath(env["TRXHIP_LIB"])
    return name, env


def last_json(log):
    for line in reversed(open(log, errors="replace").read().splitlines()):
        if line.startswith("{"):
            try:
                return json.loads(line)
            except ValueError:
                pass
    raise SystemExit(f"measure.py: no JSON line in {log}")


def pick(rec, path):
    """Value at a dotted key path; a dot-free key such as `configs[2]` is one step, an integer indexes a list."""
    for k in path.split("."):
        rec = rec[int(k)] if isinstance(rec, list) else rec[k]
    return rec


def ab(a, arms, cmd):
    vals = collections.defaultdict(list)
    for r in range(a.rounds):
        for name, env in (arms if r % 2 == 0 else arms[::-1]):
            log = os.path.join(a.out, f"{a.tag}_ab_{name}_{r + 1}.log")
            step(f"{name} (round {r + 1})", cmd, log, a.timeout, env)
            v = [pick(last_json(log), f) for f in a.field]
            vals[name].append(v)
            print(f"round {r + 1} {name:12s} " + " ".join(str(x) for x in v), flush=True)
    for i, f in enumerate(a.field):
        base = statistics.mean(vals[arms[0][0]][k][i] for k in range(a.rounds))
        for name, _ in arms:
            xs = [v[i] for v in vals[name]]
            sd = statistics.stdev(xs) if len(xs) > 1 else 0.0
            print(f"{f} {name:12s} {statistics.mean(xs):.4f} ± {sd:.4f} (n={len(xs)})  ratio {statistics.mean(xs) / base:.4f}")


def aggregate(paths, per):
    """{kernel: {counter: mean over launches / per}} of rocprofv3 *_counter_collection.csv files."""
    acc = collections.defaultdict(list)
    for p in paths:
        with open(p) as f:
            for r in csv.DictReader(f):
                acc[(r["Kernel_Name"].split("(")[0], r["Counter_Name"])].append(float(r["Counter_Value"]))
    out = collections.defaultdict(dict)
    for (k, c), v in sorted(acc.items()):
        out[k][c] = sum(v) / len(v) / per
    return dict(out)


def derived(counters, per):
    """Busy shares and waves per SIMD of one kernel from GRBM_GUI_ACTIVE (8 dies) and the SQ cycle counters, when present."""
    g = lambda c: counters.get(c, 0.0) * per
    if not g("GRBM_GUI_ACTIVE"):
        return None
    kcyc = g("GRBM_GUI_ACTIVE") / 8
    return (f"valu_busy {4 * g('SQ_ACTIVE_INST_VALU') / (kcyc * 1024):.3f} lds_busy {g('SQ_LDS_IDX_ACTIVE') / (kcyc * 256):.3f} "
            f"waves/SIMD {4 * g('SQ_WAVE_CYCLES') / (kcyc * 1024):.2f} wait_share {g('SQ_WAIT_ANY') / max(g('SQ_WAVE_CYCLES'), 1e-9):.3f}")


def pmc(a, arms, cmd):
    result = {}
    for name, env in arms:
        paths = []
        for s in a.set:
            d = os.path.join(a.out, f"{a.tag}_pmc_{name}_{s}")
            shutil.rmtree(d, ignore_errors=True)
            prof = ["rocprofv3", "--output-format", "csv", "--kernel-include-regex", a.kernels, "--pmc", *SETS[s].split(),
                    "-d", d, "-o", a.tag, "--"] + cmd
            step(f"{name} {s}", prof, d + ".log", a.timeout, env)
            found = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not found:
                raise SystemExit(f"measure.py: no counter_collection.csv under {d} (log: {d}.log)")
            paths += found
        result[name] = aggregate(paths, a.per)
        for s in a.set:                                         # keep the logs, drop rocprofv3's output directories
            shutil.rmtree(os.path.join(a.out, f"{a.tag}_pmc_{name}_{s}"))
        for k, cs in result[name].items():
            for c, v in cs.items():
                print(f"{name:10s} {k:48s} {c:30s} {v:12.3f}")
            line = derived(cs, a.per)
            if line:
                print(f"{name:10s} {k}: {line}")
    out = os.path.join(a.out, f"{a.tag}_pmc.json")
    json.dump({"tag": a.tag, "sets": a.set, "kernels": a.kernels, "per": a.per, "command": cmd, "arms": result}, open(out, "w"), indent=1)
    print("wrote", out)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    cmd = argv[argv.index("--") + 1:] if "--" in argv else None
    argv = argv[:argv.index("--")] if "--" in argv else argv
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter,
                                 epilog=__doc__.split("\n\n", 1)[1])
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--arm", action="append", default=[], help="NAME[:VAR=VAL,...] (no variables: the default build)")
    common.add_argument("--timeout", type=int, default=300, help="seconds per step")
    common.add_argument("--tag", default="m", help="prefix of the logs and outputs")
    common.add_argument("--out", default=os.path.join(ROOT, "build", "measure"), help="directory of the logs and outputs")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("ab", parents=[common], help="alternate arms over one command, summarise JSON fields")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--field", action="append", help="dotted key path into the last JSON line of stdout (default: value)")
    p = sub.add_parser("pmc", parents=[common], help="rocprofv3 --pmc passes, per-unit means per kernel and counter")
    p.add_argument("--set", action="append", choices=sorted(SETS), required=True)
    p.add_argument("--kernels", default="pull4", help="--kernel-include-regex")
    p.add_argument("--per", type=float, default=1 << 20, help="units per launch (default: 1 Mi bursts)")
    a = ap.parse_args(argv)
    a.out = os.path.abspath(a.out)
    os.makedirs(a.out, exist_ok=True)
    arms = [parse_arm(s) for s in a.arm] or [("default", {})]
    if a.cmd == "ab":
        a.field = a.field or ["value"]
        ab(a, arms, cmd or ["python3", "bench.py", "--main-only", "--steps", "40"])
    else:
        pmc(a, arms, cmd or ["python3", "bench.py", "--steps", "2", "--warmup", "1", "--main-only"])


if __name__ == "__main__":
    main()
