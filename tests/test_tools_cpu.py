"""The measurement tools without a GPU: the normal-burst kernel's asm blocks are what tools/gen_nb_asm.py emits, the
runner of tools/measure.py (A/B order, summary, stop at the first failing step) and its counter aggregator, the rule
every GPU step of a shell recipe follows (its own `timeout -k`, no `|| true`), and what the scheduler benches share
(tools/bench_rounds.py: the round driver, the two timing loops on a stand-in for torch, every tool's summarise() against
its committed profile)."""
import argparse
import csv
import glob
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_generator_reproduces_the_committed_asm_blocks(tmp_path):
    out = tmp_path / "trx_nb_asm.inc"
    _tool("gen_nb_asm").main(str(out))
    with open(os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_nb_asm.inc"), "rb") as f:
        assert out.read_bytes() == f.read()


def test_counter_aggregator_per_unit_means(tmp_path):
    rows = []
    for launch in range(4):
        for kernel in ("nb_pull4_kernel(float const*, int)", "burst_pull4_kernel<false, false, true, true>(float*)"):
            for counter, base in (("SQ_INSTS_VALU", 1000.0), ("SQ_INSTS_LDS", 300.0)):
                scale = 2.0 if kernel.startswith("burst") else 1.0
                rows.append({"Dispatch_Id": launch, "Kernel_Name": kernel, "Counter_Name": counter,
                             "Counter_Value": scale * base * (launch + 1)})
    d = tmp_path / "pmc" / "host" / "1234"
    d.mkdir(parents=True)
    with open(d / "q_counter_collection.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    got = _tool("measure").aggregate(glob.glob(str(tmp_path / "pmc" / "**" / "*counter_collection.csv"), recursive=True), 10)
    # mean over launches of base * (1, 2, 3, 4) = 2.5 * base, per unit: / 10
    assert got == {"nb_pull4_kernel": {"SQ_INSTS_LDS": 75.0, "SQ_INSTS_VALU": 250.0},
                   "burst_pull4_kernel<false, false, true, true>": {"SQ_INSTS_LDS": 150.0, "SQ_INSTS_VALU": 500.0}}


def _ab(tmp_path, stub):
    trail = tmp_path / "trail.txt"
    code = f"import json, os, sys; T = {str(trail)!r}; v = os.environ.get('V', '1'); " + stub
    cmd = [sys.executable, os.path.join(TOOLS, "measure.py"), "ab", "--rounds", "2", "--arm", "a", "--arm", "b:V=2",
           "--out", str(tmp_path), "--timeout", "60", "--field", "value", "--field", "c.configs[2].m", "--", sys.executable, "-c", code]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    return p, trail.read_text().split()


def test_ab_alternates_arms_and_summarises(tmp_path):
    # each run: value = 10 * V + the number of runs before it; configs[2].m = V
    p, trail = _ab(tmp_path, "k = len(open(T).read().split()) if os.path.exists(T) else 0; open(T, 'a').write(v + '\\n'); "
                             "print('log line'); print(json.dumps({'value': 10 * int(v) + k, 'c': {'configs[2]': {'m': int(v)}}}))")
    assert p.returncode == 0, p.stderr
    assert trail == ["1", "2", "2", "1"]                       # a b, then b a
    summary = {tuple(ln.split()[:2]): ln.split() for ln in p.stdout.splitlines() if "±" in ln}
    assert float(summary[("value", "a")][2]) == pytest.approx((10 + 13) / 2)
    assert float(summary[("value", "b")][2]) == pytest.approx((21 + 22) / 2)
    assert float(summary[("value", "b")][-1]) == pytest.approx(21.5 / 11.5, abs=1e-4)
    assert summary[("c.configs[2].m", "b")][2] == "2.0000" and summary[("c.configs[2].m", "b")][5] == "(n=2)"


def test_ab_stops_at_the_first_failing_step(tmp_path):
    p, trail = _ab(tmp_path, "open(T, 'a').write(v + '\\n'); print(json.dumps({'value': 1, 'c': {'configs[2]': {'m': 1}}})); "
                             "sys.exit(3 if v == '2' else 0)")
    assert p.returncode == 3
    assert trail == ["1", "2"]                                 # nothing started after arm b's first run
    assert "step b (round 1) failed with exit status 3" in p.stderr


def test_shell_recipes_run_every_gpu_step_under_a_time_limit():
    scripts = sorted(glob.glob(os.path.join(TOOLS, "*.sh")))
    assert scripts
    for path in scripts:
        text = open(path).read()
        for n, line in enumerate(text.splitlines(), 1):
            s = line.strip()
            if s.startswith("#") or not re.search(r"(^|\s)(python3|rocprofv3|\S*bench\.py)(\s|$)", s):
                continue
            where = f"{os.path.basename(path)}:{n}: {s}"
            if s.startswith("step "):                          # step <seconds> <log> <command...>
                assert re.search(r"^step\(\) \{[^}]*\n\s*timeout -k \d+ \$t ", text, re.M), where
            else:
                assert re.match(r"timeout -k \d+ \d+ (python3|rocprofv3) ", s), where
            assert not s.endswith("|| true"), where


# ---- tools/bench_rounds.py: what the scheduler benches share -------------------------------------------------------------

BENCHES = ("rx_frontend", "rx_sched", "rx_sched_frontend", "rx_sched_va", "sch_sync", "ms_rx", "ms_sched", "ms_group", "ms_tx",
           "ms_tx_group", "ms_agc")


def _bench_tool(name):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)                              # the tools import measure / bench_rounds by name
    return _tool(name)


def _run_rounds(tmp_path, stub, rounds=5, timeout=60, inner=4):
    """run_rounds() in a driver process of its own over a stub child -> (the driver, the stub's trail of [pid, argv...] lines)"""
    trail = tmp_path / "trail.txt"
    child = f"import json, os, sys, time; r = int(sys.argv[sys.argv.index('--round') + 1]); " \
            f"open({str(trail)!r}, 'a').write(' '.join([str(os.getpid())] + sys.argv[1:]) + '\\n'); " + stub
    driver = f"import argparse, json, sys; sys.path.insert(0, {TOOLS!r}); import bench_rounds as br; " \
             f"a = argparse.Namespace(rounds={rounds}, inner={inner}, even_inner=True, warmup=1, reps=2, timeout={timeout}, " \
             f"logs={str(tmp_path / 'logs')!r}); " \
             f"print(json.dumps(br.run_rounds('stub', [sys.executable, '-c', {child!r}, '--size', '7'], a)))"
    p = subprocess.run([sys.executable, "-c", driver], capture_output=True, text=True, timeout=120)
    return p, [ln.split() for ln in trail.read_text().splitlines()] if trail.exists() else []


def test_run_rounds_one_fresh_child_per_round_in_order(tmp_path):
    p, trail = _run_rounds(tmp_path, "print('log line'); print(json.dumps({'a': 10 + r, 'b': {'x': r}}))")
    assert p.returncode == 0, p.stderr
    assert [t[1:] for t in trail] == [["--size", "7", "--round", str(r), "--inner", "4", "--warmup", "1", "--reps", "2"] for r in range(5)]
    assert len({t[0] for t in trail}) == 5                     # five processes
    assert json.loads(p.stdout.splitlines()[-1]) == {"a": [10, 11, 12, 13, 14], "b": [{"x": r} for r in range(5)]}
    assert sorted(os.listdir(tmp_path / "logs")) == ["stub_round_%d.log" % k for k in range(1, 6)]


def test_run_rounds_stops_at_the_first_failing_round(tmp_path):
    p, trail = _run_rounds(tmp_path, "print('said before it failed'); print(json.dumps({'a': r})); sys.exit(3 if r == 1 else 0)")
    assert p.returncode == 3
    assert [t[t.index("--round") + 1] for t in trail] == ["0", "1"]          # nothing started after the second round
    assert "step round 2 failed with exit status 3" in p.stderr and "stub_round_2.log" in p.stderr
    assert "said before it failed" in p.stderr                 # the log's tail


def test_run_rounds_ends_a_round_at_its_time_limit(tmp_path):
    p, trail = _run_rounds(tmp_path, "time.sleep(30 if r == 1 else 0); print(json.dumps({'a': r}))", timeout=1)
    assert p.returncode == 124
    assert [t[t.index("--round") + 1] for t in trail] == ["0", "1"]
    assert "step round 2 failed with exit status 124" in p.stderr


def test_run_rounds_refuses_fewer_than_five_rounds(tmp_path):
    p, trail = _run_rounds(tmp_path, "print(json.dumps({'a': r}))", rounds=4)
    assert p.returncode == 2 and "at least five rounds" in p.stderr and trail == []


def test_run_rounds_refuses_an_odd_number_of_turns_where_the_tool_asks_for_even(tmp_path):
    p, trail = _run_rounds(tmp_path, "print(json.dumps({'a': r}))", inner=5)
    assert p.returncode == 2 and "an even number of turns" in p.stderr and trail == []


class _FakeTorch:
    """Stands in for torch in the timing loops: event creation, records and synchronisations go to `log` like the legs' own
    entries; elapsed_time() is the sum of the weights of the leg calls between the two records."""

    def __init__(self, weights):
        self.log, self.cuda = [], self
        fake = self

        class Event:
            def __init__(self, enable_timing=False):
                assert enable_timing
                fake.log.append("event")

            def record(self):
                self.at = len(fake.log)
                fake.log.append("record")

            def elapsed_time(self, other):
                return float(sum(weights.get(x, 0) for x in fake.log[self.at:other.at]))
        self.Event = Event

    def synchronize(self):
        self.log.append("sync")

    def say(self, word):
        return lambda: self.log.append(word)


def _region(calls):
    return ["event", "event", "record"] + calls + ["record", "sync"]


@pytest.mark.parametrize("rnd", [0, 1])
def test_time_in_order_is_the_loop_of_the_rx_benches(rnd):
    # bench_rx_sched.py / bench_rx_sched_va.py of the parent commit (bench_rx_frontend / rx_sched_frontend / sch_sync: no prepare
    # step): the legs reversed on odd rounds; per leg its prepare step, `warmup` calls, synchronize, two events, record, `reps`
    # calls, record, synchronize; elapsed / reps
    br = _bench_tool("bench_rounds")
    t = _FakeTorch({"a": 2.0, "b": 3.0, "c": 5.0})
    legs = {"a": (None, t.say("a")), "b": (t.say("prep_b"), t.say("b")), "c": (None, t.say("c"))}
    a = argparse.Namespace(round=rnd, warmup=2, reps=3)
    got = br.time_in_order(t, legs, ["a", "b", "c"], a)
    want = []
    for name in (["a", "b", "c"] if rnd == 0 else ["c", "b", "a"]):
        want += (["prep_b"] if name == "b" else []) + [name] * 2 + ["sync"] + _region([name] * 3)
    assert t.log == want
    assert got == {"a": 2.0, "b": 3.0, "c": 5.0} and list(got) == (["a", "b", "c"] if rnd == 0 else ["c", "b", "a"])
    # bench_rx_sched_va.py's small case: 20 times the reps, the same warm-up
    t.log.clear()
    assert br.time_in_order(t, legs, ["a"], a, reps=60) == {"a": 2.0}
    assert t.log == ["a"] * 2 + ["sync"] + _region(["a"] * 60)


def _turns(rnd, inner, names):
    return [n for i in range(inner) for n in (names if (rnd + i) % 2 == 0 else names[::-1])]


@pytest.mark.parametrize("rnd", [0, 1])
@pytest.mark.parametrize("untimed_first", [False, True])
def test_time_in_turns_is_the_loop_of_the_ms_receive_benches(rnd, untimed_first):
    # bench_ms_rx.py / bench_ms_sched.py (untimed_first=False) and bench_ms_group.py / bench_ms_agc.py (True) of the parent commit:
    # `warmup` bare calls of every leg, one synchronize; per turn and leg two events, [one untimed call,] record, `reps` calls,
    # record, synchronize; elapsed / reps / per; the round's value is the median over the turns
    br = _bench_tool("bench_rounds")
    t = _FakeTorch({"g": 6.0, "s": 51.0})
    legs = {"g": (t.say("g"), 1), "s": (t.say("s"), 51), "unused": (t.say("unused"), 1)}
    a = argparse.Namespace(round=rnd, warmup=2, reps=3, inner=3)
    got = br.time_in_turns(t, legs, ["g", "s"], a, untimed_first=untimed_first)
    want = ["g", "g", "s", "s", "sync"]
    for name in _turns(rnd, 3, ["g", "s"]):
        want += ["event", "event"] + ([name] if untimed_first else []) + ["record"] + [name] * 3 + ["record", "sync"]
    assert t.log == want
    assert got == {"g": 6.0, "s": 1.0}


@pytest.mark.parametrize("rnd", [0, 1])
@pytest.mark.parametrize("untimed_first", [False, True])
def test_time_in_turns_with_prepare_steps_is_the_loop_of_the_ms_uplink_benches(rnd, untimed_first):
    # bench_ms_tx.py (untimed_first=False; every leg call by call) and bench_ms_tx_group.py (True) of the parent commit.  A leg with
    # a prepare step: per call prepare, two events, record, the call, record, synchronize; the sum / reps / per.  A leg without
    # (bench_ms_tx_group.py): one region of all calls.  The warm-up is the same with `warmup` calls, the untimed call the same
    # with one call, in front of every turn's timed calls.
    br = _bench_tool("bench_rounds")
    t = _FakeTorch({"big": 4.0, "frames": 34.0})
    legs = {"big": (t.say("submit"), t.say("big"), 1), "frames": (None, t.say("frames"), 17)}
    a = argparse.Namespace(round=rnd, warmup=2, reps=3, inner=2)
    got = br.time_in_turns(t, legs, ["big", "frames"], a, untimed_first=untimed_first)

    def run(name, n):
        return (["submit"] + _region(["big"])) * n if name == "big" else _region(["frames"] * n)
    want = run("big", 2) + run("frames", 2)
    for name in _turns(rnd, 2, ["big", "frames"]):
        want += (run(name, 1) if untimed_first else []) + run(name, 3)
    assert t.log == want
    assert got == {"big": 4.0, "frames": 2.0}


def test_select_legs():
    br = _bench_tool("bench_rounds")
    assert br.select_legs({"a": 1, "b": 2, "c": 3}, "") == ["a", "b", "c"]
    assert br.select_legs(["a", "b", "c"], "c,a") == ["a", "c"]


def _profile(name):
    with open(os.path.join(ROOT, "profiles", name + "_bench.json")) as f:
        return json.load(f)


def _records():
    """(id, tool, committed record, the per-round values its driver collected, its options)"""
    N = argparse.Namespace

    def ms(rec):
        return {k: v["ms"] for k, v in rec["legs"].items()}

    def opts(rec, **kw):
        return N(rounds=rec["rounds"], reps=rec["reps"], inner=rec.get("inner"), **kw)
    r = _profile("rx_sched")
    s1 = r.pop("sps1")
    yield "rx_sched", "bench_rx_sched", r, ms(r), opts(r, slots=r["slots"], sps=4)
    yield "rx_sched.sps1", "bench_rx_sched", s1, ms(s1), opts(s1, slots=s1["slots"], sps=1)
    r = _profile("rx_frontend")
    yield "rx_frontend", "bench_rx_frontend", r, ms(r), opts(r, blocks=r["blocks"])
    for key, r in _profile("rx_sched_frontend").items():
        per = ms(r)
        names = list(per)                                      # a child reports the order it timed in: reversed on odd rounds
        per["order"] = [names[::-1] if k % 2 else names for k in range(r["rounds"])]
        yield "rx_sched_frontend." + key, "bench_rx_sched_frontend", r, per, opts(r, blocks=r["blocks"])
    r = _profile("rx_sched_va")                                # a child reports {case: {leg: ms}}
    per = {c: [{leg: v["legs"][leg]["ms"][k] for leg in v["legs"]} for k in range(r["rounds"])] for c, v in r["cases"].items()}
    yield "rx_sched_va", "bench_rx_sched_va", r, per, opts(r, slots=1 << 18)
    r = _profile("sch_sync")
    yield "sch_sync", "bench_sch_sync", r, ms(r), opts(r, slots=r["slots"], bufs=r["bufs"])
    for n in ("ms_rx", "ms_sched", "ms_tx"):
        r = _profile(n)
        yield n, "bench_" + n, r, ms(r), opts(r, slots=r["slots"])
    for n in ("ms_group", "ms_tx_group", "ms_agc"):
        r = _profile(n)
        yield n, "bench_" + n, r, ms(r), opts(r, slots=r["slots"], frames=r["frames_per_call"])


# what summarise() does not write or cannot reproduce from the committed (4-place) per-round values, by path
EXEMPT = {
    "kernel_trace_us": "from the kernel trace",
    "new_kernels_us_per_pull": "rx_sched: from the kernel trace",
    "pull_minus_two_calls_minus_new_kernels_ms": "rx_sched: from the kernel trace",
    "allowed_excess_ms": "rx_sched --sps 1: from the kernel trace",
    "within_allowance": "rx_sched --sps 1: from the kernel trace",
    "stream_vs_row_kernel_us": "rx_sched --sps 1: from the kernel trace",
    "stream_vs_row_kernel_ns_per_slot": "rx_sched --sps 1: from the kernel trace",
    "new_kernels": "rx_sched_va: from the kernel trace",
    "level_pass": "ms_agc: from the kernel trace",
    "resource_usage": "from tools/resource_usage.sh",
    "note": "rx_frontend: written by hand into the committed file",
    "parent_legs": "rx_frontend: written by hand into the committed file",
    "branch_within_parent_range": "rx_frontend: written by hand into the committed file",
    "legs.resamp_52_75_one_pass.frac_of_8tbs": "rx_frontend: 3 places of bytes / median; the median's 4th place moves the 3rd (0.516 / 0.517)",
    "cases.s16_8.legs.composition.ns_per_slot": "rx_sched_va: median * 1e6 / 8 slots: the median's rounding (5e-5 ms) is 6 ns",
    "cases.s16_8.legs.pull.ns_per_slot": "rx_sched_va: the same",
    "cases.cf32_8.legs.composition.ns_per_slot": "rx_sched_va: the same",
    "cases.cf32_8.legs.pull.ns_per_slot": "rx_sched_va: the same",
}


def _differences(path, got, want, out):
    if path in EXEMPT:
        return
    if isinstance(want, dict) and isinstance(got, dict):
        for k in sorted(set(want) | set(got)):
            p = (path + "." if path else "") + k
            if p in EXEMPT and k not in got:
                continue
            if k not in got or k not in want:
                out.append((p, "only in the committed file" if k in want else "only in summarise()"))
            else:
                _differences(p, got[k], want[k], out)
    elif isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        for k, (g, w) in enumerate(zip(got, want)):
            _differences("%s[%d]" % (path, k), g, w, out)
    elif isinstance(want, float) and isinstance(got, float):
        # within 1e-4: the values are decimals of 4 places, so one unit of the last place (as floats 0.1114 - 0.1113 > 1e-4)
        if abs(got - want) > 1e-4 + 1e-9:
            out.append((path, got, want))
    elif got != want or type(got) is not type(want):
        out.append((path, got, want))


@pytest.mark.parametrize("case", list(_records()), ids=lambda c: c[0])
def test_summarise_reproduces_the_committed_profile(case):
    _, tool, want, per_leg, a = case
    got = _bench_tool(tool).summarise(per_leg, a)
    out = []
    _differences("", got, want, out)
    assert out == []


@pytest.mark.parametrize("name", BENCHES)
def test_bench_driver_answers_help_without_torch(name, tmp_path):
    (tmp_path / "torch.py").write_text("raise ImportError('the driver must not import torch')\n")
    p = subprocess.run([sys.executable, os.path.join(TOOLS, "bench_%s.py" % name), "--help"], capture_output=True, text=True, timeout=60,
                       env={**os.environ, "PYTHONPATH": str(tmp_path)})
    assert p.returncode == 0, p.stderr
    for flag in ("--rounds", "--warmup", "--reps", "--timeout", "--out", "--logs"):
        assert flag in p.stdout
    assert "--round " not in p.stdout and "--legs" not in p.stdout         # the child's options stay hidden
