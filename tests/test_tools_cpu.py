"""The measurement tools without a GPU: the normal-burst kernel's asm blocks are what tools/gen_nb_asm.py emits, the
runner of tools/measure.py (A/B order, summary, stop at the first failing step) and its counter aggregator, and the rule
every GPU step of a shell recipe follows (its own `timeout -k`, no `|| true`)."""
import csv
import glob
import importlib.util
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
