"""Jumps and tests on the normal-burst kernel's main path as hipcc compiled it (tools/isa_guard_nb.py), and the generated blocks
against their generator (tools/gen_nb_asm.py).  The common burst -- a normal-burst slot, detected, every decision certified,
straight-line geometry, max_toa 3 -- executes at most 22 branch instructions through the burst loop, the hand-placed blocks
included, and at most 3 of them are taken: block CORR's computed jump, its variant's exit, the back edge.  No block holds cold
code between its entry and its exit on that path.  Runs without a GPU (hipcc cross-compiles gfx950)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def compiled():
    m = tool("isa_guard_nb")
    return m.check(m.assembly())


@needs_hipcc
def test_branches_on_the_main_path(compiled):
    errs, info = compiled
    main = info["loop_main_path"]
    print({k: main[k] for k in ("branches_outside_blocks", "branches_inside_blocks", "branches", "taken_on_main_path", "taken")})
    assert not errs, (errs, info)
    assert main["branches"] == main["branches_outside_blocks"] + main["branches_inside_blocks"]
    assert main["branches"] <= 22, main
    assert main["taken_on_main_path"] <= 3, main["taken"]
    assert main["cold_labels_inside_blocks"] == [], main


@needs_hipcc
def test_resources(compiled):
    _, info = compiled
    assert info["vgpr_count"] == 128
    assert info["sgpr_count"] <= 106
    assert info["sgpr_spill_count"] == 0 and info["vgpr_spill_count"] == 0 and info["private_segment_fixed_size"] == 0


def test_generated_blocks_match_the_generator(tmp_path):
    out = tmp_path / "trx_nb_asm.inc"
    tool("gen_nb_asm").main(str(out))
    committed = open(os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_nb_asm.inc")).read()
    assert out.read_text() == committed


@needs_hipcc
def test_diag_build_compiles(tmp_path):
    """the per-phase cycle accounting (-DTRX_DIAG, tools/phase_cycles_nb.py) still compiles: device code of the burst kernels"""
    import subprocess
    from osmo_trx_amd import build as B
    flags = [f for f in B.COMMON if not f.startswith("-W")]
    subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-DTRX_DIAG"] + flags + ["-w", "-I" + os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", str(tmp_path / "k4_diag.s"), os.path.join(B.CSRC, "trx_kernel4.hip")],
                   check=True, capture_output=True)
    assert "s_memtime" in (tmp_path / "k4_diag.s").read_text()
