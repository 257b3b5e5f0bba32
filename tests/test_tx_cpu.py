"""Transmit side without a GPU: the transmit tables against the oracle, the C ABI's refusal without a context, and the seven
sigProcLib Tx calls in both shim builds (plus, where the reference checkout is present, a reference-compiled caller that links
them from libtrxsigproc.so instead of a sigProcLib.o)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from osmo_trx_amd import build as trx_build, synth, trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
LIBDIR = os.path.join(ROOT, "osmo_trx_amd", "lib")

# struct trx_tx_tables, osmo_trx_amd/csrc/trx_tx_tables.h
TX_TABLES = np.dtype([
    ("magic", "<u4"), ("version", "<u4"), ("pulse4_c0", "<f4", 16), ("pulse4_c1", "<f4", 8), ("pulse1_c0", "<f4", 4),
    ("pad0", "<f4", 4), ("rot4", "<c8", 625), ("pad1", "<c8", 3), ("rot1", "<c8", 157), ("pad2", "<c8", 3),
    ("psk8", "<c8", 8), ("edge_rot", "<c8", 156), ("dummy_burst", "u1", 148), ("rach_burst", "u1", 49), ("pad3", "u1", 3),
    ("tsc", "u1", (8, 26)), ("edge_tsc", "u1", (8, 78))])



@pytest.fixture(scope="module")
def lib():
    trx_build.build_all()
    return trxhip.load_library()


def _bits(s):
    return np.array([c == "1" for c in s], dtype=np.uint8)


def edge_phasors():
    """(cos(phase), sin(phase)) with float phase = i * 3.0f * M_PI / 8.0f, recomputed with the same float / double expression
    and the C library's cosf / sinf -- the functions orc_modulate_edge_burst calls."""
    libm = C.CDLL("libm.so.6")
    for f in (libm.cosf, libm.sinf):
        f.restype, f.argtypes = C.c_float, [C.c_float]
    out = np.zeros(156, dtype=np.complex64)
    for i in range(156):
        ph = np.float32(np.float64(np.float32(i) * np.float32(3.0)) * np.pi / np.float64(np.float32(8.0)))
        out[i] = complex(np.float32(libm.cosf(float(ph))), np.float32(libm.sinf(float(ph))))
    return out


def test_tx_tables_match_the_oracle(lib):
    assert lib.trxhip_tx_tables_size() == TX_TABLES.itemsize
    t = np.frombuffer(trxhip.generate_tx_tables_host(), dtype=TX_TABLES)[0]
    o = O.tables()
    for k in ("pulse4_c0", "pulse4_c1", "pulse1_c0", "rot4", "rot1"):
        assert t[k].tobytes() == o[k].tobytes(), k            # bit-identical
    ph = edge_phasors()
    assert t["edge_rot"].tobytes() == ph.tobytes()
    psk8 = np.array([complex(-0.70710678, 0.70710678), complex(0.0, -1.0), complex(0.0, 1.0), complex(0.70710678, -0.70710678), -1,
                     complex(-0.70710678, -0.70710678), complex(0.70710678, 0.70710678), 1], dtype=np.complex64)
    assert t["psk8"].tobytes() == psk8.tobytes()
    for k in range(8):
        assert np.array_equal(t["tsc"][k], _bits(synth.TSC_BITS[k]))
        assert np.array_equal(t["edge_tsc"][k], _bits(synth.EDGE_TSC_BITS[k]))
    assert np.array_equal(t["rach_burst"], _bits(synth.RACH_HEAD + synth.RACH_SYNC[0]))
    # the dummy burst carries the dummy midamble (gDummyBurstTSC) where a normal burst carries its TSC
    assert np.array_equal(t["dummy_burst"][61:87], _bits("01110001011100010111000101"))


def test_edge_phasors_are_the_ones_the_oracle_modulates_with(lib):
    """One-symbol probes: a 3-bit burst puts x = psk8[idx] * edge_rot[0] at sample 4 of the upsampled vector and nothing
    else, so the oracle's shaped output is out[19 - k] = 0.0f + x * c0[k] exactly: the phasor and the map the oracle uses
    are the ones in the transmit tables."""
    t = np.frombuffer(trxhip.generate_tx_tables_host(), dtype=TX_TABLES)[0]
    c0 = t["pulse4_c0"]
    for idx in range(8):
        bits = np.array([idx & 1, (idx >> 1) & 1, (idx >> 2) & 1], dtype=np.uint8)
        out = np.zeros(640, dtype=np.complex64)
        assert O.lib().orc_modulate_edge_burst(bits.ctypes.data, 3, out.ctypes.data) == 625
        s, r = t["psk8"][idx], t["edge_rot"][0]
        x = np.complex64(complex(np.float32(s.real * r.real - s.imag * r.imag), np.float32(s.real * r.imag + s.imag * r.real)))
        # the only nonzero input sits at sample 4: out[4 + 15 - k] = x * c0[k]  (0.0f + product: exact)
        for k in range(1, 16):
            y = out[4 + 15 - k]
            assert y.real == np.float32(x.real * c0[k]) and y.imag == np.float32(x.imag * c0[k]), (idx, k)


def test_modulate_without_a_context_is_refused(lib):
    buf = (C.c_ubyte * 4096)()
    args = (buf, 148, buf, buf, None, C.c_float(0.0), 625, buf, 1, 4, None)
    assert lib.trxhip_modulate_batch(None, *args) == -22
    assert lib.trxhip_modulate_trxd_batch(None, buf, 154, buf, C.c_double(32767.0), 4, buf, None, C.c_float(0.0), 625,
                                          buf, 1, None) == -22
    assert lib.trxhip_tx_tables_generate_host(buf, 17) == -22


def _nm(path):
    return subprocess.run(["nm", "-DC", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_shims_define_the_tx_calls(lib):
    sa = _nm(os.path.join(LIBDIR, "libtrxsigproc_sa.so"))
    for sig in ("modulateBurst(trxhip_sa::BitVector const&, int, int, bool)",
                "modulateEdgeBurst(trxhip_sa::BitVector const&, int, bool)",
                "generateDummyBurst(int, int)", "generateEmptyBurst(int, int)", "generateEdgeBurst(int)",
                "genRandNormalBurst(int, int, int)", "genRandAccessBurst(int, int, int)"):
        assert " T trxhip_sa::" + sig in sa, sig
    if not os.path.isdir(REF):
        pytest.skip("needs the reference checkout for libtrxsigproc.so (container only)")
    ref = _nm(os.path.join(LIBDIR, "libtrxsigproc.so"))
    for sig in ("modulateBurst(BitVector const&, int, int, bool)", "modulateEdgeBurst(BitVector const&, int, bool)",
                "generateDummyBurst(int, int)", "generateEmptyBurst(int, int)", "generateEdgeBurst(int)",
                "genRandNormalBurst(int, int, int)", "genRandAccessBurst(int, int, int)"):
        assert " T " + sig in ref, sig


CALLER = r'''
#include <cstdio>
#include "sigProcLib.h"
static const char *s(signalVector *v) { const char *r = v ? "vector" : "null"; delete v; return r; }
int main()
{
	printf("setup %d\n", (int)sigProcLibSetup());
	BitVector bits(148), edge(444);
	for (int n = 0; n < 8; n++) {                        /* Transceiver::setFiller(), Transceiver.cpp:107-120 */
		printf("dummy %s\n", s(generateDummyBurst(4, n)));
		printf("normal %s\n", s(genRandNormalBurst(0, 4, n)));
		printf("edge %s\n", s(generateEdgeBurst(0)));
		printf("access %s\n", s(genRandAccessBurst(0, 4, n)));
		printf("empty %s\n", s(generateEmptyBurst(4, n)));
	}
	printf("mod %s\n", s(modulateBurst(bits, 8, 4)));    /* addRadioVector(), :392-396 */
	printf("modedge %s\n", s(modulateEdgeBurst(edge, 4)));
	sigProcLibDestroy();
	return 0;
}
'''


def test_reference_caller_links_tx_calls_without_sigproclib_o(lib, tmp_path):
    """Transceiver.cpp's Tx calls, compiled against the reference's headers, link against libtrxsigproc.so plus the reference's
    signalVector.cpp and BitVector.cpp -- no sigProcLib.o -- and return NULL without a GPU (no context: no CPU fallback)."""
    if not os.path.isdir(REF):
        pytest.skip("needs /root/reference (container only)")
    import torch
    inc = ["-I", REF + "/Transceiver52M", "-I", REF + "/CommonLibs", "-I", REF + "/GSM"]
    objs = []
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    for s in (str(src), os.path.join(REF, "Transceiver52M/signalVector.cpp"), os.path.join(REF, "CommonLibs/BitVector.cpp")):
        obj = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-c"] + inc + [s, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "tx_caller")
    r = subprocess.run(["g++", "-o", exe] + objs + ["-L", LIBDIR, "-ltrxsigproc", "-ltrxhip", "-Wl,-rpath," + LIBDIR,
                                                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=120)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.split("\n")
    if not torch.cuda.is_available():
        assert lines[0] == "setup 0"
        for k in ("dummy", "normal", "edge", "access", "empty", "mod", "modedge"):
            assert k + " null" in lines and k + " vector" not in lines, k
