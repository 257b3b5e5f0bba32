"""The row-pair layout of the normal-burst kernel's LDS copy of the sinc LUT (csrc/trx_tables.h: trx_sincp_idx, trx_sincp_src)
against the blob's own index (trx_sincv_swz): for every (row, column) the old index and the new one address the same value,
the staging rule fills every float of the copy exactly once, and what block DETB of tools/gen_nb_asm.py reads as one 8-byte
entry is the pair of weights of two adjacent taps -- for every fraction, fraction 0 with its column slot 512 and the zero tail
included.  The header's functions are compiled for the host and called through ctypes.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "osmo_trx_amd", "csrc")
SRC = """
#include "trx_tables.h"
extern "C" int swz(int q) { return trx_sincv_swz(q); }
extern "C" int idx(int row, int slot) { return trx_sincp_idx(row, slot); }
extern "C" int src(int i) { return trx_sincp_src(i); }
extern "C" int stride(void) { return TRX_SINCP_STRIDE; }
extern "C" int lut_len(void) { return TRX_SINCV_LEN; }
"""
LDS_FLOATS = 4096 + 32                                          # TRX_SINCV_LDS (trx_device.h)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or "g++"                           # (the host compiler of osmo_trx_amd/build.py)
    d = tmp_path_factory.mktemp("sincp")
    (d / "sincp.cpp").write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(d / "libsincp.so"), str(d / "sincp.cpp")], check=True, capture_output=True)
    return ctypes.CDLL(str(d / "libsincp.so"))


@pytest.fixture(scope="module")
def staged(lib):
    """(blob, copy): a blob sincv[] whose entry at index i is i + 1 (no two alike, none zero), and the LDS copy the kernel's
    staging loop makes of it: copy[i] = blob[trx_sincp_src(i)], 0 where that is -1"""
    blob = np.arange(1, lib.lut_len() + 1, dtype=np.int64)
    s = np.array([lib.src(i) for i in range(LDS_FLOATS)])
    return blob, np.where(s >= 0, blob[np.maximum(s, 0)], 0)


def test_old_and_new_index_address_the_same_value(lib, staged):
    blob, copy = staged
    assert lib.lut_len() == 4096 and 4 * lib.stride() <= LDS_FLOATS
    seen = set()
    for row in range(8):
        for col in range(512):
            old = lib.swz(512 * row + col)
            assert old >> 9 == row                                  # the swizzle leaves the row alone: old = 512 row + slot
            new = lib.idx(row, old & 511)
            assert copy[new] == blob[old], (row, col)
            seen.add(new)
        # slot 512: column 0 of the next row (q = 512 (row + 1)); row 8 is the zero tail (q = 4096)
        new = lib.idx(row, 512)
        assert copy[new] == (blob[lib.swz(512 * (row + 1))] if row < 7 else 0), row
        seen.add(new)
    assert len(seen) == 8 * 513 and seen == set(range(4 * lib.stride()))          # every float of the pairs, once
    assert (copy[4 * lib.stride():] == 0).all()


def test_an_eight_byte_entry_is_the_weights_of_two_adjacent_taps(lib, staged):
    """block DETB: taps fl - 7 .. fl (u = 0 .. 7) take LUT index q = 512 (7 - u) + f, taps fl + 1 .. fl + 8 take q = 512 u +
    (512 - f) (trx_device.h interp_point); the block reads byte 8 swz(f) + 4 stride (3 - u / 2) and 8 swz(512 - f) + 4 stride
    (u / 2) for even u and takes tap u from the high / low half of the entry"""
    blob, copy = staged
    want = lambda q: blob[lib.swz(q)] if q < lib.lut_len() else 0
    for f in range(512):
        for u in range(0, 8, 2):
            byte = 8 * lib.swz(f) + 4 * lib.stride() * (3 - u // 2)
            assert byte % 8 == 0 and byte // 4 + 1 < LDS_FLOATS
            lo, hi = copy[byte // 4], copy[byte // 4 + 1]
            assert (hi, lo) == (want(512 * (7 - u) + f), want(512 * (6 - u) + f)), (f, u)
            byte = 8 * lib.swz(512 - f) + 4 * lib.stride() * (u // 2)
            assert byte % 8 == 0 and byte // 4 + 1 < LDS_FLOATS
            lo, hi = copy[byte // 4], copy[byte // 4 + 1]
            assert (lo, hi) == (want(512 * u + 512 - f), want(512 * (u + 1) + 512 - f)), (f, u)


def test_the_generated_block_uses_that_stride(lib):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_nb_asm", os.path.join(ROOT, "tools", "gen_nb_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.SINCP_PAIR_BYTES == 4 * lib.stride()


def test_the_gather_has_the_bank_pattern_of_the_four_byte_one(lib):
    """ds_read_b64 on MI355X: banks (byte / 4) mod 64, conflicts among the lanes of a 32-lane half; ds_read_b32: (byte / 4) mod
    32.  An 8-byte slot s takes banks 2 s and 2 s + 1: two lanes of a half collide exactly when their slots are equal mod 32 --
    when the 4-byte gather on sincv[swz] collided.  Checked on round B's positions (e + offB[lane]) & 511 of lanes 0..29 (first
    half) and 32..47 (second half) for every e the bisection can leave (16 mod 32): both gathers are conflict-free."""
    def node_offset(n, inc0):
        lv = (n + 1).bit_length() - 1
        p = n + 1 - (1 << lv)
        return ((4 * p * inc0) >> lv) - (2 * inc0 - ((2 * inc0) >> lv))
    off_b = [node_offset(l >> 1, 8) + (1024 if l & 1 else 0) for l in range(30)] + [2 * k - 15 + 512 for k in range(16)]
    halves = (off_b[:30], off_b[30:])
    for e in range(16, 512, 32):
        for side in (lambda f: f, lambda f: 512 - f):
            for half in halves:
                slots = [lib.swz(side((e + o) & 511)) for o in half]
                for width, banks in ((4, 32), (8, 64)):
                    hit = {}
                    for s in set(slots):                            # (equal addresses broadcast)
                        for d in range(width // 4):
                            hit.setdefault((s * width // 4 + d) % banks, []).append(s)
                    assert max(len(v) for v in hit.values()) == 1, (e, width, hit)
