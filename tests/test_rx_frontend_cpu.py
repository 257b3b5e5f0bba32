"""The receive front end per logical channel without a GPU: the two new entry points are exported and declared, the mode
constants of include/trxhip.h match the binding, every entry point refuses a call without a context (there is no CPU path),
and MultiArfcnRx::getLogicalChan agrees with the binding's map.  The refusals that need a context are checked on the device
(tests/test_gpu_rx_frontend_chans.py)."""
import ctypes as C
import os
import re
import subprocess

from osmo_trx_amd import trxhip

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "osmo_trx_amd", "lib")

# (mode, chans, block_len, p, q): section "Refused with TRXHIP_EINVAL" of the header
REFUSED = [(2, 1, 192, 65, 48), (-1, 1, 192, 65, 48),                        # unknown mode
           (0, 0, 192, 65, 48), (0, 4, 192, 65, 48), (1, 0, 1536, 65, 96), (1, 2, 1536, 65, 96), (1, 3, 1536, 65, 96),   # chans
           (0, 3, 8, 1, 1), (0, 3, 192, 0, 48), (0, 3, 192, 129, 48), (0, 3, 192, 65, 0), (0, 3, 3073, 65, 3073),     # geometry
           (0, 3, 191, 65, 48), (1, 1, 1500, 65, 96), (1, 1, 3072, 1, 3072)]        # block_len % q, q * ceil(256 / p) > 3072


def test_new_calls_are_exported_and_declared():
    nm = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libtrxhip.so")], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    with open(os.path.join(ROOT, "include", "trxhip.h")) as f:
        h = f.read()
    for name in ("trxhip_rx_frontend_create_chans", "trxhip_rx_frontend_rows"):
        assert name in exported, name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in trxhip.SYMBOLS
    L = trxhip.load_library()
    assert L.trxhip_rx_frontend_create_chans.argtypes is not None and len(L.trxhip_rx_frontend_create_chans.argtypes) == 7
    assert len(L.trxhip_rx_frontend_rows.argtypes) == 1


def test_rx_frontend_modes_in_header_and_binding():
    with open(os.path.join(ROOT, "include", "trxhip.h")) as f:
        h = f.read()
    assert "#define TRXHIP_RXFE_MULTI  0" in h and "#define TRXHIP_RXFE_RESAMP 1" in h
    assert (trxhip.RXFE_MULTI, trxhip.RXFE_RESAMP) == (0, 1)
    assert "#define TRXHIP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", h)


def test_rx_frontend_entry_points_refuse_without_a_context():
    L = trxhip.load_library()
    out = C.c_void_p()
    buf = (C.c_float * 16)()
    assert L.trxhip_rx_frontend_create_chans(None, 0, 3, 192, 65, 48, C.byref(out)) == EINVAL
    assert L.trxhip_rx_frontend_create_chans(None, 1, 1, 1536, 65, 96, C.byref(out)) == EINVAL
    assert L.trxhip_rx_frontend_create_chans(None, 0, 3, 192, 65, 48, None) == EINVAL
    assert out.value is None
    assert L.trxhip_rx_frontend_rows(None) == EINVAL
    assert L.trxhip_rx_frontend_reset(None, None) == EINVAL
    assert L.trxhip_rx_frontend_seed(None, buf, 1, None) == EINVAL
    assert L.trxhip_rx_frontend_pull(None, buf, 1, buf, 260, None) == EINVAL
    L.trxhip_rx_frontend_destroy(None)


def test_refusal_list_through_ctypes():
    """Without a GPU there is no context to hand over, so each refused tuple is checked to come back TRXHIP_EINVAL and to leave
    `out` alone; with a context the same list is checked on the device."""
    L = trxhip.load_library()
    for args in REFUSED:
        out = C.c_void_p()
        assert L.trxhip_rx_frontend_create_chans(None, *args, C.byref(out)) == EINVAL, args
        assert out.value is None, args


def test_get_logical_chan_agrees_with_the_binding():
    sa = C.CDLL(os.path.join(LIBDIR, "libtrxsigproc_sa.so"))
    f = getattr(sa, "_ZN12MultiArfcnRx14getLogicalChanEmm")                # static int MultiArfcnRx::getLogicalChan(size_t, size_t)
    f.restype, f.argtypes = C.c_int, [C.c_size_t, C.c_size_t]
    assert trxhip.RXFE_PCHAN == {1: (0,), 2: (0, 3), 3: (1, 0, 3)}            # radioInterfaceMulti.cpp:92-124
    for chans in (1, 2, 3):
        pch = trxhip.RXFE_PCHAN[chans]
        assert len(pch) == chans
        for pchan in range(4):
            want = pch.index(pchan) if pchan in pch else -1
            assert f(pchan, chans) == want, (pchan, chans)
    for chans in (0, 4):
        for pchan in range(4):
            assert f(pchan, chans) == -1
