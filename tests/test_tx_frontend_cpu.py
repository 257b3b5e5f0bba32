"""The transmit front end's C ABI without a GPU: every entry point exists and refuses a call without a context or front end
(there is no CPU path), and the geometry constants of include/trxhip.h."""
import ctypes as C
import os

from osmo_trx_amd import trxhip

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tx_frontend_entry_points_refuse_without_a_context():
    L = trxhip.load_library()
    out = C.c_void_p()
    buf = (C.c_float * 16)()
    assert L.trxhip_tx_frontend_create(None, 0, 3, 260, 48, 65, 1.0, C.byref(out)) == EINVAL
    assert L.trxhip_tx_frontend_create(None, 1, 1, 260, 96, 65, 0.45, C.byref(out)) == EINVAL
    assert out.value is None
    assert L.trxhip_tx_frontend_reset(None, None) == EINVAL
    assert L.trxhip_tx_frontend_seed(None, buf, 260, 1, None) == EINVAL
    assert L.trxhip_tx_frontend_push(None, buf, 260, 1, buf, None, 1.0, None) == EINVAL
    L.trxhip_tx_frontend_destroy(None)
    assert L.trxhip_synthesize_batch(None, buf, 192, buf, 1, 4, 192, 16, None) == EINVAL


def test_tx_frontend_modes_in_header_and_binding():
    with open(os.path.join(ROOT, "include", "trxhip.h")) as f:
        h = f.read()
    assert "#define TRXHIP_TXFE_MULTI  0" in h and "#define TRXHIP_TXFE_RESAMP 1" in h
    assert (trxhip.TXFE_MULTI, trxhip.TXFE_RESAMP) == (0, 1)
