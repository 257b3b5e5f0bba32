"""The uplink scheduler behind the receive front end, without a GPU: the constants and exports of
trxhip_rx_sched_pull_frontend(), what a plan-only scheduler refuses, and the slot arithmetic the GPU tests of
tests/test_gpu_rx_sched_frontend.py rely on (which pulls of their block sequences cut nothing, and which begin a slot of
157 or of 156 samples in the carried remainder)."""
import ctypes as C
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from osmo_trx_amd import trxhip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
NEW = ("trxhip_rx_frontend_out_samples", "trxhip_rx_sched_slots_frontend", "trxhip_rx_sched_pull_frontend")
MULTI_SEQ = (1, 2, 3, 1, 5, 7, 2, 11, 4, 13, 6, 17)             # blocks per pull, cycled over the 125-block stream
SPS1_SEQ = (1, 2, 1, 3, 1, 1, 2, 5, 1, 4)                       # the same for the 1-SPS stream of 40 blocks


def header():
    with open(os.path.join(ROOT, "include", "trxhip.h")) as f:
        return f.read()


def test_work_head_is_640_and_abi_stays():
    h = header()
    assert re.search(r"^#define\s+TRXHIP_RX_SCHED_WORK_HEAD\s+640\b", h, re.M)
    assert re.search(r"^#define\s+TRXHIP_ABI_VERSION\s+5\b", h, re.M)
    assert trxhip.RX_SCHED_WORK_HEAD == 640
    with open(os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_rx_sched.h")) as f:
        assert re.search(r"^#define\s+TRX_RXS_REM_STRIDE\s+640u", f.read(), re.M)      # the head holds one remainder


def test_new_symbols_are_declared_bound_and_exported():
    h = header()
    L = trxhip.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert name in trxhip.SYMBOLS and hasattr(L, name), name
    assert L.trxhip_abi_version() == 5


def test_out_samples_of_no_object_is_zero():
    assert trxhip.load_library().trxhip_rx_frontend_out_samples(None, 7) == 0


def test_plan_only_scheduler_refuses_the_join():
    """ctx == NULL: no device memory, so no front end can belong to it -- refused whatever else is passed, state untouched"""
    L = trxhip.load_library()
    s = trxhip.RxScheduler(None, chans=3)
    s.set_clock(10, 3)
    assert s.pull(n_samples=1000) == (1, 375)
    fake = C.c_void_p(0x1000)                                    # never dereferenced: the scheduler is looked at first
    ns, nc = C.c_size_t(99), C.c_size_t(99)
    for fe in (None, fake):
        assert L.trxhip_rx_sched_slots_frontend(s.h, fe, 4) == EINVAL
        assert L.trxhip_rx_sched_pull_frontend(s.h, fe, None, 4, None, 0, None, 0, None, None, None, 0, C.byref(ns), C.byref(nc),
                                               None) == EINVAL
        assert L.trxhip_rx_sched_pull_frontend(s.h, fe, None, 0, None, 0, None, 0, None, None, None, 0, C.byref(ns), C.byref(nc),
                                               None) == EINVAL
    assert L.trxhip_rx_sched_slots_frontend(None, fake, 4) == EINVAL
    assert L.trxhip_rx_sched_pull_frontend(None, fake, None, 4, None, 0, None, 0, None, None, None, 0, None, None, None) == EINVAL
    assert (ns.value, nc.value) == (99, 99)
    assert s.clock() == (10, 4) and s.slots(0) == 0 and s.slots(251) == 1      # 375 carried, as before
    s.close()


def pulls(s, seq, blocks, per_block):
    """plan-only: the (tn, carried, n_slots) of every pull of the cycled block sequence over `blocks` blocks"""
    out, at, i = [], 0, 0
    while at < blocks:
        nb = min(seq[i % len(seq)], blocks - at)
        tn, carried = s.clock()[1], s.carried
        n, _ = s.pull(n_samples=nb * per_block)
        out.append((nb, tn, carried, n))
        at += nb
        i += 1
    return out


def test_multi_block_sequence_covers_the_cases():
    """125 blocks of 260 samples: 52 slots' worth, the strict `>` cuts 51 and carries 625; the sequence holds pulls that only
    carry (with and without a remainder in front) and pulls whose first slot begins in the remainder"""
    s = trxhip.RxScheduler(None, chans=3)
    s.set_clock(0, 0)
    assert s.pull(n_samples=125 * 260) == (51, 625)
    s.set_clock(0, 0)
    p = pulls(s, MULTI_SEQ, 125, 260)
    assert [x[0] for x in p[:8]] == [1, 2, 3, 1, 5, 7, 2, 11]
    assert [x[3] for x in p[:8]] == [0, 1, 1, 0, 2, 3, 1, 5]
    assert sum(x[3] for x in p) == 51 and s.carried == 625
    assert any(n == 0 and c == 0 for _, _, c, n in p) and any(n == 0 and c > 0 for _, _, c, n in p)
    assert sum(1 for _, _, c, n in p if n > 0 and c > 0) >= 8
    s.close()


@pytest.mark.parametrize("tn0", [0, 1, 2, 3])
def test_sps1_block_sequence_begins_both_slot_lengths_in_the_remainder(tn0):
    s = trxhip.RxScheduler(None, chans=1, sps=1)
    s.set_clock(7, tn0)
    p = pulls(s, SPS1_SEQ, 40, 260)
    straddle = [tn % 4 == 0 for _, tn, c, n in p if n > 0 and c > 0]
    assert True in straddle and False in straddle, p                    # a 157-sample and a 156-sample slot 0
    total = sum(n for _, _, _, n in p)
    assert total in (66, 67) and s.carried == 40 * 260 - (total // 4 * 625 + sum(156 + ((tn0 + total // 4 * 4 + i) % 4 == 0)
                                                                                 for i in range(total % 4)))
    s.close()
