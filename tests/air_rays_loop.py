"""The dispersive channel of the two loops through the air interface: per path two rays, {1, d} and
{g2, d + 8 samples, a quarter turn}, an echo two symbols behind the direct ray.  The uplink's 18 bursts are those of
tests/test_gpu_air.py's uplink_loop; here they are rendered on the CPU -- the placement by tests/ms_tx_model.py, the samples by
the oracle's modulator cast as the product casts them -- sent through the host object and cut into the slots the BTS reads, for
the oracle's pullRadioVector() chain with and without use_va.  The radio reads 20 samples early, as the use_va flow wants it
(tests/test_gpu_rx_sched_va.py): rxtx_delay is test_gpu_air's -18 plus 20."""
import functools

import numpy as np

import ms_tx_model as M
import ms_tx_nco_model as TN
from osmo_trx_amd import trxhip

UL_TNS, UL_DELAYS, UL_TA = (1, 2, 5), (0, 8, 20), (0, 2, 5)
UL_RXTX_DELAY = -18 + 20
TSC, FRAMES, CLOCK = 5, 6, (5000, 2, 40 * 625)
ECHO, QUARTER = 8, 1 << 30
LADDER = (0.7, 0.5, 0.35, 0.25)
G2 = 0.5                               # the largest of the ladder at which the oracle's Viterbi chain has no wrong bit (the CPU test)
N_SLOTS = (FRAMES + 4) * 8
N = N_SLOTS * 625 + 1


def two_rays(delay, g2, hz=0.0):
    return [dict(gain=1.0, delay=delay, hz=hz, phase=0), dict(gain=g2, delay=delay + ECHO, hz=hz, phase=QUARTER)]


@functools.lru_cache(maxsize=None)
def bursts():
    """(member, fn, tn, bits uint8[18, 148]) as uplink_loop draws them"""
    from test_gpu_tx_frontend import _unambiguous_bursts
    rng = np.random.default_rng(77)
    member = np.tile(np.arange(3), FRAMES)
    fn = np.repeat(CLOCK[0] + 2 + np.arange(FRAMES), 3)
    tn = np.asarray(UL_TNS)[member]
    return member, fn, tn, _unambiguous_bursts(np.full(len(fn), TSC), rng)


def air_of(trx, g2):
    air = trxhip.AirChannel(trx, 3, max_delay=32, seed=1)
    for m in range(3):
        air.set_rays(trxhip.AIR_UL, m, two_rays(UL_DELAYS[m], g2))
    air.set_noise(trxhip.AIR_UL, 0, 12.0)
    return air


@functools.lru_cache(maxsize=None)
def oracle_uplink(g2):
    """{use_va: (found[18], wrong hard bits 3 .. 144 [18])} of the oracle's chain over the CPU-rendered stream"""
    import oracle_lib as O
    member, fn, tn, bits = bursts()
    rows = np.zeros((3, N, 2), np.int16)
    for m in range(3):
        tx = M.MsTx(2047, UL_RXTX_DELAY, 32)
        tx.set_ta(UL_TA[m])
        idx = np.flatnonzero(member == m)
        plan = tx.submit([(fn[i], tn[i], 0) for i in idx], CLOCK)
        assert all(p["status"] == M.QUEUED for p in plan)
        at = {p["radio_ts"]: (i, p["scale"]) for i, p in zip(idx, plan)}
        drawn, pieces = tx.render(N, CLOCK[2])
        assert drawn == FRAMES
        for off, first, length, ts in pieces:
            i, scale = at[ts]
            rows[m, off:off + length] = TN.cast(TN.scaled(O.modulate_burst(bits[i], 8, 4), scale))[first:first + length]
    y = air_of(None, g2).uplink(rows, CLOCK[2])
    ul = M.Time(CLOCK[0], CLOCK[1]).decTN(3)
    slots = np.stack([y[s * 625:(s + 1) * 625] for s in ((int(f) - ul.fn) * 8 + int(t) - ul.tn for f, t in zip(fn, tn))])
    p = np.zeros(len(slots), dtype=O.PARAMS_DTYPE)
    p["type"], p["tsc"], p["max_toa"] = 1, TSC, 20
    out = {}
    for use_va in (True, False):
        chain = O.pull_radio_vector_chain(slots, p, 1, use_va=use_va)
        found = np.array([code == 0 and not bi.idle for code, bi, _, _ in chain])
        hard = np.stack([(np.frombuffer(bi.rx_burst, dtype=np.float32)[:148] > 0.5).astype(np.uint8) for _, bi, _, _ in chain])
        out[use_va] = (found, (hard[:, 3:145] != bits[:, 3:145]).sum(axis=1))
    return out
