"""GPU parity of the MS-side downlink burst receiver: trxhip_ms_rx_batch_i16 / _cf32 vs the CPU model tests/ms_rx_model.py (pinned
to the C oracle by tests/test_ms_rx_cpu.py).  The +-127 outputs are hard decisions, the burst position comes out of a serial float
recurrence and the energy out of a serial float sum, so every comparison is equality: kind, sent, flags, start, corr_max and pow
(bit for bit), the 148 sbits and the SCH fields.  The RSSI is the floor of a double-precision logarithm: it is compared wherever
the model's value lies further than 1e-4 from an integer (many orders above what two correct log10 can differ by)."""
import ctypes as C

import numpy as np
import pytest

import ms_rx_cases as K
import ms_rx_model as M
from osmo_trx_amd import synth, trxhip

pytestmark = pytest.mark.gpu

FULL = 2047.0
EINVAL = -22
GUARD = 1e4                                                        # between the slots: must never be read
ACTIVE = trxhip.MS_SLOT_ACTIVE


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def _case(y, fn, tn, tsc, active=True, sent=None, off=None, snr=None):
    return dict(y=np.asarray(y, dtype=np.complex64), fn=fn, tn=tn, tsc=tsc, active=active, sent=sent, off=off, snr=snr)


def _traffic(rng, n, offsets, snrs=(25.0, 10.0, 0.0)):
    """n ACTIVE traffic slots cycling through offsets x SNRs x TSCs; every 13th is all zero, every 11th noise only, every 17th at
    full scale (+-32767 on both axes) and every 7th asks for another TSC than the one sent."""
    out = []
    for b in range(n):
        fn, tn, tsc = int(rng.integers(0, 2715648)), 1 + b % 7, b % 8
        if b % 13 == 12:
            out.append(_case(np.zeros(K.SLOT), fn, tn, tsc))
        elif b % 11 == 10:
            out.append(_case(K.place(rng, None, None, 0.0, float(10 ** rng.uniform(0, 3.3))), fn, tn, tsc))
        elif b % 17 == 16:
            s = rng.choice([-32767.0, 32767.0], (K.SLOT, 2))
            out.append(_case(s[:, 0] + 1j * s[:, 1], fn, tn, tsc))
        else:
            off, snr = int(offsets[b % len(offsets)]), float(snrs[(b // len(offsets)) % len(snrs)])
            y, bits = K.nb_slot(rng, tsc, off, snr, amp=float(10 ** rng.uniform(1.5, 3.3)))
            if b % 7 == 6:
                out.append(_case(y, fn, tn, (tsc + 3) % 8))
            else:
                out.append(_case(y, fn, tn, tsc, sent=bits, off=off, snr=snr))
    return out


def _slots(cases):
    s = np.zeros(len(cases), dtype=trxhip.MS_SLOT_DTYPE)
    for b, c in enumerate(cases):
        s[b] = (c["fn"], c["tn"], c["tsc"], ACTIVE if c["active"] else 0, 0)
    return s


def _run(trx, cases, stride=K.SLOT, i16=False, want_bits=True, full=FULL):
    import torch
    n = len(cases)
    x = np.full((n, stride), GUARD + 1j * GUARD, dtype=np.complex64)
    for b, c in enumerate(cases):
        x[b, :K.SLOT] = c["y"]
    if i16:
        iq = torch.from_numpy(K.to_i16(x)).to("cuda:0")
    else:
        iq = torch.from_numpy(x).to("cuda:0")
    return trx.ms_rx(iq, _slots(cases), rx_full_scale=full, want_bits=want_bits)


def _f32_bits(v):
    return np.float32(v).view(np.uint32)


def _check(rec, bits, cases, full=FULL, i16=False):
    left_out = 0
    for b, c in enumerate(cases):
        m = M.ms_rx(K.to_i16(c["y"]) if i16 else c["y"], c["fn"], c["tn"], c["tsc"], c["active"], full)
        got = rec[b]
        assert (got["fn"], got["tn"]) == (c["fn"], c["tn"]) and not got["reserved"].any(), b
        for f in ("kind", "sent", "flags", "start", "toa256", "sch_fn", "sch_rc", "sch_bsic"):
            assert got[f] == m[f], (b, f, got[f], m[f])
        assert _f32_bits(got["corr_max"]) == _f32_bits(m["corr_max"]), b
        assert _f32_bits(got["pow"]) == _f32_bits(m["pow"]), (b, got["pow"], m["pow"])
        assert np.array_equal(bits[b], m["bits"]), b
        if m["rssi_exact"] is not None and abs(m["rssi_exact"] - round(m["rssi_exact"])) < 1e-4:
            left_out += 1
        else:
            assert got["rssi"] == m["rssi"], (b, got["rssi"], m["rssi_exact"])
        if c["off"] is not None and c["sent"] is not None and c["snr"] >= 10.0 and -12 <= c["off"] <= 16:
            assert np.array_equal(bits[b], K.hard(c["sent"])), (b, c["off"], c["snr"])
    assert 100 * left_out <= len(cases), left_out
    return left_out


OFFSETS = list(range(-24, 25))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 130])
def test_traffic_slots_equal_model(trx, n):
    rng = np.random.default_rng(1000 + n)
    offs = OFFSETS if n > 9 else [int(o) for o in rng.choice(OFFSETS, n)]
    cases = _traffic(rng, n, offs)
    rec, bits = _run(trx, cases)
    _check(rec, bits, cases)
    assert (rec["kind"] == trxhip.MS_KIND_NB).all() and (rec["sent"] == 1).all()
    if n == 130:
        assert (rec["flags"] == trxhip.MS_IND_SILENT).sum() == 10 and rec["start"].min() < 0 < rec["start"].max()


def _sch_case(rng, active, off=None, snr=25.0):
    bsic, fn = int(rng.integers(0, 64)), int(synth.random_sch_frames(1, rng)[0])
    off = int(rng.integers(0, 40)) if off is None else off
    return _case(K.sch_slot(rng, bsic, fn, off, snr), fn, 0, int(rng.integers(0, 256)), active=active, sent=(bsic, fn))


def _nb_case(rng, active, fn=None, tn=None):
    tsc, off = int(rng.integers(0, 8)), int(rng.integers(-12, 17))
    y, bits = K.nb_slot(rng, tsc, off, 20.0)
    return _case(y, int(rng.integers(0, 2715648)) if fn is None else fn, int(rng.integers(1, 8)) if tn is None else tn, tsc,
                 active=active, sent=bits if active else None, off=off, snr=20.0)


def test_kinds_within_a_wave(trx):
    """Each of SCH / traffic / FCCH / inactive traffic once in every position of a wave's four rows (a Latin square over four
    waves), a wave of four SCH slots, a wave of four traffic slots (no channel decoder runs there) and BAD slots."""
    import torch
    rng = np.random.default_rng(1100)
    cases = []
    for w in range(4):
        for p in range(4):
            k = (p + w) % 4
            if k == 0:
                cases.append(_sch_case(rng, active=bool(w & 1)))
            elif k == 1:
                cases.append(_nb_case(rng, True))
            elif k == 2:
                c = _nb_case(rng, bool(p & 1), fn=51 * int(rng.integers(0, 1000)) + 10 * int(rng.integers(0, 5)), tn=0)   # FCCH
                c["sent"] = None
                cases.append(c)
            else:
                cases.append(_nb_case(rng, False))
    cases += [_sch_case(rng, active=bool(p & 1), snr=(25.0, 10.0, 0.0, 25.0)[p]) for p in range(4)]
    cases += [_nb_case(rng, True) for _ in range(4)]
    bad = [_nb_case(rng, True, tn=8), _nb_case(rng, True), _nb_case(rng, True, tn=255)]
    bad[1]["tsc"] = 8
    for c in bad:
        c["sent"] = None
    cases += bad
    rec, bits = _run(trx, cases)
    _check(rec, bits, cases)
    want = [(k + w) % 4 for w in range(4) for k in range(4)]
    names = [trxhip.MS_KIND_SCH, trxhip.MS_KIND_NB, trxhip.MS_KIND_FCCH, trxhip.MS_KIND_NB]
    assert list(rec["kind"][:16]) == [names[k] for k in want]
    assert list(rec["kind"][16:]) == [trxhip.MS_KIND_SCH] * 4 + [trxhip.MS_KIND_NB] * 4 + [trxhip.MS_KIND_BAD] * 3
    assert not rec["sent"][24:].any() and not bits[24:].any() and (rec["sch_fn"][24:] == -1).all()
    # the SCH rows are the SCH receiver's, ACTIVE or not
    idx = [b for b, c in enumerate(cases) if rec[b]["kind"] == trxhip.MS_KIND_SCH]
    assert len(idx) == 8
    x = torch.from_numpy(np.stack([cases[b]["y"] for b in idx])).to("cuda:0")
    ref, rbits = trx.sch_sync(x, trxhip.SCH_SYNC_TRACK, scale=float(np.float32(1.0) / np.float32(FULL)), want_bits=True)
    for k, b in enumerate(idx):
        got = rec[b]
        assert (got["start"], got["sch_rc"], got["sch_fn"], got["sch_bsic"]) == (ref[k]["start"], ref[k]["rc"], ref[k]["fn"], ref[k]["bsic"])
        assert _f32_bits(got["corr_max"]) == _f32_bits(ref[k]["corr_max"]) and np.array_equal(bits[b], rbits[k])
        assert (got["sent"], got["rssi"], got["toa256"], got["pow"]) == (int(cases[b]["active"]), 10, 0, 0)
        if k < 5 or k == 7:                                        # every SCH slot but the two at 10 and 0 dB
            assert (got["sch_rc"], got["sch_bsic"], got["sch_fn"]) == (1,) + cases[b]["sent"], b
    # FCCH: an indication without content where trxcon listens
    for b in range(16):
        if rec[b]["kind"] == trxhip.MS_KIND_FCCH:
            assert rec[b]["flags"] == (trxhip.MS_IND_TRASH if cases[b]["active"] else 0) and rec[b]["sent"] == int(cases[b]["active"])


@pytest.mark.parametrize("stride", [625, 700])
def test_stride_guard_and_entry_points(trx, stride):
    """A stride above 625 never reads the gap; the int16 entry equals the complex64 entry on the same integer-valued samples; a
    NULL d_bits gives the same records; a slot's result does not depend on where in the batch it lies."""
    rng = np.random.default_rng(1200 + stride)
    n = 11
    cases = _traffic(rng, n, [-20, -3, 0, 9, 24])
    cases[4] = _sch_case(rng, True)
    probe = _nb_case(rng, True)
    for k in (0, 3, n - 1):
        cases[k] = probe
    for c in cases:                                                # integer-valued samples: what the int16 entry sees
        q = K.to_i16(c["y"])
        c["y"] = (q[..., 0].astype(np.float32) + 1j * q[..., 1].astype(np.float32)).astype(np.complex64)
    rf, bf = _run(trx, cases, stride=stride)
    ri, bi = _run(trx, cases, stride=stride, i16=True)
    _check(rf, bf, cases)
    _check(ri, bi, cases, i16=True)
    assert ri.tobytes() == rf.tobytes() and np.array_equal(bi, bf)
    r0, none = _run(trx, cases, stride=stride, i16=True, want_bits=False)
    assert none is None and r0.tobytes() == ri.tobytes()
    for k in (3, n - 1):
        assert ri[k].tobytes() == ri[0].tobytes() and np.array_equal(bi[k], bi[0])
    assert np.array_equal(bi[0], K.hard(probe["sent"])) and ri[4]["sch_rc"] == 1


def test_another_full_scale(trx):
    rng = np.random.default_rng(1300)
    cases = _traffic(rng, 9, [-7, 0, 5, 16])
    rec, bits = _run(trx, cases, full=32767.0, i16=True)
    _check(rec, bits, cases, full=32767.0, i16=True)


def test_one_multiframe_of_a_cell(trx):
    """The 408 slots of one 51-multiframe as a stream cut at 625: SCH bursts of the cell, normal bursts through the product's own
    modulator (int16 rows), FCCH slots holding anything."""
    import torch
    rng = np.random.default_rng(1400)
    bsic, tsc, base = 0o52, 5, 51 * 4321
    fns = np.repeat(np.arange(base, base + 51), 8)
    tns = np.tile(np.arange(8), 51)
    kinds = np.array([trxhip.ms_slot_kind(int(f), int(t)) for f, t in zip(fns, tns)])
    sent = np.stack([synth.sch_burst_bits(bsic, int(f)) if k == trxhip.MS_KIND_SCH else K.nb_bits(rng, tsc) for f, k in zip(fns, kinds)])
    p = np.zeros(408, dtype=trxhip.TX_PARAMS_DTYPE)
    p["nbits"], p["guard"], p["scale_re"] = 148, 8, 1.0
    _, iq, _ = trx.modulate(torch.from_numpy(sent).to("cuda:0"), trx.tx_params_tensor(p), sps=4, cf32=False, s16_scale=1400.0)
    slots = np.zeros(408, dtype=trxhip.MS_SLOT_DTYPE)
    slots["fn"], slots["tn"], slots["tsc"], slots["flags"] = fns, tns, tsc, ACTIVE
    rec, bits = trx.ms_rx(iq, trx.ms_slots_tensor(slots), rx_full_scale=FULL)
    assert np.array_equal(rec["kind"], kinds) and (kinds == trxhip.MS_KIND_SCH).sum() == 5 == (kinds == trxhip.MS_KIND_FCCH).sum()
    assert np.array_equal(rec["fn"], fns) and np.array_equal(rec["tn"], tns) and (rec["sent"] == 1).all()
    sch, nb, fcch = (kinds == k for k in (trxhip.MS_KIND_SCH, trxhip.MS_KIND_NB, trxhip.MS_KIND_FCCH))
    assert (rec["sch_rc"][sch] == 1).all() and np.array_equal(rec["sch_fn"][sch], fns[sch]) and (rec["sch_bsic"][sch] == bsic).all()
    assert (rec["sch_fn"][~sch] == -1).all() and not rec["sch_rc"][~sch].any()
    assert np.array_equal(bits[nb | sch], K.hard(sent[nb | sch]))
    assert (rec["flags"][fcch] == trxhip.MS_IND_TRASH).all() and not bits[fcch].any() and not rec["flags"][~fcch].any()
    # 20 log10(2047 / (1400 / 2047)) = 69.5: the level of the scaled samples under the reference's rxFullScale (ms_upper.cpp:272);
    # the burst lies at the slot's start, within one 20-sample energy window of it
    assert (rec["rssi"][nb] == 69).all() and (rec["rssi"][sch] == 10).all() and (np.abs(rec["start"][nb | sch]) < 20).all()
    # and a few of its slots against the model
    q = iq.cpu().numpy()
    for b in (0, 8, 9, 15, 88, 407):
        m = M.ms_rx(q[b], int(fns[b]), int(tns[b]), tsc, True, FULL)
        assert (rec[b]["kind"], rec[b]["start"], rec[b]["rssi"]) == (m["kind"], m["start"], m["rssi"]), b
        assert _f32_bits(rec[b]["pow"]) == _f32_bits(m["pow"]) and np.array_equal(bits[b], m["bits"]), b


def test_refusals_leave_the_outputs_untouched(trx):
    import torch
    L = trx.L
    x = torch.zeros((2, 700), dtype=torch.complex64, device="cuda:0")
    xi = torch.zeros((2, 700, 2), dtype=torch.int16, device="cuda:0")
    slots = trx.ms_slots_tensor(np.array([(5, 1, 0, ACTIVE, 0), (1, 0, 0, ACTIVE, 0)], dtype=trxhip.MS_SLOT_DTYPE))
    ind = torch.full((2, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    bits = torch.full((2, 148), 0x5A, dtype=torch.int8, device="cuda:0")
    vp = C.c_void_p
    st = trx._stream()
    P = lambda t: vp(t.data_ptr())                                 # noqa: E731
    for fn, xin in ((L.trxhip_ms_rx_batch_cf32, x), (L.trxhip_ms_rx_batch_i16, xi)):
        calls = [
            (vp(0), P(xin), 700, P(slots), P(ind), P(bits), 2, FULL, st),      # NULL pointers
            (trx.h, vp(0), 700, P(slots), P(ind), P(bits), 2, FULL, st),
            (trx.h, P(xin), 700, vp(0), P(ind), P(bits), 2, FULL, st),
            (trx.h, P(xin), 700, P(slots), vp(0), P(bits), 2, FULL, st),
            (trx.h, P(xin), 700, P(slots), P(ind), P(bits), 0, FULL, st),      # n_slots == 0
            (trx.h, P(xin), 624, P(slots), P(ind), P(bits), 2, FULL, st),      # slot_stride < 625
            (trx.h, P(xin), 0, P(slots), P(ind), P(bits), 2, FULL, st),
            (trx.h, P(xin), 700, P(slots), P(ind), P(bits), 2, 0.0, st),       # rx_full_scale not finite or <= 0
            (trx.h, P(xin), 700, P(slots), P(ind), P(bits), 2, -2047.0, st),
            (trx.h, P(xin), 700, P(slots), P(ind), P(bits), 2, float("inf"), st),
            (trx.h, P(xin), 700, P(slots), P(ind), P(bits), 2, float("nan"), st),
        ]
        for a in calls:
            assert fn(*a) == EINVAL, a[2:8]
    torch.cuda.synchronize()
    assert (ind.cpu().numpy() == 0xAB).all() and (bits.cpu().numpy() == 0x5A).all()
    # what is accepted writes every record and every bit
    assert L.trxhip_ms_rx_batch_i16(trx.h, P(xi), 700, P(slots), P(ind), P(bits), 2, FULL, st) == 0
    torch.cuda.synchronize()
    rec = ind.cpu().numpy().reshape(-1).view(trxhip.MS_IND_DTYPE)
    assert list(rec["kind"]) == [trxhip.MS_KIND_NB, trxhip.MS_KIND_SCH] and list(rec["flags"]) == [trxhip.MS_IND_SILENT, 0]
    assert (bits.cpu().numpy() != 0x5A).all()
