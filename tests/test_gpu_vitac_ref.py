"""The four MLSE receivers on the GPU (pytest -m gpu) against what the reference's own compiled code returned for the same int16
inputs (tests/golden/ref_vitac_vectors.npz: grgsm_vitac.cpp + viterbi_detector.cc compiled unmodified, written by
tests/golden/make_vitac_vectors.py) -- directly, not through the oracle or the Python models:

  va_demod_kernel         TrxHip.demod_va (trxhip_demod_va_batch_cf32)
  ms_rx_kernel            TrxHip.ms_rx, int16 and complex64
  sch_sync_demod_kernel   TrxHip.sch_sync, TRACK and ACQ
  rx_va_slot_kernel       RxScheduler(use_va=True)

Everything is equality: burst starts, corr_max bit for bit, every +-127 output.  At TSC 1 the kernels use the 3GPP training
sequence, not row 1 of the reference's grgsm_vitac/constants.h (bit 20 inverted): those rows are compared with the tsc1b_* records,
the same compiled functions fed the compiled gmsk_mapper's mapping of the 3GPP string (tests/test_vitac_ref_cpu.py)."""
import os

import numpy as np
import pytest

import oracle_lib as O
import vitac_cases as V
from osmo_trx_amd import trxhip
from osmo_trx_amd.trxhip import PARAMS_DTYPE

pytestmark = pytest.mark.gpu
ACTIVE = trxhip.MS_SLOT_ACTIVE


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


@pytest.fixture(scope="module")
def vec(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ref_vitac_vectors.npz")))


@pytest.fixture(scope="module")
def va_rows(vec):
    """The 64 normal + 24 access + 3 tie slots (as normal bursts) + 3 tie slots (as access bursts) as demod_va takes them:
    (complex64[94, 625], params, start after max(.., 0), soft float32[94, 156])."""
    start, _, _, out = V.expected_nb(vec, "bts")
    n_nb, n_ab, n_tie = len(vec["nb_iq"]), len(vec["ab_iq"]), len(vec["tie_iq"])
    x = V.to_cf(np.concatenate([vec["nb_iq"], vec["ab_iq"], vec["tie_iq"], vec["tie_iq"]]))
    params = np.zeros(len(x), dtype=PARAMS_DTYPE)
    params[:n_nb] = [(O.TSC, t, 3, 0) for t in vec["nb_tsc"]]
    params[n_nb:n_nb + n_ab] = [(O.RACH if b % 2 else O.EXT_RACH, 0, ss, 0) for b, ss in enumerate(vec["ab_ss"])]
    params[n_nb + n_ab:n_nb + n_ab + n_tie] = [(O.TSC, t, 3, 0) for t in vec["tie_tsc"]]
    params[n_nb + n_ab + n_tie:] = (O.RACH, 0, 3, 0)
    starts = np.maximum(np.concatenate([start, vec["ab_start"], vec["tie_bts_start"], vec["tie_ab_start"]]), 0)
    soft = np.zeros((len(x), 156), dtype=np.float32)
    for lo, sb in ((0, out), (n_nb, vec["ab_out"]), (n_nb + n_ab, vec["tie_bts_out"]), (n_nb + n_ab + n_tie, vec["tie_ab_out"])):
        soft[lo:lo + len(sb), :sb.shape[1]] = -sb.astype(np.float32)       # demodAnyBurst_va's "* -1" (Transceiver.cpp:638)
    return x, params, starts.astype(np.int32), soft


def _demod_va(trx, x, params):
    import torch
    soft, starts = trx.demod_va(torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0"), trx.params_tensor(params))
    return soft.cpu().numpy(), starts.cpu().numpy()


def _assert_va(soft, starts, want_soft, want_starts, rows=None):
    rows = np.arange(len(starts)) if rows is None else rows
    assert np.array_equal(starts, want_starts), rows[np.flatnonzero(starts != want_starts)[:10]]
    assert np.array_equal(soft, want_soft), rows[np.flatnonzero((soft != want_soft).any(1))[:10]]


def test_demod_va_equals_compiled_reference(trx, va_rows):
    x, params, starts, soft = va_rows
    got_soft, got_starts = _demod_va(trx, x, params)
    _assert_va(got_soft, got_starts, soft, starts)
    access = params["type"] != O.TSC
    assert access.sum() == 27 and not got_soft[access, 88:].any()
    assert (np.abs(got_soft[~access, :148]) == 127).all() and (np.abs(got_soft[access, :88]) == 127).all()


@pytest.mark.parametrize("batch", [1, 3, 5, 7])
def test_demod_va_tail_batches(trx, va_rows, batch):
    """The kernel runs four bursts per wave: batches that leave idle rows in the last wave, and a single burst."""
    x, params, starts, soft = va_rows
    for lo in range(0, len(x), batch):
        rows = np.arange(lo, min(lo + batch, len(x)))
        got_soft, got_starts = _demod_va(trx, x[rows], params[rows])
        _assert_va(got_soft, got_starts, soft[rows], starts[rows], rows)


def test_demod_va_interleaved_normal_and_access(trx, va_rows):
    """Normal and access rows alternate, so the rows of one wave differ in length (148 / 88 steps of the trellis)."""
    x, params, starts, soft = va_rows
    nb, ab = np.flatnonzero(params["type"] == O.TSC), np.flatnonzero(params["type"] != O.TSC)
    rows = np.concatenate([np.stack([nb[:len(ab)], ab], 1).reshape(-1), nb[len(ab):]])
    assert sorted(rows) == list(range(len(x)))
    got_soft, got_starts = _demod_va(trx, x[rows], params[rows])
    _assert_va(got_soft, got_starts, soft[rows], starts[rows], rows)


@pytest.mark.parametrize("length", [600, 665])
def test_demod_va_row_lengths(trx, va_rows, length):
    """Rows cut to 600 samples or zero-extended to 665.  Samples outside a row read as zero, so a zero-extended row gives the
    625-sample record, and so does a cut row wherever the reference read nothing behind sample 599: the search ends at sample
    363 (normal) / 211 (access), the matched filter reads samples start .. start + 4 * nbits - 1.  The other cut rows are
    compared with the oracle on the cut row."""
    x, params, starts, soft = va_rows
    xl = np.zeros((len(x), length), dtype=np.complex64)
    xl[:, :min(length, 625)] = x[:, :length]
    got_soft, got_starts = _demod_va(trx, xl, params)
    nbits = np.where(params["type"] == O.TSC, 148, 88)
    inside = starts + 4 * nbits <= length
    assert inside[params["type"] != O.TSC].all() and (inside.all() if length == 665 else (~inside).any() and inside[:64].any())
    _assert_va(got_soft[inside], got_starts[inside], soft[inside], starts[inside], np.flatnonzero(inside))
    for b in np.flatnonzero(~inside):
        st, ref = O.demod_any_burst_va(xl[b], int(params["type"][b]), int(params["tsc"][b]), int(params["max_toa"][b]))
        assert got_starts[b] == st and np.array_equal(got_soft[b], ref), b


# ---- the MS side ---------------------------------------------------------------------------------------------------------------
def _ms_rx(trx, iq, slots, cf32):
    import torch
    x = torch.from_numpy(V.to_cf(iq) if cf32 else np.ascontiguousarray(iq)).to("cuda:0")
    return trx.ms_rx(x, slots, rx_full_scale=V.MS_FULL_SCALE)


def _f32_same(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@pytest.mark.parametrize("kind", ["i16", "cf32"])
@pytest.mark.parametrize("batch", [64, 5])
def test_ms_rx_traffic_slots_equal_compiled_reference(trx, vec, kind, batch):
    start, _, corr_max, out = V.expected_nb(vec, "ms")
    iq = np.concatenate([vec["nb_iq"], vec["tie_iq"]])
    tsc = np.concatenate([vec["nb_tsc"], vec["tie_tsc"]])
    start = np.clip(np.concatenate([start, vec["tie_ms_start"]]), -39, 39)
    corr_max, out = np.concatenate([corr_max, vec["tie_ms_corr_max"]]), np.concatenate([out, vec["tie_ms_out"]])
    assert (start < 0).sum() >= 8
    slots = np.zeros(len(iq), dtype=trxhip.MS_SLOT_DTYPE)
    for b in range(len(iq)):
        slots[b] = (2 + 51 * b, 1 + b % 7, tsc[b], ACTIVE, 0)
    for lo in range(0, len(iq), batch):
        hi = min(lo + batch, len(iq))
        rec, bits = _ms_rx(trx, iq[lo:hi], slots[lo:hi], kind == "cf32")
        assert (rec["kind"] == trxhip.MS_KIND_NB).all() and (rec["sent"] == 1).all() and not rec["toa256"].any()
        assert np.array_equal(rec["start"], start[lo:hi]), lo + np.flatnonzero(rec["start"] != start[lo:hi])
        assert _f32_same(rec["corr_max"], corr_max[lo:hi]), lo + np.flatnonzero(rec["corr_max"] != corr_max[lo:hi])
        assert np.array_equal(bits, out[lo:hi]), lo + np.flatnonzero((bits != out[lo:hi]).any(1))


def _sch_records(vec):
    iq = np.concatenate([vec["sch_iq"], vec["tie_iq"]])
    start = np.clip(np.concatenate([vec["sch_start"], vec["tie_sch_start"]]), -39, 39)
    return (iq, start, np.concatenate([vec["sch_corr_max"], vec["tie_sch_corr_max"]]), np.concatenate([vec["sch_out"], vec["tie_sch_out"]]),
            np.concatenate([vec["sch_off"], np.full(3, -1000)]), np.concatenate([vec["sch_sent"], np.full((3, 2), -1)]))


def _whole(off):
    """Coded bursts that lie whole in the slot behind at most the tail bits, inside the clamp, at 10 dB or more: they decode."""
    return (off >= -12) & (off <= 25)


@pytest.mark.parametrize("kind", ["i16", "cf32"])
def test_ms_rx_sch_slots_equal_compiled_reference(trx, vec, kind):
    import sch_sync_model as M
    iq, start, corr_max, out, off, sent = _sch_records(vec)
    slots = np.zeros(len(iq), dtype=trxhip.MS_SLOT_DTYPE)
    for b in range(len(iq)):
        slots[b] = (1 + 10 * (b % 5) + 51 * b, 0, 0, ACTIVE, 0)
    rec, bits = _ms_rx(trx, iq, slots, kind == "cf32")
    assert (rec["kind"] == trxhip.MS_KIND_SCH).all()
    assert np.array_equal(rec["start"], start) and _f32_same(rec["corr_max"], corr_max)
    assert np.array_equal(bits, out), np.flatnonzero((bits != out).any(1))
    coded = np.flatnonzero((sent[:, 0] >= 0) & _whole(off))
    assert len(coded) >= 2
    for b in coded:
        assert (rec["sch_rc"][b], rec["sch_bsic"][b], rec["sch_fn"][b]) == (1, sent[b, 0], sent[b, 1]), b
    for b in range(len(iq)):                                           # decode_sch has no compiled reference: the model's, on the record's bits
        d = M.decode_sch(out[b])
        assert (rec["sch_rc"][b], rec["sch_fn"][b], rec["sch_bsic"][b]) == (d["rc"], d["fn"], d["bsic"]), b


@pytest.mark.parametrize("kind", ["i16", "cf32"])
def test_sch_sync_track_and_acq_equal_compiled_reference(trx, vec, kind):
    import torch
    assert np.float32(1.0 / 2047.0) == V.SCALE_MS

    def run(iq, mode):
        x = torch.from_numpy(V.to_cf(iq) if kind == "cf32" else np.ascontiguousarray(iq)).to("cuda:0")
        return trx.sch_sync(x, mode, scale=1.0 / 2047.0, want_bits=True)

    iq, start, corr_max, out, off, sent = _sch_records(vec)
    rec, bits = run(iq, trxhip.SCH_SYNC_TRACK)
    assert np.array_equal(rec["start"], start), (rec["start"], start)
    assert _f32_same(rec["corr_max"], corr_max)
    assert np.array_equal(bits, out), np.flatnonzero((bits != out).any(1))
    for b in np.flatnonzero((sent[:, 0] >= 0) & _whole(off)):
        assert (rec["rc"][b], rec["bsic"][b], rec["fn"][b]) == (1, sent[b, 0], sent[b, 1]), b
    rec, bits = run(vec["acq_iq"], trxhip.SCH_SYNC_ACQ)
    assert np.array_equal(rec["start"], vec["acq_start"]), (rec["start"], vec["acq_start"])
    assert _f32_same(rec["corr_max"], vec["acq_corr_max"]) and np.array_equal(bits, vec["acq_out"])


# ---- the uplink scheduler's Viterbi flow -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tsc", [3, 1])
def test_rx_scheduler_use_va_equals_compiled_reference(trx, vec, tsc):
    """One pull over a stream made of the 8 fixture slots of one TSC.  The slots are what the radio reads 20 samples early (a burst
    `nb_delay` samples into its slot; the detector looks at the slot from sample 20 on), as tests/test_gpu_rx_sched_va.py lays its
    streams out.  A slot the detector finds is demodulated by rx_va_slot_kernel from the slot as read: its sliced soft row is the
    record's (1.0 where the sbit is -127).  The stream ends with one more sample: the cutter hands a slot on once the sample behind
    it has arrived."""
    import torch
    import rx_sched_model as SM
    import test_gpu_rx_sched_va as T
    rows = np.flatnonzero(vec["nb_tsc"] == tsc)
    assert len(rows) == 8
    _, _, _, out = V.expected_nb(vec, "bts")
    combs, clock = ([1] * 8,), (100, 0)
    model = SM.Model(1, tsc=tsc, ul_fn_offset=-3, ext_rach=True)
    T.configure(model, 1, combs=combs, clock=clock)
    plan = model.cut(8 * 625 + 1)[0]
    assert len(plan) == 8 and all(p[2] == SM.TSC for p in plan)
    s = trxhip.RxScheduler(trx, chans=1, tsc=tsc, ul_fn_offset=-3, ext_rach=True, full_scale=T.FULL, max_slots=64, use_va=True)
    T.configure(s, 1, combs=combs, clock=clock)
    stream = T.dev(np.concatenate([vec["nb_iq"][rows].reshape(1, 8 * 625, 2), np.zeros((1, 1, 2), np.int16)], 1))
    assert s.slots(8 * 625 + 1) == 8
    _, _, ind, soft = s.pull(stream, want_soft=True)
    torch.cuda.synchronize()
    ind, soft = s.ind_to_numpy(ind)[0], soft.cpu().numpy()[0]
    s.close()
    found = ind["rc"] > 0
    # a burst 7 .. 21 samples in lies -3.25 .. +0.25 symbols from where the detector expects it, inside its window: all four
    # cannot be missed unless the detector is broken
    assert found[(vec["nb_kind"][rows] == 1) & (vec["nb_delay"][rows] >= 7)].any()
    want = (out[rows] < 0).astype(np.float32)
    assert np.array_equal(soft[found], want[found]), np.flatnonzero(found)[(soft[found] != want[found]).any(1)]
