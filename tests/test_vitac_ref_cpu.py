"""The restatements of gr-gsm's MLSE receiver against the reference's own compiled code (Transceiver52M/grgsm_vitac/grgsm_vitac.cpp +
viterbi_detector.cc, unmodified: oracle/_ref/libref_vitac.so): the C oracle's orc_demod_any_burst_va, tests/sch_sync_model.py and
tests/ms_rx_model.py, and the training-sequence literals of the kernels.  Everything is equality: burst start, the 20 CIR taps
and corr_max bit for bit, every +-127 output.

The stored records (tests/golden/ref_vitac_vectors.npz, written by tests/golden/make_vitac_vectors.py) are checked everywhere;
where the compiled reference is present the same comparisons run on freshly seeded inputs.

TSC 1 is a deliberate deviation: row 1 of the reference's grgsm_vitac/constants.h has bit 20 inverted against 3GPP TS 45.002
5.2.3 (and against the reference's own transmit table in sigProcLib.cpp), so the reference correlates TSC 1 bursts with one of
16 taps negated.  The project uses the 3GPP row; it is pinned to the compiled get_chan_imp_resp + detect_burst_nb fed the
compiled gmsk_mapper's mapping of the 3GPP string (the tsc1b_* records)."""
import os
import re

import numpy as np
import pytest

import ms_rx_model as MR
import oracle_lib as O
import sch_sync_model as M
import vitac_cases as V

ROOT = O.ROOT
CSRC = os.path.join(ROOT, "osmo_trx_amd", "csrc")


@pytest.fixture(scope="module")
def vec(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ref_vitac_vectors.npz")))


def _same_f32(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def _sbits(out):
    return np.where(out > 0, -127, 127).astype(np.int8)                # "pre flip bits!" (grgsm_vitac.cpp:101-102)


# ---- the comparisons, on any set of records ----------------------------------------------------------------------------------------
def check_oracle_normal(iq, tsc, start, out):
    """orc_demod_any_burst_va, normal bursts: the start after max(.., 0) and every output (the oracle's are the sbits times -1,
    Transceiver.cpp:638, with 8 zeros behind)."""
    for b in range(len(iq)):
        st, soft = O.demod_any_burst_va(V.to_cf(iq[b]), O.TSC, int(tsc[b]), 3)
        assert st == max(int(start[b]), 0), (b, st, start[b])
        assert np.array_equal(soft[:148], -out[b].astype(np.float32)) and not soft[148:].any(), b


def check_oracle_access(iq, ss, start, out):
    for b in range(len(iq)):
        st, soft = O.demod_any_burst_va(V.to_cf(iq[b]), O.RACH if b % 2 else O.EXT_RACH, 0, int(ss[b]))
        assert st == max(int(start[b]), 0), (b, st, start[b])
        assert np.array_equal(soft[:88], -out[b][:88].astype(np.float32)) and not soft[88:].any(), b


def check_model_normal(iq, tsc, scale, ms, start, cir, corr_max, out):
    """sch_sync_model.get_chan_imp_resp + detect_burst over get_norm_chan_imp_resp's window."""
    for b in range(len(iq)):
        x = V.to_x(iq[b], scale)
        pos, c, cm = M.get_chan_imp_resp(x, V.NB_SEARCH[0], V.NB_SEARCH[1], M.norm_seq(V.tsc_bits(int(tsc[b]))))
        st = pos - V.TRAIN_POS * 4
        assert st == start[b], (b, st, start[b])
        assert c.tobytes() == cir[b].tobytes(), b
        assert _same_f32(cm, corr_max[b]), (b, cm, corr_max[b])
        o = M.detect_burst(x, c, V.clamp_ms(st) if ms else max(st, 0))
        assert np.array_equal(_sbits(o), out[b]), b


def check_ms_rx(iq, tsc, start, corr_max, out):
    """ms_rx_model.ms_rx on traffic slots (fn, tn, tsc, ACTIVE)."""
    for b in range(len(iq)):
        r = MR.ms_rx(iq[b], 2 + 51 * b, 1 + b % 7, int(tsc[b]), True, V.MS_FULL_SCALE)
        assert r["kind"] == MR.KIND_NB and r["sent"] == 1
        assert r["start"] == V.clamp_ms(start[b]), (b, r["start"], start[b])
        assert _same_f32(r["corr_max"], corr_max[b]), b
        assert np.array_equal(r["bits"], out[b]), b


def check_sch(iq, mode, start, cir, corr_max, out):
    """sch_sync_model.sch_sync; in TRACK mode also ms_rx_model.ms_rx on the slot as an SCH slot, and the model's taps."""
    c0 = M.SYNC_POS + M.TRAIN_BEGINNING
    for b in range(len(iq)):
        want = V.clamp_ms(start[b]) if mode == M.TRACK else int(start[b])
        r = M.sch_sync(iq[b], mode, V.SCALE_MS)
        assert r["start"] == want, (b, r["start"], start[b])
        assert _same_f32(r["corr_max"], corr_max[b]), b
        assert np.array_equal(r["bits"], out[b]), b
        x = V.to_x(iq[b], V.SCALE_MS)
        lo, hi = ((c0 - 10) * 4, (c0 + M.SYNC_SEARCH_RANGE) * 4) if mode == M.TRACK else (0, len(x) - 64 * 8)
        pos, c, _ = M.get_chan_imp_resp(x, lo, hi, M.sch_seq())
        assert pos - c0 * 4 == start[b] and c.tobytes() == cir[b].tobytes(), b
        if mode == M.TRACK:
            r = MR.ms_rx(iq[b], 1 + 51 * b, 0, 0, True, V.MS_FULL_SCALE)
            assert r["kind"] == MR.KIND_SCH and r["start"] == want and _same_f32(r["corr_max"], corr_max[b]), b
            assert np.array_equal(r["bits"], out[b]), b
            assert (r["sch_rc"], r["sch_fn"], r["sch_bsic"]) == tuple(M.decode_sch(out[b])[k] for k in ("rc", "fn", "bsic")), b


# ---- against the stored records: never skipped ---------------------------------------------------------------------------------
def test_fixture_holds_what_its_generator_promises(vec):
    v = vec
    assert v["nb_iq"].shape == (64, 625, 2) and v["nb_iq"].dtype == np.int16
    assert all((v["nb_tsc"] == t).sum() == 8 and (v["nb_kind"][v["nb_tsc"] == t] == 0).sum() == 2 for t in range(8))
    assert (v["nb_ms_start"] < 0).sum() >= 8 and (v["nb_bts_start"] < 0).sum() >= 8
    assert v["ab_iq"].shape == (24, 625, 2) and set(v["ab_ss"]) == set(V.AB_START_STATES)
    assert v["sch_iq"].shape == (16, 625, 2) and v["sch_start"].min() < -39 and v["sch_start"].max() > 39
    assert v["acq_iq"].shape == (2, V.ACQ_LEN, 2)
    assert np.array_equal(v["tsc1b_rows"], np.flatnonzero(v["nb_tsc"] == 1))
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "ref_vitac_vectors.npz")) <= 400 * 1000


def test_oracle_equals_compiled_reference_normal_bursts(vec):
    start, _, _, out = V.expected_nb(vec, "bts")
    check_oracle_normal(vec["nb_iq"], vec["nb_tsc"], start, out)
    check_oracle_normal(vec["tie_iq"], vec["tie_tsc"], vec["tie_bts_start"], vec["tie_bts_out"])


def test_oracle_equals_compiled_reference_access_bursts(vec):
    check_oracle_access(vec["ab_iq"], vec["ab_ss"], vec["ab_start"], vec["ab_out"])
    check_oracle_access(vec["tie_iq"], np.full(3, 3), vec["tie_ab_start"], vec["tie_ab_out"])


@pytest.mark.parametrize("side", ["bts", "ms"])
def test_model_equals_compiled_reference_normal_bursts(vec, side):
    scale, ms = (V.SCALE_BTS, False) if side == "bts" else (V.SCALE_MS, True)
    check_model_normal(vec["nb_iq"], vec["nb_tsc"], scale, ms, *V.expected_nb(vec, side))
    check_model_normal(vec["tie_iq"], vec["tie_tsc"], scale, ms, *(vec[f"tie_{side}_{k}"] for k in ("start", "cir", "corr_max", "out")))


def test_ms_rx_model_equals_compiled_reference(vec):
    start, _, corr_max, out = V.expected_nb(vec, "ms")
    check_ms_rx(vec["nb_iq"], vec["nb_tsc"], start, corr_max, out)
    check_ms_rx(vec["tie_iq"], vec["tie_tsc"], vec["tie_ms_start"], vec["tie_ms_corr_max"], vec["tie_ms_out"])


def test_sch_sync_model_equals_compiled_reference(vec):
    whole = np.flatnonzero((vec["sch_sent"][:, 0] >= 0) & (vec["sch_off"] >= -12) & (vec["sch_off"] <= 25))
    assert len(whole) >= 2                                             # coded bursts that lie whole in the slot: the record decodes
    for b in whole:
        d = M.decode_sch(vec["sch_out"][b])
        assert (d["rc"], d["bsic"], d["fn"]) == (1, vec["sch_sent"][b, 0], vec["sch_sent"][b, 1]), b
    check_sch(vec["sch_iq"], M.TRACK, *(vec[f"sch_{k}"] for k in ("start", "cir", "corr_max", "out")))
    check_sch(vec["tie_iq"], M.TRACK, *(vec[f"tie_sch_{k}"] for k in ("start", "cir", "corr_max", "out")))
    check_sch(vec["acq_iq"], M.ACQ, *(vec[f"acq_{k}"] for k in ("start", "cir", "corr_max", "out")))


def test_tsc1_as_the_reference_ships_it_differs_from_the_3gpp_row(vec):
    """If the reference's table is ever corrected (the fixture regenerated), or the project's row drifts, this fires."""
    rows = vec["tsc1b_rows"]
    for side in ("bts", "ms"):
        differs = [(vec[f"nb_{side}_start"][r] != vec[f"tsc1b_{side}_start"][k]) or not np.array_equal(vec[f"nb_{side}_out"][r], vec[f"tsc1b_{side}_out"][k])
                   or vec[f"nb_{side}_cir"][r].tobytes() != vec[f"tsc1b_{side}_cir"][k].tobytes() for k, r in enumerate(rows)]
        assert any(differs), side
    a, b, n, d_start, d_out, bursts = (int(x) for x in vec["tsc1_bit_errors"])         # the generator's measurement of the cost
    assert n == 148 * bursts and b <= a and d_start > 0
    # the reference's mapped row differs from the 3GPP one from element 20 on (a differential walk), the product uses 5 .. 20
    ref1, our1 = vec["seq_norm"][1], vec["seq_norm1_3gpp"]
    assert np.array_equal(ref1[:20], our1[:20]) and ref1[20] == -our1[20]


def _define(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+0x([0-9a-fA-F]+)ull\s*$", text, re.M)
    assert m, name
    return int(m.group(1), 16)


def test_training_sequence_literals_equal_the_compiled_mapper(vec):
    """VA_TSC_CODES0 .. 7 / VA_ACC_CODES (trx_va_common.h) and SS_SCH_CODES_LO / _HI (trx_sch_common.h, trx_sch_sync.hip) are the
    quarter-turn codes of what the compiled gmsk_mapper made of the reference's tables, row 1 of the 3GPP string."""
    va = open(os.path.join(CSRC, "trx_va_common.h")).read()
    for t in range(8):
        seq = vec["seq_norm1_3gpp"] if t == 1 else vec["seq_norm"][t]
        assert _define(va, f"VA_TSC_CODES{t}") == M.quarter_codes(seq[5:21]), t
        assert np.array_equal(M.norm_seq(V.tsc_bits(t)), seq[5:21]), t
    assert _define(va, "VA_TSC_CODES1") != M.quarter_codes(vec["seq_norm"][1][5:21])
    assert _define(va, "VA_ACC_CODES") == M.quarter_codes(vec["seq_acc"][5:36])
    assert np.array_equal(M.acc_seq(), vec["seq_acc"][5:36]) and np.array_equal(M.sch_seq(), vec["seq_sch"][5:59])
    sch = M.quarter_codes(vec["seq_sch"][5:59])
    for name in ("trx_sch_common.h", "trx_sch_sync.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert _define(txt, "SS_SCH_CODES_LO") == sch & ((1 << 64) - 1), name
        assert _define(txt, "SS_SCH_CODES_HI") == sch >> 64, name


# ---- against the live library ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not O.ref_vitac_available(), reason="oracle/_ref/libref_vitac.so not built (no reference at build time)")
def test_restatements_equal_the_live_compiled_reference(vec):
    """The same comparisons on about 400 freshly seeded inputs, the buffer search included; and the stored records are what the
    library returns today."""
    R = O.ref_vitac()
    rng = np.random.default_rng(0xBEEF)
    seq1 = V.ref_tsc1_3gpp_seq(R)

    def nb_rec(iq, tsc, scale, ms):
        return V.records(lambda x, t: V.ref_normal(R, x, int(t), scale, ms, seq=seq1 if t == 1 else None), zip(iq, tsc))

    for early in ((), V.NB_EARLY, (-20, -3, 2, 5, 11, 17)):                                   # 3 x 64 normal slots
        nb = V.normal_slots(rng, early=early)
        start, cir, cm, out = nb_rec(nb["iq"], nb["tsc"], V.SCALE_BTS, False)
        check_oracle_normal(nb["iq"], nb["tsc"], start, out)
        check_model_normal(nb["iq"], nb["tsc"], V.SCALE_BTS, False, start, cir, cm, out)
        start, cir, cm, out = nb_rec(nb["iq"], nb["tsc"], V.SCALE_MS, True)
        check_model_normal(nb["iq"][::4], nb["tsc"][::4], V.SCALE_MS, True, start[::4], cir[::4], cm[::4], out[::4])
        check_ms_rx(nb["iq"], nb["tsc"], start, cm, out)
    ab = V.access_slots(rng, 96)
    check_oracle_access(ab["iq"], ab["ss"], *[a for k, a in enumerate(V.records(lambda x, s: V.ref_access(R, x, s), zip(ab["iq"], ab["ss"])))
                                              if k in (0, 3)])
    for _ in range(6):                                                                        # 6 x 16 SCH slots
        sch = V.sch_slots(rng, plain=rng.integers(0, 101, 10), coded=rng.integers(-40, 40, 4))
        check_sch(sch["iq"], M.TRACK, *V.records(lambda x: V.ref_sch_track(R, x), [(x,) for x in sch["iq"]]))
    for length in (V.ACQ_LEN, V.ACQ_LEN + 1, 1250, 2600):
        acq = V.acq_buffers(rng, 4, length)
        check_sch(acq, M.ACQ, *V.records(lambda x: V.ref_sch_acq(R, x), [(x,) for x in acq]))

    # the stored records against the library as it is built today
    for side, scale, ms in (("bts", V.SCALE_BTS, False), ("ms", V.SCALE_MS, True)):
        got = V.records(lambda x, t: V.ref_normal(R, x, int(t), scale, ms), zip(vec["nb_iq"], vec["nb_tsc"]))
        for g, k in zip(got, ("start", "cir", "corr_max", "out")):
            assert g.tobytes() == vec[f"nb_{side}_{k}"].tobytes(), (side, k)
    norm, acc, sch_seq = R.training_seqs()
    assert np.array_equal(norm, vec["seq_norm"]) and np.array_equal(acc, vec["seq_acc"]) and np.array_equal(sch_seq, vec["seq_sch"])
