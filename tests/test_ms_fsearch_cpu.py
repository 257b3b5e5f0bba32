"""CPU tests of the MS-side FCCH search (include/trxhip.h, "MS-side FCCH search"): the numpy restatement
(tests/ms_fsearch_model.py) on streams from the oracle's modulator -- where it finds the frequency-correction burst, how far its
scores on the burst stand above its scores on everything else (the two figures the default min_score lies between), the rows that
pin the definition's corners --, the header, the exports, and the refusal of plan-only objects."""
import os
import re

import numpy as np
import pytest

import ms_fsearch_cases as FC
import ms_fsearch_model as FM
import osmo_trx_amd
from osmo_trx_amd import trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_SCORE = trxhip.MS_FSEARCH_MIN_SCORE
CFOS = (0.0, 2000.0, -40000.0, 80000.0)
SEEDS = (11, 12)
LEAD = 137


def scan(snr_db, cfo, seed):
    """(hit, distance of pos from the nearest burst's first sample, the largest score more than 700 samples away from every burst,
    the smallest of the bursts' best scores within 32 samples of their first sample) on 12 frames with traffic on every slot"""
    x, starts, _ = FC.cell(seed, snr_db, cfo, 12, LEAD)
    w = FM.windows(x)
    pos = FM.HOP * np.arange(len(w["score"]))
    far = np.ones(len(pos), dtype=bool)
    on = []
    for s in starts:
        far &= np.abs(pos - s) > 700
        on.append(w["score"][np.abs(pos - s) <= 32].max())
    hit = FM.search(x, MIN_SCORE, w)
    return hit, min(abs(int(hit["pos"]) - s) for s in starts), float(w["score"][far].max()), float(min(on))


@pytest.mark.parametrize("snr_db", [25.0, 10.0])
@pytest.mark.parametrize("cfo", CFOS)
def test_burst_is_found_where_it_lies(snr_db, cfo):
    for seed in SEEDS:
        hit, dist, _, _ = scan(snr_db, cfo, seed)
        print(f"snr {snr_db} cfo {cfo} seed {seed}: pos {int(hit['pos'])} score {float(hit['score']):.4f} |pos - start| {dist}")
        assert hit["found"] == 1 and dist <= 32


def test_default_min_score_lies_between_the_two_figures():
    """the figures of DESIGN §4o and of the header: 0.08 and 0.81"""
    off = max(scan(snr, cfo, seed)[2] for snr in (25.0, 10.0) for cfo in CFOS for seed in SEEDS)
    on10 = min(scan(10.0, cfo, seed)[3] for cfo in CFOS for seed in SEEDS)
    on25 = min(scan(25.0, cfo, seed)[3] for cfo in CFOS for seed in SEEDS)
    print(f"largest score more than 700 samples from a burst {off:.4f}; smallest burst score at 10 dB {on10:.4f}, at 25 dB {on25:.4f}")
    assert off < MIN_SCORE < on10
    assert abs(MIN_SCORE - (off + on10) / 2) < 0.01                # midway
    assert round(off, 2) == 0.08 and round(on10, 2) == 0.81 and on25 > 0.98    # as written down
    # the score does not depend on the carrier offset: the same stream at another offset scores the same to rounding of the int16
    a, b = scan(25.0, 0.0, 11)[0], scan(25.0, 80000.0, 11)[0]
    assert a["pos"] == b["pos"] and abs(float(a["score"]) - float(b["score"])) < 1e-3


def test_zero_row():
    for x in (np.zeros((FM.MIN_LEN, 2), np.int16), np.zeros((4000, 2), np.int16), np.zeros(700, np.complex64)):
        hit = FM.search(x, MIN_SCORE)
        assert hit["found"] == 0 and hit["pos"] == 0 and hit["score"] == 0.0 and all(hit[k] == 0 for k in FM.SUMS)


def test_tie_row_takes_the_lowest_pos():
    x = FC.tie_row(5000)
    w = FM.windows(x)
    assert len(set(w["score"].tolist())) == 1 and w["score"][0] > 0.99      # every window the same bits
    hit = FM.search(x, MIN_SCORE, w)
    assert hit["pos"] == 0 and hit["found"] == 1


def test_fragment_at_the_rows_start_is_not_found():
    """a tone that the row's start cuts off after 300 samples: the two halves' product rejects it"""
    x = FC.tone_row(4000, -292)
    hit = FM.search(x, MIN_SCORE)
    print(f"fragment: pos {int(hit['pos'])} score {float(hit['score']):.4f}")
    assert hit["found"] == 0
    whole = FM.search(FC.tone_row(4000, 1000), MIN_SCORE)          # the same tone, whole
    assert whole["found"] == 1 and abs(int(whole["pos"]) - 1000) <= 16


def test_window_counts():
    assert FM.n_windows(584) == 1 and FM.n_windows(599) == 1 and FM.n_windows(600) == 2
    assert FM.n_windows(4096 + 560 + 8 - 1) == FM.SEG - 1 and FM.n_windows(4096 + 560 + 8) == FM.SEG       # a segment one short, full
    assert FM.n_windows(4096 + 560 + 8 + 15) == FM.SEG and FM.n_windows(4096 + 560 + 8 + 16) == FM.SEG + 1  # one segment, two
    assert FM.n_windows(60000) == 3714


def test_measurement_reads_inside_the_window():
    """the estimator's samples pos + 52 .. pos + 175 lie inside the window's 576 + 8 samples"""
    import ms_afc_model as AM
    assert AM.FIRST == 52 and AM.LAST == 175 and AM.LAST < FM.MIN_LEN
    x = FC.tone_row(584, 0)
    hit = FM.search(x, MIN_SCORE)
    assert hit["pos"] == 0 and hit["found"] == 1
    m = FM.measure(x, 0)
    assert abs(float(m["hz"]) - trxhip.MS_FCCH_BIAS_HZ) < 100.0


def test_plain_acquire_finds_nothing_at_2000_hz():
    """the CPU model of the SCH receiver on the cold-start stream of tests/test_gpu_ms_fsearch.py: acquired on frequency, not
    acquired 2000 Hz off -- while the search finds the burst on both and the estimator reads the offset"""
    import ms_sched_cases as SC
    import sch_sync_model as SS
    for cfo, rc in ((0.0, 1), (2000.0, 0)):
        x, starts, _ = FC.cell(7301, 25.0, cfo, 24, 0, 0x0F)
        assert SS.sch_sync(x[:FC.ACQ_LEN], SS.ACQ, SC.SCALE)["rc"] == rc
        hit = FM.search(x[:FC.ACQ_LEN], MIN_SCORE)
        assert hit["found"] == 1 and min(abs(int(hit["pos"]) - s) for s in starts) <= 32
        assert abs(float(FM.measure(x, int(hit["pos"]))["hz"]) - trxhip.MS_FCCH_BIAS_HZ - cfo) <= 100.0


def test_header_exports_and_abi():
    L = trxhip.load_library()
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    for name in ("trxhip_ms_fcch_search_i16", "trxhip_ms_fcch_search_cf32", "trxhip_ms_afc_sched_acquire_s16", "trxhip_ms_afc_sched_acquire_cf32",
                 "trxhip_ms_afc_group_acquire_s16", "trxhip_ms_afc_group_acquire_cf32"):
        assert hasattr(L, name) and name in trxhip.SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
        assert getattr(L, name).argtypes is not None, name
    assert L.trxhip_abi_version() == 5 and re.search(r"^#define\s+TRXHIP_ABI_VERSION\s+5\b", hdr, re.M)
    for name, value in (("HOP", 16), ("W", 576), ("LAG", 8)):
        assert re.search(r"^#define TRXHIP_MS_FSEARCH_%s\s+%d$" % (name, value), hdr, re.M), name
        assert getattr(trxhip, "MS_FSEARCH_" + name) == value == getattr(FM, name)
    m = re.search(r"^#define TRXHIP_MS_FSEARCH_MIN_SCORE\s+([0-9.]+)$", hdr, re.M)
    assert m and float(m.group(1)) == trxhip.MS_FSEARCH_MIN_SCORE and 0.0 < trxhip.MS_FSEARCH_MIN_SCORE <= 1.0
    assert trxhip.MS_FCCH_HIT_DTYPE.itemsize == 64 and trxhip.MS_FCCH_HIT_DTYPE == FM.HIT_DTYPE
    assert re.search(r"typedef struct trxhip_ms_fcch_hit \{\s*/\* 64 bytes \*/", hdr)
    for name in ("MS_FCCH_HIT_DTYPE", "MS_FSEARCH_HOP", "MS_FSEARCH_W", "MS_FSEARCH_LAG", "MS_FSEARCH_MIN_SCORE"):
        assert name in osmo_trx_amd.__all__ and getattr(osmo_trx_amd, name) is getattr(trxhip, name)
    assert hasattr(trxhip.TrxHip, "ms_fcch_search")
    for cls in (trxhip.MsRxScheduler, trxhip.MsRxSchedulerGroup):
        assert hasattr(cls, "acquire_afc")


def test_plan_only_objects_refuse_and_keep_their_state():
    s = trxhip.MsRxScheduler(None, tracking=True)
    s.set_clock(100, 3, 5000)
    s.set_nco(True, 1234.0)
    before = (s.clock(), s.state().tobytes(), s.nco_state(), s.plan().tobytes())
    with pytest.raises(trxhip.TrxHipError, match="-22"):
        s.acquire_afc(first_ts=0)
    assert (s.clock(), s.state().tobytes(), s.nco_state(), s.plan().tobytes()) == before
    g = trxhip.MsRxSchedulerGroup(None, 3)
    g.set_clock(1, 7, 0, 99)
    g.set_nco(2, True, -500.0)
    snap = lambda: [g.clock(1)] + [(g.state(m).tobytes(), g.nco_state(m)) for m in range(3)]
    before = snap()
    with pytest.raises(trxhip.TrxHipError, match="-22"):
        g.acquire_afc([0, 2], first_ts=[0, 5])
    assert snap() == before
    # the plain acquire of a plan-only object is what it was
    rec = np.zeros((), dtype=trxhip.SCH_SYNC_DTYPE)
    rec["rc"], rec["fn"] = 1, 1000
    assert s.acquire(result=rec, first_ts=0)[0] is True
