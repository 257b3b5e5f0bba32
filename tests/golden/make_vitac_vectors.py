#!/usr/bin/env python3
"""tests/golden/ref_vitac_vectors.npz -- the MLSE receivers' inputs and what the reference's own compiled code returns for them.

Run in the build container only (needs the reference for oracle/_ref/libref_vitac.so: grgsm_vitac.cpp + viterbi_detector.cc
compiled where they lie, oracle/Makefile; the output is committed data).  Seeded: a second run writes the same arrays.
The case builders and the calls are tests/vitac_cases.py.  Inputs are int16 IQ; every record is (raw start, 20 CIR taps,
corr_max, sbits) of the compiled functions on x.astype(float32) * scale:

  nb_*      64 slots, 8 per TSC (2 noise-only, 6 bursts): get_norm_chan_imp_resp + detect_burst_nb(.., 3)
              nb_bts_*  at 1 / 16383, burst start max(start, 0)          (Transceiver.cpp:620-645, :783)
              nb_ms_*   at 1 / 2047,  burst start clamped to [-39, 39]   (ms_upper.cpp:203-230)
            The TSC 1 rows are the reference as it ships: row 1 of grgsm_vitac/constants.h has bit 20 inverted against
            3GPP TS 45.002 and the reference's own transmit table.
  tsc1b_*   the TSC 1 rows again (nb_*[tsc1b_rows]) with the compiled get_chan_imp_resp + detect_burst_nb fed the compiled
            gmsk_mapper's mapping of the 3GPP bit string, conjugated, elements 5 .. 20, over get_norm_chan_imp_resp's window:
            what the product computes at TSC 1.  tsc1_bit_errors: what the reference's row costs, measured on 200 further
            seeded TSC 1 bursts that are not stored (vitac_cases.tsc1_cost): wrong hard bits as shipped, wrong hard bits with the
            3GPP row, bits sent, bursts whose start differs, bursts whose sbits differ, bursts.
  ab_*      24 slots: get_access_imp_resp(.., 0) + max(start, 0) + detect_burst_ab(.., ab_ss), ab_ss in {0, 3, 12, 15}; 88 sbits
  sch_*     16 slots: get_sch_chan_imp_resp + clamp + detect_burst_nb at 1 / 2047 (ms_rx_lower.cpp:171-177); sch_sent: the BSIC
            and frame number the coded bursts carry
  acq_*     2 buffers of 532 samples: get_sch_buffer_chan_imp_resp + detect_burst_nb at 1 / 2047
  tie_*     3 slots whose window energies tie exactly at the maximum (all zero, single impulses): std::max_element's pick.
            tie_bts_* / tie_ms_* as nb_*, tie_ab_* as ab_* with start state 3, tie_sch_* as sch_*
  seq_*     d_norm_training_seq[0..8], d_acc_training_seq, d_sch_training_seq after initvita(); seq_norm1_3gpp: the 26 mapped,
            conjugated elements of the 3GPP TSC 1 string

Consumers: tests/test_vitac_ref_cpu.py (the oracle and the Python models) and tests/test_gpu_vitac_ref.py (the kernels)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O                                   # noqa: E402
import vitac_cases as V                                  # noqa: E402

OUT = os.path.join(HERE, "ref_vitac_vectors.npz")
MAX_BYTES = 400 * 1000


def build_arrays():
    O.build()
    R = O.ref_vitac()
    out = {}

    nb = V.normal_slots(np.random.default_rng(0x71AC0), early=V.NB_EARLY)
    assert len(nb["iq"]) == 64 and all((nb["tsc"] == t).sum() == 8 for t in range(8))
    out.update(nb_iq=nb["iq"], nb_tsc=nb["tsc"], nb_kind=nb["kind"], nb_delay=nb["delay"], nb_bits=nb["bits"])
    for side, scale, ms in (("bts", V.SCALE_BTS, False), ("ms", V.SCALE_MS, True)):
        st, cir, cm, sb = V.records(lambda iq, t: V.ref_normal(R, iq, int(t), scale, ms), zip(nb["iq"], nb["tsc"]))
        out.update({f"nb_{side}_start": st, f"nb_{side}_cir": cir, f"nb_{side}_corr_max": cm, f"nb_{side}_out": sb})
    assert (out["nb_ms_start"] < 0).sum() >= 8, "the MS path needs raw starts below 0"
    assert out["nb_ms_start"].min() >= -39 and out["nb_ms_start"].max() <= 39      # the search window lies inside the clamp

    rows = np.flatnonzero(nb["tsc"] == 1)
    seq = V.ref_tsc1_3gpp_seq(R)
    out["tsc1b_rows"] = rows.astype(np.int32)
    for side, scale, ms in (("bts", V.SCALE_BTS, False), ("ms", V.SCALE_MS, True)):
        st, cir, cm, sb = V.records(lambda iq: V.ref_normal(R, iq, 1, scale, ms, seq=seq), [(nb["iq"][r],) for r in rows])
        out.update({f"tsc1b_{side}_start": st, f"tsc1b_{side}_cir": cir, f"tsc1b_{side}_corr_max": cm, f"tsc1b_{side}_out": sb})
    out["tsc1_bit_errors"] = V.tsc1_cost(R, np.random.default_rng(0x71AC4), 200)

    ab = V.access_slots(np.random.default_rng(0x71AC1), 24)
    st, cir, cm, sb = V.records(lambda iq, ss: V.ref_access(R, iq, ss), zip(ab["iq"], ab["ss"]))
    out.update(ab_iq=ab["iq"], ab_ss=ab["ss"], ab_start=st, ab_cir=cir, ab_corr_max=cm, ab_out=sb)

    sch = V.sch_slots(np.random.default_rng(0x71AC2))
    assert len(sch["iq"]) == 16
    st, cir, cm, sb = V.records(lambda iq: V.ref_sch_track(R, iq), [(x,) for x in sch["iq"]])
    out.update(sch_iq=sch["iq"], sch_off=sch["off"], sch_sent=sch["sent"], sch_start=st, sch_cir=cir, sch_corr_max=cm, sch_out=sb)
    assert st.min() < -39 < 39 < st.max(), "both ends of the clamp"

    acq = V.acq_buffers(np.random.default_rng(0x71AC3), 2)
    st, cir, cm, sb = V.records(lambda iq: V.ref_sch_acq(R, iq), [(x,) for x in acq])
    out.update(acq_iq=acq, acq_start=st, acq_cir=cir, acq_corr_max=cm, acq_out=sb)

    tie = V.tie_slots()
    out.update(tie_iq=tie["iq"], tie_tsc=tie["tsc"])
    for side, fn in (("bts", lambda iq, t: V.ref_normal(R, iq, int(t), V.SCALE_BTS, False)),
                     ("ms", lambda iq, t: V.ref_normal(R, iq, int(t), V.SCALE_MS, True)),
                     ("ab", lambda iq, t: V.ref_access(R, iq, 3)), ("sch", lambda iq, t: V.ref_sch_track(R, iq))):
        st, cir, cm, sb = V.records(fn, zip(tie["iq"], tie["tsc"]))
        out.update({f"tie_{side}_start": st, f"tie_{side}_cir": cir, f"tie_{side}_corr_max": cm, f"tie_{side}_out": sb})
    assert out["tie_bts_start"][0] == V.NB_SEARCH[0] - V.TRAIN_POS * 4                # all zero: the first window

    norm, acc, sch_seq = R.training_seqs()
    b = V.tsc_bits(1)
    out.update(seq_norm=norm, seq_acc=acc, seq_sch=sch_seq,
               seq_norm1_3gpp=np.conj(R.gmsk_mapper(b, 1.0 if b[0] == 0 else -1.0)).astype(np.complex64))
    return out


def main():
    out = build_arrays()
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("ref_vitac_vectors.npz:", len(out), "arrays,", size, "bytes")
    print("raw starts below 0 (MS side):", int((out["nb_ms_start"] < 0).sum()), "of", len(out["nb_ms_start"]))
    a, b, n, ds, do, nb = out["tsc1_bit_errors"]
    print(f"TSC 1: {a} wrong hard bits of {n} as the reference ships it, {b} of {n} with the 3GPP row; "
          f"start differs on {ds}, sbits on {do} of {nb} bursts")
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
