"""osmo_trx_amd -- MI355X (gfx950) receive-side burst DSP for osmo-trx.

The product is the HIP library osmo_trx_amd/lib/libtrxhip.so behind the C ABI of include/trxhip.h
(kernels: csrc/trx_kernels.hip, csrc/trx_aux_kernels.hip, csrc/trx_rx_frontend.hip, ...) plus the C++ host shim that keeps the
reference's sigProcLib.h signatures (host/).  This Python package is plumbing only: a ctypes
binding that hands torch device pointers to the C ABI (trxhip.py), the synthetic workload
generator (synth.py), batch sharding + RCCL table broadcast (shard.py) and the build driver
(build.py).  There is no CPU fallback: without the built library or without a GPU every
compute entry point raises.
"""
from .trxhip import (TrxHip, TrxHipError, PARAMS_DTYPE, RESULT_DTYPE, lib_path, load_library,  # noqa: F401
                     OFF, TSC, EXT_RACH, RACH, SCH, EDGE, IDLE,
                     MS_SLOT_DTYPE, MS_IND_DTYPE, MS_KIND_BAD, MS_KIND_FCCH, MS_KIND_SCH, MS_KIND_NB, MS_SLOT_ACTIVE,
                     MS_IND_TRASH, MS_IND_SILENT, ms_slot_kind, MsRxScheduler, MsRxSchedulerGroup, MS_PLAN_DTYPE, MS_SCHED_STATE_DTYPE,
                     MS_SCHED_NO_SCH, MsTxScheduler, MsTxSchedulerGroup, ms_tx_requests, MS_TX_REQ_DTYPE, MS_TX_PLAN_DTYPE, MS_TX_STATE_DTYPE,
                     MS_TX_QUEUED, MS_TX_LATE, MS_TX_WRAPPED, MS_TX_EXPIRED, MS_TX_OVERLAP, MS_TX_FULL,
                     ms_agc_gate, MS_AGC_RAISE, MS_AGC_SEARCH, MS_AGC_RECORD_DTYPE, MS_AGC_STATE_DTYPE,
                     MS_FCCH_DTYPE, MS_AFC_ENTRY_DTYPE, MS_AFC_STATE_DTYPE, MS_AFC_RING,
                     MS_NCO_ROW_DTYPE, MS_NCO_STATE_DTYPE, MS_FCCH_BIAS_HZ, nco_hz_from_fcch, nco_tx_hz, ms_nco_inc, ms_nco_phase, ms_nco_tables_host,
                     MS_FCCH_HIT_DTYPE, MS_FSEARCH_HOP, MS_FSEARCH_W, MS_FSEARCH_LAG, MS_FSEARCH_MIN_SCORE,
                     AirChannel, AIR_UL, AIR_DL, AIR_PATH_STATE_DTYPE, air_noise_host, AIR_RAY_DTYPE, AIR_MAX_RAYS, air_rays)

__all__ = ["TrxHip", "TrxHipError", "PARAMS_DTYPE", "RESULT_DTYPE", "lib_path", "load_library",
           "OFF", "TSC", "EXT_RACH", "RACH", "SCH", "EDGE", "IDLE",
           "MS_SLOT_DTYPE", "MS_IND_DTYPE", "MS_KIND_BAD", "MS_KIND_FCCH", "MS_KIND_SCH", "MS_KIND_NB", "MS_SLOT_ACTIVE",
           "MS_IND_TRASH", "MS_IND_SILENT", "ms_slot_kind", "MsRxScheduler", "MsRxSchedulerGroup", "MS_PLAN_DTYPE", "MS_SCHED_STATE_DTYPE",
           "MS_SCHED_NO_SCH", "MsTxScheduler", "MsTxSchedulerGroup", "ms_tx_requests", "MS_TX_REQ_DTYPE", "MS_TX_PLAN_DTYPE", "MS_TX_STATE_DTYPE",
           "MS_TX_QUEUED", "MS_TX_LATE", "MS_TX_WRAPPED", "MS_TX_EXPIRED", "MS_TX_OVERLAP", "MS_TX_FULL",
           "ms_agc_gate", "MS_AGC_RAISE", "MS_AGC_SEARCH", "MS_AGC_RECORD_DTYPE", "MS_AGC_STATE_DTYPE",
           "MS_FCCH_DTYPE", "MS_AFC_ENTRY_DTYPE", "MS_AFC_STATE_DTYPE", "MS_AFC_RING",
           "MS_NCO_ROW_DTYPE", "MS_NCO_STATE_DTYPE", "MS_FCCH_BIAS_HZ", "nco_hz_from_fcch", "nco_tx_hz", "ms_nco_inc", "ms_nco_phase", "ms_nco_tables_host",
           "MS_FCCH_HIT_DTYPE", "MS_FSEARCH_HOP", "MS_FSEARCH_W", "MS_FSEARCH_LAG", "MS_FSEARCH_MIN_SCORE",
           "AirChannel", "AIR_UL", "AIR_DL", "AIR_PATH_STATE_DTYPE", "air_noise_host", "AIR_RAY_DTYPE", "AIR_MAX_RAYS", "air_rays"]
