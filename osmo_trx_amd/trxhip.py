"""ctypes binding of libtrxhip.so (include/trxhip.h).  Plumbing only.

Device memory, streams and torch.distributed come from PyTorch; every compute call goes through the
C ABI with raw device pointers.  There is no CPU path here: if the library is not built, or no GPU is
present, construction of TrxHip raises TrxHipError.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))

# CorrType, sigProcLib.h:30-38
OFF, TSC, EXT_RACH, RACH, SCH, EDGE, IDLE = range(7)

PARAMS_DTYPE = np.dtype([("type", "u1"), ("tsc", "u1"), ("max_toa", "<u2"), ("reserved", "<u4")])
RESULT_DTYPE = np.dtype([
    ("rc", "<i4"), ("toa", "<f4"), ("amp_re", "<f4"), ("amp_im", "<f4"), ("ci", "<f4"),
    ("energy", "<f4"), ("rssi", "<f4"), ("tsc", "u1"), ("clip", "u1"), ("idle", "u1"), ("nbits_div4", "u1"),
])
TRXD_META_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("version", "u1"), ("tss", "u1"), ("reserved", "u1")])
# trxhip_tx_params / trxhip_tx_info (include/trxhip.h, the transmit side)
TX_PARAMS_DTYPE = np.dtype([("nbits", "<u2"), ("guard", "u1"), ("flags", "u1"), ("scale_re", "<f4"), ("scale_im", "<f4"),
                            ("reserved", "<u4")])
TX_INFO_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("version", "u1"), ("tx_att", "u1"), ("mod_8psk", "u1"),
                          ("nbits", "<u2"), ("length", "<u2"), ("status", "<i4")])
assert PARAMS_DTYPE.itemsize == 8 and RESULT_DTYPE.itemsize == 32 and TRXD_META_DTYPE.itemsize == 8
assert TX_PARAMS_DTYPE.itemsize == 16 and TX_INFO_DTYPE.itemsize == 16
TX_8PSK = 1             # TRXHIP_TX_8PSK
TX_EMPTY_PULSE = 2      # TRXHIP_TX_EMPTY_PULSE

TRXD_RECORD_BYTES = 156
FLAG_SLICE = 1          # TRXHIP_FLAG_SLICE
FLAG_EXACT_DEMOD = 2    # TRXHIP_FLAG_EXACT_DEMOD
FLAG_IDLE_DUMMY = 4     # TRXHIP_FLAG_IDLE_DUMMY
FLAG_USE_VA = 8         # TRXHIP_FLAG_USE_VA (host pipe, uplink scheduler)
FLAG_FEW_NB_SLOTS = 16 # TRXHIP_FLAG_FEW_NB_SLOTS (a hint: see include/trxhip.h)
SCH_DETECT_FULL, SCH_DETECT_NARROW, SCH_DETECT_BUFFER = 0, 1, 2   # sch_detect_type (sigProcLib.h:139-143)
SCH_SYNC_TRACK, SCH_SYNC_ACQ = 0, 1                               # TRXHIP_SCH_SYNC_*
SCH_SYNC_MAX_LEN = 1 << 20                                        # TRXHIP_SCH_SYNC_MAX_LEN
# trxhip_sch_sync_result
SCH_SYNC_DTYPE = np.dtype([("rc", "<i4"), ("start", "<i4"), ("corr_max", "<f4"), ("fn", "<i4"), ("t1", "<u2"), ("bsic", "u1"),
                           ("t2", "u1"), ("t3p", "u1"), ("reserved", "u1", (3,))])
assert SCH_SYNC_DTYPE.itemsize == 24
# the MS-side downlink burst receiver: trxhip_ms_slot / trxhip_ms_burst_ind, TRXHIP_MS_*
MS_KIND_BAD, MS_KIND_FCCH, MS_KIND_SCH, MS_KIND_NB = 0, 1, 2, 3
MS_SLOT_ACTIVE = 1
MS_IND_TRASH, MS_IND_SILENT = 1, 2
MS_SLOT_LEN = 625
MS_SLOT_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("tsc", "u1"), ("flags", "u1"), ("reserved", "u1")])
MS_IND_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("kind", "u1"), ("sent", "u1"), ("flags", "u1"), ("rssi", "<i2"), ("toa256", "<i2"),
                         ("start", "<i4"), ("corr_max", "<f4"), ("pow", "<f4"), ("sch_fn", "<i4"), ("sch_rc", "u1"), ("sch_bsic", "u1"),
                         ("reserved", "u1", (2,))])
assert MS_SLOT_DTYPE.itemsize == 8 and MS_IND_DTYPE.itemsize == 32


def ms_slot_kind(fn, tn, tsc=0):
    """TRXHIP_MS_KIND_* of slot (fn, tn): gsm_fcch_check_ts / gsm_sch_check_ts (ms/sch.c:100-139); BAD for tn > 7 and for a traffic
    slot with tsc > 7.  The receiver computes the same on the device."""
    if tn > 7:
        return MS_KIND_BAD
    fn51 = fn % 51
    if tn == 0 and fn51 in (0, 10, 20, 30, 40):
        return MS_KIND_FCCH
    if tn == 0 and fn51 in (1, 11, 21, 31, 41):
        return MS_KIND_SCH
    return MS_KIND_NB if tsc <= 7 else MS_KIND_BAD


def few_nb_hint(host_params):
    """TRXHIP_FLAG_FEW_NB_SLOTS when more than 1/32 of the slots of `host_params` (PARAMS_DTYPE[n], or None: no hint) are NOT
    normal-burst slots the normal-burst kernel takes (type TSC = 1, tsc < 8, max_toa <= 32)."""
    if host_params is None or len(host_params) == 0:
        return 0
    nb = (host_params["type"] == 1) & (host_params["tsc"] < 8) & (host_params["max_toa"] <= 32)
    return FLAG_FEW_NB_SLOTS if 32 * (len(host_params) - int(nb.sum())) > len(host_params) else 0


class TrxHipError(RuntimeError):
    pass


def lib_path():
    # TRXHIP_LIB: profiling override (e.g. the -DTRX_DIAG build); default = the product library
    return os.environ.get("TRXHIP_LIB") or os.path.join(PKG, "lib", "libtrxhip.so")


_LIB = None

# every symbol include/trxhip.h declares: (name, restype, argtypes)
_VP, _I, _F, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
SYMBOLS = {
    "trxhip_abi_version": (_I, []),
    "trxhip_device_count": (_I, []),
    "trxhip_create": (_I, [C.POINTER(_VP), _I]),
    "trxhip_destroy": (None, [_VP]),
    "trxhip_strerror": (C.c_char_p, [_I]),
    "trxhip_set_work_pool": (_I, [_VP, _I]),
    "trxhip_set_nb_kernel": (_I, [_VP, _I]),
    "trxhip_fast_stats": (_I, [_VP, C.POINTER(C.c_uint64), _I]),
    "trxhip_tables_size": (_SZ, []),
    "trxhip_tables_generate_host": (_I, [_VP, _SZ]),
    "trxhip_create_from_tables": (_I, [C.POINTER(_VP), _I, _VP, _SZ]),
    "trxhip_tables_device_ptr": (_I, [_VP, C.POINTER(_VP)]),
    "trxhip_tables_checksum": (C.c_uint64, [_VP, _SZ]),
    "trxhip_detect_demod_batch": (_I, [_VP, _VP, _VP, _VP, _VP, _SZ, _I, _I, _F, _F, _I, _I, _VP]),
    "trxhip_detect_demod_batch_cf32": (_I, [_VP, _VP, _VP, _VP, _VP, _SZ, _I, _I, _F, _F, _I, _I, _VP]),
    "trxhip_demod_batch_cf32": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _SZ, _I, _I, _I, _I, _VP]),
    "trxhip_energy_detect_batch_cf32": (_I, [_VP, _VP, _SZ, _I, C.c_uint, _VP, _VP]),
    "trxhip_delay_vector_batch_cf32": (_I, [_VP, _VP, _VP, _VP, _SZ, _I, _VP]),
    "trxhip_scale_vector_cf32": (_I, [_VP, _VP, _SZ, C.c_float, C.c_float, _VP]),
    "trxhip_demod_va_batch_cf32": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _SZ, _I, C.c_float, _I, _I, _VP]),
    "trxhip_detect_sch_batch_cf32": (_I, [_VP, _VP, _VP, _SZ, _SZ, _I, _I, C.c_float, _VP]),
    "trxhip_sch_sync_batch_cf32": (_I, [_VP, _VP, _SZ, _VP, _VP, _SZ, _SZ, _I, _F, _VP]),
    "trxhip_sch_sync_batch_i16": (_I, [_VP, _VP, _SZ, _VP, _VP, _SZ, _SZ, _I, _F, _VP]),
    "trxhip_ms_rx_batch_i16": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP, _SZ, _F, _VP]),
    "trxhip_ms_rx_batch_cf32": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP, _SZ, _F, _VP]),
    "trxhip_vector_slicer": (_I, [_VP, _VP, _VP, _SZ, _VP]),
    "trxhip_pack_trxd_batch": (_I, [_VP, _VP, _VP, _I, _VP, _SZ, _F, _VP]),
    "trxhip_pack_trxd_wire_batch": (_I, [_VP, _VP, _VP, _VP, _I, _VP, _VP, _I, _VP, _SZ, _F, _VP]),
    "trxhip_select_diversity_batch": (_I, [_VP, _VP, _SZ, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "trxhip_apply_diversity_power": (_I, [_VP, _VP, _VP, _VP, _SZ, C.c_float, _VP]),
    "trxhip_hostpipe_create": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_hostpipe_destroy": (None, [_VP]),
    "trxhip_hostpipe_slot_buffers": (_I, [_VP, _I, _VP]),
    "trxhip_hostpipe_set_levels": (_I, [_VP, C.c_float, C.c_float, C.c_float]),
    "trxhip_hostpipe_submit": (_I, [_VP, _I, _SZ]),
    "trxhip_hostpipe_wait": (_I, [_VP, _I]),
    "trxhip_hostpipe_query": (_I, [_VP, _I]),
    "trxhip_hostpipe_run": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "trxhip_hostpipe_register_host": (_I, [_VP, _VP, _SZ]),
    "trxhip_hostpipe_unregister_host": (_I, [_VP, _VP]),
    "trxhip_hostpipe_slot_sources": (_I, [_VP, _I, C.POINTER(_VP)]),
    "trxhip_hostpipe_submit_by_ref": (_I, [_VP, _I, _SZ]),
    "trxhip_convolve_real_batch": (_I, [_VP, _VP, _I, _VP, _I, _VP, _I, _I, _I, _SZ, _VP]),
    "trxhip_convolve_complex_batch": (_I, [_VP, _VP, _I, _VP, _I, _VP, _I, _I, _I, _SZ, _VP]),
    "trxhip_convert_short_float": (_I, [_VP, _VP, _VP, _SZ, _VP]),
    "trxhip_convert_float_short": (_I, [_VP, _VP, _VP, _F, _SZ, _VP]),
    "trxhip_dft_batch": (_I, [_VP, _VP, _VP, _I, _SZ, _SZ, _SZ, _I, _VP]),
    "trxhip_channelize_batch": (_I, [_VP, _VP, _VP, _SZ, _I, _I, _I, _VP]),
    "trxhip_resample_batch": (_I, [_VP, _VP, _VP, _SZ, _I, _I, _SZ, _SZ, _SZ, _VP]),
    "trxhip_modulate_batch": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP, _F, _SZ, _VP, _SZ, _I, _VP]),
    "trxhip_modulate_trxd_batch": (_I, [_VP, _VP, _SZ, _VP, C.c_double, _I, _VP, _VP, _F, _SZ, _VP, _SZ, _VP]),
    "trxhip_tx_tables_size": (_SZ, []),
    "trxhip_tx_tables_generate_host": (_I, [_VP, _SZ]),
    "trxhip_rx_frontend_create": (_I, [_VP, _I, _I, _I, C.POINTER(_VP)]),
    "trxhip_rx_frontend_create_chans": (_I, [_VP, _I, _I, _I, _I, _I, C.POINTER(_VP)]),
    "trxhip_rx_frontend_rows": (_I, [_VP]),
    "trxhip_rx_frontend_out_samples": (_SZ, [_VP, _SZ]),
    "trxhip_rx_frontend_destroy": (None, [_VP]),
    "trxhip_rx_frontend_reset": (_I, [_VP, _VP]),
    "trxhip_rx_frontend_seed": (_I, [_VP, _VP, _SZ, _VP]),
    "trxhip_rx_frontend_pull": (_I, [_VP, _VP, _SZ, _VP, _SZ, _VP]),
    "trxhip_synthesize_batch": (_I, [_VP, _VP, _SZ, _VP, _SZ, _I, _I, _I, _VP]),
    "trxhip_tx_frontend_create": (_I, [_VP, _I, _I, _I, _I, _I, _F, C.POINTER(_VP)]),
    "trxhip_tx_frontend_destroy": (None, [_VP]),
    "trxhip_tx_frontend_reset": (_I, [_VP, _VP]),
    "trxhip_tx_frontend_seed": (_I, [_VP, _VP, _SZ, _SZ, _VP]),
    "trxhip_tx_frontend_push": (_I, [_VP, _VP, _SZ, _SZ, _VP, _VP, _F, _VP]),
    "trxhip_tx_sched_create": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_tx_sched_destroy": (None, [_VP]),
    "trxhip_tx_sched_set_clock": (_I, [_VP, C.c_uint32, _I]),
    "trxhip_tx_sched_clock": (_I, [_VP, C.POINTER(C.c_uint32), C.POINTER(_I)]),
    "trxhip_tx_sched_set_slot": (_I, [_VP, _I, _I, _I]),
    "trxhip_tx_sched_set_muted": (_I, [_VP, _I, _I]),
    "trxhip_tx_sched_submit": (_I, [_VP, _I, _VP, _SZ, C.POINTER(C.c_int64)]),
    "trxhip_tx_sched_render": (_I, [_VP, _SZ, _VP, _SZ, _VP, _VP, _VP]),
    "trxhip_tx_sched_render_frontend": (_I, [_VP, _SZ, _VP, _VP, _VP, _F, _SZ, C.POINTER(_SZ), C.POINTER(_SZ), _VP]),
    "trxhip_tx_sched_plan": (_I, [_VP, _I, _VP, _SZ]),
    "trxhip_tx_sched_counters": (_I, [_VP, _I, _VP]),
    "trxhip_rx_sched_create": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_rx_sched_create_sps": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_rx_sched_destroy": (None, [_VP]),
    "trxhip_rx_sched_set_clock": (_I, [_VP, C.c_uint32, _I]),
    "trxhip_rx_sched_clock": (_I, [_VP, C.POINTER(C.c_uint32), C.POINTER(_I)]),
    "trxhip_rx_sched_set_slot": (_I, [_VP, _I, _I, _I]),
    "trxhip_rx_sched_set_handover": (_I, [_VP, _I, _I, _I]),
    "trxhip_rx_sched_set_muted": (_I, [_VP, _I, _I]),
    "trxhip_rx_sched_set_trxd_version": (_I, [_VP, _I, _I]),
    "trxhip_rx_sched_set_rssi_offset": (_I, [_VP, _I, _F]),
    "trxhip_rx_sched_set_max_toa": (_I, [_VP, _I, _I]),
    "trxhip_rx_sched_slots": (C.c_int64, [_VP, _SZ]),
    "trxhip_rx_sched_pull_s16": (_I, [_VP, _VP, _SZ, _SZ, _VP, _I, _VP, _VP, _VP, _SZ, C.POINTER(_SZ), C.POINTER(_SZ), _VP]),
    "trxhip_rx_sched_pull_cf32": (_I, [_VP, _VP, _SZ, _SZ, _VP, _I, _VP, _VP, _VP, _SZ, C.POINTER(_SZ), C.POINTER(_SZ), _VP]),
    "trxhip_rx_sched_slots_frontend": (C.c_int64, [_VP, _VP, _SZ]),
    "trxhip_rx_sched_pull_frontend": (_I, [_VP, _VP, _VP, _SZ, _VP, _SZ, _VP, _I, _VP, _VP, _VP, _SZ, C.POINTER(_SZ), C.POINTER(_SZ),
                                           _VP]),
    "trxhip_rx_sched_plan": (_I, [_VP, _I, _VP, _SZ]),
    "trxhip_rx_sched_counters": (_I, [_VP, _I, _VP]),
    "trxhip_rx_sched_noise_state": (_I, [_VP, _I, _VP, C.POINTER(C.c_uint32), C.POINTER(_F)]),
    "trxhip_ms_sched_create": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_ms_sched_destroy": (None, [_VP]),
    "trxhip_ms_sched_set_clock": (_I, [_VP, C.c_uint32, _I, C.c_int64]),
    "trxhip_ms_sched_clock": (_I, [_VP, C.POINTER(C.c_uint32), C.POINTER(_I), C.POINTER(C.c_int64)]),
    "trxhip_ms_sched_set_tsc": (_I, [_VP, _I]),
    "trxhip_ms_sched_set_active": (_I, [_VP, C.c_uint8]),
    "trxhip_ms_sched_set_tracking": (_I, [_VP, _I]),
    "trxhip_ms_sched_feed_starts": (_I, [_VP, _VP, _SZ]),
    "trxhip_ms_sched_acquire_s16": (_I, [_VP, _VP, _SZ, C.c_int64, _VP, _VP]),
    "trxhip_ms_sched_acquire_cf32": (_I, [_VP, _VP, _SZ, C.c_int64, _VP, _VP]),
    "trxhip_ms_sched_slots": (C.c_int64, [_VP, _SZ]),
    "trxhip_ms_sched_pull_s16": (_I, [_VP, _VP, _SZ, C.c_int64, _VP, _VP, _SZ, C.POINTER(_SZ), C.POINTER(_SZ), _VP]),
    "trxhip_ms_sched_pull_cf32": (_I, [_VP, _VP, _SZ, C.c_int64, _VP, _VP, _SZ, C.POINTER(_SZ), C.POINTER(_SZ), _VP]),
    "trxhip_ms_sched_plan": (_I, [_VP, _VP, _SZ]),
    "trxhip_ms_sched_state": (_I, [_VP, _VP]),
    "trxhip_ms_group_create": (_I, [_VP, _F, _SZ, _VP, C.POINTER(_VP)]),
    "trxhip_ms_group_destroy": (None, [_VP]),
    "trxhip_ms_group_members": (_I, [_VP]),
    "trxhip_ms_group_set_clock": (_I, [_VP, C.c_uint32, C.c_uint32, _I, C.c_int64]),
    "trxhip_ms_group_clock": (_I, [_VP, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(_I), C.POINTER(C.c_int64)]),
    "trxhip_ms_group_set_tsc": (_I, [_VP, C.c_uint32, _I]),
    "trxhip_ms_group_set_active": (_I, [_VP, C.c_uint32, C.c_uint8]),
    "trxhip_ms_group_set_tracking": (_I, [_VP, C.c_uint32, _I]),
    "trxhip_ms_group_feed_starts": (_I, [_VP, C.c_uint32, _VP, _SZ]),
    "trxhip_ms_group_slots": (C.c_int64, [_VP, C.c_uint32, _SZ]),
    "trxhip_ms_group_plan": (_I, [_VP, C.c_uint32, _VP, _SZ]),
    "trxhip_ms_group_state": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_group_acquire_s16": (_I, [_VP, _VP, _SZ, _VP, _SZ, _SZ, _VP, _VP, _VP, _VP]),
    "trxhip_ms_group_acquire_cf32": (_I, [_VP, _VP, _SZ, _VP, _SZ, _SZ, _VP, _VP, _VP, _VP]),
    "trxhip_ms_group_pull_s16": (_I, [_VP, _VP, _VP, _VP, _SZ, _VP, _VP, C.POINTER(_I), _VP]),
    "trxhip_ms_group_pull_cf32": (_I, [_VP, _VP, _VP, _VP, _SZ, _VP, _VP, C.POINTER(_I), _VP]),
    "trxhip_ms_level_batch_i16": (_I, [_VP, _VP, _SZ, _SZ, _SZ, _VP, _VP]),
    "trxhip_ms_agc_gate": (_I, [_F, _F, _F, C.POINTER(_F)]),
    "trxhip_ms_agc_sched_set": (_I, [_VP, _VP]),
    "trxhip_ms_agc_sched_set_gain": (_I, [_VP, _F]),
    "trxhip_ms_agc_sched_state": (_I, [_VP, _VP]),
    "trxhip_ms_agc_sched_feed_levels": (_I, [_VP, _VP, _SZ]),
    "trxhip_ms_agc_group_set": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_agc_group_set_gain": (_I, [_VP, C.c_uint32, _F]),
    "trxhip_ms_agc_group_state": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_agc_group_feed_levels": (_I, [_VP, C.c_uint32, _VP, _SZ]),
    "trxhip_ms_fcch_batch_i16": (_I, [_VP, _VP, _SZ, _VP, _SZ, _F, _VP]),
    "trxhip_ms_fcch_batch_cf32": (_I, [_VP, _VP, _SZ, _VP, _SZ, _F, _VP]),
    "trxhip_ms_afc_sched_set": (_I, [_VP, _VP]),
    "trxhip_ms_afc_sched_state": (_I, [_VP, _VP]),
    "trxhip_ms_afc_group_set": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_afc_group_state": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_nco_tables_host": (_I, [_VP]),
    "trxhip_ms_nco_inc": (_I, [C.c_double, C.POINTER(C.c_int32)]),
    "trxhip_ms_nco_phase": (C.c_uint32, [C.c_uint32, C.c_int64, C.c_int32, C.c_int64]),
    "trxhip_ms_nco_batch_i16": (_I, [_VP, _VP, _SZ, _VP, _VP, _SZ, _SZ, _SZ, _VP]),
    "trxhip_ms_nco_batch_cf32": (_I, [_VP, _VP, _SZ, _VP, _VP, _SZ, _SZ, _SZ, _VP]),
    "trxhip_ms_nco_sched_set": (_I, [_VP, _VP]),
    "trxhip_ms_nco_sched_state": (_I, [_VP, _VP]),
    "trxhip_ms_nco_group_set": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_nco_group_state": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_fcch_search_i16": (_I, [_VP, _VP, _SZ, _SZ, _SZ, C.c_double, C.c_float, _VP, _VP, _VP]),
    "trxhip_ms_fcch_search_cf32": (_I, [_VP, _VP, _SZ, _SZ, _SZ, C.c_double, C.c_float, _VP, _VP, _VP]),
    "trxhip_ms_afc_sched_acquire_s16": (_I, [_VP, _VP, _SZ, C.c_int64, C.c_double, _VP, _VP, _VP, _VP]),
    "trxhip_ms_afc_sched_acquire_cf32": (_I, [_VP, _VP, _SZ, C.c_int64, C.c_double, _VP, _VP, _VP, _VP]),
    "trxhip_ms_afc_group_acquire_s16": (_I, [_VP, _VP, _SZ, _VP, _SZ, _SZ, _VP, C.c_double, _VP, _VP, _VP, _VP, _VP]),
    "trxhip_ms_afc_group_acquire_cf32": (_I, [_VP, _VP, _SZ, _VP, _SZ, _SZ, _VP, C.c_double, _VP, _VP, _VP, _VP, _VP]),
    "trxhip_ms_tx_create": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_ms_tx_destroy": (None, [_VP]),
    "trxhip_ms_tx_set_ta": (_I, [_VP, _I]),
    "trxhip_ms_tx_submit": (_I, [_VP, _VP, _SZ, C.c_uint32, _I, C.c_int64, _VP, _VP]),
    "trxhip_ms_tx_render_s16": (_I, [_VP, _VP, _SZ, C.c_int64, C.POINTER(_SZ), _VP]),
    "trxhip_ms_tx_state": (_I, [_VP, _VP]),
    "trxhip_ms_tx_group_create": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_ms_tx_group_destroy": (None, [_VP]),
    "trxhip_ms_tx_group_size": (_I, [_VP]),
    "trxhip_ms_tx_group_set_ta": (_I, [_VP, C.c_uint32, _I]),
    "trxhip_ms_tx_group_submit": (_I, [_VP, _VP, _VP, _SZ, _VP, _VP, C.POINTER(_SZ), _VP]),
    "trxhip_ms_tx_group_render_s16": (_I, [_VP, _VP, _SZ, _VP, _VP, _VP, C.POINTER(_I), _VP]),
    "trxhip_ms_tx_group_state": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_nco_tx_set": (_I, [_VP, _VP]),
    "trxhip_ms_nco_tx_state": (_I, [_VP, _VP]),
    "trxhip_ms_nco_tx_group_set": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_ms_nco_tx_group_state": (_I, [_VP, C.c_uint32, _VP]),
    "trxhip_air_create": (_I, [_VP, _VP, C.POINTER(_VP)]),
    "trxhip_air_destroy": (None, [_VP]),
    "trxhip_air_set_path": (_I, [_VP, _I, C.c_uint32, _VP]),
    "trxhip_air_set_noise": (_I, [_VP, _I, C.c_uint32, C.c_double]),
    "trxhip_air_path_state": (_I, [_VP, _I, C.c_uint32, _VP]),
    "trxhip_air_reset": (_I, [_VP, _I, C.c_int64]),
    "trxhip_air_uplink_s16": (_I, [_VP, _VP, _SZ, C.c_int64, _SZ, _VP, _VP]),
    "trxhip_air_downlink_s16": (_I, [_VP, _VP, C.c_int64, _SZ, _VP, _SZ, _VP]),
    "trxhip_air_noise_host": (C.c_int32, [C.c_uint32, C.c_uint32, C.c_int64, C.c_int32]),
    "trxhip_multipath_set": (_I, [_VP, _I, C.c_uint32, _VP, C.c_uint32]),
    "trxhip_multipath_state": (_I, [_VP, _I, C.c_uint32, _VP, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]),
}


def load_library():
    """dlopen libtrxhip.so and bind every symbol of include/trxhip.h.  Raises if it is not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise TrxHipError(f"{path} is not built (run `python -m osmo_trx_amd.build`); there is no CPU fallback")
    try:
        L = C.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise TrxHipError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        if (name == "trxhip_fast_stats" or name.startswith(("trxhip_hostpipe_", "trxhip_ms_agc_", "trxhip_ms_level_", "trxhip_ms_afc_", "trxhip_ms_fcch_", "trxhip_ms_nco_", "trxhip_air_", "trxhip_multipath_"))) and \
                os.environ.get("TRXHIP_LIB") and not hasattr(L, name):
            continue          # tools/measure.py ab against an older measurement build of the library (product: always bound)
        f = getattr(L, name)  # AttributeError if the export is missing
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def _check(rc, what):
    if rc != 0:
        msg = load_library().trxhip_strerror(rc).decode()
        raise TrxHipError(f"{what} failed: {rc} ({msg})")


def generate_tables_host():
    """The table blob as bytes (host-only; works without a GPU)."""
    L = load_library()
    n = L.trxhip_tables_size()
    buf = (C.c_ubyte * n)()
    _check(L.trxhip_tables_generate_host(buf, n), "trxhip_tables_generate_host")
    return bytes(buf)


def generate_tx_tables_host():
    """The transmit table struct (csrc/trx_tx_tables.h) as bytes (host-only; works without a GPU)."""
    L = load_library()
    n = L.trxhip_tx_tables_size()
    buf = (C.c_ubyte * n)()
    _check(L.trxhip_tx_tables_generate_host(buf, n), "trxhip_tx_tables_generate_host")
    return bytes(buf)


def tx_params_host(nbits, guard=0, flags=0, scale=1.0, n=None):
    """TX_PARAMS_DTYPE[n] from per-burst arrays or scalars (broadcast) of nbits, guard, flags and complex scale (1.0: unscaled).
    n: the number of bursts when every argument is a scalar (default: the longest argument)."""
    args = [np.atleast_1d(np.asarray(x)) for x in (nbits, guard, flags, scale)]
    if n is None:
        n = max(len(x) for x in args)
    nbits, guard, flags, sc = (np.broadcast_to(x, (n,)) for x in args)
    p = np.zeros(n, dtype=TX_PARAMS_DTYPE)
    p["nbits"], p["guard"], p["flags"] = nbits, guard, flags
    sc = sc.astype(np.complex128)
    p["scale_re"] = sc.real.astype(np.float32)
    p["scale_im"] = sc.imag.astype(np.float32)
    return p


def tables_checksum(blob):
    L = load_library()
    b = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
    return int(L.trxhip_tables_checksum(b, len(blob)))


class TrxHip:
    """One context per GPU (owns the device-resident tables).  All tensors are torch CUDA tensors."""

    def __init__(self, device=0, tables_blob=None):
        import torch
        self.torch = torch
        self.L = load_library()
        if not torch.cuda.is_available():
            raise TrxHipError("no GPU visible: osmo_trx_amd has no CPU fallback")
        self.device = int(device)
        h = _VP()
        if tables_blob is None:
            _check(self.L.trxhip_create(C.byref(h), self.device), "trxhip_create")
        else:
            b = (C.c_ubyte * len(tables_blob)).from_buffer_copy(tables_blob)
            _check(self.L.trxhip_create_from_tables(C.byref(h), self.device, b, len(tables_blob)),
                   "trxhip_create_from_tables")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers -------------------------------------------------------------------------------
    def _stream(self, stream=None):
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device)
        return _VP(stream.cuda_stream)

    def _dev(self, t, dtype=None):
        torch = self.torch
        assert t.is_cuda and t.device.index == self.device and t.is_contiguous(), "need a contiguous tensor on this GPU"
        if dtype is not None:
            assert t.dtype == dtype, (t.dtype, dtype)
        return _VP(t.data_ptr())

    def tables_device_tensor(self):
        """uint8 view-less copy target for an in-place RCCL broadcast: (ptr, nbytes)."""
        p = _VP()
        _check(self.L.trxhip_tables_device_ptr(self.h, C.byref(p)), "trxhip_tables_device_ptr")
        return p.value, int(self.L.trxhip_tables_size())

    def set_work_pool(self, enabled):
        """Cross-die work pool of the 4-SPS kernel on / off (results never depend on it; a measurement switch)."""
        _check(self.L.trxhip_set_work_pool(self.h, 1 if enabled else 0), "trxhip_set_work_pool")

    def set_nb_kernel(self, enabled):
        """Normal-burst kernel + leftover list (default) or the general kernel alone (results are bit-identical; a measurement switch)."""
        _check(self.L.trxhip_set_nb_kernel(self.h, 1 if enabled else 0), "trxhip_set_nb_kernel")

    def fast_stats(self, reset=False):
        """Counters of the fused kernels' FAST detector since the last reset: {"reruns": bursts whose TOA search was re-run in
        the reference's operand order; left_*: bursts the normal-burst kernel left to the general one (correlation guard, peak-ratio gate
        too close to call, TOA outside the straight-line demodulator's geometry)}.  Synchronises the device."""
        out = (C.c_uint64 * 4)()
        _check(self.L.trxhip_fast_stats(self.h, out, 1 if reset else 0), "trxhip_fast_stats")
        return {"reruns": int(out[0]), "left_guard": int(out[1]), "left_gate": int(out[2]), "left_geometry": int(out[3])}

    def params_tensor(self, params_np):
        """PARAMS_DTYPE[n] numpy -> uint8[n, 8] device tensor."""
        torch = self.torch
        a = np.ascontiguousarray(params_np, dtype=PARAMS_DTYPE).view(np.uint8).reshape(-1, 8)
        return torch.from_numpy(a.copy()).to(f"cuda:{self.device}")

    def tx_params_tensor(self, params_np):
        """TX_PARAMS_DTYPE[n] numpy -> uint8[n, 16] device tensor."""
        torch = self.torch
        a = np.ascontiguousarray(params_np, dtype=TX_PARAMS_DTYPE).view(np.uint8).reshape(-1, 16)
        return torch.from_numpy(a.copy()).to(f"cuda:{self.device}")

    def select_diversity(self, iq_paths, sps=4, stream=None):
        """Transceiver.cpp:723-741.  iq_paths: int16[n, n_paths, burst_len, 2] -> (iq_sel int16[n, burst_len, 2],
        avg_energy float32[n], path uint8[n])."""
        torch = self.torch
        n, n_paths, burst_len = iq_paths.shape[0], iq_paths.shape[1], iq_paths.shape[2]
        dev = iq_paths.device
        sel = torch.empty((n, burst_len, 2), dtype=torch.int16, device=dev)
        avg = torch.empty(n, dtype=torch.float32, device=dev)
        path = torch.empty(n, dtype=torch.uint8, device=dev)
        _check(self.L.trxhip_select_diversity_batch(self.h, self._dev(iq_paths, torch.int16), n, n_paths, burst_len, sps,
                                                    self._dev(sel), self._dev(avg), self._dev(path), self._stream(stream)),
               "trxhip_select_diversity_batch")
        return sel, avg, path

    def apply_diversity_power(self, results, params, avg_energy, full_scale=32767.0, stream=None):
        _check(self.L.trxhip_apply_diversity_power(self.h, self._dev(results), self._dev(params), self._dev(avg_energy),
                                                   results.shape[0], full_scale, self._stream(stream)),
               "trxhip_apply_diversity_power")

    # ---- hot path ------------------------------------------------------------------------------
    def detect_demod(self, iq, params, sps=4, threshold=4.0, full_scale=32767.0, soft_stride=148, slice_bits=True,
                     results=None, soft=None, stream=None, want_soft=True, exact=False, idle_dummy=False,
                     host_params=None, hint=None):
        """iq: int16[n, burst_len, 2] or complex64[n, burst_len] (device).  params: uint8[n, 8] (device).
        host_params: the caller's host copy of the parameters (PARAMS_DTYPE[n]), if it has one: the slot types decide the
        TRXHIP_FLAG_FEW_NB_SLOTS hint (a batch with few normal-burst slots runs the general kernel alone; results do not change).
        hint: that flag already worked out (few_nb_hint(host_params): a pass over the host array, a few milliseconds for a million
        slots -- a caller that launches the same slot table again and again computes it once).
        Returns (results uint8[n, 32], soft float32[n, soft_stride]) device tensors."""
        torch = self.torch
        n = iq.shape[0]
        burst_len = iq.shape[1]
        dev = f"cuda:{self.device}"
        if results is None:
            results = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        if soft is None and want_soft:
            soft = torch.empty((n, soft_stride), dtype=torch.float32, device=dev)
        assert params.shape == (n, 8) and params.dtype == torch.uint8
        sp = self._dev(soft, torch.float32) if soft is not None else _VP(0)
        if iq.dtype == torch.int16:
            assert iq.shape[2] == 2
            fn = self.L.trxhip_detect_demod_batch
            ip = self._dev(iq, torch.int16)
        elif iq.dtype == torch.complex64:
            fn = self.L.trxhip_detect_demod_batch_cf32
            ip = self._dev(iq)
        else:
            raise TrxHipError(f"unsupported IQ dtype {iq.dtype}")
        rc = fn(self.h, ip, self._dev(params), self._dev(results), sp, n, burst_len, sps,
                threshold, full_scale, soft_stride,
                (FLAG_SLICE if slice_bits else 0) | (FLAG_EXACT_DEMOD if exact else 0) |
                (FLAG_IDLE_DUMMY if idle_dummy else 0) | (few_nb_hint(host_params) if hint is None else int(hint)),
                self._stream(stream))
        _check(rc, "trxhip_detect_demod_batch")
        return results, soft

    # ---- transmit side ------------------------------------------------------------------------------
    def _tx_outputs(self, n, out_stride, cf32, s16_scale):
        torch = self.torch
        dev = f"cuda:{self.device}"
        out = torch.empty((n, out_stride), dtype=torch.complex64, device=dev) if cf32 else None
        s16 = torch.empty((n, out_stride, 2), dtype=torch.int16, device=dev) if s16_scale is not None else None
        return out, s16

    def modulate(self, bits, params, sps=4, cf32=True, s16_scale=None, out_stride=625, stream=None):
        """modulateBurst() / modulateEdgeBurst() over a batch.  bits: uint8[n, bits_stride] (bit 0 of each byte counts),
        params: uint8[n, 16] (tx_params_tensor).  Returns (complex64[n, out_stride] or None, int16[n, out_stride, 2] or None
        -- only with s16_scale --, int32[n] lengths, TRXHIP_EINVAL where a descriptor was refused)."""
        torch = self.torch
        n, stride = bits.shape
        assert params.shape == (n, 16) and params.dtype == torch.uint8
        out, s16 = self._tx_outputs(n, out_stride, cf32, s16_scale)
        lens = torch.empty(n, dtype=torch.int32, device=bits.device)
        _check(self.L.trxhip_modulate_batch(self.h, self._dev(bits, torch.uint8), stride, self._dev(params),
                                            self._dev(out) if out is not None else _VP(0),
                                            self._dev(s16) if s16 is not None else _VP(0),
                                            float(s16_scale or 0.0), out_stride, self._dev(lens), n, sps, self._stream(stream)),
               "trxhip_modulate_batch")
        return out, s16, lens

    def modulate_trxd(self, dgrams, lengths, full_scale, sps=4, cf32=True, s16_scale=None, out_stride=625, stream=None):
        """TRXD downlink datagrams -> burst samples (driveTxPriorityQueue + addRadioVector).  dgrams: uint8[n, dgram_stride],
        lengths: uint16 as int16/int32 tensor of n.  Returns (complex64 rows or None, int16 rows or None, uint8[n, 16] info
        records: TX_INFO_DTYPE)."""
        torch = self.torch
        n, stride = dgrams.shape
        lens = lengths.to(torch.int32).to(torch.int16).contiguous()      # uint16 bit pattern
        assert lens.shape == (n,)
        out, s16 = self._tx_outputs(n, out_stride, cf32, s16_scale)
        info = torch.empty((n, 16), dtype=torch.uint8, device=dgrams.device)
        _check(self.L.trxhip_modulate_trxd_batch(self.h, self._dev(dgrams, torch.uint8), stride, self._dev(lens), float(full_scale),
                                                 sps, self._dev(out) if out is not None else _VP(0),
                                                 self._dev(s16) if s16 is not None else _VP(0), float(s16_scale or 0.0),
                                                 out_stride, self._dev(info), n, self._stream(stream)),
               "trxhip_modulate_trxd_batch")
        return out, s16, info

    @staticmethod
    def tx_info_to_numpy(info):
        return info.cpu().numpy().reshape(-1).view(TX_INFO_DTYPE)

    def demod_only(self, iq_cf32, params, ebp, sps=4, soft_stride=156, slice_bits=False, exact=False, stream=None):
        """demodAnyBurst() alone: iq complex64[n, L], params uint8[n, 8], ebp float32[n, 4] = {toa, amp_re, amp_im, 0}."""
        torch = self.torch
        n, burst_len = iq_cf32.shape
        results = torch.empty((n, 32), dtype=torch.uint8, device=iq_cf32.device)
        soft = torch.empty((n, soft_stride), dtype=torch.float32, device=iq_cf32.device)
        rc = self.L.trxhip_demod_batch_cf32(self.h, self._dev(iq_cf32), self._dev(params), self._dev(ebp, torch.float32),
                                            self._dev(results), self._dev(soft), n, burst_len, sps, soft_stride,
                                            (FLAG_SLICE if slice_bits else 0) | (FLAG_EXACT_DEMOD if exact else 0),
                                            self._stream(stream))
        _check(rc, "trxhip_demod_batch_cf32")
        return results, soft

    def delay_vector(self, x_cf32, delays, stream=None):
        """delayVector(): x complex64[n, len], delays float32[n] (samples).  Returns a new tensor."""
        torch = self.torch
        n, length = x_cf32.shape
        out = torch.empty_like(x_cf32)
        _check(self.L.trxhip_delay_vector_batch_cf32(self.h, self._dev(x_cf32), self._dev(out),
                                                     self._dev(delays, torch.float32), n, length, self._stream(stream)),
               "trxhip_delay_vector_batch_cf32")
        return out

    def scale_vector(self, x_cf32, scale, stream=None):
        """scaleVector(): in place x *= scale (complex)."""
        scale = complex(scale)
        _check(self.L.trxhip_scale_vector_cf32(self.h, self._dev(x_cf32), x_cf32.numel(), scale.real, scale.imag,
                                               self._stream(stream)), "trxhip_scale_vector_cf32")
        return x_cf32

    def demod_va(self, iq_cf32, params, scale=1.0 / 16383.0, soft_stride=156, slice_bits=False, detected=None, stream=None):
        """Viterbi alternative (cfg->use_va): scaleVector + demodAnyBurst_va.  iq complex64[n, L], params uint8[n, 8].
        detected: uint8[n, 32] result records of a detection launch (only bursts with rc > 0 are demodulated).
        Returns (soft float32[n, soft_stride], starts int32[n])."""
        torch = self.torch
        n, burst_len = iq_cf32.shape
        soft = torch.empty((n, soft_stride), dtype=torch.float32, device=iq_cf32.device)
        starts = torch.empty(n, dtype=torch.int32, device=iq_cf32.device)
        _check(self.L.trxhip_demod_va_batch_cf32(self.h, self._dev(iq_cf32), self._dev(params),
                                                 self._dev(detected) if detected is not None else _VP(0), self._dev(soft),
                                                 self._dev(starts), n, burst_len, scale, soft_stride,
                                                 FLAG_SLICE if slice_bits else 0, self._stream(stream)),
               "trxhip_demod_va_batch_cf32")
        return soft, starts

    def detect_sch(self, iq_cf32, state=0, sps=4, threshold=4.0, stream=None):
        """detectSCHBurst() for complex64[n_bufs, buf_len] buffers; state = SCH_DETECT_FULL / _NARROW / _BUFFER.
        Returns results uint8[n_bufs, 32] (rc, toa, amp, ci)."""
        torch = self.torch
        n, buf_len = iq_cf32.shape
        results = torch.empty((n, 32), dtype=torch.uint8, device=iq_cf32.device)
        _check(self.L.trxhip_detect_sch_batch_cf32(self.h, self._dev(iq_cf32), self._dev(results), n, buf_len, sps, state,
                                                   threshold, self._stream(stream)), "trxhip_detect_sch_batch_cf32")
        return results

    def sch_sync(self, iq, mode, scale=1.0 / 2047.0, want_bits=False, buf_len=None, stream=None):
        """The MS-side SCH receiver (ms_trx::handle_sch + decode_sch): iq complex64[n, stride] or int16[n, stride, 2] buffers of
        which the first buf_len samples (default: all) are used; mode SCH_SYNC_TRACK (one slot) or SCH_SYNC_ACQ (buffer search);
        scale: convert_and_scale's factor, 1 / rxFullScale in the reference.  Returns SCH_SYNC_DTYPE[n] (numpy; synchronises),
        and with want_bits also the demodulated sbits int8[n, 148]."""
        torch = self.torch
        n, stride = iq.shape[0], iq.shape[1]
        if iq.dtype == torch.int16:
            assert iq.dim() == 3 and iq.shape[2] == 2
            fn, name = self.L.trxhip_sch_sync_batch_i16, "trxhip_sch_sync_batch_i16"
        elif iq.dtype == torch.complex64:
            fn, name = self.L.trxhip_sch_sync_batch_cf32, "trxhip_sch_sync_batch_cf32"
        else:
            raise TrxHipError(f"unsupported IQ dtype {iq.dtype}")
        results = torch.empty((n, SCH_SYNC_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        bits = torch.empty((n, 148), dtype=torch.int8, device=iq.device) if want_bits else None
        _check(fn(self.h, self._dev(iq), stride, self._dev(results), self._dev(bits) if want_bits else _VP(0), n,
                  stride if buf_len is None else buf_len, mode, scale, self._stream(stream)), name)
        rec = results.cpu().numpy().reshape(-1).view(SCH_SYNC_DTYPE)
        return (rec, bits.cpu().numpy()) if want_bits else rec

    @staticmethod
    def ms_rx_geometry(iq, slots, rx_full_scale):
        """What ms_rx() checks before it touches the GPU: (n slots, slot stride in samples, whether iq is int16)."""
        import math
        import torch
        if iq.dtype == torch.int16 and iq.dim() == 3 and iq.shape[2] == 2:
            i16 = True
        elif iq.dtype == torch.complex64 and iq.dim() == 2:
            i16 = False
        else:
            raise TrxHipError(f"iq must be int16[n, stride, 2] or complex64[n, stride], not {iq.dtype}{list(iq.shape)}")
        n, stride = int(iq.shape[0]), int(iq.shape[1])
        if n == 0 or stride < MS_SLOT_LEN:
            raise TrxHipError(f"need at least one slot of {MS_SLOT_LEN} samples, got {n} x {stride}")
        if isinstance(slots, np.ndarray):
            ok = slots.dtype == MS_SLOT_DTYPE and slots.shape == (n,)
        else:
            ok = slots.dtype == torch.uint8 and tuple(slots.shape) == (n, MS_SLOT_DTYPE.itemsize)
        if not ok:
            raise TrxHipError(f"slots must be MS_SLOT_DTYPE[{n}] or a device uint8[{n}, {MS_SLOT_DTYPE.itemsize}] tensor")
        if not (math.isfinite(rx_full_scale) and rx_full_scale > 0):
            raise TrxHipError(f"rx_full_scale must be finite and positive, not {rx_full_scale}")
        return n, stride, i16

    def ms_slots_tensor(self, slots_np):
        """MS_SLOT_DTYPE[n] numpy -> uint8[n, 8] device tensor."""
        a = np.ascontiguousarray(slots_np, dtype=MS_SLOT_DTYPE).view(np.uint8).reshape(-1, MS_SLOT_DTYPE.itemsize)
        return self.torch.from_numpy(a.copy()).to(f"cuda:{self.device}")

    def ms_rx(self, iq, slots, rx_full_scale=2047.0, want_bits=True, stream=None):
        """The MS-side downlink burst receiver (upper_trx::pullRadioVector + the burst indication of driveReceiveFIFO): iq
        int16[n, stride, 2] or complex64[n, stride] slots of which the first 625 samples are used; slots MS_SLOT_DTYPE[n] (numpy) or a
        device uint8[n, 8] tensor; rx_full_scale: the reference's rxFullScale.  Returns (MS_IND_DTYPE[n] numpy, sbits int8[n, 148]
        numpy or None); synchronises."""
        torch = self.torch
        n, stride, i16 = self.ms_rx_geometry(iq, slots, rx_full_scale)
        fn, name = (self.L.trxhip_ms_rx_batch_i16, "trxhip_ms_rx_batch_i16") if i16 else \
            (self.L.trxhip_ms_rx_batch_cf32, "trxhip_ms_rx_batch_cf32")
        d_slots = self.ms_slots_tensor(slots) if isinstance(slots, np.ndarray) else slots
        ind = torch.empty((n, MS_IND_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        bits = torch.empty((n, 148), dtype=torch.int8, device=iq.device) if want_bits else None
        _check(fn(self.h, self._dev(iq), stride, self._dev(d_slots, torch.uint8), self._dev(ind), self._dev(bits) if want_bits else _VP(0),
                  n, rx_full_scale, self._stream(stream)), name)
        rec = ind.cpu().numpy().reshape(-1).view(MS_IND_DTYPE)
        return rec, (bits.cpu().numpy() if want_bits else None)

    def ms_level(self, rows, row_len=None, row_stride=None, n_rows=None, stream=None):
        """normed_abs_sum() (ms/ms.h:116-126) of int16 rows, bit for bit the reference's sequential float sum: rows int16[n, len, 2],
        or a flat int16[total, 2] buffer (a view that begins at any sample) holding n_rows rows of row_len samples, row_stride
        samples apart.  Returns a float32[n] device tensor; does not wait."""
        torch = self.torch
        assert rows.dtype == torch.int16 and rows.shape[-1] == 2, (rows.shape, rows.dtype)
        if rows.dim() == 3:
            n, length = rows.shape[0], rows.shape[1]
            stride = length
        else:
            n, length, stride = int(n_rows), int(row_len), int(row_stride if row_stride is not None else row_len)
            assert rows.dim() == 2 and n >= 0 and (n == 0 or (n - 1) * stride + length <= rows.shape[0]), (rows.shape, n, length, stride)
        out = torch.empty((n,), dtype=torch.float32, device=rows.device)
        _check(self.L.trxhip_ms_level_batch_i16(self.h, self._dev(rows), n, length, stride, self._dev(out), self._stream(stream)),
               "trxhip_ms_level_batch_i16")
        return out

    def ms_fcch(self, iq, rx_full_scale=2047.0, slot_stride=625, n_slots=None, stream=None):
        """gsm_fcch_offset() (ms/sch.c:255-314) of slots of 625 samples: iq int16[n, stride, 2] or complex64[n, stride], or a flat
        int16[total, 2] / complex64[total] buffer (a view that begins at any sample) holding n_slots rows slot_stride samples
        apart; samples 52 .. 175 of a row are read.  Returns MS_FCCH_DTYPE[n] (numpy); synchronises."""
        torch = self.torch
        if iq.dtype == torch.int16 and iq.shape[-1] == 2 and iq.dim() in (2, 3):
            i16, flat = True, iq.dim() == 2
        elif iq.dtype == torch.complex64 and iq.dim() in (1, 2):
            i16, flat = False, iq.dim() == 1
        else:
            raise TrxHipError(f"iq must be int16[n, stride, 2] / [total, 2] or complex64[n, stride] / [total], not {iq.dtype}{list(iq.shape)}")
        if flat:
            n, stride = int(n_slots), int(slot_stride)
            if n < 1 or stride < MS_SLOT_LEN or (n - 1) * stride + MS_SLOT_LEN > iq.shape[0]:
                raise TrxHipError(f"{n} rows of {MS_SLOT_LEN} samples, {stride} apart, do not lie in {iq.shape[0]} samples")
        else:
            n, stride = int(iq.shape[0]), int(iq.shape[1])
        if n == 0 or stride < MS_SLOT_LEN:
            raise TrxHipError(f"need at least one slot of {MS_SLOT_LEN} samples, got {n} x {stride}")
        out = torch.empty((n, MS_FCCH_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        fn, name = (self.L.trxhip_ms_fcch_batch_i16, "trxhip_ms_fcch_batch_i16") if i16 else \
            (self.L.trxhip_ms_fcch_batch_cf32, "trxhip_ms_fcch_batch_cf32")
        _check(fn(self.h, self._dev(iq), stride, self._dev(out), n, rx_full_scale, self._stream(stream)), name)
        return out.cpu().numpy().reshape(-1).view(MS_FCCH_DTYPE)

    def ms_fcch_search(self, iq, min_score=None, rx_full_scale=2047.0, buf_len=None, stream=None):
        """The FCCH search with no clock (trxhip_ms_fcch_search_*): iq int16[n, stride, 2] or complex64[n, stride], row r searched
        over its first buf_len samples (default: the whole row) for the 576-sample window that looks most like a tone, and
        gsm_fcch_offset() measured on the slot that begins there.  Returns (hits uint8[n, 64], fcch uint8[n, 32]) device tensors
        (MS_FCCH_HIT_DTYPE / MS_FCCH_DTYPE rows: fsearch_to_numpy()); does not wait."""
        torch = self.torch
        if iq.dtype == torch.int16 and iq.dim() == 3 and iq.shape[-1] == 2:
            i16 = True
        elif iq.dtype == torch.complex64 and iq.dim() == 2:
            i16 = False
        else:
            raise TrxHipError(f"iq must be int16[n, stride, 2] or complex64[n, stride], not {iq.dtype}{list(iq.shape)}")
        assert iq.is_contiguous()
        n, stride = int(iq.shape[0]), int(iq.shape[1])
        length = stride if buf_len is None else int(buf_len)
        hits = torch.empty((n, MS_FCCH_HIT_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        fcch = torch.empty((n, MS_FCCH_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        fn, name = (self.L.trxhip_ms_fcch_search_i16, "trxhip_ms_fcch_search_i16") if i16 else \
            (self.L.trxhip_ms_fcch_search_cf32, "trxhip_ms_fcch_search_cf32")
        _check(fn(self.h, self._dev(iq), stride, length, n, MS_FSEARCH_MIN_SCORE if min_score is None else min_score, rx_full_scale,
                  self._dev(hits), self._dev(fcch), self._stream(stream)), name)
        return hits, fcch

    @staticmethod
    def fsearch_to_numpy(hits, fcch):
        """(MS_FCCH_HIT_DTYPE[n], MS_FCCH_DTYPE[n]) of ms_fcch_search()'s tensors; synchronises"""
        return hits.cpu().numpy().reshape(-1).view(MS_FCCH_HIT_DTYPE), fcch.cpu().numpy().reshape(-1).view(MS_FCCH_DTYPE)

    def ms_nco(self, rows, phase0, inc, stream=None):
        """The NCO alone (trxhip_ms_nco_batch_*): rows int16[n, len, 2] or complex64[n, len], row r rotated by the phase
        phase0[r] + i * inc[r] at sample i (uint32 / int32, one value or one per row), no scale.  Returns a complex64[n, len]
        device tensor; does not wait."""
        torch = self.torch
        if rows.dtype == torch.int16 and rows.dim() == 3 and rows.shape[-1] == 2:
            i16 = True
        elif rows.dtype == torch.complex64 and rows.dim() == 2:
            i16 = False
        else:
            raise TrxHipError(f"rows must be int16[n, len, 2] or complex64[n, len], not {rows.dtype}{list(rows.shape)}")
        assert rows.is_contiguous()
        n, length = int(rows.shape[0]), int(rows.shape[1])
        rec = np.zeros(n, dtype=MS_NCO_ROW_DTYPE)
        rec["phase0"] = np.asarray(phase0, dtype=np.uint64) & 0xFFFFFFFF
        rec["inc"] = inc
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(n, 8)).to(rows.device)
        out = torch.empty((n, length), dtype=torch.complex64, device=rows.device)
        fn, name = (self.L.trxhip_ms_nco_batch_i16, "trxhip_ms_nco_batch_i16") if i16 else \
            (self.L.trxhip_ms_nco_batch_cf32, "trxhip_ms_nco_batch_cf32")
        _check(fn(self.h, self._dev(rows), length, self._dev(d_rec), self._dev(out), length, n, length, self._stream(stream)), name)
        self._nco_rec = d_rec                                # (kept alive until the next call: the launch reads it)
        return out

    @staticmethod
    def results_to_numpy(results):
        return results.cpu().numpy().view(RESULT_DTYPE).reshape(-1)

    def pack_trxd(self, results, soft, rssi_offset=0.0, stream=None):
        torch = self.torch
        n = results.shape[0]
        pkt = torch.empty((n, TRXD_RECORD_BYTES), dtype=torch.uint8, device=results.device)
        rc = self.L.trxhip_pack_trxd_batch(self.h, self._dev(results), self._dev(soft, torch.float32), soft.shape[1],
                                           self._dev(pkt), n, rssi_offset, self._stream(stream))
        _check(rc, "trxhip_pack_trxd_batch")
        return pkt

    def pack_trxd_wire(self, results, params, soft, meta, pkt_stride=160, rssi_offset=0.0, stream=None):
        """TRXD v0/v1 datagrams (proto_trxd.c:68-117).  results uint8[n, 32], params uint8[n, 8], soft float32[n, stride]
        (sliced), meta uint8[n, 8] (TRXD_META_DTYPE).  Returns (pkt uint8[n, pkt_stride], pkt_len int16[n])."""
        torch = self.torch
        n = results.shape[0]
        pkt = torch.empty((n, pkt_stride), dtype=torch.uint8, device=results.device)
        plen = torch.empty(n, dtype=torch.int16, device=results.device)
        rc = self.L.trxhip_pack_trxd_wire_batch(self.h, self._dev(results), self._dev(params), self._dev(soft, torch.float32),
                                                soft.shape[1], self._dev(meta), self._dev(pkt), pkt_stride, self._dev(plen), n,
                                                rssi_offset, self._stream(stream))
        _check(rc, "trxhip_pack_trxd_wire_batch")
        return pkt, plen

    # ---- arch kernels ---------------------------------------------------------------------------
    def convolve(self, x, h, start, length, complex_taps, stream=None):
        """x: complex64[n_vec, x_len], h: complex64[h_len] -> complex64[n_vec, length]"""
        torch = self.torch
        n_vec, x_len = x.shape
        y = torch.empty((n_vec, length), dtype=torch.complex64, device=x.device)
        fn = self.L.trxhip_convolve_complex_batch if complex_taps else self.L.trxhip_convolve_real_batch
        rc = fn(self.h, self._dev(x), x_len, self._dev(h), h.shape[0], self._dev(y), length, start, length, n_vec,
                self._stream(stream))
        _check(rc, "trxhip_convolve_batch")
        return y

    def energy_detect(self, iq_cf32, window, stream=None):
        torch = self.torch
        n, burst_len = iq_cf32.shape
        out = torch.empty(n, dtype=torch.float32, device=iq_cf32.device)
        _check(self.L.trxhip_energy_detect_batch_cf32(self.h, self._dev(iq_cf32), n, burst_len, window, self._dev(out),
                                                      self._stream(stream)), "trxhip_energy_detect_batch_cf32")
        return out

    def vector_slicer(self, src, stream=None):
        torch = self.torch
        out = torch.empty_like(src)
        _check(self.L.trxhip_vector_slicer(self.h, self._dev(out), self._dev(src, torch.float32), src.numel(),
                                           self._stream(stream)), "trxhip_vector_slicer")
        return out

    def convert_short_float(self, s, stream=None):
        torch = self.torch
        out = torch.empty(s.shape, dtype=torch.float32, device=s.device)
        _check(self.L.trxhip_convert_short_float(self.h, self._dev(out), self._dev(s, torch.int16), s.numel(),
                                                 self._stream(stream)), "trxhip_convert_short_float")
        return out

    def channelize(self, wide_iq, n_blocks, m=4, block_len=192, h_len=16, stream=None):
        """wide_iq: int16[n_blocks*block_len*m, 2] -> complex64[m, n_blocks*block_len]"""
        torch = self.torch
        out = torch.empty((m, n_blocks * block_len), dtype=torch.complex64, device=wide_iq.device)
        _check(self.L.trxhip_channelize_batch(self.h, self._dev(wide_iq, torch.int16), self._dev(out), n_blocks, m,
                                              block_len, h_len, self._stream(stream)), "trxhip_channelize_batch")
        return out

    def resample(self, x, p, q, stream=None):
        """x: complex64[n_chan, n_in] -> complex64[n_chan, n_in*p/q]"""
        torch = self.torch
        n_chan, n_in = x.shape
        n_out = n_in // q * p
        out = torch.empty((n_chan, n_out), dtype=torch.complex64, device=x.device)
        _check(self.L.trxhip_resample_batch(self.h, self._dev(x), self._dev(out), n_in, p, q, n_chan, n_in, n_out,
                                            self._stream(stream)), "trxhip_resample_batch")
        return out

    def synthesize(self, rows, n_blocks, m=4, block_len=192, h_len=16, stream=None):
        """Synthesis(m, block_len, h_len)::rotate over n_blocks blocks from zero history.  rows: complex64[m, >= n_blocks*block_len]
        (Synthesis::inputBuffer(c) = rows[c]) -> complex64[n_blocks*block_len*m], interleaved"""
        torch = self.torch
        out = torch.empty(n_blocks * block_len * m, dtype=torch.complex64, device=rows.device)
        _check(self.L.trxhip_synthesize_batch(self.h, self._dev(rows, torch.complex64), rows.shape[1], self._dev(out), n_blocks, m,
                                              block_len, h_len, self._stream(stream)), "trxhip_synthesize_batch")
        return out


RXFE_MULTI, RXFE_RESAMP = 0, 1                      # TRXHIP_RXFE_*
RXFE_PCHAN = {1: (0,), 2: (0, 3), 3: (1, 0, 3)}     # filterbank path of logical channel l (radioInterfaceMulti.cpp:92-124)


class RxFrontEnd:
    """Streaming receive front end with carried history (trxhip_rx_frontend_*).  chans=None: Channelizer(4, block_len, 16) +
    Resampler(p, q, 16) on all four filterbank channels, rows in physical order.  chans=1..3, mode "multi":
    RadioInterfaceMulti::pullBuffer, the active paths only, row l = logical channel l.  chans=1, mode "resamp":
    RadioInterfaceResamp::pullBuffer, int16 samples of one channel -> convert_short_float + Resampler(p, q, 16)."""

    def __init__(self, trx, block_len=192, p=65, q=48, chans=None, mode="multi"):
        self.trx = trx
        self.block_len, self.p, self.q = block_len, p, q
        self.chans = chans
        self.mode = {"multi": RXFE_MULTI, "resamp": RXFE_RESAMP}[mode]
        h = _VP()
        if chans is None:
            if self.mode != RXFE_MULTI:
                raise ValueError('mode "resamp" needs chans=1')
            _check(trx.L.trxhip_rx_frontend_create(trx.h, block_len, p, q, C.byref(h)), "trxhip_rx_frontend_create")
        else:
            _check(trx.L.trxhip_rx_frontend_create_chans(trx.h, self.mode, chans, block_len, p, q, C.byref(h)),
                   "trxhip_rx_frontend_create_chans")
        self.h = h
        self.rows = trx.L.trxhip_rx_frontend_rows(h)

    def reset(self, stream=None):
        _check(self.trx.L.trxhip_rx_frontend_reset(self.h, self.trx._stream(stream)), "trxhip_rx_frontend_reset")

    def seed(self, wide_prev, n_blocks_prev, stream=None):
        """Start mid-stream: wide_prev = the n_blocks_prev >= 1 blocks preceding the shard (trxhip_rx_frontend_seed)."""
        ptr = self.trx._dev(wide_prev, self.trx.torch.int16) if n_blocks_prev else None
        _check(self.trx.L.trxhip_rx_frontend_seed(self.h, ptr, n_blocks_prev, self.trx._stream(stream)), "trxhip_rx_frontend_seed")

    def pull(self, wide_iq, n_blocks, stream=None, out=None):
        """wide_iq: int16[n_blocks*block_len*4, 2] (mode "resamp": int16[n_blocks*block_len, 2]) -> complex64[rows,
        n_blocks*block_len*p/q] (written into `out` when given)"""
        torch = self.trx.torch
        n_out = n_blocks * self.block_len // self.q * self.p
        if out is None:
            out = torch.empty((self.rows, n_out), dtype=torch.complex64, device=wide_iq.device)
        elif tuple(out.shape) != (self.rows, n_out) or out.dtype != torch.complex64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous complex64[%d, n_out] tensor" % self.rows)
        _check(self.trx.L.trxhip_rx_frontend_pull(self.h, self.trx._dev(wide_iq, torch.int16), n_blocks, self.trx._dev(out),
                                                  n_out, self.trx._stream(stream)), "trxhip_rx_frontend_pull")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.trx.L.trxhip_rx_frontend_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


TXFE_MULTI, TXFE_RESAMP = 0, 1


class TxFrontEnd:
    """Streaming transmit front end with carried history (trxhip_tx_frontend_*).  mode "multi": RadioInterfaceMulti::pushBuffer
    (Resampler(p, q, 16, bw) per active filterbank path + Synthesis(4, block_len*p/q, 16)); mode "resamp":
    RadioInterfaceResamp::pushBuffer (Resampler(p, q, 16, bw) alone, chans = 1)."""

    def __init__(self, trx, chans=3, block_len=260, p=48, q=65, bw=1.0, mode="multi"):
        self.trx = trx
        self.mode = {"multi": TXFE_MULTI, "resamp": TXFE_RESAMP}[mode]
        self.chans, self.block_len, self.p, self.q = chans, block_len, p, q
        h = _VP()
        _check(trx.L.trxhip_tx_frontend_create(trx.h, self.mode, chans, block_len, p, q, float(bw), C.byref(h)),
               "trxhip_tx_frontend_create")
        self.h = h

    def out_len(self, n_blocks):
        """output samples of n_blocks blocks"""
        return n_blocks * self.block_len // self.q * self.p * (4 if self.mode == TXFE_MULTI else 1)

    def _rows(self, x):
        x = x if x.dim() == 2 else x.view(1, -1)
        assert x.shape[0] == self.chans, (x.shape, self.chans)
        return self.trx._dev(x, self.trx.torch.complex64), x.shape[1]

    def reset(self, stream=None):
        _check(self.trx.L.trxhip_tx_frontend_reset(self.h, self.trx._stream(stream)), "trxhip_tx_frontend_reset")

    def seed(self, x_prev, n_blocks_prev, stream=None):
        """Start mid-stream: x_prev = complex64[chans, >= n_blocks_prev*block_len], the blocks preceding the shard."""
        ptr, stride = self._rows(x_prev) if n_blocks_prev else (None, 0)
        _check(self.trx.L.trxhip_tx_frontend_seed(self.h, ptr, stride, n_blocks_prev, self.trx._stream(stream)),
               "trxhip_tx_frontend_seed")

    def push(self, x, n_blocks, cf32=True, s16_scale=None, stream=None):
        """x: complex64[chans, >= n_blocks*block_len] (logical channel l in row l; 1-D for one channel).
        Returns (complex64[out_len] or None, int16[out_len, 2] or None -- only with s16_scale)."""
        torch = self.trx.torch
        ptr, stride = self._rows(x)
        n = self.out_len(n_blocks)
        out = torch.empty(n, dtype=torch.complex64, device=x.device) if cf32 else None
        s16 = torch.empty((n, 2), dtype=torch.int16, device=x.device) if s16_scale is not None else None
        _check(self.trx.L.trxhip_tx_frontend_push(self.h, ptr, stride, n_blocks,
                                                  self.trx._dev(out) if out is not None else None,
                                                  self.trx._dev(s16) if s16 is not None else None,
                                                  float(s16_scale or 0.0), self.trx._stream(stream)), "trxhip_tx_frontend_push")
        return out, s16

    def close(self):
        if getattr(self, "h", None):
            self.trx.L.trxhip_tx_frontend_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FILLER_DUMMY, FILLER_ZERO = 0, 1                    # TRXHIP_FILLER_* (FillerType)
COMB_FILL, COMB_NONE, COMB_LOOPBACK = 0, 14, 15     # TRXHIP_COMB_* (Transceiver::ChannelCombination; I .. XIII = 1 .. 13)
TXS_SRC_ZERO, TXS_SRC_BURST, TXS_SRC_FILLER = 0, 1, 2
TX_PLAN_DTYPE = np.dtype([("id", "<i8"), ("fn", "<u4"), ("tn", "u1"), ("src", "u1"), ("reserved", "u1", 2)])
TX_SCHED_COUNTERS = ("tx_stale_bursts", "tx_unavailable_bursts", "tx_trxd_fn_repeated", "tx_trxd_fn_outoforder",
                     "tx_trxd_fn_skipped", "refused")


class _TxSchedCfg(C.Structure):
    _fields_ = [("chans", C.c_int32), ("sps", C.c_int32), ("filler", C.c_int32), ("queue_cap", C.c_int32),
                ("max_slots", C.c_uint64), ("full_scale", C.c_double)]


class TxScheduler:
    """Downlink burst scheduler (trxhip_tx_sched_*): TRXD datagrams in, each channel's transmit stream out.
    trx=None: a plan-only object (no GPU): render() only plans, plan() reads the plan back."""

    def __init__(self, trx=None, chans=1, sps=4, filler=FILLER_DUMMY, full_scale=1.0, queue_cap=256, max_slots=8 * 1024):
        self.trx = trx
        self.L = trx.L if trx is not None else load_library()
        self.chans, self.sps = chans, sps
        cfg = _TxSchedCfg(chans, sps, filler, queue_cap, max_slots, float(full_scale))
        h = _VP()
        _check(self.L.trxhip_tx_sched_create(trx.h if trx is not None else None, C.byref(cfg), C.byref(h)), "trxhip_tx_sched_create")
        self.h = h
        self._last = 0

    def _stream(self, stream):
        return self.trx._stream(stream) if self.trx is not None else None

    def set_clock(self, fn, tn):
        _check(self.L.trxhip_tx_sched_set_clock(self.h, fn, tn), "trxhip_tx_sched_set_clock")

    def clock(self):
        fn, tn = C.c_uint32(), _I()
        _check(self.L.trxhip_tx_sched_clock(self.h, C.byref(fn), C.byref(tn)), "trxhip_tx_sched_clock")
        return fn.value, tn.value

    def set_slot(self, chan, tn, comb):
        _check(self.L.trxhip_tx_sched_set_slot(self.h, chan, tn, comb), "trxhip_tx_sched_set_slot")

    def set_muted(self, chan, muted):
        _check(self.L.trxhip_tx_sched_set_muted(self.h, chan, int(bool(muted))), "trxhip_tx_sched_set_muted")

    def submit(self, chan, dgram):
        """dgram: bytes / uint8 array of one TRXD datagram.  Returns its submission id, or -1 when refused or dropped."""
        b = bytes(bytearray(dgram))
        buf = (C.c_ubyte * max(len(b), 1)).from_buffer_copy(b if b else b"\0")
        i = C.c_int64()
        _check(self.L.trxhip_tx_sched_submit(self.h, chan, buf, len(b), C.byref(i)), "trxhip_tx_sched_submit")
        return i.value

    def samples(self, n_slots, tn0=None):
        """samples of n_slots slots rendered from TN tn0 (default: the clock's)"""
        if self.sps == 4:
            return 625 * n_slots
        tn0 = self.clock()[1] if tn0 is None else tn0
        pre = lambda t: t * 156 + (t + 3) // 4      # noqa: E731
        t = tn0 + n_slots
        return (t // 8) * 1250 + pre(t % 8) - pre(tn0)

    def render(self, n_slots, cf32=True, s16_scales=None, stream=None, out=None):
        """Plan-only: plans n_slots slots, returns None.  Otherwise (complex64[chans, n] or None, int16[chans, n, 2] or None),
        n = the render's samples; out = a preallocated complex64[chans, >= n] row buffer (cf32 only)."""
        if self.trx is None:
            _check(self.L.trxhip_tx_sched_render(self.h, n_slots, None, 0, None, None, None), "trxhip_tx_sched_render")
            self._last = n_slots
            return None
        if not cf32 and out is None and s16_scales is None:
            raise TrxHipError("TxScheduler.render: no output (cf32=False and no s16_scales)")
        torch = self.trx.torch
        n = self.samples(n_slots)
        dev = f"cuda:{self.trx.device}"
        if out is None and cf32:
            out = torch.empty((self.chans, max(n, 1)), dtype=torch.complex64, device=dev)
        s16 = sc = None
        if s16_scales is not None:
            s16 = torch.empty((self.chans, max(n, 1), 2), dtype=torch.int16, device=dev)
            sc = (C.c_float * self.chans)(*[float(x) for x in s16_scales])
        stride = out.shape[1] if out is not None else s16.shape[1]
        _check(self.L.trxhip_tx_sched_render(self.h, n_slots, self.trx._dev(out) if out is not None else None, stride,
                                             self.trx._dev(s16) if s16 is not None else None, sc, self._stream(stream)),
               "trxhip_tx_sched_render")
        self._last = n_slots
        return (out[:, :n] if out is not None else None), (s16[:, :n] if s16 is not None else None)

    def render_frontend(self, n_slots, fe, cf32=True, s16_scale=None, stream=None):
        """Render through a TxFrontEnd: returns (n_blocks, n_carried, complex64[fe.out_len(n_blocks)] or None,
        int16[.., 2] or None)."""
        torch = self.trx.torch
        cap = fe.out_len((self.block_bound(n_slots, fe)))
        dev = f"cuda:{self.trx.device}"
        out = torch.empty(max(cap, 1), dtype=torch.complex64, device=dev) if cf32 else None
        s16 = torch.empty((max(cap, 1), 2), dtype=torch.int16, device=dev) if s16_scale is not None else None
        nb, nc = _SZ(), _SZ()
        _check(self.L.trxhip_tx_sched_render_frontend(self.h, n_slots, fe.h, self.trx._dev(out) if out is not None else None,
                                                      self.trx._dev(s16) if s16 is not None else None, float(s16_scale or 0.0),
                                                      cap, C.byref(nb), C.byref(nc), self._stream(stream)),
               "trxhip_tx_sched_render_frontend")
        self._last = n_slots
        n = fe.out_len(nb.value)
        return nb.value, nc.value, (out[:n] if out is not None else None), (s16[:n] if s16 is not None else None)

    def block_bound(self, n_slots, fe):
        """blocks a render_frontend of n_slots can write at most (the carried remainder is < block_len)"""
        return (fe.block_len - 1 + self.samples(n_slots)) // fe.block_len

    def plan(self, chan, n=None):
        """TX_PLAN_DTYPE[n] of the last render (default: all its slots)"""
        n = self._last if n is None else n
        a = np.zeros(n, dtype=TX_PLAN_DTYPE)
        _check(self.L.trxhip_tx_sched_plan(self.h, chan, a.ctypes.data_as(_VP), n), "trxhip_tx_sched_plan")
        return a

    def counters(self, chan):
        a = np.zeros(6, dtype=np.uint64)
        _check(self.L.trxhip_tx_sched_counters(self.h, chan, a.ctypes.data_as(_VP)), "trxhip_tx_sched_counters")
        return dict(zip(TX_SCHED_COUNTERS, (int(x) for x in a)))

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_tx_sched_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ULIND_OFF, ULIND_MUTED, ULIND_IDLE = 1, 2, 4         # TRXHIP_ULIND_*
RX_SCHED_WORK_HEAD = 640                             # TRXHIP_RX_SCHED_WORK_HEAD
UL_IND_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("type", "u1"), ("flags", "u1"), ("tsc", "u1"), ("rc", "<i4"), ("toa", "<f4"),
                         ("ci", "<f4"), ("rssi", "<f4"), ("noise_lev", "<f4"), ("nbits", "<u2"), ("reserved", "<u2")])
RX_PLAN_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("type", "u1"), ("max_toa", "<u2")])
RX_SCHED_COUNTERS = ("rx_empty_burst", "rx_clipping", "rx_no_burst_detected")
assert UL_IND_DTYPE.itemsize == 32 and RX_PLAN_DTYPE.itemsize == 8


class _RxSchedCfg(C.Structure):
    _fields_ = [("chans", C.c_int32), ("sps", C.c_int32), ("tsc", C.c_int32), ("ul_fn_offset", C.c_int32), ("ext_rach", C.c_int32),
                ("egprs", C.c_int32), ("flags", C.c_int32), ("threshold", C.c_float), ("full_scale", C.c_float),
                ("reserved", C.c_uint32), ("max_slots", C.c_uint64)]


class RxScheduler:
    """Uplink burst scheduler (trxhip_rx_sched_*): each channel's receive stream in, TRXD uplink datagrams and indication
    records out.  trx=None: a plan-only object (no GPU): pull(n_samples=...) only cuts and plans, plan() reads the plan back.
    sps=1: the reference's default receive rate, slots of 157 / 156 / 156 / 156 samples (trxhip_rx_sched_create_sps)."""

    def __init__(self, trx=None, chans=1, sps=4, tsc=0, ul_fn_offset=0, ext_rach=False, egprs=False, exact=False, threshold=4.0,
                 full_scale=32767.0, max_slots=8 * 1024, use_va=False):
        self.trx = trx
        self.L = trx.L if trx is not None else load_library()
        self.chans, self.full_scale = chans, float(full_scale)
        self.soft_stride = 444 if egprs else 148
        self.rssi_offset = [0.0] * chans
        cfg = _RxSchedCfg(chans, sps, tsc, ul_fn_offset, int(bool(ext_rach)), int(bool(egprs)),
                          (FLAG_EXACT_DEMOD if exact else 0) | (FLAG_USE_VA if use_va else 0), threshold, full_scale, 0, max_slots)
        h = _VP()
        create = self.L.trxhip_rx_sched_create_sps if sps == 1 else self.L.trxhip_rx_sched_create
        _check(create(trx.h if trx is not None else None, C.byref(cfg), C.byref(h)), "trxhip_rx_sched_create")
        self.h = h
        self._last = 0
        self.carried = 0             # samples per channel the last pull left in the remainder

    def set_clock(self, fn, tn):
        _check(self.L.trxhip_rx_sched_set_clock(self.h, fn, tn), "trxhip_rx_sched_set_clock")
        self.carried = 0

    def clock(self):
        fn, tn = C.c_uint32(), _I()
        _check(self.L.trxhip_rx_sched_clock(self.h, C.byref(fn), C.byref(tn)), "trxhip_rx_sched_clock")
        return fn.value, tn.value

    def set_slot(self, chan, tn, comb):
        _check(self.L.trxhip_rx_sched_set_slot(self.h, chan, tn, comb), "trxhip_rx_sched_set_slot")

    def set_handover(self, tn, ss, on=True):
        _check(self.L.trxhip_rx_sched_set_handover(self.h, tn, ss, int(bool(on))), "trxhip_rx_sched_set_handover")

    def set_muted(self, chan, muted):
        _check(self.L.trxhip_rx_sched_set_muted(self.h, chan, int(bool(muted))), "trxhip_rx_sched_set_muted")

    def set_trxd_version(self, chan, version):
        _check(self.L.trxhip_rx_sched_set_trxd_version(self.h, chan, version), "trxhip_rx_sched_set_trxd_version")

    def set_rssi_offset(self, chan, db):
        _check(self.L.trxhip_rx_sched_set_rssi_offset(self.h, chan, db), "trxhip_rx_sched_set_rssi_offset")
        self.rssi_offset[chan] = float(np.float32(db))

    def set_max_toa(self, nb=30, ab=63):
        _check(self.L.trxhip_rx_sched_set_max_toa(self.h, nb, ab), "trxhip_rx_sched_set_max_toa")

    def slots(self, n_samples):
        n = self.L.trxhip_rx_sched_slots(self.h, n_samples)
        if n < 0:
            _check(int(n), "trxhip_rx_sched_slots")
        return int(n)

    def pull(self, x=None, n_samples=None, pkt_stride=None, want_soft=False, stream=None):
        """x: int16[chans, n, 2] or complex64[chans, n] device tensor (one chunk of every channel; a 1-channel object also takes
        int16[n, 2] / complex64[n]); plan-only: n_samples.  Returns (n_slots, n_carried) for a plan-only object, otherwise
        (pkt uint8[chans, n_slots, pkt_stride], pkt_len int16[chans, n_slots], ind uint8[chans, n_slots, 32] (UL_IND_DTYPE),
        soft float32[chans, n_slots, 148 | 444] or None) device tensors."""
        ns, nc = _SZ(), _SZ()
        if self.trx is None:
            _check(self.L.trxhip_rx_sched_pull_s16(self.h, None, 0, n_samples, None, 0, None, None, None, 0, C.byref(ns), C.byref(nc),
                                                   None), "trxhip_rx_sched_pull_s16")
            self._last, self.carried = ns.value, nc.value
            return ns.value, nc.value
        torch = self.trx.torch
        s16 = x.dtype == torch.int16
        if x.dim() == (2 if s16 else 1):
            x = x.unsqueeze(0)
        assert x.shape[0] == self.chans and (x.dtype == torch.complex64 or (s16 and x.shape[2] == 2)), (x.shape, x.dtype)
        n_in = x.shape[1]
        n = self.slots(n_in)
        if pkt_stride is None:
            pkt_stride = 160 if self.soft_stride == 148 else 456
        dev = f"cuda:{self.trx.device}"
        pkt = torch.empty((self.chans, n, pkt_stride), dtype=torch.uint8, device=dev)
        plen = torch.empty((self.chans, n), dtype=torch.int16, device=dev)
        ind = torch.empty((self.chans, n, 32), dtype=torch.uint8, device=dev)
        soft = torch.empty((self.chans, n, self.soft_stride), dtype=torch.float32, device=dev) if want_soft else None
        fn = self.L.trxhip_rx_sched_pull_s16 if s16 else self.L.trxhip_rx_sched_pull_cf32
        _check(fn(self.h, self.trx._dev(x) if n_in else None, n_in, n_in, self.trx._dev(pkt), pkt_stride, self.trx._dev(plen),
                  self.trx._dev(ind), self.trx._dev(soft) if soft is not None else None, n, C.byref(ns), C.byref(nc),
                  self.trx._stream(stream)), "trxhip_rx_sched_pull")
        assert ns.value == n
        self._last, self.carried = n, nc.value
        return pkt, plen, ind, soft

    def slots_frontend(self, fe, n_blocks):
        """slots the next pull_frontend of n_blocks through fe will cut"""
        n = self.L.trxhip_rx_sched_slots_frontend(self.h, fe.h, n_blocks)
        if n < 0:
            _check(int(n), "trxhip_rx_sched_slots_frontend")
        return int(n)

    def pull_frontend(self, fe, wide_iq, n_blocks, pkt_stride=None, want_soft=False, stream=None, work=None):
        """The radio's samples through the RxFrontEnd fe (chans=1..3 "multi", or "resamp") and the cutter in one call
        (trxhip_rx_sched_pull_frontend): wide_iq as RxFrontEnd.pull takes it; returns what pull() returns.  work: a contiguous
        complex64[chans, >= RX_SCHED_WORK_HEAD + n_out] device tensor with an even row length (allocated when None)."""
        torch = self.trx.torch
        n_out = self.L.trxhip_rx_frontend_out_samples(fe.h, n_blocks)
        n = self.slots_frontend(fe, n_blocks)
        dev = f"cuda:{self.trx.device}"
        if work is None:
            work = torch.empty((self.chans, RX_SCHED_WORK_HEAD + n_out + (n_out & 1)), dtype=torch.complex64, device=dev)
        elif (work.dim() != 2 or work.shape[0] != self.chans or work.shape[1] < RX_SCHED_WORK_HEAD + n_out or work.shape[1] % 2 or
              work.dtype != torch.complex64 or not work.is_contiguous()):
            raise ValueError("work must be a contiguous complex64[%d, >= %d] tensor with an even row length"
                             % (self.chans, RX_SCHED_WORK_HEAD + n_out))
        if pkt_stride is None:
            pkt_stride = 160 if self.soft_stride == 148 else 456
        pkt = torch.empty((self.chans, n, pkt_stride), dtype=torch.uint8, device=dev)
        plen = torch.empty((self.chans, n), dtype=torch.int16, device=dev)
        ind = torch.empty((self.chans, n, 32), dtype=torch.uint8, device=dev)
        soft = torch.empty((self.chans, n, self.soft_stride), dtype=torch.float32, device=dev) if want_soft else None
        ns, nc = _SZ(), _SZ()
        _check(self.L.trxhip_rx_sched_pull_frontend(self.h, fe.h, self.trx._dev(wide_iq, torch.int16), n_blocks, self.trx._dev(work),
                                                    work.shape[1], self.trx._dev(pkt), pkt_stride, self.trx._dev(plen),
                                                    self.trx._dev(ind), self.trx._dev(soft) if soft is not None else None, n,
                                                    C.byref(ns), C.byref(nc), self.trx._stream(stream)),
               "trxhip_rx_sched_pull_frontend")
        assert ns.value == n
        self._last, self.carried = n, nc.value
        return pkt, plen, ind, soft

    def plan(self, chan, n=None):
        """RX_PLAN_DTYPE[n] of the last pull (default: all its slots)"""
        n = self._last if n is None else n
        a = np.zeros(n, dtype=RX_PLAN_DTYPE)
        _check(self.L.trxhip_rx_sched_plan(self.h, chan, a.ctypes.data_as(_VP), n), "trxhip_rx_sched_plan")
        return a

    def counters(self, chan):
        """waits for the pulls issued so far"""
        a = np.zeros(3, dtype=np.uint64)
        _check(self.L.trxhip_rx_sched_counters(self.h, chan, a.ctypes.data_as(_VP)), "trxhip_rx_sched_counters")
        return dict(zip(RX_SCHED_COUNTERS, (int(x) for x in a)))

    def noise_state(self, chan):
        """(ring float32[20], itr, mNoiseLev float32); waits for the pulls issued so far"""
        ring = np.zeros(20, dtype=np.float32)
        itr, lev = C.c_uint32(), C.c_float()
        _check(self.L.trxhip_rx_sched_noise_state(self.h, chan, ring.ctypes.data_as(_VP), C.byref(itr), C.byref(lev)),
               "trxhip_rx_sched_noise_state")
        return ring, itr.value, np.float32(lev.value)

    @staticmethod
    def ind_to_numpy(ind):
        """uint8[chans, n, 32] device tensor -> UL_IND_DTYPE[chans, n]"""
        a = ind.cpu().numpy()
        return a.view(UL_IND_DTYPE).reshape(a.shape[:-1])

    def ind_db(self, ind, chan):
        """bi->rssi and bi->noise (Transceiver.cpp:750-752) of UL_IND_DTYPE records of channel chan, as float64 arrays: the record's
        rssi (dBFS, the device's float, what the datagram's rssi byte is made from) + rssi_offset, and
        20 log10(rxFullScale / mNoiseLev) + rssi_offset in double from the record's noise_lev.  OFF and muted slots give 0 (bi is
        left as initialised, :697-699)."""
        ind = np.asarray(ind)
        sent = (ind["flags"] & (ULIND_OFF | ULIND_MUTED)) == 0
        off = self.rssi_offset[chan]
        with np.errstate(divide="ignore"):
            rssi = np.where(sent, ind["rssi"].astype(np.float64) + off, 0.0)
            noise = np.where(sent, 20.0 * np.log10(self.full_scale / ind["noise_lev"].astype(np.float64)) + off, 0.0)
        return rssi, noise

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_rx_sched_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MS_SCHED_NO_SCH = -(1 << 31)                         # TRXHIP_MS_SCHED_NO_SCH
MS_PLAN_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("kind", "u1"), ("flags", "u1"), ("reserved", "u1"), ("ts", "<i8"),
                          ("src_off", "<i4"), ("reserved2", "<u4")])
MS_SCHED_STATE_DTYPE = np.dtype([("to_skip", "<i8"), ("pending", "<i8"), ("first_sch_ts_start", "<i8"), ("carried", "<u4"),
                                 ("carried_cf32", "u1"), ("first_call", "u1"), ("tracking", "u1"), ("tsc", "u1"), ("active_tns", "u1"),
                                 ("clock_set", "u1"), ("reserved", "u1", (6,)), ("clock_jumps", "<u8"), ("pulls", "<u8"),
                                 ("slots", "<u8"), ("sch_slots", "<u8")])
assert MS_PLAN_DTYPE.itemsize == 24 and MS_SCHED_STATE_DTYPE.itemsize == 72
# MS-side receive gain control: trxhip_ms_agc_record / _status, TRXHIP_MS_AGC_*
MS_AGC_RAISE, MS_AGC_SEARCH = 0, 1
MS_AGC_RING = 8
RAISE = "RAISE"                                      # acquire_gated(): the buffer is below the gate, (RAISE, new_gain)
MS_AGC_RECORD_DTYPE = np.dtype([("slot", "<u8"), ("runmean", "<f4"), ("sum", "<f4"), ("old_gain", "<f4"), ("new_gain", "<f4"),
                                ("applied", "<u4"), ("reserved", "<u4")])
MS_AGC_STATE_DTYPE = np.dtype([("rx_gain", "<f4"), ("runmean", "<f4"), ("gain_check", "<u4"), ("enable", "u1"), ("reserved", "u1", (3,)),
                               ("slots", "<u8"), ("decisions", "<u8"), ("applied", "<u8"), ("n_records", "<u4"), ("reserved2", "<u4"),
                               ("ring", MS_AGC_RECORD_DTYPE, (MS_AGC_RING,))])
assert MS_AGC_RECORD_DTYPE.itemsize == 32 and MS_AGC_STATE_DTYPE.itemsize == 304


# MS-side FCCH frequency-offset measurement: trxhip_ms_fcch, trxhip_ms_afc_entry / _status, TRXHIP_MS_AFC_RING
MS_AFC_RING = 8
MS_FCCH_DTYPE = np.dtype([("hz", "<f4"), ("alpha_one", "<f4"), ("alpha_two", "<f4"), ("mag_one", "<f4"), ("mag_two", "<f4"),
                          ("energy", "<f4"), ("p", "<i2"), ("r", "i1"), ("s", "i1"), ("reserved", "<u4")])
MS_AFC_ENTRY_DTYPE = np.dtype([("fn", "<u4"), ("hz", "<f4"), ("mag_one", "<f4"), ("energy", "<f4")])
MS_AFC_STATE_DTYPE = np.dtype([("count", "<u8"), ("n_records", "<u4"), ("enable", "u1"), ("reserved", "u1", (3,)),
                               ("last", MS_FCCH_DTYPE), ("ring", MS_AFC_ENTRY_DTYPE, (MS_AFC_RING,))])
assert MS_FCCH_DTYPE.itemsize == 32 and MS_AFC_ENTRY_DTYPE.itemsize == 16 and MS_AFC_STATE_DTYPE.itemsize == 176


class _MsAfcCfg(C.Structure):
    _fields_ = [("enable", C.c_int32), ("reserved", C.c_int32), ("d_fcch", C.c_void_p)]


def _afc_cfg(enable, out):
    """trxhip_ms_afc_cfg from set_afc()'s arguments; out: a contiguous device uint8[rows, 32] tensor (MS_FCCH_DTYPE rows) or None"""
    if out is not None:
        assert out.is_cuda and out.is_contiguous() and out.dim() == 2 and out.shape[1] == MS_FCCH_DTYPE.itemsize and \
            out.element_size() == 1, (out.shape, out.dtype)
    return _MsAfcCfg(int(bool(enable)), 0, out.data_ptr() if out is not None else None)


def _afc_state_dict(a):
    """MS_AFC_STATE_DTYPE record -> dict; "last": the last record (MS_FCCH_DTYPE) or None, "ring": the last measurements,
    oldest first, as dicts"""
    d = {"count": int(a["count"]), "enable": bool(a["enable"]), "last": a["last"].copy() if a["count"] else None}
    d["ring"] = [{k: r[k].item() for k in ("fn", "hz", "mag_one", "energy")} for r in a["ring"][:int(a["n_records"])]]
    return d


# MS-side NCO: trxhip_ms_nco_row, trxhip_ms_nco_cfg / _status, TRXHIP_MS_FCCH_BIAS_HZ
MS_FCCH_BIAS_HZ = 25.0 / 3.0
MS_NCO_ROW_DTYPE = np.dtype([("phase0", "<u4"), ("inc", "<i4")])
MS_NCO_STATE_DTYPE = np.dtype([("enable", "u1"), ("reserved", "u1", (3,)), ("inc", "<i4"), ("acc", "<u4"), ("reserved2", "<u4"),
                               ("ts_ref", "<i8"), ("hz", "<f8")])
assert MS_NCO_ROW_DTYPE.itemsize == 8 and MS_NCO_STATE_DTYPE.itemsize == 32


class _MsNcoCfg(C.Structure):
    _fields_ = [("enable", C.c_int32), ("reserved", C.c_int32), ("hz", C.c_double)]


def nco_hz_from_fcch(hz):
    """The NCO setting that cancels a measured FCCH offset: -(hz - 25 / 3) -- a tone on the FCCH frequency reads +8.33 Hz"""
    return -(float(hz) - MS_FCCH_BIAS_HZ)


def nco_tx_hz(rx_nco_hz, dl_hz=None, ul_hz=None):
    """The uplink NCO setting (MsTxScheduler.set_nco) that goes with a receive NCO setting rx_nco_hz: -rx_nco_hz * (ul_hz / dl_hz).
    The receive NCO cancels the offset seen on the downlink carrier; the same oscillator error shows on the uplink with the
    opposite sign, scaled by the ratio of the carrier frequencies (1 when none are given)."""
    if (dl_hz is None) != (ul_hz is None):
        raise ValueError("give both carrier frequencies or neither")
    ratio = 1.0 if dl_hz is None else float(ul_hz) / float(dl_hz)
    return -float(rx_nco_hz) * ratio


def ms_nco_inc(hz):
    """trxhip_ms_nco_inc(): the phase increment per sample of a shift by hz; pure host.  |hz| > 500000 and NaN raise."""
    inc = C.c_int32()
    _check(load_library().trxhip_ms_nco_inc(hz, C.byref(inc)), "trxhip_ms_nco_inc")
    return inc.value


def ms_nco_phase(acc, ts_ref, inc, ts):
    """trxhip_ms_nco_phase(): acc + (ts - ts_ref) * inc modulo 2^32; pure host"""
    return int(load_library().trxhip_ms_nco_phase(acc & 0xFFFFFFFF, ts_ref, inc, ts))


def ms_nco_tables_host():
    """trxhip_ms_nco_tables_host(): (coarse float32[1024, 2], fine float32[1024, 2]) of (cos, sin) pairs; pure host"""
    a = np.zeros(4096, dtype=np.float32)
    _check(load_library().trxhip_ms_nco_tables_host(a.ctypes.data_as(_VP)), "trxhip_ms_nco_tables_host")
    return a[:2048].reshape(1024, 2).copy(), a[2048:].reshape(1024, 2).copy()


def _nco_state_dict(a):
    return {"enable": bool(a["enable"]), "inc": int(a["inc"]), "acc": int(a["acc"]), "ts_ref": int(a["ts_ref"]), "hz": float(a["hz"])}


# MS-side FCCH search: trxhip_ms_fcch_hit, TRXHIP_MS_FSEARCH_*
MS_FSEARCH_HOP, MS_FSEARCH_W, MS_FSEARCH_LAG = 16, 576, 8
MS_FSEARCH_MIN_SCORE = 0.44
MS_FCCH_HIT_DTYPE = np.dtype([("found", "<i4"), ("pos", "<u4"), ("score", "<f8"), ("ra_re", "<f8"), ("ra_im", "<f8"), ("rb_re", "<f8"),
                              ("rb_im", "<f8"), ("energy", "<f8"), ("reserved", "<u8")])
assert MS_FCCH_HIT_DTYPE.itemsize == 64


class _MsAgcCfg(C.Structure):
    _fields_ = [("enable", C.c_int32), ("rx_gain", C.c_float), ("d_level", C.c_void_p)]


def ms_agc_gate(level, rx_full_scale, rx_gain):
    """The level gate of search_for_sch() (ms/ms_rx_lower.cpp:333-347), pure host: (MS_AGC_SEARCH, rx_gain) when level >
    rxFullScale / 8 or rx_gain >= 60, else (MS_AGC_RAISE, rx_gain + 4)."""
    new = _F()
    rc = load_library().trxhip_ms_agc_gate(level, rx_full_scale, rx_gain, C.byref(new))
    if rc < 0:
        _check(rc, "trxhip_ms_agc_gate")
    return rc, new.value


def _agc_state_dict(a):
    """MS_AGC_STATE_DTYPE record -> dict; "ring": the last decisions, oldest first, as dicts"""
    d = {k: a[k].item() for k in ("rx_gain", "runmean", "gain_check", "slots", "decisions", "applied")}
    d["enable"] = bool(a["enable"])
    d["ring"] = [{k: r[k].item() for k in ("slot", "runmean", "sum", "old_gain", "new_gain", "applied")} for r in a["ring"][:int(a["n_records"])]]
    return d


class _MsSchedCfg(C.Structure):
    _fields_ = [("rx_full_scale", C.c_float), ("tsc", C.c_uint8), ("active_tns", C.c_uint8), ("tracking", C.c_uint8),
                ("reserved", C.c_uint8)]


class MsRxScheduler:
    """MS-side downlink slot scheduler (trxhip_ms_sched_*): the radio's sample stream in, burst indications and sbits out --
    ms_trx::grab_bursts() with its time_keeper and the SCH feedback on the cut.  trx=None: a plan-only object (no GPU):
    pull(n_samples=..., first_ts=...) only cuts and plans, the SCH starts come from feed_starts()."""

    def __init__(self, trx=None, rx_full_scale=2047.0, tsc=0, active_tns=0xFF, tracking=True):
        self.trx = trx
        self.L = trx.L if trx is not None else load_library()
        cfg = _MsSchedCfg(rx_full_scale, tsc, active_tns, int(bool(tracking)), 0)
        h = _VP()
        _check(self.L.trxhip_ms_sched_create(trx.h if trx is not None else None, C.byref(cfg), C.byref(h)), "trxhip_ms_sched_create")
        self.h = h
        self._last = 0
        self.carried = 0
        self.rx_full_scale = float(rx_full_scale)
        self._agc, self._levels, self._lv = False, False, None
        self._fcch = None

    def set_clock(self, fn, tn, ts=0):
        _check(self.L.trxhip_ms_sched_set_clock(self.h, fn, tn, ts), "trxhip_ms_sched_set_clock")
        self.carried = 0

    def clock(self):
        """(fn, tn, ts) of the last slot cut"""
        fn, tn, ts = C.c_uint32(), _I(), C.c_int64()
        _check(self.L.trxhip_ms_sched_clock(self.h, C.byref(fn), C.byref(tn), C.byref(ts)), "trxhip_ms_sched_clock")
        return fn.value, tn.value, ts.value

    def set_tsc(self, tsc):
        _check(self.L.trxhip_ms_sched_set_tsc(self.h, tsc), "trxhip_ms_sched_set_tsc")

    def set_active(self, tn_mask):
        _check(self.L.trxhip_ms_sched_set_active(self.h, tn_mask), "trxhip_ms_sched_set_active")

    def set_tracking(self, on):
        _check(self.L.trxhip_ms_sched_set_tracking(self.h, int(bool(on))), "trxhip_ms_sched_set_tracking")

    def feed_starts(self, starts):
        """plan-only: the `start` of the next SCH slots cut with tracking on (MS_SCHED_NO_SCH: not decoded)"""
        a = np.ascontiguousarray(starts, dtype=np.int32)
        _check(self.L.trxhip_ms_sched_feed_starts(self.h, a.ctypes.data_as(_VP), len(a)), "trxhip_ms_sched_feed_starts")

    def acquire(self, x=None, first_ts=0, result=None, stream=None):
        """handle_sch(true) on the buffer x (int16[n, 2] or complex64[n] device tensor).  Returns (found, SCH_SYNC_DTYPE record);
        waits for the result.  Plan-only: result is the record the receiver would have given, n the buffer's length."""
        rec = np.zeros(1, dtype=SCH_SYNC_DTYPE)
        if self.trx is None:
            rec[0] = result
            rc = self.L.trxhip_ms_sched_acquire_s16(self.h, None, 60000, first_ts, rec.ctypes.data_as(_VP), None)
        else:
            s16 = x.dtype == self.trx.torch.int16
            fn = self.L.trxhip_ms_sched_acquire_s16 if s16 else self.L.trxhip_ms_sched_acquire_cf32
            rc = fn(self.h, self.trx._dev(x), x.shape[0], first_ts, rec.ctypes.data_as(_VP), self.trx._stream(stream))
        if rc < 0:
            _check(rc, "trxhip_ms_sched_acquire")
        if rc == 1:
            self.carried = 0
        return bool(rc), rec[0]

    def acquire_afc(self, x=None, first_ts=0, min_score=None, stream=None):
        """Cold start (trxhip_ms_afc_sched_acquire_*): the FCCH search over the buffer x as received, one wait, set_nco(True,
        nco_hz_from_fcch(hz)) from its measurement where the burst is found, then acquire() through the NCO.  Returns (found,
        SCH_SYNC_DTYPE record or None where no FCCH was found, MS_FCCH_HIT_DTYPE record, MS_FCCH_DTYPE record).  A found FCCH
        with no SCH behind it leaves the NCO set: retry with acquire() on the next buffer."""
        rec = np.zeros(1, dtype=SCH_SYNC_DTYPE)
        hit, fc = np.zeros(1, dtype=MS_FCCH_HIT_DTYPE), np.zeros(1, dtype=MS_FCCH_DTYPE)
        score = MS_FSEARCH_MIN_SCORE if min_score is None else min_score
        if self.trx is None:                                 # a plan-only object has no samples: the library refuses
            rc = self.L.trxhip_ms_afc_sched_acquire_s16(self.h, None, 60000, first_ts, score, hit.ctypes.data_as(_VP),
                                                        fc.ctypes.data_as(_VP), rec.ctypes.data_as(_VP), None)
        else:
            s16 = x.dtype == self.trx.torch.int16
            fn = self.L.trxhip_ms_afc_sched_acquire_s16 if s16 else self.L.trxhip_ms_afc_sched_acquire_cf32
            rc = fn(self.h, self.trx._dev(x), x.shape[0], first_ts, score, hit.ctypes.data_as(_VP), fc.ctypes.data_as(_VP),
                    rec.ctypes.data_as(_VP), self.trx._stream(stream))
        if rc < 0:
            _check(rc, "trxhip_ms_afc_sched_acquire")
        if rc == 1:
            self.carried = 0
        return bool(rc), (rec[0] if hit[0]["found"] else None), hit[0], fc[0]

    # ---- receive gain control (trxhip_ms_agc_sched_*) ----
    def _agc_set(self, enable, rx_gain, lv):
        cfg = _MsAgcCfg(int(bool(enable)), rx_gain, lv.data_ptr() if lv is not None else None)
        _check(self.L.trxhip_ms_agc_sched_set(self.h, C.byref(cfg)), "trxhip_ms_agc_sched_set")

    def set_agc(self, enable, rx_gain, levels=False):
        """maybe_update_gain() (ms/ms_rx_lower.cpp:101-126) over every slot an int16 pull cuts, starting from rx_gain; levels:
        pull() also returns the slots' levels.  gain_check, runmean, the counters and the ring stay as they are."""
        self._agc, self._levels = bool(enable), bool(enable) and bool(levels) and self.trx is not None
        if not self._levels:
            self._lv = None
        self._agc_set(enable, rx_gain, self._lv)

    def agc_set_gain(self, rx_gain):
        _check(self.L.trxhip_ms_agc_sched_set_gain(self.h, rx_gain), "trxhip_ms_agc_sched_set_gain")

    def agc_state(self):
        """dict: rx_gain, runmean, gain_check, enable, slots, decisions, applied, ring (the last 8 decisions, oldest first);
        waits for the AGC work in flight"""
        a = np.zeros(1, dtype=MS_AGC_STATE_DTYPE)
        _check(self.L.trxhip_ms_agc_sched_state(self.h, a.ctypes.data_as(_VP)), "trxhip_ms_agc_sched_state")
        return _agc_state_dict(a[0])

    def feed_levels(self, levels):
        """plan-only: the levels of the next slots cut with gain control on"""
        a = np.ascontiguousarray(levels, dtype=np.float32)
        _check(self.L.trxhip_ms_agc_sched_feed_levels(self.h, a.ctypes.data_as(_VP), len(a)), "trxhip_ms_agc_sched_feed_levels")

    def _level_room(self, n):
        """the level array of the pulls holds n floats (a larger one is set with the gain as it stands: that waits)"""
        if self._lv is None or self._lv.numel() < n:
            self._lv = self.trx.torch.empty((max(n, 64),), dtype=self.trx.torch.float32, device=f"cuda:{self.trx.device}")
            self._agc_set(True, self.agc_state()["rx_gain"], self._lv)

    def acquire_gated(self, x, first_ts=0, rx_gain=None, stream=None):
        """search_for_sch()'s worker (ms/ms_rx_lower.cpp:333-347) on the int16[n, 2] buffer x: its level, one wait, the gate with
        rx_gain (default: the object's), then acquire()'s (found, record) -- or (RAISE, rx_gain + 4), nothing else touched."""
        lv = self.trx.ms_level(x.reshape(1, -1, 2), stream=stream)
        if stream is not None:
            stream.synchronize()
        level = lv.item()
        gain = self.agc_state()["rx_gain"] if rx_gain is None else rx_gain
        what, new = ms_agc_gate(level, self.rx_full_scale, gain)
        if what == MS_AGC_RAISE:
            return RAISE, new
        return self.acquire(x, first_ts, stream=stream)

    # ---- FCCH frequency-offset measurement (trxhip_ms_afc_sched_*) ----
    def set_afc(self, enable, out=None):
        """gsm_fcch_offset() (ms/sch.c:255-314) on every FCCH slot a pull cuts, ACTIVE or not.  out: a device uint8[rows, 32]
        tensor (MS_FCCH_DTYPE rows) whose row k receives slot k's record where slot k of a pull is an FCCH slot -- the caller gives
        it as many rows as its largest pull cuts slots (slots()); other rows are not touched.  The state stays as it is; waits for
        AFC work in flight.  A plan-only object refuses."""
        cfg = _afc_cfg(enable, out)
        _check(self.L.trxhip_ms_afc_sched_set(self.h, C.byref(cfg)), "trxhip_ms_afc_sched_set")
        self._fcch = out                                     # (kept alive while the object may write it)

    def afc_state(self):
        """dict: count (FCCH slots measured), enable, last (MS_FCCH_DTYPE record or None), ring (the last 8 {fn, hz, mag_one,
        energy}, oldest first); waits for the AFC work in flight"""
        a = np.zeros(1, dtype=MS_AFC_STATE_DTYPE)
        _check(self.L.trxhip_ms_afc_sched_state(self.h, a.ctypes.data_as(_VP)), "trxhip_ms_afc_sched_state")
        return _afc_state_dict(a[0])

    # ---- frequency correction (trxhip_ms_nco_sched_*) ----
    def set_nco(self, enable, hz=0.0):
        """The NCO in the receive path: every sample a pull or an acquire receives is rotated by the phase of its absolute
        timestamp, a shift by hz (+ = up; nco_hz_from_fcch() of a measured offset cancels it).  Acts at the object's clock; the
        phase stays continuous across a change.  Host state only: no wait."""
        cfg = _MsNcoCfg(int(bool(enable)), 0, hz)
        _check(self.L.trxhip_ms_nco_sched_set(self.h, C.byref(cfg)), "trxhip_ms_nco_sched_set")

    def nco_state(self):
        """dict: enable, inc, acc (the phase at ts_ref), ts_ref, hz"""
        a = np.zeros(1, dtype=MS_NCO_STATE_DTYPE)
        _check(self.L.trxhip_ms_nco_sched_state(self.h, a.ctypes.data_as(_VP)), "trxhip_ms_nco_sched_state")
        return _nco_state_dict(a[0])

    def slots(self, n_samples):
        n = self.L.trxhip_ms_sched_slots(self.h, n_samples)
        if n < 0:
            _check(int(n), "trxhip_ms_sched_slots")
        return int(n)

    def pull(self, x=None, first_ts=0, n_samples=None, want_bits=True, stream=None):
        """x: int16[n, 2] or complex64[n] device tensor, the chunk whose first sample has timestamp first_ts; plan-only:
        n_samples.  Returns (n_slots, n_carried) for a plan-only object, otherwise (ind uint8[n_slots, 32] (MS_IND_DTYPE),
        sbits int8[n_slots, 148] or None) device tensors; after set_agc(..., levels=True) a third: the slots' levels,
        float32[n_slots]."""
        ns, nc = _SZ(), _SZ()
        if self.trx is None:
            _check(self.L.trxhip_ms_sched_pull_s16(self.h, None, n_samples, first_ts, None, None, 0, C.byref(ns), C.byref(nc), None),
                   "trxhip_ms_sched_pull_s16")
            self._last, self.carried = ns.value, nc.value
            return ns.value, nc.value
        torch = self.trx.torch
        s16 = x.dtype == torch.int16
        assert x.dtype == torch.complex64 and x.dim() == 1 or (s16 and x.dim() == 2 and x.shape[1] == 2), (x.shape, x.dtype)
        n_in = x.shape[0]
        cap = self.slots(n_in)
        dev = f"cuda:{self.trx.device}"
        ind = torch.empty((max(cap, 1), MS_IND_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        bits = torch.empty((max(cap, 1), 148), dtype=torch.int8, device=dev) if want_bits else None
        if self._levels:
            self._level_room(cap)
        fn = self.L.trxhip_ms_sched_pull_s16 if s16 else self.L.trxhip_ms_sched_pull_cf32
        _check(fn(self.h, self.trx._dev(x), n_in, first_ts, self.trx._dev(ind), self.trx._dev(bits) if want_bits else None, cap,
                  C.byref(ns), C.byref(nc), self.trx._stream(stream)), "trxhip_ms_sched_pull")
        self._last, self.carried = ns.value, nc.value
        if self._levels:                                     # (a view of the object's level array: the next pull writes it again)
            return ind[:ns.value], (bits[:ns.value] if want_bits else None), self._lv[:ns.value]
        return ind[:ns.value], (bits[:ns.value] if want_bits else None)

    def plan(self, n=None):
        """MS_PLAN_DTYPE[n] of the last pull (default: all its slots)"""
        n = self._last if n is None else n
        a = np.zeros(n, dtype=MS_PLAN_DTYPE)
        _check(self.L.trxhip_ms_sched_plan(self.h, a.ctypes.data_as(_VP), n), "trxhip_ms_sched_plan")
        return a

    def state(self):
        """MS_SCHED_STATE_DTYPE record; waits for a correction in flight"""
        a = np.zeros(1, dtype=MS_SCHED_STATE_DTYPE)
        _check(self.L.trxhip_ms_sched_state(self.h, a.ctypes.data_as(_VP)), "trxhip_ms_sched_state")
        return a[0]

    @staticmethod
    def ind_to_numpy(ind):
        """uint8[n, 32] device tensor -> MS_IND_DTYPE[n]"""
        return ind.cpu().numpy().reshape(-1).view(MS_IND_DTYPE)

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_ms_sched_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MS_GROUP_MAX_MEMBERS = 4096                          # TRXHIP_MS_GROUP_MAX_MEMBERS
MS_GROUP_CHUNK_DTYPE = np.dtype([("d_in", "<u8"), ("n_samples", "<u8"), ("first_ts", "<i8")])   # trxhip_ms_group_chunk


def _per_member(v, n, what):
    if not isinstance(v, (list, tuple, np.ndarray)):
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError("%s: %d values for %d members" % (what, len(v), n))
    return v


class MsRxSchedulerGroup:
    """A group of MS-side downlink streams (trxhip_ms_group_*): n members, each what one MsRxScheduler is, whose pulls are cut
    and received as one step -- one table, one join launch, one receiver launch, at most two waits, whatever n is.  tsc,
    active_tns and tracking: one value for all members or one per member; rx_full_scale belongs to the group.  trx=None: a
    plan-only group."""

    def __init__(self, trx=None, n=1, rx_full_scale=2047.0, tsc=0, active_tns=0xFF, tracking=True):
        self.trx = trx
        self.L = trx.L if trx is not None else load_library()
        self.n = int(n)
        if self.n < 0:
            raise ValueError("n")
        cfgs = (_MsSchedCfg * max(self.n, 1))()
        for m, (t, a, k) in enumerate(zip(_per_member(tsc, self.n, "tsc"), _per_member(active_tns, self.n, "active_tns"),
                                          _per_member(tracking, self.n, "tracking"))):
            cfgs[m] = _MsSchedCfg(rx_full_scale, t, a, int(bool(k)), 0)
        h = _VP()
        _check(self.L.trxhip_ms_group_create(trx.h if trx is not None else None, rx_full_scale, self.n, C.cast(cfgs, _VP), C.byref(h)),
               "trxhip_ms_group_create")
        self.h = h
        self.n_slots = [0] * self.n                  # of each member's last pull
        self.carried = [0] * self.n
        self.rx_full_scale = float(rx_full_scale)
        self._levels, self._lv = [False] * self.n, None
        self._fcch = {}

    def set_clock(self, m, fn, tn, ts=0):
        _check(self.L.trxhip_ms_group_set_clock(self.h, m, fn, tn, ts), "trxhip_ms_group_set_clock")
        self.carried[m] = 0

    def clock(self, m):
        """(fn, tn, ts) of the last slot member m cut"""
        fn, tn, ts = C.c_uint32(), _I(), C.c_int64()
        _check(self.L.trxhip_ms_group_clock(self.h, m, C.byref(fn), C.byref(tn), C.byref(ts)), "trxhip_ms_group_clock")
        return fn.value, tn.value, ts.value

    def set_tsc(self, m, tsc):
        _check(self.L.trxhip_ms_group_set_tsc(self.h, m, tsc), "trxhip_ms_group_set_tsc")

    def set_active(self, m, tn_mask):
        _check(self.L.trxhip_ms_group_set_active(self.h, m, tn_mask), "trxhip_ms_group_set_active")

    def set_tracking(self, m, on):
        _check(self.L.trxhip_ms_group_set_tracking(self.h, m, int(bool(on))), "trxhip_ms_group_set_tracking")

    def feed_starts(self, m, starts):
        """plan-only: the `start` of the next SCH slots member m cuts with tracking on (MS_SCHED_NO_SCH: not decoded)"""
        a = np.ascontiguousarray(starts, dtype=np.int32)
        _check(self.L.trxhip_ms_group_feed_starts(self.h, m, a.ctypes.data_as(_VP), len(a)), "trxhip_ms_group_feed_starts")

    def acquire(self, members, bufs=None, first_ts=0, results=None, stream=None):
        """handle_sch(true) for the listed members in one launch and one wait.  bufs: int16[n, len, 2] or complex64[n, len] device
        tensor, row i the buffer of members[i]; first_ts: one timestamp or one per buffer.  Returns (found: bool[n], records:
        SCH_SYNC_DTYPE[n]).  Plan-only: results are the records the receiver would have given."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        n = len(members)
        ts = np.ascontiguousarray(_per_member(first_ts, n, "first_ts"), dtype=np.int64)
        rec = np.zeros(n, dtype=SCH_SYNC_DTYPE)
        found = np.zeros(n, dtype=np.int32)
        if self.trx is None:
            rec[:] = results
            rc = self.L.trxhip_ms_group_acquire_s16(self.h, members.ctypes.data_as(_VP), n, None, 60000, 60000, ts.ctypes.data_as(_VP),
                                                    rec.ctypes.data_as(_VP), found.ctypes.data_as(_VP), None)
        else:
            s16 = bufs.dtype == self.trx.torch.int16
            assert bufs.is_contiguous() and bufs.shape[0] == n and bufs.dim() == (3 if s16 else 2), (bufs.shape, bufs.dtype)
            fn = self.L.trxhip_ms_group_acquire_s16 if s16 else self.L.trxhip_ms_group_acquire_cf32
            rc = fn(self.h, members.ctypes.data_as(_VP), n, self.trx._dev(bufs), bufs.shape[1], bufs.shape[1], ts.ctypes.data_as(_VP),
                    rec.ctypes.data_as(_VP), found.ctypes.data_as(_VP), self.trx._stream(stream))
        if rc < 0:
            _check(rc, "trxhip_ms_group_acquire")
        for m, f in zip(members, found):
            if f:
                self.carried[int(m)] = 0
        return found.astype(bool), rec

    def acquire_afc(self, members, bufs=None, first_ts=0, min_score=None, stream=None):
        """Cold start for the listed members (trxhip_ms_afc_group_acquire_*): the FCCH search over all buffers as received in one
        call, one wait, set_nco() from its measurement for the members whose burst is found, then acquire() for exactly those.
        Returns (found bool[n]: the SCH, records SCH_SYNC_DTYPE[n] (zero where no FCCH was found), hits MS_FCCH_HIT_DTYPE[n],
        fcch MS_FCCH_DTYPE[n]); members without an FCCH are untouched."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        n = len(members)
        ts = np.ascontiguousarray(_per_member(first_ts, n, "first_ts"), dtype=np.int64)
        rec = np.zeros(n, dtype=SCH_SYNC_DTYPE)
        found = np.zeros(n, dtype=np.int32)
        hit, fc = np.zeros(n, dtype=MS_FCCH_HIT_DTYPE), np.zeros(n, dtype=MS_FCCH_DTYPE)
        score = MS_FSEARCH_MIN_SCORE if min_score is None else min_score
        out = (hit.ctypes.data_as(_VP), fc.ctypes.data_as(_VP), rec.ctypes.data_as(_VP), found.ctypes.data_as(_VP))
        if self.trx is None:                                 # a plan-only group has no samples: the library refuses
            rc = self.L.trxhip_ms_afc_group_acquire_s16(self.h, members.ctypes.data_as(_VP), n, None, 60000, 60000, ts.ctypes.data_as(_VP),
                                                        score, *out, None)
        else:
            s16 = bufs.dtype == self.trx.torch.int16
            assert bufs.is_contiguous() and bufs.shape[0] == n and bufs.dim() == (3 if s16 else 2), (bufs.shape, bufs.dtype)
            fn = self.L.trxhip_ms_afc_group_acquire_s16 if s16 else self.L.trxhip_ms_afc_group_acquire_cf32
            rc = fn(self.h, members.ctypes.data_as(_VP), n, self.trx._dev(bufs), bufs.shape[1], bufs.shape[1], ts.ctypes.data_as(_VP),
                    score, *out, self.trx._stream(stream))
        if rc < 0:
            _check(rc, "trxhip_ms_afc_group_acquire")
        for m, f in zip(members, found):
            if f:
                self.carried[int(m)] = 0
        return found.astype(bool), rec, hit, fc

    # ---- receive gain control (trxhip_ms_agc_group_*), per member ----
    def _agc_set(self, m, enable, rx_gain, lv):
        cfg = _MsAgcCfg(int(bool(enable)), rx_gain, lv.data_ptr() if lv is not None else None)
        _check(self.L.trxhip_ms_agc_group_set(self.h, m, C.byref(cfg)), "trxhip_ms_agc_group_set")

    def set_agc(self, m, enable, rx_gain, levels=False):
        """member m: maybe_update_gain() over every slot its int16 pulls cut, starting from rx_gain; levels: pull() also returns
        the member's levels.  Members are on or off independently."""
        self._levels[m] = bool(enable) and bool(levels) and self.trx is not None
        self._agc_set(m, enable, rx_gain, self._lv if self._levels[m] else None)

    def agc_set_gain(self, m, rx_gain):
        _check(self.L.trxhip_ms_agc_group_set_gain(self.h, m, rx_gain), "trxhip_ms_agc_group_set_gain")

    def agc_state(self, m):
        """member m's dict as MsRxScheduler.agc_state(); waits for the group's AGC work in flight"""
        a = np.zeros(1, dtype=MS_AGC_STATE_DTYPE)
        _check(self.L.trxhip_ms_agc_group_state(self.h, m, a.ctypes.data_as(_VP)), "trxhip_ms_agc_group_state")
        return _agc_state_dict(a[0])

    def feed_levels(self, m, levels):
        """plan-only: the levels of the next slots member m cuts with gain control on"""
        a = np.ascontiguousarray(levels, dtype=np.float32)
        _check(self.L.trxhip_ms_agc_group_feed_levels(self.h, m, a.ctypes.data_as(_VP), len(a)), "trxhip_ms_agc_group_feed_levels")

    def _level_room(self, n):
        """the group-wide level array holds n floats (a larger one is set on every member that returns levels, with its gain
        as it stands: that waits)"""
        if self._lv is None or self._lv.numel() < n:
            self._lv = self.trx.torch.empty((max(n, 64),), dtype=self.trx.torch.float32, device=f"cuda:{self.trx.device}")
            for m in range(self.n):
                if self._levels[m]:
                    self._agc_set(m, True, self.agc_state(m)["rx_gain"], self._lv)

    def acquire_gated(self, members, bufs, first_ts=0, rx_gain=None, stream=None):
        """The level gate in front of acquire(), int16 buffers: the levels of all buffers in one launch, one wait, the gate per member
        with rx_gain (one value, one per buffer, or None: the members' own), then acquire() for the members that pass.  Returns
        (found bool[n], records SCH_SYNC_DTYPE[n], new_gain: None where the member searched, else the raised gain, nothing of
        that member touched)."""
        members = [int(m) for m in members]
        n = len(members)
        lv = self.trx.ms_level(bufs, stream=stream)
        if stream is not None:
            stream.synchronize()
        lv = lv.cpu().numpy()
        gains = [self.agc_state(m)["rx_gain"] for m in members] if rx_gain is None else _per_member(rx_gain, n, "rx_gain")
        ts = _per_member(first_ts, n, "first_ts")
        gate = [ms_agc_gate(float(lv[i]), self.rx_full_scale, gains[i]) for i in range(n)]
        go = [i for i in range(n) if gate[i][0] == MS_AGC_SEARCH]
        found, rec = np.zeros(n, dtype=bool), np.zeros(n, dtype=SCH_SYNC_DTYPE)
        if go:
            sub = bufs if len(go) == n else bufs[go].contiguous()
            f, r = self.acquire([members[i] for i in go], sub, [ts[i] for i in go], stream=stream)
            found[go], rec[go] = f, r
        return found, rec, [None if gate[i][0] == MS_AGC_SEARCH else gate[i][1] for i in range(n)]

    # ---- FCCH frequency-offset measurement (trxhip_ms_afc_group_*), per member ----
    def set_afc(self, m, enable, out=None):
        """member m: gsm_fcch_offset() on every FCCH slot its pulls cut.  out: a device uint8[n * out_stride, 32] tensor
        (MS_FCCH_DTYPE rows) for pulls with that out_stride: slot k of member m goes to row m * out_stride + k where it is an FCCH
        slot; a group passes one array to all its members.  Members are on or off independently."""
        cfg = _afc_cfg(enable, out)
        _check(self.L.trxhip_ms_afc_group_set(self.h, m, C.byref(cfg)), "trxhip_ms_afc_group_set")
        self._fcch[m] = out                                  # (kept alive while the group may write it)

    def afc_state(self, m):
        """member m's dict as MsRxScheduler.afc_state(); waits for the group's AFC work in flight"""
        a = np.zeros(1, dtype=MS_AFC_STATE_DTYPE)
        _check(self.L.trxhip_ms_afc_group_state(self.h, m, a.ctypes.data_as(_VP)), "trxhip_ms_afc_group_state")
        return _afc_state_dict(a[0])

    # ---- frequency correction (trxhip_ms_nco_group_*), per member ----
    def set_nco(self, m, enable, hz=0.0):
        """member m's NCO as MsRxScheduler.set_nco(); members are on or off independently"""
        cfg = _MsNcoCfg(int(bool(enable)), 0, hz)
        _check(self.L.trxhip_ms_nco_group_set(self.h, m, C.byref(cfg)), "trxhip_ms_nco_group_set")

    def nco_state(self, m):
        """member m's dict as MsRxScheduler.nco_state()"""
        a = np.zeros(1, dtype=MS_NCO_STATE_DTYPE)
        _check(self.L.trxhip_ms_nco_group_state(self.h, m, a.ctypes.data_as(_VP)), "trxhip_ms_nco_group_state")
        return _nco_state_dict(a[0])

    def slots(self, m, n_samples):
        n = self.L.trxhip_ms_group_slots(self.h, m, n_samples)
        if n < 0:
            _check(int(n), "trxhip_ms_group_slots")
        return int(n)

    def pull(self, chunks=None, first_ts=0, out_stride=None, bits=True, stream=None, out=None, n_samples=None):
        """chunks: per member an int16[n, 2] or complex64[n] device tensor (all of one format) or None (no chunk in this pull);
        first_ts: one timestamp or one per member.  Returns ([(ind uint8[k, 32], sbits int8[k, 148] or None) per member], [k per
        member]): views of outputs with out_stride rows per member (default: the largest trxhip_ms_group_slots() of the pull), or
        of out = (ind uint8[n, out_stride, 32], sbits int8[n, out_stride, 148] or None).  Plan-only: n_samples per member (0 or
        None: no chunk); returns ([n_slots], [n_carried]).  A plan-only group given an out_stride other than None / 0 refuses a
        pull in which a member would cut more slots than that, as the GPU group does; the plan-only MsRxScheduler has no such
        bound (it takes no outputs), and neither has the group with out_stride None / 0.  Where a member returns levels
        (set_agc(m, ..., levels=True)) a third list follows: per member float32[k] levels, or None."""
        ts = _per_member(first_ts, self.n, "first_ts")
        ch = np.zeros(self.n, dtype=MS_GROUP_CHUNK_DTYPE)
        ns, nc = (_SZ * self.n)(), (_SZ * self.n)()
        bad = _I(-1)
        if self.trx is None:
            sizes = _per_member(n_samples, self.n, "n_samples")
            for m in range(self.n):
                ch[m] = (0, sizes[m] or 0, ts[m])
            rc = self.L.trxhip_ms_group_pull_s16(self.h, ch.ctypes.data_as(_VP), None, None, int(out_stride or 0), C.cast(ns, _VP), C.cast(nc, _VP),
                                                 C.byref(bad), None)
            self.bad_member = bad.value
            _check(rc, "trxhip_ms_group_pull_s16 (member %d)" % bad.value)
            self.n_slots, self.carried = list(ns), list(nc)
            return list(ns), list(nc)
        torch = self.trx.torch
        chunks = _per_member(chunks, self.n, "chunks") if isinstance(chunks, (list, tuple)) else [chunks] * self.n
        have = [x for x in chunks if x is not None]
        if not have:
            raise ValueError("no member has a chunk")
        s16 = have[0].dtype == torch.int16
        cap = 1
        for m, x in enumerate(chunks):
            if x is None:
                continue
            assert x.dtype == have[0].dtype and x.is_contiguous(), (m, x.dtype)
            assert x.dtype == torch.complex64 and x.dim() == 1 or (s16 and x.dim() == 2 and x.shape[1] == 2), (x.shape, x.dtype)
            ch[m] = (x.data_ptr(), x.shape[0], ts[m])
            if out_stride is None and out is None:
                cap = max(cap, self.slots(m, x.shape[0]))
        dev = f"cuda:{self.trx.device}"
        if out is not None:
            ind, sb = out
            stride = ind.shape[1]
            assert ind.is_contiguous() and tuple(ind.shape) == (self.n, stride, MS_IND_DTYPE.itemsize) and ind.dtype == torch.uint8
            assert sb is None or (sb.is_contiguous() and tuple(sb.shape) == (self.n, stride, 148) and sb.dtype == torch.int8)
        else:
            stride = cap if out_stride is None else int(out_stride)
            ind = torch.empty((self.n, max(stride, 1), MS_IND_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            sb = torch.empty((self.n, max(stride, 1), 148), dtype=torch.int8, device=dev) if bits else None
        if any(self._levels):
            self._level_room(self.n * max(stride, 1))
        fn = self.L.trxhip_ms_group_pull_s16 if s16 else self.L.trxhip_ms_group_pull_cf32
        rc = fn(self.h, ch.ctypes.data_as(_VP), self.trx._dev(ind), self.trx._dev(sb) if sb is not None else None, stride,
                C.cast(ns, _VP), C.cast(nc, _VP), C.byref(bad), self.trx._stream(stream))
        self.bad_member = bad.value
        _check(rc, "trxhip_ms_group_pull (member %d)" % bad.value)
        self.n_slots, self.carried = list(ns), list(nc)
        res = [(ind[m, :k], sb[m, :k] if sb is not None else None) for m, k in enumerate(self.n_slots)]
        if any(self._levels):                                # (views of the group's level array: the next pull writes it again)
            return res, list(self.n_slots), [self._lv[m * stride:m * stride + k] if self._levels[m] else None
                                             for m, k in enumerate(self.n_slots)]
        return res, list(self.n_slots)

    def plan(self, m, n=None):
        """MS_PLAN_DTYPE[n] of member m's last pull (default: all its slots)"""
        if n is None:
            n = self.n_slots[m]
        a = np.zeros(n, dtype=MS_PLAN_DTYPE)
        _check(self.L.trxhip_ms_group_plan(self.h, m, a.ctypes.data_as(_VP), n), "trxhip_ms_group_plan")
        return a

    def state(self, m):
        """MS_SCHED_STATE_DTYPE record of member m; waits for the group's corrections in flight"""
        a = np.zeros(1, dtype=MS_SCHED_STATE_DTYPE)
        _check(self.L.trxhip_ms_group_state(self.h, m, a.ctypes.data_as(_VP)), "trxhip_ms_group_state")
        return a[0]

    ind_to_numpy = staticmethod(MsRxScheduler.ind_to_numpy)

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_ms_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the MS-side uplink burst scheduler: trxhip_ms_tx_req / _plan / _status, TRXHIP_MS_TX_*
MS_TX_QUEUED, MS_TX_LATE, MS_TX_WRAPPED, MS_TX_EXPIRED, MS_TX_OVERLAP, MS_TX_FULL = range(6)
MS_TX_REQ_DTYPE = np.dtype([("fn", "<u4"), ("tn", "u1"), ("pwr", "u1"), ("reserved", "u1", (2,)), ("bits", "u1", (148,))])
MS_TX_PLAN_DTYPE = np.dtype([("send_ts", "<i8"), ("radio_ts", "<i8"), ("diff_fn", "<i4"), ("diff_tn", "<i4"), ("scale", "<f4"),
                             ("status", "<i4")])
MS_TX_STATE_DTYPE = np.dtype([("submitted", "<u8"), ("queued", "<u8"), ("late", "<u8"), ("wrapped", "<u8"), ("expired", "<u8"),
                              ("overlap", "<u8"), ("full", "<u8"), ("drawn", "<u8"), ("missed", "<u8"), ("pending", "<u8"),
                              ("rendered_end", "<i8"), ("timing_advance", "<i4"), ("window_set", "u1"), ("reserved", "u1", (3,))])
assert MS_TX_REQ_DTYPE.itemsize == 156 and MS_TX_PLAN_DTYPE.itemsize == 32 and MS_TX_STATE_DTYPE.itemsize == 96


def ms_tx_requests(fn, tn, pwr, bits):
    """MS_TX_REQ_DTYPE[n] from fn, tn, pwr (scalars or n values each) and bits uint8[n, 148] (or [148]: one request)"""
    bits = np.asarray(bits, dtype=np.uint8).reshape(-1, 148)
    r = np.zeros(len(bits), dtype=MS_TX_REQ_DTYPE)
    r["fn"], r["tn"], r["pwr"], r["bits"] = fn, tn, pwr, bits
    return r


class _MsTxCfg(C.Structure):
    _fields_ = [("tx_full_scale", C.c_uint32), ("rxtx_delay", C.c_int32), ("max_pending", C.c_uint32), ("reserved", C.c_uint32)]


class MsTxScheduler:
    """MS-side uplink burst scheduler (trxhip_ms_tx_*): burst requests in, the radio's int16 transmit stream out --
    driveTx()'s scale and ms_trx::submit_burst()'s timestamp arithmetic, then a render of any window of the stream.
    trx=None: a plan-only object (no GPU): submit, plan, window and counters; render draws nothing."""

    def __init__(self, trx=None, tx_full_scale=2047, rxtx_delay=0, max_pending=1024):
        self.trx = trx
        self.L = trx.L if trx is not None else load_library()
        cfg = _MsTxCfg(tx_full_scale, rxtx_delay, max_pending, 0)
        h = _VP()
        _check(self.L.trxhip_ms_tx_create(trx.h if trx is not None else None, C.byref(cfg), C.byref(h)), "trxhip_ms_tx_create")
        self.h = h

    def set_ta(self, val):
        _check(self.L.trxhip_ms_tx_set_ta(self.h, val), "trxhip_ms_tx_set_ta")

    def submit(self, reqs, clock, stream=None):
        """reqs: MS_TX_REQ_DTYPE[n] (ms_tx_requests()); clock: the timekeeper's (fn, tn, ts), MsRxScheduler.clock().
        Returns the plan, MS_TX_PLAN_DTYPE[n]."""
        reqs = np.ascontiguousarray(reqs, dtype=MS_TX_REQ_DTYPE).reshape(-1)
        plan = np.zeros(len(reqs), dtype=MS_TX_PLAN_DTYPE)
        fn, tn, ts = clock
        _check(self.L.trxhip_ms_tx_submit(self.h, reqs.ctypes.data_as(_VP), len(reqs), fn, tn, ts, plan.ctypes.data_as(_VP),
                                          self.trx._stream(stream) if self.trx is not None else None), "trxhip_ms_tx_submit")
        return plan

    def render(self, n_samples, first_ts, out=None, stream=None):
        """samples [first_ts, first_ts + n_samples) of the uplink stream.  Returns (int16[n_samples, 2] device tensor, n_drawn);
        out: an int16 device tensor of at least n_samples (I, Q) pairs to write instead.  Plan-only: (None, n_drawn)."""
        nd = _SZ()
        if self.trx is None:
            _check(self.L.trxhip_ms_tx_render_s16(self.h, None, n_samples, first_ts, C.byref(nd), None), "trxhip_ms_tx_render_s16")
            return None, nd.value
        torch = self.trx.torch
        if out is None:
            out = torch.empty((max(n_samples, 1), 2), dtype=torch.int16, device=f"cuda:{self.trx.device}")
        assert out.dtype == torch.int16 and out.is_contiguous() and out.numel() >= 2 * n_samples, (out.shape, out.dtype)
        _check(self.L.trxhip_ms_tx_render_s16(self.h, out.data_ptr(), n_samples, first_ts, C.byref(nd), self.trx._stream(stream)),
               "trxhip_ms_tx_render_s16")
        return out, nd.value

    def state(self):
        """MS_TX_STATE_DTYPE record: the counters and the window state"""
        a = np.zeros(1, dtype=MS_TX_STATE_DTYPE)
        _check(self.L.trxhip_ms_tx_state(self.h, a.ctypes.data_as(_VP)), "trxhip_ms_tx_state")
        return a[0]

    # ---- uplink frequency correction (trxhip_ms_nco_tx_*) ----
    def set_nco(self, enable, hz=0.0):
        """The uplink NCO: every burst sample rendered from now on is rotated by a phase that depends only on its timestamp, a
        shift by hz (+ = up; nco_tx_hz() of the receive NCO's hz cancels the oscillator's error).  Acts at the end of the last
        rendered window, phase-continuous across a change; host state only, no GPU work.  |hz| > 500000 raises."""
        cfg = _MsNcoCfg(1 if enable else 0, 0, float(hz))
        _check(self.L.trxhip_ms_nco_tx_set(self.h, C.byref(cfg)), "trxhip_ms_nco_tx_set")

    def nco_state(self):
        """dict(enable, inc, acc, ts_ref, hz) as MsRxScheduler.nco_state(), on the radio_ts timeline of the windows"""
        a = np.zeros(1, dtype=MS_NCO_STATE_DTYPE)
        _check(self.L.trxhip_ms_nco_tx_state(self.h, a.ctypes.data_as(_VP)), "trxhip_ms_nco_tx_state")
        return _nco_state_dict(a[0])

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_ms_tx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MS_TX_GROUP_MAX_MEMBERS = 4096                       # TRXHIP_MS_TX_GROUP_MAX_MEMBERS
MS_TX_CLOCK_DTYPE = np.dtype([("fn", "<u4"), ("tn", "<i4"), ("ts", "<i8")])        # trxhip_ms_tx_clock
assert MS_TX_CLOCK_DTYPE.itemsize == 16


class _MsTxGroupCfg(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("tx_full_scale", C.c_uint32), ("rxtx_delay", C.c_int32), ("max_pending", C.c_uint32)]


class MsTxSchedulerGroup:
    """N MS-side uplink burst schedulers behind one radio type (trxhip_ms_tx_group_*): every member is a MsTxScheduler -- its own
    timing advance, queue, window state and counters -- and the group issues the members' submits as one copy and one launch and
    their renders as one table copy and one launch, whatever N is.
    trx=None: a plan-only group (no GPU): submit, plan, windows and counters; render draws nothing."""

    def __init__(self, trx=None, n_members=1, tx_full_scale=2047, rxtx_delay=0, max_pending=1024):
        self.trx = trx
        self.L = trx.L if trx is not None else load_library()
        self.n = int(n_members)
        cfg = _MsTxGroupCfg(self.n, tx_full_scale, rxtx_delay, max_pending)
        h = _VP()
        _check(self.L.trxhip_ms_tx_group_create(trx.h if trx is not None else None, C.byref(cfg), C.byref(h)), "trxhip_ms_tx_group_create")
        self.h = h
        self.bad = -1                                # of the last refused submit (a request) or render (a member)

    def set_ta(self, m, val):
        _check(self.L.trxhip_ms_tx_group_set_ta(self.h, m, val), "trxhip_ms_tx_group_set_ta")

    def submit(self, members, reqs, clocks, stream=None):
        """members: the member of each request (one index for all, or n); reqs: MS_TX_REQ_DTYPE[n] (ms_tx_requests()); clocks: per
        member its timekeeper's (fn, tn, ts), MsRxSchedulerGroup.clock(m) -- a sequence of n_members entries or a dict by member;
        None or a missing entry is fine for a member no request names.  Returns the plan, MS_TX_PLAN_DTYPE[n]."""
        reqs = np.ascontiguousarray(reqs, dtype=MS_TX_REQ_DTYPE).reshape(-1)
        members = np.ascontiguousarray(np.broadcast_to(np.asarray(members, dtype=np.uint32), (len(reqs),)))
        now = np.zeros(self.n, dtype=MS_TX_CLOCK_DTYPE)
        now["fn"] = 0xFFFFFFFF                       # not a clock: a request that names a member without one is refused
        for m, c in (clocks.items() if isinstance(clocks, dict) else enumerate(_per_member(list(clocks), self.n, "clocks"))):
            if c is not None:
                now[m] = tuple(c)
        plan = np.zeros(len(reqs), dtype=MS_TX_PLAN_DTYPE)
        bad = _SZ()
        rc = self.L.trxhip_ms_tx_group_submit(self.h, members.ctypes.data_as(_VP), reqs.ctypes.data_as(_VP), len(reqs),
                                              now.ctypes.data_as(_VP), plan.ctypes.data_as(_VP), C.byref(bad),
                                              self.trx._stream(stream) if self.trx is not None else None)
        self.bad = -1 if bad.value == _SZ(-1).value else bad.value
        _check(rc, "trxhip_ms_tx_group_submit (request %d)" % self.bad)
        return plan

    def render(self, n_samples, first_ts, out=None, out_stride=None, stream=None):
        """member m's window [first_ts[m], first_ts[m] + n_samples[m]); n_samples, first_ts: one value for all members or one per
        member, n_samples[m] == 0 (or None): m is not rendered.  Returns (int16[n_members, out_stride, 2] device tensor -- member
        m's window is [m, :n_samples[m]] --, [n_drawn per member]); out: such a tensor to write instead; out_stride: default the
        longest window.  Plan-only: (None, [n_drawn]); out_stride None / 0 leaves the window lengths unbounded."""
        ns = np.array([x or 0 for x in _per_member(n_samples, self.n, "n_samples")], dtype=np.uintp)
        ts = np.array(_per_member(first_ts, self.n, "first_ts"), dtype=np.int64)
        nd = np.zeros(self.n, dtype=np.uintp)
        bad = _I(-1)
        if self.trx is None:
            rc = self.L.trxhip_ms_tx_group_render_s16(self.h, None, int(out_stride or 0), ts.ctypes.data_as(_VP), ns.ctypes.data_as(_VP),
                                                      nd.ctypes.data_as(_VP), C.byref(bad), None)
            self.bad = bad.value
            _check(rc, "trxhip_ms_tx_group_render_s16 (member %d)" % bad.value)
            return None, [int(x) for x in nd]
        torch = self.trx.torch
        if out is None:
            stride = max(int(ns.max()), 1) if out_stride is None else int(out_stride)
            out = torch.empty((self.n, max(stride, 1), 2), dtype=torch.int16, device=f"cuda:{self.trx.device}")
        else:
            assert out.dtype == torch.int16 and out.is_contiguous() and out.dim() == 3 and out.shape[0] == self.n and out.shape[2] == 2, \
                (out.shape, out.dtype)
            stride = out.shape[1] if out_stride is None else int(out_stride)
            assert stride <= out.shape[1]
        rc = self.L.trxhip_ms_tx_group_render_s16(self.h, out.data_ptr(), stride, ts.ctypes.data_as(_VP), ns.ctypes.data_as(_VP),
                                                  nd.ctypes.data_as(_VP), C.byref(bad), self.trx._stream(stream))
        self.bad = bad.value
        _check(rc, "trxhip_ms_tx_group_render_s16 (member %d)" % bad.value)
        return out, [int(x) for x in nd]

    def state(self, m):
        """MS_TX_STATE_DTYPE record of member m: the counters and the window state"""
        a = np.zeros(1, dtype=MS_TX_STATE_DTYPE)
        _check(self.L.trxhip_ms_tx_group_state(self.h, m, a.ctypes.data_as(_VP)), "trxhip_ms_tx_group_state")
        return a[0]

    # ---- uplink frequency correction (trxhip_ms_nco_tx_group_*), per member ----
    def set_nco(self, m, enable, hz=0.0):
        """member m's uplink NCO as MsTxScheduler.set_nco(); members are on or off independently"""
        cfg = _MsNcoCfg(1 if enable else 0, 0, float(hz))
        _check(self.L.trxhip_ms_nco_tx_group_set(self.h, m, C.byref(cfg)), "trxhip_ms_nco_tx_group_set")

    def nco_state(self, m):
        """member m's dict as MsTxScheduler.nco_state()"""
        a = np.zeros(1, dtype=MS_NCO_STATE_DTYPE)
        _check(self.L.trxhip_ms_nco_tx_group_state(self.h, m, a.ctypes.data_as(_VP)), "trxhip_ms_nco_tx_group_state")
        return _nco_state_dict(a[0])

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_ms_tx_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


AIR_UL, AIR_DL = 0, 1                                # TRXHIP_AIR_UL, TRXHIP_AIR_DL
AIR_MAX_MEMBERS = 4096                               # TRXHIP_AIR_MAX_MEMBERS
AIR_MAX_DELAY = 65536                                # TRXHIP_AIR_MAX_DELAY
AIR_PATH_STATE_DTYPE = np.dtype([("gain", "<f4"), ("delay", "<u4"), ("hz", "<f8"), ("inc", "<i4"), ("acc", "<u4"), ("ts_ref", "<i8"),
                                 ("noise_scale", "<i4"), ("started", "<u4"), ("end_ts", "<i8")])
assert AIR_PATH_STATE_DTYPE.itemsize == 48
AIR_MAX_RAYS = 64                                    # TRXHIP_MULTIPATH_MAX_RAYS
AIR_RAY_DTYPE = np.dtype([("gain", "<f4"), ("delay", "<u4"), ("hz", "<f8"), ("phase", "<u4"), ("reserved", "<u4")])   # trxhip_multipath_ray
assert AIR_RAY_DTYPE.itemsize == 24
AIR_SAMPLE_HZ = 13e6 / 12.0


def air_rays(delays_us, powers_db, doppler_hz=0.0, sinusoids=1, seed=0, gain=1.0):
    """A tap-delay profile as AIR_RAY_DTYPE rays for AirChannel.set_rays; pure numpy, deterministic in seed.  Tap k lies
    delays_us[k] behind the first sample, rounded to whole samples of 13e6 / 12 Hz, at powers_db[k] relative to the others, and
    is `sinusoids` rays of equal gain: ray j of tap k at doppler_hz * cos(angle), angle = 2 pi (j + offset_k) / sinusoids with
    offset_k drawn from numpy.random.default_rng(seed), as its uint32 phase is.  The sum of gain_r^2 is gain^2.  The profile is
    the caller's: no standard tables are shipped."""
    delays = np.atleast_1d(np.asarray(delays_us, dtype=np.float64))
    powers = np.atleast_1d(np.asarray(powers_db, dtype=np.float64))
    sinusoids = int(sinusoids)
    if delays.shape != powers.shape or delays.ndim != 1 or len(delays) < 1 or sinusoids < 1 or (delays < 0).any() or \
            len(delays) * sinusoids > AIR_MAX_RAYS:
        raise ValueError("air_rays: 1 .. %d rays from matching 1-D delays (>= 0) and powers" % AIR_MAX_RAYS)
    rng = np.random.default_rng(seed)
    lin = 10.0 ** (powers / 10.0)
    tap_gain = float(gain) * np.sqrt(lin / lin.sum() / sinusoids)
    offset = rng.uniform(0.0, 1.0, size=len(delays))
    phase = rng.integers(0, 1 << 32, size=(len(delays), sinusoids), dtype=np.uint64)
    angle = 2.0 * np.pi * (np.arange(sinusoids)[None, :] + offset[:, None]) / sinusoids
    rays = np.zeros((len(delays), sinusoids), dtype=AIR_RAY_DTYPE)
    rays["gain"] = tap_gain[:, None]
    rays["delay"] = np.rint(delays * 1e-6 * AIR_SAMPLE_HZ).astype(np.uint32)[:, None]
    rays["hz"] = float(doppler_hz) * np.cos(angle)
    rays["phase"] = phase.astype(np.uint32)
    return rays.reshape(-1)


class _AirCfg(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("max_delay", C.c_uint32), ("seed", C.c_uint32), ("reserved", C.c_uint32)]


class _AirPath(C.Structure):
    _fields_ = [("gain", C.c_float), ("delay", C.c_uint32), ("hz", C.c_double)]


def air_noise_host(seed, lane, ts, scale=256):
    """nq of receiver lane `lane` at ts (trxhip_air_noise_host); scale = 256 returns s itself.  ts: any int, taken modulo 2^64"""
    ts = ((int(ts) + (1 << 63)) % (1 << 64)) - (1 << 63)
    return int(load_library().trxhip_air_noise_host(seed & 0xFFFFFFFF, lane, ts, scale))


class AirChannel:
    """The air interface (trxhip_air_*): n_members MSs and one BTS joined on the device.  uplink() sums the members' int16 rows --
    MsTxSchedulerGroup.render()'s tensor -- into the one stream RxScheduler.pull() takes; downlink() turns the one stream
    TxScheduler.render() writes into the members' rows MsRxSchedulerGroup.pull() takes.  Per path and direction a gain, a delay in
    whole samples (<= max_delay), a carrier offset and the receiver's noise; integer arithmetic behind one float stage, so the
    bytes do not depend on the grid or the chunking.  Windows of a direction are contiguous.  The object holds
    (n_members + 1) * max_delay * 4 bytes of history from creation on (1 GiB at 4096 members and 65536): ask for the largest
    delay the paths will use.
    set_rays() gives a path 1 .. AIR_MAX_RAYS rays instead (trxhip_multipath_*): each a gain, a delay, a carrier offset and a start
    phase, summed as integers -- echoes, Doppler, fading; air_rays() turns a tap-delay profile into them.
    trx=None: a host object -- numpy arrays in and out, the plain loop over the same arithmetic, no GPU."""

    def __init__(self, trx=None, n_members=1, max_delay=0, seed=0):
        self.trx = trx
        self.L = trx.L if trx is not None else load_library()
        self.n = int(n_members)
        if not 1 <= self.n <= AIR_MAX_MEMBERS or not 0 <= int(max_delay) <= AIR_MAX_DELAY:      # before a c_uint32 wraps them
            _check(-22, "trxhip_air_create (n_members %r, max_delay %r)" % (n_members, max_delay))
        cfg = _AirCfg(self.n, int(max_delay), seed & 0xFFFFFFFF, 0)
        h = _VP()
        _check(self.L.trxhip_air_create(trx.h if trx is not None else None, C.byref(cfg), C.byref(h)), "trxhip_air_create")
        self.h = h

    def set_path(self, dir, member, gain=1.0, delay=0, hz=0.0):
        """acts at the direction's end_ts: the phase stays continuous, gain and delay jump; hz = 0 is the identity rotation"""
        if not 0 <= int(member) < self.n or not 0 <= int(delay) <= AIR_MAX_DELAY:
            _check(-22, "trxhip_air_set_path (member %r, delay %r)" % (member, delay))
        p = _AirPath(float(gain), int(delay), float(hz))
        _check(self.L.trxhip_air_set_path(self.h, dir, member, C.byref(p)), "trxhip_air_set_path")

    def set_noise(self, dir, member, rms):
        """the rms, in int16 units, of member's receiver (AIR_DL) or of the BTS's (AIR_UL, member ignored)"""
        member = 0 if dir == AIR_UL else int(member)
        if not 0 <= member < self.n:
            _check(-22, "trxhip_air_set_noise (member %r)" % member)
        _check(self.L.trxhip_air_set_noise(self.h, dir, member, float(rms)), "trxhip_air_set_noise")

    def set_rays(self, dir, member, rays):
        """the path's rays (trxhip_multipath_set): an AIR_RAY_DTYPE array, or a list of dicts with gain, delay, hz, phase (the
        defaults of set_path, phase 0; phase is a uint32, 2^32 one turn).  Acts at the direction's end_ts, all or nothing.  None or
        an empty list clears them: the path is its plain state again"""
        if rays is None:
            rays = []
        if not isinstance(rays, np.ndarray):
            a = np.zeros(len(rays), dtype=AIR_RAY_DTYPE)
            for k, r in enumerate(rays):
                extra = set(r) - {"gain", "delay", "hz", "phase"}
                if extra or not 0 <= int(r.get("delay", 0)) <= AIR_MAX_DELAY or not 0 <= int(r.get("phase", 0)) < 1 << 32:
                    _check(-22, "trxhip_multipath_set (ray %d: %r)" % (k, r))
                a[k] = (r.get("gain", 1.0), int(r.get("delay", 0)), r.get("hz", 0.0), int(r.get("phase", 0)), 0)
            rays = a
        assert rays.dtype == AIR_RAY_DTYPE and rays.ndim == 1, (rays.dtype, rays.shape)
        rays = np.ascontiguousarray(rays)
        if not 0 <= int(member) < self.n or len(rays) > AIR_MAX_RAYS:
            _check(-22, "trxhip_multipath_set (member %r, %d rays)" % (member, len(rays)))
        _check(self.L.trxhip_multipath_set(self.h, dir, member, rays.ctypes.data_as(_VP) if len(rays) else None, len(rays)),
               "trxhip_multipath_set")

    def rays(self, dir, member):
        """(AIR_RAY_DTYPE array, ts_set): the path's rays with their phases at the direction's current end_ts, and the end_ts of
        the last set_rays.  set_rays(dir, member, rays(dir, member)[0]) changes no later byte"""
        if not 0 <= int(member) < self.n:
            _check(-22, "trxhip_multipath_state (member %r)" % member)
        a = np.zeros(AIR_MAX_RAYS, dtype=AIR_RAY_DTYPE)
        n, ts = C.c_uint32(0), C.c_int64(0)
        _check(self.L.trxhip_multipath_state(self.h, dir, member, a.ctypes.data_as(_VP), AIR_MAX_RAYS, C.byref(n), C.byref(ts)),
               "trxhip_multipath_state")
        return a[:n.value].copy(), ts.value

    def path_state(self, dir, member):
        """AIR_PATH_STATE_DTYPE record"""
        a = np.zeros(1, dtype=AIR_PATH_STATE_DTYPE)
        if not 0 <= int(member) < self.n:
            _check(-22, "trxhip_air_path_state (member %r)" % member)
        _check(self.L.trxhip_air_path_state(self.h, dir, member, a.ctypes.data_as(_VP)), "trxhip_air_path_state")
        return a[0]

    def reset(self, dir, ts):
        """forget the direction's past: its next window starts at ts"""
        _check(self.L.trxhip_air_reset(self.h, dir, ts), "trxhip_air_reset")

    def _out(self, shape, out):
        if self.trx is None:
            if out is None:
                out = np.empty(shape, dtype=np.int16)
            assert out.dtype == np.int16 and out.flags.c_contiguous and out.shape == shape, (out.shape, out.dtype)
            return out, out.ctypes.data
        torch = self.trx.torch
        if out is None:
            out = torch.empty(shape, dtype=torch.int16, device=f"cuda:{self.trx.device}")
        assert out.dtype == torch.int16 and out.is_contiguous() and tuple(out.shape) == shape, (out.shape, out.dtype)
        assert out.is_cuda and out.device.index == self.trx.device, out.device
        return out, out.data_ptr()

    def _in(self, x, dims):
        if self.trx is None:
            assert isinstance(x, np.ndarray) and x.dtype == np.int16 and x.flags.c_contiguous and x.ndim == dims and x.shape[-1] == 2, \
                (type(x), getattr(x, "shape", None))
            return x.ctypes.data
        assert x.dtype == self.trx.torch.int16 and x.is_contiguous() and x.dim() == dims and x.shape[-1] == 2, (x.shape, x.dtype)
        assert x.is_cuda and x.device.index == self.trx.device, x.device
        return x.data_ptr()

    def uplink(self, rows, first_ts, n=None, out=None, stream=None):
        """rows: int16[n_members, stride, 2], member m's window [first_ts, first_ts + n) in rows[m, :n] (n: default stride).
        Returns the BTS's int16[n, 2]; out: such an array to write instead"""
        p = self._in(rows, 3)
        assert rows.shape[0] == self.n, rows.shape
        n = rows.shape[1] if n is None else int(n)
        out, po = self._out((n, 2), out)
        _check(self.L.trxhip_air_uplink_s16(self.h, p, rows.shape[1], first_ts, n, po,
                                            self.trx._stream(stream) if self.trx is not None else None), "trxhip_air_uplink_s16")
        return out

    def downlink(self, x, first_ts, out=None, stream=None):
        """x: int16[n, 2], the BTS's window [first_ts, first_ts + n).  Returns int16[n_members, n, 2]; out: such an array to write
        instead"""
        p = self._in(x, 2)
        n = x.shape[0]
        out, po = self._out((self.n, n, 2), out)
        _check(self.L.trxhip_air_downlink_s16(self.h, p, first_ts, n, po, n, self.trx._stream(stream) if self.trx is not None else None),
               "trxhip_air_downlink_s16")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.trxhip_air_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _HostPipeCfg(C.Structure):
    _fields_ = [("max_bursts", C.c_uint32), ("depth", C.c_int32), ("burst_len", C.c_int32), ("sps", C.c_int32),
                ("soft_stride", C.c_int32), ("pkt_stride", C.c_int32), ("flags", C.c_int32), ("threshold", C.c_float),
                ("full_scale", C.c_float), ("rssi_offset", C.c_float), ("n_paths", C.c_int32)]


class _HostPipeSlot(C.Structure):
    _fields_ = [("iq", _VP), ("params", _VP), ("meta", _VP), ("results", _VP), ("soft", _VP), ("pkt", _VP), ("pkt_len", _VP)]


class HostPipe:
    """Host-fed, stream-pipelined hot path (trxhip_hostpipe_*): pinned staging slots, one stream each.

    slot(i) gives numpy views of slot i's pinned buffers; fill iq/params(/meta), submit(i, n), wait(i), read
    results/soft/pkt.  run() is the convenience form for ordinary numpy arrays."""

    def __init__(self, trx, max_bursts, depth=3, burst_len=625, sps=4, soft_stride=148, pkt_stride=0, flags=FLAG_SLICE,
                 threshold=4.0, full_scale=32767.0, rssi_offset=0.0, n_paths=1):
        self.trx = trx
        self.cfg = _HostPipeCfg(max_bursts, depth, burst_len, sps, soft_stride, pkt_stride, flags, threshold, full_scale,
                                rssi_offset, n_paths)
        h = _VP()
        _check(trx.L.trxhip_hostpipe_create(trx.h, C.byref(self.cfg), C.byref(h)), "trxhip_hostpipe_create")
        self.h = h
        self.depth = depth
        self._slots = [self._views(i) for i in range(depth)]

    def _views(self, i):
        s = _HostPipeSlot()
        _check(self.trx.L.trxhip_hostpipe_slot_buffers(self.h, i, C.byref(s)), "trxhip_hostpipe_slot_buffers")
        c = self.cfg
        n = c.max_bursts

        def view(ptr, nbytes, dtype, shape):
            if not ptr:
                return None
            buf = (C.c_ubyte * nbytes).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype).reshape(shape)
        return {
            "iq": (view(s.iq, n * c.burst_len * 4, np.int16, (n, c.burst_len, 2)) if c.n_paths <= 1 else
                   view(s.iq, n * c.n_paths * c.burst_len * 4, np.int16, (n, c.n_paths, c.burst_len, 2))),
            "params": view(s.params, n * 8, PARAMS_DTYPE, (n,)),
            "meta": view(s.meta, n * 8, TRXD_META_DTYPE, (n,)),
            "results": view(s.results, n * 32, RESULT_DTYPE, (n,)),
            "soft": view(s.soft, n * c.soft_stride * 4, np.float32, (n, c.soft_stride)) if c.soft_stride else None,
            "pkt": view(s.pkt, n * c.pkt_stride, np.uint8, (n, c.pkt_stride)) if c.pkt_stride else None,
            "pkt_len": view(s.pkt_len, n * 2, np.uint16, (n,)) if c.pkt_stride else None,
        }

    def slot(self, i):
        return self._slots[i]

    def submit(self, i, n):
        _check(self.trx.L.trxhip_hostpipe_submit(self.h, i, n), "trxhip_hostpipe_submit")

    # ---- bursts by reference: the samples stay where they are (a registered host range), the slot carries pointers ----
    def register_host(self, array):
        """Pin a numpy array (the radio's receive ring) and map it into the device: bursts inside it can be submitted by
        address.  The caller keeps the array alive until unregister_host() / close()."""
        _check(self.trx.L.trxhip_hostpipe_register_host(self.h, _VP(array.ctypes.data), array.nbytes), "trxhip_hostpipe_register_host")
        self._registered = getattr(self, "_registered", []) + [array]     # pinned pages must not be freed under the device

    def unregister_host(self, array):
        _check(self.trx.L.trxhip_hostpipe_unregister_host(self.h, _VP(array.ctypes.data)), "trxhip_hostpipe_unregister_host")
        self._registered = [a for a in getattr(self, "_registered", []) if a is not array]

    def sources(self, i):
        """uint64 view of slot i's pointer array (max_bursts host addresses)."""
        q = _VP()
        _check(self.trx.L.trxhip_hostpipe_slot_sources(self.h, i, C.byref(q)), "trxhip_hostpipe_slot_sources")
        buf = (C.c_ubyte * (self.cfg.max_bursts * 8)).from_address(q.value)
        return np.frombuffer(buf, dtype=np.uint64)

    def submit_by_ref(self, i, n):
        _check(self.trx.L.trxhip_hostpipe_submit_by_ref(self.h, i, n), "trxhip_hostpipe_submit_by_ref")

    def wait(self, i):
        _check(self.trx.L.trxhip_hostpipe_wait(self.h, i), "trxhip_hostpipe_wait")

    def query(self, i):
        return int(self.trx.L.trxhip_hostpipe_query(self.h, i))

    def run(self, iq, params, meta=None):
        """iq int16[n, burst_len, 2], params PARAMS_DTYPE[n], meta TRXD_META_DTYPE[n] (numpy, pageable).
        Returns dict(results, soft, pkt, pkt_len) of numpy arrays."""
        c = self.cfg
        n = iq.shape[0]
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE)
        res = np.empty(n, dtype=RESULT_DTYPE)
        soft = np.empty((n, c.soft_stride), dtype=np.float32) if c.soft_stride else None
        pkt = np.empty((n, c.pkt_stride), dtype=np.uint8) if c.pkt_stride else None
        plen = np.empty(n, dtype=np.uint16) if c.pkt_stride else None
        if meta is not None:
            meta = np.ascontiguousarray(meta, dtype=TRXD_META_DTYPE)

        def ptr(a):
            return _VP(a.ctypes.data) if a is not None else _VP(0)
        _check(self.trx.L.trxhip_hostpipe_run(self.h, ptr(iq), ptr(params), ptr(meta), ptr(res), ptr(soft), ptr(pkt), ptr(plen), n),
               "trxhip_hostpipe_run")
        return {"results": res, "soft": soft, "pkt": pkt, "pkt_len": plen}

    def close(self):
        if getattr(self, "h", None):
            self._slots = None
            self.trx.L.trxhip_hostpipe_destroy(self.h)
            self.h = None
            self._registered = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
