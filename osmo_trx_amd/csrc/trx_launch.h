// trx_launch.h -- the launchers and other internals that one csrc/ translation unit defines and another calls.  They have C
// linkage and are declared here only: every file that defines or calls one includes this header, so a definition whose
// signature drifts from its declaration does not compile.  All return 0 or a TRXHIP_* error code.
#ifndef TRX_LAUNCH_H
#define TRX_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/trxhip.h"
#include "trx_tables.h"
#include "trx_tx_tables.h"

/* RadioInterfaceMulti's ARFCN map (radioInterfaceMulti.cpp:92-124, :214-231): the filterbank path (0..3) of logical channel l
 * with `rows` = 1..3 logical channels; rows = 4 names the four paths themselves (the four-row receive object) */
constexpr int trx_arfcn_pchan(int rows, int l)
{
	return rows == 4 ? l : (rows == 1 ? 0 : (rows == 2 ? (l == 0 ? 0 : 3) : (l == 0 ? 1 : (l == 1 ? 0 : 3))));
}

extern "C" {

/* ---- trxhip_detect_demod_batch() and friends: trx_capi.cpp's pull_common() makes every choice, these only launch it ---- */

/* trx_kernel4.hip: the 4-SPS kernel (L 624..628), instance burst_pull4_kernel<cf32, exact, common>.  d_pool_ctr (both 4-SPS
 * launchers): the launch's counter pair of the cross-die work pool, or NULL; given only with n_bursts >= 128 * n_cu, so that
 * the grid is the persistent one and every workgroup owns >= 8 groups of 16 bursts */
int trx_launch_pull4(unsigned *d_pool_ctr, const void *d_iq, int cf32, int exact, int common, const trxhip_burst_params *d_params,
		     trxhip_burst_result *d_results, float *d_soft, const trx_tables *d_tab, const float *d_ebp_in, size_t n_bursts,
		     int L, float thresh, float full_scale, int soft_stride, int flags, int n_cu, hipStream_t stream);
/* trx_kernel4.hip: the split -- the normal-burst kernel over the batch, then burst_pull4_kernel's common instance over the
 * bursts it left on the list d_redo; h_left: pinned word that receives how many it left */
int trx_launch_pull4_nb(unsigned *d_pool_ctr, const void *d_iq, const trxhip_burst_params *d_params, trxhip_burst_result *d_results,
			float *d_soft, const trx_tables *d_tab, size_t n_bursts, float thresh, float full_scale, int n_cu,
			unsigned *d_redo, unsigned *h_left, hipStream_t stream);
/* trx_kernels.hip: the generic kernel, instance burst_pull_kernel<sps, cf32, nld> */
int trx_launch_pull(const void *d_iq, int cf32, int nld, const trxhip_burst_params *d_params, trxhip_burst_result *d_results,
		    float *d_soft, const trx_tables *d_tab, const float *d_ebp_in, size_t n_bursts, int L, int sps, float thresh,
		    float full_scale, int soft_stride, int flags, int n_cu, hipStream_t stream);
size_t trx_pull_lds_bytes(int L, int waves_per_block);                 /* trx_kernels.hip */
/* trx_kernels.hip: the stream form of the 1-SPS kernel, instance burst_pull_stream_kernel<cf32>, for the uplink scheduler.  d_iq:
 * the first of n_slots slots of a 1-SPS receive stream that lie back to back, 157 samples where the slot's TN is a multiple of
 * 4 and 156 elsewhere; tn_phase: that first slot's TN & 3.  Slot k is read where it lies, trx_rxs_slot_start() samples behind
 * d_iq, and nothing outside the slots is read.  Slot k's record and soft row are those of burst_pull_kernel<1, cf32, 3> over a
 * row of that slot's length, bit for bit.  flags: TRXHIP_FLAG_SLICE and the TRX_IFLAG_* bits */
int trx_launch_pull_stream(const void *d_iq, int cf32, unsigned tn_phase, const trxhip_burst_params *d_params,
			   trxhip_burst_result *d_results, float *d_soft, const trx_tables *d_tab, size_t n_slots, float thresh,
			   float full_scale, int soft_stride, int flags, int n_cu, hipStream_t stream);

int trx_fast_stats_read(unsigned long long *out4, int reset);          /* trx_kernel4.hip: the FAST detector's counters */
int trx_unit_masks_match(const trx_tables *t);                        /* trx_kernel4.hip: compiled-in sign masks vs the tables */
int trx_unit_mask_sch_match(const trx_tables *t);                     /* trx_sch.hip: the SCH sequence's sign mask vs the tables */

/* ---- trx_sch.hip, trx_va.hip ---- */
int trx_launch_sch_detect(const float *d_iq, size_t buf_stride, trxhip_burst_result *d_results, const trx_tables *d_tab,
			  size_t n_bufs, int len, int start, int toa_sub, float thresh, int unit_tables, hipStream_t stream);
size_t trx_va_lds_bytes(int L);
int trx_launch_va_demod(const float *d_iq, const trxhip_burst_params *d_params, const trxhip_burst_result *d_detected, float *d_soft,
			int32_t *d_starts, size_t n_bursts, int L, float scale, int soft_stride, int flags, hipStream_t stream);

/* trx_rx_sched_va.hip: the uplink scheduler's use_va flow over the chans * n_slots slots of one pull, slot chan * n_slots + k at
 * d_in + chan * in_stride + k * 625 - carried samples (int16 pairs, or complex64 with cf32), slot 0 of every channel at
 * d_edge + chan * 625 instead when d_edge is given.  _prep: the detector's rows (samples 20 .. 604, then 40 zeros) into d_shift
 * in the input's format, and energyDetect(slot, 80) of the slots as read.  _slots: va_demod_kernel's work with slicing for the
 * slots whose record in d_detected has rc > 0, a zero soft row for the others */
int trx_launch_rx_va_prep(const void *d_in, int cf32, size_t in_stride, const void *d_edge, uint32_t carried, size_t n_slots, int chans,
			  void *d_shift, float *d_energy, hipStream_t stream);
int trx_launch_rx_va_slots(const void *d_in, int cf32, size_t in_stride, const void *d_edge, uint32_t carried, size_t n_slots,
			   int chans, const trxhip_burst_params *d_params, const trxhip_burst_result *d_detected, float *d_soft,
			   float scale, int soft_stride, hipStream_t stream);

/* trx_sch_sync.hip: the MS-side SCH receiver.  d_iq: int16 IQ (i16) or complex64 buffers, buf_stride samples apart; acq: the
 * buffer search over the lags 0 .. len - 513 through d_power (n_bufs x (len - 512) floats) and d_best (n_bufs), else the
 * one-slot search (both NULL) */
int trx_launch_sch_sync(const void *d_iq, int i16, size_t buf_stride, trxhip_sch_sync_result *d_results, int8_t *d_bits,
			size_t n_bufs, int len, int acq, float scale, float *d_power, int32_t *d_best, hipStream_t stream);

/* trx_ms_rx.hip: the MS-side downlink burst receiver, n_slots slots of 625 samples slot_stride samples apart; scale: 1 / rx_full_scale */
int trx_launch_ms_rx(const void *d_iq, int i16, size_t slot_stride, const trxhip_ms_slot *d_slots, trxhip_ms_burst_ind *d_ind,
		     int8_t *d_bits, size_t n_slots, float scale, float rx_full_scale, hipStream_t stream);
/* its stream form (trx_ms_sched.h): the slots of one pull of the MS-side slot scheduler, read where they lie in d_chunk */
struct trx_mss_stream;
int trx_launch_ms_rx_stream(const void *d_chunk, int i16, const struct trx_mss_stream *sa, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
			    size_t n_slots, float scale, float rx_full_scale, hipStream_t stream);
/* its group form (trx_ms_sched.h): n_waves waves over the n_entries members of the table d_tab, each wave's slots those of one
 * member */
struct trx_mss_member;
int trx_launch_ms_rx_group(const struct trx_mss_member *d_tab, int i16, size_t n_entries, size_t n_waves, float scale, float rx_full_scale,
			   hipStream_t stream);
#define TRX_MS_RX_SLOTS_PER_WAVE 4      /* VA_BPW: slots per wave in all three forms */

/* trx_ms_agc.hip: the MS-side receive gain control.  _level_rows: normed_abs_sum() of n_rows rows of row_len int16 samples,
 * row_stride samples apart.  _agc: the three launches of a pull with gain control on (trx_ms_agc.h) -- the levels of n_waves
 * slots, one per wave, the recurrence over n_pieces pieces, the decisions of n_entries members -- over the one entry h_entry,
 * passed as a kernel argument (d_tab unused), or over the n_entries entries of d_tab (h_entry NULL) */
struct trx_agc_entry;
int trx_launch_ms_level_rows(const int16_t *d_in, size_t n_rows, size_t row_len, size_t row_stride, float *d_level, hipStream_t stream);
int trx_launch_ms_agc(const struct trx_agc_entry *h_entry, const struct trx_agc_entry *d_tab, size_t n_entries, size_t n_waves,
		      size_t n_pieces, uint32_t full_scale, hipStream_t stream);

/* trx_ms_afc.hip: the MS-side FCCH frequency-offset measurement.  _fcch_rows: gsm_fcch_offset() of n_slots rows of 625 samples
 * (int16 pairs or complex64), slot_stride samples apart.  _afc: the one launch of a pull with AFC on (trx_ms_afc.h) -- n_waves
 * FCCH slots, one per wave -- over the one job h_job, passed as a kernel argument (d_tab unused), or over the n_jobs jobs of
 * d_tab (h_job NULL) */
struct trx_afc_job;
int trx_launch_ms_fcch_rows(const void *d_iq, int i16, size_t slot_stride, trxhip_ms_fcch *d_out, size_t n_slots, float scale,
			    hipStream_t stream);
int trx_launch_ms_afc(const struct trx_afc_job *h_job, const struct trx_afc_job *d_tab, int i16, size_t n_jobs, size_t n_waves,
		      float scale, hipStream_t stream);

/* trx_ms_nco.hip: the MS-side NCO (trx_ms_nco.h).  _nco_rows: n_rows rows of row_len samples (int16 pairs or complex64),
 * row_stride samples apart, row r rotated by d_rec[r] into the complex64 row at d_out + r * out_stride samples; d_tab: the
 * context's phasor tables.
 * trx_ms_rx.hip: the rotating instances of the receiver's stream and group forms -- the same launches as above with the launch's
 * oscillator (the stream form: *nco, by value) or the entries' (the group form: d_nco[k] beside d_tab[k]) */
struct trx_nco_slot;
int trx_launch_ms_nco_rows(const void *d_in, int i16, size_t row_stride, const trxhip_ms_nco_row *d_rec, float *d_out, size_t out_stride,
			   size_t n_rows, size_t row_len, const float *d_tab, hipStream_t stream);
int trx_launch_ms_rx_stream_nco(const void *d_chunk, int i16, const struct trx_mss_stream *sa, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
				size_t n_slots, float scale, float rx_full_scale, const struct trx_nco_slot *nco, const float *d_nco_tab,
				hipStream_t stream);
int trx_launch_ms_rx_group_nco(const struct trx_mss_member *d_tab, int i16, size_t n_entries, size_t n_waves, float scale,
			       float rx_full_scale, const struct trx_nco_slot *d_nco, const float *d_nco_tab, hipStream_t stream);

/* trx_ms_fsearch.hip: the MS-side FCCH search (trx_ms_fsearch.h).  n_bufs rows of buf_len samples (>= 584), buf_stride samples
 * apart; d_cand: room for n_bufs * trx_fs_segments(buf_len) candidates; the hit of row r to d_hit[r] and, where d_fcch is given, the
 * estimator's record of the slot at its pos to d_fcch[r].  Two launches */
int trx_launch_ms_fsearch(const void *d_iq, int i16, size_t buf_stride, size_t buf_len, size_t n_bufs, double min_score, float scale,
			  trxhip_ms_fcch_hit *d_cand, trxhip_ms_fcch_hit *d_hit, trxhip_ms_fcch *d_fcch, hipStream_t stream);

/* ---- trx_aux_kernels.hip ---- */
int trx_launch_pack_trxd(const trxhip_burst_result *d_results, const float *d_soft, int soft_stride, uint8_t *d_pkt,
			 size_t n_bursts, float rssi_offset, hipStream_t stream);
/* the TRXD wire packer; d_results_copy (may be NULL): every result record is also written there -- the host pipe points it at
 * pinned memory and saves the download */
int trx_launch_pack_trxd_wire(const trxhip_burst_result *d_results, const trxhip_burst_params *d_params, const float *d_soft,
			      int soft_stride, const trxhip_trxd_meta *d_meta, uint8_t *d_pkt, int pkt_stride, uint16_t *d_pkt_len,
			      size_t n_bursts, float rssi_offset, hipStream_t stream, trxhip_burst_result *d_results_copy);
/* bursts by reference: n bursts of `dwords` 4-byte words each from the device-side addresses d_src[] */
int trx_launch_gather_bursts(const unsigned long long *d_src, void *d_dst, size_t n, unsigned dwords, hipStream_t stream);
int trx_launch_convolve(const float *d_x, int x_len, const float *d_h, int h_len, int h_complex, float *d_y, int y_len, int start,
			int len, size_t n_vec, hipStream_t stream);
int trx_launch_convert_short_float(float *d_out, const int16_t *d_in, size_t len, hipStream_t stream);
int trx_launch_convert_float_short(int16_t *d_out, const float *d_in, float scale, size_t len, hipStream_t stream);
int trx_launch_dft_strided(const float *d_in, float *d_out, int m, size_t howmany, size_t istride, size_t ostride, int reverse,
			   hipStream_t stream);
int trx_launch_energy_detect(const float *d_x, size_t n_bursts, int burst_len, unsigned window, float *d_out, hipStream_t stream);
int trx_launch_diversity_select(const int16_t *d_iq_paths, size_t n_bursts, int n_paths, int burst_len, int sps, int16_t *d_iq_sel,
				float *d_avg_energy, uint8_t *d_path, hipStream_t stream);
int trx_launch_diversity_power(trxhip_burst_result *d_res, const trxhip_burst_params *d_params, const float *d_avg_energy,
			       size_t n_bursts, float full_scale, hipStream_t stream);
int trx_launch_delay_vector(const float *d_in, float *d_out, const float *d_delays, const trx_tables *d_tab, size_t n_vec, int len,
			    hipStream_t stream);
int trx_launch_scale_vector(float *d_x, size_t len, float sr, float si, hipStream_t stream);
int trx_launch_vector_slicer(float *d_dst, const float *d_src, size_t len, hipStream_t stream);

/* ---- trx_rx_frontend.hip: the receive front end ----
 * trx_launch_channelize / trx_launch_resample: Channelizer(4, ., 16)::rotate and Resampler(p, q, 16)::rotate over a continuous
 * stream; d_hist_io (may be NULL): the carried samples -15 .. -1, read and then replaced by the call's last 15.
 * trx_launch_frontend_fused: the two in one pass (frontend_fused_kernel<rows>).  rows = 4: the four filterbank paths in physical
 * order; rows = 1..3: row l of d_out = logical channel l = path trx_arfcn_pchan(rows, l).  The channel histories are
 * [rows][16].  Returns 1 when the geometry fits no tile: the caller then runs the two launchers above.
 * trx_launch_rx_resamp_s16: convert_short_float + Resampler(p, q, 16)::rotate of one int16 channel; d_hist_in / d_hist_out:
 * 16 int16 IQ samples each, the samples -16 .. -1 of this call and of the next */
int trx_launch_channelize(const int16_t *d_in, float *d_out, size_t n_total, size_t out_stride, const trx_tables *d_tab,
			  void *d_hist_io, hipStream_t stream);
int trx_launch_resample(const float *d_in, float *d_out, size_t n_in, int p, int q, size_t n_chan, size_t in_stride,
			size_t out_stride, const float *d_parts, void *d_hist_io, hipStream_t stream);
int trx_launch_frontend_fused(const int16_t *d_wide, float *d_out, size_t n_total, int rows, int p, int q, size_t out_stride,
			      const float *parts, const trx_tables *d_tab, void *d_wide_hist_io, const void *d_chan_hist_in,
			      void *d_chan_hist_out, hipStream_t stream);
int trx_launch_rx_resamp_s16(const int16_t *d_in, float *d_out, size_t n_in, int p, int q, const float *parts,
			     const void *d_hist_in, void *d_hist_out, hipStream_t stream);

/* ---- trx_tx_frontend.hip: Synthesis(4, ., 16) and the fused multi-ARFCN transmit front end ----
 * d_hist of trx_launch_synthesize: NULL (zero history) or the 4 rows' samples -15 .. -1 at [c * 16 + 0 .. 14] */
int trx_launch_synthesize(const float *d_in, size_t in_stride, const void *d_hist, float *d_out_cf32, int16_t *d_out_s16,
			  float scale, size_t n_times, const trx_tables *d_tab, hipStream_t stream);
int trx_launch_tx_save_hist(const float *d_x, size_t n, size_t stride, int n_chan, void *d_hist, int hn, int hs, hipStream_t stream);
int trx_tx_fused_tm(int p, int q);
int trx_launch_tx_frontend_fused(const float *d_in, size_t in_stride, size_t n_in, const void *d_hist, int hl, float *d_out_cf32,
				 int16_t *d_out_s16, float scale, int chans, int p, int q, const float *d_parts, const trx_tables *d_tab,
				 hipStream_t stream);

/* ---- trx_tx.hip: the burst modulators (trxhip_modulate_batch, trxhip_modulate_trxd_batch) ----
 * d_dgram_len == NULL: d_in holds bits (in_stride bytes per burst) and d_params the descriptors; otherwise d_in holds TRXD
 * datagrams (in_stride bytes each), d_dgram_len their lengths and h_att_scale the 256 scales by tx_att (host memory, passed
 * by value) */
int trx_launch_tx_modulate(const uint8_t *d_in, size_t in_stride, const trxhip_tx_params *d_params, const uint16_t *d_dgram_len,
			   const float *h_att_scale, const trx_tx_tables *d_tab, float *d_out_cf32, int16_t *d_out_s16,
			   float s16_scale, size_t out_stride, int32_t *d_out_len, trxhip_tx_info *d_info, size_t n, int sps,
			   hipStream_t stream);
int trx_tx_tables_generate(trx_tx_tables *t);                         /* host only */
/* the downlink burst scheduler's render (trx_tx.hip, tx_render_kernel; trx_tx_sched.h): n_slots slots of chans channels from
 * the slot words d_slots[chan * n_slots + s] (a staged row holds its datagram's length, uint16, in its last two bytes), then
 * the filler-table updates of the render */
struct trx_tx_fill;
struct trx_tx_fill_update;
int trx_launch_tx_render(const uint32_t *d_slots, size_t n_slots, int chans, int tn0, int sps, const uint8_t *d_rows,
			 const trx_tx_fill *d_fill, const float *h_att_scale, const trx_tx_tables *d_tab,
			 float *d_out_cf32, int16_t *d_out_s16, const float *h_s16_scales, size_t out_stride, hipStream_t stream);
int trx_launch_tx_fill_update(const trx_tx_fill_update *d_upd, size_t n, const uint8_t *d_rows, trx_tx_fill *d_fill,
			      hipStream_t stream);
/* the MS-side uplink burst scheduler's render (trx_tx.hip, ms_tx_render_kernel; trx_ms_tx.h): the n_segs segments that tile a
 * window of d_out (int16 I, Q; 4-byte aligned), one wave each, from the staged bursts d_rows */
struct trx_mstx_seg;
struct trx_mstx_row;
int trx_launch_ms_tx_render(const trx_mstx_seg *d_segs, size_t n_segs, const trx_mstx_row *d_rows, const trx_tx_tables *d_tab,
			    int16_t *d_out, hipStream_t stream);
/* the group's two launches (trx_tx.hip): ms_tx_stage_kernel scatters the n rows of a submit to ring rows d_dst[i] < ring_rows;
 * ms_tx_render_group_kernel draws the n_waves tiles of the n_entries members of a table (trx_ms_tx.h), its bursts behind the
 * entries, into d_out (int16 I, Q; 4-byte aligned) */
struct trx_mstx_gmember;
int trx_launch_ms_tx_stage(const trx_mstx_row *d_src, const uint32_t *d_dst, size_t n, trx_mstx_row *d_rows, size_t ring_rows,
			   hipStream_t stream);
int trx_launch_ms_tx_render_group(const trx_mstx_gmember *d_tab, uint32_t n_entries, uint32_t n_waves, const trx_mstx_row *d_rows,
				  const trx_tx_tables *d_tab_tx, int16_t *d_out, hipStream_t stream);
/* the rotating instances of the two renders (ms_tx_render_nco_kernel, ms_tx_render_group_nco_kernel): the member's uplink
 * oscillator between the modulator's sample and the cast.  nco = {phase of the window's first sample, inc} (the group: in the
 * entries), d_nco_tab the context's phasor tables (trx_ms_nco.h) */
int trx_launch_ms_tx_render_nco(const trx_mstx_seg *d_segs, size_t n_segs, const trx_mstx_row *d_rows, const trx_tx_tables *d_tab,
				int16_t *d_out, trxhip_ms_nco_row nco, const float *d_nco_tab, hipStream_t stream);
int trx_launch_ms_tx_render_group_nco(const trx_mstx_gmember *d_tab, uint32_t n_entries, uint32_t n_waves, const trx_mstx_row *d_rows,
				      const trx_tx_tables *d_tab_tx, int16_t *d_out, const float *d_nco_tab, hipStream_t stream);
/* trx_capi.cpp: a transmit front end's logical channels, block length and output samples per block */
int trx_tx_frontend_geometry(const trxhip_tx_frontend *f, int *chans, int *block_len, size_t *out_per_block);

/* trx_capi.cpp: a receive front end of trxhip_rx_frontend_create_chans() -- its context, rows, whether it is a RESAMP object,
 * block length and ratio; TRXHIP_EINVAL for NULL and for the four-row object of trxhip_rx_frontend_create() */
int trx_rx_frontend_geometry(const trxhip_rx_frontend *f, trxhip_ctx **ctx, int *rows, int *resamp, int *block_len, int *p, int *q);

}  // extern "C"
#endif
