/*
 * trxhip.h -- C ABI of the MI355X (gfx950) burst DSP for osmo-trx: the receive side and the burst modulators.
 *
 * This is the thin extern "C" HIP seam that sits where the reference calls its burst DSP:
 *
 *   Transceiver::pullRadioVector()            Transceiver52M/Transceiver.cpp:665-815
 *     energyDetect()                          Transceiver52M/sigProcLib.cpp:1573-1585   (Transceiver.cpp:725)
 *     detectAnyBurst()                        Transceiver52M/sigProcLib.cpp:1926-1957   (Transceiver.cpp:768)
 *     demodAnyBurst()                         Transceiver52M/sigProcLib.cpp:2130-2137   (Transceiver.cpp:786)
 *     vectorSlicer()                          Transceiver52M/sigProcLib.cpp:546-556     (Transceiver.cpp:803)
 *   convert_short_float()                     Transceiver52M/arch/common/convert.h:9    (radioInterface.cpp:344-348)
 *   convolve_real()/convolve_complex()        Transceiver52M/arch/common/convolve.h:6-14
 *   Channelizer::rotate()                     Transceiver52M/Channelizer.cpp:74-99
 *   Resampler::rotate()                       Transceiver52M/Resampler.cpp:131-150
 *   Synthesis::rotate()                       Transceiver52M/Synthesis.cpp:66-104
 *   RadioInterfaceMulti::pushBuffer()         Transceiver52M/radioInterfaceMulti.cpp:316-362
 *   RadioInterfaceResamp::pushBuffer()        Transceiver52M/radioInterfaceResamp.cpp:196-230
 *
 * The reference runs these one burst at a time on one CPU thread per ARFCN; here they are batched:
 * one call processes N independent bursts that are resident in device memory (HBM).  The
 * single-burst C++ signatures of sigProcLib.h are kept by the host shim in
 * osmo_trx_amd/host/ (batch of 1 over this ABI); INTEGRATION.md shows the binding.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * TRXHIP_E* code and never throws.  Pointers named d_* are DEVICE pointers (hipMalloc / torch
 * CUDA tensors); h_* are host pointers.  `stream` is a hipStream_t passed as void* (NULL = the
 * default stream).  Calls on different contexts/streams may run concurrently from different
 * host threads (one RxUpper thread per ARFCN in the reference, Transceiver.cpp:308-314).
 */
#ifndef TRXHIP_H
#define TRXHIP_H

#include <math.h>     /* powf() in TRXHIP_FAST_CI_ATOL_DB */
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRXHIP_ABI_VERSION 5

/* error codes */
#define TRXHIP_OK          0
#define TRXHIP_EINVAL     (-22)   /* bad argument */
#define TRXHIP_ENOMEM     (-12)
#define TRXHIP_ENODEV     (-19)   /* no usable gfx950 device / HIP runtime failure at init */
#define TRXHIP_EIO        (-5)    /* HIP launch/runtime error (maps to pullRadioVector's -EIO, Transceiver.cpp:686) */
#define TRXHIP_ENOTSUP    (-95)

/* CorrType, sigProcLib.h:30-38 (same numeric values) */
enum trxhip_corr_type {
	TRXHIP_OFF = 0, TRXHIP_TSC = 1, TRXHIP_EXT_RACH = 2, TRXHIP_RACH = 3,
	TRXHIP_SCH = 4, TRXHIP_EDGE = 5, TRXHIP_IDLE = 6
};
/* SignalError, sigProcLib.h:40-46: detect returns -TRXHIP_SIGERR_* */
enum trxhip_signal_error {
	TRXHIP_SIGERR_NONE = 0, TRXHIP_SIGERR_BOUNDS = 1, TRXHIP_SIGERR_CLIP = 2,
	TRXHIP_SIGERR_UNSUPPORTED = 3, TRXHIP_SIGERR_INTERNAL = 4
};

#define TRXHIP_MAX_TOA        112   /* largest max_toa the kernels accept (reference default: 63 AB / 30 NB) */
#define TRXHIP_MAX_BURST_LEN 1536   /* samples per burst the kernels accept (625 @4 SPS, 156/157 @1 SPS) */
#define TRXHIP_BURST_THRESH   4.0f  /* BURST_THRESH, sigProcLib.h:54 */

/* `flags` of the detect/demod entry points */
#define TRXHIP_FLAG_SLICE        1  /* soft bits through vectorSlicer(): 0..1, 148 per burst (else raw -1..+1) */
#define TRXHIP_FLAG_EXACT_DEMOD  2  /* the bit-exact kernel: demodulate with the reference's two FIR stages in its operand order and
                                     * search the TOA with the reference's sums: rc, TOA, amp, C/I and soft bits bit-identical to the
                                     * generic-C reference.  Default (flag clear) is the fused kernel: delay-o-decimate filter with
                                     * FMA (24 of its 35 taps), soft bits within TRXHIP_FUSED_SOFT_ATOL (below) of the reference's,
                                     * ~4x fewer multiply-adds; and the FAST detector (round 5): rc, TSC and TOA still IDENTICAL to
                                     * the reference's -- every early / late decision of peakDetect()'s bisection is either
                                     * certified by a proven rounding-error margin or re-run in the reference's operand order
                                     * (csrc/trx_device.h, peak_detect_fast) -- while the interpolated peak value is an FMA sum:
                                     * amp within TRXHIP_FAST_AMP_RTOL, C/I within TRXHIP_FAST_CI_ATOL_DB(ci) of the reference's.
                                     * Only the 4-SPS / 625-sample kernel has a fused path; others are always exact. */
#define TRXHIP_FLAG_IDLE_DUMMY   4  /* search IDLE slots for the dummy burst, as detectAnyBurst(IDLE) does (detectDummyBurst,
                                     * sigProcLib.cpp:1863-1877, :1945-1947; rc = IDLE on a hit) instead of skipping them as
                                     * pullRadioVector does (Transceiver.cpp:754-755) */
#define TRXHIP_FLAG_USE_VA       8  /* trxhip_hostpipe_cfg.flags and trxhip_rx_sched_cfg.flags only: cfg->use_va, see there */
#define TRXHIP_FLAG_FEW_NB_SLOTS 16 /* a HINT from a caller that knows its slot types (expectedCorrType() runs on the host,
                                     * Transceiver.cpp:513-601): more than 1/32 of the batch's slots are not normal-burst slots
                                     * (type TSC, tsc < 8, max_toa <= 32).  Results never depend on it; the call then runs the
                                     * general kernel alone instead of the normal-burst kernel + the general one over what that
                                     * leaves (which reads every burst of another type twice).  The host pipe sets it from the
                                     * parameters it is handed; without a hint the library finds out by itself -- the second
                                     * kernel reports how much it was left, and a context that sees more than 1/32 runs the
                                     * general kernel alone for its next 63 launches before it tries again. */
/* The FAST detector's tolerance statement (fused kernels only; tests quote these).  amp = interpolated correlation peak / gain:
 * one 16-term sum per component, FMA against product-then-sum; |amp - ref| <= TRXHIP_FAST_AMP_RTOL * |ref| (complex distance;
 * proven bound 2.6 * 25 u = 3.9e-6 relative to the correlation's arg-max magnitude, measured <= 3e-7).
 * C/I = 10 log10(C / (S - C)) with C = |peak|^2 / den and S the mean sample power (tree-summed in the FAST detector: within
 * 1.2e-6 of the reference's ordered sum): S - C cancels by the factor 1 + C/I, so relative errors eC of C and eS of S become
 * (eC + eS) (1 + 10^(ci/10)) of the ratio:  |ci - ref| <= 1e-4 dB + 4.35 * (2 * TRXHIP_FAST_AMP_RTOL + 1.2e-6) * (1 + 10^(ci/10)) dB.
 * NaN: S < C (a noise slot whose peak estimate exceeds the mean sample power) makes C / (S - C) negative and C/I NaN in the
 * reference as here (sigProcLib.cpp:1637 has no guard); the tests require the SAME NaN pattern (tests/oracle_lib.py
 * assert_fast_ci).  Where S - C cancels to within the relative errors above -- |S - C| <= 3e-6 S, i.e. C/I beyond +55 dB: a peak that
 * explains the whole sample power to six digits, which no burst with any noise or sample rounding in it reaches -- its sign is not
 * covered by the bar: NaN on one side could meet a large finite value on the other. */
#define TRXHIP_FAST_AMP_RTOL        1e-6f
#define TRXHIP_FAST_CI_ATOL_DB(ci)  (1e-4f + 1.4e-5f * (1.0f + powf(10.0f, (ci) * 0.1f)))
/* The one statement of the default (fused) demodulator's tolerance; tests/, tools/parity_campaign.py, bench.py and DESIGN.md
 * quote these two numbers and nothing else.  ABSOLUTE error of a soft bit against the generic-C reference, on soft bits
 * whose full scale is 1 (raw -1..+1 or sliced 0..1):
 *     |soft - ref| <= TRXHIP_FUSED_SOFT_ATOL * max(1, rms / (4 |amp|))        GMSK, 148 / 156 soft bits
 * rms = sqrt(energyDetect()), amp = the detector's amplitude estimate.  The filter's rounding error is relative to the
 * SAMPLES while the soft bits are scaled by 1/amp: for every real detection rms <= 4 |amp| and the bound is the plain
 * 1e-5; a noise-only slot that passes the detector at C/I < -12 dB has samples many times its amplitude estimate and the
 * bound grows with that ratio (worst seen over 4 x 1M bursts: 1.14e-5 on one value in 155 M).  8-PSK rows (444 soft
 * bits: equaliser gain ~2 behind the filter, three soft bits per symbol) and deliberately extreme inputs (tests' fuzz:
 * saturation, impulses, silence): TRXHIP_FUSED_SOFT_ATOL_8PSK.  The north-star bar is 1e-4. */
#define TRXHIP_FUSED_SOFT_ATOL       1e-5f
#define TRXHIP_FUSED_SOFT_ATOL_8PSK  5e-5f

/* Per-burst input: what pullRadioVector() knows before calling detectAnyBurst()
 * (expectedCorrType() Transceiver.cpp:513-601, mTSC, mMaxExpectedDelayAB/NB :757-758). 8 bytes. */
typedef struct trxhip_burst_params {
	uint8_t  type;      /* enum trxhip_corr_type expected for the slot */
	uint8_t  tsc;       /* training sequence code 0..7 */
	uint16_t max_toa;   /* search window, symbols */
	uint32_t reserved;  /* must be 0 */
} trxhip_burst_params;

/* Per-burst output: estim_burst_params (sigProcLib.h:113-118) + what pullRadioVector() derives. 32 bytes. */
typedef struct trxhip_burst_result {
	int32_t rc;          /* detectAnyBurst(): CorrType (>0) | 0 (nothing found) | -SignalError */
	float   toa;         /* ebp.toa, symbols */
	float   amp_re;      /* ebp.amp */
	float   amp_im;
	float   ci;          /* ebp.ci, dB */
	float   energy;      /* energyDetect(burst, 20*sps) */
	float   rssi;        /* 20*log10(full_scale/sqrt(energy)), dBFS without rssi_offset (Transceiver.cpp:751) */
	uint8_t tsc;         /* ebp.tsc */
	uint8_t clip;        /* maxAmplitude() > 30000 (sigProcLib.cpp:1746-1750) */
	uint8_t idle;        /* bi->idle */
	uint8_t nbits_div4;  /* bi->nbits / 4: 37 (148 GMSK), 111 (444 8-PSK), 0 when idle */
} trxhip_burst_result;

typedef struct trxhip_ctx trxhip_ctx;   /* one per device; owns the device-resident tables */

/* ---- lifetime: sigProcLibSetup()/sigProcLibDestroy(), sigProcLib.h:57-60; convolve_init()/convert_init() ---- */
int  trxhip_abi_version(void);
int  trxhip_device_count(void);                       /* number of visible HIP devices (0 if none) */
/* Generates all tables on the host exactly as sigProcLibSetup() does (sigProcLib.cpp:2139-2172)
 * and uploads them to device `device`.  Fails with TRXHIP_ENODEV when no GPU is usable: there is
 * no CPU fallback. */
int  trxhip_create(trxhip_ctx **out, int device);
void trxhip_destroy(trxhip_ctx *ctx);
const char *trxhip_strerror(int err);
/* Work distribution of the 4-SPS kernel for large batches: 1 (default) = the last eighth of the 16-burst groups is drawn from
 * a device-wide counter by whichever CU gets there (evens out the eight dies), 0 = every group dealt statically.  Results
 * never depend on it (tests/test_gpu_parity.py); a measurement switch.  TRXHIP_NO_POOL in the environment makes 0 the
 * default of contexts created afterwards. */
int  trxhip_set_work_pool(trxhip_ctx *ctx, int enabled);
/* Kernel split of trxhip_detect_demod_batch() for the call pullRadioVector() makes (int16 bursts of 625 samples at 4 SPS, fused
 * demodulator, TRXHIP_FLAG_SLICE alone, soft_stride 148): 1 (default) = the normal-burst kernel (csrc/trx_kernel_nb.hip: TSC
 * slots with max_toa <= 32 and nothing else) runs over the batch and the general kernel over the list of bursts it left --
 * slots of other types, wide windows, the rare bursts outside its straight-line paths; 0 = the general kernel alone, as in
 * rounds 1-5.  Results are bit-identical either way (tests/test_gpu_nb_kernel.py); a measurement switch.  TRXHIP_NO_NB_KERNEL in
 * the environment makes 0 the default of contexts created afterwards. */
int  trxhip_set_nb_kernel(trxhip_ctx *ctx, int enabled);
/* Counters of the fused kernels' FAST detector on the context's device since the last reset (synchronises the device):
 * out4[0] = bursts whose TOA search found an uncertified early / late decision on its path and was re-run in the
 * reference's operand order; out4[1..3] reserved.  Diagnostics (tests and tools report the re-run rate). */
int  trxhip_fast_stats(trxhip_ctx *ctx, uint64_t *out4, int reset);

/* ---- table blob: generated once on rank 0, broadcast to the other ranks (RCCL), adopted there ---- */
size_t trxhip_tables_size(void);                                      /* bytes of the device table blob */
int  trxhip_tables_generate_host(void *h_blob, size_t size);          /* host-only: no GPU needed */
int  trxhip_create_from_tables(trxhip_ctx **out, int device, const void *h_blob, size_t size);
int  trxhip_tables_device_ptr(trxhip_ctx *ctx, void **d_blob);        /* for an in-place RCCL broadcast */
uint64_t trxhip_tables_checksum(const void *h_blob, size_t size);     /* FNV-1a over the blob */

/* ---- the hot path: batched pullRadioVector() DSP core ----
 * For each burst b < n_bursts (independent):
 *   int16 IQ -> fp32 (convert_short_float, no scaling) -> energyDetect -> rssi -> clip flag ->
 *   detectAnyBurst(type,tsc,threshold,sps,max_toa) -> if rc>0: demodAnyBurst -> soft bits.
 *   d_iq     : n_bursts * burst_len * 2 int16 (I,Q interleaved, burst-major), 4-byte aligned
 *   d_params : n_bursts trxhip_burst_params
 *   d_results: n_bursts trxhip_burst_result
 *   d_soft   : n_bursts * soft_stride float32 (may be NULL to skip soft output).
 *              TRXHIP_FLAG_SLICE set: rx_burst[] after vectorSlicer(), 0..1, first nbits valid (148) -- what
 *              pullRadioVector() hands to TRXD; clear: raw demodAnyBurst() SoftVector
 *              (-1..+1; 156 values @4 SPS, burst_len @1 SPS).  A burst detected as EDGE (8-PSK) yields 444 soft
 *              bits (nbits_div4 = 111): give soft_stride >= 444 when EDGE slots are possible, otherwise the row is
 *              truncated to soft_stride.  Unused tail and undetected bursts are zero-filled.
 *   flags    : TRXHIP_FLAG_* bits
 *   sps      : 1 or 4; burst_len: 625 @4 SPS (>= 624), 156/157 @1 SPS (148..192 is accepted at 1 SPS)
 *              1 SPS with TRXHIP_FLAG_SLICE clear: the reference's GMSKReverseRotation1 table has 157 entries
 *              (sigProcLib.cpp:207), so raw soft values exist for i < min(burst_len, 157); the rest of the row is 0.
 *              Sliced rows (148 values) are not affected.
 * Asynchronous on `stream`, with two exceptions on the kernel split (trxhip_set_nb_kernel()): the call waits until the split
 * launch four split launches back on this context has completed (its leftover list is reused), and when a batch is larger
 * than that list has room for, the hipFree / hipMalloc that grow it can wait for the device.
 */
int trxhip_detect_demod_batch(trxhip_ctx *ctx,
			      const int16_t *d_iq, const trxhip_burst_params *d_params,
			      trxhip_burst_result *d_results, float *d_soft,
			      size_t n_bursts, int burst_len, int sps,
			      float threshold, float full_scale,
			      int soft_stride, int flags, void *stream);

/* Diversity-path selection in front of the hot path (Transceiver.cpp:723-741): every burst arrives on n_paths receive
 * paths (radioVector::chans()); pullRadioVector() measures energyDetect(path, 20*sps) on each, demodulates the FIRST path
 * with the highest energy and reports rssi / noise from avg = sqrt(sum of the path energies / n_paths).
 *   d_iq_paths   : n_bursts x n_paths x burst_len x 2 int16 (the paths of one burst back to back), 4-byte aligned
 *   d_iq_sel     : n_bursts x burst_len x 2 int16: the chosen path of every burst -> trxhip_detect_demod_batch()
 *   d_avg_energy : n_bursts floats, sum_i pow_i / n_paths (= avg^2)
 *   d_path       : n_bursts chosen path indices (may be NULL)
 * trxhip_apply_diversity_power() then writes energy = avg^2 and rssi = 20*log10(full_scale / avg) into the result records
 * of the detect/demod launch over d_iq_sel (slots that are OFF keep their zeros).  1 <= n_paths <= 8. */
int trxhip_select_diversity_batch(trxhip_ctx *ctx, const int16_t *d_iq_paths, size_t n_bursts, int n_paths, int burst_len, int sps,
				  int16_t *d_iq_sel, float *d_avg_energy, uint8_t *d_path, void *stream);
int trxhip_apply_diversity_power(trxhip_ctx *ctx, trxhip_burst_result *d_results, const trxhip_burst_params *d_params,
				 const float *d_avg_energy, size_t n_bursts, float full_scale, void *stream);

/* Same, from complex64 device samples (the form sigProcLib's detectAnyBurst()/demodAnyBurst() take). */
int trxhip_detect_demod_batch_cf32(trxhip_ctx *ctx,
				   const float *d_iq_cf32, const trxhip_burst_params *d_params,
				   trxhip_burst_result *d_results, float *d_soft,
				   size_t n_bursts, int burst_len, int sps,
				   float threshold, float full_scale,
				   int soft_stride, int flags, void *stream);

/* demodAnyBurst() on its own (sigProcLib.h:151-152): the caller supplies, per burst, the CorrType
 * (d_params[b].type; EDGE selects the 8-PSK demodulator, 444 soft bits, C/I replaced by the EVM estimate) and the
 * estim_burst_params it got from detection as d_ebp[b] = {toa, amp_re, amp_im, unused} (16-byte aligned).
 * Detection is skipped; d_soft receives the soft bits, d_results echoes the parameters. */
int trxhip_demod_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, const trxhip_burst_params *d_params,
			    const float *d_ebp, trxhip_burst_result *d_results, float *d_soft,
			    size_t n_bursts, int burst_len, int sps, int soft_stride, int flags, void *stream);

/* detectSCHBurst() (sigProcLib.h:139-148, sigProcLib.cpp:1805-1861), the MS-side synchronisation-burst search, for
 * n_bufs independent buffers of buf_len complex64 samples at 4 samples per symbol.  `state` is sch_detect_type in the
 * reference's order; the search covers len = 156 (FULL), 8 (NARROW) or 15000 (BUFFER, 12 frames) symbol positions of
 * the first 4*len samples (the reference decimates by 4 whatever `sps` says, :1841), so buf_len >= 4*len is required
 * (the reference asserts, Vector.h:236-237).  sps other than 1 or 4 is the reference's "return -1": -TRXHIP_EINVAL.
 * d_results[b]: rc = 1 / 0 (detectBurst()'s return), toa (symbols, head or 3+39+64 already subtracted, :1853-1858),
 * amp, ci; toa = amp = 0 on a miss (:1846-1850); the other fields are zero. */
enum { TRXHIP_SCH_DETECT_FULL = 0, TRXHIP_SCH_DETECT_NARROW = 1, TRXHIP_SCH_DETECT_BUFFER = 2 };
int trxhip_detect_sch_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, trxhip_burst_result *d_results,
				 size_t n_bufs, size_t buf_len, int sps, int state, float threshold, void *stream);

/* The MS-side synchronisation-burst receiver, the live branch of ms_trx::handle_sch() (ms/ms_rx_lower.cpp:157-205) with
 * decode_sch() (:59-100): convert_and_scale by `scale` (the reference: 1 / rxFullScale), gr-gsm's channel estimate on the 64-bit
 * extended training sequence at 4 samples per symbol, detect_burst_nb() and gsm_sch_decode / gsm_sch_parse / gsm_sch_to_fn
 * (ms/sch.c:141-204), for n_bufs independent buffers of buf_len samples that lie buf_stride >= buf_len samples apart.
 *   TRXHIP_SCH_SYNC_TRACK  get_sch_chan_imp_resp(): one slot.  At most the first 625 samples of a buffer are used, everything
 *                          outside them reads as zero; 160 lags, start clamped to [-39, 39] (buf_len >= 1)
 *   TRXHIP_SCH_SYNC_ACQ    get_sch_buffer_chan_imp_resp(): the lags 0 .. buf_len - 513 of the whole buffer, start not clamped;
 *                          532 <= buf_len <= TRXHIP_SCH_SYNC_MAX_LEN (the reference's buffer: 12 frames = 60000 samples).  Where the
 *                          burst would start in front of the buffer (start < 0; the reference reads in front of its array) the
 *                          missing samples are zeros.  Uses a scratch of the context, n_bufs * (buf_len - 512) floats: ACQ calls
 *                          on one context run one behind the other
 * d_results[b]: see below.  d_bits (may be NULL): int8 [n_bufs][148], detect_burst_nb()'s output (+-127, -127 = a one).
 * -TRXHIP_EINVAL (nothing launched, nothing written): unknown mode, n_bufs == 0, a NULL pointer, buf_stride < buf_len, buf_len
 * outside the mode's range. */
enum { TRXHIP_SCH_SYNC_TRACK = 0, TRXHIP_SCH_SYNC_ACQ = 1 };
#define TRXHIP_SCH_SYNC_MAX_LEN (1 << 20)
typedef struct {             /* 24 bytes */
	int32_t rc;          /* 0: 1 = parity good (and fn >= 0); 0 = not decoded */
	int32_t start;       /* 4: burst start in samples as the reference's function returns it (TRACK: after the clamp) */
	float corr_max;      /* 8: largest |correlation| of the 20-tap channel estimate */
	int32_t fn;          /* 12: gsm_sch_to_fn(); -1 when rc == 0 */
	uint16_t t1;         /* 16: the decoded fields; 0 when rc == 0 */
	uint8_t bsic;        /* 18 */
	uint8_t t2;          /* 19 */
	uint8_t t3p;         /* 20 */
	uint8_t reserved[3]; /* 21: zero */
} trxhip_sch_sync_result;
int trxhip_sch_sync_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, size_t buf_stride, trxhip_sch_sync_result *d_results,
			       int8_t *d_bits, size_t n_bufs, size_t buf_len, int mode, float scale, void *stream);
int trxhip_sch_sync_batch_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t buf_stride, trxhip_sch_sync_result *d_results,
			      int8_t *d_bits, size_t n_bufs, size_t buf_len, int mode, float scale, void *stream);

/* The MS-side downlink burst receiver: upper_trx::pullRadioVector() and the burst indication of driveReceiveFIFO()
 * (ms/ms_upper.cpp:161-304) for n_slots slots of 625 samples at 4 samples per symbol.  Slot b is the 625 samples at
 * d_iq + b * slot_stride (slot_stride in complex samples, >= 625; a stream cut at a constant 625 is slot_stride = 625); nothing
 * outside them is read, and where the receiver reaches outside (the reference's zeroed workbuf, 40 samples either side) it reads
 * zeros.  convert_and_scale's factor is 1.f / rx_full_scale (the reference: 1.f / float(rxFullScale)).
 * d_slots[b] says where the slot lies in the frame structure and what trxcon answered; its kind follows from (fn, tn) alone, on
 * the device.  d_ind[b] is always written (fn, tn copied through, reserved bytes zero, sch_fn = -1 where no SCH was decoded):
 *   SCH      demodulated whether or not ACTIVE is set (the lower layer does, ms_rx_lower.cpp:130-153): start, corr_max, sch_rc,
 *            sch_fn, sch_bsic and the 148 bits are those of trxhip_sch_sync_batch_*(TRXHIP_SCH_SYNC_TRACK) on the same samples, bit
 *            for bit; rssi = 10, toa256 = 0 (:194-200); sent = ACTIVE
 *   FCCH     nothing is computed; with ACTIVE sent = 1 and flags = TRXHIP_MS_IND_TRASH (:189-192), bits zero
 *   traffic  with ACTIVE: pow = energyDetect(x, 80), gr-gsm's channel estimate on training sequence tsc (59 lags), start clamped to
 *            [-39, 39], detect_burst_nb; sent = 1, toa256 = 0, rssi = (int)floor(20.0 * log10(rx_full_scale / sqrtf(pow))).  An
 *            all-zero slot (pow == 0, where the reference divides by zero): rssi = 0, flags = TRXHIP_MS_IND_SILENT, bits and start
 *            as the receiver gives them.  Without ACTIVE: sent = 0, nothing computed, zeros
 *   BAD      tn > 7, or a traffic slot with tsc > 7: sent = 0, nothing computed, zeros
 * d_bits (may be NULL): int8 [n_slots][148], +-127 with -127 a one; zeros where nothing was demodulated.
 * -TRXHIP_EINVAL (nothing launched, nothing written): a NULL ctx, d_iq, d_slots or d_ind, n_slots == 0, slot_stride < 625,
 * rx_full_scale not finite or <= 0. */
#define TRXHIP_MS_KIND_BAD 0    /* tn > 7, or a traffic slot with tsc > 7 */
#define TRXHIP_MS_KIND_FCCH 1   /* gsm_fcch_check_ts(): tn == 0 && fn % 51 in {0, 10, 20, 30, 40} (ms/sch.c:100-135) */
#define TRXHIP_MS_KIND_SCH 2    /* gsm_sch_check_ts(): tn == 0 && fn % 51 in {1, 11, 21, 31, 41} */
#define TRXHIP_MS_KIND_NB 3     /* every other slot */
#define TRXHIP_MS_SLOT_ACTIVE 1 /* trxcon answered the RTR indication with TRXCON_PHYIF_RTR_F_ACTIVE (ms_upper.cpp:183-187) */
#define TRXHIP_MS_IND_TRASH 1   /* FCCH slot: the reference returns true without writing anything (:189-192) */
#define TRXHIP_MS_IND_SILENT 2  /* traffic slot whose energyDetect() is 0: the reference's RSSI is undefined there */
typedef struct {             /* 8 bytes */
	uint32_t fn;         /* 0 */
	uint8_t tn;          /* 4 */
	uint8_t tsc;         /* 5: the cell's training sequence (traffic slots) */
	uint8_t flags;       /* 6: TRXHIP_MS_SLOT_* */
	uint8_t reserved;    /* 7 */
} trxhip_ms_slot;
typedef struct {             /* 32 bytes */
	uint32_t fn;         /* 0 */
	uint8_t tn;          /* 4 */
	uint8_t kind;        /* 5: TRXHIP_MS_KIND_* */
	uint8_t sent;        /* 6: 1 where driveReceiveFIFO() would call trxcon_phyif_handle_burst_ind */
	uint8_t flags;       /* 7: TRXHIP_MS_IND_* */
	int16_t rssi;        /* 8 */
	int16_t toa256;      /* 10 */
	int32_t start;       /* 12: burst start in samples, after the +-39 clamp (SCH, traffic); else 0 */
	float corr_max;      /* 16: largest |correlation| of the 20-tap channel estimate */
	float pow;           /* 20: energyDetect()'s return (traffic); else 0 */
	int32_t sch_fn;      /* 24: SCH with good parity: gsm_sch_to_fn(); else -1 */
	uint8_t sch_rc;      /* 28: 1 = SCH decoded */
	uint8_t sch_bsic;    /* 29 */
	uint8_t reserved[2]; /* 30: zero */
} trxhip_ms_burst_ind;
int trxhip_ms_rx_batch_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t slot_stride, const trxhip_ms_slot *d_slots,
			   trxhip_ms_burst_ind *d_ind, int8_t *d_bits, size_t n_slots, float rx_full_scale, void *stream);
int trxhip_ms_rx_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, size_t slot_stride, const trxhip_ms_slot *d_slots,
			    trxhip_ms_burst_ind *d_ind, int8_t *d_bits, size_t n_slots, float rx_full_scale, void *stream);

/* delayVector() (sigProcLib.h:97, sigProcLib.cpp:1046-1098) for n_vec complex64 vectors of `len` samples, one delay
 * (in samples) per vector in d_delays: 64-phase 20-tap fractional filter when |frac| > 0.01, then the integer shift
 * with zero fill.  d_out must not alias d_in. */
int trxhip_delay_vector_batch_cf32(trxhip_ctx *ctx, const float *d_in_cf32, float *d_out_cf32, const float *d_delays,
				   size_t n_vec, int len, void *stream);

/* scaleVector() (sigProcLib.h:94, sigProcLib.cpp:1188-1213): in-place x[i] *= (scale_re + j scale_im) over `len`
 * complex64 samples. */
int trxhip_scale_vector_cf32(trxhip_ctx *ctx, float *d_x_cf32, size_t len, float scale_re, float scale_im, void *stream);

/* The Viterbi alternative of pullRadioVector (cfg->use_va): scaleVector(burst, scale) + demodAnyBurst_va()
 * (Transceiver.cpp:782-784 with scale = 1/16383, :620-645) over gr-gsm's 4-samples-per-symbol MLSE receiver in
 * Transceiver52M/grgsm_vitac/ (get_norm_chan_imp_resp / get_access_imp_resp, detect_burst_nb / _ab, viterbi_detector).
 * d_iq_cf32: n_bursts x burst_len complex64, the burst as that path sees it (it starts 20 samples before the one the
 * detector looks at, Transceiver.cpp:760-762); d_params[b].type TSC selects the normal-burst branch, anything else
 * the access-burst branch (whose Viterbi start state is max_toa, as in the reference; >= 16 selects none); tsc 0..7.
 * d_soft[b][0..soft_stride): +-127 for the 148 (normal) / 88 (access) demodulated bits, 0 behind them; with
 * TRXHIP_FLAG_SLICE through vectorSlicer() (0 / 1).  d_starts (may be NULL): estimated burst start in samples.
 * Samples outside the burst read as 0.  soft_stride >= 148.
 * One deliberate deviation: at tsc 1 the MLSE receivers (this one, TRXHIP_FLAG_USE_VA, trxhip_ms_rx_batch_*) use the training
 * sequence of 3GPP TS 45.002, not row 1 of the reference's grgsm_vitac/constants.h, which has bit 20 inverted: the reference
 * correlates with one of its 16 taps negated there and loses bits.  Every other tsc equals the reference's compiled code bit for
 * bit; tsc 1 equals the same compiled code fed the 3GPP row (tests/test_vitac_ref_cpu.py, tests/test_gpu_vitac_ref.py).
 * d_detected (may be NULL): the result records of a preceding detection launch on the same batch; burst b is then
 * demodulated only if d_detected[b].rc > 0, with that rc as the CorrType (Transceiver.cpp:769-784); the others get
 * zeros and start -1.  This chains detection and the Viterbi demodulator on one stream without a host round trip. */
int trxhip_demod_va_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, const trxhip_burst_params *d_params,
			       const trxhip_burst_result *d_detected, float *d_soft, int32_t *d_starts, size_t n_bursts,
			       int burst_len, float scale, int soft_stride, int flags, void *stream);

/* energyDetect() on its own (sigProcLib.h:105, sigProcLib.cpp:1573-1585): mean |x|^2 of `window` samples at
 * stride 4 from sample 0 of each burst (complex64); d_energy: n_bursts floats. */
int trxhip_energy_detect_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, size_t n_bursts, int burst_len,
				    unsigned window, float *d_energy, void *stream);
/* vectorSlicer() (sigProcLib.h:63): dest = clamp(0.5*(src+1), 0, 1), device arrays */
int trxhip_vector_slicer(trxhip_ctx *ctx, float *d_dest, const float *d_src, size_t len, void *stream);

/* TRXD field quantisation into a fixed 156-byte record (a compact device-side format, NOT the wire format -- see
 * trxhip_pack_trxd_wire_batch below), proto_trxd.c:36-66:
 *   d_pkt: n_bursts * 156 bytes: [0..1] toa_int be16 (1/256 sym), [2] rssi u8 (-dBFS), [3..4] ci cB be16,
 *          [5] tsc, [6] idle, [7] nbits/4, [8..155] 148 soft bits uint8 = round(rx_burst*255) */
int trxhip_pack_trxd_batch(trxhip_ctx *ctx, const trxhip_burst_result *d_results, const float *d_soft_sliced,
			   int soft_stride, uint8_t *d_pkt, size_t n_bursts, float rssi_offset, void *stream);

/* TRXD v0 / v1 uplink burst indications in wire format: byte for byte what trxd_send_burst_ind_v0() / _v1()
 * hand to write() (proto_trxd.c:68-117; struct trxd_hdr_common / _v0_specific / _v1_specific, proto_trxd.h:56-106):
 *   [0]     version << 4 | tn & 7             trxd_fill_common()        proto_trxd.c:28-34
 *   [1..4]  fn, big endian
 *   [5]     rssi = (uint8_t) bi->rssi         trxd_fill_v0_specific()   :36-45   (rssi = result.rssi + rssi_offset)
 *   [6..7]  (int)(toa * 256.0 + 0.5), be16
 *   v0:  [8..8+nbits) soft bits, then two trailing bytes (the reference leaves the first uninitialised and zeroes the
 *        second, :83-87; both are 0 here); idle indications are not sent (length 0, :71-73)
 *   v1:  [8] idle << 7 | modulation << 3 | tsc & 7    trxd_fill_v1_specific() :47-60; modulation = GMSK: tss & 3,
 *        8-PSK: 4 | tss & 1 (TRXD_MODULATION_*, proto_trxd.h:84-88); [9..10] (int16)(ci * 10 + 0.5) be16;
 *        [11..11+nbits) soft bits unless idle (:100-109)
 *   soft bits: (uint8_t) round(rx_burst[i] * 255.0), nbits = 148 (GMSK) or 444 (8-PSK)     :62-66
 * An idle indication carries toa = ci = tsc = 0 and GMSK, as pullRadioVector() leaves them (Transceiver.cpp:694-704,
 * ret_idle :808-814).  A slot that is OFF produces nothing (pullRadioVector() returns -ENOENT, :704-707): length 0.
 * rssi outside 0..255 (or NaN) is undefined behaviour in the reference's double -> uint8_t conversion; here it
 * saturates.
 *   d_results, d_params : the records of the detect/demod launch over the same batch (d_params gives OFF)
 *   d_soft_sliced       : its soft output with TRXHIP_FLAG_SLICE, soft_stride >= 148 (>= 444 for 8-PSK rows)
 *   d_meta              : per burst {fn, tn, version 0|1, tss}
 *   d_pkt               : n_bursts x pkt_stride bytes, pkt_stride a multiple of 4 and >= 160 (>= 456 when 8-PSK rows
 *                         are possible; a datagram that does not fit is truncated to pkt_stride); burst b's datagram
 *                         starts at d_pkt + b * pkt_stride, bytes behind its length are 0
 *   d_pkt_len           : n_bursts datagram lengths (0 = nothing to send) */
typedef struct trxhip_trxd_meta {
	uint32_t fn;        /* TDMA frame number */
	uint8_t  tn;        /* timeslot 0..7 */
	uint8_t  version;   /* TRXD header version negotiated for the channel: 0 or 1 (mVersionTRXD[chan]) */
	uint8_t  tss;       /* training sequence set (the reference always sends 0, Transceiver.cpp:703) */
	uint8_t  reserved;
} trxhip_trxd_meta;
#define TRXHIP_TRXD_V0_HDR   8
#define TRXHIP_TRXD_V1_HDR  11
#define TRXHIP_TRXD_MAX_PKT (TRXHIP_TRXD_V1_HDR + 444)
int trxhip_pack_trxd_wire_batch(trxhip_ctx *ctx, const trxhip_burst_result *d_results, const trxhip_burst_params *d_params,
				const float *d_soft_sliced, int soft_stride, const trxhip_trxd_meta *d_meta,
				uint8_t *d_pkt, int pkt_stride, uint16_t *d_pkt_len, size_t n_bursts, float rssi_offset,
				void *stream);

/* ---- host-fed, stream-pipelined form of the hot path (host buffers in, host buffers out) ----
 * pullRadioVector()'s callers hold their bursts in host memory.  A hostpipe owns `depth` staging slots of pinned
 * host memory, each with its own device buffers and HIP stream; a submitted slot runs
 *     H2D (iq, params, meta) -> trxhip_detect_demod_batch [-> trxhip_pack_trxd_wire_batch] -> D2H (results, soft | pkt)
 * asynchronously, so that slot k+1's upload, slot k's kernels and slot k-1's download overlap.  Nothing is
 * allocated after create.  The producer writes bursts straight into trxhip_hostpipe_slot_buffers().iq (no second
 * copy); trxhip_hostpipe_run() is the convenience form for pageable caller buffers (it copies through the slots). */
typedef struct trxhip_hostpipe trxhip_hostpipe;
typedef struct trxhip_hostpipe_cfg {
	uint32_t max_bursts;   /* capacity of one slot */
	int32_t  depth;        /* number of slots, 2..16 */
	int32_t  burst_len;    /* 625 at 4 SPS */
	int32_t  sps;
	int32_t  soft_stride;  /* floats per burst downloaded (148 / 156 / 444); 0 = no float soft output */
	int32_t  pkt_stride;   /* bytes per burst of TRXD datagrams downloaded (multiple of 4, >= 160); 0 = no TRXD packing */
	int32_t  flags;        /* TRXHIP_FLAG_*; TRXD packing implies TRXHIP_FLAG_SLICE.  TRXHIP_FLAG_USE_VA (here and in the uplink
	                        * burst scheduler's config): the cfg->use_va flow of pullRadioVector (Transceiver.cpp:760-787) -- the slot's bursts are what the radio
	                        * read 20 samples early; power / rssi come from them as read, detection runs on the copy shifted by 20
	                        * samples (zeros behind), the soft bits from scaleVector(1 / 16383) + demodAnyBurst_va() on the unshifted
	                        * burst (trxhip_demod_va_batch_cf32 chained behind the detection records): hard 0 / 1 rows of 148 */
	float    threshold;    /* TRXHIP_BURST_THRESH */
	float    full_scale;
	float    rssi_offset;  /* enters the TRXD rssi byte only; result.rssi stays without it */
	int32_t  n_paths;      /* diversity paths per burst (0 or 1: none).  > 1: a slot's iq holds max_bursts x n_paths x burst_len
	                        * samples, every submit runs trxhip_select_diversity_batch() first and
	                        * trxhip_apply_diversity_power() behind the detector (Transceiver.cpp:723-751) */
} trxhip_hostpipe_cfg;
typedef struct trxhip_hostpipe_slot {      /* pinned host memory, valid until trxhip_hostpipe_destroy() */
	int16_t             *iq;       /* in : max_bursts x [n_paths x] burst_len x 2 */
	trxhip_burst_params *params;   /* in : max_bursts */
	trxhip_trxd_meta    *meta;     /* in : max_bursts (NULL without TRXD packing) */
	trxhip_burst_result *results;  /* out: max_bursts */
	float               *soft;     /* out: max_bursts x soft_stride (NULL when soft_stride = 0) */
	uint8_t             *pkt;      /* out: max_bursts x pkt_stride  (NULL when pkt_stride = 0) */
	uint16_t            *pkt_len;  /* out: max_bursts */
} trxhip_hostpipe_slot;
int  trxhip_hostpipe_create(trxhip_ctx *ctx, const trxhip_hostpipe_cfg *cfg, trxhip_hostpipe **out);
void trxhip_hostpipe_destroy(trxhip_hostpipe *p);
int  trxhip_hostpipe_slot_buffers(trxhip_hostpipe *p, int slot, trxhip_hostpipe_slot *out);
/* change the scalar parameters of later submits (detection threshold, rxFullScale, rssi_offset) without touching the
 * staging buffers: callers whose channels differ in full scale share one pipe */
int  trxhip_hostpipe_set_levels(trxhip_hostpipe *p, float threshold, float full_scale, float rssi_offset);
/* enqueue slot's first n_bursts bursts; returns at once.  The slot's buffers must not be touched until wait(). */
int  trxhip_hostpipe_submit(trxhip_hostpipe *p, int slot, size_t n_bursts);
/* block until the slot's job has finished (TRXHIP_OK), or return TRXHIP_EIO if it failed */
int  trxhip_hostpipe_wait(trxhip_hostpipe *p, int slot);
/* 0 = finished (or never submitted), 1 = still running, < 0 error */
int  trxhip_hostpipe_query(trxhip_hostpipe *p, int slot);
/* ---- bursts by reference (round 5): no CPU copy of the samples at all ----
 * The reference cuts every burst out of the radio's receive ring with one CPU copy (radioInterface.cpp:272-291,
 * unRadioifyVector into a new radioVector); writing the burst into slot.iq is that copy.  When the ring itself is
 * registered with the pipe, a slot can instead carry one host POINTER per burst: submit_by_ref() uploads only
 * [params][meta], and a device kernel fetches the n bursts from the ring over the link (burst_len x 4 bytes from
 * each pointer, x n_paths with diversity) into the slot's device buffer; everything behind is trxhip_hostpipe_submit().
 * Contract: every src[i] is 4-byte aligned and lies, with its whole burst, inside one registered range (TRXHIP_EINVAL
 * otherwise, nothing enqueued); the samples stay unchanged until wait() on the slot has returned.
 * register_host: pins [base, base + bytes) and maps it into the device's address space (hipHostRegister; a range some
 * other pipe of the process has registered already is shared -- accepted only if that registration is mapped and covers
 * the whole range, TRXHIP_EINVAL otherwise; the sharing pipe does not own the pin: whoever registered first must outlive
 * every pipe that shares the range, which is how a multi-device gatherer destroys its pipes -- in reverse order of creation);
 * round 6: runs of 16 or more addresses a constant step apart are moved by the copy engine (one copy per run), the rest by
 * the fetch kernel; at most 8 ranges per pipe; unregister_host (or destroy)
 * releases what this pipe pinned -- before the memory is freed, and with no slot that refers to the range in flight.
 * register / unregister are not synchronised against submits of the same pipe on other threads. */
int  trxhip_hostpipe_register_host(trxhip_hostpipe *p, const void *base, size_t bytes);
int  trxhip_hostpipe_unregister_host(trxhip_hostpipe *p, const void *base);
/* the slot's pointer array: max_bursts entries of pinned host memory, valid until trxhip_hostpipe_destroy() */
int  trxhip_hostpipe_slot_sources(trxhip_hostpipe *p, int slot, const int16_t ***out_src);
int  trxhip_hostpipe_submit_by_ref(trxhip_hostpipe *p, int slot, size_t n_bursts);
/* Pageable buffers: n bursts are cut into slot-sized chunks, staged, processed with all slots in flight and copied
 * out.  h_meta / h_soft / h_pkt / h_pkt_len may be NULL (must be NULL when the pipe was created without them). */
int  trxhip_hostpipe_run(trxhip_hostpipe *p, const int16_t *h_iq, const trxhip_burst_params *h_params,
			 const trxhip_trxd_meta *h_meta, trxhip_burst_result *h_results, float *h_soft, uint8_t *h_pkt,
			 uint16_t *h_pkt_len, size_t n_bursts);

/* ---- arch kernels, batched (arch/common/convolve.h:6-14, convert.h:9) ----
 * y[b][i] = sum_k x[b][i + start - (h_len-1) + k] * h[k]  (correlation form, no tap flip), b < n_vec.
 * x: n_vec * x_len complex64; the caller guarantees start >= h_len-1 and start+len <= x_len
 * (the reference's bounds_check(), convolve_base.c:88-105 -> returns TRXHIP_EINVAL otherwise).
 * h: h_len complex64 on device (imag ignored for _real). */
int trxhip_convolve_real_batch(trxhip_ctx *ctx, const float *d_x, int x_len, const float *d_h, int h_len,
			       float *d_y, int y_len, int start, int len, size_t n_vec, void *stream);
int trxhip_convolve_complex_batch(trxhip_ctx *ctx, const float *d_x, int x_len, const float *d_h, int h_len,
				  float *d_y, int y_len, int start, int len, size_t n_vec, void *stream);
int trxhip_convert_short_float(trxhip_ctx *ctx, float *d_out, const int16_t *d_in, size_t len, void *stream);
/* convert_float_short() in its generic-C form (convert.h:6, convert_base.c:20-25): out[i] = (short)(in[i] * scale) */
int trxhip_convert_float_short(trxhip_ctx *ctx, int16_t *d_out, const float *d_in, float scale, size_t len, void *stream);
/* cxvec_fft() (fft.h:6-11, fft.c:55-114): `howmany` M-point DFTs, transform t reading d_in[j*istride + t] and writing
 * d_out[k*ostride + t] (complex64 units), forward (reverse = 0) or backward, unnormalised -- the layout of the
 * reference's fftwf_plan_many_dft() call.  d_out must not alias d_in. */
int trxhip_dft_batch(trxhip_ctx *ctx, const float *d_in, float *d_out, int m, size_t howmany, size_t istride, size_t ostride,
		     int reverse, void *stream);

/* ---- Channelizer::rotate (M-path polyphase analysis bank + M-point DFT), batched over blocks ----
 * d_in : n_blocks * block_len * m wideband samples as int16 IQ (a continuous stream; block j's
 *        filter history is the tail of block j-1, zero for block 0 -- Channelizer.cpp:86-88)
 * d_out: m * (n_blocks * block_len) complex64, channel-major (outputBuffer(chan), Channelizer.cpp:60-66) */
int trxhip_channelize_batch(trxhip_ctx *ctx, const int16_t *d_in, float *d_out,
			    size_t n_blocks, int m, int block_len, int h_len, void *stream);
/* Resampler(p,q,16)::rotate over a continuous stream per channel: in n_in samples -> out n_in*p/q.  (p,q) = (65,48), (1,4) and
 * RadioInterfaceResamp's receive ratios (65,96) and (52,75) with cutoff 1.0; TRXHIP_ENOTSUP otherwise. */
int trxhip_resample_batch(trxhip_ctx *ctx, const float *d_in, float *d_out, size_t n_in, int p, int q,
			  size_t n_chan, size_t in_stride, size_t out_stride, void *stream);

/* Synthesis(m, block_len, h_len)::rotate batched over blocks: the counterpart of trxhip_channelize_batch (m = 4, h_len = 16,
 * TRXHIP_ENOTSUP otherwise).  A forward, unnormalised 4-point DFT across the m rows at every time (cxvec_fft), the 16-tap
 * path filters (convolve_real with ChannelizerBase's sub-filters), the interleave out[m*t + k] = y_k[t] (Synthesis.cpp:39-50).
 * d_in : m rows x (n_blocks*block_len) complex64, row c at d_in + 2*c*in_stride (Synthesis::inputBuffer(c))
 * d_out: n_blocks*block_len*m complex64, interleaved; zero history before block 0, carried between blocks */
int trxhip_synthesize_batch(trxhip_ctx *ctx, const float *d_in, size_t in_stride, float *d_out,
			    size_t n_blocks, int m, int block_len, int h_len, void *stream);

/* ---- transmit side: the GMSK / 8-PSK burst modulators of sigProcLib.cpp, batched ----
 * modulateBurst()       sigProcLib.cpp:970-979   (Transceiver.cpp:392-396, :107-120 through the burst generators)
 *   modulateBurstLaurent  :595-670  GMSK at 4 SPS: c0 through the 16-tap pulse + c1 through the 8-tap pulse, 625 samples
 *   modulateBurstBasic    :938-967  GMSK at 1 SPS: one 4-tap pulse, nbits + guard samples
 *   rotateBurst           :558-580  empty pulse: rotation only, sps * (nbits + guard) samples
 * modulateEdgeBurst()   sigProcLib.cpp:917-936
 *   mapEdgeSymbols + shapeEdgeBurst :713-763  8-PSK at 4 SPS, delayed by one symbol, 625 samples
 *   rotateEdgeBurst       :672-689  empty pulse: rotation only, sps * nbits / 3 samples
 * Every sample is bit-identical to the reference's generic-C arithmetic.  Only bit 0 of each input byte
 * counts (bits[i] & 0x01, as in the reference).
 *
 * Descriptor ranges; a burst outside them gets status TRXHIP_EINVAL and a zero row.  Some of these cases are undefined
 * behaviour in the reference and are refused rather than reproduced:
 *   GMSK, 4 SPS          2 <= nbits <= 155 (guard ignored, as in the reference).  nbits == 156 writes c0[4 * (nbits + 1)],
 *                        past the reference's 625-sample buffer; nbits < 2 reads bits[-1] (:654-656)
 *   GMSK, 1 SPS          1 <= nbits + guard <= 157 (GMSKRotation1 has 157 entries)
 *   GMSK, empty pulse    1 <= sps * (nbits + guard) <= 625 at 4 SPS, <= 157 at 1 SPS.  At 4 SPS guard 9 (148 + 9 = 157
 *                        symbols, 628 samples) reads GMSKRotation4[625..627], past the table
 *   8-PSK, 4 SPS         nbits % 3 == 0, nbits <= 468 (156 symbols fill the 625 samples)
 *   8-PSK, empty pulse   nbits % 3 == 0, 3 <= nbits <= 468, any sps of the call
 *   8-PSK shaped at 1 SPS: refused (the reference returns NULL, :923-924)
 *   always               nbits <= bits_stride, length <= out_stride, no unknown flag bits */
#define TRXHIP_TX_8PSK         1   /* modulateEdgeBurst() instead of modulateBurst() */
#define TRXHIP_TX_EMPTY_PULSE  2   /* emptyPulse = true: rotation only */
typedef struct trxhip_tx_params {
	uint16_t nbits;      /* bits of the burst (bytes at d_bits + b * bits_stride) */
	uint8_t  guard;      /* guardPeriodLength (GMSK at 1 SPS and the empty pulse) */
	uint8_t  flags;      /* TRXHIP_TX_* */
	float    scale_re;   /* complex scale applied after modulation, as scaleVector() does (sigProcLib.cpp:1188-1213): */
	float    scale_im;   /* (a.re*s.re - a.im*s.im, a.re*s.im + a.im*s.re).  Exactly (1, 0): the row is left unscaled */
	uint32_t reserved;
} trxhip_tx_params;
/* n bursts, one launch:
 *   d_bits     : n x bits_stride bytes
 *   d_params   : n trxhip_tx_params
 *   d_out_cf32 : n x out_stride complex64 (may be NULL); samples behind a burst's length are 0
 *   d_out_s16  : n x out_stride x (I, Q) int16 (may be NULL): (int16_t)(int)(x * s16_scale) per component, the expression of
 *                trxhip_convert_float_short().  4-SPS bursts in TN order at out_stride 625 are one TDMA frame's sample stream
 *   d_out_len  : n int32 (may be NULL): the burst's length in samples, or TRXHIP_EINVAL for a refused descriptor
 *   sps        : 1 or 4 (the reference's tx_sps)
 * Asynchronous on `stream`.  TRXHIP_EINVAL without a context: there is no CPU path. */
int trxhip_modulate_batch(trxhip_ctx *ctx, const uint8_t *d_bits, size_t bits_stride, const trxhip_tx_params *d_params,
			  float *d_out_cf32, int16_t *d_out_s16, float s16_scale, size_t out_stride, int32_t *d_out_len,
			  size_t n, int sps, void *stream);

/* TRXD downlink datagrams to burst samples: Transceiver::driveTxPriorityQueue() + addRadioVector()
 * (Transceiver.cpp:1087-1185, :373-399), parsed on the device.  Datagram b (struct trxd_hdr_v01_dl + bits, proto_trxd.h):
 *   [0]     version << 4 | tn & 7 (version 0 or 1)   [1..4] fn, big endian   [5] tx_att (dB)   [6..] one bit per byte
 *   length  6 + 148: GMSK, modulateBurst(bits, 8 + (tn % 4 == 0), sps)
 *           6 + 444: 8-PSK, modulateEdgeBurst(bits, sps); only at 4 SPS (status TRXHIP_ENOTSUP otherwise, :1112-1116)
 *   scale   (float)(full_scale * pow(10, (double)-tx_att / 20)), the expression of :396 with txFullScale = full_scale
 * A datagram of any other length or version gets status TRXHIP_EINVAL; refused datagrams get a zero row (the reference
 * drops them).  The FN-order bookkeeping (:1137-1171) and the filler table stay with the caller.
 *   d_dgram     : n x dgram_stride bytes (dgram_stride >= 6; a datagram longer than dgram_stride is refused)
 *   d_dgram_len : n uint16
 *   d_info      : n trxhip_tx_info (may be NULL); outputs as trxhip_modulate_batch() */
typedef struct trxhip_tx_info {
	uint32_t fn;        /* TDMA frame number */
	uint8_t  tn;        /* timeslot */
	uint8_t  version;   /* TRXD header version */
	uint8_t  tx_att;    /* attenuation, dB */
	uint8_t  mod_8psk;  /* 1: 8-PSK burst */
	uint16_t nbits;     /* 148, 444, or 0 when refused */
	uint16_t length;    /* samples written, 0 when refused */
	int32_t  status;    /* 0 or TRXHIP_E* */
} trxhip_tx_info;
int trxhip_modulate_trxd_batch(trxhip_ctx *ctx, const uint8_t *d_dgram, size_t dgram_stride, const uint16_t *d_dgram_len,
			       double full_scale, int sps, float *d_out_cf32, int16_t *d_out_s16, float s16_scale,
			       size_t out_stride, trxhip_tx_info *d_info, size_t n, void *stream);

/* The transmit table struct (csrc/trx_tx_tables.h), host-only, no GPU needed: pulses, rotations, 8-PSK map and phasors, burst
 * bit patterns */
size_t trxhip_tx_tables_size(void);
int  trxhip_tx_tables_generate_host(void *h_buf, size_t size);

/* ---- streaming multi-ARFCN receive front end: RadioInterfaceMulti::pullBuffer(), radioInterfaceMulti.cpp:237-314 ----
 * Channelizer(4, block_len, 16)::rotate followed by Resampler(p, q, 16)::rotate on every filterbank channel, called
 * chunk after chunk: the object carries what the reference carries between calls (Channelizer::hist,
 * Channelizer.cpp:86-88; history[lchan], radioInterfaceMulti.cpp:283-300), so any chunking of a stream gives the
 * result of processing it in one piece.  (p,q) = (65,48) in RadioInterfaceMulti; RadioInterfaceResamp uses the
 * same Resampler with (65,96) and (52,75), radioInterfaceResamp.cpp:36-41: block_len must be a multiple of q. */
typedef struct trxhip_rx_frontend trxhip_rx_frontend;
int  trxhip_rx_frontend_create(trxhip_ctx *ctx, int block_len, int p, int q, trxhip_rx_frontend **out);
void trxhip_rx_frontend_destroy(trxhip_rx_frontend *f);
int  trxhip_rx_frontend_reset(trxhip_rx_frontend *f, void *stream);           /* zero the carried history */
/* Start mid-stream (a stream is sharded in time, one shard per GPU, with overlap at the shard edges): make the
 * carried state what it would be had the stream been processed up to the shard's first block.  d_wide_prev = the
 * n_blocks_prev >= 1 blocks (n_blocks_prev * block_len * 4 wideband int16 IQ samples, 16-byte aligned) that immediately
 * precede the shard; one block is enough, because both filters are FIR -- the channelizer carries 15 time steps
 * (Channelizer::hist, Channelizer.cpp:86-88), the resampler 15 channel samples (history[lchan],
 * radioInterfaceMulti.cpp:283-300).  The shard's output is then bit-identical to the same blocks' output of an unsharded
 * run.  n_blocks_prev = 0 (stream start) is trxhip_rx_frontend_reset(). */
int  trxhip_rx_frontend_seed(trxhip_rx_frontend *f, const int16_t *d_wide_prev, size_t n_blocks_prev, void *stream);
/* d_wide: n_blocks * block_len * 4 wideband int16 IQ samples (16-byte aligned);
 * d_out : 4 channels x (n_blocks*block_len*p/q) complex64, channel c at d_out + 2*c*out_stride floats.
 * Objects of trxhip_rx_frontend_create_chans(): d_wide and the rows of d_out as described there. */
int  trxhip_rx_frontend_pull(trxhip_rx_frontend *f, const int16_t *d_wide, size_t n_blocks, float *d_out,
			     size_t out_stride, void *stream);

/* The receive front end per logical channel: what RadioInterfaceMulti::pullBuffer() and RadioInterfaceResamp::pullBuffer()
 * (radioInterfaceResamp.cpp:156-193) compute, and nothing else.  trxhip_rx_frontend_create() and every object it makes keep
 * their behaviour (four rows, physical order); _destroy, _reset, _seed and _pull accept both kinds of object.
 * MULTI : chans 1..3 logical channels.  pullBuffer() skips the inactive filterbank paths and writes recvBuffer[lchan]
 *         (:237-314); the active paths and their order are radioInterfaceMulti.cpp:92-124, :214-231 -- 1 chan: lchan 0 <- path 0;
 *         2: 0 <- 0, 1 <- 3; 3: 0 <- 1, 1 <- 0, 2 <- 3.  d_wide as above; _pull writes chans rows, logical channel l at
 *         d_out + 2*l*out_stride floats.  Nothing is computed or stored for an inactive path; row l is bit-identical to row
 *         pchan(l) of a four-row object fed the same stream, under any chunking.
 * RESAMP: chans == 1.  d_wide is n_blocks*block_len int16 IQ samples of the one channel (4-byte aligned), block_len the
 *         device-side chunk (1536 for (65,96), 1200 for (52,75) at 4 SPS); convert_short_float, then Resampler(p, q, 16) with
 *         Resampler::init()'s default cutoff 1.0 (Resampler.h:44); one row of n_blocks*block_len/q*p samples.  The object carries
 *         dnsampler->len() = 16 input samples between calls (:146-147, :191), zero at a fresh or reset object; _seed takes the
 *         preceding blocks in this layout.
 * Refused with TRXHIP_EINVAL: no context or no `out`, an unknown mode, chans outside 1..3 (MULTI) or != 1 (RESAMP),
 * block_len < 16, p outside 1..128, q outside 1..3072, block_len % q != 0, q * ceil(256 / p) > 3072. */
#define TRXHIP_RXFE_MULTI  0   /* RadioInterfaceMulti::pullBuffer: Channelizer(4) + Resampler(p,q) on the active paths */
#define TRXHIP_RXFE_RESAMP 1   /* RadioInterfaceResamp::pullBuffer: convert_short_float + Resampler(p,q), chans == 1 */
int trxhip_rx_frontend_create_chans(trxhip_ctx *ctx, int mode, int chans, int block_len, int p, int q,
                                    trxhip_rx_frontend **out);
int trxhip_rx_frontend_rows(const trxhip_rx_frontend *f);   /* rows pull() writes: 4 for trxhip_rx_frontend_create() objects */
/* samples per row a pull of n_blocks writes: n_blocks*block_len/q*p (0 for NULL); host arithmetic only */
size_t trxhip_rx_frontend_out_samples(const trxhip_rx_frontend *f, size_t n_blocks);

/* ---- streaming transmit front end: RadioInterfaceMulti::pushBuffer() (radioInterfaceMulti.cpp:316-362) and
 * RadioInterfaceResamp::pushBuffer() (radioInterfaceResamp.cpp:196-230) ----
 * MULTI : chans 1..3 logical channels at the low rate; Resampler(p, q, 16) per active filterbank path (1 chan: path 0 <-
 *         lchan 0; 2: 0 <- 0, 3 <- 1; 3: 0 <- 1, 1 <- 0, 3 <- 2: radioInterfaceMulti.cpp:92-124, :214-231), zero rows on the
 *         others, then Synthesis(4, block_len*p/q, 16).  The reference: Resampler(48, 65) at block_len 260.
 * RESAMP: chans == 1, Resampler(p, q, 16) alone: (96, 65) at 64 MHz clocking and block_len 260, (75, 52) at 100 MHz and 208.
 * bw is Resampler::init's cutoff: 1.0 in RadioInterfaceMulti, 0.45 in RadioInterfaceResamp at tx_sps 4, 1.0 otherwise.
 * The object carries what the reference carries between calls (the RadioBuffer headroom in front of every segment,
 * radioBuffer.cpp:29-47, and Synthesis::hist), so any chunking of a stream gives the result of processing it in one
 * piece; a fresh or reset object starts from zero history.
 * Refused with TRXHIP_EINVAL: no context, an unknown mode, chans outside 1..3 (MULTI) or != 1 (RESAMP), p outside 1..128,
 * q < 1, block_len % q != 0, q * ceil(256 / p) > 3072, bw not positive. */
#define TRXHIP_TXFE_MULTI  0   /* RadioInterfaceMulti::pushBuffer: chans 1..3, per-path Resampler(p,q) + Synthesis(4) */
#define TRXHIP_TXFE_RESAMP 1   /* RadioInterfaceResamp::pushBuffer: chans == 1, Resampler(p,q) only */
typedef struct trxhip_tx_frontend trxhip_tx_frontend;
int  trxhip_tx_frontend_create(trxhip_ctx *ctx, int mode, int chans, int block_len, int p, int q, float bw,
			       trxhip_tx_frontend **out);   /* block_len = low-rate samples per block per channel */
void trxhip_tx_frontend_destroy(trxhip_tx_frontend *f);
int  trxhip_tx_frontend_reset(trxhip_tx_frontend *f, void *stream);   /* zero the carried history */
/* Start mid-stream: the carried state of a stream processed up to here.  d_in_prev holds the n_blocks_prev blocks that
 * immediately precede the shard, laid out as d_in of trxhip_tx_frontend_push(); one block suffices, because every filter
 * is FIR with at most 15 + ceil(15 q / p) low-rate samples of memory.  n_blocks_prev = 0 is trxhip_tx_frontend_reset(). */
int  trxhip_tx_frontend_seed(trxhip_tx_frontend *f, const float *d_in_prev, size_t in_stride, size_t n_blocks_prev,
			     void *stream);
/* d_in: chans logical channels, complex64, lchan l at d_in + 2*l*in_stride, n_blocks*block_len samples each.
 * Output per block: MULTI 4*block_len*p/q wideband samples, RESAMP block_len*p/q.
 * d_out_cf32 and/or d_out_s16 (at least one non-NULL); s16 = (int16_t)(int)(x * s16_scale), the expression of
 * trxhip_convert_float_short().  RadioInterfaceMulti passes s16_scale = (float)(1.0 / chans). */
int  trxhip_tx_frontend_push(trxhip_tx_frontend *f, const float *d_in, size_t in_stride, size_t n_blocks,
			     float *d_out_cf32, int16_t *d_out_s16, float s16_scale, void *stream);

/* ---- downlink burst scheduler: TRXD datagrams to each channel's transmit sample stream ----
 * For batch callers ("datagrams in, radio samples out"); osmo-trx linked through the shims keeps its own Transceiver.
 * Per logical channel (1..8) the object keeps what Transceiver keeps (Transceiver.cpp): the priority queue of bursts by
 * GSM::Time (FN modulo the hyperframe 2715648 through FNDelta / FNCompare, then TN), the per-TN FN-order state of
 * driveTxPriorityQueue() (:1137-1171), the filler table [102][8] (:95-135; channel 0 holds the configured filler, every
 * other channel FILLER_ZERO, :255-256; retransmission into it on channel 0 exactly when the filler is FILLER_DUMMY,
 * :218-219), the slot combinations with setModulus()'s moduli 26 / 51 / 102 / 52 (:483-512) and the RF mute flag.
 * A render of n slots runs pushRadioVector()'s loop body (:416-481) for every slot from the clock, then advances the clock
 * (incTN): stale bursts are dropped (the filler table updated first when retransmission is on), the current burst goes out
 * (and into the filler table when retransmission is on), otherwise the filler entry fillerTable[FN % modulus[TN]][TN]; a slot
 * whose combination is NONE or whose channel is muted is zeros and still consumes its burst.
 * Duplicate times: of two queued bursts with the same (FN, TN) the earlier submission is transmitted and the later one is
 * dropped as stale in the next slot (the reference's std::priority_queue leaves the order unspecified).
 * Submit refuses, counting it in `refused` and queueing nothing: a length other than 6 + 148 (GMSK) or 6 + 444 (8-PSK; at
 * 1 SPS refused too), a header version above 1.  A repeated FN of a TN is dropped (tx_trxd_fn_repeated); an earlier FN is
 * counted (tx_trxd_fn_outoforder) and queued; a later FN past the next on channel 0 with FILLER_ZERO counts the FNs lost
 * (tx_trxd_fn_skipped).  Random fillers (FILLER_NORM_RAND & co.) are not offered: they use rand().
 * Samples: slot s of a render starts at s * 625 (4 SPS) or at its 1-SPS offset (slots of 157 / 156 / 156 / 156 / 157 / 156 /
 * 156 / 156 samples from TN 0, a frame 1250) counted from the render's first slot.  A burst slot is the row
 * trxhip_modulate_trxd_batch() gives its datagram; the dummy filler is modulateBurst(dummy, 8 + (tn % 4 == 0), sps) scaled by
 * (full_scale, 0); other slots are zeros.
 * Blocking: submit waits (hipEventSynchronize) only when all 2 * chans * queue_cap staging rows are taken, i.e. when renders
 * still in flight hold more than chans * queue_cap consumed rows; render and render_frontend wait only for the render issued
 * 4 calls earlier on the object (its slot buffer is reused).  render_frontend also allocates its remainder buffer (hipMalloc,
 * which may wait for the device) on its first call and again, after hipStreamSynchronize on `stream`, when a front end with
 * a longer block_len is attached; the buffer is sized for max_slots from any TN, so the clock never makes it grow.  Nothing
 * calls hipDeviceSynchronize.  Issue every render of one object on one stream.  One object is not thread-safe.
 * TRXHIP_EIO from a render (a failed copy or launch, after hipStreamSynchronize on `stream`): the queue and the filler
 * table have moved on while the device's filler entries have not; the object is unusable and must be destroyed.
 * ctx == NULL: a plan-only object (no device memory, no outputs); the queue logic and trxhip_tx_sched_plan() as on the GPU.
 * Every refusal of an argument (config, channel, TN, combination, render before set_clock, more slots than max_slots, a
 * front end whose chans differ, outputs too small) is TRXHIP_EINVAL and leaves the state untouched. */
#define TRXHIP_FILLER_DUMMY 0     /* FillerType FILLER_DUMMY */
#define TRXHIP_FILLER_ZERO  1     /* FillerType FILLER_ZERO */
#define TRXHIP_COMB_FILL     0    /* Transceiver::ChannelCombination FILL, I .. XIII = 1 .. 13, NONE, LOOPBACK */
#define TRXHIP_COMB_NONE     14
#define TRXHIP_COMB_LOOPBACK 15
typedef struct trxhip_tx_sched_cfg {
	int32_t  chans;          /* logical channels, 1..8 */
	int32_t  sps;            /* 1 or 4 */
	int32_t  filler;         /* TRXHIP_FILLER_DUMMY or TRXHIP_FILLER_ZERO (channel 0) */
	int32_t  queue_cap;      /* queued bursts per channel, 1 .. 2^20 (submit: TRXHIP_ENOMEM when full) */
	uint64_t max_slots;      /* the largest render, slots per channel, 1 .. 2^26 */
	double   full_scale;     /* txFullScale */
} trxhip_tx_sched_cfg;
#define TRXHIP_TXS_SRC_ZERO   0   /* zeros: slot combination NONE or RF muted */
#define TRXHIP_TXS_SRC_BURST  1   /* a submitted burst, id = its submission id */
#define TRXHIP_TXS_SRC_FILLER 2   /* the filler entry, id = the submission id of the burst that wrote it, -1: initial filler */
typedef struct trxhip_tx_plan {
	int64_t  id;
	uint32_t fn;
	uint8_t  tn;
	uint8_t  src;            /* TRXHIP_TXS_SRC_* */
	uint8_t  reserved[2];
} trxhip_tx_plan;
typedef struct trxhip_tx_sched_ctrs {
	uint64_t tx_stale_bursts, tx_unavailable_bursts, tx_trxd_fn_repeated, tx_trxd_fn_outoforder, tx_trxd_fn_skipped;
	uint64_t refused;        /* datagrams refused at submit (length, version, 8-PSK at 1 SPS) */
} trxhip_tx_sched_ctrs;
typedef struct trxhip_tx_sched trxhip_tx_sched;
int  trxhip_tx_sched_create(trxhip_ctx *ctx, const trxhip_tx_sched_cfg *cfg, trxhip_tx_sched **out);
void trxhip_tx_sched_destroy(trxhip_tx_sched *s);
/* the transmit clock: the (FN, TN) of the next rendered slot; fn < 2715648.  Also drops render_frontend's remainder */
int  trxhip_tx_sched_set_clock(trxhip_tx_sched *s, uint32_t fn, int tn);
int  trxhip_tx_sched_clock(const trxhip_tx_sched *s, uint32_t *fn, int *tn);
int  trxhip_tx_sched_set_slot(trxhip_tx_sched *s, int chan, int tn, int comb);   /* SETSLOT: comb = TRXHIP_COMB_* / 1..13 */
int  trxhip_tx_sched_set_muted(trxhip_tx_sched *s, int chan, int muted);         /* RFMUTE */
/* h_dgram: one TRXD downlink datagram of len bytes (the layout of trxhip_modulate_trxd_batch()), copied at once.
 * *id = its submission id (0, 1, .. over the object's queued bursts) or -1 when refused or dropped */
int  trxhip_tx_sched_submit(trxhip_tx_sched *s, int chan, const uint8_t *h_dgram, size_t len, int64_t *id);
/* n_slots slots of every channel: channel c's stream at d_out_cf32 + 2*c*out_stride floats and / or d_out_s16 + 2*c*out_stride
 * int16, (int16_t)(int)(x * s16_scales[c]) (RadioInterface::pushBuffer's convert_float_short per channel).  out_stride >= the
 * samples of the render.  Plan-only objects take no outputs.  Asynchronous on `stream` */
int  trxhip_tx_sched_render(trxhip_tx_sched *s, size_t n_slots, float *d_out_cf32, size_t out_stride, int16_t *d_out_s16,
			    const float *s16_scales, void *stream);
/* The same through a transmit front end of chans == the scheduler's (RadioInterface::driveTransmitRadio: append, then
 * while (pushBuffer());): the rendered samples are appended to a remainder the object carries, every whole block_len block
 * goes through trxhip_tx_frontend_push(fe, ..., d_out_cf32, d_out_s16, s16_scale), the rest stays.  *n_blocks = blocks
 * written (out_cap: output samples the outputs hold, >= n_blocks * the front end's samples per block), *n_carried (may be
 * NULL) = samples carried per channel.  A plain render or set_clock drops the remainder. */
int  trxhip_tx_sched_render_frontend(trxhip_tx_sched *s, size_t n_slots, trxhip_tx_frontend *fe, float *d_out_cf32,
				     int16_t *d_out_s16, float s16_scale, size_t out_cap, size_t *n_blocks, size_t *n_carried,
				     void *stream);
int  trxhip_tx_sched_plan(const trxhip_tx_sched *s, int chan, trxhip_tx_plan *h_out, size_t n);   /* the last render's first n slots */
int  trxhip_tx_sched_counters(const trxhip_tx_sched *s, int chan, trxhip_tx_sched_ctrs *out);

/* ---- uplink burst scheduler: each channel's receive sample stream to TRXD uplink indications ----
 * The counterpart of the downlink scheduler, for batch callers ("radio samples in, datagrams out"): what lies between
 * trxhip_rx_frontend_pull() and the wire in the reference --
 *   RadioInterface::driveReceiveRadio()        radioInterface.cpp:240-294   (cut the stream into slots, keep the receive clock)
 *   Transceiver::pullRadioVector(), its head   Transceiver.cpp:665-815      (burstTime, OFF, mute, power, noise ring, counters)
 *   Transceiver::expectedCorrType()            Transceiver.cpp:513-601      (SETSLOT / HANDOVER state to the slot's CorrType)
 *   Transceiver::driveReceiveFIFO()            Transceiver.cpp:1187-1224    (one TRXD v0 / v1 datagram per indication)
 * trxhip_rx_sched_pull_frontend() joins the two: the radio's samples through the front end and the cutter in one call.
 * Slot cutter: at 4 SPS burstSize = 625; at 1 SPS -- the reference's default receive rate (DEFAULT_RX_SPS,
 * CommonLibs/trx_vty.h:29), an object from trxhip_rx_sched_create_sps() -- burstSize = 156 + (tN % 4 == 0), recomputed after
 * every incTN() (radioInterface.cpp:257-258, :283-288): slots of 157 / 156 / 156 / 156 samples from a TN that is a multiple of 4,
 * 625 samples to four slots.  A pull appends its n_samples per channel to a remainder the object carries on the device and cuts
 * slots `while (recvSz > burstSize)` -- strictly greater than the size of the slot that would be cut next, as in the reference,
 * so the remainder may hold exactly 625 samples (1 SPS: 156 in front of a slot of 156, 157 in front of one of 157).  All
 * channels advance together.  Each cut slot takes the receive clock's (FN, TN), then incTN().  There is no FIFO between the
 * cutter and the DSP, so the reference's "drop when 32 are queued" (radioInterface.cpp:277-280) has no counterpart.
 * At 1 SPS the slots inside a pull's chunk are read where they lie, like the 625-sample slots at 4 SPS, by an instance of the
 * 1-SPS burst kernel that knows where slot k starts and how long it is; a slot's record and soft row are bit for bit those of
 * trxhip_detect_demod_batch[_cf32](burst_len = 156 or 157, sps = 1) over that slot as a row.  energyDetect's window is 20 * sps
 * samples (Transceiver.cpp:725).  Not at 1 SPS: EDGE (cfg.egprs; the reference forces 4 SPS for it, osmo-trx.cpp:485-490).
 * Slot time and type: burstTime = time + ul_fn_offset (GSM::Time::operator+=(int): FN modulo 2715648, the offset may be
 * negative); type = expectedCorrType(burstTime, chan) over the combinations TRXHIP_COMB_*; mHandover[tn][ss] belongs to the
 * object, not to a channel; tsc = mTSC; max_toa = mMaxExpectedDelayAB for RACH / EXT_RACH, else mMaxExpectedDelayNB (:757-758;
 * 63 and 30 until set_max_toa).  Settings changed between pulls apply to the slots cut by later pulls.
 * Per slot, in pullRadioVector()'s order: OFF -- nothing (no datagram, no power, no noise update; the record carries fn, tn and
 * the OFF flag).  Muted channel -- an idle indication with rssi 0, noise ring untouched, no DSP: v1 sends an idle datagram with
 * rssi byte 0, v0 nothing.  Otherwise avg = sqrt(energy) (float, correctly rounded; one diversity path).  IDLE --
 * mNoises.insert(avg), mNoiseLev = mNoises.avg() (20 entries summed in float in index order, / 20.0f), an idle indication.
 * Any other type -- trxhip_detect_demod_batch[_cf32] with TRXHIP_FLAG_SLICE (and cfg.flags): rc <= 0 is an idle indication,
 * rc == -TRXHIP_SIGERR_CLIP counts in rx_clipping, any other negative rc in rx_no_burst_detected; rx_empty_burst stays 0.
 * cfg.flags & TRXHIP_FLAG_USE_VA: cfg->use_va ("viterbi-eq", Transceiver.cpp:760-787).  The stream handed to such an object is
 * what the radio read with readTimestamp -= 20 (rif_va_wrapper, osmo-trx.cpp:84-99) -- the early read is the caller's -- so
 * every slot begins 20 samples before the burst the detector expects.  OFF, mute and the noise ring are as above.  Power, rssi
 * and the ring's avg come from energyDetect over the slot as read; detection runs on shift_vec, the slot's samples 20 .. 604
 * with 40 zeros behind, and gives rc, toa, tsc and ci; rc <= 0 is the idle indication with the counters as above; otherwise the
 * soft row is vectorSlicer over scaleVector(burst, 1 / 16383) + demodAnyBurst_va() on the unshifted slot
 * (trxhip_demod_va_batch_cf32's bits: hard 0 / 1 for 148 bits, or for 88 on the access branch with 0.5 behind them).  Every slot
 * is read where it lies: one kernel writes the detector's rows and the slots' power, the detect entry point runs over those
 * rows, one kernel runs the Viterbi receiver over the slots in the stream (int16 streams are converted and scaled as they
 * are loaded; no complex64 copy is made).  The detector's rows are the object's: chans * max_slots * 625 samples of the pull's
 * format (2500 bytes a slot for int16, 5000 for complex64: 655 MB / 1.31 GB at one channel and 2^18 slots), allocated with
 * hipMalloc on the first such pull and again when a pull's format differs from the last one's (possible only with nothing
 * carried); TRXHIP_ENOMEM, state untouched, when that fails.  As the reference does (osmo-trx.cpp:492-496), create refuses the
 * flag with sps = 1 or egprs, and with TRXHIP_FLAG_EXACT_DEMOD (no filter demodulator runs); trxhip_rx_sched_pull_frontend()
 * takes a RESAMP front end and refuses a MULTI one.  A plan-only object accepts the flag and cuts and plans as without it.
 * Outputs of a pull that cuts n slots, device buffers indexed [chan * n + slot]:
 *   d_pkt, d_pkt_len : datagram rows of pkt_stride bytes and their lengths, exactly trxhip_pack_trxd_wire_batch()'s (one call
 *                      per channel with its version and rssi_offset over the slot's result record)
 *   d_ind            : trxhip_ul_ind records; rc, toa, ci, tsc, rssi, nbits as trxhip_burst_result has them (rssi in dBFS without
 *                      rssi_offset); noise_lev = mNoiseLev after this slot.  The reference's bi->noise,
 *                      20 log10(rxFullScale / mNoiseLev) + rssi_offset in double, is the caller's to take from noise_lev
 *   d_soft (or NULL) : sliced soft bits, 148 floats per slot, 444 with cfg.egprs.  The wire packer reads these rows, so the first
 *                      pull without d_soft allocates the object's own chans * max_slots rows (592 or 1776 bytes each: 155 MB at
 *                      one channel and 2^18 slots, 14.9 GB at the limits of the config) with hipMalloc, which may wait for the
 *                      device (TRXHIP_ENOMEM, state untouched, when it fails); a caller that always passes d_soft never pays it
 * Alignment: d_pkt, d_ind and d_soft 4 bytes, d_pkt_len 2.  Besides the rows every object holds 64 bytes per slot of
 * chans * max_slots for parameters, meta, result records and ring positions.
 * Waiting: trxhip_rx_sched_counters() and _noise_state() wait for the pulls issued so far; create waits for its own
 * initialisation; nothing else in the scheduler waits and nothing calls hipDeviceSynchronize (the detect entry point keeps its own rule, see trxhip_detect_demod_batch).
 * Issue every pull of one object on one stream; one object is not thread-safe.  TRXHIP_EIO from a pull: destroy the object.
 * ctx == NULL: a plan-only object (no device memory, inputs and outputs NULL): cutter, clock and trxhip_rx_sched_plan() as on
 * the GPU.  Every refused argument (config, chan, tn, ss, comb, version, sps other than 4 -- or 1 through
 * trxhip_rx_sched_create_sps() --, egprs with sps = 1, a pull before set_clock, more slots than
 * max_slots or out_slots, a missing or misaligned buffer, int16 and complex64 pulls mixed over a carried remainder -- by a
 * device object, and by a plan-only one of sps = 1, where the entry point called names the format --) is
 * TRXHIP_EINVAL and leaves the state untouched. */
#define TRXHIP_ULIND_OFF    1   /* type OFF: nothing is sent (pullRadioVector() returns -ENOENT) */
#define TRXHIP_ULIND_MUTED  2   /* the channel was muted */
#define TRXHIP_ULIND_IDLE   4   /* bi->idle */
typedef struct trxhip_ul_ind {
	uint32_t fn;             /* burstTime */
	uint8_t  tn;
	uint8_t  type;           /* enum trxhip_corr_type the slot was searched for */
	uint8_t  flags;          /* TRXHIP_ULIND_* */
	uint8_t  tsc;
	int32_t  rc;
	float    toa, ci, rssi;
	float    noise_lev;      /* mNoiseLev after this slot */
	uint16_t nbits;          /* 148, 444, or 0 */
	uint16_t reserved;
} trxhip_ul_ind;
typedef struct trxhip_rx_plan {
	uint32_t fn;             /* burstTime */
	uint8_t  tn;
	uint8_t  type;           /* expectedCorrType() */
	uint16_t max_toa;
} trxhip_rx_plan;
typedef struct trxhip_rx_sched_ctrs {
	uint64_t rx_empty_burst, rx_clipping, rx_no_burst_detected;
} trxhip_rx_sched_ctrs;
typedef struct trxhip_rx_sched_cfg {
	int32_t  chans;          /* logical channels, 1..8 */
	int32_t  sps;            /* 4; trxhip_rx_sched_create_sps() also takes 1 */
	int32_t  tsc;            /* mTSC, 0..7 */
	int32_t  ul_fn_offset;   /* cfg->ul_fn_offset, |offset| < 2715648 */
	int32_t  ext_rach;       /* cfg->ext_rach */
	int32_t  egprs;          /* cfg->egprs: soft rows of 444; 0 with sps = 1 */
	int32_t  flags;          /* 0, TRXHIP_FLAG_EXACT_DEMOD (sps = 1: accepted, the 1-SPS kernels are exact already) or
	                          * TRXHIP_FLAG_USE_VA (sps = 4, egprs = 0) */
	float    threshold;      /* TRXHIP_BURST_THRESH */
	float    full_scale;     /* rxFullScale */
	uint32_t reserved;
	uint64_t max_slots;      /* the largest pull, slots per channel, 1 .. 2^20 */
} trxhip_rx_sched_cfg;
typedef struct trxhip_rx_sched trxhip_rx_sched;
int  trxhip_rx_sched_create(trxhip_ctx *ctx, const trxhip_rx_sched_cfg *cfg, trxhip_rx_sched **out);   /* cfg->sps = 4 */
/* the same with cfg->sps = 1 or 4: at 4 it is trxhip_rx_sched_create(); at 1 the object cuts 157 / 156 / 156 / 156 slots, its
 * soft rows are 148 floats and cfg->egprs != 0 is TRXHIP_EINVAL.  Every other call takes either object */
int  trxhip_rx_sched_create_sps(trxhip_ctx *ctx, const trxhip_rx_sched_cfg *cfg, trxhip_rx_sched **out);
void trxhip_rx_sched_destroy(trxhip_rx_sched *s);
/* the receive clock: the (FN, TN) the next cut slot takes; fn < 2715648.  set_clock also drops the carried remainder */
int  trxhip_rx_sched_set_clock(trxhip_rx_sched *s, uint32_t fn, int tn);
int  trxhip_rx_sched_clock(const trxhip_rx_sched *s, uint32_t *fn, int *tn);
int  trxhip_rx_sched_set_slot(trxhip_rx_sched *s, int chan, int tn, int comb);       /* SETSLOT */
int  trxhip_rx_sched_set_handover(trxhip_rx_sched *s, int tn, int ss, int on);       /* HANDOVER / NOHANDOVER, ss 0..7 */
int  trxhip_rx_sched_set_muted(trxhip_rx_sched *s, int chan, int muted);             /* RFMUTE */
int  trxhip_rx_sched_set_trxd_version(trxhip_rx_sched *s, int chan, int version);    /* SETFORMAT: 0 or 1 */
int  trxhip_rx_sched_set_rssi_offset(trxhip_rx_sched *s, int chan, float rssi_offset_db);
int  trxhip_rx_sched_set_max_toa(trxhip_rx_sched *s, int max_toa_nb, int max_toa_ab);   /* SETMAXDLYNB / SETMAXDLY, 0..65535 */
/* slots the next pull of n_samples will cut (it depends only on the carried count and, at 1 SPS, on the clock's TN), or
 * TRXHIP_EINVAL */
int64_t trxhip_rx_sched_slots(const trxhip_rx_sched *s, size_t n_samples);
/* n_samples samples of every channel: channel c's chunk at d_in + 2*c*in_stride (int16 I, Q / floats; 4- / 8-byte aligned;
 * in_stride >= n_samples).  Slots that lie inside the chunk are read where they are.  out_slots: slots per channel the outputs
 * hold; *n_slots (may be NULL) = slots cut; *n_carried (may be NULL) = samples carried per channel.  Asynchronous on `stream` */
int  trxhip_rx_sched_pull_s16(trxhip_rx_sched *s, const int16_t *d_in, size_t in_stride, size_t n_samples, uint8_t *d_pkt,
			      int pkt_stride, uint16_t *d_pkt_len, trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots,
			      size_t *n_slots, size_t *n_carried, void *stream);
int  trxhip_rx_sched_pull_cf32(trxhip_rx_sched *s, const float *d_in, size_t in_stride, size_t n_samples, uint8_t *d_pkt,
			       int pkt_stride, uint16_t *d_pkt_len, trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots,
			       size_t *n_slots, size_t *n_carried, void *stream);
/* Through the receive front end -- RadioInterface::driveReceiveRadio() as one step, pullBuffer() and then the cutter: the
 * radio's int16 samples in, indications out.  fe: an object of trxhip_rx_frontend_create_chans() on the scheduler's context
 * whose trxhip_rx_frontend_rows() equals the scheduler's chans -- MULTI with 1..3 logical channels, or RESAMP with one; d_wide
 * and n_blocks as trxhip_rx_frontend_pull() takes them.  The scheduler's sps states the front end's output rate: 4, or 1 (a
 * RESAMP object at 1 SPS has block_len 384 at (65, 96): resamp_inchunk = inrate * 4 * sps, radioInterfaceResamp.cpp).
 * The effect on every output and on the carried state of both objects -- the front end's histories; the scheduler's remainder,
 * clock, noise rings, counters and last plan -- is that of
 *   trxhip_rx_frontend_pull(fe, d_wide, n_blocks, rows, stride, stream);
 *   trxhip_rx_sched_pull_cf32(s, rows, stride, trxhip_rx_frontend_out_samples(fe, n_blocks), ...the same outputs..., stream);
 * byte for byte, and the remainder is kept where pull_cf32 keeps it: the two forms may alternate on one object (an int16 pull
 * over the complex64 remainder, or this call over an int16 one, stays refused).  n_blocks == 0 cuts nothing and launches nothing.
 * d_work: caller-owned, 16-byte aligned, chans rows of work_stride complex64 samples, work_stride even and >=
 * TRXHIP_RX_SCHED_WORK_HEAD + out_samples; its content matters only during the call's work on `stream`.  The front end stores
 * channel l at d_work + 2*(l*work_stride + TRXHIP_RX_SCHED_WORK_HEAD), the carried remainder is put in front of it, and every
 * slot, the one that begins in the remainder too, is detected where it lies: no slot is assembled and no second detect launch
 * runs.  Refused with TRXHIP_EINVAL before anything is launched, both objects untouched: a NULL, plan-only or foreign-context
 * object, rows != chans, the four-row object of trxhip_rx_frontend_create(), d_wide NULL or misaligned, d_work NULL or
 * misaligned, work_stride odd or too small, a MULTI front end with a TRXHIP_FLAG_USE_VA scheduler (the reference refuses
 * use_va with multi-ARFCN), and whatever trxhip_rx_sched_pull_cf32() refuses.
 * trxhip_rx_sched_slots_frontend(): trxhip_rx_sched_slots(s, out_samples), or TRXHIP_EINVAL for a pair the pull refuses */
#define TRXHIP_RX_SCHED_WORK_HEAD 640   /* samples in front of the front end's output in a work row */
int64_t trxhip_rx_sched_slots_frontend(const trxhip_rx_sched *s, const trxhip_rx_frontend *fe, size_t n_blocks);
int  trxhip_rx_sched_pull_frontend(trxhip_rx_sched *s, trxhip_rx_frontend *fe, const int16_t *d_wide, size_t n_blocks,
				   float *d_work, size_t work_stride, uint8_t *d_pkt, int pkt_stride, uint16_t *d_pkt_len,
				   trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots, size_t *n_slots, size_t *n_carried,
				   void *stream);
int  trxhip_rx_sched_plan(const trxhip_rx_sched *s, int chan, trxhip_rx_plan *h_out, size_t n);   /* the last pull's first n slots */
int  trxhip_rx_sched_counters(trxhip_rx_sched *s, int chan, trxhip_rx_sched_ctrs *out);
/* the channel's noise ring as the reference holds it: ring[20], the insert position (0..20) and mNoiseLev */
int  trxhip_rx_sched_noise_state(trxhip_rx_sched *s, int chan, float *ring20, uint32_t *itr, float *lev);

/* ---- The MS-side downlink slot scheduler: the radio's sample stream in, burst indications out -----------------------------
 * What the reference does between the radio's receive buffers and upper_trx::pullRadioVector(): ms_trx::search_for_sch() /
 * handle_sch(true) (first acquisition), ms_trx::grab_bursts() / handle_sch_or_nb() (ms/ms_rx_lower.cpp:130-153, :157-205,
 * :310-422) and time_keeper (ms/ms.h:160-221), for one downlink stream at 4 samples per symbol.  The object carries the
 * partial slot between chunks, keeps the GSM clock with its sample timestamp, and moves the cut by what the SCH bursts
 * measure (temp_ts_corr_offset).  Per cut slot the kind, ACTIVE, the indication record and the 148 sbits are those of
 * trxhip_ms_rx_batch_*() on the same 625 samples with {fn, tn, tsc, ACTIVE = bit tn of active_tns}, byte for byte.
 *
 * acquire: handle_sch(true) on a buffer the caller has filled (the reference: 60000 samples; 532 .. TRXHIP_SCH_SYNC_MAX_LEN):
 *   trxhip_sch_sync_batch_*(TRXHIP_SCH_SYNC_ACQ) with scale 1 / rx_full_scale, WAITS for the 24-byte result, copies it to h_res
 *   (may be NULL) and returns 1 (burst found) or 0 (not found, state untouched).  On 1: the clock becomes (fn, 0) with ts 0
 *   (timekeeper.set(fn, 0), :91), mTSC = bsic & 7 (:90), first_sch_ts_start = first_ts + start - 16 - 1 (:198); the carried
 *   partial slot and any pending correction are dropped, and the next pull is grab_bursts()' first call.  The level gate and
 *   the gain steps around it (:333-347) stay with the caller (trxhip_ms_level_batch_i16() and trxhip_ms_agc_gate(), below).
 *   A plan-only object READS *h_res as the receiver's answer.
 * pull: one call of grab_bursts() with the chunk as `rcd` (n_samples samples from timestamp first_ts), literally:
 *   first call after an acquire (:362-383): next_burst_start = first_ts - first_sch_ts_start in int64; fullts, fracts by C's
 *     division; to_skip = 625 - fracts (a whole slot when fracts == 0); the clock fullts incTN() later, one more when fracts,
 *     one back (dec_by_one), and ts = first_ts - 625 + to_skip
 *   carried partial slot (:385-396): a chunk shorter than the missing part only extends it and cuts nothing (the correction
 *     stays pending); else the completed slot is cut first, with ts = first_ts - carried, and to_skip = the missing part
 *   correction (:399-406): to_skip -= pending; negative: to_skip = 0 and the pending value is kept whole; else pending = 0
 *   full = (n_samples - to_skip) / 625 slots at to_skip + i * 625, the rest is the new partial slot (:408-421)
 *   each cut slot FIRST does incTN(1) with ts = its first sample's timestamp (inc_and_update_safe) and THEN takes the clock --
 *     the clock an object reports is that of the last slot cut; the asserts of inc_and_update_safe (0.5 < diff / 625 < 1.5)
 *     count in clock_jumps
 *   with tracking on, every SCH slot with sch_rc == 1 && abs(start) > 1 adds -start to the pending correction (:199-203);
 *     several SCH slots of one pull add up, as in one reference buffer (an integer atomic: no ordering effect)
 *   d_ind[k], d_bits[k * 148] (d_bits may be NULL): slot k of the pull, k < *n_slots <= out_slots
 * Waits: a pull with tracking on that follows a pull which cut an SCH slot waits for that pull's correction (4 bytes, pinned,
 *   one event) before it plans; when the completed partial slot is itself an SCH slot, the pull demodulates that slot alone,
 *   waits for it, and plans the rest (the reference handles it before :399).  Nothing else waits, nothing calls
 *   hipDeviceSynchronize, and with tracking off no pull waits.  trxhip_ms_sched_state() waits for a correction in flight.
 * trxhip_ms_sched_slots(): slots the next pull of n_samples cuts -- exact when it is not the first pull after an acquire and
 *   tracking is off or no correction can be pending; else the upper bound (carried + n_samples) / 625 + 1.
 * Defined where the reference is not: where the literal arithmetic leaves the chunk (to_skip > n_samples; the reference calls
 *   read_n with a negative count) the pull is TRXHIP_EINVAL -- a longer chunk is accepted.  (Where such a pull, or one refused
 *   for out_slots, had to demodulate a straddling SCH slot first, d_ind[0] and the first row of d_bits may have been written;
 *   the object's state is untouched all the same.)
 * TRXHIP_EINVAL, state untouched: n_samples == 0, a pull before set_clock or a successful acquire, out_slots too small, a
 *   NULL or misaligned buffer (int16: 4 bytes, complex64: 8, d_ind: 4), int16 and complex64 pulls mixed over a carried partial
 *   slot, tsc > 7, fn >= 2715648, tn > 7, rx_full_scale not finite or not positive; a plan-only object takes no buffers.
 * ctx == NULL: a plan-only object -- cutter, clock, plan and state as on the GPU; the SCH results come from the queue of
 *   trxhip_ms_sched_feed_starts() (it replaces the queue; one entry per SCH slot cut with tracking on,
 *   TRXHIP_MS_SCHED_NO_SCH or an empty queue: not decoded; a refused pull consumes none).  Issue every call of one object on one stream; one object is not thread-safe. */
#define TRXHIP_MS_SCHED_NO_SCH INT32_MIN
typedef struct trxhip_ms_sched_cfg {
	float    rx_full_scale;  /* rxFullScale */
	uint8_t  tsc;            /* mTSC, 0..7 */
	uint8_t  active_tns;     /* bit tn: trxcon answers TRXCON_PHYIF_RTR_F_ACTIVE on that TN */
	uint8_t  tracking;       /* 0: SCH starts are reported but never move the cut */
	uint8_t  reserved;
} trxhip_ms_sched_cfg;
typedef struct trxhip_ms_plan {  /* 24 bytes */
	uint32_t fn;
	uint8_t  tn;
	uint8_t  kind;           /* TRXHIP_MS_KIND_* */
	uint8_t  flags;          /* TRXHIP_MS_SLOT_* */
	uint8_t  reserved;
	int64_t  ts;             /* timestamp of the slot's first sample */
	int32_t  src_off;        /* ts - first_ts: where the slot begins in the chunk (< 0: in the carried partial slot) */
	uint32_t reserved2;
} trxhip_ms_plan;
typedef struct trxhip_ms_sched_status {  /* 72 bytes */
	int64_t  to_skip;            /* applied by the last pull that reached the correction (:399-406) */
	int64_t  pending;            /* temp_ts_corr_offset */
	int64_t  first_sch_ts_start;
	uint32_t carried;            /* partial_rdofs */
	uint8_t  carried_cf32, first_call, tracking, tsc;
	uint8_t  active_tns, clock_set, reserved[6];
	uint64_t clock_jumps;        /* inc_and_update_safe()'s asserts that would have fired */
	uint64_t pulls, slots, sch_slots;
} trxhip_ms_sched_status;
typedef struct trxhip_ms_sched trxhip_ms_sched;
int  trxhip_ms_sched_create(trxhip_ctx *ctx, const trxhip_ms_sched_cfg *cfg, trxhip_ms_sched **out);
void trxhip_ms_sched_destroy(trxhip_ms_sched *s);
/* timekeeper.set(): the clock of the last slot cut and its timestamp; drops the carried partial slot and any pending
 * correction; the next pull is not a first call */
int  trxhip_ms_sched_set_clock(trxhip_ms_sched *s, uint32_t fn, int tn, int64_t ts);
int  trxhip_ms_sched_clock(const trxhip_ms_sched *s, uint32_t *fn, int *tn, int64_t *ts);
int  trxhip_ms_sched_set_tsc(trxhip_ms_sched *s, int tsc);
int  trxhip_ms_sched_set_active(trxhip_ms_sched *s, uint8_t tn_mask);
int  trxhip_ms_sched_set_tracking(trxhip_ms_sched *s, int on);
int  trxhip_ms_sched_feed_starts(trxhip_ms_sched *s, const int32_t *starts, size_t n);   /* plan-only objects */
int  trxhip_ms_sched_acquire_s16(trxhip_ms_sched *s, const int16_t *d_buf, size_t n_samples, int64_t first_ts,
				 trxhip_sch_sync_result *h_res, void *stream);
int  trxhip_ms_sched_acquire_cf32(trxhip_ms_sched *s, const float *d_buf, size_t n_samples, int64_t first_ts,
				  trxhip_sch_sync_result *h_res, void *stream);
int64_t trxhip_ms_sched_slots(const trxhip_ms_sched *s, size_t n_samples);
int  trxhip_ms_sched_pull_s16(trxhip_ms_sched *s, const int16_t *d_in, size_t n_samples, int64_t first_ts,
			      trxhip_ms_burst_ind *d_ind, int8_t *d_bits, size_t out_slots, size_t *n_slots, size_t *n_carried,
			      void *stream);
int  trxhip_ms_sched_pull_cf32(trxhip_ms_sched *s, const float *d_in, size_t n_samples, int64_t first_ts,
			       trxhip_ms_burst_ind *d_ind, int8_t *d_bits, size_t out_slots, size_t *n_slots, size_t *n_carried,
			       void *stream);
int  trxhip_ms_sched_plan(const trxhip_ms_sched *s, trxhip_ms_plan *h_out, size_t n);   /* the last pull's first n slots */
int  trxhip_ms_sched_state(trxhip_ms_sched *s, trxhip_ms_sched_status *out);

/* ---- A group of MS-side downlink streams: the pulls of all members cut and received as one step ---------------------------
 * n_members (1 .. TRXHIP_MS_GROUP_MAX_MEMBERS) streams, each what one trxhip_ms_sched is -- its own tsc, active_tns, tracking,
 * clock, carried partial slot, pending correction, counters and last plan --, behind one radio type: rx_full_scale belongs to
 * the group, and every cfgs[i].rx_full_scale must equal it.  Every call that names a member has the semantics of the
 * trxhip_ms_sched_* call of the same name on that member; a member index >= n_members is TRXHIP_EINVAL.
 * pull: h_chunks[m] = {d_in, n_samples, first_ts} is member m's chunk; n_samples == 0: the member has no chunk in this pull --
 *   nothing of it changes, h_n_slots[m] = 0, its last plan is kept.  The sample format is that of the call; the carried-format
 *   rule holds per member.  Member m's slot k goes to d_ind[m * out_stride + k] and d_bits[(m * out_stride + k) * 148] (d_bits
 *   may be NULL), k < h_n_slots[m] <= out_stride; nothing else of the outputs is written.  h_n_slots, h_n_carried (each may be
 *   NULL): n_members values.
 *   All or nothing: where any member's pull is one the single object refuses (above, per member, with out_stride as out_slots),
 *   the call returns that member's code, *bad_member (may be NULL; -1 otherwise) is the lowest such index, and no member's state
 *   moves (rows of straddling SCH slots may already have been written, as above).  What a refused pull may have done all the
 *   same, none of it visible in any member's state: waited for and folded the corrections in flight (wait (1) below; state()
 *   folds them too), waited for a pinned table area, and run the launch set of wait (2) -- its table copy, its join, a clear and
 *   a copy of all n_members correction words.  A pull in which no member has a chunk, or whose slots need more than 2^31 - 1
 *   wavefronts, is TRXHIP_EINVAL.
 *   Issued per pull, whatever n_members is: one copy of a table (64 bytes per member with slots, 64 per member with a join) from
 *   one of four pinned areas taken in turn, one join launch, one clear and one copy of the n_members correction words where a
 *   tracking member cuts an SCH slot, one receiver launch, one event record behind all of it.
 * Waits: (1) once for the group, for the corrections of an earlier pull, when a tracking member plans and any member's
 *   correction is in flight; (2) once for the group, where the straddling slot of one or more tracking members is an SCH slot:
 *   those slots are demodulated together in a launch set of their own (table, join, clear, receiver, copy, event) first.  A
 *   pinned table area is written again only behind the event of the launch set that read it, four launch sets earlier: a host
 *   that runs further ahead of the device than that waits there.  With tracking off everywhere a pull waits for nothing else.
 * acquire: one trxhip_sch_sync_batch_*(TRXHIP_SCH_SYNC_ACQ) over n buffers of buf_len samples, buf_stride samples apart (buffer i
 *   is members[i]'s, first_ts[i] its first sample's timestamp), one wait; h_res (may be NULL), h_found (may be NULL): n values.
 *   Per found member the assignments of trxhip_ms_sched_acquire_*; members not found are untouched.  Returns the number found.
 *   TRXHIP_EINVAL, nothing changed: a member listed twice, n == 0, a found record with fn outside the hyperframe.
 * ctx == NULL: a plan-only group -- no buffers, starts from per-member queues, acquire READS h_res[i]; out_stride == 0 leaves
 *   the counts unbounded, as the plan-only single object does, any other value bounds them as on the GPU.
 * Issue every call of one group on one stream; one group is not thread-safe. */
#define TRXHIP_MS_GROUP_MAX_MEMBERS 4096
typedef struct trxhip_ms_group_chunk {  /* 24 bytes */
	const void *d_in;        /* int16 I, Q pairs or complex64, as the call says; 4- / 8-byte aligned */
	size_t      n_samples;   /* 0: no chunk for this member */
	int64_t     first_ts;
} trxhip_ms_group_chunk;
typedef struct trxhip_ms_group trxhip_ms_group;
int  trxhip_ms_group_create(trxhip_ctx *ctx, float rx_full_scale, size_t n_members, const trxhip_ms_sched_cfg *cfgs,
			    trxhip_ms_group **out);
void trxhip_ms_group_destroy(trxhip_ms_group *g);
int  trxhip_ms_group_members(const trxhip_ms_group *g);
int  trxhip_ms_group_set_clock(trxhip_ms_group *g, uint32_t member, uint32_t fn, int tn, int64_t ts);
int  trxhip_ms_group_clock(const trxhip_ms_group *g, uint32_t member, uint32_t *fn, int *tn, int64_t *ts);
int  trxhip_ms_group_set_tsc(trxhip_ms_group *g, uint32_t member, int tsc);
int  trxhip_ms_group_set_active(trxhip_ms_group *g, uint32_t member, uint8_t tn_mask);
int  trxhip_ms_group_set_tracking(trxhip_ms_group *g, uint32_t member, int on);
int  trxhip_ms_group_feed_starts(trxhip_ms_group *g, uint32_t member, const int32_t *starts, size_t n);   /* plan-only groups */
int64_t trxhip_ms_group_slots(const trxhip_ms_group *g, uint32_t member, size_t n_samples);
int  trxhip_ms_group_plan(const trxhip_ms_group *g, uint32_t member, trxhip_ms_plan *h_out, size_t n);
int  trxhip_ms_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_sched_status *out);
int  trxhip_ms_group_acquire_s16(trxhip_ms_group *g, const uint32_t *members, size_t n, const int16_t *d_bufs, size_t buf_stride,
				 size_t buf_len, const int64_t *first_ts, trxhip_sch_sync_result *h_res, int *h_found, void *stream);
int  trxhip_ms_group_acquire_cf32(trxhip_ms_group *g, const uint32_t *members, size_t n, const float *d_bufs, size_t buf_stride,
				  size_t buf_len, const int64_t *first_ts, trxhip_sch_sync_result *h_res, int *h_found, void *stream);
int  trxhip_ms_group_pull_s16(trxhip_ms_group *g, const trxhip_ms_group_chunk *h_chunks, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
			      size_t out_stride, size_t *h_n_slots, size_t *h_n_carried, int *bad_member, void *stream);
int  trxhip_ms_group_pull_cf32(trxhip_ms_group *g, const trxhip_ms_group_chunk *h_chunks, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
			       size_t out_stride, size_t *h_n_slots, size_t *h_n_carried, int *bad_member, void *stream);

/* ---- MS-side receive gain control: slot levels and maybe_update_gain() on the device ----------------------------------------
 * What the reference does with do_auto_gain (ms/ms_upper.cpp:491): normed_abs_sum() (ms/ms.h:116-126) of every cut slot and
 * ms_trx::maybe_update_gain() on it (ms/ms_rx_lower.cpp:101-126, called at :149-150), and the level gate of search_for_sch()
 * (:333-347) in front of an acquire.  Bit for bit: there is no tolerance in any of it.
 * level: float sum = 0; for the 2 * len int16 values in order: sum += abs(value) (abs(-32768) is 32768); sum /= 2 * len -- the
 *   reference's sequential float sum.
 * maybe_update_gain(sum), per cut slot: runmean = gain_check ? (runmean * (gain_check + 2) - 1 + sum) / (gain_check + 2) : sum,
 *   every operation rounded to float; at gain_check == 159 the decision: gainoffset (a bool: the variable is `auto` from a
 *   comparison) = runmean < (rxFullScale / 2 ? 2 : 1); newgain = runmean < (rxFullScale * 2) / 3 ? rxgain + gainoffset : rxgain -
 *   gainoffset; applied when newgain != rxgain && newgain <= 60; then runmean = 0; gain_check = (gain_check + 1) % 160.
 * gate: search when level > rxFullScale / 8 (unsigned division) || rxgain >= 60, else raise the gain by 4.
 * rxFullScale is the object's rx_full_scale truncated to unsigned.  Defined where the reference is not: an SCH slot is measured
 *   on its own 625 samples (the reference sums a union that holds the 148 sch_bits and stale stack, ms/ms.h:128-144); an applied
 *   decision is the member's rx_gain at once (the reference hands setRxGain() to a worker thread).
 * trxhip_ms_level_batch_i16(): d_level[r] = the level of row r, row_len (1 .. TRXHIP_SCH_SYNC_MAX_LEN) int16 I, Q samples at
 *   d_in + 2 * r * row_stride; d_in 4-byte aligned, row_stride >= row_len in samples (rows are 4-byte aligned only).
 * trxhip_ms_agc_gate(): pure host; TRXHIP_MS_AGC_SEARCH (*new_gain = rx_gain) or TRXHIP_MS_AGC_RAISE (*new_gain = rx_gain + 4).
 * A scheduler member with gain control on (trxhip_ms_agc_sched_set / trxhip_ms_agc_group_set: {enable, rx_gain, d_level}; the
 *   calls of the single object are those of member 0 of a group of one): every int16 pull measures the slots it cuts, slot k
 *   of member m to d_level[m * out_stride + k] where d_level is given (float, 4-byte aligned; the single object: d_level[k],
 *   k < *n_slots; a group passes one array to all its members), and runs maybe_update_gain() over them in order.  The state is
 *   per member and lives on the device: gain_check, runmean, rx_gain, counters, the last TRXHIP_MS_AGC_RING decisions.
 *   set leaves gain_check, runmean, the counters and the ring as they are; set_clock and acquire do not touch any of it (the
 *   reference's gain_check and runmean are function statics).  Members are on or off independently; a member without a chunk,
 *   or one whose chunk only extends the partial slot, keeps its state.  A refused pull moves no AGC state.  A complex64 pull
 *   on a member with gain control on is TRXHIP_EINVAL, state untouched (the reference's radio buffers are int16).
 *   Issued per pull in which a member with gain control on cuts a slot, whatever n_members is: three launches (levels, the
 *   recurrence by pieces of a 160-slot window, the decisions) and one event record behind the pull's own; 64 bytes per such
 *   member ride in the pull's table; no wait, no further copy.  A pull whose level and piece results need more room than any
 *   before it allocates first.  With gain control off everywhere a pull issues what it issued before.
 *   _set, _set_gain and _state wait for the AGC launches in flight.  _state: ring[0 .. n_records) oldest first.
 *   Plan-only objects take the levels of the slots they cut from the queue of _feed_levels (it replaces the queue; a pull that
 *   cuts more slots than the queue holds is TRXHIP_EINVAL) and run the same recurrence on the host; they take no d_level. */
#define TRXHIP_MS_AGC_RING   8
#define TRXHIP_MS_AGC_RAISE  0
#define TRXHIP_MS_AGC_SEARCH 1
typedef struct trxhip_ms_agc_cfg {  /* 16 bytes */
	int32_t  enable;
	float    rx_gain;        /* rxgain, dB */
	float   *d_level;        /* device, may be NULL */
} trxhip_ms_agc_cfg;
typedef struct trxhip_ms_agc_record {  /* 32 bytes: one decision */
	uint64_t slot;           /* the slots measured before the one that closed the window */
	float    runmean, sum;   /* at the decision; sum: the closing slot's level */
	float    old_gain, new_gain;
	uint32_t applied;        /* newgain != rxgain && newgain <= 60: new_gain became rx_gain */
	uint32_t reserved;
} trxhip_ms_agc_record;
typedef struct trxhip_ms_agc_status {  /* 304 bytes */
	float    rx_gain, runmean;
	uint32_t gain_check;
	uint8_t  enable, reserved[3];
	uint64_t slots, decisions, applied;
	uint32_t n_records, reserved2;
	trxhip_ms_agc_record ring[TRXHIP_MS_AGC_RING];
} trxhip_ms_agc_status;
int  trxhip_ms_level_batch_i16(trxhip_ctx *ctx, const int16_t *d_in, size_t n_rows, size_t row_len, size_t row_stride, float *d_level,
			       void *stream);
int  trxhip_ms_agc_gate(float level, float rx_full_scale, float rx_gain, float *new_gain);
int  trxhip_ms_agc_sched_set(trxhip_ms_sched *s, const trxhip_ms_agc_cfg *cfg);
int  trxhip_ms_agc_sched_set_gain(trxhip_ms_sched *s, float rx_gain);
int  trxhip_ms_agc_sched_state(trxhip_ms_sched *s, trxhip_ms_agc_status *out);
int  trxhip_ms_agc_sched_feed_levels(trxhip_ms_sched *s, const float *levels, size_t n);   /* plan-only objects */
int  trxhip_ms_agc_group_set(trxhip_ms_group *g, uint32_t member, const trxhip_ms_agc_cfg *cfg);
int  trxhip_ms_agc_group_set_gain(trxhip_ms_group *g, uint32_t member, float rx_gain);
int  trxhip_ms_agc_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_agc_status *out);
int  trxhip_ms_agc_group_feed_levels(trxhip_ms_group *g, uint32_t member, const float *levels, size_t n);   /* plan-only groups */

/* ---- MS-side FCCH frequency-offset measurement (AFC) on the device -----------------------------------------------------------
 * The estimator the reference ships for the FCCH slot and never calls: gsm_fcch_offset() with ac_sum_with_lag() and pinv()
 * (ms/sch.c:255-314), restated literally on the slot's 625 samples after convert_and_scale by 1.f / rx_full_scale -- the float
 * samples ms_rx_kernel makes for a traffic slot; complex64 samples need no conversion and are multiplied by the same factor, as
 * trxhip_ms_rx_batch_cf32() does:
 *   start = 3 * 4 + 10 * 4 = 52, L1 = 3, L2 = 32, N1 = N2 = 92 (:206, :255-258, :292)
 *   v_L = sum over s < 92 of x[52 + L + s] * conj(x[52 + s]) (:273-279): samples 52 .. 175 are read and no others
 *   alpha_L = cargf(v_L); P = roundf((L1 * alpha_two - L2 * alpha_one) / (2 * M_PI)) (:293-297)
 *   (r, s): the first pair with P == 32 * i - 3 * j, i < 3, j < 32, or (0, 0) (:262-270, :299-300)
 *   omegal1 = (alpha_one + 2 * M_PI * r) / 3, omegal2 = (alpha_two + 2 * M_PI * s) / 32 (:302-303)
 *   reval = GSM_SYM_RATE / (2 * M_PI) * (expected_fcch_val - (omegal1 + omegal2) / 2); the result is -reval (:308, :313)
 * with the reference's types at every step: the float locals, the double M_PI sub-expressions, fs = 13. / 48. * 1e6 * 4 as a
 * float, expected_fcch_val = ((2 * M_PI) / fs) * 67700 (67700, not 67708.33: a tone exactly on the FCCH frequency reads
 * +8.33 Hz).  Only the order of the 92 additions differs (one wave per slot, a cross-lane reduction).  An all-zero slot has
 * atan2f(0, 0) = 0 for both angles and follows from that.  The range is about -85 .. +90 kHz; below it the estimate aliases.
 * Deliberately not reproduced: gsm_fcch_offset() also calls org_gsm_fcch_offset() (:305), whose value is discarded and which
 *   multiplies the caller's burst by a reference tone in place -- the input is never written here; the len > GSM_MAX_BURST_LEN
 *   clamp (:289-290) has no effect at 625.
 * mag_one, mag_two and energy are defined here, not by the reference, which has no validity test: mag_one / energy is near 1 on
 *   a tone and near 0 on noise, and is the caller's to threshold.
 * trxhip_ms_fcch_batch_*(): row r = the 625 samples at d_iq + r * slot_stride samples -> d_out[r].  The arguments are those of
 *   trxhip_ms_rx_batch_*(): slot_stride >= 625, n_slots 1 .. 2^31 - 1, rx_full_scale finite and positive; int16 rows are 4-byte
 *   aligned only (complex64: 8), d_out 4-byte aligned; else TRXHIP_EINVAL.  The int16 conversion happens in the load.
 * A scheduler member with AFC on (trxhip_ms_afc_sched_set / trxhip_ms_afc_group_set: {enable, d_fcch}; the single object's
 *   calls are those of member 0 of a group of one): every pull, int16 or complex64, measures the FCCH slots it cuts, ACTIVE or
 *   not (the policy the lower layer has for SCH slots), on exactly the 625 samples the receiver sees -- the slot assembled
 *   across two pulls and a slot that begins in the carried partial slot included -- and slot k of member m goes to
 *   d_fcch[m * out_stride + k] where d_fcch is given (4-byte aligned; the single object: d_fcch[k]); entries of other slots are
 *   not touched.  Per member on the device: the count of FCCH slots measured, the last record, and the last TRXHIP_MS_AFC_RING
 *   {fn, hz, mag_one, energy}.  _set leaves the state alone; set_clock and acquire do not touch it; a refused pull moves none
 *   of it.  The measurement feeds nothing back by itself: the caller reads it and sets the NCO below.  Issued per pull in which a member with AFC on cuts an FCCH slot: one launch (a wave per FCCH slot, found by
 *   arithmetic on the pull's clock) and one event record behind the pull's own; 64 bytes per such member ride in the pull's
 *   table; no wait, no copy.  With AFC off everywhere a pull issues what it issued before.  _set and _state wait for the AFC
 *   launches in flight.  _state: ring[0 .. n_records) oldest first.  Plan-only objects have no samples: _set is TRXHIP_EINVAL. */
#define TRXHIP_MS_AFC_RING 8
typedef struct {            /* 32 bytes */
	float hz;               /* -reval: the carrier offset in Hz, + = received tone above 67.7 kHz */
	float alpha_one, alpha_two;
	float mag_one, mag_two; /* |v_L1|, |v_L2| */
	float energy;           /* sum over s < 92 of |x[52 + s]|^2: mag_one / energy is the caller's tone test */
	int16_t p;              /* P */
	int8_t r, s;
	uint32_t reserved;      /* zero */
} trxhip_ms_fcch;
typedef struct trxhip_ms_afc_cfg {  /* 16 bytes */
	int32_t enable;
	int32_t reserved;
	trxhip_ms_fcch *d_fcch;  /* device, may be NULL */
} trxhip_ms_afc_cfg;
typedef struct trxhip_ms_afc_entry {  /* 16 bytes: one measured FCCH slot */
	uint32_t fn;
	float hz, mag_one, energy;
} trxhip_ms_afc_entry;
typedef struct trxhip_ms_afc_status {  /* 176 bytes */
	uint64_t count;          /* FCCH slots measured */
	uint32_t n_records;
	uint8_t  enable, reserved[3];
	trxhip_ms_fcch last;     /* zero while count == 0 */
	trxhip_ms_afc_entry ring[TRXHIP_MS_AFC_RING];
} trxhip_ms_afc_status;
int  trxhip_ms_fcch_batch_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t slot_stride, trxhip_ms_fcch *d_out, size_t n_slots,
			      float rx_full_scale, void *stream);
int  trxhip_ms_fcch_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, size_t slot_stride, trxhip_ms_fcch *d_out, size_t n_slots,
			       float rx_full_scale, void *stream);
int  trxhip_ms_afc_sched_set(trxhip_ms_sched *s, const trxhip_ms_afc_cfg *cfg);
int  trxhip_ms_afc_sched_state(trxhip_ms_sched *s, trxhip_ms_afc_status *out);
int  trxhip_ms_afc_group_set(trxhip_ms_group *g, uint32_t member, const trxhip_ms_afc_cfg *cfg);
int  trxhip_ms_afc_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_afc_status *out);

/* ---- MS-side frequency correction: a numerically controlled oscillator (NCO) per member in the receive path -------------------
 * The AFC above measures the carrier offset; this acts on it.  A group holds thousands of streams and no hardware can be trimmed
 * per member, so the oscillator is software: the receiver rotates every sample of a member's stream while it fills the slot's
 * window, in the same pass that converts and scales it.  The loop is feed-forward: the caller reads afc_state() and sets the NCO.
 * State per member: inc (int32, phase increment per sample), acc (uint32, the phase at ts_ref), ts_ref (int64), enable.
 *   phase      p(ts) = acc + (uint32_t)(ts - ts_ref) * (uint32_t)inc, all modulo 2^32; ts - ts_ref may be negative.  The phase of
 *              a sample depends on its absolute timestamp alone, so the result does not depend on how the stream is chunked.
 *   increment  inc = (int32_t)llrint(hz * (4294967296.0 / (13e6 / 12.0))) in double; |hz| <= 500000, else TRXHIP_EINVAL (NaN too).
 *              hz is the shift applied to the stream, + = the spectrum moves up: to cancel a measured offset pass
 *              -(fcch.hz - TRXHIP_MS_FCCH_BIAS_HZ) -- a tone on the FCCH frequency reads +25 / 3 Hz (see above).
 *   phasor     two float tables of 1024 (cos, sin) pairs: C[a] = (cos, sin)(2 pi a / 2^10), a = p >> 22, and
 *              F[b] = (cos, sin)(2 pi b / 2^20), b = (p >> 12) & 1023; the low 12 bits of p are dropped (a phase error below
 *              6e-6 rad, under float32 resolution of the products).  Entries are made in double and rounded to float; C is its
 *              first quadrant turned three times, so C[0] = (1, 0), C[256] = (0, 1), C[512] = (-1, 0), C[768] = (0, -1) exactly.
 *              r = (Cc Fc - Cs Fs, Cc Fs + Cs Fc), every product and sum rounded to float (no contraction).  16 KB on the
 *              device, made on the host at context creation and uploaded once.
 *   rotation   out = ((xr rc - xi rs) scale, (xr rs + xi rc) scale), x the float of the int16 sample or the complex64 sample:
 *              rotation first, convert_and_scale's factor second, each product and sum rounded to float.  The receiver with the
 *              NCO on therefore equals "rotate, then the complex64 receiver" bit for bit.  inc = 0 at phase 0 is the identity
 *              (r = (1, 0); a complex64 component of -0.0 may come out as +0.0).
 * Host-only, no GPU: trxhip_ms_nco_tables_host() (C then F, 4096 floats), trxhip_ms_nco_inc(), trxhip_ms_nco_phase().
 * trxhip_ms_nco_batch_*(): the rotation alone, no scale.  Row r = the row_len samples (1 .. 2^31 - 1) at d_in + r * row_stride
 *   samples, rotated by d_rec[r] = {phase0, inc} (sample i: phase0 + i * inc; a device array of 8-byte records, 4-byte aligned)
 *   into the complex64 row at d_out_cf32 + r * out_stride samples (8-byte aligned).  int16 rows are 4-byte aligned, complex64
 *   rows 8-byte; n_rows 1 .. 2^31 - 1; both strides >= row_len; else TRXHIP_EINVAL.  A wave per run of 64 samples.
 * A scheduler member (trxhip_ms_nco_sched_set / trxhip_ms_nco_group_set: {enable, hz}; the single object's calls are those of
 *   member 0 of a group of one).  _set acts at the member's clock ts_now, the ts trxhip_ms_sched_clock() reports (0 before a
 *   clock is set): acc <- p(ts_now), ts_ref <- ts_now, inc <- new, so the phase stays continuous across a change of frequency;
 *   switching on from off starts at acc = 0, and switching off leaves acc = 0.  A slot that straddles two pulls and is received
 *   after a _set is rotated whole with the new setting, extrapolated backwards.  _set and _state touch host state only and wait
 *   for nothing: a pull takes the member's setting by value.  set_clock, set_tsc, set_active, acquire and a refused pull leave the
 *   NCO alone.  Plan-only objects keep the same bookkeeping with no samples.
 *   Pulls (int16 and complex64, single and group): a pull in which any member with work has the NCO on runs the rotating
 *   instance of the receiver; members with it off ride with inc = 0 at phase 0.  Per receiver entry 16 bytes ride beside the
 *   table (the single object: a kernel argument): {phase of the first slot in the chunk, inc, phase of the slot assembled across
 *   two pulls, 0} -- the two phases are separate because a correction of the cut (temp_ts_corr_offset) can lie between those
 *   two slots.  They are computed on the host from the planner's timestamps after the waits the pull already has: no new launch,
 *   no new wait, no other copy.  With the NCO off everywhere a pull issues exactly what it issued before.  The join, the AGC
 *   levels and the FCCH measurement keep reading the stream as received: hz of the AFC stays the radio's offset, and d_fcch, the
 *   AFC ring and the AGC state are the same bytes with the NCO on or off.
 *   Acquire (trxhip_ms_sched_acquire_*, trxhip_ms_group_acquire_*): when a listed member has the NCO on, the buffers of the call
 *   go through trxhip_ms_nco_batch_*() (row i: phase p(first_ts[i]) of members[i], inc 0 at phase 0 for a member with it off)
 *   into an internal complex64 work buffer of n * buf_len * 8 bytes for the n buffers of that call, grown on demand and kept
 *   until the object is destroyed, and the search runs on that: the result is that of acquire_cf32 on the batch call's output. */
#define TRXHIP_MS_FCCH_BIAS_HZ (25.0 / 3.0)
typedef struct trxhip_ms_nco_row {  /* 8 bytes */
	uint32_t phase0;
	int32_t  inc;
} trxhip_ms_nco_row;
typedef struct trxhip_ms_nco_cfg {  /* 16 bytes */
	int32_t enable;
	int32_t reserved;
	double  hz;
} trxhip_ms_nco_cfg;
typedef struct trxhip_ms_nco_status {  /* 32 bytes */
	uint8_t  enable, reserved[3];
	int32_t  inc;
	uint32_t acc;
	uint32_t reserved2;
	int64_t  ts_ref;
	double   hz;
} trxhip_ms_nco_status;
int  trxhip_ms_nco_tables_host(float *out4096);
int  trxhip_ms_nco_inc(double hz, int32_t *inc);
uint32_t trxhip_ms_nco_phase(uint32_t acc, int64_t ts_ref, int32_t inc, int64_t ts);
int  trxhip_ms_nco_batch_i16(trxhip_ctx *ctx, const int16_t *d_in, size_t row_stride, const trxhip_ms_nco_row *d_rec, float *d_out_cf32,
			     size_t out_stride, size_t n_rows, size_t row_len, void *stream);
int  trxhip_ms_nco_batch_cf32(trxhip_ctx *ctx, const float *d_in_cf32, size_t row_stride, const trxhip_ms_nco_row *d_rec,
			      float *d_out_cf32, size_t out_stride, size_t n_rows, size_t row_len, void *stream);
int  trxhip_ms_nco_sched_set(trxhip_ms_sched *s, const trxhip_ms_nco_cfg *cfg);
int  trxhip_ms_nco_sched_state(trxhip_ms_sched *s, trxhip_ms_nco_status *out);
int  trxhip_ms_nco_group_set(trxhip_ms_group *g, uint32_t member, const trxhip_ms_nco_cfg *cfg);
int  trxhip_ms_nco_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_nco_status *out);

/* ---- MS-side FCCH search: cold-start frequency acquisition ---------------------------------------------------------------------
 * The AFC above measures FCCH slots that a clock points at, the clock comes from acquire, and acquire is the SCH receiver, which
 * decodes nothing from a carrier a few kHz off: an MS whose oscillator is that far off at power-up could never start the loop.
 * This finds the frequency-correction burst in a buffer with NO clock, at any carrier offset the estimator covers, measures it with
 * the estimator above and -- in the scheduler calls -- sets the NCO and runs the existing acquire through it.  The reference has no
 * such search (it trusts the radio's oscillator): the definition is this project's.
 * The search of one row of buf_len samples, x[n] = re + i im (int16 parts as integers, nothing is scaled: the score is a ratio):
 *   constants  HOP = 16, W = 576 (36 blocks of 16, two halves of 18), lag L = 8 samples (two symbols)
 *   per sample p[n] = x[n + L] conj(x[n]),  e[n] = |x[n]|^2            (int16: exact in int64)
 *   per block  block b = samples 16 b .. 16 b + 15: the sums of p and of e over them; nb = (buf_len - L) / 16 whole blocks, samples
 *              behind the last whole block are ignored
 *   per window window j, pos = 16 j, for every j with j + 36 <= nb:  Ra = sum of p over blocks j .. j + 17,  Rb = sum of p over blocks
 *              j + 18 .. j + 35,  E = sum of e over all 36 blocks     (int16: integers below 2^41, the same bits in any order)
 *   score      4 (Ra.re Rb.re + Ra.im Rb.im) / (E E) in IEEE double from the sums converted to double, in exactly that order of
 *              operations, no contraction; E == 0 gives 0, and so does a NaN (complex64 rows with non-finite samples).  On a clean
 *              tone it is |Ra + Rb|^2 / E^2 = 1, everywhere it is at most that; it does not depend on the carrier offset
 *   answer     the window with the largest score, the comparison strict >, so the lowest pos wins ties; found = score >= min_score
 *   complex64  the same definition; the products are unfused float operations, block and window sums in the order the kernel has
 *              (16-term block sums in float, everything above them in double), so these rows are specified to a bar -- each sum within
 *              2^-19 of the sum of |x[n + L]| |x[n]| (of |x[n]|^2 for E) over its terms --, not to the bit
 * The record (trxhip_ms_fcch_hit, 64 bytes): found, pos, score and the five sums as doubles (int16: exact integers).
 * The measurement: in the same call, with no host round trip, gsm_fcch_offset() as trxhip_ms_fcch_batch_*() computes it on the 625
 *   samples that begin at the row's pos -- it reads pos + 52 .. pos + 175 and nothing else, which lies inside the window -- into
 *   d_fcch[r] (may be NULL): the same bytes as trxhip_ms_fcch_batch_*() on that slot.  A row with found == 0 is measured too; its
 *   record is what the estimator says there.  rx_full_scale is used by the measurement only.
 * What the score cannot tell apart: a burst of all ones is the same tone, and an alternating bit pattern is a tone 135 kHz lower,
 *   where the estimator aliases.  The SCH decode that follows in the scheduler calls is the verification.
 * min_score: TRXHIP_MS_FSEARCH_MIN_SCORE lies midway between the two figures of tests/test_ms_fsearch_cpu.py, measured on the numpy
 *   model with the oracle's modulator: 0.08, the largest score more than 700 samples away from an FCCH burst (traffic on every
 *   slot, 10 and 25 dB), and 0.81, the smallest score of an FCCH burst at 10 dB.
 * trxhip_ms_fcch_search_*(): row r = the buf_len samples at d_iq + r * buf_stride samples.  Two launches (a workgroup per row and
 *   segment of 256 windows writes one candidate; a wave per row picks, writes the hit and measures), no atomics, no wait; the
 *   candidates live in a work array of the context (64 bytes per row and segment) that grows on demand and is kept -- calls on
 *   one stream follow each other without a wait, a call on another stream waits for the one before.  TRXHIP_EINVAL, nothing
 *   written: buf_len < 584 (W + L) or > 2^31 - 1, buf_stride < buf_len, n_bufs == 0 or > 2^31 - 1, min_score not in (0, 1] (NaN
 *   too), rx_full_scale not finite and positive, d_iq or d_hit NULL, d_iq not 4-byte (int16) / 8-byte (complex64) aligned, d_hit or
 *   d_fcch not 8-byte aligned.
 * The scheduler calls (trxhip_ms_afc_sched_acquire_*, trxhip_ms_afc_group_acquire_*; named like trxhip_ms_afc_*_set: the objects'
 *   own lists of entry points, trxhip_ms_sched_* and trxhip_ms_group_*, stay as they are) are the composition of public calls:
 *   1. trxhip_ms_fcch_search_*() over the buffers AS RECEIVED -- an NCO that is already on does not rotate them: AFC reads the
 *      stream as received -- with the object's rx_full_scale;
 *   2. one wait; hit and fcch of every buffer to the host (h_hit, h_fcch: n records each, either may be NULL);
 *   3. for every member with found: trxhip_ms_nco_*_set({1, -(fcch.hz - TRXHIP_MS_FCCH_BIAS_HZ)}) -- an absolute setting, not an
 *      increment on what the member had;
 *   4. trxhip_ms_group_acquire_*() for exactly those members, in the caller's order: one call per run of consecutive listed
 *      members with found (one call where every member is found; each call has its own wait).
 *   Members without found are not acquired and nothing of theirs is touched: h_found[i] = 0, h_res[i] is not written.  A member
 *   whose FCCH is found but whose SCH is not keeps its new NCO setting: the frequency is known, and the caller retries with the
 *   plain acquire on the next buffer.  Returns the number of members whose SCH was found; h_found[i] (may be NULL) says which.
 *   Refusals are those of acquire plus those of the search, all-or-nothing, decided before anything is set: TRXHIP_EINVAL with no
 *   member's state, NCO or output changed.  (A measured offset that trxhip_ms_nco_*_set refuses -- only non-finite complex64
 *   samples give one -- refuses the call in the same way, behind the search's wait.)  Plan-only objects have no samples:
 *   TRXHIP_EINVAL, as trxhip_ms_afc_*_set. */
#define TRXHIP_MS_FSEARCH_HOP 16
#define TRXHIP_MS_FSEARCH_W   576
#define TRXHIP_MS_FSEARCH_LAG 8
#define TRXHIP_MS_FSEARCH_MIN_SCORE 0.44
typedef struct trxhip_ms_fcch_hit {  /* 64 bytes */
	int32_t  found;          /* score >= min_score */
	uint32_t pos;            /* the best window's first sample in the row */
	double   score;
	double   ra_re, ra_im;   /* Ra, Rb and E of that window */
	double   rb_re, rb_im;
	double   energy;
	uint64_t reserved;       /* 0 */
} trxhip_ms_fcch_hit;
int  trxhip_ms_fcch_search_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t buf_stride, size_t buf_len, size_t n_bufs, double min_score,
			       float rx_full_scale, trxhip_ms_fcch_hit *d_hit, trxhip_ms_fcch *d_fcch, void *stream);
int  trxhip_ms_fcch_search_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, size_t buf_stride, size_t buf_len, size_t n_bufs,
				double min_score, float rx_full_scale, trxhip_ms_fcch_hit *d_hit, trxhip_ms_fcch *d_fcch, void *stream);
int  trxhip_ms_afc_sched_acquire_s16(trxhip_ms_sched *s, const int16_t *d_buf, size_t n_samples, int64_t first_ts, double min_score,
				     trxhip_ms_fcch_hit *h_hit, trxhip_ms_fcch *h_fcch, trxhip_sch_sync_result *h_res, void *stream);
int  trxhip_ms_afc_sched_acquire_cf32(trxhip_ms_sched *s, const float *d_buf, size_t n_samples, int64_t first_ts, double min_score,
				      trxhip_ms_fcch_hit *h_hit, trxhip_ms_fcch *h_fcch, trxhip_sch_sync_result *h_res, void *stream);
int  trxhip_ms_afc_group_acquire_s16(trxhip_ms_group *g, const uint32_t *members, size_t n, const int16_t *d_bufs, size_t buf_stride,
				     size_t buf_len, const int64_t *first_ts, double min_score, trxhip_ms_fcch_hit *h_hit,
				     trxhip_ms_fcch *h_fcch, trxhip_sch_sync_result *h_res, int *h_found, void *stream);
int  trxhip_ms_afc_group_acquire_cf32(trxhip_ms_group *g, const uint32_t *members, size_t n, const float *d_bufs, size_t buf_stride,
				      size_t buf_len, const int64_t *first_ts, double min_score, trxhip_ms_fcch_hit *h_hit,
				      trxhip_ms_fcch *h_fcch, trxhip_sch_sync_result *h_res, int *h_found, void *stream);

/* ---- The MS-side uplink burst scheduler: burst requests in, the radio's transmit sample stream out --------------------------
 * What the reference does between trxcon's burst request and the radio: upper_trx::driveTx() (ms/ms_upper.cpp:306-355),
 * ms_trx::submit_burst() (ms/ms.cpp:114-160), set_ta() (ms/ms.h:299-303) and submit_burst_ts() (ms/uhd_specific.h:260-269,
 * ms/bladerf_specific.h:461-478), for one MS at 4 samples per symbol, int16 out.
 * A request is what trxcon_phyif_handle_burst_req() queues (ms/ms_trxcon_if.cpp:36-46): {fn, tn, pwr, 148 bits}; a request
 * with burst_len == 0 never reaches the queue there, and is not submitted here.
 * submit, per request, with the timekeeper's pair (now_fn, now_tn, now_ts) the caller passes (trxhip_ms_sched_clock()):
 *   target = (fn, tn).incTN(3); diff_fn = FNDelta(target.fn, now_fn); diff_tn = (target.tn - (int)now_tn) % 8 (C remainder);
 *   tosend = Time(diff_fn, 0).incTN(diff_tn) when diff_tn > 0, else .decTN(-diff_tn) (FN borrow, below 0 to the hyperframe)
 *   "TX too late": diff_fn < 0 || (diff_fn == 0 && (target.tn - now.TN() < 3)) with TN() unsigned -> TRXHIP_MS_TX_LATE
 *   send_ts = now_ts + tosend.FN * 8 * 625 + tosend.TN * 625 - timing_advance: ONE_TS_BURST_LEN is an unsigned int (ms/ms.h:50),
 *     so the two products are formed modulo 2^32 before they widen to the int64 sum, and so they are here (they differ from
 *     the int64 products from tosend.FN = 858994 on, 66 minutes ahead); radio_ts = send_ts + rxtx_delay
 *   scale = (float)((double)tx_full_scale * pow(10, -RSSI / 10)), RSSI = (int)pwr, -RSSI / 10 an INTEGER division (:336):
 *     pwr 0..9 is full scale, 10..19 a tenth, ...
 *   The unsigned TN: with diff_fn == 0 and target.tn < now_tn the difference wraps, the burst is not "too late", and tosend is
 *     Time(0, 0).decTN(k) = (2715647, 8 - k).  The plan reports that literal send_ts with TRXHIP_MS_TX_WRAPPED and stages nothing.
 * The burst's int16 samples are row b of trxhip_modulate_batch({148, 8 + (tn % 4 == 0), 0, scale, 0}, sps 4, s16_scale 1):
 *   modulateBurst(bits, guard, 4), scaleVector(complex(scale)), static_cast<int16_t>(x * 1) (ms/ms.h:74-78).
 * Defined where the reference is not (its radio decides, or its behaviour is undefined):
 *   tx_full_scale > 21477 is refused: a Laurent modulator sample is at most 1.52568 (the largest per-phase sum of |taps|, c0 plus
 *     c1) and the largest scale is tx_full_scale, so above 21477 the product can reach 32768, where the reference's cast is
 *     undefined.  2047 (bladeRF) and 9830 = (unsigned)(32767 * 0.3) (UHD) pass.
 *   EXPIRED: radio_ts lies before the end of the last rendered window.  OVERLAP: the 625 samples intersect those of a queued
 *     burst; the later request loses.  FULL: max_pending bursts are queued.  Checked in this order, after LATE and WRAPPED.
 *   LATE requests report send_ts = radio_ts = 0 (the reference returns before it forms them).
 * Only QUEUED bursts are staged: bits and scale into a ring of max_pending rows on the device, one asynchronous copy per run of
 * consecutive ring rows (one per call while the free rows are not fragmented).
 * render: samples [first_ts, first_ts + n_samples) of the uplink stream as (I, Q) int16.  Queued bursts lie where their
 *   radio_ts puts them, clipped to the window; every other sample is 0; every sample is written exactly once.  A burst that
 *   ends inside the window is retired; one that crosses the window's end stays queued and the next render draws the rest from
 *   its bits (no sample state is carried: the modulator is deterministic).  Windows must not go backwards; a gap between
 *   windows is allowed.  A retired burst counts in `drawn` when at least one of its samples lay in a window, in `missed` when
 *   none did (it lay wholly in a gap); *n_drawn (may be NULL) = bursts this render retired as drawn.
 * Waits: submit waits for the copy issued 4 submit calls earlier, render for the render issued 4 render calls earlier (their
 *   pinned buffers are reused), and either may call hipHostMalloc / hipMalloc when a call is larger than any before.  Nothing
 *   calls hipDeviceSynchronize.  Issue every call of one object on one stream; one object is not thread-safe.  TRXHIP_EIO from
 *   submit or render (a failed copy or launch): destroy the object.
 * ctx == NULL: a plan-only object -- submit, plan, render's window and retire logic, counters as on the GPU; nothing is drawn
 *   and render takes d_out == NULL.
 * TRXHIP_EINVAL, state untouched: tx_full_scale > 21477, max_pending outside 1 .. 2^22, set_ta outside -126 .. 127, a request
 *   with tn > 7 or fn >= 2715648 (the whole call fails), now_fn >= 2715648, now_tn > 7, |now_ts| or |first_ts| > 2^62, h_reqs NULL
 *   with n > 0, first_ts before the end of the previous window, n_samples > 2^31, d_out NULL or not 4-byte aligned on a device
 *   object, d_out given to a plan-only one. */
#define TRXHIP_MS_TX_QUEUED  0
#define TRXHIP_MS_TX_LATE    1
#define TRXHIP_MS_TX_WRAPPED 2
#define TRXHIP_MS_TX_EXPIRED 3
#define TRXHIP_MS_TX_OVERLAP 4
#define TRXHIP_MS_TX_FULL    5
typedef struct trxhip_ms_tx_cfg {
	uint32_t tx_full_scale;  /* txFullScale: 2047 (bladeRF), 9830 (UHD); <= 21477 */
	int32_t  rxtx_delay;     /* rxtxdelay: -60 (bladeRF), -67 (UHD) */
	uint32_t max_pending;    /* queued bursts, 1 .. 2^22 */
	uint32_t reserved;
} trxhip_ms_tx_cfg;
typedef struct trxhip_ms_tx_req {  /* 156 bytes */
	uint32_t fn;
	uint8_t  tn;
	uint8_t  pwr;
	uint8_t  reserved[2];
	uint8_t  bits[148];      /* one bit per byte; bit 0 counts */
} trxhip_ms_tx_req;
typedef struct trxhip_ms_tx_plan {  /* 32 bytes */
	int64_t  send_ts;
	int64_t  radio_ts;       /* send_ts + rxtx_delay: the timestamp of the burst's first sample */
	int32_t  diff_fn, diff_tn;
	float    scale;
	int32_t  status;         /* TRXHIP_MS_TX_* */
} trxhip_ms_tx_plan;
typedef struct trxhip_ms_tx_status {  /* 96 bytes */
	uint64_t submitted, queued, late, wrapped, expired, overlap, full;   /* requests, by plan status */
	uint64_t drawn, missed;  /* retired bursts */
	uint64_t pending;        /* queued and not retired */
	int64_t  rendered_end;   /* the end of the last window; 0 before the first */
	int32_t  timing_advance; /* set_ta's val * 4 */
	uint8_t  window_set;     /* a window has been rendered */
	uint8_t  reserved[3];
} trxhip_ms_tx_status;
typedef struct trxhip_ms_tx trxhip_ms_tx;
int  trxhip_ms_tx_create(trxhip_ctx *ctx, const trxhip_ms_tx_cfg *cfg, trxhip_ms_tx **out);
void trxhip_ms_tx_destroy(trxhip_ms_tx *s);
/* set_ta(): timing_advance = val * 4, -126 <= val <= 127; applies to bursts submitted afterwards */
int  trxhip_ms_tx_set_ta(trxhip_ms_tx *s, int val);
/* n requests in host memory, in order; h_plan (may be NULL): one record per request */
int  trxhip_ms_tx_submit(trxhip_ms_tx *s, const trxhip_ms_tx_req *h_reqs, size_t n, uint32_t now_fn, int now_tn, int64_t now_ts,
			 trxhip_ms_tx_plan *h_plan, void *stream);
int  trxhip_ms_tx_render_s16(trxhip_ms_tx *s, int16_t *d_out, size_t n_samples, int64_t first_ts, size_t *n_drawn, void *stream);
int  trxhip_ms_tx_state(const trxhip_ms_tx *s, trxhip_ms_tx_status *out);

/* ---- The MS-side uplink scheduler group: N uplink streams, their submits and their renders each issued as one step ----------
 * N of the objects above behind one radio type: tx_full_scale, rxtx_delay and max_pending (per member) belong to the group, and
 * every member has its own timing advance, queue, window state and counters.  A member IS the single object -- the same code
 * plans its requests, places them in its queue, walks its windows and retires its bursts -- so per request the plan record and
 * the status rules (LATE, WRAPPED, EXPIRED, OVERLAP, FULL, QUEUED, in that order), and per member the 96-byte state record, are
 * the single object's, and so is every int16 of a member's window.
 * submit: h_member[i] names the member of request i; requests of one member keep their order, members do not interact.  h_now
 *   holds one clock per member (trxhip_ms_group_clock()) and is read only for the members that are named.  All or nothing: a
 *   member index out of range, tn > 7, fn >= 2715648 or a bad clock of a named member fails the whole call with every member
 *   untouched, *bad (may be NULL; (size_t)-1 otherwise) the first such request.  h_plan (may be NULL): one record per request.
 *   Issued per call, whatever N is: the QUEUED rows (160 bytes each), packed and followed by their ring destinations, go up in one
 *   copy from one of four pinned buffers taken in turn; one launch scatters them into the [N][max_pending] ring; one event.
 * render: member m's window [h_first_ts[m], h_first_ts[m] + h_n_samples[m]) is written at d_out + 2 * m * out_stride int16.
 *   h_n_samples[m] == 0: member m is not rendered and its state does not move.  Every member has its own window, as every MS has
 *   its own timebase.  Every sample of every rendered window is written exactly once, nothing outside a window is written.
 *   h_n_drawn (may be NULL): N values, per member the bursts this render retired as drawn.  All or nothing: a window that goes
 *   backwards, h_n_samples[m] > out_stride (or > 2^31), |h_first_ts[m]| > 2^62 fails the call with *bad_member (may be NULL; -1
 *   otherwise) the lowest such member, no member moved and no sample written; so does a d_out that is NULL or not 4-byte
 *   aligned, and a render of more than 2^31 - 1 tiles of 625 samples.
 *   Issued per call, whatever N is: one copy of a table from one of four pinned areas taken in turn -- 32 bytes per rendered
 *   member {out offset, n_samples, first_wave, first burst, n_bursts}, then 8 bytes {radio_ts - first_ts, ring row} per queued
 *   burst with samples in that member's window, no zero stretches -- one launch (one wave per tile of at most 625 samples) and
 *   one event.
 * Waits: a submit waits for the submit issued 4 submits earlier, a render for the render issued 4 renders earlier (a pinned area
 *   is written again only behind the event of the launch that read its copy), and either may allocate when a call is larger
 *   than any before.  Nothing else waits; nothing calls hipDeviceSynchronize.  Issue every call of one group on one stream; one
 *   group is not thread-safe.  TRXHIP_EIO from submit or render: destroy the group.
 * ctx == NULL: a plan-only group -- submit, plan, windows, counters; render takes d_out == NULL, and out_stride == 0 leaves the
 *   window lengths unbounded while any other value bounds them as on the GPU.
 * TRXHIP_EINVAL from create: n_members outside 1 .. 4096, what the single object refuses (tx_full_scale > 21477, max_pending
 *   outside 1 .. 2^22), n_members * max_pending > 2^32 - 1. */
#define TRXHIP_MS_TX_GROUP_MAX_MEMBERS 4096
typedef struct trxhip_ms_tx_group_cfg {
	uint32_t n_members;      /* 1 .. 4096 */
	uint32_t tx_full_scale;  /* as trxhip_ms_tx_cfg, for every member */
	int32_t  rxtx_delay;
	uint32_t max_pending;    /* queued bursts per member */
} trxhip_ms_tx_group_cfg;
typedef struct trxhip_ms_tx_clock {  /* 16 bytes: a member's timekeeper pair */
	uint32_t fn;
	int32_t  tn;
	int64_t  ts;
} trxhip_ms_tx_clock;
typedef struct trxhip_ms_tx_group trxhip_ms_tx_group;
int  trxhip_ms_tx_group_create(trxhip_ctx *ctx, const trxhip_ms_tx_group_cfg *cfg, trxhip_ms_tx_group **out);
void trxhip_ms_tx_group_destroy(trxhip_ms_tx_group *g);
int  trxhip_ms_tx_group_size(const trxhip_ms_tx_group *g);   /* n_members */
int  trxhip_ms_tx_group_set_ta(trxhip_ms_tx_group *g, uint32_t member, int val);
int  trxhip_ms_tx_group_submit(trxhip_ms_tx_group *g, const uint32_t *h_member, const trxhip_ms_tx_req *h_reqs, size_t n,
			       const trxhip_ms_tx_clock *h_now, trxhip_ms_tx_plan *h_plan, size_t *bad, void *stream);
int  trxhip_ms_tx_group_render_s16(trxhip_ms_tx_group *g, int16_t *d_out, size_t out_stride, const int64_t *h_first_ts,
				   const size_t *h_n_samples, size_t *h_n_drawn, int *bad_member, void *stream);
int  trxhip_ms_tx_group_state(const trxhip_ms_tx_group *g, uint32_t member, trxhip_ms_tx_status *out);

/* ---- MS-side uplink frequency correction: the NCO in the transmit render ------------------------------------------------------
 * The receive-side NCO above cancels the MS oscillator's error on the downlink; the same error leaves on the uplink.  One
 * oscillator per uplink member -- the single object, every member of a group -- applied inside the render between the modulator's
 * scaled sample and the int16 cast.  It is the oscillator defined above (phase, increment, phasor, rotation: the same tables, the
 * same expressions); nothing is defined again here.
 *   state      per member {enable, inc, acc, ts_ref, hz}, on the render's timeline: first_ts + i, the radio_ts of the plans.  The
 *              sample with timestamp ts has phase p(ts) = acc + (uint32_t)(ts - ts_ref) * (uint32_t)inc, a function of the absolute
 *              timestamp alone: windowing, tiling and a burst drawn across two renders cannot change a bit.
 *   sample     x = the modulator's sample after scaleVector's (scale, 0); r = the phasor of p(ts); y = (xr rc - xi rs, xr rs + xi rc);
 *              then the cast (int16_t)(int)(y * 1.0f).  Scale, rotate, cast; every product and sum rounded to float.  The int16
 *              are those of trxhip_modulate_batch (complex64, the plan's scale) -> trxhip_ms_nco_batch_cf32 with {p(radio_ts), inc}
 *              -> trxhip_convert_float_short(scale 1), placed at radio_ts - first_ts.
 *   direction  hz > 0 moves the spectrum up, as on the receive side.  An MS whose receive NCO is set to rx_hz (it cancels the
 *              offset seen on the downlink carrier) sets -rx_hz * (f_uplink / f_downlink) here.
 *   zeros      every sample outside a burst is written as 0 and reads no table.
 *   _set       {enable, hz} acts at ts_now = the member's rendered_end, or 0 before its first window: acc <- p(ts_now),
 *              ts_ref <- ts_now, inc <- new, so the phase stays continuous across a change of frequency; on from off starts at
 *              acc = 0, off leaves acc = 0.  It applies to samples rendered afterwards: a burst that crosses the end of a window
 *              and is finished by the next render after a _set is drawn partly with the old setting and partly with the new one,
 *              continuous at rendered_end.  _set and _state touch host state only and wait for nothing; a render takes the
 *              setting by value.  set_ta, submit and a refused render leave it alone.  Plan-only objects keep the same bookkeeping.
 *   render     a render in which a rendered member has the NCO on runs the rotating instance of its kernel; members with it off
 *              ride with inc = 0 at phase 0, the identity on the int16 (r = (1, 0) exactly).  The single object passes {p(first_ts),
 *              inc} and the context's 16 KB tables as two more kernel arguments; the group writes them into the 8 bytes of the
 *              member's table entry that were reserved.  No table grows; no copy, launch, event or wait is added.  With the NCO
 *              off everywhere a render issues exactly what it issued before.
 *   the cast   stays defined for every tx_full_scale that create accepts.  The component bound 1.52568 * scale rests on real taps
 *              against symbols of modulus 1, so the same triangle inequality bounds the MODULUS of x, and a component of x * r is
 *              at most |x||r|.  Roundings (u = 2^-24): the modulator's and the scale's, below 2^-20 relative on |x| (the allowance
 *              create already carries); table entries |C|, |F| <= 1 + u; the phasor's three per component, |r| < 1 + 6.3u; the
 *              rotation's three, 3u: together below 2^-20 again.  1.52568 * 21477 = 32767.03 leaves 2.96e-5 = 497u; the two
 *              allowances use 32u, so 21477 passes.  The check is made at create from the generated tables (with the largest
 *              modulus of the rotation table's entries as max|symbol|); should it ever fail, _set with enable != 0 returns
 *              TRXHIP_EINVAL on that object and create's own bound stays what it is.
 * TRXHIP_EINVAL, the member's NCO and every other state untouched: |hz| > 500000 or NaN (trxhip_ms_nco_inc()), cfg / out / object
 *   NULL, member >= n_members.  trxhip_ms_tx_status stays 96 bytes; the NCO has its own record, trxhip_ms_nco_status. */
int  trxhip_ms_nco_tx_set(trxhip_ms_tx *s, const trxhip_ms_nco_cfg *cfg);
int  trxhip_ms_nco_tx_state(const trxhip_ms_tx *s, trxhip_ms_nco_status *out);
int  trxhip_ms_nco_tx_group_set(trxhip_ms_tx_group *g, uint32_t member, const trxhip_ms_nco_cfg *cfg);
int  trxhip_ms_nco_tx_group_state(const trxhip_ms_tx_group *g, uint32_t member, trxhip_ms_nco_status *out);

/* ---- The air interface: an MS group and one BTS joined on the device ----------------------------------------------------------
 * One object between a group of N MSs and one BTS.  uplink: the N member rows trxhip_ms_tx_group_render_s16 wrote in, one summed
 * int16 stream out, what trxhip_rx_sched_pull_s16 takes.  downlink: one int16 stream in (trxhip_tx_sched_render's), N member rows out,
 * what trxhip_ms_group_chunk.d_in takes.  Every path -- one per member and direction -- has a gain, a delay in whole samples, a
 * carrier offset and the receiver's noise.  The reference has antennas here; this is the project's own definition.  Everything is
 * an integer behind one float stage, so the output is fixed to the bit whatever the grid, the split of the members or the chunking,
 * and a parallel sum needs no fixed order.
 *   ts, x      ts = the int64 timestamp of an output sample, d the path's delay, x the source's int16 sample at ts - d, or 0 where
 *              that lies in front of the direction's first sample or its last reset.
 *   rotation   the oscillator of "MS-side frequency correction" above as it is: p(ts) from the path's {acc, ts_ref, inc}, r the
 *              phasor of p, y = ((float)xr rc - (float)xi rs, (float)xr rs + (float)xi rc), every product and sum rounded to
 *              float.  The phase belongs to the output timestamp, not the source's.
 *   contribution  c = rint(y * g256) per component, round-half-even to a 32-bit integer, g256 = gain * 256.0f, 0 <= gain <= 16.
 *              |y| <= 46342, so |c| < 2^31.  A zero sample contributes exactly 0.
 *   noise      of receiver lane L = 2 rx + component at ts; rx = the member on the downlink, 4096 on the uplink.  fmix32 is
 *              murmur3's finaliser (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16), lo and hi the
 *              halves of (uint64_t)ts: key = fmix32(seed ^ fmix32(L)) + hi * 0x9e3779b9; w = fmix32(fmix32(lo) + key); s = the
 *              sum of w's four bytes minus 510 (an Irwin-Hall sum: symmetric, variance 21845, kurtosis 2.7);
 *              nq = (scale * s + 128) >> 8 with scale = llrint(rms * 65536 / 147.80054127099805), 0 <= rms <= 8192 in int16
 *              units, so the product fits 32 bits.  seed 2024, L 3, ts 0, 1, 2, 2^32, 2^63: s = 34, 185, -111, -16, 259.
 *   output     uplink: acc = the exact integer sum of c over all members + nq; downlink: acc = c + nq per member;
 *              out = clamp((acc + 128) >> 8, -32768, 32767), arithmetic shift, per component.
 *   windows    the windows of a direction are contiguous: first_ts must equal the direction's end_ts, except on the first call,
 *              which takes any first_ts.  _reset(dir, ts) forgets the source's past and sets end_ts = ts: the next window starts
 *              there.  The object carries the last max_delay samples of every source row (on the device for a device object), so
 *              chunking never changes a bit, also where n < d.
 *   _set_path  {gain, delay, hz} acts at end_ts (0 before the first window).  The oscillator changes as _set of the NCO does, on
 *              for hz != 0: the phase is continuous across a change of frequency, gain and delay jump.  hz = 0 rides as inc = 0
 *              at phase 0, the identity (r = (1, 0) exactly): gain 1, delay 0, hz 0, no noise and one member return the input
 *              bytes.  A new object has every path at {1, 0, 0} and no noise.
 *   _set_noise the rms of a receiver: the member's on the downlink, the BTS's on the uplink (member ignored).
 *   layout     uplink: member m's row at d_tx + 2 * m * tx_stride, n samples out at d_out.  downlink: n samples at d_in, member
 *              m's row at d_out + 2 * m * out_stride.  Source and output must not overlap.
 * Issued per call, whatever N is: one copy of a table (16 bytes per path, 16 more per downlink receiver) from one of four pinned
 *   areas taken in turn, at most three launches (the mix; the sum of its partials when the members are split across blocks; the
 *   save of the source's tail) and one event.  A call waits for the call of its direction issued 4 calls earlier, and may
 *   allocate when it is larger than any before; nothing else waits, nothing calls hipDeviceSynchronize.  Issue every call of one
 *   direction on one stream; one object is not thread-safe.  TRXHIP_EIO: destroy the object.
 * ctx == NULL: a host object.  The same calls on host pointers, the plain loop over the same inline functions, synchronous; the
 *   stream is ignored.  Its phasor tables are trxhip_ms_nco_tables_host's.
 * TRXHIP_EINVAL, nothing changed: n_members outside 1 .. 4096, max_delay > 65536, delay > max_delay, gain outside 0 .. 16 or NaN,
 *   rms outside 0 .. 8192 or NaN, |hz| > 500000 or NaN, dir not TRXHIP_AIR_UL / _DL, member >= n_members, a window that is not
 *   contiguous, a stride < n, pointers NULL or not 4-byte aligned, n == 0 or n > 2^31 - 1.
 * Memory: the two rings hold (n_members + 1) * max_delay samples of 4 bytes, allocated at create -- device memory for a device
 *   object, host memory (zero-filled) for a host object: 1 GiB at 4096 members and max_delay 65536, 1 MiB at 4096 and 64.  Ask for
 *   the largest delay the paths will use, not for the limit.  A device object also keeps 64 KB of pinned tables per direction
 *   and, once an uplink window has split its members, shares * n * 16 bytes of partials (about 2 MB at 4096 x 5000).
 * trxhip_air_noise_host: nq of (seed, lane, ts) for a scale in 0 .. 3632402; scale = 256 returns s; a scale outside that range
 *   returns 0.  Host only. */
#define TRXHIP_AIR_UL 0
#define TRXHIP_AIR_DL 1
#define TRXHIP_AIR_MAX_MEMBERS 4096
#define TRXHIP_AIR_MAX_DELAY   65536
#define TRXHIP_AIR_UL_RX       4096
typedef struct trxhip_air_cfg {  /* 16 bytes */
	uint32_t n_members;      /* 1 .. 4096 */
	uint32_t max_delay;      /* samples of every source row the object carries: 0 .. 65536 */
	uint32_t seed;           /* of the noise */
	uint32_t reserved;
} trxhip_air_cfg;
typedef struct trxhip_air_path {  /* 16 bytes */
	float    gain;           /* 0 .. 16 */
	uint32_t delay;          /* 0 .. max_delay */
	double   hz;             /* |hz| <= 500000, + = up */
} trxhip_air_path;
typedef struct trxhip_air_path_status {  /* 48 bytes */
	float    gain;
	uint32_t delay;
	double   hz;
	int32_t  inc;
	uint32_t acc;
	int64_t  ts_ref;
	int32_t  noise_scale;    /* of the path's receiver */
	uint32_t started;        /* the direction has had a window or a reset */
	int64_t  end_ts;         /* of the direction */
} trxhip_air_path_status;
typedef struct trxhip_air trxhip_air;
int  trxhip_air_create(trxhip_ctx *ctx, const trxhip_air_cfg *cfg, trxhip_air **out);
void trxhip_air_destroy(trxhip_air *a);
int  trxhip_air_set_path(trxhip_air *a, int dir, uint32_t member, const trxhip_air_path *p);
int  trxhip_air_set_noise(trxhip_air *a, int dir, uint32_t member, double rms);
int  trxhip_air_path_state(const trxhip_air *a, int dir, uint32_t member, trxhip_air_path_status *out);
int  trxhip_air_reset(trxhip_air *a, int dir, int64_t ts);
int  trxhip_air_uplink_s16(trxhip_air *a, const int16_t *d_tx, size_t tx_stride, int64_t first_ts, size_t n, int16_t *d_out, void *stream);
int  trxhip_air_downlink_s16(trxhip_air *a, const int16_t *d_in, int64_t first_ts, size_t n, int16_t *d_out, size_t out_stride,
			     void *stream);
int32_t trxhip_air_noise_host(uint32_t seed, uint32_t lane, int64_t ts, int32_t scale);

/* ---- The air interface: multipath rays per path (echoes, Doppler, fading) ------------------------------------------------------
 * A path (member, direction) of a trxhip_air has either the plain state _set_path sets, or a list of 1 .. 64 rays; a ray is what
 * a path is, {gain 0 .. 16, delay 0 .. max_delay in whole samples, hz with |hz| <= 500000, phase (uint32, 2^32 = one turn)}.
 *   ray phase  p_r(ts) = phase + (uint32_t)(ts - ts_set) * (uint32_t)inc, inc = trxhip_ms_nco_inc(hz), ts_set the direction's
 *              end_ts at the set call (0 before the first window).  Modulo 2^32 that is phase_at_0 + (uint32_t)ts * inc with
 *              phase_at_0 = phase - (uint32_t)ts_set * inc: a function of the absolute timestamp, untouched by windows and resets.
 *   ray        x = the source sample at ts - delay, or 0 in front of the direction's first sample or reset; c_r = the contribution
 *              of x through {p_r(ts), gain * 256.0f} exactly as a path's above (phasor, rotation, rint).  A zero sample gives 0.
 *   path       the exact integer sum of c_r over its rays.  |c_r| < 2^28, so 64 rays x 4096 members stay far inside int64; the
 *              downlink too carries its per-member sum in 64 bits.  Noise, output, windows, rings and reset are as above.
 *   side by side  while a path has rays its output is theirs.  _set_path still updates the plain state and _path_state reports
 *              it, as without rays; setting zero rays returns the path to its plain state, whose oscillator has kept running (it
 *              is a function of the absolute timestamp).  One ray {g, d, 0 Hz, phase 0} gives the bytes of the plain path {g, d, 0}.
 * trxhip_multipath_set acts at the direction's end_ts and is all-or-nothing.  TRXHIP_EINVAL, nothing changed: n_rays > 64, rays
 *   NULL with n_rays > 0, a gain outside 0 .. 16 or NaN, delay > max_delay, |hz| > 500000 or NaN, reserved != 0, a bad dir or
 *   member, object NULL.
 * trxhip_multipath_state writes min(cap, *n_rays) rays with phase advanced to the current end_ts, the number the path has to
 *   *n_rays and the end_ts of the last _set (0 when there was none) to *ts_set; n_rays and ts_set may be NULL, out too when cap
 *   is 0.  Feeding its output back to _set changes no later byte: that is how a caller changes a profile with continuous phases.
 * Both work on host objects (the plain loop over the same inline functions) and on device objects.  On the device a direction in
 *   which some path has rays keeps one flat list of ray entries (32 bytes each; a plain member of it is one entry; the downlink
 *   adds 24 bytes per member) resident: the first window after a _set_path, trxhip_multipath_set or (downlink) _set_noise copies
 *   it from the window's pinned area, a window with nothing changed copies nothing, whatever N and the number of rays.  Per
 *   window: at most that one copy, three launches, one event, and the waits stated above.  A direction without rays issues what
 *   it issued before. */
#define TRXHIP_MULTIPATH_MAX_RAYS 64
typedef struct trxhip_multipath_ray {  /* 24 bytes */
	float    gain;           /* 0 .. 16 */
	uint32_t delay;          /* 0 .. max_delay */
	double   hz;             /* |hz| <= 500000, + = up */
	uint32_t phase;          /* at the direction's end_ts; 2^32 = one turn */
	uint32_t reserved;       /* 0 */
} trxhip_multipath_ray;
int  trxhip_multipath_set(trxhip_air *a, int dir, uint32_t member, const trxhip_multipath_ray *rays, uint32_t n_rays);
int  trxhip_multipath_state(const trxhip_air *a, int dir, uint32_t member, trxhip_multipath_ray *out, uint32_t cap, uint32_t *n_rays,
			    int64_t *ts_set);

#ifdef __cplusplus
}
#endif
#endif /* TRXHIP_H */
