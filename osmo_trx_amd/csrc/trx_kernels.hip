// trx_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for osmo-trx's receive-side burst DSP.
//
// Hot kernel: burst_pull_kernel = the DSP core of Transceiver::pullRadioVector()
// (Transceiver52M/Transceiver.cpp:724-803): convert_short_float -> energyDetect -> clip check ->
// detectAnyBurst -> demodAnyBurst -> vectorSlicer, for a batch of independent bursts.
//
// Mapping (MI355X-first, not a translation of the SSE code):
//   * ONE WAVEFRONT (64 lanes) PER BURST, persistent waves grid-striding over the batch, 12 waves per
//     workgroup = one workgroup per CU.  A burst (625 x int16 IQ = 2500 B) is read from HBM exactly once
//     with coalesced dword loads that are software-prefetched one burst ahead, converted to fp32 in
//     flight and kept in that wave's private LDS slice (~8 KB) until its soft bits and 32-byte result
//     record are written: zero intermediate HBM traffic (measured: 1.02 x algorithmic bytes).
//   * every table the path touches (sinc LUT, 64 fractional-delay filters, decimator taps, training
//     sequences, reverse rotation) is staged ONCE per workgroup into LDS (26 KB); wave-uniform taps are
//     LDS broadcast reads, per-lane gathers (sinc LUT) use a bank-swizzled layout.
//   * waves never synchronise with each other after that staging; intra-wave ordering relies on
//     wave-lockstep LDS execution (wave_sync()).
//   * the kernel is VALU-issue bound (not HBM bound: ~26 FLOP/B), so the code is organised to spend
//     vector instructions on the FIR arithmetic only: reductions are DPP (v_max/v_add with row/bcast
//     controls), arg-max and the TOA bisection walk are v_cmp ballots consumed by the scalar unit,
//     range checks are replaced by zero-padded LDS buffers.
//   * peak/TOA: the reference's 9-step early/late bisection (19 data-dependent sinc interpolations) is
//     evaluated SPECULATIVELY: the binary decision tree is expanded across lanes (2 rounds: levels 0-4,
//     then 5-8 + the 16 possible final positions), each lane doing one sequential 16-tap interpolation.
//   * no MFMA: these are short 1-D real/complex convolutions (<= 40 taps).
//
// Numerics: every sum that feeds a DECISION (correlation, peak ratio, bisection compares, filter
// choice) is accumulated in the reference's generic-C order (arch/common/convolve_base.c:28-54) and
// the file is compiled with -ffp-contract=off, so rc / TOA / amp / soft bits are bit-identical to the
// generic-C reference.  Only energyDetect (tree-summed), log2f (C/I) and log10f (RSSI) differ at the
// 1e-6 level.
#include "trx_device.h"
#include "trx_launch.h"

// ------------------------------------------------------------------------------------------------
// the hot kernel
// ------------------------------------------------------------------------------------------------
// (1 SPS: a burst's LDS slice is 4.4 KB and the kernel fits 128 registers, so 16 waves share a CU as in the 4-SPS kernel;
//  the generic 4-SPS instantiations keep 12 waves and their 147-168 registers)
#define TRX_WPB_OF(SPS_) ((SPS_) == 1 ? 16 : TRX_WPB)
template <int SPS, bool CF32, int NLD>
__global__ void __launch_bounds__(TRX_WPB_OF(SPS) * WAVE, (SPS == 1 ? 4 : 3))
burst_pull_kernel(const void *__restrict__ iq_, const trxhip_burst_params *__restrict__ params,
		  trxhip_burst_result *__restrict__ results, float *__restrict__ soft,
		  const trx_tables *__restrict__ tab, const float4 *__restrict__ ebp_in,
		  unsigned n_bursts, int Lmax, float thresh, float full_scale, int soft_stride, int slice)
{
	constexpr bool STREAM = false;
	constexpr unsigned ph = 0u;
#include "trx_pull_body.inc"
}

// the stream form of burst_pull_kernel<1, CF32, 3>, for the uplink scheduler (trx_rx_sched.hip): the slots of a 1-SPS receive
// stream read in place.  Same work distribution, prefetch and per-burst arithmetic
template <bool CF32>
__global__ void __launch_bounds__(TRX_WPB_OF(1) * WAVE, 4)
burst_pull_stream_kernel(const void *__restrict__ iq_, const trxhip_burst_params *__restrict__ params,
			 trxhip_burst_result *__restrict__ results, float *__restrict__ soft,
			 const trx_tables *__restrict__ tab, unsigned n_bursts, unsigned ph, float thresh, float full_scale,
			 int soft_stride, int slice)
{
	constexpr int SPS = 1, NLD = 3, Lmax = 157;
	constexpr bool STREAM = true;
	const float4 *const ebp_in = nullptr;
#include "trx_pull_body.inc"
}

// ------------------------------------------------------------------------------------------------
// launch wrappers (called from trx_capi.cpp)
// ------------------------------------------------------------------------------------------------
extern "C" size_t trx_pull_lds_bytes(int L, int waves_per_block)
{
	const int xs_len = TRX_PAD + L + TRX_PAD;
	const size_t slice_c32 = ((xs_len + 1) & ~1) + TRX_DEC_LEN + TRX_CZ_LEN;
	return TRX_TABLES_LDS_BYTES + (size_t)waves_per_block * slice_c32 * sizeof(c32) + 16;   // + the workgroup's work counter
}

// burst_pull_kernel<sps, cf32, nld>
extern "C" int trx_launch_pull(const void *d_iq, int cf32, int nld, const trxhip_burst_params *d_params, trxhip_burst_result *d_results,
			       float *d_soft, const trx_tables *d_tab, const float *d_ebp_in, size_t n_bursts, int L, int sps, float thresh,
			       float full_scale, int soft_stride, int flags, int n_cu, hipStream_t stream)
{
	if (n_bursts == 0)
		return 0;
	// as many waves per workgroup as the 160 KB of LDS admit (12 at L = 625), one workgroup per CU
	int wpb = TRX_WPB_OF(sps);
	while (wpb > 1 && trx_pull_lds_bytes(L, wpb) > 160 * 1024)
		wpb--;
	const size_t lds = trx_pull_lds_bytes(L, wpb);
	if (lds > 160 * 1024)
		return TRXHIP_EINVAL;
	const size_t grid = trx_burst_grid(n_bursts, (size_t)n_cu * (size_t)((160 * 1024) / lds));

#define LAUNCH(SPS_, CF_, NLD_)                                                                                 \
	do {                                                                                                    \
		constexpr auto k = burst_pull_kernel<SPS_, CF_, NLD_>;                                          \
		if (trx_arm_dynamic_lds<k>())                                                                   \
			return TRXHIP_EIO;                                                                      \
		hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(wpb * WAVE), lds, stream, d_iq, d_params, d_results, \
				   d_soft, d_tab, reinterpret_cast<const float4 *>(d_ebp_in), (unsigned)n_bursts, L, thresh,     \
				   full_scale, soft_stride, flags);                                             \
	} while (0)

	if (sps == 4) {
		if (nld == 10) { if (cf32) LAUNCH(4, true, 10); else LAUNCH(4, false, 10); }
		else           { if (cf32) LAUNCH(4, true, 0);  else LAUNCH(4, false, 0); }
	} else {
		if (cf32) LAUNCH(1, true, 3); else LAUNCH(1, false, 3);
	}
#undef LAUNCH
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// burst_pull_stream_kernel<cf32>: geometry of trx_launch_pull() at sps = 1, L = 157
extern "C" int trx_launch_pull_stream(const void *d_iq, int cf32, unsigned tn_phase, const trxhip_burst_params *d_params,
				      trxhip_burst_result *d_results, float *d_soft, const trx_tables *d_tab, size_t n_slots, float thresh,
				      float full_scale, int soft_stride, int flags, int n_cu, hipStream_t stream)
{
	if (n_slots == 0)
		return 0;
	if (!d_iq || !d_params || !d_results || n_slots > 0x7fffffffull || tn_phase > 3u)
		return TRXHIP_EINVAL;
	const int wpb = TRX_WPB_OF(1);
	const size_t lds = trx_pull_lds_bytes(157, wpb);
	const size_t grid = trx_burst_grid(n_slots, (size_t)n_cu * (size_t)((160 * 1024) / lds));
	if (cf32) {
		constexpr auto k = burst_pull_stream_kernel<true>;
		if (trx_arm_dynamic_lds<k>())
			return TRXHIP_EIO;
		hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(wpb * WAVE), lds, stream, d_iq, d_params, d_results, d_soft, d_tab,
				   (unsigned)n_slots, tn_phase, thresh, full_scale, soft_stride, flags);
	} else {
		constexpr auto k = burst_pull_stream_kernel<false>;
		if (trx_arm_dynamic_lds<k>())
			return TRXHIP_EIO;
		hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(wpb * WAVE), lds, stream, d_iq, d_params, d_results, d_soft, d_tab,
				   (unsigned)n_slots, tn_phase, thresh, full_scale, soft_stride, flags);
	}
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
