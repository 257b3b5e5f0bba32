// trx_ms_afc.hip -- the MS-side FCCH frequency-offset measurement for gfx950: gsm_fcch_offset() with its helpers ac_sum_with_lag()
// and pinv() (Transceiver52M/ms/sch.c:255-314), the estimator the reference ships for the slot kind that pullRadioVector() returns
// as trash (ms/ms_upper.cpp:189-192).  include/trxhip.h states the arithmetic; here it is line by line.
//
// ONE WAVE PER SLOT.  The two autocorrelations v_L = sum_{s < 92} x[52 + L + s] * conj(x[52 + s]), L = 3 and 32 (:273-279, :293-294),
// and our own energy sum share the 92 samples x[52 + s]: lane l takes the products s = l and, below lane 28, s = l + 64, reads its
// at most six samples where they lie (the int16 conversion and the scale happen in the load; nothing outside samples 52 .. 175 is
// touched), and a butterfly over the lanes adds the partial sums.  Additions commute, so every lane ends with the same five
// floats; the order of the 92 additions is the only thing that differs from the reference's loop.  Everything behind the sums --
// cargf, P, pinv, the two omegas, reval -- runs in every lane on those wave-uniform values with the reference's types: float
// locals, and double wherever M_PI (a double) enters an expression.  Lane 0 stores.
//
// NOT REPRODUCED, on purpose: gsm_fcch_offset() also calls org_gsm_fcch_offset() (:305), discards its value, and thereby multiplies
// the caller's burst by a reference tone in place -- the input is never written here; the len > GSM_MAX_BURST_LEN clamp (:289-290)
// has no effect at 625.  mag_one, mag_two and energy are this project's: the reference has no validity test.
//
// The body itself, afc_measure(), lives in trx_ms_afc_dev.h: the FCCH search (trx_ms_fsearch.hip) measures with it too.
// Three forms of one body: rows (trxhip_ms_fcch_batch_*), and the scheduler's stream and group forms, in which a wave finds its
// FCCH slot among the slots of a member's pull by arithmetic on the pull's clock (trx_ms_afc.h) and also moves the member's state.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_afc.h"
#include "trx_ms_afc_dev.h"
#include "trx_ms_sched.h"

namespace {

constexpr int WAVE = 64;
constexpr int WPB = 4;                         /* waves per block */
constexpr int kThreads = WPB * WAVE;

static_assert(sizeof(trxhip_ms_fcch) == 32 && sizeof(trxhip_ms_afc_entry) == 16 && sizeof(trxhip_ms_afc_status) == 176 &&
	      sizeof(trxhip_ms_afc_cfg) == 16, "public AFC structs");
static_assert(sizeof(trx_afc_job) == 64 && sizeof(trx_afc_state) == 8 + 32 + 16 * TRX_AFC_RING, "table entry and state");
static_assert(TRX_AFC_LAST == 175 && TRX_AFC_LAST < TRX_MSS_SLOT && TRX_AFC_N > WAVE && TRX_AFC_N <= 2 * WAVE, "two products per lane at most");

__device__ __forceinline__ unsigned uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

/* the row form: row q at iq + q * slot_stride samples */
template <bool I16>
__global__ void __launch_bounds__(kThreads)
ms_fcch_rows_kernel(const void *__restrict__ iq, size_t slot_stride, trxhip_ms_fcch *__restrict__ out, unsigned n_slots, float scale)
{
	const unsigned q = uni(blockIdx.x * WPB + (threadIdx.x >> 6));
	if (q >= n_slots)
		return;
	const int lane = (int)(threadIdx.x & 63);
	const char *row = static_cast<const char *>(iq) + (size_t)q * slot_stride * (I16 ? 4 : 8);
	const trxhip_ms_fcch o = afc_measure<I16>(row, scale, lane);
	if (lane == 0)
		out[q] = o;
}

/* FCCH slot j of a job: measured where the receiver reads it, stored, and into the member's state -- every wave of a pull that
 * measures one of the member's last TRX_AFC_RING FCCH slots writes its own ring entry, the last of them the count and the record */
template <bool I16>
__device__ __forceinline__ void afc_job_slot(const trx_afc_job &e, unsigned j, float scale, int lane)
{
	uint64_t frames;
	const uint64_t k = trx_afc_slot(e.fn0, (int)e.tn0, j, &frames);
	const bool edge = e.edge_row != nullptr;
	const char *row = (edge && k == 0) ? static_cast<const char *>(e.edge_row)
					   : static_cast<const char *>(e.chunk) + (e.first + (int64_t)(k - (edge ? 1u : 0u)) * TRX_MSS_SLOT) * (I16 ? 4 : 8);
	const trxhip_ms_fcch o = afc_measure<I16>(row, scale, lane);
	if (lane != 0)
		return;
	if (e.out)
		e.out[k] = o;
	trx_afc_state *st = e.state;
	if (j + TRX_AFC_RING >= e.n_fcch) {
		trxhip_ms_afc_entry r;
		r.fn = (uint32_t)(((uint64_t)e.fn0 + frames) % TRX_MSS_HYPERFRAME);
		r.hz = o.hz;
		r.mag_one = o.mag_one;
		r.energy = o.energy;
		st->ring[(e.count + j) % TRX_AFC_RING] = r;
	}
	if (j + 1u == e.n_fcch) {
		st->last = o;
		st->count = e.count + e.n_fcch;
	}
}

template <bool I16>
__global__ void __launch_bounds__(kThreads)
ms_fcch_stream_kernel(const trx_afc_job e, float scale)
{
	const unsigned j = uni(blockIdx.x * WPB + (threadIdx.x >> 6));
	if (j < e.n_fcch)
		afc_job_slot<I16>(e, j, scale, (int)(threadIdx.x & 63));
}

template <bool I16>
__global__ void __launch_bounds__(kThreads)
ms_fcch_group_kernel(const trx_afc_job *__restrict__ tab, unsigned n_jobs, unsigned n_waves, float scale)
{
	const unsigned gw = uni(blockIdx.x * WPB + (threadIdx.x >> 6));
	if (gw >= n_waves)
		return;
	unsigned lo = 0, hi = n_jobs;                                  // tab[lo].first_wave <= gw < tab[hi].first_wave
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) >> 1;
		if (tab[mid].first_wave <= gw)
			lo = mid;
		else
			hi = mid;
	}
	const trx_afc_job e = tab[lo];
	afc_job_slot<I16>(e, gw - e.first_wave, scale, (int)(threadIdx.x & 63));
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO; }

unsigned blocks(size_t n) { return (unsigned)((n + WPB - 1) / WPB); }

int fcch_batch(trxhip_ctx *ctx, const void *d_iq, int i16, size_t slot_stride, trxhip_ms_fcch *d_out, size_t n_slots, float rx_full_scale,
	       void *stream)
{
	if (!ctx || !d_iq || (reinterpret_cast<uintptr_t>(d_iq) & (i16 ? 3 : 7)) || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 3) ||
	    n_slots == 0 || n_slots > 0x7fffffffull || slot_stride < TRX_MSS_SLOT)
		return TRXHIP_EINVAL;
	if (!std::isfinite(rx_full_scale) || rx_full_scale <= 0.0f)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_ms_fcch_rows(d_iq, i16, slot_stride, d_out, n_slots, 1.0f / rx_full_scale, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" int trx_launch_ms_fcch_rows(const void *d_iq, int i16, size_t slot_stride, trxhip_ms_fcch *d_out, size_t n_slots, float scale,
				       hipStream_t stream)
{
	if (n_slots == 0)
		return 0;
	if (i16)
		hipLaunchKernelGGL(ms_fcch_rows_kernel<true>, dim3(blocks(n_slots)), dim3(kThreads), 0, stream, d_iq, slot_stride, d_out,
				   (unsigned)n_slots, scale);
	else
		hipLaunchKernelGGL(ms_fcch_rows_kernel<false>, dim3(blocks(n_slots)), dim3(kThreads), 0, stream, d_iq, slot_stride, d_out,
				   (unsigned)n_slots, scale);
	return launched();
}

extern "C" int trx_launch_ms_afc(const trx_afc_job *h_job, const trx_afc_job *d_tab, int i16, size_t n_jobs, size_t n_waves, float scale,
				 hipStream_t stream)
{
	if (n_jobs == 0 || n_waves == 0)
		return 0;
	if (n_jobs > n_waves || n_waves > 0x7fffffffu)
		return TRXHIP_EINVAL;
	if (h_job && i16)
		hipLaunchKernelGGL(ms_fcch_stream_kernel<true>, dim3(blocks(n_waves)), dim3(kThreads), 0, stream, *h_job, scale);
	else if (h_job)
		hipLaunchKernelGGL(ms_fcch_stream_kernel<false>, dim3(blocks(n_waves)), dim3(kThreads), 0, stream, *h_job, scale);
	else if (i16)
		hipLaunchKernelGGL(ms_fcch_group_kernel<true>, dim3(blocks(n_waves)), dim3(kThreads), 0, stream, d_tab, (unsigned)n_jobs,
				   (unsigned)n_waves, scale);
	else
		hipLaunchKernelGGL(ms_fcch_group_kernel<false>, dim3(blocks(n_waves)), dim3(kThreads), 0, stream, d_tab, (unsigned)n_jobs,
				   (unsigned)n_waves, scale);
	return launched();
}

extern "C" {

int trxhip_ms_fcch_batch_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t slot_stride, trxhip_ms_fcch *d_out, size_t n_slots,
			     float rx_full_scale, void *stream)
{
	return fcch_batch(ctx, d_iq, 1, slot_stride, d_out, n_slots, rx_full_scale, stream);
}

int trxhip_ms_fcch_batch_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, size_t slot_stride, trxhip_ms_fcch *d_out, size_t n_slots,
			      float rx_full_scale, void *stream)
{
	return fcch_batch(ctx, d_iq_cf32, 0, slot_stride, d_out, n_slots, rx_full_scale, stream);
}

}  // extern "C"
