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
// Three forms of one body: rows (trxhip_ms_fcch_batch_*), and the scheduler's stream and group forms, in which a wave finds its
// FCCH slot among the slots of a member's pull by arithmetic on the pull's clock (trx_ms_afc.h) and also moves the member's state.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_afc.h"
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

/* sample i of a slot as ms_rx_kernel makes it: convert_and_scale by 1.f / rxFullScale (ms_upper.cpp:203) */
template <bool I16>
__device__ __forceinline__ float2 afc_load(const void *row, unsigned i, float scale)
{
	if (I16) {
		const short2 v = static_cast<const short2 *>(row)[i];
		return make_float2(__fmul_rn((float)v.x, scale), __fmul_rn((float)v.y, scale));
	}
	const float2 v = static_cast<const float2 *>(row)[i];
	return make_float2(__fmul_rn(v.x, scale), __fmul_rn(v.y, scale));
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
	for (int s = 1; s < WAVE; s <<= 1)
		v += __shfl_xor(v, s);
	return v;
}

/* in[s + lag] * conjf(in[s]) (:277) into (re, im), every product and sum rounded on its own */
__device__ __forceinline__ void afc_mac(float2 a, float2 b, float &re, float &im)
{
	re = __fadd_rn(re, __fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)));
	im = __fadd_rn(im, __fsub_rn(__fmul_rn(a.y, b.x), __fmul_rn(a.x, b.y)));
}

/* gsm_fcch_offset() on the 625 samples at row; the same record in every lane */
template <bool I16>
__device__ __forceinline__ trxhip_ms_fcch afc_measure(const void *row, float scale, int lane)
{
	// ---- ac_sum_with_lag(in, L1, start, N1) and (in, L2, start, N2) (:273-279, :293-294), and the energy of the 92 samples
	float re1 = 0.0f, im1 = 0.0f, re2 = 0.0f, im2 = 0.0f, en = 0.0f;
#pragma unroll
	for (int h = 0; h < 2; h++) {
		const unsigned s = (unsigned)lane + (unsigned)h * WAVE;
		if (s < TRX_AFC_N) {                                       /* s + 52 + 32 <= 175 */
			const float2 x0 = afc_load<I16>(row, TRX_AFC_START + s, scale);
			const float2 x1 = afc_load<I16>(row, TRX_AFC_START + TRX_AFC_L1 + s, scale);
			const float2 x2 = afc_load<I16>(row, TRX_AFC_START + TRX_AFC_L2 + s, scale);
			afc_mac(x1, x0, re1, im1);
			afc_mac(x2, x0, re2, im2);
			en = __fadd_rn(en, __fadd_rn(__fmul_rn(x0.x, x0.x), __fmul_rn(x0.y, x0.y)));
		}
	}
	re1 = wave_sum(re1);
	im1 = wave_sum(im1);
	re2 = wave_sum(re2);
	im2 = wave_sum(im2);
	en = wave_sum(en);

	// ---- :286-313 on wave-uniform values, with the reference's types
	const float fs = (float)(13. / 48. * 1e6 * 4);                                 /* :286 */
	const float expected_fcch_val = (float)(((2 * M_PI) / (double)fs) * 67700);    /* :287 */
	const float alpha_one = atan2f(im1, re1);                                      /* cargf(v), :278 */
	const float alpha_two = atan2f(im2, re2);
	const float lin = __fsub_rn(__fmul_rn((float)TRX_AFC_L1, alpha_two), __fmul_rn((float)TRX_AFC_L2, alpha_one));
	const float P_unrounded = (float)((double)lin / (2 * M_PI));                   /* :296 */
	const int P = (int)roundf(P_unrounded);                                        /* :297 */
	// pinv(), :262-270: the first (i, j), i < 3, j < 32, with P == 32 * i - 3 * j, else the caller's r = s = 0 (:299).  Without the
	// loop: 32 = 2 (mod 3) and 2 * 2 = 1 (mod 3), so P = 2 i (mod 3) fixes i = 2 P mod 3, and then j = (32 i - P) / 3, an exact
	// division; 3 and 32 are coprime, so no P has a second pair and this one is the loop's first (tests/test_ms_afc_cpu.py
	// walks the table).  |P| <= 18: the angles are within +-pi
	int pi3 = (2 * P) % TRX_AFC_L1;
	pi3 += pi3 < 0 ? TRX_AFC_L1 : 0;
	const int pj = (TRX_AFC_L2 * pi3 - P) / TRX_AFC_L1;
	const bool found = pj >= 0 && pj < TRX_AFC_L2;
	const int r = found ? pi3 : 0, s = found ? pj : 0;
	const float omegal1 = (float)(((double)alpha_one + 2 * M_PI * (double)r) / (double)TRX_AFC_L1);    /* :302 */
	const float omegal2 = (float)(((double)alpha_two + 2 * M_PI * (double)s) / (double)TRX_AFC_L2);    /* :303 */
	const float mid = __fsub_rn(expected_fcch_val, __fdiv_rn(__fadd_rn(omegal1, omegal2), 2.0f));
	const float reval = (float)((1625e3 / 6) * 4 / (2 * M_PI) * (double)mid);      /* GSM_SYM_RATE / (2 * M_PI) * (...), :83, :308 */

	trxhip_ms_fcch o;
	o.hz = -reval;                                                                 /* :313 */
	o.alpha_one = alpha_one;
	o.alpha_two = alpha_two;
	o.mag_one = sqrtf(__fadd_rn(__fmul_rn(re1, re1), __fmul_rn(im1, im1)));
	o.mag_two = sqrtf(__fadd_rn(__fmul_rn(re2, re2), __fmul_rn(im2, im2)));
	o.energy = en;
	o.p = (int16_t)P;
	o.r = (int8_t)r;
	o.s = (int8_t)s;
	o.reserved = 0;
	return o;
}

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
