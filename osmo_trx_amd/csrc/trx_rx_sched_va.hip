// trx_rx_sched_va.hip -- the kernels of the uplink burst scheduler's Viterbi-equaliser flow (cfg->use_va, TRXHIP_FLAG_USE_VA;
// Transceiver.cpp:760-787): the slots of a pull are read where they lie, as trx_rx_sched.hip's other flow reads them.
//   rx_va_prep_kernel<T>  per slot, one pass: the detector's view of it -- shift_vec, samples 20 .. 604 in front and 40 zeros
//                         behind (:679, :762, :768), in the stream's own format -- and energyDetect(slot, 20 * sps) of the slot
//                         as read (:724-752), the sum in energy_detect_kernel's order (trx_aux_kernels.hip)
//   rx_va_slot_kernel<T>  scaleVector(burst, 1/16383) + demodAnyBurst_va() (:620-645, :782-784) + vectorSlicer over the unshifted
//                         slots the detector found (rc > 0, the CorrType): va_demod_kernel (trx_va.hip) with the slot's place in
//                         the stream for a row and, for int16 streams, convert_short_float folded into the LDS fill
// Slot b = chan * n_slots + k of a pull lies at in + chan * in_stride + k * 625 - carried; with a straddling row (edge != NULL)
// slot 0 of channel chan is edge + chan * 625 instead.  T: one IQ sample (uint32_t: int16 pair; float2).
#include "trx_va_common.h"
#include "trx_launch.h"
#include "trx_rx_sched.h"

namespace {

constexpr int kSlot = TRX_RXS_SLOT;
constexpr int kShift = 20;                 // rif_va_wrapper reads 20 samples early (osmo-trx.cpp:84-99)
constexpr int kXA = VA_XA(kSlot);
constexpr int kRounds = (kSlot + WAVE - 1) / WAVE;   // a wave covers a slot in 10 rounds of 64 samples
constexpr int kWpb = 2;                    // waves per workgroup of rx_va_slot_kernel, as va_demod_kernel has them
// per-wave LDS slice of rx_va_slot_kernel: trx_va.hip's, for L = 625
constexpr size_t kSliceBytes = (size_t)(4 * kXA + 64 + VA_FL + 32) * sizeof(c32) + 64 * sizeof(float) +
			       (size_t)VA_BPW * (VA_FSTRIDE * sizeof(float) + 8 * sizeof(c32)) + VA_BPW * 16;

// convert_short_float: the int16 pair as floats; a complex64 sample as it is
__device__ __forceinline__ c32 as_c32(uint32_t w) { return make_float2((float)(int16_t)(w & 0xffffu), (float)(int16_t)(w >> 16)); }
__device__ __forceinline__ c32 as_c32(float2 v) { return v; }
__device__ __forceinline__ void set_zero(uint32_t &w) { w = 0u; }
__device__ __forceinline__ void set_zero(float2 &v) { v = make_float2(0.0f, 0.0f); }

template <typename T>
__device__ __forceinline__ const T *slot_ptr(const T *in, size_t in_stride, const T *edge, uint32_t carried, uint32_t n_slots, uint32_t b)
{
	const uint32_t chan = b / n_slots, k = b - chan * n_slots;     /* b < chans * max_slots <= 2^23 */
	if (edge && k == 0)
		return edge + (size_t)chan * kSlot;
	return in + ((ptrdiff_t)(chan * in_stride + (size_t)k * kSlot) - (ptrdiff_t)carried);
}

// one wave per slot, four per workgroup
template <typename T>
__global__ void __launch_bounds__(256)
rx_va_prep_kernel(const T *__restrict__ in, size_t in_stride, const T *__restrict__ edge, uint32_t carried, uint32_t n_slots,
		  uint32_t total, T *__restrict__ shift, float *__restrict__ energy)
{
	const int lane = threadIdx.x & 63;
	const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (b >= total)
		return;
	const T *x = slot_ptr(in, in_stride, edge, carried, n_slots, b);
	T *row = shift + (size_t)b * kSlot;
	T v[kRounds];                                                  // every load of the slot in flight before the first store
#pragma unroll
	for (int r = 0; r < kRounds; r++) {
		const int i = lane + WAVE * r;
		set_zero(v[r]);
		if (i < kSlot - 2 * kShift)
			v[r] = x[i + kShift];
	}
#pragma unroll
	for (int r = 0; r < kRounds; r++) {
		const int i = lane + WAVE * r;
		if (i < kSlot)
			row[i] = v[r];
	}
	// energyDetect (sigProcLib.cpp:1573-1585), window 20 * sps = 80 samples at stride 4 from sample 0
	float e = 0.0f;
	for (unsigned i = lane; i < 80u; i += 64) {
		const c32 v = as_c32(x[4 * i]);
		e += v.y * v.y + v.x * v.x;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		e += __shfl_xor(e, o, 64);
	if (lane == 0)
		energy[b] = e / 80.0f;
}

// one wave per four slots; the body is va_demod_kernel's (trx_va.hip) with L = 625, slicing on and no start positions
template <typename T>
__global__ void __launch_bounds__(kWpb * WAVE)
rx_va_slot_kernel(const T *__restrict__ in, size_t in_stride, const T *__restrict__ edge, uint32_t carried, uint32_t n_slots,
		  unsigned total, const trxhip_burst_params *__restrict__ params, const trxhip_burst_result *__restrict__ detected,
		  float *__restrict__ soft, float scale, int soft_stride)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int lane = threadIdx.x & (WAVE - 1);
	const int wave = uni((int)(threadIdx.x >> 6));
	char *base = smem + (size_t)wave * kSliceBytes;
	c32 *xs = reinterpret_cast<c32 *>(base);                       // polyphase: sample i at xs[(i & 3) * kXA + (i >> 2)]
	c32 *corr = xs + 4 * kXA;
	c32 *cir = corr + 64;
	c32 *seq = cir + VA_FL;
	float *power = reinterpret_cast<float *>(seq + 32);
	c32 *prod = seq;                                               // 64 c32 over seq[] + power[]: the autocorrelation products
	float *sym_all = power + 64;
	c32 *rhh_all = reinterpret_cast<c32 *>(sym_all + VA_BPW * VA_FSTRIDE);
	int4 *meta = reinterpret_cast<int4 *>(rhh_all + VA_BPW * 8);
	uint4 *words = reinterpret_cast<uint4 *>(xs);                  // 148 x 16 bytes over the head of xs[]

	const unsigned q0 = (blockIdx.x * kWpb + wave) * VA_BPW;       // first slot of this wave
	if (q0 >= total)
		return;

	// =================== front end, one slot at a time (all 64 lanes) ===================
	for (int qb = 0; qb < VA_BPW; qb++) {
		const unsigned b = q0 + qb;
		float *sym = sym_all + qb * VA_FSTRIDE;
		c32 *rhh = rhh_all + qb * 8;
		if (b >= total) {                                          // grid tail: an idle row
			if (lane == 0) meta[qb] = make_int4(0, 0, -1, 0);
			continue;
		}
		const unsigned prm = reinterpret_cast<const uint32_t *>(params)[2 * (size_t)b];
		const int tsc = (prm >> 8) & 0xff, max_toa = prm >> 16;
		const int type = uni(detected[b].rc);                      // rc > 0 is the CorrType (Transceiver.cpp:784)
		if (tsc > 7 || type <= 0) {                                // not detected (OFF, muted and IDLE slots too): a zero row
			float *so = soft + (size_t)b * soft_stride;
			for (int i = lane; i < soft_stride; i += WAVE) so[i] = 0.0f;
			if (lane == 0) meta[qb] = make_int4(0, 0, -1, 0);
			continue;
		}
		const bool nb = (type == TRXHIP_TSC);                      // Transceiver.cpp:629: TSC, else the access branch
		const int nbits = nb ? VA_NB : VA_AB;

		// ---- convert_short_float + scaleVector in the fill: (float)v * scale
		const T *src = slot_ptr(in, in_stride, edge, carried, n_slots, b);
		{
			// sample lane + 64 r: phase lane & 3, entry (lane >> 2) + 16 r; the slot's loads go out together
			c32 *xp = xs + (lane & 3) * kXA + (lane >> 2);
			T w[kRounds];
#pragma unroll
			for (int r = 0; r < kRounds; r++) {
				set_zero(w[r]);
				if (lane + WAVE * r < kSlot)
					w[r] = src[lane + WAVE * r];
			}
#pragma unroll
			for (int r = 0; r < kRounds; r++)
				if (lane + WAVE * r < kSlot) {
					const c32 v = as_c32(w[r]);
					xp[16 * r] = make_float2(v.x * scale, v.y * scale);
				}
		}
		for (int i = kSlot + lane; i < 4 * kXA; i += WAVE)         // zero behind the slot
			xs[(i & 3) * kXA + (i >> 2)] = make_float2(0.0f, 0.0f);
		wave_sync();

		// ---- get_chan_imp_resp (grgsm_vitac.cpp:183-232)
		const int center = nb ? (3 + 58 + 5) : (8 + 5);
		const int start_pos = (center - 5) * VA_OSR + 1, stop_pos = (center + 5 + VA_CIR) * VA_OSR;
		const int nw = stop_pos - start_pos;                       // 59
		{
			const int j0 = start_pos + (lane < nw ? lane : 0);
			const c32 *p = xs + (j0 & 3) * kXA + (j0 >> 2);
			trx_v2f r;
			switch (nb ? tsc : 8) {
			case 0: r = va_corr<VA_TSC_CODES0, 16>(p); break;
			case 1: r = va_corr<VA_TSC_CODES1, 16>(p); break;
			case 2: r = va_corr<VA_TSC_CODES2, 16>(p); break;
			case 3: r = va_corr<VA_TSC_CODES3, 16>(p); break;
			case 4: r = va_corr<VA_TSC_CODES4, 16>(p); break;
			case 5: r = va_corr<VA_TSC_CODES5, 16>(p); break;
			case 6: r = va_corr<VA_TSC_CODES6, 16>(p); break;
			case 7: r = va_corr<VA_TSC_CODES7, 16>(p); break;
			default: r = va_corr<VA_ACC_CODES, 31>(p); break;
			}
			const c32 c = nb ? make_float2(r.x * 0.0625f, -r.y * 0.0625f) : make_float2(r.x / 31.0f, -r.y / 31.0f);
			if (lane < nw) {
				corr[lane] = c;
				const float h = (float)sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);   // abs(): hypotf
				power[lane] = (float)((double)h * (double)h);      // std::pow(float, int)
			}
		}
		wave_sync();
		// sliding 20-sample window energy (:199-214) as a serial DPP scan, its first maximum
		int best;
		{
			const float pw = (lane < nw) ? power[lane] : 0.0f;
			const float pp = (lane >= VA_FL && lane < nw) ? power[lane - VA_FL] : 0.0f;
			const float q = (lane < VA_FL) ? pw : pw - pp;
			float acc = q;
#pragma unroll
			for (int i = 1; i < 59; i++)
				asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(q));
			const bool inwin = (lane >= VA_FL - 1) && (lane < nw);
			const float e = inwin ? acc : -3.0e38f;
			const float m = wave_max(e);
			const unsigned long long hit = __ballot(inwin && e == m);
			best = hit ? (int)__ffsll((unsigned long long)hit) - 1 - (VA_FL - 1) : 0;
		}
		if (lane < VA_FL)
			cir[lane] = corr[best + lane];
		int start = start_pos + best - center * VA_OSR;
		if (start < 0) start = 0;                                  // Transceiver.cpp:631, :635
		if (lane < VA_FL + 4) {                                    // the matched filter stops at sample start + 4 * nbits
			const int j = start + nbits * VA_OSR + lane;
			xs[(j & 3) * kXA + (j >> 2)] = make_float2(0.0f, 0.0f);
		}
		wave_sync();

		va_rhh_mafi(xs, kXA, cir, prod, rhh, sym, start, nbits, lane);
		if (lane == 0)                                             // Transceiver.cpp:633: rach_max_toa as the start state
			meta[qb] = make_int4(nbits, nb ? 3 : max_toa, start, 0);
		wave_sync();
	}
	wave_sync();

	unsigned ones[5];
	va_trellis(sym_all, rhh_all, meta, words, lane, ones);
	const int row = lane >> 4, l4 = lane & 15;
	const int nbits_row = meta[row].x;

	// ---- +-127 for nbits outputs, zeros behind (:638-641), then vectorSlicer; lane l of a row writes outputs l, l + 16, ...
	const unsigned bme = q0 + row;
	if (bme < total && nbits_row > 0) {
		float *so = soft + (size_t)bme * soft_stride;
#pragma unroll
		for (int t = 0; t < 10; t++) {
			const int i = 16 * t + l4;
			float v = 0.0f;
			if (i < nbits_row)
				v = ((ones[t >> 1] >> (16 * (t & 1) + l4)) & 1u) ? 127.0f : -127.0f;
			v = (i < 148) ? __builtin_amdgcn_fmed3f(0.5f * (v + 1.0f), 0.0f, 1.0f) : 0.0f;
			if (i < soft_stride)
				so[i] = v;
		}
		for (int i = 160 + l4; i < soft_stride; i += 16)
			so[i] = 0.0f;
	}
}

}  // namespace

extern "C" int trx_launch_rx_va_prep(const void *d_in, int cf32, size_t in_stride, const void *d_edge, uint32_t carried, size_t n_slots,
				     int chans, void *d_shift, float *d_energy, hipStream_t stream)
{
	const size_t total = n_slots * (size_t)chans;
	if (total == 0)
		return 0;
	const dim3 grid((unsigned)((total + 3) / 4));
	if (cf32)
		hipLaunchKernelGGL(rx_va_prep_kernel<float2>, grid, dim3(256), 0, stream, static_cast<const float2 *>(d_in), in_stride,
				   static_cast<const float2 *>(d_edge), carried, (uint32_t)n_slots, (uint32_t)total, static_cast<float2 *>(d_shift),
				   d_energy);
	else
		hipLaunchKernelGGL(rx_va_prep_kernel<uint32_t>, grid, dim3(256), 0, stream, static_cast<const uint32_t *>(d_in), in_stride,
				   static_cast<const uint32_t *>(d_edge), carried, (uint32_t)n_slots, (uint32_t)total,
				   static_cast<uint32_t *>(d_shift), d_energy);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" int trx_launch_rx_va_slots(const void *d_in, int cf32, size_t in_stride, const void *d_edge, uint32_t carried, size_t n_slots,
				      int chans, const trxhip_burst_params *d_params, const trxhip_burst_result *d_detected, float *d_soft,
				      float scale, int soft_stride, hipStream_t stream)
{
	const size_t total = n_slots * (size_t)chans;
	if (total == 0)
		return 0;
	const size_t lds = kWpb * kSliceBytes, per_block = kWpb * VA_BPW;
	const dim3 grid((unsigned)((total + per_block - 1) / per_block));
	if (cf32) {
		if (trx_arm_dynamic_lds<rx_va_slot_kernel<float2>>())
			return TRXHIP_EIO;
		hipLaunchKernelGGL(rx_va_slot_kernel<float2>, grid, dim3(kWpb * WAVE), lds, stream, static_cast<const float2 *>(d_in), in_stride,
				   static_cast<const float2 *>(d_edge), carried, (uint32_t)n_slots, (unsigned)total, d_params, d_detected, d_soft,
				   scale, soft_stride);
	} else {
		if (trx_arm_dynamic_lds<rx_va_slot_kernel<uint32_t>>())
			return TRXHIP_EIO;
		hipLaunchKernelGGL(rx_va_slot_kernel<uint32_t>, grid, dim3(kWpb * WAVE), lds, stream, static_cast<const uint32_t *>(d_in),
				   in_stride, static_cast<const uint32_t *>(d_edge), carried, (uint32_t)n_slots, (unsigned)total, d_params,
				   d_detected, d_soft, scale, soft_stride);
	}
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
