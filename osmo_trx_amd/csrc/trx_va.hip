// trx_va.hip -- the Viterbi alternative of pullRadioVector (cfg->use_va) for gfx950:
// scaleVector(burst, 1/16383) + demodAnyBurst_va() (Transceiver52M/Transceiver.cpp:782-784, :620-645) over gr-gsm's
// receiver in Transceiver52M/grgsm_vitac/: channel impulse response from the training sequence at 4 samples per
// symbol (grgsm_vitac.cpp:147-232, :244-272), matched filter (:168-181), 16-state MLSE (viterbi_detector.cc:62-392).
//
// Mapping: ONE WAVEFRONT PER FOUR BURSTS.  The front end (channel estimate, matched filter) runs burst after burst with
// all 64 lanes; the 16-state trellis and its traceback then run for the four bursts AT ONCE, one burst per DPP row of 16
// lanes -- the add-compare-select butterfly only ever talks to lanes of its own row, and the traceback, the reference's
// serial walk, is carried by the vector lanes of each row instead of the scalar unit (a scalar instruction costs a wave
// the same issue slot as a vector one, and the scalar walk could serve one burst only).
//   * the 59 training-sequence correlations: one lag per lane; |.|^2 the way libstdc++/glibc evaluate
//     std::pow(abs(c), 2): hypot in double, rounded to float, squared in double, rounded to float
//   * the sliding 20-sample energy window and its first maximum: the reference's serial float recurrence, kept
//     serial (59 steps on wave-uniform LDS reads) -- it decides the burst position
//   * matched filter: one output symbol per lane and round, 20 complex taps in order
//   * add-compare-select as a butterfly on 16 lanes: the lane holding old state S produces new state rotl4(S) from
//     its own metric and that of the lane holding S ^ 8, fetched with one DPP move (the state-to-lane map rotates
//     with period 4); the 32 hand-written ACS statements of the reference reduced to their sign/increment pattern; of every
//     path-metric difference only (d > 0, d != 0) matter for the +-127 output, so a step's table row is one ballot
//     word; the traceback is the reference's serial walk on the scalar unit
// Operand order follows the reference statement by statement (-ffp-contract=off): the +-127 outputs are bit-exact.
#include "trx_va_common.h"
#include "trx_launch.h"

#define VA_WPB 2                       // waves per workgroup (11.4 KB of LDS per wave: 14 waves per CU)
// bursts per wave, the burst layout in LDS and the shared device code: trx_va_common.h
// per-wave LDS slice, every region 16-byte aligned:
//   scratch of the burst in the front end: xs[4][XA] | corr[64] | cir[20] | seq[32] : c32;  power[64] : float
//   kept for the trellis, per burst:       sym[4][152] : float | rhh[4][8] : c32;  meta[4] : int4 {nbits, start state, start, -}
//   decision words of the four trellises:  words[148] : uint4 {pos lo, pos hi, nz lo, nz hi} -- over xs[], which the
//                                          front end no longer needs by then
#define VA_SLICE_BYTES(L) ((size_t)(4 * VA_XA(L) + 64 + VA_FL + 32) * sizeof(c32) + 64 * sizeof(float) +                  \
			   (size_t)VA_BPW * (VA_FSTRIDE * sizeof(float) + 8 * sizeof(c32)) + VA_BPW * 16)

// the training sequences' quarter-turn codes (VA_TSC_CODES0 .. 7, VA_ACC_CODES): trx_va_common.h

__global__ void __launch_bounds__(VA_WPB * WAVE)
va_demod_kernel(const c32 *__restrict__ iq, const trxhip_burst_params *__restrict__ params,
		const trxhip_burst_result *__restrict__ detected, float *__restrict__ soft,
		int32_t *__restrict__ starts, unsigned n_bursts, int L, float scale, int soft_stride, int slice)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int lane = threadIdx.x & (WAVE - 1);
	const int wave = uni((int)(threadIdx.x >> 6));
	const int XA = uni(VA_XA(L));
	const size_t slice_bytes = VA_SLICE_BYTES(L);
	char *base = smem + (size_t)wave * slice_bytes;
	c32 *xs = reinterpret_cast<c32 *>(base);                       // polyphase: sample i at xs[(i & 3) * XA + (i >> 2)]
	c32 *corr = xs + 4 * XA;
	c32 *cir = corr + 64;
	c32 *seq = cir + VA_FL;
	float *power = reinterpret_cast<float *>(seq + 32);
	c32 *prod = seq;                                               // 64 c32 over seq[] + power[]: the autocorrelation products
	float *sym_all = power + 64;
	c32 *rhh_all = reinterpret_cast<c32 *>(sym_all + VA_BPW * VA_FSTRIDE);
	int4 *meta = reinterpret_cast<int4 *>(rhh_all + VA_BPW * 8);
	uint4 *words = reinterpret_cast<uint4 *>(xs);                  // 148 x 16 bytes over the head of xs[] (4 * XA >= 672 entries)

	const unsigned q0 = (blockIdx.x * VA_WPB + wave) * VA_BPW;     // first burst of this wave
	if (q0 >= n_bursts)
		return;

	// =================== front end, one burst at a time (all 64 lanes) ===================
	for (int qb = 0; qb < VA_BPW; qb++) {
		const unsigned b = q0 + qb;
		float *sym = sym_all + qb * VA_FSTRIDE;
		c32 *rhh = rhh_all + qb * 8;
		if (b >= n_bursts) {                                       // batch tail: an idle row
			if (lane == 0) meta[qb] = make_int4(0, 0, -1, 0);
			continue;
		}
		const unsigned prm = reinterpret_cast<const uint32_t *>(params)[2 * (size_t)b];
		int type = prm & 0xff;
		const int tsc = (prm >> 8) & 0xff, max_toa = prm >> 16;
		float *so = soft + (size_t)b * soft_stride;
		bool skip = false;
		if (detected) {                                            // chained behind detection: rc is the CorrType (Transceiver.cpp:784)
			const int rc = uni(detected[b].rc);
			skip = rc <= 0;
			type = rc;
		}
		if (tsc > 7 || skip) {                                     // train_seq has 8 entries (+ dummy): reject
			for (int i = lane; i < soft_stride; i += WAVE) so[i] = 0.0f;
			if (starts && lane == 0) starts[b] = -1;
			if (lane == 0) meta[qb] = make_int4(0, 0, -1, 0);
			continue;
		}
		const bool nb = (type == TRXHIP_TSC);                      // Transceiver.cpp:629: TSC, else the access branch
		const int nbits = nb ? VA_NB : VA_AB;

		// ---- scaleVector (sigProcLib.cpp:1198-1205): x * (scale, 0).  Complex.h:74 evaluates (x.r*s - x.i*0, x.r*0 + x.i*s);
		// the products with 0 are +-0 and only ever decide the sign of a zero result, which nothing downstream can see
		// (sums, comparisons, |.|^2): two multiplies per sample instead of four and two additions.
		const c32 *src = iq + (size_t)b * L;
		{
			// sample lane + 64 r: phase lane & 3, entry (lane >> 2) + 16 r -- one address per lane, immediate offsets
			c32 *xp = xs + (lane & 3) * XA + (lane >> 2);
			for (int i = lane, r = 0; i < L; i += WAVE, r++) {
				const c32 v = src[i];
				xp[16 * r] = make_float2(v.x * scale, v.y * scale);
			}
		}
		for (int i = L + lane; i < 4 * XA; i += WAVE)              // zero behind the burst (the reference's "j < L ? x[j] : 0")
			xs[(i & 3) * XA + (i >> 2)] = make_float2(0.0f, 0.0f);
		wave_sync();

		// ---- get_chan_imp_resp (grgsm_vitac.cpp:183-232)
		const int center = nb ? (3 + 58 + 5) : (8 + 5);
		const int start_pos = (center - 5) * VA_OSR + 1, stop_pos = (center + 5 + VA_CIR) * VA_OSR;   // max_delay = 0 (:631)
		const int nw = stop_pos - start_pos;                       // 59
		{
			const int j0 = start_pos + (lane < nw ? lane : 0);
			const c32 *p = xs + (j0 & 3) * XA + (j0 >> 2);
			trx_v2f r;
			switch (nb ? tsc : 8) {                                // wave-uniform: one specialised loop per training sequence
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
			// conj(result) / (length + 0j), length = tseqlen = 26 - 10 / 41 - 10: a division by 16 is an exact scaling
			const c32 c = nb ? make_float2(r.x * 0.0625f, -r.y * 0.0625f) : make_float2(r.x / 31.0f, -r.y / 31.0f);
			if (lane < nw) {
				corr[lane] = c;
				const float h = (float)sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);   // abs(): hypotf
				power[lane] = (float)((double)h * (double)h);      // std::pow(float, int)
			}
		}
		wave_sync();
		// sliding 20-sample window energy (:199-214): ws = p[0] + ... + p[19], then ws += p[i] - p[i-20].  With q[i] = p[i]
		// (i < 20) or p[i] - p[i-20], the window sums are the left-to-right prefix sums of q: a serial DPP scan along the
		// lanes reproduces the reference's additions one for one (lane 19 + j ends with window j's energy).
		int best;
		{
			const float pw = (lane < nw) ? power[lane] : 0.0f;
			const float pp = (lane >= VA_FL && lane < nw) ? power[lane - VA_FL] : 0.0f;
			const float q = (lane < VA_FL) ? pw : pw - pp;
			float acc = q;
#pragma unroll
			for (int i = 1; i < 59; i++)                           // nw = 59 for both burst types
				asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(q));
			const bool inwin = (lane >= VA_FL - 1) && (lane < nw);
			const float e = inwin ? acc : -3.0e38f;
			const float m = wave_max(e);
			const unsigned long long hit = __ballot(inwin && e == m);  // std::max_element: the first largest
			best = hit ? (int)__ffsll((unsigned long long)hit) - 1 - (VA_FL - 1) : 0;
		}
		if (lane < VA_FL)
			cir[lane] = corr[best + lane];
		int start = start_pos + best - center * VA_OSR;
		if (start < 0) start = 0;                                  // Transceiver.cpp:631, :635
		// the matched filter stops at sample start + 4 * nbits ("if (a + ii >= nbits * OSR) break", :99-100): the same
		// condition for every output, i.e. the samples from there on do not exist -- zero them (adding +-0 changes no sum)
		if (lane < VA_FL + 4) {
			const int j = start + nbits * VA_OSR + lane;
			xs[(j & 3) * XA + (j >> 2)] = make_float2(0.0f, 0.0f);
		}
		wave_sync();

		va_rhh_mafi(xs, XA, cir, prod, rhh, sym, start, nbits, lane);
		if (lane == 0)                                             // Transceiver.cpp:633: rach_max_toa as the start state
			meta[qb] = make_int4(nbits, nb ? 3 : max_toa, start, 0);
		wave_sync();                                               // xs / corr / cir / seq are the next burst's scratch
	}
	wave_sync();

	unsigned ones[5];
	va_trellis(sym_all, rhh_all, meta, words, lane, ones);
	const int row = lane >> 4, l4 = lane & 15;
	const int4 mt = meta[row];
	const int nbits_row = mt.x;

	// ---- "pre flip" (:107), "* -1" (Transceiver.cpp:638), zeros behind the burst (:640-641); optional vectorSlicer.
	// Lane l of a row writes outputs l, l + 16, ... of its burst.
	const unsigned bme = q0 + row;
	if (bme < n_bursts && nbits_row > 0) {
		float *so = soft + (size_t)bme * soft_stride;
#pragma unroll
		for (int t = 0; t < 10; t++) {                             // outputs 0 .. 159; bit (16 t + l4) of the 160-bit string
			const int i = 16 * t + l4;
			float v = 0.0f;
			if (i < nbits_row)
				v = ((ones[t >> 1] >> (16 * (t & 1) + l4)) & 1u) ? 127.0f : -127.0f;
			if (slice & 1)
				v = (i < 148) ? __builtin_amdgcn_fmed3f(0.5f * (v + 1.0f), 0.0f, 1.0f) : 0.0f;
			if (i < soft_stride)
				so[i] = v;
		}
		for (int i = 160 + l4; i < soft_stride; i += 16)
			so[i] = (slice & 1) ? 0.0f : 0.0f;
		if (starts && l4 == 0)
			starts[bme] = mt.z;
	}
}

extern "C" size_t trx_va_lds_bytes(int L)
{
	return VA_WPB * VA_SLICE_BYTES(L);
}

extern "C" int trx_launch_va_demod(const float *d_iq, const trxhip_burst_params *d_params,
				   const trxhip_burst_result *d_detected, float *d_soft, int32_t *d_starts,
				   size_t n_bursts, int L, float scale, int soft_stride, int flags, hipStream_t stream)
{
	if (n_bursts == 0)
		return 0;
	const size_t lds = trx_va_lds_bytes(L);
	if (lds > 160 * 1024)
		return TRXHIP_EINVAL;
	if (trx_arm_dynamic_lds<va_demod_kernel>())
		return TRXHIP_EIO;
	const size_t per_block = VA_WPB * VA_BPW;
	const size_t grid = (n_bursts + per_block - 1) / per_block;
	hipLaunchKernelGGL(va_demod_kernel, dim3((unsigned)grid), dim3(VA_WPB * WAVE), lds, stream,
			   reinterpret_cast<const c32 *>(d_iq), d_params, d_detected, d_soft, d_starts, (unsigned)n_bursts, L, scale, soft_stride,
			   flags);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
