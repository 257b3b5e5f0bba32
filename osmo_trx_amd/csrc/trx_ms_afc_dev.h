// trx_ms_afc_dev.h -- the device body of the MS-side FCCH frequency-offset measurement: gsm_fcch_offset() with ac_sum_with_lag() and
// pinv() (Transceiver52M/ms/sch.c:255-314) on the 625 samples of one slot, by one wave.  Written once for the kernels that measure:
// those of trx_ms_afc.hip (rows, and the FCCH slots of a pull) and the pick kernel of trx_ms_fsearch.hip (the slot the FCCH search
// found).  trx_ms_afc.hip's head says what is and what is not reproduced.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/trxhip.h"
#include "trx_ms_afc.h"

namespace {

constexpr int TRX_AFC_WAVE = 64;

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
	for (int s = 1; s < TRX_AFC_WAVE; s <<= 1)
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
		const unsigned s = (unsigned)lane + (unsigned)h * TRX_AFC_WAVE;
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

}  // namespace
