// trx_tx.hip -- the transmit side: the GMSK / 8-PSK burst modulators of sigProcLib.cpp (modulateBurst :970-979,
// modulateEdgeBurst :917-936) batched over N bursts, plus the TRXD downlink front (Transceiver.cpp:1087-1185, :373-399) and
// the host generator of the transmit tables (trx_tx_tables.h).
//
// Kernel shape.  One wave per burst, four bursts per 256-thread workgroup.  The wave stages the burst's bits (bit 0 of each
// byte) in LDS, then the symbol-rate values the reference places at every sps-th sample of its upsampled vectors (c0 and c1
// of the Laurent modulator, the rotated 8-PSK symbols, the rotated 1-SPS symbols), then writes the row: every lane two samples
// per round, 16-byte non-temporal stores for cf32 (8 bytes for int16), the row zero-filled behind the burst up to out_stride.
// The kernel is store-bound: a 4-SPS burst is 5000 bytes of cf32 or 2500 of int16 against ~150 bytes of bits.
//
// Exactness.  The reference convolves (START_ONLY, sigProcLib.cpp:297-398 -> convolve_base.c:28-33, generic C) the upsampled
// vector with the pulse: y[i] = sum_{k=0..H-1} x[i - (H-1) + k] * h[k], in ascending k, from 0.0f.  x is zero except at
// multiples of sps, so here only the taps that meet a symbol position are summed, still in ascending k and still from 0.0f
// (the argument is stated at sum_sparse4()).  All rotations and phasors come from the tables; the device computes no cos / sin / pow.  Built with
// -ffp-contract=off (build.py): no multiply-add is fused.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/trxhip.h"
#include "trx_tx_tables.h"
#include "trx_tx_sched.h"
#include "trx_ms_tx.h"
#include "trx_ms_nco.h"
#include "trx_launch.h"

typedef float2 c32;
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));

#define TX_WAVES 4                 /* bursts (waves) per workgroup */
#define TX_SYMS 160                /* symbol slots per burst in LDS: 157 used (positions 0 .. 624 at 4 SPS, 0 .. 156 at 1 SPS) */
#define TX_BITS 480                /* bit bytes per burst in LDS: 468 used */

enum { TX_LAURENT = 0, TX_BASIC1 = 1, TX_ROTATE = 2, TX_EDGE4 = 3, TX_EDGE_ROTATE = 4 };

struct trx_tx_desc {
	int mode, nbits, len, status;
	c32 scale;
	bool scaled;
};

// The range checks of include/trxhip.h: the mode and the length of a burst, or status TRXHIP_EINVAL and length 0.
__device__ static inline trx_tx_desc tx_describe(int nbits, int guard, int flags, int sps, size_t bits_stride, size_t out_stride)
{
	trx_tx_desc d;
	d.nbits = nbits;
	d.status = TRXHIP_EINVAL;
	d.len = 0;
	d.mode = TX_LAURENT;
	d.scale = make_float2(1.0f, 0.0f);
	d.scaled = false;
	if (flags & ~(TRXHIP_TX_8PSK | TRXHIP_TX_EMPTY_PULSE) || (size_t)nbits > bits_stride)
		return d;
	int len = 0;
	if (flags & TRXHIP_TX_8PSK) {
		if (nbits % 3 != 0 || nbits > 3 * TRX_TX_EDGE_SYMS)
			return d;
		if (flags & TRXHIP_TX_EMPTY_PULSE) {
			if (nbits < 3)
				return d;
			d.mode = TX_EDGE_ROTATE;
			len = sps * (nbits / 3);
		} else {
			if (sps != 4)
				return d;
			d.mode = TX_EDGE4;
			len = 625;
		}
	} else if (flags & TRXHIP_TX_EMPTY_PULSE) {
		len = sps * (nbits + guard);
		if (len < 1 || len > (sps == 4 ? 625 : 157))
			return d;
		d.mode = TX_ROTATE;
	} else if (sps == 4) {
		if (nbits < 2 || nbits > 155)
			return d;
		d.mode = TX_LAURENT;
		len = 625;
	} else {
		len = nbits + guard;
		if (len < 1 || len > 157)
			return d;
		d.mode = TX_BASIC1;
	}
	if ((size_t)len > out_stride)
		return d;
	d.len = len;
	d.status = 0;
	return d;
}

// Complex<float> operator* (Complex.h:73): (r*a.r - i*a.i, r*a.i + i*a.r)
__device__ static inline c32 cmul(c32 x, c32 a) { return make_float2(x.x * a.x - x.y * a.y, x.x * a.y + x.y * a.x); }

// y[i] of the 4-SPS START_ONLY convolution with an H-tap real pulse h (H = 16: c0, H = 8: c1) over a vector that is nonzero
// only at positions 4m, whose values are sym[m] (m < TX_SYMS; the vector is 625 samples, so m <= 156).
// The reference sums all H taps from 0.0f in ascending k: yr += x[j].re * h[k], j = i - (H-1) + k.  The skipped terms have
// x[j] = (+-0, +-0), so each is a product +-0.  A sum that starts at +0.0f is never -0 in round-to-nearest (a + b is -0 only
// if a and b are both -0), and s + (+-0) == s for every s that is not -0.  So adding the skipped terms would not change
// one bit: summing only the contributing taps (at most 4 for c0, 2 for c1), in the same ascending order and from the same
// 0.0f, gives the reference's float.
template <int H>
__device__ static inline c32 sum_sparse4(const c32 *sym, const float *h, int i)
{
	float yr = 0.0f, yi = 0.0f;
	int m = (i - (H - 1) + 3) >> 2;            /* first symbol position 4m >= i - (H-1) */
	if (m < 0)
		m = 0;
	for (; 4 * m <= i && m <= 156; m++) {
		const c32 x = sym[m];
		const float t = h[4 * m - i + (H - 1)];
		yr += x.x * t;
		yi += x.y * t;
	}
	return make_float2(yr, yi);
}

struct tx_lds {
	c32 sym0[TX_WAVES][TX_SYMS];               /* c0 / 8-PSK / 1-SPS symbol values */
	c32 sym1[TX_WAVES][TX_SYMS];               /* c1 of the Laurent modulator */
	uint8_t bits[TX_WAVES][TX_BITS];
	float p0[16], p1[8], q1[4];                /* pulse4_c0, pulse4_c1, pulse1_c0 */
};

struct tx_att_table { float s[256]; };

// TRXD: the datagram's header decides the descriptor (driveTxPriorityQueue(), Transceiver.cpp:1099-1130; addRadioVector()
// :388-396).  Returns the bits' address.
__device__ static inline const uint8_t *trxd_describe(const uint8_t *dg, int dlen, size_t dgram_stride, int sps, const tx_att_table &att,
						       size_t out_stride, trx_tx_desc &d, trxhip_tx_info &info)
{
	const uint8_t h0 = dg[0];
	info.tn = h0 & 7;
	info.version = h0 >> 4;
	info.fn = ((uint32_t)dg[1] << 24) | ((uint32_t)dg[2] << 16) | ((uint32_t)dg[3] << 8) | (uint32_t)dg[4];
	info.tx_att = dg[5];
	info.mod_8psk = 0;
	int nbits = 0, flags = 0, status = 0;
	if (dlen == 6 + 148) {
		nbits = 148;
	} else if (dlen == 6 + 444) {
		nbits = 444;
		flags = TRXHIP_TX_8PSK;
		info.mod_8psk = 1;
		if (sps != 4)
			status = TRXHIP_ENOTSUP;
	} else {
		status = TRXHIP_EINVAL;
	}
	if (info.version > 1 || (size_t)dlen > dgram_stride)
		status = TRXHIP_EINVAL;
	d = tx_describe(nbits, 8 + (info.tn % 4 == 0), flags, sps, dgram_stride - 6, out_stride);
	if (status != 0) {
		d.status = status;
		d.len = 0;
	}
	if (d.status == 0) {
		d.scale = make_float2(att.s[info.tx_att], 0.0f);        /* scaleVector(*burst, complex(scale)): imaginary part 0 */
		d.scaled = true;
	}
	info.nbits = d.status == 0 ? (uint16_t)nbits : 0;
	info.length = (uint16_t)d.len;
	info.status = d.status;
	return dg + 6;
}

template <bool TRXD>
__global__ void __launch_bounds__(64 * TX_WAVES)
tx_modulate_kernel(const uint8_t *__restrict__ in, size_t in_stride, const trxhip_tx_params *__restrict__ params,
		   const uint16_t *__restrict__ dgram_len, tx_att_table att, const trx_tx_tables *__restrict__ tab,
		   float *__restrict__ out_cf32, int16_t *__restrict__ out_s16, float s16_scale, size_t out_stride,
		   int32_t *__restrict__ out_len, trxhip_tx_info *__restrict__ info_out, size_t n, int sps)
{
	__shared__ tx_lds L;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const size_t b = (size_t)blockIdx.x * TX_WAVES + w;
	const bool active = b < n;

	if (threadIdx.x < 16)
		L.p0[threadIdx.x] = tab->pulse4_c0[threadIdx.x];
	else if (threadIdx.x < 24)
		L.p1[threadIdx.x - 16] = tab->pulse4_c1[threadIdx.x - 16];
	else if (threadIdx.x < 28)
		L.q1[threadIdx.x - 24] = tab->pulse1_c0[threadIdx.x - 24];

	// ---- descriptor (wave-uniform) ----
	trx_tx_desc d;
	d.status = TRXHIP_EINVAL;
	d.len = 0;
	d.nbits = 0;
	d.mode = TX_LAURENT;
	d.scaled = false;
	const uint8_t *bits = nullptr;
	if (active) {
		if (TRXD) {
			trxhip_tx_info info;
			bits = trxd_describe(in + b * in_stride, dgram_len[b], in_stride, sps, att, out_stride, d, info);
			if (info_out && lane == 0)
				info_out[b] = info;
		} else {
			const trxhip_tx_params p = params[b];
			d = tx_describe(p.nbits, p.guard, p.flags, sps, in_stride, out_stride);
			d.scale = make_float2(p.scale_re, p.scale_im);
			d.scaled = !(p.scale_re == 1.0f && p.scale_im == 0.0f && !signbit(p.scale_im));
			bits = in + b * in_stride;
		}
		if (out_len && lane == 0)
			out_len[b] = d.status == 0 ? d.len : d.status;
	}
	const bool ok = active && d.status == 0;
	const int nbits = d.nbits, len = d.len;

	// ---- stage the bits: only bit 0 counts (bits[i] & 0x01) ----
	uint8_t *lb = L.bits[w];
	if (ok)
		for (int i = lane; i < nbits; i += 64)
			lb[i] = bits[i] & 0x01;
	__syncthreads();

	// ---- symbol-rate values ----
	c32 *s0 = L.sym0[w], *s1 = L.sym1[w];
	if (ok) {
		const c32 *rot4 = reinterpret_cast<const c32 *>(tab->rot4);
		const c32 *rot1 = reinterpret_cast<const c32 *>(tab->rot1);
		const c32 *psk8 = reinterpret_cast<const c32 *>(tab->psk8);
		const c32 *erot = reinterpret_cast<const c32 *>(tab->edge_rot);
		const c32 zero = make_float2(0.0f, 0.0f);
		for (int m = lane; m < TX_SYMS; m += 64) {
			c32 v0 = zero, v1 = zero;
			if (d.mode == TX_LAURENT) {
				// modulateBurstLaurent :615-656.  c0: padded tail (-1), the bits, padded tail (-1) at 4m, m = 0 .. nbits+1, then
				// GMSKRotate's real branch (*rotPtr * x.real(), :247-251).  c1 = c0 * (0, phase) at m = 2 .. nbits+1, phase -1 at
				// m = 2 (start magic) and 2 (b[m-2] ^ b[m-3]) - 1 after it (the loop and the end magic)
				if (m <= nbits + 1) {
					const float x = (m == 0 || m == nbits + 1) ? -1.0f : (lb[m - 1] ? 1.0f : -1.0f);   /* 2.0 * bit - 1.0 */
					const c32 r = rot4[4 * m];
					v0 = make_float2(r.x * x, r.y * x);
					if (m >= 2) {
						const float ph = (m == 2) ? -1.0f : ((lb[m - 2] ^ lb[m - 3]) ? 1.0f : -1.0f);
						v1 = cmul(v0, make_float2(0.0f, ph));
					}
				}
			} else if (d.mode == TX_BASIC1) {
				// modulateBurstBasic :938-967 at 1 SPS: +-1 at m < nbits, 0 behind, GMSKRotate's real branch over all len samples
				if (m < len) {
					const float x = m < nbits ? (lb[m] ? 1.0f : -1.0f) : 0.0f;
					const c32 r = rot1[m];
					v0 = make_float2(r.x * x, r.y * x);
				}
			} else if (d.mode == TX_EDGE4 || d.mode == TX_EDGE_ROTATE) {
				// mapEdgeSymbols :713-729 then symbol * rot (shapeEdgeBurst :750-756 one symbol late; rotateEdgeBurst :680-686)
				const int k = d.mode == TX_EDGE4 ? m - 1 : m;
				if (k >= 0 && k < nbits / 3) {
					const unsigned idx = (unsigned)lb[3 * k] | ((unsigned)lb[3 * k + 1] << 1) | ((unsigned)lb[3 * k + 2] << 2);
					v0 = cmul(psk8[idx], erot[k]);
				}
			}
			s0[m] = v0;
			s1[m] = v1;
		}
	}
	__syncthreads();
	if (!active)
		return;

	// ---- the row: samples [0, len) of the burst, zeros behind it up to out_stride ----
	const c32 *rot = reinterpret_cast<const c32 *>(sps == 4 ? tab->rot4 : tab->rot1);
	auto sample = [&](int i) -> c32 {
		c32 y = make_float2(0.0f, 0.0f);
		if (i >= len)
			return y;
		switch (d.mode) {
		case TX_LAURENT: {
			// c0_shaped + c1_shaped (:659-666): each convolution summed on its own, then added
			const c32 a = sum_sparse4<16>(s0, L.p0, i), c = sum_sparse4<8>(s1, L.p1, i);
			y = make_float2(a.x + c.x, a.y + c.y);
			break;
		}
		case TX_EDGE4:
			y = sum_sparse4<16>(s0, L.p0, i);
			break;
		case TX_BASIC1: {
			// every sample is a symbol position at 1 SPS: the plain 4-tap START_ONLY sum, x[j] = 0 outside [0, len)
			float yr = 0.0f, yi = 0.0f;
			for (int k = 0; k < 4; k++) {
				const int j = i - 3 + k;
				if (j >= 0) {
					yr += s0[j].x * L.q1[k];
					yi += s0[j].y * L.q1[k];
				}
			}
			y = make_float2(yr, yi);
			break;
		}
		case TX_ROTATE: {
			// rotateBurst :558-580: (+-1, 0) at every sps-th sample, GMSKRotate's complex branch, then the 1-tap empty pulse
			// (real taps: 0.0f + x.re * 1.0f)
			const int m = i / sps;
			const float x = (i == m * sps && m < nbits) ? (lb[m] ? 1.0f : -1.0f) : 0.0f;
			const c32 v = cmul(rot[i], make_float2(x, 0.0f));
			y = make_float2(0.0f + v.x * 1.0f, 0.0f + v.y * 1.0f);
			break;
		}
		default: {                             /* TX_EDGE_ROTATE: no filter, zeros between the symbols */
			const int m = i / sps;
			if (i == m * sps)
				y = s0[m];
			break;
		}
		}
		if (d.scaled)                          /* scaleVector's complex branch, :1199-1203 */
			y = make_float2(y.x * d.scale.x - y.y * d.scale.y, y.x * d.scale.y + y.y * d.scale.x);
		return y;
	};

	const int stride = (int)out_stride;
	if (out_cf32) {
		float *row = out_cf32 + 2 * b * out_stride;
		const int head = (reinterpret_cast<uintptr_t>(row) & 15) ? 1 : 0;     /* sample 0 alone when the row is 8-byte aligned */
		if (head && lane == 0) {
			const c32 y = sample(0);
			__builtin_nontemporal_store((f2v){y.x, y.y}, reinterpret_cast<f2v *>(row));
		}
		for (int i0 = head + 2 * lane; i0 < stride; i0 += 128) {
			const c32 y0 = sample(i0);
			if (i0 + 1 < stride) {
				const c32 y1 = sample(i0 + 1);
				__builtin_nontemporal_store((f4v){y0.x, y0.y, y1.x, y1.y}, reinterpret_cast<f4v *>(row + 2 * i0));
			} else {
				__builtin_nontemporal_store((f2v){y0.x, y0.y}, reinterpret_cast<f2v *>(row + 2 * i0));
			}
		}
	}
	if (out_s16) {
		// convert_float_short_kernel's expression (trx_aux_kernels.hip): (int16_t)(int)(x * scale)
		int16_t *row = out_s16 + 2 * b * out_stride;
		auto q = [&](float v) -> unsigned { return (unsigned)(uint16_t)(int16_t)(int)(v * s16_scale); };
		const int head = (reinterpret_cast<uintptr_t>(row) & 7) ? 1 : 0;
		if (head && lane == 0) {
			const c32 y = sample(0);
			__builtin_nontemporal_store(q(y.x) | (q(y.y) << 16), reinterpret_cast<unsigned *>(row));
		}
		for (int i0 = head + 2 * lane; i0 < stride; i0 += 128) {
			const c32 y0 = sample(i0);
			if (i0 + 1 < stride) {
				const c32 y1 = sample(i0 + 1);
				__builtin_nontemporal_store((u2v){q(y0.x) | (q(y0.y) << 16), q(y1.x) | (q(y1.y) << 16)},
							    reinterpret_cast<u2v *>(row + 2 * i0));
			} else {
				__builtin_nontemporal_store(q(y0.x) | (q(y0.y) << 16), reinterpret_cast<unsigned *>(row + 2 * i0));
			}
		}
	}
}

extern "C" int trx_launch_tx_modulate(const uint8_t *d_in, size_t in_stride, const trxhip_tx_params *d_params, const uint16_t *d_dgram_len,
				      const float *h_att_scale, const trx_tx_tables *d_tab, float *d_out_cf32, int16_t *d_out_s16,
				      float s16_scale, size_t out_stride, int32_t *d_out_len, trxhip_tx_info *d_info, size_t n, int sps,
				      hipStream_t stream)
{
	if (n == 0)
		return 0;
	const size_t blocks = (n + TX_WAVES - 1) / TX_WAVES;
	if (blocks > 0x7fffffffu)
		return TRXHIP_EINVAL;
	tx_att_table att;
	if (h_att_scale)
		memcpy(att.s, h_att_scale, sizeof(att.s));
	else
		memset(att.s, 0, sizeof(att.s));
	if (d_dgram_len)
		hipLaunchKernelGGL(tx_modulate_kernel<true>, dim3((unsigned)blocks), dim3(64 * TX_WAVES), 0, stream, d_in, in_stride,
				   nullptr, d_dgram_len, att, d_tab, d_out_cf32, d_out_s16, s16_scale, out_stride, nullptr, d_info, n, sps);
	else
		hipLaunchKernelGGL(tx_modulate_kernel<false>, dim3((unsigned)blocks), dim3(64 * TX_WAVES), 0, stream, d_in, in_stride,
				   d_params, nullptr, att, d_tab, d_out_cf32, d_out_s16, s16_scale, out_stride, d_out_len, nullptr, n, sps);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// The symbol-rate values of one burst in LDS (wave-wide, lb = its staged bits): what the reference places at every sps-th
// sample of its upsampled vectors.  tx_render_kernel's form of
// tx_modulate_kernel's staging (that kernel keeps its own inline copy, so that its code object stays what it was).
__device__ static inline void tx_stage_syms(const trx_tx_desc &d, const uint8_t *lb, c32 *s0, c32 *s1, int lane,
					     const trx_tx_tables *__restrict__ tab)
{
	const int nbits = d.nbits, len = d.len;
	const c32 *rot4 = reinterpret_cast<const c32 *>(tab->rot4);
	const c32 *rot1 = reinterpret_cast<const c32 *>(tab->rot1);
	const c32 *psk8 = reinterpret_cast<const c32 *>(tab->psk8);
	const c32 *erot = reinterpret_cast<const c32 *>(tab->edge_rot);
	const c32 zero = make_float2(0.0f, 0.0f);
	for (int m = lane; m < TX_SYMS; m += 64) {
		c32 v0 = zero, v1 = zero;
		if (d.mode == TX_LAURENT) {
			// modulateBurstLaurent :615-656.  c0: padded tail (-1), the bits, padded tail (-1) at 4m, m = 0 .. nbits+1, then
			// GMSKRotate's real branch (*rotPtr * x.real(), :247-251).  c1 = c0 * (0, phase) at m = 2 .. nbits+1, phase -1 at
			// m = 2 (start magic) and 2 (b[m-2] ^ b[m-3]) - 1 after it (the loop and the end magic)
			if (m <= nbits + 1) {
				const float x = (m == 0 || m == nbits + 1) ? -1.0f : (lb[m - 1] ? 1.0f : -1.0f);   /* 2.0 * bit - 1.0 */
				const c32 r = rot4[4 * m];
				v0 = make_float2(r.x * x, r.y * x);
				if (m >= 2) {
					const float ph = (m == 2) ? -1.0f : ((lb[m - 2] ^ lb[m - 3]) ? 1.0f : -1.0f);
					v1 = cmul(v0, make_float2(0.0f, ph));
				}
			}
		} else if (d.mode == TX_BASIC1) {
			// modulateBurstBasic :938-967 at 1 SPS: +-1 at m < nbits, 0 behind, GMSKRotate's real branch over all len samples
			if (m < len) {
				const float x = m < nbits ? (lb[m] ? 1.0f : -1.0f) : 0.0f;
				const c32 r = rot1[m];
				v0 = make_float2(r.x * x, r.y * x);
			}
		} else if (d.mode == TX_EDGE4 || d.mode == TX_EDGE_ROTATE) {
			// mapEdgeSymbols :713-729 then symbol * rot (shapeEdgeBurst :750-756 one symbol late; rotateEdgeBurst :680-686)
			const int k = d.mode == TX_EDGE4 ? m - 1 : m;
			if (k >= 0 && k < nbits / 3) {
				const unsigned idx = (unsigned)lb[3 * k] | ((unsigned)lb[3 * k + 1] << 1) | ((unsigned)lb[3 * k + 2] << 2);
				v0 = cmul(psk8[idx], erot[k]);
			}
		}
		s0[m] = v0;
		s1[m] = v1;
	}
}

// Sample i of the burst described by d (0 at i >= d.len), from its symbol-rate values, then scaled as scaleVector() does
// (tx_modulate_kernel's sample lambda).
__device__ static inline c32 tx_sample(const trx_tx_desc &d, const c32 *s0, const c32 *s1, const uint8_t *lb, const tx_lds &L,
				       const c32 *rot, int sps, int i)
{
	c32 y = make_float2(0.0f, 0.0f);
	if (i >= d.len)
		return y;
	switch (d.mode) {
	case TX_LAURENT: {
		// c0_shaped + c1_shaped (:659-666): each convolution summed on its own, then added
		const c32 a = sum_sparse4<16>(s0, L.p0, i), c = sum_sparse4<8>(s1, L.p1, i);
		y = make_float2(a.x + c.x, a.y + c.y);
		break;
	}
	case TX_EDGE4:
		y = sum_sparse4<16>(s0, L.p0, i);
		break;
	case TX_BASIC1: {
		// every sample is a symbol position at 1 SPS: the plain 4-tap START_ONLY sum, x[j] = 0 outside [0, len)
		float yr = 0.0f, yi = 0.0f;
		for (int k = 0; k < 4; k++) {
			const int j = i - 3 + k;
			if (j >= 0) {
				yr += s0[j].x * L.q1[k];
				yi += s0[j].y * L.q1[k];
			}
		}
		y = make_float2(yr, yi);
		break;
	}
	case TX_ROTATE: {
		// rotateBurst :558-580: (+-1, 0) at every sps-th sample, GMSKRotate's complex branch, then the 1-tap empty pulse
		// (real taps: 0.0f + x.re * 1.0f)
		const int m = i / sps;
		const float x = (i == m * sps && m < d.nbits) ? (lb[m] ? 1.0f : -1.0f) : 0.0f;
		const c32 v = cmul(rot[i], make_float2(x, 0.0f));
		y = make_float2(0.0f + v.x * 1.0f, 0.0f + v.y * 1.0f);
		break;
	}
	default: {                             /* TX_EDGE_ROTATE: no filter, zeros between the symbols */
		const int m = i / sps;
		if (i == m * sps)
			y = s0[m];
		break;
	}
	}
	if (d.scaled)                          /* scaleVector's complex branch, :1199-1203 */
		y = make_float2(y.x * d.scale.x - y.y * d.scale.y, y.x * d.scale.y + y.y * d.scale.x);
	return y;
}

// tx_modulate_kernel's store loop: samples [0, stride) of the row that starts `off` values (2 per sample) into out_cf32 and / or out_s16, every
// lane two samples per round, 16-byte non-temporal stores for cf32 (8 bytes for int16) after a lone head sample when the row
// is only 8- (4-) byte aligned.  Either output may be NULL.
template <class F>
__device__ static inline void tx_store_row(const F &sample, float *out_cf32, int16_t *out_s16, size_t off, float s16_scale, int stride,
					    int lane)
{
	if (out_cf32) {
		float *row = out_cf32 + off;
		const int head = (reinterpret_cast<uintptr_t>(row) & 15) ? 1 : 0;     /* sample 0 alone when the row is 8-byte aligned */
		if (head && lane == 0) {
			const c32 y = sample(0);
			__builtin_nontemporal_store((f2v){y.x, y.y}, reinterpret_cast<f2v *>(row));
		}
		for (int i0 = head + 2 * lane; i0 < stride; i0 += 128) {
			const c32 y0 = sample(i0);
			if (i0 + 1 < stride) {
				const c32 y1 = sample(i0 + 1);
				__builtin_nontemporal_store((f4v){y0.x, y0.y, y1.x, y1.y}, reinterpret_cast<f4v *>(row + 2 * i0));
			} else {
				__builtin_nontemporal_store((f2v){y0.x, y0.y}, reinterpret_cast<f2v *>(row + 2 * i0));
			}
		}
	}
	if (out_s16) {
		// convert_float_short_kernel's expression (trx_aux_kernels.hip): (int16_t)(int)(x * scale)
		int16_t *row = out_s16 + off;
		auto q = [&](float v) -> unsigned { return (unsigned)(uint16_t)(int16_t)(int)(v * s16_scale); };
		const int head = (reinterpret_cast<uintptr_t>(row) & 7) ? 1 : 0;
		if (head && lane == 0) {
			const c32 y = sample(0);
			__builtin_nontemporal_store(q(y.x) | (q(y.y) << 16), reinterpret_cast<unsigned *>(row));
		}
		for (int i0 = head + 2 * lane; i0 < stride; i0 += 128) {
			const c32 y0 = sample(i0);
			if (i0 + 1 < stride) {
				const c32 y1 = sample(i0 + 1);
				__builtin_nontemporal_store((u2v){q(y0.x) | (q(y0.y) << 16), q(y1.x) | (q(y1.y) << 16)},
							    reinterpret_cast<u2v *>(row + 2 * i0));
			} else {
				__builtin_nontemporal_store(q(y0.x) | (q(y0.y) << 16), reinterpret_cast<unsigned *>(row + 2 * i0));
			}
		}
	}
}

// 1-SPS slot offsets in a frame: 157 / 156 / 156 / 156 / 157 / 156 / 156 / 156 samples (148 + 8 + (tn % 4 == 0))
__device__ static inline size_t tx_slot1_start(int tn) { return (size_t)tn * 156 + (size_t)((tn + 3) >> 2); }

// The downlink burst scheduler's render (trx_tx_sched.cpp plans, this kernel draws): one wave per (channel, slot), four per
// workgroup, wave b = chan * n_slots + s.  The wave reads its slot word, describes the source (a staged TRXD datagram row, a
// filler-table descriptor, or zeros), stages and modulates it as tx_modulate_kernel does and writes the samples straight
// into the slot's place of the channel's stream: slot s of the render starts at s * 625 (4 SPS) or at its 1-SPS offset
// counted from the render's first TN tn0.  Each output sample is written once; there are no burst rows in between.
__global__ void __launch_bounds__(64 * TX_WAVES)
tx_render_kernel(const uint32_t *__restrict__ slots, size_t n_slots, int chans, int tn0, int sps, const uint8_t *__restrict__ rows,
		 const trx_tx_fill *__restrict__ fill, tx_att_table att,
		 const trx_tx_tables *__restrict__ tab, float *__restrict__ out_cf32, int16_t *__restrict__ out_s16,
		 trx_tx_s16_scales s16, size_t out_stride)
{
	__shared__ tx_lds L;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const size_t b = (size_t)blockIdx.x * TX_WAVES + w;
	const bool active = b < n_slots * (size_t)chans;

	if (threadIdx.x < 16)
		L.p0[threadIdx.x] = tab->pulse4_c0[threadIdx.x];
	else if (threadIdx.x < 24)
		L.p1[threadIdx.x - 16] = tab->pulse4_c1[threadIdx.x - 16];
	else if (threadIdx.x < 28)
		L.q1[threadIdx.x - 24] = tab->pulse1_c0[threadIdx.x - 24];

	// ---- the slot and its source (wave-uniform) ----
	trx_tx_desc d;
	d.status = TRXHIP_EINVAL;
	d.len = 0;
	d.nbits = 0;
	d.mode = TX_LAURENT;
	d.scaled = false;
	const uint8_t *bits = nullptr;
	int chan = 0, len = 0;
	size_t off = 0;
	if (active) {
		chan = (int)(b / n_slots);
		const size_t s = b - (size_t)chan * n_slots, t = (size_t)tn0 + s;
		const int tn = (int)(t & 7);
		if (sps == 4) {
			off = s * 625;
			len = 625;
		} else {
			off = (t >> 3) * 1250 + tx_slot1_start(tn) - tx_slot1_start(tn0);
			len = 156 + (tn % 4 == 0);
		}
		const uint32_t word = slots[b], idx = word & 0x3fffffffu;
		if ((word >> 30) == TRX_TXS_ROW) {
			trxhip_tx_info info;
			const uint8_t *row = rows + (size_t)idx * TRX_TXS_ROW_STRIDE;
			const int dlen = row[TRX_TXS_ROW_STRIDE - 2] | (row[TRX_TXS_ROW_STRIDE - 1] << 8);      /* the datagram's length */
			bits = trxd_describe(row, dlen, TRX_TXS_ROW_STRIDE - 2, sps, att, (size_t)len, d, info);
		} else if ((word >> 30) == TRX_TXS_ENTRY) {
			const trx_tx_fill *f = fill + idx;
			d = tx_describe(f->nbits, f->guard, f->flags, sps, TRX_TXS_FILL_BITS, (size_t)len);
			d.scale = make_float2(f->scale_re, f->scale_im);
			d.scaled = true;                   /* scaleVector() ran on every filler burst (Transceiver.cpp:123, :396) */
			bits = f->bits;
		}
	}
	const bool ok = active && d.status == 0;

	// ---- stage the bits: only bit 0 counts (bits[i] & 0x01) ----
	uint8_t *lb = L.bits[w];
	if (ok)
		for (int i = lane; i < d.nbits; i += 64)
			lb[i] = bits[i] & 0x01;
	__syncthreads();

	c32 *s0 = L.sym0[w], *s1 = L.sym1[w];
	if (ok)
		tx_stage_syms(d, lb, s0, s1, lane, tab);
	__syncthreads();
	if (!active)
		return;

	// ---- the slot's samples: the burst, or zeros (d.len == 0: a zero slot, radioifyVector()'s zero(), radioInterface.cpp:132-141) ----
	const c32 *rot = reinterpret_cast<const c32 *>(sps == 4 ? tab->rot4 : tab->rot1);
	auto sample = [&](int i) -> c32 { return tx_sample(d, s0, s1, lb, L, rot, sps, i); };
	tx_store_row(sample, out_cf32, out_s16, 2 * ((size_t)chan * out_stride + off), s16.s[chan], len, lane);
}

// End of a render: the filler-table entries the render's bursts wrote (updateFillerTable(), Transceiver.cpp:403-414) take
// the bits of the staged row and the planner's parameters.  One wave per entry; at most one update per entry and render.
__global__ void __launch_bounds__(64)
tx_fill_update_kernel(const trx_tx_fill_update *__restrict__ upd, size_t n, const uint8_t *__restrict__ rows, trx_tx_fill *__restrict__ fill)
{
	const size_t k = blockIdx.x;
	if (k >= n)
		return;
	const trx_tx_fill_update u = upd[k];
	trx_tx_fill *f = fill + u.entry;
	const uint8_t *src = rows + (size_t)u.row * TRX_TXS_ROW_STRIDE + 6;
	for (int i = threadIdx.x; i < (int)TRX_TXS_FILL_BITS; i += 64)
		f->bits[i] = i < (int)u.nbits ? src[i] : 0;
	if (threadIdx.x == 0) {
		f->nbits = u.nbits;
		f->guard = u.guard;
		f->flags = u.flags;
		f->scale_re = u.scale_re;
		f->scale_im = 0.0f;
		f->reserved = 0;
	}
}

extern "C" int trx_launch_tx_render(const uint32_t *d_slots, size_t n_slots, int chans, int tn0, int sps, const uint8_t *d_rows,
				    const trx_tx_fill *d_fill, const float *h_att_scale, const trx_tx_tables *d_tab,
				    float *d_out_cf32, int16_t *d_out_s16, const float *h_s16_scales, size_t out_stride, hipStream_t stream)
{
	if (n_slots == 0)
		return 0;
	if (chans < 1 || chans > TRX_TXS_MAX_CHANS || tn0 < 0 || tn0 > 7)
		return TRXHIP_EINVAL;
	const size_t blocks = (n_slots * (size_t)chans + TX_WAVES - 1) / TX_WAVES;
	if (blocks > 0x7fffffffu)
		return TRXHIP_EINVAL;
	tx_att_table att;
	memcpy(att.s, h_att_scale, sizeof(att.s));
	trx_tx_s16_scales s16;
	memset(&s16, 0, sizeof(s16));
	if (h_s16_scales)
		memcpy(s16.s, h_s16_scales, (size_t)chans * sizeof(float));
	hipLaunchKernelGGL(tx_render_kernel, dim3((unsigned)blocks), dim3(64 * TX_WAVES), 0, stream, d_slots, n_slots, chans, tn0, sps,
			   d_rows, d_fill, att, d_tab, d_out_cf32, d_out_s16, s16, out_stride);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" int trx_launch_tx_fill_update(const trx_tx_fill_update *d_upd, size_t n, const uint8_t *d_rows, trx_tx_fill *d_fill,
					 hipStream_t stream)
{
	if (n == 0)
		return 0;
	if (n > 0x7fffffffu)
		return TRXHIP_EINVAL;
	hipLaunchKernelGGL(tx_fill_update_kernel, dim3((unsigned)n), dim3(64), 0, stream, d_upd, n, d_rows, d_fill);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// The MS-side uplink burst scheduler's render (trx_ms_tx.cpp plans, this kernel draws): one wave per segment, four per
// workgroup.  Uplink bursts lie at any sample offset of the window (send_ts - timing_advance + rxtxdelay) and may begin or end
// outside it, so the planner tiles the window with segments of at most 625 samples: a stretch of a staged burst, from its
// sample `first` on, or zeros.  A burst segment stages the burst's bits and symbols as tx_render_kernel does and evaluates
// tx_sample at i + first: a burst drawn in two windows gives the samples of one drawn whole.  The int16 are those of
// tx_modulate_kernel with s16_scale 1 -- driveTx()'s static_cast<int16_t>(x * 1) -- through tx_store_row: a lone head sample when
// the segment starts 4 bytes off an 8-byte boundary, 8-byte stores, a lone tail.  Every sample of the window is written once.
//
// ROT (ms_tx_render_nco_kernel): the member's uplink oscillator (trx_ms_nco.h, include/trxhip.h) between tx_sample() and the cast.
// nco = {phase of the window's first sample, inc}: sample i of a segment has phase phase0 + (out_off + i) * inc modulo 2^32, a
// function of its timestamp alone, so the tiling cannot change a bit.  The order is scale (inside tx_sample), rotate, cast.  Zero
// segments are written as zeros and read no table.  The two table reads go through the vector cache, as the receive side's do:
// the tables are 16 KB that every wave of the launch reads and that stay cache-resident, where a staged copy would move 16 KB
// into LDS per workgroup of at most 2500 samples and more than double the workgroup's LDS.
template <bool ROT>
__device__ __forceinline__ void ms_tx_render_body(const trx_mstx_seg *__restrict__ segs, size_t n_segs, const trx_mstx_row *__restrict__ rows,
						  const trx_tx_tables *__restrict__ tab, int16_t *__restrict__ out, trxhip_ms_nco_row nco,
						  const float *__restrict__ nco_tab)
{
	__shared__ tx_lds L;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const size_t b = (size_t)blockIdx.x * TX_WAVES + w;
	const bool active = b < n_segs;

	if (threadIdx.x < 16)
		L.p0[threadIdx.x] = tab->pulse4_c0[threadIdx.x];
	else if (threadIdx.x < 24)
		L.p1[threadIdx.x - 16] = tab->pulse4_c1[threadIdx.x - 16];

	// ---- the segment and its source (wave-uniform) ----
	trx_tx_desc d;
	d.status = 0;
	d.mode = TX_LAURENT;                       /* modulateBurst(bits, 8 + (tn % 4 == 0), 4), ms_upper.cpp:335 */
	d.nbits = 148;
	d.len = 0;                                 /* zeros until a burst is found */
	d.scale = make_float2(1.0f, 0.0f);
	d.scaled = true;                           /* scaleVector() runs on every burst, :336 */
	const uint8_t *bits = nullptr;
	int first = 0, len = 0;
	size_t off = 0;
	if (active) {
		const trx_mstx_seg g = segs[b];
		off = g.out_off;
		len = g.len;
		first = g.first;
		if (g.src != TRX_MSTX_ZERO) {
			const trx_mstx_row *r = rows + g.src;
			bits = r->bits;
			d.len = (int)TRX_MSTX_BURST;
			d.scale = make_float2(r->scale, 0.0f);
		}
	}
	const bool ok = bits != nullptr;

	uint8_t *lb = L.bits[w];
	if (ok)
		for (int i = lane; i < d.nbits; i += 64)
			lb[i] = bits[i] & 0x01;
	__syncthreads();

	c32 *s0 = L.sym0[w], *s1 = L.sym1[w];
	if (ok)
		tx_stage_syms(d, lb, s0, s1, lane, tab);
	__syncthreads();
	if (!active)
		return;

	const c32 *rot = reinterpret_cast<const c32 *>(tab->rot4);
	if (ROT) {
		const uint32_t p0 = nco.phase0 + (uint32_t)off * (uint32_t)nco.inc;
		auto rotated = [&](int i) -> c32 {
			const c32 x = tx_sample(d, s0, s1, lb, L, rot, 4, i + first);
			float rc, rs, yr, yi;
			trx_nco_phasor(nco_tab, p0 + (uint32_t)i * (uint32_t)nco.inc, &rc, &rs);
			trx_nco_rotate(x.x, x.y, rc, rs, &yr, &yi);
			return make_float2(yr, yi);
		};
		auto zeros = [](int) -> c32 { return make_float2(0.0f, 0.0f); };
		if (ok)
			tx_store_row(rotated, nullptr, out, 2 * off, 1.0f, len, lane);
		else
			tx_store_row(zeros, nullptr, out, 2 * off, 1.0f, len, lane);
		return;
	}
	auto sample = [&](int i) -> c32 { return tx_sample(d, s0, s1, lb, L, rot, 4, i + first); };
	tx_store_row(sample, nullptr, out, 2 * off, 1.0f, len, lane);
}

__global__ void __launch_bounds__(64 * TX_WAVES)
ms_tx_render_kernel(const trx_mstx_seg *__restrict__ segs, size_t n_segs, const trx_mstx_row *__restrict__ rows,
		    const trx_tx_tables *__restrict__ tab, int16_t *__restrict__ out)
{
	ms_tx_render_body<false>(segs, n_segs, rows, tab, out, trxhip_ms_nco_row{ 0u, 0 }, nullptr);
}

__global__ void __launch_bounds__(64 * TX_WAVES)
ms_tx_render_nco_kernel(const trx_mstx_seg *__restrict__ segs, size_t n_segs, const trx_mstx_row *__restrict__ rows,
			const trx_tx_tables *__restrict__ tab, int16_t *__restrict__ out, trxhip_ms_nco_row nco,
			const float *__restrict__ nco_tab)
{
	ms_tx_render_body<true>(segs, n_segs, rows, tab, out, nco, nco_tab);
}

extern "C" int trx_launch_ms_tx_render(const trx_mstx_seg *d_segs, size_t n_segs, const trx_mstx_row *d_rows, const trx_tx_tables *d_tab,
				       int16_t *d_out, hipStream_t stream)
{
	if (n_segs == 0)
		return 0;
	const size_t blocks = (n_segs + TX_WAVES - 1) / TX_WAVES;
	if (blocks > 0x7fffffffu)
		return TRXHIP_EINVAL;
	hipLaunchKernelGGL(ms_tx_render_kernel, dim3((unsigned)blocks), dim3(64 * TX_WAVES), 0, stream, d_segs, n_segs, d_rows, d_tab, d_out);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" int trx_launch_ms_tx_render_nco(const trx_mstx_seg *d_segs, size_t n_segs, const trx_mstx_row *d_rows, const trx_tx_tables *d_tab,
					   int16_t *d_out, trxhip_ms_nco_row nco, const float *d_nco_tab, hipStream_t stream)
{
	if (n_segs == 0)
		return 0;
	const size_t blocks = (n_segs + TX_WAVES - 1) / TX_WAVES;
	if (blocks > 0x7fffffffu || !d_nco_tab)
		return TRXHIP_EINVAL;
	hipLaunchKernelGGL(ms_tx_render_nco_kernel, dim3((unsigned)blocks), dim3(64 * TX_WAVES), 0, stream, d_segs, n_segs, d_rows, d_tab, d_out,
			   nco, d_nco_tab);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// The second burst of a tile of ms_tx_render_group_kernel: its staging areas, per wave as tx_lds's (which holds the first
// burst's and the pulse taps).
struct tx_lds_second {
	c32 sym0[TX_WAVES][TX_SYMS];
	c32 sym1[TX_WAVES][TX_SYMS];
	uint8_t bits[TX_WAVES][TX_BITS];
};

// The uplink scheduler group's render (trxhip_ms_tx_group_*; trx_ms_tx.cpp builds the table, trx_ms_tx.h describes it): one wave
// per tile of at most 625 samples of one member's window, four per workgroup.  Wave gw finds its member by bisection on
// first_wave, its tile is gw - first_wave, and it finds the bursts that have samples in the tile by a search over the member's
// sorted burst list (a bisection with 64 probes per round, one per lane): the first burst that ends behind the tile's start (A)
// and, when that one begins before the tile's end, its successor (B) if it begins in the tile too.  A member's bursts are disjoint and 625 long, so no third one meets a tile of 625.  The wave stages A in tx_lds and B in
// tx_lds_second, then writes five pieces in order, each through tx_store_row: zeros, A's stretch, zeros, B's stretch, zeros.  A
// burst piece evaluates tx_sample at i + first exactly as ms_tx_render_kernel does, so a burst drawn by two tiles, or in two
// windows, gives the samples of one drawn whole.  Every sample of every rendered window is written once, nothing else is.
// Barriers: all four waves reach both __syncthreads(), idle waves (behind n_waves) and tiles with one burst or none included; no
// wave returns before the second.
//
// ROT (ms_tx_render_group_nco_kernel): every member's uplink oscillator as in ms_tx_render_body.  The entry carries the member's
// {nco_phase0, nco_inc}, nco_phase0 the phase of its window's first sample, and sample i of a piece that begins `from` samples
// into the tile that begins t0 samples into the window has phase nco_phase0 + (t0 + from + i) * nco_inc.  A member with its
// oscillator off rides with inc 0 at phase 0: r = (1, 0) exactly, the identity on the int16.  Zero pieces read no table.
template <bool ROT>
__device__ __forceinline__ void ms_tx_render_group_body(const trx_mstx_gmember *__restrict__ tab, uint32_t n_entries, uint32_t n_waves,
							const trx_mstx_row *__restrict__ rows, const trx_tx_tables *__restrict__ ttab,
							int16_t *__restrict__ out, const float *__restrict__ nco_tab)
{
	__shared__ tx_lds L;
	__shared__ tx_lds_second L2;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t gw = blockIdx.x * TX_WAVES + w;
	const bool active = gw < n_waves;

	if (threadIdx.x < 16)
		L.p0[threadIdx.x] = ttab->pulse4_c0[threadIdx.x];
	else if (threadIdx.x < 24)
		L.p1[threadIdx.x - 16] = ttab->pulse4_c1[threadIdx.x - 16];

	// ---- the tile and its bursts (wave-uniform); positions count from the tile's first sample ----
	const trx_mstx_row *ra = nullptr, *rb = nullptr;
	size_t off = 0;
	int len = 0, a_lo = 0, a_hi = 0, a_first = 0, b_lo = 0, b_hi = 0;
	uint32_t nco_p0 = 0, nco_inc = 0;                             // ROT: the phase of the tile's first sample, the increment
	if (active) {
		unsigned lo = 0, hi = n_entries;                           // tab[lo].first_wave <= gw < tab[hi].first_wave
		while (hi - lo > 1) {
			const unsigned mid = (lo + hi) >> 1;
			if (tab[mid].first_wave <= gw)
				lo = mid;
			else
				hi = mid;
		}
		const trx_mstx_gmember e = tab[lo];
		const uint32_t t0 = (gw - e.first_wave) * TRX_MSTX_BURST;  // the tile's first sample in the window: < n_samples <= 2^31
		len = (int)min(TRX_MSTX_BURST, e.n_samples - t0);
		off = (size_t)e.out_off + t0;
		if (ROT) {
			nco_inc = (uint32_t)e.nco_inc;
			nco_p0 = e.nco_phase0 + t0 * nco_inc;
		}
		const trx_mstx_gburst *bl = reinterpret_cast<const trx_mstx_gburst *>(tab + n_entries) + e.first_burst;
		// The first burst that ends behind the tile's start, i0 in [i0, i1].  The list is sorted, so "burst i ends at or before the
		// tile's start" holds for a prefix of it.  The search is the wave's: the range is cut into 64 chunks, lane l asks about the
		// last burst of chunk l, and the number of lanes that say yes names the chunk that holds i0 -- three rounds of one load
		// for 262 144 bursts where a lane's bisection takes eighteen loads one behind the other.
		unsigned i0 = 0, i1 = e.n_bursts;
		while (i0 < i1) {
			const unsigned step = (i1 - i0 + 63) >> 6;
			const uint64_t at = (uint64_t)i0 + (uint64_t)lane * step + (step - 1);
			const bool before = at < i1 && (int64_t)bl[at].rel + (int64_t)TRX_MSTX_BURST <= (int64_t)t0;
			const unsigned whole = (unsigned)__popcll(__ballot(before));               // chunks that lie wholly before the tile
			i0 = (unsigned)min((uint64_t)i1, (uint64_t)i0 + (uint64_t)whole * step);
			i1 = (unsigned)min((uint64_t)i1, (uint64_t)i0 + step - 1);                 // that chunk's last burst said no, or lies at i1
		}
		if (i0 < e.n_bursts) {
			const trx_mstx_gburst ba = bl[i0];
			const int64_t da = (int64_t)ba.rel - (int64_t)t0;      // > -625
			if (da < len) {
				ra = rows + ba.row;
				a_lo = da > 0 ? (int)da : 0;
				a_hi = min((int)da + (int)TRX_MSTX_BURST, len);
				a_first = a_lo - (int)da;
				if (i0 + 1 < e.n_bursts) {
					const trx_mstx_gburst bb = bl[i0 + 1];
					const int64_t db = (int64_t)bb.rel - (int64_t)t0;      // >= da + 625 > 0: B begins in the tile or behind it
					if (db >= a_hi && db < len) {
						rb = rows + bb.row;
						b_lo = (int)db;
						b_hi = len;                                    // db + 625 > len
					}
				}
			}
		}
		if (!rb)
			b_lo = b_hi = a_hi;
	}

	trx_tx_desc d;
	d.status = 0;
	d.mode = TX_LAURENT;                       /* modulateBurst(bits, 8 + (tn % 4 == 0), 4), ms_upper.cpp:335 */
	d.nbits = 148;
	d.len = (int)TRX_MSTX_BURST;
	d.scale = make_float2(1.0f, 0.0f);
	d.scaled = true;                           /* scaleVector() runs on every burst, :336 */

	uint8_t *lba = L.bits[w], *lbb = L2.bits[w];
	if (ra)
		for (int i = lane; i < d.nbits; i += 64)
			lba[i] = ra->bits[i] & 0x01;
	if (rb)
		for (int i = lane; i < d.nbits; i += 64)
			lbb[i] = rb->bits[i] & 0x01;
	__syncthreads();

	if (ra)
		tx_stage_syms(d, lba, L.sym0[w], L.sym1[w], lane, ttab);
	if (rb)
		tx_stage_syms(d, lbb, L2.sym0[w], L2.sym1[w], lane, ttab);
	__syncthreads();
	if (!active)
		return;

	// ---- the five pieces: zeros [0, a_lo), A [a_lo, a_hi), zeros [a_hi, b_lo), B [b_lo, b_hi), zeros [b_hi, len) ----
	const c32 *rot = reinterpret_cast<const c32 *>(ttab->rot4);
	const float scale_a = ra ? ra->scale : 1.0f, scale_b = rb ? rb->scale : 1.0f;
	for (int p = 0; p < 5; p++) {
		const int from = p == 0 ? 0 : p == 1 ? a_lo : p == 2 ? a_hi : p == 3 ? b_lo : b_hi;
		const int to = p == 0 ? a_lo : p == 1 ? a_hi : p == 2 ? b_lo : p == 3 ? b_hi : len;
		if (to <= from)
			continue;
		const bool second = p == 3;
		trx_tx_desc dp = d;
		dp.len = (p & 1) ? (int)TRX_MSTX_BURST : 0;             /* 0: zeros */
		dp.scale = make_float2(second ? scale_b : scale_a, 0.0f);
		const c32 *s0 = second ? L2.sym0[w] : L.sym0[w], *s1 = second ? L2.sym1[w] : L.sym1[w];
		const uint8_t *lb = second ? lbb : lba;
		const int first = p == 1 ? a_first : 0;                    /* B begins in the tile: its sample 0 */
		if (ROT) {
			const uint32_t p0 = nco_p0 + (uint32_t)from * nco_inc;
			auto rotated = [&](int i) -> c32 {
				const c32 x = tx_sample(dp, s0, s1, lb, L, rot, 4, i + first);
				float rc, rs, yr, yi;
				trx_nco_phasor(nco_tab, p0 + (uint32_t)i * nco_inc, &rc, &rs);
				trx_nco_rotate(x.x, x.y, rc, rs, &yr, &yi);
				return make_float2(yr, yi);
			};
			auto zeros = [](int) -> c32 { return make_float2(0.0f, 0.0f); };
			if (p & 1)
				tx_store_row(rotated, nullptr, out, 2 * (off + (size_t)from), 1.0f, to - from, lane);
			else
				tx_store_row(zeros, nullptr, out, 2 * (off + (size_t)from), 1.0f, to - from, lane);
			continue;
		}
		auto sample = [&](int i) -> c32 { return tx_sample(dp, s0, s1, lb, L, rot, 4, i + first); };
		tx_store_row(sample, nullptr, out, 2 * (off + (size_t)from), 1.0f, to - from, lane);
	}
}

__global__ void __launch_bounds__(64 * TX_WAVES)
ms_tx_render_group_kernel(const trx_mstx_gmember *__restrict__ tab, uint32_t n_entries, uint32_t n_waves,
			  const trx_mstx_row *__restrict__ rows, const trx_tx_tables *__restrict__ ttab, int16_t *__restrict__ out)
{
	ms_tx_render_group_body<false>(tab, n_entries, n_waves, rows, ttab, out, nullptr);
}

__global__ void __launch_bounds__(64 * TX_WAVES)
ms_tx_render_group_nco_kernel(const trx_mstx_gmember *__restrict__ tab, uint32_t n_entries, uint32_t n_waves,
			      const trx_mstx_row *__restrict__ rows, const trx_tx_tables *__restrict__ ttab, int16_t *__restrict__ out,
			      const float *__restrict__ nco_tab)
{
	ms_tx_render_group_body<true>(tab, n_entries, n_waves, rows, ttab, out, nco_tab);
}

// A group submit's rows to their ring rows: row i of the call goes to rows[dst[i]], one thread per 32-bit word of a row.
__global__ void __launch_bounds__(256)
ms_tx_stage_kernel(const trx_mstx_row *__restrict__ src, const uint32_t *__restrict__ dst, size_t n, trx_mstx_row *__restrict__ rows,
		   size_t ring_rows)
{
	const int words = (int)(sizeof(trx_mstx_row) / 4);
	const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x, i = id / words;
	if (i >= n)
		return;
	const uint32_t r = dst[i];
	if (r >= ring_rows)
		return;                                /* the host names rows of the ring only */
	const int k = (int)(id - i * words);
	reinterpret_cast<uint32_t *>(rows + r)[k] = reinterpret_cast<const uint32_t *>(src + i)[k];
}

extern "C" int trx_launch_ms_tx_stage(const trx_mstx_row *d_src, const uint32_t *d_dst, size_t n, trx_mstx_row *d_rows, size_t ring_rows,
				      hipStream_t stream)
{
	if (n == 0)
		return 0;
	const size_t blocks = (n * (sizeof(trx_mstx_row) / 4) + 255) / 256;
	if (blocks > 0x7fffffffu)
		return TRXHIP_EINVAL;
	hipLaunchKernelGGL(ms_tx_stage_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_src, d_dst, n, d_rows, ring_rows);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" int trx_launch_ms_tx_render_group(const trx_mstx_gmember *d_tab, uint32_t n_entries, uint32_t n_waves, const trx_mstx_row *d_rows,
					     const trx_tx_tables *d_tab_tx, int16_t *d_out, hipStream_t stream)
{
	if (n_waves == 0)
		return 0;
	if (n_entries == 0 || n_waves > 0x7fffffffu)
		return TRXHIP_EINVAL;
	const unsigned blocks = (n_waves + TX_WAVES - 1) / TX_WAVES;
	hipLaunchKernelGGL(ms_tx_render_group_kernel, dim3(blocks), dim3(64 * TX_WAVES), 0, stream, d_tab, n_entries, n_waves, d_rows, d_tab_tx,
			   d_out);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" int trx_launch_ms_tx_render_group_nco(const trx_mstx_gmember *d_tab, uint32_t n_entries, uint32_t n_waves, const trx_mstx_row *d_rows,
						 const trx_tx_tables *d_tab_tx, int16_t *d_out, const float *d_nco_tab, hipStream_t stream)
{
	if (n_waves == 0)
		return 0;
	if (n_entries == 0 || n_waves > 0x7fffffffu || !d_nco_tab)
		return TRXHIP_EINVAL;
	const unsigned blocks = (n_waves + TX_WAVES - 1) / TX_WAVES;
	hipLaunchKernelGGL(ms_tx_render_group_nco_kernel, dim3(blocks), dim3(64 * TX_WAVES), 0, stream, d_tab, n_entries, n_waves, d_rows,
			   d_tab_tx, d_out, d_nco_tab);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// Host: the transmit tables, built as sigProcLibSetup() builds the reference's (sigProcLib.cpp:2139-2172), with each
// generator's operand order and float/double promotion points.
// ------------------------------------------------------------------------------------------------
static void tx_bits(uint8_t *dst, const char *s, size_t n)
{
	for (size_t i = 0; i < n; i++)
		dst[i] = s[i] == '1';
}

extern "C" int trx_tx_tables_generate(trx_tx_tables *t)
{
	memset(t, 0, sizeof(*t));
	t->magic = TRX_TX_TABLES_MAGIC;
	t->version = TRX_TX_TABLES_VERSION;

	// generateGSMPulse(4) :501-517 and generateC1Pulse :447-458: the Laurent pulses as tabulated doubles, stored as float
	static const double c0_4[16] = {
		0.0, 4.46348606e-03, 2.84385729e-02, 1.03184855e-01, 2.56065552e-01, 4.76375085e-01,
		7.05961177e-01, 8.71291644e-01, 9.29453645e-01, 8.71291644e-01, 7.05961177e-01,
		4.76375085e-01, 2.56065552e-01, 1.03184855e-01, 2.84385729e-02, 4.46348606e-03 };
	static const double c1_4[8] = {
		0.0, 8.16373112e-03, 2.84385729e-02, 5.64158904e-02, 7.05463553e-02, 5.64158904e-02,
		2.84385729e-02, 8.16373112e-03 };
	for (int i = 0; i < 16; i++) t->pulse4_c0[i] = (float)c0_4[i];
	for (int i = 0; i < 8; i++) t->pulse4_c1[i] = (float)c1_4[i];

	// generateGSMPulse(1) :519-533, normalised by sqrt(vectorNorm2) :535-543 (norm2 = i*i + r*r, Complex.h:113)
	{
		const int len = 4, sps = 1;
		float center = (float)(len - 1.0) / 2.0;
		float energy = 0.0f;
		for (int i = 0; i < len; i++) {
			float arg = ((float)i - center) / (float)sps;
			t->pulse1_c0[i] = 0.96 * std::exp(-1.1380 * arg * arg - 0.527 * arg * arg * arg * arg);
			energy += 0.0f * 0.0f + t->pulse1_c0[i] * t->pulse1_c0[i];
		}
		float avg = sqrtf(energy / sps);
		for (int i = 0; i < len; i++)
			t->pulse1_c0[i] /= avg;
	}

	// initGMSKRotationTables :191-216: phase accumulated in double, complex(cos(phase), sin(phase)) narrows to float
	double phase = 0.0;
	for (int i = 0; i < 625; i++) {
		t->rot4[i].re = std::cos(phase);
		t->rot4[i].im = std::sin(phase);
		phase += M_PI / 2.0 / 4.0;
	}
	phase = 0.0;
	for (int i = 0; i < 157; i++) {
		t->rot1[i].re = std::cos(phase);
		t->rot1[i].im = std::sin(phase);
		phase += M_PI / 2.0;
	}

	// psk8_table :66-75: Complex<float> from double literals
	static const double psk8[8][2] = {
		{ -0.70710678, 0.70710678 }, { 0.0, -1.0 }, { 0.0, 1.0 }, { 0.70710678, -0.70710678 },
		{ -1.0, 0.0 }, { -0.70710678, -0.70710678 }, { 0.70710678, 0.70710678 }, { 1.0, 0.0 } };
	for (int i = 0; i < 8; i++) {
		t->psk8[i].re = (float)psk8[i][0];
		t->psk8[i].im = (float)psk8[i][1];
	}

	// shapeEdgeBurst :750-756 / rotateEdgeBurst :680-686: float phase = i * 3.0f * M_PI / 8.0f (size_t i: i * 3.0f is
	// float, * M_PI double, / 8.0f double, narrowed to float), then cos / sin of that float (the float overloads)
	for (size_t i = 0; i < TRX_TX_EDGE_SYMS; i++) {
		float ph = i * 3.0f * M_PI / 8.0f;
		t->edge_rot[i].re = std::cos(ph);
		t->edge_rot[i].im = std::sin(ph);
	}

	// 3GPP TS 45.002 sections 5.2.3, 5.2.6, 5.2.7
	tx_bits(t->dummy_burst,
		"0001111101101110110000010100100111000001001000100000001111100011100010111000101110001010111010010100011001100111001111010011111000100101111101010000",
		148);
	tx_bits(t->rach_burst, "0011101001001011011111111001100110101010001111000", 49);
	static const char *const tsc[8] = {
		"00100101110000100010010111", "00101101110111100010110111", "01000011101110100100001110",
		"01000111101101000100011110", "00011010111001000001101011", "01001110101100000100111010",
		"10100111110110001010011111", "11101111000100101110111100" };
	static const char *const edge_tsc[8] = {
		"111111001111111001111001001001111111111111001111111111001111111001111001001001",
		"111111001111001001111001001001111001001001001111111111001111001001111001001001",
		"111001111111111111001001001111001001001111001111111001111111111111001001001111",
		"111001111111111001001001001111001001111001111111111001111111111001001001001111",
		"111111111001001111001111001001001111111001111111111111111001001111001111001001",
		"111001111111001001001111001111001001111111111111111001111111001001001111001111",
		"001111001111111001001001001001111001001111111111001111001111111001001001001001",
		"001001001111001001001001111111111001111111001111001001001111001001001001111111" };
	for (int k = 0; k < 8; k++) {
		tx_bits(t->tsc[k], tsc[k], 26);
		tx_bits(t->edge_tsc[k], edge_tsc[k], 78);
	}
	return 0;
}
