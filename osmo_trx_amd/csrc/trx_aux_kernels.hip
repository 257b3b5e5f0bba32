// trx_aux_kernels.hip -- the kernels either side of the burst hot path (gfx950, wave64):
//   * convert_short_float / _float_short   arch/common/convert_base.c:20-31 (radioInterface.cpp:344-348)
//   * cxvec_fft                      arch/common/fft.c:55-114
//   * convolve_real / _complex       arch/common/convolve_base.c:57-85, batched
//   * TRXD payload packing           proto_trxd.c:28-117
//   * energyDetect, the diversity selection, vectorSlicer, delayVector, scaleVector (sigProcLib.cpp), bursts by reference
// The receive front end (Channelizer, Resampler and the two fused) is trx_rx_frontend.hip.
// All are streaming, HBM-bound kernels: coalesced loads, int16->fp32 fused into the load,
// taps in LDS, sums in the reference's generic-C order (compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "trx_tables.h"
#include "../../include/trxhip.h"
#include "trx_launch.h"

typedef float2 c32;

// ------------------------------------------------------------------------------------------------
// int16 -> fp32, no scaling.  4 shorts (8 B) in, 16 B out per thread-iteration.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
convert_short_float_kernel(float *__restrict__ out, const int16_t *__restrict__ in, size_t len)
{
	const size_t nvec = len / 4;
	const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	const bool aligned = ((reinterpret_cast<uintptr_t>(in) & 7) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
	if (aligned) {
		const short4 *in4 = reinterpret_cast<const short4 *>(in);
		float4 *out4 = reinterpret_cast<float4 *>(out);
		for (size_t i = tid; i < nvec; i += stride) {
			const short4 s = in4[i];
			out4[i] = make_float4((float)s.x, (float)s.y, (float)s.z, (float)s.w);
		}
		for (size_t i = nvec * 4 + tid; i < len; i += stride)
			out[i] = (float)in[i];
	} else {
		for (size_t i = tid; i < len; i += stride)
			out[i] = (float)in[i];
	}
}

extern "C" int trx_launch_convert_short_float(float *d_out, const int16_t *d_in, size_t len, hipStream_t stream)
{
	if (len == 0)
		return 0;
	size_t blocks = (len / 4 + 255) / 256;
	if (blocks > 2048) blocks = 2048;
	if (blocks < 1) blocks = 1;
	hipLaunchKernelGGL(convert_short_float_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_out, d_in, len);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// fp32 -> int16 with scaling, the generic-C form: out[i] = (short)(in[i] * scale)  (convert_base.c:20-25: truncation
// toward zero; the SSE path of the reference rounds to nearest and saturates instead, convert_sse_3.c:29-102)
__global__ void __launch_bounds__(256)
convert_float_short_kernel(int16_t *__restrict__ out, const float *__restrict__ in, float scale, size_t len)
{
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
		out[i] = (int16_t)(int)(in[i] * scale);
}

extern "C" int trx_launch_convert_float_short(int16_t *d_out, const float *d_in, float scale, size_t len, hipStream_t stream)
{
	if (len == 0)
		return 0;
	size_t blocks = (len + 255) / 256;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(convert_float_short_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_out, d_in, scale, len);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// cxvec_fft() (arch/common/fft.c:55-114): `howmany` independent M-point DFTs laid out as the reference's
// fftwf_plan_many_dft(rank 1, n = m, howmany, in, istride, idist = 1, out, ostride, odist = 1) call does:
// transform t reads in[j * istride + t] and writes out[k * ostride + t].  One thread per transform.
// M = 4 (the only size the reference instantiates: Channelizer / Synthesis) uses exact +-1 / +-j butterflies;
// other M evaluate X[k] = sum_j x[j] w^(jk) directly with twiddles from sincospi (double) -- FFTW is absent here, so
// there is nothing to be bit-compatible with beyond the mathematical definition ("parity unpinned").
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
dft_strided_kernel(const c32 *__restrict__ in, c32 *__restrict__ out, int m, size_t howmany, size_t istride, size_t ostride,
		   int reverse)
{
	for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < howmany; t += (size_t)gridDim.x * blockDim.x) {
		if (m == 4) {
			const c32 y0 = in[t], y1 = in[istride + t], y2 = in[2 * istride + t], y3 = in[3 * istride + t];
			const c32 t1 = make_float2(y0.x + y2.x, y0.y + y2.y);
			const c32 t2 = make_float2(y0.x - y2.x, y0.y - y2.y);
			const c32 t3 = make_float2(y1.x + y3.x, y1.y + y3.y);
			const c32 t4 = make_float2(y1.x - y3.x, y1.y - y3.y);
			const c32 a = make_float2(t2.x + t4.y, t2.y - t4.x);       // t2 - j*t4
			const c32 b = make_float2(t2.x - t4.y, t2.y + t4.x);       // t2 + j*t4
			out[t] = make_float2(t1.x + t3.x, t1.y + t3.y);
			out[ostride + t] = reverse ? b : a;
			out[2 * ostride + t] = make_float2(t1.x - t3.x, t1.y - t3.y);
			out[3 * ostride + t] = reverse ? a : b;
		} else {
			for (int k = 0; k < m; k++) {
				double ar = 0.0, ai = 0.0;
				for (int j = 0; j < m; j++) {
					double sn, cs;
					sincospi(2.0 * (double)((j * k) % m) / (double)m, &sn, &cs);
					if (!reverse) sn = -sn;
					const c32 x = in[(size_t)j * istride + t];
					ar += (double)x.x * cs - (double)x.y * sn;
					ai += (double)x.x * sn + (double)x.y * cs;
				}
				out[(size_t)k * ostride + t] = make_float2((float)ar, (float)ai);
			}
		}
	}
}

extern "C" int trx_launch_dft_strided(const float *d_in, float *d_out, int m, size_t howmany, size_t istride, size_t ostride,
				      int reverse, hipStream_t stream)
{
	if (howmany == 0)
		return 0;
	size_t blocks = (howmany + 255) / 256;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(dft_strided_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const c32 *>(d_in),
			   reinterpret_cast<c32 *>(d_out), m, howmany, istride, ostride, reverse);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// batched correlation-form FIR:  y[v][i] = sum_k x[v][i + start - (H-1) + k] * h[k]
// one thread per output sample, taps staged in LDS, sequential k (generic-C order)
// ------------------------------------------------------------------------------------------------
template <bool HCPLX>
__global__ void __launch_bounds__(256)
convolve_kernel(const c32 *__restrict__ x, int x_len, const c32 *__restrict__ h, int h_len,
		c32 *__restrict__ y, int y_len, int start, int len, size_t n_vec)
{
	__shared__ c32 hs[256];
	for (int k = threadIdx.x; k < h_len; k += blockDim.x)
		hs[k] = h[k];
	__syncthreads();
	const size_t total = n_vec * (size_t)len;
	for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
		const size_t v = o / len;
		const int i = (int)(o - v * len);
		const c32 *xp = x + v * (size_t)x_len + (i + start - (h_len - 1));
		float yr = 0.0f, yi = 0.0f;
		for (int k = 0; k < h_len; k++) {
			const c32 xv = xp[k];
			const c32 t = hs[k];
			if (HCPLX) {                                  // mac_cmplx
				yr += xv.x * t.x - xv.y * t.y;
				yi += xv.x * t.y + xv.y * t.x;
			} else {                                      // mac_real: imag of the tap ignored
				yr += xv.x * t.x;
				yi += xv.y * t.x;
			}
		}
		y[v * (size_t)y_len + i] = make_float2(yr, yi);
	}
}

// The same sums with the vector's window staged in LDS (round 3): one workgroup per vector loads x[start - (H-1) ..
// start + len - 1] once, coalesced, instead of H global loads per output; taps are wave-uniform (scalar loads).
// Used when the window fits 48 KB; the form above otherwise.
template <bool HCPLX>
__global__ void __launch_bounds__(256)
convolve_lds_kernel(const c32 *__restrict__ x, int x_len, const c32 *__restrict__ h, int h_len,
		    c32 *__restrict__ y, int y_len, int start, int len)
{
	extern __shared__ __attribute__((aligned(16))) char cv_smem[];
	c32 *xs = reinterpret_cast<c32 *>(cv_smem);                          // xs[j] = x[v][start - (H-1) + j]
	const size_t v = blockIdx.x;
	const c32 *xv0 = x + v * (size_t)x_len + (start - (h_len - 1));
	const int span = len + h_len - 1;
	for (int j = threadIdx.x; j < span; j += blockDim.x)
		xs[j] = xv0[j];
	__syncthreads();
	for (int i = threadIdx.x; i < len; i += blockDim.x) {
		const c32 *xp = xs + i;
		float yr = 0.0f, yi = 0.0f;
		for (int k = 0; k < h_len; k++) {
			const c32 xv = xp[k];
			const c32 t = h[k];
			if (HCPLX) {                                  // mac_cmplx
				yr += xv.x * t.x - xv.y * t.y;
				yi += xv.x * t.y + xv.y * t.x;
			} else {                                      // mac_real: imag of the tap ignored
				yr += xv.x * t.x;
				yi += xv.y * t.x;
			}
		}
		y[v * (size_t)y_len + i] = make_float2(yr, yi);
	}
}

extern "C" int trx_launch_convolve(const float *d_x, int x_len, const float *d_h, int h_len, int h_complex,
				   float *d_y, int y_len, int start, int len, size_t n_vec, hipStream_t stream)
{
	const size_t total = n_vec * (size_t)len;
	if (total == 0)
		return 0;
	const c32 *x = reinterpret_cast<const c32 *>(d_x);
	const size_t span_bytes = ((size_t)len + h_len - 1) * sizeof(c32);
	if (span_bytes <= 48 * 1024 && n_vec <= 0x7fffffffu && len >= 64) {  // one workgroup per vector, its window in LDS
		const c32 *hh = reinterpret_cast<const c32 *>(d_h);
		c32 *yy = reinterpret_cast<c32 *>(d_y);
		if (h_complex)
			hipLaunchKernelGGL(convolve_lds_kernel<true>, dim3((unsigned)n_vec), dim3(256), span_bytes, stream, x, x_len, hh, h_len, yy,
					   y_len, start, len);
		else
			hipLaunchKernelGGL(convolve_lds_kernel<false>, dim3((unsigned)n_vec), dim3(256), span_bytes, stream, x, x_len, hh, h_len, yy,
					   y_len, start, len);
		return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
	}
	size_t blocks = (total + 255) / 256;
	if (blocks > 256 * 8) blocks = 256 * 8;
	const c32 *h = reinterpret_cast<const c32 *>(d_h);
	c32 *y = reinterpret_cast<c32 *>(d_y);
	if (h_complex)
		hipLaunchKernelGGL(convolve_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, x, x_len, h, h_len, y,
				   y_len, start, len, n_vec);
	else
		hipLaunchKernelGGL(convolve_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, x, x_len, h, h_len, y,
				   y_len, start, len, n_vec);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// TRXD payload packing (proto_trxd.c:36-66): one 156-byte record per burst, one wave per 4 bursts
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
pack_trxd_kernel(const trxhip_burst_result *__restrict__ res, const float *__restrict__ soft, int soft_stride,
		 uint8_t *__restrict__ pkt, size_t n_bursts, float rssi_offset)
{
	const size_t total = n_bursts * 39;                                  // 39 dwords per record
	uint32_t *out = reinterpret_cast<uint32_t *>(pkt);
	for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
		const size_t b = o / 39;
		const int wd = (int)(o - b * 39);
		const trxhip_burst_result r = res[b];
		uint32_t word;
		if (wd == 0) {
			const int toa_int = (int)((double)r.toa * 256.0 + 0.5);        // trxd_fill_v0_specific
			double rssi = (double)r.rssi + (double)rssi_offset;
			uint32_t rssi_u8 = (rssi >= 255.0 || rssi != rssi) ? 255u : (rssi <= 0.0 ? 0u : (uint32_t)rssi);
			const int ci_cb = (int16_t)((double)(r.ci * 10) + 0.5);        // trxd_fill_v1_specific
			word = ((uint32_t)(toa_int >> 8) & 0xffu) | (((uint32_t)toa_int & 0xffu) << 8) | (rssi_u8 << 16) |
			       ((((uint32_t)ci_cb >> 8) & 0xffu) << 24);
		} else if (wd == 1) {
			const int ci_cb = (int16_t)((double)(r.ci * 10) + 0.5);
			word = ((uint32_t)ci_cb & 0xffu) | ((uint32_t)r.tsc << 8) | ((uint32_t)r.idle << 16) |
			       ((uint32_t)r.nbits_div4 << 24);
		} else {
			word = 0;
			const float *s = soft + b * (size_t)soft_stride + (wd - 2) * 4;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const uint32_t u = r.idle ? 0u : (uint32_t)(uint8_t)round((double)s[k] * 255.0);   // normalized255
				word |= u << (8 * k);
			}
		}
		out[o] = word;
	}
}

extern "C" int trx_launch_pack_trxd(const trxhip_burst_result *d_results, const float *d_soft, int soft_stride,
				    uint8_t *d_pkt, size_t n_bursts, float rssi_offset, hipStream_t stream)
{
	if (n_bursts == 0)
		return 0;
	size_t blocks = (n_bursts * 39 + 255) / 256;
	if (blocks > 256 * 8) blocks = 256 * 8;
	hipLaunchKernelGGL(pack_trxd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_results, d_soft, soft_stride,
			   d_pkt, n_bursts, rssi_offset);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// TRXD v0 / v1 uplink burst indications in wire format (proto_trxd.c:28-117, proto_trxd.h:56-106): the datagram of
// burst b at pkt + b * pkt_stride, its length in pkt_len[b].  One thread per output dword (coalesced stores); each
// thread rebuilds the few header fields it needs from the 32-byte result record (L1/L2 hits) -- the kernel moves
// 32 + 592 B in and <= 160 B out per burst and is a small fraction of the detect/demod launch in front of it.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t trxd_byte(int p, int hdr_len, int nbits, bool v1, const uint8_t *hdr, const float *s)
{
	if (p < hdr_len)
		return hdr[p];
	const int k = p - hdr_len;
	if (k < nbits)
		return (uint32_t)(uint8_t)round((double)s[k] * 255.0);      // trxd_fill_burst_normalized255(), :62-66
	return 0u;                                                           // v0's two trailing bytes (:83-87), padding
}

__global__ void __launch_bounds__(256)
pack_trxd_wire_kernel(const trxhip_burst_result *__restrict__ res, const trxhip_burst_params *__restrict__ prm,
		      const float *__restrict__ soft, int soft_stride, const trxhip_trxd_meta *__restrict__ meta,
		      uint8_t *__restrict__ pkt, int pkt_stride, uint16_t *__restrict__ pkt_len, size_t n_bursts, float rssi_offset,
		      trxhip_burst_result *__restrict__ res_copy)
{
	const int wpb = pkt_stride >> 2;                                     // dwords per burst
	const size_t total = n_bursts * (size_t)wpb;
	uint32_t *out = reinterpret_cast<uint32_t *>(pkt);
	for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
		const size_t b = o / wpb;
		const int wd = (int)(o - b * wpb);
		const trxhip_burst_result r = res[b];
		const trxhip_trxd_meta m = meta[b];
		const bool v1 = m.version != 0;
		const bool off = prm[b].type == TRXHIP_OFF;                      // -ENOENT: nothing is sent (Transceiver.cpp:704-707)
		const bool idle = r.idle != 0;
		int nbits = idle ? 0 : 4 * (int)r.nbits_div4;
		const int hdr_len = v1 ? TRXHIP_TRXD_V1_HDR : TRXHIP_TRXD_V0_HDR;
		int len = v1 ? hdr_len + nbits : hdr_len + nbits + 2;            // :76, :96-99
		if (off || (!v1 && idle))                                        // v0 drops idle indications (:71-73)
			len = 0;
		if (len > pkt_stride) {
			len = pkt_stride;
			nbits = nbits < pkt_stride - hdr_len ? nbits : pkt_stride - hdr_len;
		}
		if (nbits > soft_stride) nbits = soft_stride;

		uint8_t hdr[TRXHIP_TRXD_V1_HDR];
		hdr[0] = (uint8_t)(((v1 ? 1u : 0u) << 4) | (m.tn & 7u));         // trxd_fill_common(): version:4 | reserved:1 | tn:3
		hdr[1] = (uint8_t)(m.fn >> 24); hdr[2] = (uint8_t)(m.fn >> 16); hdr[3] = (uint8_t)(m.fn >> 8); hdr[4] = (uint8_t)m.fn;
		const double rssi = (double)r.rssi + (double)rssi_offset;        // bi->rssi (Transceiver.cpp:751)
		hdr[5] = (rssi >= 255.0) ? 255u : (rssi > 0.0 ? (uint8_t)rssi : 0u);   // v0->rssi = bi->rssi (NaN -> 0)
		const int toa_int = idle ? 0 : (int)((double)r.toa * 256.0 + 0.5);     // trxd_fill_v0_specific(), :36-45
		hdr[6] = (uint8_t)((uint32_t)toa_int >> 8); hdr[7] = (uint8_t)toa_int;
		const bool psk = !idle && r.nbits_div4 == 111;                   // bi->modulation (Transceiver.cpp:794-800)
		const uint32_t mod = psk ? (4u | (m.tss & 1u)) : (m.tss & 3u);   // TRXD_MODULATION_8PSK / _GMSK
		hdr[8] = (uint8_t)(((idle ? 1u : 0u) << 7) | (mod << 3) | (idle ? 0u : (r.tsc & 7u)));   // tsc:3 | modulation:4 | idle:1
		const int ci_cb = idle ? 0 : (int16_t)((double)(r.ci * 10) + 0.5);    // trxd_fill_v1_specific(), :47-60
		hdr[9] = (uint8_t)((uint32_t)ci_cb >> 8); hdr[10] = (uint8_t)ci_cb;

		const float *s = soft + b * (size_t)soft_stride;
		uint32_t word = 0;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const int p = 4 * wd + k;
			if (p < len)
				word |= trxd_byte(p, hdr_len, nbits, v1, hdr, s) << (8 * k);
		}
		out[o] = word;
		if (wd == 0) {
			pkt_len[b] = (uint16_t)len;
			if (res_copy)                                                // (host pipe: the record goes out with the datagram)
				res_copy[b] = r;
		}
	}
}

// Round 3: 16 datagram bytes per thread for rows that are a multiple of 16 bytes (the 160-byte rows of the host pipe).
// The per-burst fields (result record, meta word, type) are fetched by 10 threads per burst instead of 40, a thread behind
// the header and in front of the row's end reads its sixteen soft bits as four 4-byte-aligned 16-byte loads and quantises
// them with one round-to-nearest-even each (x in [0, 1]: x * 255 is exact in double and its only tie, 127.5 at x = 0.5,
// goes to 128 under round() and under rint() alike; anything outside [0, 1] takes the generic expression), and writes one
// 16-byte store.  Header and tail threads take the byte-by-byte form above.  (One WAVE per burst was tried and measured
// 0.65 ms against 0.41: the per-burst loads become exposed latency; a thread per dword with the header skipped: 0.48.)
__device__ __forceinline__ uint32_t trxd_q255(float x)
{
	return (x >= 0.0f && x <= 1.0f) ? (uint32_t)__builtin_rint((double)x * 255.0) : (uint32_t)(uint8_t)round((double)x * 255.0);
}

__global__ void __launch_bounds__(256)
pack_trxd_wire16_kernel(const trxhip_burst_result *__restrict__ res, const trxhip_burst_params *__restrict__ prm,
			const float *__restrict__ soft, int soft_stride, const trxhip_trxd_meta *__restrict__ meta,
			uint8_t *__restrict__ pkt, int pkt_stride, uint16_t *__restrict__ pkt_len, unsigned n_bursts, float rssi_offset,
			trxhip_burst_result *__restrict__ res_copy)
{
	const unsigned cpb = (unsigned)pkt_stride >> 4;                      // 16-byte chunks per burst
	const unsigned total = n_bursts * cpb;                               // (the launcher keeps this below 2^32)
	uint4 *out = reinterpret_cast<uint4 *>(pkt);
	for (unsigned o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gridDim.x * blockDim.x) {
		const unsigned b = o / cpb;
		const int p0 = 16 * (int)(o - b * cpb);                          // first datagram byte of this thread
		const uint32_t rlast = reinterpret_cast<const uint32_t *>(res + b)[7];   // tsc | clip << 8 | idle << 16 | nbits / 4 << 24
		const trxhip_trxd_meta m = meta[b];
		const bool v1 = m.version != 0;
		const bool off = prm[b].type == TRXHIP_OFF;                      // -ENOENT: nothing is sent (Transceiver.cpp:704-707)
		const bool idle = ((rlast >> 16) & 0xffu) != 0;
		int nbits = idle ? 0 : 4 * (int)(rlast >> 24);
		const int hdr_len = v1 ? TRXHIP_TRXD_V1_HDR : TRXHIP_TRXD_V0_HDR;
		int len = v1 ? hdr_len + nbits : hdr_len + nbits + 2;            // :76, :96-99
		if (off || (!v1 && idle))                                        // v0 drops idle indications (:71-73)
			len = 0;
		if (len > pkt_stride) {
			len = pkt_stride;
			nbits = nbits < pkt_stride - hdr_len ? nbits : pkt_stride - hdr_len;
		}
		if (nbits > soft_stride) nbits = soft_stride;
		const float *s = soft + b * (size_t)soft_stride;
		const int q0 = p0 - hdr_len;                                     // first soft bit of this thread
		uint32_t w[4] = {0u, 0u, 0u, 0u};
		if (q0 >= 0 && q0 + 16 <= nbits && p0 + 16 <= len) {             // sixteen soft bits, nothing else
#pragma unroll
			for (int j = 0; j < 4; j++) {
				float4 v;
				__builtin_memcpy(&v, s + q0 + 4 * j, sizeof(v));         // 4-byte aligned: one global_load_dwordx4
				w[j] = trxd_q255(v.x) | (trxd_q255(v.y) << 8) | (trxd_q255(v.z) << 16) | (trxd_q255(v.w) << 24);
			}
		} else if (p0 < len) {
			uint8_t hdr[TRXHIP_TRXD_V1_HDR];
#pragma unroll
			for (int k = 0; k < TRXHIP_TRXD_V1_HDR; k++) hdr[k] = 0;
			if (p0 == 0) {                                               // the header lives in the first chunk (hdr_len <= 11)
				const trxhip_burst_result r = res[b];
				if (res_copy)                                                // (host pipe: the record goes out with the datagram)
					res_copy[b] = r;
				hdr[0] = (uint8_t)(((v1 ? 1u : 0u) << 4) | (m.tn & 7u));     // trxd_fill_common(): version:4 | reserved:1 | tn:3
				hdr[1] = (uint8_t)(m.fn >> 24); hdr[2] = (uint8_t)(m.fn >> 16); hdr[3] = (uint8_t)(m.fn >> 8); hdr[4] = (uint8_t)m.fn;
				const double rssi = (double)r.rssi + (double)rssi_offset;    // bi->rssi (Transceiver.cpp:751)
				hdr[5] = (rssi >= 255.0) ? 255u : (rssi > 0.0 ? (uint8_t)rssi : 0u);   // v0->rssi = bi->rssi (NaN -> 0)
				const int toa_int = idle ? 0 : (int)((double)r.toa * 256.0 + 0.5);     // trxd_fill_v0_specific(), :36-45
				hdr[6] = (uint8_t)((uint32_t)toa_int >> 8); hdr[7] = (uint8_t)toa_int;
				const bool psk = !idle && r.nbits_div4 == 111;               // bi->modulation (Transceiver.cpp:794-800)
				const uint32_t mod = psk ? (4u | (m.tss & 1u)) : (m.tss & 3u);   // TRXD_MODULATION_8PSK / _GMSK
				hdr[8] = (uint8_t)(((idle ? 1u : 0u) << 7) | (mod << 3) | (idle ? 0u : (r.tsc & 7u)));   // tsc:3 | modulation:4 | idle:1
				const int ci_cb = idle ? 0 : (int16_t)((double)(r.ci * 10) + 0.5);    // trxd_fill_v1_specific(), :47-60
				hdr[9] = (uint8_t)((uint32_t)ci_cb >> 8); hdr[10] = (uint8_t)ci_cb;
			}
#pragma unroll
			for (int k = 0; k < 16; k++) {
				const int p = p0 + k;
				if (p < len)
					w[k >> 2] |= trxd_byte(p, hdr_len, nbits, v1, hdr, s) << (8 * (k & 3));
			}
		}
		out[o] = make_uint4(w[0], w[1], w[2], w[3]);
		if (p0 == 0) {
			pkt_len[b] = (uint16_t)len;
			if (res_copy && !(p0 < len))                                 // (nothing to send: the header branch did not run)
				res_copy[b] = res[b];
		}
	}
}

extern "C" int trx_launch_pack_trxd_wire(const trxhip_burst_result *d_results, const trxhip_burst_params *d_params,
					 const float *d_soft, int soft_stride, const trxhip_trxd_meta *d_meta, uint8_t *d_pkt,
					 int pkt_stride, uint16_t *d_pkt_len, size_t n_bursts, float rssi_offset, hipStream_t stream,
					 trxhip_burst_result *d_results_copy)
{
	if (n_bursts == 0)
		return 0;
	if ((pkt_stride & 15) == 0 && n_bursts * (size_t)(pkt_stride >> 4) < 0xffffff00ull && ((uintptr_t)d_pkt & 15) == 0) {
		size_t blocks16 = (n_bursts * (size_t)(pkt_stride >> 4) + 255) / 256;
		if (blocks16 > 256 * 16) blocks16 = 256 * 16;
		hipLaunchKernelGGL(pack_trxd_wire16_kernel, dim3((unsigned)blocks16), dim3(256), 0, stream, d_results, d_params, d_soft,
				   soft_stride, d_meta, d_pkt, pkt_stride, d_pkt_len, (unsigned)n_bursts, rssi_offset, d_results_copy);
		return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
	}
	size_t blocks = (n_bursts * (size_t)(pkt_stride >> 2) + 255) / 256;
	if (blocks > 256 * 8) blocks = 256 * 8;
	hipLaunchKernelGGL(pack_trxd_wire_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_results, d_params, d_soft,
			   soft_stride, d_meta, d_pkt, pkt_stride, d_pkt_len, n_bursts, rssi_offset, d_results_copy);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// energyDetect() as a stand-alone call (sigProcLib.cpp:1573-1585): one wave per burst, mean |x|^2 over
// `window` samples taken at stride 4 from sample 0 (window clamped to the burst length as the reference does)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
energy_detect_kernel(const c32 *__restrict__ x, size_t n_bursts, int burst_len, unsigned window, float *__restrict__ out)
{
	const int lane = threadIdx.x & 63;
	const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
	const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
	if (window > (unsigned)burst_len) window = burst_len;
	for (size_t b = wave; b < n_bursts; b += nwaves) {
		float e = 0.0f;
		for (unsigned i = lane; i < window; i += 64) {
			const c32 v = x[b * (size_t)burst_len + 4 * (size_t)i];
			e += v.y * v.y + v.x * v.x;
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
			e += __shfl_xor(e, o, 64);
		if (lane == 0)
			out[b] = window ? e / (float)window : 0.0f;
	}
}

extern "C" int trx_launch_energy_detect(const float *d_x, size_t n_bursts, int burst_len, unsigned window, float *d_out,
					hipStream_t stream)
{
	if (n_bursts == 0)
		return 0;
	size_t blocks = (n_bursts + 3) / 4;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(energy_detect_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
			   reinterpret_cast<const c32 *>(d_x), n_bursts, burst_len, window, d_out);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// Diversity-path selection of pullRadioVector() (Transceiver.cpp:723-741): a burst arrives on n_paths receive paths;
//   for each path i: pow = energyDetect(path i, 20 * sps); the FIRST path with the highest energy is demodulated
//   ("if (pow > max)" from max = -1, path order); avg += pow;  avg = sqrt(avg / chans) feeds rssi and the noise average.
// The selection is a decision, so each path's energy is the reference's serial sum (:1573-1585: energy += norm2 in
// sample order, one division) evaluated by one lane per path; then the whole wave copies the chosen path into the compact
// [n][burst_len] array the detector reads.  One wave per burst.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
diversity_select_kernel(const uint32_t *__restrict__ iq_paths, size_t n_bursts, int n_paths, int burst_len, unsigned window,
			uint32_t *__restrict__ iq_sel, float *__restrict__ avg_energy, uint8_t *__restrict__ path_out)
{
	const int lane = threadIdx.x & 63;
	const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
	const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
	if (window > (unsigned)burst_len) window = burst_len;
	for (size_t b = wave; b < n_bursts; b += nwaves) {
		const uint32_t *src = iq_paths + b * (size_t)n_paths * burst_len;
		float pow = 0.0f;
		if (lane < n_paths) {
			const uint32_t *x = src + (size_t)lane * burst_len;
			float e = 0.0f;
			for (unsigned i = 0; i < window; i++) {
				const uint32_t w = x[4 * (size_t)i];
				const float re = (float)(int16_t)(w & 0xffffu), im = (float)(int16_t)(w >> 16);
				e += im * im + re * re;                                 /* Complex.h:113 norm2(): i*i + r*r */
			}
			pow = window ? e / (float)window : 0.0f;
		}
		float mx = -1.0f, avg = 0.0f;
		int sel = -1;
		for (int i = 0; i < n_paths; i++) {                                 /* wave-uniform: readlane per path */
			const float pi = __shfl(pow, i, 64);
			if (pi > mx) { mx = pi; sel = i; }
			avg += pi;
		}
		if (sel < 0) sel = 0;                                                   /* (cannot happen for finite input: pow >= 0 > -1) */
		const uint32_t *from = src + (size_t)sel * burst_len;
		uint32_t *to = iq_sel + b * (size_t)burst_len;
		for (int i = lane; i < burst_len; i += 64)
			to[i] = from[i];
		if (lane == 0) {
			avg_energy[b] = avg / (float)n_paths;                           /* avg^2 of Transceiver.cpp:741 */
			if (path_out) path_out[b] = (uint8_t)sel;
		}
	}
}

// result records of a detect/demod launch over the selected paths: energy and rssi from the path average
// (Transceiver.cpp:741,751: avg = sqrt(sum pow / chans); rssi = 20 log10(rxFullScale / avg)); OFF slots keep their zeros
__global__ void __launch_bounds__(256)
diversity_power_kernel(trxhip_burst_result *__restrict__ res, const trxhip_burst_params *__restrict__ params,
		       const float *__restrict__ avg_energy, size_t n_bursts, float full_scale)
{
	for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n_bursts; b += (size_t)gridDim.x * blockDim.x) {
		if (params[b].type == TRXHIP_OFF)
			continue;
		const float e = avg_energy[b];
		res[b].energy = e;
		res[b].rssi = 6.02059991f * __log2f(full_scale * __builtin_amdgcn_rsqf(e));   // as rssi_db() (trx_device.h)
	}
}

extern "C" int trx_launch_diversity_select(const int16_t *d_iq_paths, size_t n_bursts, int n_paths, int burst_len, int sps,
					   int16_t *d_iq_sel, float *d_avg_energy, uint8_t *d_path, hipStream_t stream)
{
	if (n_bursts == 0)
		return 0;
	size_t blocks = (n_bursts + 3) / 4;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(diversity_select_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
			   reinterpret_cast<const uint32_t *>(d_iq_paths), n_bursts, n_paths, burst_len, (unsigned)(20 * sps),
			   reinterpret_cast<uint32_t *>(d_iq_sel), d_avg_energy, d_path);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" int trx_launch_diversity_power(trxhip_burst_result *d_res, const trxhip_burst_params *d_params, const float *d_avg_energy,
					  size_t n_bursts, float full_scale, hipStream_t stream)
{
	if (n_bursts == 0)
		return 0;
	size_t blocks = (n_bursts + 255) / 256;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(diversity_power_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_res, d_params, d_avg_energy,
			   n_bursts, full_scale);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// vectorSlicer() (sigProcLib.cpp:546-556): dest = clamp(0.5 * (src + 1), 0, 1)
__global__ void __launch_bounds__(256)
vector_slicer_kernel(float *__restrict__ dst, const float *__restrict__ src, size_t len)
{
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
		dst[i] = __builtin_amdgcn_fmed3f(0.5f * (src[i] + 1.0f), 0.0f, 1.0f);
}

extern "C" int trx_launch_vector_slicer(float *d_dst, const float *d_src, size_t len, hipStream_t stream)
{
	if (len == 0)
		return 0;
	size_t blocks = (len + 255) / 256;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(vector_slicer_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_dst, d_src, len);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// delayVector() (sigProcLib.cpp:1046-1098) for a batch of equally long vectors, one delay per vector:
//   whole = floor(d), frac = d - whole; |frac| > 0.01: fshift[m] = sum_k X(m - 9 + k) * h_f[k], f = floorf(frac * 64),
//   20 real taps (convolve NO_DELAY, zero-padded :318-323), else fshift = x; out[i] = fshift[i - whole], 0 outside.
// One workgroup per vector: the vector is staged once in LDS between two zero pads (round 3: every output used to fetch its
// 20 samples from global memory -- 20 vector-memory instructions per output, 0.47 ms per 65536 x 625 samples), outputs are
// then computed from consecutive LDS entries (conflict-free) and stored coalesced; taps are wave-uniform (scalar loads), sums
// in tap order.  Vectors too long for the LDS take the direct form.
#define DV_PAD 10                                                       // X(m - 9 + k), k = 0..19: 9 before, 10 behind
__global__ void __launch_bounds__(256)
delay_vector_kernel(const c32 *__restrict__ in, c32 *__restrict__ out, const float *__restrict__ delays,
		    const trx_tables *__restrict__ tab, int len)
{
	extern __shared__ __attribute__((aligned(16))) char dv_smem[];
	c32 *xs = reinterpret_cast<c32 *>(dv_smem);                          // xs[DV_PAD + j] = x[j], zeros either side
	const size_t v = blockIdx.x;
	const c32 *x = in + v * (size_t)len;
	c32 *y = out + v * (size_t)len;
	const float delay = delays[v];
	const float fl = floorf(delay);
	const int whole = (int)fl;
	const float frac = delay - (float)whole;
	const bool use_filt = (double)fabsf(frac) > 1e-2;                  // :1056
	const int fidx = use_filt ? (int)floorf(frac * (float)TRX_DELAY_FILTS) : 0;
	const float *h = tab->delay_filt[fidx];
	for (int j = threadIdx.x; j < len + 2 * DV_PAD; j += blockDim.x) {
		const int jj = j - DV_PAD;
		xs[j] = (jj >= 0 && jj < len) ? x[jj] : make_float2(0.0f, 0.0f);
	}
	__syncthreads();
	for (int i = threadIdx.x; i < len; i += blockDim.x) {
		const int m = i - whole;
		c32 r = make_float2(0.0f, 0.0f);
		if (m >= 0 && m < len) {
			if (use_filt) {
				const c32 *xp = xs + (m - 9 + DV_PAD);
				float yr = 0.0f, yi = 0.0f;
#pragma unroll
				for (int k = 0; k < TRX_DELAY_HLEN; k++) {
					const c32 xv = xp[k];
					yr += xv.x * h[k];
					yi += xv.y * h[k];
				}
				r = make_float2(yr, yi);
			} else {
				r = xs[m + DV_PAD];
			}
		}
		y[i] = r;
	}
}

// the direct form (any length): one thread per output, samples from global memory
__global__ void __launch_bounds__(256)
delay_vector_long_kernel(const c32 *__restrict__ in, c32 *__restrict__ out, const float *__restrict__ delays,
			 const trx_tables *__restrict__ tab, int len)
{
	const size_t v = blockIdx.y;
	const c32 *x = in + v * (size_t)len;
	c32 *y = out + v * (size_t)len;
	const float delay = delays[v];
	const float fl = floorf(delay);
	const int whole = (int)fl;
	const float frac = delay - (float)whole;
	const bool use_filt = (double)fabsf(frac) > 1e-2;                  // :1056
	const int fidx = use_filt ? (int)floorf(frac * (float)TRX_DELAY_FILTS) : 0;
	const float *h = tab->delay_filt[fidx];
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) {
		const int m = i - whole;
		c32 r = make_float2(0.0f, 0.0f);
		if (m >= 0 && m < len) {
			if (use_filt) {
				float yr = 0.0f, yi = 0.0f;
#pragma unroll
				for (int k = 0; k < TRX_DELAY_HLEN; k++) {
					const int j = m - 9 + k;
					const c32 xv = (j >= 0 && j < len) ? x[j] : make_float2(0.0f, 0.0f);
					yr += xv.x * h[k];
					yi += xv.y * h[k];
				}
				r = make_float2(yr, yi);
			} else {
				r = x[m];
			}
		}
		y[i] = r;
	}
}

extern "C" int trx_launch_delay_vector(const float *d_in, float *d_out, const float *d_delays, const trx_tables *d_tab,
				       size_t n_vec, int len, hipStream_t stream)
{
	if (n_vec == 0 || len == 0)
		return 0;
	if (len <= 4096 && n_vec <= 0x7fffffffu) {                         // one workgroup per vector, the vector in LDS (<= 32 KB)
		const size_t lds = (size_t)(len + 2 * DV_PAD) * sizeof(c32);
		hipLaunchKernelGGL(delay_vector_kernel, dim3((unsigned)n_vec), dim3(256), lds, stream, reinterpret_cast<const c32 *>(d_in),
				   reinterpret_cast<c32 *>(d_out), d_delays, d_tab, len);
		return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
	}
	unsigned bx = (unsigned)((len + 255) / 256);
	if (bx > 64) bx = 64;
	for (size_t v0 = 0; v0 < n_vec; v0 += 65535) {                     // gridDim.y limit
		const size_t nv = (n_vec - v0 < 65535) ? n_vec - v0 : 65535;
		hipLaunchKernelGGL(delay_vector_long_kernel, dim3(bx, (unsigned)nv), dim3(256), 0, stream,
				   reinterpret_cast<const c32 *>(d_in) + v0 * (size_t)len,
				   reinterpret_cast<c32 *>(d_out) + v0 * (size_t)len, d_delays + v0, d_tab, len);
	}
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// scaleVector() (sigProcLib.cpp:1188-1213): x[i] = x[i] * scale, Complex.h:74 operand order; in place
__global__ void __launch_bounds__(256)
scale_vector_kernel(c32 *__restrict__ x, size_t len, c32 scale)
{
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
	{
		const c32 a = x[i];
		x[i] = make_float2(a.x * scale.x - a.y * scale.y, a.x * scale.y + a.y * scale.x);
	}
}

extern "C" int trx_launch_scale_vector(float *d_x, size_t len, float sr, float si, hipStream_t stream)
{
	if (len == 0)
		return 0;
	size_t blocks = (len + 255) / 256;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(scale_vector_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<c32 *>(d_x), len,
			   make_float2(sr, si));
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}


// ---- bursts by reference (trxhip_hostpipe_submit_by_ref): fetch n bursts through n pointers into one dense block ----
// src[b] is the device-side address of burst b in host memory that was pinned and mapped (hipHostRegister): the loads cross
// the link.  One wave per burst, `dwords` 4-byte words each (625 at 4 SPS: ten rounds of 256 contiguous bytes); five loads of a
// lane are issued before the first store so that a wave keeps 1.25 KB in flight -- 256 CUs x 8 waves hold 2.6 MB on the link,
// an order of magnitude above its bandwidth-delay product.  Plain loads: with the non-temporal hint the same kernel fetched
// 37.7 GB/s instead of 44.7, 16-byte loads from the aligned body of every burst 41.4 / 42.8 (with / without the hint;
// profiles/r05_gather.txt; the copy engine
// moves the staged form of the same batch at 55 GB/s -- a cache line per request against the engine's long bursts).
// Nothing of this data is read twice: HBM sees one write.
__global__ void __launch_bounds__(256)
gather_bursts_kernel(const unsigned long long *__restrict__ src, uint32_t *__restrict__ dst, size_t n, unsigned dwords)
{
	const unsigned lane = threadIdx.x & 63u;
	const size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (b >= n)
		return;
	const unsigned long long a = src[b];                                   // wave-uniform: a scalar base, 32-bit lane offsets
	if (a == 0ull)                                                         // this burst came with a run the copy engine moved
		return;
	const unsigned a_lo = __builtin_amdgcn_readfirstlane((unsigned)a), a_hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
	const uint32_t *__restrict__ s = reinterpret_cast<const uint32_t *>(((unsigned long long)a_hi << 32) | a_lo);
	uint32_t *__restrict__ d = dst + b * dwords;
	unsigned i = lane;
	for (; i + 4u * 64u < dwords; i += 5u * 64u) {
		uint32_t v[5];
#pragma unroll
		for (int k = 0; k < 5; k++)
			v[k] = s[i + 64u * k];
#pragma unroll
		for (int k = 0; k < 5; k++)
			d[i + 64u * k] = v[k];
	}
	for (; i < dwords; i += 64u)
		d[i] = s[i];
}

extern "C" int trx_launch_gather_bursts(const unsigned long long *d_src, void *d_dst, size_t n, unsigned dwords, hipStream_t stream)
{
	if (n == 0)
		return 0;
	hipLaunchKernelGGL(gather_bursts_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, d_src, reinterpret_cast<uint32_t *>(d_dst), n, dwords);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
