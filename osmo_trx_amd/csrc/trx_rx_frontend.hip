// trx_rx_frontend.hip -- the receive front end (gfx950, wave64):
//   * channelize_kernel                Channelizer::rotate, Channelizer.cpp:74-99 (M = 4 polyphase bank + 4-point DFT)
//   * resample_kernel                  Resampler::rotate, Resampler.cpp:131-150 (65/48, 1/4, 65/96, 52/75)
//   * frontend_fused_kernel<NACT>      RadioInterfaceMulti::pullBuffer (radioInterfaceMulti.cpp:237-314): the two above in one
//                                      pass; NACT = 4: the four filterbank paths in physical order, NACT = 1..3: the active
//                                      paths of 1..3 ARFCNs only, rows handed over by logical channel
//   * rx_resamp_s16_kernel             RadioInterfaceResamp::pullBuffer (radioInterfaceResamp.cpp:156-193): convert_short_float +
//                                      Resampler(p, q, 16)::rotate of one int16 channel in one pass
// Streaming, HBM-bound kernels: coalesced loads, int16->fp32 fused into the load, taps in LDS, sums in the reference's
// generic-C order, product then add (compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trx_tables.h"
#include "../../include/trxhip.h"
#include "trx_launch.h"

typedef float2 c32;

// ------------------------------------------------------------------------------------------------
// Channelizer(4, blockLen, 16)::rotate over a continuous wideband int16 stream.
//   path p takes wideband samples (M-1-p), (M-1-p)+M, ...                 (deinterleave, :37-48)
//   y_p[T] = sum_k xp[T-15+k] * sub_p[k]   with the previous block as history   (:86-94)
//   X_c[T] = 4-point forward DFT over p of y_p[T]                          (cxvec_fft, :96)
// Block boundaries of the reference are invisible in the maths (history carry == continuous stream,
// zero history before the first sample).  A workgroup takes CH_TILE consecutive output times; a thread computes
// CH_J = 4 consecutive ones for all 4 channels, so that the 16-tap windows of its outputs share their samples: 19 LDS
// reads per path for 4 outputs instead of 64 (the one-output-per-thread version of round 1 was bound by LDS
// bandwidth, not by HBM).  The staged samples are kept per path in a 4-phase layout -- xs[p][t & 3][t >> 2] -- so
// that lane l's sample t = 4 l + v sits at entry l + (v >> 2) of phase v & 3: consecutive lanes read consecutive
// 8-byte entries (bank-conflict-free) although each lane advances by 4 samples.  Sums run k = 0..15 per output,
// product then add, as convolve_base.c:41-54 does.
// ------------------------------------------------------------------------------------------------
#define CH_M 4
#define CH_H 16
#define CH_TPB 256
#define CH_J 4
#define CH_TILE (CH_TPB * CH_J)
#define CH_PHA 264                     // entries per phase array: >= (CH_TILE + 15 + 3) / 4 = 260; 2 * 264 = 16 (mod 64) dwords, so
                                       // the four phases of one loader pass fall on disjoint bank groups

typedef float ch_v2f __attribute__((ext_vector_type(2)));
template <int HI>
__device__ __forceinline__ ch_v2f ch_mul_tap(ch_v2f x, ch_v2f hpair)
{
	ch_v2f r;                          // x * (tap HI of the pair): one v_pk_mul_f32, the tap picked by op_sel
	if (HI)
		asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(x), "v"(hpair));
	else
		asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(x), "v"(hpair));
	return r;
}

// one complex sample from LDS as its own ds_read_b64 (a merged ds_read2_b64 occupies the LDS twice as long as two single
// reads, MI355X_MICROARCH.md); volatile only stops the merge
__device__ __forceinline__ ch_v2f ch_lds(const c32 *p)
{
	typedef const volatile ch_v2f __attribute__((address_space(3))) *lds_ptr;
	return *(lds_ptr)(p);
}

__global__ void __launch_bounds__(CH_TPB) __attribute__((amdgpu_waves_per_eu(4, 4)))     // 4 workgroups of 34 KB LDS per CU
channelize_kernel(const uint32_t *__restrict__ in, c32 *__restrict__ out, size_t n_total, size_t out_stride,
		  const trx_tables *__restrict__ tab, const uint4 *__restrict__ hist)
{
	// wideband time steps (T0-15) .. (T0+CH_TILE-1) as fp32, per path and phase: xs[p][t & 3][t >> 2], t = T - (T0-15)
	__shared__ __attribute__((aligned(16))) c32 xs[CH_M][4][CH_PHA];
	__shared__ __attribute__((aligned(16))) float taps[CH_M][CH_H];
	if (threadIdx.x < CH_M * CH_H)
		taps[threadIdx.x / CH_H][threadIdx.x % CH_H] = tab->chan_taps[threadIdx.x / CH_H][threadIdx.x % CH_H];
	const uint4 *in4 = reinterpret_cast<const uint4 *>(in);
	auto stage = [&](int t, uint4 u) {         // time step t of the tile (0..14 = history) -> the four paths' fp32 samples
		const uint32_t w[4] = { u.x, u.y, u.z, u.w };
#pragma unroll
		for (int n = 0; n < CH_M; n++)         // path M-1-n <- wideband sample n of the time step (Channelizer.cpp:37-48)
			xs[CH_M - 1 - n][t & 3][t >> 2] = make_float2((float)(int16_t)(w[n] & 0xffffu), (float)(int16_t)(w[n] >> 16));
	};

	// A workgroup owns a contiguous run of tiles: the last 15 time steps of one tile are the history of the next, so every
	// tile costs exactly CH_J aligned 16-byte loads per thread, and those of tile k+1 are issued before tile k is
	// computed (register prefetch: the loads stay in flight during the arithmetic instead of in front of a barrier).
	const size_t n_tiles = (n_total + CH_TILE - 1) / CH_TILE;
	const size_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
	const size_t tile_lo = (size_t)blockIdx.x * per_wg;
	const size_t tile_hi = (tile_lo + per_wg < n_tiles) ? tile_lo + per_wg : n_tiles;
	uint4 pre[CH_J], carry = make_uint4(0u, 0u, 0u, 0u);
	auto prefetch = [&](size_t tile) {
#pragma unroll
		for (int i = 0; i < CH_J; i++) {
			const size_t ts = tile * CH_TILE + (size_t)i * CH_TPB + threadIdx.x;
			pre[i] = (ts < n_total) ? in4[ts] : make_uint4(0u, 0u, 0u, 0u);
		}
	};
	if (tile_lo < tile_hi) {
		prefetch(tile_lo);
		if (threadIdx.x >= CH_TPB - (CH_H - 1)) {                              // history of the run's first tile, from memory
			const long long ts = (long long)(tile_lo * CH_TILE) - CH_TPB + threadIdx.x;   // time steps T0-15 .. T0-1
			if (ts >= 0)
				carry = in4[ts];
			else if (hist)
				carry = hist[(CH_H - 1) + ts];                                 // carried history of a stream: time steps -15..-1
		}
	}
	for (size_t tile = tile_lo; tile < tile_hi; tile++) {
		const size_t T0 = tile * CH_TILE;
		__syncthreads();
		if (threadIdx.x >= CH_TPB - (CH_H - 1))
			stage(threadIdx.x - (CH_TPB - (CH_H - 1)), carry);                 // t = 0..14
#pragma unroll
		for (int i = 0; i < CH_J; i++)
			stage((CH_H - 1) + i * CH_TPB + threadIdx.x, pre[i]);
		carry = pre[CH_J - 1];                                                 // threads 241..255: the tile's last 15 time steps
		__syncthreads();
		if (tile + 1 < tile_hi)
			prefetch(tile + 1);
		const size_t T = T0 + (size_t)CH_J * threadIdx.x;                     // first of this thread's CH_J output times
		if (T < n_total) {
			c32 yp[CH_J][CH_M];
#pragma unroll
			for (int p = 0; p < CH_M; p++) {
				// samples v = 0 .. 18 of the thread's window: tap k of output j is sample j + k
				ch_v2f x[CH_J + CH_H - 1];
#pragma unroll
				for (int v = 0; v < CH_J + CH_H - 1; v++) {
					x[v] = ch_lds(&xs[p][v & 3][threadIdx.x + (v >> 2)]);
				}
				const float2 *g2 = reinterpret_cast<const float2 *>(&taps[p][0]);   // broadcast reads, a pair of taps each
				ch_v2f acc[CH_J];
#pragma unroll
				for (int j = 0; j < CH_J; j++)
					acc[j] = (ch_v2f){ 0.0f, 0.0f };
#pragma unroll
				for (int k = 0; k < CH_H; k++) {
					const float2 gq = g2[k >> 1];
					const ch_v2f gp = (ch_v2f){ gq.x, gq.y };
#pragma unroll
					for (int j = 0; j < CH_J; j++)
						acc[j] = acc[j] + ((k & 1) ? ch_mul_tap<1>(x[j + k], gp) : ch_mul_tap<0>(x[j + k], gp));
					if (k & 1)
						__builtin_amdgcn_sched_barrier(0);                     // keeps the products from piling up in registers
				}
#pragma unroll
				for (int j = 0; j < CH_J; j++) {
					asm volatile("" : "+v"(acc[j]));                           // the sums are finished here (not sunk into the store branches)
					yp[j][p] = make_float2(acc[j].x, acc[j].y);
				}
				__builtin_amdgcn_sched_barrier(0);                             // one path's window in registers at a time
			}
			// forward 4-point DFT per output time, radix-2 butterflies (exact +-1 / +-j twiddles)
			c32 o[CH_M][CH_J];
#pragma unroll
			for (int j = 0; j < CH_J; j++) {
				const c32 t1 = make_float2(yp[j][0].x + yp[j][2].x, yp[j][0].y + yp[j][2].y);
				const c32 t2 = make_float2(yp[j][0].x - yp[j][2].x, yp[j][0].y - yp[j][2].y);
				const c32 t3 = make_float2(yp[j][1].x + yp[j][3].x, yp[j][1].y + yp[j][3].y);
				const c32 t4 = make_float2(yp[j][1].x - yp[j][3].x, yp[j][1].y - yp[j][3].y);
				o[0][j] = make_float2(t1.x + t3.x, t1.y + t3.y);
				o[1][j] = make_float2(t2.x + t4.y, t2.y - t4.x);               // t2 - j*t4
				o[2][j] = make_float2(t1.x - t3.x, t1.y - t3.y);
				o[3][j] = make_float2(t2.x - t4.y, t2.y + t4.x);               // t2 + j*t4
			}
			// 32 contiguous bytes per channel and thread: two 16-byte stores when the row allows it
			const bool vec = (T + CH_J <= n_total) && ((out_stride & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
#pragma unroll
			for (int c = 0; c < CH_M; c++) {
				c32 *dst = out + c * out_stride + T;
				if (vec) {
					reinterpret_cast<float4 *>(dst)[0] = make_float4(o[c][0].x, o[c][0].y, o[c][1].x, o[c][1].y);
					reinterpret_cast<float4 *>(dst)[1] = make_float4(o[c][2].x, o[c][2].y, o[c][3].x, o[c][3].y);
				} else {
#pragma unroll
					for (int j = 0; j < CH_J; j++)
						if (T + j < n_total)
							dst[j] = o[c][j];
				}
			}
		}
	}
}

// tail of a chunk -> history for the next one: the last 15 time steps (wideband) / samples (per channel)
__global__ void save_wide_hist_kernel(const uint4 *__restrict__ in4, size_t n_total, uint4 *__restrict__ hist)
{
	const int t = threadIdx.x;
	if (t < CH_H - 1) {
		const long long ts = (long long)n_total - (CH_H - 1) + t;
		const uint4 v = (ts >= 0) ? in4[ts] : hist[t + (int)n_total];       // chunk shorter than the history: shift
		__syncthreads();
		hist[t] = v;
	}
}

__global__ void save_chan_hist_kernel(const c32 *__restrict__ x, size_t n_in, size_t in_stride, c32 *__restrict__ hist)
{
	const int t = threadIdx.x, c = blockIdx.x;
	if (t < 15) {
		const long long s = (long long)n_in - 15 + t;
		const c32 v = (s >= 0) ? x[c * in_stride + s] : hist[c * 16 + t + (int)n_in];
		__syncthreads();
		hist[c * 16 + t] = v;
	}
}

extern "C" int trx_launch_channelize(const int16_t *d_in, float *d_out, size_t n_total, size_t out_stride,
				     const trx_tables *d_tab, void *d_hist_io, hipStream_t stream)
{
	if (n_total == 0)
		return 0;
	size_t blocks = (n_total + CH_TILE - 1) / CH_TILE;
	if (blocks > 256 * 4) blocks = 256 * 4;                              // 4 workgroups of 34 KB LDS per CU, each a run of tiles
	hipLaunchKernelGGL(channelize_kernel, dim3((unsigned)blocks), dim3(CH_TPB), 0, stream,
			   reinterpret_cast<const uint32_t *>(d_in), reinterpret_cast<c32 *>(d_out), n_total, out_stride, d_tab,
			   reinterpret_cast<const uint4 *>(d_hist_io));
	if (d_hist_io)
		hipLaunchKernelGGL(save_wide_hist_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const uint4 *>(d_in),
				   n_total, reinterpret_cast<uint4 *>(d_hist_io));
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// Resampler(p, q, 16)::rotate over a continuous stream per channel:
//   out[I] = sum_k in[n - 15 + k] * part[path][k],  n = (q*I)/p,  path = (q*I)%p     (Resampler.cpp:139-147,157-162)
// (per-block processing with history splice in the reference == the continuous formula, because
//  q*out_block == p*in_block; zero history before the first sample)
// Tiling: one workgroup handles TM periods = p*TM outputs from q*TM inputs (+15 of history) staged in LDS with
// coalesced loads; outputs are written coalesced; taps sit in LDS as [k][path] so that lanes (different
// paths) spread over the banks.  Index math is 32-bit inside a tile (the tile base is a multiple of the period).
// ------------------------------------------------------------------------------------------------
#define RS_TPB 256
#define RS_TILE_IN 3072                                                  // about q*TM input samples per tile

// Outputs o and o + p*m share their filter path ((q*o) % p), so a thread that walks o = t, t + S, t + 2S, ... with
// S = p*m (m = ceil(256 / p): S = 260 for 65/48, 65/96 and 52/75) keeps its 16 taps in registers for the whole kernel and
// reads only its 16 input samples from LDS per output; its input index advances by q*m per step.  The S - 256 output
// residues no thread owns (4 of 260) are swept afterwards with the taps read from LDS per output.
__global__ void __launch_bounds__(RS_TPB)
resample_kernel(const c32 *__restrict__ in, c32 *__restrict__ out, size_t n_in, size_t n_out, int p, int q, int tm, int m,
		size_t n_tiles, size_t in_stride, size_t out_stride, const float *__restrict__ parts,
		const c32 *__restrict__ hist)
{
	extern __shared__ __attribute__((aligned(16))) char rs_smem[];
	c32 *xs = reinterpret_cast<c32 *>(rs_smem);                          // [15 + q*tm]
	float *taps = reinterpret_cast<float *>(xs + 16 + q * tm);           // [16][p + 1]
	const int pst = p + 1;
	for (int i = threadIdx.x; i < p * 16; i += RS_TPB)
		taps[(i % 16) * pst + (i / 16)] = parts[i];
	const size_t chan = blockIdx.y;
	const c32 *x = in + chan * in_stride;
	c32 *y = out + chan * out_stride;
	const int tile_in = q * tm, tile_out = p * tm;
	const int S = p * m, iters = tm / m;                                 // tm is a multiple of m (launcher)
	const int t = threadIdx.x;
	const bool owner = t < S;                                            // (S >= 256 unless p > 256: then S = p and some threads idle)
	const unsigned qt = (unsigned)q * (unsigned)t;
	const int n_t = (int)(qt / (unsigned)p), path_t = (int)(qt % (unsigned)p);
	ch_v2f h2[8];                                                        // this thread's 16 taps, in pairs
#pragma unroll
	for (int k = 0; k < 8; k++)
		h2[k] = owner ? (ch_v2f){ parts[path_t * 16 + 2 * k], parts[path_t * 16 + 2 * k + 1] } : (ch_v2f){ 0.0f, 0.0f };
	const int nstep = q * m;
	// a workgroup owns a contiguous run of tiles and fetches tile k+1 into registers before it computes tile k
	constexpr int NPRE = (RS_TILE_IN + RS_TPB - 1) / RS_TPB;             // tile_in <= RS_TILE_IN
	const size_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
	const size_t tile_lo = (size_t)blockIdx.x * per_wg;
	const size_t tile_hi = (tile_lo + per_wg < n_tiles) ? tile_lo + per_wg : n_tiles;
	c32 pre[NPRE], pre_h = make_float2(0.0f, 0.0f);
	auto prefetch = [&](size_t tile) {
		const long long n0 = (long long)tile * tile_in;                    // first input sample of the tile
#pragma unroll
		for (int i = 0; i < NPRE; i++) {
			const int j = i * RS_TPB + t;
			const size_t sidx = (size_t)n0 + j;
			pre[i] = (j < tile_in && sidx < n_in) ? x[sidx] : make_float2(0.0f, 0.0f);
		}
		if (t < 15) {                                                      // the 15 samples in front of the tile
			const long long sidx = n0 - 15 + t;
			pre_h = make_float2(0.0f, 0.0f);
			if (sidx >= 0) { if ((size_t)sidx < n_in) pre_h = x[sidx]; }
			else if (hist) pre_h = hist[chan * 16 + 15 + sidx];                // carried history: samples -15..-1
		}
	};
	if (tile_lo < tile_hi)
		prefetch(tile_lo);
	for (size_t tile = tile_lo; tile < tile_hi; tile++) {
		__syncthreads();
		if (t < 15)
			xs[t] = pre_h;
#pragma unroll
		for (int i = 0; i < NPRE; i++) {
			const int j = i * RS_TPB + t;
			if (j < tile_in)
				xs[15 + j] = pre[i];
		}
		__syncthreads();
		if (tile + 1 < tile_hi)
			prefetch(tile + 1);
		const size_t o0 = tile * (size_t)tile_out;
		if (owner) {
			const c32 *xp = xs + n_t;                                      // xs[j] = in[n0 - 15 + j]
			c32 *yo = y + o0 + t;
			size_t o = o0 + t;
			for (int it = 0; it < iters && o < n_out; it++, o += S, xp += nstep, yo += S) {
				ch_v2f acc = { 0.0f, 0.0f };
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const ch_v2f xv = ch_lds(xp + k);
					acc = acc + ((k & 1) ? ch_mul_tap<1>(xv, h2[k >> 1]) : ch_mul_tap<0>(xv, h2[k >> 1]));   // product, then sum
				}
				*yo = make_float2(acc.x, acc.y);
			}
		}
		// residues RS_TPB .. S-1 of every step: (S - RS_TPB) * iters outputs, taps from LDS
		const int nres = S - RS_TPB;
		for (int idx = t; idx < nres * iters; idx += RS_TPB) {
			const int o = RS_TPB + idx % nres + S * (idx / nres);
			if (o0 + o >= n_out)
				continue;
			const unsigned qi = (unsigned)q * (unsigned)o;
			const int n = (int)(qi / (unsigned)p), path = (int)(qi % (unsigned)p);
			const c32 *xp = xs + n;
			float yr = 0.0f, yi = 0.0f;
#pragma unroll
			for (int k = 0; k < 16; k++) {
				const c32 xv = xp[k];
				const float h = taps[k * pst + path];
				yr += xv.x * h;
				yi += xv.y * h;
			}
			y[o0 + o] = make_float2(yr, yi);
		}
	}
}

extern "C" int trx_launch_resample(const float *d_in, float *d_out, size_t n_in, int p, int q, size_t n_chan,
				   size_t in_stride, size_t out_stride, const float *parts, void *d_hist_io, hipStream_t stream)
{
	const size_t n_out = n_in / q * p;
	if (n_chan * n_out == 0)
		return 0;
	const int m = (RS_TPB + p - 1) / p;                                  // outputs o and o + p*m share a filter path
	int tm = RS_TILE_IN / q / m * m;                                     // periods per tile: a multiple of m
	if (tm < m) tm = m;
	const size_t n_tiles = (n_out + (size_t)p * tm - 1) / ((size_t)p * tm);
	size_t gx = n_tiles;
	const size_t gmax = 1024 / n_chan > 0 ? 1024 / n_chan : 1;           // 4 workgroups (29 KB of LDS, 112 VGPRs) per CU over all channels,
	if (gx > gmax) gx = gmax;                                            // each walking a contiguous run of tiles
	const size_t lds = (size_t)(16 + q * tm) * sizeof(c32) + (size_t)16 * (p + 1) * sizeof(float);
	hipLaunchKernelGGL(resample_kernel, dim3((unsigned)gx, (unsigned)n_chan), dim3(RS_TPB), lds, stream,
			   reinterpret_cast<const c32 *>(d_in), reinterpret_cast<c32 *>(d_out), n_in, n_out, p, q, tm, m, n_tiles,
			   in_stride, out_stride, parts, reinterpret_cast<const c32 *>(d_hist_io));
	if (d_hist_io)
		hipLaunchKernelGGL(save_chan_hist_kernel, dim3((unsigned)n_chan), dim3(64), 0, stream,
				   reinterpret_cast<const c32 *>(d_in), n_in, in_stride, reinterpret_cast<c32 *>(d_hist_io));
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// frontend_fused_kernel<NACT>: RadioInterfaceMulti::pullBuffer (radioInterfaceMulti.cpp:237-314) --
// Channelizer(4, ., 16)::rotate and Resampler(p, q, 16)::rotate of the four channels in ONE pass (round 3): the channel-rate
// streams never touch HBM.  The two kernels above move  16 B in + 32 B out  and  32 B in + 32 p/q B out  per wideband
// time step; fused it is 16 B in + 32 p/q B out -- 59 B instead of 123 B for 65/48.
// A workgroup owns a run of tiles of tm resampler periods = q*tm channel-rate time steps (960 for 65/48).  Per tile:
//   1. the wideband steps [T0 - 30, T0 + q*tm) are staged as fp32 in the channelizer's 4-phase layout (prefetched into
//      registers while the previous tile is computed; the 30 steps of overlap with the previous tile come from L2);
//   2. every thread computes 4 consecutive channel-rate times of all 4 channels -- the same 16-tap sums and the same
//      4-point DFT as channelize_kernel -- for the times [T0 - 15, T0 + q*tm): the resampler's 15 samples of history are
//      recomputed, not carried (the stream's very first tile takes them from the carried history instead);
//   3. behind a barrier the channel samples go to LDS OVER the staged wideband samples (34 KB per workgroup, four
//      workgroups per CU as before);
//   4. every thread resamples the outputs t, t + S, ... (S = p*m: same filter path, taps in registers) of all four
//      channels, exactly as resample_kernel does, and the residues S - 256 .. S - 1 are swept afterwards.
// Arithmetic and operand order are those of the two kernels: the results are bit-identical to running them in sequence
// (tests/test_gpu_aux_kernels.py).  The last tile's workgroup leaves the final 15 channel samples in hist_out.
// NACT = 4 is that: the four filterbank paths in physical order (trxhip_rx_frontend_create).  NACT = 1..3 is the reference's
// object for 1..3 ARFCNs (trxhip_rx_frontend_create_chans): all four path filters feed every DFT bin, so steps 1 and the
// filters of 2 do not shrink, but only the NACT active bins are formed, parked and resampled, and row l of out, of cs and of
// the [NACT][16] channel histories is logical channel l = filterbank path trx_arfcn_pchan(NACT, l).  Every output is the same
// products and sums in the same order for every NACT (tests/test_gpu_rx_frontend_chans.py); per 192-step block at 65/48 the
// kernel moves 3072 + NACT * 2080 B.
// ------------------------------------------------------------------------------------------------
#define FE_CS 1056                      // entries per channel in the aliased LDS array (>= q*tm + 15, <= 4 * CH_PHA)

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations, not for its global loads and stores.
// __syncthreads() also drains vmcnt -- here that would wait, at every phase change, for the previous tile's output stores
// to be acknowledged by HBM and for the next tile's prefetch loads to land, which is most of what the two-kernel form spends.
__device__ __forceinline__ void fe_lds_barrier()
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// bin pc of the forward 4-point DFT from the radix-2 terms (exact +-1 / +-j twiddles), channelize_kernel's expressions
__device__ __forceinline__ c32 fe_bin(int pc, c32 t1, c32 t2, c32 t3, c32 t4)
{
	switch (pc) {
	case 0: return make_float2(t1.x + t3.x, t1.y + t3.y);
	case 1: return make_float2(t2.x + t4.y, t2.y - t4.x);              // t2 - j*t4
	case 2: return make_float2(t1.x - t3.x, t1.y - t3.y);
	default: return make_float2(t2.x - t4.y, t2.y + t4.x);             // t2 + j*t4
	}
}

template <int NACT>
__global__ void __launch_bounds__(CH_TPB) __attribute__((amdgpu_waves_per_eu(4, 4)))
frontend_fused_kernel(const uint4 *__restrict__ in4, size_t n_total, c32 *__restrict__ out, size_t n_out, size_t out_stride,
		      int p, int q, int tm, int m, size_t n_tiles, const float *__restrict__ parts,
		      const trx_tables *__restrict__ tab, const uint4 *__restrict__ wide_hist,
		      const c32 *__restrict__ chan_hist_in, c32 *__restrict__ chan_hist_out)
{
	__shared__ __attribute__((aligned(16))) c32 xs[CH_M][4][CH_PHA];     // wideband staging, then cs[NACT][FE_CS]
	__shared__ __attribute__((aligned(16))) float taps[CH_M][CH_H];
	extern __shared__ __attribute__((aligned(16))) char fe_smem[];        // resampler taps [16][p + 1] (residue sweep)
	float *rtaps = reinterpret_cast<float *>(fe_smem);
	c32 *const cs = &xs[0][0][0];
	static_assert(NACT >= 1 && NACT <= CH_M, "1..3 logical channels, or the four paths");
	static_assert(NACT * FE_CS <= CH_M * 4 * CH_PHA, "the channel samples alias the wideband staging");
	const int t = threadIdx.x;
	const int pst = p + 1;
	if (t < CH_M * CH_H)
		taps[t / CH_H][t % CH_H] = tab->chan_taps[t / CH_H][t % CH_H];
	for (int i = t; i < p * 16; i += CH_TPB)
		rtaps[(i % 16) * pst + (i / 16)] = parts[i];
	const int tile_in = q * tm, tile_out = p * tm;
	const int n_stage = tile_in + 30;                                    // wideband steps staged per tile (<= 4 * CH_TPB)
	const int n_cs = tile_in + 15;                                       // channel-rate times computed per tile
	// Resampling as in resample_kernel: thread t owns the outputs t, t + S, ... (S = p*m: the same filter path at every step,
	// taps in registers).  (A variant with output PAIRS per thread -- 17 LDS reads for two outputs instead of 32, the second
	// output's taps shifted inside 17 entries -- read a third less from LDS and was slower: smaller tiles, more of the
	// per-tile latency chain below.  The kernel is bound by that chain, not by LDS or arithmetic; profiles/r03_ab_runs.txt.)
	const int S = p * m, iters = tm / m;
	const bool owner = t < S;
	const unsigned qt = (unsigned)q * (unsigned)t;
	const int n_t0 = (int)(qt / (unsigned)p), path_t0 = (int)(qt % (unsigned)p);
	const int nstep = q * m;

	// The residues S - 256 .. S - 1 of every resampler step (all channels) are swept item by item.  Which output, which filter
	// path and which input sample an item is depends on the item alone, not on the tile: worked out once, here, and parked in
	// LDS as two packed words -- per tile the four integer divisions (~ 160 instructions on the waves that hold items, which
	// the other waves of the workgroup then wait for at the next barrier) become one 8-byte read.
	// (first sample, filter path) of this thread's output positions: a function of the thread alone, but kept in two registers
	// across the tile loop it was what the allocator spilled at 128 -- and a scratch reload in front of the resampler loop waits
	// for vmcnt(0), i.e. for the next tile's prefetch that has just been issued.  Parked in LDS, one ds_read_b32 per tile.
	int *const thr_item = reinterpret_cast<int *>(rtaps + 16 * pst);
	thr_item[t] = (n_t0 << 16) | path_t0;
	const int n_res = (S - CH_TPB) * iters * NACT;
	int2 *const res_item = reinterpret_cast<int2 *>(rtaps + 16 * pst + CH_TPB);
	for (int idx = t; idx < n_res; idx += CH_TPB) {
		const int nres0 = S - CH_TPB;
		const int c = idx / (nres0 * iters), r = idx % (nres0 * iters);
		const int oi = CH_TPB + r % nres0 + S * (r / nres0);
		const unsigned qi = (unsigned)q * (unsigned)oi;
		res_item[idx] = make_int2((c << 16) | (int)(qi / (unsigned)p), (oi << 16) | (int)(qi % (unsigned)p));
	}
	const size_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
	const size_t tile_lo = (size_t)blockIdx.x * per_wg;
	const size_t tile_hi = (tile_lo + per_wg < n_tiles) ? tile_lo + per_wg : n_tiles;
	uint4 pre[4];
	auto prefetch = [&](size_t tile) {
		// staged step j (0 <= j < n_stage) is wideband step t0 + j.  Everything that depends on the tile is wave-uniform: the
		// range [jlo, jhi) of steps inside the stream and a base pointer; a thread adds its 32-bit j.  (Round 5: the 64-bit
		// per-thread step numbers this replaces were spilled to scratch, and every reload waited for vmcnt(0) -- for the
		// previous tile's output stores -- in the middle of the tile loop.)
		const long long t0 = (long long)tile * tile_in - 30;               // first staged wideband step
		const long long lo = t0 < 0 ? -t0 : 0, hi = (long long)n_total - t0;
		const int jlo = (int)(lo < n_stage ? lo : n_stage), jhi = (int)(hi < 0 ? 0 : (hi < n_stage ? hi : n_stage));
		const uint4 *const base = in4 + t0;                                 // (dereferenced for jlo <= j < jhi only)
		const int hoff = (int)((CH_H - 1) + t0);                            // tile 0: steps -15 .. -1 come from the carried history
		if (jlo == 0 && jhi == n_stage) {
			// a tile inside the stream (all but the first and the last): four unconditional loads.  A branch of its own, and
			// wave-uniform -- with the edge cases as the other arm of a per-lane if, both arms ran one after the other in every
			// wave, both wrote pre[i], and the compiler put an s_waitcnt vmcnt(0) between them: loads three and four of every
			// tile waited for loads one and two to come back from HBM.
			unsigned tt = (unsigned)t;                                       // opaque per tile: the four clamped offsets are three instructions
			asm volatile("" : "+v"(tt));                                    // each to recompute, and 8 registers (spilled) to keep across tiles
			const unsigned jmax = (unsigned)n_stage - 1u;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const unsigned j = (unsigned)(i * CH_TPB) + tt;
				pre[i] = base[j < jmax ? j : jmax];                            // (j >= n_stage is never staged)
			}
			return;
		}
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int j = i * CH_TPB + t;
			uint4 v = make_uint4(0u, 0u, 0u, 0u);
			if (j >= jlo && j < jhi)
				v = base[j];
			else if (j < jlo && hoff + j >= 0 && wide_hist)
				v = wide_hist[hoff + j];
			pre[i] = v;
		}
	};
	if (tile_lo < tile_hi)
		prefetch(tile_lo);
	for (size_t tile = tile_lo; tile < tile_hi; tile++) {
		fe_lds_barrier();                                                   // (the previous tile's channel samples are done with)
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int j = i * CH_TPB + t;
			if (j < n_stage) {
				const uint32_t w[4] = { pre[i].x, pre[i].y, pre[i].z, pre[i].w };
#pragma unroll
				for (int n = 0; n < CH_M; n++)                                 // path M-1-n <- wideband sample n of the time step
					xs[CH_M - 1 - n][j & 3][j >> 2] = make_float2((float)(int16_t)(w[n] & 0xffffu), (float)(int16_t)(w[n] >> 16));
			}
		}
		fe_lds_barrier();

		// ---- channelizer: channel-rate times u = 4t .. 4t+3 of the tile (time T0 - 15 + u); tap k of output u is staged step u + k
		c32 o[NACT][CH_J];
		const bool active = CH_J * t < n_cs;
		if (active) {
			c32 yp[CH_J][CH_M];
#pragma unroll
			for (int pp = 0; pp < CH_M; pp++) {
				// The window is requested LAST sample first: the first product needs x[0], the newest request, and its s_waitcnt
				// covers the whole window (LDS returns in order) -- one wait per path where the ascending order had one per tap.
				ch_v2f x[CH_J + CH_H - 1];
#pragma unroll
				for (int v = CH_J + CH_H - 2; v >= 0; v--)
					x[v] = ch_lds(&xs[pp][v & 3][t + (v >> 2)]);
				// (round 5 measured these 16 wave-uniform taps as scalar operands of the packed multiplies, fetched per path through
				// the scalar cache instead of LDS: 1.30 ms against 1.04 -- the s_load and its lgkmcnt wait sit in front of every
				// path's sums; profiles/r05_ab_runs.txt)
				// A pair of taps is one broadcast 8-byte read, requested one pair AHEAD of its use (the compiler had sunk each read
				// to its first use: request, s_waitcnt lgkmcnt(0), multiply -- a full LDS round trip in front of every tap pair).
				// Products of tap k alternate with the sums of tap k - 1: a dependent packed pair costs a pad, and a packed
				// instruction in between does not count as one (see the resampler loop below).
				typedef const volatile ch_v2f __attribute__((address_space(3))) *lds_tap;
				const lds_tap g2 = (lds_tap)(&taps[pp][0]);
				ch_v2f acc[CH_J], pr[CH_J];
#pragma unroll
				for (int j = 0; j < CH_J; j++)
					acc[j] = pr[j] = (ch_v2f){ 0.0f, 0.0f };
				ch_v2f gcur = g2[0];
#pragma unroll
				for (int kp = 0; kp < CH_H / 2; kp++) {
					ch_v2f gnext = gcur;
					if (kp + 1 < CH_H / 2)
						gnext = g2[kp + 1];
#pragma unroll
					for (int kk = 0; kk < 2; kk++) {
						const int k = 2 * kp + kk;
#pragma unroll
						for (int j = 0; j < CH_J; j++) {
							const ch_v2f pn = kk ? ch_mul_tap<1>(x[j + k], gcur) : ch_mul_tap<0>(x[j + k], gcur);
							if (k > 0)
								acc[j] = acc[j] + pr[j];                               // product, then sum: tap k - 1
							pr[j] = pn;
							__builtin_amdgcn_sched_barrier(0);
						}
					}
					gcur = gnext;
				}
#pragma unroll
				for (int j = 0; j < CH_J; j++)
					acc[j] = acc[j] + pr[j];                                           // tap 15
#pragma unroll
				for (int j = 0; j < CH_J; j++) {
					asm volatile("" : "+v"(acc[j]));
					yp[j][pp] = make_float2(acc[j].x, acc[j].y);
				}
				__builtin_amdgcn_sched_barrier(0);
			}
#pragma unroll
			for (int j = 0; j < CH_J; j++) {                                   // the rows' bins of the forward 4-point DFT
				const c32 t1 = make_float2(yp[j][0].x + yp[j][2].x, yp[j][0].y + yp[j][2].y);
				const c32 t2 = make_float2(yp[j][0].x - yp[j][2].x, yp[j][0].y - yp[j][2].y);
				const c32 t3 = make_float2(yp[j][1].x + yp[j][3].x, yp[j][1].y + yp[j][3].y);
				const c32 t4 = make_float2(yp[j][1].x - yp[j][3].x, yp[j][1].y - yp[j][3].y);
#pragma unroll
				for (int c = 0; c < NACT; c++)
					o[c][j] = fe_bin(trx_arfcn_pchan(NACT, c), t1, t2, t3, t4);
			}
		}
		if (tile + 1 < tile_hi)                                            // (here, not before the filters: 16 registers they need)
			prefetch(tile + 1);
		fe_lds_barrier();                                                   // every window has been read: the staging area is free
		if (active) {
#pragma unroll
			for (int c = 0; c < NACT; c++) {
				float4 *dst = reinterpret_cast<float4 *>(cs + c * FE_CS + CH_J * t);
				dst[0] = make_float4(o[c][0].x, o[c][0].y, o[c][1].x, o[c][1].y);
				dst[1] = make_float4(o[c][2].x, o[c][2].y, o[c][3].x, o[c][3].y);
			}
		}
		if (tile == 0) {                                                   // the stream's first tile: times -15 .. -1 are the carried history
			fe_lds_barrier();
			if (t < NACT * 15)
				cs[(t / 15) * FE_CS + (t % 15)] = chan_hist_in ? chan_hist_in[(t / 15) * 16 + (t % 15)] : make_float2(0.0f, 0.0f);
		}
		fe_lds_barrier();

		// ---- resampler: cs[c][j] = row c at time T0 - 15 + j
		const size_t o0 = tile * (size_t)tile_out;
		if (owner) {
			// this thread's 16 taps (path (q t) mod p), re-read from LDS per tile: 16 registers the channelizer above needs more
			// than this loop does.  Two CHANNELS of an output position per pass: the same taps and offsets, 32 LDS reads in
			// flight and two independent sum chains instead of one (the waves of this kernel wait two thirds of their time:
			// profiles/r04_ab_runs.txt); each output's sum still runs k = 0..15, product then add.
			typedef const volatile int __attribute__((address_space(3))) *lds_int;
			int tl = t;                                                     // (opaque: the address is one instruction to form per tile -- hoisted
			asm volatile("" : "+v"(tl));                                    // out of the tile loop it was the next value to be spilled)
			const int ti = *(lds_int)(thr_item + tl);
			const int n_t = ti >> 16, path_t = ti & 0xffff;
			ch_v2f h2[8];
#pragma unroll
			for (int k = 0; k < 8; k++)
				h2[k] = (ch_v2f){ rtaps[(2 * k) * pst + path_t], rtaps[(2 * k + 1) * pst + path_t] };
			{
				// all NACT rows of an output position per pass: NACT independent sum chains over the same taps and offsets,
				// 4 * NACT LDS reads in flight per block of four taps
				const c32 *xa = cs + n_t;
				c32 *const ob = out + o0;                                   // wave-uniform base; the thread adds a 32-bit offset
				unsigned yo = (unsigned)t;                                  // (a per-thread 64-bit pointer here was spilled and reloaded --
				size_t oo = o0 + t;                                         // behind a vmcnt(0) wait -- once per tile)
				for (int it = 0; it < iters && oo < n_out; it++, oo += S, xa += nstep, yo += (unsigned)S) {
					ch_v2f acc[NACT], pr[NACT];
#pragma unroll
					for (int c = 0; c < NACT; c++)
						acc[c] = pr[c] = (ch_v2f){ 0.0f, 0.0f };
#pragma unroll
					for (int k0 = 0; k0 < 16; k0 += 4) {
						ch_v2f x[NACT][4];
#pragma unroll
						for (int k = 0; k < 4; k++)
#pragma unroll
							for (int c = 0; c < NACT; c++)
								x[c][k] = ch_lds(xa + c * FE_CS + k0 + k);
						// (Written for NACT = 4.)  A tap at a time, software-pipelined: the four channels' products of tap k (the LAST-read channel first -- its
						// s_waitcnt covers the other three, LDS returns in order) alternate with the four sums of tap k - 1.  Written as
						// product + sum per channel the compiler ran all sixteen through one product register: wait, multiply, s_nop
						// (the pad of a dependent packed pair), add -- four issue slots per tap and channel where two do the
						// arithmetic; a packed instruction between the two does not count as their pad, so products and sums of the
						// SAME tap in two groups of four still paid one s_nop per tap (round 5).
#pragma unroll
						for (int k = 0; k < 4; k++) {
							const int kk = k0 + k;
#pragma unroll
							for (int c = NACT - 1; c >= 0; c--) {
								const ch_v2f pn = (kk & 1) ? ch_mul_tap<1>(x[c][k], h2[kk >> 1]) : ch_mul_tap<0>(x[c][k], h2[kk >> 1]);
								if (kk > 0)
									acc[c] = acc[c] + pr[c];                           // product, then sum: tap kk - 1
								pr[c] = pn;
								__builtin_amdgcn_sched_barrier(0);
							}
						}
					}
#pragma unroll
					for (int c = NACT - 1; c >= 0; c--)
						acc[c] = acc[c] + pr[c];                                       // tap 15
#pragma unroll
					for (int c = 0; c < NACT; c++)
						(ob + (size_t)c * out_stride)[yo] = make_float2(acc[c].x, acc[c].y);
				}
			}
		}
		int tr = t;                                                         // (opaque, as above: the item's address is formed per tile)
		asm volatile("" : "+v"(tr));
		for (int idx = tr; idx < n_res; idx += CH_TPB) {                   // residues of every step, all rows
			const int2 e = res_item[idx];
			const int c = e.x >> 16, n = e.x & 0xffff, oi = e.y >> 16, path = e.y & 0xffff;
			if (o0 + oi >= n_out)
				continue;
			const c32 *xp = cs + c * FE_CS + n;
			ch_v2f acc = { 0.0f, 0.0f };                                    // product, then sum, k ascending, on both components at once:
#pragma unroll
			for (int k = 0; k < 16; k++) {                                  // the two roundings per tap of yr += x.x * h, yi += x.y * h
				const float h = rtaps[k * pst + path];
				acc = acc + ch_lds(xp + k) * (ch_v2f){ h, h };
			}
			out[c * out_stride + o0 + oi] = make_float2(acc.x, acc.y);
		}
		if (chan_hist_out && tile + 1 == n_tiles && t < NACT * 15) {        // the call's last 15 channel samples of every row
			const long long j = (long long)n_total - (long long)tile * tile_in + (t % 15);   // time n_total - 15 + i -> cs index
			chan_hist_out[(t / 15) * 16 + (t % 15)] = cs[(t / 15) * FE_CS + j];
		}
	}
}

// the fused front end for rows = 1..3 logical channels or the 4 filterbank paths; returns 1 when the geometry fits no tile
// (the caller then runs channelize_kernel and resample_kernel), 0 / TRXHIP_E* otherwise
extern "C" int trx_launch_frontend_fused(const int16_t *d_wide, float *d_out, size_t n_total, int rows, int p, int q, size_t out_stride,
					 const float *parts, const trx_tables *d_tab, void *d_wide_hist_io, const void *d_chan_hist_in,
					 void *d_chan_hist_out, hipStream_t stream)
{
	if (rows < 1 || rows > CH_M)
		return TRXHIP_EINVAL;
	const int m = (CH_TPB + p - 1) / p;                                  // outputs o and o + p*m share a filter path
	const int tm = (4 * CH_TPB - 30) / q / m * m;                         // periods per tile: staging fits 4 loads per thread
	const size_t n_out = n_total / q * p;
	if (tm < m || p * m < CH_TPB || p * m > 2 * CH_TPB || q * tm + 15 > FE_CS || (n_total % (size_t)q) != 0 || n_total < 30 || n_out == 0)
		return 1;
	const size_t n_tiles = (n_out + (size_t)p * tm - 1) / ((size_t)p * tm);
	size_t gx = n_tiles < 1024 ? n_tiles : 1024;                         // 4 workgroups of 34 KB LDS per CU, each a run of tiles
	const size_t n_res = (size_t)(p * m - CH_TPB) * (tm / m) * rows;    // residue items per tile (80 at 65 / 48 and four rows)
	if (n_res > 1024)
		return 1;
	const size_t lds = (size_t)16 * (p + 1) * sizeof(float) + CH_TPB * sizeof(int) + n_res * sizeof(int2);   // resampler taps + the threads' items + the residue items
	auto *const kernel = rows == 1 ? frontend_fused_kernel<1> : rows == 2 ? frontend_fused_kernel<2> :
			     rows == 3 ? frontend_fused_kernel<3> : frontend_fused_kernel<4>;
	hipLaunchKernelGGL(kernel, dim3((unsigned)gx), dim3(CH_TPB), lds, stream, reinterpret_cast<const uint4 *>(d_wide),
			   n_total, reinterpret_cast<c32 *>(d_out), n_out, out_stride, p, q, tm, m, n_tiles, parts, d_tab,
			   reinterpret_cast<const uint4 *>(d_wide_hist_io), reinterpret_cast<const c32 *>(d_chan_hist_in),
			   reinterpret_cast<c32 *>(d_chan_hist_out));
	if (d_wide_hist_io)
		hipLaunchKernelGGL(save_wide_hist_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const uint4 *>(d_wide),
				   n_total, reinterpret_cast<uint4 *>(d_wide_hist_io));
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// RadioInterfaceResamp::pullBuffer in one pass: int16 IQ in (4 B per sample), (float)int16 while staging -- exact, so this
// is convert_short_float (convert_base.c:27-31) -- then Resampler(p, q, 16)::rotate as resample_kernel runs it:
//   out[I] = sum_k in[n - 15 + k] * part[path][k],  n = (q*I)/p,  path = (q*I)%p,  product then add, k ascending from 0.0f.
// A workgroup owns a run of tiles of tm periods (q*tm <= 3072 input samples) and fetches tile k+1 into registers while it
// computes tile k.  VEC: 16-byte loads, four samples each, when the tiles and the stream allow it (they do for the
// reference's 1536 / 1200-sample chunks).  xs[j] = in[n0 - 16 + j]: the 16 samples in front of the stream's first tile are
// the carried history (dnsampler->len() samples, radioInterfaceResamp.cpp:146-147, :191; zero at a fresh object), and the
// last tile's workgroup leaves the call's last 16 input samples in hist_out -- the other half of a pair of buffers, the
// first and the last workgroup run at the same time.
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ c32 rx_cvt(uint32_t w)
{
	return make_float2((float)(int16_t)(w & 0xffffu), (float)(int16_t)(w >> 16));
}

template <bool VEC>
__global__ void __launch_bounds__(RS_TPB)
rx_resamp_s16_kernel(const uint32_t *__restrict__ in, c32 *__restrict__ out, size_t n_in, size_t n_out, int p, int q, int tm, int m,
		     size_t n_tiles, const float *__restrict__ parts, const uint32_t *__restrict__ hist_in, uint32_t *__restrict__ hist_out)
{
	extern __shared__ __attribute__((aligned(16))) char rxr_smem[];
	c32 *xs = reinterpret_cast<c32 *>(rxr_smem);                         // [16 + q*tm]
	const int tile_in = q * tm, tile_out = p * tm;
	float *taps = reinterpret_cast<float *>(xs + 16 + ((tile_in + 1) & ~1));   // [16][p + 1]
	const int pst = p + 1;
	const int t = threadIdx.x;
	for (int i = t; i < p * 16; i += RS_TPB)
		taps[(i % 16) * pst + (i / 16)] = parts[i];
	const int S = p * m, iters = tm / m;                                 // tm is a multiple of m (launcher); S >= 256 (p <= 128)
	const bool owner = t < S;
	const unsigned qt = (unsigned)q * (unsigned)t;
	const int n_t = (int)(qt / (unsigned)p), path_t = (int)(qt % (unsigned)p);
	ch_v2f h2[8];                                                        // this thread's 16 taps, in pairs
#pragma unroll
	for (int k = 0; k < 8; k++)
		h2[k] = owner ? (ch_v2f){ parts[path_t * 16 + 2 * k], parts[path_t * 16 + 2 * k + 1] } : (ch_v2f){ 0.0f, 0.0f };
	const int nstep = q * m;
	constexpr int NPRE = VEC ? RS_TILE_IN / 4 / RS_TPB : RS_TILE_IN / RS_TPB;   // tile_in <= RS_TILE_IN
	constexpr int W = VEC ? 4 : 1;                                       // samples per load
	const size_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
	const size_t tile_lo = (size_t)blockIdx.x * per_wg;
	const size_t tile_hi = (tile_lo + per_wg < n_tiles) ? tile_lo + per_wg : n_tiles;
	uint32_t pre[NPRE * W], pre_h = 0u;
	auto prefetch = [&](size_t tile) {
		const size_t n0 = tile * (size_t)tile_in;                          // first input sample of the tile (VEC: a multiple of 4)
#pragma unroll
		for (int i = 0; i < NPRE; i++) {
			const int j = (i * RS_TPB + t) * W;
			const bool in_range = j < tile_in && n0 + j < n_in;            // VEC: tile_in and n_in are multiples of 4, so all four are inside
			if constexpr (VEC) {
				const uint4 v = in_range ? *reinterpret_cast<const uint4 *>(in + n0 + j) : make_uint4(0u, 0u, 0u, 0u);
				pre[4 * i] = v.x; pre[4 * i + 1] = v.y; pre[4 * i + 2] = v.z; pre[4 * i + 3] = v.w;
			} else {
				pre[i] = in_range ? in[n0 + j] : 0u;
			}
		}
		if (t < 16) {                                                      // the 16 samples in front of the tile
			pre_h = 0u;
			if (n0 >= 16) pre_h = in[n0 - 16 + t];                         // (n0 < n_in for every tile of the call)
			else if (hist_in) pre_h = hist_in[t];                          // n0 == 0 (a tile holds >= 1536 samples): the carried samples -16 .. -1
		}
	};
	if (tile_lo < tile_hi)
		prefetch(tile_lo);
	for (size_t tile = tile_lo; tile < tile_hi; tile++) {
		__syncthreads();
		if (t < 16)
			xs[t] = rx_cvt(pre_h);
#pragma unroll
		for (int i = 0; i < NPRE; i++) {
			const int j = (i * RS_TPB + t) * W;
			if (j < tile_in) {
				if constexpr (VEC) {
					const c32 a = rx_cvt(pre[4 * i]), b = rx_cvt(pre[4 * i + 1]), c = rx_cvt(pre[4 * i + 2]), d = rx_cvt(pre[4 * i + 3]);
					float4 *dst = reinterpret_cast<float4 *>(xs + 16 + j);      // 16 + j is a multiple of 4 entries: 32-byte aligned
					dst[0] = make_float4(a.x, a.y, b.x, b.y);
					dst[1] = make_float4(c.x, c.y, d.x, d.y);
				} else {
					xs[16 + j] = rx_cvt(pre[i]);
				}
			}
		}
		__syncthreads();
		if (tile + 1 < tile_hi)
			prefetch(tile + 1);
		const size_t o0 = tile * (size_t)tile_out;
		if (owner) {
			const c32 *xp = xs + 1 + n_t;                                  // xs[j] = in[n0 - 16 + j]: tap k of sample n is xs[n + 1 + k]
			c32 *yo = out + o0 + t;
			size_t o = o0 + t;
			for (int it = 0; it < iters && o < n_out; it++, o += S, xp += nstep, yo += S) {
				ch_v2f acc = { 0.0f, 0.0f };
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const ch_v2f xv = ch_lds(xp + k);
					acc = acc + ((k & 1) ? ch_mul_tap<1>(xv, h2[k >> 1]) : ch_mul_tap<0>(xv, h2[k >> 1]));   // product, then sum
				}
				*yo = make_float2(acc.x, acc.y);
			}
		}
		// residues RS_TPB .. S-1 of every step: (S - RS_TPB) * iters outputs, taps from LDS
		const int nres = S - RS_TPB;
		for (int idx = t; idx < nres * iters; idx += RS_TPB) {
			const int o = RS_TPB + idx % nres + S * (idx / nres);
			if (o0 + o >= n_out)
				continue;
			const unsigned qi = (unsigned)q * (unsigned)o;
			const int n = (int)(qi / (unsigned)p), path = (int)(qi % (unsigned)p);
			const c32 *xp = xs + 1 + n;
			float yr = 0.0f, yi = 0.0f;
#pragma unroll
			for (int k = 0; k < 16; k++) {
				const c32 xv = xp[k];
				const float h = taps[k * pst + path];
				yr += xv.x * h;
				yi += xv.y * h;
			}
			out[o0 + o] = make_float2(yr, yi);
		}
		if (hist_out && tile + 1 == n_tiles && t < 16)                     // the call's last 16 input samples (n_in >= 16: launcher)
			hist_out[t] = in[n_in - 16 + t];
	}
}

extern "C" int trx_launch_rx_resamp_s16(const int16_t *d_in, float *d_out, size_t n_in, int p, int q, const float *parts,
					const void *d_hist_in, void *d_hist_out, hipStream_t stream)
{
	const size_t n_out = n_in / q * p;
	if (n_out == 0)
		return 0;
	if (p < 1 || p > 128 || q < 1 || (n_in % (size_t)q) != 0 || n_in < 16)
		return TRXHIP_EINVAL;
	const int m = (RS_TPB + p - 1) / p;                                  // outputs o and o + p*m share a filter path
	int tm = RS_TILE_IN / q / m * m;                                    // periods per tile: a multiple of m
	if (tm < m) tm = m;
	if ((long long)q * tm > RS_TILE_IN)
		return TRXHIP_EINVAL;                                            // the tile's registers and LDS
	const int tile_in = q * tm;
	const size_t n_tiles = (n_out + (size_t)p * tm - 1) / ((size_t)p * tm);
	const size_t gx = n_tiles < 1024 ? n_tiles : 1024;                   // 4 workgroups (<= 33 KB of LDS) per CU, each a run of tiles
	const size_t lds = (size_t)(16 + ((tile_in + 1) & ~1)) * sizeof(c32) + (size_t)16 * (p + 1) * sizeof(float);
	const uint32_t *in = reinterpret_cast<const uint32_t *>(d_in);
	const bool vec = (tile_in % 4) == 0 && (n_in % 4) == 0 && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
	if (vec)
		hipLaunchKernelGGL(rx_resamp_s16_kernel<true>, dim3((unsigned)gx), dim3(RS_TPB), lds, stream, in, reinterpret_cast<c32 *>(d_out),
				   n_in, n_out, p, q, tm, m, n_tiles, parts, reinterpret_cast<const uint32_t *>(d_hist_in),
				   reinterpret_cast<uint32_t *>(d_hist_out));
	else
		hipLaunchKernelGGL(rx_resamp_s16_kernel<false>, dim3((unsigned)gx), dim3(RS_TPB), lds, stream, in, reinterpret_cast<c32 *>(d_out),
				   n_in, n_out, p, q, tm, m, n_tiles, parts, reinterpret_cast<const uint32_t *>(d_hist_in),
				   reinterpret_cast<uint32_t *>(d_hist_out));
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
