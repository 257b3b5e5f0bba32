// trx_tx_frontend.hip -- the multi-ARFCN transmit front end (gfx950, wave64), the mirror image of the receive front end
// in trx_rx_frontend.hip:
//   * Synthesis(4, blockLen, 16)::rotate       Synthesis.cpp:66-104: forward 4-point DFT across the 4 paths, 16-tap path
//                                              filters with carried history, interleave out[4t + k] = y_k[t] (:39-50)
//   * RadioInterfaceMulti::pushBuffer()        radioInterfaceMulti.cpp:316-362: Resampler(p, q, 16)::rotate of every active
//                                              path, Synthesis::rotate, convert_float_short -- in one pass
// Sums in the reference's generic-C order (product, then add, k ascending; compiled with -ffp-contract=off), the 4-point DFT
// with the exact +-1 / +-j butterflies of channelize_kernel.  Inactive paths are real zeros inside the butterflies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trx_tables.h"
#include "../../include/trxhip.h"
#include "trx_launch.h"

typedef float2 c32;
typedef float tx_v2f __attribute__((ext_vector_type(2)));

#define TX_TPB 256
#define TX_H 16                         // Synthesis / Resampler filter length (hLen)
#define TX_J 4                          // output times per thread in the path filters
#define TX_PHA 264                      // entries per phase array of the path-filter input: >= (TX_TPB * TX_J + 15 + 3) / 4
#define TX_NSP 1408                     // staged low-rate samples per channel and tile (fused kernel): 3 * 1408 = 4 * 4 * 264

__device__ __forceinline__ tx_v2f tx_lds(const c32 *p)
{
	typedef const volatile tx_v2f __attribute__((address_space(3))) *lds_ptr;
	return *(lds_ptr)(p);
}

// Workgroup barrier for LDS hand-offs only (as fe_lds_barrier, trx_rx_frontend.hip): waits for this wave's LDS operations,
// not for its global loads and stores, so the next tile's prefetch and this tile's output stores stay in flight.
__device__ __forceinline__ void tx_lds_barrier()
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// forward 4-point DFT of one time step (cxvec_fft, reverse = 0): the butterflies of channelize_kernel
__device__ __forceinline__ void tx_dft4(c32 x0, c32 x1, c32 x2, c32 x3, c32 y[4])
{
	const c32 t1 = make_float2(x0.x + x2.x, x0.y + x2.y);
	const c32 t2 = make_float2(x0.x - x2.x, x0.y - x2.y);
	const c32 t3 = make_float2(x1.x + x3.x, x1.y + x3.y);
	const c32 t4 = make_float2(x1.x - x3.x, x1.y - x3.y);
	y[0] = make_float2(t1.x + t3.x, t1.y + t3.y);
	y[1] = make_float2(t2.x + t4.y, t2.y - t4.x);                    // t2 - j*t4
	y[2] = make_float2(t1.x - t3.x, t1.y - t3.y);
	y[3] = make_float2(t2.x - t4.y, t2.y + t4.x);                    // t2 + j*t4
}

__device__ __forceinline__ uint32_t tx_s16(c32 v, float scale)    // convert_float_short: (short)(x * scale) per component
{
	return (uint32_t)(uint16_t)(int16_t)(int)(v.x * scale) | ((uint32_t)(uint16_t)(int16_t)(int)(v.y * scale) << 16);
}

// The path filters and the interleaved store of TX_J consecutive output times per thread (times t0 + 4 thr .. + 3).
//   ys[k][j & 3][j >> 2] = DFT bin k at time t0 - 15 + j    (phase layout: lane l's window starts at entry l of every phase,
//                                                            so consecutive lanes read consecutive 8-byte entries)
//   y_k[t] = sum_i Y_k[t - 15 + i] * sub_k[i]               (convolve_real, Synthesis.cpp:90-96; sub_k = chan_taps[k])
//   out[4 t + k] = y_k[t]                                   (interleave, Synthesis.cpp:39-50)
__device__ __forceinline__ void tx_filter_store(const c32 (*ys)[4][TX_PHA], const float (*taps)[TX_H], int thr, size_t t0,
						size_t n_times, c32 *__restrict__ out_cf32, uint32_t *__restrict__ out_s16, float scale)
{
	const size_t t = t0 + (size_t)TX_J * thr;
	if (t >= n_times)
		return;
	const size_t w = 4 * t;                                               // first wideband sample of the thread
	const bool full = t + TX_J <= n_times;
	const bool vec_cf32 = (reinterpret_cast<uintptr_t>(out_cf32) & 15) == 0, vec_s16 = (reinterpret_cast<uintptr_t>(out_s16) & 7) == 0;
	// two paths at a time: their outputs of one time are 16 contiguous bytes (cf32) / 8 (int16), stored as soon as they are done
#pragma unroll
	for (int kp = 0; kp < 4; kp += 2) {
		c32 y[TX_J][2];
#pragma unroll
		for (int kk = 0; kk < 2; kk++) {
			const int k = kp + kk;
			tx_v2f x[TX_J + TX_H - 1];
#pragma unroll
			for (int v = TX_J + TX_H - 2; v >= 0; v--)
				x[v] = tx_lds(&ys[k][v & 3][thr + (v >> 2)]);
			tx_v2f acc[TX_J];
#pragma unroll
			for (int j = 0; j < TX_J; j++)
				acc[j] = (tx_v2f){ 0.0f, 0.0f };
#pragma unroll
			for (int i = 0; i < TX_H; i++) {
				const float h = taps[k][i];
#pragma unroll
				for (int j = 0; j < TX_J; j++)
					acc[j] = acc[j] + x[j + i] * (tx_v2f){ h, h };         // product, then sum
			}
#pragma unroll
			for (int j = 0; j < TX_J; j++)
				y[j][kk] = make_float2(acc[j].x, acc[j].y);
			__builtin_amdgcn_sched_barrier(0);                            // one path's window in registers at a time
		}
#pragma unroll
		for (int j = 0; j < TX_J; j++) {
			if (!full && t + j >= n_times)                                // the stream's last, partial group of times
				break;
			const size_t o = w + 4 * j + kp;
			if (out_cf32) {
				if (vec_cf32)
					*reinterpret_cast<float4 *>(out_cf32 + o) = make_float4(y[j][0].x, y[j][0].y, y[j][1].x, y[j][1].y);
				else
					out_cf32[o] = y[j][0], out_cf32[o + 1] = y[j][1];
			}
			if (out_s16) {
				if (vec_s16)
					*reinterpret_cast<uint2 *>(out_s16 + o) = make_uint2(tx_s16(y[j][0], scale), tx_s16(y[j][1], scale));
				else
					out_s16[o] = tx_s16(y[j][0], scale), out_s16[o + 1] = tx_s16(y[j][1], scale);
			}
		}
	}
}

__device__ __forceinline__ void tx_load_chan_taps(float (*taps)[TX_H], const trx_tables *__restrict__ tab)
{
	if (threadIdx.x < 4 * TX_H)
		taps[threadIdx.x / TX_H][threadIdx.x % TX_H] = tab->chan_taps[threadIdx.x / TX_H][threadIdx.x % TX_H];
}

// ------------------------------------------------------------------------------------------------
// Synthesis(4, ., 16)::rotate over a continuous stream of the 4 path inputs (Synthesis::inputBuffer(c) = row c at
// in + c * in_stride).  Block boundaries of the reference are invisible in the maths: the history carry equals one
// continuous stream.  hist == NULL: zero history before time 0 (a fresh Synthesis); otherwise the rows' 15 samples before
// time 0 at hist[c * 16 + 0 .. 14].  A workgroup takes tiles of TX_TPB * TX_J output times: per tile the DFT of the times
// [t0 - 15, t0 + 1024) into LDS, then the path filters.
// ------------------------------------------------------------------------------------------------
#define SY_TILE (TX_TPB * TX_J)

__global__ void __launch_bounds__(TX_TPB)
synthesis_kernel(const c32 *__restrict__ in, size_t in_stride, const c32 *__restrict__ hist, c32 *__restrict__ out_cf32,
		 uint32_t *__restrict__ out_s16, float scale, size_t n_times, const trx_tables *__restrict__ tab)
{
	__shared__ __attribute__((aligned(16))) c32 ys[4][4][TX_PHA];
	__shared__ float taps[4][TX_H];
	tx_load_chan_taps(taps, tab);
	const int thr = threadIdx.x;
	const size_t n_tiles = (n_times + SY_TILE - 1) / SY_TILE;
	for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const size_t t0 = tile * SY_TILE;
		__syncthreads();                                                  // (the previous tile's windows are read)
		for (int j = thr; j < SY_TILE + TX_H - 1; j += TX_TPB) {
			const long long u = (long long)t0 - (TX_H - 1) + j;
			c32 x[4];
#pragma unroll
			for (int c = 0; c < 4; c++) {
				x[c] = make_float2(0.0f, 0.0f);
				if (u < 0) {
					if (hist)
						x[c] = hist[c * 16 + (TX_H - 1) + u];
				} else if ((size_t)u < n_times) {
					x[c] = in[c * in_stride + (size_t)u];
				}
			}
			c32 y[4];
			tx_dft4(x[0], x[1], x[2], x[3], y);
#pragma unroll
			for (int k = 0; k < 4; k++)
				ys[k][j & 3][j >> 2] = y[k];
		}
		__syncthreads();
		tx_filter_store(ys, taps, thr, t0, n_times, out_cf32, out_s16, scale);
	}
}

extern "C" int trx_launch_synthesize(const float *d_in, size_t in_stride, const void *d_hist, float *d_out_cf32, int16_t *d_out_s16,
				     float scale, size_t n_times, const trx_tables *d_tab, hipStream_t stream)
{
	if (n_times == 0)
		return 0;
	size_t blocks = (n_times + SY_TILE - 1) / SY_TILE;
	if (blocks > 1024) blocks = 1024;
	hipLaunchKernelGGL(synthesis_kernel, dim3((unsigned)blocks), dim3(TX_TPB), 0, stream, reinterpret_cast<const c32 *>(d_in),
			   in_stride, reinterpret_cast<const c32 *>(d_hist), reinterpret_cast<c32 *>(d_out_cf32),
			   reinterpret_cast<uint32_t *>(d_out_s16), scale, n_times, d_tab);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// The last hn samples of every row -> hist[c * hs + 0 .. hn - 1] (a chunk shorter than hn shifts the old history).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TX_TPB)
tx_save_hist_kernel(const c32 *__restrict__ x, size_t n, size_t stride, c32 *__restrict__ hist, int hn, int hs)
{
	const int t = threadIdx.x, c = blockIdx.x;
	const bool on = t < hn;
	c32 v = make_float2(0.0f, 0.0f);
	if (on) {
		const long long s = (long long)n - hn + t;
		v = (s >= 0) ? x[c * stride + (size_t)s] : hist[c * hs + t + (int)n];
	}
	__syncthreads();
	if (on)
		hist[c * hs + t] = v;
}

extern "C" int trx_launch_tx_save_hist(const float *d_x, size_t n, size_t stride, int n_chan, void *d_hist, int hn, int hs,
				       hipStream_t stream)
{
	if (hn > TX_TPB || hn > hs)
		return TRXHIP_EINVAL;
	hipLaunchKernelGGL(tx_save_hist_kernel, dim3((unsigned)n_chan), dim3(TX_TPB), 0, stream, reinterpret_cast<const c32 *>(d_x), n,
			   stride, reinterpret_cast<c32 *>(d_hist), hn, hs);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// ------------------------------------------------------------------------------------------------
// RadioInterfaceMulti::pushBuffer() in one pass: Resampler(p, q, 16) of every active path, Synthesis(4, ., 16), int16.
// The active paths and their logical channels (radioInterfaceMulti.cpp:92-124, :214-231), slot c of CHANS:
//   1 chan: path 0 <- lchan 0      2 chans: 0 <- 0, 3 <- 1      3 chans: 0 <- 1, 1 <- 0, 3 <- 2
// Path 2 is never active: its row is zero (Synthesis::resetBuffer) and enters the butterflies as 0.0f.
// A workgroup owns a run of tiles of tm resampler periods = TT = p*tm channel-rate times (1008 for 48/65).  Per tile:
//   1. the active channels' low-rate samples [n0 - H, n0 + q*tm) go to LDS (prefetched into registers while the previous
//      tile is computed), H = 15 + ceil(15 q / p): enough for the 15 channel-rate times before the tile, which are
//      recomputed, not carried; at the stream's start samples n < 0 come from the carried input history (zeros when fresh);
//   2. every thread resamples 4 channel-rate times of all active paths (out[I] = sum_k in[n - 15 + k] * part[path][k],
//      n = q I / p, path = q I % p: Resampler.cpp:131-168) and takes their 4-point DFT, in registers;
//   3. behind a barrier the DFT bins go to LDS over the staged samples, in the path filters' phase layout;
//   4. the path filters and the store (tx_filter_store).
// The channel-rate rows never touch HBM.  Results are bit-identical to resample_kernel + synthesis_kernel.
// ------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int tx_slot_pchan(int chans, int c) { return chans == 3 ? (c == 2 ? 3 : c) : (c == 1 ? 3 : 0); }
__host__ __device__ constexpr int tx_slot_lchan(int chans, int c) { return chans == 3 ? (c == 0 ? 1 : (c == 1 ? 0 : 2)) : c; }

template <int CHANS>
__global__ void __launch_bounds__(TX_TPB)
tx_frontend_fused_kernel(const c32 *__restrict__ in, size_t in_stride, size_t n_in, const c32 *__restrict__ hist, int hl,
			 c32 *__restrict__ out_cf32, uint32_t *__restrict__ out_s16, float scale, size_t n_times, int p, int q,
			 int tm, int H, size_t n_tiles, const float *__restrict__ parts, const trx_tables *__restrict__ tab)
{
	__shared__ __attribute__((aligned(16))) c32 smem[4 * 4 * TX_PHA];       // xs[CHANS][TX_NSP], then ys[4][4][TX_PHA]
	__shared__ float taps[4][TX_H];
	extern __shared__ float rtaps[];                                      // resampler taps [p][17]: one base address per path,
	                                                                      // 17 dwords apart (different paths, different banks)
	static_assert(CHANS * TX_NSP <= 4 * 4 * TX_PHA, "the DFT bins alias the staged samples");
	c32 *const xs = smem;
	const c32 (*const ys)[4][TX_PHA] = reinterpret_cast<const c32 (*)[4][TX_PHA]>(smem);
	c32 (*const ysw)[4][TX_PHA] = reinterpret_cast<c32 (*)[4][TX_PHA]>(smem);
	const int thr = threadIdx.x;
	tx_load_chan_taps(taps, tab);
	for (int i = thr; i < p * TX_H; i += TX_TPB)
		rtaps[(i / TX_H) * (TX_H + 1) + (i % TX_H)] = parts[i];
	const int TT = p * tm, NU = TT + (TX_H - 1), NS = H + q * tm;
	// (staged sample, filter path) of this thread's channel-rate times j = thr + 256 i (time t0 - 15 + j): the same in
	// every tile, because t0 is a multiple of p.  With K = ceil(15 / p), n = floor(q (j - 15) / p) = floor(q (j + pK - 15) / p) - qK.
	int item[4];
	{
		const int K = (TX_H - 1 + p - 1) / p, off = p * K - (TX_H - 1);
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int j = thr + TX_TPB * i;
			const int a = q * (j + off);
			item[i] = (j < NU) ? (((a / p - q * K - (TX_H - 1) + H) << 8) | (a % p)) : -1;
		}
	}
	const size_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
	const size_t tile_lo = (size_t)blockIdx.x * per_wg;
	const size_t tile_hi = (tile_lo + per_wg < n_tiles) ? tile_lo + per_wg : n_tiles;
	// staged entry idx = i * 256 + thr of channel slot c: the same thread and register for every tile
	constexpr int NPRE = (TX_NSP + TX_TPB - 1) / TX_TPB;
	c32 pre[CHANS][NPRE];
	auto prefetch = [&](size_t tile) {
		// Everything that depends on the tile is wave-uniform: the first staged sample s0 and the channels' base pointers;
		// a thread adds its 32-bit entry index.  A tile inside the stream takes unconditional loads (a branch of its own).
		const long long s0 = (long long)tile * q * tm - H;                    // low-rate sample of staged entry 0
		const bool inside = s0 >= 0 && (unsigned long long)s0 + NS <= n_in;
#pragma unroll
		for (int c = 0; c < CHANS; c++) {
			const int l = tx_slot_lchan(CHANS, c);
			const c32 *const base = in + l * in_stride + s0;                   // (dereferenced for samples inside the stream only)
#pragma unroll
			for (int i = 0; i < NPRE; i++) {
				const int idx = i * TX_TPB + thr;
				c32 v = make_float2(0.0f, 0.0f);
				if (inside) {
					if (idx < NS)
						v = base[idx];
				} else if (idx < NS) {
					const long long n = s0 + idx;
					if (n < 0)
						v = hist[l * hl + hl + n];                             // carried history: samples -hl .. -1
					else if ((unsigned long long)n < n_in)
						v = base[idx];
				}
				pre[c][i] = v;
			}
		}
	};
	if (tile_lo < tile_hi)
		prefetch(tile_lo);
	for (size_t tile = tile_lo; tile < tile_hi; tile++) {
		tx_lds_barrier();                                                 // (the previous tile's DFT bins are read)
#pragma unroll
		for (int c = 0; c < CHANS; c++)
#pragma unroll
			for (int i = 0; i < NPRE; i++) {
				const int idx = i * TX_TPB + thr;
				if (idx < TX_NSP)
					xs[c * TX_NSP + idx] = pre[c][i];
			}
		tx_lds_barrier();

		// ---- resampler + DFT: channel-rate times j = thr + 256 i of the tile
		c32 Y[4][4];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			int it = item[i];
			asm volatile("" : "+v"(it));                                  // (opaque per tile: addresses formed here, not
			if (it < 0)                                                   // hoisted out of the tile loop into 16 registers each)
				continue;
			const int s = it >> 8, path = it & 0xff;
			float h[TX_H];
#pragma unroll
			for (int k = 0; k < TX_H; k++)
				h[k] = rtaps[path * (TX_H + 1) + k];
			c32 r[4] = { make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f) };
#pragma unroll
			for (int c = 0; c < CHANS; c++) {
				const c32 *xp = xs + c * TX_NSP + s;
				tx_v2f acc = { 0.0f, 0.0f };
#pragma unroll
				for (int k = 0; k < TX_H; k++)
					acc = acc + tx_lds(xp + k) * (tx_v2f){ h[k], h[k] };      // product, then sum, k ascending
				r[tx_slot_pchan(CHANS, c)] = make_float2(acc.x, acc.y);
				__builtin_amdgcn_sched_barrier(0);                        // one channel's window in registers at a time
			}
			tx_dft4(r[0], r[1], r[2], r[3], Y[i]);
			__builtin_amdgcn_sched_barrier(0);                            // one time step's taps in registers at a time
		}
		if (tile + 1 < tile_hi)                                            // (here, not before the resampler: registers it needs)
			prefetch(tile + 1);
		tx_lds_barrier();                                                 // every staged sample is read: the area is free
#pragma unroll
		for (int i = 0; i < 4; i++) {
			if (item[i] < 0)
				continue;
			const int j = thr + TX_TPB * i;
#pragma unroll
			for (int k = 0; k < 4; k++)
				ysw[k][j & 3][j >> 2] = Y[i][k];
		}
		tx_lds_barrier();

		// ---- path filters + store
		int tc = thr;
		asm volatile("" : "+v"(tc));                                      // (opaque per tile, as above)
		if (TX_J * tc < TT)
			tx_filter_store(ys, taps, tc, tile * (size_t)TT, n_times, out_cf32, out_s16, scale);
	}
}

// periods per tile of the fused kernel, or 0 when the geometry does not fit its tiles
extern "C" int trx_tx_fused_tm(int p, int q)
{
	if (p < 1 || q < 1 || p > 128)
		return 0;
	const int H = (TX_H - 1) + ((TX_H - 1) * q + p - 1) / p;
	for (int tm = (SY_TILE - (TX_H - 1)) / p; tm >= 1; tm--)
		if ((p * tm) % TX_J == 0 && H + q * tm <= TX_NSP)
			return tm;
	return 0;
}

// fused Tx front end; returns 1 when the geometry does not fit (the caller then runs the separate kernels), 0 / TRXHIP_EIO
// otherwise.  d_hist: chans x hl complex64, the low-rate samples -hl .. -1 of every logical channel (hl >= 15 + ceil(15 q / p)).
extern "C" int trx_launch_tx_frontend_fused(const float *d_in, size_t in_stride, size_t n_in, const void *d_hist, int hl,
					    float *d_out_cf32, int16_t *d_out_s16, float scale, int chans, int p, int q,
					    const float *d_parts, const trx_tables *d_tab, hipStream_t stream)
{
	const int tm = trx_tx_fused_tm(p, q);
	const int H = (TX_H - 1) + ((TX_H - 1) * q + p - 1) / p;
	if (tm == 0 || hl < H || chans < 1 || chans > 3 || (n_in % (size_t)q) != 0)
		return 1;
	const size_t n_times = n_in / q * p;
	if (n_times == 0)
		return 0;
	const size_t n_tiles = (n_times + (size_t)p * tm - 1) / ((size_t)p * tm);
	const size_t gx = n_tiles < 1024 ? n_tiles : 1024;                    // 4 workgroups per CU, each a run of tiles
	const size_t lds = (size_t)p * (TX_H + 1) * sizeof(float);
	const c32 *in = reinterpret_cast<const c32 *>(d_in);
	const c32 *hist = reinterpret_cast<const c32 *>(d_hist);
	c32 *oc = reinterpret_cast<c32 *>(d_out_cf32);
	uint32_t *os = reinterpret_cast<uint32_t *>(d_out_s16);
	switch (chans) {
	case 1:
		hipLaunchKernelGGL(tx_frontend_fused_kernel<1>, dim3((unsigned)gx), dim3(TX_TPB), lds, stream, in, in_stride, n_in, hist, hl,
				   oc, os, scale, n_times, p, q, tm, H, n_tiles, d_parts, d_tab);
		break;
	case 2:
		hipLaunchKernelGGL(tx_frontend_fused_kernel<2>, dim3((unsigned)gx), dim3(TX_TPB), lds, stream, in, in_stride, n_in, hist, hl,
				   oc, os, scale, n_times, p, q, tm, H, n_tiles, d_parts, d_tab);
		break;
	default:
		hipLaunchKernelGGL(tx_frontend_fused_kernel<3>, dim3((unsigned)gx), dim3(TX_TPB), lds, stream, in, in_stride, n_in, hist, hl,
				   oc, os, scale, n_times, p, q, tm, H, n_tiles, d_parts, d_tab);
		break;
	}
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
