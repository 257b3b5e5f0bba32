// trx_rx_frontend.hip -- the receive front end per logical channel (gfx950, wave64):
//   * rx_frontend_chans_kernel<NACT>   RadioInterfaceMulti::pullBuffer (radioInterfaceMulti.cpp:237-314) for 1..3 ARFCNs:
//                                      Channelizer(4, ., 16)::rotate + Resampler(p, q, 16)::rotate on the ACTIVE filterbank
//                                      paths only, rows handed over by logical channel
//   * rx_resamp_s16_kernel             RadioInterfaceResamp::pullBuffer (radioInterfaceResamp.cpp:156-193): convert_short_float +
//                                      Resampler(p, q, 16)::rotate of one int16 channel in one pass
// The four-row object (trxhip_rx_frontend_create) keeps its own kernels in trx_aux_kernels.hip; the small helpers both files
// need are repeated here so that that file stays the code it was.  Sums run in the reference's generic-C order, product
// then add (compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trx_tables.h"
#include "../../include/trxhip.h"
#include "trx_launch.h"

typedef float2 c32;

#define RX_M 4                          // filterbank paths
#define RX_H 16                         // taps per path filter
#define RX_TPB 256
#define RX_J 4                          // channel-rate times per thread
#define RX_PHA 264                      // entries per phase array of the wideband staging (trx_aux_kernels.hip, CH_PHA)
#define RX_CS 1056                      // entries per channel row in the aliased LDS array (>= q*tm + 15, <= 4 * RX_PHA)

typedef float rx_v2f __attribute__((ext_vector_type(2)));
template <int HI>
__device__ __forceinline__ rx_v2f rx_mul_tap(rx_v2f x, rx_v2f hpair)
{
	rx_v2f r;                          // x * (tap HI of the pair): one v_pk_mul_f32, the tap picked by op_sel
	if (HI)
		asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(x), "v"(hpair));
	else
		asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(x), "v"(hpair));
	return r;
}

// one complex sample from LDS as its own ds_read_b64 (volatile only stops the merge into a ds_read2_b64)
__device__ __forceinline__ rx_v2f rx_lds(const c32 *p)
{
	typedef const volatile rx_v2f __attribute__((address_space(3))) *lds_ptr;
	return *(lds_ptr)(p);
}

// workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations, not for its global loads and stores
__device__ __forceinline__ void rx_lds_barrier()
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// filterbank path of logical channel l with nact channels (radioInterfaceMulti.cpp:92-124, :214-231)
__host__ __device__ constexpr int rx_pchan(int nact, int l)
{
	return nact == 1 ? 0 : (nact == 2 ? (l == 0 ? 0 : 3) : (l == 0 ? 1 : (l == 1 ? 0 : 3)));
}

// bin pc of the forward 4-point DFT from the radix-2 terms, the expressions of frontend_fused_kernel / channelize_kernel
__device__ __forceinline__ c32 rx_bin(int pc, c32 t1, c32 t2, c32 t3, c32 t4)
{
	switch (pc) {
	case 0: return make_float2(t1.x + t3.x, t1.y + t3.y);
	case 1: return make_float2(t2.x + t4.y, t2.y - t4.x);              // t2 - j*t4
	case 2: return make_float2(t1.x - t3.x, t1.y - t3.y);
	default: return make_float2(t2.x - t4.y, t2.y + t4.x);             // t2 + j*t4
	}
}

// ------------------------------------------------------------------------------------------------
// frontend_fused_kernel (trx_aux_kernels.hip: read its comments, every one records a measured trap) for NACT logical
// channels.  Per tile of tm resampler periods = q*tm channel-rate times:
//   1. the wideband steps [T0 - 30, T0 + q*tm) are staged as fp32 in the channelizer's 4-phase layout -- all four path
//      filters feed every DFT bin, so staging and filtering do not shrink;
//   2. of the 4-point DFT only the NACT active bins are formed, from the same t1..t4 with the same expressions;
//   3. NACT channel rows are parked in LDS, row l = logical channel l = filterbank path rx_pchan(NACT, l);
//   4. NACT rows are resampled: NACT sum chains per output position in the owner loop, residue items for NACT rows;
//   5. row l is stored at out + l * out_stride; the carried channel history is [NACT][16], logical order.
// Every output is the same products and sums in the same order as the four-row kernel's: row l equals its row
// rx_pchan(NACT, l) bit for bit (tests/test_gpu_rx_frontend_chans.py).  Per 192-step block at 65/48 it moves
// 3072 + NACT * 2080 B instead of 3072 + 8320.
// ------------------------------------------------------------------------------------------------
template <int NACT>
__global__ void __launch_bounds__(RX_TPB) __attribute__((amdgpu_waves_per_eu(4, 4)))
rx_frontend_chans_kernel(const uint4 *__restrict__ in4, size_t n_total, c32 *__restrict__ out, size_t n_out, size_t out_stride,
			 int p, int q, int tm, int m, size_t n_tiles, const float *__restrict__ parts,
			 const trx_tables *__restrict__ tab, const uint4 *__restrict__ wide_hist,
			 const c32 *__restrict__ chan_hist_in, c32 *__restrict__ chan_hist_out)
{
	__shared__ __attribute__((aligned(16))) c32 xs[RX_M][4][RX_PHA];     // wideband staging, then cs[NACT][RX_CS]
	__shared__ __attribute__((aligned(16))) float taps[RX_M][RX_H];
	extern __shared__ __attribute__((aligned(16))) char rx_smem[];        // resampler taps [16][p + 1], then the items
	float *rtaps = reinterpret_cast<float *>(rx_smem);
	c32 *const cs = &xs[0][0][0];
	static_assert(NACT >= 1 && NACT <= 3, "1..3 logical channels");
	static_assert(NACT * RX_CS <= RX_M * 4 * RX_PHA, "the channel samples alias the wideband staging");
	const int t = threadIdx.x;
	const int pst = p + 1;
	if (t < RX_M * RX_H)
		taps[t / RX_H][t % RX_H] = tab->chan_taps[t / RX_H][t % RX_H];
	for (int i = t; i < p * 16; i += RX_TPB)
		rtaps[(i % 16) * pst + (i / 16)] = parts[i];
	const int tile_in = q * tm, tile_out = p * tm;
	const int n_stage = tile_in + 30;                                    // wideband steps staged per tile (<= 4 * RX_TPB)
	const int n_cs = tile_in + 15;                                       // channel-rate times computed per tile
	const int S = p * m, iters = tm / m;                                 // thread t owns the outputs t, t + S, ...: one filter path
	const bool owner = t < S;
	const unsigned qt = (unsigned)q * (unsigned)t;
	const int n_t0 = (int)(qt / (unsigned)p), path_t0 = (int)(qt % (unsigned)p);
	const int nstep = q * m;

	// (first sample, filter path) of this thread's output positions and the residue items S - 256 .. S - 1 of every step and
	// row: functions of the thread / the item alone, worked out once and parked in LDS (kept in registers across the tile
	// loop they were what the allocator spilled in the four-row kernel)
	int *const thr_item = reinterpret_cast<int *>(rtaps + 16 * pst);
	thr_item[t] = (n_t0 << 16) | path_t0;
	const int n_res = (S - RX_TPB) * iters * NACT;
	int2 *const res_item = reinterpret_cast<int2 *>(rtaps + 16 * pst + RX_TPB);
	for (int idx = t; idx < n_res; idx += RX_TPB) {
		const int nres0 = S - RX_TPB;
		const int c = idx / (nres0 * iters), r = idx % (nres0 * iters);
		const int oi = RX_TPB + r % nres0 + S * (r / nres0);
		const unsigned qi = (unsigned)q * (unsigned)oi;
		res_item[idx] = make_int2((c << 16) | (int)(qi / (unsigned)p), (oi << 16) | (int)(qi % (unsigned)p));
	}
	const size_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
	const size_t tile_lo = (size_t)blockIdx.x * per_wg;
	const size_t tile_hi = (tile_lo + per_wg < n_tiles) ? tile_lo + per_wg : n_tiles;
	uint4 pre[4];
	auto prefetch = [&](size_t tile) {
		// staged step j (0 <= j < n_stage) is wideband step t0 + j; everything that depends on the tile is wave-uniform: the
		// range [jlo, jhi) of steps inside the stream and a base pointer; a thread adds its 32-bit j
		const long long t0 = (long long)tile * tile_in - 30;               // first staged wideband step
		const long long lo = t0 < 0 ? -t0 : 0, hi = (long long)n_total - t0;
		const int jlo = (int)(lo < n_stage ? lo : n_stage), jhi = (int)(hi < 0 ? 0 : (hi < n_stage ? hi : n_stage));
		const uint4 *const base = in4 + t0;                                 // (dereferenced for jlo <= j < jhi only)
		const int hoff = (int)((RX_H - 1) + t0);                            // tile 0: steps -15 .. -1 come from the carried history
		if (jlo == 0 && jhi == n_stage) {
			// a tile inside the stream: four unconditional loads in a wave-uniform branch of their own (as one arm of a
			// per-lane if the compiler put an s_waitcnt vmcnt(0) between the arms)
			unsigned tt = (unsigned)t;                                       // opaque per tile: cheaper to recompute than to keep
			asm volatile("" : "+v"(tt));
			const unsigned jmax = (unsigned)n_stage - 1u;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const unsigned j = (unsigned)(i * RX_TPB) + tt;
				pre[i] = base[j < jmax ? j : jmax];                            // (j >= n_stage is never staged)
			}
			return;
		}
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int j = i * RX_TPB + t;
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
		rx_lds_barrier();                                                   // (the previous tile's channel samples are done with)
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int j = i * RX_TPB + t;
			if (j < n_stage) {
				const uint32_t w[4] = { pre[i].x, pre[i].y, pre[i].z, pre[i].w };
#pragma unroll
				for (int n = 0; n < RX_M; n++)                                 // path M-1-n <- wideband sample n of the time step
					xs[RX_M - 1 - n][j & 3][j >> 2] = make_float2((float)(int16_t)(w[n] & 0xffffu), (float)(int16_t)(w[n] >> 16));
			}
		}
		rx_lds_barrier();

		// ---- channelizer: channel-rate times u = 4t .. 4t+3 of the tile (time T0 - 15 + u); tap k of output u is staged step u + k
		c32 o[NACT][RX_J];
		const bool active = RX_J * t < n_cs;
		if (active) {
			c32 yp[RX_J][RX_M];
#pragma unroll
			for (int pp = 0; pp < RX_M; pp++) {
				// the window is requested LAST sample first (one s_waitcnt per path: LDS returns in order); a pair of taps is one
				// broadcast 8-byte read requested one pair AHEAD of its use; products of tap k alternate with the sums of tap k - 1
				rx_v2f x[RX_J + RX_H - 1];
#pragma unroll
				for (int v = RX_J + RX_H - 2; v >= 0; v--)
					x[v] = rx_lds(&xs[pp][v & 3][t + (v >> 2)]);
				typedef const volatile rx_v2f __attribute__((address_space(3))) *lds_tap;
				const lds_tap g2 = (lds_tap)(&taps[pp][0]);
				rx_v2f acc[RX_J], pr[RX_J];
#pragma unroll
				for (int j = 0; j < RX_J; j++)
					acc[j] = pr[j] = (rx_v2f){ 0.0f, 0.0f };
				rx_v2f gcur = g2[0];
#pragma unroll
				for (int kp = 0; kp < RX_H / 2; kp++) {
					rx_v2f gnext = gcur;
					if (kp + 1 < RX_H / 2)
						gnext = g2[kp + 1];
#pragma unroll
					for (int kk = 0; kk < 2; kk++) {
						const int k = 2 * kp + kk;
#pragma unroll
						for (int j = 0; j < RX_J; j++) {
							const rx_v2f pn = kk ? rx_mul_tap<1>(x[j + k], gcur) : rx_mul_tap<0>(x[j + k], gcur);
							if (k > 0)
								acc[j] = acc[j] + pr[j];                               // product, then sum: tap k - 1
							pr[j] = pn;
							__builtin_amdgcn_sched_barrier(0);
						}
					}
					gcur = gnext;
				}
#pragma unroll
				for (int j = 0; j < RX_J; j++)
					acc[j] = acc[j] + pr[j];                                           // tap 15
#pragma unroll
				for (int j = 0; j < RX_J; j++) {
					asm volatile("" : "+v"(acc[j]));
					yp[j][pp] = make_float2(acc[j].x, acc[j].y);
				}
				__builtin_amdgcn_sched_barrier(0);
			}
#pragma unroll
			for (int j = 0; j < RX_J; j++) {                                   // the active bins of the forward 4-point DFT
				const c32 t1 = make_float2(yp[j][0].x + yp[j][2].x, yp[j][0].y + yp[j][2].y);
				const c32 t2 = make_float2(yp[j][0].x - yp[j][2].x, yp[j][0].y - yp[j][2].y);
				const c32 t3 = make_float2(yp[j][1].x + yp[j][3].x, yp[j][1].y + yp[j][3].y);
				const c32 t4 = make_float2(yp[j][1].x - yp[j][3].x, yp[j][1].y - yp[j][3].y);
#pragma unroll
				for (int l = 0; l < NACT; l++)
					o[l][j] = rx_bin(rx_pchan(NACT, l), t1, t2, t3, t4);
			}
		}
		if (tile + 1 < tile_hi)                                            // (here, not before the filters: 16 registers they need)
			prefetch(tile + 1);
		rx_lds_barrier();                                                   // every window has been read: the staging area is free
		if (active) {
#pragma unroll
			for (int l = 0; l < NACT; l++) {
				float4 *dst = reinterpret_cast<float4 *>(cs + l * RX_CS + RX_J * t);
				dst[0] = make_float4(o[l][0].x, o[l][0].y, o[l][1].x, o[l][1].y);
				dst[1] = make_float4(o[l][2].x, o[l][2].y, o[l][3].x, o[l][3].y);
			}
		}
		if (tile == 0) {                                                   // the stream's first tile: times -15 .. -1 are the carried history
			rx_lds_barrier();
			if (t < NACT * 15)
				cs[(t / 15) * RX_CS + (t % 15)] = chan_hist_in ? chan_hist_in[(t / 15) * 16 + (t % 15)] : make_float2(0.0f, 0.0f);
		}
		rx_lds_barrier();

		// ---- resampler: cs[l][j] = logical channel l at time T0 - 15 + j
		const size_t o0 = tile * (size_t)tile_out;
		if (owner) {
			// this thread's 16 taps (path (q t) mod p), re-read from LDS per tile; all NACT rows of an output position per pass:
			// NACT independent sum chains over the same taps and offsets, each still k = 0..15, product then add
			typedef const volatile int __attribute__((address_space(3))) *lds_int;
			int tl = t;                                                     // (opaque: the address is one instruction to form per tile)
			asm volatile("" : "+v"(tl));
			const int ti = *(lds_int)(thr_item + tl);
			const int n_t = ti >> 16, path_t = ti & 0xffff;
			rx_v2f h2[8];
#pragma unroll
			for (int k = 0; k < 8; k++)
				h2[k] = (rx_v2f){ rtaps[(2 * k) * pst + path_t], rtaps[(2 * k + 1) * pst + path_t] };
			const c32 *xa = cs + n_t;
			c32 *const ob = out + o0;                                       // wave-uniform base; the thread adds a 32-bit offset
			unsigned yo = (unsigned)t;
			size_t oo = o0 + t;
			for (int it = 0; it < iters && oo < n_out; it++, oo += S, xa += nstep, yo += (unsigned)S) {
				rx_v2f acc[NACT], pr[NACT];
#pragma unroll
				for (int c = 0; c < NACT; c++)
					acc[c] = pr[c] = (rx_v2f){ 0.0f, 0.0f };
#pragma unroll
				for (int k0 = 0; k0 < 16; k0 += 4) {
					rx_v2f x[NACT][4];
#pragma unroll
					for (int k = 0; k < 4; k++)
#pragma unroll
						for (int c = 0; c < NACT; c++)
							x[c][k] = rx_lds(xa + c * RX_CS + k0 + k);
					// a tap at a time, software-pipelined: the rows' products of tap k (the LAST-read row first: its s_waitcnt
					// covers the others) alternate with the sums of tap k - 1
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const int kk = k0 + k;
#pragma unroll
						for (int c = NACT - 1; c >= 0; c--) {
							const rx_v2f pn = (kk & 1) ? rx_mul_tap<1>(x[c][k], h2[kk >> 1]) : rx_mul_tap<0>(x[c][k], h2[kk >> 1]);
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
		int tr = t;                                                         // (opaque, as above: the item's address is formed per tile)
		asm volatile("" : "+v"(tr));
		for (int idx = tr; idx < n_res; idx += RX_TPB) {                   // residues of every step, NACT rows
			const int2 e = res_item[idx];
			const int c = e.x >> 16, n = e.x & 0xffff, oi = e.y >> 16, path = e.y & 0xffff;
			if (o0 + oi >= n_out)
				continue;
			const c32 *xp = cs + c * RX_CS + n;
			rx_v2f acc = { 0.0f, 0.0f };                                    // product, then sum, k ascending, on both components at once
#pragma unroll
			for (int k = 0; k < 16; k++) {
				const float h = rtaps[k * pst + path];
				acc = acc + rx_lds(xp + k) * (rx_v2f){ h, h };
			}
			out[c * out_stride + o0 + oi] = make_float2(acc.x, acc.y);
		}
		if (chan_hist_out && tile + 1 == n_tiles && t < NACT * 15) {        // the call's last 15 channel samples of every row
			const long long j = (long long)n_total - (long long)tile * tile_in + (t % 15);   // time n_total - 15 + i -> cs index
			chan_hist_out[(t / 15) * 16 + (t % 15)] = cs[(t / 15) * RX_CS + j];
		}
	}
}

// tail of a chunk -> Channelizer::hist for the next one: the last 15 wideband time steps
__global__ void rx_save_wide_hist_kernel(const uint4 *__restrict__ in4, size_t n_total, uint4 *__restrict__ hist)
{
	const int t = threadIdx.x;
	if (t < RX_H - 1) {
		const long long ts = (long long)n_total - (RX_H - 1) + t;
		const uint4 v = (ts >= 0) ? in4[ts] : hist[t + (int)n_total];       // chunk shorter than the history: shift
		__syncthreads();
		hist[t] = v;
	}
}

// the per-channel front end; returns 1 when the geometry fits no tile (the caller then runs channelize_kernel and
// resample_kernel on the active rows), 0 / TRXHIP_EIO otherwise.  The conditions are trx_launch_frontend_fused's.
extern "C" int trx_launch_rx_frontend_chans(const int16_t *d_wide, float *d_out, size_t n_total, int chans, int p, int q,
					    size_t out_stride, const float *parts, const trx_tables *d_tab, void *d_wide_hist_io,
					    const void *d_chan_hist_in, void *d_chan_hist_out, hipStream_t stream)
{
	if (chans < 1 || chans > 3)
		return TRXHIP_EINVAL;
	const int m = (RX_TPB + p - 1) / p;                                  // outputs o and o + p*m share a filter path
	const int tm = (4 * RX_TPB - 30) / q / m * m;                         // periods per tile: staging fits 4 loads per thread
	const size_t n_out = n_total / q * p;
	if (tm < m || p * m < RX_TPB || p * m > 2 * RX_TPB || q * tm + 15 > RX_CS || (n_total % (size_t)q) != 0 || n_total < 30 || n_out == 0)
		return 1;
	const size_t n_tiles = (n_out + (size_t)p * tm - 1) / ((size_t)p * tm);
	const size_t gx = n_tiles < 1024 ? n_tiles : 1024;                   // 4 workgroups of 34 KB LDS per CU, each a run of tiles
	const size_t n_res = (size_t)(p * m - RX_TPB) * (tm / m) * chans;   // residue items per tile (60 at 65 / 48 and 3 channels)
	if (n_res > 1024)
		return 1;
	const size_t lds = (size_t)16 * (p + 1) * sizeof(float) + RX_TPB * sizeof(int) + n_res * sizeof(int2);
	const uint4 *in4 = reinterpret_cast<const uint4 *>(d_wide);
	c32 *out = reinterpret_cast<c32 *>(d_out);
	const uint4 *wh = reinterpret_cast<const uint4 *>(d_wide_hist_io);
	const c32 *hin = reinterpret_cast<const c32 *>(d_chan_hist_in);
	c32 *hout = reinterpret_cast<c32 *>(d_chan_hist_out);
	if (chans == 1)
		hipLaunchKernelGGL(rx_frontend_chans_kernel<1>, dim3((unsigned)gx), dim3(RX_TPB), lds, stream, in4, n_total, out, n_out,
				   out_stride, p, q, tm, m, n_tiles, parts, d_tab, wh, hin, hout);
	else if (chans == 2)
		hipLaunchKernelGGL(rx_frontend_chans_kernel<2>, dim3((unsigned)gx), dim3(RX_TPB), lds, stream, in4, n_total, out, n_out,
				   out_stride, p, q, tm, m, n_tiles, parts, d_tab, wh, hin, hout);
	else
		hipLaunchKernelGGL(rx_frontend_chans_kernel<3>, dim3((unsigned)gx), dim3(RX_TPB), lds, stream, in4, n_total, out, n_out,
				   out_stride, p, q, tm, m, n_tiles, parts, d_tab, wh, hin, hout);
	if (d_wide_hist_io)
		hipLaunchKernelGGL(rx_save_wide_hist_kernel, dim3(1), dim3(64), 0, stream, in4, n_total, reinterpret_cast<uint4 *>(d_wide_hist_io));
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
#define RXR_TILE_IN 3072

__device__ __forceinline__ c32 rx_cvt(uint32_t w)
{
	return make_float2((float)(int16_t)(w & 0xffffu), (float)(int16_t)(w >> 16));
}

template <bool VEC>
__global__ void __launch_bounds__(RX_TPB)
rx_resamp_s16_kernel(const uint32_t *__restrict__ in, c32 *__restrict__ out, size_t n_in, size_t n_out, int p, int q, int tm, int m,
		     size_t n_tiles, const float *__restrict__ parts, const uint32_t *__restrict__ hist_in, uint32_t *__restrict__ hist_out)
{
	extern __shared__ __attribute__((aligned(16))) char rxr_smem[];
	c32 *xs = reinterpret_cast<c32 *>(rxr_smem);                         // [16 + q*tm]
	const int tile_in = q * tm, tile_out = p * tm;
	float *taps = reinterpret_cast<float *>(xs + 16 + ((tile_in + 1) & ~1));   // [16][p + 1]
	const int pst = p + 1;
	const int t = threadIdx.x;
	for (int i = t; i < p * 16; i += RX_TPB)
		taps[(i % 16) * pst + (i / 16)] = parts[i];
	const int S = p * m, iters = tm / m;                                 // tm is a multiple of m (launcher); S >= 256 (p <= 128)
	const bool owner = t < S;
	const unsigned qt = (unsigned)q * (unsigned)t;
	const int n_t = (int)(qt / (unsigned)p), path_t = (int)(qt % (unsigned)p);
	rx_v2f h2[8];                                                        // this thread's 16 taps, in pairs
#pragma unroll
	for (int k = 0; k < 8; k++)
		h2[k] = owner ? (rx_v2f){ parts[path_t * 16 + 2 * k], parts[path_t * 16 + 2 * k + 1] } : (rx_v2f){ 0.0f, 0.0f };
	const int nstep = q * m;
	constexpr int NPRE = VEC ? RXR_TILE_IN / 4 / RX_TPB : RXR_TILE_IN / RX_TPB;   // tile_in <= RXR_TILE_IN
	constexpr int W = VEC ? 4 : 1;                                       // samples per load
	const size_t per_wg = (n_tiles + gridDim.x - 1) / gridDim.x;
	const size_t tile_lo = (size_t)blockIdx.x * per_wg;
	const size_t tile_hi = (tile_lo + per_wg < n_tiles) ? tile_lo + per_wg : n_tiles;
	uint32_t pre[NPRE * W], pre_h = 0u;
	auto prefetch = [&](size_t tile) {
		const size_t n0 = tile * (size_t)tile_in;                          // first input sample of the tile (VEC: a multiple of 4)
#pragma unroll
		for (int i = 0; i < NPRE; i++) {
			const int j = (i * RX_TPB + t) * W;
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
			const int j = (i * RX_TPB + t) * W;
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
				rx_v2f acc = { 0.0f, 0.0f };
#pragma unroll
				for (int k = 0; k < 16; k++) {
					const rx_v2f xv = rx_lds(xp + k);
					acc = acc + ((k & 1) ? rx_mul_tap<1>(xv, h2[k >> 1]) : rx_mul_tap<0>(xv, h2[k >> 1]));   // product, then sum
				}
				*yo = make_float2(acc.x, acc.y);
			}
		}
		// residues RX_TPB .. S-1 of every step: (S - RX_TPB) * iters outputs, taps from LDS
		const int nres = S - RX_TPB;
		for (int idx = t; idx < nres * iters; idx += RX_TPB) {
			const int o = RX_TPB + idx % nres + S * (idx / nres);
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
	const int m = (RX_TPB + p - 1) / p;                                  // outputs o and o + p*m share a filter path
	int tm = RXR_TILE_IN / q / m * m;                                    // periods per tile: a multiple of m
	if (tm < m) tm = m;
	if ((long long)q * tm > RXR_TILE_IN)
		return TRXHIP_EINVAL;                                            // the tile's registers and LDS
	const int tile_in = q * tm;
	const size_t n_tiles = (n_out + (size_t)p * tm - 1) / ((size_t)p * tm);
	const size_t gx = n_tiles < 1024 ? n_tiles : 1024;                   // 4 workgroups (<= 33 KB of LDS) per CU, each a run of tiles
	const size_t lds = (size_t)(16 + ((tile_in + 1) & ~1)) * sizeof(c32) + (size_t)16 * (p + 1) * sizeof(float);
	const uint32_t *in = reinterpret_cast<const uint32_t *>(d_in);
	const bool vec = (tile_in % 4) == 0 && (n_in % 4) == 0 && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
	if (vec)
		hipLaunchKernelGGL(rx_resamp_s16_kernel<true>, dim3((unsigned)gx), dim3(RX_TPB), lds, stream, in, reinterpret_cast<c32 *>(d_out),
				   n_in, n_out, p, q, tm, m, n_tiles, parts, reinterpret_cast<const uint32_t *>(d_hist_in),
				   reinterpret_cast<uint32_t *>(d_hist_out));
	else
		hipLaunchKernelGGL(rx_resamp_s16_kernel<false>, dim3((unsigned)gx), dim3(RX_TPB), lds, stream, in, reinterpret_cast<c32 *>(d_out),
				   n_in, n_out, p, q, tm, m, n_tiles, parts, reinterpret_cast<const uint32_t *>(d_hist_in),
				   reinterpret_cast<uint32_t *>(d_hist_out));
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
