// trx_ms_agc.hip -- the MS-side receive gain control on the device: the level of a slot (normed_abs_sum(), ms/ms.h:116-126) and
// maybe_update_gain() (ms/ms_rx_lower.cpp:101-126) over the slots of a pull.  The arithmetic is trx_ms_agc.h's.
//
// THE LEVEL.  The reference adds abs() of 2 * len int16 values into a float, one after the other.  While every partial sum is an
// integer <= 2^24 it is a float, so each of those additions is exact and the float the loop holds IS the integer prefix sum:
// where the integer total of a row is <= 2^24, float(total) is the reference's sum, whatever order the integers were added in.
// That is the hot path: per lane an integer sum over 16-byte loads (a slot begins at any sample, so the loads have a head of up
// to 3 samples in front of them and a tail behind), then a wave reduction.  One slot of 1250 values of at most 32768 reaches
// 4.1e7 > 2^24 only on a radio with rxFullScale 32767 near clipping, never at 2047.  For such a row the wave goes through it
// once more in tiles of 64 samples, in order: the integer prefix grows tile by tile while it stays <= 2^24, and from the first
// tile that would pass 2^24 on every value is added in float in the reference's order (additions that are still exact give
// what the integers would).  The ordered additions run on wave-uniform values (one readlane per value), every lane holding the
// same sum: no memory latency lies between two of them.
//
// THE GAIN.  gain_check only counts slots, so the host knows where the 160-slot windows of a pull lie: the rest of the open window,
// whole windows, a new open one.  Only the first piece needs the carried runmean; every other begins at gain_check == 0, where
// runmean = sum.  ms_gain_piece_kernel runs the recurrence of one piece per lane; ms_gain_decide_kernel then takes a member's
// closed windows in order, with one wave per member: rxgain chains through the decisions, and the state on the device moves.
#include <hip/hip_runtime.h>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_agc.h"
#include "trx_ms_sched.h"

namespace {

constexpr int WAVE = 64;
constexpr int WPB = 4;                         /* waves per block of the level kernel */
constexpr int kThreads = WPB * WAVE;

__device__ __forceinline__ unsigned uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

/* |I| + |Q| of one int16 pair; abs(-32768) is 32768 (the int16 is promoted) */
__device__ __forceinline__ unsigned abs_lo(uint32_t w) { const int v = (int)(int16_t)(w & 0xffffu); return (unsigned)(v < 0 ? -v : v); }
__device__ __forceinline__ unsigned abs_hi(uint32_t w) { const int v = (int)(int16_t)(w >> 16); return (unsigned)(v < 0 ? -v : v); }
__device__ __forceinline__ unsigned abs_pair(uint32_t w) { return abs_lo(w) + abs_hi(w); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
	for (int s = 1; s < WAVE; s <<= 1)
		v += __shfl_xor(v, s);
	return v;
}

/* the reference's float sum over the 2 * len values of one row (len >= 1 samples, 4-byte aligned), the same in every lane */
__device__ __forceinline__ float row_sum(const uint32_t *__restrict__ row, unsigned len, int lane)
{
	// the integer total: head (to the next 16-byte boundary), body in 16-byte loads, tail
	const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u);
	unsigned head = (4u - mis) & 3u;
	if (head > len)
		head = len;
	const unsigned nb = (len - head) >> 2, tail = (len - head) & 3u;
	const uint4 *body = reinterpret_cast<const uint4 *>(row + head);
	unsigned acc = 0;                                              /* <= 2^20 / 64 samples * 65536 = 2^30 per lane */
	for (unsigned i = (unsigned)lane; i < nb; i += WAVE) {
		const uint4 v = body[i];
		acc += abs_pair(v.x) + abs_pair(v.y) + abs_pair(v.z) + abs_pair(v.w);
	}
	if ((unsigned)lane < head)
		acc += abs_pair(row[lane]);
	if ((unsigned)lane < tail)
		acc += abs_pair(row[head + 4u * nb + (unsigned)lane]);
	const unsigned long long total = wave_sum(acc);
	if (total <= TRX_AGC_EXACT)
		return (float)(unsigned)total;                             /* exact: every partial sum of the reference's loop is this integer's prefix */

	// the ordered path: the integer prefix by tiles while it stays <= 2^24, then the reference's additions
	unsigned run = 0;
	float f = 0.0f;
	bool ordered = false;
	for (unsigned base = 0; base < len; base += WAVE) {
		const uint32_t w = base + (unsigned)lane < len ? row[base + lane] : 0u;   /* (behind the row: + 0.0f changes nothing) */
		const unsigned a0 = abs_lo(w), a1 = abs_hi(w);
		if (!ordered) {
			const unsigned t = uni((unsigned)wave_sum(a0 + a1));   /* <= 64 * 65536 */
			if (run + t <= TRX_AGC_EXACT) {
				run += t;
				continue;
			}
			ordered = true;
			f = (float)run;
		}
#pragma unroll
		for (int j = 0; j < WAVE; j++) {
			f = trx_agc_add(f, (float)__builtin_amdgcn_readlane((int)a0, j));
			f = trx_agc_add(f, (float)__builtin_amdgcn_readlane((int)a1, j));
		}
	}
	return f;
}

/* the row form: row r at in + r * row_stride samples */
__global__ void __launch_bounds__(kThreads)
ms_level_rows_kernel(const uint32_t *__restrict__ in, unsigned n_rows, unsigned row_len, size_t row_stride, float *__restrict__ out)
{
	const unsigned r = uni(blockIdx.x * WPB + (threadIdx.x >> 6));
	if (r >= n_rows)
		return;
	const int lane = (int)(threadIdx.x & 63);
	const float lv = trx_agc_level(row_sum(in + (size_t)r * row_stride, row_len, lane), 2u * row_len);
	if (lane == 0)
		out[r] = lv;
}

/* slot k of an entry: the stream form */
__device__ __forceinline__ void slot_level(const trx_agc_entry &e, unsigned k, int lane)
{
	const bool edge = e.edge_row != nullptr;
	const uint32_t *row = (edge && k == 0) ? static_cast<const uint32_t *>(e.edge_row)
					       : static_cast<const uint32_t *>(e.chunk) + (e.first + (int64_t)(k - (edge ? 1u : 0u)) * TRX_MSS_SLOT);
	const float lv = trx_agc_level(row_sum(row, TRX_MSS_SLOT, lane), 2u * TRX_MSS_SLOT);
	if (lane == 0) {
		e.work[k] = lv;
		if (e.level)
			e.level[k] = lv;
	}
}

/* the entry whose [first, next first) holds x; `first` rises strictly from 0 */
template <uint32_t trx_agc_entry::*FIRST>
__device__ __forceinline__ const trx_agc_entry *entry_of(const trx_agc_entry *__restrict__ tab, unsigned n_entries, unsigned x)
{
	unsigned lo = 0, hi = n_entries;
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) >> 1;
		if (tab[mid].*FIRST <= x)
			lo = mid;
		else
			hi = mid;
	}
	return tab + lo;
}

__global__ void __launch_bounds__(kThreads)
ms_level_stream_kernel(const trx_agc_entry e)
{
	const unsigned k = uni(blockIdx.x * WPB + (threadIdx.x >> 6));
	if (k < e.n_slots)
		slot_level(e, k, (int)(threadIdx.x & 63));
}

__global__ void __launch_bounds__(kThreads)
ms_level_group_kernel(const trx_agc_entry *__restrict__ tab, unsigned n_entries, unsigned n_waves)
{
	const unsigned gw = uni(blockIdx.x * WPB + (threadIdx.x >> 6));
	if (gw >= n_waves)
		return;
	const trx_agc_entry e = *entry_of<&trx_agc_entry::first_wave>(tab, n_entries, gw);
	slot_level(e, gw - e.first_wave, (int)(threadIdx.x & 63));
}

/* piece j of an entry: the recurrence over its slots, {runmean, sum of its last slot} behind the entry's levels */
__device__ __forceinline__ void gain_piece(const trx_agc_entry &e, unsigned j)
{
	const unsigned rest = TRX_AGC_WINDOW - e.gain_check;
	const unsigned start = j ? rest + (j - 1) * TRX_AGC_WINDOW : 0u;
	const unsigned gc = j ? 0u : e.gain_check;
	unsigned cnt = e.n_slots - start;
	if (cnt > TRX_AGC_WINDOW - gc)
		cnt = TRX_AGC_WINDOW - gc;
	float runmean = j ? 0.0f : e.state->runmean, sum = 0.0f;
	for (unsigned i = 0; i < cnt; i++) {
		sum = e.work[start + i];
		runmean = trx_agc_step(runmean, (int)(gc + i), sum);
	}
	e.work[e.n_slots + 2u * j] = runmean;
	e.work[e.n_slots + 2u * j + 1u] = sum;
}

__global__ void __launch_bounds__(kThreads)
ms_gain_piece_kernel(const trx_agc_entry e)
{
	const unsigned j = blockIdx.x * kThreads + threadIdx.x;
	if (j < trx_agc_pieces(e.gain_check, e.n_slots))
		gain_piece(e, j);
}

__global__ void __launch_bounds__(kThreads)
ms_gain_piece_group_kernel(const trx_agc_entry *__restrict__ tab, unsigned n_entries, unsigned n_pieces)
{
	const unsigned p = blockIdx.x * kThreads + threadIdx.x;
	if (p >= n_pieces)
		return;
	const trx_agc_entry e = *entry_of<&trx_agc_entry::first_piece>(tab, n_entries, p);
	gain_piece(e, p - e.first_piece);
}

/* The closed windows of one member's pull in order, by one wave: the lanes fetch 64 pieces' results at a time and each works out
 * its own window's gainoffset, which needs no gain; every lane then runs the same chain of decisions (rxgain goes from one to
 * the next) over the windows whose offset is not 0 and over those the ring keeps, and lane 0 writes the state: the records of
 * the pull's last TRX_AGC_RING decisions, rxgain, the counters, and the open window's gain_check and runmean */
__device__ __forceinline__ void gain_decide(const trx_agc_entry &e, uint32_t full_scale, int lane)
{
	trx_agc_state *s = e.state;
	const unsigned n = e.n_slots, gc0 = e.gain_check;
	const unsigned n_dec = (gc0 + n) / TRX_AGC_WINDOW, n_p = trx_agc_pieces(gc0, n);
	const float *res = e.work + n;
	float g = s->rx_gain;
	const uint64_t dec0 = s->decisions, slots0 = s->slots;
	unsigned n_applied = 0;
	for (unsigned base = 0; base < n_dec; base += WAVE) {
		const unsigned idx = base + (unsigned)lane;
		const float rm_v = idx < n_dec ? res[2u * idx] : 0.0f, sum_v = idx < n_dec ? res[2u * idx + 1u] : 0.0f;
		// a decision whose gainoffset is 0 has newgain == rxgain: it is not applied and leaves the chain as it is.  The chain
		// runs over the others (windows of near silence) and over those whose records the ring keeps
		const bool mine = idx < n_dec && (trx_agc_gainoffset(rm_v, full_scale) || idx + TRX_AGC_RING >= n_dec);
		unsigned long long todo = __ballot(mine);
		while (todo) {
			const unsigned j = (unsigned)__ffsll((long long)todo) - 1u;
			todo &= todo - 1;
			const float rm = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rm_v), (int)j));
			const float sum = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sum_v), (int)j));
			int applied;
			const float newgain = trx_agc_decide(rm, g, full_scale, &applied);
			const unsigned d = base + j;
			if (lane == 0 && d + TRX_AGC_RING >= n_dec) {
				trxhip_ms_agc_record *r = &s->ring[(dec0 + d) % TRX_AGC_RING];
				r->slot = slots0 + (TRX_AGC_WINDOW - gc0) + (uint64_t)d * TRX_AGC_WINDOW - 1;
				r->runmean = rm;
				r->sum = sum;
				r->old_gain = g;
				r->new_gain = newgain;
				r->applied = (uint32_t)applied;
				r->reserved = 0;
			}
			if (applied) {
				g = newgain;
				n_applied++;
			}
		}
	}
	if (lane == 0) {
		s->rx_gain = g;
		s->runmean = n_p > n_dec ? res[2u * (n_p - 1u)] : 0.0f;        /* the open window's, or :123 */
		s->gain_check = (gc0 + n) % TRX_AGC_WINDOW;
		s->slots = slots0 + n;
		s->decisions = dec0 + n_dec;
		s->applied += n_applied;
	}
}

__global__ void __launch_bounds__(WAVE)
ms_gain_decide_kernel(const trx_agc_entry e, uint32_t full_scale)
{
	gain_decide(e, full_scale, (int)threadIdx.x);
}

__global__ void __launch_bounds__(kThreads)
ms_gain_decide_group_kernel(const trx_agc_entry *__restrict__ tab, unsigned n_entries, uint32_t full_scale)
{
	const unsigned i = uni(blockIdx.x * WPB + (threadIdx.x >> 6));
	if (i >= n_entries)
		return;
	const trx_agc_entry e = tab[i];
	gain_decide(e, full_scale, (int)(threadIdx.x & 63));
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO; }

unsigned blocks(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int trx_launch_ms_level_rows(const int16_t *d_in, size_t n_rows, size_t row_len, size_t row_stride, float *d_level, hipStream_t stream)
{
	hipLaunchKernelGGL(ms_level_rows_kernel, dim3(blocks(n_rows, WPB)), dim3(kThreads), 0, stream, reinterpret_cast<const uint32_t *>(d_in),
			   (unsigned)n_rows, (unsigned)row_len, row_stride, d_level);
	return launched();
}

extern "C" int trx_launch_ms_agc(const trx_agc_entry *h_entry, const trx_agc_entry *d_tab, size_t n_entries, size_t n_waves, size_t n_pieces,
				 uint32_t full_scale, hipStream_t stream)
{
	if (h_entry) {
		hipLaunchKernelGGL(ms_level_stream_kernel, dim3(blocks(n_waves, WPB)), dim3(kThreads), 0, stream, *h_entry);
		hipLaunchKernelGGL(ms_gain_piece_kernel, dim3(blocks(n_pieces, kThreads)), dim3(kThreads), 0, stream, *h_entry);
		hipLaunchKernelGGL(ms_gain_decide_kernel, dim3(1), dim3(WAVE), 0, stream, *h_entry, full_scale);
	} else {
		hipLaunchKernelGGL(ms_level_group_kernel, dim3(blocks(n_waves, WPB)), dim3(kThreads), 0, stream, d_tab, (unsigned)n_entries,
				   (unsigned)n_waves);
		hipLaunchKernelGGL(ms_gain_piece_group_kernel, dim3(blocks(n_pieces, kThreads)), dim3(kThreads), 0, stream, d_tab,
				   (unsigned)n_entries, (unsigned)n_pieces);
		hipLaunchKernelGGL(ms_gain_decide_group_kernel, dim3(blocks(n_entries, WPB)), dim3(kThreads), 0, stream, d_tab,
				   (unsigned)n_entries, full_scale);
	}
	return launched();
}

extern "C" {

int trxhip_ms_level_batch_i16(trxhip_ctx *ctx, const int16_t *d_in, size_t n_rows, size_t row_len, size_t row_stride, float *d_level,
			      void *stream)
{
	if (!ctx || !d_in || (reinterpret_cast<uintptr_t>(d_in) & 3) || !d_level || (reinterpret_cast<uintptr_t>(d_level) & 3) || row_len < 1 ||
	    row_len > TRXHIP_SCH_SYNC_MAX_LEN || row_stride < row_len || n_rows > 0x7fffffffu)
		return TRXHIP_EINVAL;
	if (n_rows == 0)
		return TRXHIP_OK;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_ms_level_rows(d_in, n_rows, row_len, row_stride, d_level, static_cast<hipStream_t>(stream));
}

int trxhip_ms_agc_gate(float level, float rx_full_scale, float rx_gain, float *new_gain)
{
	if (!new_gain || !(rx_full_scale > 0.0f) || !(rx_full_scale <= 4294967040.0f) || !(level == level) || !(rx_gain == rx_gain))
		return TRXHIP_EINVAL;
	return trx_agc_gate(level, trx_agc_full_scale(rx_full_scale), rx_gain, new_gain) ? TRXHIP_MS_AGC_SEARCH : TRXHIP_MS_AGC_RAISE;
}

}  // extern "C"
