// trx_sch_sync.hip -- the MS-side synchronisation-burst receiver for gfx950, the live branch of ms_trx::handle_sch()
// (Transceiver52M/ms/ms_rx_lower.cpp:157-205): convert_and_scale, get_sch_chan_imp_resp / get_sch_buffer_chan_imp_resp
// (grgsm_vitac.cpp:283-309) over get_chan_imp_resp (:183-235), detect_burst_nb (:82-119) and decode_sch
// (ms_rx_lower.cpp:59-100: gsm_sch_decode / gsm_sch_parse / gsm_sch_to_fn, ms/sch.c:141-204) -- samples in, {BSIC, T1, T2, T3', FN}
// out, for a batch of buffers.  The receiver's device code is that of trx_va.hip (trx_va_common.h).
//
// TRACK (one slot, at most 625 samples): sch_sync_demod_kernel alone.  ONE WAVEFRONT PER FOUR BURSTS, as in trx_va.hip: the front
// end burst after burst on 64 lanes (160 correlations, the window search, matched filter), then the four trellises at once, one
// per DPP row, and behind them the four channel decoders, again one per row: the K = 5 code has 16 states, one per lane.
// ACQ (a buffer of up to TRXHIP_SCH_SYNC_MAX_LEN samples), three launches on the caller's stream:
//   sch_acq_power_kernel   |correlation|^2 of every lag (one lag per lane, 256 lags per workgroup from an LDS tile) into a scratch
//                          of the context -- 59 488 floats per 60 000-sample buffer do not fit next to each other in LDS
//   sch_acq_scan_kernel    the reference's window recurrence over all lags and its first maximum, one wave per buffer
//   sch_sync_demod_kernel  as above, with the 20 correlations of the chosen window computed again (the same instructions on the
//                          same samples: the same bits) in place of the search
// The window energy is the reference's SERIAL float recurrence ws += p[i] - p[i-20] (:203-215) and `best` its first maximum
// (std::max_element): together they decide the burst position, so neither is re-associated.  sch_scan_round() runs 64 steps of it
// as a DPP shift-add along the lanes, carrying the sum from round to round.
#include "trx_sch_common.h"
#include "trx_launch.h"

// d_sch_training_seq[5 .. 58] once more, where tests/test_sch_sync_cpu.py reads it: the kernels use trx_sch_common.h's, and a value
// that differs from it does not compile
#pragma clang diagnostic error "-Wmacro-redefined"
#define SS_SCH_CODES_LO 0x4eec46c4c6cecce6ull
#define SS_SCH_CODES_HI 0x6ccece4c4e4ull

#define SS_ACQ_TILE 256                  // lags per workgroup of sch_acq_power_kernel
#define SS_SCAN_R 4                      // rounds of 64 lags per pass of sch_acq_scan_kernel
#define SS_ACQ_TA 136                    // tile entries per phase: (256 + 4 * 53 + 3) / 4 = 117 used; 8 mod 32 like VA_XA

// ---- ACQ, step 1: power_buffer[] of get_chan_imp_resp() for the lags 0 .. n_lags-1 of every buffer
template <bool I16>
__global__ void __launch_bounds__(SS_ACQ_TILE)
sch_acq_power_kernel(const void *__restrict__ iq, size_t buf_stride, float *__restrict__ power, unsigned chunks, int len, int n_lags,
		     float scale)
{
	__shared__ __attribute__((aligned(16))) c32 tile[4 * SS_ACQ_TA];
	const unsigned buf = blockIdx.x / chunks;
	const int l0 = (int)(blockIdx.x % chunks) * SS_ACQ_TILE;
	const char *src = reinterpret_cast<const char *>(iq) + (size_t)buf * buf_stride * (I16 ? 4 : 8);
	for (int r = threadIdx.x; r < 4 * SS_ACQ_TA; r += SS_ACQ_TILE) {
		const int g = l0 + r;
		tile[(r & 3) * SS_ACQ_TA + (r >> 2)] = (g < len) ? ss_load<I16>(src, (size_t)g, scale) : make_float2(0.0f, 0.0f);
	}
	__syncthreads();
	const int r = threadIdx.x;
	float mag, pw;
	(void)ss_corr(tile + (r & 3) * SS_ACQ_TA + (r >> 2), mag, pw);
	if (l0 + r < n_lags)
		power[(size_t)buf * (size_t)n_lags + (size_t)(l0 + r)] = pw;
}

// ---- ACQ, step 2: the window energies and strongest_window_nr (:203-218), one wave per buffer
__global__ void __launch_bounds__(WAVE)
sch_acq_scan_kernel(const float *__restrict__ power, int32_t *__restrict__ best_out, int n_lags)
{
	const int lane = threadIdx.x;
	const float *p = power + (size_t)blockIdx.x * (size_t)n_lags;
	float carry = 0.0f;                                            // windowSum = 0
	float best_e = -__builtin_inff();
	int best_i = 0;
	// SS_SCAN_R rounds of 64 lags per pass, two passes per trip: each pass' powers are loaded (always, from clamped addresses)
	// into the register set the other pass is not using, one pass ahead of the chains that consume them
	float pa[2 * SS_SCAN_R], pb[2 * SS_SCAN_R];                    // {p[i], p[i-20]} per round
	auto fetch = [&](float (&d)[2 * SS_SCAN_R], int base) {
#pragma unroll
		for (int r = 0; r < SS_SCAN_R; r++) {
			const int ic = min(base + r * WAVE + lane, n_lags - 1);
			d[2 * r] = p[ic];
			d[2 * r + 1] = p[max(ic - VA_FL, 0)];
		}
	};
	auto pass = [&](const float (&d)[2 * SS_SCAN_R], int base) {
#pragma unroll
		for (int r = 0; r < SS_SCAN_R; r++) {
			const int i = base + r * WAVE + lane;
			// lags past the last one add nothing (they lie behind every lag that counts)
			const float q = (i < n_lags) ? sch_scan_term(d[2 * r], d[2 * r + 1], i) : 0.0f;
			const float e = sch_scan_round(q, carry, lane);
			// window i - 19 ends at lag i; a lane keeps the first largest of its own windows, which come in ascending order
			if (i >= VA_FL - 1 && i < n_lags && e > best_e) {
				best_e = e;
				best_i = i - (VA_FL - 1);
			}
		}
	};
	fetch(pa, 0);
	for (int base = 0; base < n_lags; base += 2 * SS_SCAN_R * WAVE) {
		// the barriers keep the scheduler from pulling a pass' first use of its powers (and with it the wait for them) up into
		// the pass before
		fetch(pb, base + SS_SCAN_R * WAVE);
		__builtin_amdgcn_sched_barrier(0);
		pass(pa, base);
		__builtin_amdgcn_sched_barrier(0);
		fetch(pa, base + 2 * SS_SCAN_R * WAVE);
		__builtin_amdgcn_sched_barrier(0);
		pass(pb, base + SS_SCAN_R * WAVE);
		__builtin_amdgcn_sched_barrier(0);
	}
	// std::max_element: the first largest = the lowest window number among the lanes that hold the maximum
	const float m = wave_max(best_e);
	int cand = (best_e == m) ? best_i : 0x7fffffff;
#pragma unroll
	for (int s = 1; s < WAVE; s <<= 1)
		cand = min(cand, __shfl_xor(cand, s));
	if (cand > n_lags - VA_FL)                                     // no lane holds the maximum (NaN input): window 0
		cand = 0;
	if (lane == 0)
		best_out[blockIdx.x] = cand;
}

// ---- TRACK: the whole receiver; ACQ, step 3: everything behind the search
template <bool I16>
__global__ void __launch_bounds__(SS_WPB * WAVE)
sch_sync_demod_kernel(const void *__restrict__ iq, size_t buf_stride, const int32_t *__restrict__ acq_best,
		      trxhip_sch_sync_result *__restrict__ results, int8_t *__restrict__ bits, unsigned n_bufs, int len, float scale)
{
	__shared__ __attribute__((aligned(16))) char smem[SS_WPB * SS_SLICE_BYTES];
	const int lane = threadIdx.x & (WAVE - 1);
	const int wave = uni((int)(threadIdx.x >> 6));
	char *base = smem + wave * SS_SLICE_BYTES;
	c32 *xs = reinterpret_cast<c32 *>(base);                       // polyphase: local sample j at xs[(j & 3) * SS_XA + (j >> 2)]
	c32 *corr = xs + 4 * SS_XA;
	c32 *cir = corr + SS_CORR;
	c32 *prod = cir + VA_FL;
	float *power = reinterpret_cast<float *>(prod + 64);
	float *sym_all = power + SS_CORR;
	c32 *rhh_all = reinterpret_cast<c32 *>(sym_all + VA_BPW * VA_FSTRIDE);
	int4 *meta = reinterpret_cast<int4 *>(rhh_all + VA_BPW * 8);
	unsigned long long *dec_all = reinterpret_cast<unsigned long long *>(meta + VA_BPW);
	uint4 *words = reinterpret_cast<uint4 *>(xs);                  // 148 x 16 bytes over the head of xs[]
	const bool acq = acq_best != nullptr;

	const unsigned q0 = (blockIdx.x * SS_WPB + wave) * VA_BPW;     // first burst of this wave
	if (q0 >= n_bufs)
		return;

	// =================== front end, one burst at a time (all 64 lanes) ===================
	for (int qb = 0; qb < VA_BPW; qb++) {
		const unsigned b = q0 + qb;
		if (b >= n_bufs) {                                         // batch tail: an idle row
			if (lane == 0) meta[qb] = make_int4(0, 0, 0, 0);
			continue;
		}
		const char *src = reinterpret_cast<const char *>(iq) + (size_t)b * buf_stride * (I16 ? 4 : 8);
		// TRACK: the first min(len, 625) samples, 40 samples into the zeroed array; ACQ: the window at the burst start, where a
		// negative start (a window among the first 188 lags) reads zeros in front of the buffer
		const int best_acq = acq ? uni(acq_best[b]) : 0;
		const int org = acq ? best_acq - SS_LAG0 : -40;
		const int lim = acq ? len : (len < 625 ? len : 625);
		for (int j = lane; j < SS_WIN; j += WAVE) {
			const int g = org + j;
			xs[(j & 3) * SS_XA + (j >> 2)] = (g >= 0 && g < lim) ? ss_load<I16>(src, (size_t)g, scale) : make_float2(0.0f, 0.0f);
		}
		wave_sync();

		// ---- get_chan_imp_resp (grgsm_vitac.cpp:183-235): TRACK 160 lags; ACQ the 20 of the chosen window
		const int nl = acq ? VA_FL : SS_NLAG;
		for (int r0 = 0; r0 < nl; r0 += WAVE) {
			const int k = r0 + lane;
			const int j0 = SS_LAG0 + (k < nl ? k : 0);
			float mag, pw;
			const c32 c = ss_corr(xs + (j0 & 3) * SS_XA + (j0 >> 2), mag, pw);
			corr[k] = c;                                           // k < SS_CORR: lanes past nl store a copy of lag 0's, never read
			power[k] = pw;
		}
		wave_sync();
		int best = 0;
		if (!acq) {
			float carry = 0.0f, best_e = -__builtin_inff();
			int best_i = 0;
			for (int r0 = 0; r0 < SS_NLAG; r0 += WAVE) {
				const int i = r0 + lane;
				const float pw = (i < SS_NLAG) ? power[i] : 0.0f;
				const float pp = (i >= VA_FL && i < SS_NLAG) ? power[i - VA_FL] : 0.0f;
				const float e = sch_scan_round(sch_scan_term(pw, pp, i), carry, lane);
				if (i >= VA_FL - 1 && i < SS_NLAG && e > best_e) {
					best_e = e;
					best_i = i - (VA_FL - 1);
				}
			}
			const float m = wave_max(best_e);
			int cand = (best_e == m) ? best_i : 0x7fffffff;        // std::max_element: the first largest
#pragma unroll
			for (int s = 1; s < WAVE; s <<= 1)
				cand = min(cand, __shfl_xor(cand, s));
			best = uni(cand > SS_NLAG - VA_FL ? 0 : cand);
		}
		// chan_imp_resp and max_correlation (:220-228)
		float mag = 0.0f;
		if (lane < VA_FL) {
			const c32 c = corr[best + lane];
			cir[lane] = c;
			mag = (float)sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);
		}
		const float corr_max = wave_max(mag);
		// what the reference's function returns, and the local sample detect_burst_nb starts at
		int start, sl;
		if (acq) {
			start = best_acq - SS_LAG0;
			sl = 0;
		} else {
			start = 148 + best - SS_LAG0;
			start = start < 39 ? start : 39;                       // ms_rx_lower.cpp:174-175
			start = start > -39 ? start : -39;
			sl = start + 40;
		}
		// the matched filter stops at sample start + 4 * 148 (grgsm_vitac.cpp:175-176): zero what lies behind
		if (lane < VA_FL + 4) {
			const int j = sl + SS_NBITS * VA_OSR + lane;
			xs[(j & 3) * SS_XA + (j >> 2)] = make_float2(0.0f, 0.0f);
		}
		wave_sync();
		va_rhh_mafi(xs, SS_XA, cir, prod, rhh_all + qb * 8, sym_all + qb * VA_FSTRIDE, sl, SS_NBITS, lane);
		if (lane == 0)
			meta[qb] = make_int4(SS_NBITS, 3, start, __float_as_int(corr_max));
		wave_sync();                                               // xs / corr / cir are the next burst's scratch
	}
	wave_sync();

	// =================== detect_burst_nb's trellis: start state 3, stop states {4, 12} ===================
	unsigned ones[5];
	va_trellis(sym_all, rhh_all, meta, words, lane, ones);
	const int row = lane >> 4, l4 = lane & 15;
	const int4 mt = meta[row];
	const unsigned bme = q0 + row;
	const bool live = bme < n_bufs;
	// output_binary[i] = output[i] > 0 ? -127 : 127 ("pre flip bits!", grgsm_vitac.cpp:101-102)
	if (live && bits) {
		int8_t *bo = bits + (size_t)bme * SS_NBITS;
#pragma unroll
		for (int t = 0; t < 10; t++) {
			const int i = 16 * t + l4;
			if (i < SS_NBITS)
				bo[i] = ((ones[t >> 1] >> (16 * (t & 1) + l4)) & 1u) ? -127 : 127;
		}
	}

	// =================== decode_sch (ms_rx_lower.cpp:59-100), one decoder per row ===================
	unsigned bsic, t1, t2, t3p;
	int fn;
	const bool ok = ss_decode_sch(ones, dec_all, lane, bsic, t1, t2, t3p, fn);
	if (live && l4 == 0) {
		trxhip_sch_sync_result r;
		r.rc = ok ? 1 : 0;
		r.start = mt.z;
		r.corr_max = __int_as_float(mt.w);
		r.fn = ok ? fn : -1;
		r.t1 = ok ? (uint16_t)t1 : 0;
		r.bsic = ok ? (uint8_t)bsic : 0;
		r.t2 = ok ? (uint8_t)t2 : 0;
		r.t3p = ok ? (uint8_t)t3p : 0;
		r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
		results[bme] = r;
	}
}

extern "C" int trx_launch_sch_sync(const void *d_iq, int i16, size_t buf_stride, trxhip_sch_sync_result *d_results, int8_t *d_bits,
				   size_t n_bufs, int len, int acq, float scale, float *d_power, int32_t *d_best, hipStream_t stream)
{
	if (n_bufs == 0)
		return 0;
	if (acq) {
		const int n_lags = len - 512;                              // search_stop_pos = len - N_SYNC_BITS * 8 (:304)
		const size_t chunks = ((size_t)n_lags + SS_ACQ_TILE - 1) / SS_ACQ_TILE;
		if (!d_power || !d_best || n_lags < VA_FL || chunks * n_bufs > 0x7fffffffull)
			return TRXHIP_EINVAL;
		if (i16)
			hipLaunchKernelGGL(sch_acq_power_kernel<true>, dim3((unsigned)(chunks * n_bufs)), dim3(SS_ACQ_TILE), 0, stream, d_iq,
					   buf_stride, d_power, (unsigned)chunks, len, n_lags, scale);
		else
			hipLaunchKernelGGL(sch_acq_power_kernel<false>, dim3((unsigned)(chunks * n_bufs)), dim3(SS_ACQ_TILE), 0, stream, d_iq,
					   buf_stride, d_power, (unsigned)chunks, len, n_lags, scale);
		hipLaunchKernelGGL(sch_acq_scan_kernel, dim3((unsigned)n_bufs), dim3(WAVE), 0, stream, d_power, d_best, n_lags);
	}
	const size_t per_block = SS_WPB * VA_BPW;
	const size_t grid = (n_bufs + per_block - 1) / per_block;
	const int32_t *best = acq ? d_best : nullptr;
	if (i16)
		hipLaunchKernelGGL(sch_sync_demod_kernel<true>, dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_iq, buf_stride, best,
				   d_results, d_bits, (unsigned)n_bufs, len, scale);
	else
		hipLaunchKernelGGL(sch_sync_demod_kernel<false>, dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_iq, buf_stride, best,
				   d_results, d_bits, (unsigned)n_bufs, len, scale);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
