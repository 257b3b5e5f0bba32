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
#include "trx_va_common.h"
#include "trx_launch.h"

#define SS_WPB 2                         // waves per workgroup of sch_sync_demod_kernel
// the 4-samples-per-symbol window a burst is demodulated from: local sample j = buffer sample org + j, zeros outside the buffer.
// TRACK: org = -40 (the reference copies the slot 40 samples into a zeroed array, ms_rx_lower.cpp:162-164); ACQ: org = burst start.
#define SS_WIN 800                       // >= 79 + 4 * 148 + 24 (latest clamped start, burst, filter tail) and a multiple of 64
#define SS_XA VA_XA(SS_WIN - 100)        // 200 entries per phase: 4 * SS_XA = SS_WIN
#define SS_LAG0 188                      // local lag of the first correlation: (SYNC_POS + TRAIN_BEGINNING - 10) * 4 + 40 (TRACK),
                                         // (SYNC_POS + TRAIN_BEGINNING) * 4 (ACQ, where local sample 0 is the burst start)
#define SS_NLAG 160                      // TRACK: lags 148 .. 307 of the slot
#define SS_CORR 192                      // corr[] / power[] entries: three rounds of 64
#define SS_NBITS 148
// per-wave LDS slice, every region 16-byte aligned:
//   xs[4][SS_XA] | corr[192] | cir[20] | prod[64] : c32;  power[192] : float;  sym[4][152] : float | rhh[4][8] : c32;
//   meta[4] : int4 {nbits, start state, start, corr_max};  dec[4][16] : 64-bit decision words of the channel decoder
//   (the trellis' decision words lie over xs[], as in trx_va.hip)
#define SS_SLICE_BYTES ((4 * SS_XA + SS_CORR + VA_FL + 64) * 8 + SS_CORR * 4 + VA_BPW * (VA_FSTRIDE * 4 + 8 * 8) + VA_BPW * 16 +       \
			VA_BPW * 16 * 8)
static_assert(4 * SS_XA == SS_WIN && SS_SLICE_BYTES % 16 == 0 && SS_WPB * SS_SLICE_BYTES <= 64 * 1024, "LDS layout");

// d_sch_training_seq[5 .. 58] (grgsm_vitac.cpp:60-62, :288-289): gmsk_mapper over the 64 extended training bits of
// 3GPP TS 45.002 5.2.5 from the start point -j, conjugated, as quarter-turn codes like VA_ACC_CODES (trx_va.hip): elements
// 0 .. 31 and 32 .. 53.  tests/test_sch_sync_cpu.py compares with a run-time walk.
#define SS_SCH_CODES_LO 0x4eec46c4c6cecce6ull
#define SS_SCH_CODES_HI 0x6ccece4c4e4ull
#define SS_SEQ_LEN 54

#define SS_ACQ_TILE 256                  // lags per workgroup of sch_acq_power_kernel
#define SS_SCAN_R 4                      // rounds of 64 lags per pass of sch_acq_scan_kernel
#define SS_ACQ_TA 136                    // tile entries per phase: (256 + 4 * 53 + 3) / 4 = 117 used; 8 mod 32 like VA_XA

// convert_and_scale (ms_rx_lower.cpp:168): every component times scale
template <bool I16>
__device__ __forceinline__ c32 ss_load(const void *src, size_t i, float scale)
{
	if (I16) {
		const short2 v = reinterpret_cast<const short2 *>(src)[i];
		return make_float2((float)v.x * scale, (float)v.y * scale);
	}
	const c32 v = reinterpret_cast<const c32 *>(src)[i];
	return make_float2(v.x * scale, v.y * scale);
}

// correlate_sequence() for the lane's lag (p: the address of its first sample in a polyphase array), :148-156, and
// std::pow(abs(c), 2) the way libstdc++ / glibc evaluate it (:199): hypot in double rounded to float, squared in double
__device__ __forceinline__ c32 ss_corr(const c32 *p, float &mag, float &power)
{
	const trx_v2f r = va_corr<SS_SCH_CODES_LO, SS_SEQ_LEN, SS_SCH_CODES_HI>(p);
	const c32 c = make_float2(r.x / 54.0f, -r.y / 54.0f);          // conj(result) / gr_complex(length, 0)
	mag = (float)sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);
	power = (float)((double)mag * (double)mag);
	return c;
}

// 64 steps of ws += q: lane l ends with carry + q[0] + ... + q[l], added left to right one term at a time (wave_shr:1 leaves
// lane 0 alone, so after step i the lanes 0 .. i hold their final sums).  Returns the lane's sum; carry becomes lane 63's.
// The 63 dependent steps are ONE asm block: nothing the compiler schedules lands between two links of the chain, whose length
// is the kernel's run time (s_nop 1: the two wait states a DPP source written by the previous VALU op needs on gfx9).
#define SS_STEP1 "s_nop 1\n\tv_add_f32_dpp %0, %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define SS_STEP4 SS_STEP1 SS_STEP1 SS_STEP1 SS_STEP1
#define SS_STEP16 SS_STEP4 SS_STEP4 SS_STEP4 SS_STEP4
__device__ __forceinline__ float sch_scan_round(float q, float &carry, int lane)
{
	float acc = (lane == 0) ? carry + q : q;
	asm volatile(SS_STEP16 SS_STEP16 SS_STEP16 SS_STEP4 SS_STEP4 SS_STEP4 SS_STEP1 SS_STEP1 SS_STEP1 : "+v"(acc) : "v"(q));
	carry = lane_val(acc, 63);
	return acc;
}

// the term the recurrence adds at lag i: p[i] while the first window fills (:206-208), then p[i] - p[i-20] (:212-213)
__device__ __forceinline__ float sch_scan_term(float p, float p20, int i)
{
	return (i < VA_FL) ? p : p - p20;
}

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

// 3GPP TS 45.003 4.7, the trellis of sch_next_output (sch.c:60-65): the cost of leaving state p with input u when the two soft
// bits are x0, x1 (a coded 0 expects +127, a coded 1 expects -127; cost |x - e|)
__device__ __forceinline__ int ss_branch(int p, int u, int x0, int x1)
{
	const int b0 = p & 1, b2 = (p >> 2) & 1, b3 = (p >> 3) & 1;
	const int c0 = u ^ b2 ^ b3, c1 = u ^ b0 ^ b2 ^ b3;
	return abs(x0 - (c0 ? -127 : 127)) + abs(x1 - (c1 ? -127 : 127));
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
	// osmo_conv_decode of the K = 5 code over data = bits[3 .. 41] | bits[106 .. 144] (:66-67): 39 steps from state 0, flushed to
	// state 0.  Lane l4 holds state n = l4, reached from p = n >> 1 and p + 8 with input n & 1; the candidate from the higher
	// state replaces the other only when strictly smaller.
	int pm = (l4 == 0) ? 0 : (1 << 24);
	unsigned long long dec = 0ull;
	const int p0 = l4 >> 1, p1 = p0 + 8, u = l4 & 1;
#pragma unroll
	for (int k = 0; k < 39; k++) {
		const int d0 = 2 * k, d1 = 2 * k + 1;
		const int i0 = d0 < 39 ? 3 + d0 : 106 + (d0 - 39), i1 = d1 < 39 ? 3 + d1 : 106 + (d1 - 39);
		const int x0 = ((ones[i0 >> 5] >> (i0 & 31)) & 1u) ? -127 : 127;
		const int x1 = ((ones[i1 >> 5] >> (i1 & 31)) & 1u) ? -127 : 127;
		const int m0 = __builtin_amdgcn_ds_bpermute(((lane & ~15) | p0) << 2, pm);
		const int m1 = __builtin_amdgcn_ds_bpermute(((lane & ~15) | p1) << 2, pm);
		const int c0 = m0 + ss_branch(p0, u, x0, x1), c1 = m1 + ss_branch(p1, u, x0, x1);
		const bool d = c1 < c0;
		pm = d ? c1 : c0;
		dec |= (unsigned long long)d << k;
	}
	unsigned long long *dec_row = dec_all + row * 16;
	dec_row[l4] = dec;
	wave_sync();
	unsigned long long ub = 0ull;                                  // bit k: u(k); every lane of a row walks its row's path
	{
		int s = 0;
		for (int k = 38; k >= 0; k--) {
			ub |= (unsigned long long)(s & 1) << k;
			s = (s >> 1) + (int)((dec_row[s] >> k) & 1ull) * 8;
		}
	}
	// osmo_crc16gen_check_bits(gsm0503_sch_crc10): D^10 + D^8 + D^6 + D^5 + D^4 + D^2 + 1 over the 25 information bits, remainder
	// inverted, against bits 25 .. 34 (sch.c:195-199)
	unsigned reg = 0u;
	for (int k = 0; k < 25; k++) {
		reg ^= (unsigned)((ub >> k) & 1ull) << 9;
		reg = (reg & 0x200u) ? ((reg << 1) ^ 0x175u) : (reg << 1);
		reg &= 0x3ffu;
	}
	reg ^= 0x3ffu;
	unsigned par = 0u;
	for (int k = 0; k < 10; k++)
		par |= (unsigned)((ub >> (25 + k)) & 1ull) << (9 - k);
	if (live && l4 == 0) {
		// gsm_sch_parse (sch.c:162-185) over sch_packed_info (:41-49): t1_hi[2] bsic[6] t1_md[8] t3p_hi[2] t2[5] t1_lo t3p_lo
		const unsigned w = (unsigned)ub;
		const unsigned bsic = (w >> 2) & 63u;
		const unsigned t1 = ((w >> 23) & 1u) | (((w >> 8) & 0xffu) << 1) | ((w & 3u) << 9);
		const unsigned t2 = (w >> 18) & 31u;
		const unsigned t3p = ((w >> 24) & 1u) | (((w >> 16) & 3u) << 1);
		// gsm_sch_to_fn (sch.c:142-159); the fields are unsigned here, so fn >= 0 always
		const int t3 = (int)t3p * 10 + 1;
		const int tt = (t3 < (int)t2) ? (t3 + 26) - (int)t2 : (t3 - (int)t2) % 26;
		const int fn = (int)t1 * 51 * 26 + tt * 51 + t3;
		const bool ok = par == reg;
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
