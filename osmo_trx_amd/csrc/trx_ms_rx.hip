// trx_ms_rx.hip -- the MS-side downlink burst receiver for gfx950: upper_trx::pullRadioVector() and what driveReceiveFIFO() hands to
// trxcon (Transceiver52M/ms/ms_upper.cpp:161-304), for a batch of slots of 625 samples.  Per slot: its kind from (FN, TN)
// (gsm_fcch_check_ts / gsm_sch_check_ts, ms/sch.c:100-139), and then
//   SCH      what ms_trx::handle_sch() demodulates whether or not the upper layer listens (ms_rx_lower.cpp:130-153, :157-205): the
//            TRACK receiver of trx_sch_sync.hip, instruction for instruction (trx_sch_common.h), with decode_sch()
//   traffic  convert_and_scale, energyDetect(sv, 80) (sigProcLib.cpp:1573-1585), get_norm_chan_imp_resp on the cell's TSC
//            (grgsm_vitac.cpp:265-274 over :183-235), the clamp to +-39, detect_burst_nb (:82-119) and the RSSI (ms_upper.cpp:203-230,
//            :272-274) -- only where trxcon answered ACTIVE (:183-187)
//   FCCH     nothing ("return trash", :189-192); BAD and inactive traffic slots: nothing
// ONE WAVEFRONT PER FOUR SLOTS, as in trx_sch_sync.hip: the front end slot after slot on 64 lanes, the kind a wave-uniform choice
// of training sequence, first lag and number of lags; then the four trellises at once, one per DPP row (a slot with nothing to
// demodulate is an idle row, like the batch tail), and the channel decoder only in waves that hold an SCH slot.
// Both of the reference's serial float sums keep their order: the window recurrence (sch_scan_round) and energyDetect's 80 terms
// (the same DPP shift-add chain: 64 steps and 16).
// THE STREAM FORM (trx_ms_sched.hip) is a second instantiation of the same body: a slot's record is computed from the pull's base
// clock and the slot index, the slot is read where it lies in the caller's chunk (or from the row that holds the straddling
// slot), and a decoded SCH slot with abs(start) > 1 adds -start to the pull's correction word.
// THE GROUP FORM (trxhip_ms_group_*) is the stream form behind a table: a wave's four slots belong to one member of a group of
// streams, and the wave takes chunk, descriptor and outputs from that member's table entry.
// THE ROTATING INSTANCES (ROT) of the stream and group forms are the same body with the NCO (trx_ms_nco.h) in the slot fill: the
// sample is read unscaled, multiplied by the phasor of its phase and then by scale, so the window holds what the non-rotating
// instance makes of the rotated stream, bit for bit.  The zero padding stays zero; nothing else changes.
#include "trx_sch_common.h"
#include "trx_launch.h"
#include "trx_ms_nco.h"
#include "trx_ms_sched.h"

#define MS_SLOT 625                      // ONE_TS_BURST_LEN (ms.h:50)
// get_norm_chan_imp_resp: search_center = TRAIN_POS = 3 + 57 + 1 + 5; lags (66 - 5) * 4 + 1 .. (66 + 5 + 5) * 4 - 1 of the slot, which
// lies 40 samples into the window
#define MS_NB_CENTER (66 * VA_OSR)
#define MS_NB_LAG0 ((66 - 5) * VA_OSR + 1 + 40)
#define MS_NB_NLAG 59
#define MS_EN_TERMS 80                   // energyDetect(sv, 20 * 4): samples 0, 4, ..., 316
// per-wave LDS slice: trx_sch_common.h's, and behind it info[4] : int4 {kind | sent << 8 | flags << 16, pow, -, -}
#define MS_SLICE_BYTES (SS_SLICE_BYTES + VA_BPW * 16)
static_assert(MS_SLICE_BYTES % 16 == 0 && SS_WPB * MS_SLICE_BYTES <= 64 * 1024, "LDS layout");
static_assert(MS_NB_LAG0 + MS_NB_NLAG - 1 + 15 * VA_OSR < SS_WIN && MS_NB_NLAG <= WAVE, "normal-burst search inside the window");
static_assert(sizeof(trxhip_ms_slot) == 8 && sizeof(trxhip_ms_burst_ind) == 32, "record layout");

// correlate_sequence() on d_norm_training_seq[tsc][5 .. 20] for the lane's lag, and std::pow(abs(c), 2), as ss_corr() does for the
// synchronisation sequence.  conj(result) / (16, 0): a division by 16 is an exact scaling
__device__ __forceinline__ c32 ms_nb_corr(const c32 *p, int tsc, float &mag, float &power)
{
	trx_v2f r;
	switch (tsc) {                                                 // wave-uniform: one specialised loop per training sequence
	case 0: r = va_corr<VA_TSC_CODES0, 16>(p); break;
	case 1: r = va_corr<VA_TSC_CODES1, 16>(p); break;
	case 2: r = va_corr<VA_TSC_CODES2, 16>(p); break;
	case 3: r = va_corr<VA_TSC_CODES3, 16>(p); break;
	case 4: r = va_corr<VA_TSC_CODES4, 16>(p); break;
	case 5: r = va_corr<VA_TSC_CODES5, 16>(p); break;
	case 6: r = va_corr<VA_TSC_CODES6, 16>(p); break;
	default: r = va_corr<VA_TSC_CODES7, 16>(p); break;
	}
	const c32 c = make_float2(r.x * 0.0625f, -r.y * 0.0625f);
	mag = (float)sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);
	power = (float)((double)mag * (double)mag);
	return c;
}

// energyDetect(sv, 80): energy += norm2(x[4 i]) for i = 0 .. 79 one term at a time, then energy / 80.  x0: slot sample 0 in its
// phase array, where the samples 4 i lie one entry apart.  Terms 0 .. 63 are one sch_scan_round(), terms 64 .. 79 fifteen more
// links of the same chain on the lanes 0 .. 15.
__device__ __forceinline__ float ms_energy_detect(const c32 *x0, int lane)
{
	float carry = 0.0f;                                            // float energy = 0.0
	(void)sch_scan_round(norm2(x0[lane]), carry, lane);
	const float q = norm2(x0[WAVE + (lane & 15)]);
	float acc = (lane == 0) ? carry + q : q;
	asm volatile(SS_STEP4 SS_STEP4 SS_STEP4 SS_STEP1 SS_STEP1 SS_STEP1 : "+&v"(acc) : "v"(q));
	return lane_val(acc, MS_EN_TERMS - WAVE - 1) / (float)MS_EN_TERMS;
}

// The two words of slot b's record {fn | tn, tsc, flags}: read from the slot records, or (STREAM) made from the pull's base clock
template <bool STREAM>
__device__ __forceinline__ void ms_slot_words(const trxhip_ms_slot *slots, const trx_mss_stream &sa, unsigned b, uint32_t &w0, uint32_t &w1)
{
	if (STREAM) {
		int tn;
		trx_mss_clock_add(sa.fn0, sa.tn0, b, &w0, &tn);
		w1 = (uint32_t)tn | (uint32_t)sa.tsc << 8 | (((sa.active >> tn) & 1u) ? (uint32_t)TRXHIP_MS_SLOT_ACTIVE << 16 : 0u);
	} else {
		w0 = reinterpret_cast<const uint32_t *>(slots)[2 * (size_t)b];
		w1 = reinterpret_cast<const uint32_t *>(slots)[2 * (size_t)b + 1];
	}
}

// Where slot b's 625 samples lie: row b of the batch, or (STREAM) in the chunk / in the straddling slot's row
template <bool I16, bool STREAM>
__device__ __forceinline__ const char *ms_slot_src(const void *iq, size_t slot_stride, const trx_mss_stream &sa, unsigned b)
{
	if (STREAM) {
		if (sa.edge_row && b == 0)
			return reinterpret_cast<const char *>(sa.edge_row);
		const int64_t at = sa.first + (int64_t)(b - (sa.edge_row ? 1u : 0u)) * MS_SLOT;
		return reinterpret_cast<const char *>(iq) + at * (I16 ? 4 : 8);
	}
	return reinterpret_cast<const char *>(iq) + (size_t)b * slot_stride * (I16 ? 4 : 8);
}

// The oscillator of a rotating instance: the entry's record and the phasor tables; empty in the others
struct ms_rx_nco {
	trx_nco_slot o;
	const float *tab;
};

// convert_and_scale behind the NCO: sample i of the slot whose first sample has the phase p_slot
template <bool I16>
__device__ __forceinline__ c32 ms_load_rot(const void *src, size_t i, float scale, uint32_t p_slot, const ms_rx_nco &nco)
{
	const c32 x = ss_load<I16>(src, i, 1.0f);                      // (x * 1.0f is x)
	float rc, rs, yr, yi;
	trx_nco_phasor(nco.tab, p_slot + (uint32_t)i * (uint32_t)nco.o.inc, &rc, &rs);
	trx_nco_rotate(x.x, x.y, rc, rs, &yr, &yi);
	return make_float2(yr * scale, yi * scale);
}

// The receiver of one wave: the VA_BPW slots from q0 on, of n_slots.  wave: the wave's index in its block (its LDS slice)
template <bool I16, bool STREAM, bool ROT = false>
__device__ __forceinline__ void ms_rx_wave(const void *__restrict__ iq, size_t slot_stride, const trxhip_ms_slot *__restrict__ slots,
					   trxhip_ms_burst_ind *__restrict__ ind, int8_t *__restrict__ bits, unsigned n_slots, float scale,
					   float rx_full_scale, const trx_mss_stream &sa, const int wave, const unsigned q0,
					   const ms_rx_nco &nco = ms_rx_nco())
{
	__shared__ __attribute__((aligned(16))) char smem[SS_WPB * MS_SLICE_BYTES];
	const int lane = threadIdx.x & (WAVE - 1);
	char *base = smem + wave * MS_SLICE_BYTES;
	c32 *xs = reinterpret_cast<c32 *>(base);                       // polyphase: local sample j at xs[(j & 3) * SS_XA + (j >> 2)]
	c32 *corr = xs + 4 * SS_XA;
	c32 *cir = corr + SS_CORR;
	c32 *prod = cir + VA_FL;
	float *power = reinterpret_cast<float *>(prod + 64);
	float *sym_all = power + SS_CORR;
	c32 *rhh_all = reinterpret_cast<c32 *>(sym_all + VA_BPW * VA_FSTRIDE);
	int4 *meta = reinterpret_cast<int4 *>(rhh_all + VA_BPW * 8);
	unsigned long long *dec_all = reinterpret_cast<unsigned long long *>(meta + VA_BPW);
	int4 *info = reinterpret_cast<int4 *>(base + SS_SLICE_BYTES);
	uint4 *words = reinterpret_cast<uint4 *>(xs);                  // 148 x 16 bytes over the head of xs[]

	if (q0 >= n_slots)
		return;

	// =================== front end, one slot at a time (all 64 lanes) ===================
	for (int qb = 0; qb < VA_BPW; qb++) {
		const unsigned b = q0 + qb;
		if (b >= n_slots) {                                        // batch tail: an idle row
			if (lane == 0) {
				meta[qb] = make_int4(0, 0, 0, 0);
				info[qb] = make_int4(0, 0, 0, 0);
			}
			continue;
		}
		// the slot's kind (ms_upper.cpp:180-181 over sch.c:100-139) and what the reference does with it
		uint32_t sw0, sw1;
		ms_slot_words<STREAM>(slots, sa, b, sw0, sw1);
		const unsigned w1 = (unsigned)uni((int)sw1);
		const unsigned fn51 = (unsigned)uni((int)sw0) % 51u;
		const unsigned tn = w1 & 0xffu, tsc = (w1 >> 8) & 0xffu;
		const bool active = ((w1 >> 16) & TRXHIP_MS_SLOT_ACTIVE) != 0;
		int kind = TRXHIP_MS_KIND_NB;
		if (tn == 0 && fn51 % 10u == 0 && fn51 <= 40u)
			kind = TRXHIP_MS_KIND_FCCH;
		if (tn == 0 && fn51 % 10u == 1 && fn51 <= 41u)
			kind = TRXHIP_MS_KIND_SCH;
		if (tn > 7 || (kind == TRXHIP_MS_KIND_NB && tsc > 7))
			kind = TRXHIP_MS_KIND_BAD;
		const bool sch = kind == TRXHIP_MS_KIND_SCH;
		const bool sent = active && kind != TRXHIP_MS_KIND_BAD;    // :186-187: not active, no indication
		if (!(sch || (kind == TRXHIP_MS_KIND_NB && active))) {     // nothing to demodulate: an idle row
			if (lane == 0) {
				meta[qb] = make_int4(0, 0, 0, 0);
				info[qb] = make_int4(kind | (sent ? 1 << 8 : 0) | (sent && kind == TRXHIP_MS_KIND_FCCH ? TRXHIP_MS_IND_TRASH << 16 : 0), 0, 0, 0);
			}
			continue;
		}
		// the slot 40 samples into the zeroed array (ms_upper.cpp:164-171, ms_rx_lower.cpp:162-164), scaled on the way in
		const char *src = ms_slot_src<I16, STREAM>(iq, slot_stride, sa, b);
		if (ROT) {
			// slot b's first sample: the edge row's own phase, else b slots of 625 behind the chunk's first (trx_ms_nco.h)
			const bool edge = sa.edge_row != nullptr;
			const uint32_t ps = (edge && b == 0) ? nco.o.edge : nco.o.phase0 + (b - (edge ? 1u : 0u)) * (uint32_t)MS_SLOT * (uint32_t)nco.o.inc;
			for (int j = lane; j < SS_WIN; j += WAVE) {
				const int g = j - 40;
				xs[(j & 3) * SS_XA + (j >> 2)] =
					(g >= 0 && g < MS_SLOT) ? ms_load_rot<I16>(src, (size_t)g, scale, ps, nco) : make_float2(0.0f, 0.0f);
			}
		} else {
			for (int j = lane; j < SS_WIN; j += WAVE) {
				const int g = j - 40;
				xs[(j & 3) * SS_XA + (j >> 2)] = (g >= 0 && g < MS_SLOT) ? ss_load<I16>(src, (size_t)g, scale) : make_float2(0.0f, 0.0f);
			}
		}
		wave_sync();
		float pow = 0.0f;
		if (!sch)
			pow = ms_energy_detect(xs + 40 / VA_OSR, lane);        // slot sample 0 = local sample 40: phase 0

		// ---- get_chan_imp_resp (grgsm_vitac.cpp:183-235): 160 lags on the synchronisation sequence, 59 on the TSC
		const int nl = sch ? SS_NLAG : MS_NB_NLAG, lag0 = sch ? SS_LAG0 : MS_NB_LAG0;
		for (int r0 = 0; r0 < nl; r0 += WAVE) {
			const int k = r0 + lane;
			const int j0 = lag0 + (k < nl ? k : 0);
			const c32 *p = xs + (j0 & 3) * SS_XA + (j0 >> 2);
			float mag, pw;
			const c32 c = sch ? ss_corr(p, mag, pw) : ms_nb_corr(p, (int)tsc, mag, pw);
			corr[k] = c;                                           // k < SS_CORR: lanes past nl store a copy of lag 0's, never read
			power[k] = pw;
		}
		wave_sync();
		int best;
		{
			float carry = 0.0f, best_e = -__builtin_inff();
			int best_i = 0;
			for (int r0 = 0; r0 < nl; r0 += WAVE) {
				const int i = r0 + lane;
				const float pw = (i < nl) ? power[i] : 0.0f;
				const float pp = (i >= VA_FL && i < nl) ? power[i - VA_FL] : 0.0f;
				const float e = sch_scan_round(sch_scan_term(pw, pp, i), carry, lane);
				if (i >= VA_FL - 1 && i < nl && e > best_e) {
					best_e = e;
					best_i = i - (VA_FL - 1);
				}
			}
			const float m = wave_max(best_e);
			int cand = (best_e == m) ? best_i : 0x7fffffff;        // std::max_element: the first largest
#pragma unroll
			for (int s = 1; s < WAVE; s <<= 1)
				cand = min(cand, __shfl_xor(cand, s));
			best = uni(cand > nl - VA_FL ? 0 : cand);
		}
		// chan_imp_resp and max_correlation (:220-228)
		float mag = 0.0f;
		if (lane < VA_FL) {
			const c32 c = corr[best + lane];
			cir[lane] = c;
			mag = (float)sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);
		}
		const float corr_max = wave_max(mag);
		// search_start_pos + strongest_window_nr - search_center * d_OSR, and the clamp (ms_rx_lower.cpp:174-175, ms_upper.cpp:224-225)
		int start = sch ? 148 + best - SS_LAG0 : (MS_NB_LAG0 - 40) + best - MS_NB_CENTER;
		start = start < 39 ? start : 39;
		start = start > -39 ? start : -39;
		const int sl = start + 40;
		// the matched filter stops at sample start + 4 * 148 (grgsm_vitac.cpp:175-176): zero what lies behind
		if (lane < VA_FL + 4) {
			const int j = sl + SS_NBITS * VA_OSR + lane;
			xs[(j & 3) * SS_XA + (j >> 2)] = make_float2(0.0f, 0.0f);
		}
		wave_sync();
		va_rhh_mafi(xs, SS_XA, cir, prod, rhh_all + qb * 8, sym_all + qb * VA_FSTRIDE, sl, SS_NBITS, lane);
		if (lane == 0) {
			meta[qb] = make_int4(SS_NBITS, 3, start, __float_as_int(corr_max));
			// an all-zero traffic slot: the reference's rxFullScale / 0 has no RSSI
			const int fl = (!sch && pow == 0.0f) ? TRXHIP_MS_IND_SILENT : 0;
			info[qb] = make_int4(kind | (sent ? 1 << 8 : 0) | (fl << 16), __float_as_int(pow), 0, 0);
		}
		wave_sync();                                               // xs / corr / cir are the next slot's scratch
	}
	wave_sync();

	// =================== detect_burst_nb's trellis: start state 3, stop states {4, 12} ===================
	const int row = lane >> 4, l4 = lane & 15;
	const int4 mt = meta[row];
	const int4 nf = info[row];
	const int kind = nf.x & 0xff;
	const unsigned bme = q0 + row;
	const bool live = bme < n_slots;
	unsigned ones[5] = { 0u, 0u, 0u, 0u, 0u };
	if (__ballot(mt.x > 0) != 0ull)                                // wave-uniform: a wave of idle rows has no trellis to run
		va_trellis(sym_all, rhh_all, meta, words, lane, ones);
	// output_binary[i] = output[i] > 0 ? -127 : 127 ("pre flip bits!", grgsm_vitac.cpp:101-102); zeros where nothing was demodulated
	if (live && bits) {
		int8_t *bo = bits + (size_t)bme * SS_NBITS;
#pragma unroll
		for (int t = 0; t < 10; t++) {
			const int i = 16 * t + l4;
			if (i < SS_NBITS)
				bo[i] = (mt.x == 0) ? 0 : ((ones[t >> 1] >> (16 * (t & 1) + l4)) & 1u) ? -127 : 127;
		}
	}

	// =================== decode_sch (ms_rx_lower.cpp:59-100), in the waves that hold an SCH slot ===================
	unsigned bsic = 0u, t1 = 0u, t2 = 0u, t3p = 0u;
	int sfn = -1;
	bool ok = false;
	if (__ballot(kind == TRXHIP_MS_KIND_SCH) != 0ull) {            // wave-uniform
		ok = ss_decode_sch(ones, dec_all, lane, bsic, t1, t2, t3p, sfn);
		ok = ok && kind == TRXHIP_MS_KIND_SCH;
	}

	// =================== the indication record (ms_upper.cpp:194-200, :272-274, :288-297) ===================
	if (live && l4 == 0) {
		uint32_t w0, w1;
		ms_slot_words<STREAM>(slots, sa, bme, w0, w1);
		const float pow = __int_as_float(nf.y);
		const int fl = (nf.x >> 16) & 0xff;
		trxhip_ms_burst_ind r;
		r.fn = w0;
		r.tn = (uint8_t)(w1 & 0xffu);
		r.kind = (uint8_t)kind;
		r.sent = (uint8_t)((nf.x >> 8) & 1);
		r.flags = (uint8_t)fl;
		r.rssi = 0;
		if (kind == TRXHIP_MS_KIND_SCH)
			r.rssi = 10;                                           // RSSI = 10 (:197)
		if (kind == TRXHIP_MS_KIND_NB && mt.x > 0 && !(fl & TRXHIP_MS_IND_SILENT)) {
			const float avg = sqrtf(pow);                          // :211
			r.rssi = (int16_t)(int)floor(20.0 * log10((double)(rx_full_scale / avg)));   // :272: unsigned / float, then log10(double)
		}
		r.toa256 = 0;                                              // (int)round(0) (:274), timingOffset = 0 (:198)
		r.start = mt.z;
		r.corr_max = __int_as_float(mt.w);
		r.pow = pow;
		r.sch_fn = ok ? sfn : -1;
		r.sch_rc = ok ? 1 : 0;
		r.sch_bsic = ok ? (uint8_t)bsic : 0;
		r.reserved[0] = r.reserved[1] = 0;
		ind[bme] = r;
		// continuous sch tracking, only update if off too much (ms_rx_lower.cpp:199-203): temp_ts_corr_offset += -start
		if (STREAM && sa.corr && ok && (mt.z > 1 || mt.z < -1))
			atomicAdd(sa.corr, -mt.z);
	}
}

template <bool I16, bool STREAM>
__global__ void __launch_bounds__(SS_WPB * WAVE)
ms_rx_kernel(const void *__restrict__ iq, size_t slot_stride, const trxhip_ms_slot *__restrict__ slots,
	     trxhip_ms_burst_ind *__restrict__ ind, int8_t *__restrict__ bits, unsigned n_slots, float scale, float rx_full_scale,
	     const trx_mss_stream sa)
{
	const int wave = uni((int)(threadIdx.x >> 6));
	const unsigned q0 = (blockIdx.x * SS_WPB + wave) * VA_BPW;     // first slot of this wave
	ms_rx_wave<I16, STREAM>(iq, slot_stride, slots, ind, bits, n_slots, scale, rx_full_scale, sa, wave, q0);
}

// THE GROUP FORM (trxhip_ms_group_*): the pulls of many streams in one launch.  A wave's four slots belong to one member: the wave
// finds its entry in the table by its first wave (wave-uniform loads), and from there on it is the stream form on that member's
// chunk, descriptor and outputs.  A member's last wave has idle rows, as the batch tail has.
template <bool I16>
__global__ void __launch_bounds__(SS_WPB * WAVE)
ms_rx_group_kernel(const trx_mss_member *__restrict__ tab, unsigned n_entries, unsigned n_waves, float scale, float rx_full_scale)
{
	const int wave = uni((int)(threadIdx.x >> 6));
	const unsigned gw = blockIdx.x * SS_WPB + wave;
	if (gw >= n_waves)
		return;
	unsigned lo = 0, hi = n_entries;                               // tab[lo].first_wave <= gw < tab[hi].first_wave
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) >> 1;
		if (tab[mid].first_wave <= gw)
			lo = mid;
		else
			hi = mid;
	}
	const trx_mss_member *e = tab + lo;
	const trx_mss_stream sa = e->sa;
	const unsigned n_slots = e->n_slots;
	const unsigned q0 = (gw - e->first_wave) * VA_BPW;
	ms_rx_wave<I16, true>(e->chunk, (size_t)MS_SLOT, nullptr, e->ind, e->bits, n_slots, scale, rx_full_scale, sa, wave, q0);
}

// the rotating instances of the two: the launch's oscillator as an argument, the entries' beside the table
template <bool I16>
__global__ void __launch_bounds__(SS_WPB * WAVE)
ms_rx_nco_kernel(const void *__restrict__ iq, trxhip_ms_burst_ind *__restrict__ ind, int8_t *__restrict__ bits, unsigned n_slots, float scale,
		 float rx_full_scale, const trx_mss_stream sa, const trx_nco_slot o, const float *__restrict__ nco_tab)
{
	const int wave = uni((int)(threadIdx.x >> 6));
	const unsigned q0 = (blockIdx.x * SS_WPB + wave) * VA_BPW;
	const ms_rx_nco nco = { o, nco_tab };
	ms_rx_wave<I16, true, true>(iq, (size_t)MS_SLOT, nullptr, ind, bits, n_slots, scale, rx_full_scale, sa, wave, q0, nco);
}

template <bool I16>
__global__ void __launch_bounds__(SS_WPB * WAVE)
ms_rx_group_nco_kernel(const trx_mss_member *__restrict__ tab, unsigned n_entries, unsigned n_waves, float scale, float rx_full_scale,
		       const trx_nco_slot *__restrict__ osc, const float *__restrict__ nco_tab)
{
	const int wave = uni((int)(threadIdx.x >> 6));
	const unsigned gw = blockIdx.x * SS_WPB + wave;
	if (gw >= n_waves)
		return;
	unsigned lo = 0, hi = n_entries;                               // tab[lo].first_wave <= gw < tab[hi].first_wave
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) >> 1;
		if (tab[mid].first_wave <= gw)
			lo = mid;
		else
			hi = mid;
	}
	const trx_mss_member *e = tab + lo;
	const trx_mss_stream sa = e->sa;
	const unsigned n_slots = e->n_slots;
	const unsigned q0 = (gw - e->first_wave) * VA_BPW;
	const ms_rx_nco nco = { osc[lo], nco_tab };
	ms_rx_wave<I16, true, true>(e->chunk, (size_t)MS_SLOT, nullptr, e->ind, e->bits, n_slots, scale, rx_full_scale, sa, wave, q0, nco);
}

extern "C" int trx_launch_ms_rx(const void *d_iq, int i16, size_t slot_stride, const trxhip_ms_slot *d_slots, trxhip_ms_burst_ind *d_ind,
				int8_t *d_bits, size_t n_slots, float scale, float rx_full_scale, hipStream_t stream)
{
	if (n_slots == 0)
		return 0;
	const size_t per_block = SS_WPB * VA_BPW;
	const size_t grid = (n_slots + per_block - 1) / per_block;
	const trx_mss_stream none = {};
	if (i16)
		hipLaunchKernelGGL((ms_rx_kernel<true, false>), dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_iq, slot_stride, d_slots,
				   d_ind, d_bits, (unsigned)n_slots, scale, rx_full_scale, none);
	else
		hipLaunchKernelGGL((ms_rx_kernel<false, false>), dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_iq, slot_stride, d_slots,
				   d_ind, d_bits, (unsigned)n_slots, scale, rx_full_scale, none);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// the stream form: n_slots slots of one pull, described by sa (trx_ms_sched.h); d_chunk: the caller's chunk
extern "C" int trx_launch_ms_rx_stream(const void *d_chunk, int i16, const trx_mss_stream *sa, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
				       size_t n_slots, float scale, float rx_full_scale, hipStream_t stream)
{
	if (n_slots == 0)
		return 0;
	const size_t per_block = SS_WPB * VA_BPW;
	const size_t grid = (n_slots + per_block - 1) / per_block;
	if (i16)
		hipLaunchKernelGGL((ms_rx_kernel<true, true>), dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_chunk, (size_t)MS_SLOT,
				   nullptr, d_ind, d_bits, (unsigned)n_slots, scale, rx_full_scale, *sa);
	else
		hipLaunchKernelGGL((ms_rx_kernel<false, true>), dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_chunk, (size_t)MS_SLOT,
				   nullptr, d_ind, d_bits, (unsigned)n_slots, scale, rx_full_scale, *sa);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

// the group form: n_waves waves over the n_entries members of d_tab (trx_ms_sched.h)
extern "C" int trx_launch_ms_rx_group(const trx_mss_member *d_tab, int i16, size_t n_entries, size_t n_waves, float scale, float rx_full_scale,
				      hipStream_t stream)
{
	if (n_entries == 0 || n_waves == 0)
		return 0;
	if (n_entries > n_waves || n_waves > 0x7fffffffu)
		return TRXHIP_EINVAL;
	const size_t grid = (n_waves + SS_WPB - 1) / SS_WPB;
	if (i16)
		hipLaunchKernelGGL((ms_rx_group_kernel<true>), dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_tab, (unsigned)n_entries,
				   (unsigned)n_waves, scale, rx_full_scale);
	else
		hipLaunchKernelGGL((ms_rx_group_kernel<false>), dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_tab, (unsigned)n_entries,
				   (unsigned)n_waves, scale, rx_full_scale);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
extern "C" int trx_launch_ms_rx_stream_nco(const void *d_chunk, int i16, const trx_mss_stream *sa, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
					   size_t n_slots, float scale, float rx_full_scale, const trx_nco_slot *nco, const float *d_nco_tab,
					   hipStream_t stream)
{
	if (n_slots == 0)
		return 0;
	if (!nco || !d_nco_tab)
		return TRXHIP_EINVAL;
	const size_t per_block = SS_WPB * VA_BPW;
	const size_t grid = (n_slots + per_block - 1) / per_block;
	if (i16)
		hipLaunchKernelGGL(ms_rx_nco_kernel<true>, dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_chunk, d_ind, d_bits,
				   (unsigned)n_slots, scale, rx_full_scale, *sa, *nco, d_nco_tab);
	else
		hipLaunchKernelGGL(ms_rx_nco_kernel<false>, dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_chunk, d_ind, d_bits,
				   (unsigned)n_slots, scale, rx_full_scale, *sa, *nco, d_nco_tab);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" int trx_launch_ms_rx_group_nco(const trx_mss_member *d_tab, int i16, size_t n_entries, size_t n_waves, float scale,
					  float rx_full_scale, const trx_nco_slot *d_nco, const float *d_nco_tab, hipStream_t stream)
{
	if (n_entries == 0 || n_waves == 0)
		return 0;
	if (n_entries > n_waves || n_waves > 0x7fffffffu || !d_nco || !d_nco_tab)
		return TRXHIP_EINVAL;
	const size_t grid = (n_waves + SS_WPB - 1) / SS_WPB;
	if (i16)
		hipLaunchKernelGGL(ms_rx_group_nco_kernel<true>, dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_tab, (unsigned)n_entries,
				   (unsigned)n_waves, scale, rx_full_scale, d_nco, d_nco_tab);
	else
		hipLaunchKernelGGL(ms_rx_group_nco_kernel<false>, dim3((unsigned)grid), dim3(SS_WPB * WAVE), 0, stream, d_tab, (unsigned)n_entries,
				   (unsigned)n_waves, scale, rx_full_scale, d_nco, d_nco_tab);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}
static_assert(TRX_MS_RX_SLOTS_PER_WAVE == VA_BPW, "slots per wave");
static_assert(sizeof(trx_mss_member) == 64, "table entry");
