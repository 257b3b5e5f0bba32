// trx_sch_common.h -- the device code that the MS-side receivers share: trx_sch_sync.hip (synchronisation bursts alone) and
// trx_ms_rx.hip (the slots of a cell: synchronisation and normal bursts).  The slot window and the per-wave LDS slice, convert_and_scale,
// the correlation on the 64-bit extended training sequence, the serial window recurrence as a DPP chain, and decode_sch().
#ifndef TRX_SCH_COMMON_H
#define TRX_SCH_COMMON_H
#include "trx_va_common.h"

#define SS_WPB 2                         // waves per workgroup of sch_sync_demod_kernel and ms_rx_kernel
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
	// "+&v": acc never shares q's register, not even where the compiler can prove acc == q on entry (carry == 0 and q >= 0)
	asm volatile(SS_STEP16 SS_STEP16 SS_STEP16 SS_STEP4 SS_STEP4 SS_STEP4 SS_STEP1 SS_STEP1 SS_STEP1 : "+&v"(acc) : "v"(q));
	carry = lane_val(acc, 63);
	return acc;
}

// the term the recurrence adds at lag i: p[i] while the first window fills (:206-208), then p[i] - p[i-20] (:212-213)
__device__ __forceinline__ float sch_scan_term(float p, float p20, int i)
{
	return (i < VA_FL) ? p : p - p20;
}

// 3GPP TS 45.003 4.7, the trellis of sch_next_output (sch.c:60-65): the cost of leaving state p with input u when the two soft
// bits are x0, x1 (a coded 0 expects +127, a coded 1 expects -127; cost |x - e|)
__device__ __forceinline__ int ss_branch(int p, int u, int x0, int x1)
{
	const int b0 = p & 1, b2 = (p >> 2) & 1, b3 = (p >> 3) & 1;
	const int c0 = u ^ b2 ^ b3, c1 = u ^ b0 ^ b2 ^ b3;
	return abs(x0 - (c0 ? -127 : 127)) + abs(x1 - (c1 ? -127 : 127));
}

// decode_sch (ms_rx_lower.cpp:59-100) for the four bursts of a wave, one decoder per row, on the trellis' output strings (ones:
// va_trellis).  dec_all: [4][16] 64-bit words of LDS.  Every lane of a row returns its row's parity check and parsed fields.
__device__ __forceinline__ bool ss_decode_sch(const unsigned (&ones)[5], unsigned long long *dec_all, int lane, unsigned &bsic,
					      unsigned &t1, unsigned &t2, unsigned &t3p, int &fn)
{
	const int row = lane >> 4, l4 = lane & 15;
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
	// gsm_sch_parse (sch.c:162-185) over sch_packed_info (:41-49): t1_hi[2] bsic[6] t1_md[8] t3p_hi[2] t2[5] t1_lo t3p_lo
	const unsigned w = (unsigned)ub;
	bsic = (w >> 2) & 63u;
	t1 = ((w >> 23) & 1u) | (((w >> 8) & 0xffu) << 1) | ((w & 3u) << 9);
	t2 = (w >> 18) & 31u;
	t3p = ((w >> 24) & 1u) | (((w >> 16) & 3u) << 1);
	// gsm_sch_to_fn (sch.c:142-159); the fields are unsigned here, so fn >= 0 always
	const int t3 = (int)t3p * 10 + 1;
	const int tt = (t3 < (int)t2) ? (t3 + 26) - (int)t2 : (t3 - (int)t2) % 26;
	fn = (int)t1 * 51 * 26 + tt * 51 + t3;
	return par == reg;
}
#endif
