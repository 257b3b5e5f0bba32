// trx_ms_agc.h -- the arithmetic of the MS-side receive gain control, written once for the host and for the device: the plan-only
// objects (trx_ms_sched.hip, ctx == NULL) and the kernels (trx_ms_agc.hip) run the same code.
//   normed_abs_sum()               ms/ms.h:116-126               the final division (the sum itself: trx_ms_agc.hip)
//   ms_trx::maybe_update_gain()    ms/ms_rx_lower.cpp:101-126    one step of runmean, the decision at gain_check == 159
//   search_for_sch()'s level gate  ms/ms_rx_lower.cpp:333-347
// Every float operation is rounded on its own: the reference is generic C++ without contraction, and hipcc would make an FMA of
// runmean * n - 1 where it is allowed to.
// and the entries the AGC launches of a pull take, as arguments (the single object) or from the pull's table (a group).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/trxhip.h"

#if defined(__HIPCC__)
#define TRX_AGC_HD __host__ __device__
#else
#define TRX_AGC_HD
#endif

#define TRX_AGC_WINDOW   160               /* avgburst_num = 8 * 20, :104 */
#define TRX_AGC_MAX_GAIN 60.0f             /* :118, :338 */
#define TRX_AGC_GATE_STEP 4.0f             /* setRxGain(rxgain + 4), :343 */
#define TRX_AGC_EXACT    16777216u         /* 2^24: every integer up to it is a float */
#define TRX_AGC_RING     TRXHIP_MS_AGC_RING

TRX_AGC_HD inline float trx_agc_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __fmul_rn(a, b);
#else
	volatile float r = a * b;
	return r;
#endif
}

TRX_AGC_HD inline float trx_agc_add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __fadd_rn(a, b);
#else
	volatile float r = a + b;
	return r;
#endif
}

TRX_AGC_HD inline float trx_agc_sub(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __fsub_rn(a, b);
#else
	volatile float r = a - b;
	return r;
#endif
}

TRX_AGC_HD inline float trx_agc_div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __fdiv_rn(a, b);
#else
	volatile float r = a / b;
	return r;
#endif
}

/* sum /= len * len_mul (ms.h:124): n_values = 2 * samples, an int the division converts to float */
TRX_AGC_HD inline float trx_agc_level(float sum, uint32_t n_values) { return trx_agc_div(sum, (float)(int32_t)n_values); }

/* runmean = gain_check ? (runmean * (gain_check + 2) - 1 + sum) / (gain_check + 2) : sum (:110); gain_check 0..159 */
TRX_AGC_HD inline float trx_agc_step(float runmean, int gain_check, float sum)
{
	if (!gain_check)
		return sum;
	const float n = (float)(gain_check + 2);
	return trx_agc_div(trx_agc_add(trx_agc_sub(trx_agc_mul(runmean, n), 1.0f), sum), n);
}

/* The decision at gain_check == 159 (:114-118).  gainoffset is `auto` from a comparison, a bool; its first value (:114) is
 * overwritten (:115).  full_scale: rxFullScale, unsigned.  Returns newgain; *applied: newgain != rxgain && newgain <= 60 */
TRX_AGC_HD inline bool trx_agc_gainoffset(float runmean, uint32_t full_scale)
{
	bool gainoffset = runmean < (float)(full_scale / 4u ? 4 : 2);
	gainoffset = runmean < (float)(full_scale / 2u ? 2 : 1);
	return gainoffset;
}

TRX_AGC_HD inline float trx_agc_decide(float runmean, float rx_gain, uint32_t full_scale, int *applied)
{
	const uint32_t rx_max_cutoff = (full_scale * 2u) / 3u;
	const float off = (float)(int)trx_agc_gainoffset(runmean, full_scale);
	const float newgain = runmean < (float)rx_max_cutoff ? trx_agc_add(rx_gain, off) : trx_agc_sub(rx_gain, off);
	*applied = newgain != rx_gain && newgain <= TRX_AGC_MAX_GAIN;
	return newgain;
}

/* the gate (:334-344): 1 = search (sum > rxFullScale / 8 || rxgain >= 60), 0 = raise the gain to *new_gain = rxgain + 4 */
TRX_AGC_HD inline int trx_agc_gate(float level, uint32_t full_scale, float rx_gain, float *new_gain)
{
	const uint32_t target_val = full_scale / 8u;
	*new_gain = rx_gain;
	if (level > (float)target_val || rx_gain >= TRX_AGC_MAX_GAIN)
		return 1;
	*new_gain = trx_agc_add(rx_gain, TRX_AGC_GATE_STEP);
	return 0;
}

/* rxFullScale as the reference holds it (unsigned int) from the objects' float */
TRX_AGC_HD inline uint32_t trx_agc_full_scale(float rx_full_scale)
{
	return rx_full_scale >= 4294967040.0f ? 0xffffff00u : (uint32_t)rx_full_scale;
}

/* A member's AGC state: the function statics of maybe_update_gain() (gain_check, runmean), rxgain, counters, and the last
 * TRX_AGC_RING decisions, record d at ring[d % TRX_AGC_RING].  On the device for a GPU object, on the host for a plan-only one */
struct trx_agc_state {
	float    rx_gain, runmean;
	uint32_t gain_check, reserved;
	uint64_t slots, decisions, applied;
	trxhip_ms_agc_record ring[TRX_AGC_RING];
};

/* One decision into the state: the window that closes at slot counter `slot` with (runmean, sum) */
TRX_AGC_HD inline void trx_agc_close(trx_agc_state *s, uint64_t slot, float runmean, float sum, uint32_t full_scale)
{
	int applied;
	const float newgain = trx_agc_decide(runmean, s->rx_gain, full_scale, &applied);
	trxhip_ms_agc_record *r = &s->ring[s->decisions % TRX_AGC_RING];
	r->slot = slot;
	r->runmean = runmean;
	r->sum = sum;
	r->old_gain = s->rx_gain;
	r->new_gain = newgain;
	r->applied = (uint32_t)applied;
	r->reserved = 0;
	if (applied) {
		s->rx_gain = newgain;
		s->applied++;
	}
	s->decisions++;
}

/* maybe_update_gain() over n levels in order, one call per slot: what the plan-only objects run, and what the two gain kernels
 * compute between them in pieces */
TRX_AGC_HD inline void trx_agc_run(trx_agc_state *s, const float *levels, size_t n, uint32_t full_scale)
{
	for (size_t k = 0; k < n; k++) {
		s->runmean = trx_agc_step(s->runmean, (int)s->gain_check, levels[k]);
		if (s->gain_check == TRX_AGC_WINDOW - 1) {
			trx_agc_close(s, s->slots + k, s->runmean, levels[k], full_scale);
			s->runmean = 0.0f;                             /* :123 */
		}
		s->gain_check = (s->gain_check + 1) % TRX_AGC_WINDOW;
	}
	s->slots += n;
}

/* pieces of n slots behind gain_check gc: the rest of the open window (or the whole pull), then windows of 160 */
TRX_AGC_HD inline uint32_t trx_agc_pieces(uint32_t gc, uint64_t n)
{
	const uint64_t rest = TRX_AGC_WINDOW - gc;
	return n <= rest ? 1u : (uint32_t)(1 + (n - rest + TRX_AGC_WINDOW - 1) / TRX_AGC_WINDOW);
}

/* The AGC work of one member in one pull: the level kernel's stream / group form and the two gain kernels read it -- as a kernel
 * argument (the single object) or from the pull's table behind the join entries (a group).  The member's n_slots slots are the
 * receiver's: slot 0 from edge_row where that is set, the others where they lie in the chunk at sample first + (k - (edge_row !=
 * NULL)) * 625.  A wave of the level kernel measures one slot: wave w serves the entry with the largest first_wave <= w.
 * first_piece: the same for the lanes of the piece kernel, trx_agc_pieces(gain_check, n_slots) of them; gain_check: the state's
 * before the pull -- a counter of slots, which the host keeps as well.  64 bytes */
struct trx_agc_entry {
	const void    *chunk;
	const void    *edge_row;
	int64_t        first;
	trx_agc_state *state;
	float         *level;          /* the caller's d_level row of this member, or NULL */
	float         *work;           /* n_slots levels, then 2 floats {runmean, sum} per piece */
	uint32_t       n_slots;
	uint32_t       first_wave;
	uint32_t       first_piece;
	uint32_t       gain_check;
};
