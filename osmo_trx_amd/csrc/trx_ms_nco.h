// trx_ms_nco.h -- the MS-side numerically controlled oscillator, written once for the host (trx_ms_sched.hip's bookkeeping, the
// host-only exports) and for the device (trx_ms_nco.hip's batch kernel, the rotating instances of ms_rx_kernel in trx_ms_rx.hip).
// include/trxhip.h states the contract; here it is expression by expression:
//   phase      p(ts) = acc + (uint32_t)(ts - ts_ref) * (uint32_t)inc, modulo 2^32: a function of the absolute timestamp alone
//   increment  inc = (int32_t)llrint(hz * (2^32 / (13e6 / 12))), |hz| <= 500000
//   phasor     two tables of 1024 (cos, sin) pairs, coarse C[p >> 22] and fine F[(p >> 12) & 1023]; the low 12 bits are dropped;
//              r = (Cc Fc - Cs Fs, Cc Fs + Cs Fc), every product and sum rounded to float (-ffp-contract=off)
//   rotation   out = ((xr rc - xi rs) scale, (xr rs + xi rc) scale): rotation first, convert_and_scale's factor second
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/trxhip.h"

#if defined(__HIPCC__)
#define TRX_NCO_HD __host__ __device__
#else
#define TRX_NCO_HD
#endif

#define TRX_NCO_TAB      1024              /* entries of each table */
#define TRX_NCO_FLOATS   (4 * TRX_NCO_TAB) /* C then F, (cos, sin) pairs: 16 KB */
#define TRX_NCO_MAX_HZ   500000.0
#define TRX_NCO_SAMPLE_HZ (13e6 / 12.0)    /* 4 samples per symbol of 13e6 / 48 */

/* What a member's receiver entry of a pull carries beside it (the parallel array of the group's table, the stream form's kernel
 * argument): slot b of the entry, b counted behind the edge row, starts at phase0 + b * 625 * inc; the slot read from the edge
 * row starts at edge -- a correction of the cut (temp_ts_corr_offset) lies between that slot and the chunk's first, so the two
 * are not always 625 samples apart.  16 bytes */
struct trx_nco_slot {
	uint32_t phase0;
	int32_t  inc;
	uint32_t edge;
	uint32_t reserved;
};

/* a member's oscillator on the host */
struct trx_nco_state {
	int32_t  inc;
	uint32_t acc;              /* the phase at ts_ref */
	int64_t  ts_ref;
	double   hz;
	bool     enable;
};

TRX_NCO_HD inline uint32_t trx_nco_phase(uint32_t acc, int64_t ts_ref, int32_t inc, int64_t ts)
{
	return acc + (uint32_t)((uint64_t)ts - (uint64_t)ts_ref) * (uint32_t)inc;
}

/* 0, or TRXHIP_EINVAL for |hz| > 500000 and NaN */
inline int trx_nco_inc(double hz, int32_t *inc)
{
	if (!(fabs(hz) <= TRX_NCO_MAX_HZ))
		return TRXHIP_EINVAL;
	*inc = (int32_t)llrint(hz * (4294967296.0 / TRX_NCO_SAMPLE_HZ));
	return 0;
}

/* the two tables, host only: entries made in double and rounded to float.  The coarse table is its first quadrant turned three
 * times (a quarter turn of (c, s) is (-s, c)), so the entries 0, 256, 512 and 768 are (1, 0), (0, 1), (-1, 0), (0, -1) exactly;
 * 0.0f - x keeps a zero positive */
inline void trx_nco_tables(float *out)
{
	const double two_pi = 6.283185307179586476925286766559;
	float *c = out, *f = out + 2 * TRX_NCO_TAB;
	const int q = TRX_NCO_TAB / 4;
	for (int a = 0; a < q; a++) {
		const float co = (float)cos(two_pi * (double)a / (double)TRX_NCO_TAB);
		const float si = (float)sin(two_pi * (double)a / (double)TRX_NCO_TAB);
		c[2 * a] = co;
		c[2 * a + 1] = si;
		c[2 * (a + q)] = 0.0f - si;
		c[2 * (a + q) + 1] = co;
		c[2 * (a + 2 * q)] = 0.0f - co;
		c[2 * (a + 2 * q) + 1] = 0.0f - si;
		c[2 * (a + 3 * q)] = si;
		c[2 * (a + 3 * q) + 1] = 0.0f - co;
	}
	for (int b = 0; b < TRX_NCO_TAB; b++) {
		f[2 * b] = (float)cos(two_pi * (double)b / 1048576.0);
		f[2 * b + 1] = (float)sin(two_pi * (double)b / 1048576.0);
	}
}

/* the phasor of phase p from the tables (tab: TRX_NCO_FLOATS floats) */
TRX_NCO_HD inline void trx_nco_phasor(const float *tab, uint32_t p, float *rc, float *rs)
{
	const uint32_t a = p >> 22, b = (p >> 12) & (TRX_NCO_TAB - 1);
	const float cc = tab[2 * a], cs = tab[2 * a + 1];
	const float fc = tab[2 * TRX_NCO_TAB + 2 * b], fs = tab[2 * TRX_NCO_TAB + 2 * b + 1];
	const float t0 = cc * fc, t1 = cs * fs, t2 = cc * fs, t3 = cs * fc;
	*rc = t0 - t1;
	*rs = t2 + t3;
}

/* x times the phasor: (xr rc - xi rs, xr rs + xi rc) */
TRX_NCO_HD inline void trx_nco_rotate(float xr, float xi, float rc, float rs, float *yr, float *yi)
{
	const float t0 = xr * rc, t1 = xi * rs, t2 = xr * rs, t3 = xi * rc;
	*yr = t0 - t1;
	*yi = t2 + t3;
}

/* trxhip_ms_nco_*_set at the member's clock ts_now: the phase stays continuous across a change of frequency; switching on from
 * off starts at phase 0 */
inline void trx_nco_set(trx_nco_state *s, bool enable, double hz, int32_t inc, int64_t ts_now)
{
	s->acc = (s->enable && enable) ? trx_nco_phase(s->acc, s->ts_ref, s->inc, ts_now) : 0u;
	s->ts_ref = ts_now;
	s->inc = inc;
	s->hz = hz;
	s->enable = enable;
}
