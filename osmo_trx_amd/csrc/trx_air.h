// trx_air.h -- the air interface's integer arithmetic, written once for the host object and for the kernels of trx_air.hip.
// include/trxhip.h ("the air interface") states the contract; here it is expression by expression, behind the oscillator of
// trx_ms_nco.h (phase, phasor, rotation), which is used as it is:
//   contribution  c = rint(y * g256) per component, round-half-even to a 32-bit integer; g256 = gain * 256.0f, 0 <= gain <= 16
//   noise         s(seed, lane, ts) = the four bytes of a murmur3-finalised hash of (seed, lane, ts) summed, minus 510;
//                 nq = (scale * s + 128) >> 8, scale = llrint(rms * 65536 / sqrt(21845))
//   output        clamp((acc + 128) >> 8, -32768, 32767), arithmetic shift
// and for a path with rays (include/trxhip.h, "multipath rays"):
//   ray phase     p_r(ts) = phase_at_0 + (uint32_t)ts * (uint32_t)inc, phase_at_0 = phase - (uint32_t)ts_set * (uint32_t)inc
//   ray           c_r = trx_air_path(tab, x at ts - delay, p_r(ts), gain * 256.0f), as a path
//   path          the exact integer sum of c_r over its rays; |c_r| < 2^28 at int16 input, 64 bits carry every sum
#pragma once
#include <math.h>
#include <stdint.h>

#include "trx_ms_nco.h"

#define TRX_AIR_MAX_MEMBERS 4096
#define TRX_AIR_MAX_DELAY   65536u
#define TRX_AIR_MAX_GAIN    16.0f
#define TRX_AIR_MAX_RMS     8192.0
#define TRX_AIR_UL_RX       4096u              /* the BTS's receiver: lanes 8192 and 8193 */
#define TRX_AIR_NOISE_SIGMA 147.80054127099805 /* sqrt(21845): four uniform bytes, 4 * (256^2 - 1) / 12 */

/* what a call hands its kernels per path: 16 bytes */
struct trx_air_row {
	uint32_t phase0;           /* the oscillator's phase at the window's first_ts */
	int32_t  inc;
	float    g256;
	uint32_t delay;
};

/* a receiver's noise, beside the path rows of a downlink table: 16 bytes */
struct trx_air_rx {
	int32_t  scale;
	uint32_t key_re, key_im;   /* trx_air_lane_key of the lanes 2 rx and 2 rx + 1 */
	uint32_t reserved;
};

#define TRX_AIR_MAX_RAYS 64

/* one ray of a direction's resident list (a plain member of such a direction is one entry): 32 bytes.  The row does not depend
 * on the window: the phase of output sample ts is phase_at_0 + (uint32_t)ts * inc.  A ray with inc == 0 carries its phasor,
 * trx_nco_phasor(tab, phase_at_0) made on the host from the same tables, and reads no table on the device */
struct trx_air_ray {
	uint32_t phase_at_0;
	int32_t  inc;
	float    g256;
	uint32_t delay;
	uint32_t row;              /* the source row: the member on the uplink, 0 on the downlink */
	float    rc, rs;           /* inc == 0 only */
	uint32_t reserved;
};

/* a member's entries in the list, for the downlink: 8 bytes */
struct trx_air_span {
	uint32_t first, count;
};

/* phase_at_0 of an oscillator that stands at acc at ts_ref */
inline uint32_t trx_air_phase_at_0(uint32_t acc, int64_t ts_ref, int32_t inc) { return acc - (uint32_t)(uint64_t)ts_ref * (uint32_t)inc; }

/* one int16 sample */
struct alignas(4) trx_air_s16 {
	int16_t re, im;
};

/* a window of one direction: n samples from first_ts on.  The source's last H samples in front of it lie in a ring per source
 * row, the sample with timestamp ts at (ts - start_ts) mod H, start_ts the direction's first sample; p0 is first_ts's place and
 * avail = min(first_ts - start_ts, H) says how many of them exist */
struct trx_air_win {
	int64_t  first_ts;
	uint32_t n, H, p0, avail;
};

/* the source sample j of the window, j >= -H: from the row, from the ring in front of it, or 0 in front of the first sample */
TRX_NCO_HD inline trx_air_s16 trx_air_fetch(const trx_air_s16 *row, const trx_air_s16 *ring, const trx_air_win &w, int64_t j)
{
	if (j >= 0)
		return row[j];
	if (-j > (int64_t)w.avail)
		return trx_air_s16{0, 0};
	uint32_t q = w.p0 + w.H - (uint32_t)(-j);
	if (q >= w.H)
		q -= w.H;
	return ring[q];
}

/* y (the rotated sample, one component) times the gain, rounded half-even.  |y| <= 46342 and g256 <= 4096: |c| < 2^31 */
TRX_NCO_HD inline int32_t trx_air_contrib(float y, float g256)
{
	const float v = y * g256;
	return (int32_t)rintf(v);
}

/* the source sample (xr, xi) through the path {p, g256}: rotation, then the contribution per component */
TRX_NCO_HD inline void trx_air_path(const float *tab, int16_t xr, int16_t xi, uint32_t p, float g256, int32_t *cr, int32_t *ci)
{
	float rc, rs, yr, yi;
	trx_nco_phasor(tab, p, &rc, &rs);
	trx_nco_rotate((float)xr, (float)xi, rc, rs, &yr, &yi);
	*cr = trx_air_contrib(yr, g256);
	*ci = trx_air_contrib(yi, g256);
}

/* p_r(ts) of a ray: a function of the absolute timestamp alone, modulo 2^32 */
TRX_NCO_HD inline uint32_t trx_air_ray_phase(uint32_t phase_at_0, int32_t inc, int64_t ts)
{
	return phase_at_0 + (uint32_t)(uint64_t)ts * (uint32_t)inc;
}

TRX_NCO_HD inline uint32_t trx_air_fmix32(uint32_t h)
{
	h ^= h >> 16;
	h *= 0x85ebca6bu;
	h ^= h >> 13;
	h *= 0xc2b2ae35u;
	h ^= h >> 16;
	return h;
}

/* the part of the key that belongs to the lane alone */
TRX_NCO_HD inline uint32_t trx_air_lane_key(uint32_t seed, uint32_t lane) { return trx_air_fmix32(seed ^ trx_air_fmix32(lane)); }

/* s of a lane (its key from trx_air_lane_key) at ts: -510 .. 510 */
TRX_NCO_HD inline int32_t trx_air_noise_s(uint32_t lane_key, int64_t ts)
{
	const uint32_t lo = (uint32_t)(uint64_t)ts, hi = (uint32_t)((uint64_t)ts >> 32);
	const uint32_t key = lane_key + hi * 0x9e3779b9u;
	const uint32_t w = trx_air_fmix32(trx_air_fmix32(lo) + key);
	return (int32_t)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)) - 510;
}

/* scale <= llrint(8192 * 65536 / 147.8) = 3632402, |s| <= 510: the product stays below 2^31 */
TRX_NCO_HD inline int32_t trx_air_nq(int32_t scale, int32_t s) { return (scale * s + 128) >> 8; }

/* 0, or TRXHIP_EINVAL for rms outside 0 .. 8192 and NaN */
inline int trx_air_noise_scale(double rms, int32_t *scale)
{
	if (!(rms >= 0.0 && rms <= TRX_AIR_MAX_RMS))
		return TRXHIP_EINVAL;
	*scale = (int32_t)llrint(rms * 65536.0 / TRX_AIR_NOISE_SIGMA);
	return 0;
}

TRX_NCO_HD inline int16_t trx_air_out(int64_t acc)
{
	const int64_t v = (acc + 128) >> 8;
	return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}
