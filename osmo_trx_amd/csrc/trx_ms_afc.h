// trx_ms_afc.h -- what the MS-side FCCH frequency-offset measurement shares between the slot scheduler (trx_ms_sched.hip, host) and
// its kernels (trx_ms_afc.hip, device), written once for both:
//   gsm_fcch_check_ts()            ms/sch.c:100-116              which of a pull's slots are FCCH slots, by arithmetic
//   gsm_fcch_offset()'s constants  ms/sch.c:206-207, :255-258, :292
// and the job a member's pull hands to the kernel, as an argument (the single object) or in the pull's table (a group).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/trxhip.h"
#include "trx_ms_sched.h"

#if defined(__HIPCC__)
#define TRX_AFC_HD __host__ __device__
#else
#define TRX_AFC_HD
#endif

#define TRX_AFC_START 52                   /* FCCH_TAIL_BITS_LEN + 10 * 4 = 3 * 4 + 10 * 4, :206, :292 */
#define TRX_AFC_L1    3                    /* :255 */
#define TRX_AFC_L2    32                   /* :256 */
#define TRX_AFC_N     92                   /* N1 = N2, :257-258 */
#define TRX_AFC_LAST  (TRX_AFC_START + TRX_AFC_L2 + TRX_AFC_N - 1)     /* 175: the last sample read */
#define TRX_AFC_RING  TRXHIP_MS_AFC_RING

/* FCCH frames (FN % 51 in {0, 10, 20, 30, 40}) among the multiframe positions [0, p), p <= 51 */
TRX_AFC_HD inline unsigned trx_afc_before(unsigned p)
{
	const unsigned c = (p + 9u) / 10u;
	return c < 5u ? c : 5u;
}

/* the first slot with TN 0 among the slots from the clock (fn0, tn0) on, and its frame's position in the multiframe */
TRX_AFC_HD inline void trx_afc_origin(uint32_t fn0, int tn0, unsigned *d, unsigned *p0)
{
	*d = (unsigned)(8 - tn0) & 7u;
	*p0 = (unsigned)(((uint64_t)fn0 + (((unsigned)tn0 + *d) >> 3)) % 51u);     /* (the hyperframe is a multiple of 51) */
}

/* FCCH slots among the k slots from the clock (fn0, tn0) on */
TRX_AFC_HD inline uint64_t trx_afc_count(uint32_t fn0, int tn0, uint64_t k)
{
	unsigned d, p0;
	trx_afc_origin(fn0, tn0, &d, &p0);
	if (d >= k)
		return 0;
	const uint64_t end = p0 + ((k - d + 7) >> 3);              /* the frames [p0, end) of a multiframe that repeats */
	return end / 51u * 5u + trx_afc_before((unsigned)(end % 51u)) - trx_afc_before(p0);
}

/* FCCH slot j of them (j < trx_afc_count()): its index among the slots, and the frames it lies behind fn0's */
TRX_AFC_HD inline uint64_t trx_afc_slot(uint32_t fn0, int tn0, uint64_t j, uint64_t *frames)
{
	unsigned d, p0;
	trx_afc_origin(fn0, tn0, &d, &p0);
	const uint64_t q = j + trx_afc_before(p0);                 /* the q-th FCCH frame from the multiframe's start */
	const uint64_t f = q / 5u * 51u + q % 5u * 10u - p0;        /* frames behind the first TN 0 */
	*frames = f + (((unsigned)tn0 + d) >> 3);
	return d + 8u * f;
}

/* A member's AFC state on the device: the count of FCCH slots measured, the last record, and the last TRX_AFC_RING measurements,
 * measurement c at ring[c % TRX_AFC_RING].  The count only counts slots: the host keeps it as well */
struct trx_afc_state {
	uint64_t count;
	trxhip_ms_fcch last;
	trxhip_ms_afc_entry ring[TRX_AFC_RING];
};

/* The AFC work of one member in one pull.  The member's slots are the receiver's: slot 0 from edge_row where that is set, the
 * others where they lie in the chunk at sample first + (k - (edge_row != NULL)) * 625; slot 0 has the clock (fn0, tn0).  A wave
 * measures one FCCH slot: wave w serves the job with the largest first_wave <= w, and its FCCH slot w - first_wave, of n_fcch.
 * count: the state's before the pull.  64 bytes */
struct trx_afc_job {
	const void     *chunk;
	const void     *edge_row;
	int64_t         first;
	trx_afc_state  *state;
	trxhip_ms_fcch *out;           /* the caller's d_fcch row of this member (slot k at out[k]), or NULL */
	uint64_t        count;
	uint32_t        n_fcch;
	uint32_t        first_wave;
	uint32_t        fn0;
	uint8_t         tn0, reserved[3];
};
