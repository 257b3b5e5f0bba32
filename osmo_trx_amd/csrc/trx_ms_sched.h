// trx_ms_sched.h -- what the MS-side downlink slot scheduler (trx_ms_sched.hip) and the stream form of the MS receiver
// (trx_ms_rx.hip) share, written once for the host and for the device:
//   GSM::Time::incTN()                     GSM/GSMCommon.h:141-150     the clock k slots later
//   gsm_fcch_check_ts / gsm_sch_check_ts   ms/sch.c:100-139            the slot's kind (as trxhip.h's TRXHIP_MS_KIND_*)
// and the arguments the stream instance of ms_rx_kernel takes instead of slot records.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/trxhip.h"

#if defined(__HIPCC__)
#define TRX_MSS_HD __host__ __device__
#else
#define TRX_MSS_HD
#endif

#define TRX_MSS_SLOT       625             /* ONE_TS_BURST_LEN, ms/ms.h:50 */
#define TRX_MSS_REM_STRIDE 640u            /* samples of one half of the partial-slot area (it holds < 625) */
#define TRX_MSS_HYPERFRAME 2715648u        /* GSM::gHyperframe: a multiple of 51 */

/* the clock k incTN(1) behind (fn0, tn0) */
TRX_MSS_HD inline void trx_mss_clock_add(uint32_t fn0, int tn0, uint64_t k, uint32_t *fn, int *tn)
{
	const uint64_t q = (uint64_t)tn0 + k;
	*tn = (int)(q & 7);
	*fn = (uint32_t)(((uint64_t)fn0 + (q >> 3)) % TRX_MSS_HYPERFRAME);
}

/* gsm_sch_check_ts(tn, fn), ms/sch.c:118-139 */
TRX_MSS_HD inline bool trx_mss_is_sch(uint32_t fn, int tn)
{
	const unsigned fn51 = fn % 51u;
	return tn == 0 && fn51 % 10u == 1 && fn51 <= 41u;
}

/* TRXHIP_MS_KIND_* of a slot, tn <= 7 (what ms_rx_kernel computes from a slot record) */
TRX_MSS_HD inline int trx_mss_kind(uint32_t fn, int tn, unsigned tsc)
{
	const unsigned fn51 = fn % 51u;
	if (tn == 0 && fn51 % 10u == 0 && fn51 <= 40u)
		return TRXHIP_MS_KIND_FCCH;
	if (trx_mss_is_sch(fn, tn))
		return TRXHIP_MS_KIND_SCH;
	return tsc > 7 ? TRXHIP_MS_KIND_BAD : TRXHIP_MS_KIND_NB;
}

/* SCH slots among the k slots from the clock (fn0, tn0) on: the frames whose TN 0 lies among them, with FN % 51 in
 * {1, 11, 21, 31, 41} -- whole multiframes by division (the hyperframe is a multiple of 51), the rest frame by frame */
TRX_MSS_HD inline uint64_t trx_mss_count_sch(uint32_t fn0, int tn0, uint64_t k)
{
	const unsigned d = (unsigned)(8 - tn0) & 7u;               /* the first slot with TN 0 */
	if (d >= k)
		return 0;
	const uint64_t frames = (k - d + 7) >> 3;
	const unsigned first = (unsigned)(((uint64_t)fn0 + (((unsigned)tn0 + d) >> 3)) % 51u);
	uint64_t n = frames / 51u * 5u;
	for (unsigned i = 0; i < (unsigned)(frames % 51u); i++)
		n += trx_mss_is_sch((first + i) % 51u, 0);
	return n;
}

/* The stream form of ms_rx_kernel: slot b of the launch has the clock b incTN() behind (fn0, tn0), the cell's tsc, ACTIVE from
 * bit tn of `active`; it is read from edge_row when b == 0 and edge_row is set (the slot that straddles the carried partial slot
 * and the chunk), else where it lies in the chunk, at sample first + (b - (edge_row != NULL)) * 625. */
struct trx_mss_stream {
	const void *edge_row;
	int64_t     first;
	int32_t    *corr;              /* temp_ts_corr_offset of this pull, or NULL: tracking off */
	uint32_t    fn0;
	uint8_t     tn0, tsc, active, reserved;
};

/* The group form of ms_rx_kernel (trxhip_ms_group_*): a table of the members that have receiver work in this launch, in the order
 * of their waves.  A wave's VA_BPW slots belong to one member: wave w serves the entry with the largest first_wave <= w, whose
 * slots (w - first_wave) * VA_BPW .. are the stream form's with this entry's chunk, descriptor and outputs.  first_wave rises
 * strictly from 0; an entry has n_slots >= 1.  64 bytes */
struct trx_mss_member {
	const void            *chunk;      /* the member's chunk of this pull */
	trx_mss_stream         sa;         /* sa.corr: the member's own word of the group's correction words, or NULL */
	trxhip_ms_burst_ind   *ind;        /* where the entry's slot 0 goes */
	int8_t                *bits;       /* the same for the sbits, or NULL */
	uint32_t               n_slots;
	uint32_t               first_wave;
};

/* The join of one member: ms_join_kernel's argument (the single object), one block's table entry of ms_join_group_kernel.  64 bytes */
struct trx_mss_join {
	const void *in, *rem_in;
	void       *rem_out, *edge_row;
	uint64_t    tail_at;
	uint32_t    carried, keep, n_tail;
	int32_t     do_edge;
	uint64_t    reserved;
};
