// trx_rx_sched.h -- what the uplink burst scheduler (trx_rx_sched.hip) decides per channel and timeslot of the receive clock,
// written once for the device kernels and for the host (the plan-only object, trxhip_rx_sched_plan()):
//   GSM::Time::operator+=(int)            GSM/GSMCommon.h:152-159     burstTime = time + ul_fn_offset (Transceiver.cpp:690)
//   Transceiver::expectedCorrType()       Transceiver.cpp:513-601     with its three subslot tables
//   max_toa                               Transceiver.cpp:757-758
//   RadioInterface::driveReceiveRadio()   radioInterface.cpp:252-291   the slot cutter at 4 SPS (625) and at 1 SPS (157/156/156/156)
// and the per-pull device state the kernels share.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/trxhip.h"

#if defined(__HIPCC__)
#define TRX_RXS_HD __host__ __device__
#else
#define TRX_RXS_HD
#endif

#define TRX_RXS_MAX_CHANS  8
#define TRX_RXS_SLOT       625u            /* burstSize at 4 SPS, radioInterface.cpp:257-258 */
#define TRX_RXS_SLOT1_MAX  157u            /* the longer burstSize at 1 SPS, radioInterface.cpp:257-258 */
#define TRX_RXS_REM_STRIDE 640u            /* samples per channel of one half of the remainder area (it holds <= 625) */
#define TRX_RXS_NOISE_CNT  20              /* mNoises(NOISE_CNT), Transceiver.h:48, Transceiver.cpp:64 */
#define TRX_RXS_HYPERFRAME 2715648u        /* GSM::gHyperframe = 2048 * 26 * 51: a multiple of 26, 51, 52 and 102 */

/* What Transceiver keeps for expectedCorrType() and the head of pullRadioVector(): 88 bytes, handed to rx_plan_kernel by value
 * with every pull, so that a setter on the host never races a pull in flight and nothing is uploaded. */
struct trx_rxs_settings {
	uint8_t  chan_type[TRX_RXS_MAX_CHANS][8];  /* mStates[chan].chanType[tn], TRXHIP_COMB_* */
	uint8_t  handover[8];                      /* bit ss of [tn]: mHandover[tn][ss], one table for all channels (:150-153, :944-961) */
	uint8_t  muted;                            /* bit chan: mStates[chan].mMuted */
	uint8_t  version;                          /* bit chan: mVersionTRXD[chan] */
	uint8_t  ext_rach, egprs;                  /* cfg->ext_rach, cfg->egprs */
	uint8_t  tsc;                              /* mTSC */
	uint8_t  reserved[3];
	uint16_t max_toa_nb, max_toa_ab;           /* mMaxExpectedDelayNB / AB */
	int32_t  ul_fn_offset;                     /* cfg->ul_fn_offset */
};
static_assert(sizeof(trx_rxs_settings) == 88, "trx_rxs_settings layout");

/* the noise ring of one channel (RxChanState in host/trxPullRadioVector.cpp; noiseVector, radioVector.cpp:84-108) */
struct trx_rxs_noise {
	float    ring[TRX_RXS_NOISE_CNT];
	uint32_t itr;                              /* 0 .. 20, as noiseVector::itr */
	float    lev;                              /* mNoiseLev */
	uint32_t reserved[2];
};
static_assert(sizeof(trx_rxs_noise) == 96, "trx_rxs_noise layout");

/* GSM::Time::operator+=(int), GSMCommon.h:152-159; |step| < the hyperframe */
TRX_RXS_HD inline uint32_t trx_rxs_fn_add(uint32_t fn, int32_t step)
{
	int64_t v = (int64_t)fn + step;
	if (v < 0)
		v += TRX_RXS_HYPERFRAME;
	return (uint32_t)(v % TRX_RXS_HYPERFRAME);
}

/* expectedCorrType(), Transceiver.cpp:513-601.  fn, tn: burstTime */
TRX_RXS_HD inline int trx_rxs_expected_type(const trx_rxs_settings &st, int chan, uint32_t fn, int tn)
{
	static constexpr uint8_t tchh_subslot[26] = { 0,1,0,1,0,1,0,1,0,1,0,1,0,0,1,0,1,0,1,0,1,0,1,0,1,1 };
	static constexpr uint8_t sdcch4_subslot[102] = { 3,3,3,3,0,0,2,2,2,2,3,3,3,3,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,0,0,2,2,2,2,
							 3,3,3,3,0,0,0,0,0,0,1,1,1,1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,0,0,2,2,2,2 };
	static constexpr uint8_t sdcch8_subslot[102] = { 5,5,5,5,6,6,6,6,7,7,7,7,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,6,6,6,6,7,7,7,7,0,0,0,0,
							 1,1,1,1,2,2,2,2,3,3,3,3,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,6,6,6,6,7,7,7,7,4,4,4,4 };
	const unsigned ho = st.handover[tn];
	const int rach = st.ext_rach ? TRXHIP_EXT_RACH : TRXHIP_RACH;
	switch (st.chan_type[chan][tn]) {
	case TRXHIP_COMB_NONE:
		return TRXHIP_OFF;
	case TRXHIP_COMB_FILL:
		return TRXHIP_IDLE;
	case 1:                                                    /* I */
		return (ho & 1u) ? TRXHIP_RACH : TRXHIP_TSC;
	case 2:                                                    /* II */
		if (tchh_subslot[fn % 26] == 1)
			return TRXHIP_IDLE;
		return (ho & 1u) ? TRXHIP_RACH : TRXHIP_TSC;
	case 3:                                                    /* III */
		return ((ho >> tchh_subslot[fn % 26]) & 1u) ? TRXHIP_RACH : TRXHIP_TSC;
	case 4:                                                    /* IV */
	case 6:                                                    /* VI */
		return rach;
	case 5: {                                                  /* V */
		const unsigned mod51 = fn % 51;
		if ((mod51 <= 36 && mod51 >= 14) || mod51 == 4 || mod51 == 5 || mod51 == 45 || mod51 == 46)
			return rach;
		return ((ho >> sdcch4_subslot[fn % 102]) & 1u) ? TRXHIP_RACH : TRXHIP_TSC;
	}
	case 7:                                                    /* VII */
		if (fn % 51 <= 14 && fn % 51 >= 12)
			return TRXHIP_IDLE;
		return ((ho >> sdcch8_subslot[fn % 102]) & 1u) ? TRXHIP_RACH : TRXHIP_TSC;
	case 13: {                                                 /* XIII */
		const unsigned mod52 = fn % 52;
		if (mod52 == 12 || mod52 == 38)
			return TRXHIP_RACH;                            /* RACH is always 8-bit on PTCCH/U */
		if (mod52 == 25 || mod52 == 51)
			return TRXHIP_IDLE;
		return st.egprs ? TRXHIP_EDGE : TRXHIP_TSC;
	}
	case TRXHIP_COMB_LOOPBACK:
		if (fn % 51 <= 50 && fn % 51 >= 48)
			return TRXHIP_IDLE;
		return TRXHIP_TSC;
	default:                                                   /* VIII .. XII */
		return TRXHIP_OFF;
	}
}

/* Transceiver.cpp:757-758 */
TRX_RXS_HD inline unsigned trx_rxs_max_toa(const trx_rxs_settings &st, int type)
{
	return (type == TRXHIP_RACH || type == TRXHIP_EXT_RACH) ? st.max_toa_ab : st.max_toa_nb;
}

/* The burst parameters of one cut slot: its burstTime and what detectAnyBurst() is called with. */
struct trx_rxs_slot {
	uint32_t fn;
	uint8_t  tn, type, muted;
	uint16_t max_toa;
};

/* slot k of a pull whose first slot takes the receive clock (fn0, tn0): the clock k incTN() later (GSMCommon.h:141-150,
 * radioInterface.cpp:283-284), plus ul_fn_offset */
TRX_RXS_HD inline trx_rxs_slot trx_rxs_plan_slot(const trx_rxs_settings &st, int chan, uint32_t fn0, int tn0, uint64_t k)
{
	const uint64_t q = (uint64_t)tn0 + k;
	trx_rxs_slot p;
	p.tn = (uint8_t)(q & 7);
	p.fn = trx_rxs_fn_add((uint32_t)(((uint64_t)fn0 + (q >> 3)) % TRX_RXS_HYPERFRAME), st.ul_fn_offset);
	p.type = (uint8_t)trx_rxs_expected_type(st, chan, p.fn, p.tn);
	p.muted = (uint8_t)((st.muted >> chan) & 1u);
	p.max_toa = (uint16_t)trx_rxs_max_toa(st, p.type);
	return p;
}

/* A frame count M such that a TN of this combination has the same type at FN and FN + M (the moduli expectedCorrType() reads) */
TRX_RXS_HD inline unsigned trx_rxs_type_period(int comb)
{
	switch (comb) {
	case 2: case 3: return 26;
	case 5: case 7: return 102;
	case 13: return 52;
	case TRXHIP_COMB_LOOPBACK: return 51;
	default: return 1;
	}
}

/* How many of the k consecutive frames from burst-time FN `fn` give timeslot tn of `chan` the type IDLE.  The type repeats every
 * M = trx_rxs_type_period() frames, and the hyperframe is a multiple of M, so FN % M runs on through the wrap: whole periods
 * are counted once, the rest frame by frame (at most 2 * 102 evaluations). */
TRX_RXS_HD inline uint32_t trx_rxs_idle_frames(const trx_rxs_settings &st, int chan, int tn, uint32_t fn, uint64_t k)
{
	const unsigned M = trx_rxs_type_period(st.chan_type[chan][tn]);
	const uint64_t full = k / M;
	const unsigned rest = (unsigned)(k % M);
	uint32_t per = 0, part = 0;
	if (full)
		for (unsigned r = 0; r < M; r++)
			per += trx_rxs_expected_type(st, chan, r, tn) == TRXHIP_IDLE;
	for (unsigned i = 0; i < rest; i++)
		part += trx_rxs_expected_type(st, chan, (fn % M + i) % M, tn) == TRXHIP_IDLE;
	return (uint32_t)(full * per) + part;
}

/* Of the first k slots of a pull from the receive clock (fn0, tn0), those of timeslot tn that insert into channel chan's noise
 * ring: type IDLE on a channel that is not muted (Transceiver.cpp:719-721, :744-748).  Summed over tn = 0 .. 7 it is the ring
 * position, counted from the pull's first insertion, of the next inserting slot. */
TRX_RXS_HD inline uint32_t trx_rxs_inserts_before(const trx_rxs_settings &st, int chan, uint32_t fn0, int tn0, uint64_t k, int tn)
{
	if ((st.muted >> chan) & 1u)
		return 0;
	const unsigned d = (unsigned)(tn - tn0) & 7u;              /* the first slot with this TN */
	if (d >= k)
		return 0;
	const uint64_t frames = (k - d + 7) >> 3;
	const uint32_t first = trx_rxs_fn_add((uint32_t)(((uint64_t)fn0 + (((unsigned)tn0 + d) >> 3)) % TRX_RXS_HYPERFRAME), st.ul_fn_offset);
	return trx_rxs_idle_frames(st, chan, tn, first, frames);
}

/* radioInterface.cpp:272-291: `while (recvSz > burstSize)` over carried + n_samples samples -- strict, so 625 samples stay */
TRX_RXS_HD inline uint64_t trx_rxs_slots(uint64_t carried, uint64_t n_samples)
{
	const uint64_t total = carried + n_samples;
	return total ? (total - 1) / TRX_RXS_SLOT : 0;
}

/* ---- 1 SPS: burstSize = 156 + (tN % 4 == 0), recomputed after every incTN() (radioInterface.cpp:257-258, :283-288) ----
 * tn0: the TN of slot 0 (the receive clock when the pull starts).  j0 = (4 - tn0) & 3 is the first slot of 157 samples; four
 * consecutive slots are always 625 samples, eight 1250. */

/* samples of slot k */
TRX_RXS_HD inline uint32_t trx_rxs_slot_len(int tn0, uint64_t k)
{
	return 156u + (uint32_t)((((uint64_t)tn0 + k) & 3u) == 0u);
}

/* where slot k starts, in samples behind the start of slot 0: 156 k + the slots of 157 among 0 .. k - 1 */
TRX_RXS_HD inline uint64_t trx_rxs_slot_start(int tn0, uint64_t k)
{
	const uint64_t j0 = (uint64_t)((4 - tn0) & 3);
	return 156u * k + ((k + 3u - j0) >> 2);
}

/* `while (recvSz > burstSize)` over carried + n_samples samples with the clock at tn0: slot k is cut when more than its own
 * length is left behind its start, i.e. when slot k + 1 starts before the stream's last sample -- the count is the largest m
 * with trx_rxs_slot_start(m) <= total - 1.  The starts repeat every 4 slots, 625 samples on: whole groups by division, the rest
 * by at most three compares.  Strict against the size of the slot that would be cut next: 156 samples stay in front of a slot
 * of 156, 157 in front of one of 157. */
TRX_RXS_HD inline uint64_t trx_rxs_slots1(int tn0, uint64_t carried, uint64_t n_samples)
{
	const uint64_t total = carried + n_samples;
	if (!total)
		return 0;
	const uint64_t q = (total - 1) / TRX_RXS_SLOT, r = (total - 1) % TRX_RXS_SLOT;
	uint64_t m = 0;
	for (uint64_t i = 1; i < 4; i++)
		m += trx_rxs_slot_start(tn0, i) <= r;
	return 4 * q + m;
}
