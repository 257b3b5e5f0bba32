// trx_ms_tx.h -- what the MS-side uplink burst scheduler (trx_ms_tx.cpp, the host planner) hands its render kernel
// (trx_tx.hip, ms_tx_render_kernel): the staged bursts and the segments of a window.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define TRX_MSTX_BURST 625u                /* samples of a burst: modulateBurst(bits, guard, 4), guard ignored at 4 SPS */
#define TRX_MSTX_ZERO  0xffffffffu         /* trx_mstx_seg.src of a segment of zeros */

/* A queued burst on the device: its bits and the scale driveTx() gives scaleVector() -- not samples (the modulator is
 * deterministic: modulating again gives the same int16, the argument the downlink filler table rests on). */
struct trx_mstx_row {
	uint8_t  bits[148];                    /* one bit per byte */
	uint8_t  pad[4];
	float    scale;                        /* (float)(txFullScale * pow(10, -RSSI / 10)); the imaginary part is 0 */
	uint32_t reserved;
};
static_assert(sizeof(trx_mstx_row) == 160, "trx_mstx_row layout");

/* One wave's work: samples [out_off, out_off + len) of the window, len <= 625, taken from samples [first, first + len) of
 * the burst staged in row src, or zeros.  The segments of a render tile its window: every sample lies in exactly one. */
struct trx_mstx_seg {
	uint32_t out_off;
	uint32_t src;                          /* ring row, or TRX_MSTX_ZERO */
	uint16_t len, first;                   /* first + len <= 625 */
	uint32_t reserved;
};
static_assert(sizeof(trx_mstx_seg) == 16, "trx_mstx_seg layout");

/* The group's render (trxhip_ms_tx_group_*, ms_tx_render_group_kernel): one table per call -- an entry per rendered member, in the
 * order of their waves, and right behind the entries the queued bursts that have samples in those members' windows.  The window
 * is cut into tiles of 625 samples (the last one shorter); wave w draws tile w - first_wave of the entry with the largest
 * first_wave <= w.  first_wave rises strictly from 0; an entry has n_samples >= 1.  32 bytes */
struct trx_mstx_gmember {
	uint64_t out_off;                      /* the window's first sample, in samples from d_out */
	uint32_t n_samples;
	uint32_t first_wave;
	uint32_t first_burst, n_bursts;        /* its bursts in the list behind the entries: ascending rel, 625 or more apart */
	uint32_t nco_phase0;                   /* the uplink oscillator (trx_ms_nco.h): the phase of the window's first sample and the */
	int32_t  nco_inc;                      /* increment; 0 and 0 for a member with it off.  Read by the rotating instance only */
};
static_assert(sizeof(trx_mstx_gmember) == 32, "trx_mstx_gmember layout");

struct trx_mstx_gburst {
	int32_t  rel;                          /* radio_ts - first_ts: -624 .. n_samples - 1 */
	uint32_t row;                          /* member * max_pending + ring row */
};
static_assert(sizeof(trx_mstx_gburst) == 8, "trx_mstx_gburst layout");
