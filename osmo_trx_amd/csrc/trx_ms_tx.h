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
