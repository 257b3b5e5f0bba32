// trx_tx_sched.h -- what the downlink burst scheduler (trx_tx_sched.cpp, the host planner) hands the render kernel
// (trx_tx.hip, tx_render_kernel): the staged datagram rows, the filler-table descriptors and the per-slot source words.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define TRX_TXS_ROW_STRIDE 464u            /* one staged TRXD datagram: 6 + 444 bytes, rounded up to 16 */
#define TRX_TXS_FILL_BITS  448u            /* bits of a filler descriptor (444 used by an 8-PSK burst) */
#define TRX_TXS_ENTRIES    (102u * 8u)     /* filler table entries per channel: [FN % 102][TN] */

/* slot word: kind << 30 | index.  ROW: a staged datagram row (TRX_TXS_ROW_STRIDE bytes at rows + index * stride, the
 * datagram's length as a little-endian uint16 in the row's last two bytes); ENTRY: the filler descriptor fill[index] (index = chan * TRX_TXS_ENTRIES + modFN * 8 + TN); ZERO: zeros */
#define TRX_TXS_ZERO  0u
#define TRX_TXS_ROW   1u
#define TRX_TXS_ENTRY 2u
#define TRX_TXS_WORD(kind, index) (((uint32_t)(kind) << 30) | (uint32_t)(index))

/* A filler-table entry on the device: a burst as its bits and the parameters of its modulation, not as samples
 * (the modulator is deterministic: modulating again gives the floats the reference stored). */
struct trx_tx_fill {
	uint16_t nbits;                        /* 148 (GMSK) or 444 (8-PSK) */
	uint8_t  guard;                        /* 8 + (tn % 4 == 0) */
	uint8_t  flags;                        /* TRXHIP_TX_8PSK or 0 */
	float    scale_re, scale_im;           /* the complex scale scaleVector() applied */
	uint32_t reserved;
	uint8_t  bits[TRX_TXS_FILL_BITS];      /* one bit per byte */
};
static_assert(sizeof(trx_tx_fill) == 464, "trx_tx_fill layout");

/* end of a render: entry <- the burst staged in row (its bits; nbits, guard, flags, scale from the planner) */
struct trx_tx_fill_update {
	uint32_t entry, row;
	uint16_t nbits;
	uint8_t  guard, flags;
	float    scale_re;                     /* the attenuation scale; the imaginary part is 0 (Transceiver.cpp:396) */
};
static_assert(sizeof(trx_tx_fill_update) == 16, "trx_tx_fill_update layout");

#define TRX_TXS_MAX_CHANS 8
struct trx_tx_s16_scales { float s[TRX_TXS_MAX_CHANS]; };
