// trx_tx_tables.h -- layout of the transmit-side table struct: what the reference's modulators read
// (Transceiver52M/sigProcLib.cpp:66-75, :191-216, :405-543, :672-763) and the burst bit patterns its generators
// copy (:768-915).  Built on the host at context creation (trx_tx.hip, trx_tx_tables_generate) and uploaded next
// to the receive blob of trx_tables.h, which it does not touch.  The attenuation scales of the TRXD entry point
// depend on the caller's full_scale: they live in the context (trx_ctx.h), not here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "trx_tables.h"

#define TRX_TX_TABLES_MAGIC   0x54585454u      /* 'TTXT' */
#define TRX_TX_TABLES_VERSION 1
#define TRX_TX_EDGE_SYMS      156              /* 8-PSK symbols a 625-sample burst holds: 468 bits */

struct trx_tx_tables {
	uint32_t magic;
	uint32_t version;
	float    pulse4_c0[16];                     // generateGSMPulse(4) c0, sigProcLib.cpp:501-517
	float    pulse4_c1[8];                      // generateC1Pulse, :447-458
	float    pulse1_c0[4];                      // generateGSMPulse(1) c0, :519-533 (normalised, :535-543)
	float    pad0[4];
	trx_c32  rot4[625];                         // GMSKRotation4, :195-204
	trx_c32  pad1[3];
	trx_c32  rot1[157];                         // GMSKRotation1, :206-215
	trx_c32  pad2[3];
	trx_c32  psk8[8];                           // psk8_table, :66-75
	trx_c32  edge_rot[TRX_TX_EDGE_SYMS];        // (cos(phase), sin(phase)), float phase = i * 3.0f * M_PI / 8.0f, :683-685 / :752-754
	// 3GPP TS 45.002 bit patterns, one bit (0 / 1) per byte
	uint8_t  dummy_burst[148];                  // gDummyBurst, section 5.2.6
	uint8_t  rach_burst[49];                    // gRACHBurst head (8) + synchronisation sequence TS0 (41), section 5.2.7
	uint8_t  pad3[3];
	uint8_t  tsc[8][26];                        // gTrainingSequence, section 5.2.3
	uint8_t  edge_tsc[8][78];                   // gEdgeTrainingSequence (8-PSK symbols as bit triples), section 5.2.3
};
