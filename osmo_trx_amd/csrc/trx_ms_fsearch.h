// trx_ms_fsearch.h -- the geometry of the MS-side FCCH search (include/trxhip.h, "MS-side FCCH search"), written once
// for the host that sizes the work array and the kernels of trx_ms_fsearch.hip that fill it.
//   a row of buf_len samples has nb = (buf_len - LAG) / HOP whole blocks of HOP samples and nb - 35 grid windows of 36 blocks;
//   window j (pos = HOP * j) is blocks j .. j + 35, its halves blocks j .. j + 17 and j + 18 .. j + 35;
//   segment s of a row holds the windows s * SEG .. s * SEG + SEG - 1 and needs the block sums of SEG + 35 blocks.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/trxhip.h"

#if defined(__HIPCC__)
#define TRX_FS_HD __host__ __device__
#else
#define TRX_FS_HD
#endif

#define TRX_FS_HOP     TRXHIP_MS_FSEARCH_HOP       /* 16 */
#define TRX_FS_W       TRXHIP_MS_FSEARCH_W         /* 576 */
#define TRX_FS_LAG     TRXHIP_MS_FSEARCH_LAG       /* 8 */
#define TRX_FS_BLOCKS  (TRX_FS_W / TRX_FS_HOP)     /* 36 blocks per window */
#define TRX_FS_HALF    (TRX_FS_BLOCKS / 2)         /* 18 blocks per half */
#define TRX_FS_SEG     256                         /* windows (and first blocks) per segment: 4096 samples */
#define TRX_FS_MIN_LEN (TRX_FS_W + TRX_FS_LAG)     /* 584: one window */

TRX_FS_HD inline uint32_t trx_fs_blocks(uint32_t buf_len) { return (buf_len - TRX_FS_LAG) / TRX_FS_HOP; }
TRX_FS_HD inline uint32_t trx_fs_windows(uint32_t buf_len) { return trx_fs_blocks(buf_len) - (TRX_FS_BLOCKS - 1); }
TRX_FS_HD inline uint32_t trx_fs_segments(uint32_t buf_len) { return (trx_fs_windows(buf_len) + TRX_FS_SEG - 1) / TRX_FS_SEG; }
