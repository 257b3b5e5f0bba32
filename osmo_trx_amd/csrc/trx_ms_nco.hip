// trx_ms_nco.hip -- the MS-side numerically controlled oscillator for gfx950, as a call of its own: rows of int16 or complex64
// samples in, each rotated by its own {phase0, inc}, complex64 rows out, no scale.  trx_ms_nco.h states the arithmetic; this is
// its device-side statement, the thing the rotating instances of ms_rx_kernel (trx_ms_rx.hip) are byte-compared with, and what
// the scheduler's acquire path runs in front of the SCH search when a member's oscillator is on.
//
// A WAVE PER 64-SAMPLE RUN: thread t of a block takes sample blockIdx.x * 256 + t of every row the block serves (blockIdx.y, then
// every gridDim.y-th row), so loads and stores of a wave are one coalesced run of 256 / 512 bytes; the row's record is a
// wave-uniform load, the two table reads hit 16 KB that stay in cache.  Nothing is shared between threads.
// The host-only exports (tables, increment, phase) need no GPU and no context.
#include <hip/hip_runtime.h>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_nco.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxRowsY = 65535;

static_assert(sizeof(trxhip_ms_nco_row) == 8 && sizeof(trx_nco_slot) == 16, "records");
static_assert(sizeof(trxhip_ms_nco_cfg) == 16 && sizeof(trxhip_ms_nco_status) == 32, "public NCO structs");

template <bool I16>
__global__ void __launch_bounds__(kThreads)
ms_nco_rows_kernel(const void *__restrict__ in, size_t row_stride, const trxhip_ms_nco_row *__restrict__ rec, float2 *__restrict__ out,
		   size_t out_stride, unsigned n_rows, unsigned row_len, const float *__restrict__ tab)
{
	const unsigned i = blockIdx.x * kThreads + threadIdx.x;        /* row_len < 2^31: no wrap */
	if (i >= row_len)
		return;
	for (unsigned r = blockIdx.y; r < n_rows; r += gridDim.y) {
		const trxhip_ms_nco_row o = rec[r];
		float xr, xi;
		if (I16) {
			const short2 v = static_cast<const short2 *>(in)[(size_t)r * row_stride + i];
			xr = (float)v.x;
			xi = (float)v.y;
		} else {
			const float2 v = static_cast<const float2 *>(in)[(size_t)r * row_stride + i];
			xr = v.x;
			xi = v.y;
		}
		float rc, rs, yr, yi;
		trx_nco_phasor(tab, o.phase0 + i * (uint32_t)o.inc, &rc, &rs);
		trx_nco_rotate(xr, xi, rc, rs, &yr, &yi);
		out[(size_t)r * out_stride + i] = make_float2(yr, yi);
	}
}

int nco_batch(trxhip_ctx *ctx, const void *d_in, int i16, size_t row_stride, const void *d_rec, float *d_out, size_t out_stride, size_t n_rows,
	      size_t row_len, void *stream)
{
	if (!ctx || !ctx->d_nco_tab || !d_in || (reinterpret_cast<uintptr_t>(d_in) & (i16 ? 3 : 7)) || !d_rec ||
	    (reinterpret_cast<uintptr_t>(d_rec) & 3) || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 7) || n_rows == 0 ||
	    n_rows > 0x7fffffffull || row_len == 0 || row_len > 0x7fffffffull || row_stride < row_len || out_stride < row_len)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_ms_nco_rows(d_in, i16, row_stride, static_cast<const trxhip_ms_nco_row *>(d_rec), d_out, out_stride, n_rows, row_len,
				      ctx->d_nco_tab, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" int trx_launch_ms_nco_rows(const void *d_in, int i16, size_t row_stride, const trxhip_ms_nco_row *d_rec, float *d_out, size_t out_stride,
				      size_t n_rows, size_t row_len, const float *d_tab, hipStream_t stream)
{
	if (n_rows == 0 || row_len == 0)
		return 0;
	if (n_rows > 0x7fffffffull || row_len > 0x7fffffffull)
		return TRXHIP_EINVAL;
	const dim3 grid((unsigned)((row_len + kThreads - 1) / kThreads), (unsigned)(n_rows < kMaxRowsY ? n_rows : kMaxRowsY));
	if (i16)
		hipLaunchKernelGGL(ms_nco_rows_kernel<true>, grid, dim3(kThreads), 0, stream, d_in, row_stride, d_rec,
				   reinterpret_cast<float2 *>(d_out), out_stride, (unsigned)n_rows, (unsigned)row_len, d_tab);
	else
		hipLaunchKernelGGL(ms_nco_rows_kernel<false>, grid, dim3(kThreads), 0, stream, d_in, row_stride, d_rec,
				   reinterpret_cast<float2 *>(d_out), out_stride, (unsigned)n_rows, (unsigned)row_len, d_tab);
	return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO;
}

extern "C" {

int trxhip_ms_nco_tables_host(float *out4096)
{
	if (!out4096)
		return TRXHIP_EINVAL;
	trx_nco_tables(out4096);
	return TRXHIP_OK;
}

int trxhip_ms_nco_inc(double hz, int32_t *inc)
{
	if (!inc)
		return TRXHIP_EINVAL;
	return trx_nco_inc(hz, inc) == 0 ? TRXHIP_OK : TRXHIP_EINVAL;
}

uint32_t trxhip_ms_nco_phase(uint32_t acc, int64_t ts_ref, int32_t inc, int64_t ts) { return trx_nco_phase(acc, ts_ref, inc, ts); }

int trxhip_ms_nco_batch_i16(trxhip_ctx *ctx, const int16_t *d_in, size_t row_stride, const trxhip_ms_nco_row *d_rec, float *d_out_cf32,
			    size_t out_stride, size_t n_rows, size_t row_len, void *stream)
{
	return nco_batch(ctx, d_in, 1, row_stride, d_rec, d_out_cf32, out_stride, n_rows, row_len, stream);
}

int trxhip_ms_nco_batch_cf32(trxhip_ctx *ctx, const float *d_in_cf32, size_t row_stride, const trxhip_ms_nco_row *d_rec, float *d_out_cf32,
			     size_t out_stride, size_t n_rows, size_t row_len, void *stream)
{
	return nco_batch(ctx, d_in_cf32, 0, row_stride, d_rec, d_out_cf32, out_stride, n_rows, row_len, stream);
}

}  // extern "C"
