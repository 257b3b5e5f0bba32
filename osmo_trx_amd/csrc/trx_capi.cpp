// trx_capi.cpp -- the extern "C" seam declared in include/trxhip.h.
// Thin: argument checks, table upload, kernel launches.  No CPU fallback anywhere: when no HIP
// device is usable trxhip_create() fails with TRXHIP_ENODEV and nothing else can be called.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/trxhip.h"
#include "trx_tables.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_nco.h"

extern "C" {

int trxhip_abi_version(void) { return TRXHIP_ABI_VERSION; }

int trxhip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

const char *trxhip_strerror(int err)
{
	switch (err) {
	case TRXHIP_OK: return "ok";
	case TRXHIP_EINVAL: return "invalid argument";
	case TRXHIP_ENOMEM: return "out of device memory";
	case TRXHIP_ENODEV: return "no usable HIP device (gfx950 required; there is no CPU fallback)";
	case TRXHIP_EIO: return "HIP runtime / kernel launch error";
	case TRXHIP_ENOTSUP: return "not supported";
	default: return "unknown error";
	}
}

size_t trxhip_tables_size(void) { return sizeof(trx_tables); }

int trxhip_tables_generate_host(void *h_blob, size_t size)
{
	if (!h_blob || size != sizeof(trx_tables))
		return TRXHIP_EINVAL;
	return trx_tables_generate(static_cast<trx_tables *>(h_blob)) == 0 ? TRXHIP_OK : TRXHIP_EINVAL;
}

uint64_t trxhip_tables_checksum(const void *h_blob, size_t size)
{
	const unsigned char *p = static_cast<const unsigned char *>(h_blob);
	uint64_t h = 1469598103934665603ull;          /* FNV-1a 64 */
	for (size_t i = 0; i < size; i++) {
		h ^= p[i];
		h *= 1099511628211ull;
	}
	return h;
}

int trxhip_create_from_tables(trxhip_ctx **out, int device, const void *h_blob, size_t size)
{
	if (!out || !h_blob || size != sizeof(trx_tables))
		return TRXHIP_EINVAL;
	const trx_tables *t = static_cast<const trx_tables *>(h_blob);
	if (t->magic != TRX_TABLES_MAGIC || t->version != TRX_TABLES_VERSION)
		return TRXHIP_EINVAL;
	/* the composite-tap window is a build-time choice of generator AND kernels (TRX_FUSED_U0 / TRX_FUSED_NT): a blob made by a
	 * build with another window would be read with shifted taps */
	if (t->fused_u0 != TRX_FUSED_U0 || t->fused_nt != TRX_FUSED_NT)
		return TRXHIP_EINVAL;
	/* the exact delay filters of the kernels skip taps 0, 17, 18, 19: exactly 0.0f in every filter sigProcLibSetup() can
	 * generate (the sinc LUT is zero beyond 8 pi, sigProcLib.cpp:990-998, :2164-2172).  A blob that breaks this is not such a
	 * table set: refused rather than silently evaluated with 16 of its 20 taps.  (Non-finite samples: the
	 * reference's x * 0 turns an Inf / NaN inside the 20-tap span into NaN where the skipped taps drop it -- complex64 input
	 * only; int16 input is always finite.) */
	for (int f = 0; f < TRX_DELAY_FILTS; f++)
		if (t->delay_filt[f][0] != 0.0f || t->delay_filt[f][17] != 0.0f || t->delay_filt[f][18] != 0.0f || t->delay_filt[f][19] != 0.0f)
			return TRXHIP_ENOTSUP;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
		return TRXHIP_ENODEV;
	if (hipSetDevice(device) != hipSuccess)
		return TRXHIP_ENODEV;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess)
		return TRXHIP_ENODEV;

	trxhip_ctx *ctx = new (std::nothrow) trxhip_ctx;
	if (!ctx)
		return TRXHIP_ENOMEM;
	ctx->device = device;
	ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	ctx->no_unit = trx_unit_masks_match(t) ? 0 : 1;
	ctx->sch_unit = trx_unit_mask_sch_match(t) ? 1 : 0;
	ctx->pool_enabled = getenv("TRXHIP_NO_POOL") ? 0 : 1;          /* measurement switch, read once per context */
	ctx->nb_enabled = getenv("TRXHIP_NO_NB_KERNEL") ? 0 : 1;       /* the same for the normal-burst kernel (A/B against the general one) */
	for (int k = 0; k < 8; k++)                                    /* the straight-line decimator reads taps 0..7 and mirrors them */
		if (memcmp(&t->dec_taps[k], &t->dec_taps[15 - k], sizeof(float)) != 0)
			ctx->no_sym = 1;
	/* the FAST detector's margin assumes sum_u |w_u| <= 2.6 for the 16 sinc weights of every fractional position
	 * (trx_device.h, TRX_FAST_W): taps i <= fl use q = 512 k + f, taps i > fl use q = 512 k + (512 - f), k = 0 .. 7 */
	for (int f = 0; f < 512 && !ctx->no_fast; f++) {
		double sum = 0.0;
		for (int k = 0; k < 8; k++) {
			const int qa = 512 * k + f, qb = 512 * k + (512 - f);
			sum += fabs((double)t->sincv[trx_sincv_swz(qa)]);
			if (qb < TRX_SINCV_LEN)
				sum += fabs((double)t->sincv[trx_sincv_swz(qb)]);
		}
		if (!(sum <= 2.6))
			ctx->no_fast = 1;
	}
	int rc = ctx->d_tables.alloc(1);
	if (rc == TRXHIP_OK && hipMemcpy(ctx->d_tables, h_blob, sizeof(trx_tables), hipMemcpyHostToDevice) != hipSuccess)
		rc = TRXHIP_EIO;
	if (rc == TRXHIP_OK)
		rc = ctx->redo.create();
	if (rc == TRXHIP_OK) {
		/* the transmit tables (trx_tx_tables.h), next to the receive blob */
		trx_tx_tables *tx = static_cast<trx_tx_tables *>(malloc(sizeof(trx_tx_tables)));
		if (!tx || trx_tx_tables_generate(tx) != 0)
			rc = TRXHIP_ENOMEM;
		else if ((rc = ctx->d_tx_tables.alloc(1)) == TRXHIP_OK &&
			 hipMemcpy(ctx->d_tx_tables, tx, sizeof(trx_tx_tables), hipMemcpyHostToDevice) != hipSuccess)
			rc = TRXHIP_EIO;
		free(tx);
	}
	if (rc == TRXHIP_OK) {
		/* the NCO's phasor tables (trx_ms_nco.h) */
		float *nco = static_cast<float *>(malloc(TRX_NCO_FLOATS * sizeof(float)));
		if (!nco) {
			rc = TRXHIP_ENOMEM;
		} else {
			trx_nco_tables(nco);
			if ((rc = ctx->d_nco_tab.alloc(TRX_NCO_FLOATS)) == TRXHIP_OK &&
			    hipMemcpy(ctx->d_nco_tab, nco, TRX_NCO_FLOATS * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
				rc = TRXHIP_EIO;
			free(nco);
		}
	}
	if (rc != TRXHIP_OK) {
		trxhip_destroy(ctx);
		return rc;
	}
	if (ctx->d_pool.alloc(TRX_POOL_SLOTS * 16) != TRXHIP_OK || hipMemset(ctx->d_pool, 0, TRX_POOL_SLOTS * 64) != hipSuccess)
		(void)ctx->d_pool.reset();                             /* (the kernels run without the pool) */
	*out = ctx;
	return TRXHIP_OK;
}

int trxhip_create(trxhip_ctx **out, int device)
{
	if (!out)
		return TRXHIP_EINVAL;
	trx_tables *t = static_cast<trx_tables *>(malloc(sizeof(trx_tables)));
	if (!t)
		return TRXHIP_ENOMEM;
	int rc = trx_tables_generate(t) == 0 ? TRXHIP_OK : TRXHIP_EINVAL;
	if (rc == TRXHIP_OK)
		rc = trxhip_create_from_tables(out, device, t, sizeof(trx_tables));
	free(t);
	return rc;
}

void trxhip_destroy(trxhip_ctx *ctx)
{
	if (!ctx)
		return;
	(void)with_device(ctx);
	delete ctx;
}

int trxhip_set_nb_kernel(trxhip_ctx *ctx, int enabled)
{
	if (!ctx)
		return TRXHIP_EINVAL;
	ctx->nb_enabled = enabled ? 1 : 0;
	return TRXHIP_OK;
}

int trxhip_set_work_pool(trxhip_ctx *ctx, int enabled)
{
	if (!ctx)
		return TRXHIP_EINVAL;
	ctx->pool_enabled = enabled ? 1 : 0;
	return TRXHIP_OK;
}

int trxhip_fast_stats(trxhip_ctx *ctx, uint64_t *out4, int reset)
{
	if (!ctx || !out4)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	unsigned long long v[4] = { 0, 0, 0, 0 };
	if (trx_fast_stats_read(v, reset) != 0)
		return TRXHIP_EIO;
	for (int k = 0; k < 4; k++)
		out4[k] = v[k];
	return TRXHIP_OK;
}

size_t trxhip_tx_tables_size(void) { return sizeof(trx_tx_tables); }

int trxhip_tx_tables_generate_host(void *h_buf, size_t size)
{
	if (!h_buf || size != sizeof(trx_tx_tables))
		return TRXHIP_EINVAL;
	return trx_tx_tables_generate(static_cast<trx_tx_tables *>(h_buf)) == 0 ? TRXHIP_OK : TRXHIP_EINVAL;
}

/* the row and stride limits both modulator entry points share: rows of at most 2^20 samples, 8-byte aligned cf32 rows and
 * 4-byte aligned int16 rows (the kernel realigns each row to its 16- / 8-byte stores itself) */
static int tx_check_outputs(const float *d_out_cf32, const int16_t *d_out_s16, size_t out_stride, int sps)
{
	if ((sps != 1 && sps != 4) || out_stride == 0 || out_stride > (1u << 20))
		return TRXHIP_EINVAL;
	if ((reinterpret_cast<uintptr_t>(d_out_cf32) & 7) || (reinterpret_cast<uintptr_t>(d_out_s16) & 3))
		return TRXHIP_EINVAL;
	return TRXHIP_OK;
}

int trxhip_modulate_batch(trxhip_ctx *ctx, const uint8_t *d_bits, size_t bits_stride, const trxhip_tx_params *d_params,
			  float *d_out_cf32, int16_t *d_out_s16, float s16_scale, size_t out_stride, int32_t *d_out_len,
			  size_t n, int sps, void *stream)
{
	if (!ctx || !ctx->d_tx_tables || (n && (!d_bits || !d_params)) || bits_stride == 0 ||
	    tx_check_outputs(d_out_cf32, d_out_s16, out_stride, sps) != TRXHIP_OK)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_tx_modulate(d_bits, bits_stride, d_params, nullptr, nullptr, ctx->d_tx_tables, d_out_cf32, d_out_s16,
				      s16_scale, out_stride, d_out_len, nullptr, n, sps, static_cast<hipStream_t>(stream));
}

int trxhip_modulate_trxd_batch(trxhip_ctx *ctx, const uint8_t *d_dgram, size_t dgram_stride, const uint16_t *d_dgram_len,
			       double full_scale, int sps, float *d_out_cf32, int16_t *d_out_s16, float s16_scale,
			       size_t out_stride, trxhip_tx_info *d_info, size_t n, void *stream)
{
	if (!ctx || !ctx->d_tx_tables || (n && (!d_dgram || !d_dgram_len)) || dgram_stride < 6 ||
	    tx_check_outputs(d_out_cf32, d_out_s16, out_stride, sps) != TRXHIP_OK)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	float att[256];
	{
		/* addRadioVector(), Transceiver.cpp:396: txFullScale * pow(10, (double) -RSSI / 20), narrowed to float by scaleVector()'s
		 * complex argument.  Computed on the host in double once per full_scale; the kernel receives the 256 values by value */
		std::lock_guard<std::mutex> lk(ctx->tx_mu);
		if (!ctx->tx_att_valid || memcmp(&ctx->tx_full_scale, &full_scale, sizeof(double)) != 0) {
			for (int a = 0; a < 256; a++)
				ctx->tx_att_scale[a] = (float)(full_scale * pow(10, (double)-a / 20));
			ctx->tx_full_scale = full_scale;
			ctx->tx_att_valid = true;
		}
		memcpy(att, ctx->tx_att_scale, sizeof(att));
	}
	return trx_launch_tx_modulate(d_dgram, dgram_stride, nullptr, d_dgram_len, att, ctx->d_tx_tables, d_out_cf32, d_out_s16,
				      s16_scale, out_stride, nullptr, d_info, n, sps, static_cast<hipStream_t>(stream));
}

int trxhip_tables_device_ptr(trxhip_ctx *ctx, void **d_blob)
{
	if (!ctx || !d_blob)
		return TRXHIP_EINVAL;
	*d_blob = ctx->d_tables;
	return TRXHIP_OK;
}

static int pull_common(trxhip_ctx *ctx, const void *d_iq, int cf32, const trxhip_burst_params *d_params,
		       const float *d_ebp_in, trxhip_burst_result *d_results, float *d_soft, size_t n_bursts, int burst_len, int sps,
		       float threshold, float full_scale, int soft_stride, int flags, void *stream)
{
	if (!ctx)
		return TRXHIP_EINVAL;
	if (sps != 1 && sps != 4)
		return TRXHIP_EINVAL;                                  /* sigProcLib.cpp:1740-1741 */
	if (burst_len > TRXHIP_MAX_BURST_LEN || (sps == 4 && burst_len < 624) ||
	    (sps == 1 && (burst_len < 148 || burst_len > 192)))
		return TRXHIP_EINVAL;
	if (d_soft && soft_stride < 1)
		return TRXHIP_EINVAL;
	if (n_bursts == 0)
		return TRXHIP_OK;                                      /* empty batch: nothing to do */
	if (!d_iq || !d_params || !d_results || n_bursts > 0x7fffffffull)   /* 32-bit burst index + grid stride in the kernels */
		return TRXHIP_EINVAL;
	if ((reinterpret_cast<uintptr_t>(d_iq) & 3) != 0)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	if (flags & ~(TRXHIP_FLAG_SLICE | TRXHIP_FLAG_EXACT_DEMOD | TRXHIP_FLAG_IDLE_DUMMY | TRXHIP_FLAG_FEW_NB_SLOTS))
		return TRXHIP_EINVAL;
	const bool few_nb = (flags & TRXHIP_FLAG_FEW_NB_SLOTS) != 0;  /* a hint, not a kernel flag */
	flags &= ~TRXHIP_FLAG_FEW_NB_SLOTS;
	if (ctx->no_unit)
		flags |= TRX_IFLAG_NO_UNIT;
	if (ctx->no_sym)
		flags |= TRX_IFLAG_NO_SYM;
	if (ctx->no_fast)
		flags |= TRX_IFLAG_NO_FAST;
	const hipStream_t st = static_cast<hipStream_t>(stream);

	/* ---- the kernel choice ---- */
	/* A launch that is being captured into a HIP graph keeps whatever it is handed for as long as the graph lives, and replays
	 * may overlap later launches: it gets neither a pool counter pair (static split) nor a leftover list (general kernel only) --
	 * both are recycled between launches. */
	hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
	const bool capturing = st && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
	const bool exact = (flags & TRXHIP_FLAG_EXACT_DEMOD) != 0;
	/* the transceiver's 4-SPS burst size gets the production kernel (polyphase LDS layout, fused or exact demodulator) */
	const bool k4 = sps == 4 && burst_len >= 624 && burst_len <= 628;
	/* the launch pullRadioVector() makes: 625 samples, sliced rows of 148 soft bits, no flag but SLICE (and EXACT_DEMOD), none
	 * of the internal TRX_IFLAG_* bits -- the 4-SPS kernel's COMMON instance folds these parameters, except with cf32 and exact
	 * together */
	const bool common = k4 && burst_len == 625 && d_soft && !d_ebp_in && soft_stride == 148 &&
			    (flags & ~TRXHIP_FLAG_EXACT_DEMOD) == TRXHIP_FLAG_SLICE && !(cf32 && exact);
	/* ... and with int16 input and the fused demodulator it is the split: the normal-burst kernel over the batch, then the
	 * general kernel over whatever it left on its list */
	const bool split = common && !cf32 && !exact && ctx->nb_enabled && !few_nb && !capturing;
	/* a counter pair of the 4-SPS kernels' cross-die pool for this launch (zero: the previous user's last workgroup re-armed it;
	 * trx_ctx.h).  The pool needs the persistent grid (one workgroup per CU) and >= 8 groups of 16 bursts per workgroup. */
	unsigned *pool = nullptr;
	if (k4 && ctx->d_pool && ctx->pool_enabled && !capturing && n_bursts >= (size_t)ctx->n_cu * 128)
		pool = ctx->d_pool + (size_t)(ctx->pool_next.fetch_add(1u, std::memory_order_relaxed) % TRX_POOL_SLOTS) * 16;

	if (!k4) {
		/* NLD: dword loads per lane held in registers for the prefetched burst (0: generic length, no prefetch) */
		const int nld = sps == 1 ? 3 : burst_len <= 640 ? 10 : 0;
		return trx_launch_pull(d_iq, cf32, nld, d_params, d_results, d_soft, ctx->d_tables, d_ebp_in, n_bursts, burst_len, sps,
				       threshold, full_scale, soft_stride, flags, ctx->n_cu, st);
	}
	if (split) {
		std::lock_guard<std::mutex> lk(ctx->redo.mu);
		if (trx_redo_lists::slot *sl = ctx->redo.acquire(n_bursts, st)) {
			const int rc = trx_launch_pull4_nb(pool, d_iq, d_params, d_results, d_soft, ctx->d_tables, n_bursts, threshold,
							   full_scale, ctx->n_cu, sl->d, sl->h_left, st);
			ctx->redo.launched(*sl, rc, st);
			return rc;
		}
		/* (back-off, or no list buffer: the general kernel alone) */
	}
	return trx_launch_pull4(pool, d_iq, cf32, exact, common, d_params, d_results, d_soft, ctx->d_tables, d_ebp_in, n_bursts,
				burst_len, threshold, full_scale, soft_stride, flags, ctx->n_cu, st);
}

int trxhip_select_diversity_batch(trxhip_ctx *ctx, const int16_t *d_iq_paths, size_t n_bursts, int n_paths, int burst_len, int sps,
				  int16_t *d_iq_sel, float *d_avg_energy, uint8_t *d_path, void *stream)
{
	if (!ctx || n_paths < 1 || n_paths > 8 || (sps != 1 && sps != 4) || burst_len < 1 || burst_len > TRXHIP_MAX_BURST_LEN)
		return TRXHIP_EINVAL;
	/* energyDetect(path, 20 * sps) reads samples 0, 4, 8, ... of the path (sigProcLib.cpp:1576-1584, window clamped to the
	 * vector's size): the last one, 4 * (window - 1), must lie inside the path -- 317 samples at 4 SPS, 77 at 1 SPS */
	{
		const int window = 20 * sps < burst_len ? 20 * sps : burst_len;
		if (4 * (window - 1) >= burst_len)
			return TRXHIP_EINVAL;
	}
	if (n_bursts == 0)
		return TRXHIP_OK;
	if (!d_iq_paths || !d_iq_sel || !d_avg_energy || (reinterpret_cast<uintptr_t>(d_iq_paths) & 3) ||
	    (reinterpret_cast<uintptr_t>(d_iq_sel) & 3))
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_diversity_select(d_iq_paths, n_bursts, n_paths, burst_len, sps, d_iq_sel, d_avg_energy, d_path,
					   static_cast<hipStream_t>(stream));
}

int trxhip_apply_diversity_power(trxhip_ctx *ctx, trxhip_burst_result *d_results, const trxhip_burst_params *d_params,
				 const float *d_avg_energy, size_t n_bursts, float full_scale, void *stream)
{
	if (!ctx || !(full_scale > 0.0f))
		return TRXHIP_EINVAL;
	if (n_bursts == 0)
		return TRXHIP_OK;
	if (!d_results || !d_params || !d_avg_energy)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_diversity_power(d_results, d_params, d_avg_energy, n_bursts, full_scale, static_cast<hipStream_t>(stream));
}

int trxhip_detect_demod_batch(trxhip_ctx *ctx, const int16_t *d_iq, const trxhip_burst_params *d_params,
			      trxhip_burst_result *d_results, float *d_soft, size_t n_bursts, int burst_len, int sps,
			      float threshold, float full_scale, int soft_stride, int flags, void *stream)
{
	return pull_common(ctx, d_iq, 0, d_params, nullptr, d_results, d_soft, n_bursts, burst_len, sps, threshold, full_scale,
			   soft_stride, flags, stream);
}

int trxhip_detect_demod_batch_cf32(trxhip_ctx *ctx, const float *d_iq, const trxhip_burst_params *d_params,
				   trxhip_burst_result *d_results, float *d_soft, size_t n_bursts, int burst_len,
				   int sps, float threshold, float full_scale, int soft_stride, int flags, void *stream)
{
	return pull_common(ctx, d_iq, 1, d_params, nullptr, d_results, d_soft, n_bursts, burst_len, sps, threshold, full_scale,
			   soft_stride, flags, stream);
}

int trxhip_demod_batch_cf32(trxhip_ctx *ctx, const float *d_iq, const trxhip_burst_params *d_params,
			    const float *d_ebp, trxhip_burst_result *d_results, float *d_soft, size_t n_bursts,
			    int burst_len, int sps, int soft_stride, int flags, void *stream)
{
	if (n_bursts > 0 && (!d_ebp || (reinterpret_cast<uintptr_t>(d_ebp) & 15) != 0))
		return TRXHIP_EINVAL;
	return pull_common(ctx, d_iq, 1, d_params, d_ebp, d_results, d_soft, n_bursts, burst_len, sps,
			   TRXHIP_BURST_THRESH, 1.0f, soft_stride, flags, stream);
}

int trxhip_pack_trxd_batch(trxhip_ctx *ctx, const trxhip_burst_result *d_results, const float *d_soft_sliced,
			   int soft_stride, uint8_t *d_pkt, size_t n_bursts, float rssi_offset, void *stream)
{
	if (!ctx || !d_results || !d_soft_sliced || !d_pkt || soft_stride < 148)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_pack_trxd(d_results, d_soft_sliced, soft_stride, d_pkt, n_bursts, rssi_offset,
				    static_cast<hipStream_t>(stream));
}

int trxhip_pack_trxd_wire_batch(trxhip_ctx *ctx, const trxhip_burst_result *d_results, const trxhip_burst_params *d_params,
				const float *d_soft_sliced, int soft_stride, const trxhip_trxd_meta *d_meta,
				uint8_t *d_pkt, int pkt_stride, uint16_t *d_pkt_len, size_t n_bursts, float rssi_offset,
				void *stream)
{
	if (!ctx || soft_stride < 148 || pkt_stride < 160 || (pkt_stride & 3))
		return TRXHIP_EINVAL;
	if (n_bursts == 0)
		return TRXHIP_OK;
	if (!d_results || !d_params || !d_soft_sliced || !d_meta || !d_pkt || !d_pkt_len || n_bursts > 0x7fffffffull ||
	    (reinterpret_cast<uintptr_t>(d_pkt) & 3) != 0)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_pack_trxd_wire(d_results, d_params, d_soft_sliced, soft_stride, d_meta, d_pkt, pkt_stride, d_pkt_len,
					 n_bursts, rssi_offset, static_cast<hipStream_t>(stream), nullptr);
}

static int conv_common(trxhip_ctx *ctx, const float *d_x, int x_len, const float *d_h, int h_len, int h_complex,
		       float *d_y, int y_len, int start, int len, size_t n_vec, void *stream)
{
	if (!ctx || !d_x || !d_h || !d_y)
		return TRXHIP_EINVAL;
	/* bounds_check(), arch/common/convolve_base.c:88-105, plus the head-room rule */
	if (x_len < 1 || h_len < 1 || y_len < 1 || len < 1 || h_len > 256)
		return TRXHIP_EINVAL;
	if (start + len > x_len || len > y_len || x_len < h_len || start < h_len - 1)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_convolve(d_x, x_len, d_h, h_len, h_complex, d_y, y_len, start, len, n_vec,
				   static_cast<hipStream_t>(stream));
}

int trxhip_convolve_real_batch(trxhip_ctx *ctx, const float *d_x, int x_len, const float *d_h, int h_len,
			       float *d_y, int y_len, int start, int len, size_t n_vec, void *stream)
{
	return conv_common(ctx, d_x, x_len, d_h, h_len, 0, d_y, y_len, start, len, n_vec, stream);
}

int trxhip_convolve_complex_batch(trxhip_ctx *ctx, const float *d_x, int x_len, const float *d_h, int h_len,
				  float *d_y, int y_len, int start, int len, size_t n_vec, void *stream)
{
	return conv_common(ctx, d_x, x_len, d_h, h_len, 1, d_y, y_len, start, len, n_vec, stream);
}

int trxhip_convert_short_float(trxhip_ctx *ctx, float *d_out, const int16_t *d_in, size_t len, void *stream)
{
	if (!ctx || !d_out || !d_in)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_convert_short_float(d_out, d_in, len, static_cast<hipStream_t>(stream));
}

int trxhip_convert_float_short(trxhip_ctx *ctx, int16_t *d_out, const float *d_in, float scale, size_t len, void *stream)
{
	if (!ctx || (len && (!d_out || !d_in)))
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_convert_float_short(d_out, d_in, scale, len, static_cast<hipStream_t>(stream));
}

int trxhip_dft_batch(trxhip_ctx *ctx, const float *d_in, float *d_out, int m, size_t howmany, size_t istride, size_t ostride,
		     int reverse, void *stream)
{
	if (!ctx || m < 1 || m > 4096 || istride < howmany || ostride < howmany)
		return TRXHIP_EINVAL;
	if (howmany == 0)
		return TRXHIP_OK;
	if (!d_in || !d_out || d_in == d_out)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_dft_strided(d_in, d_out, m, howmany, istride, ostride, reverse, static_cast<hipStream_t>(stream));
}

int trxhip_energy_detect_batch_cf32(trxhip_ctx *ctx, const float *d_iq, size_t n_bursts, int burst_len,
				    unsigned window, float *d_energy, void *stream)
{
	if (!ctx || burst_len < 1)
		return TRXHIP_EINVAL;
	if (n_bursts == 0)
		return TRXHIP_OK;
	if (!d_iq || !d_energy)
		return TRXHIP_EINVAL;
	if (window > 0 && 4 * (size_t)(window > (unsigned)burst_len ? (unsigned)burst_len : window) - 3 > (size_t)burst_len)
		return TRXHIP_EINVAL;                  /* the reference would read past the burst (sigProcLib.cpp:1580-1583) */
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_energy_detect(d_iq, n_bursts, burst_len, window, d_energy, static_cast<hipStream_t>(stream));
}

int trxhip_detect_sch_batch_cf32(trxhip_ctx *ctx, const float *d_iq, trxhip_burst_result *d_results, size_t n_bufs,
				 size_t buf_len, int sps, int state, float threshold, void *stream)
{
	if (!ctx || (sps != 1 && sps != 4))
		return TRXHIP_EINVAL;                  /* sigProcLib.cpp:1814-1815 */
	/* window of the search (:1817-1838) */
	int target = 3 + 39 + 64, head, tail;
	switch (state) {
	case TRXHIP_SCH_DETECT_NARROW: head = 4; tail = 4; break;
	case TRXHIP_SCH_DETECT_BUFFER: target = 1; head = 0; tail = (12 * 8 * 625) / 4; break;
	case TRXHIP_SCH_DETECT_FULL:
	default: head = target - 1; tail = 39 + 3 + 9; break;
	}
	const int start = (target - head) * 1 - 1, len = (head + tail) * 1;
	if (buf_len < 4 * (size_t)len)
		return TRXHIP_EINVAL;
	if (n_bufs == 0)
		return TRXHIP_OK;
	if (!d_iq || !d_results || n_bufs > 0x7fffffffull)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	const int toa_sub = (state == TRXHIP_SCH_DETECT_BUFFER) ? 3 + 39 + 64 : head;      /* :1853-1858 */
	return trx_launch_sch_detect(d_iq, buf_len, d_results, ctx->d_tables, n_bufs, len, start, toa_sub, threshold,
				     ctx->sch_unit, static_cast<hipStream_t>(stream));
}

static int sch_sync_common(trxhip_ctx *ctx, const void *d_iq, int i16, size_t buf_stride, trxhip_sch_sync_result *d_results,
			   int8_t *d_bits, size_t n_bufs, size_t buf_len, int mode, float scale, void *stream)
{
	if (!ctx || !d_iq || !d_results || n_bufs == 0 || n_bufs > 0x7fffffffull || buf_stride < buf_len)
		return TRXHIP_EINVAL;
	if (mode == TRXHIP_SCH_SYNC_TRACK) {
		if (buf_len < 1 || buf_len > 0x7fffffffull)
			return TRXHIP_EINVAL;
	} else if (mode == TRXHIP_SCH_SYNC_ACQ) {
		/* search_stop_pos = len - 512 lags (grgsm_vitac.cpp:304), of which 20 make the first window */
		if (buf_len < 512 + 20 || buf_len > TRXHIP_SCH_SYNC_MAX_LEN)
			return TRXHIP_EINVAL;
	} else {
		return TRXHIP_EINVAL;
	}
	if (with_device(ctx))
		return TRXHIP_EIO;
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (mode == TRXHIP_SCH_SYNC_TRACK)
		return trx_launch_sch_sync(d_iq, i16, buf_stride, d_results, d_bits, n_bufs, (int)buf_len, 0, scale, nullptr, nullptr, st);
	trx_sch_scratch &sc = ctx->sch_sync;
	std::lock_guard<std::mutex> lock(sc.mu);
	if (!sc.acquire(n_bufs, buf_len - 512))
		return TRXHIP_ENOMEM;
	const int rc = trx_launch_sch_sync(d_iq, i16, buf_stride, d_results, d_bits, n_bufs, (int)buf_len, 1, scale, sc.d_power,
					   sc.d_best, st);
	sc.launched(st);
	return rc;
}

int trxhip_sch_sync_batch_cf32(trxhip_ctx *ctx, const float *d_iq, size_t buf_stride, trxhip_sch_sync_result *d_results,
			       int8_t *d_bits, size_t n_bufs, size_t buf_len, int mode, float scale, void *stream)
{
	return sch_sync_common(ctx, d_iq, 0, buf_stride, d_results, d_bits, n_bufs, buf_len, mode, scale, stream);
}

int trxhip_sch_sync_batch_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t buf_stride, trxhip_sch_sync_result *d_results,
			      int8_t *d_bits, size_t n_bufs, size_t buf_len, int mode, float scale, void *stream)
{
	return sch_sync_common(ctx, d_iq, 1, buf_stride, d_results, d_bits, n_bufs, buf_len, mode, scale, stream);
}

static int ms_rx_common(trxhip_ctx *ctx, const void *d_iq, int i16, size_t slot_stride, const trxhip_ms_slot *d_slots,
			trxhip_ms_burst_ind *d_ind, int8_t *d_bits, size_t n_slots, float rx_full_scale, void *stream)
{
	if (!ctx || !d_iq || !d_slots || !d_ind || n_slots == 0 || n_slots > 0x7fffffffull || slot_stride < 625)
		return TRXHIP_EINVAL;
	if (!std::isfinite(rx_full_scale) || rx_full_scale <= 0.0f)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	/* 1.f / float(rxFullScale) (ms_upper.cpp:203) */
	return trx_launch_ms_rx(d_iq, i16, slot_stride, d_slots, d_ind, d_bits, n_slots, 1.0f / rx_full_scale, rx_full_scale,
				static_cast<hipStream_t>(stream));
}

int trxhip_ms_rx_batch_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t slot_stride, const trxhip_ms_slot *d_slots,
			   trxhip_ms_burst_ind *d_ind, int8_t *d_bits, size_t n_slots, float rx_full_scale, void *stream)
{
	return ms_rx_common(ctx, d_iq, 1, slot_stride, d_slots, d_ind, d_bits, n_slots, rx_full_scale, stream);
}

int trxhip_ms_rx_batch_cf32(trxhip_ctx *ctx, const float *d_iq, size_t slot_stride, const trxhip_ms_slot *d_slots,
			    trxhip_ms_burst_ind *d_ind, int8_t *d_bits, size_t n_slots, float rx_full_scale, void *stream)
{
	return ms_rx_common(ctx, d_iq, 0, slot_stride, d_slots, d_ind, d_bits, n_slots, rx_full_scale, stream);
}

int trxhip_delay_vector_batch_cf32(trxhip_ctx *ctx, const float *d_in, float *d_out, const float *d_delays, size_t n_vec,
				   int len, void *stream)
{
	if (!ctx || len < 0)
		return TRXHIP_EINVAL;
	if (n_vec == 0 || len == 0)
		return TRXHIP_OK;
	if (!d_in || !d_out || !d_delays || d_in == d_out)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_delay_vector(d_in, d_out, d_delays, ctx->d_tables, n_vec, len, static_cast<hipStream_t>(stream));
}

int trxhip_scale_vector_cf32(trxhip_ctx *ctx, float *d_x, size_t len, float scale_re, float scale_im, void *stream)
{
	if (!ctx || (len && !d_x))
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_scale_vector(d_x, len, scale_re, scale_im, static_cast<hipStream_t>(stream));
}

int trxhip_demod_va_batch_cf32(trxhip_ctx *ctx, const float *d_iq, const trxhip_burst_params *d_params,
			       const trxhip_burst_result *d_detected, float *d_soft, int32_t *d_starts, size_t n_bursts,
			       int burst_len, float scale, int soft_stride, int flags, void *stream)
{
	if (!ctx || burst_len < 1 || burst_len > TRXHIP_MAX_BURST_LEN || soft_stride < 148)
		return TRXHIP_EINVAL;
	if (n_bursts == 0)
		return TRXHIP_OK;
	if (!d_iq || !d_params || !d_soft || n_bursts > 0x7fffffffull)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_va_demod(d_iq, d_params, d_detected, d_soft, d_starts, n_bursts, burst_len, scale, soft_stride, flags,
				   static_cast<hipStream_t>(stream));
}

int trxhip_vector_slicer(trxhip_ctx *ctx, float *d_dest, const float *d_src, size_t len, void *stream)
{
	if (!ctx || (len && (!d_dest || !d_src)))
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_vector_slicer(d_dest, d_src, len, static_cast<hipStream_t>(stream));
}

int trxhip_channelize_batch(trxhip_ctx *ctx, const int16_t *d_in, float *d_out, size_t n_blocks, int m,
			    int block_len, int h_len, void *stream)
{
	if (!ctx || !d_in || !d_out || block_len < 1)
		return TRXHIP_EINVAL;
	if (m != 4 || h_len != 16)
		return TRXHIP_ENOTSUP;                 /* the reference instantiates Channelizer(4, 192, 16) only */
	if ((reinterpret_cast<uintptr_t>(d_in) & 15) != 0)
		return TRXHIP_EINVAL;                  /* one 16-byte load per time step */
	if (with_device(ctx))
		return TRXHIP_EIO;
	const size_t n_total = n_blocks * (size_t)block_len;
	return trx_launch_channelize(d_in, d_out, n_total, n_total, ctx->d_tables, nullptr, static_cast<hipStream_t>(stream));
}

int trxhip_resample_batch(trxhip_ctx *ctx, const float *d_in, float *d_out, size_t n_in, int p, int q,
			  size_t n_chan, size_t in_stride, size_t out_stride, void *stream)
{
	if (!ctx || !d_in || !d_out)
		return TRXHIP_EINVAL;
	const int resamp = (p == 65 && q == 96) ? 0 : ((p == 52 && q == 75) ? 1 : -1);
	if (!((p == 65 && q == 48) || (p == 1 && q == 4) || resamp >= 0))
		return TRXHIP_ENOTSUP;                 /* Resampler(65,48) radioInterfaceMulti.cpp:35-36; (1,4) sigProcLib.cpp:2161;
		                                        * (65,96) and (52,75) radioInterfaceResamp.cpp:36-41 */
	if (n_in % q)
		return TRXHIP_EINVAL;                  /* Resampler.cpp:100-104 */
	if (with_device(ctx))
		return TRXHIP_EIO;
	const float *parts = (p == 65 && q == 48) ? &ctx->d_tables.p->rs6548_taps[0][0] : &ctx->d_tables.p->dec_taps[0];
	if (resamp >= 0) {
		std::lock_guard<std::mutex> lock(ctx->rs_mu);
		if (!ctx->d_rs_resamp[resamp]) {
			std::vector<float> taps((size_t)p * 16);
			trx_polyphase_taps((unsigned)p, (unsigned)q, 16, 1.0f, taps.data());
			trx_dev<float> d;
			if (d.alloc(taps.size()) != TRXHIP_OK)
				return TRXHIP_ENOMEM;
			if (hipMemcpy(d, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
				return TRXHIP_EIO;
			ctx->d_rs_resamp[resamp] = std::move(d);
		}
		parts = ctx->d_rs_resamp[resamp];
	}
	return trx_launch_resample(d_in, d_out, n_in, p, q, n_chan, in_stride, out_stride, parts, nullptr,
				   static_cast<hipStream_t>(stream));
}

/* ---- streaming Rx front end: RadioInterfaceMulti::pullBuffer (radioInterfaceMulti.cpp:237-314) and
 *      RadioInterfaceResamp::pullBuffer (radioInterfaceResamp.cpp:156-193) ---- */
enum { RXFE_FOUR_ROWS = -1 };    /* trxhip_rx_frontend_create(): all four filterbank channels in physical order */
struct trxhip_rx_frontend {
	trxhip_ctx *ctx;
	int mode;                /* RXFE_FOUR_ROWS, TRXHIP_RXFE_MULTI or TRXHIP_RXFE_RESAMP */
	int rows;                /* rows pull() writes: 4, chans, 1 */
	int block_len, p, q;
	trx_dev<float> d_parts;  /* [p][16] resampler partitions */
	trx_dev<char> d_wide_hist; /* 15 time steps x 4 int16 IQ samples; RESAMP: [2][16] int16 IQ samples, halves as d_chan_hist's */
	trx_dev<char> d_chan_hist; /* [2][4][16] complex64 ([2][rows][16] by logical channel in a MULTI object): the fused kernel reads
	                          * one half and leaves the other (its first and its last workgroup run at the same time) */
	int hist_cur;
	trx_dev<float> d_chan;   /* [4][d_chan.cap / 8] complex64: channelizer output scratch */
};

static int rxfe_create(trxhip_ctx *ctx, int mode, int rows, int block_len, int p, int q, trxhip_rx_frontend **out)
{
	if (!ctx || !out || block_len < 16 || p < 1 || q < 1 || p > 128 || q > 3072 || (block_len % q) != 0)
		return TRXHIP_EINVAL;                  /* Resampler::rotate needs whole q-sample groups per block (Resampler.cpp:100-112) */
	if (with_device(ctx))
		return TRXHIP_EIO;
	trxhip_rx_frontend *f = new (std::nothrow) trxhip_rx_frontend();
	if (!f)
		return TRXHIP_ENOMEM;
	f->ctx = ctx; f->mode = mode; f->rows = rows;
	f->block_len = block_len; f->p = p; f->q = q; f->hist_cur = 0;
	float *taps = static_cast<float *>(malloc((size_t)p * 16 * sizeof(float)));
	if (!taps) { delete f; return TRXHIP_ENOMEM; }
	trx_polyphase_taps((unsigned)p, (unsigned)q, 16, 1.0f, taps);
	bool ok = f->d_parts.alloc((size_t)p * 16) == TRXHIP_OK && f->d_wide_hist.alloc(16 * 16) == TRXHIP_OK &&
		  f->d_chan_hist.alloc(2 * 4 * 16 * 8) == TRXHIP_OK &&
		  hipMemcpy(f->d_parts, taps, (size_t)p * 16 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
		  hipMemset(f->d_wide_hist, 0, 16 * 16) == hipSuccess && hipMemset(f->d_chan_hist, 0, 2 * 4 * 16 * 8) == hipSuccess;
	free(taps);
	if (!ok) { trxhip_rx_frontend_destroy(f); return TRXHIP_ENOMEM; }
	*out = f;
	return TRXHIP_OK;
}

int trxhip_rx_frontend_create(trxhip_ctx *ctx, int block_len, int p, int q, trxhip_rx_frontend **out)
{
	return rxfe_create(ctx, RXFE_FOUR_ROWS, 4, block_len, p, q, out);
}

int trxhip_rx_frontend_create_chans(trxhip_ctx *ctx, int mode, int chans, int block_len, int p, int q, trxhip_rx_frontend **out)
{
	if (!ctx || !out || (mode != TRXHIP_RXFE_MULTI && mode != TRXHIP_RXFE_RESAMP))
		return TRXHIP_EINVAL;
	if (mode == TRXHIP_RXFE_MULTI ? (chans < 1 || chans > 3) : chans != 1)
		return TRXHIP_EINVAL;
	if (p >= 1 && p <= 128 && (long long)q * ((256 + p - 1) / p) > 3072)
		return TRXHIP_EINVAL;                  /* the resampler kernels' tile */
	return rxfe_create(ctx, mode, chans, block_len, p, q, out);
}

int trxhip_rx_frontend_rows(const trxhip_rx_frontend *f)
{
	return f ? f->rows : TRXHIP_EINVAL;
}

size_t trxhip_rx_frontend_out_samples(const trxhip_rx_frontend *f, size_t n_blocks)
{
	return f ? n_blocks * (size_t)f->block_len / f->q * f->p : 0;
}

int trx_rx_frontend_geometry(const trxhip_rx_frontend *f, trxhip_ctx **ctx, int *rows, int *resamp, int *block_len, int *p, int *q)
{
	if (!f || f->mode == RXFE_FOUR_ROWS)
		return TRXHIP_EINVAL;
	*ctx = f->ctx;
	*rows = f->rows;
	*resamp = f->mode == TRXHIP_RXFE_RESAMP;
	*block_len = f->block_len;
	*p = f->p;
	*q = f->q;
	return TRXHIP_OK;
}

void trxhip_rx_frontend_destroy(trxhip_rx_frontend *f)
{
	if (!f)
		return;
	(void)with_device(f->ctx);
	delete f;
}

int trxhip_rx_frontend_reset(trxhip_rx_frontend *f, void *stream)
{
	if (!f || with_device(f->ctx))
		return TRXHIP_EINVAL;
	if (hipMemsetAsync(f->d_wide_hist, 0, 16 * 16, static_cast<hipStream_t>(stream)) != hipSuccess ||
	    hipMemsetAsync(f->d_chan_hist, 0, 2 * 4 * 16 * 8, static_cast<hipStream_t>(stream)) != hipSuccess)
		return TRXHIP_EIO;
	return TRXHIP_OK;
}

int trxhip_rx_frontend_seed(trxhip_rx_frontend *f, const int16_t *d_wide_prev, size_t n_blocks_prev, void *stream)
{
	if (!f)
		return TRXHIP_EINVAL;
	int rc = trxhip_rx_frontend_reset(f, stream);
	if (rc || n_blocks_prev == 0)
		return rc;
	if (!d_wide_prev)
		return TRXHIP_EINVAL;
	/* run the preceding blocks through the very same two launches (their output is discarded): what they leave in
	 * d_wide_hist / d_chan_hist is the state of a stream processed up to here */
	const size_t n_out = n_blocks_prev * (size_t)f->block_len / f->q * f->p;
	trx_dev<float> scratch;
	if (scratch.alloc((size_t)f->rows * n_out * 2) != TRXHIP_OK)
		return TRXHIP_ENOMEM;
	rc = trxhip_rx_frontend_pull(f, d_wide_prev, n_blocks_prev, scratch, n_out, stream);
	if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess && rc == TRXHIP_OK)
		rc = TRXHIP_EIO;
	return rc;
}

int trxhip_rx_frontend_pull(trxhip_rx_frontend *f, const int16_t *d_wide, size_t n_blocks, float *d_out,
			    size_t out_stride, void *stream)
{
	if (!f || !d_wide || !d_out)
		return TRXHIP_EINVAL;
	if ((reinterpret_cast<uintptr_t>(d_wide) & (f->mode == TRXHIP_RXFE_RESAMP ? 3 : 15)) != 0)
		return TRXHIP_EINVAL;                  /* one 16-byte load per wideband time step; RESAMP: one 4-byte sample */
	if (n_blocks == 0)
		return TRXHIP_OK;
	if (with_device(f->ctx))
		return TRXHIP_EIO;
	const size_t n_total = n_blocks * (size_t)f->block_len;
	if (out_stride < n_total / f->q * f->p)
		return TRXHIP_EINVAL;
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (f->mode == TRXHIP_RXFE_RESAMP) {
		/* int16 in, one row out (trx_rx_frontend.hip, rx_resamp_s16_kernel); the kernel reads one half of the carried samples
		 * and leaves the other */
		char *const sh = f->d_wide_hist;
		const int rc = trx_launch_rx_resamp_s16(d_wide, d_out, n_total, f->p, f->q, f->d_parts, sh + (size_t)f->hist_cur * 64,
							sh + (size_t)(f->hist_cur ^ 1) * 64, s);
		if (rc == 0)
			f->hist_cur ^= 1;
		return rc;
	}
	/* the four-row object: rows = the filterbank paths; a MULTI object: the active paths only, row l = logical channel l */
	const size_t half = (size_t)f->rows * 16 * 8;
	char *const hist = f->d_chan_hist;
	char *const hist_in = hist + (size_t)f->hist_cur * half, *const hist_out = hist + (size_t)(f->hist_cur ^ 1) * half;
	/* one pass, the channel-rate streams stay on the chip (trx_rx_frontend.hip, frontend_fused_kernel<rows>) ... */
	int rc = trx_launch_frontend_fused(d_wide, d_out, n_total, f->rows, f->p, f->q, out_stride, f->d_parts, f->ctx->d_tables,
					   f->d_wide_hist, hist_in, hist_out, s);
	if (rc == 0)
		f->hist_cur ^= 1;
	if (rc != 1)
		return rc;
	/* ... or, for a geometry that fits no tile, the two kernels with the channel streams in a scratch buffer */
	if ((rc = f->d_chan.reserve(4 * n_total * 2)) != TRXHIP_OK)
		return rc;
	const size_t cap = f->d_chan.cap / 8;                  /* samples per row */
	rc = trx_launch_channelize(d_wide, f->d_chan, n_total, cap, f->ctx->d_tables, f->d_wide_hist, s);
	if (f->mode == RXFE_FOUR_ROWS)
		return rc ? rc : trx_launch_resample(f->d_chan, d_out, n_total, f->p, f->q, 4, cap, out_stride, f->d_parts, hist_in, s);
	for (int l = 0; l < f->rows && rc == TRXHIP_OK; l++)
		rc = trx_launch_resample(f->d_chan + 2 * (size_t)trx_arfcn_pchan(f->rows, l) * cap, d_out + 2 * (size_t)l * out_stride,
					 n_total, f->p, f->q, 1, cap, out_stride, f->d_parts, hist_in + (size_t)l * 16 * 8, s);
	return rc;
}


int trxhip_synthesize_batch(trxhip_ctx *ctx, const float *d_in, size_t in_stride, float *d_out, size_t n_blocks, int m,
			    int block_len, int h_len, void *stream)
{
	if (!ctx || !d_in || !d_out || block_len < 1)
		return TRXHIP_EINVAL;
	if (m != 4 || h_len != 16)
		return TRXHIP_ENOTSUP;                 /* the reference instantiates Synthesis(4, 192, 16) only */
	const size_t n_total = n_blocks * (size_t)block_len;
	if (n_total == 0)
		return TRXHIP_OK;
	if (in_stride < n_total)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	return trx_launch_synthesize(d_in, in_stride, nullptr, d_out, nullptr, 0.0f, n_total, ctx->d_tables,
				     static_cast<hipStream_t>(stream));
}

/* ---- streaming Tx front end: RadioInterfaceMulti::pushBuffer (radioInterfaceMulti.cpp:316-362) and
 *      RadioInterfaceResamp::pushBuffer (radioInterfaceResamp.cpp:196-230) ---- */
struct trxhip_tx_frontend {
	trxhip_ctx *ctx;
	int mode, chans, block_len, p, q;
	bool fused;              /* MULTI whose geometry fits the fused kernel's tiles */
	int hl;                  /* fused: low-rate samples of history per logical channel */
	trx_dev<float> d_parts;  /* [p][16] resampler partitions, Resampler::initFilters(bw) */
	trx_dev<char> d_hist;    /* fused: [chans][hl] complex64, the low-rate samples -hl .. -1 */
	trx_dev<char> d_rs_hist; /* otherwise: resample_kernel's [chans][16] (samples -15 .. -1 at 0 .. 14) */
	trx_dev<char> d_row_hist; /* MULTI unfused: [4][16], the channel-rate rows' samples -15 .. -1 */
	trx_dev<float> d_scratch; /* complex64; MULTI unfused: [4][cap] channel-rate rows; RESAMP: cap resampled samples (int16-only output) */
};

static size_t txfe_out_per_block(const trxhip_tx_frontend *f)
{
	return (size_t)f->block_len / f->q * f->p * (f->mode == TRXHIP_TXFE_MULTI ? 4 : 1);
}

int trx_tx_frontend_geometry(const trxhip_tx_frontend *f, int *chans, int *block_len, size_t *out_per_block)
{
	if (!f)
		return TRXHIP_EINVAL;
	*chans = f->chans;
	*block_len = f->block_len;
	*out_per_block = txfe_out_per_block(f);
	return TRXHIP_OK;
}

int trxhip_tx_frontend_create(trxhip_ctx *ctx, int mode, int chans, int block_len, int p, int q, float bw, trxhip_tx_frontend **out)
{
	if (!ctx || !out || (mode != TRXHIP_TXFE_MULTI && mode != TRXHIP_TXFE_RESAMP))
		return TRXHIP_EINVAL;
	if (mode == TRXHIP_TXFE_MULTI ? (chans < 1 || chans > 3) : chans != 1)
		return TRXHIP_EINVAL;
	if (p < 1 || p > 128 || q < 1 || block_len < 1 || (block_len % q) != 0 || !(bw > 0.0f) || !std::isfinite(bw))
		return TRXHIP_EINVAL;                  /* Resampler::rotate needs whole q-sample groups per block (Resampler.cpp:100-112) */
	if ((long long)q * ((256 + p - 1) / p) > 3072)
		return TRXHIP_EINVAL;                  /* resample_kernel's tile */
	if (with_device(ctx))
		return TRXHIP_EIO;
	trxhip_tx_frontend *f = new (std::nothrow) trxhip_tx_frontend();
	if (!f)
		return TRXHIP_ENOMEM;
	f->ctx = ctx; f->mode = mode; f->chans = chans; f->block_len = block_len; f->p = p; f->q = q;
	f->hl = 15 + (15 * q + p - 1) / p;
	f->fused = mode == TRXHIP_TXFE_MULTI && trx_tx_fused_tm(p, q) > 0 && f->hl <= 256;
	float *taps = static_cast<float *>(malloc((size_t)p * 16 * sizeof(float)));
	if (!taps) { delete f; return TRXHIP_ENOMEM; }
	trx_polyphase_taps((unsigned)p, (unsigned)q, 16, bw, taps);
	bool ok = f->d_parts.alloc((size_t)p * 16) == TRXHIP_OK &&
		  hipMemcpy(f->d_parts, taps, (size_t)p * 16 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
		  f->d_hist.alloc((size_t)chans * f->hl * 8) == TRXHIP_OK && f->d_rs_hist.alloc((size_t)chans * 16 * 8) == TRXHIP_OK &&
		  f->d_row_hist.alloc(4 * 16 * 8) == TRXHIP_OK;
	free(taps);
	if (!ok || trxhip_tx_frontend_reset(f, nullptr) != TRXHIP_OK || hipDeviceSynchronize() != hipSuccess) {
		trxhip_tx_frontend_destroy(f);
		return TRXHIP_ENOMEM;
	}
	*out = f;
	return TRXHIP_OK;
}

void trxhip_tx_frontend_destroy(trxhip_tx_frontend *f)
{
	if (!f)
		return;
	(void)with_device(f->ctx);
	delete f;
}

int trxhip_tx_frontend_reset(trxhip_tx_frontend *f, void *stream)
{
	if (!f || with_device(f->ctx))
		return TRXHIP_EINVAL;
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (hipMemsetAsync(f->d_hist, 0, (size_t)f->chans * f->hl * 8, s) != hipSuccess ||
	    hipMemsetAsync(f->d_rs_hist, 0, (size_t)f->chans * 16 * 8, s) != hipSuccess ||
	    hipMemsetAsync(f->d_row_hist, 0, 4 * 16 * 8, s) != hipSuccess)
		return TRXHIP_EIO;
	return TRXHIP_OK;
}

int trxhip_tx_frontend_seed(trxhip_tx_frontend *f, const float *d_in_prev, size_t in_stride, size_t n_blocks_prev, void *stream)
{
	if (!f)
		return TRXHIP_EINVAL;
	int rc = trxhip_tx_frontend_reset(f, stream);
	if (rc || n_blocks_prev == 0)
		return rc;
	if (!d_in_prev)
		return TRXHIP_EINVAL;
	/* run the preceding blocks through the very same launches (their output is discarded): what they leave behind is the
	 * state of a stream processed up to here */
	trx_dev<float> scratch;
	if (scratch.alloc(n_blocks_prev * txfe_out_per_block(f) * 2) != TRXHIP_OK)
		return TRXHIP_ENOMEM;
	rc = trxhip_tx_frontend_push(f, d_in_prev, in_stride, n_blocks_prev, scratch, nullptr, 0.0f, stream);
	if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess && rc == TRXHIP_OK)
		rc = TRXHIP_EIO;
	return rc;
}

/* room for n samples per row, zeroed when it grows: the rows of inactive paths stay zero */
static int txfe_scratch(trxhip_tx_frontend *f, size_t n, hipStream_t s)
{
	const size_t floats = (f->mode == TRXHIP_TXFE_MULTI ? 4 : 1) * n * 2;
	if (floats <= f->d_scratch.cap)
		return TRXHIP_OK;
	const int rc = f->d_scratch.reserve(floats);
	if (rc != TRXHIP_OK || hipMemsetAsync(f->d_scratch, 0, floats * sizeof(float), s) == hipSuccess)
		return rc;
	(void)f->d_scratch.reset();
	return TRXHIP_EIO;
}

int trxhip_tx_frontend_push(trxhip_tx_frontend *f, const float *d_in, size_t in_stride, size_t n_blocks, float *d_out_cf32,
			    int16_t *d_out_s16, float s16_scale, void *stream)
{
	if (!f || !d_in || (!d_out_cf32 && !d_out_s16))
		return TRXHIP_EINVAL;
	if ((reinterpret_cast<uintptr_t>(d_in) & 7) != 0 || (reinterpret_cast<uintptr_t>(d_out_cf32) & 7) != 0 ||
	    (reinterpret_cast<uintptr_t>(d_out_s16) & 3) != 0)
		return TRXHIP_EINVAL;
	if (n_blocks == 0)
		return TRXHIP_OK;
	const size_t n_in = n_blocks * (size_t)f->block_len;
	if (f->chans > 1 && in_stride < n_in)
		return TRXHIP_EINVAL;
	if (with_device(f->ctx))
		return TRXHIP_EIO;
	hipStream_t s = static_cast<hipStream_t>(stream);
	const size_t n_times = n_in / f->q * f->p;                /* channel-rate samples per path */
	int rc;
	if (f->mode == TRXHIP_TXFE_RESAMP) {
		float *cf = d_out_cf32;
		if (!cf) {
			if ((rc = txfe_scratch(f, n_times, s)) != TRXHIP_OK)
				return rc;
			cf = f->d_scratch;
		}
		rc = trx_launch_resample(d_in, cf, n_in, f->p, f->q, 1, in_stride, n_times, f->d_parts, f->d_rs_hist, s);
		if (rc == TRXHIP_OK && d_out_s16)
			rc = trx_launch_convert_float_short(d_out_s16, cf, s16_scale, 2 * n_times, s);
		return rc;
	}
	if (f->fused) {
		/* one pass, the channel-rate rows stay on the chip (trx_tx_frontend.hip, tx_frontend_fused_kernel) */
		rc = trx_launch_tx_frontend_fused(d_in, in_stride, n_in, f->d_hist, f->hl, d_out_cf32, d_out_s16, s16_scale, f->chans, f->p,
						  f->q, f->d_parts, f->ctx->d_tables, s);
		if (rc != 1)
			return rc ? rc : trx_launch_tx_save_hist(d_in, n_in, in_stride, f->chans, f->d_hist, f->hl, f->hl, s);
	}
	/* a geometry that does not fit the fused kernel's tiles: the resampler into channel-rate rows, then the synthesis bank */
	if ((rc = txfe_scratch(f, n_times, s)) != TRXHIP_OK)
		return rc;
	const size_t cap = f->d_scratch.cap / 8;               /* samples per row */
	for (int l = 0; l < f->chans; l++) {
		const int pc = trx_arfcn_pchan(f->chans, l);
		rc = trx_launch_resample(d_in + 2 * (size_t)l * in_stride, f->d_scratch + 2 * (size_t)pc * cap, n_in, f->p, f->q, 1,
					 in_stride, cap, f->d_parts, f->d_rs_hist + (size_t)l * 16 * 8, s);
		if (rc)
			return rc;
	}
	rc = trx_launch_synthesize(f->d_scratch, cap, f->d_row_hist, d_out_cf32, d_out_s16, s16_scale, n_times, f->ctx->d_tables, s);
	if (rc)
		return rc;
	return trx_launch_tx_save_hist(f->d_scratch, n_times, cap, 4, f->d_row_hist, 15, 16, s);
}

}  // extern "C"
