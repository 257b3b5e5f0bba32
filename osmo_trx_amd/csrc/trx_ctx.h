// trx_ctx.h -- the context object behind trxhip_ctx* (internal to csrc/; the C ABI only hands out the pointer).
#ifndef TRX_CTX_H
#define TRX_CTX_H
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include "../../include/trxhip.h"
#include "trx_tables.h"
#include "trx_tx_tables.h"
#include "trx_mem.h"

#define TRX_POOL_SLOTS 1024
#define TRX_REDO_SLOTS 4

/* The lists of bursts the normal-burst kernel (trx_kernel_nb.hip) leaves to the general kernel: TRX_REDO_SLOTS device buffers of
 * TRX_REDO_HDR words + one flag byte per burst, handed out round-robin per split launch under `mu` (held from acquire() to
 * launched()).  A slot's header is zero between launches (the general kernel's last workgroup re-arms it); its event marks the
 * end of the launch pair that used it last -- a slot is only handed out again (or re-allocated larger) once that event has
 * completed.
 * Feedback: the general kernel reports (into the slot's pinned word h_left) how many bursts the normal-burst kernel left it.
 * Read when the slot comes round again: a batch that left more than 1/32 of its bursts -- slots of other types the caller gave
 * no hint about -- makes the next 63 eligible launches run the general kernel alone (every left burst is read twice and stalls
 * the first kernel's prefetch), then one launch probes again. */
struct trx_redo_lists {
	struct slot {
		trx_dev<unsigned> d;           /* TRX_REDO_HDR words + one flag byte per burst */
		trx_pin<unsigned> h_left;
		size_t n_last = 0;             /* bursts of the launch that used the slot last */
		trx_event ev;                  /* pending: recorded after a launch that has not been waited for */
	};
	std::mutex mu;
	slot s[TRX_REDO_SLOTS];
	unsigned next = 0;
	unsigned backoff = 0;

	/* every slot's event and pinned word; TRXHIP_ENOMEM: out of memory */
	int create()
	{
		for (slot &sl : s)
			if (sl.ev.create() != TRXHIP_OK || sl.h_left.alloc(16) != TRXHIP_OK)
				return TRXHIP_ENOMEM;
		return TRXHIP_OK;
	}
	/* the slot for a split launch of n bursts on `stream`, or NULL: back-off, or no list buffer (the general kernel alone) */
	slot *acquire(size_t n, hipStream_t stream)
	{
		if (backoff) {
			backoff--;
			return nullptr;
		}
		slot &sl = s[next++ % TRX_REDO_SLOTS];
		if (sl.ev.pending()) {
			if (sl.ev.wait() != TRXHIP_OK)
				return nullptr;
			if (sl.n_last && (size_t)*reinterpret_cast<volatile unsigned *>(sl.h_left.p) * 32 > sl.n_last)
				backoff = 63;
		}
		*sl.h_left = 0u;
		sl.n_last = n;
		/* header words + one flag byte per burst (room for 65536 at the least), padded to whole chunks of 256 */
		const size_t words = TRX_REDO_HDR + (((n < 65536 ? 65536 : n) + 255) & ~(size_t)255) / sizeof(unsigned);
		if (sl.d.cap < words) {
			/* all zero between launches.  The memset goes on the caller's stream, ahead of the two kernels that use the buffer
			 * (the slot's last launch has completed) */
			if (sl.d.reserve(words) != TRXHIP_OK || hipMemsetAsync(sl.d, 0, words * sizeof(unsigned), stream) != hipSuccess) {
				(void)sl.d.reset();
				return nullptr;
			}
		}
		return &sl;
	}
	/* after the launch into sl (rc: its result) */
	void launched(slot &sl, int rc, hipStream_t stream)
	{
		if (rc == 0 && sl.ev.record(stream) != TRXHIP_OK)
			(void)hipStreamSynchronize(stream);   /* no event: the slot is free once the stream has drained */
	}
};

/* Scratch of trxhip_sch_sync_batch_*() in ACQ mode (trx_sch_sync.hip): the correlation powers of every lag, n_bufs x (len - 512)
 * floats, and the chosen window per buffer.  One pair per context, grown on demand and reused from call to call: `mu` is held
 * from acquire() to launched(), and the buffers are handed out again only once the launches that used them last have completed
 * (the event), so ACQ calls on one context from several threads or streams run one behind the other. */
struct trx_sch_scratch {
	std::mutex mu;
	trx_dev<float> d_power;
	trx_dev<int32_t> d_best;           /* one per buffer */
	trx_event ev;

	/* room for n_bufs buffers of n_lags lags; false: out of memory */
	bool acquire(size_t n_bufs, size_t n_lags)
	{
		return ev.create() == TRXHIP_OK && ev.wait() == TRXHIP_OK && d_power.reserve(n_bufs * n_lags) == TRXHIP_OK &&
		       d_best.reserve(n_bufs) == TRXHIP_OK;
	}
	void launched(hipStream_t stream)
	{
		if (ev.record(stream) != TRXHIP_OK)
			(void)hipStreamSynchronize(stream);
	}
};

/* Work array of trxhip_ms_fcch_search_*() (trx_ms_fsearch.hip): one 64-byte candidate per (buffer, segment).  One per context,
 * grown on demand and kept, under the rules of trx_sch_scratch: `mu` is held from acquire() to launched(), and the array is handed
 * out to another stream, or freed to grow, only once the launches that used it last have completed; calls on one stream follow each
 * other without a wait. */
struct trx_fsearch_scratch {
	std::mutex mu;
	trx_dev<trxhip_ms_fcch_hit> d_cand;
	hipStream_t last = nullptr;        /* the stream of the launches the event is behind */
	trx_event ev;

	bool acquire(size_t n_cand, hipStream_t stream)
	{
		if (ev.create() != TRXHIP_OK)
			return false;
		if ((stream != last || d_cand.cap < n_cand) && ev.wait() != TRXHIP_OK)     /* the same stream orders the calls itself: no wait */
			return false;
		return d_cand.reserve(n_cand) == TRXHIP_OK;
	}
	void launched(hipStream_t stream)
	{
		last = stream;
		if (ev.record(stream) != TRXHIP_OK)
			(void)hipStreamSynchronize(stream);
	}
};

struct trxhip_ctx {
	int device = 0;
	int n_cu = 0;
	trx_dev<trx_tables> d_tables;
	int no_unit = 0;    /* tables do not have the compiled-in unit structure: keep the multiplying correlation */
	int sch_unit = 0;   /* the SCH sequence has the unit structure the kernel's compiled-in mask expects (trx_sch.hip) */
	int no_sym = 0;     /* decimator taps not bitwise symmetric: the kernels' straight-line paths (mirrored taps) are off */
	int no_fast = 0;    /* sinc LUT row sums above TRX_FAST_W: the fused kernels' FAST detector (proven margins) is off */
	/* cross-die work pool of the 4-SPS kernel (trx_kernel4.hip): TRX_POOL_SLOTS counter pairs {drawn, workgroups done} of 64
	 * bytes each, handed out round-robin PER LAUNCH.  The kernel re-arms its pair itself -- the last workgroup to finish
	 * zeroes both words -- so there is no memset in front of a launch: nothing that two host threads launching on one stream
	 * could interleave (round 4's per-stream counter was zeroed by a hipMemsetAsync queued separately from the launch: memset A,
	 * memset B, kernel A, kernel B left kernel B without a pool), no table of streams that fills up, and a launch
	 * captured into a HIP graph is complete in itself (replays of one graph serialise).  Two launches share a pair only when
	 * they are TRX_POOL_SLOTS pooled launches apart and still overlap -- 1024 outstanding batches of >= 32768 bursts. */
	trx_dev<unsigned> d_pool;
	int pool_enabled = 1;              /* trxhip_set_work_pool(); 0 when TRXHIP_NO_POOL is set at creation */
	std::atomic<unsigned> pool_next{0u};
	int nb_enabled = 1;                /* trxhip_set_nb_kernel(); 0 when TRXHIP_NO_NB_KERNEL is set at creation */
	trx_redo_lists redo;
	trx_dev<trx_tx_tables> d_tx_tables;     /* transmit tables (trx_tx.hip), uploaded at creation */
	/* trxhip_modulate_trxd_batch(): (float)(full_scale * pow(10, -att / 20.0)) for att = 0 .. 255, for the last full_scale */
	std::mutex tx_mu;
	double tx_full_scale = 0.0;
	bool tx_att_valid = false;
	float tx_att_scale[256];
	/* trxhip_resample_batch(): the partitions [p][16] of RadioInterfaceResamp's receive ratios (65, 96) and (52, 75), cutoff 1.0,
	 * uploaded on first use */
	std::mutex rs_mu;
	trx_dev<float> d_rs_resamp[2];
	trx_sch_scratch sch_sync;
	trx_fsearch_scratch fsearch;
	trx_dev<float> d_nco_tab;          /* the NCO's two phasor tables (trx_ms_nco.h): 4096 floats, made on the host and uploaded at creation */
};

static inline int with_device(const trxhip_ctx *ctx)
{
	return hipSetDevice(ctx->device) == hipSuccess ? 0 : TRXHIP_EIO;
}
#endif
