// trx_ms_sched.hip -- the MS-side downlink slot scheduler: the radio's sample stream in, burst indications out.
//
// The counterpart of trx_rx_sched.hip on the MS side.  It restates what the reference does between the radio's receive buffers
// and upper_trx::pullRadioVector():
//   ms_trx::search_for_sch() / handle_sch(true)   ms/ms_rx_lower.cpp:310-352, :157-205   first acquisition (trxhip_ms_sched_acquire_*)
//   ms_trx::grab_bursts()                         ms/ms_rx_lower.cpp:354-422             the cutter (trxhip_ms_sched_pull_*)
//   ms_trx::handle_sch_or_nb() / handle_sch(false) :130-153, :157-205                    what a cut slot is, temp_ts_corr_offset
//   time_keeper                                   ms/ms.h:160-221                        the GSM clock and its timestamp
// A pull is: the plan on the host (cut position, clock, count -- integers), ms_join_kernel (the slot that straddles the carried
// partial slot and the chunk is assembled into a row; the chunk's tail is saved as the new partial slot) and the stream instance
// of ms_rx_kernel (trx_ms_rx.hip) over every slot of the pull, read where it lies.  The cut position depends on SCH results of
// the device in two places, which are the scheduler's only waits (see include/trxhip.h).  Per SCH-carrying launch the correction
// is summed on the device into one word that starts at zero and is copied to a pinned mailbox behind the launch; the host adds
// it to temp_ts_corr_offset when the next pull plans.
// With ctx == NULL the object is plan-only: cutter, clock and plan, no device memory; SCH starts come from a queue.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_sched.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kMaxSamples = (size_t)1 << 40;

// ------------------------------------------------------------------------------------------------
// ms_join_kernel: one block.  The stream of a pull is the carried partial slot (rem_in, `carried` samples) followed by the chunk.
//   do_edge : its first 625 samples, the one slot that does not lie in the chunk, are assembled into edge_row (:385-394)
//   the new partial slot (:419-421) goes to the OTHER half of the partial-slot area: the first `keep` samples of the old one
//   (a chunk shorter than the missing part: :388-391) and n_tail samples of the chunk from tail_at on
// T: one IQ sample (uint32_t: int16 pair; float2).  carried + (625 - carried) <= 625, keep + n_tail < 625.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads)
ms_join_kernel(const T *__restrict__ in, const T *__restrict__ rem_in, T *__restrict__ rem_out, T *__restrict__ edge_row,
	       uint32_t carried, int do_edge, uint32_t keep, size_t tail_at, uint32_t n_tail)
{
	if (do_edge)
		for (uint32_t i = threadIdx.x; i < TRX_MSS_SLOT; i += kThreads)
			edge_row[i] = i < carried ? rem_in[i] : in[i - carried];
	for (uint32_t i = threadIdx.x; i < keep; i += kThreads)
		rem_out[i] = rem_in[i];
	for (uint32_t i = threadIdx.x; i < n_tail; i += kThreads)
		rem_out[keep + i] = in[tail_at + i];
}

}  // namespace

struct trxhip_ms_sched {
	trxhip_ctx *ctx = nullptr;
	float rx_full_scale = 0.0f;
	uint8_t tsc = 0, active = 0;
	bool tracking = false;
	// time_keeper, and grab_bursts()' statics
	bool clock_set = false, first_call = false;
	uint32_t fn = 0;
	int tn = 0;
	int64_t ts = 0;
	int64_t first_sch_ts_start = -1;       /* ms.h:261 */
	uint32_t carried = 0;                  /* partial_rdofs */
	int carried_cf32 = 0;                  /* its format */
	int64_t pending = 0;                   /* temp_ts_corr_offset, without what `unread` says is still on its way */
	bool unread = false;                   /* a launch with SCH slots was issued: its sum arrives in *h_corr behind ev_corr */
	int64_t to_skip_last = 0;
	uint64_t clock_jumps = 0, pulls = 0, slots = 0, sch_slots = 0;
	// the last pull, for trxhip_ms_sched_plan()
	struct {
		uint32_t fn0 = 0;                  /* the clock of slot 0 */
		int tn0 = 0;
		size_t n = 0;
		bool straddle = false;
		uint32_t carried = 0;
		int64_t to_skip = 0, first_ts = 0;
		uint8_t tsc = 0, active = 0;
	} last;
	// plan-only: the SCH starts fed from outside
	std::vector<int32_t> feed;
	size_t feed_at = 0;
	// device state (ctx != NULL)
	void *d_rem = nullptr;                 /* [2][TRX_MSS_REM_STRIDE] samples of either format */
	void *d_edge_row = nullptr;            /* 625 samples of either format */
	int32_t *d_corr = nullptr, *h_corr = nullptr;
	trxhip_sch_sync_result *d_acq = nullptr, *h_acq = nullptr;
	int rem_half = 0;                      /* the half the next pull reads */
	hipEvent_t ev_corr = nullptr, ev = nullptr;
	bool ev_used = false;
};

namespace {

int launched() { return hipGetLastError() == hipSuccess ? TRXHIP_OK : TRXHIP_EIO; }

// the sum of a launch in flight joins temp_ts_corr_offset: the wait of the pull behind a pull that cut an SCH slot
int fold_correction(trxhip_ms_sched *s)
{
	if (!s->unread)
		return TRXHIP_OK;
	if (with_device(s->ctx) || hipEventSynchronize(s->ev_corr) != hipSuccess)
		return TRXHIP_EIO;
	s->pending += *s->h_corr;
	s->unread = false;
	return TRXHIP_OK;
}

// inc_and_update_safe()'s asserts (ms.h:192-194): diff < 1.5 * 625 and diff > 0.5 * 625
bool jump(int64_t diff) { return !(2 * diff < 3 * TRX_MSS_SLOT) || !(2 * diff > TRX_MSS_SLOT); }

int launch_join(trxhip_ms_sched *s, const void *d_in, int cf32, int do_edge, uint32_t keep, size_t tail_at, uint32_t n_tail,
		hipStream_t st)
{
	const size_t esz = cf32 ? 8 : 4;
	const char *rem_in = static_cast<const char *>(s->d_rem) + (size_t)s->rem_half * TRX_MSS_REM_STRIDE * esz;
	char *rem_out = static_cast<char *>(s->d_rem) + (size_t)(s->rem_half ^ 1) * TRX_MSS_REM_STRIDE * esz;
	if (cf32)
		hipLaunchKernelGGL(ms_join_kernel<float2>, dim3(1), dim3(kThreads), 0, st, static_cast<const float2 *>(d_in),
				   reinterpret_cast<const float2 *>(rem_in), reinterpret_cast<float2 *>(rem_out),
				   static_cast<float2 *>(s->d_edge_row), s->carried, do_edge, keep, tail_at, n_tail);
	else
		hipLaunchKernelGGL(ms_join_kernel<uint32_t>, dim3(1), dim3(kThreads), 0, st, static_cast<const uint32_t *>(d_in),
				   reinterpret_cast<const uint32_t *>(rem_in), reinterpret_cast<uint32_t *>(rem_out),
				   static_cast<uint32_t *>(s->d_edge_row), s->carried, do_edge, keep, tail_at, n_tail);
	return launched();
}

// the stream instance of ms_rx_kernel over `cnt` slots whose first has the clock (fn0, tn0); sum: the launch holds SCH slots
// whose starts the cutter follows -- the correction word starts at zero and goes to the mailbox behind the launch
int launch_rx(trxhip_ms_sched *s, const void *d_in, int cf32, bool edge, int64_t first, uint32_t fn0, int tn0, trxhip_ms_burst_ind *d_ind,
	      int8_t *d_bits, size_t cnt, bool sum, hipStream_t st)
{
	trx_mss_stream sa;
	memset(&sa, 0, sizeof(sa));
	sa.edge_row = edge ? s->d_edge_row : nullptr;
	sa.first = first;
	sa.corr = sum ? s->d_corr : nullptr;
	sa.fn0 = fn0;
	sa.tn0 = (uint8_t)tn0;
	sa.tsc = s->tsc;
	sa.active = s->active;
	if (sum && hipMemsetAsync(s->d_corr, 0, sizeof(int32_t), st) != hipSuccess)
		return TRXHIP_EIO;
	/* 1.f / float(rxFullScale) (ms_upper.cpp:203), as trxhip_ms_rx_batch_*() */
	if (trx_launch_ms_rx_stream(d_in, !cf32, &sa, d_ind, d_bits, cnt, 1.0f / s->rx_full_scale, s->rx_full_scale, st) != 0)
		return TRXHIP_EIO;
	if (sum && (hipMemcpyAsync(s->h_corr, s->d_corr, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipEventRecord(s->ev_corr, st) != hipSuccess))
		return TRXHIP_EIO;
	return TRXHIP_OK;
}

// plan-only: the next fed start as handle_sch(false) would add it (:199-203)
int64_t fed_correction(const trxhip_ms_sched *s, size_t &at)
{
	if (at >= s->feed.size())
		return 0;
	const int32_t start = s->feed[at++];
	if (start == TRXHIP_MS_SCHED_NO_SCH || (start <= 1 && start >= -1))
		return 0;
	return -(int64_t)start;
}

int pull(trxhip_ms_sched *s, const void *d_in, int cf32, size_t n_samples, int64_t first_ts, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
	 size_t out_slots, size_t *n_slots, size_t *n_carried, void *stream)
{
	if (!s || !s->clock_set || n_samples == 0 || n_samples > kMaxSamples)
		return TRXHIP_EINVAL;
	if (s->carried && cf32 != s->carried_cf32)
		return TRXHIP_EINVAL;
	if (s->ctx) {
		if (!d_in || (reinterpret_cast<uintptr_t>(d_in) & (cf32 ? 7 : 3)) || !d_ind || (reinterpret_cast<uintptr_t>(d_ind) & 3))
			return TRXHIP_EINVAL;
		if (with_device(s->ctx))
			return TRXHIP_EIO;
	} else if (d_in || d_ind || d_bits) {
		return TRXHIP_EINVAL;                                  /* a plan-only object takes no buffers */
	}
	const hipStream_t st = static_cast<hipStream_t>(stream);
	const int64_t n = (int64_t)n_samples;
	uint32_t fn = s->fn;
	int tn = s->tn;
	int64_t ts = s->ts;
	size_t feed_at = s->feed_at;
	uint64_t jumps = 0;

	// partial burst samples read from the last buffer: a chunk shorter than the missing part only extends them (:385-391)
	if (!s->first_call && s->carried && n_samples < TRX_MSS_SLOT - s->carried) {
		if (s->ctx) {
			if (launch_join(s, d_in, cf32, 0, s->carried, 0, (uint32_t)n_samples, st) != TRXHIP_OK ||
			    hipEventRecord(s->ev, st) != hipSuccess)
				return TRXHIP_EIO;
			s->ev_used = true;
			s->rem_half ^= 1;
		}
		s->carried += (uint32_t)n_samples;
		s->carried_cf32 = cf32;
		s->last.n = 0;
		s->pulls++;
		if (n_slots)
			*n_slots = 0;
		if (n_carried)
			*n_carried = s->carried;
		return TRXHIP_OK;
	}

	// the correction of the pull before: the first of the two waits
	if (s->tracking && fold_correction(s) != TRXHIP_OK)
		return TRXHIP_EIO;
	int64_t pending = s->pending;
	int64_t to_skip = 0;

	// round up to next burst by calculating the time between sch detection and now (:362-383)
	if (s->first_call) {
		const int64_t next_burst_start = first_ts - s->first_sch_ts_start;
		const int64_t fullts = next_burst_start / TRX_MSS_SLOT, fracts = next_burst_start % TRX_MSS_SLOT;
		to_skip = TRX_MSS_SLOT - fracts;
		/* fullts inc_and_update() (none when fullts <= 0), inc_both() when fracts, dec_by_one(): TNs on the clock; the final
		 * set() keeps the clock and overwrites every timestamp the steps left */
		int64_t steps = (fullts > 0 ? fullts : 0) + (fracts ? 1 : 0) - 1;
		const int64_t period = (int64_t)TRX_MSS_HYPERFRAME * 8;
		steps = ((steps % period) + period) % period;
		trx_mss_clock_add(fn, tn, (uint64_t)steps, &fn, &tn);
		ts = first_ts - TRX_MSS_SLOT + to_skip;
	}

	const uint32_t carried = s->first_call ? 0u : s->carried;      /* (an acquire drops the partial slot) */
	const bool straddle = carried != 0;
	const uint32_t fnb = fn;                                       /* slot k of the pull: k + 1 incTN() behind (fnb, tnb) */
	const int tnb = tn;
	bool waited = false;
	if (straddle) {
		if (s->ctx && out_slots < 1)
			return TRXHIP_EINVAL;
		jumps += jump(first_ts - carried - ts);                    /* inc_and_update_safe(first_ts - partial_rdofs), :393 */
		trx_mss_clock_add(fn, tn, 1, &fn, &tn);
		ts = first_ts - carried;
		// handle_sch_or_nb() on the completed slot comes before the correction is applied (:394, :399): where it is an SCH slot
		// the cutter follows, this slot alone is demodulated first -- the second of the two waits
		if (s->tracking && trx_mss_is_sch(fn, tn)) {
			if (s->ctx) {
				if (launch_join(s, d_in, cf32, 1, 0, 0, 0, st) != TRXHIP_OK ||
				    launch_rx(s, d_in, cf32, true, 0, fn, tn, d_ind, d_bits, 1, true, st) != TRXHIP_OK ||
				    hipEventSynchronize(s->ev_corr) != hipSuccess)
					return TRXHIP_EIO;
				pending += *s->h_corr;
				waited = true;
			} else {
				pending += fed_correction(s, feed_at);
			}
		}
		to_skip = TRX_MSS_SLOT - carried;
	}

	// apply sample rate slippage compensation (:398-406); with tracking off nothing moves the cut and the value stays
	if (s->tracking) {
		to_skip -= pending;
		if (to_skip < 0)
			to_skip = 0;
		else
			pending = 0;
	}
	if (to_skip > n)                                               /* the reference: read_n with a negative count */
		return TRXHIP_EINVAL;
	const int64_t left_after_burst = n - to_skip;
	const int64_t full = left_after_burst / TRX_MSS_SLOT, frac = left_after_burst % TRX_MSS_SLOT;
	const int64_t cnt = full + (straddle ? 1 : 0);
	if (cnt > 0x7fffffff || (s->ctx && (uint64_t)cnt > out_slots))
		return TRXHIP_EINVAL;

	uint32_t fn_full, fn0;                                         /* the clocks of the first slot in the chunk and of slot 0 */
	int tn_full, tn0;
	trx_mss_clock_add(fn, tn, 1, &fn_full, &tn_full);
	trx_mss_clock_add(fnb, tnb, 1, &fn0, &tn0);
	const uint64_t sch_full = full ? trx_mss_count_sch(fn_full, tn_full, (uint64_t)full) : 0;
	const uint64_t sch_all = cnt ? trx_mss_count_sch(fn0, tn0, (uint64_t)cnt) : 0;

	if (s->ctx) {
		int rc = TRXHIP_OK;
		const bool edge = straddle && !waited;
		if (edge || frac)
			rc = launch_join(s, d_in, cf32, edge, 0, (size_t)(to_skip + full * TRX_MSS_SLOT), (uint32_t)frac, st);
		const size_t k0 = waited ? 1 : 0;
		const bool sum = s->tracking && sch_full != 0;
		if (rc == TRXHIP_OK && (size_t)cnt > k0) {
			uint32_t fnk;
			int tnk;
			trx_mss_clock_add(fn0, tn0, k0, &fnk, &tnk);
			rc = launch_rx(s, d_in, cf32, edge, to_skip, fnk, tnk, d_ind + k0, d_bits ? d_bits + k0 * 148 : nullptr, (size_t)cnt - k0, sum,
				       st);
		}
		if (rc == TRXHIP_OK && hipEventRecord(s->ev, st) != hipSuccess)
			rc = TRXHIP_EIO;
		if (rc != TRXHIP_OK)
			return TRXHIP_EIO;
		s->ev_used = true;
		if (frac)
			s->rem_half ^= 1;
		if (sum)
			s->unread = true;
	} else if (s->tracking) {
		for (uint64_t i = 0; i < sch_full; i++)
			pending += fed_correction(s, feed_at);
	}

	// the slots in the chunk: inc_and_update_safe(first_ts + to_skip + i * 625), :413-417
	if (full) {
		jumps += jump(first_ts + to_skip - ts);
		trx_mss_clock_add(fn, tn, (uint64_t)full, &fn, &tn);
		ts = first_ts + to_skip + (full - 1) * TRX_MSS_SLOT;
	}
	s->last.fn0 = fn0;
	s->last.tn0 = tn0;
	s->last.n = (size_t)cnt;
	s->last.straddle = straddle;
	s->last.carried = carried;
	s->last.to_skip = to_skip;
	s->last.first_ts = first_ts;
	s->last.tsc = s->tsc;
	s->last.active = s->active;
	s->fn = fn;
	s->tn = tn;
	s->ts = ts;
	s->first_call = false;
	s->carried = (uint32_t)frac;
	s->carried_cf32 = cf32;
	s->pending = pending;
	s->feed_at = feed_at;
	s->to_skip_last = to_skip;
	s->clock_jumps += jumps;
	s->pulls++;
	s->slots += (uint64_t)cnt;
	s->sch_slots += sch_all;
	if (n_slots)
		*n_slots = (size_t)cnt;
	if (n_carried)
		*n_carried = (size_t)frac;
	return TRXHIP_OK;
}

int acquire(trxhip_ms_sched *s, const void *d_buf, int cf32, size_t n_samples, int64_t first_ts, trxhip_sch_sync_result *h_res, void *stream)
{
	if (!s || n_samples < 512 + 20 || n_samples > TRXHIP_SCH_SYNC_MAX_LEN)
		return TRXHIP_EINVAL;
	trxhip_sch_sync_result r;
	if (!s->ctx) {
		if (d_buf || !h_res)
			return TRXHIP_EINVAL;
		r = *h_res;                                            /* plan-only: the receiver's answer comes from outside */
	} else {
		if (!d_buf || (reinterpret_cast<uintptr_t>(d_buf) & (cf32 ? 7 : 3)))
			return TRXHIP_EINVAL;
		const float scale = 1.0f / s->rx_full_scale;           /* 1.f / float(rxFullScale), :168 */
		const int rc = cf32 ? trxhip_sch_sync_batch_cf32(s->ctx, static_cast<const float *>(d_buf), n_samples, s->d_acq, nullptr, 1, n_samples,
								 TRXHIP_SCH_SYNC_ACQ, scale, stream)
				    : trxhip_sch_sync_batch_i16(s->ctx, static_cast<const int16_t *>(d_buf), n_samples, s->d_acq, nullptr, 1, n_samples,
								TRXHIP_SCH_SYNC_ACQ, scale, stream);
		if (rc != TRXHIP_OK)
			return rc;
		const hipStream_t st = static_cast<hipStream_t>(stream);
		if (hipMemcpyAsync(s->h_acq, s->d_acq, sizeof(r), hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipEventRecord(s->ev, st) != hipSuccess || hipEventSynchronize(s->ev) != hipSuccess)
			return TRXHIP_EIO;
		s->ev_used = false;
		r = *s->h_acq;
		if (h_res)
			*h_res = r;
	}
	if (r.rc != 1)
		return 0;
	if (r.fn < 0 || (uint32_t)r.fn >= TRX_MSS_HYPERFRAME)
		return TRXHIP_EINVAL;
	s->fn = (uint32_t)r.fn;                                        /* timekeeper.set(fn, 0): GSM::Time(fn), ts 0 (:91) */
	s->tn = 0;
	s->ts = 0;
	s->tsc = (uint8_t)(r.bsic & 7);                                /* mTSC = sch.bsic & 0x7 (:90) */
	s->first_sch_ts_start = first_ts + r.start - 4 * 4 - 1;        /* :198 */
	s->clock_set = true;
	s->first_call = true;
	s->carried = 0;
	s->pending = 0;
	s->unread = false;
	return 1;
}

}  // namespace

extern "C" {

int trxhip_ms_sched_create(trxhip_ctx *ctx, const trxhip_ms_sched_cfg *cfg, trxhip_ms_sched **out)
{
	if (!cfg || !out || cfg->tsc > 7 || !std::isfinite(cfg->rx_full_scale) || !(cfg->rx_full_scale > 0.0f))
		return TRXHIP_EINVAL;
	if (ctx && with_device(ctx))
		return TRXHIP_EINVAL;
	trxhip_ms_sched *s = new (std::nothrow) trxhip_ms_sched();
	if (!s)
		return TRXHIP_ENOMEM;
	s->rx_full_scale = cfg->rx_full_scale;
	s->tsc = cfg->tsc;
	s->active = cfg->active_tns;
	s->tracking = cfg->tracking != 0;
	if (!ctx) {
		*out = s;
		return TRXHIP_OK;
	}
	s->ctx = ctx;
	const size_t rem_bytes = 2 * TRX_MSS_REM_STRIDE * 8;
	bool ok = hipMalloc(&s->d_rem, rem_bytes) == hipSuccess && hipMalloc(&s->d_edge_row, TRX_MSS_SLOT * 8) == hipSuccess &&
		  hipMalloc((void **)&s->d_corr, sizeof(int32_t)) == hipSuccess && hipMalloc((void **)&s->d_acq, sizeof(*s->d_acq)) == hipSuccess &&
		  hipHostMalloc((void **)&s->h_corr, sizeof(int32_t), hipHostMallocDefault) == hipSuccess &&
		  hipHostMalloc((void **)&s->h_acq, sizeof(*s->h_acq), hipHostMallocDefault) == hipSuccess &&
		  hipEventCreateWithFlags(&s->ev_corr, hipEventDisableTiming) == hipSuccess &&
		  hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) == hipSuccess;
	ok = ok && hipMemset(s->d_rem, 0, rem_bytes) == hipSuccess && hipMemset(s->d_corr, 0, sizeof(int32_t)) == hipSuccess &&
	     hipStreamSynchronize(nullptr) == hipSuccess;      /* the first pull may come on a stream that does not wait for the null stream */
	if (!ok) {
		trxhip_ms_sched_destroy(s);
		return TRXHIP_ENOMEM;
	}
	*s->h_corr = 0;
	*out = s;
	return TRXHIP_OK;
}

void trxhip_ms_sched_destroy(trxhip_ms_sched *s)
{
	if (!s)
		return;
	if (s->ctx && with_device(s->ctx) == 0) {
		if (s->unread && s->ev_corr)
			(void)hipEventSynchronize(s->ev_corr);
		if (s->ev_used && s->ev)
			(void)hipEventSynchronize(s->ev);
		if (s->ev_corr) (void)hipEventDestroy(s->ev_corr);
		if (s->ev) (void)hipEventDestroy(s->ev);
		void *bufs[] = { s->d_rem, s->d_edge_row, s->d_corr, s->d_acq };
		for (void *p : bufs)
			if (p) (void)hipFree(p);
		if (s->h_corr) (void)hipHostFree(s->h_corr);
		if (s->h_acq) (void)hipHostFree(s->h_acq);
	}
	delete s;
}

int trxhip_ms_sched_set_clock(trxhip_ms_sched *s, uint32_t fn, int tn, int64_t ts)
{
	if (!s || fn >= TRX_MSS_HYPERFRAME || tn < 0 || tn > 7)
		return TRXHIP_EINVAL;
	s->fn = fn;
	s->tn = tn;
	s->ts = ts;
	s->clock_set = true;
	s->first_call = false;
	s->carried = 0;
	s->pending = 0;
	s->unread = false;
	return TRXHIP_OK;
}

int trxhip_ms_sched_clock(const trxhip_ms_sched *s, uint32_t *fn, int *tn, int64_t *ts)
{
	if (!s || !fn || !tn || !ts || !s->clock_set)
		return TRXHIP_EINVAL;
	*fn = s->fn;
	*tn = s->tn;
	*ts = s->ts;
	return TRXHIP_OK;
}

int trxhip_ms_sched_set_tsc(trxhip_ms_sched *s, int tsc)
{
	if (!s || tsc < 0 || tsc > 7)
		return TRXHIP_EINVAL;
	s->tsc = (uint8_t)tsc;
	return TRXHIP_OK;
}

int trxhip_ms_sched_set_active(trxhip_ms_sched *s, uint8_t tn_mask)
{
	if (!s)
		return TRXHIP_EINVAL;
	s->active = tn_mask;
	return TRXHIP_OK;
}

int trxhip_ms_sched_set_tracking(trxhip_ms_sched *s, int on)
{
	if (!s)
		return TRXHIP_EINVAL;
	s->tracking = on != 0;
	return TRXHIP_OK;
}

int trxhip_ms_sched_feed_starts(trxhip_ms_sched *s, const int32_t *starts, size_t n)
{
	if (!s || s->ctx || (!starts && n))
		return TRXHIP_EINVAL;
	s->feed.assign(starts, starts + n);                            /* replaces what is still queued */
	s->feed_at = 0;
	return TRXHIP_OK;
}

int trxhip_ms_sched_acquire_s16(trxhip_ms_sched *s, const int16_t *d_buf, size_t n_samples, int64_t first_ts, trxhip_sch_sync_result *h_res,
				void *stream)
{
	return acquire(s, d_buf, 0, n_samples, first_ts, h_res, stream);
}

int trxhip_ms_sched_acquire_cf32(trxhip_ms_sched *s, const float *d_buf, size_t n_samples, int64_t first_ts, trxhip_sch_sync_result *h_res,
				 void *stream)
{
	return acquire(s, d_buf, 1, n_samples, first_ts, h_res, stream);
}

int64_t trxhip_ms_sched_slots(const trxhip_ms_sched *s, size_t n_samples)
{
	if (!s || n_samples > kMaxSamples)
		return TRXHIP_EINVAL;
	const uint32_t carried = s->first_call ? 0u : s->carried;
	const int64_t bound = (int64_t)((carried + n_samples) / TRX_MSS_SLOT) + 1;
	if (s->first_call)
		return bound;
	const bool straddle = carried && n_samples >= TRX_MSS_SLOT - carried;
	if (s->tracking) {
		uint32_t fn;
		int tn;
		trx_mss_clock_add(s->fn, s->tn, 1, &fn, &tn);
		if (s->unread || s->pending || (straddle && trx_mss_is_sch(fn, tn)))
			return bound;
	}
	if (!carried)
		return (int64_t)(n_samples / TRX_MSS_SLOT);
	return straddle ? 1 + (int64_t)((n_samples - (TRX_MSS_SLOT - carried)) / TRX_MSS_SLOT) : 0;
}

int trxhip_ms_sched_pull_s16(trxhip_ms_sched *s, const int16_t *d_in, size_t n_samples, int64_t first_ts, trxhip_ms_burst_ind *d_ind,
			     int8_t *d_bits, size_t out_slots, size_t *n_slots, size_t *n_carried, void *stream)
{
	return pull(s, d_in, 0, n_samples, first_ts, d_ind, d_bits, out_slots, n_slots, n_carried, stream);
}

int trxhip_ms_sched_pull_cf32(trxhip_ms_sched *s, const float *d_in, size_t n_samples, int64_t first_ts, trxhip_ms_burst_ind *d_ind,
			      int8_t *d_bits, size_t out_slots, size_t *n_slots, size_t *n_carried, void *stream)
{
	return pull(s, d_in, 1, n_samples, first_ts, d_ind, d_bits, out_slots, n_slots, n_carried, stream);
}

int trxhip_ms_sched_plan(const trxhip_ms_sched *s, trxhip_ms_plan *h_out, size_t n)
{
	if (!s || (!h_out && n) || n > s->last.n)
		return TRXHIP_EINVAL;
	for (size_t k = 0; k < n; k++) {
		trxhip_ms_plan p;
		memset(&p, 0, sizeof(p));
		int tn;
		trx_mss_clock_add(s->last.fn0, s->last.tn0, k, &p.fn, &tn);
		p.tn = (uint8_t)tn;
		p.kind = (uint8_t)trx_mss_kind(p.fn, tn, s->last.tsc);
		p.flags = (uint8_t)(((s->last.active >> tn) & 1u) ? TRXHIP_MS_SLOT_ACTIVE : 0);
		p.ts = (s->last.straddle && k == 0) ? s->last.first_ts - s->last.carried
						     : s->last.first_ts + s->last.to_skip + (int64_t)(k - (s->last.straddle ? 1 : 0)) * TRX_MSS_SLOT;
		p.src_off = (int32_t)(p.ts - s->last.first_ts);
		h_out[k] = p;
	}
	return TRXHIP_OK;
}

int trxhip_ms_sched_state(trxhip_ms_sched *s, trxhip_ms_sched_status *out)
{
	if (!s || !out)
		return TRXHIP_EINVAL;
	if (s->ctx && fold_correction(s) != TRXHIP_OK)
		return TRXHIP_EIO;
	memset(out, 0, sizeof(*out));
	out->to_skip = s->to_skip_last;
	out->pending = s->pending;
	out->first_sch_ts_start = s->first_sch_ts_start;
	out->carried = s->carried;
	out->carried_cf32 = (uint8_t)s->carried_cf32;
	out->first_call = s->first_call;
	out->tracking = s->tracking;
	out->tsc = s->tsc;
	out->active_tns = s->active;
	out->clock_set = s->clock_set;
	out->clock_jumps = s->clock_jumps;
	out->pulls = s->pulls;
	out->slots = s->slots;
	out->sch_slots = s->sch_slots;
	return TRXHIP_OK;
}

}  // extern "C"
