// trx_ms_sched.hip -- the MS-side downlink slot scheduler: the radio's sample stream in, burst indications out.
//
// The counterpart of trx_rx_sched.hip on the MS side.  It restates what the reference does between the radio's receive buffers
// and upper_trx::pullRadioVector():
//   ms_trx::search_for_sch() / handle_sch(true)   ms/ms_rx_lower.cpp:310-352, :157-205   first acquisition (trxhip_ms_sched_acquire_*)
//   ms_trx::grab_bursts()                         ms/ms_rx_lower.cpp:354-422             the cutter (trxhip_ms_sched_pull_*)
//   ms_trx::handle_sch_or_nb() / handle_sch(false) :130-153, :157-205                    what a cut slot is, temp_ts_corr_offset
//   time_keeper                                   ms/ms.h:160-221                        the GSM clock and its timestamp
// There is one object, the group of streams (trxhip_ms_group_*); the single object (trxhip_ms_sched_*) is a group of one member
// whose entry points forward to the group's.  A pull is: per member the plan on the host (plan_begin / plan_finish: cut position,
// clock, count -- integers only, nothing moves), the issue of one launch set for all members, and commit(), which moves the
// members' states.  A launch set is a join (the slot that straddles the carried partial slot and the chunk is assembled into a
// row; the chunk's tail is saved as the new partial slot), a clear of the correction words, the receiver (trx_ms_rx.hip) over
// every slot of the pull, read where it lies, a copy of the correction words to a pinned mailbox, and one event.  The cut
// position depends on SCH results of the device in two places, which are the scheduler's only waits (see include/trxhip.h): per
// SCH-carrying launch set the correction is summed on the device into a word per member that starts at zero; the host adds it to
// temp_ts_corr_offset when the next pull plans.
// issue_table() says once what a member's plan puts into a launch set, as entries (trx_ms_sched.h), and sends them one of two
// ways.  A group copies them up as one table from a pinned area and launches ms_join_group_kernel and the receiver's group form
// over it.  The single object (`direct`) has at most one entry of each kind and passes them as kernel arguments, to
// ms_join_kernel and the receiver's stream form: no table, no pinned area, none of a table's waits.
// With ctx == NULL the object is plan-only: cutter, clock and plan, no device memory; SCH starts come from a queue.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_afc.h"
#include "trx_ms_agc.h"
#include "trx_ms_nco.h"
#include "trx_ms_sched.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kMaxSamples = (size_t)1 << 40;
constexpr int kTabSlots = 4;                   /* pinned table areas of a group: the host runs at most this many launch sets ahead */
constexpr size_t kTabEntries = 5;              /* table entries per member: receiver, join, gain control, AFC; the fifth holds the NCO's 16 bytes */

// ------------------------------------------------------------------------------------------------
// The join of one member, one block, from its entry (trx_mss_join).  The stream of a pull is the carried partial slot (rem_in,
// `carried` samples) followed by the chunk.
//   do_edge : its first 625 samples, the one slot that does not lie in the chunk, are assembled into edge_row (:385-394)
//   the new partial slot (:419-421) goes to the OTHER half of the partial-slot area: the first `keep` samples of the old one
//   (a chunk shorter than the missing part: :388-391) and n_tail samples of the chunk from tail_at on
// T: one IQ sample (uint32_t: int16 pair; float2).  carried + (625 - carried) <= 625, keep + n_tail < 625.
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void ms_join(const T *__restrict__ in, const T *__restrict__ rem_in, T *__restrict__ rem_out, T *__restrict__ edge_row,
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

template <typename T>
__device__ __forceinline__ void ms_join(const trx_mss_join &j)
{
	ms_join<T>(static_cast<const T *>(j.in), static_cast<const T *>(j.rem_in), static_cast<T *>(j.rem_out), static_cast<T *>(j.edge_row),
		   j.carried, j.do_edge, j.keep, (size_t)j.tail_at, j.n_tail);
}

// ms_join_kernel: the single object's join, its entry a kernel argument
template <typename T>
__global__ void __launch_bounds__(kThreads)
ms_join_kernel(const trx_mss_join j)
{
	ms_join<T>(j);
}

// ms_join_group_kernel: one block per member of a group pull that needs a join, its entry from the table
template <typename T>
__global__ void __launch_bounds__(kThreads)
ms_join_group_kernel(const trx_mss_join *__restrict__ tab)
{
	const trx_mss_join j = tab[blockIdx.x];
	ms_join<T>(j);
}

static_assert(sizeof(trx_mss_join) == 64 && sizeof(trx_mss_member) == 64 && sizeof(trx_agc_entry) == 64 && sizeof(trx_afc_job) == 64,
	      "table entries");
static_assert(sizeof(trxhip_ms_agc_record) == 32 && sizeof(trxhip_ms_agc_status) == 304 && sizeof(trxhip_ms_agc_cfg) == 16, "public AGC structs");

// One downlink stream on the host: what a group holds per member
struct ms_member {
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
	bool unread = false;                   /* a launch with SCH slots was issued: its sum arrives in the mailbox behind the set's event */
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
	int rem_half = 0;                      /* device: the half of the partial-slot area the next pull reads */
	// gain control (trx_ms_agc.h).  agc: the state of a plan-only member; of a device member its gain_check alone, which only
	// counts slots -- the rest lives on the device
	bool agc_on = false;
	float *d_level = nullptr;
	trx_agc_state agc = {};
	std::vector<float> lv_feed;            /* plan-only: the levels fed from outside */
	size_t lv_at = 0;
	// FCCH frequency-offset measurement (trx_ms_afc.h): the count of FCCH slots measured -- the rest of the state is on the device
	bool afc_on = false;
	trxhip_ms_fcch *d_fcch = nullptr;
	uint64_t afc_count = 0;
	// the NCO (trx_ms_nco.h): all of it is here -- a pull takes it by value
	trx_nco_state nco = {};
};

// The plan of one member's pull.  plan_begin() fills the first part, plan_finish() the second; neither moves the member.
struct ms_plan {
	int cf32 = 0;
	size_t n_samples = 0;
	int64_t first_ts = 0;
	bool extend = false;                   /* the chunk only extends the partial slot (:385-391): nothing else is planned */
	bool straddle = false;
	bool prelim = false;                   /* the straddling slot is an SCH slot the cutter follows: it is demodulated first */
	uint32_t carried = 0;
	uint32_t fn = 0, fnb = 0;              /* (fn, tn): the clock behind the first call's steps and the straddling slot; */
	int tn = 0, tnb = 0;                   /* (fnb, tnb): in front of the straddling slot */
	int64_t ts = 0, to_skip = 0;
	uint64_t jumps = 0;
	// plan_finish()
	bool waited = false;                   /* the straddling slot's indication is written already */
	int64_t pending = 0, full = 0, frac = 0, cnt = 0;
	uint32_t fn0 = 0;                      /* the clock of slot 0 */
	int tn0 = 0;
	uint64_t sch_full = 0, sch_all = 0;
	size_t feed_at = 0;
};

}  // namespace

// A trxhip_ms_sched * is the handle of a group of one member that issues directly (trxhip_ms_sched_create()); the type has no
// definition of its own.
struct trxhip_ms_group {
	trxhip_ctx *ctx = nullptr;
	float rx_full_scale = 0.0f;
	bool direct = false;                   /* the single object: one member, its entries sent as kernel arguments, no table */
	std::vector<ms_member> m;
	std::vector<ms_plan> plan;             /* scratch of a pull */
	std::vector<int> rc;
	// device state (ctx != NULL)
	trx_dev<char> d_rem;                   /* [n][2][TRX_MSS_REM_STRIDE] samples of either format */
	trx_dev<char> d_edge;                  /* [n][625] samples of either format */
	trx_dev<int32_t> d_corr;               /* [n] correction words and their pinned mailbox */
	trx_pin<int32_t> h_corr;
	trx_dev<trxhip_sch_sync_result> d_acq; /* [n] */
	trx_pin<trxhip_sch_sync_result> h_acq;
	// A launch set records ONE event behind everything it issues, the next of kTabSlots taken in turn: where the set sums
	// corrections the event says that the mailbox holds them.
	// The table of a launch set (not with `direct`): up to n receiver entries followed by up to n join entries, then those of gain
	// control and of AFC where members have them on, 64 bytes each.  It is staged in the pinned area that belongs to the set's
	// event: the area is written again only behind that event
	trx_dev<char> d_tab;
	trx_pin<char> h_tab;
	int tab_at = 0;                        /* the event, and the area, the next launch set takes */
	int corr_at = 0;                       /* those of the last launch set that summed corrections */
	// gain control: the members' states, the levels and piece results of the pull in flight (it grows), the event behind the
	// AGC launches of the last pull that had any
	trx_dev<trx_agc_state> d_agc;
	trx_dev<float> d_work;
	// AFC: the members' states, the event behind the AFC launch of the last pull that had one
	trx_dev<trx_afc_state> d_afc;
	size_t afc_members = 0;                /* members with AFC on: while there is none a pull does not look at its slots' kinds */
	// the NCO in front of acquire: the rows' records and their pinned staging ([n] each), the complex64 work buffer (it grows)
	trx_dev<trxhip_ms_nco_row> d_nco_rec;
	trx_pin<trxhip_ms_nco_row> h_nco_rec;
	trx_dev<float> d_nco_work;
	// acquire_afc: the search's hit and measurement per listed buffer and their pinned copies ([n] each)
	trx_dev<trxhip_ms_fcch_hit> d_fs_hit;
	trx_pin<trxhip_ms_fcch_hit> h_fs_hit;
	trx_dev<trxhip_ms_fcch> d_fs_fcch;
	trx_pin<trxhip_ms_fcch> h_fs_fcch;
	// the events stand last: what is in flight is waited for before a buffer above is freed
	trx_event ev_tab[kTabSlots];           /* the launch sets' */
	trx_event ev;                          /* acquire's */
	trx_event ev_agc, ev_afc;
};

namespace {

int launched() { return hipGetLastError() == hipSuccess ? TRXHIP_OK : TRXHIP_EIO; }

// the sums of a launch set in flight join temp_ts_corr_offset: the wait of the pull behind a pull that cut an SCH slot -- one wait,
// and every member's word
int fold_correction(trxhip_ms_group *g)
{
	bool any = false;
	for (const ms_member &m : g->m)
		any = any || m.unread;
	if (!any)
		return TRXHIP_OK;
	if (with_device(g->ctx) || g->ev_tab[g->corr_at].wait() != TRXHIP_OK)
		return TRXHIP_EIO;
	for (size_t i = 0; i < g->m.size(); i++)
		if (g->m[i].unread) {
			g->m[i].pending += g->h_corr[i];
			g->m[i].unread = false;
		}
	return TRXHIP_OK;
}

// inc_and_update_safe()'s asserts (ms.h:192-194): diff < 1.5 * 625 and diff > 0.5 * 625
bool jump(int64_t diff) { return !(2 * diff < 3 * TRX_MSS_SLOT) || !(2 * diff > TRX_MSS_SLOT); }

// plan-only: the next fed start as handle_sch(false) would add it (:199-203)
int64_t fed_correction(const ms_member &m, size_t &at)
{
	if (at >= m.feed.size())
		return 0;
	const int32_t start = m.feed[at++];
	if (start == TRXHIP_MS_SCHED_NO_SCH || (start <= 1 && start >= -1))
		return 0;
	return -(int64_t)start;
}

// ------------------------------------------------------------------------------------------------
// The plan of one member's pull, in two steps around the second of the two waits.
// plan_begin: what the single object refuses before it launches anything; the chunk that only extends the partial slot; the
//   first call after an acquire (:362-383); the straddling slot's clock (:385-396), and whether that slot has to be demodulated
//   before the rest can be planned.  device: the object has buffers (else it takes none); bounded: out_slots limits the count
// ------------------------------------------------------------------------------------------------
int plan_begin(const ms_member &m, bool device, bool bounded, int cf32, size_t n_samples, int64_t first_ts, const void *d_in, const void *d_ind,
	       const void *d_bits, size_t out_slots, ms_plan &p)
{
	if (!m.clock_set || n_samples == 0 || n_samples > kMaxSamples)
		return TRXHIP_EINVAL;
	if (m.carried && cf32 != m.carried_cf32)
		return TRXHIP_EINVAL;
	if (device) {
		if (!d_in || (reinterpret_cast<uintptr_t>(d_in) & (cf32 ? 7 : 3)) || !d_ind || (reinterpret_cast<uintptr_t>(d_ind) & 3))
			return TRXHIP_EINVAL;
	} else if (d_in || d_ind || d_bits) {
		return TRXHIP_EINVAL;                                  /* a plan-only object takes no buffers */
	}
	p = ms_plan();
	p.cf32 = cf32;
	p.n_samples = n_samples;
	p.first_ts = first_ts;
	p.fn = m.fn;
	p.tn = m.tn;
	p.ts = m.ts;
	// partial burst samples read from the last buffer: a chunk shorter than the missing part only extends them (:385-391)
	if (!m.first_call && m.carried && n_samples < TRX_MSS_SLOT - m.carried) {
		p.extend = true;
		return TRXHIP_OK;
	}
	// round up to next burst by calculating the time between sch detection and now (:362-383)
	if (m.first_call) {
		const int64_t next_burst_start = first_ts - m.first_sch_ts_start;
		const int64_t fullts = next_burst_start / TRX_MSS_SLOT, fracts = next_burst_start % TRX_MSS_SLOT;
		p.to_skip = TRX_MSS_SLOT - fracts;
		/* fullts inc_and_update() (none when fullts <= 0), inc_both() when fracts, dec_by_one(): TNs on the clock; the final
		 * set() keeps the clock and overwrites every timestamp the steps left */
		int64_t steps = (fullts > 0 ? fullts : 0) + (fracts ? 1 : 0) - 1;
		const int64_t period = (int64_t)TRX_MSS_HYPERFRAME * 8;
		steps = ((steps % period) + period) % period;
		trx_mss_clock_add(p.fn, p.tn, (uint64_t)steps, &p.fn, &p.tn);
		p.ts = first_ts - TRX_MSS_SLOT + p.to_skip;
	}
	p.carried = m.first_call ? 0u : m.carried;                     /* (an acquire drops the partial slot) */
	p.straddle = p.carried != 0;
	p.fnb = p.fn;                                                  /* slot k of the pull: k + 1 incTN() behind (fnb, tnb) */
	p.tnb = p.tn;
	if (p.straddle) {
		if (bounded && out_slots < 1)
			return TRXHIP_EINVAL;
		p.jumps += jump(first_ts - p.carried - p.ts);              /* inc_and_update_safe(first_ts - partial_rdofs), :393 */
		trx_mss_clock_add(p.fn, p.tn, 1, &p.fn, &p.tn);
		p.ts = first_ts - p.carried;
		// handle_sch_or_nb() on the completed slot comes before the correction is applied (:394, :399): where it is an SCH slot
		// the cutter follows, this slot alone is demodulated first -- the second of the two waits
		p.prelim = m.tracking && trx_mss_is_sch(p.fn, p.tn);
		p.to_skip = TRX_MSS_SLOT - p.carried;
	}
	return TRXHIP_OK;
}

// plan_finish: the correction (:398-406), the slots in the chunk (:408-421), the counts, the clocks.  The member's correction in
// flight has been folded.  prelim_corr: what the straddling SCH slot summed (device objects with p.prelim); a plan-only object
// takes it, and those of the slots in the chunk, from its queue
int plan_finish(const ms_member &m, bool device, bool bounded, size_t out_slots, int64_t prelim_corr, ms_plan &p)
{
	const int64_t n = (int64_t)p.n_samples;
	int64_t pending = m.pending;
	size_t feed_at = m.feed_at;
	if (p.prelim) {
		if (device) {
			pending += prelim_corr;
			p.waited = true;
		} else {
			pending += fed_correction(m, feed_at);
		}
	}
	// apply sample rate slippage compensation (:398-406); with tracking off nothing moves the cut and the value stays
	int64_t to_skip = p.to_skip;
	if (m.tracking) {
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
	const int64_t cnt = full + (p.straddle ? 1 : 0);
	if (cnt > 0x7fffffff || (bounded && (uint64_t)cnt > out_slots))
		return TRXHIP_EINVAL;

	uint32_t fn_full;                                              /* the clock of the first slot in the chunk */
	int tn_full;
	trx_mss_clock_add(p.fn, p.tn, 1, &fn_full, &tn_full);
	trx_mss_clock_add(p.fnb, p.tnb, 1, &p.fn0, &p.tn0);
	p.sch_full = full ? trx_mss_count_sch(fn_full, tn_full, (uint64_t)full) : 0;
	p.sch_all = cnt ? trx_mss_count_sch(p.fn0, p.tn0, (uint64_t)cnt) : 0;
	if (!device && m.tracking)
		for (uint64_t i = 0; i < p.sch_full; i++)
			pending += fed_correction(m, feed_at);

	// the slots in the chunk: inc_and_update_safe(first_ts + to_skip + i * 625), :413-417
	if (full) {
		p.jumps += jump(p.first_ts + to_skip - p.ts);
		trx_mss_clock_add(p.fn, p.tn, (uint64_t)full, &p.fn, &p.tn);
		p.ts = p.first_ts + to_skip + (full - 1) * TRX_MSS_SLOT;
	}
	p.to_skip = to_skip;
	p.pending = pending;
	p.full = full;
	p.frac = frac;
	p.cnt = cnt;
	p.feed_at = feed_at;
	return TRXHIP_OK;
}

// the issued pull becomes the member's state
void commit(ms_member &m, const ms_plan &p)
{
	if (p.extend) {
		m.carried += (uint32_t)p.n_samples;
		m.carried_cf32 = p.cf32;
		m.last.n = 0;
		m.pulls++;
		return;
	}
	m.last.fn0 = p.fn0;
	m.last.tn0 = p.tn0;
	m.last.n = (size_t)p.cnt;
	m.last.straddle = p.straddle;
	m.last.carried = p.carried;
	m.last.to_skip = p.to_skip;
	m.last.first_ts = p.first_ts;
	m.last.tsc = m.tsc;
	m.last.active = m.active;
	m.fn = p.fn;
	m.tn = p.tn;
	m.ts = p.ts;
	m.first_call = false;
	m.carried = (uint32_t)p.frac;
	m.carried_cf32 = p.cf32;
	m.pending = p.pending;
	m.feed_at = p.feed_at;
	m.to_skip_last = p.to_skip;
	m.clock_jumps += p.jumps;
	m.pulls++;
	m.slots += (uint64_t)p.cnt;
	m.sch_slots += p.sch_all;
}

// what a found SCH burst sets (handle_sch(true), decode_sch(bits, true))
void acquired(ms_member &m, const trxhip_sch_sync_result &r, int64_t first_ts)
{
	m.fn = (uint32_t)r.fn;                                         /* timekeeper.set(fn, 0): GSM::Time(fn), ts 0 (:91) */
	m.tn = 0;
	m.ts = 0;
	m.tsc = (uint8_t)(r.bsic & 7);                                 /* mTSC = sch.bsic & 0x7 (:90) */
	m.first_sch_ts_start = first_ts + r.start - 4 * 4 - 1;         /* :198 */
	m.clock_set = true;
	m.first_call = true;
	m.carried = 0;
	m.pending = 0;
	m.unread = false;
}

void set_clock(ms_member &m, uint32_t fn, int tn, int64_t ts)
{
	m.fn = fn;
	m.tn = tn;
	m.ts = ts;
	m.clock_set = true;
	m.first_call = false;
	m.carried = 0;
	m.pending = 0;
	m.unread = false;
}

int64_t slots_of(const ms_member &m, size_t n_samples)
{
	if (n_samples > kMaxSamples)
		return TRXHIP_EINVAL;
	const uint32_t carried = m.first_call ? 0u : m.carried;
	const int64_t bound = (int64_t)((carried + n_samples) / TRX_MSS_SLOT) + 1;
	if (m.first_call)
		return bound;
	const bool straddle = carried && n_samples >= TRX_MSS_SLOT - carried;
	if (m.tracking) {
		uint32_t fn;
		int tn;
		trx_mss_clock_add(m.fn, m.tn, 1, &fn, &tn);
		if (m.unread || m.pending || (straddle && trx_mss_is_sch(fn, tn)))
			return bound;
	}
	if (!carried)
		return (int64_t)(n_samples / TRX_MSS_SLOT);
	return straddle ? 1 + (int64_t)((n_samples - (TRX_MSS_SLOT - carried)) / TRX_MSS_SLOT) : 0;
}

int plan_of(const ms_member &m, trxhip_ms_plan *h_out, size_t n)
{
	if ((!h_out && n) || n > m.last.n)
		return TRXHIP_EINVAL;
	for (size_t k = 0; k < n; k++) {
		trxhip_ms_plan p;
		memset(&p, 0, sizeof(p));
		int tn;
		trx_mss_clock_add(m.last.fn0, m.last.tn0, k, &p.fn, &tn);
		p.tn = (uint8_t)tn;
		p.kind = (uint8_t)trx_mss_kind(p.fn, tn, m.last.tsc);
		p.flags = (uint8_t)(((m.last.active >> tn) & 1u) ? TRXHIP_MS_SLOT_ACTIVE : 0);
		p.ts = (m.last.straddle && k == 0) ? m.last.first_ts - m.last.carried
						   : m.last.first_ts + m.last.to_skip + (int64_t)(k - (m.last.straddle ? 1 : 0)) * TRX_MSS_SLOT;
		p.src_off = (int32_t)(p.ts - m.last.first_ts);
		h_out[k] = p;
	}
	return TRXHIP_OK;
}

void state_of(const ms_member &m, trxhip_ms_sched_status *out)
{
	memset(out, 0, sizeof(*out));
	out->to_skip = m.to_skip_last;
	out->pending = m.pending;
	out->first_sch_ts_start = m.first_sch_ts_start;
	out->carried = m.carried;
	out->carried_cf32 = (uint8_t)m.carried_cf32;
	out->first_call = m.first_call;
	out->tracking = m.tracking;
	out->tsc = m.tsc;
	out->active_tns = m.active;
	out->clock_set = m.clock_set;
	out->clock_jumps = m.clock_jumps;
	out->pulls = m.pulls;
	out->slots = m.slots;
	out->sch_slots = m.sch_slots;
}

bool cfg_ok(const trxhip_ms_sched_cfg *cfg) { return cfg->tsc <= 7 && std::isfinite(cfg->rx_full_scale) && cfg->rx_full_scale > 0.0f; }

// ------------------------------------------------------------------------------------------------
// The group: the pulls of its members issued as one.
// ------------------------------------------------------------------------------------------------

// a pinned area for the next table; it is free once the launch set that read it kTabSlots sets ago is through
char *stage_table(trxhip_ms_group *g)
{
	const int h = g->tab_at;
	if (g->ev_tab[h].wait() != TRXHIP_OK)
		return nullptr;
	return g->h_tab + (size_t)h * kTabEntries * g->m.size() * 64;
}

// What a member with gain control on adds to the pull's own launch set: an entry, a wave per slot, its pieces, and room for its
// levels and piece results.  Every slot the pull cuts counts, slot 0 too where the pull has waited for it (its row is assembled)
struct agc_work {
	size_t n_slots, n_pieces, floats;
};

agc_work agc_work_of(const ms_member &m, const ms_plan &p)
{
	agc_work w = { 0, 0, 0 };
	if (!m.agc_on || p.extend || p.cnt == 0)
		return w;
	w.n_slots = (size_t)p.cnt;
	w.n_pieces = trx_agc_pieces(m.agc.gain_check, (uint64_t)p.cnt);
	w.floats = w.n_slots + 2 * w.n_pieces;
	return w;
}

// The FCCH slots a member with AFC on measures in its pull: those among every slot the pull cuts, ACTIVE or not, slot 0 too
size_t afc_work_of(const ms_member &m, const ms_plan &p)
{
	if (!m.afc_on || p.extend || p.cnt == 0)
		return 0;
	return (size_t)trx_afc_count(p.fn0, p.tn0, (uint64_t)p.cnt);
}

char *rem_of(trxhip_ms_group *g, size_t i, int half, int cf32)
{
	return g->d_rem + (i * 2 * TRX_MSS_REM_STRIDE) * 8 + (size_t)half * TRX_MSS_REM_STRIDE * (cf32 ? 8 : 4);
}

// What of its plan a member puts into a launch set.  prelim: the set of the second wait -- the straddling SCH slot alone, assembled
// into its row and demodulated, its correction summed.  Else the pull's own set: a join where the partial slot is extended, a new
// one is saved, or the straddling slot's row is still to assemble (edge), and the slots from k0 on -- slot 0 is through where
// the pull has waited for it; sum: SCH slots whose starts the cutter follows are among them
struct ms_work {
	bool join, edge, sum;
	size_t k0, n_slots;
};

ms_work work_of(const ms_member &m, const ms_plan &p, bool prelim)
{
	ms_work w;
	w.edge = prelim || (!p.extend && p.straddle && !p.waited);
	w.join = w.edge || p.extend || p.frac != 0;            /* (before plan_finish() p.frac is 0) */
	w.k0 = (!prelim && p.waited) ? 1 : 0;
	w.n_slots = prelim ? 1 : p.extend ? 0 : (size_t)p.cnt - w.k0;
	w.sum = prelim || (m.tracking && p.sch_full != 0);
	return w;
}

// One launch set of a pull, and the only place that knows what its entries hold and how they reach the device.  The set is the
// prelim work of the members whose plan says prelim, or the pull's own work of every member with a chunk; the caller has counted
// its n_rx receiver entries, n_join join entries and n_waves waves.
// A group stages the entries as one table in the next pinned area, receiver entries first, and issues: one copy of the table, one
// join launch over its join entries, one clear of the correction words where a member sums, one receiver launch over its receiver
// entries, the copy of the correction words to the mailbox, one event behind all of it.
// The single object (direct) issues the same sequence without the table: its one join entry and its one receiver entry are the
// arguments of ms_join_kernel and of the receiver's stream form.
// Gain control (n_agc members of the pull's own set have it on and cut a slot; none in a prelim set): their entries
// (trx_ms_agc.h) ride in the same table behind the join entries, or are the single object's kernel argument, and BEHIND the
// set's event -- so that nothing that waits for a correction waits for them -- come the three AGC launches and their own event.
// AFC (n_afc members of the pull's own set have it on and cut an FCCH slot) does the same with its jobs (trx_ms_afc.h), behind
// the AGC entries: one launch and its own event at the very end.
int issue_table(trxhip_ms_group *g, const trxhip_ms_group_chunk *h_chunks, int cf32, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
		size_t out_stride, bool prelim, size_t n_rx, size_t n_join, size_t n_waves, size_t n_agc, size_t n_afc, hipStream_t st)
{
	trx_mss_member own_rx;
	trx_mss_join own_join;
	trx_agc_entry own_agc;
	trx_mss_member *rx = &own_rx;
	trx_mss_join *jn = &own_join;
	trx_agc_entry *ag = &own_agc;
	trx_afc_job own_afc;
	trx_afc_job *af = &own_afc;
	trx_nco_slot own_nco;
	trx_nco_slot *nc = &own_nco;                           /* the receiver entries' oscillators, beside them: nc[k] with rx[k] */
	const size_t n_ent = n_rx + n_join + n_agc + n_afc;
	if (!g->direct) {
		char *tab = stage_table(g);
		if (!tab)
			return TRXHIP_EIO;
		rx = reinterpret_cast<trx_mss_member *>(tab);
		jn = reinterpret_cast<trx_mss_join *>(tab + n_rx * 64);
		ag = reinterpret_cast<trx_agc_entry *>(tab + (n_rx + n_join) * 64);
		af = reinterpret_cast<trx_afc_job *>(tab + (n_rx + n_join + n_agc) * 64);
		nc = reinterpret_cast<trx_nco_slot *>(tab + n_ent * 64);
	}
	if (n_ent == 0)
		return TRXHIP_OK;                                      /* (no slot and no join: no sum either) */

	size_t kr = 0, kj = 0, wave = 0, ka = 0, agc_waves = 0, agc_pieces = 0, agc_floats = 0, kf = 0, afc_waves = 0;
	bool sum = false, rot = false;                         /* rot: a member with receiver work has the NCO on */
	for (size_t i = 0; i < g->m.size(); i++) {
		const ms_plan &p = g->plan[i];
		if (!h_chunks[i].n_samples || g->rc[i] != TRXHIP_OK || (prelim && !p.prelim))
			continue;
		const ms_member &m = g->m[i];
		const ms_work w = work_of(m, p, prelim);
		char *edge_row = g->d_edge + i * TRX_MSS_SLOT * 8;
		if (w.join) {
			trx_mss_join &j = jn[kj++];
			memset(&j, 0, sizeof(j));
			j.in = h_chunks[i].d_in;
			j.rem_in = rem_of(g, i, m.rem_half, cf32);
			j.rem_out = rem_of(g, i, m.rem_half ^ 1, cf32);
			j.edge_row = edge_row;
			j.carried = m.carried;
			j.do_edge = w.edge;
			if (p.extend) {
				j.keep = m.carried;
				j.n_tail = (uint32_t)p.n_samples;
			} else if (!prelim) {
				j.tail_at = (uint64_t)(p.to_skip + p.full * TRX_MSS_SLOT);
				j.n_tail = (uint32_t)p.frac;
			}
		}
		const agc_work a = prelim ? agc_work{ 0, 0, 0 } : agc_work_of(m, p);
		if (a.n_slots) {
			trx_agc_entry &e = ag[ka++];
			memset(&e, 0, sizeof(e));
			e.chunk = h_chunks[i].d_in;
			e.edge_row = p.straddle ? edge_row : nullptr;          /* assembled by this set's join, or by the prelim set's */
			e.first = p.to_skip;
			e.state = g->d_agc + i;
			e.level = m.d_level ? m.d_level + i * out_stride : nullptr;
			e.work = g->d_work + agc_floats;
			e.n_slots = (uint32_t)a.n_slots;
			e.first_wave = (uint32_t)agc_waves;
			e.first_piece = (uint32_t)agc_pieces;
			e.gain_check = m.agc.gain_check;
			agc_waves += a.n_slots;
			agc_pieces += a.n_pieces;
			agc_floats += a.floats;
		}
		const size_t n_fcch = (prelim || !n_afc) ? 0 : afc_work_of(m, p);
		if (n_fcch) {
			trx_afc_job &e = af[kf++];
			memset(&e, 0, sizeof(e));
			e.chunk = h_chunks[i].d_in;
			e.edge_row = p.straddle ? edge_row : nullptr;          /* assembled by this set's join, or by the prelim set's */
			e.first = p.to_skip;
			e.state = g->d_afc + i;
			e.out = m.d_fcch ? m.d_fcch + i * out_stride : nullptr;
			e.count = m.afc_count;
			e.n_fcch = (uint32_t)n_fcch;
			e.first_wave = (uint32_t)afc_waves;
			e.fn0 = p.fn0;
			e.tn0 = (uint8_t)p.tn0;
			afc_waves += n_fcch;
		}
		if (!w.n_slots)
			continue;
		sum = sum || w.sum;
		// the oscillator by absolute timestamp: the straddling slot begins at first_ts - carried, the chunk's first at first_ts + to_skip
		trx_nco_slot &o = nc[kr];
		memset(&o, 0, sizeof(o));
		if (m.nco.enable) {
			rot = true;
			o.inc = m.nco.inc;
			o.edge = trx_nco_phase(m.nco.acc, m.nco.ts_ref, m.nco.inc, p.first_ts - (int64_t)p.carried);
			o.phase0 = trx_nco_phase(m.nco.acc, m.nco.ts_ref, m.nco.inc, p.first_ts + p.to_skip);
		}
		trx_mss_member &e = rx[kr++];
		memset(&e, 0, sizeof(e));
		uint32_t fnk = p.fn;                                   /* prelim: the straddling slot's clock */
		int tnk = p.tn;
		if (!prelim)
			trx_mss_clock_add(p.fn0, p.tn0, w.k0, &fnk, &tnk);
		e.chunk = h_chunks[i].d_in;
		e.sa.edge_row = w.edge ? edge_row : nullptr;
		e.sa.first = prelim ? 0 : p.to_skip;
		e.sa.corr = w.sum ? g->d_corr + i : nullptr;
		e.sa.fn0 = fnk;
		e.sa.tn0 = (uint8_t)tnk;
		e.sa.tsc = m.tsc;
		e.sa.active = m.active;
		e.ind = d_ind + i * out_stride + w.k0;
		e.bits = d_bits ? d_bits + (i * out_stride + w.k0) * 148 : nullptr;
		e.n_slots = (uint32_t)w.n_slots;
		e.first_wave = (uint32_t)wave;
		wave += (w.n_slots + TRX_MS_RX_SLOTS_PER_WAVE - 1) / TRX_MS_RX_SLOTS_PER_WAVE;
	}
	if (kr != n_rx || kj != n_join || wave != n_waves || ka != n_agc || agc_floats > g->d_work.cap || kf != n_afc)
		return TRXHIP_EIO;

	if (!g->direct && hipMemcpyAsync(g->d_tab, rx, n_ent * 64 + (rot ? n_rx * sizeof(trx_nco_slot) : 0), hipMemcpyHostToDevice, st) != hipSuccess)
		return TRXHIP_EIO;
	if (n_join) {
		const trx_mss_join *jt = g->direct ? nullptr : reinterpret_cast<const trx_mss_join *>(g->d_tab + n_rx * 64);
		if (g->direct && cf32)
			hipLaunchKernelGGL(ms_join_kernel<float2>, dim3(1), dim3(kThreads), 0, st, *jn);
		else if (g->direct)
			hipLaunchKernelGGL(ms_join_kernel<uint32_t>, dim3(1), dim3(kThreads), 0, st, *jn);
		else if (cf32)
			hipLaunchKernelGGL(ms_join_group_kernel<float2>, dim3((unsigned)n_join), dim3(kThreads), 0, st, jt);
		else
			hipLaunchKernelGGL(ms_join_group_kernel<uint32_t>, dim3((unsigned)n_join), dim3(kThreads), 0, st, jt);
		if (launched() != TRXHIP_OK)
			return TRXHIP_EIO;
	}
	const size_t corr_bytes = g->m.size() * sizeof(int32_t);
	if (sum && hipMemsetAsync(g->d_corr, 0, corr_bytes, st) != hipSuccess)
		return TRXHIP_EIO;
	if (n_rx) {
		const float fs = g->rx_full_scale;                     /* 1.f / float(rxFullScale) (ms_upper.cpp:203), as trxhip_ms_rx_batch_*() */
		const trx_mss_member *rt = reinterpret_cast<const trx_mss_member *>(g->d_tab.p);
		const float *nt = g->ctx->d_nco_tab;
		int rc;
		if (!rot)
			rc = g->direct ? trx_launch_ms_rx_stream(rx->chunk, !cf32, &rx->sa, rx->ind, rx->bits, rx->n_slots, 1.0f / fs, fs, st)
				       : trx_launch_ms_rx_group(rt, !cf32, n_rx, n_waves, 1.0f / fs, fs, st);
		else
			rc = g->direct ? trx_launch_ms_rx_stream_nco(rx->chunk, !cf32, &rx->sa, rx->ind, rx->bits, rx->n_slots, 1.0f / fs, fs, nc, nt, st)
				       : trx_launch_ms_rx_group_nco(rt, !cf32, n_rx, n_waves, 1.0f / fs, fs,
								    reinterpret_cast<const trx_nco_slot *>(g->d_tab + n_ent * 64), nt, st);
		if (rc != 0)
			return TRXHIP_EIO;
	}
	if (sum && hipMemcpyAsync(g->h_corr, g->d_corr, corr_bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
		return TRXHIP_EIO;
	const int h = g->tab_at;
	if (g->ev_tab[h].record(st) != TRXHIP_OK)
		return TRXHIP_EIO;
	if (sum)
		g->corr_at = h;
	g->tab_at = (h + 1) % kTabSlots;
	if (n_agc) {
		const trx_agc_entry *at = g->direct ? nullptr : reinterpret_cast<const trx_agc_entry *>(g->d_tab + (n_rx + n_join) * 64);
		if (trx_launch_ms_agc(g->direct ? ag : nullptr, at, n_agc, agc_waves, agc_pieces, trx_agc_full_scale(g->rx_full_scale), st) != 0 ||
		    g->ev_agc.record(st) != TRXHIP_OK)
			return TRXHIP_EIO;
	}
	if (n_afc) {
		const trx_afc_job *ft = g->direct ? nullptr : reinterpret_cast<const trx_afc_job *>(g->d_tab + (n_rx + n_join + n_agc) * 64);
		if (trx_launch_ms_afc(g->direct ? af : nullptr, ft, !cf32, n_afc, afc_waves, 1.0f / g->rx_full_scale, st) != 0 ||
		    g->ev_afc.record(st) != TRXHIP_OK)
			return TRXHIP_EIO;
	}
	return TRXHIP_OK;
}

int group_pull(trxhip_ms_group *g, const trxhip_ms_group_chunk *h_chunks, int cf32, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
	       size_t out_stride, size_t *h_n_slots, size_t *h_n_carried, int *bad_member, void *stream)
{
	if (bad_member)
		*bad_member = -1;
	if (!g || !h_chunks)
		return TRXHIP_EINVAL;
	const size_t n = g->m.size();
	const bool device = g->ctx != nullptr;
	/* a plan-only group checks the counts against a stride it is given; the plan-only single object checks none */
	const bool bounded = device || (!g->direct && out_stride != 0);
	size_t first = n;
	for (size_t i = n; i-- > 0;)
		if (h_chunks[i].n_samples)
			first = i;
	if (first == n)
		return TRXHIP_EINVAL;                                  /* no member has a chunk */
	if (device && with_device(g->ctx))
		return TRXHIP_EIO;
	const hipStream_t st = static_cast<hipStream_t>(stream);

	// ---- every member's plan up to its straddling slot
	int worst = TRXHIP_OK;
	size_t bad = n;
	auto refuse = [&](size_t i, int rc) {
		g->rc[i] = rc;
		if (i < bad) {
			bad = i;
			worst = rc;
		}
	};
	bool any_tracked = false;
	size_t n_pre = 0;
	for (size_t i = 0; i < n; i++) {
		g->rc[i] = TRXHIP_OK;
		if (!h_chunks[i].n_samples)
			continue;
		const int rc = plan_begin(g->m[i], device, bounded, cf32, h_chunks[i].n_samples, h_chunks[i].first_ts, h_chunks[i].d_in,
					  d_ind, d_bits, out_stride, g->plan[i]);     /* (a record is 32 bytes: d_ind's alignment is every row's) */
		if (rc != TRXHIP_OK) {
			refuse(i, rc);
			continue;
		}
		if (g->m[i].agc_on && cf32) {
			refuse(i, TRXHIP_EINVAL);                              /* gain control measures int16 samples */
			continue;
		}
		if (!g->plan[i].extend) {
			any_tracked = any_tracked || g->m[i].tracking;
			n_pre += g->plan[i].prelim;
		}
	}

	// ---- the corrections of the pull before: the first of the two waits, once for the group
	if (device && any_tracked && fold_correction(g) != TRXHIP_OK)
		return TRXHIP_EIO;

	// ---- the straddling SCH slots the cutters follow, one slot per member in one launch set: the second
	if (device && n_pre &&
	    (issue_table(g, h_chunks, cf32, d_ind, d_bits, out_stride, true, n_pre, n_pre, n_pre, 0, 0, st) != TRXHIP_OK ||
	     g->ev_tab[g->corr_at].wait() != TRXHIP_OK))
		return TRXHIP_EIO;

	// ---- the rest of every plan
	size_t n_rx = 0, n_join = 0, n_waves = 0, n_agc = 0, agc_floats = 0, n_afc = 0;
	for (size_t i = 0; i < n; i++) {
		if (!h_chunks[i].n_samples || g->rc[i] != TRXHIP_OK)
			continue;
		ms_plan &p = g->plan[i];
		if (!p.extend) {
			const int rc = plan_finish(g->m[i], device, bounded, out_stride, (device && p.prelim) ? g->h_corr[i] : 0, p);
			if (rc != TRXHIP_OK) {
				refuse(i, rc);
				continue;
			}
		}
		const agc_work a = agc_work_of(g->m[i], p);
		if (!device && a.n_slots > g->m[i].lv_feed.size() - g->m[i].lv_at) {
			refuse(i, TRXHIP_EINVAL);                              /* plan-only: more slots than levels fed */
			continue;
		}
		n_agc += a.n_slots != 0;
		agc_floats += a.floats;
		n_afc += g->afc_members && afc_work_of(g->m[i], p) != 0;
		const ms_work w = work_of(g->m[i], p, false);
		n_join += w.join;
		if (w.n_slots) {
			n_rx++;
			n_waves += (w.n_slots + TRX_MS_RX_SLOTS_PER_WAVE - 1) / TRX_MS_RX_SLOTS_PER_WAVE;
		}
	}
	if (bad == n && (n_waves > 0x7fffffffu || agc_floats > 0x7fffffffu)) {     /* (agc_floats: more than a wave per measured slot) */
		bad = first;
		worst = TRXHIP_EINVAL;
	}
	if (bad != n) {                                                /* all or nothing: no member has moved */
		if (bad_member)
			*bad_member = (int)bad;
		return worst;
	}

	// ---- the issue: the pull's own launch set; the levels and piece results of a pull that needs more room than any before wait for
	// the device and allocate
	if (device && n_agc) {
		const int rc = g->d_work.reserve(agc_floats);
		if (rc != TRXHIP_OK)
			return rc;
	}
	if (device && issue_table(g, h_chunks, cf32, d_ind, d_bits, out_stride, false, n_rx, n_join, n_waves, n_agc, n_afc, st) != TRXHIP_OK)
		return TRXHIP_EIO;

	// ---- and every member moves
	for (size_t i = 0; i < n; i++) {
		ms_member &m = g->m[i];
		if (h_chunks[i].n_samples) {
			const ms_plan &p = g->plan[i];
			if (device) {
				if (p.extend || p.frac)
					m.rem_half ^= 1;
				if (work_of(m, p, false).sum)
					m.unread = true;
			}
			const agc_work a = agc_work_of(m, p);
			if (a.n_slots && device) {
				m.agc.gain_check = (uint32_t)((m.agc.gain_check + a.n_slots) % TRX_AGC_WINDOW);
			} else if (a.n_slots) {
				trx_agc_run(&m.agc, m.lv_feed.data() + m.lv_at, a.n_slots, trx_agc_full_scale(g->rx_full_scale));
				m.lv_at += a.n_slots;
			}
			if (g->afc_members)
				m.afc_count += afc_work_of(m, p);
			commit(m, p);
		}
		if (h_n_slots)
			h_n_slots[i] = h_chunks[i].n_samples ? m.last.n : 0;
		if (h_n_carried)
			h_n_carried[i] = m.first_call ? 0 : m.carried;
	}
	return TRXHIP_OK;
}

// what an acquire refuses before it looks at a buffer
int acquire_list(const trxhip_ms_group *g, const uint32_t *members, size_t n, size_t buf_len, const int64_t *first_ts)
{
	if (!g || !members || !first_ts || n == 0 || n > g->m.size() || buf_len < 512 + 20 || buf_len > TRXHIP_SCH_SYNC_MAX_LEN)
		return TRXHIP_EINVAL;
	std::vector<bool> seen(g->m.size(), false);
	for (size_t i = 0; i < n; i++) {
		if (members[i] >= g->m.size() || seen[members[i]])
			return TRXHIP_EINVAL;                                  /* a member listed twice */
		seen[members[i]] = true;
	}
	return TRXHIP_OK;
}

int group_acquire(trxhip_ms_group *g, const uint32_t *members, size_t n, const void *d_bufs, int cf32, size_t buf_stride, size_t buf_len,
		  const int64_t *first_ts, trxhip_sch_sync_result *h_res, int *h_found, void *stream)
{
	const int la = acquire_list(g, members, n, buf_len, first_ts);
	if (la != TRXHIP_OK)
		return la;
	const trxhip_sch_sync_result *res;
	if (!g->ctx) {
		if (d_bufs || !h_res)
			return TRXHIP_EINVAL;
		res = h_res;                                           /* plan-only: the receiver's answers come from outside */
	} else {
		if (!d_bufs || (reinterpret_cast<uintptr_t>(d_bufs) & (cf32 ? 7 : 3)) || buf_stride < buf_len)
			return TRXHIP_EINVAL;
		const float scale = 1.0f / g->rx_full_scale;
		const hipStream_t st = static_cast<hipStream_t>(stream);
		bool rot = false;
		for (size_t i = 0; i < n; i++)
			rot = rot || g->m[members[i]].nco.enable;
		if (rot) {
			// the buffers by absolute timestamp through the batch call into the work buffer; the search then reads complex64
			if (with_device(g->ctx))
				return TRXHIP_EIO;
			// a call that needs more room than any before frees and allocates (nothing is in flight: an acquire ends with a wait)
			const int rw = g->d_nco_work.reserve(n * buf_len * 2);
			if (rw != TRXHIP_OK)
				return rw;
			for (size_t i = 0; i < n; i++) {
				const trx_nco_state &o = g->m[members[i]].nco;
				g->h_nco_rec[i].phase0 = o.enable ? trx_nco_phase(o.acc, o.ts_ref, o.inc, first_ts[i]) : 0u;
				g->h_nco_rec[i].inc = o.enable ? o.inc : 0;
			}
			if (hipMemcpyAsync(g->d_nco_rec, g->h_nco_rec, n * sizeof(trxhip_ms_nco_row), hipMemcpyHostToDevice, st) != hipSuccess ||
			    trx_launch_ms_nco_rows(d_bufs, !cf32, buf_stride, g->d_nco_rec, g->d_nco_work, buf_len, n, buf_len, g->ctx->d_nco_tab, st) != 0)
				return TRXHIP_EIO;
			d_bufs = g->d_nco_work;
			buf_stride = buf_len;
			cf32 = 1;
		}
		const int rc = cf32 ? trxhip_sch_sync_batch_cf32(g->ctx, static_cast<const float *>(d_bufs), buf_stride, g->d_acq, nullptr, n, buf_len,
								 TRXHIP_SCH_SYNC_ACQ, scale, stream)
				    : trxhip_sch_sync_batch_i16(g->ctx, static_cast<const int16_t *>(d_bufs), buf_stride, g->d_acq, nullptr, n, buf_len,
								TRXHIP_SCH_SYNC_ACQ, scale, stream);
		if (rc != TRXHIP_OK)
			return rc;
		if (hipMemcpyAsync(g->h_acq, g->d_acq, n * sizeof(*g->h_acq), hipMemcpyDeviceToHost, st) != hipSuccess ||
		    g->ev.record(st) != TRXHIP_OK || g->ev.wait() != TRXHIP_OK)
			return TRXHIP_EIO;
		res = g->h_acq;
		if (h_res)
			memcpy(h_res, res, n * sizeof(*res));
	}
	for (size_t i = 0; i < n; i++)
		if (res[i].rc == 1 && (res[i].fn < 0 || (uint32_t)res[i].fn >= TRX_MSS_HYPERFRAME))
			return TRXHIP_EINVAL;
	int found = 0;
	for (size_t i = 0; i < n; i++) {
		const bool ok = res[i].rc == 1;
		if (ok)
			acquired(g->m[members[i]], res[i], first_ts[i]);
		if (h_found)
			h_found[i] = ok;
		found += ok;
	}
	return found;
}

// Cold start (include/trxhip.h, "MS-side FCCH search"): the composition of the public calls -- the search over the buffers as
// received, one wait, the NCO of every member whose FCCH is found set from its measurement, then the acquire above for exactly
// those members, one call per run of consecutive listed members.  Every refusal comes before anything is set.
int group_acquire_afc(trxhip_ms_group *g, const uint32_t *members, size_t n, const void *d_bufs, int cf32, size_t buf_stride, size_t buf_len,
		      const int64_t *first_ts, double min_score, trxhip_ms_fcch_hit *h_hit, trxhip_ms_fcch *h_fcch,
		      trxhip_sch_sync_result *h_res, int *h_found, void *stream)
{
	const int la = acquire_list(g, members, n, buf_len, first_ts);
	if (la != TRXHIP_OK)
		return la;
	if (!g->ctx || !d_bufs || (reinterpret_cast<uintptr_t>(d_bufs) & (cf32 ? 7 : 3)) || buf_stride < buf_len)
		return TRXHIP_EINVAL;                                  /* (plan-only: no samples to search) */
	const int rs = cf32 ? trxhip_ms_fcch_search_cf32(g->ctx, static_cast<const float *>(d_bufs), buf_stride, buf_len, n, min_score,
							 g->rx_full_scale, g->d_fs_hit, g->d_fs_fcch, stream)
			    : trxhip_ms_fcch_search_i16(g->ctx, static_cast<const int16_t *>(d_bufs), buf_stride, buf_len, n, min_score,
							g->rx_full_scale, g->d_fs_hit, g->d_fs_fcch, stream);
	if (rs != TRXHIP_OK)
		return rs;
	const hipStream_t st = static_cast<hipStream_t>(stream);
	if (hipMemcpyAsync(g->h_fs_hit, g->d_fs_hit, n * sizeof(*g->h_fs_hit), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipMemcpyAsync(g->h_fs_fcch, g->d_fs_fcch, n * sizeof(*g->h_fs_fcch), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    g->ev.record(st) != TRXHIP_OK || g->ev.wait() != TRXHIP_OK)
		return TRXHIP_EIO;
	std::vector<int32_t> inc(n, 0);
	for (size_t i = 0; i < n; i++)
		if (g->h_fs_hit[i].found && trx_nco_inc(-((double)g->h_fs_fcch[i].hz - TRXHIP_MS_FCCH_BIAS_HZ), &inc[i]) != 0)
			return TRXHIP_EINVAL;                                  /* what trxhip_ms_nco_group_set would refuse */
	if (h_hit)
		memcpy(h_hit, g->h_fs_hit, n * sizeof(*h_hit));
	if (h_fcch)
		memcpy(h_fcch, g->h_fs_fcch, n * sizeof(*h_fcch));
	if (h_found)
		memset(h_found, 0, n * sizeof(*h_found));
	for (size_t i = 0; i < n; i++)
		if (g->h_fs_hit[i].found) {
			ms_member &m = g->m[members[i]];
			trx_nco_set(&m.nco, true, -((double)g->h_fs_fcch[i].hz - TRXHIP_MS_FCCH_BIAS_HZ), inc[i], m.ts);
		}
	int found = 0;
	const char *bufs = static_cast<const char *>(d_bufs);
	for (size_t a = 0; a < n;) {
		if (!g->h_fs_hit[a].found) {
			a++;
			continue;
		}
		size_t b = a + 1;
		while (b < n && g->h_fs_hit[b].found)
			b++;
		const int rc = group_acquire(g, members + a, b - a, bufs + a * buf_stride * (cf32 ? 8 : 4), cf32, buf_stride, buf_len, first_ts + a,
					     h_res ? h_res + a : nullptr, h_found ? h_found + a : nullptr, stream);
		if (rc < 0)
			return rc;
		found += rc;
		a = b;
	}
	return found;
}

ms_member *member_of(trxhip_ms_group *g, uint32_t i) { return (g && i < g->m.size()) ? &g->m[i] : nullptr; }
const ms_member *member_of(const trxhip_ms_group *g, uint32_t i) { return (g && i < g->m.size()) ? &g->m[i] : nullptr; }

// direct: the single object, which needs no table
int group_create(trxhip_ctx *ctx, float rx_full_scale, size_t n_members, const trxhip_ms_sched_cfg *cfgs, bool direct, trxhip_ms_group **out)
{
	if (!cfgs || !out || n_members < 1 || n_members > TRXHIP_MS_GROUP_MAX_MEMBERS || !std::isfinite(rx_full_scale) || !(rx_full_scale > 0.0f))
		return TRXHIP_EINVAL;
	for (size_t i = 0; i < n_members; i++)
		if (!cfg_ok(&cfgs[i]) || cfgs[i].rx_full_scale != rx_full_scale)
			return TRXHIP_EINVAL;
	if (ctx && with_device(ctx))
		return TRXHIP_EINVAL;
	trxhip_ms_group *g = new (std::nothrow) trxhip_ms_group();
	if (!g)
		return TRXHIP_ENOMEM;
	g->rx_full_scale = rx_full_scale;
	g->direct = direct;
	g->m.resize(n_members);
	g->plan.resize(n_members);
	g->rc.resize(n_members);
	for (size_t i = 0; i < n_members; i++) {
		g->m[i].tsc = cfgs[i].tsc;
		g->m[i].active = cfgs[i].active_tns;
		g->m[i].tracking = cfgs[i].tracking != 0;
	}
	if (!ctx) {
		*out = g;
		return TRXHIP_OK;
	}
	g->ctx = ctx;
	const size_t n = n_members;
	const size_t rem_bytes = n * 2 * TRX_MSS_REM_STRIDE * 8, tab_bytes = kTabEntries * n * 64;     /* tab_bytes: one table */
	bool ok = g->d_rem.alloc(rem_bytes) == TRXHIP_OK && g->d_edge.alloc(n * TRX_MSS_SLOT * 8) == TRXHIP_OK && g->d_corr.alloc(n) == TRXHIP_OK &&
		  g->d_acq.alloc(n) == TRXHIP_OK && g->h_corr.alloc(n) == TRXHIP_OK && g->h_acq.alloc(n) == TRXHIP_OK && g->ev.create() == TRXHIP_OK &&
		  g->d_agc.alloc(n) == TRXHIP_OK && g->ev_agc.create() == TRXHIP_OK && g->d_afc.alloc(n) == TRXHIP_OK &&
		  g->ev_afc.create() == TRXHIP_OK && g->d_nco_rec.alloc(n) == TRXHIP_OK && g->h_nco_rec.alloc(n) == TRXHIP_OK &&
		  g->d_fs_hit.alloc(n) == TRXHIP_OK && g->h_fs_hit.alloc(n) == TRXHIP_OK && g->d_fs_fcch.alloc(n) == TRXHIP_OK &&
		  g->h_fs_fcch.alloc(n) == TRXHIP_OK;
	if (!direct)
		ok = ok && g->d_tab.alloc(tab_bytes) == TRXHIP_OK && g->h_tab.alloc(kTabSlots * tab_bytes) == TRXHIP_OK;
	for (int h = 0; h < kTabSlots; h++)
		ok = ok && g->ev_tab[h].create() == TRXHIP_OK;
	ok = ok && hipMemset(g->d_rem, 0, rem_bytes) == hipSuccess && hipMemset(g->d_corr, 0, n * sizeof(int32_t)) == hipSuccess &&
	     hipMemset(g->d_agc, 0, n * sizeof(trx_agc_state)) == hipSuccess && hipMemset(g->d_afc, 0, n * sizeof(trx_afc_state)) == hipSuccess &&
	     hipStreamSynchronize(nullptr) == hipSuccess;      /* the first pull may come on a stream that does not wait for the null stream */
	if (!ok) {
		trxhip_ms_group_destroy(g);
		return TRXHIP_ENOMEM;
	}
	memset(g->h_corr, 0, n * sizeof(int32_t));
	*out = g;
	return TRXHIP_OK;
}

// the single object's handle and the group of one behind it
trxhip_ms_group *group_of(trxhip_ms_sched *s) { return reinterpret_cast<trxhip_ms_group *>(s); }
const trxhip_ms_group *group_of(const trxhip_ms_sched *s) { return reinterpret_cast<const trxhip_ms_group *>(s); }

}  // namespace

extern "C" {

int trxhip_ms_group_create(trxhip_ctx *ctx, float rx_full_scale, size_t n_members, const trxhip_ms_sched_cfg *cfgs, trxhip_ms_group **out)
{
	return group_create(ctx, rx_full_scale, n_members, cfgs, false, out);
}

// waits for what is in flight before it frees
void trxhip_ms_group_destroy(trxhip_ms_group *g)
{
	if (!g)
		return;
	if (g->ctx)
		(void)with_device(g->ctx);
	delete g;
}

int trxhip_ms_group_members(const trxhip_ms_group *g) { return g ? (int)g->m.size() : TRXHIP_EINVAL; }

int trxhip_ms_group_set_clock(trxhip_ms_group *g, uint32_t member, uint32_t fn, int tn, int64_t ts)
{
	ms_member *m = member_of(g, member);
	if (!m || fn >= TRX_MSS_HYPERFRAME || tn < 0 || tn > 7)
		return TRXHIP_EINVAL;
	set_clock(*m, fn, tn, ts);
	return TRXHIP_OK;
}

int trxhip_ms_group_clock(const trxhip_ms_group *g, uint32_t member, uint32_t *fn, int *tn, int64_t *ts)
{
	const ms_member *m = member_of(g, member);
	if (!m || !fn || !tn || !ts || !m->clock_set)
		return TRXHIP_EINVAL;
	*fn = m->fn;
	*tn = m->tn;
	*ts = m->ts;
	return TRXHIP_OK;
}

int trxhip_ms_group_set_tsc(trxhip_ms_group *g, uint32_t member, int tsc)
{
	ms_member *m = member_of(g, member);
	if (!m || tsc < 0 || tsc > 7)
		return TRXHIP_EINVAL;
	m->tsc = (uint8_t)tsc;
	return TRXHIP_OK;
}

int trxhip_ms_group_set_active(trxhip_ms_group *g, uint32_t member, uint8_t tn_mask)
{
	ms_member *m = member_of(g, member);
	if (!m)
		return TRXHIP_EINVAL;
	m->active = tn_mask;
	return TRXHIP_OK;
}

int trxhip_ms_group_set_tracking(trxhip_ms_group *g, uint32_t member, int on)
{
	ms_member *m = member_of(g, member);
	if (!m)
		return TRXHIP_EINVAL;
	m->tracking = on != 0;
	return TRXHIP_OK;
}

int trxhip_ms_group_feed_starts(trxhip_ms_group *g, uint32_t member, const int32_t *starts, size_t n)
{
	ms_member *m = member_of(g, member);
	if (!m || g->ctx || (!starts && n))
		return TRXHIP_EINVAL;
	m->feed.assign(starts, starts + n);
	m->feed_at = 0;
	return TRXHIP_OK;
}

int64_t trxhip_ms_group_slots(const trxhip_ms_group *g, uint32_t member, size_t n_samples)
{
	const ms_member *m = member_of(g, member);
	return m ? slots_of(*m, n_samples) : TRXHIP_EINVAL;
}

int trxhip_ms_group_plan(const trxhip_ms_group *g, uint32_t member, trxhip_ms_plan *h_out, size_t n)
{
	const ms_member *m = member_of(g, member);
	return m ? plan_of(*m, h_out, n) : TRXHIP_EINVAL;
}

int trxhip_ms_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_sched_status *out)
{
	const ms_member *m = member_of(g, member);
	if (!m || !out)
		return TRXHIP_EINVAL;
	if (g->ctx && fold_correction(g) != TRXHIP_OK)
		return TRXHIP_EIO;
	state_of(*m, out);
	return TRXHIP_OK;
}

int trxhip_ms_group_acquire_s16(trxhip_ms_group *g, const uint32_t *members, size_t n, const int16_t *d_bufs, size_t buf_stride,
				size_t buf_len, const int64_t *first_ts, trxhip_sch_sync_result *h_res, int *h_found, void *stream)
{
	return group_acquire(g, members, n, d_bufs, 0, buf_stride, buf_len, first_ts, h_res, h_found, stream);
}

int trxhip_ms_group_acquire_cf32(trxhip_ms_group *g, const uint32_t *members, size_t n, const float *d_bufs, size_t buf_stride,
				 size_t buf_len, const int64_t *first_ts, trxhip_sch_sync_result *h_res, int *h_found, void *stream)
{
	return group_acquire(g, members, n, d_bufs, 1, buf_stride, buf_len, first_ts, h_res, h_found, stream);
}

int trxhip_ms_afc_group_acquire_s16(trxhip_ms_group *g, const uint32_t *members, size_t n, const int16_t *d_bufs, size_t buf_stride,
				    size_t buf_len, const int64_t *first_ts, double min_score, trxhip_ms_fcch_hit *h_hit, trxhip_ms_fcch *h_fcch,
				    trxhip_sch_sync_result *h_res, int *h_found, void *stream)
{
	return group_acquire_afc(g, members, n, d_bufs, 0, buf_stride, buf_len, first_ts, min_score, h_hit, h_fcch, h_res, h_found, stream);
}

int trxhip_ms_afc_group_acquire_cf32(trxhip_ms_group *g, const uint32_t *members, size_t n, const float *d_bufs, size_t buf_stride,
				     size_t buf_len, const int64_t *first_ts, double min_score, trxhip_ms_fcch_hit *h_hit, trxhip_ms_fcch *h_fcch,
				     trxhip_sch_sync_result *h_res, int *h_found, void *stream)
{
	return group_acquire_afc(g, members, n, d_bufs, 1, buf_stride, buf_len, first_ts, min_score, h_hit, h_fcch, h_res, h_found, stream);
}

int trxhip_ms_group_pull_s16(trxhip_ms_group *g, const trxhip_ms_group_chunk *h_chunks, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
			     size_t out_stride, size_t *h_n_slots, size_t *h_n_carried, int *bad_member, void *stream)
{
	return group_pull(g, h_chunks, 0, d_ind, d_bits, out_stride, h_n_slots, h_n_carried, bad_member, stream);
}

int trxhip_ms_group_pull_cf32(trxhip_ms_group *g, const trxhip_ms_group_chunk *h_chunks, trxhip_ms_burst_ind *d_ind, int8_t *d_bits,
			      size_t out_stride, size_t *h_n_slots, size_t *h_n_carried, int *bad_member, void *stream)
{
	return group_pull(g, h_chunks, 1, d_ind, d_bits, out_stride, h_n_slots, h_n_carried, bad_member, stream);
}

// ---- gain control (trx_ms_agc.h) -----------------------------------------------------------------

// the AGC launches in flight are through: the member's state on the device may be read or written from the host
static int agc_settled(trxhip_ms_group *g)
{
	if (with_device(g->ctx) || g->ev_agc.wait() != TRXHIP_OK)
		return TRXHIP_EIO;
	return TRXHIP_OK;
}

int trxhip_ms_agc_group_set_gain(trxhip_ms_group *g, uint32_t member, float rx_gain)
{
	ms_member *m = member_of(g, member);
	if (!m || !std::isfinite(rx_gain))
		return TRXHIP_EINVAL;
	if (g->ctx && (agc_settled(g) != TRXHIP_OK ||
		       hipMemcpy(&g->d_agc[member].rx_gain, &rx_gain, sizeof(float), hipMemcpyHostToDevice) != hipSuccess))
		return TRXHIP_EIO;
	m->agc.rx_gain = rx_gain;
	return TRXHIP_OK;
}

int trxhip_ms_agc_group_set(trxhip_ms_group *g, uint32_t member, const trxhip_ms_agc_cfg *cfg)
{
	ms_member *m = member_of(g, member);
	if (!m || !cfg || !std::isfinite(cfg->rx_gain) || (cfg->d_level && (!g->ctx || (reinterpret_cast<uintptr_t>(cfg->d_level) & 3))))
		return TRXHIP_EINVAL;
	const int rc = trxhip_ms_agc_group_set_gain(g, member, cfg->rx_gain);
	if (rc != TRXHIP_OK)
		return rc;
	m->agc_on = cfg->enable != 0;
	m->d_level = cfg->d_level;
	return TRXHIP_OK;
}

int trxhip_ms_agc_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_agc_status *out)
{
	const ms_member *m = member_of(g, member);
	if (!m || !out)
		return TRXHIP_EINVAL;
	trx_agc_state s = m->agc;
	if (g->ctx && (agc_settled(g) != TRXHIP_OK || hipMemcpy(&s, g->d_agc + member, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess))
		return TRXHIP_EIO;
	memset(out, 0, sizeof(*out));
	out->rx_gain = s.rx_gain;
	out->runmean = s.runmean;
	out->gain_check = s.gain_check;
	out->enable = m->agc_on;
	out->slots = s.slots;
	out->decisions = s.decisions;
	out->applied = s.applied;
	out->n_records = (uint32_t)(s.decisions < TRX_AGC_RING ? s.decisions : TRX_AGC_RING);
	for (uint32_t k = 0; k < out->n_records; k++)
		out->ring[k] = s.ring[(s.decisions - out->n_records + k) % TRX_AGC_RING];
	return TRXHIP_OK;
}

int trxhip_ms_agc_group_feed_levels(trxhip_ms_group *g, uint32_t member, const float *levels, size_t n)
{
	ms_member *m = member_of(g, member);
	if (!m || g->ctx || (!levels && n))
		return TRXHIP_EINVAL;
	m->lv_feed.assign(levels, levels + n);
	m->lv_at = 0;
	return TRXHIP_OK;
}

int trxhip_ms_agc_sched_set(trxhip_ms_sched *s, const trxhip_ms_agc_cfg *cfg) { return trxhip_ms_agc_group_set(group_of(s), 0, cfg); }

int trxhip_ms_agc_sched_set_gain(trxhip_ms_sched *s, float rx_gain) { return trxhip_ms_agc_group_set_gain(group_of(s), 0, rx_gain); }

int trxhip_ms_agc_sched_state(trxhip_ms_sched *s, trxhip_ms_agc_status *out) { return trxhip_ms_agc_group_state(group_of(s), 0, out); }

int trxhip_ms_agc_sched_feed_levels(trxhip_ms_sched *s, const float *levels, size_t n)
{
	return trxhip_ms_agc_group_feed_levels(group_of(s), 0, levels, n);
}

// ---- FCCH frequency-offset measurement (trx_ms_afc.h) ---------------------------------------------

// the AFC launch in flight is through: the members' states on the device may be read from the host, d_fcch may change
static int afc_settled(trxhip_ms_group *g)
{
	if (with_device(g->ctx) || g->ev_afc.wait() != TRXHIP_OK)
		return TRXHIP_EIO;
	return TRXHIP_OK;
}

int trxhip_ms_afc_group_set(trxhip_ms_group *g, uint32_t member, const trxhip_ms_afc_cfg *cfg)
{
	ms_member *m = member_of(g, member);
	if (!m || !cfg || !g->ctx || (reinterpret_cast<uintptr_t>(cfg->d_fcch) & 3))      /* a plan-only object has no samples */
		return TRXHIP_EINVAL;
	if (afc_settled(g) != TRXHIP_OK)
		return TRXHIP_EIO;
	g->afc_members += (cfg->enable != 0) - (m->afc_on ? 1 : 0);
	m->afc_on = cfg->enable != 0;
	m->d_fcch = cfg->d_fcch;
	return TRXHIP_OK;
}

int trxhip_ms_afc_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_afc_status *out)
{
	const ms_member *m = member_of(g, member);
	if (!m || !out)
		return TRXHIP_EINVAL;
	trx_afc_state s = {};
	if (g->ctx && (afc_settled(g) != TRXHIP_OK || hipMemcpy(&s, g->d_afc + member, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess))
		return TRXHIP_EIO;
	memset(out, 0, sizeof(*out));
	out->count = s.count;
	out->enable = m->afc_on;
	out->last = s.last;
	out->n_records = (uint32_t)(s.count < TRX_AFC_RING ? s.count : TRX_AFC_RING);
	for (uint32_t k = 0; k < out->n_records; k++)
		out->ring[k] = s.ring[(s.count - out->n_records + k) % TRX_AFC_RING];
	return TRXHIP_OK;
}

int trxhip_ms_afc_sched_set(trxhip_ms_sched *s, const trxhip_ms_afc_cfg *cfg) { return trxhip_ms_afc_group_set(group_of(s), 0, cfg); }

int trxhip_ms_afc_sched_state(trxhip_ms_sched *s, trxhip_ms_afc_status *out) { return trxhip_ms_afc_group_state(group_of(s), 0, out); }

// ---- the NCO (trx_ms_nco.h): host state only, a pull takes it by value -----------------------------

int trxhip_ms_nco_group_set(trxhip_ms_group *g, uint32_t member, const trxhip_ms_nco_cfg *cfg)
{
	ms_member *m = member_of(g, member);
	int32_t inc;
	if (!m || !cfg || trx_nco_inc(cfg->hz, &inc) != 0)
		return TRXHIP_EINVAL;
	trx_nco_set(&m->nco, cfg->enable != 0, cfg->hz, inc, m->ts);
	return TRXHIP_OK;
}

int trxhip_ms_nco_group_state(trxhip_ms_group *g, uint32_t member, trxhip_ms_nco_status *out)
{
	const ms_member *m = member_of(g, member);
	if (!m || !out)
		return TRXHIP_EINVAL;
	memset(out, 0, sizeof(*out));
	out->enable = m->nco.enable;
	out->inc = m->nco.inc;
	out->acc = m->nco.acc;
	out->ts_ref = m->nco.ts_ref;
	out->hz = m->nco.hz;
	return TRXHIP_OK;
}

int trxhip_ms_nco_sched_set(trxhip_ms_sched *s, const trxhip_ms_nco_cfg *cfg) { return trxhip_ms_nco_group_set(group_of(s), 0, cfg); }

int trxhip_ms_nco_sched_state(trxhip_ms_sched *s, trxhip_ms_nco_status *out) { return trxhip_ms_nco_group_state(group_of(s), 0, out); }

// ---- the single object: member 0 of a group of one that issues directly -------------------------

int trxhip_ms_sched_create(trxhip_ctx *ctx, const trxhip_ms_sched_cfg *cfg, trxhip_ms_sched **out)
{
	trxhip_ms_group *g = nullptr;
	if (!cfg || !out)
		return TRXHIP_EINVAL;
	const int rc = group_create(ctx, cfg->rx_full_scale, 1, cfg, true, &g);
	if (rc == TRXHIP_OK)
		*out = reinterpret_cast<trxhip_ms_sched *>(g);
	return rc;
}

void trxhip_ms_sched_destroy(trxhip_ms_sched *s) { trxhip_ms_group_destroy(group_of(s)); }

int trxhip_ms_sched_set_clock(trxhip_ms_sched *s, uint32_t fn, int tn, int64_t ts) { return trxhip_ms_group_set_clock(group_of(s), 0, fn, tn, ts); }

int trxhip_ms_sched_clock(const trxhip_ms_sched *s, uint32_t *fn, int *tn, int64_t *ts) { return trxhip_ms_group_clock(group_of(s), 0, fn, tn, ts); }

int trxhip_ms_sched_set_tsc(trxhip_ms_sched *s, int tsc) { return trxhip_ms_group_set_tsc(group_of(s), 0, tsc); }

int trxhip_ms_sched_set_active(trxhip_ms_sched *s, uint8_t tn_mask) { return trxhip_ms_group_set_active(group_of(s), 0, tn_mask); }

int trxhip_ms_sched_set_tracking(trxhip_ms_sched *s, int on) { return trxhip_ms_group_set_tracking(group_of(s), 0, on); }

int trxhip_ms_sched_feed_starts(trxhip_ms_sched *s, const int32_t *starts, size_t n)
{
	return trxhip_ms_group_feed_starts(group_of(s), 0, starts, n);
}

int64_t trxhip_ms_sched_slots(const trxhip_ms_sched *s, size_t n_samples) { return trxhip_ms_group_slots(group_of(s), 0, n_samples); }

int trxhip_ms_sched_plan(const trxhip_ms_sched *s, trxhip_ms_plan *h_out, size_t n) { return trxhip_ms_group_plan(group_of(s), 0, h_out, n); }

int trxhip_ms_sched_state(trxhip_ms_sched *s, trxhip_ms_sched_status *out) { return trxhip_ms_group_state(group_of(s), 0, out); }

// 1 (found) or 0, as the group's count of one buffer
int trxhip_ms_sched_acquire_s16(trxhip_ms_sched *s, const int16_t *d_buf, size_t n_samples, int64_t first_ts, trxhip_sch_sync_result *h_res,
				void *stream)
{
	const uint32_t member = 0;
	return group_acquire(group_of(s), &member, 1, d_buf, 0, n_samples, n_samples, &first_ts, h_res, nullptr, stream);
}

int trxhip_ms_sched_acquire_cf32(trxhip_ms_sched *s, const float *d_buf, size_t n_samples, int64_t first_ts, trxhip_sch_sync_result *h_res,
				 void *stream)
{
	const uint32_t member = 0;
	return group_acquire(group_of(s), &member, 1, d_buf, 1, n_samples, n_samples, &first_ts, h_res, nullptr, stream);
}

// one chunk, out_slots as the stride; *n_slots and *n_carried (the new partial slot, or the extended one) are member 0's
int trxhip_ms_afc_sched_acquire_s16(trxhip_ms_sched *s, const int16_t *d_buf, size_t n_samples, int64_t first_ts, double min_score,
				    trxhip_ms_fcch_hit *h_hit, trxhip_ms_fcch *h_fcch, trxhip_sch_sync_result *h_res, void *stream)
{
	const uint32_t member = 0;
	return group_acquire_afc(group_of(s), &member, 1, d_buf, 0, n_samples, n_samples, &first_ts, min_score, h_hit, h_fcch, h_res, nullptr,
				 stream);
}

int trxhip_ms_afc_sched_acquire_cf32(trxhip_ms_sched *s, const float *d_buf, size_t n_samples, int64_t first_ts, double min_score,
				     trxhip_ms_fcch_hit *h_hit, trxhip_ms_fcch *h_fcch, trxhip_sch_sync_result *h_res, void *stream)
{
	const uint32_t member = 0;
	return group_acquire_afc(group_of(s), &member, 1, d_buf, 1, n_samples, n_samples, &first_ts, min_score, h_hit, h_fcch, h_res, nullptr,
				 stream);
}

int trxhip_ms_sched_pull_s16(trxhip_ms_sched *s, const int16_t *d_in, size_t n_samples, int64_t first_ts, trxhip_ms_burst_ind *d_ind,
			     int8_t *d_bits, size_t out_slots, size_t *n_slots, size_t *n_carried, void *stream)
{
	const trxhip_ms_group_chunk c = { d_in, n_samples, first_ts };
	return group_pull(group_of(s), &c, 0, d_ind, d_bits, out_slots, n_slots, n_carried, nullptr, stream);
}

int trxhip_ms_sched_pull_cf32(trxhip_ms_sched *s, const float *d_in, size_t n_samples, int64_t first_ts, trxhip_ms_burst_ind *d_ind,
			      int8_t *d_bits, size_t out_slots, size_t *n_slots, size_t *n_carried, void *stream)
{
	const trxhip_ms_group_chunk c = { d_in, n_samples, first_ts };
	return group_pull(group_of(s), &c, 1, d_ind, d_bits, out_slots, n_slots, n_carried, nullptr, stream);
}

}  // extern "C"
