// trx_ms_tx.cpp -- the MS-side uplink burst scheduler: burst requests in, the radio's transmit sample stream out.
//
// The host half restates what the reference decides per burst request:
//   upper_trx::driveTx()          ms/ms_upper.cpp:306-355   (the power scale; modulate, scale, int16)
//   ms_trx::submit_burst()        ms/ms.cpp:114-160         (target FN/TN, timekeeper, timing advance -> send_ts; "TX too late")
//   ms_trx::set_ta()              ms/ms.h:299-303
//   submit_burst_ts()             ms/uhd_specific.h:260-269, ms/bladerf_specific.h:461-478   (ts + rxtxdelay)
//   GSM::Time::incTN / decTN      GSM/GSMCommon.h:129-150;  GSM::FNDelta  GSM/GSMCommon.cpp:71-78
// and keeps the queued bursts ordered by the timestamp of their first sample.  With ctx == NULL an object is plan-only: the same
// arithmetic and queue, no device memory.
//
// There is one object, the group (trxhip_ms_tx_group_*): N members behind one radio type.  A member -- its timing advance, queue,
// window state, counters and ring rows -- is one struct (Member) with one set of rules (plan_request, queue_place, place_request,
// retire, walk_window).  A group's render uploads one table -- an entry per rendered member, then the queued bursts that
// intersect its window -- and the device half (trx_tx.hip, ms_tx_render_group_kernel) cuts every window into tiles of 625
// samples and finds each tile's bursts.  The single object (trxhip_ms_tx_*) is a group of one member with the flag `direct`, its
// entry points forwards to member 0 through the same create, submit and render.  `direct` chooses how the one member's work
// reaches the device: a submit copies every run of consecutive ring rows to where it lies (a group sends rows and destinations
// up in one copy and scatters them with ms_tx_stage_kernel), and a render tiles the window with host-made segments --
// stretches of queued bursts and zeros in between, at most 625 samples each -- that ms_tx_render_kernel draws where they lie:
// on a render of 8 slots that kernel is 0.9 us faster than the tile kernel.
//
// The uplink oscillator (trxhip_ms_nco_tx_*; trx_ms_nco.h is the arithmetic, include/trxhip.h the contract) is a trx_nco_state in
// the Member.  _set is trx_nco_set() at the member's rendered_end; a render hands the kernel {p(first_ts), inc} by value -- a kernel
// argument with `direct`, the two words of the member's table entry otherwise -- and runs the rotating instance of its kernel
// when a rendered member has the oscillator on.  No copy, launch or event is added, and with it off everywhere a render issues
// what it issued before there was one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <queue>
#include <vector>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_nco.h"
#include "trx_ms_tx.h"
#include "trx_tx_tables.h"

namespace {

const int32_t kHyperframe = 2715648;         /* GSM::gHyperframe */
const int64_t kBurst = TRX_MSTX_BURST;
const int kBufs = 4;                          /* pinned buffers in flight per kind: a call waits for the 4th before */
const uint32_t kMaxPending = 1u << 22;
const size_t kMaxWindow = (size_t)1 << 31;
const int64_t kMaxTs = (int64_t)1 << 62;     /* |now_ts|, |first_ts|: the sums stay inside int64 */

// GSM::FNDelta, GSMCommon.cpp:71-78
int32_t fn_delta(int32_t v1, int32_t v2)
{
	const int32_t half = kHyperframe / 2;
	int32_t d = v1 - v2;
	if (d >= half)
		d -= kHyperframe;
	else if (d < -half)
		d += kHyperframe;
	return d;
}

// GSM::Time with the two members submit_burst() calls, GSMCommon.h:129-150 (step <= 8 by its asserts)
struct GsmTime {
	int fn, tn;
	void decTN(unsigned step)
	{
		tn -= (int)step;
		if (tn < 0) {
			tn += 8;
			fn -= 1;
			if (fn < 0)
				fn += kHyperframe;
		}
	}
	void incTN(unsigned step)
	{
		tn += (int)step;
		if (tn > 7) {
			tn -= 8;
			fn = (fn + 1) % kHyperframe;
		}
	}
};

struct Pending {
	int64_t radio_ts;
	uint32_t row;             /* ring row (plan-only: unused) */
	bool touched;             /* a sample of it lay in a rendered window */
};

struct PinBuf {
	trx_pin<uint8_t> h;
	trx_event ev;              /* pending: the call that used the buffer last (behind h: waited for before h is freed) */
};

// the largest |sample| the Laurent modulator makes: per phase of the 4-SPS grid a sample sums every 4th tap of c0 and of c1
// against symbol values of modulus 1 (tx_stage_syms), so each component is at most the phase's sum of |taps|
double pulse_bound()
{
	trx_tx_tables *tab = static_cast<trx_tx_tables *>(malloc(sizeof(trx_tx_tables)));
	if (!tab || trx_tx_tables_generate(tab) != 0) {
		free(tab);
		return INFINITY;
	}
	double best = 0.0;
	for (int p = 0; p < 4; p++) {
		double s = 0.0;
		for (int k = p; k < 16; k += 4)
			s += std::fabs((double)tab->pulse4_c0[k]);
		for (int k = p; k < 8; k += 4)
			s += std::fabs((double)tab->pulse4_c1[k]);
		best = std::max(best, s);
	}
	free(tab);
	return best * (1.0 + 1.0 / (1 << 20));      /* the float roundings of at most 6 products, 6 sums and the scale: < 2^-20 */
}

// The largest |component| behind the uplink oscillator, per unit of scale.  pulse_bound() bounds a component of the modulator's
// sample x; the rotation mixes the two components, so here the MODULUS of x is bounded, by the same triangle inequality: the taps
// are real and a sample is sum(tap * symbol), so |x| <= sum|taps| * max|symbol| per phase of the grid.  A c0 symbol is +-rot4[4m],
// a c1 symbol that times (0, +-1) (tx_stage_syms), so max|symbol| = max|rot4[4m]|, taken from the table (1 up to the rounding of
// cos and sin to float).  Roundings, u = 2^-24:
//   x       a component's error is at most 8u * sum|tap * symbol component| (at most 6 products, 6 sums, the real scale), so the
//           modulus grows by at most sqrt(2) * 8u < 2^-20 relative: the allowance pulse_bound() already carries
//   tables  an entry is (cos, sin) rounded per component: |C|, |F| <= 1 + u
//   phasor  r = (Cc Fc - Cs Fs, Cc Fs + Cs Fc): |C||F| <= 1 + 2u + u^2; per component two products and a sum, error at most
//           3u (|Cc Fc| + |Cs Fs|) <= 3u |C||F|, so |r| <= (1 + 2u + u^2)(1 + 3 sqrt(2) u) < 1 + 6.3u
//   rotate  a component of x * r is at most |x||r|; two products and a sum add at most 3u (|xr rc| + |xi rs|) <= 3u |x||r|
// together |y component| <= |x| (1 + 6.3u)(1 + 3u) < |x| (1 + 10u), allowed for here as 16u = 2^-20.  The cast's own factor 1.0f is
// exact.  The gap that 21477 leaves is 2.96e-5 = 497u; the two allowances use 32u.
double nco_bound()
{
	trx_tx_tables *tab = static_cast<trx_tx_tables *>(malloc(sizeof(trx_tx_tables)));
	if (!tab || trx_tx_tables_generate(tab) != 0) {
		free(tab);
		return INFINITY;
	}
	double sym = 0.0;
	for (int m = 0; m <= 149; m++)              /* tx_stage_syms: m = 0 .. nbits + 1 */
		sym = std::max(sym, std::hypot((double)tab->rot4[4 * m].re, (double)tab->rot4[4 * m].im));
	free(tab);
	return pulse_bound() * sym * (1.0 + 1.0 / (1 << 20));
}

// One MS: what set_ta(), submit_burst() and the windows of its stream act on.  A group has N, the single object one.
struct Member {
	int32_t timing_advance = 0;
	std::vector<Pending> q;                    /* [head, size): queued bursts by radio_ts */
	size_t head = 0;
	bool window_set = false;
	int64_t rendered_end = 0;
	trxhip_ms_tx_status ctr{};
	trx_nco_state nco{};                       /* the uplink oscillator, on the radio_ts timeline of the windows */
	// ring rows (device objects only)
	std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> free_rows;   /* freed rows, lowest first */
	uint32_t fresh = 0;                        /* rows >= fresh were never used */
};

}  // namespace

// A trxhip_ms_tx * is the handle of a group of one member that issues directly (trxhip_ms_tx_create()); the type has no
// definition of its own.
struct trxhip_ms_tx_group {
	trxhip_ctx *ctx = nullptr;
	trxhip_ms_tx_cfg cfg{};                    /* of every member */
	bool nco_ok = false;                       /* the cast stays defined behind the oscillator at this tx_full_scale */
	bool direct = false;                       /* the single object: one member, rows copied straight into the ring, host-made segments */
	std::vector<Member> mem;

	// device state (ctx != NULL)
	trx_dev<trx_mstx_row> d_rows;              /* [n_members][max_pending] */
	trx_dev<uint8_t> d_stage[kBufs];           /* not with `direct` */
	trx_dev<uint8_t> d_tab[kBufs];
	int next_stage = 0;
	std::vector<uint32_t> call_dst;
	int next_tab = 0;
	// behind the device buffers: the calls that read those are waited for before they are freed
	PinBuf stage[kBufs];                       /* submit: the call's rows, then (not with `direct`) their ring destinations */
	PinBuf tab[kBufs];                         /* render: the member entries, then the bursts of their windows; `direct`: the segments */
};

namespace {

size_t pending(const Member &m) { return m.q.size() - m.head; }

// the buffer for a call that needs `bytes`: waits for the call that used it last, grows it when it is too small
int pin_acquire(PinBuf &b, size_t bytes)
{
	int rc = b.ev.create();
	if (rc == TRXHIP_OK)
		rc = b.ev.wait();
	return rc != TRXHIP_OK ? rc : b.h.reserve(std::max(bytes, (size_t)4096));
}

// submit_burst() for one request: everything but the queue
trxhip_ms_tx_plan plan_request(const Member &m, const trxhip_ms_tx_cfg &cfg, const trxhip_ms_tx_req &r, uint32_t now_fn, int now_tn,
			       int64_t now_ts)
{
	trxhip_ms_tx_plan p;
	memset(&p, 0, sizeof(p));
	// driveTx(), ms_upper.cpp:328, :336: int RSSI = (int)pwr; txFullScale * pow(10, -RSSI / 10) in double, complex(float)
	const int rssi = (int)r.pwr;
	p.scale = (float)((double)cfg.tx_full_scale * pow(10, -rssi / 10));

	GsmTime target = { (int)r.fn, (int)r.tn };
	target.incTN(3);                                           /* ul dl offset, ms.cpp:118 */
	const int target_fn = target.fn, target_tn = target.tn;
	const int32_t diff_fn = fn_delta(target_fn, (int32_t)now_fn);
	const int diff_tn = (target_tn - now_tn) % 8;
	GsmTime tosend = { diff_fn, 0 };
	if (diff_tn > 0)
		tosend.incTN((unsigned)diff_tn);
	else
		tosend.decTN((unsigned)-diff_tn);
	p.diff_fn = diff_fn;
	p.diff_tn = diff_tn;
	// :133 -- now_time.TN() is unsigned: target_tn - TN() wraps when target_tn < now_tn
	if (diff_fn < 0 || (diff_fn == 0 && ((unsigned)target_tn - (unsigned)now_tn < 3u))) {
		p.status = TRXHIP_MS_TX_LATE;
		return p;
	}
	// :139 -- ONE_TS_BURST_LEN is unsigned int: int * int, then * unsigned (modulo 2^32), widened by the int64 sum
	const unsigned one_ts = (unsigned)TRX_MSTX_BURST;
	p.send_ts = now_ts + (unsigned)(tosend.fn * 8) * one_ts + (unsigned)tosend.tn * one_ts - m.timing_advance;
	p.radio_ts = p.send_ts + cfg.rxtx_delay;                    /* submit_burst_ts(): ts + rxtxdelay */
	p.status = (diff_fn == 0 && target_tn < now_tn) ? TRXHIP_MS_TX_WRAPPED : TRXHIP_MS_TX_QUEUED;
	return p;
}

// where a burst at radio_ts goes in the queue, or -1: its samples intersect a queued burst's
ptrdiff_t queue_place(const Member &m, int64_t radio_ts)
{
	const auto first = m.q.begin() + (ptrdiff_t)m.head;
	const auto it = std::upper_bound(first, m.q.end(), radio_ts, [](int64_t t, const Pending &b) { return t < b.radio_ts; });
	if (it != first && (it - 1)->radio_ts + kBurst > radio_ts)
		return -1;
	if (it != m.q.end() && radio_ts + kBurst > it->radio_ts)
		return -1;
	return it - m.q.begin();
}

// One request against one member: the plan record, the status rules in their order, the counters and the queue.  True when the
// burst was queued; with_rows (a device object): *row is the ring row it takes.
bool place_request(Member &m, const trxhip_ms_tx_cfg &cfg, bool with_rows, const trxhip_ms_tx_req &r, uint32_t now_fn, int now_tn,
		   int64_t now_ts, trxhip_ms_tx_plan &p, uint32_t *row)
{
	p = plan_request(m, cfg, r, now_fn, now_tn, now_ts);
	m.ctr.submitted++;
	ptrdiff_t at = -1;
	if (p.status == TRXHIP_MS_TX_QUEUED) {
		if (m.window_set && p.radio_ts < m.rendered_end)
			p.status = TRXHIP_MS_TX_EXPIRED;
		else if ((at = queue_place(m, p.radio_ts)) < 0)
			p.status = TRXHIP_MS_TX_OVERLAP;
		else if (pending(m) >= cfg.max_pending)
			p.status = TRXHIP_MS_TX_FULL;
	}
	switch (p.status) {
	case TRXHIP_MS_TX_LATE: m.ctr.late++; return false;
	case TRXHIP_MS_TX_WRAPPED: m.ctr.wrapped++; return false;
	case TRXHIP_MS_TX_EXPIRED: m.ctr.expired++; return false;
	case TRXHIP_MS_TX_OVERLAP: m.ctr.overlap++; return false;
	case TRXHIP_MS_TX_FULL: m.ctr.full++; return false;
	default: break;
	}
	Pending b = { p.radio_ts, 0u, false };
	if (with_rows) {
		/* pending < max_pending: a freed row, or a row never used, exists */
		if (!m.free_rows.empty()) {
			b.row = m.free_rows.top();
			m.free_rows.pop();
		} else {
			b.row = m.fresh++;
		}
		*row = b.row;
	}
	m.q.insert(m.q.begin() + at, b);
	m.ctr.queued++;
	return true;
}

// what a queued burst is on the device
void fill_row(trx_mstx_row &row, const trxhip_ms_tx_req &r, float scale)
{
	memcpy(row.bits, r.bits, sizeof(row.bits));
	memset(row.pad, 0, sizeof(row.pad));
	row.scale = scale;
	row.reserved = 0;
}

void retire(Member &m, bool with_rows, const Pending &b, size_t *n_drawn)
{
	if (b.touched) {
		m.ctr.drawn++;
		if (n_drawn)
			(*n_drawn)++;
	} else {
		m.ctr.missed++;
	}
	if (with_rows)
		m.free_rows.push(b.row);
}

// The window [first_ts, end) of one member: retire what lies before it, hand every queued burst that has samples in it to
// on_burst(burst, from, to) -- [from, to) its stretch inside the window, in ascending order -- and retire what ends in it.
template <class F>
void walk_window(Member &m, bool with_rows, int64_t first_ts, int64_t end, size_t *n_drawn, const F &on_burst)
{
	while (m.head < m.q.size() && m.q[m.head].radio_ts + kBurst <= first_ts)       /* ended in the gap in front of the window */
		retire(m, with_rows, m.q[m.head++], n_drawn);
	while (m.head < m.q.size() && m.q[m.head].radio_ts < end) {
		Pending &b = m.q[m.head];
		on_burst(b, std::max(b.radio_ts, first_ts), std::min(b.radio_ts + kBurst, end));
		b.touched = true;
		if (b.radio_ts + kBurst > end)
			break;                                             /* crosses the window's end: the next render draws the rest */
		retire(m, with_rows, b, n_drawn);
		m.head++;
	}
	if (m.head > 4096 && m.head * 2 > m.q.size()) {
		m.q.erase(m.q.begin(), m.q.begin() + (ptrdiff_t)m.head);
		m.head = 0;
	}
	m.window_set = true;
	m.rendered_end = end;
}

// queued bursts that begin before `end`: no window that ends there meets more
size_t bursts_before(const Member &m, int64_t end)
{
	const auto first = m.q.begin() + (ptrdiff_t)m.head;
	return (size_t)(std::lower_bound(first, m.q.end(), end, [](const Pending &b, int64_t t) { return b.radio_ts < t; }) - first);
}

bool valid_request(const trxhip_ms_tx_req &r) { return r.tn <= 7 && r.fn < (uint32_t)kHyperframe; }

bool valid_clock(uint32_t now_fn, int now_tn, int64_t now_ts)
{
	return now_fn < (uint32_t)kHyperframe && now_tn >= 0 && now_tn <= 7 && now_ts >= -kMaxTs && now_ts <= kMaxTs;
}

bool valid_window(const Member &m, size_t n_samples, int64_t first_ts)
{
	return n_samples <= kMaxWindow && !(m.window_set && first_ts < m.rendered_end) && first_ts >= -kMaxTs && first_ts <= kMaxTs;
}

bool valid_ta(int val) { return val > -127 && val < 128; }         /* set_ta(), ms/ms.h:299-303 */

// the largest scale is tx_full_scale itself (pwr 0..9): the product with a modulator sample must stay below 32768, where
// static_cast<int16_t>(float) is defined
bool valid_cfg(const trxhip_ms_tx_cfg &c)
{
	return c.max_pending >= 1 && c.max_pending <= kMaxPending && (double)c.tx_full_scale * pulse_bound() < 32768.0;
}

// the rotated product must stay below 32768 too: nco_bound() in place of pulse_bound()
bool valid_nco_scale(const trxhip_ms_tx_cfg &c) { return (double)c.tx_full_scale * nco_bound() < 32768.0; }

// trxhip_ms_nco_tx_*_set for one member: at rendered_end, or 0 before the first window
int member_nco_set(Member &m, bool nco_ok, const trxhip_ms_nco_cfg *cfg)
{
	int32_t inc;
	if (!cfg || trx_nco_inc(cfg->hz, &inc) != 0 || (cfg->enable != 0 && !nco_ok))
		return TRXHIP_EINVAL;
	trx_nco_set(&m.nco, cfg->enable != 0, cfg->hz, inc, m.window_set ? m.rendered_end : 0);
	return TRXHIP_OK;
}

void member_nco_state(const Member &m, trxhip_ms_nco_status *out)
{
	memset(out, 0, sizeof(*out));
	out->enable = m.nco.enable;
	out->inc = m.nco.inc;
	out->acc = m.nco.acc;
	out->ts_ref = m.nco.ts_ref;
	out->hz = m.nco.hz;
}

// what a render that begins at first_ts hands the kernel for this member; off rides as the identity
trxhip_ms_nco_row member_nco_row(const Member &m, int64_t first_ts)
{
	if (!m.nco.enable)
		return trxhip_ms_nco_row{ 0u, 0 };
	return trxhip_ms_nco_row{ trx_nco_phase(m.nco.acc, m.nco.ts_ref, m.nco.inc, first_ts), m.nco.inc };
}

void member_state(const Member &m, trxhip_ms_tx_status *out)
{
	*out = m.ctr;
	out->pending = pending(m);
	out->rendered_end = m.window_set ? m.rendered_end : 0;
	out->timing_advance = m.timing_advance;
	out->window_set = m.window_set;
	memset(out->reserved, 0, sizeof(out->reserved));
}

// a device buffer of at least `bytes`, kept between calls
int dev_reserve(trx_dev<uint8_t> &d, size_t bytes) { return d.reserve(std::max(bytes, (size_t)4096)); }

// zeros over [from, to) of the window that starts at first_ts, in segments of at most 625 samples
size_t zero_segs(trx_mstx_seg *segs, size_t k, int64_t from, int64_t to, int64_t first_ts)
{
	for (int64_t t = from; t < to; t += kBurst, k++) {
		if (!segs)
			continue;
		trx_mstx_seg &g = segs[k];
		g.out_off = (uint32_t)(t - first_ts);
		g.src = TRX_MSTX_ZERO;
		g.len = (uint16_t)std::min(kBurst, to - t);
		g.first = 0;
		g.reserved = 0;
	}
	return k;
}

// The window [first_ts, end): retire what lies before it, tile it with segments (written when segs != NULL), retire what ends
// in it.  Returns the number of segments.
size_t plan_window(Member &m, bool with_rows, int64_t first_ts, int64_t end, trx_mstx_seg *segs, size_t *n_drawn)
{
	size_t k = 0;
	int64_t cur = first_ts;
	walk_window(m, with_rows, first_ts, end, n_drawn, [&](const Pending &b, int64_t from, int64_t to) {
		k = zero_segs(segs, k, cur, from, first_ts);
		if (segs) {
			trx_mstx_seg &g = segs[k];
			g.out_off = (uint32_t)(from - first_ts);
			g.src = b.row;
			g.len = (uint16_t)(to - from);
			g.first = (uint16_t)(from - b.radio_ts);
			g.reserved = 0;
		}
		k++;
		cur = to;
	});
	return zero_segs(segs, k, cur, end, first_ts);
}

// group_render() with `direct`: the one member's checked window of n_samples >= 1 as segments, one copy, one launch, one event
int render_segments(trxhip_ms_tx_group *g, int16_t *d_out, size_t n_samples, int64_t first_ts, size_t *n_drawn, hipStream_t st)
{
	Member &m = g->mem[0];
	const int64_t end = first_ts + (int64_t)n_samples;
	if (!g->ctx) {
		plan_window(m, false, first_ts, end, nullptr, n_drawn);
		return TRXHIP_OK;
	}
	if (with_device(g->ctx))
		return TRXHIP_EIO;
	// at most: a zero segment per 625 samples, and per queued burst that begins before the window's end the burst's segment and
	// one more zero segment in front of it
	const size_t bound = n_samples / (size_t)kBurst + 2 * bursts_before(m, end) + 2;
	const int k = g->next_tab;
	PinBuf &pb = g->tab[k];
	int rc = pin_acquire(pb, bound * sizeof(trx_mstx_seg));     /* waits for the render 4 calls back: it read d_tab[k] */
	if (rc == TRXHIP_OK)
		rc = dev_reserve(g->d_tab[k], bound * sizeof(trx_mstx_seg));
	if (rc != TRXHIP_OK)
		return rc;
	trx_mstx_seg *segs = reinterpret_cast<trx_mstx_seg *>(pb.h.p);
	const trx_mstx_seg *d_segs = reinterpret_cast<const trx_mstx_seg *>(g->d_tab[k].p);
	const trxhip_ms_nco_row nco = member_nco_row(m, first_ts);
	const size_t n_segs = plan_window(m, true, first_ts, end, segs, n_drawn);
	if (n_segs > bound)
		return TRXHIP_EIO;                                     /* cannot happen: see the bound */
	rc = hipMemcpyAsync(g->d_tab[k], segs, n_segs * sizeof(trx_mstx_seg), hipMemcpyHostToDevice, st) == hipSuccess ? TRXHIP_OK : TRXHIP_EIO;
	if (rc == TRXHIP_OK)
		rc = m.nco.enable ? trx_launch_ms_tx_render_nco(d_segs, n_segs, g->d_rows, g->ctx->d_tx_tables, d_out, nco, g->ctx->d_nco_tab, st)
				  : trx_launch_ms_tx_render(d_segs, n_segs, g->d_rows, g->ctx->d_tx_tables, d_out, st);
	if (rc == TRXHIP_OK)
		rc = pb.ev.record(st);
	if (rc != TRXHIP_OK) {
		(void)hipStreamSynchronize(st);
		return TRXHIP_EIO;
	}
	g->next_tab = (k + 1) % kBufs;
	return TRXHIP_OK;
}

// direct: the single object, which needs neither a scatter nor a table
int group_create(trxhip_ctx *ctx, const trxhip_ms_tx_cfg &c, size_t n_members, bool direct, trxhip_ms_tx_group **out)
{
	// a ring row is named by a uint32 over all members
	if (n_members < 1 || n_members > TRXHIP_MS_TX_GROUP_MAX_MEMBERS || !valid_cfg(c) || (uint64_t)n_members * c.max_pending > 0xffffffffull)
		return TRXHIP_EINVAL;
	if (ctx && (!ctx->d_tx_tables || with_device(ctx)))
		return TRXHIP_EINVAL;
	trxhip_ms_tx_group *g = new (std::nothrow) trxhip_ms_tx_group();
	if (!g)
		return TRXHIP_ENOMEM;
	g->cfg = c;
	g->cfg.reserved = 0;
	g->nco_ok = valid_nco_scale(c);
	g->direct = direct;
	try {
		g->mem.resize(n_members);
	} catch (const std::bad_alloc &) {
		delete g;
		return TRXHIP_ENOMEM;
	}
	if (ctx) {
		g->ctx = ctx;
		if (g->d_rows.alloc(n_members * c.max_pending) != TRXHIP_OK) {
			trxhip_ms_tx_group_destroy(g);
			return TRXHIP_ENOMEM;
		}
	}
	*out = g;
	return TRXHIP_OK;
}

trxhip_ms_tx_group *group_of(trxhip_ms_tx *s) { return reinterpret_cast<trxhip_ms_tx_group *>(s); }
const trxhip_ms_tx_group *group_of(const trxhip_ms_tx *s) { return reinterpret_cast<const trxhip_ms_tx_group *>(s); }

// n requests, all or nothing.  h_member == NULL: every request is member 0's (the single object).  The QUEUED rows are packed
// into a pinned buffer; a group sends them up in one copy with their ring destinations behind them and one launch scatters
// them, `direct` copies every run of consecutive ring rows to where it lies.
int group_submit(trxhip_ms_tx_group *g, const uint32_t *h_member, const trxhip_ms_tx_req *h_reqs, size_t n, const trxhip_ms_tx_clock *h_now,
		 trxhip_ms_tx_plan *h_plan, size_t *bad, void *stream)
{
	if (bad)
		*bad = (size_t)-1;
	if (!g || ((!h_reqs || !h_now) && n))
		return TRXHIP_EINVAL;
	for (size_t i = 0; i < n; i++) {
		const uint32_t mi = h_member ? h_member[i] : 0;
		const bool ok = mi < g->mem.size() && valid_request(h_reqs[i]) && valid_clock(h_now[mi].fn, h_now[mi].tn, h_now[mi].ts);
		if (!ok) {
			if (bad)
				*bad = i;
			return TRXHIP_EINVAL;
		}
	}
	if (n == 0)
		return TRXHIP_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	const bool dev = g->ctx != nullptr;
	const size_t ring = g->mem.size() * (size_t)g->cfg.max_pending;
	const size_t most = std::min(n, ring);                         /* no call queues more */
	const size_t per_row = sizeof(trx_mstx_row) + (g->direct ? 0 : sizeof(uint32_t));
	const int k = g->next_stage;
	PinBuf &pb = g->stage[k];
	if (dev) {
		if (with_device(g->ctx))
			return TRXHIP_EIO;
		int rc = pin_acquire(pb, most * per_row);                  /* waits for the submit 4 calls back: its copies read the buffer */
		if (rc == TRXHIP_OK && !g->direct)
			rc = dev_reserve(g->d_stage[k], most * per_row);
		if (rc != TRXHIP_OK)
			return rc;
	}
	trx_mstx_row *rows = reinterpret_cast<trx_mstx_row *>(pb.h.p);
	std::vector<uint32_t> &call_dst = g->call_dst;                 /* a group's go behind the rows once their number is known */
	call_dst.clear();
	size_t nq = 0;
	for (size_t i = 0; i < n; i++) {
		const uint32_t mi = h_member ? h_member[i] : 0;
		const trxhip_ms_tx_clock &now = h_now[mi];
		trxhip_ms_tx_plan p;
		uint32_t ring_row = 0;
		if (place_request(g->mem[mi], g->cfg, dev, h_reqs[i], now.fn, now.tn, now.ts, p, &ring_row) && dev) {
			fill_row(rows[nq++], h_reqs[i], p.scale);
			call_dst.push_back(mi * g->cfg.max_pending + ring_row);
		}
		if (h_plan)
			h_plan[i] = p;
	}
	if (!dev || nq == 0)
		return TRXHIP_OK;
	int rc = TRXHIP_OK;
	if (g->direct) {
		// one copy per run of consecutive ring rows: one per call while the free rows are not fragmented
		for (size_t i = 0, j; i < nq && rc == TRXHIP_OK; i = j) {
			j = i + 1;
			while (j < nq && call_dst[j] == call_dst[j - 1] + 1)
				j++;
			if (hipMemcpyAsync(g->d_rows + call_dst[i], rows + i, (j - i) * sizeof(trx_mstx_row), hipMemcpyHostToDevice, st) != hipSuccess)
				rc = TRXHIP_EIO;
		}
	} else {
		memcpy(rows + nq, call_dst.data(), nq * sizeof(uint32_t));
		if (hipMemcpyAsync(g->d_stage[k], pb.h, nq * per_row, hipMemcpyHostToDevice, st) != hipSuccess)
			rc = TRXHIP_EIO;
		if (rc == TRXHIP_OK)
			rc = trx_launch_ms_tx_stage(reinterpret_cast<const trx_mstx_row *>(g->d_stage[k].p),
						    reinterpret_cast<const uint32_t *>(g->d_stage[k] + nq * sizeof(trx_mstx_row)), nq, g->d_rows, ring, st);
	}
	if (rc == TRXHIP_OK)
		rc = pb.ev.record(st);
	if (rc != TRXHIP_OK) {
		(void)hipStreamSynchronize(st);
		return TRXHIP_EIO;
	}
	g->next_stage = (k + 1) % kBufs;
	return TRXHIP_OK;
}

// Every member's window, all or nothing: one table (`direct`: the one member's segments), one copy, one launch, one event, for a
// group of any size.
int group_render(trxhip_ms_tx_group *g, int16_t *d_out, size_t out_stride, const int64_t *h_first_ts, const size_t *h_n_samples,
		 size_t *h_n_drawn, int *bad_member, void *stream)
{
	if (bad_member)
		*bad_member = -1;
	if (!g || !h_first_ts || !h_n_samples)
		return TRXHIP_EINVAL;
	const bool dev = g->ctx != nullptr;
	if (dev ? (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 3)) : d_out != nullptr)
		return TRXHIP_EINVAL;
	const size_t n_mem = g->mem.size();
	// every member's window, before anything moves; a plan-only group with out_stride 0 has no output to bound
	size_t n_rendered = 0, n_bursts = 0;
	uint64_t n_waves = 0;
	for (size_t m = 0; m < n_mem; m++) {
		const size_t ns = h_n_samples[m];
		if (ns == 0)
			continue;
		if (!valid_window(g->mem[m], ns, h_first_ts[m]) || ((dev || out_stride) && ns > out_stride)) {
			if (bad_member)
				*bad_member = (int)m;
			return TRXHIP_EINVAL;
		}
		n_rendered++;
		n_waves += (ns + TRX_MSTX_BURST - 1) / TRX_MSTX_BURST;
		n_bursts += bursts_before(g->mem[m], h_first_ts[m] + (int64_t)ns);
	}
	if (n_waves > 0x7fffffffull || n_bursts > 0xffffffffull)
		return TRXHIP_EINVAL;
	if (h_n_drawn)
		memset(h_n_drawn, 0, n_mem * sizeof(size_t));
	if (n_rendered == 0)
		return TRXHIP_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (g->direct)
		return render_segments(g, d_out, h_n_samples[0], h_first_ts[0], h_n_drawn, st);
	const int k = g->next_tab;
	PinBuf &pb = g->tab[k];
	if (dev) {
		if (with_device(g->ctx))
			return TRXHIP_EIO;
		const size_t bytes = n_rendered * sizeof(trx_mstx_gmember) + n_bursts * sizeof(trx_mstx_gburst);
		int rc = pin_acquire(pb, bytes);                           /* waits for the render 4 calls back: it read d_tab[k] */
		if (rc == TRXHIP_OK)
			rc = dev_reserve(g->d_tab[k], bytes);
		if (rc != TRXHIP_OK)
			return rc;
	}
	trx_mstx_gmember *ent = reinterpret_cast<trx_mstx_gmember *>(pb.h.p);
	trx_mstx_gburst *bur = dev ? reinterpret_cast<trx_mstx_gburst *>(ent + n_rendered) : nullptr;
	size_t ke = 0, kb = 0;
	uint32_t wave = 0;
	bool nco_on = false;                                           /* a rendered member has its oscillator on */
	for (size_t m = 0; m < n_mem; m++) {
		const size_t ns = h_n_samples[m];
		if (ns == 0)
			continue;
		const int64_t first_ts = h_first_ts[m];
		const size_t kb0 = kb;
		walk_window(g->mem[m], dev, first_ts, first_ts + (int64_t)ns, h_n_drawn ? h_n_drawn + m : nullptr,
			    [&](const Pending &b, int64_t, int64_t) {
				    if (dev) {
					    bur[kb].rel = (int32_t)(b.radio_ts - first_ts);      /* -624 .. ns - 1: it has samples in the window */
					    bur[kb].row = (uint32_t)m * g->cfg.max_pending + b.row;
				    }
				    kb++;
			    });
		if (dev) {
			trx_mstx_gmember &e = ent[ke];
			e.out_off = (uint64_t)m * out_stride;
			e.n_samples = (uint32_t)ns;
			e.first_wave = wave;
			e.first_burst = (uint32_t)kb0;
			e.n_bursts = (uint32_t)(kb - kb0);
			const trxhip_ms_nco_row nco = member_nco_row(g->mem[m], first_ts);
			e.nco_phase0 = nco.phase0;
			e.nco_inc = nco.inc;
			nco_on = nco_on || g->mem[m].nco.enable;
		}
		ke++;
		wave += (uint32_t)((ns + TRX_MSTX_BURST - 1) / TRX_MSTX_BURST);
	}
	if (!dev)
		return TRXHIP_OK;
	if (ke != n_rendered || kb > n_bursts || wave != (uint32_t)n_waves)
		return TRXHIP_EIO;                                     /* cannot happen: see the bounds */
	// the bursts stand right behind the entries: the table is one piece whatever kb is
	int rc = hipMemcpyAsync(g->d_tab[k], pb.h, n_rendered * sizeof(trx_mstx_gmember) + kb * sizeof(trx_mstx_gburst), hipMemcpyHostToDevice,
				st) == hipSuccess
			 ? TRXHIP_OK
			 : TRXHIP_EIO;
	if (rc == TRXHIP_OK)
		rc = nco_on ? trx_launch_ms_tx_render_group_nco(reinterpret_cast<const trx_mstx_gmember *>(g->d_tab[k].p), (uint32_t)n_rendered, wave,
								g->d_rows, g->ctx->d_tx_tables, d_out, g->ctx->d_nco_tab, st)
			    : trx_launch_ms_tx_render_group(reinterpret_cast<const trx_mstx_gmember *>(g->d_tab[k].p), (uint32_t)n_rendered, wave,
							    g->d_rows, g->ctx->d_tx_tables, d_out, st);
	if (rc == TRXHIP_OK)
		rc = pb.ev.record(st);
	if (rc != TRXHIP_OK) {
		(void)hipStreamSynchronize(st);
		return TRXHIP_EIO;
	}
	g->next_tab = (k + 1) % kBufs;
	return TRXHIP_OK;
}

}  // namespace

extern "C" {

// ---- the group: N members, their submits and their renders each issued as one step ----

int trxhip_ms_tx_group_create(trxhip_ctx *ctx, const trxhip_ms_tx_group_cfg *cfg, trxhip_ms_tx_group **out)
{
	if (!cfg || !out)
		return TRXHIP_EINVAL;
	return group_create(ctx, trxhip_ms_tx_cfg{ cfg->tx_full_scale, cfg->rxtx_delay, cfg->max_pending, 0 }, cfg->n_members, false, out);
}

void trxhip_ms_tx_group_destroy(trxhip_ms_tx_group *g)
{
	if (!g)
		return;
	if (g->ctx)
		(void)with_device(g->ctx);
	delete g;
}

int trxhip_ms_tx_group_size(const trxhip_ms_tx_group *g)
{
	return g ? (int)g->mem.size() : TRXHIP_EINVAL;
}

int trxhip_ms_tx_group_set_ta(trxhip_ms_tx_group *g, uint32_t member, int val)
{
	if (!g || member >= g->mem.size() || !valid_ta(val))
		return TRXHIP_EINVAL;
	g->mem[member].timing_advance = val * 4;
	return TRXHIP_OK;
}

int trxhip_ms_tx_group_submit(trxhip_ms_tx_group *g, const uint32_t *h_member, const trxhip_ms_tx_req *h_reqs, size_t n,
			      const trxhip_ms_tx_clock *h_now, trxhip_ms_tx_plan *h_plan, size_t *bad, void *stream)
{
	if (!h_member && n) {
		if (bad)
			*bad = (size_t)-1;
		return TRXHIP_EINVAL;
	}
	return group_submit(g, h_member, h_reqs, n, h_now, h_plan, bad, stream);
}

int trxhip_ms_tx_group_render_s16(trxhip_ms_tx_group *g, int16_t *d_out, size_t out_stride, const int64_t *h_first_ts,
				  const size_t *h_n_samples, size_t *h_n_drawn, int *bad_member, void *stream)
{
	return group_render(g, d_out, out_stride, h_first_ts, h_n_samples, h_n_drawn, bad_member, stream);
}

int trxhip_ms_tx_group_state(const trxhip_ms_tx_group *g, uint32_t member, trxhip_ms_tx_status *out)
{
	if (!g || member >= g->mem.size() || !out)
		return TRXHIP_EINVAL;
	member_state(g->mem[member], out);
	return TRXHIP_OK;
}

int trxhip_ms_nco_tx_group_set(trxhip_ms_tx_group *g, uint32_t member, const trxhip_ms_nco_cfg *cfg)
{
	return g && member < g->mem.size() ? member_nco_set(g->mem[member], g->nco_ok, cfg) : TRXHIP_EINVAL;
}

int trxhip_ms_nco_tx_group_state(const trxhip_ms_tx_group *g, uint32_t member, trxhip_ms_nco_status *out)
{
	if (!g || member >= g->mem.size() || !out)
		return TRXHIP_EINVAL;
	member_nco_state(g->mem[member], out);
	return TRXHIP_OK;
}

// ---- the single object: member 0 of a group of one that issues directly ----

int trxhip_ms_tx_create(trxhip_ctx *ctx, const trxhip_ms_tx_cfg *cfg, trxhip_ms_tx **out)
{
	return cfg && out ? group_create(ctx, *cfg, 1, true, reinterpret_cast<trxhip_ms_tx_group **>(out)) : TRXHIP_EINVAL;
}

void trxhip_ms_tx_destroy(trxhip_ms_tx *s) { trxhip_ms_tx_group_destroy(group_of(s)); }

int trxhip_ms_tx_set_ta(trxhip_ms_tx *s, int val) { return trxhip_ms_tx_group_set_ta(group_of(s), 0, val); }

int trxhip_ms_tx_state(const trxhip_ms_tx *s, trxhip_ms_tx_status *out) { return trxhip_ms_tx_group_state(group_of(s), 0, out); }

int trxhip_ms_nco_tx_set(trxhip_ms_tx *s, const trxhip_ms_nco_cfg *cfg) { return trxhip_ms_nco_tx_group_set(group_of(s), 0, cfg); }

int trxhip_ms_nco_tx_state(const trxhip_ms_tx *s, trxhip_ms_nco_status *out) { return trxhip_ms_nco_tx_group_state(group_of(s), 0, out); }

// the one clock is h_now[0], read even when there is no request
int trxhip_ms_tx_submit(trxhip_ms_tx *s, const trxhip_ms_tx_req *h_reqs, size_t n, uint32_t now_fn, int now_tn, int64_t now_ts,
			trxhip_ms_tx_plan *h_plan, void *stream)
{
	if (!valid_clock(now_fn, now_tn, now_ts))
		return TRXHIP_EINVAL;
	const trxhip_ms_tx_clock now = { now_fn, now_tn, now_ts };
	return group_submit(group_of(s), nullptr, h_reqs, n, &now, h_plan, nullptr, stream);
}

// The one window as arrays of length one, its stride its length.  A window of no samples is checked here: the group skips a
// member with none unchecked.
int trxhip_ms_tx_render_s16(trxhip_ms_tx *s, int16_t *d_out, size_t n_samples, int64_t first_ts, size_t *n_drawn, void *stream)
{
	if (!s || !valid_window(group_of(s)->mem[0], n_samples, first_ts))
		return TRXHIP_EINVAL;
	return group_render(group_of(s), d_out, n_samples, &first_ts, &n_samples, n_drawn, nullptr, stream);
}

}  // extern "C"
