// trx_ms_tx.cpp -- the MS-side uplink burst scheduler: burst requests in, the radio's transmit sample stream out.
//
// The host half restates what the reference decides per burst request:
//   upper_trx::driveTx()          ms/ms_upper.cpp:306-355   (the power scale; modulate, scale, int16)
//   ms_trx::submit_burst()        ms/ms.cpp:114-160         (target FN/TN, timekeeper, timing advance -> send_ts; "TX too late")
//   ms_trx::set_ta()              ms/ms.h:299-303
//   submit_burst_ts()             ms/uhd_specific.h:260-269, ms/bladerf_specific.h:461-478   (ts + rxtxdelay)
//   GSM::Time::incTN / decTN      GSM/GSMCommon.h:129-150;  GSM::FNDelta  GSM/GSMCommon.cpp:71-78
// keeps the queued bursts ordered by the timestamp of their first sample, and turns a window of the stream into segments:
// stretches of queued bursts and zeros in between, at most 625 samples each, that tile the window.  The device half
// (trx_tx.hip, ms_tx_render_kernel) draws every segment where it lies.  With ctx == NULL the object is plan-only: the same
// arithmetic and queue, no device memory.
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
#include "trx_ms_tx.h"

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
	uint8_t *h = nullptr;
	size_t cap = 0;            /* bytes */
	hipEvent_t ev = nullptr;
	bool used = false;
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

}  // namespace

struct trxhip_ms_tx {
	trxhip_ctx *ctx = nullptr;
	trxhip_ms_tx_cfg cfg{};
	int32_t timing_advance = 0;
	std::vector<Pending> q;                    /* [head, size): queued bursts by radio_ts */
	size_t head = 0;
	bool window_set = false;
	int64_t rendered_end = 0;
	trxhip_ms_tx_status ctr{};

	// device state (ctx != NULL)
	trx_mstx_row *d_rows = nullptr;
	std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> free_rows;   /* freed rows, lowest first */
	uint32_t fresh = 0;                        /* rows >= fresh were never used */
	PinBuf stage[kBufs];                       /* submit: the call's rows */
	int next_stage = 0;
	PinBuf seg[kBufs];                         /* render: the window's segments */
	trx_mstx_seg *d_seg[kBufs] = {};
	size_t d_seg_cap[kBufs] = {};
	int next_seg = 0;
	std::vector<uint32_t> call_rows;
};

namespace {

size_t pending(const trxhip_ms_tx *s) { return s->q.size() - s->head; }

// the buffer for a call that needs `bytes`: waits for the call that used it last, grows it when it is too small
int pin_acquire(PinBuf &b, size_t bytes)
{
	if (!b.ev && hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess) {
		b.ev = nullptr;
		return TRXHIP_ENOMEM;
	}
	if (b.used) {
		if (hipEventSynchronize(b.ev) != hipSuccess)
			return TRXHIP_EIO;
		b.used = false;
	}
	if (b.cap < bytes) {
		if (b.h)
			(void)hipHostFree(b.h);
		b.h = nullptr;
		b.cap = 0;
		const size_t cap = std::max(bytes, (size_t)4096);
		if (hipHostMalloc(reinterpret_cast<void **>(&b.h), cap, hipHostMallocDefault) != hipSuccess) {
			b.h = nullptr;
			return TRXHIP_ENOMEM;
		}
		b.cap = cap;
	}
	return TRXHIP_OK;
}

void pin_destroy(PinBuf &b)
{
	if (b.used)
		(void)hipEventSynchronize(b.ev);
	if (b.ev)
		(void)hipEventDestroy(b.ev);
	if (b.h)
		(void)hipHostFree(b.h);
}

// submit_burst() for one request: everything but the queue
trxhip_ms_tx_plan plan_request(const trxhip_ms_tx *s, const trxhip_ms_tx_req &r, uint32_t now_fn, int now_tn, int64_t now_ts)
{
	trxhip_ms_tx_plan p;
	memset(&p, 0, sizeof(p));
	// driveTx(), ms_upper.cpp:328, :336: int RSSI = (int)pwr; txFullScale * pow(10, -RSSI / 10) in double, complex(float)
	const int rssi = (int)r.pwr;
	p.scale = (float)((double)s->cfg.tx_full_scale * pow(10, -rssi / 10));

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
	p.send_ts = now_ts + (unsigned)(tosend.fn * 8) * one_ts + (unsigned)tosend.tn * one_ts - s->timing_advance;
	p.radio_ts = p.send_ts + s->cfg.rxtx_delay;                 /* submit_burst_ts(): ts + rxtxdelay */
	p.status = (diff_fn == 0 && target_tn < now_tn) ? TRXHIP_MS_TX_WRAPPED : TRXHIP_MS_TX_QUEUED;
	return p;
}

// where a burst at radio_ts goes in the queue, or -1: its samples intersect a queued burst's
ptrdiff_t queue_place(const trxhip_ms_tx *s, int64_t radio_ts)
{
	const auto first = s->q.begin() + (ptrdiff_t)s->head;
	const auto it = std::upper_bound(first, s->q.end(), radio_ts, [](int64_t t, const Pending &b) { return t < b.radio_ts; });
	if (it != first && (it - 1)->radio_ts + kBurst > radio_ts)
		return -1;
	if (it != s->q.end() && radio_ts + kBurst > it->radio_ts)
		return -1;
	return it - s->q.begin();
}

void retire(trxhip_ms_tx *s, const Pending &b, size_t *n_drawn)
{
	if (b.touched) {
		s->ctr.drawn++;
		if (n_drawn)
			(*n_drawn)++;
	} else {
		s->ctr.missed++;
	}
	if (s->ctx)
		s->free_rows.push(b.row);
}

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
size_t plan_window(trxhip_ms_tx *s, int64_t first_ts, int64_t end, trx_mstx_seg *segs, size_t *n_drawn)
{
	while (s->head < s->q.size() && s->q[s->head].radio_ts + kBurst <= first_ts)       /* ended in the gap in front of the window */
		retire(s, s->q[s->head++], n_drawn);
	size_t k = 0;
	int64_t cur = first_ts;
	while (s->head < s->q.size() && s->q[s->head].radio_ts < end) {
		Pending &b = s->q[s->head];
		const int64_t from = std::max(b.radio_ts, first_ts), to = std::min(b.radio_ts + kBurst, end);
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
		b.touched = true;
		if (b.radio_ts + kBurst > end)
			break;                                             /* crosses the window's end: the next render draws the rest */
		retire(s, b, n_drawn);
		s->head++;
	}
	k = zero_segs(segs, k, cur, end, first_ts);
	if (s->head > 4096 && s->head * 2 > s->q.size()) {
		s->q.erase(s->q.begin(), s->q.begin() + (ptrdiff_t)s->head);
		s->head = 0;
	}
	s->window_set = true;
	s->rendered_end = end;
	return k;
}

}  // namespace

extern "C" {

int trxhip_ms_tx_create(trxhip_ctx *ctx, const trxhip_ms_tx_cfg *cfg, trxhip_ms_tx **out)
{
	if (!cfg || !out)
		return TRXHIP_EINVAL;
	const trxhip_ms_tx_cfg c = *cfg;
	if (c.max_pending < 1 || c.max_pending > kMaxPending)
		return TRXHIP_EINVAL;
	// the largest scale is tx_full_scale itself (pwr 0..9): the product with a modulator sample must stay below 32768, where
	// static_cast<int16_t>(float) is defined
	if (!((double)c.tx_full_scale * pulse_bound() < 32768.0))
		return TRXHIP_EINVAL;
	if (ctx && (!ctx->d_tx_tables || with_device(ctx)))
		return TRXHIP_EINVAL;
	trxhip_ms_tx *s = new (std::nothrow) trxhip_ms_tx();
	if (!s)
		return TRXHIP_ENOMEM;
	s->cfg = c;
	s->cfg.reserved = 0;
	if (ctx) {
		s->ctx = ctx;
		if (hipMalloc(reinterpret_cast<void **>(&s->d_rows), (size_t)c.max_pending * sizeof(trx_mstx_row)) != hipSuccess) {
			s->d_rows = nullptr;
			trxhip_ms_tx_destroy(s);
			return TRXHIP_ENOMEM;
		}
	}
	*out = s;
	return TRXHIP_OK;
}

void trxhip_ms_tx_destroy(trxhip_ms_tx *s)
{
	if (!s)
		return;
	if (s->ctx && with_device(s->ctx) == 0) {
		for (int k = 0; k < kBufs; k++) {
			pin_destroy(s->stage[k]);
			pin_destroy(s->seg[k]);
			if (s->d_seg[k])
				(void)hipFree(s->d_seg[k]);
		}
		if (s->d_rows)
			(void)hipFree(s->d_rows);
	}
	delete s;
}

int trxhip_ms_tx_set_ta(trxhip_ms_tx *s, int val)
{
	if (!s || !(val > -127 && val < 128))                      /* set_ta(), ms/ms.h:299-303 */
		return TRXHIP_EINVAL;
	s->timing_advance = val * 4;
	return TRXHIP_OK;
}

int trxhip_ms_tx_submit(trxhip_ms_tx *s, const trxhip_ms_tx_req *h_reqs, size_t n, uint32_t now_fn, int now_tn, int64_t now_ts,
			trxhip_ms_tx_plan *h_plan, void *stream)
{
	if (!s || (!h_reqs && n) || now_fn >= (uint32_t)kHyperframe || now_tn < 0 || now_tn > 7 || now_ts < -kMaxTs || now_ts > kMaxTs)
		return TRXHIP_EINVAL;
	for (size_t i = 0; i < n; i++)
		if (h_reqs[i].tn > 7 || h_reqs[i].fn >= (uint32_t)kHyperframe)
			return TRXHIP_EINVAL;
	if (n == 0)
		return TRXHIP_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	trx_mstx_row *rows = nullptr;
	PinBuf *pb = nullptr;
	if (s->ctx) {
		if (with_device(s->ctx))
			return TRXHIP_EIO;
		pb = &s->stage[s->next_stage];
		const size_t most = std::min(n, (size_t)s->cfg.max_pending);          /* no call queues more */
		const int rc = pin_acquire(*pb, most * sizeof(trx_mstx_row));
		if (rc != TRXHIP_OK)
			return rc;
		rows = reinterpret_cast<trx_mstx_row *>(pb->h);
		s->call_rows.clear();
	}
	for (size_t i = 0; i < n; i++) {
		const trxhip_ms_tx_req &r = h_reqs[i];
		trxhip_ms_tx_plan p = plan_request(s, r, now_fn, now_tn, now_ts);
		s->ctr.submitted++;
		ptrdiff_t at = -1;
		if (p.status == TRXHIP_MS_TX_QUEUED) {
			if (s->window_set && p.radio_ts < s->rendered_end)
				p.status = TRXHIP_MS_TX_EXPIRED;
			else if ((at = queue_place(s, p.radio_ts)) < 0)
				p.status = TRXHIP_MS_TX_OVERLAP;
			else if (pending(s) >= s->cfg.max_pending)
				p.status = TRXHIP_MS_TX_FULL;
		}
		switch (p.status) {
		case TRXHIP_MS_TX_LATE: s->ctr.late++; break;
		case TRXHIP_MS_TX_WRAPPED: s->ctr.wrapped++; break;
		case TRXHIP_MS_TX_EXPIRED: s->ctr.expired++; break;
		case TRXHIP_MS_TX_OVERLAP: s->ctr.overlap++; break;
		case TRXHIP_MS_TX_FULL: s->ctr.full++; break;
		default: {
			Pending b = { p.radio_ts, 0u, false };
			if (s->ctx) {
				/* pending < max_pending: a freed row, or a row never used, exists */
				if (!s->free_rows.empty()) {
					b.row = s->free_rows.top();
					s->free_rows.pop();
				} else {
					b.row = s->fresh++;
				}
				trx_mstx_row &row = rows[s->call_rows.size()];
				memcpy(row.bits, r.bits, sizeof(row.bits));
				memset(row.pad, 0, sizeof(row.pad));
				row.scale = p.scale;
				row.reserved = 0;
				s->call_rows.push_back(b.row);
			}
			s->q.insert(s->q.begin() + at, b);
			s->ctr.queued++;
			break;
		}
		}
		if (h_plan)
			h_plan[i] = p;
	}
	if (s->ctx && !s->call_rows.empty()) {
		// one copy per run of consecutive ring rows
		const std::vector<uint32_t> &cr = s->call_rows;
		for (size_t i = 0; i < cr.size();) {
			size_t j = i + 1;
			while (j < cr.size() && cr[j] == cr[j - 1] + 1)
				j++;
			if (hipMemcpyAsync(s->d_rows + cr[i], rows + i, (j - i) * sizeof(trx_mstx_row), hipMemcpyHostToDevice, st) != hipSuccess) {
				(void)hipStreamSynchronize(st);
				return TRXHIP_EIO;
			}
			i = j;
		}
		if (hipEventRecord(pb->ev, st) != hipSuccess) {
			(void)hipStreamSynchronize(st);
			return TRXHIP_EIO;
		}
		pb->used = true;
		s->next_stage = (s->next_stage + 1) % kBufs;
	}
	return TRXHIP_OK;
}

int trxhip_ms_tx_render_s16(trxhip_ms_tx *s, int16_t *d_out, size_t n_samples, int64_t first_ts, size_t *n_drawn, void *stream)
{
	if (!s || n_samples > kMaxWindow || (s->window_set && first_ts < s->rendered_end) || first_ts < -kMaxTs || first_ts > kMaxTs)
		return TRXHIP_EINVAL;
	if (s->ctx ? (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 3)) : d_out != nullptr)
		return TRXHIP_EINVAL;
	if (n_drawn)
		*n_drawn = 0;
	if (n_samples == 0)
		return TRXHIP_OK;
	const int64_t end = first_ts + (int64_t)n_samples;
	if (!s->ctx) {
		plan_window(s, first_ts, end, nullptr, n_drawn);
		return TRXHIP_OK;
	}
	if (with_device(s->ctx))
		return TRXHIP_EIO;
	hipStream_t st = static_cast<hipStream_t>(stream);
	// at most: a zero segment per 625 samples, and per queued burst that begins before the window's end the burst's segment and
	// one more zero segment in front of it
	const auto first = s->q.begin() + (ptrdiff_t)s->head;
	const size_t nb = (size_t)(std::lower_bound(first, s->q.end(), end, [](const Pending &b, int64_t t) { return b.radio_ts < t; }) - first);
	const size_t bound = n_samples / (size_t)kBurst + 2 * nb + 2;
	const int k = s->next_seg;
	PinBuf &pb = s->seg[k];
	int rc = pin_acquire(pb, bound * sizeof(trx_mstx_seg));     /* waits for the render 4 calls back: it read d_seg[k] */
	if (rc != TRXHIP_OK)
		return rc;
	if (s->d_seg_cap[k] < bound) {
		if (s->d_seg[k])
			(void)hipFree(s->d_seg[k]);
		s->d_seg[k] = nullptr;
		s->d_seg_cap[k] = 0;
		const size_t cap = std::max(bound, (size_t)256);
		if (hipMalloc(reinterpret_cast<void **>(&s->d_seg[k]), cap * sizeof(trx_mstx_seg)) != hipSuccess) {
			s->d_seg[k] = nullptr;
			return TRXHIP_ENOMEM;
		}
		s->d_seg_cap[k] = cap;
	}
	trx_mstx_seg *segs = reinterpret_cast<trx_mstx_seg *>(pb.h);
	const size_t n_segs = plan_window(s, first_ts, end, segs, n_drawn);
	if (n_segs > bound)
		return TRXHIP_EIO;                                     /* cannot happen: see the bound */
	rc = hipMemcpyAsync(s->d_seg[k], segs, n_segs * sizeof(trx_mstx_seg), hipMemcpyHostToDevice, st) == hipSuccess ? TRXHIP_OK : TRXHIP_EIO;
	if (rc == TRXHIP_OK)
		rc = trx_launch_ms_tx_render(s->d_seg[k], n_segs, s->d_rows, s->ctx->d_tx_tables, d_out, st);
	if (rc == TRXHIP_OK && hipEventRecord(pb.ev, st) != hipSuccess)
		rc = TRXHIP_EIO;
	if (rc != TRXHIP_OK) {
		(void)hipStreamSynchronize(st);
		return TRXHIP_EIO;
	}
	pb.used = true;
	s->next_seg = (k + 1) % kBufs;
	return TRXHIP_OK;
}

int trxhip_ms_tx_state(const trxhip_ms_tx *s, trxhip_ms_tx_status *out)
{
	if (!s || !out)
		return TRXHIP_EINVAL;
	*out = s->ctr;
	out->pending = pending(s);
	out->rendered_end = s->window_set ? s->rendered_end : 0;
	out->timing_advance = s->timing_advance;
	out->window_set = s->window_set;
	memset(out->reserved, 0, sizeof(out->reserved));
	return TRXHIP_OK;
}

}  // extern "C"
