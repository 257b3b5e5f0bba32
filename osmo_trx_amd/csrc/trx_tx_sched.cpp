// trx_tx_sched.cpp -- the downlink burst scheduler: TRXD datagrams in, each channel's transmit sample stream out.
//
// The host half restates what the reference decides per channel and timeslot of the transmit clock:
//   Transceiver::driveTxPriorityQueue()        Transceiver.cpp:1087-1185   (submit: length, version, FN order)
//   Transceiver::pushRadioVector()             Transceiver.cpp:416-481     (render: stale, current, filler, zeros)
//   Transceiver::updateFillerTable()           Transceiver.cpp:403-414
//   Transceiver::setModulus()                  Transceiver.cpp:483-512     (SETSLOT, :1047-1048)
//   TransceiverState::init() / the filler set-up  Transceiver.cpp:95-135, :218-219, :255-256
//   VectorQueue::getStaleBurst / getCurrentBurst  radioVector.cpp:124-148, ordered by GSM::Time (GSMCommon.h:187-215)
// and writes a plan: per channel and slot, a staged datagram row, a filler-table descriptor or zeros.  The device half
// (trx_tx.hip, tx_render_kernel) modulates every slot straight into its place of the stream.  With ctx == NULL the object
// is plan-only: the same queue logic, no device memory, the plan read back with trxhip_tx_sched_plan().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_tx_sched.h"

namespace {

const uint32_t kHyperframe = 2715648;       /* GSM::gHyperframe */
const int kBufs = 4;                         /* slot-word buffers (pinned + device) in flight: a render waits for the 4th before */

// GSM::FNDelta / FNCompare, GSMCommon.cpp:71-86
int32_t fn_delta(int32_t v1, int32_t v2)
{
	const int32_t half = (int32_t)kHyperframe / 2;
	int32_t d = v1 - v2;
	if (d >= half)
		d -= (int32_t)kHyperframe;
	else if (d < -half)
		d += (int32_t)kHyperframe;
	return d;
}

// GSM::Time::operator< (GSMCommon.h:187-191)
bool time_less(uint32_t fn1, int tn1, uint32_t fn2, int tn2)
{
	if (fn1 == fn2)
		return tn1 < tn2;
	return fn_delta((int32_t)fn1, (int32_t)fn2) < 0;
}

struct QItem {
	uint32_t fn;
	int tn;
	int64_t id;           /* submission id: the order of submission */
	int32_t row;          /* staging row (-1: plan-only) */
	uint16_t nbits;
	uint8_t flags;
	float att_scale;
};

// min-heap order: GSM::Time, then the earlier submission (the documented rule for duplicate times)
struct QLater {
	bool operator()(const QItem &a, const QItem &b) const
	{
		if (a.fn == b.fn && a.tn == b.tn)
			return a.id > b.id;
		return time_less(b.fn, b.tn, a.fn, a.tn);
	}
};

struct FillMirror {
	int64_t writer = -1;  /* submission id of the burst that wrote the entry, -1: the initial filler */
	int32_t row = -1;     /* >= 0: written during the current render, its bits still in this staging row */
	QItem item{};
};

struct Chan {
	std::vector<QItem> q;                   /* heap, QLater */
	FillMirror fill[TRX_TXS_ENTRIES];        /* [modFN * 8 + TN] */
	int chan_type[8];
	int modulus[8];
	bool muted = false, retrans = false;
	int filler = TRXHIP_FILLER_ZERO;
	bool first_dl[8] = {};
	uint32_t last_dl_fn[8] = {};
	trxhip_tx_sched_ctrs ctr{};
	std::vector<trxhip_tx_plan> plan;       /* the last render */
	std::vector<int> dirty;                  /* entries written in the current render */
};

}  // namespace

struct trxhip_tx_sched {
	trxhip_ctx *ctx = nullptr;
	trxhip_tx_sched_cfg cfg{};
	std::vector<Chan> ch;
	bool clock_set = false;
	uint32_t fn = 0;
	int tn = 0;
	int64_t next_id = 0;
	float att[256];

	// device state (ctx != NULL)
	size_t n_rows = 0;
	trx_pin<uint8_t> h_rows;                               /* pinned mirror and device ring, TRX_TXS_ROW_STRIDE each */
	trx_dev<uint8_t> d_rows;
	std::vector<int32_t> free_rows, dirty_rows;
	trx_dev<trx_tx_fill> d_fill;                           /* [chans][TRX_TXS_ENTRIES] */
	size_t buf_words = 0, buf_bytes = 0;
	trx_pin<uint8_t> h_buf[kBufs];                         /* slot words, then fill updates */
	trx_dev<uint8_t> d_buf[kBufs];
	std::vector<int32_t> held[kBufs];                      /* rows the render in buffer k consumed */
	int next_buf = 0;
	uint64_t n_renders = 0;
	std::vector<int32_t> consumed;                         /* rows consumed by the render being planned */
	std::vector<trx_tx_fill_update> upd;
	// front end remainder (render_frontend)
	trx_dev<float> d_carry;                                /* [chans][d_carry.cap / (2 * chans)] complex64 */
	size_t carried = 0;
	trx_event ev[kBufs];                                   /* pending: the render in buffer k (last: waited for before anything is freed) */
};

namespace {

size_t slot_start(int tn0, size_t s, int sps)
{
	if (sps == 4)
		return s * 625;
	auto pre = [](int tn) -> size_t { return (size_t)tn * 156 + (size_t)((tn + 3) >> 2); };
	const size_t t = (size_t)tn0 + s;
	return (t >> 3) * 1250 + pre((int)(t & 7)) - pre(tn0);
}

void release_buf(trxhip_tx_sched *s, int k)
{
	for (int32_t r : s->held[k])
		s->free_rows.push_back(r);
	s->held[k].clear();
}

// wait for the oldest render still holding rows (only when every staging row is taken)
int reclaim_rows(trxhip_tx_sched *s)
{
	for (int i = 0; i < kBufs; i++) {
		const int k = (s->next_buf + i) % kBufs;     /* oldest first */
		if (!s->ev[k].pending() || s->held[k].empty())
			continue;
		if (s->ev[k].wait() != TRXHIP_OK)
			return TRXHIP_EIO;
		release_buf(s, k);
		return TRXHIP_OK;
	}
	return TRXHIP_ENOMEM;
}

void fill_update(trxhip_tx_sched *s, Chan &c, const QItem &b)
{
	// updateFillerTable(), Transceiver.cpp:403-414: the entry of the burst's own TN at FN % the TN's current modulus
	const int e = (int)(b.fn % (uint32_t)c.modulus[b.tn]) * 8 + b.tn;
	FillMirror &f = c.fill[e];
	if (f.row < 0)
		c.dirty.push_back(e);
	f.writer = b.id;
	f.row = b.row >= 0 ? b.row : 0;       /* plan-only: marks "written in this render" */
	f.item = b;
}

void consume(trxhip_tx_sched *s, const QItem &b)
{
	if (b.row >= 0)
		s->consumed.push_back(b.row);
}

// pushRadioVector()'s loop body for every channel over n_slots slots from the clock, then incTN (GSMCommon.h:141-150).
// Writes words[c * n_slots + k] when words != NULL.
void plan_slots(trxhip_tx_sched *s, size_t n_slots, uint32_t *words)
{
	for (size_t ci = 0; ci < s->ch.size(); ci++) {
		Chan &c = s->ch[ci];
		c.plan.resize(n_slots);
		uint32_t fn = s->fn;
		int tn = s->tn;
		for (size_t k = 0; k < n_slots; k++) {
			trxhip_tx_plan &p = c.plan[k];
			p.fn = fn;
			p.tn = (uint8_t)tn;
			p.reserved[0] = p.reserved[1] = 0;
			const bool zeros = c.chan_type[tn] == TRXHIP_COMB_NONE || c.muted;
			while (!c.q.empty() && time_less(c.q.front().fn, c.q.front().tn, fn, tn)) {
				std::pop_heap(c.q.begin(), c.q.end(), QLater());
				const QItem b = c.q.back();
				c.q.pop_back();
				c.ctr.tx_stale_bursts++;
				if (c.retrans)
					fill_update(s, c, b);
				consume(s, b);
			}
			uint32_t word;
			if (!c.q.empty() && c.q.front().fn == fn && c.q.front().tn == tn) {
				std::pop_heap(c.q.begin(), c.q.end(), QLater());
				const QItem b = c.q.back();
				c.q.pop_back();
				if (c.retrans)
					fill_update(s, c, b);
				consume(s, b);
				p.src = TRXHIP_TXS_SRC_BURST;
				p.id = b.id;
				word = TRX_TXS_WORD(TRX_TXS_ROW, b.row < 0 ? 0 : b.row);
			} else {
				const int e = (int)(fn % (uint32_t)c.modulus[tn]) * 8 + tn;
				const FillMirror &f = c.fill[e];
				p.src = TRXHIP_TXS_SRC_FILLER;
				p.id = f.writer;
				if (f.row >= 0)                       /* written earlier in this render: the staged row is the entry */
					word = TRX_TXS_WORD(TRX_TXS_ROW, f.row);
				else if (f.writer < 0 && c.filler != TRXHIP_FILLER_DUMMY)
					word = TRX_TXS_WORD(TRX_TXS_ZERO, 0);     /* generateEmptyBurst(), scaled: zeros */
				else
					word = TRX_TXS_WORD(TRX_TXS_ENTRY, ci * TRX_TXS_ENTRIES + e);
				if (ci == 0 && c.filler == TRXHIP_FILLER_ZERO)
					c.ctr.tx_unavailable_bursts++;
			}
			if (zeros) {                                  /* the burst is still consumed, radioifyVector() writes zeros */
				p.src = TRXHIP_TXS_SRC_ZERO;
				p.id = -1;
				word = TRX_TXS_WORD(TRX_TXS_ZERO, 0);
			}
			if (words)
				words[ci * n_slots + k] = word;
			if (++tn > 7) {
				tn = 0;
				fn = (fn + 1) % kHyperframe;
			}
		}
		// the entries written in this render become device descriptors at its end
		for (int e : c.dirty) {
			FillMirror &f = c.fill[e];
			if (s->ctx) {
				trx_tx_fill_update u;
				u.entry = (uint32_t)(ci * TRX_TXS_ENTRIES + e);
				u.row = (uint32_t)f.row;
				u.nbits = f.item.nbits;
				u.guard = (uint8_t)(8 + (f.item.tn % 4 == 0));
				u.flags = f.item.flags;
				u.scale_re = f.item.att_scale;
				s->upd.push_back(u);
			}
			f.row = -1;
		}
		c.dirty.clear();
	}
	// the clock after the render
	const uint64_t t = (uint64_t)s->tn + n_slots;
	s->tn = (int)(t & 7);
	s->fn = (uint32_t)(((uint64_t)s->fn + (t >> 3)) % kHyperframe);
}

size_t render_samples(const trxhip_tx_sched *s, size_t n_slots)
{
	return slot_start(s->tn, n_slots, s->cfg.sps);
}

// plan n_slots and, on a device object, launch the render into out (channel c at out + 2 * c * out_stride floats)
int render_into(trxhip_tx_sched *s, size_t n_slots, float *d_cf32, size_t out_stride, int16_t *d_s16, const float *s16_scales,
		hipStream_t stream)
{
	if (!s->ctx) {
		plan_slots(s, n_slots, nullptr);
		return TRXHIP_OK;
	}
	if (with_device(s->ctx))
		return TRXHIP_EIO;
	const int k = s->next_buf;
	if (s->ev[k].pending()) {                              /* the render 4 calls back still reads this buffer */
		if (s->ev[k].wait() != TRXHIP_OK)
			return TRXHIP_EIO;
		release_buf(s, k);
	}
	// rows submitted since the last render: H2D, one copy per run of consecutive rows
	std::sort(s->dirty_rows.begin(), s->dirty_rows.end());
	for (size_t i = 0; i < s->dirty_rows.size();) {
		size_t j = i + 1;
		while (j < s->dirty_rows.size() && s->dirty_rows[j] == s->dirty_rows[j - 1] + 1)
			j++;
		const size_t off = (size_t)s->dirty_rows[i] * TRX_TXS_ROW_STRIDE;
		if (hipMemcpyAsync(s->d_rows + off, s->h_rows + off, (j - i) * TRX_TXS_ROW_STRIDE, hipMemcpyHostToDevice, stream) != hipSuccess)
			return TRXHIP_EIO;
		i = j;
	}
	s->dirty_rows.clear();

	uint32_t *words = reinterpret_cast<uint32_t *>(s->h_buf[k].p);
	const int tn0 = s->tn;
	s->consumed.clear();
	s->upd.clear();
	plan_slots(s, n_slots, words);
	const size_t wbytes = n_slots * s->ch.size() * sizeof(uint32_t);
	const size_t uoff = (wbytes + 15) & ~(size_t)15;
	memcpy(s->h_buf[k] + uoff, s->upd.data(), s->upd.size() * sizeof(trx_tx_fill_update));
	int rc = TRXHIP_OK;
	if (hipMemcpyAsync(s->d_buf[k], s->h_buf[k], uoff + s->upd.size() * sizeof(trx_tx_fill_update), hipMemcpyHostToDevice, stream) !=
	    hipSuccess)
		rc = TRXHIP_EIO;
	if (rc == TRXHIP_OK)
		rc = trx_launch_tx_render(reinterpret_cast<const uint32_t *>(s->d_buf[k].p), n_slots, (int)s->ch.size(), tn0,
					  s->cfg.sps, s->d_rows, s->d_fill, s->att,
					  s->ctx->d_tx_tables, d_cf32, d_s16, s16_scales, out_stride, stream);
	if (rc == TRXHIP_OK)
		rc = trx_launch_tx_fill_update(reinterpret_cast<const trx_tx_fill_update *>(s->d_buf[k] + uoff), s->upd.size(), s->d_rows,
					       s->d_fill, stream);
	if (rc == TRXHIP_OK)
		rc = s->ev[k].record(stream);
	if (rc != TRXHIP_OK) {
		/* the launch did not go in: wait for the stream before the rows are reused */
		(void)hipStreamSynchronize(stream);
		for (int32_t r : s->consumed)
			s->free_rows.push_back(r);
		s->consumed.clear();
		return rc;
	}
	s->held[k].swap(s->consumed);
	s->next_buf = (k + 1) % kBufs;
	s->n_renders++;
	return TRXHIP_OK;
}

}  // namespace

extern "C" {

int trxhip_tx_sched_create(trxhip_ctx *ctx, const trxhip_tx_sched_cfg *cfg, trxhip_tx_sched **out)
{
	if (!cfg || !out)
		return TRXHIP_EINVAL;
	const trxhip_tx_sched_cfg c = *cfg;
	if (c.chans < 1 || c.chans > TRX_TXS_MAX_CHANS || (c.sps != 1 && c.sps != 4) ||
	    (c.filler != TRXHIP_FILLER_DUMMY && c.filler != TRXHIP_FILLER_ZERO) || c.queue_cap < 1 || c.queue_cap > (1 << 20) ||
	    c.max_slots < 1 || c.max_slots > ((uint64_t)1 << 26) || !std::isfinite(c.full_scale))
		return TRXHIP_EINVAL;
	if (ctx && (!ctx->d_tx_tables || with_device(ctx)))
		return TRXHIP_EINVAL;
	trxhip_tx_sched *s = new (std::nothrow) trxhip_tx_sched();
	if (!s)
		return TRXHIP_ENOMEM;
	s->cfg = c;
	s->ch.resize(c.chans);
	for (int i = 0; i < c.chans; i++) {
		Chan &ch = s->ch[i];
		for (int t = 0; t < 8; t++) {                  /* TransceiverState(), Transceiver.cpp:67-72 */
			ch.chan_type[t] = TRXHIP_COMB_NONE;
			ch.modulus[t] = 26;
		}
		ch.filler = i == 0 ? c.filler : TRXHIP_FILLER_ZERO;      /* :255-256 */
		ch.retrans = i == 0 && c.filler == TRXHIP_FILLER_DUMMY;   /* :218-219 */
		ch.q.reserve(c.queue_cap);
	}
	for (int a = 0; a < 256; a++)                          /* addRadioVector(), Transceiver.cpp:396 */
		s->att[a] = (float)(c.full_scale * pow(10, (double)-a / 20));
	if (!ctx) {
		*out = s;
		return TRXHIP_OK;
	}
	s->ctx = ctx;
	s->n_rows = 2 * (size_t)c.chans * c.queue_cap;
	s->buf_words = (size_t)c.max_slots * c.chans;
	s->buf_bytes = ((s->buf_words * 4 + 15) & ~(size_t)15) + (size_t)c.chans * TRX_TXS_ENTRIES * sizeof(trx_tx_fill_update);
	const size_t fill_bytes = (size_t)c.chans * TRX_TXS_ENTRIES * sizeof(trx_tx_fill);
	bool ok = s->h_rows.alloc(s->n_rows * TRX_TXS_ROW_STRIDE) == TRXHIP_OK && s->d_rows.alloc(s->n_rows * TRX_TXS_ROW_STRIDE) == TRXHIP_OK &&
		  s->d_fill.alloc((size_t)c.chans * TRX_TXS_ENTRIES) == TRXHIP_OK;
	for (int k = 0; ok && k < kBufs; k++)
		ok = s->h_buf[k].alloc(s->buf_bytes) == TRXHIP_OK && s->d_buf[k].alloc(s->buf_bytes) == TRXHIP_OK &&
		     s->ev[k].create() == TRXHIP_OK;
	if (ok) {
		/* the filler table as descriptors: channel 0 with FILLER_DUMMY holds the dummy burst (generateDummyBurst(), sigProcLib.cpp:
		 * 856-862) scaled by (full_scale, 0) (init()'s float scale, :123); the zero fillers are never read (the plan says ZERO) */
		std::vector<trx_tx_fill> fill((size_t)c.chans * TRX_TXS_ENTRIES);
		memset(fill.data(), 0, fill_bytes);
		if (c.filler == TRXHIP_FILLER_DUMMY) {
			trx_tx_tables *tab = static_cast<trx_tx_tables *>(malloc(sizeof(trx_tx_tables)));
			ok = tab && trx_tx_tables_generate(tab) == 0;
			for (int e = 0; ok && e < (int)TRX_TXS_ENTRIES; e++) {
				trx_tx_fill &f = fill[e];
				f.nbits = 148;
				f.guard = (uint8_t)(8 + (e % 8 % 4 == 0));
				f.flags = 0;
				f.scale_re = (float)c.full_scale;
				f.scale_im = 0.0f;
				memcpy(f.bits, tab->dummy_burst, 148);
			}
			free(tab);
		}
		ok = ok && hipMemcpy(s->d_fill, fill.data(), fill_bytes, hipMemcpyHostToDevice) == hipSuccess &&
		     hipMemset(s->d_rows, 0, s->n_rows * TRX_TXS_ROW_STRIDE) == hipSuccess;
	}
	if (!ok) {
		trxhip_tx_sched_destroy(s);
		return TRXHIP_ENOMEM;
	}
	s->free_rows.reserve(s->n_rows);
	for (size_t r = s->n_rows; r-- > 0;)
		s->free_rows.push_back((int32_t)r);
	*out = s;
	return TRXHIP_OK;
}

void trxhip_tx_sched_destroy(trxhip_tx_sched *s)
{
	if (!s)
		return;
	if (s->ctx)
		(void)with_device(s->ctx);
	delete s;
}

int trxhip_tx_sched_set_clock(trxhip_tx_sched *s, uint32_t fn, int tn)
{
	if (!s || fn >= kHyperframe || tn < 0 || tn > 7)
		return TRXHIP_EINVAL;
	s->fn = fn;
	s->tn = tn;
	s->clock_set = true;
	s->carried = 0;
	return TRXHIP_OK;
}

int trxhip_tx_sched_clock(const trxhip_tx_sched *s, uint32_t *fn, int *tn)
{
	if (!s || !fn || !tn || !s->clock_set)
		return TRXHIP_EINVAL;
	*fn = s->fn;
	*tn = s->tn;
	return TRXHIP_OK;
}

int trxhip_tx_sched_set_slot(trxhip_tx_sched *s, int chan, int tn, int comb)
{
	if (!s || chan < 0 || chan >= (int)s->ch.size() || tn < 0 || tn > 7 || comb < 0 || comb > TRXHIP_COMB_LOOPBACK)
		return TRXHIP_EINVAL;
	Chan &c = s->ch[chan];
	c.chan_type[tn] = comb;
	switch (comb) {                                        /* setModulus(), Transceiver.cpp:483-512 */
	case TRXHIP_COMB_NONE: case 1: case 2: case 3: case TRXHIP_COMB_FILL:
		c.modulus[tn] = 26;
		break;
	case 4: case 5: case 6:
		c.modulus[tn] = 51;
		break;
	case 7:
		c.modulus[tn] = 102;
		break;
	case 13:
		c.modulus[tn] = 52;
		break;
	default:
		break;
	}
	return TRXHIP_OK;
}

int trxhip_tx_sched_set_muted(trxhip_tx_sched *s, int chan, int muted)
{
	if (!s || chan < 0 || chan >= (int)s->ch.size())
		return TRXHIP_EINVAL;
	s->ch[chan].muted = muted != 0;                       /* RFMUTE, Transceiver.cpp:1068 */
	return TRXHIP_OK;
}

int trxhip_tx_sched_submit(trxhip_tx_sched *s, int chan, const uint8_t *h_dgram, size_t len, int64_t *id)
{
	if (!s || chan < 0 || chan >= (int)s->ch.size() || (!h_dgram && len))
		return TRXHIP_EINVAL;
	Chan &c = s->ch[chan];
	if (id)
		*id = -1;
	// driveTxPriorityQueue(), Transceiver.cpp:1102-1130: the length, then the header version
	uint16_t nbits;
	uint8_t flags = 0;
	if (len == 6 + 148) {
		nbits = 148;
	} else if (len == 6 + 444 && s->cfg.sps == 4) {
		nbits = 444;
		flags = TRXHIP_TX_8PSK;
	} else {
		c.ctr.refused++;
		return TRXHIP_OK;
	}
	if ((h_dgram[0] >> 4) > 1) {
		c.ctr.refused++;
		return TRXHIP_OK;
	}
	const int tn = h_dgram[0] & 7;
	const uint32_t fn = ((uint32_t)h_dgram[1] << 24) | ((uint32_t)h_dgram[2] << 16) | ((uint32_t)h_dgram[3] << 8) | h_dgram[4];
	// FN order per TN (:1137-1171); a repeated FN is dropped, nothing else is
	int32_t delta = 0;
	if (c.first_dl[tn]) {
		delta = fn_delta((int32_t)fn, (int32_t)c.last_dl_fn[tn]);
		if (delta == 0) {
			c.ctr.tx_trxd_fn_repeated++;
			return TRXHIP_OK;
		}
	}
	if (c.q.size() >= (size_t)s->cfg.queue_cap)
		return TRXHIP_ENOMEM;                          /* before any state changes */
	int32_t row = -1;
	if (s->ctx) {
		if (s->free_rows.empty()) {
			const int rc = reclaim_rows(s);
			if (rc != TRXHIP_OK)
				return rc;
		}
		row = s->free_rows.back();
		s->free_rows.pop_back();
		uint8_t *dst = s->h_rows + (size_t)row * TRX_TXS_ROW_STRIDE;
		memcpy(dst, h_dgram, len);
		const uint16_t l16 = (uint16_t)len;
		memcpy(dst + TRX_TXS_ROW_STRIDE - 2, &l16, 2);       /* the row's length, read by tx_render_kernel */
		s->dirty_rows.push_back(row);
	}
	if (c.first_dl[tn]) {
		if (delta < 0)
			c.ctr.tx_trxd_fn_outoforder++;
		else if (delta > 1 && chan == 0 && c.filler == TRXHIP_FILLER_ZERO)
			c.ctr.tx_trxd_fn_skipped += (uint64_t)(delta - 1);
		if (delta > 0)
			c.last_dl_fn[tn] = fn;
	} else {
		c.first_dl[tn] = true;
		c.last_dl_fn[tn] = fn;
	}
	QItem b;
	b.fn = fn;
	b.tn = tn;
	b.id = s->next_id++;
	b.row = row;
	b.nbits = nbits;
	b.flags = flags;
	b.att_scale = s->att[h_dgram[5]];
	c.q.push_back(b);
	std::push_heap(c.q.begin(), c.q.end(), QLater());
	if (id)
		*id = b.id;
	return TRXHIP_OK;
}

static int render_check(const trxhip_tx_sched *s, size_t n_slots)
{
	if (!s || !s->clock_set || n_slots > s->cfg.max_slots)
		return TRXHIP_EINVAL;
	return TRXHIP_OK;
}

int trxhip_tx_sched_render(trxhip_tx_sched *s, size_t n_slots, float *d_out_cf32, size_t out_stride, int16_t *d_out_s16,
			   const float *s16_scales, void *stream)
{
	if (render_check(s, n_slots) != TRXHIP_OK)
		return TRXHIP_EINVAL;
	if (s->ctx) {
		if ((!d_out_cf32 && !d_out_s16) || (d_out_s16 && !s16_scales) || out_stride < render_samples(s, n_slots) ||
		    (reinterpret_cast<uintptr_t>(d_out_cf32) & 7) || (reinterpret_cast<uintptr_t>(d_out_s16) & 3))
			return TRXHIP_EINVAL;
	}
	if (n_slots == 0)
		return TRXHIP_OK;
	s->carried = 0;                                        /* a plain render breaks the front end's stream */
	return render_into(s, n_slots, d_out_cf32, out_stride, d_out_s16, s16_scales, static_cast<hipStream_t>(stream));
}

int trxhip_tx_sched_render_frontend(trxhip_tx_sched *s, size_t n_slots, trxhip_tx_frontend *fe, float *d_out_cf32,
				    int16_t *d_out_s16, float s16_scale, size_t out_cap, size_t *n_blocks, size_t *n_carried, void *stream)
{
	if (render_check(s, n_slots) != TRXHIP_OK || !s->ctx || !fe || !n_blocks || (!d_out_cf32 && !d_out_s16))
		return TRXHIP_EINVAL;
	int fe_chans = 0, block_len = 0;
	size_t out_per_block = 0;
	if (trx_tx_frontend_geometry(fe, &fe_chans, &block_len, &out_per_block) != TRXHIP_OK || fe_chans != (int)s->ch.size())
		return TRXHIP_EINVAL;
	const size_t n_new = render_samples(s, n_slots), total = s->carried + n_new, nb = total / (size_t)block_len;
	if (nb * out_per_block > out_cap)
		return TRXHIP_EINVAL;
	hipStream_t st = static_cast<hipStream_t>(stream);
	// the remainder (< block_len) plus the largest render from any TN: sized once per block_len, whatever the clock
	size_t most = 0;
	for (int t = 0; t < 8; t++)
		most = std::max(most, slot_start(t, s->cfg.max_slots, s->cfg.sps));
	const size_t need = (size_t)block_len + most + 8, row_floats = 2 * s->ch.size();
	if (s->d_carry.cap < need * row_floats) {              /* first use, or a front end of a longer block */
		if (with_device(s->ctx))
			return TRXHIP_EIO;
		/* the one growth that keeps contents: copy, wait for the copy, then the old block goes */
		trx_dev<float> p;
		if (p.alloc(need * row_floats) != TRXHIP_OK)
			return TRXHIP_ENOMEM;
		if (s->carried && s->d_carry &&
		    hipMemcpy2DAsync(p, need * 8, s->d_carry, s->d_carry.cap / row_floats * 8, s->carried * 8, s->ch.size(),
				     hipMemcpyDeviceToDevice, st) != hipSuccess)
			return TRXHIP_EIO;
		if (s->d_carry)
			(void)hipStreamSynchronize(st);
		s->d_carry = std::move(p);
	}
	const size_t carry_stride = s->d_carry.cap / row_floats;
	*n_blocks = 0;
	int rc = n_slots ? render_into(s, n_slots, s->d_carry + 2 * s->carried, carry_stride, nullptr, nullptr, st) : TRXHIP_OK;
	if (rc != TRXHIP_OK)
		return rc;
	if (nb) {
		// RadioInterface::driveTransmitRadio(): while (pushBuffer()); -- every whole block goes out, the rest stays
		rc = trxhip_tx_frontend_push(fe, s->d_carry, carry_stride, nb, d_out_cf32, d_out_s16, s16_scale, stream);
		if (rc != TRXHIP_OK)
			return rc;
		const size_t used = nb * (size_t)block_len, rest = total - used;
		if (rest && hipMemcpy2DAsync(s->d_carry, carry_stride * 8, s->d_carry + 2 * used, carry_stride * 8, rest * 8, s->ch.size(),
					     hipMemcpyDeviceToDevice, st) != hipSuccess)
			return TRXHIP_EIO;                          /* rest < block_len <= used: the ranges do not overlap */
	}
	s->carried = total - nb * (size_t)block_len;
	*n_blocks = nb;
	if (n_carried)
		*n_carried = s->carried;
	return TRXHIP_OK;
}

int trxhip_tx_sched_plan(const trxhip_tx_sched *s, int chan, trxhip_tx_plan *h_out, size_t n)
{
	if (!s || chan < 0 || chan >= (int)s->ch.size() || (!h_out && n) || n > s->ch[chan].plan.size())
		return TRXHIP_EINVAL;
	if (n)
		memcpy(h_out, s->ch[chan].plan.data(), n * sizeof(trxhip_tx_plan));
	return TRXHIP_OK;
}

int trxhip_tx_sched_counters(const trxhip_tx_sched *s, int chan, trxhip_tx_sched_ctrs *out)
{
	if (!s || !out || chan < 0 || chan >= (int)s->ch.size())
		return TRXHIP_EINVAL;
	*out = s->ch[chan].ctr;
	return TRXHIP_OK;
}

}  // extern "C"
