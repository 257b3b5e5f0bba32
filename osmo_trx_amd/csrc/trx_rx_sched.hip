// trx_rx_sched.hip -- the uplink burst scheduler: each channel's receive sample stream in, TRXD uplink indications out.
//
// The counterpart of trx_tx_sched.cpp.  It restates what the reference does between the radio's receive buffer and the wire:
//   RadioInterface::driveReceiveRadio()        radioInterface.cpp:240-294   cut slots `while (recvSz > burstSize)`, incTN;
//                                                                           burstSize 625 at 4 SPS, 157/156/156/156 at 1 SPS
//   Transceiver::pullRadioVector()             Transceiver.cpp:665-815      burstTime, OFF, mute, power, noise ring, counters
//   Transceiver::expectedCorrType()            Transceiver.cpp:513-601      (trx_rx_sched.h)
//   noiseVector::insert() / avg()              radioVector.cpp:84-108
//   trxd_send_burst_ind_v0 / _v1               proto_trxd.c:68-117          (the existing wire packer, once per channel)
// A pull is: rx_plan_kernel (burst parameters, TRXD meta, noise-ring positions of every cut slot, from the clock and the
// settings alone), rx_edge_kernel (the one slot per channel that straddles the carried remainder and the chunk; the new
// remainder), trxhip_detect_demod_batch[_cf32] over the straddling rows and, per channel, over the slots that lie inside the
// caller's chunk -- read where they are --, rx_ind_kernel (records, counters, noise ring), trx_launch_pack_trxd_wire per channel.
// At 1 SPS the slots in the chunk are not one length apart: they go to burst_pull_stream_kernel (trx_launch_pull_stream), which
// finds slot k from the run's first slot and its TN; the straddling rows, all of slot 0's length, take the batch entry point.
// trxhip_rx_sched_pull_frontend() is driveReceiveRadio()'s one step, pullBuffer() then the cutter: the receive front end stores its
// rows into the caller's work rows behind TRX_RXS_REM_STRIDE samples of room, rx_join_kernel puts the carried remainder in front
// of them and saves the new one, and every slot of the pull -- the one that begins in the remainder too -- is detected where it
// lies: no slot is assembled, no launch over straddling rows runs, and the plan, the epilogue and the packer are the same.
// With TRXHIP_FLAG_USE_VA (cfg->use_va, Transceiver.cpp:760-787; the stream is what the radio read 20 samples early) the detect
// launches above give way to one detect launch between trx_rx_sched_va.hip's two kernels: rx_va_prep_kernel (the detector's rows -- every slot's
// samples 20 .. 604, zeros behind -- and the power of the slots as read), trxhip_detect_demod_batch[_cf32] over those rows
// without soft output, rx_va_slot_kernel (the Viterbi receiver over the unshifted slots it found, read where they lie, sliced)
// and trxhip_apply_diversity_power (energy and rssi from the slots as read); the straddling row is one of the slots.
// With ctx == NULL the object is plan-only: cutter, clock and plan, no device memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_rx_sched.h"

static_assert(TRXHIP_RX_SCHED_WORK_HEAD == TRX_RXS_REM_STRIDE, "the work row's head holds one carried remainder");

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------
// rx_plan_kernel: one thread per (chan, slot); blockIdx.y = chan.  Nothing is read but the arguments.
//   plan   : the slot as pullRadioVector() sees it (type, mTSC, max_toa) -- the packer's d_params (OFF: nothing is sent)
//   params : the same for the detector, with muted slots as OFF so that no DSP runs on them (Transceiver.cpp:719-721)
//   meta   : burstTime and the channel's TRXD version
//   rank   : noise-ring insertions of this pull before the slot (type IDLE on a channel that is not muted, :744-748); it
//            depends on the plan alone: trx_rxs_inserts_before() up to the block's first slot, a block scan behind it
//   idle_slot[chan * n + r] : the slot of the pull's r-th insertion
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
rx_plan_kernel(const trx_rxs_settings st, uint32_t fn0, int tn0, uint32_t n_slots, trxhip_burst_params *__restrict__ plan,
	       trxhip_burst_params *__restrict__ params, trxhip_trxd_meta *__restrict__ meta, uint32_t *__restrict__ rank,
	       uint32_t *__restrict__ idle_slot, trxhip_burst_params *__restrict__ edge_params)
{
	__shared__ uint32_t s_base, s_wave[kThreads / 64];
	const int chan = blockIdx.y;
	const uint32_t first = blockIdx.x * kThreads, k = first + threadIdx.x;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0)
		s_base = 0;
	__syncthreads();
	if (threadIdx.x < 8) {
		const uint32_t c = trx_rxs_inserts_before(st, chan, fn0, tn0, first, (int)threadIdx.x);
		if (c)
			atomicAdd(&s_base, c);
	}
	const bool live = k < n_slots;
	trx_rxs_slot p = trx_rxs_plan_slot(st, chan, fn0, tn0, live ? k : 0);
	const bool ins = live && p.type == TRXHIP_IDLE && !p.muted;
	const unsigned long long m = __ballot(ins);
	if (lane == 0)
		s_wave[wave] = (uint32_t)__popcll(m);
	__syncthreads();
	uint32_t r = s_base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
	for (int w = 0; w < wave; w++)
		r += s_wave[w];
	if (!live)
		return;
	const size_t o = (size_t)chan * n_slots + k;
	trxhip_burst_params q;
	q.type = p.type;
	q.tsc = st.tsc;
	q.max_toa = p.max_toa;
	q.reserved = 0;
	plan[o] = q;
	if (p.muted)
		q.type = TRXHIP_OFF;
	params[o] = q;
	if (k == 0)
		edge_params[chan] = q;
	trxhip_trxd_meta mt;
	mt.fn = p.fn;
	mt.tn = p.tn;
	mt.version = (uint8_t)((st.version >> chan) & 1u);
	mt.tss = 0;                                                /* Transceiver.cpp:702 */
	mt.reserved = 0;
	meta[o] = mt;
	rank[o] = r;
	if (ins && r < n_slots)                                    /* (r < the pull's insertions <= n_slots) */
		idle_slot[(size_t)chan * n_slots + r] = k;
}

// ------------------------------------------------------------------------------------------------
// rx_edge_kernel: one block per channel.  The stream of this pull is the carried remainder followed by the chunk.  Its first
// slot0 samples (625; at 1 SPS slot 0's 157 or 156), when some of them are carried, are the one slot that does not lie in the
// caller's chunk: it is assembled into edge_row, rows slot0 apart.  The samples from `cut` on, behind the last cut slot, go to the
// OTHER half of the remainder area (the scheme of rx_resamp_s16_kernel): nothing a pull reads is overwritten by it.
// T: one IQ sample (uint32_t: int16 pair; float2).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads)
rx_edge_kernel(const T *__restrict__ in, size_t in_stride, const T *__restrict__ rem_in, T *__restrict__ rem_out, uint32_t carried,
	       uint32_t n_slots, uint32_t slot0, size_t cut, uint32_t n_rem, T *__restrict__ edge_row)
{
	const int chan = blockIdx.x;
	const T *x = in + (size_t)chan * in_stride;
	const T *r = rem_in + (size_t)chan * TRX_RXS_REM_STRIDE;
	if (n_slots && carried)
		for (uint32_t i = threadIdx.x; i < slot0; i += kThreads)
			edge_row[(size_t)chan * slot0 + i] = i < carried ? r[i] : x[i - carried];
	/* cut < carried + n_samples; n_rem = the difference, <= the next slot's length */
	for (uint32_t i = threadIdx.x; i < n_rem; i += kThreads) {
		const size_t j = cut + i;
		rem_out[(size_t)chan * TRX_RXS_REM_STRIDE + i] = j < carried ? r[j] : x[j - carried];
	}
}

// ------------------------------------------------------------------------------------------------
// rx_join_kernel: one block per channel, behind the front end's kernels of a trxhip_rx_sched_pull_frontend().  The front end has
// stored this pull's samples of channel `chan` from work[chan * work_stride + TRX_RXS_REM_STRIDE] on, the same aligned place
// every pull.  The `carried` samples of the remainder go in front of them, to [TRX_RXS_REM_STRIDE - carried, TRX_RXS_REM_STRIDE),
// so that the pull's stream lies in one piece and all its slots are read where they lie (nothing to do when no slot is cut).
// The samples from `cut` on go to the OTHER half of the remainder area, in rx_edge_kernel's format and place: a pull_cf32 may
// follow.  What is read (rem_in, the front end's samples) and what is written (the row's head, rem_out) never overlap.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
rx_join_kernel(float2 *work, size_t work_stride, const float2 *__restrict__ rem_in, float2 *__restrict__ rem_out, uint32_t carried,
	       uint32_t n_slots, size_t cut, uint32_t n_rem)
{
	const int chan = blockIdx.x;
	float2 *x = work + (size_t)chan * work_stride + TRX_RXS_REM_STRIDE;         /* the front end's first sample */
	const float2 *r = rem_in + (size_t)chan * TRX_RXS_REM_STRIDE;
	if (n_slots)
		for (uint32_t i = threadIdx.x; i < carried; i += kThreads)
			(x - carried)[i] = r[i];                                   /* carried <= 625 < TRX_RXS_REM_STRIDE */
	/* cut < carried + the front end's samples; n_rem = the difference, <= the next slot's length */
	for (uint32_t i = threadIdx.x; i < n_rem; i += kThreads) {
		const size_t j = cut + i;
		rem_out[(size_t)chan * TRX_RXS_REM_STRIDE + i] = j < carried ? r[j] : x[j - carried];
	}
}

// ------------------------------------------------------------------------------------------------
// rx_ind_kernel: the epilogue, one thread per (chan, slot); blockIdx.y = chan.  With a straddling row, block gridDim.x - 1 of
// every channel only moves that row's soft bits to slot 0.
// Noise ring (noiseVector, radioVector.cpp:84-108; Transceiver.cpp:744-748) without walking the slots: the pull's r-th insertion
// goes to ring position (itr0 + r) % 20, so after the insertion of rank R position j holds the insertion of the largest rank
// r <= R with (itr0 + r) % 20 == j, or the carried-in entry when there is none; mNoiseLev is their float sum in index order,
// / 20.0f -- the reference's additions in its order.  The state is read from noise_in and left for the next pull in noise_out.
// ------------------------------------------------------------------------------------------------
struct RssiOffsets { float v[TRX_RXS_MAX_CHANS]; };

struct NoiseView {
	const trx_rxs_noise *in;
	const uint32_t *idle_slot;          /* this channel's */
	const trxhip_burst_result *res;     /* this channel's */
	const trxhip_burst_result *edge;    /* the straddling row's record, or NULL */
	uint32_t n_slots;

	__device__ float energy(uint32_t slot) const
	{
		if (slot >= n_slots)                                            /* (never: idle_slot holds slots of this pull) */
			slot = n_slots - 1;
		return (slot == 0 && edge) ? edge->energy : res[slot].energy;
	}
	/* ring[j] after the insertion of rank R */
	__device__ float entry(int j, uint32_t R) const
	{
		const uint32_t i0 = in->itr % TRX_RXS_NOISE_CNT;                /* insert(): itr >= size -> 0 */
		const uint32_t d = ((uint32_t)j + TRX_RXS_NOISE_CNT - i0) % TRX_RXS_NOISE_CNT;   /* the first rank that lands on j */
		if (d > R)
			return in->ring[j];
		const uint32_t r = R - (R - d) % TRX_RXS_NOISE_CNT;
		return sqrtf(energy(idle_slot[r]));                             /* avg = sqrt(avg / chans()), one path (:742) */
	}
	/* noiseVector::avg() after the insertion of rank R */
	__device__ float level(uint32_t R) const
	{
		float val = 0.0f;
		for (int j = 0; j < TRX_RXS_NOISE_CNT; j++)
			val += entry(j, R);
		return val / (float)TRX_RXS_NOISE_CNT;
	}
};

__global__ void __launch_bounds__(kThreads)
rx_ind_kernel(uint32_t n_slots, const trxhip_burst_params *__restrict__ plan, const trxhip_burst_params *__restrict__ params,
	      const trxhip_trxd_meta *__restrict__ meta, trxhip_burst_result *res, const trxhip_burst_result *__restrict__ edge_res,
	      const uint32_t *__restrict__ rank, const uint32_t *__restrict__ idle_slot, const trx_rxs_noise *__restrict__ noise_in,
	      trx_rxs_noise *__restrict__ noise_out, unsigned long long *__restrict__ ctrs, trxhip_ul_ind *__restrict__ ind,
	      const float *__restrict__ edge_soft, float *__restrict__ soft, int soft_stride, const RssiOffsets offs)
{
	__shared__ uint32_t s_clip, s_nodet;
	const int chan = blockIdx.y;
	const size_t base = (size_t)chan * n_slots;
	if (edge_res && blockIdx.x == gridDim.x - 1) {
		for (int i = threadIdx.x; i < soft_stride; i += kThreads)
			soft[base * (size_t)soft_stride + i] = edge_soft[(size_t)chan * soft_stride + i];
		return;
	}
	if (threadIdx.x == 0)
		s_clip = s_nodet = 0;
	__syncthreads();
	NoiseView nv;
	nv.in = noise_in + chan;
	nv.idle_slot = idle_slot + base;
	nv.res = res + base;
	nv.edge = edge_res ? edge_res + chan : nullptr;
	nv.n_slots = n_slots;
	const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
	bool clip = false, nodet = false;
	if (k < n_slots) {
		const trxhip_burst_params pl = plan[base + k];
		const bool muted = pl.type != TRXHIP_OFF && params[base + k].type == TRXHIP_OFF;
		trxhip_burst_result r = (k == 0 && edge_res) ? edge_res[chan] : res[base + k];
		/* a muted slot went through the detector as OFF: rc 0, idle, rssi 0 -- bi as ret_idle leaves it (:693-704, :719-721).
		 * The packer adds the channel's rssi_offset to every record; bi->rssi of a muted slot is 0.0 without it */
		if (muted)
			r.rssi = -offs.v[chan];
		if (muted || (k == 0 && edge_res))
			res[base + k] = r;                                 /* the packer reads the channel's records in slot order */
		const trxhip_trxd_meta mt = meta[base + k];
		const uint32_t done = rank[base + k] + (uint32_t)(pl.type == TRXHIP_IDLE && !muted);   /* insertions up to this slot */
		trxhip_ul_ind o;
		o.fn = mt.fn;
		o.tn = mt.tn;
		o.type = pl.type;
		o.flags = (uint8_t)((pl.type == TRXHIP_OFF ? TRXHIP_ULIND_OFF : 0) | (muted ? TRXHIP_ULIND_MUTED : 0) |
				    ((pl.type != TRXHIP_OFF && r.idle) ? TRXHIP_ULIND_IDLE : 0));
		o.tsc = r.tsc;
		o.rc = r.rc;
		o.toa = r.toa;
		o.ci = r.ci;
		o.rssi = muted ? 0.0f : r.rssi;
		o.noise_lev = done ? nv.level(done - 1) : nv.in->lev;
		o.nbits = (uint16_t)(4u * r.nbits_div4);
		o.reserved = 0;
		ind[base + k] = o;
		clip = r.rc == -TRXHIP_SIGERR_CLIP;                        /* Transceiver.cpp:769-778 */
		nodet = r.rc < 0 && !clip;
	}
	const unsigned long long mc = __ballot(clip), mn = __ballot(nodet);
	if ((threadIdx.x & 63) == 0) {
		if (mc) atomicAdd(&s_clip, (uint32_t)__popcll(mc));
		if (mn) atomicAdd(&s_nodet, (uint32_t)__popcll(mn));
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		if (s_clip) atomicAdd(&ctrs[2 * chan + 0], (unsigned long long)s_clip);
		if (s_nodet) atomicAdd(&ctrs[2 * chan + 1], (unsigned long long)s_nodet);
	}
	// the state the next pull starts from
	if (blockIdx.x == 0 && threadIdx.x <= TRX_RXS_NOISE_CNT) {
		const size_t last = base + n_slots - 1;
		const uint32_t total = rank[last] + (uint32_t)(params[last].type == TRXHIP_IDLE);
		trx_rxs_noise *out = noise_out + chan;
		if (threadIdx.x < TRX_RXS_NOISE_CNT) {
			out->ring[threadIdx.x] = total ? nv.entry((int)threadIdx.x, total - 1) : nv.in->ring[threadIdx.x];
		} else {
			out->itr = total ? (nv.in->itr % TRX_RXS_NOISE_CNT + total - 1) % TRX_RXS_NOISE_CNT + 1 : nv.in->itr;
			out->lev = total ? nv.level(total - 1) : nv.in->lev;
			out->reserved[0] = out->reserved[1] = 0;
		}
	}
}

}  // namespace

struct trxhip_rx_sched {
	trxhip_ctx *ctx = nullptr;
	trxhip_rx_sched_cfg cfg{};
	trx_rxs_settings st{};
	float rssi_offset[TRX_RXS_MAX_CHANS] = {};
	bool clock_set = false;
	uint32_t fn = 0;
	int tn = 0;
	uint32_t carried = 0;                  /* samples per channel in the remainder */
	int carried_cf32 = 0;                  /* their format */
	// the last pull, for trxhip_rx_sched_plan()
	trx_rxs_settings last_st{};
	uint32_t last_fn = 0;
	int last_tn = 0;
	size_t last_n = 0;
	// device state (ctx != NULL)
	int soft_stride = 148;
	trx_dev<trxhip_burst_params> d_plan, d_params, d_edge_params;
	trx_dev<trxhip_trxd_meta> d_meta;
	trx_dev<trxhip_burst_result> d_res, d_edge_res;
	trx_dev<uint32_t> d_rank, d_idle_slot;
	trx_dev<float> d_soft, d_edge_soft;
	trx_dev<char> d_shift;                 /* TRXHIP_FLAG_USE_VA: [chans][max_slots][625] samples of shift_cf32's format, the detector's rows */
	int shift_cf32 = 0;
	trx_dev<float> d_energy;               /* TRXHIP_FLAG_USE_VA: [chans][max_slots], energyDetect of the slots as read */
	trx_dev<char> d_edge_row;              /* [chans][625] samples of either format (1 SPS: rows of slot 0's 157 or 156) */
	trx_dev<char> d_rem;                   /* [2][chans][TRX_RXS_REM_STRIDE] samples of either format */
	trx_dev<trx_rxs_noise> d_noise;        /* [2][chans] */
	trx_dev<unsigned long long> d_ctrs;    /* [chans][2]: rx_clipping, rx_no_burst_detected */
	int rem_half = 0, noise_half = 0;      /* the halves the next pull reads */
	trx_event ev;                          /* behind the last pull (the last member: waited for before the buffers are freed) */
};

namespace {

bool chan_ok(const trxhip_rx_sched *s, int chan) { return s && chan >= 0 && chan < s->cfg.chans; }

// the pulls issued so far have completed
int wait_pulls(trxhip_rx_sched *s)
{
	if (with_device(s->ctx))
		return TRXHIP_EIO;
	return s->ev.wait();
}

int launched() { return hipGetLastError() == hipSuccess ? TRXHIP_OK : TRXHIP_EIO; }

// radioInterface.cpp:272-291: the slots a pull of n_samples cuts.  At 1 SPS the count depends on the clock's TN as well
uint64_t slots_of(const trxhip_rx_sched *s, size_t n_samples)
{
	return s->cfg.sps == 1 ? trx_rxs_slots1(s->tn, s->carried, n_samples) : trx_rxs_slots(s->carried, n_samples);
}

// a pull through the receive front end: d_in is then the place in the work rows where the front end stores (complex64)
struct FrontEndPull {
	trxhip_rx_frontend *fe;
	const int16_t *d_wide;
	size_t n_blocks;
};

int pull(trxhip_rx_sched *s, const void *d_in, int cf32, size_t in_stride, size_t n_samples, uint8_t *d_pkt, int pkt_stride,
	 uint16_t *d_pkt_len, trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots, size_t *n_slots, size_t *n_carried, void *stream,
	 const FrontEndPull *fep = nullptr)
{
	if (!s || !s->clock_set)
		return TRXHIP_EINVAL;
	const uint64_t n64 = slots_of(s, n_samples);
	if (n64 > s->cfg.max_slots)
		return TRXHIP_EINVAL;
	const uint32_t n = (uint32_t)n64;
	const int chans = s->cfg.chans;
	const bool sps1 = s->cfg.sps == 1;
	/* a 1-SPS object refuses mixed formats without a context too: its plan-only form refuses what the device form refuses */
	if (!s->ctx && sps1 && n_samples && s->carried && cf32 != s->carried_cf32)
		return TRXHIP_EINVAL;
	if (s->ctx) {
		const uintptr_t align = cf32 ? 7 : 3;
		if (n_samples && (!d_in || (reinterpret_cast<uintptr_t>(d_in) & align) || in_stride < n_samples))
			return TRXHIP_EINVAL;
		if (n_samples && s->carried && cf32 != s->carried_cf32)
			return TRXHIP_EINVAL;
		if (n && (n > out_slots || !d_pkt || !d_pkt_len || !d_ind || pkt_stride < 160 || (pkt_stride & 3) ||
			  (reinterpret_cast<uintptr_t>(d_pkt) & 3) || (reinterpret_cast<uintptr_t>(d_soft) & 3) ||
			  (reinterpret_cast<uintptr_t>(d_ind) & 3) || (reinterpret_cast<uintptr_t>(d_pkt_len) & 1)))
			return TRXHIP_EINVAL;
	} else if (d_in || d_pkt || d_pkt_len || d_ind || d_soft) {
		return TRXHIP_EINVAL;                                  /* a plan-only object takes no buffers */
	}
	/* where the remainder begins in this pull's stream, and the length of slot 0 (the straddling one, the same for all channels) */
	const uint64_t cut = sps1 ? trx_rxs_slot_start(s->tn, n) : (uint64_t)n * TRX_RXS_SLOT;
	const uint32_t slot0 = sps1 ? trx_rxs_slot_len(s->tn, 0) : TRX_RXS_SLOT;
	const uint32_t n_rem = (uint32_t)(s->carried + n_samples - cut);
	if (s->ctx && n_samples) {
		if (with_device(s->ctx))
			return TRXHIP_EIO;
		const hipStream_t st = static_cast<hipStream_t>(stream);
		const bool straddle = n && s->carried && !fep;         /* through the front end the stream lies in one piece */
		const bool va = (s->cfg.flags & TRXHIP_FLAG_USE_VA) != 0;
		const bool edge_rec = straddle && !va;                 /* the straddling row has a record and a soft row of its own */
		const size_t esz = cf32 ? 8 : 4;
		const char *rem_in = s->d_rem + (size_t)s->rem_half * chans * TRX_RXS_REM_STRIDE * esz;
		char *rem_out = s->d_rem + (size_t)(s->rem_half ^ 1) * chans * TRX_RXS_REM_STRIDE * esz;
		const unsigned bpc = (n + kThreads - 1) / kThreads;     /* blocks per channel */
		if (n && !d_soft && !s->d_soft) {
			/* the wire packer reads soft rows: a caller that takes none gets the object's own, chans * max_slots rows, allocated
			 * on its first such pull (hipMalloc may wait for the device); nothing has changed yet if it fails */
			if (s->d_soft.alloc((size_t)chans * s->cfg.max_slots * (size_t)s->soft_stride) != TRXHIP_OK)
				return TRXHIP_ENOMEM;
		}
		if (va && n && (!s->d_shift || s->shift_cf32 != cf32)) {
			/* the detector's rows, in the stream's format: allocated on the first use_va pull, and again when the format changes
			 * (only with nothing carried, see above); hipFree waits for the pulls that read the old rows.  Nothing has changed
			 * yet if it fails */
			(void)s->d_shift.reset();
			if (s->d_shift.alloc((size_t)chans * s->cfg.max_slots * TRX_RXS_SLOT * esz) != TRXHIP_OK)
				return TRXHIP_ENOMEM;
			s->shift_cf32 = cf32;
		}
		float *soft = d_soft ? d_soft : s->d_soft;
		const int ss = s->soft_stride;
		int rc = TRXHIP_OK;
		if (n) {
			hipLaunchKernelGGL(rx_plan_kernel, dim3(bpc, chans), dim3(kThreads), 0, st, s->st, s->fn, s->tn, n, s->d_plan, s->d_params,
					   s->d_meta, s->d_rank, s->d_idle_slot, s->d_edge_params);
			rc = launched();
		}
		if (rc == TRXHIP_OK && fep) {
			float *rows = const_cast<float *>(static_cast<const float *>(d_in));
			rc = trxhip_rx_frontend_pull(fep->fe, fep->d_wide, fep->n_blocks, rows, in_stride, stream);
			if (rc == TRXHIP_OK) {
				hipLaunchKernelGGL(rx_join_kernel, dim3(chans), dim3(kThreads), 0, st,
						   reinterpret_cast<float2 *>(rows) - TRX_RXS_REM_STRIDE, in_stride,
						   reinterpret_cast<const float2 *>(rem_in), reinterpret_cast<float2 *>(rem_out), s->carried, n,
						   (size_t)cut, n_rem);
				rc = launched();
			}
		} else if (rc == TRXHIP_OK) {
			if (cf32)
				hipLaunchKernelGGL(rx_edge_kernel<float2>, dim3(chans), dim3(kThreads), 0, st, static_cast<const float2 *>(d_in),
						   in_stride, reinterpret_cast<const float2 *>(rem_in), reinterpret_cast<float2 *>(rem_out),
						   s->carried, n, slot0, (size_t)cut, n_rem, reinterpret_cast<float2 *>(s->d_edge_row.p));
			else
				hipLaunchKernelGGL(rx_edge_kernel<uint32_t>, dim3(chans), dim3(kThreads), 0, st, static_cast<const uint32_t *>(d_in),
						   in_stride, reinterpret_cast<const uint32_t *>(rem_in), reinterpret_cast<uint32_t *>(rem_out),
						   s->carried, n, slot0, (size_t)cut, n_rem, reinterpret_cast<uint32_t *>(s->d_edge_row.p));
			rc = launched();
		}
		/* use_va: detection alone, no soft bits from it (Transceiver.cpp:762-768) */
		const int flags = va ? 0 : TRXHIP_FLAG_SLICE | (s->cfg.flags & TRXHIP_FLAG_EXACT_DEMOD);
		auto detect = [&](const void *iq, const trxhip_burst_params *p, trxhip_burst_result *r, float *so, size_t cnt) {
			return cf32 ? trxhip_detect_demod_batch_cf32(s->ctx, static_cast<const float *>(iq), p, r, so, cnt, (int)slot0, s->cfg.sps,
								     s->cfg.threshold, s->cfg.full_scale, ss, flags, stream)
				    : trxhip_detect_demod_batch(s->ctx, static_cast<const int16_t *>(iq), p, r, so, cnt, (int)slot0, s->cfg.sps,
								s->cfg.threshold, s->cfg.full_scale, ss, flags, stream);
		};
		/* 1 SPS, the slots from k0 on: back to back from slot k0's start, 157 or 156 samples each.  The flags are those the
		 * batch entry point hands the row kernel (trx_capi.cpp, pull_common()) */
		auto detect_stream = [&](const void *iq, size_t k0, const trxhip_burst_params *p, trxhip_burst_result *r, float *so, size_t cnt) {
			const int kf = flags | (s->ctx->no_unit ? TRX_IFLAG_NO_UNIT : 0) | (s->ctx->no_sym ? TRX_IFLAG_NO_SYM : 0) |
				       (s->ctx->no_fast ? TRX_IFLAG_NO_FAST : 0);
			return trx_launch_pull_stream(iq, cf32, (unsigned)(((size_t)s->tn + k0) & 3u), p, r, so, s->ctx->d_tables, cnt,
						      s->cfg.threshold, s->cfg.full_scale, ss, kf, s->ctx->n_cu, st);
		};
		if (va && n) {
			/* cfg->use_va (Transceiver.cpp:760-787): every slot of the pull, the assembled straddling row among them, in one
			 * launch each -- the detector's rows and the power of the slots as read; detection over those rows; the Viterbi
			 * receiver over the unshifted slots it found, sliced; energy and rssi of the records from the slots as read */
			const void *edge = straddle ? s->d_edge_row : nullptr;
			const size_t all = (size_t)chans * n;
			if (rc == TRXHIP_OK)
				rc = trx_launch_rx_va_prep(d_in, cf32, in_stride, edge, s->carried, n, chans, s->d_shift, s->d_energy, st);
			if (rc == TRXHIP_OK)
				rc = detect(s->d_shift, s->d_params, s->d_res, nullptr, all);
			if (rc == TRXHIP_OK)
				rc = trx_launch_rx_va_slots(d_in, cf32, in_stride, edge, s->carried, n, chans, s->d_params, s->d_res, soft,
							    1.0f / (float)((1 << 14) - 1), ss, st);
			if (rc == TRXHIP_OK)
				rc = trxhip_apply_diversity_power(s->ctx, s->d_res, s->d_params, s->d_energy, all, s->cfg.full_scale, stream);
		}
		if (rc == TRXHIP_OK && edge_rec)
			rc = detect(s->d_edge_row, s->d_edge_params, s->d_edge_res, s->d_edge_soft, (size_t)chans);
		// the slots inside the chunk, where they are: slot k starts k * 625 - carried samples into it (1 SPS:
		// trx_rxs_slot_start(tn, k) - carried); the last of them ends before the chunk does.  Through the front end slot 0 is
		// one of them: it starts `carried` samples in front of the chunk, in the work row's head
		const size_t k0 = straddle ? 1 : 0;
		const ptrdiff_t first = (ptrdiff_t)(sps1 ? trx_rxs_slot_start(s->tn, k0) : k0 * TRX_RXS_SLOT) - (ptrdiff_t)s->carried;
		for (int c = 0; rc == TRXHIP_OK && !va && c < chans && n > k0; c++) {
			const size_t o = (size_t)c * n + k0;
			const char *iq = static_cast<const char *>(d_in) + ((ptrdiff_t)((size_t)c * in_stride) + first) * (ptrdiff_t)esz;
			rc = sps1 ? detect_stream(iq, k0, s->d_params + o, s->d_res + o, soft + o * (size_t)ss, n - k0)
				  : detect(iq, s->d_params + o, s->d_res + o, soft + o * (size_t)ss, n - k0);
		}
		if (rc == TRXHIP_OK && n) {
			RssiOffsets offs;
			memcpy(offs.v, s->rssi_offset, sizeof(offs.v));
			hipLaunchKernelGGL(rx_ind_kernel, dim3(bpc + (edge_rec ? 1u : 0u), chans), dim3(kThreads), 0, st, n, s->d_plan, s->d_params,
					   s->d_meta, s->d_res, edge_rec ? s->d_edge_res : nullptr, s->d_rank, s->d_idle_slot,
					   s->d_noise + (size_t)s->noise_half * chans, s->d_noise + (size_t)(s->noise_half ^ 1) * chans, s->d_ctrs,
					   d_ind, s->d_edge_soft, soft, ss, offs);
			rc = launched();
		}
		for (int c = 0; rc == TRXHIP_OK && c < chans && n; c++) {
			const size_t o = (size_t)c * n;
			rc = trx_launch_pack_trxd_wire(s->d_res + o, s->d_plan + o, soft + o * (size_t)ss, ss, s->d_meta + o,
						       d_pkt + o * (size_t)pkt_stride, pkt_stride, d_pkt_len + o, n, s->rssi_offset[c], st, nullptr);
		}
		if (rc == TRXHIP_OK)
			rc = s->ev.record(st);
		if (rc != TRXHIP_OK)
			return rc == TRXHIP_EINVAL ? TRXHIP_EIO : rc;      /* (the arguments were the scheduler's own) */
		s->rem_half ^= 1;
		if (n)
			s->noise_half ^= 1;
	}
	if (n_samples)
		s->carried_cf32 = cf32;
	if (n) {
		s->last_st = s->st;
		s->last_fn = s->fn;
		s->last_tn = s->tn;
	}
	s->last_n = n;
	// the clock n incTN() later
	const uint64_t t = (uint64_t)s->tn + n;
	s->tn = (int)(t & 7);
	s->fn = (uint32_t)(((uint64_t)s->fn + (t >> 3)) % TRX_RXS_HYPERFRAME);
	s->carried = n_rem;
	if (n_slots)
		*n_slots = n;
	if (n_carried)
		*n_carried = n_rem;
	return TRXHIP_OK;
}

// the pair trxhip_rx_sched_pull_frontend() takes: a device scheduler and a per-channel front end (1..3 ARFCNs, or RESAMP) on its
// context with one row per scheduler channel.  *n_out: the samples per channel n_blocks blocks give
bool frontend_ok(const trxhip_rx_sched *s, const trxhip_rx_frontend *fe, size_t n_blocks, int *resamp, size_t *n_out)
{
	trxhip_ctx *ctx = nullptr;
	int rows = 0, block_len = 0, p = 0, q = 0;
	if (!s || !s->ctx || trx_rx_frontend_geometry(fe, &ctx, &rows, resamp, &block_len, &p, &q) != TRXHIP_OK)
		return false;
	if (ctx != s->ctx || rows != s->cfg.chans)
		return false;
	/* the reference refuses use_va with multi-ARFCN (osmo-trx.cpp:492-496) */
	if ((s->cfg.flags & TRXHIP_FLAG_USE_VA) && !*resamp)
		return false;
	/* max_slots <= 2^20: a pull that could be accepted is far below this */
	if (n_blocks > ((size_t)1 << 40) / (size_t)block_len)
		return false;
	*n_out = trxhip_rx_frontend_out_samples(fe, n_blocks);
	return true;
}

// create: sps is 4, or 1 where the caller admits it (trxhip_rx_sched_create_sps)
int create(trxhip_ctx *ctx, const trxhip_rx_sched_cfg *cfg, trxhip_rx_sched **out, bool admit_sps1)
{
	if (!cfg || !out)
		return TRXHIP_EINVAL;
	const trxhip_rx_sched_cfg c = *cfg;
	/* EDGE needs 4 SPS on receive (osmo-trx.cpp:485-490) */
	if (c.sps != 4 && !(admit_sps1 && c.sps == 1 && !c.egprs))
		return TRXHIP_EINVAL;
	if (c.chans < 1 || c.chans > TRX_RXS_MAX_CHANS || c.tsc < 0 || c.tsc > 7 ||
	    c.ul_fn_offset <= -(int32_t)TRX_RXS_HYPERFRAME || c.ul_fn_offset >= (int32_t)TRX_RXS_HYPERFRAME ||
	    (c.flags & ~(TRXHIP_FLAG_EXACT_DEMOD | TRXHIP_FLAG_USE_VA)) || !(c.full_scale > 0.0f) || !std::isfinite(c.full_scale) || !std::isfinite(c.threshold) ||
	    c.max_slots < 1 || c.max_slots > ((uint64_t)1 << 20))
		return TRXHIP_EINVAL;
	/* use_va: 4 SPS, no EDGE (osmo-trx.cpp:492-496), and no filter demodulator whose operand order could be chosen */
	const bool va = (c.flags & TRXHIP_FLAG_USE_VA) != 0;
	if (va && (c.sps != 4 || c.egprs || (c.flags & TRXHIP_FLAG_EXACT_DEMOD)))
		return TRXHIP_EINVAL;
	if (ctx && with_device(ctx))
		return TRXHIP_EINVAL;
	trxhip_rx_sched *s = new (std::nothrow) trxhip_rx_sched();
	if (!s)
		return TRXHIP_ENOMEM;
	s->cfg = c;
	memset(&s->st, 0, sizeof(s->st));
	for (int i = 0; i < TRX_RXS_MAX_CHANS; i++)
		for (int t = 0; t < 8; t++)
			s->st.chan_type[i][t] = TRXHIP_COMB_NONE;              /* TransceiverState(), Transceiver.cpp:67-72 */
	s->st.ext_rach = c.ext_rach != 0;
	s->st.egprs = c.egprs != 0;
	s->st.tsc = (uint8_t)c.tsc;
	s->st.max_toa_nb = 30;
	s->st.max_toa_ab = 63;
	s->st.ul_fn_offset = c.ul_fn_offset;
	s->soft_stride = c.egprs ? 444 : 148;
	if (!ctx) {
		*out = s;
		return TRXHIP_OK;
	}
	s->ctx = ctx;
	const size_t slots = (size_t)c.chans * c.max_slots, ch = (size_t)c.chans;
	const size_t rem_bytes = 2 * ch * TRX_RXS_REM_STRIDE * 8, noise_bytes = 2 * ch * sizeof(trx_rxs_noise);
	bool ok = s->d_plan.alloc(slots) == TRXHIP_OK && s->d_params.alloc(slots) == TRXHIP_OK && s->d_meta.alloc(slots) == TRXHIP_OK &&
		  s->d_res.alloc(slots) == TRXHIP_OK && s->d_rank.alloc(slots) == TRXHIP_OK && s->d_idle_slot.alloc(slots) == TRXHIP_OK &&
		  s->d_edge_params.alloc(ch) == TRXHIP_OK && s->d_edge_res.alloc(ch) == TRXHIP_OK &&
		  s->d_edge_soft.alloc(ch * (size_t)s->soft_stride) == TRXHIP_OK && s->d_edge_row.alloc(ch * TRX_RXS_SLOT * 8) == TRXHIP_OK &&
		  s->d_rem.alloc(rem_bytes) == TRXHIP_OK && s->d_noise.alloc(2 * ch) == TRXHIP_OK && s->d_ctrs.alloc(ch * 2) == TRXHIP_OK &&
		  (!va || s->d_energy.alloc(slots) == TRXHIP_OK) && s->ev.create() == TRXHIP_OK;
	/* the ring starts as std::vector<float>(20): zeros, itr 0, mNoiseLev 0 (Transceiver.cpp:64) */
	ok = ok && hipMemset(s->d_rem, 0, rem_bytes) == hipSuccess && hipMemset(s->d_noise, 0, noise_bytes) == hipSuccess &&
	     hipMemset(s->d_ctrs, 0, ch * 2 * sizeof(unsigned long long)) == hipSuccess &&
	     hipStreamSynchronize(nullptr) == hipSuccess;      /* the first pull may come on a stream that does not wait for the null stream */
	if (!ok) {
		trxhip_rx_sched_destroy(s);
		return TRXHIP_ENOMEM;
	}
	*out = s;
	return TRXHIP_OK;
}

}  // namespace

extern "C" {

int trxhip_rx_sched_create(trxhip_ctx *ctx, const trxhip_rx_sched_cfg *cfg, trxhip_rx_sched **out)
{
	return create(ctx, cfg, out, false);
}

int trxhip_rx_sched_create_sps(trxhip_ctx *ctx, const trxhip_rx_sched_cfg *cfg, trxhip_rx_sched **out)
{
	return create(ctx, cfg, out, true);
}

void trxhip_rx_sched_destroy(trxhip_rx_sched *s)
{
	if (!s)
		return;
	if (s->ctx)
		(void)with_device(s->ctx);
	delete s;
}

int trxhip_rx_sched_set_clock(trxhip_rx_sched *s, uint32_t fn, int tn)
{
	if (!s || fn >= TRX_RXS_HYPERFRAME || tn < 0 || tn > 7)
		return TRXHIP_EINVAL;
	s->fn = fn;
	s->tn = tn;
	s->clock_set = true;
	s->carried = 0;
	return TRXHIP_OK;
}

int trxhip_rx_sched_clock(const trxhip_rx_sched *s, uint32_t *fn, int *tn)
{
	if (!s || !fn || !tn || !s->clock_set)
		return TRXHIP_EINVAL;
	*fn = s->fn;
	*tn = s->tn;
	return TRXHIP_OK;
}

int trxhip_rx_sched_set_slot(trxhip_rx_sched *s, int chan, int tn, int comb)
{
	if (!chan_ok(s, chan) || tn < 0 || tn > 7 || comb < 0 || comb > TRXHIP_COMB_LOOPBACK)
		return TRXHIP_EINVAL;
	s->st.chan_type[chan][tn] = (uint8_t)comb;                     /* SETSLOT, Transceiver.cpp:1047-1048 */
	return TRXHIP_OK;
}

int trxhip_rx_sched_set_handover(trxhip_rx_sched *s, int tn, int ss, int on)
{
	if (!s || tn < 0 || tn > 7 || ss < 0 || ss > 7)                    /* Transceiver.cpp:944-961 */
		return TRXHIP_EINVAL;
	if (on)
		s->st.handover[tn] |= (uint8_t)(1u << ss);
	else
		s->st.handover[tn] &= (uint8_t)~(1u << ss);
	return TRXHIP_OK;
}

int trxhip_rx_sched_set_muted(trxhip_rx_sched *s, int chan, int muted)
{
	if (!chan_ok(s, chan))
		return TRXHIP_EINVAL;
	s->st.muted = (uint8_t)(muted ? s->st.muted | (1u << chan) : s->st.muted & ~(1u << chan));   /* RFMUTE, Transceiver.cpp:1068 */
	return TRXHIP_OK;
}

int trxhip_rx_sched_set_trxd_version(trxhip_rx_sched *s, int chan, int version)
{
	if (!chan_ok(s, chan) || (version != 0 && version != 1))
		return TRXHIP_EINVAL;
	s->st.version = (uint8_t)(version ? s->st.version | (1u << chan) : s->st.version & ~(1u << chan));
	return TRXHIP_OK;
}

int trxhip_rx_sched_set_rssi_offset(trxhip_rx_sched *s, int chan, float rssi_offset_db)
{
	if (!chan_ok(s, chan) || !std::isfinite(rssi_offset_db))
		return TRXHIP_EINVAL;
	s->rssi_offset[chan] = rssi_offset_db;
	return TRXHIP_OK;
}

int trxhip_rx_sched_set_max_toa(trxhip_rx_sched *s, int max_toa_nb, int max_toa_ab)
{
	if (!s || max_toa_nb < 0 || max_toa_nb > 65535 || max_toa_ab < 0 || max_toa_ab > 65535)
		return TRXHIP_EINVAL;
	s->st.max_toa_nb = (uint16_t)max_toa_nb;                       /* SETMAXDLYNB, Transceiver.cpp:968-973 */
	s->st.max_toa_ab = (uint16_t)max_toa_ab;                       /* SETMAXDLY, :962-967 */
	return TRXHIP_OK;
}

int64_t trxhip_rx_sched_slots(const trxhip_rx_sched *s, size_t n_samples)
{
	if (!s)
		return TRXHIP_EINVAL;
	return (int64_t)slots_of(s, n_samples);
}

int trxhip_rx_sched_pull_s16(trxhip_rx_sched *s, const int16_t *d_in, size_t in_stride, size_t n_samples, uint8_t *d_pkt,
			     int pkt_stride, uint16_t *d_pkt_len, trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots, size_t *n_slots,
			     size_t *n_carried, void *stream)
{
	return pull(s, d_in, 0, in_stride, n_samples, d_pkt, pkt_stride, d_pkt_len, d_ind, d_soft, out_slots, n_slots, n_carried, stream);
}

int trxhip_rx_sched_pull_cf32(trxhip_rx_sched *s, const float *d_in, size_t in_stride, size_t n_samples, uint8_t *d_pkt,
			      int pkt_stride, uint16_t *d_pkt_len, trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots, size_t *n_slots,
			      size_t *n_carried, void *stream)
{
	return pull(s, d_in, 1, in_stride, n_samples, d_pkt, pkt_stride, d_pkt_len, d_ind, d_soft, out_slots, n_slots, n_carried, stream);
}

int64_t trxhip_rx_sched_slots_frontend(const trxhip_rx_sched *s, const trxhip_rx_frontend *fe, size_t n_blocks)
{
	int resamp;
	size_t n_out;
	if (!frontend_ok(s, fe, n_blocks, &resamp, &n_out))
		return TRXHIP_EINVAL;
	return (int64_t)slots_of(s, n_out);
}

int trxhip_rx_sched_pull_frontend(trxhip_rx_sched *s, trxhip_rx_frontend *fe, const int16_t *d_wide, size_t n_blocks, float *d_work,
				  size_t work_stride, uint8_t *d_pkt, int pkt_stride, uint16_t *d_pkt_len, trxhip_ul_ind *d_ind,
				  float *d_soft, size_t out_slots, size_t *n_slots, size_t *n_carried, void *stream)
{
	int resamp;
	size_t n_out;
	if (!frontend_ok(s, fe, n_blocks, &resamp, &n_out))
		return TRXHIP_EINVAL;
	if (!d_wide || (reinterpret_cast<uintptr_t>(d_wide) & (resamp ? 3 : 15)))     /* trxhip_rx_frontend_pull()'s rule */
		return TRXHIP_EINVAL;
	if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15) || (work_stride & 1) || work_stride < TRXHIP_RX_SCHED_WORK_HEAD + n_out)
		return TRXHIP_EINVAL;
	/* the front end's kernels store single complex64 samples (8 bytes) at d_out: every row's place behind the head, a multiple of
	 * 16 bytes from d_work, is more than they need.  From here on it is a complex64 pull of the chunk that will lie there */
	const FrontEndPull fep = { fe, d_wide, n_blocks };
	return pull(s, d_work + 2 * (size_t)TRXHIP_RX_SCHED_WORK_HEAD, 1, work_stride, n_out, d_pkt, pkt_stride, d_pkt_len, d_ind, d_soft,
		    out_slots, n_slots, n_carried, stream, &fep);
}

int trxhip_rx_sched_plan(const trxhip_rx_sched *s, int chan, trxhip_rx_plan *h_out, size_t n)
{
	if (!chan_ok(s, chan) || (!h_out && n) || n > s->last_n)
		return TRXHIP_EINVAL;
	for (size_t k = 0; k < n; k++) {
		const trx_rxs_slot p = trx_rxs_plan_slot(s->last_st, chan, s->last_fn, s->last_tn, k);
		h_out[k].fn = p.fn;
		h_out[k].tn = p.tn;
		h_out[k].type = p.type;
		h_out[k].max_toa = p.max_toa;
	}
	return TRXHIP_OK;
}

int trxhip_rx_sched_counters(trxhip_rx_sched *s, int chan, trxhip_rx_sched_ctrs *out)
{
	if (!chan_ok(s, chan) || !out)
		return TRXHIP_EINVAL;
	unsigned long long v[2] = { 0, 0 };
	if (s->ctx) {
		if (wait_pulls(s) != TRXHIP_OK || hipMemcpy(v, s->d_ctrs + 2 * chan, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
			return TRXHIP_EIO;
	}
	out->rx_empty_burst = 0;                                       /* a radioVector without paths cannot be formed here (:733-738) */
	out->rx_clipping = v[0];
	out->rx_no_burst_detected = v[1];
	return TRXHIP_OK;
}

int trxhip_rx_sched_noise_state(trxhip_rx_sched *s, int chan, float *ring20, uint32_t *itr, float *lev)
{
	if (!chan_ok(s, chan) || !ring20 || !itr || !lev)
		return TRXHIP_EINVAL;
	trx_rxs_noise v;
	memset(&v, 0, sizeof(v));
	if (s->ctx) {
		if (wait_pulls(s) != TRXHIP_OK ||
		    hipMemcpy(&v, s->d_noise + (size_t)s->noise_half * s->cfg.chans + chan, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
			return TRXHIP_EIO;
	}
	memcpy(ring20, v.ring, sizeof(v.ring));
	*itr = v.itr;
	*lev = v.lev;
	return TRXHIP_OK;
}

}  // extern "C"
