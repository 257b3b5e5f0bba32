// trx_air.hip -- the air interface for gfx950: a group of N MSs and one BTS joined on the device.  include/trxhip.h ("the air
// interface") is the contract, trx_air.h its arithmetic; this file holds the kernels, the host object's plain loop over the same
// inline functions, and the C ABI.
//
// UPLINK (the hot path: N x n x 4 bytes in, n x 4 out).  A block is four waves over one tile of 64 samples; lane l of every
// wave takes sample 64 tile + l, so a wave's read of a member row is one coalesced run of 256 bytes.  The members of the block's
// share (blockIdx.y of gridDim.y shares) are dealt to the four waves in turn: the path row is a wave-uniform load, the sample a
// vector load, the two table reads hit 16 KB that stay in cache, and a zero sample is skipped before them.  The waves' integer
// partials meet in LDS (3 x 64 x 16 bytes); wave 0 adds them.  With one share it adds the noise and writes the int16; with more
// it writes its 64 x 16 bytes into a partial buffer [share][n] that a second, small kernel sums.  Shares are chosen so that a
// frame of 5000 samples under 4096 members still starts about eight blocks per CU.  A window long enough to fill the chip with
// blocks of 256 samples takes the instance without the split: one sample per thread, every member, no LDS.
// Partials are 64-bit throughout: a member contributes up to 46342 * 4096 = 1.9e8 per component, so no 32-bit bound holds past
// 11 members at the largest gain, and the two extra adds per member hide behind the loads.
// DOWNLINK: one thread per (member, sample), a block per 256 samples, members on blockIdx.y.
// HISTORY: the last max_delay samples of every source row, a ring per row written by a launch behind the mix (trx_air.h:
// trx_air_win); the mix reads it only where ts - delay lies in front of the window.
// Per call: one table copy from one of four pinned areas taken in turn, at most three launches, one event.
// RAYS: a direction in which a path has rays (trxhip_multipath_set) keeps one flat list of ray entries on the device instead of
// the per-call table -- a plain member of it is one entry -- and runs air_ul_rays_kernel / air_dl_rays_kernel over the entries;
// the list is copied by the first window after a set call that changed it and by no other.  A ray that does not rotate carries
// its phasor and reads no table; the long-window instance puts the tables into LDS when the list has rotating rays (measured
// both ways).  A direction without rays issues what it issued before they existed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/trxhip.h"
#include "trx_air.h"
#include "trx_ctx.h"
#include "trx_mem.h"

namespace {

constexpr int kWave = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWave * kWaves;
constexpr unsigned kMaxY = 65535;
constexpr int kAreas = 4;
constexpr unsigned kTabTiles = 4;       /* tiles a block of the LDS-table instance walks behind one copy of the tables */

static_assert(sizeof(trx_air_row) == 16 && sizeof(trx_air_rx) == 16 && sizeof(trx_air_s16) == 4, "records");
static_assert(sizeof(trxhip_air_path) == 16 && sizeof(trxhip_air_path_status) == 48, "public air structs");
static_assert(sizeof(trx_air_ray) == 32 && sizeof(trx_air_span) == 8 && sizeof(trxhip_multipath_ray) == 24, "ray records");
static_assert(TRX_AIR_MAX_RAYS == TRXHIP_MULTIPATH_MAX_RAYS, "rays per path");

struct part2 {
	long long re, im;
};

__device__ inline trx_air_s16 air_finish(long long ar, long long ai, const trx_air_rx rx, int64_t ts)
{
	ar += trx_air_nq(rx.scale, trx_air_noise_s(rx.key_re, ts));
	ai += trx_air_nq(rx.scale, trx_air_noise_s(rx.key_im, ts));
	return trx_air_s16{trx_air_out(ar), trx_air_out(ai)};
}

/* the contribution of sample x of the path r to output sample i; a zero sample reads no table */
__device__ inline void air_add(const float *__restrict__ nco, trx_air_s16 x, const trx_air_row &r, unsigned i, long long &ar, long long &ai)
{
	if (x.re | x.im) {
		int32_t cr, ci;
		trx_air_path(nco, x.re, x.im, r.phase0 + i * (uint32_t)r.inc, r.g256, &cr, &ci);
		ar += cr;
		ai += ci;
	}
}

/* SPLIT: the block's members are dealt to its four waves over one tile of 64 samples, partials meet in LDS.  !SPLIT: every thread
 * takes one of 256 samples and all members of the share -- no LDS, a quarter of the blocks: for windows long enough to fill the
 * chip without splitting the members */
template <bool FINAL, bool SPLIT>
__global__ void __launch_bounds__(kThreads)
air_ul_mix_kernel(const trx_air_s16 *__restrict__ tx, size_t stride, const trx_air_s16 *__restrict__ ring, const trx_air_row *__restrict__ tab,
		  unsigned n_members, unsigned per_share, trx_air_win w, trx_air_rx rx, const float *__restrict__ nco, part2 *__restrict__ part,
		  trx_air_s16 *__restrict__ out)
{
	__shared__ part2 lds[SPLIT ? kWaves - 1 : 1][SPLIT ? kWave : 1];
	const unsigned lane = threadIdx.x & (kWave - 1);
	const unsigned wave = SPLIT ? __builtin_amdgcn_readfirstlane(threadIdx.x / kWave) : 0u;
	const unsigned i = SPLIT ? blockIdx.x * kWave + lane : blockIdx.x * kThreads + threadIdx.x;      /* n < 2^31: no wrap */
	const unsigned m0 = blockIdx.y * per_share;
	const unsigned m1 = m0 + per_share < n_members ? m0 + per_share : n_members;
	long long ar = 0, ai = 0;
	if (i < w.n) {
		/* four members at a time: their rows and samples are fetched before the first is used, so four loads are in flight */
		constexpr unsigned kStep = SPLIT ? kWaves : 1, kAhead = 4;
		unsigned m = m0 + wave;
		for (; m + (kAhead - 1) * kStep < m1; m += kAhead * kStep) {
			trx_air_row r[kAhead];
			trx_air_s16 x[kAhead];
#pragma unroll
			for (unsigned u = 0; u < kAhead; u++)
				r[u] = tab[m + u * kStep];
#pragma unroll
			for (unsigned u = 0; u < kAhead; u++)
				x[u] = trx_air_fetch(tx + (size_t)(m + u * kStep) * stride, ring + (size_t)(m + u * kStep) * w.H, w,
						     (int64_t)i - (int64_t)r[u].delay);
#pragma unroll
			for (unsigned u = 0; u < kAhead; u++)
				air_add(nco, x[u], r[u], i, ar, ai);
		}
		for (; m < m1; m += kStep) {
			const trx_air_row r = tab[m];
			air_add(nco, trx_air_fetch(tx + (size_t)m * stride, ring + (size_t)m * w.H, w, (int64_t)i - (int64_t)r.delay), r, i, ar, ai);
		}
	}
	if (SPLIT) {
		if (wave)
			lds[wave - 1][lane] = part2{ar, ai};
		__syncthreads();
		if (wave == 0)
			for (int k = 0; k < kWaves - 1; k++) {
				ar += lds[k][lane].re;
				ai += lds[k][lane].im;
			}
	}
	if (wave || i >= w.n)
		return;
	if (FINAL)
		out[i] = air_finish(ar, ai, rx, w.first_ts + (int64_t)i);
	else
		part[(size_t)blockIdx.y * w.n + i] = part2{ar, ai};
}

__global__ void __launch_bounds__(kThreads)
air_ul_sum_kernel(const part2 *__restrict__ part, unsigned shares, trx_air_win w, trx_air_rx rx, trx_air_s16 *__restrict__ out)
{
	const unsigned i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= w.n)
		return;
	long long ar = 0, ai = 0;
	for (unsigned s = 0; s < shares; s++) {
		const part2 p = part[(size_t)s * w.n + i];
		ar += p.re;
		ai += p.im;
	}
	out[i] = air_finish(ar, ai, rx, w.first_ts + (int64_t)i);
}

__global__ void __launch_bounds__(kThreads)
air_dl_kernel(const trx_air_s16 *__restrict__ in, const trx_air_s16 *__restrict__ ring, const trx_air_row *__restrict__ tab,
	      const trx_air_rx *__restrict__ rxs, unsigned n_members, trx_air_win w, const float *__restrict__ nco, trx_air_s16 *__restrict__ out,
	      size_t out_stride)
{
	const unsigned i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= w.n)
		return;
	for (unsigned m = blockIdx.y; m < n_members; m += gridDim.y) {
		const trx_air_row r = tab[m];
		const trx_air_s16 x = trx_air_fetch(in, ring, w, (int64_t)i - (int64_t)r.delay);
		int32_t cr = 0, ci = 0;
		if (x.re | x.im)
			trx_air_path(nco, x.re, x.im, r.phase0 + i * (uint32_t)r.inc, r.g256, &cr, &ci);
		out[(size_t)m * out_stride + i] = air_finish(cr, ci, rxs[m], w.first_ts + (int64_t)i);
	}
}

/* the last `len` samples of every source row's window into its ring, from place q0 on */
__global__ void __launch_bounds__(kThreads)
air_save_kernel(const trx_air_s16 *__restrict__ src, size_t stride, unsigned n_rows, unsigned n, unsigned len, unsigned H, unsigned q0,
		trx_air_s16 *__restrict__ ring)
{
	const unsigned k = blockIdx.x * kThreads + threadIdx.x;
	if (k >= len)
		return;
	unsigned q = q0 + k;
	if (q >= H)
		q -= H;
	for (unsigned r = blockIdx.y; r < n_rows; r += gridDim.y)
		ring[(size_t)r * H + q] = src[(size_t)r * stride + (n - len) + k];
}

/* ---- rays (include/trxhip.h, "multipath rays"): these kernels run only in a direction where a path has rays ------------------ */

/* the contribution of sample x through the list entry r to the output sample whose timestamp is ts32 modulo 2^32.  r is
 * wave-uniform, so is the branch: a ray that does not rotate brings its phasor along and reads no table */
__device__ inline void air_add_ray(const float *__restrict__ nco, trx_air_s16 x, const trx_air_ray &r, uint32_t ts32, long long &ar, long long &ai)
{
	if (x.re | x.im) {
		float rc = r.rc, rs = r.rs, yr, yi;
		if (r.inc != 0)
			trx_nco_phasor(nco, r.phase_at_0 + ts32 * (uint32_t)r.inc, &rc, &rs);
		trx_nco_rotate((float)x.re, (float)x.im, rc, rs, &yr, &yi);
		ar += trx_air_contrib(yr, r.g256);
		ai += trx_air_contrib(yi, r.g256);
	}
}

/* air_ul_mix_kernel's tiling over the entries of the ray list instead of the members: a share is per_share consecutive entries,
 * whichever members they belong to, so a member with many rays does not weigh on one block.
 * TABS: the block copies the 16 KB of phasor tables into LDS once and then walks the tiles blockIdx.x, + gridDim.x, ...; the
 * (cos, sin) pairs keep their layout, so a phasor is two 8-byte LDS reads: neighbouring samples share the coarse entry (one
 * address, a broadcast) and spread over the fine table (banks per half-wave, two to a pair).  !TABS: one tile per block, the
 * tables through the cache.  Launched: TABS only with !SPLIT, for long windows whose list has rotating rays */
template <bool FINAL, bool SPLIT, bool TABS>
__global__ void __launch_bounds__(kThreads)
air_ul_rays_kernel(const trx_air_s16 *__restrict__ tx, size_t stride, const trx_air_s16 *__restrict__ ring, const trx_air_ray *__restrict__ list,
		   unsigned n_entries, unsigned per_share, trx_air_win w, trx_air_rx rx, const float *__restrict__ nco, part2 *__restrict__ part,
		   trx_air_s16 *__restrict__ out)
{
	__shared__ part2 lds[SPLIT ? kWaves - 1 : 1][SPLIT ? kWave : 1];
	__shared__ __align__(16) float tabs[TABS ? TRX_NCO_FLOATS : 4];
	constexpr unsigned kTile = SPLIT ? kWave : kThreads;
	const unsigned lane = threadIdx.x & (kWave - 1);
	const unsigned wave = SPLIT ? __builtin_amdgcn_readfirstlane(threadIdx.x / kWave) : 0u;
	const unsigned e0 = blockIdx.y * per_share;
	const unsigned e1 = e0 + per_share < n_entries ? e0 + per_share : n_entries;
	const unsigned n_tiles = (w.n + kTile - 1) / kTile;
	if (TABS) {
		for (unsigned k = threadIdx.x; k < TRX_NCO_FLOATS / 4; k += kThreads)
			reinterpret_cast<float4 *>(tabs)[k] = reinterpret_cast<const float4 *>(nco)[k];
		__syncthreads();
	}
	const float *tab = TABS ? tabs : nco;
	for (unsigned tile = blockIdx.x; tile < n_tiles; tile += TABS ? gridDim.x : n_tiles) {
		const unsigned i = tile * kTile + (SPLIT ? lane : threadIdx.x);      /* n < 2^31: no wrap */
		const uint32_t ts32 = (uint32_t)(uint64_t)w.first_ts + i;
		long long ar = 0, ai = 0;
		if (i < w.n) {
			constexpr unsigned kStep = SPLIT ? kWaves : 1, kAhead = 4;
			unsigned e = e0 + wave;
			for (; e + (kAhead - 1) * kStep < e1; e += kAhead * kStep) {
				trx_air_ray r[kAhead];
				trx_air_s16 x[kAhead];
#pragma unroll
				for (unsigned u = 0; u < kAhead; u++)
					r[u] = list[e + u * kStep];
#pragma unroll
				for (unsigned u = 0; u < kAhead; u++)
					x[u] = trx_air_fetch(tx + (size_t)r[u].row * stride, ring + (size_t)r[u].row * w.H, w,
							     (int64_t)i - (int64_t)r[u].delay);
#pragma unroll
				for (unsigned u = 0; u < kAhead; u++)
					air_add_ray(tab, x[u], r[u], ts32, ar, ai);
			}
			for (; e < e1; e += kStep) {
				const trx_air_ray r = list[e];
				air_add_ray(tab, trx_air_fetch(tx + (size_t)r.row * stride, ring + (size_t)r.row * w.H, w, (int64_t)i - (int64_t)r.delay), r,
					    ts32, ar, ai);
			}
		}
		if (SPLIT) {
			if (wave)
				lds[wave - 1][lane] = part2{ar, ai};
			__syncthreads();
			if (wave == 0)
				for (int k = 0; k < kWaves - 1; k++) {
					ar += lds[k][lane].re;
					ai += lds[k][lane].im;
				}
			if (TABS)
				__syncthreads();       /* the next tile writes the partials again */
		}
		if (wave == 0 && i < w.n) {
			if (FINAL)
				out[i] = air_finish(ar, ai, rx, w.first_ts + (int64_t)i);
			else
				part[(size_t)blockIdx.y * w.n + i] = part2{ar, ai};
		}
	}
}

/* one thread per (member, sample): the member's entries summed in 64 bits, then its receiver's noise */
__global__ void __launch_bounds__(kThreads)
air_dl_rays_kernel(const trx_air_s16 *__restrict__ in, const trx_air_s16 *__restrict__ ring, const trx_air_ray *__restrict__ list,
		   const trx_air_span *__restrict__ span, const trx_air_rx *__restrict__ rxs, unsigned n_members, trx_air_win w,
		   const float *__restrict__ nco, trx_air_s16 *__restrict__ out, size_t out_stride)
{
	const unsigned i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= w.n)
		return;
	const uint32_t ts32 = (uint32_t)(uint64_t)w.first_ts + i;
	for (unsigned m = blockIdx.y; m < n_members; m += gridDim.y) {
		const trx_air_span s = span[m];
		long long ar = 0, ai = 0;
		for (unsigned e = s.first; e < s.first + s.count; e++) {
			const trx_air_ray r = list[e];
			air_add_ray(nco, trx_air_fetch(in, ring, w, (int64_t)i - (int64_t)r.delay), r, ts32, ar, ai);
		}
		out[(size_t)m * out_stride + i] = air_finish(ar, ai, rxs[m], w.first_ts + (int64_t)i);
	}
}

struct Area {
	trx_pin<uint8_t> h;
	trx_event ev;              /* pending: the call that read the area last */
};

struct Ray {
	float gain;
	uint32_t delay;
	double hz;
	int32_t inc;
	uint32_t phase_at_0;
};

struct Path {
	float gain = 1.0f;
	uint32_t delay = 0;
	trx_nco_state osc{0, 0u, 0, 0.0, false};
	int32_t noise_scale = 0;   /* downlink: the member's receiver; uplink: member 0's entry is the BTS's */
	std::vector<Ray> rays;     /* not empty: the path's output is theirs; the plain state above lives on beside them */
	int64_t rays_ts = 0;       /* end_ts at the last trxhip_multipath_set */
};

struct Dir {
	std::vector<Path> path;
	bool started = false;
	int64_t end_ts = 0;        /* where the next window starts; what set_path acts at */
	int64_t start_ts = 0;      /* the first sample since creation or the last reset */
	uint32_t p0 = 0;           /* end_ts's place in the rings */
	std::vector<trx_air_s16> h_ring;       /* host object */
	trx_dev<trx_air_s16> d_ring;
	trx_dev<uint8_t> d_tab;
	trx_dev<part2> d_part;     /* uplink */
	Area area[kAreas];
	unsigned next_area = 0;
	uint32_t n_rayed = 0;      /* paths with rays; 0: the direction issues what it issued before rays existed */
	bool list_dirty = true;    /* the ray list on the device is not what the paths say */
	uint32_t n_entries = 0;    /* of the list on the device */
	uint32_t n_rotating = 0;   /* those of them with inc != 0 */
	trx_dev<uint8_t> d_list;
};

}  // namespace

struct trxhip_air {
	trxhip_ctx *ctx = nullptr;
	uint32_t n = 0, H = 0, seed = 0;
	std::vector<float> nco_tab;            /* host object */
	Dir dir[2];
};

namespace {

size_t n_src_rows(const trxhip_air *a, int dir) { return dir == TRXHIP_AIR_UL ? a->n : 1; }

trx_air_rx rx_of(const trxhip_air *a, int dir, uint32_t m)
{
	const uint32_t rx = dir == TRXHIP_AIR_UL ? TRX_AIR_UL_RX : m;
	return trx_air_rx{a->dir[dir].path[dir == TRXHIP_AIR_UL ? 0 : m].noise_scale, trx_air_lane_key(a->seed, 2 * rx),
			  trx_air_lane_key(a->seed, 2 * rx + 1), 0u};
}

/* the table of a window that starts at first_ts: n path rows, then (downlink) n receivers */
void fill_table(const trxhip_air *a, int dir, int64_t first_ts, uint8_t *dst)
{
	const Dir &d = a->dir[dir];
	trx_air_row *rows = reinterpret_cast<trx_air_row *>(dst);
	for (uint32_t m = 0; m < a->n; m++) {
		const Path &p = d.path[m];
		rows[m] = trx_air_row{trx_nco_phase(p.osc.acc, p.osc.ts_ref, p.osc.inc, first_ts), p.osc.inc, p.gain * 256.0f, p.delay};
	}
	if (dir == TRXHIP_AIR_DL) {
		trx_air_rx *rxs = reinterpret_cast<trx_air_rx *>(rows + a->n);
		for (uint32_t m = 0; m < a->n; m++)
			rxs[m] = rx_of(a, dir, m);
	}
}

size_t table_bytes(const trxhip_air *a, int dir) { return (size_t)a->n * (dir == TRXHIP_AIR_DL ? 32 : 16); }

/* the entries of the direction's ray list: a path's rays, or one for a plain path */
uint32_t list_entries(const trxhip_air *a, int dir)
{
	size_t e = 0;
	for (const Path &p : a->dir[dir].path)
		e += std::max<size_t>(p.rays.size(), 1);
	return (uint32_t)e;                     /* <= 4096 * 64 */
}

/* entries, then (downlink) the members' spans and their receivers */
size_t list_bytes(const trxhip_air *a, int dir, uint32_t entries)
{
	return (size_t)entries * sizeof(trx_air_ray) + (dir == TRXHIP_AIR_DL ? (size_t)a->n * (sizeof(trx_air_span) + sizeof(trx_air_rx)) : 0);
}

trx_air_ray list_entry(const float *tab, uint32_t phase_at_0, int32_t inc, float gain, uint32_t delay, uint32_t row)
{
	trx_air_ray r{phase_at_0, inc, gain * 256.0f, delay, row, 0.0f, 0.0f, 0u};
	if (inc == 0)
		trx_nco_phasor(tab, phase_at_0, &r.rc, &r.rs);
	return r;
}

/* the list, sorted by member; it holds no timestamp of a window, so it stays good until a path or a receiver changes */
void fill_list(const trxhip_air *a, int dir, uint32_t entries, uint8_t *dst)
{
	const Dir &d = a->dir[dir];
	const float *tab = a->nco_tab.data();
	trx_air_ray *list = reinterpret_cast<trx_air_ray *>(dst);
	trx_air_span *span = reinterpret_cast<trx_air_span *>(list + entries);
	uint32_t e = 0;
	for (uint32_t m = 0; m < a->n; m++) {
		const Path &p = d.path[m];
		const uint32_t row = dir == TRXHIP_AIR_UL ? m : 0u, first = e;
		if (p.rays.empty())
			list[e++] = list_entry(tab, trx_air_phase_at_0(p.osc.acc, p.osc.ts_ref, p.osc.inc), p.osc.inc, p.gain, p.delay, row);
		for (const Ray &r : p.rays)
			list[e++] = list_entry(tab, r.phase_at_0, r.inc, r.gain, r.delay, row);
		if (dir == TRXHIP_AIR_DL)
			span[m] = trx_air_span{first, e - first};
	}
	if (dir == TRXHIP_AIR_DL) {
		trx_air_rx *rxs = reinterpret_cast<trx_air_rx *>(span + a->n);
		for (uint32_t m = 0; m < a->n; m++)
			rxs[m] = rx_of(a, dir, m);
	}
}

/* the host object: the plain loop over trx_air.h */
void host_path(const float *tab, const Path &p, const trx_air_row &row, const trx_air_s16 *src, const trx_air_s16 *ring, const trx_air_win &w,
	       uint32_t i, int64_t *ar, int64_t *ai)
{
	int32_t cr, ci;
	if (p.rays.empty()) {
		const trx_air_s16 x = trx_air_fetch(src, ring, w, (int64_t)i - (int64_t)row.delay);
		trx_air_path(tab, x.re, x.im, row.phase0 + i * (uint32_t)row.inc, row.g256, &cr, &ci);
		*ar += cr;
		*ai += ci;
		return;
	}
	for (const Ray &r : p.rays) {
		const trx_air_s16 x = trx_air_fetch(src, ring, w, (int64_t)i - (int64_t)r.delay);
		trx_air_path(tab, x.re, x.im, trx_air_ray_phase(r.phase_at_0, r.inc, w.first_ts + (int64_t)i), r.gain * 256.0f, &cr, &ci);
		*ar += cr;
		*ai += ci;
	}
}

void host_window(trxhip_air *a, int dir, const trx_air_s16 *src, size_t src_stride, const trx_air_win &w, const uint8_t *table, trx_air_s16 *dst,
		 size_t dst_stride)
{
	Dir &d = a->dir[dir];
	const trx_air_row *rows = reinterpret_cast<const trx_air_row *>(table);
	const float *tab = a->nco_tab.data();
	if (dir == TRXHIP_AIR_UL) {
		const trx_air_rx rx = rx_of(a, dir, 0);
		for (uint32_t i = 0; i < w.n; i++) {
			int64_t ar = 0, ai = 0;
			for (uint32_t m = 0; m < a->n; m++)
				host_path(tab, d.path[m], rows[m], src + (size_t)m * src_stride, d.h_ring.data() + (size_t)m * w.H, w, i, &ar, &ai);
			const int64_t ts = w.first_ts + (int64_t)i;
			ar += trx_air_nq(rx.scale, trx_air_noise_s(rx.key_re, ts));
			ai += trx_air_nq(rx.scale, trx_air_noise_s(rx.key_im, ts));
			dst[i] = trx_air_s16{trx_air_out(ar), trx_air_out(ai)};
		}
	} else {
		const trx_air_rx *rxs = reinterpret_cast<const trx_air_rx *>(rows + a->n);
		for (uint32_t m = 0; m < a->n; m++)
			for (uint32_t i = 0; i < w.n; i++) {
				int64_t ar = 0, ai = 0;
				host_path(tab, d.path[m], rows[m], src, d.h_ring.data(), w, i, &ar, &ai);
				const int64_t ts = w.first_ts + (int64_t)i;
				ar += trx_air_nq(rxs[m].scale, trx_air_noise_s(rxs[m].key_re, ts));
				ai += trx_air_nq(rxs[m].scale, trx_air_noise_s(rxs[m].key_im, ts));
				dst[(size_t)m * dst_stride + i] = trx_air_s16{trx_air_out(ar), trx_air_out(ai)};
			}
	}
}

/* uplink: the blocks that fill the chip, eight per CU (eight waves per SIMD at four waves a block) */
size_t ul_blocks_wanted(const trxhip_air *a) { return (size_t)8 * (a->ctx->n_cu > 0 ? a->ctx->n_cu : 256); }

/* uplink shares: enough of them to fill the chip with tiles of 64 samples, at least 8 members to a share */
unsigned ul_shares(const trxhip_air *a, uint32_t n)
{
	const size_t tiles = ((size_t)n + kWave - 1) / kWave;
	size_t s = (ul_blocks_wanted(a) + tiles - 1) / tiles;
	s = std::min(s, (size_t)(a->n + 7) / 8);
	return (unsigned)std::max<size_t>(s, 1);
}

/* a window of a direction with rays.  The list is resident: it is copied (from the window's area, as the table is) only when a
 * set call has changed it since the last window.  ul_shares' rule on entries instead of members */
int device_window_rays(trxhip_air *a, int dir, const trx_air_s16 *src, size_t src_stride, const trx_air_win &w, uint32_t len, uint32_t q0,
		       trx_air_s16 *dst, size_t dst_stride, hipStream_t st)
{
	Dir &d = a->dir[dir];
	if (with_device(a->ctx))
		return TRXHIP_EIO;
	const uint32_t entries = d.list_dirty ? list_entries(a, dir) : d.n_entries;
	const size_t bytes = list_bytes(a, dir, entries);
	Area &ar = d.area[d.next_area % kAreas];
	int rc = ar.ev.create();
	if (rc == TRXHIP_OK)
		rc = ar.ev.wait();
	unsigned shares = 1, per_share = entries;
	if (rc == TRXHIP_OK && dir == TRXHIP_AIR_UL) {
		const size_t tiles = ((size_t)w.n + kWave - 1) / kWave;
		shares = (unsigned)std::max<size_t>(std::min((ul_blocks_wanted(a) + tiles - 1) / tiles, ((size_t)entries + 7) / 8), 1);
		per_share = (entries + shares - 1) / shares;
		shares = (entries + per_share - 1) / per_share;
	}
	const bool grow_list = d.list_dirty && d.d_list.cap < bytes, grow_part = shares > 1 && d.d_part.cap < (size_t)shares * w.n;
	if (rc == TRXHIP_OK && (grow_list || grow_part)) {
		/* the launches that used the smaller buffers are behind the events of the areas */
		for (Area &o : d.area)
			if (o.ev.wait() != TRXHIP_OK)
				return TRXHIP_EIO;
		if (grow_list)
			rc = d.d_list.reserve(bytes);
		if (rc == TRXHIP_OK && grow_part)
			rc = d.d_part.reserve((size_t)shares * w.n);
	}
	if (rc == TRXHIP_OK && d.list_dirty)
		rc = ar.h.reserve(bytes);
	if (rc != TRXHIP_OK)
		return rc;
	d.next_area++;
	if (d.list_dirty) {
		fill_list(a, dir, entries, ar.h);
		if (hipMemcpyAsync(d.d_list, ar.h, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
			return TRXHIP_EIO;
		d.n_entries = entries;
		d.n_rotating = 0;
		for (uint32_t e = 0; e < entries; e++)
			d.n_rotating += reinterpret_cast<const trx_air_ray *>(ar.h.p)[e].inc != 0;
		d.list_dirty = false;
	}
	const trx_air_ray *list = reinterpret_cast<const trx_air_ray *>(d.d_list.p);
	const float *nco = a->ctx->d_nco_tab;
	if (dir == TRXHIP_AIR_UL) {
		const trx_air_rx rx = rx_of(a, dir, 0);
		const unsigned long_blocks = (w.n + kThreads - 1) / kThreads, tile_blocks = (w.n + kWave - 1) / kWave;
#define RAYS_LAUNCH(FINAL, SPLIT, TABS, gx, gy)                                                                                          \
	hipLaunchKernelGGL((air_ul_rays_kernel<FINAL, SPLIT, TABS>), dim3(gx, gy), dim3(kThreads), 0, st, src, src_stride, d.d_ring.p, list,     \
			   entries, per_share, w, rx, nco, d.d_part.p, dst)
		if (shares == 1 && long_blocks >= ul_blocks_wanted(a) / 2) {
			/* the long window: with rotating rays in the list the tables go to LDS and a block walks kTabTiles tiles (measured,
			 * 2.50 against 3.59 ms on dense rows; under the tiles of 64 samples the cache form is the faster one) */
			if (d.n_rotating)
				RAYS_LAUNCH(true, false, true, (long_blocks + kTabTiles - 1) / kTabTiles, 1);
			else
				RAYS_LAUNCH(true, false, false, long_blocks, 1);
		} else if (shares == 1) {
			RAYS_LAUNCH(true, true, false, tile_blocks, 1);
		} else {
			RAYS_LAUNCH(false, true, false, tile_blocks, shares);
			hipLaunchKernelGGL(air_ul_sum_kernel, dim3((w.n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d.d_part.p, shares, w, rx, dst);
		}
#undef RAYS_LAUNCH
	} else {
		const trx_air_span *span = reinterpret_cast<const trx_air_span *>(list + entries);
		const dim3 grid((w.n + kThreads - 1) / kThreads, std::min<unsigned>(a->n, kMaxY));
		hipLaunchKernelGGL(air_dl_rays_kernel, grid, dim3(kThreads), 0, st, src, d.d_ring.p, list, span,
				   reinterpret_cast<const trx_air_rx *>(span + a->n), a->n, w, nco, dst, dst_stride);
	}
	if (len) {
		const dim3 grid((len + kThreads - 1) / kThreads, (unsigned)std::min<size_t>(n_src_rows(a, dir), kMaxY));
		hipLaunchKernelGGL(air_save_kernel, grid, dim3(kThreads), 0, st, src, src_stride, (unsigned)n_src_rows(a, dir), w.n, len, w.H, q0,
				   d.d_ring.p);
	}
	if (hipGetLastError() != hipSuccess)
		return TRXHIP_EIO;
	if (ar.ev.record(st) != TRXHIP_OK)
		(void)hipStreamSynchronize(st);   /* no event: the area is free once the stream has drained */
	return TRXHIP_OK;
}

int device_window(trxhip_air *a, int dir, const trx_air_s16 *src, size_t src_stride, const trx_air_win &w, uint32_t len, uint32_t q0,
		  trx_air_s16 *dst, size_t dst_stride, hipStream_t st)
{
	Dir &d = a->dir[dir];
	if (d.n_rayed)
		return device_window_rays(a, dir, src, src_stride, w, len, q0, dst, dst_stride, st);
	if (with_device(a->ctx))
		return TRXHIP_EIO;
	const size_t bytes = table_bytes(a, dir);
	Area &ar = d.area[d.next_area % kAreas];
	int rc = ar.ev.create();
	if (rc == TRXHIP_OK)
		rc = ar.ev.wait();
	if (rc == TRXHIP_OK)
		rc = ar.h.reserve(bytes);
	if (rc == TRXHIP_OK)
		rc = d.d_tab.reserve(bytes);
	unsigned shares = 1, per_share = a->n;
	if (rc == TRXHIP_OK && dir == TRXHIP_AIR_UL) {
		shares = ul_shares(a, w.n);
		per_share = (a->n + shares - 1) / shares;
		shares = (a->n + per_share - 1) / per_share;
		if (shares > 1 && d.d_part.cap < (size_t)shares * w.n) {
			/* the launches that used the smaller buffer are behind the events of the areas */
			for (Area &o : d.area)
				if (o.ev.wait() != TRXHIP_OK)
					return TRXHIP_EIO;
			rc = d.d_part.reserve((size_t)shares * w.n);
		}
	}
	if (rc != TRXHIP_OK)
		return rc;
	d.next_area++;
	fill_table(a, dir, w.first_ts, ar.h);
	if (hipMemcpyAsync(d.d_tab, ar.h, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
		return TRXHIP_EIO;
	const trx_air_row *rows = reinterpret_cast<const trx_air_row *>(d.d_tab.p);
	const float *nco = a->ctx->d_nco_tab;
	if (dir == TRXHIP_AIR_UL) {
		const trx_air_rx rx = rx_of(a, dir, 0);
		if (shares == 1 && ((size_t)w.n + kThreads - 1) / kThreads >= ul_blocks_wanted(a) / 2) {     /* whole blocks of four busy waves */
			hipLaunchKernelGGL((air_ul_mix_kernel<true, false>), dim3((w.n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, src, src_stride,
					   d.d_ring.p, rows, a->n, per_share, w, rx, nco, (part2 *)nullptr, dst);
		} else if (shares == 1) {
			hipLaunchKernelGGL((air_ul_mix_kernel<true, true>), dim3((w.n + kWave - 1) / kWave), dim3(kThreads), 0, st, src, src_stride,
					   d.d_ring.p, rows, a->n, per_share, w, rx, nco, (part2 *)nullptr, dst);
		} else {
			hipLaunchKernelGGL((air_ul_mix_kernel<false, true>), dim3((w.n + kWave - 1) / kWave, shares), dim3(kThreads), 0, st, src,
					   src_stride, d.d_ring.p, rows, a->n, per_share, w, rx, nco, d.d_part.p, dst);
			hipLaunchKernelGGL(air_ul_sum_kernel, dim3((w.n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d.d_part.p, shares, w, rx, dst);
		}
	} else {
		const dim3 grid((w.n + kThreads - 1) / kThreads, std::min<unsigned>(a->n, kMaxY));
		hipLaunchKernelGGL(air_dl_kernel, grid, dim3(kThreads), 0, st, src, d.d_ring.p, rows, reinterpret_cast<const trx_air_rx *>(rows + a->n),
				   a->n, w, nco, dst, dst_stride);
	}
	if (len) {
		const dim3 grid((len + kThreads - 1) / kThreads, (unsigned)std::min<size_t>(n_src_rows(a, dir), kMaxY));
		hipLaunchKernelGGL(air_save_kernel, grid, dim3(kThreads), 0, st, src, src_stride, (unsigned)n_src_rows(a, dir), w.n, len, w.H, q0,
				   d.d_ring.p);
	}
	if (hipGetLastError() != hipSuccess)
		return TRXHIP_EIO;
	if (ar.ev.record(st) != TRXHIP_OK)
		(void)hipStreamSynchronize(st);   /* no event: the area is free once the stream has drained */
	return TRXHIP_OK;
}

int air_window(trxhip_air *a, int dir, const int16_t *src, size_t src_stride, int64_t first_ts, size_t n, int16_t *dst, size_t dst_stride,
	       void *stream)
{
	if (!a || !src || (reinterpret_cast<uintptr_t>(src) & 3) || !dst || (reinterpret_cast<uintptr_t>(dst) & 3) || n == 0 || n > 0x7fffffffull ||
	    src_stride < n || dst_stride < n)
		return TRXHIP_EINVAL;
	Dir &d = a->dir[dir];
	if (d.started && first_ts != d.end_ts)
		return TRXHIP_EINVAL;
	const int64_t start_ts = d.started ? d.start_ts : first_ts;
	const uint64_t behind = (uint64_t)first_ts - (uint64_t)start_ts;
	const trx_air_win w{first_ts, (uint32_t)n, a->H, d.started ? d.p0 : 0u, (uint32_t)std::min<uint64_t>(behind, a->H)};
	const uint32_t len = (uint32_t)std::min<size_t>(n, a->H);
	uint32_t q0 = 0, p_next = 0;
	if (a->H) {
		q0 = (uint32_t)((w.p0 + (n - len)) % a->H);
		p_next = (uint32_t)((w.p0 + n) % a->H);
	}
	const trx_air_s16 *s = reinterpret_cast<const trx_air_s16 *>(src);
	trx_air_s16 *o = reinterpret_cast<trx_air_s16 *>(dst);
	if (a->ctx) {
		const int rc = device_window(a, dir, s, src_stride, w, len, q0, o, dst_stride, static_cast<hipStream_t>(stream));
		if (rc != TRXHIP_OK)
			return rc;
	} else {
		std::vector<uint8_t> table(table_bytes(a, dir));
		fill_table(a, dir, first_ts, table.data());
		host_window(a, dir, s, src_stride, w, table.data(), o, dst_stride);
		for (size_t r = 0; r < n_src_rows(a, dir); r++)
			for (uint32_t k = 0; k < len; k++)
				d.h_ring[r * a->H + (q0 + k) % a->H] = s[r * src_stride + (n - len) + k];
	}
	d.started = true;
	d.start_ts = start_ts;
	d.end_ts = (int64_t)((uint64_t)first_ts + n);
	d.p0 = p_next;
	return TRXHIP_OK;
}

bool bad_dir(int dir) { return dir != TRXHIP_AIR_UL && dir != TRXHIP_AIR_DL; }

}  // namespace

extern "C" {

int trxhip_air_create(trxhip_ctx *ctx, const trxhip_air_cfg *cfg, trxhip_air **out)
{
	if (!cfg || !out || cfg->n_members < 1 || cfg->n_members > TRX_AIR_MAX_MEMBERS || cfg->max_delay > TRX_AIR_MAX_DELAY)
		return TRXHIP_EINVAL;
	if (ctx && !ctx->d_nco_tab)
		return TRXHIP_EINVAL;
	trxhip_air *a = new (std::nothrow) trxhip_air;
	if (!a)
		return TRXHIP_ENOMEM;
	a->ctx = ctx;
	a->n = cfg->n_members;
	a->H = cfg->max_delay;
	a->seed = cfg->seed;
	int rc = TRXHIP_OK;
	try {
		for (int dir = 0; dir < 2; dir++) {
			a->dir[dir].path.resize(a->n);
			if (!ctx)
				a->dir[dir].h_ring.resize(n_src_rows(a, dir) * a->H);
		}
		if (!ctx) {
			a->nco_tab.resize(TRX_NCO_FLOATS);
			trx_nco_tables(a->nco_tab.data());
		}
	} catch (const std::bad_alloc &) {
		rc = TRXHIP_ENOMEM;
	}
	if (rc == TRXHIP_OK && ctx) {
		rc = with_device(ctx) ? TRXHIP_EIO : TRXHIP_OK;
		/* nothing reads a ring before the window that wrote it (trx_air_win.avail): no memset */
		for (int dir = 0; dir < 2 && rc == TRXHIP_OK; dir++)
			rc = a->dir[dir].d_ring.reserve(std::max<size_t>(n_src_rows(a, dir) * a->H, 1));
	}
	if (rc != TRXHIP_OK) {
		delete a;
		return rc;
	}
	*out = a;
	return TRXHIP_OK;
}

void trxhip_air_destroy(trxhip_air *a)
{
	if (!a)
		return;
	if (a->ctx)
		(void)with_device(a->ctx);
	/* an area's event goes (waited for) before its pinned block; the device blocks go behind every area */
	for (Dir &d : a->dir)
		for (Area &ar : d.area)
			ar.ev.reset();
	delete a;
}

int trxhip_air_set_path(trxhip_air *a, int dir, uint32_t member, const trxhip_air_path *p)
{
	int32_t inc;
	if (!a || !p || bad_dir(dir) || member >= a->n || !(p->gain >= 0.0f && p->gain <= TRX_AIR_MAX_GAIN) || p->delay > a->H ||
	    trx_nco_inc(p->hz, &inc) != 0)
		return TRXHIP_EINVAL;
	Dir &d = a->dir[dir];
	Path &q = d.path[member];
	q.gain = p->gain;
	q.delay = p->delay;
	trx_nco_set(&q.osc, p->hz != 0.0, p->hz, inc, d.end_ts);
	d.list_dirty = true;
	return TRXHIP_OK;
}

int trxhip_multipath_set(trxhip_air *a, int dir, uint32_t member, const trxhip_multipath_ray *rays, uint32_t n_rays)
{
	if (!a || bad_dir(dir) || member >= a->n || n_rays > TRX_AIR_MAX_RAYS || (n_rays && !rays))
		return TRXHIP_EINVAL;
	Dir &d = a->dir[dir];
	std::vector<Ray> v;
	try {
		v.reserve(n_rays);
		if (n_rays && a->nco_tab.empty()) {     /* a device object makes its host copy of the tables with its first rays */
			a->nco_tab.resize(TRX_NCO_FLOATS);
			trx_nco_tables(a->nco_tab.data());
		}
	} catch (const std::bad_alloc &) {
		return TRXHIP_ENOMEM;
	}
	for (uint32_t k = 0; k < n_rays; k++) {
		const trxhip_multipath_ray &r = rays[k];
		int32_t inc;
		if (!(r.gain >= 0.0f && r.gain <= TRX_AIR_MAX_GAIN) || r.delay > a->H || trx_nco_inc(r.hz, &inc) != 0 || r.reserved != 0)
			return TRXHIP_EINVAL;
		v.push_back(Ray{r.gain, r.delay, r.hz, inc, trx_air_phase_at_0(r.phase, d.end_ts, inc)});
	}
	Path &q = d.path[member];
	d.n_rayed += (v.empty() ? 0u : 1u) - (q.rays.empty() ? 0u : 1u);
	q.rays.swap(v);
	q.rays_ts = d.end_ts;
	d.list_dirty = true;
	return TRXHIP_OK;
}

int trxhip_multipath_state(const trxhip_air *a, int dir, uint32_t member, trxhip_multipath_ray *out, uint32_t cap, uint32_t *n_rays,
			   int64_t *ts_set)
{
	if (!a || bad_dir(dir) || member >= a->n || (cap && !out))
		return TRXHIP_EINVAL;
	const Dir &d = a->dir[dir];
	const Path &q = d.path[member];
	for (uint32_t k = 0; k < cap && k < q.rays.size(); k++) {
		const Ray &r = q.rays[k];
		out[k] = trxhip_multipath_ray{r.gain, r.delay, r.hz, trx_air_ray_phase(r.phase_at_0, r.inc, d.end_ts), 0u};
	}
	if (n_rays)
		*n_rays = (uint32_t)q.rays.size();
	if (ts_set)
		*ts_set = q.rays_ts;
	return TRXHIP_OK;
}

int trxhip_air_set_noise(trxhip_air *a, int dir, uint32_t member, double rms)
{
	int32_t scale;
	if (!a || bad_dir(dir) || (dir == TRXHIP_AIR_DL && member >= a->n) || trx_air_noise_scale(rms, &scale) != 0)
		return TRXHIP_EINVAL;
	a->dir[dir].path[dir == TRXHIP_AIR_UL ? 0 : member].noise_scale = scale;
	if (dir == TRXHIP_AIR_DL)           /* the downlink's receivers lie behind its ray list; the uplink's is a kernel argument */
		a->dir[dir].list_dirty = true;
	return TRXHIP_OK;
}

int trxhip_air_path_state(const trxhip_air *a, int dir, uint32_t member, trxhip_air_path_status *out)
{
	if (!a || !out || bad_dir(dir) || member >= a->n)
		return TRXHIP_EINVAL;
	const Dir &d = a->dir[dir];
	const Path &q = d.path[member];
	*out = trxhip_air_path_status{q.gain, q.delay, q.osc.hz, q.osc.inc, q.osc.acc, q.osc.ts_ref,
				      d.path[dir == TRXHIP_AIR_UL ? 0 : member].noise_scale, d.started ? 1u : 0u, d.end_ts};
	return TRXHIP_OK;
}

int trxhip_air_reset(trxhip_air *a, int dir, int64_t ts)
{
	if (!a || bad_dir(dir))
		return TRXHIP_EINVAL;
	Dir &d = a->dir[dir];
	d.started = true;
	d.start_ts = d.end_ts = ts;
	d.p0 = 0;
	return TRXHIP_OK;
}

int trxhip_air_uplink_s16(trxhip_air *a, const int16_t *d_tx, size_t tx_stride, int64_t first_ts, size_t n, int16_t *d_out, void *stream)
{
	return air_window(a, TRXHIP_AIR_UL, d_tx, tx_stride, first_ts, n, d_out, n, stream);
}

int trxhip_air_downlink_s16(trxhip_air *a, const int16_t *d_in, int64_t first_ts, size_t n, int16_t *d_out, size_t out_stride, void *stream)
{
	return air_window(a, TRXHIP_AIR_DL, d_in, n, first_ts, n, d_out, out_stride, stream);
}

int32_t trxhip_air_noise_host(uint32_t seed, uint32_t lane, int64_t ts, int32_t scale)
{
	int32_t largest;
	(void)trx_air_noise_scale(TRX_AIR_MAX_RMS, &largest);
	if (scale < 0 || scale > largest)       /* the product would leave 32 bits */
		return 0;
	return trx_air_nq(scale, trx_air_noise_s(trx_air_lane_key(seed, lane), ts));
}

}  // extern "C"
