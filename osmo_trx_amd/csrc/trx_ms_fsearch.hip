// trx_ms_fsearch.hip -- the MS-side FCCH search for gfx950: where in a buffer of samples, with no clock and at any carrier offset the
// estimator covers, the frequency-correction burst lies.  The reference has no such search (it trusts the radio's oscillator);
// include/trxhip.h ("MS-side FCCH search") defines this one, DESIGN §4o says why it is what it is.  Two launches per call:
//
// ms_fsearch_kernel<I16>: ONE WORKGROUP PER (ROW, SEGMENT) of TRX_FS_SEG = 256 grid windows.  It needs the sums of p[n] = x[n + 8]
//   conj(x[n]) and e[n] = |x[n]|^2 over 256 + 35 blocks of 16 samples.  Every lane takes four consecutive samples -- one 16-byte load
//   of x[n .. n + 3] and one of x[n + 8 .. n + 11] (int16; two of 16 bytes each for complex64), both coalesced, the second served by
//   the lines the first brought --, adds its four p and e, and four lanes make a block by two exchanges.  The block sums go to LDS.
//   int16: everything is int64 and exact, so three waves turn the three arrays into prefix sums (five entries per lane, a scan of the
//   lane totals over the wave) and a window's sums are differences of prefixes.  complex64: products and the 16-term block sums are
//   unfused float operations, everything above a block is double, and a window's sums are added block by block from LDS -- no
//   difference of prefixes, which would carry the rounding of everything in front of the window into it.  One lane per window
//   computes the score in double in the header's operation order; the workgroup reduces to its best window under the tie rule (the
//   larger score, of equal scores the lower pos) and the lane that owns it writes the candidate: one 64-byte record per workgroup.
// ms_fsearch_pick_kernel<I16>: ONE WAVE PER ROW reduces the row's candidates under the same rule, writes the hit, and runs
//   gsm_fcch_offset() (trx_ms_afc_dev.h, the estimator of trxhip_ms_fcch_batch_*) on the slot that begins at pos.
// No atomics, no host wait, no scratch; the candidates live in a work array of the context that grows on demand.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <type_traits>

#include "../../include/trxhip.h"
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_afc_dev.h"
#include "trx_ms_fsearch.h"

namespace {

constexpr int WAVE = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE;
constexpr int SEG = TRX_FS_SEG;
constexpr int LB_MAX = SEG + TRX_FS_BLOCKS - 1;                /* 291 block sums per segment */
constexpr int PER_LANE = 5;                                    /* entries per lane of the scan */
constexpr int PFX = WAVE * PER_LANE;                           /* 320 >= LB_MAX + 1 prefix entries */
constexpr int ITER = (LB_MAX * 4 + kThreads - 1) / kThreads;   /* 5 passes of 256 lanes x 4 samples */
constexpr unsigned kMaxGrid = 1u << 20;                        /* workgroups of a launch; the rest by grid stride */

static_assert(sizeof(trxhip_ms_fcch_hit) == 64 && TRX_FS_HOP == 16 && TRX_FS_W == 576 && TRX_FS_LAG == 8 && TRX_FS_BLOCKS == 36, "the search's record and constants");
static_assert(PFX >= LB_MAX + 1 && SEG == kThreads && TRX_FS_LAG % 4 == 0 && TRX_FS_HOP == 16, "one lane per window; a block is four lanes of four samples");
static_assert(TRX_FS_MIN_LEN > TRX_AFC_LAST, "the estimator's samples lie inside every window");

__device__ __forceinline__ unsigned uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

typedef int   v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

/* 16 bytes from an address that is only as aligned as a sample (4 bytes int16, 8 bytes complex64): one global_load_dwordx4 */
template <typename V, int ALIGN>
__device__ __forceinline__ V load16(const void *p)
{
	V v;
	__builtin_memcpy(&v, __builtin_assume_aligned(p, ALIGN), sizeof(V));
	return v;
}

/* p = a conj(b) and e = |b|^2 of one sample pair, added to the lane's sums */
__device__ __forceinline__ void mac_i16(int a, int b, long long &re, long long &im, long long &en)
{
	const int ar = (short)a, ai = a >> 16, br = (short)b, bi = b >> 16;      /* each product is below 2^30 in magnitude */
	re += (long long)(ar * br) + (long long)(ai * bi);
	im += (long long)(ai * br) - (long long)(ar * bi);
	en += (long long)(br * br) + (long long)(bi * bi);
}

__device__ __forceinline__ void mac_f32(float ar, float ai, float br, float bi, float &re, float &im, float &en)
{
	re = __fadd_rn(re, __fadd_rn(__fmul_rn(ar, br), __fmul_rn(ai, bi)));
	im = __fadd_rn(im, __fsub_rn(__fmul_rn(ai, br), __fmul_rn(ar, bi)));
	en = __fadd_rn(en, __fadd_rn(__fmul_rn(br, br), __fmul_rn(bi, bi)));
}

template <typename T>
__device__ __forceinline__ T quad_sum(T v)
{
	v += __shfl_xor(v, 1);
	v += __shfl_xor(v, 2);
	return v;
}

/* (score, pos) a goes before b: the larger score, of equal scores the lower pos -- a strict total order, so a reduction in any
 * shape gives what the row's windows taken in order under strict > give */
__device__ __forceinline__ bool before(double sa, unsigned pa, double sb, unsigned pb) { return sa > sb || (sa == sb && pa < pb); }

__device__ __forceinline__ void wave_best(double &s, unsigned &p, unsigned &tag)
{
#pragma unroll
	for (int d = 1; d < WAVE; d <<= 1) {
		const double so = __shfl_xor(s, d);
		const unsigned po = __shfl_xor(p, d), to = __shfl_xor(tag, d);
		if (before(so, po, s, p)) {
			s = so;
			p = po;
			tag = to;
		}
	}
}

/* the header's score from the five sums as doubles: 4 (Ra.re Rb.re + Ra.im Rb.im) / (E E), E == 0 and a NaN give 0 */
__device__ __forceinline__ double score_of(double ar, double ai, double br, double bi, double e)
{
	if (e == 0.0)
		return 0.0;
	const double s = 4.0 * (ar * br + ai * bi) / (e * e);
	return s == s ? s : 0.0;
}

template <bool I16>
__global__ void __launch_bounds__(kThreads)
ms_fsearch_kernel(const void *__restrict__ iq, size_t buf_stride, unsigned buf_len, unsigned n_seg, unsigned long long n_work,
		  trxhip_ms_fcch_hit *__restrict__ cand)
{
	using T = typename std::conditional<I16, long long, double>::type;     /* what a block sum is kept as */
	using A = typename std::conditional<I16, long long, float>::type;      /* what a lane adds in */
	__shared__ T s_sum[3][PFX];                                            /* p.re, p.im, e: block sums, then (int16) their prefixes */
	__shared__ double s_score[kWaves];
	__shared__ unsigned s_pos[kWaves];

	const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const unsigned nb = trx_fs_blocks(buf_len), nwin = nb - (TRX_FS_BLOCKS - 1);

	for (unsigned long long wk = blockIdx.x; wk < n_work; wk += gridDim.x) {
		const unsigned long long row = wk / n_seg;
		const unsigned seg = (unsigned)(wk - row * n_seg);
		const char *rowp = static_cast<const char *>(iq) + row * buf_stride * (I16 ? 4 : 8);
		const unsigned b0 = seg * SEG;                                 /* the segment's first block and first window */
		const unsigned lb = min(nb - b0, (unsigned)LB_MAX);            /* its blocks: every sample read is below 16 nb + 8 <= buf_len */

		// ---- block sums: lane g of the segment takes samples 4 g .. 4 g + 3 of it, four lanes a block
#pragma unroll
		for (int it = 0; it < ITER; it++) {
			const unsigned g = (unsigned)it * kThreads + tid;
			const bool live = g < lb * 4u;
			A re = 0, im = 0, en = 0;
			if (live) {
				const size_t n = (size_t)b0 * TRX_FS_HOP + (size_t)g * 4u;
				if constexpr (I16) {
					const v4i b = load16<v4i, 4>(rowp + n * 4), a = load16<v4i, 4>(rowp + (n + TRX_FS_LAG) * 4);
#pragma unroll
					for (int k = 0; k < 4; k++)
						mac_i16(a[k], b[k], re, im, en);
				} else {
					const v4f b0v = load16<v4f, 8>(rowp + n * 8), b1v = load16<v4f, 8>(rowp + (n + 2) * 8);
					const v4f a0v = load16<v4f, 8>(rowp + (n + TRX_FS_LAG) * 8), a1v = load16<v4f, 8>(rowp + (n + TRX_FS_LAG + 2) * 8);
					mac_f32(a0v[0], a0v[1], b0v[0], b0v[1], re, im, en);
					mac_f32(a0v[2], a0v[3], b0v[2], b0v[3], re, im, en);
					mac_f32(a1v[0], a1v[1], b1v[0], b1v[1], re, im, en);
					mac_f32(a1v[2], a1v[3], b1v[2], b1v[3], re, im, en);
				}
			}
			re = quad_sum(re);                                     /* (a quad is live or dead as one: lb * 4 is a multiple of 4) */
			im = quad_sum(im);
			en = quad_sum(en);
			if (live && (tid & 3u) == 0) {
				s_sum[0][g >> 2] = (T)re;
				s_sum[1][g >> 2] = (T)im;
				s_sum[2][g >> 2] = (T)en;
			}
		}
		__syncthreads();

		// ---- int16: waves 0 .. 2 turn one array each into exclusive prefixes, P[k] = the sum of blocks < k, k <= lb
		if constexpr (I16) {
			if (wave < 3) {
				T *s = s_sum[wave];
				T v[PER_LANE], t = 0;
#pragma unroll
				for (int i = 0; i < PER_LANE; i++) {
					const unsigned k = lane * PER_LANE + i;
					v[i] = k < lb ? s[k] : 0;
					t += v[i];
				}
				T inc = t;                                             /* inclusive scan of the lanes' totals */
#pragma unroll
				for (int d = 1; d < WAVE; d <<= 1) {
					const T o = __shfl_up(inc, d);
					if ((int)lane >= d)
						inc += o;
				}
				T run = inc - t;
#pragma unroll
				for (int i = 0; i < PER_LANE; i++) {
					s[lane * PER_LANE + i] = run;
					run += v[i];
				}
			}
			__syncthreads();
		}

		// ---- one lane per window
		const unsigned j = b0 + tid;
		const bool mine = j < nwin;
		double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0, e = 0.0, score = -INFINITY;
		unsigned pos = 0xffffffffu, tag = 0;
		if (mine) {
			if constexpr (I16) {
				const unsigned h = tid + TRX_FS_HALF, w = tid + TRX_FS_BLOCKS;
				ar = (double)(s_sum[0][h] - s_sum[0][tid]);
				ai = (double)(s_sum[1][h] - s_sum[1][tid]);
				br = (double)(s_sum[0][w] - s_sum[0][h]);
				bi = (double)(s_sum[1][w] - s_sum[1][h]);
				e = (double)(s_sum[2][w] - s_sum[2][tid]);
			} else {
#pragma unroll 6
				for (int k = 0; k < TRX_FS_HALF; k++) {
					ar += s_sum[0][tid + k];
					ai += s_sum[1][tid + k];
					br += s_sum[0][tid + TRX_FS_HALF + k];
					bi += s_sum[1][tid + TRX_FS_HALF + k];
					e += s_sum[2][tid + k];
				}
#pragma unroll 6
				for (int k = TRX_FS_HALF; k < TRX_FS_BLOCKS; k++)
					e += s_sum[2][tid + k];
			}
			score = score_of(ar, ai, br, bi, e);
			pos = j * TRX_FS_HOP;
		}
		double bs = score;
		unsigned bp = pos;
		wave_best(bs, bp, tag);
		if (lane == 0) {
			s_score[wave] = bs;
			s_pos[wave] = bp;
		}
		__syncthreads();
#pragma unroll
		for (int w = 0; w < kWaves; w++)
			if (before(s_score[w], s_pos[w], bs, bp)) {
				bs = s_score[w];
				bp = s_pos[w];
			}
		if (mine && pos == bp) {                                       /* the segment's first window is always there: one lane writes */
			trxhip_ms_fcch_hit c;
			c.found = 0;
			c.pos = pos;
			c.score = score;
			c.ra_re = ar;
			c.ra_im = ai;
			c.rb_re = br;
			c.rb_im = bi;
			c.energy = e;
			c.reserved = 0;
			cand[wk] = c;
		}
		__syncthreads();                                               /* the next piece of work writes LDS again */
	}
}

template <bool I16>
__global__ void __launch_bounds__(kThreads)
ms_fsearch_pick_kernel(const void *__restrict__ iq, size_t buf_stride, unsigned n_seg, unsigned long long n_rows, double min_score,
		       float scale, const trxhip_ms_fcch_hit *__restrict__ cand, trxhip_ms_fcch_hit *__restrict__ hit,
		       trxhip_ms_fcch *__restrict__ fcch)
{
	const int lane = (int)(threadIdx.x & 63u);
	for (unsigned long long row = (unsigned long long)blockIdx.x * kWaves + (threadIdx.x >> 6); row < n_rows;
	     row += (unsigned long long)gridDim.x * kWaves) {
		const trxhip_ms_fcch_hit *c = cand + row * n_seg;
		double bs = -INFINITY;
		unsigned bp = 0xffffffffu, bseg = 0;
		for (unsigned s = (unsigned)lane; s < n_seg; s += WAVE) {
			const double sc = c[s].score;
			const unsigned ps = c[s].pos;
			if (before(sc, ps, bs, bp)) {
				bs = sc;
				bp = ps;
				bseg = s;
			}
		}
		wave_best(bs, bp, bseg);
		bseg = uni(bseg);
		trxhip_ms_fcch_hit h = c[bseg];
		h.found = h.score >= min_score ? 1 : 0;
		if (lane == 0)
			hit[row] = h;
		if (fcch) {
			const char *slot = static_cast<const char *>(iq) + (row * buf_stride + uni(h.pos)) * (I16 ? 4 : 8);
			const trxhip_ms_fcch o = afc_measure<I16>(slot, scale, lane);
			if (lane == 0)
				fcch[row] = o;
		}
	}
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : TRXHIP_EIO; }

int fsearch_batch(trxhip_ctx *ctx, const void *d_iq, int i16, size_t buf_stride, size_t buf_len, size_t n_bufs, double min_score,
		  float rx_full_scale, trxhip_ms_fcch_hit *d_hit, trxhip_ms_fcch *d_fcch, void *stream)
{
	if (!ctx || !d_iq || (reinterpret_cast<uintptr_t>(d_iq) & (i16 ? 3 : 7)) || !d_hit || (reinterpret_cast<uintptr_t>(d_hit) & 7) ||
	    (reinterpret_cast<uintptr_t>(d_fcch) & 7))
		return TRXHIP_EINVAL;
	if (buf_len < TRX_FS_MIN_LEN || buf_len > 0x7fffffffull || buf_stride < buf_len || n_bufs == 0 || n_bufs > 0x7fffffffull)
		return TRXHIP_EINVAL;
	if (!(min_score > 0.0 && min_score <= 1.0) || !std::isfinite(rx_full_scale) || rx_full_scale <= 0.0f)
		return TRXHIP_EINVAL;
	if (with_device(ctx))
		return TRXHIP_EIO;
	const size_t n_seg = trx_fs_segments((uint32_t)buf_len);
	trx_fsearch_scratch &sc = ctx->fsearch;
	std::lock_guard<std::mutex> lock(sc.mu);
	if (!sc.acquire(n_bufs * n_seg, static_cast<hipStream_t>(stream)))
		return TRXHIP_ENOMEM;
	const hipStream_t st = static_cast<hipStream_t>(stream);
	const int rc = trx_launch_ms_fsearch(d_iq, i16, buf_stride, buf_len, n_bufs, min_score, 1.0f / rx_full_scale, sc.d_cand, d_hit, d_fcch, st);
	sc.launched(st);
	return rc;
}

}  // namespace

extern "C" int trx_launch_ms_fsearch(const void *d_iq, int i16, size_t buf_stride, size_t buf_len, size_t n_bufs, double min_score,
				     float scale, trxhip_ms_fcch_hit *d_cand, trxhip_ms_fcch_hit *d_hit, trxhip_ms_fcch *d_fcch,
				     hipStream_t stream)
{
	if (n_bufs == 0 || buf_len < TRX_FS_MIN_LEN || buf_len > 0x7fffffffull)
		return TRXHIP_EINVAL;
	const unsigned n_seg = trx_fs_segments((uint32_t)buf_len);
	const unsigned long long n_work = (unsigned long long)n_bufs * n_seg;
	const unsigned g1 = (unsigned)(n_work < kMaxGrid ? n_work : kMaxGrid);
	const unsigned long long pb = (n_bufs + kWaves - 1) / kWaves;
	const unsigned g2 = (unsigned)(pb < kMaxGrid ? pb : kMaxGrid);
	if (i16) {
		hipLaunchKernelGGL(ms_fsearch_kernel<true>, dim3(g1), dim3(kThreads), 0, stream, d_iq, buf_stride, (unsigned)buf_len, n_seg, n_work,
				   d_cand);
		hipLaunchKernelGGL(ms_fsearch_pick_kernel<true>, dim3(g2), dim3(kThreads), 0, stream, d_iq, buf_stride, n_seg,
				   (unsigned long long)n_bufs, min_score, scale, d_cand, d_hit, d_fcch);
	} else {
		hipLaunchKernelGGL(ms_fsearch_kernel<false>, dim3(g1), dim3(kThreads), 0, stream, d_iq, buf_stride, (unsigned)buf_len, n_seg, n_work,
				   d_cand);
		hipLaunchKernelGGL(ms_fsearch_pick_kernel<false>, dim3(g2), dim3(kThreads), 0, stream, d_iq, buf_stride, n_seg,
				   (unsigned long long)n_bufs, min_score, scale, d_cand, d_hit, d_fcch);
	}
	return launched();
}

extern "C" {

int trxhip_ms_fcch_search_i16(trxhip_ctx *ctx, const int16_t *d_iq, size_t buf_stride, size_t buf_len, size_t n_bufs, double min_score,
			      float rx_full_scale, trxhip_ms_fcch_hit *d_hit, trxhip_ms_fcch *d_fcch, void *stream)
{
	return fsearch_batch(ctx, d_iq, 1, buf_stride, buf_len, n_bufs, min_score, rx_full_scale, d_hit, d_fcch, stream);
}

int trxhip_ms_fcch_search_cf32(trxhip_ctx *ctx, const float *d_iq_cf32, size_t buf_stride, size_t buf_len, size_t n_bufs, double min_score,
			       float rx_full_scale, trxhip_ms_fcch_hit *d_hit, trxhip_ms_fcch *d_fcch, void *stream)
{
	return fsearch_batch(ctx, d_iq_cf32, 0, buf_stride, buf_len, n_bufs, min_score, rx_full_scale, d_hit, d_fcch, stream);
}

}  // extern "C"
