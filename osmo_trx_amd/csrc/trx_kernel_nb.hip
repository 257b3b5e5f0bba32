// trx_kernel_nb.hip -- the NORMAL-BURST kernel: 625-sample int16 bursts at 4 SPS whose slot expects a GMSK normal burst
// (analyzeTrafficBurst, sigProcLib.cpp:1887-1904 -> detectGeneralBurst :1732-1771 -> detectBurst :1649-1709; demodGmskBurst
// :2055-2072 -> demodCommon :2030-2048; vectorSlicer :546-556), fused demodulator + FAST detector, 148 sliced soft bits --
// the call pullRadioVector() makes for a traffic slot and bench.py times.  (Included by trx_kernel4.hip: one translation
// unit, one copy of the device-side counters.)
//
// Same arithmetic as the COMMON instantiation of burst_pull4_kernel (trx_kernel4.hip) -- results are bit-identical to it --
// but nothing else is in here: no access / EDGE / dummy / wide-window / exact-demodulator code, no run-time flags.  A burst
// this kernel cannot finish is FLAGGED (a byte per burst) and left to the general kernel, which is launched behind it over the flags:
//   * the slot is not a normal-burst slot (type != TSC, tsc > 7) or its window is wider than one round (max_toa > 32);
//   * (a decimated sample that fails the addition-only correlation's guard -- about one burst in 3000 -- takes the multiplying form here)
//   * the peak-ratio gate is too close to call for the estimate (about one in 1e5);
//   * the detected TOA is outside the straight-line demodulator's geometry (toa < -0.25 or > 9 symbols).
// What is different from the general kernel, beside what is absent:
//   * soft bits never go through LDS: the three outputs of a lane (lanes 2..49: symbols 3 lane - 2 + j, the sums the demodulator's
//     moving accumulators end in; symbols 0..3 come from the low-edge lanes 54, 57, 60, 63) are rotated, scaled and sliced in registers -- the (-j)^i rotation is a quad permutation of ONE
//     per-lane multiplier, applied by the DPP operand of the multiply -- and stored as one 12-byte store per lane (a
//     contiguous 576-byte run per burst), one burst late like the general kernel's (the stores must be older than the
//     prefetch loads: vmcnt retires in order);
//   * a workgroup's static share is one CONTIGUOUS range of bursts (burst = base + item: one scalar add).
#include "trx_k4_common.h"
#include "trx_nb_asm.inc"

#define NB_D_LEN    160                                           /* decimated window (64 used) / parking space of the low-edge tap rows (1 KB) / the
                                                                      156 symbols of the general demodulator (cold) */
#define NB_CZ_LEN   (TRX_CZ_PAD + TRX_CORR_NARROW + TRX_CZ_PAD)
#define NB_SLICE    (K4_XS + NB_D_LEN + NB_CZ_LEN)                /* complex samples per wave */
#define NB_COMP_ROWS (TRX_DELAY_FILTS + 1)
#define NB_AMP_FLOATS (8 * 8)                                      /* [8 TSC][A by lane & 3, B by lane & 3]: trx_tables.h, trx_amp_lane_coef */
#define NB_TABLES_FLOATS (TRX_SINCV_LDS + 16 * WAVE + NB_COMP_ROWS * 36 + 16 + 8 * 8 + 5 * WAVE + 5 * WAVE + 2 * 8 * 16 + NB_AMP_FLOATS)
#define NB_TABLES_BYTES (NB_TABLES_FLOATS * 4)
#define NB_WPB 16
#define NB_POOL_RING 64
#define NB_POOL_UNSET (-1)
#define NB_POOL_END (-2)
#define NB_NO_BURST 0xffffffffu
#define NB_LDS_TAIL (16 + 4 * NB_POOL_RING)
#define NB_LDS_BYTES (NB_TABLES_BYTES + NB_WPB * NB_SLICE * 8 + NB_LDS_TAIL)
#define NB_MAX_TOA 32                                             /* window of 16 + max_toa <= 48 lags: 15 + 48 = 63 decimated samples, one per lane */



// Wave priority by phase: s_setprio 0 in front of the demodulator's filter (TAIL), 2 behind it.  The filter is the one phase
// that is dense in vector work -- 72 packed FMAs back to back; everything else is chains of LDS round trips and scalar glue.
// With the filter at priority 0 and the rest at 2, a wave that comes out of a wait gets the next issue slot and the filter
// waves fill what is left: +0.5 % same box (5 rounds, three alternatives within +-0.3 % of it: profiles/r06_ab_runs.txt).
typedef float v3f __attribute__((ext_vector_type(3)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) v2f lds_v2f;

// byte address of an LDS object (what the ds_* instructions of the asm blocks take)
template <typename T>
__device__ __forceinline__ unsigned lds_addr(const T *p)
{
	return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) T *)p;
}

// the lane's number, for the cold paths of the burst loop: each derives its own where it starts (the loop's main path carries
// none -- what it needs of the lane are the addresses made once in front of the loop)
__device__ __forceinline__ int nb_lane_id()
{
	int lane;
	asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
	return lane;
}

// Lane layout of the TOA search in the hand-placed blocks DETA / DETB (tools/gen_nb_asm.py, walk_rank): the nodes of a round of
// LEVELS levels stand in POSITION order -- node (level k, index i) at in-order rank r = (2 i + 1) * 2^(LEVELS - 1 - k) - 1, on
// lanes 2 r (early) and 2 r + 1 (late) -- where peak_const() (trx_device.h) has heap node n = 2^k - 1 + i on lanes 2 n, 2 n + 1.
// The layout is this kernel's own: only what the blocks read by lane is staged through it (wa4f, ka, kb).  Lanes that hold no
// node of the round (round A: 62, 63; round B: 30 .. 63) keep their place.
//   nb_walk_src(l): the peak_const() lane whose constants lane l of the blocks takes;  nb_walk_dst(): its inverse
template <int LEVELS>
__device__ __forceinline__ int nb_walk_src(int l)
{
	const int r = l >> 1;
	if (r >= (1 << LEVELS) - 1)
		return l;
	const int t = __ffs(r + 1) - 1;                                // LEVELS - 1 - k
	const int k = LEVELS - 1 - t, i = (r + 1) >> (t + 1);
	return 2 * ((1 << k) - 1 + i) + (l & 1);
}
template <int LEVELS>
__device__ __forceinline__ int nb_walk_dst(int l)
{
	const int n = l >> 1;
	if (n >= (1 << LEVELS) - 1)
		return l;
	const int k = 31 - __clz(n + 1), i = n + 1 - (1 << k);
	return 2 * (((2 * i + 1) << (LEVELS - 1 - k)) - 1) + (l & 1);
}

__global__ void __launch_bounds__(NB_WPB * WAVE)
nb_pull4_kernel(const uint32_t *__restrict__ iq, const trxhip_burst_params *__restrict__ params,
		trxhip_burst_result *__restrict__ results, float *__restrict__ soft, const trx_tables *__restrict__ tab,
		unsigned n_bursts, float thresh, float full_scale, unsigned *__restrict__ pool_ctr, unsigned *__restrict__ redo,
		float gk5, float gk6, float gk7, float gk8)
{
	static_assert(NB_TABLES_BYTES % 16 == 0 && (NB_SLICE * 8) % 16 == 0 && (K4_XS * 8) % 16 == 0 && (NB_D_LEN * 8) % 16 == 0, "16-byte LDS accesses");
	static_assert(NB_LDS_BYTES <= 160 * 1024, "LDS");
	static_assert(NB_ASM_GDEC_OFF == (TRX_SINCV_LDS + 16 * WAVE + NB_COMP_ROWS * 36) * 4, "tools/gen_nb_asm.py: LDS offset of the decimator taps");
	static_assert(NB_ASM_DEC_MAX_NACT == 15 + NB_ASM_CORR_MAX_LEN, "tools/gen_nb_asm.py: DEC and CORR change form at the same window (one test)");
	static_assert(NB_ASM_LSEQ_OFF == (NB_TABLES_FLOATS - NB_AMP_FLOATS - 2 * 8 * 16) * 4, "tools/gen_nb_asm.py: LDS offset of the training-sequence taps");
	static_assert(NB_ASM_AW_PD == (PH_M0 + 52) * 8 && NB_ASM_AW_D == K4_XS * 8 && NB_ASM_AW_CZ == (K4_XS + NB_D_LEN + TRX_CZ_PAD) * 8,
		      "tools/gen_nb_asm.py: offsets of P, D[] and cz[] inside a wave's slice");
	constexpr int NLD = 10;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int lane0 = threadIdx.x & (WAVE - 1);
	const int wave = uni((int)(threadIdx.x >> 6));

	// ---- LDS carve: [tables][per-wave slices][work counter, pool ring]
	float *const sincv = reinterpret_cast<float *>(smem);           // [4128] swizzled sinc LUT as row pairs (at LDS offset 0; trx_sincp_idx)
	float *const wa4f = sincv + TRX_SINCV_LDS;                     // [4][64] float4: round A's interpolation weights by lane
	const float4 *const wa4 = reinterpret_cast<const float4 *>(wa4f);
	float *const comp = wa4f + 16 * WAVE;                          // [65][36] composite delay-o-decimate filters (shifted by TRX_FUSED_SH)
	float *const gdec = comp + NB_COMP_ROWS * 36;                  // [16] decimator taps
	float *const lhdr = gdec + 16;                                 // [8][8] headers of the eight training sequences
	int *const pkcl = reinterpret_cast<int *>(lhdr + 8 * 8);       // [5][64] PeakConst fields by lane (the exact re-run of the TOA search)
	int *const lcn = pkcl + 5 * WAVE;                              // lane constants of the hand-placed blocks (below): [2][64] pairs, [64]
	c32 *const lseq = reinterpret_cast<c32 *>(lcn + 5 * WAVE);     // [8][16] training-sequence taps (the multiplying correlation: guard failures)
	float *const lamp = reinterpret_cast<float *>(lseq + 8 * 16);  // [8][8] 1 / gain of the eight sequences as block TAIL's lanes take it: a row of 32 bytes
	                                                               // per sequence, (A, B) of lane & 3 sixteen bytes apart (trx_tables.h, trx_amp_lane_coef)
	c32 *const wbase = reinterpret_cast<c32 *>(smem + NB_TABLES_BYTES) + (size_t)wave * NB_SLICE;
	int *const wg_next = reinterpret_cast<int *>(reinterpret_cast<c32 *>(smem + NB_TABLES_BYTES) + (size_t)NB_WPB * NB_SLICE);
	int *const pool_g = wg_next + 4;
	c32 *const P = wbase;                                          // polyphase burst: P[r*PH_A + PH_M0 + m] = x[4m + r]
	c32 *const D = wbase + K4_XS;                                  // D[i] = decimated sample 56 + i
	c32 *const cz = D + NB_D_LEN + TRX_CZ_PAD;                     // zero-padded correlation

	// ---- one-time staging of the tables; zero this wave's slice (pads stay zero)
	// (the sinc LUT as pairs of rows -- trx_tables.h, trx_sincp_idx: block DETB reads the weights of two taps as one 8-byte entry.
	// The blob's index 512 r + s is row r, column slot s: the swizzle leaves the row alone.  Slot 512 of a pair: column 0 of the next row)
	static_assert(4 * TRX_SINCP_STRIDE <= TRX_SINCV_LDS, "the row pairs fit the LUT's LDS space");
	for (int i = threadIdx.x; i < TRX_SINCV_LDS; i += blockDim.x) {
		const int src = trx_sincp_src(i);
		sincv[i] = (src >= 0) ? tab->sincv[src] : 0.0f;
	}
	for (int i = threadIdx.x; i < 16 * WAVE; i += blockDim.x) {
		const int l = i & (WAVE - 1), u = i >> 6;
		const PeakConst pcl = peak_const(nb_walk_src<5>(l));         // (round A's weights: in the blocks' lane layout)
		const int q = (u < 8) ? pcl.loA + 512 * (7 - u) : pcl.hiA + 512 * (u - 8);
		wa4f[((u >> 2) * WAVE + l) * 4 + (u & 3)] = (q < TRX_SINCV_LEN) ? tab->sincv[q] : 0.0f;
	}
	for (int i = threadIdx.x; i < NB_COMP_ROWS * 36; i += blockDim.x) {
		const int f = i / 36, j = i % 36;
		comp[i] = (j >= TRX_FUSED_SH) ? tab->comp_filt[f][j - TRX_FUSED_SH] : 0.0f;
	}
	if (threadIdx.x < 16)
		gdec[threadIdx.x] = tab->dec_taps[threadIdx.x];
	if (threadIdx.x < 128)
		lseq[threadIdx.x] = make_float2(tab->seq[TRX_SEQ_TSC0 + (threadIdx.x >> 4)].taps[threadIdx.x & 15].re,
						tab->seq[TRX_SEQ_TSC0 + (threadIdx.x >> 4)].taps[threadIdx.x & 15].im);
	if (threadIdx.x < 64)
		lhdr[threadIdx.x] = reinterpret_cast<const float *>(&tab->seq[TRX_SEQ_TSC0 + (threadIdx.x >> 3)].gain)[threadIdx.x & 7];
	if (threadIdx.x < NB_AMP_FLOATS) {
		const trx_c32 gi = tab->seq[TRX_SEQ_TSC0 + (threadIdx.x >> 3)].gain_inv;
		lamp[threadIdx.x] = trx_amp_lane_coef(gi.re, gi.im, (int)(threadIdx.x & 7));
	}
	if (threadIdx.x < WAVE) {
		const PeakConst pc0 = peak_const(threadIdx.x);
		pkcl[0 * WAVE + threadIdx.x] = pc0.flA;
		pkcl[1 * WAVE + threadIdx.x] = pc0.loA;
		pkcl[2 * WAVE + threadIdx.x] = pc0.hiA;
		pkcl[3 * WAVE + threadIdx.x] = pc0.offB;
		pkcl[4 * WAVE + threadIdx.x] = pc0.ratio_off;
		// byte offsets relative to &cz[bidx]: the lane's peak-ratio term; round A's first tap (cz + bidx - 1 + flA - 7); round B's offset
		// (two 8-byte entries per lane -- (kr, ka), (kb, kic) -- and ktp by itself: three reads in block AMAX's wait states)
		// (ka and kb in the blocks' lane layout, nb_walk_src; the gate's terms kr are no nodes: lanes 0 .. 7 as they are)
		lcn[2 * threadIdx.x + 0] = pc0.ratio_off * 8;
		lcn[2 * threadIdx.x + 1] = (peak_const(nb_walk_src<5>((int)threadIdx.x)).flA - 8) * 8;
		lcn[2 * (WAVE + threadIdx.x) + 0] = peak_const(nb_walk_src<4>((int)threadIdx.x)).offB;
		// the demodulator's lanes (tools/gen_nb_asm.py, fir_moving: every lane holds twelve samples = three symbols, the sums move
		// two lanes up): 0..49 samples from symbol 4 + 3 lane on, composite row (50, 51: idle, as 49); 52 + 3 e + t, low-edge symbol
		// e: t = 0, 1 main part -- samples from symbol e / e + 3, row e of the parked block; t = 2 its taps u < 8 -- samples from
		// symbol e - 3, row 4 + e
		const int l = threadIdx.x, e = (l - 52) / 3, t = (l - 52) % 3;
		const bool sp = l >= 52;
		lcn[2 * (WAVE + l) + 1] = 8 * (sp ? (t == 0 ? e : t == 1 ? e + 3 : e - 3) : 4 + 3 * (l < 49 ? l : 49));   // first symbol, bytes
		lcn[4 * WAVE + l] = sp ? (e + (t == 2 ? 4 : 0)) * K4_NTP * 4 : -1;                 // tap row inside the parked block, bytes
	}
	for (int i = lane0; i < NB_SLICE; i += WAVE)
		wbase[i] = make_float2(0.0f, 0.0f);
	if (threadIdx.x == 0) {
		wg_next[0] = NB_WPB;
		wg_next[1] = 0;                                             // the epilogue's election
	}
	if (threadIdx.x < NB_POOL_RING)
		pool_g[threadIdx.x] = NB_POOL_UNSET;
	__syncthreads();

	// the peak-ratio gate's estimate (tools/gen_nb_asm.py, DETA): thresh^2 / num for the four possible term counts, and the
	// constant term of its certain-pass bound
	const float thr2 = thresh * thresh;
	// (gk5 .. gk8 = thresh^2 / 5 .. thresh^2 / 8 come as kernel arguments; the loop keeps them in lanes 5 .. 8 of ONE vector
	// register, from which the gate reads the one it needs by lane number: four scalar registers less across the loop)
	float gkv = lane0 == 5 ? gk5 : lane0 == 6 ? gk6 : lane0 == 7 ? gk7 : gk8;
	asm volatile("" : "+v"(gkv));
	const float gc0 = thr2 * 1.0001e-5f;
	// (int)(sync->toa * 512) of the eight training sequences, 4 bits each (+-1 for the reference's tables); a table set whose
	// offsets do not fit leaves every burst to the general kernel
	int t5pk = 0;
	bool t5_ok = true;
	for (int t = 0; t < 8; t++) {
		const int v = (int)(lhdr[8 * t + 5] * 512.0f);
		t5_ok = t5_ok && v >= -8 && v <= 7 && (float)v == lhdr[8 * t + 5] * 512.0f;   // (exact: toa = -nk / 512 then is, too)
		t5pk |= (v & 15) << (4 * t);
	}
	t5pk = uni(t5pk);
	// (the burst loop's conditions are kept as wave-uniform integers in scalar registers: a bool that depends on LDS contents, or
	// that is carried round the loop as a phi of constants, is a 64-bit lane mask to the compiler, and every test of it an
	// s_and_b64 vcc, exec, mask + s_cbranch_vcc pair in a structurised flow graph)
	// a slot's word (max_toa << 16 | tsc << 8 | type) is below this for the windows the kernel takes; 0: it takes none
	const unsigned toa_lim = (unsigned)uni(t5_ok ? (int)((NB_MAX_TOA + 1u) << 16) : 0);
	const unsigned long long e8_addr = reinterpret_cast<unsigned long long>(&tab->edge8[0][0][0]);
	// ---- work distribution: groups of 16 consecutive bursts.  Static part: workgroup w owns ONE contiguous range of groups
	// (7/8 of the batch when the cross-die pool is on, everything otherwise); the rest is drawn group by group from a
	// device-wide counter (see burst_pull4_kernel).  Waves claim items one at a time from the workgroup's LDS counter.
	const unsigned n_wg = gridDim.x;
	const unsigned n_groups = (n_bursts + 15u) >> 4;
	const bool pooled = pool_ctr != nullptr;
	const unsigned n_static_groups = pooled ? ((n_groups - (n_groups >> 3)) / n_wg) * n_wg : n_groups;
	const unsigned n_pool_groups = n_groups - n_static_groups;
	const unsigned gq = n_static_groups / n_wg, gr = n_static_groups % n_wg;
	const unsigned my_groups = gq + (blockIdx.x < gr ? 1u : 0u);
	const unsigned base16 = (blockIdx.x * gq + (blockIdx.x < gr ? blockIdx.x : gr)) << 4;   // first burst of this workgroup's range
	unsigned items = my_groups << 4;
	if (base16 + items > n_bursts)
		items = (base16 < n_bursts) ? n_bursts - base16 : 0u;       // the batch's last group may be short
	auto burst_of = [&](unsigned jj) -> unsigned {
		if (__builtin_expect(jj < items, 1))
			return base16 + jj;
		if (!pooled)
			return NB_NO_BURST;
		const unsigned k = (jj - items) >> 4;
		volatile int *slot = pool_g + (k & (NB_POOL_RING - 1));
		int g;
		while ((g = *slot) == NB_POOL_UNSET)
			__builtin_amdgcn_s_sleep(2);
		g = uni(g);
		if (g < 0)
			return NB_NO_BURST;
		const unsigned bb = ((n_static_groups + (unsigned)g) << 4) + (jj & 15u);
		return bb < n_bursts ? bb : NB_NO_BURST;
	};
	auto pool_draw = [&](unsigned jj, bool ended) {
		const int lane = nb_lane_id();
		const unsigned k = (jj + 16u - items) >> 4;
		int g = NB_POOL_END;
		if (!ended) {
			unsigned p = 0;
			if (lane == 0)
				p = __hip_atomic_fetch_add(pool_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			p = (unsigned)uni((int)p);
			g = (p < n_pool_groups) ? (int)p : NB_POOL_END;
		}
		if (lane == 0) {
			pool_g[(k + NB_POOL_RING / 2) & (NB_POOL_RING - 1)] = NB_POOL_UNSET;
			pool_g[k & (NB_POOL_RING - 1)] = g;
		}
	};

	// ---- what the burst loop needs of the lane and the wave, made ONCE and carried in registers: left to the compiler, each is
	// rebuilt from the lane id wherever it is used -- 28 vector instructions per burst, two 32-bit multiplies among them, at the
	// head of the chains the first LDS write and DEC's first read wait for.  Opaque copies: a value the compiler cannot see
	// through is kept, not rematerialised.
	//   a_p    byte address of the conversion's first row: P + (lane & 3) * PH_A + PH_M0 + (lane >> 2) of this wave's slice;
	//          row r is offset 128 r of it
	//   a_w    slice base + 8 * lane: P + PH_M0 + 52 + lane, D[lane], D[lane - 4 / - 19], cz[lane], cz[lane - 19] are
	//          compile-time offsets of it in the blocks DEC, CORR and TAIL (tools/gen_nb_asm.py: NB_ASM_AW_*)
	//   a_l4   4 * lane (prefetch rows 0..8, the lane constants' fetch in AMAX, the record's store), a_l4c 4 * min(lane, 48) (the
	//          tenth prefetch row: no load goes behind word 624 of its burst), a_l16 16 * lane (DETA, TAIL)
	//   a_st   byte offset of the lane's soft bits inside a burst's 148: lanes 2..49 (lane - 2) * 12 + 16, lanes 54 + 3 e: 4 e
	unsigned a_p = lds_addr(wbase) + 8u * (unsigned)((lane0 & 3) * PH_A + PH_M0 + (lane0 >> 2));
	unsigned a_w = lds_addr(wbase) + 8u * (unsigned)lane0;
	unsigned a_l4 = 4u * (unsigned)lane0;
	unsigned a_l4c = 4u * min((unsigned)lane0, 48u);
	unsigned a_l16 = 16u * (unsigned)lane0;
	unsigned a_st = (lane0 >= 54) ? 4u * (unsigned)((lane0 - 54) / 3) : (unsigned)(lane0 - 2) * 12u + 16u;
	asm volatile("" : "+v"(a_p));
	asm volatile("" : "+v"(a_w));
	asm volatile("" : "+v"(a_l4));
	asm volatile("" : "+v"(a_l4c));
	asm volatile("" : "+v"(a_l16));
	asm volatile("" : "+v"(a_st));

	// ---- software prefetch of the next burst: ten dwords per lane + the slot's parameters
	uint32_t pre_i[NLD];
	uint32_t pre_prm = 0u;
	auto prefetch = [&](unsigned bb) {
		pre_prm = reinterpret_cast<const uint32_t *>(params)[2 * (size_t)bb];
		const char *src = reinterpret_cast<const char *>(iq + (size_t)bb * 625);
		// (an unsigned 32-bit byte offset: it zero-extends, the loads take the scalar-base form -- no 64-bit vector address whose
		// high half the compiler would build in one of the destination registers, with a wait for vmcnt(0) in front)
		const uint32_t *const row = reinterpret_cast<const uint32_t *>(src + a_l4);
#pragma unroll
		for (int r = 0; r < NLD - 1; r++)
			pre_i[r] = __builtin_nontemporal_load(row + r * WAVE);                         // read once: streaming
		// the tenth row has 49 words: lanes 49..63 re-read word 624 (never stored to the LDS).  An exec-masked load behind a
		// "v_mov 0" made the compiler wait for vmcnt(0) -- the nine loads just issued -- in front of the v_mov (measured: -4 %)
		pre_i[NLD - 1] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(src + a_l4c) + (NLD - 1) * WAVE);
	};
	// items j < 16 * my_groups of the static range exist for every workgroup of a launch the launcher sizes (>= 1 group each)
	const unsigned b_first = burst_of((unsigned)wave);
	if (b_first != NB_NO_BURST)
		prefetch(b_first);

	// ---- deferred output (registers): o = the lane's three sliced soft bits, recw = the result record (lanes 0..7)
	v3f o = { 0.0f, 0.0f, 0.0f };
	int recw = 0;
	int pend_m = 0;                                                // 0 / -1: o holds the soft bits of burst pend_b, not yet stored
	int pend_rm = 0;                                               // 0 / 0xff: and recw its record (a slot without a burst)
	unsigned pend_b = 0;
	int left_any = 0;
	// the three stores carry their own EXEC masks, ANDed with pend_m / taken from pend_rm: with nothing pending they store nothing,
	// and no branch goes round them
	// (one offset register for both soft-bit stores: a lane is in at most one of their masks)
	auto store_pending = [&]() {
		float *const so = soft + (size_t)pend_b * 148;
		int *const rp = reinterpret_cast<int *>(results + pend_b);
		const float oe = o.x;
		asm volatile("s_bfm_b64 exec, 48, 2\n\t"
			     "s_and_b32 exec_lo, exec_lo, %7\n\t"
			     "s_and_b32 exec_hi, exec_hi, %7\n\t"
			     "global_store_dwordx3 %0, %1, %2\n\t"
			     "s_mov_b32 exec_lo, 0\n\t"
			     "s_and_b32 exec_hi, %7, 0x92400000\n\t"
			     "global_store_dword %0, %3, %2\n\t"
			     "s_mov_b32 exec_lo, %8\n\t"
			     "s_mov_b32 exec_hi, 0\n\t"
			     "global_store_dword %4, %5, %6\n\t"
			     "s_mov_b64 exec, -1\n\t"
			     "s_nop 0"
			     :: "v"(a_st), "v"(o), "s"(so), "v"(oe), "v"(a_l4), "v"(recw), "s"(rp), "s"(pend_m), "s"(pend_rm)
			     : "memory", "scc");
	};
	// ---- the records of detected bursts are made 64 at a time: what computeCI / amp / toa / RSSI need of burst k of the batch
	// goes into lane k of these registers (seven moves under a one-lane mask), flush_records() does the arithmetic once per lane -- the same
	// operations in the same order as block TAIL did per burst on a wave-uniform value (two logarithms and two reciprocals
	// at a quarter of the rate among them), and one 32-byte store per record
	int q_xr = 0, q_xi = 0, q_es = 0, q_toa = 0, q_s = 0, q_fl = 0, q_b = 0;
	int q_n = 0;
	auto flush_records = [&]() {
		const int lane = nb_lane_id();
		if (lane < q_n) {
			const float *const h = lhdr + 8 * (q_fl & 0xff);        // {gain, 1 / gain, ci_den, toa, n, 1 / ci_den} of the slot's sequence
			const float xr = __int_as_float(q_xr), xi = __int_as_float(q_xi);
			const float a0 = xr * h[2], a1 = xr * h[3], a2 = xi * h[3], a3 = xi * h[2];
			const float amp_re = a0 - a2, amp_im = a1 + a3;         // amp = peak / gain (:1701): peak * (1 / gain), Complex.h:74
			const float toa = (float)q_toa * 0.001953125f;          // position - sync->toa (:1704) - head (:1768): exact in 1/512
			const float energy = __int_as_float(q_es) * 0.0125f;    // energyDetect(burst, 20 * sps): / 80
			const float rssi = rssi_db(full_scale, energy);
			const float p2 = xi * xi + xr * xr;
			const float C = p2 * h[7];                              // |peak|^2 / ci_den (:1633), table: RN(1 / ci_den)
			const float S = __int_as_float(q_s) * 0.0625f;          // computeCI's sum / 16: block TAIL parks the raw sum (a power of two: exact here as there)
			const float ci = 3.0103f * __log2f(C * __builtin_amdgcn_rcpf(S - C));   // (:1637)
			// (stores the compiler does not see, like every other store of the loop: with its own stores outstanding across the
			// loop's back edge it waits for vmcnt(0) -- the soft bits just stored -- in front of the next prefetch; measured: -3 %)
			const v4i r0 = { 1, __float_as_int(toa), __float_as_int(amp_re), __float_as_int(amp_im) };
			const v4i r1 = { __float_as_int(ci), __float_as_int(energy), __float_as_int(rssi), q_fl };
			asm volatile("global_store_dwordx4 %0, %1, off\n\t"
				     "global_store_dwordx4 %0, %2, off offset:16\n\t"
				     "s_nop 1"
				     :: "v"(results + (unsigned)q_b), "v"(r0), "v"(r1) : "memory");
		}
		// (the lanes rejoin HERE, in a block of its own: folded into the loop's latch, the join would make every value the loop
		// carries -- q_n, the pending masks -- a phi behind a divergent branch, that is a vector register or a lane mask)
		asm volatile("");
		q_n = 0;
	};

	// the record's inputs of a detected burst: lane q_n of the seven registers (toa in 1/512 symbol: position - sync->toa - head)
	auto queue_record = [&](const int xr_bits, const int xi_bits, const int es_bits, const int toa, const int s_bits, const int fl, const unsigned bb) {
		asm("s_lshl_b64 exec, 1, %[n]\n\t"
		    "v_mov_b32_e32 %[qxr], %[xr]\n\t"
		    "v_mov_b32_e32 %[qxi], %[xi]\n\t"
		    "v_mov_b32_e32 %[qes], %[es]\n\t"
		    "v_mov_b32_e32 %[qtoa], %[toa]\n\t"
		    "v_mov_b32_e32 %[qs], %[ss]\n\t"
		    "v_mov_b32_e32 %[qfl], %[fl]\n\t"
		    "v_mov_b32_e32 %[qb], %[b]\n\t"
		    "s_mov_b64 exec, -1"
		    : [qxr] "+v"(q_xr), [qxi] "+v"(q_xi), [qes] "+v"(q_es), [qtoa] "+v"(q_toa), [qs] "+v"(q_s), [qfl] "+v"(q_fl),
		      [qb] "+v"(q_b)
		    : [n] "s"(uni(q_n)), [xr] "s"(xr_bits), [xi] "s"(xi_bits), [es] "s"(es_bits), [toa] "s"(toa),
		      [ss] "s"(s_bits), [fl] "s"(fl), [b] "s"((int)bb)
		    : "scc");                                              // (s_lshl_b64 writes SCC: the geometry's compare may not be carried across it)
		q_n++;
	};

	// ---- cold: demodGmskBurst for a TOA outside the straight-line geometry (shift w = nk >> 7 above 0: an early burst; below -36:
	// later than 9 symbols).  The general kernel's fused demodulator (trx_kernel4.hip, "FUSED": same sums, same order -- the
	// results are bit-identical to its) on this kernel's buffers: full outputs from the composite filter, the partial ones at the
	// low / high edge from the truncated-composite tables or the masked two-stage sum; the 156 symbols go through D[], from
	// where every lane picks up its three (rotation, slicer: the general kernel's flush()).
	// Returns false for a geometry whose partial outputs the tables do not cover (the general kernel's masked two-stage sum:
	// bursts shorter than the window -- cannot happen with 625 samples and |TOA| within the search windows; such a burst is left to
	// the general kernel).
	auto demod_general = [&](const int nk, const c32 ampv, const int lane) -> bool {
		constexpr int L = 625, nwrite = 148;
		c32 *const dec = D;
		// (the table addresses of this cold path are formed here, from the one address the loop keeps for block TAIL, behind an
		// opaque copy: none of them is kept in scalar registers across the burst loop)
		const trx_tables *tabc = reinterpret_cast<const trx_tables *>(e8_addr - offsetof(trx_tables, edge8));
		asm volatile("" : "+s"(tabc));
		const int w = nk >> 7, fr = nk & 127;
		const int fidx = (fr >= 2) ? (fr >> 1) : TRX_DELAY_FILTS;
		const float ian = __builtin_amdgcn_rcpf(norm2(ampv));
		const c32 scale = make_float2(ampv.x * ian, -ampv.y * ian);
		const int n_lo = w > 0 ? w : 0;
		const int n_hi = (L - 1 + w < 623) ? L - 1 + w : 623;
		const int i_full_lo = cdiv4(n_lo + 15), i_full_hi = fdiv4(n_hi);
		const int i0l = cdiv4(n_lo), i0h = i_full_hi + 1;
		const bool need_lo = (n_hi >= n_lo) && (i0l < i_full_lo) && (i0l < nwrite);
		const bool need_hi = (n_hi >= n_lo) && (i0h <= fdiv4(n_hi + 15)) && (i0h < nwrite);
		// (the wave-uniform conditions of this path as integers read from lane 0, the per-lane ones formed again where they are
		// used: as bools they are lane masks, two scalar registers each, live across the filter -- more than the burst loop has left)
		// (a partial output the tables do not cover is known from the shift alone: the burst leaves here, in front of the table
		// reads, and behind this the tables cover whatever is needed -- no condition of it stays live as a mask)
		if (uni((need_lo && !(n_hi >= 4 * (i_full_lo - 1))) || (need_hi && !((w <= -2) && (n_lo <= 4 * i0h - 15)))))
			return false;
		const int lo_tab = uni(need_lo);
		float ct0 = 0.0f, ct1 = 0.0f, ct2 = 0.0f;
		const int le = lane >> 4, lt = lane & 15;
		const int li = i0l + le;
		const int lt0 = n_lo + 15 - 4 * li;
		const bool lact = lt0 >= 1;
		if (lo_tab) {
			const float *row = &tabc->edge_lo[fidx][(lact ? lt0 : 1) - 1][lt];
			ct0 = row[0];
			ct1 = row[16];
			ct2 = (lt < 4) ? row[32] : 0.0f;
		}
		const int hi_tab = uni(need_hi);
		float ch0 = 0.0f, ch1 = 0.0f, ch2 = 0.0f;
		const int hi_i = i0h + le;
		const int htm = n_hi + 15 - 4 * hi_i;
		const bool hact = htm >= 0;
		if (hi_tab) {
			const float *row = &tabc->edge_hi[fidx][hact ? htm : 0][lt];
			ch0 = row[0];
			ch1 = row[16];
			ch2 = (lt < 4) ? row[32] : 0.0f;
		}
		int tabv = lo_tab | (hi_tab << 1);                          // (across the filter in one vector register, not as two masks)
		asm volatile("" : "+v"(tabv));
		{
			const int c_full = -24 - w;
			const int i_min = cdiv4(-36 - c_full), i_max = fdiv4(L + 1 - c_full);
			int ic = 3 * lane;
			if (ic < i_min) ic = i_min;
			if (ic > i_max - 2) ic = i_max - 2;
			// (the filter as a hand-placed block -- fir24x3's sums in its order -- so that the compiler does not have to find
			// fifty registers for it inside the burst loop)
			v2f acc[3];
			asm volatile(NB_ASM_FIRG
				     : [a0] "=&v"(acc[0]), [a1] "=&v"(acc[1]), [a2] "=&v"(acc[2])
				     : [nk] "s"(nk), [pb] "s"(lds_addr(P)), [cb] "s"(lds_addr(comp) + 4u * (K4_U0 + TRX_FUSED_SH)), [kic] "v"(8 * ic)
				     : NB_ASM_CLOBBERS);
			if (n_lo == 0 && lo_tab && i_full_hi >= nwrite - 1) {
				if (lane < 52) {
#pragma unroll
					for (int j = 0; j < 3; j++)
						dec[3 * lane + j] = cmul(make_float2(acc[j].x, acc[j].y), scale);
				}
			} else {
#pragma unroll
				for (int j = 0; j < 3; j++) {
					const int i = 3 * lane + j;
					const bool full = (i >= i_full_lo) && (i <= i_full_hi);
					const c32 d = full ? cmul(make_float2(acc[j].x, acc[j].y), scale) : make_float2(0.0f, 0.0f);
					if (i < 156)
						dec[i] = d;
				}
			}
		}
		const int tab2 = uni(tabv), lo_tab2 = tab2 & 1, hi_tab2 = tab2 & 2;
		if (lo_tab2) {
			const int s0 = 4 * li - 24 - w + lt;
			const c32 *pp = P + ((s0 & 3) * PH_A + PH_M0 + (s0 >> 2));
			const c32 x0 = lds_c32(pp), x1 = lds_c32(pp + 4), x2 = lds_c32(pp + 8);
			float ar = x0.x * ct0, ai = x0.y * ct0;
			ar = fmaf(x1.x, ct1, ar); ai = fmaf(x1.y, ct1, ai);
			ar = fmaf(x2.x, ct2, ar); ai = fmaf(x2.y, ct2, ai);
			const float sr = row_sum(ar), si = row_sum(ai);
			int lt0s = lt0;
			asm volatile("" : "+v"(lt0s));
			if (lt == 0 && lt0s >= 1)
				dec[li] = cmul(make_float2(sr, si), scale);
		}
		if (hi_tab2) {
			const int s0 = 4 * hi_i - 24 - w + lt;
			const c32 *pp = P + ((s0 & 3) * PH_A + PH_M0 + (s0 >> 2));
			const c32 x0 = lds_c32(pp), x1 = lds_c32(pp + 4), x2 = lds_c32(pp + 8);
			float ar = x0.x * ch0, ai = x0.y * ch0;
			ar = fmaf(x1.x, ch1, ar); ai = fmaf(x1.y, ch1, ai);
			ar = fmaf(x2.x, ch2, ar); ai = fmaf(x2.y, ch2, ai);
			const float sr = row_sum(ar), si = row_sum(ai);
			int htms = htm;
			asm volatile("" : "+v"(htms));
			if (lt == 0 && htms >= 0 && hi_i < 156)
				dec[hi_i] = cmul(make_float2(sr, si), scale);
		}
		wave_sync();
		// this kernel's lanes: 2..49 symbols 3 lane - 2 + j, 54 + 3 e symbol e (the other lanes' values are never stored: any valid
		// index); real((-j)^i x) and the slicer as the general kernel's flush() has them (component i & 1, sign by i & 2)
		auto pick = [&](int i) {
			const float d = reinterpret_cast<const float *>(dec + i)[i & 1];
			return __builtin_amdgcn_fmed3f(fmaf((i & 2) ? -0.5f : 0.5f, d, 0.5f), 0.0f, 1.0f);
		};
		const bool reg = lane >= 2 && lane < 50;
		const int i0 = reg ? 3 * lane - 2 : ((((lane - 54) * 11) >> 5) & 3);
		o.x = pick(i0);
		o.y = pick(reg ? i0 + 1 : 0);
		o.z = pick(reg ? i0 + 2 : 0);
		wave_sync();
		return true;
	};

	DIAG_DECL;
	unsigned j_next = 0, b_next = NB_NO_BURST;
	// the next burst of this wave from the ticket just taken: its number, the pool's draw at a group boundary, its prefetch
	// (items below j_plain are in the static range and off the pool's group boundaries: one scalar compare and one add give the
	// burst; the compiler joins the two branches in front of ONE copy of the prefetch loads, behind a flag -- kept apart, the
	// pool branch's copy waited for vmcnt(0), the stores just issued, in front of its loads: tools/isa_guard_nb.py checks every copy)
	const unsigned j_plain = (unsigned)uni((int)(!pooled ? items : items >= 16u ? items - 16u : 0u));
	auto advance = [&](const int taken) {
		j_next = (unsigned)taken;
		if (__builtin_expect(j_next < j_plain, 1)) {
			b_next = base16 + j_next;
			DIAG_MARK(17);
			prefetch(b_next);
		} else {
			b_next = burst_of(j_next);
			if (pooled && (j_next & 15u) == 0u && j_next + 16u >= items)
				pool_draw(j_next, b_next == NB_NO_BURST && j_next >= items);
			DIAG_MARK(17);
			if (b_next != NB_NO_BURST)
				prefetch(b_next);
		}
	};
	// left to the general kernel: the burst's flag byte, and "something was left" (plain stores: a type-mixed batch leaves a
	// million bursts, and a million atomics on one counter cost ten times the batch)
	// ("something was left" once per wave: a million stores to one address serialise in the L2 like a million atomics)
	auto mark_left = [&](const unsigned bb) {
		if (nb_lane_id() == 0) {
			reinterpret_cast<uint8_t *>(redo + TRX_REDO_HDR)[bb] = 1;
			if (!left_any)
				__hip_atomic_store(redo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		asm volatile("");                                           // (the lanes rejoin here, not in the loop's latch: see flush_records)
		left_any = 1;
	};
	// (the back edge is the likely one: the copies of the carried burst number and slot word are laid out behind the loop's last
	// test, not out of line with a jump of their own there and back)
	for (unsigned b = b_first; __builtin_expect(b != NB_NO_BURST, 1); b = b_next) {
		// (the prefetch offsets pass through an empty statement once per burst: the zero-extension of a value defined in front of
		// the loop is hoisted there as a register pair, and the prefetch loads then take the 64-bit vector address after all.  No
		// instruction, the same register.)
		asm volatile("" : "+v"(a_l4));
		asm volatile("" : "+v"(a_l4c));
		const int ticket = claim_issue(wg_next);
		const unsigned prm0 = (unsigned)uni((int)pre_prm);
		// ---- is this a slot the kernel handles?  (a slot of another type is flagged before anything is spent on its samples)
		const unsigned max_toa = prm0 >> 16;
		const int tsc = (prm0 >> 8) & 0xff;
#ifdef TRX_DIAG
		DIAG_MARK(12);                                              // (loop top: ticket issue, slot type)
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		DIAG_MARK(13);                                              // the prefetched samples' arrival, apart from their conversion
#endif
		// (one compare: a type or TSC that does not fit sets the high bits of the word whose upper half is max_toa)
		const unsigned slot_key = prm0 | (0u - ((prm0 & 0xf8ffu) ^ (unsigned)TRXHIP_TSC));
		// (a burst that is left to the general kernel is flagged where that is decided, on a rare side, and stores nothing:
		// pend_m = 0.  A value carried to the loop's end, not a test on the main path)
		int keep = -1;
		if (__builtin_expect(slot_key >= toa_lim, 0)) {
			// the prefetched samples are dropped, but they must be "used": a path that reaches the next prefetch with loads
			// the compiler still counts as outstanding makes it wait for vmcnt(0) right behind the new loads (measured: -4 %)
#pragma unroll
			for (int r = 0; r < NLD; r++)
				asm volatile("" :: "v"(pre_i[r]));
			store_pending();
			advance(claim_take(ticket));
			pend_rm = 0;
			mark_left(b);
			keep = 0;                                               // nothing of this burst is stored
		} else {
			// ---- phase 0: registers -> fp32 polyphase LDS; clip scan and energyDetect partial sums on the fly
			// (row r of the ten is offset 128 r of a_p: one address register, the offsets fit the 8-bit fields of ds_write2_b64)
			lds_v2f *const pload = reinterpret_cast<lds_v2f *>(a_p);
			float amax = 0.0f, epart = 0.0f;
#pragma unroll
			for (int r = 0; r < NLD; r++) {
				const v2f v = { (float)(int16_t)(pre_i[r] & 0xffffu), (float)(int16_t)(pre_i[r] >> 16) };
				// the tenth row has 49 samples: lanes 49..63 hold sample 624 once more (prefetch) -- the maximum may take it again,
				// the LDS may not: the row is written under a constant mask, with no compare and no branch round it
				if (r < NLD - 1)
					pload[16 * r] = v;
				else
					asm volatile("s_bfm_b64 exec, 49, 0\n\t"
						     "ds_write_b64 %0, %1 offset:%c2\n\t"
						     "s_mov_b64 exec, -1"
						     :: "v"(a_p), "v"(v), "n"(128 * (NLD - 1)) : "memory");
				asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(v.x), "v"(v.y));
				if (r < 5)
					epart = fmaf(v.x, v.x, fmaf(v.y, v.y, epart));
			}
			DIAG_MARK(14);
			// ---- the previous burst's output: 148 soft bits (lanes 2..49: symbols 3 lane - 2 + j as one 12-byte store, lanes
			// 54, 57, 60, 63: symbols 0..3) and the result record (lanes 0..7)
			store_pending();
			DIAG_MARK(16);
			// (a converted burst has at least five LDS writes behind the ticket's request -- ten rows, at most two per instruction --
			// and nothing else on lgkmcnt: the ticket is there when five are outstanding, the writes drain under the next block)
			advance(claim_take_behind<5>(ticket));
			DIAG_MARK(15);

			pend_rm = 0;                                                // (0xff: a slot without a burst -- the rare side below)
			{
				// maxAmplitude() > 30000 (:1711-1722, :1746)
				// (an integer in ONE scalar register: as a bool it is a lane mask, a register pair, from here to the record)
				int clip;
				asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, 1, 0" : "=s"(clip) : "s"(__ballot(amax > TRX_CLIP_THRESH)) : "scc");

				// ---- detectGeneralBurst window of a normal burst (:1887-1904: target 82, head 10, tail 6 + max_toa -> start 71,
				// len 16 + max_toa): decimated samples 56 .. 70 + len, one per lane
				const int len = 16 + (int)max_toa;
				__builtin_assume(len >= 16 && len <= 16 + NB_MAX_TOA);
				// (hand-placed blocks: tools/gen_nb_asm.py)  decimator of the window + the addition-only correlation's guard
				// (P, D[] and cz[] of this lane: compile-time offsets of a_w inside the blocks)
				// (windows of up to NB_ASM_CORR_MAX_LEN lags: the accumulators of DEC and CORR move across the lanes -- decimated sample i
				// ends in lane i + 4, lag k in lane k + NB_ASM_CORR_LANE0; wider windows: lane = sample / lag, the samples through LDS)
				// (DEC and CORR are ONE statement: their rare forms -- the wide window, a sample that fails the guard -- lie in the shadow
				// of CORR's computed jump, and the main path falls through to it)
				// ---- correlation (lag k in lane k + lag0; the right zero pad of cz[] is stored too)
				float v;                                                    // |corr|^2 by lane
				const int lag0 = (len <= NB_ASM_CORR_MAX_LEN) ? NB_ASM_CORR_LANE0 : 0;   // lane of lag 0
				asm volatile(NB_ASM_DECCORR
					     : [nrm] "=&v"(v)
					     : [aw] "v"(a_w), [zero] "v"(0), [len] "s"(len), [tsc] "s"(tsc)
					     : NB_ASM_CLOBBERS);
				{
					// ---- arg-max and the energyDetect sum (:1573-1585); the lane constants of the TOA search are fetched in the
					// reductions' wait states
					DIAG_MARK(3);
					int m_bits, es_bits, bidx;
					v2i kra, kbc;                                               // lane constants (lcn[]): (kr, ka), (kb, kic)
					int ktp;
					// (8 * lane for the two 8-byte entries is made here, in one of the block's temporaries: no register is kept for it)
					asm volatile(NB_ASM_AMAX("v_lshlrev_b32_e32 v90, 1, %[l4]", "ds_read_b64 %[kra], v90 offset:%c[lc]",
								 "ds_read_b64 %[kbc], v90 offset:%c[lc]+512", "ds_read_b32 %[ktp], %[l4] offset:%c[lc]+1024",
								 "s_nop 0", "s_nop 0", "s_nop 0", "s_nop 0")
						     "s_sub_u32 %[bidx], %[bidx], %[lag0]\n\t"                 // arg-max lane -> lag (no maximum: -lag0)
						     "s_waitcnt lgkmcnt(0)"
						     : [m] "=&s"(m_bits), [es] "=&s"(es_bits), [bidx] "=&s"(bidx), [kra] "=&v"(kra), [kbc] "=&v"(kbc), [ktp] "=&v"(ktp)
						     : [nrm] "v"(v), [ep] "v"(epart), [l4] "v"(a_l4), [lag0] "s"(lag0),
						       [lc] "n"((TRX_SINCV_LDS + 16 * WAVE + NB_COMP_ROWS * 36 + 16 + 64 + 5 * WAVE) * 4)
						     : NB_ASM_CLOBBERS);
					DIAG_MARK(4);
					// edge gate, peak-ratio gate, round A of the TOA bisection and its walk (DETA); round B, walk, peak value (DETB).
					// fastPeakDetect's "a maximum above zero exists" (:1120-1139) is DETA's edge gate: without one every |corr|^2 is +0,
					// the arg-max is the first lane and bidx = -lag0 <= 0 -- status 0, like any peak at the window's edge.
					// (the status lives in the blocks' fixed register NB_ASM_ST: their rare sides, behind the loop, write it too)
					// INVARIANT of NB_ASM_COLD (control flow the compiler does not see: it is entered from and left for labels inside DETA,
					// DETB and TAIL): the cold code reads and writes only registers that are in the clobber list of all three statements, and
					// NB_ASM_ST, which must stay the bound output of DETA and DETB.  No %[operand] of these statements may be named there (the
					// generator asserts it), and none of the statements may be duplicated (their labels would be, too: the assembler refuses).
					int st, e512;
					float km;
					asm volatile(NB_ASM_DETA
						     : [st] "=&" NB_ASM_ST(st), [e] "=&s"(e512), [km] "=&v"(km)
						     : [bidx] "s"(bidx), [len] "s"(len), [czb] "s"(lds_addr(cz)), [m] "s"(m_bits), [kr] "v"(kra.x), [ka] "v"(kra.y), [l16] "v"(a_l16),
						       [gkv] "v"(gkv), [c0] "v"(gc0)
						     : NB_ASM_CLOBBERS_ST);
					DIAG_MARK(5);
					int toa512 = 0, xr_bits = 0, xi_bits = 0;
					if (__builtin_expect(st == 1, 1)) {
						asm volatile(NB_ASM_DETB
							     : [st] "=&" NB_ASM_ST(st), [toa] "=&s"(toa512), [xr] "=&s"(xr_bits), [xi] "=&s"(xi_bits)
							     : [e] "s"(e512), [kb] "v"(kbc.x), [czb] "s"(lds_addr(cz)), [km] "v"(km)
							     : NB_ASM_CLOBBERS_ST);
						DIAG_MARK(6);
					}
					// ---- everything but "detected, every decision certified": ONE test on the main path, the rare side tells them apart
					if (__builtin_expect(st != 1, 0)) {
						// (an opaque copy: the three values are told apart HERE, not by a comparison tree in front of the main path's test)
						int stc = st;
						asm volatile("" : "+s"(stc));
						if (stc == 3) {
							// an uncertified early / late decision on the path: the search again in the reference's operand order
							const int lane = nb_lane_id();
							if (lane == 0)
								atomicAdd(&g_trx_fast_stats[0], 1ull);
							PeakConst pkc;
							pkc.flA = pkcl[0 * WAVE + lane]; pkc.loA = pkcl[1 * WAVE + lane]; pkc.hiA = pkcl[2 * WAVE + lane];
							pkc.offB = pkcl[3 * WAVE + lane]; pkc.ratio_off = pkcl[4 * WAVE + lane];
							c32 xcorr;
							// (pkcl[] is in peak_const()'s order; the one thing peak_detect_spec() takes by lane number is round A's
							// weights, which stand in the blocks' layout: the lane that holds this lane's node there)
							peak_detect_spec<true>(cz, bidx, sincv, pkc, nb_walk_dst<5>(lane), &toa512, &xcorr, wa4);
							toa512 = uni(toa512);
							xr_bits = uni(__float_as_int(xcorr.x));
							xi_bits = uni(__float_as_int(xcorr.y));
							st = 1;
						} else if (stc == 2) {
							// the gate is too close to call for the estimate
							if (nb_lane_id() == 0) atomicAdd(&g_trx_fast_stats[2], 1ull);
							mark_left(b);
							keep = 0;
						} else {
							// nothing found: rc (:1764), energy and RSSI (Transceiver.cpp:741,751), zero soft bits
							const float energy = __int_as_float(es_bits) * 0.0125f;
							const float rssi = rssi_db(full_scale, energy);
							const uint32_t flags = ((uint32_t)clip << 8) | (1u << 16);
							int word = clip ? -TRXHIP_SIGERR_CLIP : 0;
							word = put_lane<1>(word, 0.0f);
							word = put_lane<2>(word, 0.0f);
							word = put_lane<3>(word, 0.0f);
							word = put_lane<4>(word, 0.0f);
							word = put_lane<5>(word, energy);
							word = put_lane<6>(word, rssi);
							word = write_lane<7>(word, (int)flags);
							recw = word;
							o = (v3f){ 0.0f, 0.0f, 0.0f };
							pend_rm = 0xff;                                 // (a slot without a burst: the record goes with the soft bits)
						}
					}
					if (__builtin_expect(st == 1, 1)) {
						// ---- computeCI, amp, toa, the result record, 1 / amp; then demodGmskBurst of the usual geometry (TAIL)
						int ok, s_bits;
						float d0, d1, d2;
						const int t5 = (t5pk << (28 - 4 * tsc)) >> 28;
						asm volatile("s_setprio 0");
						asm volatile(NB_ASM_TAIL
							     : [ok] "=&s"(ok), [ssum] "=&s"(s_bits), [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2)
							     : [toa] "s"(toa512), [xr] "s"(xr_bits), [xi] "s"(xi_bits), [t5] "s"(t5), [ampb] "s"(lds_addr(lamp) + 32u * (unsigned)tsc),
							       [e8lo] "s"((unsigned)e8_addr), [e8hi] "s"((unsigned)(e8_addr >> 32)), [l16] "v"(a_l16), [l4] "v"(a_l4),
							       [aw] "v"(a_w), [pb] "s"(lds_addr(P)), [cb] "s"(lds_addr(comp) + 4u * (K4_U0 + TRX_FUSED_SH)), [db] "s"(lds_addr(D)),
							       [kic] "v"(kbc.y), [ktp] "v"(ktp)
							     : NB_ASM_CLOBBERS);
						DIAG_MARK(10);
						asm volatile("s_setprio 2");
						// (sliced in the block's output stage -- vectorSlicer: 0.5 * (x + 1), clamped (:546-556); the cold demodulator
						// below writes its own over them)
						o.x = d0;
						o.y = d1;
						o.z = d2;
						// the record's inputs are queued in front of the geometry test -- no test of "left" behind it, and none of them is
						// carried across the rare side's filter in a scalar register; a burst left to the general kernel there gives its
						// place in the queue back
						queue_record(xr_bits, xi_bits, es_bits, toa512 - t5 - 10 * 512, s_bits,
							     (int)((uint32_t)tsc | ((uint32_t)clip << 8) | (37u << 24)), b);
						if (__builtin_expect(!ok, 0)) {
							// TOA outside the straight-line geometry (an early burst, or one later than 9 symbols): the general form
							const int lane = nb_lane_id();
							if (lane == 0) atomicAdd(&g_trx_fast_stats[3], 1ull);
							const float *const h = lhdr + 8 * tsc;
							const float xr = __int_as_float(xr_bits), xi = __int_as_float(xi_bits);
							const float a0 = xr * h[2], a1 = xr * h[3], a2 = xi * h[3], a3 = xi * h[2];
							// amp = peak / gain (Complex.h:74), whole: block TAIL forms per lane only the component its multiplier needs
							const c32 ampv = make_float2(unif(a0 - a2), unif(a1 + a3));
							if (!demod_general(t5 + 10 * 512 - toa512, ampv, lane)) {
								q_n--;
								mark_left(b);
								keep = 0;
							}
						}
					}
				}
			}
		}
		pend_b = b;
		pend_m = keep;
		if (__builtin_expect(q_n == WAVE, 0))
			flush_records();
		DIAG_MARK(11);
	}
	// ---- the rare sides of the blocks DETA, DETB and TAIL (tools/gen_nb_asm.py: NB_ASM_COLD), entered from and left for labels
	// inside those blocks; here it is jumped over
	asm volatile(NB_ASM_COLD ::: NB_ASM_CLOBBERS);
	// ---- the last burst's output
	store_pending();
	flush_records();                                               // the records still in the registers
	DIAG_FLUSH();
	if (pooled) {
		__syncthreads();
		int tid0;                                                   // (re-derived: not a mask kept in scalar registers since the prologue)
		asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(tid0));
		// one wave of the workgroup -- whichever reaches the LDS counter first; the wave's index is not kept in a scalar
		// register through the burst loop for this
		if (tid0 == 0 && atomicAdd(wg_next + 1, 1) == 0) {
			const unsigned d = __hip_atomic_fetch_add(pool_ctr + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
			if (d == gridDim.x - 1u) {
				__hip_atomic_store(pool_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_store(pool_ctr + 1, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
			}
		}
	}
}
