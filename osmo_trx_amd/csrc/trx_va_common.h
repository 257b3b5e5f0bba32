// trx_va_common.h -- the device code of gr-gsm's 4-samples-per-symbol MLSE receiver (Transceiver52M/grgsm_vitac/) that the
// kernels of trx_va.hip (normal and access bursts) and trx_sch_sync.hip (synchronisation bursts) share: the polyphase burst
// layout, the training-sequence correlation, autocorrelation + matched filter, and the 16-state trellis with its traceback for
// four bursts per wave.  Operand order follows the reference statement by statement (-ffp-contract=off).
#ifndef TRX_VA_COMMON_H
#define TRX_VA_COMMON_H
#include "trx_device.h"

#define VA_BPW 4                       // bursts per wave: one per DPP row
#define VA_OSR 4
#define VA_CIR 5
#define VA_FL (VA_CIR * VA_OSR)
#define VA_NB 148
#define VA_AB 88
#define VA_FSTRIDE 152                 // floats per burst of trellis input symbols (148 + pad): the imaginary part of matched-filter
                                       // output k for even k, the real part for odd k -- all the trellis reads (one ds_read_b128 per 4 steps)
// The scaled burst is kept in a POLYPHASE layout, xs[ph * XA + i / 4] = x[i] with ph = i % 4: the matched filter walks
// the burst in steps of 4 samples per lane (one output symbol per lane), so consecutive lanes read consecutive words of
// one phase array (the linear layout was an 8-way bank conflict: 32-byte lane stride), and the training-sequence
// correlation (consecutive samples per lane) sees the four arrays 16 banks apart (XA = 8 mod 32).  Everything from x[L]
// to the end of the arrays is zero, which replaces the reference's "j < L" checks, and the arrays reach the last sample
// any stage can touch (start + 4 * 147 + 19 + 4 < 640) whatever L is.
#define VA_XA(L) (((((L) > 640 ? (L) : 640) + 3) / 4 + 31) / 32 * 32 + 8)

// The training sequences after gmsk_mapper() and conj() (grgsm_vitac.cpp:57-79, :122-145) are walks over
// {1, j, -1, -j}: out[i] = (+-j) * out[i-1] from the start point 1 / -1 (normal burst, first bit 0 / 1) or -j (access),
// then conjugated.  Stored as 2-bit quarter-turn codes (0: 1, 1: j, 2: -1, 3: -j) of the elements the channel
// estimate uses, i = 5 .. 20 of the 26 TSC bits and i = 5 .. 35 of the 41 access bits (TRAIN_BEGINNING = 5), element
// k at bits 2k, 2k+1 -- computed from the 3GPP TS 45.002 bit strings by the same walk.  tests/test_vitac_ref_cpu.py reads
// these literals and compares them with what the reference's compiled gmsk_mapper() makes of its own tables.
// VA_TSC_CODES1 is a deliberate deviation: row 1 of the reference's grgsm_vitac/constants.h has bit 20 inverted against
// 3GPP TS 45.002 (and the reference's own transmit table), which negates the last of the 16 elements used here; the
// reference therefore estimates TSC 1 channels with one tap negated and loses bits.  This is the 3GPP row, pinned to the
// compiled reference fed that row (the tsc1b_* records of tests/golden/ref_vitac_vectors.npz).
#define VA_TSC_CODES0 0x131319b9ull
#define VA_TSC_CODES1 0x9311b9b9ull
#define VA_TSC_CODES2 0x1913b3b3ull
#define VA_TSC_CODES3 0x191933b1ull
#define VA_TSC_CODES4 0xbb191193ull
#define VA_TSC_CODES5 0x991b3391ull
#define VA_TSC_CODES6 0x139bb9b1ull
#define VA_TSC_CODES7 0x91933b31ull
#define VA_ACC_CODES 0x464e4ccccc6c644ull

// correlate_sequence() (grgsm_vitac.cpp:147-155) for one lag: sum_ii seq[ii] * x[j0 + 4 ii], seq[ii] a quarter turn.
// std::complex's a * b with a in {1, j, -1, -j} is b with its parts swapped / negated exactly (the products with 0 only
// contribute +-0), so every term of the reference's sum is ONE v_pk_add_f32 whose op_sel / neg modifiers carry the
// quarter turn (unit_mac<>, trx_device.h): code 0: (x, y), 1: (-y, x), 2: (-x, -y), 3: (y, -x).  p = the lane's address of
// x[j0] inside its phase array: the taps are 4 samples = 1 entry apart.
// N > 32: the codes of elements 32 .. N-1 are CODES_HI.
template <unsigned long long CODES, int N, unsigned long long CODES_HI = 0ull>
__device__ __forceinline__ trx_v2f va_corr(const c32 *p)
{
	trx_v2f acc = { 0.0f, 0.0f };
#pragma unroll
	for (int k0 = 0; k0 < N; k0 += 8) {
		c32 x[8];
#pragma unroll
		for (int u = 0; u < 8; u++)
			if (k0 + u < N)
				x[u] = lds_c32(p + k0 + u);
#pragma unroll
		for (int u = 0; u < 8; u++)
			if (k0 + u < N) {
				const unsigned c = (unsigned)(((k0 + u < 32 ? CODES : CODES_HI) >> (2 * ((k0 + u) & 31))) & 3ull);
				const trx_v2f xv = { x[u].x, x[u].y };
				if (c == 0) acc = unit_mac<false, false>(acc, xv);
				if (c == 1) acc = unit_mac<true, false>(acc, xv);
				if (c == 2) acc = unit_mac<false, true>(acc, xv);
				if (c == 3) acc = unit_mac<true, true>(acc, xv);
			}
		__builtin_amdgcn_sched_barrier(0);
	}
	return acc;
}

// ---- detect_burst_generic (grgsm_vitac.cpp:82-108): rhh = conj(autocorrelation at multiples of 4), mafi.
// rhh[k] = conj(sum_{i >= 4k} cir[i] * conj(cir[i - 4k])): the 60 products in parallel (segment k = 20 - 4k of them,
// parked in prod[], 64 c32 of scratch), then lane k adds its segment in order.  sym[m]: the part of matched-filter output m that feeds the trellis.
__device__ __forceinline__ void va_rhh_mafi(const c32 *xs, int XA, const c32 *cir, c32 *prod, c32 *rhh, float *sym, int start,
					    int nbits, int lane)
{
	{
#pragma unroll
		for (int k = 0; k < VA_CIR; k++)
			if (lane >= k * VA_OSR && lane < VA_FL) {
				const c32 a = cir[lane], bb = cir[lane - k * VA_OSR];
				prod[(20 * k - 2 * k * (k - 1)) + lane - k * VA_OSR] = cmul(a, make_float2(bb.x, -bb.y));   // offsets 0, 20, 36, 48, 56
			}
		wave_sync();
		if (lane < VA_CIR) {
			const int seg = 20 * lane - 2 * lane * (lane - 1), len = VA_FL - VA_OSR * lane;
			float ar = 0.0f, ai = 0.0f;
#pragma unroll
			for (int i = 0; i < VA_FL; i++)
				if (i < len) {
					const c32 t = prod[seg + i];
					ar += t.x;
					ai += t.y;
				}
			rhh[lane] = make_float2(ar, -ai);
		}
		wave_sync();
	}
	{
		// mafi: filt[m] = sum_{ii < 20} x[start + 4m + ii] * cir[ii]: tap ii of every lane is phase (start + ii) & 3,
		// entry m + ((start + ii) >> 2) -- conflict-free, no range checks (zeros behind start + 4 nbits and behind L).
		// Taps in two halves of ten (registers), the three symbol rounds inside: every output still adds ii = 0 .. 19
		// in order.  Only one part of each output feeds the trellis: imaginary for even symbols, real for odd ones.
		trx_v2f acc[3] = { { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f } };
#pragma unroll
		for (int half = 0; half < 2; half++) {
			c32 hc[VA_FL / 2];
#pragma unroll
			for (int u = 0; u < VA_FL / 2; u++)
				hc[u] = cir[half * (VA_FL / 2) + u];           // wave-uniform: broadcast reads
#pragma unroll
			for (int rnd = 0; rnd < 3; rnd++) {
				if (rnd * WAVE < nbits) {                      // wave-uniform
					const int m = lane + rnd * WAVE;
					const int mc = m < VA_NB ? m : VA_NB - 1;      // lanes past the last symbol recompute it (not stored)
					// sample start + 4 mc + ii: phase (start + ii) & 3; four per-lane bases, then immediate offsets
					const c32 *pb[4];
#pragma unroll
					for (int k = 0; k < 4; k++)
						pb[k] = xs + ((start + k) & 3) * XA + ((start + k) >> 2) + mc;
#pragma unroll
					for (int u = 0; u < VA_FL / 2; u++) {
						const int ii = half * (VA_FL / 2) + u;
						const c32 xv = lds_c32(pb[ii & 3] + (ii >> 2));
						const c32 t = cmul(xv, hc[u]);
						acc[rnd] = acc[rnd] + (trx_v2f){ t.x, t.y };
					}
				}
			}
		}
#pragma unroll
		for (int rnd = 0; rnd < 3; rnd++) {
			const int m = lane + rnd * WAVE;
			if (m < nbits)
				sym[m] = (m & 1) ? acc[rnd].x : acc[rnd].y;
		}
	}
}

// =================== viterbi_detector (viterbi_detector.cc:62-392) for the four bursts of a wave, row = burst ===================
// meta[row] = {nbits (0: an idle row), start state, -, -}; words: 148 uint4 of scratch.  ones: bit k & 31 of word k >> 5 is set
// when output k of the lane's row is > 0 (every lane of a row ends with its row's string).
	// Add-compare-select as a DPP butterfly.  New state n comes from old states p = n >> 1 and p + 8, i.e. the pair
	// (S, S ^ 8) feeds the pair rotl4(S), rotl4(S ^ 8).  So a lane holding old state S computes new state rotl4(S) from its
	// own metric and the metric of the lane holding S ^ 8: lane l of a row holds state rotl4^k(l) at step k (identity again
	// every 4 steps) and its partner is lane l ^ (8 >> (k & 3)) of the same row -- one or two row-local DPP moves.
__device__ __forceinline__ void va_trellis(const float *sym_all, const c32 *rhh_all, const int4 *meta, uint4 *words, int lane,
					   unsigned (&ones)[5])
{
	const int row = lane >> 4, l4 = lane & 15;
	const int4 mt = meta[row];
	const int nbits_row = mt.x;
	const float *mysym = sym_all + row * VA_FSTRIDE;
	const c32 *rhh = rhh_all + row * 8;
	float inc[8];
	{
		const float r1 = rhh[1].y, r2 = rhh[2].x, r3 = rhh[3].y, r4 = rhh[4].x;
#pragma unroll
		for (int m = 0; m < 8; m++) {
			float v = (m & 1) ? r1 : -r1;
			v = (m & 2) ? v + r2 : v - r2;
			v = (m & 4) ? v + r3 : v - r3;
			inc[m] = v + r4;
		}
	}
	// per layout r = k & 3: the state this lane holds, and for the state n = rotl4(S) it produces (p = S & 7,
	// odd = S >> 3) the signed reference levels and the sign of the input symbol:
	//   imaginary step (r even): even n: o1 + sym - inc[p^2], o2 + sym + inc[p^5];  odd n: o1 - sym + inc[p^2], o2 - sym - inc[p^5]
	//   real step      (r odd):  even n: o1 - sym - inc[7-p], o2 - sym + inc[p];    odd n: o1 + sym + inc[7-p], o2 + sym - inc[p]
	float a1[4], a2[4];
	unsigned sflip[4];                                             // sign-bit mask applied to the symbol
	bool oddr[4];
#pragma unroll
	for (int r = 0; r < 4; r++) {
		const int S = ((l4 << r) | (l4 >> (4 - r))) & 15;          // rotl4^r(lane)
		const int p = S & 7;
		const bool odd = (S >> 3) != 0;
		float l1 = 0.0f, l2 = 0.0f;
#pragma unroll
		for (int m = 0; m < 8; m++) {
			l1 = (m == ((r & 1) ? 7 - p : (p ^ 2))) ? inc[m] : l1;
			l2 = (m == ((r & 1) ? p : (p ^ 5))) ? inc[m] : l2;
		}
		a1[r] = odd ? l1 : -l1;
		a2[r] = odd ? -l2 : l2;
		const bool plus = (r & 1) ? odd : !odd;
		sflip[r] = plus ? 0u : 0x80000000u;
		oddr[r] = odd;
	}
	float pm = (-10e30);
	if (l4 == mt.y)                                                // start state (>= 16 selects none, as in the reference's quirk)
		pm = 0.0f;
	const int nmax = max(max(uni(meta[0].x), uni(meta[1].x)), max(uni(meta[2].x), uni(meta[3].x)));
	// Only two bits of every path-metric difference survive into the +-127 output: d > 0 (the decision) and d != 0
	// (an output of +-0 is "not > 0").  Per step the 64 lanes' bits are two ballot words (row r = bits 16r .. 16r + 15,
	// bit l = the new state rotl4^(k+1)(l)), parked in LDS for the traceback.
	float4 f4 = *reinterpret_cast<const float4 *>(mysym);          // symbols 0 .. 3 of this row's burst
	for (int k0 = 0; k0 < nmax; k0 += 4) {                         // 148 and 88 are multiples of 4
		const float4 fc = f4;
		f4 = *reinterpret_cast<const float4 *>(mysym + k0 + 4);    // next group in flight while this one runs (pad: 152 entries)
		const bool act = k0 < nbits_row;                           // this row's burst is still running (rows may differ in length)
		unsigned long long posw[4], nzw[4];
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const float sym = (r == 0) ? fc.x : (r == 1) ? fc.y : (r == 2) ? fc.z : fc.w;
			const int pmi = __float_as_int(pm);
			int other;
			if (r == 0)      other = __builtin_amdgcn_update_dpp(pmi, pmi, 0x128, 0xf, 0xf, false);   // row_ror:8   (l ^ 8)
			else if (r == 1) {                                                                           // l ^ 4
				other = __builtin_amdgcn_update_dpp(pmi, pmi, 0x104, 0xf, 0x5, false);                   // row_shl:4 into banks 0, 2
				other = __builtin_amdgcn_update_dpp(other, pmi, 0x114, 0xf, 0xa, false);                 // row_shr:4 into banks 1, 3
			}
			else if (r == 2) other = __builtin_amdgcn_update_dpp(pmi, pmi, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1] (l ^ 2)
			else             other = __builtin_amdgcn_update_dpp(pmi, pmi, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2] (l ^ 1)
			const float po = __int_as_float(other);
			const float o1 = oddr[r] ? po : pm, o2 = oddr[r] ? pm : po;
			const float ss = __int_as_float(__float_as_int(sym) ^ (int)sflip[r]);
			const float c1 = (o1 + ss) + a1[r];
			const float c2 = (o2 + ss) + a2[r];
			const float d = c2 - c1;
			const float npm = (d < 0) ? c1 : c2;
			pm = act ? npm : pm;
			posw[r] = __ballot(d > 0);
			nzw[r] = __ballot(d != 0);
		}
		if (lane == 0) {                                           // one masked block per four steps
#pragma unroll
			for (int r = 0; r < 4; r++)
				words[k0 + r] = make_uint4((unsigned)posw[r], (unsigned)(posw[r] >> 32), (unsigned)nzw[r], (unsigned)(nzw[r] >> 32));
		}
	}
	wave_sync();

	// ---- best of the stop states {4, 12}; traceback with differential decoding (viterbi_detector.cc:340-392), every
	// lane of a row walking its row's path.  out[k] = +-d with the sign flipped when decision != out_bit, so
	// out[k] > 0 <=> out_bit && d != 0.  After a multiple of 4 steps lane l of a row holds state l again.
	const float m4 = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane & ~15) | 4) << 2, __float_as_int(pm)));
	const float m12 = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane & ~15) | 12) << 2, __float_as_int(pm)));
	// The walk tracks, instead of the state s_k, the LANE of the row that produced s_k's decision at step k,
	// l_k = rotr4^(k+1)(s_k) (new state n of step k sits at lane rotr4^(k+1)(n)): s_(k-1) = (s_k >> 1) + (decision << 3) is
	// rotr4(s_k) with bit 3 replaced by the decision, hence l_(k-1) = l_k with bit q = (3 - k) & 3 replaced by it -- no
	// rotation per step; bits 0 and 1 of s_k (its parity) sit at bits q and (q + 1) & 3 of l_k.  nbits = 0 mod 4: l = s at
	// the start.  The row's 16 decision / non-zero bits of step k are the u16 at bytes 2 row / 8 + 2 row of words[k].
	unsigned ln = (m12 > m4) ? 12u : 4u;
	unsigned out_bit = 0u;                                         // only bit 0 is meaningful (masked by `nonzero` where used)
#pragma unroll
	for (int i = 0; i < 5; i++)
		ones[i] = 0u;                                              // bit k & 31 of word k >> 5: output k is > 0
	const unsigned short *w16 = reinterpret_cast<const unsigned short *>(words) + row;
#pragma unroll
	for (int wq = 4; wq >= 0; wq--) {
		if (32 * wq >= nmax)
			continue;
		const int khi = (nmax - 1 < 32 * wq + 31) ? nmax - 1 - 32 * wq : 31;
		unsigned acc = 0u;
		unsigned pnext = w16[8 * (32 * wq + khi)], nnext = w16[8 * (32 * wq + khi) + 4];   // one step ahead
		for (int kk = khi; kk >= 0; kk--) {
			const int k = 32 * wq + kk;
			const unsigned pw = pnext, nw2 = nnext;
			const int kp = k > 0 ? k - 1 : 0;
			pnext = w16[8 * kp];
			nnext = w16[8 * kp + 4];
			if (k < nbits_row) {
				// type of step k: the last step processed is step nbits - 1 with real_imag = nbits & 1 = 0 (148 and 88 are
				// even) and the flag alternates, so real_imag(k) = (nbits - 1 - k) & 1 = (k + 1) & 1
				const unsigned real_imag = (unsigned)(k + 1) & 1u;
				const unsigned q = (unsigned)(3 - k) & 3u, q1 = (q + 1u) & 3u;
				const unsigned decision = (pw >> ln) & 1u, nonzero = (nw2 >> ln) & 1u;
				acc |= (out_bit & nonzero) << kk;
				out_bit = out_bit ^ real_imag ^ (ln >> q) ^ (ln >> q1);
				ln = (ln & ~(1u << q)) | (decision << q);
			}
		}
		ones[wq] = acc;
	}
}
#endif
