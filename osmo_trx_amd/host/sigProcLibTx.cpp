// sigProcLibTx.cpp -- host shim, transmit side: the seven sigProcLib.h calls a transmitting osmo-trx makes
// (Transceiver.cpp:107-120 fills the filler table, :392-396 modulates every downlink burst) on top of
// trxhip_modulate_batch().  Each call is a batch of one on the calling thread's stream and scratch (sigProcLib.cpp of the
// shim); the modulation runs on the MI355X, the host only draws the reference's rand() values and moves the burst.
//
// Conventions: NULL without a context (sigProcLibSetup() failed or was not called), like demodAnyBurst(), and NULL for
// inputs that the reference refuses or that overrun the reference's own buffers (for example genRandAccessBurst(68, 4, tn):
// 156 bits into the 625-sample Laurent modulator, include/trxhip.h).  Built twice like sigProcLib.cpp: against the
// reference's headers (libtrxsigproc.so) and against host/compat (libtrxsigproc_sa.so).  BitVector is only read through its
// inline members (size(), operator[]), so the library imports nothing of BitVector.cpp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "shim_internal.h"
#include "../csrc/trx_tx_tables.h"

TRX_SHIM_NS_BEGIN
namespace {

/* the bit patterns the generators copy (3GPP TS 45.002), from the library's own transmit tables */
const trx_tx_tables *tx_tables()
{
	static trx_tx_tables t;
	static bool ok = false;
	static std::once_flag once;
	std::call_once(once, [] { ok = trxhip_tx_tables_generate_host(&t, sizeof(t)) == TRXHIP_OK; });
	return ok ? &t : nullptr;
}

/* scratch layout of a batch of one: [625 samples][length][descriptor][bits] */
constexpr size_t kOutStride = 625;
constexpr size_t kLenOff = kOutStride * 2 * sizeof(float);
constexpr size_t kPrmOff = kLenOff + 16;
constexpr size_t kBitsOff = kPrmOff + sizeof(trxhip_tx_params);
constexpr size_t kMaxBits = 3 * TRX_TX_EDGE_SYMS;

/* modulateBurst() / modulateEdgeBurst() of one burst: a new vector of the burst's length, or NULL */
signalVector *modulate_one(const uint8_t *bits, size_t nbits, int guard, int sps, int flags)
{
	trxhip_ctx *ctx = trxsigproc_context();
	if (!ctx || nbits > kMaxBits || guard < 0 || guard > 255)
		return NULL;
	void *sp = nullptr;
	uint8_t *d = static_cast<uint8_t *>(trxsigproc_thread_scratch(kBitsOff + kMaxBits, &sp));
	hipStream_t stream = static_cast<hipStream_t>(sp);
	if (!d)
		return NULL;
	/* host staging: descriptor followed by the bits, one upload */
	uint8_t h_in[sizeof(trxhip_tx_params) + kMaxBits];
	trxhip_tx_params prm;
	memset(&prm, 0, sizeof(prm));
	prm.nbits = (uint16_t)nbits;
	prm.guard = (uint8_t)guard;
	prm.flags = (uint8_t)flags;
	prm.scale_re = 1.0f;                                            /* unscaled: the caller's scaleVector() follows */
	memcpy(h_in, &prm, sizeof(prm));
	if (nbits)
		memcpy(h_in + sizeof(prm), bits, nbits);
	/* samples and length come back in one download */
	std::vector<float> h_out(2 * kOutStride + 4);
	if (hipMemcpyAsync(d + kPrmOff, h_in, sizeof(prm) + nbits, hipMemcpyHostToDevice, stream) != hipSuccess ||
	    trxhip_modulate_batch(ctx, d + kBitsOff, nbits ? nbits : 1, reinterpret_cast<const trxhip_tx_params *>(d + kPrmOff),
				  reinterpret_cast<float *>(d), NULL, 0.0f, kOutStride, reinterpret_cast<int32_t *>(d + kLenOff), 1,
				  sps, stream) != TRXHIP_OK ||
	    hipMemcpyAsync(h_out.data(), d, kLenOff + sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipStreamSynchronize(stream) != hipSuccess)
		return NULL;
	int32_t len;
	memcpy(&len, reinterpret_cast<const uint8_t *>(h_out.data()) + kLenOff, sizeof(len));
	if (len < 0 || (size_t)len > kOutStride)
		return NULL;
	signalVector *out = new signalVector(len);
	memcpy(out->begin(), h_out.data(), (size_t)len * 2 * sizeof(float));
	return out;
}

std::vector<uint8_t> bit_bytes(const BitVector &v)
{
	std::vector<uint8_t> b(v.size());
	for (size_t i = 0; i < b.size(); i++)
		b[i] = (uint8_t)v[i];
	return b;
}

}  // namespace

/* sigProcLib.cpp:970-979 */
signalVector *modulateBurst(const BitVector &wBurst, int guardPeriodLength, int sps, bool emptyPulse)
{
	const std::vector<uint8_t> b = bit_bytes(wBurst);
	return modulate_one(b.data(), b.size(), guardPeriodLength, sps, emptyPulse ? TRXHIP_TX_EMPTY_PULSE : 0);
}

/* sigProcLib.cpp:917-936 */
signalVector *modulateEdgeBurst(const BitVector &bits, int sps, bool emptyPulse)
{
	const std::vector<uint8_t> b = bit_bytes(bits);
	return modulate_one(b.data(), b.size(), 0, sps, TRXHIP_TX_8PSK | (emptyPulse ? TRXHIP_TX_EMPTY_PULSE : 0));
}

/* sigProcLib.cpp:768-807: rand() % 2 for bits 3 .. 59, then 88 .. 144 */
signalVector *genRandNormalBurst(int tsc, int sps, int tn)
{
	if ((tsc < 0) || (tsc > 7) || (tn < 0) || (tn > 7))
		return NULL;
	if ((sps != 1) && (sps != 4))
		return NULL;
	const trx_tx_tables *t = tx_tables();
	if (!t || !trxsigproc_context())
		return NULL;
	uint8_t bits[148];
	int i = 0;
	for (; i < 3; i++)
		bits[i] = 0;
	for (; i < 60; i++)
		bits[i] = rand() % 2;
	bits[i++] = 0;
	for (int n = 0; i < 87; i++, n++)
		bits[i] = t->tsc[tsc][n];
	bits[i++] = 0;
	for (; i < 145; i++)
		bits[i] = rand() % 2;
	for (; i < 148; i++)
		bits[i] = 0;
	return modulate_one(bits, 148, 8 + !(tn % 4), sps, 0);
}

/* sigProcLib.cpp:812-842: 88 + delay bits, rand() % 2 for the 36 data bits.  A negative delay is refused here (the reference
 * would size its BitVector from it) */
signalVector *genRandAccessBurst(int delay, int sps, int tn)
{
	if ((tn < 0) || (tn > 7))
		return NULL;
	if ((sps != 1) && (sps != 4))
		return NULL;
	if (delay > 68 || delay < 0)
		return NULL;
	const trx_tx_tables *t = tx_tables();
	if (!t || !trxsigproc_context())
		return NULL;
	uint8_t bits[88 + 68];
	int i = 0;
	for (; i < delay; i++)
		bits[i] = 0;
	for (int n = 0; i < 49 + delay; i++, n++)
		bits[i] = t->rach_burst[n];
	for (; i < 85 + delay; i++)
		bits[i] = rand() % 2;
	for (; i < 88 + delay; i++)
		bits[i] = 0;
	return modulate_one(bits, 88 + delay, 68 - delay + !(tn % 4), sps, 0);
}

/* sigProcLib.cpp:844-855: the zero vector of the burst's length */
signalVector *generateEmptyBurst(int sps, int tn)
{
	if ((tn < 0) || (tn > 7))
		return NULL;
	if (!trxsigproc_context())
		return NULL;
	size_t n;
	if (sps == 4)
		n = 625;
	else if (sps == 1)
		n = 148 + 8 + !(tn % 4);
	else
		return NULL;
	signalVector *v = new signalVector(n);
	memset(static_cast<void *>(v->begin()), 0, n * sizeof(*v->begin()));
	return v;
}

/* sigProcLib.cpp:857-863 */
signalVector *generateDummyBurst(int sps, int tn)
{
	if (((sps != 1) && (sps != 4)) || (tn < 0) || (tn > 7))
		return NULL;
	const trx_tx_tables *t = tx_tables();
	if (!t)
		return NULL;
	return modulate_one(t->dummy_burst, 148, 8 + !(tn % 4), sps, 0);
}

/* sigProcLib.cpp:869-915: 148 8-PSK symbols, psk8_table[rand() % 8] for the 2 x 58 data symbols.  Symbol index s is passed as
 * its bits (s & 1, s >> 1 & 1, s >> 2 & 1), which mapEdgeSymbols (:713-729) maps back to psk8_table[s] */
signalVector *generateEdgeBurst(int tsc)
{
	const int tail = 9 / 3, data = 174 / 3, train = 78 / 3;
	if ((tsc < 0) || (tsc > 7))
		return NULL;
	const trx_tx_tables *t = tx_tables();
	if (!t || !trxsigproc_context())
		return NULL;
	uint8_t bits[444];
	auto put = [&](int i, unsigned s) {
		bits[3 * i + 0] = s & 1;
		bits[3 * i + 1] = (s >> 1) & 1;
		bits[3 * i + 2] = (s >> 2) & 1;
	};
	int n, i = 0;
	for (; i < tail; i++)
		put(i, 7);
	for (; i < tail + data; i++)
		put(i, rand() % 8);
	for (n = 0; i < tail + data + train; i++, n++)
		put(i, (unsigned)(t->edge_tsc[tsc][3 * n] & 1) | ((unsigned)(t->edge_tsc[tsc][3 * n + 1] & 1) << 1) |
			       ((unsigned)(t->edge_tsc[tsc][3 * n + 2] & 1) << 2));
	for (; i < tail + data + train + data; i++)
		put(i, rand() % 8);
	for (; i < tail + data + train + data + tail; i++)
		put(i, 7);
	return modulate_one(bits, 444, 0, 4, TRXHIP_TX_8PSK);
}

TRX_SHIM_NS_END
