// MultiArfcnTx.h -- the transmit half of RadioInterfaceMulti (Transceiver52M/radioInterfaceMulti.{h,cpp}) on the GPU:
// per-ARFCN 4-SPS sample streams in, wideband int16 chunks out.  Same constants and channel mapping as the reference:
// MCHANS = 4 filterbank paths, Resampler(48, 65) from the GSM rate to the channel rate (radioInterfaceMulti.cpp:174-175),
// Synthesis(4, 192, 16), physical -> logical channel map getLogicalChan() (:92-124), int16 scale 1 / chans (:346-348).
#ifndef TRX_HOST_MULTIARFCNTX_H
#define TRX_HOST_MULTIARFCNTX_H
#include <cstddef>
#include <cstdint>
#include <vector>
#include "signalVector.h"

struct trxhip_tx_frontend;

class MultiArfcnTx {
public:
	static const size_t MCHANS = 4;                 /* radioInterfaceMulti.cpp:42 */
	explicit MultiArfcnTx(size_t chans, size_t block_len = 260, int resamp_p = 48, int resamp_q = 65);
	~MultiArfcnTx();
	bool init();                                    /* needs sigProcLibSetup() first; false without a GPU */
	/* One pushBuffer() worth of work for n_blocks blocks (radioInterfaceMulti.cpp:316-362): in[lchan] holds the next
	 * n_blocks * block_len low-rate samples of every logical channel (segments of the send buffers, in order).  Writes
	 * n_blocks * MCHANS * block_len * p / q int16 IQ pairs to wide, as handed to the device.  0 or -EIO. */
	int pushBuffer(const std::vector<std::vector<complex> > &in, size_t n_blocks, int16_t *wide);
	size_t chans() const { return chans_; }
	/* radioInterfaceMulti.cpp:92-124 */
	static int getLogicalChan(size_t pchan, size_t chans);
private:
	size_t chans_, block_len_;
	int p_, q_;
	trxhip_tx_frontend *fe_;
	void *stream_, *d_in_, *d_wide_;
	size_t cap_blocks_;
};
#endif
