// MultiArfcnTx.cpp -- see MultiArfcnTx.h.  All DSP runs on the GPU through trxhip_tx_frontend_* (include/trxhip.h).
#include <hip/hip_runtime.h>

#include <cerrno>

#include "MultiArfcnTx.h"
#include "MultiArfcnRx.h"
#include "trxhip.h"

extern "C" trxhip_ctx *trxsigproc_context(void);      /* sigProcLib.cpp: the context sigProcLibSetup() created */

MultiArfcnTx::MultiArfcnTx(size_t chans, size_t block_len, int resamp_p, int resamp_q)
	: chans_(chans), block_len_(block_len), p_(resamp_p), q_(resamp_q), fe_(nullptr), stream_(nullptr),
	  d_in_(nullptr), d_wide_(nullptr), cap_blocks_(0)
{
}

MultiArfcnTx::~MultiArfcnTx()
{
	if (fe_) trxhip_tx_frontend_destroy(fe_);
	if (d_in_) hipFree(d_in_);
	if (d_wide_) hipFree(d_wide_);
	if (stream_) hipStreamDestroy(static_cast<hipStream_t>(stream_));
}

/* the same map as the receive side (radioInterfaceMulti.cpp:92-124) */
int MultiArfcnTx::getLogicalChan(size_t pchan, size_t chans)
{
	return MultiArfcnRx::getLogicalChan(pchan, chans);
}

bool MultiArfcnTx::init()
{
	if (chans_ < 1 || chans_ > 3 || !trxsigproc_context())
		return false;
	hipStream_t s;
	if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
		return false;
	stream_ = s;
	return trxhip_tx_frontend_create(trxsigproc_context(), TRXHIP_TXFE_MULTI, (int)chans_, (int)block_len_, p_, q_, 1.0f,
					 &fe_) == TRXHIP_OK;
}

int MultiArfcnTx::pushBuffer(const std::vector<std::vector<complex> > &in, size_t n_blocks, int16_t *wide)
{
	if (!fe_ || !wide || in.size() < chans_)
		return -EIO;
	if (!n_blocks)
		return 0;
	const size_t n_in = n_blocks * block_len_;                      /* per logical channel */
	const size_t n_wide = n_blocks * block_len_ / q_ * p_ * MCHANS; /* complex int16 samples */
	for (size_t l = 0; l < chans_; l++)
		if (in[l].size() < n_in)
			return -EIO;
	hipStream_t s = static_cast<hipStream_t>(stream_);
	if (n_blocks > cap_blocks_) {
		if (d_in_) hipFree(d_in_);
		if (d_wide_) hipFree(d_wide_);
		d_in_ = d_wide_ = nullptr;
		if (hipMalloc(&d_in_, chans_ * n_in * 8) != hipSuccess || hipMalloc(&d_wide_, n_wide * 4) != hipSuccess) {
			cap_blocks_ = 0;
			return -EIO;
		}
		cap_blocks_ = n_blocks;
	}
	for (size_t l = 0; l < chans_; l++)
		if (hipMemcpyAsync(static_cast<char *>(d_in_) + l * n_in * 8, in[l].data(), n_in * 8, hipMemcpyHostToDevice, s) != hipSuccess)
			return -EIO;
	/* convert_float_short(convertSendBuffer[0], ..., 1.0 / (float) mChans, ...): radioInterfaceMulti.cpp:346-348 */
	const float scale = (float)(1.0 / (float)chans_);
	if (trxhip_tx_frontend_push(fe_, static_cast<const float *>(d_in_), n_in, n_blocks, nullptr, static_cast<int16_t *>(d_wide_),
				    scale, s) != TRXHIP_OK ||
	    hipMemcpyAsync(wide, d_wide_, n_wide * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
		return -EIO;
	return hipStreamSynchronize(s) == hipSuccess ? 0 : -EIO;
}
