// ResampRx.cpp -- see ResampRx.h.  All DSP runs on the GPU through trxhip_rx_frontend_* (include/trxhip.h).
#include <hip/hip_runtime.h>

#include <cerrno>

#include "ResampRx.h"
#include "trxhip.h"

extern "C" trxhip_ctx *trxsigproc_context(void);      /* sigProcLib.cpp: the context sigProcLibSetup() created */

ResampRx::ResampRx(size_t chunk_len, int resamp_p, int resamp_q)
	: chunk_len_(chunk_len), p_(resamp_p), q_(resamp_q), fe_(nullptr), stream_(nullptr), d_in_(nullptr), d_out_(nullptr),
	  cap_chunks_(0)
{
}

ResampRx::~ResampRx()
{
	if (fe_) trxhip_rx_frontend_destroy(fe_);
	if (d_in_) hipFree(d_in_);
	if (d_out_) hipFree(d_out_);
	if (stream_) hipStreamDestroy(static_cast<hipStream_t>(stream_));
}

bool ResampRx::init()
{
	if (!trxsigproc_context())
		return false;
	hipStream_t s;
	if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
		return false;
	stream_ = s;
	return trxhip_rx_frontend_create_chans(trxsigproc_context(), TRXHIP_RXFE_RESAMP, 1, (int)chunk_len_, p_, q_, &fe_) == TRXHIP_OK;
}

int ResampRx::pullBuffer(const int16_t *in, size_t n_chunks, std::vector<complex> &out)
{
	if (!fe_ || !in)
		return -EIO;
	if (!n_chunks)
		return 0;
	const size_t n_in = n_chunks * chunk_len_;                      /* complex int16 samples */
	const size_t n_out = n_in / q_ * p_;
	hipStream_t s = static_cast<hipStream_t>(stream_);
	if (n_chunks > cap_chunks_) {
		if (d_in_) hipFree(d_in_);
		if (d_out_) hipFree(d_out_);
		d_in_ = d_out_ = nullptr;
		if (hipMalloc(&d_in_, n_in * 4) != hipSuccess || hipMalloc(&d_out_, n_out * 8) != hipSuccess) {
			cap_chunks_ = 0;
			return -EIO;
		}
		cap_chunks_ = n_chunks;
	}
	if (hipMemcpyAsync(d_in_, in, n_in * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
	    trxhip_rx_frontend_pull(fe_, static_cast<const int16_t *>(d_in_), n_chunks, static_cast<float *>(d_out_), n_out, s) != TRXHIP_OK)
		return -EIO;
	const size_t old = out.size();
	out.resize(old + n_out);
	if (hipMemcpyAsync(&out[old], d_out_, n_out * 8, hipMemcpyDeviceToHost, s) != hipSuccess)
		return -EIO;
	return hipStreamSynchronize(s) == hipSuccess ? 0 : -EIO;
}

int ResampRx::pullScheduled(trxhip_rx_sched *sched, const int16_t *d_in, size_t n_chunks, float *d_work, size_t work_stride,
				uint8_t *d_pkt, int pkt_stride, uint16_t *d_pkt_len, trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots,
				size_t *n_slots, size_t *n_carried)
{
	return trxhip_rx_sched_pull_frontend(sched, fe_, d_in, n_chunks, d_work, work_stride, d_pkt, pkt_stride, d_pkt_len, d_ind, d_soft,
					     out_slots, n_slots, n_carried, stream_);
}
