// ResampRx.h -- the receive half of RadioInterfaceResamp (Transceiver52M/radioInterfaceResamp.{h,cpp}) on the GPU: int16
// chunks of one channel as read from the device in, the 4-SPS sample stream out.  pullBuffer() (:156-193) converts the chunk
// (convert_short_float) and runs dnsampler = Resampler(p, q) over it with the history it carries between calls: (65, 96) on
// 1536-sample chunks at 64 MHz clocking, (52, 75) on 1200 at 100 MHz (:36-41, :98-118).
#ifndef TRX_HOST_RESAMPRX_H
#define TRX_HOST_RESAMPRX_H
#include <cstddef>
#include <cstdint>
#include <vector>
#include "signalVector.h"

struct trxhip_rx_frontend;
struct trxhip_rx_sched;
struct trxhip_ul_ind;

class ResampRx {
public:
	explicit ResampRx(size_t chunk_len = 1536, int resamp_p = 65, int resamp_q = 96);
	~ResampRx();
	bool init();                                    /* needs sigProcLibSetup() first; false without a GPU */
	/* One or more pullBuffer() calls' worth of work: in = n_chunks * chunk_len int16 IQ samples as read from the device.
	 * Appends n_chunks * chunk_len * p / q samples to out.  0 or -EIO. */
	int pullBuffer(const int16_t *in, size_t n_chunks, std::vector<complex> &out);
	/* RadioInterface::driveReceiveRadio() as one step, on the device: the same chunks through this object's front end and the
	 * one-channel uplink scheduler sched (on sigProcLibSetup()'s context; its sps states this object's output rate) to TRXD
	 * indications -- trxhip_rx_sched_pull_frontend() (include/trxhip.h) with this object's front-end handle and stream.  Every
	 * pointer is device memory: d_in as `in` above, d_work the call's work row, the rest the scheduler's outputs.
	 * A scheduler created with TRXHIP_FLAG_USE_VA (cfg->use_va; d_in is then what the radio read 20 samples early) is taken
	 * as any other: the handle is passed through.  Asynchronous; returns the call's TRXHIP_* code. */
	int pullScheduled(trxhip_rx_sched *sched, const int16_t *d_in, size_t n_chunks, float *d_work, size_t work_stride,
			  uint8_t *d_pkt, int pkt_stride, uint16_t *d_pkt_len, trxhip_ul_ind *d_ind, float *d_soft, size_t out_slots,
			  size_t *n_slots, size_t *n_carried);
	void *stream() const { return stream_; }        /* the stream pullBuffer() and pullScheduled() work on */
private:
	size_t chunk_len_;
	int p_, q_;
	trxhip_rx_frontend *fe_;
	void *stream_, *d_in_, *d_out_;
	size_t cap_chunks_;
};
#endif
