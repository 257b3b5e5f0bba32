// ref_shim_vitac.cpp -- C handles around the reference's MLSE front end (Transceiver52M/grgsm_vitac/grgsm_vitac.cpp and
// viterbi_detector.cc, compiled unmodified by oracle/Makefile into oracle/_ref/libref_vitac.so; oracle/compat/ supplies the
// one libosmocore header they include).  Test infrastructure: pins the restatements of the channel estimate, the matched
// filter and the search geometry in oracle/trx_oracle.c, tests/sch_sync_model.py, tests/ms_rx_model.py and the kernels.
//
// Every wrapper copies the caller's n samples into a zeroed buffer with VT_FRONT zeros in front and VT_BACK behind: the
// reference reads input[burst_start + 4 * 147 + 19] and beyond and allows starts down to -39 (ms_upper.cpp:224-225), -188
// in a buffer search; the oracle and the models define x = 0 outside [0, n).  Outputs are zeroed before the call
// (detect_burst_ab writes 88 values).
#include <algorithm>
#include <complex>
#include <cstring>
#include <vector>

#include "grgsm_vitac.h"

extern gr_complex d_acc_training_seq[N_ACCESS_BITS];
extern gr_complex d_sch_training_seq[N_SYNC_BITS];
extern gr_complex d_norm_training_seq[TRAIN_SEQ_NUM][N_TRAIN_BITS];
int get_chan_imp_resp(const gr_complex *input, gr_complex *chan_imp_resp, int search_start_pos, int search_stop_pos,
		      gr_complex *tseq, int tseqlen, float *corr_max);

#define VT_FRONT 256
#define VT_BACK 1024
#define VT_CIR (CHAN_IMP_RESP_LENGTH * 4)

namespace {
struct padded {
	std::vector<gr_complex> v;
	padded(const float *x, int n) : v((size_t)VT_FRONT + (size_t)std::max(n, 0) + VT_BACK, gr_complex(0.0f, 0.0f))
	{
		for (int i = 0; i < n; i++)
			v[VT_FRONT + i] = gr_complex(x[2 * i], x[2 * i + 1]);
	}
	const gr_complex *p() const { return &v[VT_FRONT]; }
};

void init_once()
{
	static const bool done = (initvita(), true);
	(void)done;
}

int finish(const gr_complex *cir, float *cir_out, int start)
{
	std::memcpy(cir_out, cir, VT_CIR * sizeof(gr_complex));
	return start;
}
} // namespace

extern "C" {

// 0 when the search [start_pos, stop_pos) with a sequence of tseqlen elements and the demodulation that may follow stay
// inside the padded copy of n samples
int ref_vitac_geometry_ok(int n, int start_pos, int stop_pos, int tseqlen)
{
	return n >= 0 && tseqlen > 0 && start_pos >= -VT_FRONT && stop_pos - start_pos >= VT_CIR &&
	       stop_pos + 4 * (tseqlen - 1) <= n + VT_BACK ? 0 : -1;
}

int ref_vitac_norm_imp_resp(const float *x, int n, int bcc, float *cir, float *corr_max)
{
	init_once();
	if (bcc < 0 || bcc >= TRAIN_SEQ_NUM)
		return -100000;
	padded in(x, n);
	gr_complex c[VT_CIR] = {};
	*corr_max = 0.0f;
	return finish(c, cir, get_norm_chan_imp_resp(in.p(), c, corr_max, bcc));
}

int ref_vitac_access_imp_resp(const float *x, int n, int max_delay, float *cir, float *corr_max)
{
	init_once();
	if (max_delay < 0 || max_delay > 63)
		return -100000;
	padded in(x, n);
	gr_complex c[VT_CIR] = {};
	*corr_max = 0.0f;
	return finish(c, cir, get_access_imp_resp(in.p(), c, corr_max, max_delay));
}

int ref_vitac_sch_imp_resp(const float *x, int n, float *cir)
{
	init_once();
	padded in(x, n);
	gr_complex c[VT_CIR] = {};
	return finish(c, cir, get_sch_chan_imp_resp(in.p(), c));
}

// get_sch_buffer_chan_imp_resp(): len = n; needs one whole window, n >= 64 * 8 + 20
int ref_vitac_sch_buffer_imp_resp(const float *x, int n, float *cir, float *corr_max)
{
	init_once();
	if (n < N_SYNC_BITS * 8 + VT_CIR)
		return -100000;
	padded in(x, n);
	gr_complex c[VT_CIR] = {};
	*corr_max = 0.0f;
	return finish(c, cir, get_sch_buffer_chan_imp_resp(in.p(), c, (unsigned)n, corr_max));
}

// get_chan_imp_resp() with the caller's sequence (tseqlen complex values) and search window; returns the absolute position
int ref_vitac_chan_imp_resp(const float *x, int n, int start_pos, int stop_pos, const float *tseq, int tseqlen, float *cir,
			    float *corr_max)
{
	init_once();
	if (ref_vitac_geometry_ok(n, start_pos, stop_pos, tseqlen))
		return -100000;
	padded in(x, n);
	std::vector<gr_complex> seq(tseqlen);
	for (int i = 0; i < tseqlen; i++)
		seq[i] = gr_complex(tseq[2 * i], tseq[2 * i + 1]);
	gr_complex c[VT_CIR] = {};
	*corr_max = 0.0f;
	return finish(c, cir, get_chan_imp_resp(in.p(), c, start_pos, stop_pos, seq.data(), tseqlen, corr_max));
}

void ref_vitac_gmsk_mapper(const unsigned char *bits, int nitems, float start_re, float start_im, float *out)
{
	std::vector<gr_complex> o(nitems);
	gmsk_mapper(bits, nitems, o.data(), gr_complex(start_re, start_im));
	std::memcpy(out, o.data(), (size_t)nitems * sizeof(gr_complex));
}

// the sequences initvita() prepared: norm[9][26], acc[41], sch[64] complex values
void ref_vitac_training_seqs(float *norm, float *acc, float *sch)
{
	init_once();
	std::memcpy(norm, d_norm_training_seq, sizeof(d_norm_training_seq));
	std::memcpy(acc, d_acc_training_seq, sizeof(d_acc_training_seq));
	std::memcpy(sch, d_sch_training_seq, sizeof(d_sch_training_seq));
}

// detect_burst_nb / detect_burst_ab with an explicit start state (0 .. 15: the reference stores out of bounds above);
// out: 148 values, zeroed first.  Returns -1 where the call would leave the padded copy or the start state's range.
static int detect(const float *x, int n, const float *cir, int burst_start, int ss, signed char *out, bool ab)
{
	init_once();
	std::memset(out, 0, BURST_SIZE);
	if (ss < 0 || ss > 15 || burst_start < -VT_FRONT || burst_start + 4 * BURST_SIZE + VT_CIR > n + VT_BACK)
		return -1;
	padded in(x, n);
	gr_complex c[VT_CIR];
	std::memcpy(c, cir, sizeof(c));
	sbit_t o[BURST_SIZE] = {};
	if (ab)
		detect_burst_ab(in.p(), c, burst_start, o, ss);
	else
		detect_burst_nb(in.p(), c, burst_start, o, ss);
	std::memcpy(out, o, BURST_SIZE);
	return 0;
}

int ref_vitac_detect_burst_nb(const float *x, int n, const float *cir, int burst_start, int ss, signed char *out)
{
	return detect(x, n, cir, burst_start, ss, out, false);
}

int ref_vitac_detect_burst_ab(const float *x, int n, const float *cir, int burst_start, int ss, signed char *out)
{
	return detect(x, n, cir, burst_start, ss, out, true);
}
}
