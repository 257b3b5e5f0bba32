"""A literal Python restatement of the MS uplink path of the reference, for the tests of trxhip_ms_tx_* (MsTxScheduler):

    ms_trx::submit_burst()       ms/ms.cpp:114-160
    ms_trx::set_ta()             ms/ms.h:299-303
    upper_trx::driveTx()         ms/ms_upper.cpp:328, :336   (the scale)
    submit_burst_ts()            ms/uhd_specific.h:266, ms/bladerf_specific.h:476   (ts + rxtxdelay)
    GSM::Time, GSM::FNDelta      GSM/GSMCommon.h:91-150, GSM/GSMCommon.cpp:71-78

and of the queue rules include/trxhip.h defines where the reference leaves the matter to its radio.  C's integer semantics are
written out: % and / truncate toward zero, `int - unsigned` is computed modulo 2^32, `int * unsigned` too."""
import numpy as np

HYPERFRAME = 2048 * 26 * 51        # gHyperframe, GSMCommon.h:72
ONE_TS_BURST_LEN = 625             # ms/ms.h:50 -- an `unsigned int`
U32 = 1 << 32

QUEUED, LATE, WRAPPED, EXPIRED, OVERLAP, FULL = range(6)


def c_rem(a, b):
    """C's a % b (the sign of the dividend)"""
    return a - b * int(a / b)


def c_div(a, b):
    """C's a / b on ints (toward zero)"""
    return int(a / b)


def fn_delta(v1, v2):
    """GSM::FNDelta, GSMCommon.cpp:71-78"""
    half = HYPERFRAME // 2
    d = v1 - v2
    if d >= half:
        d -= HYPERFRAME
    elif d < -half:
        d += HYPERFRAME
    return d


class Time:
    """GSM::Time, GSMCommon.h:91-150: int mFN, int mTN; TN() returns unsigned"""

    def __init__(self, fn=0, tn=0):
        self.fn, self.tn = fn, tn

    def decTN(self, step=1):        # :129-139
        assert step <= 8
        self.tn -= step
        if self.tn < 0:
            self.tn += 8
            self.fn -= 1
            if self.fn < 0:
                self.fn += HYPERFRAME
        return self

    def incTN(self, step=1):        # :141-150
        assert step <= 8
        self.tn += step
        if self.tn > 7:
            self.tn -= 8
            self.fn = (self.fn + 1) % HYPERFRAME
        return self


def scale_of(tx_full_scale, pwr):
    """driveTx(): int RSSI = (int)pwr; scaleVector(*txburst, txFullScale * pow(10, -RSSI / 10)) -- -RSSI / 10 is an int
    division, the product a double, complex(float) narrows it"""
    rssi = int(pwr)
    return np.float32(float(tx_full_scale) * 10.0 ** c_div(-rssi, 10))


def submit_burst(fn, tn, now_fn, now_tn, now_ts, timing_advance):
    """ms.cpp:114-160.  Returns (status, send_ts, diff_fn, diff_tn); send_ts is None where the reference returns before it."""
    target = Time(fn, tn)
    target.incTN(3)                                     # :118 ul dl offset
    target_fn, target_tn = target.fn, target.tn
    diff_fn = fn_delta(target_fn, now_fn)               # :123
    diff_tn = c_rem(target_tn - now_tn, 8)              # :124
    tosend = Time(diff_fn, 0)                           # :125
    if diff_tn > 0:
        tosend.incTN(diff_tn)
    else:
        tosend.decTN(-diff_tn)
    # :133 -- target_tn - now_time.TN(): int - unsigned, modulo 2^32, compared with (unsigned)3
    if diff_fn < 0 or (diff_fn == 0 and (target_tn - now_tn) % U32 < 3):
        return LATE, None, diff_fn, diff_tn
    # :139 -- tosend.FN() * 8 is int, * ONE_TS_BURST_LEN (unsigned int) is unsigned; TN() * ONE_TS_BURST_LEN is unsigned;
    # int64 + unsigned + unsigned - int
    send_ts = now_ts + (tosend.fn * 8 * ONE_TS_BURST_LEN) % U32 + (tosend.tn * ONE_TS_BURST_LEN) % U32 - timing_advance
    # the unsigned-TN case: not "too late" although the target slot lies behind the clock
    status = WRAPPED if diff_fn == 0 and target_tn < now_tn else QUEUED
    return status, send_ts, diff_fn, diff_tn


class MsTx:
    """the object's rules around submit_burst(): set_ta, the queue, the windows"""

    def __init__(self, tx_full_scale=2047, rxtx_delay=0, max_pending=1024):
        self.fs, self.delay, self.max_pending = tx_full_scale, rxtx_delay, max_pending
        self.timing_advance = 0
        self.q = []                  # [radio_ts, touched, key] by radio_ts
        self.rendered_end = None
        self.ctr = dict.fromkeys(("submitted", "queued", "late", "wrapped", "expired", "overlap", "full", "drawn", "missed"), 0)

    def set_ta(self, val):           # ms.h:299-303
        assert -127 < val < 128
        self.timing_advance = val * 4

    def submit(self, reqs, clock):
        """reqs: (fn, tn, pwr) triples; returns a list of dicts like the plan records"""
        now_fn, now_tn, now_ts = clock
        out = []
        for fn, tn, pwr in reqs:
            st, send_ts, dfn, dtn = submit_burst(int(fn), int(tn), now_fn, now_tn, now_ts, self.timing_advance)
            self.ctr["submitted"] += 1
            radio_ts = None if send_ts is None else send_ts + self.delay
            if st == QUEUED:
                if self.rendered_end is not None and radio_ts < self.rendered_end:
                    st = EXPIRED
                elif any(abs(b[0] - radio_ts) < ONE_TS_BURST_LEN for b in self.q):
                    st = OVERLAP
                elif len(self.q) >= self.max_pending:
                    st = FULL
                else:
                    self.q.append([radio_ts, False])
                    self.q.sort()
            self.ctr[("queued", "late", "wrapped", "expired", "overlap", "full")[st]] += 1
            out.append(dict(send_ts=send_ts or 0, radio_ts=radio_ts or 0, diff_fn=dfn, diff_tn=dtn, scale=scale_of(self.fs, pwr),
                            status=st))
        return out

    def render(self, n_samples, first_ts):
        """returns (n_drawn, [(offset in the window, first burst sample, length, radio_ts)] of the bursts drawn)"""
        assert self.rendered_end is None or first_ts >= self.rendered_end
        end = first_ts + n_samples
        drawn, pieces, keep = 0, [], []
        for b in self.q:
            ts = b[0]
            lo, hi = max(ts, first_ts), min(ts + ONE_TS_BURST_LEN, end)
            if lo < hi:
                pieces.append((lo - first_ts, lo - ts, hi - lo, ts))
                b[1] = True
            if ts + ONE_TS_BURST_LEN <= end:
                if b[1]:
                    self.ctr["drawn"] += 1
                    drawn += 1
                else:
                    self.ctr["missed"] += 1
            else:
                keep.append(b)
        self.q = keep
        self.rendered_end = end
        return drawn, pieces

    def state(self):
        d = dict(self.ctr)
        d.update(pending=len(self.q), rendered_end=self.rendered_end or 0, timing_advance=self.timing_advance,
                 window_set=int(self.rendered_end is not None))
        return d
