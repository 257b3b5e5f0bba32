"""A literal Python restatement of the reference's MS-side slot cutter, for the tests of the MS-side downlink slot scheduler
(tests/test_ms_sched_cpu.py, tests/test_gpu_ms_sched.py):

    time_keeper                          Transceiver52M/ms/ms.h:160-221
    GSM::Time::incTN / decTN             GSM/GSMCommon.h:129-150
    ms_trx::grab_bursts()                Transceiver52M/ms/ms_rx_lower.cpp:354-422
    ms_trx::handle_sch_or_nb()           :130-153   (only what touches the cutter: is the slot an SCH slot)
    ms_trx::handle_sch(false)            :194-203   temp_ts_corr_offset += -start when decoded and abs(start) > 1
    ms_trx::handle_sch(true)/decode_sch  :88-91, :196-198   what a first acquisition sets

The SCH `start` values come from outside: `starts(fn, tn, ts)` is called for every SCH slot the cutter hands to handle_sch() and
returns the start of a decoded burst, or None when decode_sch() failed.  The line numbers in the comments are the reference's."""

ONE_TS_BURST_LEN = 625                                             # ms.h:50
HYPERFRAME = 2048 * 26 * 51                                        # GSM::gHyperframe


def cdiv(a, b):
    """C's integer division and remainder (truncation toward zero), b > 0"""
    q = abs(a) // b
    q = -q if a < 0 else q
    return q, a - q * b


def is_sch(fn, tn):
    """gsm_sch_check_ts(), ms/sch.c:118-139"""
    return tn == 0 and fn % 51 in (1, 11, 21, 31, 41)


def is_fcch(fn, tn):
    """gsm_fcch_check_ts(), ms/sch.c:100-116"""
    return tn == 0 and fn % 51 in (0, 10, 20, 30, 40)


class TimeKeeper:
    """ms.h:160-221.  The asserts of inc_and_update_safe() count in `jumps`."""

    def __init__(self):
        self.fn, self.tn, self.ts, self.jumps = 0, 0, 0, 0

    def set(self, fn, tn, ts):                                     # :170-175
        self.fn, self.tn, self.ts = fn, tn, ts

    def _inc_tn(self):                                             # GSMCommon.h:141-150
        self.tn += 1
        if self.tn > 7:
            self.tn -= 8
            self.fn = (self.fn + 1) % HYPERFRAME

    def _dec_tn(self):                                             # GSMCommon.h:129-139
        self.tn -= 1
        if self.tn < 0:
            self.tn += 8
            self.fn -= 1
            if self.fn < 0:
                self.fn += HYPERFRAME

    def inc_both(self):                                            # :176-181
        self._inc_tn()
        self.ts += ONE_TS_BURST_LEN

    def inc_and_update(self, new_ts):                              # :182-188
        self._inc_tn()
        self.ts = new_ts

    def inc_and_update_safe(self, new_ts):                         # :189-198
        diff = new_ts - self.ts
        if not diff < 1.5 * ONE_TS_BURST_LEN or not diff > 0.5 * ONE_TS_BURST_LEN:
            self.jumps += 1
        self._inc_tn()
        self.ts = new_ts

    def dec_by_one(self):                                          # :199-204
        self._dec_tn()
        self.ts -= ONE_TS_BURST_LEN


class Refused(Exception):
    """where the reference's arithmetic leaves the buffer (read_n with a negative count): the scheduler refuses the pull"""


class Cutter:
    """grab_bursts() with its statics.  tracking=False: handle_sch() reports but temp_ts_corr_offset never moves the cut."""

    def __init__(self, starts=None, tracking=True):
        self.tk = TimeKeeper()
        self.partial_rdofs = 0
        self.first_call = False
        self.temp_ts_corr_offset = 0                               # ms.h:260
        self.first_sch_ts_start = -1                               # ms.h:261
        self.tracking = tracking
        self.starts = starts or (lambda fn, tn, ts: None)
        self.to_skip = 0
        self.plan = []

    def set_clock(self, fn, tn, ts):
        self.tk.set(fn, tn, ts)
        self.partial_rdofs, self.first_call, self.temp_ts_corr_offset = 0, False, 0

    def acquired(self, fn, start, first_sch_buf_rcv_ts):
        """decode_sch(bits, true) and handle_sch(true) on success"""
        self.tk.set(fn, 0, 0)                                      # timekeeper.set(fn, 0), :91
        self.first_sch_ts_start = first_sch_buf_rcv_ts + start - (4 * 4) - 1   # :198
        self.partial_rdofs, self.first_call, self.temp_ts_corr_offset = 0, True, 0

    def _handle_sch_or_nb(self, src_off):                          # :130-153
        fn, tn, ts = self.tk.fn, self.tk.tn, self.tk.ts
        self.plan.append((fn, tn, ts, src_off))
        if is_sch(fn, tn) and self.tracking:                       # handle_sch(false)
            start = self.starts(fn, tn, ts)
            if start is not None and abs(start) > 1:               # :194, :199
                self.temp_ts_corr_offset += -start                 # :201

    def grab_bursts(self, first_ts, n_samples):
        """One buffer.  Returns the slots cut as (fn, tn, ts, src_off); raises Refused with nothing changed."""
        saved = (self.tk.fn, self.tk.tn, self.tk.ts, self.tk.jumps, self.partial_rdofs, self.first_call, self.temp_ts_corr_offset,
                 self.to_skip)
        self.plan = []
        to_skip = 0                                                # :359
        if self.first_call:                                        # :362
            next_burst_start = first_ts - self.first_sch_ts_start  # :363
            fullts, fracts = cdiv(next_burst_start, ONE_TS_BURST_LEN)   # :364-365
            to_skip = ONE_TS_BURST_LEN - fracts                    # :366
            for i in range(max(fullts, 0)):                        # :368-369
                self.tk.inc_and_update(self.first_sch_ts_start + i * ONE_TS_BURST_LEN)
            if fracts:                                             # :371-372
                self.tk.inc_both()
            self.tk.dec_by_one()                                   # :375
            self.tk.set(self.tk.fn, self.tk.tn, first_ts - ONE_TS_BURST_LEN + to_skip)   # :377
            self.first_call = False                                # :382
        if self.partial_rdofs:                                     # :385
            first_remaining = ONE_TS_BURST_LEN - self.partial_rdofs
            rd = min(first_remaining, n_samples)                   # :387
            if rd != first_remaining:                              # :388-391
                self.partial_rdofs += rd
                return []
            self.tk.inc_and_update_safe(first_ts - self.partial_rdofs)   # :393
            self._handle_sch_or_nb(-self.partial_rdofs)            # :394
            to_skip = first_remaining                              # :395
        if self.tracking:
            to_skip -= self.temp_ts_corr_offset                    # :399
            if to_skip < 0:                                        # :403-406
                to_skip = 0
            else:
                self.temp_ts_corr_offset = 0
        left_after_burst = n_samples - to_skip                     # :408
        if left_after_burst < 0:
            (self.tk.fn, self.tk.tn, self.tk.ts, self.tk.jumps, self.partial_rdofs, self.first_call, self.temp_ts_corr_offset,
             self.to_skip) = saved
            self.plan = []
            raise Refused()
        full, frac = cdiv(left_after_burst, ONE_TS_BURST_LEN)      # :410-411
        for i in range(full):                                      # :413-417
            self.tk.inc_and_update_safe(first_ts + to_skip + i * ONE_TS_BURST_LEN)
            self._handle_sch_or_nb(to_skip + i * ONE_TS_BURST_LEN)
        self.partial_rdofs = frac                                  # :421
        self.to_skip = to_skip
        return self.plan
