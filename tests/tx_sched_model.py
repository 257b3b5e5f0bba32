"""Python restatement of the reference's downlink scheduling, for the tests of the burst scheduler (trxhip_tx_sched_*).

Cited functions (osmo-trx, Transceiver52M/ unless noted):
  Transceiver::driveTxPriorityQueue()   Transceiver.cpp:1087-1185   length / version checks, per-TN FN-order bookkeeping
  Transceiver::pushRadioVector()        Transceiver.cpp:416-481     stale bursts, current burst, filler, zeros
  Transceiver::updateFillerTable()      Transceiver.cpp:403-414
  Transceiver::setModulus()             Transceiver.cpp:483-512     (SETSLOT :1047-1048, RFMUTE :1068)
  TransceiverState(), init()            Transceiver.cpp:60-135      NONE on every slot, modulus 26, filler table
  Transceiver::init()                   Transceiver.cpp:218-219, :255-256   retransmission on channel 0 with FILLER_DUMMY;
                                                                     the other channels get FILLER_ZERO
  VectorQueue::getStaleBurst / getCurrentBurst  radioVector.cpp:124-148
  GSM::FNDelta / FNCompare, Time::operator<, incTN   GSM/GSMCommon.cpp:71-86, GSM/GSMCommon.h:141-150, :187-215
Duplicate (FN, TN): the earlier submission is transmitted, the later one is dropped as stale (the rule of include/trxhip.h).
The queue is a heap keyed by (FNDelta(fn, first clock FN), TN, id): the reference's GSM::Time order while every queued time
lies within half a hyperframe of the first clock, which the tests keep to.

A slot's source is ("burst", id), ("filler", id) -- id of the burst that wrote the entry, -1 for the initial filler -- or
("zero", -1).  Submission ids count the queued bursts from 0.
"""
import heapq

HYPERFRAME = 2715648
FILLER_DUMMY, FILLER_ZERO = 0, 1
COMB_NONE = 14


def fn_delta(v1, v2):
    half = HYPERFRAME // 2
    d = v1 - v2
    if d >= half:
        d -= HYPERFRAME
    elif d < -half:
        d += HYPERFRAME
    return d


def time_less(a, b):
    (f1, t1), (f2, t2) = a, b
    if f1 == f2:
        return t1 < t2
    return fn_delta(f1, f2) < 0


def modulus_of(comb, prev):
    if comb in (COMB_NONE, 1, 2, 3, 0):
        return 26
    if comb in (4, 5, 6):
        return 51
    if comb == 7:
        return 102
    if comb == 13:
        return 52
    return prev


COUNTERS = ("tx_stale_bursts", "tx_unavailable_bursts", "tx_trxd_fn_repeated", "tx_trxd_fn_outoforder", "tx_trxd_fn_skipped",
            "refused")


class Chan:
    def __init__(self, filler, retrans):
        self.filler, self.retrans = filler, retrans
        self.q = []                          # heap of (FNDelta(fn, ref), tn, id, fn)
        self.fill = {}                       # (modFN, tn) -> writer id
        self.chan_type = [COMB_NONE] * 8
        self.modulus = [26] * 8
        self.muted = False
        self.last = [None] * 8
        self.ctr = dict.fromkeys(COUNTERS, 0)


class Model:
    def __init__(self, chans, sps, filler):
        self.sps = sps
        self.ch = [Chan(filler if i == 0 else FILLER_ZERO, i == 0 and filler == FILLER_DUMMY) for i in range(chans)]
        self.next_id = 0
        self.clock = None

    def set_clock(self, fn, tn):
        self.clock = (fn, tn)
        self.ref = fn

    def set_slot(self, chan, tn, comb):
        c = self.ch[chan]
        c.chan_type[tn] = comb
        c.modulus[tn] = modulus_of(comb, c.modulus[tn])

    def set_muted(self, chan, on):
        self.ch[chan].muted = bool(on)

    def submit(self, chan, dgram):
        c = self.ch[chan]
        n = len(dgram)
        if not (n == 6 + 148 or (n == 6 + 444 and self.sps == 4)) or (dgram[0] >> 4) > 1:
            c.ctr["refused"] += 1
            return -1
        tn = dgram[0] & 7
        fn = int.from_bytes(bytes(dgram[1:5]), "big")
        if c.last[tn] is not None:
            delta = fn_delta(fn, c.last[tn])
            if delta == 0:
                c.ctr["tx_trxd_fn_repeated"] += 1
                return -1
            if delta < 0:
                c.ctr["tx_trxd_fn_outoforder"] += 1
            elif delta > 1 and chan == 0 and c.filler == FILLER_ZERO:
                c.ctr["tx_trxd_fn_skipped"] += delta - 1
            if delta > 0:
                c.last[tn] = fn
        else:
            c.last[tn] = fn
        i = self.next_id
        self.next_id += 1
        heapq.heappush(c.q, (fn_delta(fn, self.ref), tn, i, fn))
        return i

    def _top(self, c):
        if not c.q:
            return None
        _, tn, i, fn = c.q[0]
        return (fn, tn, i)

    def _update_fill(self, c, b):
        fn, tn, i = b
        c.fill[(fn % c.modulus[tn], tn)] = i

    def render(self, n_slots):
        """list (per channel) of n_slots sources"""
        out = [[] for _ in self.ch]
        fn0, tn0 = self.clock
        for ci, c in enumerate(self.ch):
            fn, tn = fn0, tn0
            for _ in range(n_slots):
                zeros = c.chan_type[tn] == COMB_NONE or c.muted
                while True:
                    b = self._top(c)
                    if b is None or not time_less(b[:2], (fn, tn)):
                        break
                    heapq.heappop(c.q)
                    c.ctr["tx_stale_bursts"] += 1
                    if c.retrans:
                        self._update_fill(c, b)
                b = self._top(c)
                if b is not None and b[:2] == (fn, tn):
                    heapq.heappop(c.q)
                    if c.retrans:
                        self._update_fill(c, b)
                    src = ("burst", b[2])
                else:
                    src = ("filler", c.fill.get((fn % c.modulus[tn], tn), -1))
                    if ci == 0 and c.filler == FILLER_ZERO:
                        c.ctr["tx_unavailable_bursts"] += 1
                if zeros:
                    src = ("zero", -1)
                out[ci].append(src)
                tn += 1
                if tn > 7:
                    tn, fn = 0, (fn + 1) % HYPERFRAME
        t = tn0 + n_slots
        self.clock = ((fn0 + t // 8) % HYPERFRAME, t % 8)
        return out


def dgram(fn, tn, bits, att=0, version=0):
    """a TRXD downlink datagram (trxd_hdr_v01_dl + one bit per byte)"""
    return bytes([(version << 4) | (tn & 7)]) + int(fn).to_bytes(4, "big") + bytes([att]) + bytes(int(b) & 1 for b in bits)
