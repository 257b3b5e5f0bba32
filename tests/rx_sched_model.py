"""Python restatement of the reference's uplink scheduling, for the tests of the burst scheduler (trxhip_rx_sched_*).

Cited functions (osmo-trx, Transceiver52M/ unless noted):
  RadioInterface::driveReceiveRadio()   radioInterface.cpp:240-294   burstSize 625 at 4 SPS, `while (recvSz > burstSize)`, incTN
  GSM::Time::incTN, operator+=(int)     GSM/GSMCommon.h:141-159      FN modulo the hyperframe, the step may be negative
  Transceiver::expectedCorrType()       Transceiver.cpp:513-601      with its three subslot tables
  Transceiver::pullRadioVector()        Transceiver.cpp:665-815      burstTime (:690), OFF (:714-717), mute (:719-721), avg (:742),
                                                                     noise ring (:744-748), max_toa (:757-758), counters (:769-780)
  noiseVector::avg() / insert()         radioVector.cpp:84-108       float sum in index order / (float) size(); itr wraps at size()
  TransceiverState(), Transceiver()     Transceiver.cpp:60-72, :144-153   NONE on every slot, mNoises(20), mHandover all false
  HANDOVER / NOHANDOVER, SETMAXDLY[NB]  Transceiver.cpp:944-973

The DSP is not restated: run() takes the device's result records (rc, energy, ...) of the cut slots, the way the oracle's
orc_pull_radio_vector takes pow_avg and rc, so that every comparison with the device is exact.
"""
import numpy as np

HYPERFRAME = 2715648
SLOT = 625
NOISE_CNT = 20
OFF, TSC, EXT_RACH, RACH, SCH, EDGE, IDLE = range(7)
COMB_FILL, COMB_NONE, COMB_LOOPBACK = 0, 14, 15
SIGERR_CLIP = 2
FLAG_OFF, FLAG_MUTED, FLAG_IDLE = 1, 2, 4

TCHH_SUBSLOT = [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1]
SDCCH4_SUBSLOT = [3, 3, 3, 3, 0, 0, 2, 2, 2, 2, 3, 3, 3, 3] + [0] * 27 + [1, 1, 1, 1, 0, 0, 2, 2, 2, 2,
                  3, 3, 3, 3, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1] + [0] * 27 + [1, 1, 1, 1, 0, 0, 2, 2, 2, 2]
SDCCH8_SUBSLOT = [5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4,
                  5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 0, 0, 0, 0,
                  1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4,
                  5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 4, 4, 4, 4]
assert len(TCHH_SUBSLOT) == 26 and len(SDCCH4_SUBSLOT) == 102 and len(SDCCH8_SUBSLOT) == 102


def fn_add(fn, step):
    """GSM::Time::operator+=(int), GSMCommon.h:152-159"""
    fn += step
    if fn < 0:
        fn += HYPERFRAME
    return fn % HYPERFRAME


class NoiseRing:
    """noiseVector (radioVector.cpp:84-108) in float32"""

    def __init__(self):
        self.ring = np.zeros(NOISE_CNT, dtype=np.float32)
        self.itr = 0
        self.lev = np.float32(0.0)

    def insert(self, val):
        if self.itr >= NOISE_CNT:
            self.itr = 0
        self.ring[self.itr] = val
        self.itr += 1

    def avg(self):
        val = np.float32(0.0)
        for x in self.ring:
            val = np.float32(val + x)
        return np.float32(val / np.float32(NOISE_CNT))


class Model:
    def __init__(self, chans, tsc=0, ul_fn_offset=0, ext_rach=False, egprs=False):
        self.chans, self.tsc, self.ul_fn_offset, self.ext_rach, self.egprs = chans, tsc, ul_fn_offset, ext_rach, egprs
        self.chan_type = [[COMB_NONE] * 8 for _ in range(chans)]
        self.handover = [[False] * 8 for _ in range(8)]              # one table for all channels
        self.muted = [False] * chans
        self.version = [0] * chans
        self.max_toa_nb, self.max_toa_ab = 30, 63
        self.noise = [NoiseRing() for _ in range(chans)]
        self.ctr = [dict(rx_empty_burst=0, rx_clipping=0, rx_no_burst_detected=0) for _ in range(chans)]
        self.clock = None
        self.carried = 0

    def set_clock(self, fn, tn):
        self.clock = (fn, tn)
        self.carried = 0

    def set_slot(self, chan, tn, comb):
        self.chan_type[chan][tn] = comb

    def set_handover(self, tn, ss, on=True):
        self.handover[tn][ss] = bool(on)

    def set_muted(self, chan, on):
        self.muted[chan] = bool(on)

    def set_trxd_version(self, chan, v):
        self.version[chan] = v

    def set_max_toa(self, nb, ab):
        self.max_toa_nb, self.max_toa_ab = nb, ab

    def slots(self, n_samples):
        """radioInterface.cpp:272-291: the slots `while (recvSz > burstSize)` cuts from carried + n_samples"""
        recv, n = self.carried + n_samples, 0
        while recv > SLOT:
            recv -= SLOT
            n += 1
        return n

    def expected_type(self, fn, tn, chan):
        """expectedCorrType(), Transceiver.cpp:513-601"""
        comb, ho = self.chan_type[chan][tn], self.handover[tn]
        rach = EXT_RACH if self.ext_rach else RACH
        if comb == COMB_NONE:
            return OFF
        if comb == COMB_FILL:
            return IDLE
        if comb == 1:
            return RACH if ho[0] else TSC
        if comb == 2:
            if TCHH_SUBSLOT[fn % 26] == 1:
                return IDLE
            return RACH if ho[0] else TSC
        if comb == 3:
            return RACH if ho[TCHH_SUBSLOT[fn % 26]] else TSC
        if comb in (4, 6):
            return rach
        if comb == 5:
            m = fn % 51
            if 14 <= m <= 36 or m in (4, 5, 45, 46):
                return rach
            return RACH if ho[SDCCH4_SUBSLOT[fn % 102]] else TSC
        if comb == 7:
            if 12 <= fn % 51 <= 14:
                return IDLE
            return RACH if ho[SDCCH8_SUBSLOT[fn % 102]] else TSC
        if comb == 13:
            m = fn % 52
            if m in (12, 38):
                return RACH
            if m in (25, 51):
                return IDLE
            return EDGE if self.egprs else TSC
        if comb == COMB_LOOPBACK:
            return IDLE if 48 <= fn % 51 <= 50 else TSC
        return OFF

    def cut(self, n_samples):
        """One pull: the plan of the cut slots, per channel a list of (fn, tn, type, max_toa) in burstTime; the clock moves on"""
        n = self.slots(n_samples)
        self.carried = self.carried + n_samples - n * SLOT
        fn, tn = self.clock
        times = []
        for _ in range(n):
            times.append((fn_add(fn, self.ul_fn_offset), tn))
            tn += 1
            if tn > 7:
                tn, fn = 0, (fn + 1) % HYPERFRAME
        self.clock = (fn, tn)
        plan = []
        for c in range(self.chans):
            rows = []
            for bfn, btn in times:
                t = self.expected_type(bfn, btn, c)
                rows.append((bfn, btn, t, self.max_toa_ab if t in (RACH, EXT_RACH) else self.max_toa_nb))
            plan.append(rows)
        return plan

    def run(self, chan, plan, res):
        """pullRadioVector() over one channel's cut slots.  plan: cut()'s rows of the channel; res: the device's result records of
        the same slots (RESULT_DTYPE: rc, toa, ci, tsc, rssi, energy, idle, nbits_div4).  Returns a list of dicts: flags, rc, toa,
        ci, tsc, rssi, nbits, noise_lev; the ring and the counters move on."""
        out = []
        nz = self.noise[chan]
        for (fn, tn, typ, _), r in zip(plan, res):
            o = dict(fn=fn, tn=tn, type=typ, flags=0, rc=0, toa=np.float32(0), ci=np.float32(0), tsc=0, rssi=np.float32(0), nbits=0)
            if typ == OFF:                                           # :714-717
                o["flags"] = FLAG_OFF
            elif self.muted[chan]:                                   # :719-721
                o["flags"] = FLAG_MUTED | FLAG_IDLE
            else:
                avg = np.sqrt(np.float32(r["energy"]))               # :742, one path
                assert avg.dtype == np.float32
                if typ == IDLE:                                      # :744-748
                    nz.insert(avg)
                    nz.lev = nz.avg()
                o["rssi"] = np.float32(r["rssi"])
                rc = 0 if typ == IDLE else int(r["rc"])              # :754-755
                o["rc"] = rc
                if rc <= 0:                                          # :769-780
                    if rc == -SIGERR_CLIP:
                        self.ctr[chan]["rx_clipping"] += 1
                    elif rc != 0:
                        self.ctr[chan]["rx_no_burst_detected"] += 1
                    o["flags"] = FLAG_IDLE
                else:
                    o.update(toa=np.float32(r["toa"]), ci=np.float32(r["ci"]), tsc=int(r["tsc"]), nbits=4 * int(r["nbits_div4"]))
            o["noise_lev"] = np.float32(nz.lev)
            out.append(o)
        return out
