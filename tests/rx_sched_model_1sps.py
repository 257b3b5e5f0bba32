"""The uplink scheduling model of tests/rx_sched_model.py at one sample per symbol: the same Model with the slot cutter of
RadioInterface::driveReceiveRadio() for mSPSRx == 1 (radioInterface.cpp:252-291) written as the reference's literal loop --

    burstSize = 156 + (tN % 4 == 0)
    while (recvSz > burstSize) { ...; incTN(); recvSz -= burstSize; burstSize = 156 + (tN % 4 == 0); }

-- so that the closed forms of csrc/trx_rx_sched.h are held against the loop itself.  Types, burstTime, the noise ring and the
counters work on slot indices and are the base class's."""
import rx_sched_model as M
from rx_sched_model import *  # noqa: F401,F403  (the constants: OFF, TSC, ..., COMB_*, HYPERFRAME, FLAG_*)

SYMBOLS_PER_SLOT = 156                # gSlotLen + 8, radioInterface.cpp:254


def burst_size(tn):
    return SYMBOLS_PER_SLOT + (tn % 4 == 0)


class Model(M.Model):
    def _loop(self, n_samples):
        """-> (slot lengths cut, samples left), from the clock's TN"""
        tn = self.clock[1]
        recv = self.carried + n_samples
        size = burst_size(tn)
        lens = []
        while recv > size:
            lens.append(size)
            tn = (tn + 1) % 8
            recv -= size
            size = burst_size(tn)
        return lens, recv

    def slots(self, n_samples):
        return len(self._loop(n_samples)[0])

    def slot_lens(self, n_samples):
        """the lengths of the slots the next pull of n_samples cuts"""
        return self._loop(n_samples)[0]

    def cut(self, n_samples):
        lens, left = self._loop(n_samples)
        # the base class moves the clock and plans the slots; it takes the count from slots() and sets carried by its own rule
        plan = super().cut(n_samples)
        assert len(plan[0]) == len(lens)
        self.carried = left
        return plan
