"""The reference's MS-side receive gain control, restated literally in numpy float32.  Nothing is imported from the product.

    normed_abs_sum()               ms/ms.h:116-126
    ms_trx::maybe_update_gain()    ms/ms_rx_lower.cpp:101-126 (called per cut slot, :149-150)
    search_for_sch()'s level gate  ms/ms_rx_lower.cpp:333-347

Every float operation is rounded to float32 on its own (the reference is generic C++, FLT_EVAL_METHOD 0, no contraction).
Defined where the reference is not: an SCH slot is measured on its own 625 samples; an applied decision is the
object's rx_gain at once."""
import numpy as np

F = np.float32
AVGBURST_NUM = 8 * 20          # :104
MAX_GAIN = 60                  # :118, :338
RAISE, SEARCH = 0, 1


def normed_abs_sum(iq):
    """iq: int16[len, 2] (or any int16 array: its values in memory order).  float sum = 0; for i < 2 * len: sum += std::abs(ptr[i]);
    sum /= 2 * len -- np.add.accumulate in float32 IS the sequential sum; abs of the promoted int (abs(-32768) = 32768)"""
    v = np.abs(np.asarray(iq, dtype=np.int16).reshape(-1).astype(np.int32)).astype(F)      # every |value| <= 32768 is a float32
    s = np.add.accumulate(v, dtype=F)[-1] if len(v) else F(0)
    return F(s) / F(len(v))


class Agc:
    """maybe_update_gain()'s statics (gain_check, runmean), rxgain, and a record of every decision"""

    def __init__(self, rx_full_scale, rx_gain):
        self.fs = int(rx_full_scale)                               # const unsigned int rxFullScale
        self.rxgain = F(rx_gain)                                   # float rxgain
        self.gain_check = 0
        self.runmean = F(0)
        self.slots = 0
        self.records = []                                          # {slot, runmean, sum, old_gain, new_gain, applied}

    def update(self, s):
        s = F(s)
        rx_max_cutoff = (self.fs * 2) // 3                         # :106, unsigned
        gc = self.gain_check
        if gc:                                                     # :110
            n = F(gc + 2)
            self.runmean = F(F(F(F(self.runmean * n) - F(1)) + s) / n)
        else:
            self.runmean = s
        if gc == AVGBURST_NUM - 1:                                 # :112
            gainoffset = bool(self.runmean < F(4 if self.fs // 4 else 2))      # :114, `auto` from a comparison: a bool
            gainoffset = bool(self.runmean < F(2 if self.fs // 2 else 1))      # :115
            off = F(int(gainoffset))
            newgain = F(self.rxgain + off) if self.runmean < F(rx_max_cutoff) else F(self.rxgain - off)     # :116
            applied = bool(newgain != self.rxgain and newgain <= F(MAX_GAIN))  # :118
            self.records.append(dict(slot=self.slots, runmean=float(self.runmean), sum=float(s), old_gain=float(self.rxgain),
                                     new_gain=float(newgain), applied=int(applied)))
            if applied:
                self.rxgain = newgain                              # setRxGain(newgain), at once
            self.runmean = F(0)                                    # :123
        self.gain_check = (gc + 1) % AVGBURST_NUM                  # :125
        self.slots += 1

    def run(self, levels):
        for s in levels:
            self.update(s)

    def state(self):
        """what the product's agc_state() reports, but `enable`"""
        applied = sum(r["applied"] for r in self.records)
        return dict(rx_gain=float(self.rxgain), runmean=float(self.runmean), gain_check=self.gain_check, slots=self.slots,
                    decisions=len(self.records), applied=applied, ring=self.records[-8:])


def gate(level, rx_full_scale, rx_gain):
    """:334-344: (SEARCH, rxgain) when sum > target_val || rxgain >= 60, else (RAISE, rxgain + 4)"""
    target_val = int(rx_full_scale) // 8
    if F(level) > F(target_val) or F(rx_gain) >= F(MAX_GAIN):
        return SEARCH, float(F(rx_gain))
    return RAISE, float(F(F(rx_gain) + F(4)))


def same_state(got, want):
    """the product's agc_state() dict against Agc.state(), bit for bit (floats compared as float32 patterns)"""
    def bits(x):
        return np.float32(x).view(np.uint32)

    for k in ("gain_check", "slots", "decisions", "applied"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("rx_gain", "runmean"):
        assert bits(got[k]) == bits(want[k]), (k, got[k], want[k])
    assert len(got["ring"]) == len(want["ring"])
    for g, w in zip(got["ring"], want["ring"]):
        assert (g["slot"], g["applied"]) == (w["slot"], w["applied"]), (g, w)
        for k in ("runmean", "sum", "old_gain", "new_gain"):
            assert bits(g[k]) == bits(w[k]), (k, g, w)
