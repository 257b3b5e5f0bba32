#!/usr/bin/env python3
"""Bank conflicts of ds_read_b64 on the 4-SPS kernel's polyphase LDS layout (trx_kernel4.hip) when lane l reads sample
stride * l + c: entry ((s & 3) * PH_A + PH_M0 + (s >> 2)) of 8 bytes, banks (address / 4) mod 64, lane groups {0-31} and
{32-63} (MI355X_MICROARCH.md, LDS).  Answers "why does the exact demodulator's delay filter run 12 outputs per lane on 52
lanes and not 10 on 63" (VERDICT r3 item 4b): only strides that are a multiple of 4 keep every lane of an instruction in one
phase array and are conflict-free; every other stride is 2-way conflicted (or worse) for every PH_A, which doubles the LDS
time of the filter's 25-27 reads per lane and more than eats the 17 % fewer multiply-adds.
   python tools/lds_stride_conflicts.py"""


def conflicts(PH_A, stride, PH_M0=12):
    worst, tot, cnt = 0, 0, 0
    for c in range(4):
        for j in range(4):
            for g in range(2):
                banks = {}
                for l in range(32 * g, 32 * g + 32):
                    s = stride * l + c + j + 48
                    a = (s & 3) * PH_A + PH_M0 + (s >> 2)
                    for d in (2 * a, 2 * a + 1):
                        banks.setdefault(d % 64, set()).add(d)
                m = max(len(v) for v in banks.values())
                worst = max(worst, m)
                tot += m
                cnt += 1
    return worst, tot / cnt


def sinc_pairs():
    """The normal-burst kernel's gather on its sinc LUT (trx_kernel_nb.hip, block DETB of tools/gen_nb_asm.py): round B's lanes
    read column slot swz(f) (taps at and below the peak) and swz(512 - f) (above it) of the positions f = (e + offB[lane]) & 511,
    lanes 0..29 and 32..47, for every e round A can leave (16 mod 32).  As 4-byte reads of sincv[] (banks (a / 4) mod 32) and as
    8-byte reads of the row pairs (trx_tables.h trx_sincp_idx: slot s at byte 8 s of a pair, banks (a / 4) mod 64): an 8-byte slot
    takes banks 2 s, 2 s + 1, so two lanes of a half collide exactly when s is equal mod 32 -- in both forms.  The swizzle
    q ^ ((q >> 4) & 31) stays.  -> (worst, mean) LDS cycles per 32-lane half for the two forms"""
    def node_offset(n, inc0):
        lv = (n + 1).bit_length() - 1
        p = n + 1 - (1 << lv)
        return ((4 * p * inc0) >> lv) - (2 * inc0 - ((2 * inc0) >> lv))
    swz = lambda q: q ^ ((q >> 4) & 31)
    off_b = [node_offset(l >> 1, 8) + (1024 if l & 1 else 0) for l in range(30)] + [2 * k - 15 + 512 for k in range(16)]
    out = {}
    for width, nbanks in ((4, 32), (8, 64)):
        worst, tot, cnt = 0, 0, 0
        for e in range(16, 512, 32):
            for side in (lambda f: f, lambda f: 512 - f):
                for half in (off_b[:30], off_b[30:]):
                    banks = {}
                    for s in {swz(side((e + o) & 511)) for o in half}:          # (equal addresses broadcast)
                        for d in range(width // 4):
                            banks.setdefault((s * width // 4 + d) % nbanks, set()).add(s)
                    m = max(len(v) for v in banks.values())
                    worst, tot, cnt = max(worst, m), tot + m, cnt + 1
        out[width] = (worst, tot / cnt)
    return out


print("sinc LUT gather of round B, LDS cycles per 32-lane half (worst, mean): 4-byte reads", sinc_pairs()[4], " 8-byte row pairs", sinc_pairs()[8])
print("stride  PH_A=180 (worst, mean LDS cycles per group)   best PH_A in 164..229")
for stride in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16):
    best = min(((pa,) + conflicts(pa, stride) for pa in range(164, 230)), key=lambda t: (t[1], t[2]))
    print(f"{stride:6d}  {conflicts(180, stride)}   {best}")
