"""The TOA search's walks of the normal-burst kernel (tools/gen_nb_asm.py: walk_rank, walk_first_zero, careful_walk; blocks
DETA / DETB and NB_ASM_COLD of csrc/trx_nb_asm.inc), modelled on the CPU.

peakDetect()'s early / late bisection (sigProcLib.cpp:1141-1186) moves right where |early| < |late| and left otherwise.  The
kernel evaluates all nodes of a round at once, node (level k, index i) in POSITION order on lanes 2 r, 2 r + 1, r = walk_rank, and
its compare leaves bit 2 r for a certain "right", bit 2 r + 1 for a certain "left", neither for an uncertified node (both is
no outcome of the compare: hi_E < lo_L <= hi_L < lo_E <= hi_E).  A certified mask whose decisions, read in position order, are
n times "right" and then "left" ends at leaf n: the main path finds that n as a first zero.  Every other mask takes the
level-by-level walk in the cold code.

Checked here, on a numpy model of both forms AND on the generated instructions themselves (a small interpreter of the scalar
instructions between the compare and .Lnb_d?_walked, cold code included):
  * the first-zero form is taken exactly on the certified monotone masks and gives the reference walk's leaf there;
  * every other mask gives what the reference's walk over heap-ordered nodes gives: its leaf, or "unsure" when a node ON the
    path is uncertified;
  * round A (31 nodes): all 32 monotone masks, every mask at Hamming distance 1 and 2 of one (15 904), 10^6 seeded random
    certified masks and 10^6 with uncertified nodes (all 2^31 take minutes in numpy: the issue's alternative);
    round B (15 nodes): all 2^15 certified masks and 10^6 random ones with uncertified nodes;
  * rank <-> (level, index) is a bijection, the kernel's nb_walk_src / nb_walk_dst (csrc/trx_kernel_nb.hip) are that map and its
    inverse, and the positions of the permuted lane constants ascend."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_nb_asm as G  # noqa: E402

INC = os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_nb_asm.inc")
ROUNDS = {"A": dict(levels=5, inc0=256, blk="DETA", lab="da", w=64), "B": dict(levels=4, inc0=8, blk="DETB", lab="db", w=32)}


# ---- the layout ---------------------------------------------------------------------------------------------------
def heap_of_rank(levels):
    """heap node n = 2^k - 1 + i at every in-order rank"""
    out = [None] * ((1 << levels) - 1)
    for k in range(levels):
        for i in range(1 << k):
            r = G.walk_rank(levels, k, i)
            assert out[r] is None
            out[r] = (1 << k) - 1 + i
    return out


def nb_walk_src(levels, l):
    """csrc/trx_kernel_nb.hip nb_walk_src<LEVELS>: the peak_const() lane whose constants lane l of the blocks takes"""
    r = l >> 1
    if r >= (1 << levels) - 1:
        return l
    t = ((r + 1) & -(r + 1)).bit_length() - 1
    k, i = levels - 1 - t, (r + 1) >> (t + 1)
    return 2 * ((1 << k) - 1 + i) + (l & 1)


def nb_walk_dst(levels, l):
    n = l >> 1
    if n >= (1 << levels) - 1:
        return l
    k = (n + 1).bit_length() - 1
    i = n + 1 - (1 << k)
    return 2 * (((2 * i + 1) << (levels - 1 - k)) - 1) + (l & 1)


def node_offset(n, inc0):
    """trx_device.h node_offset(): earlyIndex offset of heap node n of a bisection subtree whose first step is inc0"""
    lv = (n + 1).bit_length() - 1
    p = n + 1 - (1 << lv)
    return ((4 * p * inc0) >> lv) - (2 * inc0 - ((2 * inc0) >> lv))


@pytest.mark.parametrize("rnd", ["A", "B"])
def test_permutation(rnd):
    levels, inc0 = ROUNDS[rnd]["levels"], ROUNDS[rnd]["inc0"]
    nodes = (1 << levels) - 1
    h = heap_of_rank(levels)
    assert sorted(h) == list(range(nodes))                              # rank <-> (level, index): a bijection
    src = [nb_walk_src(levels, l) for l in range(64)]
    assert sorted(src) == list(range(64))
    for l in range(64):
        assert nb_walk_dst(levels, src[l]) == l
        if l < 2 * nodes:
            assert src[l] == 2 * h[l >> 1] + (l & 1)
        else:
            assert src[l] == l                                          # lanes without a node (and round B's final positions) stay
    # the permuted lane constants: early positions by rank ascend, by one leaf spacing; late = early + 2 symbols' halves (1024)
    early = [node_offset(src[2 * r] >> 1, inc0) for r in range(nodes)]
    step = inc0 >> (levels - 2)                                         # twice the last level's increment
    assert early == sorted(early) and set(np.diff(early)) == {step}
    # in-order: everything in a node's left subtree is left of it
    for k in range(levels - 1):
        for i in range(1 << k):
            r = G.walk_rank(levels, k, i)
            assert G.walk_rank(levels, k + 1, 2 * i) < r < G.walk_rank(levels, k + 1, 2 * i + 1)


# ---- the reference's walk, on heap-ordered decisions ------------------------------------------------------------------
def ref_walk(levels, right_h, sure_h):
    """peakDetect()'s path over heap-ordered node decisions (uint64 arrays, bit n = node n): (leaf, unsure) -- unsure when a node
    on the path has no certified decision (the walk of trx_device.h walk_tree / the blocks' former heap layout)"""
    p = np.zeros(right_h.shape, np.uint64)
    unsure = np.zeros(right_h.shape, bool)
    one = np.uint64(1)
    for k in range(levels):
        n = p + np.uint64((1 << k) - 1)
        unsure |= ((sure_h >> n) & one) == 0
        p = p * np.uint64(2) + ((right_h >> n) & one)
    return p.astype(np.int64), unsure


def to_heap(levels, x_r):
    """bit r of x_r (rank order) -> bit heap_of_rank[r]"""
    out = np.zeros(x_r.shape, np.uint64)
    for r, n in enumerate(heap_of_rank(levels)):
        out |= ((x_r >> np.uint64(r)) & np.uint64(1)) << np.uint64(n)
    return out


def spread(x, nodes):
    """bit r -> bit 2 r"""
    out = np.zeros(x.shape, np.uint64)
    for r in range(nodes):
        out |= ((x >> np.uint64(r)) & np.uint64(1)) << np.uint64(2 * r)
    return out


# ---- the kernel's two forms, as numpy ---------------------------------------------------------------------------------
def kernel_walk(levels, right_r, sure_r, junk):
    """The compare's mask from rank-ordered decisions (junk: what the lanes without a node leave in the bits above the round's),
    then the blocks' arithmetic: (leaf, unsure, took the first-zero form)"""
    nodes = (1 << levels) - 1
    nb = 2 * nodes
    low = np.uint64((1 << nb) - 1)
    c = spread(right_r & sure_r, nodes) | (spread(~right_r & sure_r, nodes) << np.uint64(1)) | (junk << np.uint64(nb))
    odd = np.uint64(sum(1 << (2 * r + 1) for r in range(nodes)))
    x = (c & low) ^ odd
    m = np.zeros(x.shape, np.int64)                                     # s_ff0: the first zero
    found = np.zeros(x.shape, bool)
    for b in range(nb + 1):
        z = ~found & (((x >> np.uint64(b)) & np.uint64(1)) == 0)
        m[z] = b
        found |= z
    assert found.all()
    fast = x == ((np.uint64(1) << m.astype(np.uint64)) - np.uint64(1))  # s_bfm, s_cmp_eq
    # the level-by-level walk: node (k, p) at bit (p << (levels + 1 - k)) + (1 << (levels - k)) - 2
    cd = c | (c >> np.uint64(1))
    p = np.zeros(x.shape, np.uint64)
    unsure = np.zeros(x.shape, bool)
    for k in range(levels):
        pos = (p << np.uint64(levels + 1 - k)) + np.uint64((1 << (levels - k)) - 2)
        unsure |= ((cd >> pos) & np.uint64(1)) == 0
        p = p * np.uint64(2) + ((c >> pos) & np.uint64(1))
    leaf = np.where(fast, m >> 1, p.astype(np.int64))
    assert (m[fast] & 1).sum() == 0
    return leaf, unsure & ~fast, fast


def check_round(levels, right_r, sure_r, seed=1):
    nodes = (1 << levels) - 1
    rng = np.random.default_rng(seed)
    junk = rng.integers(0, 4, size=right_r.shape, dtype=np.uint64)
    full = np.uint64((1 << nodes) - 1)
    right_r, sure_r = right_r & full, sure_r & full
    leaf, unsure, fast = kernel_walk(levels, right_r, sure_r, junk)
    ref_leaf, ref_unsure = ref_walk(levels, to_heap(levels, right_r & sure_r), to_heap(levels, sure_r))
    ones = np.zeros(right_r.shape, np.int64)
    for r in range(nodes):
        ones += ((right_r >> np.uint64(r)) & np.uint64(1)).astype(np.int64)
    monotone = right_r == ((np.uint64(1) << ones.astype(np.uint64)) - np.uint64(1))
    assert np.array_equal(fast, monotone & (sure_r == full))            # the first-zero form: exactly there
    assert np.array_equal(leaf[fast], ones[fast])
    assert np.array_equal(unsure, ref_unsure & ~fast) and not (ref_unsure & fast).any()
    ok = ~ref_unsure
    assert np.array_equal(leaf[ok], ref_leaf[ok])                       # both forms: the reference's leaf
    # where the first-zero arithmetic would differ from the walk, the fallback fires
    n0 = np.zeros(right_r.shape, np.int64)
    done = np.zeros(right_r.shape, bool)
    for r in range(nodes + 1):
        z = ~done & (((right_r >> np.uint64(r)) & np.uint64(1)) == 0)
        n0[z] = r
        done |= z
    differ = ok & (n0 != ref_leaf)
    assert not (differ & fast).any()
    return int(fast.sum()), int(differ.sum()), int(unsure.sum())


def near_monotone(nodes):
    out = []
    for n in range(nodes + 1):
        base = (1 << n) - 1
        out.append(base)
        for d in (1, 2):
            for bits in itertools.combinations(range(nodes), d):
                out.append(base ^ sum(1 << b for b in bits))
    return np.array(out, np.uint64)


def test_round_a():
    full = np.uint64((1 << 31) - 1)
    nm = near_monotone(31)
    assert len(nm) == 32 * (1 + 31 + 31 * 30 // 2)
    nm = np.unique(nm)                                                  # (a neighbour of one monotone mask can be another)
    fast, differ, _ = check_round(5, nm, np.full(nm.shape, full))
    assert fast == 32 and differ > 1000                                # (the set holds masks on which the two forms part)
    rng = np.random.default_rng(1701)
    r = rng.integers(0, 1 << 31, size=10**6, dtype=np.uint64)
    check_round(5, r, np.full(r.shape, full))
    # uncertified nodes: a few per mask, on monotone and on random decisions
    s = full & ~((np.uint64(1) << rng.integers(0, 31, size=10**6, dtype=np.uint64)) | (np.uint64(1) << rng.integers(0, 31, size=10**6, dtype=np.uint64)))
    mono = (np.uint64(1) << rng.integers(0, 32, size=10**6, dtype=np.uint64)) - np.uint64(1)
    _, _, unsure = check_round(5, mono, s)
    assert unsure > 1000
    check_round(5, r, s)
    check_round(5, nm, np.resize(s, nm.shape))


def test_round_b():
    full = np.uint64((1 << 15) - 1)
    allm = np.arange(1 << 15, dtype=np.uint64)
    fast, differ, _ = check_round(4, allm, np.full(allm.shape, full))
    assert fast == 16 and differ > 0
    rng = np.random.default_rng(1702)
    r = rng.integers(0, 1 << 15, size=10**6, dtype=np.uint64)
    s = rng.integers(0, 1 << 15, size=10**6, dtype=np.uint64) | rng.integers(0, 1 << 15, size=10**6, dtype=np.uint64)
    check_round(4, r, s)
    for sure in (0x7fff ^ 0x80, 0x7fff ^ 1, 0x7fff ^ 0x4000, 0):        # one uncertified node (the root: rank 7), none certified
        check_round(4, allm, np.full(allm.shape, np.uint64(sure)))


# ---- the generated instructions ---------------------------------------------------------------------------------------
def macro_lines(name):
    text = open(INC).read()
    m = re.search(r"#define NB_ASM_%s \\\n((?:\t\".*\\n\\t\"(?: \\)?\n)+)" % name, text)
    return [re.match(r'\t"(.*)\\n\\t"', t).group(1) for t in m.group(1).splitlines()]


def walk_program(rnd):
    """the scalar instructions behind the compare up to the block's `walked` label, and the cold code"""
    blk, lab = ROUNDS[rnd]["blk"], ROUNDS[rnd]["lab"]
    main = macro_lines(blk)
    i0 = max(i for i, t in enumerate(main) if t.startswith("v_cmp_lt_f32_e64 s[88:89]"))
    i1 = main.index(f".Lnb_{lab}_walked:")
    assert all(t.startswith("s_") for t in main[i0 + 1:i1]), main[i0 + 1:i1]
    # (constants the block sets ahead of the compare, in the wait states of its vector instructions)
    consts = [t for t in main[:i0] if re.match(r"s_mov_b32 s\d+, (0x[0-9a-f]+|\d+)$", t)]
    return consts + main[i0 + 1:i1] + [f"s_branch .Lnb_{lab}_walked"] + macro_lines("COLD")


class Salu:
    """the scalar instructions the walks use, on Python integers"""

    def __init__(self, prog):
        self.prog = prog
        self.labels = {t[:-1]: i for i, t in enumerate(prog) if t.endswith(":")}
        self.s = {}
        self.scc = 0

    def rd(self, tok, w=32):
        m = re.match(r"s\[(\d+):(\d+)\]$", tok)
        if m:
            return self.s.get(int(m.group(1)), 0) | (self.s.get(int(m.group(2)), 0) << 32)
        if tok.startswith("s"):
            return self.s.get(int(tok[1:]), 0)
        return int(tok, 0) & ((1 << w) - 1)

    def wr(self, tok, v):
        m = re.match(r"s\[(\d+):(\d+)\]$", tok)
        if m:
            self.s[int(m.group(1))], self.s[int(m.group(2))] = v & 0xffffffff, (v >> 32) & 0xffffffff
        else:
            self.s[int(tok[1:])] = v & 0xffffffff

    def run(self, stops):
        """-> the label of `stops` that was reached, and the labels jumped to on the way"""
        pc, taken, steps = 0, [], 0
        while True:
            steps += 1
            assert steps < 500
            t = self.prog[pc]
            pc += 1
            if t.endswith(":"):
                continue
            op, rest = t.split(None, 1)
            a = [x.strip() for x in rest.split(",")]
            w = 64 if op.endswith("64") else 32
            mask = (1 << w) - 1
            if op in ("s_branch", "s_cbranch_scc0", "s_cbranch_scc1"):
                if op == "s_branch" or self.scc == int(op[-1]):
                    taken.append(a[0])
                    if a[0] in stops:
                        return a[0], taken
                    pc = self.labels[a[0]]
            elif op == "s_bfe_u64":
                v, f = self.rd(a[1]), self.rd(a[2])
                self.wr(a[0], (v >> (f & 63)) & ((1 << ((f >> 16) & 127)) - 1))
            elif op in ("s_xor_b64", "s_xor_b32", "s_and_b32", "s_or_b64", "s_or_b32"):
                x, y = self.rd(a[1], w), self.rd(a[2], w)
                v = x ^ y if "xor" in op else x & y if "and" in op else x | y
                self.wr(a[0], v)
                self.scc = int(v != 0)
            elif op in ("s_ff0_i32_b64", "s_ff0_i32_b32"):
                v = self.rd(a[1])
                self.wr(a[0], next((b for b in range(w) if not (v >> b) & 1), 0xffffffff))
            elif op in ("s_bfm_b64", "s_bfm_b32"):
                n, o = self.rd(a[1]) & (w - 1), self.rd(a[2]) & (w - 1)
                self.wr(a[0], (((1 << n) - 1) << o) & mask)
            elif op in ("s_cmp_eq_u64", "s_cmp_eq_u32"):
                self.scc = int(self.rd(a[0], w) == self.rd(a[1], w))
            elif op in ("s_lshr_b64", "s_lshr_b32", "s_lshl_b32"):
                v, n = self.rd(a[1]), self.rd(a[2]) & (w - 1)
                v = (v >> n) if "lshr" in op else (v << n) & mask
                self.wr(a[0], v)
                self.scc = int(v != 0)
            elif op == "s_mov_b32":
                self.wr(a[0], self.rd(a[1]))
            elif op == "s_add_u32":
                v = self.rd(a[1]) + self.rd(a[2])
                self.wr(a[0], v)
                self.scc = v >> 32
            elif op == "s_addc_u32":
                v = self.rd(a[1]) + self.rd(a[2]) + self.scc
                self.wr(a[0], v)
                self.scc = v >> 32
            elif op in ("s_bitcmp0_b64", "s_bitcmp1_b64", "s_bitcmp0_b32", "s_bitcmp1_b32"):
                bit = (self.rd(a[0]) >> (self.rd(a[1]) & (w - 1))) & 1
                self.scc = int(bit == int(op[8]))
            else:
                raise AssertionError("instruction outside the walks' set: " + t)


@pytest.mark.parametrize("rnd", ["A", "B"])
def test_generated_instructions_follow_the_model(rnd):
    levels, lab = ROUNDS[rnd]["levels"], ROUNDS[rnd]["lab"]
    nodes = (1 << levels) - 1
    full = (1 << nodes) - 1
    prog = walk_program(rnd)
    m_reg = {"A": 95, "B": 94}[rnd]                                     # twice the leaf, at .Lnb_d?_walked
    rng = np.random.default_rng(1703)
    rights = [(1 << n) - 1 for n in range(nodes + 1)]
    rights += [b ^ (1 << k) for b in rights for k in range(nodes)]
    rights += [int(x) for x in rng.integers(0, 1 << nodes, size=1500)]
    sures = [full] * len(rights) + [full & ~(1 << int(k)) for k in rng.integers(0, nodes, size=len(rights))]
    rights = rights + rights
    leaf, unsure, fast = kernel_walk(levels, np.array(rights, np.uint64), np.array(sures, np.uint64), np.full(len(rights), 3, np.uint64))
    ref_leaf, ref_unsure = ref_walk(levels, to_heap(levels, np.array(rights, np.uint64) & np.array(sures, np.uint64)), to_heap(levels, np.array(sures, np.uint64)))
    n_cold = 0
    for j, (r, s) in enumerate(zip(rights, sures)):
        c = sum(((1 << (2 * q)) if (r >> q) & 1 else (2 << (2 * q))) for q in range(nodes) if (s >> q) & 1) | (3 << (2 * nodes))
        if rnd == "B":
            c |= 0xdeadbeef << 32                                       # lanes 32 .. 63: the final positions' compare bits, never read
        cpu = Salu(prog)
        cpu.s[88], cpu.s[89] = c & 0xffffffff, (c >> 32) & 0xffffffff
        end, taken = cpu.run((f".Lnb_{lab}_walked", f".Lnb_{lab}_end"))
        cold = f".Lnbc_{lab}_careful" in taken
        n_cold += cold
        assert cold == (not fast[j]), (hex(r), hex(s))
        if end.endswith("_end"):
            assert cpu.s[98] == 3 and unsure[j] and ref_unsure[j], (hex(r), hex(s))
        else:
            assert cpu.s[98] == 1 and not unsure[j] and not ref_unsure[j], (hex(r), hex(s))
            assert cpu.s[m_reg] == 2 * leaf[j] == 2 * ref_leaf[j], (hex(r), hex(s), cpu.s[m_reg], leaf[j])
    assert n_cold > 1000
