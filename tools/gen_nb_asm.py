#!/usr/bin/env python3
"""Generator of the hand-placed instruction blocks of the normal-burst kernel (osmo_trx_amd/csrc/trx_kernel_nb.hip).

    python tools/gen_nb_asm.py [OUT]      # writes osmo_trx_amd/csrc/trx_nb_asm.inc (committed), or OUT

Why generated: hipcc treats an `asm` statement as one opaque instruction -- it pads neither the hazards nor the memory
waits of what is inside, and it pads every boundary between two dependent asm statements with an s_nop of its own.  The
blocks below are therefore whole phases of a burst, and this script CHECKS what hipcc does not, on the sequence it emits:
  * wait states (gfx950 rules as the compiler's own code shows them): packed-fp32 result -> VALU reader 1; VALU-written
    VGPR -> DPP source 2; VALU-written SGPR / VCC -> VALU reader 2; transcendental result -> VALU reader 1; VALU-written
    VGPR -> v_readlane 1; VALU-written SGPR -> v_readlane lane select 4, -> VMEM address 5; x3 / x4 store data 2;
  * every register loaded from LDS is covered by an s_waitcnt lgkmcnt(n) before its first use (LDS returns in order);
  * a DPP source lane that EXEC disables is invalid: the mask of a wave_shr:1 instruction is a run of lanes from lane 0.
Registers: operands the compiler allocates are %[name]; the blocks' temporaries are the fixed VGPRs v64..v127 and SGPRs
s87..s99, declared as clobbers of every statement (NB_ASM_CLOBBERS).
Jumps: the burst loop's main path FALLS THROUGH every block -- no jump over cold code.  A block's rare side lies either in
the shadow of a taken jump the main path cannot avoid (DEC and CORR are one statement: the wide and the multiplying forms sit
between CORR's computed jump and its first variant), or in NB_ASM_COLD, one statement behind the loop that names fixed
registers only (DETA's gate exit and careful walk, DETB's careful walk, TAIL's geometry exit), which is why the detection status
has a fixed register (NB_ASM_ST).  Cold labels carry the prefix .Lnbc_; where they may lie is checked here, and on the compiled
kernel by tools/isa_guard_nb.py."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "osmo_trx_amd", "csrc", "trx_nb_asm.inc")

PH_A, PH_M0 = 180, 12
# %[aw]: the one per-lane LDS address the blocks DEC, CORR and TAIL take -- the wave's slice base + 8 * lane, computed once in
# front of the burst loop (trx_kernel_nb.hip: a_w).  What the blocks address is a compile-time byte offset of it in the ds_*
# offset field (16 bits; a slice is 7.7 KB): the kernel static_asserts these against its LDS carve.
NB_D_LEN, CZ_PAD = 160, 12
AW_PD = (PH_M0 + 52) * 8                         # P + PH_M0 + (56 + lane) - 4
AW_D = 4 * PH_A * 8                              # D[lane]
AW_CZ = (4 * PH_A + NB_D_LEN + CZ_PAD) * 8       # cz[lane]
TRANS = ("v_rcp_", "v_sqrt_", "v_log_", "v_exp_", "v_rsq_", "v_sin_", "v_cos_")
NEG_MASKS = [0x447b, 0xc5bb, 0x7488, 0x7709, 0xa75c, 0xf60d, 0x4eb9, 0xdc21]   # TRX_UNIT_NEG_TSC0..7 (trx_device.h)


def regs_of(tok):
    """set of register names an operand token touches: v5, v[4:7], s3, s[2:3], vcc, exec, %[x] (symbolic, one unit)"""
    tok = tok.strip()
    tok = re.sub(r"^-", "", tok)
    tok = re.sub(r"^\|(.*)\|$", r"\1", tok)
    tok = re.sub(r"^abs\((.*)\)$", r"\1", tok)
    m = re.match(r"^([vs])\[(\d+):(\d+)\]$", tok)
    if m:
        return {f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    if re.match(r"^[vs]\d+$", tok):
        return {tok}
    if tok in ("vcc", "exec"):
        return {tok}
    if tok.startswith("%["):
        return {tok}
    return set()


class Block:
    def __init__(self, name, sgpr_ops=()):
        self.name = name
        self.ins = []
        self.sgpr_ops = {f"%[{n}]" for n in sgpr_ops}      # operands the compiler allocates in SGPRs (the rest are VGPRs)

    def raw(self, text):
        self.ins.append(text)

    def __call__(self, text):
        self.ins.append(text)

    def label(self, l):
        self.ins.append(l + ":")

    # ---- checks -------------------------------------------------------------------------------------------------
    @staticmethod
    def parse(text):
        t = text.split("//")[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            return None
        parts = t.split(None, 1)
        op = parts[0]
        ops = []
        if len(parts) > 1:
            rest = parts[1]
            # operands are separated by commas outside brackets; modifiers (op_sel:.., quad_perm:.., offset:..) follow by spaces
            depth = 0
            cur = ""
            for ch in rest:
                if ch == "[":
                    depth += 1
                if ch == "]":
                    depth -= 1
                if ch == "," and depth == 0:
                    ops.append(cur.strip())
                    cur = ""
                else:
                    cur += ch
            ops.append(cur.strip())
            # strip trailing modifiers from the last operand
            last = ops[-1].split()
            mods = " ".join(last[1:]) if len(last) > 1 else ""
            ops[-1] = last[0] if last else ""
        else:
            mods = ""
        return op, ops, mods

    def check(self):
        """linear hazard / waitcnt check of the emitted sequence (branches: the fall-through order is checked; code after a
        label is checked with the state that reaches it in program order, which is the worst case for the blocks here)"""
        last_w = {}            # reg -> (index in wait states, kind of writer)
        exec_tok = "full"      # symbolic value of EXEC: "full" or the text of the instruction that narrowed it
        w_exec = {}            # VGPR -> EXEC token it was last written under
        pos = 0                # position in wait states
        lds_q = []             # outstanding LDS ops in order: set of dst regs (empty set for writes)
        pending = {}           # reg -> True while its LDS load is outstanding
        errs = []
        for text in self.ins:
            p = self.parse(text)
            if p is None:
                continue
            op, ops, mods = p
            if op == "s_nop":
                pos += int(ops[0]) + 1
                continue
            if op == "s_waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", text)
                if m:
                    n = int(m.group(1))
                    while len(lds_q) > n:
                        for r in lds_q.pop(0):
                            pending.pop(r, None)
                pos += 1
                continue
            is_valu = op.startswith("v_")
            is_dpp = "_dpp" in op or "quad_perm" in mods or "row_" in mods or "wave_" in mods
            is_pk = op.startswith("v_pk_")
            is_trans = op.startswith(TRANS)
            is_lds = op.startswith("ds_")
            is_vmem = op.startswith(("global_", "buffer_", "flat_"))
            is_cmp = op.startswith("v_cmp")
            is_readlane = op.startswith(("v_readlane", "v_readfirstlane"))
            is_store = is_vmem and "store" in op
            # destination / sources
            if is_lds and ("write" in op or op.startswith("ds_add_u32") and "rtn" not in op):
                dsts, srcs = [], ops
            elif is_store:
                dsts, srcs = [], ops
            elif op.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_setpc", "s_endpgm", "s_barrier", "s_sleep")):
                dsts, srcs = [], ops
            else:
                dsts, srcs = ops[:1], ops[1:]
            if is_cmp and op.endswith("_e32"):
                dsts, srcs = ["vcc"], ops[1:]
            if op.startswith(("v_cndmask_b32_e32", "v_addc", "v_subb")) or (op.startswith("v_cndmask_b32") and len(ops) == 3):
                srcs = srcs + ["vcc"]
            if op in ("v_fmac_f32_e32", "v_fmac_f32_dpp", "v_pk_fma_f32") or op.startswith(("v_fmac", "v_mac")) or \
               op.startswith("v_writelane"):
                srcs = srcs + dsts                                   # read-modify-write
            if op.startswith("v_max3") or "_dpp" in op:
                srcs = srcs + []                                     # (dst listed again in the operands when it is also a source)
            rd = set()
            for s in srcs:
                rd |= regs_of(s)
            wr = set()
            for d in dsts:
                wr |= regs_of(d)
            # ---- EXEC: a value written under a narrowed mask is only defined in that mask's lanes
            if (is_valu or is_lds or is_vmem) and not is_readlane:
                for r in rd:
                    if r in w_exec and w_exec[r] != "full" and w_exec[r] != exec_tok and r not in getattr(self, "exec_ok", ()):
                        errs.append(f"{self.name}: `{text.strip()}` under EXEC {exec_tok!r} reads {r}, written under {w_exec[r]!r}")
            # ---- a DPP source lane that EXEC disables is invalid (the write is dropped, or reads 0 with bound_ctrl): under wave_shr:1
            # lane l reads lane l - 1, so the mask must be full or a run of lanes that starts at lane 0
            if is_dpp and "wave_shr:1" in mods and exec_tok != "full" and not re.match(r"^(s_bfm_b64 exec, \S+, 0|s_lshr_b64 exec, -1, \S+)$", exec_tok):
                errs.append(f"{self.name}: `{text.strip()}` under EXEC {exec_tok!r}: the mask does not cover every DPP source lane")
            # ---- LDS data must have arrived
            for r in rd:
                if r in pending:
                    errs.append(f"{self.name}: `{text.strip()}` reads {r} before its LDS load is waited for")
            # ---- wait states
            for k, s in enumerate(srcs):
                for r in regs_of(s):
                    if r not in last_w:
                        continue
                    r_is_s = (r.startswith("s") and not r.startswith("%")) or r == "vcc" or r in self.sgpr_ops
                    wpos, wkind = last_w[r]
                    gap = pos - wpos - 1
                    need = 0
                    if is_valu and wkind["pk"]:
                        need = max(need, 1)
                    if is_valu and wkind["trans"]:
                        need = max(need, 1)
                    if is_dpp and k == 0 and wkind["valu"] and not r_is_s:
                        need = max(need, 2)
                    if is_valu and wkind["valu"] and r_is_s:
                        need = max(need, 2)
                    if is_readlane and k == 0 and wkind["valu"]:
                        need = max(need, 1)
                    if is_readlane and k == 1 and wkind["valu"]:
                        need = max(need, 4)
                    if is_vmem and wkind["valu"] and r_is_s:
                        need = max(need, 5)
                    if gap < need:
                        errs.append(f"{self.name}: `{text.strip()}` reads {r} {gap} wait state(s) after its writer, needs {need}")
            if is_store and ("dwordx3" in op or "dwordx4" in op):
                self._wide_store = (pos, rd)
            kind = {"pk": is_pk, "trans": is_trans, "valu": is_valu}
            for r in wr:
                last_w[r] = (pos, kind)
                if r.startswith(("v", "%")) and r not in self.sgpr_ops:
                    # a full overwrite under the full mask defines every lane; a write under a narrowed mask leaves the other
                    # lanes as they were: defined only if they were defined before (tracked as the narrower of the two)
                    if exec_tok == "full" or w_exec.get(r) != "full":
                        w_exec[r] = exec_tok
            if "exec" in wr or any(d.strip().startswith("exec") for d in dsts):
                exec_tok = "full" if re.search(r"exec(_lo|_hi)?, -1$", text.strip()) and "exec_" not in text else text.strip()
            if is_lds:
                is_load = "read" in op or "rtn" in op
                lds_q.append(set(wr) if is_load else set())
                if is_load:
                    for r in wr:
                        pending[r] = True
            pos += 1
        if pending:
            errs.append(f"{self.name}: LDS loads still outstanding at the end of the block: {sorted(pending)[:6]}")
        return errs

    def text(self):
        lines = []
        for t in self.ins:
            lines.append(t)
        return lines


def vreg(i, n=1):
    return f"v{i}" if n == 1 else f"v[{i}:{i + n - 1}]"


def sreg(i, n=1):
    return f"s{i}" if n == 1 else f"s[{i}:{i + n - 1}]"


# ------------------------------------------------------------------------------------------------------------------
# block DEC: the /4 decimator of the detection window (downsampleBurst restricted to what the correlation and computeCI
# read, sigProcLib.cpp:1587-1601) + the addition-only correlation's guard (unit_unsafe, trx_device.h).
#   %[aw]   VGPR  slice base + 8 * lane: P + PH_M0 + (56 + lane) - 4 (polyphase burst, trx_k4_common.h) is offset AW_PD of it,
#                 D[lane] offset AW_D, D[lane - 4] offset AW_D - 32 (ds_write2_b32's offsets have 8 bits: that one address is formed
#                 in a wait state of the sum's last adds)
#   %[zero] VGPR  0 (address of the wave-uniform tap reads)
#   %[len]  SGPR  window length; 15 + len decimated samples (NACT, a fixed register)
#   out: VCC lanes whose decimated sample fails the guard; DRI (fixed registers) the decimated sample, re / im (lane l + 4:
#        sample l; moving form only)
# y = sum_k x[4i-15+k] * g[k], product then sum, k ascending, first sum = first product (decimate16_sym<true>); taps 0..7
# only (bitwise symmetric filter).  Tap k of output l is polyphase entry P[(k+1)&3][m0 + l + ((k+1)>>2)]: for one phase the
# entry output l takes at row offset j+1 is the one output l+1 takes at offset j.
#   * windows of up to 60 samples (max_toa <= 29): every lane loads ITS OWN four entries X_r = P[r][m0 + lane] and forms all
#     sixteen products with them; the accumulator of output l starts in lane l and MOVES one lane up (wave_shr:1 on the
#     accumulator operand of the add) whenever the next tap's sample lives one row further -- in front of taps 3, 7, 11, 15.
#     The same products, summed in the same order; output l ends in lane l + 4.  4 sample reads instead of 16.
#   * wider windows (15 + len + 4 > 64 lanes): lane = output, sixteen reads per lane (cold: .Lnbc_dc_wide).
# ------------------------------------------------------------------------------------------------------------------
DEC_SHIFT = 4                    # lanes the moving accumulator travels
NACT = "s92"                     # 15 + len, decimated samples: made at the head of the statement (DEC and CORR are ONE statement)
DRI = ("v110", "v111")           # the decimated sample of lane - 4, re / im: from DEC's moving form to CORR's
DEC_MAX_NACT = 64 - DEC_SHIFT    # widest window of the moving form
DPP_SHR = "wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"


def dec_guard(b, re, im, t0, t1):
    b(f"v_min_f32_e64 {t0}, |{re}|, |{im}|")
    b(f"v_max_f32_e64 {t1}, |{re}|, |{im}|")
    b(f"v_ldexp_f32 {t0}, {t0}, 17")
    b(f"v_cmp_lt_f32_e32 vcc, {t0}, {t1}")                          # VCC: lanes whose decimated sample fails the guard
    b("s_mov_b64 exec, -1")
    b("s_waitcnt lgkmcnt(0)")          # (the store: nothing of this block may be outstanding for the checker; costs nothing behind the guard)


def dec_tap(kk):
    base = (124 if (kk >> 2) else 120) + (2 if (kk & 2) else 0)
    sel = "op_sel:[0,1] op_sel_hi:[1,1]" if (kk & 1) else "op_sel:[0,0] op_sel_hi:[1,0]"
    return f"{vreg(base, 2)} {sel}"


def dec_moving(gdec_off):
    b = Block("DEC", ("len",))
    PR = lambda k: 64 + 2 * k                  # product of tap k: v[64+2k : 65+2k]
    XR = lambda r: vreg(96 + 2 * r, 2)         # this lane's entry of phase r
    ACC = 104
    b(f"s_sub_u32 s88, {DEC_MAX_NACT}, {NACT}")
    b("s_lshr_b64 exec, -1, s88")             # lanes 0 .. nact + 3 (all 64 at the widest window, which s_bfm_b64 cannot express):
                                              # every lane an accumulator passes through (a DPP source lane must be enabled)
    b(f"ds_read_b128 {vreg(120, 4)}, %[zero] offset:{gdec_off}")
    b(f"ds_read_b128 {vreg(124, 4)}, %[zero] offset:{gdec_off + 16}")
    for r in (1, 2, 3, 0):
        b(f"ds_read_b64 {XR(r)}, %[aw] offset:{AW_PD + r * PH_A * 8}")

    def mul(k):
        b(f"v_pk_mul_f32 {vreg(PR(k), 2)}, {XR((k + 1) & 3)}, {dec_tap(k if k < 8 else 15 - k)}")

    def add(k):
        src0 = vreg(PR(0), 2) if k == 1 else vreg(ACC, 2)
        b(f"v_pk_add_f32 {vreg(ACC, 2)}, {src0}, {vreg(PR(k), 2)}")

    def add_moving(k, dst=(f"v{ACC}", f"v{ACC + 1}")):
        for c in range(2):
            b(f"v_add_f32_dpp {dst[c]}, v{ACC + c}, v{PR(k) + c} {DPP_SHR}")

    b("s_waitcnt lgkmcnt(3)")
    mul(0)
    b("s_waitcnt lgkmcnt(2)")
    mul(1)
    b("s_waitcnt lgkmcnt(1)")
    mul(2); add(1)
    b("s_waitcnt lgkmcnt(0)")
    mul(3); add(2); mul(4); mul(5); add_moving(3)
    mul(6); add(4); mul(7); add(5); mul(8); add(6); mul(9); mul(10); add_moving(7)
    mul(11); add(8); mul(12); add(9); mul(13); add(10); mul(14); mul(15); add_moving(11)
    add(12)
    b("s_nop 0")
    add(13)
    b("s_nop 0")
    add(14)
    b(f"v_add_u32_e32 v108, {AW_D - 8 * DEC_SHIFT}, %[aw]")        # &D[lane - 4] (one of the two wait states in front of the DPP source)
    b("s_nop 0")
    out = DRI
    add_moving(15, out)
    b(f"s_bfm_b64 exec, {NACT}, {DEC_SHIFT}")                      # output l sits in lane l + 4
    b(f"ds_write2_b32 v108, {out[0]}, {out[1]} offset1:1")         # D[] stays: computeCI's samples (TAIL), the multiplying correlation
    dec_guard(b, out[0], out[1], "v106", "v107")
    b.exec_ok = {f"v{ACC}", f"v{ACC + 1}", out[0], out[1], "v108"}       # (lanes 4 .. nact + 3 are inside the mask they were written under)
    return b


def dec_wide(gdec_off):
    b = Block("DEC_WIDE", ("len",))
    X = lambda k: vreg(88 + 2 * k, 2)
    b(f"s_bfm_b64 exec, {NACT}, 0")
    b(f"ds_read_b128 {vreg(120, 4)}, %[zero] offset:{gdec_off}")
    b(f"ds_read_b128 {vreg(124, 4)}, %[zero] offset:{gdec_off + 16}")
    for k in range(16):
        off = (((k + 1) & 3) * PH_A + ((k + 1) >> 2)) * 8
        b(f"ds_read_b64 {X(k)}, %[aw] offset:{AW_PD + off}")

    def mul(k):
        b(f"v_pk_mul_f32 {X(k)}, {X(k)}, {dec_tap(k if k < 8 else 15 - k)}")

    def add(k):            # y (in X(0)) += product k
        b(f"v_pk_add_f32 {X(0)}, {X(0)}, {X(k)}")

    b("s_waitcnt lgkmcnt(12)")
    mul(0); mul(1); mul(2); add(1); mul(3); add(2)
    b("s_waitcnt lgkmcnt(8)")
    mul(4); add(3); mul(5); add(4); mul(6); add(5); mul(7); add(6)
    b("s_waitcnt lgkmcnt(4)")
    mul(8); add(7); mul(9); add(8); mul(10); add(9); mul(11); add(10)
    b("s_waitcnt lgkmcnt(0)")
    mul(12); add(11); mul(13); add(12); mul(14); add(13); mul(15); add(14)
    b("s_nop 0")
    add(15)
    b(f"ds_write_b64 %[aw], {X(0)} offset:{AW_D}")
    dec_guard(b, "v88", "v89", "v90", "v91")
    return b


# ------------------------------------------------------------------------------------------------------------------
# block CORR: correlation of the window against the slot's training sequence without multiplications (corr_unit,
# trx_device.h: every tap is +-1 rotated by k pi/2 under the guard); arg-max input.
#   %[aw]  VGPR  slice base + 8 * lane: D[lane] is offset AW_D of it, cz[lane] offset AW_CZ; the moving form's D[lane - 19] and
#                cz[lane - 19] are 152 bytes below those
#   %[len] SGPR  window length                    %[tsc] SGPR  training sequence 0..7
#   %[nrm] VGPR out: |corr|^2 (0 for lanes that hold no lag)
#   DRI (fixed registers) the decimated sample of lane - 4 (block DEC, moving form)
# DEC and CORR are ONE statement (NB_ASM_DECCORR): the main path -- the moving forms, a guard that holds -- falls through DEC, tests
# the window's width and the guard once each, and leaves CORR by two taken jumps, the computed one into a variant and the variant's
# own to the end (every variant carries the short tail: the stores of cz[], |corr|^2; the last one falls through).  The rare forms
# lie in the computed jump's shadow, between it and the first variant.
# The sum is one chain by definition (the reference's order: k ascending from +0, convolve_base.c:28-54).  Eight variants
# (the sign / component pattern of a training sequence), entered by a computed jump.
#   * wide windows (more than 45 lags): lane = lag; D[lag + k] from LDS, one v_pk_add_f32 per tap (sign / swap are
#     instruction modifiers); a dependent v_pk_add_f32 needs a wait state: the waits for the next sample ARE those.
#   * windows of up to 45 lags: decimated sample i sits in lane i + 4 (block DEC), and the accumulator moves:
#     acc[l] = acc[l - 1] +- d_c[l] (wave_shr:1 on the accumulator, re and im chains interleaved: a VALU-written DPP source
#     needs two wait states, the other chain's add is one of them).  After tap k lane l holds sum_{k' <= k} s_k' d[l - 4 - k + k']:
#     lag lam ends in lane lam + 19.  No LDS read.  Lanes below 19 hold partial sums: |corr|^2 = 0 there.
# ------------------------------------------------------------------------------------------------------------------
CORR_LANE0 = DEC_SHIFT + 15      # lane of lag 0 in the moving form
CORR_MAX_LEN = 64 - CORR_LANE0


def corr_jump(b, sfx, pfx=".Lnb_corr"):
    b("s_getpc_b64 s[88:89]")
    b(f"{pfx}{sfx}_pc:")
    b(f"s_mul_i32 s90, %[tsc], {pfx}{sfx}_v1-{pfx}{sfx}_v0")
    b("s_add_u32 s88, s88, s90")
    b("s_addc_u32 s89, s89, 0")
    b(f"s_add_u32 s88, s88, {pfx}{sfx}_v0-{pfx}{sfx}_pc")
    b("s_addc_u32 s89, s89, 0")
    b("s_setpc_b64 s[88:89]")


def corr_mul(b, sfx, lseq_off, X, ACC, join=True):
    """cold (about one burst in 3000): convolve_complex() as written (convolve_base.c:28-40, :72-85), taps from LDS:
    (yr, yi) += (xr hr - xi hi, xr hi + xi hr) as two packed multiplies, one packed add with the low half negated, one accumulate"""
    b("s_lshl_b32 s90, %[tsc], 7")
    b("v_mov_b32_e32 v64, s90")
    H = lambda k: vreg(66 + 2 * (k & 7), 2)
    for half in range(2):
        for q in range(4):
            b(f"ds_read_b128 {vreg(66 + 4 * q, 4)}, v64 offset:{lseq_off + 64 * half + 16 * q}")
        b("s_waitcnt lgkmcnt(0)")
        for k in range(8 * half, 8 * half + 8):
            b(f"v_pk_mul_f32 v[82:83], {X(k)}, {H(k)} op_sel:[0,0] op_sel_hi:[0,1]")
            b(f"v_pk_mul_f32 v[84:85], {X(k)}, {H(k)} op_sel:[1,1] op_sel_hi:[1,0]")
            b("s_nop 0")
            b("v_pk_add_f32 v[86:87], v[82:83], v[84:85] neg_lo:[0,1] neg_hi:[0,0]")
            b("s_nop 0")
            b(f"v_pk_add_f32 {ACC}, {ACC}, v[86:87]")
    if join:
        b(f"s_branch .Lnbc_corr{sfx}_join")


def corr_lanes(lseq_off, sfx):
    """lane = lag, samples from D[] -> (head, [variant t], join, mul): lists of lines"""
    X = lambda k: vreg(88 + 2 * k, 2)
    ACC = vreg(120, 2)
    h = Block("h")
    h(f"v_mov_b64_e32 {ACC}, 0")
    h("s_bfm_b64 exec, %[len], 0")
    for k in range(16):
        h(f"ds_read_b64 {X(k)}, %[aw] offset:{AW_D + 8 * k}")
    h(f"s_cbranch_vccnz .Lnbc_corr{sfx}_mul")                      # a sample failed the guard (VCC: block DEC): the multiplying form
    corr_jump(h, sfx, ".Lnbc_corr")
    vs = []
    for t in range(8):
        v = Block("v")
        v(f".Lnbc_corr{sfx}_v{t}:")
        for k in range(16):
            odd, neg = (k & 1), (NEG_MASKS[t] >> k) & 1
            if not odd and not neg:
                mod = ""
            elif not odd and neg:
                mod = " neg_lo:[0,1] neg_hi:[0,1]"
            elif odd and not neg:
                mod = " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,0]"
            else:
                mod = " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,1]"
            v(f"s_waitcnt lgkmcnt({15 - k})")
            v(f"v_pk_add_f32 {ACC}, {ACC}, {X(k)}{mod}")
        v(f"s_branch .Lnbc_corr{sfx}_join")
        vs.append(v.ins)
    j = Block("j")
    j(f".Lnbc_corr{sfx}_join:")
    j("s_add_u32 s90, %[len], 12")
    j("s_bfm_b64 exec, s90, 0")
    j(f"ds_write_b64 %[aw], {ACC} offset:{AW_CZ}")
    j("s_mov_b64 exec, -1")                         # (lanes >= len hold the 0 they were initialised with: |corr|^2 = 0 there)
    j(f"v_pk_mul_f32 v[122:123], {ACC}, {ACC}")
    j("s_waitcnt lgkmcnt(0)")
    j("v_add_f32_e32 %[nrm], v123, v122")
    m = Block("m")
    m(f".Lnbc_corr{sfx}_mul:")
    corr_mul(m, sfx, lseq_off, X, ACC)
    return h.ins, vs, j.ins, m.ins


def corr_moving(lseq_off):
    """lane = lag + 19, samples from block DEC's registers -> (head, [variant t], tail, mul): lists of lines.  The tail (the
    stores of cz[], |corr|^2) closes EVERY variant: a variant leaves for the block's end itself, the last one by falling through"""
    sfx = "r"
    X = lambda k: vreg(88 + 2 * k, 2)
    ACC = vreg(120, 2)
    D = DRI
    h = Block("h")
    h(f"v_mov_b64_e32 {ACC}, 0")
    h("v_mov_b64_e32 v[122:123], 0")
    h("v_mov_b32_e32 %[nrm], 0")
    h("s_lshl_b32 s90, %[len], 3")
    h(f"s_sub_u32 s91, {CORR_MAX_LEN}, %[len]")
    h("v_add_u32_e32 v64, s90, %[aw]")                              # &cz[len + lane]: the right zero pad, stored by lanes 0..11
    h("s_lshr_b64 exec, -1, s91")                                  # lanes 0 .. len + 18: every lane that holds a sample or passes an accumulator on
    j = Block("j")
    j("s_bfm_b64 exec, 12, 0")
    j(f"ds_write_b64 v64, v[122:123] offset:{AW_CZ}")
    j(f"s_bfm_b64 exec, %[len], {CORR_LANE0}")
    j(f"ds_write_b64 %[aw], {ACC} offset:{AW_CZ - 8 * CORR_LANE0}")
    j(f"v_pk_mul_f32 v[124:125], {ACC}, {ACC}")
    j("s_nop 0")
    j("v_add_f32_e32 %[nrm], v125, v124")
    j("s_mov_b64 exec, -1")
    j("s_waitcnt lgkmcnt(0)")
    vs = []
    for t in range(8):
        v = Block("v")
        v(f".Lnb_corr{sfx}_v{t}:")
        for k in range(16):
            odd, neg = (k & 1), (NEG_MASKS[t] >> k) & 1
            # tap k = (+-1) (j)^k... as the packed form has it: even: (re, im) +- (d.re, d.im); odd: (re -+ d.im, im +- d.re)
            if not odd:
                ops = [("sub" if neg else "add", D[0]), ("sub" if neg else "add", D[1])]
            else:
                ops = [("add" if neg else "sub", D[1]), ("sub" if neg else "add", D[0])]
            for c in range(2):
                if k == 0:
                    v(f"v_{ops[c][0]}_f32_e32 v{120 + c}, 0, {ops[c][1]}")
                else:
                    v(f"v_{ops[c][0]}_f32_dpp v{120 + c}, v{120 + c}, {ops[c][1]} {DPP_SHR}")
            if k < 15:
                v("s_nop 0")
        v.ins += j.ins
        if t < 7:
            v("s_branch .Lnb_corr_end")
        vs.append(v.ins)
    m = Block("m")
    m(f"s_bfm_b64 exec, %[len], {CORR_LANE0}")
    for k in range(16):
        m(f"ds_read_b64 {X(k)}, %[aw] offset:{AW_D - 8 * CORR_LANE0 + 8 * k}")
    corr_mul(m, sfx, lseq_off, X, ACC, join=False)
    return h.ins, vs, j.ins, m.ins


def block_deccorr(gdec_off, lseq_off):
    """-> (block, [straight-line paths to check])"""
    ops = ("len", "tsc")
    pre = [f"s_add_u32 {NACT}, %[len], 15", f"s_cmp_gt_u32 %[len], {CORR_MAX_LEN}", "s_cbranch_scc1 .Lnbc_dc_wide"]
    mv, wd = dec_moving(gdec_off), dec_wide(gdec_off)
    h, vs, j, m = corr_moving(lseq_off)
    wh, wvs, wj, wm = corr_lanes(lseq_off, "w")
    hj = Block("hj")
    corr_jump(hj, "r")
    b = Block("DECCORR", ops)
    b.ins = pre + mv.ins + ["s_cbranch_vccnz .Lnbc_dc_mul"] + h + hj.ins
    # ---- in the computed jump's shadow: the wide window's forms; the moving form's multiplying variant
    b.ins += [".Lnbc_dc_wide:"] + wd.ins + wh
    for v in wvs:
        b.ins += v
    b.ins += wj + ["s_branch .Lnb_corr_end"] + wm
    b.ins += [".Lnbc_dc_mul:"] + h + m + j + ["s_branch .Lnb_corr_end"]
    for v in vs:
        b.ins += v
    b.ins += [".Lnb_corr_end:"]
    paths = []
    for t, v in enumerate(vs):
        p = Block(f"DECCORR[moving, tsc {t}]", ops)
        p.ins = pre + mv.ins + h + hj.ins + v
        paths.append(p)
    p = Block("DECCORR[moving, mul]", ops)
    p.ins = pre + mv.ins + h + m + j
    paths.append(p)
    ibr = next(i for i, t in enumerate(wh) if t.startswith("s_cbranch_vccnz"))
    for t, v in enumerate(wvs):
        p = Block(f"DECCORR[lanes, tsc {t}]", ops)
        p.ins = pre + wd.ins + wh + v + wj
        paths.append(p)
    p = Block("DECCORR[lanes, mul]", ops)
    p.ins = pre + wd.ins + wh[:ibr] + wm + wj
    paths.append(p)
    for p in paths:
        # (the lanes read are inside the mask they were written under: DEC's outputs in lanes 4 .. nact + 3, the accumulators)
        p.exec_ok = set(mv.exec_ok) | {"v120", "v121"}
    return b, paths


def check_paths(b):
    """blocks with forward branches: the fall-through order and, for every label, the order that starts at the block's head and
    continues at the label from each branch to it (state at the branch)"""
    errs = b.check()
    lines = b.ins
    for i, t in enumerate(lines):
        m = re.match(r"^s_cbranch_\w+ (\S+)$|^s_branch (\S+)$", t.strip())
        if not m:
            continue
        lab = (m.group(1) or m.group(2)) + ":"
        if lab not in lines:
            continue
        j = lines.index(lab)
        if j < i:
            continue                                                # (a backward branch: the join re-enters checked code)
        v = Block(f"{b.name}[{t.strip()}]", [n[2:-1] for n in b.sgpr_ops])
        v.ins = lines[:i] + lines[j:]
        v.exec_ok = getattr(b, "exec_ok", ())
        for e in v.check():
            if e.split(": ", 1)[1] not in [x.split(": ", 1)[1] for x in errs]:
                errs.append(e)
    return errs


# ------------------------------------------------------------------------------------------------------------------
# block AMAX: wave maximum of |corr|^2 (fastPeakDetect, :1120-1139) and the energyDetect sum (:1573-1585: the lanes = 0
# mod 4 hold the partial sums), two DPP chains interleaved with each other and with the lane-constant / header loads the
# following phases need -- a DPP source written by the instruction in front needs two wait states, and every one of them
# here is an instruction that had to be issued anyway.
#   %[nrm] VGPR |corr|^2   %[ep] VGPR energy partial sums
#   %[m] SGPR out: max     %[es] SGPR out: energy sum      %[bidx] SGPR out: first lane holding the maximum (-1: none)
#   fillers: eight independent single instructions handed in by the caller (strings)
# ------------------------------------------------------------------------------------------------------------------
def block_amax(fill):
    assert len(fill) == 8
    b = Block("AMAX", ("m", "es", "bidx"))
    D = "row_mask:0xf bank_mask:0xf"
    b("v_mov_b32_e32 v88, %[nrm]")
    b(f"v_mov_b32_dpp v89, %[ep] quad_perm:[0,0,0,0] {D}")
    b(fill[0])
    b(f"v_max_f32_dpp v88, v88, v88 quad_perm:[1,0,3,2] {D}")
    b(f"v_add_f32_dpp v89, v89, v89 row_half_mirror {D}")
    b(fill[1])
    b(f"v_max_f32_dpp v88, v88, v88 quad_perm:[2,3,0,1] {D}")
    b(f"v_add_f32_dpp v89, v89, v89 row_mirror {D}")
    b(fill[2])
    b(f"v_max_f32_dpp v88, v88, v88 row_half_mirror {D}")
    b("v_add_f32_dpp v89, v89, v89 row_bcast:15 row_mask:0xa bank_mask:0xf")
    b(fill[3])
    b(f"v_max_f32_dpp v88, v88, v88 row_mirror {D}")
    b("v_add_f32_dpp v89, v89, v89 row_bcast:31 row_mask:0xc bank_mask:0xf")
    b(fill[4])
    b("v_max_f32_dpp v88, v88, v88 row_bcast:15 row_mask:0xa bank_mask:0xf")
    b(fill[5])
    b("v_readlane_b32 %[es], v89, 63")
    b("v_max_f32_dpp v88, v88, v88 row_bcast:31 row_mask:0xc bank_mask:0xf")
    b(fill[6])
    b(fill[7])
    b("v_readlane_b32 %[m], v88, 63")
    b("s_nop 1")
    b("v_cmp_eq_f32_e32 vcc, %[m], %[nrm]")
    b("s_ff1_i32_b64 %[bidx], vcc")
    return b



def fhex(x):
    import struct
    return "0x%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


ST = "s98"                       # the detection status of DETA / DETB: a fixed register, written by the cold code too
KAPPA = 6e-6                     # TRX_FAST_KAPPA (trx_device.h): certified-comparison margin of the FAST detector
D_ALL = "row_mask:0xf bank_mask:0xf"


def chain_term(b, acc, x, hp, half, first):
    """One term of a product-sum chain acc += x * h, h = the low (half 0) or high (half 1) float of the pair hp, on both
    components of x.  The chain's FIRST term is the product itself (v_pk_mul_f32), not an FMA onto an accumulator zeroed for it:
    fma(x, h, +0) and fl(x h) round the same exact product the same way and differ only where that product is an exact zero --
    +0 + -0 = +0, while the product keeps -0.  What that does to a chain: a sum in round-to-nearest is -0 only if both addends
    are -0, so a chain is -0 at some point only if EVERY product up to there is -0; behind the first product that is +0 or not a
    zero the accumulator is what it was when the chain started at +0 (s + -0 = s for every s but -0, and fma(x, h, -0) =
    fl(x h) for a non-zero product).  So the one difference a chain can show is an END at -0 in place of +0, when all of its
    products are -0 -- an x that is +0 (no sample and no correlation value of this kernel is ever -0: converted int16, and sums
    that start at +0) under weights that are all negative.  Where each chain's end goes, and why the sign of that zero reaches
    no output, is said at the chain: DETA, DETB, fir_moving."""
    sel = ("op_sel:[0,1{z}] op_sel_hi:[1,1{o}]" if half else "op_sel:[0,0{z}] op_sel_hi:[1,0{o}]")
    if first:
        b(f"v_pk_mul_f32 {acc}, {x}, {hp} " + sel.format(z="", o=""))
    else:
        b(f"v_pk_fma_f32 {acc}, {x}, {hp}, {acc} " + sel.format(z=",0", o=",1"))


# The TOA search's lane layout (this kernel's own: trx_kernel_nb.hip stages wa4f, ka and kb by nb_walk_src<LEVELS>()).  peakDetect()'s
# early / late bisection moves right where |early| < |late| and left otherwise; the candidate positions of a round's levels form a
# complete binary tree whose IN-ORDER traversal is the sorted list of positions.  Node (level k, index i) of a round of `levels`
# levels sits at in-order rank r = (2 i + 1) * 2^(levels - 1 - k) - 1, on lanes 2 r (early) and 2 r + 1 (late).  The compare
# gives, per lane, "my upper bound < my quad neighbour's lower bound": bit 2 r = a certain "early < late" (go right), bit 2 r + 1
# a certain "early > late" (go left); the two exclude each other (hi_E < lo_L <= hi_L < lo_E <= hi_E is no order; a NaN bound
# fails its compare).  Read in position order, a certified mask whose decisions are MONOTONE -- right, ..., right, left, ...,
# left: n times right -- ends the bisection at leaf n (the walk leaves exactly the n nodes that say "right" on its left), and
# such a mask is, on the round's 2 * nodes bits,
#     c = 0101..01 (bits >= 2 n)  1010..10 (bits < 2 n),   that is   c ^ ODD = the run of ones bfm(2 n),   ODD = the odd bits:
# one XOR, the first zero (2 n), and ONE compare with s_bfm of that length are certification and monotony at once (walk_first_zero).
# Every other mask -- an uncertified node, or certified decisions out of order -- takes the level-by-level walk
# (careful_walk: NB_ASM_COLD), which follows the reference's path whatever the mask is and asks certification of the nodes ON the
# path only.  Both hand on TWICE the leaf index.  tests/test_nb_toa_walk_cpu.py models both forms.
def walk_rank(levels, k, i):
    """in-order rank of node (level k, index i) of a complete tree of `levels` levels"""
    return (2 * i + 1) * (1 << (levels - 1 - k)) - 1


def walk_first_zero(b, x, m, t, cold_label, w="b64"):
    """x = c ^ ODD on the round's bits (no other bit set) -> m = 2 * leaf, or off to the level-by-level walk"""
    b(f"s_ff0_i32_{w} {m}, {x}")                                   # (x has zeros above the round's bits: never -1)
    b(f"s_bfm_{w} {t}, {m}, 0")
    b(f"s_cmp_eq_u{w[1:]} {t}, {x}")
    b(f"s_cbranch_scc0 {cold_label}")


def careful_walk(b, c, cd, p, pos, levels, unsure_label, w="b64"):
    """the reference's walk on the in-order layout, checking that every node ON THE PATH has a certified decision (cd = c | c >> 1):
    node (k, p) at bit 2 * rank = (p << (levels + 1 - k)) + (1 << (levels - k)) - 2.  Out: p = 2 * leaf"""
    b(f"s_lshr_{w} {cd}, {c}, 1")
    b(f"s_or_{w} {cd}, {cd}, {c}")
    b(f"s_mov_b32 {p}, 0")
    for lw in range(levels):
        assert 2 * walk_rank(levels, lw, 1) == (1 << (levels + 1 - lw)) + (1 << (levels - lw)) - 2
        b(f"s_lshl_b32 {pos}, {p}, {levels + 1 - lw}")
        b(f"s_add_u32 {pos}, {pos}, {(1 << (levels - lw)) - 2}")
        b(f"s_bitcmp0_{w} {cd}, {pos}")
        b(f"s_cbranch_scc1 {unsure_label}")
        b(f"s_bitcmp1_{w} {c}, {pos}")
        b(f"s_addc_u32 {p}, {p}, {p}")
    b(f"s_lshl_b32 {p}, {p}, 1")


# ------------------------------------------------------------------------------------------------------------------
# block DETA: detectBurst() behind fastPeakDetect (sigProcLib.cpp:1683-1695): edge gate, computePeakRatio gate (:1541-1571)
# on an estimate with a proven margin, round A of peakDetect()'s bisection (levels 0..4, trx_device.h peak_detect_fast; the 31
# nodes on lanes 0..61 in position order -- walk_rank) and its certified walk.
#   in : %[bidx] %[len] %[czb] SGPR (czb = LDS byte address of cz[0]); %[m] SGPR |corr[bidx]|^2 (block AMAX's maximum); %[kr] %[ka] VGPR lane constants (byte offsets of the
#        lane's peak-ratio term and of round A's first tap, relative to &cz[bidx]); %[l16] VGPR 16 * lane; %[gkv] VGPR lane n =
#        thresh^2 / n (n = 5..8); %[c0] VGPR thresh^2 * 1.0001e-5
#   out: status in the FIXED register NB_ASM_ST (the kernel binds its operand to it: "={s98}"), 0 miss / 1 found / 2 gate too
#        close to call / 3 an uncertified decision on the path; %[e] SGPR earlyIndex * 512 after round A; %[km] VGPR KAPPA *
#        |corr[bidx]|^2 (round B's margin term)
# The main path falls through the block: its rare sides -- the gate's exit, the careful walk -- are in NB_ASM_COLD, a statement
# behind the burst loop that names fixed registers only (which is why the status has one), and come back to .Lnb_da_walked /
# .Lnb_da_end; the edge gate leaves for .Lnb_da_end directly.
# The gate: reference |amp| / (sqrtf(avg / num) + 1e-5) < thresh.  Estimate t2 = avg * thresh^2 / num (avg tree-summed: within
# 6e-7; t2 within 1.2e-6 of the reference's squared threshold without its 1e-5).  (rms + 1e-5)^2 >= rms^2, so amp2 < t2 (1 -
# 1.2e-5) is a certain miss; (rms + 1e-5)^2 <= rms^2 (1 + 1e-5) + 1.0001e-5 (2ab <= a^2 + b^2), so amp2 > t2 * 1.000024 + c0 is
# a certain pass; in between (one burst in ~5e4) the burst is left to the general kernel, which rounds as the reference does.
# ------------------------------------------------------------------------------------------------------------------
def block_deta(wa4_off):
    b = Block("DETA", ("bidx", "len", "czb", "e", "m"))
    cold = Block("DETA_COLD")
    X = lambda k: vreg(88 + 2 * k, 2)            # round A samples 0..7
    Y = lambda k: vreg(112 + 2 * k, 2)           # samples 8..15
    # the edge gate (:1683): 3 <= bidx <= len - 3 as ONE unsigned range compare (len >= 16).  A window without a maximum above
    # zero (fastPeakDetect, :1120-1139: every |corr|^2 is +0, so the first lane holds "the maximum" and bidx = -lag0 <= 0) leaves here, too
    b(f"s_mov_b32 {ST}, 0")
    b("s_sub_u32 s88, %[bidx], 3")
    b("s_sub_u32 s89, %[len], 6")
    b("s_cmp_gt_u32 s88, s89")
    b("s_cbranch_scc1 .Lnb_da_end")
    b("s_lshl3_add_u32 s89, %[bidx], %[czb]")                      # &cz[bidx]
    b("s_add_u32 s90, %[len], -1")
    b("v_add_u32_e32 v65, s89, %[kr]")
    b("s_lshl3_add_u32 s90, s90, %[czb]")                          # &cz[len - 1]
    b("v_add_u32_e32 v66, s89, %[ka]")
    b("v_mov_b32_e32 v67, s90")
    b("v_mov_b64_e32 v[72:73], 0")
    # (the chip runs at its power limit: what only a few lanes need runs on those lanes -- the eight terms of the gate on lanes 0..7)
    b("s_bfm_b64 exec, 8, 0")
    b("ds_read_b64 v[70:71], v65")                                 # this lane's peak-ratio term (read before cz[len - 1] is zeroed)
    b("s_mov_b64 exec, 1")
    b("ds_write_b64 v67, v[72:73]")                                # interpolatePoint() never reads the last correlation sample (:1105)
    b("s_mov_b64 exec, -1")
    b(f"ds_read_b128 v[76:79], %[l16] offset:{wa4_off}")
    b(f"ds_read_b128 v[80:83], %[l16] offset:{wa4_off + 1024}")
    for u in range(8):
        b(f"ds_read_b64 {X(u)}, v66 offset:{8 * u}")
    # m = |corr[bidx]|^2 is block AMAX's wave maximum, bit for bit: CORR's tail forms |corr|^2 of the lane that holds lag bidx as
    # v_pk_mul_f32 / v_add_f32 (im^2 + re^2) on the value it stores to cz[bidx] -- in the moving, the wide and the multiplying
    # form alike -- and the maximum IS that lane's value (v_cmp_eq found it): no read of cz[bidx], no second square.  It goes
    # into the fixed register the cold gate exit reads.
    b("v_mov_b32_e32 v74, %[m]")
    # number of in-range terms (:1555-1562) -> thresh^2 / num: scalar instructions, placed in the wait states of the vector ones
    # (thresh^2 / num, num = 5..8: lane num of %[gkv], made in front of the burst loop -- one v_readlane in place of three
    # compare / select pairs, and no scalar register is held for the four constants across the loop)
    sc = ["s_add_u32 s91, %[bidx], -1", "s_sub_u32 s92, %[len], %[bidx]", "s_min_u32 s91, s91, 4", "s_add_u32 s92, s92, -2",
          "s_min_u32 s92, s92, 4", "s_add_u32 s91, s91, s92", "v_readlane_b32 s92, %[gkv], s91"]
    for t in sc[:3]:
        b(t)
    b(f"v_mul_f32_e32 %[km], {fhex(KAPPA)}, v74")
    b(sc[3])
    b("s_waitcnt lgkmcnt(11)")
    # (the chip runs at its power limit: what only a few lanes need runs on those lanes -- the eight terms of the gate on lanes 0..7)
    b("s_bfm_b64 exec, 8, 0")
    b("v_pk_mul_f32 v[70:71], v[70:71], v[70:71]")
    b(sc[4])
    b("v_add_f32_e32 v75, v71, v70")
    b(sc[5])
    b(sc[6])
    b(f"v_add_f32_dpp v75, v75, v75 quad_perm:[1,0,3,2] {D_ALL}")
    b("s_nop 1")
    b(f"v_add_f32_dpp v75, v75, v75 quad_perm:[2,3,0,1] {D_ALL}")
    b("s_nop 1")
    b(f"v_add_f32_dpp v75, v75, v75 row_half_mirror {D_ALL}")     # lanes 0..7: sum of the eight terms
    b("v_mul_f32_e32 v112, s92, v75")                              # t2
    b(f"v_mul_f32_e32 v113, {fhex(1.0 - 1.2e-5)}, v112")
    b(f"v_fmamk_f32 v114, v112, {fhex(1.000024)}, %[c0]")
    # (v113 <= v112 <= v114: what is no certain pass leaves, and the cold exit tells the certain miss from the too-close-to-call)
    b("v_cmp_gt_f32_e32 vcc, v74, v114")
    b("s_cbranch_vccz .Lnbc_da_gate")
    b("s_mov_b64 exec, -1")
    # ---- round A: interp over taps fl-7 .. fl+8 with this lane's weights, two FMA chains (even / odd taps)
    b(f"ds_read_b128 v[104:107], %[l16] offset:{wa4_off + 2048}")
    b(f"ds_read_b128 v[108:111], %[l16] offset:{wa4_off + 3072}")
    for u in range(8):
        b(f"ds_read_b64 {Y(u)}, v66 offset:{8 * (8 + u)}")
    b("s_waitcnt lgkmcnt(10)")

    # (p0, p1 of the two-chain sums START as the product of their first tap -- chain_term, below; a chain that ends at -0
    # where it ended at +0 vanishes in |interp|^2)
    def fmas(xs, qa, qb, first):
        for u in range(0, 8, 2):
            q = qb if (u & 4) else qa
            hp = vreg(q + (2 if (u & 2) else 0), 2)
            chain_term(b, "v[84:85]", xs(u), hp, 0, first and u == 0)
            chain_term(b, "v[86:87]", xs(u + 1), hp, 1, first and u == 0)
    fmas(X, 76, 80, True)
    b("s_waitcnt lgkmcnt(0)")
    fmas(Y, 104, 108, False)
    # (the three wait states of the packed results carry scalar set-up: ODD of the walk -- the odd bits of round A's 31 nodes,
    # bits 1 .. 61 -- and the status of a found burst)
    b("s_mov_b32 s96, 0xaaaaaaaa")
    b("v_pk_add_f32 v[84:85], v[84:85], v[86:87]")
    b("s_mov_b32 s97, 0x2aaaaaaa")
    b("v_pk_mul_f32 v[84:85], v[84:85], v[84:85]")
    b(f"s_mov_b32 {ST}, 1")
    b("v_add_f32_e32 v88, v85, v84")                               # nv = |interp|^2
    # certified comparison: r = KAPPA (nv + m); sure "early < late" when hi_E < lo_L, sure "early > late" when hi_L < lo_E
    b(f"v_fmamk_f32 v89, v88, {fhex(KAPPA)}, %[km]")
    b("v_sub_f32_e32 v90, v88, v89")
    b("v_add_f32_e32 v91, v88, v89")
    b("s_lshl_b32 s94, %[bidx], 9")
    b(f"v_mov_b32_dpp v90, v90 quad_perm:[1,0,3,2] {D_ALL}")
    b("v_cmp_lt_f32_e64 s[88:89], v91, v90")
    b("s_bfe_u64 s[90:91], s[88:89], 0x3e0000")                    # the 31 nodes' bits (lanes 62, 63 hold no node)
    b("s_xor_b64 s[90:91], s[90:91], s[96:97]")
    walk_first_zero(b, "s[90:91]", "s95", "s[92:93]", ".Lnbc_da_careful")
    b(".Lnb_da_walked:")
    b("s_lshl4_add_u32 s94, s95, s94")                             # off = 32 leaf - 496 (s95 = 2 leaf); E = (bidx - 1) * 512 + off
    b("s_add_u32 %[e], s94, -1008")
    b(".Lnb_da_end:")
    # ---- cold (NB_ASM_COLD, behind the burst loop): fixed registers only
    cold(".Lnbc_da_careful:")
    careful_walk(cold, "s[88:89]", "s[90:91]", "s95", "s96", 5, ".Lnbc_da_unsure")
    cold("s_branch .Lnb_da_walked")
    cold(".Lnbc_da_unsure:")
    cold(f"s_mov_b32 {ST}, 3")
    cold("s_branch .Lnb_da_end")
    cold(".Lnbc_da_gate:")                                         # (EXEC: lanes 0..7, as the gate's compare left it)
    cold("v_cmp_lt_f32_e32 vcc, v74, v113")                        # certain miss: status 0; else too close to call
    cold("s_cmp_eq_u64 vcc, 0")
    cold(f"s_cselect_b32 {ST}, 2, 0")
    cold("s_mov_b64 exec, -1")
    cold("s_waitcnt lgkmcnt(0)")
    cold("s_branch .Lnb_da_end")
    return b, cold


# ------------------------------------------------------------------------------------------------------------------
# block DETB: round B of the bisection (levels 5..8 on lanes 0..29 in position order -- walk_rank --, the sixteen possible final positions on lanes 32..47),
# its certified walk, and the interpolated peak value at the final position (peakDetect(), :1141-1186).
#   in : %[e] SGPR earlyIndex * 512; %[kb] VGPR lane constant offB; %[czb] SGPR; %[km] VGPR
#   out: status 1 / 3 in the fixed register NB_ASM_ST; %[toa] SGPR final position * 512; %[xr] %[xi] SGPR interpolated value
#        (status 3: undefined).  The careful walk is in NB_ASM_COLD (see DETA).
# sinc LUT index of a fraction f: taps i <= fl use q = 512 k + f, taps i > fl use q = 512 k + (512 - f), XOR-swizzled
# (trx_tables.h: q ^ ((q >> 4) & 31), which leaves the row 512 k alone; swz(512) = 512).  This kernel's LDS copy of the LUT
# (offset 0) holds rows 2j and 2j + 1 interleaved -- trx_tables.h, trx_sincp_idx: entry (row r, column slot s) at float
# (r >> 1) * 1026 + 2 s + (r & 1) -- so that the weights of taps k and k + 1 are ONE 8-byte read (a 4-byte read costs the LDS
# pipe what an 8-byte one costs).  The descending side (rows 7 - u) finds its pair in swapped order: the op_sel of the FMA
# picks the half.  The ascending side's column slot 512 (f = 0: q = 512 (u + 1), column 0 of the NEXT row) is a pair of its own,
# rows 2j + 1 and 2j + 2 at column 0, behind the 512 slots of pair j (the zero tail is its last entry): no special case here.
# Banks: an 8-byte slot s of a 32-lane half occupies banks 2 s, 2 s + 1 mod 64 -- conflict-free exactly where the 4-byte gather
# was (s mod 32 distinct), so the swizzle stays (tools/lds_stride_conflicts.py, sinc_pairs()).
# ------------------------------------------------------------------------------------------------------------------
SINCP_PAIR_BYTES = 1026 * 4     # TRX_SINCP_STRIDE floats (trx_tables.h): one pair of rows, 513 column slots of 8 bytes


def block_detb():
    b = Block("DETB", ("e", "czb", "toa", "xr", "xi"))
    cold = Block("DETB_COLD")
    X = lambda k: vreg(80 + 2 * k, 2)
    W = lambda k: 96 + k
    Y = lambda k: vreg(104 + 2 * k, 2)
    V = lambda k: 120 + k
    # p0, p1 (v[64:65], v[66:67]) start as the products of taps 0 and 1 (chain_term), under the round's mask: lanes 30, 31 and
    # 48..63 keep whatever the block in front left there, the sum and the compare below run on it, and NOTHING reads the
    # result -- the walks test bits 0..29 of the compare (first zero: masked to them; level by level: bit pos and,
    # through c | c >> 1, bit pos + 1 <= 29), the v_readlane pair reads lanes 32 + p, p = 0..15.  (exec_ok: told to the checker.)
    # The sign of a zero: lanes 0..29 go through |interp|^2.  The final positions' value (lanes 32..47) is read as it is, per
    # component p0 + p1.  p1 holds tap fl, the tap AT the peak's floor: its weight is sincv[f], f = 0..511 -- sinc on [0, 1),
    # positive for every fraction, 1 at fraction 0 (tests/test_nb_amp_lanes_cpu.py checks the blob) -- and cz[] is never -0
    # (sums from +0) nor subnormal, so that product is -0 for no input: p1 never ends at -0, and p0 + p1 with p0 = -0 is p1 +
    # (+0) bit for bit (p1 = +0: +0 + -0 = +0).
    b("v_add_u32_e32 v68, %[e], %[kb]")                            # position of this lane (1/512 symbol)
    b("s_add_u32 s88, %[czb], -56")
    b("s_mov_b32 exec_lo, 0x3fffffff")                             # lanes 0..29: 15 nodes x {early, late}; 32..47: final positions
    b("s_mov_b32 exec_hi, 0xffff")
    b("v_ashrrev_i32_e32 v69, 9, v68")
    b("v_and_b32_e32 v70, 0x1ff, v68")
    b("v_lshl_add_u32 v69, v69, 3, s88")                           # &cz[fl - 7]
    b("v_bfe_u32 v71, v70, 4, 5")
    b("v_sub_u32_e32 v72, 0x200, v70")
    b("v_xor_b32_e32 v71, v71, v70")
    b("v_bfe_u32 v73, v72, 4, 5")
    b("v_lshlrev_b32_e32 v71, 3, v71")                             # taps fl-7 .. fl: rows 7 - u, column slot swz(f) of the row pairs
    b("v_xor_b32_e32 v72, v73, v72")
    b("v_lshlrev_b32_e32 v72, 3, v72")                             # taps fl+1 .. fl+8: rows u, column slot swz(512 - f)
    for u in range(8):
        b(f"ds_read_b64 {X(u)}, v69 offset:{8 * u}")
        if not (u & 1):
            # rows 6 - u, 7 - u are ONE 8-byte entry of pair 3 - u / 2: the weight of tap u + 1 in the low register, of tap u in the high one
            b(f"ds_read_b64 {vreg(W(u), 2)}, v71 offset:{SINCP_PAIR_BYTES * (3 - (u >> 1))}")

    def fma2(xs, ws, u, swapped, first=False):
        chain_term(b, "v[64:65]", xs(u), vreg(ws(u), 2), 1 if swapped else 0, first)
        chain_term(b, "v[66:67]", xs(u + 1), vreg(ws(u), 2), 0 if swapped else 1, first)
    # software pipeline: 12 loads in flight; each step consumes two taps of the first half and issues two of the second
    for k in range(4):
        b("s_waitcnt lgkmcnt(9)")
        fma2(X, W, 2 * k, True, k == 0)
        b(f"ds_read_b64 {Y(2 * k)}, v69 offset:{8 * (8 + 2 * k)}")
        b(f"ds_read_b64 {vreg(V(2 * k), 2)}, v72 offset:{SINCP_PAIR_BYTES * k}")      # rows 2k, 2k + 1: taps 2k, 2k + 1 in order
        b(f"ds_read_b64 {Y(2 * k + 1)}, v69 offset:{8 * (8 + 2 * k + 1)}")
    for k in range(4):
        b(f"s_waitcnt lgkmcnt({9 - 3 * k})")
        fma2(Y, V, 2 * k, False)
    b("s_mov_b64 exec, -1")
    b("v_pk_add_f32 v[74:75], v[64:65], v[66:67]")                 # interpolated value at this lane's position
    b("s_add_u32 s92, %[e], 497")
    b("v_pk_mul_f32 v[76:77], v[74:75], v[74:75]")
    b(f"s_mov_b32 {ST}, 1")
    b("v_add_f32_e32 v78, v77, v76")
    b(f"v_fmamk_f32 v79, v78, {fhex(KAPPA)}, %[km]")
    b("v_sub_f32_e32 v96, v78, v79")
    b("v_add_f32_e32 v97, v78, v79")
    b("s_nop 0")
    b(f"v_mov_b32_dpp v96, v96 quad_perm:[1,0,3,2] {D_ALL}")
    b("v_cmp_lt_f32_e64 s[88:89], v97, v96")
    b("s_and_b32 s90, s88, 0x3fffffff")                            # the 15 nodes' bits
    b("s_xor_b32 s90, s90, 0x2aaaaaaa")
    walk_first_zero(b, "s90", "s94", "s91", ".Lnbc_db_careful", "b32")
    b(".Lnb_db_walked:")
    b("s_lshr_b32 s93, s94, 1")
    b("s_add_u32 %[toa], s94, s92")                                # E + offB + 512, offB = 2 leaf - 15 (s94 = 2 leaf)
    b("s_add_u32 s93, s93, 32")                                    # lane that evaluated the final position
    b("v_readlane_b32 %[xr], v74, s93")
    b("v_readlane_b32 %[xi], v75, s93")
    b(".Lnb_db_end:")
    b.exec_ok = {"v64", "v65", "v66", "v67"}                       # (read under the full mask, used from the round's lanes only: above)
    # ---- cold (NB_ASM_COLD): fixed registers only
    cold(".Lnbc_db_careful:")
    careful_walk(cold, "s88", "s90", "s94", "s95", 4, ".Lnbc_db_unsure", "b32")
    cold("s_branch .Lnb_db_walked")
    cold(".Lnbc_db_unsure:")
    cold(f"s_mov_b32 {ST}, 3")
    cold("s_branch .Lnb_db_end")
    return b, cold

# ------------------------------------------------------------------------------------------------------------------
# block TAIL: what detectBurst() does behind peakDetect (:1695-1708) for a found burst, the demodulator's set-up and the
# burst's result record.
#   * TOA in 1/512 symbol -> shift and delay-filter row of the straight-line demodulator; fetch of the burst's low-edge
#     tap rows (trx_tables.edge8: 768 bytes, 16 per lane) from L2, as early as possible
#   * computeCI (:1608-1639): 16 S = the summed power of the 16 samples at the rounded TOA (tree sum; the scale 1 / 16, exact, and
#     C = |peak|^2 / ci_den are flush_records()'s, once per 64 bursts)
#   * amp = peak / gain (:1701), toa = position - sync->toa - head (:1704, :1768)
#   * 1 / amp -> the per-lane multiplier VP of the output stage (block DEMOD), each lane its own component: amp_lane()
#   * the result record: field k in lane k of one register (rc, toa, amp.re, amp.im, ci, energy, rssi, flags)
#   in : SGPR toa (position * 512), xr / xi (peak value), t5 ((int)(sync->toa * 512)), ampb (LDS byte address of the
#        sequence's row of (A, B) pairs: trx_kernel_nb.hip lamp, 16-byte aligned), e8lo / e8hi (address of tab->edge8), es (energy sum), fsdb (20 log10 full_scale), flags;
#        VGPR l16 (16 * lane), l4 (4 * lane), aw (slice base + 8 * lane: D[lane] is offset AW_D of it)
#   out: SGPR ok (0: TOA outside the straight-line geometry -- left through NB_ASM_COLD, the sum done), ssum (16 S); VGPR d0 d1 d2 (block DEMOD)
# ------------------------------------------------------------------------------------------------------------------
FIDX = "s99"                     # TAIL: the burst's delay-filter row, from the row fetch at the head to the composite row's address


def block_tail():
    b = Block("TAIL", ("toa", "xr", "xi", "t5", "ampb", "e8lo", "e8hi", "ok", "ssum", "pb", "cb", "db"))
    cold = Block("TAIL_COLD")
    b("v_and_or_b32 v65, %[l4], 12, %[ampb]")                      # &A[lane & 3] of the sequence's row (32 bytes, 16-byte aligned)
    b("ds_read2_b32 v[70:71], v65 offset1:4")                      # this lane's (A, B) of 1 / gain: amp_lane(), below
    b("s_sub_u32 s88, %[t5], %[toa]")
    b("s_add_u32 s87, s88, 5120")                                  # nk = -(toa512 - t5 - 10 * 512)
    b("s_mov_b32 %[ok], 0")
    b("s_and_b32 s91, s87, 127")
    b(f"s_lshr_b32 {FIDX}, s91, 1")
    b("s_cmp_ge_u32 s91, 2")
    b(f"s_cselect_b32 {FIDX}, {FIDX}, 64")                           # delay filter row (64 = none): kept for the composite row (DEMOD)
    b(f"s_mul_i32 s93, {FIDX}, 768")
    b("s_add_u32 s94, %[e8lo], s93")
    b("s_addc_u32 s95, %[e8hi], 0")
    b("s_abs_i32 s96, %[toa]")                                     # roundf(toa): half away from zero on k / 512
    b("s_add_u32 s96, s96, 256")
    b("global_load_dwordx4 v[120:123], %[l16], s[94:95]")
    b("s_lshr_b32 s96, s96, 9")
    b("s_sub_u32 s97, 0, s96")
    b("s_cmp_lt_i32 %[toa], 0")
    b("s_cselect_b32 s96, s97, s96")
    b("s_lshl_b32 s96, s96, 3")
    b("v_add_u32_e32 v64, s96, %[aw]")                             # &D[rt + lane] - AW_D: sample ps + lane, ps = start + 1 - N + rt
    b("s_bfm_b64 exec, 16, 0")
    b(f"ds_read_b64 v[66:67], v64 offset:{AW_D}")                              # computeCI's sixteen samples (:1608-1639)
    b("s_mov_b64 exec, -1")
    # (the burst's record -- C/I, RSSI, amp, toa -- is not made here: its inputs go into lane `slot` of seven registers and 64
    # records are made at once, trx_kernel_nb.hip flush_records; what is per burst is S, computeCI's mean sample power)
    block_demod(b)
    b(".Lnb_tl_end:")
    # ---- cold (NB_ASM_COLD): the geometry's exit
    cold(".Lnbc_tl_wait:")
    cold("s_waitcnt vmcnt(0)")                                     # (the tap rows were requested: their registers are free again behind this)
    cold("s_branch .Lnb_tl_end")
    return b, cold


# ------------------------------------------------------------------------------------------------------------------
# block DEMOD: demodGmskBurst (:2055-2072) of the usual geometry, fused: delay o decimate as one 24-tap filter at the
# symbol instants (fir24x3, trx_k4_common.h -- the same sums in the same order), rotation / 1/amp / slicer input in
# registers.  The filter is a MOVING accumulator (fir_moving, below): every lane reads only its own twelve samples.
#   lane m < 50: samples x[12 m + c + 16 + r], composite row; the sums of symbols 4 + 3 l + j (l < 48) start in lane l and
#   end in lane l + 2.  Lanes 52 + 3 e + t carry low-edge symbol e = 0..3 (truncated rows, parked in D): t = 0, 1 the main
#   part (row e) in slot 0 -- it ends in slot 0 of lane 54 + 3 e; t = 2 the taps u < 8 (row 4 + e) as a sum that stays in
#   slot 1 of that lane; the two are joined by one add there.
#   CONSUMED (lane, slot) pairs: lanes 2..49, slots 0..2; lanes 54, 57, 60, 63, slot 0.  Everything else (lanes 0, 1, 50, 51, the
#   other slots of lanes 52..63) holds partial sums of no symbol and is never stored.
#   in : SGPR nk, pb (LDS byte address of P[0] of this wave), cb (LDS byte address of comp + 32: tap U0 of row 0), db (LDS
#        byte address of D); VGPR rows (4), vp, l16, kic (lane constant: 8 * first symbol of the lane's twelve samples), ktp
#        (lane constant: byte offset of the lane's tap row inside D, -1 for the lanes on the composite row)
#   out: VGPR d0 d1 d2: the sliced soft bits of the three symbols that END in the lane: real((-j)^i z / amp) through vectorSlicer
# ------------------------------------------------------------------------------------------------------------------
def amp_lane(b, fill):
    """amp = peak / gain (:1701) and the output stage's multiplier VP[lane & 3] = (sx, sy, -sx, -sy), (sx, sy) = 1 / amp =
    conj(amp) / |amp|^2 (Complex.h:75, 144-150), made per LANE: a lane needs its own component of amp and the square of the
    other one, not the whole wave-uniform value and two selects.  The kernel stages, per training sequence, the four pairs
    (A, B) by lane & 3 of (g0, g1) = 1 / gain (trx_tables.h, trx_amp_lane_pair: (g0, -g1), (-g1, -g0), (-g0, g1), (g1, g0)):
        comp = fl(fl(xr A) + fl(xi B)) = +amp.re, -amp.im, -amp.re, +amp.im  -- the bits of Complex.h:74's fl(xr g0) - fl(xi g1)
                                         and fl(xr g1) + fl(xi g0): negation is exact, and a - b IS a + (-b);
        n    = fl(comp^2) + the quad neighbour's fl(comp^2) (lanes 0 <-> 1, 2 <-> 3)  = |amp|^2 as fl(im^2) + fl(re^2): a square
                                         loses the sign, the addition is commutative;
        VP   = fl(comp * rcp(n))         -- sx = fl(re r), sy = fl(-im r), and fl(-x r) = -fl(x r).
    One case is not the same bits: a component of amp that cancels to an EXACT zero is +0 in every lane here, where the negated
    variants (-amp.im, -amp.re) had -(+0) = -0.  That lane's VP is then a zero of the other sign, its product with a filter sum a
    zero of some sign, and the output stage adds the other component's product onto it (a non-zero addend absorbs it; two zeros
    give a zero) in front of the slicer's fma(d, 0.5, 0.5), which takes +0 and -0 alike to 0.5: no soft bit sees it, and n, a sum
    of squares, does not either (tests/test_nb_amp_lanes_cpu.py models both forms through the slicer).
    In: v[70:71] = (A, B), the peak in %[xr] %[xi] (SGPR); out: v119.  Temporaries: v70, v71, v112 (P[0], dead behind the
    sample reads).  fill: five independent instructions of the caller -- the DPP source's two wait states and the reciprocal's
    one among them.  The geometry's cold exit leaves in front of this: it forms amp in C++ (trx_kernel_nb.hip), as it did."""
    assert len(fill) == 5
    b("v_mul_f32_e32 v70, %[xr], v70")
    b("v_mul_f32_e32 v71, %[xi], v71")
    b(fill[0])
    b("v_add_f32_e32 v119, v70, v71")                              # comp
    b(fill[1])
    b("v_mul_f32_e32 v112, v119, v119")
    b(fill[2])
    b(fill[3])
    b(f"v_add_f32_dpp v112, v112, v112 quad_perm:[1,0,3,2] {D_ALL}")     # |amp|^2
    b("v_rcp_f32_e32 v112, v112")
    b(fill[4])
    b("v_mul_f32_e32 v119, v119, v112")                            # VP


def block_demod(b):
    # the straight-line geometry: shift w = nk >> 7 in -36 .. 0 (0 <= TOA <= 9 symbols); other bursts leave with ok = 0 -- the sum
    # of computeCI is done, 1 / amp is not -- and take the general form of the demodulator (trx_kernel_nb.hip, cold)
    ACC = [64, 66, 68]
    X = lambda r: vreg(72 + 2 * r, 2)
    P = [112, 113, 114, 115]
    # 16 S = the sum of |sample|^2 over computeCI's sixteen samples (lanes 0..15: a tree sum), in the wait states of the address arithmetic
    b("s_bfm_b64 exec, 16, 0")
    b("s_waitcnt lgkmcnt(0)")
    b("v_pk_mul_f32 v[66:67], v[66:67], v[66:67]")
    b("s_ashr_i32 s88, s87, 7")                                    # w
    b("v_add_f32_e32 v81, v67, v66")                               # |sample|^2
    b("s_sub_u32 s91, -18, s88")                                   # c = -24 - w + U0: tap U0 of symbol i reads sample 4 i + c
    b("s_and_b32 s92, s91, 3")                                     # ph0
    b(f"v_add_f32_dpp v81, v81, v81 quad_perm:[1,0,3,2] {D_ALL}")
    b("s_ashr_i32 s93, s91, 2")
    b("s_mul_i32 s94, s92, 180")
    b(f"v_add_f32_dpp v81, v81, v81 quad_perm:[2,3,0,1] {D_ALL}")
    b("s_add_u32 s94, s94, s93")
    b("s_lshl3_add_u32 s94, s94, %[pb]")                           # &P[ph0][m = c >> 2] - 12 entries
    b(f"v_add_f32_dpp v81, v81, v81 row_half_mirror {D_ALL}")
    b(f"s_mul_i32 s95, {FIDX}, 144")                                 # (the filter's row: made once, at the block's head)
    b("s_add_u32 s95, s95, %[cb]")                                 # composite row of the burst's delay filter, from tap U0
    b(f"v_add_f32_dpp v81, v81, v81 row_mirror {D_ALL}")         # 16 S (row 0): the power-of-two scale is flush_records()'s, once per 64 bursts
    b("s_sub_u32 s96, 0, s88")
    b("v_readlane_b32 %[ssum], v81, 0")
    b("s_mov_b64 exec, -1")
    b("s_cmp_gt_u32 s96, 36")
    b("s_cbranch_scc1 .Lnbc_tl_wait")
    b("s_mov_b32 %[ok], 1")
    b(f"v_add_u32_e32 {vreg(P[0])}, s94, %[kic]")
    for k in range(1, 4):
        # p[k] = p[0] + (k * PH_A + ((ph0 + k) >> 2) * (1 - 4 * PH_A)) entries: the carry (ph0 + k >= 4) is one compare, and the
        # k * PH_A entries are in the offset field of the reads
        b(f"s_cmp_gt_u32 s92, {3 - k}")
        b(f"s_cselect_b32 s96, {(1 - 4 * PH_A) * 8}, 0")
        b(f"v_add_u32_e32 {vreg(P[k])}, s96, {vreg(P[0])}")
    PH0 = 96                                                       # byte offset of PH_M0 entries
    # (all 64 lanes run the filter: an accumulator passes through every lane below the one it ends in)
    # the lane's twelve samples do not depend on the tap rows: requested in front of the wait for those (L2 latency)
    for r in range(12):
        b(f"ds_read_b64 {X(r)}, {vreg(P[r & 3])} offset:{PH0 + 8 * (r >> 2) + (r & 3) * PH_A * 8}")
    # the tap row's address and the output stage's multiplier (amp_lane) share the slots: each is the other's wait states
    amp_lane(b, ["v_cmp_lt_i32_e32 vcc, -1, %[ktp]", "v_add_u32_e32 v117, %[db], %[ktp]", "v_mov_b32_e32 v118, s95",
                 "v_add_u32_e32 v116, %[db], %[l16]",
                 "v_cndmask_b32_e32 v117, v118, v117, vcc"])       # this lane's tap row
    b("s_waitcnt vmcnt(0)")
    b("ds_write_b128 v116, v[120:123]")                            # park the low-edge rows: lane l < 48 holds floats 4l .. 4l+3 of the 8 x 24 block
    fir_moving(b, ACC, X)
    # output stage: low-edge symbol e = main part (slot 0, arrived in lane 54 + 3 e) + taps u < 8 (slot 1 of that lane); symbol i
    # wants real((-j)^i z / amp) = z.x * VP[k] + z.y * VP[k - 1], k = i & 3: a quad permutation of VP, applied by the DPP operand.
    # The sums of lane L are those of symbols 3 L - 2 + j (lanes 54 + 3 e: 160 + 9 e = e mod 4, slot 0): k = (2 + j - L) & 3
    b("s_mov_b32 exec_lo, 0")
    b("s_mov_b32 exec_hi, 0xfff00000")
    b("v_pk_add_f32 v[64:65], v[64:65], v[66:67]")                 # main + low (lanes 52..63; consumed: 54, 57, 60, 63)
    b("s_mov_b64 exec, -1")
    b(f"v_mul_f32_dpp %[d1], v119, v66 quad_perm:[3,2,1,0] {D_ALL}")
    b(f"v_mul_f32_dpp %[d2], v119, v68 quad_perm:[0,3,2,1] {D_ALL}")
    b(f"v_mul_f32_dpp %[d0], v119, v64 quad_perm:[2,1,0,3] {D_ALL}")
    b(f"v_fmac_f32_dpp %[d1], v119, v67 quad_perm:[2,1,0,3] {D_ALL}")
    b(f"v_fmac_f32_dpp %[d2], v119, v69 quad_perm:[3,2,1,0] {D_ALL}")
    b(f"v_fmac_f32_dpp %[d0], v119, v65 quad_perm:[1,0,3,2] {D_ALL}")
    # vectorSlicer (:546-556): 0.5 * (x + 1) clamped to [0, 1] -- the clamp is the output modifier of the FMA that forms the value
    for d in ("d1", "d2", "d0"):
        b(f"v_fma_f32 %[{d}], %[{d}], 0.5, 0.5 clamp")


# ------------------------------------------------------------------------------------------------------------------
# block FIRG: the composite filter alone, for the general form of the demodulator (cold: trx_kernel_nb.hip demod_general) --
# lane l < 52 computes the raw sums of symbols ic .. ic + 2 over taps U0 .. U0 + 23 of the burst's composite row.
#   in : SGPR %[nk], %[pb], %[cb] (as DEMOD); VGPR %[kic] 8 * ic of this lane (clamped by the caller)
#   out: VGPR pairs %[a0] %[a1] %[a2]
# ------------------------------------------------------------------------------------------------------------------
def block_firg():
    b = Block("FIRG", ("nk", "pb", "cb"))
    ACC = ["%[a0]", "%[a1]", "%[a2]"]
    RING = lambda v: vreg(72 + 2 * (v & 15), 2)
    CQ = [104, 108]
    P = [112, 113, 114, 115]
    b("s_ashr_i32 s88, %[nk], 7")                                  # w
    b("s_and_b32 s89, %[nk], 127")
    b("s_lshr_b32 s90, s89, 1")
    b("s_cmp_ge_u32 s89, 2")
    b("s_cselect_b32 s90, s90, 64")                                # fidx
    b("s_sub_u32 s91, -18, s88")                                   # c = -24 - w + U0
    b("s_and_b32 s92, s91, 3")
    b("s_ashr_i32 s93, s91, 2")
    b("s_mul_i32 s94, s92, 180")
    b("s_add_u32 s94, s94, s93")
    b("s_lshl3_add_u32 s94, s94, %[pb]")
    b("s_mul_i32 s95, s90, 144")
    b("s_add_u32 s95, s95, %[cb]")
    b(f"v_add_u32_e32 {vreg(P[0])}, s94, %[kic]")
    for k in range(1, 4):
        b(f"s_add_u32 s96, s92, {k}")
        b("s_lshr_b32 s96, s96, 2")
        b(f"s_mul_i32 s96, s96, {(1 - 4 * PH_A) * 8}")
        b(f"s_add_u32 s96, s96, {k * PH_A * 8}")
        b(f"v_add_u32_e32 {vreg(P[k])}, s96, {vreg(P[0])}")
    for j_ in range(3):
        b(f"v_mov_b64_e32 {ACC[j_]}, 0")
    b("v_mov_b32_e32 v117, s95")
    b("s_bfm_b64 exec, 52, 0")
    fir_core(b, ACC, RING, CQ, P, preload=True)
    b("s_mov_b64 exec, -1")
    return b


FIRM_LOW_LANE0 = 52              # first lane of the low-edge symbols (three lanes per symbol)


def fir_moving(b, ACC, X):
    """The composite filter as a moving accumulator.  Today's sum of lane l, slot j: ACC[j] = sum_{u = 0..23} x[12 l + c + 4 j + u] h[u],
    u ascending from +0.  With 4 j + u = 12 s + r (stage s = 0, 1, 2; r = 0..11) the sample is X_{l + s}[r], one of the twelve that
    lane l + s holds: in stage s lane m adds X_m[r] h[12 s + r - 4 j] into slot j for the r with 0 <= 12 s + r - 4 j < 24, r
    ascending, and between two stages the slot's accumulator moves one lane up (v_mov_b32_dpp wave_shr:1).  Every output is the
    same 24 FMAs in the same order from the same +0 -- the same bits -- and ends in lane l + 2 (slot 0 has no stage 2: it is
    carried there by a second move, so that the three sums of a lane belong to adjacent symbols).  (Since the chains start as
    products -- chain_term, no accumulator is zeroed -- "from the same +0" reads "up to the sign of an exact zero": see the
    paragraph on zero taps below.)
        terms (stage, slot):   slot 0: 12 12 0    slot 1: 8 12 4    slot 2: 4 12 8           = 72 FMAs per lane
    A slot is one dependent chain (packed FMA -> reader: 1 wait state, -> DPP source: 2); the three chains are interleaved so
    that every wait state is another chain's instruction.
    Low-edge symbols (lanes 52 + 3 e + t, rows of the parked block -- trx_tables.h edge8, unchanged):
      t = 0, 1: row e, samples [W, W + 12) and [W + 12, W + 24), W = 4 e + c: slot 0 is the main part, 24 FMAs from +0 like
                any other, and ends in lane 54 + 3 e;
      t = 2:    row 4 + e = [0, 0, six low taps, sixteen zeros], samples [W - 12, W): stage 0 of slot 1 is
                sum_{r = 4..11} x[W - 12 + r] row[r - 4] = sum_{u = 0..7} x[W - 8 + u] row[u] -- the low part, u ascending from +0.
                Slot 1's moves are masked off for lanes 52..63 (EXEC = lanes 0..51 around them), so the sum stays in its lane,
                and its stages 1 and 2 multiply the zero taps 8..23.
      Zero taps are bit-safe: the samples are converted int16, hence finite and never -0, so x * 0 = +-0.  A chain starts as the
      product of its first term (chain_term), so behind leading zero taps -- the low part's two, a truncated row's -- the
      accumulator is +0 or -0 where a chain from +0 had +0; the first tap T that is not zero then gives fma(x, T, +-0) =
      fl(x T), the same bits either way, unless that product is a zero too, and from the first non-zero product on the chain
      is what it was (s + -0 = s).  Zero taps BEHIND a sum leave it alone (fma(x, 0, s) = s for s not zero; a zero stays a
      zero).  So a slot's sum is the same bits as before, or -- all of its products zeros: every sample under a non-zero tap
      is 0 -- a zero whose sign may differ.  Where such a zero goes: main + low is one add (a zero of either sign added to a
      non-zero sum changes nothing, two zeros give a zero); the output stage multiplies z by VP, adds the other component's
      product -- a zero of either sign is absorbed by a non-zero addend, two zeros give a zero -- and the slicer's fma(d, 0.5,
      0.5) takes +0 and -0 alike to 0.5.  No soft bit sees the sign.  (tests/test_gpu_nb_amp_lanes.py: bursts whose first 48
      samples are zero, an all-zero burst, a zeroed polyphase row -- bytes against the general kernel.)
    Registers: six tap quads v96..v111, v124..v127, v120..v123 (the last one behind the first LDS wait: v120..v123 hold the
    parked rows until the ds_write in front has read them); v117 = the lane's tap row."""
    Q = [96, 100, 104, 108, 124, 120]
    for q in range(5):
        b(f"ds_read_b128 {vreg(Q[q], 4)}, v117 offset:{16 * q}")
    lds_q = list(range(5))                                         # tap quads outstanding, oldest first (everything older: in front)
    arrived = set()
    # per-slot programs
    prog = []
    for j in range(3):
        pj = []
        for s_ in range(3):
            for r in range(12):
                t = 12 * s_ + r - 4 * j
                if 0 <= t < 24:
                    pj.append(("fma", r, t))
            if s_ < 2:
                pj.append(("mov",))
        if j == 0:
            assert pj[-1] == ("mov",)                              # (slot 0: the carry to lane l + 2)
        else:
            assert pj[-1][0] == "fma"
        prog.append(pj)
    assert sum(1 for pj in prog for i in pj if i[0] == "fma") == 72
    pos = 0
    last = [(-10, "mov")] * 3                                      # (position, kind) of the slot's last writer
    ip = [0, 0, 0]
    q5_issued = False

    def ready(j):
        ins = prog[j][ip[j]]
        gap = pos - last[j][0] - 1
        if ins[0] == "fma":
            return gap >= (1 if last[j][1] == "fma" else 0)
        return gap >= 2

    while any(ip[j] < len(prog[j]) for j in range(3)):
        cand = [j for j in range(3) if ip[j] < len(prog[j]) and ready(j)]
        if not cand:
            b("s_nop 0")
            pos += 1
            continue
        # the chain with the most left first; among equals one whose taps have arrived
        def key(j):
            ins = prog[j][ip[j]]
            there = ins[0] == "mov" or (ins[2] >> 2) in arrived
            return (there, len(prog[j]) - ip[j])
        j = max(cand, key=key)
        ins = prog[j][ip[j]]
        ip[j] += 1
        if ins[0] == "fma":
            _, r, t = ins
            q = t >> 2
            if q not in arrived:
                n = len(lds_q) - 1 - lds_q.index(q)
                b(f"s_waitcnt lgkmcnt({n})")
                pos += 1
                for qq in lds_q[:lds_q.index(q) + 1]:
                    arrived.add(qq)
                del lds_q[:len(lds_q) - n]
                if not q5_issued:
                    b(f"ds_read_b128 {vreg(Q[5], 4)}, v117 offset:{16 * 5}")
                    lds_q.append(5)
                    q5_issued = True
                    pos += 1
            hp = vreg(Q[q] + (2 if (t & 2) else 0), 2)
            chain_term(b, vreg(ACC[j], 2), X(r), hp, t & 1, ip[j] == 1)   # (a slot's first term starts its chain: no zeroed accumulator)
            last[j] = (pos, "fma")
            pos += 1
        else:
            if j == 1:
                b(f"s_bfm_b64 exec, {FIRM_LOW_LANE0}, 0")          # the low parts (slot 1 of lanes 52..63) stay where they are
                pos += 1
            for c in range(2):
                b(f"v_mov_b32_dpp v{ACC[j] + c}, v{ACC[j] + c} {DPP_SHR}")
            pos += 2
            last[j] = (pos - 1, "mov")
            if j == 1:
                b("s_mov_b64 exec, -1")
                pos += 1
    b.firm_nops = sum(1 for t in b.ins if t == "s_nop 0")


def fir_core(b, ACC, RING, CQ, P, preload):
    """fir24x3 (trx_k4_common.h): taps outer, a ring of sixteen samples running four ahead, taps four at a time; v117 = the lane's
    tap row.  preload: the first twelve samples are requested here (DEMOD requests them earlier)"""
    D, NT, NV = 4, 24, 32
    PH0 = 96                                                       # byte offset of PH_M0 entries
    if preload:
        for v in range(8 + D):
            b(f"ds_read_b64 {RING(v)}, {vreg(P[v & 3])} offset:{PH0 + 8 * (v >> 2)}")
    b(f"ds_read_b128 {vreg(CQ[0], 4)}, v117")
    for u in range(NT):
        if (u & 3) == 0 and u + 4 < NT:
            b(f"ds_read_b128 {vreg(CQ[((u >> 2) + 1) & 1], 4)}, v117 offset:{16 * ((u >> 2) + 1)}")
        if (u & 3) == 0:
            n_new = 0
            for k in range(4):
                v = u + 8 + D + k
                if v < NV:
                    b(f"ds_read_b64 {RING(v)}, {vreg(P[v & 3])} offset:{PH0 + 8 * (v >> 2)}")
                    n_new += 1
            # everything older than this group's own loads (taps of the next group + four samples) must have arrived
            b(f"s_waitcnt lgkmcnt({n_new + (1 if u + 4 < NT else 0)})")
        ca = CQ[(u >> 2) & 1]
        hp = vreg(ca + (2 if (u & 2) else 0), 2)
        sel = "op_sel:[0,1,0] op_sel_hi:[1,1,1]" if (u & 1) else "op_sel:[0,0,0] op_sel_hi:[1,0,1]"
        for j in range(3):
            b(f"v_pk_fma_f32 {ACC[j]}, {RING(u + 4 * j)}, {hp}, {ACC[j]} {sel}")


def c_string(lines):
    out = []
    for t in lines:
        out.append('\t"' + t.replace("\\", "\\\\").replace('"', '\\"') + '\\n\\t"')
    return "\n".join(out)


def main(out=OUT):
    sys.path.insert(0, ROOT)
    # LDS layout of the kernel's tables (must match trx_kernel_nb.hip; the kernel static_asserts these numbers)
    SINCV_LDS = 4096 + 32
    gdec_off = (SINCV_LDS + 16 * 64 + 65 * 36) * 4
    NB_TABLES_END_OLD = SINCV_LDS + 16 * 64 + 65 * 36 + 16 + 64 + 5 * 64 + 5 * 64      # floats in front of the training-sequence taps
    blocks = {}
    lseq_off = NB_TABLES_END_OLD * 4
    blocks["DECCORR"], dc_paths = block_deccorr(gdec_off, lseq_off)
    wa4_off = SINCV_LDS * 4
    blocks["DETA"], da_cold = block_deta(wa4_off)
    blocks["DETB"], db_cold = block_detb()
    blocks["TAIL"], tl_cold = block_tail()
    blocks["FIRG"] = block_firg()
    # the rare sides of DETA, DETB and TAIL: one statement behind the burst loop, jumped over where it lies.  It is entered from
    # and left for labels inside those blocks, so it may name fixed registers only -- no %[operand]
    cold = Block("COLD")
    cold.ins = ["s_branch .Lnbc_end"] + da_cold.ins + db_cold.ins + tl_cold.ins + [".Lnbc_end:"]
    assert not any("%[" in t for t in cold.ins)
    blocks["COLD"] = cold

    def with_cold(b, c):
        """the hazard checker's view of a block and its cold part: the cold code in front of the block's last label, jumped over
        (the order the two had as one statement; check_paths() then follows every branch into it)"""
        v = Block(b.name, [n[2:-1] for n in b.sgpr_ops])
        assert b.ins[-1].endswith("_end:")
        v.ins = b.ins[:-1] + ["s_branch " + b.ins[-1][:-1]] + c.ins + [b.ins[-1]]
        v.exec_ok = getattr(b, "exec_ok", ())
        return v
    errs = [e for p in dc_paths for e in p.check()] + \
        check_paths(with_cold(blocks["DETA"], da_cold)) + check_paths(with_cold(blocks["DETB"], db_cold)) + \
        check_paths(with_cold(blocks["TAIL"], tl_cold)) + check_paths(blocks["FIRG"])
    # no jump over cold code: cold labels (.Lnbc_*) lie behind the loop or in the shadow of DECCORR's computed jump only
    for name in ("DETA", "DETB", "TAIL"):
        errs += [f"{name}: cold label {t} inside a block of the main path" for t in blocks[name].ins if t.startswith(".Lnbc_")]
    dc = blocks["DECCORR"].ins
    i_pc, i_v0 = min(i for i, t in enumerate(dc) if t.startswith("s_setpc_b64")), dc.index(".Lnb_corrr_v0:")
    errs += [f"DECCORR: cold label {t} outside the computed jump's shadow" for i, t in enumerate(dc)
             if t.startswith(".Lnbc_") and not i_pc < i < i_v0]
    hdr = ["// trx_nb_asm.inc -- GENERATED by tools/gen_nb_asm.py (hazards and LDS waits checked there); do not edit.",
           f"#define NB_ASM_GDEC_OFF {gdec_off}",
           f"#define NB_ASM_LSEQ_OFF {lseq_off}",
           f"#define NB_ASM_DEC_MAX_NACT {DEC_MAX_NACT}",
           f"#define NB_ASM_CORR_LANE0 {CORR_LANE0}",
           f"#define NB_ASM_CORR_MAX_LEN {CORR_MAX_LEN}",
           f"#define NB_ASM_AW_PD {AW_PD}",
           f"#define NB_ASM_AW_D {AW_D}",
           f"#define NB_ASM_AW_CZ {AW_CZ}",
           f'#define NB_ASM_ST "{{{ST}}}"',
           "#define NB_ASM_CLOBBERS " + ", ".join(f'"v{i}"' for i in range(64, 128)) + ", " +
           ", ".join(f'"s{i}"' for i in range(87, 100)) + ', "vcc", "scc", "memory"',
           # (DETA, DETB: the status register is an output there)
           "#define NB_ASM_CLOBBERS_ST " + ", ".join(f'"v{i}"' for i in range(64, 128)) + ", " +
           ", ".join(f'"s{i}"' for i in range(87, 100) if f"s{i}" != ST) + ', "vcc", "scc", "memory"']
    for name, b in blocks.items():
        hdr.append(f"#define NB_ASM_{name} \\")
        lines = b.text()
        hdr.append(" \\\n".join('\t"' + t + '\\n\\t"' for t in lines))
    # AMAX is parameterised by the caller's fillers: emitted as a function-like macro
    fill = [f"FILL{i}" for i in range(8)]
    am = block_amax([f"@@{i}@@" for i in range(8)])
    chk = block_amax(["s_nop 0"] * 8)
    errs += chk.check()
    hdr.append("#define NB_ASM_AMAX(" + ", ".join(fill) + ") \\")
    body = []
    for t in am.text():
        m = re.match(r"^@@(\d)@@$", t)
        if m:
            body.append(f"\tFILL{m.group(1)} \"\\n\\t\"")
        else:
            body.append('\t"' + t + '\\n\\t"')
    hdr.append(" \\\n".join(body))
    if errs:
        print("\n".join(errs))
        sys.exit(1)
    open(out, "w").write("\n".join(hdr) + "\n")
    print("wrote", os.path.relpath(out, ROOT), {k: len([t for t in b.text() if Block.parse(t)]) for k, b in blocks.items()})


if __name__ == "__main__":
    main(*sys.argv[1:2])
