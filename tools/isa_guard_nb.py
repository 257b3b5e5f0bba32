#!/usr/bin/env python3
"""What the compiler made of the normal-burst kernel's burst loop (csrc/trx_kernel_nb.hip), checked on its assembly:

    python tools/isa_guard_nb.py [--keep out.s]

The loop is C++ around hand-placed blocks, and twice in round 6 a harmless-looking source change made hipcc put
`s_waitcnt vmcnt(0)` between the next burst's prefetch loads (an exec-masked tenth load; a 64-bit vector address built in
one of the destination registers) -- 3-4 % of the headline each time, invisible to every test.  Checked here (and by
tests/test_isa_guard_cpu.py on every CPU run):
  * the ten prefetch loads of the loop (and of every copy on its out-of-line paths) are issued back to back: no s_waitcnt between
    the first and the last of them; one group lies on the loop's main path;
  * the work ticket is taken with a partial wait (lgkmcnt(5)), not a drain of the converted samples' LDS writes;
  * no spills, no scratch, 128 VGPRs (4 waves per SIMD), and the code size.
  * the stores of flush_records() do not lie on the loop's main path (they belong behind it: once per 64 bursts).
  * what depends only on the lane and the wave is made once in front of the loop (the kernel's a_p, a_w, a_l4, ...): the main path
    outside the hand-placed blocks holds no lane id (v_mbcnt_*) and none of the integer multiplies that addresses were built
    with per burst (v_mul_lo_u32, v_mad_u64_u32, v_mul_u32_u24).
  * the common burst's path through the loop, blocks included, executes at most 22 branch instructions, at most 3 of them taken
    (block CORR's computed jump, its variant's exit, the back edge), and no cold code lies on it between a block's entry and
    its exit (tools/gen_nb_asm.py: labels .Lnbc_*): the main path falls through every block.
Reported, not checked: the static instruction and vector-instruction counts of the main path outside the hand-placed blocks,
its branches outside and inside them (branches_outside_blocks, branches_inside_blocks), the taken ones (taken_on_main_path).
Prints a JSON summary; exit status 1 on a violation."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from osmo_trx_amd import build as B   # noqa: E402

KERNEL = "_Z15nb_pull4_kernel"
# per-lane work that belongs in front of the loop: the lane id and the slow integer multiplies of address arithmetic
LANE_ONLY = re.compile(r"\s*(v_mbcnt_\w+|v_mul_lo_u32|v_mad_u64_u32|v_mul_u32_u24)\w*\s")


def assembly(keep=None):
    out = keep or os.path.join(tempfile.mkdtemp(prefix="isa_guard_"), "k4.s")
    flags = [f for f in B.COMMON if not f.startswith("-W")]
    subprocess.run([B.HIPCC, "--offload-arch=gfx950"] + flags + ["-w", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    "-o", out, os.path.join(B.CSRC, "trx_kernel4.hip")], check=True, capture_output=True)
    return open(out).read()


def check(text):
    lines = text.splitlines()
    start = next(i for i, t in enumerate(lines) if re.match(KERNEL + r"\w*:", t))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    errs = []
    # ---- the prefetch of the loop: the LAST run of non-temporal dword loads (the first one is in front of the loop)
    nt = [i for i, t in enumerate(body) if re.match(r"\s*global_load_dword v\d+, .* nt\s*$", t)]
    groups, cur = [], []
    for i in nt:
        if cur and i - cur[-1] > 8:
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    # (every group behind the first: the loop's own prefetch and the copies on its out-of-line paths -- the foreign slot, the
    # pool boundary -- wherever the layout puts them)
    if len(groups) < 2 or any(len(g) != 10 for g in groups[1:]):
        errs.append(f"expected groups of 10 non-temporal prefetch loads behind the first, found groups of {[len(g) for g in groups]}")
    for g in groups[1:] if len(groups) >= 2 else []:
        if len(g) != 10:
            continue
        between = [body[i].strip() for i in range(g[0], g[-1]) if "s_waitcnt" in body[i]]
        # and in front of the group, behind the address arithmetic: a wait for vmcnt(0) there stalls on the stores just issued
        before = [body[i].strip() for i in range(max(0, g[0] - 12), g[0]) if re.search(r"s_waitcnt.*vmcnt\(0\)", body[i])]
        if between:
            errs.append(f"s_waitcnt between the loop's prefetch loads (line {g[0]}): {between}")
        if before:
            errs.append(f"s_waitcnt vmcnt(0) right in front of the loop's prefetch loads (line {g[0]}): {before}")
        if any(re.search(r"v\[\d+:\d+\], off", body[i]) for i in g):
            errs.append(f"prefetch loads with a 64-bit vector address (line {g[0]}; expected the scalar-base form)")
    if not any(re.search(r"s_waitcnt lgkmcnt\(5\)", t) for t in body):
        errs.append("no `s_waitcnt lgkmcnt(5)`: the work ticket is taken behind a full drain of the LDS")
    # ---- resources (the kernel's metadata record)
    md = text[text.index(".name:           " + KERNEL):]
    md = md[:md.index("  - .agpr_count") if "  - .agpr_count" in md else len(md)]
    res = {k: int(re.search(rf"\.{k}:\s+(\d+)", md).group(1)) for k in
           ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")}
    if res["sgpr_spill_count"] or res["vgpr_spill_count"] or res["private_segment_fixed_size"]:
        errs.append(f"spills / scratch: {res}")
    if res["vgpr_count"] > 128:
        errs.append(f"{res['vgpr_count']} VGPRs: fewer than 4 waves per SIMD")
    n_ins = sum(1 for t in body if re.match(r"\s+[a-z_0-9]+(\s|$)", t) and not t.strip().startswith((".", ";")))
    rep = loop_report(body)
    main = rep["loop_main_path"]
    if main is None:
        errs.append("the burst loop's main path was not found (the ticket's ds_add_rtn_u32 .. a branch back to the loop's head)")
    else:
        # the join blocks that keep the loop's carried state in scalar registers are empty asm statements: a compiler that folds
        # them away brings flush_records() back into the loop, and with it the masks
        if main["flush_records_stores_on_it"]:
            errs.append("flush_records' stores lie on the loop's main path")
        if not any(all(i in main["lines"] for i in g) for g in groups[1:]):
            errs.append("no prefetch group on the loop's main path")
        # jumps and tests: the common burst executes at most MAX_BRANCHES branch instructions, MAX_TAKEN of them taken (block CORR's
        # computed jump, its variant's exit, the back edge), and falls through every block -- no cold code inside one to jump over
        if main["branches"] > MAX_BRANCHES:
            errs.append(f"{main['branches']} branch instructions on the loop's main path (at most {MAX_BRANCHES})")
        if main["taken_on_main_path"] > MAX_TAKEN:
            errs.append(f"{main['taken_on_main_path']} taken branches on the loop's main path (at most {MAX_TAKEN}): {main['taken']}")
        if main["cold_labels_inside_blocks"]:
            errs.append(f"cold code on the loop's main path, between a block's entry and its exit: {main['cold_labels_inside_blocks']}")
        main["lines"] = len(main["lines"])
        if main["lane_only_work_on_it"]:
            errs.append(f"per-lane constants are rebuilt on the loop's main path: {main['lane_only_work_on_it']}")
    return errs, {"kernel": "nb_pull4_kernel", **res, "instructions": n_ins,
                  "prefetch_groups": [len(g) for g in groups], **rep}


COLD_LABEL = re.compile(r"(\.Lnbc_\w+|\.Lnb_(dec_wide|corr_wide|corr\w_mul|corr\w_join|da_careful|da_unsure|da_wait_end|db_careful|db_unsure|"
                        r"tl_wait_end)):")
MAX_BRANCHES, MAX_TAKEN = 22, 3


def loop_report(body):
    """The burst loop's main path AS EXECUTED by the common burst -- a normal-burst slot, detected, every decision certified,
    straight-line geometry, a narrow window, training sequence 0 -- walked from the loop header's label (the last one in front of
    the work ticket's request, the kernel's first ds_add_rtn_u32): a conditional branch falls through, the jumps whose target is
    known statically are followed (s_branch; block CORR's s_setpc_b64, to its first variant), and the walk ends at the first branch
    to a label at the loop's head, the back edge.  Reported: the path's instructions, vector instructions and branches outside every
    `asm` statement of the source (valu_outside_blocks: the short asm statements of the source -- the clip scan's v_max3, the
    record's moves -- count, a statement that names one of the blocks' fixed registers v64..v127 does not), its branches inside
    the statements, how many of all its branches are taken, the cold labels the path falls into (tools/gen_nb_asm.py: .Lnbc_*; those in the shadow of block CORR's computed jump are not
    on it),
    whether flush_records' 16-byte stores lie on it, and what it holds of per-lane work that belongs in front of the loop."""
    try:
        ticket = next(i for i, t in enumerate(body) if "ds_add_rtn_u32" in t)
        head = max(i for i in range(ticket) if re.match(r"\.LBB\d+_\d+:", body[i]))
    except (StopIteration, ValueError):
        return {"loop_main_path": None}
    where = {m.group(1): i for i, t in enumerate(body) for m in [re.match(r"(\.\w+):", t.strip())] if m}

    def reaches_head(i):
        """a label of the loop's head: from it the header is reached by a few scalar moves and waits (the copies of the carried
        state), wherever the layout put them -- in front of the header, or out of line with a jump to it"""
        for _ in range(32):
            if i is None or i >= len(body):
                return 0
            if i == head:
                return 1
            m = re.match(r"\s*(s_c?branch\w*|s_setpc_b64|s_endpgm)\s*(\S*)", body[i])
            if m and m.group(1) != "s_branch":
                return 0
            i = where.get(m.group(2)) if m else i + 1
        return 0
    labels = {l for l, i in where.items() if re.match(r"\.LBB\d+_\d+$", l) and reaches_head(i)}
    in_asm, ins, valu, lane_only, stmt = False, 0, 0, [], []
    br_out, br_in, taken, cold, visited, back = 0, 0, [], [], set(), None

    def short_stmt():
        nonlocal valu
        if not any(re.search(r"\bv(6[4-9]|[7-9]\d|1[01]\d|12[0-7])\b|\bv\[(6[4-9]|[7-9]\d|1[01]\d|12[0-7]):", t) for t in stmt):
            valu += sum(1 for t in stmt if re.match(r"\s*v_", t))
            lane_only.extend(t.strip() for t in stmt if LANE_ONLY.match(t))

    i = head
    while back is None and i < len(body) and i not in visited:
        t = body[i]
        visited.add(i)
        nxt = i + 1
        if "#ASMSTART" in t:
            in_asm, stmt = True, []
        elif "#ASMEND" in t:
            short_stmt()
            in_asm = False
        elif COLD_LABEL.match(t.strip()):                          # the path falls into (or through) cold code
            cold.append(t.strip()[:-1])
        elif re.match(r"\s+[a-z_0-9]+(\s|$)", t) and not t.strip().startswith((".", ";")):
            m = re.match(r"\s*(s_cbranch_\w+|s_branch|s_setpc_b64)\s+(\S+)", t)
            if in_asm:
                stmt.append(t)
            else:
                ins += 1
                valu += bool(re.match(r"\s*v_", t))
                if LANE_ONLY.match(t):
                    lane_only.append(t.strip())
            if m:
                br_in += in_asm
                br_out += not in_asm
                if m.group(1) == "s_setpc_b64":                   # the computed jump of block CORR: its first variant
                    nxt = next((k for k in range(i, len(body)) if re.match(r"\.Lnb_corr\w*_v0:", body[k].strip())), None)
                    taken.append(t.strip())
                elif m.group(2) in labels:
                    back = i
                    taken.append(t.strip())
                    # (copies of the carried state that the layout put out of line reach the header by a jump of their own)
                    k = where[m.group(2)]
                    while k != head:
                        mm = re.match(r"\s*s_branch\s+(\S+)", body[k])
                        if mm:
                            br_out += 1
                            taken.append(body[k].strip())
                        k = where[mm.group(1)] if mm else k + 1
                elif m.group(1) == "s_branch":
                    nxt = where.get(m.group(2))
                    taken.append(t.strip())
                if nxt is None:
                    break
        i = nxt
    if back is None:
        return {"loop_main_path": None}
    return {"loop_main_path": {"first": head, "last": back, "instructions_outside_blocks": ins, "valu_outside_blocks": valu,
                               "branches_outside_blocks": br_out, "branches_inside_blocks": br_in, "branches": br_out + br_in,
                               "taken_on_main_path": len(taken), "taken": taken, "cold_labels_inside_blocks": cold,
                               "lane_only_work_on_it": lane_only,
                               "flush_records_stores_on_it": any("global_store_dwordx4" in body[k] for k in visited),
                               "lines": sorted(visited)}}


def main():
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    errs, info = check(assembly(keep))
    info["violations"] = errs
    print(json.dumps(info, indent=1))
    return 1 if errs else 0


if __name__ == "__main__":
    sys.exit(main())
