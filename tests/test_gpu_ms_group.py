"""GPU tests of the MS-side scheduler group (trxhip_ms_group_*, osmo_trx_amd.MsRxSchedulerGroup).

Every comparison is equality.  A member of a group is one trxhip_ms_sched: the group form of the receiver is the stream form's
body behind a table lookup, and the plan is the single object's planner, so a group pull must equal the pulls of N single
objects on the same chunks byte for byte -- indications, sbits, plan, state and clock -- and leave every output row it does not
own as it found it.  With tracking on the cutter is compared with the literal model (tests/ms_sched_model.py) fed with the
device's own SCH starts: the model is the yardstick, not the group."""
import ctypes as C

import numpy as np
import pytest

import ms_group_cases as GC
import ms_rx_cases as K
import ms_sched_cases as SC
import ms_sched_model as SM
from osmo_trx_amd import trxhip

pytestmark = pytest.mark.gpu

EINVAL = -22
N_FRAMES = 12
# five cells: seed, fn0, bsic (tsc = bsic & 7), late, lead, active mask, tracking, slots of the stream left out in front.
# Every stream of 12 frames holds two SCH bursts.
# Members 3 and 4 begin 3 slots into a frame whose successor carries the SCH burst (fn0 % 51 == 0): cutting 5 slots and 75 samples
# leaves the SCH slot (fn0 + 1, 0) straddling the next chunk.
CELLS = [
    dict(seed=4300, fn0=51 * 600, bsic=0o31, late=0, lead=0, active=0b11011011, tracking=True, skip=0),
    dict(seed=4301, fn0=51 * 40 + 10, bsic=0o52, late=3, lead=0, active=0b00100101, tracking=True, skip=0),
    dict(seed=4302, fn0=51 * 9 + 41, bsic=0o17, late=3, lead=1, active=0xFF, tracking=False, skip=0),
    dict(seed=4303, fn0=51 * 77, bsic=0o04, late=0, lead=2, active=0b10000001, tracking=True, skip=3),
    dict(seed=4304, fn0=51 * 7, bsic=0o66, late=0, lead=0, active=0b01111110, tracking=True, skip=3),
]
CYCLE = [5300, 700, 6000, 1875, 1250, 4999, 3333]              # (>= 700: a correction never pushes the cut out of a chunk)
# the first pulls of the two chunkings, per member (0: no chunk); then CYCLE, rotated per member, to the end of every stream.
# A, pull 0 (no partial slots yet): 9, 0 (a chunk shorter than a slot: a join and no receiver work), 4, 5 and 1 slots;
#    pull 1: member 3's straddling slot is the SCH slot and is demodulated first, the straddling slots of members 0 and 2 are
#            not; member 1's chunk only extends its partial slot; member 4 has no chunk
# B, pull 0: 9, 0, 1, 4 and 5 slots; pull 1: member 4 in member 3's role; pull 2: member 0's chunk only extends its partial slot
FIRST = {
    "A": [[6000, 300, 2600, 3200, 700], [700, 100, 3025, 5300, 0], [6000, 6000, 2500, 0, 3000]],
    "B": [[6000, 300, 700, 2600, 3200], [0, 700, 650, 3000, 5300], [100, 3000, 0, 700, 1300]],
}


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


@pytest.fixture(scope="module")
def cells():
    """per member the int16 stream from its first pulled slot on and the clock in front of it"""
    out = []
    for c in CELLS:
        x = SC.cell_stream(c["seed"], c["fn0"], N_FRAMES, c["bsic"], tsc=c["bsic"] & 7, late=c["late"], lead=c["lead"])[0]
        x = np.ascontiguousarray(x[c["skip"] * 625:])
        k = c["skip"] - 1
        clock = (c["fn0"] + k // 8, k % 8, -625) if c["skip"] else (c["fn0"] - 1, 7, -625)
        out.append(dict(c, x=x, clock=clock, tsc=c["bsic"] & 7))
    return out


def _dev(x, cf32):
    import torch
    if cf32:
        return torch.from_numpy((x[:, 0].astype(np.float32) + 1j * x[:, 1].astype(np.float32)).astype(np.complex64)).to("cuda:0")
    return torch.from_numpy(x).to("cuda:0")


def _schedule(cells, which):
    """[[(at, n) or None per member] per pull]"""
    at = [0] * len(cells)
    left = [len(c["x"]) for c in cells]
    rows, k = [], 0
    while any(left):
        row = []
        for m, c in enumerate(cells):
            n = FIRST[which][k][m] if k < len(FIRST[which]) else CYCLE[(k + 2 * m + (which == "B")) % len(CYCLE)]
            if n > left[m]:                                        # the stream's end: a last chunk of at least 700 samples, or none
                n = left[m] if left[m] >= 700 else 0
                left[m] = n
            row.append((at[m], n) if n else None)
            at[m] += n
            left[m] -= n
        if any(row):
            rows.append(row)
        k += 1
    return rows


def _make_group(trx, cells, tracking=None):
    g = trxhip.MsRxSchedulerGroup(trx, n=len(cells), rx_full_scale=SC.FULL, tsc=[c["tsc"] for c in cells],
                                  active_tns=[c["active"] for c in cells],
                                  tracking=[c["tracking"] for c in cells] if tracking is None else tracking)
    for m, c in enumerate(cells):
        g.set_clock(m, *c["clock"])
    return g


def _run_group(trx, cells, d_x, rows, stride=14):
    """the group over the schedule; per pull and member (ind bytes, sbits bytes, plan bytes, state bytes, clock) or None"""
    import torch
    g = _make_group(trx, cells)
    n = len(cells)
    out = []
    for row in rows:
        ind = torch.full((n, stride, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
        bits = torch.full((n, stride, 148), 0x5A, dtype=torch.int8, device="cuda:0")
        chunks = [d_x[m][r[0]:r[0] + r[1]] if r else None for m, r in enumerate(row)]
        views, counts = g.pull(chunks, first_ts=[r[0] if r else 0 for r in row], out=(ind, bits))
        h_ind, h_bits = ind.cpu().numpy(), bits.cpu().numpy()
        res = []
        for m, r in enumerate(row):
            k = counts[m]
            assert (h_ind[m, k:] == 0xAB).all() and (h_bits[m, k:] == 0x5A).all(), (m, k)     # rows the member does not own
            assert views[m][0].shape[0] == k
            res.append((h_ind[m, :k].tobytes(), h_bits[m, :k].tobytes(), g.plan(m, k), g.state(m).tobytes(), g.clock(m)) if r else None)
            if not r:
                assert k == 0
        out.append(res)
    g.close()
    return out


def _run_singles(trx, cells, d_x, rows):
    ss = [trxhip.MsRxScheduler(trx, rx_full_scale=SC.FULL, tsc=c["tsc"], active_tns=c["active"], tracking=c["tracking"]) for c in cells]
    for s, c in zip(ss, cells):
        s.set_clock(*c["clock"])
    out = []
    for row in rows:
        res = []
        for m, r in enumerate(row):
            if not r:
                res.append(None)
                continue
            i, b = ss[m].pull(d_x[m][r[0]:r[0] + r[1]], first_ts=r[0])
            res.append((i.cpu().numpy().tobytes(), b.cpu().numpy().tobytes(), ss[m].plan(), ss[m].state().tobytes(), ss[m].clock()))
        out.append(res)
    for s in ss:
        s.close()
    return out


def _same(a, b):
    return a is None and b is None or (a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes() and a[3:] == b[3:])


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("cf32", [False, True])
def test_group_equals_single_objects_byte_for_byte(trx, cells, cf32, which):
    """5 members on their own cells (seed, fn0, bsic / tsc, late, lead and ACTIVE mask differ; member 2 has tracking off) against 5
    MsRxScheduler objects on the same chunks: after every pull and for every member the indication bytes, all 148 sbits per slot,
    plan(), state() and clock() are equal, and the output rows behind a member's count keep the pattern written before the pull.
    Within one group pull members cut 0, 1, 4, 5 and >= 9 slots, some straddle and some do not, and one member's straddling slot
    is an SCH slot (demodulated first) while another's is not."""
    d_x = [_dev(c["x"], cf32) for c in cells]
    rows = _schedule(cells, which)
    got, want = _run_group(trx, cells, d_x, rows), _run_singles(trx, cells, d_x, rows)
    counts_seen = mixed_straddle = prelim_beside = False
    for k, (g_row, s_row) in enumerate(zip(got, want)):
        for m, (a, b) in enumerate(zip(g_row, s_row)):
            assert _same(a, b), (k, m)
        plans = [r[2] for r in g_row if r is not None]
        counts = sorted(len(p) for p in plans)
        counts_seen |= len(plans) == 5 and counts[:4] == [0, 1, 4, 5] and counts[4] >= 9
        straddles = [len(p) > 0 and p[0]["src_off"] < 0 for p in plans]
        mixed_straddle |= any(straddles) and not all(straddles)
        sch_first = [m for m, r in enumerate(g_row) if r is not None and len(r[2]) and r[2][0]["src_off"] < 0 and cells[m]["tracking"]
                     and r[2][0]["kind"] == trxhip.MS_KIND_SCH]
        other = [m for m, r in enumerate(g_row) if r is not None and len(r[2]) and r[2][0]["src_off"] < 0
                 and r[2][0]["kind"] != trxhip.MS_KIND_SCH]
        prelim_beside |= bool(sch_first) and bool(other)
    assert counts_seen and mixed_straddle and prelim_beside
    total = sum(len(r[2]) for row in got for r in row if r is not None)
    assert total >= 5 * (N_FRAMES * 8 - 8)


def test_a_member_does_not_depend_on_the_others(trx, cells):
    """Member 0's outputs, plan, state and clock are the same when the other members' chunks hold other streams, and when the
    other members have no chunks at all."""
    d_x = [_dev(c["x"], False) for c in cells]
    rows = _schedule(cells, "A")
    base = [row[0] for row in _run_group(trx, cells, d_x, rows)]
    swapped = [d_x[0]] + [d_x[1 + (m % 4)] for m in range(1, 5)]   # members 1..4 read the streams of members 2, 3, 4, 1
    lens = [len(cells[0]["x"])] + [len(cells[1 + (m % 4)]["x"]) for m in range(1, 5)]
    rows_sw = [[r if r is None or r[0] + r[1] <= lens[m] else None for m, r in enumerate(row)] for row in rows]
    rows_sw = [row for row in rows_sw if any(r is not None for r in row)]
    other = [row[0] for row in _run_group(trx, cells, swapped, rows_sw)]
    alone = [row[0] for row in _run_group(trx, cells, d_x, [[row[0]] + [None] * 4 for row in rows if row[0] is not None])]
    mine = [r for r in base if r is not None]
    assert len(mine) == len(alone) >= 10 and all(_same(a, b) for a, b in zip(mine, alone))
    assert all(_same(a, b) for a, b in zip(mine, [r for r in other if r is not None])) and len([r for r in other if r is not None]) == len(mine)


@pytest.mark.parametrize("sizes", [[5300], [20000, 700, 6000]])
def test_tracking_follows_the_model(trx, cells, sizes):
    """Members 0 .. 3 with tracking on, bursts 3 samples late on members 1 and 2 and on time on the others: after every group pull
    plan, to_skip, pending, carried and clock of every member equal ms_sched_model fed with the device's own starts."""
    four = cells[:4]
    d_x = [_dev(c["x"], False) for c in four]
    g = _make_group(trx, four, tracking=True)
    got = [dict() for _ in four]
    models = []
    for m, c in enumerate(four):
        models.append(SM.Cutter(lambda fn, tn, ts, m=m: got[m][fn], tracking=True))
        models[m].set_clock(*c["clock"])
    at = [0] * 4
    k = 0
    starts = [[] for _ in four]
    left = [len(c["x"]) for c in four]
    while any(left):
        ns = [min(sizes[(k + m) % len(sizes)], left[m]) for m in range(4)]
        ns = [n if n >= 700 else 0 for n in ns]                    # (a shorter tail is left unpulled: a correction could leave it)
        left = [v - n if n else 0 for v, n in zip(left, ns)]
        if not any(ns):
            break
        bounds = [g.slots(m, n) if n else 0 for m, n in enumerate(ns)]
        views, counts = g.pull([d_x[m][at[m]:at[m] + n] if n else None for m, n in enumerate(ns)], first_ts=at)
        for m, n in enumerate(ns):
            if not n:
                continue
            ind, p = g.ind_to_numpy(views[m][0]), g.plan(m)
            assert len(p) == counts[m] <= bounds[m]
            for r in ind:
                if r["kind"] == trxhip.MS_KIND_SCH:
                    got[m][int(r["fn"])] = int(r["start"]) if r["sch_rc"] == 1 else None
                    starts[m].append(int(r["start"]))
            want = models[m].grab_bursts(at[m], n)
            assert [(int(q["fn"]), int(q["tn"]), int(q["ts"]), int(q["src_off"])) for q in p] == want, (k, m)
            st, mod = g.state(m), models[m]
            assert (st["to_skip"], st["pending"], st["carried"]) == (mod.to_skip, mod.temp_ts_corr_offset, mod.partial_rdofs), (k, m)
            assert g.clock(m) == (mod.tk.fn, mod.tk.tn, mod.tk.ts) and st["clock_jumps"] == 0
            at[m] += n
        k += 1
    g.close()
    # the late members measured their offset (the receiver's zero lies 2 samples behind a burst's first sample) and followed it
    for m in (1, 2):                                               # 2 + late + lead
        assert abs(starts[m][0] - (5 + four[m]["lead"])) <= 1 and abs(starts[m][-1]) <= 1, starts[m]
    assert all(len(s) == 2 for s in starts)


def test_batched_acquire_then_pull_loopback(trx):
    """Three members on the cells of tests/ms_group_cases.py (tests/test_ms_group_cpu.py checks the precondition on the CPU
    models): one acquire over the three buffers finds the cells of members 0 and 2 and reports member 1 (noise) as not found and
    leaves it untouched; the two then return the FN sent, the bits sent in every ACTIVE traffic slot and the SCH slot's FN."""
    import torch
    Ls = GC.LOOPS
    xs, sents = zip(*[GC.loop_stream(L) for L in Ls])
    d_x = [_dev(x, False) for x in xs]
    g = trxhip.MsRxSchedulerGroup(trx, n=3, rx_full_scale=SC.FULL, tsc=0, active_tns=[L["active"] for L in Ls], tracking=True)
    before = g.state(1).tobytes()
    bufs = torch.stack([d[:60000] for d in d_x]).contiguous()
    found, rec = g.acquire([0, 1, 2], bufs, first_ts=[L["t0"] for L in Ls])
    assert list(found) == [True, False, True] and rec["rc"][1] == 0
    assert g.state(1).tobytes() == before and g.state(1)["clock_set"] == 0
    for m in (0, 2):
        L = Ls[m]
        assert (rec[m]["rc"], rec[m]["fn"], rec[m]["bsic"]) == (1, L["fn0"] + 7, L["bsic"]) and g.clock(m) == (L["fn0"] + 7, 0, 0)
        st = g.state(m)
        assert st["tsc"] == L["tsc"] and st["first_call"] == 1 and st["first_sch_ts_start"] == L["t0"] + int(rec[m]["start"]) - 17
    # the same buffers as complex64, members in another order: the same records
    g2 = trxhip.MsRxSchedulerGroup(trx, n=3, rx_full_scale=SC.FULL)
    bufs_f = torch.stack([_dev(xs[m][:60000], True) for m in (2, 0)]).contiguous()
    found2, rec2 = g2.acquire([2, 0], bufs_f, first_ts=0)
    assert found2.all() and rec2[0].tobytes() == rec[2].tobytes() and rec2[1].tobytes() == rec[0].tobytes()
    g2.close()
    at = [60000] * 3
    n_traffic, n_sch = [0] * 3, [0] * 3
    for k in range(3):
        chunks = [None if m == 1 else d_x[m][at[m]:at[m] + Ls[m]["chunks"][k]] for m in range(3)]
        views, counts = g.pull(chunks, first_ts=[Ls[m]["t0"] + at[m] for m in range(3)])
        assert counts[1] == 0
        for m in (0, 2):
            L = Ls[m]
            ind, bits = g.ind_to_numpy(views[m][0]), views[m][1].cpu().numpy()
            for r, hard in zip(ind, bits):
                key = (int(r["fn"]), int(r["tn"]))
                if r["kind"] == trxhip.MS_KIND_NB and r["sent"]:
                    assert np.array_equal(hard, K.hard(sents[m][key])), (m, key)
                    n_traffic[m] += 1
                elif r["kind"] == trxhip.MS_KIND_NB:
                    assert not hard.any() and not (L["active"] >> key[1]) & 1
                elif r["kind"] == trxhip.MS_KIND_SCH:
                    assert (r["sch_rc"], r["sch_fn"], r["sch_bsic"]) == (1, key[0], L["bsic"])
                    n_sch[m] += 1
            at[m] += chunks[m].shape[0]
    assert n_traffic == [48, 0, 46] and n_sch == [1, 0, 1]
    assert all(g.state(m)["clock_jumps"] == 0 and g.state(m)["slots"] == 96 for m in (0, 2)) and g.state(1).tobytes() == before
    g.close()


def test_a_group_of_one_equals_the_single_object(trx, cells):
    one = cells[1:2]
    d_x = [_dev(one[0]["x"], False)]
    rows = _schedule(one, "A")
    got, want = _run_group(trx, one, d_x, rows), _run_singles(trx, one, d_x, rows)
    assert len(got) >= 10 and all(_same(a[0], b[0]) for a, b in zip(got, want))


def test_refusals_leave_every_member_and_the_outputs_untouched(trx):
    import torch
    L = trx.L
    vp = C.c_void_p
    x = torch.zeros((3, 4000, 2), dtype=torch.int16, device="cuda:0")
    xf = torch.zeros((3, 4000), dtype=torch.complex64, device="cuda:0")
    ind = torch.full((3, 8, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    bits = torch.full((3, 8, 148), 0x5A, dtype=torch.int8, device="cuda:0")
    st = trx._stream()
    h = vp()
    cfgs = (trxhip._MsSchedCfg * 2)(trxhip._MsSchedCfg(SC.FULL, 0, 0xFF, 0, 0), trxhip._MsSchedCfg(SC.FULL + 1, 0, 0xFF, 0, 0))
    assert L.trxhip_ms_group_create(trx.h, SC.FULL, 2, C.cast(cfgs, vp), C.byref(h)) == EINVAL
    assert L.trxhip_ms_group_create(trx.h, SC.FULL, 0, C.cast(cfgs, vp), C.byref(h)) == EINVAL
    g = trxhip.MsRxSchedulerGroup(trx, n=3, rx_full_scale=SC.FULL, tsc=2, tracking=False)
    ns, nc = (C.c_size_t * 3)(), (C.c_size_t * 3)()
    bad = C.c_int(-7)

    def pull(fn, ptrs, sizes, d_ind=None, d_bits=None, stride=8):
        ch = np.zeros(3, dtype=trxhip.MS_GROUP_CHUNK_DTYPE)
        ch["d_in"], ch["n_samples"], ch["first_ts"] = ptrs, sizes, 0
        return fn(g.h, ch.ctypes.data_as(vp), vp(ind.data_ptr()) if d_ind is None else d_ind, vp(bits.data_ptr()) if d_bits is None else d_bits,
                  stride, C.cast(ns, vp), C.cast(nc, vp), C.byref(bad), st)

    p16, pf = L.trxhip_ms_group_pull_s16, L.trxhip_ms_group_pull_cf32
    P = [x[m].data_ptr() for m in range(3)]
    PF = [xf[m].data_ptr() for m in range(3)]
    assert pull(p16, P, [700, 700, 700]) == EINVAL and bad.value == 0      # before set_clock or a successful acquire
    assert L.trxhip_ms_group_feed_starts(g.h, 0, None, 0) == EINVAL        # a device group takes its starts from the device
    for m in range(3):
        g.set_clock(m, 7, 7, -625)
    assert pull(p16, P, [700, 700, 700]) == 0 and list(ns) == [1, 1, 1] and list(nc) == [75, 75, 75] and bad.value == -1
    torch.cuda.synchronize()
    ind.fill_(0xAB)
    bits.fill_(0x5A)
    before = [(g.state(m).tobytes(), g.clock(m), g.plan(m, 1).tobytes()) for m in range(3)]
    calls = [
        (p16, P, [0, 0, 0], {}, -1),                                       # no member has a chunk
        (p16, [P[0], 0, P[2]], [700, 700, 700], {}, 1),                    # a NULL or misaligned member chunk
        (p16, [P[0], P[1], P[2] + 2], [700, 700, 700], {}, 2),
        (pf, PF, [700, 0, 700], {}, 0),                                    # complex64 over the int16 partial slots
        (p16, P, [700, 700, 700], dict(d_ind=vp(0)), 0),                   # d_ind NULL or misaligned
        (p16, P, [700, 700, 700], dict(d_ind=vp(ind.data_ptr() + 1)), 0),
        (p16, P, [100, 700, 100], dict(stride=0), 1),                      # out_stride too small: member 1 alone cuts a slot
        (p16, P, [4000, 4000, 3150], dict(stride=5), 0),                   # members 0 and 1 would cut 6, member 2 cuts 5
    ]
    for fn, ptrs, sizes, kw, who in calls:
        assert pull(fn, ptrs, sizes, **kw) == EINVAL and bad.value == who, (sizes, kw)
    torch.cuda.synchronize()
    assert [(g.state(m).tobytes(), g.clock(m), g.plan(m, 1).tobytes()) for m in range(3)] == before
    assert (ind.cpu().numpy() == 0xAB).all() and (bits.cpu().numpy() == 0x5A).all()
    # the complex64 entry point's alignment is 8 bytes; member 1's format is its own (its partial slot was dropped)
    g.set_clock(1, 7, 7, -625)
    assert pull(pf, [0, PF[1] + 4, 0], [0, 700, 0]) == EINVAL and bad.value == 1
    assert pull(pf, [0, PF[1], 0], [0, 700, 0]) == 0 and list(ns) == [0, 1, 0]
    assert pull(p16, P, [700, 700, 700]) == EINVAL and bad.value == 1 and pull(p16, [P[0], 0, P[2]], [700, 0, 700]) == 0
    # what is accepted goes on from the untouched state; a NULL d_bits gives the same records
    torch.cuda.synchronize()
    ind.fill_(0xAB)
    for m in range(3):
        g.set_clock(m, 7, 7, -625)
    assert pull(p16, P, [700, 700, 700]) == 0 and pull(p16, P, [4000, 4000, 3150], stride=6) == 0 and list(ns) == [6, 6, 5]
    torch.cuda.synchronize()
    a = ind.cpu().numpy().copy()
    for m in range(3):
        g.set_clock(m, 7, 7, -625)
    assert pull(p16, P, [700, 700, 700]) == 0 and pull(p16, P, [4000, 4000, 3150], d_bits=vp(0), stride=6) == 0
    torch.cuda.synchronize()
    b = ind.cpu().numpy()
    flat = a.reshape(-1, 32)                                       # out_stride 6: members 0 and 1 own 6 rows each, member 2 five
    assert np.array_equal(a, b) and (flat[:17] != 0xAB).any(axis=1).all() and (flat[17:] == 0xAB).all()
    g.close()
