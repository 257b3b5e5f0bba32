"""GPU tests of the MS-side FCCH frequency-offset measurement: both batch entry points against the float64 form of the literal model
(tests/ms_afc_model.py) under a derived bound, the read and write windows, and the slot scheduler and its group with AFC on --
byte-identical to the batch entry point over the same slots, and everything else byte-identical to AFC off.

The per-row bar against the float64 model (derived, not measured; ms_afc_model.hz_bar): a 92-term float sum in any order errs by
<= 92 * 2^-23 * S, S = sum |a| |b|, so the angle of v_L moves by <= d_alpha_L = 92 * 2^-23 * S_L / |v_L| and
|d hz| <= fs / (4 pi) * (d_alpha_1 / 3 + d_alpha_2 / 32) = 0.32 * S_1 / |v_1| + 0.03 * S_2 / |v_2| Hz, plus 0.02 Hz for a few ulps of
hz.  (p, r, s) is compared on every row whose P_unrounded is further from a half-integer than (3 d_alpha_2 + 32 d_alpha_1) / (2 pi)."""
import ctypes as C

import numpy as np
import pytest

import ms_afc_cases as AC
import ms_afc_model as AM
from osmo_trx_amd import trxhip

pytestmark = pytest.mark.gpu

EINVAL = -22
FCCH = trxhip.MS_FCCH_DTYPE
CANARY = 0xA5


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")      # (a copy: the shared row sets are read-only)


def to_c64(rows):
    return (rows[..., 0].astype(np.float32) + 1j * rows[..., 1].astype(np.float32)).astype(np.complex64)


# ---- the batch entry points against the float64 model -------------------------------------------------------------------------

def check_against_model(got, want, tone):
    """one device record against the float64 model's dict; returns whether the row's (p, r, s) was compared"""
    if want["E"] == 0:                                             # the all-zero slot: no sum has an error
        for k in ("hz", "alpha_one", "alpha_two", "mag_one", "mag_two", "energy"):
            assert got[k] == want[k], k
        assert (got["p"], got["r"], got["s"]) == (0, 0, 0)
        return True
    assert got["reserved"] == 0
    for k, S in (("mag_one", want["S_one"]), ("mag_two", want["S_two"]), ("energy", want["E"])):
        assert abs(float(got[k]) - float(want[k])) <= AM.EPS_SUM * S, (k, got[k], want[k])
    decided = AM.decision_margin(want) > 0
    assert decided or not tone
    same = (int(got["p"]), int(got["r"]), int(got["s"])) == (want["p"], want["r"], want["s"])
    assert same or not decided, (got, want)
    if same:
        for k, which in (("alpha_one", 1), ("alpha_two", 2)):
            assert abs(float(got[k]) - float(want[k])) <= AM.d_alpha(want, which), (k, got[k], want[k])
        d = abs(float(got["hz"]) - float(want["hz"]))
        assert d <= AM.hz_bar(want), (d, AM.hz_bar(want), got, want)
    return decided


@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_i16_rows_against_float64_model(trx, n):
    rows, n_tones = AC.device_row_set()
    want = AC.models("device")
    pick = list(range(len(rows) - n, len(rows))) if n < 257 else list(range(257))          # the tail holds the clipped rows and the zero row
    got = trx.ms_fcch(dev(rows[pick]), AC.FULL)
    left_out = sum(not check_against_model(got[i], want[r], r < n_tones) for i, r in enumerate(pick))
    assert left_out <= 0.02 * len(rows)


def test_all_rows_both_entry_points_strides_and_odd_starts(trx):
    """the whole row set through both entry points: int16 at stride 641 from an odd sample on, complex64 at stride 625 and 641;
    the three agree byte for byte with the plain int16 call (the complex64 of an int16 value is that value), and that one meets
    the model"""
    import torch
    rows, n_tones = AC.device_row_set()
    want = AC.models("device")
    n = len(rows)
    plain = trx.ms_fcch(dev(rows), AC.FULL)
    left_out = sum(not check_against_model(plain[i], want[i], i < n_tones) for i in range(n))
    assert left_out <= 0.02 * n
    assert left_out == sum(AM.decision_margin(m) <= 0 for m in want[:-1])
    rng = np.random.default_rng(3)
    for stride, off in ((641, 1), (641, 3), (625, 1)):
        buf = rng.integers(-32768, 32768, (off + n * stride, 2)).astype(np.int16)
        for r in range(n):
            buf[off + r * stride:off + r * stride + 625] = rows[r]
        got = trx.ms_fcch(dev(buf)[off:], AC.FULL, slot_stride=stride, n_slots=n)
        assert got.tobytes() == plain.tobytes(), (stride, off)
    c = to_c64(rows)
    assert trx.ms_fcch(dev(c), AC.FULL).tobytes() == plain.tobytes()
    wide = np.full((n, 641), np.nan + 1j * np.nan, dtype=np.complex64)
    wide[:, :625] = c
    assert trx.ms_fcch(dev(wide), AC.FULL).tobytes() == plain.tobytes()
    assert trx.ms_fcch(dev(wide.reshape(-1)), AC.FULL, slot_stride=641, n_slots=n).tobytes() == plain.tobytes()
    torch.cuda.synchronize()


def test_read_window(trx):
    """complex64 rows with NaN at every sample outside 52 .. 175: byte-identical to the clean rows"""
    rows, _ = AC.device_row_set()
    c = to_c64(rows[:70])
    clean = trx.ms_fcch(dev(c), AC.FULL)
    dirty = np.full_like(c, np.nan + 1j * np.nan)
    dirty[:, AM.FIRST:AM.LAST + 1] = c[:, AM.FIRST:AM.LAST + 1]
    got = trx.ms_fcch(dev(dirty), AC.FULL)
    assert got.tobytes() == clean.tobytes() and not np.isnan(got["hz"]).any()
    assert (AM.FIRST, AM.LAST) == (52, 175)


def test_write_window_and_refusals(trx):
    import torch
    rows, _ = AC.device_row_set()
    L = trx.L
    for n in (1, 5, 65):
        x = dev(rows[:n])
        out = torch.full((n + 2, 32), CANARY, dtype=torch.uint8, device="cuda:0")
        assert L.trxhip_ms_fcch_batch_i16(trx.h, x.data_ptr(), 625, out.data_ptr() + 32, n, AC.FULL, None) == 0
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[0] == CANARY).all() and (o[-1] == CANARY).all()
        assert o[1:-1].tobytes() == trx.ms_fcch(x, AC.FULL).tobytes()
    x = dev(rows[:2])
    xc = dev(to_c64(rows[:2]))
    out = torch.full((2, 32), CANARY, dtype=torch.uint8, device="cuda:0")
    i16, c32 = L.trxhip_ms_fcch_batch_i16, L.trxhip_ms_fcch_batch_cf32
    for fn, args in ((i16, (x.data_ptr(), 624, out.data_ptr(), 1, AC.FULL)), (i16, (x.data_ptr(), 625, out.data_ptr(), 0, AC.FULL)),
                     (i16, (x.data_ptr() + 2, 625, out.data_ptr(), 1, AC.FULL)), (i16, (0, 625, out.data_ptr(), 1, AC.FULL)),
                     (i16, (x.data_ptr(), 625, 0, 1, AC.FULL)), (i16, (x.data_ptr(), 625, out.data_ptr(), 1, 0.0)),
                     (i16, (x.data_ptr(), 625, out.data_ptr(), 1, float("nan"))), (i16, (x.data_ptr(), 625, out.data_ptr(), 1 << 31, AC.FULL)),
                     (c32, (xc.data_ptr() + 4, 625, out.data_ptr(), 1, AC.FULL)), (c32, (xc.data_ptr(), 600, out.data_ptr(), 1, AC.FULL)),
                     (c32, (xc.data_ptr(), 625, out.data_ptr() + 1, 1, AC.FULL))):
        assert fn(trx.h, *args, None) == EINVAL, args
    assert i16(None, x.data_ptr(), 625, out.data_ptr(), 1, AC.FULL, None) == EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all()


# ---- the scheduler and the group -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def burst(trx):
    """an all-zero-bit GMSK burst from the project's own modulator: the FCCH tone, complex64 at unit amplitude"""
    import torch
    bits = torch.zeros((1, 148), dtype=torch.uint8, device="cuda:0")
    out, _, lens = trx.modulate(bits, trx.tx_params_tensor(trxhip.tx_params_host(148, 8)), sps=4)
    y = out[0, :int(lens[0])].cpu().numpy()
    assert 400 <= len(y) <= 625
    y = (y / np.abs(y[100:400]).mean()).astype(np.complex64)
    m = AM.fcch_offset(np.concatenate([y, np.zeros(625 - len(y), np.complex64)]))  # the tone of a carrier that is on frequency
    assert abs(float(m["hz"]) - AC.BIAS_HZ) <= 100.0 and float(m["mag_one"]) / float(m["energy"]) > 0.99
    return y


CFOS = (1500.0, -23000.0, 41000.0)
# samples per pull.  Member 0: the FCCH slot at frame 10 (sample 50 000) straddles two pulls; the one at frame 20 (100 000) begins
# in the carried partial slot, which a short chunk extends before a third pull completes it; the others lie whole in a chunk
CHUNKS = ((50300, 49800, 200, 99700, 55017, 254983), (625 * 8 * 51 + 77, 1000, 625 * 8 * 51 - 1077), (100111, 400, 199489, 210000))
ACTIVE = (0b01100110, 0xFF, 0b00000001)                            # member 0: TN 0 is not ACTIVE -- its FCCH slots are measured all the same


@pytest.fixture(scope="module")
def streams(burst):
    return [AC.stream(burst, cfo, 900 + m) for m, cfo in enumerate(CFOS)]


def gather(x, plan, origin):
    """(the FCCH slots' indices in the pull, their 625 samples as rows) from the pull's plan"""
    ks = [k for k, p in enumerate(plan) if p["kind"] == trxhip.MS_KIND_FCCH]
    rows = [x[int(plan[k]["ts"]) - origin:int(plan[k]["ts"]) - origin + 625] for k in ks]
    return ks, (np.stack(rows) if rows else np.zeros((0, 625) + x.shape[1:], x.dtype))


class Expect:
    """what _state must report after the FCCH slots seen so far"""

    def __init__(self):
        self.recs, self.fns = [], []

    def add(self, recs, fns):
        self.recs += list(recs)
        self.fns += [int(f) for f in fns]

    def check(self, st, enable=True):
        assert st["count"] == len(self.recs) and st["enable"] == enable
        if not self.recs:
            assert st["last"] is None and st["ring"] == []
            return
        assert st["last"].tobytes() == self.recs[-1].tobytes()
        want = [dict(fn=f, hz=r["hz"].item(), mag_one=r["mag_one"].item(), energy=r["energy"].item())
                for f, r in zip(self.fns[-8:], self.recs[-8:])]
        assert st["ring"] == want


def check_pull(trx, x, plan, origin, fcch_rows, exp, cfo):
    """d_fcch of one member's pull (uint8[rows, 32] numpy, canaried before the pull) against the batch entry point over the same
    slots gathered into rows"""
    ks, rows = gather(x, plan, origin)
    untouched = np.ones(len(fcch_rows), bool)
    untouched[ks] = False
    assert (fcch_rows[untouched] == CANARY).all()
    if ks:
        want = trx.ms_fcch(dev(rows), AC.FULL)
        got = fcch_rows[ks].reshape(-1).view(FCCH)
        assert got.tobytes() == want.tobytes()
        for r in got:
            assert abs(float(r["hz"]) - (cfo + AC.BIAS_HZ)) <= 100.0, (r["hz"], cfo)
            assert float(r["mag_one"]) / float(r["energy"]) > 0.9
        exp.add(got, [plan[k]["fn"] for k in ks])
    return ks


def test_single_object(trx, streams):
    import torch
    x, cfo = streams[0], CFOS[0]
    d_x = dev(x)
    on, off = (trxhip.MsRxScheduler(trx, rx_full_scale=AC.FULL, tsc=0o53 & 7, active_tns=ACTIVE[0], tracking=True) for _ in range(2))
    cap = max(CHUNKS[0]) // 625 + 2
    fc = torch.full((cap, 32), CANARY, dtype=torch.uint8, device="cuda:0")
    on.set_afc(True, out=fc)
    for o in (on, off):
        o.set_clock(AC.FN0 - 1, 7, -625)
    exp = Expect()
    exp.check(on.afc_state())
    at, seen = 0, []
    for n in CHUNKS[0]:
        fc.fill_(CANARY)
        ind1, sb1 = on.pull(d_x[at:at + n], first_ts=at)
        ind0, sb0 = off.pull(d_x[at:at + n], first_ts=at)
        assert torch.equal(ind1, ind0) and torch.equal(sb1, sb0)                   # nothing existing moves
        assert on.state().tobytes() == off.state().tobytes() and on.clock() == off.clock()
        plan = on.plan()
        ks = check_pull(trx, x, plan, 0, fc.cpu().numpy(), exp, cfo)
        seen += [(int(plan[k]["ts"]), int(plan[k]["src_off"]), k) for k in ks]
        ind = on.ind_to_numpy(ind1)
        for k in ks:                                               # an inactive FCCH slot: no indication, and measured all the same
            assert ind[k]["kind"] == trxhip.MS_KIND_FCCH and ind[k]["sent"] == 0 and not plan[k]["flags"] & trxhip.MS_SLOT_ACTIVE
        exp.check(on.afc_state())
        at += n
    assert at == len(x) and len(exp.recs) == 10 == len(AC.fcch_slots())
    assert sorted(fn % 51 for fn in exp.fns) == [0, 0, 10, 10, 20, 20, 30, 30, 40, 40]
    # the three ways a slot reaches the kernel: whole in a chunk, straddling two pulls, begun in a partial slot that a pull extended
    assert any(off_ >= 0 for _, off_, _ in seen) and sum(off_ < 0 and k == 0 for _, off_, k in seen) >= 2
    assert off.afc_state() == dict(count=0, enable=False, last=None, ring=[])
    # _set leaves the state alone; off: pulls measure nothing; set_clock does not touch it
    before = on.afc_state()
    on.set_afc(False)
    on.set_clock(AC.FN0 - 1, 7, -625)
    fc.fill_(CANARY)
    on.pull(d_x[:625 * 100], first_ts=0)
    assert {**on.afc_state(), "enable": True} == {**before, "enable": True} and (fc.cpu().numpy() == CANARY).all()
    assert before["last"].tobytes() == on.afc_state()["last"].tobytes()
    # a refused pull (out_slots too small) leaves the state as it was
    on.set_afc(True, out=fc)
    on.set_clock(AC.FN0 - 1, 7, -625)
    ns, nc = C.c_size_t(), C.c_size_t()
    ind = torch.empty((200, 32), dtype=torch.uint8, device="cuda:0")
    rc = on.L.trxhip_ms_sched_pull_s16(on.h, d_x.data_ptr(), 625 * 100, 0, ind.data_ptr(), None, 50, C.byref(ns), C.byref(nc), None)
    st = on.afc_state()
    assert rc == EINVAL and st["count"] == before["count"] and st["ring"] == before["ring"] and (fc.cpu().numpy() == CANARY).all()
    # on without an output array: the state alone moves
    on.set_afc(True)
    on.pull(d_x[:625 * 100], first_ts=0)
    st = on.afc_state()
    assert st["count"] == before["count"] + 2 and [r["fn"] for r in st["ring"][-2:]] == [AC.FN0, AC.FN0 + 10]
    assert (fc.cpu().numpy() == CANARY).all()
    cfg = trxhip._MsAfcCfg(1, 0, fc.data_ptr() + 1)
    assert on.L.trxhip_ms_afc_sched_set(on.h, C.byref(cfg)) == EINVAL             # a misaligned d_fcch


def test_single_object_more_than_a_ring_in_one_pull(trx, streams):
    """one pull that cuts all 10 FCCH slots: the ring keeps the last 8, oldest first"""
    import torch
    x = streams[1]
    d_x = dev(x)
    s = trxhip.MsRxScheduler(trx, rx_full_scale=AC.FULL, tsc=0o53 & 7, tracking=False)
    s.set_clock(AC.FN0 - 1, 7, -625)
    fc = torch.full((len(x) // 625, 32), CANARY, dtype=torch.uint8, device="cuda:0")
    s.set_afc(True, out=fc)
    s.pull(d_x, first_ts=0)
    exp = Expect()
    assert check_pull(trx, x, s.plan(), 0, fc.cpu().numpy(), exp, CFOS[1]) == AC.fcch_slots()
    exp.check(s.afc_state())
    assert len(s.afc_state()["ring"]) == 8 and s.afc_state()["count"] == 10


def test_complex64_pull(trx, streams):
    import torch
    x = to_c64(streams[2][:625 * 8 * 23])
    d_x = dev(x)
    on, off = (trxhip.MsRxScheduler(trx, rx_full_scale=AC.FULL, tsc=0o53 & 7, tracking=True) for _ in range(2))
    fc = torch.full((8 * 23, 32), CANARY, dtype=torch.uint8, device="cuda:0")
    on.set_afc(True, out=fc)
    exp = Expect()
    at = 0
    for o in (on, off):
        o.set_clock(AC.FN0 - 1, 7, -625)
    for n in (50100, 300, len(x) - 50400):                        # the slot at frame 10 begins in the partial slot and is extended once
        fc.fill_(CANARY)
        ind1, sb1 = on.pull(d_x[at:at + n], first_ts=at)
        ind0, sb0 = off.pull(d_x[at:at + n], first_ts=at)
        assert torch.equal(ind1, ind0) and torch.equal(sb1, sb0)
        check_pull(trx, x, on.plan(), 0, fc.cpu().numpy(), exp, CFOS[2])
        exp.check(on.afc_state())
        at += n
    assert len(exp.recs) == 3


def test_group_of_three(trx, streams):
    """3 members, different CFOs, chunkings and ACTIVE masks, member 1 without AFC output array, against an identical group with
    AFC off; a refused pull in between moves no member's state"""
    import torch
    n = 3
    d_xs = [dev(x) for x in streams]
    mk = lambda: trxhip.MsRxSchedulerGroup(trx, n=n, rx_full_scale=AC.FULL, tsc=0o53 & 7, active_tns=list(ACTIVE), tracking=True)
    on, off = mk(), mk()
    stride = max(max(c) for c in CHUNKS) // 625 + 2
    fc = torch.full((n * stride, 32), CANARY, dtype=torch.uint8, device="cuda:0")
    for m in range(n):
        on.set_afc(m, True, out=None if m == 1 else fc)
        for g in (on, off):
            g.set_clock(m, AC.FN0 - 1, 7, -625)
    exps = [Expect() for _ in range(n)]
    at = [0] * n
    for k in range(max(len(c) for c in CHUNKS)):
        sizes = [CHUNKS[m][k] if k < len(CHUNKS[m]) else 0 for m in range(n)]
        chunks = [d_xs[m][at[m]:at[m] + sizes[m]] if sizes[m] else None for m in range(n)]
        if k == 1:                                                 # refused for member 0's 80 slots: nothing moves
            before = [on.afc_state(m) for m in range(n)]
            with pytest.raises(trxhip.TrxHipError):
                on.pull(chunks, first_ts=list(at), out_stride=20)
            assert on.bad_member == 0
            for m in range(n):
                exps[m].check(on.afc_state(m))
                assert on.afc_state(m)["ring"] == before[m]["ring"]
        fc.fill_(CANARY)
        res1, ns1 = on.pull(chunks, first_ts=list(at), out_stride=stride)
        res0, ns0 = off.pull(chunks, first_ts=list(at), out_stride=stride)
        assert ns1 == ns0
        h = fc.cpu().numpy().reshape(n, stride, 32)
        for m in range(n):
            if not sizes[m]:
                assert ns1[m] == 0 and (h[m] == CANARY).all()
                continue
            assert torch.equal(res1[m][0], res0[m][0]) and torch.equal(res1[m][1], res0[m][1]), (k, m)
            assert on.state(m).tobytes() == off.state(m).tobytes() and on.clock(m) == off.clock(m)
            if m == 1:                                             # no array: its rows keep the canary; the state is checked below
                assert (h[m] == CANARY).all()
                ks, rows = gather(streams[m], on.plan(m), 0)
                if ks:
                    exps[m].add(trx.ms_fcch(dev(rows), AC.FULL), [on.plan(m)[j]["fn"] for j in ks])
            else:
                assert (h[m, ns1[m]:] == CANARY).all()
                check_pull(trx, streams[m], on.plan(m), 0, h[m, :ns1[m]], exps[m], CFOS[m])
            at[m] += sizes[m]
        for m in range(n):
            exps[m].check(on.afc_state(m))
            assert off.afc_state(m)["count"] == 0
    assert at == [len(x) for x in streams] and [len(e.recs) for e in exps] == [10, 10, 10]
    for m in range(n):
        hz = np.array([r["hz"] for r in exps[m].recs])
        assert np.abs(hz - (CFOS[m] + AC.BIAS_HZ)).max() <= 100.0
