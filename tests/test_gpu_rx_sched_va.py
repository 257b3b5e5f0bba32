"""The uplink burst scheduler's Viterbi-equaliser flow on the GPU (pytest -m gpu): RxScheduler(use_va=True), cfg->use_va of
Transceiver::pullRadioVector() (Transceiver.cpp:760-787), against the composition of the public calls it restates -- the rows
shifted by 20 samples through trxhip_detect_demod_batch without soft output, trxhip_convert_short_float,
trxhip_energy_detect_batch_cf32(window 80) and trxhip_demod_va_batch_cf32 over the slots as read, trxhip_apply_diversity_power,
the model of tests/rx_sched_model.py and trxhip_pack_trxd_wire_batch -- byte for byte, so the flow brings no tolerance of its
own; against the oracle's pull_radio_vector_chain(use_va=True); behind the RESAMP receive front end; and in a loopback from
TxScheduler.render.  The stream handed to the object is what the radio reads with readTimestamp -= 20 (osmo-trx.cpp:84-99):
every burst lies 20 samples into its slot."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rx_sched_model as M  # noqa: E402
import tx_sched_model as TM  # noqa: E402
from osmo_trx_amd import synth, trxhip  # noqa: E402

pytestmark = pytest.mark.gpu
FULL = 32767.0
TSC = 3
EINVAL = -22
VA_SCALE = 1.0 / 16383.0
# TSC traffic (I, VII), a RACH combination (IV), IDLE (FILL) and NONE (OFF)
COMBS = ([1, 4, 1, M.COMB_FILL, 1, M.COMB_NONE, 7, 1],
         [1, 1, M.COMB_FILL, 1, 4, 1, M.COMB_NONE, 1])
VERSIONS = (0, 1)
OFFSETS = (0.0, 9.0)
CLOCK = (2715648 - 2, 5)                             # the hyperframe wraps inside the stream
# (slots the pull cuts, samples it leaves): every slot count and remainder at which the receiver -- 4 slots per wave, 8 per
# workgroup -- and the cutter can go wrong
CUTS_A = [(0, 625), (1, 1), (3, 20), (4, 39), (5, 40), (8, 585), (9, 604), (1, 624), (0, 625), (3, 1)]
CUTS_B = [(4, 313), (0, 330), (9, 330), (8, 430), (13, 1)]
N = sum(k for k, _ in CUTS_A)
MUTED = (13, 21)                                     # channel 1 is muted while these slots are cut: a pull of its own in A and in B
LOUD, SILENT = slice(5, None, 11), slice(7, None, 13)   # slots with clipped noise / with noise alone, whatever their type
assert N == sum(k for k, _ in CUTS_B) == 34


def sizes(cuts):
    out, rem = [], 0
    for k, r in cuts:
        out.append(k * 625 + r - rem)
        rem = r
    assert min(out) >= 0
    return out


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = trxhip.TrxHip(0)
    yield t
    t.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def configure(o, chans=2, combs=COMBS, clock=CLOCK):
    o.set_clock(*clock)
    for c in range(chans):
        for tn in range(8):
            o.set_slot(c, tn, combs[c][tn])
        o.set_trxd_version(c, VERSIONS[c])
    o.set_handover(6, 2, True)


def new_sched(trx, chans=2, max_slots=64, **kw):
    s = trxhip.RxScheduler(trx, chans=chans, tsc=TSC, ul_fn_offset=-3, ext_rach=True, full_scale=FULL, max_slots=max_slots,
                           use_va=True)
    configure(s, chans, **kw)
    if chans > 1:
        s.set_rssi_offset(1, OFFSETS[1])
    return s


def new_model(chans=2, **kw):
    m = M.Model(chans, tsc=TSC, ul_fn_offset=-3, ext_rach=True)
    configure(m, chans, **kw)
    return m


def early_read(rows):
    """burst rows as the detector wants them -> the slots a radio that reads 20 samples early cuts: the burst 20 samples in"""
    import torch
    return torch.roll(rows, 20, dims=1)


def composition(trx, rows, p_det):
    """The existing public calls over one channel's slots as rows (int16[n, 625, 2] or complex64[n, 625]) with the detector's
    parameters -> (result records uint8[n, 32], sliced soft rows float32[n, 148]) on the device"""
    import torch
    shifted = torch.zeros_like(rows)
    shifted[:, :585] = rows[:, 20:605]                                   # shift_vec: samples 20 .. 604, zeros behind
    pt = trx.params_tensor(p_det)
    res, _ = trx.detect_demod(shifted, pt, sps=4, full_scale=FULL, slice_bits=False, want_soft=False)
    cf = rows if rows.dtype == torch.complex64 else torch.view_as_complex(trx.convert_short_float(rows))
    energy = trx.energy_detect(cf, 80)
    soft, _ = trx.demod_va(cf, pt, scale=VA_SCALE, soft_stride=148, slice_bits=True, detected=res)
    trx.apply_diversity_power(res, pt, energy, full_scale=FULL)
    return res, soft


def ind_records(want):
    """the model's indications as the 32-byte records"""
    a = np.zeros(len(want), dtype=trxhip.UL_IND_DTYPE)
    for k in ("fn", "tn", "type", "flags", "tsc", "rc", "toa", "ci", "rssi", "noise_lev", "nbits"):
        a[k] = [w[k] for w in want]
    return a


class Scenario:
    """two channels, N slots + 1 sample: synth normal and access bursts by the model's slot type, 20 samples into their slots,
    with clipped and noise-only slots among them"""

    def __init__(self):
        import torch
        self.plan = new_model().cut(N * 625 + 1)
        nb, _, _ = synth.make_normal_bursts(2 * N, "cpu", 4, seed=301, tsc=TSC, p_noise=0.0, p_clip=0.0)
        ab, _, _ = synth.make_access_bursts(2 * N, "cpu", seed=302, ext=False, p_noise=0.0)
        xb, _, _ = synth.make_access_bursts(2 * N, "cpu", seed=303, ext=True, p_noise=0.0)
        rng = np.random.default_rng(304)
        loud = np.round(rng.standard_normal((2 * N, 625, 2)) * 14000.0).clip(-32768, 32767).astype(np.int16)
        assert (np.abs(loud.astype(np.int32)).max((1, 2)) > 30000).all()
        silent = np.round(rng.standard_normal((2 * N, 625, 2)) * 40.0).astype(np.int16)
        self.stream = torch.zeros((2, N * 625 + 1, 2), dtype=torch.int16)
        self.judged = np.zeros((2, N), bool)             # neither OFF, IDLE, muted, nor deliberately noise-only or clipped
        for c in range(2):
            typ = np.array([p[2] for p in self.plan[c]])
            rows = nb[c * N:(c + 1) * N].clone()
            for t, pool in ((M.RACH, ab), (M.EXT_RACH, xb)):
                idx = torch.from_numpy(np.flatnonzero(typ == t))
                rows[idx] = pool[c * N + idx]
            rows = early_read(rows)
            rows[LOUD] = torch.from_numpy(loud[c * N:(c + 1) * N][LOUD])
            rows[SILENT] = torch.from_numpy(silent[c * N:(c + 1) * N][SILENT])
            self.stream[c, :N * 625] = rows.reshape(N * 625, 2)
            self.judged[c] = (typ != M.OFF) & (typ != M.IDLE)
            self.judged[c][LOUD] = self.judged[c][SILENT] = False
            assert {M.TSC, M.IDLE, M.OFF} < set(typ) and (M.RACH in typ or M.EXT_RACH in typ), set(typ)
        self.judged[1, MUTED[0]:MUTED[1]] = False
        self.stream = self.stream.to("cuda:0")
        self._want = {}

    def input(self, cf32):
        import torch
        return torch.view_as_complex(self.stream.to(torch.float32)) if cf32 else self.stream

    def params_meta(self, c):
        p = np.zeros(N, dtype=trxhip.PARAMS_DTYPE)
        m = np.zeros(N, dtype=trxhip.TRXD_META_DTYPE)
        a = np.array(self.plan[c], dtype=np.int64).reshape(-1, 4)
        m["fn"], m["tn"], p["type"], p["max_toa"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        p["tsc"] = TSC
        m["version"] = VERSIONS[c]
        return p, m

    def want(self, trx, cf32):
        """per channel (ind records, pkt, pkt_len, soft), the model behind them -- the composition, computed once per format"""
        import torch
        if cf32 in self._want:
            return self._want[cf32]
        m = new_model()
        m.cut(N * 625 + 1)
        out = []
        for c in range(2):
            p, mt = self.params_meta(c)
            muted = np.zeros(N, bool)
            if c == 1:
                muted[MUTED[0]:MUTED[1]] = True
            p_det = p.copy()
            p_det["type"][muted] = M.OFF                                 # no DSP on a muted slot (Transceiver.cpp:719-721)
            x = self.input(cf32)[c, :N * 625]
            rows = x.view(N, 625) if cf32 else x.view(N, 625, 2)
            res_t, soft = composition(trx, rows, p_det)
            torch.cuda.synchronize()
            res = trx.results_to_numpy(res_t).copy()
            # at least three quarters of the slots with something to find are found: the comparison is not one of idle records
            found = res["rc"][self.judged[c]] > 0
            assert found.mean() >= 0.75, (c, found.mean())
            # a muted slot that is not OFF is an idle indication with bi->rssi 0: the packer adds the channel's offset
            res["rssi"][muted & (p["type"] != M.OFF)] = -np.float32(OFFSETS[c])
            want = []
            for a, b, mu in ((0, MUTED[0], False), (MUTED[0], MUTED[1], True), (MUTED[1], N, False)):
                m.set_muted(1, mu)
                want += m.run(c, self.plan[c][a:b], res[a:b])
            pkt, plen = trx.pack_trxd_wire(dev(res.view(np.uint8).reshape(N, 32)), trx.params_tensor(p), soft,
                                           dev(mt.view(np.uint8).reshape(N, 8)), pkt_stride=160, rssi_offset=OFFSETS[c])
            torch.cuda.synchronize()
            out.append((ind_records(want), pkt.cpu().numpy(), plen.cpu().numpy(), soft.cpu().numpy()))
        self._want[cf32] = (out, m)
        return self._want[cf32]


@pytest.fixture(scope="module")
def scn(trx):
    return Scenario()


def run_chunked(trx, scn, cf32, cuts):
    """the stream through a fresh scheduler in pulls of sizes(cuts) -> (scheduler, ind, pkt, pkt_len, soft) concatenated"""
    import torch
    s = new_sched(trx)
    x = scn.input(cf32)
    parts, at, done = [], 0, 0
    for (k, r), n in zip(cuts, sizes(cuts)):
        s.set_muted(1, MUTED[0] <= done < MUTED[1])
        assert s.slots(n) == k
        pkt, plen, ind, soft = s.pull(x[:, at:at + n].contiguous(), want_soft=True)
        assert pkt.shape[1] == k and s.carried == r
        parts.append((s.ind_to_numpy(ind), pkt, plen, soft))
        at += n
        done += k
    torch.cuda.synchronize()
    assert at == N * 625 + 1 and done == N
    ind = np.concatenate([p[0] for p in parts], 1)
    pkt, plen, soft = (torch.cat([p[k] for p in parts], 1).cpu().numpy() for k in (1, 2, 3))
    return s, ind, pkt, plen, soft


@pytest.mark.parametrize("kind", ["s16", "cf32"])
def test_pull_equals_the_composition(trx, scn, kind):
    cf32 = kind == "cf32"
    want, m = scn.want(trx, cf32)
    s, ind, pkt, plen, soft = run_chunked(trx, scn, cf32, CUTS_A)
    assert s.clock() == m.clock
    for c in range(2):
        w_ind, w_pkt, w_len, w_soft = want[c]
        assert np.array_equal(plen[c], w_len), np.flatnonzero(plen[c] != w_len)[:10]
        assert np.array_equal(pkt[c], w_pkt), np.flatnonzero((pkt[c] != w_pkt).any(1))[:10]
        assert np.array_equal(raw(soft[c]), raw(w_soft)), np.flatnonzero((soft[c] != w_soft).any(1))[:10]
        assert np.array_equal(raw(ind[c]), raw(w_ind)), [k for k in w_ind.dtype.names if not np.array_equal(raw(ind[c][k]), raw(w_ind[k]))]
        assert s.counters(c) == m.ctr[c]
        ring, itr, lev = s.noise_state(c)
        assert np.array_equal(raw(ring), raw(m.noise[c].ring)) and itr == m.noise[c].itr
        assert np.float32(lev).tobytes() == np.float32(m.noise[c].lev).tobytes()
    typ = ind[0]["type"]
    assert (ind[0]["rc"][typ == M.TSC] == M.TSC).sum() > 8 and (ind[0]["rc"][typ == M.EXT_RACH] == M.EXT_RACH).any()
    assert set(np.unique(soft)) <= {0.0, 0.5, 1.0} and (soft == 1.0).any()       # hard decisions; 0.5 behind an access burst's 88 bits
    assert m.ctr[0]["rx_clipping"] > 0 and m.noise[0].itr > 0 and m.noise[1].lev > 0
    muted = ind[1][MUTED[0]:MUTED[1]]
    assert ((muted["flags"] & trxhip.ULIND_MUTED) != 0)[muted["type"] != M.OFF].all()


@pytest.mark.parametrize("kind", ["s16", "cf32"])
def test_chunking_never_changes_the_output(trx, scn, kind):
    a = run_chunked(trx, scn, kind == "cf32", CUTS_A)
    b = run_chunked(trx, scn, kind == "cf32", CUTS_B)
    for x, y in zip(a[1:], b[1:]):
        assert x.shape == y.shape and np.array_equal(raw(x), raw(y))
    assert a[0].clock() == b[0].clock()
    for c in range(2):
        assert a[0].counters(c) == b[0].counters(c)
        na, nb = a[0].noise_state(c), b[0].noise_state(c)
        assert np.array_equal(raw(na[0]), raw(nb[0])) and na[1] == nb[1] and np.float32(na[2]).tobytes() == np.float32(nb[2]).tobytes()


def test_against_the_oracle(trx, scn):
    """channel 0's slots as rows through the oracle's pullRadioVector() chain with use_va: the same decisions, times of arrival
    and hard bits; rssi within the bar of test_pull_radio_vector_adapter_with_use_va (2e-5 dB)"""
    import oracle_lib as O
    _, ind, _, _, soft = run_chunked(trx, scn, False, CUTS_A)
    ind, soft = ind[0], soft[0]
    p, _ = scn.params_meta(0)
    rows = scn.stream[0, :N * 625].view(N, 625, 2).cpu().numpy()
    chain = O.pull_radio_vector_chain(rows, p, 1, use_va=True)
    n_det, clip, nodet = 0, 0, 0
    for i, (code, bi, clipc, nodetc) in enumerate(chain):
        assert (code != 0) == (p["type"][i] == M.OFF) == bool(ind["flags"][i] & trxhip.ULIND_OFF), i
        if code != 0:
            continue
        clip += ind["rc"][i] == -M.SIGERR_CLIP
        nodet += ind["rc"][i] < 0 and ind["rc"][i] != -M.SIGERR_CLIP
        assert (clip, nodet) == (clipc, nodetc), i
        assert bool(bi.idle) == (ind["rc"][i] <= 0) == bool(ind["flags"][i] & trxhip.ULIND_IDLE), i
        assert abs(float(ind["rssi"][i]) - bi.rssi) < 2e-5, i
        if not bi.idle:
            n_det += 1
            assert ind["rc"][i] == p["type"][i] and ind["toa"][i] == bi.toa and ind["tsc"][i] == bi.tsc and ind["nbits"][i] == bi.nbits, i
            assert np.array_equal(soft[i], np.frombuffer(bi.rx_burst, dtype=np.float32)[:148]), i
    assert n_det >= 0.75 * scn.judged[0].sum()


def resamp_wide(n_blocks, block_len, seed):
    """a RESAMP front end's int16 input with something in it: noise that the detector finds nothing in would leave the soft rows
    zero, so the slots carry synth normal bursts stretched to the input rate by repetition and interpolation"""
    import torch
    rng = np.random.default_rng(seed)
    n_in = n_blocks * block_len
    n_out = n_in * 65 // 96
    n_slots = n_out // 625 + 1
    nb, _, _ = synth.make_normal_bursts(n_slots, "cpu", 4, seed=seed, tsc=TSC, p_noise=0.0, p_clip=0.0, amp_range=(2000.0, 8000.0),
                                        snr_range=(20.0, 30.0))
    x = early_read(nb).reshape(-1, 2).numpy().astype(np.float64)
    t = np.arange(n_in) * (65.0 / 96.0)
    wide = np.stack([np.interp(t, np.arange(len(x)), x[:, k]) for k in range(2)], 1)
    wide += rng.standard_normal(wide.shape) * 10.0
    return torch.from_numpy(np.round(wide).clip(-32768, 32767).astype(np.int16)).to("cuda:0")


def state(s):
    out = [s.clock(), s.carried, s.slots(0), s.slots(1)]
    for c in range(s.chans):
        ring, itr, lev = s.noise_state(c)
        out += [ring.tobytes(), itr, np.float32(lev).tobytes(), tuple(sorted(s.counters(c).items()))]
    return out


def host(out):
    return tuple(t.cpu().numpy().reshape(t.shape[0], -1).view(np.uint8) for t in out)


FE_COMBS = ([1, 1, M.COMB_FILL, 1, 1, M.COMB_NONE, 1, 1],)


def test_through_the_resamp_front_end(trx):
    """pull_frontend in runs of 1, 2, 3, ... blocks of 1536 input samples (1040 output samples), alternating with pull_cf32 over
    rows of a second front end, against a second pair of objects that only ever uses trxhip_rx_frontend_pull + pull_cf32: the
    outputs and the carried state byte for byte, slots that begin in the remainder among them"""
    import torch
    block = 1536
    runs = [1, 2, 3, 1, 4, 2, 5]
    wide = resamp_wide(sum(runs), block, 77)
    mk = lambda: trxhip.RxFrontEnd(trx, block, 65, 96, chans=1, mode="resamp")    # noqa: E731
    fe, fe_alt, fe_ref = mk(), mk(), mk()
    s, s_ref = (new_sched(trx, chans=1, combs=FE_COMBS, clock=(40, 1)) for _ in range(2))
    at, found, straddled = 0, 0, 0
    for i, nb in enumerate(runs):
        w = wide[at * block:(at + nb) * block]
        carried = s.carried
        if i % 2 == 0:
            got = s.pull_frontend(fe, w, nb, want_soft=True)
            fe_alt.seed(w, nb)                                           # the other front end has not seen these blocks
        else:
            got = s.pull(fe_alt.pull(w, nb), want_soft=True)
            fe.seed(w, nb)
        want = s_ref.pull(fe_ref.pull(w, nb), want_soft=True)
        torch.cuda.synchronize()
        for a, b in zip(host(got), host(want)):
            assert a.shape == b.shape and np.array_equal(a, b), i
        assert state(s) == state(s_ref), i
        straddled += bool(carried and got[0].shape[1] and i % 2 == 0)
        found += int((s.ind_to_numpy(got[2])["rc"] == M.TSC).sum())
        at += nb
    total = sum(runs) * 1040
    assert s.carried == total - (total - 1) // 625 * 625 and straddled >= 2
    assert found >= 0.75 * ((total - 1) // 625) * 6 / 8 - 1


def test_multi_front_end_is_refused(trx):
    """the reference refuses use_va with multi-ARFCN: TRXHIP_EINVAL, nothing launched, both objects where clean ones are"""
    import torch
    L = trx.L
    rng = np.random.default_rng(5)
    nb = 6
    wide = dev(np.round(rng.standard_normal((nb * 192 * 4, 2)) * 300.0).astype(np.int16))
    fe, fe_c = (trxhip.RxFrontEnd(trx, 192, 65, 48, chans=1) for _ in range(2))
    s, s_c = (new_sched(trx, chans=1, combs=FE_COMBS) for _ in range(2))
    n_out = nb * 260
    k = n_out // 625
    stride = trxhip.RX_SCHED_WORK_HEAD + n_out
    work = torch.full((1, stride), 7.0, dtype=torch.complex64, device="cuda:0")
    pkt = torch.full((1, k, 160), 0xAB, dtype=torch.uint8, device="cuda:0")
    plen = torch.full((1, k), -1, dtype=torch.int16, device="cuda:0")
    ind = torch.full((1, k, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    soft = torch.full((1, k, 148), -7.0, dtype=torch.float32, device="cuda:0")
    ns, nc = C.c_size_t(99), C.c_size_t(99)
    p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731
    rc = L.trxhip_rx_sched_pull_frontend(s.h, fe.h, p(wide), nb, p(work), stride, p(pkt), 160, p(plen), p(ind), p(soft), k, C.byref(ns),
                                         C.byref(nc), trx._stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and (ns.value, nc.value) == (99, 99)
    assert L.trxhip_rx_sched_slots_frontend(s.h, fe.h, nb) == EINVAL
    assert (pkt == 0xAB).all() and (plen == -1).all() and (ind == 0xAB).all() and (soft == -7.0).all() and (work == 7.0).all()
    assert state(s) == state(s_c)
    # the front end's histories too: both give the same rows for the same blocks, and the scheduler takes them
    a, b = fe.pull(wide, nb), fe_c.pull(wide, nb)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    got, want = s.pull(a, want_soft=True), s_c.pull(b, want_soft=True)
    for x, y in zip(host(got), host(want)):
        assert np.array_equal(x, y)
    # the same scheduler without the flag takes the MULTI object
    plain = trxhip.RxScheduler(trx, chans=1, tsc=TSC, full_scale=FULL, max_slots=64)
    plain.set_clock(0, 0)
    assert plain.slots_frontend(fe, nb) == k


def va_unambiguous_bursts(n, tsc, rng):
    """_unambiguous_bursts (test_gpu_tx_frontend.py) for the Viterbi receiver too.  Its channel search (grgsm_vitac.cpp:183-232)
    takes the 20-sample window with the most training-sequence correlation energy among 40 lags round the nominal position, and
    the transmit side's own delay (4.6 symbols, synth.BASE_TOA; the reference's modulateBurst measures the same) puts an on-time
    burst at the late end of that range, burst start 18 of 0 .. 20.  Data bits that resemble the training sequence some symbols
    early then win the search, and the reference's receiver loses the burst whatever carried it (about one random burst in
    200).  The oracle's receiver over the modulated burst 20 samples into its slot tells; such candidates are drawn again."""
    import torch
    import oracle_lib as O
    from test_gpu_tx_frontend import _unambiguous_bursts
    bits = _unambiguous_bursts(np.full(n, tsc), rng)
    todo = np.arange(n)
    while len(todo):
        wave = synth.modulate_laurent_4sps(torch.from_numpy(bits[todo])).numpy() * 6000.0
        lost = []
        for i, w in zip(todo, wave):
            _, soft = O.demod_any_burst_va(np.roll(w, 20).astype(np.complex64), O.TSC, tsc, 30)
            if not np.array_equal(soft[3:145] > 0, bits[i][3:145].astype(bool)):
                lost.append(i)
        todo = np.array(lost, dtype=np.int64)
        bits[todo] = _unambiguous_bursts(np.full(len(todo), tsc), rng)
    return bits


def test_loopback_from_the_transmit_scheduler(trx):
    """TxScheduler.render -> the stream delayed by 20 samples (the early read) -> RxScheduler(use_va=True).  No noise and no
    front end lie between the two, so every submitted burst comes back at its FN / TN with its TSC, and the hard decisions of
    the Viterbi receiver are its bits at 3 .. 144 exactly; the tail bits, zeros the receiver knows, carry no information and
    are not judged, as in the loopbacks of test_gpu_tx_sched.py and test_gpu_rx_sched.py.  Slots without a submitted burst carry
    the dummy filler (no normal burst of this TSC: those loopbacks' bar of 3 % false alarms); the receiver's IDLE and OFF slots
    come out as idle indications with a moving noise level and as nothing"""
    import torch
    chans, n_slots, tsc = 2, 26 * 8, 5
    rng = np.random.default_rng(43)
    slot = np.arange(n_slots)
    bits = [va_unambiguous_bursts(n_slots, tsc, rng) for _ in range(chans)]
    filler = (slot % 7 == 3)                               # channel 0: nothing submitted, the dummy filler goes out
    tx = trxhip.TxScheduler(trx, chans=chans, sps=4, filler=TM.FILLER_DUMMY, full_scale=6000.0, queue_cap=512, max_slots=512)
    tx.set_clock(0, 0)
    for c in range(chans):
        for tn in range(8):
            tx.set_slot(c, tn, 1)
        for i in range(n_slots):
            if not (c == 0 and filler[i]):
                assert tx.submit(c, TM.dgram(i // 8, i % 8, bits[c][i])) >= 0
    x, _ = tx.render(n_slots)
    torch.cuda.synchronize()
    assert x.shape == (chans, n_slots * 625)
    x = torch.cat([torch.zeros((chans, 20), dtype=torch.complex64, device="cuda:0"), x], 1)[:, :n_slots * 625].contiguous()
    rx_combs = ([1] * 8, [1, 1, 1, M.COMB_FILL, 1, 1, M.COMB_NONE, 1])
    rx = trxhip.RxScheduler(trx, chans=chans, tsc=tsc, full_scale=FULL, max_slots=512, use_va=True)
    rx.set_clock(0, 0)
    for c in range(chans):
        rx.set_trxd_version(c, 1)
        for tn in range(8):
            rx.set_slot(c, tn, rx_combs[c][tn])
    pkt, plen, ind, _ = rx.pull(x)
    torch.cuda.synchronize()
    n = n_slots - 1                                        # the last slot waits for one sample more
    assert pkt.shape[1] == n and rx.carried == 625
    pkt, plen, ind = pkt.cpu().numpy(), plen.cpu().numpy(), rx.ind_to_numpy(ind)
    k = np.arange(n)
    for c in range(chans):
        comb = np.array(rx_combs[c])[k % 8]
        sent = comb == 1
        if c == 0:
            sent &= ~filler[:n]
            assert (ind[0]["rc"][filler[:n]] == M.TSC).mean() < 0.03
        assert np.array_equal(ind[c]["fn"], k // 8) and np.array_equal(ind[c]["tn"], k % 8)
        assert (ind[c]["rc"][sent] == M.TSC).all(), (c, np.flatnonzero(sent & (ind[c]["rc"] != M.TSC))[:10])
        assert (ind[c]["tsc"][sent] == tsc).all() and (plen[c][sent] == 11 + 148).all()
        d = pkt[c][sent]
        i = np.flatnonzero(sent)
        assert np.array_equal(d[:, 0], 0x10 | (i % 8)) and np.array_equal(d[:, 4] | (d[:, 3].astype(np.int64) << 8), i // 8)
        wrong = (d[:, 11:159] > 127).astype(np.uint8) != bits[c][:n][sent]
        print("channel", c, "bursts", int(sent.sum()), "wrong bits", int(wrong.sum()), "of them in 3..144", int(wrong[:, 3:145].sum()))
        assert not wrong[:, 3:145].any(), (c, np.argwhere(wrong[:, 3:145])[:10])
    idle, off = np.array(rx_combs[1])[k % 8] == M.COMB_FILL, np.array(rx_combs[1])[k % 8] == M.COMB_NONE
    assert (ind[1]["flags"][idle] == trxhip.ULIND_IDLE).all() and (plen[1][idle] == 11).all() and (ind[1]["rc"][idle] == 0).all()
    assert (ind[1]["flags"][off] == trxhip.ULIND_OFF).all() and (plen[1][off] == 0).all()
    lev = ind[1]["noise_lev"]
    assert lev[0] == 0 and (lev[3:] > 0).all() and (np.diff(lev)[~idle[1:]] == 0).all()     # it moves on IDLE slots alone


def test_outputs_stay_inside_their_slots(trx, scn):
    """the raw C call with output buffers four rows longer than the pull cuts, canary-filled: rows at and beyond n_slots keep
    the canary, the rows in front are the composition's"""
    import torch
    L = trx.L
    want, _ = scn.want(trx, False)
    s = new_sched(trx)
    n = 9 * 625 + 30
    k, cap = 9, 13
    x = scn.stream[:, :n].contiguous()
    pkt = torch.full((2 * k + 4, 160), 0xAB, dtype=torch.uint8, device="cuda:0")
    plen = torch.full((2 * k + 4,), -1, dtype=torch.int16, device="cuda:0")
    ind = torch.full((2 * k + 4, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    soft = torch.full((2 * k + 4, 148), -7.0, dtype=torch.float32, device="cuda:0")
    ns, nc = C.c_size_t(99), C.c_size_t(99)
    p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731
    rc = L.trxhip_rx_sched_pull_s16(s.h, p(x), n, n, p(pkt), 160, p(plen), p(ind), p(soft), cap, C.byref(ns), C.byref(nc), trx._stream())
    torch.cuda.synchronize()
    assert rc == 0 and (ns.value, nc.value) == (k, 30)
    assert (pkt[2 * k:] == 0xAB).all() and (plen[2 * k:] == -1).all() and (ind[2 * k:] == 0xAB).all() and (soft[2 * k:] == -7.0).all()
    for c in range(2):                                                   # outputs are indexed [chan * n_slots + slot]
        w_ind, w_pkt, w_len, w_soft = want[c]
        rows = slice(c * k, (c + 1) * k)
        assert np.array_equal(pkt[rows].cpu().numpy(), w_pkt[:k]) and np.array_equal(plen[rows].cpu().numpy(), w_len[:k])
        assert np.array_equal(raw(soft[rows].cpu().numpy()), raw(w_soft[:k]))
        assert np.array_equal(ind[rows].cpu().numpy().reshape(-1), raw(w_ind[:k]).reshape(-1))


def test_grid_tail(trx):
    """4097 slots of one channel in one pull: one slot more than a multiple of the receiver's eight per workgroup and of the
    prep kernel's four, in int16 and complex64, against the composition over the rows"""
    import torch
    n = 4097
    pool, _, _ = synth.make_normal_bursts(256, "cpu", 4, seed=401, tsc=TSC, p_noise=0.05, p_clip=0.02)
    rng = np.random.default_rng(402)
    rows = early_read(pool)[torch.from_numpy(rng.integers(0, 256, n))]
    x = torch.zeros((1, n * 625 + 1, 2), dtype=torch.int16)
    x[0, :n * 625] = rows.reshape(n * 625, 2)
    x = x.to("cuda:0")
    combs = ([1, 1, 1, M.COMB_FILL, 1, 1, 1, M.COMB_NONE],)
    for cf32 in (False, True):
        s = new_sched(trx, chans=1, max_slots=n, combs=combs)
        m = new_model(1, combs=combs)
        plan = m.cut(n * 625 + 1)[0]
        xin = torch.view_as_complex(x.to(torch.float32)) if cf32 else x
        pkt, plen, ind, soft = s.pull(xin, want_soft=True)
        torch.cuda.synchronize()
        assert pkt.shape == (1, n, 160)
        a = np.array(plan, dtype=np.int64)
        p = np.zeros(n, dtype=trxhip.PARAMS_DTYPE)
        mt = np.zeros(n, dtype=trxhip.TRXD_META_DTYPE)
        mt["fn"], mt["tn"], p["type"], p["max_toa"], p["tsc"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3], TSC
        r = xin[0, :n * 625]
        res_t, w_soft = composition(trx, r.view(n, 625) if cf32 else r.view(n, 625, 2), p)
        w_pkt, w_len = trx.pack_trxd_wire(res_t, trx.params_tensor(p), w_soft, dev(mt.view(np.uint8).reshape(n, 8)), pkt_stride=160)
        torch.cuda.synchronize()
        assert torch.equal(pkt[0], w_pkt) and torch.equal(plen[0], w_len) and torch.equal(soft[0].view(torch.int32), w_soft.view(torch.int32))
        res = trx.results_to_numpy(res_t)
        w_ind = ind_records(m.run(0, plan, res))
        assert np.array_equal(raw(s.ind_to_numpy(ind)[0]), raw(w_ind))
        assert s.counters(0) == m.ctr[0] and (res["rc"] == M.TSC).mean() > 0.6
        s.close()
