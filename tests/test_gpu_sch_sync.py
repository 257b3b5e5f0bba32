"""GPU parity of the MS-side SCH receiver: trxhip_sch_sync_batch_cf32 / _i16 vs the CPU model tests/sch_sync_model.py (pinned to
the C oracle by tests/test_sch_sync_cpu.py).  The +-127 outputs are hard decisions and the burst position comes out of a serial
float recurrence, so every comparison is equality: start, corr_max (bit for bit), the 148 sbits, rc and the decoded fields."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sch_sync_model as M
from osmo_trx_amd import synth, trxhip

pytestmark = pytest.mark.gpu

SCALE = 1.0 / 2047.0
EINVAL = -22


@pytest.fixture(scope="module")
def trx():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def _wave(bsic, fn):
    return O.modulate_burst(synth.sch_burst_bits(bsic, fn), 8, 4)


def _buffer(rng, L, off=None, snr_db=25.0, amp=3000.0, bsic=0, fn=1):
    """L samples of noise (amp / snr below the burst's amplitude) with an SCH burst `off` samples in (None: noise only)."""
    sigma = amp * 10 ** (-snr_db / 20) / np.sqrt(2)
    y = ((rng.normal(size=L) + 1j * rng.normal(size=L)) * sigma).astype(np.complex64)
    if off is not None and off < L:
        w = _wave(bsic, fn)
        m = min(len(w), L - off)
        y[off:off + m] += w[:m] * np.complex64(amp * np.exp(1j * rng.uniform(0, 2 * np.pi)))
    return y


def _cases(rng, n, L, offsets, snrs=(25.0, 10.0, 0.0)):
    """n buffers cycling through offsets x SNRs; every 11th is noise only, every 13th all zero.  Returns (buffers, truth) with
    truth[b] = (bsic, fn, off, snr) or None where nothing decodable was sent."""
    bufs, truth = [], []
    for b in range(n):
        if b % 13 == 12:
            bufs.append(np.zeros(L, dtype=np.complex64))
            truth.append(None)
        elif b % 11 == 10:
            bufs.append(_buffer(rng, L, None, amp=float(10 ** rng.uniform(0, 4))))
            truth.append(None)
        else:
            off, snr = int(offsets[b % len(offsets)]), float(snrs[(b // len(offsets)) % len(snrs)])
            bsic, fn = int(rng.integers(0, 64)), int(synth.random_sch_frames(1, rng)[0])
            bufs.append(_buffer(rng, L, off, snr, amp=float(10 ** rng.uniform(2.5, 4.0)), bsic=bsic, fn=fn))
            truth.append((bsic, fn, off, snr))
    return bufs, truth


def _run(trx, bufs, mode, stride=None, want_bits=True, scale=SCALE):
    import torch
    L = len(bufs[0])
    x = np.zeros((len(bufs), stride or L), dtype=np.complex64)
    x[:, L:] = 1e4 + 1e4j                                          # between the buffers: must never be read
    for b, y in enumerate(bufs):
        x[b, :L] = y
    return trx.sch_sync(torch.from_numpy(x).to("cuda:0"), mode, scale=scale, want_bits=want_bits, buf_len=L)


def _check(rec, bits, bufs, mode, truth=None, max_off=39, scale=SCALE):
    for b, y in enumerate(bufs):
        m = M.sch_sync(y, mode, scale)
        got = rec[b]
        assert got["start"] == m["start"], (b, got["start"], m["start"])
        assert np.float32(got["corr_max"]).view(np.uint32) == np.float32(m["corr_max"]).view(np.uint32), b
        assert np.array_equal(bits[b], m["bits"]), b
        for f in ("rc", "fn", "t1", "bsic", "t2", "t3p"):
            assert got[f] == m[f], (b, f, got[f], m[f])
        assert not got["reserved"].any()
        if truth is not None and truth[b] is not None:
            bsic, fn, off, snr = truth[b]
            if snr >= 10.0 and off <= max_off:
                assert (got["rc"], got["bsic"], got["fn"]) == (1, bsic, fn), (b, truth[b])
                assert (got["t1"], got["t2"], got["t3p"]) == (fn // 1326, fn % 26, (fn % 51 - 1) // 10)


TRACK_OFFSETS = list(range(40)) + [60]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 130])
def test_track_equals_model(trx, n):
    rng = np.random.default_rng(200 + n)
    offs = TRACK_OFFSETS if n > 9 else [int(o) for o in rng.choice(TRACK_OFFSETS, n)]
    bufs, truth = _cases(rng, n, 625, offs)
    rec, bits = _run(trx, bufs, trxhip.SCH_SYNC_TRACK)
    _check(rec, bits, bufs, M.TRACK, truth)


@pytest.mark.parametrize("L", [600, 157, 700])
def test_track_lengths_and_stride(trx, L):
    """Shorter slots read zeros behind their end, samples past 625 are ignored (the model cuts there), and a stride above the
    length never reads the gap."""
    rng = np.random.default_rng(300 + L)
    bufs, truth = _cases(rng, 14, L, [0, 3, 17, 39, 60, 8])
    rec, bits = _run(trx, bufs, trxhip.SCH_SYNC_TRACK, stride=L + 37)
    # a burst `off` samples in is whole only when its 148 symbols and the filter's tail lie inside the slot, off + 600 <= L;
    # a burst that is cut off is compared with the model only
    _check(rec, bits, bufs, M.TRACK, truth, max_off=min(39, L - 600))


@pytest.mark.parametrize("L,offsets", [(532, [0]), (533, [0]), (1250, [0, 7, 300]), (5000, [0, 7, 300, 1250, 2503, 4300])])
def test_acq_equals_model(trx, L, offsets):
    rng = np.random.default_rng(400 + L)
    bufs, truth = _cases(rng, 13, L, offsets, snrs=(25.0, 10.0))
    if L < 1250:
        truth = None                                               # one / two windows: the burst does not fit, equality only
    rec, bits = _run(trx, bufs, trxhip.SCH_SYNC_ACQ, stride=L + 5)
    # the search reaches lag len - 513: a burst at offset o has its window near lag o + 188
    _check(rec, bits, bufs, M.ACQ, truth, max_off=L - 512 - 188 - 25)
    if L == 5000:
        # the 20-sample energy window is coarse by design: the estimate lies within one window of the true position
        assert all(abs(int(rec[b]["start"]) - t[2]) < 20 for b, t in enumerate(truth) if t and t[2] <= 2503)


def test_acq_full_length_buffers(trx):
    """Two buffers of the reference's 12 frames: a burst in the middle, and one behind the last lag (equality only)."""
    rng = np.random.default_rng(500)
    sent = [(17, 1234 * 51 + 11, 31111), (42, 999 * 51 + 41, 59200)]
    bufs = [_buffer(rng, 60000, off, 20.0, bsic=bsic, fn=fn) for bsic, fn, off in sent]
    rec, bits = _run(trx, bufs, trxhip.SCH_SYNC_ACQ)
    _check(rec, bits, bufs, M.ACQ)
    assert (rec[0]["rc"], rec[0]["bsic"], rec[0]["fn"]) == (1, 17, 1234 * 51 + 11)
    assert abs(int(rec[0]["start"]) - 31111) < 20


@pytest.mark.parametrize("mode,L", [(trxhip.SCH_SYNC_TRACK, 625), (trxhip.SCH_SYNC_ACQ, 3000)])
def test_int16_entry_equals_cf32(trx, mode, L):
    import torch
    rng = np.random.default_rng(600 + L)
    bufs, _ = _cases(rng, 9, L, [0, 5, 39, 22])
    q = np.stack([np.stack([np.round(y.real), np.round(y.imag)], axis=-1) for y in bufs]).clip(-32768, 32767).astype(np.int16)
    xi = torch.from_numpy(q).to("cuda:0")
    xf = torch.from_numpy((q[..., 0].astype(np.float32) + 1j * q[..., 1].astype(np.float32)).astype(np.complex64)).to("cuda:0")
    ri, bi = trx.sch_sync(xi, mode, scale=SCALE, want_bits=True)
    rf, bf = trx.sch_sync(xf, mode, scale=SCALE, want_bits=True)
    assert ri.tobytes() == rf.tobytes() and np.array_equal(bi, bf)
    m = M.sch_sync(q[0], mode, SCALE)                              # and the model's int16 path
    assert (ri[0]["start"], ri[0]["rc"], ri[0]["fn"]) == (m["start"], m["rc"], m["fn"]) and np.array_equal(bi[0], m["bits"])
    assert ri["rc"].sum() >= 5


@pytest.mark.parametrize("mode,L", [(trxhip.SCH_SYNC_TRACK, 625), (trxhip.SCH_SYNC_ACQ, 2000)])
def test_batch_position(trx, mode, L):
    rng = np.random.default_rng(700 + L)
    n = 11
    bufs, _ = _cases(rng, n, L, [3, 9, 30])
    probe = _buffer(rng, L, 12, 15.0, bsic=33, fn=51 * 77 + 21)
    for k in (0, 3, n - 1):
        bufs[k] = probe
    rec, bits = _run(trx, bufs, mode)
    for k in (3, n - 1):
        assert rec[k].tobytes() == rec[0].tobytes() and np.array_equal(bits[k], bits[0])
    assert (rec[0]["rc"], rec[0]["bsic"], rec[0]["fn"]) == (1, 33, 51 * 77 + 21)


@pytest.mark.parametrize("mode", [trxhip.SCH_SYNC_TRACK, trxhip.SCH_SYNC_ACQ])
def test_loopback_through_the_product_modulator(trx, mode):
    iq, truth = synth.make_sch_buffers(10, "cuda:0", mode, trx, snr_db=20.0)
    rec = trx.sch_sync(iq, mode, scale=SCALE)
    assert (rec["rc"] == 1).all()
    assert np.array_equal(rec["bsic"], truth["bsic"]) and np.array_equal(rec["fn"], truth["fn"])
    assert (np.abs(rec["start"] - truth["offset"]) < 20).all()


@pytest.mark.parametrize("mode,L", [(trxhip.SCH_SYNC_TRACK, 625), (trxhip.SCH_SYNC_ACQ, 1500)])
def test_null_bits_gives_the_same_records(trx, mode, L):
    rng = np.random.default_rng(800 + L)
    bufs, _ = _cases(rng, 7, L, [0, 20, 39])
    rec, _ = _run(trx, bufs, mode)
    rec0 = _run(trx, bufs, mode, want_bits=False)
    assert rec.tobytes() == rec0.tobytes()


def test_refusals_leave_the_outputs_untouched(trx):
    import torch
    L = trx.L
    x = torch.zeros((2, 1000), dtype=torch.complex64, device="cuda:0")
    xi = torch.zeros((2, 1000, 2), dtype=torch.int16, device="cuda:0")
    big = torch.zeros((1, trxhip.SCH_SYNC_MAX_LEN + 1), dtype=torch.complex64, device="cuda:0")
    res = torch.full((2, 24), 0xAB, dtype=torch.uint8, device="cuda:0")
    bits = torch.full((2, 148), 0x5A, dtype=torch.int8, device="cuda:0")
    vp = C.c_void_p
    st = trx._stream()
    P = lambda t: vp(t.data_ptr())
    TRACK, ACQ = trxhip.SCH_SYNC_TRACK, trxhip.SCH_SYNC_ACQ
    for fn, xin in ((L.trxhip_sch_sync_batch_cf32, x), (L.trxhip_sch_sync_batch_i16, xi)):
        calls = [
            (trx.h, P(xin), 1000, P(res), P(bits), 2, 625, 2, SCALE, st),        # unknown mode
            (trx.h, P(xin), 1000, P(res), P(bits), 2, 625, -1, SCALE, st),
            (trx.h, P(xin), 1000, P(res), P(bits), 0, 625, TRACK, SCALE, st),    # n_bufs == 0
            (vp(0), P(xin), 1000, P(res), P(bits), 2, 625, TRACK, SCALE, st),    # NULL pointers
            (trx.h, vp(0), 1000, P(res), P(bits), 2, 625, TRACK, SCALE, st),
            (trx.h, P(xin), 1000, vp(0), P(bits), 2, 625, TRACK, SCALE, st),
            (trx.h, P(xin), 624, P(res), P(bits), 2, 625, TRACK, SCALE, st),     # buf_stride < buf_len
            (trx.h, P(xin), 1000, P(res), P(bits), 2, 0, TRACK, SCALE, st),      # TRACK: buf_len < 1
            (trx.h, P(xin), 1000, P(res), P(bits), 2, 531, ACQ, SCALE, st),      # ACQ: fewer than one window
        ]
        for a in calls:
            assert fn(*a) == EINVAL, a[5:8]
    assert L.trxhip_sch_sync_batch_cf32(trx.h, P(big), big.shape[1], P(res), P(bits), 1, big.shape[1], ACQ, SCALE, st) == EINVAL
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 0xAB).all() and (bits.cpu().numpy() == 0x5A).all()
    # the shortest lengths that are accepted
    assert L.trxhip_sch_sync_batch_cf32(trx.h, P(x), 1000, P(res), P(bits), 2, 1, TRACK, SCALE, st) == 0
    assert L.trxhip_sch_sync_batch_cf32(trx.h, P(x), 1000, P(res), P(bits), 2, 532, ACQ, SCALE, st) == 0
    torch.cuda.synchronize()
    assert (bits.cpu().numpy() != 0x5A).all()
