"""CPU tests of the air interface (trxhip_air_*, AirChannel): the host object (ctx == NULL, the plain loop over csrc/trx_air.h)
against the numpy model (tests/air_model.py) byte for byte, the identity path, the noise pin and its statistics, rounding and
clamping, every refusal, and the exports.  No GPU is opened."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import air_model as A
import osmo_trx_amd
from osmo_trx_amd import trxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
UL, DL = trxhip.AIR_UL, trxhip.AIR_DL
N = 700
PATHS = [dict(gain=1.0, delay=0, hz=0.0), dict(gain=0.37, delay=7, hz=2000.0), dict(gain=16.0, delay=40, hz=-67.7)]
MAX_DELAY, SEED, RMS = 48, 2024, 12.0
CHUNKS = (1, 5, 63, 64, 65, 625)
FIRST_TS = (0, (1 << 32) - 100, -300)


@functools.lru_cache(maxsize=None)
def tabs():
    t = trxhip.ms_nco_tables_host()
    for x in t:
        x.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def rows3():
    """int16[3, N, 2]: bursts of amplitude ~2500 between zero stretches, so that gain 16 clamps here and there and not always"""
    rng = np.random.default_rng(77)
    x = rng.integers(-2500, 2501, size=(3, N, 2)).astype(np.int16)
    x[0, 100:180] = 0
    x[1, :33] = 0
    x[2, 300:] //= 40
    x[2, 650:] = 0
    x.setflags(write=False)
    return x


def make(cls_args, paths, dirs=(UL, DL), rms=RMS):
    """(host object, model) with the same paths and noise"""
    n = len(paths)
    a, m = trxhip.AirChannel(None, n, *cls_args), A.Air(tabs(), n, *cls_args)
    for d in dirs:
        for k, p in enumerate(paths):
            a.set_path(d, k, **p)
            m.set_path(d, k, **p)
            a.set_noise(d, k, rms)
            m.set_noise(d, k, rms)
    return a, m


@functools.lru_cache(maxsize=None)
def ul_ref(first_ts):
    """the model's uplink of rows3() in one window: the reference every chunking shares"""
    _, m = make((MAX_DELAY, SEED), PATHS)
    y = m.uplink(rows3(), first_ts)
    y.setflags(write=False)
    return y


def in_chunks(call, x, first_ts, chunk, axis, out_axis=0):
    out, n = [], x.shape[axis]
    for k in range(0, n, chunk):
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(k, min(k + chunk, n))
        out.append(call(np.ascontiguousarray(x[tuple(sl)]), first_ts + k))
    return np.concatenate(out, axis=out_axis)


# ---- against the model -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_uplink_equals_the_model(first_ts):
    a, _ = make((MAX_DELAY, SEED), PATHS)
    y = a.uplink(rows3(), first_ts)
    ref = ul_ref(first_ts)
    assert y.dtype == np.int16 and y.shape == (N, 2) and y.tobytes() == ref.tobytes()
    clamped = (np.abs(ref.astype(np.int32)) >= 32767).mean()
    assert 0.0 < clamped < 0.9                                     # both sides of the clamp are in the case
    assert a.path_state(UL, 0)["end_ts"] == first_ts + N


@pytest.mark.parametrize("chunk", CHUNKS)
def test_uplink_chunking_changes_no_bit(chunk):
    """also where n < d: chunks of 1 and 5 under delays 7 and 40"""
    for first_ts in (0, (1 << 32) - 100):
        a, _ = make((MAX_DELAY, SEED), PATHS)
        y = in_chunks(a.uplink, rows3(), first_ts, chunk, 1)
        assert y.tobytes() == ul_ref(first_ts).tobytes(), (chunk, first_ts)


def test_model_chunked_equals_model_whole():
    _, m = make((MAX_DELAY, SEED), PATHS)
    assert in_chunks(m.uplink, rows3(), -300, 65, 1).tobytes() == ul_ref(-300).tobytes()


def test_a_longer_history_changes_nothing():
    a, _ = make((65536, SEED), PATHS)
    assert in_chunks(a.uplink, rows3(), 0, 5, 1).tobytes() == ul_ref(0).tobytes()


def test_set_path_between_windows():
    """the phase is continuous, gain and delay jump, and the state is the model's"""
    a, m = make((MAX_DELAY, SEED), PATHS)
    x = rows3()
    out = [[], []]
    for k, (lo, hi) in enumerate(((0, 300), (300, 520), (520, N))):
        if k == 1:
            for o in (a, m):
                o.set_path(UL, 1, gain=0.5, delay=31, hz=-1234.5)
                o.set_path(UL, 2, gain=2.0, delay=0, hz=0.0)        # off: phase 0
        if k == 2:
            for o in (a, m):
                o.set_path(UL, 2, gain=2.0, delay=48, hz=500000.0)  # on from off: starts at phase 0
                o.set_noise(UL, 0, 100.0)
        for j, o in enumerate((a, m)):
            out[j].append(o.uplink(np.ascontiguousarray(x[:, lo:hi]), 1000 + lo))
        for k2 in range(3):
            st = a.path_state(UL, k2)
            assert {f: st[f].item() for f in st.dtype.names} == m.path_state(UL, k2), (k, k2)
    assert np.concatenate(out[0]).tobytes() == np.concatenate(out[1]).tobytes()
    st = a.path_state(UL, 1)
    assert st["ts_ref"] == 1300 and st["acc"] == A.NM.phase(0, 0, A.NM.inc_of(2000.0), 1300) and st["delay"] == 31
    assert a.path_state(UL, 2)["acc"] == 0 and a.path_state(UL, 2)["ts_ref"] == 1520


@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_downlink_equals_the_model(first_ts):
    a, m = make((MAX_DELAY, SEED), PATHS)
    x = rows3()[0]
    ref = m.downlink(x, first_ts)
    assert a.downlink(x, first_ts).tobytes() == ref.tobytes() and ref.shape == (3, N, 2)
    # the members' receivers have their own noise: the same path on two members differs by the noise alone
    c, _ = make((MAX_DELAY, SEED), [PATHS[1], PATHS[1]])
    y = c.downlink(x, first_ts)
    assert not np.array_equal(y[0], y[1]) and np.abs(y[0].astype(np.int32) - y[1]).max() < 200


def test_downlink_chunking_changes_no_bit():
    x = rows3()[0]
    _, m = make((MAX_DELAY, SEED), PATHS)
    ref = m.downlink(x, (1 << 32) - 100)
    for chunk in (5, 63, 64):
        a, _ = make((MAX_DELAY, SEED), PATHS)
        parts = [a.downlink(np.ascontiguousarray(x[k:k + chunk]), (1 << 32) - 100 + k) for k in range(0, N, chunk)]
        assert np.array_equal(np.concatenate(parts, axis=1), ref), chunk


def test_reset_forgets_the_past():
    a, m = make((MAX_DELAY, SEED), PATHS)
    x = rows3()
    for o in (a, m):
        o.uplink(np.ascontiguousarray(x[:, :200]), 0)
        o.reset(UL, 5000)
    assert a.path_state(UL, 0)["end_ts"] == 5000
    with pytest.raises(trxhip.TrxHipError):
        a.uplink(np.ascontiguousarray(x[:, 200:]), 200)
    y, ref = (o.uplink(np.ascontiguousarray(x[:, 200:]), 5000) for o in (a, m))
    assert y.tobytes() == ref.tobytes()
    fresh, _ = make((MAX_DELAY, SEED), PATHS)
    fresh.reset(UL, 5000)
    assert fresh.uplink(np.ascontiguousarray(x[:, 200:]), 5000).tobytes() == y.tobytes()


def test_identity_path_returns_its_input():
    x = rows3()[0]
    for first_ts in (0, -77, 1 << 40):
        a = trxhip.AirChannel(None, 1)
        assert a.uplink(x[None], first_ts).tobytes() == x.tobytes()
        assert a.downlink(x, first_ts)[0].tobytes() == x.tobytes()
    edge = np.array([[32767, -32768], [-32768, 32767], [0, 1], [-1, 0]], dtype=np.int16)
    assert trxhip.AirChannel(None, 1).uplink(edge[None], 3).tobytes() == edge.tobytes()
    a = trxhip.AirChannel(None, 1, 8)
    a.set_path(UL, 0, 1.0, 0, 2000.0)
    a.uplink(x[None], 0)
    a.set_path(UL, 0, 1.0, 0, 0.0)                                  # back to hz = 0: phase 0 again
    assert a.uplink(x[None], N).tobytes() == x.tobytes()


# ---- the noise ------------------------------------------------------------------------------------------------------------------------

def test_noise_pin():
    ts = [0, 1, 2, 1 << 32, 1 << 63]
    assert list(A.noise_s(2024, 3, ts)) == [34, 185, -111, -16, 259]
    assert [trxhip.air_noise_host(2024, 3, t) for t in ts] == [34, 185, -111, -16, 259]
    assert A.noise_scale(8192.0) == 3632402 and A.noise_scale(8192.0) * 510 < 1 << 31
    for bad in (-1, 3632403, (1 << 31) - 1, -(1 << 31)):                 # outside the range: 0, the product is never formed
        assert trxhip.air_noise_host(2024, 3, 1, bad) == 0
    assert trxhip.air_noise_host(2024, 3, 1, 3632402) == int(A.nq(3632402, np.int64(185)))
    rng = np.random.default_rng(5)
    for seed, lane, t, scale in zip(rng.integers(0, 1 << 32, 50), rng.integers(0, 8194, 50), rng.integers(-(1 << 63), 1 << 63, 50),
                                    rng.integers(0, 3632403, 50)):
        s = A.noise_s(int(seed), int(lane), [int(t)])
        assert trxhip.air_noise_host(int(seed), int(lane), int(t), int(scale)) == int(A.nq(int(scale), s)[0])


def test_noise_statistics():
    """10^6 samples of three lanes (member 0's I and Q, the BTS's I) under bars derived from n: 5 sigma of the estimator of a
    mean (sigma / sqrt(n)), of a variance (sqrt((kurtosis - 1) / n), kurtosis 2.7) and of a correlation (1 / sqrt(n))"""
    n = 1000000
    ts = (np.arange(n, dtype=np.int64) + ((1 << 32) - n // 2)).view(np.uint64)     # across a carry into hi
    lanes = [A.noise_s(SEED, lane, ts).astype(np.float64) for lane in (0, 1, 2 * A.UL_RX)]
    for s in lanes:
        assert s.min() >= -510 and s.max() <= 510
        mean, var = s.mean(), s.var()
        print(f"mean {mean:+.4f} (bar {5 * 147.8 / np.sqrt(n):.4f})  var / 21845 - 1 = {var / 21845 - 1:+.5f} (bar {5 * np.sqrt(1.7 / n):.5f})")
        assert abs(mean) <= 5 * 147.8 / np.sqrt(n)
        assert abs(var / 21845.0 - 1.0) <= 5 * np.sqrt(1.7 / n)

    def corr(u, v):
        return np.mean((u - u.mean()) * (v - v.mean())) / (u.std() * v.std())

    for name, c in (("I-Q", corr(lanes[0], lanes[1])), ("two lanes", corr(lanes[0], lanes[2])), ("lag 1", corr(lanes[0][:-1], lanes[0][1:]))):
        print(f"corr {name}: {c:+.5f} (bar {5 / np.sqrt(n):.5f})")
        assert abs(c) <= 5 / np.sqrt(n)


def test_noise_level_of_the_object():
    """zero input: the output is the receiver's noise, rms as set, the model's bytes"""
    a, m = make((0, SEED), [dict()], rms=300.0)
    z = np.zeros((1, 20000, 2), np.int16)
    y = a.uplink(z, 123)
    assert y.tobytes() == m.uplink(z, 123).tobytes()
    assert abs(y.astype(np.float64).std() / 300.0 - 1.0) < 0.02
    d = a.downlink(z[0], 123)
    assert d.tobytes() == m.downlink(z[0], 123).tobytes() and not np.array_equal(d[0], y)


# ---- rounding and clamping ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("acc, out", [(-129, -1), (-128, 0), (127, 0), (128, 1)])
def test_rounding(acc, out):
    """one member, hz 0: c = x * gain * 256 exactly, so x = +-1 at gain |acc| / 256 puts acc itself in front of the shift"""
    a = trxhip.AirChannel(None, 1)
    a.set_path(UL, 0, abs(acc) / 256.0, 0, 0.0)
    a.set_path(DL, 0, abs(acc) / 256.0, 0, 0.0)
    x = np.array([[np.sign(acc), 0], [0, np.sign(acc)]], dtype=np.int16)
    want = np.array([[out, 0], [0, out]], dtype=np.int16)
    assert np.array_equal(a.uplink(x[None], 0), want) and np.array_equal(a.downlink(x, 0)[0], want)
    assert np.array_equal(A.finish(np.array([acc])), [out])


def test_two_full_scale_members_clamp_at_both_rails():
    x = np.array([[32767, -32768], [-32768, 32767]], dtype=np.int16)
    rows = np.stack([x, x])
    a, m = make((0, 0), [dict(), dict()], rms=0.0)
    y = a.uplink(rows, 0)
    assert np.array_equal(y, x) and y.tobytes() == m.uplink(rows, 0).tobytes()
    a.set_path(UL, 1, 1.0, 0, 0.0)
    a.set_path(UL, 0, 0.0, 0, 0.0)                                  # gain 0: the member is silent
    assert np.array_equal(a.uplink(rows, 2), x)
    b = trxhip.AirChannel(None, 1)
    b.set_path(DL, 0, 16.0, 0, 0.0)
    assert np.array_equal(b.downlink(x, 0)[0], x)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def snapshot(a, n):
    return [a.path_state(d, m).tobytes() for d in (UL, DL) for m in range(n)]


def test_refusals_change_nothing():
    L = trxhip.load_library()
    h = C.c_void_p()
    for n_members, max_delay in ((0, 0), (4097, 0), (1, 65537), (0xFFFFFFFF, 0)):
        cfg = trxhip._AirCfg(n_members, max_delay, 0, 0)
        assert L.trxhip_air_create(None, C.byref(cfg), C.byref(h)) == EINVAL and not h.value
    ok = trxhip._AirCfg(1, 0, 0, 0)
    assert L.trxhip_air_create(None, None, C.byref(h)) == EINVAL and L.trxhip_air_create(None, C.byref(ok), None) == EINVAL
    for n_members, max_delay in ((0, 0), (-1, 0), (4097, 0), (1, -1), (1, 65537), (1 - (1 << 32), 0)):   # nothing wraps into range
        with pytest.raises(trxhip.TrxHipError):
            trxhip.AirChannel(None, n_members, max_delay)
    for n_members, max_delay in ((4096, 0), (1, 65536)):
        trxhip.AirChannel(None, n_members, max_delay).close()

    a, m = make((MAX_DELAY, SEED), PATHS)
    x = rows3()
    a.uplink(np.ascontiguousarray(x[:, :100]), 10)
    a.downlink(np.ascontiguousarray(x[0, :50]), -20)
    before = snapshot(a, 3)

    def path(gain=1.0, delay=0, hz=0.0):
        return C.byref(trxhip._AirPath(gain, delay, hz))

    for d in (UL, DL):
        for bad in (path(delay=MAX_DELAY + 1), path(gain=16.0001), path(gain=-0.001), path(gain=float("nan")), path(gain=float("inf")),
                    path(hz=500000.1), path(hz=-500000.1), path(hz=float("nan")), None):
            assert L.trxhip_air_set_path(a.h, d, 1, bad) == EINVAL
        assert L.trxhip_air_set_path(a.h, d, 3, path()) == EINVAL and L.trxhip_air_set_path(None, d, 0, path()) == EINVAL
        for rms in (-0.001, 8192.001, float("nan"), float("inf")):
            assert L.trxhip_air_set_noise(a.h, d, 0, rms) == EINVAL
        assert L.trxhip_air_path_state(a.h, d, 3, None) == EINVAL and L.trxhip_air_path_state(a.h, d, 0, None) == EINVAL
    assert L.trxhip_air_set_noise(a.h, DL, 3, 1.0) == EINVAL and L.trxhip_air_set_noise(None, UL, 0, 1.0) == EINVAL
    for d in (2, -1):
        assert L.trxhip_air_set_path(a.h, d, 0, path()) == EINVAL and L.trxhip_air_set_noise(a.h, d, 0, 1.0) == EINVAL
        assert L.trxhip_air_reset(a.h, d, 0) == EINVAL
    assert L.trxhip_air_reset(None, UL, 0) == EINVAL

    for member, delay in ((-1, 0), (3, 0), (0, -1), (0, (1 << 32) + 1), (1 << 32, 0)):
        with pytest.raises(trxhip.TrxHipError):
            a.set_path(UL, member, 1.0, delay, 0.0)
    assert snapshot(a, 3) == before

    rows = np.ascontiguousarray(x[:, 100:200])
    out = np.full((101, 2), 0x5A5A, dtype=np.int16)
    po, pr = out.ctypes.data, rows.ctypes.data
    ul, dl = L.trxhip_air_uplink_s16, L.trxhip_air_downlink_s16
    assert ul(a.h, pr, 100, 111, 100, po, None) == EINVAL          # not contiguous: end_ts is 110
    assert ul(a.h, pr, 100, 109, 100, po, None) == EINVAL
    assert ul(a.h, pr, 99, 110, 100, po, None) == EINVAL           # stride < n
    assert ul(a.h, pr, 100, 110, 0, po, None) == EINVAL
    assert ul(a.h, pr, 1 << 31, 110, 1 << 31, po, None) == EINVAL
    assert ul(a.h, None, 100, 110, 100, po, None) == EINVAL and ul(a.h, pr, 100, 110, 100, None, None) == EINVAL
    assert ul(a.h, pr + 2, 100, 110, 99, po, None) == EINVAL and ul(a.h, pr, 100, 110, 100, po + 2, None) == EINVAL
    assert ul(None, pr, 100, 110, 100, po, None) == EINVAL
    big = np.zeros((3, 30, 2), np.int16)
    assert dl(a.h, pr, 31, 30, big.ctypes.data, 30, None) == EINVAL  # not contiguous: end_ts is 30
    assert dl(a.h, pr, 30, 30, big.ctypes.data, 29, None) == EINVAL  # stride < n
    assert dl(a.h, pr, 30, 0, big.ctypes.data, 30, None) == EINVAL
    assert dl(a.h, None, 30, 30, big.ctypes.data, 30, None) == EINVAL and dl(a.h, pr, 30, 30, None, 30, None) == EINVAL
    assert dl(a.h, pr + 2, 30, 30, big.ctypes.data, 30, None) == EINVAL and dl(a.h, pr, 30, 30, big.ctypes.data + 2, 30, None) == EINVAL
    assert (out == 0x5A5A).all() and not big.any()
    assert snapshot(a, 3) == before
    # and the windows go on as if nothing had been asked
    m.uplink(np.ascontiguousarray(x[:, :100]), 10)
    assert a.uplink(rows, 110).tobytes() == m.uplink(rows, 110).tobytes()
    # the limits themselves pass
    a.set_path(UL, 0, 16.0, MAX_DELAY, 500000.0)
    a.set_path(DL, 2, 0.0, 0, -500000.0)
    a.set_noise(UL, 99, 8192.0)                                     # the member is ignored on the uplink
    assert a.path_state(UL, 2)["noise_scale"] == 3632402 and a.path_state(UL, 0)["inc"] == A.NM.inc_of(500000.0)


# ---- exports ----------------------------------------------------------------------------------------------------------------------------------

def test_symbols_header_and_abi():
    L = trxhip.load_library()
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    names = ["trxhip_air_" + x for x in ("create", "destroy", "set_path", "set_noise", "path_state", "reset", "uplink_s16", "downlink_s16",
                                         "noise_host")]
    for name in names:
        assert hasattr(L, name) and name in trxhip.SYMBOLS and name + "(" in hdr, name
    assert sorted(s for s in trxhip.SYMBOLS if s.startswith("trxhip_air_")) == sorted(names)
    assert L.trxhip_abi_version() == 5 and re.search(r"^#define\s+TRXHIP_ABI_VERSION\s+5\b", hdr, re.M)
    for name in ("AirChannel", "AIR_UL", "AIR_DL"):
        assert getattr(osmo_trx_amd, name) is getattr(trxhip, name) and name in osmo_trx_amd.__all__
    assert (trxhip.AIR_UL, trxhip.AIR_DL) == (0, 1) and re.search(r"^#define\s+TRXHIP_AIR_DL\s+1\b", hdr, re.M)
    from test_ms_afc_cpu import struct_fields
    assert struct_fields(hdr, "trxhip_air_path_status") == list(trxhip.AIR_PATH_STATE_DTYPE.names)
    assert "typedef struct trxhip_air_path_status {  /* 48 bytes */" in hdr
    buf = np.full(48 + 16, 0xA5, dtype=np.uint8)
    a = trxhip.AirChannel(None, 2, 5, 9)
    assert L.trxhip_air_path_state(a.h, DL, 1, buf.ctypes.data_as(C.c_void_p)) == 0 and (buf[48:] == 0xA5).all()
    st = a.path_state(DL, 1)
    assert (st["gain"], st["delay"], st["hz"], st["inc"], st["acc"], st["noise_scale"], st["started"], st["end_ts"]) == (1.0, 0, 0.0, 0, 0, 0, 0, 0)
