"""CPU tests of the air interface's multipath rays (trxhip_multipath_*, AirChannel.set_rays / rays, air_rays): the host object
(ctx == NULL, the plain loop over csrc/trx_air.h) against the numpy model (tests/air_rays_model.py) byte for byte, chunking, the
equivalences that pin a ray to a path of the object as it was, set_rays between windows, every refusal, the exports and the
profile helper.  No GPU is opened."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import air_rays_model as R
import osmo_trx_amd
from osmo_trx_amd import trxhip
from test_air_cpu import CHUNKS, FIRST_TS, MAX_DELAY, N, RMS, SEED, in_chunks, rows3, tabs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
UL, DL = trxhip.AIR_UL, trxhip.AIR_DL
NM = R.NM

PLAIN0 = dict(gain=0.37, delay=7, hz=2000.0)
RAYS1 = [dict(gain=1.0, delay=0, hz=0.0, phase=0), dict(gain=0.5, delay=2, hz=0.0, phase=1 << 30),
         dict(gain=16.0, delay=40, hz=-67.7, phase=12345)]


@functools.lru_cache(maxsize=None)
def rays64():
    """64 rays of small gains, every third one static, delays 0 .. 48 with both ends in"""
    rng = np.random.default_rng(64)
    out = []
    for k in range(64):
        hz = 0.0 if k % 3 == 0 else float(rng.uniform(-300.0, 300.0)) if k % 3 == 1 else float(rng.uniform(-500000.0, 500000.0))
        out.append(dict(gain=float(np.float32(rng.uniform(0.0, 0.12))), delay=(0, 48)[k] if k < 2 else int(rng.integers(0, 49)), hz=hz,
                        phase=int(rng.integers(0, 1 << 32))))
    return tuple(out)


def case1(o, dirs=(UL, DL), rms=RMS):
    """member 0 plain, member 1 three rays, member 2 sixty-four; o: an AirChannel or the model"""
    for d in dirs:
        o.set_path(d, 0, **PLAIN0)
        o.set_rays(d, 1, RAYS1)
        o.set_rays(d, 2, list(rays64()))
        for m in range(3):
            o.set_noise(d, m, rms)
    return o


def make(n=3, max_delay=MAX_DELAY, seed=SEED):
    return trxhip.AirChannel(None, n, max_delay, seed), R.AirRays(tabs(), n, max_delay, seed)


@functools.lru_cache(maxsize=None)
def ul_ref(first_ts):
    y = case1(make()[1]).uplink(rows3(), first_ts)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def dl_ref(first_ts):
    y = case1(make()[1]).downlink(rows3()[0], first_ts)
    y.setflags(write=False)
    return y


# ---- 1. against the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_uplink_equals_the_model(first_ts):
    a = case1(make()[0])
    y, ref = a.uplink(rows3(), first_ts), ul_ref(first_ts)
    assert y.dtype == np.int16 and y.shape == (N, 2) and y.tobytes() == ref.tobytes()
    clamped = (np.abs(ref.astype(np.int32)) >= 32767).mean()
    assert 0.0 < clamped < 0.9
    plain = trxhip.AirChannel(None, 3, MAX_DELAY, SEED)
    plain.set_path(UL, 0, **PLAIN0)
    plain.set_noise(UL, 0, RMS)
    assert plain.uplink(rows3(), first_ts).tobytes() != ref.tobytes()          # the rays are in the output


@pytest.mark.parametrize("first_ts", FIRST_TS)
def test_downlink_equals_the_model(first_ts):
    a = case1(make()[0])
    y, ref = a.downlink(rows3()[0], first_ts), dl_ref(first_ts)
    assert y.shape == (3, N, 2) and y.tobytes() == ref.tobytes()
    assert 0.0 < (np.abs(ref.astype(np.int32)) >= 32767).mean() < 0.9


# ---- 2. chunking ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunking_changes_no_bit(chunk):
    """also where n < delay: chunks of 1 and 5 under delays up to 48"""
    first_ts = (1 << 32) - 100
    a = case1(make()[0])
    assert in_chunks(a.uplink, rows3(), first_ts, chunk, 1).tobytes() == ul_ref(first_ts).tobytes()
    if chunk in (5, 63, 64):
        assert in_chunks(a.downlink, rows3()[0], first_ts, chunk, 0, out_axis=1).tobytes() == dl_ref(first_ts).tobytes()


def test_model_chunked_equals_model_whole():
    m = case1(make()[1])
    assert in_chunks(m.uplink, rows3(), -300, 65, 1).tobytes() == ul_ref(-300).tobytes()


# ---- 3. equivalences ----------------------------------------------------------------------------------------------------------------------

def test_one_static_ray_is_the_plain_path():
    x = rows3()
    for g, d in ((1.0, 0), (0.37, 7), (16.0, 48)):
        a, b = (trxhip.AirChannel(None, 3, MAX_DELAY, SEED) for _ in range(2))
        for dir in (UL, DL):
            a.set_rays(dir, 1, [dict(gain=g, delay=d, hz=0.0, phase=0)])
            b.set_path(dir, 1, g, d, 0.0)
            for o in (a, b):
                o.set_noise(dir, 1, RMS)
        assert a.uplink(x, -5).tobytes() == b.uplink(x, -5).tobytes()
        assert a.downlink(x[1], 77).tobytes() == b.downlink(x[1], 77).tobytes()


def test_rays_equal_one_member_per_ray():
    """the object as it was, one member per ray, fed the repeated rows, set_path at the same end_ts: the ray phases are 0 there"""
    t0 = (1 << 32) - 321
    counts = (1, 3, 64)
    rays = [[dict(PLAIN0, phase=0)], [dict(r, phase=0) for r in RAYS1], [dict(r, phase=0) for r in rays64()]]
    a = trxhip.AirChannel(None, 3, MAX_DELAY, SEED)
    b = trxhip.AirChannel(None, sum(counts), MAX_DELAY, SEED)
    for o in (a, b):
        o.reset(UL, t0)
        o.set_noise(UL, 0, RMS)
    k = 0
    for m in range(3):
        a.set_rays(UL, m, rays[m])
        for r in rays[m]:
            b.set_path(UL, k, r["gain"], r["delay"], r["hz"])
            k += 1
    x = rows3()
    wide = np.repeat(x, counts, axis=0)
    for lo, hi in ((0, 300), (300, N)):
        assert a.uplink(np.ascontiguousarray(x[:, lo:hi]), t0 + lo).tobytes() == b.uplink(np.ascontiguousarray(wide[:, lo:hi]), t0 + lo).tobytes()


def test_a_rotating_ray_with_a_phase_is_the_plain_path_set_earlier():
    """phase k * inc: the plain path whose oscillator was switched on k samples before t0"""
    t0, k, hz = 5000, 1234, -67.7
    inc = NM.inc_of(hz)
    a, b = (trxhip.AirChannel(None, 3, MAX_DELAY, SEED) for _ in range(2))
    b.reset(UL, t0 - k)
    b.set_path(UL, 2, 2.5, 40, hz)
    b.reset(UL, t0)
    a.reset(UL, t0)
    a.set_rays(UL, 2, [dict(gain=2.5, delay=40, hz=hz, phase=(k * inc) & NM.M32)])
    assert b.path_state(UL, 2)["ts_ref"] == t0 - k and a.rays(UL, 2)[1] == t0
    assert a.uplink(rows3(), t0).tobytes() == b.uplink(rows3(), t0).tobytes()


# ---- 4. set_rays between windows ----------------------------------------------------------------------------------------------------------

def same_rays(a, m, d, k):
    got, ts = a.rays(d, k)
    want, ts_m = m.rays(d, k)
    assert ts == ts_m and len(got) == len(want)
    for g, w in zip(got, want):
        assert (float(g["gain"]), int(g["delay"]), float(g["hz"]), int(g["phase"]), int(g["reserved"])) == \
            (w["gain"], w["delay"], w["hz"], w["phase"], 0)


def test_state_round_trip_changes_no_later_byte():
    x = rows3()
    a, m = (case1(o) for o in make())
    y = [a.uplink(np.ascontiguousarray(x[:, :333]), -300)]
    m.uplink(np.ascontiguousarray(x[:, :333]), -300)
    for k in range(3):
        same_rays(a, m, UL, k)
    got, ts = a.rays(UL, 1)
    assert ts == 0 and got["phase"][2] == NM.phase(12345, 0, NM.inc_of(-67.7), 33) and got["phase"][1] == 1 << 30
    for k in (1, 2):
        a.set_rays(UL, k, a.rays(UL, k)[0])
        assert a.rays(UL, k)[1] == 33
    y.append(a.uplink(np.ascontiguousarray(x[:, 333:]), 33))
    assert np.concatenate(y).tobytes() == ul_ref(-300).tobytes()


def test_clearing_and_set_path_under_rays():
    """set_path while rays are set changes path_state and not the output; clearing returns the plain path, its phase as if the rays
    had never been set"""
    x = rows3()
    a, m = (case1(o) for o in make())
    plain = trxhip.AirChannel(None, 3, MAX_DELAY, SEED)                # never sees a ray
    plain.set_path(UL, 0, **PLAIN0)
    plain.set_noise(UL, 0, RMS)
    cuts = ((0, 200), (200, 450), (450, N))
    for k, (lo, hi) in enumerate(cuts):
        w = np.ascontiguousarray(x[:, lo:hi])
        if k == 1:
            for o in (a, m, plain):
                o.set_path(UL, 1, gain=0.5, delay=31, hz=-1234.5)
            st = a.path_state(UL, 1)
            assert {f: st[f].item() for f in st.dtype.names} == m.path_state(UL, 1) and st["delay"] == 31 and st["ts_ref"] == 1200
            assert len(a.rays(UL, 1)[0]) == 3
        if k == 2:
            for o in (a, m):
                o.set_rays(UL, 1, None)
                o.set_rays(UL, 2, [])
            assert len(a.rays(UL, 1)[0]) == 0 and a.rays(UL, 1)[1] == 1450
        y, ref, p = a.uplink(w, 1000 + lo), m.uplink(w, 1000 + lo), plain.uplink(w, 1000 + lo)
        assert y.tobytes() == ref.tobytes(), k
        assert (y.tobytes() == p.tobytes()) == (k == 2), k


def test_set_path_under_rays_leaves_the_output():
    x = rows3()
    a, b = (case1(make()[0]) for _ in range(2))
    a.set_path(UL, 1, gain=3.0, delay=5, hz=9999.0)
    a.set_path(DL, 2, gain=3.0, delay=5, hz=9999.0)
    assert a.uplink(x, 9).tobytes() == b.uplink(x, 9).tobytes() and a.downlink(x[0], 9).tobytes() == b.downlink(x[0], 9).tobytes()
    assert a.path_state(UL, 1)["gain"] == 3.0 and b.path_state(UL, 1)["gain"] == 1.0


# ---- 5. refusals and exports ----------------------------------------------------------------------------------------------------------------

def snapshot(a):
    return [(a.path_state(d, m).tobytes(), a.rays(d, m)[0].tobytes(), a.rays(d, m)[1]) for d in (UL, DL) for m in range(3)]


def test_refusals_change_nothing():
    L = trxhip.load_library()
    x = rows3()
    a, m = (case1(o) for o in make())
    for o in (a, m):
        o.uplink(np.ascontiguousarray(x[:, :100]), 10)
        o.downlink(np.ascontiguousarray(x[0, :50]), -20)
    before = snapshot(a)

    def rays(n=1, **kw):
        r = np.zeros(n, dtype=trxhip.AIR_RAY_DTYPE)
        r["gain"] = 1.0
        for k, v in kw.items():
            r[k][n - 1] = v                                            # the last one is the bad one: the good ones in front are not kept
        return r

    def call(d, member, r, n=None):
        return L.trxhip_multipath_set(a.h, d, member, r.ctypes.data_as(C.c_void_p) if r is not None else None, len(r) if n is None else n)

    for d in (UL, DL):
        for bad in (rays(3, gain=16.0001), rays(2, gain=-0.001), rays(gain=float("nan")), rays(gain=float("inf")), rays(4, delay=MAX_DELAY + 1),
                    rays(hz=500000.1), rays(2, hz=-500000.1), rays(hz=float("nan")), rays(5, reserved=1)):
            assert call(d, 1, bad) == EINVAL and call(d, 0, bad) == EINVAL
        assert call(d, 1, np.zeros(65, dtype=trxhip.AIR_RAY_DTYPE)) == EINVAL
        assert call(d, 1, None, 1) == EINVAL
        assert call(d, 3, rays()) == EINVAL
        assert L.trxhip_multipath_set(None, d, 0, rays().ctypes.data_as(C.c_void_p), 1) == EINVAL
        assert L.trxhip_multipath_state(a.h, d, 3, None, 0, None, None) == EINVAL
        assert L.trxhip_multipath_state(a.h, d, 1, None, 1, None, None) == EINVAL
        assert L.trxhip_multipath_state(None, d, 1, None, 0, None, None) == EINVAL
    for d in (2, -1):
        assert call(d, 0, rays()) == EINVAL and L.trxhip_multipath_state(a.h, d, 0, None, 0, None, None) == EINVAL
    for member, r in ((-1, []), (3, []), (0, [dict(delay=-1)]), (0, [dict(phase=1 << 32)]), (0, [dict(phase=-1)]), (0, [dict(gain=1.0, foo=1)]),
                      (0, [dict()] * 65)):
        with pytest.raises(trxhip.TrxHipError):
            a.set_rays(UL, member, r)
    with pytest.raises(trxhip.TrxHipError):
        a.rays(UL, 3)
    assert snapshot(a) == before
    for k in range(3):
        same_rays(a, m, UL, k)
        same_rays(a, m, DL, k)
    w = np.ascontiguousarray(x[:, 100:200])
    assert a.uplink(w, 110).tobytes() == m.uplink(w, 110).tobytes()
    w = np.ascontiguousarray(x[0, 50:200])
    assert a.downlink(w, 30).tobytes() == m.downlink(w, 30).tobytes()
    # the limits themselves pass, and a short buffer gets what fits
    a.set_rays(UL, 0, [dict(gain=16.0, delay=MAX_DELAY, hz=500000.0, phase=(1 << 32) - 1), dict(gain=0.0, delay=0, hz=-500000.0)] * 32)
    two = np.zeros(2, dtype=trxhip.AIR_RAY_DTYPE)
    n, ts = C.c_uint32(0), C.c_int64(-1)
    assert L.trxhip_multipath_state(a.h, UL, 0, two.ctypes.data_as(C.c_void_p), 2, C.byref(n), C.byref(ts)) == 0
    assert n.value == 64 and ts.value == 210 and two["gain"].tolist() == [16.0, 0.0]
    assert L.trxhip_multipath_state(a.h, UL, 0, None, 0, C.byref(n), None) == 0 and n.value == 64


def test_symbols_header_and_abi():
    L = trxhip.load_library()
    hdr = open(os.path.join(ROOT, "include", "trxhip.h")).read()
    for name in ("trxhip_multipath_set", "trxhip_multipath_state"):
        assert hasattr(L, name) and name in trxhip.SYMBOLS and name + "(" in hdr, name
    assert L.trxhip_abi_version() == 5 and re.search(r"^#define\s+TRXHIP_ABI_VERSION\s+5\b", hdr, re.M)
    assert "typedef struct trxhip_multipath_ray {  /* 24 bytes */" in hdr and trxhip.AIR_RAY_DTYPE.itemsize == 24
    from test_ms_afc_cpu import struct_fields
    assert struct_fields(hdr, "trxhip_multipath_ray") == list(trxhip.AIR_RAY_DTYPE.names)
    assert trxhip.AIR_MAX_RAYS == 64 and re.search(r"^#define\s+TRXHIP_MULTIPATH_MAX_RAYS\s+64\b", hdr, re.M)
    for name in ("AIR_RAY_DTYPE", "AIR_MAX_RAYS", "air_rays"):
        assert getattr(osmo_trx_amd, name) is getattr(trxhip, name) and name in osmo_trx_amd.__all__
    # sizeof: a state call into a buffer of one ray writes 24 bytes and no more
    a = trxhip.AirChannel(None, 1)
    a.set_rays(DL, 0, [dict(gain=2.0, delay=0, hz=1.0, phase=7)])
    buf = np.full(24 + 16, 0xA5, dtype=np.uint8)
    assert L.trxhip_multipath_state(a.h, DL, 0, buf.ctypes.data_as(C.c_void_p), 1, None, None) == 0
    assert (buf[24:] == 0xA5).all() and buf[:24].view(trxhip.AIR_RAY_DTYPE)[0]["phase"] == 7


# ---- 6. air_rays() ----------------------------------------------------------------------------------------------------------------------------

def test_air_rays_profile():
    delays_us, powers_db = [0.0, 0.2, 0.5, 1.6, 2.3, 5.0], [-3.0, 0.0, -2.0, -6.0, -8.0, -10.0]
    r = trxhip.air_rays(delays_us, powers_db, doppler_hz=100.0, sinusoids=8, seed=3, gain=0.8)
    assert r.dtype == trxhip.AIR_RAY_DTYPE and r.shape == (48,) and not r["reserved"].any()
    assert abs(float((r["gain"].astype(np.float64) ** 2).sum()) / 0.64 - 1.0) < 48 * 2.0 ** -23      # float32 gains: half an ulp each, squared
    want = np.rint(np.array(delays_us) * 1e-6 * (13e6 / 12.0)).astype(int)
    assert want.tolist() == [0, 0, 1, 2, 2, 5] and r["delay"].reshape(6, 8).tolist() == [[d] * 8 for d in want]
    p = (r["gain"].astype(np.float64) ** 2).reshape(6, 8)
    assert np.allclose(p, p[:, :1]) and np.allclose(10 * np.log10(p[:, 0] / p[1, 0]), powers_db, atol=1e-5)
    assert (np.abs(r["hz"]) <= 100.0).all() and len(np.unique(r["hz"])) == 48 and len(np.unique(r["phase"])) == 48
    c = r["hz"].reshape(6, 8) / 100.0                                  # evenly spread angles behind an offset per tap
    ang = np.arccos(np.clip(c[:, 0], -1, 1))
    assert np.allclose(c, np.cos(ang[:, None] + 2 * np.pi * np.arange(8)[None, :] / 8), atol=1e-9)
    again = trxhip.air_rays(delays_us, powers_db, doppler_hz=100.0, sinusoids=8, seed=3, gain=0.8)
    other = trxhip.air_rays(delays_us, powers_db, doppler_hz=100.0, sinusoids=8, seed=4, gain=0.8)
    assert again.tobytes() == r.tobytes() and other.tobytes() != r.tobytes()
    one = trxhip.air_rays([0.0], [0.0])
    assert one.shape == (1,) and one["gain"][0] == 1.0 and one["hz"][0] == 0.0
    for bad in (dict(delays_us=[0.0, 1.0], powers_db=[0.0]), dict(delays_us=[-1.0], powers_db=[0.0]), dict(delays_us=[0.0] * 9, powers_db=[0.0] * 9, sinusoids=8),
                dict(delays_us=[0.0], powers_db=[0.0], sinusoids=0)):
        with pytest.raises(ValueError):
            trxhip.air_rays(**bad)


def test_a_jakes_set_fades_at_the_set_power():
    """16 rays of one tap on a constant carrier of amplitude 8192 over n = 200 000 samples, Doppler fd = 20 kHz.  The envelope of a
    Rayleigh process decorrelates within about 1 / fd, so the stretch holds about K = fd * n / fs = 3692 independent fades; the
    power of one fade is exponentially distributed (standard deviation = mean), so the mean power of the stretch has a relative
    standard deviation of 1 / sqrt(K) = 0.0165 and the bar is five of them, 0.082.  (A sum of 16 sinusoids is smoother than that:
    its cross terms average out as 1 / (pi df n / fs) per pair; the bar does not rely on it.)"""
    n, fd, amp = 200000, 20000.0, 8192
    r = trxhip.air_rays([0.0], [0.0], doppler_hz=fd, sinusoids=16, seed=11)
    a = trxhip.AirChannel(None, 1)
    a.set_rays(UL, 0, r)
    x = np.zeros((1, n, 2), np.int16)
    x[0, :, 0] = amp
    y = a.uplink(x, 0).astype(np.float64)
    p = (y ** 2).sum(axis=1)
    want = float((r["gain"].astype(np.float64) ** 2).sum()) * amp * amp
    K = fd * n / (13e6 / 12.0)
    bar = 5.0 / np.sqrt(K)
    print(f"mean power / set power - 1 = {p.mean() / want - 1.0:+.5f} (bar {bar:.4f}, K = {K:.0f} fades); envelope / rms: min "
          f"{np.sqrt(p.min() / p.mean()):.3f} max {np.sqrt(p.max() / p.mean()):.3f}")
    assert abs(p.mean() / want - 1.0) <= bar
    env = np.sqrt(p / p.mean())
    assert env.min() < 1.0 < env.max()                                 # it fades: below its rms and above it


# ---- the dispersive channel of the loops, chosen on the oracle ----------------------------------------------------------------------------

def test_the_echo_of_the_loops_is_the_largest_the_oracle_equalises():
    """tests/air_rays_loop.py: of the ladder 0.7, 0.5, 0.35, 0.25 the loops use the largest g2 at which the oracle's Viterbi chain
    finds the 18 bursts of the uplink loop behind {1, d} + {g2, d + 8 samples, a quarter turn} and has no wrong hard bit 3 .. 144"""
    import air_rays_loop as RL
    clean = []
    for g2 in RL.LADDER:
        res = RL.oracle_uplink(g2)
        print(f"g2 {g2}: use_va found {int(res[True][0].sum())} / 18, wrong bits {int(res[True][1].sum())}; plain found "
              f"{int(res[False][0].sum())} / 18, wrong bits {int(res[False][1].sum())}")
        if res[True][0].all() and not res[True][1].any():
            clean.append(g2)
    assert max(clean) == RL.G2
