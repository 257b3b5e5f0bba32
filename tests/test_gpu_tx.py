"""The transmit side on the MI355X: trxhip_modulate_batch / trxhip_modulate_trxd_batch against the oracle's restatement of
the reference's modulators (generic C, sigProcLib.cpp:558-979) with np.array_equal on float32, the int16 and TRXD paths,
a modulate -> detect / demodulate round trip through the project's own receiver, and the sigProcLib Tx calls of the
stand-alone shim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from osmo_trx_amd import synth, trxhip
from osmo_trx_amd.trxhip import TX_8PSK, TX_EMPTY_PULSE, tx_params_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "osmo_trx_amd", "host")
LIBDIR = os.path.join(ROOT, "osmo_trx_amd", "lib")
EINVAL, ENOTSUP = -22, -95


@pytest.fixture(scope="module")
def trx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    O.lib().orc_setup()
    t = trxhip.TrxHip(0)
    yield t
    t.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def f32(x):
    return np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)


def orc_gmsk(bits, guard, sps, empty=False):
    return O.modulate_burst(bits, guard, sps, empty)


def orc_edge(bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    out = np.zeros(640, dtype=np.complex64)
    assert O.lib().orc_modulate_edge_burst(bits.ctypes.data, len(bits), out.ctypes.data) == 625
    return out[:625].copy()


def edge_rotate(bits, sps):
    """rotateEdgeBurst(mapEdgeSymbols(bits), sps), sigProcLib.cpp:672-729, in float32 with the transmit tables' map and phasors
    (pinned against the oracle by tests/test_tx_cpu.py)"""
    from test_tx_cpu import TX_TABLES
    t = np.frombuffer(trxhip.generate_tx_tables_host(), dtype=TX_TABLES)[0]
    b = np.asarray(bits) & 1
    n = len(b) // 3
    idx = b[0::3] | (b[1::3] << 1) | (b[2::3] << 2)
    s, r = t["psk8"][idx], t["edge_rot"][:n]
    re = s.real * r.real - s.imag * r.imag
    im = s.real * r.imag + s.imag * r.real
    out = np.zeros(n * sps, dtype=np.complex64)
    out.real[::sps], out.imag[::sps] = re, im
    return out


def run(trx, bits, params, sps, **kw):
    out, s16, lens = trx.modulate(dev(bits), trx.tx_params_tensor(params), sps=sps, **kw)
    import torch
    torch.cuda.synchronize()
    return (out.cpu().numpy() if out is not None else None), (s16.cpu().numpy() if s16 is not None else None), lens.cpu().numpy()


def test_gmsk_4sps_random_bytes_and_scales(trx):
    import torch
    rng = np.random.default_rng(11)
    n = 4096
    bits = rng.integers(0, 256, (n, 148), dtype=np.uint8)      # only bit 0 counts
    tn = np.arange(n) % 8
    out, _, lens = run(trx, bits, tx_params_host(148, 8 + (tn % 4 == 0)), 4)
    assert (lens == 625).all()
    ref = np.stack([orc_gmsk(bits[i], 8 + (tn[i] % 4 == 0), 4) for i in range(n)])
    assert np.array_equal(f32(out), f32(ref))
    # the fused scale equals scaleVector over the unscaled row
    sc = (rng.uniform(-3000, 3000, n) + 1j * rng.uniform(-3000, 3000, n)).astype(np.complex64)
    out_s, _, _ = run(trx, bits, tx_params_host(148, 8, 0, sc), 4)
    want = torch.from_numpy(out.copy()).to("cuda:0")
    for i in range(n):
        trx.scale_vector(want[i], complex(sc[i]))
    torch.cuda.synchronize()
    assert np.array_equal(f32(out_s), f32(want.cpu().numpy()))


def test_gmsk_1sps_normal_and_access(trx):
    rng = np.random.default_rng(12)
    rows, params, refs = [], [], []
    for tn in range(8):
        for _ in range(16):
            b = rng.integers(0, 2, 148, dtype=np.uint8)
            g = 8 + (tn % 4 == 0)
            rows.append(np.pad(b, (0, 160 - 148)))
            params.append((148, g))
            refs.append(orc_gmsk(b, g, 1))
        for delay in (0, 20, 67):
            b = rng.integers(0, 2, 88 + delay, dtype=np.uint8)
            g = 68 - delay + (tn % 4 == 0)
            rows.append(np.pad(b, (0, 160 - len(b))))
            params.append((88 + delay, g))
            refs.append(orc_gmsk(b, g, 1))
    p = tx_params_host([q[0] for q in params], [q[1] for q in params])
    out, _, lens = run(trx, np.stack(rows), p, 1, out_stride=157)
    for i, r in enumerate(refs):
        assert lens[i] == len(r)
        assert np.array_equal(f32(out[i, :len(r)]), f32(r)), i
        assert not out[i, len(r):].any()


def test_empty_pulse_and_out_of_range_descriptors(trx):
    rng = np.random.default_rng(13)
    for sps, lim in ((4, 625), (1, 157)):
        rows, prm, refs = [], [], []
        for k in range(64):
            nb = int(rng.integers(1, 148))
            g = int(rng.integers(0, lim // sps - nb + 1))
            b = rng.integers(0, 2, nb, dtype=np.uint8)
            rows.append(np.pad(b, (0, 160 - nb)))
            prm.append((nb, g, TX_EMPTY_PULSE))
            refs.append(orc_gmsk(b, g, sps, empty=True))
        # refused: the empty pulse past the rotation table (4 SPS: 148 + 9 symbols read GMSKRotation4[625..627]); at 4 SPS a
        # Laurent burst of 156 bits (writes past the reference's 625 samples) and of 1 bit
        bad = [(148, 9 if sps == 4 else 10, TX_EMPTY_PULSE)] + ([(156, 8, 0), (1, 8, 0)] if sps == 4 else [(150, 8, 0)])
        for j, q in enumerate(bad):
            rows.insert(10 * j + 5, np.ones(160, dtype=np.uint8))
            prm.insert(10 * j + 5, q)
            refs.insert(10 * j + 5, None)
        p = tx_params_host([q[0] for q in prm], [q[1] for q in prm], [q[2] for q in prm])
        out, _, lens = run(trx, np.stack(rows), p, sps, out_stride=lim)
        for i, r in enumerate(refs):
            if r is None:
                assert lens[i] == EINVAL and not out[i].any(), (sps, i)
            else:
                assert lens[i] == len(r)
                assert np.array_equal(f32(out[i, :len(r)]), f32(r)), (sps, i)
                assert not out[i, len(r):].any()


def test_8psk_shaped_and_empty_pulse(trx):
    rng = np.random.default_rng(14)
    n = 512
    bits = rng.integers(0, 256, (n, 444), dtype=np.uint8)
    out, _, lens = run(trx, bits, tx_params_host(444, 0, TX_8PSK, n=n), 4)
    assert (lens == 625).all()
    assert np.array_equal(f32(out), f32(np.stack([orc_edge(b) for b in bits])))
    for sps in (4, 1):
        out, _, lens = run(trx, bits, tx_params_host(444, 0, TX_8PSK | TX_EMPTY_PULSE, n=n), sps, out_stride=148 * sps)
        assert (lens == 148 * sps).all()
        assert np.array_equal(f32(out), f32(np.stack([edge_rotate(b, sps) for b in bits])))
    # shaped 8-PSK at 1 SPS and a bit count that is not a multiple of 3: refused
    _, _, lens = run(trx, bits[:2], tx_params_host([444, 443], 0, TX_8PSK), 1)
    assert (lens == EINVAL).all()


def test_int16_frame(trx):
    import torch
    rng = np.random.default_rng(15)
    bits = rng.integers(0, 2, (8, 148), dtype=np.uint8)
    tn = np.arange(8)
    p = tx_params_host(148, 8 + (tn % 4 == 0), 0, rng.uniform(0.5, 1.5, 8).astype(np.complex64))
    out, s16, lens = trx.modulate(dev(bits), trx.tx_params_tensor(p), sps=4, s16_scale=20000.0)
    conv = torch.empty(8 * 625 * 2, dtype=torch.int16, device="cuda:0")
    rc = trx.L.trxhip_convert_float_short(trx.h, C.c_void_p(conv.data_ptr()), C.c_void_p(out.data_ptr()), C.c_float(20000.0),
                                          8 * 625 * 2, trx._stream())
    assert rc == 0
    torch.cuda.synchronize()
    frame = s16.cpu().numpy().reshape(-1)              # one TDMA frame: 8 x 625 samples, TN order
    assert frame.size == 5000 * 2
    assert np.array_equal(frame, conv.cpu().numpy())
    assert np.abs(frame).max() > 10000
    # int16 only (no cf32 row)
    _, s16b, _ = trx.modulate(dev(bits), trx.tx_params_tensor(p), sps=4, cf32=False, s16_scale=20000.0)
    torch.cuda.synchronize()
    assert np.array_equal(s16b.cpu().numpy().reshape(-1), frame)


def _dgram(version, tn, fn, att, bits):
    return np.concatenate([np.array([(version << 4) | tn, (fn >> 24) & 255, (fn >> 16) & 255, (fn >> 8) & 255, fn & 255, att],
                                    dtype=np.uint8), bits])


def test_trxd_downlink(trx):
    rng = np.random.default_rng(16)
    dg, dlen, want = [], [], []
    for att in range(256):
        for version in (0, 1):
            for nb in (148, 444):
                tn, fn = int(rng.integers(0, 8)), int(rng.integers(0, 2715648))
                b = rng.integers(0, 2, nb, dtype=np.uint8)
                dg.append(np.pad(_dgram(version, tn, fn, att, b), (0, 450 - 6 - nb)))
                dlen.append(6 + nb)
                want.append((fn, tn, version, att, nb, b))
    # refused: version 2, a bad length
    b = rng.integers(0, 2, 148, dtype=np.uint8)
    dg += [np.pad(_dgram(2, 1, 5, 0, b), (0, 296)), np.pad(_dgram(0, 1, 5, 0, b), (0, 296))]
    dlen += [154, 155]
    want += [None, None]
    D, Lg = dev(np.stack(dg)), dev(np.array(dlen, dtype=np.int32))
    import torch
    for fs in (32767.0, 2047.0):
        out, _, info = trx.modulate_trxd(D, Lg, fs, sps=4)
        torch.cuda.synchronize()
        out, info = out.cpu().numpy(), trx.tx_info_to_numpy(info)
        for i, w in enumerate(want):
            if w is None:
                assert info["status"][i] == EINVAL and not out[i].any()
                continue
            fn, tn, version, att, nb, bits = w
            assert (info["fn"][i], info["tn"][i], info["version"][i], info["tx_att"][i]) == (fn, tn, version, att)
            assert info["status"][i] == 0 and info["nbits"][i] == nb and info["length"][i] == 625
            a = orc_gmsk(bits, 8 + (tn % 4 == 0), 4) if nb == 148 else orc_edge(bits)
            s = np.float32(fs * 10.0 ** (-att / 20.0))           # (float)(txFullScale * pow(10, -att / 20.0))
            re = a.real * s - a.imag * np.float32(0.0)
            im = a.real * np.float32(0.0) + a.imag * s
            assert np.array_equal(out[i].real, re) and np.array_equal(out[i].imag, im), i
    # 1 SPS: GMSK through modulateBurstBasic, 8-PSK refused
    sel = [0, 1, 2, 3]
    out, _, info = trx.modulate_trxd(D[sel].contiguous(), Lg[sel].contiguous(), 32767.0, sps=1, out_stride=157)
    torch.cuda.synchronize()
    out, info = out.cpu().numpy(), trx.tx_info_to_numpy(info)
    for k, i in enumerate(sel):
        fn, tn, version, att, nb, bits = want[i]
        if nb == 444:
            assert info["status"][k] == ENOTSUP and not out[k].any()
        else:
            g = 8 + (tn % 4 == 0)
            a = orc_gmsk(bits, g, 1)
            assert info["length"][k] == 148 + g
            assert np.array_equal(out[k, :148 + g].real, a.real * np.float32(32767.0) - a.imag * np.float32(0.0))


def test_round_trip_through_the_receiver(trx):
    import torch
    gen = torch.Generator().manual_seed(17)
    n = 4096
    tsc = torch.arange(n) % 8
    bits = synth.normal_burst_bits(n, tsc, gen, "cpu").numpy()
    _, s16, lens = trx.modulate(dev(bits), trx.tx_params_tensor(tx_params_host(148, 8, n=n)), sps=4, cf32=False, s16_scale=10000.0)
    params = np.zeros(n, dtype=trxhip.PARAMS_DTYPE)
    params["type"], params["tsc"], params["max_toa"] = trxhip.TSC, tsc.numpy(), 8
    res, soft = trx.detect_demod(s16, trx.params_tensor(params), sps=4, exact=True)
    torch.cuda.synchronize()
    r = trx.results_to_numpy(res)
    assert (r["rc"] == trxhip.TSC).all()
    assert (np.abs(r["toa"] - synth.BASE_TOA[4]) < 0.5).all()
    assert np.array_equal(soft.cpu().numpy()[:, :148] > 0.5, bits.astype(bool))

    ebits = synth.edge_burst_bits(n, tsc, gen, "cpu").numpy()
    _, s16, _ = trx.modulate(dev(ebits), trx.tx_params_tensor(tx_params_host(444, 0, TX_8PSK, n=n)), sps=4, cf32=False,
                             s16_scale=10000.0)
    params["type"] = trxhip.EDGE
    res, soft = trx.detect_demod(s16, trx.params_tensor(params), sps=4, soft_stride=444, exact=True)
    torch.cuda.synchronize()
    r = trx.results_to_numpy(res)
    assert (r["rc"] == trxhip.EDGE).all()
    assert (np.abs(r["toa"] - synth.BASE_TOA[4]) < 0.5).all()
    # hard decisions of the data and training symbols (the first tail symbol sits half outside the reference receiver's 5-tap
    # equaliser, which the oracle reproduces; tail bits carry no information)
    hard = soft.cpu().numpy()[:, :444] > 0.5
    assert np.array_equal(hard[:, 9:435], ebits[:, 9:435].astype(bool))


SHIM_CALLER = r'''
#include <cstdio>
#include <cstdlib>
#include "sigProcLib.h"
static void dump(FILE *f, signalVector *v)
{
	int n = v ? (int)v->size() : -1;
	fwrite(&n, 4, 1, f);
	if (v) fwrite(v->begin(), 8, n, f);
	delete v;
}
int main(int argc, char **argv)
{
	if (argc != 3 || !sigProcLibSetup()) return 2;
	unsigned char buf[148 + 444];
	FILE *in = fopen(argv[1], "rb");
	if (!in || fread(buf, 1, sizeof(buf), in) != sizeof(buf)) return 3;
	fclose(in);
	BitVector g(148), e(444);
	for (int i = 0; i < 148; i++) g[i] = buf[i];
	for (int i = 0; i < 444; i++) e[i] = buf[148 + i];
	FILE *o = fopen(argv[2], "wb");
	dump(o, modulateBurst(g, 8, 4));
	dump(o, modulateBurst(g, 9, 1));
	dump(o, modulateEdgeBurst(e, 4));
	for (int tn = 0; tn < 8; tn++) dump(o, generateDummyBurst(4, tn));
	srand(7);
	dump(o, genRandNormalBurst(3, 4, 0));
	dump(o, genRandAccessBurst(20, 4, 1));
	dump(o, generateEdgeBurst(5));
	dump(o, genRandAccessBurst(68, 4, 2));
	dump(o, generateEmptyBurst(1, 0));
	fclose(o);
	sigProcLibDestroy();
	return 0;
}
'''


def test_standalone_shim_tx_calls(trx, tmp_path):
    import torch
    from test_tx_cpu import TX_TABLES
    src = tmp_path / "tx_caller.cpp"
    src.write_text(SHIM_CALLER)
    exe = str(tmp_path / "tx_caller")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(HOST, "compat"),
                           "-I", HOST, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", LIBDIR, "-ltrxsigproc_sa",
                           "-ltrxhip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    rng = np.random.default_rng(18)
    g = rng.integers(0, 256, 148, dtype=np.uint8)
    e = rng.integers(0, 256, 444, dtype=np.uint8)
    (tmp_path / "in.bin").write_bytes(g.tobytes() + e.tobytes())
    torch.cuda.synchronize()
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=120)
    assert r.returncode == 0
    raw = (tmp_path / "out.bin").read_bytes()
    vecs, off = [], 0
    while off < len(raw):
        n = int(np.frombuffer(raw, np.int32, 1, off)[0])
        off += 4
        vecs.append(None if n < 0 else np.frombuffer(raw, np.complex64, n, off).copy())
        off += max(n, 0) * 8
    t = np.frombuffer(trxhip.generate_tx_tables_host(), dtype=TX_TABLES)[0]
    want = [orc_gmsk(g, 8, 4), orc_gmsk(g, 9, 1), orc_edge(e)] + [orc_gmsk(t["dummy_burst"], 8 + (tn % 4 == 0), 4) for tn in range(8)]
    # the same rand() draws, in the reference's order and count (sigProcLib.cpp:768-915)
    libc = C.CDLL(None)
    libc.srand(7)
    nb = np.zeros(148, dtype=np.uint8)
    nb[3:60] = [libc.rand() % 2 for _ in range(57)]
    nb[61:87] = t["tsc"][3]
    nb[88:145] = [libc.rand() % 2 for _ in range(57)]
    want.append(orc_gmsk(nb, 9, 4))
    ab = np.zeros(108, dtype=np.uint8)
    ab[20:69] = t["rach_burst"]
    ab[69:105] = [libc.rand() % 2 for _ in range(36)]
    want.append(orc_gmsk(ab, 68 - 20, 4))
    sym = np.full(148, 7)
    sym[3:61] = [libc.rand() % 8 for _ in range(58)]
    et = t["edge_tsc"][5]
    sym[61:87] = et[0::3] | (et[1::3] << 1) | (et[2::3] << 2)
    sym[87:145] = [libc.rand() % 8 for _ in range(58)]
    eb = np.stack([sym & 1, (sym >> 1) & 1, (sym >> 2) & 1], axis=1).reshape(-1).astype(np.uint8)
    want.append(orc_edge(eb))
    assert len(vecs) == len(want) + 2
    for i, w in enumerate(want):
        assert vecs[i] is not None and np.array_equal(f32(vecs[i]), f32(w)), i
    assert vecs[-2] is None                               # genRandAccessBurst(68, 4, tn): 156 bits overrun the reference
    assert vecs[-1] is not None and len(vecs[-1]) == 157 and not vecs[-1].any()
