"""The multi-ARFCN transmit front end on the MI355X: trxhip_synthesize_batch and trxhip_tx_frontend_* (RadioInterfaceMulti::
pushBuffer / RadioInterfaceResamp::pushBuffer), bit for bit against the reference-compiled Resampler and convert_float_short,
the oracle's resampler and the numpy restatement of Synthesis::rotate (tests/tx_frontend_model.py); streaming, seeding, the
device loopback through the receive front end, and the C++ MultiArfcnTx class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import tx_frontend_model as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, ENOTSUP = -22, -95
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "osmo_trx_amd", "lib", "sigproc_selftest")


@pytest.fixture(scope="module")
def trx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def streams(chans, n, seed, amp=2000.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((chans, n, 2)) * amp).astype(np.float32).view(np.complex64)[..., 0]


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fe(trx, **kw):
    from osmo_trx_amd.trxhip import TxFrontEnd
    return TxFrontEnd(trx, **kw)


@pytest.mark.parametrize("p,q,bw,bl", [(48, 65, 1.0, 260), (96, 65, 0.45, 260), (75, 52, 0.45, 208)])
def test_tx_resampler_against_compiled_reference(trx, p, q, bw, bl):
    """RESAMP mode, cf32: Resampler(p, q, 16)::rotate fed block by block with the RadioBuffer's 16 samples of history in front
    (radioBuffer.cpp:29-47), the reference's own Resampler (oracle/_ref/libref_generic.so) and the oracle's restatement."""
    n_blocks = 40
    x = streams(1, n_blocks * bl, seed=p + q)[0]
    f = fe(trx, chans=1, block_len=bl, p=p, q=q, bw=bw, mode="resamp")
    out, _ = f.push(dev(x), n_blocks)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert bits_of(got).tobytes() == bits_of(M.resample(x, p, q, bw)).tobytes()
    if not O.ref_arch_available("generic"):
        return
    R = C.CDLL(os.path.join(O.REF_DIR, "libref_generic.so"))
    R.convolve_init()                                               # the arch function table Resampler::rotate calls through
    R.ref_resampler_new.restype = C.c_void_p
    R.ref_resampler_new.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_float]
    R.ref_resampler_rotate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    R.ref_resampler_free.argtypes = [C.c_void_p]
    h = R.ref_resampler_new(p, q, 16, bw)
    assert h
    nb_out = bl // q * p
    ref = np.zeros(n_blocks * nb_out, dtype=np.complex64)
    buf = np.zeros(16 + bl, dtype=np.complex64)
    for b in range(n_blocks):
        buf[16:] = x[b * bl:(b + 1) * bl]
        o = np.zeros(nb_out, dtype=np.complex64)
        assert R.ref_resampler_rotate(h, buf[16:].ctypes.data, bl, o.ctypes.data, nb_out) >= 0
        ref[b * nb_out:(b + 1) * nb_out] = o
        buf[:16] = buf[-16:]
    R.ref_resampler_free(h)
    assert bits_of(got).tobytes() == bits_of(ref).tobytes()


def test_synthesize_batch_against_model(trx):
    """trxhip_synthesize_batch over 48 blocks (history carried across blocks, zero before block 0), rows with padding"""
    n_blocks, bl = 48, 192
    rows = np.zeros((4, n_blocks * bl + 40), dtype=np.complex64)
    rows[:, :n_blocks * bl] = streams(4, n_blocks * bl, seed=3)
    rows[:, n_blocks * bl:] = 1e9                                   # behind the stream: must not be read
    out = trx.synthesize(dev(rows), n_blocks, block_len=bl)
    torch.cuda.synchronize()
    want = M.synthesis(np.ascontiguousarray(rows[:, :n_blocks * bl]))
    assert bits_of(out.cpu().numpy()).tobytes() == bits_of(want).tobytes()


@pytest.mark.parametrize("chans", [1, 2, 3])
def test_multi_chain_against_model(trx, chans):
    """MULTI, cf32 and int16 at 1 / chans: the resampler per active path, zero rows elsewhere, Synthesis, convert_float_short"""
    n_blocks = 50
    x = streams(chans, n_blocks * 260, seed=10 + chans)
    scale = np.float32(1.0 / chans)
    f = fe(trx, chans=chans)
    out, s16 = f.push(dev(x), n_blocks, cf32=True, s16_scale=float(scale))
    torch.cuda.synchronize()
    want = M.multi_chain(x, chans)
    got = out.cpu().numpy()
    assert got.shape == (n_blocks * 768,)
    assert bits_of(got).tobytes() == bits_of(want).tobytes()
    assert np.array_equal(s16.cpu().numpy(), M.to_s16(want, scale))
    if O.ref_arch_available("generic"):
        assert np.array_equal(s16.cpu().numpy(), M.ref_convert_float_short(want, scale))


def test_multi_geometry_outside_the_fused_tiles(trx):
    """Resampler(127, 400): no tile of the fused kernel fits, the front end runs resample_kernel + synthesis_kernel"""
    n_blocks, bl, p, q = 12, 400, 127, 400
    x = streams(3, n_blocks * bl, seed=21)
    f = fe(trx, chans=3, block_len=bl, p=p, q=q)
    out, s16 = f.push(dev(x), n_blocks, s16_scale=0.5)
    torch.cuda.synchronize()
    want = M.multi_chain(x, 3, p, q)
    assert bits_of(out.cpu().numpy()).tobytes() == bits_of(want).tobytes()
    assert np.array_equal(s16.cpu().numpy(), M.to_s16(want, 0.5))


def test_fused_equals_unfused_at_full_size(trx):
    """262 144 blocks, 3 chans: the fused kernel against the composition of the separate calls (RESAMP-mode resampler per
    logical channel into the path rows, trxhip_synthesize_batch, int16 by torch); then random 64-block windows against the
    model (every filter is FIR with less than a block of memory: one block in front of a window settles it)."""
    n_blocks, chans = 1 << 18, 3
    scale = np.float32(1.0 / 3)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    x = torch.view_as_complex((torch.randn((chans, n_blocks * 260, 2), generator=g, device="cuda:0") * 2000.0).contiguous())
    out, s16 = fe(trx, chans=chans).push(x, n_blocks, s16_scale=float(scale))
    rows = torch.zeros((4, n_blocks * 192), dtype=torch.complex64, device="cuda:0")
    for pchan, lchan in M.ACTIVE[chans].items():
        r = fe(trx, chans=1, mode="resamp")
        rows[pchan], _ = r.push(x[lchan].contiguous(), n_blocks)
        r.close()
    ref = trx.synthesize(rows, n_blocks)
    del rows
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    ref_s16 = (torch.view_as_real(ref) * float(scale)).trunc().to(torch.int32).to(torch.int16)
    assert torch.equal(s16, ref_s16)
    del ref, ref_s16
    rng = np.random.default_rng(9)
    for b in [1, n_blocks - 64] + [int(v) for v in rng.integers(1, n_blocks - 64, 3)]:
        xs = x[:, (b - 1) * 260:(b + 64) * 260].cpu().numpy()
        want = M.multi_chain(xs, chans)[768:]
        got = out[b * 768:(b + 64) * 768].cpu().numpy()
        assert bits_of(got).tobytes() == bits_of(want).tobytes(), b
        assert np.array_equal(s16[b * 768:(b + 64) * 768].cpu().numpy(), M.to_s16(want, scale))


@pytest.mark.parametrize("kw", [dict(chans=3), dict(chans=2), dict(chans=1, p=96, q=65, bw=0.45, mode="resamp"),
                                dict(chans=3, block_len=400, p=127, q=400)])
def test_streaming_any_chunking_and_seeded_shards(trx, kw):
    """Any chunking of a stream equals the one-piece result (cf32 and int16); a shard started with trxhip_tx_frontend_seed()
    from the one block before it equals the same blocks of the unsharded run; without the seed it differs at its start."""
    chunks = (1, 7, 2, 19, 1, 30)
    n_blocks = sum(chunks)
    f1 = fe(trx, **kw)
    bl, chans = f1.block_len, f1.chans
    x = dev(streams(chans, n_blocks * bl, seed=33))
    full, full16 = f1.push(x, n_blocks, s16_scale=0.25)
    f2 = fe(trx, **kw)
    parts, parts16, pos = [], [], 0
    for nb in chunks:
        o, o16 = f2.push(x[:, pos * bl:(pos + nb) * bl].contiguous(), nb, s16_scale=0.25)
        parts.append(o)
        parts16.append(o16)
        pos += nb
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(parts).view(torch.int32), full.view(torch.int32))
    assert torch.equal(torch.cat(parts16), full16)
    per = f1.out_len(1)
    cut = 25
    shard = fe(trx, **kw)
    shard.seed(x[:, (cut - 1) * bl:cut * bl].contiguous(), 1)
    o, _ = shard.push(x[:, cut * bl:].contiguous(), n_blocks - cut)
    cold = fe(trx, **kw)
    oc, _ = cold.push(x[:, cut * bl:].contiguous(), n_blocks - cut)
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int32), full[cut * per:].view(torch.int32))
    assert not torch.equal(oc[:per].view(torch.int32), full[cut * per:(cut + 1) * per].view(torch.int32))
    shard.seed(None, 0)                                             # seed with nothing = reset: the cold result again
    o0, _ = shard.push(x[:, cut * bl:].contiguous(), n_blocks - cut)
    torch.cuda.synchronize()
    assert torch.equal(o0.view(torch.int32), oc.view(torch.int32))


def _dgram(tn, fn, bits):
    return np.concatenate([np.array([tn, (fn >> 24) & 255, (fn >> 16) & 255, (fn >> 8) & 255, fn & 255, 0], dtype=np.uint8), bits])


def _unambiguous_bursts(tsc, rng):
    """normal bursts whose data bits nowhere repeat the 16 midamble bits the detector correlates with (TSC bits 5..20, or their
    complement) inside its search window: such a burst has two equal correlation peaks, whatever carried it"""
    from osmo_trx_amd import synth
    out = np.zeros((len(tsc), 148), dtype=np.uint8)
    for i, t in enumerate(tsc):
        tb = np.array([int(c) for c in synth.TSC_BITS[t]], dtype=np.uint8)
        core = tb[5:21]
        while True:
            b = rng.integers(0, 2, 148).astype(np.uint8)
            b[:3] = b[145:] = 0
            b[61:87] = tb
            if not any((b[j:j + 16] == core).all() or (b[j:j + 16] != core).all() for j in range(40, 133) if j != 66):
                break
        out[i] = b
    return out


def test_device_loopback_modulator_synthesis_channelizer_detector(trx):
    """bits -> modulate_trxd (3 logical channels) -> TxFrontEnd(chans=3) int16 -> RxFrontEnd(192, 65, 48) -> detect_demod:
    one Tx block (768 wideband samples) is one Rx block, 416 timeslots are 1000 blocks.  Logical channel k arrives on
    logical channel k (both sides use getLogicalChan).  Logical channel l carries TSC (slot + 3 l) % 8; the path no carrier
    uses, searched for a TSC no carrier sends in that slot, yields false alarms only."""
    from osmo_trx_amd import trxhip
    n_slots, chans = 52 * 8, 3
    rng = np.random.default_rng(41)
    slot = np.arange(n_slots)
    tsc = [(slot + 3 * l) % 8 for l in range(chans)]
    bits = [_unambiguous_bursts(tsc[l], rng) for l in range(chans)]
    full_scale = 6000.0
    x = torch.empty((chans, n_slots * 625), dtype=torch.complex64, device="cuda:0")
    for l in range(chans):
        D = np.stack([_dgram(i % 8, i // 8, bits[l][i]) for i in range(n_slots)])
        out, _, info = trx.modulate_trxd(dev(D), dev(np.full(n_slots, 154, dtype=np.int32)), full_scale, sps=4)
        assert (trx.tx_info_to_numpy(info)["status"] == 0).all()
        x[l] = out.reshape(-1)
    n_blocks = n_slots * 625 // 260
    assert n_blocks == 1000
    _, wide = fe(trx, chans=chans).push(x, n_blocks, cf32=False, s16_scale=float(np.float32(1.0 / chans)))
    torch.cuda.synchronize()
    peak = int(wide.abs().max())
    assert 1000 < peak < 32767, peak                                   # no int16 sample at the rails
    noise = torch.from_numpy(np.round(rng.standard_normal(tuple(wide.shape)) * 20.0).astype(np.int16)).to("cuda:0")
    wide = (wide.to(torch.int32) + noise).clamp(-32768, 32767).to(torch.int16)   # a receiver's noise floor
    rx = trxhip.RxFrontEnd(trx, 192, 65, 48)
    rs = rx.pull(wide, n_blocks)
    assert rs.shape == (4, n_slots * 625)
    body = slice(1, n_slots - 1)
    toas = []
    for pchan in range(4):
        lchan = {0: 1, 1: 0, 3: 2}.get(pchan)                          # MultiArfcnRx::getLogicalChan(pchan, 3)
        params = np.zeros(n_slots, dtype=O.PARAMS_DTYPE)
        params["type"], params["max_toa"] = O.TSC, 20
        params["tsc"] = tsc[lchan] if lchan is not None else (slot + 1) % 8
        res, soft = trx.detect_demod(rs[pchan].view(n_slots, 625), trx.params_tensor(params), sps=4, full_scale=32767.0,
                                     exact=True)
        r = trx.results_to_numpy(res)
        if lchan is None:
            assert (r["rc"] > 0).mean() < 0.03, pchan
            continue
        assert (r["rc"][body] == O.TSC).all(), (pchan, np.flatnonzero(r["rc"][body] != O.TSC)[:10])
        assert r["toa"][body].std() < 0.05, pchan
        toas.append(r["toa"][body].mean())
        hard = (soft.cpu().numpy()[body] > 0.5).astype(np.uint8)
        ber = (hard[:, 3:145] != bits[lchan][body][:, 3:145]).mean()
        assert ber < 1e-3, (pchan, lchan, ber)
    assert max(toas) - min(toas) < 0.05


def test_multi_arfcn_tx_class(trx, tmp_path):
    """The C++ MultiArfcnTx (host/MultiArfcnTx.cpp) driven in chunks of 1, 2, 3, ... blocks equals TxFrontEnd's int16 output"""
    from osmo_trx_amd import build as trx_build
    trx_build.build_all()
    n_blocks, chans = 45, 3
    x = streams(chans, n_blocks * 260, seed=77)
    (tmp_path / "x.cf32").write_bytes(x.tobytes())
    subprocess.check_call([EXE, "multi_tx", str(tmp_path / "x.cf32"), str(n_blocks), str(chans), str(tmp_path / "w.s16")])
    got = np.fromfile(tmp_path / "w.s16", dtype=np.int16).reshape(-1, 2)
    _, s16 = fe(trx, chans=chans).push(dev(x), n_blocks, cf32=False, s16_scale=float(np.float32(1.0 / chans)))
    torch.cuda.synchronize()
    assert np.array_equal(got, s16.cpu().numpy())


def test_refusals(trx):
    L, h = trx.L, trx.h
    out = C.c_void_p()
    for args in [(2, 1, 260, 48, 65, 1.0), (-1, 1, 260, 48, 65, 1.0),             # bad mode
                 (0, 0, 260, 48, 65, 1.0), (0, 4, 260, 48, 65, 1.0), (1, 2, 260, 96, 65, 0.45),   # bad chans
                 (0, 3, 259, 48, 65, 1.0), (1, 1, 208, 96, 65, 0.45),               # block_len % q
                 (0, 3, 260, 129, 65, 1.0), (0, 3, 260, 0, 65, 1.0), (0, 3, 260, 48, 0, 1.0),   # p, q
                 (0, 3, 260, 48, 65, 0.0), (0, 3, 260, 48, 65, -1.0)]:              # bw
        assert L.trxhip_tx_frontend_create(h, *args, C.byref(out)) == EINVAL, args
    assert L.trxhip_tx_frontend_create(None, 0, 3, 260, 48, 65, 1.0, C.byref(out)) == EINVAL
    assert L.trxhip_tx_frontend_create(h, 0, 3, 260, 48, 65, 1.0, None) == EINVAL
    f = fe(trx, chans=3)
    x = torch.zeros((3, 260), dtype=torch.complex64, device="cuda:0")
    o = torch.empty(768, dtype=torch.complex64, device="cuda:0")
    assert L.trxhip_tx_frontend_push(f.h, C.c_void_p(x.data_ptr()), 260, 1, None, None, 1.0, None) == EINVAL   # no output
    assert L.trxhip_tx_frontend_push(f.h, None, 260, 1, C.c_void_p(o.data_ptr()), None, 1.0, None) == EINVAL
    assert L.trxhip_tx_frontend_push(f.h, C.c_void_p(x.data_ptr()), 100, 1, C.c_void_p(o.data_ptr()), None, 1.0, None) == EINVAL
    assert L.trxhip_tx_frontend_push(None, C.c_void_p(x.data_ptr()), 260, 1, C.c_void_p(o.data_ptr()), None, 1.0, None) == EINVAL
    assert L.trxhip_tx_frontend_seed(f.h, None, 260, 1, None) == EINVAL
    rows = torch.zeros((4, 192), dtype=torch.complex64, device="cuda:0")
    assert L.trxhip_synthesize_batch(h, C.c_void_p(rows.data_ptr()), 192, C.c_void_p(o.data_ptr()), 1, 8, 192, 16, None) == ENOTSUP
    assert L.trxhip_synthesize_batch(h, C.c_void_p(rows.data_ptr()), 192, C.c_void_p(o.data_ptr()), 1, 4, 192, 12, None) == ENOTSUP
    assert L.trxhip_synthesize_batch(h, None, 192, C.c_void_p(o.data_ptr()), 1, 4, 192, 16, None) == EINVAL
    assert L.trxhip_synthesize_batch(h, C.c_void_p(rows.data_ptr()), 100, C.c_void_p(o.data_ptr()), 1, 4, 192, 16, None) == EINVAL
    torch.cuda.synchronize()
