"""The receive front end per logical channel on the MI355X: trxhip_rx_frontend_create_chans() in its two modes.
MULTI (RadioInterfaceMulti::pullBuffer for 1..3 ARFCNs): every logical row bit for bit the four-row object's row of its
filterbank path and the oracle's Channelizer + Resampler chain, under any chunking, seeded mid-stream, at full size, and end to
end into the burst detector.  RESAMP (RadioInterfaceResamp::pullBuffer): int16 in, bit for bit the oracle's Resampler over
float32(int16) and the two separate calls."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL = -22
PCHAN = {1: (0,), 2: (0, 3), 3: (1, 0, 3)}                   # radioInterfaceMulti.cpp:92-124, :214-231
GEOMETRIES = [(65, 48, 192), (65, 96, 192), (52, 75, 300)]
UNFUSED = (65, 384, 384)                                     # q too long for a tile: channelize_kernel + resample_kernel
CHUNKS = (1, 7, 2, 19, 1, 30)


@pytest.fixture(scope="module")
def trx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from osmo_trx_amd import TrxHip
    return TrxHip(0)


def front_end(trx, **kw):
    from osmo_trx_amd.trxhip import RxFrontEnd
    return RxFrontEnd(trx, **kw)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def chunked_pull(fe, x, per_block, chunks=CHUNKS):
    pieces, pos = [], 0
    for nb in chunks:
        pieces.append(fe.pull(x[pos * per_block:(pos + nb) * per_block].contiguous(), nb))
        pos += nb
    torch.cuda.synchronize()
    return torch.cat(pieces, dim=1), pos


def oracle_rows(wide, block_len, p, q, pchans, lead=None):
    """The oracle's chain on the CPU: Channelizer(4, block_len, 16)::rotate block by block, then Resampler(p, q, 16)::rotate on
    the paths `pchans`.  wide: int16[n_blocks*block_len*4, 2].  lead: the block in front of `wide` (None: the stream starts
    here); it runs through the channelizer first, and its last 16 channel samples are the resampler's history."""
    L = O.lib()
    n_blocks = len(wide) // (block_len * 4)
    if lead is None:
        lead = np.zeros((block_len * 4, 2), dtype=np.int16)
    x = np.concatenate([lead, wide]).astype(np.float32).view(np.complex64).reshape(n_blocks + 1, block_len * 4)
    c = L.orc_channelizer_new(4, block_len, 16)
    chan = np.zeros((4, (n_blocks + 1) * block_len), dtype=np.complex64)
    for b in range(n_blocks + 1):
        out = np.zeros((4, block_len), dtype=np.complex64)
        blk = np.ascontiguousarray(x[b])
        assert L.orc_channelizer_rotate(c, blk.ctypes.data, block_len * 4, out.ctypes.data) == 0
        chan[:, b * block_len:(b + 1) * block_len] = out
    L.orc_channelizer_free(c)
    r = L.orc_resampler_new(p, q, 16, 1.0)
    n_in = n_blocks * block_len
    rows = []
    for k in pchans:
        row = np.ascontiguousarray(chan[k])
        ref = np.zeros(n_in // q * p, dtype=np.complex64)
        L.orc_resampler_rotate(r, row[block_len:].ctypes.data, n_in, ref.ctypes.data, len(ref))
        rows.append(ref)
    L.orc_resampler_free(r)
    return rows


@pytest.mark.parametrize("p,q,block_len", GEOMETRIES + [UNFUSED])
@pytest.mark.parametrize("chans", [1, 2, 3])
def test_rows_equal_the_four_row_objects(trx, chans, p, q, block_len):
    """Row l is the four-row object's row pchan(l), bit for bit, in one piece and in chunks; rows == chans."""
    from osmo_trx_amd import synth
    n_blocks = 60
    wide = synth.make_wideband_stream(n_blocks, "cuda:0", block_len=block_len)
    four = front_end(trx, block_len=block_len, p=p, q=q)
    fe = front_end(trx, block_len=block_len, p=p, q=q, chans=chans)
    assert four.rows == 4 and fe.rows == chans
    want = four.pull(wide, n_blocks)
    whole = fe.pull(wide, n_blocks)
    torch.cuda.synchronize()
    assert whole.shape == (chans, n_blocks * block_len // q * p)
    for l, pc in enumerate(PCHAN[chans]):
        assert torch.equal(whole[l].view(torch.float32), want[pc].view(torch.float32)), (l, pc)
    fe.reset()
    chunked, pos = chunked_pull(fe, wide, block_len * 4)
    assert pos == n_blocks
    assert torch.equal(chunked.view(torch.float32), whole.view(torch.float32))
    four.close(); fe.close()


@pytest.mark.parametrize("p,q,block_len", GEOMETRIES + [UNFUSED])
def test_rows_against_the_oracle_directly(trx, p, q, block_len):
    """Every instance of the one fused kernel (and, for UNFUSED, the one fallback) against orc_channelizer_rotate block by block
    and orc_resampler_rotate on the rows' paths: the four-row object (chans=None) on paths 0..3, chans = 1..3 on the active
    ones.  At 65/48 the 60 blocks are a first tile fed from history, interior tiles and a partial last tile (5 blocks a tile)."""
    from osmo_trx_amd import synth
    n_blocks = 60
    wide = synth.make_wideband_stream(n_blocks, "cuda:0", block_len=block_len)
    ref = dict(zip(range(4), oracle_rows(wide.cpu().numpy(), block_len, p, q, range(4))))
    for chans in (None, 1, 2, 3):
        fe = front_end(trx, block_len=block_len, p=p, q=q, chans=chans)
        got = fe.pull(wide, n_blocks).cpu().numpy()
        pchans = range(4) if chans is None else PCHAN[chans]
        assert got.shape[0] == len(pchans)
        for l, pc in enumerate(pchans):
            assert bits_equal(got[l], ref[pc]), (chans, l, pc)
        fe.close()


@pytest.mark.parametrize("kind", ["chans3", "resamp"])
def test_time_shards_seeded_mid_stream(trx, kind):
    """Shards cut at 0, 1000, 1001, 3000, 4096, each on its own object seeded with the one block in front of it, concatenate
    to the one-piece output; an unseeded second shard differs."""
    from osmo_trx_amd import synth
    n_blocks = 4096
    cases = [(65, 48, 192), (65, 96, 192), (52, 75, 300)] if kind == "chans3" else [(65, 96, 1536), (52, 75, 1200)]
    for (p, q, bl) in cases:
        if kind == "chans3":
            kw, per = dict(block_len=bl, p=p, q=q, chans=3), bl * 4
            x = synth.make_wideband_stream(n_blocks, "cuda:0", seed=77 + p, block_len=bl)
        else:
            kw, per = dict(block_len=bl, p=p, q=q, chans=1, mode="resamp"), bl
            g = torch.Generator(device="cuda:0")
            g.manual_seed(91 + p)
            x = torch.randint(-32768, 32768, (n_blocks * bl, 2), generator=g, device="cuda:0", dtype=torch.int32).to(torch.int16)
        one = front_end(trx, **kw)
        full = one.pull(x, n_blocks)
        torch.cuda.synchronize()
        cuts = [0, 1000, 1001, 3000, n_blocks]
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            fe = front_end(trx, **kw)
            if a:
                fe.seed(x[(a - 1) * per:a * per].contiguous(), 1)
            else:
                fe.seed(None, 0)
            parts.append(fe.pull(x[a * per:b * per].contiguous(), b - a))
            fe.close()
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts, dim=1).view(torch.float32), full.view(torch.float32)), (p, q)
        cold = front_end(trx, **kw)
        unseeded = cold.pull(x[1000 * per:1001 * per].contiguous(), 1)
        torch.cuda.synchronize()
        assert not torch.equal(unseeded.view(torch.float32), parts[1].view(torch.float32))
        one.close(); cold.close()


def test_full_size_three_channels(trx):
    """262 144 blocks, chans = 3 (the size bench.py times).  On the device every row equals the four-row object's row over the
    whole stream; eight 64-block windows at fixed seeded offsets, the first and the last block among them, equal the oracle's
    chain on the CPU, which is fed the block in front of the window (its channel samples' last 16 are the resampler's history)."""
    from osmo_trx_amd import synth
    n_blocks, bl, p, q, nb = 1 << 18, 192, 65, 48, 64
    wide = synth.make_wideband_stream(n_blocks, "cuda:0")
    four = front_end(trx, block_len=bl, p=p, q=q)
    fe = front_end(trx, block_len=bl, p=p, q=q, chans=3)
    want = four.pull(wide, n_blocks)
    got = fe.pull(wide, n_blocks)
    torch.cuda.synchronize()
    assert got.shape == (3, n_blocks * 260)
    for l, pc in enumerate(PCHAN[3]):
        assert torch.equal(got[l].view(torch.float32), want[pc].view(torch.float32)), (l, pc)
    del want
    four.close()
    torch.cuda.empty_cache()
    rng = np.random.default_rng(20260)
    starts = [0, n_blocks - nb] + sorted(int(s) for s in rng.integers(1, n_blocks - nb, size=6))
    for s in starts:
        seg = wide[s * bl * 4:(s + nb) * bl * 4].cpu().numpy()
        lead = wide[(s - 1) * bl * 4:s * bl * 4].cpu().numpy() if s else None
        ref = oracle_rows(seg, bl, p, q, PCHAN[3], lead)
        win = got[:, s * 260:(s + nb) * 260].cpu().numpy()
        for l in range(3):
            assert bits_equal(win[l], ref[l]), (s, l)
    fe.close()


@pytest.mark.parametrize("p,q,block_len", [(65, 96, 1536), (52, 75, 1200)])
def test_resamp_mode(trx, p, q, block_len):
    """RESAMP: one piece == orc_resampler_rotate (bw 1.0) over float32(int16) with 16 zeros of history == convert_short_float +
    resample; any chunking == one piece; rows == 1."""
    n_blocks = 48
    rng = np.random.default_rng(p * q)
    s16 = rng.integers(-32768, 32768, size=(n_blocks * block_len, 2)).astype(np.int16)
    x = torch.from_numpy(s16).to("cuda:0")
    fe = front_end(trx, block_len=block_len, p=p, q=q, chans=1, mode="resamp")
    assert fe.rows == 1
    whole = fe.pull(x, n_blocks)
    torch.cuda.synchronize()
    n_in = n_blocks * block_len
    assert whole.shape == (1, n_in // q * p)
    L = O.lib()
    r = L.orc_resampler_new(p, q, 16, 1.0)
    padded = np.concatenate([np.zeros(16, dtype=np.complex64), s16.astype(np.float32).view(np.complex64)[:, 0]])
    ref = np.zeros(n_in // q * p, dtype=np.complex64)
    L.orc_resampler_rotate(r, padded[16:].ctypes.data, n_in, ref.ctypes.data, len(ref))
    L.orc_resampler_free(r)
    assert bits_equal(whole[0].cpu().numpy(), ref)
    two = trx.resample(torch.view_as_complex(trx.convert_short_float(x)).view(1, -1), p, q)
    torch.cuda.synchronize()
    assert torch.equal(two.view(torch.float32), whole.view(torch.float32))
    fe.reset()
    chunked, pos = chunked_pull(fe, x, block_len, chunks=(1, 7, 2, 19, 1, 18))
    assert pos == n_blocks
    assert torch.equal(chunked.view(torch.float32), whole.view(torch.float32))
    # a view that is only 4-byte aligned takes the kernel's one-sample loads
    off = torch.empty((n_in + 1, 2), dtype=torch.int16, device="cuda:0")
    off[1:] = x
    fe.reset()
    assert torch.equal(fe.pull(off[1:], n_blocks).view(torch.float32), whole.view(torch.float32))
    fe.close()


# The carrier synth.make_multi_arfcn_wideband() puts at k/4 cycles per wideband sample comes out of filterbank path (4 - k) % 4
# (the deinterleaver's path reversal, Channelizer.cpp:43-44; tests/test_gpu_aux_kernels.py::test_multi_arfcn_end_to_end).
PATH_OF_CARRIER = {0: 0, 1: 3, 3: 1}


@pytest.mark.parametrize("chans,carriers", [(1, (0,)), (2, (0, 3)), (3, (0, 1, 3)), (2, (0, 1))])
def test_end_to_end_into_the_detector(trx, chans, carriers):
    """Wideband int16 -> the chans-row front end -> 625-sample timeslots -> detect + demod (exact).  Every logical row whose
    filterbank path holds a carrier finds every burst of slots 1 .. n-2 with a TOA spread < 0.05 and BER < 1e-3 against that
    carrier's bits (the bars of test_multi_arfcn_end_to_end).  With carriers (0, 3) and chans = 2 the second carrier sits at
    -1/4 cycle per sample and comes out of path 1, which two channels do not use: logical row 1 (path 3) holds noise and is
    held to the empty channel's bar of that test (false alarms below 3 %); the case (0, 1) puts a carrier on both active paths."""
    from osmo_trx_amd import synth
    n_slots = 52 * 8
    wide, n_blocks, bits, tsc = synth.make_multi_arfcn_wideband(n_slots, "cuda:0", carriers=carriers)
    fe = front_end(trx, chans=chans)
    rs = fe.pull(wide, n_blocks)
    assert rs.shape == (chans, n_slots * 625)
    params = np.zeros(n_slots, dtype=O.PARAMS_DTYPE)
    params["type"], params["tsc"], params["max_toa"] = O.TSC, tsc, 20
    d_p = trx.params_tensor(params)
    carrier_on_path = {PATH_OF_CARRIER[k]: i for i, k in enumerate(carriers)}
    body = slice(1, n_slots - 1)
    means = []
    for l, pc in enumerate(PCHAN[chans]):
        res, soft = trx.detect_demod(rs[l].view(n_slots, 625), d_p, sps=4, full_scale=32767.0, exact=True)
        r = trx.results_to_numpy(res)
        if pc not in carrier_on_path:
            assert (r["rc"] > 0).mean() < 0.03, (l, pc)
            continue
        assert (r["rc"][body] == O.TSC).all(), (l, pc)
        toa = r["toa"][body]
        assert toa.std() < 0.05, (l, pc, toa.std())
        means.append(toa.mean())
        hard = (soft.cpu().numpy()[body] > 0.5).astype(np.uint8)
        ber = (hard[:, 3:145] != bits[carrier_on_path[pc]][body][:, 3:145]).mean()
        assert ber < 1e-3, (l, pc, ber)
    assert len(means) >= 1 and max(means) - min(means) < 0.05
    fe.close()


def test_refusals_on_the_device(trx):
    L, h = trx.L, trx.h
    out = C.c_void_p()
    for args in [(2, 1, 192, 65, 48), (-1, 1, 192, 65, 48),                                        # bad mode
                 (0, 0, 192, 65, 48), (0, 4, 192, 65, 48), (1, 0, 1536, 65, 96), (1, 2, 1536, 65, 96),   # bad chans
                 (0, 3, 191, 65, 48), (1, 1, 1500, 65, 96),                                         # block_len % q
                 (0, 3, 8, 1, 1), (0, 3, 192, 129, 48), (0, 3, 192, 0, 48), (0, 3, 192, 65, 0),         # block_len, p, q
                 (0, 3, 3073, 65, 3073), (1, 1, 3072, 1, 3072)]:                                    # q, q * ceil(256 / p)
        assert L.trxhip_rx_frontend_create_chans(h, *args, C.byref(out)) == EINVAL, args
        assert out.value is None
    assert L.trxhip_rx_frontend_create_chans(None, 0, 3, 192, 65, 48, C.byref(out)) == EINVAL
    assert L.trxhip_rx_frontend_create_chans(h, 0, 3, 192, 65, 48, None) == EINVAL
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    f = front_end(trx, chans=3)
    w = torch.zeros((192 * 4 + 4, 2), dtype=torch.int16, device="cuda:0")
    o = torch.empty((3, 260), dtype=torch.complex64, device="cuda:0")
    assert L.trxhip_rx_frontend_rows(f.h) == 3 and L.trxhip_rx_frontend_rows(None) == EINVAL
    assert L.trxhip_rx_frontend_pull(f.h, ptr(w), 1, ptr(o), 259, None) == EINVAL           # out_stride below a row
    assert L.trxhip_rx_frontend_pull(f.h, C.c_void_p(w.data_ptr() + 4), 1, ptr(o), 260, None) == EINVAL   # d_wide not 16-byte aligned
    assert L.trxhip_rx_frontend_pull(f.h, None, 1, ptr(o), 260, None) == EINVAL
    assert L.trxhip_rx_frontend_pull(f.h, ptr(w), 1, None, 260, None) == EINVAL
    assert L.trxhip_rx_frontend_pull(None, ptr(w), 1, ptr(o), 260, None) == EINVAL
    assert L.trxhip_rx_frontend_seed(f.h, None, 1, None) == EINVAL
    assert L.trxhip_rx_frontend_pull(f.h, ptr(w), 1, ptr(o), 260, None) == 0
    r = front_end(trx, block_len=1536, p=65, q=96, chans=1, mode="resamp")
    x = torch.zeros((1536 + 1, 2), dtype=torch.int16, device="cuda:0")
    y = torch.empty((1, 1040), dtype=torch.complex64, device="cuda:0")
    assert L.trxhip_rx_frontend_rows(r.h) == 1
    assert L.trxhip_rx_frontend_pull(r.h, ptr(x), 1, ptr(y), 1039, None) == EINVAL
    assert L.trxhip_rx_frontend_pull(r.h, C.c_void_p(x.data_ptr() + 2), 1, ptr(y), 1040, None) == EINVAL   # not 4-byte aligned
    assert L.trxhip_rx_frontend_pull(r.h, None, 1, ptr(y), 1040, None) == EINVAL
    assert L.trxhip_rx_frontend_pull(r.h, ptr(x), 1, None, 1040, None) == EINVAL
    assert L.trxhip_rx_frontend_seed(r.h, None, 1, None) == EINVAL
    assert L.trxhip_rx_frontend_pull(r.h, ptr(x), 1, ptr(y), 1040, None) == 0
    torch.cuda.synchronize()
    f.close(); r.close()


def test_resamp_rx_class(trx, tmp_path):
    """ResampRx (host shim) driven from C++ in runs of 1, 2, 3, ... chunks == the oracle's Resampler(65, 96) on the whole stream."""
    import os
    import subprocess
    from osmo_trx_amd import build as trx_build
    trx_build.build_all()
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "osmo_trx_amd", "lib", "sigproc_selftest")
    n_chunks, bl, p, q = 21, 1536, 65, 96
    s16 = np.random.default_rng(5).integers(-32768, 32768, size=(n_chunks * bl, 2)).astype(np.int16)
    (tmp_path / "in.s16").write_bytes(s16.tobytes())
    subprocess.check_call([exe, "resamp_rx", str(tmp_path / "in.s16"), str(n_chunks), str(bl), str(p), str(q), str(tmp_path / "out.cf32")])
    L = O.lib()
    r = L.orc_resampler_new(p, q, 16, 1.0)
    padded = np.concatenate([np.zeros(16, dtype=np.complex64), s16.astype(np.float32).view(np.complex64)[:, 0]])
    ref = np.zeros(n_chunks * bl // q * p, dtype=np.complex64)
    L.orc_resampler_rotate(r, padded[16:].ctypes.data, n_chunks * bl, ref.ctypes.data, len(ref))
    L.orc_resampler_free(r)
    assert bits_equal(np.fromfile(tmp_path / "out.cf32", dtype=np.complex64), ref)
