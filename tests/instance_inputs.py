"""Inputs for tests/test_gpu_kernel_instances.py that osmo_trx_amd.synth (the benchmark's workload generator) does not make:
1-SPS access / EDGE / dummy bursts and complex64 views of int16 batches.  Built from synth's public pieces; CPU tensors."""
import numpy as np
import torch

from osmo_trx_amd import synth
from osmo_trx_amd.trxhip import PARAMS_DTYPE, RACH, EXT_RACH, IDLE

CPU = torch.device("cpu")
# the dummy burst's midamble (GSM 05.02 5.2.6), as tests/test_gpu_parity.py::test_dummy_burst_detection_on_idle_slots uses it
DUMMY_MIDAMBLE = "01110001011100010111000101"


def _levels(n, gen, amp_range=(500.0, 20000.0), snr_range=(10.0, 30.0)):
    u = torch.rand((4, n), generator=gen)
    amp = amp_range[0] * torch.pow(torch.tensor(amp_range[1] / amp_range[0]), u[0])
    snr = snr_range[0] + (snr_range[1] - snr_range[0]) * u[1]
    return amp, snr, u[2], u[3]


def access_bursts_1sps(n, L, ext, seed, max_toa=63, p_noise=0.05):
    """Access bursts at 1 SPS, delays 0 .. min(max_toa, 60) symbols.  Returns (iq int16[n, L, 2], params, sync index[n])."""
    gen = synth._gen(seed, CPU)
    ts = torch.randint(0, 3, (n,), generator=gen) if ext else torch.zeros(n, dtype=torch.int64)
    wave = synth.modulate_basic_1sps(synth.access_burst_bits(n, ts, gen, CPU), L)
    amp, snr, u_dly, u_noise = _levels(n, gen)
    dly = u_dly * float(min(max_toa, 60))
    iq = synth._channel(wave, amp, snr, (dly - synth.BASE_TOA[1]) * 1.0, u_noise < p_noise, gen)
    params = np.zeros(n, dtype=PARAMS_DTYPE)
    params["type"] = EXT_RACH if ext else RACH
    params["max_toa"] = max_toa
    return iq, params, ts.numpy().astype(np.uint8)


def _fit(iq, L):
    """Cut or zero-pad int16[n, m, 2] to L samples."""
    out = torch.zeros((iq.shape[0], L, 2), dtype=torch.int16)
    m = min(L, iq.shape[1])
    out[:, :m] = iq[:, :m]
    return out


def edge_bursts_1sps(n, L, off, seed):
    """synth.make_edge_bursts decimated by 4 from sample `off`.  Returns (iq int16[n, L, 2], params, bits uint8[n, 444])."""
    iq, params, bits = synth.make_edge_bursts(n, "cpu", seed=seed)
    return _fit(iq[:, off::4].contiguous(), L), params, bits


def dummy_bursts_1sps(n, L, seed):
    """Bursts carrying the dummy midamble between random data bits, single-pulse GMSK at 1 SPS, slots typed IDLE."""
    gen = synth._gen(seed, CPU)
    bits = torch.randint(0, 2, (n, 148), generator=gen, dtype=torch.uint8)
    bits[:, :3] = 0
    bits[:, -3:] = 0
    bits[:, 61:87] = synth._bits(DUMMY_MIDAMBLE, CPU)
    wave = synth.modulate_basic_1sps(bits, L)
    amp, snr, u_dly, _ = _levels(n, gen, amp_range=(2000.0, 12000.0), snr_range=(20.0, 35.0))
    iq = synth._channel(wave, amp, snr, (u_dly * 3.0 - synth.BASE_TOA[1]) * 1.0, torch.zeros(n, dtype=torch.bool), gen)
    params = np.zeros(n, dtype=PARAMS_DTYPE)
    params["type"] = IDLE
    params["max_toa"] = 5
    return iq, params


def as_cf32(iq_int16, scale=1.0, dither=None):
    """int16[n, L, 2] -> complex64[n, L]: the samples as floats, plus (dither = a seed) uniform noise of +-1/4 LSB so that the
    values are no integers, times a float32 scale (one rounding per component; none for a power of two)."""
    x = iq_int16.to(torch.float32)
    if dither is not None:
        x = x + (torch.rand(x.shape, generator=synth._gen(int(dither), CPU)) - 0.5) * 0.5
    x = x * torch.tensor(scale, dtype=torch.float32)
    return torch.view_as_complex(x.contiguous())

