"""numpy restatement of the multi-ARFCN transmit front end, for the tests of trxhip_synthesize_batch / trxhip_tx_frontend_*:

  Synthesis(4, blockLen, 16)::rotate (Synthesis.cpp:66-104) over a continuous stream, zero history:
    cxvec_fft     forward, unnormalised 4-point DFT across the 4 rows at every time, with the +-1 / +-j butterflies of
                  orc_channelizer_rotate (oracle/trx_oracle.c)
    convolve_real y_k[t] = sum_i Y_k[t - 15 + i] * sub_k[i], float32, product then add, i ascending; sub_k from
                  orc_channelizer_subfilter (ChannelizerBase::initFilters, the same taps as the receive channelizer)
    interleave    out[4 t + k] = y_k[t]   (Synthesis.cpp:39-50; not reversed)
  RadioInterfaceMulti::pushBuffer (radioInterfaceMulti.cpp:316-362): Resampler(p, q, 16, bw) of every active path through the
  oracle's orc_resampler_rotate, zero rows elsewhere, the synthesis above, then (short)(x * scale)."""
import ctypes as C
import os

import numpy as np

import oracle_lib as O

F32 = np.float32
ACTIVE = {1: {0: 0}, 2: {0: 0, 3: 1}, 3: {1: 0, 0: 1, 3: 2}}       # chans -> {pchan: lchan}, radioInterfaceMulti.cpp:92-124, :214-231


def synthesis_taps():
    L = O.lib()
    c = L.orc_channelizer_new(4, 192, 16)
    taps = np.array([np.ctypeslib.as_array(L.orc_channelizer_subfilter(c, k), shape=(16,)).copy() for k in range(4)],
                    dtype=F32)
    L.orc_channelizer_free(c)
    return taps


def dft4(rows):
    """rows: complex64[4, n] -> complex64[4, n], the butterflies of orc_channelizer_rotate, component by component in float32"""
    xr = [np.ascontiguousarray(r.real, dtype=F32) for r in rows]
    xi = [np.ascontiguousarray(r.imag, dtype=F32) for r in rows]
    t1r, t1i = xr[0] + xr[2], xi[0] + xi[2]
    t2r, t2i = xr[0] - xr[2], xi[0] - xi[2]
    t3r, t3i = xr[1] + xr[3], xi[1] + xi[3]
    t4r, t4i = xr[1] - xr[3], xi[1] - xi[3]
    out = np.empty((4, rows.shape[1]), dtype=np.complex64)
    out[0].real, out[0].imag = t1r + t3r, t1i + t3i
    out[1].real, out[1].imag = t2r + t4i, t2i - t4r                    # t2 - j*t4
    out[2].real, out[2].imag = t1r - t3r, t1i - t3i
    out[3].real, out[3].imag = t2r - t4i, t2i + t4r                    # t2 + j*t4
    return out


def synthesis(rows, taps=None):
    """Synthesis(4, ., 16)::rotate of the whole stream rows (complex64[4, n]) from zero history -> complex64[4 n]"""
    taps = synthesis_taps() if taps is None else taps
    n = rows.shape[1]
    Y = dft4(rows)
    out = np.empty((n, 4), dtype=np.complex64)
    for k in range(4):
        yr = np.concatenate([np.zeros(15, F32), Y[k].real.astype(F32)])
        yi = np.concatenate([np.zeros(15, F32), Y[k].imag.astype(F32)])
        ar, ai = np.zeros(n, F32), np.zeros(n, F32)
        for i in range(16):
            h = taps[k, i]
            ar = ar + yr[i:i + n] * h
            ai = ai + yi[i:i + n] * h
        out[:, k].real, out[:, k].imag = ar, ai
    return out.reshape(-1)


def resample(x, p, q, bw=1.0):
    """Resampler(p, q, 16, bw)::rotate of the whole stream x (complex64[n], n % q == 0) from zero history (orc_resampler_*)"""
    L = O.lib()
    n_in = len(x)
    assert n_in % q == 0
    padded = np.concatenate([np.zeros(16, dtype=np.complex64), np.asarray(x, dtype=np.complex64)])
    out = np.zeros(n_in // q * p, dtype=np.complex64)
    r = L.orc_resampler_new(p, q, 16, float(bw))
    L.orc_resampler_rotate(r, padded[16:].ctypes.data, n_in, out.ctypes.data, len(out))
    L.orc_resampler_free(r)
    return out


def to_s16(y, scale):
    """(short)(x * scale) per component (convert_base.c:20-25), as int16[n, 2]"""
    v = y.view(F32).reshape(-1, 2) * F32(scale)
    return np.trunc(v).astype(np.int32).astype(np.int16)


def multi_chain(x, chans, p=48, q=65, bw=1.0, taps=None):
    """RadioInterfaceMulti::pushBuffer over a whole stream: x complex64[chans, n] -> wideband complex64[4 n p / q]"""
    n_times = x.shape[1] // q * p
    rows = np.zeros((4, n_times), dtype=np.complex64)
    for pchan, lchan in ACTIVE[chans].items():
        rows[pchan] = resample(x[lchan], p, q, bw)
    return synthesis(rows, taps)


def ref_convert_float_short(y, scale):
    """convert_float_short of the reference's generic-C build (oracle/_ref/libref_generic.so) as int16[n, 2]"""
    R = C.CDLL(os.path.join(O.REF_DIR, "libref_generic.so"))
    R.convolve_init()
    R.convert_init()
    R.convert_float_short.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int]
    src = np.ascontiguousarray(y.view(F32))
    out = np.zeros(src.shape, dtype=np.int16)
    R.convert_float_short(out.ctypes.data, src.ctypes.data, float(F32(scale)), len(src))
    return out.reshape(-1, 2)
