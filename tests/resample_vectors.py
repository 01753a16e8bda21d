"""The resampler's definition (include/wvgpu.h) restated in numpy float64, for the host and GPU
suites of wvg_batch_resample.  Written from the definition, not from the library: the filter
table, the resampled signal, the per-output magnitude and the tolerance derived from them.
"""
from __future__ import annotations

import math

import numpy as np

LPW = 6
ROLLOFF = 0.99

# the pairs of the host suite
PAIRS = [(32000, 48000), (48000, 32000), (48000, 24000), (22050, 44100), (8000, 48000), (44100, 48000),
         (48000, 44100), (44100, 16000), (11025, 16000)]


def geometry(in_rate: int, out_rate: int):
    """(orig, new, width, K) of a rate pair."""
    g = math.gcd(in_rate, out_rate)
    orig, new = in_rate // g, out_rate // g
    base = min(orig, new) * ROLLOFF
    width = int(math.ceil(LPW * orig / base))
    return orig, new, width, 2 * width + orig


def table64(in_rate: int, out_rate: int) -> np.ndarray:
    """h64[new][K] in float64, before the flush and the rounding to float32."""
    orig, new, width, K = geometry(in_rate, out_rate)
    base = min(orig, new) * ROLLOFF
    p = np.arange(new, dtype=np.float64)[:, None]
    j = np.arange(K, dtype=np.float64)[None, :]
    t = np.clip((-p / new + (j - width) / orig) * base, -LPW, LPW)
    return np.sinc(t) * np.cos(np.pi * t / (2 * LPW)) ** 2 * (base / orig)  # np.sinc(t) = sin(pi t) / (pi t)


def out_frames(frames: int, in_rate: int, out_rate: int) -> int:
    orig, new, _, _ = geometry(in_rate, out_rate)
    return -(-frames * new // orig)


def _windows(x64: np.ndarray, in_rate: int, out_rate: int):
    """x[c][i * orig + j - width] for every block i: shape (C, blocks, K), zeros outside the file."""
    orig, new, width, K = geometry(in_rate, out_rate)
    x64 = np.atleast_2d(np.asarray(x64, dtype=np.float64))
    C, F = x64.shape
    nblk = -(-out_frames(F, in_rate, out_rate) // new)
    pad = np.zeros((C, width + nblk * orig + K), dtype=np.float64)
    pad[:, width: width + F] = x64
    idx = (np.arange(nblk) * orig)[:, None] + np.arange(K)[None, :]
    return pad[:, idx]


def resample64(x64: np.ndarray, in_rate: int, out_rate: int):
    """(y, S): the resampled rows (C, F') in float64 and S[n] = sum_j |h64[p][j] * x[...]|."""
    new = geometry(in_rate, out_rate)[1]
    h = table64(in_rate, out_rate)
    h = np.where(np.abs(h) < 2.0 ** -64, 0.0, h)
    w = _windows(x64, in_rate, out_rate)
    C, F = np.atleast_2d(x64).shape
    fo = out_frames(F, in_rate, out_rate)
    y = np.einsum("cik,pk->cip", w, h).reshape(C, -1)[:, :fo]
    s = np.einsum("cik,pk->cip", np.abs(w), np.abs(h)).reshape(C, -1)[:, :fo]
    assert y.shape[1] == fo and new > 0
    return y, s


def tol(s: np.ndarray, in_rate: int, out_rate: int) -> np.ndarray:
    """The derived bound on |y32 - y64|: the float32 rounding of each tap and of each 32-bit
    sample above 2^24 (2 * 2^-24 * S), the gamma_K bound of a K-step fma chain (K * 2^-24 * S)
    and libm-versus-numpy differences in the double table (within the remaining 2 * 2^-24 * S
    and the absolute 2^-40)."""
    K = geometry(in_rate, out_rate)[3]
    return (K + 4) * 2.0 ** -24 * s + 2.0 ** -40


def conv64(ints: np.ndarray, kind: int) -> np.ndarray:
    """planar's conversion in float64: (frames, C) ints -> (C, frames) of v * 2^-k, exact."""
    a = np.asarray(ints, dtype=np.int64)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    return a.T.astype(np.float64) * 2.0 ** -kind
