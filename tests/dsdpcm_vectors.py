"""A restatement of the DSD-to-PCM filter of WVG_OPEN_DSD_AS_PCM (include/wvgpu.h) in numpy,
independent of the library: the tap formula in float64, the bits unpacked with
np.unpackbits to +-1, and an int64 correlation with the taps, 0x55 outside the file.

Expected values in tests/test_dsd_pcm_host.py and tests/test_gpu_dsd_pcm.py come from here,
never from the code under test."""
import functools

import numpy as np

NTAPS = 104          # taps over bits: 13 bytes of history centred on the output's byte
NBYTES = 13
HALO = 6
IDLE = 0x55          # the byte outside the file
FULL = (1 << 23) - 1


def formula_taps_float() -> np.ndarray:
    """h_t / sum |h| * (2^23 - 1) in float64, before the truncation."""
    t = np.arange(NTAPS, dtype=np.float64)
    x = np.clip((t - 51.5) * 0.99 / 8.0, -6.0, 6.0)
    px = np.pi * x
    sinc = np.where(px == 0.0, 1.0, np.sin(px) / np.where(px == 0.0, 1.0, px))
    h = sinc * np.cos(np.pi * x / 12.0) ** 2
    return h / np.abs(h).sum() * float(FULL)


@functools.lru_cache(maxsize=None)
def _formula_taps():
    return tuple(int(v) for v in np.trunc(formula_taps_float()))


def formula_taps() -> np.ndarray:
    """The integer taps by the formula (truncated toward zero), int64."""
    return np.array(_formula_taps(), dtype=np.int64)


def restate(src: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """y[m][c] = sum_t taps[t] * s[8 (m - 6) + t][c] over the +-1 bit stream of src's low
    bytes (MSB first), 0x55 bytes outside the file.  src: (frames, channels) ints; int64 out."""
    a = np.asarray(src)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    frames, nch = a.shape
    taps = np.asarray(taps, dtype=np.int64)
    assert taps.shape == (NTAPS,)
    out = np.zeros((frames, nch), dtype=np.int64)
    if frames == 0:
        return out
    by = (a.astype(np.int64) & 0xFF).astype(np.uint8)
    pad = np.full((HALO, nch), IDLE, dtype=np.uint8)
    by = np.concatenate([pad, by, pad], axis=0)                 # frames + 12 bytes a channel
    for c in range(nch):
        bits = np.unpackbits(by[:, c])                          # MSB first: the earliest bit first
        s = bits.astype(np.int64) * 2 - 1
        # windows of 104 bits starting at bit 8 m: one row per output
        win = np.lib.stride_tricks.sliding_window_view(s, NTAPS)[::8][:frames]
        out[:, c] = win @ taps
    return out


def le24(e: np.ndarray) -> bytes:
    """3-byte little-endian form of the integers (WavpackFormatSamples at 3 bytes)."""
    v = np.asarray(e, dtype=np.int64).reshape(-1) & 0xFFFFFF
    b = np.empty((v.size, 3), dtype=np.uint8)
    b[:, 0] = v & 0xFF
    b[:, 1] = (v >> 8) & 0xFF
    b[:, 2] = (v >> 16) & 0xFF
    return b.tobytes()
