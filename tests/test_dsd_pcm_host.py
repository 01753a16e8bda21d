"""WVG_OPEN_DSD_AS_PCM on the host (no device): the committed tap table against its formula,
the kernel's tile code run on the CPU (wvg_dsd_pcm_ints, wv_dsdpcm.h) against the numpy
restatement of tests/dsdpcm_vectors.py bit for bit, and what wvg_probe_file reports with the
flag.  The filter is exact integer arithmetic: no tolerance anywhere but the +-1 the tap
check grants the formula's last libm bit."""
import ctypes
import os

import numpy as np
import pytest

from tests import dsdpcm_vectors as DV
from wavpackdecoder_amd import _lib, api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHANNELS = (1, 2, 3, 6, 255)


def _frames_cases(ch):
    t = api.dsd_pcm_tile_frames(ch)
    return [0, 1, 6, 7, 12, 13, t - 1, t, t + 1, 2 * t + 5]


def _phased(n, phase, fill=0):
    """An int32 array of n values whose first int lies `phase` ints past a 16-byte boundary."""
    raw = np.full(n + 8, fill, dtype=np.int32)
    base = (-(raw.ctypes.data >> 2)) & 3
    v = raw[base + phase: base + phase + n]
    assert ((v.ctypes.data >> 2) & 3) == phase or n == 0
    return v


def _run(src, sp=0, dp=0):
    """wvg_dsd_pcm_ints with the source at phase sp and the destination at phase dp; the
    destination is pre-filled, so an int the call does not write shows."""
    frames, ch = src.shape
    s = _phased(frames * ch, sp)
    s[:] = src.reshape(-1)
    d = _phased(frames * ch, dp, fill=0x7F7F7F7F)
    rc = _lib.lib().wvg_dsd_pcm_ints(s.ctypes.data, frames, ch, d.ctypes.data)
    assert rc == 0
    return d.reshape(frames, ch).astype(np.int64)


@pytest.fixture(scope="module")
def taps():
    return DV.formula_taps()


def test_taps_match_the_formula():
    t, s, a = api.dsd_pcm_taps()
    f = DV.formula_taps()
    assert t.shape == (104,) and t.dtype == np.int32
    assert int(np.abs(t.astype(np.int64) - f).max()) <= 1
    assert np.array_equal(t, t[::-1])
    assert not t[:4].any() and not t[100:].any()
    assert a <= (1 << 23) - 1
    assert s == int(t.astype(np.int64).sum()) and a == int(np.abs(t.astype(np.int64)).sum())
    # the issue's figures for this table
    assert int(np.count_nonzero(t)) == 96 and a == 8388570 and s == 5355358


def test_tile_frames():
    for ch in range(1, 256):
        t = api.dsd_pcm_tile_frames(ch)
        assert t % 16 == 0 and t >= 16 and (t * ch <= 4096 or t == 16)
    L = _lib.lib()
    assert L.wvg_dsd_pcm_tile_frames(0) == _lib.WVG_ERR_ARG and L.wvg_dsd_pcm_tile_frames(256) == _lib.WVG_ERR_ARG


def test_argument_errors():
    L = _lib.lib()
    x = np.zeros(8, dtype=np.int32)
    assert L.wvg_dsd_pcm_ints(x.ctypes.data, 4, 0, x.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_dsd_pcm_ints(x.ctypes.data, 4, 256, x.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_dsd_pcm_ints(x.ctypes.data, -1, 1, x.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_dsd_pcm_ints(None, 4, 1, x.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_dsd_pcm_ints(None, 0, 1, None) == 0
    assert L.wvg_dsd_pcm_taps(None, None, None) == _lib.WVG_ERR_ARG


@pytest.mark.parametrize("ch", CHANNELS)
def test_random_bytes_all_phases(ch, taps):
    rng = np.random.default_rng(1000 + ch)
    for k, frames in enumerate(_frames_cases(ch)):
        src = rng.integers(0, 256, size=(frames, ch), dtype=np.int64).astype(np.int32)
        want = DV.restate(src, taps)
        assert int(np.abs(want).max(initial=0)) <= DV.FULL
        for sp in range(4):
            for dp in range(4):
                got = _run(src, sp, dp)
                assert np.array_equal(got, want), (ch, frames, sp, dp)


@pytest.mark.parametrize("ch", CHANNELS)
def test_constant_patterns(ch, taps):
    _, s, _ = api.dsd_pcm_taps()
    for k, frames in enumerate(_frames_cases(ch)):
        for byte in (0xFF, 0x00, 0x55):
            src = np.full((frames, ch), byte, dtype=np.int32)
            got = _run(src, (k + 1) & 3, (k + 2) & 3)
            assert np.array_equal(got, DV.restate(src, taps)), (ch, frames, hex(byte))
            assert int(np.abs(got).max(initial=0)) <= DV.FULL
            inner = got[6: frames - 6] if frames > 12 else got[:0]
            if byte == 0xFF:
                assert (inner == s).all()
            elif byte == 0x00:
                assert (inner == -s).all()
            else:  # the idle pattern inside and outside: one value everywhere
                assert (got == got.reshape(-1)[0]).all() if got.size else True


@pytest.mark.parametrize("ch", CHANNELS)
def test_single_bits_pin_order_and_alignment(ch, taps):
    t = api.dsd_pcm_tile_frames(ch)
    frames = 2 * t + 5
    for n, f in enumerate((0, t - 1, t, frames - 1)):  # first / last frame of a tile and of the file
        c = (n * 7 + 1) % ch
        for bit in range(8):
            src = np.zeros((frames, ch), dtype=np.int32)
            src[f, c] = 1 << bit
            got = _run(src, bit & 3, (bit + n) & 3)
            want = DV.restate(src, taps)
            assert np.array_equal(got, want), (ch, f, bit)
            # the set bit is bit 7 - `bit` in time order: output m sees it at tap 8 (f - m + 6) + 7 - bit
            base = DV.restate(np.zeros((frames, ch), dtype=np.int32), taps)
            for m in range(max(0, f - 6), min(frames, f + 7)):
                tap = 8 * (f - m + 6) + 7 - bit
                assert got[m, c] - base[m, c] == 2 * int(taps[tap]), (ch, f, bit, m)


@pytest.mark.parametrize("ch", CHANNELS)
def test_only_the_low_byte_counts(ch, taps):
    rng = np.random.default_rng(2000 + ch)
    t = api.dsd_pcm_tile_frames(ch)
    for frames in (13, t + 1, 2 * t + 5):
        low = rng.integers(0, 256, size=(frames, ch), dtype=np.int64)
        high = rng.integers(-(1 << 23), 1 << 23, size=(frames, ch), dtype=np.int64) << 8
        dirty = (high | low).astype(np.int32)
        clean = low.astype(np.int32)
        a, b = _run(dirty, 1, 3), _run(clean, 1, 3)
        assert np.array_equal(a, b) and np.array_equal(a, DV.restate(clean, taps))


def test_api_wrapper_matches(taps):
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, size=(300, 2)).astype(np.int32)
    assert np.array_equal(api.dsd_pcm_ints(src).astype(np.int64), DV.restate(src, taps))
    assert np.array_equal(api.dsd_pcm_ints(src[:, 0]).astype(np.int64), DV.restate(src[:, :1], taps))


def _probe(data, flags):
    info = _lib.WvgFileInfo()
    rc = _lib.lib().wvg_probe_file(data, len(data), flags, 4096, ctypes.byref(info))
    return rc, info


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_probe_flagged_dsd_golden(mode):
    data = open(os.path.join(GOLDEN, f"dsd_mode{mode}.wv"), "rb").read()
    rc0, plain = _probe(data, 0)
    rc1, pcm = _probe(data, api.OPEN_DSD_AS_PCM)
    assert rc0 == 0 and rc1 == 0 and plain.dsd_multiplier > 0
    assert pcm.bits_per_sample == 24 and pcm.bytes_per_sample == 3
    assert plain.sample_rate % 8 == 0 and pcm.sample_rate == plain.sample_rate // 8
    for name in ("open_ok", "num_channels", "reduced_channels", "version", "mode", "is_float", "is_five",
                 "file_format", "lossy", "dsd_multiplier", "total_samples", "out_frames", "header_off", "header_len",
                 "trailer_off", "trailer_len"):
        assert getattr(pcm, name) == getattr(plain, name), name
    # OPEN_2CH_MAX combines as it does without the flag
    rc2, both = _probe(data, api.OPEN_DSD_AS_PCM | api.OPEN_2CH_MAX)
    rc3, red = _probe(data, api.OPEN_2CH_MAX)
    assert rc2 == rc3 == 0 and both.reduced_channels == red.reduced_channels and both.bits_per_sample == 24
    assert both.out_frames == red.out_frames


@pytest.mark.parametrize("name", ["stereo16_default.wv", "stereo24_high.wv", "mono16_high.wv", "float_hybrid.wv"])
def test_probe_flag_changes_nothing_on_pcm(name):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    rc0, plain = _probe(data, 0)
    rc1, pcm = _probe(data, api.OPEN_DSD_AS_PCM)
    assert rc0 == rc1 == 0
    assert bytes(plain) == bytes(pcm)


def test_probe_flag_with_all_channels_is_an_argument_error():
    data = open(os.path.join(GOLDEN, "dsd_mode3.wv"), "rb").read()
    rc, _ = _probe(data, api.OPEN_DSD_AS_PCM | api.OPEN_ALL_CHANNELS)
    assert rc == _lib.WVG_ERR_ARG
