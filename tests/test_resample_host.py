"""The resampler on the CPU: the filter table (wvg_resample_filter) and the kernel's job
builder and tile code (wv_resample.h through wvg_resample_float) against the float64
restatement of the definition in resample_vectors.py, within the derived tolerance
tol[n] = (K + 4) * 2^-24 * S[n] + 2^-40; equal rates against planar's bits; the filter's
quality on a sine.  (The batch layout -- wvg_batch_resample_floats, wvg_batch_file_resample --
needs a batch, which needs a device, as planar's: test_gpu_resample.py checks it on a batch
that is not uploaded.)

Frame counts: an output length F' that an up-sampling pair cannot produce exactly (F' moves in
steps of more than one frame there) is replaced by the next one it can."""
import numpy as np
import pytest

from tests import resample_vectors as rv
from wavpackdecoder_amd import _lib, api

CHANNELS = (1, 2, 3, 17, 255)
KINDS = (7, 15, 23, 31)
GUARD = 8
GUARD_BITS = 0x7FC0BEEF


def _source(frames, nch, kind, seed):
    """(frames, nch) ints of a k-bit file with values on both rails, the first and last included"""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << kind), (1 << kind) - 1
    x = rng.integers(lo, hi, size=frames * nch, dtype=np.int64, endpoint=True)
    sp = np.array([lo, hi, hi, lo, 0, -1, 1, (1 << 24) + 1 if kind == 31 else hi - 1], dtype=np.int64)
    n = min(len(sp), x.size)
    x[np.linspace(0, x.size - 1, n).astype(np.int64)] = sp[:n]
    return x.astype(np.int32).reshape(frames, nch)


def _frames_for(target, in_rate, out_rate):
    """the fewest input frames whose F' is at least `target`"""
    orig, new, _, _ = rv.geometry(in_rate, out_rate)
    f = max(1, -(-target * orig // new))
    while rv.out_frames(f, in_rate, out_rate) < target:
        f += 1
    while f > 1 and rv.out_frames(f - 1, in_rate, out_rate) >= target:
        f -= 1
    return f


def _run(src, kind, in_rate, out_rate, row_len, row_stride, src_shift, out_shift):
    """wvg_resample_float into an image pre-filled with 0xFF between guards; returns uint32 (C, row_stride)"""
    frames, nch = src.shape
    raw = np.zeros(src.size + 8, dtype=np.int32)
    lead = (-(raw.ctypes.data // 4)) % 4
    s = raw[lead + src_shift: lead + src_shift + src.size]
    s[:] = src.reshape(-1)
    n = nch * row_stride
    rawo = np.zeros(n + 2 * GUARD + 8, dtype=np.uint32)
    leado = (-(rawo.ctypes.data // 4)) % 4
    buf = rawo[leado + out_shift: leado + out_shift + n + 2 * GUARD]
    buf[:] = 0xFFFFFFFF
    buf[:GUARD] = GUARD_BITS
    buf[GUARD + n:] = GUARD_BITS
    img = buf[GUARD: GUARD + n]
    rc = _lib.lib().wvg_resample_float(s.ctypes.data, frames, nch, kind, in_rate, out_rate, row_len, row_stride,
                                       img.ctypes.data)
    assert rc == 0
    assert np.all(buf[:GUARD] == GUARD_BITS) and np.all(buf[GUARD + n:] == GUARD_BITS), "a guard float was written"
    return img.reshape(nch, row_stride).copy()


def _check(got_bits, src, kind, in_rate, out_rate, row_len):
    """got_bits: uint32 (C, row_stride)"""
    y64, s = rv.resample64(rv.conv64(src, kind), in_rate, out_rate)
    n = min(y64.shape[1], row_len)
    got = got_bits.view(np.float32)
    assert np.all(np.isfinite(got))
    d = np.abs(got[:, :n].astype(np.float64) - y64[:, :n])
    t = rv.tol(s[:, :n], in_rate, out_rate)
    assert np.all(d <= t), f"worst error / tolerance {np.max(d / t):.3g}"
    assert np.all(got_bits[:, n:] == 0), "frames past the file are +0.0f"


@pytest.mark.parametrize("in_rate,out_rate", rv.PAIRS)
def test_filter_matches_definition(in_rate, out_rate):
    orig, new, width, h = api.resample_filter(in_rate, out_rate)
    assert (orig, new, width, h.shape[1]) == rv.geometry(in_rate, out_rate)
    assert h.shape == (new, 2 * width + orig) and h.dtype == np.float32
    h64 = rv.table64(in_rate, out_rate)
    assert np.all(np.abs(h.astype(np.float64) - h64) <= 2.0 ** -24 * np.abs(h64) + 2.0 ** -60)
    small = np.abs(h64) < 2.0 ** -64
    assert np.all(h.view(np.uint32)[small] == 0), "a flushed tap is +0.0f"
    assert np.all(np.abs(h[~small]) >= np.float32(2.0 ** -65))


def test_filter_unsupported_pairs():
    L = _lib.lib()
    for a, b in ((44100, 44101), (192000, 11025), (11025, 192000), (1024, 1), (0, 48000), (48000, 0)):
        assert L.wvg_resample_filter(a, b, None, None, None, None, 0) == _lib.WVG_ERR_ARG
        assert L.wvg_resample_tile_frames(a, b, 2) == _lib.WVG_ERR_ARG
        with pytest.raises(ValueError):
            api.resample_filter(a, b)
    # the rule decides: 441:80 is supported, 441:1280 has new > 1024
    assert L.wvg_resample_filter(11025, 32000, None, None, None, None, 0) == _lib.WVG_ERR_ARG
    assert api.resample_filter(176400, 32000)[:2] == (441, 80)
    assert L.wvg_resample_filter(176400, 32000, None, None, None, None, 0) > 0
    x = np.zeros((4, 1), dtype=np.int32)
    out = np.zeros(16, dtype=np.float32)
    assert L.wvg_resample_float(x.ctypes.data, 4, 1, 15, 44100, 44101, 4, 4, out.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_resample_float(x.ctypes.data, 4, 1, 0, 44100, 48000, 4, 4, out.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_resample_float(x.ctypes.data, 4, 1, 15, 44100, 48000, 8, 4, out.ctypes.data) == _lib.WVG_ERR_ARG


@pytest.mark.parametrize("nch", CHANNELS)
@pytest.mark.parametrize("in_rate,out_rate", rv.PAIRS)
def test_resample_float_matches_definition(in_rate, out_rate, nch):
    orig, new, width, K = rv.geometry(in_rate, out_rate)
    tile = api.resample_tile_frames(in_rate, out_rate, nch)
    assert tile > 0 and tile % new == 0
    counts = [1, max(width - 1, 1), width + 1, orig, orig + 1]
    counts += [_frames_for(t, in_rate, out_rate) for t in (tile - 1, tile, tile + 1, 2 * tile + 5)]
    for n, frames in enumerate(counts):
        fo = rv.out_frames(frames, in_rate, out_rate)
        kind = KINDS[(n + nch) % 4]
        src = _source(frames, nch, kind, seed=1000 * n + nch)
        # the row as long as the file, shorter, longer; a stride beyond it; every phase of both ends
        row_len = (fo, max(fo - 3, 1), fo + 5)[n % 3]
        row_stride = row_len + (0, 1, 6, 3)[(n + nch) % 4]
        got = _run(src, kind, in_rate, out_rate, row_len, row_stride, src_shift=n % 4, out_shift=(n // 2 + nch) % 4)
        _check(got, src, kind, in_rate, out_rate, row_len)


@pytest.mark.parametrize("shift", range(4))
def test_source_and_image_phases(shift):
    """every phase of the source against every phase of the image, across a tile seam"""
    in_rate, out_rate, nch = 44100, 48000, 3
    frames = _frames_for(api.resample_tile_frames(in_rate, out_rate, nch) + 7, in_rate, out_rate)
    src = _source(frames, nch, 23, seed=shift)
    fo = rv.out_frames(frames, in_rate, out_rate)
    ref = None
    for out_shift in range(4):
        got = _run(src, 23, in_rate, out_rate, fo, fo + 1, shift, out_shift)
        _check(got, src, 23, in_rate, out_rate, fo)
        ref = got if ref is None else ref
        assert np.array_equal(got, ref), "the bits do not depend on where the image lies"


def test_equal_rates_are_planar():
    rng = np.random.default_rng(5)
    for nch, frames, kind in ((1, 1, 7), (2, 4099, 15), (3, 2731, 23), (17, 500, 31), (2, 33, 0)):
        src = rng.integers(-(1 << 31), (1 << 31) - 1, size=(frames, nch), dtype=np.int64).astype(np.int32)
        for row_len, row_stride in ((frames, frames), (frames + 9, frames + 11), (max(frames - 5, 1), frames)):
            a = api.resample_float(src, kind, 44100, 44100, row_len, row_stride)
            b = api.planar_float(src, kind, row_len, row_stride)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert api.resample_tile_frames(48000, 48000, nch) == api.planar_tile_frames(nch)


@pytest.mark.parametrize("in_rate,out_rate", [(44100, 16000), (48000, 44100), (44100, 48000)])
def test_filter_quality(in_rate, out_rate):
    """a 0.5-amplitude sine of 1 kHz comes out as the same sine at the new rate"""
    m = np.arange(4000)
    x = np.round(0.5 * np.sin(2 * np.pi * 1000 * m / in_rate) * 2 ** 23).astype(np.int32).reshape(-1, 1)
    y = api.resample_float(x, 23, in_rate, out_rate)[0].astype(np.float64)
    n = np.arange(y.size)
    want = 0.5 * np.sin(2 * np.pi * 1000 * n / out_rate)
    assert y.size == rv.out_frames(4000, in_rate, out_rate) and y.size > 600
    assert np.max(np.abs(y - want)[200:-200]) <= 1e-3
    sums = api.resample_filter(in_rate, out_rate)[3].astype(np.float64).sum(axis=1)
    assert np.all(sums >= 1.0000 - 1e-6) and np.all(sums <= 1.0009)
