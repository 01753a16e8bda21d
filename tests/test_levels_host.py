"""The levels kernels' tile and combine code (wv_levels.h) run on the CPU through
wvg_levels_ints: the index code (head / 16-byte body / tail, the tiles' seams, the rows'
lane groups and their butterfly), the 128-bit carry and the first / last bookkeeping,
against Python integers, field for field.

Expected values are numpy / Python integers over the source arrays, never the code under
test; sumsq is sum(int(v) * int(v)) split at 2^64.  (The batch path needs a device:
test_gpu_levels.py.)"""
import numpy as np
import pytest

from tests.levels_vectors import check, expected
from wavpackdecoder_amd import _lib, api

CHANNELS = (1, 2, 3, 4, 5, 6, 17, 255)
KS = (7, 15, 23, 31)
I32 = np.iinfo(np.int32)


def at_phase(values, phase):
    """the same values in memory that starts `phase` ints past a 16-byte boundary"""
    big = np.zeros(values.size + 8, dtype=np.int32)
    base = (-(big.ctypes.data // 4)) % 4  # ints to the first 16-byte boundary
    lo = base + phase
    view = big[lo: lo + values.size]
    view[:] = values.reshape(-1)
    assert not view.size or (view.ctypes.data // 4) % 4 == phase
    return view.reshape(values.shape)


def lengths(nch):
    t = api.levels_tile_frames(nch)
    assert t >= 16 and t % 16 == 0 and t == max((4096 // nch) & ~15, 16)
    return t, (0, 1, t - 1, t, t + 1, 2 * t + 5)


def test_record_layout():
    assert np.dtype(_lib.LEVELS_DTYPE).itemsize == 64


@pytest.mark.parametrize("nch", CHANNELS)
def test_random_full_range_every_length_and_phase(nch):
    rng = np.random.default_rng(1000 + nch)
    for frames in lengths(nch)[1]:
        x = rng.integers(I32.min, I32.max, size=(frames, nch), dtype=np.int64, endpoint=True).astype(np.int32)
        want = expected(x, 31, 1 << 30)
        for phase in range(4):
            check(api.levels_ints(at_phase(x, phase), 31, 1 << 30), want, (nch, frames, phase))


@pytest.mark.parametrize("nch", CHANNELS)
@pytest.mark.parametrize("value", [I32.min, I32.max])
def test_all_one_rail(nch, value):
    for frames in lengths(nch)[1]:
        x = np.full((frames, nch), value, dtype=np.int32)
        check(api.levels_ints(at_phase(x, frames % 4), 31), expected(x, 31), (nch, frames, value))


@pytest.mark.parametrize("nch", CHANNELS)
def test_a_single_nonzero_sample_at_the_seams(nch):
    """first / last frame of a tile and of the file, one channel at a time; every other
    channel is all zero (-1 / -1) beside the active one"""
    t, _ = lengths(nch)
    frames = 2 * t + 5
    for pos in (0, t - 1, t, 2 * t - 1, 2 * t, frames - 1):
        for c in sorted({0, nch // 2, nch - 1}):
            x = np.zeros((frames, nch), dtype=np.int32)
            x[pos, c] = -3
            got = api.levels_ints(at_phase(x, (pos + c) % 4), 15)
            check(got, expected(x, 15), (nch, pos, c))
            assert int(got[c]["first_active"]) == pos and int(got[c]["last_active"]) == pos
            for o in range(nch):
                if o != c:
                    assert (int(got[o]["first_active"]), int(got[o]["last_active"]), int(got[o]["active"])) == (-1, -1, 0)


@pytest.mark.parametrize("nch", CHANNELS)
def test_first_and_last_in_other_tiles(nch):
    t, _ = lengths(nch)
    frames = 2 * t + 5
    x = np.zeros((frames, nch), dtype=np.int32)
    x[t - 1, 0] = 5
    x[2 * t + 1, 0] = -5
    x[t + 3, nch - 1] = 1
    check(api.levels_ints(x, 23), expected(x, 23), nch)


def test_the_smallest_carry_out_of_64_bits():
    x = np.full((4, 1), I32.min, dtype=np.int32)
    r = api.levels_ints(x, 31)[0]
    assert (int(r["sumsq_lo"]), int(r["sumsq_hi"]), int(r["clipped"])) == (0, 1, 4)
    assert int(r["min"]) == int(r["max"]) == I32.min
    check([r], expected(x, 31), "carry")
    t, _ = lengths(1)
    x = np.full((2 * t + 5, 1), I32.min, dtype=np.int32)
    check(api.levels_ints(x, 31), expected(x, 31), "carry, three tiles")
    assert int(api.levels_ints(x, 31)[0]["sumsq_hi"]) == (2 * t + 5) // 4


@pytest.mark.parametrize("k", KS)
def test_thresholds_and_rails(k):
    for q in (0, 1, 1 << (31 - k), (1 << (31 - k)) - 1, 0x7FFFFFFF):
        thr = q >> (31 - k)
        vals = [thr, thr + 1, -thr, -thr - 1, (1 << k) - 1, (1 << k) - 2, -(1 << k), -(1 << k) + 1, 0]
        vals = [v for v in vals if I32.min <= v <= I32.max]
        # one value a frame, in both channels at other frames; then each value alone in a file
        x = np.zeros((len(vals) + 3, 2), dtype=np.int32)
        x[1: 1 + len(vals), 0] = vals
        x[2: 2 + len(vals), 1] = vals[::-1]
        check(api.levels_ints(x, k, q), expected(x, k, q), (k, q))
        for v in vals:
            one = np.array([[0], [v], [0]], dtype=np.int32)
            got = api.levels_ints(one, k, q)
            check(got, expected(one, k, q), (k, q, v))
            assert int(got[0]["active"]) == int(v > thr or v < -thr)
            assert int(got[0]["clipped"]) == int(v >= (1 << k) - 1 or v <= -(1 << k))


def test_argument_errors():
    L = _lib.lib()
    x = np.zeros(1024, dtype=np.int32)
    out = np.zeros(256, dtype=_lib.LEVELS_DTYPE)
    call = lambda frames, nch, k, q: L.wvg_levels_ints(x.ctypes.data, frames, nch, k, q, out.ctypes.data)  # noqa: E731
    assert call(2, 2, 15, 0) == 0
    for nch in (0, -1, 256):
        assert call(1, nch, 15, 0) == _lib.WVG_ERR_ARG
        assert L.wvg_levels_tile_frames(nch) == _lib.WVG_ERR_ARG
    for k in (0, 8, 16, 24, 30, 32, -1):
        assert call(2, 2, k, 0) == _lib.WVG_ERR_ARG
    assert call(2, 2, 15, 0x7FFFFFFF) == 0
    assert call(2, 2, 15, 0x80000000) == _lib.WVG_ERR_ARG
    assert call(2, 2, 15, 0xFFFFFFFF) == _lib.WVG_ERR_ARG
    assert call(-1, 2, 15, 0) == _lib.WVG_ERR_ARG
    with pytest.raises(ValueError):
        api.levels_ints(np.zeros((2, 2), dtype=np.int32), 15, 0x80000000)
    with pytest.raises(ValueError):
        api.levels_tile_frames(256)
