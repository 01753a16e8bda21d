"""The planar-float kernel's tile code (wv_planar.h) run on the CPU through
wvg_planar_float: the index code (head / 16-byte body / tail on both sides, the tile's row
skew, the tiles' seams) and the conversion, against numpy, bit for bit.

Expected: plane c, frame f = conv(src[f, c]) for f < min(frames, row_len), +0.0 up to
row_stride; conv = v.astype(float32) * float32(2.0 ** -k), or the 32 bits unchanged for
kind 0.  The image is pre-filled with 0xFF bytes between guard floats: every float of it
must be written and the guards untouched.  (The batch layout -- wvg_batch_planar_floats,
wvg_batch_file_planar -- needs a batch, which needs a device: test_gpu_planar_float.py.)"""
import numpy as np
import pytest

from wavpackdecoder_amd import _lib

KINDS = (7, 15, 23, 31, 0)
CHANNELS = (1, 2, 3, 6, 17, 255)
GUARD = 8  # guard floats on each side of the image
GUARD_BITS = 0x7FC0BEEF
I32 = np.iinfo(np.int32)
SPECIAL = np.array([I32.min, I32.max, 0, -1, (1 << 24) + 1, -((1 << 24) + 1), (1 << 31) - 129, -((1 << 31) - 129),
                    1, 127, -128, 32767, -32768, (1 << 23) - 1, -(1 << 23), (1 << 24) + 3, (1 << 30) + 65],
                   dtype=np.int64).astype(np.int32)
# float32 patterns for kind 0: NaNs with payloads (quiet, signalling, negative), -0.0,
# denormals (the smallest, the largest, a negative one), infinities, ordinary values
BITS = np.array([0x7FC00001, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000400,
                 0x7F800000, 0xFF800000, 0x3F800000, 0xBF000000, 0x00000000], dtype=np.uint32).view(np.int32)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _tile(L, nch):
    t = L.wvg_planar_tile_frames(nch)
    assert t > 0 and t % 16 == 0
    return t


def _source(frames, nch, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(I32.min, I32.max, size=frames * nch, dtype=np.int64, endpoint=True).astype(np.int32)
    sp = BITS if kind == 0 else SPECIAL
    n = min(len(sp), x.size)
    if n:  # the special values spread over the array, the first and the last value included
        x[np.linspace(0, x.size - 1, n).astype(np.int64)] = sp[:n]
    return x.reshape(frames, nch)


def _expected(src, kind, row_len, row_stride):
    """uint32 bit patterns, shape (channels, row_stride)"""
    frames, nch = src.shape
    n = min(frames, row_len)
    want = np.zeros((nch, row_stride), dtype=np.uint32)
    v = src[:n].T
    if kind == 0:
        want[:, :n] = v.view(np.uint32)
    else:
        want[:, :n] = (v.astype(np.float32) * np.float32(2.0 ** -kind)).view(np.uint32)
    return want


def _shifted(dtype, n, shift):
    """an n-element array that starts `shift` elements past a 16-byte boundary"""
    raw = np.zeros(n + 8, dtype=dtype)
    lead = (-(raw.ctypes.data // 4)) % 4
    a = raw[lead + shift: lead + shift + n]
    assert (a.ctypes.data // 4) % 4 == shift % 4
    return a


def _run(L, src, kind, row_len, row_stride, src_shift=0, out_shift=0):
    frames, nch = src.shape
    s = _shifted(np.int32, max(src.size, 1), src_shift)
    s[: src.size] = src.reshape(-1)
    n = nch * row_stride
    buf = _shifted(np.uint32, n + 2 * GUARD, out_shift)  # (GUARD is a multiple of 4: the image keeps the phase)
    buf[:] = 0xFFFFFFFF
    buf[:GUARD] = GUARD_BITS
    buf[GUARD + n:] = GUARD_BITS
    img = buf[GUARD: GUARD + n]
    assert (img.ctypes.data // 4) % 4 == out_shift % 4
    rc = L.wvg_planar_float(s.ctypes.data, frames, nch, kind, row_len, row_stride, img.ctypes.data)
    assert rc == 0
    assert (buf[:GUARD] == GUARD_BITS).all() and (buf[GUARD + n:] == GUARD_BITS).all(), "guards"
    return img.reshape(nch, row_stride).copy()


def _check(L, src, kind, row_len, row_stride, src_shift=0, out_shift=0):
    got = _run(L, src, kind, row_len, row_stride, src_shift, out_shift)
    want = _expected(src, kind, row_len, row_stride)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (src.shape, kind, row_len, row_stride, src_shift, out_shift, bad[:4].tolist(),
                           [hex(got[tuple(b)]) for b in bad[:4]], [hex(want[tuple(b)]) for b in bad[:4]])


def test_tile_frames(L):
    for nch in range(1, 256):
        t = _tile(L, nch)
        assert t * nch <= 4096 or t == 16
    assert _tile(L, 1) == 4096 and _tile(L, 2) == 2048 and _tile(L, 255) == 16
    assert L.wvg_planar_tile_frames(0) == _lib.WVG_ERR_ARG and L.wvg_planar_tile_frames(256) == _lib.WVG_ERR_ARG


@pytest.mark.parametrize("nch", CHANNELS)
def test_shapes_ragged_rows(L, nch):
    """every frame count around the tile seams, the ragged layout's rows (row_len = frames,
    row_stride the next multiple of 4), every kind"""
    t = _tile(L, nch)
    for k, frames in enumerate((0, 1, t - 1, t, t + 1, 2 * t + 7)):
        for kind in KINDS:
            src = _source(frames, nch, kind, seed=1000 * nch + 10 * k + kind)
            _check(L, src, kind, frames, (frames + 3) & ~3)


@pytest.mark.parametrize("nch", CHANNELS)
def test_alignment(L, nch):
    """src 0..3 ints and the image 0..3 floats past a 16-byte boundary, rows of an odd length
    (row_stride == row_len: every row at another phase), shorter and longer than the file"""
    t = _tile(L, nch)
    frames = t + 1 if nch > 2 else 2 * t + 7
    short, long_ = frames - 4, frames + 6  # (frames is odd)
    assert short % 2 == 1 and long_ % 2 == 1 and 0 < short < frames < long_
    k = 0
    for src_shift in range(4):
        for out_shift in range(4):
            k += 1
            kind = KINDS[k % len(KINDS)]
            src = _source(frames, nch, kind, seed=7000 + 100 * nch + k)
            for row in (short, long_):
                _check(L, src, kind, row, row, src_shift, out_shift)


@pytest.mark.parametrize("nch", (1, 2, 3, 17))
def test_fixed_rows_around_the_file(L, nch):
    """fixed-frames rows: shorter than one tile, between tiles, much longer than the file
    (tiles that hold zeros only), and rows with a stride beyond their length"""
    t = _tile(L, nch)
    frames = t + 5
    for k, (row_len, row_stride) in enumerate(((1, 1), (37, 37), (t, t), (frames, frames + 3), (3 * t + 2, 3 * t + 2),
                                               (0, 0), (0, 5), (frames - 1, frames + 9))):
        kind = KINDS[k % len(KINDS)]
        _check(L, _source(frames, nch, kind, seed=300 + 10 * nch + k), kind, row_len, row_stride, k % 4, (k + 1) % 4)
    # a file without frames still owns its rows of zeros
    _check(L, np.zeros((0, nch), dtype=np.int32), 15, 37, 37, 1, 3)


@pytest.mark.parametrize("kind", (7, 15, 23, 31))
def test_scale_values(L, kind):
    """the values the conversion can get wrong: the int32 range's ends, the first integers a
    float32 cannot hold (round to nearest even), and what they scale to"""
    src = SPECIAL.reshape(-1, 1)
    got = _run(L, src, kind, len(SPECIAL), len(SPECIAL)).view(np.float32)[0]
    want = SPECIAL.astype(np.float32) * np.float32(2.0 ** -kind)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert got[0] == -(2.0 ** (31 - kind)) and got[1] == 2.0 ** (31 - kind)  # INT32_MAX rounds up to 2^31
    assert got[2] == 0 and not np.signbit(got[2])
    assert got[3] == -(2.0 ** -kind)
    assert got[4] == 2.0 ** (24 - kind) and got[5] == -(2.0 ** (24 - kind))  # 2^24 + 1 ties to even: 2^24
    assert got[6] == (2.0 ** 31 - 128) * 2.0 ** -kind  # 2^31 - 129 rounds up to 2^31 - 128
    assert got[15] == (2.0 ** 24 + 4) * 2.0 ** -kind  # 2^24 + 3 ties to even: 2^24 + 4
    if kind == 15:
        assert got[11] == 32767 / 32768 and got[12] == -1.0
    if kind == 23:
        assert got[13] == (2.0 ** 23 - 1) / 2.0 ** 23 and got[14] == -1.0


def test_bits_pass_through(L):
    src = BITS.reshape(-1, 1)
    got = _run(L, src, 0, len(BITS), len(BITS) + 3)[0]
    assert got[: len(BITS)].tolist() == BITS.view(np.uint32).tolist()
    assert got[len(BITS):].tolist() == [0, 0, 0]
    # and interleaved with a second channel
    two = np.stack([BITS, BITS[::-1]], axis=1)
    got = _run(L, two, 0, len(BITS), len(BITS), 1, 1)
    assert got[0].tolist() == BITS.view(np.uint32).tolist() and got[1].tolist() == BITS[::-1].view(np.uint32).tolist()


def test_arguments(L):
    src = np.zeros(8, dtype=np.int32)
    out = np.zeros(8, dtype=np.float32)
    call = lambda *a: L.wvg_planar_float(src.ctypes.data, *a, out.ctypes.data)  # noqa: E731
    assert call(4, 2, 15, 4, 4) == 0
    assert call(4, 0, 15, 4, 4) == _lib.WVG_ERR_ARG and call(4, 256, 15, 0, 0) == _lib.WVG_ERR_ARG
    assert call(4, 2, 16, 4, 4) == _lib.WVG_ERR_ARG and call(4, 2, -1, 4, 4) == _lib.WVG_ERR_ARG
    assert call(-1, 2, 15, 4, 4) == _lib.WVG_ERR_ARG and call(4, 2, 15, -1, 4) == _lib.WVG_ERR_ARG
    assert call(4, 2, 15, 4, 3) == _lib.WVG_ERR_ARG  # a stride shorter than the row
    assert L.wvg_planar_float(None, 4, 2, 15, 4, 4, out.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_planar_float(src.ctypes.data, 4, 2, 15, 4, 4, None) == _lib.WVG_ERR_ARG
    assert L.wvg_planar_float(None, 0, 2, 15, 0, 0, None) == 0


def test_header_and_binding_list_the_entry_points(L):
    names = ("wvg_batch_planar", "wvg_batch_planar_floats", "wvg_batch_file_planar", "wvg_batch_device_planar",
             "wvg_batch_download_planar", "wvg_planar_float", "wvg_planar_tile_frames")
    for n in names:
        assert n in _lib.EXPORTED and hasattr(L, n)
