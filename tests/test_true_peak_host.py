"""The true-peak kernels' tile and combine code (wv_tpeak.h) run on the CPU through
wvg_true_peak_ints: the index code (the halo, head / 16-byte body / tail, the tiles' seams,
the threads' runs and their butterfly), both exact arithmetic forms and the first-position
bookkeeping, against the restatement in Python integers (tests/true_peak_vectors.py), field
for field.  No tolerance anywhere.  (The batch path needs a device: test_gpu_true_peak.py.)

The definition's text gives the largest sum of |c| as 31,247,512; the table it prints sums
to 31,247,516 (2 x 15,623,758), which is what is asserted here."""
import numpy as np
import pytest

from tests.true_peak_vectors import ROW2_ABS_SUM, TABLE, check, derive_taps, expected, oversample_of, sine_45
from wavpackdecoder_amd import _lib, api

CHANNELS = (1, 2, 3, 6, 17, 129, 255)
KS = (7, 15, 23, 31)
OS = (1, 2, 4)
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
    t = api.true_peak_tile_frames(nch)
    assert 5 <= t <= 4352 and (t + 11) * nch <= 4530  # (255 channels: a halo wider than the tile)
    return t, (0, 1, 5, 6, 11, 12, t - 1, t, t + 1, 2 * t + 7)


def full_range(rng, frames, nch, k):
    return rng.integers(-(1 << k), (1 << k) - 1, size=(frames, nch), dtype=np.int64, endpoint=True).astype(np.int32)


def test_record_layout():
    dt = np.dtype(_lib.TRUE_PEAK_DTYPE)
    assert dt.itemsize == 48
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24, 32, 40, 44]
    assert dt.names == ("true_peak", "true_peak_pos", "overs", "sample_peak", "sample_peak_frame", "oversample", "k")


def test_the_taps():
    rows, margin = derive_taps()
    assert rows == TABLE and rows[3] == rows[1][::-1] and rows[2] == rows[2][::-1]
    assert api.true_peak_taps().tolist() == TABLE
    assert margin > 0.038
    assert all(sum(r) == 1 << 24 for r in TABLE)
    sums = [sum(abs(v) for v in r) for r in TABLE]
    assert max(sums) == sums[2] == ROW2_ABS_SUM and abs(ROW2_ABS_SUM / 2 ** 24 - 1.8625) < 1e-4
    assert (1 << 31) * ROW2_ABS_SUM < 1 << 56  # no sum leaves int64
    assert (1 << 28) * ROW2_ABS_SUM < 1 << 53  # the float64 form's limit (wv_tpeak.h)


def test_oversample_by_rate():
    L = _lib.lib()
    for rate, o in ((95999, 4), (96000, 2), (191999, 2), (192000, 1), (8000, 4), (44100, 4), (352800, 1)):
        assert L.wvg_true_peak_oversample(rate) == o == oversample_of(rate) == api.true_peak_oversample(rate)


@pytest.mark.parametrize("nch", CHANNELS)
def test_random_every_length_alignment_factor_and_depth(nch):
    """every frame count at every O; the alignment and the depth rotate so that each of the
    four of either meets each O and short and long files (k = 31 takes the int64 form, the
    others the float64 form)"""
    rng = np.random.default_rng(2000 + nch)
    _, lens = lengths(nch)
    for li, frames in enumerate(lens):
        for oi, o in enumerate(OS):
            k, phase = KS[(li + oi) % 4], (li // 4 + oi + li) % 4
            x = full_range(rng, frames, nch, k)
            got = api.true_peak_ints(at_phase(x, phase), k, o)
            check(got, expected(x, k, o), (nch, frames, o, k, phase))
    seen = {(KS[(li + oi) % 4], (li // 4 + oi + li) % 4) for li in range(len(lens)) for oi in range(3)}
    assert {k for k, _ in seen} == set(KS) and {p for _, p in seen} == {0, 1, 2, 3}


@pytest.mark.parametrize("o", OS)
def test_every_alignment_at_every_depth(o):
    rng = np.random.default_rng(77 + o)
    t = api.true_peak_tile_frames(3)
    for k in KS:
        x = full_range(rng, t + 9, 3, k)
        want = expected(x, k, o)
        for phase in range(4):
            check(api.true_peak_ints(at_phase(x, phase), k, o), want, (o, k, phase))


@pytest.mark.parametrize("nch", CHANNELS)
def test_single_impulses_at_the_tile_seam(nch):
    """an output of one tile depends on samples of its neighbour, at both signs"""
    t, _ = lengths(nch)
    frames = 2 * t + 7
    for i, f in enumerate((t - 6, t - 5, t - 1, t, t + 4, t + 5)):
        if f < 0:  # (a tile of 5 frames has no frame T - 6)
            continue
        for sign in (1, -1):
            c = (i + (sign > 0)) % nch
            for k, v in ((15, sign * 20000), (31, sign * 2000000000)):
                x = np.zeros((frames, nch), dtype=np.int32)
                x[f, c] = v
                for o in (2, 4):
                    want = expected(x, k, o)
                    assert want[c]["true_peak"] == abs(v) << 24 and want[c]["true_peak_pos"] == f * o
                    check(api.true_peak_ints(at_phase(x, (f + c) % 4), k, o), want, (nch, f, sign, k, o))


def test_two_equal_peaks_give_the_first():
    t = api.true_peak_tile_frames(1)
    # the same |y| at phases 1 and 3 of two frames: a dip between two equal samples
    for base in (8, t - 2, t - 1, 2 * t - 1):
        x = np.zeros((2 * t + 7, 1), dtype=np.int32)
        x[base], x[base + 1], x[base + 2] = 1000, 900, 1000
        want = expected(x, 15, 4)
        assert want[0]["true_peak_pos"] == 4 * base + 1 and want[0]["true_peak"] > 1000 << 24
        xp = [0] * 5 + [int(v) for v in x[:, 0]] + [0] * 6
        twin = abs(sum(a * b for a, b in zip(TABLE[3], xp[base + 1: base + 13])))  # frame base + 1, phase 3
        assert twin == want[0]["true_peak"]
        check(api.true_peak_ints(x, 15, 4), want, ("two phases", base))
    # the same |y| at opposite signs, in two tiles, in two channels' own orders
    x = np.zeros((2 * t + 7, 2), dtype=np.int32)
    x[t + 40, 0], x[3, 0] = -30000, 30000
    x[2 * t + 1, 1], x[t - 1, 1], x[t, 1] = 12345, -12345, 12345
    for o in OS:
        want = expected(x, 15, o)
        assert want[0]["true_peak_pos"] == 3 * o and want[0]["sample_peak_frame"] == 3
        assert want[1]["sample_peak_frame"] == t - 1
        check(api.true_peak_ints(x, 15, o), want, ("two signs", o))
    # all zero: peak 0 at position 0; no frames: peak 0 at position -1
    z = api.true_peak_ints(np.zeros((t + 3, 2), dtype=np.int32), 23, 4)
    assert [(int(r["true_peak"]), int(r["true_peak_pos"]), int(r["sample_peak_frame"])) for r in z] == [(0, 0, 0)] * 2
    e = api.true_peak_ints(np.zeros((0, 3), dtype=np.int32), 23, 2)
    assert [tuple(int(r[f]) for f in e.dtype.names) for r in e] == [(0, -1, 0, 0, -1, 2, 23)] * 3


def test_int32_min_run_leaves_2_to_the_55():
    """above 2^55: a 32-bit or an FP64 shortcut cannot hold it"""
    x = np.full((30, 1), I32.min, dtype=np.int32)
    want = expected(x, 31, 4)[0]
    assert (want["true_peak"], want["true_peak_pos"], want["overs"]) == (40539895659233280, 2, 18)
    assert want["true_peak"] > 1 << 55 and want["sample_peak"] == 1 << 31
    for phase in range(4):
        check(api.true_peak_ints(at_phase(x, phase), 31, 4), [want], phase)
    for o in (1, 2):
        check(api.true_peak_ints(x, 31, o), expected(x, 31, o), o)


@pytest.mark.parametrize("k,lo,hi", [(15, -32768, 32767), (31, I32.min, I32.max)])
def test_the_worst_case_pattern_at_both_rails(k, lo, hi):
    """row 2's sign pattern reads 1.86245 of full scale"""
    for flip in (1, -1):
        x = np.zeros((40, 1), dtype=np.int32)
        x[14:26, 0] = [hi if c * flip > 0 else lo for c in TABLE[2]]
        want = expected(x, k, 4)
        assert want[0]["true_peak_pos"] == 19 * 4 + 2
        assert abs(want[0]["true_peak"] / 2.0 ** (k + 24) - 1.86245) < 1e-4
        check(api.true_peak_ints(x, k, 4), want, (k, flip))
        check(api.true_peak_ints(x, k, 2), expected(x, k, 2), (k, flip, 2))


def test_a_wide_value_in_a_narrow_file():
    """a 16-bit file whose ints leave 2^28 in one tile: that tile takes the int64 form, its
    neighbours the float64 one, and the records do not show it"""
    t = api.true_peak_tile_frames(2)
    rng = np.random.default_rng(5)
    x = full_range(rng, 3 * t + 1, 2, 15)
    for f, v in ((t + 5, I32.max), (2 * t - 1, I32.min), (t - 3, (1 << 28) + 1), (7, 1 << 28)):
        y = x.copy()
        y[f, 1] = v
        for o in (2, 4):
            check(api.true_peak_ints(y, 15, o), expected(y, 15, o), (f, v, o))


def test_the_sine_between_the_samples():
    """sample peak -3.01 dBFS, true peak 0 dBTP: the feature visibly does its job"""
    x = sine_45(200)
    want = expected(x, 15, 4)
    r = api.true_peak_ints(x, 15, 4)
    check(r, want, "sine")
    assert int(r[0]["true_peak"]) == 555833285840
    assert 0.99 < int(r[0]["true_peak"]) / 2.0 ** 39 < 1.02
    assert abs(int(r[0]["true_peak"]) / 2.0 ** 39 - 1.01105) < 1e-5
    assert abs(int(r[0]["sample_peak"]) / 2.0 ** 15 - 0.70709) < 1e-5
    check(api.true_peak_ints(x, 15, 2), expected(x, 15, 2), "sine, 2x")
    assert int(api.true_peak_ints(x, 15, 1)[0]["true_peak"]) == 23170 << 24


def test_argument_errors():
    L = _lib.lib()
    x = np.zeros(1024, dtype=np.int32)
    out = np.zeros(256, dtype=_lib.TRUE_PEAK_DTYPE)
    ok = (x.ctypes.data, 4, 2, 15, 4, out.ctypes.data)
    assert L.wvg_true_peak_ints(*ok) == 0
    for i, bad in ((1, -1), (2, 0), (2, 256), (3, 16), (3, 0), (4, 0), (4, 3), (4, 8), (0, None), (5, None)):
        a = list(ok)
        a[i] = bad
        assert L.wvg_true_peak_ints(*a) == _lib.WVG_ERR_ARG, (i, bad)
    assert L.wvg_true_peak_tile_frames(0) == _lib.WVG_ERR_ARG and L.wvg_true_peak_tile_frames(256) == _lib.WVG_ERR_ARG
    assert L.wvg_true_peak_taps(None) == _lib.WVG_ERR_ARG
    with pytest.raises(ValueError):
        api.true_peak_tile_frames(0)
    with pytest.raises(ValueError):
        api.true_peak_ints(x.reshape(-1, 2), 15, 3)
