"""WVG_OPEN_DSD_AS_PCM on the device: a DSD file opened with the flag decodes into a staging
range and the decimation kernel (wv_dsdpcm.hip) writes 24-bit PCM at the DSD byte rate into
its visible range.  Expected values are the numpy restatement (tests/dsdpcm_vectors.py)
applied to what the same file gives without the flag -- exact integers, no tolerance -- and
every downstream call (format, md5, planar, levels, resample, decode_to_tensors) is checked
on those integers."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

try:  # before the library loads: torch ships a HIP runtime of its own, and the process must hold one
    import torch  # noqa: F401
except ImportError:
    pass

from synth import wvsynth as S
from tests import dsdpcm_vectors as DV
from tests import vectors as V
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PCM = api.OPEN_DSD_AS_PCM
TAPS = DV.formula_taps()


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _dsd(frames, nch=2, fs=False, mode=3, seed=0, block=700, log2=0, md5=False):
    dd = S.dsd_like(frames, 1 if fs else nch, seed=seed)
    if fs:
        dd = np.repeat(dd, 2, axis=1)
    p = S.DsdParams(nch=nch, false_stereo=fs, mode=mode, block_samples=block, rate_multiplier_log2=log2)
    if md5:
        p.write_md5 = 1
        p.md5 = S.source_md5(dd, 1, dsd=True)
    return S.encode_dsd(dd, p)


@pytest.fixture(scope="module")
def dsd_files():
    t = api.dsd_pcm_tile_frames(2)
    return [
        ("golden_mode0", _golden("dsd_mode0.wv")),
        ("golden_mode1", _golden("dsd_mode1.wv")),
        ("golden_mode3", _golden("dsd_mode3.wv")),
        ("mono_m3", _dsd(3001, 1, mode=3, seed=1)),
        ("stereo_m3_2t5", _dsd(2 * t + 5, 2, mode=3, seed=2)),
        ("false_stereo_m3", _dsd(2500, 2, fs=True, mode=3, seed=3)),
        ("stereo_m1", _dsd(3333, 2, mode=1, seed=4, block=900)),
        ("mono_m1", _dsd(api.dsd_pcm_tile_frames(1) + 1, 1, mode=1, seed=5, block=1024)),
    ]


@pytest.fixture(scope="module")
def pcm_file():
    return _golden("stereo16_default.wv")


def _decode(entries, kernel="lane", chunk=4096):
    """entries: (data, open_flags).  Returns (batch, indices, out); the caller closes."""
    b = api.DecodeBatch(chunk)
    b.set_kernel(kernel)
    idx = [b.add_file(d, f) for d, f in entries]
    b.decode()
    out = b.download()
    return b, idx, out


def _vis(out, info):
    n = info.out_frames * info.reduced_channels
    return out[info.out_offset: info.out_offset + n].reshape(info.out_frames, info.reduced_channels)


def _same_result(b, i, j):
    r, q = b.result(i), b.result(j)
    for name, _ in _lib.WvgFileResult._fields_:
        assert getattr(r, name) == getattr(q, name), name
    (e1, s1), (e2, s2) = b.file_blocks(i), b.file_blocks(j)
    assert np.array_equal(e1, e2) and np.array_equal(s1, s2)


@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
def test_flagged_equals_restated_unflagged(dsd_files, pcm_file, kernel):
    entries = []
    for _, d in dsd_files:
        entries += [(d, PCM), (d, 0)]
    entries.append((pcm_file, PCM))
    b, idx, out = _decode(entries, kernel)
    try:
        assert all(i >= 0 for i in idx)
        infos = list(b.infos)
        for k, (name, _) in enumerate(dsd_files):
            fl, un = infos[2 * k], infos[2 * k + 1]
            assert un.dsd_multiplier > 0 and un.bits_per_sample == 1 and un.bytes_per_sample == 1, name
            assert fl.bits_per_sample == 24 and fl.bytes_per_sample == 3, name
            assert fl.sample_rate * 8 == un.sample_rate, name
            for f in ("num_channels", "reduced_channels", "mode", "dsd_multiplier", "out_frames", "total_samples"):
                assert getattr(fl, f) == getattr(un, f), (name, f)
            assert fl.out_frames > 0
            want = DV.restate(_vis(out, un), TAPS)
            got = _vis(out, fl).astype(np.int64)
            assert np.array_equal(got, want), name
            assert int(np.abs(got).max()) <= DV.FULL
            _same_result(b, 2 * k, 2 * k + 1)
        plain_b, plain_idx, plain_out = _decode([(d, 0) for _, d in dsd_files] + [(pcm_file, 0)], kernel)
        try:
            pinfos = list(plain_b.infos)
            for k, (name, _) in enumerate(dsd_files):
                assert np.array_equal(_vis(out, infos[2 * k + 1]), _vis(plain_out, pinfos[k])), name
            # the flag changes nothing on a file that is not DSD: info (but the offset), output
            a, p = infos[-1], pinfos[-1]
            a_off, p_off = a.out_offset, p.out_offset
            a.out_offset = p.out_offset = 0
            assert bytes(a) == bytes(p)
            a.out_offset, p.out_offset = a_off, p_off
            assert np.array_equal(_vis(out, a), _vis(plain_out, p))
            # ... nor on the batch's size: the PCM file takes its own ints only
            assert b.out_ints - a_off == plain_b.out_ints - p_off
        finally:
            plain_b.close()
    finally:
        b.close()


def test_add_files_path_and_out_ints(dsd_files, pcm_file):
    """wvg_batch_add_files (threaded framing, merged at the batch's end) gives what one
    wvg_batch_add_file per file gives; an all-PCM batch keeps its size under the flag."""
    files = [d for _, d in dsd_files] + [pcm_file]
    b = api.DecodeBatch(4096)
    c = api.DecodeBatch(4096)
    p = api.DecodeBatch(4096)
    q = api.DecodeBatch(4096)
    try:
        b.add_files(files, PCM)
        b.decode()
        out = b.download()
        for d in files:
            c.add_file(d, 0)
        c.decode()
        ref = c.download()
        for fl, un in zip(b.infos, c.infos):
            if un.dsd_multiplier:
                assert np.array_equal(_vis(out, fl).astype(np.int64), DV.restate(_vis(ref, un), TAPS))
            else:
                assert np.array_equal(_vis(out, fl), _vis(ref, un))
        p.add_files([pcm_file, pcm_file], PCM)
        q.add_files([pcm_file, pcm_file], 0)
        assert p.out_ints == q.out_ints and [i.out_offset for i in p.infos] == [i.out_offset for i in q.infos]
    finally:
        for x in (b, c, p, q):
            x.close()


def test_poison_and_repeat(dsd_files):
    entries = []
    for _, d in dsd_files:
        entries += [(d, PCM), (d, 0)]
    b, idx, first = _decode(entries)
    try:
        b.poison(0x7F)
        b.decode()
        one = b.download().copy()
        b.decode()
        two = b.download().copy()
        assert np.array_equal(one, two)
        infos = list(b.infos)
        for k, (name, _) in enumerate(dsd_files):
            v = _vis(one, infos[2 * k])
            assert not (v == 0x7F7F7F7F).any(), name  # every int of the visible range is written
            assert np.array_equal(v, _vis(first, infos[2 * k])), name
            assert np.array_equal(v.astype(np.int64), DV.restate(_vis(one, infos[2 * k + 1]), TAPS)), name
    finally:
        b.close()


@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
def test_damaged_files_keep_the_relation(kernel):
    entries = []
    for mode in (0, 1, 3):
        g = _golden(f"dsd_mode{mode}.wv")
        for seed in (11, 12, 13):
            bad = V.corrupt(g, 100 * mode + seed, nflips=1, start=len(g) // 4)
            entries += [(bad, PCM), (bad, 0)]
    b, idx, out = _decode(entries, kernel)
    try:
        infos = list(b.infos)
        for k in range(0, len(entries), 2):
            assert idx[k] == k and idx[k + 1] == k + 1  # (a flipped payload byte leaves the file openable)
            fl, un = infos[k], infos[k + 1]
            assert fl.out_frames == un.out_frames
            assert b.result(k).crc_errors >= 1  # (the oracle counts one CRC error in each of these files)
            assert np.array_equal(_vis(out, fl).astype(np.int64), DV.restate(_vis(out, un), TAPS)), k
            _same_result(b, k, k + 1)
    finally:
        b.close()


@pytest.fixture(scope="module")
def downstream():
    """One batch of DSD64-rate files (byte rate 352,800), flagged and not: the batch, the
    flagged indices and the restatement's integers E per flagged file."""
    files = [_dsd(4101, 2, mode=3, seed=21, block=1500, log2=3, md5=True),
             _dsd(2999, 1, mode=1, seed=22, block=1000, log2=3),
             _dsd(1203, 2, fs=True, mode=3, seed=23, block=600, log2=3)]
    entries = []
    for d in files:
        entries += [(d, PCM), (d, 0)]
    b, idx, out = _decode(entries)
    infos = list(b.infos)
    E = [DV.restate(_vis(out, infos[2 * k + 1]), TAPS) for k in range(len(files))]
    for k in range(len(files)):
        assert np.array_equal(_vis(out, infos[2 * k]).astype(np.int64), E[k])
    yield b, infos, E, files
    b.close()


def test_format_is_three_byte_little_endian(downstream):
    b, infos, E, _ = downstream
    b.format()
    pcm = b.download_pcm()
    for k, e in enumerate(E):
        off = b.pcm_offset(2 * k)
        want = DV.le24(e)
        assert pcm[off: off + len(want)].tobytes() == want


def test_planar(downstream):
    b, infos, E, _ = downstream
    lay = b.planar()
    b.sync()
    img = b.download_planar()
    for k, e in enumerate(E):
        off, rs, ch, fr = lay[2 * k]
        assert off >= 0 and ch == e.shape[1] and fr == e.shape[0]
        assert lay[2 * k + 1][0] == -1  # the unflagged twin is still DSD bytes: not convertible
        got = img[off: off + ch * rs].reshape(ch, rs)[:, :fr]
        want = (e.astype(np.float32) * np.float32(2.0 ** -23)).T
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_levels(downstream):
    b, infos, E, _ = downstream
    thr = 0x01000000
    b.levels(thr)
    b.sync()
    for k, e in enumerate(E):
        got = b.file_levels(2 * k)
        assert got is not None and b.file_levels(2 * k + 1) is None
        want = api.levels_ints(e.astype(np.int32), 23, thr)
        assert got.tobytes() == want.tobytes()
        assert int(got["clipped"].sum()) == 0


def test_resample_to_an_eighth(downstream):
    b, infos, E, _ = downstream
    rate = int(infos[0].sample_rate)
    assert rate == 352800 and all(int(infos[2 * k].sample_rate) == rate for k in range(len(E)))
    lay = b.resample(rate // 8)
    b.sync()
    img = b.download_resampled()
    for k, e in enumerate(E):
        off, rs, ch, fr = lay[2 * k]
        assert off >= 0 and ch == e.shape[1] and fr == -(-e.shape[0] // 8)
        assert lay[2 * k + 1][0] == -1
        got = img[off: off + ch * rs].reshape(ch, rs)[:, :fr]
        want = api.resample_float(e.astype(np.int32), 23, rate, rate // 8)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_md5_is_not_comparable_and_hashes_the_pcm(downstream):
    b, infos, E, _ = downstream
    b.md5()
    b.sync()
    r = b.file_md5(0)
    assert r.has_stored == 1 and r.verdict == _lib.WVG_MD5_NOT_COMPARABLE
    assert bytes(r.computed) == hashlib.md5(DV.le24(E[0])).digest()
    assert r.bytes == 3 * E[0].size
    u = b.file_md5(1)  # the unflagged twin still matches its stored sum over the DSD bytes
    assert u.verdict == _lib.WVG_MD5_MATCH
    for k in (1, 2):
        q = b.file_md5(2 * k)
        assert q.verdict == _lib.WVG_MD5_NONE and bytes(q.computed) == hashlib.md5(DV.le24(E[k])).digest()


def test_wav_refuses_a_flagged_dsd_file(downstream):
    b, infos, E, _ = downstream
    b.format()
    n, rc = ctypes.c_int64(), ctypes.c_int32()
    L = _lib.lib()
    assert L.wvg_batch_wav(b._b, 0, None, 0, ctypes.byref(n), ctypes.byref(rc)) == _lib.WVG_ERR_ARG
    assert L.wvg_batch_wav(b._b, 1, None, 0, ctypes.byref(n), ctypes.byref(rc)) == 0 and n.value > 0


def test_refused_combinations():
    f = _golden("dsd_mode3.wv")
    L = _lib.lib()
    b = api.DecodeBatch(4096)
    try:
        info = _lib.WvgFileInfo()
        assert L.wvg_batch_add_file(b._b, f, len(f), PCM | api.OPEN_ALL_CHANNELS, ctypes.byref(info)) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_add_file_at(b._b, f, len(f), PCM, 10, ctypes.byref(info)) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_add_file_wvc(b._b, f, len(f), f, len(f), PCM, ctypes.byref(info)) == _lib.WVG_ERR_ARG
        with pytest.raises(RuntimeError):
            b.add_files([f], PCM | api.OPEN_ALL_CHANNELS)
        assert b.out_ints == 0 and len(b.infos) == 0
        info = _lib.WvgFileInfo()
        assert L.wvg_stream_open(api._context(), f, len(f), PCM, 0, ctypes.byref(info)) is None
        assert info.open_ok == 0 and info.error
        wpc = api.WavpackOpenFileInput(f, PCM)
        with pytest.raises(RuntimeError):
            api.WavpackUnpackSamples(wpc, np.zeros(4096 * 2, dtype=np.int32), 4096)
    finally:
        b.close()


def test_decode_to_tensors_at_44100(downstream, pcm_file):
    pytest.importorskip("torch")
    _, infos, E, files = downstream
    rows = api.decode_to_tensors(files, open_flags=PCM, sample_rate=44100)
    assert len(rows) == len(files)
    for k, (row, e) in enumerate(zip(rows, E)):
        assert row is not None
        assert tuple(row.shape) == (e.shape[1], -(-e.shape[0] // 8))
        want = api.resample_float(e.astype(np.int32), 23, 352800, 44100)
        assert np.array_equal(row.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # without the flag a DSD file has no row
    assert api.decode_to_tensors(files[:1], sample_rate=44100) == [None]
