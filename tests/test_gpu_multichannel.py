"""GPU: files of more than two channels decoded with every channel
(WVG_OPEN_ALL_CHANNELS): the streams' blocks by the existing kernels into staging, then
wv_mc_interleave into N-channel frames.

Files are tiny (block_samples 32) and built by tests/mc_vectors.py from streams encoded
on their own; the expected output is the N-channel source array (lossless layouts) or
the oracle's decode of the stand-alone streams (hybrid), never the code under test.
Host side: test_multichannel_host.py."""
import ctypes
import hashlib

import numpy as np
import pytest

from synth import wvsynth as S
from tests import mc_vectors as M
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

ALL = api.OPEN_ALL_CHANNELS
BAD = _lib.WVG_ST_TIMEOUT | _lib.WVG_ST_UNSUPPORTED | _lib.WVG_ST_UNWRITTEN
POISON = 0x7F7F7F7F


def _decode(files, flags=ALL, chunk=4096, kernel="auto", bulk=False, poison=False):
    """-> (batch, indices, the whole int32 output); the caller closes the batch"""
    b = api.DecodeBatch(chunk)
    b.set_kernel(kernel)
    idx = b.add_files(files, flags) if bulk else [b.add_file(f, flags) for f in files]
    if poison:
        b.poison(0x7F)
    b.decode()
    return b, idx, b.download()


def _visible(b, out, i):
    info = b.infos[i]
    n = info.out_frames * info.reduced_channels
    return out[info.out_offset: info.out_offset + n].reshape(-1, info.reduced_channels)


def _check_clean(b, i, nblocks=None):
    res = b.result(i)
    assert res.crc_errors == 0 and res.exception == 0 and not (res.status_or & BAD), (i, hex(res.status_or))
    ends, st = b.file_blocks(i)
    assert len(st) == res.num_blocks and all(s & _lib.WVG_ST_CRC_CHECKED for s in st)
    if nblocks is not None:
        assert res.num_blocks == nblocks
    return res


def _roundtrip_cases():
    cases = []
    T3, T17 = api.interleave_tile_frames(3), api.interleave_tile_frames(17)
    k = 0
    for widths in ([2, 1], [1, 1, 1], [2, 1, 1, 2], [2] * 8 + [1]):
        for bits in (8, 16, 24, 32):
            for frames in (1, 31, 32, 33, 150):
                k += 1
                if bits != 16 and frames not in (33, 150):
                    continue  # every width at two lengths, 16-bit at all of them
                cases.append((f"{len(widths)}s{sum(widths)}ch_{bits}b_{frames}", widths, bits, frames, 32, k))
    # longer than one interleave tile and no multiple of it
    cases.append(("tile_n3", [2, 1], 16, 2 * T3 + 7, 512, 901))
    cases.append(("tile_n17", [2] * 8 + [1], 16, 2 * T17 + 5, 128, 902))
    return cases


@pytest.fixture(scope="module")
def roundtrip():
    """the lossless files, made once (at the first test, not at import: the tile sizes come
    from the library, which a test module must not load while the suite is collected)"""
    return [(name, *M.pcm_file(widths, frames, bits, seed=seed, block_samples=bs), widths, frames, bs)
            for name, widths, bits, frames, bs, seed in _roundtrip_cases()]


@pytest.mark.parametrize("bulk", [False, True], ids=["add_file", "add_files"])
@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
@pytest.mark.parametrize("chunk", [4096, 50])
def test_lossless_round_trips(roundtrip, chunk, kernel, bulk):
    files = [c[1] for c in roundtrip]
    b, idx, out = _decode(files, chunk=chunk, kernel=kernel, bulk=bulk)
    try:
        st = b.block_status()
        assert not (np.bitwise_or.reduce(st) & BAD)
        for i, (name, f, src, full, widths, frames, bs) in zip(idx, roundtrip):
            assert i >= 0, name
            info = b.infos[i]
            assert info.num_channels == info.reduced_channels == sum(widths) and info.out_frames == frames, name
            _check_clean(b, i, nblocks=len(widths) * ((frames + bs - 1) // bs))
            np.testing.assert_array_equal(_visible(b, out, i), full, err_msg=name)
            assert b.file_streams(i)[0] == widths
    finally:
        b.close()


def test_stream_zero_is_the_reference_under_two_channel_max():
    f, src, full = M.pcm_file([2, 1, 1, 2], 150, 16, seed=21)
    ref, errs = M.oracle_open(f, api.OPEN_2CH_MAX, 50)
    assert errs == 0
    b, idx, out = _decode([f, f], flags=ALL, chunk=50)
    b2, idx2, out2 = _decode([f], flags=api.OPEN_2CH_MAX, chunk=50)
    try:
        np.testing.assert_array_equal(_visible(b, out, 0)[:, :2], ref)
        # the batch's own OPEN_2CH_MAX decode is what it was
        assert b2.infos[0].reduced_channels == 2 and b2.infos[0].num_channels == 6
        np.testing.assert_array_equal(_visible(b2, out2, 0), ref)
        assert b2.result(0).crc_errors == 0 and b2.out_ints == ref.size
        assert b2.file_streams(0)[0] == [2]
    finally:
        b.close()
        b2.close()


def test_hybrid_streams_equal_the_oracle_on_each_stream_alone():
    widths = [2, 2]
    src = M.pcm_sources(widths, 150, 16, seed=31)
    encs = [S.encode_pcm(x, S.EncParams(nch=2, block_samples=32, terms=S.TERMS_DEFAULT, hybrid=True,
                                        hybrid_bitrate=True, bitrate_x256=768)) for x in src]
    alone = [M.oracle_open(e, 0, 50)[0] for e in encs]
    assert not np.array_equal(alone[0], src[0])
    b, idx, out = _decode([M.mux(encs, 4)], chunk=50)
    try:
        assert b.result(0).crc_errors == 0
        np.testing.assert_array_equal(_visible(b, out, 0), np.concatenate(alone, axis=1))
    finally:
        b.close()


@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
@pytest.mark.parametrize("mode", [1, 3])
def test_dsd_round_trip(mode, kernel):
    f, src, full = M.dsd_file([2, 2, 1], 150, mode, seed=mode)
    b, idx, out = _decode([f], chunk=50, kernel=kernel)
    try:
        _check_clean(b, 0, nblocks=15)
        assert b.infos[0].reduced_channels == 5
        np.testing.assert_array_equal(_visible(b, out, 0), full)
    finally:
        b.close()


def test_exact_float():
    rng = np.random.default_rng(41)
    src = [(rng.standard_normal((150, 2)) * 0.3).astype(np.float32) for _ in range(2)]
    encs = [S.encode_float_exact(x, S.EncParams(nch=2, block_samples=32, terms=S.TERMS_DEFAULT)) for x in src]
    b, idx, out = _decode([M.mux(encs, 4)], flags=ALL | api.OPEN_EXACT_FLOAT, chunk=50)
    try:
        _check_clean(b, 0)
        np.testing.assert_array_equal(_visible(b, out, 0), np.concatenate(src, axis=1).view(np.int32))
    finally:
        b.close()


def _mono(frames, seed):
    x = S.audio_like(frames, 1, 16, seed=seed)
    return S.encode_pcm(x, S.EncParams(nch=1, terms=[18, 2, 17], block_samples=32)), x


@pytest.mark.parametrize("bulk", [False, True], ids=["add_file", "add_files"])
def test_mixed_batch(bulk):
    m1, x1 = _mono(33, 51)
    m2, x2 = _mono(31, 52)
    m3, x3 = _mono(77, 53)
    a, _, fa = M.pcm_file([2, 1, 1, 2], 150, 16, seed=54)
    c, _, fc = M.pcm_file([2, 1], 45, 24, seed=55)
    files = [m1, a, m2, c, m3]
    b, idx, out = _decode(files, chunk=50, bulk=bulk)
    b0, idx0, out0 = _decode([m1, m2, m3], flags=0, chunk=50, bulk=bulk)
    try:
        assert b.infos[1].out_offset % 2 == 1  # the multichannel file's visible range starts at an odd int
        np.testing.assert_array_equal(_visible(b, out, 1), fa)
        np.testing.assert_array_equal(_visible(b, out, 3), fc)
        for i in (1, 3):
            _check_clean(b, i)
        for i, i0, x in ((0, 0, x1), (2, 1, x2), (4, 2, x3)):
            np.testing.assert_array_equal(_visible(b, out, i), x)
            np.testing.assert_array_equal(_visible(b, out, i), _visible(b0, out0, i0))
            r, r0 = b.result(i), b0.result(i0)
            assert [getattr(r, n) for n, _ in r._fields_] == [getattr(r0, n) for n, _ in r0._fields_]
            e, s = b.file_blocks(i)
            e0, s0 = b0.file_blocks(i0)
            assert e.tolist() == e0.tolist() and s.tolist() == s0.tolist()
            assert b.file_streams(i) == ([1], 0x4)
    finally:
        b.close()
        b0.close()


def test_poison_redecode_and_refill():
    a, _, fa = M.pcm_file([2, 1, 1, 2], 150, 16, seed=61)
    c, _, fc = M.pcm_file([1, 1, 1], 33, 16, seed=62)
    m1, x1 = _mono(33, 63)
    b, idx, out = _decode([m1, a], chunk=50, poison=True)
    try:
        v = _visible(b, out, 1)
        assert not (v == POISON).any()
        np.testing.assert_array_equal(v, fa)
        _check_clean(b, 1)
        b.decode()
        b.decode()
        out = b.download()
        np.testing.assert_array_equal(_visible(b, out, 1), fa)
        np.testing.assert_array_equal(_visible(b, out, 0), x1)
        b.reset()
        assert b.add_file(c, ALL) == 0 and b.add_file(m1, ALL) == 1 and b.add_file(a, ALL) == 2
        b.decode()
        out = b.download()
        np.testing.assert_array_equal(_visible(b, out, 0), fc)
        np.testing.assert_array_equal(_visible(b, out, 1), x1)
        np.testing.assert_array_equal(_visible(b, out, 2), fa)
        for i in range(3):
            _check_clean(b, i)
    finally:
        b.close()


def _bitstream_mid(wv, block):
    """an offset in the middle of the ID_WV_BITSTREAM payload of block `block` of the file"""
    pos = 0
    for _ in range(block):
        pos += 8 + int.from_bytes(wv[pos + 4:pos + 8], "little")
    end, p = pos + 8 + int.from_bytes(wv[pos + 4:pos + 8], "little"), pos + 32
    while p + 2 <= end:
        i, bl, hl = wv[p], wv[p + 1] * 2, 2
        if i & 0x80:
            bl += (wv[p + 2] << 9) + (wv[p + 3] << 17)
            hl = 4
        if (i & 0x3F) == 0x0A:
            return p + hl + bl // 2
        p += hl + bl
    raise AssertionError("no bitstream")


@pytest.mark.parametrize("where", [1, 2], ids=["last_block", "trailing_block"])
def test_md5(where):
    f, src, full = M.pcm_file([2, 1, 1, 2], 150, 16, seed=71, md5=where)
    digest = hashlib.md5(full.astype("<i2").tobytes()).digest()
    bad = bytearray(f)
    bad[_bitstream_mid(f, 2)] ^= 0x10  # a payload byte of stream 2's first block
    b = api.DecodeBatch(4096)
    try:
        assert b.add_file(f, ALL) == 0 and b.add_file(bytes(bad), ALL) == 1
        b.decode()
        b.md5()
        b.sync()
        b.download()
        good, hurt = b.file_md5(0), b.file_md5(1)
        assert bytes(good.stored) == digest and bytes(good.computed) == digest
        assert good.verdict == api.MD5_MATCH and good.bytes == full.size * 2
        assert hurt.verdict == api.MD5_MISMATCH and bytes(hurt.stored) == digest
        assert b.result(1).crc_errors >= 1 and b.result(0).crc_errors == 0
    finally:
        b.close()


def test_format_gives_the_source_bytes():
    a, _, fa = M.pcm_file([2, 1, 1, 2], 150, 16, seed=81)
    c, _, fc = M.pcm_file([2, 1], 45, 24, seed=82)
    m1, x1 = _mono(33, 83)
    b, idx, out = _decode([m1, a, c], chunk=50)
    try:
        b.format()
        pcm = b.download_pcm()
        want_a = fa.astype("<i2").tobytes()
        want_c = np.ascontiguousarray(fc.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
        assert pcm[b.pcm_offset(1): b.pcm_offset(1) + len(want_a)].tobytes() == want_a
        assert pcm[b.pcm_offset(2): b.pcm_offset(2) + len(want_c)].tobytes() == want_c
        assert pcm[b.pcm_offset(0): b.pcm_offset(0) + 66].tobytes() == x1.astype("<i2").tobytes()
    finally:
        b.close()


@pytest.mark.parametrize("cut_block", [5, 6, 7])
def test_truncated_in_the_middle_of_a_group(cut_block):
    """the file ends inside block `cut_block` (group 1 of 4 streams): the decode returns, and
    frames and stream 0's blocks are what the OPEN_2CH_MAX decode of the same bytes reports"""
    f, src, full = M.pcm_file([2, 1, 1, 2], 150, 16, seed=91)
    cut = _bitstream_mid(f, cut_block)
    t = f[:cut]
    ref, _ = M.oracle_open(t, api.OPEN_2CH_MAX, 50)
    b, idx, out = _decode([t], chunk=50)
    b2, idx2, out2 = _decode([t], flags=api.OPEN_2CH_MAX, chunk=50)
    try:
        info, res, res2 = b.infos[0], b.result(0), b2.result(0)
        assert info.out_frames == b2.infos[0].out_frames == ref.shape[0] and info.reduced_channels == 6
        if not res.exception:  # (set when any stream throws; stream 0's alone is res2's)
            assert res.frames == res2.frames
        assert res.exception >= res2.exception
        assert not (res.status_or & (_lib.WVG_ST_TIMEOUT | _lib.WVG_ST_UNWRITTEN))
        v = _visible(b, out, 0)
        np.testing.assert_array_equal(v[:, :2], ref)
        np.testing.assert_array_equal(v[:, :2], _visible(b2, out2, 0))
        e, s = b.file_blocks(0)
        e2, s2 = b2.file_blocks(0)
        assert e[: len(e2)].tolist() == e2.tolist() and s[: len(s2)].tolist() == s2.tolist()
        # whole groups before the cut decoded in every stream
        np.testing.assert_array_equal(v[:32], full[:32])
    finally:
        b.close()
        b2.close()


def test_a_group_that_departs_from_the_layout_is_unsupported():
    """two groups of widths 2,1,2, then groups of widths 1,2,1: the later blocks are not
    decoded (WVG_ST_UNSUPPORTED), their frames stay zero, nothing before them changes"""
    def enc(widths, seed):
        src = M.pcm_sources(widths, 150, 16, seed=seed)
        return src, [S.encode_pcm(x, S.EncParams(nch=w, block_samples=32,
                                                 terms=S.TERMS_DEFAULT if w == 2 else [18, 2, 17]))
                     for w, x in zip(widths, src)]
    sa, ea = enc([2, 1, 2], 101)
    sb, eb = enc([1, 2, 1], 102)
    ba, bb = M.split_blocks(M.mux(ea, 5)), M.split_blocks(M.mux(eb, 5))
    f = b"".join(bytes(x) for x in ba[:6] + bb[6:])
    b, idx, out = _decode([f], chunk=50)
    try:
        info, res = b.infos[0], b.result(0)
        assert info.out_frames == 150 and info.reduced_channels == 5 and b.file_streams(0)[0] == [2, 1, 2]
        assert res.status_or & _lib.WVG_ST_UNSUPPORTED and not (res.status_or & _lib.WVG_ST_TIMEOUT)
        assert res.num_blocks == 15
        ends, st = b.file_blocks(0)
        for s in range(3):  # per stream: two decoded blocks, then three unsupported ones
            assert not any(x & _lib.WVG_ST_UNSUPPORTED for x in st[5 * s: 5 * s + 2])
            assert all(x & _lib.WVG_ST_UNSUPPORTED for x in st[5 * s + 2: 5 * s + 5])
        v = _visible(b, out, 0)
        np.testing.assert_array_equal(v[:64], np.concatenate(sa, axis=1)[:64])
        assert not v[64:].any()
    finally:
        b.close()


def test_refused_combinations():
    f, _, _ = M.pcm_file([2, 1, 1, 2], 64, 16, seed=95)
    L = _lib.lib()
    b = api.DecodeBatch(4096)
    try:
        info = _lib.WvgFileInfo()
        assert L.wvg_batch_add_file_at(b._b, f, len(f), ALL, 10, ctypes.byref(info)) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_add_file_wvc(b._b, f, len(f), f, len(f), ALL, ctypes.byref(info)) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_add_file(b._b, f, len(f), ALL | api.OPEN_2CH_MAX, ctypes.byref(info)) == _lib.WVG_ERR_ARG
        with pytest.raises(RuntimeError):
            b.add_file(f, ALL, start_sample=10)
        with pytest.raises(RuntimeError):
            b.add_file(f, ALL, wvc=f)
        assert b.infos == [] and b.out_ints == 0
        assert b.add_file(f, 0) == _lib.WVG_ERR_OPEN  # without the flag: the reference's refusal
        assert b.infos[0].error.startswith(b"only two channels supported!")
        assert L.wvg_stream_open(api._context(), f, len(f), ALL, 0, ctypes.byref(info)) is None
        assert info.open_ok == 0 and info.error
    finally:
        b.close()


def test_decode_all_channels_convenience():
    f, _, full = M.pcm_file([2] * 8 + [1], 100, 24, seed=97)
    got = api.decode_all_channels(f)
    assert got.shape == (100, 17)
    np.testing.assert_array_equal(got, full)
    x = S.audio_like(100, 2, 16, seed=98)
    np.testing.assert_array_equal(api.decode_all_channels(S.encode_pcm(x, S.EncParams(block_samples=32))), x)
