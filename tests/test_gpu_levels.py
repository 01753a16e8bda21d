"""GPU: per-channel level statistics of a decoded batch on the device (wvg_batch_levels,
wv_levels.hip) and the front end (api.scan_levels).

Files are tiny (block_samples 32; the multichannel ones longer than two tiles of the
kernel); their odd int counts leave later files' ranges off 16-byte boundaries.  The
expected records are Python integers (tests/levels_vectors.py) over the source arrays
(lossless files) or the oracle's decode (hybrid, float without WVG_OPEN_EXACT_FLOAT, the
corrupt golden file); never over the code under test.  Every field of every record is
compared.  (The encoder writes nothing for an array of no frames, so there is no
zero-frame file here; test_levels_host.py has the zero-frame records.)  Host side:
test_levels_host.py."""
import hashlib
import os

import numpy as np
import pytest

try:  # before the library loads: torch ships a HIP runtime of its own, and the process must hold one
    import torch  # noqa: F401
except ImportError:
    pass

from oracle import oracle as O
from synth import wvsynth as S
from tests import mc_vectors as M
from tests.levels_vectors import check, expected
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

ALL, EXACT = api.OPEN_ALL_CHANNELS, api.OPEN_EXACT_FLOAT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 4096
Q = 1 << 20  # a silence threshold that is 0 at 8 bits, 16 at 16, 4,096 at 24 and 2^20 at 32


class Case:
    def __init__(self, name, data, flags=0, ints=None, k=None, bps=None):
        self.name, self.data, self.flags = name, data, flags
        self.ints = ints  # (frames, channels) int32: what the decode leaves; None: not measurable
        self.k = k        # full scale is 2^k
        self.bps = bps    # bytes per sample of a lossless integer file (its MD5 is hashlib's over the source)
        self._want = {}

    def want(self, q):
        """the expected records for threshold q, computed once"""
        if q not in self._want:
            self._want[q] = expected(self.ints, self.k, q)
        return self._want[q]


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _oracle(data, nch):
    r = O.decode_file(data, chunk=CHUNK)
    assert r.status == 0 and r.nch == nch
    return r.samples.reshape(-1, nch)


@pytest.fixture(scope="module")
def corpus():
    """the mixed batch, made once (at the first test: the tile sizes come from the library)"""
    cases = []
    seed = 0
    for nch in (1, 2):
        for bits in (8, 16, 24, 32):
            for frames in (1, 33, 150):
                seed += 1
                x = S.audio_like(frames, nch, min(bits, 24), seed=seed)
                kw = {}
                if bits == 32:
                    x = (x.astype(np.int64) << 8).astype(np.int32)
                    kw["int32_zeros"] = 8
                p = S.EncParams(nch=nch, bytes_per_sample=bits // 8, block_samples=32,
                                terms=S.TERMS_DEFAULT if nch == 2 else [18, 2, 17], **kw)
                cases.append(Case(f"{nch}ch_{bits}b_{frames}", S.encode_pcm(x, p), 0, x, bits - 1, bits // 8))
    # the smallest input whose sum of squares carries out of 64 bits, through a real decode
    cx = np.full((4, 1), (-2 ** 23) << 8, dtype=np.int64).astype(np.int32)
    cases.append(Case("carry", S.encode_pcm(cx, S.EncParams(nch=1, bytes_per_sample=4, block_samples=32,
                                                             terms=[18, 2, 17], int32_zeros=8)), 0, cx, 31, 4))
    # full scale at 16 bits, both rails (api.scan_levels's peak is 0 dB)
    fs = S.audio_like(150, 2, 16, seed=77)
    fs[40, 0], fs[41, 1], fs[90, 1] = -32768, 32767, -32768
    cases.append(Case("full_scale_16", S.encode_pcm(fs, S.EncParams(nch=2, block_samples=32, terms=S.TERMS_DEFAULT)),
                      0, fs, 15, 2))
    # a float file: not measurable under EXACT_FLOAT, the reference's clipped 24-bit ints without
    rng = np.random.default_rng(7)
    fx = (S.audio_like(150, 2, 16, seed=90).astype(np.float32) / 32768.0 + rng.normal(0, 1e-6, (150, 2))).astype(
        np.float32)
    for i, v in enumerate((-0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-39, 0.0, 7e-8)):
        fx[(37 * i + 5) % 150, i % 2] = v
    fwv = S.encode_float_exact(fx, S.EncParams(block_samples=32, terms=S.TERMS_DEFAULT))
    cases.append(Case("float_exact", fwv, EXACT))
    cases.append(Case("float_clipped", fwv, 0, _oracle(fwv, 2), 23))
    cases.append(Case("dsd", _golden("dsd_mode3.wv")))
    # 3 and 17 channels, longer than two tiles and no multiple of one
    t3, t17 = api.levels_tile_frames(3), api.levels_tile_frames(17)
    f3, _, full3 = M.pcm_file([2, 1], 2 * t3 + 7, 16, seed=101, block_samples=512)
    cases.append(Case("3ch", f3, ALL, full3, 15))
    cases.append(Case("does_not_open", b"this is not a WavPack file, whatever its length " * 4))
    f17, _, full17 = M.pcm_file([2] * 8 + [1], 2 * t17 + 5, 24, seed=102, block_samples=128)
    cases.append(Case("17ch", f17, ALL, full17, 23))
    t4 = api.levels_tile_frames(4)
    f4, _, full4 = M.pcm_file([2, 2], 2 * t4 + 3, 16, seed=104, block_samples=512)
    cases.append(Case("4ch", f4, ALL, full4, 15))
    cor = _golden("corrupt_default.wv")
    cases.append(Case("corrupt", cor, 0, _oracle(cor, 2), 15))
    hx = S.audio_like(150, 2, 16, seed=103)
    hyb = S.encode_pcm(hx, S.EncParams(nch=2, block_samples=32, terms=S.TERMS_DEFAULT, hybrid=True,
                                       hybrid_bitrate=True, bitrate_x256=768))
    cases.append(Case("hybrid", hyb, 0, _oracle(hyb, 2), 15))
    return cases


def _batch(cases, kernel="auto"):
    b = api.DecodeBatch(CHUNK)
    b.set_kernel(kernel)
    for c in cases:
        i = b.add_file(c.data, c.flags)
        assert (i >= 0) == (c.name != "does_not_open"), c.name
    b.decode()
    return b


def _check_all(b, cases, q, what=""):
    L = b._L
    for i, c in enumerate(cases):
        got = b.file_levels(i)
        if c.ints is None:
            assert got is None, c.name
            assert L.wvg_batch_file_levels(b._b, i, None, 0) == _lib.WVG_ERR_OPEN, c.name
            continue
        assert got is not None and len(got) == c.ints.shape[1] == b.infos[i].reduced_channels, c.name
        check(got, c.want(q), (what, c.name, q))


def test_the_decode_leaves_what_the_expectations_assume(corpus):
    """(the int32 output itself: the sources and the oracle's decodes the records are made
    from; some ranges start off a 16-byte boundary)"""
    b = _batch(corpus)
    try:
        out = b.download()
        for i, c in enumerate(corpus):
            if c.ints is None:
                continue
            info = b.infos[i]
            assert (info.out_frames, info.reduced_channels) == c.ints.shape, c.name
            np.testing.assert_array_equal(out[info.out_offset: info.out_offset + c.ints.size], c.ints.reshape(-1),
                                          err_msg=c.name)
        assert len({b.infos[i].out_offset % 4 for i, c in enumerate(corpus) if c.ints is not None}) > 1
    finally:
        b.close()


@pytest.mark.parametrize("kernel", ["auto", "lane", "two_wave"])
def test_every_record_of_every_file(corpus, kernel):
    b = _batch(corpus, kernel)
    try:
        b.levels(Q)
        b.sync()
        _check_all(b, corpus, Q, kernel)
        # fewer records than channels on request; the channel count comes back
        i = [c.name for c in corpus].index("17ch")
        two = np.zeros(2, dtype=_lib.LEVELS_DTYPE)
        assert b._L.wvg_batch_file_levels(b._b, i, two.ctypes.data, 2) == 17
        check(two, corpus[i].want(Q)[:2], "cap_channels")
    finally:
        b.close()


def test_the_carry_through_a_real_decode(corpus):
    c = next(c for c in corpus if c.name == "carry")
    b = _batch([c])
    try:
        b.levels()
        b.sync()
        r = b.file_levels(0)[0]
        assert (int(r["sumsq_lo"]), int(r["sumsq_hi"]), int(r["clipped"])) == (0, 1, 4)
        assert int(r["min"]) == int(r["max"]) == -2 ** 31
        assert (int(r["active"]), int(r["first_active"]), int(r["last_active"])) == (4, 0, 3)
    finally:
        b.close()


def test_arguments_and_state(corpus):
    """WVG_ERR_ARG before any levels call and again after a re-upload; a batch reset and
    refilled with other files gives the new files' records"""
    L = _lib.lib()
    b = api.DecodeBatch(CHUNK)
    try:
        first, second = corpus[4:7], [corpus[10], corpus[2], corpus[20]]
        for c in first:
            b.add_file(c.data, c.flags)
        one = np.zeros(4, dtype=_lib.LEVELS_DTYPE)
        assert L.wvg_batch_levels(b._b, 0, None) == _lib.WVG_ERR_ARG  # before an upload
        b.decode()
        assert L.wvg_batch_file_levels(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG  # no levels call yet
        assert L.wvg_batch_levels(b._b, 0x80000000, None) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_file_levels(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG
        with pytest.raises(ValueError):
            b.levels(0x80000000)
        with pytest.raises(ValueError):
            b.levels(-1)
        b.levels(0x7FFFFFFF)
        b.sync()
        _check_all(b, first, 0x7FFFFFFF, "first")
        assert L.wvg_batch_file_levels(b._b, len(first), one.ctypes.data, 4) == _lib.WVG_ERR_ARG  # no such file
        with pytest.raises(RuntimeError):
            b.file_levels(-1)
        # a refilled batch starts over
        b.reset()
        for c in second:
            b.add_file(c.data, c.flags)
        b.upload()
        assert L.wvg_batch_file_levels(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG
        b.decode()
        assert L.wvg_batch_file_levels(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG
        b.levels(Q)
        b.sync()
        _check_all(b, second, Q, "refilled")
    finally:
        b.close()


def test_two_thresholds_queued_back_to_back(corpus):
    b = _batch(corpus)
    try:
        b.levels(0)
        b.levels(Q)
        b.sync()
        _check_all(b, corpus, Q, "second of two")
        b.levels(Q)
        b.levels(0)
        b.sync()
        _check_all(b, corpus, 0, "second of two, swapped")
    finally:
        b.close()


def _md5(c):
    x = c.ints.reshape(-1)
    if c.bps == 1:
        return hashlib.md5(((x + 128) & 0xFF).astype(np.uint8).tobytes()).digest()
    return hashlib.md5(np.ascontiguousarray(x.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :c.bps]).tobytes()).digest()


def test_queued_behind_md5_and_planar(corpus):
    """md5, planar and levels with no sync in between: all three results are right"""
    b = _batch(corpus)
    try:
        b.md5()
        lay = b.planar()
        b.levels(Q)
        b.sync()
        _check_all(b, corpus, Q, "behind md5 and planar")
        img = b.download_planar()
        for i, c in enumerate(corpus):
            if c.bps is None:
                continue
            assert bytes(b.file_md5(i).computed) == _md5(c), c.name
            off, rs, ch, fr = lay[i]
            got = img[off: off + ch * rs].reshape(ch, rs)[:, :fr]
            want = np.ascontiguousarray(c.ints.T).astype(np.float32) * np.float32(2.0 ** -c.k)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), c.name
    finally:
        b.close()


def test_on_torchs_current_stream(corpus):
    torch = pytest.importorskip("torch")
    b = _batch(corpus)
    try:
        dev = api.context_device()
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            b.levels(Q, stream=torch.cuda.current_stream(dev).cuda_stream)
        b.sync()
        _check_all(b, corpus, Q, "torch stream")
    finally:
        b.close()


def test_scan_levels(corpus):
    """equals the per-batch path; the derived floats are what their definitions give"""
    cases = [c for c in corpus if c.flags == 0]
    res = api.scan_levels([c.data for c in cases], 0, Q)
    assert len(res) == len(cases)
    for c, r in zip(cases, res):
        if c.ints is None:
            assert r is None, c.name
            continue
        want = c.want(Q)
        check(r["records"], want, ("scan", c.name))
        assert r["k"] == c.k and r["out_frames"] == c.ints.shape[0], c.name
        assert r["sumsq"] == [(w["sumsq_hi"] << 64) | w["sumsq_lo"] for w in want], c.name
        assert all(isinstance(v, float) for key in ("peak_dbfs", "rms_dbfs", "dc") for v in r[key]), c.name
    fs = res[[c.name for c in cases].index("full_scale_16")]
    assert fs["peak_dbfs"][0] == pytest.approx(0.0, abs=1e-12) and fs["peak_dbfs"][1] == pytest.approx(0.0, abs=1e-12)
    assert all(v < 0 for v in fs["rms_dbfs"]) and all(abs(v) < 1 for v in fs["dc"])
    # with the files' own flags: the multichannel ones, and the exact-float file is not measurable
    sub = [c for c in corpus if c.flags == ALL]
    for c, r in zip(sub, api.scan_levels([c.data for c in sub], ALL, 0)):
        check(r["records"], c.want(0), ("scan, all channels", c.name))
    fe = next(c for c in corpus if c.name == "float_exact")
    assert api.scan_levels([fe.data], EXACT) == [None]
    assert api.scan_levels([]) == []
