"""GPU: the decoded batch as planar float32 at one sample rate on the device
(wvg_batch_resample, wv_resample.hip) and api.decode_to_tensors(sample_rate=...).

Files are tiny (block_samples 32 to 512; one file per rate long enough to cross two seams of
the kernel's tiles, the multichannel ones longer than one tile).  Two checks of every image:
  * bit for bit, as uint32, every float of it, against the kernel's own job builder and tile
    code run on the host (api.resample_float) over the expected ints -- the sources of the
    lossless files, the oracle's decode of the others -- laid out by the rules of
    include/wvgpu.h restated here;
  * within the derived tolerance of resample_vectors.tol against the float64 restatement of
    the definition (resample_vectors.resample64): the check that does not rest on the code
    under test.
Host side: test_resample_host.py.  The layout queries of a batch that is not uploaded are
checked here too: a batch needs a device."""
import ctypes
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
from tests import resample_vectors as rv
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

ALL, EXACT = api.OPEN_ALL_CHANNELS, api.OPEN_EXACT_FLOAT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 4096
OUT_RATES = (16000, 48000)
RATES = (8000, 16000, 22050, 32000, 44100, 48000, 12000)  # 12000: not a standard rate; it reduces to 3:4 and 1:4


class Case:
    def __init__(self, name, data, flags=0, ints=None, kind=None, rate=0):
        self.name, self.data, self.flags = name, data, flags
        self.ints = ints  # (frames, channels) int32: what the decode leaves; None: not resamplable at any rate
        self.kind = kind  # k of SCALE(k)
        self.rate = rate  # info.sample_rate


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _oracle(data, nch):
    r = O.decode_file(data, chunk=CHUNK)
    assert r.status == 0 and r.nch == nch
    return r.samples.reshape(-1, nch)


def _supported(in_rate, out_rate):
    if in_rate == out_rate:
        return True
    orig, new, _, K = rv.geometry(in_rate, out_rate)
    return orig <= 1024 and new <= 1024 and K <= 4096


def _seam_frames(rate, nch):
    """input frames that cross two tile seams at both output rates"""
    need = 0
    for out in OUT_RATES:
        t = api.resample_tile_frames(rate, out, nch)
        g = np.gcd(rate, out)
        need = max(need, -(-(2 * t + 5) * (rate // g) // (out // g)))
    return int(need)


@pytest.fixture(scope="module")
def corpus():
    cases = []
    seed = 0
    for k, rate in enumerate(RATES):
        for nch in (1, 2):
            for frames in (1, 33, 150):
                seed += 1
                bits = (8, 16, 24, 32)[seed % 4]
                x = S.audio_like(frames, nch, min(bits, 24), seed=seed)
                kw = {}
                if bits == 32:
                    x = (x.astype(np.int64) << 8).astype(np.int32)
                    kw["int32_zeros"] = 8
                p = S.EncParams(nch=nch, bytes_per_sample=bits // 8, block_samples=32, sample_rate=rate,
                                terms=S.TERMS_DEFAULT if nch == 2 else [18, 2, 17], **kw)
                cases.append(Case(f"{rate}_{nch}ch_{bits}b_{frames}", S.encode_pcm(x, p), 0, x, bits - 1, rate))
        nch = 1 + k % 2
        frames = _seam_frames(rate, nch)
        x = S.audio_like(frames, nch, 16, seed=200 + k)
        p = S.EncParams(nch=nch, bytes_per_sample=2, block_samples=512, sample_rate=rate,
                        terms=S.TERMS_DEFAULT if nch == 2 else [18, 2, 17])
        cases.append(Case(f"{rate}_seams", S.encode_pcm(x, p), 0, x, 15, rate))
    # a float file: not resamplable under EXACT_FLOAT, the reference's clipped 24-bit ints without
    fx = (S.audio_like(150, 2, 16, seed=90).astype(np.float32) / 32768.0).astype(np.float32)
    fwv = S.encode_float_exact(fx, S.EncParams(block_samples=32, terms=S.TERMS_DEFAULT))
    cases.append(Case("float_exact", fwv, EXACT))
    cases.append(Case("float_clipped", fwv, 0, _oracle(fwv, 2), 23, 44100))
    cases.append(Case("dsd", _golden("dsd_mode3.wv")))
    f3, _, full3 = M.pcm_file([2, 1], _seam_frames(44100, 3) // 2 + 9, 16, seed=101, block_samples=512,
                              sample_rate=44100)
    cases.append(Case("3ch", f3, ALL, full3, 15, 44100))
    cases.append(Case("does_not_open", b"this is not a WavPack file, whatever its length " * 4))
    f17, _, full17 = M.pcm_file([2] * 8 + [1], _seam_frames(22050, 17) // 2 + 5, 24, seed=102, block_samples=128,
                                sample_rate=22050)
    cases.append(Case("17ch", f17, ALL, full17, 23, 22050))
    cor = _golden("corrupt_default.wv")
    cases.append(Case("corrupt", cor, 0, _oracle(cor, 2), 15, 44100))
    hx = S.audio_like(150, 2, 16, seed=103)
    hyb = S.encode_pcm(hx, S.EncParams(nch=2, block_samples=32, terms=S.TERMS_DEFAULT, hybrid=True,
                                       hybrid_bitrate=True, bitrate_x256=768))
    cases.append(Case("hybrid", hyb, 0, _oracle(hyb, 2), 15, 44100))
    return cases


def _out_frames(c, out_rate):
    return c.ints.shape[0] if c.rate == out_rate else rv.out_frames(c.ints.shape[0], c.rate, out_rate)


def _layout(cases, out_rate, fixed):
    """[(offset, row_stride, channels, frames)] per file by the header's rules, and the total"""
    lay, off = [], 0
    for c in cases:
        if c.ints is None or not _supported(c.rate, out_rate):
            lay.append((-1, 0, 0, 0))
            continue
        fo, nch = _out_frames(c, out_rate), c.ints.shape[1]
        rs = fixed if fixed else (fo + 3) & ~3
        lay.append((off, rs, nch, min(fo, rs)))
        off += nch * rs
    return lay, off


_images = {}
_refs = {}


def _image(cases, out_rate, fixed):
    """the expected image (uint32) from the host run of the tile code; computed once per key"""
    key = (tuple(c.name for c in cases), out_rate, fixed)
    if key not in _images:
        lay, total = _layout(cases, out_rate, fixed)
        img = np.zeros(total, dtype=np.uint32)
        for c, (off, rs, nch, fr) in zip(cases, lay):
            if off >= 0:
                got = api.resample_float(c.ints, c.kind, c.rate, out_rate, rs, rs)
                img[off: off + nch * rs] = got.view(np.uint32).reshape(-1)
        img.setflags(write=False)
        _images[key] = (lay, img)
    return _images[key]


def _within_tol(cases, img, out_rate, fixed):
    """the image against the float64 restatement of the definition"""
    lay, _ = _layout(cases, out_rate, fixed)
    f = np.asarray(img).view(np.float32)
    for c, (off, rs, nch, fr) in zip(cases, lay):
        if off < 0:
            continue
        got = f[off: off + nch * rs].reshape(nch, rs)
        assert np.all(got.view(np.uint32)[:, fr:] == 0), c.name
        if c.rate == out_rate:
            want = (c.ints.T.astype(np.float32) * np.float32(2.0 ** -c.kind))[:, :fr]
            assert np.array_equal(got[:, :fr].view(np.uint32), want.view(np.uint32)), c.name
            continue
        key = (c.name, out_rate)
        if key not in _refs:
            _refs[key] = rv.resample64(rv.conv64(c.ints, c.kind), c.rate, out_rate)
        y64, s = _refs[key]
        d = np.abs(got[:, :fr].astype(np.float64) - y64[:, :fr])
        t = rv.tol(s[:, :fr], c.rate, out_rate)
        assert np.all(d <= t), (c.name, float(np.max(d / t)))


def _same(got, want, what):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:4].tolist(), [hex(v) for v in got[bad[:4]]],
                           [hex(v) for v in want[bad[:4]]])


def _batch(cases):
    b = api.DecodeBatch(CHUNK)
    for c in cases:
        b.add_file(c.data, c.flags)
    b.decode()
    return b


def _fixed_values(cases, out_rate):
    """T odd and short, odd between the lengths, and 2 mod 4 beyond the longest file"""
    longest = max(_out_frames(c, out_rate) for c in cases if c.ints is not None and _supported(c.rate, out_rate))
    return (37, 1001, (longest + 8) // 4 * 4 + 2)


@pytest.mark.parametrize("out_rate", OUT_RATES)
def test_mixed_batch(corpus, out_rate):
    b = _batch(corpus)
    try:
        # the decode leaves what the expectations assume
        out = b.download()
        for i, c in enumerate(corpus):
            if c.ints is not None:
                info = b.infos[i]
                assert (info.out_frames, info.reduced_channels, info.sample_rate) == c.ints.shape + (c.rate,), c.name
                np.testing.assert_array_equal(out[info.out_offset: info.out_offset + c.ints.size],
                                              c.ints.reshape(-1), err_msg=c.name)
        assert b.device_resampled_ptr() == 0  # none yet
        for fixed in (0,) + _fixed_values(corpus, out_rate):
            want_lay, want = _image(corpus, out_rate, fixed)
            assert b.resample_floats(out_rate, fixed) == want.size
            lay = b.resample(out_rate, fixed)
            assert lay == want_lay, fixed
            got = b.download_resampled()
            _same(got, want, (out_rate, fixed))
            _within_tol(corpus, got, out_rate, fixed)
        assert b.device_resampled_ptr() != 0
        names = [c.name for c in corpus]
        lay = b.resample(out_rate)
        for skip in ("dsd", "does_not_open", "float_exact"):
            assert lay[names.index(skip)] == (-1, 0, 0, 0)
        assert all(off % 4 == 0 and rs % 4 == 0 for off, rs, _, _ in lay if off >= 0)
    finally:
        b.close()


def test_a_rate_that_no_file_reaches(corpus):
    """out_rate 44101: 44100 : 44101 does not reduce -- those files take no room; a file at 44101 is copied"""
    x = S.audio_like(70, 2, 16, seed=300)
    own = Case("44101", S.encode_pcm(x, S.EncParams(nch=2, bytes_per_sample=2, block_samples=32, sample_rate=44101,
                                                     terms=S.TERMS_DEFAULT)), 0, x, 15, 44101)
    cases = [c for c in corpus if c.name.startswith("44100_2ch")][:2] + [own] + [corpus[0]]
    b = _batch(cases)
    try:
        lay = b.resample(44101)
        assert lay == [(-1, 0, 0, 0), (-1, 0, 0, 0), (0, 72, 2, 70), (-1, 0, 0, 0)]
        assert b.resample_floats(44101) == 144
        want = np.zeros((2, 72), dtype=np.float32)
        want[:, :70] = x.T.astype(np.float32) * np.float32(2.0 ** -15)
        _same(b.download_resampled(), want.reshape(-1), "44101")
        L = b._L
        o = ctypes.c_int64(5)
        assert L.wvg_batch_file_resample(b._b, 0, 44101, 0, ctypes.byref(o), None, None, None) == _lib.WVG_ERR_OPEN
        assert o.value == -1
    finally:
        b.close()


def test_caller_memory_and_queued_calls(corpus):
    torch = pytest.importorskip("torch")
    b = _batch(corpus)
    try:
        dev = api.context_device()
        s = torch.cuda.Stream(device=dev)
        b.planar(0)
        planar_before = b.download_planar().copy()
        keys = ((16000, 0), (48000, 37))
        outs = []
        for out_rate, fixed in keys:  # queued back to back, nothing waited for in between
            want = _image(corpus, out_rate, fixed)[1]
            out = torch.full((want.size + 3 + 4,), float("nan"), dtype=torch.float32, device=f"cuda:{dev}")
            lay = b.resample(out_rate, fixed, out=out[3: 3 + want.size], stream=s.cuda_stream)  # 12 bytes off
            assert lay == _layout(corpus, out_rate, fixed)[0]
            outs.append((out, want))
        b.sync()
        for out, want in outs:
            _same(out[3: 3 + want.size].cpu().numpy(), want, "tensor")
            assert torch.isnan(out[:3]).all() and torch.isnan(out[3 + want.size:]).all(), "guards"
        # one float short
        out, want = outs[0]
        assert b._L.wvg_batch_resample(b._b, 16000, 0, ctypes.c_void_p(out.data_ptr()), want.size - 1,
                                       None) == _lib.WVG_ERR_SPACE
        with pytest.raises(ValueError):
            b.resample(16000, 0, out=out[: want.size - 1])
        with pytest.raises(ValueError):
            b.resample(16000, 0, out=torch.zeros(want.size, dtype=torch.float32))  # not on the batch's device
        # more pairs of arguments than the batch keeps job tables for, into its own buffer and a tensor
        big = torch.empty(max(_image(corpus, r, f)[1].size for r in OUT_RATES for f in (0, 37, 41)), device=f"cuda:{dev}")
        for out_rate, fixed in ((16000, 37), (48000, 0), (16000, 41), (48000, 41), (16000, 0)):
            b.resample(out_rate, fixed, stream=s.cuda_stream)
            b.resample(out_rate, fixed, out=big, stream=s.cuda_stream)
        b.sync()
        want = _image(corpus, 16000, 0)[1]
        _same(b.download_resampled(), want, "own")
        _same(big[: want.size].cpu().numpy(), want, "big")
        # planar's image is its own
        _same(b.download_planar(), planar_before, "planar's image")
    finally:
        b.close()


def test_decode_to_tensors_at_one_rate(corpus):
    torch = pytest.importorskip("torch")
    cases = [c for c in corpus if c.ints is None or (c.ints.shape[1] == 2 and c.name != "float_clipped")]
    assert len({c.rate for c in cases if c.ints is not None}) >= 5 and any(c.ints is None for c in cases)
    dev = api.context_device()
    fixed = 1001
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        batch, lengths = api.decode_to_tensors([c.data for c in cases], ALL | EXACT, fixed_frames=fixed,
                                               sample_rate=16000)
        ragged = api.decode_to_tensors([c.data for c in cases], ALL | EXACT, sample_rate=16000)
        plain = api.decode_to_tensors([c.data for c in cases], ALL | EXACT)
        plain0 = api.decode_to_tensors([c.data for c in cases], ALL | EXACT, sample_rate=0)
    s.synchronize()
    conv = [c for c in cases if c.ints is not None]
    assert tuple(batch.shape) == (len(conv), 2, fixed) and batch.is_contiguous() and batch.device.index == dev
    assert list(lengths) == [min(_out_frames(c, 16000), fixed) for c in conv]
    want = _image(conv, 16000, fixed)[1]
    _same(batch.cpu().numpy().reshape(-1), want, "fixed")
    _within_tol(conv, want, 16000, fixed)
    assert len(ragged) == len(cases)
    for c, t in zip(cases, ragged):
        if c.ints is None:
            assert t is None, c.name
            continue
        fo = _out_frames(c, 16000)
        assert tuple(t.shape) == (2, fo), c.name
        _same(t.cpu().contiguous().numpy(), api.resample_float(c.ints, c.kind, c.rate, 16000), c.name)
    # sample_rate 0 is the call as it was
    for a, z in zip(plain, plain0):
        assert (a is None) == (z is None)
        if a is not None:
            assert tuple(a.shape) == tuple(z.shape) and torch.equal(a.view(torch.int32), z.view(torch.int32))
    mixed = [c for c in corpus if c.ints is not None][:8]
    assert len({c.ints.shape[1] for c in mixed}) > 1
    with pytest.raises(ValueError):
        api.decode_to_tensors([c.data for c in mixed], 0, fixed_frames=fixed, sample_rate=16000)
    with pytest.raises(ValueError):
        api.decode_to_tensors([mixed[0].data], 0, sample_rate=-1)


@pytest.mark.parametrize("out_rate", OUT_RATES)
def test_same_rate_files_are_planar(corpus, out_rate):
    b = _batch(corpus)
    try:
        for fixed in (0, 37):
            rl = b.resample(out_rate, fixed)
            pl = b.planar(fixed)
            r, p = b.download_resampled(), b.download_planar()
            n = 0
            for c, (ro, rrs, rch, rfr), (po, prs, pch, pfr) in zip(corpus, rl, pl):
                if c.ints is not None and c.rate == out_rate:
                    assert (rrs, rch, rfr) == (prs, pch, pfr), c.name
                    _same(r[ro: ro + rch * rrs], p[po: po + pch * prs], c.name)
                    n += 1
            assert n >= 7
    finally:
        b.close()


def test_layout_and_arguments(corpus):
    """the layout queries before an upload, and the argument checks"""
    L = _lib.lib()
    b = api.DecodeBatch(CHUNK)
    try:
        for c in corpus:
            b.add_file(c.data, c.flags)
        assert L.wvg_batch_resample(b._b, 16000, 0, None, 0, None) == _lib.WVG_ERR_ARG  # before an upload
        for out_rate, fixed in ((16000, 0), (48000, 0), (16000, 77), (44101, 0), (7, 3)):
            lay, total = _layout(corpus, out_rate, fixed)
            assert [b.file_resample(i, out_rate, fixed) for i in range(len(corpus))] == lay
            assert b.resample_floats(out_rate, fixed) == total
        b.decode()
        for rate, fixed in ((0, 0), (-5, 0), (1 << 31, 0), (16000, -1)):
            assert L.wvg_batch_resample(b._b, rate, fixed, None, 0, None) == _lib.WVG_ERR_ARG
            assert L.wvg_batch_resample_floats(b._b, rate, fixed) == _lib.WVG_ERR_ARG
            assert L.wvg_batch_file_resample(b._b, 0, rate, fixed, None, None, None, None) == _lib.WVG_ERR_ARG
            with pytest.raises(ValueError):
                b.resample(rate, fixed)
        assert L.wvg_batch_device_resampled(b._b) is None
        host = np.zeros(4, dtype=np.float32)
        assert L.wvg_batch_download_resampled(b._b, host.ctypes.data, 4) == _lib.WVG_ERR_ARG  # no image yet
        b.resample(16000)
        assert L.wvg_batch_download_resampled(b._b, host.ctypes.data, 0) == _lib.WVG_ERR_SPACE
        # a refilled batch starts over
        b.reset()
        c2 = corpus[10]
        b.add_file(c2.data, c2.flags)
        b.decode()
        b.resample(48000, 7)
        _same(b.download_resampled(), _image([c2], 48000, 7)[1], "refilled")
    finally:
        b.close()
