"""GPU: the decoded batch as planar float32 on the device (wvg_batch_planar, wv_planar.hip)
and the torch front end (api.decode_to_tensors).

Files are tiny (block_samples 32; the multichannel ones longer than one tile of the
kernel).  The expected planes are numpy's v.astype(float32) * float32(2.0 ** -k) -- or the
bits themselves for exact float -- over the source arrays (lossless files) or the oracle's
decode (hybrid, float without WVG_OPEN_EXACT_FLOAT, the corrupt golden file), laid out by
the rules of include/wvgpu.h restated here; never over the code under test.  Images are
compared as uint32, every float of them, and caller buffers carry guard floats around an
image that starts at an odd float.  Host side: test_planar_float_host.py."""
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
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

ALL, EXACT = api.OPEN_ALL_CHANNELS, api.OPEN_EXACT_FLOAT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 4096
GUARD = 5  # guard floats in front of a caller's image (odd: the image starts off a 16-byte boundary)
GUARD_BITS = 0x7FC0BEEF


class Case:
    def __init__(self, name, data, flags=0, ints=None, kind=None, any_flags=True):
        self.name, self.data, self.flags = name, data, flags
        self.ints = ints  # (frames, channels) int32: what the decode leaves; None: not convertible
        self.kind = kind  # k of SCALE(k), 0 for the bits
        self.any_flags = any_flags  # decodes the same under ALL | EXACT (decode_to_tensors has one flag set)


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
                cases.append(Case(f"{nch}ch_{bits}b_{frames}", S.encode_pcm(x, p), 0, x, bits - 1))
    # a float file: its bits under EXACT_FLOAT, the reference's clipped 24-bit ints without
    rng = np.random.default_rng(7)
    fx = (S.audio_like(150, 2, 16, seed=90).astype(np.float32) / 32768.0 + rng.normal(0, 1e-6, (150, 2))).astype(
        np.float32)
    for i, v in enumerate((-0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-39, 0.0, 7e-8)):
        fx[(37 * i + 5) % 150, i % 2] = v
    fwv = S.encode_float_exact(fx, S.EncParams(block_samples=32, terms=S.TERMS_DEFAULT))
    cases.append(Case("float_exact", fwv, EXACT, fx.view(np.int32), 0))
    cases.append(Case("float_clipped", fwv, 0, _oracle(fwv, 2), 23, any_flags=False))
    cases.append(Case("dsd", _golden("dsd_mode3.wv")))
    # 3 and 17 channels, longer than one tile and no multiple of it
    t3, t17 = api.planar_tile_frames(3), api.planar_tile_frames(17)
    f3, _, full3 = M.pcm_file([2, 1], 2 * t3 + 7, 16, seed=101, block_samples=512)
    cases.append(Case("3ch", f3, ALL, full3, 15))
    cases.append(Case("does_not_open", b"this is not a WavPack file, whatever its length " * 4))
    f17, _, full17 = M.pcm_file([2] * 8 + [1], 2 * t17 + 5, 24, seed=102, block_samples=128)
    cases.append(Case("17ch", f17, ALL, full17, 23))
    cor = _golden("corrupt_default.wv")
    cases.append(Case("corrupt", cor, 0, _oracle(cor, 2), 15))
    hx = S.audio_like(150, 2, 16, seed=103)
    hyb = S.encode_pcm(hx, S.EncParams(nch=2, block_samples=32, terms=S.TERMS_DEFAULT, hybrid=True,
                                       hybrid_bitrate=True, bitrate_x256=768))
    cases.append(Case("hybrid", hyb, 0, _oracle(hyb, 2), 15))
    return cases


def _planes(c):
    """uint32 (channels, frames)"""
    v = np.ascontiguousarray(c.ints.T)
    if c.kind == 0:
        return v.view(np.uint32)
    return (v.astype(np.float32) * np.float32(2.0 ** -c.kind)).view(np.uint32)


def _layout(cases, fixed):
    """[(offset, row_stride, channels, frames)] per file by the header's rules, and the total"""
    lay, off = [], 0
    for c in cases:
        if c.ints is None:
            lay.append((-1, 0, 0, 0))
            continue
        frames, nch = c.ints.shape
        rs = fixed if fixed else (frames + 3) & ~3
        lay.append((off, rs, nch, min(frames, rs)))
        off += nch * rs
    return lay, off


def _image(cases, fixed):
    lay, total = _layout(cases, fixed)
    img = np.zeros(total, dtype=np.uint32)
    for c, (off, rs, nch, fr) in zip(cases, lay):
        if off >= 0:
            img[off: off + nch * rs].reshape(nch, rs)[:, :fr] = _planes(c)[:, :fr]
    return lay, img


def _same(got, want, what):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:4].tolist(), [hex(v) for v in got[bad[:4]]],
                           [hex(v) for v in want[bad[:4]]])


def _batch(cases, kernel="auto"):
    b = api.DecodeBatch(CHUNK)
    b.set_kernel(kernel)
    for c in cases:
        i = b.add_file(c.data, c.flags)
        assert (i >= 0) == (c.ints is not None or c.name == "dsd"), c.name
    b.decode()
    return b


class Hip:
    """device buffers and a stream of the test's own, from the HIP runtime the library links"""

    def __init__(self):
        self.L = L = ctypes.CDLL(_lib.LIB_PATH)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
        L.hipMemset.argtypes = [vp, ctypes.c_int, sz]
        L.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
        L.hipFree.argtypes = [vp]
        L.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
        L.hipStreamSynchronize.argtypes = [vp]
        L.hipStreamDestroy.argtypes = [vp]
        self.bufs, self.streams = [], []

    def guarded(self, floats):
        """(pointer to the image, read()): `floats` floats of 0xFF bytes between guard floats"""
        n = GUARD + floats + GUARD
        p = ctypes.c_void_p()
        assert self.L.hipMalloc(ctypes.byref(p), 4 * n) == 0
        self.bufs.append(p)
        host = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        host[:GUARD] = GUARD_BITS
        host[GUARD + floats:] = GUARD_BITS
        assert self.L.hipMemcpy(p, host.ctypes.data, 4 * n, 1) == 0

        def read():
            assert self.L.hipMemcpy(host.ctypes.data, p, 4 * n, 2) == 0
            assert (host[:GUARD] == GUARD_BITS).all() and (host[GUARD + floats:] == GUARD_BITS).all(), "guards"
            return host[GUARD: GUARD + floats].copy()
        return ctypes.c_void_p(p.value + 4 * GUARD), read

    def stream(self):
        s = ctypes.c_void_p()
        assert self.L.hipStreamCreate(ctypes.byref(s)) == 0
        self.streams.append(s)
        return s

    def close(self):
        for s in self.streams:
            self.L.hipStreamSynchronize(s)
            self.L.hipStreamDestroy(s)
        for p in self.bufs:
            self.L.hipFree(p)


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


def test_the_decode_leaves_what_the_expectations_assume(corpus):
    """(the int32 output itself: the sources and the oracle's decodes the planes are made from)"""
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
    finally:
        b.close()


@pytest.mark.parametrize("kernel", ["auto", "lane", "two_wave"])
def test_ragged_into_the_batch_buffer(corpus, kernel):
    b = _batch(corpus, kernel)
    try:
        want_lay, want = _image(corpus, 0)
        assert b.planar_floats(0) == want.size
        assert b.device_planar_ptr() == 0  # none yet
        lay = b.planar()
        assert lay == want_lay
        assert all(off % 4 == 0 and rs % 4 == 0 for off, rs, _, _ in lay if off >= 0)
        assert b.device_planar_ptr() != 0
        _same(b.download_planar(), want, kernel)
        # the neighbours of the files that are not convertible are where they would be without them
        names = [c.name for c in corpus]
        for skip in ("dsd", "does_not_open"):
            k = names.index(skip)
            assert lay[k] == (-1, 0, 0, 0)
            assert lay[k + 1][0] == lay[k - 1][0] + lay[k - 1][1] * lay[k - 1][2]
    finally:
        b.close()


@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
def test_ragged_into_a_caller_buffer(corpus, hip, kernel):
    b = _batch(corpus, kernel)
    try:
        _, want = _image(corpus, 0)
        ptr, read = hip.guarded(want.size)
        L = b._L
        assert L.wvg_batch_planar(b._b, 0, ptr, want.size - 1, None) == _lib.WVG_ERR_SPACE
        assert L.wvg_batch_planar(b._b, 0, ptr, want.size, None) == 0
        b.sync()
        _same(read(), want, kernel)
    finally:
        b.close()


def test_fixed_frames(corpus, hip):
    """T below every length but the one-frame files', between lengths, odd, above the longest"""
    b = _batch(corpus)
    try:
        longest = max(c.ints.shape[0] for c in corpus if c.ints is not None)
        for fixed in (1, 20, 37, 100, 2 * longest + 3):
            want_lay, want = _image(corpus, fixed)
            assert b.planar_floats(fixed) == want.size
            ptr, read = hip.guarded(want.size)
            assert b._L.wvg_batch_planar(b._b, fixed, ptr, want.size, None) == 0
            assert [b.file_planar(i, fixed) for i in range(len(corpus))] == want_lay
            b.sync()
            _same(read(), want, fixed)
        # and into the batch's own buffer, which grows and shrinks with T
        for fixed in (37, 1, 100):
            b.planar(fixed)
            _same(b.download_planar(), _image(corpus, fixed)[1], fixed)
    finally:
        b.close()


def test_fixed_frames_below_the_shortest_file(corpus, hip):
    sub = [c for c in corpus if c.ints is not None and c.ints.shape[0] >= 33]
    assert {c.ints.shape[1] for c in sub} >= {1, 2, 3, 17}
    b = _batch(sub)
    try:
        fixed = 21
        lay, want = _image(sub, fixed)
        assert all(fr == fixed for _, _, _, fr in lay)
        ptr, read = hip.guarded(want.size)
        assert b._L.wvg_batch_planar(b._b, fixed, ptr, want.size, None) == 0
        b.sync()
        _same(read(), want, fixed)
    finally:
        b.close()


def test_calls_queued_back_to_back(corpus, hip):
    """several calls with other T and other destinations on one stream, nothing waited for in
    between (more values of T than the batch keeps job tables for), then every image checked"""
    b = _batch(corpus)
    try:
        s = hip.stream()
        pending = []
        for fixed in (37, 0, 100, 1, 20, 55, 0, 37):
            want = _image(corpus, fixed)[1]
            ptr, read = hip.guarded(want.size)
            assert b._L.wvg_batch_planar(b._b, fixed, ptr, want.size, s) == 0
            pending.append((fixed, read, want))
        b.planar(37, stream=s)  # and the batch's own buffer last
        b.sync()
        for fixed, read, want in pending:
            _same(read(), want, fixed)
        _same(b.download_planar(), _image(corpus, 37)[1], "own")
    finally:
        b.close()


def test_arguments_and_state(corpus):
    L = _lib.lib()
    b = api.DecodeBatch(CHUNK)
    try:
        c = corpus[4]
        b.add_file(c.data, c.flags)
        assert L.wvg_batch_planar(b._b, 0, None, 0, None) == _lib.WVG_ERR_ARG  # before an upload
        assert b.file_planar(0) == _layout([c], 0)[0][0]  # the layout is known once the file is framed
        b.decode()
        assert L.wvg_batch_planar(b._b, -1, None, 0, None) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_planar_floats(b._b, -1) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_device_planar(b._b) is None
        host = np.zeros(4, dtype=np.float32)
        assert L.wvg_batch_download_planar(b._b, host.ctypes.data, 4) == _lib.WVG_ERR_ARG  # no image yet
        b.planar()
        assert L.wvg_batch_download_planar(b._b, host.ctypes.data, 0) == _lib.WVG_ERR_SPACE
        with pytest.raises(RuntimeError):
            b.file_planar(1)
        # a refilled batch starts over
        b.reset()
        c2 = corpus[10]
        b.add_file(c2.data, c2.flags)
        b.decode()
        b.planar(7)
        _same(b.download_planar(), _image([c2], 7)[1], "refilled")
    finally:
        b.close()


# ---- torch ----

def _torch_cases(corpus):
    return [c for c in corpus if c.any_flags]


def test_decode_to_tensors_ragged(corpus):
    torch = pytest.importorskip("torch")
    cases = _torch_cases(corpus)
    dev = api.context_device()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        got = api.decode_to_tensors([c.data for c in cases], ALL | EXACT)
        # (work queued on the stream afterwards sees the tensors complete)
        sums = [None if t is None else t.abs().nan_to_num(0.0, 0.0, 0.0).sum() for t in got]
    s.synchronize()
    assert len(got) == len(cases)
    for c, t, sm in zip(cases, got, sums):
        if c.ints is None:
            assert t is None, c.name
            continue
        assert t.dtype == torch.float32 and t.is_cuda and t.device.index == dev, c.name
        assert tuple(t.shape) == c.ints.shape[::-1], c.name
        _same(t.cpu().contiguous().numpy(), _planes(c), c.name)
        assert np.isfinite(float(sm))


def test_decode_to_tensors_fixed(corpus):
    torch = pytest.importorskip("torch")
    cases = [c for c in _torch_cases(corpus) if c.ints is None or c.ints.shape[1] == 2]
    assert any(c.ints is None for c in cases) and sum(c.ints is not None for c in cases) > 10
    dev = api.context_device()
    s = torch.cuda.Stream(device=dev)
    fixed = 37
    with torch.cuda.stream(s):
        batch, lengths = api.decode_to_tensors([c.data for c in cases], ALL | EXACT, fixed_frames=fixed)
    s.synchronize()
    conv = [c for c in cases if c.ints is not None]
    assert tuple(batch.shape) == (len(conv), 2, fixed) and batch.is_contiguous() and batch.device.index == dev
    assert list(lengths) == [min(c.ints.shape[0], fixed) for c in conv]
    _same(batch.cpu().numpy().reshape(-1), _image(conv, fixed)[1], "fixed")
    with pytest.raises(ValueError):
        api.decode_to_tensors([c.data for c in _torch_cases(corpus)], ALL | EXACT, fixed_frames=fixed)
    with pytest.raises(ValueError):
        api.decode_to_tensors([cases[0].data], 0, fixed_frames=-1)


def test_planar_into_a_torch_tensor(corpus):
    torch = pytest.importorskip("torch")
    b = _batch(corpus)
    try:
        dev = api.context_device()
        _, want = _image(corpus, 0)
        out = torch.full((want.size + 3,), float("nan"), dtype=torch.float32, device=f"cuda:{dev}")
        s = torch.cuda.Stream(device=dev)
        lay = b.planar(0, out=out[3:], stream=s.cuda_stream)  # (an image 12 bytes off the allocation's alignment)
        b.sync()
        assert lay == _layout(corpus, 0)[0]
        _same(out[3:].cpu().numpy(), want, "tensor")
        assert torch.isnan(out[:3]).all()
        with pytest.raises(ValueError):
            b.planar(0, out=torch.zeros(want.size, dtype=torch.float32))  # not on the batch's device
        with pytest.raises(ValueError):
            b.planar(0, out=out[3:].double())
        with pytest.raises(ValueError):
            b.planar(0, out=out[3:][::2])
        with pytest.raises(ValueError):
            b.planar(0, out=out[: want.size - 1])
    finally:
        b.close()
