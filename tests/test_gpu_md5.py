"""GPU: the files' MD5 sums computed on the device (wvg_batch_md5, wv_md5.hip) against
the sum stored in the file (ID_MD5_CHECKSUM).

The expected digest is always hashlib's MD5 of the *source array* in its native byte
form (little-endian at the file's bytes per sample, one-byte PCM unsigned, DSD raw,
float32 bit patterns) -- independent of the oracle, of the encoder's bitstream and of
the kernels.  Files are tiny (block_samples 32, so they span blocks); their lengths sit
on the kernel's seams: the 55/56-byte padding boundary, the 64-byte block, the 64-value
super-step (64, 128, 192, 256 bytes) at every sample width.  Host side: test_md5_host.py.
"""
import ctypes
import hashlib

import numpy as np
import pytest

from synth import wvsynth as S
from wavpackdecoder_amd import _lib
from wavpackdecoder_amd.api import (MD5_MATCH, MD5_MISMATCH, MD5_NONE, MD5_NOT_COMPARABLE, OPEN_EXACT_FLOAT,
                                    verify_files)

pytestmark = pytest.mark.gpu

B = 32  # block_samples


def _h(x, bps, dsd=False):
    """hashlib over the source array's bytes"""
    if dsd:
        return hashlib.md5(np.ascontiguousarray(x, dtype=np.uint8).tobytes()).digest()
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)
    if bps == 1:
        return hashlib.md5(((x + 128) & 0xFF).astype(np.uint8).tobytes()).digest()
    return hashlib.md5(np.ascontiguousarray(x.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :bps]).tobytes()).digest()


class Case:
    def __init__(self, name, data, digest, verdict, wvc=None, flags=0, start=None, dsd=False, nbytes=None):
        self.name, self.data, self.digest, self.verdict = name, data, digest, verdict
        self.wvc, self.flags, self.start, self.dsd, self.nbytes = wvc, flags, start, dsd, nbytes


def _pcm(name, frames, nch, bps, seed, write_md5=1, verdict=MD5_MATCH, **kw):
    bits = 8 * bps if bps < 4 else 24
    x = S.audio_like(frames, nch, bits, seed=seed)
    if bps == 4:  # 32-bit integers: 24-bit audio with 8 zero bits below it (INT32_DATA, lossless)
        x = (x.astype(np.int64) << 8).astype(np.int32)
        kw.setdefault("int32_zeros", 8)
    terms = kw.pop("terms", S.TERMS_MONO_HIGH if nch == 1 else S.TERMS_DEFAULT)
    p = S.EncParams(nch=nch, bytes_per_sample=bps, terms=terms, block_samples=B, write_md5=write_md5,
                    md5=S.source_md5(x, bps) if write_md5 else b"", **kw)
    return Case(name, S.encode_pcm(x, p), _h(x, bps), verdict if write_md5 else MD5_NONE, nbytes=x.size * bps)


def seam_cases():
    out = []
    for f in (1, 55, 56, 57, 63, 64, 65, 119, 120, 128, 129):
        out.append(_pcm(f"m8_{f}", f, 1, 1, 100 + f))
    for f in (13, 14, 16, 17, 31, 32, 33):
        out.append(_pcm(f"s16_{f}", f, 2, 2, 200 + f))
    for f in (18, 19, 21, 22, 63, 64, 65, 85, 86):
        out.append(_pcm(f"m24_{f}", f, 1, 3, 300 + f))
    for f in (19, 21, 22, 64):
        out.append(_pcm(f"s24_{f}", f, 2, 3, 400 + f))
    for f in (13, 14, 15, 16, 17, 63, 64, 65):
        out.append(_pcm(f"m32_{f}", f, 1, 4, 500 + f))
    # more than one wave, lengths unlike their neighbours': the length sort must return
    # each digest to its own file; every other one carries the sum in a trailing block
    for k in range(30):
        out.append(_pcm(f"fill_{k}", 700 - 23 * k, 2, 2, 600 + k, write_md5=1 + (k & 1)))
    return out


def _flip(data, off, mask=0x10):
    b = bytearray(data)
    b[off] ^= mask
    return bytes(b)


def _bitstream_mid(wv):
    """an offset in the middle of the first block's ID_WV_BITSTREAM payload"""
    end, p = 8 + int.from_bytes(wv[4:8], "little"), 32
    while p + 2 <= end:
        i, bl, hl = wv[p], wv[p + 1] * 2, 2
        if i & 0x80:
            bl += (wv[p + 2] << 9) + (wv[p + 3] << 17)
            hl = 4
        if (i & 0x3F) == 0x0A:
            return p + hl + bl // 2
        p += hl + bl
    raise AssertionError("no bitstream")


def verdict_cases():
    out = []
    good = _pcm("intact", 200, 2, 2, 701)
    out.append(good)
    at = good.data.rfind(bytes([0x26, 8]) + good.digest)
    assert at > 0
    out.append(Case("stored_flipped", _flip(good.data, at + 2 + 5), good.digest, MD5_MISMATCH))
    out.append(Case("payload_flipped", _flip(good.data, _bitstream_mid(good.data)), None, MD5_MISMATCH))
    out.append(_pcm("no_sum", 200, 2, 2, 702, write_md5=0))
    out.append(_pcm("trailing_block", 200, 2, 2, 703, write_md5=2))
    out.append(_pcm("int32_wvx", 100, 2, 4, 704, int32_zeros=0, int32_sent_bits=8, wvx=1))
    out.append(_pcm("int32_lossy", 100, 2, 4, 705, int32_zeros=0, int32_sent_bits=8, verdict=MD5_NOT_COMPARABLE))
    sk = _pcm("seek", 200, 2, 2, 706, verdict=MD5_NOT_COMPARABLE)
    sk.start = 40
    sk.digest = None
    sk.nbytes = (200 - 40) * 2 * 2  # the frames from the seek target on
    out.append(sk)
    # hybrid: lossy alone, exact with its .wvc
    x = S.audio_like(300, 2, 16, seed=707)
    wv, wvc = S.encode_pcm_wvc(x, S.EncParams(terms=S.TERMS_FAST, block_samples=B, hybrid_bitrate=True,
                                              bitrate_x256=768, write_md5=1, md5=S.source_md5(x, 2)))
    out.append(Case("hybrid_alone", wv, None, MD5_NOT_COMPARABLE))
    out.append(Case("hybrid_wvc", wv, _h(x, 2), MD5_MATCH, wvc=wvc))
    # float: the reference's 24-bit integers are not the source; the exact output is
    rng = np.random.default_rng(708)
    fx = (S.audio_like(300, 2, 16, seed=708).astype(np.float32) / 32768.0 + rng.normal(0, 1e-6, (300, 2))).astype(
        np.float32)
    bits = fx.view(np.int32)
    fwv = S.encode_float_exact(fx, S.EncParams(terms=S.TERMS_FAST, block_samples=B, write_md5=2,
                                               md5=S.source_md5(bits, 4)))
    out.append(Case("float_plain", fwv, None, MD5_NOT_COMPARABLE))
    out.append(Case("float_exact", fwv, hashlib.md5(fx.astype("<f4").tobytes()).digest(), MD5_MATCH,
                    flags=OPEN_EXACT_FLOAT))
    for mode in (0, 1, 3):
        for nch in (1, 2):
            d = S.dsd_random_like(150 + 7 * mode + nch, nch, seed=710 + 2 * mode + nch, density=0.3)
            f = S.encode_dsd(d, S.DsdParams(nch=nch, mode=mode, block_samples=B, write_md5=1 + (nch & 1),
                                            md5=S.source_md5(d, 1, dsd=True)))
            out.append(Case(f"dsd{mode}_ch{nch}", f, _h(d, 1, dsd=True), MD5_MATCH, dsd=True, nbytes=d.size))
    return out


SEAMS = seam_cases()
VERDICTS = verdict_cases()


def _add(b, c):
    i = b.add_file(c.data, open_flags=c.flags, start_sample=c.start, wvc=c.wvc)
    assert i >= 0, c.name
    return i


def _check(b, i, c):
    r = b.file_md5(i)
    assert r.verdict == c.verdict, (c.name, r.verdict)
    if c.digest is not None:
        assert bytes(r.computed) == c.digest, c.name
    if c.nbytes is not None:
        assert r.bytes == c.nbytes, c.name
    assert r.has_stored == (c.verdict != MD5_NONE), c.name
    return r


@pytest.fixture(scope="module")
def mixed(gpu_batch_cls):
    """SEAMS + VERDICTS in one batch (unequal trip counts share a wave; more than one
    wave), decoded and hashed once: never formatted, no PCM downloaded"""
    b = gpu_batch_cls(4096)
    cases = SEAMS + VERDICTS
    idx = [_add(b, c) for c in cases]
    assert len(idx) > 64
    b.upload()
    r = _lib.WvgFileMd5()
    assert b._L.wvg_batch_file_md5(b._b, 0, ctypes.byref(r)) == _lib.WVG_ERR_ARG  # no md5 issued yet
    b.decode()
    b.md5()
    b.sync()
    yield b, dict(zip([c.name for c in cases], idx))
    b.close()


@pytest.mark.parametrize("c", SEAMS, ids=[c.name for c in SEAMS])
def test_gpu_md5_padding_and_super_step_seams(mixed, c):
    b, idx = mixed
    _check(b, idx[c.name], c)


@pytest.mark.parametrize("c", VERDICTS, ids=[c.name for c in VERDICTS])
def test_gpu_md5_verdicts(mixed, c):
    b, idx = mixed
    r = _check(b, idx[c.name], c)
    if c.name == "stored_flipped":
        assert bytes(r.stored) != c.digest
    if c.name == "payload_flipped":
        good = next(v for v in VERDICTS if v.name == "intact")
        assert bytes(r.computed) != good.digest and bytes(r.stored) == good.digest


def test_gpu_md5_file_that_did_not_open(gpu_batch_cls):
    b = gpu_batch_cls(4096)
    assert b.add_file(b"no wavpack in here") == _lib.WVG_ERR_OPEN
    i = _add(b, VERDICTS[0])
    b.decode()
    b.md5()
    b.sync()
    r = _lib.WvgFileMd5()
    assert b._L.wvg_batch_file_md5(b._b, 0, ctypes.byref(r)) == _lib.WVG_ERR_OPEN
    _check(b, i, VERDICTS[0])
    b.close()


def test_gpu_md5_device_framed(gpu_batch_cls):
    """files framed on the device keep their sum (DBlock.md5_off) and stay device-framed;
    one with a trailing zero-sample block goes to the host framer and is found there"""
    in_block = [c for c in SEAMS if c.verdict == MD5_MATCH and not c.name.startswith("fill_")][:20]
    in_block += [c for c in SEAMS if c.name.startswith("fill_")][0::2]
    trailing = next(c for c in VERDICTS if c.name == "trailing_block")
    cases = in_block + [trailing]
    b = gpu_batch_cls(4096)
    idx = b.add_files_device([c.data for c in cases])
    b.decode()
    b.md5()
    b.sync()
    assert b.framing_stats() == (len(in_block), 1)
    for i, c in zip(idx, cases):
        _check(b, i, c)
    b.close()


def test_gpu_md5_hashes_what_this_decode_wrote(gpu_batch_cls):
    first, second = SEAMS[5:25], SEAMS[30:44]
    b = gpu_batch_cls(4096)
    idx = [_add(b, c) for c in first]
    b.poison(0x5A)
    b.decode()
    b.md5()
    b.sync()
    for i, c in zip(idx, first):
        _check(b, i, c)
    b.reset()
    idx = [_add(b, c) for c in second]
    b.upload()
    r = _lib.WvgFileMd5()
    assert b._L.wvg_batch_file_md5(b._b, 0, ctypes.byref(r)) == _lib.WVG_ERR_ARG  # none since this upload
    b.decode()
    b.md5()
    b.sync()
    for i, c in zip(idx, second):
        _check(b, i, c)
    b.close()


def test_gpu_md5_equals_md5_of_the_formatted_pcm(gpu_batch_cls):
    """a second batch that is formatted and downloaded: hashlib over each file's slice of
    the host PCM image is the device digest (DSD files from the dsd=True image)"""
    cases = [c for c in SEAMS + VERDICTS if c.nbytes is not None][::3] + [c for c in VERDICTS if c.dsd]
    b = gpu_batch_cls(4096)
    idx = [_add(b, c) for c in cases]
    b.decode()
    b.md5()
    b.format(dsd=False)
    pcm = b.download_pcm().copy()
    b.format(dsd=True)
    pcm_dsd = b.download_pcm().copy()
    for i, c in zip(idx, cases):
        r = _check(b, i, c)
        o = b.pcm_offset(i)
        img = pcm_dsd if c.dsd else pcm
        assert hashlib.md5(img[o:o + r.bytes].tobytes()).digest() == bytes(r.computed), c.name
    b.close()


def test_gpu_md5_ordered_after_concurrent_lane_decodes(gpu_batch_cls):
    """four batches decode at once on their own streams under WVG_KERNEL_LANE, each followed
    by its md5 with no sync in between: the kernel waits for the whole decode"""
    sets = []
    for k in range(4):
        cs = [_pcm(f"o{k}_{j}", 1500 + 97 * j + 13 * k, 2, 2 + (j & 1), 900 + 10 * k + j, write_md5=1 + (j & 1),
                   terms=S.TERMS_FAST) for j in range(8)]
        sets.append(cs)
    batches = []
    for cs in sets:
        b = gpu_batch_cls(4096)
        b.set_kernel("lane")
        idx = [_add(b, c) for c in cs]
        b.upload()
        batches.append((b, idx))
    for b, _ in batches:
        b.decode()
        b.md5()
    for b, _ in batches:
        b.sync()
    for (b, idx), cs in zip(batches, sets):
        for i, c in zip(idx, cs):
            _check(b, i, c)
        b.close()


def test_gpu_verify_files():
    cases = [c for c in SEAMS[:12] + VERDICTS if c.wvc is None and not c.flags and c.start is None]
    res = verify_files([c.data for c in cases] + [b"junk"])
    assert res[-1] is None
    for r, c in zip(res, cases):
        assert r.verdict == c.verdict, c.name
        if c.digest is not None:
            assert bytes(r.computed) == c.digest, c.name
