"""The stored MD5 sum (ID_MD5_CHECKSUM), host side: the MD5 core the kernel runs
(wv_md5.h through wvg_md5_bytes) against hashlib, the framing's search for the
stored sum (wvg_probe_file_md5: the last audio block, a trailing zero-sample
block, the last of several, only 16-byte payloads), and that carrying a sum
changes nothing else of what the framing and the oracle report.

The expected digests come from hashlib, never from project code.  GPU side:
test_gpu_md5.py.
"""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from synth import wvsynth as S
from wavpackdecoder_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "wavpackdecoder_amd")])
    return _lib.lib()


def _md5(L, data: bytes) -> bytes:
    out = (ctypes.c_uint8 * 16)()
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
    assert L.wvg_md5_bytes(buf.ctypes.data, len(data), out) == 0
    return bytes(out)


def test_md5_names_in_header_binding_and_library(L):
    """the four entry points are declared, bound and exported (test_abi.py's header scan
    skips names with a digit)"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wvgpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wvg_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = set(re.findall(r" T (wvg_[a-z0-9_]+)$", out, flags=re.M))
    assert declared == set(_lib.EXPORTED) | set(_lib.EXPORTED_MD5)
    for name in _lib.EXPORTED_MD5:
        assert name in syms and getattr(L, name).argtypes is not None
    assert ctypes.sizeof(_lib.WvgFileMd5) == 48


def test_md5_bytes_every_length_to_200(L):
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, size=200, dtype=np.uint8).tobytes()
    for n in range(201):
        assert _md5(L, data[:n]) == hashlib.md5(data[:n]).digest(), n


def test_md5_bytes_one_mib(L):
    data = np.random.default_rng(2).integers(0, 256, size=1 << 20, dtype=np.uint8).tobytes()
    assert _md5(L, data) == hashlib.md5(data).digest()


RFC1321 = [
    (b"", "d41d8cd98f00b204e9800998ecf8427e"),
    (b"a", "0cc175b9c0f1b6a831c399e269772661"),
    (b"abc", "900150983cd24fb0d6963f7d28e17f72"),
    (b"message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
    (b"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
    (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"),
    (b"1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a"),
]


@pytest.mark.parametrize("msg,hexd", RFC1321, ids=[str(i) for i in range(7)])
def test_md5_bytes_rfc1321(L, msg, hexd):
    assert _md5(L, msg).hex() == hexd


# ---- the stored sum ---------------------------------------------------------
X = S.audio_like(300, 2, 16, seed=11)
SUM_A = S.source_md5(X, 2)
SUM_B = bytes(range(16))
SUM_C = bytes(range(100, 116))


def _enc(write_md5, md5=SUM_A, **kw):
    return S.encode_pcm(X, S.EncParams(terms=S.TERMS_FAST, block_samples=128, write_md5=write_md5, md5=md5, **kw))


def test_source_md5_is_hashlib_over_the_source_bytes():
    assert SUM_A == hashlib.md5(X.astype("<i2").tobytes()).digest()
    x8 = np.array([-128, -1, 0, 127], dtype=np.int32)
    assert S.source_md5(x8, 1) == hashlib.md5(bytes([0, 127, 128, 255])).digest()
    x24 = np.array([-2, 0x123456], dtype=np.int32)
    assert S.source_md5(x24, 3) == hashlib.md5(bytes([0xFE, 0xFF, 0xFF, 0x56, 0x34, 0x12])).digest()
    d = np.array([0, 200, 255], dtype=np.uint8)
    assert S.source_md5(d, 1, dsd=True) == hashlib.md5(bytes([0, 200, 255])).digest()


def test_probe_md5_in_last_audio_block(L):
    assert api.probe_md5(_enc(1)) == SUM_A


def test_probe_md5_in_trailing_block(L):
    f0, f2 = _enc(0), _enc(2)
    assert f2[: len(f0)] == f0 and len(f2) == len(f0) + 32 + 18  # a zero-sample block after the audio
    assert int.from_bytes(f2[len(f0) + 20: len(f0) + 24], "little") == 0
    assert api.probe_md5(f2) == SUM_A


def test_probe_md5_none(L):
    assert api.probe_md5(_enc(0)) is None
    out = (ctypes.c_uint8 * 16)()
    assert L.wvg_probe_file_md5(b"not a wavpack file", 18, out) == _lib.WVG_ERR_OPEN
    with pytest.raises(ValueError):
        api.probe_md5(b"")


def test_probe_md5_last_one_wins(L):
    f0 = _enc(0)
    tail_b = _enc(2, SUM_B)[len(f0):]
    tail_c = _enc(2, SUM_C)[len(f0):]
    assert api.probe_md5(_enc(1, SUM_A) + tail_b) == SUM_B       # audio block, then a trailing block
    assert api.probe_md5(f0 + tail_b + tail_c) == SUM_C          # two trailing blocks
    assert api.probe_md5(f0 + tail_c + tail_b) == SUM_B
    # a DSD file: the reference's unpack_init rejects a zero-sample block there and its
    # walk stops at the first one; the tail walk still reaches the second
    d = S.dsd_random_like(200, 1, seed=6)
    enc = lambda w, m: S.encode_dsd(d, S.DsdParams(nch=1, mode=0, block_samples=128, write_md5=w, md5=m))
    g0 = enc(0, b"")
    assert api.probe_md5(g0 + enc(2, SUM_B)[len(g0):] + enc(2, SUM_C)[len(g0):]) == SUM_C


def test_probe_md5_ignores_a_15_byte_sub_block(L):
    f0 = _enc(0)
    tail = bytearray(_enc(2, SUM_B)[len(f0):])
    assert tail[32] == 0x26 and tail[33] == 8
    tail[32] |= 0x40  # ID_ODD_SIZE: 15 bytes and a pad byte
    assert api.probe_md5(f0 + bytes(tail)) is None
    assert api.probe_md5(_enc(1, SUM_A) + bytes(tail)) == SUM_A  # and it does not hide an earlier sum


def test_probe_md5_junk_after_the_last_block_ends_the_walk(L):
    assert api.probe_md5(_enc(0) + b"junk" * 20) is None
    assert api.probe_md5(_enc(2) + b"junk" * 20) == SUM_A


INFO_FIELDS = [n for n, _ in _lib.WvgFileInfo._fields_]


def _probe(L, data, flags=0):
    info = _lib.WvgFileInfo()
    rc = L.wvg_probe_file(data, len(data), flags, 4096, ctypes.byref(info))
    return rc, {n: (bytes(getattr(info, n)) if n == "error" else getattr(info, n)) for n in INFO_FIELDS}


def _variants():
    """(name, the same audio encoded with write_md5 0, 1 and 2)"""
    out = []
    for name, kw in (("plain", {}), ("riff", {"write_riff": True}), ("unknown_total", {"total_unknown": True})):
        out.append((name, [_enc(w, **kw) for w in (0, 1, 2)]))
    d = S.dsd_random_like(300, 2, seed=5)
    for mode in (0, 1, 3):
        out.append((f"dsd{mode}", [S.encode_dsd(d, S.DsdParams(mode=mode, block_samples=128, write_md5=w,
                                                                md5=S.source_md5(d, 1, dsd=True)))
                                   for w in (0, 1, 2)]))
    return out


VARIANTS = _variants()


@pytest.mark.parametrize("name,files", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_a_stored_sum_changes_nothing_else(L, name, files):
    """wvg_probe_file's info (the header / trailer offsets included: the sum is written
    after them) and the oracle's decode are the same with and without the sum"""
    base_rc, base = _probe(L, files[0])
    ref = O.decode_file(files[0])
    assert base_rc == 0
    for f in files[1:]:
        rc, info = _probe(L, f)
        assert rc == base_rc and info == base, name
        r = O.decode_file(f)
        assert r.crc_errors == ref.crc_errors == 0 and r.frames == ref.frames
        np.testing.assert_array_equal(r.samples, ref.samples)


def test_md5_off_leaves_the_encoder_output_unchanged():
    """write_md5 = 1 inserts exactly the 18-byte sub-block at the end of the last block"""
    f0, f1 = _enc(0), _enc(1)
    assert len(f1) == len(f0) + 18 and f1[-18:] == bytes([0x26, 8]) + SUM_A
