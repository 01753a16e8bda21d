"""Multichannel test files: streams encoded on their own with the repo encoder and muxed
block by block into WavPack's multichannel layout (one group INITIAL_BLOCK .. FINAL_BLOCK
per time slice, one mono or stereo block per stream, ID_CHANNEL_INFO in the first block
of every group).  The expected values are the sources themselves (lossless streams) or
the oracle's decode of the stand-alone stream, so none comes from the code under test."""
import ctypes

import numpy as np

from oracle import oracle as O
from synth import wvsynth as S

INITIAL_BLOCK, FINAL_BLOCK = 0x800, 0x1000
OPEN_2CH_MAX = 0x8


def split_blocks(data: bytes):
    """the blocks of a stand-alone stream, headers back to back"""
    out, i = [], 0
    while i + 32 <= len(data):
        assert data[i:i + 4] == b"wvpk"
        n = 8 + int.from_bytes(data[i + 4:i + 8], "little")
        out.append(bytearray(data[i:i + n]))
        i += n
    assert i == len(data)
    return out


def _samples(blk) -> int:
    return int.from_bytes(blk[20:24], "little")


def mux(streams, nch: int, mask: int = 0, rotate: int = 0) -> bytes:
    """streams: stand-alone .wv files with the same block_samples and frame count; their
    blocks woven into groups.  rotate: stream `rotate` first (the mux then holds the same
    blocks in another stream order).  Zero-sample blocks after the audio (a stored MD5)
    follow the last group as they are."""
    lists = [split_blocks(s) for s in streams]
    lists = lists[rotate:] + lists[:rotate]
    audio = [[b for b in l if _samples(b)] for l in lists]
    tails = [b for l in lists for b in l if not _samples(b)]
    ngroups = len(audio[0])
    assert all(len(a) == ngroups for a in audio)
    out = bytearray()
    for g in range(ngroups):
        for s, a in enumerate(audio):
            b = bytearray(a[g])
            fl = int.from_bytes(b[24:28], "little") & ~(INITIAL_BLOCK | FINAL_BLOCK)
            if s == 0:
                fl |= INITIAL_BLOCK
                b[32:32] = bytes([0x0D, 0x01, nch & 0xFF, mask & 0xFF])
                b[4:8] = (int.from_bytes(b[4:8], "little") + 4).to_bytes(4, "little")
            if s == len(audio) - 1:
                fl |= FINAL_BLOCK
            b[24:28] = fl.to_bytes(4, "little")
            out += b
    for b in tails:
        out += b
    return bytes(out)


def oracle_open(data: bytes, flags: int = OPEN_2CH_MAX, chunk: int = 4096):
    """the reference's call loop under `flags` -> (samples (frames, nch), crc errors), or
    None when the file does not open"""
    L = O.lib()
    ctx = L.wvo_open(data, len(data), flags)
    if not ctx:
        return None
    try:
        if L.wvo_get_error_message(ctx):  # (empty: the file opened)
            return None
        nch = max(L.wvo_get_reduced_channels(ctx), 1)
        buf = np.zeros(chunk * nch, dtype=np.int32)
        parts = []
        for _ in range(1 << 20):
            n = L.wvo_unpack_samples(ctx, buf.ctypes.data, buf.size, chunk)
            if n <= 0:
                break
            parts.append(buf[: n * nch].copy())
        x = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        return x.reshape(-1, nch), int(L.wvo_get_num_errors(ctx))
    finally:
        L.wvo_close(ctx)


def pcm_sources(widths, frames: int, bits: int = 16, seed: int = 0):
    return [S.audio_like(frames, w, bits, seed=seed + 11 * k) for k, w in enumerate(widths)]


def pcm_file(widths, frames: int, bits: int = 16, seed: int = 0, block_samples: int = 32, mask: int = 0,
             md5: bool = False, **kw):
    """(file, sources, the N-channel source) for a lossless PCM layout"""
    bps = (bits + 7) // 8
    src = pcm_sources(widths, frames, bits if bits < 32 else 24, seed)
    if bits == 32:
        src = [(x.astype(np.int64) << 8).astype(np.int32) for x in src]
        kw.setdefault("int32_zeros", 8)
    full = np.concatenate(src, axis=1)
    encs = []
    for k, (w, x) in enumerate(zip(widths, src)):
        p = S.EncParams(nch=w, bytes_per_sample=bps, block_samples=block_samples,
                        terms=S.TERMS_DEFAULT if w == 2 else [18, 2, 17], **kw)
        if md5 and k == len(widths) - 1:
            p.write_md5 = md5 if isinstance(md5, int) and not isinstance(md5, bool) else 1
            p.md5 = S.source_md5(full, bps)
        encs.append(S.encode_pcm(x, p))
    return mux(encs, sum(widths), mask), src, full


def dsd_file(widths, frames: int, mode: int, seed: int = 0, block_samples: int = 32):
    src = [S.dsd_random_like(frames, w, seed=seed + 7 * k) for k, w in enumerate(widths)]
    encs = [S.encode_dsd(x, S.DsdParams(nch=w, mode=mode, block_samples=block_samples)) for w, x in zip(widths, src)]
    return mux(encs, sum(widths), 0), src, np.concatenate(src, axis=1).astype(np.int32)


def self_check(encs, widths, chunk: int = 50):
    """For every k: the mux with stream k first, under OPEN_2CH_MAX, is the oracle's decode
    of the stand-alone stream k with no CRC error.  Returns the stand-alone decodes."""
    alone = []
    for k, e in enumerate(encs):
        a, errs = oracle_open(e, 0, chunk)
        assert errs == 0
        m, merrs = oracle_open(mux(encs, sum(widths), 0, rotate=k), OPEN_2CH_MAX, chunk)
        assert merrs == 0, (k, merrs)
        assert m.shape == a.shape and np.array_equal(m, a), k
        alone.append(a)
    return alone
