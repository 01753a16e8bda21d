"""What decoding every channel of a multichannel file costs (WVG_OPEN_ALL_CHANNELS), as
JSON lines (profiles/mc_rates.jsonl).

Workload: one 6-channel file, streams of widths 2,1,1,2, 16-bit, 1,024 block groups of
22,050 frames (C2's shape; the audio of 128 groups repeated 8 times).  Each figure is the
median of --reps runs (default 7) after one warm run, all in one process:
  a  decode + sync of the multichannel batch (the LDS tile kernel, and the plain
     strided-store kernel: WVG_MC_PLAIN=1 when the batch is made)
  b  decode + sync of the same four streams added as separate ordinary files: what the
     decode kernels alone take
  c  a hipMemcpyAsync device-to-device copy of as many bytes as the interleave reads
The interleave's time is a - b, its rate the bytes it reads over that.  The output of
both kernels is compared with the 6-channel source once.

usage: python3 scripts/mc_rates.py [--groups N] [--reps R]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WIDTHS = (2, 1, 1, 2)
BLOCK = 22050


def med(v):
    return round(float(np.median(v)), 3)


def workload(groups):
    from synth import wvsynth as S
    from tests import mc_vectors as M
    base = min(groups, 128)
    src, encs = [], []
    for k, w in enumerate(WIDTHS):
        x = np.concatenate([S.audio_like(BLOCK, w, 16, seed=0x6C00 + 131 * k + g) for g in range(base)], axis=0)
        x = np.tile(x, ((groups + base - 1) // base, 1))[: groups * BLOCK]
        src.append(x)
        encs.append(S.encode_pcm_parallel(x, S.EncParams(nch=w, terms=S.TERMS_FAST if w == 2 else [17, 17],
                                                         block_samples=BLOCK)))
    return M.mux(encs, sum(WIDTHS), 0x3F), encs, src


def timed_decodes(b, reps):
    b.upload()
    b.sync()
    ms = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        b.decode()
        b.sync()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def multichannel(f, full, reps, plain):
    from wavpackdecoder_amd import api
    os.environ["WVG_MC_PLAIN"] = "1" if plain else "0"
    b = api.DecodeBatch(4096)
    assert b.add_file(f, api.OPEN_ALL_CHANNELS) == 0
    ms = timed_decodes(b, reps)
    out = b.download()
    info = b.infos[0]
    got = out[info.out_offset: info.out_offset + info.out_frames * info.reduced_channels]
    ok = bool(np.array_equal(got.reshape(-1, info.reduced_channels), full)) and b.result(0).crc_errors == 0
    b.close()
    return ms, ok


def separate(encs, reps):
    from wavpackdecoder_amd import api
    b = api.DecodeBatch(4096)
    assert b.add_files(list(encs)) == list(range(len(encs)))
    ms = timed_decodes(b, reps)
    b.close()
    return ms


def memcpy_d2d(nbytes, reps):
    hip = ctypes.CDLL("libamdhip64.so")
    src, dst, stream = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)) == 0
    assert hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)) == 0
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    assert hip.hipMemsetAsync(src, 1, ctypes.c_size_t(nbytes), stream) == 0
    ms = []
    for r in range(reps + 1):
        assert hip.hipStreamSynchronize(stream) == 0
        t0 = time.perf_counter()
        assert hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, stream) == 0  # hipMemcpyDeviceToDevice
        assert hip.hipStreamSynchronize(stream) == 0
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    hip.hipFree(src)
    hip.hipFree(dst)
    hip.hipStreamDestroy(stream)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    f, encs, src = workload(a.groups)
    full = np.concatenate(src, axis=1)
    read_bytes = int(full.size) * 4
    b_ms = separate(encs, a.reps)
    tile_ms, tile_ok = multichannel(f, full, a.reps, plain=False)
    plain_ms, plain_ok = multichannel(f, full, a.reps, plain=True)
    c_ms = memcpy_d2d(read_bytes, a.reps)

    def rate(ms):  # GB/s of bytes read
        d = np.median(ms) - np.median(b_ms)
        return round(read_bytes / d / 1e6, 1) if d > 0 else None

    print(json.dumps({
        "what": "mc_rates", "channels": sum(WIDTHS), "widths": list(WIDTHS), "groups": a.groups, "frames": int(full.shape[0]),
        "interleave_read_bytes": read_bytes, "reps": a.reps,
        "a_multichannel_decode_sync_ms": {"tile": med(tile_ms), "plain": med(plain_ms)},
        "b_separate_files_decode_sync_ms": med(b_ms),
        "c_memcpy_d2d_ms": med(c_ms),
        "a_minus_b_ms": {"tile": round(med(tile_ms) - med(b_ms), 3), "plain": round(med(plain_ms) - med(b_ms), 3)},
        "interleave_read_GBps": {"tile": rate(tile_ms), "plain": rate(plain_ms)},
        "memcpy_d2d_GBps": round(read_bytes / np.median(c_ms) / 1e6, 1),
        "output_equals_source": {"tile": tile_ok, "plain": plain_ok},
        "runs_ms": {"a_tile": [round(v, 3) for v in tile_ms], "a_plain": [round(v, 3) for v in plain_ms],
                    "b": [round(v, 3) for v in b_ms], "c": [round(v, 3) for v in c_ms]},
    }), flush=True)


if __name__ == "__main__":
    main()
