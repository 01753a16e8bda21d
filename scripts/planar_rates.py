"""What turning a decoded batch into planar float32 costs (wvg_batch_planar), as JSON lines
(profiles/planar_rates.jsonl).

Workloads, both 22.6 M frames:
  stereo  1,024 files of one 22,050-frame 16-bit stereo block (C2's shape; 128 distinct
          files, each added 8 times)
  six     64 copies of one 6-channel file (streams of widths 2,1,1,2, 16 block groups of
          22,050 frames), opened with WVG_OPEN_ALL_CHANNELS
Each figure is the median of --reps runs (default 9) after one warm run, all in one process:
  planar      wvg_batch_planar on the batch's stream between two events (ragged rows into
              the batch's buffer, and fixed rows of 22,050 / 22,051 frames: 16-byte aligned
              and odd; the six-channel files are cut to them), over the bytes it reads
              (4 a value inside the rows) plus writes (4 a float of the image)
  memcpy_d2d  a hipMemcpyAsync device-to-device copy of 4 bytes a value between the same
              events: the same bytes read plus written
  interleave  six only: wv_mc_interleave as scripts/mc_rates.py measures it, decode + sync
              of the 6-channel batch minus decode + sync of the same streams as separate
              files, over the bytes it reads plus writes
The planar image of the first and the last file is compared with numpy over the
downloaded ints once.

usage: python3 scripts/planar_rates.py [--reps R] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BLOCK = 22050
WIDTHS = (2, 1, 1, 2)


def med(v):
    return round(float(np.median(v)), 4)


class Events:
    """an event pair on a stream, from the HIP runtime the library links"""

    def __init__(self, L):
        self.L = L
        vp = ctypes.c_void_p
        L.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
        L.hipEventRecord.argtypes = [vp, vp]
        L.hipEventSynchronize.argtypes = [vp]
        L.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
        self.a, self.b = vp(), vp()
        assert L.hipEventCreate(ctypes.byref(self.a)) == 0 and L.hipEventCreate(ctypes.byref(self.b)) == 0

    def time(self, stream, fn):
        assert self.L.hipEventRecord(self.a, stream) == 0
        fn()
        assert self.L.hipEventRecord(self.b, stream) == 0
        assert self.L.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.L.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def stereo_files():
    from synth import wvsynth as S
    base = [S.encode_pcm(S.audio_like(BLOCK, 2, 16, seed=0xC2 + k),
                         S.EncParams(terms=S.TERMS_FAST, block_samples=BLOCK)) for k in range(128)]
    return base * 8


def six_files():
    from synth import wvsynth as S
    from tests import mc_vectors as M
    encs = [S.encode_pcm_parallel(S.audio_like(16 * BLOCK, w, 16, seed=0x6C00 + 131 * k),
                                  S.EncParams(nch=w, terms=S.TERMS_FAST if w == 2 else [17, 17], block_samples=BLOCK))
            for k, w in enumerate(WIDTHS)]
    return [M.mux(encs, sum(WIDTHS), 0x3F)] * 64, encs * 64


def check_file(b, out, img, lay, i):
    info = b.infos[i]
    off, rs, ch, fr = lay[i]
    v = out[info.out_offset: info.out_offset + info.out_frames * ch].reshape(-1, ch)[:fr].T
    k = 8 * info.bytes_per_sample - 1
    want = v.astype(np.float32) * np.float32(2.0 ** -k)
    got = img[off: off + ch * rs].reshape(ch, rs)
    return bool(np.array_equal(got[:, :fr].view(np.uint32), want.view(np.uint32)) and not got[:, fr:].any())


def planar_rates(name, files, flags, reps):
    from wavpackdecoder_amd import _lib, api
    b = api.DecodeBatch(4096)
    idx = b.add_files(files, flags)
    assert min(idx) >= 0
    b.decode()
    b.sync()
    values = sum(i.out_frames * i.reduced_channels for i in b.infos)
    L = ctypes.CDLL(_lib.LIB_PATH)
    ev = Events(L)
    stream = ctypes.c_void_p(b._L.wvg_batch_stream(b._b))
    res = {"what": "planar_rates", "workload": name, "files": len(files), "channels": int(b.infos[0].reduced_channels),
           "values": int(values), "bytes_read_plus_written": int(values) * 8, "reps": reps}
    lay = b.planar(0)
    img = b.download_planar()
    out = b.download()
    res["output_equals_numpy"] = check_file(b, out, img, lay, 0) and check_file(b, out, img, lay, len(files) - 1)
    del img
    for label, fixed in (("ragged", 0), ("fixed_22050", BLOCK), ("fixed_22051", BLOCK + 1)):
        floats = b.planar_floats(fixed)
        run = lambda: b._check(b._L.wvg_batch_planar(b._b, fixed, None, 0, None))  # noqa: E731
        ms = [ev.time(stream, run) for _ in range(reps + 1)][1:]
        # what the kernel moves: the frames inside the rows read, every float of the image written
        read = sum(min(i.out_frames, fixed or i.out_frames) * i.reduced_channels for i in b.infos)
        moved = int(read) * 4 + int(floats) * 4
        res[label] = {"ms": med(ms), "GBps": round(moved / np.median(ms) / 1e6, 1), "image_floats": int(floats),
                      "bytes_read_plus_written": moved, "runs_ms": [round(v, 4) for v in ms]}
    # the same bytes through the copy engine's front door: device to device, 4 bytes a value
    nbytes = int(values) * 4
    src, dst = ctypes.c_void_p(), ctypes.c_void_p()
    L.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.hipFree.argtypes = [ctypes.c_void_p]
    assert L.hipMalloc(ctypes.byref(src), nbytes) == 0 and L.hipMalloc(ctypes.byref(dst), nbytes) == 0
    assert L.hipMemsetAsync(src, 1, nbytes, stream) == 0
    ms = [ev.time(stream, lambda: L.hipMemcpyAsync(dst, src, nbytes, 3, stream)) for _ in range(reps + 1)][1:]
    res["memcpy_d2d"] = {"ms": med(ms), "GBps": round(2 * nbytes / np.median(ms) / 1e6, 1),
                         "runs_ms": [round(v, 4) for v in ms]}
    b.sync()
    L.hipFree(src)
    L.hipFree(dst)
    b.close()
    return res


def decode_sync_ms(files, flags, reps):
    from wavpackdecoder_amd import api
    b = api.DecodeBatch(4096)
    assert min(b.add_files(files, flags)) >= 0
    b.upload()
    b.sync()
    ms = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        b.decode()
        b.sync()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    b.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wavpackdecoder_amd import api
    lines = [planar_rates("stereo", stereo_files(), 0, a.reps)]
    six, streams = six_files()
    r = planar_rates("six", six, api.OPEN_ALL_CHANNELS, a.reps)
    a_ms = decode_sync_ms(six, api.OPEN_ALL_CHANNELS, a.reps)
    b_ms = decode_sync_ms(streams, 0, a.reps)
    d = float(np.median(a_ms) - np.median(b_ms))
    r["interleave"] = {"a_multichannel_decode_sync_ms": med(a_ms), "b_separate_files_decode_sync_ms": med(b_ms),
                       "a_minus_b_ms": round(d, 4),
                       "GBps": round(r["bytes_read_plus_written"] / d / 1e6, 1) if d > 0 else None}
    lines.append(r)
    text = "".join(json.dumps(x) + "\n" for x in lines)
    sys.stdout.write(text)
    sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
