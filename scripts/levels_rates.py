"""What the level statistics of a decoded batch cost (wvg_batch_levels), as JSON lines
(profiles/levels_rates.jsonl).

Workloads, both 22.6 M frames (scripts/planar_rates.py's):
  stereo  1,024 files of one 22,050-frame 16-bit stereo block (C2's shape; 128 distinct
          files, each added 8 times)
  six     64 copies of one 6-channel file (streams of widths 2,1,1,2, 16 block groups of
          22,050 frames), opened with WVG_OPEN_ALL_CHANNELS
Each figure is the median of --reps runs (default 9) after one warm run, between two
events on the batch's stream, all in one process:
  levels      wvg_batch_levels: wv_levels_tiles, wv_levels_combine and the download of the
              records, over the bytes of the ints it reads (4 a value)
  planar      wvg_batch_planar, ragged rows into the batch's buffer, on the same batch: it
              reads the same ints and writes as many bytes again.  The levels call has no
              reason to take longer: `levels_vs_planar` is levels / planar, and
              `within_planar` says whether it is at most 1.03 (the run-to-run spread of
              one box)
  memcpy_d2d  a hipMemcpyAsync device-to-device copy of the same ints
The records of the first and the last file are compared with Python integers over the
generator's arrays once.

usage: python3 scripts/levels_rates.py [--reps R] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BLOCK = 22050
WIDTHS = (2, 1, 1, 2)
Q = 1 << 20


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


def stereo_sources():
    from synth import wvsynth as S
    return [S.audio_like(BLOCK, 2, 16, seed=0xC2 + k) for k in range(128)]


def stereo_files(src):
    from synth import wvsynth as S
    base = [S.encode_pcm(x, S.EncParams(terms=S.TERMS_FAST, block_samples=BLOCK)) for x in src]
    return base * 8


def six_sources():
    from synth import wvsynth as S
    return [S.audio_like(16 * BLOCK, w, 16, seed=0x6C00 + 131 * k) for k, w in enumerate(WIDTHS)]


def six_files(src):
    from synth import wvsynth as S
    from tests import mc_vectors as M
    encs = [S.encode_pcm_parallel(x, S.EncParams(nch=w, terms=S.TERMS_FAST if w == 2 else [17, 17],
                                                 block_samples=BLOCK)) for x, w in zip(src, WIDTHS)]
    return [M.mux(encs, sum(WIDTHS), 0x3F)] * 64


def check_file(b, i, want):
    """file i's records against Python integers over its source array (levels_vectors.expected)"""
    from tests.levels_vectors import FIELDS
    got = b.file_levels(i)
    return got is not None and len(got) == len(want) and all(
        int(g[f]) == w[f] for g, w in zip(got, want) for f in FIELDS)


def levels_rates(name, files, flags, first, last, reps):
    from wavpackdecoder_amd import _lib, api
    b = api.DecodeBatch(4096)
    idx = b.add_files(files, flags)
    assert min(idx) >= 0
    b.decode()
    b.sync()
    values = sum(i.out_frames * i.reduced_channels for i in b.infos)
    nbytes = int(values) * 4
    L = ctypes.CDLL(_lib.LIB_PATH)
    ev = Events(L)
    stream = ctypes.c_void_p(b._L.wvg_batch_stream(b._b))
    nch = int(b.infos[0].reduced_channels)
    res = {"what": "levels_rates", "workload": name, "files": len(files), "channels": nch, "values": int(values),
           "bytes_read": nbytes, "records": sum(int(i.reduced_channels) for i in b.infos),
           "tile_frames": api.levels_tile_frames(nch), "reps": reps}
    b.levels(Q)
    b.sync()
    k = 8 * b.infos[0].bytes_per_sample - 1
    from tests.levels_vectors import expected
    want0 = expected(np.asarray(first), k, Q)
    want1 = want0 if last is first else expected(np.asarray(last), k, Q)
    res["records_equal_python_integers"] = bool(check_file(b, 0, want0) and check_file(b, len(files) - 1, want1))
    run = lambda: b._check(b._L.wvg_batch_levels(b._b, Q, None))  # noqa: E731
    lv = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    res["levels"] = {"ms": med(lv), "GBps_read": round(nbytes / np.median(lv) / 1e6, 1),
                     "runs_ms": [round(v, 4) for v in lv]}
    b.planar(0)
    b.sync()
    run = lambda: b._check(b._L.wvg_batch_planar(b._b, 0, None, 0, None))  # noqa: E731
    pl = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    floats = b.planar_floats(0)
    res["planar"] = {"ms": med(pl), "GBps_read_plus_written": round((nbytes + 4 * floats) / np.median(pl) / 1e6, 1),
                     "runs_ms": [round(v, 4) for v in pl]}
    ratio = float(np.median(lv) / np.median(pl))
    res["levels_vs_planar"] = round(ratio, 4)
    res["within_planar"] = bool(ratio <= 1.03)
    # the same ints through the copy engine's front door: device to device
    src, dst = ctypes.c_void_p(), ctypes.c_void_p()
    L.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.hipFree.argtypes = [ctypes.c_void_p]
    assert L.hipMalloc(ctypes.byref(src), nbytes) == 0 and L.hipMalloc(ctypes.byref(dst), nbytes) == 0
    assert L.hipMemsetAsync(src, 1, nbytes, stream) == 0
    ms = [ev.time(stream, lambda: L.hipMemcpyAsync(dst, src, nbytes, 3, stream)) for _ in range(reps + 1)][1:]
    res["memcpy_d2d"] = {"ms": med(ms), "GBps_read_plus_written": round(2 * nbytes / np.median(ms) / 1e6, 1),
                         "runs_ms": [round(v, 4) for v in ms]}
    b.sync()
    L.hipFree(src)
    L.hipFree(dst)
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wavpackdecoder_amd import api
    ss = stereo_sources()
    lines = [levels_rates("stereo", stereo_files(ss), 0, ss[0], ss[-1], a.reps)]
    xs = six_sources()
    woven = np.concatenate(xs, axis=1)  # the streams' channels in stream order (tests/mc_vectors.py's mux)
    lines.append(levels_rates("six", six_files(xs), api.OPEN_ALL_CHANNELS, woven, woven, a.reps))
    text = "".join(json.dumps(x) + "\n" for x in lines)
    sys.stdout.write(text)
    sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
