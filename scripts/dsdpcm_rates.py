"""What opening DSD files as 24-bit PCM costs (WVG_OPEN_DSD_AS_PCM, wv_dsdpcm.hip), as JSON
lines (profiles/dsdpcm_rates.jsonl).

Workload: 1,024 stereo DSD files of one 22,050-frame block (C2's block shape; 128 distinct
files, each added 8 times): 45.2 M values, 4 bytes read and 4 written a value by the
decimation kernel.  Each figure is the median of --reps runs (default 9) after one warm run,
all in one process; a decode is timed on the device (wvg_batch_time: events on the batch's
stream around one wvg_batch_decode).
  decode          wvg_batch_decode of the batch with and without the flag, per DSD mode (0:
                  stored bytes, 1: fast, 3: high)
  dsd_pcm_kernel  the decimation kernel: flagged minus unflagged decode of the mode-0 batch
                  (the cheapest decode, so the difference is the kernel plus its launch),
                  over the bytes it reads plus writes
  planar          wvg_batch_planar (ragged) on a 16-bit stereo PCM batch of the same number
                  of values between two events: the same bytes read plus written
  decode_groups   one line per DSD mode (1, 3), kernel choice (auto, lane, two_wave) and flag:
                  the end of the last launch group against the decode's start
                  (wvg_batch_group_times: the decode kernels alone, before the decimation
                  kernel) and the whole decode (wvg_batch_timed), medians of 5 after a warm run
The flagged output of the first and the last file is compared once with the host tile code
(wvg_dsd_pcm_ints) over the unflagged output.

usage: python3 scripts/dsdpcm_rates.py [--reps R] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from scripts.planar_rates import BLOCK, Events, med, stereo_files  # noqa: E402


_SOURCES = []


def dsd_files(mode):
    from synth import wvsynth as S
    if not _SOURCES:  # (the sigma-delta sources are the slow part: made once for the three modes)
        _SOURCES.extend(S.dsd_like(BLOCK, 2, seed=0xD5D + k) for k in range(128))
    base = [S.encode_dsd(x, S.DsdParams(nch=2, mode=mode, block_samples=BLOCK, rate_multiplier_log2=3))
            for x in _SOURCES]
    return base * 8


def decode_ms(files, flags, reps, keep=False):
    from wavpackdecoder_amd import api
    b = api.DecodeBatch(4096)
    assert min(b.add_files(files, flags)) >= 0
    b.upload()
    ms = [b.time(1) for _ in range(reps + 1)][1:]
    if keep:
        return ms, b
    b.close()
    return ms


def decode_groups(mode, files):
    from wavpackdecoder_amd import api
    lines = []
    for kernel in ("auto", "lane", "two_wave"):
        for flags in (0, api.OPEN_DSD_AS_PCM):
            b = api.DecodeBatch(4096)
            b.set_kernel(kernel)
            assert min(b.add_files(files, flags)) >= 0
            b.upload()
            b.set_timing(True)
            ends, whole = [], []
            for r in range(6):
                b.set_timing(True)  # (drops the pairs before: timed() is this decode's)
                b.decode()
                b.sync()
                if r:
                    ends.append(max(b.group_times().values()))
                    whole.append(b.timed()[0])
            lines.append({"what": "dsdpcm_decode_groups", "mode": mode, "kernel": kernel, "flagged": bool(flags),
                          "last_group_end_ms": med(ends), "decode_ms": med(whole), "out_ints": b.out_ints})
            b.close()
    return lines


def planar_ms(reps):
    from wavpackdecoder_amd import _lib, api
    b = api.DecodeBatch(4096)
    assert min(b.add_files(stereo_files(), 0)) >= 0
    b.decode()
    b.sync()
    values = sum(i.out_frames * i.reduced_channels for i in b.infos)
    ev = Events(ctypes.CDLL(_lib.LIB_PATH))
    stream = ctypes.c_void_p(b._L.wvg_batch_stream(b._b))
    run = lambda: b._check(b._L.wvg_batch_planar(b._b, 0, None, 0, None))  # noqa: E731
    ms = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    b.close()
    return ms, int(values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wavpackdecoder_amd import api
    res = {"what": "dsdpcm_rates", "workload": "stereo_dsd_c2_blocks", "files": 1024, "channels": 2, "reps": a.reps}
    groups = []
    for mode in (0, 1, 3):
        files = dsd_files(mode)
        if mode:
            groups += decode_groups(mode, files)
        plain = decode_ms(files, 0, a.reps)
        flagged, b = decode_ms(files, api.OPEN_DSD_AS_PCM, a.reps, keep=True)
        res[f"decode_mode{mode}"] = {"unflagged_ms": med(plain), "flagged_ms": med(flagged),
                                     "unflagged_runs_ms": [round(v, 4) for v in plain],
                                     "flagged_runs_ms": [round(v, 4) for v in flagged]}
        if mode == 0:
            values = sum(i.out_frames * i.reduced_channels for i in b.infos)
            d = float(np.median(flagged) - np.median(plain))
            res["values"] = int(values)
            res["bytes_read_plus_written"] = int(values) * 8
            res["dsd_pcm_kernel"] = {"flagged_minus_unflagged_ms": round(d, 4),
                                     "GBps": round(values * 8 / d / 1e6, 1) if d > 0 else None}
            out = b.download()
            c = api.DecodeBatch(4096)
            c.add_files(files, 0)
            c.decode()
            ref = c.download()
            ok = True
            for i in (0, len(files) - 1):
                fl, un = b.infos[i], c.infos[i]
                n = fl.out_frames * 2
                want = api.dsd_pcm_ints(ref[un.out_offset: un.out_offset + n].reshape(-1, 2))
                ok = ok and bool(np.array_equal(out[fl.out_offset: fl.out_offset + n].reshape(-1, 2), want))
            res["output_equals_host_tile_code"] = ok
            c.close()
        b.close()
    ms, values = planar_ms(a.reps)
    res["planar"] = {"values": values, "ms": med(ms), "GBps": round(values * 8 / np.median(ms) / 1e6, 1),
                     "runs_ms": [round(v, 4) for v in ms]}
    text = "".join(json.dumps(x) + "\n" for x in [res] + groups)
    sys.stdout.write(text)
    sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
