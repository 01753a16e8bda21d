"""What the integrated loudness of a decoded batch costs (wvg_batch_loudness), as JSON lines
(profiles/loudness_rates.jsonl).

Workloads:
  stereo  1,024 files of one 22,050-frame 16-bit stereo block at 44,100 Hz (C2's shape,
          scripts/levels_rates.py's files): 5 steps and 2 blocks a file
  long    one 10-minute 16-bit stereo file at 48,000 Hz (28.8 M frames, 6,000 steps): the
          shape with the fewest lanes per frame
  six     64 copies of one 6-channel file (scripts/levels_rates.py's), WVG_OPEN_ALL_CHANNELS
Each figure is the median of --reps runs (default 9) after one warm run, between two
events on the batch's stream, all in one process:
  loudness  wvg_batch_loudness: wv_loud_runs, wv_loud_blocks, wv_loud_gate and the download
            of the records
  levels    wvg_batch_levels on the same batch (threshold 2^20): it reads the same ints once
  planar    wvg_batch_planar, ragged rows into the batch's buffer, on the same batch
`loudness_vs_levels` and `loudness_vs_planar` are the ratios of the medians; `ns_per_frame`
is loudness over the batch's frames.  `run_steps` is the library's R (a build constant:
an A/B runs this script once per build, WVG_LIB naming the library).  After the timed
region the first and the last file's records and block powers are compared bit for bit
with the host build of the same code (wvg_loudness_ints) over the generator's arrays.

usage: python3 scripts/loudness_rates.py [--reps R] [--shapes stereo,long,six] [--cache DIR] [--out FILE]
  --cache DIR   keep the encoded files in DIR between runs (an A/B encodes once)
  --out FILE    append the lines to FILE"""
import argparse
import ctypes
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

import levels_rates as LR  # noqa: E402  (the stereo and six workloads, the event pair)

LONG_RATE, LONG_FRAMES, MINUTE = 48000, 600 * 48000, 60 * 48000
Q = 1 << 20


def long_source():
    """ten minutes from one minute of the generator's audio, each minute at another level"""
    from synth import wvsynth as S
    x = S.audio_like(MINUTE, 2, 16, seed=0x10AD).astype(np.int64)
    gains = (1.0, 0.5, 0.05, 0.8, 0.002, 1.0, 0.3, 0.0, 0.6, 0.9)
    return np.concatenate([np.round(x * g).astype(np.int32) for g in gains], axis=0)


def long_files(src):
    from synth import wvsynth as S
    return [S.encode_pcm_parallel(src, S.EncParams(terms=S.TERMS_FAST, block_samples=LR.BLOCK,
                                                   sample_rate=LONG_RATE))]


def cached(cache, name, make):
    if not cache:
        return make()
    path = os.path.join(cache, name + ".pickle")
    if os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    v = make()
    os.makedirs(cache, exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(v, f)
    return v


def same_as_host(b, i, src, k, rate, mask, img):
    from wavpackdecoder_amd import api
    rec = b.file_loudness(i)
    hrec, hblk = api.loudness_ints(np.asarray(src), k, rate, mask)
    if rec is None:
        return False
    o, n = int(rec["block_offset"]), int(rec["blocks"])
    hrec["block_offset"] = o
    return rec.tobytes() == hrec.tobytes() and img[o: o + n].tobytes() == hblk.tobytes()


def loudness_rates(name, files, flags, first, last, rate, mask, reps):
    from wavpackdecoder_amd import _lib, api
    b = api.DecodeBatch(4096)
    idx = b.add_files(files, flags)
    assert min(idx) >= 0
    b.decode()
    b.sync()
    frames = int(sum(i.out_frames for i in b.infos))
    values = int(sum(i.out_frames * i.reduced_channels for i in b.infos))
    L = ctypes.CDLL(_lib.LIB_PATH)
    ev = LR.Events(L)
    stream = ctypes.c_void_p(b._L.wvg_batch_stream(b._b))
    nch = int(b.infos[0].reduced_channels)
    res = {"what": "loudness_rates", "workload": name, "files": len(files), "channels": nch, "rate": rate,
           "frames": frames, "bytes_read_once": values * 4, "run_steps": int(b._L.wvg_loudness_run_steps()),
           "library": os.path.relpath(_lib.LIB_PATH, os.path.join(HERE, "..")), "reps": reps}
    b.loudness()
    b.sync()
    res["blocks"] = int(b._L.wvg_batch_loudness_blocks(b._b))
    run = lambda: b._check(b._L.wvg_batch_loudness(b._b, None))  # noqa: E731
    ld = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    res["loudness"] = {"ms": LR.med(ld), "ns_per_frame": round(float(np.median(ld)) * 1e6 / frames, 4),
                       "runs_ms": [round(v, 4) for v in ld]}
    b.levels(Q)
    b.sync()
    run = lambda: b._check(b._L.wvg_batch_levels(b._b, Q, None))  # noqa: E731
    lv = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    res["levels"] = {"ms": LR.med(lv), "runs_ms": [round(v, 4) for v in lv]}
    b.planar(0)
    b.sync()
    run = lambda: b._check(b._L.wvg_batch_planar(b._b, 0, None, 0, None))  # noqa: E731
    pl = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    res["planar"] = {"ms": LR.med(pl), "runs_ms": [round(v, 4) for v in pl]}
    res["loudness_vs_levels"] = round(float(np.median(ld) / np.median(lv)), 2)
    res["loudness_vs_planar"] = round(float(np.median(ld) / np.median(pl)), 2)
    # after the timed region: the last call's results against the host code
    b.sync()
    img = b.download_loudness_blocks()
    k = 8 * b.infos[0].bytes_per_sample - 1
    res["equal_host_code_bit_for_bit"] = bool(same_as_host(b, 0, first, k, rate, mask, img) and
                                              same_as_host(b, len(files) - 1, last, k, rate, mask, img))
    rec = b.file_loudness(0)
    res["file0"] = {"power": float(rec["power"]), "blocks": int(rec["blocks"]), "gated_blocks": int(rec["gated_blocks"])}
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="stereo,long,six")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wavpackdecoder_amd import api
    lines = []
    for shape in a.shapes.split(","):
        if shape == "stereo":
            ss = LR.stereo_sources()
            files = cached(a.cache, "stereo", lambda: LR.stereo_files(ss))
            lines.append(loudness_rates("stereo", files, 0, ss[0], ss[-1], 44100, 0, a.reps))
        elif shape == "long":
            src = long_source()
            files = cached(a.cache, "long", lambda: long_files(src))
            lines.append(loudness_rates("long", files, 0, src, src, LONG_RATE, 0, a.reps))
        elif shape == "six":
            xs = LR.six_sources()
            woven = np.concatenate(xs, axis=1)
            files = cached(a.cache, "six", lambda: LR.six_files(xs))
            lines.append(loudness_rates("six", files, api.OPEN_ALL_CHANNELS, woven, woven, 44100, 0x3F, a.reps))
        else:
            raise SystemExit(f"unknown shape {shape}")
        sys.stdout.write(json.dumps(lines[-1]) + "\n")
        sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
