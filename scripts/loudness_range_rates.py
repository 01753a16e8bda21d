"""What the loudness range of a decoded batch costs beyond its integrated loudness
(wvg_batch_loudness_range), as JSON lines (profiles/loudness_range_rates.jsonl).

Workloads:
  stereo  scripts/loudness_rates.py's: 1,024 half-second files, none long enough for one
          short-term value -- the call's fixed cost
  long    scripts/loudness_rates.py's: one 10-minute stereo file at 48,000 Hz, 5,971 values in
          one workgroup of the select kernel
  six     scripts/loudness_rates.py's: 64 six-channel files of 8 s, 51 values each
  many    64 copies of one 3-minute 16-bit stereo file at 44,100 Hz (1,771 values each): the
          shape of an album or a dataset shard
Each figure is the median of --reps runs (default 9) after one warm run, between two
events on the batch's stream, all in one process:
  loudness  wvg_batch_loudness on the batch: the yardstick
  range     wvg_batch_loudness_range with that loudness call already issued: the call's
            additional time -- wv_lra_short, wv_lra_gate, wv_lra_select and the download of
            the records
`range_vs_loudness` is the ratio of the medians.  After the timed region the first and the
last file's records and short-term powers are compared bit for bit with the host build of
the same code (wvg_loudness_range_ints) over the generator's arrays.

usage: python3 scripts/loudness_range_rates.py [--reps R] [--shapes stereo,long,six,many] [--cache DIR] [--out FILE]
  --cache DIR   keep the encoded files in DIR between runs
  --out FILE    append the lines to FILE"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

import levels_rates as LR  # noqa: E402  (the stereo and six workloads, the event pair)
import loudness_rates as LD  # noqa: E402  (the long workload, the cache)

MANY_RATE, MANY_MINUTE, MANY_FILES = 44100, 60 * 44100, 64


def many_source():
    """three minutes from one minute of the generator's audio, every 20 s at another level"""
    from synth import wvsynth as S
    x = S.audio_like(MANY_MINUTE, 2, 16, seed=0x3342).astype(np.float64)
    gains = (1.0, 0.3, 0.02, 0.6, 0.0005, 0.9, 0.1, 0.0, 0.5)
    g = np.repeat(np.asarray(gains), MANY_MINUTE // 3)[:, None]
    return np.round(np.tile(x, (3, 1)) * g).astype(np.int32)


def many_files(src):
    from synth import wvsynth as S
    return [S.encode_pcm_parallel(src, S.EncParams(terms=S.TERMS_FAST, block_samples=LR.BLOCK,
                                                   sample_rate=MANY_RATE))] * MANY_FILES


def same_as_host(b, i, src, k, rate, mask, img):
    from wavpackdecoder_amd import api
    rec = b.file_loudness_range(i)
    hrec, hst = api.loudness_range_ints(np.asarray(src), k, rate, mask)
    if rec is None:
        return False
    o, n = int(rec["short_offset"]), int(rec["shorts"])
    hrec["short_offset"] = o
    return rec.tobytes() == hrec.tobytes() and img[o: o + n].tobytes() == hst.tobytes()


def range_rates(name, files, flags, first, last, rate, mask, reps):
    from wavpackdecoder_amd import _lib, api
    b = api.DecodeBatch(4096)
    idx = b.add_files(files, flags)
    assert min(idx) >= 0
    b.decode()
    b.sync()
    frames = int(sum(i.out_frames for i in b.infos))
    L = ctypes.CDLL(_lib.LIB_PATH)
    ev = LR.Events(L)
    stream = ctypes.c_void_p(b._L.wvg_batch_stream(b._b))
    res = {"what": "loudness_range_rates", "workload": name, "files": len(files),
           "channels": int(b.infos[0].reduced_channels), "rate": rate, "frames": frames,
           "library": os.path.relpath(_lib.LIB_PATH, os.path.join(HERE, "..")), "reps": reps}
    b.loudness()
    b.sync()
    run = lambda: b._check(b._L.wvg_batch_loudness(b._b, None))  # noqa: E731
    ld = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    res["loudness"] = {"ms": LR.med(ld), "runs_ms": [round(v, 4) for v in ld]}
    b.loudness_range()  # behind the loudness calls above: only the three new kernels and the download
    b.sync()
    res["shorts"] = int(b._L.wvg_batch_loudness_shorts(b._b))
    run = lambda: b._check(b._L.wvg_batch_loudness_range(b._b, None))  # noqa: E731
    lr = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    res["range"] = {"ms": LR.med(lr), "runs_ms": [round(v, 4) for v in lr]}
    res["range_vs_loudness"] = round(float(np.median(lr) / np.median(ld)), 4)
    # after the timed region: the last call's results against the host code
    b.sync()
    img = b.download_loudness_shorts()
    k = 8 * b.infos[0].bytes_per_sample - 1
    res["equal_host_code_bit_for_bit"] = bool(same_as_host(b, 0, first, k, rate, mask, img) and
                                              same_as_host(b, len(files) - 1, last, k, rate, mask, img))
    rec = b.file_loudness_range(0)
    lra = 10.0 * np.log10(float(rec["high_power"]) / float(rec["low_power"])) if int(rec["gated_shorts"]) else 0.0
    res["file0"] = {"shorts": int(rec["shorts"]), "gated_shorts": int(rec["gated_shorts"]), "lra_lu": round(float(lra), 4)}
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="stereo,long,six,many")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wavpackdecoder_amd import api
    lines = []
    for shape in a.shapes.split(","):
        if shape == "stereo":
            ss = LR.stereo_sources()
            files = LD.cached(a.cache, "stereo", lambda: LR.stereo_files(ss))
            lines.append(range_rates("stereo", files, 0, ss[0], ss[-1], 44100, 0, a.reps))
        elif shape == "long":
            src = LD.long_source()
            files = LD.cached(a.cache, "long", lambda: LD.long_files(src))
            lines.append(range_rates("long", files, 0, src, src, LD.LONG_RATE, 0, a.reps))
        elif shape == "six":
            xs = LR.six_sources()
            woven = np.concatenate(xs, axis=1)
            files = LD.cached(a.cache, "six", lambda: LR.six_files(xs))
            lines.append(range_rates("six", files, api.OPEN_ALL_CHANNELS, woven, woven, 44100, 0x3F, a.reps))
        elif shape == "many":
            src = many_source()
            files = LD.cached(a.cache, "many", lambda: many_files(src))
            lines.append(range_rates("many", files, 0, src, src, MANY_RATE, 0, a.reps))
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
