"""What the true peak of a decoded batch costs (wvg_batch_true_peak), as JSON lines
(profiles/true_peak_rates.jsonl).

Workloads: scripts/levels_rates.py's two, both 22.6 M frames (1,024 stereo files of 22,050
frames; 64 six-channel files of 352,800 frames under WVG_OPEN_ALL_CHANNELS).
Each figure is the median of --reps runs (default 9) after one warm run, between two
events on the batch's stream, all in one process:
  true_peak   wvg_batch_true_peak at O = 1, 2 and 4: wv_tpeak_tiles, wv_tpeak_combine and
              the download of the records
  levels      wvg_batch_levels on the same ints: the yardstick.  `vs_levels` is true_peak /
              levels at each O; at O = 1 the call reads the same bytes and writes as little,
              and `o1_within_levels` says whether it is at most 1.03 (the run-to-run spread)
  planar      wvg_batch_planar, ragged rows into the batch's buffer, on the same batch
After the timed region the records of the first and the last file at each O are compared
with the kernels' code run on the host (wvg_true_peak_ints) over the generator's arrays.

usage: python3 scripts/true_peak_rates.py [--reps R] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

import levels_rates as LR  # noqa: E402

FACTORS = (1, 2, 4)


def same(got, want):
    return got is not None and len(got) == len(want) and all(
        int(g[f]) == int(w[f]) for g, w in zip(got, want) for f in got.dtype.names)


def true_peak_rates(name, files, flags, first, last, reps):
    from wavpackdecoder_amd import _lib, api
    b = api.DecodeBatch(4096)
    idx = b.add_files(files, flags)
    assert min(idx) >= 0
    b.decode()
    b.sync()
    values = sum(i.out_frames * i.reduced_channels for i in b.infos)
    nbytes = int(values) * 4
    ev = LR.Events(ctypes.CDLL(_lib.LIB_PATH))
    stream = ctypes.c_void_p(b._L.wvg_batch_stream(b._b))
    nch = int(b.infos[0].reduced_channels)
    k = 8 * b.infos[0].bytes_per_sample - 1
    res = {"what": "true_peak_rates", "workload": name, "files": len(files), "channels": nch, "values": int(values),
           "bytes_read": nbytes, "records": sum(int(i.reduced_channels) for i in b.infos),
           "tile_frames": api.true_peak_tile_frames(nch), "levels_tile_frames": api.levels_tile_frames(nch),
           "reps": reps}

    def timed(call):
        call()
        b.sync()
        ms = [ev.time(stream, call) for _ in range(reps + 1)][1:]
        return ms

    lv = timed(lambda: b._check(b._L.wvg_batch_levels(b._b, LR.Q, None)))
    res["levels"] = {"ms": LR.med(lv), "GBps_read": round(nbytes / np.median(lv) / 1e6, 1),
                     "runs_ms": [round(v, 4) for v in lv]}
    pl = timed(lambda: b._check(b._L.wvg_batch_planar(b._b, 0, None, 0, None)))
    res["planar"] = {"ms": LR.med(pl), "runs_ms": [round(v, 4) for v in pl]}
    got = {}
    for o in FACTORS:
        tp = timed(lambda: b._check(b._L.wvg_batch_true_peak(b._b, o, None)))
        b.sync()
        got[o] = (b.file_true_peak(0), b.file_true_peak(len(files) - 1))
        res[f"true_peak_o{o}"] = {"ms": LR.med(tp), "GBps_read": round(nbytes / np.median(tp) / 1e6, 1),
                                  "G_multiply_adds_per_s": round(values * 12 * (o - 1) / np.median(tp) / 1e6, 1),
                                  "vs_levels": round(float(np.median(tp) / np.median(lv)), 4),
                                  "runs_ms": [round(v, 4) for v in tp]}
    # the yardstick once more, behind the true-peak runs: the spread of levels itself
    lv2 = timed(lambda: b._check(b._L.wvg_batch_levels(b._b, LR.Q, None)))
    res["levels_again"] = {"ms": LR.med(lv2), "runs_ms": [round(v, 4) for v in lv2]}
    res["o1_within_levels"] = bool(res["true_peak_o1"]["vs_levels"] <= 1.03)
    b.close()
    # after the timed region: the device's records against the kernels' code on the host
    ok = True
    for o in FACTORS:
        ok = ok and same(got[o][0], api.true_peak_ints(np.asarray(first), k, o))
        ok = ok and same(got[o][1], api.true_peak_ints(np.asarray(last), k, o))
    res["records_equal_host_code"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wavpackdecoder_amd import api
    ss = LR.stereo_sources()
    lines = [true_peak_rates("stereo", LR.stereo_files(ss), 0, ss[0], ss[-1], a.reps)]
    xs = LR.six_sources()
    woven = np.concatenate(xs, axis=1)  # the streams' channels in stream order (tests/mc_vectors.py's mux)
    lines.append(true_peak_rates("six", LR.six_files(xs), api.OPEN_ALL_CHANNELS, woven, woven, a.reps))
    text = "".join(json.dumps(x) + "\n" for x in lines)
    sys.stdout.write(text)
    sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
