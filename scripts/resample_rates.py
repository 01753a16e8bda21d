"""What bringing a decoded batch to one sample rate costs (wvg_batch_resample), as JSON lines
(profiles/resample_rates.jsonl).

Workloads:
  c2_441_160   1,024 files of one 22,050-frame 16-bit stereo block at 44,100 Hz (C2's shape;
               128 distinct files, each added 8 times) -> 16,000 Hz (441:160, K = 475)
  c2_160_147   the same shape at 48,000 Hz -> 44,100 Hz (160:147, K = 174)
  six_3_1      64 copies of one 6-channel file of 352,800 frames at 48,000 Hz, opened with
               WVG_OPEN_ALL_CHANNELS -> 16,000 Hz (3:1, K = 41)
  mixed        768 stereo files of 22,050 frames, 128 each at 8,000 / 16,000 / 22,050 /
               32,000 / 44,100 / 48,000 Hz -> 16,000 Hz
Each figure is the median of --reps runs (default 9) after one warm run, device events on the
batch's stream, all in one process:
  resample   wvg_batch_resample into a torch tensor (ragged rows), with its multiply-adds
             (F' * C * K a file) as a share of the FP32 vector peak (157.3 TFLOP/s = 78.65 T
             multiply-adds a second) and the bytes it reads (4 a value) plus writes (4 a float)
  bar        what the call replaces, on the same stream between the same events, single-rate
             batches only: wvg_batch_planar into a dense [B, C, F] tensor, plus one
             torch.nn.functional.conv1d (stride orig, the same table, the rows padded by
             `width` in front and K - width behind) and the transpose / reshape to [B, C, F']
The resampled image of the first file is compared with the host run of the tile code once,
and the bar's largest difference from the call's output is recorded.

usage: python3 scripts/resample_rates.py [--reps R] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from scripts.planar_rates import Events, med  # noqa: E402

BLOCK = 22050
WIDTHS = (2, 1, 1, 2)
PEAK_FMA = 157.3e12 / 2


def stereo_files(rate, n=128, copies=8, seed=0xC2):
    from synth import wvsynth as S
    base = [S.encode_pcm(S.audio_like(BLOCK, 2, 16, seed=seed + k),
                         S.EncParams(terms=S.TERMS_FAST, block_samples=BLOCK, sample_rate=rate)) for k in range(n)]
    return base * copies


def six_files(rate):
    from synth import wvsynth as S
    from tests import mc_vectors as M
    encs = [S.encode_pcm_parallel(S.audio_like(16 * BLOCK, w, 16, seed=0x6C00 + 131 * k),
                                  S.EncParams(nch=w, terms=S.TERMS_FAST if w == 2 else [17, 17], block_samples=BLOCK,
                                              sample_rate=rate))
            for k, w in enumerate(WIDTHS)]
    return [M.mux(encs, sum(WIDTHS), 0x3F)] * 64


def rates(name, files, flags, out_rate, reps, bar):
    import torch
    from wavpackdecoder_amd import _lib, api
    b = api.DecodeBatch(4096)
    assert min(b.add_files(files, flags)) >= 0
    b.decode()
    b.sync()
    L = ctypes.CDLL(_lib.LIB_PATH)
    ev = Events(L)
    sp = b._L.wvg_batch_stream(b._b)
    stream = ctypes.c_void_p(sp)
    dev = torch.device("cuda", api.context_device())
    ts = torch.cuda.ExternalStream(sp, device=dev)
    lay = [b.file_resample(i, out_rate) for i in range(len(files))]
    floats = b.resample_floats(out_rate)
    out = torch.empty(floats, dtype=torch.float32, device=dev)
    fma, read = 0, 0
    for i, (off, rs, ch, fr) in zip(b.infos, lay):
        assert off >= 0
        read += i.out_frames * ch
        if i.sample_rate != out_rate:
            fma += fr * ch * api.resample_filter(i.sample_rate, out_rate)[3].shape[1]
    ptr = ctypes.c_void_p(out.data_ptr())
    run = lambda: b._check(b._L.wvg_batch_resample(b._b, out_rate, 0, ptr, floats, stream))  # noqa: E731
    ms = [ev.time(stream, run) for _ in range(reps + 1)][1:]
    m = float(np.median(ms))
    res = {"what": "resample_rates", "workload": name, "files": len(files), "out_rate": out_rate,
           "channels": int(b.infos[0].reduced_channels), "reps": reps,
           "resample": {"ms": med(ms), "fma": int(fma), "fma_share_of_fp32_vector_peak": round(fma / (m * 1e-3) / PEAK_FMA, 4),
                        "bytes_read_plus_written": int(read + floats) * 4,
                        "GBps": round((read + floats) * 4 / m / 1e6, 1), "runs_ms": [round(v, 4) for v in ms]}}
    b.sync()
    info = b.infos[0]
    ints = b.download()[info.out_offset: info.out_offset + info.out_frames * lay[0][2]].reshape(-1, lay[0][2])
    k = 8 * info.bytes_per_sample - 1
    want = api.resample_float(ints, k, info.sample_rate, out_rate, lay[0][3], lay[0][1])
    got = out[lay[0][0]: lay[0][0] + lay[0][1] * lay[0][2]].cpu().numpy()
    res["output_equals_host"] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32).reshape(-1)))
    if bar:
        in_rate = int(info.sample_rate)
        orig, new, width, h = api.resample_filter(in_rate, out_rate)
        K = h.shape[1]
        F, C, B = int(info.out_frames), lay[0][2], len(files)
        Fo = lay[0][3]
        dense = torch.empty(B * C * F, dtype=torch.float32, device=dev)
        w = torch.from_numpy(h).to(dev).view(new, 1, K)
        box = {}
        dptr = ctypes.c_void_p(dense.data_ptr())

        def both():
            b._check(b._L.wvg_batch_planar(b._b, F, dptr, dense.numel(), stream))
            with torch.cuda.stream(ts):
                x = torch.nn.functional.pad(dense.view(B * C, 1, F), (width, K - width + orig))
                y = torch.nn.functional.conv1d(x, w, stride=orig)
                box["y"] = y.transpose(1, 2).reshape(B * C, -1)[:, :Fo].contiguous()

        def only_planar():
            b._check(b._L.wvg_batch_planar(b._b, F, dptr, dense.numel(), stream))

        bms = [ev.time(stream, both) for _ in range(reps + 1)][1:]
        pms = [ev.time(stream, only_planar) for _ in range(reps + 1)][1:]
        b.sync()
        ref = box["y"].view(B, C, Fo)[0].cpu().numpy()
        mine = got.reshape(C, -1)[:, :Fo]
        res["bar"] = {"ms": med(bms), "planar_ms": med(pms), "conv1d_and_reshape_ms": round(med(bms) - med(pms), 4),
                      "max_abs_difference_from_resample": float(np.max(np.abs(ref - mine))),
                      "runs_ms": [round(v, 4) for v in bms]}
        res["resample_faster_than_bar"] = bool(m < float(np.median(bms)))
    b.sync()
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library loads: the process must hold one HIP runtime)
    from wavpackdecoder_amd import api
    jobs = {
        "c2_441_160": lambda: rates("c2_441_160", stereo_files(44100), 0, 16000, a.reps, True),
        "c2_160_147": lambda: rates("c2_160_147", stereo_files(48000), 0, 44100, a.reps, True),
        "six_3_1": lambda: rates("six_3_1", six_files(48000), api.OPEN_ALL_CHANNELS, 16000, a.reps, False),
        "mixed": lambda: rates("mixed", [f for k, r in enumerate((8000, 16000, 22050, 32000, 44100, 48000))
                                         for f in stereo_files(r, 16, 8, seed=0x700 + 16 * k)], 0, 16000, a.reps, False),
    }
    text = ""
    for name, job in jobs.items():
        if a.only and name not in a.only.split(","):
            continue
        line = json.dumps(job()) + "\n"
        sys.stdout.write(line)
        sys.stdout.flush()
        text += line
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
