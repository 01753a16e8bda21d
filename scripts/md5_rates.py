"""What verifying stored MD5 sums on the device costs (wvg_batch_md5), as JSON lines:

  c5_verify    the first N files of C5 (default 4,000): the device time of wvg_batch_md5
               alone (an event pair on the batch stream; the 16-byte-a-file digest copy
               queued behind the kernel is inside it) and the wall time of decode + md5 +
               sync, against the route a caller had without it -- decode + format +
               page-locked PCM download + hashlib.md5 per file on 16 threads -- and the
               ratio.  Every device digest is compared with hashlib's over the downloaded
               PCM (DSD files over the dsd=True image).
  serial_chain one long file alone (C1): bytes per second of one lane's chain, beside
               hashlib's rate on one host thread over the same bytes.

Medians of --reps runs after one warm run.  usage: python3 scripts/md5_rates.py [--files N] [--reps R]"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


class Events:
    """a hipEvent pair on a raw hipStream_t"""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.e = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def record(self, k, stream):
        assert self.hip.hipEventRecord(self.e[k], ctypes.c_void_p(stream)) == 0

    def ms(self):
        out = ctypes.c_float()
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        assert self.hip.hipEventElapsedTime(ctypes.byref(out), self.e[0], self.e[1]) == 0
        return float(out.value)


def md5_event_ms(b, ev):
    stream = b._L.wvg_batch_stream(b._b)
    ev.record(0, stream)
    b.md5()
    ev.record(1, stream)
    ms = ev.ms()
    b.sync()
    return ms


def med(v):
    return round(float(np.median(v)), 3)


def c5_verify(nfiles, reps, ev):
    from synth import corpora
    from wavpackdecoder_amd.api import DecodeBatch
    files = corpora.c5(nfiles)
    b = DecodeBatch(4096)
    b.add_files(files)
    b.upload()
    b.sync()
    n = len(files)
    pool = ThreadPoolExecutor(16)
    dev_wall, dev_decode, dev_md5, host_wall, host_gpu, host_hash = [], [], [], [], [], []
    host_digests = None
    for r in range(reps + 1):  # the first run warms both routes (code objects, buffers grown)
        t0 = time.perf_counter()
        b.decode()
        b.md5()
        b.sync()
        t1 = time.perf_counter()
        b.decode()
        b.sync()
        t2 = time.perf_counter()
        kernel_ms = md5_event_ms(b, ev)
        t3 = time.perf_counter()
        b.decode()
        b.format(dsd=False)
        pcm = b.download_pcm(pinned=True)
        t4 = time.perf_counter()
        spans = [(b.pcm_offset(i), b.file_md5(i).bytes) for i in range(n)]
        t5 = time.perf_counter()
        host_digests = list(pool.map(lambda s: hashlib.md5(pcm[s[0]:s[0] + s[1]]).digest(), spans))
        t6 = time.perf_counter()
        if r:
            dev_wall.append((t1 - t0) * 1e3)
            dev_decode.append((t2 - t1) * 1e3)
            dev_md5.append(kernel_ms)
            host_gpu.append((t4 - t3) * 1e3)
            host_hash.append((t6 - t5) * 1e3)
            host_wall.append((t4 - t3 + t6 - t5) * 1e3)
    # every device digest against hashlib over the downloaded PCM
    dsd = [b.infos[i].dsd_multiplier > 0 for i in range(n)]
    b.format(dsd=True)
    pcm_d = b.download_pcm(pinned=True)
    wrong = 0
    for i in range(n):
        r = b.file_md5(i)
        o = b.pcm_offset(i)
        want = hashlib.md5(pcm_d[o:o + r.bytes]).digest() if dsd[i] else host_digests[i]
        wrong += bytes(r.computed) != want
    pcm_bytes = int(sum(s[1] for s in spans))
    b.close()
    return {"what": "c5_verify", "files": n, "pcm_bytes": pcm_bytes, "digests_wrong": int(wrong),
            "device": {"md5_kernel_ms": med(dev_md5), "decode_sync_ms": med(dev_decode),
                       "decode_md5_sync_wall_ms": med(dev_wall)},
            "download_and_hash": {"decode_format_download_ms": med(host_gpu), "hashlib_16_threads_ms": med(host_hash),
                                  "wall_ms": med(host_wall)},
            "ratio_host_over_device": round(float(np.median(host_wall) / np.median(dev_wall)), 2),
            "md5_kernel_GBps": round(pcm_bytes / np.median(dev_md5) / 1e6, 2), "reps": reps}


def serial_chain(reps, ev):
    from synth import corpora
    from wavpackdecoder_amd.api import DecodeBatch
    pcm, wv = corpora.c1()
    b = DecodeBatch(4096)
    b.add_file(wv)
    b.decode()
    b.sync()
    ms = [md5_event_ms(b, ev) for _ in range(reps + 1)][1:]
    r = b.file_md5(0)
    src = pcm.astype("<i2").tobytes()
    ok = bytes(r.computed) == hashlib.md5(src).digest()
    th = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hashlib.md5(src).digest()
        th.append((time.perf_counter() - t0) * 1e3)
    b.close()
    return {"what": "serial_chain", "file": "C1", "bytes": int(r.bytes), "digest_ok": bool(ok), "md5_kernel_ms": med(ms),
            "lane_MBps": round(r.bytes / np.median(ms) / 1e3, 2), "hashlib_one_thread_ms": med(th),
            "hashlib_MBps": round(r.bytes / np.median(th) / 1e3, 1), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ev = Events()
    print(json.dumps(serial_chain(a.reps, ev)), flush=True)
    print(json.dumps(c5_verify(a.files, a.reps, ev)), flush=True)


if __name__ == "__main__":
    main()
