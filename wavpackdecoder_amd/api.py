"""Host-side mirror of the reference's public API for the decode path.

Reference (C#, Quake4/WavPackDecoder WavPackUtils.cs):
    WavpackOpenFileInput(BinaryReader, uint flags=0)      :36-120
    WavpackUnpackSamples(WavpackContext, int[] buffer, long samples)  :200-282
    WavpackFormatSamples(int[] src, long samcnt, int bps, byte[] pcm, int offset=0, bool dsd=false) :288-341
    WavpackGetNumSamples / GetSampleIndex / GetNumErrors / Lossy / GetSampleRate /
    GetNumChannels / GetBitsPerSample / GetBytesPerSample / GetReducedChannels /
    GetMode / GetFileFormat / GetFileExtension / GetErrorMessage / GetHeader /
    GetTrailer / GetIsFive / GetVersion / GetIsFloat       :346-499

Same names, same argument meaning and the same error behaviour (errors are
reported through GetErrorMessage; a call that the reference would abort with a
C# exception raises WavpackException here, after every earlier call has
returned its frames).  Underneath, the whole file is decoded by the MI355X
kernels on the first WavpackUnpackSamples call and served from the decoded
buffer; the chunk schedule is the caller's request size (the reference's
seams are a function of it).  GetSampleIndex / GetNumErrors follow the calls
made so far (WavPackUtils.cs:273-275, 355-366).  A caller that changes its
request size mid-stream gets the samples of a decode scheduled at the first
request size: identical for every well-formed stream (seams only matter for
the (short) weight store of pathological weights and for the mute granularity
of corrupted streams), and reported through `schedule_changed`.

For throughput use DecodeBatch: many files, one upload, one decode.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np

from . import _lib as _L  # noqa: E402


def configure_hw_queues(n: int = 16) -> None:
    """Opt-in: ask HIP for `n` hardware queues per process (GPU_MAX_HW_QUEUES; HIP's
    default is 4).  A decode runs its launch groups on streams of their own and a
    server keeps several batches in flight; streams beyond the process's queues
    share one and their kernels serialise.  It only takes effect before the
    process's first HIP call, and it applies to every HIP user of the process, so
    the library never sets it by itself: call this (or export the variable in the
    launcher) first.  Measured (profiles/r06_pipe_pc.jsonl): a producer/consumer
    server over 16-20 batches serves ~7,000 Msamples/s of C2 PCM on HIP's 4 queues
    and 9,500-10,400 on 24 (bench.py's setting)."""
    if not 1 <= int(n) <= 32:
        raise ValueError("GPU_MAX_HW_QUEUES must be in 1..32")
    os.environ["GPU_MAX_HW_QUEUES"] = str(int(n))

SAMPLE_BUFFER_SIZE = 4096  # Defines.cs:18
OPEN_2CH_MAX = 0x8         # Defines.cs:26
# beyond the reference: float files decode to float32 bit patterns, exact via the wvx stream
# (WVG_OPEN_EXACT_FLOAT, include/wvgpu.h)
OPEN_EXACT_FLOAT = 0x40000000
# beyond the reference: a file of more than two channels opens and every channel is decoded
# (WVG_OPEN_ALL_CHANNELS, include/wvgpu.h); not with OPEN_2CH_MAX, start_sample or wvc
OPEN_ALL_CHANNELS = 0x20000000
# beyond the reference: a DSD file opens as 24-bit PCM at the DSD byte rate, decimated on the
# device (WVG_OPEN_DSD_AS_PCM, include/wvgpu.h); not with OPEN_ALL_CHANNELS, start_sample or
# wvc; a file that is not DSD is unchanged
OPEN_DSD_AS_PCM = 0x10000000


class WavpackException(RuntimeError):
    """The reference would have raised a C# exception (WvDemo.cs:144 catch)."""


class DecoderTimeout(RuntimeError):
    """A decode kernel's bounded wait ran out (WVG_ST_TIMEOUT): a decoder fault, never a
    property of the stream and never reported as a reference exception."""


_ctx = None
_ctx_device = -1  # the HIP device of the context (the process's current device when it was opened)


def _context():
    global _ctx, _ctx_device
    if _ctx is None:
        L = _L.lib()
        _ctx = L.wvg_open(-1)
        if not _ctx:
            raise RuntimeError("wvg_open failed: no HIP device visible (the decode path is GPU-only)")
        dev = ctypes.c_int(-1)
        if L.hipGetDevice(ctypes.byref(dev)) == 0:  # (the HIP runtime libwvgpu.so is linked against)
            _ctx_device = int(dev.value)
    return _ctx


def _torch():
    """torch, imported lazily (the package works without it), and the check that the process
    holds one HIP runtime: torch's wheels ship their own libamdhip64, which the loader
    shares with libwvgpu.so only when torch is imported first.  With two runtimes a
    tensor's pointer means nothing to the kernels here, so that is an error, not a try."""
    import torch
    seen = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    seen.add(line.split()[-1])
    except OSError:
        pass
    if len(seen) > 1:
        raise RuntimeError("two HIP runtimes in this process (" + ", ".join(sorted(seen)) + "): import torch "
                           "before the first use of wavpackdecoder_amd, so that both share torch's")
    return torch


def context_device() -> int:
    """The HIP device index every DecodeBatch of this process decodes on."""
    _context()
    return _ctx_device


def _file_arrays(files):
    """(the files as bytes objects, a c_char_p array of them, their lengths as a uint64
    array) for the C-ABI's file-array calls; bytes inputs are passed as they are."""
    bufs = files if all(type(f) is bytes for f in files) else [bytes(f) for f in files]
    ptrs = (ctypes.c_char_p * len(bufs))(*bufs)
    lens = np.fromiter(map(len, bufs), dtype=np.uint64, count=len(bufs))
    return bufs, ptrs, lens


class DecodeBatch:
    """A batch of .wv files decoded together on one GPU (files shard across GPUs)."""

    def __init__(self, chunk_frames: int = SAMPLE_BUFFER_SIZE):
        self._L = _L.lib()
        self._b = self._L.wvg_batch_new(_context(), int(chunk_frames))
        if not self._b:
            raise RuntimeError("wvg_batch_new failed")
        self.infos: list = []
        self._dev_infos: list = []  # indices of device-framed files (their infos come with the upload)
        self._uploaded = False
        self._planar_fixed = 0  # fixed_frames of the last planar(out=None)
        self._resample_key = (1, 0)  # (out_rate, fixed_frames) of the last resample(out=None)
        self._data: list = []

    def add_file(self, data: bytes, open_flags: int = 0, start_sample: int | None = None, wvc: bytes | None = None):
        """Frame one file; with start_sample, as a caller that calls SetSample(start_sample)
        right after WavpackOpenFileInput (WavPackUtils.cs:509-594).  wvc: the hybrid file's
        .wvc correction file -- its hybrid blocks then decode exactly (beyond the reference)."""
        info = _L.WvgFileInfo()
        if wvc is not None:
            if start_sample is not None:
                raise ValueError("wvc with start_sample is not supported")
            idx = self._L.wvg_batch_add_file_wvc(self._b, data, len(data), wvc, len(wvc), int(open_flags),
                                                 ctypes.byref(info))
        elif start_sample is None:
            idx = self._L.wvg_batch_add_file(self._b, data, len(data), int(open_flags), ctypes.byref(info))
        else:
            idx = self._L.wvg_batch_add_file_at(self._b, data, len(data), int(open_flags), int(start_sample),
                                                ctypes.byref(info))
        # the C side reserves a file slot on success and on WVG_ERR_OPEN (an input that
        # does not open); any other negative code reserved nothing, so infos[i] must
        # not grow either (it mirrors the C file index i)
        if idx < 0 and idx != _L.WVG_ERR_OPEN:
            self._check(idx)
        self.infos.append(info)
        self._uploaded = False
        return idx

    def reset(self):
        """Drop every file, keep the device and page-locked buffers (wvg_batch_reset)."""
        self._check(self._L.wvg_batch_reset(self._b))
        self.infos = []
        self._dev_infos = []
        self._uploaded = False

    def add_files(self, files, open_flags: int = 0, threads: int = 0):
        """Frame many files on host threads (wvg_batch_add_files); returns their indices."""
        n = len(files)
        if n == 0:
            return []
        bufs, ptrs, lens = _file_arrays(files)
        infos = (_L.WvgFileInfo * n)()
        idx = np.empty(n, dtype=np.int32)
        rc = self._L.wvg_batch_add_files(self._b, n, ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data,
                                         int(open_flags), int(threads), ctypes.cast(infos, ctypes.c_void_p),
                                         idx.ctypes.data)
        if rc < 0:
            self._check(rc)
        self.infos.extend(infos)
        self._uploaded = False
        return idx.tolist()

    def add_files_device(self, files):
        """Queue files for device-side framing at the next upload
        (wvg_batch_add_files_device); returns their indices.  Their infos are
        filled in by upload()."""
        n = len(files)
        if n == 0:
            return []
        bufs, ptrs, lens = _file_arrays(files)
        idx = np.empty(n, dtype=np.int32)
        rc = self._L.wvg_batch_add_files_device(self._b, n, ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data,
                                                idx.ctypes.data)
        if rc < 0:
            self._check(rc)
        self._dev_infos.extend(range(len(self.infos), len(self.infos) + n))
        self.infos.extend(_L.WvgFileInfo() for _ in range(n))
        self._uploaded = False
        return idx.tolist()

    def framing_stats(self):
        """(files framed on the device, files framed by the host fallback)"""
        dev, host = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.wvg_batch_framing_stats(self._b, ctypes.byref(dev), ctypes.byref(host)))
        return int(dev.value), int(host.value)

    def lane_groups(self) -> int:
        """Diagnostics: the launch groups the last decode ran on lane / row kernels (bit t:
        PCM term set t; 8 .wvc; 9 DSD mode 3; 10 DSD mode 1) -- wvg_batch_lane_groups."""
        m = ctypes.c_uint32()
        self._check(self._L.wvg_batch_lane_groups(self._b, ctypes.byref(m)))
        return int(m.value)

    def upload(self):
        self._check(self._L.wvg_batch_upload(self._b))
        if self._dev_infos:  # device-framed files get their infos here (one call for the lot)
            lo, hi = min(self._dev_infos), max(self._dev_infos) + 1
            arr = (_L.WvgFileInfo * (hi - lo))()
            got = self._L.wvg_batch_file_infos(self._b, lo, hi - lo, ctypes.cast(arr, ctypes.c_void_p))
            for i in self._dev_infos:
                if i - lo < got:
                    self.infos[i] = arr[i - lo]
            self._dev_infos = []
        self._uploaded = True

    def decode(self, stream=None):
        if not self._uploaded:
            self.upload()
        self._check(self._L.wvg_batch_decode(self._b, stream))

    def sync(self):
        self._check(self._L.wvg_batch_sync(self._b))

    def poison(self, byte: int = 0x7F):
        """Overwrite the output with `byte` and mark every decodable block's status
        WVG_ST_UNWRITTEN (wvg_batch_poison): what a later download shows was written by
        the decodes issued after this call."""
        if not self._uploaded:
            self.upload()
        self._check(self._L.wvg_batch_poison(self._b, int(byte)))

    def set_kernel(self, kernel: str):
        """'auto' (the default: the lane kernels once the context has had batches in
        flight together, until then one workgroup per block for groups of up to 2,048
        blocks), 'lane' (one lane per
        block: the most blocks per second with batches in flight) or 'two_wave' (one
        workgroup per block: lowest latency for a batch alone) -- wvg_batch_set_kernel;
        results are identical in every mode."""
        k = {"two_wave": _L.WVG_KERNEL_TWO_WAVE, "lane": _L.WVG_KERNEL_LANE, "auto": _L.WVG_KERNEL_AUTO}[kernel]
        self._check(self._L.wvg_batch_set_kernel(self._b, k))

    def set_timing(self, on: bool = True):
        """Record a device event pair around every following decode (wvg_batch_set_timing)."""
        self._check(self._L.wvg_batch_set_timing(self._b, int(bool(on))))

    def timed(self):
        """(mean ms, count) of the decodes recorded since set_timing(True)."""
        ms, n = ctypes.c_float(), ctypes.c_int()
        self._check(self._L.wvg_batch_timed(self._b, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def group_times(self):
        """With timing on: {group: ms from the last decode's start to the group's end}
        (groups: 'ts0'..'ts7' term sets, 'pcm' generic, 'dsd', 'dsd1')."""
        ms = (ctypes.c_float * 11)()
        rc = self._L.wvg_batch_group_times(self._b, ms, 11)
        if rc < 0:
            self._check(rc)
        names = [f"ts{i}" for i in range(8)] + ["pcm", "dsd", "dsd1"]
        return {n: round(float(v), 3) for n, v in zip(names, ms) if v >= 0}

    def time(self, iters: int) -> float:
        ms = ctypes.c_float()
        self._check(self._L.wvg_batch_time(self._b, int(iters), ctypes.byref(ms)))
        return float(ms.value)

    @property
    def out_ints(self) -> int:
        return int(self._L.wvg_batch_out_ints(self._b))

    @property
    def num_blocks(self) -> int:
        return int(self._L.wvg_batch_num_blocks(self._b))

    @property
    def frames(self) -> int:
        return int(self._L.wvg_batch_frames(self._b))

    @property
    def bytes_in(self) -> int:
        return int(self._L.wvg_batch_bytes_in(self._b))

    def device_out_ptr(self) -> int:
        return int(self._L.wvg_batch_device_out(self._b) or 0)

    def download(self, pinned: bool = False) -> np.ndarray:
        """The int32 output.  pinned=True: DMA into the batch's page-locked buffer and
        return a view of it (valid until the next download or close)."""
        if pinned:
            self._check(self._L.wvg_batch_download(self._b, None, -1))
            p = self._L.wvg_batch_host_out(self._b)
            n = self.out_ints
            if not p or n == 0:
                return np.zeros(0, dtype=np.int32)
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)), shape=(n,))
        out = np.empty(max(self.out_ints, 1), dtype=np.int32)
        self._check(self._L.wvg_batch_download(self._b, out.ctypes.data, out.size))
        return out[: self.out_ints]

    def block_status(self) -> np.ndarray:
        n = self.num_blocks + 1024
        st = np.zeros(n, dtype=np.uint32)
        k = self._L.wvg_batch_block_status(self._b, st.ctypes.data, n)
        if k < 0:
            raise RuntimeError("block status unavailable (download first)")
        return st[:k]

    def lane_counters(self, ts: int) -> np.ndarray:
        """Diagnostics (a batch made with WVG_LANE_COUNTERS=1): per parser wave of term set
        `ts`'s last lane decode [cycles, groups, bulk, norun, split, fast, checked, replay,
        wait_consumed, wait_loads, words, stage, 0...] (wvg_batch_lane_counters)."""
        buf = np.zeros(16 * 4096, dtype=np.uint32)
        k = self._L.wvg_batch_lane_counters(self._b, int(ts), buf.ctypes.data, buf.size)
        if k < 0:
            raise RuntimeError("lane counters unavailable (WVG_LANE_COUNTERS=1 before the batch is made)")
        return buf[: 16 * k].reshape(k, 16)

    def file_blocks(self, i: int):
        """(end_frame, status) per block of file i (wvg_batch_file_blocks)."""
        n = self.num_blocks + 1
        ends = np.zeros(n, dtype=np.int64)
        st = np.zeros(n, dtype=np.uint32)
        k = self._L.wvg_batch_file_blocks(self._b, int(i), ends.ctypes.data, st.ctypes.data, n)
        if k < 0:
            raise RuntimeError("file blocks unavailable (download first)")
        return ends[:k], st[:k]

    def file_streams(self, i: int):
        """(widths, channel_mask) of file i (wvg_batch_file_streams): the ints a frame of each
        stream of a file opened with OPEN_ALL_CHANNELS, in channel order; ([its width],
        the default mask) for an ordinary file."""
        w = np.zeros(256, dtype=np.int32)
        mask = ctypes.c_uint32()
        n = self._L.wvg_batch_file_streams(self._b, int(i), w.ctypes.data, w.size, ctypes.byref(mask))
        if n < 0:
            self._check(n)
        return w[:n].tolist(), int(mask.value)

    def format(self, dsd: bool = False, stream=None):
        """WavpackFormatSamples (WavPackUtils.cs:288-341) over the decoded batch, on the device."""
        self._check(self._L.wvg_batch_format(self._b, int(bool(dsd)), stream))

    def pcm_offset(self, i: int) -> int:
        return int(self._L.wvg_batch_pcm_offset(self._b, int(i)))

    def download_pcm_async(self):
        """Queue the PCM download into the batch's page-locked buffer behind the format
        (wvg_batch_download_pcm_async); after sync(), host_pcm() is the image."""
        self._check(self._L.wvg_batch_download_pcm_async(self._b))

    def host_pcm(self) -> np.ndarray:
        """The page-locked PCM image of the last pinned / async download (a view)."""
        n = int(self._L.wvg_batch_pcm_bytes(self._b))
        p = self._L.wvg_batch_host_pcm(self._b)
        if not p or n == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))

    def download_pcm(self, pinned: bool = False) -> np.ndarray:
        """The formatted PCM bytes.  pinned=True: DMA into the batch's page-locked
        buffer and return a view of it (valid until the next such download or close)."""
        n = int(self._L.wvg_batch_pcm_bytes(self._b))
        if pinned:
            self._check(self._L.wvg_batch_download_pcm(self._b, None, -1))
            p = self._L.wvg_batch_host_pcm(self._b)
            if not p or n == 0:
                return np.zeros(0, dtype=np.uint8)
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))
        out = np.empty(max(n, 1), dtype=np.uint8)
        self._check(self._L.wvg_batch_download_pcm(self._b, out.ctypes.data, out.size))
        return out[:n]

    def md5(self, stream=None):
        """Hash every file's decoded audio on the device (wvg_batch_md5), after the whole of
        the last decode; needs neither format() nor a download and returns without
        waiting -- sync() covers it."""
        self._check(self._L.wvg_batch_md5(self._b, stream))

    def file_md5(self, i: int) -> _L.WvgFileMd5:
        """File i's digest, stored sum and verdict (wvg_batch_file_md5; after sync())."""
        r = _L.WvgFileMd5()
        self._check(self._L.wvg_batch_file_md5(self._b, int(i), ctypes.byref(r)))
        return r

    def planar_floats(self, fixed_frames: int = 0) -> int:
        """Floats of the planar image for fixed_frames (wvg_batch_planar_floats)."""
        n = int(self._L.wvg_batch_planar_floats(self._b, int(fixed_frames)))
        if n < 0:
            raise ValueError("fixed_frames must be >= 0")
        return n

    def file_planar(self, i: int, fixed_frames: int = 0):
        """(offset, row_stride, channels, frames) of file i in the planar image
        (wvg_batch_file_planar); offset -1 for a file that is not convertible (it did not
        open, or it is DSD opened without OPEN_DSD_AS_PCM)."""
        off, rs, fr = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        ch = ctypes.c_int32()
        rc = self._L.wvg_batch_file_planar(self._b, int(i), int(fixed_frames), ctypes.byref(off), ctypes.byref(rs),
                                           ctypes.byref(ch), ctypes.byref(fr))
        if rc < 0 and rc != _L.WVG_ERR_OPEN:
            self._check(rc)
        return int(off.value), int(rs.value), int(ch.value), int(fr.value)

    def planar(self, fixed_frames: int = 0, out=None, stream=None):
        """The decoded batch as planar float32 in [-1, 1) on the device (wvg_batch_planar;
        the layout and the conversion: include/wvgpu.h), after decode(), on `stream`, without
        waiting -- sync() covers it.  fixed_frames 0: every file's rows at their own length
        (padded to a multiple of 4 floats); T > 0: rows of T frames, cut or zero-padded.
        out: a contiguous float32 torch tensor on the batch's device with room for
        planar_floats(fixed_frames) floats, or None for a buffer the batch owns
        (download_planar, device_planar_ptr).  Returns (offset, row_stride, channels,
        frames) per file, offset -1 for a file that is not convertible."""
        if not self._uploaded:
            self.upload()
        ptr, cap = None, 0
        if out is not None:
            torch = _torch()  # (only a caller that passes a tensor needs it)
            if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or \
                    not out.is_contiguous():
                raise ValueError("out: a contiguous float32 torch tensor on the GPU")
            if out.device.index != context_device():
                raise ValueError(f"out is on {out.device}, the batch decodes on device {context_device()}")
            ptr, cap = ctypes.c_void_p(out.data_ptr()), out.numel()
        rc = self._L.wvg_batch_planar(self._b, int(fixed_frames), ptr, cap, stream)
        if rc == _L.WVG_ERR_SPACE:
            raise ValueError(f"out holds {cap} floats, the image needs {self.planar_floats(fixed_frames)}")
        if rc == _L.WVG_ERR_ARG and int(fixed_frames) < 0:
            raise ValueError("fixed_frames must be >= 0")
        self._check(rc)
        if out is None:
            self._planar_fixed = int(fixed_frames)
        return [self.file_planar(i, fixed_frames) for i in range(len(self.infos))]

    def device_planar_ptr(self) -> int:
        """Device pointer of the batch-owned planar image (the last planar(out=None))."""
        return int(self._L.wvg_batch_device_planar(self._b) or 0)

    def download_planar(self) -> np.ndarray:
        """The batch-owned planar image of the last planar(out=None), as a flat float32
        array (wvg_batch_download_planar; waits for it)."""
        n = self.planar_floats(self._planar_fixed)
        out = np.empty(max(n, 1), dtype=np.float32)
        self._check(self._L.wvg_batch_download_planar(self._b, out.ctypes.data, out.size))
        return out[:n]

    def resample_floats(self, out_rate: int, fixed_frames: int = 0) -> int:
        """Floats of the resampled image for (out_rate, fixed_frames) (wvg_batch_resample_floats)."""
        n = int(self._L.wvg_batch_resample_floats(self._b, int(out_rate), int(fixed_frames)))
        if n < 0:
            raise ValueError("out_rate must be in 1..2^31-1 and fixed_frames >= 0")
        return n

    def file_resample(self, i: int, out_rate: int, fixed_frames: int = 0):
        """(offset, row_stride, channels, frames) of file i in the resampled image
        (wvg_batch_file_resample), frames at out_rate; offset -1 for a file that is not
        resamplable (it did not open, it is DSD opened without OPEN_DSD_AS_PCM or an exact-float decode, it has no sample
        rate, or its rate pair is not supported)."""
        off, rs, fr = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        ch = ctypes.c_int32()
        rc = self._L.wvg_batch_file_resample(self._b, int(i), int(out_rate), int(fixed_frames), ctypes.byref(off),
                                             ctypes.byref(rs), ctypes.byref(ch), ctypes.byref(fr))
        if rc == _L.WVG_ERR_ARG and not (1 <= int(out_rate) < 2 ** 31 and int(fixed_frames) >= 0):
            raise ValueError("out_rate must be in 1..2^31-1 and fixed_frames >= 0")
        if rc < 0 and rc != _L.WVG_ERR_OPEN:
            self._check(rc)
        return int(off.value), int(rs.value), int(ch.value), int(fr.value)

    def resample(self, out_rate: int, fixed_frames: int = 0, out=None, stream=None):
        """The decoded batch as planar float32 in [-1, 1) at one sample rate on the device
        (wvg_batch_resample; the filter, the layout and the conversion: include/wvgpu.h),
        after decode(), on `stream`, without waiting -- sync() covers it.  The mirror of
        planar(): fixed_frames 0 gives every file's rows at their own resampled length
        (padded to a multiple of 4 floats), T > 0 rows of T frames at out_rate, cut or
        zero-padded.  out: a contiguous float32 torch tensor on the batch's device with room
        for resample_floats(out_rate, fixed_frames) floats, or None for a buffer the batch
        owns (download_resampled, device_resampled_ptr).  Returns (offset, row_stride,
        channels, frames) per file, offset -1 for a file that is not resamplable."""
        if not (1 <= int(out_rate) < 2 ** 31) or int(fixed_frames) < 0:
            raise ValueError("out_rate must be in 1..2^31-1 and fixed_frames >= 0")
        if not self._uploaded:
            self.upload()
        ptr, cap = None, 0
        if out is not None:
            torch = _torch()  # (only a caller that passes a tensor needs it)
            if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or \
                    not out.is_contiguous():
                raise ValueError("out: a contiguous float32 torch tensor on the GPU")
            if out.device.index != context_device():
                raise ValueError(f"out is on {out.device}, the batch decodes on device {context_device()}")
            ptr, cap = ctypes.c_void_p(out.data_ptr()), out.numel()
        rc = self._L.wvg_batch_resample(self._b, int(out_rate), int(fixed_frames), ptr, cap, stream)
        if rc == _L.WVG_ERR_SPACE:
            raise ValueError(f"out holds {cap} floats, the image needs {self.resample_floats(out_rate, fixed_frames)}")
        self._check(rc)
        if out is None:
            self._resample_key = (int(out_rate), int(fixed_frames))
        return [self.file_resample(i, out_rate, fixed_frames) for i in range(len(self.infos))]

    def device_resampled_ptr(self) -> int:
        """Device pointer of the batch-owned resampled image (the last resample(out=None))."""
        return int(self._L.wvg_batch_device_resampled(self._b) or 0)

    def download_resampled(self) -> np.ndarray:
        """The batch-owned image of the last resample(out=None), as a flat float32 array
        (wvg_batch_download_resampled; waits for it)."""
        n = self.resample_floats(*self._resample_key)
        out = np.empty(max(n, 1), dtype=np.float32)
        self._check(self._L.wvg_batch_download_resampled(self._b, out.ctypes.data, out.size))
        return out[:n]

    def levels(self, threshold_q31: int = 0, stream=None):
        """Every measurable file's per-channel level statistics on the device
        (wvg_batch_levels; the fields: include/wvgpu.h), after decode(), on `stream`, without
        waiting -- sync() covers it.  threshold_q31: the silence threshold in Q31 full-scale
        units (0 .. 0x7FFFFFFF), shifted down to each file's depth."""
        threshold_q31 = int(threshold_q31)
        if not 0 <= threshold_q31 <= 0x7FFFFFFF:
            raise ValueError("threshold_q31 must be in 0..0x7FFFFFFF")
        if not self._uploaded:
            self.upload()
        self._check(self._L.wvg_batch_levels(self._b, threshold_q31, stream))

    def file_levels(self, i: int):
        """File i's records of the last levels() (wvg_batch_file_levels; after sync()): a
        structured array (_lib.LEVELS_DTYPE) of one record per channel, or None for a file
        that is not measurable (it did not open, it is DSD opened without OPEN_DSD_AS_PCM, or it is a float file decoded
        under OPEN_EXACT_FLOAT)."""
        n = self._L.wvg_batch_file_levels(self._b, int(i), None, 0)
        if n == _L.WVG_ERR_OPEN:
            return None
        if n < 0:
            self._check(n)
        out = np.zeros(n, dtype=_L.LEVELS_DTYPE)
        got = self._L.wvg_batch_file_levels(self._b, int(i), out.ctypes.data, n)
        if got != n:
            self._check(got if got < 0 else _L.WVG_ERR_ARG)
        return out

    def true_peak(self, oversample: int = 0, stream=None):
        """Every measurable file's per-channel true peak (ITU-R BS.1770 Annex 2) on the device
        (wvg_batch_true_peak; the definition: include/wvgpu.h), after decode(), on `stream`,
        without waiting -- sync() covers it.  oversample: 1, 2 or 4, or 0 for each file's own
        factor by its sample rate (4 below 96,000, 2 below 192,000, else 1)."""
        oversample = int(oversample)
        if oversample not in (0, 1, 2, 4):
            raise ValueError("oversample must be 0, 1, 2 or 4")
        if not self._uploaded:
            self.upload()
        self._check(self._L.wvg_batch_true_peak(self._b, oversample, stream))

    def file_true_peak(self, i: int):
        """File i's records of the last true_peak() (wvg_batch_file_true_peak; after sync()): a
        structured array (_lib.TRUE_PEAK_DTYPE) of one record per channel, or None for a file
        that is not measurable (levels' rule)."""
        n = self._L.wvg_batch_file_true_peak(self._b, int(i), None, 0)
        if n == _L.WVG_ERR_OPEN:
            return None
        if n < 0:
            self._check(n)
        out = np.zeros(n, dtype=_L.TRUE_PEAK_DTYPE)
        got = self._L.wvg_batch_file_true_peak(self._b, int(i), out.ctypes.data, n)
        if got != n:
            self._check(got if got < 0 else _L.WVG_ERR_ARG)
        return out

    def loudness(self, stream=None):
        """Every measurable file's integrated loudness (ITU-R BS.1770) on the device
        (wvg_batch_loudness; the definition: include/wvgpu.h), after decode(), on `stream`,
        without waiting -- sync() covers it."""
        if not self._uploaded:
            self.upload()
        self._check(self._L.wvg_batch_loudness(self._b, stream))

    def file_loudness(self, i: int):
        """File i's record of the last loudness() (wvg_batch_file_loudness; after sync()): one
        element of a structured array (_lib.LOUDNESS_DTYPE), or None for a file that is not
        measurable (levels' rule, or a sample rate outside 6,000 .. 3,072,000)."""
        out = np.zeros(1, dtype=_L.LOUDNESS_DTYPE)
        rc = self._L.wvg_batch_file_loudness(self._b, int(i), out.ctypes.data)
        if rc == _L.WVG_ERR_OPEN:
            return None
        self._check(rc)
        return out[0]

    def download_loudness_blocks(self) -> np.ndarray:
        """The block image of the last loudness(): every measurable file's block powers P_j,
        file after file, as float64 (wvg_batch_download_loudness_blocks; waits for it)."""
        n = self._L.wvg_batch_loudness_blocks(self._b)
        if n < 0:
            self._check(n)
        out = np.zeros(max(n, 1), dtype=np.float64)
        self._check(self._L.wvg_batch_download_loudness_blocks(self._b, out.ctypes.data, out.size))
        return out[:n]

    def loudness_blocks(self, i: int):
        """File i's block powers of the last loudness() (float64, one per 400 ms block every
        100 ms), or None for a file that is not measurable.  Downloads the whole image: a
        caller that wants many files' takes download_loudness_blocks() once and slices it by
        the records' block_offset and blocks."""
        rec = self.file_loudness(i)
        if rec is None:
            return None
        o, n = int(rec["block_offset"]), int(rec["blocks"])
        return self.download_loudness_blocks()[o: o + n].copy()

    def loudness_range(self, stream=None):
        """Every measurable file's loudness range and short-term series (EBU Tech 3342) on the
        device (wvg_batch_loudness_range; the definition: include/wvgpu.h), after decode(), on
        `stream`, without waiting -- sync() covers it.  Where no loudness() was issued since
        the last decode() it is issued first, and file_loudness() is readable too."""
        if not self._uploaded:
            self.upload()
        self._check(self._L.wvg_batch_loudness_range(self._b, stream))

    def file_loudness_range(self, i: int):
        """File i's record of the last loudness_range() (wvg_batch_file_loudness_range; after
        sync()): one element of a structured array (_lib.LOUDNESS_RANGE_DTYPE), or None for a
        file that is not measurable (loudness's rule)."""
        out = np.zeros(1, dtype=_L.LOUDNESS_RANGE_DTYPE)
        rc = self._L.wvg_batch_file_loudness_range(self._b, int(i), out.ctypes.data)
        if rc == _L.WVG_ERR_OPEN:
            return None
        self._check(rc)
        return out[0]

    def download_loudness_shorts(self) -> np.ndarray:
        """The short-term image of the last loudness_range(): every measurable file's short-term
        powers ST_j, file after file, as float64 (wvg_batch_download_loudness_shorts; waits
        for it)."""
        n = self._L.wvg_batch_loudness_shorts(self._b)
        if n < 0:
            self._check(n)
        out = np.zeros(max(n, 1), dtype=np.float64)
        self._check(self._L.wvg_batch_download_loudness_shorts(self._b, out.ctypes.data, out.size))
        return out[:n]

    def loudness_shorts(self, i: int):
        """File i's short-term powers of the last loudness_range() (float64, one per 3 s window
        every 100 ms), or None for a file that is not measurable.  Downloads the whole image:
        a caller that wants many files' takes download_loudness_shorts() once and slices it
        by the records' short_offset and shorts."""
        rec = self.file_loudness_range(i)
        if rec is None:
            return None
        o, n = int(rec["short_offset"]), int(rec["shorts"])
        return self.download_loudness_shorts()[o: o + n].copy()

    def wav(self, i: int):
        """WvDemo.Main for file i (WvDemo.cs:15-168): (exit_code, .wav bytes)."""
        n, rc = ctypes.c_int64(), ctypes.c_int32()
        self._check(self._L.wvg_batch_wav(self._b, int(i), None, 0, ctypes.byref(n), ctypes.byref(rc)))
        buf = np.empty(max(n.value, 1), dtype=np.uint8)
        self._check(self._L.wvg_batch_wav(self._b, int(i), buf.ctypes.data, buf.size, ctypes.byref(n), ctypes.byref(rc)))
        return int(rc.value), buf[: n.value].tobytes()

    def result(self, i: int) -> _L.WvgFileResult:
        r = _L.WvgFileResult()
        self._check(self._L.wvg_batch_file_result(self._b, int(i), ctypes.byref(r)))
        return r

    def _check(self, rc: int):
        if rc == _L.WVG_ERR_TIMEOUT:
            raise DecoderTimeout(self._L.wvg_last_error(_context()).decode())
        if rc != 0:
            raise RuntimeError(f"libwvgpu error {rc}: {self._L.wvg_last_error(_context()).decode()}")

    def close(self):
        if self._b:
            self._L.wvg_batch_free(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WavpackContext:
    """Opaque context (WavpackContext.cs:13-35) over a wvg_stream: the file is decoded
    on the device by the first WavpackUnpackSamples call and served a window at a
    time, so host memory holds the compressed file and two windows, not the output."""

    def __init__(self, data: bytes, open_flags: int, window_frames: int = 0):
        self._data = data
        self._flags = open_flags
        self._window = int(window_frames)
        self._info = _L.WvgFileInfo()
        self._s = None
        self.error_message = None

    def _stream(self):
        if self._s is None:
            self._s = _L.lib().wvg_stream_open(_context(), self._data, len(self._data), int(self._flags),
                                               self._window, ctypes.byref(self._info))
            if not self._s:
                raise RuntimeError("wvg_stream_open failed: " + _L.lib().wvg_last_error(_context()).decode())
        return self._s

    def _state(self):
        idx, err = ctypes.c_int64(), ctypes.c_int64()
        lossy, changed = ctypes.c_int32(), ctypes.c_int32()
        _L.lib().wvg_stream_state(self._stream(), ctypes.byref(idx), ctypes.byref(err), ctypes.byref(lossy),
                                  ctypes.byref(changed))
        return int(idx.value), int(err.value), bool(lossy.value), bool(changed.value)

    @property
    def schedule_changed(self) -> bool:
        return self._state()[3] if self._s else False

    def close(self):
        if self._s:
            _L.lib().wvg_stream_close(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def WavpackOpenFileInput(reader, flags: int = 0, window_frames: int = 0) -> WavpackContext:
    """WavPackUtils.cs:36-120.  `reader` is bytes or a binary file object."""
    data = reader if isinstance(reader, (bytes, bytearray, memoryview)) else reader.read()
    data = bytes(data)
    wpc = WavpackContext(data, flags, window_frames)
    L = _L.lib()
    rc = L.wvg_probe_file(data, len(data), int(flags), SAMPLE_BUFFER_SIZE, ctypes.byref(wpc._info))  # host only
    if rc < 0 or not wpc._info.open_ok:
        wpc.error_message = wpc._info.error.decode() or "not compatible with this version of WavPack file!"
    return wpc


def WavpackUnpackSamples(wpc: WavpackContext, buffer: np.ndarray, samples: int) -> int:
    """WavPackUtils.cs:200-282: fill `buffer` (int32, >= samples * reduced channels)."""
    if wpc.error_message:
        return 0
    nch = max(int(wpc._info.reduced_channels), 1)
    if buffer.dtype != np.int32 or not buffer.flags.c_contiguous or buffer.size < int(samples) * nch:
        raise ValueError("buffer: contiguous int32 of samples x reduced channels")
    n = _L.lib().wvg_stream_unpack(wpc._stream(), buffer.ctypes.data, int(samples))
    if n == _L.WVG_ERR_EXCEPTION:
        raise WavpackException("the reference decoder raises an exception in this call")
    if n == _L.WVG_ERR_TIMEOUT:
        raise DecoderTimeout(_L.lib().wvg_last_error(_context()).decode())
    if n < 0:
        raise RuntimeError(f"libwvgpu error {n}: {_L.lib().wvg_last_error(_context()).decode()}")
    return int(n)


def SetSample(wpc: WavpackContext, sample: int) -> bool:
    """WavPackUtils.cs:509-594.  The block search runs on the host framing; the file
    is then decoded from the block the reference's search lands on (its discard
    calls included), and the result is the C# return value.  (After samples were
    already handed out, the block search of the reference starts from the current
    block; for well-formed files it ends on the same block, which is what this
    mirror decodes from.)"""
    if wpc.error_message:
        return False
    rc = _L.lib().wvg_stream_set_sample(wpc._stream(), int(sample))
    if rc == _L.WVG_ERR_EXCEPTION:
        raise WavpackException("the reference's SetSample raises an exception on this file")
    if rc == _L.WVG_ERR_TIMEOUT:
        raise DecoderTimeout(_L.lib().wvg_last_error(_context()).decode())
    if rc < 0:
        raise RuntimeError(f"libwvgpu error {rc}: {_L.lib().wvg_last_error(_context()).decode()}")
    return rc == 1


def SetTime(wpc: WavpackContext, milliseconds: int) -> bool:
    """WavPackUtils.cs:504-507: SetSample(ms / 1000 * sample_rate) (integer division first)."""
    return SetSample(wpc, int(milliseconds) // 1000 * int(wpc._info.sample_rate))


def WavpackFormatSamples(src: np.ndarray, samcnt: int, bps: int, pcm_buffer: bytearray, offset: int = 0,
                         dsd: bool = False) -> bool:
    """WavPackUtils.cs:288-341 (host C implementation in libwvgpu)."""
    L = _L.lib()
    s = np.ascontiguousarray(src, dtype=np.int32)
    if pcm_buffer is None or len(pcm_buffer) < int(samcnt) * int(bps) + int(offset):
        return False
    if int(bps) in (1, 2, 3, 4) and int(samcnt) > s.size:  # src[counter2++] past the array
        raise WavpackException("IndexOutOfRangeException in WavpackFormatSamples")
    view = (ctypes.c_uint8 * len(pcm_buffer)).from_buffer(pcm_buffer)
    return bool(L.wvg_format_samples(s.ctypes.data, int(samcnt), int(bps), ctypes.addressof(view), len(pcm_buffer),
                                     int(offset), int(bool(dsd))))


def wv_demo(data: bytes):
    """WvDemo.Main (WvDemo.cs:15-168) on the GPU path: (exit_code, .wav bytes).

    Decode (WavpackUnpackSamples calls of SAMPLE_BUFFER_SIZE frames), the
    WavpackFormatSamples epilogue on the device, then the header / PCM /
    trailer layout WvDemo writes."""
    b = DecodeBatch(SAMPLE_BUFFER_SIZE)
    try:
        idx = b.add_file(bytes(data))
        if idx < 0:
            return 1, b""
        b.decode()
        b.format(dsd=False)
        return b.wav(idx)
    finally:
        b.close()


MD5_NONE, MD5_MATCH, MD5_MISMATCH, MD5_NOT_COMPARABLE = (_L.WVG_MD5_NONE, _L.WVG_MD5_MATCH, _L.WVG_MD5_MISMATCH,
                                                         _L.WVG_MD5_NOT_COMPARABLE)


def probe_md5(data: bytes):
    """The MD5 sum a .wv file stores (ID_MD5_CHECKSUM; host only, wvg_probe_file_md5):
    16 bytes, None when it stores none; ValueError when the file does not open."""
    data = bytes(data)
    out = (ctypes.c_uint8 * 16)()
    rc = _L.lib().wvg_probe_file_md5(data, len(data), out)
    if rc < 0:
        raise ValueError("the file does not open")
    return bytes(out) if rc == 1 else None


def probe_streams(data: bytes):
    """(widths, channel_mask) of a file opened with OPEN_ALL_CHANNELS (host only,
    wvg_probe_file_streams); ValueError when the file does not open."""
    data = bytes(data)
    w = np.zeros(256, dtype=np.int32)
    mask = ctypes.c_uint32()
    n = _L.lib().wvg_probe_file_streams(data, len(data), w.ctypes.data, w.size, ctypes.byref(mask))
    if n < 0:
        raise ValueError("the file does not open")
    return w[:n].tolist(), int(mask.value)


def interleave_tile_frames(channels: int) -> int:
    """Frames of one tile of the interleave kernel for a channel count (wv_mc.h)."""
    t = _L.lib().wvg_interleave_tile_frames(int(channels))
    if t < 0:
        raise ValueError("channels must be in 1..255")
    return int(t)


def interleave_streams(streams, out: np.ndarray | None = None) -> np.ndarray:
    """The interleave kernel's tile code run on the host (wvg_interleave_streams): `streams`
    are int32 arrays of shape (frames, 1 or 2) (or (frames,) for one channel); returns
    (frames, sum of widths).  out: a flat int32 array to write into (frames x channels)."""
    arrs = [np.ascontiguousarray(s, dtype=np.int32) for s in streams]
    arrs = [a.reshape(-1, 1) if a.ndim == 1 else a for a in arrs]
    frames = arrs[0].shape[0]
    widths = np.array([a.shape[1] for a in arrs], dtype=np.int32)
    nch = int(widths.sum())
    if out is None:
        out = np.empty(frames * nch, dtype=np.int32)
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    rc = _L.lib().wvg_interleave_streams(ctypes.cast(ptrs, ctypes.c_void_p), widths.ctypes.data, len(arrs), frames,
                                         out.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_interleave_streams: {rc}")
    return out[: frames * nch].reshape(frames, nch)


def decode_all_channels(data: bytes, open_flags: int = 0) -> np.ndarray:
    """Decode one file with every channel (OPEN_ALL_CHANNELS): int32 of shape (frames, N)."""
    b = DecodeBatch(SAMPLE_BUFFER_SIZE)
    try:
        idx = b.add_file(bytes(data), int(open_flags) | OPEN_ALL_CHANNELS)
        if idx < 0:
            raise ValueError("the file does not open: " + b.infos[-1].error.decode(errors="replace"))
        b.decode()
        out = b.download()
        b.result(idx)
        info = b.infos[idx]
        n = info.out_frames * info.reduced_channels
        return out[info.out_offset: info.out_offset + n].reshape(-1, info.reduced_channels).copy()
    finally:
        b.close()


def planar_tile_frames(channels: int) -> int:
    """Frames of one tile of the planar-float kernel for a channel count (wv_planar.h)."""
    t = _L.lib().wvg_planar_tile_frames(int(channels))
    if t < 0:
        raise ValueError("channels must be in 1..255")
    return int(t)


def planar_float(src: np.ndarray, kind: int, row_len: int | None = None, row_stride: int | None = None,
                 out: np.ndarray | None = None) -> np.ndarray:
    """The planar-float kernel's tile code run on the host (wvg_planar_float): `src` is int32
    of shape (frames, channels); kind 7 / 15 / 23 / 31 scales by 2^-kind, 0 passes the bits
    through.  Returns float32 of shape (channels, row_stride) (row_len defaults to frames,
    row_stride to row_len).  out: a flat float32 array to write into."""
    a = np.ascontiguousarray(src, dtype=np.int32)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    frames, nch = a.shape
    row_len = frames if row_len is None else int(row_len)
    row_stride = row_len if row_stride is None else int(row_stride)
    if out is None:
        out = np.empty(max(nch * row_stride, 1), dtype=np.float32)
    rc = _L.lib().wvg_planar_float(a.ctypes.data, frames, nch, int(kind), row_len, row_stride, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_planar_float: {rc}")
    return out[: nch * row_stride].reshape(nch, row_stride)


def resample_filter(in_rate: int, out_rate: int):
    """The resampler's filter for a rate pair (wvg_resample_filter): (orig, new, width,
    float32 taps of shape [new, K]); ValueError for a pair that is not supported."""
    L = _L.lib()
    o, n, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    cnt = L.wvg_resample_filter(int(in_rate), int(out_rate), ctypes.byref(o), ctypes.byref(n), ctypes.byref(w), None, 0)
    if cnt < 0:
        raise ValueError(f"resample_filter: {in_rate} -> {out_rate} is not a supported pair")
    taps = np.empty(cnt, dtype=np.float32)
    cnt = L.wvg_resample_filter(int(in_rate), int(out_rate), None, None, None, taps.ctypes.data, taps.size)
    if cnt < 0:
        raise ValueError(f"wvg_resample_filter: {cnt}")
    return int(o.value), int(n.value), int(w.value), taps.reshape(int(n.value), -1)


def resample_tile_frames(in_rate: int, out_rate: int, channels: int) -> int:
    """Output frames of one job of the resample kernel for a rate pair and a channel count
    (wv_resample.h)."""
    t = _L.lib().wvg_resample_tile_frames(int(in_rate), int(out_rate), int(channels))
    if t < 0:
        raise ValueError("channels must be in 1..255 and the rate pair supported")
    return int(t)


def resample_float(src: np.ndarray, kind: int, in_rate: int, out_rate: int, row_len: int | None = None,
                   row_stride: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
    """The resample kernel's job builder and tile code run on the host (wvg_resample_float):
    `src` is int32 of shape (frames, channels) at in_rate; kind 7 / 15 / 23 / 31 scales by
    2^-kind.  Returns float32 of shape (channels, row_stride) at out_rate (row_len defaults
    to the resampled length ceil(frames * new / orig), row_stride to row_len).  out: a flat
    float32 array to write into."""
    a = np.ascontiguousarray(src, dtype=np.int32)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    frames, nch = a.shape
    if row_len is None:
        g = math.gcd(int(in_rate), int(out_rate)) if in_rate > 0 and out_rate > 0 else 1
        o, n = int(in_rate) // g, int(out_rate) // g
        row_len = -(-frames * n // o) if o else 0
    row_len = int(row_len)
    row_stride = row_len if row_stride is None else int(row_stride)
    if out is None:
        out = np.empty(max(nch * row_stride, 1), dtype=np.float32)
    rc = _L.lib().wvg_resample_float(a.ctypes.data, frames, nch, int(kind), int(in_rate), int(out_rate), row_len,
                                     row_stride, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_resample_float: {rc}")
    return out[: nch * row_stride].reshape(nch, row_stride)


def decode_to_tensors(files, open_flags: int = 0, fixed_frames: int = 0, sample_rate: int = 0):
    """Decode `files` into float32 torch tensors on the GPU, channels first, in [-1, 1):
    add, upload, decode and planar() on torch's current stream of the batch's device, into
    one flat tensor, with nothing downloaded.  fixed_frames 0: a list with a [C_i, T_i]
    view per file, None for a file that is not convertible (it did not open, or it is DSD
    opened without OPEN_DSD_AS_PCM).
    fixed_frames T > 0: (tensor [B, C, T], lengths) over the convertible files in file
    order, every file cut or zero-padded to T frames, lengths[i] = its frames in the
    tensor; ValueError when their channel counts differ.  Work queued on the same torch
    stream afterwards sees the tensors complete.  sample_rate R > 0: every file is
    resampled to R on the device (resample() in place of planar()); lengths and T count
    frames at R, and a file that is not resamplable is None or left out."""
    torch = _torch()  # lazily: the package imports without it
    fixed_frames, sample_rate = int(fixed_frames), int(sample_rate)
    if fixed_frames < 0:
        raise ValueError("fixed_frames must be >= 0")
    if sample_rate < 0 or sample_rate >= 2 ** 31:
        raise ValueError("sample_rate must be in 0..2^31-1")
    b = DecodeBatch(SAMPLE_BUFFER_SIZE)
    try:
        dev = torch.device("cuda", context_device())
        if len(files):
            b.add_files(files, open_flags)
        b.upload()
        if sample_rate:
            lay = [b.file_resample(i, sample_rate, fixed_frames) for i in range(len(b.infos))]
        else:
            lay = [b.file_planar(i, fixed_frames) for i in range(len(b.infos))]
        conv = [l for l in lay if l[0] >= 0]
        if fixed_frames and len({l[2] for l in conv}) > 1:
            raise ValueError("fixed_frames needs files of one channel count, got " +
                             str(sorted({l[2] for l in conv})))
        floats = b.resample_floats(sample_rate, fixed_frames) if sample_rate else b.planar_floats(fixed_frames)
        flat = torch.empty(floats, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        b.decode(stream)
        if sample_rate:
            b.resample(sample_rate, fixed_frames, out=flat, stream=stream)
        else:
            b.planar(fixed_frames, out=flat, stream=stream)
        if fixed_frames:
            nch = conv[0][2] if conv else 0
            return flat.view(len(conv), nch, fixed_frames), [l[3] for l in conv]
        return [None if off < 0 else flat[off: off + ch * rs].view(ch, rs)[:, :fr] for off, rs, ch, fr in lay]
    finally:
        b.close()  # (waits for the batch's work: the tensors are complete on return)


def verify_files(files, open_flags: int = 0) -> list:
    """Decode `files` and check each against its stored MD5 on the device: add, upload,
    decode, md5 and sync, with no PCM formatted or downloaded (16 bytes a file come
    back).  Returns one WvgFileMd5 per file (verdict MD5_*), None for a file that did
    not open."""
    if not len(files):
        return []
    b = DecodeBatch(SAMPLE_BUFFER_SIZE)
    try:
        idx = b.add_files(files, open_flags)
        b.decode()
        b.md5()
        b.sync()
        return [b.file_md5(i) if i >= 0 else None for i in idx]
    finally:
        b.close()


def dsd_pcm_taps():
    """The decimation filter of OPEN_DSD_AS_PCM (wvg_dsd_pcm_taps): (taps, sum, sum_abs) -- 104
    int32 taps over bits, oldest first, and their sums as Python ints.  The DC gain is
    sum / 2^23."""
    taps = np.zeros(104, dtype=np.int32)
    s, a = ctypes.c_int64(), ctypes.c_int64()
    rc = _L.lib().wvg_dsd_pcm_taps(taps.ctypes.data, ctypes.byref(s), ctypes.byref(a))
    if rc != 0:
        raise ValueError(f"wvg_dsd_pcm_taps: {rc}")
    return taps, int(s.value), int(a.value)


def dsd_pcm_tile_frames(channels: int) -> int:
    """Frames of one tile of the DSD-to-PCM kernel for a channel count (wv_dsdpcm.h)."""
    t = _L.lib().wvg_dsd_pcm_tile_frames(int(channels))
    if t < 0:
        raise ValueError("channels must be in 1..255")
    return int(t)


def dsd_pcm_ints(src: np.ndarray, out: np.ndarray | None = None) -> np.ndarray:
    """The DSD-to-PCM kernel's tile code run on the host (wvg_dsd_pcm_ints): `src` is int32 of
    shape (frames, channels) -- decoded DSD, one byte value per int, only the low 8 bits
    count; any int alignment -- and the result is int32 of the same shape, 24-bit PCM at the
    byte rate.  `out`: a C-contiguous int32 destination of that shape (not `src`)."""
    a = np.asarray(src)
    if a.dtype != np.int32:
        a = a.astype(np.int32)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    frames, nch = a.shape
    if out is None:
        out = np.zeros((frames, nch), dtype=np.int32)
    elif out.dtype != np.int32 or out.shape != (frames, nch) or not out.flags.c_contiguous:
        raise ValueError("out must be C-contiguous int32 of src's shape")
    rc = _L.lib().wvg_dsd_pcm_ints(a.ctypes.data, frames, nch, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_dsd_pcm_ints: {rc}")
    return out


def levels_tile_frames(channels: int) -> int:
    """Frames of one tile of the levels kernel for a channel count (wv_levels.h)."""
    t = _L.lib().wvg_levels_tile_frames(int(channels))
    if t < 0:
        raise ValueError("channels must be in 1..255")
    return int(t)


def levels_ints(src: np.ndarray, k: int, threshold_q31: int = 0) -> np.ndarray:
    """The levels kernels' tile and combine code run on the host (wvg_levels_ints): `src` is
    int32 of shape (frames, channels) -- any int alignment -- and full scale is 2^k (k 7 /
    15 / 23 / 31).  Returns one record (_lib.LEVELS_DTYPE) per channel."""
    a = np.asarray(src)
    if a.dtype != np.int32:
        a = a.astype(np.int32)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    frames, nch = a.shape
    threshold_q31 = int(threshold_q31)
    if not 0 <= threshold_q31 <= 0xFFFFFFFF:
        raise ValueError("threshold_q31 must be in 0..0x7FFFFFFF")
    out = np.zeros(max(nch, 1), dtype=_L.LEVELS_DTYPE)
    rc = _L.lib().wvg_levels_ints(a.ctypes.data, frames, nch, int(k), threshold_q31, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_levels_ints: {rc}")
    return out[:nch]


def _dbfs(x: float) -> float:
    return 20.0 * math.log10(x) if x > 0 else float("-inf")


def scan_levels(files, open_flags: int = 0, threshold_q31: int = 0) -> list:
    """Decode `files` and measure each channel's levels on the device: add, upload, decode,
    levels and sync, with no PCM formatted or downloaded (64 bytes a channel come back).
    Returns one dict per file, None for a file that is not measurable:
      records     the structured array of DecodeBatch.file_levels (exact integers)
      sumsq       per channel, sumsq_hi * 2^64 + sumsq_lo as a Python int
      k           full scale is 2^k
      out_frames  the frames measured
      peak_dbfs, rms_dbfs, dc   per channel, Python floats relative to full scale
                  (max(|min|, |max|) / 2^k and sqrt(sumsq / frames) / 2^k in dB, -inf for
                  silence; sum / frames / 2^k)
    The last three are conveniences derived here in floating point; they are not part of
    the exact contract the records keep."""
    if not len(files):
        return []
    b = DecodeBatch(SAMPLE_BUFFER_SIZE)
    try:
        idx = b.add_files(files, open_flags)
        b.decode()
        b.levels(threshold_q31)
        b.sync()
        res = []
        for i in idx:
            rec = b.file_levels(i) if i >= 0 else None
            if rec is None:
                res.append(None)
                continue
            info = b.infos[i]
            k = 23 if info.is_float else 8 * min(max(int(info.bytes_per_sample), 1), 4) - 1
            n, fs = int(info.out_frames), float(1 << k)
            sumsq = [(int(r["sumsq_hi"]) << 64) | int(r["sumsq_lo"]) for r in rec]
            res.append({
                "records": rec, "sumsq": sumsq, "k": k, "out_frames": n,
                "peak_dbfs": [_dbfs(max(-int(r["min"]), int(r["max"])) / fs) for r in rec],
                "rms_dbfs": [_dbfs(math.sqrt(q / n) / fs) if n else float("-inf") for q in sumsq],
                "dc": [int(r["sum"]) / n / fs if n else 0.0 for r in rec],
            })
        return res
    finally:
        b.close()


def true_peak_taps() -> np.ndarray:
    """The interpolator's integer taps (wvg_true_peak_taps): int32 of shape (4, 12), row q the
    quarter-phase q, scaled by 2^24."""
    t = np.zeros(48, dtype=np.int32)
    rc = _L.lib().wvg_true_peak_taps(t.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_true_peak_taps: {rc}")
    return t.reshape(4, 12)


def true_peak_oversample(rate: int) -> int:
    """The oversampling factor a sample rate gets (wvg_true_peak_oversample): 4, 2 or 1."""
    return int(_L.lib().wvg_true_peak_oversample(int(rate)))


def true_peak_tile_frames(channels: int) -> int:
    """Frames of one tile of the true-peak kernel for a channel count (wv_tpeak.h)."""
    t = _L.lib().wvg_true_peak_tile_frames(int(channels))
    if t < 0:
        raise ValueError("channels must be in 1..255")
    return int(t)


def true_peak_ints(src: np.ndarray, k: int, oversample: int) -> np.ndarray:
    """The true-peak kernels' tile and combine code run on the host (wvg_true_peak_ints):
    `src` is int32 of shape (frames, channels) -- any int alignment --, full scale is 2^k (k
    7 / 15 / 23 / 31) and oversample 1, 2 or 4.  Returns one record (_lib.TRUE_PEAK_DTYPE)
    per channel."""
    a = np.asarray(src)
    if a.dtype != np.int32:
        a = a.astype(np.int32)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    frames, nch = a.shape
    out = np.zeros(max(nch, 1), dtype=_L.TRUE_PEAK_DTYPE)
    rc = _L.lib().wvg_true_peak_ints(a.ctypes.data, frames, nch, int(k), int(oversample), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_true_peak_ints: {rc}")
    return out[:nch]


def _true_peak_dict(rec, info) -> dict:
    k, n = int(rec[0]["k"]), int(info.out_frames)
    fs, rate = float(1 << (k + 24)), float(info.sample_rate)
    tp = [int(r["true_peak"]) / fs for r in rec]
    dbtp = [_dbfs(x) for x in tp]
    return {
        "records": rec, "k": k, "out_frames": n,
        "true_peak": tp, "dbtp": dbtp,
        "sample_peak_dbfs": [_dbfs(int(r["sample_peak"]) / float(1 << k)) for r in rec],
        "overs": [int(r["overs"]) for r in rec],
        "position_s": [int(r["true_peak_pos"]) / int(r["oversample"]) / rate if int(r["true_peak_pos"]) >= 0 and rate > 0
                       else None for r in rec],
        "max_dbtp": max(dbtp),
    }


def scan_true_peak(files, open_flags: int = 0, oversample: int = 0) -> list:
    """Decode `files` and measure each channel's true peak on the device: add, upload, decode,
    true_peak and sync, with no PCM formatted or downloaded (48 bytes a channel come back).
    Returns one dict per file, None for a file that is not measurable:
      records     the structured array of DecodeBatch.file_true_peak (exact integers)
      k           full scale is 2^k
      out_frames  the frames measured
      true_peak, dbtp, sample_peak_dbfs, overs, position_s   per channel: peak / 2^(k+24) as
                  a float, that in dB (-inf for silence), the sample peak in dB, the outputs
                  above 0 dBTP, and (pos / O) / sample_rate in seconds (None for no frames)
      max_dbtp    the file's maximum of dbtp
    The floats are conveniences derived here in floating point; they are not part of the
    exact contract the records keep."""
    if not len(files):
        return []
    b = DecodeBatch(SAMPLE_BUFFER_SIZE)
    try:
        idx = b.add_files(files, open_flags)
        b.decode()
        b.true_peak(oversample)
        b.sync()
        res = []
        for i in idx:
            rec = b.file_true_peak(i) if i >= 0 else None
            res.append(None if rec is None else _true_peak_dict(rec, b.infos[i]))
        return res
    finally:
        b.close()


def loudness_filter(rate: int):
    """The K-weighting's coefficients at `rate` (wvg_loudness_filter): (float64 array b0 b1 b2
    a1 a2 c1 c2, step frames S)."""
    cf, s = np.zeros(7, dtype=np.float64), ctypes.c_int32()
    rc = _L.lib().wvg_loudness_filter(int(rate), cf.ctypes.data, ctypes.byref(s))
    if rc != 0:
        raise ValueError("rate must be in 6000..3072000")
    return cf, int(s.value)


def loudness_weights(channels: int, channel_mask: int) -> np.ndarray:
    """The channel weights G_c of a channel count and mask (wvg_loudness_weights)."""
    if not 1 <= int(channels) <= 255:
        raise ValueError("channels must be in 1..255")
    w = np.zeros(int(channels), dtype=np.float64)
    rc = _L.lib().wvg_loudness_weights(int(channels), int(channel_mask) & 0xFFFFFFFF, w.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_loudness_weights: {rc}")
    return w


def loudness_ints(src: np.ndarray, k: int, rate: int, channel_mask: int = 0):
    """The loudness kernels' code run on the host (wvg_loudness_ints): `src` is int32 of shape
    (frames, channels) -- any int alignment -- and full scale is 2^k (k 7 / 15 / 23 / 31).
    Returns (record, block powers): one element of _lib.LOUDNESS_DTYPE and a float64 array."""
    a = np.asarray(src)
    if a.dtype != np.int32:
        a = a.astype(np.int32)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    frames, nch = a.shape
    _, s = loudness_filter(rate)
    n = max(frames // s - 3, 0)
    rec, blocks = np.zeros(1, dtype=_L.LOUDNESS_DTYPE), np.zeros(max(n, 1), dtype=np.float64)
    rc = _L.lib().wvg_loudness_ints(a.ctypes.data, frames, nch, int(k), int(rate), int(channel_mask) & 0xFFFFFFFF,
                                    rec.ctypes.data, blocks.ctypes.data, n)
    if rc != 0:
        raise ValueError(f"wvg_loudness_ints: {rc}")
    return rec[0], blocks[:n]


def loudness_gate(blocks):
    """The gate code over any list of block powers (wvg_loudness_gate), an album's for one:
    one element of _lib.LOUDNESS_DTYPE with power, ungated_power, max_block_power and the
    three counts filled."""
    p = np.ascontiguousarray(np.asarray(blocks, dtype=np.float64).reshape(-1))
    rec = np.zeros(1, dtype=_L.LOUDNESS_DTYPE)
    rc = _L.lib().wvg_loudness_gate(p.ctypes.data if p.size else None, p.size, rec.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_loudness_gate: {rc}")
    return rec[0]


def loudness_range_ints(src: np.ndarray, k: int, rate: int, channel_mask: int = 0):
    """The loudness-range kernels' code run on the host (wvg_loudness_range_ints): `src` as
    loudness_ints takes it.  Returns (record, short-term powers): one element of
    _lib.LOUDNESS_RANGE_DTYPE and a float64 array."""
    a = np.asarray(src)
    if a.dtype != np.int32:
        a = a.astype(np.int32)
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    frames, nch = a.shape
    _, s = loudness_filter(rate)
    n = max(frames // s - 29, 0)
    rec, shorts = np.zeros(1, dtype=_L.LOUDNESS_RANGE_DTYPE), np.zeros(max(n, 1), dtype=np.float64)
    rc = _L.lib().wvg_loudness_range_ints(a.ctypes.data, frames, nch, int(k), int(rate),
                                          int(channel_mask) & 0xFFFFFFFF, rec.ctypes.data, shorts.ctypes.data, n)
    if rc != 0:
        raise ValueError(f"wvg_loudness_range_ints: {rc}")
    return rec[0], shorts[:n]


def loudness_range_gate(shorts):
    """The gates and the percentile selection over any list of short-term powers
    (wvg_loudness_range_gate), an album's for one: one element of _lib.LOUDNESS_RANGE_DTYPE
    with the four powers and the three counts filled."""
    p = np.ascontiguousarray(np.asarray(shorts, dtype=np.float64).reshape(-1))
    rec = np.zeros(1, dtype=_L.LOUDNESS_RANGE_DTYPE)
    rc = _L.lib().wvg_loudness_range_gate(p.ctypes.data if p.size else None, p.size, rec.ctypes.data)
    if rc != 0:
        raise ValueError(f"wvg_loudness_range_gate: {rc}")
    return rec[0]


def _power_lufs(p: float) -> float:
    return -0.691 + 10.0 * math.log10(p) if p > 0 else float("-inf")


def _range_fields(d: dict, rec) -> None:
    """the loudness-range record's fields and what R 128 calls them, into a scan_loudness dict"""
    for n in rec.dtype.names:
        d[n] = float(rec[n]) if rec.dtype[n].kind == "f" else int(rec[n])
    d["range_record"] = rec
    ok = d["gated_shorts"] > 0 and d["low_power"] > 0
    d["lra_lu"] = 10.0 * math.log10(d["high_power"] / d["low_power"]) if ok else 0.0
    d["lra_low_lufs"] = _power_lufs(d["low_power"])
    d["lra_high_lufs"] = _power_lufs(d["high_power"])
    d["max_short_term_lufs"] = _power_lufs(d["max_short_power"])
    d["max_momentary_lufs"] = _power_lufs(d["max_block_power"])


def _lufs_dict(rec, target_lufs: float) -> dict:
    d = {n: (float(rec[n]) if rec.dtype[n].kind == "f" else int(rec[n])) for n in rec.dtype.names}
    lufs = -0.691 + 10.0 * math.log10(d["power"]) if d["gated_blocks"] > 0 and d["power"] > 0 else float("-inf")
    d["record"] = rec
    d["lufs"] = lufs
    d["gain_db"] = None if lufs == float("-inf") else float(target_lufs) - lufs
    return d


def _clip_safe(d: dict, tp_dbtp: float) -> None:
    d["true_peak_dbtp"] = tp_dbtp
    d["clip_safe_gain_db"] = None if d["gain_db"] is None else min(d["gain_db"], -tp_dbtp)


def scan_loudness(files, open_flags: int = 0, target_lufs: float = -18.0, album: bool = False,
                  true_peak: bool = False, loudness_range: bool = False) -> list:
    """Decode `files` and measure each one's integrated loudness on the device: add, upload,
    decode, loudness and sync, with no PCM formatted or downloaded.  Returns one dict per
    file, None for a file that is not measurable: the record's fields by name (and `record`
    itself), `lufs` = -0.691 + 10 log10(power) (-inf when no block passed the gates) and
    `gain_db` = target_lufs - lufs (None for -inf).  With album=True one more dict follows:
    the gate (loudness_gate) over the block powers of all measurable files together -- block
    powers are normalised by their rate, so files of several rates mix.
    With true_peak=True the true peak (DecodeBatch.true_peak, each file's own oversampling
    factor) is queued on the same decode, and each dict gains `true_peak_dbtp`, the maximum
    over the file's channels, and `clip_safe_gain_db` = min(gain_db, -true_peak_dbtp) (None
    where gain_db is None); the album dict gains the maximum over the files.
    With loudness_range=True the loudness range (DecodeBatch.loudness_range, EBU Tech 3342) is
    queued on the same decode, and each dict gains that record's fields (and `range_record`),
    `lra_lu` = 10 log10(high_power / low_power) (0.0 when no short-term value passed the
    gates), `lra_low_lufs`, `lra_high_lufs`, `max_short_term_lufs` and `max_momentary_lufs`
    (from max_block_power), each -0.691 + 10 log10(power) or -inf; the album dict takes
    loudness_range_gate over the short-term powers of all measurable files together."""
    b = DecodeBatch(SAMPLE_BUFFER_SIZE)
    try:
        res, recs, peaks, ranges = [], [], [], []
        if len(files):
            idx = b.add_files(files, open_flags)
            b.decode()
            b.loudness()
            if loudness_range:
                b.loudness_range()
            if true_peak:
                b.true_peak(0)
            b.sync()
            for i in idx:
                rec = b.file_loudness(i) if i >= 0 else None
                recs.append(rec)
                res.append(None if rec is None else _lufs_dict(rec, target_lufs))
                if true_peak and rec is not None:
                    peaks.append(_true_peak_dict(b.file_true_peak(i), b.infos[i])["max_dbtp"])
                    _clip_safe(res[-1], peaks[-1])
                if loudness_range and rec is not None:
                    ranges.append(b.file_loudness_range(i))
                    _range_fields(res[-1], ranges[-1])
        if album:
            img = b.download_loudness_blocks() if any(r is not None for r in recs) else np.zeros(0)
            parts = [img[int(r["block_offset"]): int(r["block_offset"]) + int(r["blocks"])] for r in recs
                     if r is not None]
            res.append(_lufs_dict(loudness_gate(np.concatenate(parts) if parts else np.zeros(0)), target_lufs))
            if true_peak:
                _clip_safe(res[-1], max(peaks) if peaks else float("-inf"))
            if loudness_range:
                img = b.download_loudness_shorts() if ranges else np.zeros(0)
                parts = [img[int(r["short_offset"]): int(r["short_offset"]) + int(r["shorts"])] for r in ranges]
                _range_fields(res[-1], loudness_range_gate(np.concatenate(parts) if parts else np.zeros(0)))
        return res
    finally:
        b.close()


def WavpackGetNumSamples(wpc, native: bool = False) -> int:
    t = wpc._info.total_samples
    return t * 8 if native and wpc._info.dsd_multiplier > 0 else t


def WavpackGetSampleIndex(wpc) -> int:
    """stream.sample_index (WavPackUtils.cs:355-358): where the next call starts."""
    if wpc.error_message:
        return int(wpc._info.sample_index0)
    return wpc._state()[0]


def WavpackGetNumErrors(wpc) -> int:
    """crc_errors: blocks whose last frame a call has unpacked and whose check failed
    (WavPackUtils.cs:273-275), SetSample's discard calls included."""
    if wpc.error_message:
        return 0
    return wpc._state()[1]


def WavpackLossy(wpc) -> bool:
    if wpc.error_message:
        return bool(wpc._info.lossy)
    return wpc._state()[2]


# wvg_file_info carries the getters' results (wv_api.cpp fill_info applies
# WavPackUtils.cs:379-442: DSD rate x multiplier x 8, bits / 8, defaults).
def WavpackGetSampleRate(wpc) -> int:
    return int(wpc._info.sample_rate)


def WavpackGetNumChannels(wpc) -> int:
    return int(wpc._info.num_channels)


def WavpackGetBitsPerSample(wpc) -> int:
    return int(wpc._info.bits_per_sample)


def WavpackGetBytesPerSample(wpc) -> int:
    return int(wpc._info.bytes_per_sample)


def WavpackGetReducedChannels(wpc) -> int:
    return int(wpc._info.reduced_channels)


def WavpackGetMode(wpc) -> int:
    return int(wpc._info.mode)


def WavpackGetFileFormat(wpc) -> int:
    return int(wpc._info.file_format)


def WavpackGetErrorMessage(wpc):
    return wpc.error_message


def WavpackGetVersion(wpc) -> int:
    return int(wpc._info.version)


def WavpackGetIsFloat(wpc) -> bool:
    return bool(wpc._info.is_float)


def WavpackGetIsFive(wpc) -> bool:
    return bool(wpc._info.is_five)


def WavpackGetHeader(wpc):
    i = wpc._info
    return None if i.header_off < 0 else wpc._data[i.header_off:i.header_off + i.header_len]


def WavpackGetTrailer(wpc):
    i = wpc._info
    return None if i.trailer_off < 0 else wpc._data[i.trailer_off:i.trailer_off + i.trailer_len]
