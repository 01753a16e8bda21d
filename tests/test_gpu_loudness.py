"""GPU: integrated loudness of a decoded batch on the device (wvg_batch_loudness,
wv_loud.hip) and the front end (api.scan_loudness).

One mixed batch, made once.  The files are a few thousand frames at 8,000 Hz (S = 800,
block_samples 512), with the frame counts at which the run code can go wrong
(loudness_vectors.host_frames); their odd int counts leave later files' ranges off 16-byte
boundaries.  What the decode leaves is known without the code under test: the source
arrays (lossless files) or the oracle's decode (hybrid, float without WVG_OPEN_EXACT_FLOAT,
the corrupt golden file); for the DSD file opened as PCM, whose decode test_gpu_dsd_pcm.py
checks, the batch's own download.  Over those ints every record field and the whole block
image are compared bit for bit with the host build of the same header (api.loudness_ints),
and within loudness_vectors.TOL, counts exactly, with the restatement that never restarts
the filter.  Host side: test_loudness_host.py."""
import math
import os

import numpy as np
import pytest

try:  # before the library loads: torch ships a HIP runtime of its own, and the process must hold one
    import torch  # noqa: F401
except ImportError:
    pass

from oracle import oracle as O
from synth import wvsynth as S
from tests import loudness_vectors as V
from tests import mc_vectors as M
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

ALL, EXACT, DSDPCM = api.OPEN_ALL_CHANNELS, api.OPEN_EXACT_FLOAT, api.OPEN_DSD_AS_PCM
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 4096
RATE = V.RATE
FIELDS = [n for n, _ in _lib.LOUDNESS_DTYPE]


class Case:
    def __init__(self, name, data, flags=0, ints=None, k=None, rate=RATE, mask=0, measurable=True):
        self.name, self.data, self.flags = name, data, flags
        self.ints = ints  # (frames, channels) int32: what the decode leaves; None: taken from the download
        self.k, self.rate, self.mask, self.measurable = k, rate, mask, measurable
        self.host = self.want = None  # (record, blocks) of api.loudness_ints; loudness_vectors.measure


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _oracle(data, nch):
    r = O.decode_file(data, chunk=CHUNK)
    assert r.nch == nch
    return r.samples.reshape(-1, nch)


def _pcm(x, bits, **kw):
    nch, rate = x.shape[1], kw.pop("rate", RATE)
    if bits == 32:
        x = (x.astype(np.int64) << 8).astype(np.int32)
        kw["int32_zeros"] = 8
    p = S.EncParams(nch=nch, bytes_per_sample=bits // 8, block_samples=512, sample_rate=rate,
                    terms=S.TERMS_DEFAULT if nch == 2 else [18, 2, 17], **kw)
    return S.encode_pcm(x, p), x


def _cases():
    R = _lib.lib().wvg_loudness_run_steps()
    F = V.host_frames(R)
    cases = []
    for nch in (1, 2):
        for i, frames in enumerate(F):  # every frame count, the depths taking turns
            bits = (8, 16, 24, 32)[(i + nch) % 4]
            data, x = _pcm(V.noise(frames, nch, min(bits, 24) - 1, 300 * nch + i), bits)
            cases.append(Case(f"{nch}ch_{bits}b_{frames}", data, 0, x, bits - 1))
    f3, _, full3 = M.pcm_file([2, 1], F[6], 16, seed=101, block_samples=512, sample_rate=RATE)
    cases.append(Case("3ch", f3, ALL, full3, 15, mask=0))
    cases.append(Case("does_not_open", b"this is not a WavPack file, whatever its length " * 4, measurable=False))
    f6, _, full6 = M.pcm_file([2, 1, 1, 2], F[4] + 3, 24, seed=102, block_samples=512, mask=0x3F, sample_rate=RATE)
    cases.append(Case("6ch", f6, ALL, full6, 23, mask=0x3F))
    data, x = _pcm(V.noise(6 * 4410 + 5, 2, 15, 7), 16, rate=44100)
    cases.append(Case("44100", data, 0, x, 15, rate=44100))
    t = np.arange(48000)
    sine = np.round(((1 << 23) - 1) * np.sin(2.0 * np.pi * 997.0 * t / 48000.0)).astype(np.int32).reshape(-1, 1)
    data, x = _pcm(sine, 24, rate=48000)
    cases.append(Case("sine_997", data, 0, x, 23, rate=48000))
    hx = V.noise(F[4] + 1, 2, 15, 11)
    hyb = S.encode_pcm(hx, S.EncParams(nch=2, block_samples=512, sample_rate=RATE, terms=S.TERMS_DEFAULT, hybrid=True,
                                       hybrid_bitrate=True, bitrate_x256=768))
    cases.append(Case("hybrid", hyb, 0, _oracle(hyb, 2), 15))
    rng = np.random.default_rng(7)
    fx = (V.noise(F[4], 2, 15, 13).astype(np.float32) / 32768.0 + rng.normal(0, 1e-6, (F[4], 2))).astype(np.float32)
    for i, v in enumerate((-0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-39, 0.0, 7e-8)):
        fx[(37 * i + 5) % F[4], i % 2] = v
    fwv = S.encode_float_exact(fx, S.EncParams(block_samples=512, sample_rate=RATE, terms=S.TERMS_DEFAULT))
    cases.append(Case("float_exact", fwv, EXACT, measurable=False))
    cases.append(Case("float_clipped", fwv, 0, _oracle(fwv, 2), 23))
    cor = _golden("corrupt_default.wv")
    cases.append(Case("corrupt", cor, 0, _oracle(cor, 2), 15, rate=None))
    dsd = _golden("dsd_mode3.wv")
    cases.append(Case("dsd", dsd, 0, measurable=False))
    cases.append(Case("dsd_as_pcm", dsd, DSDPCM, None, 23, rate=None))
    data, x = _pcm(np.zeros((F[5] + 9, 2), dtype=np.int32), 16)
    cases.append(Case("zeros", data, 0, x, 15))
    return cases


def _batch(cases, kernel="auto"):
    b = api.DecodeBatch(CHUNK)
    b.set_kernel(kernel)
    for c in cases:
        i = b.add_file(c.data, c.flags)
        assert (i >= 0) == (c.name != "does_not_open"), c.name
    b.decode()
    return b


def _results(b, n):
    """after sync: every file's record (None: not measurable) and block powers"""
    img = b.download_loudness_blocks()
    out = []
    for i in range(n):
        rec = b.file_loudness(i)
        out.append(None if rec is None else
                   (rec, img[int(rec["block_offset"]): int(rec["block_offset"]) + int(rec["blocks"])].copy()))
    return out, img


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        assert got[0].tobytes() == want[0].tobytes(), (what, got[0], want[0])
        assert got[1].tobytes() == want[1].tobytes(), what


@pytest.fixture(scope="module")
def corpus():
    """the mixed batch decoded and measured once: the cases with the ints the decode left,
    the host code's and the restatement's answers over them, and what the device gave"""
    cases = _cases()
    b = _batch(cases)
    try:
        out = b.download()
        infos = list(b.infos)
        b.loudness()
        b.sync()
        got, img = _results(b, len(cases))
    finally:
        b.close()
    off = 0
    for i, c in enumerate(cases):
        info = infos[i]
        if c.name == "does_not_open":
            continue
        if c.rate is None:
            c.rate = int(info.sample_rate)
        vis = out[info.out_offset: info.out_offset + info.out_frames * info.reduced_channels].reshape(
            info.out_frames, info.reduced_channels)
        if c.ints is None:
            c.ints = vis.copy()
        c.decoded = vis
        if c.measurable:
            c.host = api.loudness_ints(c.ints, c.k, c.rate, c.mask)
            c.host[0]["block_offset"] = off
            off += int(c.host[0]["blocks"])
            c.want = V.measure(c.ints, c.k, c.rate, c.mask)
    return cases, infos, got, img


def test_the_decode_leaves_what_the_expectations_assume(corpus):
    cases, infos, _, _ = corpus
    for c, info in zip(cases, infos):
        if c.name == "does_not_open":
            continue
        assert (info.out_frames, info.reduced_channels) == c.ints.shape, c.name
        np.testing.assert_array_equal(c.decoded, c.ints, err_msg=c.name)
        if c.measurable:
            assert int(info.sample_rate) == c.rate, c.name
    assert len({info.out_offset % 4 for c, info in zip(cases, infos) if c.measurable}) > 1
    by = {c.name: c for c in cases}
    # (the flagged DSD file presents itself at its byte rate, an eighth of the unflagged bit rate)
    assert by["dsd_as_pcm"].rate * 8 == int(infos[[c.name for c in cases].index("dsd")].sample_rate)
    assert by["6ch"].ints.shape[1] == 6 and by["3ch"].ints.shape[1] == 3


def test_bit_for_bit_with_the_host_code(corpus):
    """every field of every record and the whole block image"""
    cases, _, got, img = corpus
    n = 0
    for c, g in zip(cases, got):
        if not c.measurable:
            assert g is None, c.name
            continue
        for f in FIELDS:
            assert g[0][f].tobytes() == c.host[0][f].tobytes(), (c.name, f, g[0][f], c.host[0][f])
        assert g[1].tobytes() == c.host[1].tobytes(), c.name
        n += len(g[1])
    assert n == len(img) > 0
    assert img.tobytes() == np.concatenate([c.host[1] for c in cases if c.measurable]).tobytes()


def test_against_the_restatement(corpus):
    cases, _, got, _ = corpus
    for c, g in zip(cases, got):
        if c.measurable:
            V.check(g[0], g[1], c.want, c.name)


def test_what_is_not_measurable_and_what_is_short(corpus):
    cases, _, got, _ = corpus
    by = {c.name: g for c, g in zip(cases, got)}
    for name in ("float_exact", "dsd", "does_not_open"):
        assert by[name] is None, name
    rec, blocks = by["dsd_as_pcm"]
    c = next(c for c in cases if c.name == "dsd_as_pcm")
    assert int(rec["step_frames"]) == (c.rate + 5) // 10
    if c.ints.shape[0] < 4 * int(rec["step_frames"]):
        assert (int(rec["blocks"]), float(rec["power"]), len(blocks)) == (0, 0.0, 0)
    rec, blocks = by["zeros"]
    assert int(rec["blocks"]) > 0 and (int(rec["abs_blocks"]), int(rec["gated_blocks"])) == (0, 0)
    assert float(rec["power"]) == 0.0 == float(rec["max_block_power"]) and not blocks.any()
    rec, _ = by["sine_997"]
    assert abs(V.lufs(float(rec["power"])) - (-3.01)) <= 0.01
    rec, _ = by["6ch"]
    assert int(rec["channels"]) == 6


def test_error_codes(corpus):
    cases = corpus[0]
    L = _lib.lib()
    rec = np.zeros(1, dtype=_lib.LOUDNESS_DTYPE)
    b = api.DecodeBatch(CHUNK)
    try:
        for c in cases[:3]:
            b.add_file(c.data, c.flags)
        assert L.wvg_batch_loudness(b._b, None) == _lib.WVG_ERR_ARG  # before an upload
        b.decode()
        assert L.wvg_batch_file_loudness(b._b, 0, rec.ctypes.data) == _lib.WVG_ERR_ARG  # no loudness call yet
        b.loudness()
        b.sync()
        assert L.wvg_batch_file_loudness(b._b, 0, rec.ctypes.data) == 0
        assert L.wvg_batch_file_loudness(b._b, 3, rec.ctypes.data) == _lib.WVG_ERR_ARG  # no such file
        assert L.wvg_batch_file_loudness(b._b, 0, None) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_download_loudness_blocks(b._b, None, 0) in (_lib.WVG_ERR_ARG, _lib.WVG_ERR_SPACE)
        n = L.wvg_batch_loudness_blocks(b._b)
        buf = np.zeros(max(n, 1))
        assert L.wvg_batch_download_loudness_blocks(b._b, buf.ctypes.data, n - 1) == _lib.WVG_ERR_SPACE
        with pytest.raises(RuntimeError):
            b.file_loudness(-1)
    finally:
        b.close()
    nope = [c for c in cases if not c.measurable]
    b = _batch(nope)
    try:
        b.loudness()
        b.sync()
        for i in range(len(nope)):
            assert L.wvg_batch_file_loudness(b._b, i, rec.ctypes.data) == _lib.WVG_ERR_OPEN
            assert b.file_loudness(i) is None and b.loudness_blocks(i) is None
        assert L.wvg_batch_loudness_blocks(b._b) == 0 and len(b.download_loudness_blocks()) == 0
    finally:
        b.close()


def test_two_calls_back_to_back_and_a_refill(corpus):
    cases, _, got, _ = corpus
    L = _lib.lib()
    rec = np.zeros(1, dtype=_lib.LOUDNESS_DTYPE)
    b = _batch(cases)
    try:
        b.loudness()
        b.loudness()
        b.sync()
        again, _ = _results(b, len(cases))
        for c, g, a in zip(cases, got, again):
            _same(a, g, ("second of two", c.name))
        # reset and refill with fewer files: nothing stale
        keep = sorted({i for i, c in enumerate(cases) if c.name in ("6ch", "zeros", "dsd")} | {2, 12}, reverse=True)
        b.reset()
        for i in keep:
            b.add_file(cases[i].data, cases[i].flags)
        b.upload()
        assert L.wvg_batch_file_loudness(b._b, 0, rec.ctypes.data) == _lib.WVG_ERR_ARG
        b.decode()
        assert L.wvg_batch_file_loudness(b._b, 0, rec.ctypes.data) == _lib.WVG_ERR_ARG
        b.loudness()
        b.sync()
        res, img = _results(b, len(keep))
        off = 0
        for j, i in enumerate(keep):
            if not cases[i].measurable:
                assert res[j] is None
                continue
            want = cases[i].host[0].copy()
            want["block_offset"] = off
            off += int(want["blocks"])
            _same(res[j], (want, cases[i].host[1]), ("refilled", cases[i].name))
        assert len(img) == off
        assert L.wvg_batch_file_loudness(b._b, len(keep), rec.ctypes.data) == _lib.WVG_ERR_ARG
    finally:
        b.close()


def test_interleaved_with_levels_and_planar(corpus):
    """levels, loudness, planar, loudness with no sync in between: every result is what it is alone"""
    cases, _, got, _ = corpus
    b = _batch(cases)
    try:
        b.levels(1 << 20)
        b.planar()
        b.sync()
        lv = [b.file_levels(i) for i in range(len(cases))]
        img = b.download_planar().copy()
        b.levels(1 << 20)
        b.loudness()
        lay = b.planar()
        b.loudness()
        b.sync()
        res, _ = _results(b, len(cases))
        for i, (c, g) in enumerate(zip(cases, got)):
            _same(res[i], g, ("interleaved", c.name))
            l2 = b.file_levels(i)
            assert (l2 is None) == (lv[i] is None) and (l2 is None or l2.tobytes() == lv[i].tobytes()), c.name
        img2 = b.download_planar()
        assert img2.view(np.uint32).tobytes() == img.view(np.uint32).tobytes() and len(lay) == len(cases)
    finally:
        b.close()


@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
def test_kernel_choice_gives_the_same_records(corpus, kernel):
    cases, _, got, _ = corpus
    b = _batch(cases, kernel)
    try:
        b.loudness()
        b.sync()
        res, _ = _results(b, len(cases))
        for c, g, r in zip(cases, got, res):
            _same(r, g, (kernel, c.name))
    finally:
        b.close()


def test_on_torchs_current_stream(corpus):
    torch = pytest.importorskip("torch")
    cases, _, got, _ = corpus
    b = _batch(cases)
    try:
        dev = api.context_device()
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            b.loudness(stream=torch.cuda.current_stream(dev).cuda_stream)
        b.sync()
        res, _ = _results(b, len(cases))
        for c, g, r in zip(cases, got, res):
            _same(r, g, ("torch stream", c.name))
    finally:
        b.close()


def test_scan_loudness_and_the_album(corpus):
    cases, _, got, _ = corpus
    sub = [(c, g) for c, g in zip(cases, got) if c.flags == 0]
    res = api.scan_loudness([c.data for c, _ in sub], 0, target_lufs=-23.0, album=True)
    assert len(res) == len(sub) + 1
    union = []
    for (c, g), r in zip(sub, res):
        if not c.measurable:
            assert r is None, c.name
            continue
        for f in FIELDS:
            if f != "block_offset":
                assert r[f] == g[0][f], (c.name, f)
        if int(g[0]["gated_blocks"]):
            assert r["lufs"] == -0.691 + 10.0 * math.log10(float(g[0]["power"])), c.name
            assert r["gain_db"] == -23.0 - r["lufs"]
        else:
            assert r["lufs"] == float("-inf") and r["gain_db"] is None, c.name
        union += c.want["P"]
    z = res[[c.name for c, _ in sub].index("zeros")]
    assert z["lufs"] == float("-inf") and z["gain_db"] is None and z["blocks"] > 0
    album, want = res[-1], V.gate(union)
    assert len({c.rate for c, _ in sub if c.measurable}) > 1  # rates mix
    for f in ("blocks", "abs_blocks", "gated_blocks"):
        assert album[f] == want[f], f
    assert all(abs(p - g) > V.GATE_MARGIN * g for p in union for g in (V.ABS_GATE, want["rel"]) if g > 0)
    for f in ("power", "ungated_power", "max_block_power"):
        assert abs(album[f] - want[f]) <= V.TOL * want["max_block_power"], f
    assert abs(album["lufs"] - V.lufs(want["power"])) <= 1e-9
    # with the files' own flags, and nothing to measure
    mc = [(c, g) for c, g in zip(cases, got) if c.flags == ALL]
    for (c, g), r in zip(mc, api.scan_loudness([c.data for c, _ in mc], ALL)):
        assert r["power"] == float(g[0]["power"]) and r["channels"] == c.ints.shape[1], c.name
    fe = next(c for c in cases if c.name == "float_exact")
    assert api.scan_loudness([fe.data], EXACT) == [None]
    assert api.scan_loudness([]) == []
    alone = api.scan_loudness([fe.data], EXACT, album=True)
    assert alone[0] is None and alone[1]["blocks"] == 0 and alone[1]["lufs"] == float("-inf")
