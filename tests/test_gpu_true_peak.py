"""GPU: per-channel true peak of a decoded batch on the device (wvg_batch_true_peak,
wv_tpeak.hip) and the front ends (api.scan_true_peak, api.scan_loudness(true_peak=True)).

Files are tiny (block_samples 32; the multichannel ones longer than two tiles of the
kernel, with impulses planted at a tile seam); their odd int counts leave later files'
ranges off 16-byte boundaries, and their sample rates give O = 4, 2 and 1 in one launch.
The expected records are Python integers (tests/true_peak_vectors.py) over the source
arrays (lossless files) or the oracle's decode (hybrid, float without WVG_OPEN_EXACT_FLOAT,
the corrupt golden file, the DSD file as PCM); never over the code under test.  Every field
of every record is compared, with no tolerance.  Host side: test_true_peak_host.py."""
import os

import numpy as np
import pytest

try:  # before the library loads: torch ships a HIP runtime of its own, and the process must hold one
    import torch  # noqa: F401
except ImportError:
    pass

from oracle import oracle as O
from synth import wvsynth as S
from tests import mc_vectors as M
from tests.true_peak_vectors import check, expected, oversample_of, sine_45
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

ALL, EXACT, DSDPCM = api.OPEN_ALL_CHANNELS, api.OPEN_EXACT_FLOAT, api.OPEN_DSD_AS_PCM
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 4096


class Case:
    def __init__(self, name, data, flags=0, ints=None, k=None, rate=44100):
        self.name, self.data, self.flags = name, data, flags
        self.ints = ints  # (frames, channels) int32: what the decode leaves; None: not measurable
        self.k = k        # full scale is 2^k
        self.rate = rate  # None: whatever the file says (golden files)
        self._want = {}

    def want(self, o):
        """the expected records at factor o (0: the rate's own), computed once"""
        o = o or oversample_of(self.rate)
        if o not in self._want:
            self._want[o] = expected(self.ints, self.k, o)
        return self._want[o]


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _oracle(data, nch):
    r = O.decode_file(data, chunk=CHUNK)
    assert r.status == 0 and r.nch == nch
    return r.samples.reshape(-1, nch)


def _mc(widths, frames, bits, seed, rate, plant):
    """M.pcm_file's layout with values planted in the N-channel source first: {(frame, channel): value}"""
    src = M.pcm_sources(widths, frames, bits, seed)
    full = np.concatenate(src, axis=1)
    for (f, c), v in plant.items():
        full[f, c] = v
    encs, c0 = [], 0
    for w in widths:
        p = S.EncParams(nch=w, bytes_per_sample=(bits + 7) // 8, block_samples=128, sample_rate=rate,
                        terms=S.TERMS_DEFAULT if w == 2 else [18, 2, 17])
        encs.append(S.encode_pcm(np.ascontiguousarray(full[:, c0: c0 + w]), p))
        c0 += w
    return M.mux(encs, sum(widths), 0), full


@pytest.fixture(scope="module")
def corpus():
    """the mixed batch, made once (at the first test: the tile sizes come from the library)"""
    cases = []
    seed = 0
    rates = (44100, 96000, 192000)
    for nch in (1, 2):
        for bits in (8, 16, 24, 32):
            for frames in (1, 33, 150):
                seed += 1
                rate = rates[seed % 3]
                x = S.audio_like(frames, nch, min(bits, 24), seed=seed)
                kw = {}
                if bits == 32:
                    x = (x.astype(np.int64) << 8).astype(np.int32)
                    kw["int32_zeros"] = 8
                p = S.EncParams(nch=nch, bytes_per_sample=bits // 8, block_samples=32, sample_rate=rate,
                                terms=S.TERMS_DEFAULT if nch == 2 else [18, 2, 17], **kw)
                cases.append(Case(f"{nch}ch_{bits}b_{frames}", S.encode_pcm(x, p), 0, x, bits - 1, rate))
    # 30 frames of INT32_MIN through a real decode: the peak leaves 2^55
    mx = np.full((30, 1), (-2 ** 23) << 8, dtype=np.int64).astype(np.int32)
    cases.append(Case("int32_min", S.encode_pcm(mx, S.EncParams(nch=1, bytes_per_sample=4, block_samples=32,
                                                                terms=[18, 2, 17], int32_zeros=8)), 0, mx, 31))
    # a full-scale sine at fs/4, 45 degrees off its crests: -3.01 dBFS of samples, 0 dBTP
    sx = sine_45(200)
    cases.append(Case("sine_45", S.encode_pcm(sx, S.EncParams(nch=1, block_samples=32, terms=[18, 2, 17])), 0, sx, 15))
    # a float file: not measurable under EXACT_FLOAT, the reference's clipped 24-bit ints without
    rng = np.random.default_rng(7)
    fx = (S.audio_like(150, 2, 16, seed=90).astype(np.float32) / 32768.0 + rng.normal(0, 1e-6, (150, 2))).astype(
        np.float32)
    for i, v in enumerate((-0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-39, 0.0, 7e-8)):
        fx[(37 * i + 5) % 150, i % 2] = v
    fwv = S.encode_float_exact(fx, S.EncParams(block_samples=32, terms=S.TERMS_DEFAULT))
    cases.append(Case("float_exact", fwv, EXACT))
    cases.append(Case("float_clipped", fwv, 0, _oracle(fwv, 2), 23))
    dsd = _golden("dsd_mode3.wv")
    cases.append(Case("dsd", dsd))
    dr = O.decode_file(dsd, chunk=CHUNK)
    assert dr.status == 0
    cases.append(Case("dsd_as_pcm", dsd, DSDPCM, api.dsd_pcm_ints(dr.samples.reshape(-1, dr.nch)), 23, None))
    # 3, 4 and 17 channels, longer than two tiles and no multiple of one, impulses at the seam
    t3, t4, t17 = (api.true_peak_tile_frames(n) for n in (3, 4, 17))
    f3, full3 = _mc([2, 1], 2 * t3 + 7, 16, 101, 44100, {(t3 - 1, 0): 32767, (t3, 1): -32768, (t3 + 5, 2): 32767})
    cases.append(Case("3ch", f3, ALL, full3, 15))
    cases.append(Case("does_not_open", b"this is not a WavPack file, whatever its length " * 4))
    f17, full17 = _mc([2] * 8 + [1], 2 * t17 + 5, 24, 102, 96000,
                      {(t17 - 6, 0): -8388608, (t17 - 5, 7): 8388607, (t17 + 4, 16): -8388608, (2 * t17, 9): 8388607})
    cases.append(Case("17ch", f17, ALL, full17, 23, 96000))
    f4, full4 = _mc([2, 2], 2 * t4 + 3, 16, 104, 44100, {(t4 - 1, 3): -32768, (t4, 3): 32767, (2 * t4 - 1, 0): 32767})
    cases.append(Case("4ch", f4, ALL, full4, 15))
    cor = _golden("corrupt_default.wv")
    cases.append(Case("corrupt", cor, 0, _oracle(cor, 2), 15, None))
    hx = S.audio_like(150, 2, 16, seed=103)
    hyb = S.encode_pcm(hx, S.EncParams(nch=2, block_samples=32, terms=S.TERMS_DEFAULT, hybrid=True,
                                       hybrid_bitrate=True, bitrate_x256=768))
    cases.append(Case("hybrid", hyb, 0, _oracle(hyb, 2), 15))
    # the golden files' rates are whatever they say
    b = api.DecodeBatch(CHUNK)
    try:
        for c in cases:
            if c.rate is None:
                c.rate = int(b.infos[b.add_file(c.data, c.flags)].sample_rate)
    finally:
        b.close()
    return cases


def _batch(cases):
    b = api.DecodeBatch(CHUNK)
    for c in cases:
        i = b.add_file(c.data, c.flags)
        assert (i >= 0) == (c.name != "does_not_open"), c.name
    b.decode()
    return b


def _check_all(b, cases, o, what=""):
    L = b._L
    for i, c in enumerate(cases):
        got = b.file_true_peak(i)
        if c.ints is None:
            assert got is None, c.name
            assert L.wvg_batch_file_true_peak(b._b, i, None, 0) == _lib.WVG_ERR_OPEN, c.name
            continue
        assert got is not None and len(got) == c.ints.shape[1] == b.infos[i].reduced_channels, c.name
        check(got, c.want(o), (what, c.name, o))


def test_the_decode_leaves_what_the_expectations_assume(corpus):
    """(the int32 output itself: the sources and the oracle's decodes the records are made
    from; some ranges start off a 16-byte boundary; the rates give all three factors)"""
    b = _batch(corpus)
    try:
        out = b.download()
        for i, c in enumerate(corpus):
            if c.ints is None:
                continue
            info = b.infos[i]
            assert (info.out_frames, info.reduced_channels) == c.ints.shape, c.name
            assert int(info.sample_rate) == c.rate, c.name
            np.testing.assert_array_equal(out[info.out_offset: info.out_offset + c.ints.size], c.ints.reshape(-1),
                                          err_msg=c.name)
        assert len({b.infos[i].out_offset % 4 for i, c in enumerate(corpus) if c.ints is not None}) > 1
        assert {oversample_of(c.rate) for c in corpus if c.ints is not None} == {1, 2, 4}
        # (the flagged DSD file presents itself at its byte rate, an eighth of the unflagged bit rate)
        names = [c.name for c in corpus]
        assert corpus[names.index("dsd_as_pcm")].rate * 8 == int(b.infos[names.index("dsd")].sample_rate)
    finally:
        b.close()


@pytest.mark.parametrize("oversample", [0, 1, 2, 4])
def test_every_record_of_every_file(corpus, oversample):
    b = _batch(corpus)
    try:
        b.true_peak(oversample)
        b.sync()
        _check_all(b, corpus, oversample)
        # fewer records than channels on request; the channel count comes back
        i = [c.name for c in corpus].index("17ch")
        two = np.zeros(2, dtype=_lib.TRUE_PEAK_DTYPE)
        assert b._L.wvg_batch_file_true_peak(b._b, i, two.ctypes.data, 2) == 17
        check(two, corpus[i].want(oversample)[:2], "cap_channels")
    finally:
        b.close()


def test_what_the_feature_is_for(corpus):
    """through a real decode: the INT32_MIN run's peak above 2^55, and the sine whose samples
    read -3 dBFS while its true peak is 0 dBTP"""
    cases = [next(c for c in corpus if c.name == n) for n in ("int32_min", "sine_45")]
    b = _batch(cases)
    try:
        b.true_peak()
        b.sync()
        r = b.file_true_peak(0)[0]
        assert (int(r["true_peak"]), int(r["true_peak_pos"]), int(r["overs"])) == (40539895659233280, 2, 18)
        assert (int(r["sample_peak"]), int(r["oversample"]), int(r["k"])) == (1 << 31, 4, 31)
        r = b.file_true_peak(1)[0]
        assert int(r["true_peak"]) == cases[1].want(4)[0]["true_peak"] == 555833285840
        assert 0.99 < int(r["true_peak"]) / 2.0 ** 39 < 1.02
        assert abs(int(r["sample_peak"]) / 2.0 ** 15 - 0.70709) < 1e-5
    finally:
        b.close()


def test_arguments_and_state(corpus):
    """WVG_ERR_ARG before any call and again after a re-upload; a batch reset and refilled
    with other files gives the new files' records"""
    L = _lib.lib()
    b = api.DecodeBatch(CHUNK)
    try:
        first, second = corpus[4:7], [corpus[10], corpus[2], corpus[20]]
        for c in first:
            b.add_file(c.data, c.flags)
        one = np.zeros(4, dtype=_lib.TRUE_PEAK_DTYPE)
        assert L.wvg_batch_true_peak(b._b, 0, None) == _lib.WVG_ERR_ARG  # before an upload
        b.decode()
        assert L.wvg_batch_file_true_peak(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG  # no call yet
        with pytest.raises(RuntimeError):
            b.file_true_peak(0)
        for bad in (3, 8, -1, 5):
            assert L.wvg_batch_true_peak(b._b, bad, None) == _lib.WVG_ERR_ARG
            with pytest.raises(ValueError):
                b.true_peak(bad)
        assert L.wvg_batch_file_true_peak(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG
        b.true_peak(2)
        b.sync()
        _check_all(b, first, 2, "first")
        assert L.wvg_batch_file_true_peak(b._b, len(first), one.ctypes.data, 4) == _lib.WVG_ERR_ARG  # no such file
        with pytest.raises(RuntimeError):
            b.file_true_peak(-1)
        # a refilled batch starts over
        b.reset()
        for c in second:
            b.add_file(c.data, c.flags)
        b.upload()
        assert L.wvg_batch_file_true_peak(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG
        b.decode()
        assert L.wvg_batch_file_true_peak(b._b, 0, one.ctypes.data, 4) == _lib.WVG_ERR_ARG
        b.true_peak()
        b.sync()
        _check_all(b, second, 0, "refilled")
    finally:
        b.close()


def test_two_factors_queued_back_to_back(corpus):
    b = _batch(corpus)
    try:
        b.true_peak(4)
        b.true_peak(1)
        b.sync()
        _check_all(b, corpus, 1, "second of two")
        b.true_peak(2)
        b.levels()
        b.true_peak(0)
        b.sync()
        _check_all(b, corpus, 0, "second of two, levels between")
    finally:
        b.close()


def test_scan_true_peak(corpus):
    """equals the per-batch path; the derived floats are what their definitions give"""
    cases = [c for c in corpus if c.flags == 0]
    res = api.scan_true_peak([c.data for c in cases])
    assert len(res) == len(cases)
    for c, r in zip(cases, res):
        if c.ints is None:
            assert r is None, c.name
            continue
        want = c.want(0)
        check(r["records"], want, ("scan", c.name))
        o = want[0]["oversample"]
        assert r["k"] == c.k and r["out_frames"] == c.ints.shape[0], c.name
        assert r["overs"] == [w["overs"] for w in want], c.name
        assert r["true_peak"] == [w["true_peak"] / 2.0 ** (c.k + 24) for w in want], c.name
        assert r["position_s"] == [w["true_peak_pos"] / o / c.rate for w in want], c.name
        assert r["max_dbtp"] == max(r["dbtp"]), c.name
        assert all(isinstance(v, float) for key in ("true_peak", "dbtp", "sample_peak_dbfs") for v in r[key]), c.name
    sine = res[[c.name for c in cases].index("sine_45")]
    assert sine["sample_peak_dbfs"][0] == pytest.approx(-3.0103, abs=1e-3)
    assert sine["dbtp"][0] == pytest.approx(0.0955, abs=1e-3) and sine["overs"][0] > 0
    # forced factors, the files' own flags: the multichannel ones; what is not measurable
    sub = [c for c in corpus if c.flags == ALL]
    for c, r in zip(sub, api.scan_true_peak([c.data for c in sub], ALL, 2)):
        check(r["records"], c.want(2), ("scan, all channels", c.name))
    fe = next(c for c in corpus if c.name == "float_exact")
    assert api.scan_true_peak([fe.data], EXACT) == [None]
    assert api.scan_true_peak([]) == []
    with pytest.raises(ValueError):
        api.scan_true_peak([fe.data], 0, 3)


def test_scan_loudness_with_true_peak(corpus):
    """the same decode carries both; without the keyword nothing changes"""
    cases = [c for c in corpus if c.flags == 0 and (c.ints is None or c.ints.shape[0] >= 150)]
    assert {c.name for c in cases if c.ints is None} == {"dsd", "does_not_open"}
    # half a second at 8 kHz: long enough for a gated block, so a gain exists
    lx = S.audio_like(4000, 1, 16, seed=301)
    cases.append(Case("loud_8k", S.encode_pcm(lx, S.EncParams(nch=1, block_samples=512, sample_rate=8000,
                                                              terms=[18, 2, 17])), 0, lx, 15, 8000))
    files = [c.data for c in cases]
    plain = api.scan_loudness(files, album=True)
    both = api.scan_loudness(files, album=True, true_peak=True)
    peaks = api.scan_true_peak(files)
    base = {n for n, _ in _lib.LOUDNESS_DTYPE} | {"record", "lufs", "gain_db"}
    assert len(plain) == len(both) == len(cases) + 1
    tops = []
    for c, p, t, s in zip(cases, plain, both, peaks):
        if c.ints is None:
            assert p is None and t is None and s is None, c.name
            continue
        assert set(p) == base and set(t) == base | {"true_peak_dbtp", "clip_safe_gain_db"}, c.name
        assert all(p[key] == t[key] for key in base - {"record"}), c.name
        assert t["true_peak_dbtp"] == s["max_dbtp"], c.name
        check(s["records"], c.want(0), ("scan_loudness's files", c.name))
        want = None if t["gain_db"] is None else min(t["gain_db"], -s["max_dbtp"])
        assert t["clip_safe_gain_db"] == want, c.name
        tops.append(s["max_dbtp"])
    assert both[-2]["gain_db"] is not None and both[-2]["clip_safe_gain_db"] is not None  # loud_8k
    assert set(plain[-1]) == base and both[-1]["true_peak_dbtp"] == max(tops)
    g = both[-1]["gain_db"]
    assert both[-1]["clip_safe_gain_db"] == (None if g is None else min(g, -max(tops)))
