"""GPU: loudness range and short-term loudness of a decoded batch on the device
(wvg_batch_loudness_range, wv_lra.hip) and the front end (api.scan_loudness).

One mixed batch, made once, of lossless files at 6,000 .. 8,000 Hz (S = 600 .. 800), so what
the decode leaves is the source arrays.  Over those ints every record field and the whole
short-term image are compared bit for bit with the host build of the same header
(api.loudness_range_ints), and for the smaller files within loudness_range_vectors.TOL,
counts exactly, with the restatement built on the never-restarted filter and sorted().  Host
side: test_loudness_range_host.py."""
import numpy as np
import pytest

try:  # before the library loads: torch ships a HIP runtime of its own, and the process must hold one
    import torch  # noqa: F401
except ImportError:
    pass

from synth import wvsynth as S
from tests import loudness_range_vectors as W
from tests import mc_vectors as M
from wavpackdecoder_amd import _lib, api

pytestmark = pytest.mark.gpu

ALL = api.OPEN_ALL_CHANNELS
CHUNK = 4096
FIELDS = [n for n, _ in _lib.LOUDNESS_RANGE_DTYPE]
LD_FIELDS = [n for n, _ in _lib.LOUDNESS_DTYPE]
R = _lib.lib().wvg_loudness_run_steps()


class Case:
    def __init__(self, name, data, flags=0, ints=None, k=None, rate=None, mask=0, measurable=True, restate=False):
        self.name, self.data, self.flags = name, data, flags
        self.ints = ints  # (frames, channels) int32: what the decode leaves
        self.k, self.rate, self.mask, self.measurable, self.restate = k, rate, mask, measurable, restate
        self.host = self.loud = self.want = None  # api.loudness_range_ints', api.loudness_ints', W.measure's


def _pcm(x, bits, rate, block_samples=512):
    nch = x.shape[1]
    kw = {}
    if bits == 32:
        x = (x.astype(np.int64) << 8).astype(np.int32)
        kw["int32_zeros"] = 8
    p = S.EncParams(nch=nch, bytes_per_sample=bits // 8, block_samples=block_samples, sample_rate=rate,
                    terms=S.TERMS_DEFAULT if nch == 2 else [18, 2, 17], **kw)
    return S.encode_pcm(x, p), x


def _step(rate):
    return (rate + 5) // 10


def _cases():
    cases = []
    # steady noise at nsteps 29, 30, 31, 39, 40, 50: 0, 1, 2, 10, 11 and 21 values; odd tails
    for i, steps in enumerate((29, 30, 31, 39, 40, 50)):
        rate, nch, bits = (6000, 7000, 8000)[i % 3], 1 + i % 2, (16, 24, 8)[i % 3]
        x = W.steady(steps, nch, bits - 1, 500 + i, _step(rate), tail=1 + 2 * i)
        data, x = _pcm(x, bits, rate)
        cases.append(Case(f"steady_{steps}", data, 0, x, bits - 1, rate, restate=True))
    # the level jumps over seconds: both gates have work; about 300 values
    x = W.jumping(330, 1, 15, 21, 600, 40, W.JUMP_LEVELS, tail=7)
    data, x = _pcm(x, 16, 6000, 4096)
    cases.append(Case("jumping", data, 0, x, 15, 6000, restate=True))
    cases.append(Case("does_not_open", b"this is not a WavPack file, whatever its length " * 4, measurable=False))
    # period R * S: the runs restart from zero state, so from the second run on every step
    # energy depends on its phase alone and the selection meets exact ties
    one = W.steady(R, 1, 15, 22, 600)
    x = np.concatenate([np.tile(one, (330 // R + 1, 1))[:330 * 600], one[:5]])
    data, x = _pcm(x, 16, 6000, 4096)
    cases.append(Case("periodic", data, 0, x, 15, 6000))
    # more values than four per thread of the select kernel
    x = W.jumping(1135, 1, 15, 23, 600, 90, W.JUMP_LEVELS, tail=3)
    data, x = _pcm(x, 16, 6000, 8192)
    cases.append(Case("long_mono", data, 0, x, 15, 6000))
    f6, _, full6 = M.pcm_file([2, 1, 1, 2], 40 * 700 + 3, 24, seed=102, block_samples=512, mask=0x3F, sample_rate=7000)
    cases.append(Case("6ch", f6, ALL, full6, 23, 7000, mask=0x3F, restate=True))
    data, x = _pcm(W.steady(33, 2, 23, 24, 800, tail=9), 32, 8000)
    cases.append(Case("32bit", data, 0, x, 31, 8000, restate=True))
    data, x = _pcm(np.zeros((35 * 600 + 9, 2), dtype=np.int32), 16, 6000)
    cases.append(Case("zeros", data, 0, x, 15, 6000, restate=True))
    data, x = _pcm(W.steady(35, 2, 15, 25, 600, level=1e-4, tail=1), 16, 6000)
    cases.append(Case("minus_80_dbfs", data, 0, x, 15, 6000, restate=True))
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
    """after sync: every file's record (None: not measurable) and short-term powers"""
    img = b.download_loudness_shorts()
    out = []
    for i in range(n):
        rec = b.file_loudness_range(i)
        out.append(None if rec is None else
                   (rec, img[int(rec["short_offset"]): int(rec["short_offset"]) + int(rec["shorts"])].copy()))
    return out, img


def _loud(b, n):
    return [b.file_loudness(i) for i in range(n)]


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        assert got[0].tobytes() == want[0].tobytes(), (what, got[0], want[0])
        assert got[1].tobytes() == want[1].tobytes(), what


@pytest.fixture(scope="module")
def corpus():
    """the mixed batch decoded and measured once -- by a range call with no loudness call
    before it -- with the host code's and the restatement's answers over the source ints"""
    cases = _cases()
    b = _batch(cases)
    try:
        out = b.download()
        infos = list(b.infos)
        b.loudness_range()
        b.sync()
        got, img = _results(b, len(cases))
        loud = _loud(b, len(cases))
    finally:
        b.close()
    off = boff = 0
    for i, c in enumerate(cases):
        info = infos[i]
        if c.name == "does_not_open":
            continue
        c.decoded = out[info.out_offset: info.out_offset + info.out_frames * info.reduced_channels].reshape(
            info.out_frames, info.reduced_channels)
        c.host = api.loudness_range_ints(c.ints, c.k, c.rate, c.mask)
        c.host[0]["short_offset"] = off
        off += int(c.host[0]["shorts"])
        c.loud = api.loudness_ints(c.ints, c.k, c.rate, c.mask)[0]
        c.loud["block_offset"] = boff
        boff += int(c.loud["blocks"])
        if c.restate:
            c.want = W.measure(c.ints, c.k, c.rate, c.mask)
    return cases, infos, got, img, loud


def test_the_decode_leaves_what_the_expectations_assume(corpus):
    cases, infos, _, _, _ = corpus
    for c, info in zip(cases, infos):
        if c.name == "does_not_open":
            continue
        assert (info.out_frames, info.reduced_channels) == c.ints.shape, c.name
        np.testing.assert_array_equal(c.decoded, c.ints, err_msg=c.name)
        assert int(info.sample_rate) == c.rate and 6000 <= c.rate <= 8000, c.name
    assert len({info.out_offset % 4 for c, info in zip(cases, infos) if c.measurable}) > 1
    by = {c.name: c for c in cases}
    assert [int(by[f"steady_{s}"].host[0]["gated_shorts"]) for s in (29, 30, 31, 39, 40, 50)] == [0, 1, 2, 10, 11, 21]
    j = by["jumping"].host[0]
    assert 250 <= int(j["shorts"]) <= 350 and 0 < int(j["gated_shorts"]) < int(j["abs_shorts"]) < int(j["shorts"])
    p = by["periodic"].host
    assert 250 <= int(p[0]["shorts"]) <= 350 and len(set(p[1][4 * R:].tolist())) <= R  # exact ties
    lm = by["long_mono"].host[0]
    assert int(lm["shorts"]) >= 1100 and 0 < int(lm["gated_shorts"]) < int(lm["abs_shorts"]) < int(lm["shorts"])
    assert by["6ch"].ints.shape[1] == 6 and by["32bit"].k == 31
    assert (int(by["minus_80_dbfs"].host[0]["abs_shorts"]), int(by["minus_80_dbfs"].host[0]["shorts"])) == (0, 6)
    assert 0 < float(by["minus_80_dbfs"].host[0]["max_short_power"]) < W.ABS_GATE


def test_no_short_term_power_is_near_a_gate(corpus):
    for c in corpus[0]:
        if c.restate:
            assert W.gates_are_clear(c.want), c.name


def test_bit_for_bit_with_the_host_code(corpus):
    """every field of every record and the whole short-term image"""
    cases, _, got, img, _ = corpus
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
    cases, _, got, _, _ = corpus
    worst = 0.0
    for c, g in zip(cases, got):
        if c.restate:
            worst = max(worst, W.check(g[0], g[1], c.want, c.name))
    print(f"d = {worst:.3e}")
    assert sum(c.restate for c in cases) >= 10


def test_a_range_call_alone_makes_loudness_readable(corpus):
    """the fixture issued no loudness call: its records are wvg_batch_loudness's all the same"""
    cases, _, _, _, loud = corpus
    for c, l in zip(cases, loud):
        assert (l is None) == (not c.measurable), c.name
        if l is not None:
            for f in LD_FIELDS:
                assert l[f].tobytes() == c.loud[f].tobytes(), (c.name, f)


def test_after_a_loudness_call_gives_the_same_bits(corpus):
    cases, _, got, _, loud = corpus
    b = _batch(cases)
    try:
        b.loudness()
        b.loudness_range()
        b.sync()
        res, _ = _results(b, len(cases))
        for c, g, r, l, l2 in zip(cases, got, res, loud, _loud(b, len(cases))):
            _same(r, g, ("after loudness", c.name))
            assert (l is None) == (l2 is None) and (l is None or l.tobytes() == l2.tobytes()), c.name
    finally:
        b.close()


def test_a_second_decode_makes_the_step_energies_stale(corpus):
    """decode, poison, loudness (over the poison), decode, range: the range call must measure
    again, not read the energies of the poisoned output"""
    cases, _, got, _, loud = corpus
    b = _batch(cases)
    try:
        b.sync()
        b.poison(0x35)
        b.loudness()
        b.sync()
        i = [c.name for c in cases].index("jumping")
        assert b.file_loudness(i).tobytes() != loud[i].tobytes()  # the poison was measured
        b.decode()
        b.loudness_range()
        b.sync()
        res, _ = _results(b, len(cases))
        for c, g, r, l, l2 in zip(cases, got, res, loud, _loud(b, len(cases))):
            _same(r, g, ("second decode", c.name))
            assert (l is None) == (l2 is None) and (l is None or l.tobytes() == l2.tobytes()), c.name
    finally:
        b.close()


def test_error_codes(corpus):
    cases = corpus[0]
    L = _lib.lib()
    rec = np.zeros(1, dtype=_lib.LOUDNESS_RANGE_DTYPE)
    b = api.DecodeBatch(CHUNK)
    try:
        for c in cases[:3]:
            b.add_file(c.data, c.flags)
        assert L.wvg_batch_loudness_range(b._b, None) == _lib.WVG_ERR_ARG  # before an upload
        b.decode()
        assert L.wvg_batch_file_loudness_range(b._b, 0, rec.ctypes.data) == _lib.WVG_ERR_ARG  # no range call yet
        assert L.wvg_batch_loudness_shorts(b._b) == _lib.WVG_ERR_ARG
        b.loudness()
        b.sync()
        assert L.wvg_batch_file_loudness_range(b._b, 0, rec.ctypes.data) == _lib.WVG_ERR_ARG  # a loudness call is none
        b.loudness_range()
        b.sync()
        assert L.wvg_batch_file_loudness_range(b._b, 0, rec.ctypes.data) == 0
        assert L.wvg_batch_file_loudness_range(b._b, 3, rec.ctypes.data) == _lib.WVG_ERR_ARG  # no such file
        assert L.wvg_batch_file_loudness_range(b._b, 0, None) == _lib.WVG_ERR_ARG
        assert L.wvg_batch_download_loudness_shorts(b._b, None, 0) == _lib.WVG_ERR_ARG  # the argument is checked first
        n = L.wvg_batch_loudness_shorts(b._b)
        assert n == 1 + 2
        buf = np.full(n + 1, -7.25)
        assert L.wvg_batch_download_loudness_shorts(b._b, buf.ctypes.data, n - 1) == _lib.WVG_ERR_SPACE
        assert (buf == -7.25).all()
        assert L.wvg_batch_download_loudness_shorts(b._b, buf.ctypes.data, n) == 0 and buf[n] == -7.25
        with pytest.raises(RuntimeError):
            b.file_loudness_range(-1)
    finally:
        b.close()
    nope = [c for c in cases if not c.measurable]
    b = _batch(nope)
    try:
        b.loudness_range()
        b.sync()
        for i in range(len(nope)):
            assert L.wvg_batch_file_loudness_range(b._b, i, rec.ctypes.data) == _lib.WVG_ERR_OPEN
            assert b.file_loudness_range(i) is None and b.loudness_shorts(i) is None
        assert L.wvg_batch_loudness_shorts(b._b) == 0 and len(b.download_loudness_shorts()) == 0
    finally:
        b.close()


def test_two_calls_back_to_back_and_a_refill(corpus):
    cases, _, got, _, _ = corpus
    L = _lib.lib()
    rec = np.zeros(1, dtype=_lib.LOUDNESS_RANGE_DTYPE)
    b = _batch(cases)
    try:
        b.loudness_range()
        b.loudness_range()
        b.sync()
        again, _ = _results(b, len(cases))
        for c, g, a in zip(cases, got, again):
            _same(a, g, ("second of two", c.name))
        i = [c.name for c in cases].index("jumping")
        assert b.loudness_shorts(i).tobytes() == got[i][1].tobytes()
        # reset and refill with fewer files: nothing stale
        names = ("6ch", "zeros", "does_not_open", "steady_40", "jumping", "steady_29")
        keep = [[c.name for c in cases].index(n) for n in names]
        b.reset()
        for i in keep:
            b.add_file(cases[i].data, cases[i].flags)
        b.upload()
        assert L.wvg_batch_file_loudness_range(b._b, 0, rec.ctypes.data) == _lib.WVG_ERR_ARG
        b.decode()
        assert L.wvg_batch_file_loudness_range(b._b, 0, rec.ctypes.data) == _lib.WVG_ERR_ARG
        b.loudness_range()
        b.sync()
        res, img = _results(b, len(keep))
        off = 0
        for j, i in enumerate(keep):
            if not cases[i].measurable:
                assert res[j] is None
                continue
            want = cases[i].host[0].copy()
            want["short_offset"] = off
            off += int(want["shorts"])
            _same(res[j], (want, cases[i].host[1]), ("refilled", cases[i].name))
        assert len(img) == off
        assert L.wvg_batch_file_loudness_range(b._b, len(keep), rec.ctypes.data) == _lib.WVG_ERR_ARG
    finally:
        b.close()


def test_interleaved_with_levels_and_planar(corpus):
    """levels, range, planar, range with no sync in between: every result is what it is alone"""
    cases, _, got, _, _ = corpus
    b = _batch(cases)
    try:
        b.levels(1 << 20)
        b.planar()
        b.sync()
        lv = [b.file_levels(i) for i in range(len(cases))]
        img = b.download_planar().copy()
        b.levels(1 << 20)
        b.loudness_range()
        lay = b.planar()
        b.loudness_range()
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
    cases, _, got, _, _ = corpus
    b = _batch(cases, kernel)
    try:
        b.loudness_range()
        b.sync()
        res, _ = _results(b, len(cases))
        for c, g, r in zip(cases, got, res):
            _same(r, g, (kernel, c.name))
    finally:
        b.close()


def test_on_torchs_current_stream(corpus):
    torch = pytest.importorskip("torch")
    cases, _, got, _, _ = corpus
    b = _batch(cases)
    try:
        dev = api.context_device()
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            b.loudness_range(stream=torch.cuda.current_stream(dev).cuda_stream)
        b.sync()
        res, _ = _results(b, len(cases))
        for c, g, r in zip(cases, got, res):
            _same(r, g, ("torch stream", c.name))
    finally:
        b.close()


def test_scan_loudness_with_the_range_and_the_album(corpus):
    """Tech 3342's first compliance signal (-20 then -30 dBFS, 20 s each) beside a corpus file"""
    cases, _, got, _, _ = corpus
    other = next(c for c in cases if c.name == "steady_50")
    og = got[cases.index(other)]
    levels, want_lra = W.TECH_3342[0]
    x = W.sine_segments(levels, 8000)
    data, _ = _pcm(x, 16, 8000, 8192)
    # the two channels are the same ints, so every stereo ST_j is exactly twice the mono one
    # (a power of two): the restatement runs over one channel and its powers are doubled
    mono = W.measure(x[:, :1], 15, 8000)
    st2 = [2.0 * p for p in mono["ST"]]
    want = W.gate(st2)
    assert W.gates_are_clear(mono) and W.gates_are_clear(want, st2)
    plain = api.scan_loudness([data, other.data], 0, album=True)
    res = api.scan_loudness([data, other.data], 0, album=True, loudness_range=True)
    assert len(res) == 3 == len(plain)
    for p, r in zip(plain, res):  # the default output is unchanged: the same keys, the same values
        assert set(p) < set(r)
        for key in p:
            if key != "record":
                assert r[key] == p[key], key
        assert "lra_lu" not in p and "shorts" not in p
    r = res[0]
    for f in W.COUNTS:
        assert r[f] == want[f], f
    for f in W.POWERS:
        assert abs(r[f] - want[f]) <= W.TOL * want["max_short_power"], f
    assert abs(r["lra_lu"] - W.lra(want)) <= 1e-9 and abs(r["lra_lu"] - want_lra) <= 1.0
    assert abs(r["lra_low_lufs"] - (-0.691 + 10.0 * np.log10(want["low_power"]))) <= 1e-9
    assert abs(r["lra_high_lufs"] - (-0.691 + 10.0 * np.log10(want["high_power"]))) <= 1e-9
    assert abs(r["max_short_term_lufs"] - (-0.691 + 10.0 * np.log10(want["max_short_power"]))) <= 1e-9
    assert r["max_momentary_lufs"] == -0.691 + 10.0 * np.log10(r["max_block_power"])
    for f in FIELDS:
        if f != "short_offset":
            assert res[1][f] == og[0][f], f
    album, awant = res[2], W.gate(st2 + other.want["ST"])
    assert W.gates_are_clear(awant, st2 + other.want["ST"])
    for f in W.COUNTS:
        assert album[f] == awant[f], f
    for f in W.POWERS:
        assert abs(album[f] - awant[f]) <= W.TOL * awant["max_short_power"], f
    assert abs(album["lra_lu"] - W.lra(awant)) <= 1e-9
    assert album["max_momentary_lufs"] == max(res[0]["max_momentary_lufs"], res[1]["max_momentary_lufs"])
    # nothing to measure
    assert api.scan_loudness([], loudness_range=True) == []
    alone = api.scan_loudness([b"not a WavPack file " * 8], 0, album=True, loudness_range=True)
    assert alone[0] is None and alone[1]["shorts"] == 0 and alone[1]["lra_lu"] == 0.0
    assert alone[1]["lra_low_lufs"] == float("-inf") == alone[1]["max_short_term_lufs"]
