"""CPU side of the magnitude-seam corpus (tests/magnitude_vectors.py): what the reference
does with each file, the host build of the decode core against it, and the conditions
that keep the GPU tests (test_gpu_magnitude.py) from passing on an empty band.

Measured with the oracle: the mute compare is `abs(sample) > limit` (UnpackUtils.cs:572,
:620) -- a sample of magnitude 2^k + 2 decodes, 2^k + 3 mutes its block (block
MUTE_BLOCK = 17 of the *_past_limit files: zeros, one CRC error).  A header magnitude of
31 -- and of 30 in a hybrid file, where the limit is doubled -- wraps the limit negative:
every block is muted."""
import collections

import numpy as np
import pytest

from tests import magnitude_vectors as M
from tests.emu import emu as E

ST_NONDET = 0x80

CORPUS = M.corpus()
CORRUPT = M.corrupt_variants()
NAMES = [f.name for f in CORPUS]


def test_exp2s_restatement_matches_the_oracle():
    from oracle import oracle as O
    assert M.EXP2_TABLE == bytes(int(256.0 * (2.0 ** (i / 256.0) - 1.0) + 0.5) for i in range(256))
    L = O.lib()
    for log in range(-8192, 8448):  # the range WordsUtils.cs:631 names
        assert M.exp2s(log) == L.wvo_exp2s(log), log
    assert M.exp2s(0) == 0 and M.exp2s(0x100) == 1 and M.exp2s(0x900) == 256 and M.exp2s(0x1D00) == 1 << 28


def test_block_start_medians_reads_every_block():
    for f in CORPUS:
        med = M.block_start_medians(f.data)
        assert len(med) == M.NBLOCKS, f.name
        assert med[0] == 0, f.name  # a file starts from zero medians
    assert [M.band_of(v) for v in (0, 17, 18, 65, 66, 131, 132, (1 << 17) - 1, 1 << 17, (1 << 29) - 1, 1 << 29,
                                   -5)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 9, 10, 10]


@pytest.mark.parametrize("f", [f for f in CORPUS if f.pcm is not None and not f.muted],
                         ids=lambda f: f.name)
def test_lossless_files_round_trip_through_the_oracle(f):
    r = M.reference(f.name, f.data)
    assert r.status == 0 and r.crc_errors == 0 and r.frames == f.pcm.shape[0]
    np.testing.assert_array_equal(r.samples, f.pcm.reshape(-1))


@pytest.mark.parametrize("name", ["mute_mag31", "mute_mag30_hybrid"])
def test_wrapped_mute_limit_mutes_every_block(name):
    f = M.by_name(name)
    r = M.reference(f.name, f.data)
    assert f.muted == "all"
    assert r.status == 0 and r.frames == M.FRAMES and r.crc_errors == M.NBLOCKS
    assert not r.samples.any()


def test_mag30_lossless_decodes():
    f = M.by_name("mute_mag30_lossless")  # limit 2^30 + 2: not wrapped
    r = M.reference(f.name, f.data)
    assert r.status == 0 and r.crc_errors == 0
    np.testing.assert_array_equal(r.samples, f.pcm.reshape(-1))


@pytest.mark.parametrize("tag", ["s_pos", "m_neg"])
def test_mute_compare_is_strictly_greater(tag):
    """2^k + 2 is exact; 2^k + 3 mutes block MUTE_BLOCK alone (one CRC error)."""
    on = M.by_name(f"mute_k{M.MUTE_K}_{tag}_on_limit")
    past = M.by_name(f"mute_k{M.MUTE_K}_{tag}_past_limit")
    lo, hi = M.MUTE_BLOCK * M.BLOCK, (M.MUTE_BLOCK + 1) * M.BLOCK
    a = np.abs(on.pcm.astype(np.int64))
    assert a.max() == M.MUTE_LIMIT and a[lo:hi].max() == M.MUTE_LIMIT  # the limit is reached, in that block
    assert (on.pcm[lo:hi] == M.MUTE_LIMIT).any() or (on.pcm[lo:hi] == -M.MUTE_LIMIT).any()
    d = np.flatnonzero((on.pcm != past.pcm).reshape(-1))
    assert d.size == 1 and abs(int(past.pcm.reshape(-1)[d[0]])) == M.MUTE_LIMIT + 1
    r = M.reference(on.name, on.data)
    assert r.status == 0 and r.crc_errors == 0
    np.testing.assert_array_equal(r.samples, on.pcm.reshape(-1))
    r = M.reference(past.name, past.data)
    assert r.status == 0 and r.crc_errors == 1 and past.muted == (M.MUTE_BLOCK,)
    got = r.samples.reshape(-1, past.nch)
    assert not got[lo:hi].any()
    np.testing.assert_array_equal(r.samples, M.expected_output(past))


def _emu_equals_oracle(name, data, chunk=4096):
    r = M.reference(name, data, chunk)
    n, out, crc, st = E.decode(data, chunk)
    if r.status != 0:
        assert n == r.status, name  # the same open error / exception
        return st
    assert n == r.frames, name
    assert crc == r.crc_errors, name
    if not (st & ST_NONDET):  # (the reference reads the caller's stale buffer there)
        np.testing.assert_array_equal(out, r.samples, err_msg=name)
    return st


@pytest.mark.parametrize("f", CORPUS, ids=NAMES)
def test_host_core_equals_oracle(f):
    st = _emu_equals_oracle(f.name, f.data)
    assert not (st & ST_NONDET), f.name
    if f.group == "sweep":
        _emu_equals_oracle(f.name, f.data, 37)


@pytest.mark.parametrize("name,data", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_host_core_equals_oracle_on_corrupted_streams(name, data):
    _emu_equals_oracle(name, data)


def test_corrupt_variants_are_the_ones_asked_for():
    n = collections.Counter(name.split("#")[0] for name, _ in CORRUPT)
    assert n == {"ladder_s24_default": 8, "ladder_s26_default": 8, "hybrid26_bitrate": 6}
    for name, data in CORRUPT:
        assert data != M.by_name(name.split("#")[0]).data


# ---- corpus conditions: a band nothing starts in would make the GPU checks vacuous ----
def _band_counts(files, skip_first=False):
    c = collections.Counter()
    for f in files:
        med = M.block_start_medians(f.data)
        c.update(M.band_of(m) for m in (med[1:] if skip_first else med))
    return c


def test_bands_cut_at_every_threshold():
    assert [c for c, _ in M.CUTS] == [18, 66, 132, 1 << 17, 1 << 19, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 29]
    assert all(src for _, src in M.CUTS)
    assert len(M.BANDS) == len(M.CUTS) + 1 and M.BANDS[-1][0] == M.TOP == 1 << 29


def test_every_band_is_populated():
    ladder = [f for f in CORPUS if f.group == "ladder"]
    c = _band_counts(ladder, skip_first=True)  # (a file's first block starts from zero medians: not counted)
    for k in range(len(M.BANDS) - 1):
        assert c[k] >= 2, (M.band_name(k), dict(c))
    sweeps = [f for f in CORPUS if f.group == "sweep"]
    assert len(sweeps) == 10
    for f in sweeps:
        c = _band_counts([f])
        for k in range(len(M.BANDS) - 1):
            assert c[k] >= 1, (f.name, M.band_name(k), dict(c))
    lossless = [f for f in CORPUS if f.pcm is not None]
    assert _band_counts(lossless)[len(M.BANDS) - 1] >= 8  # at or above 2^29
    # the files said to straddle / pass 2^29 do
    c = _band_counts([M.by_name("ladder_s26_default")], skip_first=True)
    assert c[len(M.BANDS) - 1] >= 4 and c[len(M.BANDS) - 2] >= 4
    for name in ("ladder_s27_fast", "ladder_m27", "ladder_m28"):
        med = M.block_start_medians(M.by_name(name).data)
        assert all(M.band_of(m) == len(M.BANDS) - 1 for m in med[2:]), name


def test_corpus_shape():
    assert len(CORPUS) == 2 * len(M.STEREO_BITS) + 2 + len(M.MONO_BITS) + 10 + 1 + 4 * len(M.HYBRID_BITS) + 1 + 7
    for f in CORPUS:
        blocks = M.audio_blocks(f.data)
        assert len(blocks) <= 40, f.name
        if f.pcm is not None:
            assert f.pcm.ndim == 2 and f.pcm.shape[1] == f.nch, f.name
    # the hybrid files start blocks on both sides of the hybrid narrow run's bounds (2^26 mono, 2^28
    # stereo: wv_wave2.h:1101) and past 2^29, where a lossless block would be handed back
    hy = [f for f in CORPUS if f.group == "hybrid"]
    c = _band_counts(hy)
    assert c[M.band_of(1 << 25)] and c[M.band_of(1 << 27)] and c[M.band_of(1 << 28)] and c[len(M.BANDS) - 1]
