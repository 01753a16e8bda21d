"""CPU side of the decorrelation-seam corpus (tests/decorr_vectors.py): the oracle against
the plain reader at each case's own chunk size and at two others, the host build of the
decode core against the oracle, and the conditions that keep the GPU tests
(test_gpu_decorr_seams.py) from passing on stores that change nothing.

Measured with the oracle: a positive term's weight past +-32767 wraps at the next (short)
store and the samples after it depend on the caller's chunk size (the cross_* files decode
CRC-clean at the chunk size they were written for and with CRC errors or mutes at others);
a block written without knowledge of the stores (foreign_*) mutes within a few frames of
the first wrapping store."""
import numpy as np
import pytest

from tests import decorr_vectors as D
from tests.emu import emu as E

ST_NONDET = 0x80

CASES = D.cases()
NAMES = [c.name for c in CASES]
CHUNK_POOL = (4096, 1000, 37, 13)
STORE_SITES = ("call_end", "frame8", "block_end", "mute_call")


def other_chunks(c):
    """two chunk sizes other than the case's own"""
    return [k for k in CHUNK_POOL if k != c.chunk][:2] if c.chunk != 1000 else [37, 13]


def _group(*names):
    out = [c for c in CASES if c.group in names]
    assert out, names
    return out


def _agree(c, chunk):
    ref, got = D.reference(c, chunk), D.expected(c, chunk)
    assert ref.status == 0, c.name   # every case opens and decodes without an exception
    assert ref.frames == got.frames == sum(len(b.words) for b in c.blocks), c.name
    assert ref.crc_errors == got.crc_errors, (c.name, chunk)
    np.testing.assert_array_equal(ref.samples, got.samples, err_msg=f"{c.name} chunk {chunk}")
    # the mute frame: the reader's muting call is zeros in the oracle's output from its first frame on
    at = 0
    for blk, m in zip(c.blocks, got.mute_frame):
        if m is not None:
            a = next(a for a, b in D.calls(len(blk.words), chunk, at) if a <= m < b)
            assert not ref.samples.reshape(-1, c.nch)[at + a: at + len(blk.words)].any(), c.name
        at += len(blk.words)
    return ref, got


@pytest.mark.parametrize("c", CASES, ids=NAMES)
def test_oracle_equals_reader_at_own_chunk(c):
    ref, got = _agree(c, c.chunk)
    if c.group in ("cross_end", "cross_neg", "seam8", "edge", "position", "one_group", "ab", "shifted", "sticky",
                   "hug", "control", "clamp"):
        assert c.clean, c.name
    if c.clean:
        assert ref.crc_errors == 0 and got.mute_frame == [None] * len(c.blocks), c.name


@pytest.mark.parametrize("c", CASES, ids=NAMES)
def test_oracle_equals_reader_at_other_chunks(c):
    own = D.expected(c)
    for chunk in other_chunks(c):
        ref, got = _agree(c, chunk)
        if c.group in ("cross_end", "cross_neg"):
            assert not np.array_equal(got.samples, own.samples), (c.name, chunk)


@pytest.mark.parametrize("c", CASES, ids=NAMES)
def test_host_core_equals_oracle(c):
    for chunk in [c.chunk] + other_chunks(c):
        r = D.reference(c, chunk)
        n, out, crc, st = E.decode(c.data, chunk)
        assert n == r.frames, (c.name, chunk)
        assert crc == r.crc_errors, (c.name, chunk)
        assert not (st & ST_NONDET), c.name
        np.testing.assert_array_equal(out, r.samples, err_msg=f"{c.name} chunk {chunk}")


def _unmuted_difference(c, site):
    """the reader with one store site switched off differs from the full reader in a frame the full reader
    does not mute"""
    full = D.expected(c)
    part = D.expected(c, sites=tuple(s for s in STORE_SITES if s != site))
    f, p = full.samples.reshape(-1, c.nch), part.samples.reshape(-1, c.nch)
    keep = np.ones(len(f), dtype=bool)
    at = 0
    for blk, m in zip(c.blocks, full.mute_frame):
        if m is not None:
            a = next(a for a, b in D.calls(len(blk.words), c.chunk, at) if a <= m < b)
            keep[at + a: at + len(blk.words)] = False
        at += len(blk.words)
    return bool((f[keep] != p[keep]).any())


def test_every_seam_is_live():
    """each store site: a file where dropping that one store changes samples the full decode does not mute
    (so a kernel without it fails the parity tests); the other SEAMS by their own conditions below"""
    assert set(STORE_SITES) | {"lane_wbad", "clamp"} == set(D.SEAMS) and all(D.SEAMS.values())
    for c in CASES:
        assert set(c.seams) <= set(D.SEAMS), c.name
    live = {site: [c.name for c in CASES if site in c.seams and _unmuted_difference(c, site)] for site in STORE_SITES}
    for site in STORE_SITES:
        assert live[site], site
    # what each group is for
    for c in _group("cross_end", "cross_neg", "shifted"):
        assert c.name in live["call_end"], c.name
    for c in _group("seam8"):
        assert (c.name in live["frame8"]) == ("frame8" in c.seams), c.name
        if "frame8" in c.seams:   # only the frame-8 store wraps: the other sites change nothing
            assert {s[2] for s in D.expected(c).changed} == {"frame8"}, c.name
        else:
            assert not D.expected(c).changed, c.name
    assert {c.chunk for c in _group("seam8") if "frame8" in c.seams} >= {16, 1000}   # (16: n >= 16, not n > 16)
    assert sum("frame8" not in c.seams for c in _group("seam8")) >= 4   # chunk 13, cut call, mono, false stereo
    # the two-wave kernel runs the compile-time lists only: one frame-8 file has the default list's shape
    assert any(c.blocks[0].terms == (-2, 3, 2, 18, 18) for c in _group("seam8") if "frame8" in c.seams)
    for grp in ("cross_end", "cross_neg"):
        assert sorted((c.nch, c.chunk) for c in _group(grp)) == [(1, 1000), (1, 4096), (2, 1000), (2, 4096)], grp
    for c in _group("sticky"):
        assert c.name in live["block_end"], c.name
    assert "foreign_sticky_m" in live["mute_call"] and "foreign_sticky_m" in live["block_end"]


def test_edge_files_sit_on_each_side_of_each_edge():
    e = {c.name: c for c in _group("edge")}
    for sign, edge in (("pos", 32767), ("neg", -32768)):
        on, over = D.expected(e[f"edge_{sign}_on"]), D.expected(e[f"edge_{sign}_over"])
        # identity side: a store sees exactly the edge value and keeps it; no store changes anything, and
        # the decode without any store is the same decode
        assert not on.changed and any(s[4] == edge and s[6] == edge for s in on.stores), sign
        none = D.expected(e[f"edge_{sign}_on"], sites=())
        np.testing.assert_array_equal(none.samples, on.samples)
        # one step further: the store wraps it
        first = over.changed[0]
        assert first[4] == edge + (7 if edge > 0 else -7) and first[6] == D.i16(first[4]), sign
        assert _unmuted_difference(e[f"edge_{sign}_over"], "call_end"), sign


def test_one_group_cases_cross_and_store_inside_one_group():
    """at every group start the weight is in int16 (a test for |w| > 32767 at group starts would keep the
    block); the store that wraps it is a call end inside a group, with frames of that group after it"""
    for c in _group("one_group"):
        r = D.expected(c)
        assert r.gmax[0] <= 32767 and r.ghand[0], c.name
        (blk, f, site, _, w, _, w1, _), = r.changed
        assert site == "call_end" and w > 32767 and f % D.GF == 6 and len(c.blocks[0].words) == f + 2
        assert c.chunk % D.GF, c.name
        assert _unmuted_difference(c, "call_end"), c.name
        # the decode of a kernel that makes no store: not muted (it would be handed back for that), in
        # int16 at every group start, and wrong in the block's last frame
        none = D.expected(c, sites=())
        assert none.mute_frame == [None] and none.gmax[0] <= 32767, c.name
        assert none.samples[-1] != r.samples[-1] and np.array_equal(none.samples[:-1], r.samples[:-1]), c.name


def test_ab_cases_wrap_the_channel_they_name():
    for c in _group("ab"):
        ch = D.expected(c).changed
        a = any(s[4] != s[6] for s in ch)
        b = any(s[5] != s[7] for s in ch)
        if c.name.startswith("A_only"):
            assert a and not b, c.name
        elif c.name.startswith("B_only"):
            assert b and not a, c.name
        else:   # both, at different stores
            fa = next(s[1] for s in ch if s[4] != s[6])
            fb = next(s[1] for s in ch if s[5] != s[7])
            assert a and b and fa != fb, c.name
    for name in ("A_only", "B_only", "AB_apart"):   # each with joint stereo off and on
        assert sorted(c.blocks[0].joint for c in _group("ab") if c.name.startswith(name)) == [False, True], name


def test_position_cases_cover_lists_places_and_terms():
    seen = set()
    for c in _group("position"):
        blk = c.blocks[0]
        k, = [i for i, d in enumerate(blk.deltas) if d]
        n = len(blk.terms)
        where = "first" if k == 0 else "last" if k == n - 1 else "middle"
        seen.add((n, where, blk.terms[k]))
        assert all(w == (0, 0) for i, w in enumerate(blk.wbytes) if i != k), c.name   # the rest is transparent
        assert D.expected(c).changed, c.name
    for n in (16, 9, 4):
        assert {w for m, w, _ in seen if m == n} == {"first", "middle", "last"}, n
    assert {t for _, _, t in seen} == {2, 8, 17, 18}   # (term 1: the cross_* and every one-term file)
    assert any(m in (2, 5) for m, _, _ in seen)        # the compile-time lists' shapes


def test_hug_and_control_never_wrap():
    for c in _group("hug"):
        r = D.expected(c)
        assert not r.changed and r.gmax == [32767 - D.GF * 7] and r.ghand == [False], c.name
        for chunk in other_chunks(c):
            assert not D.expected(c, chunk).changed, c.name
    for c in _group("control"):
        r = D.expected(c)
        assert not r.changed and r.ghand == [False] and 16340 - 14 <= r.gmax[0] <= 16340 < 16384, c.name


def test_foreign_cases_mute_after_the_first_wrapping_store():
    for c in _group("foreign"):
        r = D.expected(c)
        first = r.changed[0]
        assert r.mute_frame[0] is not None and first[1] < r.mute_frame[0] <= first[1] + 1000, c.name
        assert r.crc_errors >= 1 and D.reference(c, c.chunk).crc_errors == r.crc_errors, c.name
        # as its encoder believes (no stores) the block decodes clean
        none = D.expected(c, sites=())
        assert none.mute_frame[0] is None and none.crc[0] == c.header_crc[0], c.name


def test_clamp_cases_reach_and_leave_the_clamp():
    """every file, so every term: pushed outward ((w += delta) > 1024 holds and is cut back), inward, and
    outward again (a step from 1024 - delta lands on +-1024 exactly: the frame before the clamp first holds)"""
    for c in _group("clamp"):
        r = D.expected(c)
        assert r.counts["clamp_cut"] >= 8, (c.name, r.counts)
        assert r.counts["clamp_on"] >= 1, (c.name, r.counts)
        assert max(abs(v) for s in r.stores for v in s[4:]) == 1024, c.name
    one = {c.blocks[0].terms[0] for c in _group("clamp") if len(c.blocks[0].terms) == 1}
    assert one == {-1, -2, -3}
    assert any(len(c.blocks[0].terms) == 5 for c in _group("clamp"))   # the default list's shape


def test_wrap32_cases_wrap_int32():
    """2 s0 - s1 (term 17), 3 s0 - s1 (term 18) and the >> 10 of the 64-bit product each leave int32 in a frame
    that is not muted"""
    prod = next(c for c in _group("wrap32") if c.name == "wrap32_t17_product")
    r = D.expected(prod)
    assert r.mute_frame == [None] and r.crc_errors == 0 and r.counts["aw_wrap"] >= 1, r.counts
    assert (1 << 29) < abs(int(r.samples[-1])) <= (1 << 30) + 2   # the last sample is made of the wrapped prediction
    for c in _group("wrap32"):
        if c is prod:
            continue
        blk = c.blocks[0]
        term = blk.terms[0]
        assert D.hist_layout_ok(blk), c.name
        r = D.expected(c)
        out = r.samples.reshape(-1, c.nch).astype(np.int64)
        assert r.mute_frame == [None] and np.abs(out).max() <= (1 << 30) + 2, c.name
        wraps = 0
        for ch in range(c.nch):
            h = [D.exp2s(v) for v in blk.hist[0][ch]] + [int(v) for v in out[:, ch]]
            for s1, s0 in zip(h, h[1:-1]):   # the two values each frame's sample is made of
                v = 2 * s0 - s1 if term == 17 else 3 * s0 - s1
                wraps += v != D.i32(v)
        assert wraps >= (50 if term == 17 else 1), (c.name, wraps)
        assert r.counts["sam_wrap"] == wraps, (c.name, r.counts)   # (the reader's own count of the same thing)
    s = D.cases()
    t17 = next(c for c in s if c.name == "wrap32_t17_s").blocks[0]
    assert D.i32(2 * D.exp2s(t17.hist[0][0][1]) - D.exp2s(t17.hist[0][0][0])) == -(1 << 31)   # INT32_MIN as a sample


def test_chooser_bounds_and_corpus_shape():
    assert len(CASES) <= D.MAX_FILES
    for c in CASES:
        assert 1 <= len(c.blocks) <= 2, c.name
        assert all(len(b.words) <= D.MAX_FRAMES for b in c.blocks), c.name
        assert len(c.data) < 1 << 20, c.name
        out = np.abs(D.expected(c).samples.astype(np.int64)).max()
        res = max(max(abs(w[0]), abs(w[1])) for b in c.blocks for w in b.words)
        if c.group == "wrap32":            # its own limits: the 32-bit container's mute limit, the word coder's width
            assert out <= (1 << 30) + 2 and res <= 1 << 27, c.name
        elif c.name == "foreign_sticky_m":  # (one residual cancels the exploded history the mute left)
            assert out <= D.OUT_MAX and res < 1 << 30, c.name
        else:
            assert out <= D.OUT_MAX and res <= D.RES_MAX, (c.name, out, res)
            assert all(b.mag == D.MAG and (1 << b.mag) + 2 >= 2 * D.OUT_MAX for b in c.blocks), c.name
        from tests.magnitude_vectors import block_start_medians
        assert max(block_start_medians(c.data)) <= D.MED_MAX, c.name
