"""CPU side of the DSD seam cases (tests/dsd_vectors.py): what the reference does with
each file, the plain reader and the host build of the decode core against it, and the
conditions that keep the GPU tests (test_gpu_dsd_seams.py) from passing on a seam
nothing stands on.

Measured with the oracle: a mode-3 payload cut by up to 6 bytes (stereo) still decodes
to its source -- the last bytes only pin the final interval --, further cuts fail the
block's CRC; none of the mode-3 cuts is NONDET.  A mode-1 payload cut by 1 or 2 bytes
decodes too; deeper cuts end in a CRC error or in a failed symbol (index >= total),
and only the failed symbols are NONDET (the reference's 0x55 fill covers less than the
call there)."""
import numpy as np
import pytest

from tests import dsd_vectors as D
from tests.emu import emu as E

ST_NONDET = 0x80

CASES = D.cases()
NAMES = [c.name for c in CASES]
WELL = [c for c in CASES if c.well_formed]
OTHER = [c for c in CASES if not c.well_formed]
EXACT = ("declined", "failed", "max_prob", "rle_after")

_EVENTS = {}


def events(c):
    """the plain reader's (bytes, events) of a case's first block, computed once"""
    if c.name not in _EVENTS:
        _EVENTS[c.name] = D.read_block(c.data)
    return _EVENTS[c.name]


def _emu_equals_oracle(c, chunk=4096):
    """as test_emu_parity.check"""
    r = D.reference(c, chunk)
    n, out, crc, st = E.decode(c.data, chunk)
    if r.status != 0:
        assert n == r.status, c.name
        return r, st
    assert n == r.frames, c.name
    assert crc == r.crc_errors, c.name
    if not (st & ST_NONDET):
        np.testing.assert_array_equal(out, r.samples, err_msg=c.name)
    return r, st


@pytest.mark.parametrize("c", WELL, ids=lambda c: c.name)
def test_well_formed_cases_round_trip(c):
    r = D.reference(c)
    assert r.status == 0 and r.crc_errors == 0 and r.frames == c.nframes
    np.testing.assert_array_equal(r.samples, D.expected_output(c))
    got, ev = events(c)
    if c.kind == "chain":  # (the reader takes the first block: the first half of the frames)
        assert got == c.source[:len(c.source) // 2]
    else:
        assert got == c.source and ev["crc_ok"] and ev["left"] == 0
    _, st = _emu_equals_oracle(c)
    assert not (st & ST_NONDET), c.name
    _emu_equals_oracle(c, 5)  # 5-frame calls: every call seam inside the block


@pytest.mark.parametrize("c", OTHER, ids=lambda c: c.name)
def test_declined_and_damaged_cases(c):
    r, st = _emu_equals_oracle(c)
    got, ev = events(c)
    if c.kind == "declined":
        assert r.status == -2 and got is None and ev["declined"]  # the only block: the open fails
    else:
        assert r.status == 0 and r.frames == c.nframes and got is not None
        # the reference's verdict follows from what the reader saw: a failed symbol or a crc mismatch
        assert r.crc_errors == (0 if ev["crc_ok"] else 1), c.name
    _emu_equals_oracle(c, 5)


def test_nondet_cap():
    """The truncated cases that must compare in full do."""
    full = {1: 0, 3: 0}
    for c in OTHER:
        if "_tail_cut" not in c.name:
            continue
        _, st = _emu_equals_oracle(c)
        if c.mode == 3:
            assert not (st & ST_NONDET), c.name
        full[c.mode] += not (st & ST_NONDET)
    assert full[1] >= 2 and full[3] >= 8 + 3 + 2


# ---- coverage: counted by the plain reader, never by the writers ----
@pytest.mark.parametrize("c", CASES, ids=NAMES)
def test_case_shows_the_events_its_name_promises(c):
    _, ev = events(c)
    for k, v in c.expect.items():
        if k in EXACT:
            assert ev.get(k) == v, (c.name, k, ev.get(k))
        elif k == "codes":
            assert set(v) <= ev["codes"], (c.name, sorted(ev["codes"]))
        else:
            assert ev.get(k, 0) >= v, (c.name, k, ev.get(k, 0))
    assert all(s in D.SEAMS for s in c.seams), c.name


def _on(seam, **kw):
    out = [c for c in CASES if seam in c.seams and all(getattr(c, k) == v for k, v in kw.items())]
    assert out, (seam, kw)
    return out


def test_every_seam_is_populated():
    assert all(src for src in D.SEAMS.values())
    for seam in D.SEAMS:
        _on(seam)
    ok3 = [c for c in WELL if c.mode == 3 and c.kind == "ok"]
    filt = [events(c)[1]["filt"] for c in ok3]
    # mode 3: every byte value in every filter, both channels; every factor; every rate
    for ch in (0, 1):
        seen = {(k, f[ch][k]) for f in filt if len(f) > ch for k in range(5)}
        assert seen >= {(k, b) for k in range(5) for b in D.FILTER_BYTES}, ch
        assert {f[ch][5] for f in filt if len(f) > ch} >= set(D.FACTORS), ch
    assert any(f[0][:5] != f[1][:5] and f[0][5] != f[1][5] for f in filt if len(f) == 2)
    assert any(f[c][4] == 0xFF and f[c][3] == 0 for f in filt for c in range(len(f)))
    assert ((255, 0, 255, 0, 255, 0x7FFF), (1, 128, 127, 255, 0, -0x8000)) in [tuple(f) for f in filt]
    assert {events(c)[1]["rate_i"] for c in _on("m3_rate_i")} == set(D.RATES)
    for layout in D.LAYOUTS:
        assert {c.nframes for c in _on("m3_frames", layout=layout)} == set(D.M3_FRAMES)
        assert _on("m3_improbable", layout=layout) and _on("m3_high_eq_low", layout=layout)
        assert _on("m3_tail", layout=layout) and _on("m1_tail", layout=layout)
        assert _on("m3_chain", layout=layout) and _on("m1_chain", layout=layout)
        assert _on("m1_reload", layout=layout) and _on("m1_reload_short", layout=layout)
        assert _on("m1_big_bin", layout=layout, kind="ok") and _on("m1_empty_bin", layout=layout)
        assert _on("m1_narrow", layout=layout) and _on("m1_rle_runs", layout=layout)
    assert {c.name for c in _on("m3_tail", layout="s")} == {f"m3_tail_cut{k}_s" for k in range(1, 9)}
    assert {c.kind for c in _on("m3_rate_s")} == {"declined"} and len(_on("m3_rate_s")) == 2
    assert sorted((c.kind, c.layout) for c in _on("m3_length")) == [("declined", "m"), ("declined", "s"), ("ok", "m"),
                                                                   ("ok", "s")]
    # an improbable stream costs the lane window about a byte a decision (the generator's: a bit or less)
    for c in _on("m3_improbable"):
        ev = events(c)[1]
        if c.name.startswith("m3_improbable_then"):
            continue
        assert sum(n * k for n, k in enumerate(ev["renorm"])) * 2 >= ev["decisions"], c.name
    # mode 1: the totals, the frame counts, the reload on both sides of `left >= 4`
    totals = {events(c)[1]["totals"][0] for c in WELL if c.mode == 1 and len(events(c)[1]["totals"]) == 1}
    assert totals >= {1, 2, 3, 255, 256, 257, 1279, 1280}
    codes = set().union(*(events(c)[1]["codes"] for c in _on("m1_entry_0_255") + _on("m1_segment_edges")))
    assert codes >= {0, 15, 16, 239, 240, 255}
    for c in _on("m1_big_bin", kind="ok"):
        t = events(c)[1]["totals"]
        assert max(t) == D.BIG_BIN == 40712 and sorted(t)[:31] == [8] * 31 and sum(t) == 32 * 1280
        assert 5 in {s & 31 for s in c.source}  # the big bin is selected
    (c,) = _on("m1_big_bin", kind="declined")
    assert sum(events(c)[1]["totals"][:6]) + 26 * 8 == 32 * 1280 + 1
    for c in WELL:
        if c.mode == 1 and c.name.endswith("_straddle") and max(events(c)[1]["totals"]) >= 256:
            assert events(c)[1]["reload_ge4"] >= 1 and events(c)[1]["reload_lt4"] == 0, c.name
    assert len(_on("m1_reload_short")) >= 12
    assert {(c.layout, c.nframes) for c in _on("m1_frames")} == \
        {("s", 1), ("s", 7), ("s", 8), ("s", 9), ("m", 15), ("m", 16), ("m", 17), ("fs", 7), ("fs", 8), ("fs", 9)}
    assert {k for c in _on("m1_tail", layout="s") for k in range(1, 10) if c.name == f"m1_tail_cut{k}_s"} == \
        set(range(1, 10))
    assert {c.name for c in _on("m1_raw_length")} == {"m1_raw_plus3_m", "m1_raw_plus4_m", "m1_raw_plus5_m"}
    assert {c.kind for c in _on("m1_index_ge_tot")} == {"damaged"}


def test_collapse_cases_tell_a_three_byte_shift_from_four():
    """after high == low the byte loop runs four times; a reader that stops at three decodes
    the collapse_then_hug cases to other bytes (the plain straddle cases it may well survive:
    the two states differ by 2^-16 of the range)"""
    hug = [c for c in CASES if c.name.startswith("m3_collapse_hug_")]
    assert sorted(c.layout for c in hug) == ["fs", "m", "s"]
    for c in hug:
        assert D.read_block(c.data)[0] == c.source
        got, ev = D.read_block(c.data, renorm_cap=3)
        assert got != c.source and not ev["crc_ok"], c.name
        # ... and take too few bytes to run a lane's window dry: the lane kernels have to keep them
        assert D.bytes_per_refill(events(c)[1]) <= 4, c.name
    keep = [c for c in WELL if c.mode == 3 and c.kind == "ok" and D.bytes_per_refill(events(c)[1]) <= 4]
    assert len(keep) >= 60 and {c.layout for c in keep} == set(D.LAYOUTS)


def test_run_length_tables_are_the_shapes_asked_for():
    def rle(name):
        (c,) = [c for c in CASES if c.name == name]
        return events(c)[1]
    ev = rle("m1_rle_maxp254_s")
    assert ev["max_prob"] == 0xFE and (False, 1) in ev["rle"] and all(n == 1 for _, n in ev["rle"][:-1])
    assert sum(z for z, _ in ev["rle"]) >= 250  # runs of length 1, one code each
    assert rle("m1_rle_maxp1_m")["max_prob"] == 1 and rle("m1_rle_maxp0_s")["max_prob"] == 0
    c = next(c for c in CASES if c.name == "m1_rle_code_eq_maxp_fs")
    assert events(c)[1]["max_prob"] == 17 and 9 in events(c)[1]["codes"] | set(c.source)
    for layout in D.LAYOUTS:
        r = rle(f"m1_rle_steps_{layout}")["rle"]
        # codes 63 and 64, 127 and 128 of the kernel's 64-code steps are zero runs longer than one entry
        for k in (63, 64, 127, 128):
            assert r[k][0] and r[k][1] > 1, (k, r[k])
        assert not r[62][0] and not r[65][0] and not r[126][0] and not r[129][0]
    for name, over in (("m1_rle_overshoot_s", 9), ("m1_rle_overshoot_m", 1)):
        assert rle(name)["rle_overshoot"] == over and rle(name)["rle_after"] == 0
    ev = rle("m1_rle_exact_zero_s")
    assert not ev["rle"][-1][0] and ev["rle"][-1][1] == 1 and ev["rle_after"] == 0  # full on a literal, then the 0
    ev = rle("m1_rle_exact_run_zero_m")
    assert ev["rle"][-1][0] and "rle_overshoot" not in ev and ev["rle_after"] == 0
    assert rle("m1_rle_exact_nonzero_s")["rle_after"] == 1
    ev = rle("m1_rle_early_end_s")
    assert ev["rle"][-1] == (False, 0) and len(ev["rle"]) == 301 and ev["declined"] == "fast"


def test_cases_are_small_and_one_block():
    from tests import vectors as V
    assert 150 <= len(CASES) <= 260
    for c in CASES:
        spans = V.block_spans(c.data)
        assert len(spans) == (2 if c.kind == "chain" else 1), c.name
        per_block = c.nframes // len(spans)
        assert per_block <= 64 or (c.mode == 1 and per_block * D.LAYOUTS[c.layout][1] <= 128), c.name
        assert sum(n for _, n in spans) == len(c.data), c.name
    name, data, source, expect, well_formed = CASES[0]  # a case unpacks as the five fields
    assert (name, data, well_formed) == (CASES[0].name, CASES[0].data, True) and source and expect == {}


def test_splice_forms():
    """odd and even lengths, the large-size form (a 32-bin raw table is 8 KiB), false stereo"""
    from tests import vectors as V
    for layout in D.LAYOUTS:
        nch, wch, fs = D.LAYOUTS[layout]
        for n in (12, 13, 510, 511, 512, 8200, 8201):
            payload = bytes((7 * k + n) & 0xFF for k in range(n))
            f = D.block_file(layout, 3, payload, None, 9)
            ((off, ln),) = V.block_spans(f)
            assert off == 0 and ln == len(f)
            from tests.magnitude_vectors import audio_blocks
            ((flags, subs),) = audio_blocks(f)
            assert subs[D.ID_DSD_BLOCK] == bytes([0, 3]) + payload
            assert bool(flags & 0x40000000) == fs and bool(flags & 4) == (nch == 1)


def test_ptable_init_for_every_rate():
    """dsd_ptable_init (the table every kernel starts a mode-3 block from) for all 256 rate_i,
    reached through the host core: one 16-frame mono block per rate, written from the plain
    init_ptable with filter bytes that spread the table index, must decode to the writer's
    source -- one wrong entry among those a block reads moves a split and the bytes after it"""
    entries = []
    for rate_i in range(256):
        filt = ((37 * rate_i + 11) & 255, (91 * rate_i + 5) & 255, (53 * rate_i) & 255, (17 * rate_i + 200) & 255,
                (29 * rate_i + 77) & 255, D.FACTORS[rate_i % 9])
        payload, src = D.mode3_payload(16, 1, rate_i, (filt,), D.random(900 + rate_i, 0.5))
        data = D.block_file("m", 3, payload, src, 16)
        n, out, crc, st = E.decode(data)
        assert (n, crc, st & ST_NONDET) == (16, 0, 0) and bytes(out.astype(np.uint8)) == src, rate_i
        got, ev = D.read_block(data)
        assert got == src and ev["rate_i"] == rate_i and ev["crc_ok"], rate_i
        entries.append(len(ev["pp"]))
    print("table entries read per block: least", min(entries), "mean", sum(entries) / 256)
    assert min(entries) >= 64  # a quarter of the table in every block (observed: 87 at the least)
    t = D.init_ptable(0)
    assert t[0] == 0x808000 and t[255] == 0x100FFFF - 0x808000
    t = D.init_ptable(255)
    assert t[0] > D.DOWN and t[127] == D.DOWN and t[128] == 0x100FFFF - D.DOWN  # (UP - t[128]) >> 8 == 0: on the rail


@pytest.mark.parametrize("c", CASES, ids=NAMES)
def test_device_framing_parses_the_headers_like_the_host(c):
    """wv_dframe.h's own parse of both headers, run on the host: a block the reference
    sets up (damaged payloads included) is framed on the device with the host framing's
    descriptor, byte for byte; a declined block, a FALSE_STEREO block and a block that
    continues another's state go to the host framing"""
    from tests.test_dframe import check_same
    accepted = check_same(c.data, 4096)
    assert accepted == (c.kind in ("ok", "damaged") and c.layout != "fs"), c.name
