"""CPU: the loudness code of wv_loud.h as the host runs it (wvg_loudness_filter / _weights /
_ints / _gate) against tests/loudness_vectors.py, the restatement that never restarts the
filter, uses no fused multiply-add and sums with math.fsum.  The GPU runs the same header;
test_gpu_loudness.py compares the two bit for bit.

    python -m tests.test_loudness_host
prints d, the measured error the tolerance is made from (loudness_vectors.TOL)."""
import ctypes
import math
import struct

import numpy as np
import pytest

from tests import loudness_vectors as V
from wavpackdecoder_amd import _lib, api

R = _lib.lib().wvg_loudness_run_steps()


def _ulps(a, b):
    ia, ib = (struct.unpack("<q", struct.pack("<d", v))[0] for v in (a, b))
    return abs(ia - ib)


@pytest.fixture(scope="module")
def corpus():
    """the host corpus and its restated records, made once"""
    return [(name, x, k, mask, V.measure(x, k, V.RATE, mask)) for name, x, k, mask in V.host_corpus(R)]


def test_run_steps_is_one_of_the_three():
    assert R in (1, 2, 4)
    assert V.ABS_GATE == float.fromhex("0x1.f791ec6e1d5b7p-24")
    assert V.TOL <= 2.0 ** -30


# ---- filter ----
def test_filter_at_48000_is_the_standards_table():
    cf, S = api.loudness_filter(48000)
    assert S == 4800
    for got, want in zip(cf, V.BS1770_48K):
        assert abs(got - want) <= 1e-14, (got, want)


@pytest.mark.parametrize("rate", [6000, 8000, 44100, 352800])
def test_filter_against_the_restatement(rate):
    cf, S = api.loudness_filter(rate)
    want, wS = V.design(float(rate))
    assert S == wS == (rate + 5) // 10
    for got, w in zip(cf, want):
        assert _ulps(float(got), w) <= 4, (rate, got, w)


@pytest.mark.parametrize("rate", [5999, 3072001, 0, -1])
def test_filter_rate_limits(rate):
    cf, S = np.zeros(7), ctypes.c_int32(-7)
    assert _lib.lib().wvg_loudness_filter(rate, cf.ctypes.data, ctypes.byref(S)) == _lib.WVG_ERR_ARG
    assert S.value == -7 and not cf.any()
    with pytest.raises(ValueError):
        api.loudness_filter(rate)


def test_filter_limits_themselves_are_designed():
    for rate in (6000, 3072000):
        cf, S = api.loudness_filter(rate)
        assert S == (rate + 5) // 10 and np.isfinite(cf).all()


# ---- weights ----
@pytest.mark.parametrize("nch,mask,want", [
    (1, 0x4, [1.0]), (2, 0x3, [1.0, 1.0]), (2, 0x30, [1.0, 1.0]), (1, 0x8, [1.0]),
    (6, 0x3F, [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]),
    (6, 0x60F, [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]),       # FL FR FC LFE SL SR: the side pair
    (6, 0, [1.0] * 6),
    (4, 0x33, [1.0, 1.0, 1.41, 1.41]),
    (8, 0x3F, [1.0, 1.0, 1.0, 0.0, 1.41, 1.41, 1.0, 1.0]),  # more channels than bits
    (3, 0x80000008, [0.0, 1.0, 1.0]),
    (8, 0x63F, [1.0, 1.0, 1.0, 0.0, 1.41, 1.41, 1.41, 1.41]),
])
def test_weights(nch, mask, want):
    assert api.loudness_weights(nch, mask).tolist() == want == V.weights(nch, mask)


def test_weights_arguments():
    L, w = _lib.lib(), np.zeros(256)
    assert L.wvg_loudness_weights(0, 0, w.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_weights(256, 0, w.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_weights(2, 0, None) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_weights(255, 0x3F, w.ctypes.data) == 0 and w[255] == 0.0 and w[254] == 1.0


# ---- the host code against the restatement ----
def test_corpus_covers_what_it_claims(corpus):
    S = 800
    assert V.host_frames(R) == [4 * S - 1, 4 * S, 4 * S + 1, 5 * S - 1, 5 * S, 7 * S, 7 * S + 1, (4 * R + 5) * S + 137]
    for nch in (1, 2):
        assert {x.shape[0] for _, x, _, _, _ in corpus if x.shape[1] == nch} >= set(V.host_frames(R))
    assert {x.shape[1] for _, x, _, _, _ in corpus} == {1, 2, 3, 6, 17}
    assert {k for _, _, k, _, _ in corpus} == {7, 15, 23, 31}
    for name, x, k, _, _ in corpus:
        if name[0].isdigit():  # the noise files: both rails
            assert x.min() == -(1 << k) and x.max() == (1 << k) - 1, name
    # the gates have work: some file loses blocks to each of them
    assert any(w["abs_blocks"] < w["blocks"] for *_, w in corpus)
    assert any(0 < w["gated_blocks"] < w["abs_blocks"] for *_, w in corpus)


def test_no_block_power_is_near_a_gate(corpus):
    for name, _, _, _, want in corpus:
        assert V.gates_are_clear(want), name


def test_host_code_against_the_restatement(corpus):
    worst = 0.0
    for name, x, k, mask, want in corpus:
        rec, blocks = api.loudness_ints(x, k, V.RATE, mask)
        assert int(rec["block_offset"]) == 0
        worst = max(worst, V.check(rec, blocks, want, name))
    print(f"d = {worst:.3e}")


def test_below_one_block_and_zeros(corpus):
    by = {name: (x, k, mask, want) for name, x, k, mask, want in corpus}
    short = next(n for n in by if n.endswith(f"_{4 * 800 - 1}"))
    rec, blocks = api.loudness_ints(by[short][0], by[short][1], V.RATE)
    assert len(blocks) == 0 and int(rec["blocks"]) == 0 and float(rec["power"]) == 0.0
    assert float(rec["max_block_power"]) == 0.0 and int(rec["step_frames"]) == 800
    x, k, mask, want = by["zeros"]
    rec, blocks = api.loudness_ints(x, k, V.RATE)
    assert int(rec["blocks"]) == len(blocks) == x.shape[0] // 800 - 3 > 0
    assert (int(rec["abs_blocks"]), int(rec["gated_blocks"])) == (0, 0)
    assert (float(rec["power"]), float(rec["ungated_power"]), float(rec["max_block_power"])) == (0.0, 0.0, 0.0)
    assert not blocks.any()


def test_the_tail_is_never_read(corpus):
    """frames past nsteps * S do not change a bit of the result"""
    name, x, k, mask, _ = next(c for c in corpus if c[0].startswith("2ch") and c[1].shape[0] == (4 * R + 5) * 800 + 137)
    rec, blocks = api.loudness_ints(x, k, V.RATE)
    y = x.copy()
    y[(4 * R + 5) * 800:] = 12345
    rec2, blocks2 = api.loudness_ints(y, k, V.RATE)
    assert rec.tobytes() == rec2.tobytes() and blocks.tobytes() == blocks2.tobytes()
    rec3, blocks3 = api.loudness_ints(x[:(4 * R + 5) * 800], k, V.RATE)
    assert rec.tobytes() == rec3.tobytes() and blocks.tobytes() == blocks3.tobytes()


# ---- the gate on hand-made lists ----
def _gate_check(P, what):
    rec, want = api.loudness_gate(P), V.gate(list(P))
    for f in ("blocks", "abs_blocks", "gated_blocks"):
        assert int(rec[f]) == want[f], (what, f)
    top = want["max_block_power"]
    for f in ("power", "ungated_power", "max_block_power"):
        assert abs(float(rec[f]) - want[f]) <= V.TOL * top, (what, f, float(rec[f]), want[f])
    assert (int(rec["block_offset"]), int(rec["step_frames"]), int(rec["channels"])) == (0, 0, 0)
    return rec


def test_gate_empty_and_below_abs():
    rec = _gate_check([], "empty")
    assert (int(rec["blocks"]), float(rec["power"]), float(rec["max_block_power"])) == (0, 0.0, 0.0)
    rec = _gate_check([V.ABS_GATE, V.ABS_GATE / 2, 0.0, 1e-12], "all at or below ABS")
    assert (int(rec["blocks"]), int(rec["abs_blocks"]), int(rec["gated_blocks"])) == (4, 0, 0)
    assert float(rec["power"]) == 0.0 == float(rec["ungated_power"]) and float(rec["max_block_power"]) == V.ABS_GATE


def test_gate_one_block():
    rec = _gate_check([0.25], "one")
    assert (float(rec["power"]), float(rec["ungated_power"]), int(rec["gated_blocks"])) == (0.25, 0.25, 1)
    rec = _gate_check([math.nextafter(V.ABS_GATE, 1.0)], "just above ABS")
    assert int(rec["gated_blocks"]) == 1


def test_gate_relative_removes_blocks():
    P = [0.5, 0.4, 0.01, 0.02, 1e-5, 1e-9, 0.3]   # ungated mean over six, rel = 0.0205...: three stay
    rec = _gate_check(P, "relative")
    assert (int(rec["blocks"]), int(rec["abs_blocks"]), int(rec["gated_blocks"])) == (7, 6, 3)
    assert float(rec["power"]) == pytest.approx(0.4, rel=1e-15)


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 1000])
def test_gate_across_the_partial_sum_seams(n):
    rng = np.random.default_rng(n)
    P = 10.0 ** rng.uniform(-9.0, 0.0, size=n)
    want = V.gate(P.tolist())
    assert 0 < want["gated_blocks"] < want["abs_blocks"] < n
    assert all(abs(p - g) > V.GATE_MARGIN * g for p in P for g in (V.ABS_GATE, want["rel"]))
    _gate_check(P, n)
    # the order is fixed and data independent: partial l adds P_l, P_(l+64), ..., then the butterfly
    part = [0.0] * 64
    for j, p in enumerate(P.tolist()):
        if p > V.ABS_GATE:
            part[j % 64] = part[j % 64] + p
    m = 32
    while m:
        part = [part[i] + part[i ^ m] for i in range(64)]
        m >>= 1
    assert float(api.loudness_gate(P)["ungated_power"]) == part[0] / want["abs_blocks"]


def test_gate_arguments():
    L, rec, p = _lib.lib(), np.zeros(1, dtype=_lib.LOUDNESS_DTYPE), np.ones(4)
    assert L.wvg_loudness_gate(p.ctypes.data, -1, rec.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_gate(None, 4, rec.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_gate(p.ctypes.data, 4, None) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_gate(None, 0, rec.ctypes.data) == 0


# ---- known answers ----
def test_997_hz_full_scale_sine_reads_minus_3_01():
    """BS.1770's own statement: a 0 dBFS 997 Hz sine in one channel reads -3.01 LKFS"""
    t = np.arange(48000)
    x = np.round(((1 << 23) - 1) * np.sin(2.0 * np.pi * 997.0 * t / 48000.0)).astype(np.int32).reshape(-1, 1)
    rec, _ = api.loudness_ints(x, 23, 48000)
    assert int(rec["blocks"]) == 7 == int(rec["gated_blocks"])
    assert abs(V.lufs(float(rec["power"])) - (-3.01)) <= 0.01


def test_ebu_tech_3341_case_1():
    """a stereo 1 kHz sine at -23 dBFS reads -23.0 +/- 0.1 LUFS"""
    t = np.arange(2 * 48000)
    a = 10.0 ** (-23.0 / 20.0) * 32768.0
    ch = np.round(a * np.sin(2.0 * np.pi * 1000.0 * t / 48000.0)).astype(np.int32)
    rec, _ = api.loudness_ints(np.stack([ch, ch], axis=1), 15, 48000, 0x3)
    assert abs(V.lufs(float(rec["power"])) - (-23.0)) <= 0.1


# ---- the host entry's hygiene ----
def _raw(x, k, rate, mask, cap, guard=8):
    """wvg_loudness_ints with guard words around `out` and `blocks`"""
    frames, nch = x.shape
    out = np.full(64 + 2 * guard, 0xA5, dtype=np.uint8)
    blk = np.full(cap + 2 * guard, -7.25, dtype=np.float64)
    rc = _lib.lib().wvg_loudness_ints(x.ctypes.data, frames, nch, k, rate, mask, out.ctypes.data + guard,
                                      blk.ctypes.data + 8 * guard, cap)
    assert (out[:guard] == 0xA5).all() and (out[-guard:] == 0xA5).all()
    assert (blk[:guard] == -7.25).all() and (blk[guard + cap:] == -7.25).all()
    return rc, out[guard:-guard].copy().view(_lib.LOUDNESS_DTYPE)[0], blk[guard: guard + cap]


def test_host_entry_guards_space_and_arguments():
    x = V.noise(7 * 800 + 1, 2, 15, 5)
    rec, blocks = api.loudness_ints(x, 15, V.RATE)
    rc, rec2, blk2 = _raw(x, 15, V.RATE, 0, 4)
    assert rc == 0 and rec2.tobytes() == rec.tobytes() and blk2.tobytes() == blocks.tobytes()
    rc, _, blk3 = _raw(x, 15, V.RATE, 0, 3)
    assert rc == _lib.WVG_ERR_SPACE and (blk3 == -7.25).all()
    L, o, b = _lib.lib(), np.zeros(1, dtype=_lib.LOUDNESS_DTYPE), np.zeros(8)
    args = lambda **kw: [kw.get("src", x.ctypes.data), kw.get("frames", x.shape[0]), kw.get("nch", 2), kw.get("k", 15),
                         kw.get("rate", V.RATE), 0, kw.get("out", o.ctypes.data), kw.get("blk", b.ctypes.data),
                         kw.get("cap", 8)]
    assert L.wvg_loudness_ints(*args()) == 0
    for bad in ({"nch": 0}, {"nch": 256}, {"k": 16}, {"k": 0}, {"rate": 5999}, {"rate": 3072001}, {"frames": -1},
                {"src": None}, {"out": None}, {"blk": None}, {"cap": -1}):
        assert L.wvg_loudness_ints(*args(**bad)) == _lib.WVG_ERR_ARG, bad
    assert L.wvg_loudness_ints(*args(src=None, frames=0, blk=None, cap=0)) == 0 and int(o[0]["blocks"]) == 0


def test_source_at_every_int_alignment():
    x = V.noise(5 * 800, 1, 23, 9)
    want_rec, want_blk = api.loudness_ints(x, 23, V.RATE)
    raw = np.zeros(x.size + 8, dtype=np.int32)
    base = (-(raw.ctypes.data // 4)) % 4  # the first int on a 16-byte boundary
    for a in range(4):
        raw[:] = 0x55555555
        raw[base + a: base + a + x.size] = x.reshape(-1)
        view = raw[base + a: base + a + x.size].reshape(-1, 1)
        assert (view.ctypes.data // 4) % 4 == a
        o, b = np.zeros(1, dtype=_lib.LOUDNESS_DTYPE), np.zeros(2)
        assert _lib.lib().wvg_loudness_ints(view.ctypes.data, x.shape[0], 1, 23, V.RATE, 0, o.ctypes.data,
                                            b.ctypes.data, 2) == 0
        assert o[0].tobytes() == want_rec.tobytes() and b.tobytes() == want_blk.tobytes(), a


if __name__ == "__main__":
    d = 0.0
    for name, x, k, mask in V.host_corpus(R):
        rec, blocks = api.loudness_ints(x, k, V.RATE, mask)
        di = V.worst(blocks, V.measure(x, k, V.RATE, mask)["P"])
        print(f"{name:28s} {di:.3e}")
        d = max(d, di)
    print(f"R = {R}: d = {d:.3e} (2^{math.log2(d):.1f}), 64 d = 2^{math.log2(64 * d):.1f}")
