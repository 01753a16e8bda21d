"""CPU: the loudness-range code of wv_lra.h as the host runs it (wvg_loudness_range_ints /
_gate) against tests/loudness_range_vectors.py, the restatement built on the never-restarted
filter, math.fsum and sorted().  The GPU runs the same header; test_gpu_loudness_range.py
compares the two bit for bit.

    python -m tests.test_loudness_range_host
prints d, the measured error the tolerance is made from (loudness_range_vectors.TOL)."""
import math

import numpy as np
import pytest

from tests import loudness_range_vectors as W
from tests import loudness_vectors as V
from wavpackdecoder_amd import _lib, api

S = (W.RATE + 5) // 10
DT = _lib.LOUDNESS_RANGE_DTYPE


@pytest.fixture(scope="module")
def corpus():
    """the host corpus and its restated records, made once"""
    return [(name, x, k, mask, W.measure(x, k, W.RATE, mask)) for name, x, k, mask in W.host_corpus()]


def test_the_tolerance_is_the_measured_one():
    assert 64 * W.D_MEASURED <= W.TOL <= 2.0 ** -30
    assert math.log2(W.TOL) == math.ceil(math.log2(64 * W.D_MEASURED))  # rounded up to a power of two, no further
    assert W.ABS_GATE == float.fromhex("0x1.f791ec6e1d5b7p-24")


# ---- the index rule and the selection on hand-made lists ----
def _sorted_want(P):
    """the record by sorted(), the gates in plain Python"""
    return W.gate([float(p) for p in P])


def _gate_exact(P, what):
    """wvg_loudness_range_gate against sorted(): counts, both percentiles and the maximum bit
    for bit; the mean within TOL (its sum is the library's 64 partial sums, not an fsum)"""
    P = np.asarray(P, dtype=np.float64)
    rec, want = api.loudness_range_gate(P), _sorted_want(P)
    for f in W.COUNTS:
        assert int(rec[f]) == want[f], (what, f, int(rec[f]), want[f])
    for f in ("low_power", "high_power", "max_short_power"):
        assert float(rec[f]).hex() == float(want[f]).hex(), (what, f, float(rec[f]), want[f])
    assert abs(float(rec["ungated_short_power"]) - want["ungated_short_power"]) <= W.TOL * max(want["max_short_power"], 0.0)
    assert int(rec["short_offset"]) == 0
    return rec, want


@pytest.mark.parametrize("n", [0, 1, 2, 9, 10, 11, 20, 21])
def test_index_rule(n):
    """distinct values all inside the gates: g[(n + 4) / 10] and g[(19 (n - 1) + 10) / 20]"""
    vals = [0.5 + 0.01 * i for i in range(n)]
    rng = np.random.default_rng(n)
    rec = api.loudness_range_gate(rng.permutation(vals))
    assert int(rec["gated_shorts"]) == n == int(rec["abs_shorts"]) == int(rec["shorts"])
    if n == 0:
        assert (float(rec["low_power"]), float(rec["high_power"]), float(rec["max_short_power"])) == (0.0, 0.0, 0.0)
        return
    lo, hi = {1: (0, 0), 2: (0, 1), 9: (1, 8), 10: (1, 9), 11: (1, 10), 20: (2, 18), 21: (2, 19)}[n]
    assert (W.low_index(n), W.high_index(n)) == (lo, hi)
    assert (float(rec["low_power"]), float(rec["high_power"])) == (vals[lo], vals[hi])
    assert float(rec["max_short_power"]) == vals[-1]


def _lists(n, rng):
    """the synthetic lists of length n: (name, values)"""
    base = 0.125
    low_byte = np.frombuffer((np.frombuffer(np.full(n, base).tobytes(), dtype=np.uint64)
                              + rng.integers(0, 256, size=n, dtype=np.uint64)).tobytes(), dtype=np.float64)
    spread = 10.0 ** rng.uniform(-6.5, 0.0, size=n)         # many exponents, all above ABS
    spread[0] = 1.0                                          # (and a loud one: rel = 0.01 * mean is well inside)
    mixed = 10.0 ** rng.uniform(-12.0, 0.0, size=n)          # some below ABS, some between ABS and rel
    return [("all_equal", np.full(n, 0.3)),
            ("heavy_ties", rng.choice([0.2, 0.21, 0.5, 0.9], size=n)),
            ("low_mantissa_byte", low_byte),
            ("many_exponents", spread),
            ("below_abs_and_between_the_gates", mixed)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_gate_and_selection_against_sorted(n):
    rng = np.random.default_rng(1000 + n)
    for name, P in _lists(n, rng):
        rec, want = _gate_exact(P, (name, n))
        assert W.gates_are_clear(want, [float(p) for p in P]), (name, n)
        if name in ("all_equal", "heavy_ties", "low_mantissa_byte"):
            assert int(rec["gated_shorts"]) == n
    if n >= 255:
        want = _sorted_want(_lists(n, np.random.default_rng(1000 + n))[4][1])
        assert 0 < want["gated_shorts"] < want["abs_shorts"] < n  # both gates had work


def test_gate_only_below_abs_and_only_between_the_gates():
    rec, _ = _gate_exact([W.ABS_GATE, W.ABS_GATE / 2, 0.0, 1e-12], "at or below ABS")
    assert (int(rec["shorts"]), int(rec["abs_shorts"]), int(rec["gated_shorts"])) == (4, 0, 0)
    assert (float(rec["low_power"]), float(rec["high_power"]), float(rec["ungated_short_power"])) == (0.0, 0.0, 0.0)
    assert float(rec["max_short_power"]) == W.ABS_GATE
    # one loud value and many between ABS and rel: only the loud one is in G
    rec, _ = _gate_exact([1.0] + [1e-5] * 40, "between the gates")
    assert (int(rec["abs_shorts"]), int(rec["gated_shorts"])) == (41, 1)
    assert (float(rec["low_power"]), float(rec["high_power"])) == (1.0, 1.0)


def test_gate_arguments():
    L, rec, p = _lib.lib(), np.zeros(1, dtype=DT), np.ones(4)
    assert L.wvg_loudness_range_gate(p.ctypes.data, -1, rec.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_range_gate(None, 4, rec.ctypes.data) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_range_gate(p.ctypes.data, 4, None) == _lib.WVG_ERR_ARG
    assert L.wvg_loudness_range_gate(None, 0, rec.ctypes.data) == 0
    assert L.wvg_loudness_range_gate(p.ctypes.data, 1 << 32, rec.ctypes.data) == _lib.WVG_ERR_SPACE


# ---- the host code against the restatement ----
def test_corpus_covers_what_it_claims(corpus):
    assert W.host_steps() == [(29, S - 1), (30, 0), (31, 0), (33, 137)]
    for nch in (1, 2):
        assert {x.shape[0] for _, x, _, _, _ in corpus if x.shape[1] == nch} >= {st * S + t for st, t in W.host_steps()}
    assert {x.shape[1] for _, x, _, _, _ in corpus} == {1, 2, 6}
    assert {k for _, _, k, _, _ in corpus} == {7, 15, 23, 31}
    by = {name: want for name, _, _, _, want in corpus}
    assert [by[f"1ch_k{k}_{st}"]["shorts"] for k, st in ((15, 29), (23, 30), (31, 31), (7, 33))] == [0, 1, 2, 4]
    j = by["jumping"]
    assert 0 < j["gated_shorts"] < j["abs_shorts"] < j["shorts"]  # both gates have work
    q = by["minus_80_dbfs"]
    assert q["shorts"] == 4 and q["abs_shorts"] == 0 and 0 < q["max_short_power"] < W.ABS_GATE


def test_no_short_term_power_is_near_a_gate(corpus):
    for name, _, _, _, want in corpus:
        assert W.gates_are_clear(want), name


def test_host_code_against_the_restatement(corpus):
    worst = 0.0
    for name, x, k, mask, want in corpus:
        rec, shorts = api.loudness_range_ints(x, k, W.RATE, mask)
        assert int(rec["short_offset"]) == 0
        worst = max(worst, W.check(rec, shorts, want, name))
    print(f"d = {worst:.3e}")


def test_one_step_short_of_a_window_and_zeros(corpus):
    by = {name: (x, k, mask, want) for name, x, k, mask, want in corpus}
    x, k, mask, _ = by["2ch_k23_29"]
    assert x.shape[0] == 29 * S + S - 1
    rec, shorts = api.loudness_range_ints(x, k, W.RATE)
    assert len(shorts) == 0 and rec.tobytes() == np.zeros(1, dtype=DT).tobytes()
    x, k, mask, _ = by["zeros"]
    rec, shorts = api.loudness_range_ints(x, k, W.RATE)
    assert int(rec["shorts"]) == len(shorts) == 4 and not shorts.any()
    assert rec.tobytes() == np.array([(0.0, 0.0, 0.0, 0.0, 4, 0, 0, 0)], dtype=DT).tobytes()
    x, k, mask, _ = by["minus_80_dbfs"]
    rec, shorts = api.loudness_range_ints(x, k, W.RATE)
    assert (int(rec["shorts"]), int(rec["abs_shorts"]), int(rec["gated_shorts"])) == (4, 0, 0)
    assert (float(rec["low_power"]), float(rec["high_power"]), float(rec["ungated_short_power"])) == (0.0, 0.0, 0.0)
    assert 0.0 < float(rec["max_short_power"]) == shorts.max() < W.ABS_GATE


def test_the_tail_is_never_read(corpus):
    """frames past nsteps * S do not change a bit of the result"""
    name, x, k, mask, _ = next(c for c in corpus if c[0].startswith("2ch") and c[1].shape[0] == 33 * S + 137)
    rec, shorts = api.loudness_range_ints(x, k, W.RATE)
    y = x.copy()
    y[33 * S:] = 12345
    rec2, shorts2 = api.loudness_range_ints(y, k, W.RATE)
    assert rec.tobytes() == rec2.tobytes() and shorts.tobytes() == shorts2.tobytes()
    rec3, shorts3 = api.loudness_range_ints(x[:33 * S], k, W.RATE)
    assert rec.tobytes() == rec3.tobytes() and shorts.tobytes() == shorts3.tobytes()


def test_the_record_is_the_gate_over_the_series(corpus):
    """wvg_loudness_range_ints' record is wvg_loudness_range_gate's over its own short-term powers"""
    for name, x, k, mask, _ in corpus:
        rec, shorts = api.loudness_range_ints(x, k, W.RATE, mask)
        assert api.loudness_range_gate(shorts).tobytes() == rec.tobytes(), name


def test_six_channels_weigh_as_loudness_does(corpus):
    name, x, k, mask, want = next(c for c in corpus if c[0] == "6ch_k23_31")
    _, with_lfe = api.loudness_range_ints(x, k, W.RATE, 0x3F)
    y = x.copy()
    y[:, 3] = 0
    _, without = api.loudness_range_ints(y, k, W.RATE, 0x3F)
    assert with_lfe.tobytes() == without.tobytes()     # the LFE weighs 0.0
    _, unweighted = api.loudness_range_ints(x, k, W.RATE, 0)
    assert (unweighted != with_lfe).all()


# ---- Tech 3342's compliance signals ----
@pytest.mark.parametrize("levels,want_lra", W.TECH_3342)
def test_tech_3342_compliance_signals(levels, want_lra):
    """each must read within the +/- 1 LU that Tech 3342 itself allows"""
    x = W.sine_segments(levels, 8000)
    rec, shorts = api.loudness_range_ints(x, 15, 8000, 0x3)
    assert int(rec["shorts"]) == len(levels) * 200 - 29
    got = 10.0 * math.log10(float(rec["high_power"]) / float(rec["low_power"]))
    print(f"{levels}: LRA = {got:.4f} LU")
    assert abs(got - want_lra) <= 1.0, (levels, got)


# ---- the host entry's hygiene ----
def _raw(x, k, rate, mask, cap, guard=8):
    """wvg_loudness_range_ints with guard words around `out` and `shorts`"""
    frames, nch = x.shape
    out = np.full(64 + 2 * guard, 0xA5, dtype=np.uint8)
    st = np.full(cap + 2 * guard, -7.25, dtype=np.float64)
    rc = _lib.lib().wvg_loudness_range_ints(x.ctypes.data, frames, nch, k, rate, mask, out.ctypes.data + guard,
                                            st.ctypes.data + 8 * guard, cap)
    assert (out[:guard] == 0xA5).all() and (out[-guard:] == 0xA5).all()
    assert (st[:guard] == -7.25).all() and (st[guard + cap:] == -7.25).all()
    return rc, out[guard:-guard].copy().view(DT)[0], st[guard: guard + cap]


def test_host_entry_guards_space_and_arguments():
    x = W.steady(32, 2, 15, 5, S, tail=1)
    rec, shorts = api.loudness_range_ints(x, 15, W.RATE)
    rc, rec2, st2 = _raw(x, 15, W.RATE, 0, 3)
    assert rc == 0 and rec2.tobytes() == rec.tobytes() and st2.tobytes() == shorts.tobytes()
    rc, _, st3 = _raw(x, 15, W.RATE, 0, 2)
    assert rc == _lib.WVG_ERR_SPACE and (st3 == -7.25).all()
    L, o, b = _lib.lib(), np.zeros(1, dtype=DT), np.zeros(8)
    args = lambda **kw: [kw.get("src", x.ctypes.data), kw.get("frames", x.shape[0]), kw.get("nch", 2), kw.get("k", 15),
                         kw.get("rate", W.RATE), 0, kw.get("out", o.ctypes.data), kw.get("st", b.ctypes.data),
                         kw.get("cap", 8)]
    assert L.wvg_loudness_range_ints(*args()) == 0
    for bad in ({"nch": 0}, {"nch": 256}, {"k": 16}, {"k": 0}, {"rate": 5999}, {"rate": 3072001}, {"frames": -1},
                {"src": None}, {"out": None}, {"st": None}, {"cap": -1}):
        assert L.wvg_loudness_range_ints(*args(**bad)) == _lib.WVG_ERR_ARG, bad
    assert L.wvg_loudness_range_ints(*args(src=None, frames=0, st=None, cap=0)) == 0 and int(o[0]["shorts"]) == 0


if __name__ == "__main__":
    d = 0.0
    for name, x, k, mask in W.host_corpus():
        rec, shorts = api.loudness_range_ints(x, k, W.RATE, mask)
        di = V.worst(shorts, W.measure(x, k, W.RATE, mask)["ST"])
        print(f"{name:28s} {di:.3e}")
        d = max(d, di)
    print(f"d = {d:.3e} (2^{math.log2(d):.1f}), 64 d = 2^{math.log2(64 * d):.1f}")
