"""Expected loudness range and short-term powers for the wvg_batch_loudness_range tests: an
independent restatement of include/wvgpu.h's definition in plain Python floats, never taken
from the code under test (nothing here calls the library).

It is built on loudness_vectors.step_energies -- the filter never restarted, no fused
multiply-add, every step's squares summed by math.fsum -- and differs from the library in the
same way further on: a short-term power is one math.fsum over its thirty steps of every
channel, the gates are plain Python, the mean is an fsum, and the two percentiles are
sorted(G)[index] with Tech 3342's / libebur128's index rule.

The tolerance.  d is the largest |ST_library - ST_restated| / (running maximum of ST_restated
up to that value) over the host corpus below (loudness_vectors.worst), measured with
    python -m tests.test_loudness_range_host
which printed  d = 5.891e-15 (2^-47.3)  for the library as built (R = 2).  The noise files read
5.1e-16 or less -- the rounding floor of the same step energies that the block powers are
made of (loudness measured 1.5e-15 for its four-step blocks; a sum of thirty non-negative
numbers does not amplify their relative error, it averages it) -- and the pure tone sets d:
its rounding errors in the recursive filter are systematic, not averaged out.
The four powers of a record are compared
relative to max_short_power: a mean or an order statistic moves by no more than the largest
change of any element.  TOL is 64 x d rounded up to a power of two, the margin for inputs the
corpus lacks; the condition on it is TOL <= 2^-30.
"""
import math

import numpy as np

from tests import loudness_vectors as V

D_MEASURED = 5.891e-15
TOL = 2.0 ** -41          # 64 * D_MEASURED = 3.77e-13 = 2^-41.3, rounded up
assert 64 * D_MEASURED <= TOL <= 2.0 ** -30

ABS_GATE = V.ABS_GATE
RATE = V.RATE             # of the host corpus: S = 800
SHORT_STEPS = 30
GATE_MARGIN = 2.0 ** -20  # no test input has a short-term power this close (relatively) to a gate
POWERS = ("low_power", "high_power", "max_short_power", "ungated_short_power")
COUNTS = ("shorts", "abs_shorts", "gated_shorts")


def low_index(n):
    return (n + 4) // 10


def high_index(n):
    return (19 * (n - 1) + 10) // 20


def gate(ST):
    """the record's fields over a list of short-term powers, and `rel`"""
    above = [p for p in ST if p > ABS_GATE]
    ungated = math.fsum(above) / len(above) if above else 0.0
    rel = 0.01 * ungated
    G = sorted(p for p in above if p > rel)
    n = len(G)
    return {"low_power": G[low_index(n)] if n else 0.0, "high_power": G[high_index(n)] if n else 0.0,
            "max_short_power": max(ST) if len(ST) else 0.0, "ungated_short_power": ungated, "shorts": len(ST),
            "abs_shorts": len(above), "gated_shorts": n, "rel": rel}


def measure(ints, k, rate, mask=0):
    """ints: (frames, channels) int32.  The record's fields, `ST` (the short-term powers) and `rel`."""
    ints = np.asarray(ints)
    frames, nch = ints.shape
    cf, S = V.design(float(rate))
    w = V.weights(nch, mask)
    scale = 2.0 ** -k
    E = [V.step_energies([float(v) * scale for v in ints[:, c].tolist()], cf, S) for c in range(nch)]
    nsteps = frames // S
    ST = [math.fsum(w[c] * e for c in range(nch) for e in E[c][j:j + SHORT_STEPS]) / (SHORT_STEPS * S)
          for j in range(max(0, nsteps - (SHORT_STEPS - 1)))]
    r = gate(ST)
    r["ST"] = ST
    return r


def lra(r):
    """10 log10(high / low), 0.0 when nothing passed the gates"""
    return 10.0 * math.log10(r["high_power"] / r["low_power"]) if r["gated_shorts"] and r["low_power"] > 0 else 0.0


def gates_are_clear(r, ST=None):
    """the precondition of comparing counts exactly: no short-term power near a gate"""
    for p in (r["ST"] if ST is None else ST):
        for g in (ABS_GATE, r["rel"]):
            if g > 0 and abs(p - g) <= GATE_MARGIN * g:
                return False
    return True


def check(rec, shorts, want, what, tol=TOL):
    """a library record and its short-term powers against measure()'s: counts exactly, the series
    by loudness_vectors.worst, the four powers within tol of the largest short-term power"""
    assert gates_are_clear(want), (what, "a short-term power is too close to a gate for exact counts")
    for f in COUNTS:
        assert int(rec[f]) == want[f], (what, f, int(rec[f]), want[f])
    d = V.worst(shorts, want["ST"])
    assert d <= tol, (what, "short-term powers", d)
    top = want["max_short_power"]
    for f in POWERS:
        assert abs(float(rec[f]) - want[f]) <= tol * top, (what, f, float(rec[f]), want[f])
    return d


# ---- signals ----
def jumping(steps, nch, k, seed, S, seg_steps, levels, tail=0):
    """white noise at full scale 2^k whose level takes `levels` in turn, `seg_steps` steps of S
    frames each, over `steps` steps and `tail` more frames"""
    rng = np.random.default_rng(seed)
    frames = steps * S + tail
    env = np.repeat(np.resize(np.asarray(levels, dtype=np.float64), frames // (seg_steps * S) + 1), seg_steps * S)
    x = rng.uniform(-1.0, 1.0, size=(frames, nch)) * env[:frames, None] * float(1 << k)
    return np.clip(np.round(x), -(1 << k), (1 << k) - 1).astype(np.int32)


def steady(steps, nch, k, seed, S, level=0.25, tail=0):
    return jumping(steps, nch, k, seed, S, max(steps, 1), (level,), tail)


def sine_segments(levels_dbfs, rate, seconds=20, freq=1000.0, k=15):
    """Tech 3342's compliance signals: a stereo in-phase sine, one segment per level"""
    t = np.arange(len(levels_dbfs) * seconds * rate)
    amp = np.repeat([10.0 ** (db / 20.0) for db in levels_dbfs], seconds * rate)
    ch = np.round(amp * float(1 << k) * np.sin(2.0 * np.pi * freq * t / rate)).astype(np.int32)
    return np.stack([ch, ch], axis=1)


TECH_3342 = [((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)]

JUMP_LEVELS = (0.5, 0.1, 0.002, 0.00004, 0.25, 0.001)   # the last but two is under the absolute gate


def host_steps():
    """the step counts at which the window code can go wrong (with their tails): one step
    short of a window, one window, two, and a tail that must be ignored"""
    S = (RATE + 5) // 10
    return [(29, S - 1), (30, 0), (31, 0), (33, 137)]


def host_corpus():
    """[(name, ints, k, mask)] at RATE: every step count mono and stereo with the depths taking
    turns, six channels with an LFE, a file whose level jumps so that both gates have work,
    zeros, a file wholly under the absolute gate, loudness's two hard signals, and Tech 3342's
    first compliance signal"""
    S = (RATE + 5) // 10
    ks = (7, 15, 23, 31)
    out = []
    for i, (steps, tail) in enumerate(host_steps()):
        for nch in (1, 2):
            k = ks[(i + nch) % 4]
            out.append((f"{nch}ch_k{k}_{steps}", steady(steps, nch, k, 40 * nch + i, S, tail=tail), k, 0))
    out.append(("6ch_k23_31", steady(31, 6, 23, 77, S), 23, 0x3F))
    out.append(("jumping", jumping(240, 2, 15, 5, S, 40, JUMP_LEVELS), 15, 0))
    out.append(("zeros", np.zeros((33 * S, 2), dtype=np.int32), 15, 0))
    out.append(("minus_80_dbfs", steady(33, 2, 15, 9, S, level=1e-4), 15, 0))
    for name in ("dc_half_scale", "loud_then_silence"):  # loudness's hard inputs for the restarted filter
        out.append((name, V.special(name, 45 * S + 137), 15, 0))
    # a pure tone: its rounding errors are systematic where noise's average out
    out.append(("tech_3342_signal_1", sine_segments(TECH_3342[0][0], RATE), 15, 0x3))
    return out
