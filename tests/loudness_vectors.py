"""Expected integrated loudness for the wvg_batch_loudness tests: an independent restatement
of include/wvgpu.h's definition in plain Python floats, never taken from the code under test
(nothing here calls the library).

It differs from the library on purpose where the definition allows a difference to show:
the filter is never restarted (one recurrence over the whole channel, no runs, no warm-up),
products and sums are ordinary `*` and `+` (no fused multiply-add), and every sum -- a
step's squares, a block's steps and channels, the gates' means -- is math.fsum, exact up to
its one final rounding.  So the comparison bounds everything the library's way of computing
adds: the overlap-discard restart, the fma rounding and the order of its sums.

The tolerance.  d is the largest |P_library - P_restated| / (running maximum of P_restated
up to that block) over the host corpus below (the running maximum: after a loud passage
the filter's tail, not the block's own level, sets the error), measured with
    python -m tests.test_loudness_host
which printed  d = 1.512e-15 (2^-49.2)  for the library as built (R = 2) and for a build with
R = 1, and 1.600e-15 for one with R = 4 (the corpus' longest files grow with R): the
rounding floor, with nothing of the restart in it.  D_MEASURED is the largest of the three.
TOL is 64 x d rounded up to a power of two, the margin for inputs the corpus lacks; the
condition on it is TOL <= 2^-30 (4e-9 dB, seven orders under a meter's 0.1 LU).
"""
import math

import numpy as np

D_MEASURED = 1.600e-15
TOL = 2.0 ** -43          # 64 * D_MEASURED = 1.02e-13 = 2^-43.2, rounded up
assert 64 * D_MEASURED <= TOL <= 2.0 ** -30

ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
RATE = 8000               # of the host corpus: S = 800
GATE_MARGIN = 2.0 ** -20  # no test input has a block power this close (relatively) to a gate


def design(fs):
    """b0 b1 b2 a1 a2 c1 c2 and S"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    d = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / d, 2.0 * (K * K - Vh) / d, (Vh - Vb * K / Q + K * K) / d,
             2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    d = 1.0 + K / Q + K * K
    return shelf + [2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d], (int(fs) + 5) // 10


# BS.1770-4, table 1 and table 2 (48 kHz); the RLB numerator is 1, -2, 1
BS1770_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621]


def weights(nch, mask):
    if nch <= 2:
        return [1.0] * nch
    bits = [b for b in range(32) if (mask >> b) & 1]
    w = []
    for c in range(nch):
        b = bits[c] if c < len(bits) else None
        w.append(0.0 if b == 3 else 1.41 if b in (4, 5, 9, 10) else 1.0)
    return w


def step_energies(xs, cf, S):
    """one channel, the recurrence run once over all of it"""
    b0, b1, b2, a1, a2, c1, c2 = cf
    s1 = s2 = t1 = t2 = 0.0
    E = []
    for j in range(len(xs) // S):
        sq = []
        for x in xs[j * S:(j + 1) * S]:
            y1 = b0 * x + s1
            s1 = b1 * x + s2 - a1 * y1
            s2 = b2 * x - a2 * y1
            y2 = y1 + t1
            t1 = t2 - 2.0 * y1 - c1 * y2
            t2 = y1 - c2 * y2
            sq.append(y2 * y2)
        E.append(math.fsum(sq))
    return E


def gate(P):
    """the record's gate fields over a list of block powers"""
    above = [p for p in P if p > ABS_GATE]
    ungated = math.fsum(above) / len(above) if above else 0.0
    rel = 0.1 * ungated
    kept = [p for p in above if p > rel]
    return {"power": math.fsum(kept) / len(kept) if kept else 0.0, "ungated_power": ungated,
            "max_block_power": max(P) if len(P) else 0.0, "blocks": len(P), "abs_blocks": len(above),
            "gated_blocks": len(kept), "rel": rel}


def measure(ints, k, rate, mask=0):
    """ints: (frames, channels) int32.  The record's fields, `P` (the block powers) and `rel`."""
    ints = np.asarray(ints)
    frames, nch = ints.shape
    cf, S = design(float(rate))
    w = weights(nch, mask)
    scale = 2.0 ** -k
    E = [step_energies([float(v) * scale for v in ints[:, c].tolist()], cf, S) for c in range(nch)]
    nsteps = frames // S
    P = [math.fsum(w[c] * e for c in range(nch) for e in E[c][j:j + 4]) / (4 * S) for j in range(max(0, nsteps - 3))]
    r = gate(P)
    r.update(P=P, step_frames=S, channels=nch)
    return r


def lufs(power):
    return -0.691 + 10.0 * math.log10(power) if power > 0 else float("-inf")


def gates_are_clear(r):
    """the precondition of comparing counts exactly: no block power near a gate"""
    for p in r["P"]:
        for g in (ABS_GATE, r["rel"]):
            if g > 0 and abs(p - g) <= GATE_MARGIN * g:
                return False
    return True


def worst(P_got, P_want):
    """max |got - want| / running max of want (0 where want has been 0 throughout and got is 0)"""
    d, top = 0.0, 0.0
    assert len(P_got) == len(P_want)
    for g, w in zip(P_got, P_want):
        top = max(top, w)
        if top == 0.0:
            assert g == 0.0
            continue
        d = max(d, abs(float(g) - w) / top)
    return d


def check(rec, blocks, want, what, tol=TOL):
    """a library record and its block powers against measure()'s: counts exactly, powers
    within tol of the loudest block"""
    assert gates_are_clear(want), (what, "a block power is too close to a gate for exact counts")
    for f in ("blocks", "abs_blocks", "gated_blocks", "step_frames", "channels"):
        assert int(rec[f]) == want[f], (what, f, int(rec[f]), want[f])
    d = worst(blocks, want["P"])
    assert d <= tol, (what, "block powers", d)
    top = want["max_block_power"]
    for f in ("power", "ungated_power", "max_block_power"):
        assert abs(float(rec[f]) - want[f]) <= tol * top, (what, f, float(rec[f]), want[f])
    return d


# ---- signals ----
def noise(frames, nch, k, seed, levels=(1.0, 0.25, 0.02, 0.001), rails=True):
    """white noise whose level changes every 100 ms among `levels` (so both gates have work),
    at full scale 2^k, with both rails present"""
    rng = np.random.default_rng(seed)
    S = (RATE + 5) // 10
    env = np.repeat(rng.choice(levels, size=(frames // S + 1, nch)), S, axis=0)[:frames]
    x = rng.uniform(-1.0, 1.0, size=(frames, nch)) * env * float(1 << k)
    v = np.clip(np.round(x), -(1 << k), (1 << k) - 1).astype(np.int64)
    if rails and frames >= 8:
        v[3, 0], v[frames - 2, nch - 1] = -(1 << k), (1 << k) - 1
    return v.astype(np.int32)


def special(name, frames, k=15):
    """the named hard inputs, stereo at 2^k full scale"""
    rng = np.random.default_rng(len(name))
    fs = float(1 << k)
    if name == "dc_half_scale":  # the worst case for the discarded state: the high pass's input never rests
        x = 0.5 * fs + rng.uniform(-0.2, 0.2, size=(frames, 2)) * fs
    elif name == "loud_then_silence":
        x = rng.uniform(-0.9, 0.9, size=(frames, 2)) * fs
        x[frames // 3:] = 0.0
    elif name == "zeros":
        x = np.zeros((frames, 2))
    else:
        raise KeyError(name)
    return np.round(x).astype(np.int32)


def host_frames(R):
    """the frame counts at which the run code can go wrong (S = 800): below one block, one
    block, the first run whose warm-up starts at 0 and the first that starts past 0, a run
    boundary, and a tail that must be ignored"""
    S = (RATE + 5) // 10
    return [4 * S - 1, 4 * S, 4 * S + 1, 5 * S - 1, 5 * S, 7 * S, 7 * S + 1, (4 * R + 5) * S + 137]


def host_corpus(R):
    """[(name, ints, k, mask)]: every frame count mono and stereo with the depths taking
    turns, every channel count at two lengths, and the special signals"""
    F = host_frames(R)
    ks = (7, 15, 23, 31)
    out = []
    for i, frames in enumerate(F):
        for nch in (1, 2):
            k = ks[(i + nch) % 4]
            out.append((f"{nch}ch_k{k}_{frames}", noise(frames, nch, k, 100 * nch + i), k, 0))
    for nch, mask, fr, k in ((3, 0x7, F[2], 15), (3, 0x7, F[6], 31), (6, 0x3F, F[4], 23), (6, 0x3F, F[7], 7),
                             (17, 0x3F, F[2], 23), (17, 0x60F, F[5], 15)):
        out.append((f"{nch}ch_k{k}_{fr}", noise(fr, nch, k, 1000 + nch + fr), k, mask))
    for name in ("dc_half_scale", "loud_then_silence", "zeros"):
        out.append((name, special(name, F[7]), 15, 0))
    return out
