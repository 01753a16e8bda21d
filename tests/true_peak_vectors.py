"""Expected true-peak records for the wvg_batch_true_peak tests: a restatement of the
definition in include/wvgpu.h in Python integers -- the taps from the formula with `math`,
the records by the plain double loop over frames and phases -- never taken from the code
under test."""
import math

import numpy as np

from wavpackdecoder_amd import _lib

FIELDS = [n for n, _ in _lib.TRUE_PEAK_DTYPE]

# the table as the definition prints it (row 3 is row 1 reversed)
TABLE = [
    [0, 0, 0, 0, 0, 16777216, 0, 0, 0, 0, 0, 0],
    [-27363, 173728, -504882, 1159730, -2707526, 15032977, 4840980, -1734883, 775827, -310666, 82102, -2808],
    [-16528, 173638, -564942, 1343293, -3036105, 10489252, 10489252, -3036105, 1343293, -564942, 173638, -16528],
    [-2808, 82102, -310666, 775827, -1734883, 4840980, 15032977, -2707526, 1159730, -504882, 173728, -27363],
]
ROW2_ABS_SUM = 31247516  # the largest sum of |c|: 1.8625 * 2^24


def _h(t):
    if abs(t) >= 6.0:
        return 0.0
    s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
    return s * math.cos(math.pi * t / 12.0) ** 2


def derive_taps():
    """(the four rows, the smallest distance of a scaled tap of rows 1..3 to a rounding boundary)"""
    rows, margin = [], 1.0
    for q in range(4):
        h = [_h((j - 5) - q / 4.0) for j in range(12)]
        if q == 0:
            assert all(abs(v - (j == 5)) < 1e-15 for j, v in enumerate(h))  # the identity, up to sin(pi n)'s rounding
            rows.append([0] * 5 + [1 << 24] + [0] * 6)
            continue
        total = math.fsum(h)
        scaled = [v / total * (1 << 24) for v in h]
        rows.append([int(math.floor(v + 0.5)) for v in scaled])
        margin = min(margin, min(0.5 - abs(v - math.floor(v + 0.5)) for v in scaled))
    return rows, margin


def oversample_of(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def expected(src, k, oversample):
    """[{field: int}] per channel, in Python integers; src: (frames, channels)"""
    src = np.asarray(src)
    assert src.ndim == 2 and oversample in (1, 2, 4)
    frames, over = src.shape[0], 1 << (k + 24)
    rows = [TABLE[p * 4 // oversample] for p in range(1, oversample)]
    out = []
    for c in range(src.shape[1]):
        x = [0] * 5 + [int(v) for v in src[:, c]] + [0] * 6
        tp, pos, overs, sp, sf = 0, -1, 0, 0, -1
        for n in range(frames):
            m = abs(x[n + 5])
            if sf < 0 or m > sp:
                sp, sf = m, n
            win = x[n: n + 12]
            ys = [x[n + 5] << 24] + [sum(a * b for a, b in zip(row, win)) for row in rows]
            for p, y in enumerate(ys):
                y = abs(y)
                if pos < 0 or y > tp:
                    tp, pos = y, n * oversample + p
                overs += y > over
        out.append({"true_peak": tp, "true_peak_pos": pos, "overs": overs, "sample_peak": sp,
                    "sample_peak_frame": sf, "oversample": oversample, "k": k})
    return out


def check(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert int(g[f]) == w[f], (what, "channel", c, f, int(g[f]), w[f])


def sine_45(frames=200):
    """a full-scale 16-bit sine at fs/4, sampled 45 degrees off its crests"""
    return np.array([[int(round(32767 * math.sin(math.pi / 2 * n + math.pi / 4)))] for n in range(frames)],
                    dtype=np.int32)
