"""Expected level statistics for the wvg_batch_levels tests: Python integers over the source
arrays by the definitions of include/wvgpu.h, never taken from the code under test."""
import numpy as np

from wavpackdecoder_amd import _lib

FIELDS = [n for n, _ in _lib.LEVELS_DTYPE]


def expected(src, k, threshold_q31=0):
    """[{field: int}] per channel, in Python integers"""
    src = np.asarray(src)
    assert src.ndim == 2
    thr = threshold_q31 >> (31 - k)
    out = []
    for c in range(src.shape[1]):
        v = src[:, c].astype(np.int64)
        sq = sum(int(x) * int(x) for x in v)
        act = np.flatnonzero((v > thr) | (v < -thr))
        out.append({
            "min": int(v.min()) if v.size else 0, "max": int(v.max()) if v.size else 0,
            "sum": sum(int(x) for x in v), "sumsq_lo": sq & ((1 << 64) - 1), "sumsq_hi": sq >> 64,
            "clipped": int(((v >= (1 << k) - 1) | (v <= -(1 << k))).sum()), "active": int(act.size),
            "first_active": int(act[0]) if act.size else -1, "last_active": int(act[-1]) if act.size else -1,
        })
    return out


def check(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert int(g[f]) == w[f], (what, "channel", c, f, int(g[f]), w[f])
