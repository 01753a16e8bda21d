"""GPU: the PCM kernels on their magnitude seams (tests/magnitude_vectors.py), bit-exact
against the oracle on every kernel route, and -- on the lane route -- which kernel
decoded each block (WVG_ST_REDONE: handed back by the lane kernel).

A kernel that is wrong on a seam stays CRC-clean when the block is handed back anyway,
so parity alone cannot say that a seam was reached: the hand-back checks below tie every
band of magnitude_vectors.BANDS to the kernel that decoded it.  The conditions on the
corpus itself (every band populated) are in test_magnitude_host.py.

What this corpus found: hybrid27_bitrate, block 1 (medians climbing from 2^17 under 27-bit
data) decoded wrong on the lane route from frame 50 on -- the first group of SPLIT words with
no escape in it, where a 16-bit unary count ran past the 12 bits left in the window and the
replay by the checked words did not happen (wv_lane.h lmerge; DESIGN.md, lane kernel)."""
import collections
import contextlib
import os

import numpy as np
import pytest

from tests import magnitude_vectors as M
from tests.test_gpu_parity import ROUTE_VARS, ROUTES
from wavpackdecoder_amd._lib import WVG_ST_REDONE, WVG_ST_TIMEOUT

pytestmark = pytest.mark.gpu

CORPUS = M.corpus()
CORRUPT = M.corrupt_variants()
ALL = [(f.name, f.data) for f in CORPUS] + CORRUPT
SWEEPS = [(f.name, f.data) for f in CORPUS if f.group == "sweep" or f.name == "hybrid_sweep_bitrate"]
ROUTE_NAMES = ("2wave", "generic", "pipe", "lane")
TOP_BAND = len(M.BANDS) - 1

Decoded = collections.namedtuple("Decoded", "open_ok exception frames crc_errors status_or samples block_status")


@contextlib.contextmanager
def _route_env(route):
    env = {k: ROUTES[route].get(k, "0") for k in ROUTE_VARS}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _collect(b, idx, out, nblocks_known=True):
    st = b.block_status()
    res, at = [], 0
    for i in idx:
        if i < 0:
            res.append(Decoded(False, 0, 0, 0, 0, None, None))
            continue
        r, info = b.result(i), b.infos[i]
        n = r.frames * info.reduced_channels
        res.append(Decoded(True, r.exception, r.frames, r.crc_errors, r.status_or,
                           out[info.out_offset: info.out_offset + n].copy(),
                           st[at: at + r.num_blocks].copy() if nblocks_known else None))
        at += r.num_blocks
    return res


_PER_FILE = {}


def per_file(batch_cls, route, chunk):
    """{name: Decoded} of every file (chunk 37: the sweeps) decoded alone in its batch on
    `route`, once a module (one batch object a route, reset between files)"""
    key = (route, chunk)
    if key not in _PER_FILE:
        with _route_env(route):
            b = batch_cls(chunk)
        got = {}
        for name, data in (ALL if chunk == 4096 else SWEEPS):
            b.reset()
            i = b.add_file(data)
            if i >= 0:
                b.decode()
                out = b.download()
            got[name] = _collect(b, [i], out if i >= 0 else None)[0]
        b.close()
        _PER_FILE[key] = got
    return _PER_FILE[key]


def _assert_parity(name, data, chunk, g):
    ref = M.reference(name, data, chunk)
    if ref.status == -2:
        assert not g.open_ok, name
        return
    assert g.open_ok, name
    assert not (g.status_or & WVG_ST_TIMEOUT), name  # never a reference outcome
    if ref.status == -3:
        assert g.exception == 1, name
        return
    assert g.exception == 0, name
    assert g.frames == ref.frames, name
    assert g.crc_errors == ref.crc_errors, name
    np.testing.assert_array_equal(g.samples, ref.samples, err_msg=name)


@pytest.mark.parametrize("chunk", [4096, 37])
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_every_route_matches_the_oracle(route, chunk, gpu_batch_cls):
    """Every corpus file and corrupt variant (chunk 37, call seams inside the blocks: the
    sweeps), alone in its batch: the oracle's open / exception outcome, frames, crc_errors
    and samples; the lossless files also equal their source array (zeros over a block the
    reference mutes), a pin that does not pass through the oracle."""
    got = per_file(gpu_batch_cls, route, chunk)
    files = ALL if chunk == 4096 else SWEEPS
    assert len(got) == len(files)
    for name, data in files:
        _assert_parity(name, data, chunk, got[name])
    for f in CORPUS:
        if f.pcm is not None and f.name in got:
            np.testing.assert_array_equal(got[f.name].samples, M.expected_output(f), err_msg=f.name)


def test_lane_whole_corpus_in_one_batch(gpu_batch_cls):
    """All files in one batch under set_kernel("lane"): the bands sit side by side in one
    wave (a wave takes its word path from its largest median), in the host's lane order;
    every file decodes as it did alone."""
    alone = per_file(gpu_batch_cls, "lane", 4096)
    b = gpu_batch_cls(4096)
    b.set_kernel("lane")
    idx = [b.add_file(d) for _, d in ALL]
    b.decode()
    out = b.download()
    res = _collect(b, idx, out, nblocks_known=False)
    b.close()
    for (name, data), g in zip(ALL, res):
        a = alone[name]
        assert (g.open_ok, g.exception, g.frames, g.crc_errors) == (a.open_ok, a.exception, a.frames,
                                                                    a.crc_errors), name
        _assert_parity(name, data, 4096, g)
        if g.open_ok and not g.exception:
            np.testing.assert_array_equal(g.samples, a.samples, err_msg=name)


def test_lane_four_ladders_in_flight(gpu_batch_cls):
    """four batches of the steady ladder (each in another file order) decode at once on the
    lane kernel with no sync in between; every file comes back as its source array"""
    ladder = [f for f in CORPUS if f.group == "ladder"]
    batches = []
    for k in range(4):
        order = ladder[k::4] + ladder[(k + 1) % 4::4] + ladder[(k + 2) % 4::4] + ladder[(k + 3) % 4::4]
        if k & 1:
            order.reverse()
        b = gpu_batch_cls(4096)
        b.set_kernel("lane")
        idx = [b.add_file(f.data) for f in order]
        assert min(idx) >= 0
        b.upload()
        batches.append((b, idx, order))
    for b, _, _ in batches:
        b.decode()
    for b, _, _ in batches:
        b.sync()
    for b, idx, order in batches:
        out = b.download()
        for i, f in zip(idx, order):
            r, info = b.result(i), b.infos[i]
            assert (r.exception, r.crc_errors, r.frames) == (0, 0, M.FRAMES), f.name
            assert not (r.status_or & WVG_ST_TIMEOUT), f.name
            np.testing.assert_array_equal(out[info.out_offset: info.out_offset + f.pcm.size], f.pcm.reshape(-1),
                                          err_msg=f.name)
        b.close()


# ---- which kernel decoded it (lane route, one file a batch: blocks in file order) ----
def _lane_blocks(batch_cls, files):
    """(file, block number, start band, REDONE) of every block of `files` on the lane route"""
    got = per_file(batch_cls, "lane", 4096)
    for f in files:
        med = M.block_start_medians(f.data)
        st = got[f.name].block_status
        assert st is not None and len(st) == len(med), f.name
        for k, (m, s) in enumerate(zip(med, st)):
            yield f, k, M.band_of(m), bool(s & WVG_ST_REDONE)


def _share_table(rows):
    """{band: (redone, blocks)} and its one-line rendering"""
    t = {k: [0, 0] for k in range(len(M.BANDS))}
    for _, _, band, redone in rows:
        t[band][0] += redone
        t[band][1] += 1
    text = "  ".join(f"{M.band_name(k)}: {r}/{n}" for k, (r, n) in t.items())
    return t, text


def test_lane_hands_back_from_2_29(gpu_batch_cls):
    """(a) a lossless block that starts at or above 2^29 is decoded by the fallback
    (wv_lane.h:1583, at its first group)"""
    lossless = [f for f in CORPUS if f.pcm is not None]
    n = 0
    for f, k, band, redone in _lane_blocks(gpu_batch_cls, lossless):
        if band == TOP_BAND:
            assert redone, (f.name, k)
            n += 1
    assert n >= 8


def test_lane_hands_back_every_muted_block(gpu_batch_cls):
    """(b) a mute is the fallback's to report (lane_finish: mx > ml || mn < -ml): every block
    of the files whose limit wrapped negative, and the one block with a sample past the limit"""
    for name in ("mute_mag31", "mute_mag30_hybrid"):
        rows = list(_lane_blocks(gpu_batch_cls, [M.by_name(name)]))
        assert len(rows) == M.NBLOCKS and all(r[3] for r in rows), name
    for f in CORPUS:
        if f.name.endswith("_past_limit"):
            rows = list(_lane_blocks(gpu_batch_cls, [f]))
            assert rows[M.MUTE_BLOCK][3], f.name


def test_lane_keeps_the_blocks_on_the_mute_limit(gpu_batch_cls):
    """samples of magnitude exactly 2^k + 2 are not a mute: the block holding them stays on
    the lane kernel (steady 13-bit noise, no escapes after the first block) -- `>=` in
    lane_finish would hand it back and still decode it exactly"""
    for f in CORPUS:
        if f.name.endswith("_on_limit"):
            rows = list(_lane_blocks(gpu_batch_cls, [f]))
            t, text = _share_table(rows[1:])
            assert not rows[M.MUTE_BLOCK][3], (f.name, text)


def test_lane_decodes_the_bands_below_2_28(gpu_batch_cls, capsys):
    """(c) in each band below 2^28 at least half of the steady-ladder blocks that start in
    it stay on the lane kernel (first blocks aside: zero medians give escapes); (d) the
    share handed back, band by band, is in the message and printed"""
    ladder = [f for f in CORPUS if f.group == "ladder"]
    rows = [r for r in _lane_blocks(gpu_batch_cls, ladder) if r[1] > 0]
    t, text = _share_table(rows)
    with capsys.disabled():
        print("\nlane hand-backs (REDONE / blocks) by start band, steady ladder without first blocks:\n  " + text)
        for grp in ("sweep", "burst", "hybrid", "mute"):
            print(f"  {grp}: " + _share_table(_lane_blocks(gpu_batch_cls, [f for f in CORPUS if f.group == grp]))[1])
    for k, (lo, hi) in enumerate(M.BANDS):
        if hi <= 1 << 28:
            redone, n = t[k]
            assert n >= 2, (M.band_name(k), text)
            assert 2 * (n - redone) >= n, (M.band_name(k), text)
