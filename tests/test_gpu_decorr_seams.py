"""GPU: the decorrelation passes where a weight leaves int16 (tests/decorr_vectors.py),
bit-exact against the oracle on every kernel route at each case's own chunk size and at
another one, and -- on the lane route -- which blocks the lane kernel handed back
(WVG_ST_REDONE): exactly those whose weight could leave int16 within a group.

The four kernels re-create the reference's (short) weight stores from the descriptor's
chunk schedule (host core, two-wave, pipelined: a per-lane seam mask) or hand the block
back before a store can matter (lane kernels' wbad()); decorr_vectors.SEAMS names the
lines.  The conditions on the corpus itself (every store site changes a value somewhere,
hug / control never wrap) are in test_decorr_seams_host.py."""
import collections

import numpy as np
import pytest

from tests import decorr_vectors as D
from tests.test_gpu_magnitude import _route_env
from wavpackdecoder_amd._lib import WVG_ST_REDONE, WVG_ST_TIMEOUT

pytestmark = pytest.mark.gpu

CASES = D.cases()
ROUTE_NAMES = ("2wave", "generic", "pipe", "lane")

Decoded = collections.namedtuple("Decoded", "exception frames crc_errors status_or samples block_status")


def other_chunk(c):
    """a second chunk size: the seams fall elsewhere (and, for the stereo cases, 37 has a frame-8
    store in every call where 13 has none)"""
    return 37 if c.chunk >= 1000 else 1000


def _decode(b, data):
    b.reset()
    i = b.add_file(data)
    assert i >= 0
    b.decode()
    out = b.download()
    r, info = b.result(i), b.infos[i]
    n = r.frames * info.reduced_channels
    return Decoded(r.exception, r.frames, r.crc_errors, r.status_or, out[info.out_offset: info.out_offset + n].copy(),
                   b.block_status()[: r.num_blocks].copy())


_PER_FILE = {}


def per_file(batch_cls, route, chunk):
    """{name: Decoded} of every case whose own (or other) chunk size is `chunk` -- at 1000 of every
    case --, each alone in its batch on `route`: one batch object per (route, chunk), once a module"""
    key = (route, chunk)
    if key not in _PER_FILE:
        with _route_env(route):
            b = batch_cls(chunk)
        _PER_FILE[key] = {c.name: _decode(b, c.data) for c in CASES
                          if chunk == 1000 or chunk in (c.chunk, other_chunk(c))}
        b.close()
    return _PER_FILE[key]


def _assert_parity(c, chunk, g):
    ref = D.reference(c, chunk)
    assert ref.status == 0, c.name
    assert not (g.status_or & WVG_ST_TIMEOUT), c.name
    assert g.exception == 0, c.name
    assert g.frames == ref.frames, c.name
    assert g.crc_errors == ref.crc_errors, (c.name, chunk)
    np.testing.assert_array_equal(g.samples, ref.samples, err_msg=f"{c.name} chunk {chunk}")


CHUNKS = sorted({c.chunk for c in CASES} | {other_chunk(c) for c in CASES})


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_every_route_matches_the_oracle(route, chunk, gpu_batch_cls):
    """every case at its own chunk size and at one other: the oracle's frames, crc_errors and
    samples; at its own chunk size a CRC-clean case also equals the plain reader's samples (a pin
    that does not pass through the oracle)"""
    got = per_file(gpu_batch_cls, route, chunk)
    assert got
    for c in CASES:
        if c.name not in got:
            continue
        _assert_parity(c, chunk, got[c.name])
        if chunk == c.chunk and c.clean:
            assert got[c.name].crc_errors == 0, c.name
            np.testing.assert_array_equal(got[c.name].samples, D.expected(c).samples, err_msg=c.name)


def test_lane_whole_corpus_in_one_batch(gpu_batch_cls):
    """every case in one batch of chunk size 1000 under set_kernel("lane"): wrapping, hugging and
    clamping blocks side by side in one wave; every file decodes as it did alone"""
    alone = per_file(gpu_batch_cls, "lane", 1000)
    sel = CASES
    assert set(alone) == {c.name for c in sel}
    b = gpu_batch_cls(1000)
    b.set_kernel("lane")
    idx = [b.add_file(c.data) for c in sel]
    assert min(idx) >= 0
    b.decode()
    out = b.download()
    for c, i in zip(sel, idx):
        r, info = b.result(i), b.infos[i]
        g = Decoded(r.exception, r.frames, r.crc_errors, r.status_or,
                    out[info.out_offset: info.out_offset + r.frames * info.reduced_channels], None)
        _assert_parity(c, 1000, g)
        np.testing.assert_array_equal(g.samples, alone[c.name].samples, err_msg=c.name)
    b.close()


def _lane_rows(batch_cls):
    """(case, block, reader says a weight could leave int16 in a group, REDONE, status) on the lane route,
    each case at its own chunk size"""
    for c in CASES:
        g = per_file(batch_cls, "lane", c.chunk)[c.name]
        e = D.expected(c)
        assert len(g.block_status) == len(c.blocks), c.name
        for k, st in enumerate(g.block_status):
            yield c, k, e.ghand[k], bool(st & WVG_ST_REDONE), int(st)


def test_lane_hands_back_by_the_weight_and_nothing_else(gpu_batch_cls, capsys):
    """a block is handed back (wbad(): rbad |= 4) when the reader's trace has max(|wA|, |wB|) >
    32767 - 8 * delta at a group start, on the compile-time chains, the run-time chain and the rt3
    pipeline alike; the hug and control blocks -- the same chooser, the same residual magnitudes,
    the weight held on the limit or far under it -- stay on the lane kernel.  The per-case table is
    printed."""
    rows = list(_lane_rows(gpu_batch_cls))
    with capsys.disabled():
        print("\nlane hand-backs (case/block: reader says weight past the limit, REDONE, status):")
        for c, k, want, redone, st in rows:
            print(f"  {c.name}/{k}: {int(want)} {int(redone)} {st:#010x}")
    for c, k, want, redone, st in rows:
        if any(b.sticky for b in c.blocks):
            continue   # (a file with a block that continues the passes is one chain on the wave-per-block kernel)
        if c.group in ("hug", "control"):
            assert not want and not redone, (c.name, k, hex(st))
        elif want:
            assert redone, (c.name, k, hex(st))
    assert sum(1 for r in rows if r[2] and r[3]) >= 30


@pytest.mark.parametrize("c", [c for c in CASES if c.group == "sticky"], ids=lambda c: c.name)
def test_sticky_block_continues_the_stored_weight(c, gpu_batch_cls):
    """the default route (the wave-per-block chain kernel for a block without pass metadata): the second
    block starts from the first block's block-end store, which wrapped"""
    e = D.expected(c)
    assert any(s[2] == "block_end" for s in e.changed), c.name
    for chunk in (c.chunk, other_chunk(c)):
        b = gpu_batch_cls(chunk)
        g = _decode(b, c.data)
        b.close()
        _assert_parity(c, chunk, g)
    np.testing.assert_array_equal(per_file(gpu_batch_cls, "2wave", c.chunk)[c.name].samples, e.samples)
