"""GPU: the DSD seam cases (tests/dsd_vectors.py; their coverage conditions are in
test_dsd_seams_host.py) on every route, bit-exact against the oracle: output, per-file
crc_errors, the 0x55 mutes, the open verdict of a declined block.

* set_kernel("lane"): wv_dsd1_lane<1/2> (mode 1, 16 lanes a block), dsd3_lanes<1> and
  dsd3_pairs (mode 3); with WVG_DSD3_PAIR=0 (a child process: the knob is read once)
  the one-lane stereo kernel dsd3_lanes<2>;
* set_kernel("two_wave"): the wave-per-block kernels (dsd_simple_wave, dsd_high_wave,
  dsd_high_v2);
* add_files_device: the device framing's own parse of both headers; what it declines
  goes to the host framing and ends as the host framing ends it;
* the two-block chain files: the generic core (decode_dsd_chain) on the crafted block.

The mode-1 row kernel must keep every well-formed block (reloads, the 40,712 bin and
every run-length table included) and hand back exactly the blocks whose symbol fails.
Which mode-3 blocks the lane kernels hand back (a window run dry) depends on the stream:
it is printed here and DESIGN.md has the table as observed.  Asserted is only what follows
from the one-lane kernel's refill schedule: a well-formed block that takes at most 4 bytes
between refills (dsd_vectors.bytes_per_refill) cannot run its window dry, so it is kept --
a lane that decodes such a block wrongly fails the CRC and would hand it back unseen."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dsd_vectors as D
from wavpackdecoder_amd._lib import WVG_ST_NONDET, WVG_ST_REDONE, WVG_ST_TIMEOUT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = D.cases()


def _run(cases, chunk=4096, kernel="lane", device=False):
    """-> per case (samples or None, result or None, info, [block status])"""
    from wavpackdecoder_amd.api import DecodeBatch
    b = DecodeBatch(chunk)
    b.set_kernel(kernel)
    files = [c.data for c in cases]
    if device:
        b.add_files_device(files)
    else:
        for d in files:
            b.add_file(d)
    b.decode()
    out = b.download()
    st = b.block_status()
    got, k = [], 0
    for i in range(len(cases)):
        info = b.infos[i]
        if not info.open_ok:
            got.append((None, None, info, []))
            continue
        r = b.result(i)
        seg = out[info.out_offset: info.out_offset + r.frames * info.reduced_channels].copy()
        got.append((seg, r, info, [int(x) for x in st[k:k + r.num_blocks]] if not device else []))
        k += r.num_blocks
    stats = b.framing_stats() + (b.lane_groups(),)
    b.close()
    return got, stats


def _check(cases, got, chunk=4096):
    for c, (seg, r, info, st) in zip(cases, got):
        ref = D.reference(c, chunk)
        if ref.status == -2:
            assert not info.open_ok, c.name
            continue
        assert info.open_ok and r is not None and not (r.status_or & WVG_ST_TIMEOUT), c.name
        assert ref.status == 0 and r.exception == 0, c.name
        assert r.frames == ref.frames, c.name
        assert r.crc_errors == ref.crc_errors, f"{c.name}: crc_errors {r.crc_errors} vs {ref.crc_errors}, status {st}"
        if c.well_formed:
            assert not (r.status_or & WVG_ST_NONDET), c.name
        if r.status_or & WVG_ST_NONDET:  # (the reference reads the caller's stale buffer there)
            continue
        bad = np.nonzero(seg != ref.samples)[0]
        assert bad.size == 0, f"{c.name}: {bad.size} values differ from index {bad[:1].tolist()}, block status " \
                              f"{[hex(x) for x in st]}"
        if c.well_formed:
            np.testing.assert_array_equal(seg, D.expected_output(c), err_msg=c.name)


@pytest.mark.parametrize("chunk", [4096, 5])
@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
def test_seam_cases_equal_the_oracle(kernel, chunk):
    got, (dev, host, groups) = _run(CASES, chunk, kernel)
    assert dev == 0
    # (bits 9 / 10 of lane_groups: the mode-3 lanes / the mode-1 rows ran)
    assert (groups >> 9) & 3 == (3 if kernel == "lane" else 0), hex(groups)
    _check(CASES, got, chunk)


def test_lane_route_hand_backs():
    from tests.test_dsd_seams_host import events
    got, _ = _run(CASES, 4096, "lane")
    _check(CASES, got)
    table = {}
    for c, (seg, r, info, st) in zip(CASES, got):
        if r is None or c.kind == "chain":
            continue
        redone = bool(st[0] & WVG_ST_REDONE)
        failed = events(c)[1]["failed"]
        if c.mode == 1 and c.well_formed:
            assert not redone, f"{c.name}: a well-formed mode-1 block was handed back, status {hex(st[0])}"
        if c.mode == 1 and failed:
            assert redone, f"{c.name}: a failed symbol ({failed}) was not handed back, status {hex(st[0])}"
        if c.mode == 3 and c.well_formed:
            table[c.name] = redone
            # a fresh block whose CRC is right is handed back only for a dry window; the one-lane
            # kernel's (mono blocks) cannot run dry at 4 bytes or less between refills
            if c.layout != "s" and D.bytes_per_refill(events(c)[1]) <= 4:
                assert not redone, f"{c.name}: handed back with a window that cannot run dry, status {hex(st[0])}"
    assert table
    print("mode-3 hand-backs (lane route):", json.dumps({k: v for k, v in table.items() if v}))
    print("mode-3 kept:", sum(not v for v in table.values()), "of", len(table))


@pytest.mark.parametrize("kernel", ["lane", "two_wave"])
def test_device_framing_route(kernel):
    """every case framed by add_files_device: those it takes decode from its own parse of
    the headers, those it declines end as the host framing ends them"""
    got, (dev, host, groups) = _run(CASES, 4096, kernel, device=True)
    assert (groups >> 9) & 3 == (3 if kernel == "lane" else 0), hex(groups)
    expect_dev = sum(c.kind in ("ok", "damaged") and c.layout != "fs" for c in CASES)
    assert (dev, host) == (expect_dev, len(CASES) - expect_dev)
    _check(CASES, got)
    ref, _ = _run(CASES, 4096, kernel)
    for c, a, b in zip(CASES, got, ref):
        assert (a[0] is None) == (b[0] is None), c.name
        if a[0] is None:
            continue
        assert (a[1].frames, a[1].crc_errors, a[1].exception, a[1].status_or) == \
               (b[1].frames, b[1].crc_errors, b[1].exception, b[1].status_or), c.name
        np.testing.assert_array_equal(a[0], b[0], err_msg=c.name)


_CHILD = r'''
import json, sys
sys.path.insert(0, ROOT)
from tests import dsd_vectors as D
from tests import test_gpu_dsd_seams as T
cases = [c for c in D.cases() if c.mode == 3 and c.layout == "s"]
got, (_, _, groups) = T._run(cases, 4096, "lane")
assert groups & (1 << 9), hex(groups)
T._check(cases, got)
kept = sum(not (st[0] & T.WVG_ST_REDONE) for _, r, _, st in got if r is not None)
# (as test_lane_route_hand_backs: at 4 bytes or less between refills the window cannot run dry)
wrong = [c.name for c, (_, r, _, st) in zip(cases, got)
         if r is not None and c.well_formed and c.kind == "ok" and (st[0] & T.WVG_ST_REDONE)
         and D.bytes_per_refill(D.read_block(c.data)[1]) <= 4]
print(json.dumps({"cases": len(cases), "kept": kept, "wrongly_handed_back": wrong}))
'''


def test_one_lane_stereo_kernel():
    """WVG_DSD3_PAIR=0: the stereo mode-3 cases on dsd3_lanes<2>"""
    env = dict(os.environ, WVG_DSD3_PAIR="0")
    code = "ROOT = " + repr(ROOT) + "\n" + _CHILD
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    n = sum(c.mode == 3 and c.layout == "s" for c in CASES)
    assert d["cases"] == n >= 40 and d["kept"] >= 1 and d["wrongly_handed_back"] == [], d
