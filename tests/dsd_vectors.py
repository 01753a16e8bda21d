"""DSD blocks placed on the seams of the range coder and the block headers (modes 1 and
3): pure-Python writers whose data follows from a caller-chosen "chooser", a plain
reader of both modes that counts what a stream made the decoder do, and the case table.

Every stream the generator (synth/) writes is random bits behind an all-zero mode-3
header, or a scaled histogram (bin totals <= 1200) for mode 1.  The decoder accepts far
more: live filter bytes and a signed 16-bit factor in every mode-3 block, any rate_i,
bins of total 1 or 40,712, run-length tables of any shape, a `mult == 0` reload with
fewer than 4 bytes left.  SEAMS names each such place and the line that makes it; CASES
puts one-block files (at most 64 frames; 128 mode-1 symbols) on each of them.

The writers and the reader are separate code: the reader restates DsdUtils.cs:149-493
statement by statement and is what the tests count events with, the writers mirror only
the interval arithmetic.  32-bit wrap is explicit (Python integers do not wrap).
"""
import dataclasses
import random as _random

import numpy as np

from synth import wvsynth as S

M32 = 0xFFFFFFFF
ID_DSD_BLOCK = 0xE
MAX_BYTES_PER_BIN = 1280
UP, DOWN = 0x010000FE, 0x00010000
VALUE_ONE = 1 << 20

# csrc/ = wavpackdecoder_amd/csrc/.  key -> where the decoders branch on it
SEAMS = {
    # ---- mode 3 (decode_high)
    "m3_filter_bytes": "DsdUtils.cs:369-373 / wv_framing.cpp:704 / wv_dframe.h:407-416: five bytes << 12, each of "
                       "{0, 1, 0x7F, 0x80, 0xFF} in each of filter1..5",
    "m3_filter5_ff_filter4_0": "DsdUtils.cs:438 the largest first (filter4 - filter5) >> 4; "
                               "wv_dsd_lane.hip:112-114 / :353",
    "m3_filters_per_channel": "DsdUtils.cs:365-378: each channel reads its own seven bytes",
    "m3_factor": "DsdUtils.cs:375-377 / wv_framing.cpp:705-707: 16 bits sign-extended; {0, 1, -1, 0x7FFF, -0x8000}; "
                 "wv_dsd_lane.hip:96-116 24-bit multiplies of filter6 * factor",
    "m3_factor_decay": "DsdUtils.cs:483 factor -= (factor + 512) >> 10: {511, 512, -512, -513} sit on its rounding",
    "m3_rate_i": "DsdUtils.cs:321-341 init_ptable / wv_decode_core.h dsd_ptable_init: "
                 "rate_i in {0, 1, 39, 40, 127, 128, 254, 255}",
    "m3_rate_s": "DsdUtils.cs:354: rate_s != 20 is declined",
    "m3_length": "DsdUtils.cs:348: 13 (mono) / 20 (stereo) bytes after the mode bytes are the least accepted",
    "m3_rails": "DsdUtils.cs:414 / :420: a ptable entry that stopped moving (UP - p < 256; p == DOWN)",
    "m3_improbable": "wv_dsd_lane.hip:189-240 / :400-455: the lane window drained (several bytes a decision)",
    "m3_narrow": "DsdUtils.cs:409: (high - low) >> 8 == 0, split == low",
    "m3_high_eq_low": "wv_dsd_lane.hip:77-81 / :318-319: v_ffbh_u32 of high ^ low == 0, a 4-byte shift",
    "m3_frames": "frame counts 1, 7, 8, 9, 63, 64 (wv_dsd_lane.hip's 8-frame steps)",
    "m3_tail": "DsdUtils.cs:424: the byte loop stopped by the end of data (payload cut by 1..8 bytes)",
    "m3_chain": "wv_decode.hip decode_dsd_chain: the crafted block decoded by the generic core",
    # ---- mode 1 (decode_fast)
    "m1_total_small": "wv_dsd1_lane.hip:212-218 the reciprocal of a bin total of 1 (l = 0), 2, 3",
    "m1_total_pow2": "wv_dsd1_lane.hip:214-217 totals 255 / 256 / 257 around a power of two",
    "m1_total_1280": "DsdUtils.cs:146 totals 1279 / 1280, the most a lone bin may hold",
    "m1_entry_0_255": "DsdUtils.cs:281-284: code 0 (no summed_probabilities[code - 1]) and code 255",
    "m1_segment_edges": "wv_dsd1_lane.hip:297-325: entries 15/16 and 239/240, cnt == 0, one segment with all the mass, "
                        "alternating zero entries",
    "m1_big_bin": "DsdUtils.cs:216 the budget is the sum over bins: 40,712 beside 31 bins of 8; one more is declined",
    "m1_empty_bin": "DsdUtils.cs:257 summed_probabilities[255] == 0 -> return 0",
    "m1_index_ge_tot": "DsdUtils.cs:278 index >= total -> return 0 (all-0xFF value bytes)",
    "m1_reload": "DsdUtils.cs:262-274 / wv_dsd1_lane.hip:283-295: mult == 0, four more value bytes",
    "m1_reload_short": "DsdUtils.cs:264: fewer than 4 bytes left, the value kept",
    "m1_rle_max_prob": "DsdUtils.cs:171-191: max_probability 0, 1, 0xFE; a code equal to it",
    "m1_rle_runs": "wv_dsd1_lane.hip:180-192: runs of length 1; runs in codes 63|64 and 127|128 of the 64-code steps",
    "m1_rle_overshoot": "DsdUtils.cs:184: a run longer than the entries left",
    "m1_rle_exact": "DsdUtils.cs:193: a table that fills exactly, then 0 (taken) or a non-zero byte (declined)",
    "m1_rle_early_end": "DsdUtils.cs:189-193: a 0 code before the table is full (declined)",
    "m1_raw_length": "DsdUtils.cs:196 / :231: a raw table with 3, 4, 5 bytes after it",
    "m1_narrow": "wv_dsd1_lane.hip:343-347: high - low < 256 entering a symbol; high == low after one",
    "m1_frames": "wv_dsd1_lane.hip:358-390: 1, 7, 8, 9 frames stereo; 15, 16, 17 mono; 7, 8, 9 false stereo",
    "m1_tail": "DsdUtils.cs:295: the byte loop stopped by the end of data (payload cut by 1..9 bytes)",
    "m1_chain": "wv_decode.hip decode_dsd_chain: the crafted block decoded by the generic core",
}


def s32(v: int) -> int:
    v &= M32
    return v - (1 << 32) if v & 0x80000000 else v


# =====================================================================================
# choosers: f(low, high, split-or-mult, probabilities, index) -> bit / symbol
#   mode 3: probabilities is the 9-bit weight of a 1 (ptable[pp] >> 16), bit 1 takes
#           [low, split], bit 0 [split + 1, high];
#   mode 1: probabilities is the bin's 256 entries, symbol c takes
#           [low + summed[c - 1] * mult, low + summed[c] * mult - 1].
# =====================================================================================
def random(seed: int, p_one: float = 0.5):
    rng = _random.Random(seed)

    def f(low, high, x, probs, index):
        if isinstance(probs, int):
            return 1 if rng.random() < p_one else 0
        live = [c for c in range(256) if probs[c]]
        return live[rng.randrange(len(live))]
    return f


def probable(low, high, x, probs, index):
    if isinstance(probs, int):
        return 1 if (x - low + 1) >= (high - x) else 0
    return max(range(256), key=lambda c: (probs[c], -c))


def improbable(low, high, x, probs, index):
    if isinstance(probs, int):
        return 0 if (x - low + 1) >= (high - x) > 0 else 1
    return min((c for c in range(256) if probs[c]), key=lambda c: (probs[c], c))


def straddle(seed: int):
    """the bit / symbol whose interval holds both B - 1 and B, B = high & 0xFF000000: the
    range shrinks without its top bytes ever agreeing, down to high - low < 256 (mode 3)
    or below the bin's total (mode 1: mult == 0); a random choice where no interval does"""
    rnd = random(seed)

    def f(low, high, x, probs, index):
        B = high & 0xFF000000
        if low >= B:
            return rnd(low, high, x, probs, index)
        if isinstance(probs, int):
            if x >= B:
                return 1
            if x + 1 <= B - 1:
                return 0
            return rnd(low, high, x, probs, index)
        tot = sum(probs)
        ia, ib = (B - 1 - low) // x, (B - low) // x
        if ib < tot:
            run = 0
            for c in range(256):
                run += probs[c]
                if ia < run:
                    return c if ib < run else rnd(low, high, x, probs, index)
        return rnd(low, high, x, probs, index)
    return f


def collapse_then_hug(seed: int, hug: int = 40):
    """mode 3: `straddle` until the range has collapsed (high == low: the four-byte shift leaves
    low 0, high 0xFFFFFFFF), then a 1 and `hug` times the upper part: the value ends just
    under that first split, 0xFFFFFF * p.  A decoder that shifted only three bytes there
    compares the value's top 24 bits with 0xFFFF * p and takes the 1 for a 0."""
    st = straddle(seed)
    left = [0]

    def f(low, high, x, probs, index):
        if index and low == 0 and high == M32:
            left[0] = hug
            return 1
        if left[0]:
            left[0] -= 1
            return 0
        return st(low, high, x, probs, index)
    return f


def edges(low, high, x, probs, index):
    """mode 1: the first and the last non-zero entry of each 16-entry segment, in turn"""
    cand = []
    for s in range(16):
        live = [c for c in range(16 * s, 16 * s + 16) if probs[c]]
        if live:
            cand += [live[0], live[-1]]
    return cand[index % len(cand)]


def switch(first, then, at: int):
    """`first` for decisions [0, at), `then` from there"""
    return lambda low, high, x, probs, index: (first if index < at else then)(low, high, x, probs, index)


def fixed(symbols, then=None):
    """the listed bits / symbols, then `then`"""
    return lambda low, high, x, probs, index: (symbols[index] if index < len(symbols)
                                               else then(low, high, x, probs, index))


# =====================================================================================
# writers
# =====================================================================================
def init_ptable(rate_i: int, rate_s: int = 20) -> list:
    """DsdUtils.cs:321-341"""
    table = [0] * 256
    value, rate = 0x808000, rate_i << 8
    for _ in range((rate + 128) >> 8):
        value += (DOWN - value) >> 8
    for i in range(128):
        table[i] = value
        table[255 - i] = 0x100FFFF - value
        if value > 0x010000:
            rate += (rate * rate_s + 128) >> 8
            for _ in range((rate + 64) >> 7):
                value += (DOWN - value) >> 8
    return table


class _Filter:
    """one channel of decode_high's filter state (DsdUtils.cs:431-441, :483), 32-bit wrap explicit"""

    def __init__(self, b5, factor):
        self.f1, self.f2, self.f3, self.f4, self.f5 = (b << 12 for b in b5)
        self.f6 = 0
        self.factor = s32((factor & 0xFFFF) << 16) >> 16
        self.byte = 0
        self.start()

    def start(self):
        self.value = s32(self.f1 - self.f5 + (s32(self.f6 * self.factor) >> 2))

    def pp(self):
        return (self.value >> 8) & 255

    def step(self, bit):
        f0 = -1 if bit else 0
        v = s32(self.value + s32(self.f6 * 8))
        self.byte = ((self.byte << 1) | (f0 & 1)) & 0xFF
        self.factor = s32(self.factor + ((((v ^ f0) >> 31) | 1) & ((v ^ s32(v - s32(self.f6 * 16))) >> 31)))
        self.f1 = s32(self.f1 + (s32((f0 & VALUE_ONE) - self.f1) >> 6))
        self.f2 = s32(self.f2 + (s32((f0 & VALUE_ONE) - self.f2) >> 4))
        self.f3 = s32(self.f3 + (s32(self.f2 - self.f3) >> 4))
        self.f4 = s32(self.f4 + (s32(self.f3 - self.f4) >> 4))
        v = s32(self.f4 - self.f5) >> 4
        self.f5 = s32(self.f5 + v)
        self.f6 = s32(self.f6 + (s32(v - self.f6) >> 3))
        self.start()

    def end_frame(self):
        self.factor = s32(self.factor - ((self.factor + 512) >> 10))


def mode3_payload(nframes, wch, rate_i, filt, chooser, rate_s=20):
    """The bytes after the two mode bytes of a mode-3 ID_DSD_BLOCK, and the source bytes
    (wch a frame) they decode to.  filt: per channel (filter1..5 bytes, factor)."""
    o = bytearray([rate_i, rate_s])
    for c in range(wch):
        o += bytes(filt[c][:5]) + (filt[c][5] & 0xFFFF).to_bytes(2, "little")
    sp = [_Filter(filt[c][:5], filt[c][5]) for c in range(wch)]
    ptable = init_ptable(rate_i, rate_s)
    low, high, n = 0, M32, 0
    src = bytearray()
    for _ in range(nframes):
        for q in sp:
            q.start()
        for _ in range(8):
            for q in sp:
                pp = q.pp()
                p16 = ptable[pp] >> 16
                split = (low + ((high - low) >> 8) * p16) & M32
                bit = chooser(low, high, split, p16, n)
                if split == high:
                    bit = 1  # (bit 0's interval is empty)
                n += 1
                if bit:
                    high = split
                    ptable[pp] += (UP - ptable[pp]) >> 8
                else:
                    low = split + 1
                    ptable[pp] += (DOWN - ptable[pp]) >> 8
                while not ((high ^ low) & 0xFF000000):
                    o.append(high >> 24)
                    high = ((high << 8) | 0xFF) & M32
                    low = (low << 8) & M32
                q.step(bit)
        for q in sp:
            src.append(q.byte)
            q.end_frame()
    o += low.to_bytes(4, "big")
    return bytes(o), bytes(src)


def rle_table(prob, max_prob, breaks=(), overshoot=0, tail=b"\0"):
    """run-length coding of the probabilities (DsdUtils.cs:171-191): a zero run starts a
    new code at every entry in `breaks` and where a code is full; the last run is written
    `overshoot` longer than the entries left; `tail` follows the last code"""
    o, i, n = bytearray(), 0, len(prob)
    brk = set(breaks)
    while i < n:
        if prob[i]:
            assert prob[i] <= max_prob
            o.append(prob[i])
            i += 1
            continue
        z = 1
        while i + z < n and not prob[i + z] and z < 255 - max_prob and (i + z) not in brk:
            z += 1
        i += z
        if i == n and overshoot:
            assert z + overshoot <= 255 - max_prob
            z += overshoot
        o.append(max_prob + z)
    return bytes(o) + tail


def mode1_payload(nsym, wch, history_bits, prob, chooser, rle_max_prob=None, rle_breaks=(), rle_overshoot=0,
                  rle_tail=b"\0"):
    """The bytes after the two mode bytes of a mode-1 ID_DSD_BLOCK, and the source bytes
    they decode to (fewer than nsym where a symbol selected an empty bin).  prob: bins x 256
    entries, flat.  rle_max_prob: the run-length coding with that max_probability."""
    bins = 1 << history_bits
    prob = list(prob)
    assert len(prob) == bins * 256
    o = bytearray([history_bits])
    if rle_max_prob is None:
        o += bytes([0xFF]) + bytes(prob)
    else:
        o += bytes([rle_max_prob]) + rle_table(prob, rle_max_prob, rle_breaks, rle_overshoot, rle_tail)
    rows = [prob[b * 256:(b + 1) * 256] for b in range(bins)]
    sums = []
    for r in rows:
        run, acc = 0, []
        for p in r:
            run += p
            acc.append(run)
        sums.append(acc)
    low, high, p0, p1 = 0, M32, 0, 0
    src = bytearray()
    for n in range(nsym):
        tot = sums[p0][255]
        if not tot:
            break
        mult = (high - low) // tot
        if not mult:
            o += low.to_bytes(4, "big")  # pins the old interval; the decoder reads four new bytes
            low, high = 0, M32
            mult = high // tot
        code = chooser(low, high, mult, rows[p0], n)
        assert rows[p0][code]
        if code:
            low = (low + sums[p0][code - 1] * mult) & M32
        high = (low + rows[p0][code] * mult - 1) & M32
        src.append(code)
        if wch == 1:
            p0 = code & (bins - 1)
        else:
            p0, p1 = p1, code & (bins - 1)
        while not ((high ^ low) & 0xFF000000):
            o.append(high >> 24)
            high = ((high << 8) | 0xFF) & M32
            low = (low << 8) & M32
    o += low.to_bytes(4, "big")
    return bytes(o), bytes(src)


# =====================================================================================
# the block around a payload
# =====================================================================================
def _subblock(ident: int, data: bytes) -> bytes:
    """id, length in words, the LARGE (3 length bytes) and ODD forms"""
    words = (len(data) + 1) // 2
    idb = ident | (0x40 if len(data) & 1 else 0)
    head = bytes([idb | 0x80, words & 0xFF, (words >> 8) & 0xFF, words >> 16]) if words > 255 else bytes([idb, words])
    return head + data + (b"\0" if len(data) & 1 else b"")


def replace_dsd(data: bytes, block: int, dsd: bytes) -> bytes:
    """the file with block number `block`'s ID_DSD_BLOCK data replaced by `dsd`, ckSize rewritten
    (the header's crc is of the source bytes: it stays)"""
    from tests import vectors as V
    off, n = V.block_spans(data)[block]
    b = data[off:off + n]
    body, p = bytearray(), 32
    while p < n:
        i, ln, hl = b[p], b[p + 1] << 1, 2
        if i & 0x80:
            ln += (b[p + 2] << 9) + (b[p + 3] << 17)
            hl = 4
        body += _subblock(ID_DSD_BLOCK, dsd) if (i & 0x3F) == ID_DSD_BLOCK else b[p:p + hl + ln]
        p += hl + ln
    hdr = bytearray(b[:32])
    hdr[4:8] = (24 + len(body)).to_bytes(4, "little")
    return data[:off] + bytes(hdr) + bytes(body) + data[off + n:]


def splice(nch, mode, data, payload, false_stereo=False):
    """a one-block DSD file of the frames `data` (frames x nch) whose ID_DSD_BLOCK holds
    `payload` after the mode bytes"""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, nch)
    f = S.encode_dsd(data, S.DsdParams(nch=nch, false_stereo=false_stereo, mode=0, block_samples=data.shape[0]))
    return replace_dsd(f, 0, bytes([0, mode]) + payload)


LAYOUTS = {"s": (2, 2, False), "m": (1, 1, False), "fs": (2, 1, True)}  # nch, coded channels, FALSE_STEREO


def frames_of(source: bytes, layout: str, nframes: int) -> np.ndarray:
    nch, wch, fs = LAYOUTS[layout]
    x = np.zeros((nframes, wch), np.uint8)
    if source is not None and len(source) == nframes * wch:
        x[:] = np.frombuffer(source, np.uint8).reshape(nframes, wch)
    return np.repeat(x, 2, axis=1) if fs else x


def block_file(layout, mode, payload, source, nframes):
    nch, wch, fs = LAYOUTS[layout]
    return splice(nch, mode, frames_of(source, layout, nframes), payload, fs)


# =====================================================================================
# the plain reader (DsdUtils.cs:17-54, :149-493)
# =====================================================================================
def new_events() -> dict:
    return {"reload_ge4": 0, "reload_lt4": 0, "reload_eq4": 0, "reload_at": [], "reload_sym": [], "cnt0": 0,
            "renorm": [0, 0, 0, 0, 0], "renorm_seq": bytearray(), "renorm_cut": 0,
            "narrow": 0, "high_eq_low": 0, "rail_up": 0, "rail_down": 0, "codes": set(), "totals": [], "rle": [],
            "filt": [], "pp": set(), "rate_i": None, "decisions": 0, "declined": None, "failed": None, "crc_ok": None,
            "max_prob": None}


class _Dsd:
    pass


def _renorm(d, ev):
    n = 0
    while not ((d.high ^ d.low) & 0xFF000000) and d.byteptr < len(d.data) and n < d.renorm_cap:
        d.value = ((d.value << 8) | d.data[d.byteptr]) & M32
        d.byteptr += 1
        d.high = ((d.high << 8) | 0xFF) & M32
        d.low = (d.low << 8) & M32
        n += 1
    ev["renorm"][n] += 1
    ev["renorm_seq"].append(n)
    ev[f"renorm{n}"] = ev["renorm"][n]
    if not ((d.high ^ d.low) & 0xFF000000):
        ev["renorm_cut"] += 1


def _init_fast(d, ev):
    """init_dsd_block_fast; False where it declines"""
    data = d.data
    if d.byteptr == len(data):
        return False
    history_bits = data[d.byteptr]
    d.byteptr += 1
    if d.byteptr == len(data) or history_bits > 5:
        return False
    d.bins = 1 << history_bits
    d.lookup = bytearray(d.bins * MAX_BYTES_PER_BIN)
    d.value_lookup = [0] * d.bins
    d.summed = [0] * (256 * d.bins)
    d.prob = [0] * (256 * d.bins)
    max_probability = data[d.byteptr]
    d.byteptr += 1
    ev["max_prob"] = max_probability
    if max_probability < 0xFF:
        outptr, outend = 0, len(d.prob)
        while outptr < outend and d.byteptr < len(data):
            code = data[d.byteptr]
            d.byteptr += 1
            if code > max_probability:
                zcount = code - max_probability
                ev["rle"].append((True, zcount))
                while outptr < outend and zcount > 0:
                    zcount -= 1
                    d.prob[outptr] = 0
                    outptr += 1
                if zcount > 0:
                    ev["rle_overshoot"] = zcount
            elif code != 0:
                ev["rle"].append((False, 1))
                d.prob[outptr] = code
                outptr += 1
            else:
                ev["rle"].append((False, 0))
                break
        if outptr < outend:
            return False
        if d.byteptr < len(data):
            after = data[d.byteptr]
            d.byteptr += 1
            ev["rle_after"] = after
            if after > 0:
                return False
    elif len(data) - d.byteptr > len(d.prob):
        d.prob[:] = data[d.byteptr:d.byteptr + len(d.prob)]
        d.byteptr += len(d.prob)
    else:
        return False
    total, lb = 0, 0
    for bi in range(d.bins):
        s = 0
        for i in range(256):
            s = (s + d.prob[bi * 256 + i]) & 0xFFFF
            d.summed[bi * 256 + i] = s
        ev["totals"].append(s)
        if s:
            total += s
            if total > d.bins * MAX_BYTES_PER_BIN:
                return False
            d.value_lookup[bi] = lb
            for i in range(256):
                for _ in range(d.prob[bi * 256 + i]):
                    d.lookup[lb] = i
                    lb += 1
    if len(data) - d.byteptr < 4 or total > d.bins * MAX_BYTES_PER_BIN:
        return False
    for _ in range(4):
        d.value = ((d.value << 8) | data[d.byteptr]) & M32
        d.byteptr += 1
    d.p0 = d.p1 = 0
    d.low, d.high = 0, M32
    return True


def _decode_fast(d, nframes, mono, ev, out):
    """decode_fast; False at its `return 0`"""
    for n in range(nframes * (1 if mono else 2)):
        p0i = d.p0 * 256
        tot = d.summed[p0i + 255]
        if tot == 0:
            ev["failed"] = "empty_bin"
            return False
        ev["decisions"] += 1
        if d.high - d.low < 256:
            ev["narrow"] += 1
        mult = ((d.high - d.low) & M32) // tot
        if mult == 0:
            ev["reload_at"].append(d.byteptr)
            ev["reload_sym"].append(n)
            ev["reload_eq4"] += len(d.data) - d.byteptr == 4
            if len(d.data) - d.byteptr >= 4:
                ev["reload_ge4"] += 1
                for _ in range(4):
                    d.value = ((d.value << 8) | d.data[d.byteptr]) & M32
                    d.byteptr += 1
            else:
                ev["reload_lt4"] += 1
            d.low, d.high = 0, M32
            mult = d.high // tot
            if mult == 0:
                ev["failed"] = "mult0"
                return False
        index = ((d.value - d.low) & M32) // mult
        if index >= tot:
            ev["failed"] = "index_ge_tot"
            return False
        code = d.lookup[d.value_lookup[d.p0] + index]
        out.append(code)
        if code > 0:
            d.low = (d.low + d.summed[p0i + code - 1] * mult) & M32
        d.high = (d.low + d.prob[p0i + code] * mult - 1) & M32
        d.crc = (d.crc + (d.crc << 1) + code) & M32
        ev["codes"].add(code)
        if not (code & 15):
            ev["cnt0"] += 1
        if d.high == d.low:
            ev["high_eq_low"] += 1
        if mono:
            d.p0 = code & (d.bins - 1)
        else:
            d.p0 = d.p1
            d.p1 = code & (d.bins - 1)
        _renorm(d, ev)
    return True


def _init_high(d, mono, ev):
    """init_dsd_block_high; False where it declines"""
    data = d.data
    if len(data) - d.byteptr < (13 if mono else 20):
        return False
    rate_i, rate_s = data[d.byteptr], data[d.byteptr + 1]
    d.byteptr += 2
    if rate_s != 20:
        return False
    ev["rate_i"] = rate_i
    d.ptable = init_ptable(rate_i, rate_s)
    d.sp = []
    for _ in range(1 if mono else 2):
        b = data[d.byteptr:d.byteptr + 7]
        d.byteptr += 7
        factor = b[5] | (b[6] << 8)
        factor = s32(factor << 16) >> 16
        ev["filt"].append(tuple(b[:5]) + (factor,))
        d.sp.append(_Filter(b[:5], factor))
    d.high, d.low = M32, 0
    for _ in range(4):
        d.value = ((d.value << 8) | data[d.byteptr]) & M32
        d.byteptr += 1
    return True


def _decode_high(d, nframes, ev, out):
    for _ in range(nframes):
        for q in d.sp:
            q.start()
        for _ in range(8):
            for q in d.sp:
                pp = q.pp()
                ev["decisions"] += 1
                ev["pp"].add(pp)
                if d.high - d.low < 256:
                    ev["narrow"] += 1
                split = (d.low + (((d.high - d.low) & M32) >> 8) * ((d.ptable[pp] & M32) >> 16)) & M32
                if d.value <= split:
                    d.high = split
                    step = (UP - d.ptable[pp]) >> 8
                    ev["rail_up"] += step == 0
                    bit = 1
                else:
                    d.low = (split + 1) & M32
                    step = (DOWN - d.ptable[pp]) >> 8
                    ev["rail_down"] += step == 0
                    bit = 0
                d.ptable[pp] += step
                if d.high == d.low:
                    ev["high_eq_low"] += 1
                _renorm(d, ev)
                q.step(bit)
        for q in d.sp:
            out.append(q.byte)
            d.crc = (d.crc + (d.crc << 1) + q.byte) & M32
            q.end_frame()
    return True


def read_block(wv: bytes, block: int = 0, renorm_cap: int = 4):
    """One block of a file through the plain reader: (the bytes it decodes to -- coded
    channels only, None where the block is declined, short where a symbol fails --, events).
    renorm_cap below 4 is a wrong reader (the byte loop never runs more than 4 times): what a
    kernel that capped its one-shift renormalisation there would decode."""
    from tests import vectors as V
    off, n = V.block_spans(wv)[block]
    b = wv[off:off + n]
    nframes = int.from_bytes(b[20:24], "little")
    flags = int.from_bytes(b[24:28], "little")
    hcrc = int.from_bytes(b[28:32], "little")
    mono = bool(flags & 0x40000004)  # MONO_DATA = MONO_FLAG | FALSE_STEREO
    ev = new_events()
    p, dsd = 32, None
    while p < n:
        i, ln, hl = b[p], b[p + 1] << 1, 2
        if i & 0x80:
            ln += (b[p + 2] << 9) + (b[p + 3] << 17)
            hl = 4
        if (i & 0x3F) == ID_DSD_BLOCK:
            dsd = b[p + hl:p + hl + ln - (1 if i & 0x40 else 0)]
        p += hl + ln
    d = _Dsd()
    d.data, d.byteptr, d.value, d.crc, d.renorm_cap = dsd, 0, 0, M32, renorm_cap
    if dsd is None or len(dsd) < 2 or dsd[0] > 31:
        ev["declined"] = "block"
        return None, ev
    d.byteptr = 2
    mode = dsd[1]
    out = bytearray()
    if mode == 1:
        if not _init_fast(d, ev):
            ev["declined"] = "fast"
            return None, ev
        ok = _decode_fast(d, nframes, mono, ev, out)
    elif mode == 3:
        if not _init_high(d, mono, ev):
            ev["declined"] = "high"
            return None, ev
        ok = _decode_high(d, nframes, ev, out)
    else:
        ev["declined"] = "mode"
        return None, ev
    ev["crc_ok"] = bool(ok) and d.crc == hcrc
    ev["left"] = len(dsd) - d.byteptr
    return bytes(out), ev


def bytes_per_refill(ev: dict) -> int:
    """The most bytes a mode-3 stream takes between two refills of the one-lane kernel's
    payload window: dsd3_lanes refills every 4 decisions (wv_dsd_lane.hip:196, :219), to at
    least 4 valid bytes (:54-60), and is dry when a decision leaves fewer than 0 (:212).
    At 4 or less the window cannot run dry, whatever it held before."""
    q = ev["renorm_seq"]
    return max(sum(q[k:k + 4]) for k in range(0, len(q), 4))


# =====================================================================================
# the case table
# =====================================================================================
@dataclasses.dataclass
class Case:
    name: str
    data: bytes            # the file
    source: bytes | None   # what the writer encoded (coded channels, frame-major); None: declined / damaged
    expect: dict           # event -> least count the plain reader must see (or an exact value for non-counts)
    well_formed: bool
    mode: int = 0
    layout: str = "s"
    kind: str = "ok"       # ok / declined / damaged
    seams: tuple = ()
    nframes: int = 0

    def __iter__(self):  # (name, file bytes, source or None, expected events, well_formed)
        return iter((self.name, self.data, self.source, self.expect, self.well_formed))


FILTER_BYTES = (0, 1, 0x7F, 0x80, 0xFF)
FACTORS = (0, 1, -1, 511, 512, -512, -513, 0x7FFF, -0x8000)
RATES = (0, 1, 39, 40, 127, 128, 254, 255)
M3_FRAMES = (1, 7, 8, 9, 63, 64)
ZERO_FILT = ((0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0))
_KINDS = ("s", "m", "fs")


def _m3(name, layout, nframes, rate_i, filt, chooser, seams, expect=None, **kw):
    wch = LAYOUTS[layout][1]
    payload, src = mode3_payload(nframes, wch, rate_i, filt, chooser, **kw)
    return Case(name, block_file(layout, 3, payload, src, nframes), src, expect or {}, True, 3, layout, "ok",
                tuple(seams), nframes), payload


def _cut(base: Case, payload: bytes, k: int, name: str, seams, expect=None, mode=None):
    """the case's file with its payload cut by k bytes at the end: damaged"""
    mode = mode or base.mode
    return Case(name, block_file(base.layout, mode, payload[:len(payload) - k], base.source, base.nframes), None,
                expect or {}, False, mode, base.layout, "damaged", tuple(seams), base.nframes)


def _mode3_cases():
    out = []
    # filter bytes: case r puts FILTER_BYTES[(k + r) % 5] into filter k+1 (channel 1: the rotation before it)
    for r in range(5):
        f = [tuple(FILTER_BYTES[(k + r + c) % 5] for k in range(5)) + (FACTORS[(r + 4 * c) % 9],) for c in range(2)]
        for layout in ("s", _KINDS[1 + r % 2]):
            out.append(_m3(f"m3_filt_rot{r}_{layout}", layout, 16, 3, f, random(300 + r, 0.4),
                           ("m3_filter_bytes", "m3_filters_per_channel"))[0])
    for tag, f in (("a", ((255, 0, 255, 0, 255, 0x7FFF), (1, 128, 127, 255, 0, -0x8000))),
                   ("b", ((1, 128, 127, 255, 0, -0x8000), (255, 0, 255, 0, 255, 0x7FFF))),
                   ("f5ff_f40", ((0, 0, 0, 0, 255, -0x8000), (255, 255, 255, 0, 255, 0x7FFF)))):
        for layout in _KINDS:
            for ch_nm, ch in (("rnd", random(310, 0.5)), ("ones", random(311, 0.95)), ("zeros", random(312, 0.05))):
                out.append(_m3(f"m3_filt_{tag}_{layout}_{ch_nm}", layout, 24, 7, f, ch,
                               ("m3_filter_bytes", "m3_filter5_ff_filter4_0", "m3_factor",
                                "m3_filters_per_channel"))[0])
    for k, fac in enumerate(FACTORS):
        f = ((0x80, 0x7F, 0x80, 0x7F, 0x80, fac), (0x7F, 0x80, 0x7F, 0x80, 0x7F, FACTORS[(k + 3) % 9]))
        for layout in ("s", _KINDS[1 + k % 2]):
            out.append(_m3(f"m3_factor_{fac}_{layout}", layout, 32, 3, f, random(320 + k, 0.5),
                           ("m3_factor", "m3_factor_decay"))[0])
    # rate_i; `probable` for 64 frames pushes the entries it meets onto the rails, then random bits
    for k, ri in enumerate(RATES):
        layout = _KINDS[k % 3]
        wch = LAYOUTS[layout][1]
        out.append(_m3(f"m3_rate{ri}_{layout}", layout, 64, ri, ZERO_FILT,
                       switch(probable, random(330 + k, 0.5), 48 * 8 * wch), ("m3_rate_i",))[0])
    out.append(_m3("m3_rails_s", "s", 64, 255, ZERO_FILT, switch(probable, random(340, 0.5), 60 * 16),
                   ("m3_rails",), {"rail_up": 1, "rail_down": 1})[0])
    out.append(_m3("m3_rails_m", "m", 64, 255, ((0x80, 0x80, 0x80, 0x80, 0x80, 0),) * 2,
                   switch(probable, random(341, 0.5), 60 * 8), ("m3_rails",), {"rail_up": 1})[0])
    # rate_s != 20
    for rs in (19, 21):
        payload, src = mode3_payload(8, 2, 3, ZERO_FILT, random(350), rate_s=rs)
        out.append(Case(f"m3_rate_s{rs}", block_file("s", 3, payload, src, 8), None, {"declined": "high"}, False, 3,
                        "s", "declined", ("m3_rate_s",), 8))
    # the least payload: no byte shifted out of a `probable` frame at rate_i 255
    for layout, least in (("m", 13), ("s", 20)):
        c, payload = _m3(f"m3_len{least}_{layout}", layout, 1, 255, ZERO_FILT, probable, ("m3_length",))
        assert len(payload) == least, len(payload)
        out.append(c)
        d = _cut(c, payload, 1, f"m3_len{least - 1}_{layout}", ("m3_length",), {"declined": "high"})
        d.kind = "declined"
        out.append(d)
    # choosers
    for layout in _KINDS:
        out.append(_m3(f"m3_improbable_{layout}", layout, 64, 3, ZERO_FILT, improbable, ("m3_improbable",))[0])
        out.append(_m3(f"m3_improbable_then_random_{layout}", layout, 64, 20, ZERO_FILT,
                       switch(improbable, random(360, 0.3), 100), ("m3_improbable",))[0])
        out.append(_m3(f"m3_straddle_{layout}", layout, 64, 3, ((0x80, 0x80, 0x80, 0x80, 0x80, 0),) * 2,
                       straddle(370 + len(layout)), ("m3_narrow", "m3_high_eq_low"),
                       {"narrow": 1, "high_eq_low": 1, "renorm4": 1})[0])
        for seed in range(375, 400):  # (the first seed whose stream a lane's window surely holds: bytes_per_refill)
            c = _m3(f"m3_collapse_hug_{layout}", layout, 64, 3, ((0x80, 0x80, 0x80, 0x80, 0x80, 0),) * 2,
                    collapse_then_hug(seed), ("m3_high_eq_low",), {"high_eq_low": 1, "renorm4": 1})[0]
            ev = read_block(c.data)[1]
            if ev["high_eq_low"] and bytes_per_refill(ev) <= 4:
                break
        out.append(c)
    # frame counts
    for nf in M3_FRAMES:
        for layout in _KINDS:
            out.append(_m3(f"m3_frames{nf}_{layout}", layout, nf, 5,
                           ((3, 9, 27, 81, 243, 100), (243, 81, 27, 9, 3, -100)),
                           random(380 + nf, 0.35), ("m3_frames",))[0])
    # tails
    for layout, ks in (("s", range(1, 9)), ("m", (1, 4, 8)), ("fs", (2, 5))):
        base, payload = _m3(f"m3_tailbase_{layout}", layout, 64, 3, ZERO_FILT, random(390, 0.3), ())
        for k in ks:
            out.append(_cut(base, payload, k, f"m3_tail_cut{k}_{layout}", ("m3_tail",), {"renorm_cut": 1}))
    return out


def _one_bin(entries: dict) -> list:
    p = [0] * 256
    for k, v in entries.items():
        p[k] = v
    return p


def single_bin_tables():
    """(name, 256 probabilities): the lone-bin totals and shapes"""
    t = [("tot1_e0", _one_bin({0: 1})), ("tot1_e255", _one_bin({255: 1})), ("tot2", _one_bin({0: 1, 255: 1})),
         ("tot3", _one_bin({7: 1, 8: 1, 200: 1})),
         ("tot255", _one_bin({0: 100, 15: 50, 16: 5, 128: 99, 255: 1})),
         ("tot256", _one_bin({0: 128, 15: 64, 16: 32, 239: 16, 240: 8, 255: 8})),
         ("tot257", _one_bin({1: 100, 14: 50, 17: 5, 129: 100, 254: 2})),
         ("tot1279", [5] * 255 + [4]),
         ("tot1280", [5] * 256),
         ("one_segment", _one_bin({32 + k: 3 + k for k in range(16)})),
         ("edges_15_16_239_240", _one_bin({15: 7, 16: 9, 239: 1, 240: 200})),
         ("alternating", [(k & 1) * (1 + k % 7) for k in range(256)])]
    return t


BIG_BIN = 32 * MAX_BYTES_PER_BIN - 31 * 8  # 40,712


def big_bin_table(extra: int = 0) -> list:
    """32 bins: bin 5 of total 40,712 (+ extra), the others of total 8"""
    prob = []
    for b in range(32):
        if b == 5:
            row = [159] * 256                     # 40,704
            row[0] += 8 + extra
        else:
            row = _one_bin({b: 2, 5: 3, 37: 2, 255: 1})  # (every bin can reach bin 5, and itself)
        prob += row
    return prob


def _m1(name, layout, nframes, hb, prob, chooser, seams, expect=None, **kw):
    wch = LAYOUTS[layout][1]
    payload, src = mode1_payload(nframes * wch, wch, hb, prob, chooser, **kw)
    assert len(src) == nframes * wch, name
    return Case(name, block_file(layout, 1, payload, src, nframes), src, expect or {}, True, 1, layout, "ok",
                tuple(seams), nframes), payload


def _m1_raw(name, layout, nframes, payload, seams, kind, expect=None):
    return Case(name, block_file(layout, 1, payload, None, nframes), None, expect or {}, False, 1, layout, kind,
                tuple(seams), nframes)


RLE_STEP_TABLE = ([3] * 63 + [0] * 40 + [2] * 62 + [0] * 30 + [1] * 61)  # codes 63|64 and 127|128 are zero runs
RLE_STEP_BREAKS = (63 + 17, 63 + 40 + 62 + 9)


def _mode1_cases():
    out = []
    tables = single_bin_tables()
    seam_of = {"tot1_e0": ("m1_total_small", "m1_entry_0_255"), "tot1_e255": ("m1_total_small", "m1_entry_0_255"),
               "tot2": ("m1_total_small", "m1_entry_0_255"), "tot3": ("m1_total_small",),
               "tot255": ("m1_total_pow2",), "tot256": ("m1_total_pow2", "m1_segment_edges"),
               "tot257": ("m1_total_pow2",), "tot1279": ("m1_total_1280",), "tot1280": ("m1_total_1280",),
               "one_segment": ("m1_segment_edges",), "edges_15_16_239_240": ("m1_segment_edges",),
               "alternating": ("m1_segment_edges",)}
    for k, (nm, prob) in enumerate(tables):
        for layout in _KINDS:
            out.append(_m1(f"m1_{nm}_{layout}_random", layout, 32, 0, prob, random(400 + k), seam_of[nm])[0])
        layout = _KINDS[k % 3]
        out.append(_m1(f"m1_{nm}_{layout}_edges", layout, 64, 0, prob, edges, seam_of[nm],
                       {"codes": [c for c in (0, 15, 16, 239, 240, 255) if prob[c]]})[0])
        if sum(prob) >= 256:
            nf = 128 // LAYOUTS[layout][1]
            c, payload = _m1(f"m1_{nm}_{layout}_straddle", layout, nf, 0, prob, straddle(420 + k),
                             ("m1_reload", "m1_narrow"), {"reload_ge4": 1})
            out.append(c)
            # the same file cut inside the four bytes of its first, a middle and its last reload
            _, ev = read_block(c.data)
            at = [a for a in ev["reload_at"]]
            for j, a in enumerate(sorted({at[0], at[len(at) // 2], at[-1]})):
                keep = a - 2 + (j % 4)  # 0..3 of the reload's bytes left (a counts the two mode bytes)
                out.append(Case(f"m1_{nm}_{layout}_straddle_cut_reload{j}",
                                block_file(layout, 1, payload[:keep], c.source, nf), None, {"reload_lt4": 1}, False, 1,
                                layout, "damaged", ("m1_reload_short",), nf))
    # a reload that finds exactly four bytes: the block's last symbol reloads, and is not the symbol the
    # bytes before would give (the straddled values all look alike)
    first_live = lambda low, high, x, probs, index: next(c for c in range(256) if probs[c])
    for k, layout in enumerate(_KINDS):
        wch = LAYOUTS[layout][1]
        nm, prob = tables[(5, 7, 6)[k]]
        for nsym in range(128, 32, -wch):
            c, _ = _m1(f"m1_{nm}_{layout}_reload_last", layout, nsym // wch, 0, prob,
                       switch(straddle(425 + k), first_live, nsym - 1), ("m1_reload",), {"reload_eq4": 1})
            if read_block(c.data)[1]["reload_sym"][-1:] == [nsym - 1]:
                break
        out.append(c)
    # high - low below 256 and high == low (a 4-byte shift): totals 2 and 3 narrowed onto a byte boundary
    for layout in _KINDS:
        nf = 128 // LAYOUTS[layout][1]
        out.append(_m1(f"m1_tot2_{layout}_straddle", layout, nf, 0, tables[2][1], straddle(430), ("m1_narrow",),
                       {"narrow": 1, "high_eq_low": 1, "renorm4": 1})[0])
        out.append(_m1(f"m1_tot3_{layout}_straddle", layout, nf, 0, tables[3][1], straddle(431),
                       ("m1_narrow", "m1_reload"), {"narrow": 1, "reload_ge4": 1})[0])
    # 32 bins, one of them at the budget
    big = big_bin_table()
    for layout in _KINDS:
        wch = LAYOUTS[layout][1]
        out.append(_m1(f"m1_bigbin_{layout}_random", layout, 64, 5, big, random(440), ("m1_big_bin",))[0])
        out.append(_m1(f"m1_bigbin_{layout}_straddle", layout, 128 // wch, 5, big,
                       fixed([5, 5], straddle(441)), ("m1_big_bin", "m1_reload"), {"reload_ge4": 1})[0])
    payload, _ = mode1_payload(16, 2, 5, big_bin_table(1), random(442))
    out.append(_m1_raw("m1_bigbin_plus1", "s", 8, payload, ("m1_big_bin",), "declined", {"declined": "fast"}))
    # empty bins
    two = _one_bin({0: 3, 1: 1, 2: 4}) + [0] * 256  # bin 1 is empty; symbol 1 selects it
    for layout in _KINDS:
        wch = LAYOUTS[layout][1]
        payload, src = mode1_payload(16 * wch, wch, 1, two, fixed([0, 2, 2, 0, 1], random(450)))
        assert len(src) < 16 * wch
        out.append(_m1_raw(f"m1_empty_bin_{layout}", layout, 16, payload, ("m1_empty_bin",), "damaged",
                           {"failed": "empty_bin"}))
    for nm, prob in (("tot3", tables[3][1]), ("tot256", tables[5][1])):
        payload = bytes([0, 0xFF]) + bytes(prob) + b"\xff" * 8
        for layout in ("s", "m"):
            out.append(_m1_raw(f"m1_ff_value_{nm}_{layout}", layout, 8, payload, ("m1_index_ge_tot",), "damaged",
                               {"failed": "index_ge_tot"}))
    # run-length tables
    t254 = _one_bin({0: 254, 1: 1, 3: 254, 255: 200})
    out.append(_m1("m1_rle_maxp254_s", "s", 32, 0, t254, random(460), ("m1_rle_max_prob", "m1_rle_runs"),
                   rle_max_prob=0xFE)[0])
    t1 = [(k % 3 == 0) * 1 for k in range(256)] + [1] * 256
    out.append(_m1("m1_rle_maxp1_m", "m", 48, 1, t1, random(461), ("m1_rle_max_prob", "m1_rle_runs"),
                   rle_max_prob=1)[0])
    out.append(_m1("m1_rle_code_eq_maxp_fs", "fs", 24, 0, _one_bin({9: 17, 10: 5, 200: 17}), random(462),
                   ("m1_rle_max_prob",), rle_max_prob=17)[0])
    payload = bytes([0, 0]) + rle_table([0] * 256, 0) + b"\0" * 8
    out.append(_m1_raw("m1_rle_maxp0_s", "s", 8, payload, ("m1_rle_max_prob", "m1_empty_bin"), "damaged",
                       {"failed": "empty_bin", "max_prob": 0}))
    for layout in _KINDS:
        out.append(_m1(f"m1_rle_steps_{layout}", layout, 40, 0, RLE_STEP_TABLE, random(463), ("m1_rle_runs",),
                       rle_max_prob=5, rle_breaks=RLE_STEP_BREAKS)[0])
    sparse = [0] * 1024
    for k in (3, 4, 260, 515, 700, 1000):
        sparse[k] = 6
    for b in range(4):
        sparse[256 * b + b] = 2  # every bin is live
    out.append(_m1("m1_rle_overshoot_s", "s", 40, 2, sparse, random(464), ("m1_rle_overshoot",), {"rle_overshoot": 1},
                   rle_max_prob=6, rle_overshoot=9)[0])
    out.append(_m1("m1_rle_overshoot_m", "m", 40, 2, sparse, random(465), ("m1_rle_overshoot",), {"rle_overshoot": 1},
                   rle_max_prob=100, rle_overshoot=1)[0])
    full = [1 + (k * 7) % 8 for k in range(512)]  # no zero entry: the table fills on a literal
    out.append(_m1("m1_rle_exact_zero_s", "s", 40, 1, full, random(466), ("m1_rle_exact",), {"rle_after": 0},
                   rle_max_prob=9)[0])
    c, payload = _m1("m1_rle_exact_nonzero_s", "s", 40, 1, full, random(466), ("m1_rle_exact",), rle_max_prob=9,
                     rle_tail=b"\x01")
    out.append(dataclasses.replace(c, source=None, well_formed=False, kind="declined",
                                   expect={"declined": "fast", "rle_after": 1}))
    ends0 = sparse[:1023] + [0]
    out.append(_m1("m1_rle_exact_run_zero_m", "m", 40, 2, ends0, random(467), ("m1_rle_exact",), {"rle_after": 0},
                   rle_max_prob=6)[0])
    c, payload = _m1("m1_rle_early_end_s", "s", 40, 1, full, random(468), ("m1_rle_early_end",), rle_max_prob=9)
    early = payload[:2 + 300] + b"\0" + payload[2 + 301:]
    out.append(Case("m1_rle_early_end_s", block_file("s", 1, early, None, 40), None, {"declined": "fast"}, False, 1,
                    "s", "declined", ("m1_rle_early_end",), 40))
    # raw tables with 3, 4, 5 bytes after them
    c, payload = _m1("m1_raw_plus4_m", "m", 1, 0, tables[2][1], fixed([255]), ("m1_raw_length",))
    assert len(payload) == 2 + 256 + 4
    out.append(c)
    out.append(Case("m1_raw_plus3_m", block_file("m", 1, payload[:-1], None, 1), None, {"declined": "fast"}, False, 1,
                    "m", "declined", ("m1_raw_length",), 1))
    c, payload = _m1("m1_raw_plus5_m", "m", 1, 0, _one_bin({0: 1, 1: 255}), fixed([0]), ("m1_raw_length",))
    assert len(payload) == 2 + 256 + 5
    out.append(c)
    # frame counts
    mix = [1 + (k % 5) for k in range(256)] * 2
    for layout, counts in (("s", (1, 7, 8, 9)), ("m", (15, 16, 17)), ("fs", (7, 8, 9))):
        for nf in counts:
            out.append(_m1(f"m1_frames{nf}_{layout}", layout, nf, 1, mix, random(470 + nf), ("m1_frames",))[0])
    # tails
    for layout, ks in (("s", range(1, 10)), ("m", (1, 2, 7, 8)), ("fs", (3, 9))):
        base, payload = _m1(f"m1_tailbase_{layout}", layout, 64, 1, mix, random(480), ())
        for k in ks:
            out.append(_cut(base, payload, k, f"m1_tail_cut{k}_{layout}", ("m1_tail",), {"renorm_cut": 1}))
    return out


def _chain_cases():
    """two blocks, the second without ID_DSD_BLOCK: it continues the first one's data and
    state, so the first block's payload codes both blocks' frames and the pair goes to
    the chain decode"""
    from tests import vectors as V
    out = []
    nf = 24
    for mode in (3, 1):
        for layout in _KINDS:
            nch, wch, fs = LAYOUTS[layout]
            if mode == 3:
                payload, src = mode3_payload(2 * nf, wch, 40,
                                             ((255, 0, 255, 0, 255, 0x7FFF), (1, 128, 127, 255, 0, -0x8000)),
                                             random(500, 0.4))
            else:
                payload, src = mode1_payload(2 * nf * wch, wch, 0, single_bin_tables()[5][1], straddle(501))
            x = frames_of(src, layout, 2 * nf)
            f = S.encode_dsd(x, S.DsdParams(nch=nch, false_stereo=fs, mode=0, block_samples=nf))
            f = V.strip_subblocks(replace_dsd(f, 0, bytes([0, mode]) + payload), 1, {ID_DSD_BLOCK})
            out.append(Case(f"m{mode}_chain_{layout}", f, src, {}, True, mode, layout, "chain", (f"m{mode}_chain",),
                            2 * nf))
    return out


_CASES = None


def cases() -> list:
    """every case, built once"""
    global _CASES
    if _CASES is None:
        _CASES = _mode3_cases() + _mode1_cases() + _chain_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def __getattr__(name):  # dsd_vectors.CASES: the table, built on first use
    if name == "CASES":
        return cases()
    raise AttributeError(name)


def expected_output(c: Case) -> np.ndarray | None:
    """what a well-formed case decodes to: its source, a false-stereo frame twice"""
    if c.source is None:
        return None
    x = np.frombuffer(c.source, np.uint8).reshape(-1, LAYOUTS[c.layout][1]).astype(np.int32)
    if c.layout == "fs":
        x = np.repeat(x, 2, axis=1)
    return x.reshape(-1)


_REFS = {}


def reference(c: Case, chunk: int = 4096):
    """the oracle's decode of a case, computed once and shared (read-only)"""
    from oracle import oracle as O
    key = (c.name, chunk)
    if key not in _REFS:
        r = O.decode_file(c.data, chunk=chunk)
        r.samples.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]
