"""Streams that carry a decorrelation weight out of int16, and the plain reader that says
what the reference does with them (generated here: synth/ codes the words, the pass
metadata is spliced in).

The reference runs each pass over one caller chunk at a time and stores the pass weights
back as (short) when the pass call returns (UnpackUtils.cs:942-943, :1152-1153, :1239); a
stereo call of 16 frames or more is an 8-frame call and a "cont" call (:597-607), so
there is a store after frame 8 too.  A positive term's weight is otherwise unclamped and
moves by delta a frame: past +-32767 the next store wraps it, and every later sample
depends on where the caller's chunk seams fell.  SEAMS names the places that re-create
those stores (or hand the block back before one can matter); CASES puts files on them.

Three separate pieces:
  * write_file(): a decoder-domain writer -- residual words, a term list (decode order),
    weight bytes and history logs in, a lossless .wv out.  The synth encoder with an empty
    term list codes its input array as the words; ID_DECORR_TERMS / _WEIGHTS / _SAMPLES
    replace its empty ID_DECORR_TERMS, the header's flags, CRC and ckSize are rewritten.
  * read(): the plain reader -- decorr_stereo_pass, decorr_stereo_pass_cont,
    decorr_mono_pass, joint stereo, the mute test and the CRC, pass-major per call for a
    chunk size, each (short) store site switchable.  A pass keeps its last 8 outputs in
    time order, which is what the reference's rings and the cont call's look-back into
    the buffer both hold; 32-bit wrap is explicit (Python integers do not wrap).
  * the choosers: they pick each residual by simulating one ("driven") pass forward so
    that its weight moves the wanted way while the outputs stay bounded.  Every other
    pass of a list is transparent (weight byte 0, delta 0: output = input), which puts
    the driven pass at any position of any list.

Limits the choosers keep (test_decorr_seams_host asserts them): |output| <= OUT_MAX,
|residual| <= RES_MAX (the wrap32 files and the one residual that cancels an exploded
history have their own), every block at most MAX_FRAMES frames.  Every block is coded from
zero medians (one encoder call a block), so no block starts above MED_MAX.
"""
import dataclasses

import numpy as np

from synth import wvsynth as S
from tests import vectors as V
from tests.magnitude_vectors import exp2s

MAX_FRAMES = 12288
# The named cases number 44 taken once each (cross 4 + 4, edge 4, seam8 1 + 4 siblings, one_group 1, A / B 3 x 2,
# position 3 x 3 + 1, hug, control, foreign, sticky, shifted, clamp 3, wrap32 2).  On top of them: calls of exactly
# 16 frames (n >= 16, not n > 16), a frame-8 file and a clamp file on the default list (the two-wave kernel), a second
# compile-time position, hug and control both mono and stereo and hug on each lane kernel (+5), foreign stereo and
# foreign into a sticky block (+2), sticky stereo (+1), a wrap32 file for the product's >> 10 (+1).
MAX_FILES = 57
OUT_MAX = 1 << 21    # |output| (joint stereo doubles the passes' 2^20)
RES_MAX = 1 << 23    # |residual word|
MAG = 22             # header magnitude field: mute limit 2^22 + 2, twice OUT_MAX
MED_MAX = 1 << 17    # raw start median of a block after the first (DESIGN.md's table: kept by the lanes)
GF = 8               # frames a lane group

B31, M32 = 1 << 31, (1 << 32) - 1

MONO_FLAG, JOINT_STEREO, CROSS_DECORR, FALSE_STEREO = 4, 0x10, 0x20, 0x40000000
MAG_LSB = 18

# name -> where the store (or the test that avoids it) is made: csrc/ = wavpackdecoder_amd/csrc/
SEAMS = {
    "call_end": "UnpackUtils.cs:942-943, :1152-1153, :1239 (short) store when a pass call returns; "
                "wv_decode_core.h:1030 j == n - 1 / wv_wave2.h:1978 t == chunk_end - 1 / wv_pipe.h:204-207 seam mask",
    "frame8": "UnpackUtils.cs:597-607 a stereo call of >= 16 frames is an 8-frame call and a cont call; "
              "wv_decode_core.h:1030 n >= 16 && j == 7 / wv_wave2.h:1978 sm.seam8 / wv_pipe.h:159, :173 seam8",
    "block_end": "UnpackUtils.cs:524-525 the last call of a block is cut at the block end, its store decides the "
                 "weights a block without ID_DECORR_WEIGHTS continues from; wv_decode_core.h:1030 with n cut at :961 / "
                 "decode_chain (wv_decode.hip) carries the stored weight",
    "mute_call": "UnpackUtils.cs:556-607 precede the mute test at :567-578 / :613-646: the muting call's passes run "
                 "to its end and store; wv_decode_core.h:1083-1087",
    "lane_wbad": "wv_lane.h:154-158, :283, :1693, :1785, :1826 wbad(): max(|wA|, |wB|) > 32767 - GF * delta at a "
                 "group start hands the block back (rbad |= 4)",
    "clamp": "UnpackUtils.cs:778-799 (and the cont forms :1016-1038 ...): terms -1..-3 clamp at +-1024 where "
             "(w += delta) > 1024 first holds; wv_decode_core.h vupdc / wv_pipe.h:203 lo, hi",
}


ALL_SITES = ("call_end", "frame8", "block_end", "mute_call")


def i32(v: int) -> int:
    return v if -B31 <= v < B31 else ((v + B31) & M32) - B31


def i16(v: int) -> int:
    return ((v + 0x8000) & 0xFFFF) - 0x8000


def restore_weight(b: int) -> int:
    """WordsUtils.cs:653-661 of a stored signed byte"""
    r = b << 3
    if r > 0:
        r += (r + 64) >> 7
    return r


def aw(w: int, s: int) -> int:
    """(int)((weight * (long)sam + 512) >> 10)"""
    return i32((w * s + 512) >> 10)


# ---------------------------------------------------------------------------------------
# block description (what the writer writes and the reader reads)
# ---------------------------------------------------------------------------------------
@dataclasses.dataclass
class Block:
    words: list                 # [(L, R)] residual words, R = 0 for a mono / false-stereo block
    terms: tuple                # decode order (the stored order is the reverse)
    deltas: tuple
    wbytes: tuple = ()          # ((a, b), ...) stored weight bytes, decode order; () with sticky
    hist: tuple = ()            # per pass (decode order): (logs A, logs B), time order, oldest first; () = none
    mono: bool = False          # MONO_FLAG
    false_stereo: bool = False  # FALSE_STEREO: the mono path, each value written twice
    joint: bool = False
    sticky: bool = False        # no pass metadata: the passes of the block before continue
    bps: int = 3
    mag: int = MAG

    @property
    def mono_path(self):
        return self.mono or self.false_stereo


def calls(nfr: int, chunk: int, phase: int):
    """[(a, b)): the pieces of the caller's chunks that fall into a block starting `phase`
    frames into the file (WavPackUtils.cs WavpackUnpackSamples: a call ends at the block end)"""
    out, a = [], 0
    while a < nfr:
        n = min(chunk - (phase + a) % chunk, nfr - a)
        out.append((a, a + n))
        a += n
    return out


def store_frames(nfr, chunk, phase, stereo_path, sites=ALL_SITES[:3]):
    """{frame: site}: the frames of a block after which the passes' weights are stored"""
    out = {}
    for a, b in calls(nfr, chunk, phase):
        if stereo_path and b - a >= 16 and "frame8" in sites:
            out[a + 7] = "frame8"
        site = "block_end" if b == nfr else "call_end"
        if site in sites:
            out[b - 1] = site
    return out


# ---------------------------------------------------------------------------------------
# the plain reader
# ---------------------------------------------------------------------------------------
class _Pass:
    def __init__(self, term, delta):
        self.term, self.delta = term, delta
        self.wA = self.wB = 0
        self.hA, self.hB = [0] * 8, [0] * 8   # the pass's last 8 outputs, oldest first

    def transparent(self):
        return self.delta == 0 and self.wA == 0 and self.wB == 0


def _upd(w, s, x, d):
    """UnpackUtils.cs:893-899: update_weight"""
    if s and x:
        return w - d if (s ^ x) < 0 else w + d
    return w


def new_counts():
    """what read() counts on its way (ReadResult.counts): steps a clamp cut back to +-1024 /
    steps that landed on +-1024 by themselves / 2 s0 - s1 or 3 s0 - s1 outside int32 /
    (weight * sam + 512) >> 10 outside int32"""
    return {"clamp_cut": 0, "clamp_on": 0, "sam_wrap": 0, "aw_wrap": 0}


def _updc(w, s, x, d, cnt):
    """UnpackUtils.cs:776-785: update_weight_clip"""
    if s and x:
        if (s ^ x) < 0:
            w -= d
            if w < -1024:
                w = -1024
                cnt["clamp_cut"] += 1
            elif w == -1024:
                cnt["clamp_on"] += 1
        else:
            w += d
            if w > 1024:
                w = 1024
                cnt["clamp_cut"] += 1
            elif w == 1024:
                cnt["clamp_on"] += 1
    return w


def _run_one(term, w, d, ext, a, b, cnt):
    """positive term over ext[a:b) in place (ext = 8 history values, then the call's
    buffer); -> the weight.  :1206-1223 / :885-918 by ring, :1119-1135 by look-back: the
    same values; 17 and 18 :700-768, :958-1002"""
    sw = pw = 0
    for i in range(a, b):
        if term == 17:
            s = 2 * ext[i - 1] - ext[i - 2]
        elif term == 18:
            s = 3 * ext[i - 1] - ext[i - 2]
        else:
            s = ext[i - term]
        if not -B31 <= s < B31:
            sw += 1
            s = i32(s)
        if term == 18:
            s >>= 1
        x = ext[i]
        pr = (w * s + 512) >> 10
        if not -B31 <= pr < B31:
            pw += 1
            pr = i32(pr)
        ext[i] = i32(pr + x)
        if s and x:
            w = w - d if (s ^ x) < 0 else w + d
    cnt["sam_wrap"] += sw
    cnt["aw_wrap"] += pw
    return w


def _run_neg(p, eL, eR, a, b, cnt):
    """terms -1, -2, -3 over frames [a, b) (:771-880, :1011-1116): the other channel's
    output of this frame (-1: R from L; -2: L from R) or of the frame before"""
    t, d = p.term, p.delta
    wA, wB = p.wA, p.wB
    for i in range(a, b):
        xL, xR = eL[i], eR[i]
        if t == -1:
            s = eR[i - 1]
            oL = i32(xL + aw(wA, s))
            wA = _updc(wA, s, xL, d, cnt)
            oR = i32(xR + aw(wB, oL))
            wB = _updc(wB, oL, xR, d, cnt)
        elif t == -2:
            s = eL[i - 1]
            oR = i32(xR + aw(wB, s))
            wB = _updc(wB, s, xR, d, cnt)
            oL = i32(xL + aw(wA, oR))
            wA = _updc(wA, oR, xL, d, cnt)
        else:
            sA, sB = eR[i - 1], eL[i - 1]
            oL = i32(xL + aw(wA, sA))
            wA = _updc(wA, sA, xL, d, cnt)
            oR = i32(xR + aw(wB, sB))
            wB = _updc(wB, sB, xR, d, cnt)
        eL[i], eR[i] = oL, oR
    p.wA, p.wB = wA, wB


@dataclasses.dataclass
class ReadResult:
    samples: np.ndarray     # int32, interleaved as the file's channels
    frames: int
    crc: list               # per block: the CRC the reader ends with
    crc_errors: int
    mute_frame: list        # per block: the block frame whose value muted it, or None
    stores: list            # (block, frame, site, pass, wA before, wB before, wA after, wB after)
    changed: list           # the entries of `stores` that changed a value
    gmax: list              # per block: max over the positive-term passes of |w| at a group start (t % 8 == 0)
    ghand: list             # per block: some group start had max(|wA|, |wB|) > 32767 - 8 * delta of its pass
    final: list             # the passes as the last block left them: (term, delta, wA, wB, hA, hB)
    counts: dict            # new_counts(): clamp steps and int32 wraps met on the way


def _load_hist(blk, passes):
    """read_decorr_samples (UnpackUtils.cs:250-360): every entry is laid out by the term of
    the decoder's last pass (dpp.term is set once, :264); hist holds logs per pass"""
    if not blk.hist:
        return
    for p, (la, lb) in zip(passes, blk.hist):
        p.hA, p.hB = [0] * 8, [0] * 8
        va, vb = [exp2s(v) for v in la], [exp2s(v) for v in lb]
        if va:
            p.hA[-len(va):] = va
        if vb:
            p.hB[-len(vb):] = vb


def read(blocks, chunk, sites=ALL_SITES, header_crc=None) -> ReadResult:
    """the reference's decode of `blocks` in file order, WavpackUnpackSamples(chunk) at a time.
    `sites`: the (short) stores that are made -- "call_end", "frame8", "block_end" by where they
    fall; without "mute_call" the call that mutes its block makes none of them"""
    out, crcs, mutes, stores, changed, gmax, ghand = [], [], [], [], [], [], []
    passes, phase, crc_errors, cnt = [], 0, 0, new_counts()
    for bi, blk in enumerate(blocks):
        mp = blk.mono_path
        if not blk.sticky:
            passes = [_Pass(t, d) for t, d in zip(blk.terms, blk.deltas)]
            for p, (a, b) in zip(passes, blk.wbytes):
                p.wA = restore_weight(a)
                p.wB = 0 if mp else restore_weight(b)
            _load_hist(blk, passes)
        nfr = len(blk.words)
        limit = i32((1 << blk.mag) + 2)
        crc, muted, mute_at = -1, False, None
        gm, gh = 0, False
        och = 1 if blk.mono else 2
        bsp_frames = phase % chunk   # frames of this call already in the caller's buffer
        for ci, (a, b) in enumerate(calls(nfr, chunk, phase)):
            n = b - a
            bsp = (bsp_frames if ci == 0 else 0) * och
            if muted:   # :527-543
                out.extend([0] * (n * och))
                continue
            eL = [w[0] for w in blk.words[a:b]]
            eR = None if mp else [w[1] for w in blk.words[a:b]]
            cut = 8 if (not mp and n >= 16) else n     # :587-607
            if "mute_call" not in sites:   # (a copy to run the call again from, should it mute)
                saved = [(p.wA, p.wB, list(p.hA), list(p.hB)) for p in passes]
                saved_words, n_st, n_ch = (list(eL), None if mp else list(eR)), len(stores), len(changed)
            for pi, p in enumerate(passes):
                pos = p.term > 0
                if pos:   # group-start weights, before the frame runs (the store of t - 1 is behind it)
                    lim = 32767 - GF * p.delta
                if p.transparent() and pos:
                    # weight 0, delta 0: (0 * s + 512) >> 10 = 0 and the weight never moves -- output = input
                    xa = p.hA + eL
                    p.hA = xa[-8:]
                    if not mp:
                        xb = p.hB + eR
                        p.hB = xb[-8:]
                    segs = ((0, cut), (cut, n)) if cut < n else ((0, n),)
                    for s0, s1 in segs:
                        f = a + s1 - 1
                        site = "frame8" if s1 < n else ("block_end" if b == nfr else "call_end")
                        if site in sites:
                            stores.append((bi, f, site, pi, 0, 0, 0, 0))
                    continue
                xa = p.hA + eL
                xb = None if mp else p.hB + eR
                segs = ((0, cut), (cut, n)) if cut < n else ((0, n),)
                for s0, s1 in segs:
                    # the pass runs group by group so the weight at each group start is seen
                    k = s0
                    while k < s1:
                        t = a + k
                        k1 = min(s1, k + (GF - t % GF))
                        if pos and t % GF == 0:
                            m = max(abs(p.wA), abs(p.wB))
                            gm = max(gm, m)
                            gh = gh or m > lim
                        if pos:
                            p.wA = _run_one(p.term, p.wA, p.delta, xa, 8 + k, 8 + k1, cnt)
                            if not mp:
                                p.wB = _run_one(p.term, p.wB, p.delta, xb, 8 + k, 8 + k1, cnt)
                        else:
                            _run_neg(p, xa, xb, 8 + k, 8 + k1, cnt)
                        k = k1
                    site = "frame8" if s1 < n else ("block_end" if b == nfr else "call_end")
                    if site in sites:   # dpp.weight_A = (short) weight_A
                        wa, wb = i16(p.wA), i16(p.wB)
                        rec = (bi, a + s1 - 1, site, pi, p.wA, p.wB, wa, wb)
                        stores.append(rec)
                        if (wa, wb) != (p.wA, p.wB):
                            changed.append(rec)
                        p.wA, p.wB = wa, wb
                eL = xa[8:]
                p.hA = xa[-8:]
                if not mp:
                    eR = xb[8:]
                    p.hB = xb[-8:]
            # joint stereo, the mute test and the CRC (:564-578, :609-646)
            stop = None
            if mp:
                for j in range(n):
                    v = eL[j]
                    if (-v if v < 0 else v) > limit:
                        stop = j
                        break
                    crc = i32(crc * 3 + v)
                # (i = q counts from the buffer's start, :574: a stop at q == n is not a mute)
                is_mute = stop is not None and stop + bsp != n
            else:
                for j in range(n):
                    l, r = eL[j], eR[j]
                    if blk.joint:
                        r = i32(r - (l >> 1))
                        l = i32(l + r)
                        eL[j], eR[j] = l, r
                    if (-l if l < 0 else l) > limit or (-r if r < 0 else r) > limit:
                        stop = j
                        break
                    crc = i32(i32(crc * 3 + l) * 3 + r)
                is_mute = stop is not None
            if is_mute:
                muted, mute_at = True, a + stop
                out.extend([0] * (n * och))
                if "mute_call" not in sites:   # the same call without its stores
                    del stores[n_st:], changed[n_ch:]
                    for p, (wa, wb, ha, hb) in zip(passes, saved):
                        p.wA, p.wB, p.hA, p.hB = wa, wb, ha, hb
                    one = Block(words=list(zip(saved_words[0], saved_words[1] or [0] * n)), terms=blk.terms,
                                deltas=blk.deltas, sticky=True, mono=blk.mono, false_stereo=blk.false_stereo)
                    _rerun(passes, one, cnt)
            elif mp:
                if blk.mono:
                    out.extend(eL)
                else:
                    for v in eL:
                        out.append(v)
                        out.append(v)
            else:
                for l, r in zip(eL, eR):
                    out.append(l)
                    out.append(r)
        crcs.append(crc)
        mutes.append(mute_at)
        gmax.append(gm)
        ghand.append(gh)
        if header_crc is not None and crc != header_crc[bi]:
            crc_errors += 1
        phase += nfr
    nch = 1 if blocks[0].mono else 2
    final = [(p.term, p.delta, p.wA, p.wB, list(p.hA), list(p.hB)) for p in passes]
    return ReadResult(np.array(out, dtype=np.int64).astype(np.int32), len(out) // nch, crcs, crc_errors, mutes, stores,
                      changed, gmax, ghand, final, cnt)


def _rerun(passes, one, cnt):
    """the passes over one call's words with no store at all (read() without "mute_call")"""
    mp = one.mono_path
    eL = [w[0] for w in one.words]
    eR = None if mp else [w[1] for w in one.words]
    n = len(eL)
    for p in passes:
        xa = p.hA + eL
        xb = None if mp else p.hB + eR
        if p.term > 0:
            p.wA = _run_one(p.term, p.wA, p.delta, xa, 8, 8 + n, cnt)
            if not mp:
                p.wB = _run_one(p.term, p.wB, p.delta, xb, 8, 8 + n, cnt)
        else:
            _run_neg(p, xa, xb, 8, 8 + n, cnt)
        eL, p.hA = xa[8:], xa[-8:]
        if not mp:
            eR, p.hB = xb[8:], xb[-8:]


# ---------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------
def _sub(i, payload: bytes) -> bytes:
    odd = len(payload) & 1
    body = payload + (b"\0" if odd else b"")
    assert len(body) // 2 < 256
    return bytes([i | (0x40 if odd else 0), len(body) // 2]) + body


def _le16(v):
    return int(v & 0xFFFF).to_bytes(2, "little")


def _pass_meta(blk: Block) -> bytes:
    """ID_DECORR_TERMS, _WEIGHTS, _SAMPLES: stored from the decoder's last pass to its first"""
    n = len(blk.terms)
    order = range(n - 1, -1, -1)
    out = _sub(V.ID_DECORR_TERMS, bytes(((blk.terms[k] + 5) & 0x1F) | ((blk.deltas[k] & 7) << 5) for k in order))
    wt = bytearray()
    for k in order:
        a, b = blk.wbytes[k]
        wt.append(a & 0xFF)
        if not blk.mono_path:
            wt.append(b & 0xFF)
    out += _sub(V.ID_DECORR_WEIGHTS, bytes(wt))
    if blk.hist:
        # every entry in the layout of the decoder's last pass's term (read_decorr_samples sets dpp.term once)
        t0 = blk.terms[n - 1]
        cnt = 2 if t0 > 8 else (1 if t0 < 0 else t0)
        sm = bytearray()
        for k in order:
            la, lb = blk.hist[k]
            la = ([0] * cnt + list(la))[-cnt:]
            lb = ([0] * cnt + list(lb))[-cnt:]
            if t0 > 8:   # samples_A[0] is the newest
                sm += _le16(la[1]) + _le16(la[0])
                if not blk.mono_path:
                    sm += _le16(lb[1]) + _le16(lb[0])
            elif t0 < 0:
                sm += _le16(la[0]) + _le16(lb[0])
            else:
                for m in range(cnt):
                    sm += _le16(la[m])
                    if not blk.mono_path:
                        sm += _le16(lb[m])
        out += _sub(V.ID_DECORR_SAMPLES, bytes(sm))
    return out


def hist_layout_ok(blk: Block) -> bool:
    """the writer's history entries come back as given only when each pass's own term reads
    the layout of the last pass's term (same class and count)"""
    t0 = blk.terms[-1]
    return all((t > 8) == (t0 > 8) and (t < 0) == (t0 < 0) and (t > 8 or t < 0 or t == t0) for t in blk.terms)


def write_file(blocks, crcs) -> bytes:
    """the blocks as one lossless .wv: each coded by the synth encoder with an empty term
    list (its input array is then the words); then the pass metadata spliced in and the
    header's flags, CRC and ckSize rewritten"""
    b0 = blocks[0]
    nch = 1 if b0.mono else 2
    total = sum(len(b.words) for b in blocks)
    # (the blocks differ in length: one encoder call each, the medians restarting from zero)
    out, index = b"", 0
    for blk, crc in zip(blocks, crcs):
        assert 0 < len(blk.words) <= MAX_FRAMES
        x = np.array(blk.words, dtype=np.int64).astype(np.int32)
        if blk.mono:
            x = x[:, :1]
        elif blk.false_stereo:
            x[:, 1] = x[:, 0]
        f = S.encode_pcm(x, S.EncParams(nch=nch, terms=[], joint_stereo=False, false_stereo=blk.false_stereo,
                                        bytes_per_sample=blk.bps, block_samples=len(blk.words),
                                        block_index_start=index, total_override=total, mag_override=blk.mag))
        (off, n), = V.block_spans(f)
        assert off == 0
        body, p = bytearray(), 32
        while p < n:
            i, ln = f[p], f[p + 1] << 1
            hl = 2
            if i & 0x80:
                ln += (f[p + 2] << 9) + (f[p + 3] << 17)
                hl = 4
            if (i & 0x3F) == V.ID_DECORR_TERMS:
                assert ln == 0
                if not blk.sticky:
                    body += _pass_meta(blk)
            else:
                body += f[p:p + hl + ln]
            p += hl + ln
        hdr = bytearray(f[:32])
        flags = int.from_bytes(hdr[24:28], "little") & ~(JOINT_STEREO | CROSS_DECORR)
        if blk.joint:
            flags |= JOINT_STEREO
        if any(t < 0 for t in blk.terms):
            flags |= CROSS_DECORR
        assert (flags >> MAG_LSB) & 0x1F == blk.mag
        assert bool(flags & MONO_FLAG) == blk.mono and bool(flags & FALSE_STEREO) == blk.false_stereo
        hdr[4:8] = (24 + len(body)).to_bytes(4, "little")
        hdr[24:28] = flags.to_bytes(4, "little")
        hdr[28:32] = (crc & M32).to_bytes(4, "little")
        out += bytes(hdr) + bytes(body)
        index += len(blk.words)
    return out


# ---------------------------------------------------------------------------------------
# the choosers
# ---------------------------------------------------------------------------------------
def _sgn(v):
    return (v > 0) - (v < 0)


class Driver:
    """One channel of one driven positive-term pass, simulated sample-major with the
    (short) stores of a store schedule.  step(t, dir) picks the residual of frame t so
    that the weight moves by dir * delta (dir = +-1) when the outputs allow it:

    terms 1..8: the residual takes the sign of the pass's sample to grow the weight
    (UnpackUtils.cs:893-899); once |w| > 1024 the output then outgrows the sample, so a
    *reset* frame (output +-1, the residual cancelling the prediction: one delta toward 0)
    is put in whenever the next prediction would pass PRED_MAX.

    terms 17, 18: the sample is 2 s0 - s1 (or (3 s0 - s1) >> 1): an output of about half
    (a third of) the one before makes the next sample +-1..3, and then the residual's sign
    alone decides the step -- a halving chain from JUMP down, a jump back up, and one
    frame against the wanted direction after each jump."""
    PRED_MAX = 1 << 21
    OUT = 1 << 20
    JUMP = 1 << 15

    def __init__(self, term, delta, w0, rng, hist=None):
        self.term, self.d, self.w, self.rng = term, delta, w0, rng
        self.h = list(hist) if hist else [0] * 8   # last 8 outputs, oldest first

    def sam(self):
        h = self.h
        if self.term == 17:
            return i32(2 * h[-1] - h[-2])
        if self.term == 18:
            return i32(3 * h[-1] - h[-2]) >> 1
        return h[-self.term]

    def _next_sam(self, out):
        if self.term == 17:
            return 2 * out - self.h[-1]
        return (3 * out - self.h[-1]) >> 1

    def _pick(self, s, want, nd):
        """(residual, output): `want` = the residual's sign that moves the weight the wanted way;
        nd = the direction wanted of the next frame"""
        w, rng = self.w, self.rng
        pred = aw(w, s)
        if self.term <= 8:
            u = int(rng.integers(16, 33))
            out = pred + want * u
            if abs(out) <= self.OUT and ((abs(w) + 64) * abs(out)) >> 10 <= self.PRED_MAX:
                return want * u, out
            if s == 0 or abs(pred) < 2:   # (nothing to cancel: a small step)
                return want, pred + want
            out = _sgn(pred)              # reset: the residual cancels the prediction
            return out - pred, out
        # 17 / 18
        x0 = self.h[-1]
        cands = []
        div = 2 if self.term == 17 else 3
        for dn in (1, -1, 2, -2, 3, -3):   # halve: the next sample becomes dn
            o = (x0 + dn * (1 if self.term == 17 else 2)) // div
            for oo in (o, o + 1):
                ns = self._next_sam(oo)
                if ns and abs(ns) <= 3 and oo not in cands:
                    cands.append(oo)
        # the next residual will have the output's sign (it is about half of it): the next sample's
        # sign then decides the next step
        cands.sort(key=lambda oo: _sgn(self._next_sam(oo)) != nd * (_sgn(oo) or 1))
        jump = [sg * int(rng.integers(self.JUMP // 2, self.JUMP)) for sg in (1, -1)]
        order = cands + jump if abs(x0) >= 256 else jump + cands
        for out in order:
            r = out - pred
            if r and _sgn(r) == want and abs(r) <= RES_MAX // 2 and abs(out) <= self.OUT:
                return r, out
        for out in cands + [1]:            # no candidate moves the wanted way: stay bounded
            r = out - pred
            if r and abs(out) <= self.OUT:
                return r, out
        raise AssertionError("no bounded output")

    def step(self, direction, fixed=None, nxt=None):
        """one frame; `fixed`: a residual given from outside (the weight moves as it will);
        nxt(w) -> the direction wanted of the next frame"""
        s = self.sam()
        if fixed is not None:
            r, out = fixed, i32(aw(self.w, s) + fixed)
        elif direction == 0:   # a reset frame wherever it falls: output +-1 (one delta toward 0 when |prediction| >= 2)
            pred = aw(self.w, s)
            out = _sgn(pred) or 1
            r = (out - pred) or 1
            out = pred + r
        else:
            want = direction * (_sgn(s) or 1)
            r, out = self._pick(s, want, nxt(self.w + direction * self.d) if nxt else direction)
            out = i32(out)
        self.w = _upd(self.w, s, r, self.d)
        self.h = self.h[1:] + [out]
        return r, out

    def store(self):
        self.w = i16(self.w)


def drive(nfr, policyA, policyB, drvA, drvB, stores, stop=None, zeros=0):
    """residual words of up to nfr frames: channel A by drvA under policyA(t, w) -> +-1, channel B
    likewise (drvB None: zeros); `stores`: {frame: site} or None (an encoder that does not know of
    the stores); stop(t, drvA, drvB) -> True ends the block after frame t; zeros: that many leading
    frames of zero words (frames in which no weight moves: they shift the frame parity of a weight
    that alternates between two values)"""
    words = []
    for t in range(nfr):
        fixed = 0 if t < zeros else None
        a, _ = drvA.step(policyA(t, drvA.w), fixed=fixed, nxt=lambda w: policyA(t + 1, w))
        b = 0
        if drvB is not None:
            b, _ = drvB.step(policyB(t, drvB.w), fixed=fixed, nxt=lambda w: policyB(t + 1, w))
        words.append((a, b))
        done = stop is not None and stop(t, drvA, drvB)
        if stores is not None and t in stores:
            drvA.store()
            if drvB is not None:
                drvB.store()
        if done:
            break
    return words


def up(t, w):
    return 1


def down(t, w):
    return -1


def hold(level):
    """grow to `level`, then stay on it: a step down whenever the weight stands on it"""
    if level >= 0:
        return lambda t, w: 1 if w < level else -1
    return lambda t, w: -1 if w > level else 1


def noise_words(nfr, rng, bits=6, stereo=True):
    v = rng.integers(-(1 << bits), (1 << bits) + 1, size=(nfr, 2))
    return [(int(a), int(b) if stereo else 0) for a, b in v]


# ---------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    group: str
    blocks: list
    chunk: int                # the chunk size the residuals were chosen for
    seams: tuple = ()         # SEAMS this case is meant to make live
    clean: bool = True        # CRC-clean and unmuted at its own chunk size
    data: bytes = b""
    note: str = ""

    @property
    def nch(self):
        return 1 if self.blocks[0].mono else 2

    @property
    def header_crc(self):
        return [int.from_bytes(self.data[o + 28:o + 32], "little", signed=True) for o, _ in V.block_spans(self.data)]


_READS = {}


def expected(c: Case, chunk=None, sites=ALL_SITES) -> ReadResult:
    """the reader's decode of a case (its own chunk size by default), computed once and shared"""
    key = (c.name, chunk or c.chunk, tuple(sites))
    if key not in _READS:
        r = read(c.blocks, chunk or c.chunk, sites, header_crc=c.header_crc)
        r.samples.setflags(write=False)
        _READS[key] = r
    return _READS[key]


def _finish(name, group, blocks, chunk, seams, clean=True, note=""):
    """header CRCs from the reader at the case's own chunk size (a `foreign` case: from the
    reader with the stores switched off, as its encoder believes)"""
    sites = () if group == "foreign" else ALL_SITES
    r = read(blocks, chunk, sites)
    c = Case(name, group, blocks, chunk, tuple(seams), clean, write_file(blocks, r.crc), note)
    return c


def _lists(kind, term, pos):
    """a term list (decode order) with `term` at `pos` (0 first, 1 middle, 2 last) and every other
    pass transparent.  kinds: "one"; "rt4" a run-time list of 4 (no compile-time instantiation);
    "mid9" nine terms; "t16" sixteen; "fast" / "default" / "m5" (mono): the compile-time lists' shapes"""
    if kind == "one":
        return (term,), 0
    if kind == "fast":          # {17, 17}
        assert term == 17
        return (17, 17), (0, 1, 1)[pos]
    if kind in ("default", "m5"):   # stored {18, 18, 2, 3, -2}: decoded -2, 3, 2, 18, 18; mono {18, 18, 2, 3, 18}
        base = [-2, 3, 2, 18, 18] if kind == "default" else [18, 3, 2, 18, 18]
        k = base.index(term) if pos == 0 else len(base) - 1 - base[::-1].index(term)
        return tuple(base), k
    fill = {"rt4": [3, 5, 1, 4], "mid9": [2, 18, 3, 4, 17, 5, 6, 7, 8],
            "t16": [2, 18, 3, 4, 17, 5, 6, 7, 8, 1, 2, 3, 18, 4, 17, 5]}[kind]
    k = (0, len(fill) // 2, len(fill) - 1)[pos]
    fill = list(fill)
    fill[k] = term
    return tuple(fill), k


def _block(words, terms, k, delta, wA, wB=0, **kw):
    """a block whose pass k is the driven one (weight bytes wA / wB), every other pass transparent"""
    n = len(terms)
    deltas = tuple(delta if i == k else 0 for i in range(n))
    wbytes = tuple((wA, wB) if i == k else (0, 0) for i in range(n))
    return Block(words=words, terms=tuple(terms), deltas=deltas, wbytes=wbytes, **kw)


def _cross(name, group, chunk, term=1, kind="one", pos=0, mono=True, sign=1, delta=7, fs=False, joint=False,
           drive_b="same", phase_block=0, tail=100, seams=("call_end", "lane_wbad"), seed=1, known=True):
    """the driven weight(s) pass +-32767; the block runs on to `tail` frames past the next call end.
    drive_b (stereo): "same" both channels driven, "late" B from half the start weight (it crosses
    later), "hold" B held at 0, "only" A held at 0 and B driven.  known=False: the residuals are
    chosen without the stores (group "foreign").  phase_block: a leading block of that many frames"""
    rng = np.random.default_rng(seed)
    terms, k = _lists(kind, term, pos)
    mp = mono or fs
    pol = up if sign > 0 else down
    wb = 127 if sign > 0 else -128
    byA, byB = wb, 0
    polA, polB = pol, hold(0)
    if not mp:
        if drive_b == "same":
            byB, polB = wb, pol
        elif drive_b == "late":
            byB, polB = wb // 2, pol
        elif drive_b == "only":
            byA, byB, polA, polB = 0, wb, hold(0), pol
    lead = []
    if phase_block:
        lead = [_block(noise_words(phase_block, rng, stereo=not mp), terms, k, delta, 0, 0, mono=mono,
                       false_stereo=fs, joint=joint)]
    dA = Driver(term, delta, restore_weight(byA), rng)
    dB = None if mp else Driver(term, delta, restore_weight(byB), np.random.default_rng(seed + 1000))
    sched = store_frames(MAX_FRAMES, chunk, phase_block, not mp)
    ends = sorted(f for f, s in sched.items() if s != "frame8")
    driven = [d for d, q in ((dA, polA), (dB, polB)) if d is not None and q is pol]
    seen, state = set(), {"end": None}

    def stop(t, a, b):   # (runs before the frame's store: a weight is seen past the edge in the frames before it)
        for d in driven:
            if abs(d.w) > 32767:
                seen.add(id(d))
        if state["end"] is None and len(seen) == len(driven):
            state["end"] = min(next(e for e in ends if e >= t) + tail, MAX_FRAMES - 1)
        return state["end"] is not None and t >= state["end"]

    words = drive(MAX_FRAMES, polA, polB, dA, dB, sched if known else None, stop)
    assert state["end"] is not None, name
    blk = _block(words, terms, k, delta, byA, byB, mono=mono, false_stereo=fs, joint=joint)
    return _finish(name, group, lead + [blk], chunk, seams, clean=known)


def _hold_case(name, group, chunk, level, mono, term=1, kind="one", pos=0, delta=7, wbyte=125, frames=None, seed=5,
               seams=("lane_wbad",), joint=False):
    """the weight(s) climb to `level` and stay on it to the block end (max |w| at group starts == level
    when level - w0 is a multiple of delta)"""
    terms, k = _lists(kind, term, pos)
    w0 = restore_weight(wbyte)
    assert (level - w0) % delta == 0
    st = store_frames(MAX_FRAMES, chunk, 0, not mono)
    for zeros in (0, 1):   # (a held weight alternates level - delta / level: the one leading zero frame
        #                     puts `level` on the even frames, where the group starts are)
        rng = np.random.default_rng(seed)
        dA = Driver(term, delta, w0, rng)
        dB = None if mono else Driver(term, delta, w0, np.random.default_rng(seed + 1000))
        state = {"at": None}

        def stop(t, a, b):
            if state["at"] is None and a.w >= level and (b is None or b.w >= level):
                state["at"] = t
            return state["at"] is not None and t >= state["at"] + 300 or t == MAX_FRAMES - 1

        words = drive(MAX_FRAMES, hold(level), hold(level), dA, dB, st, stop, zeros=zeros)
        blk = _block(words, terms, k, delta, wbyte, 0 if mono else wbyte, mono=mono, joint=joint)
        if read([blk], chunk).gmax[0] == level:
            break
    return _finish(name, group, [blk], chunk, seams)


def _edge(name, sign, over, chunk=1001, delta=7, seed=9):
    """mono term 1: the weight reaches exactly +32767 (start 1008) / -32768 (start -1016) in the last
    frame of a call (over=0: the store is the identity), or a frame earlier and takes one more step
    (over=1: the store wraps it).  Held one step inside the edge the weight alternates between two
    values, so which call end fits is tried out with the reader."""
    wb = 125 if sign > 0 else -127
    w0 = restore_weight(wb)
    edge = 32767 if sign > 0 else -32768
    assert (edge - w0) % delta == 0
    near = edge - sign * delta
    st = store_frames(MAX_FRAMES, chunk, 0, False)
    ends = sorted(st)
    for skip in range(6):
        d = Driver(1, delta, w0, np.random.default_rng(seed))
        state = {"end": None}

        def pol(t, w):
            e = state["end"]
            if e is not None and (t == e or (over and t == e - 1)):
                return sign
            return hold(near)(t, w)

        def stop(t, a, b):
            if state["end"] is None and a.w == near:
                state["end"] = [x for x in ends if x >= t + 8][skip]
            return state["end"] is not None and t >= state["end"] + 50

        words = drive(MAX_FRAMES, pol, None, d, None, st, stop)
        blk = _block(words, (1,), 0, delta, wb, 0, mono=True)
        r = read([blk], chunk)
        at = [x for x in r.stores if x[1] == state["end"]][0]
        if at[4] == edge + (sign * delta if over else 0) and len(r.changed) == over:
            break
    else:
        raise AssertionError(name)
    c = _finish(name, "edge", [blk], chunk, ("call_end",) if over else ())
    c.note = "over" if over else "identity"
    return c


def _seam8(name, chunk, mono=False, fs=False, cut_short=False, seed=21, delta=7, term=1, kind="one"):
    """the weights are in range at a call end and pass +32767 within the next 8 frames, then come
    back into range before that call ends: only a store after frame 8 can wrap them.  Siblings
    without that store: chunk 13, mono, false stereo, a call cut under 16 frames by the block end.
    kind / term: the driven pass inside a longer list (the default list: the two-wave kernel's own)"""
    rng = np.random.default_rng(seed)
    terms, kk = _lists(kind, term, 0)
    mp = mono or fs
    wb = 125
    w0 = restore_weight(wb)
    near = 32767 - delta    # 32760: in range
    dA = Driver(term, delta, w0, rng)
    dB = None if mp else Driver(term, delta, w0, np.random.default_rng(seed + 1000))
    st = store_frames(MAX_FRAMES, chunk, 0, not mp)
    ends = sorted(f for f, s in st.items() if s != "frame8")
    state = {"e": None}

    def pol(t, w):
        e = state["e"]
        if e is not None and e < t <= e + 16:
            k = t - e          # frames 1..16 of the call after the chosen call end
            if k <= 4:
                return 1       # 32760 (or 32753) -> past 32767 within the first 8 frames
            if k <= 8:
                return 1 if w <= 32767 + delta else -1
            return -1 if w > near - delta else 1   # back inside before any later store (if it did not wrap)
        return hold(near)(t, w)

    def stop(t, a, b):
        if state["e"] is None and a.w >= near - delta and (b is None or b.w >= near - delta):
            state["e"] = next(x for x in ends if x >= t + 16)
            if cut_short:   # the block ends 12 frames into the next call: a call under 16 frames, no frame-8 store
                st.pop(state["e"] + 8, None)
        if state["e"] is None:
            return False
        return t >= state["e"] + (12 if cut_short else 60)

    words = drive(MAX_FRAMES, pol, pol, dA, dB, st, stop)
    blk = _block(words, terms, kk, delta, wb, 0 if mp else wb, mono=mono, false_stereo=fs)
    has8 = not mp and chunk >= 16 and not cut_short
    return _finish(name, "seam8", [blk], chunk, ("frame8",) if has8 else ())


def _one_group(name, chunk, seed=31, delta=7):
    """mono term 1, the chunk no multiple of 8: at a group start the weight is in range (32753 or
    32760); inside the group it passes 32767 and a call ends (the store wraps it); the block ends
    with that group.  A lane that only looked for |w| > 32767 at group starts would keep this block
    and decode the frame after the call end with the unwrapped weight (test_decorr_seams_host checks
    that such a decode -- the reader without stores -- neither mutes nor matches)."""
    wb = 125
    near = 32767 - delta
    st = store_frames(MAX_FRAMES, chunk, 0, False)
    limit = (1 << MAG) + 2
    # (held, the weight and the outputs run through a short cycle: which call end and which place for a
    # reset frame before the steps up fit is tried out with the reader)
    for skip, back in [(k, b) for k in range(3) for b in (3, 4, 5, 6, 99)]:
        d = Driver(1, delta, restore_weight(wb), np.random.default_rng(seed))
        state = {"e": None}

        def pol(t, w):
            e = state["e"]
            if e is None or t < e - 6:
                return hold(near)(t, w)
            return 0 if t == e - back else 1   # the group of the call end: a reset frame, else up

        def stop(t, a, b):
            if state["e"] is None and a.w >= near - delta and t % GF == GF - 1:
                # a call end at frame 6 of its group: three steps up fit before it, and one frame after it, which
                # a decode that kept the unwrapped weight gets wrong without running past the mute limit
                state["e"] = [x for x in sorted(st) if x >= t + 16 and x % GF == 6][skip]
            return state["e"] is not None and t == state["e"] + 1

        words = drive(MAX_FRAMES, pol, None, d, None, st, stop)
        blk = _block(words, (1,), 0, delta, wb, 0, mono=True)
        r, none = read([blk], chunk), read([blk], chunk, ())
        if (len(r.changed) == 1 and r.changed[0][1] == state["e"] and none.mute_frame == [None] and
                none.gmax[0] <= 32767 and none.samples[-1] != r.samples[-1] and
                abs(int(none.samples[-1])) <= limit):
            break
    else:
        raise AssertionError(name)
    c = _finish(name, "one_group", [blk], chunk, ("call_end", "lane_wbad"))
    c.note = f"call end {state['e']}"
    return c


def _sticky(name, chunk, mono, seed=41, delta=7):
    """two blocks, the second without pass metadata: the first ends with the weight past 32767 in its
    last (cut) call, so the block-end store decides what the second block starts from"""
    rng = np.random.default_rng(seed)
    wb = 125
    w0 = restore_weight(wb)
    near = 32767 - delta
    dA = Driver(1, delta, w0, rng)
    dB = None if mono else Driver(1, delta, w0, np.random.default_rng(seed + 1000))
    stall = store_frames(MAX_FRAMES, chunk, 0, not mono)
    ends = sorted(f for f, s in stall.items() if s != "frame8")
    state = {"e": None}

    def pol(t, w):
        e = state["e"]
        if e is not None and t > e + 8:
            return 1                      # after a call end (+ frame 8): climb past the edge
        return hold(near)(t, w)

    def stop(t, a, b):
        if state["e"] is None and a.w >= near - delta and (b is None or b.w >= near - delta):
            state["e"] = next(x for x in ends if x >= t + 16)
        return state["e"] is not None and t >= state["e"] + 8 + 12   # the block ends 20 frames into a call

    words = drive(MAX_FRAMES, pol, pol, dA, dB, stall, stop)
    n1 = len(words)
    b1 = _block(words, (1,), 0, delta, wb, 0 if mono else wb, mono=mono)
    # the second block: the stored (wrapped) weights continue, chosen with its own call schedule
    dA.store()
    if dB is not None:
        dB.store()
    st2 = store_frames(600, chunk, n1, not mono)
    words2 = drive(600, up, up, dA, dB, st2)
    b2 = Block(words=words2, terms=b1.terms, deltas=b1.deltas, sticky=True, mono=mono)
    return _finish(name, "sticky", [b1, b2], chunk, ("block_end",))


def _foreign_sticky(name, chunk=1001, seed=45, delta=7):
    """mono: a block written without knowledge of the stores, cut inside the call that mutes it at a
    frame where the (exploded) pass has its weight outside int16 -- the muting call's passes run to its
    end and store (UnpackUtils.cs:556-607 precede the mute test) -- then a block without pass metadata
    whose residuals continue the state those stores left"""
    wb, near = 125, 32767 - delta
    d0 = Driver(1, delta, restore_weight(wb), np.random.default_rng(seed))
    ends = sorted(store_frames(MAX_FRAMES, chunk, 0, False))
    state = {"e": None}

    def pol(t, w):   # held just inside the edge, then over it in a call's last frames: the store lands near -32768
        e = state["e"]
        return hold(near)(t, w) if e is None or t < e - 2 else 1

    def stop(t, a, b):
        if state["e"] is None and a.w == near:
            # held, the weight is on near - delta after every other frame: after frame e - 3 too, and the
            # three frames up that follow a reset frame fit
            state["e"] = next(x for x in ends if x >= t + 16 and (x - t) % 2 == 0)
        return state["e"] is not None and t >= state["e"] + chunk - 1

    words = drive(MAX_FRAMES, pol, None, d0, None, None, stop)   # (no stores: the encoder does not know of them)
    base = _block(words, (1,), 0, delta, wb, 0, mono=True)
    full = read([base], chunk)
    mute = full.mute_frame[0]
    assert mute is not None
    # the one pass sample-major, with the stores, for its weight at every frame of the muting call
    d = Driver(1, delta, restore_weight(wb), np.random.default_rng(0))
    st = store_frames(len(words), chunk, 0, False)
    n1 = None
    for t, (r, _) in enumerate(words):
        d.step(1, fixed=r)
        if t >= mute + 8 and abs(d.w) > 32767 and (t + 1) % chunk:
            n1 = t + 1
            break
        if t in st:
            d.store()
    assert n1 is not None and n1 // chunk == mute // chunk, name
    b1 = dataclasses.replace(base, words=words[:n1])
    r1 = read([b1], chunk)
    assert r1.mute_frame[0] == mute and r1.changed and r1.changed[-1][1:3] == (n1 - 1, "block_end")
    term, dl, wA, _, hA, _ = r1.final[0]
    d2 = Driver(term, dl, wA, np.random.default_rng(seed + 1), hist=hA)
    # the exploded history is cancelled by the first residual; the rest climbs as usual
    words2 = []
    st2 = store_frames(700, chunk, n1, False)
    for t in range(700):
        if t == 0:
            r = i32(1 - aw(d2.w, d2.sam())) or 1
            d2.step(1, fixed=r)
        else:
            r, _ = d2.step(1)
        words2.append((r, 0))
        if t in st2:
            d2.store()
    b2 = Block(words=words2, terms=b1.terms, deltas=b1.deltas, sticky=True, mono=True)
    # header CRCs: block 1 as its encoder believes (no stores), block 2 from the real decode
    crc1 = read([b1], chunk, ()).crc[0]
    crc2 = read([b1, b2], chunk).crc[1]
    return Case(name, "foreign", [b1, b2], chunk, ("mute_call", "block_end"), False, write_file([b1, b2], [crc1, crc2]))


def _clamp(name, term, outward, chunk=1000, seed=51, delta=5, joint=False, kind="one"):
    """stereo terms -1 / -2 / -3 from +1024 / -1024 (bytes 127 / -128): noise words whose signs push the
    weights outward (they stay on the clamp) or inward and back"""
    rng = np.random.default_rng(seed)
    nfr = 400
    terms, k = _lists(kind, term, 0)
    blk = _block([], terms, k, delta, 127, -128, joint=joint)
    # sample-major simulation of the one pass to pick the signs (the other passes are transparent)
    p = _Pass(term, delta)
    p.wA, p.wB = restore_weight(127), restore_weight(-128)
    hL, hR, scratch = [0] * 8, [0] * 8, new_counts()
    words = []
    for t in range(nfr):
        mL, mR = int(rng.integers(8, 64)), int(rng.integers(8, 64))
        phase = (t // 40) % 2 if not outward else 0
        # wanted moves: A up / B down (outward), or the other way every other 40 frames
        da, db = (1, -1) if phase == 0 else (-1, 1)
        best = None
        for sl in (1, -1):
            for sr in (1, -1):
                q = _Pass(term, delta)
                q.wA, q.wB = p.wA, p.wB
                eL, eR = hL + [sl * mL], hR + [sr * mR]
                _run_neg(q, eL, eR, 8, 9, scratch)
                score = (_sgn(q.wA - p.wA) == da or (q.wA == p.wA and abs(p.wA) == 1024 and da * p.wA > 0)) + \
                        (_sgn(q.wB - p.wB) == db or (q.wB == p.wB and abs(p.wB) == 1024 and db * p.wB > 0))
                small = max(abs(eL[8]), abs(eR[8])) <= 1 << 12
                key = (small, score)
                if best is None or key > best[0]:
                    best = (key, sl * mL, sr * mR, q, eL, eR)
        _, l, r, q, eL, eR = best
        if not best[0][0]:   # outputs grew: a frame of words that cancel the predictions
            q = _Pass(term, delta)
            q.wA, q.wB = p.wA, p.wB
            l = r = 0
            eL, eR = hL + [0], hR + [0]
            _run_neg(q, eL, eR, 8, 9, scratch)
            l, r = -eL[8] + 1, -eR[8] - 1
            q = _Pass(term, delta)
            q.wA, q.wB = p.wA, p.wB
            eL, eR = hL + [l], hR + [r]
            _run_neg(q, eL, eR, 8, 9, scratch)
        p = q
        hL, hR = eL[1:], eR[1:]
        words.append((l, r))
    blk.words = words
    return _finish(name, "clamp", [blk], chunk, ("clamp",))


def _wrap32(name, term, mono, seed=61):
    """terms 17 / 18 from histories of +-2^30 in a 32-bit container (header magnitude 30: limit 2^30 + 2;
    31 would wrap the limit): 2 s0 - s1 and 3 s0 - s1 wrap int32 (the >> 10 of the 64-bit product does
    not: _wrap32_product).  Each residual (at most 2^27: what the word coder takes) steers the output
    toward +-2^30 on the prediction's side, so term 17 at weight -1024 keeps wrapping frame after frame.
    Stereo: channel A starts from weight 129 and the histories (0, 2^30): its first sample is INT32_MIN."""
    rng = np.random.default_rng(seed)
    nfr, top, rmax = 160, 1 << 30, 1 << 27
    if mono:
        hist, wbytes = ((-0x1F00, 0x1EFF), ()), ((127, 0),)
    else:
        hist, wbytes = ((0, 0x1F00), (0x1F00, -0x1F00)), ((16, -128),)
    blk = Block(words=[], terms=(term,), deltas=(7,), wbytes=wbytes, hist=(hist,), mono=mono, bps=4, mag=30)
    ds = [Driver(term, 7, restore_weight(wbytes[0][c]), rng, hist=[0] * 6 + [exp2s(v) for v in hist[c]])
          for c in range(1 if mono else 2)]
    st = store_frames(nfr, 37, 0, not mono)
    words = []
    for t in range(nfr):
        row = []
        for d in ds:
            pred = aw(d.w, d.sam())
            target = (_sgn(pred) or 1) * (top - int(rng.integers(0, 1 << 12)))
            r = max(-rmax, min(rmax, target - pred)) or 1
            d.step(1, fixed=r)
            row.append(r)
        words.append((row[0], row[1] if len(row) > 1 else 0))
        if t in st:
            for d in ds:
                d.store()
    blk.words = words
    c = _finish(name, "wrap32", [blk], 37, ())
    c.clean = False   # (it may mute: the outputs are what the arithmetic gives)
    return c


def _wrap32_product(name, seed=63, delta=7):
    """mono term 17: the >> 10 of the 64-bit product leaves int32 only where |weight * sam| >= 2^41, which the
    two files above never reach (their weights settle where the prediction is about 2^30).  Here the weight first
    climbs to 2048 over small values; then two frames of output +-1 and four large ones: outputs 2^26, 2^28 and
    0.9 * 2^30 make the sample 2 s0 - s1 about 1.55 * 2^30 (inside int32), the product's >> 10 about 3.1 * 2^30,
    which wraps to about -0.9 * 2^30: within the mute limit, so the block's last sample is made of a wrapped
    prediction.  Each residual is at most 2^27."""
    d = Driver(17, delta, restore_weight(127), np.random.default_rng(seed))
    words = []
    while d.w < 2048:
        words.append((d.step(1)[0], 0))
        assert len(words) < 1000, name
    for _ in range(2):
        words.append((d.step(0)[0], 0))
    for target in (1 << 26, 1 << 28, int(0.9 * (1 << 30))):
        r = (target - aw(d.w, d.sam())) or 1
        assert abs(r) <= 1 << 27, (name, r)
        words.append((d.step(1, fixed=r)[0], 0))
    true = (d.w * d.sam() + 512) >> 10
    assert abs(d.sam()) < B31 and true != i32(true) and abs(i32(true)) < 1 << 30, (name, d.w, d.sam(), true)
    words.append((d.step(1, fixed=-_sgn(i32(true)) * (1 << 27))[0], 0))
    blk = Block(words=words, terms=(17,), deltas=(delta,), wbytes=((127, 0),), mono=True, bps=4, mag=30)
    c = _finish(name, "wrap32", [blk], 37, ())   # (the weight passes no store's range: any chunk size decodes alike)
    return c


def _build():
    C = []
    # cross_end / cross_neg: mono and stereo, chunks 1000 and 4096
    for sign, grp in ((1, "cross_end"), (-1, "cross_neg")):
        for mono in (True, False):
            for chunk in (1000, 4096):
                # (one mono file on the mono compile-time list, term 2 driven: its two-wave and lane instantiations)
                m5 = dict(term=2, kind="m5") if (grp, mono, chunk) == ("cross_end", True, 4096) else {}
                C.append(_cross(f"{grp}_{'m' if mono else 's'}_c{chunk}", grp, chunk, mono=mono, sign=sign,
                                seed=100 + chunk + mono + 7 * (sign > 0), **m5))
    # edge: both sides of +32767 and -32768
    for sign in (1, -1):
        for over in (0, 1):
            C.append(_edge(f"edge_{'pos' if sign > 0 else 'neg'}_{'over' if over else 'on'}", sign, over))
    # seam8 and its siblings without a frame-8 store
    C.append(_seam8("seam8_s_c1000", 1000))
    C.append(_seam8("seam8_s_c16", 16, seed=27))     # calls of exactly 16 frames: the least with a frame-8 store
    C.append(_seam8("seam8_sib_c13", 13, seed=23))
    C.append(_seam8("seam8_sib_short", 1000, cut_short=True, seed=24))
    C.append(_seam8("seam8_sib_mono", 1000, mono=True, seed=25))
    C.append(_seam8("seam8_sib_fs", 1000, fs=True, seed=26))
    C.append(_one_group("one_group_c37", 37))
    C.append(_seam8("seam8_default_t2", 1000, seed=28, term=2, kind="default"))   # (the two-wave kernel's frame-8 store)
    # A only / B only / both at different frames, joint stereo off and on
    for joint in (False, True):
        j = "_joint" if joint else ""
        C.append(_cross(f"A_only{j}", "ab", 1000, mono=False, drive_b="hold", joint=joint, seed=200 + joint))
        C.append(_cross(f"B_only{j}", "ab", 1000, mono=False, drive_b="only", joint=joint, seed=210 + joint))
        C.append(_cross(f"AB_apart{j}", "ab", 1000, mono=False, drive_b="late", joint=joint, seed=220 + joint))
    # position: the driven pass first / middle / last of several lists
    C.append(_cross("pos_t16_first_t2", "position", 1000, term=2, kind="t16", pos=0, mono=False, seed=301))
    C.append(_cross("pos_t16_mid_t17", "position", 1000, term=17, kind="t16", pos=1, mono=False, seed=302))
    C.append(_cross("pos_t16_last_t8", "position", 1000, term=8, kind="t16", pos=2, mono=True, seed=303))
    C.append(_cross("pos_mid9_first_t18", "position", 1000, term=18, kind="mid9", pos=0, mono=False, seed=304))
    C.append(_cross("pos_mid9_mid_t8", "position", 1000, term=8, kind="mid9", pos=1, mono=False, seed=305))
    C.append(_cross("pos_mid9_last_t2", "position", 1000, term=2, kind="mid9", pos=2, mono=False, seed=306))
    C.append(_cross("pos_rt4_first_t8", "position", 1000, term=8, kind="rt4", pos=0, mono=False, seed=307))
    C.append(_cross("pos_rt4_mid_t18", "position", 1000, term=18, kind="rt4", pos=1, mono=True, seed=308))
    C.append(_cross("pos_rt4_last_t17", "position", 1000, term=17, kind="rt4", pos=2, mono=False, seed=309))
    C.append(_cross("pos_fast_first", "position", 1000, term=17, kind="fast", pos=0, mono=False, seed=310))
    C.append(_cross("pos_default_t18_last", "position", 1000, term=18, kind="default", pos=2, mono=False, seed=311))
    # hug / control: never a wrap
    for mono in (True, False):
        m = "m" if mono else "s"
        C.append(_hold_case(f"hug_{m}", "hug", 1000, 32767 - 8 * 7, mono, seed=400 + mono))
        C.append(_hold_case(f"control_{m}", "control", 1000, 16340, mono, wbyte=127, seed=410 + mono))
    C.append(_hold_case("hug_default_t2", "hug", 1000, 32767 - 8 * 7, False, term=2, kind="default", pos=0,
                        seed=420))
    C.append(_hold_case("hug_rt4_t8", "hug", 1000, 32767 - 8 * 7, False, term=8, kind="rt4", pos=0, seed=421))
    C.append(_hold_case("hug_t16_t2", "hug", 1000, 32767 - 8 * 7, False, term=2, kind="t16", pos=0, seed=422))
    # foreign: an encoder that does not know of the stores
    C.append(_cross("foreign_m_c1000", "foreign", 1000, mono=True, known=False, tail=700, seed=500,
                    seams=("call_end", "mute_call")))
    C.append(_cross("foreign_s_c1000", "foreign", 1000, mono=False, known=False, tail=700, seed=501,
                    seams=("call_end", "mute_call")))
    C.append(_foreign_sticky("foreign_sticky_m"))
    C.append(_sticky("sticky_m", 1000, True))
    C.append(_sticky("sticky_s", 1000, False, seed=42))
    C.append(_cross("shifted_s", "shifted", 1000, mono=False, phase_block=333, seed=601))
    for term in (-1, -2, -3):   # each file: outward (the weights stay on the clamp), then inward and back, every 40 frames
        C.append(_clamp(f"clamp_t{-term}", term, False, seed=710 - term, joint=term == -2))
    C.append(_clamp("clamp_default_t2", -2, False, seed=720, kind="default"))   # (the two-wave kernel's own list)
    C.append(_wrap32("wrap32_t17_s", 17, False))
    C.append(_wrap32("wrap32_t18_m", 18, True, seed=62))
    C.append(_wrap32_product("wrap32_t17_product"))
    assert len({c.name for c in C}) == len(C)
    return C


_CASES = None


def cases() -> list:
    """every case, built once"""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


_REFS = {}


def reference(c: Case, chunk: int):
    """the oracle's decode of a case, computed once and shared (read-only)"""
    from oracle import oracle as O
    key = (c.name, chunk)
    if key not in _REFS:
        r = O.decode_file(c.data, chunk=chunk)
        r.samples.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]
