// wv_tpeak.h -- per-channel true peak of the decoded ints (wvg_batch_true_peak, BS.1770
// Annex 2).
//
// The true peak of a channel is the maximum of its O-times oversampled signal, O = 4, 2 or 1.
// The interpolator is a 12-tap polyphase filter whose taps are integers scaled by 2^24
// (kTpTaps; include/wvgpu.h has the formula), so an output y[n][p] = sum_j c_q[j] * x[n-5+j]
// is an exact integer in units of 2^-(k+24) of full scale, |y| < 2^56 for any int32 input.
// Per channel: max |y| and the first n * O + p that attains it, the outputs above 0 dBTP,
// and the sample peak with its first frame.
//
// Two passes, no atomics, as wv_levels.h:
//   tiles:   one job per (file, frame tile) reduces its part to one TpRecord per channel;
//   combine: one wave per (file, channel) folds that channel's partials.
// The fold is (larger magnitude, then smaller position): associative and commutative, so
// neither the tile order nor a butterfly's order can change a record.
//
// The code is compiled for the host and the device (WVF_HD): the kernels (wv_tpeak.hip) run
// it with the tile in LDS and one call per thread, the host entry wvg_true_peak_ints with the
// tile in memory and the thread index as a loop.
//   tp_load:  the tile and its halo, (nvalid + 11) x C ints starting 5 frames before the
//             tile, are contiguous in the batch output: they are read once, 16 bytes a work
//             item where the address is aligned and all four ints lie in the file, single
//             ints otherwise, zeros outside the file, and written channels first.  A thread
//             reports whether one of its ints lies outside +-2^28 (see Arithmetic).
//   tp_scan:  row c is shared by S = tp_segments(C) threads; thread c * S + s owns the R =
//             tp_run(C) consecutive frames s * R ..: it reads each of its R + 11 words once
//             and slides the 12-value window in registers (the loop is unrolled 12 times,
//             so the window rotates by renaming).  Phase 0 is the sample itself: the thread
//             keeps the sample peak and joins it as the candidate (peak * 2^24, frame * O)
//             at the end.
// The tile: row c starts at tile[c * pitch] and holds the frames from 5 before the tile's
// first; T = S * R.  R is odd, so the S lanes of a row, R words apart, fall on
// different banks modulo S; and pitch is an odd multiple of S where S < 32, so the 32 / S rows
// that one 32-lane group of a ds_read_b32 covers fill the banks of each residue class modulo
// S exactly once.
//
// Arithmetic.  Both forms are exact, so they give the same integers:
//   int64:  acc += (int64)c * x, for any int32 input (|y| < 2^56);
//   double: acc = fma(c, x, acc) while every |x| of the tile and its halo is at most 2^28:
//           every partial sum is below 2^28 * 31,247,516 < 2^53.  Chosen per tile from the
//           data (uniform for the workgroup), whatever the file's depth.
// Positions inside a tile fit 32 bits (at most 4,352 frames x 4); "none" is the all-ones
// pattern, the largest unsigned value, and peak 0: a real zero at any position beats it.
// Every offset into the batch output is 64-bit.
#pragma once
#include <stdint.h>

#include "wv_format.h"

// (the host compiler does not know the pragma; there the loops are the optimiser's)
#if defined(__HIPCC__)
#define TP_UNROLL _Pragma("unroll")
#else
#define TP_UNROLL
#endif

namespace wvg {

constexpr uint32_t kTpTileInts = 4530;    // values of one tile and its halo, at most (see tp_run)
constexpr uint32_t kTpThreads = 256;      // threads of one workgroup of the tile kernel
constexpr uint32_t kTpWave = 64;          // lanes of a wave: the widest butterfly
constexpr uint32_t kTpMaxChannels = 255;  // ID_CHANNEL_INFO's one-byte count
constexpr uint32_t kTpTaps_n = 12;        // taps of one phase
constexpr uint32_t kTpBefore = 5, kTpAfter = 6;  // the halo: frames before and after the tile's own
constexpr uint32_t kTpHalo = kTpBefore + kTpAfter;
constexpr uint32_t kTpUnroll = 12;        // steps of one trip of the scan: the window's length
constexpr uint32_t kTpCombineLanes = 64;  // threads of one workgroup (one wave) of the combine kernel
constexpr uint32_t kTpNone = 0xFFFFFFFFu;
constexpr int32_t kTpNarrow = 1 << 28;    // |x| up to here: the double form is exact

// round(h_q[j] / sum_j h_q[j] * 2^24), h_q[j] = sinc(pi t) cos^2(pi t / 12), t = (j - 5) - q / 4
constexpr int32_t kTpTaps[4][kTpTaps_n] = {
    {0, 0, 0, 0, 0, 16777216, 0, 0, 0, 0, 0, 0},
    {-27363, 173728, -504882, 1159730, -2707526, 15032977, 4840980, -1734883, 775827, -310666, 82102, -2808},
    {-16528, 173638, -564942, 1343293, -3036105, 10489252, 10489252, -3036105, 1343293, -564942, 173638, -16528},
    {-2808, 82102, -310666, 775827, -1734883, 4840980, 15032977, -2707526, 1159730, -504882, 173728, -27363},
};

// the factor a rate gets: BS.1770-4 Annex 2's "4x at 48 kHz, proportionally less above"
WVF_HD uint32_t tp_oversample(int64_t rate) { return rate < 96000 ? 4u : rate < 192000 ? 2u : 1u; }

// threads that share one row of the tile: the largest power of two <= 256 / nch
WVF_HD uint32_t tp_segments(uint32_t nch) {
    uint32_t s = kTpThreads;
    while (s > 1u && s * nch > kTpThreads) s >>= 1;
    return s;
}

// frames of one thread's run: the largest odd count with nch * (S * run + 11) <= kTpTileInts,
// 17 for mono and stereo, 1 .. 33 (128 < nch * S <= 256)
WVF_HD uint32_t tp_run(uint32_t nch) {
    const uint32_t c = nch ? nch : 1u, r = (kTpTileInts / c - kTpHalo) / tp_segments(c);
    return r ? (r - 1u) | 1u : 1u;
}

// frames of one tile of an nch-channel file (1 <= nch <= 255): every thread of a row a whole run
WVF_HD uint32_t tp_tile_frames(uint32_t nch) { return tp_segments(nch) * tp_run(nch); }

// words from one row of the tile to the next
WVF_HD uint32_t tp_pitch(uint32_t nch) {
    const uint32_t s = tp_segments(nch), need = tp_tile_frames(nch) + kTpHalo;
    return s >= 32u ? need : need + ((s - need) & (2u * s - 1u));
}

// nch * tp_pitch(nch) <= kTpTileInts + nch * (2 S - 1) < kTpTileInts + 512; a discarded step of
// the last trip of a run may read up to 2 * kTpUnroll + kTpHalo words past the last row's own.
// 20,312 bytes: with the slots below 20 KiB, eight workgroups a CU
constexpr uint32_t kTpLdsInts = kTpTileInts + 512 + 2 * kTpUnroll + kTpHalo + 1;

struct TpJob {
    uint64_t in_off;   // first int of the tile's first frame in the batch output
    uint64_t frame0;   // the file's frame index of the tile's first frame
    uint64_t frames;   // frames of the file: the halo holds zeros outside them
    uint64_t part;     // index of the tile's channel-0 record in the partials
    uint32_t nvalid;   // frames of the tile (1 .. tp_tile_frames(nch))
    uint32_t nch;      // channels of the file
    uint32_t k;        // full scale is 2^k (7, 15, 23, 31)
    uint32_t o_rate;   // the factor the file's rate gets (oversample = 0)
};

// one per (measurable file, channel): where its partials are
struct TpFold {
    uint64_t part;     // index of tile 0's record of this channel in the partials
    uint32_t ntiles;   // records to fold, `nch` records apart
    uint32_t nch;
    uint32_t k;
    uint32_t o_rate;
};

// wvg_channel_true_peak (include/wvgpu.h), field for field
struct TpRecord {
    int64_t true_peak, true_peak_pos, overs, sample_peak, sample_peak_frame;
    int32_t oversample, k;
};

typedef int32_t tp_i4 __attribute__((vector_size(16)));

// a thread's result inside one tile
struct TpAcc {
    uint64_t peak;   // max |y|
    uint32_t pos;    // frame in the tile * O + p, kTpNone none
    uint32_t overs;
    uint32_t speak;  // max |x| (2^31 for INT32_MIN)
    uint32_t sframe; // frame in the tile, kTpNone none
};

WVF_HD TpAcc tp_acc_none() {
    TpAcc a;
    a.peak = 0;
    a.pos = kTpNone;
    a.overs = 0;
    a.speak = 0;
    a.sframe = kTpNone;
    return a;
}

// (by value, fields into scalars first: a select between the two references would keep
// both structs in memory)
WVF_HD TpAcc tp_merge(const TpAcc a, const TpAcc b) {
    const uint64_t ap = a.peak, bp = b.peak;
    const uint32_t apos = a.pos, bpos = b.pos, as = a.speak, bs = b.speak, af = a.sframe, bf = b.sframe;
    const bool tb = bp > ap || (bp == ap && bpos < apos);
    const bool sb = bs > as || (bs == as && bf < af);
    TpAcc r;
    r.peak = tb ? bp : ap;
    r.pos = tb ? bpos : apos;
    r.overs = a.overs + b.overs;
    r.speak = sb ? bs : as;
    r.sframe = sb ? bf : af;
    return r;
}

// `src`: the tile's first int in the batch output.  Returns whether one of the ints this
// thread read lies outside +-2^28
WVF_HD bool tp_load(const TpJob &j, const int32_t *src, int32_t *tile, uint32_t tid, uint32_t nthreads) {
    const uint32_t nch = j.nch, pitch = tp_pitch(nch), lead = kTpBefore * nch, total = (j.nvalid + kTpHalo) * nch;
    // value e of the tile is channel e % nch of row index e / nch and int g0 + e of the file
    const int64_t g0 = (int64_t)(j.frame0 * nch) - (int64_t)lead, gn = (int64_t)(j.frames * nch);
    const int32_t *p0 = src - lead;  // (not dereferenced outside the file)
    uint32_t head = (0u - ((uint32_t)((uintptr_t)src >> 2) - lead)) & 3u;
    if (head > total) head = total;
    // item 0: the values before the first 16-byte boundary; item i >= 1: values head + 4 (i - 1) .. + 3
    const uint32_t nitems = 1u + (total - head + 3u) / 4u;
    uint32_t wide = 0;
    for (uint32_t i = tid; i < nitems; i += nthreads) {
        const int32_t e0 = (int32_t)head + 4 * ((int32_t)i - 1);  // >= -4
        const int64_t g = g0 + e0;
        int32_t v[4] = {0, 0, 0, 0};
        if (e0 >= 0 && (uint32_t)e0 + 4u <= total && g >= 0 && g + 4 <= gn) {
            const tp_i4 q = *reinterpret_cast<const tp_i4 *>(p0 + e0);
            v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
        } else {
TP_UNROLL
            for (int32_t t = 0; t < 4; t++)
                if (e0 + t >= 0 && (uint32_t)(e0 + t) < total && g + t >= 0 && g + t < gn) v[t] = p0[e0 + t];
        }
        const uint32_t e1 = e0 < 0 ? 0u : (uint32_t)e0;
        uint32_t f = e1 / nch, c = e1 - f * nch;
TP_UNROLL
        for (int32_t t = 0; t < 4; t++) {
            if (e0 + t < 0 || (uint32_t)(e0 + t) >= total) continue;
            tile[c * pitch + f] = v[t];
            wide |= (uint32_t)(v[t] > kTpNarrow) | (uint32_t)(v[t] < -kTpNarrow);
            if (++c == nch) c = 0, f++;
        }
    }
    return wide != 0u;
}

// the window's element: the int itself in the int64 form (a 32 x 32 -> 64 multiply-add)
template <class A>
struct TpWin {
    typedef A type;
};
template <>
struct TpWin<int64_t> {
    typedef int32_t type;
};

template <class A>
WVF_HD A tp_abs(A v) {
    return v < (A)0 ? -v : v;
}

// one phase's output at step u of a trip: window value j is w[(u + j) % 12]
template <class A, int Q, int U>
WVF_HD A tp_dot(const typename TpWin<A>::type (&w)[kTpUnroll]) {
    A y = (A)0;
TP_UNROLL
    for (int t = 0; t < (int)kTpTaps_n; t++) y += (A)kTpTaps[Q][t] * (A)w[(U + t) % (int)kTpUnroll];
    return y;
}

template <class A, int O, int U>
WVF_HD void tp_step(const typename TpWin<A>::type (&w)[kTpUnroll], uint32_t it, A thr, A sthr, A &peak, uint32_t &pos, uint32_t &overs, A &speak,
                    uint32_t &sframe) {
    const A m0 = tp_abs<A>((A)w[(U + (int)kTpBefore) % (int)kTpUnroll]);
    if (m0 > speak) speak = m0, sframe = it;
    overs += (uint32_t)(m0 > sthr);
    if constexpr (O == 4) {
        const A m = tp_abs<A>(tp_dot<A, 1, U>(w));
        if (m > peak) peak = m, pos = it * 4u + 1u;
        overs += (uint32_t)(m > thr);
    }
    if constexpr (O >= 2) {
        const A m = tp_abs<A>(tp_dot<A, 2, U>(w));
        if (m > peak) peak = m, pos = it * (uint32_t)O + (uint32_t)(O / 2);
        overs += (uint32_t)(m > thr);
    }
    if constexpr (O == 4) {
        const A m = tp_abs<A>(tp_dot<A, 3, U>(w));
        if (m > peak) peak = m, pos = it * 4u + 3u;
        overs += (uint32_t)(m > thr);
    }
}

// steps U .. 11 of one trip: frames it0 + U .. of the tile, the thread's own below `end`
template <class A, int O, int U>
WVF_HD void tp_trip(const int32_t (&win)[kTpUnroll], typename TpWin<A>::type (&w)[kTpUnroll], uint32_t it0,
                    uint32_t end, A thr, A sthr, A &peak, uint32_t &pos, uint32_t &overs, A &speak, uint32_t &sframe) {
    if constexpr (U < (int)kTpUnroll) {
        typedef typename TpWin<A>::type W;
        if constexpr (O > 1) w[(U + 11) % (int)kTpUnroll] = (W)win[U];
        else w[(U + (int)kTpBefore) % (int)kTpUnroll] = (W)win[U];
        if (it0 + (uint32_t)U < end) tp_step<A, O, U>(w, it0 + (uint32_t)U, thr, sthr, peak, pos, overs, speak, sframe);
        tp_trip<A, O, U + 1>(win, w, it0, end, thr, sthr, peak, pos, overs, speak, sframe);
    }
}

// thread tid's run of its row (threads past nch * tp_segments(nch) have none)
template <class A, int O>
WVF_HD TpAcc tp_scan_as(const TpJob &j, const int32_t *tile, uint32_t tid) {
    const uint32_t nch = j.nch, segs = tp_segments(nch), run = tp_run(nch), pitch = tp_pitch(nch);
    const uint32_t c = tid / segs, s = tid - c * segs, first = s * run;
    TpAcc a = tp_acc_none();
    if (c >= nch || first >= j.nvalid) return a;
    const uint32_t end = first + run < j.nvalid ? first + run : j.nvalid;
    // row word i holds frame i - 5 of the tile: frame it's window is words it .. it + 11
    const int32_t *row = tile + c * pitch;
    const A sthr = (A)((int64_t)1 << j.k), thr = sthr * (A)(1 << 24);
    typedef typename TpWin<A>::type W;
    W w[kTpUnroll];
TP_UNROLL
    for (uint32_t t = 0; t < kTpUnroll; t++) w[t] = (W)0;
    if constexpr (O > 1) {
TP_UNROLL
        for (uint32_t t = 0; t < kTpUnroll - 1u; t++) w[t] = (W)row[first + t];
    }
    // -1: below every magnitude, so the first step always takes the position
    A peak = (A)-1, speak = (A)-1;
    uint32_t pos = kTpNone, sframe = kTpNone, overs = 0;
    for (uint32_t it0 = first; it0 < end; it0 += kTpUnroll) {
        // the trip's twelve new words, in flight together before its first step (a discarded
        // step's word lies inside the array: kTpLdsInts)
        int32_t nx[kTpUnroll];
        TP_UNROLL
        for (uint32_t t = 0; t < kTpUnroll; t++) nx[t] = row[it0 + t + (O > 1 ? kTpUnroll - 1u : kTpBefore)];
        tp_trip<A, O, 0>(nx, w, it0, end, thr, sthr, peak, pos, overs, speak, sframe);
    }
    // phase 0 is the sample: its first maximum is the sample peak's frame
    a.speak = (uint32_t)(int64_t)speak;
    a.sframe = sframe;
    a.overs = overs;
    a.peak = (uint64_t)a.speak << 24;
    a.pos = sframe * (uint32_t)O;
    if constexpr (O > 1) {
        const uint64_t pk = (uint64_t)(int64_t)peak;
        if (pk > a.peak || (pk == a.peak && pos < a.pos)) a.peak = pk, a.pos = pos;
    }
    return a;
}

// `O`: 1, 2 or 4; `wide`: some int of the tile or its halo lies outside +-2^28.  Both are
// uniform for the workgroup
WVF_HD TpAcc tp_scan(const TpJob &j, const int32_t *tile, uint32_t tid, uint32_t O, bool wide) {
    if (O == 1u) return tp_scan_as<int64_t, 1>(j, tile, tid);
    if (wide) return O == 2u ? tp_scan_as<int64_t, 2>(j, tile, tid) : tp_scan_as<int64_t, 4>(j, tile, tid);
    return O == 2u ? tp_scan_as<double, 2>(j, tile, tid) : tp_scan_as<double, 4>(j, tile, tid);
}

// lanes of the butterfly inside a wave, and the waves whose results one channel then joins
WVF_HD uint32_t tp_tree_lanes(uint32_t nch) {
    const uint32_t s = tp_segments(nch);
    return s < kTpWave ? s : kTpWave;
}
WVF_HD uint32_t tp_row_waves(uint32_t nch) {
    const uint32_t s = tp_segments(nch);
    return s > kTpWave ? s / kTpWave : 1u;
}

// a row's total as the tile's record of that channel: positions become the file's
WVF_HD void tp_partial(const TpJob &j, const TpAcc &a, uint32_t O, TpRecord *out) {
    TpRecord r;
    r.true_peak = (int64_t)a.peak;
    r.true_peak_pos = a.pos == kTpNone ? -1 : (int64_t)(j.frame0 * O + a.pos);
    r.overs = a.overs;
    r.sample_peak = a.speak;
    r.sample_peak_frame = a.sframe == kTpNone ? -1 : (int64_t)(j.frame0 + a.sframe);
    r.oversample = (int32_t)O;
    r.k = (int32_t)j.k;
    *out = r;
}

// ---- combine ----
WVF_HD TpRecord tp_rec_none() {
    TpRecord r;
    r.true_peak = r.overs = r.sample_peak = 0;
    r.true_peak_pos = r.sample_peak_frame = -1;
    r.oversample = r.k = 0;
    return r;
}

// (-1 is the largest unsigned position: none)
WVF_HD TpRecord tp_rec_merge(const TpRecord a, const TpRecord b) {
    const int64_t ap = a.true_peak, bp = b.true_peak, as = a.sample_peak, bs = b.sample_peak;
    const uint64_t apos = (uint64_t)a.true_peak_pos, bpos = (uint64_t)b.true_peak_pos;
    const uint64_t af = (uint64_t)a.sample_peak_frame, bf = (uint64_t)b.sample_peak_frame;
    const bool tb = bp > ap || (bp == ap && bpos < apos);
    const bool sb = bs > as || (bs == as && bf < af);
    TpRecord r;
    r.true_peak = tb ? bp : ap;
    r.true_peak_pos = (int64_t)(tb ? bpos : apos);
    r.overs = a.overs + b.overs;
    r.sample_peak = sb ? bs : as;
    r.sample_peak_frame = (int64_t)(sb ? bf : af);
    r.oversample = r.k = 0;
    return r;
}

// lane `lane` of `nlanes`: its share of one channel's partials
WVF_HD TpRecord tp_fold(const TpFold &f, const TpRecord *partials, uint32_t lane, uint32_t nlanes) {
    TpRecord r = tp_rec_none();
    for (uint32_t t = lane; t < f.ntiles; t += nlanes) r = tp_rec_merge(r, partials[f.part + (uint64_t)t * f.nch]);
    return r;
}

WVF_HD void tp_final(const TpFold &f, TpRecord r, uint32_t oversample, TpRecord *out) {
    r.oversample = (int32_t)(oversample ? oversample : f.o_rate);
    r.k = (int32_t)f.k;
    *out = r;
}

}  // namespace wvg
