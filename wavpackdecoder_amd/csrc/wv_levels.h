// wv_levels.h -- per-channel level statistics of the decoded ints (wvg_batch_levels).
//
// After a decode a file's visible range holds out_frames x C interleaved int32.  What a
// consumer computes next -- peak, DC, RMS, clip count, where the audio starts and ends --
// is a handful of reductions over each channel.  They are done here in integers, exactly:
// min, max, sum, the sum of squares as 128 bits, the samples on the rails, the samples
// above a silence threshold and the first and last frame that holds one.
//
// Two passes, no atomics (nothing depends on scheduling):
//   tiles:   one job per (file, frame tile) reduces its part of the range to one LvRecord
//            per channel, positions as frame indices of the file (`partials`);
//   combine: one wave per (file, channel) folds that channel's partials, lanes striding
//            over the tiles, and writes the final record.
//
// The code is compiled for the host and the device (WVF_HD): the kernels (wv_levels.hip)
// run it with the tile in LDS and one call per thread, the host entry wvg_levels_ints with
// the tile in memory and the thread index as a loop, so the CPU suite checks exactly the
// index, carry and position code the GPU runs.
//   lv_load:  the tile's nvalid x C ints are contiguous in the batch output, which may
//             start at any int: single ints up to the first 16-byte boundary, 16-byte
//             loads, single ints after the last whole one (pl_load's split), written to
//             the tile channels first.
//   lv_scan:  row c (one channel, nvalid values) is shared by S = lv_segments(C) threads,
//             thread c * S + s taking values s, s + S, s + 2S, ...: consecutive lanes read
//             consecutive words of the tile, and with S a power of two the S threads of a
//             row are one aligned lane group, so the tree that follows is a butterfly
//             (lane ^ m).  C * S <= 256: a 255-channel tile of 16 frames keeps the
//             workgroup as busy as a stereo one.
//   lv_merge: two accumulators into one; every field is an exact integer reduction, so the
//             order of the merges cannot change a result.
// The tile: row c starts at tile[c * pitch], pitch = lv_tile_frames(C) + 1 -- odd, so the
// rows that the lanes of one wave read at S < 64 (and with S = 1 one row a lane) start on
// different banks; the transpose happens on the write side, in ds_write_b32, as in
// wv_planar.h.
//
// Widths.  Inside a tile (at most 4,096 values) counts and positions fit 32 bits and the
// sum 64 (4,096 * 2^31 = 2^43).  The sum of squares does not fit 64 bits even there
// (v = INT32_MIN: v * v = 2^62, four of them are 2^64), so it is carried from the first
// add: lo += x; hi += lo < x.  One code path for every depth.
// Positions.  "None" is the all-ones pattern of first (the largest unsigned value: an
// unsigned min finds the first) and -1 of last (the smallest signed value: a signed max
// finds the last); no lane branches on whether it saw an active sample.
// Every offset into the batch output is 64-bit; offsets inside a tile fit 32 bits.
#pragma once
#include <stdint.h>

#include "wv_format.h"

namespace wvg {

constexpr uint32_t kLvTileInts = 4096;    // values of one tile (16 KiB)
constexpr uint32_t kLvThreads = 256;      // threads of one workgroup of the tile kernel
constexpr uint32_t kLvWave = 64;          // lanes of a wave: the widest butterfly
constexpr uint32_t kLvMaxChannels = 255;  // ID_CHANNEL_INFO's one-byte count
constexpr uint32_t kLvLdsInts = kLvTileInts + kLvMaxChannels;  // C * (lv_tile_frames(C) + 1) values at most
constexpr uint32_t kLvCombineLanes = 64;  // threads of one workgroup (one wave) of the combine kernel

// frames of one tile of an nch-channel file (1 <= nch <= 255): as pl_tile_frames
WVF_HD uint32_t lv_tile_frames(uint32_t nch) {
    const uint32_t t = (kLvTileInts / (nch ? nch : 1u)) & ~15u;
    return t ? t : 16u;
}

// threads that share one row of the tile: the largest power of two <= 256 / nch
WVF_HD uint32_t lv_segments(uint32_t nch) {
    uint32_t s = kLvThreads;
    while (s > 1u && s * nch > kLvThreads) s >>= 1;
    return s;
}

struct LvJob {
    uint64_t in_off;   // first int of the tile in the batch output
    uint64_t frame0;   // the file's frame index of the tile's first frame
    uint64_t part;     // index of the tile's channel-0 record in the partials
    uint32_t nvalid;   // frames of the tile (1 .. lv_tile_frames(nch))
    uint32_t nch;      // channels of the file
    uint32_t k;        // full scale is 2^k (7, 15, 23, 31)
    uint32_t pad_;
};

// one per (measurable file, channel): where its partials are
struct LvFold {
    uint64_t part;     // index of tile 0's record of this channel in the partials
    uint32_t ntiles;   // records to fold, `nch` records apart
    uint32_t nch;
};

// wvg_channel_levels (include/wvgpu.h), field for field
struct LvRecord {
    int32_t min, max;
    int64_t sum;
    uint64_t sumsq_lo, sumsq_hi;
    int64_t clipped, active, first_active, last_active;
};

typedef int32_t lv_i4 __attribute__((vector_size(16)));

// a thread's accumulator inside one tile
struct LvAcc {
    int32_t mn, mx;
    int64_t sum;
    uint64_t lo;
    uint32_t hi;
    uint32_t clipped, active;
    uint32_t first;  // index in the tile, 0xFFFFFFFF none
    int32_t last;    // index in the tile, -1 none
};

WVF_HD LvAcc lv_acc_none() {
    LvAcc a;
    a.mn = INT32_MAX;
    a.mx = INT32_MIN;
    a.sum = 0;
    a.lo = 0;
    a.hi = 0;
    a.clipped = a.active = 0;
    a.first = 0xFFFFFFFFu;
    a.last = -1;
    return a;
}

// the rails and the silence threshold of a depth: v >= rail or v <= -rail - 1 is clipped,
// v > thr or v < -thr is active.  Both fit int32 (k <= 31, threshold_q31 <= 0x7FFFFFFF), and
// so does -thr >= -INT32_MAX: no abs(v), INT32_MIN is a legal value
WVF_HD int32_t lv_rail(uint32_t k) { return (int32_t)((1u << (k & 31u)) - 1u); }
WVF_HD int32_t lv_threshold(uint32_t threshold_q31, uint32_t k) { return (int32_t)(threshold_q31 >> (31u - (k & 31u))); }

WVF_HD void lv_acc_add(LvAcc &a, int32_t v, uint32_t idx, int32_t rail, int32_t thr) {
    a.mn = v < a.mn ? v : a.mn;
    a.mx = v > a.mx ? v : a.mx;
    a.sum += v;
    const uint64_t x = (uint64_t)((int64_t)v * (int64_t)v);
    a.lo += x;
    a.hi += a.lo < x;
    a.clipped += (uint32_t)(v >= rail) | (uint32_t)(v <= -rail - 1);
    const uint32_t act = (uint32_t)(v > thr) | (uint32_t)(v < -thr);
    a.active += act;
    const uint32_t f = act ? idx : 0xFFFFFFFFu;
    const int32_t l = act ? (int32_t)idx : -1;
    a.first = f < a.first ? f : a.first;
    a.last = l > a.last ? l : a.last;
}

WVF_HD LvAcc lv_merge(const LvAcc &a, const LvAcc &b) {
    LvAcc r;
    r.mn = b.mn < a.mn ? b.mn : a.mn;
    r.mx = b.mx > a.mx ? b.mx : a.mx;
    r.sum = a.sum + b.sum;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (uint32_t)(r.lo < b.lo);
    r.clipped = a.clipped + b.clipped;
    r.active = a.active + b.active;
    r.first = b.first < a.first ? b.first : a.first;
    r.last = b.last > a.last ? b.last : a.last;
    return r;
}

// `src`: the tile's first int in the batch output
WVF_HD void lv_load(const LvJob &j, const int32_t *src, int32_t *tile, uint32_t tid, uint32_t nthreads) {
    const uint32_t nch = j.nch, pitch = lv_tile_frames(nch) + 1u, total = j.nvalid * nch;
    uint32_t head = (4u - (uint32_t)(((uintptr_t)src >> 2) & 3u)) & 3u;
    if (head > total) head = total;
    const uint32_t body = (total - head) / 4u, tail0 = head + 4u * body;
    // value k of the tile is channel k % nch of frame k / nch
    if (tid < head) {
        const uint32_t f = tid / nch, c = tid - f * nch;
        tile[c * pitch + f] = src[tid];
    }
    for (uint32_t q = tid; q < body; q += nthreads) {
        const uint32_t k = head + 4u * q;
        const lv_i4 v = *reinterpret_cast<const lv_i4 *>(src + k);
        uint32_t f = k / nch, c = k - f * nch;
        for (uint32_t i = 0; i < 4u; i++) {
            tile[c * pitch + f] = v[i];
            if (++c == nch) c = 0, f++;
        }
    }
    if (tid < total - tail0) {
        const uint32_t k = tail0 + tid, f = k / nch, c = k - f * nch;
        tile[c * pitch + f] = src[k];
    }
}

// thread tid's share of its row (threads past nch * lv_segments(nch) have none)
WVF_HD LvAcc lv_scan(const LvJob &j, const int32_t *tile, uint32_t tid, uint32_t threshold_q31) {
    const uint32_t nch = j.nch, pitch = lv_tile_frames(nch) + 1u, segs = lv_segments(nch);
    const uint32_t c = tid / segs, s = tid - c * segs;
    const int32_t rail = lv_rail(j.k), thr = lv_threshold(threshold_q31, j.k);
    LvAcc a = lv_acc_none();
    if (c < nch) {
        const int32_t *row = tile + c * pitch;
        uint32_t f = s;
        // four values a trip: their tile reads are in flight together (measured: DESIGN.md §5)
        for (; f + 3u * segs < j.nvalid; f += 4u * segs) {
            const int32_t v0 = row[f], v1 = row[f + segs], v2 = row[f + 2u * segs], v3 = row[f + 3u * segs];
            lv_acc_add(a, v0, f, rail, thr);
            lv_acc_add(a, v1, f + segs, rail, thr);
            lv_acc_add(a, v2, f + 2u * segs, rail, thr);
            lv_acc_add(a, v3, f + 3u * segs, rail, thr);
        }
        for (; f < j.nvalid; f += segs) lv_acc_add(a, row[f], f, rail, thr);
    }
    return a;
}

// lanes of the butterfly inside a wave, and the waves whose results one channel then joins
WVF_HD uint32_t lv_tree_lanes(uint32_t nch) {
    const uint32_t s = lv_segments(nch);
    return s < kLvWave ? s : kLvWave;
}
WVF_HD uint32_t lv_row_waves(uint32_t nch) {
    const uint32_t s = lv_segments(nch);
    return s > kLvWave ? s / kLvWave : 1u;
}

// a row's total as the tile's record of that channel: positions become the file's frames
WVF_HD void lv_partial(const LvJob &j, const LvAcc &a, LvRecord *out) {
    LvRecord r;
    r.min = a.mn;
    r.max = a.mx;
    r.sum = a.sum;
    r.sumsq_lo = a.lo;
    r.sumsq_hi = a.hi;
    r.clipped = a.clipped;
    r.active = a.active;
    r.first_active = a.first == 0xFFFFFFFFu ? -1 : (int64_t)(j.frame0 + a.first);
    r.last_active = a.last < 0 ? -1 : (int64_t)(j.frame0 + (uint32_t)a.last);
    *out = r;
}

// ---- combine ----
WVF_HD LvRecord lv_rec_none() {
    LvRecord r;
    r.min = INT32_MAX;
    r.max = INT32_MIN;
    r.sum = 0;
    r.sumsq_lo = r.sumsq_hi = 0;
    r.clipped = r.active = 0;
    r.first_active = r.last_active = -1;
    return r;
}

WVF_HD LvRecord lv_rec_merge(const LvRecord &a, const LvRecord &b) {
    LvRecord r;
    r.min = b.min < a.min ? b.min : a.min;
    r.max = b.max > a.max ? b.max : a.max;
    r.sum = (int64_t)((uint64_t)a.sum + (uint64_t)b.sum);
    r.sumsq_lo = a.sumsq_lo + b.sumsq_lo;
    r.sumsq_hi = a.sumsq_hi + b.sumsq_hi + (uint64_t)(r.sumsq_lo < b.sumsq_lo);
    r.clipped = a.clipped + b.clipped;
    r.active = a.active + b.active;
    // -1 is the largest unsigned value and the smallest signed one
    r.first_active = (uint64_t)b.first_active < (uint64_t)a.first_active ? b.first_active : a.first_active;
    r.last_active = b.last_active > a.last_active ? b.last_active : a.last_active;
    return r;
}

// lane `lane` of `nlanes`: its share of one channel's partials
WVF_HD LvRecord lv_fold(const LvFold &f, const LvRecord *partials, uint32_t lane, uint32_t nlanes) {
    LvRecord r = lv_rec_none();
    for (uint32_t t = lane; t < f.ntiles; t += nlanes) r = lv_rec_merge(r, partials[f.part + (uint64_t)t * f.nch]);
    return r;
}

// the final record: a file of no frames has no minimum
WVF_HD void lv_final(const LvFold &f, LvRecord r, LvRecord *out) {
    if (!f.ntiles) r.min = r.max = 0;
    *out = r;
}

}  // namespace wvg
