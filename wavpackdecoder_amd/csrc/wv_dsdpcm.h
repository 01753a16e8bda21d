// wv_dsdpcm.h -- decoded DSD bytes decimated to 24-bit PCM (OPEN_DSD_AS_PCM).
//
// A DSD file opened with OPEN_DSD_AS_PCM decodes its blocks into a staging range (one int
// per channel-byte, as an unflagged file's output); after the decode kernels one job per
// (file, frame tile) filters the bytes into the file's visible range, one int32 per byte:
//   B[q][c] = stage[q * C + c] & 0xFF   0 <= q < F, else 0x55 (DSD's idle pattern)
//   y[m][c] = sum_{j = 0..12} sum_{i = 0..7} kDpTaps[8 j + i] * s_i(B[m - 6 + j][c])
//   s_i(b)  = +1 if (b >> (7 - i)) & 1 else -1        (bit 7 is the earliest in time)
// kDpTaps: 104 integer taps, 13 bytes centred on the output's byte -- the resampler's
// Hann-windowed sinc (lpw = 6, rolloff = 0.99) at ratio 8:1, scaled so that sum |c| <=
// 2^23 - 1 (include/wvgpu.h has the formula).  Every output therefore fits 24 bits and
// the int32 sum is exact in any order.
//
// One byte of one tap row is a table entry: kDpTables.t[j * 256 + b] = sum_i c[8j+i] s_i(b),
// so an output is 13 table lookups.  The tables (13 x 256 int32, 13,312 bytes) are built
// at compile time from the taps.
//
// The tile code is compiled for the host and the device (WVF_HD): the kernel
// (wv_dsdpcm.hip) runs it with the window and the tables in LDS and one call per thread,
// the host entry wvg_dsd_pcm_ints with both in memory and the thread index as a loop, so
// the CPU suite checks exactly the index code the GPU runs.
//   dp_load:  the tile and its 6-frame halo on each side, (nframes + 12) x C ints, are
//             contiguous in the staging range: they are read once, 16 bytes a work item
//             where the source is aligned and whole (on the device always: a staging range
//             starts at a multiple of 4 ints and a window word at a multiple of 4 ints of
//             the file), and their low bytes packed four to a window word, 0x55 for every
//             int outside the file.  The halo is part of that one read.
//   dp_store: the tile's nframes x C outputs are contiguous in the visible range, which
//             starts at any int: one work item per 16-byte slot of the destination (the
//             first and the last may be partial: single stores).  Value k of the tile
//             needs window bytes k + j * C, j = 0..12, so the four values of an item read
//             four consecutive bytes per j: two consecutive window words and a byte
//             shift.  Consecutive lanes read consecutive words (no bank conflict); the
//             table reads depend on the data (random over a 1 KiB table row: the bound of
//             this kernel).
// Window byte 0 is int g0 of the file, g0 = floor4((frame0 - 6) * C) - 4: a multiple of 4
// (aligned loads), and one word before the tile's first byte so that the partial first
// slot of the destination (values -3 .. -1 of the tile, never stored) reads inside it.
// Every offset into the batch output is 64-bit; offsets inside a tile fit 32 bits.
#pragma once
#include <stdint.h>

#include "wv_format.h"

namespace wvg {

constexpr uint32_t kDpTaps_n = 104;       // taps over bits
constexpr uint32_t kDpBytes = 13;         // bytes of history an output reads
constexpr uint32_t kDpHalo = 6;           // frames before and after the output's own
constexpr uint32_t kDpTileInts = 4096;    // outputs of one tile
constexpr uint32_t kDpThreads = 256;      // threads of one workgroup
constexpr uint32_t kDpMaxChannels = 255;  // ID_CHANNEL_INFO's one-byte count
constexpr uint32_t kDpIdle = 0x55;        // the byte outside the file
// the window: 4 + 3 bytes of lead, (tile + 12 frames) x C <= 4096 + 12 * 255 bytes, 3 values
// past the tile's last one, and the second word of the last read
constexpr uint32_t kDpWinWords = 1800;

constexpr int32_t kDpTaps[kDpTaps_n] = {
    0, 0, 0, 0, -13, -105, -320, -634,
    -945, -1083, -854, -102, 1223, 3016, 4986, 6681,
    7557, 7086, 4891, 882, -4653, -11010, -17117, -21672,
    -23363, -21125, -14413, -3418, 10815, 26405, 40817, 51191,
    54797, 49540, 34443, 10029, -21485, -56243, -89043, -113903,
    -124799, -116500, -85384, -30119, 47919, 144544, 253034, 364745,
    470019, 559255, 624028, 658079, 658079, 624028, 559255, 470019,
    364745, 253034, 144544, 47919, -30119, -85384, -116500, -124799,
    -113903, -89043, -56243, -21485, 10029, 34443, 49540, 54797,
    51191, 40817, 26405, 10815, -3418, -14413, -21125, -23363,
    -21672, -17117, -11010, -4653, 882, 4891, 7086, 7557,
    6681, 4986, 3016, 1223, -102, -854, -1083, -945,
    -634, -320, -105, -13, 0, 0, 0, 0,
};

struct DpTables {
    int32_t t[kDpBytes * 256];
};

constexpr DpTables dp_make_tables() {
    DpTables r = {};
    for (uint32_t j = 0; j < kDpBytes; j++)
        for (uint32_t b = 0; b < 256; b++) {
            int32_t s = 0;
            for (uint32_t i = 0; i < 8; i++) s += ((b >> (7u - i)) & 1u) ? kDpTaps[8u * j + i] : -kDpTaps[8u * j + i];
            r.t[j * 256u + b] = s;
        }
    return r;
}

// frames of one tile of an nch-channel file (1 <= nch <= 255): a multiple of 16, as
// mc_tile_frames
WVF_HD uint32_t dp_tile_frames(uint32_t nch) {
    const uint32_t t = (kDpTileInts / (nch ? nch : 1u)) & ~15u;
    return t ? t : 16u;
}

struct DpJob {
    uint64_t in_off;   // the file's staging range in the batch output (frame 0; a multiple of 4 ints)
    uint64_t out_off;  // the tile's first int in the batch output (the file's visible range)
    uint64_t frames;   // frames of the file (0x55 outside them)
    uint64_t frame0;   // the tile's first frame
    uint32_t nframes;  // its frames (<= dp_tile_frames(nch))
    uint32_t nch;      // ints a frame
};

typedef int32_t dp_i4 __attribute__((vector_size(16)));

// the file's int that window byte 0 holds (it may lie before the file)
WVF_HD int64_t dp_win_g0(const DpJob &j) {
    const int64_t first = ((int64_t)j.frame0 - (int64_t)kDpHalo) * (int64_t)j.nch;
    return (first & ~(int64_t)3) - 4;
}
// the window byte of the tile's value 0 at tap row 0 (4 .. 7)
WVF_HD uint32_t dp_win_lead(const DpJob &j) {
    const int64_t first = ((int64_t)j.frame0 - (int64_t)kDpHalo) * (int64_t)j.nch;
    return (uint32_t)(first - dp_win_g0(j));
}
// words of the window that dp_store reads (<= kDpWinWords)
WVF_HD uint32_t dp_win_words(const DpJob &j) {
    const uint32_t last = dp_win_lead(j) + j.nframes * j.nch + 2u + (kDpBytes - 1u) * j.nch;
    return (last >> 2) + 2u;
}

// `src`: the file's first int (frame 0) in its staging range
WVF_HD void dp_load(const DpJob &j, const int32_t *src, uint32_t *win, uint32_t tid, uint32_t nthreads) {
    const int64_t total = (int64_t)j.frames * (int64_t)j.nch, g0 = dp_win_g0(j);
    const uint32_t nwords = dp_win_words(j);
    const bool aligned = ((uintptr_t)src & 15u) == 0;  // (g0 is a multiple of 4 ints)
    for (uint32_t w = tid; w < nwords; w += nthreads) {
        const int64_t g = g0 + 4 * (int64_t)w;
        uint32_t b0 = kDpIdle, b1 = kDpIdle, b2 = kDpIdle, b3 = kDpIdle;
        if (g >= 0 && g + 4 <= total) {
            if (aligned) {
                const dp_i4 v = *reinterpret_cast<const dp_i4 *>(src + g);
                b0 = (uint32_t)v[0], b1 = (uint32_t)v[1], b2 = (uint32_t)v[2], b3 = (uint32_t)v[3];
            } else {
                b0 = (uint32_t)src[g], b1 = (uint32_t)src[g + 1], b2 = (uint32_t)src[g + 2], b3 = (uint32_t)src[g + 3];
            }
        } else {
            if (g >= 0 && g < total) b0 = (uint32_t)src[g];
            if (g + 1 >= 0 && g + 1 < total) b1 = (uint32_t)src[g + 1];
            if (g + 2 >= 0 && g + 2 < total) b2 = (uint32_t)src[g + 2];
            if (g + 3 >= 0 && g + 3 < total) b3 = (uint32_t)src[g + 3];
        }
        win[w] = (b0 & 255u) | ((b1 & 255u) << 8) | ((b2 & 255u) << 16) | (b3 << 24);
    }
}

// `tab`: kDpTables.t; `dst`: the tile's first int in the visible range
WVF_HD void dp_store(const DpJob &j, const uint32_t *win, const int32_t *tab, int32_t *dst, uint32_t tid,
                     uint32_t nthreads) {
    const uint32_t nch = j.nch, total = j.nframes * nch, lead = dp_win_lead(j);
    uint32_t head = (4u - (uint32_t)(((uintptr_t)dst >> 2) & 3u)) & 3u;
    if (head > total) head = total;
    // item 0: the values before the first 16-byte boundary (none when head == 0); item i >= 1:
    // values head + 4 (i - 1) .. + 3, the last one cut at the tile's end
    const uint32_t nitems = 1u + (total - head + 3u) / 4u;
    for (uint32_t i = tid; i < nitems; i += nthreads) {
        const int32_t k0 = (int32_t)head + 4 * ((int32_t)i - 1);  // >= -4
        if (k0 + 4 <= 0) continue;
        uint32_t o = (uint32_t)((int32_t)lead + k0);  // window byte of value k0 at tap row 0 (lead >= 4)
        int32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (uint32_t r = 0; r < kDpBytes; r++, o += nch) {
            const uint32_t lo = win[o >> 2], hi = win[(o >> 2) + 1u];
            const uint32_t b = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (o & 3u)));
            const int32_t *t = tab + r * 256u;
            a0 += t[b & 255u];
            a1 += t[(b >> 8) & 255u];
            a2 += t[(b >> 16) & 255u];
            a3 += t[b >> 24];
        }
        if (k0 >= 0 && (uint32_t)k0 + 4u <= total) {
            dp_i4 v;
            v[0] = a0, v[1] = a1, v[2] = a2, v[3] = a3;
            *reinterpret_cast<dp_i4 *>(dst + k0) = v;
        } else {
            if (k0 >= 0 && (uint32_t)k0 < total) dst[k0] = a0;
            if (k0 + 1 >= 0 && (uint32_t)(k0 + 1) < total) dst[k0 + 1] = a1;
            if (k0 + 2 >= 0 && (uint32_t)(k0 + 2) < total) dst[k0 + 2] = a2;
            if (k0 + 3 >= 0 && (uint32_t)(k0 + 3) < total) dst[k0 + 3] = a3;
        }
    }
}

}  // namespace wvg
