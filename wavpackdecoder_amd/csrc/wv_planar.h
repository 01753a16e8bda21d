// wv_planar.h -- the decoded ints as planar float32 (wvg_batch_planar).
//
// After a decode a file's visible range holds out_frames x C interleaved int32; a model,
// a resampler or any DSP on the same device wants float32 in [-1, 1), channels first.
// One job per (file, frame tile) reads its part of the range, converts, transposes
// through a tile and writes a segment of each of the file's C rows of the float image
// (the layout: include/wvgpu.h):
//   img[out_off + c * row_stride + f] = conv(in[in_off + f * C + c])   f < nvalid
//                                     = +0.0f                          nvalid <= f < nframes
//
// The tile code is compiled for the host and the device (WVF_HD): the kernel
// (wv_planar.hip) runs it with the tile in LDS and one call per thread, the host entry
// wvg_planar_float with the tile in memory and the thread index as a loop, so the CPU
// suite checks exactly the index and conversion code the GPU runs.
//   pl_load:  the tile's nvalid x C ints are contiguous in the batch output, which may
//             start at any int: single ints up to the first 16-byte boundary, 16-byte
//             loads, single ints after the last whole one (mc_store's split).  Every
//             value is converted as it arrives and written to the tile channels first.
//   pl_store: every row segment goes out with the same split -- single floats up to the
//             first 16-byte boundary of the image, 16-byte stores, single floats after
//             the last whole one -- with one work item per (row, 16-byte slot), so that a
//             255-channel tile of 16 frames keeps the workgroup as busy as a stereo one.
//
// The tile: row c starts at tile[c * pitch + skew_c], pitch = pl_tile_frames(C) + 4 and
//   skew_c = (the float index of the row segment's first float in memory) mod 4.
// Skew: a row segment starts at any float of the image (fixed-frames rows of odd length,
// a caller's buffer at any offset), so the 16-byte slots of the destination sit at a
// different phase in every row.  Starting each row at the phase of its destination makes
// every 16-byte store of the image one 16-byte aligned read of the tile (ds_read_b128; a
// misaligned one would split into single reads), the lanes of a wave reading consecutive
// slots of a row: no two lanes of a ds_read_b128 lane group share a bank.  Pad: the
// pitch is a multiple of 4 (it keeps that alignment from row to row) but 4 mod 16, never a
// multiple of 32, so the rows that the lanes of one 16-byte load scatter into (C rows,
// lane i at row (4i + j) mod C) do not all start on one bank.  The transpose happens on
// the write side, in ds_write_b32: for stereo lane i writes frame 2i + (j >> 1) of row
// j & 1, a stride of 2 dwords over the 32 banks a ds_write_b32 sees, and a 2-way store
// conflict costs no extra cycle there (the store's cycles are its register transfer).
// Reading an interleaved tile at a stride of C dwords instead would be an 8-way conflict
// for stereo (32 lanes on 4 banks).
// Every offset into the batch output or the image is 64-bit; offsets inside a tile fit
// 32 bits.
#pragma once
#include <stdint.h>
#include <string.h>

#include "wv_format.h"

namespace wvg {

constexpr uint32_t kPlTileInts = 4096;    // values of one tile (16 KiB)
constexpr uint32_t kPlThreads = 256;      // threads of one workgroup
constexpr uint32_t kPlMaxChannels = 255;  // ID_CHANNEL_INFO's one-byte count
// the tile with its rows' pad: C * (pl_tile_frames(C) + 4) <= 4096 + 4 * 255 values (20 KiB)
constexpr uint32_t kPlLdsInts = kPlTileInts + 4u * kPlMaxChannels + 4u;
constexpr uint32_t kPlBits = 0;  // PlJob::kind: the 32 bits pass through (exact float); else k of SCALE(k)

// frames of one tile of an nch-channel file (1 <= nch <= 255): a multiple of 16, as
// mc_tile_frames
WVF_HD uint32_t pl_tile_frames(uint32_t nch) {
    const uint32_t t = (kPlTileInts / (nch ? nch : 1u)) & ~15u;
    return t ? t : 16u;
}

struct PlJob {
    uint64_t in_off;      // first int of the tile in the batch output
    uint64_t out_off;     // first float of row 0's segment in the image
    uint64_t row_stride;  // floats from a row to the next
    uint32_t nframes;     // frames of the segment (<= pl_tile_frames(nch)), zeros from nvalid on
    uint32_t nvalid;      // frames read from the batch output (<= nframes)
    uint32_t nch;         // channels of the file
    uint32_t kind;        // kPlBits, or k: value * 2^-k (7, 15, 23, 31)
};

typedef int32_t pl_i4 __attribute__((vector_size(16)));
typedef uint32_t pl_u4 __attribute__((vector_size(16)));

// one value: the float's bit pattern
WVF_HD uint32_t pl_conv(int32_t v, uint32_t kind) {
    if (kind == kPlBits) return (uint32_t)v;
    // (float)v rounds to nearest even on both sides; 2^-k is exact and the product of a
    // float in [-2^31, 2^31] and 2^-k (k <= 31) is a normal number or zero: exact
    const uint32_t sb = (127u - kind) << 23;
    float s, r;
    memcpy(&s, &sb, 4);
#if defined(__HIP_DEVICE_COMPILE__)
    r = __int2float_rn(v) * s;
#else
    r = (float)v * s;
#endif
    uint32_t u;
    memcpy(&u, &r, 4);
    return u;
}

// the phase of row c's segment among the 16-byte slots of the image; dst: row 0's segment
WVF_HD uint32_t pl_skew(const PlJob &j, const float *dst, uint32_t c) {
    return ((uint32_t)((uintptr_t)dst >> 2) + c * (uint32_t)(j.row_stride & 3u)) & 3u;
}

// `src`: the tile's first int in the batch output; `dst`: row 0's segment in the image
WVF_HD void pl_load(const PlJob &j, const int32_t *src, const float *dst, uint32_t *tile, uint32_t tid,
                    uint32_t nthreads) {
    const uint32_t nch = j.nch, pitch = pl_tile_frames(nch) + 4u, total = j.nvalid * nch;
    uint32_t head = (4u - (uint32_t)(((uintptr_t)src >> 2) & 3u)) & 3u;
    if (head > total) head = total;
    const uint32_t body = (total - head) / 4u, tail0 = head + 4u * body;
    // value k of the tile is channel k % nch of frame k / nch
    if (tid < head) {
        const uint32_t f = tid / nch, c = tid - f * nch;
        tile[c * pitch + pl_skew(j, dst, c) + f] = pl_conv(src[tid], j.kind);
    }
    for (uint32_t q = tid; q < body; q += nthreads) {
        const uint32_t k = head + 4u * q;
        const pl_i4 v = *reinterpret_cast<const pl_i4 *>(src + k);
        uint32_t f = k / nch, c = k - f * nch;
        for (uint32_t i = 0; i < 4u; i++) {
            tile[c * pitch + pl_skew(j, dst, c) + f] = pl_conv(v[i], j.kind);
            if (++c == nch) c = 0, f++;
        }
    }
    if (tid < total - tail0) {
        const uint32_t k = tail0 + tid, f = k / nch, c = k - f * nch;
        tile[c * pitch + pl_skew(j, dst, c) + f] = pl_conv(src[k], j.kind);
    }
}

// `dst`: row 0's segment in the image
WVF_HD void pl_store(const PlJob &j, const uint32_t *tile, float *dst, uint32_t tid, uint32_t nthreads) {
    const uint32_t nch = j.nch, pitch = pl_tile_frames(nch) + 4u, nf = j.nframes;
    if (!nf) return;
    // slots a row: the 16-byte slots of the image that [skew, skew + nf) touches are
    // slots 0 .. (skew + nf - 1) / 4 counted from the one its first float lies in
    const uint32_t slots = (nf + 6u) / 4u, items = nch * slots;
    uint32_t *out = reinterpret_cast<uint32_t *>(dst);
    for (uint32_t w = tid; w < items; w += nthreads) {
        const uint32_t c = w / slots, q = w - c * slots, s = pl_skew(j, dst, c);
        const uint32_t lo = 4u * q;  // the slot is floats [lo - s, lo - s + 4) of the segment
        if (lo >= s + nf) continue;
        const uint32_t *t = tile + c * pitch + lo;
        uint64_t row = (uint64_t)c * j.row_stride;
        if (lo >= s && lo + 4u <= s + nf) {
            pl_u4 v = *reinterpret_cast<const pl_u4 *>(t);
            const uint32_t e = lo - s;
            if (e + 4u > j.nvalid)
                for (uint32_t i = 0; i < 4u; i++)
                    if (e + i >= j.nvalid) v[i] = 0u;
            *reinterpret_cast<pl_u4 *>(out + row + e) = v;
        } else {
            for (uint32_t i = 0; i < 4u; i++) {
                if (lo + i < s || lo + i >= s + nf) continue;
                const uint32_t e = lo + i - s;
                out[row + e] = e < j.nvalid ? t[i] : 0u;
            }
        }
    }
}

}  // namespace wvg
