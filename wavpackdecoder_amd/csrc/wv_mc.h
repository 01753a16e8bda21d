// wv_mc.h -- the streams of a multichannel file woven into N-channel frames.
//
// A file opened with OPEN_ALL_CHANNELS decodes every stream (a mono or stereo block
// per block group) into a staging range of its own; after the decode kernels one job
// per (file, frame tile) weaves them into the file's visible range:
//   out[(frame0 + f) * nch + ch_s + c] = stream_s[(frame0 + f) * width_s + c]
// with zeros where a stream delivered fewer frames than the file.
//
// The tile code is compiled for the host and the device (WVF_HD): the kernel
// (wv_mc.hip) runs it with the tile in LDS and one call per thread, the host entry
// wvg_interleave_streams with the tile in memory and the thread index as a loop, so the
// CPU suite checks exactly the index code the GPU runs.
//   mc_gather: a stream's part of the tile is contiguous in its staging range; every
//              thread takes four consecutive ints (one 16-byte load where the source is
//              aligned and whole, which it always is on the device: staging ranges
//              start at a multiple of 4 ints and a tile at a multiple of 16 frames) and
//              writes them to tile[f * nch + ch + c].
//   mc_store:  the tile's nframes x nch ints are contiguous in the output, which may
//              start at any int: single ints up to the first 16-byte boundary, 16-byte
//              stores, single ints after the last whole one.
// Every offset into the batch output is 64-bit; offsets inside a tile fit 32 bits.
#pragma once
#include <stdint.h>

#include "wv_format.h"

namespace wvg {

constexpr uint32_t kMcTileInts = 4096;  // ints of one tile (16 KiB of LDS)
constexpr uint32_t kMcThreads = 256;    // threads of one workgroup
constexpr uint32_t kMcMaxChannels = 255;  // ID_CHANNEL_INFO's one-byte count

// frames of one tile of an nch-channel file (1 <= nch <= 255): a multiple of 16, so that
// every stream's part of every tile starts at a 16-byte boundary of its staging range
WVF_HD uint32_t mc_tile_frames(uint32_t nch) {
    const uint32_t t = (kMcTileInts / (nch ? nch : 1u)) & ~15u;
    return t ? t : 16u;
}

struct McStreamDev {
    uint64_t off;     // first int of the stream's staging range in the batch output
    uint64_t frames;  // frames it delivers (zeros from there on)
    uint32_t width;   // ints a frame: 1 or 2
    uint32_t ch;      // its first channel in the file's frames
};

struct McJob {
    uint64_t out_off;  // first int of the tile in the batch output (the file's visible range)
    uint64_t frame0;   // the tile's first frame
    uint32_t nframes;  // its frames (<= mc_tile_frames(nch))
    uint32_t nch;      // channels of the file
    uint32_t first_stream, nstreams;  // the file's streams in the stream table
};

typedef int32_t mc_i4 __attribute__((vector_size(16)));

// `src`: the stream's first int (frame 0)
WVF_HD void mc_gather(const McJob &j, const McStreamDev &st, const int32_t *src, int32_t *tile, uint32_t tid,
                      uint32_t nthreads) {
    const uint32_t w = st.width;
    const uint64_t have = st.frames > j.frame0 ? st.frames - j.frame0 : 0;
    const uint32_t nf = have < (uint64_t)j.nframes ? (uint32_t)have : j.nframes;
    const uint32_t n = nf * w, total = j.nframes * w;
    const int32_t *p = src + j.frame0 * (uint64_t)w;
    const bool aligned = ((uintptr_t)p & 15u) == 0;
    for (uint32_t i = tid * 4u; i < total; i += nthreads * 4u) {
        int32_t q0, q1, q2, q3;
        if (aligned && i + 4u <= n) {
            const mc_i4 v = *reinterpret_cast<const mc_i4 *>(p + i);
            q0 = v[0], q1 = v[1], q2 = v[2], q3 = v[3];
        } else {
            q0 = i < n ? p[i] : 0;
            q1 = i + 1u < n ? p[i + 1u] : 0;
            q2 = i + 2u < n ? p[i + 2u] : 0;
            q3 = i + 3u < n ? p[i + 3u] : 0;
        }
        // int k of the stream's part is channel (k % w) of frame (k / w)
        int32_t *t = tile + st.ch;
        if (w == 2u) {
            const uint32_t f = i >> 1;
            t[f * j.nch] = q0;
            t[f * j.nch + 1u] = q1;
            if (i + 2u < total) {
                t[(f + 1u) * j.nch] = q2;
                t[(f + 1u) * j.nch + 1u] = q3;
            }
        } else {
            t[i * j.nch] = q0;
            if (i + 1u < total) t[(i + 1u) * j.nch] = q1;
            if (i + 2u < total) t[(i + 2u) * j.nch] = q2;
            if (i + 3u < total) t[(i + 3u) * j.nch] = q3;
        }
    }
}

// `dst`: the tile's first int in the output
WVF_HD void mc_store(const McJob &j, const int32_t *tile, int32_t *dst, uint32_t tid, uint32_t nthreads) {
    const uint32_t total = j.nframes * j.nch;
    uint32_t head = (4u - (uint32_t)(((uintptr_t)dst >> 2) & 3u)) & 3u;
    if (head > total) head = total;
    const uint32_t body = (total - head) / 4u, tail0 = head + 4u * body;
    if (tid < head) dst[tid] = tile[tid];
    for (uint32_t q = tid; q < body; q += nthreads) {
        const uint32_t i = head + 4u * q;
        mc_i4 v;
        v[0] = tile[i];
        v[1] = tile[i + 1u];
        v[2] = tile[i + 2u];
        v[3] = tile[i + 3u];
        *reinterpret_cast<mc_i4 *>(dst + i) = v;
    }
    if (tid < total - tail0) dst[tail0 + tid] = tile[tail0 + tid];
}

}  // namespace wvg
