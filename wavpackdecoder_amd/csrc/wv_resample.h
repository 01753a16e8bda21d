// wv_resample.h -- the decoded ints as planar float32 at one sample rate (wvg_batch_resample).
//
// planar's twin (wv_planar.h): every resamplable file of a decoded batch is converted to
// float32 by pl_conv and brought from its own rate to the caller's by a polyphase FIR, the
// Hann-windowed sinc of include/wvgpu.h.  With in_rate : out_rate = orig : new in lowest
// terms, output frame n = i * new + p (block i, phase p) of channel c is the chain
//   acc_0 = +0.0f, acc_{j+1} = fmaf(h[p][j], x[c][i * orig + j - width], acc_j), j = 0 .. K-1
// over the file's converted frames x (+0.0f outside the file): one accumulator, one order.
//
// One job is one tile of `nb` blocks (nb * new output frames) of `cg` channels of one file.
// The tile code is compiled for the host and the device (WVF_HD), as planar's: the kernel
// (wv_resample.hip) runs it with the tile in LDS, the host entry wvg_resample_float with the
// tile in memory and the thread index as a loop.
//   rs_load:  the input window, frames [i0 * orig - width, (i0 + nb - 1) * orig + K - width),
//             cut to the file, is one contiguous run of ints in the batch output: single ints
//             up to the first 16-byte boundary, 16-byte loads, single ints after the last
//             whole one (planar's split).  Every value is converted once as it arrives and
//             written channels first, row c at xw[c * xpitch]; the frames of the window that
//             lie outside the file are +0.0f.  A job of a channel group (cg < nch: the
//             window of all channels does not fit) reads the whole frames and keeps its own.
//   rs_fir:   one work item per (channel, group of R blocks, pair of phases), phases
//             fastest: the lanes of a wave read consecutive dwords of the transposed table
//             tab[j][p] (8 bytes a lane: coalesced) and, where they share the block, one
//             address of the window (an LDS broadcast).  An item keeps 2 x R accumulators:
//             per tap 1 table load and R window reads feed 2 * R FMAs, so the loop is not
//             bound by one LDS read per FMA.  The R blocks of an item lie G = ceil(nb / R)
//             apart, so that for few phases neighbouring lanes read the window at a stride
//             of orig dwords and not of R * orig.  Each output's own chain runs j ascending
//             in one accumulator; blocking only interleaves independent chains.
//   rs_store: the outputs pass through a tile whose rows start at the phase of their
//             destination among the image's 16-byte slots (planar's skew), and leave as
//             16-byte stores with single floats at the unaligned ends and +0.0f from the
//             file's last output frame on.
// A file whose rate is the caller's has no filter: its jobs are planar's (new_ == 0) and
// run pl_load / pl_store in the same launch.
// Every offset into the batch output or the image is 64-bit; offsets inside a tile fit 32.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "wv_planar.h"

namespace wvg {

constexpr uint32_t kRsThreads = 256;   // threads of one workgroup
constexpr uint32_t kRsXFloats = 8192;  // the input window (32 KiB)
constexpr uint32_t kRsYFloats = 5120;  // the output tile with its rows' pad (20 KiB) >= kPlLdsInts
constexpr uint32_t kRsLdsFloats = kRsXFloats + kRsYFloats;
constexpr uint32_t kRsBlocks = 4;      // R: blocks of one work item
constexpr uint32_t kRsMaxRatio = 1024; // orig, new
constexpr uint32_t kRsMaxTaps = 4096;  // K
// a tile row beyond its nb * new floats: up to 3 of round-up, the skew's 3, and the 16-byte
// read of the row's last slot, which may reach 2 floats past them
constexpr uint32_t kRsYPad = 12;
static_assert(kRsYFloats >= kPlLdsInts, "a same-rate job runs planar's tile code in the output tile");
static_assert(kRsMaxTaps <= kRsXFloats && kRsMaxRatio + kRsYPad <= kRsYFloats, "one block of one channel fits");

struct RsJob {
    uint64_t in_off;      // the file's first int in the batch output (new_ == 0: the tile's, as PlJob)
    uint64_t out_off;     // first float of the job's first row segment in the image
    uint64_t row_stride;  // floats from a row to the next
    uint64_t frames;      // F: the file's input frames
    int64_t win0;         // first input frame of the window (i0 * orig - width; may be negative)
    const float *tab;     // the transposed table: tab[j * npad + p], npad = (new + 1) & ~1, pad +0.0f
    uint32_t orig, new_;  // the reduced rates; new_ == 0: a same-rate job (planar's)
    uint32_t taps;        // K
    uint32_t nb;          // blocks computed (ceil(nvalid / new))
    uint32_t nframes;     // frames of the segment, zeros from nvalid on
    uint32_t nvalid;      // frames computed (<= nframes)
    uint32_t nch;         // channels of the file
    uint32_t c0, cg;      // the job's channels [c0, c0 + cg)
    uint32_t kind;        // k of SCALE(k): 7, 15, 23, 31 (kPlBits in a same-rate job only)
};

// the tile of an nch-channel file: blocks a job (nb) and channels a job (cg)
struct RsGeom {
    uint32_t nb, cg;
};

// the most blocks a job of cg channels can have: the windows (nb - 1) * orig + K and the
// tile rows nb * new + kRsYPad of its channels fit
WVF_HD uint32_t rs_fit(uint32_t orig, uint32_t new_, uint32_t taps, uint32_t cg) {
    const uint32_t xc = kRsXFloats / cg, yc = kRsYFloats / cg;
    const uint32_t nb = xc >= taps ? (xc - taps) / orig + 1u : 0u;
    const uint32_t ny = yc > kRsYPad ? (yc - kRsYPad) / new_ : 0u;
    return ny < nb ? ny : nb;
}

// the share (in 1/1024) of the FIR's lane slots that hold a work item: the items fill whole
// rounds of kRsThreads
WVF_HD uint32_t rs_fill(uint32_t new_, uint32_t nb, uint32_t cg) {
    const uint32_t items = cg * ((nb + kRsBlocks - 1u) / kRsBlocks) * ((new_ + 1u) / 2u);
    return items * 1024u / ((items + kRsThreads - 1u) / kRsThreads * kRsThreads);
}

WVF_HD RsGeom rs_geom(uint32_t orig, uint32_t new_, uint32_t taps, uint32_t nch) {
    // all channels in one job while that leaves 2 * R blocks (or all that one channel could
    // have); else 2 * R blocks of as many channels as fit
    const uint32_t nb1 = rs_fit(orig, new_, taps, 1u), nbc = rs_fit(orig, new_, taps, nch);
    const uint32_t want = nb1 < 2u * kRsBlocks ? nb1 : 2u * kRsBlocks;
    RsGeom g;
    if (nbc >= want) {
        g.nb = nbc;
        g.cg = nch;
    } else {
        g.nb = want;
        g.cg = nch;
        while (rs_fit(orig, new_, taps, g.cg) < want) g.cg--;
    }
    if (g.nb >= kRsBlocks) g.nb -= g.nb % kRsBlocks;  // whole items
    // a long filter's work is its FMAs, not its loads: a job of fewer channels (it reads the
    // whole frames and keeps its own) or fewer blocks is worth it when it fills the lanes
    // of its rounds better by a tenth
    if (taps >= 64u && nch <= 8u && g.nb >= kRsBlocks) {
        uint32_t best = rs_fill(new_, g.nb, g.cg);
        const RsGeom g0 = g;
        for (uint32_t cg = g0.cg; cg >= 1u; cg--) {
            uint32_t nb = rs_fit(orig, new_, taps, cg);
            nb -= nb % kRsBlocks;
            for (uint32_t n = 0; n < 16u && nb >= kRsBlocks; n++, nb -= kRsBlocks) {
                const uint32_t f = rs_fill(new_, nb, cg);
                if (f > best + 102u) {
                    best = f;
                    g.nb = nb;
                    g.cg = cg;
                }
            }
        }
    }
    return g;
}

// floats of a window row, of a tile row
WVF_HD uint32_t rs_xpitch(const RsJob &j) { return (j.nb - 1u) * j.orig + j.taps; }
WVF_HD uint32_t rs_ypitch(const RsJob &j) { return ((j.nb * j.new_ + 3u) & ~3u) + 8u; }

// the phase of row c's segment (c from c0) among the 16-byte slots of the image
WVF_HD uint32_t rs_skew(const RsJob &j, const float *dst, uint32_t c) {
    return ((uint32_t)((uintptr_t)dst >> 2) + c * (uint32_t)(j.row_stride & 3u)) & 3u;
}

// `src`: the file's first int in the batch output; xw: the window, cg rows of rs_xpitch floats
WVF_HD void rs_load(const RsJob &j, const int32_t *src, uint32_t *xw, uint32_t tid, uint32_t nthreads) {
    const uint32_t nch = j.nch, xp = rs_xpitch(j);
    // the window's frames inside the file: [a, b)
    const int64_t wend = j.win0 + (int64_t)xp;
    const uint64_t a = j.win0 > 0 ? (uint64_t)j.win0 : 0u;
    uint64_t b = wend > 0 ? (uint64_t)wend : 0u;
    if (b > j.frames) b = j.frames;
    const uint32_t lo = (uint32_t)((int64_t)a - j.win0);  // a's place in a window row
    const uint32_t nin = b > a ? (uint32_t)(b - a) : 0u;
    // zeros before and after the file
    for (uint32_t w = tid; w < j.cg * xp; w += nthreads) {
        const uint32_t e = w % xp;
        if (e < lo || e >= lo + nin) xw[w] = 0u;
    }
    if (!nin) return;
    src += a * nch;
    const uint32_t total = nin * nch;
    uint32_t head = (4u - (uint32_t)(((uintptr_t)src >> 2) & 3u)) & 3u;
    if (head > total) head = total;
    const uint32_t body = (total - head) / 4u, tail0 = head + 4u * body;
    // value k of the run is channel k % nch of frame a + k / nch
    if (tid < head) {
        const uint32_t f = tid / nch, c = tid - f * nch - j.c0;
        if (c < j.cg) xw[c * xp + lo + f] = pl_conv(src[tid], j.kind);
    }
    for (uint32_t q = tid; q < body; q += nthreads) {
        const uint32_t k = head + 4u * q;
        const pl_i4 v = *reinterpret_cast<const pl_i4 *>(src + k);
        uint32_t f = k / nch, c = k - f * nch;
        for (uint32_t i = 0; i < 4u; i++) {
            if (c - j.c0 < j.cg) xw[(c - j.c0) * xp + lo + f] = pl_conv(v[i], j.kind);
            if (++c == nch) c = 0, f++;
        }
    }
    if (tid < total - tail0) {
        const uint32_t k = tail0 + tid, f = k / nch, c = k - f * nch - j.c0;
        if (c < j.cg) xw[c * xp + lo + f] = pl_conv(src[k], j.kind);
    }
}

typedef float rs_f2 __attribute__((vector_size(8)));

WVF_HD float rs_fma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);  // v_fma_f32
#else
    return fmaf(a, b, c);
#endif
}

WVF_HD uint32_t rs_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// xw: the loaded window; yt: the output tile, cg rows of rs_ypitch floats; `dst`: the job's
// first row segment in the image (the rows' skew)
WVF_HD void rs_fir(const RsJob &j, const uint32_t *xw, uint32_t *yt, const float *dst, uint32_t tid,
                   uint32_t nthreads) {
    constexpr uint32_t R = kRsBlocks;
    const uint32_t xp = rs_xpitch(j), yp = rs_ypitch(j), orig = j.orig, new_ = j.new_, taps = j.taps;
    const uint32_t npad = (new_ + 1u) & ~1u, npair = npad / 2u, G = (j.nb + R - 1u) / R;
    const uint32_t items = j.cg * G * npair;
    const float *xf = reinterpret_cast<const float *>(xw);
    for (uint32_t w = tid; w < items; w += nthreads) {
        const uint32_t pq = w % npair, rest = w / npair, ig = rest % G, c = rest / G;
        // a block past the job's last repeats it (computed, not kept)
        uint32_t ib[R];
        const float *x[R];
        for (uint32_t r = 0; r < R; r++) {
            ib[r] = ig + r * G;
            const uint32_t bb = ib[r] < j.nb ? ib[r] : j.nb - 1u;
            x[r] = xf + c * xp + bb * orig;
        }
        const float *h = j.tab + 2u * pq;
        float a0[R], a1[R];
        for (uint32_t r = 0; r < R; r++) a0[r] = a1[r] = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
        for (uint32_t t = 0; t < taps; t++) {
            const rs_f2 hv = *reinterpret_cast<const rs_f2 *>(h + t * npad);  // (8-byte aligned: npad is even)
            const float h0 = hv[0], h1 = hv[1];
            for (uint32_t r = 0; r < R; r++) {
                const float xv = x[r][t];
                a0[r] = rs_fma(h0, xv, a0[r]);
                a1[r] = rs_fma(h1, xv, a1[r]);
            }
        }
        uint32_t *y = yt + c * yp + rs_skew(j, dst, c) + 2u * pq;
        for (uint32_t r = 0; r < R; r++) {
            if (ib[r] >= j.nb) continue;
            y[ib[r] * new_] = rs_bits(a0[r]);
            if (2u * pq + 1u < new_) y[ib[r] * new_ + 1u] = rs_bits(a1[r]);
        }
    }
}

// `dst`: the job's first row segment in the image (pl_store with the job's own pitch)
WVF_HD void rs_store(const RsJob &j, const uint32_t *yt, float *dst, uint32_t tid, uint32_t nthreads) {
    const uint32_t yp = rs_ypitch(j), nf = j.nframes;
    if (!nf) return;
    const uint32_t slots = (nf + 6u) / 4u, items = j.cg * slots;
    uint32_t *out = reinterpret_cast<uint32_t *>(dst);
    for (uint32_t w = tid; w < items; w += nthreads) {
        const uint32_t c = w / slots, q = w - c * slots, s = rs_skew(j, dst, c);
        const uint32_t lo = 4u * q;  // the slot is floats [lo - s, lo - s + 4) of the segment
        if (lo >= s + nf) continue;
        const uint32_t *t = yt + c * yp + lo;
        const uint64_t row = (uint64_t)c * j.row_stride;
        if (lo >= s && lo + 4u <= s + nf) {
            const uint32_t e = lo - s;
            pl_u4 v = {0u, 0u, 0u, 0u};
            if (e < j.nvalid) {  // (a tile past the file's frames is never read)
                v = *reinterpret_cast<const pl_u4 *>(t);
                if (e + 4u > j.nvalid)
                    for (uint32_t i = 0; i < 4u; i++)
                        if (e + i >= j.nvalid) v[i] = 0u;
            }
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

// a same-rate job as planar's
WVF_HD PlJob rs_planar_job(const RsJob &j) {
    PlJob p;
    p.in_off = j.in_off;
    p.out_off = j.out_off;
    p.row_stride = j.row_stride;
    p.nframes = j.nframes;
    p.nvalid = j.nvalid;
    p.nch = j.nch;
    p.kind = j.kind;
    return p;
}

}  // namespace wvg
