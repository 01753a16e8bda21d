// wv_loud.h -- integrated loudness of the decoded ints (wvg_batch_loudness): ITU-R BS.1770's
// K-weighting, 400 ms blocks every 100 ms and the two gates, in float64.
//
// After a decode a file's visible range holds out_frames x C interleaved int32.  Each
// channel runs through two biquads (the high shelf and the 38 Hz "RLB" high pass), the
// squares are summed over steps of S = (rate + 5) / 10 frames, four steps and the channel
// weights make a block power, and the blocks above the absolute and the relative gate make
// the file's power.  The definition is in include/wvgpu.h; this header is its code.
//
// Three passes, no atomics (nothing depends on scheduling):
//   runs:    one lane per (file, channel, run of kLdRunSteps steps) filters its frames and
//            writes the run's step energies E[channel][step].  The filter is recursive, so a
//            run does not continue the run before it: it starts up to kLdWarmSteps steps
//            early with all four states +0.0 and discards those steps' energies (overlap-
//            discard).  That restart is the definition, on the host as on the device; what
//            it leaves out of the never-restarted filter has decayed by the 38 Hz pole pair
//            over 0.3 s, about 2^-103.
//   blocks:  one thread per (file, block) sums four steps of every channel into P_j.
//   gate:    one wave per file, lanes striding over the blocks: count and sum above the
//            absolute gate, a butterfly, then the same above both gates.
//
// The code is compiled for the host and the device (WVF_HD).  The kernels (wv_loud.hip) call
// it once per thread, the host entry wvg_loudness_ints with the thread index as a loop, so
// the CPU suite checks the index and summation code the GPU runs, and the two agree bit for
// bit: every product-sum below is either an explicit fused multiply-add (ld_fma) or a
// separate multiply and add, and contraction is switched off so that neither compiler
// fuses or splits one.  No transcendental function is called here: the filter design (tan,
// pow) is host code in wv_api.cpp and only its seven doubles per rate arrive.
// Every offset into the batch output is 64-bit.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "wv_format.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#if defined(__clang__)
#define WV_LD_UNROLL _Pragma("unroll")
#else
#define WV_LD_UNROLL
#endif

namespace wvg {

#ifndef WV_LOUD_RUN_STEPS
#define WV_LOUD_RUN_STEPS 2
#endif
constexpr uint32_t kLdRunSteps = WV_LOUD_RUN_STEPS;  // R: steps of one run (measured: DESIGN.md §5)
static_assert(kLdRunSteps == 1 || kLdRunSteps == 2 || kLdRunSteps == 4, "R is 1, 2 or 4");
constexpr uint32_t kLdWarmSteps = 3;     // steps a run starts early, their energies discarded
constexpr uint32_t kLdBlockSteps = 4;    // steps of one block (400 ms)
constexpr uint32_t kLdChunk = 16;        // frames a lane has in flight while it filters the 16 before
constexpr uint32_t kLdRunThreads = 64;   // threads of one workgroup of the runs kernel (one wave)
constexpr uint32_t kLdBlockThreads = 256;
constexpr uint32_t kLdGateLanes = 64;    // threads of one workgroup (one wave) of the gate kernel
constexpr uint32_t kLdMaxChannels = 255;
constexpr uint32_t kLdCoefDoubles = 8;   // b0 b1 b2 a1 a2 c1 c2 and one unused, per rate
constexpr int64_t kLdMinRate = 6000, kLdMaxRate = 3072000;
constexpr double kLdAbsGate = 0x1.f791ec6e1d5b7p-24;  // the double nearest 10^((-70 + 0.691) / 10)

// one per measurable file
struct LdFile {
    uint64_t in_off;    // the file's first int in the batch output
    uint64_t e_off;     // its first step energy in the scratch image, [channel][step]
    uint64_t blk_off;   // its first P_j in the block image
    uint32_t nsteps;    // out_frames / S
    uint32_t nblocks;   // max(0, nsteps - 3)
    uint32_t S;         // frames of one step
    uint32_t nch;
    uint32_t k;         // full scale is 2^k (7, 15, 23, 31)
    uint32_t coef;      // index of its rate's coefficients, in units of kLdCoefDoubles
    uint64_t w_off;     // its first channel weight in the weight table
};

// one per (file, channel, run); files of fewer than four steps have none
struct LdRun {
    uint32_t file;      // index into the LdFile table
    uint32_t ch;
    uint32_t j0;        // first step of the run
    uint32_t nst;       // its steps (1 .. kLdRunSteps)
};

// wvg_file_loudness (include/wvgpu.h), field for field
struct LdRecord {
    double power, ungated_power, max_block_power;
    int64_t blocks, abs_blocks, gated_blocks;
    int64_t block_offset;
    int32_t step_frames;
    int32_t channels;
};

WVF_HD double ld_fma(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fma_rn(a, b, c);  // v_fma_f64
#else
    return fma(a, b, c);
#endif
}

// 2^-k as a double (k <= 31: a normal number), without a library call
WVF_HD double ld_scale(uint32_t k) {
    const uint64_t u = (uint64_t)(1023u - (k & 31u)) << 52;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// the channel weights: C <= 2 all 1; otherwise the channels take the mask's set bits in
// ascending order, LFE (bit 3) 0, the back and side pairs (bits 4, 5, 9, 10) 1.41, every
// other bit and every channel past the mask's bits 1
WVF_HD void ld_weights(uint32_t nch, uint32_t mask, double *w) {
    uint32_t bit = 0;
    for (uint32_t c = 0; c < nch; c++) {
        double g = 1.0;
        if (nch > 2u) {
            while (bit < 32u && !((mask >> bit) & 1u)) bit++;
            if (bit < 32u) {
                if (bit == 3u) g = 0.0;
                else if (bit == 4u || bit == 5u || bit == 9u || bit == 10u) g = 1.41;
                bit++;
            }
        }
        w[c] = g;
    }
}

struct LdState {
    double s1, s2, t1, t2, e;
};

// one sample through both biquads (transposed direct form II) and into the step's energy
WVF_HD void ld_sample(LdState &q, const double *cf, double x) {
    const double b0 = cf[0], b1 = cf[1], b2 = cf[2], a1 = cf[3], a2 = cf[4], c1 = cf[5], c2 = cf[6];
    const double y1 = ld_fma(b0, x, q.s1);
    q.s1 = ld_fma(-a1, y1, ld_fma(b1, x, q.s2));
    q.s2 = ld_fma(-a2, y1, b2 * x);
    const double y2 = y1 + q.t1;
    q.t1 = ld_fma(-c1, y2, ld_fma(-2.0, y1, q.t2));
    q.t2 = ld_fma(-c2, y2, y1);
    q.e = ld_fma(y2, y2, q.e);
}

// a run's position: frames done of the current step, steps done (warm-up steps included)
struct LdPos {
    uint32_t n, st;
};

// one frame of a run; a step's last frame writes the step's energy unless it is a warm-up step
WVF_HD void ld_frame(LdState &q, LdPos &at, const double *cf, double scale, int32_t v, uint32_t S, uint32_t warm,
                     double *eo) {
    ld_sample(q, cf, (double)v * scale);
    if (++at.n == S) {
        if (at.st >= warm) eo[at.st - warm] = q.e;
        q.e = 0.0;
        at.n = 0;
        at.st++;
    }
}

// One run.  `src`: the file's first int; `E`: the file's first step energy.  The lane reads
// frames [start * S, (j0 + nst) * S) of its channel, start = max(0, j0 - 3), and nothing else.
// The next kLdChunk values are loaded before the current ones are filtered: the stream is
// lane-private and strided, so a lane hides its own latency.  The last frames, fewer than
// two chunks, are read one by one.
WVF_HD void ld_run(const LdFile &f, const LdRun &r, const double *cf8, const int32_t *src, double *E) {
    const uint32_t warm = r.j0 < kLdWarmSteps ? r.j0 : kLdWarmSteps;
    const uint64_t C = f.nch;
    const uint64_t total = (uint64_t)(warm + r.nst) * f.S;
    const int32_t *p = src + (uint64_t)(r.j0 - warm) * f.S * C + r.ch;
    double *eo = E + (uint64_t)r.ch * f.nsteps + r.j0;
    double cf[7];
    for (int i = 0; i < 7; i++) cf[i] = cf8[i];
    const double scale = ld_scale(f.k);
    LdState q;
    q.s1 = q.s2 = q.t1 = q.t2 = q.e = 0.0;
    LdPos at;
    at.n = at.st = 0;
    uint64_t base = 0;
    if (total >= 2u * kLdChunk) {
        int32_t cur[kLdChunk], nxt[kLdChunk];
        WV_LD_UNROLL
        for (uint32_t i = 0; i < kLdChunk; i++) cur[i] = p[(uint64_t)i * C];
        for (; base + 2u * kLdChunk <= total; base += kLdChunk) {
            WV_LD_UNROLL
            for (uint32_t i = 0; i < kLdChunk; i++) nxt[i] = p[(base + kLdChunk + i) * C];
            WV_LD_UNROLL
            for (uint32_t i = 0; i < kLdChunk; i++) ld_frame(q, at, cf, scale, cur[i], f.S, warm, eo);
            WV_LD_UNROLL
            for (uint32_t i = 0; i < kLdChunk; i++) cur[i] = nxt[i];
        }
        WV_LD_UNROLL
        for (uint32_t i = 0; i < kLdChunk; i++) ld_frame(q, at, cf, scale, cur[i], f.S, warm, eo);
        base += kLdChunk;
    }
    for (; base < total; base++) ld_frame(q, at, cf, scale, p[base * C], f.S, warm, eo);
}

// the file that holds block `idx` of the image (idx < the image's doubles): the last file
// whose blk_off is <= idx; files of no blocks share their successor's offset and come before it
WVF_HD uint32_t ld_find_file(const LdFile *files, uint32_t nfiles, uint64_t idx) {
    uint32_t lo = 0, hi = nfiles;  // files[lo].blk_off <= idx < files[hi].blk_off
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (files[mid].blk_off <= idx) lo = mid;
        else hi = mid;
    }
    return lo;
}

// block j of a file: channels ascending
WVF_HD double ld_block(const LdFile &f, const double *E, const double *w, uint32_t j) {
    double acc = 0.0;
    for (uint32_t c = 0; c < f.nch; c++) {
        const double *e = E + (uint64_t)c * f.nsteps + j;
        acc = ld_fma(w[c], ((e[0] + e[1]) + e[2]) + e[3], acc);
    }
    return acc / (double)(4u * (uint64_t)f.S);
}

// ---- gate ----
struct LdGate {
    double sum;
    int64_t cnt;
    double mx;
};

// lane `lane` of `nlanes`: its share of the blocks above ABS (and above `rel`), j ascending
WVF_HD LdGate ld_gate_part(const double *P, uint64_t n, uint32_t lane, uint32_t nlanes, double rel) {
    LdGate g;
    g.sum = 0.0;
    g.cnt = 0;
    g.mx = 0.0;
    for (uint64_t j = lane; j < n; j += nlanes) {
        const double p = P[j];
        g.mx = p > g.mx ? p : g.mx;
        if (p > kLdAbsGate && p > rel) {
            g.sum = g.sum + p;
            g.cnt++;
        }
    }
    return g;
}

// (a + b == b + a: after a butterfly step lanes l and l ^ m hold the same bits)
WVF_HD LdGate ld_gate_merge(const LdGate &a, const LdGate &b) {
    LdGate r;
    r.sum = a.sum + b.sum;
    r.cnt = a.cnt + b.cnt;
    r.mx = b.mx > a.mx ? b.mx : a.mx;
    return r;
}

WVF_HD double ld_gate_mean(const LdGate &g) { return g.cnt ? g.sum / (double)g.cnt : 0.0; }

WVF_HD void ld_record(const LdFile *f, uint64_t n, const LdGate &ungated, const LdGate &gated, LdRecord *out) {
    LdRecord r;
    r.power = ld_gate_mean(gated);
    r.ungated_power = ld_gate_mean(ungated);
    r.max_block_power = ungated.mx;
    r.blocks = (int64_t)n;
    r.abs_blocks = ungated.cnt;
    r.gated_blocks = gated.cnt;
    r.block_offset = f ? (int64_t)f->blk_off : 0;
    r.step_frames = f ? (int32_t)f->S : 0;
    r.channels = f ? (int32_t)f->nch : 0;
    *out = r;
}

}  // namespace wvg

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
