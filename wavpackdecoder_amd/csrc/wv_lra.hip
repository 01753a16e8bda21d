// wv_lra.hip -- loudness range and short-term loudness of the decoded batch (gfx950): see
// wv_lra.h for the window, gate and selection code.
//
// wv_lra_short: one thread per ST_j of the short-term image; the file is found by bisection
// over the files' short offsets.  Neighbouring threads read neighbouring step energies, thirty
// loads per channel from an image that wvg_batch_loudness has just written (L2).
//
// wv_lra_gate: one wave per file, wv_loud_gate's arrangement with the factor 0.01: the
// counts, the mean and the maximum into the record, the relative gate beside it.
//
// wv_lra_select: one workgroup of 256 threads per file, both order statistics by a radix
// select over the doubles' bit patterns (wv_lra.h).  A thread keeps its first kLrHeld values
// in registers over the eight passes, already gated; a file of more than 1,024 values reads
// the rest again in every pass.  The 256-bin histograms are in LDS and take integer adds
// only, one per value: short-term powers of one file share their top bytes, so in the first
// passes nearly every add goes to one bin, and measured that costs nothing a per-wave
// aggregation would win back.  Waves 0 and 1 walk the two ranks' histograms side
// by side, four bins a lane and a scan over the lanes.  While both ranks share their known
// bytes one histogram serves both.  No float atomics, no scratch image.
#include <hip/hip_runtime.h>

#include "wv_lra.h"

namespace wvg {

__device__ __forceinline__ uint64_t lr_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ double lr_xord(double v, int m) {
    return __longlong_as_double((long long)lr_xor64((uint64_t)__double_as_longlong(v), m));
}

// lane ^ m's accumulator
__device__ __forceinline__ LdGate lr_gate_xchg(const LdGate &a, int m) {
    LdGate r;
    r.sum = lr_xord(a.sum, m);
    r.cnt = (int64_t)lr_xor64((uint64_t)a.cnt, m);
    r.mx = lr_xord(a.mx, m);
    return r;
}

__global__ void __launch_bounds__(kLrShortThreads) wv_lra_short(const LdFile *__restrict__ files,
                                                                const LrFile *__restrict__ lr, uint32_t nfiles,
                                                                uint64_t nshorts, const double *__restrict__ weights,
                                                                const double *__restrict__ E,
                                                                double *__restrict__ ST) {
    const uint64_t idx = (uint64_t)blockIdx.x * kLrShortThreads + threadIdx.x;
    if (idx >= nshorts) return;
    const uint32_t fi = lr_find_file(lr, nfiles, idx);
    const LdFile f = files[fi];
    ST[idx] = lr_short(f, E + f.e_off, weights + f.w_off, (uint32_t)(idx - lr[fi].st_off));
}

__global__ void __launch_bounds__(kLdGateLanes) wv_lra_gate(const LrFile *__restrict__ lr,
                                                            const double *__restrict__ ST, double *__restrict__ rel,
                                                            LrRecord *__restrict__ out) {
    const LrFile f = lr[blockIdx.x];
    const double *p = ST + f.st_off;
    LdGate u = ld_gate_part(p, f.nshort, threadIdx.x, kLdGateLanes, 0.0);
#pragma unroll
    for (int m = (int)kLdGateLanes / 2; m; m >>= 1) u = ld_gate_merge(u, lr_gate_xchg(u, m));
    const double r = lr_rel(u);
    LdGate g = ld_gate_part(p, f.nshort, threadIdx.x, kLdGateLanes, r);
#pragma unroll
    for (int m = (int)kLdGateLanes / 2; m; m >>= 1) g = ld_gate_merge(g, lr_gate_xchg(g, m));
    if (threadIdx.x == 0) {
        lr_record(&f, f.nshort, u, g, out + blockIdx.x);
        rel[blockIdx.x] = r;
    }
}

constexpr uint64_t kLrNone = ~0ull;  // no value: the pattern of no ST_j (their sign bit is clear)

// one value into `hist`: an integer LDS add (ds_add_u32).  Adding a wave's count once when all
// its takers hold one digit (a ballot) was measured and is not kept: DESIGN.md §5.
__device__ __forceinline__ void lr_count(uint32_t *hist, bool take, uint32_t d) {
    if (take) atomicAdd(&hist[d], 1u);
}

__device__ __forceinline__ void lr_count_both(uint32_t (*hist)[kLrBins], uint64_t u, const LrRank &lo, const LrRank &hi,
                                              bool same, uint32_t pass) {
    const bool valid = u != kLrNone;
    const uint32_t d = lr_digit(u, pass);
    lr_count(hist[0], valid && lr_candidate(u, lo, pass), d);
    if (!same) lr_count(hist[1], valid && lr_candidate(u, hi, pass), d);
}

__global__ void __launch_bounds__(kLrSelectThreads) wv_lra_select(const LrFile *__restrict__ lr,
                                                                  const double *__restrict__ ST,
                                                                  const double *__restrict__ rel, LrRecord *out) {
    static_assert(kLrSelectThreads == kLrBins, "a thread clears one bin of each histogram");
    static_assert(kLrSelectThreads >= 2 * kLrWalkLanes && kLrWalkLanes == 64, "two whole waves walk");
    __shared__ uint32_t hist[2][kLrBins];
    __shared__ LrRank found[2];
    const LrFile f = lr[blockIdx.x];
    LrRecord *rec = out + blockIdx.x;
    const uint64_t n = (uint64_t)rec->gated_shorts;  // wv_lra_gate's, earlier on the stream
    if (n == 0) return;                              // (the whole workgroup; low and high stay 0.0)
    const double r = rel[blockIdx.x];
    const double *st = ST + f.st_off;
    const uint32_t tid = threadIdx.x;
    uint64_t held[kLrHeld];
#pragma unroll
    for (uint32_t i = 0; i < kLrHeld; i++) {
        const uint32_t j = i * kLrSelectThreads + tid;
        const double v = j < f.nshort ? st[j] : 0.0;
        held[i] = j < f.nshort && lr_gated(v, r) ? lr_bits(v) : kLrNone;
    }
    LrRank lo, hi;
    lo.prefix = hi.prefix = 0;
    lo.rank = lr_low_rank(n);
    hi.rank = lr_high_rank(n);
    if (tid < 2u) {  // (what a walk that finds no bin would leave: ordered by the pass's first barrier)
        found[tid].prefix = 0;
        found[tid].rank = tid ? hi.rank : lo.rank;
    }
    for (uint32_t pass = 0; pass < kLrPasses; pass++) {
        hist[0][tid] = 0;
        hist[1][tid] = 0;
        __syncthreads();
        const bool same = lo.prefix == hi.prefix;
#pragma unroll
        for (uint32_t i = 0; i < kLrHeld; i++) lr_count_both(hist, held[i], lo, hi, same, pass);
        for (uint32_t base = kLrHeld * kLrSelectThreads; base < f.nshort; base += kLrSelectThreads) {
            const uint32_t j = base + tid;
            const double v = j < f.nshort ? st[j] : 0.0;
            lr_count_both(hist, j < f.nshort && lr_gated(v, r) ? lr_bits(v) : kLrNone, lo, hi, same, pass);
        }
        __syncthreads();
        const uint32_t wave = tid / kLrWalkLanes, lane = tid % kLrWalkLanes;
        if (wave < 2u) {  // wave 0 walks for the low rank, wave 1 for the high one
            const uint32_t *h = hist[wave && !same ? 1 : 0];
            LrRank a;
            a.prefix = wave ? hi.prefix : lo.prefix;
            a.rank = wave ? hi.rank : lo.rank;
            const uint32_t own = lr_walk_sum(h, lane);
            uint32_t upto = own;  // an inclusive scan over the wave's lanes
#pragma unroll
            for (uint32_t d = 1; d < kLrWalkLanes; d <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)upto, d, 64);
                if (lane >= d) upto += t;
            }
            if (lr_walk_lane(h, lane, upto - own, a, pass)) found[wave] = a;
        }
        __syncthreads();
        lo = found[0];
        hi = found[1];
    }
    if (tid == 0) {
        rec->low_power = lr_value(lo.prefix);
        rec->high_power = lr_value(hi.prefix);
    }
}

hipError_t launch_loudness_range(const LdFile *files, const LrFile *lr, uint32_t nfiles, uint64_t nshorts,
                                 const double *weights, const double *E, double *ST, double *rel, LrRecord *out,
                                 hipStream_t s) {
    if (nshorts) {
        hipLaunchKernelGGL(wv_lra_short, dim3((uint32_t)((nshorts + kLrShortThreads - 1) / kLrShortThreads)),
                           dim3(kLrShortThreads), 0, s, files, lr, nfiles, nshorts, weights, E, ST);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (nfiles) {
        hipLaunchKernelGGL(wv_lra_gate, dim3(nfiles), dim3(kLdGateLanes), 0, s, lr, ST, rel, out);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(wv_lra_select, dim3(nfiles), dim3(kLrSelectThreads), 0, s, lr, ST, rel, out);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace wvg
