// wv_levels.hip -- per-channel level statistics of the decoded ints (gfx950): see
// wv_levels.h for the tile and combine code.
//
// wv_levels_tiles: one workgroup of 256 threads per job (one frame tile of one file).  The
// tile's interleaved ints are read with 16-byte loads, each wave a contiguous 1 KiB (single
// ints up to the first and after the last 16-byte boundary: a file's visible range starts
// at any int) and written to the LDS tile channels first; after a barrier the S threads of
// a row scan it with consecutive lanes on consecutive words, and their accumulators meet
// in a butterfly over lane ^ m inside the wave (S <= 64 lanes), for mono and stereo then
// across the row's waves through 4 LDS slots.  One lane per channel writes the tile's
// 64-byte record with plain vector stores.  No atomics, no scratch; it is a streaming
// kernel: 4 bytes read per value, 64 bytes written per (tile, channel).
//
// wv_levels_combine: one wave per (file, channel); lane l folds tiles l, l + 64, ... of
// that channel and a butterfly over the 64 lanes gives the record, which lane 0 writes.
#include <hip/hip_runtime.h>

#include "wv_levels.h"

namespace wvg {

__device__ __forceinline__ uint64_t lv_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// lane ^ m's accumulator
__device__ __forceinline__ LvAcc lv_xchg(const LvAcc &a, int m) {
    LvAcc r;
    r.mn = __shfl_xor(a.mn, m, 64);
    r.mx = __shfl_xor(a.mx, m, 64);
    r.sum = (int64_t)lv_xor64((uint64_t)a.sum, m);
    r.lo = lv_xor64(a.lo, m);
    r.hi = (uint32_t)__shfl_xor((int)a.hi, m, 64);
    r.clipped = (uint32_t)__shfl_xor((int)a.clipped, m, 64);
    r.active = (uint32_t)__shfl_xor((int)a.active, m, 64);
    r.first = (uint32_t)__shfl_xor((int)a.first, m, 64);
    r.last = __shfl_xor(a.last, m, 64);
    return r;
}

__device__ __forceinline__ LvRecord lv_rec_xchg(const LvRecord &a, int m) {
    LvRecord r;
    r.min = __shfl_xor(a.min, m, 64);
    r.max = __shfl_xor(a.max, m, 64);
    r.sum = (int64_t)lv_xor64((uint64_t)a.sum, m);
    r.sumsq_lo = lv_xor64(a.sumsq_lo, m);
    r.sumsq_hi = lv_xor64(a.sumsq_hi, m);
    r.clipped = (int64_t)lv_xor64((uint64_t)a.clipped, m);
    r.active = (int64_t)lv_xor64((uint64_t)a.active, m);
    r.first_active = (int64_t)lv_xor64((uint64_t)a.first_active, m);
    r.last_active = (int64_t)lv_xor64((uint64_t)a.last_active, m);
    return r;
}

__global__ void __launch_bounds__(kLvThreads) wv_levels_tiles(const LvJob *__restrict__ jobs,
                                                              const int32_t *__restrict__ in,
                                                              LvRecord *__restrict__ partials,
                                                              uint32_t threshold_q31) {
    __shared__ __attribute__((aligned(16))) int32_t tile[kLvLdsInts];
    __shared__ LvAcc wacc[kLvThreads / kLvWave];
    const LvJob j = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    lv_load(j, in + j.in_off, tile, tid, kLvThreads);
    __syncthreads();
    LvAcc a = lv_scan(j, tile, tid, threshold_q31);
    // the row's lane group is aligned and a power of two wide: the steps above its width
    // would mix rows (the job is uniform: no lane diverges here)
    const uint32_t lanes = lv_tree_lanes(j.nch);
#pragma unroll
    for (int m = (int)kLvWave / 2; m; m >>= 1)
        if (lanes > (uint32_t)m) a = lv_merge(a, lv_xchg(a, m));
    const uint32_t waves = lv_row_waves(j.nch);
    if (waves > 1u) {  // mono, stereo: a row is 4 or 2 waves wide
        if ((tid & (kLvWave - 1u)) == 0u) wacc[tid / kLvWave] = a;
        __syncthreads();
        if (tid < j.nch) {
            a = wacc[tid * waves];
            for (uint32_t w = 1; w < waves; w++) a = lv_merge(a, wacc[tid * waves + w]);
            lv_partial(j, a, partials + j.part + tid);
        }
    } else {
        const uint32_t segs = lv_segments(j.nch), c = tid / segs;
        if (c < j.nch && tid == c * segs) lv_partial(j, a, partials + j.part + c);
    }
}

__global__ void __launch_bounds__(kLvCombineLanes) wv_levels_combine(const LvFold *__restrict__ folds,
                                                                     const LvRecord *__restrict__ partials,
                                                                     LvRecord *__restrict__ out) {
    const LvFold f = folds[blockIdx.x];
    LvRecord r = lv_fold(f, partials, threadIdx.x, kLvCombineLanes);
#pragma unroll
    for (int m = (int)kLvCombineLanes / 2; m; m >>= 1) r = lv_rec_merge(r, lv_rec_xchg(r, m));
    if (threadIdx.x == 0) lv_final(f, r, out + blockIdx.x);
}

hipError_t launch_levels(const LvJob *jobs, uint32_t njobs, const LvFold *folds, uint32_t nfolds, const int32_t *in,
                         LvRecord *partials, LvRecord *out, uint32_t threshold_q31, hipStream_t s) {
    if (njobs) {
        hipLaunchKernelGGL(wv_levels_tiles, dim3(njobs), dim3(kLvThreads), 0, s, jobs, in, partials, threshold_q31);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (nfolds) {
        hipLaunchKernelGGL(wv_levels_combine, dim3(nfolds), dim3(kLvCombineLanes), 0, s, folds, partials, out);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace wvg
