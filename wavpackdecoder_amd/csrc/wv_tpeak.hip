// wv_tpeak.hip -- per-channel true peak of the decoded ints (gfx950): see wv_tpeak.h for
// the tile and combine code.
//
// wv_tpeak_tiles: one workgroup of 256 threads per job (one frame tile of one file).  The
// tile and its halo of 5 + 6 frames are read once, 16 bytes a work item where the address is
// aligned and the four ints lie in the file, and written to the LDS tile channels first,
// zeros outside the file.  The waves' "an int outside +-2^28" flags meet in 4 LDS words
// behind the same barrier: the workgroup then takes the float64 or the int64 form of the
// filter (both exact; the job's O and the flag are uniform, so no lane diverges on them).
// A thread owns a run of R consecutive frames of one row, R odd: the lanes of a wave read
// words R apart, conflict-free, each word once, and the 12-value window slides in
// registers.  The S threads of a row meet in a butterfly over lane ^ m inside the wave, for
// mono and stereo then across the row's waves through 4 LDS slots.  One lane per channel
// writes the tile's 48-byte record with plain vector stores.  No atomics, no scratch.
//
// wv_tpeak_combine: one wave per (file, channel); lane l folds tiles l, l + 64, ... of that
// channel and a butterfly over the 64 lanes gives the record, which lane 0 writes.
#include <hip/hip_runtime.h>

#include "wv_tpeak.h"

namespace wvg {

__device__ __forceinline__ uint64_t tp_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// lane ^ m's accumulator
__device__ __forceinline__ TpAcc tp_xchg(const TpAcc &a, int m) {
    TpAcc r;
    r.peak = tp_xor64(a.peak, m);
    r.pos = (uint32_t)__shfl_xor((int)a.pos, m, 64);
    r.overs = (uint32_t)__shfl_xor((int)a.overs, m, 64);
    r.speak = (uint32_t)__shfl_xor((int)a.speak, m, 64);
    r.sframe = (uint32_t)__shfl_xor((int)a.sframe, m, 64);
    return r;
}

__device__ __forceinline__ TpRecord tp_rec_xchg(const TpRecord &a, int m) {
    TpRecord r;
    r.true_peak = (int64_t)tp_xor64((uint64_t)a.true_peak, m);
    r.true_peak_pos = (int64_t)tp_xor64((uint64_t)a.true_peak_pos, m);
    r.overs = (int64_t)tp_xor64((uint64_t)a.overs, m);
    r.sample_peak = (int64_t)tp_xor64((uint64_t)a.sample_peak, m);
    r.sample_peak_frame = (int64_t)tp_xor64((uint64_t)a.sample_peak_frame, m);
    r.oversample = r.k = 0;
    return r;
}

// (8 waves a SIMD: 64 VGPRs, which the scan fits without a spill, and 20 KiB of LDS; the tile
// read is bound by the bytes in flight a CU)
__global__ void __launch_bounds__(kTpThreads, 8) wv_tpeak_tiles(const TpJob *__restrict__ jobs,
                                                                const int32_t *__restrict__ in,
                                                                TpRecord *__restrict__ partials,
                                                                uint32_t oversample) {
    __shared__ __attribute__((aligned(16))) int32_t tile[kTpLdsInts];
    __shared__ TpAcc wacc[kTpThreads / kTpWave];
    __shared__ uint32_t wwide[kTpThreads / kTpWave];
    const TpJob j = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x, O = oversample ? oversample : j.o_rate;
    const bool mine = tp_load(j, in + j.in_off, tile, tid, kTpThreads);
    const bool wave_wide = __any((int)mine) != 0;
    if ((tid & (kTpWave - 1u)) == 0u) wwide[tid / kTpWave] = wave_wide;
    __syncthreads();
    const bool wide = (wwide[0] | wwide[1] | wwide[2] | wwide[3]) != 0u;
    TpAcc a = tp_scan(j, tile, tid, O, wide);
    // the row's lane group is aligned and a power of two wide: the steps above its width
    // would mix rows (the job is uniform: no lane diverges here)
    const uint32_t lanes = tp_tree_lanes(j.nch);
#pragma unroll
    for (int m = (int)kTpWave / 2; m; m >>= 1)
        if (lanes > (uint32_t)m) a = tp_merge(a, tp_xchg(a, m));
    const uint32_t waves = tp_row_waves(j.nch);
    if (waves > 1u) {  // mono, stereo: a row is 4 or 2 waves wide
        if ((tid & (kTpWave - 1u)) == 0u) wacc[tid / kTpWave] = a;
        __syncthreads();
        if (tid < j.nch) {
            a = wacc[tid * waves];
            for (uint32_t w = 1; w < waves; w++) a = tp_merge(a, wacc[tid * waves + w]);
            tp_partial(j, a, O, partials + j.part + tid);
        }
    } else {
        const uint32_t segs = tp_segments(j.nch), c = tid / segs;
        if (c < j.nch && tid == c * segs) tp_partial(j, a, O, partials + j.part + c);
    }
}

__global__ void __launch_bounds__(kTpCombineLanes) wv_tpeak_combine(const TpFold *__restrict__ folds,
                                                                    const TpRecord *__restrict__ partials,
                                                                    TpRecord *__restrict__ out, uint32_t oversample) {
    const TpFold f = folds[blockIdx.x];
    TpRecord r = tp_fold(f, partials, threadIdx.x, kTpCombineLanes);
#pragma unroll
    for (int m = (int)kTpCombineLanes / 2; m; m >>= 1) r = tp_rec_merge(r, tp_rec_xchg(r, m));
    if (threadIdx.x == 0) tp_final(f, r, oversample, out + blockIdx.x);
}

hipError_t launch_true_peak(const TpJob *jobs, uint32_t njobs, const TpFold *folds, uint32_t nfolds, const int32_t *in,
                            TpRecord *partials, TpRecord *out, uint32_t oversample, hipStream_t s) {
    if (njobs) {
        hipLaunchKernelGGL(wv_tpeak_tiles, dim3(njobs), dim3(kTpThreads), 0, s, jobs, in, partials, oversample);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (nfolds) {
        hipLaunchKernelGGL(wv_tpeak_combine, dim3(nfolds), dim3(kTpCombineLanes), 0, s, folds, partials, out, oversample);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace wvg
