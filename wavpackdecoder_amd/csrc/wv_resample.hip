// wv_resample.hip -- planar float32 at one sample rate from the decoded ints (gfx950): see
// wv_resample.h for the tile code.
//
// wv_resample_float: one workgroup of 256 threads per job (one tile of output frames of a
// channel group of one file).  The job's input window is read with 16-byte loads, converted
// once and written to LDS channels first (32 KiB); the FIR runs out of LDS and the
// transposed filter table (L2: a table is shared by every job of its rate pair) with
// 2 phases x 4 blocks of accumulators a lane, each output's chain of v_fma_f32 in tap
// order; the outputs pass through a skewed LDS tile (20 KiB) and leave as 16-byte stores.
// A same-rate job runs planar's tile code in that tile.  52 KiB of LDS per workgroup, no
// scratch, no atomics, vector memory instructions only; every loop is bounded by the job.
#include <hip/hip_runtime.h>

#include "wv_resample.h"

namespace wvg {

__global__ void __launch_bounds__(kRsThreads) wv_resample_float(const RsJob *__restrict__ jobs,
                                                                const int32_t *__restrict__ in, float *img) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kRsLdsFloats];
    const RsJob j = jobs[blockIdx.x];
    float *dst = img + j.out_off;
    if (j.new_ == 0u) {  // (uniform: the job's)
        const PlJob p = rs_planar_job(j);
        pl_load(p, in + p.in_off, dst, lds, threadIdx.x, kRsThreads);
        __syncthreads();
        pl_store(p, lds, dst, threadIdx.x, kRsThreads);
        return;
    }
    uint32_t *xw = lds, *yt = lds + kRsXFloats;
    if (j.nvalid) {
        rs_load(j, in + j.in_off, xw, threadIdx.x, kRsThreads);
        __syncthreads();
        rs_fir(j, xw, yt, dst, threadIdx.x, kRsThreads);
        __syncthreads();
    }
    rs_store(j, yt, dst, threadIdx.x, kRsThreads);
}

hipError_t launch_resample(const RsJob *jobs, uint32_t njobs, const int32_t *in, float *img, hipStream_t s) {
    if (!njobs) return hipSuccess;
    hipLaunchKernelGGL(wv_resample_float, dim3(njobs), dim3(kRsThreads), 0, s, jobs, in, img);
    return hipGetLastError();
}

}  // namespace wvg
