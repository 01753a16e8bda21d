// wv_planar.hip -- planar float32 from the decoded ints (gfx950): see wv_planar.h for the
// tile code.
//
// wv_planar_float: one workgroup of 256 threads per job (one frame tile of one file).
// The tile's interleaved ints are read with 16-byte loads, each wave a contiguous 1 KiB
// (single ints up to the first and after the last 16-byte boundary: a file's visible
// range starts at any int), converted in registers and written to the LDS tile channels
// first; after a barrier each row segment goes out as 16-byte stores, one aligned
// ds_read_b128 each (the rows' skew, wv_planar.h), with single floats at its unaligned
// ends and +0.0f past the file's frames.  20 KiB of LDS per workgroup, no scratch, vector
// memory instructions only.  It is a streaming kernel: 4 bytes read and 4 written per
// value, nothing reused.
#include <hip/hip_runtime.h>

#include "wv_planar.h"

namespace wvg {

__global__ void __launch_bounds__(kPlThreads) wv_planar_float(const PlJob *__restrict__ jobs,
                                                              const int32_t *__restrict__ in, float *img) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[kPlLdsInts];
    const PlJob j = jobs[blockIdx.x];
    float *dst = img + j.out_off;
    pl_load(j, in + j.in_off, dst, tile, threadIdx.x, kPlThreads);
    __syncthreads();
    pl_store(j, tile, dst, threadIdx.x, kPlThreads);
}

hipError_t launch_planar(const PlJob *jobs, uint32_t njobs, const int32_t *in, float *img, hipStream_t s) {
    if (!njobs) return hipSuccess;
    hipLaunchKernelGGL(wv_planar_float, dim3(njobs), dim3(kPlThreads), 0, s, jobs, in, img);
    return hipGetLastError();
}

}  // namespace wvg
