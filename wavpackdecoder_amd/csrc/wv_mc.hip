// wv_mc.hip -- the multichannel interleave (gfx950): see wv_mc.h for the tile code.
//
// wv_mc_interleave: one workgroup of 256 threads per job (one frame tile of one file).
// Every stream's part of the tile is read with 16-byte loads, each wave a contiguous
// 1 KiB, and written to the LDS tile at [f * nch + ch]; after a barrier the tile goes
// out as contiguous 16-byte stores (scalar ints up to the first and after the last
// 16-byte boundary: a file's visible range starts at any int).  16 KiB of LDS per
// workgroup, no scratch, vector memory instructions only.
//
// wv_mc_plain (WVG_MC_PLAIN=1, the A/B): no LDS; one lane per frame per stream, a 4- or
// 8-byte load and a strided 4- or 8-byte store.  Kept for the measurement in DESIGN §5.
#include <hip/hip_runtime.h>

#include "wv_mc.h"

namespace wvg {

__global__ void __launch_bounds__(kMcThreads) wv_mc_interleave(const McJob *__restrict__ jobs,
                                                               const McStreamDev *__restrict__ streams,
                                                               int32_t *out) {
    __shared__ __attribute__((aligned(16))) int32_t tile[kMcTileInts];
    const McJob j = jobs[blockIdx.x];
    for (uint32_t s = 0; s < j.nstreams; s++) {
        const McStreamDev st = streams[j.first_stream + s];
        mc_gather(j, st, out + st.off, tile, threadIdx.x, kMcThreads);
    }
    __syncthreads();
    mc_store(j, tile, out + j.out_off, threadIdx.x, kMcThreads);
}

__global__ void __launch_bounds__(kMcThreads) wv_mc_plain(const McJob *__restrict__ jobs,
                                                          const McStreamDev *__restrict__ streams, int32_t *out) {
    typedef int32_t i2 __attribute__((ext_vector_type(2)));
    const McJob j = jobs[blockIdx.x];
    int32_t *dst = out + j.out_off;
    for (uint32_t s = 0; s < j.nstreams; s++) {
        const McStreamDev st = streams[j.first_stream + s];
        const uint64_t have = st.frames > j.frame0 ? st.frames - j.frame0 : 0;
        const uint32_t nf = have < (uint64_t)j.nframes ? (uint32_t)have : j.nframes;
        const int32_t *p = out + st.off + j.frame0 * (uint64_t)st.width;
        for (uint32_t f = threadIdx.x; f < j.nframes; f += kMcThreads) {
            int32_t *o = dst + f * j.nch + st.ch;
            if (st.width == 2u) {
                i2 v = {0, 0};
                if (f < nf) v = *reinterpret_cast<const i2 *>(p + 2u * f);  // (8-byte aligned: see wv_mc.h)
                if (((uintptr_t)o & 7u) == 0) {
                    *reinterpret_cast<i2 *>(o) = v;
                } else {
                    o[0] = v.x;
                    o[1] = v.y;
                }
            } else {
                o[0] = f < nf ? p[f] : 0;
            }
        }
    }
}

hipError_t launch_mc(const McJob *jobs, uint32_t njobs, const McStreamDev *streams, int32_t *out, int plain,
                     hipStream_t s) {
    if (!njobs) return hipSuccess;
    if (plain)
        hipLaunchKernelGGL(wv_mc_plain, dim3(njobs), dim3(kMcThreads), 0, s, jobs, streams, out);
    else
        hipLaunchKernelGGL(wv_mc_interleave, dim3(njobs), dim3(kMcThreads), 0, s, jobs, streams, out);
    return hipGetLastError();
}

}  // namespace wvg
