// wv_dsdpcm.hip -- DSD bytes to 24-bit PCM (gfx950): see wv_dsdpcm.h for the tile code.
//
// wv_dsd_pcm: workgroups of 256 threads; each copies the 13 x 256 byte tables into LDS once
// (13,312 bytes) and then takes jobs blockIdx.x, blockIdx.x + gridDim.x, ... (one frame
// tile of one file each), so a large batch pays the table copy once per workgroup and not
// once per tile.  Per job the tile and its halo are read once from HBM with 16-byte loads
// and packed into the byte window (7,200 bytes of LDS); after a barrier every 16-byte
// slot of the destination is 13 window reads (two words each) and 52 table reads, added in
// int32, and one 16-byte store.  No scratch, vector memory instructions only.
#include <hip/hip_runtime.h>

#include "wv_dsdpcm.h"

namespace wvg {

__constant__ DpTables kDpTablesDev = dp_make_tables();

constexpr uint32_t kDpMaxGroups = 2048;  // 8 per CU: enough to keep 256 CUs' memory pipes busy

__global__ void __launch_bounds__(kDpThreads) wv_dsd_pcm(const DpJob *__restrict__ jobs, uint32_t njobs, int32_t *out) {
    __shared__ __attribute__((aligned(16))) int32_t tab[kDpBytes * 256];
    __shared__ __attribute__((aligned(16))) uint32_t win[kDpWinWords];
    for (uint32_t i = threadIdx.x; i < kDpBytes * 256u; i += kDpThreads) tab[i] = kDpTablesDev.t[i];
    for (uint32_t q = blockIdx.x; q < njobs; q += gridDim.x) {
        const DpJob j = jobs[q];
        __syncthreads();  // the tables; the window's readers of the job before
        dp_load(j, out + j.in_off, win, threadIdx.x, kDpThreads);
        __syncthreads();
        dp_store(j, win, tab, out + j.out_off, threadIdx.x, kDpThreads);
    }
}

hipError_t launch_dsdpcm(const DpJob *jobs, uint32_t njobs, int32_t *out, hipStream_t s) {
    if (!njobs) return hipSuccess;
    const uint32_t groups = njobs < kDpMaxGroups ? njobs : kDpMaxGroups;
    hipLaunchKernelGGL(wv_dsd_pcm, dim3(groups), dim3(kDpThreads), 0, s, jobs, njobs, out);
    return hipGetLastError();
}

}  // namespace wvg
