// wv_loud.hip -- integrated loudness of the decoded ints (gfx950): see wv_loud.h for the
// filter, block and gate code.
//
// wv_loud_runs: one lane per job (one run of one channel of one file), 64 jobs a workgroup.
// The jobs of a run's channels are neighbours, so the lanes that share a frame share its
// cache line; a lane's own stream is strided by C ints and read kLdChunk values ahead.  The
// loop-carried chain is two FP64 FMAs per biquad; the second biquad, the square and the
// loads sit beside it.  A lane writes its run's step energies with plain vector stores.
//
// wv_loud_blocks: one thread per P_j of the block image; the file is found by bisection
// over the files' block offsets.
//
// wv_loud_gate: one wave per file; lane l takes blocks l, l + 64, ..., a butterfly over the
// 64 lanes gives the ungated sum, count and maximum, the same again above the relative gate
// the gated ones, and lane 0 writes the 64-byte record.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "wv_loud.h"

namespace wvg {

__device__ __forceinline__ uint64_t ld_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ double ld_xord(double v, int m) {
    return __longlong_as_double((long long)ld_xor64((uint64_t)__double_as_longlong(v), m));
}

// lane ^ m's accumulator
__device__ __forceinline__ LdGate ld_gate_xchg(const LdGate &a, int m) {
    LdGate r;
    r.sum = ld_xord(a.sum, m);
    r.cnt = (int64_t)ld_xor64((uint64_t)a.cnt, m);
    r.mx = ld_xord(a.mx, m);
    return r;
}

__global__ void __launch_bounds__(kLdRunThreads) wv_loud_runs(const LdFile *__restrict__ files,
                                                              const LdRun *__restrict__ runs, uint32_t nruns,
                                                              const double *__restrict__ coefs,
                                                              const int32_t *__restrict__ in, double *__restrict__ E) {
    const uint32_t i = blockIdx.x * kLdRunThreads + threadIdx.x;
    if (i >= nruns) return;
    const LdRun r = runs[i];
    const LdFile f = files[r.file];
    ld_run(f, r, coefs + (uint64_t)f.coef * kLdCoefDoubles, in + f.in_off, E + f.e_off);
}

__global__ void __launch_bounds__(kLdBlockThreads) wv_loud_blocks(const LdFile *__restrict__ files, uint32_t nfiles,
                                                                  uint64_t nblocks, const double *__restrict__ weights,
                                                                  const double *__restrict__ E,
                                                                  double *__restrict__ P) {
    const uint64_t idx = (uint64_t)blockIdx.x * kLdBlockThreads + threadIdx.x;
    if (idx >= nblocks) return;
    const LdFile f = files[ld_find_file(files, nfiles, idx)];
    P[idx] = ld_block(f, E + f.e_off, weights + f.w_off, (uint32_t)(idx - f.blk_off));
}

__global__ void __launch_bounds__(kLdGateLanes) wv_loud_gate(const LdFile *__restrict__ files,
                                                             const double *__restrict__ P,
                                                             LdRecord *__restrict__ out) {
    const LdFile f = files[blockIdx.x];
    const double *p = P + f.blk_off;
    LdGate u = ld_gate_part(p, f.nblocks, threadIdx.x, kLdGateLanes, 0.0);
#pragma unroll
    for (int m = (int)kLdGateLanes / 2; m; m >>= 1) u = ld_gate_merge(u, ld_gate_xchg(u, m));
    LdGate g = ld_gate_part(p, f.nblocks, threadIdx.x, kLdGateLanes, 0.1 * ld_gate_mean(u));
#pragma unroll
    for (int m = (int)kLdGateLanes / 2; m; m >>= 1) g = ld_gate_merge(g, ld_gate_xchg(g, m));
    if (threadIdx.x == 0) ld_record(&f, f.nblocks, u, g, out + blockIdx.x);
}

hipError_t launch_loudness(const LdFile *files, uint32_t nfiles, const LdRun *runs, uint32_t nruns, uint64_t nblocks,
                           const double *coefs, const double *weights, const int32_t *in, double *E, double *P,
                           LdRecord *out, hipStream_t s) {
    if (nruns) {
        hipLaunchKernelGGL(wv_loud_runs, dim3((nruns + kLdRunThreads - 1) / kLdRunThreads), dim3(kLdRunThreads), 0, s,
                           files, runs, nruns, coefs, in, E);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (nblocks) {
        hipLaunchKernelGGL(wv_loud_blocks, dim3((uint32_t)((nblocks + kLdBlockThreads - 1) / kLdBlockThreads)),
                           dim3(kLdBlockThreads), 0, s, files, nfiles, nblocks, weights, E, P);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (nfiles) {
        hipLaunchKernelGGL(wv_loud_gate, dim3(nfiles), dim3(kLdGateLanes), 0, s, files, P, out);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace wvg
