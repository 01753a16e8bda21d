// wv_md5.hip -- the MD5 of every file's decoded audio, on the device (gfx950).
//
// wv_md5_files: one lane per file, one wave of 64 files per workgroup.  A lane
// reads its file's int32 output (never the PCM image: no wvg_batch_format is
// needed), packs each value into the byte form WavPack hashed when it wrote the
// file -- WavpackFormatSamples' forms, WavPackUtils.cs:288-341, with `dsd` per
// file: little-endian at 1..4 bytes per value, one-byte PCM as (t + 128) & 0xFF,
// one-byte DSD as the raw byte -- and runs wv_md5.h's transform on it.  The digest
// (16 bytes) is one dwordx4 store at the file's own index.
//
// 64 values are bytes-per-sample whole MD5 blocks, so the main loop walks the
// file in super-steps of 64 int32 (dwordx4 loads; each value is read once) and
// runs one transform per iteration: block t of the bps blocks of the super-step,
// its 16 words built by the packing of the file's width.  The packing branches
// diverge between lanes of different widths, the transform (9/10 of the
// work) does not, and a lane's trip count is its byte length / 64: the host
// orders the jobs by byte length so that a wave's lanes finish together.  The
// last < 64 values and the padding go through wv_md5.h's finish(), byte by byte.
// The 16 message words and the state live in VGPRs (constant indices only): no
// scratch, no LDS, no cross-lane traffic.
//
// Known limit: MD5 is a serial chain per file, so the kernel's time is the
// longest file's chain at one lane's rate: measured 57 MB/s (C1's 3.5 MB in
// 62 ms, profiles/md5_rates.jsonl), against 1,050 MB/s for hashlib on one host
// thread.  A single very long file is hashed slower than on a host core; the
// kernel is for batches of many files (4,000 C5 files, 255 MB, in 5.6 ms).
#include <hip/hip_runtime.h>

#include "wv_desc.h"
#include "wv_md5.h"

namespace wvg {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// a file's output starts at any int32 of the batch output: 16-byte loads at 4-byte alignment
struct __attribute__((packed, aligned(4))) Quad {
    u32x4 v;
};
__device__ __forceinline__ u32x4 ld4(const int32_t *p) { return reinterpret_cast<const Quad *>(p)->v; }

// four 3-byte values -> three words
#define WV_MD5_Q3(q, w0, w1, w2)                      \
    do {                                              \
        w0 = ((q).x & 0xffffffu) | ((q).y << 24);     \
        w1 = (((q).y >> 8) & 0xffffu) | ((q).z << 16); \
        w2 = (((q).z >> 16) & 0xffu) | ((q).w << 8);  \
    } while (0)

}  // namespace

__global__ void __launch_bounds__(64) wv_md5_files(const Md5Job *__restrict__ jobs, uint32_t njobs,
                                                   const int32_t *__restrict__ out, u32x4 *__restrict__ digests) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= njobs) return;
    const Md5Job job = jobs[j];
    const int32_t *p = out + job.in_off;
    const uint32_t bps = job.bps;
    const uint32_t flip = (bps == 1 && !job.dsd) ? 0x80808080u : 0u;  // (t + 128) & 0xFF == (t & 0xFF) ^ 0x80
    uint64_t left = (job.nvals / 64u) * bps;  // the blocks of the whole super-steps
    uint32_t t = 0;                           // the block of the current super-step
    uint32_t c0 = 0, c1 = 0;                  // 3-byte values: the words a quad leaves to the next block
    wvmd5::State s;
    wvmd5::init(s);
    while (left) {
        uint32_t m[16];
        if (bps == 4) {
            const int32_t *b = p + 16u * t;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const u32x4 q = ld4(b + 4 * i);
                m[4 * i] = q.x;
                m[4 * i + 1] = q.y;
                m[4 * i + 2] = q.z;
                m[4 * i + 3] = q.w;
            }
        } else if (bps == 2) {
            const int32_t *b = p + 32u * t;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const u32x4 q = ld4(b + 4 * i);
                m[2 * i] = (q.x & 0xffffu) | (q.y << 16);
                m[2 * i + 1] = (q.z & 0xffffu) | (q.w << 16);
            }
        } else if (bps == 1) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const u32x4 q = ld4(p + 4 * i);
                m[i] = ((q.x & 0xffu) | ((q.y & 0xffu) << 8) | ((q.z & 0xffu) << 16) | (q.w << 24)) ^ flip;
            }
        } else if (t == 0) {  // 3 bytes: quads 0..5 (bytes 0..71)
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const u32x4 q = ld4(p + 4 * i);
                WV_MD5_Q3(q, m[3 * i], m[3 * i + 1], m[3 * i + 2]);
            }
            const u32x4 q = ld4(p + 20);
            WV_MD5_Q3(q, m[15], c0, c1);
        } else if (t == 1) {  // quads 6..10 (bytes 72..131) after the two words left over
            m[0] = c0;
            m[1] = c1;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const u32x4 q = ld4(p + 24 + 4 * i);
                WV_MD5_Q3(q, m[2 + 3 * i], m[3 + 3 * i], m[4 + 3 * i]);
            }
            const u32x4 q = ld4(p + 40);
            WV_MD5_Q3(q, m[14], m[15], c0);
        } else {  // quads 11..15 (bytes 132..191) after the word left over
            m[0] = c0;
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const u32x4 q = ld4(p + 44 + 4 * i);
                WV_MD5_Q3(q, m[1 + 3 * i], m[2 + 3 * i], m[3 + 3 * i]);
            }
        }
        wvmd5::transform(s, m);
        left--;
        if (++t == bps) {
            t = 0;
            p += 64;
        }
    }
    // the last < 64 values (p points at them), then the padding
    const uint32_t ntail = (uint32_t)(job.nvals % 64u) * bps;
    const int32_t *own = reinterpret_cast<const int32_t *>(jobs + j);  // readable whatever the file holds
    // q / bps for q < 320 as (q * dmul) >> dsh (3: 43691 / 2^17, exact below 2^16)
    const uint32_t dmul = bps == 3 ? 43691u : 1u, dsh = bps == 3 ? 17u : bps >> 1;
    wvmd5::finish(s, ntail, job.nvals * bps, [&](uint32_t q) -> uint32_t {
        // past the tail the load goes to the lane's own job instead (finish drops its result)
        const uint32_t idx = (q * dmul) >> dsh;
        const uint32_t v = (uint32_t)*(q < ntail ? p + idx : own);
        return ((v >> (8u * (q - idx * bps))) ^ flip) & 0xffu;
    });
    u32x4 d;
    d.x = s.a;
    d.y = s.b;
    d.z = s.c;
    d.w = s.d;
    digests[job.file] = d;
}

#undef WV_MD5_Q3

hipError_t launch_md5(const Md5Job *jobs, uint32_t njobs, const int32_t *out, uint8_t *digests, hipStream_t s) {
    if (!njobs) return hipSuccess;
    hipLaunchKernelGGL(wv_md5_files, dim3((njobs + 63) / 64), dim3(64), 0, s, jobs, njobs, out,
                       reinterpret_cast<u32x4 *>(digests));
    return hipGetLastError();
}

}  // namespace wvg
