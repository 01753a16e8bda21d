// wv_md5.h -- MD5 (RFC 1321) written once for the host and the device: the state,
// the 64-byte transform and the finalisation (0x80, zero padding, the bit length).
// No dependency beyond <stdint.h>; wv_md5.hip runs it one lane per file and
// wvg_md5_bytes (wv_api.cpp) runs the same text on the host.
//
// The transform is 64 fully unrolled steps over 16 message words passed by
// reference with constant indices only, so on the device the words and the state
// stay in registers.  Per step the dependent chain is four operations: the round
// function (gfx950: one v_bitop3_b32 for each of F, G, H and I), a three-operand
// add of it, the constant and (a + m) -- which does not depend on the chain --,
// the rotate (v_alignbit_b32) and the add of b: 5 VALU a step, 347 a block with
// the loop's own (read from the ISA, DESIGN.md §5 "MD5 on the device").
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WVMD5_HD __host__ __device__ __forceinline__
#define WVMD5_UNROLL _Pragma("unroll")
#else
#define WVMD5_HD inline
#define WVMD5_UNROLL
#endif

namespace wvmd5 {

struct State {
    uint32_t a, b, c, d;
};

WVMD5_HD void init(State &s) {
    s.a = 0x67452301u;
    s.b = 0xefcdab89u;
    s.c = 0x98badcfeu;
    s.d = 0x10325476u;
}

WVMD5_HD uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define WVMD5_STEP(f, a, b, c, d, m, k, r) \
    a = b + rotl(a + (f) + ((m) + (uint32_t)(k)), r)
#define WVMD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define WVMD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define WVMD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define WVMD5_I(b, c, d) ((c) ^ ((b) | ~(d)))

// one 64-byte block: m[j] is bytes 4j..4j+3 of it, little-endian
WVMD5_HD void transform(State &s, const uint32_t (&m)[16]) {
    uint32_t a = s.a, b = s.b, c = s.c, d = s.d;
    WVMD5_STEP(WVMD5_F(b, c, d), a, b, c, d, m[0], 0xd76aa478u, 7);
    WVMD5_STEP(WVMD5_F(a, b, c), d, a, b, c, m[1], 0xe8c7b756u, 12);
    WVMD5_STEP(WVMD5_F(d, a, b), c, d, a, b, m[2], 0x242070dbu, 17);
    WVMD5_STEP(WVMD5_F(c, d, a), b, c, d, a, m[3], 0xc1bdceeeu, 22);
    WVMD5_STEP(WVMD5_F(b, c, d), a, b, c, d, m[4], 0xf57c0fafu, 7);
    WVMD5_STEP(WVMD5_F(a, b, c), d, a, b, c, m[5], 0x4787c62au, 12);
    WVMD5_STEP(WVMD5_F(d, a, b), c, d, a, b, m[6], 0xa8304613u, 17);
    WVMD5_STEP(WVMD5_F(c, d, a), b, c, d, a, m[7], 0xfd469501u, 22);
    WVMD5_STEP(WVMD5_F(b, c, d), a, b, c, d, m[8], 0x698098d8u, 7);
    WVMD5_STEP(WVMD5_F(a, b, c), d, a, b, c, m[9], 0x8b44f7afu, 12);
    WVMD5_STEP(WVMD5_F(d, a, b), c, d, a, b, m[10], 0xffff5bb1u, 17);
    WVMD5_STEP(WVMD5_F(c, d, a), b, c, d, a, m[11], 0x895cd7beu, 22);
    WVMD5_STEP(WVMD5_F(b, c, d), a, b, c, d, m[12], 0x6b901122u, 7);
    WVMD5_STEP(WVMD5_F(a, b, c), d, a, b, c, m[13], 0xfd987193u, 12);
    WVMD5_STEP(WVMD5_F(d, a, b), c, d, a, b, m[14], 0xa679438eu, 17);
    WVMD5_STEP(WVMD5_F(c, d, a), b, c, d, a, m[15], 0x49b40821u, 22);

    WVMD5_STEP(WVMD5_G(b, c, d), a, b, c, d, m[1], 0xf61e2562u, 5);
    WVMD5_STEP(WVMD5_G(a, b, c), d, a, b, c, m[6], 0xc040b340u, 9);
    WVMD5_STEP(WVMD5_G(d, a, b), c, d, a, b, m[11], 0x265e5a51u, 14);
    WVMD5_STEP(WVMD5_G(c, d, a), b, c, d, a, m[0], 0xe9b6c7aau, 20);
    WVMD5_STEP(WVMD5_G(b, c, d), a, b, c, d, m[5], 0xd62f105du, 5);
    WVMD5_STEP(WVMD5_G(a, b, c), d, a, b, c, m[10], 0x02441453u, 9);
    WVMD5_STEP(WVMD5_G(d, a, b), c, d, a, b, m[15], 0xd8a1e681u, 14);
    WVMD5_STEP(WVMD5_G(c, d, a), b, c, d, a, m[4], 0xe7d3fbc8u, 20);
    WVMD5_STEP(WVMD5_G(b, c, d), a, b, c, d, m[9], 0x21e1cde6u, 5);
    WVMD5_STEP(WVMD5_G(a, b, c), d, a, b, c, m[14], 0xc33707d6u, 9);
    WVMD5_STEP(WVMD5_G(d, a, b), c, d, a, b, m[3], 0xf4d50d87u, 14);
    WVMD5_STEP(WVMD5_G(c, d, a), b, c, d, a, m[8], 0x455a14edu, 20);
    WVMD5_STEP(WVMD5_G(b, c, d), a, b, c, d, m[13], 0xa9e3e905u, 5);
    WVMD5_STEP(WVMD5_G(a, b, c), d, a, b, c, m[2], 0xfcefa3f8u, 9);
    WVMD5_STEP(WVMD5_G(d, a, b), c, d, a, b, m[7], 0x676f02d9u, 14);
    WVMD5_STEP(WVMD5_G(c, d, a), b, c, d, a, m[12], 0x8d2a4c8au, 20);

    WVMD5_STEP(WVMD5_H(b, c, d), a, b, c, d, m[5], 0xfffa3942u, 4);
    WVMD5_STEP(WVMD5_H(a, b, c), d, a, b, c, m[8], 0x8771f681u, 11);
    WVMD5_STEP(WVMD5_H(d, a, b), c, d, a, b, m[11], 0x6d9d6122u, 16);
    WVMD5_STEP(WVMD5_H(c, d, a), b, c, d, a, m[14], 0xfde5380cu, 23);
    WVMD5_STEP(WVMD5_H(b, c, d), a, b, c, d, m[1], 0xa4beea44u, 4);
    WVMD5_STEP(WVMD5_H(a, b, c), d, a, b, c, m[4], 0x4bdecfa9u, 11);
    WVMD5_STEP(WVMD5_H(d, a, b), c, d, a, b, m[7], 0xf6bb4b60u, 16);
    WVMD5_STEP(WVMD5_H(c, d, a), b, c, d, a, m[10], 0xbebfbc70u, 23);
    WVMD5_STEP(WVMD5_H(b, c, d), a, b, c, d, m[13], 0x289b7ec6u, 4);
    WVMD5_STEP(WVMD5_H(a, b, c), d, a, b, c, m[0], 0xeaa127fau, 11);
    WVMD5_STEP(WVMD5_H(d, a, b), c, d, a, b, m[3], 0xd4ef3085u, 16);
    WVMD5_STEP(WVMD5_H(c, d, a), b, c, d, a, m[6], 0x04881d05u, 23);
    WVMD5_STEP(WVMD5_H(b, c, d), a, b, c, d, m[9], 0xd9d4d039u, 4);
    WVMD5_STEP(WVMD5_H(a, b, c), d, a, b, c, m[12], 0xe6db99e5u, 11);
    WVMD5_STEP(WVMD5_H(d, a, b), c, d, a, b, m[15], 0x1fa27cf8u, 16);
    WVMD5_STEP(WVMD5_H(c, d, a), b, c, d, a, m[2], 0xc4ac5665u, 23);

    WVMD5_STEP(WVMD5_I(b, c, d), a, b, c, d, m[0], 0xf4292244u, 6);
    WVMD5_STEP(WVMD5_I(a, b, c), d, a, b, c, m[7], 0x432aff97u, 10);
    WVMD5_STEP(WVMD5_I(d, a, b), c, d, a, b, m[14], 0xab9423a7u, 15);
    WVMD5_STEP(WVMD5_I(c, d, a), b, c, d, a, m[5], 0xfc93a039u, 21);
    WVMD5_STEP(WVMD5_I(b, c, d), a, b, c, d, m[12], 0x655b59c3u, 6);
    WVMD5_STEP(WVMD5_I(a, b, c), d, a, b, c, m[3], 0x8f0ccc92u, 10);
    WVMD5_STEP(WVMD5_I(d, a, b), c, d, a, b, m[10], 0xffeff47du, 15);
    WVMD5_STEP(WVMD5_I(c, d, a), b, c, d, a, m[1], 0x85845dd1u, 21);
    WVMD5_STEP(WVMD5_I(b, c, d), a, b, c, d, m[8], 0x6fa87e4fu, 6);
    WVMD5_STEP(WVMD5_I(a, b, c), d, a, b, c, m[15], 0xfe2ce6e0u, 10);
    WVMD5_STEP(WVMD5_I(d, a, b), c, d, a, b, m[6], 0xa3014314u, 15);
    WVMD5_STEP(WVMD5_I(c, d, a), b, c, d, a, m[13], 0x4e0811a1u, 21);
    WVMD5_STEP(WVMD5_I(b, c, d), a, b, c, d, m[4], 0xf7537e82u, 6);
    WVMD5_STEP(WVMD5_I(a, b, c), d, a, b, c, m[11], 0xbd3af235u, 10);
    WVMD5_STEP(WVMD5_I(d, a, b), c, d, a, b, m[2], 0x2ad7d2bbu, 15);
    WVMD5_STEP(WVMD5_I(c, d, a), b, c, d, a, m[9], 0xeb86d391u, 21);
    s.a += a;
    s.b += b;
    s.c += c;
    s.d += d;
}

#undef WVMD5_STEP
#undef WVMD5_F
#undef WVMD5_G
#undef WVMD5_H
#undef WVMD5_I

// Finalisation: the message's last `ntail` bytes (those after the blocks already
// transformed; any count, so a caller may leave more than one block to it), 0x80,
// zeros up to 56 mod 64 and the 64-bit bit count of all `total_bytes`.  at(q)
// returns tail byte q; it is called once for every q of the padded blocks, without
// a branch around it (so a device caller's loads are all in flight together), and
// its result is dropped for q >= ntail: it must be safe to call there.
template <class ByteAt>
WVMD5_HD void finish(State &s, uint32_t ntail, uint64_t total_bytes, const ByteAt &at) {
    const uint32_t nblocks = (ntail + 9 + 63) / 64;
    for (uint32_t blk = 0; blk < nblocks; blk++) {
        uint32_t m[16];
        WVMD5_UNROLL
        for (int j = 0; j < 16; j++) {
            uint32_t w = 0;
            WVMD5_UNROLL
            for (int k = 0; k < 4; k++) {
                const uint32_t q = blk * 64 + (uint32_t)(j * 4 + k);
                const uint32_t v = (uint32_t)at(q) & 0xffu;
                const uint32_t byte = q < ntail ? v : (q == ntail ? 0x80u : 0u);
                w |= byte << (8 * k);
            }
            m[j] = w;
        }
        if (blk == nblocks - 1) {
            m[14] = (uint32_t)(total_bytes << 3);
            m[15] = (uint32_t)(total_bytes >> 29);
        }
        transform(s, m);
    }
}

// the 16 digest bytes: a, b, c, d little-endian
WVMD5_HD void digest(const State &s, uint8_t out[16]) {
    const uint32_t w[4] = {s.a, s.b, s.c, s.d};
    for (int i = 0; i < 16; i++) out[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

}  // namespace wvmd5
