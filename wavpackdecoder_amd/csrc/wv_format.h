// wv_format.h -- WavPack 4 format constants and table math shared by the host
// framing (wv_framing.cpp), the HIP kernels (wv_decode.hip) and the synthetic
// stream generator (synth/wv_encoder.cpp).
//
// Everything here restates the reference's L0 layer: Defines.cs:13-156 and the
// tables/helpers of WordsUtils.cs:33-66, 513-661.  Functions are
// host+device inline; all integer arithmetic wraps like C# `unchecked`
// (done explicitly through uint32_t so no -fwrapv is needed on the device).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WVF_HD __host__ __device__ __forceinline__
#else
#define WVF_HD inline
#endif

namespace wvf {

// ---- Defines.cs ------------------------------------------------------------
constexpr int SAMPLE_BUFFER_SIZE = 4096;          // Defines.cs:18 (the caller's chunk)
constexpr int BITSTREAM_BUFFER_SIZE = 16 * 1024;  // Defines.cs:20
constexpr uint32_t BYTES_STORED = 3;
constexpr uint32_t MONO_FLAG = 4;
constexpr uint32_t HYBRID_FLAG = 8;
constexpr uint32_t JOINT_STEREO = 0x10;
constexpr uint32_t CROSS_DECORR = 0x20;
constexpr uint32_t HYBRID_SHAPE = 0x40;
constexpr uint32_t FLOAT_DATA = 0x80;
constexpr uint32_t INT32_DATA = 0x100;
constexpr uint32_t HYBRID_BITRATE = 0x200;
constexpr uint32_t HYBRID_BALANCE = 0x400;
constexpr uint32_t INITIAL_BLOCK = 0x800;
constexpr uint32_t FINAL_BLOCK = 0x1000;
constexpr int SHIFT_LSB = 13;
constexpr uint32_t SHIFT_MASK = 0x1fu << SHIFT_LSB;
constexpr int MAG_LSB = 18;
constexpr uint32_t MAG_MASK = 0x1fu << MAG_LSB;
constexpr int SRATE_LSB = 23;
constexpr uint32_t SRATE_MASK = 0xfu << SRATE_LSB;
constexpr uint32_t FALSE_STEREO = 0x40000000u;
constexpr uint32_t MONO_DATA = MONO_FLAG | FALSE_STEREO;
constexpr uint32_t DSD_FLAG = 0x80000000u;
constexpr int MIN_STREAM_VERS = 0x402;
constexpr int MAX_STREAM_VERS = 0x410;

constexpr uint8_t ID_OPTIONAL_DATA = 0x20;
constexpr uint8_t ID_ODD_SIZE = 0x40;
constexpr uint8_t ID_LARGE = 0x80;
constexpr uint8_t ID_DUMMY = 0x0;
constexpr uint8_t ID_ENCODER_INFO = 0x1;
constexpr uint8_t ID_DECORR_TERMS = 0x2;
constexpr uint8_t ID_DECORR_WEIGHTS = 0x3;
constexpr uint8_t ID_DECORR_SAMPLES = 0x4;
constexpr uint8_t ID_ENTROPY_VARS = 0x5;
constexpr uint8_t ID_HYBRID_PROFILE = 0x6;
constexpr uint8_t ID_SHAPING_WEIGHTS = 0x7;
constexpr uint8_t ID_FLOAT_INFO = 0x8;
constexpr uint8_t ID_INT32_INFO = 0x9;
constexpr uint8_t ID_WV_BITSTREAM = 0xa;
constexpr uint8_t ID_WVC_BITSTREAM = 0xb;
constexpr uint8_t ID_WVX_BITSTREAM = 0xc;
constexpr uint8_t ID_CHANNEL_INFO = 0xd;
constexpr uint8_t ID_DSD_BLOCK = 0xe;
constexpr uint8_t ID_RIFF_HEADER = ID_OPTIONAL_DATA | 0x1;
constexpr uint8_t ID_RIFF_TRAILER = ID_OPTIONAL_DATA | 0x2;
constexpr uint8_t ID_ALT_HEADER = ID_OPTIONAL_DATA | 0x3;
constexpr uint8_t ID_ALT_TRAILER = ID_OPTIONAL_DATA | 0x4;
constexpr uint8_t ID_CONFIG_BLOCK = ID_OPTIONAL_DATA | 0x5;
constexpr uint8_t ID_MD5_CHECKSUM = ID_OPTIONAL_DATA | 0x6;
constexpr uint8_t ID_SAMPLE_RATE = ID_OPTIONAL_DATA | 0x7;
constexpr uint8_t ID_ALT_EXTENSION = ID_OPTIONAL_DATA | 0x8;
constexpr uint8_t ID_NEW_CONFIG_BLOCK = ID_OPTIONAL_DATA | 0xa;
constexpr uint8_t ID_WVX_NEW_BITSTREAM = ID_OPTIONAL_DATA | ID_WVX_BITSTREAM;
constexpr uint8_t ID_BLOCK_CHECKSUM = ID_OPTIONAL_DATA | 0xf;

constexpr int MAX_NTERMS = 16;
constexpr int MAX_TERM = 8;
constexpr int LIMIT_ONES = 16;
constexpr int SLS = 8;
constexpr int SLO = 1 << (SLS - 1);

constexpr int FLOAT_SHIFT_ONES = 1;
constexpr int FLOAT_SHIFT_SAME = 2;
constexpr int FLOAT_SHIFT_SENT = 4;
constexpr int FLOAT_ZEROS_SENT = 8;
constexpr int FLOAT_NEG_ZEROS = 0x10;
constexpr int FLOAT_EXCEPTIONS = 0x20;

// open flag beyond the reference (its only one is OPEN_2CH_MAX = 0x8, Defines.cs:26):
// FLOAT_DATA blocks decode to IEEE-754 float32 bit patterns, restored exactly
// from the wvx stream when the block carries one, instead of FloatUtils.cs:32-56's
// scaling to 24-bit integers
constexpr uint32_t OPEN_EXACT_FLOAT = 0x40000000u;
// open flag beyond the reference: a file of more than two channels opens and every
// stream of its block groups is decoded (wv_framing.h, wv_mc.h)
constexpr uint32_t OPEN_ALL_CHANNELS = 0x20000000u;
// open flag beyond the reference: a DSD file opens as 24-bit PCM at the DSD byte rate; its
// blocks decode into a staging range and one more kernel decimates them (wv_dsdpcm.h)
constexpr uint32_t OPEN_DSD_AS_PCM = 0x10000000u;
constexpr uint32_t OPEN_2CH_MAX = 0x8u;

constexpr int64_t CONFIG_HYBRID_FLAG = 8;
constexpr int64_t CONFIG_FLOAT_DATA = 0x80;
constexpr int64_t CONFIG_FAST_FLAG = 0x200;
constexpr int64_t CONFIG_HIGH_FLAG = 0x800;
constexpr int64_t CONFIG_VERY_HIGH_FLAG = 0x1000;
constexpr int64_t CONFIG_LOSSY_MODE = 0x1000000;
constexpr int64_t CONFIG_EXTRA_MODE = 0x2000000;

// ---- C#-semantics integer helpers ---------------
WVF_HD int32_t shl32(int32_t v, int n) { return (int32_t)((uint32_t)v << (n & 31)); }
WVF_HD int32_t sar32(int32_t v, int n) { return v >> (n & 31); }
WVF_HD int32_t add32(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
WVF_HD int32_t sub32(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
WVF_HD int32_t mul32(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
WVF_HD int64_t shl64(int64_t v, int n) { return (int64_t)((uint64_t)v << (n & 63)); }
WVF_HD int64_t sar64(int64_t v, int n) { return v >> (n & 63); }

// (int)((w * (long)s + 512) >> 10) -- the decorrelation weight product
// (UnpackUtils.cs:745 and every pass variant).
WVF_HD int32_t apply_weight(int32_t w, int32_t s) {
    return (int32_t)(((int64_t)w * (int64_t)s + 512) >> 10);
}

// ---- WordsUtils.cs tables (:33-66) -----------------------------------------
#define WVF_EXP2_TABLE                                                                                  \
    0x00, 0x01, 0x01, 0x02, 0x03, 0x03, 0x04, 0x05, 0x06, 0x06, 0x07, 0x08, 0x08, 0x09, 0x0a, 0x0b,   \
        0x0b, 0x0c, 0x0d, 0x0e, 0x0e, 0x0f, 0x10, 0x10, 0x11, 0x12, 0x13, 0x13, 0x14, 0x15, 0x16, 0x16, \
        0x17, 0x18, 0x19, 0x19, 0x1a, 0x1b, 0x1c, 0x1d, 0x1d, 0x1e, 0x1f, 0x20, 0x20, 0x21, 0x22, 0x23, \
        0x24, 0x24, 0x25, 0x26, 0x27, 0x28, 0x28, 0x29, 0x2a, 0x2b, 0x2c, 0x2c, 0x2d, 0x2e, 0x2f, 0x30, \
        0x30, 0x31, 0x32, 0x33, 0x34, 0x35, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x3a, 0x3b, 0x3c, 0x3d, \
        0x3e, 0x3f, 0x40, 0x41, 0x41, 0x42, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x48, 0x49, 0x4a, 0x4b, \
        0x4c, 0x4d, 0x4e, 0x4f, 0x50, 0x51, 0x51, 0x52, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, \
        0x5b, 0x5c, 0x5d, 0x5e, 0x5e, 0x5f, 0x60, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, \
        0x6a, 0x6b, 0x6c, 0x6d, 0x6e, 0x6f, 0x70, 0x71, 0x72, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, \
        0x7a, 0x7b, 0x7c, 0x7d, 0x7e, 0x7f, 0x80, 0x81, 0x82, 0x83, 0x84, 0x85, 0x87, 0x88, 0x89, 0x8a, \
        0x8b, 0x8c, 0x8d, 0x8e, 0x8f, 0x90, 0x91, 0x92, 0x93, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0x9b, \
        0x9c, 0x9d, 0x9f, 0xa0, 0xa1, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa8, 0xa9, 0xaa, 0xab, 0xac, 0xad, \
        0xaf, 0xb0, 0xb1, 0xb2, 0xb3, 0xb4, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xbc, 0xbd, 0xbe, 0xbf, 0xc0, \
        0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc8, 0xc9, 0xca, 0xcb, 0xcd, 0xce, 0xcf, 0xd0, 0xd2, 0xd3, 0xd4, \
        0xd6, 0xd7, 0xd8, 0xd9, 0xdb, 0xdc, 0xdd, 0xde, 0xe0, 0xe1, 0xe2, 0xe4, 0xe5, 0xe6, 0xe8, 0xe9, \
        0xea, 0xec, 0xed, 0xee, 0xf0, 0xf1, 0xf2, 0xf4, 0xf5, 0xf6, 0xf8, 0xf9, 0xfa, 0xfc, 0xfd, 0xff

#define WVF_LOG2_TABLE                                                                                  \
    0x00, 0x01, 0x03, 0x04, 0x06, 0x07, 0x09, 0x0a, 0x0b, 0x0d, 0x0e, 0x10, 0x11, 0x12, 0x14, 0x15,   \
        0x16, 0x18, 0x19, 0x1a, 0x1c, 0x1d, 0x1e, 0x20, 0x21, 0x22, 0x24, 0x25, 0x26, 0x28, 0x29, 0x2a, \
        0x2c, 0x2d, 0x2e, 0x2f, 0x31, 0x32, 0x33, 0x34, 0x36, 0x37, 0x38, 0x39, 0x3b, 0x3c, 0x3d, 0x3e, \
        0x3f, 0x41, 0x42, 0x43, 0x44, 0x45, 0x47, 0x48, 0x49, 0x4a, 0x4b, 0x4d, 0x4e, 0x4f, 0x50, 0x51, \
        0x52, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x5c, 0x5d, 0x5e, 0x5f, 0x60, 0x61, 0x62, 0x63, \
        0x64, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x6b, 0x6c, 0x6d, 0x6e, 0x6f, 0x70, 0x71, 0x72, 0x74, 0x75, \
        0x76, 0x77, 0x78, 0x79, 0x7a, 0x7b, 0x7c, 0x7d, 0x7e, 0x7f, 0x80, 0x81, 0x82, 0x83, 0x84, 0x85, \
        0x86, 0x87, 0x88, 0x89, 0x8a, 0x8b, 0x8c, 0x8d, 0x8e, 0x8f, 0x90, 0x91, 0x92, 0x93, 0x94, 0x95, \
        0x96, 0x97, 0x98, 0x99, 0x9a, 0x9b, 0x9b, 0x9c, 0x9d, 0x9e, 0x9f, 0xa0, 0xa1, 0xa2, 0xa3, 0xa4, \
        0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xa9, 0xaa, 0xab, 0xac, 0xad, 0xae, 0xaf, 0xb0, 0xb1, 0xb2, 0xb2, \
        0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xb9, 0xba, 0xbb, 0xbc, 0xbd, 0xbe, 0xbf, 0xc0, 0xc0, \
        0xc1, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xcb, 0xcb, 0xcc, 0xcd, 0xce, \
        0xcf, 0xd0, 0xd0, 0xd1, 0xd2, 0xd3, 0xd4, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd8, 0xd9, 0xda, 0xdb, \
        0xdc, 0xdc, 0xdd, 0xde, 0xdf, 0xe0, 0xe0, 0xe1, 0xe2, 0xe3, 0xe4, 0xe4, 0xe5, 0xe6, 0xe7, 0xe7, \
        0xe8, 0xe9, 0xea, 0xea, 0xeb, 0xec, 0xed, 0xee, 0xee, 0xef, 0xf0, 0xf1, 0xf1, 0xf2, 0xf3, 0xf4, \
        0xf4, 0xf5, 0xf6, 0xf7, 0xf7, 0xf8, 0xf9, 0xf9, 0xfa, 0xfb, 0xfc, 0xfc, 0xfd, 0xfe, 0xff, 0xff

#if !defined(__HIP_DEVICE_COMPILE__)
static const uint8_t host_exp2_table[256] = {WVF_EXP2_TABLE};
static const uint8_t host_log2_table[256] = {WVF_LOG2_TABLE};
#endif

// nbits_table[v] == bit length of v (WordsUtils.cs:33-51)
WVF_HD int nbits8(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// count_bits(long) for 0 <= av < 2^32 (WordsUtils.cs:513-537)
WVF_HD int count_bits_u32(uint32_t av) { return av ? 32 - __builtin_clz(av) : 0; }

// exp2s (WordsUtils.cs:633-646) -- host version; the device has its own copy
// reading the table from constant memory.
#if !defined(__HIP_DEVICE_COMPILE__)
static inline int exp2s_host(int log) {
    if (log < 0) return -exp2s_host(-log);
    int64_t value = host_exp2_table[log & 0xff] | 0x100;
    if ((log >>= 8) <= 9) return (int)sar64(value, 9 - log);
    return (int)shl64(value, log - 9);
}

// mylog2 (WordsUtils.cs:588-608) for 0 <= avalue < 2^32 (callers guarantee it)
static inline int mylog2_host(int64_t avalue) {
    int dbits;
    if ((avalue += (avalue >> 9)) < (1 << 8)) {
        dbits = nbits8((uint32_t)avalue);
        return (dbits << 8) + host_log2_table[(int)shl64(avalue, 9 - dbits) & 0xff];
    }
    if (avalue < (1LL << 16))
        dbits = nbits8((uint32_t)(avalue >> 8)) + 8;
    else if (avalue < (1LL << 24))
        dbits = nbits8((uint32_t)(avalue >> 16)) + 16;
    else
        dbits = nbits8((uint32_t)(avalue >> 24)) + 24;
    return (dbits << 8) + host_log2_table[(int)sar64(avalue, dbits - 9) & 0xff];
}

// log2s (WordsUtils.cs:615-625)
static inline int log2s_host(int32_t v) { return v < 0 ? -mylog2_host(-(int64_t)v) : mylog2_host(v); }
#endif

// restore_weight (WordsUtils.cs:653-661)
WVF_HD int restore_weight(int8_t weight) {
    int result = weight * 8;
    if (result > 0) result += (result + 64) >> 7;
    return result;
}

// store_weight: the encoder-side inverse [ext, WavPack 4 words.c]; only the
// generator uses it, the decoder never does.
WVF_HD int8_t store_weight(int weight) {
    if (weight > 1024) weight = 1024;
    else if (weight < -1024) weight = -1024;
    if (weight > 0) weight -= (weight + 64) >> 7;
    return (int8_t)((weight + 4) >> 3);
}

}  // namespace wvf
