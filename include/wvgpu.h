/*
 * wvgpu.h -- C-ABI of the MI355X WavPack block-decode path (libwvgpu.so).
 *
 * Drop-in boundary for the reference's hot path
 *   public static long WavPackUtils.WavpackUnpackSamples(WavpackContext wpc, int[] buffer, long samples)
 *   (Quake4/WavPackDecoder WavPackUtils.cs:200-282)
 * and the calls around it that a C# host needs to keep its API:
 *   WavpackOpenFileInput   WavPackUtils.cs:36-120   -> wvg_batch_add_file (framing, info)
 *   WavpackUnpackSamples   WavPackUtils.cs:200-282  -> wvg_batch_decode (+ download)
 *   WavpackFormatSamples   WavPackUtils.cs:288-341  -> wvg_format_samples
 *   WavpackGetNumErrors    WavPackUtils.cs:363      -> wvg_file_result.crc_errors
 *   WavpackLossy           WavPackUtils.cs:371      -> wvg_file_result.lossy
 *   other getters          WavPackUtils.cs:346-499  -> wvg_file_info
 *
 * Blittable types only (P/Invoke ready): every buffer is caller-owned; the
 * library keeps device copies owned by the batch handle.  Errors are int
 * return codes (0 = OK, < 0 = error) plus wvg_last_error(); no C++
 * exception crosses the ABI.  One context per device per host thread.
 *
 * Output contract: a batch decodes every file exactly as a caller looping
 * WavpackUnpackSamples(wpc, buffer, chunk_frames) (WvDemo.cs:110-135) would
 * receive it, concatenated: int32 per channel-sample, interleaved,
 * right-justified; float files as clipped 24-bit ints (FloatUtils.cs:32-56);
 * DSD as one byte value per channel-sample.
 */
#ifndef WVGPU_H
#define WVGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WVG_OK 0
#define WVG_ERR_HIP (-1)      /* HIP runtime error (see wvg_last_error) */
#define WVG_ERR_ARG (-2)      /* bad argument / state */
#define WVG_ERR_OPEN (-3)     /* WavpackOpenFileInput failed (info.error holds the message) */
#define WVG_ERR_SPACE (-4)    /* caller buffer too small */
#define WVG_ERR_TIMEOUT (-5)  /* a kernel's bounded wait ran out (a decoder bug, never a property of the stream) */
#define WVG_ERR_EXCEPTION (-6) /* wvg_stream_*: the reference raises a C# exception in this call */

/* per-block status bits (wvg_file_result.status_or) */
#define WVG_ST_CRC_CHECKED 0x01u
#define WVG_ST_CRC_ERROR 0x02u
#define WVG_ST_MUTED 0x04u
#define WVG_ST_BITS_ERROR 0x08u
#define WVG_ST_EXCEPTION 0x10u   /* the reference raises a C# exception in this block */
#define WVG_ST_UNSUPPORTED 0x20u /* depends on decode state of an earlier block (never in well-formed files) */
#define WVG_ST_DSD_MUTE 0x40u
#define WVG_ST_NONDET 0x80u      /* reference output depends on stale caller-buffer contents */
#define WVG_ST_TIMEOUT 0x100u    /* the parser/reconstruction handshake timed out: output invalid (not a reference outcome) */
#define WVG_ST_REDONE 0x200u     /* wvg_batch_block_status only: the lane kernel handed this block back and the
                                    one-workgroup-per-block kernel decoded it (a cost, never a result: masked out
                                    of wvg_file_result.status_or) */
#define WVG_ST_UNWRITTEN 0x40000000u /* wvg_batch_block_status only: no decode has stored this block's status since
                                        wvg_batch_poison (a bench/test check that a decode really ran) */

typedef struct wvg_ctx wvg_ctx;
typedef struct wvg_batch wvg_batch;

/* What WavpackOpenFileInput + the getters report (WavPackUtils.cs:36-120, 346-499). */
typedef struct {
    int32_t open_ok;            /* 0 => error[] holds wpc.error_message */
    int32_t num_channels;       /* WavpackGetNumChannels */
    int32_t reduced_channels;   /* WavpackGetReducedChannels (ints per output frame) */
    int32_t bits_per_sample;    /* WavpackGetBitsPerSample (DSD: /8 applied like the getter) */
    int32_t bytes_per_sample;   /* WavpackGetBytesPerSample */
    int32_t version;            /* WavpackGetVersion */
    int32_t mode;               /* WavpackGetMode */
    int32_t is_float;           /* WavpackGetIsFloat */
    int32_t is_five;            /* WavpackGetIsFive */
    int32_t file_format;        /* WavpackGetFileFormat */
    int32_t lossy;              /* WavpackLossy at open */
    uint32_t dsd_multiplier;
    int64_t sample_rate;        /* WavpackGetSampleRate */
    int64_t total_samples;      /* WavpackGetNumSamples(native=false), -1 unknown */
    int64_t out_frames;         /* frames the chunked caller receives */
    int64_t out_offset;         /* int32 index of this file's output inside the batch */
    int64_t header_off, header_len;   /* RIFF/ALT header bytes inside the file (WavpackGetHeader), -1 none */
    int64_t trailer_off, trailer_len; /* WavpackGetTrailer */
    char error[96];
    int32_t seek_result;        /* wvg_batch_add_file_at: SetSample's result (1 true, 0 false, -1 it threw) */
    int32_t reserved;
    int64_t sample_index0;      /* WavpackGetSampleIndex when the first WavpackUnpackSamples call starts
                                   (after SetSample: the target); it then advances by the frames returned */
} wvg_file_info;

typedef struct {
    int64_t frames;             /* == info.out_frames unless an exception stopped the decode */
    int64_t crc_errors;         /* WavpackGetNumErrors after the last call */
    int32_t lossy;              /* WavpackLossy after the last call */
    int32_t exception;          /* the reference would have thrown (WvDemo exits 1) */
    uint32_t status_or;         /* OR of the WVG_ST_* bits of all blocks */
    int32_t num_blocks;
    int64_t exception_frame;    /* with exception: frames the calls before the throwing call returned
                                   (the throwing call is the one that starts there); -1 otherwise */
} wvg_file_result;

/* Device + stream ownership.  device < 0 => current device. */
wvg_ctx *wvg_open(int device);
void wvg_close(wvg_ctx *ctx);
const char *wvg_last_error(wvg_ctx *ctx);

/* A batch of files decoded together.  chunk_frames is the caller's per-call
 * frame count (Defines.SAMPLE_BUFFER_SIZE = 4096 for WvDemo); it fixes the
 * reference's chunk seams (weight (short) stores, mute granularity). */
wvg_batch *wvg_batch_new(wvg_ctx *ctx, int chunk_frames);
void wvg_batch_free(wvg_batch *b);

/* Frame one file (host): parses headers/metadata, records the blocks.
 * The bytes are copied into the batch.  Returns the file index (>= 0) or
 * WVG_ERR_OPEN (info->error set; the file contributes no output). */
int wvg_batch_add_file(wvg_batch *b, const uint8_t *file, size_t len, uint32_t open_flags, wvg_file_info *info);

/* n files at once, framed on `threads` host threads (<= 0: WVG_FRAME_THREADS or
 * the hardware concurrency, at most 16); the same result as n wvg_batch_add_file
 * calls in order.  indices[i] receives file i's index or WVG_ERR_OPEN; returns n. */
int wvg_batch_add_files(wvg_batch *b, int n, const uint8_t *const *files, const size_t *lens, uint32_t open_flags,
                        int threads, wvg_file_info *infos, int32_t *indices);

/* The same, for a caller that calls WavPackUtils.SetSample(wpc, start_sample)
 * (WavPackUtils.cs:509-594: the block search, then decode-and-discard up to the
 * sample in calls of 4096 / reduced-channels frames) right after opening: the
 * file's output is what the following WavpackUnpackSamples calls return.
 * info->seek_result holds SetSample's result; when it is 0 the output starts
 * at the beginning, as the reference's context does. */
int wvg_batch_add_file_at(wvg_batch *b, const uint8_t *file, size_t len, uint32_t open_flags, int64_t start_sample,
                          wvg_file_info *info);

/* open_flags bit beyond the reference (whose only flag is OPEN_2CH_MAX = 0x8,
 * Defines.cs:26): FLOAT_DATA blocks decode to IEEE-754 float32 bit patterns by
 * WavPack 4's float_values -- exact when the block carries its classic
 * ID_WVX_BITSTREAM (in the .wv, or in the .wvc for a hybrid file) -- instead of
 * FloatUtils.cs:32-56's scaling to 24-bit integers.  Blocks with a wvx stream
 * check its crc (WVG_ST_CRC_ERROR); a NEW-format float wvx stream is
 * WVG_ST_UNSUPPORTED.  Parity: round trip to the encoder's float input. */
#define WVG_OPEN_EXACT_FLOAT 0x40000000u

/* open_flags bit beyond the reference (which refuses a file of more than two channels,
 * "only two channels supported!", or with OPEN_2CH_MAX decodes its first stream only):
 * every channel is decoded.  A multichannel WavPack file is a sequence of block groups
 * INITIAL_BLOCK .. FINAL_BLOCK, one mono or stereo block per stream; with this flag a
 * file whose ID_CHANNEL_INFO count N is greater than 2 opens with info.num_channels =
 * info.reduced_channels = N, and its output is info.out_frames frames of N interleaved
 * int32 at info.out_offset, channels in stream order (stream s at channel offset
 * sum(widths[:s]), wvg_batch_file_streams).
 *   Semantics: stream s is framed exactly as the reference frames, under OPEN_2CH_MAX, a
 * file in which stream s's blocks are the INITIAL_BLOCK ones -- the same call loop at
 * chunk_frames, seams, gaps, mute, CRC and exception rules, the stream's own width -- so
 * stream 0 is bit for bit the reference's OPEN_2CH_MAX output.  out_frames is stream
 * 0's: a stream that delivers fewer frames leaves zeros, one that delivers more is cut.
 * The layout (streams and widths) is the first group's and must add up to N (else the
 * file does not open); a later block of another width is WVG_ST_UNSUPPORTED.
 * wvg_file_result aggregates over all streams' blocks (exception_frame: the smallest),
 * wvg_batch_file_blocks lists them stream after stream, wvg_batch_md5 hashes the
 * N-channel output.  WVG_OPEN_EXACT_FLOAT may be combined (it acts per block).
 *   Cost: every stream decodes into a staging range of its own inside the batch's int32
 * output, after the file's visible range (16-byte aligned), and one more kernel weaves
 * them into the N-channel frames at the end of wvg_batch_decode; wvg_batch_out_ints and
 * a full wvg_batch_download include the staging (about twice the file's output).
 *   On a file of at most two channels the flag changes nothing.
 *   Out of scope (WVG_ERR_ARG): together with OPEN_2CH_MAX, wvg_batch_add_file_at (seek)
 * and wvg_batch_add_file_wvc; wvg_stream_open returns NULL; wvg_batch_add_files_device
 * takes no flags. */
#define WVG_OPEN_ALL_CHANNELS 0x20000000u
/* The stream layout of a file opened with WVG_OPEN_ALL_CHANNELS (host only): widths[s] =
 * ints a frame of stream s (1 or 2; up to `cap` are written), *channel_mask = its
 * ID_CHANNEL_INFO mask.  Returns the stream count -- 1 for a file of at most two channels
 * (its own width, the default mask) -- or WVG_ERR_OPEN when the file does not open. */
int wvg_probe_file_streams(const uint8_t *file, size_t len, int32_t *widths, int cap, uint32_t *channel_mask);
/* the same for a file of a batch */
int wvg_batch_file_streams(const wvg_batch *b, int file, int32_t *widths, int cap, uint32_t *channel_mask);
/* The interleave kernel's tile code (wv_mc.h) run on the host: `frames` frames of
 * nstreams streams (widths[s] ints a frame each) woven into out[frames x sum(widths)].
 * wvg_interleave_tile_frames: the frames of one tile for a channel count (1..255). */
int wvg_interleave_streams(const int32_t *const *streams, const int32_t *widths, int nstreams, int64_t frames,
                           int32_t *out);
int wvg_interleave_tile_frames(int channels);

/* ---- DSD files as 24-bit PCM (open_flags bit beyond the reference, whose DSD output is
 * one byte value -- eight one-bit samples -- per channel-sample; WavPack's own library has
 * OPEN_DSD_AS_PCM).  A DSD file added or probed with this flag presents itself as a 24-bit
 * PCM file at the DSD byte rate: info.bits_per_sample = 24, bytes_per_sample = 3,
 * sample_rate = the unflagged value / 8 (dsd_multiplier x the stored rate; 352,800 for
 * DSD64), every other field as without the flag -- dsd_multiplier, mode, out_frames,
 * total_samples, reduced_channels.  Its output is info.out_frames frames of
 * info.reduced_channels interleaved int32 at info.out_offset, each within +-(2^23 - 1), and
 * every later call works on it as on any 24-bit file: wvg_batch_format (3-byte little
 * endian), md5, planar (k = 23), levels (k = 23), resample (352,800 -> 44,100 is 8:1, ->
 * 48,000 is 147:20, -> 16,000 is 441:20: all inside the resampler's limits), and
 * decode_to_tensors.  OPEN_2CH_MAX combines with it as it does without.  On a file that is
 * not DSD the flag changes nothing: info, offsets, wvg_batch_out_ints, output.
 *   The filter (fixed; exact integer arithmetic): T = 104 taps over bits, 13 bytes of history
 * centred on the output's byte.  Tap t = 8 j + i is bit i of window byte j (j = 0 oldest;
 * i = 0 the byte's MSB, the earliest in time).  In float64
 *     x_t = clamp((t - 51.5) * 0.99 / 8, -6, +6)
 *     h_t = sinc(pi x_t) * cos(pi x_t / 12)^2              (sinc(0) = 1)
 *     c_t = trunc(h_t / sum |h| * (2^23 - 1))              (toward zero)
 * -- wvg_batch_resample's Hann-windowed sinc (lpw 6, rolloff 0.99) at ratio 8:1, byte
 * aligned.  The table is 104 committed integer constants (wvg_dsd_pcm_taps), symmetric, taps
 * 0..3 and 100..103 zero, sum |c| = 8,388,570 <= 2^23 - 1 (no output can leave 24 bits: no
 * clipping rule, no int32 overflow), sum c = 5,355,358: the DC gain is sum c / 2^23 = 0.638.
 *   Output, with F = out_frames, C = ints per frame and src the decoded DSD ints:
 *     B[q][c] = src[q * C + c] & 0xFF  for 0 <= q < F, else 0x55 (DSD's idle pattern)
 *     s_i(b)  = +1 if (b >> (7 - i)) & 1 else -1
 *     y[m][c] = sum_{j=0..12} sum_{i=0..7} c_{8j+i} * s_i(B[m - 6 + j][c])
 * The filter runs over whatever the DSD decode left over out_frames, as format, md5 and
 * planar define their input: a zero-filled gap or the frames after an exception are bytes
 * of 0x00 (eight -1 bits).
 *   Cost: the file's blocks decode into a staging range inside its part of the batch's int32
 * output (16-byte aligned, before the visible range; only info.out_offset is contract), and
 * one more kernel (wv_dsdpcm.hip) filters it into the visible range at the end of every
 * wvg_batch_decode; wvg_batch_out_ints and a full wvg_batch_download include the staging
 * (twice the file's output).  Statuses, wvg_file_result, wvg_batch_file_blocks and the
 * kernel routing are those of the unflagged file.  wvg_batch_md5: the stored sum is over the
 * DSD bytes, so the verdict is WVG_MD5_NOT_COMPARABLE; `computed` covers the 3-byte form.
 *   Out of scope: WVG_ERR_ARG together with WVG_OPEN_ALL_CHANNELS (multichannel DSD; the
 * kernel and wvg_dsd_pcm_ints take 1..255 channels, so that is a change to the framing's
 * offsets only), with wvg_batch_add_file_at and wvg_batch_add_file_wvc; wvg_stream_open
 * returns NULL; wvg_batch_add_files_device takes no flags; wvg_batch_wav returns WVG_ERR_ARG
 * for a flagged DSD file (its stored header describes one-bit audio).  Other filters, a
 * gain, and decimation past the byte rate are the resampler's job.
 *   Host only: wvg_dsd_pcm_taps copies the table (*sum = sum c, *sum_abs = sum |c|; either may
 * be NULL); wvg_dsd_pcm_ints runs the kernel's tile code (wv_dsdpcm.h) over `frames` x
 * `channels` interleaved ints (channels 1..255, any 4-byte alignment, src != out);
 * wvg_dsd_pcm_tile_frames: the frames of one tile for a channel count (1..255). */
#define WVG_OPEN_DSD_AS_PCM 0x10000000u
int wvg_dsd_pcm_taps(int32_t taps[104], int64_t *sum, int64_t *sum_abs);
int wvg_dsd_pcm_ints(const int32_t *src, int64_t frames, int channels, int32_t *out);
int wvg_dsd_pcm_tile_frames(int channels);

/* A hybrid .wv file with its .wvc correction file: the hybrid blocks decode
 * EXACTLY (lossless) instead of the reference's lossy output.  Beyond the
 * reference (it opens ID_WVC_BITSTREAM, UnpackUtils.cs:96-106, but never reads
 * it): parity is the round trip to the encoder's input.  Returns the
 * file index or WVG_ERR_OPEN, as wvg_batch_add_file. */
int wvg_batch_add_file_wvc(wvg_batch *b, const uint8_t *file, size_t len, const uint8_t *wvc, size_t wvc_len,
                           uint32_t open_flags, wvg_file_info *info);

/* n files framed ON THE DEVICE at the next wvg_batch_upload (the
 * WavpackOpenFileInput header + sub-block walk of WavPackUtils.cs:36-120,600-671,
 * UnpackUtils.cs:24-68, MetadataUtils.cs:15-192 as kernels, open_flags 0).  The
 * bytes are copied now and file slots reserved (indices[i]); a file outside the
 * device framer's scope (DSD mode 1, wvx, sticky state, junk, damaged headers) is framed
 * by the host at the same upload with the same result as wvg_batch_add_file.
 * The files' infos are available after the upload (wvg_batch_file_info). */
int wvg_batch_add_files_device(wvg_batch *b, int n, const uint8_t *const *files, const size_t *lens,
                               int32_t *indices);
/* A file's info (after the upload for device-framed files); WVG_ERR_OPEN if it did not open. */
int wvg_batch_file_info(const wvg_batch *b, int file, wvg_file_info *info);
/* Files [first, first + n) at once (one call for a whole device-framed slice); returns how
 * many were copied (fewer when the batch has fewer files). */
int wvg_batch_file_infos(const wvg_batch *b, int first, int n, wvg_file_info *infos);
/* Files of the batch framed on the device / by the host fallback at its uploads. */
int wvg_batch_framing_stats(const wvg_batch *b, int64_t *device_files, int64_t *host_files);
/* Diagnostics: which launch groups the last wvg_batch_decode ran on the lane / row
 * kernels (bit t: PCM term-set group t, 0..7; bit 8: .wvc blocks; bit 9: DSD mode 3;
 * bit 10: DSD mode 1) -- under WVG_KERNEL_AUTO the choice depends on whether other
 * batches of the context overlapped within the last second.  No reference counterpart. */
int wvg_batch_lane_groups(const wvg_batch *b, uint32_t *mask);

/* Drop every file of the batch but keep its device and page-locked host
 * buffers (a decode server refills one batch per request). */
int wvg_batch_reset(wvg_batch *b);

/* Copy blob + descriptors to the device and zero the output (device buffers are
 * kept across uploads of a refilled batch and only grown). */
int wvg_batch_upload(wvg_batch *b);

/* Enqueue the decode kernels on `stream` (hipStream_t, NULL = the batch's own
 * stream).  Input and output stay in HBM.  Every batch owns its streams, so
 * batches decode concurrently; nothing synchronises the whole device. */
int wvg_batch_decode(wvg_batch *b, void *stream);
/* Wait for the batch's last decode / format (an event on the stream it ran on). */
int wvg_batch_sync(wvg_batch *b);
/* Which kernel decodes the batch's lossless PCM blocks whose decorr list has a
 * compile-time specialisation (no reference counterpart: a scheduling choice).
 * WVG_KERNEL_LANE: one lane per block, 64 blocks per workgroup -- one SIMD issue
 * slot moves 64 blocks, so batches in flight decode many times more per second --
 * for lossless PCM blocks, hybrid stereo blocks of WavPack's default list and DSD
 * mode-3 blocks; blocks a lane cannot follow exactly are decoded again by the
 * two-wave kernel (the pipelined kernel for WavPack's 16-term 'high' list, the
 * wave-per-block kernel for DSD) within the same decode.  WVG_KERNEL_TWO_WAVE: one
 * workgroup per block (a scalar parser wave and a reconstruction wave; one wave
 * per DSD block), the lowest latency for a batch alone.  WVG_KERNEL_AUTO (the
 * default): the lane kernels once the context has had a decode issued while another
 * of its batches was running; until then (one batch at a time) the two-wave /
 * wave-per-block kernels for launch groups of at most 2,048 blocks (larger ones on
 * lanes).  A decode issued while other batches
 * run also keeps all its launch groups on its own stream (streams share the
 * process's few hardware queues).  Results are identical in every mode
 * (WVG_LANE_KERNEL=0/1 in the environment fixes the kernel for new batches). */
#define WVG_KERNEL_TWO_WAVE 0
#define WVG_KERNEL_LANE 1
#define WVG_KERNEL_AUTO 2
int wvg_batch_set_kernel(wvg_batch *b, int kernel);
void *wvg_batch_stream(wvg_batch *b);  /* the batch's own hipStream_t */
/* Verification aid (no reference counterpart): overwrite the uploaded batch's int32
 * output with `byte` in every byte and mark every decodable block WVG_ST_UNWRITTEN, so
 * that what a download shows afterwards was written by the decodes issued after this
 * call.  Waits for the batch's earlier work.  (Gaps the reference zero-fills are left
 * poisoned until the next wvg_batch_upload.) */
int wvg_batch_poison(wvg_batch *b, int byte);
/* Device timing of every following decode (an event pair around each launch, on its
 * stream); wvg_batch_timed waits for them and returns the mean and the count. */
int wvg_batch_set_timing(wvg_batch *b, int on);
int wvg_batch_timed(wvg_batch *b, float *avg_ms, int *count);
/* With timing on: for the last decode, the time from its start to the end of
 * each launch group on its own stream, ms[g] for g = term set 0..7, 8 generic
 * PCM, 9 DSD, 10 DSD mode 1 (-1: not launched); cap >= 11. */
int wvg_batch_group_times(wvg_batch *b, float *ms, int cap);

int64_t wvg_batch_out_ints(const wvg_batch *b);
int32_t *wvg_batch_device_out(wvg_batch *b);      /* device pointer to the int32 output */
int64_t wvg_batch_num_blocks(const wvg_batch *b);
int64_t wvg_batch_bytes_in(const wvg_batch *b);   /* compressed bytes of all decoded blocks */
int64_t wvg_batch_frames(const wvg_batch *b);     /* frames of all decoded blocks */

/* Download output (and per-block statuses) and fill per-file results.
 * host_out == NULL with cap_ints == -1: into the batch's own page-locked
 * buffer (full PCIe rate), read through wvg_batch_host_out until the next
 * download or wvg_batch_free; host_out == NULL otherwise: statuses only. */
int wvg_batch_download(wvg_batch *b, int32_t *host_out, int64_t cap_ints);
int32_t *wvg_batch_host_out(wvg_batch *b);
int wvg_batch_file_result(wvg_batch *b, int file, wvg_file_result *res);
/* per-block status words (after download), one per decoded block in file order */
int wvg_batch_block_status(wvg_batch *b, uint32_t *out, int64_t cap);
/* Diagnostics (a library built with -DWV_LANE_COUNTERS=1 -- make counters -- and
 * batches created with WVG_LANE_COUNTERS=1 in the environment; zeros otherwise): per
 * parser wave of term set `ts`'s last lane-kernel decode, 16 words -- cycles, groups,
 * then groups taken as a zero-run bulk step / no-run words / split no-run words /
 * run-aware words / checked words at once / checked replay, then the cycles spent
 * waiting for the reconstruction wave and for the payload loads, in the groups'
 * words and in their ring stores (low 32 bits of each count).  Returns the wave
 * count (out needs 16 per wave), WVG_ERR_ARG without counters. */
int wvg_batch_lane_counters(wvg_batch *b, int ts, uint32_t *out, int64_t cap);
/* The blocks of one file (after download): for block k, end_frame[k] = the number of
 * frames the caller has received when the block's last frame is unpacked (that is
 * when WavpackUnpackSamples runs check_crc_error, WavPackUtils.cs:273-275), and its
 * status word.  Returns the block count, or < 0. */
int wvg_batch_file_blocks(wvg_batch *b, int file, int64_t *end_frame, uint32_t *status, int64_t cap);

/* Device-side timing of `iters` back-to-back decodes (hipEvents on the
 * batch stream).  *ms receives the average per decode. */
int wvg_batch_time(wvg_batch *b, int iters, float *ms);

/* One-shot convenience: frame + upload + decode + download one file (open_flags 0: a file of
 * more than two channels needs a batch and WVG_OPEN_ALL_CHANNELS). */
int wvg_decode_file(wvg_ctx *ctx, const uint8_t *file, size_t len, int chunk_frames, int32_t *out, int64_t cap_ints,
                    wvg_file_info *info, wvg_file_result *res);

/* WavpackOpenFileInput (WavPackUtils.cs:36-120) without a device: host framing
 * only, fills what the getters report.  WVG_ERR_OPEN when the file does not open. */
int wvg_probe_file(const uint8_t *file, size_t len, uint32_t open_flags, int chunk_frames, wvg_file_info *info);

/* WavpackFormatSamples (WavPackUtils.cs:288-341) on the host: int32 -> LE PCM bytes. */
int wvg_format_samples(const int32_t *src, int64_t samcnt, int bps, uint8_t *pcm, int64_t pcm_len, int offset,
                       int dsd);

/* WavpackFormatSamples over a decoded batch, on the device (epilogue kernel on
 * `stream` after wvg_batch_decode): every file's int32 output becomes its
 * little-endian PCM image at info.bytes_per_sample, 1-byte samples +128 unless
 * `dsd` (the reference's dsd argument; WvDemo.cs:125 passes false).  The image
 * stays in HBM; file i starts at byte wvg_batch_pcm_offset(b, i). */
int wvg_batch_format(wvg_batch *b, int dsd, void *stream);
int64_t wvg_batch_pcm_bytes(const wvg_batch *b);
int64_t wvg_batch_pcm_offset(const wvg_batch *b, int file);  /* -1: the file did not open */
uint8_t *wvg_batch_device_pcm(wvg_batch *b);                 /* device pointer to the PCM image */
/* host == NULL and cap == -1: into the batch's page-locked buffer (full PCIe
 * rate), read through wvg_batch_host_pcm until the next such download. */
int wvg_batch_download_pcm(wvg_batch *b, uint8_t *host, int64_t cap);
uint8_t *wvg_batch_host_pcm(wvg_batch *b);
/* The same download into the batch's page-locked buffer, queued behind the format
 * on the batch stream without waiting for it: a decode server issues a request's
 * upload, decode, format and download back to back and takes the PCM
 * (wvg_batch_host_pcm) after wvg_batch_sync -- the next reset/upload of the batch
 * waits for it too.  (The reference's WavpackUnpackSamples + WavpackFormatSamples
 * calls, WavPackUtils.cs:200-341, return the PCM synchronously; this is their
 * batched, overlapped form.) */
int wvg_batch_download_pcm_async(wvg_batch *b);

/* ---- The stored MD5 sums, verified on the device (beyond the reference, which skips
 * ID_MD5_CHECKSUM as optional data; `wvunpack -v -m` is the WavPack tool's form).
 * WavPack stores the MD5 of the source audio bytes -- little-endian at
 * bytes_per_sample, one-byte PCM unsigned, DSD the raw bytes: WavpackFormatSamples'
 * forms (WavPackUtils.cs:288-341) -- in a 16-byte sub-block of the last audio block or
 * of a zero-sample block after it.  wvg_batch_md5 hashes every file's int32 output in
 * that form, one lane per file (wv_md5.hip), after the whole of the batch's last decode;
 * it needs neither wvg_batch_format nor a download, returns without waiting
 * (wvg_batch_sync covers it; the next reset / upload waits for it), and only the
 * digests (16 bytes a file) come back to the host.  Float files hash their float32 bit
 * patterns (4 bytes a value) under WVG_OPEN_EXACT_FLOAT.
 * Known limit: MD5 is a serial chain, so the kernel takes as long as its longest file
 * at one lane's rate -- measured 57 MB/s of audio bytes per lane, where hashlib does
 * 1,050 MB/s on one host thread (DESIGN.md §5 "MD5 on the device") -- and pays off for
 * batches of many files: 4,000 C5 files (255 MB of audio) hash in 5.6 ms.
 * verdict, from framing facts only: NONE without a stored sum; NOT_COMPARABLE when a sum
 * is stored but this decode cannot reproduce the source bytes (a hybrid file without its
 * .wvc, lossy INT32 / float blocks, a float file without WVG_OPEN_EXACT_FLOAT, a file
 * added with wvg_batch_add_file_at or reduced by OPEN_2CH_MAX, a DSD file opened with
 * WVG_OPEN_DSD_AS_PCM); else MATCH / MISMATCH
 * (a CRC error, a mute or an exception changes the output: MISMATCH).  `computed` is
 * always filled; `bytes` is the hashed length. */
#define WVG_MD5_NONE 0
#define WVG_MD5_MATCH 1
#define WVG_MD5_MISMATCH 2
#define WVG_MD5_NOT_COMPARABLE 3
typedef struct {
    uint8_t computed[16];
    uint8_t stored[16];
    int32_t has_stored;
    int32_t verdict;
    int64_t bytes;
} wvg_file_md5;
int wvg_batch_md5(wvg_batch *b, void *stream);                     /* after wvg_batch_decode */
int wvg_batch_file_md5(wvg_batch *b, int file, wvg_file_md5 *out); /* after wvg_batch_sync / wvg_batch_download;
                                                                      WVG_ERR_ARG: no wvg_batch_md5 since the last
                                                                      upload; WVG_ERR_OPEN: the file did not open */
/* host only: the stored sum of a file (the last one; a trailing zero-sample block's
 * included): 1 found, 0 none, WVG_ERR_OPEN */
int wvg_probe_file_md5(const uint8_t *file, size_t len, uint8_t stored[16]);
/* the kernel's MD5 core (wv_md5.h) run on the host over `len` bytes */
int wvg_md5_bytes(const uint8_t *data, size_t len, uint8_t digest[16]);

/* ---- Planar float32 on the device (beyond the reference, which has no float output):
 * the decoded batch as float32 in [-1, 1), channels first, for a model, a resampler or
 * any DSP on the same device -- one kernel per batch (wv_planar.hip), no download.
 *   A file is convertible when it opened and its output is not DSD bytes (a DSD byte holds
 * eight one-bit samples; a DSD file opened with WVG_OPEN_DSD_AS_PCM is 24-bit PCM and
 * convertible).  The image holds the convertible files in file
 * order, file i as C = info.reduced_channels rows (planes) of row_stride floats, row c at
 * float offset + c * row_stride; with F = info.out_frames:
 *     fixed_frames == 0 (ragged): row length L = F, row_stride = (F + 3) & ~3, offset =
 *       the sum of C_j * row_stride_j over the convertible files before it -- every row
 *       starts at a multiple of 16 bytes from the image's base;
 *     fixed_frames == T > 0: L = row_stride = T, offset = T * the sum of C_j over the
 *       convertible files before it -- files of equal C form one dense [B, C, T] array
 *       (rows are not 16-byte aligned when T % 4 != 0; the kernel does not need them to be).
 *   Plane c, frame f is conv(out[info.out_offset + f * C + c]) for f < min(F, L); the
 * frames from min(F, L) to row_stride are +0.0f.  Every float of the image is written by
 * every call (the destination may be uninitialised memory) and nothing outside it.  What
 * is converted is whatever the int32 output holds over out_frames, as wvg_batch_format: a
 * file stopped by an exception has zeros where the decode left zeros.
 *   conv, by file: (float)v * 2^-k with k = 8 * info.bytes_per_sample - 1 (7, 15, 23, 31;
 * one-byte samples are signed in the int32 output: no +128), and k = 23 for a float file
 * decoded without WVG_OPEN_EXACT_FLOAT (the reference's clipped 24-bit integers) whatever
 * its bytes_per_sample.  The cast rounds to nearest even (it matters above 2^24 only) and
 * the multiplication by a power of two is exact, so the result is bit for bit numpy's
 * v.astype(float32) * float32(2.0 ** -k).  A float file decoded under
 * WVG_OPEN_EXACT_FLOAT holds IEEE-754 patterns already: its 32 bits pass through
 * unchanged, NaN payloads included (the decision is the framing's, as wvg_batch_md5's
 * byte form).
 *   wvg_batch_planar runs after wvg_batch_decode, on `stream` (NULL: the batch's own)
 * behind the upload and the batch's last decode / format / md5, and returns without
 * waiting (wvg_batch_sync covers it; the next reset / upload waits for it).  dev_dst ==
 * NULL: into a buffer the batch owns (cap_floats is ignored), read through
 * wvg_batch_device_planar / wvg_batch_download_planar until the next such call;
 * otherwise into the caller's device memory of cap_floats floats on the batch's device
 * (a torch tensor's data_ptr(), any 4-byte alignment).  Calls with other fixed_frames or
 * destinations may be queued back to back.  WVG_ERR_SPACE: cap_floats is less than
 * wvg_batch_planar_floats(b, fixed_frames); WVG_ERR_ARG: before an upload, fixed_frames < 0.
 *   wvg_batch_file_planar: file i's place in the image -- *frames = min(F, L) -- or
 * WVG_ERR_OPEN with *offset = -1 for a file that is not convertible (host only, as
 * wvg_batch_planar_floats; device-framed files are known after the upload).
 *   wvg_planar_float: the kernel's tile code (wv_planar.h) run on the host over one file's
 * `frames` x `channels` interleaved ints: `channels` rows of row_stride floats at `out`,
 * min(frames, row_len) frames converted (kind: 7 / 15 / 23 / 31 = k, 0 = the bits pass
 * through), +0.0f up to row_stride (>= row_len).  wvg_planar_tile_frames: the frames of one
 * tile for a channel count (1..255). */
int wvg_batch_planar(wvg_batch *b, int64_t fixed_frames, float *dev_dst, int64_t cap_floats, void *stream);
int64_t wvg_batch_planar_floats(const wvg_batch *b, int64_t fixed_frames);
int wvg_batch_file_planar(const wvg_batch *b, int file, int64_t fixed_frames, int64_t *offset, int64_t *row_stride,
                          int32_t *channels, int64_t *frames);
float *wvg_batch_device_planar(wvg_batch *b); /* the batch-owned image of the last dev_dst == NULL call */
int wvg_batch_download_planar(wvg_batch *b, float *host, int64_t cap_floats); /* that image; waits */
int wvg_planar_float(const int32_t *src, int64_t frames, int channels, int kind, int64_t row_len, int64_t row_stride,
                     float *out);
int wvg_planar_tile_frames(int channels);

/* ---- Planar float32 at one sample rate on the device (beyond the reference): planar's
 * twin.  After a decode every resamplable file is converted as above and brought from its
 * own info.sample_rate to the caller's out_rate by a polyphase FIR, float32 and channels
 * first in planar's two layouts -- one kernel per batch (wv_resample.hip) plus the uploads
 * of the filter tables, no download.  With fixed_frames files of one channel count form one
 * dense [B, C, T] array at one rate.
 *   Rates: g = gcd(in_rate, out_rate), orig = in_rate / g, new = out_rate / g.  The pair is
 * supported when orig <= 1024, new <= 1024 and K <= 4096 (K below).
 *   Filter: a Hann-windowed sinc in the layout of torchaudio's sinc_interp_hann resampler,
 * with fixed parameters lpw = 6 zero crossings and rolloff = 0.99, in float64 on the host:
 *     base  = min(orig, new) * rolloff
 *     width = ceil(lpw * orig / base)          K = 2 * width + orig
 *     for p in 0..new-1, j in 0..K-1:
 *         t = clamp((-p / new + (j - width) / orig) * base, -lpw, +lpw)
 *         h64[p][j] = sinc(pi * t) * cos(pi * t / (2 * lpw))^2 * (base / orig)     (sinc(0) = 1)
 *         h[p][j]   = +0.0f if |h64| < 2^-64 else (float)h64     (one rounding, to nearest even)
 * (the flush keeps every product away from float32 denormals: host and device cannot
 * differ by a denormal mode).
 *   Output: with F = info.out_frames and x[c][m] = planar's conv(out[out_offset + m * C + c])
 * for 0 <= m < F (SCALE(k), the same k rule), else +0.0f, the file has
 * F' = ceil(F * new / orig) output frames, and for n = i * new + p with 0 <= p < new
 *     y[c][n] = acc_K,  acc_0 = +0.0f,  acc_{j+1} = fmaf(h[p][j], x[c][i * orig + j - width], acc_j)
 * with j = 0 .. K-1 ascending: one accumulator, one order, fused multiply-adds.  A tap
 * outside the file adds exactly nothing.  in_rate == out_rate: no filter; the row is
 * planar's conversion bit for bit.
 *   A file is resamplable when it opened, its output is not DSD bytes (WVG_OPEN_DSD_AS_PCM
 * makes a DSD file resamplable), is not a float file decoded under
 * WVG_OPEN_EXACT_FLOAT (levels' rule: use the default clipped 24-bit decode), has
 * sample_rate > 0, and its pair is supported.  The others take no room in the image: their
 * offset is -1 and wvg_batch_file_resample returns WVG_ERR_OPEN.  WVG_OPEN_ALL_CHANNELS
 * files are resampled over their woven N channels, 1 to 255.
 *   Image: planar's rules with F' in place of F -- ragged: row length F', row_stride =
 * (F' + 3) & ~3; fixed_frames == T > 0: rows of T output-rate frames, cut or zero-padded.
 * Every float of the image is written by every call and nothing outside it; the
 * destination is at any 4-byte alignment; all offsets are 64-bit.
 *   wvg_batch_resample is ordered as wvg_batch_planar: after wvg_batch_decode, on `stream`
 * (NULL: the batch's own) behind the upload and the batch's last decode / format / md5 /
 * planar / levels / resample; it returns without waiting, and wvg_batch_sync, reset and
 * upload cover it.  dev_dst == NULL: into a buffer the batch owns, its own and not
 * planar's (wvg_batch_device_resampled / wvg_batch_download_resampled until the next such
 * call).  Job tables are built once per upload and (out_rate, fixed_frames), filter tables
 * once per batch and (in_rate, out_rate), each into memory of its own, so calls with other
 * arguments may be queued back to back; four job tables are kept per upload, a fifth pair
 * of arguments waits for the batch's work and reuses the oldest.  WVG_ERR_SPACE:
 * cap_floats is less than wvg_batch_resample_floats; WVG_ERR_ARG: before an upload,
 * out_rate < 1, out_rate > INT32_MAX, fixed_frames < 0.
 *   wvg_batch_file_resample: file i's place in the image, *frames = min(F', L) (host only,
 * as wvg_batch_file_planar).
 *   Host only: wvg_resample_filter returns new * K and, with taps != NULL, fills the table
 * row-major [new][K] (WVG_ERR_ARG: the pair is not supported; WVG_ERR_SPACE: cap_floats is
 * short); wvg_resample_float runs the kernel's job builder and tile code (wv_resample.h)
 * over one file's `frames` x `channels` interleaved ints: `channels` rows of row_stride
 * floats at `out`, min(F', row_len) frames computed, +0.0f up to row_stride (>= row_len),
 * kind = k (7 / 15 / 23 / 31; equal rates: wvg_planar_float); wvg_resample_tile_frames:
 * the output frames of one job for a rate pair and a channel count (1..255). */
int wvg_batch_resample(wvg_batch *b, int64_t out_rate, int64_t fixed_frames, float *dev_dst, int64_t cap_floats,
                       void *stream);
int64_t wvg_batch_resample_floats(const wvg_batch *b, int64_t out_rate, int64_t fixed_frames);
int wvg_batch_file_resample(const wvg_batch *b, int file, int64_t out_rate, int64_t fixed_frames, int64_t *offset,
                            int64_t *row_stride, int32_t *channels, int64_t *frames);
float *wvg_batch_device_resampled(wvg_batch *b); /* the batch-owned image of the last dev_dst == NULL call */
int wvg_batch_download_resampled(wvg_batch *b, float *host, int64_t cap_floats); /* that image; waits */
int wvg_resample_filter(int64_t in_rate, int64_t out_rate, int32_t *orig, int32_t *new_, int32_t *width, float *taps,
                        int64_t cap_floats);
int wvg_resample_float(const int32_t *src, int64_t frames, int channels, int kind, int64_t in_rate, int64_t out_rate,
                       int64_t row_len, int64_t row_stride, float *out);
int wvg_resample_tile_frames(int64_t in_rate, int64_t out_rate, int channels);

/* ---- Per-channel level statistics on the device (beyond the reference): what a consumer
 * of a decoded batch computes next -- peak, DC offset, RMS, clip count, where the audio
 * starts and ends -- as exact integers, 64 bytes per channel, with two kernels per batch
 * (wv_levels.hip) and no PCM downloaded: the statistics twin of wvg_batch_md5.
 *   A file is measurable when it opened, its output is not DSD bytes (a DSD byte holds eight
 * one-bit samples; with WVG_OPEN_DSD_AS_PCM a DSD file is measured at k = 23) and is not a float file decoded under WVG_OPEN_EXACT_FLOAT (its ints are
 * IEEE-754 patterns, and sums of floats are not exact).  Measured is whatever the int32
 * output holds over info.out_frames frames of C = info.reduced_channels interleaved ints at
 * info.out_offset, as wvg_batch_format, md5 and planar: a file stopped by an exception has
 * its zeros counted, a WVG_OPEN_ALL_CHANNELS file is measured over its woven N channels.
 *   One record per channel, over the channel's values v:
 *     min, max      0, 0 for a file of no frames
 *     sum           exact
 *     sumsq         the sum of v * v as a 128-bit integer, sumsq_hi * 2^64 + sumsq_lo, exact
 *     clipped       values on the rails: v >= 2^k - 1 or v <= -2^k
 *     active        values with v > thr or v < -thr
 *     first_active, last_active   frame index of the first / last active value, -1: none
 * k is planar's full-scale exponent: 8 * info.bytes_per_sample - 1 (7, 15, 23, 31), and 23
 * for a float file decoded without WVG_OPEN_EXACT_FLOAT.  thr = threshold_q31 >> (31 - k):
 * one silence threshold in Q31 full-scale units, applied by each file at its own depth.
 * INT32_MIN is a legal value of 32-bit files; no absolute value is taken anywhere.
 *   wvg_batch_levels runs after wvg_batch_decode, on `stream` (NULL: the batch's own)
 * behind the upload and the batch's last decode / format / md5 / planar / levels, and
 * returns without waiting (wvg_batch_sync covers it; the next reset / upload waits for
 * it).  The records come down with the call, queued behind the kernels into page-locked
 * memory.  Calls with other thresholds may be queued back to back: each starts on the
 * device when the one before has downloaded its records, and the last one defines what
 * wvg_batch_file_levels returns.  Every record is written by every call.  WVG_ERR_ARG:
 * before an upload, threshold_q31 above 0x7FFFFFFF.
 *   wvg_batch_file_levels, after wvg_batch_sync: returns C and fills min(C, cap_channels)
 * records; WVG_ERR_OPEN for a file that is not measurable; WVG_ERR_ARG when no
 * wvg_batch_levels ran since the last upload.
 *   wvg_levels_ints: the kernels' tile and combine code (wv_levels.h) run on the host over
 * `frames` x `channels` interleaved ints (channels 1..255, k one of 7 / 15 / 23 / 31):
 * `channels` records at `out`.  wvg_levels_tile_frames: the frames of one tile for a channel
 * count (1..255). */
typedef struct {            /* 64 bytes, one per (measurable file, channel) */
    int32_t  min, max;
    int64_t  sum;
    uint64_t sumsq_lo, sumsq_hi;
    int64_t  clipped;
    int64_t  active;
    int64_t  first_active;
    int64_t  last_active;
} wvg_channel_levels;

int wvg_batch_levels(wvg_batch *b, uint32_t threshold_q31, void *stream);
int wvg_batch_file_levels(wvg_batch *b, int file, wvg_channel_levels *out, int cap_channels);
int wvg_levels_ints(const int32_t *src, int64_t frames, int channels, int k, uint32_t threshold_q31,
                    wvg_channel_levels *out);
int wvg_levels_tile_frames(int channels);

/* ---- True peak on the device (beyond the reference): ITU-R BS.1770 Annex 2's maximum of
 * the oversampled signal, per channel, as exact integers, 48 bytes per channel, with two
 * kernels per batch (wv_tpeak.hip) and no PCM downloaded.  What ReplayGain 2.0 and EBU R 128
 * pair with programme loudness: whether a gain clips.  wvg_batch_levels' min / max is the
 * sample peak; a full-scale sine at fs/4 sampled 45 degrees off its crests has a sample peak
 * of -3.01 dBFS and a true peak of 0 dBTP.
 *   A file is measurable by levels' rule, unchanged: it opened, its output is not DSD bytes
 * (with WVG_OPEN_DSD_AS_PCM a DSD file is measured at k = 23) and it is not a float file
 * decoded under WVG_OPEN_EXACT_FLOAT.  Measured is whatever the int32 output holds over
 * info.out_frames frames of C = info.reduced_channels interleaved ints at info.out_offset;
 * a WVG_OPEN_ALL_CHANNELS file is measured over its woven N channels.  k is planar's
 * full-scale exponent (7, 15, 23, 31; 23 for a float file without the exact flag).
 *   Oversampling factor O: `oversample` is 0, 1, 2 or 4 (anything else: WVG_ERR_ARG).  With 0
 * each file takes its own from info.sample_rate: 4 below 96,000, 2 below 192,000, 1 from
 * there on (Annex 2's "4x at 48 kHz, proportionally less above"; libebur128's rule; a DSD
 * file as PCM at 352,800 Hz gets 1).  wvg_true_peak_oversample(rate) reports it.
 *   Filter: 12 taps per phase, as Annex 2's 48-tap filter has; the project's own
 * Hann-windowed sinc (lpw = 6, rolloff 1.0), evaluated in float64.  For quarter-phase q =
 * 0..3 and tap j = 0..11: t = (j - 5) - q/4, h_q[j] = sinc(pi t) * cos^2(pi t / 12) (sinc(0) =
 * 1; 0 for |t| >= 6).  Phase 0 is the identity; for q >= 1, c_q[j] = round-to-nearest(h_q[j] /
 * sum_j h_q[j] * 2^24):
 *     q=0: 0 0 0 0 0 16777216 0 0 0 0 0 0
 *     q=1: -27363 173728 -504882 1159730 -2707526 15032977 4840980 -1734883 775827 -310666 82102 -2808
 *     q=2: -16528 173638 -564942 1343293 -3036105 10489252 10489252 -3036105 1343293 -564942 173638 -16528
 *     q=3: row q=1 reversed
 * Every row sums to exactly 2^24 (DC gain 1); the largest sum of |c| is row 2's, 31,247,516 =
 * 1.8625 * 2^24; no scaled tap is closer than 0.038 to a rounding boundary, so any libm gives
 * these integers.  O = 4 uses rows 0, 1, 2, 3; O = 2 rows 0 and 2; O = 1 row 0.
 *   Outputs: x[m] is the channel's value at frame m for 0 <= m < F, else 0.  For 0 <= n < F
 * and phase index p = 0..O-1 (row q = p * 4/O): y[n][p] = sum_{j=0..11} c_q[j] * x[n - 5 + j],
 * an exact integer in units of 2^-(k+24) of full scale; |y| <= 2^31 * 1.8625 * 2^24 < 2^56 for
 * any int32 input, INT32_MIN included, so no sum leaves int64 in any order.  The interval
 * before frame 0 is not interpolated.
 *   One record per (measurable file, channel):
 *     true_peak          max |y[n][p]|; 0 for no frames
 *     true_peak_pos      n * O + p of the first output that attains it; -1 for no frames
 *     overs              outputs with |y| > 2^(k+24): above 0 dBTP
 *     sample_peak        max |x[m]| (2^31 for INT32_MIN)
 *     sample_peak_frame  first frame that attains it; -1 for no frames
 *     oversample, k      the O used and the depth
 * "First" makes the fold (larger magnitude, then smaller position): associative and
 * commutative, so tile order and butterfly order cannot change a record.  An all-zero
 * channel has peak 0 at position 0.
 *   wvg_batch_true_peak is ordered exactly as wvg_batch_levels: after wvg_batch_decode, on
 * `stream` (NULL: the batch's own) behind the upload and the batch's earlier work, and it
 * returns without waiting (wvg_batch_sync covers it; the next reset / upload waits for it).
 * The records come down with the call into page-locked memory; every partial and record is
 * written by every call; the job tables are built once per upload.  Calls with other
 * `oversample` values may be queued back to back: the last one defines what
 * wvg_batch_file_true_peak returns.  WVG_ERR_ARG before an upload.
 *   wvg_batch_file_true_peak, after wvg_batch_sync: returns C and fills min(C, cap_channels)
 * records; WVG_ERR_OPEN for a file that is not measurable; WVG_ERR_ARG when no
 * wvg_batch_true_peak ran since the last upload.
 *   Host only: wvg_true_peak_taps gives the four rows; wvg_true_peak_tile_frames the frames
 * of one tile for a channel count (1..255); wvg_true_peak_ints runs the kernels' tile and
 * combine code (wv_tpeak.h) on the host over `frames` x `channels` interleaved ints
 * (channels 1..255, k one of 7 / 15 / 23 / 31, oversample 1, 2 or 4): `channels` records at
 * `out`. */
typedef struct {              /* 48 bytes, one per (measurable file, channel) */
    int64_t true_peak;        /* max |y[n][p]|; 0 for no frames */
    int64_t true_peak_pos;    /* n * O + p of the first output that attains it; -1 for no frames */
    int64_t overs;            /* outputs with |y| > 2^(k+24): above 0 dBTP */
    int64_t sample_peak;      /* max |x[m]| (2^31 for INT32_MIN) */
    int64_t sample_peak_frame;/* first frame that attains it; -1 for no frames */
    int32_t oversample;       /* the O used */
    int32_t k;
} wvg_channel_true_peak;

int wvg_batch_true_peak(wvg_batch *b, int oversample, void *stream);
int wvg_batch_file_true_peak(wvg_batch *b, int file, wvg_channel_true_peak *out, int cap_channels);
int wvg_true_peak_taps(int32_t taps[48]);
int wvg_true_peak_oversample(int64_t rate);
int wvg_true_peak_tile_frames(int channels);
int wvg_true_peak_ints(const int32_t *src, int64_t frames, int channels, int k, int oversample,
                       wvg_channel_true_peak *out);

/* ---- Integrated loudness on the device (beyond the reference): ITU-R BS.1770 / EBU R 128
 * programme loudness of every file of a decoded batch -- K-weighting, 400 ms blocks every
 * 100 ms, the absolute and the relative gate -- in float64, 64 bytes per file, with three
 * kernels per batch (wv_loud.hip) and no PCM downloaded.  What ReplayGain 2.0 and dataset
 * normalisation are built on; RMS from wvg_batch_levels has neither the weighting nor the
 * gates.
 *   A file is measurable by levels' rule (it opened, its output is not DSD bytes -- with
 * WVG_OPEN_DSD_AS_PCM a DSD file is measured at k = 23 -- and it is not a float file decoded
 * under WVG_OPEN_EXACT_FLOAT) when also 6,000 <= info.sample_rate <= 3,072,000; other files
 * get WVG_ERR_OPEN and take no room.  Measured is whatever the int32 output holds over
 * info.out_frames frames of C = info.reduced_channels interleaved ints, as format / md5 /
 * planar / levels: a file stopped by an exception has its zeros measured, a
 * WVG_OPEN_ALL_CHANNELS file is measured over its woven N channels.
 *   Filter (float64, designed on the host per distinct rate fs; libebur128's re-derivation
 * of the standard's two biquads, which at 48,000 reproduces BS.1770-4's table to 1e-15):
 *     shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *            K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, d = 1 + K/Q + K^2
 *            b0 = (Vh + Vb K/Q + K^2)/d   b1 = 2 (K^2 - Vh)/d   b2 = (Vh - Vb K/Q + K^2)/d
 *            a1 = 2 (K^2 - 1)/d           a2 = (1 - K/Q + K^2)/d
 *     RLB:   f0 = 38.13547087602444, Q = 0.5003270373238773, K = tan(pi f0 / fs), d = 1 + K/Q + K^2
 *            numerator 1, -2, 1           c1 = 2 (K^2 - 1)/d    c2 = (1 - K/Q + K^2)/d
 *   Per sample v of a channel (transposed direct form II, this order, fma = fused
 * multiply-add), x = (double)v * 2^-k with k as planar's (7, 15, 23, 31; exact):
 *     y1 = fma(b0, x, s1);   s1 = fma(-a1, y1, fma(b1, x, s2));   s2 = fma(-a2, y1, b2 * x);
 *     y2 = y1 + t1;          t1 = fma(-c1, y2, fma(-2.0, y1, t2)); t2 = fma(-c2, y2, y1);
 *     e  = fma(y2, y2, e);
 *   Steps: S = (fs + 5) / 10 frames (100 ms), nsteps = out_frames / S; frames past
 * nsteps * S are never read.  E[c][j] is e after step j's S frames, e = +0.0 at its first.
 *   Runs (how the recursive filter is made parallel; a definition, the same on the host):
 * a run is R = wvg_loudness_run_steps() consecutive steps of one channel, R a build
 * constant.  The run whose first step is j0 starts the recurrence with s1 = s2 = t1 = t2 =
 * +0.0 at frame max(0, j0 - 3) * S and discards the energies of those up to three warm-up
 * steps.  Against the never-restarted filter this leaves out a state that the 38 Hz pole
 * pair has damped over 0.3 s: about 2^-103, far under float64's rounding.
 *   Blocks: N = max(0, nsteps - 3); for 0 <= j < N, P_j = acc / (double)(4 * S) with
 * acc = +0.0 and acc = fma(G_c, ((E[c][j] + E[c][j+1]) + E[c][j+2]) + E[c][j+3], acc) for c
 * ascending.  Weights G_c: all 1.0 for C <= 2; otherwise the channels take the set bits of
 * the file's channel mask (wvg_batch_file_streams) in ascending order, bit 3 (LFE) weighs
 * 0.0, bits 4, 5, 9 and 10 (back and side pairs) 1.41, every other bit and every channel
 * past the mask's bits 1.0.
 *   Gating, in the linear domain (no logarithm in this library): ABS = 0x1.f791ec6e1d5b7p-24
 * (the double nearest 10^((-70 + 0.691) / 10)).  abs_blocks = #{P_j > ABS}, ungated_power =
 * their mean or 0.0 for none; rel = 0.1 * ungated_power; gated_blocks = #{P_j > ABS and
 * P_j > rel}, power = their mean or 0.0 for none; max_block_power = max P_j, 0.0 for N = 0.
 * Each sum over blocks is 64 partial sums (partial l adds P_l, P_(l+64), ... in that order)
 * joined by a butterfly (l with l ^ 32, then ^ 16, ... ^ 1); a mean is sum / (double)count.
 * LUFS = -0.691 + 10 log10(power) is the caller's (api.scan_loudness).
 *   wvg_batch_loudness is ordered exactly as wvg_batch_levels: after wvg_batch_decode, on
 * `stream` (NULL: the batch's own) behind the upload and the batch's earlier work, and it
 * returns without waiting (wvg_batch_sync covers it; the next reset / upload waits for it).
 * The records come down with the call into page-locked memory; tables and coefficients are
 * built once per upload; the block image (every measurable file's P_j, file after file)
 * stays on the device and is overwritten by the next call.  WVG_ERR_ARG before an upload.
 *   wvg_batch_file_loudness, after wvg_batch_sync: WVG_ERR_OPEN for a file that is not
 * measurable, WVG_ERR_ARG when no wvg_batch_loudness ran since the last upload.
 * wvg_batch_loudness_blocks: the doubles of the block image; wvg_batch_download_loudness_blocks
 * waits for the batch's work and copies them (WVG_ERR_SPACE: cap too small).
 *   Host only: wvg_loudness_filter gives b0 b1 b2 a1 a2 c1 c2 and S for a rate (WVG_ERR_ARG
 * outside 6,000 .. 3,072,000); wvg_loudness_weights the G_c (channels 1..255);
 * wvg_loudness_ints runs the kernels' code (wv_loud.h) on the host over `frames` x `channels`
 * interleaved ints and fills the record (block_offset 0) and the N block powers
 * (WVG_ERR_SPACE: cap_blocks < N); wvg_loudness_gate runs the gate over any list of block
 * powers -- an album's, block powers being normalised by their rate -- and fills power,
 * ungated_power, max_block_power and the three counts (the other fields 0). */
typedef struct {              /* 64 bytes, one per measurable file */
    double  power, ungated_power, max_block_power;
    int64_t blocks, abs_blocks, gated_blocks;
    int64_t block_offset;     /* the file's first P_j in the block image */
    int32_t step_frames;      /* S */
    int32_t channels;
} wvg_file_loudness;

int wvg_batch_loudness(wvg_batch *b, void *stream);
int wvg_batch_file_loudness(wvg_batch *b, int file, wvg_file_loudness *out);
int64_t wvg_batch_loudness_blocks(const wvg_batch *b);
int wvg_batch_download_loudness_blocks(wvg_batch *b, double *host, int64_t cap);
int wvg_loudness_filter(int64_t rate, double coef[7], int32_t *step_frames);
int wvg_loudness_weights(int channels, uint32_t channel_mask, double *w);
int wvg_loudness_ints(const int32_t *src, int64_t frames, int channels, int k, int64_t rate, uint32_t channel_mask,
                      wvg_file_loudness *out, double *blocks, int64_t cap_blocks);
int wvg_loudness_gate(const double *blocks, int64_t n, wvg_file_loudness *out);
int wvg_loudness_run_steps(void);

/* ---- Loudness range and short-term loudness on the device (beyond the reference): EBU Tech
 * 3342's loudness range (LRA) and the short-term series it is made from, which with
 * max_block_power (the maximum momentary loudness) complete EBU R 128's descriptors -- 64
 * bytes per file, three more kernels per batch (wv_lra.hip) over the step energies that
 * wvg_batch_loudness leaves on the device, and no PCM or series downloaded.
 *   A file is measurable exactly by loudness's rule; S, nsteps, the weights G_c and the step
 * energies E[c][j] are wvg_batch_loudness's, runs and their restarts included.
 *   Short-term power: a window is 30 steps (3 s), the hop one step (100 ms).  nshort =
 * max(0, nsteps - 29); for 0 <= j < nshort, ST_j = acc / (double)(30 * S) with acc = +0.0
 * and, for c ascending, t = E[c][j], t = t + E[c][j+i] for i = 1 .. 29 ascending, acc =
 * fma(G_c, t, acc).
 *   Gates, in the linear domain, strict > as the integrated gate's: ABS as above.
 * abs_shorts = #{ST_j > ABS}, ungated_short_power = their mean or 0.0 for none, summed as
 * loudness's gate sums (64 partial sums, partial l adds ST_l, ST_(l+64), ... in that order,
 * joined by the butterfly l with l ^ 32, ^ 16, ... ^ 1; mean = sum / (double)count).  rel =
 * 0.01 * ungated_short_power (-20 LU).  The gated multiset G = {ST_j : ST_j > ABS and ST_j >
 * rel}, gated_shorts = n = |G|; max_short_power = max ST_j, 0.0 for nshort = 0.
 *   Percentiles, exact (libebur128's index rule in integers): with g_0 <= ... <= g_(n-1) the
 * sorted G, low_power = g[(n + 4) / 10] and high_power = g[(19 * (n - 1) + 10) / 20], integer
 * divisions, both 0.0 for n = 0.  An order statistic does not depend on how it is found: the
 * device finds both by a radix select over the doubles' bit patterns (no ST_j is negative,
 * so they order as unsigned integers).  LRA = 10 log10(high_power / low_power) LU, the
 * short-term loudness -0.691 + 10 log10(ST_j) LUFS: the caller's (api.scan_loudness).
 *   wvg_batch_loudness_range is ordered exactly as wvg_batch_loudness, and returns without
 * waiting (wvg_batch_sync covers it; the next reset / upload waits for it).  It reads the
 * step energies of a wvg_batch_loudness issued on this batch after the batch's latest
 * wvg_batch_decode; where there is none it issues exactly that call first, on the same
 * stream, and that call's records become readable too.  Every record and every ST_j is
 * written by every call; the short-term image (every measurable file's ST_j, file after
 * file) stays on the device and is overwritten by the next call.  WVG_ERR_ARG before an
 * upload.
 *   wvg_batch_file_loudness_range, after wvg_batch_sync: WVG_ERR_OPEN for a file that is not
 * measurable, WVG_ERR_ARG when no wvg_batch_loudness_range ran since the last upload.
 * wvg_batch_loudness_shorts: the doubles of the short-term image;
 * wvg_batch_download_loudness_shorts waits for the batch's work and copies them
 * (WVG_ERR_SPACE: cap too small).
 *   Host only: wvg_loudness_range_ints runs the kernels' code (wv_loud.h, wv_lra.h) on the
 * host over `frames` x `channels` interleaved ints and fills the record (short_offset 0) and
 * the nshort short-term powers (WVG_ERR_SPACE: cap_shorts < nshort); wvg_loudness_range_gate
 * runs the gates and the selection over any list of short-term powers -- an album's, or
 * values with no audio behind them -- and fills the four powers and the three counts
 * (short_offset 0; WVG_ERR_SPACE for n >= 2^32). */
typedef struct {              /* 64 bytes, one per measurable file */
    double  low_power, high_power, max_short_power, ungated_short_power;
    int64_t shorts, abs_shorts, gated_shorts;
    int64_t short_offset;     /* the file's first ST_j in the short-term image */
} wvg_file_loudness_range;

int wvg_batch_loudness_range(wvg_batch *b, void *stream);
int wvg_batch_file_loudness_range(wvg_batch *b, int file, wvg_file_loudness_range *out);
int64_t wvg_batch_loudness_shorts(const wvg_batch *b);
int wvg_batch_download_loudness_shorts(wvg_batch *b, double *host, int64_t cap);
int wvg_loudness_range_ints(const int32_t *src, int64_t frames, int channels, int k, int64_t rate,
                            uint32_t channel_mask, wvg_file_loudness_range *out, double *shorts, int64_t cap_shorts);
int wvg_loudness_range_gate(const double *shorts, int64_t n, wvg_file_loudness_range *out);

/* WvDemo.Main (WvDemo.cs:15-168) for one file of a formatted batch built with
 * chunk_frames 4096: the .wav bytes it writes (stored RIFF header or the
 * synthesized RIFF/fmt/data headers, the PCM, the stored trailer) and its exit
 * code.  out == NULL queries the length only. */
int wvg_batch_wav(wvg_batch *b, int file, uint8_t *out, int64_t cap, int64_t *wav_len, int32_t *exit_code);

/* ---- Streaming WavpackUnpackSamples (WavPackUtils.cs:200-282) --------------
 * One file opened like WavpackOpenFileInput (WavPackUtils.cs:36-120; NULL when
 * it does not open -- info->error holds the message), then served call by call.
 * The first wvg_stream_unpack decodes the file on the device, its calls
 * scheduled at that call's `samples` (the reference's seams follow the caller's
 * request size; a different size before any frame went out re-decodes, a later
 * one is served from the first schedule and flagged).  Host memory holds the
 * compressed file and two staged windows of `window_frames` frames (0: 262,144);
 * the int32 output stays in HBM.  wvg_stream_unpack returns the frames written
 * to `buffer` (samples x reduced channels ints), 0 at the end, or
 * WVG_ERR_EXCEPTION on the call the reference throws in (the calls before it
 * returned their frames).  wvg_stream_set_sample is SetSample
 * (WavPackUtils.cs:509-594): 1, 0 (false) or WVG_ERR_EXCEPTION.
 * wvg_stream_state: WavpackGetSampleIndex (:355-358), WavpackGetNumErrors
 * (:363-366, counted as each block's last frame is handed out, :273-275),
 * WavpackLossy (:371-374). */
typedef struct wvg_stream wvg_stream;
wvg_stream *wvg_stream_open(wvg_ctx *ctx, const uint8_t *file, size_t len, uint32_t open_flags, int64_t window_frames,
                            wvg_file_info *info);
int64_t wvg_stream_unpack(wvg_stream *s, int32_t *buffer, int64_t samples);
int wvg_stream_set_sample(wvg_stream *s, int64_t sample);
int wvg_stream_state(const wvg_stream *s, int64_t *sample_index, int64_t *crc_errors, int32_t *lossy,
                     int32_t *schedule_changed);
void wvg_stream_close(wvg_stream *s);

#ifdef __cplusplus
}
#endif
#endif
