// wv_framing.h -- host-side framing: .wv file bytes -> device block descriptors.
//
// Restates the part of the reference that runs *around* the hot path:
//   WavpackOpenFileInput   (WavPackUtils.cs:36-120)
//   read_next_header       (WavPackUtils.cs:600-671)
//   unpack_init + readers  (UnpackUtils.cs:24-491, MetadataUtils.cs, WordsUtils.cs:75-187,
//                           FloatUtils.cs:15-30, DsdUtils.cs:17-54,149-242,343-389)
//   the block-walking loop of WavpackUnpackSamples (WavPackUtils.cs:200-282)
//     driven by a caller that asks for `chunk` frames per call (WvDemo.cs:110-135)
// It produces one BlockDesc per decoded block with the exact start state, the
// output offset and the chunk seams.  No sample is decoded here.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "wv_desc.h"
#include "wv_dframe.h"
#include "wv_meta.h"

namespace wvg {

// One stream of a file opened with OPEN_ALL_CHANNELS (a file of more than two channels
// is a sequence of block groups INITIAL_BLOCK .. FINAL_BLOCK, one mono or stereo block
// per stream): its blocks decode into a staging range of their own.
struct McStream {
    int32_t width = 0;      // ints a frame (1 or 2)
    int32_t ch = 0;         // its first channel in the file's frames (sum of the widths before it)
    int64_t stage_off = 0;  // its staging range inside the batch output (ints, a multiple of 4)
    int64_t frames = 0;     // frames it delivers, cut to the file's out_frames
    int64_t first_desc = 0, num_desc = 0;
};

struct FileInfo {
    // WavpackOpenFileInput outcome (WavPackUtils.cs:36-120)
    int32_t open_ok = 0;
    std::string error;  // wpc.error_message (empty when none)
    int32_t num_channels = 0, reduced_channels = 0, bits_per_sample = 0, bytes_per_sample = 0;
    int32_t version = 0, mode = 0, is_float = 0, is_five = 0, file_format = 0;
    int64_t sample_rate = 0, total_samples = -1, config_flags = 0;
    uint32_t dsd_multiplier = 0;
    int32_t lossy_blocks = 0;   // after the whole walk
    int32_t exception = 0;      // framing hit a C# exception; output stops there
    int32_t nondet = 0;
    // output of the chunked caller
    int32_t out_nch = 0;        // ints per frame
    int64_t out_frames = 0;     // frames all calls return
    int64_t first_call_frames = -1;  // frames the first call returns (-1: it threw)
    // output frame counts at which a call returned fewer frames than it asked for (the
    // reference's loop breaks on a header or unpack_init failure, WavPackUtils.cs:215-221;
    // and the file's last call): the stream API ends its calls there too
    std::vector<int64_t> call_cuts;
    int32_t seek_result = 0;    // SetSample: 1 positioned, 0 false, -1 exception (0 when no seek was asked)
    int64_t sample_index0 = 0;  // stream.sample_index when the caller's first (non-discard) call starts
    uint64_t blob_base = 0;     // the file's first byte inside the batch blob (header/trailer offsets are file-relative)
    int64_t header_off = -1, header_len = 0, trailer_off = -1, trailer_len = 0;  // RIFF/ALT header+trailer
    // the stored MD5 of the source audio (ID_MD5_CHECKSUM, 16 bytes; the last one in the
    // file, a trailing zero-sample block's included): its file offset, -1 none.  It is
    // comparable when this decode reproduces the source bytes (lossless, whole, all
    // channels), md5_bps bytes a value.
    int64_t md5_off = -1;
    int32_t md5_comparable = 0, md5_bps = 0;
    // a float file under OPEN_EXACT_FLOAT: its output ints are float32 bit patterns (the
    // fact behind md5_bps = 4; wvg_batch_planar passes them through)
    int32_t exact_float = 0;
    // blocks of this file inside the batch descriptor array
    int64_t first_desc = 0, num_desc = 0;
    // OPEN_ALL_CHANNELS on a file of more than two channels: its streams (empty otherwise;
    // the descriptors are the streams' one after another), the ID_CHANNEL_INFO mask and
    // the end of the staging ranges (an int index of the batch output)
    std::vector<McStream> streams;
    uint32_t channel_mask = 0;
    int64_t mc_end = 0;
    // OPEN_DSD_AS_PCM on a DSD file: its descriptors write the DSD bytes into a staging range
    // [dsd_stage_off, dsd_vis_off) of the batch output (ints; the start a multiple of 4) and
    // its visible range, out_frames x out_nch ints of 24-bit PCM (wv_dsdpcm.h), follows at
    // dsd_vis_off.  "Is this output DSD bytes" is dsd_multiplier > 0 && !dsd_as_pcm.
    int32_t dsd_as_pcm = 0;
    int64_t dsd_stage_off = 0, dsd_vis_off = 0;
    bool dsd_bytes() const { return dsd_multiplier > 0 && !dsd_as_pcm; }
};

// DSD fast/high tables live in a side area (bytes) appended per block.
struct FramingOutput {
    std::vector<ZeroSeg> zeros;   // gap zero-fills (ZeroSeg)
    std::vector<BlockDesc> descs;
    std::vector<uint8_t> tables;  // DSD tables (see BlockDesc::dsd_table_off)
    // defer_values: the decorr weight/sample and entropy/hybrid values are left
    // to meta_apply (wv_meta.h) -- the device parse kernel, or apply_meta_jobs on
    // the host; until then those descriptor fields hold the older stream values
    bool defer_values = false;
    // chain_tables_only: keep the DSD mode-1 tables only for blocks in a decode chain
    // (the device's decode_dsd_chain reads them; every other mode-1 block has its tables
    // built on the device, dsd_fast_tables / wv_dsd1_lane), so a batch does not copy and
    // upload ~2 KB per history bin of every mode-1 block
    bool chain_tables_only = false;
    std::vector<MetaItem> items;  // offsets into the batch blob
    std::vector<MetaJob> jobs;
};

// Host application of the deferred metadata values (what wv_meta_parse does on
// the device); `blob` is the buffer the item offsets point into.
void apply_meta_jobs(FramingOutput &out, const uint8_t *blob);

// Frame one file.  `file` must stay valid until the batch is uploaded.
// `blob_base` is the file's byte offset inside the device blob; descriptors are
// appended to `out` with out_off relative to `out_base_ints`.
// seek_to >= 0: the caller calls SetSample(seek_to) (WavPackUtils.cs:509-594)
// right after opening, and its calls return the frames from there on.
// open_flags & OPEN_ALL_CHANNELS on a file of more than two channels: every stream is
// walked on its own (the reference's OPEN_2CH_MAX walk of a file in which that stream's
// blocks are the INITIAL_BLOCK ones, out_nch = the stream's width) into a staging range
// after the file's visible range of out_frames x num_channels ints; info.streams
// describes them (no seek, no .wvc: the file then does not open).
// open_flags & OPEN_DSD_AS_PCM on a DSD file: the ordinary walk, its descriptors and zero
// fills moved to the next multiple of 4 ints at or after out_base_ints (the staging range),
// the visible range right after everything they write (info.dsd_as_pcm, dsd_stage_off,
// dsd_vis_off; callers pass neither a seek nor a .wvc with it).  Any other file: no change.
// wvc (optional): the file's .wvc correction file, whose bytes start at blob
// offset wvc_base; hybrid blocks then decode exactly (beyond the reference).
void frame_file(const uint8_t *file, size_t len, uint64_t blob_base, uint64_t out_base_ints, uint32_t open_flags,
                int chunk, FramingOutput &out, FileInfo &info, int64_t seek_to = -1, const uint8_t *wvc = nullptr,
                size_t wvc_len = 0, uint64_t wvc_base = 0);

// The stream layout of a file's first block group: each stream's width (ints a frame, as
// the framing counts them: PCM FALSE_STEREO is 2), the ID_CHANNEL_INFO count and mask of
// its first block (0 channels: none stored).  False when no audio block is found or the
// group does not start with INITIAL_BLOCK.
bool probe_streams(const uint8_t *file, size_t len, std::vector<int32_t> &widths, int &num_channels,
                   uint32_t &channel_mask);

// Output ints a batch reserves for a framed file: its reported values
// (out_frames x out_nch) or more when a descriptor writes past them -- a file
// that raised the C# exception mid-call keeps the descriptor of that call,
// whose writes must not reach the next file's range.  A multichannel file's
// extent covers its visible range and its streams' staging.
int64_t file_out_extent(const FramingOutput &out, const FileInfo &info, uint64_t out_base_ints);

// FileInfo of a file framed on the device (wv_dframe.h) from its walk and its
// blocks' records (nblocks of them); false when a block left the device scope
// or the blocks disagree on what they carry (the host frames the file instead).
// first_desc / blob_base are the caller's.
bool dframe_file_info(const DFile &df, const DBlock *blocks, FileInfo &fi);

// WavpackGetMode (WavPackUtils.cs:133-167) from the framed context values
int compute_mode(const FileInfo &info);

}  // namespace wvg
