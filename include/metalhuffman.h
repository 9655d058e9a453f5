/*
 * metalhuffman.h -- C-ABI of the MI355X-native Huffman block decoder.
 *
 * Drop-in boundary for the per-frame decode path of mdejong/MetalHuffman.
 * The reference binds five buffers to its Metal fragment shaders
 * (Shared/AAPLRenderer.m:1233-1253, slot enum Shared/AAPLShaderTypes.h:32-38):
 *   [0] blockStartBitOffsets  u32[NB]             (AAPLRenderer.m:1237, :863-864, :672-685)
 *   [1] huffBuff              u8[codes + 2 pad]   (AAPLRenderer.m:1243, :576-585)
 *   [2] huffSymbolTable1      HuffLookupSymbol[256] (AAPLRenderer.m:1247, :657)
 *   [3] huffSymbolTable2      HuffLookupSymbol[(k+1)*256] (AAPLRenderer.m:1250, :660)
 *   [4] dims uniform          {u16 width, height, blockWidth, blockHeight}
 *                             (AAPLShaderTypes.h:89-95, AAPLRenderer.m:1253, :768-775)
 * mh_decode() takes exactly those buffers (device pointers) and replaces the five
 * huffFragmentShaderB8W12/B8W16 passes, the 16-slice blit and the
 * cropAndGrayscaleFromTexturesFragmentShader reorder (AAPLShaders.metal:127-518,
 * AAPLRenderer.m:1192-1678) with one kernel launch that writes the W x H 8-bit
 * raster directly. The decoded value is the reference output texture's B byte.
 *
 * The producer side (mh_encode_*, mh_build_tables, ...) mirrors the reference's
 * HuffmanUtil statics / Huffman ObjC facade (Shared/HuffmanUtil.hpp:22-100,
 * Shared/Huffman.h:9-77) without module state: every call is reentrant.
 *
 * Conventions: plain pointers and sizes; `stream` is a hipStream_t (NULL = the
 * default stream); device pointers are marked d_. The library never allocates
 * on a decode call; tables are read-only during a decode. Every entry point
 * returns MH_OK (0) or a negative MH_ERR_* code; decode calls never modify the
 * output for a valid stream.
 */
#ifndef METALHUFFMAN_H
#define METALHUFFMAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_VERSION_MAJOR 0
#define MH_VERSION_MINOR 1

/* --- status codes (the reference only asserts: HuffmanEncoder.cpp:131,
 *     AAPLRenderer.m:199,215,721) --------------------------------------- */
#define MH_OK 0
#define MH_ERR_INVALID_ARG (-1)   /* NULL pointer, zero size, bad flags          */
#define MH_ERR_DIMS (-2)          /* dims inconsistent or above the u16 limits   */
#define MH_ERR_CODE_TOO_LONG (-3) /* Huffman depth > 16 (the reference asserts codei < 16;
                                     an encoder given MH_ENCODE_LIMIT_LENGTHS never
                                     reports it: it limits the lengths instead)   */
#define MH_ERR_CAPACITY (-4)      /* caller buffer too small                     */
#define MH_ERR_TABLE (-5)         /* table2 smaller than 256 or not 256-aligned  */
#define MH_ERR_ALIGN (-6)         /* codes not 16-byte aligned / pitch % 8 != 0  */
#define MH_ERR_HIP (-7)           /* HIP runtime error (launch / no device)      */
#define MH_ERR_EMPTY (-8)         /* no symbols to encode                        */
#define MH_ERR_STREAM (-9)        /* a frame's code bits and block offsets disagree: its
                                     report is not 0, 0, 0, 0xFFFFFFFF (mh_check_frames /
                                     mh_check_headers, in the per-frame verdict only)  */

/* --- constants (Shared/AAPLShaderTypes.h:109-123) --------------------- */
#define MH_BLOCK_DIM 8           /* HUFF_BLOCK_DIM                              */
#define MH_TABLE1_NUM_BITS 8     /* HUFF_TABLE1_NUM_BITS                        */
#define MH_TABLE2_NUM_BITS 8     /* HUFF_TABLE2_NUM_BITS                        */
#define MH_TABLE1_SIZE 256       /* HUFF_TABLE1_SIZE                            */
#define MH_TABLE2_SIZE 256       /* HUFF_TABLE2_SIZE (entries per subtable)     */
#define MH_TABLE2_MAX_ENTRIES (257 * 256)
#define MH_MAX_DIM 65535         /* u16 fields of the dims uniform              */
#define MH_CODES_PAD 4           /* zero bytes after the payload: 2 from the
                                    encoder (HuffmanEncoder.cpp:377-378) + 2 from
                                    the renderer (AAPLRenderer.m:576-585)       */

/* decode flags */
#define MH_FLAG_NO_DELTA 0x1u    /* IMPL_DELTAS_BEFORE_HUFF_ENCODING off
                                    (AAPLShaders.metal:263-265): emit symbols raw */
#define MH_FLAG_LANE_PAIRS 0x2u  /* diagnostic only: mh_decode accepts and ignores
                                    it (the default kernels decode; round 5 briefly
                                    returned MH_ERR_INVALID_ARG). The lane-pair kernel
                                    (each block on two lanes -- one from the block
                                    start, one speculatively from its middle bit,
                                    re-synchronised through ds_bpermute; same output;
                                    3.5x slower) is in the
                                    diagnostic library libmh_diag_lanepairs.so, whose
                                    mh_diag_decode_lanepairs takes mh_decode's
                                    arguments */
#define MH_FLAG_ANY_ORDER 0x4u   /* the launch may start before earlier work on
                                    the stream has finished (the AQL dispatch packet
                                    goes out without its barrier bit, HIP's
                                    hipExtAnyOrderLaunch). The caller guarantees that
                                    nothing still running on the stream writes this
                                    call's inputs or touches its output -- e.g. a run
                                    of decodes of resident frames into distinct
                                    rasters, the first of them launched without the
                                    flag. Later work on the stream still waits for it.
                                    Same output. On gfx950 the dispatches still run
                                    one after another (scripts/micro/any_order_probe
                                    .hip); the flag trims ~0.1-0.2 us of the gap
                                    between them */

/* Shared/HuffmanLookupSymbol.h:7-10: 2-byte entry. In T1, bitWidth == 0 marks
 * an escape whose `symbol` is the T2 subtable index (HuffmanUtil.cpp:639-646). */
typedef struct {
  uint8_t symbol;
  uint8_t bitWidth;
} mh_lookup_symbol;

/* Shared/AAPLShaderTypes.h:89-95 RenderTargetDimensionsAndBlockDimensionsUniform,
 * widened to u32 (values must still fit the reference's u16 fields). */
typedef struct {
  uint32_t width;
  uint32_t height;
  uint32_t block_width;  /* ceil(width / 8)  (AAPLRenderer.m:753-761) */
  uint32_t block_height; /* ceil(height / 8) */
} mh_dims;

/* One frame, or a batch of frames of one size that share one table pair (mh_decode)
 * or bring a prepared table each (mh_decode_frames, which ignores the table fields).
 * Frame f's block offsets are d_block_offsets[f*NB .. f*NB+NB) (bit offsets
 * relative to frame f's first code byte); its code bytes start at
 * d_codes + frame_code_offsets[f] (16-byte aligned).
 * Every declared byte must be readable: all codes_bytes bytes at d_codes for one frame
 * without an offset array, and for a batch every byte of every slot
 * [frame_code_offsets[f], frame_code_offsets[f+1]) -- a decode may load anywhere inside
 * them, not only where the frame's codes lie (lanes without a block load near byte
 * 0xFFFFFF00 of a frame that large). Code bytes are addressed with 32 bits per frame: one
 * frame takes codes_bytes <= 0xFFFFFFF0 (more: MH_ERR_CAPACITY); a batch slot may be any
 * size and one over 0xFFFFFFF0 bytes is treated as 0xFFFFFFF0 bytes (bytes behind that read
 * as zero). frame_code_offsets themselves are 64-bit: a batch may lie beyond 4 GiB.
 *
 * Defective streams: a defective frame harms only its own undecodable blocks. This holds for a
 * launch whose tables or headers are valid (incomplete codes, with a Kraft sum below 1, included),
 * in which every frame's block offsets are non-decreasing and at most 8 x the slot's bytes, and
 * every declared byte is readable; the code bytes themselves may be anything.
 * The reference walk of block b is 64 steps from offsets[b] over the slot's bytes -- a step looks
 * up the 16-bit window at its bit position and advances by the entry's width -- where bytes at or
 * past the slot's end read as zero and a zero-width lookup repeats `prev` and does not advance.
 * Block b is SPECIFIED if its walk ends at or before offsets[b + 1]; the frame's last block, if it
 * ends at or before 8 x the slot's bytes. A block whose code bits and offsets are intact is always
 * specified. No margin applies: a tile's staged span runs to its last block's recorded end plus
 * 24 bytes (16 at the slot's end, where zeros follow), and a specified walk's last window ends
 * at most 16 bits past that end.
 *   1. Every pixel of a specified block equals the reference walk's, through every decode entry
 *      and at every scale (a scaled cell lies inside one block).
 *   2. Pixels of unspecified blocks are unspecified, but written only where the entry's contract
 *      lets that block write: write containment holds exactly as for valid streams.
 *   3. No frame, window, crop or plane depends on any other frame's bytes, offsets or table. A
 *      frame that mh_check reports 0, 0, 0, 0xFFFFFFFF decodes exactly, whatever its batch
 *      neighbours hold.
 *   4. mh_check's report is the reference walk's for every frame of ANY input: offsets that run
 *      backwards or point past the slot and a truncated T2 included (see mh_check).
 * The decoders do not walk as mh_check does: they stage a tile's code bytes once, so a block
 * that walks past its recorded end reads whatever the staging window held. That is why such a
 * block is unspecified, and all it costs. */
typedef struct {
  const uint32_t *d_block_offsets;        /* slot [0], u32[n_frames * NB]      */
  const uint8_t *d_codes;                 /* slot [1], 16-byte aligned          */
  uint64_t codes_bytes;                   /* bytes readable at d_codes          */
  const uint64_t *d_frame_code_offsets;   /* u64[n_frames + 1], or NULL when
                                             n_frames == 1 (frame = whole buf) */
  const mh_lookup_symbol *d_table1;       /* slot [2], 256 entries              */
  const mh_lookup_symbol *d_table2;       /* slot [3], table2_entries entries   */
  uint32_t table2_entries;                /* (k+1)*256, k = #subtables          */
  const uint16_t *d_lut;                  /* optional: mh_prepare_lut() output,
                                             NULL = derive it inside the kernel */
  const uint8_t *d_block_init;            /* optional u8[n_frames*NB]: per-block
                                             initial prev symbol
                                             (IMPL_DELTAS_AND_INIT_ZERO_DELTA_...,
                                             AAPLRenderer.m:449-473,
                                             AAPLShaders.metal:324); NULL = 0  */
  mh_dims dims;                           /* slot [4]                           */
  uint32_t n_frames;
  uint32_t flags;                         /* MH_FLAG_*                          */
} mh_frame;

/* ---------------------------------------------------------------------- */
/* GPU decode (the hot path).                                              */

/* Decode n_frames frames into d_out: frame f, row y starts at
 * d_out + f*out_frame_stride + y*out_pitch. round_up(W, 8) bytes of each row
 * y < H are written (the kernel stores whole 8-pixel block rows, so a right-edge
 * block also writes the padding between W and round_up(W, 8)); the rest of the
 * pitch and rows >= H are not touched. out_pitch must be a multiple of 8 and
 * >= W (hence >= round_up(W, 8): rows never overlap).
 * Asynchronous on `stream`; one kernel launch. */
int mh_decode(const mh_frame *frame, uint8_t *d_out, size_t out_pitch,
              size_t out_frame_stride, void *stream);

/* mh_decode with the frame's mid-block marks (mh_encode_frame_marks / mh_mid_marks; device
 * memory, u32[NB], 4-byte aligned -- else MH_ERR_ALIGN with the other alignments; NULL is
 * mh_decode itself). Every check, in mh_decode's order, is mh_decode's, and for valid marks every
 * byte written equals mh_decode's. The marks are used when the launch is one frame with a prepared
 * table (d_lut) and no frame-offset array, small enough for the single-frame kernel, and the marks
 * lie within +-8 GiB of d_block_offsets (they travel as a 32-bit word distance; a producer lays
 * them out beside the offsets): two lanes then decode each block, rows 0-3 from the block's offset
 * and rows 4-7 from the mark, 32 steps each. Every other launch ignores the marks and is
 * mh_decode's. MH_FLAG_NO_DELTA and MH_FLAG_ANY_ORDER as in mh_decode.
 * Marks are not trusted: the bit count is clamped to 512 on the device, so the upper lane reads
 * no further than a 64-step walk from the block's offset could, writes only rows 4-7 of its own
 * block, and a wrong mark spoils those rows alone.
 * Defective streams (mh_frame): item 1 there -- a specified block equals the reference walk -- holds
 * through this entry when the marks are the walk's own, i.e. mh_mid_marks over the code bytes,
 * offsets and tables AS DELIVERED to the decode. A producer's marks describe the bytes it wrote:
 * over bytes damaged since, rows 4-7 of a block start from a point the walk may never reach and
 * may differ from it (rows 0-3 and items 2 and 3 hold for any marks). A consumer that cannot vouch
 * for its stream derives the marks again or calls mh_decode. */
int mh_decode_marked(const mh_frame *frame, const uint32_t *d_mid_marks, uint8_t *d_out, size_t out_pitch,
                     size_t out_frame_stride, void *stream);

/* Debug mode of the decode contract: the reference walk of every block of
 * `frame` (see mh_frame: 64 steps from the block's offset over the real bytes of the frame's slot,
 * one thread per block, zero at or past the slot's end, whatever the offsets are -- NOT the
 * decoders' staged walk, which agrees with it on specified blocks only). An escape at or past
 * table2_entries counts in [1] and as a zero-width lookup in [0]. Writes, per frame f, all four
 * words of u32 d_report[4f..4f+3], whatever they held, and nothing else:
 *   [0] zero-width lookups (windows no code matches -- the reference's {0,0}
 *       entry, HuffmanUtil.cpp:550-556, which repeats prev without advancing),
 *   [1] T1 escapes to a subtable at or past table2_entries (table index > k),
 *   [2] blocks whose 64 codes do not end at the next block's offset (a frame's last block,
 *       whose end is not recorded: blocks whose codes run past the slot's end, bit 8 x the
 *       slot's bytes -- so a frame that reports 0, 0, 0, 0xFFFFFFFF is specified in full),
 *   [3] the first such block (frame relative), or 0xFFFFFFFF.
 * Never writes the raster; valid reference streams report 0, 0, 0, 0xFFFFFFFF.
 * Asynchronous on `stream`. */
int mh_check(const mh_frame *frame, uint32_t *d_report, void *stream);

/* Bytes needed for the derived lookup table mh_prepare_lut() writes. */
size_t mh_lut_bytes(void);

/* Derive the decoder's 2^MH_LUT_BITS-entry first-level table from T1/T2 on the
 * device (one small kernel). Rebuild only when the tables change, exactly as
 * the reference builds T1/T2 once (AAPLRenderer.m:608). The buffer is opaque:
 * write it only through mh_prepare_lut or mh_build_tables_device -- besides the
 * entries it carries facts derived from them (longest / shortest code, whether
 * the code is the identity 8-bit code) that the decode kernels act on. */
int mh_prepare_lut(const mh_lookup_symbol *d_table1, const mh_lookup_symbol *d_table2,
                   uint32_t table2_entries, uint16_t *d_lut, void *stream);

/* Number of LUT index bits used by the kernel (first-level lookup width). */
int mh_lut_bits(void);

/* GPU-side table build from the 256-byte canonical header (the device twin of
 * mh_build_tables: HuffmanUtil.cpp:270-310 parseCanonicalHeader + :338-667
 * generateSplitLookupTables 8/8). Writes T1 (256 entries), T2 through its full
 * MH_TABLE2_MAX_ENTRIES capacity (zero beyond the (k+1)*256 used entries, so
 * mh_decode may be given table2_entries = MH_TABLE2_MAX_ENTRIES), the used entry
 * count to *d_table2_entries, and -- when d_lut is non-NULL -- the prepared
 * table (mh_prepare_lut). d_status (optional, device int32): MH_OK, or
 * MH_ERR_CODE_TOO_LONG / MH_ERR_TABLE (lengths that are not a prefix code), in
 * which case the tables are left zero. All pointers are device pointers;
 * asynchronous on `stream`. Lets a multi-GPU job broadcast 256 bytes. */
int mh_build_tables_device(const uint8_t *d_canon_header, mh_lookup_symbol *d_table1,
                           mh_lookup_symbol *d_table2, uint32_t *d_table2_entries,
                           uint16_t *d_lut, int32_t *d_status, void *stream);

/* ---------------------------------------------------------------------- */
/* Batches with one Huffman table per frame (video, tiles of a scan, whatever  */
/* mh_encode_frames_device_async produced): encode batch -> mh_build_luts_device */
/* -> mh_decode_frames are three asynchronous steps on one stream, no host     */
/* synchronisation in between; mh_decode_headers is the same decode in one     */
/* step, straight from the canonical headers, and mh_stream_create_headers     */
/* streams such frames from host memory; mh_check_frames / mh_check_headers    */
/* are mh_check for such a batch. Not covered: a truncated-T2 report with per- */
/* frame tables, stream groups and the multi-GPU paths with per-frame tables, and an */
/* in-kernel table build from T1/T2 for mh_decode_frames (it needs prepared    */
/* tables). A batch of different frames that should decode under ONE table     */
/* (mh_decode, the fastest route) is encoded by                                */
/* mh_encode_frames_shared_device_async instead.                               */

/* n prepared tables (mh_prepare_lut's buffer) from n 256-byte canonical headers in ONE
 * launch: header i at d_canon_headers + 256 i -> d_luts + i * lut_stride_bytes, byte-identical
 * to what mh_build_tables_device writes to d_lut for that header. d_status[i] (optional) as
 * mh_build_tables_device's d_status; a rejected header leaves the prepared table of all-zero
 * tables. lut_stride_bytes: multiple of 16, >= mh_lut_bytes(). d_luts 16-byte aligned.
 * 1 <= n_headers <= 65535. The launch is sized to about one resident round of the device
 * (clamp(CUs / n_headers, 1, 32) workgroups per header). Asynchronous on `stream`. */
int mh_build_luts_device(const uint8_t *d_canon_headers, uint32_t n_headers, uint16_t *d_luts,
                         uint64_t lut_stride_bytes, int32_t *d_status, void *stream);

/* mh_decode for a batch whose frame f has its own prepared table d_luts + f * lut_stride_bytes.
 * frame->d_table1 / d_table2 / table2_entries / d_lut are ignored (may be NULL / 0).
 * d_frame_status (optional, device int32[n_frames]): a frame whose word is non-zero is not
 * decoded and no byte of its raster is written (the batched encoder's / table build's status
 * array goes here unchanged). Same output contract, alignment rules and error codes as mh_decode
 * (n_frames == 1 with NULL d_frame_code_offsets included), and: NULL d_luts ->
 * MH_ERR_INVALID_ARG; d_luts or lut_stride_bytes not a multiple of 16 -> MH_ERR_ALIGN;
 * lut_stride_bytes < mh_lut_bytes() -> MH_ERR_CAPACITY. flags: MH_FLAG_NO_DELTA |
 * MH_FLAG_ANY_ORDER only (MH_FLAG_LANE_PAIRS -> MH_ERR_INVALID_ARG). One kernel launch of
 * n_frames * G workgroups of 8 waves, G = clamp(ceil(R / n_frames), 1, ceil(tiles / 8)) with R the
 * workgroups resident on the device at once and tiles = ceil(NB / 64); asynchronous. */
int mh_decode_frames(const mh_frame *frame, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                     const int32_t *d_frame_status, uint8_t *d_out, size_t out_pitch,
                     size_t out_frame_stride, void *stream);

/* The launch shape mh_decode_frames would use on `stream`'s device (no launch): workgroups
 * per frame (G above) and waves per workgroup. For tests and tools. */
int mh_decode_frames_shape(const mh_frame *frame, void *stream, uint32_t *groups_per_frame,
                           uint32_t *waves_per_group);

/* mh_decode_frames without the prepared tables: frame f's table comes from its canonical
 * header d_canon_headers + 256 f (device), built in LDS by every workgroup that decodes a
 * slice of the frame -- no mh_build_luts_device launch, no table in memory. Output contract,
 * alignment rules, flag set (MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER), error codes, check order
 * and launch shape rule are mh_decode_frames' (all checks before any HIP call); NULL
 * d_canon_headers -> MH_ERR_INVALID_ARG; frame->d_table1 / d_table2 / table2_entries / d_lut
 * are ignored. d_frame_status (optional input) as in mh_decode_frames: a non-zero word means
 * the frame is not decoded, no byte of its raster is written and its d_header_status word is
 * not written. d_header_status (optional output, device int32[n_frames], must not alias
 * d_frame_status -> MH_ERR_INVALID_ARG): for every frame not skipped, MH_OK,
 * MH_ERR_CODE_TOO_LONG (a length over 16) or MH_ERR_TABLE (Kraft sum over 1), the verdicts of
 * mh_build_tables_device, written by one workgroup of the frame. A rejected header never
 * writes the frame's raster, with or without d_header_status. An incomplete code (Kraft sum
 * under 1, e.g. one symbol) is valid: windows no code matches are the zero-width entry, as in
 * the prepared table. One kernel launch; asynchronous. */
int mh_decode_headers(const mh_frame *frame, const uint8_t *d_canon_headers,
                      const int32_t *d_frame_status, int32_t *d_header_status,
                      uint8_t *d_out, size_t out_pitch, size_t out_frame_stride, void *stream);

/* mh_decode_frames_shape for mh_decode_headers (the same rule with that kernel's occupancy).
 * For tests and tools. */
int mh_decode_headers_shape(const mh_frame *frame, void *stream, uint32_t *groups_per_frame,
                            uint32_t *waves_per_group);

/* mh_check for a batch whose frame f has its own prepared table, by mh_decode_region's table rule:
 * d_luts + f * lut_stride_bytes, lut_stride_bytes == 0 one table for all frames, any other stride a
 * multiple of 16 and >= mh_lut_bytes(). frame->d_table1 / d_table2 / table2_entries / d_lut are
 * ignored. flags: MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER only; neither changes anything (the walk
 * does not depend on the delta, and both launches keep the stream's order), they are accepted so
 * that one mh_frame serves the check and the decode.
 * d_report (required, u32[4 * n_frames], 4-byte aligned): all four words of every frame are
 * written, whatever they held, and nothing else. For a walked frame they are exactly mh_check's
 * words for that frame alone under its own whole tables -- the reference walk of mh_frame's
 * comment, 64 steps from offsets[b] over the slot's real bytes, zero at or past the slot's end, a
 * zero-width lookup not advancing, whatever the offsets are (backwards, equal, past the slot up
 * to 0xFFFFFFFF); sums wrap mod 2^32. Word [1] is always 0: a prepared or header-built table has
 * no truncated T2.
 * d_verdict (optional, int32[n_frames], 4-byte aligned): MH_OK for a frame whose report is 0, 0,
 * 0, 0xFFFFFFFF, MH_ERR_STREAM otherwise. It goes unchanged into d_frame_status of any decode
 * entry on the same stream, no host synchronisation in between.
 * d_frame_status (optional input): a frame whose word is non-zero is not walked; its report is
 * the clean pattern and its verdict is that word, so one array carries the encoder's or the table
 * build's rejections and the stream's into the decode. d_verdict must not alias d_frame_status
 * (MH_ERR_INVALID_ARG: a frame's workgroups read the one while others write the other).
 * All checks before any HIP call, in mh_decode_frames' order with its codes, without the raster
 * rules: the aliasing pairs and NULL d_report -> MH_ERR_INVALID_ARG with the other NULL checks;
 * a misaligned d_report or d_verdict -> MH_ERR_ALIGN with the other alignments. Two launches (a
 * small one that writes the clean reports and the passed-through verdicts, then the walk: n_frames
 * * G workgroups of 8 waves by mh_decode_frames' shape rule with the walk kernel's occupancy);
 * asynchronous, no host synchronisation. */
int mh_check_frames(const mh_frame *frame, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                    const int32_t *d_frame_status, uint32_t *d_report, int32_t *d_verdict, void *stream);

/* mh_check_frames with the tables of mh_decode_headers: frame f's canonical header at
 * d_canon_headers + 256 f, built in LDS. A rejected header is not walked: its report is the clean
 * pattern and its verdict the header's code (MH_ERR_CODE_TOO_LONG / MH_ERR_TABLE).
 * d_header_status (optional output) is written as mh_decode_headers writes it. d_verdict,
 * d_frame_status and d_header_status are pairwise distinct (MH_ERR_INVALID_ARG). Checks in
 * mh_decode_headers' order. */
int mh_check_headers(const mh_frame *frame, const uint8_t *d_canon_headers, const int32_t *d_frame_status,
                     int32_t *d_header_status, uint32_t *d_report, int32_t *d_verdict, void *stream);

/* The launch shape of the walk of mh_check_frames / mh_check_headers on `stream`'s device (no
 * launch): workgroups per frame and waves per workgroup. For tests and tools. */
int mh_check_frames_shape(const mh_frame *frame, void *stream, uint32_t *groups_per_frame,
                          uint32_t *waves_per_group);
int mh_check_headers_shape(const mh_frame *frame, void *stream, uint32_t *groups_per_frame,
                           uint32_t *waves_per_group);

/* ---------------------------------------------------------------------- */
/* A block-aligned region of every frame in one launch. Every block has its own bit offset,  */
/* so the blocks [bx0, bx0 + bw) x [by0, by0 + bh) of the frame's 8x8 grid decode without the */
/* rest of the frame and without a full-size raster: a window of a large scan, a pan of it,   */
/* the same crop of every frame of a sequence. Not covered: regions for mh_decode_headers,    */
/* the streams and the multi-GPU paths; a check of a region alone (a frame's verdict from      */
/* mh_check_frames covers every region of it); pixel-granular stores (a region is whole       */
/* blocks; rectangles at pixel origins are mh_decode_crops below); a CPU twin; packing        */
/* several rows of a region narrower than 64 blocks into one wave (lane utilisation is        */
/* bw / (64 ceil(bw / 64))).                                                                  */
typedef struct {
  uint32_t bx0, by0, bw, bh; /* in 8x8 blocks of the frame's grid */
} mh_region;

/* mh_decode_frames for the region's blocks only. The region's pixel size is
 *   RW = min(W, 8 (bx0 + bw)) - 8 bx0,  RH = min(H, 8 (by0 + bh)) - 8 by0.
 * Output: frame f, region row y starts at d_out + f * out_frame_stride + y * out_pitch; 8 bw
 * (= round_up(RW, 8)) bytes of every row y < RH are written; the rest of the pitch and rows
 * >= RH are not touched. The written bytes equal the same bytes of the rectangle at
 * (8 bx0, 8 by0) of the raster mh_decode_frames writes for that frame; for the region
 * {0, 0, block_width, block_height} the two outputs are byte-identical.
 * Tables: frame f decodes with the prepared table d_luts + f * lut_stride_bytes (from
 * mh_prepare_lut, mh_build_tables_device or mh_build_luts_device). lut_stride_bytes == 0: one
 * table shared by all frames (one scan, one table, many windows); any other stride is a
 * multiple of 16 and >= mh_lut_bytes(). frame->d_table1 / d_table2 / table2_entries / d_lut are
 * ignored. d_frame_status as in mh_decode_frames: a non-zero word means no byte of that frame's
 * region raster is written. d_block_init works as elsewhere, indexed by the frame's block number.
 * Checks: all before any HIP call, in mh_decode_frames' order and with its codes, RW / RH in the
 * place of W / H in the pitch and frame stride rules (out_pitch >= RW, out_frame_stride >=
 * out_pitch * RH); and NULL region -> MH_ERR_INVALID_ARG; bw == 0, bh == 0, bx0 + bw >
 * block_width or by0 + bh > block_height (computed without wrapping) -> MH_ERR_DIMS, with the
 * frame's dims; more than 2^31 - 1 tiles or workgroups -> MH_ERR_CAPACITY. flags:
 * MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER only.
 * One kernel launch, asynchronous on `stream`: a tile is a run of <= 64 consecutive blocks
 * inside one block row of the region (S = ceil(bw / 64) per row, bh * S per frame), and the
 * launch is n_frames * G workgroups of 8 waves, G = clamp(ceil(R / n_frames), 1,
 * ceil(bh * S / 8)), R the workgroups of this kernel resident on the device at once. */
int mh_decode_region(const mh_frame *frame, const mh_region *region, const uint16_t *d_luts,
                     uint64_t lut_stride_bytes, const int32_t *d_frame_status, uint8_t *d_out,
                     size_t out_pitch, size_t out_frame_stride, void *stream);

/* The launch shape mh_decode_region would use on `stream`'s device (no launch): workgroups per
 * frame (G above) and waves per workgroup. For tests and tools. */
int mh_decode_region_shape(const mh_frame *frame, const mh_region *region, void *stream,
                           uint32_t *groups_per_frame, uint32_t *waves_per_group);

/* ---------------------------------------------------------------------- */
/* A region at 1/2, 1/4 or 1/8 scale in one launch: an overview of a large scan, a thumbnail  */
/* strip of a sequence, a pyramid level. One lane decodes one 8x8 block, and a 2x2, 4x4 or    */
/* 8x8 box never crosses a block, so the decoder averages in registers and stores 1/4, 1/16   */
/* or 1/64 of the raster; no full-size raster exists. Not covered: scaling for mh_decode,     */
/* mh_decode_frames and mh_decode_headers (the whole frame is the full region); the streams;  */
/* the multi-GPU paths; scales other than 2, 4 and 8; any filter other than the box.          */

/* mh_decode_region at scale s = 2^log2_scale; c = 8 >> log2_scale is the number of output
 * bytes per block and output row. With RW / RH mh_decode_region's, the scaled size is
 *   SW = ceil(RW / s),  SH = ceil(RH / s).
 * Output: frame f, output row Y starts at d_out + f * out_frame_stride + Y * out_pitch; bw * c
 * (= round_up(SW, c)) bytes of every row Y < SH are written and nothing else is touched.
 * Pixel (X, Y), X < SW: over the region pixels (x, y) with s X <= x < min(s (X + 1), RW) and
 * s Y <= y < min(s (Y + 1), RH) -- n of them, of sum S in the raster mh_decode_region writes --
 * the byte is floor((2 S + n) / (2 n)): the mean of the cell's pixels INSIDE the frame, halves
 * rounded up. An edge block's padding never enters S or n. Bytes at X >= SW (cells of a
 * right-edge block wholly outside the frame) are written as 0. A region starts on a block and s
 * divides 8, so cells are those of the whole frame's grid: a scaled region is the matching
 * rectangle of the scaled whole frame.
 * log2_scale == 0 is mh_decode_region (same checks, same kernel, same bytes); 1, 2, 3 are
 * kernels of their own; > 3 -> MH_ERR_INVALID_ARG, reported where a bad flag is.
 * Tables, d_frame_status, d_block_init and flags: mh_decode_region's.
 * Checks: all before any HIP call, in mh_decode_region's order and with its codes, with SW / SH
 * in the place of RW / RH (out_pitch >= SW, out_frame_stride >= out_pitch * SH) and c in the
 * place of 8 in the alignment rules (d_out, out_pitch and, for n_frames > 1, out_frame_stride
 * are multiples of c; at log2_scale 3 any pitch is legal).
 * One kernel launch, asynchronous; tiles and the launch-shape rule are mh_decode_region's, with
 * this kernel's own occupancy. */
int mh_decode_region_scaled(const mh_frame *frame, const mh_region *region, uint32_t log2_scale,
                            const uint16_t *d_luts, uint64_t lut_stride_bytes,
                            const int32_t *d_frame_status, uint8_t *d_out, size_t out_pitch,
                            size_t out_frame_stride, void *stream);

/* The launch shape mh_decode_region_scaled would use (no launch), as mh_decode_region_shape. */
int mh_decode_region_scaled_shape(const mh_frame *frame, const mh_region *region, uint32_t log2_scale,
                                  void *stream, uint32_t *groups_per_frame, uint32_t *waves_per_group);

/* The CPU twin of that output stage: the same definition applied to a width x height raster in
 * host memory (rows `pitch` bytes apart), writing ceil(width / s) x ceil(height / s) bytes into
 * `out` (rows `out_pitch` apart) and nothing else. log2_scale 0..3; 0 copies.
 * MH_ERR_INVALID_ARG: a NULL pointer, a zero size, log2_scale > 3; MH_ERR_CAPACITY: pitch <
 * width or out_pitch < ceil(width / s). */
int mh_box_reduce(const uint8_t *raster, uint32_t width, uint32_t height, size_t pitch,
                  uint32_t log2_scale, uint8_t *out, size_t out_pitch);

/* ---------------------------------------------------------------------- */
/* A list of windows in one launch: rectangles of one size in blocks, each with its own frame   */
/* and origin -- random crops of a set of scans, the tiles a viewer's cache misses after a     */
/* jump, a tracked box that moves from frame to frame. mh_decode_region decodes the SAME        */
/* rectangle of every frame; N rectangles took N launches of it. Windows at a reduced scale:  */
/* mh_decode_windows_scaled below. Not covered: windows for mh_decode_headers, the streams, the */
/* multi-GPU paths; a check of a window list (mh_check_frames' verdict covers the whole frame); */
/* windows of different sizes in one launch; packing several rows of a window narrower than 64  */
/* blocks into one wave (lane utilisation is bw / (64 ceil(bw / 64)), as for a region);         */
/* pixel-granular stores (windows are whole blocks; mh_decode_crops below takes pixel origins);  */
/* a CPU twin.                                                                                  */
typedef struct {
  uint32_t frame, bx0, by0, reserved; /* 16 bytes; reserved must be 0 */
} mh_window;

/* Window p = d_windows[p] is the blocks [bx0, bx0 + bw) x [by0, by0 + bh) of frame `frame`; its
 * pixel size RW_p x RH_p is mh_decode_region's RW x RH for that rectangle.
 * d_windows is a DEVICE array of n_windows descriptors, 16-byte aligned (a sampler on the GPU can
 * write it; the host never reads it). Windows may overlap, repeat and name frames in any order.
 * Output: window p, row y starts at d_out + p * out_window_stride + y * out_pitch; 8 bw bytes of
 * every row y < RH_p are written; nothing else is touched, in that slot or outside it (rows
 * >= RH_p of a window at the frame's bottom edge keep what they held). The written bytes equal the
 * same bytes of the rectangle at (8 bx0, 8 by0) of the raster mh_decode_frames writes for that frame.
 * Tables, lut_stride_bytes == 0, d_block_init and flags: mh_decode_region's. d_frame_status
 * (optional, device int32[n_frames]) is indexed by the window's FRAME: a non-zero word means no
 * byte of any window of that frame is written.
 * Windows are validated on the device, by the workgroups that serve them and from the descriptor
 * alone: frame >= n_frames, bx0 + bw > block_width, by0 + bh > block_height (compared without
 * wrapping: bx0 = 0xFFFFFFFF is rejected) or reserved != 0 reject the window. A rejected window
 * loads nothing through its descriptor and writes no byte of the raster; the others are decoded.
 * d_window_status (optional output, device int32[n_windows], must not alias d_frame_status ->
 * MH_ERR_INVALID_ARG), written by one workgroup of window p: MH_ERR_DIMS for a rejected window;
 * else its frame's status word when that is non-zero (the slot is then untouched, as above); else
 * MH_OK.
 * Checks: all before any HIP call, in mh_decode_region's order and with its codes, with n_windows
 * rasters of 8 bw x 8 bh in the place of n_frames rasters of RW x RH, and: NULL d_windows or
 * n_windows == 0 -> MH_ERR_INVALID_ARG; bw == 0, bh == 0, bw > block_width or bh > block_height ->
 * MH_ERR_DIMS; d_windows not 16-byte aligned -> MH_ERR_ALIGN; out_pitch < 8 bw (the full block
 * width: windows differ in RW) or, for n_windows > 1, out_window_stride < out_pitch * 8 bh ->
 * MH_ERR_CAPACITY (the window stride is a multiple of 8 as the frame stride is, for n_windows > 1);
 * n_windows * bh * S tiles or the grid above 2^31 - 1 -> MH_ERR_CAPACITY. flags: MH_FLAG_NO_DELTA |
 * MH_FLAG_ANY_ORDER only.
 * One kernel launch, asynchronous on `stream`: tiles are mh_decode_region's (S = ceil(bw / 64) per
 * block row, bh * S per window), and the launch is n_windows * G workgroups of 8 waves, workgroup g
 * serving window g / G, G = clamp(ceil(R / n_windows), 1, ceil(bh * S / 8)), R the workgroups of this
 * kernel resident on the device at once. */
int mh_decode_windows(const mh_frame *frame, const mh_window *d_windows, uint32_t n_windows,
                      uint32_t bw, uint32_t bh, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                      const int32_t *d_frame_status, int32_t *d_window_status, uint8_t *d_out,
                      size_t out_pitch, size_t out_window_stride, void *stream);

/* The launch shape mh_decode_windows would use on `stream`'s device (no launch): workgroups per
 * window (G above) and waves per workgroup. For tests and tools. */
int mh_decode_windows_shape(const mh_frame *frame, uint32_t n_windows, uint32_t bw, uint32_t bh,
                            void *stream, uint32_t *groups_per_window, uint32_t *waves_per_group);

/* ---------------------------------------------------------------------- */
/* A list of windows at 1/2, 1/4 or 1/8 scale in one launch: the tiles a viewer's cache misses  */
/* at pyramid level k, one crop per scan of a thumbnail sheet, multi-scale random crops.        */
/* Not covered: a scale per window; windows clipped at the grid's edge; and what                */
/* mh_decode_windows and mh_decode_region_scaled leave out.                                     */

/* mh_decode_windows at scale s = 2^log2_scale; c = 8 >> log2_scale. Window p is
 * mh_decode_windows' window p, of pixel size RW_p x RH_p; its scaled size is
 *   SW_p = ceil(RW_p / s),  SH_p = ceil(RH_p / s).
 * Output: window p, output row Y starts at d_out + p * out_window_stride + Y * out_pitch; bw * c
 * bytes of every row Y < SH_p are written, those at X >= SW_p as 0; nothing else is touched, in
 * that slot or outside it. Pixel (X, Y), X < SW_p, is mh_decode_region_scaled's: the mean of the
 * cell's pixels inside the frame, floor((2 S + n) / (2 n)). The written bytes equal those
 * mh_decode_region_scaled writes for the region {bx0, by0, bw, bh} of that frame.
 * log2_scale == 0 is mh_decode_windows (same checks, same kernel, same bytes); 1, 2, 3 are kernels
 * of their own; > 3 -> MH_ERR_INVALID_ARG, reported where a bad flag is.
 * d_windows, tables, d_frame_status, d_window_status, the validation of a window on the device and
 * flags: mh_decode_windows'.
 * Checks: all before any HIP call, in mh_decode_windows' order and with its codes, with n_windows
 * rasters of c bw x c bh in the place of 8 bw x 8 bh (out_pitch >= c bw; for n_windows > 1,
 * out_window_stride >= out_pitch * c bh) and c in the place of 8 in the alignment rules (d_out,
 * out_pitch and, for n_windows > 1, out_window_stride are multiples of c; at log2_scale 3 any
 * value is legal).
 * One kernel launch, asynchronous; tiles and the launch-shape rule are mh_decode_windows', with
 * this kernel's own occupancy. */
int mh_decode_windows_scaled(const mh_frame *frame, const mh_window *d_windows, uint32_t n_windows,
                             uint32_t bw, uint32_t bh, uint32_t log2_scale,
                             const uint16_t *d_luts, uint64_t lut_stride_bytes,
                             const int32_t *d_frame_status, int32_t *d_window_status,
                             uint8_t *d_out, size_t out_pitch, size_t out_window_stride, void *stream);

/* The launch shape mh_decode_windows_scaled would use (no launch), as mh_decode_windows_shape. */
int mh_decode_windows_scaled_shape(const mh_frame *frame, uint32_t n_windows, uint32_t bw, uint32_t bh,
                                   uint32_t log2_scale, void *stream,
                                   uint32_t *groups_per_window, uint32_t *waves_per_group);

/* ---------------------------------------------------------------------- */
/* A list of crops at PIXEL origins in one launch: rectangles of one size in pixels, each with   */
/* its own frame and origin, every one stored densely from its own byte 0 -- a batch of random   */
/* crops as one [n, h, w] array, a tracked box that moves by pixels. mh_decode_windows stops at  */
/* the block grid: its caller decoded windows one block larger and viewed rectangle i at its own */
/* (dx, dy) inside slot i, which is no array. Here the decoder moves every row onto the crop's   */
/* byte grid in registers, at the moment it stores it; no intermediate raster exists.            */
/* Not covered: crops at a reduced scale; crops of different sizes in one launch; flips of a byte */
/* output (mh_decode_crops_norm below mirrors as it normalises); crops                            */
/* for mh_decode_headers, the streams and the multi-GPU paths; a check of a crop list            */
/* (mh_check_frames' verdict covers the whole frame); stores of exactly w                        */
/* bytes (a row is written in whole 8-byte words); a CPU twin.                                   */
typedef struct {
  uint32_t frame, x0, y0, reserved; /* 16 bytes; pixels; reserved must be 0 */
} mh_crop;

/* Crop p = d_crops[p] is the pixels [x0, x0 + w) x [y0, y0 + h) of frame `frame`. A crop lies
 * wholly inside the declared W x H: there is no clipping.
 * d_crops is a DEVICE array of n_crops descriptors, 16-byte aligned (a sampler on the GPU can
 * write it; the host never reads it). Crops may overlap, repeat and name frames in any order.
 * Output: crop p, row y starts at d_out + p * out_crop_stride + y * out_pitch; round_up(w, 8)
 * bytes of every row y < h are written. The first w of them are the bytes at (x0 + x, y0 + y) of
 * the raster mh_decode_frames writes for that frame; bytes w .. round_up(w, 8) - 1 are
 * unspecified (as the columns past RW of a region are). Nothing else is touched, in that slot or
 * outside it. For w a multiple of 8 and out_pitch == w the slots are dense rasters.
 * Tables, lut_stride_bytes == 0, d_block_init, d_frame_status (indexed by the crop's FRAME) and
 * flags (MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER only): mh_decode_windows'.
 * Crops are validated on the device as windows are, by the workgroups that serve them and from
 * the descriptor alone, before anything is addressed through it: frame >= n_frames, x0 > W - w,
 * y0 > H - h or reserved != 0 reject the crop. The two limits come from the host, so no sum of
 * descriptor values is formed: x0 = 0xFFFFFFFF is rejected. A rejected crop loads nothing through
 * its descriptor and writes no byte of the raster; the others are decoded.
 * d_crop_status (optional output, device int32[n_crops], must not alias d_frame_status ->
 * MH_ERR_INVALID_ARG) has d_window_status' semantics and precedence: MH_ERR_DIMS for a rejected
 * crop; else its frame's status word when that is non-zero (the slot is then untouched); else MH_OK.
 * Checks: all before any HIP call, in mh_decode_windows' order and with its codes, with n_crops
 * rasters of w x h in the place of n_windows rasters of 8 bw x 8 bh: d_out, out_pitch and, for
 * n_crops > 1, out_crop_stride are multiples of 8 (MH_ERR_ALIGN); out_pitch >= w and, for n_crops
 * > 1, out_crop_stride >= out_pitch * h (MH_ERR_CAPACITY) -- a pitch that is a multiple of 8 and
 * >= w holds the round_up(w, 8) written bytes; NULL d_crops or n_crops == 0 -> MH_ERR_INVALID_ARG;
 * w == 0, h == 0, w > W or h > H -> MH_ERR_DIMS; d_crops not 16-byte aligned -> MH_ERR_ALIGN;
 * n_crops * CBH * S tiles or the grid above 2^31 - 1 -> MH_ERR_CAPACITY.
 * One kernel launch, asynchronous on `stream`. Tiles: with dx = x0 & 7, output word j of a row
 * (8 bytes) is bytes dx..7 of block (x0 >> 3) + j followed by bytes 0..dx-1 of the block after it,
 * so a wave of 64 blocks yields 63 words and tiles step by 63 blocks: OW = ceil(w / 8) words per
 * row, S = ceil(OW / 63) tiles per block row, CBH = (h + 14) / 8 block rows (the most any y0 & 7
 * needs), CBH * S tiles per crop. A crop that needs fewer block rows -- ((y0 & 7) + h + 7) / 8 --
 * skips the rest before loading anything for them. The launch is n_crops * G workgroups of 8
 * waves, workgroup g serving crop g / G, G = clamp(ceil(R / n_crops), 1, ceil(CBH * S / 8)), R the
 * workgroups of this kernel resident on the device at once. */
int mh_decode_crops(const mh_frame *frame, const mh_crop *d_crops, uint32_t n_crops,
                    uint32_t w, uint32_t h, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                    const int32_t *d_frame_status, int32_t *d_crop_status, uint8_t *d_out,
                    size_t out_pitch, size_t out_crop_stride, void *stream);

/* The launch shape mh_decode_crops would use on `stream`'s device (no launch): workgroups per
 * crop (G above) and waves per workgroup. For tests and tools. */
int mh_decode_crops_shape(const mh_frame *frame, uint32_t n_crops, uint32_t w, uint32_t h,
                          void *stream, uint32_t *groups_per_crop, uint32_t *waves_per_group);

/* ---------------------------------------------------------------------- */
/* Crops decoded straight into normalised binary16, bfloat16 or binary32 elements, optionally     */
/* mirrored: what data loaders call crop-mirror-normalize, in the decode launch. The consumer of  */
/* a batch of crops is a model, and no model eats bytes: after mh_decode_crops every caller       */
/* converts, scales and shifts the batch, and flips some samples, each a pass over it. Here the   */
/* decoder does all three on the row it holds in registers, and no byte batch ever exists.        */
/* Not covered: mirrored crops whose width is no multiple of 8; vertical flips; a mirrored byte   */
/* output; a scale or bias per crop (mh_decode_crops_norm_planes below takes one per plane of a   */
/* C-plane image); normalised output for the other entries; a general per-value output table;     */
/* crops at a reduced scale.                                                                      */
#define MH_NORM_F16 0u  /* IEEE binary16 */
#define MH_NORM_BF16 1u /* bfloat16      */
#define MH_NORM_F32 2u
#define MH_CROP_MIRROR 0x1u
typedef struct {
  uint32_t frame, x0, y0, flags; /* 16 bytes; pixels; flags: MH_CROP_MIRROR only */
} mh_norm_crop;

/* mh_decode_crops with elements of E = 2, 2 or 4 bytes (`format`) in the place of bytes. Crop p is
 * the pixels [x0, x0 + w) x [y0, y0 + h) of its frame, wholly inside W x H; everything
 * mh_decode_crops says about descriptors holds (a device array, never read on the host; crops may
 * overlap and repeat).
 * Output: crop p, row y starts at d_out + p * out_crop_stride + y * out_pitch (bytes), element X
 * at + X * E. round_up(w, 8) elements of every row y < h are written: the first w are specified,
 * the rest unspecified. Nothing else is touched, in that slot or outside it.
 * Element (X, y): let v be the byte mh_decode_frames writes at (x0 + X, y0 + y) of that frame --
 * with MH_CROP_MIRROR set, the byte at (x0 + w - 1 - X, y0 + y). The element is T[v] =
 * cvt(fmaf((float)v, scale, bias)): one fused multiply-add in binary32 with a single rounding, then
 * round-to-nearest-even to the format (the identity for MH_NORM_F32). Subnormals are kept, overflow
 * gives +-inf, and finite scale and bias cannot produce a NaN. mh_norm_table below writes T on the
 * host. Normalisation by a mean and a deviation is scale = 1 / (255 * std), bias = -mean / std.
 * Device validation, by the crop's workgroups and before anything is addressed through the
 * descriptor: frame >= n_frames, x0 > W - w, y0 > H - h (limits from the host, no sums of
 * descriptor words), any bit of flags other than MH_CROP_MIRROR, or MH_CROP_MIRROR with w % 8 != 0
 * (a mirrored row would carry its unspecified tail at its front) reject the crop: it loads nothing
 * through its descriptor, writes no byte of the raster and gets MH_ERR_DIMS in d_crop_status[p].
 * Status semantics and precedence, d_frame_status, the aliasing rule, tables, lut_stride_bytes ==
 * 0, d_block_init and flags (MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER only): mh_decode_crops'.
 * Checks: all before any HIP call, in mh_decode_crops' order and with its codes, except: format >
 * 2 or a scale or bias that is not finite -> MH_ERR_INVALID_ARG, reported where a bad flag is;
 * d_out, out_pitch and, for n_crops > 1, out_crop_stride are multiples of 16 (MH_ERR_ALIGN: a row
 * is stored 16 bytes at a time); out_pitch >= round_up(w, 8) * E, the bytes a row is written with
 * (for the 16-bit formats that is every multiple of 16 that is >= w * E), out_pitch <= 2^20 and,
 * for n_crops > 1, out_crop_stride >= out_pitch * h (MH_ERR_CAPACITY).
 * Tiles, CBH, S and the launch-shape rule are mh_decode_crops', with this kernel's occupancy. */
int mh_decode_crops_norm(const mh_frame *frame, const mh_norm_crop *d_crops, uint32_t n_crops,
                         uint32_t w, uint32_t h, uint32_t format, float scale, float bias,
                         const uint16_t *d_luts, uint64_t lut_stride_bytes,
                         const int32_t *d_frame_status, int32_t *d_crop_status,
                         void *d_out, size_t out_pitch, size_t out_crop_stride, void *stream);

/* The launch shape mh_decode_crops_norm would use on `stream`'s device (no launch), as
 * mh_decode_crops_shape; format > 2 -> MH_ERR_INVALID_ARG. */
int mh_decode_crops_norm_shape(const mh_frame *frame, uint32_t n_crops, uint32_t w, uint32_t h,
                               uint32_t format, void *stream,
                               uint32_t *groups_per_crop, uint32_t *waves_per_group);

/* Host: the 256 elements T[0..255] above, 512 or 1024 bytes -- the CPU twin of the kernel's
 * conversion and the contract's reference. NULL table, format > 2 or a scale or bias that is not
 * finite -> MH_ERR_INVALID_ARG; table_bytes below 256 * E -> MH_ERR_CAPACITY. */
int mh_norm_table(uint32_t format, float scale, float bias, void *table, size_t table_bytes);

/* ---------------------------------------------------------------------- */
/* Crops of C-plane images decoded into normalised [n, C, h, w] tensors in one launch. A colour    */
/* image is stored in this format as C grayscale planes, one frame each, and a model takes         */
/* [n, C, h, w] with a mean and a deviation per channel. With mh_decode_crops_norm that is C       */
/* launches, C descriptor arrays that must agree on the origin and the mirror flag, and C pairs;   */
/* at a loader's batch sizes the launches, not the decode work, are the cost. Here a descriptor is */
/* a SAMPLE: its C planes are the same crop of C frames, each under its own (scale, bias).         */
/* Not covered: channels-last output; a pair per crop; vertical flips; crops at a reduced scale; a */
/* byte output with planes (mh_decode_crops already gives planar bytes with C descriptors per      */
/* sample). mh_encode_images_device_async produces such plane frames from interleaved pixels.      */
#define MH_MAX_PLANES 4u

/* mh_decode_crops_norm's contract, with these differences.
 * Sample and planes: descriptor p is one sample. Its plane c (c < n_planes) is the crop [x0, x0 + w)
 * x [y0, y0 + h) of frame `frame + c * plane_frame_stride`; all planes share the origin and the
 * mirror flag. plane_frame_stride is 1 for images stored plane after plane and the number of
 * images for plane-major storage; 0 is legal: one gray frame replicated into C differently
 * normalised channels.
 * Element (c, X, y) is T_c[v], v the byte mh_decode_frames writes at (x0 + X, y0 + y) of that
 * plane's frame -- at (x0 + w - 1 - X, y0 + y) under MH_CROP_MIRROR -- and T_c =
 * mh_norm_table(format, scale[c], bias[c]). scale and bias are HOST arrays of n_planes values each,
 * read during the call and passed by value to the kernel.
 * Output: plane c of sample p, row y starts at d_out + p * out_crop_stride + c * out_plane_stride +
 * y * out_pitch. round_up(w, 8) elements of every row y < h are written, the first w specified, the
 * rest unspecified; nothing else is touched, in or between planes and slots. A dense
 * [n, C, h, round_up(w, 8)] tensor is out_plane_stride = h * out_pitch, out_crop_stride = C * h *
 * out_pitch.
 * Tables: plane c decodes with its own frame's prepared table, d_luts + (frame + c *
 * plane_frame_stride) * lut_stride_bytes; a stride of 0 is one shared table.
 * Device validation, by each of the sample's workgroups, from the descriptor alone and before
 * anything is addressed through it: mh_decode_crops_norm's terms with `frame >= n_frames` replaced
 * by `frame > n_frames - 1 - (n_planes - 1) * plane_frame_stride`. That limit comes from the host,
 * so no sum of descriptor words is formed: frame = 0xFFFFFFFF is rejected. A rejected sample loads
 * nothing through its descriptor, writes no byte of any plane and gets MH_ERR_DIMS in
 * d_crop_status[p].
 * Status: a sample is written whole or not at all. If d_frame_status is given and the word of any
 * of the sample's C frames is non-zero, no byte of any of its planes is written and
 * d_crop_status[p] is the first non-zero word in plane order; otherwise it is MH_OK. The word is
 * written once, by one workgroup of the sample. d_crop_status must not alias d_frame_status.
 * Checks: all before any HIP call, in mh_decode_crops_norm's order and with its codes, plus:
 * n_planes == 0 or > MH_MAX_PLANES, NULL scale or bias, or any of the n_planes values not finite ->
 * MH_ERR_INVALID_ARG, reported where a bad flag or format is (values at index >= n_planes are not
 * read); (n_planes - 1) * plane_frame_stride >= n_frames -> MH_ERR_DIMS, right after the crop-size
 * check; for n_planes > 1, out_plane_stride is a multiple of 16 (MH_ERR_ALIGN, with the other raster
 * alignments) and >= out_pitch * h (MH_ERR_CAPACITY); for n_crops > 1, out_crop_stride >=
 * (n_planes - 1) * out_plane_stride + out_pitch * h (MH_ERR_CAPACITY); n_crops * n_planes * CBH * S
 * tiles or the grid above 2^31 - 1 -> MH_ERR_CAPACITY. With n_planes == 1, plane_frame_stride and
 * out_plane_stride are ignored, and the call accepts and writes exactly what mh_decode_crops_norm
 * does with scale[0], bias[0].
 * One kernel launch of n_crops * n_planes * G workgroups of 8 waves: workgroup g serves unit g / G,
 * which is sample unit / n_planes, plane unit % n_planes. G follows mh_decode_crops' rule with
 * n_crops * n_planes units and this kernel's own occupancy. */
int mh_decode_crops_norm_planes(const mh_frame *frame, const mh_norm_crop *d_crops, uint32_t n_crops,
                                uint32_t w, uint32_t h, uint32_t format,
                                uint32_t n_planes, uint32_t plane_frame_stride,
                                const float *scale, const float *bias,
                                const uint16_t *d_luts, uint64_t lut_stride_bytes,
                                const int32_t *d_frame_status, int32_t *d_crop_status,
                                void *d_out, size_t out_pitch, size_t out_plane_stride,
                                size_t out_crop_stride, void *stream);

/* The launch shape mh_decode_crops_norm_planes would use on `stream`'s device (no launch):
 * workgroups per (sample, plane) unit and waves per workgroup. format > 2, n_planes == 0 or
 * n_planes > MH_MAX_PLANES -> MH_ERR_INVALID_ARG. */
int mh_decode_crops_norm_planes_shape(const mh_frame *frame, uint32_t n_crops, uint32_t w, uint32_t h,
                                      uint32_t format, uint32_t n_planes, void *stream,
                                      uint32_t *groups_per_plane, uint32_t *waves_per_group);

/* ---------------------------------------------------------------------- */
/* Crops from a SET of frames of different sizes in one launch. An mh_frame is a batch of frames   */
/* of one size, and no image dataset is one size: a caller with K sizes kept K batches, sorted     */
/* every sampled batch by size and made K launches into scattered slots of one tensor -- K times   */
/* the cost of a whole batch, since at a loader's batch sizes the launch is the cost. A frame set  */
/* is n frames, each with its own width, height and table; the two entries below decode crops of   */
/* any mix of them in one launch, through the bodies of mh_decode_crops and                        */
/* mh_decode_crops_norm_planes.                                                                    */
/* The frames of a set whole, each at its own size: mh_decode_set_frames, further below.            */
/* Not covered: a set for the region, window and scaled entries; mh_check_frames over a set        */
/* (a caller checks per size group and scatters the verdicts into one d_frame_status); sets in the */
/* streams and the multi-GPU paths. (The set's device producer is mh_encode_set_device_async; what */
/* it does not cover -- a shared table over a set, compaction of the code slots -- is listed there.)*/
typedef struct {
  uint32_t first_block;   /* index of the frame's block 0 in d_block_offsets / d_block_init */
  uint32_t width, height; /* pixels, 1..65535 */
  uint32_t reserved;      /* must be 0 */
} mh_frame_geom;          /* 16 bytes */

/* A set is an mh_frame read under these rules. n_frames frames; frame f is W_f x H_f =
 * d_geoms[f].width x .height pixels and NB_f = ceil(W_f / 8) * ceil(H_f / 8) blocks.
 * d_block_offsets and d_block_init (optional) hold total_blocks entries, frame f's at
 * [first_block_f, first_block_f + NB_f); frames may lie in any order and may share entries.
 * d_frame_code_offsets, d_codes and codes_bytes are as for every batch: frame f's codes are its own
 * 16-byte aligned slot, and its block offsets are bits from that slot's start.
 * dims.width and dims.height carry the LARGEST width and height in the set (1..65535);
 * dims.block_width and dims.block_height are ignored. Table fields and flags are as for
 * mh_decode_crops: the in-frame tables are ignored, MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER only.
 * d_geoms is a DEVICE array of n_frames records, 16-byte aligned, never read on the host. The
 * records are the packer's, not a sampler's; the device checks them all the same, so that a stale
 * or corrupt record cannot move a read outside d_block_offsets or a store outside the crop's slot.
 *
 * mh_decode_set_crops is mh_decode_crops' contract over a set: descriptors (mh_crop), the output
 * layout, what is written and what is unspecified, d_crop_status' semantics and precedence, the
 * aliasing rule, tables addressed by the crop's frame number (d_luts + frame * lut_stride_bytes, 0
 * for one shared table), d_frame_status indexed by the frame number, and the tiles (CBH, S, G) are
 * all that entry's, with W_f x H_f in the place of W x H.
 * Device validation, by each of the crop's workgroups, in this order, each step passing before
 * anything is addressed through what it validates:
 *  1. the descriptor's own words: frame >= n_frames or reserved != 0 reject the crop;
 *  2. only then d_geoms[frame] is loaded: reserved != 0, width or height 0 or above 65535,
 *     NB > total_blocks or first_block > total_blocks - NB (formed in that order: nothing wraps)
 *     reject it;
 *  3. w > W_f or h > H_f reject it; only then x0 > W_f - w or y0 > H_f - h do.
 * A rejected crop gets MH_ERR_DIMS in d_crop_status[p], loads nothing further and writes no byte of
 * the raster; the others are decoded.
 * Checks: all before any HIP call, in mh_decode_crops' order and with its codes, except that w > W
 * and h > H are taken against dims, the set's maxima (a crop larger than its own frame is rejected
 * on the device), plus, reported where a NULL d_crops / its alignment is: NULL d_geoms or
 * total_blocks == 0 -> MH_ERR_INVALID_ARG; d_geoms not 16-byte aligned -> MH_ERR_ALIGN.
 * One kernel launch, asynchronous on `stream`: every workgroup makes one more dependent 16-byte
 * load than mh_decode_crops' (the geometry record, behind the descriptor). */
int mh_decode_set_crops(const mh_frame *frame, const mh_frame_geom *d_geoms, uint32_t total_blocks,
                        const mh_crop *d_crops, uint32_t n_crops, uint32_t w, uint32_t h,
                        const uint16_t *d_luts, uint64_t lut_stride_bytes,
                        const int32_t *d_frame_status, int32_t *d_crop_status, uint8_t *d_out,
                        size_t out_pitch, size_t out_crop_stride, void *stream);

/* The launch shape mh_decode_set_crops would use on `stream`'s device (no launch), as
 * mh_decode_crops_shape with dims the set's maxima: G depends on the crop size and the device only. */
int mh_decode_set_crops_shape(const mh_frame *frame, uint32_t n_crops, uint32_t w, uint32_t h,
                              void *stream, uint32_t *groups_per_crop, uint32_t *waves_per_group);

/* mh_decode_crops_norm_planes' contract over a set (above): its argument list with d_geoms and
 * total_blocks behind `frame`, descriptors of type mh_norm_crop, and with n_planes == 1 the plain
 * normalised crops (mh_decode_crops_norm with scale[0], bias[0]) over a set.
 * Device validation, by each of the sample's workgroups, in this order:
 *  1. the descriptor's words: frame > n_frames - 1 - (n_planes - 1) * plane_frame_stride (from the
 *     host) or a flag bit other than MH_CROP_MIRROR reject the sample;
 *  2. only then the geometry records of ALL the sample's n_planes frames are loaded, each is
 *     judged as in mh_decode_set_crops' step 2, and every plane's (width, height) must equal
 *     plane 0's: a sample is written whole or not at all, so each of its workgroups reaches the
 *     same verdict from the same records;
 *  3. w > W_f or h > H_f; then x0 > W_f - w, y0 > H_f - h, or MH_CROP_MIRROR with w % 8 != 0.
 * A rejected sample gets MH_ERR_DIMS in d_crop_status[p] and no byte of any of its planes is
 * written. Status words, precedence and everything else: mh_decode_crops_norm_planes'.
 * Checks: that entry's, with the differences and additions listed for mh_decode_set_crops. */
int mh_decode_set_crops_norm_planes(const mh_frame *frame, const mh_frame_geom *d_geoms,
                                    uint32_t total_blocks, const mh_norm_crop *d_crops, uint32_t n_crops,
                                    uint32_t w, uint32_t h, uint32_t format,
                                    uint32_t n_planes, uint32_t plane_frame_stride,
                                    const float *scale, const float *bias,
                                    const uint16_t *d_luts, uint64_t lut_stride_bytes,
                                    const int32_t *d_frame_status, int32_t *d_crop_status,
                                    void *d_out, size_t out_pitch, size_t out_plane_stride,
                                    size_t out_crop_stride, void *stream);

/* The launch shape mh_decode_set_crops_norm_planes would use (no launch), as
 * mh_decode_crops_norm_planes_shape with dims the set's maxima. */
int mh_decode_set_crops_norm_planes_shape(const mh_frame *frame, uint32_t n_crops, uint32_t w, uint32_t h,
                                          uint32_t format, uint32_t n_planes, void *stream,
                                          uint32_t *groups_per_plane, uint32_t *waves_per_group);

/* ---------------------------------------------------------------------- */
/* Every frame of a set WHOLE, each at its own size into its own raster, in one launch: the       */
/* consumer that closes encode set -> tables -> decode without regrouping the frames by size into  */
/* K mh_frame batches (K mh_decode_frames launches; n when every size differs).                    */
/* The frames differ in size, so neither one pitch nor one workgroup count fits them all: frame    */
/* f's raster and its share of the launch are two more 16-byte device records beside its           */
/* mh_frame_geom, and a group map gives every workgroup of the launch its frame. All three come    */
/* from mh_decode_set_plan (pure host code) or from the caller; the device validates every record  */
/* before anything is addressed through it, as every set record.                                   */
typedef struct {
  uint64_t offset;      /* bytes from d_out to the frame's row 0; multiple of 8                    */
  uint32_t pitch;       /* bytes per raster row; multiple of 8, >= round_up(W_f, 8), <= 2^20       */
  uint32_t reserved;    /* must be 0                                                               */
} mh_set_raster;        /* 16 bytes: where frame f is written */

typedef struct {
  uint32_t first_group; /* index of the frame's first workgroup in the launch                      */
  uint32_t groups;      /* workgroups that share the frame, 1..2^20                                */
  uint32_t reserved[2]; /* must be 0                                                               */
} mh_set_share;         /* 16 bytes: how frame f's tiles are shared out. The slice count of a frame
                           lives in this one record: its workgroups cannot disagree about it. */

#define MH_DECODE_GROUP_WAVES 8 /* waves of a workgroup of the frame-slice kernels: each decodes a tile */

/* `frame` is a set (the rules above mh_decode_set_crops: dims the maxima, d_frame_code_offsets,
 * tables by frame number with lut_stride_bytes 0 for one shared table, MH_FLAG_NO_DELTA |
 * MH_FLAG_ANY_ORDER only). Frame f is written as mh_decode_frames writes a frame: only rows
 * y < H_f, and round_up(W_f, 8) bytes of each, at d_out + offset_f + y * pitch_f, bit-exact to
 * mh_decode_frame_cpu; the rest of the pitch and every other byte of d_out are not touched.
 * d_group_frame: device u32[n_groups]; the launch has n_groups workgroups of
 * MH_DECODE_GROUP_WAVES waves, and workgroup g serves frame d_group_frame[g] as slice
 * g - first_group of its `groups`: wave w of slice j decodes the frame's tiles j * 8 + w,
 * + groups * 8, ... -- a tile is 64 consecutive blocks of the frame in block order, counted from
 * the frame's own block 0, so every lane of every tile but a frame's last holds a block whatever
 * the width.
 * Device validation, by workgroup g, in this order, each step passing before anything is addressed
 * through what it validates:
 *  1. the group map: d_group_frame[g] >= n_frames -> the workgroup returns and writes nothing;
 *  2. the frame's three records (they depend on f alone: two dependent trips, as the set crops'):
 *     share: reserved != 0, groups == 0 or above 2^20, g < first_group or g - first_group >= groups
 *       -> the workgroup returns and writes nothing: it is not one of the frame's. The share is
 *       judged ahead of the other two records because it says which workgroup is the frame's slice
 *       0, the writer of d_set_status[f]: a frame whose share AND geometry (or raster) are bad
 *       reports nothing, not MH_ERR_DIMS;
 *     geometry: judged exactly as mh_decode_set_crops' step 2 -> MH_ERR_DIMS;
 *     raster: reserved != 0, offset % 8 != 0, pitch % 8 != 0, pitch < round_up(W_f, 8), pitch above
 *       2^20 (every entry's pitch limit), or offset + (H_f - 1) * pitch + round_up(W_f, 8) >
 *       out_bytes (formed so that nothing wraps) -> MH_ERR_CAPACITY;
 *  3. d_frame_status[f] != 0 (optional input) skips the frame, as in every decode entry.
 * No byte of a rejected or skipped frame's raster is written, and the other frames are decoded.
 * d_set_status (optional, device int32[n_frames], must not alias d_frame_status ->
 * MH_ERR_INVALID_ARG): one thread of the frame's slice 0 writes d_set_status[f] with a vector
 * store: MH_OK, MH_ERR_DIMS, MH_ERR_CAPACITY, or the frame's non-zero status word. A word whose
 * slice-0 workgroup never arrives (a corrupt map or share) is left as the caller set it.
 * A stale or corrupt record may lose or repeat tiles of its own frame. It never moves a load
 * outside d_block_offsets / d_block_init / d_geoms nor a store outside [d_out, d_out + out_bytes).
 * Rasters that overlap are the caller's business: the planner's never do.
 * Checks, all before any HIP call, in mh_decode_set_crops' order and with its codes:
 * MH_ERR_INVALID_ARG: d_set_status == d_frame_status; NULL frame, d_out, d_block_offsets, d_codes,
 * d_geoms, d_rasters, d_shares, d_group_frame, d_luts; total_blocks, n_groups or out_bytes 0;
 * n_groups above 2^31 - 1; n_frames 0 or n_frames > 1 without d_frame_code_offsets; a flag outside
 * the two. MH_ERR_DIMS: dims' maxima outside 1..65535. MH_ERR_ALIGN: d_codes, d_luts,
 * lut_stride_bytes or a record array not 16-byte aligned; d_group_frame not 4-byte aligned; d_out
 * not 8-byte aligned. MH_ERR_CAPACITY: codes_bytes < MH_CODES_PAD; lut_stride_bytes neither 0 nor
 * >= mh_lut_bytes(). One kernel launch, asynchronous on `stream`. */
int mh_decode_set_frames(const mh_frame *frame, const mh_frame_geom *d_geoms, uint32_t total_blocks,
                         const mh_set_raster *d_rasters, const mh_set_share *d_shares,
                         const uint32_t *d_group_frame, uint32_t n_groups,
                         const uint16_t *d_luts, uint64_t lut_stride_bytes,
                         const int32_t *d_frame_status, int32_t *d_set_status,
                         uint8_t *d_out, uint64_t out_bytes, void *stream);

/* The planner's budget on `stream`'s device (no launch): the workgroups of the kernel resident on
 * the device at once (CUs x the kernel's occupancy, the R of mh_decode_frames' shape rule) and the
 * waves per workgroup. Only frame->flags is read (MH_FLAG_NO_DELTA selects the kernel). */
int mh_decode_set_frames_shape(const mh_frame *frame, void *stream,
                               uint32_t *resident_groups, uint32_t *waves_per_group);

/* The records and the group map for mh_decode_set_frames from the host copy of the geometry
 * records. Pure host code: no HIP, callable without a GPU.
 * Rasters: dense, in frame order; with A = max(8, pitch_align), pitch_f = round_up(W_f, A) and
 * every offset is rounded up to A; *out_bytes is the end of the last raster (offset + H * pitch).
 * pitch_align: 0 or a power of two <= 4096.
 * Groups: with tiles_f = ceil(NB_f / 64) and cap_f = ceil(tiles_f / MH_DECODE_GROUP_WAVES),
 *   groups_f = clamp(round(group_budget * tiles_f / sum of tiles), 1, cap_f)   (half rounds up),
 * so a budget of one resident round (mh_decode_set_frames_shape) gives each frame workgroups in
 * proportion to its work, and no workgroup is left without a tile. first_group is the running
 * sum; the map names frame f for groups_f consecutive workgroups; *n_groups is the sum.
 * MH_ERR_INVALID_ARG: NULL h_geoms, n_groups or out_bytes; n_frames == 0; group_budget == 0; a
 * bad pitch_align; group_capacity != 0 with a NULL output array. MH_ERR_DIMS: a record with
 * reserved != 0, a width or height outside 1..65535, first_block + NB_f above 2^32, more than
 * 2^31 - 1 workgroups, or a byte total above 2^64 - 1. MH_ERR_CAPACITY: group_capacity <
 * *n_groups; *n_groups and *out_bytes are reported and no array is written, so a first call with
 * capacity 0 (the three output arrays may then be NULL) sizes them. */
int mh_decode_set_plan(uint32_t n_frames, const mh_frame_geom *h_geoms, uint32_t group_budget,
                       uint32_t pitch_align, mh_set_raster *h_rasters, mh_set_share *h_shares,
                       uint32_t *h_group_frame, uint32_t group_capacity,
                       uint32_t *n_groups, uint64_t *out_bytes);

/* For tests and tools: the table mh_decode_headers builds in LDS, copied out. One workgroup per
 * header runs the same builder and writes the 13-bit table (the first 18,464 bytes of a
 * prepared table) and the 16-byte lengths word at their prepared-table offsets in
 * d_luts + i * lut_stride_bytes, byte-identical to mh_build_luts_device's there; every other
 * byte of the slot is left untouched. A rejected header writes a zero table and the lengths
 * word of an all-zero table (as mh_build_luts_device does), plus its status. Argument rules:
 * mh_build_luts_device's. */
int mh_header_luts_device(const uint8_t *d_canon_headers, uint32_t n_headers, uint16_t *d_luts,
                          uint64_t lut_stride_bytes, int32_t *d_status, void *stream);

/* ---------------------------------------------------------------------- */
/* GPU encoder (the producer side on the device; output byte-identical to   */
/* mh_encode_frame: HuffmanEncoder.cpp:310-381, HuffmanUtil.cpp:1051-1131,  */
/* AAPLRenderer.m:374-688).                                                 */

/* Device workspace mh_encode_frame_device / _async need for a width x height
 * frame (the larger figure, the synchronous call's). */
size_t mh_encode_workspace_bytes(uint32_t width, uint32_t height);

/* Encode the device frame d_gray (W x H bytes, row stride W) without a host
 * synchronisation: block split, deltas (unless MH_FLAG_NO_DELTA) and histogram,
 * the reference's Huffman tree (HuffmanEncoder.cpp:29-145, same tie-breaking as
 * mh_code_lengths) and canonical codes on one workgroup, block offsets (a prefix
 * sum of per-block bit lengths) and MSB-first bit packing, all on `stream`.
 * Writes d_canon_header (device u8[256]), d_codes (4-byte aligned; the byte
 * count is payload + MH_CODES_PAD zero bytes), *d_codes_len (device u64,
 * optional), d_block_offsets (u32[NB]) and, if non-NULL, d_block_init (u8[NB],
 * the IMPL_DELTAS_AND_INIT_ZERO_DELTA variant). *d_status (device int32,
 * optional) becomes MH_OK, MH_ERR_EMPTY, MH_ERR_CODE_TOO_LONG (depth > 16, unless
 * MH_ENCODE_LIMIT_LENGTHS is set: then the tree workgroup limits the lengths) or
 * MH_ERR_CAPACITY (round_up(codes_len, 4) > codes_cap, or >= 2^32 code bits);
 * on an error no code bytes or offsets are written, *d_codes_len is 0 and the
 * header's content is unspecified; d_block_init is then UNSPECIFIED too (the split
 * writes it before the verdict exists: the tests see it written).
 * What is written of d_codes: bytes [0, round_up(codes_len, 4)) and nothing behind
 * them, whatever codes_cap -- the last code word is stored whole, so the up to three
 * bytes [codes_len, round_up(codes_len, 4)) are written, as zero in every encoder
 * here (tests/encode_helpers.py checks the bytes behind them, not their value).
 * codes_cap counts as it stands: one that is no multiple of 4 and lies below
 * round_up(codes_len, 4) is MH_ERR_CAPACITY even where codes_len itself would fit.
 * d_gray needs no alignment (8-byte aligned frames of W % 8 == 0 take wider loads);
 * d_canon_header and d_block_init none, d_block_offsets and d_status 4, d_codes_len 8.
 * d_workspace: 256-byte aligned, mh_encode_workspace_bytes(). The return value
 * covers only argument checks and launch errors. A frame encoded this way goes to
 * mh_build_tables_device (the header) and mh_decode without touching the host.
 * Every call leaves the workspace's symbol histogram zeroed; a caller that
 * zero-filled the workspace once before its first use may pass
 * MH_ENCODE_WORKSPACE_ZEROED in `flags` to skip the per-call clear (one memset
 * launch, ~2 us of a ~33 us frame). */
#define MH_ENCODE_WORKSPACE_ZEROED 0x100u
/* Encoder-only flag (mh_encode_frame, mh_encode_frame_device[_async],
 * mh_encode_frames_device_async; every mh_decode* refuses it): never reject a frame
 * for its tree's depth. The reference tree is built as always; if no leaf is deeper
 * than 16 the output is byte-identical to the unflagged call. Only a deeper tree has
 * its lengths replaced by the optimal code of at most 16 bits
 * (mh_code_lengths_limited(freq, 16, ...): package-merge, host and device byte for
 * byte the same), and the status is MH_OK where it was MH_ERR_CODE_TOO_LONG. The
 * decoders need nothing: they work from the 256 lengths alone. */
#define MH_ENCODE_LIMIT_LENGTHS 0x200u
int mh_encode_frame_device_async(const uint8_t *d_gray, uint32_t width, uint32_t height, uint32_t flags,
                                 uint8_t *d_canon_header, uint8_t *d_codes, uint64_t codes_cap,
                                 uint64_t *d_codes_len, uint32_t *d_block_offsets, uint8_t *d_block_init,
                                 int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);

/* mh_encode_frame_device_async, then one copy and one synchronisation of
 * `stream` to return canon_header and *codes_len on the host; the device status
 * becomes the return value (output byte-identical to mh_encode_frame:
 * HuffmanEncoder.cpp:310-381, HuffmanUtil.cpp:1051-1131, AAPLRenderer.m:374-688). */
int mh_encode_frame_device(const uint8_t *d_gray, uint32_t width, uint32_t height, uint32_t flags,
                           uint8_t canon_header[256], uint8_t *d_codes, uint64_t codes_cap,
                           uint64_t *codes_len, uint32_t *d_block_offsets, uint8_t *d_block_init,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* Device workspace mh_encode_frames_device_async needs for n_frames frames of
 * width x height. */
size_t mh_encode_frames_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_frames);

/* Batched GPU encode: n_frames independent frames of one size (frame f's pixels at
 * d_gray + f * gray_frame_stride, rows of W bytes), each with its OWN histogram,
 * Huffman tree, canonical header and codes -- byte-identical, frame by frame, to
 * mh_encode_frame (HuffmanEncoder.cpp:310-381, HuffmanUtil.cpp:1051-1131) -- in
 * three launches whatever n_frames (tiled split; one tree workgroup per frame, which
 * also turns the frame's per-tile symbol counts into tile bit offsets; packing), so
 * frames no longer queue behind one workgroup's tree each. Outputs, per frame f:
 * d_canon_headers + 256 f, codes at d_codes + f * codes_frame_stride (16-byte
 * aligned slots; the slot size is the capacity), d_codes_len[f] (optional),
 * d_block_offsets + f * NB, d_block_init + f * NB (optional), d_status[f]
 * (optional; the values of mh_encode_frame_device_async), and d_frame_code_offsets
 * (optional, n_frames + 1 u64 = f * codes_frame_stride): the slots are then one
 * mh_frame batch: for mh_decode_frames with one table per frame (mh_build_luts_device over
 * d_canon_headers; d_status goes in as d_frame_status), or for mh_decode when all frames
 * happen to share one canonical table (block shuffles of one image). A rejected frame writes
 * no codes or offsets and does not affect the others; its d_block_init slice is UNSPECIFIED
 * (written by the split before the verdict exists). Of an accepted frame's slot the bytes
 * [0, round_up(codes_len, 4)) are written ([codes_len, ..) as zero) and nothing behind them, so
 * a slot of exactly round_up(codes_len, 4) rounded up to 16 bytes lies flush against the next.
 * gray_frame_stride: any value >= W * H (padding between frames is never read), and any value
 * at all for n_frames == 1; below W * H with n_frames > 1 -> MH_ERR_CAPACITY before any launch.
 * d_gray and the stride need no alignment (frames that are all 8-byte aligned, with W % 8 == 0,
 * take 8-byte loads, and 16-byte ones for an even width in blocks). d_workspace: 256-byte aligned,
 * mh_encode_frames_workspace_bytes(), any content (every part is written before it
 * is read within the call; MH_ENCODE_WORKSPACE_ZEROED is accepted and changes nothing).
 * Asynchronous on `stream`; the return value covers argument checks and launches. */
int mh_encode_frames_device_async(const uint8_t *d_gray, uint64_t gray_frame_stride, uint32_t n_frames,
                                  uint32_t width, uint32_t height, uint32_t flags, uint8_t *d_canon_headers,
                                  uint8_t *d_codes, uint64_t codes_frame_stride, uint64_t *d_codes_len,
                                  uint64_t *d_frame_code_offsets, uint32_t *d_block_offsets, uint8_t *d_block_init,
                                  int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);

/* Device workspace mh_encode_frames_shared_device_async needs for n_frames frames of
 * width x height (mh_encode_frames_workspace_bytes' plus the one table's state). */
size_t mh_encode_frames_shared_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_frames);

/* Batched GPU encode under ONE Huffman table: the producer of what mh_decode, the
 * table-mode streams and the multi-GPU paths consume (n frames, one 256-byte canonical
 * header). Two modes:
 *   built (d_canon_in == NULL): one histogram over all n frames' symbols, one tree, one
 *     header -- mh_code_lengths of the summed histogram (the reference tree and its
 *     tie-breaking) or, with MH_ENCODE_LIMIT_LENGTHS and a tree deeper than 16,
 *     mh_code_lengths_limited(sum, 16, ...) -- written to d_canon_header (required);
 *   supplied (d_canon_in != NULL, device u8[256]): no histogram reduction and no tree; the
 *     caller's lengths are validated and turned into mh_canonical_codes' codes (a header
 *     fixed for a sequence, an earlier batch's, one broadcast to several GPUs before they
 *     encode). d_canon_header is then optional and receives a copy (it may alias
 *     d_canon_in). MH_ENCODE_LIMIT_LENGTHS is ignored.
 * Every frame is packed with that header's codes. Frame layout, slots (16-byte aligned,
 * the slot size is the capacity), d_frame_code_offsets, d_block_init, alignment and the
 * argument checks and their order are mh_encode_frames_device_async's, plus: NULL
 * d_canon_in AND NULL d_canon_header -> MH_ERR_INVALID_ARG (with the other NULL checks);
 * built mode with n_frames * NB * 64 >= 2^32 symbols -> MH_ERR_CAPACITY (ahead of the
 * workspace check; the tree's node weights are 32-bit: 1,365 frames of 2048 x 1536 fit).
 * The batch's total code bits are not limited; one frame's are (u32 block offsets). All
 * checks come before any HIP call. flags: MH_FLAG_NO_DELTA | MH_ENCODE_WORKSPACE_ZEROED |
 * MH_ENCODE_LIMIT_LENGTHS.
 * *d_header_status (device int32, optional), the header's verdict: MH_OK;
 * MH_ERR_CODE_TOO_LONG (the built tree is deeper than 16 without MH_ENCODE_LIMIT_LENGTHS,
 * or a supplied length is over 16); MH_ERR_TABLE (a supplied header whose Kraft sum
 * exceeds 1). A supplied header with a Kraft sum under 1 -- an incomplete code, e.g. one
 * symbol of length 1 -- is valid, as it is for every decoder here.
 * d_status[f] (device int32[n_frames], optional), first match: the header's verdict when
 * that is not MH_OK (every frame); MH_ERR_TABLE when frame f contains a symbol to which
 * the header gives length 0 (supplied mode only); MH_ERR_CAPACITY when
 * round_up(codes_len, 4) > codes_frame_stride or the frame alone has >= 2^32 code bits;
 * MH_OK. A rejected frame writes no code byte and no block offset, its d_codes_len[f] is
 * 0 and it does not disturb the other frames; its d_block_init slice is UNSPECIFIED (the
 * split writes it before the verdict exists). On a rejected header in built mode the
 * content of d_canon_header is unspecified, as in the other encoders.
 * For every accepted frame, the codes (payload + MH_CODES_PAD zero bytes), d_codes_len[f]
 * and the block offsets are byte for byte mh_encode_frame_with_header's for that frame and
 * header.
 * Launches, whatever n_frames: five kernels in built mode (tiled split, histogram
 * reduction over frames, one tree workgroup, one plan workgroup per frame, packing), four
 * in supplied mode (split, header -> code table, plan, packing); the split and the packer
 * are mh_encode_frames_device_async's. d_workspace: 256-byte aligned,
 * mh_encode_frames_shared_workspace_bytes(), any content: built mode clears the batch
 * histogram (16 KB, one memset ahead of the kernels) unless MH_ENCODE_WORKSPACE_ZEROED
 * says the caller zero-filled the workspace once before its first use -- every call
 * leaves the histogram zeroed, as mh_encode_frame_device_async does. Asynchronous on
 * `stream`, no host synchronisation; the return value covers argument checks and
 * launches. The outputs go to mh_build_tables_device (d_canon_header) and mh_decode
 * without touching the host. */
int mh_encode_frames_shared_device_async(
    const uint8_t *d_gray, uint64_t gray_frame_stride, uint32_t n_frames,
    uint32_t width, uint32_t height, uint32_t flags,
    const uint8_t *d_canon_in,     /* device u8[256], or NULL = build the header from the batch */
    uint8_t *d_canon_header,       /* device u8[256] out: the header the frames were encoded with;
                                      required when d_canon_in is NULL, optional (a copy; may alias
                                      d_canon_in) otherwise */
    uint8_t *d_codes, uint64_t codes_frame_stride, uint64_t *d_codes_len,
    uint64_t *d_frame_code_offsets, uint32_t *d_block_offsets, uint8_t *d_block_init,
    int32_t *d_status,             /* optional, int32[n_frames] */
    int32_t *d_header_status,      /* optional, one int32: the header's verdict */
    void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* Interleaved, pitched images encoded straight into C-plane frames: the producer of what     */
/* mh_decode_crops_norm_planes consumes. Decoders, capture APIs and image tensors hand over    */
/* [H, W, K] pixels, often with a row pitch above W * K or as a window of a larger picture;     */
/* these entries read that layout in place -- no transposed copy, no second buffer -- and       */
/* write one frame per taken plane, each byte for byte the host codec's for that plane.        */
typedef struct {
  uint64_t image_stride;   /* bytes from image i to image i + 1                       */
  uint64_t row_pitch;      /* bytes from row y to row y + 1                           */
  uint32_t pixel_stride;   /* bytes from pixel x to pixel x + 1 (3 = RGB, 4 = RGBA..) */
  uint32_t first_channel;  /* plane c is byte first_channel + c of every pixel        */
  uint32_t n_planes;       /* C, 1..MH_MAX_PLANES                                     */
  uint32_t plane_major;    /* 0: frame = i*C + c   (plane_frame_stride 1 on decode)   */
                           /* 1: frame = c*n + i   (plane_frame_stride n_images)      */
} mh_image_layout;

/* The kernels address one tile of 256 blocks through one 32-bit descriptor that starts at the
 * tile's first pixel row. A tile lies in at most MH_IMAGE_TILE_ROWS(width) rows, so a layout
 * is addressable when
 *   (min(height, MH_IMAGE_TILE_ROWS(width)) - 1) * row_pitch + width * pixel_stride
 *     <= MH_IMAGE_TILE_SPAN_MAX
 * (16 rows for widths of 2,033 and more, 2,048 rows for widths up to 8). */
#define MH_IMAGE_TILE_SPAN_MAX 0x7FFFFFF0ull
#define MH_IMAGE_TILE_ROWS(width) (8u * (254u / (((width) + 7u) / 8u) + 2u))

/* Device workspace of the two entries below: the frames entries' for n_images * n_planes
 * frames (0 when that count is above 2^31 - 1). */
size_t mh_encode_images_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_images, uint32_t n_planes);
size_t mh_encode_images_shared_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_images,
                                               uint32_t n_planes);

/* mh_encode_frames_device_async reading n_images interleaved images of width x height pixels.
 * Input: sample (i, c, x, y) -- image i, plane c < C = layout->n_planes -- is the byte at
 * d_pixels + i * image_stride + y * row_pitch + x * pixel_stride + first_channel + c.
 * Output: n_images * C frames of width x height, plane c of image i being frame i * C + c
 * (plane_major 0) or c * n_images + i (plane_major 1). Every per-frame output -- header, code
 * slot, d_codes_len, d_block_offsets, d_block_init, d_status, d_frame_code_offsets -- is indexed
 * by that frame number and laid out as mh_encode_frames_device_async lays it out for n_frames =
 * n_images * C, so the result is one mh_frame batch of n_images * C frames: for
 * mh_build_luts_device, mh_decode_frames, the region / windows / crops entries, and
 * mh_decode_crops_norm_planes with plane_frame_stride 1 (plane_major 0) or n_images (1).
 * Exactness: for every accepted frame the header, the codes with their pad, d_codes_len, the
 * block offsets and the init bytes are byte for byte mh_encode_frame's for the de-interleaved
 * plane. With n_planes = 1, pixel_stride = 1, first_channel = 0 and row_pitch = width the call
 * accepts and writes exactly what mh_encode_frames_device_async does with gray_frame_stride =
 * image_stride.
 * Reads: of image i only bytes in [i * image_stride, i * image_stride + (height - 1) * row_pitch
 * + width * pixel_stride) are loaded: wide loads may touch row padding and unselected channels
 * inside that span, nothing behind the last pixel of the last row and nothing between images.
 * No output depends on a byte that is not a selected sample.
 * Alignment: none is required of d_pixels or of any stride. With pixel_stride <= 4 and d_pixels,
 * row_pitch (height > 1) and image_stride (n_images > 1) all multiples of 4, a block row's 8 *
 * pixel_stride bytes are loaded as dwords and the plane's bytes picked in registers; every
 * other layout takes one byte load per sample.
 * Checks, all before any HIP call, in mh_encode_frames_device_async's order and with its codes
 * (n_images where it has n_frames), plus: NULL layout, n_planes == 0 or > MH_MAX_PLANES, or
 * plane_major > 1 -> MH_ERR_INVALID_ARG (with the NULL checks); pixel_stride == 0 or
 * first_channel + n_planes > pixel_stride -> MH_ERR_DIMS (with the dims check); and, in the
 * place of the gray_frame_stride check, MH_ERR_CAPACITY for height > 1 and row_pitch < width *
 * pixel_stride, for n_images > 1 and image_stride below an image's span (above), and for a
 * layout that is not addressable (MH_IMAGE_TILE_SPAN_MAX above; row_pitch is ignored for height
 * == 1 and image_stride for n_images == 1). n_images * C counts as n_frames in every limit of
 * the frames entry: above 2^31 - 1 frames or tiles -> MH_ERR_CAPACITY, and the workspace is
 * mh_encode_images_workspace_bytes().
 * flags, d_status and every other argument: mh_encode_frames_device_async's. A rejected plane
 * frame disturbs neither its sibling planes nor the other images.
 * Launches: three, as the frames entry; the split and the packer are its kernels with another
 * pixel fetch. The planes of one tile are served by workgroups eight apart in the grid, so
 * that the later ones find the source lines in the first one's L2. */
int mh_encode_images_device_async(const uint8_t *d_pixels, const mh_image_layout *layout, uint32_t n_images,
                                  uint32_t width, uint32_t height, uint32_t flags, uint8_t *d_canon_headers,
                                  uint8_t *d_codes, uint64_t codes_frame_stride, uint64_t *d_codes_len,
                                  uint64_t *d_frame_code_offsets, uint32_t *d_block_offsets, uint8_t *d_block_init,
                                  int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);

/* mh_encode_frames_shared_device_async reading interleaved images: input, frame order, reads,
 * alignment and the added checks are mh_encode_images_device_async's; modes, outputs, statuses
 * and the remaining checks are mh_encode_frames_shared_device_async's with n_frames = n_images *
 * C (built mode: n_images * C * NB * 64 < 2^32 symbols). For every accepted frame the codes,
 * d_codes_len and the block offsets are byte for byte mh_encode_frame_with_header's for the
 * de-interleaved plane and the one header; in built mode that header is mh_code_lengths (or
 * the length-limited code) of the histogram summed over all n_images * C planes. */
int mh_encode_images_shared_device_async(
    const uint8_t *d_pixels, const mh_image_layout *layout, uint32_t n_images,
    uint32_t width, uint32_t height, uint32_t flags,
    const uint8_t *d_canon_in, uint8_t *d_canon_header,
    uint8_t *d_codes, uint64_t codes_frame_stride, uint64_t *d_codes_len,
    uint64_t *d_frame_code_offsets, uint32_t *d_block_offsets, uint8_t *d_block_init,
    int32_t *d_status, int32_t *d_header_status,
    void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* A SET of frames of different sizes encoded in one call: the producer of what the            */
/* mh_decode_set_* entries consume. n frames, each with its own width, height, source address  */
/* and Huffman table, go straight into the frame-set layout (mh_frame_geom above) in three      */
/* launches whatever n and whatever the number of sizes; every accepted frame is byte for byte */
/* mh_encode_frame's. A host planner (no HIP call) turns the n source records into a plan blob */
/* in device format; the caller uploads it and hands it to the entry.                          */
/* Not covered: a shared table over a set; mh_check_frames over a set; compaction of the code  */
/* slots (frame f keeps its whole codes_cap slot).                                              */
typedef struct {
  uint64_t pixels;        /* absolute device address of sample (0, 0); frames may be separate
                             allocations */
  uint64_t row_pitch;     /* bytes from row y to row y + 1 (ignored for height == 1) */
  uint32_t pixel_stride;  /* bytes from pixel x to pixel x + 1, 1..255 */
  uint32_t width, height; /* pixels, 1..65535 */
  uint32_t reserved;      /* must be 0 */
  uint64_t codes_cap;     /* the frame's code slot in bytes: a multiple of 16, at least 16 */
} mh_set_source;          /* 40 bytes */

/* Sample (x, y) of frame f is the byte at pixels + y * row_pitch + x * pixel_stride, so plane c of
 * an interleaved K-channel image is a frame with pixel_stride = K and pixels = image +
 * first_channel + c. Reads: of frame f only bytes in [pixels, pixels + (height - 1) * row_pitch +
 * width * pixel_stride), and no output depends on a byte that is not a sample (as for
 * mh_encode_images_device_async). */

/* The plan's record of frame f, as the kernels read it (device format; written by the planner). */
typedef struct {
  uint64_t pixels;
  uint64_t slot_offset;   /* the frame's code slot: the prefix sum of codes_cap in frame order */
  uint64_t codes_cap;
  uint32_t row_pitch;     /* 0 for height == 1 */
  uint32_t pixel_stride;
  uint32_t width, height;
  uint32_t block_width;   /* ceil(width / 8) */
  uint32_t n_blocks;      /* NB_f */
  uint32_t n_tiles;       /* ceil(NB_f / MH_SET_TILE_BLOCKS) */
  uint32_t first_tile;    /* the prefix sum of n_tiles */
  uint32_t first_block;   /* the prefix sum of NB: mh_frame_geom.first_block */
  uint32_t reserved;
} mh_set_frame;           /* 64 bytes */

#define MH_SET_TILE_BLOCKS 256u /* blocks per split workgroup and per packer wave */
#define MH_SET_PACK_TILES 4u    /* tiles of ONE frame per pack workgroup */
#define MH_SET_FETCH_BYTES 0xFFu

/* What the planner derives from the n records: the entry takes it back as it is. */
typedef struct {
  uint64_t codes_bytes;      /* the sum of codes_cap: the least d_codes may hold */
  uint64_t workspace_bytes;  /* the least d_workspace may hold */
  uint64_t plan_bytes;       /* mh_encode_set_plan_bytes() */
  uint64_t geoms_offset;     /* d_plan + geoms_offset: n mh_frame_geom records, 16-byte aligned,
                                the d_geoms of the mh_decode_set_* entries */
  uint64_t split_map_offset; /* split_grid x (u32 frame, u32 tile) */
  uint64_t pack_map_offset;  /* pack_grid x (u32 frame, u32 first tile of MH_SET_PACK_TILES) */
  uint32_t n_frames;
  uint32_t total_blocks;     /* sum of NB_f: entries of d_block_offsets / d_block_init */
  uint32_t total_tiles;
  uint32_t split_grid;       /* workgroups of the split (= total_tiles) ... */
  uint32_t pack_grid;        /* ... and of the packer */
  uint32_t max_width, max_height; /* the largest in the set: the dims of the set's mh_frame */
  uint32_t fetch_mode;       /* 1..4: dword loads at that pixel stride; MH_SET_FETCH_BYTES */
} mh_set_totals;             /* 80 bytes */

/* Bytes of the plan blob for these records; 0 when mh_encode_set_plan would refuse them. The blob
 * holds the n mh_set_frame records at offset 0, then the geometry records, the split map and the
 * pack map at the offsets in mh_set_totals (each 16-byte aligned). */
size_t mh_encode_set_plan_bytes(uint32_t n_frames, const mh_set_source *sources);

/* Write the plan of n_frames records into h_plan (host memory, plan_bytes) and its totals. Pure
 * host code: no HIP call, runs without a GPU. flags are the entry's (they are only validated).
 * Geometry: first_block is the prefix sum of NB_f in frame order, exactly what a packer of the
 * host-encoded frames produces. Fetch mode, one per call: dword loads when every record has the
 * same pixel_stride <= 4, every row_pitch (for height > 1) is a multiple of 4 and every pixels is
 * either a multiple of 4 or the address of a later byte of a pixel that starts on one (pixels % 4
 * < pixel_stride: plane c of an aligned interleaved image); byte loads otherwise. In the dword
 * mode the loads are whole aligned dwords from the one that holds sample (0, 0) on, so the up to 3
 * bytes between that dword's start and `pixels` may be loaded too (never used); no load reaches
 * past the frame's last sample.
 * Checks, in this order, each over all records before the next:
 *  1. NULL sources, h_plan or totals, n_frames == 0 -> MH_ERR_INVALID_ARG;
 *  2. a reserved word != 0 or a flag other than MH_FLAG_NO_DELTA | MH_ENCODE_WORKSPACE_ZEROED |
 *     MH_ENCODE_LIMIT_LENGTHS -> MH_ERR_INVALID_ARG;
 *  3. width or height 0 or above 65535, pixel_stride 0 or above 255 -> MH_ERR_DIMS;
 *  4. codes_cap not a multiple of 16, or 0 -> MH_ERR_ALIGN;
 *  5. MH_ERR_CAPACITY: height > 1 and row_pitch < width * pixel_stride; a record that is not
 *     addressable (MH_IMAGE_TILE_SPAN_MAX above, for this record's width, height, row_pitch and
 *     pixel_stride); total_blocks above 2^32 - 1; more than 2^31 - 1 tiles or frames; a sum of
 *     codes_cap above 2^64 - 1; plan_bytes below mh_encode_set_plan_bytes(). */
int mh_encode_set_plan(uint32_t n_frames, const mh_set_source *sources, uint32_t flags, void *h_plan,
                       size_t plan_bytes, mh_set_totals *totals);

/* Encode the set. d_plan: the uploaded blob (16-byte aligned); totals: the planner's, unchanged.
 * Outputs, per frame f: d_canon_headers + 256 f; codes at d_codes + slot_offset_f, the slot's size
 * codes_cap_f being the frame's capacity; d_codes_len[f] (optional); d_block_offsets and
 * d_block_init (optional) at [first_block_f, first_block_f + NB_f) of total_blocks entries;
 * d_status[f] (optional); d_frame_code_offsets (REQUIRED, n_frames + 1 u64, written by the device
 * from the plan: slot_offset_f, then codes_bytes). With d_plan + geoms_offset they are one frame
 * set: for mh_build_luts_device over d_canon_headers and the mh_decode_set_* entries, d_status
 * going in as d_frame_status, without touching the host.
 * flags, the status values, what is written of a slot ([0, round_up(codes_len, 4)) and nothing
 * behind it) and what a rejected frame leaves behind (no code byte, no offset, d_codes_len 0, its
 * d_block_init entries unspecified) are mh_encode_frames_device_async's, with codes_cap_f in the
 * place of codes_frame_stride. A rejected frame disturbs no other frame, whatever their sizes.
 * Checks, all before any HIP call, in that entry's order: NULL d_plan, totals, d_canon_headers,
 * d_codes, d_frame_code_offsets, d_block_offsets or d_workspace, n_frames, total_tiles or
 * total_blocks 0, an unknown flag or fetch mode -> MH_ERR_INVALID_ARG; max_width or max_height 0
 * or above 65535 -> MH_ERR_DIMS; d_codes or d_plan not 16-byte, d_workspace not 256-byte aligned
 * -> MH_ERR_ALIGN; codes_bytes below totals->codes_bytes, more than 2^31 - 1 frames or tiles, grids
 * that do not match the tile count, workspace_bytes below totals->workspace_bytes ->
 * MH_ERR_CAPACITY.
 * The plan is trusted as a prepared table is: the kernels do not validate its records. Their
 * stores of init bytes, block offsets and code words are bounded by the totals all the same (a
 * frame's descriptors end at total_blocks and codes_bytes), so a stale plan cannot store outside
 * the caller's arrays.
 * Launches: three (split, one tree workgroup per frame, packer), the batched entries' kernels
 * with one more source type: each split and pack workgroup loads its map entry and then its
 * frame's record, both wave-uniform. d_workspace: 256-byte aligned, any content. Asynchronous on
 * `stream`; d_plan must stay alive and unchanged until the launches have run. */
int mh_encode_set_device_async(const void *d_plan, const mh_set_totals *totals, uint32_t flags,
                               uint8_t *d_canon_headers, uint8_t *d_codes, uint64_t codes_bytes,
                               uint64_t *d_codes_len, uint64_t *d_frame_code_offsets,
                               uint32_t *d_block_offsets, uint8_t *d_block_init, int32_t *d_status,
                               void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* Streaming from host memory (BASELINE config 5; the reference's per-frame  */
/* command buffer, AAPLRenderer.m:1178-1921).                               */

typedef struct mh_stream mh_stream;

/* A decode stream for frames shaped like `proto` (dims, flags, tables, d_lut;
 * a non-NULL proto->d_block_init means frames carry per-block init bytes; the
 * frame pointers in proto are ignored). It owns n_slots device slots of
 * codes_capacity code bytes each, one HIP stream per slot (its copies, then its
 * decode), and one captured decode graph per slot. Slot i decodes into d_outputs[i] (caller
 * device buffers of round_up(W, 8) * H bytes, 8-byte aligned) or, when
 * d_outputs is NULL, into rasters the stream allocates.
 * proto->flags: MH_FLAG_NO_DELTA only; any other bit -> MH_ERR_INVALID_ARG with the other
 * argument checks, before any HIP call (mh_stream_create_headers and, through its members,
 * mh_stream_group_create alike). MH_FLAG_ANY_ORDER in particular is refused: the stream itself
 * queues the H2D copy that writes a slot's inputs ahead of the slot's decode, so that decode
 * must keep its dispatch barrier.
 * codes_capacity need not be a multiple of 16: a slot holds round_up(codes_capacity, 16) code
 * bytes, and a submit is accepted up to that many (MH_CODES_PAD <= codes_bytes <=
 * round_up(codes_capacity, 16)); a refused submit does not advance the slot rotation.
 * Creation runs one warm-up decode per slot over zeroed slot buffers, so it does store into
 * the rasters (d_outputs included), and only inside their round_up(W, 8) * H bytes. */
int mh_stream_create(const mh_frame *proto, uint64_t codes_capacity, uint32_t n_slots,
                     uint8_t *const *d_outputs, mh_stream **out);
/* Queue one frame: H2D copy of its host buffers (pinned memory for a DMA) into
 * the next slot, after that slot's previous decode (same stream), then the slot's
 * decode. codes_bytes includes the MH_CODES_PAD zero bytes; h_block_init must
 * be given iff the stream was created with it. When the host codes follow the
 * block offsets at byte round_up(4*NB, 16) of one buffer, both move in one DMA.
 * Returns the slot in *slot. */
int mh_stream_submit(mh_stream *s, const uint8_t *h_codes, uint64_t codes_bytes,
                     const uint32_t *h_block_offsets, const uint8_t *h_block_init,
                     uint32_t *slot);
/* The slot's output raster (device); valid until n_slots further submits. */
uint8_t *mh_stream_output(mh_stream *s, uint32_t slot, size_t *out_pitch);
/* Each slot copies and decodes on its own hipStream_t (stream order keeps a slot's
 * decode ahead of the copy that reuses it). mh_stream_slot_stream: the stream of
 * `slot`, for events or work that consumes its raster; mh_stream_compute_stream:
 * the stream of the most recent submit. */
void *mh_stream_slot_stream(mh_stream *s, uint32_t slot);
void *mh_stream_compute_stream(mh_stream *s);
int mh_stream_wait(mh_stream *s, uint32_t slot);  /* that slot's decode done */
/* Device-side latency of the slot's most recent frame (waits for it): from the
 * start of its H2D copy to the end of its decode, in milliseconds. */
int mh_stream_slot_time(mh_stream *s, uint32_t slot, float *ms);
int mh_stream_device(mh_stream *s);               /* the HIP device it runs on */
int mh_stream_synchronize(mh_stream *s);
int mh_stream_destroy(mh_stream *s);

/* The stream in table-per-frame mode: every frame brings its own 256-byte canonical header
 * (what mh_encode_frame and the GPU encoders write per frame). proto: dims, flags
 * (MH_FLAG_NO_DELTA only) and whether frames carry init bytes, and codes_capacity, as
 * mh_stream_create; its table fields are ignored and may be NULL.
 * A slot is one allocation [status, 16 B][header, 256 B][block offsets, padded to 16 B][codes]
 * and its decode is one mh_decode_headers launch (n_frames = 1) that writes the header's
 * verdict into the slot's status word -- launched directly by default (it measured faster than
 * its graph replay); MH_STREAM_GRAPHS=1 in the environment replays it from
 * a per-slot captured graph, 0 means direct launches as in table mode. Creating the stream
 * stores nothing into the rasters. mh_stream_output / slot_stream / compute_stream / wait / slot_time / device /
 * synchronize / destroy work on such a stream unchanged; mh_stream_submit returns
 * MH_ERR_INVALID_ARG on it, as mh_stream_submit_header does on a table-mode stream. Stream
 * groups stay table-mode only. (Frames that are to share ONE table -- the table-mode stream,
 * mh_decode, the stream groups -- come from mh_encode_frames_shared_device_async or
 * mh_encode_frame_with_header.) */
int mh_stream_create_headers(const mh_frame *proto, uint64_t codes_capacity, uint32_t n_slots,
                             uint8_t *const *d_outputs, mh_stream **out);
/* mh_stream_submit with the frame's header (256 host bytes; same capacity and init-byte
 * rules). When the host buffers lie header | block offsets padded to 16 B | codes in one
 * buffer -- h_block_offsets == h_canon_header + 256 and h_codes == h_block_offsets +
 * round_up(4*NB, 16) -- the frame moves in one DMA; otherwise in one copy per part. */
int mh_stream_submit_header(mh_stream *s, const uint8_t *h_canon_header, const uint8_t *h_codes,
                            uint64_t codes_bytes, const uint32_t *h_block_offsets,
                            const uint8_t *h_block_init, uint32_t *slot);
/* Waits for the slot's decode and returns its header's verdict in *status: MH_OK,
 * MH_ERR_CODE_TOO_LONG or MH_ERR_TABLE. A rejected header leaves the slot's raster exactly
 * as it was; the next frame submitted to the slot decodes normally. MH_OK for a slot never
 * used and on a table-mode stream. */
int mh_stream_slot_status(mh_stream *s, uint32_t slot, int32_t *status);

/* Stream groups (config 5 on N GPUs of one node): n_members streams, member i on
 * HIP device devices[i] with protos[i] (tables and d_lut resident on that device),
 * n slots each; frames are round-robined over the members in submit order (frame
 * k -> member k mod n). Every call sets the member's device for its duration and
 * restores the caller's. A device may appear more than once. */
typedef struct mh_stream_group mh_stream_group;
int mh_stream_group_create(const mh_frame *protos, uint32_t n_members, const int *devices,
                           uint64_t codes_capacity, uint32_t slots_per_member,
                           mh_stream_group **out);
int mh_stream_group_submit(mh_stream_group *g, const uint8_t *h_codes, uint64_t codes_bytes,
                           const uint32_t *h_block_offsets, const uint8_t *h_block_init,
                           uint32_t *member, uint32_t *slot);
mh_stream *mh_stream_group_member(mh_stream_group *g, uint32_t member);
uint32_t mh_stream_group_size(const mh_stream_group *g);
int mh_stream_group_synchronize(mh_stream_group *g);
int mh_stream_group_destroy(mh_stream_group *g);

/* ---------------------------------------------------------------------- */
/* Host-side producer (CPU, reentrant). Outputs are byte-identical to the   */
/* reference's C++ codec.                                                   */

/* Util.m:233-323 splitIntoBlocksOfSize (zero pad). out: bw*bh*bdim*bdim bytes. */
int mh_split_blocks(const uint8_t *img, uint32_t width, uint32_t height, uint32_t block_dim,
                    uint8_t zero_value, uint8_t *out, size_t out_bytes);

/* Inverse of mh_split_blocks: block order -> W x H raster (crop). */
int mh_merge_blocks(const uint8_t *blocks, uint32_t width, uint32_t height, uint32_t block_dim,
                    uint8_t *out, size_t out_pitch);

/* HuffmanUtil::encodeSignedByteDeltas / decodeSignedByteDeltas
 * (HuffmanUtil.cpp:1133-1145 -> :21-78), applied to n bytes; in == out allowed. */
int mh_encode_signed_byte_deltas(const uint8_t *in, uint8_t *out, size_t n);
int mh_decode_signed_byte_deltas(const uint8_t *in, uint8_t *out, size_t n);

/* Upper bound of the codes bytes mh_encode_huffman / mh_encode_frame write. */
uint64_t mh_codes_bound(uint64_t n_symbols);

/* HuffmanUtil::encodeHuffman (HuffmanUtil.cpp:1051-1131 -> HuffmanEncoder::encode
 * HuffmanEncoder.cpp:310-381): canonical header, MSB-first codes followed by the
 * encoder's 2 zero bytes (*codes_len includes them) and the bit offset of every
 * block_dim*block_dim-th symbol (n_symbols / (block_dim^2) entries). */
int mh_encode_huffman(const uint8_t *symbols, uint64_t n_symbols, uint32_t block_dim,
                      uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                      uint64_t *codes_len, uint32_t *block_bit_offsets);

/* The renderer's whole producer step (AAPLRenderer.m:374-688) for one 8-bit
 * gray frame: split into zero-padded 8x8 blocks, per-block deltas (unless
 * MH_FLAG_NO_DELTA), encode, block offsets, and MH_CODES_PAD zero bytes of
 * read-ahead after the payload (*codes_len includes them). codes_cap >=
 * mh_codes_bound(NB*64) + 2. block_offsets: NB entries. block_init (optional,
 * NB bytes): when non-NULL, the first delta of every block is moved into it
 * and zeroed (IMPL_DELTAS_AND_INIT_ZERO_DELTA_BEFORE_HUFF_ENCODING,
 * AAPLRenderer.m:449-473). flags: MH_FLAG_NO_DELTA, MH_ENCODE_LIMIT_LENGTHS (a tree
 * deeper than 16 gets the limited lengths instead of MH_ERR_CODE_TOO_LONG). */
int mh_encode_frame(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                    uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                    uint64_t *codes_len, uint32_t *block_offsets, uint8_t *block_init);

/* Mid-block marks: a second, exact entry point in the middle of every block, so that two lanes
 * can decode one block (mh_decode_marked). One u32 per block, in block order, beside the block
 * offsets:
 *   bits 0-15   the code bits from the block's offset to its symbol 32, the first symbol of block
 *               row 4 (<= 32 x 16 = 512);
 *   bits 16-23  the running `prev` byte the 64-step decode holds when it begins symbol 32 under the
 *               frame's own flags: (block_init[b] or 0) + symbols 0..31, mod 256 -- pixel 31 of
 *               the block -- and 0 under MH_FLAG_NO_DELTA, which has no running sum;
 *   bits 24-31  0.
 * The marks are a hint a producer adds for free; they change no other buffer of the frame.
 *
 * mh_encode_frame_marks is mh_encode_frame -- every argument, status and output byte -- that also
 * writes the NB marks into mid_marks as it packs (NULL: mh_encode_frame itself). */
int mh_encode_frame_marks(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                          uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                          uint64_t *codes_len, uint32_t *block_offsets, uint8_t *block_init,
                          uint32_t *mid_marks);

/* The marks of a frame that arrives without them (the reference encoder's, a GPU encoder's): the
 * reference walk (see mh_frame) of the first 32 steps of each of n_blocks blocks from
 * block_offsets[b] over table1 / table2. Bytes at or past codes_bytes read as zero, a zero-width
 * lookup repeats `prev` and does not advance, an escape past table2_entries is the zero entry; no
 * byte outside the caller's buffers is read, whatever the offsets and the code bytes hold.
 * block_init: NB bytes or NULL (ignored under MH_FLAG_NO_DELTA). flags: MH_FLAG_NO_DELTA only.
 * For a frame of mh_encode_frame_marks the result equals the encoder's marks word for word.
 * MH_ERR_INVALID_ARG (a NULL pointer but block_init, n_blocks == 0, another flag), MH_ERR_TABLE
 * (table2_entries as in mh_decode). */
int mh_mid_marks(const uint8_t *codes, uint64_t codes_bytes, const uint32_t *block_offsets,
                 uint64_t n_blocks, const mh_lookup_symbol *table1, const mh_lookup_symbol *table2,
                 uint32_t table2_entries, const uint8_t *block_init, uint32_t flags, uint32_t *mid_marks);

/* Adds the symbol counts of one frame -- what mh_encode_frame would encode: split, per-block
 * deltas unless MH_FLAG_NO_DELTA, first delta zeroed when with_block_init -- into freq[256]
 * (a second call adds to the first). A host user builds a shared header as
 * mh_frame_histogram over the frames, then mh_code_lengths[_limited]. */
int mh_frame_histogram(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                       int with_block_init, uint64_t freq[256]);

/* mh_encode_frame under the caller's header instead of the frame's own tree: the host twin
 * of mh_encode_frames_shared_device_async, frame by frame. The status is the header's
 * verdict (MH_ERR_CODE_TOO_LONG for a length over 16, MH_ERR_TABLE for a Kraft sum over 1;
 * an incomplete code is valid), then MH_ERR_TABLE when the frame contains a symbol of
 * length 0 in the header, then MH_ERR_CAPACITY (codes_len > codes_cap, or >= 2^32 code
 * bits). Nothing is written on an error. Given the frame's own header, the output equals
 * mh_encode_frame's byte for byte. flags: MH_FLAG_NO_DELTA (MH_ENCODE_LIMIT_LENGTHS is
 * accepted and ignored). */
int mh_encode_frame_with_header(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                                const uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                                uint64_t *codes_len, uint32_t *block_offsets, uint8_t *block_init);

/* huff_util.hpp:94-193 huff_generate_canonical_codes: left-justified u16 codes. */
int mh_canonical_codes(const uint8_t canon_header[256], uint16_t codes[256]);

/* HuffmanUtil::parseCanonicalHeader + generateSplitLookupTables(8, 8, ...)
 * (HuffmanUtil.cpp:270-310, :338-667), without module statics. table2 needs
 * room for MH_TABLE2_MAX_ENTRIES entries; *table2_entries = (k+1)*256. */
int mh_build_tables(const uint8_t canon_header[256], mh_lookup_symbol table1[256],
                    mh_lookup_symbol *table2, uint32_t table2_cap, uint32_t *table2_entries);

/* CPU decoders (host, reentrant; never used by the GPU path).
 * HuffmanUtil::decodeHuffmanBits (HuffmanUtil.cpp:673-823; Huffman.h:30): serial
 * decode of n_symbols from the MSB-first stream through the single 65536-entry
 * table (mh_build_single_table); bit_offsets (optional, n_symbols entries) gets
 * each symbol's starting bit. MH_ERR_CAPACITY where the reference asserts
 * (numBytesRead + 2 < huffBuffN). */
int mh_decode_huffman_bits(const mh_lookup_symbol *table, uint64_t n_symbols, const uint8_t *codes,
                           uint64_t codes_bytes, uint8_t *out, uint32_t *bit_offsets);
/* HuffmanUtil::decodeHuffmanBitsFromTables (HuffmanUtil.cpp:830-1046; Huffman.h:42,
 * Huffman.mm:101): the same through the T1/T2 pair (table1_bits = table2_bits = 8,
 * as the reference's tables are built). */
int mh_decode_huffman_bits_from_tables(const mh_lookup_symbol *table1, const mh_lookup_symbol *table2,
                                       uint32_t table2_entries, uint32_t table1_bits, uint32_t table2_bits,
                                       uint64_t n_symbols, const uint8_t *codes, uint64_t codes_bytes,
                                       uint8_t *out, uint32_t *bit_offsets);
/* The CPU twin of mh_decode for one frame: every 8x8 block from its root bit
 * offset with the shader's semantics (AAPLShaders.metal:241-268: 16-bit window,
 * T1/T2, delta fold unless MH_FLAG_NO_DELTA, optional per-block init byte), written
 * into the W x H raster at out_pitch; block rows split over n_threads host threads
 * (0 or 1: the calling thread); each thread decodes eight neighbouring blocks in
 * lock-step. Bytes past codes_bytes read as zero. MH_ERR_CAPACITY if its 128 KB
 * flat table cannot be allocated. */
int mh_decode_frame_cpu(const uint32_t *block_offsets, const uint8_t *codes, uint64_t codes_bytes,
                        const mh_lookup_symbol *table1, const mh_lookup_symbol *table2,
                        uint32_t table2_entries, const uint8_t *block_init, uint32_t width,
                        uint32_t height, uint32_t flags, uint8_t *out, size_t out_pitch,
                        uint32_t n_threads);

/* The CPU twin of mh_check_headers for one frame: the reference walk of its n_blocks blocks
 * under the table of canon_header, report[4] as mh_check_frames writes it. Returns the header's
 * verdict (MH_OK, MH_ERR_CODE_TOO_LONG, MH_ERR_TABLE; a rejected header leaves the clean pattern)
 * or MH_ERR_INVALID_ARG for a NULL pointer or n_blocks == 0. */
int mh_check_frame_cpu(const uint32_t *block_offsets, uint32_t n_blocks, const uint8_t *codes,
                       uint64_t codes_bytes, const uint8_t canon_header[256], uint32_t report[4]);

/* The 8-byte container header HuffmanEncoder::encode emits ahead of the
 * canonical table (HuffmanEncoder.cpp:326-340: u32 LE 0xFFEEEEDD, u32 LE symbol
 * count) and HuffmanUtil::encodeHuffman drops (HuffmanUtil.cpp:1073-1086). */
#define MH_CONTAINER_HEADER_BYTES 8
#define MH_CONTAINER_MAGIC 0xFFEEEEDDu
int mh_container_header(uint64_t n_symbols, uint8_t header[MH_CONTAINER_HEADER_BYTES]);
/* MH_ERR_INVALID_ARG when the magic word does not match. */
int mh_parse_container_header(const uint8_t header[MH_CONTAINER_HEADER_BYTES], uint64_t *n_symbols);

/* Huffman code lengths (the canonical header) from 256 symbol counts, with the
 * reference tree's tie-breaking (HuffmanEncoder.cpp:29-145). MH_ERR_EMPTY for no
 * symbols, MH_ERR_CODE_TOO_LONG past 16 bits (lengths still written). */
int mh_code_lengths(const uint64_t freq[256], uint8_t canon_header[256]);

/* Code lengths of at most max_bits bits: mh_code_lengths' where those fit, otherwise the
 * optimal length-limited code by package-merge. Leaves are the present symbols sorted by
 * (count, symbol); list_1 is the leaves, list_l (l = 2..max_bits) the merge of the leaves
 * with the pairs of list_{l-1} (a trailing odd item dropped; on equal weight the leaf
 * first, packages in order); from t = 2n - 2, for l = max_bits..1, a_l is the number of
 * leaves among the first t items of list_l and t becomes 2 (t - a_l); the leaf of rank r
 * gets length #{l : a_l > r}, so among equal counts the lower symbol's code is not the
 * shorter. The result has Kraft sum 1 and the least sum of count x length of any code
 * within max_bits. max_bits in 1..16 with 2^max_bits >= the number of present symbols,
 * and a count total below 2^59 (weights are exact in 64 bits), else MH_ERR_INVALID_ARG;
 * MH_ERR_EMPTY for no symbols; one symbol gets length 1. */
int mh_code_lengths_limited(const uint64_t freq[256], uint32_t max_bits, uint8_t canon_header[256]);

/* HuffmanUtil::generateLookupTable (HuffmanUtil.cpp:314-334): 65536 entries. */
int mh_build_single_table(const uint8_t canon_header[256], mh_lookup_symbol table[65536]);

/* ---------------------------------------------------------------------- */
/* Utilities */
const char *mh_error_string(int status);
int mh_device_count(void);
/* sha256 (hex) over the compile flags, sources and headers the library was built
 * from (metalhuffman_amd/build.py). The Python loader refuses a library whose
 * stamp differs from the sources beside it; a debug build's self-check in the
 * spirit of the renderer's DEBUG decode compare (AAPLRenderer.m:616-650). */
const char *mh_build_stamp(void);

#ifdef __cplusplus
}
#endif
#endif /* METALHUFFMAN_H */
