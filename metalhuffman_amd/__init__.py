"""metalhuffman_amd -- MI355X-native Huffman block decoder (drop-in for the decode path
of mdejong/MetalHuffman).

  * include/metalhuffman.h          C-ABI (the drop-in boundary)
  * csrc/mh_decode.hip              hand-written gfx950 decode kernel
  * csrc/mh_host.cpp                host producer: encoder, canonical codes, T1/T2
  * csrc/mh_cpu.cpp                 the reference's CPU decoders + a threaded CPU frame decoder
  * codec.Huffman                   the reference's `Huffman` facade (Shared/Huffman.h)
  * decoder.decode / DeviceFrames   GPU decode of one frame or a batch
  * decoder.DeviceTables            T1/T2 + prepared table (uploaded, or built on the device)
  * decoder.decode_frames / DeviceTableSet   a batch with a table per frame, one launch
  * decoder.decode_headers          the same batch straight from its canonical headers (table built in-kernel)
  * decoder.check_frames / check_headers   mh_check for such a batch: a report and a verdict word per frame that
                                    goes into the decode entries' frame_status; codec.check_frame is the CPU twin
  * decoder.decode_region / decode_rect   a block-aligned region (a pixel rectangle) of every frame, one launch
  * decoder.decode_region_scaled / decode_scaled   a region (the frame) at 1/2, 1/4 or 1/8 scale, one launch:
                                    box means taken in the decoder's registers; codec.box_reduce is the CPU twin
  * decoder.decode_windows / windows_of_rects   a list of windows of one size, each with its own frame and
                                    origin (random crops, a viewer's missing tiles, a moving box), one launch
  * decoder.decode_windows_scaled   the same list at 1/2, 1/4 or 1/8 scale (a viewer's missing tiles at a pyramid
                                    level, a thumbnail sheet, multi-scale crops), one launch
  * decoder.decode_crops            a list of crops of one size at PIXEL origins, each stored from byte 0 of its
                                    own slot (a dense [n, h, w] batch of random crops), one launch
  * decoder.decode_crops_normalized   the same crops straight into normalised float16 / bfloat16 / float32
                                    elements, optionally mirrored (crop-mirror-normalize), one launch;
                                    codec.norm_table is the CPU twin of the conversion
  * decoder.decode_crops_normalized_planes   crops of images stored as C planes (one frame each) straight into
                                    a normalised [n, C, h, w] tensor, a (scale, bias) per plane, one launch;
                                    codec.norm_coefficients makes the pairs from a mean and a deviation
  * decoder.DeviceFrameSet / decode_set_crops / decode_set_crops_normalized_planes   the crop entries over a
                                    frame SET -- frames of different sizes, a geometry record each -- so a
                                    sampled batch over images of many sizes is one launch, not one per size;
                                    codec.frame_set_layout is the host packer
  * decoder.decode_set_frames / decode_set_frames_shape / DeviceSetPlan   every frame of a set WHOLE, each at
                                    its own size into its own raster, one launch (a raster and a share record
                                    per frame and a group map, validated on the device before use: a rejected
                                    geometry is MH_ERR_DIMS, a rejected raster MH_ERR_CAPACITY, a skipped frame
                                    its status word); codec.decode_set_plan is the host planner (no GPU needed).
                                    Not covered: regions, windows and scaled decodes over a set
  * encoder.Encoder                 GPU encoder (encode / encode_async: no host sync)
  * encoder.BatchEncoder            n frames per call; AsyncEncodedBatch.decode(): encode ->
                                    n tables -> decode on one stream, no host sync;
                                    encode_shared_async: the batch under ONE table (built from the summed
                                    histogram, or a supplied header) for decoder.decode;
                                    codec.shared_header / encode_frame(header=) are the CPU twins;
                                    encode_images_async / encode_images_shared_async: interleaved, pitched
                                    [n, H, W, K] pixels (any view with adjacent channels) straight into C-plane
                                    frames, no transposed copy; codec.image_planes defines the planes
  * encoder.encode_set_async / encode_image_set_async   frames (planes of images) of DIFFERENT sizes, a table
                                    each, straight into the frame-set layout in three launches; AsyncEncodedSet
                                    .frame_set() / .table_set() feed decode_set_crops* with no host sync, and
                                    .decode() is encode -> n tables -> decode_set_frames on one stream;
                                    codec.encode_set_plan is the host planner (no GPU needed)
  * stream                          streaming from host memory (config 5); HeaderFrameStream: a header per frame
  * dist                            frame sharding, single-frame bands, table broadcast
"""
from ._native import (EXPORTS, LIB_PATH, MH_CODES_PAD, MH_CROP_MIRROR, MH_ENCODE_LIMIT_LENGTHS, MH_ERR_STREAM,
                      MH_FLAG_LANE_PAIRS,
                      MH_FLAG_NO_DELTA, MH_MAX_PLANES, MH_NORM_BF16, MH_NORM_F16, MH_NORM_F32, MHError, lib)
from .codec import (BLOCK_DIM, EncodedFrame, FrameSetLayout, Huffman, block_grid, box_reduce, check_frame, code_lengths_limited,
                    decode_frame_cpu, decode_set_plan, DecodeSetPlan, encode_frame, encode_set_plan, frame_histogram, frame_set_layout, image_planes, merge_blocks, norm_coefficients, norm_table, shared_header,
                    split_blocks)

__all__ = [
    "EXPORTS", "LIB_PATH", "MH_CODES_PAD", "MH_FLAG_LANE_PAIRS", "MH_FLAG_NO_DELTA", "MHError", "lib", "BLOCK_DIM",
    "EncodedFrame", "Huffman", "block_grid", "decode_frame_cpu", "encode_frame", "merge_blocks", "split_blocks",
    "MH_ENCODE_LIMIT_LENGTHS", "code_lengths_limited", "box_reduce", "frame_histogram", "shared_header",
    "norm_table", "MH_NORM_F16", "MH_NORM_BF16", "MH_NORM_F32", "MH_CROP_MIRROR",
    "MH_MAX_PLANES", "norm_coefficients", "image_planes", "check_frame", "MH_ERR_STREAM",
    "FrameSetLayout", "frame_set_layout", "encode_set_plan", "decode_set_plan", "DecodeSetPlan",
]
__version__ = "0.1.0"
