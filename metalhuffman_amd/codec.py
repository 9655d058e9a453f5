"""Host-side producer API (CPU) -- the reference's `Huffman` facade without module state.

Mirrors the class methods of Shared/Huffman.h:9-77 (ObjC) / HuffmanUtil statics
(Shared/HuffmanUtil.hpp:22-100) with the same names and argument meaning, backed by
the C++ codec in libmetalhuffman_amd.so (csrc/mh_host.cpp). Outputs are
byte-identical to the reference encoder and table builder.

Differences from the reference, by design:
  * no module statics: parseCanonicalHeader returns the canonical codes instead of
    stashing them (HuffmanUtil.cpp:87-102), and generateSplitLookupTables takes the
    canonical header explicitly;
  * errors raise MHError instead of assert() (e.g. a code deeper than 16 bits,
    HuffmanEncoder.cpp:131); encode_frame(limit_lengths=True) encodes such a frame
    with the optimal code of at most 16 bits instead (code_lengths_limited);
  * the CPU decoders (decodeHuffmanBits*, decode_frame_cpu) are product code in the
    native library (csrc/mh_cpu.cpp, a threaded frame decoder for the reference's CPU
    path); the GPU decoder is the hot path. Neither calls the CPU restatement in
    oracle/, which stays the test-only checker.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import NamedTuple, Optional

import numpy as np

from . import _native as N

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u16p = ctypes.POINTER(ctypes.c_uint16)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def _p(a: np.ndarray, t=_u8p):
    return a.ctypes.data_as(t)


def _u8(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


BLOCK_DIM = 8


def block_grid(width: int, height: int, block_dim: int = BLOCK_DIM) -> tuple[int, int]:
    """AAPLRenderer.m:753-761: ceil(W/8) x ceil(H/8)."""
    return -(-width // block_dim), -(-height // block_dim)


@dataclasses.dataclass
class EncodedFrame:
    """One frame in the reference's buffer contract (AAPLRenderer.m:374-688)."""
    width: int
    height: int
    canon: np.ndarray           # u8[256] canonical code lengths
    codes: np.ndarray           # u8[payload + MH_CODES_PAD] (huffBuff, read-ahead included)
    block_offsets: np.ndarray   # u32[NB] bit offset of every 8x8 block
    block_init: Optional[np.ndarray] = None  # u8[NB] (INIT_ZERO_DELTA mode) or None
    flags: int = 0
    # u32[NB] mid-block marks (metalhuffman.h: code bits to symbol 32 | prev << 16) or None: a hint
    # for the single-frame decode, filled by encode_frame; with_mid_marks() derives them for any frame.
    # Marks belong to the buffers they were made from. marks_for names those -- the (codes,
    # block_offsets, block_init) arrays themselves -- and marks are used only while the frame still
    # holds those very objects (valid_mid_marks): a frame given other code bytes, offsets or init
    # bytes (dataclasses.replace, an assignment) has no marks until with_mid_marks() makes them
    # again. Writing INTO the arrays is not seen: whoever does that clears or remakes the marks.
    mid_marks: Optional[np.ndarray] = None
    marks_for: Optional[tuple] = dataclasses.field(default=None, repr=False, compare=False)

    def _buffers(self) -> tuple:
        return (self.codes, self.block_offsets, self.block_init)

    def valid_mid_marks(self) -> Optional[np.ndarray]:
        """mid_marks if they were made for the buffers this frame holds now, else None."""
        if self.mid_marks is None or self.marks_for is None:
            return None
        return self.mid_marks if all(a is b for a, b in zip(self.marks_for, self._buffers())) else None

    @property
    def block_width(self) -> int:
        return block_grid(self.width, self.height)[0]

    @property
    def block_height(self) -> int:
        return block_grid(self.width, self.height)[1]

    @property
    def n_blocks(self) -> int:
        return self.block_width * self.block_height

    @property
    def payload_bytes(self) -> int:
        return int(self.codes.size) - N.MH_CODES_PAD

    def tables(self) -> tuple[np.ndarray, np.ndarray]:
        return Huffman.generateSplitLookupTables(self.canon)

    def band(self, by0: int, by1: int) -> "EncodedFrame":
        """Block rows [by0, by1) as a self-contained frame (the
        single-frame split): blocks are independent given their offsets, so a band
        needs only the code bytes from its first block's byte to its last block's
        end. Offsets are rebased to that byte, MH_CODES_PAD zero bytes follow, and
        the height is the band's pixel rows (the last band keeps the frame's partial
        block row). Decoding the band gives rows [8*by0, 8*by0 + height) of the frame."""
        bw, bh = self.block_width, self.block_height
        if not 0 <= by0 < by1 <= bh:
            raise ValueError(f"block rows [{by0}, {by1}) outside [0, {bh})")
        b0, b1 = by0 * bw, by1 * bw
        offs = self.block_offsets
        base = int(offs[b0]) >> 3
        end_bits = int(offs[b1]) if b1 < self.n_blocks else 8 * self.payload_bytes
        end = (end_bits + 7) >> 3
        codes = np.zeros(end - base + N.MH_CODES_PAD, np.uint8)
        codes[: end - base] = self.codes[base:end]
        band_offs = (offs[b0:b1].astype(np.int64) - 8 * base).astype(np.uint32)
        init = None if self.block_init is None else self.block_init[b0:b1].copy()
        height = min(self.height, 8 * by1) - 8 * by0
        # a mark is relative to its own block's offset, so a band's marks are the frame's
        marks = self.valid_mid_marks()
        out = EncodedFrame(self.width, height, self.canon, codes, band_offs, init, self.flags)
        if marks is not None:
            out.mid_marks, out.marks_for = marks[b0:b1].copy(), out._buffers()
        return out

    def with_mid_marks(self) -> "EncodedFrame":
        """This frame with its mid-block marks derived by the walk (mh_mid_marks): for frames that
        arrive without them -- the reference encoder's, a GPU encoder's, a foreign header's."""
        t1, t2 = self.tables()
        t1 = np.ascontiguousarray(t1).view(np.uint8).reshape(-1)
        t2 = np.ascontiguousarray(t2).view(np.uint8).reshape(-1)
        offs = np.ascontiguousarray(self.block_offsets, np.uint32)
        codes = np.ascontiguousarray(self.codes, np.uint8)
        init = None if self.block_init is None else np.ascontiguousarray(self.block_init, np.uint8)
        marks = np.zeros(self.n_blocks, np.uint32)
        N.check(N.lib().mh_mid_marks(_p(codes), codes.size, _p(offs, _u32p), self.n_blocks, t1.ctypes.data,
                                     t2.ctypes.data, t2.size // 2, _p(init) if init is not None else None,
                                     self.flags & N.MH_FLAG_NO_DELTA, _p(marks, _u32p)), "mh_mid_marks")
        return dataclasses.replace(self, mid_marks=marks, marks_for=self._buffers())


class FrameSetLayout(NamedTuple):
    """frame_set_layout's result: the host arrays of a frame set (include/metalhuffman.h,
    mh_frame_geom). Frame f's block offsets (and block_init) are [first, first + NB_f) of the
    concatenated arrays, first = geoms[f, 0]; its codes are codes[code_offsets[f]: code_offsets[f + 1]],
    a 16-byte aligned slot that holds the frame's own bytes and then zeros."""
    block_offsets: np.ndarray         # u32[total_blocks]
    codes: np.ndarray                 # u8[code_offsets[n]]
    code_offsets: np.ndarray          # int64[n + 1], multiples of 16
    geoms: np.ndarray                 # u32[n, 4] = (first_block, width, height, 0)
    total_blocks: int
    block_init: Optional[np.ndarray]  # u8[total_blocks] or None
    width: int                        # the largest width ...
    height: int                       # ... and the largest height in the set
    flags: int


FRAME_SET_ALIGN = 16  # a frame's code slot starts on a 16-byte boundary, as in a packed batch


def frame_set_layout(frames) -> FrameSetLayout:
    """The packed host layout of a frame SET: a sequence of EncodedFrame of any sizes, each with its
    own table, for decoder.DeviceFrameSet and the mh_decode_set_* entries. ValueError: no frames,
    frames of mixed flags, or block_init present on some frames only."""
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    if any(f.flags != frames[0].flags for f in frames):
        raise ValueError("a frame set holds frames of one format (flags)")
    with_init = [f.block_init is not None for f in frames]
    if any(with_init) and not all(with_init):
        raise ValueError("block_init is present on all frames of a set or on none")
    n = len(frames)
    geoms = np.zeros((n, 4), np.uint32)
    starts = np.zeros(n + 1, np.int64)
    first = 0
    for i, f in enumerate(frames):
        if not (1 <= f.width <= N.MH_MAX_DIM and 1 <= f.height <= N.MH_MAX_DIM):
            raise ValueError(f"frame {i}: {f.width}x{f.height} is outside 1..{N.MH_MAX_DIM}")
        if f.block_offsets.size != f.n_blocks:
            raise ValueError(f"frame {i}: {f.block_offsets.size} block offsets for {f.n_blocks} blocks")
        geoms[i] = (first, f.width, f.height, 0)
        first += f.n_blocks
        starts[i + 1] = starts[i] + -(-f.codes.size // FRAME_SET_ALIGN) * FRAME_SET_ALIGN
    if first > 0xFFFFFFFF:
        raise ValueError(f"{first} blocks do not fit the set's 32-bit block index")
    codes = np.zeros(int(starts[-1]), np.uint8)
    for f, s in zip(frames, starts):
        codes[s: s + f.codes.size] = f.codes
    offs = np.concatenate([np.asarray(f.block_offsets, np.uint32) for f in frames])
    init = np.concatenate([np.asarray(f.block_init, np.uint8) for f in frames]) if with_init[0] else None
    return FrameSetLayout(offs, codes, starts, geoms, first, init, max(f.width for f in frames),
                          max(f.height for f in frames), frames[0].flags)


class SetPlan(NamedTuple):
    """encode_set_plan's result: the plan blob (device format, u8) and its mh_set_totals, with the
    blob's parts as numpy views."""
    plan: np.ndarray
    totals: "N.mh_set_totals"

    @property
    def records(self) -> np.ndarray:
        """The n mh_set_frame records as a ctypes array over the blob."""
        return (N.mh_set_frame * self.totals.n_frames).from_buffer(self.plan)

    @property
    def geoms(self) -> np.ndarray:
        """u32[n, 4]: the mh_frame_geom records (first_block, width, height, 0)."""
        t = self.totals
        return self.plan[t.geoms_offset: t.geoms_offset + 16 * t.n_frames].view(np.uint32).reshape(-1, 4)

    @property
    def split_map(self) -> np.ndarray:
        """u32[split_grid, 2]: (frame, tile) of every split workgroup."""
        t = self.totals
        return self.plan[t.split_map_offset: t.split_map_offset + 8 * t.split_grid].view(np.uint32).reshape(-1, 2)

    @property
    def pack_map(self) -> np.ndarray:
        """u32[pack_grid, 2]: (frame, first tile) of every pack workgroup's MH_SET_PACK_TILES tiles."""
        t = self.totals
        return self.plan[t.pack_map_offset: t.pack_map_offset + 8 * t.pack_grid].view(np.uint32).reshape(-1, 2)


def set_sources(sources):
    """A ctypes array of mh_set_source from records or (pixels, row_pitch, pixel_stride, width, height,
    codes_cap[, reserved]) tuples."""
    sources = list(sources)
    arr = (N.mh_set_source * max(len(sources), 1))()
    for i, s in enumerate(sources):
        if isinstance(s, N.mh_set_source):
            arr[i] = s
        else:
            pixels, pitch, ps, w, h, cap = s[:6]
            arr[i] = N.mh_set_source(pixels, pitch, ps, w, h, s[6] if len(s) > 6 else 0, cap)
    return arr, len(sources)


def encode_set_plan(sources, flags: int = 0) -> SetPlan:
    """The host planner of the set encoder (mh_encode_set_plan; no GPU needed): from one source record
    per frame -- (pixels, row_pitch, pixel_stride, width, height, codes_cap) -- the plan blob the device
    reads and the set's totals. MHError carries the planner's code."""
    arr, n = set_sources(sources)
    L = N.lib()
    size = int(L.mh_encode_set_plan_bytes(n, arr))
    plan = np.zeros(max(size, 16), np.uint8)
    totals = N.mh_set_totals()
    N.check(L.mh_encode_set_plan(n, arr, flags, plan.ctypes.data, size, ctypes.byref(totals)), "mh_encode_set_plan")
    return SetPlan(plan[:size], totals)


class DecodeSetPlan(NamedTuple):
    """decode_set_plan's result, in the device's formats: what decode_set_frames uploads."""
    rasters: np.ndarray      # u32[n, 4]: mh_set_raster records (offset low, offset high, pitch, 0)
    shares: np.ndarray       # u32[n, 4]: mh_set_share records (first_group, groups, 0, 0)
    group_frame: np.ndarray  # u32[n_groups]: the frame of every workgroup of the launch
    n_groups: int
    out_bytes: int

    @property
    def offsets(self) -> np.ndarray:
        """int64[n]: each frame's byte offset into the output."""
        return self.rasters[:, 0].astype(np.int64) | (self.rasters[:, 1].astype(np.int64) << 32)

    @property
    def pitches(self) -> np.ndarray:
        return self.rasters[:, 2].astype(np.int64)


def decode_set_plan(geoms, group_budget: int, pitch_align: int = 0) -> DecodeSetPlan:
    """The host planner of decode_set_frames (mh_decode_set_plan; no GPU needed): from the set's
    geometry records u32[n, 4] (first_block, width, height, 0) the rasters laid out densely in frame
    order (pitch and offsets multiples of max(8, pitch_align)), and group_budget workgroups shared
    out in proportion to the frames' tiles, at least one and at most ceil(tiles / 8) per frame.
    MHError carries the planner's code."""
    g = np.ascontiguousarray(geoms, np.uint32).reshape(-1, 4)
    n = int(g.shape[0])
    L = N.lib()
    ng, ob = ctypes.c_uint32(0), ctypes.c_uint64(0)
    rc = L.mh_decode_set_plan(n, g.ctypes.data, group_budget, pitch_align, None, None, None, 0, ctypes.byref(ng),
                              ctypes.byref(ob))
    if rc != N.MH_ERR_CAPACITY:  # the sizing call's own answer; anything else is a refusal
        N.check(rc, "mh_decode_set_plan")
    rasters, shares = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.uint32)
    group_frame = np.zeros(ng.value, np.uint32)
    N.check(L.mh_decode_set_plan(n, g.ctypes.data, group_budget, pitch_align, rasters.ctypes.data, shares.ctypes.data,
                                 group_frame.ctypes.data, ng.value, ctypes.byref(ng), ctypes.byref(ob)),
            "mh_decode_set_plan")
    return DecodeSetPlan(rasters, shares, group_frame, int(ng.value), int(ob.value))


class Huffman:
    """Stateless mirror of the reference's `Huffman` class (Shared/Huffman.h)."""

    # +parseCanonicalHeader: (Huffman.h:14, HuffmanUtil.cpp:270-310)
    @staticmethod
    def parseCanonicalHeader(canonData) -> np.ndarray:
        canon = _u8(canonData)
        if canon.size != 256:
            raise ValueError("canonical header must be 256 bytes")
        codes = np.zeros(256, np.uint16)
        N.check(N.lib().mh_canonical_codes(_p(canon), _p(codes, _u16p)), "parseCanonicalHeader")
        return codes

    # +generateLookupTable:lookupTableNumEntries: (Huffman.h:18, HuffmanUtil.cpp:314-334)
    @staticmethod
    def generateLookupTable(canonData) -> np.ndarray:
        canon = _u8(canonData)
        table = np.zeros(65536 * 2, np.uint8)
        N.check(N.lib().mh_build_single_table(_p(canon), _p(table)), "generateLookupTable")
        return table

    # +generateSplitLookupTables:table2NumBits:table1:table2: (Huffman.h:21-24,
    # HuffmanUtil.cpp:338-667). Returns (T1, T2) as raw 2-byte-entry arrays.
    @staticmethod
    def generateSplitLookupTables(canonData, table1NumBits: int = 8, table2NumBits: int = 8):
        if (table1NumBits, table2NumBits) != (8, 8):
            # the reference's table sizes are the compile-time HUFF_TABLE{1,2}_SIZE
            # (AAPLShaderTypes.h:120-123); only the 8/8 split is a valid contract
            raise ValueError("only the 8+8 split (HUFF_TABLE1/2_NUM_BITS) is supported")
        canon = _u8(canonData)
        t1 = np.zeros(512, np.uint8)
        t2 = np.zeros(N.MH_TABLE2_MAX_ENTRIES * 2, np.uint8)
        ent = ctypes.c_uint32(0)
        N.check(N.lib().mh_build_tables(_p(canon), _p(t1), _p(t2), N.MH_TABLE2_MAX_ENTRIES,
                                        ctypes.byref(ent)), "generateSplitLookupTables")
        return t1, t2[: 2 * ent.value].copy()

    # +encodeHuffman:inNumBytes:outFileHeader:outCanonHeader:outHuffCodes:
    #  outBlockBitOffsets:width:height:blockDim: (Huffman.h:62-70, HuffmanUtil.cpp:1051-1131)
    @staticmethod
    def encodeHuffman(inBytes, width: int, height: int, blockDim: int = BLOCK_DIM):
        """-> (fileHeader, canonHeader, huffCodes, blockBitOffsets).

        fileHeader is empty, as in the reference (HuffmanUtil.cpp:1073-1086 never
        copies the encoder's header bytes out); huffCodes carries the encoder's
        2 zero bytes of read-ahead."""
        sym = _u8(inBytes)
        if sym.size == 0:
            raise N.MHError(-8, "encodeHuffman")
        cap = int(N.lib().mh_codes_bound(sym.size))
        canon = np.zeros(256, np.uint8)
        codes = np.zeros(cap, np.uint8)
        stride = blockDim * blockDim
        offs = np.zeros(max(1, sym.size // stride), np.uint32)
        ln = ctypes.c_uint64(0)
        N.check(N.lib().mh_encode_huffman(_p(sym), sym.size, blockDim, _p(canon), _p(codes), cap,
                                          ctypes.byref(ln), _p(offs, _u32p)), "encodeHuffman")
        return (np.zeros(0, np.uint8), canon, codes[: ln.value].copy(),
                offs[: sym.size // stride].copy())

    # +decodeHuffmanBits:numSymbolsToDecode:huffBuff:huffBuffN:outBuffer:bitOffsetTable:
    # (Huffman.h:30-35, HuffmanUtil.cpp:673-823). -> (symbols, bitOffsetTable)
    @staticmethod
    def decodeHuffmanBits(huffSymbolTable, numSymbolsToDecode: int, huffBuff, bitOffsets: bool = False):
        table = _u8(huffSymbolTable)
        if table.size != 65536 * 2:
            raise ValueError("the single lookup table has 65536 two-byte entries")
        buf = _u8(huffBuff)
        out = np.zeros(int(numSymbolsToDecode), np.uint8)
        offs = np.zeros(int(numSymbolsToDecode), np.uint32) if bitOffsets else None
        N.check(N.lib().mh_decode_huffman_bits(_p(table), out.size, _p(buf), buf.size, _p(out),
                                               _p(offs, _u32p) if offs is not None else None),
                "decodeHuffmanBits")
        return out, offs

    # +decodeHuffmanBitsFromTables:huffSymbolTable2:table1BitNum:table2BitNum:
    #  numSymbolsToDecode:huffBuff:huffBuffN:outBuffer:bitOffsetTable: (Huffman.h:42-50,
    # Huffman.mm:101, HuffmanUtil.cpp:830-1046). -> (symbols, bitOffsetTable)
    @staticmethod
    def decodeHuffmanBitsFromTables(huffSymbolTable1, huffSymbolTable2, table1BitNum: int,
                                    table2BitNum: int, numSymbolsToDecode: int, huffBuff,
                                    bitOffsets: bool = False):
        t1, t2, buf = _u8(huffSymbolTable1), _u8(huffSymbolTable2), _u8(huffBuff)
        if t1.size != 512:
            raise ValueError("T1 has 256 two-byte entries")
        out = np.zeros(int(numSymbolsToDecode), np.uint8)
        offs = np.zeros(int(numSymbolsToDecode), np.uint32) if bitOffsets else None
        N.check(N.lib().mh_decode_huffman_bits_from_tables(
            _p(t1), _p(t2), t2.size // 2, int(table1BitNum), int(table2BitNum), out.size, _p(buf), buf.size,
            _p(out), _p(offs, _u32p) if offs is not None else None), "decodeHuffmanBitsFromTables")
        return out, offs

    @staticmethod
    def containerHeader(n_symbols: int) -> np.ndarray:
        """The 8-byte header HuffmanEncoder::encode emits (HuffmanEncoder.cpp:326-340)
        and encodeHuffman drops: u32 LE 0xFFEEEEDD, u32 LE symbol count."""
        out = np.zeros(8, np.uint8)
        N.check(N.lib().mh_container_header(int(n_symbols), _p(out)), "containerHeader")
        return out

    @staticmethod
    def parseContainerHeader(header) -> int:
        """Symbol count of a container header (MHError on a wrong magic word)."""
        h = _u8(header)
        if h.size != 8:
            raise N.MHError(-1, "parseContainerHeader")
        n = ctypes.c_uint64(0)
        N.check(N.lib().mh_parse_container_header(_p(h), ctypes.byref(n)), "parseContainerHeader")
        return int(n.value)

    # +encodeSignedByteDeltas: / +decodeSignedByteDeltas: (Huffman.h:72-76)
    @staticmethod
    def encodeSignedByteDeltas(data) -> np.ndarray:
        a = _u8(data)
        out = np.empty_like(a)
        N.check(N.lib().mh_encode_signed_byte_deltas(_p(a), _p(out), a.size), "encodeSignedByteDeltas")
        return out

    @staticmethod
    def decodeSignedByteDeltas(deltas) -> np.ndarray:
        a = _u8(deltas)
        out = np.empty_like(a)
        N.check(N.lib().mh_decode_signed_byte_deltas(_p(a), _p(out), a.size), "decodeSignedByteDeltas")
        return out

    # snake_case aliases
    parse_canonical_header = parseCanonicalHeader
    generate_lookup_table = generateLookupTable
    generate_split_lookup_tables = generateSplitLookupTables
    encode_huffman = encodeHuffman
    decode_huffman_bits = decodeHuffmanBits
    decode_huffman_bits_from_tables = decodeHuffmanBitsFromTables
    encode_signed_byte_deltas = encodeSignedByteDeltas
    decode_signed_byte_deltas = decodeSignedByteDeltas


def split_blocks(img: np.ndarray, block_dim: int = BLOCK_DIM, zero_value: int = 0) -> np.ndarray:
    """Util.m:233-323 splitIntoBlocksOfSize (zero padded) -> block-order bytes."""
    img = _u8(img)
    h, w = img.shape
    bw, bh = block_grid(w, h, block_dim)
    out = np.empty(bw * bh * block_dim * block_dim, np.uint8)
    N.check(N.lib().mh_split_blocks(_p(img), w, h, block_dim, zero_value, _p(out), out.size),
            "split_blocks")
    return out


def merge_blocks(blocks: np.ndarray, width: int, height: int, block_dim: int = BLOCK_DIM) -> np.ndarray:
    blocks = _u8(blocks)
    out = np.empty((height, width), np.uint8)
    N.check(N.lib().mh_merge_blocks(_p(blocks), width, height, block_dim, _p(out), width),
            "merge_blocks")
    return out


def code_lengths_limited(freq, max_bits: int = 16) -> np.ndarray:
    """Code lengths (u8[256]) of at most `max_bits` bits from 256 symbol counts
    (mh_code_lengths_limited): the reference tree's where they fit, otherwise the
    optimal length-limited code (package-merge)."""
    f = np.ascontiguousarray(freq, dtype=np.uint64)
    if f.shape != (256,):
        raise ValueError("freq must hold 256 counts")
    lens = np.zeros(256, np.uint8)
    N.check(N.lib().mh_code_lengths_limited(f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(max_bits),
                                            _p(lens)), "code_lengths_limited")
    return lens


def frame_histogram(gray: np.ndarray, flags: int = 0, init_zero_delta: bool = False) -> np.ndarray:
    """uint64[256]: the counts of the symbols encode_frame would encode for this frame
    (mh_frame_histogram: split, per-block deltas unless MH_FLAG_NO_DELTA, the first delta
    of every block zeroed with init_zero_delta)."""
    gray = _u8(gray)
    if gray.ndim != 2:
        raise ValueError("expected a 2-D uint8 image")
    h, w = gray.shape
    freq = np.zeros(256, np.uint64)
    N.check(N.lib().mh_frame_histogram(_p(gray), w, h, flags, 1 if init_zero_delta else 0,
                                       freq.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), "frame_histogram")
    return freq


def shared_header(grays, flags: int = 0, init_zero_delta: bool = False, limit_lengths: bool = False) -> np.ndarray:
    """One canonical header (u8[256]) for all of `grays` (2-D uint8 images of any sizes):
    the reference tree of their summed symbol counts (mh_code_lengths), or with
    limit_lengths the code of at most 16 bits where that tree is deeper
    (mh_code_lengths_limited). What BatchEncoder.encode_shared_async builds on the device."""
    freq = np.zeros(256, np.uint64)
    for g in grays:
        freq += frame_histogram(g, flags, init_zero_delta)
    if limit_lengths:
        return code_lengths_limited(freq, 16)
    lens = np.zeros(256, np.uint8)
    N.check(N.lib().mh_code_lengths(freq.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _p(lens)), "shared_header")
    return lens


def encode_frame(gray: np.ndarray, flags: int = 0, init_zero_delta: bool = False,
                 limit_lengths: bool = False, header=None) -> EncodedFrame:
    """The renderer's producer step (AAPLRenderer.m:374-688) for one 8-bit frame.
    limit_lengths: a frame whose Huffman tree is deeper than 16 gets the length-limited
    code (MH_ENCODE_LIMIT_LENGTHS) instead of MHError -3; any other frame is unchanged.
    The keyword reaches the encoder only, never the frame's `flags`.
    header (u8[256], optional): encode under this canonical header instead of the frame's
    own tree (mh_encode_frame_with_header; e.g. shared_header of a batch). The returned
    frame's `canon` is that header; MHError -3 / -5 for a header that is no code, -5 when
    the frame holds a symbol the header has no code for. limit_lengths is then unused."""
    gray = _u8(gray)
    if gray.ndim != 2:
        raise ValueError("expected a 2-D uint8 image")
    h, w = gray.shape
    bw, bh = block_grid(w, h)
    nb = bw * bh
    cap = int(N.lib().mh_codes_bound(nb * 64)) + 2
    codes = np.zeros(cap, np.uint8)
    offs = np.zeros(nb, np.uint32)
    init = np.zeros(nb, np.uint8) if init_zero_delta else None
    ln = ctypes.c_uint64(0)
    if header is not None:
        canon = _u8(header).copy()
        if canon.shape != (256,):
            raise ValueError("header must hold 256 code lengths")
        N.check(N.lib().mh_encode_frame_with_header(_p(gray), w, h, flags, _p(canon), _p(codes), cap,
                                                    ctypes.byref(ln), _p(offs, _u32p),
                                                    _p(init) if init is not None else None),
                "encode_frame_with_header")
        return EncodedFrame(w, h, canon, codes[: ln.value].copy(), offs, init, flags)
    canon = np.zeros(256, np.uint8)
    enc_flags = flags | (N.MH_ENCODE_LIMIT_LENGTHS if limit_lengths else 0)
    if not N.has_mid_marks():  # an A/B variant library from older sources
        N.check(N.lib().mh_encode_frame(_p(gray), w, h, enc_flags, _p(canon), _p(codes), cap, ctypes.byref(ln),
                                        _p(offs, _u32p), _p(init) if init is not None else None),
                "encode_frame")
        return EncodedFrame(w, h, canon, codes[: ln.value].copy(), offs, init, flags)
    marks = np.zeros(nb, np.uint32)
    N.check(N.lib().mh_encode_frame_marks(_p(gray), w, h, enc_flags, _p(canon), _p(codes), cap, ctypes.byref(ln),
                                          _p(offs, _u32p), _p(init) if init is not None else None,
                                          _p(marks, _u32p)),
            "encode_frame")
    ef = EncodedFrame(w, h, canon, codes[: ln.value].copy(), offs, init, flags, marks)
    ef.marks_for = ef._buffers()
    return ef


def image_planes(images, first_channel: int = 0, n_planes=None, plane_major: bool = False) -> np.ndarray:
    """The plane frames of interleaved images, in the frame order of
    BatchEncoder.encode_images_async (mh_encode_images_device_async): uint8 [n, H, W, K] (or one
    [H, W, K] image) -> contiguous [n * C, H, W], plane c being byte first_channel + c of every
    pixel and C = n_planes (default: every channel from first_channel on). Plane c of image i
    is frame i * C + c, or c * n + i with plane_major. The definition the encoder's tests
    compare against: its output is encode_frame of each of these frames."""
    a = np.asarray(images)
    if a.dtype != np.uint8 or a.ndim not in (3, 4):
        raise ValueError("expected uint8 images [n, H, W, K] or one image [H, W, K]")
    if a.ndim == 3:
        a = a[None]
    n, h, w, k = a.shape
    c = k - first_channel if n_planes is None else int(n_planes)
    if first_channel < 0 or c < 1 or first_channel + c > k:
        raise ValueError(f"planes {first_channel}..{first_channel + c - 1} of {k}-channel pixels")
    planes = a[..., first_channel:first_channel + c].transpose((3, 0, 1, 2) if plane_major else (0, 3, 1, 2))
    return np.ascontiguousarray(planes).reshape(n * c, h, w)


def decode_frame_cpu(ef: EncodedFrame, threads: int = 1) -> np.ndarray:
    """CPU twin of the GPU decode for one frame (mh_decode_frame_cpu): the shader
    semantics per block, straight to the H x W raster, on `threads` host threads."""
    t1, t2 = ef.tables()
    out = np.zeros((ef.height, ef.width), np.uint8)
    offs = np.ascontiguousarray(ef.block_offsets, np.uint32)
    init = np.ascontiguousarray(ef.block_init, np.uint8) if ef.block_init is not None else None
    N.check(N.lib().mh_decode_frame_cpu(_p(offs, _u32p), _p(ef.codes), ef.codes.size, _p(t1), _p(t2),
                                        t2.size // 2, _p(init) if init is not None else None, ef.width,
                                        ef.height, ef.flags, _p(out), ef.width, int(threads)),
            "mh_decode_frame_cpu")
    return out


def check_frame(ef: EncodedFrame) -> tuple:
    """CPU twin of decoder.check_headers for one frame (mh_check_frame_cpu): the reference walk of
    every block under the table of ef.canon, over ef.codes as the frame's slot. Returns (status,
    report): the header's verdict (0, -3 or -5) and the report u32[4] = (zero-width lookups, 0,
    blocks whose codes miss the next block's offset, first offending block or 0xFFFFFFFF); a
    rejected header leaves the clean report."""
    offs = np.ascontiguousarray(ef.block_offsets, np.uint32)
    codes = np.ascontiguousarray(ef.codes, np.uint8)
    canon = np.ascontiguousarray(ef.canon, np.uint8)
    if canon.size != 256:
        raise ValueError("a canonical header is 256 code lengths")
    report = np.zeros(4, np.uint32)
    rc = N.lib().mh_check_frame_cpu(_p(offs, _u32p), offs.size, _p(codes), codes.size, _p(canon), _p(report, _u32p))
    if rc not in (0, -3, -5):
        N.check(rc, "mh_check_frame_cpu")
    return int(rc), report


def box_reduce(img: np.ndarray, log2_scale: int) -> np.ndarray:
    """The H x W image at scale s = 2^log2_scale (0..3) -> u8[ceil(H / s), ceil(W / s)]: every
    s x s cell's mean over its pixels inside the image, halves rounded up (mh_box_reduce, the CPU
    twin of decode_region_scaled's output stage)."""
    img = _u8(img)
    if img.ndim != 2 or img.size == 0:
        raise ValueError("expected a non-empty 2-D uint8 image")
    k = int(log2_scale)
    if k != log2_scale or not 0 <= k <= 3:
        raise ValueError(f"log2_scale must be 0, 1, 2 or 3, not {log2_scale!r}")
    h, w = img.shape
    s = 1 << k
    out = np.empty(((h + s - 1) // s, (w + s - 1) // s), np.uint8)
    N.check(N.lib().mh_box_reduce(_p(img), w, h, w, k, _p(out), out.shape[1]), "mh_box_reduce")
    return out


NORM_FORMATS = {"float16": N.MH_NORM_F16, "bfloat16": N.MH_NORM_BF16, "float32": N.MH_NORM_F32}


def norm_format(dtype_or_format) -> int:
    """MH_NORM_* of a format number, a numpy or torch dtype, or its name ("float16", "bfloat16",
    "float32"); ValueError for anything else."""
    if isinstance(dtype_or_format, (int, np.integer)) and not isinstance(dtype_or_format, bool):
        if int(dtype_or_format) in NORM_FORMATS.values():
            return int(dtype_or_format)
        raise ValueError(f"format must be 0 (float16), 1 (bfloat16) or 2 (float32), not {dtype_or_format!r}")
    name = str(dtype_or_format).rsplit(".", 1)[-1]  # "torch.bfloat16", "float16", dtype('float32')
    if name not in NORM_FORMATS:
        try:
            name = np.dtype(dtype_or_format).name
        except TypeError:
            pass
    if name not in NORM_FORMATS:
        raise ValueError(f"no normalised output format for {dtype_or_format!r}: float16, bfloat16 or float32")
    return NORM_FORMATS[name]


def finite_f32(x: float) -> bool:
    """x is finite once rounded to float32 (the midpoint above the largest float32 rounds to inf)."""
    return x == x and abs(x) < 2.0 ** 128 - 2.0 ** 103


def norm_table(dtype_or_format, scale: float, bias: float) -> np.ndarray:
    """The 256 elements decode_crops_normalized can write, T[v] = cvt(fmaf(float32(v), scale, bias))
    (mh_norm_table, the CPU twin of the kernel's conversion): float16 or float32 values, and for
    bfloat16 the uint16 bit patterns. scale and bias are rounded to float32 first and must be finite."""
    fmt = norm_format(dtype_or_format)
    scale, bias = float(scale), float(bias)
    if not (finite_f32(scale) and finite_f32(bias)):
        raise ValueError(f"scale and bias must be finite in float32, not {scale!r}, {bias!r}")
    out = np.empty(256, (np.float16, np.uint16, np.float32)[fmt])
    N.check(N.lib().mh_norm_table(fmt, scale, bias, out.ctypes.data_as(ctypes.c_void_p), out.nbytes), "mh_norm_table")
    return out


def norm_coefficients(mean, std) -> tuple:
    """(scale, bias) of decode_crops_normalized_planes for [0, 1] pixels normalised by a mean and a
    standard deviation per channel: per channel the float32 values of 1 / (255 * std) and -mean / std,
    computed in double and rounded once. mean and std are sequences of one length (or two numbers).
    ValueError for a zero or non-finite std, a non-finite mean, or a result that is not finite in float32."""
    m = np.atleast_1d(np.asarray(mean, np.float64))
    s = np.atleast_1d(np.asarray(std, np.float64))
    if m.ndim != 1 or m.shape != s.shape or m.size < 1:
        raise ValueError("mean and std are sequences of one length, one value per channel")
    if not np.isfinite(s).all() or (s == 0).any():
        raise ValueError(f"std must be finite and not zero, not {s.tolist()!r}")
    if not np.isfinite(m).all():
        raise ValueError(f"mean must be finite, not {m.tolist()!r}")
    scale, bias = (1.0 / (255.0 * s)).tolist(), (-m / s).tolist()
    if not all(finite_f32(v) for v in scale + bias):
        raise ValueError(f"scale and bias must be finite in float32, not {scale!r}, {bias!r}")
    return [float(np.float32(v)) for v in scale], [float(np.float32(v)) for v in bias]
