"""Frames and expectations shared by the mid-block marks' tests (CPU and GPU)."""
from __future__ import annotations

import numpy as np

import helpers as H


def padded_blocks(img: np.ndarray) -> np.ndarray:
    """u8[NB, 64]: the zero-padded 8x8 blocks of img in block order."""
    h, w = img.shape
    bh, bw = -(-h // 8), -(-w // 8)
    pad = np.zeros((bh * 8, bw * 8), np.uint8)
    pad[:h, :w] = img
    return np.ascontiguousarray(pad.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(bh * bw, 64))


def expected_marks(img: np.ndarray, canon: np.ndarray, no_delta: bool, with_init: bool) -> np.ndarray:
    """The marks from the picture and the code lengths alone: bits = the lengths of the block's
    first 32 symbols, prev = pixel 31 of the padded block (0 without deltas)."""
    blk = padded_blocks(img)
    if no_delta:
        sym, prev = blk, np.zeros(len(blk), np.uint32)
    else:
        sym = blk.copy()
        sym[:, 1:] = blk[:, 1:] - blk[:, :-1]
        if with_init:
            sym[:, 0] = 0
        prev = blk[:, 31].astype(np.uint32)
    bits = canon.astype(np.uint32)[sym[:, :32]].sum(axis=1).astype(np.uint32)
    return (bits | (prev << 16)).astype(np.uint32)


def deep_code_image(width: int = 128, height: int = 64, seed: int = 3) -> np.ndarray:
    """Deltas with a Fibonacci histogram over 17 symbols: codes of 15 and 16 bits (the two-level table)."""
    return H.image_from_block_deltas(H.fibonacci_deltas(17, width * height, seed), width, height)


def flat8_deltas_image(width: int, height: int, seed: int) -> np.ndarray:
    """A picture whose per-block deltas hold every byte value equally often: the flat 8-bit code."""
    d = H.exactly_uniform_image(width, height, seed).reshape(-1)
    return H.image_from_block_deltas(d, width, height)


def high_entropy_header() -> np.ndarray:
    """A complete code that gives the byte values 0..127 thirteen bits... and the rest what is left:
    128 codes of 13 bits are 2^-6 of the code space, so a picture of those values alone costs 13
    bits per symbol -- 104 bytes per block, over 3 KB in 32 blocks. The remaining space goes to
    symbols 128..255: one code of 1 bit, then lengths 2..6 and fillers that close the Kraft sum."""
    lens = np.zeros(256, np.uint8)
    lens[:128] = 13
    # 1 - 2^-6 = 1/2 + 1/4 + 1/8 + 1/16 + 1/32 + 1/64: one code each of 1..6 bits
    for k in range(6):
        lens[128 + k] = k + 1
    assert sum(2.0 ** -int(v) for v in lens if v) == 1.0
    return lens
