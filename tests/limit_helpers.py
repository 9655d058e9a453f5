"""Helpers of the length-limited code tests (CPU and GPU): two Python statements of
package-merge, seeded histograms whose Huffman trees are deeper than 16, and frames
with a given symbol histogram."""
from __future__ import annotations

import numpy as np

from helpers import image_of_symbols

FORMATS = {  # name -> (no_delta, init_zero_delta)
    "delta": (False, False),
    "no_delta": (True, False),
    "init_byte": (False, True),
}


def sorted_leaves(freq):
    """The present symbols by (count, symbol) -> (symbols, counts as Python ints)."""
    f = [int(x) for x in np.asarray(freq).reshape(256)]
    syms = sorted((s for s in range(256) if f[s]), key=lambda s: (f[s], s))
    return syms, [f[s] for s in syms]


def textbook_package_merge(freq, max_bits: int) -> np.ndarray:
    """Package-merge with explicit item sets (Larmore & Hirschberg's coin collector as
    textbooks state it): an item is (weight, how often each leaf is in it); level 1 holds
    the leaves; every further level holds the leaves and the packages (pairs in weight
    order) of the level before; the 2n - 2 lightest items of the last level are bought,
    and a leaf's length is the number of bought items that hold it, each as often as it
    holds it. -> u8[256]."""
    syms, w = sorted_leaves(freq)
    n = len(syms)
    lens = np.zeros(256, np.uint8)
    if n == 1:
        lens[syms[0]] = 1
    if n < 2:
        return lens
    assert (1 << max_bits) >= n and sum(w) * max_bits < 2 ** 62
    leaf_w = np.array(w, np.int64)
    leaf_set = np.eye(n, dtype=np.int64)
    W, S = leaf_w, leaf_set
    for _ in range(2, max_bits + 1):
        k = W.size // 2
        W = np.concatenate([leaf_w, W[0:2 * k:2] + W[1:2 * k:2]])
        S = np.concatenate([leaf_set, S[0:2 * k:2] + S[1:2 * k:2]])
        order = np.argsort(W, kind="stable")
        W, S = W[order], S[order]
    assert W.size >= 2 * n - 2
    per_leaf = S[: 2 * n - 2].sum(axis=0)
    lens[np.array(syms)] = per_leaf
    return lens


def normative_lengths(freq, max_bits: int) -> np.ndarray:
    """The rule of DESIGN.md "Length-limited codes", restated: level lists of weights only
    (a leaf first on equal weight, packages in their order, a trailing odd item dropped),
    then backwards from t = 2n - 2: a_l leaves among the first t items of list_l,
    t <- 2 (t - a_l); the leaf of rank r gets #{l : a_l > r}. Python integers. -> u8[256]."""
    syms, w = sorted_leaves(freq)
    n = len(syms)
    lens = np.zeros(256, np.uint8)
    if n == 1:
        lens[syms[0]] = 1
    if n < 2:
        return lens
    assert (1 << max_bits) >= n
    lists = [None, [(x, True) for x in w]]            # (weight, is a leaf)
    for l in range(2, max_bits + 1):
        prev = lists[l - 1]
        packs = [prev[2 * j][0] + prev[2 * j + 1][0] for j in range(len(prev) // 2)]
        merged, i, j = [], 0, 0
        while i < n or j < len(packs):
            if i < n and (j >= len(packs) or w[i] <= packs[j]):
                merged.append((w[i], True))
                i += 1
            else:
                merged.append((packs[j], False))
                j += 1
        lists.append(merged)
    t = 2 * n - 2
    out = [0] * n
    for l in range(max_bits, 0, -1):
        assert t <= len(lists[l])
        a = sum(1 for _, leaf in lists[l][:t] if leaf)
        for r in range(a):
            out[r] += 1
        t = 2 * (t - a)
    assert t == 0
    lens[np.array(syms)] = out
    return lens


def kraft16(lens) -> int:
    c = np.asarray(lens).astype(np.int64)
    c = c[c > 0]
    return int((1 << (16 - c)).sum())


def cost(freq, lens) -> int:
    return sum(int(f) * int(l) for f, l in zip(np.asarray(freq).reshape(256), np.asarray(lens).reshape(256)))


def fibonacci_counts(n: int, scale: int = 1, first=(1, 1)) -> list:
    a, b = first
    out = []
    for _ in range(n):
        out.append(a * scale)
        a, b = b, a + b
    return out


def chain_histogram() -> np.ndarray:
    """All 256 symbols: 239 of count 1 and 17 whose counts follow a, b <- b, a + b from
    (239, 239); 999,259 symbols, the commonest is symbol 0. The level lists of the limiter
    reach their 511 items."""
    f = np.ones(256, np.uint64)
    f[:17] = fibonacci_counts(17, 1, (239, 239))[::-1]
    assert int(f.sum()) == 999_259
    return f


def deal(counts, r, top_first: bool = False) -> np.ndarray:
    """The counts on random distinct symbols (top_first: the largest on symbol 0)."""
    counts = sorted((int(c) for c in counts), reverse=True)
    f = np.zeros(256, np.uint64)
    if top_first:
        syms = np.concatenate([[0], 1 + r.permutation(255)[: len(counts) - 1]])
    else:
        syms = r.permutation(256)[: len(counts)]
    f[syms] = np.array(counts, np.uint64)
    return f


def limit_histograms(seed: int = 16) -> list:
    """(name, u64[256]) for the test against the textbook: Fibonacci shapes over 18..40
    symbols, geometric tails over all 256, Pareto-random counts, counts up to 2^40, and
    the 256-symbol chain."""
    r = np.random.default_rng(seed)
    out = []
    for n in range(18, 41):
        for k in range(3):
            scale = int(r.integers(1, 50)) if k else 1
            out.append((f"fib{n}_{k}", deal(fibonacci_counts(n, scale), r)))
    for k in range(40):
        ratio = float(r.uniform(0.55, 0.97))
        top = float(2.0 ** r.uniform(20, 45))
        c = np.maximum(1, top * ratio ** np.arange(256)).astype(np.uint64)
        c = c + r.integers(0, 3, 256).astype(np.uint64)
        out.append((f"geo{k}", deal(c, r)))
    for k in range(50):
        n = int(r.integers(2, 257))
        c = np.minimum(np.floor(r.pareto(float(r.uniform(0.15, 0.6)), n)) + 1, 2.0 ** 40).astype(np.uint64)
        out.append((f"pareto{k}", deal(c, r)))
    for k in range(49):
        n = int(r.integers(2, 257))
        c = (2.0 ** r.uniform(0, 40, n)).astype(np.uint64) + np.uint64(1)
        out.append((f"wide{k}", deal(c, r)))
    out.append(("chain", chain_histogram()))
    return out


def symbols_from_histogram(freq, width: int, height: int, seed: int = 0) -> np.ndarray:
    """A symbol stream in block order (64 per 8x8 block) for a width x height frame whose
    histogram is `freq`, the rest of the frame filled with the commonest symbol, shuffled;
    where it has a symbol per block it also opens every block, so the init-byte format
    (which moves a block's first delta out and codes a zero in its place) keeps the
    histogram when that symbol is 0."""
    assert width % 8 == 0 and height % 8 == 0
    f = np.asarray(freq).astype(np.int64).copy()
    nb = (width // 8) * (height // 8)
    top = int(np.argmax(f))
    rest = nb * 64 - int(f.sum())
    assert rest >= 0, "the frame is too small for the histogram"
    f[top] += rest
    r = np.random.default_rng(seed)
    if f[top] < nb:
        body = np.repeat(np.arange(256, dtype=np.uint8), f)
        r.shuffle(body)
        return body
    f[top] -= nb
    body = np.repeat(np.arange(256, dtype=np.uint8), f)
    r.shuffle(body)
    sym = np.empty((nb, 64), np.uint8)
    sym[:, 0] = top
    sym[:, 1:] = body.reshape(nb, 63)
    return sym.reshape(-1)


def image_from_histogram(freq, width: int, height: int, seed: int = 0, *, no_delta: bool = False) -> np.ndarray:
    """A raster whose producer step (split, per-block deltas unless no_delta) yields
    symbols_from_histogram(freq, ...): the symbols are the pixels in block order for a
    no-delta frame, and the running sums of each block otherwise."""
    return image_of_symbols(symbols_from_histogram(freq, width, height, seed), width, height, no_delta=no_delta)


def frame_histogram(img, *, no_delta: bool = False, init_zero_delta: bool = False) -> np.ndarray:
    """u64[256]: the histogram of the symbols the encoder codes for img (multiples of 8)."""
    h, w = img.shape
    blocks = img.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    if not no_delta:
        blocks = np.diff(np.concatenate([np.zeros((blocks.shape[0], 1), np.uint8), blocks], axis=1).astype(np.int16),
                         axis=1).astype(np.uint8)
        if init_zero_delta:
            blocks = blocks.copy()
            blocks[:, 0] = 0
    return np.bincount(blocks.reshape(-1), minlength=256).astype(np.uint64)


def huffman_depth(counts) -> int:
    """The deepest leaf of the reference tree (mh_code_lengths) over these counts."""
    from metalhuffman_amd import _native as N
    f = np.zeros(256, np.uint64)
    f[: len(counts)] = np.array(counts, np.uint64)
    canon = np.zeros(256, np.uint8)
    N.lib().mh_code_lengths(f.ctypes.data_as(N._u64p), canon.ctypes.data_as(N._u8p))
    return int(canon.max())


def fib_counts_within(n: int, total: int) -> list:
    """n counts of a tree deeper than 16 that sum to at most `total`: the Fibonacci counts
    (1, 1, 2, 3, ...) where they fit; otherwise the longest Fibonacci run that fits (18 counts
    need 6,764 symbols, depth 17), grown to n counts by splitting one count in two, the
    largest count first, wherever the tree keeps its depth. Deterministic."""
    k = n
    while sum(fibonacci_counts(k)) > total:
        k -= 1
    c = fibonacci_counts(k)
    assert k >= 18
    while len(c) < n:
        for i, a in ((i, a) for i in sorted(range(len(c)), key=lambda i: -c[i]) for a in (1, 2, c[i] // 2)):
            t = sorted(c[:i] + c[i + 1:] + [a, c[i] - a])
            if 0 < a < c[i] and huffman_depth(t) >= 17:
                c = t
                break
        else:
            raise AssertionError(f"no deep histogram of {n} symbols within {total}")
    return c


def fib_histogram(n: int, total: int, seed: int = 0) -> np.ndarray:
    """fib_counts_within(n, total), the largest count on symbol 0, the others on random
    symbols (the frame builder gives the rest of the frame to symbol 0)."""
    return deal(fib_counts_within(n, total), np.random.default_rng(seed), top_first=True)


def batch_histograms(seed: int, n_frames: int = 64, nsym: int = 65536) -> list:
    """(kind, u64[256]) for one batched call of 256 x 256 frames: deep Fibonacci shapes
    (18..22 symbols, depth over 16), ordinary, one-symbol, two-symbol and uniform frames.
    The commonest symbol is 0 in every one."""
    r = np.random.default_rng(seed)
    out = []
    for i in range(n_frames):
        k = i % 16
        if k < 10:
            n = int(r.integers(18, 23))
            scale = nsym // (2 * sum(fibonacci_counts(n))) if r.integers(0, 2) else 1
            out.append(("deep", deal(fibonacci_counts(n, max(1, scale)), r, top_first=True)))
        elif k < 13:
            c = r.integers(1, 200, int(r.integers(3, 257)))
            out.append(("ordinary", deal(c, r, top_first=True)))
        elif k == 13:
            out.append(("one", deal([nsym], r, top_first=True)))
        elif k == 14:
            out.append(("two", deal([nsym - int(r.integers(1, 1000)), 1], r, top_first=True)))
        else:
            out.append(("uniform", np.full(256, nsym // 256, np.uint64)))
    return out
