"""Helpers of the scaled-windows tests (test_gpu_windows_scaled.py): the expectation of a window at
scale 2^k -- scaled_helpers.box_reduce_np of the window's crop of the oracle's full-frame decode --
and one decode through decode_windows_scaled into slots prefilled with FILL."""
from __future__ import annotations

import numpy as np

import region_helpers as R
import scaled_helpers as S
from region_helpers import FILL


def window_region(win, size):
    return (int(win[1]), int(win[2]), size[0], size[1])


def decode_windows_scaled_host(device, fr, tabs, windows, size, k, **kw):
    """decode_windows_scaled into slots prefilled with FILL -> u8[n, bh c, bw c] on the host (and the
    per-window status list when status=True is passed)."""
    import torch
    from metalhuffman_amd import decoder as D
    c = 8 >> k
    out = torch.full((len(windows), c * size[1], c * size[0]), FILL, dtype=torch.uint8, device=device)
    got = D.decode_windows_scaled(fr, tabs, windows, size, k, out=out, **kw)
    torch.cuda.synchronize(device)
    if kw.get("status") is True:
        assert got[0] is out
        return out.cpu().numpy(), got[1].cpu().tolist()
    assert got is out
    return out.cpu().numpy()


def check_windows_scaled(got, windows, size, k, wants, width=R.W, height=R.H):
    """Slot p holds the reduced crop of window p's frame in rows < SH_p, columns < SW_p, zeros in
    columns SW_p .. bw c - 1 of those rows, and the fill in every row >= SH_p."""
    c = 8 >> k
    assert got.shape == (len(windows), c * size[1], c * size[0]), got.shape
    for p, win in enumerate(windows):
        region = window_region(win, size)
        sw, sh, cols = S.scaled_size(region, k, width, height)
        assert cols == c * size[0]
        exp = S.expected_scaled(wants[int(win[0])], region, k, width, height)
        assert exp.shape == (sh, sw)
        if not np.array_equal(got[p, :sh, :sw], exp):
            ys, xs = np.nonzero(got[p, :sh, :sw] != exp)
            raise AssertionError(f"window {p} = {tuple(win)} of {size}, k {k}: {ys.size} wrong pixel(s), first at "
                                 f"row {int(ys[0])}, column {int(xs[0])}: {int(got[p, ys[0], xs[0]])}, expected "
                                 f"{int(exp[ys[0], xs[0]])}")
        assert (got[p, :sh, sw:] == 0).all(), f"window {p} = {tuple(win)}, k {k}: columns >= SW = {sw} are not 0"
        assert (got[p, sh:] == FILL).all(), f"window {p} = {tuple(win)}, k {k}: rows >= SH = {sh} were written"
