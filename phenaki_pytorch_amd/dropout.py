"""Dropout of the training kernels: the host side of the keep function in csrc/common.hpp (`drop_keys`, `drop_row`, `drop_word`, `drop_keep`).

The decision for element (row, col) of a dropout site depends on (seed, offset, row, col) only -- never on a tile shape, a wave layout or the
dispatch branch of the kernel that asks:

    k0, k1 = drop_keys(seed, offset)                        # per site, computed on the host
    word   = mix32(mix32(row ^ k0) + 0x9e3779b9 * (col >> 2) + k1)
    keep   = ((word >> 8 * (col & 3)) & 255) >= thr         # thr = round(256 p): 8 bits per decision

`row` / `col` are the two factors of the logical element index row * cols + col: attention row = (s * heads + h) * n + i and col = j over the
nnull + n_kv keys (null keys first, the layout of the reference's softmax row, attention.py:177); feed-forward row = token row and col over the
true inner width F (attention.py:45-52).  One 32-bit word serves the 4 consecutive columns of a group, which is what a lane of the attention
forward kernel and of the backward kernel that forms S^T holds.

`quantize` is the ONE place where the realised drop probability p_eff = thr / 256 and the survivor scale 1 / (1 - p_eff) are computed; the kernels
get (thr, scale).  |p_eff - p| <= 2^-9, and because survivors are scaled by 1 / (1 - p_eff), not 1 / (1 - p), the expectation is exact.
The masks are statistically equivalent to torch's nn.Dropout, not torch's stream.

`keep_mask` is the NumPy mirror of the device function (pk_dropout_mask must agree with it byte for byte: tests/test_dropout_gpu.py).
"""
import numpy as np

_M32 = np.uint32(0xFFFFFFFF)


def quantize(p):
    """drop probability p in [0, 1] -> (thr, p_eff, scale): keep iff an 8-bit draw >= thr; p_eff = thr / 256; scale = 1 / (1 - p_eff) (0 if p_eff = 1)"""
    p = float(p)
    if not 0. <= p <= 1.:
        raise ValueError(f'dropout probability has to be between 0 and 1, but got {p}')
    thr = int(round(p * 256.))
    p_eff = thr / 256.
    return thr, p_eff, (1. / (1. - p_eff) if thr < 256 else 0.)


def _mix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85ebca6b)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xc2b2ae35)
    h ^= h >> np.uint32(16)
    return h


def drop_keys(seed, offset):
    """(seed, offset) of a dropout site (64-bit each) -> the two 32-bit keys of its stream"""
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over='ignore'):
        k0 = _mix32(np.uint32(seed & 0xFFFFFFFF) ^ _mix32(np.uint32((offset + 0x9e3779b9) & 0xFFFFFFFF)))
        hi = np.uint32(((seed >> 32) + 0x85ebca6b * ((offset >> 32) + 1)) & 0xFFFFFFFF)
        k1 = _mix32(hi + k0)
    return int(k0), int(k1)


def keep_mask(seed, offset, rows, cols, p):
    """(rows, cols) uint8, 1 = keep: the decisions of the logical index range [0, rows) x [0, cols) of the site (seed, offset) at drop probability p"""
    thr = quantize(p)[0]
    k0, k1 = drop_keys(seed, offset)
    with np.errstate(over='ignore'):
        rowh = _mix32(np.arange(rows, dtype=np.uint32) ^ np.uint32(k0))[:, None]
        grp = np.arange((cols + 3) // 4, dtype=np.uint32)[None, :]
        word = _mix32(rowh + np.uint32(0x9e3779b9) * grp + np.uint32(k1))             # (rows, groups)
    shifts = (np.arange(4, dtype=np.uint32) * np.uint32(8))[None, None, :]
    draws = (word[:, :, None] >> shifts) & np.uint32(255)
    return (draws.reshape(rows, -1)[:, :cols] >= np.uint32(thr)).astype(np.uint8)
