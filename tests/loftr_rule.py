"""The coarse selection rule of LoFTR's `get_coarse_match` (no masks, eval mode) stated in numpy -- the yardstick of mve_dsmax_select.

A pair (i, j) of image pair b is kept when
  1. conf[b, i, j] > thr                                     (strictly: a value equal to thr is not a match),
  2. neither cell lies within `border` cells of its grid's edge (mask_border: rows / columns [0, border) and [size - border, size) of both grids),
  3. conf[b, i, j] equals the maximum of row i and the maximum of column j (mutual nearest neighbours),
and a row with several such j -- only possible with exactly equal floats -- keeps the lowest (`mask.max(dim=2)` returns the first maximum).
Matches come out in ascending (b, i) order, as `torch.where` lists them."""
import numpy as np


def border_ok(size_hw, border):
    """bool [H*W]: the cells at least `border` away from every edge."""
    H, W = size_hw
    ok = np.ones((H, W), dtype=bool)
    if border > 0:
        ok[:border] = False
        ok[-border:] = False
        ok[:, :border] = False
        ok[:, -border:] = False
    return ok.reshape(-1)


def coarse_matches(conf, hw0, hw1, thr=0.2, border=2):
    """conf float [N, L, S] -> (b_ids, i_ids, j_ids int64 [M], mconf [M] in conf's dtype)."""
    conf = np.asarray(conf)
    N, L, S = conf.shape
    assert L == hw0[0] * hw0[1] and S == hw1[0] * hw1[1]
    mask = conf > conf.dtype.type(thr)                             # the threshold in conf's own precision, as the kernel and torch compare
    mask &= border_ok(hw0, border)[None, :, None] & border_ok(hw1, border)[None, None, :]
    mask &= (conf == conf.max(axis=2, keepdims=True)) & (conf == conf.max(axis=1, keepdims=True))
    b_ids, i_ids = np.nonzero(mask.any(axis=2))
    j_ids = mask.argmax(axis=2)[b_ids, i_ids]                      # the first True of the row
    return b_ids.astype(np.int64), i_ids.astype(np.int64), j_ids.astype(np.int64), conf[b_ids, i_ids, j_ids]


def coarse_keypoints(ids, width, scale=8.0):
    """(x, y) * scale of cell ids on a grid `width` cells wide, float32 [M, 2]."""
    ids = np.asarray(ids)
    return (np.stack([ids % width, ids // width], axis=1) * scale).astype(np.float32)
