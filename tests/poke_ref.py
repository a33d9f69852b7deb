"""numpy / float64 restatement of the poke editing of csrc/data.hip (``ipoke_poke_stamp``, ``ipoke_poke_randomize``), written from the
description in include/ipoke_hip.h: the slice rules, the stamping order, the candidate set, the pick mapping and the value formula.
tests/test_poke_edit_cpu.py pins the slice rules against Python's own slicing."""
import math

import numpy as np


def slice_range(c, half, extent):
    """start, stop of the slice c - half : c + half + 1 on an axis of ``extent`` elements; start >= stop is the empty slice"""
    out = []
    for v in (c - half, c + half + 1):
        if v < 0:
            v = max(v + extent, 0)
        out.append(min(v, extent))
    return out[0], out[1]


def covered(r, c, half, H, W):
    """boolean [H, W]: the pixels of the square around (r, c)"""
    y0, y1 = slice_range(int(r), half, H)
    x0, x1 = slice_range(int(c), half, W)
    m = np.zeros((H, W), dtype=bool)
    if y0 < y1 and x0 < x1:
        m[y0:y1, x0:x1] = True
    return m


def stamp(centers, half, H, W, values=None, flow=None, skip_negative=True):
    """centers int [B, n, 2]; values [B, n, 2] or flow [B, 2, H, W] -> poke [B, 2, H, W] of the values' dtype (copies only)"""
    centers = np.asarray(centers)
    B, n, _ = centers.shape
    src = values if values is not None else flow
    poke = np.zeros((B, 2, H, W), dtype=np.asarray(src).dtype)
    for b in range(B):
        for j in range(n):                                     # in order: a later poke overwrites an earlier one
            r, c = int(centers[b, j, 0]), int(centers[b, j, 1])
            if skip_negative and (r < 0 or c < 0):
                continue
            if values is None:
                if not (0 <= r < H and 0 <= c < W):            # no flow value outside the map
                    continue
                v = flow[b, :, r, c]
            else:
                v = values[b, j]
            poke[b][:, covered(r, c, half, H, W)] = np.asarray(v)[:, None]
    return poke


def amplitude(flow):
    """float64 2-norm over the channel of an fp32 flow [B, 2, H, W]"""
    f = np.asarray(flow, dtype=np.float64)
    return np.sqrt(f[:, 0] ** 2 + f[:, 1] ** 2)


def candidates(amp_b):
    """row-major (the order of ``nonzero``) pixels of one [H, W] amplitude map above its mean"""
    return np.argwhere(amp_b > amp_b.mean())


def randomize(flow, centers, half, u):
    """-> pokes float64 [n_s, B, 2, H, W], picked int64 [B, n_s, 2], status int32 [B], phase float64 [B, n_s]"""
    flow, centers, u = np.asarray(flow), np.asarray(centers), np.asarray(u)
    B, _, H, W = flow.shape
    n_s = u.shape[1]
    amp = amplitude(flow)
    pokes = np.zeros((n_s, B, 2, H, W))
    picked = np.full((B, n_s, 2), -1, dtype=np.int64)
    status = np.zeros(B, dtype=np.int32)
    phase = np.zeros((B, n_s))
    for b in range(B):
        cand = candidates(amp[b])
        r0, c0 = int(centers[b, 0, 0]), int(centers[b, 0, 1])
        if len(cand) == 0:
            status[b] = 1
            continue
        if r0 < 0 or c0 < 0:
            status[b] = 2
            continue
        where = covered(r0, c0, half, H, W)
        for j in range(n_s):
            k = min(int(math.floor(float(u[b, j, 0]) * len(cand))), len(cand) - 1)      # the fp32 uniform times the count, exactly
            y, x = cand[k]
            picked[b, j] = (y, x)
            phase[b, j] = amp[b, y, x]
            angle = math.pi * float(u[b, j, 1])
            pokes[j, b, 0][where] = math.cos(angle) * phase[b, j]
            pokes[j, b, 1][where] = math.sin(angle) * phase[b, j]
    return pokes, picked, status, phase
