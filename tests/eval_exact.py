"""Kernel-by-kernel checking of the evaluation kernels (csrc/eval.hip): the clip resize with its running minimum and the conditional
de-normalisation, the TF-SAME max pooling, the weighted row pooling, the activation moments, PSNR / SSIM and the best-of-n SSIM phase by
phase on the stored workspace, the sample statistics, both diversity scores, the uint8 export and the VGG input normalisation.
References, restatements, operand generators and the case tables; the test functions are in test_eval_kernels_cpu.py (which pins the
references against the reference-named functions, checks that the case tables reach their branches and measures the yardsticks) and
test_eval_kernels_gpu.py (which runs the kernels through the C ABI).

* References are plain functions that compute in the dtype of their operands: float64 operands give the reference, the same operands
  cast to float32 (``restate``) the fp32 restatement, which never calls the library.  Operands are rounded to the type the kernel reads
  first (``f32r``, ``as_seen``).
* Fenced buffers: every buffer a kernel receives lies between two runs of FENCE sentinel elements (``fenced``), rows are wider than
  their payload and the pitch differs per operand; ``check_fence`` verifies afterwards that the sentinels on both sides and in the
  padding columns are intact.  Inputs are compared with a copy taken before the call.
* Exact where the arithmetic is: max pooling, copies, integer and dyadic families, minima / maxima, uint8, indices, refusals.
* Everything else in ulps of the output type; a sum in ulps of the sum of its terms' magnitudes (the ``mag`` a reference returns).
  Phases that a workspace stores (mm, sse, the per-tile SSIM sums) are each checked on the stored values of the phase before.

  Recorded yardsticks (worst fp32 restatement error over the case tables, rounded up) and the GPU bound max(4 x yardstick, 4):

      output         yardstick  GPU bound   unit
      resize         2          8           ulp_f32 of sum |weight| |pixel| over the four taps
      pool_rows      1.5        6           ulp_f32 of sum |w_k| |x_k|; a bf16 output adds one bf16 ulp of the value (its own rounding:
                                            half an ulp of the fp32 sum, which may lie one binade above the reference)
      ssim_tile      22         88          ulp_f32 of the tile's number of positions: an SSIM value is O(1) and its fp32 error is the
                                            cancellation of E[x^2] - mu^2, which the restatement shares
      time_cosine    5          20          ulp_f32 of mean over the locations of sum_t |u_j| |u_k|

  Derived bounds (the kernel sums in double, so no restatement is needed):

      moments        (n + 2) 2^-53 sum |term| / divisor: the two differences and the product (or the fused multiply-add) of a term, the
                     serial double sum over at most n rows and the division; mu against sum |a| / n, sigma on the STORED mu against
                     sum |(a_i - mu_i)(a_j - mu_j)| / (n - 1).  The reference is numpy long double.
      sse            n 2^-53 sse: a chain of at most n double additions of non-negative terms (per thread, across the wave, atomics)
      psnr, ssim, sample_ssim per frame, sample_stats sd / mean, pair_mse: 1 fp32 ulp of the float64 value of the stored phase before
                     (a double result, whose own error is ~1e-16 relative, rounded once to fp32; the ulp is the reference's, which
                     covers a result in the binade below)
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

from ipoke_amd import _lib, fvd
from oracle.metrics_ref import _gaussian
from tests.conv_exact import round_up  # noqa: F401
from tests.disc_exact import DTYPES, F64, SENT, assert_close_ulp, assert_same, randint64, ulp_of  # noqa: F401
from tests.flow_exact import assert_units, err_units, f32r  # noqa: F401
from tests.sn_exact import as_seen, restate  # noqa: F401

F32 = torch.float32
BF16 = torch.bfloat16
FENCE = 64                    # sentinel elements in front of and behind every buffer
U8_SENT = 0xA5
I32_SENT = -12345

# worst error of the fp32 restatement against float64, in the unit of the docstring (test_eval_kernels_cpu.py asserts them)
YARDSTICK = {"resize": 2.0, "pool_rows": 1.5, "ssim_tile": 22.0, "time_cosine": 5.0}


def gpu_bound(key):
    return max(4.0 * YARDSTICK[key], 4.0)


# ------------------------------------------------------------------ fenced buffers
def fill_of(dtype):
    return U8_SENT if dtype == torch.uint8 else I32_SENT if dtype == torch.int32 else SENT


def fenced(rows, ld, dtype, device, values=None, fill=None):
    """(whole, body): body is the [rows][ld] view of a flat buffer [FENCE | rows * ld | FENCE] filled with the dtype's sentinel; values
    ([rows][c <= ld]) go to the first columns.  The kernel receives body's address."""
    fill = fill_of(dtype) if fill is None else fill
    whole = torch.full((2 * FENCE + rows * ld,), fill, dtype=dtype, device=device)
    body = whole[FENCE: FENCE + rows * ld].view(rows, ld)
    if values is not None:
        assert values.shape[0] == rows and values.shape[1] <= ld, (values.shape, rows, ld)
        body[:, : values.shape[1]] = values.to(dtype)
    return whole, body


def check_fence(whole, rows, ld, cols, what, fill=None):
    """both fences and the columns >= cols of every row still hold the sentinel"""
    fill = fill_of(whole.dtype) if fill is None else fill
    w = whole.to(F64).cpu()
    assert bool((w[:FENCE] == fill).all()), f"{what}: write in front of the buffer"
    assert bool((w[FENCE + rows * ld:] == fill).all()), f"{what}: write behind the buffer"
    assert bool((w[FENCE: FENCE + rows * ld].view(rows, ld)[:, cols:] == fill).all()), f"{what}: write into the columns >= {cols} of the pitch"


def bits32(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ resize, running minimum, de-normalisation
def src_index(ni, no):
    """ATen's source index for align_corners=True as upsample_bilinear2d computes it in fp32: scale = (ni - 1) / (no - 1) (0 when no is
    1), real = scale * o, index = trunc(real), lambda = real - index.  Returns (i0, i1, lambda as float64)"""
    scale = np.float32(ni - 1) / np.float32(no - 1) if no > 1 else np.float32(0.0)
    real = (scale * np.arange(no, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(real.astype(np.int64), ni - 1)
    i1 = np.minimum(i0 + 1, ni - 1)
    lam = (real - i0.astype(np.float32)).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(lam.astype(np.float64))


def resize_ref(x, Ho, Wo):
    """x [frames][C][Hi][Wi] -> (value, mag) [frames][Ho][Wo][C]: the four-term blend (1 - wy) ((1 - wx) a + wx b) + wy ((1 - wx) c + wx d)
    in the dtype of x, with the fp32 weights of src_index"""
    Hi, Wi = x.shape[2:]
    y0, y1, wy = src_index(Hi, Ho)
    x0, x1, wx = src_index(Wi, Wo)
    wy, wx = wy.to(x.dtype).view(1, 1, Ho, 1), wx.to(x.dtype).view(1, 1, 1, Wo)
    g = lambda v, yy, xx: v[:, :, yy][:, :, :, xx]                                      # noqa: E731
    blend = lambda v: ((1 - wy) * ((1 - wx) * g(v, y0, x0) + wx * g(v, y0, x1)) +       # noqa: E731
                       wy * ((1 - wx) * g(v, y1, x0) + wx * g(v, y1, x1)))
    return blend(x).permute(0, 2, 3, 1).contiguous(), blend(x.abs()).permute(0, 2, 3, 1).contiguous()


def stem_pads(Wo):
    """(pad_l, pad_r) as I3D._clip_rows stores the stem's TF-SAME padding along W"""
    pad_l, pad_r = fvd._same(Wo, 7, 2, False)
    return pad_l, max(pad_r, 2 * (-(-Wo // 2) - 1) + 7 - pad_l - Wo)


ResizeCase = collections.namedtuple("ResizeCase", "name N T C Hi Wi Ho Wo pads layout exact")
RESIZE_CASES = [
    ResizeCase("5to9", 2, 2, 3, 5, 5, 9, 9, (2, 3), "perm", True),
    ResizeCase("3to5", 1, 2, 1, 3, 3, 5, 5, (0, 0), "contig", True),
    ResizeCase("9to17xid", 1, 1, 3, 9, 4, 17, 4, "stem", "slice", True),
    ResizeCase("up", 2, 2, 3, 7, 10, 12, 23, "stem", "perm", False),
    ResizeCase("up-c1", 1, 3, 1, 7, 10, 12, 23, (0, 0), "contig", False),
    ResizeCase("down", 2, 1, 3, 12, 23, 7, 10, (2, 3), "slice", False),
    ResizeCase("down-c1", 1, 2, 1, 12, 23, 7, 10, "stem", "perm", False),
    ResizeCase("ho1", 1, 2, 3, 7, 10, 1, 23, (2, 3), "contig", False),
    ResizeCase("wo1", 2, 1, 3, 7, 10, 12, 1, (0, 0), "slice", False),
]


def resize_pads(c):
    return stem_pads(c.Wo) if c.pads == "stem" else c.pads


def resize_operands(c, family=None, seed=0):
    """clip [N][T][C][Hi][Wi] as float64: integers in +-8 (exact cases), reals in [-1, 1]; family 'pos' in [0.25, 1], 'neg' in
    [-1, -0.25], 'nzero' all -0.0, 'pzero' all +0.0"""
    gen = torch.Generator().manual_seed(2000 + seed + c.Hi * 31 + c.Wo)
    shape = (c.N, c.T, c.C, c.Hi, c.Wi)
    if family == "nzero":
        return torch.full(shape, -0.0, dtype=F64)
    if family == "pzero":
        return torch.zeros(shape, dtype=F64)
    if family in ("pos", "neg"):
        x = f32r(0.25 + 0.75 * torch.rand(shape, generator=gen, dtype=F64))
        return x if family == "pos" else -x
    if c.exact:
        return randint64(-8, 8, shape, gen)
    return f32r(torch.rand(shape, generator=gen, dtype=F64) * 2 - 1)


def denorm_ref(x):
    """(x + 1) / 2: in fp32 one rounded addition and an exact halving"""
    return (x + 1.0) / 2.0


# ------------------------------------------------------------------ max pooling, TF SAME
POOL_GEOMS = [((1, 3, 3), (1, 2, 2), (4, 14, 14)), ((3, 3, 3), (2, 2, 2), (8, 12, 12)), ((3, 3, 3), (2, 2, 2), (7, 9, 9)),
              ((2, 2, 2), (2, 2, 2), (4, 14, 14)), ((2, 2, 2), (2, 2, 2), (3, 7, 7)), ((3, 3, 3), (1, 1, 1), (4, 7, 7))]
POOL_CHANNELS = [("bf16", 8), ("f32", 4), ("bf16", 24), ("f32", 24)]
POOL_N = 2


def pool_dims(N, C, dhw, k, s):
    """(dims[20], odhw) as I3D._pool builds them: front padding, padded extents, MaxPool3d(ceil_mode=True) output extents"""
    pads = [fvd._same(e, kk, ss, i == 0) for i, (e, kk, ss) in enumerate(zip(dhw, k, s))]
    odhw = []
    for e, kk, ss, (pf, pb) in zip(dhw, k, s, pads):
        pe = e + pf + pb
        o = -(-(pe - kk) // ss) + 1
        if (o - 1) * ss >= pe:
            o -= 1
        odhw.append(o)
    return [N, C, *dhw, *odhw, *k, *s, *(p[0] for p in pads), *(e + p[1] for e, p in zip(dhw, pads))], tuple(odhw)


def pool_operands(C, dhw, tdtype, negative=False, seed=0):
    """[N][C][D][H][W] float64 as the kernel's type holds it; negative: every value below zero"""
    gen = torch.Generator().manual_seed(2100 + seed + C + dhw[0] * 7 + dhw[1])
    x = torch.randn(POOL_N, C, *dhw, generator=gen, dtype=F64) - 0.5
    if negative:
        x = -x.abs() - 0.125
    return as_seen(x, tdtype)


def pool_ref(x, k, s):
    """zero padding (TF SAME, the remainder rule on the time axis only), then MaxPool3d(ceil_mode=True): [N][C][Do][Ho][Wo]"""
    pads = [fvd._same(e, kk, ss, i == 0) for i, (e, kk, ss) in enumerate(zip(x.shape[2:], k, s))]
    xp = F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
    return F.max_pool3d(xp, k, s, ceil_mode=True)


def to_rows(x):
    """[N][C][D][H][W] -> channels-last rows [N*D*H*W][C]"""
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1])


# ------------------------------------------------------------------ weighted row pooling
RowsCase = collections.namedtuple("RowsCase", "G S C")
ROWS_CASES = [RowsCase(1, 1, 5), RowsCase(3, 98, 5), RowsCase(1, 147, 1024), RowsCase(3, 147, 5), RowsCase(3, 98, 1024)]
ROWS_WEIGHTS = ["trunk", "cancel"]


def trunk_weights(S):
    """the fp32 weights I3D._trunk builds for Tf = S / 49 time steps (S == 1: the single weight 1)"""
    if S == 1:
        return torch.ones(1, dtype=F32)
    Tf = S // 49
    assert Tf * 49 == S and Tf >= 2
    wt = torch.zeros(Tf)
    for t in range(Tf - 1):
        wt[t] += 0.5; wt[t + 1] += 0.5
    return (wt / (Tf - 1)).repeat_interleave(49) / 49.0


def rows_operands(c, tdtype, weights):
    """x [G * S][C], w [S]: float64 as the kernel reads them"""
    gen = torch.Generator().manual_seed(2200 + c.G + c.S + c.C)
    x = as_seen(torch.randn(c.G * c.S, c.C, generator=gen, dtype=F64) * 2 + 0.5, tdtype)
    if weights == "trunk":
        return x, trunk_weights(c.S).to(F64)
    w = f32r(torch.randn(c.S, generator=gen, dtype=F64))
    w[1::2] = -w[: c.S // 2].abs()                         # signed: neighbours cancel
    w[0::2] = w[0::2].abs()
    return x, w


def pool_rows_ref(x, w, G):
    """y[g][c] = sum_k w[k] x[g * S + k][c]; (value, mag)"""
    S = w.numel()
    t = w.view(1, S, 1) * x.view(G, S, -1)
    return t.sum(1), t.abs().sum(1)


# ------------------------------------------------------------------ activation moments
MomCase = collections.namedtuple("MomCase", "name n D shift nan_rows part_nan")
MOM_CASES = [
    MomCase("n2", 2, 1, 0.0, (), ()),
    MomCase("d65", 37, 65, 0.0, (5,), ((7, 3),)),          # row 5 all NaN (dropped), row 7 NaN in column 3 only (kept)
    MomCase("n300", 300, 65, 0.0, (299,), ()),             # second block of the valid-row kernel
    MomCase("d400", 37, 400, 0.0, (), ((0, 399),)),
    MomCase("shifted", 37, 65, 1e4, (), ()),               # column means 1e4, unit spread
    MomCase("one-valid", 2, 5, 0.0, (0,), ()),
    MomCase("none-valid", 2, 5, 0.0, (0, 1), ()),
]


def mom_operands(c):
    gen = torch.Generator().manual_seed(2300 + c.n + c.D)
    a = torch.randn(c.n, c.D, generator=gen, dtype=F64) * (1.0 if c.shift else 3.0) + torch.randn(c.D, generator=gen, dtype=F64) + c.shift
    a = f32r(a)
    for r in c.nan_rows:
        a[r] = float("nan")
    for r, col in c.part_nan:
        a[r, col] = float("nan")
    return a


def moments_mean_ref(a):
    """a float64 [n][D] -> (valid [n] bool, mu, mag) as numpy long double: rows with no non-NaN entry dropped; mean from the definition"""
    A = a.numpy().astype(np.longdouble)
    valid = ~np.isnan(A).all(axis=1)
    V = A[valid]
    n = V.shape[0]
    with np.errstate(all="ignore"):
        mu = V.sum(0) / np.longdouble(n)
        mag = np.abs(V).sum(0) / np.longdouble(max(n, 1))
    return valid, mu, mag


def moments_cov_ref(a, mu):
    """the unbiased covariance around the GIVEN mu (long double): (sigma, mag); the degrees of freedom clamp at 0 as np.cov's"""
    A = a.numpy().astype(np.longdouble)
    V = A[~np.isnan(A).all(axis=1)]
    n = V.shape[0]
    Vc = V - np.asarray(mu, dtype=np.longdouble)[None]
    with np.errstate(all="ignore"):
        dof = np.longdouble(max(n - 1, 0))
        return (Vc.T @ Vc) / dof, (np.abs(Vc).T @ np.abs(Vc)) / np.longdouble(max(n - 1, 1))


def moments_bound(n):
    return (n + 2) * 2.0 ** -53


# ------------------------------------------------------------------ PSNR / SSIM
SSIM_SHAPES = [(1, 11, 11), (2, 42, 42), (3, 43, 75), (2, 74, 42), (300, 11, 12)]      # planes, H, W
SSIM_RANGES = ["sym-preds", "unit-target"]          # [-1, 1] with preds' range the larger, [0, 1] with target's the larger
MM_EDGES = ["all-negative", "pzero-darkest", "nzero-darkest", "constant"]
SSIM_EDGES = ["identical", "constant-target", "constant-identical"]
EDGE_SHAPE = (2, 11, 12)


def ssim_tiles(H, W):
    return -(-(H - 10) // 32), -(-(W - 10) // 32)


def image_operands(shape, kind, seed=0):
    """(preds, target) [planes][H][W] float64 of fp32 values"""
    gen = torch.Generator().manual_seed(2400 + seed + shape[0] + 3 * shape[1] + 5 * shape[2])
    r = lambda: torch.rand(shape, generator=gen, dtype=F64)                          # noqa: E731
    if kind == "sym-preds":
        t = r() * 2 - 1
        a, b = torch.clamp(t + 0.2 * (r() * 2 - 1), -1, 1), 0.8 * t
    elif kind == "unit-target":
        b = r()
        a = 0.1 + 0.8 * torch.clamp(b + 0.1 * (r() - 0.5), 0, 1)
    elif kind == "all-negative":
        a, b = -0.25 - 0.5 * r(), -0.125 - 0.75 * r()
    elif kind in ("pzero-darkest", "nzero-darkest"):
        a, b = 0.25 + 0.5 * r(), 0.125 + 0.75 * r()
        z = 0.0 if kind == "pzero-darkest" else -0.0
        a[0, 3, 4] = z; a[-1, 10, 11] = z; b[0, 0, 0] = z
    elif kind == "constant":
        a, b = torch.full(shape, 0.375, dtype=F64), torch.full(shape, -0.5, dtype=F64)
    elif kind == "identical":
        a = r() * 2 - 1
        b = a.clone()
    elif kind == "constant-target":
        a, b = r() * 2 - 1, torch.full(shape, 0.25, dtype=F64)
    elif kind == "constant-identical":
        a = torch.full(shape, 0.25, dtype=F64)
        b = a.clone()
    else:
        raise KeyError(kind)
    return f32r(a), f32r(b)


def mm_ref(a, b):
    """{-min a, max a, -min b, max b} as fp32 (the negation keeps the sign of a zero minimum reversed)"""
    return torch.stack([-a.min(), a.max(), -b.min(), b.max()]).to(F32)


def range_of_mm(mm):
    """the fp32 data range the SSIM kernels form from a stored mm row: max(mm[1] + mm[0], mm[3] + mm[2]) (fp32 tensor [..])"""
    mm = mm.to(F32)
    return torch.maximum(mm[..., 1] + mm[..., 0], mm[..., 3] + mm[..., 2])


def sse_ref(a, b):
    """sum of fl32(x - y)^2: the kernel rounds the difference to fp32 and squares and adds in double"""
    d = (a.to(F32) - b.to(F32)).to(F64)
    return (d * d).sum()


def psnr_ref(mm, sse, n):
    """10 log10(range^2 / mse) from the stored mm and sse, in the kernel's form 10 (2 ln range - ln mse) / ln 10 (float64)"""
    rng = mm[3].to(F64) + mm[2].to(F64)
    return 10.0 * (2.0 * torch.log(rng) - torch.log(sse.to(F64) / n)) / math.log(10.0)


def ssim_map_ref(a, b, rng):
    """a, b [P][H][W], rng 0-dim or [P]: the SSIM map [P][H - 10][W - 10] over the positions whose 11 x 11 window lies inside the image
    (eval_ref.ssim_map's arithmetic -- reflection padding and the crop cancel -- with the data range given), in the dtype of a"""
    dt = a.dtype
    rng = rng.to(dt).reshape(-1, 1, 1)
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    g = _gaussian(11, 1.5, dt)
    kernel = torch.matmul(g.t(), g).view(1, 1, 11, 11)
    P = a.shape[0]
    o = F.conv2d(torch.cat((a, b, a * a, b * b, a * b)).unsqueeze(1), kernel).squeeze(1)
    o = [o[i * P:(i + 1) * P] for i in range(5)]
    maa, mbb, mab = o[0] * o[0], o[1] * o[1], o[0] * o[1]
    upper = 2 * (o[4] - mab) + c2
    lower = (o[2] - maa) + (o[3] - mbb) + c2
    return ((2 * mab + c1) * upper) / ((maa + mbb + c1) * lower)


def tile_sums(m):
    """[P][Ho][Wo] -> (sums, positions) [P][tiles_y * tiles_x] of the 32 x 32 tiles, in the workspace's order"""
    P, Ho, Wo = m.shape
    ty, tx = -(-Ho // 32), -(-Wo // 32)
    pad = F.pad(m, (0, tx * 32 - Wo, 0, ty * 32 - Ho))
    cnt = F.pad(torch.ones_like(m), (0, tx * 32 - Wo, 0, ty * 32 - Ho))
    red = lambda v: v.view(P, ty, 32, tx, 32).sum((2, 4)).reshape(P, ty * tx)      # noqa: E731
    return red(pad), red(cnt)


# ------------------------------------------------------------------ best-of-n SSIM
SsCase = collections.namedtuple("SsCase", "bs ns s C H W")
SS_CASES = [SsCase(3, 3, 2, 3, 11, 11), SsCase(3, 1, 1, 1, 43, 44), SsCase(3, 3, 1, 1, 43, 44), SsCase(3, 1, 2, 3, 11, 11)]


def ss_operands(c):
    """pred [bs][ns][s][C][H][W], target [bs][1][s][C][H][W] (float64 of fp32 values), every target plane distinct; example 0: preds'
    range wins, example 1: target's wins, example 2: both are exactly [-1, 1]"""
    gen = torch.Generator().manual_seed(2500 + c.ns * 7 + c.s * 3 + c.C + c.H)
    t = torch.rand(c.bs, 1, c.s, c.C, c.H, c.W, generator=gen, dtype=F64) * 2 - 1
    p = 0.8 * t + 0.2 * (torch.rand(c.bs, c.ns, c.s, c.C, c.H, c.W, generator=gen, dtype=F64) * 2 - 1)
    t[0] *= 0.5
    p[1] *= 0.5
    for v in (p[2], t[2]):
        v.reshape(-1)[0], v.reshape(-1)[-1] = -1.0, 1.0
    return f32r(p), f32r(t)


def ss_offsets(bs):
    """byte offset of the partials in ipoke_sample_ssim's workspace"""
    return -(-16 * bs // 64) * 64


# ------------------------------------------------------------------ sample statistics
STATS_CASES = [(1, 1, 3), (3, 2, 1), (2, 65, 4), (2, 3, 65), (3, 5, 7)]              # bs, ns, s


def stats_operands(bs, ns, s):
    gen = torch.Generator().manual_seed(2600 + bs + 3 * ns + 5 * s)
    return f32r(torch.rand(bs, ns, s, generator=gen, dtype=F64) * 0.5 + 0.4)


def stats_tie_operands():
    """[2][4][2]: example 0 holds the lowest sample row twice (rows 1 and 3: the first wins); example 1 a near-tie -- row 0 = {1, 1 + 2^-23},
    row 1 = {1, 1}: both fp32 means are 1.0 (a reference computing them in fp32 takes row 0), the double means differ and row 1 is lower"""
    v = torch.full((2, 4, 2), 2.0, dtype=F64)
    v[0, 1] = v[0, 3] = torch.tensor([0.5, 0.75], dtype=F64)
    v[0, 0] = torch.tensor([0.75, 0.75], dtype=F64)
    v[1, 0] = torch.tensor([1.0, 1.0 + 2.0 ** -23], dtype=F64)
    v[1, 1] = 1.0
    return v


def stats_ref(v):
    """float64 [bs][ns][s] -> dict(nn, sd, mean [bs][s], index [bs]); the first index wins a tie; ns == 1: sd NaN"""
    bs, ns, s = v.shape
    means = v.sum(2) / s
    idx = torch.argmin(means, 1)
    mu = v.sum(1) / ns
    sd = torch.sqrt(((v - mu[:, None]) ** 2).sum(1) / (ns - 1)) if ns > 1 else torch.full((bs, s), float("nan"), dtype=F64)
    return dict(nn=v[torch.arange(bs), idx], sd=sd, mean=mu, index=idx.to(torch.int32))


# ------------------------------------------------------------------ pairwise MSE
PairCase = collections.namedtuple("PairCase", "n_ex ns L")
PAIR_CASES = [PairCase(2, 2, 1), PairCase(2, 23, 63), PairCase(1, 24, 64), PairCase(2, 64, 65), PairCase(700, 3, 320)]


def pair_operands(c, integer):
    gen = torch.Generator().manual_seed(2700 + c.ns + c.L)
    if integer:
        return randint64(-16, 16, (c.n_ex, c.ns, c.L), gen)
    return f32r(torch.rand(c.n_ex, c.ns, c.L, generator=gen, dtype=F64) * 2 - 1)


def pair_mse_ref(x):
    """float64 [n_ex][ns][L] -> [n_ex][ns][ns] of mean((v_j - v_k)^2)"""
    return ((x[:, :, None] - x[:, None, :]) ** 2).sum(-1) / x.shape[-1]


def pair_blocks(c):
    """blocks per example, from the host-only workspace query"""
    P = c.ns * (c.ns - 1) // 2
    ws = int(_lib.lib().ipoke_pair_mse_workspace_bytes(c.n_ex, c.ns, c.L))
    assert ws % (8 * c.n_ex * P) == 0
    return ws // (8 * c.n_ex * P)


# ------------------------------------------------------------------ time cosine
TcCase = collections.namedtuple("TcCase", "ns s HW C family")
TC_REG_CASES = [TcCase(ns, s, *((8, 9) if (ns + s) % 2 else (40, 25)), "relu") for ns in range(2, 9) for s in (1, 15, 16)]
TC_LDS_CASES = [TcCase(9, 15, 8, 9, "relu"), TcCase(20, 16, 40, 25, "relu"), TcCase(40, 16, 8, 9, "relu"), TcCase(64, 16, 40, 25, "relu"),
                TcCase(64, 32, 8, 9, "relu"), TcCase(9, 1, 40, 25, "relu")]
TC_LDS_WIDTHS = [64, 32, 16, 8, 4, 64]                       # the tile width each LDS case takes (test_eval_kernels_cpu.py derives them)
TC_TINY_CASES = [TcCase(3, 2, 8, 9, "tiny"), TcCase(9, 2, 8, 9, "tiny")]
TC_REFUSED = (64, 64)
E1, E2 = float(np.float32(1e-10)), float(np.float32(1e-8))   # the kernel's fp32 constants


def tc_id(c):
    return f"ns{c.ns}-s{c.s}-L{c.HW * c.C}-{c.family}"


def tc_operands(c, tdtype):
    """[ns][s][HW * C] float64 as the kernel's type holds it.  relu: max(randn, 0) with every fifth location zero in every frame of
    every sample and every seventh zero in the frames of sample 0 only; tiny: |x| ~ 1e-15 on the even locations (|u| ~ 1e-5: the
    + 1e-10 matters) and ~ 5e-19 on the odd ones (|u| < 1e-8: the max(., 1e-8) branch), no square subnormal"""
    L = c.HW * c.C
    gen = torch.Generator().manual_seed(2800 + c.ns * 11 + c.s + L)
    x = torch.randn(c.ns, c.s, L, generator=gen, dtype=F64)
    if c.family == "relu":
        x = torch.clamp(x, min=0)
        x[:, :, 0::5] = 0
        x[0, :, 0::7] = 0
    else:
        x = torch.sign(x) * (0.5 + torch.rand(c.ns, c.s, L, generator=gen, dtype=F64))
        x[:, :, 0::2] *= 1e-15
        x[:, :, 1::2] *= 5e-19
    return as_seen(x, tdtype)


def time_cosine_ref(x):
    """x [ns][s][L] -> (D [ns][ns] with a zero diagonal, mag): per location u = x / (|x|_2 + 1e-10) over time, then the cosine of ATen's
    CosineSimilarity(eps=1e-8), (u_j / max(|u_j|, eps)) . (u_k / max(|u_k|, eps)); the mean over the locations"""
    dt = x.dtype
    e1, e2 = torch.tensor(E1, dtype=F64).to(dt), torch.tensor(E2, dtype=F64).to(dt)
    u = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + e1)
    w = u / torch.maximum(torch.sqrt((u * u).sum(1, keepdim=True)), e2)
    ns, L = x.shape[0], x.shape[2]
    flat = w.reshape(ns, -1)
    off = 1 - torch.eye(ns, dtype=dt)
    return (flat @ flat.t()) / L * off, (flat.abs() @ flat.abs().t()) / L


def tc_blocks(ns, s, C, HW):
    """partial blocks of a launch, from the host-only workspace query (0: refused)"""
    return int(_lib.lib().ipoke_time_cosine_workspace_bytes(ns, s, C, HW)) // (8 * (ns * (ns - 1) // 2))


# ------------------------------------------------------------------ uint8 export
U8_FRAMES = 5


def u8_lattice():
    """for every m in 0 .. 255 the fp32 number nearest m / 127.5 - 1 and its two fp32 neighbours (where one fused multiply-add and two
    rounded operations truncate differently), then values beyond both ends, +-inf and NaN: float32 [776]"""
    mid = (np.arange(256, dtype=np.float64) / 127.5 - 1.0).astype(np.float32)
    lat = np.stack([np.nextafter(mid, np.float32(-2)), mid, np.nextafter(mid, np.float32(2))], 1).reshape(-1)
    extra = np.array([-1.5, 2.0, -1e30, 1e30, 1.0078431, -np.inf, np.inf, np.nan], dtype=np.float32)
    return torch.from_numpy(np.concatenate([lat, extra]))


def u8_operands(hw):
    """x float32 [U8_FRAMES][3][hw]: the lattice first, reals in [-1, 1] behind it"""
    gen = torch.Generator().manual_seed(2900 + hw)
    x = torch.rand(U8_FRAMES * 3 * hw, generator=gen) * 2 - 1
    lat = u8_lattice()
    x[: lat.numel()] = lat
    return x.view(U8_FRAMES, 3, hw)


def u8_ref(x):
    """numpy's ((x + 1.) * 127.5).astype(np.uint8) where it is defined; beyond [0, 255] the clamp the header states, NaN -> 0;
    [frames][3][hw] -> uint8 [frames][hw][3]"""
    with np.errstate(all="ignore"):
        v = (x.numpy() + np.float32(1.0)) * np.float32(127.5)
        v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(255)))
    return torch.from_numpy(v.astype(np.uint8)).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------ VGG input normalisation
VGG_SHAPES = [(2, 5, 7), (2, 16, 16)]


def vgg_operands(N, H, W):
    gen = torch.Generator().manual_seed(3000 + H)
    return torch.rand(N, 3, H, W, generator=gen) * 2 - 1
