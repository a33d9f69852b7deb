"""Bit-exact checking of the optimizer step and the weight-shadow refresh (csrc/prep.hip, csrc/elementwise.hip): the Adam-amsgrad
kernels, the weight-norm row statistics and backward, the relayout into the matrix-core operands and the multi-tensor row reductions.

* ctypes mirrors of the device job tables (RelayoutJob, WnJob, AdamTileJob, AdamSeg, ReduceEntry) and builders that number blocks, rows
  and tiles the way csrc/flow_engine.hip does (``block_start`` / ``row_start`` / ``tile_start`` prefix sums, the block -> job table).
* An exact fp32 emulation of ``adam_amsgrad_update`` (csrc/common.h).  The host part repeats ``adam_make_hyper``: ``pow`` in double on the
  float betas, ``lr / (float)bc1``, ``(float)sqrt(bc2)``.  The device part repeats the update operation by operation on float64 tensors
  that hold float32 values: + - * / and sqrt are computed in float64 and rounded to float32 -- double rounding cannot change these
  results because 53 >= 2 * 24 + 2 -- and ``fmaf`` takes the exact float64 product, a TwoSum for the addition, and a correction where the
  float64 sum lands exactly on a float32 midpoint (the only case in which rounding the rounded sum differs from rounding the exact one).
* Weight-norm operands for which every result is exact in any summation or contraction order: rows of v with few non-zero small
  integers whose squares sum to a power of four (``1 / ||v||`` is a power of two), gains with at most 8 significant bits, small-integer
  weight gradients.  The bf16 shadows then must equal round-to-nearest-even of the exact value, ties included.
* float64 reference layouts of the relayout (A and B operands, taps 1 / 6 / 9, padding, ``B_rows_real``, ``frag_tiled``) that describe
  the whole destination, padding zeros included, written into a copy of the sentinel-filled buffer.
* ``assert_same``: a bitwise comparator that names the first differing element through a caller-supplied locator.
"""
import ctypes
import math
from ctypes import c_int32, c_int64

import numpy as np
import torch

SENT = 4096.0                 # fills every element a launch must not touch (exact in bf16 and fp32)
F64 = torch.float64


# ------------------------------------------------------------------ job tables (mirrors of prep.hip / elementwise.hip)
class RelayoutJob(ctypes.Structure):
    _fields_ = [(n, c_int64) for n in ("src_off", "s_n", "s_k", "dstA", "dstB", "scale_off")] + [
        (n, c_int32) for n in ("taps", "n_real", "k_real", "A_rows_pad", "A_inner_pad", "B_rows_pad", "B_inner_pad", "B_rows_real",
                               "tile", "tiles_k", "block_start", "frag_tiled")]


class WnJob(ctypes.Structure):
    _fields_ = [("v_off", c_int64), ("g_off", c_int64), ("out_off", c_int64), ("rows", c_int32), ("K", c_int32), ("row_start", c_int32)]


class AdamTileJob(ctypes.Structure):
    _fields_ = [("src_off", c_int64), ("dstA", c_int64), ("dstB", c_int64), ("N", c_int32), ("K", c_int32), ("tile_start", c_int32),
                ("pad", c_int32)]


class AdamSeg(ctypes.Structure):
    _fields_ = [("off", c_int64), ("len", c_int64)]


class ReduceEntry(ctypes.Structure):
    _fields_ = [("src", c_int64), ("dst", c_int64), ("ld", c_int32), ("ncols", c_int32), ("rmul", c_int32), ("pad", c_int32)]


TABLE_SIZES = {RelayoutJob: "ipoke_relayout_job_size", WnJob: "ipoke_wn_job_size", AdamTileJob: "ipoke_adam_tile_job_size",
               AdamSeg: "ipoke_adam_seg_size", ReduceEntry: "ipoke_reduce_entry_size"}


def table_bytes(entries):
    """contiguous bytes of a list of ctypes structures (one device table)"""
    return b"".join(bytes(e) for e in entries)


def to_device(entries, device):
    buf = table_bytes(entries)
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(device)


def round_up(v, m):
    return (v + m - 1) // m * m


def relayout_job(src_off, s_n, s_k, taps, n_real, k_real, scale_off, dstA, A_rows_pad, A_inner_pad, dstB, B_rows_pad, B_inner_pad,
                 B_rows_real, frag_tiled=0):
    """one job as flow_engine.hip's relayout_pair builds it (block_start is filled in by relayout_table)"""
    tile = 64 if taps == 1 else 32
    n_ext, k_ext = max(A_rows_pad, B_inner_pad), max(A_inner_pad, B_rows_pad)
    tiles_k = (k_ext + tile - 1) // tile
    return RelayoutJob(src_off, s_n, s_k, dstA, dstB, scale_off, taps, n_real, k_real, A_rows_pad, A_inner_pad, B_rows_pad, B_inner_pad,
                       B_rows_real, tile, tiles_k, 0, frag_tiled)


def relayout_blocks(j):
    n_ext = max(j.A_rows_pad, j.B_inner_pad)
    return ((n_ext + j.tile - 1) // j.tile) * j.tiles_k


def relayout_table(jobs):
    """block_start prefix sums and the block -> job table (flow_engine.hip: ensure_device); returns (jobs, total blocks, block_job)"""
    nb = 0
    block_job = []
    for i, j in enumerate(jobs):
        j.block_start = nb
        b = relayout_blocks(j)
        block_job += [i] * b
        nb += b
    return jobs, nb, block_job


def wn_table(specs):
    """specs: (v_off, g_off, out_off, rows, K) -> WnJob list with the global row numbering (row_start)"""
    jobs, r = [], 0
    for v_off, g_off, out_off, rows, K in specs:
        jobs.append(WnJob(v_off, g_off, out_off, rows, K, r))
        r += rows
    return jobs, r


def adam_tile_table(specs):
    """specs: (src_off, dstA, dstB, N, K) -> AdamTileJob list with tile_start in 64 x 64 tiles (flow_engine.hip: relayout_pair)"""
    jobs, t = [], 0
    for src, dA, dB, N, K in specs:
        assert N % 64 == 0 and K % 64 == 0
        jobs.append(AdamTileJob(src, dA, dB, N, K, t, 0))
        t += (N // 64) * (K // 64)
    return jobs, t


# ------------------------------------------------------------------ fp32 arithmetic on float64 tensors
def rn(x):
    """round float64 to the nearest float32 (ties to even), kept as float64"""
    return x.to(torch.float32).to(F64)


def f32(x):
    """a Python float rounded to float32 (as the C ABI's float arguments are)"""
    return float(np.float32(x))


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 values held in float64 (a, b, c tensors or Python floats): a * b is exact in float64 (48 significant
    bits); s + e = a * b + c exactly (TwoSum); rounding s to float32 equals rounding the exact sum unless s lies exactly on a float32
    midpoint and e != 0, in which case the exact sum lies on e's side of the midpoint."""
    p = torch.as_tensor(a, dtype=F64) * b
    c = torch.as_tensor(c, dtype=F64)
    s, e = two_sum(p, c)
    r = s.to(torch.float32)
    r64 = r.to(F64)
    inexact = r64 != s
    if not bool(inexact.any()):
        return r64
    inf = torch.full_like(r, math.inf)
    other = torch.nextafter(r, torch.where(s > r64, inf, -inf))
    o64 = other.to(F64)
    tie = inexact & (s == (r64 + o64) * 0.5) & (e != 0)
    up = o64 > r64
    pick_other = tie & ((e > 0) == up)
    return torch.where(pick_other, o64, r64)


# ------------------------------------------------------------------ Adam-amsgrad
class Hyper:
    """adam_make_hyper (csrc/common.h) and the identical host code of ipoke_adam_amsgrad_step_grid"""

    def __init__(self, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
        b1, b2 = f32(beta1), f32(beta2)
        bc1 = 1.0 - math.pow(b1, step)            # pow in double on the float betas
        bc2 = 1.0 - math.pow(b2, step)
        self.lr_bc1 = f32(f32(lr) / f32(bc1))     # lr / (float)bc1: a float division
        self.bc2_sqrt = f32(math.sqrt(bc2))       # (float)sqrt(bc2)
        self.beta1, self.beta2, self.eps, self.wd, self.grad_scale = b1, b2, f32(eps), f32(weight_decay), f32(grad_scale)
        self.args = (f32(lr), b1, b2, f32(eps), f32(weight_decay), int(step), f32(grad_scale))


def adam_update(p, g, m, v, vx, h):
    """adam_amsgrad_update (csrc/common.h), operation by operation; float64 tensors holding float32 values -> (p, m, v, v_max)"""
    gr = fma32(h.wd, p, rn(g * h.grad_scale))
    m = fma32(h.beta1, m, rn(f32(1.0 - h.beta1) * gr))
    v = fma32(h.beta2, v, rn(rn(f32(1.0 - h.beta2) * gr) * gr))
    vx = torch.maximum(vx, v)
    denom = rn(rn(rn(torch.sqrt(vx)) / h.bc2_sqrt) + h.eps)
    p = fma32(-h.lr_bc1, rn(m / denom), p)
    return p, m, v, vx


def adam_state(n, gen, device="cpu", scale_g=1e-2):
    """p, g, m, v, v_max (float32) over n elements that cycle through the operand classes of the update:
    0 ordinary values with carried state, 1 zero gradient and zero state, 2 carried v_max > v (a gradient that flipped to small),
    3 gradients of 1e-20 (v and v_max in the denormal range), 4 gradients of 1e15 (large but finite g^2).
    In classes 1 and 3 the parameter is 0 / below 1e-19 too: weight decay adds wd * p to the gradient, and a normal-sized p would turn
    the zero gradient into a non-zero one and swamp the 1e-20 one (``assert_class_reaches`` checks what a launch's outputs cover)."""
    cls = torch.arange(n) % 5
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * scale_g
    m = torch.randn(n, generator=gen) * 1e-3
    v = torch.rand(n, generator=gen) * 1e-4
    vx = v + torch.rand(n, generator=gen) * 1e-5 * (torch.rand(n, generator=gen) < 0.5)
    z = cls == 1
    p[z] = 0.0; g[z] = 0.0; m[z] = 0.0; v[z] = 0.0; vx[z] = 0.0
    c2 = cls == 2
    g[c2] *= 1e-3; vx[c2] = v[c2] * 8.0 + 1e-6
    c3 = cls == 3
    p[c3] *= 1e-20; g[c3] = torch.sign(g[c3]) * 1e-20; m[c3] = torch.sign(m[c3]) * 1e-21; v[c3] = 1e-41; vx[c3] = 3e-41
    c4 = cls == 4
    g[c4] = torch.sign(g[c4]) * 1e15; m[c4] *= 1e12; v[c4] = 1e28; vx[c4] = 2e28
    return [t.to(torch.float32).to(device) for t in (p, g, m, v, vx)]


def operand_class(n):
    """the class of every element of an adam_state buffer"""
    return torch.arange(n) % 5


FLT_MIN = 2.0 ** -126


def assert_class_reaches(inputs, outputs, offset=0):
    """the operand classes of adam_state reach what they are there for, in the emulated outputs (p, m, v, v_max as float64) of one
    update of the inputs (p, g, m, v, v_max) over elements [offset, offset + len): class 1 runs on a zero gradient (g and wd * p both
    zero), class 3 leaves denormal v and v_max (so a kernel that flushed fp32 denormals would change bits), class 2 has v_max > v"""
    n = outputs[0].numel()
    cls = operand_class(offset + n)[offset:]
    p, g = inputs[0], inputs[1]
    z = cls == 1
    assert bool(z.any()) and bool((g[z] == 0).all() and (p[z] == 0).all()), "class 1: the gradient is not zero"
    c3 = cls == 3
    for name, t in (("v", outputs[2]), ("v_max", outputs[3])):
        x = t[c3].abs()
        assert int(((x > 0) & (x < FLT_MIN)).sum()) > 0, f"class 3: no denormal {name} among the outputs"
    c2 = cls == 2
    assert bool((outputs[3][c2] > outputs[2][c2]).any()), "class 2: v_max never above v"


# ------------------------------------------------------------------ weight norm: exact operands and formulas
def dense_pattern(K):
    """a ones and b twos, a + b = K - z (z <= 2 zeros), with a + 4 b = 4^e for the smallest 4^e >= K: a row whose every 4-group
    (every lane of the reductions) holds non-zeros while its sum of squares stays a power of four"""
    T = 1
    while T < K:
        T *= 4
    for z in range(3):
        nz = K - z
        if nz > 0 and (4 * nz - T) % 3 == 0 and 4 * nz >= T:
            a = (4 * nz - T) // 3
            return [1] * a + [2] * (nz - a)
    raise AssertionError(K)


def wn_rows(rows, K, gen, max_nz=16, dense_every=2):
    """[rows][K] float32 rows of v: small integers (random positions and signs) whose squares sum to 4^e, so ||v|| = 2^e and
    1 / ||v|| are exact.  Every dense_every-th row is dense (dense_pattern: ones and twos in every 4-group of the row), the others
    hold a few non-zeros (|x| <= 8); returns (v, e per row).  Use weight gradients with |dW| <= 3 (exact for K <= 2304)."""
    v = torch.zeros(rows, K)
    es = []
    patterns = [[1], [2], [4], [1, 1, 1, 1], [2, 2, 2, 2], [8], [4, 4, 4, 4], [1] * 16, [2, 2, 2, 2, 4, 4, 4], [6, 2, 2, 2, 2, 2, 2, 2]]
    for r in range(rows):
        if dense_every and r % dense_every == 0:
            pt = dense_pattern(K)
        else:
            cand = [pt for pt in patterns if len(pt) <= min(K, max_nz)]
            pt = cand[int(torch.randint(len(cand), (1,), generator=gen))]
        ss = sum(x * x for x in pt)
        e = int(round(math.log(ss, 4)))
        assert 4 ** e == ss, pt
        pos = torch.randperm(K, generator=gen)[:len(pt)]
        sg = torch.where(torch.rand(len(pt), generator=gen) < 0.5, -1.0, 1.0)
        v[r, pos] = torch.tensor(pt, dtype=torch.float32) * sg
        es.append(e)
    return v, es


def wn_gains(rows, gen):
    """gains with at most 8 significant bits: odd integers below 256 times 2^-6 .. 2^3, both signs"""
    mant = torch.randint(1, 128, (rows,), generator=gen) * 2 - 1
    ex = torch.randint(-6, 4, (rows,), generator=gen).to(torch.float32)
    sg = torch.where(torch.rand(rows, generator=gen) < 0.5, -1.0, 1.0)
    return (mant.to(torch.float32) * torch.pow(2.0, ex) * sg).to(torch.float32)


def wn_scale_ref(v, g):
    """(scale, inv_norm) of wn_scale_kernel: g / ||v||, 1 / ||v||, exact for wn_rows / wn_gains operands (float64)"""
    nrm = torch.sqrt((v.to(F64) ** 2).sum(1))
    return g.to(F64) / nrm, 1.0 / nrm


def wn_bwd_ref(v, g, dw, inv):
    """(dg, dv) of wn_bwd_kernel: dot = <dW_eff, v>, dg = dot / ||v||, dv = (g / ||v||) dW_eff - (g dot / ||v||^3) v (float64)"""
    v, g, dw, inv = v.to(F64), g.to(F64), dw.to(F64), inv.to(F64)
    dot = (v * dw).sum(1)
    a = g * inv
    b = g * dot * inv ** 3
    return dot * inv, a[:, None] * dw - b[:, None] * v


# ------------------------------------------------------------------ weight norm on real rows
# The exact rows above have a power-of-two norm and at most 2304 elements.  The real family: rows of 0.05 * randn with real gains and
# real dW, the present lengths plus 4608 and 18432 (2048 channels x 9 taps, the flow's longest row) at all four alignments; in every
# job one row with a norm near 1e-3, one near 1e3 and one nearly radial gradient dW = 3 v + 1e-3 * randn, where a dW - bcoef v cancels.
# References: wn_scale_ref / wn_bwd_ref in float64, the backward teacher-forced on the fp32 inv_norm it is handed.  Units: the fp32
# ulp of the result for scale and inv_norm (a sum of squares does not cancel); for dg the ulp of inv sum |dw||v|, for dv[k] the ulp of
# |g| inv |dw_k| + |g| inv^3 sum |dw||v| |v_k|.  Bound: max(4 x WN_YARDSTICK, 4); the yardstick is the worst error of the fp32
# restatement below, which follows the kernel's per-lane strides, over the GPU test's own operands (test_optim_exact_cpu.py).
WN_REAL_K = [1, 3, 6, 64, 160, 764, 768, 772, 1728, 2304, 4608, 18432]
WN_YARDSTICK = {"scale": 1.5, "inv_norm": 1.8, "dg": 2.4, "dv": 3.3}       # measured 1.48, 1.73, 2.37 and 3.24


def wn_bound(key):
    return max(4.0 * WN_YARDSTICK[key], 4.0)


def wn_real_case(seed):
    """48 jobs (every K of WN_REAL_K at v_off = 0, 1, 2, 3 mod 4), 5..8 rows each, laid out as the exact case is: gains and directions
    apart in the flat buffer with sentinel gaps, per-job output rows apart by two sentinel rows.  Returns (jobs, total_rows, nout,
    params, grads, vals) with vals = [(g, v, dW)] in float32."""
    gen = torch.Generator().manual_seed(seed)
    specs, vals, off, out = [], [], 16, 0
    for i, (K, mod) in enumerate((K, mod) for K in WN_REAL_K for mod in range(4)):
        rows = 5 + i % 4
        g_off = off
        v_off = g_off + rows + 3
        v_off += (mod - v_off) % 4
        specs.append((v_off, g_off, out, rows, K))
        v = 0.05 * torch.randn(rows, K, generator=gen)
        nrm = v.norm(dim=1, keepdim=True).clamp(min=1e-6)
        v[0] = v[0] / nrm[0] * 1.1e-3
        v[1] = v[1] / nrm[1] * 0.9e3
        dw = torch.randn(rows, K, generator=gen)
        dw[2] = 3 * v[2] + 1e-3 * torch.randn(K, generator=gen)
        vals.append((torch.randn(rows, generator=gen), v, dw))
        off = v_off + rows * K + 5
        out += rows + 2
    jobs, total_rows = wn_table(specs)
    n = off + 16
    params = torch.full((n,), SENT)
    grads = torch.full((n,), SENT)
    for j, (g, v, dw) in zip(jobs, vals):
        params[j.g_off:j.g_off + j.rows] = g
        params[j.v_off:j.v_off + j.rows * j.K] = v.reshape(-1)
        grads[j.v_off:j.v_off + j.rows * j.K] = dw.reshape(-1)
    return jobs, total_rows, out + 8, params, grads, vals


def wn_bwd_mags(v, g, dw, inv):
    """(unit of dg, unit of dv): the sums of the magnitudes of the terms each is made of (float64)"""
    v, g, dw, inv = v.to(F64), g.to(F64), dw.to(F64), inv.to(F64)
    sabs = (v * dw).abs().sum(1)
    return inv * sabs, (g.abs() * inv)[:, None] * dw.abs() + (g.abs() * inv ** 3 * sabs)[:, None] * v.abs()


def _lane_sum32(prod, vec):
    """fp32 sum of the products [rows, K] the way a wave takes it: lane l owns the elements (vec: the 4-groups) l, l + 64, ... and adds
    them in order; the 64 partial sums then meet in a butterfly"""
    rows, K = prod.shape
    w = 4 if vec else 1
    n = -(-K // (64 * w))
    p = torch.zeros(rows, n * 64 * w, dtype=torch.float32)
    p[:, :K] = prod
    p = p.view(rows, n, 64, w).permute(0, 2, 1, 3).reshape(rows, 64, n * w)
    s = torch.zeros(rows, 64, dtype=torch.float32)
    for i in range(n * w):
        s = s + p[:, :, i]
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
    return s[:, 0]


def wn_scale_restate(v, g, v_off):
    """fp32 restatement of wn_scale_kernel on float32 operands: (scale, inv_norm)"""
    vec = v.shape[1] % 4 == 0 and v_off % 4 == 0
    nrm = torch.sqrt(_lane_sum32(v * v, vec))
    return g / nrm, 1.0 / nrm


def wn_bwd_restate(v, g, dw, inv32, v_off):
    """fp32 restatement of wn_bwd_kernel on float32 operands and the fp32 inv_norm it is handed: (dg, dv)"""
    vec = v.shape[1] % 4 == 0 and v_off % 4 == 0
    dot = _lane_sum32(dw * v, vec)
    a, b = g * inv32, g * dot * inv32 * inv32 * inv32
    return dot * inv32, a[:, None] * dw - b[:, None] * v


def units(got, ref64, mag64):
    """worst |got - ref| in fp32 ulps of mag (float64 tensors; 0 for empty input)"""
    if ref64.numel() == 0:
        return 0.0
    u = torch.pow(2.0, torch.floor(torch.log2(mag64.abs().clamp(min=2.0 ** -126))) - 23)
    return float(((got.to(F64) - ref64).abs() / u).max())


def assert_exactly_representable(x, what):
    """every float64 value of x is a float32 value (the operand classes promise exact results; a failure here is a generator bug)"""
    bad = rn(x) != x
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values are not exact in fp32 (first {float(x[bad][0])})"


# ------------------------------------------------------------------ relayout reference
def tiled_offset(row, col, ld, esz):
    """prep.hip: tiled_offset<T> (esz = element size in bytes) on integer tensors"""
    KS, E16 = 64 // esz, 16 // esz
    rb, r = row // 16, row % 16
    ks = col // KS
    cq = col - ks * KS
    return (rb * (ld // KS) + ks) * (16 * KS) + (cq // E16) * (16 * E16) + r * E16 + cq % E16


def relayout_values(j, params, wn_scale):
    """W[n][k][t] (float64, n < n_real, k < k_real) as the kernel reads it: params[src_off + n s_n + k s_k + t], times scale[n] in fp32"""
    n = torch.arange(j.n_real, device=params.device).view(-1, 1, 1)
    k = torch.arange(j.k_real, device=params.device).view(1, -1, 1)
    t = torch.arange(j.taps, device=params.device).view(1, 1, -1)
    W = params.to(F64)[j.src_off + n * j.s_n + k * j.s_k + t]
    if j.scale_off >= 0:
        W = rn(W * wn_scale.to(F64)[j.scale_off:j.scale_off + j.n_real].view(-1, 1, 1))
    return W


def relayout_operands(j, params, wn_scale):
    """the whole A [A_rows_pad][taps * A_inner_pad] and B [B_rows_pad][taps * B_inner_pad] matrices of a job (float64; B None when
    dstB < 0), padding zeros included, in row-major (not yet fragment-tiled) order"""
    W = relayout_values(j, params, wn_scale)
    dev = params.device
    A = torch.zeros(j.A_rows_pad, j.taps, j.A_inner_pad, dtype=F64, device=dev)
    nA, kA = min(j.n_real, j.A_rows_pad), min(j.k_real, j.A_inner_pad)
    A[:nA, :, :kA] = W[:nA, :kA].permute(0, 2, 1)
    B = None
    if j.dstB >= 0:
        B = torch.zeros(j.B_rows_pad, j.taps, j.B_inner_pad, dtype=F64, device=dev)
        kB, nB = min(j.k_real, j.B_rows_pad, j.B_rows_real), min(j.n_real, j.B_inner_pad)
        B[:kB, :, :nB] = W[:nB, :kB].permute(1, 2, 0)
        B = B.reshape(j.B_rows_pad, -1)
    return A.reshape(j.A_rows_pad, -1), B


def place(dst, mat, base, frag_tiled, esz):
    """write the matrix mat [rows][ld] into the flat float64 buffer dst at element base (row-major, or fragment-tiled)"""
    rows, ld = mat.shape
    if not frag_tiled:
        dst[base:base + rows * ld] = mat.reshape(-1)
        return
    r = torch.arange(rows, device=dst.device).view(-1, 1).expand(rows, ld)
    c = torch.arange(ld, device=dst.device).view(1, -1).expand(rows, ld)
    dst[base + tiled_offset(r, c, ld, esz).reshape(-1)] = mat.reshape(-1)


def relayout_expect(jobs, params, wn_scale, dst, esz):
    """dst (float64 copy of the destination before the launch) with every job's A and B written"""
    for j in jobs:
        A, B = relayout_operands(j, params, wn_scale)
        place(dst, A, j.dstA, j.frag_tiled, esz)
        if B is not None:
            place(dst, B, j.dstB, j.frag_tiled, esz)
    return dst


# ------------------------------------------------------------------ comparison
def cast_like(x64, dtype):
    """the float64 expectation rounded as the kernel's output type (RNE to fp32, then RNE to bf16)"""
    x = x64.to(torch.float32)
    return x.to(torch.bfloat16) if dtype == torch.bfloat16 else x


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def assert_same(got, expect, what="", where=None):
    """bitwise equality of two tensors of one dtype (expect: same dtype, or float64 to be rounded to it); raises naming the first
    differing flat index -- through where(index) when given -- with both values and the number of differing elements"""
    if expect.dtype == F64 and got.dtype != F64:
        expect = cast_like(expect, got.dtype)
    got, expect = got.reshape(-1), expect.reshape(-1).to(got.device)
    assert got.dtype == expect.dtype and got.numel() == expect.numel(), (what, got.dtype, expect.dtype, got.numel(), expect.numel())
    bad = bits(got) != bits(expect)
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad)[0])
        loc = where(i) if where is not None else f"element {i}"
        raise AssertionError(f"{what}: {n} differing elements; first at {loc}: got {float(got[i])!r}, expected {float(expect[i])!r}")


def locate_relayout(jobs, esz, base=0):
    """where(index) for a relayout destination: the job, operand, row and column of a flat element (or 'outside every operand')"""
    regions = []
    for ji, j in enumerate(jobs):
        ldA = j.taps * j.A_inner_pad
        regions.append((j.dstA, j.A_rows_pad * ldA, ji, "A", ldA, j.A_inner_pad, j.frag_tiled))
        if j.dstB >= 0:
            ldB = j.taps * j.B_inner_pad
            regions.append((j.dstB, j.B_rows_pad * ldB, ji, "B", ldB, j.B_inner_pad, j.frag_tiled))

    def where(i):
        i -= base
        for off, size, ji, op, ld, inner, ft in regions:
            if off <= i < off + size:
                rel = i - off
                if ft:
                    return f"job {ji} operand {op} (fragment-tiled) element {rel}"
                row, col = divmod(rel, ld)
                return f"job {ji} operand {op} row {row} column {col} (tap {col // inner}, index {col % inner})"
        return f"element {i}: outside every operand (a sentinel)"
    return where


def locate_segments(segments):
    """where(index) for a flat buffer cut into named [off, off + len) pieces"""
    def where(i):
        for name, off, n in segments:
            if off <= i < off + n:
                return f"{name} element {i - off} (flat {i})"
        return f"flat element {i}: outside every range (a sentinel)"
    return where


def locate_rows(jobs, what="v"):
    """where(index) for a weight-norm parameter / gradient buffer: job, row, column"""
    def where(i):
        for ji, j in enumerate(jobs):
            if j.v_off <= i < j.v_off + j.rows * j.K:
                r, c = divmod(i - j.v_off, j.K)
                return f"job {ji} {what} row {r} (global row {j.row_start + r}) column {c}"
            if j.g_off <= i < j.g_off + j.rows:
                return f"job {ji} gain row {i - j.g_off} (global row {j.row_start + i - j.g_off})"
        return f"flat element {i}: outside every job (a sentinel)"
    return where


def sentinel(n, dtype=torch.float32, device="cpu"):
    return torch.full((n,), SENT, dtype=dtype, device=device)
