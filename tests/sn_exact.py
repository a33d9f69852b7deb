"""Kernel-by-kernel checking of the first stage's parameter path (csrc/vae_train.hip): the weight-operand writer, the spectral-norm power
iteration and its backward, the row-scale backward, the frame sum, the multi-tensor Adam and the KL term.  References, restatements,
operand generators and the case tables; the test functions are in test_sn_kernels_cpu.py (which pins the references and the input
conditions and measures the yardsticks) and test_sn_kernels_gpu.py (which runs the kernels through the C ABI).

* References: plain functions from the formulas of include/ipoke_hip.h and the kernel comments.  They compute in the dtype of their
  operands: with float64 operands they are the reference, with the same operands cast to float32 (``restate``, single-threaded CPU)
  they are the fp32 restatement, which never calls the library.  Operands are rounded to the kernel's input type first (``f32r``,
  ``as_seen``), so the reference sees exactly what the kernel reads.
* The error unit is the ulp of the output type; for a sum whose terms can cancel, the ulp of the sum of the terms' magnitudes (the
  ``mag`` each reference returns next to its value).
* The power iteration is checked phase by phase on the values the kernels STORED (workspace ``[4 reserved | tu | tv]``, u, v, out,
  snapshot), so that the conditioning of the iteration does not enter a bound: tv against W^T u, v against tv_stored / max(||tv_stored||,
  eps), tu against W v_stored, u against tu_stored / max(||tu_stored||, eps), sigma against u_stored . tu_stored, 1 / sigma against the
  correctly rounded fp32 quotient (bit for bit).
* ``ipoke_sum_frames`` promises fp32 accumulation and one rounding to the storage type.  On general fp32 operands four sequential
  additions may be 2 ulp away from the exact sum, in any order, so the 1-ulp bound is put to operands whose fp32 partial sums are exact:
  reals on the 2^-12 grid in [-8, 8] (16 significant bits, 19 for a sum of five), rounded to the storage type first.  In fp32 the sum
  is then exact, in bf16 it is rounded once.
* Guarded buffers as in disc_exact / flow_exact: every tensor a kernel receives is followed by SENT, pitches are wider than the rows.

The CPU test measures the restatement's worst error on the very operands the GPU test uses and fails when it exceeds the recorded
YARDSTICK; the GPU bound is ``gpu_bound`` = 4 x the recorded value and at least 4 units (ipoke_sum_frames: 1 ulp of the storage type).

  Recorded yardsticks (worst restatement error over the case tables below, rounded up) and the GPU bounds:

      output                  yardstick  GPU bound      output                  yardstick  GPU bound
      sn_tv                   3          12             rowscale_gs             2.2        8.8
      sn_v                    1.4        5.6            rowscale_dots           0.5        4
      sn_tu                   2          8              rowscale_dbias          0.5        4
      sn_u                    1          4              adam_p                  3.6        14.4
      sn_sigma                1          4              adam_m                  2.4        9.6
      sn_bwd                  1.5        6              adam_v                  3.8        15.2
      sn_bwd_frames           2.5        10             kl_value                0.5        4
      sum_frames              0.5        1 (fixed)      kl_dmu                  0.7        4
                                                        kl_dlv                  1.4        5.6

  Units that are not the output's own ulp: tv sum_r |W||u|, tu sum_c |W||v|, sigma sum |u||tu|; sn_bwd (|G| + sum|G W| |inv| |u||v|) |inv|;
  sn_bwd_frames |G| + sum_t |dots_t inv_t u_t v_t|; dots sum |g| (|pre| + |bias|), dbias sum |g|; Adam m |b1 m| + (1 - b1) gmag, v
  b2 v + (1 - b2) gmag^2 with gmag = |g grad_scale| + |wd p|, p |p| + |update| with m's unit in place of m; the KL value |loss_0| +
  0.5 / positions sum (1 + |lv| + mu^2 + e^lv), dlv (e^lv + 1) 0.5 / positions.  The sums' yardsticks are rounded up to the next half
  unit: the restatement's summation order is the host library's.
"""
import collections
import math

import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from tests.conv_exact import act64, act_grad_from_out64, round_up  # noqa: F401  (re-exported for the test files)
from tests.disc_exact import (DTYPES, F64, GUARD, SENT, assert_close_ulp, assert_same, check_guard, guarded, randint64,  # noqa: F401
                              ulp_of)
from tests.flow_exact import assert_units, err_units, f32r  # noqa: F401
from tests.optim_exact import cast_like  # noqa: F401

F32 = torch.float32
BF16 = torch.bfloat16
EPS = 1e-12                  # F.normalize's eps, as torch.nn.utils.spectral_norm passes it

# worst error of the fp32 restatement against float64, in the unit named in the docstring (test_sn_kernels_cpu.py asserts them)
YARDSTICK = {
    "sn_tv": 3.0, "sn_v": 1.4, "sn_tu": 2.0, "sn_u": 1.0, "sn_sigma": 1.0, "sn_bwd": 1.5, "sn_bwd_frames": 2.5, "sum_frames": 0.5,
    "rowscale_gs": 2.2, "rowscale_dots": 0.5, "rowscale_dbias": 0.5, "adam_p": 3.6, "adam_m": 2.4, "adam_v": 3.8,
    "kl_value": 0.5, "kl_dmu": 0.7, "kl_dlv": 1.4,
}


def gpu_bound(key):
    return max(4.0 * YARDSTICK[key], 4.0)


def restate(fn, *args, **kw):
    """fn on the same operands in float32 on one CPU thread: float64 tensors are cast, everything else passes"""
    cast = lambda a: a.to(F32) if torch.is_tensor(a) and a.dtype == F64 else a           # noqa: E731
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn(*[cast(a) for a in args], **{k: cast(v) for k, v in kw.items()})
    finally:
        torch.set_num_threads(n)


def as_seen(t, tdtype):
    """round a float64 tensor to the values a kernel reading `tdtype` sees"""
    return t.to(F32).to(tdtype).to(F64)


def scalar(x):
    """a C float argument as a 0-dim float64 tensor (restate casts it with the operands)"""
    return torch.tensor(float(torch.tensor(x, dtype=F32)), dtype=F64)


# ------------------------------------------------------------------ the weight as a matrix
SnCase = collections.namedtuple("SnCase", "cout cin taps transposed")
SN_CASES = [
    SnCase(3, 64, 49, 0),        # the RGB head: R below one wave group
    SnCase(40, 12, 9, 1),        # C = 108 is no multiple of 32, R no multiple of 4, ConvTranspose storage
    SnCase(260, 33, 9, 0),       # R > 256 and C = 297 > 256: every 256-stride loop takes a second trip
    SnCase(128, 32, 1, 0),
]
SN_EDGES = {"zero": SnCase(5, 7, 9, 0), "eps": SnCase(6, 10, 9, 1)}


def sn_id(c):
    return f"{c.cout}x{c.cin}x{c.taps}" + ("T" if c.transposed else "")


def storage_shape(c):
    return (c.cin, c.cout, c.taps) if c.transposed else (c.cout, c.cin, c.taps)


def to_matrix(w, c):
    """weight storage -> W [R = cout][C = cin * taps]: weight.reshape(cout, -1), or weight.transpose(0, 1).reshape(cout, -1)"""
    w = w.reshape(storage_shape(c))
    return (w.permute(1, 0, 2) if c.transposed else w).reshape(c.cout, c.cin * c.taps)


def from_matrix(W, c):
    """the inverse of to_matrix: [R][C] -> the storage layout (contiguous)"""
    W = W.reshape(c.cout, c.cin, c.taps)
    return (W.permute(1, 0, 2) if c.transposed else W).contiguous()


def sn_operands(c, seed=0, scale=0.1):
    """weight storage, u0 [R], v0 [C]: fp32 values as float64 (CPU)"""
    gen = torch.Generator().manual_seed(100 + seed)
    w = f32r(torch.randn(storage_shape(c), generator=gen, dtype=F64) * scale)
    u = f32r(F.normalize(torch.randn(c.cout, generator=gen, dtype=F64), dim=0))
    v = f32r(F.normalize(torch.randn(c.cin * c.taps, generator=gen, dtype=F64), dim=0))
    return w, u, v


def sn_edge_operands(name):
    """zero: an all-zero weight.  eps: a weight so small that ||W^T u|| < eps = 1e-12 (about 1e-13; every intermediate stays a normal
    fp32 number: tv ~ 1e-14, v = tv / eps ~ 0.03, tu ~ 1e-15, u = tu / eps ~ 1e-3, sigma ~ 1e-17)"""
    c = SN_EDGES[name]
    w, u, v = sn_operands(c, seed=50)
    if name == "zero":
        return torch.zeros_like(w), u, v
    tv = to_matrix(w, c).t() @ u
    return f32r(w * (1e-13 / float(tv.norm()))), u, v


# ------------------------------------------------------------------ the power iteration, phase by phase
def matvec_t_ref(W, u):
    """tv = W^T u and the sum of the terms' magnitudes"""
    return W.t() @ u, W.abs().t() @ u.abs()


def matvec_ref(W, v):
    """tu = W v and the sum of the terms' magnitudes"""
    return W @ v, W.abs() @ v.abs()


def normalize_ref(t, eps=EPS):
    """F.normalize(t, dim=0, eps): t / max(||t||_2, eps)"""
    return t / torch.clamp(torch.sqrt((t * t).sum()), min=eps)


def dot_ref(a, b):
    return (a * b).sum(), (a * b).abs().sum()


def power_iteration_ref(W, u, v, iterate=True, eps=EPS):
    """one call of ipoke_spectral_sigma in exact arithmetic: dict(tv, v, tu, u, sigma); torch.nn.utils.spectral_norm's
    v = normalize(W^T u), u = normalize(W v), sigma = u . W v"""
    tv = None
    if iterate:
        tv, _ = matvec_t_ref(W, u)
        v = normalize_ref(tv, eps)
    tu, _ = matvec_ref(W, v)
    if iterate:
        u = normalize_ref(tu, eps)
    return dict(tv=tv, v=v, tu=tu, u=u, sigma=dot_ref(u, tu)[0])


# ------------------------------------------------------------------ operand writer
WOP_CASES = [      # cout, cin, taps, transposed
    SnCase(5, 3, 49, 0), SnCase(40, 12, 9, 1), SnCase(16, 8, 27, 0), SnCase(64, 64, 1, 0),
    SnCase(256, 500, 9, 0),      # kc = 504 / 512: cout * taps * kc > 4096 * 256, the grid-stride loop wraps
]
WOP_MULTI_JOBS = 70              # two launches of the multi writer (64 jobs each)
WOP_MULTI_BIG = 5                # the job above 65 536 elements


def wop_ref(w, c, kc, s=None):
    """[cout][taps * kc]: out[o][t * kc + ci] = s * w(o, ci, t), columns cin .. kc - 1 of every tap zero"""
    W = to_matrix(w, c).reshape(c.cout, c.cin, c.taps).permute(0, 2, 1)
    if s is not None:
        W = (s * W).to(F32).to(W.dtype)                     # the fp32 product, which the cast to bf16 then rounds again
    out = torch.zeros(c.cout, c.taps, kc, dtype=W.dtype)
    out[:, :, : c.cin] = W
    return out.reshape(c.cout, c.taps * kc)


def wop_multi_cases():
    """70 jobs: the small shapes in turn, job WOP_MULTI_BIG with 128 x 9 x 128 = 147 456 elements"""
    small = [SnCase(5, 3, 49, 0), SnCase(40, 12, 9, 1), SnCase(16, 8, 27, 0), SnCase(64, 64, 1, 0), SnCase(3, 20, 9, 1), SnCase(1, 1, 1, 0)]
    cases = [small[i % len(small)] for i in range(WOP_MULTI_JOBS)]
    cases[WOP_MULTI_BIG] = SnCase(128, 120, 9, 1)
    return cases


# ------------------------------------------------------------------ spectral-norm backward
def sn_bwd_ref(G, W, u, v, inv):
    """(G - <G, W> inv u v^T) inv on matrices [R][C]; returns (value, mag)"""
    dot, dmag = (G * W).sum(), (G * W).abs().sum()
    uv = torch.outer(u, v)
    return (G - dot * inv * uv) * inv, (G.abs() + dmag * inv.abs() * uv.abs()) * inv.abs()


def sn_bwd_frames_ref(G, us, vs, invs, dots):
    """G - sum_t dots[t] inv_t u_t v_t^T; us [T][R], vs [T][C]; returns (value, mag)"""
    out, mag = G.clone(), G.abs()
    for t in range(us.shape[0]):
        term = dots[t] * invs[t] * torch.outer(us[t], vs[t])
        out = out - term
        mag = mag + term.abs()
    return out, mag


def sn_bwd_operands(c, frames, seed=0):
    """w, G (storage layout), snapshots us [T][R], vs [T][C], sig [T][2] = {sigma, fp32(1 / sigma)}, dots [T]: fp32 values as float64"""
    gen = torch.Generator().manual_seed(300 + seed)
    w, _, _ = sn_operands(c, seed)
    G = f32r(torch.randn(storage_shape(c), generator=gen, dtype=F64))
    us = f32r(F.normalize(torch.randn(frames, c.cout, generator=gen, dtype=F64), dim=1))
    vs = f32r(F.normalize(torch.randn(frames, c.cin * c.taps, generator=gen, dtype=F64), dim=1))
    sigma = f32r(0.5 + torch.rand(frames, generator=gen, dtype=F64) * 2.0)
    sig = torch.stack([sigma, f32r(1.0 / sigma)], 1)
    dots = f32r(torch.randn(frames, generator=gen, dtype=F64) * 3.0)
    return w, G, us, vs, sig, dots


SN_BWD_CASES = [SnCase(3, 64, 49, 0), SnCase(3, 64, 49, 1), SnCase(260, 33, 9, 0), SnCase(260, 33, 9, 1)]     # 37 / 256 partials
BwdFramesCase = collections.namedtuple("BwdFramesCase", "shape frames snap_extra sig_stride")
SN_BWD_FRAMES_CASES = [
    BwdFramesCase(SnCase(40, 12, 9, 0), 1, 5, 2), BwdFramesCase(SnCase(40, 12, 9, 1), 5, 3, 3),
    BwdFramesCase(SnCase(3, 64, 49, 1), 1, 1, 3), BwdFramesCase(SnCase(3, 64, 49, 0), 5, 7, 2),
    BwdFramesCase(SnCase(260, 226, 9, 0), 5, 5, 3),          # R * C = 260 x 2034 > 2048 * 256: the grid-stride loop wraps
]


# ------------------------------------------------------------------ row-scale backward
def pre_from_out_ref(act, y):
    """the pre-activation recovered from the saved output (ReLU's zeros and ELU's -1 cannot be recovered: their gradient is zero)"""
    if act == _lib.ACT_ELU:
        return torch.where(y > 0, y, torch.log1p(torch.clamp(y, min=-1.0)))
    if act == _lib.ACT_LRELU02:
        return torch.where(y > 0, y, 5.0 * y)
    return y


def rowscale_bwd_ref(dy, y, act, bias, scale, rows_per_group):
    """dy, y [M][C]; scale [groups].  gs = dy act'(y) scale[group], dots[group] = sum dy act'(y) (pre(y) - bias), dbias = column sums of
    dy act'(y).  Returns dict(gs, dots, dots_mag, dbias, dbias_mag)"""
    M, C = dy.shape
    groups = M // rows_per_group
    g = dy * act_grad_from_out64(act, y)
    b = torch.zeros(C, dtype=dy.dtype) if bias is None else bias
    pre = pre_from_out_ref(act, y)
    zero = torch.zeros((), dtype=dy.dtype)
    term = torch.where(g != 0, g * (pre - b), zero)                       # (0 x -inf at ELU's -1)
    tmag = torch.where(g != 0, g.abs() * (pre.abs() + b.abs()), zero)
    return dict(gs=(g.reshape(groups, rows_per_group, C) * scale.reshape(groups, 1, 1)).reshape(M, C),
                dots=term.reshape(groups, -1).sum(1), dots_mag=tmag.reshape(groups, -1).sum(1), dbias=g.sum(0), dbias_mag=g.abs().sum(0))


RsCase = collections.namedtuple("RsCase", "name groups rows C_f32 C_bf16 act bias dbias dts")
ACT_IDS = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "elu": _lib.ACT_ELU, "lrelu": _lib.ACT_LRELU02}
RS_CASES = [RsCase(a, 3, 700, 21, 20, ACT_IDS[a], True, True, ("f32", "bf16")) for a in ACT_IDS] + [
    RsCase("eight", 3, 46 * 512 + 5, 20, 20, _lib.ACT_ELU, True, True, ("f32", "bf16")),     # 141 partial rows: the eight-in-flight loop + tail
    RsCase("trip", 2, 300, 1028, 2056, _lib.ACT_LRELU02, True, True, ("f32", "bf16")),       # Cpad / E16 = 257: the second channel trip
    RsCase("nodbias", 3, 700, 21, 20, _lib.ACT_ELU, True, False, ("f32", "bf16")),
    RsCase("nobias", 3, 700, 21, 20, _lib.ACT_ELU, False, True, ("f32", "bf16")),
]
RS_SCALE_STRIDE = 2


def rs_operands(case, dt):
    """dict(C, dy, y [M][C], bias [C] or None, scale [groups]) as the kernel sees them (float64, CPU).  ELU outputs hold -1 and the
    value next to it, ReLU outputs exact zeros."""
    tdt = DTYPES[dt][1]
    C = case.C_bf16 if tdt == BF16 else case.C_f32
    M = case.groups * case.rows
    gen = torch.Generator().manual_seed(700 + len(case.name) + C)
    pre = torch.randn(M, C, generator=gen, dtype=F64) * 1.5
    y = as_seen(act64(case.act, pre), tdt)
    if case.act == _lib.ACT_ELU:
        nxt = -1.0 + (2.0 ** -8 if tdt == BF16 else 2.0 ** -24)             # the storage type's neighbour of -1
        for grp in range(case.groups):
            r = grp * case.rows
            y[r, 0], y[r + 1, 0], y[r + case.rows - 1, C - 1], y[r + 2, C - 1] = -1.0, nxt, -1.0, nxt
    dy = as_seen(torch.randn(M, C, generator=gen, dtype=F64), tdt)
    bias = f32r(torch.randn(C, generator=gen, dtype=F64) * 0.3) if case.bias else None
    scale = f32r(0.4 + torch.rand(case.groups, generator=gen, dtype=F64) * 2.0)
    return dict(C=C, M=M, dy=dy, y=y, bias=bias, scale=scale)


def rs_blocks(case, C):
    """(ngroups, nbx) as the library lays its partials out, from the host-only workspace query"""
    ws = int(_lib.lib().ipoke_rowscale_bwd_workspace_floats(case.groups * case.rows, C, case.rows))
    assert ws % (case.groups * (C + 1)) == 0
    return case.groups, ws // (case.groups * (C + 1))


# ------------------------------------------------------------------ frame sum
SUM_FRAMES = [1, 2, 5]
SUM_N = 1000                         # elements per frame of the small cases (a multiple of 8)
SUM_WRAP_VECS = 4096 * 256 + 3       # 16-byte vectors per frame of the wrap case


def sum_frames_ref(src):
    """src [frames][n] -> [n]"""
    return src.sum(0)


def sum_operands(frames, n, tdtype, integer, seed=0):
    gen = torch.Generator().manual_seed(900 + seed + frames)
    if integer:
        return randint64(-8, 8, (frames, n), gen)
    grid = torch.round(torch.randn(frames, n, generator=gen, dtype=F64) * 4096.0).clamp(-8 * 4096, 8 * 4096) / 4096.0
    return as_seen(grid, tdtype)


# ------------------------------------------------------------------ Adam
ADAM_HYPER = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=0.37)
ADAM_STEPS = [1, 2, 1000]
ADAM_SIZES = [1, 70000] + [3, 17, 64, 255, 256, 257, 1000, 5, 4097] * 6          # 56 entries, the first 49 are used
ADAM_COUNT = 49                                                                  # two launches: 48 + 1
ADAM_GAP = 8


def adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """torch.optim.Adam (amsgrad off, coupled weight decay) on gradient g * grad_scale; hyper-parameters 0-dim tensors of the operands'
    dtype.  The bias corrections are host scalars computed in double from the fp32 betas, as torch.optim.Adam computes them whatever the
    parameters' dtype.  Returns dict(p, m, v, p_mag, m_mag, v_mag); the update is linear in m, so p's unit takes m's magnitudes."""
    one = torch.ones_like(lr)
    bc1, bc2s = 1.0 - float(beta1) ** step, math.sqrt(1.0 - float(beta2) ** step)
    gr = g * grad_scale + weight_decay * p
    gmag = (g * grad_scale).abs() + (weight_decay * p).abs()
    m2 = beta1 * m + (one - beta1) * gr
    v2 = beta2 * v + (one - beta2) * gr * gr
    m_mag = (beta1 * m).abs() + (one - beta1) * gmag
    den = torch.sqrt(v2) / bc2s + eps
    return dict(p=p - (lr / bc1) * (m2 / den), m=m2, v=v2, p_mag=p.abs() + (lr / bc1) * (m_mag / den), m_mag=m_mag,
                v_mag=beta2 * v + (one - beta2) * gmag * gmag)


def adam_hyper():
    return {k: scalar(x) for k, x in ADAM_HYPER.items()}


def adam_sizes():
    return ADAM_SIZES[:ADAM_COUNT]


def adam_operands(seed=0):
    """p, g (three gradients, one per step) as flat float64 tensors over all tensors back to back (no gaps), fp32 values"""
    n = sum(adam_sizes())
    gen = torch.Generator().manual_seed(1100 + seed)
    p = f32r(torch.randn(n, generator=gen, dtype=F64) * 0.1)
    gs = [f32r(torch.randn(n, generator=gen, dtype=F64)) for _ in ADAM_STEPS]
    return p, gs


# ------------------------------------------------------------------ KL
KlCase = collections.namedtuple("KlCase", "name positions Z small")
KL_CASES = [
    KlCase("latent", 3 * 64, 32, False),
    KlCase("cancel", 3 * 64, 32, True),              # mu, lv ~ 1e-3: 1 + lv - mu^2 - e^lv cancels to ~ -lv^2 / 2 - mu^2
    KlCase("one-wg", 1 << 15, 32, False),            # n = 2^20 exactly: still one workgroup
    KlCase("atomic", (1 << 15) + 128, 32, False),    # n = 2^20 + 4096: the multi-workgroup branch
]
KL_LOSS0 = 0.75


def kl_ref(mu, lv, positions, loss0):
    """loss0 - 0.5 / positions sum (1 + lv - mu^2 - e^lv) and its gradient.  Returns dict(loss, loss_mag, dmu, dlv, dlv_mag)"""
    inv = torch.ones((), dtype=mu.dtype) / positions
    e = torch.exp(lv)
    half = 0.5 * inv
    return dict(loss=loss0 - half * (1 + lv - mu * mu - e).sum(), loss_mag=loss0.abs() + half * (1 + lv.abs() + mu * mu + e).sum(),
                dmu=mu * inv, dlv=0.5 * (e - 1) * inv, dlv_mag=(e + 1) * half)


def kl_operands(case):
    gen = torch.Generator().manual_seed(1300 + case.positions)
    n = case.positions * case.Z
    s = 1e-3 if case.small else 1.0
    return f32r(torch.randn(n, generator=gen, dtype=F64) * s), f32r(torch.randn(n, generator=gen, dtype=F64) * 0.7 * s)
