"""Kernel-by-kernel checking of the flow's state kernels: the flow part of csrc/elementwise.hip (layout changes, ActNorm, the affine
coupling transform, log-det bookkeeping, the loss) and csrc/lu.hip (the LU-parametrised 1x1 convolution).  References, table mirrors,
operand generators and the case tables; the test functions are in test_flow_kernels_cpu.py (which pins the references and the input
conditions) and test_flow_kernels_gpu.py (which runs the kernels).

* References: plain functions straight from the formulas of include/ipoke_hip.h and the kernel comments.  They compute in the dtype of
  their operands: with float64 operands they are the reference, with the same operands cast to float32 (``restate``) they are the
  "fp32 restatement" -- the same formula in torch float32 on the CPU (two-pass statistics in the init), which never calls the library.
* Exact operands: integer states and gradients, ``log_scale = 0`` (expf(0) = 1 and 1 + 1e-8f rounds to 1), ``s = 0`` in raw
  (tanhf(0) + 1 = 1, logf(1) = 0: the coupling is an exact shift with log-det 0 and ds = (g x + dld) / 2), split-K partials that are
  integers, LU factors with entries in {-1, 0, 1}, sign_s = +-1 and log_s = 0 (all four matrices are integer).  Every partial sum stays
  below 2^24 (2^8 where it is stored as bf16), so everything but the transcendental functions and true divisions is bit-exact
  whatever the summation order.  The permutations are neither the identity nor involutions.
* Inexact operands: random real log_scale, s, log_s, L / U.  The error unit is the ulp of the output type -- for outputs that are sums
  of terms that can cancel, the ulp of the sum of the terms' magnitudes (the ``mag`` each reference returns next to the value).  The
  CPU test measures the restatement's worst error in that unit on the very operands the GPU test uses and fails when it exceeds the
  recorded YARDSTICK; the GPU bound is ``gpu_bound`` = 4 x the recorded value and at least 4 units (the margin for the device's expf /
  tanhf / logf / sqrtf and fused multiply-adds differing from the host's by a unit or two each).  Every element is compared.

  Recorded yardsticks (worst restatement error over the cases of the tables below, rounded up) and the GPU bounds:

      output                       yardstick  GPU bound      output                       yardstick  GPU bound
      actnorm_fwd                  1.6        6.4            affine_bwd.dx                0.5        4
      actnorm_inv                  2.4        9.6            affine_bwd.dparams (f32)     1.8        7.2
      actnorm_inv ext (bf16)       0.5        4              affine_bwd.dparams (bf16)    0.5        4
      actnorm_bwd.dx               1.3        5.2            affine_bwd.dbias             1.0        4
      actnorm_bwd.part             1.5        6              flow_nll scalars             1.0        4
      actnorm_init                 3.0        12             flow_nll d_out / dld         1.0        4
      affine_fwd                   1.5        6              lu wl / wu                   0.5        4
      affine_inv                   2.1        8.4            lu W                         1.4        5.6
      affine scale_out             1.0        4              lu W^-1                      2.2        8.8
      affine ext (bf16)            0.5        4              log-det slot                 1.0        4

  Units that are not the output's own ulp: ActNorm / affine forward |scale x| + |shift| with the scale's own terms (|tanh| + 1) |x|;
  the inverses (|y| + |shift|) / scale, for the coupling times (|tanh| + 1) / scale; part and dbias the sums of their terms' magnitudes;
  ds (|g x| + |dld / scale|) (1 + tanh^2) / 2; the init and the LU inverse as derived at actnorm_init_mags and lu_prepare_ref.  The real
  split-K partials are multiples of 2^-10, so raw is exact in any order there too.  cond_prepare's inexact activations take the bounds
  test_add_act has for the same device function (2 ulp in fp32, 1 in bf16).
"""
import collections
import ctypes

import torch

from ipoke_amd import _lib
from tests.conv_exact import act64, round_up  # noqa: F401  (re-exported for the test files)
from tests.disc_exact import (DTYPES, F64, GUARD, SENT, assert_close_ulp, assert_same, check_guard, guarded, randint64,  # noqa: F401
                              ulp_of)

F32 = torch.float32

# worst error of the fp32 restatement against float64, in the unit named in the docstring (test_flow_kernels_cpu.py asserts them)
YARDSTICK = {
    "actnorm_fwd": 1.6, "actnorm_inv": 2.4, "actnorm_inv_ext_bf16": 0.5, "actnorm_bwd_dx": 1.3, "actnorm_bwd_part": 1.5, "actnorm_init": 3.0,
    "affine_fwd": 1.5, "affine_inv": 2.1, "affine_scale": 1.0, "affine_ext_bf16": 0.5, "affine_bwd_dx": 0.5, "affine_bwd_dparams": 1.8,
    "affine_bwd_dparams_bf16": 0.5, "affine_bwd_dbias": 1.0, "logdet_slot": 1.0, "nll_scalars": 1.0, "nll_dout": 1.0,
    "lu_W": 1.4, "lu_Winv": 2.2, "lu_wl_wu": 0.5,
}


def gpu_bound(key):
    return max(4.0 * YARDSTICK[key], 4.0)


def err_units(got, ref64, mag64, tdtype=F32):
    """worst |got - ref| in ulps (of tdtype) of mag (the output itself, or the sum of the magnitudes of the terms it is a sum of)"""
    if ref64.numel() == 0:
        return 0.0
    return float(((got.to(F64).cpu() - ref64.cpu()).abs() / ulp_of(mag64.cpu(), tdtype)).max())


def assert_units(got, ref64, mag64, bound, tdtype, what):
    """every element within `bound` units; names the first that misses"""
    g, r = got.to(F64).cpu(), ref64.cpu()
    e = (g - r).abs() / ulp_of(mag64.cpu(), tdtype)
    bad = ~(e <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements beyond {bound} units (worst {float(e.max()):.2f}); first at element {i}: "
                             f"got {float(g.reshape(-1)[i])!r}, reference {float(r.reshape(-1)[i])!r}")


def restate(fn, *args, **kw):
    """fn on the same operands in float32 (CPU): float64 tensors are cast, everything else passes"""
    cast = lambda a: a.to(F32) if torch.is_tensor(a) and a.dtype == F64 else a           # noqa: E731
    return fn(*[cast(a) for a in args], **{k: cast(v) for k, v in kw.items()})


def f32r(t):
    """round a float64 tensor to float32 values (the operands as the kernel sees them)"""
    return t.to(F32).to(F64)


# ------------------------------------------------------------------ table mirrors
class LuJob(ctypes.Structure):
    """LuJob of csrc/lu.hip (ipoke_lu_job_size)"""
    _fields_ = [(n, ctypes.c_int64) for n in ("p_l", "p_u", "p_logs", "b_perm", "b_sign", "b_lmask", "b_umask", "b_eye", "w_off")] + [
        ("C", ctypes.c_int32), ("pad", ctypes.c_int32)]


class LsRef(ctypes.Structure):
    """one entry of ipoke_actnorm_logdet's reference table (ipoke_actnorm_logdet_ref_size)"""
    _fields_ = [("off", ctypes.c_int64), ("C", ctypes.c_int32), ("pad", ctypes.c_int32)]


def table_to_device(entries, device):
    """a list of ctypes structures as a byte tensor on the device"""
    arr = (type(entries[0]) * len(entries))(*entries)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


# ------------------------------------------------------------------ permutations
def perm(C, seed):
    """a permutation of C channels that is neither the identity nor an involution (C >= 3; C = 1, 2 have none: the identity)"""
    if C < 3:
        return torch.arange(C)
    gen = torch.Generator().manual_seed(seed)
    while True:
        p = torch.randperm(C, generator=gen)
        if not torch.equal(p, torch.arange(C)) and not torch.equal(p[p], torch.arange(C)):
            return p


# ------------------------------------------------------------------ layout
def nchw_to_state_ref(x, ld=None):
    """x [B][C][P] -> state [B*P][C]"""
    B, C, P = x.shape
    return x.permute(0, 2, 1).reshape(B * P, C)


def state_to_nchw_ref(s, B, C, P):
    """state [B*P][>= C] -> [B][C][P]"""
    return s[:, :C].reshape(B, P, C).permute(0, 2, 1)


def extract_cols_ref(s, off, stride, C):
    return s[:, off: off + (C - 1) * stride + 1: stride]


def cond_prepare_ref(h, act):
    """h [B][Cc][P] -> act(h) as [B*P][Cc]"""
    return nchw_to_state_ref(act64(act, h))


# ------------------------------------------------------------------ ActNorm (+ Shuffle)
def actnorm_fwd_ref(x, c0, C, ls=None, bias=None, idx=None):
    """out[:, c0 + j] = x[:, c0 + idx[j]] * exp(ls[idx[j]]) + bias[idx[j]]; other columns copied.  Returns (out, mag of the window)"""
    src = torch.arange(C) if idx is None else idx.long()
    v = x[:, c0 + src]
    mag = v.abs()
    if ls is not None:
        e = torch.exp(ls[src])
        mag = (v * e).abs() + bias[src].abs()
        v = v * e + bias[src]
    out = x.clone()
    out[:, c0: c0 + C] = v
    return out, mag


def actnorm_inv_ref(y, c0, C, ls=None, bias=None, inv_idx=None):
    """x'[c] = y[inv_idx[c]], then x = (x' - bias) / (exp(ls) + 1e-8); other columns copied.  Returns (out, mag of the window)"""
    src = torch.arange(C) if inv_idx is None else inv_idx.long()
    v = y[:, c0 + src]
    mag = v.abs()
    if ls is not None:
        d = torch.exp(ls) + 1e-8
        mag = (v.abs() + bias.abs()) / d
        v = (v - bias) / d
    out = y.clone()
    out[:, c0: c0 + C] = v
    return out, mag


def actnorm_bwd_ref(dy, x, c0, C, ls, idx, dld, B, P):
    """dx[:, c0 + idx[j]] = dy[:, c0 + j] exp(ls[idx[j]]);  part[b] = [dls | dbias] with
    dls[idx[j]] = sum_m dy[m][c0 + j] x[m][c0 + idx[j]] exp(ls[idx[j]]) + P dld[b],  dbias[idx[j]] = sum_m dy[m][c0 + j].
    Returns (dx, part or None, mag of part or None)"""
    src = torch.arange(C) if idx is None else idx.long()
    g = dy[:, c0: c0 + C]
    e = torch.exp(ls[src]) if ls is not None else torch.ones(C, dtype=dy.dtype)
    dx = dy.clone()
    dx[:, c0 + src] = g * e
    if ls is None:
        return dx, None, None
    t = (g * x[:, c0 + src] * e).reshape(B, P, C)
    part = torch.zeros(B, 2 * C, dtype=dy.dtype)
    mag = torch.zeros(B, 2 * C, dtype=dy.dtype)
    pd = float(P) * dld.reshape(B, 1)
    part[:, src] = t.sum(1) + pd
    mag[:, src] = t.abs().sum(1) + pd.abs()
    part[:, C + src] = g.reshape(B, P, C).sum(1)
    mag[:, C + src] = g.abs().reshape(B, P, C).sum(1)
    return dx, part, mag


def actnorm_init_ref(x, c0, C, ls0, b0):
    """statistics of y0 = x exp(ls0) + b0 over all rows (mean first, then the unbiased variance of the centred values);
    ls = log(1 / (std + 1e-6)), bias = -mean / (std + 1e-6)"""
    y = x[:, c0: c0 + C] * torch.exp(ls0) + b0
    mean = y.mean(0)
    d = y - mean
    std = torch.sqrt((d * d).sum(0) / (y.shape[0] - 1))
    inv = 1.0 / (std + 1e-6)
    return torch.log(inv), -mean * inv


def actnorm_init_mags(x, c0, C, ls0, b0):
    """the error units of the init as magnitudes (unit = fp32 ulp of the magnitude).  The centred value y0 - mean is a difference of
    terms of magnitude max|y0|, so it carries an absolute error of ulp(max|y0|) whatever the arithmetic; relative to the spread that is
    rel = ulp(max|y0|) / std.  log_scale = -log(std + 1e-6) inherits rel as an absolute error, bias = -mean inv inherits |bias| rel plus
    the mean's own ulp(max|y0|) inv.  Each unit is at least the output's own ulp."""
    y = x[:, c0: c0 + C] * torch.exp(ls0) + b0
    ls, b = actnorm_init_ref(x, c0, C, ls0, b0)
    d = y - y.mean(0)
    std = torch.sqrt((d * d).sum(0) / (y.shape[0] - 1))
    uy = ulp_of(y.abs().amax(0), F32)
    rel = uy / (std + 1e-6)
    two23 = 2.0 ** 23
    return torch.maximum(ls.abs(), rel * two23), torch.maximum(b.abs(), (b.abs() * rel + uy / (std + 1e-6)) * two23)


# ------------------------------------------------------------------ affine coupling transform
def raw_sum(parts, bias=None):
    """parts [nsplit][M][2Cp] (+ bias [2Cp]) -> raw [M][2Cp]"""
    r = parts.sum(0)
    return r if bias is None else r + bias


def affine_params_ref(raw):
    Cp = raw.shape[1] // 2
    return raw[:, :Cp], torch.tanh(0.5 * raw[:, Cp:]) + 1.0


def tcols(Cp, t_off, t_stride):
    return t_off + torch.arange(Cp) * t_stride


def affine_fwd_ref(x, raw, t_off, t_stride, B, Q):
    """y = scale x + mu on the transformed columns.  Returns (out, scale [M][Cp], log-det slots [B][Q], mag of the transformed columns,
    mag of the slots)"""
    mu, sc = affine_params_ref(raw)
    Cp = mu.shape[1]
    cols = tcols(Cp, t_off, t_stride)
    out = x.clone()
    out[:, cols] = sc * x[:, cols] + mu
    lg = torch.log(sc).reshape(B, Q, -1)
    # scale = tanh(s/2) + 1 is itself a sum that cancels for s << 0: its terms' magnitudes are |tanh| and 1
    t = torch.tanh(0.5 * raw[:, Cp:])
    return out, sc, lg.sum(-1), (t.abs() + 1.0) * x[:, cols].abs() + mu.abs(), lg.abs().sum(-1)


def affine_inv_ref(y, raw, t_off, t_stride):
    """x = (y - mu) / (scale + 1e-12).  Returns (out, mag of the transformed columns)"""
    mu, sc = affine_params_ref(raw)
    cols = tcols(mu.shape[1], t_off, t_stride)
    out = y.clone()
    out[:, cols] = (y[:, cols] - mu) / (sc + 1e-12)
    # the difference's terms over the scale, times the scale's own relative error unit (|tanh| + 1) / scale >= 1
    t = torch.tanh(0.5 * raw[:, mu.shape[1]:])
    return out, (y[:, cols].abs() + mu.abs()) * (t.abs() + 1.0) / ((sc + 1e-12) * (sc + 1e-12))


def affine_bwd_ref(dy, x, scale, dld, t_off, t_stride, B, P):
    """dx = dy scale on the transformed columns (others copied); dparams = [dmu | ds] with dmu = dy and
    ds = (dy x + dld[b] / scale) / 2 (1 - tanh(s/2)^2), tanh(s/2) = scale - 1; dbias_part[b] = the column sums of dparams over sample b.
    Returns dict(dx, dparams, dbias, mag_dparams, mag_dbias)"""
    Cp = scale.shape[1]
    cols = tcols(Cp, t_off, t_stride)
    g, xv = dy[:, cols], x[:, cols]
    gl = dld.reshape(B, 1, 1).expand(B, P, Cp).reshape(B * P, Cp)
    t = scale - 1.0
    ds = (g * xv + gl / scale) * 0.5 * (1.0 - t * t)
    mag_ds = ((g * xv).abs() + (gl / scale).abs()) * 0.5 * (1.0 + t * t)
    dx = dy.clone()
    dx[:, cols] = g * scale
    dp = torch.cat([g, ds], 1)
    mag = torch.cat([g.abs(), mag_ds], 1)
    return dict(dx=dx, dparams=dp, dbias=dp.reshape(B, P, 2 * Cp).sum(1), mag_dparams=mag, mag_dbias=mag.reshape(B, P, 2 * Cp).sum(1))


# ------------------------------------------------------------------ log-det bookkeeping and the loss
def logdet_finalize_ref(slots, const_term, const_dev=None):
    """slots [nslots][B][slot_w] -> logdet [B]"""
    return slots.sum((0, 2)) + const_term + (0.0 if const_dev is None else const_dev)


def actnorm_logdet_ref(params, refs, P):
    """refs: [(off, C)] -> P * sum over the layers of sum_c params[off + c]"""
    return float(P) * sum(float(params[o: o + c].sum()) for o, c in refs)


def flow_nll_ref(z, logdet, w, B):
    """z [B*P][C] (the real columns), logdet [B] -> (scalars [loss, nll, nlogdet], d_out = z / B, dld = -w / B [B]).
    The kernel multiplies by 1 / B; so does this (in float64 the two agree to 1e-16)."""
    invB = 1.0 / torch.tensor(float(B), dtype=z.dtype)
    nll = 0.5 * (z * z).sum() * invB
    nld = -logdet.sum() * invB
    return torch.stack([nll + w * nld, nll, nld]), z * invB, torch.full((B,), -w, dtype=z.dtype) * invB


# ------------------------------------------------------------------ LU 1x1 convolution
def unit_lower_inverse(A):
    """forward substitution, row by row (exact on integer matrices)"""
    C = A.shape[0]
    X = torch.zeros_like(A)
    eye = torch.eye(C, dtype=A.dtype)
    for i in range(C):
        X[i] = eye[i] - A[i, :i] @ X[:i]
    return X


def upper_inverse(Bm):
    """backward substitution, row by row"""
    C = Bm.shape[0]
    X = torch.zeros_like(Bm)
    eye = torch.eye(C, dtype=Bm.dtype)
    for i in range(C - 1, -1, -1):
        X[i] = (eye[i] - Bm[i, i + 1:] @ X[i + 1:]) / Bm[i, i]
    return X


def lu_prepare_ref(m):
    """m: dict(l, u, log_s, perm, sign, lmask, umask, eye) -> dict(wl, wu, W, Winv) and the magnitudes of the products"""
    wl = m["l"] * m["lmask"] + m["eye"]
    wu = m["u"] * m["umask"] + torch.diag(m["sign"] * torch.exp(m["log_s"]))
    Pm = m["perm"]
    wli, wui = unit_lower_inverse(wl), upper_inverse(wu)
    # a triangular inverse X = T^-1 by substitution has the componentwise forward error u |X| |T| |X| (Higham, Accuracy and Stability,
    # ch. 8); the product of the two inverses inherits it through both factors
    mli, mui = wli.abs() @ wl.abs() @ wli.abs(), wui.abs() @ wu.abs() @ wui.abs()
    return dict(wl=wl, wu=wu, W=Pm @ (wl @ wu), Winv=(wui @ wli) @ Pm.t(),
                mag_W=Pm @ (wl.abs() @ wu.abs()), mag_Winv=(mui @ wli.abs() + wui.abs() @ mli) @ Pm.t(), wli=wli, wui=wui)


def lu_apply_ref(x, C, mat, transposed):
    """out[m][i] = sum_j mat[i][j] x[m][j]  (transposed: mat[j][i]) on the first C columns; the rest copied"""
    out = x.clone()
    out[:, :C] = x[:, :C] @ (mat if transposed else mat.t())
    return out


def lu_wgrad_ref(dy, x, m, wl, wu, dld, P8):
    """dW = dy^T x, Q = P^T dW;  dl = (Q wu^T) lmask,  du = (wl^T Q) umask,  dlog_s = diag(wl^T Q) sign exp(log_s) + P8 sum_b dld[b]"""
    Q = m["perm"].t() @ (dy.t() @ x)
    su = wl.t() @ Q
    return (Q @ wu.t()) * m["lmask"], su * m["umask"], torch.diagonal(su) * m["sign"] * torch.exp(m["log_s"]) + float(P8) * dld.sum()


# ------------------------------------------------------------------ operand generators
def int_state(M, ld, seed, lim=8):
    return randint64(-lim, lim, (M, ld), torch.Generator().manual_seed(seed))


def real_state(M, ld, seed, scale=2.0):
    return f32r(torch.randn((M, ld), generator=torch.Generator().manual_seed(seed), dtype=F64) * scale)


def pow2_multiples(n, k, lim, gen):
    """n non-zero multiples of 2^-k in [-lim, lim] (a zero log-det gradient would hide a dropped P dld[b] term)"""
    v = randint64(-lim * 2 ** k, lim * 2 ** k, (n,), gen)
    return torch.where(v == 0, torch.ones_like(v), v) / 2.0 ** k


ActCase = collections.namedtuple("ActCase", "C c0 ld")
ACTNORM_CASES = [ActCase(1, 0, 4), ActCase(5, 3, 12), ActCase(60, 0, 64), ActCase(64, 8, 80)]
ACTNORM_M = 70                                        # 70 x 80 elements: 22 blocks of 256, the last one ragged
# ipoke_actnorm_inv_ext refuses an ext padding wider than the state (ext_ld - e_C <= ld).  In bf16 the padded pitch of the one-channel
# operand is 8 (and 9): 7 (8) padding columns, which the 4-column state of ActCase(1, 0, 4) cannot carry.  Those four combinations (two
# variants x two pitches) run on the same layer in an 8-column state instead.
ACTNORM_EXT_BF16_C1 = ActCase(1, 0, 8)


def actnorm_params(C, exact, seed):
    """(log_scale, bias, idx, inv_idx): exact -> log_scale = 0 and an integer bias"""
    gen = torch.Generator().manual_seed(100 + seed)
    if exact:
        ls, b = torch.zeros(C, dtype=F64), randint64(-4, 4, (C,), gen)
    else:
        ls, b = f32r(0.3 * torch.randn(C, generator=gen, dtype=F64)), f32r(torch.randn(C, generator=gen, dtype=F64))
    p = perm(C, seed)
    return ls, b, p, torch.argsort(p)


def ext_variants(c):
    """(e_off, e_stride, e_C) of ipoke_actnorm_inv_ext for an ActNorm case: a leading block, and every other column from 1"""
    half = max(c.C // 2, 1)
    return [(0, 1, half), (1, 2, max(1, min(half, (c.ld - 2) // 2 + 1)))]


# ipoke_actnorm_bwd: one block of 1024 threads per sample, rows_par = 1024 // C rows in flight
BwdCase = collections.namedtuple("BwdCase", "name C c0 ld P B idx params")
ACTNORM_BWD_CASES = [
    BwdCase("c1", 1, 0, 4, 64, 1, False, True),                 # rows_par = 1024 > P
    BwdCase("c3-idle", 3, 2, 8, 20, 3, True, True),             # 1024 % 3 != 0: thread 1023 idles; rows_par = 341 > P = 20
    BwdCase("c60", 60, 0, 64, 64, 3, True, True),               # rows_par = 17 does not divide 64; threads 1020 .. 1023 idle
    BwdCase("c64-p20", 64, 8, 80, 20, 1, True, True),           # rows_par = 16 does not divide 20
    BwdCase("c256", 256, 0, 256, 64, 3, True, True),            # the stated maximum: rows_par = 4
    BwdCase("c256-p20", 256, 4, 264, 20, 1, False, True),
    BwdCase("no-params", 5, 3, 12, 64, 2, True, False),         # log_scale == NULL: the early return, x / dld / part NULL
]


def actnorm_bwd_operands(c, exact, seed=0):
    gen = torch.Generator().manual_seed(200 + seed)
    M = c.B * c.P
    if exact:
        dy, x = randint64(-4, 4, (M, c.ld), gen), randint64(-8, 8, (M, c.ld), gen)
        dld = pow2_multiples(c.B, 3, 2, gen)
    else:
        dy, x = (f32r(torch.randn((M, c.ld), generator=gen, dtype=F64)) for _ in range(2))
        dld = f32r(torch.randn(c.B, generator=gen, dtype=F64))
    ls, _, p, _ = actnorm_params(c.C, exact, seed)
    return dict(dy=dy, x=x, dld=dld, ls=ls if c.params else None, idx=p if c.idx else None)


INIT_MS = [2, 64, 200, 320]                           # the minimum; fewer rows than one block of 256; not a multiple of 256
INIT_CASE = ActCase(5, 3, 12)


def actnorm_init_operands(M, preinit, seed=0):
    """x [M][ld] with SENT outside the window; channel 0 of the window has its mean far from zero (1000 +- small integers), channel 1 a
    small spread (integers times 2^-10: std about 2e-3, where the init's + 1e-6 moves log_scale by 5e-4)"""
    c = INIT_CASE
    gen = torch.Generator().manual_seed(300 + M + seed)
    x = torch.full((M, c.ld), SENT, dtype=F64)
    w = randint64(-3, 3, (M, c.C), gen)
    w[0, :] = 3.0
    w[1, :] = -2.0                                    # no channel is constant, whatever M
    w[:, 0] += 1000.0
    w[:, 1] /= 1024.0
    x[:, c.c0: c.c0 + c.C] = w
    if preinit:
        ls0, b0 = f32r(0.1 * torch.randn(c.C, generator=gen, dtype=F64)), f32r(torch.randn(c.C, generator=gen, dtype=F64))
    else:
        ls0, b0 = torch.zeros(c.C, dtype=F64), torch.zeros(c.C, dtype=F64)
    return x, ls0, b0


# ipoke_affine_fwd_ext launches Q = 4 slices per sample when (slot_stride >= 4 or no slot) and P % 4 == 0, else Q = 1;
# ipoke_affine_inv_ext Q = 4 when P % 4 == 0.  A block of 256 threads prefetches kAffPre = 2 elements per thread: rows * Cp > 512 enters
# the direct loads.  slot: 4 / 1 = slot_stride, None = logdet_slot NULL.
AffCase = collections.namedtuple("AffCase", "name Cp t_off t_stride nsplit raw_pad bias slot P B scale_out ext ext_pad")
AFFINE_CASES = [
    AffCase("cp1", 1, 0, 1, 1, 0, False, 4, 64, 1, True, None, 0),                   # ldraw == 2 Cp, one split
    AffCase("cp4-upper", 4, 4, 1, 4, 5, True, 4, 64, 3, True, "f32", 4),
    AffCase("cp30-even-q1", 30, 0, 2, 32, 4, True, 1, 64, 2, False, "bf16", 10),     # Q = 1: 64 x 30 = 1920 > 512, direct loads
    AffCase("cp32-odd-q1", 32, 1, 2, 35, 8, True, 1, 64, 2, True, "bf16", 8),        # Q = 1, Cp = 32: direct loads; nsplit > 32
    AffCase("cp32-noslot", 32, 32, 1, 1, 0, False, None, 64, 1, True, "f32", 1),     # no slot: Q = 4, 16 x 32 = 512 all prefetched
    AffCase("cp4-p50", 4, 0, 1, 4, 2, False, 4, 50, 2, True, None, 0),               # P % 4 != 0: Q = 1
    AffCase("cp30-35", 30, 30, 1, 35, 4, False, 4, 64, 5, False, "f32", 2),          # nsplit > 32 without bias
    AffCase("cp30-p50", 30, 0, 2, 4, 4, True, 4, 50, 2, True, "bf16", 2),            # the inverse's Q = 1: 50 x 30 > 512
]


def aff_ld(c):
    return 2 * c.Cp + 3                               # covers every (t_off, t_stride) of the table; odd


def aff_q(c, inverse=False):
    if inverse:
        return 4 if c.P % 4 == 0 else 1
    return 4 if (c.slot is None or c.slot >= 4) and c.P % 4 == 0 else 1


def affine_operands(c, exact, seed=0):
    """dict(x [M][ld], parts [nsplit][M][2Cp], bias [2Cp] or None).  exact: integer mu partials; the s partials are integers that sum to
    zero -- through the bias where there is one, else in cancelling pairs (zeros for a single split)"""
    gen = torch.Generator().manual_seed(400 + seed)
    M, Cp, n = c.B * c.P, c.Cp, c.nsplit
    if exact:
        x = randint64(-8, 8, (M, aff_ld(c)), gen)
        parts = randint64(-2, 2, (n, M, 2 * Cp), gen)
        bias = None
        if c.bias:
            bias = torch.cat([randint64(-2, 2, (Cp,), gen), torch.zeros(Cp, dtype=F64)])
        s = parts[:, :, Cp:]
        for u in range(0, n - 1, 2):
            s[u + 1] = -s[u]
        if n % 2:
            s[n - 1] = 0.0
    else:
        x = f32r(torch.randn((M, aff_ld(c)), generator=gen, dtype=F64) * 2)
        # multiples of 2^-10 below 2^3: mu and s are real-valued, yet the sum of the partials (+ bias) is exact in any order, so that
        # the comparison measures the transform and not the order of the split-K sum (which the exact set pins)
        parts = (torch.randn((n, M, 2 * Cp), generator=gen, dtype=F64) * (1.5 / n ** 0.5) * 1024).round().clamp(-8191, 8191) / 1024
        bias = (torch.randn(2 * Cp, generator=gen, dtype=F64) * 0.3 * 1024).round() / 1024 if c.bias else None
    return dict(x=x, parts=parts, bias=bias)


# ipoke_affine_bwd: one block of 1024 threads per sample, rows_par = 1024 // Cp
AffBwdCase = collections.namedtuple("AffBwdCase", "name Cp t_off t_stride P B ldp_pad dbias")
AFFINE_BWD_CASES = [
    AffBwdCase("cp1", 1, 0, 1, 64, 1, 0, True),                 # rows_par = 1024 > P
    AffBwdCase("cp32-odd", 32, 1, 2, 64, 3, 8, True),
    AffBwdCase("cp4-p20", 4, 4, 1, 20, 2, 0, False),            # rows_par = 256 > P = 20; dbias_part NULL
    AffBwdCase("cp48", 48, 0, 1, 64, 2, 16, True),              # 1024 % 48 != 0: rows_par = 21, threads 1008 .. 1023 idle
    AffBwdCase("cp30-p20", 30, 0, 2, 20, 3, 4, True),           # rows_par = 34 > P = 20
]


def affbwd_ld(c):
    return 2 * c.Cp + 3


def affine_bwd_operands(c, exact, seed=0):
    gen = torch.Generator().manual_seed(500 + seed)
    M, ld = c.B * c.P, affbwd_ld(c)
    if exact:
        dy, x = randint64(-4, 4, (M, ld), gen), randint64(-8, 8, (M, ld), gen)
        scale = torch.ones((M, c.Cp), dtype=F64)
        dld = pow2_multiples(c.B, 2, 1, gen)
    else:
        dy, x = (f32r(torch.randn((M, ld), generator=gen, dtype=F64)) for _ in range(2))
        scale = f32r(0.05 + 1.9 * torch.rand((M, c.Cp), generator=gen, dtype=F64))
        dld = f32r(torch.randn(c.B, generator=gen, dtype=F64))
    return dict(dy=dy, x=x, scale=scale, dld=dld)


FINALIZE_CASES = [(0, 4, 3), (1, 1, 1), (7, 4, 5), (1001, 4, 2), (130, 1, 3)]        # (nslots, slot_w, B)
LOGDET_WIDTHS = [1, 8, 60, 64, 65, 200]
LOGDET_NS = [1, 17, 515]
LOGDET_STRIDE = 208                                  # floats between two layers' log_scale vectors in the parameter buffer


def actnorm_logdet_operands(n, seed=0):
    """(params buffer of SENT with integer log_scale vectors scattered in it, [(off, C)]); n = 1 takes the widest layer"""
    gen = torch.Generator().manual_seed(600 + n + seed)
    widths = [200] if n == 1 else [LOGDET_WIDTHS[int(i)] for i in torch.randint(0, len(LOGDET_WIDTHS), (n,), generator=gen)]
    slots = torch.randperm(n, generator=gen).tolist()
    params = torch.full((n * LOGDET_STRIDE + 64,), SENT, dtype=F64)
    refs = []
    for s, C in zip(slots, widths):
        off = 3 + s * LOGDET_STRIDE
        params[off: off + C] = randint64(-3, 3, (C,), gen)
        if C > 64:
            params[off + 64] = 2.0                    # the first channel of the wide-layer loop counts in every wide layer
        refs.append((off, C))
    return params, refs


NLL_CASES = [(1, 64, 8, 8), (3, 64, 6, 8), (5, 64, 7, 7), (2, 1, 50, 50), (1030, 1, 4, 4)]      # (B, P, C, ld)
NLL_SHIFTED = [(1, 64, 8, 8), (3, 64, 6, 8)]         # vector-eligible cases run again one float off a 16-byte boundary (the second: C < ld)
NLL_BLOCK = 1024                                     # ipoke_flow_nll launches one block of 1024 threads: one pass of its log-det loop


def nll_operands(B, P, C, seed=0):
    gen = torch.Generator().manual_seed(700 + B + seed)
    return randint64(-3, 3, (B * P, C), gen), randint64(-20, 20, (B,), gen)


LU_CS = [1, 5, 33, 64]


def lu_operands(C, exact, seed=0):
    """dict(l, u, log_s, perm, sign, lmask, umask, eye) ([C][C] / [C] float64).  l and u carry non-zero values where their masks are
    zero.  exact: sparse strict parts in {-1, 0, 1}, sign = +-1, log_s = 0"""
    gen = torch.Generator().manual_seed(800 + C + seed)
    lmask = torch.tril(torch.ones(C, C, dtype=F64), -1)
    if exact:
        keep = (torch.rand((2, C, C), generator=gen) < min(1.0, 1.5 / C)).to(F64)
        l, u = (randint64(0, 1, (C, C), gen) * 2 - 1) * keep[0], (randint64(0, 1, (C, C), gen) * 2 - 1) * keep[1]
        log_s = torch.zeros(C, dtype=F64)
        junk = randint64(1, 3, (C, C), gen)
    else:
        l, u = (f32r(torch.randn((C, C), generator=gen, dtype=F64) * 0.5 / C ** 0.5) for _ in range(2))
        log_s = f32r(0.2 * torch.randn(C, generator=gen, dtype=F64))
        junk = f32r(torch.randn((C, C), generator=gen, dtype=F64))
    l = l * lmask + junk * (1 - lmask)                # masked-out positions hold values the masks must remove
    u = u * lmask.t() + junk * (1 - lmask.t())
    sign = randint64(0, 1, (C,), gen) * 2 - 1
    p = perm(C, 7 + C)
    return dict(l=l, u=u, log_s=log_s, perm=torch.eye(C, dtype=F64)[p], sign=sign, lmask=lmask, umask=lmask.t().contiguous(),
                eye=torch.eye(C, dtype=F64), p=p)


LU_APPLY_CASES = [(64, 5, 5), (100, 5, 12), (192, 64, 64), (65, 33, 40)]             # (M, C, ld)
LU_WGRAD_CASES = [(2, 64, 64, 64), (3, 64, 5, 12), (1, 48, 33, 40), (5, 16, 8, 8)]   # (B, P8, C, ld)


def lu_apply_operands(M, C, ld, seed=0):
    gen = torch.Generator().manual_seed(900 + M + seed)
    return randint64(-8, 8, (M, ld), gen), randint64(-2, 2, (C, C), gen)


def lu_wgrad_operands(B, P8, C, ld, seed=0):
    gen = torch.Generator().manual_seed(1000 + B + seed)
    M = B * P8
    return randint64(-2, 2, (M, ld), gen), randint64(-3, 3, (M, ld), gen), pow2_multiples(B, 3, 2, gen)


class LuLayout:
    """several jobs in one parameter / float-buffer / workspace triple: every tensor at an offset of its own, gaps in between"""

    def __init__(self, Cs):
        self.jobs, self.Cs = [], list(Cs)
        po = fo = wo = 5
        for C in Cs:
            n = C * C
            j = LuJob()
            j.C = C
            j.p_l, j.p_u, j.p_logs = po, po + n + 3, po + 2 * n + 7
            po += 2 * n + C + 11
            j.b_perm, j.b_sign, j.b_lmask, j.b_umask, j.b_eye = fo, fo + n + 1, fo + n + C + 2, fo + 2 * n + C + 3, fo + 3 * n + C + 4
            fo += 4 * n + C + 9
            j.w_off = wo
            wo += 4 * n + 6
            self.jobs.append(j)
        self.n_params, self.n_fbuf, self.n_ws = po + 16, fo + 16, wo + 16

    def fill(self, mats):
        """(params, fbuf) float64 buffers of SENT with the operands of every job in place"""
        params, fbuf = torch.full((self.n_params,), SENT, dtype=F64), torch.full((self.n_fbuf,), SENT, dtype=F64)
        for j, m in zip(self.jobs, mats):
            n, C = j.C * j.C, j.C
            params[j.p_l: j.p_l + n], params[j.p_u: j.p_u + n], params[j.p_logs: j.p_logs + C] = m["l"].reshape(-1), m["u"].reshape(-1), m["log_s"]
            for k, o, cnt in (("perm", j.b_perm, n), ("sign", j.b_sign, C), ("lmask", j.b_lmask, n), ("umask", j.b_umask, n), ("eye", j.b_eye, n)):
                fbuf[o: o + cnt] = m[k].reshape(-1)
        return params, fbuf

    def written_params(self):
        """mask over the parameter (= gradient) buffer of the elements that belong to some job"""
        w = torch.zeros(self.n_params, dtype=torch.bool)
        for j in self.jobs:
            n = j.C * j.C
            w[j.p_l: j.p_l + n] = True
            w[j.p_u: j.p_u + n] = True
            w[j.p_logs: j.p_logs + j.C] = True
        return w
