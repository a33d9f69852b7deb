"""Phase-by-phase checking of the ConvGRU unroll (csrc/gru.hip: the two fused MFMA kernels, the two fragment-tiling operand kernels,
the element-wise kernels of the launch-per-phase form and the host dispatcher) and of the four stand-alone cell entry points
(csrc/norm.hip, csrc/vae_bwd.hip).  References, operands, the workspace reader, the checkers and the case tables; the test functions
are in test_gru_kernels_cpu.py (which pins the references, the bounds and the host-side hooks) and test_gru_kernels_gpu.py (which runs
the kernels).

* References: plain functions from the formulas of include/ipoke_hip.h and the kernel comments, one per phase, on rows [M = B H W][C]:
  ``conv_ref`` (3 x 3, padding 1, PyTorch-layout weight rounded to the compute type), ``u_ref``, ``hr_ref``, ``hnew_ref``,
  ``update_bwd_ref``, ``gates_bwd_ref``, ``dgrad_ref`` (the data gradient as a convolution with the mirrored taps), ``wgrad_ref``.  They
  compute in the dtype of their operands and return the value and the magnitude ``mag`` of the terms it sums.  ``unroll`` chains them:
  with ``tdt=None`` in float64 without any rounding (the unforced reference, equal to autograd through the oracle's ConvGRU), with a
  storage type in float32 rounded to that type wherever the kernels store -- the restatement, whose result has the shape of a workspace.
* Teacher forcing: the unroll keeps every operand of every (cell, step) in its workspace (ipoke_gru_workspace_layout says where), so
  ``check_forward`` / ``check_backward`` check each phase of each (cell, step) on the inputs the kernel itself stored.  A rounding flip
  is not carried forward, and the bounds are units in the last place of the local magnitude.  In the backward pass d o and d ur are
  stored and g, d u, d h1, d h2 and the two data-gradient results are not: the checker feeds the data-gradient convolutions from the
  stored d o / d ur, rounds where the kernel rounds, and carries its own g chain TOGETHER with the magnitude of the rounding error
  that chain can hold (one unit of every rounded value the workspace does not have, propagated through the formulas).
* Bounds.  The unit is the ulp of the output type taken of ``mag``.  Values stored as bf16: 1 unit (+ the propagated error).  fp32
  values: ``max(4 x yardstick, 4)`` units, the yardstick being the worst error of the restatement on the very operands of the GPU
  tests, which test_gru_kernels_cpu.py measures and holds against the table below (rounded up, not padded); the margin covers the
  device's expf / tanhf and fused multiply-adds.  The weight and bias gradients are fp32 functions of stored operands: fp32 units,
  no bf16 allowance.  d x0 and d h0 are fp32 sums of rounded values the workspace does not hold: fp32 units + the propagated error.

  Recorded yardsticks (units; bf16-stored values are bounded by 1 unit whatever the yardstick, which has to stay below it):

      phase      f32    bf16        phase      f32    bf16        output (fp32)   f32 operands   bf16 operands
      ur         3.5    0.5         dh1        0.9    0.5         dx0             0.5            0.5
      u          1.9    0.5         dxhr       4.1    0.5         dh0             0.5            0.5
      hr         2.2    0.6         dur_u      1.8    0.5         dw_ur           3.7            3.5
      o          3.4    0.5         dur_r      2.4    0.5         db_ur           1.1            0.5
      hn         1.6    0.6         dh2        2.1    0.5         dw_o            2.8            3.6
      do         1.5    0.5         dxh        5.3    0.5         db_o            0.7            0.5
      du         2.0    0.5

* Exact operands: every weight and bias zero, so sigmoid(0) = 1/2 and tanh(0) = 0 exactly: u = r = 1/2, hr = h / 2, o = 0,
  h' = h / 2; integer x0, and h0 and d_out multiples of 2^T, so that every buffer of both directions is a small integer (g of the
  last cell is d_out[t] + g(t + 1) / 2, d o = g / 2, d u = -g h, d ur = [-g h / 4 | 0], d h0 = g(L - 1, 0) / 2, d x0 = 0; the cells below
  the last receive no gradient).  The weight gradients of the LAST cell are not zero -- they are sums of products of these integers
  below 2^24, exact in fp32 in any order -- those of the cells below are.  Compared bit for bit, zeros of either sign alike.
"""
import collections
import ctypes

import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from tests.flow_exact import (DTYPES, F64, GUARD, SENT, assert_close_ulp, assert_same, assert_units, check_guard, guarded,  # noqa: F401
                              randint64, restate, round_up, ulp_of)

F32 = torch.float32
BF16 = torch.bfloat16
TDT = {"f32": F32, "bf16": BF16}

# worst error of the restatement against float64 in units (test_gru_kernels_cpu.py measures and asserts them)
YARDSTICK = {
    "ur_f32": 3.5, "ur_bf16": 0.5,
    "u_f32": 1.9, "u_bf16": 0.5,
    "hr_f32": 2.2, "hr_bf16": 0.6,
    "o_f32": 3.4, "o_bf16": 0.5,
    "hn_f32": 1.6, "hn_bf16": 0.6,
    "do_f32": 1.5, "do_bf16": 0.5,
    "du_f32": 2.0, "du_bf16": 0.5,
    "dh1_f32": 0.9, "dh1_bf16": 0.5,
    "dxhr_f32": 4.1, "dxhr_bf16": 0.5,
    "dur_u_f32": 1.8, "dur_u_bf16": 0.5,
    "dur_r_f32": 2.4, "dur_r_bf16": 0.5,
    "dh2_f32": 2.1, "dh2_bf16": 0.5,
    "dxh_f32": 5.3, "dxh_bf16": 0.5,
    "dx0_f32": 0.5, "dx0_bf16": 0.5,
    "dh0_f32": 0.5, "dh0_bf16": 0.5,
    "dw_ur_f32": 3.7, "dw_ur_bf16": 3.5,
    "db_ur_f32": 1.1, "db_ur_bf16": 0.5,
    "dw_o_f32": 2.8, "dw_o_bf16": 3.6,
    "db_o_f32": 0.7, "db_o_bf16": 0.5,
}
PHASES = ("ur", "u", "hr", "o", "hn", "do", "du", "dh1", "dxhr", "dur_u", "dur_r", "dh2", "dxh")      # stored (or rounded) in the compute type
FP32_OUT = ("dx0", "dh0", "dw_ur", "db_ur", "dw_o", "db_o")                                            # fp32 whatever the compute type


def gpu_bound(name, dt):
    """units allowed on the device: 1 for a value rounded to bf16, max(4 x yardstick, 4) for an fp32 value"""
    if dt == "bf16" and name in PHASES:
        return 1.0
    return max(4.0 * YARDSTICK[f"{name}_{dt}"], 4.0)


# ------------------------------------------------------------------ cases
class Case(collections.namedtuple("Case", "B T L Cx Ch H W dt form force0 pad")):
    """form: the form the call must take (1 fused, 0 launch-per-phase); force0: ipoke_gru_set_fused(0) around the call; pad: elements
    added to ldx, ldh and ldo (a multiple of 16 bytes)"""
    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def Kc(self):
        return self.Cx + self.Ch

    @property
    def id(self):
        return (f"{'fused' if self.form else 'forced' if self.force0 else 'phase'}-{self.dt}-B{self.B}T{self.T}L{self.L}-{self.Cx}x{self.Ch}-"
                f"{self.H}x{self.W}" + (f"-pad{self.pad}" if self.pad else ""))

    def desc(self):
        d = _lib.GruDesc()
        d.B, d.T, d.L, d.Cx, d.Ch, d.H, d.W = self.B, self.T, self.L, self.Cx, self.Ch, self.H, self.W
        return d


FUSED_BTL = [(2, 3, 1), (2, 3, 2), (2, 3, 3), (1, 1, 2), (3, 2, 4)]
FUSED_CASES = [Case(B, T, L, Ch, Ch, 8, 8, "bf16", 1, False, 0) for Ch in (32, 64) for B, T, L in FUSED_BTL]
FUSED_PADDED = [Case(2, 3, 2, Ch, Ch, 8, 8, "bf16", 1, False, 8) for Ch in (32, 64)]
# fits neither kernel's LDS budget together with its backward pass: must take the launch-per-phase form in both directions by itself
NOT_FITTING = [Case(1, 2, 6, 64, 64, 8, 8, "bf16", 0, False, 0)]
PHASE_GEOMS = [(2, 3, 2, 32, 32, 8, 8), (2, 3, 3, 32, 32, 8, 8), (2, 2, 1, 8, 16, 4, 8), (1, 1, 1, 16, 16, 8, 8), (2, 3, 2, 16, 16, 2, 2)]
PHASE_CASES = [Case(*g, dt, 0, True, DTYPES[dt][2]) for dt in ("bf16", "f32") for g in PHASE_GEOMS]
ALL_CASES = FUSED_CASES + FUSED_PADDED + NOT_FITTING + PHASE_CASES
# the cases the separation test mutates: one per form and dtype with T >= 2 and L >= 2
SEPARATION_CASES = [FUSED_CASES[2], PHASE_CASES[0], PHASE_CASES[5]]
LDS_LIMIT = 163840                  # bytes of LDS of an MI355X compute unit

STANDALONE_M = 70
STANDALONE_CH = (1, 5, 64)


def layout(c):
    """ipoke_gru_workspace_layout as a dict: name -> (byte offset, row width in elements), 'bytes', and the weight-operand slots"""
    out = (ctypes.c_int64 * 21)()
    d = c.desc()
    n = _lib.lib().ipoke_gru_workspace_layout(ctypes.byref(d), DTYPES[c.dt][0], out, 21)
    assert n == 21, _lib.lib().ipoke_last_error()
    lay = {k: (out[2 * i], out[2 * i + 1]) for i, k in enumerate(("XH", "XHR", "UR", "U", "O", "DO", "DUR"))}
    lay["bytes"] = out[14]
    lay["WOP"], lay["wop_cell"] = out[15], out[16]
    lay["wop"] = {"ur": out[17], "urT": out[18], "o": out[19], "oT": out[20]}
    return lay


# ------------------------------------------------------------------ operands
def rnd(v, tdt):
    """the values of v rounded as the kernels round: to fp32, then to the storage type; dtype kept"""
    return v if tdt is None else v.to(F32).to(tdt).to(v.dtype)


def operands(c, exact):
    """x0 [M][Cx], h0 [M][Ch], dout [T][M][Ch] (float64, representable in the case's type), weights: per cell w_ur [2Ch][Kc][3][3], b_ur,
    w_o [Ch][Kc][3][3], b_o (float64 holding fp32 values; cell 0 takes Cx inputs, the others Ch)"""
    gen = torch.Generator().manual_seed(1000 * c.B + 100 * c.T + 10 * c.L + c.Ch + c.H + (7 if exact else 0))
    tdt = TDT[c.dt]
    ws = []
    for l in range(c.L):
        Kc = (c.Cx if l == 0 else c.Ch) + c.Ch
        for shape in ((2 * c.Ch, Kc, 3, 3), (2 * c.Ch,), (c.Ch, Kc, 3, 3), (c.Ch,)):
            if exact:
                ws.append(torch.zeros(shape, dtype=F64))
            else:
                s = 0.3 if len(shape) == 1 else 1.5 / (9 * Kc) ** 0.5
                ws.append((torch.randn(shape, generator=gen, dtype=F64) * s).to(F32).to(F64))
    if exact:
        x0 = randint64(-9, 9, (c.M, c.Cx), gen)
        h0 = randint64(-3, 3, (c.M, c.Ch), gen) * 2.0 ** c.T
        dout = randint64(-2, 2, (c.T, c.M, c.Ch), gen) * 2.0 ** c.T
    else:
        x0 = rnd(torch.randn(c.M, c.Cx, generator=gen, dtype=F64), tdt)
        h0 = rnd(torch.randn(c.M, c.Ch, generator=gen, dtype=F64), tdt)
        dout = rnd(torch.randn(c.T, c.M, c.Ch, generator=gen, dtype=F64), tdt)
    return {"x0": x0, "h0": h0, "dout": dout, "w": ws}


# ------------------------------------------------------------------ phase references
def sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def to_map(rows, H, W):
    return rows.reshape(-1, H, W, rows.shape[-1]).permute(0, 3, 1, 2)


def to_rows(m):
    return m.permute(0, 2, 3, 1).reshape(-1, m.shape[1])


def conv_ref(a, w, b, H, W):
    """rows a [M][K] (*) w [N][K][3][3] (padding 1) + b [N] -> ([M][N], mag)"""
    y = F.conv2d(to_map(a, H, W), w, None, padding=1)
    mag = F.conv2d(to_map(a.abs(), H, W), w.abs(), None, padding=1)
    if b is not None:
        y, mag = y + b.view(1, -1, 1, 1), mag + b.abs().view(1, -1, 1, 1)
    return to_rows(y), to_rows(mag)


def dgrad_ref(dy, w, H, W, mirror=True):
    """the data gradient of conv_ref: d a[p][k] = sum over taps and n of dy[p + delta(tap)][n] w[n][k][8 - tap] -- a convolution of dy
    with the transposed weight, taps mirrored"""
    wt = w.permute(1, 0, 2, 3)
    return conv_ref(dy, wt.flip(2, 3) if mirror else wt, None, H, W)


def wgrad_ref(a, dy, H, W):
    """d w[n][k][tap] = sum over the rows of dy[p][n] a[p + delta(tap)][k]; rows of any number of images -> ([N][K][3][3], mag)"""
    shape = (dy.shape[1], a.shape[1], 3, 3)
    dw = torch.nn.grad.conv2d_weight(to_map(a, H, W), shape, to_map(dy, H, W), padding=1)
    mag = torch.nn.grad.conv2d_weight(to_map(a.abs(), H, W), shape, to_map(dy.abs(), H, W), padding=1)
    return dw, mag


def u_ref(ur, Ch, swap=False):
    u = sig(ur[:, Ch:2 * Ch] if swap else ur[:, :Ch])
    return u, u


def hr_ref(h, ur, Ch, swap=False):
    v = h * sig(ur[:, :Ch] if swap else ur[:, Ch:2 * Ch])
    return v, v.abs()


def hnew_ref(h, u, o):
    """h' = h (1 - u) + tanh(o) u; 1 - u is itself a difference of the terms 1 and u"""
    th = torch.tanh(o)
    return h * (1.0 - u) + th * u, h.abs() * (1.0 + u.abs()) + (th * u).abs()


def update_bwd_ref(g, o, u, h):
    """(d o, d u, d h1) = (g u (1 - tanh(o)^2), g (tanh(o) - h), g (1 - u)) and their magnitudes"""
    th = torch.tanh(o)
    return ((g * u * (1.0 - th * th), g * (th - h), g * (1.0 - u)),
            (g.abs() * u.abs() * (1.0 + th * th), g.abs() * (th.abs() + h.abs()), g.abs() * (1.0 + u.abs())))


def gates_bwd_ref(ur, h, d_hr, d_u, d_h1, Ch):
    """(d ur[:Ch], d ur[Ch:], d h2) = (d u u (1 - u), d hr h r (1 - r), d h1 + d hr r) with u, r = sigmoid(ur) and their magnitudes"""
    u, r = sig(ur[:, :Ch]), sig(ur[:, Ch:2 * Ch])
    return ((d_u * u * (1.0 - u), d_hr * h * r * (1.0 - r), d_h1 + d_hr * r),
            (d_u.abs() * u * (1.0 + u), (d_hr * h).abs() * r * (1.0 + r), d_h1.abs() + d_hr.abs() * r))


# ------------------------------------------------------------------ the chained unroll
def unroll(c, ops, tdt=None, cdt=F64, mut=None):
    """Both directions with the phases chained as SpadeCondMotionModel.forward drives the ConvGRU (every cell starts from h0, cell 0
    sees the constant x0).  tdt None: no rounding anywhere (the unforced reference).  tdt a storage type: weights rounded to it and
    every value rounded to it where the kernels store one -- in cdt = float32 the restatement.  Returns a workspace dict (the stored
    buffers as [L][T][M][C], out [T][M][Ch], the fp32 outputs, and the intermediates a real workspace does not keep).
    mut: a deliberate defect for the separation test."""
    q = lambda v: rnd(v, tdt)                                                                 # noqa: E731
    B, T, L, Cx, Ch, H, W = c[:7]
    x0, h0, dout = (ops[k].to(cdt) for k in ("x0", "h0", "dout"))
    w = [q(ops["w"][i].to(cdt)) if i % 2 == 0 else ops["w"][i].to(cdt) for i in range(4 * L)]
    wf = list(w)
    if mut == "tap":                       # a corner tap of the last cell's gate convolution missing in the forward pass
        wf[4 * (L - 1)] = w[4 * (L - 1)].clone()
        wf[4 * (L - 1)][:, :, 0, 0] = 0
    swap = mut == "swap"
    keys = ("XH", "XHR", "UR", "U", "O", "HN", "DO", "DUR", "G", "DU", "DH1", "DH2", "DXH", "DXHR")
    S = {k: [[None] * T for _ in range(L)] for k in keys}
    for t in range(T):
        for l in range(L):
            x = x0 if l == 0 else S["HN"][l - 1][t]
            h = h0 if t == 0 else S["HN"][l][t - 1]
            xh = torch.cat([x, h], 1)
            ur = q(conv_ref(xh, wf[4 * l], w[4 * l + 1], H, W)[0])
            u = q(u_ref(ur, Ch, swap)[0])
            xhr = torch.cat([x, q(hr_ref(h, ur, Ch, swap)[0])], 1)
            o = q(conv_ref(xhr, w[4 * l + 2], w[4 * l + 3], H, W)[0])
            for k, v in (("XH", xh), ("XHR", xhr), ("UR", ur), ("U", u), ("O", o), ("HN", q(hnew_ref(h, u, o)[0]))):
                S[k][l][t] = v
    dxh, dxhr, dh2 = [None] * L, [None] * L, [None] * L
    dx0 = torch.zeros(c.M, Cx, dtype=cdt)
    for t in range(T - 1, -1, -1):
        for l in range(L - 1, -1, -1):
            cx = Cx if l == 0 else Ch
            g = torch.zeros(c.M, Ch, dtype=cdt)
            if t + 1 < T:
                g = g + (0 if mut == "gsrc" else dh2[l]) + dxh[l][:, cx:]
            g = g + (dxh[l + 1][:, :Ch] + dxhr[l + 1][:, :Ch] if l + 1 < L else dout[t])
            h = S["XH"][l][t][:, cx:]
            d_o, d_u, d_h1 = (q(v) for v in update_bwd_ref(g, S["O"][l][t], S["U"][l][t], h)[0])
            dxhr[l] = q(dgrad_ref(d_o, w[4 * l + 2], H, W, mirror=not (mut == "mirror" and l == 0))[0])
            a, b, h2 = (q(v) for v in gates_bwd_ref(S["UR"][l][t], h, dxhr[l][:, cx:], d_u, d_h1, Ch)[0])
            dh2[l] = h2
            dur = torch.cat([a, b], 1)
            dxh[l] = q(dgrad_ref(dur, w[4 * l], H, W)[0])
            if l == 0 and not (mut == "dx0_last" and t == 0):
                dx0 = dx0 + (dxh[0][:, :Cx] + dxhr[0][:, :Cx])
            for k, v in (("DO", d_o), ("DUR", dur), ("G", g), ("DU", d_u), ("DH1", d_h1), ("DH2", h2), ("DXH", dxh[l]), ("DXHR", dxhr[l])):
                S[k][l][t] = v
    dh0 = torch.zeros(c.M, Ch, dtype=cdt)
    for l in range(L):
        if not (mut == "dh0_cell" and l == L - 1):
            dh0 = dh0 + (dh2[l] + dxh[l][:, (Cx if l == 0 else Ch):])
    dw = []
    for l in range(L):
        for src, dy in (("XH", "DUR"), ("XHR", "DO")):
            a, d = torch.cat(S[src][l], 0), torch.cat(S[dy][l], 0)
            dw += [wgrad_ref(a, d, H, W)[0], d.sum(0)]
    ws = {k: [[rnd(v, tdt).to(tdt or F64) for v in row] for row in S[k]] for k in keys}
    ws["out"] = [ws["HN"][L - 1][t] for t in range(T)]
    ws["dx0"], ws["dh0"], ws["dw"] = (dx0, dh0, dw) if tdt is None else (dx0.to(F32), dh0.to(F32), [v.to(F32) for v in dw])
    return ws


def canon(t):
    """zeros of either sign alike"""
    return t + 0.0


# ------------------------------------------------------------------ reading a device workspace
def read_workspace(ws_bytes, c, lay, names=("XH", "XHR", "UR", "U", "O", "DO", "DUR")):
    """the per-(cell, step) buffers of a workspace (uint8 tensor, CPU) as {name: [L][T] of [M][width] tensors of the case's type}.  Cell 0
    has Cx + Ch operand columns like every other cell (L > 1 requires Cx = Ch)."""
    tdt, esz = TDT[c.dt], 2 if c.dt == "bf16" else 4
    out = {}
    for k in names:
        off, wd = lay[k]
        n = c.L * c.T * c.M * wd
        v = ws_bytes[off: off + n * esz].clone().view(tdt).view(c.L, c.T, c.M, wd)
        out[k] = [[v[l, t] for t in range(c.T)] for l in range(c.L)]
    return out


# ------------------------------------------------------------------ teacher-forced checkers
class Tally:
    """collects the worst error per phase in units; with `dt` set (the GPU test, the separation test) a miss raises at once"""
    def __init__(self, dt, enforce=True):
        self.dt, self.enforce, self.worst = dt, enforce, {}

    def cmp(self, name, got, ref, mag, prop=None, where=""):
        unit = ulp_of(mag, F32 if name in FP32_OUT else TDT[self.dt])
        err = (got.to(F64) - ref).abs()
        if prop is not None:
            err = (err - prop).clamp(min=0.0)
        e = err / unit
        self.worst[name] = max(self.worst.get(name, 0.0), float(e.max()) if e.numel() else 0.0)
        if self.enforce:
            bound = gpu_bound(name, self.dt)
            bad = ~(e <= bound)
            if bool(bad.any()):
                i = int(torch.nonzero(bad.reshape(-1))[0])
                raise AssertionError(f"{name} {where}: {int(bad.sum())} elements beyond {bound} units (worst {float(e.max()):.2f}); first at "
                                     f"element {i}: got {float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}")


def weights64(c, ops):
    tdt = TDT[c.dt]
    return [rnd(v, tdt) if i % 2 == 0 else v for i, v in enumerate(ops["w"])]


def check_routing(c, ops, ws):
    """bit for bit: which buffer feeds which consumer.  Returns HN [L][T]: the one stored value of every h'."""
    sdt = ws["XH"][0][0].dtype                # the case's type (float64 for the unforced reference)
    B, T, L, Cx, Ch = c[:5]
    HN = [[None] * T for _ in range(L)]
    for l in range(L):
        for t in range(T):
            copies = []
            if t + 1 < T:
                copies.append((f"h-half of XH[{l},{t + 1}]", ws["XH"][l][t + 1][:, c.Kc - Ch:]))
            if l + 1 < L:
                copies += [(f"x-half of XH[{l + 1},{t}]", ws["XH"][l + 1][t][:, :Ch]), (f"x-half of XHR[{l + 1},{t}]", ws["XHR"][l + 1][t][:, :Ch])]
            else:
                copies.append((f"out[{t}]", ws["out"][t]))
            HN[l][t] = copies[0][1].contiguous()
            for name, v in copies[1:]:
                assert_same(v.contiguous(), HN[l][t], f"h'({l},{t}): {name} against {copies[0][0]}")
    for l in range(L):
        cx = Cx if l == 0 else Ch
        for t in range(T):
            x = ops["x0"].to(sdt) if l == 0 else HN[l - 1][t]
            h = ops["h0"].to(sdt) if t == 0 else HN[l][t - 1]
            assert_same(ws["XH"][l][t][:, :cx].contiguous(), x, f"x-half of XH[{l},{t}]")
            assert_same(ws["XH"][l][t][:, cx:].contiguous(), h, f"h-half of XH[{l},{t}]")
            assert_same(ws["XHR"][l][t][:, :cx].contiguous(), ws["XH"][l][t][:, :cx].contiguous(), f"x-half of XHR[{l},{t}]")
    return HN


def check_forward(c, ops, ws, tally):
    """every phase of every (cell, step) on the operands the workspace holds"""
    T, L, Cx, Ch, H, W = c[1:7]
    HN = check_routing(c, ops, ws)
    w = weights64(c, ops)
    for l in range(L):
        cx = Cx if l == 0 else Ch
        for t in range(T):
            at = f"(cell {l}, step {t})"
            xh, xhr, ur, u, o = (ws[k][l][t].to(F64) for k in ("XH", "XHR", "UR", "U", "O"))
            h = xh[:, cx:]
            tally.cmp("ur", ws["UR"][l][t][:, :2 * Ch], *conv_ref(xh, w[4 * l], w[4 * l + 1], H, W), where=at)
            tally.cmp("u", ws["U"][l][t], *u_ref(ur, Ch), where=at)
            tally.cmp("hr", ws["XHR"][l][t][:, cx:], *hr_ref(h, ur, Ch), where=at)
            tally.cmp("o", ws["O"][l][t][:, :Ch], *conv_ref(xhr, w[4 * l + 2], w[4 * l + 3], H, W), where=at)
            tally.cmp("hn", HN[l][t], *hnew_ref(h, u, o[:, :Ch]), where=at)


def check_backward(c, ops, ws, tally):
    """d o and d ur of every (cell, step), d x0, d h0 and the weight / bias gradients on the operands the workspace holds; g, d u, d h1,
    d h2 and the data-gradient results are the checker's own (value, error magnitude) pairs.  Where ws has the intermediates too (the
    restatement), they are compared as well."""
    T, L, Cx, Ch, H, W = c[1:7]
    dt, tdt = c.dt, TDT[c.dt]
    w = weights64(c, ops)
    q = lambda v: rnd(v, tdt)                                                                 # noqa: E731
    ulp = lambda m: ulp_of(m, tdt)                                                            # noqa: E731
    own = lambda name, m: gpu_bound(name, dt) * ulp(m)                                         # noqa: E731  what the device may add to a value
    dxh, dxhr, dh2 = [None] * L, [None] * L, [None] * L
    z = torch.zeros(c.M, Cx, dtype=F64)
    dx0, dx0_mag, dx0_err = z, z, z
    has = "DU" in ws
    for t in range(T - 1, -1, -1):
        for l in range(L - 1, -1, -1):
            at = f"(cell {l}, step {t})"
            cx = Cx if l == 0 else Ch
            g = torch.zeros(c.M, Ch, dtype=F64)
            eg = torch.zeros(c.M, Ch, dtype=F64)
            if t + 1 < T:
                g, eg = g + dh2[l][0] + dxh[l][0][:, cx:], eg + dh2[l][1] + dxh[l][1][:, cx:]
            if l + 1 < L:
                g = g + dxh[l + 1][0][:, :Ch] + dxhr[l + 1][0][:, :Ch]
                eg = eg + dxh[l + 1][1][:, :Ch] + dxhr[l + 1][1][:, :Ch]
            else:
                g = g + ops["dout"][t]
            ur, u, o = (ws[k][l][t].to(F64) for k in ("UR", "U", "O"))
            o = o[:, :Ch]
            h = ws["XH"][l][t].to(F64)[:, cx:]
            (d_o, d_u, d_h1), (m_o, m_u, m_h1) = update_bwd_ref(g, o, u, h)
            p_o, p_u, p_h1 = (v.abs() for v in update_bwd_ref(eg, o, u, h)[0])               # the phase is linear in g
            tally.cmp("do", ws["DO"][l][t][:, :Ch], d_o, m_o, p_o, where=at)
            raw_u, raw_h1 = d_u, d_h1
            d_u, e_u, d_h1, e_h1 = q(d_u), p_u + own("du", m_u), q(d_h1), p_h1 + own("dh1", m_h1)
            v, m = dgrad_ref(ws["DO"][l][t].to(F64)[:, :Ch], w[4 * l + 2], H, W)
            dxhr[l] = (q(v), own("dxhr", m))
            d_hr, e_hr = dxhr[l][0][:, cx:], dxhr[l][1][:, cx:]
            (a, b, h2), (m_a, m_b, m_h2) = gates_bwd_ref(ur, h, d_hr, d_u, d_h1, Ch)
            zero = torch.zeros_like(e_u)
            p_a = gates_bwd_ref(ur, h, zero, e_u, zero, Ch)[0][0].abs()
            p_b = gates_bwd_ref(ur, h, e_hr, zero, zero, Ch)[0][1].abs()
            e_h2 = gates_bwd_ref(ur, h, e_hr, zero, e_h1, Ch)[0][2].abs() + own("dh2", m_h2)
            tally.cmp("dur_u", ws["DUR"][l][t][:, :Ch], a, m_a, p_a, where=at)
            tally.cmp("dur_r", ws["DUR"][l][t][:, Ch:2 * Ch], b, m_b, p_b, where=at)
            dh2[l] = (q(h2), e_h2)
            v, m = dgrad_ref(ws["DUR"][l][t].to(F64)[:, :2 * Ch], w[4 * l], H, W)
            dxh[l] = (q(v), own("dxh", m))
            if has:
                tally.cmp("du", ws["DU"][l][t], raw_u, m_u, p_u, where=at)
                tally.cmp("dh1", ws["DH1"][l][t], raw_h1, m_h1, p_h1, where=at)
                tally.cmp("dxhr", ws["DXHR"][l][t], *dgrad_ref(ws["DO"][l][t].to(F64)[:, :Ch], w[4 * l + 2], H, W), where=at)
                tally.cmp("dh2", ws["DH2"][l][t], h2, m_h2, e_h2 - own("dh2", m_h2), where=at)
                tally.cmp("dxh", ws["DXH"][l][t], *dgrad_ref(ws["DUR"][l][t].to(F64)[:, :2 * Ch], w[4 * l], H, W), where=at)
            if l == 0:
                a0, b0 = dxh[0][0][:, :Cx], dxhr[0][0][:, :Cx]
                dx0, dx0_mag, dx0_err = dx0 + a0 + b0, dx0_mag + a0.abs() + b0.abs(), dx0_err + dxh[0][1][:, :Cx] + dxhr[0][1][:, :Cx]
    tally.cmp("dx0", ws["dx0"], dx0, dx0_mag, dx0_err)
    dh0, dh0_mag, dh0_err = (torch.zeros(c.M, Ch, dtype=F64) for _ in range(3))
    for l in range(L):
        cx = Cx if l == 0 else Ch
        a0, b0 = dh2[l][0], dxh[l][0][:, cx:]
        dh0, dh0_mag, dh0_err = dh0 + a0 + b0, dh0_mag + a0.abs() + b0.abs(), dh0_err + dh2[l][1] + dxh[l][1][:, cx:]
    tally.cmp("dh0", ws["dh0"], dh0, dh0_mag, dh0_err)
    for l in range(L):
        for j, (src, dy, n, name) in enumerate((("XH", "DUR", 2 * Ch, "ur"), ("XHR", "DO", Ch, "o"))):
            a = torch.cat([v.to(F64) for v in ws[src][l]], 0)
            d = torch.cat([v.to(F64)[:, :n] for v in ws[dy][l]], 0)
            tally.cmp("dw_" + name, ws["dw"][4 * l + 2 * j], *wgrad_ref(a, d, H, W), where=f"cell {l}")
            tally.cmp("db_" + name, ws["dw"][4 * l + 2 * j + 1], d.sum(0), d.abs().sum(0), where=f"cell {l}")


def assert_exact(c, ws, ref, backward):
    """a workspace on the exact operand set against the float64 unroll, bit for bit (zeros of either sign alike)"""
    tdt = TDT[c.dt]
    names = ["XH", "XHR", "UR", "U", "O"] + (["DO", "DUR"] if backward else [])
    width = {"XH": c.Kc, "XHR": c.Kc, "UR": 2 * c.Ch, "U": c.Ch, "O": c.Ch, "DO": c.Ch, "DUR": 2 * c.Ch}
    for k in names:
        for l in range(c.L):
            for t in range(c.T):
                assert_same(canon(ws[k][l][t][:, :width[k]].contiguous()), canon(ref[k][l][t].to(tdt)), f"{k}[{l},{t}]")
    for t in range(c.T):
        assert_same(canon(ws["out"][t].contiguous()), canon(ref["out"][t].to(tdt)), f"out[{t}]")
    if backward:
        assert_same(canon(ws["dx0"]), canon(ref["dx0"].to(F32)), "d x0")
        assert_same(canon(ws["dh0"]), canon(ref["dh0"].to(F32)), "d h0")
        for i, (a, b) in enumerate(zip(ws["dw"], ref["dw"])):
            assert_same(canon(a), canon(b.to(F32)), f"gradient of weight tensor {i % 4} of cell {i // 4}")


# ------------------------------------------------------------------ the fragment-tiled operands of the fused kernels
def tile_operand_ref(w, tdt=BF16):
    """gru_tile_operand_kernel: w [N][Kc][3][3] -> element i = 512 (nf nfr + q) + 8 lane + e is w[16 nf + (lane & 15)][c][tap] with
    tap Kc + c = 32 q + 8 (lane >> 4) + e"""
    N, Kc = w.shape[:2]
    i = torch.arange(N * 9 * Kc)
    e, lane, fq = i & 7, (i >> 3) & 63, i >> 9
    nfr = 9 * Kc // 32
    q, nf = fq % nfr, fq // nfr
    o, kk = nf * 16 + (lane & 15), q * 32 + (lane >> 4) * 8 + e
    return w.reshape(N, Kc, 9)[o, kk % Kc, kk // Kc].to(F32).to(tdt)


def tile_operand_t_ref(w, tdt=BF16):
    """gru_tile_operand_t_kernel: w [Nw][Kc][3][3] -> element i is w[c][16 nf + (lane & 15)][8 - tap] with tap Nw + c = 32 q + 8 (lane >> 4) + e"""
    Nw, Kc = w.shape[:2]
    i = torch.arange(Kc * 9 * Nw)
    e, lane, fq = i & 7, (i >> 3) & 63, i >> 9
    nfr = 9 * Nw // 32
    q, nf = fq % nfr, fq // nfr
    j, kk = nf * 16 + (lane & 15), q * 32 + (lane >> 4) * 8 + e
    return w.reshape(Nw, Kc, 9)[kk % Nw, j, 8 - kk // Nw].to(F32).to(tdt)


# ------------------------------------------------------------------ the stand-alone entry points
def standalone_operands(Ch, dt, exact, M=STANDALONE_M):
    """ur [M][2Ch], o [M][Ch], h, u, the incoming gradients g (d h'), d_hr, d_u [M][Ch] (float64, representable in the type).  Exact: the
    pre-activations are zero and u = 1/2 (sigmoid and tanh exact), everything else small integers."""
    gen = torch.Generator().manual_seed(31 * Ch + (1 if exact else 0) + (2 if dt == "bf16" else 0))
    tdt = TDT[dt]
    if exact:
        i = lambda: randint64(-6, 6, (M, Ch), gen) * 4.0                                       # noqa: E731
        return {"ur": torch.zeros(M, 2 * Ch, dtype=F64), "o": torch.zeros(M, Ch, dtype=F64), "h": i(), "u": torch.full((M, Ch), 0.5, dtype=F64),
                "g": i(), "d_hr": i(), "d_u": i()}
    r = lambda *s: rnd(torch.randn(*s, generator=gen, dtype=F64), tdt)                        # noqa: E731
    return {"ur": r(M, 2 * Ch) * 2.0, "o": r(M, Ch) * 2.0, "h": r(M, Ch), "u": rnd(torch.rand(M, Ch, generator=gen, dtype=F64), tdt),
            "g": r(M, Ch), "d_hr": r(M, Ch), "d_u": r(M, Ch)}


def standalone_phases(o, Ch, d_u_given=True):
    """what the four entry points compute from standalone_operands, name -> (value, mag), in the dtype of the operands: ipoke_gru_gates
    (u, hr), ipoke_gru_update (hn), ipoke_gru_update_bwd (do, du, dh1 = its d_h) and ipoke_gru_gates_bwd (dur_u, dur_r, dh2 = its d_h:
    d hr r, there is no d h1 to add)"""
    zero = torch.zeros_like(o["h"])
    (d_o, d_u, d_h1), (m_o, m_u, m_h1) = update_bwd_ref(o["g"], o["o"], o["u"], o["h"])
    (a, b, h2), (m_a, m_b, m_h2) = gates_bwd_ref(o["ur"], o["h"], o["d_hr"], o["d_u"] if d_u_given else zero, zero, Ch)
    return {"u": u_ref(o["ur"], Ch), "hr": hr_ref(o["h"], o["ur"], Ch), "hn": hnew_ref(o["h"], o["u"], o["o"]),
            "do": (d_o, m_o), "du": (d_u, m_u), "dh1": (d_h1, m_h1), "dur_u": (a, m_a), "dur_r": (b, m_b), "dh2": (h2, m_h2)}
