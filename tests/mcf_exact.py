"""Phase-by-phase checking of the masked-convolution flow kernels (csrc/mcf.hip: the per-layer forward / inverse / backward kernels;
csrc/mcf_unit.hip: the fused MaCowUnit, one workgroup per sample; csrc/mcf_unit_split.hip: its row-split and two-unit forms).
References, operands, the teacher-forced checkers, the case tables and the yardsticks; the test functions are in
test_mcf_kernels_cpu.py (which pins the references, the input conditions and the yardsticks) and test_mcf_kernels_gpu.py (which runs
the kernels).

* References: plain functions from the formulas of include/ipoke_hip.h and the kernel comments, one per phase, on rows [M = 64 B][.]
  (position p = 8 y + x inside a sample): ``shiftconv_ref`` (six taps; input (y + ky + oy, x + kx + ox) feeds output (y, x), the four
  (kh, kw, oy, ox) of ``OFFSETS`` restated from the comment of mcf_geom), ``hidden_ref`` (ELU(c) next to the prepared conditioning
  rows), ``params_ref`` (W2 a2 + bias2 -> mu, s), ``coupling_ref`` (scale = tanh(s / 2) + 1, y = scale x + mu, log-det terms
  log scale), ``post_actnorm_ref`` (y exp(ls) + b; the constant log-det left out as the kernels leave it out), ``dparams_ref``
  ([dy' | ds], ds = (dy' x + dld / scale) (1 - (scale - 1)^2) / 2, dy' = dy exp(ls) behind a fused ActNorm), ``dc_ref``
  ((dparams W2[:, :H]) ELU' from the stored output), ``dx_ref`` (dy' scale + the adjoint shifted convolution), ``dbias_ref`` and
  ``post_part_ref`` (d_log_scale = sum dy (y_post - b) + 64 dld, d_bias = sum dy), ``inverse_layer`` (x = (y - mu) / (scale + 1e-12),
  strip by strip).  They compute in the dtype of their operands and return the value and the magnitude ``mag`` of the terms it sums.
  ``chain`` composes four or eight layers: ``tdt=None`` float64 without any rounding (equal to the oracle's MaskedConvFlow / MaCowUnit
  and autograd through them), with a storage type the fp32 restatement, rounded wherever the kernels store or stage (x -> T for the
  first contraction, a2 -> T, dparams -> T, dc -> T).  ``fast=True`` is the algebra of the fused and split kernels (mcf_unit_dev.h):
  exp(x) - 1, 2 / (1 + exp(-s)), log(sc0 sc1); in float64 both forms are the same reference.
* Teacher forcing: the forward calls store every layer's output state, a2_save and scale_save, the backward calls dparams_save, dc_save
  (and x_op_save), so ``check_forward`` / ``check_backward`` check each phase of each layer on the inputs the kernel itself stored.  A
  bf16 rounding flip is not carried forward.  The fused backward keeps its running gradient on chip: the checker carries its own
  gradient chain (float64, fed from the stored dc) TOGETHER with the error that chain can hold, propagated through the formulas.
* Bounds.  A value stored as bf16: 1 bf16 ulp of the value + b fp32 units of ``mag``; an fp32 value: b fp32 units of ``mag``
  (+ the propagated error), b = max(4 x yardstick, 4).  The unit is the fp32 ulp of ``mag``: the pre-activation's mag is sum |x w|,
  carried through the ELU (the negative branch adds |ELU| -- exp(c) + 1 in the fast form, whose subtraction cancels); the scale's mag is
  what one unit of s moves it by plus its own terms; the log-det slot's mag includes what one unit in each scale propagates,
  ulp(sc) / sc; dbias_part and post_part take the sum of their terms' magnitudes and are compared after summing the split parts.
  The yardstick is the worst error of the fp32 restatement against float64, teacher-forced, on the very operands of the GPU tests;
  test_mcf_kernels_cpu.py measures it and holds it against YARDSTICK (rounded up, not padded).
* The inverse stores no intermediate, and a flip in an early strip moves every later one: in the inexact family the forward residual is
  checked instead.  With mu, scale computed in float64 from round_T(x_rec): |scale x_rec + mu - y| within the fp32 bound plus one bf16
  unit of every hidden activation (which the call did not store) carried through |W2| (zero for f32).  Pass-through columns bit for bit.
* Exact operands (``exact_layer``, ``exact_inputs``): integer x >= 0 that differs from position to position and channel to channel;
  sparse integer W1 >= 0, so c >= 0 and the ELU is the identity; integer conditioning rows; sparse integer mu rows of W2 with an
  integer bias, all-zero s rows and bias, so scale = 1, log-det 0, y = x + mu; ActNorms with log_scale = 0 and an integer bias; even integer dy and dld (ds = (dy x + dld) / 2).
  Every value staged or stored as bf16 stays <= 2^8 in magnitude through all four or eight layers and every partial sum < 2^24
  (test_mcf_kernels_cpu.py asserts it for every case): both directions and the inverse are exact whatever the summation order or the
  exp / log / rcp flavour, and everything is compared bit for bit.
* Inexact operands: random real weights with |s| <= 4 (asserted), pre-activations of both signs including small negative ones,
  log_scale of both signs.

Recorded yardsticks (fp32 units of mag beyond the allowances above; worst over the cases of the tables below, rounded up) and the
GPU bounds max(4 x yardstick, 4); "fast" is the fused / split kernels' algebra, bf16 only:

    quantity     f32          bf16         bf16 fast        quantity     f32          bf16         bf16 fast
    a2           1.9 -> 7.6   0.0 -> 4     0.1 -> 4         dc           5.2 -> 20.8  0.1 -> 4     0.1 -> 4
    scale        1.8 -> 7.2   1.0 -> 4     1.4 -> 5.6       dx           1.8 -> 7.2   2.2 -> 8.8   0.0 -> 4
    y            2.5 -> 10    2.3 -> 9.2   2.0 -> 8         dbias        1.6 -> 6.4   2.1 -> 8.4   1.8 -> 7.2
    slot         0.2 -> 4     0.2 -> 4     0.1 -> 4         post_part    0.8 -> 4     0.8 -> 4     0.9 -> 4
    dp_mu        1.3 -> 5.2   0.0 -> 4     0.0 -> 4         inv          3.0 -> 12    1.6 -> 6.4   2.3 -> 9.2
    dp_s         2.6 -> 10.4  0.0 -> 4     0.0 -> 4

Worst error measured on the MI355X over the same cases (same units; bound in the table above):

    f32        a2 4.53  scale 1.80  y 3.69  slot 0.22  dp_mu 1.27  dp_s 1.91  dc 6.01  dx 3.05  dbias 3.44  post_part 0.62  inv 3.10
    bf16       a2 0.00  scale 0.97  y 1.35  slot 0.16  dp_mu 0.00  dp_s 0.00  dc 0.00  dx 1.96  dbias 2.86  post_part 0.70  inv 1.51
    bf16 fast  a2 0.14  scale 1.08  y 1.37  slot 0.17  dp_mu 0.00  dp_s 0.00  dc 0.03  dx 0.00  dbias 2.10  post_part 0.79  inv 2.23

(Measured on one CPU thread, the worst value observed being recorded.  The fused backward keeps its gradient on chip, so the "bf16
fast" entries dp_mu, dp_s, dbias, post_part and dx are measured BEYOND the error the checker's own gradient chain may hold: that
allowance starts at zero at the last layer and grows by the dx bound -- 4 fp32 units of dx's mag -- with every layer passed; the 0.0 of
dx there means "inside that allowance", not "exact".  inv is the forward residual in fp32 units of the mag of scale x + mu, beyond one
bf16 unit of every hidden activation carried through |W2| into mu and, times |x| (1 - t^2) / 2, into the scale -- nothing in f32.  The
fused inverse stores no state between its four layers: in the inexact family it is run with ONE real layer at a time, the other three
being ``identity_layer``s, which it inverts bit for bit, so that the residual of that layer -- behind the inverse of its ActNorm -- is
the launch's whole error.)
"""
import collections

import torch

from ipoke_amd import ops
from tests.flow_exact import F64, assert_same, f32r, randint64, ulp_of
from tests.helpers import frag_tile, shadow_nt, shadow_t

F32 = torch.float32
BF16 = torch.bfloat16
TDT = {"f32": F32, "bf16": BF16}

# (kh, kw, oy, ox) of orders A..D: input (y + ky + oy, x + kx + ox) feeds output (y, x) -- strictly above / below / left / right
OFFSETS = {0: (2, 3, -2, -1), 1: (2, 3, +1, -1), 2: (3, 2, -1, -2), 3: (3, 2, -1, +1)}

# worst error of the restatement against float64 in units (test_mcf_kernels_cpu.py measures and asserts them); form "fast" is the
# algebra of the fused / split kernels (bf16 only), the others the libm-grade per-layer kernels
YARDSTICK = {
    "a2_f32": 1.9, "a2_bf16": 0.0, "a2_bf16_fast": 0.1,
    "scale_f32": 1.8, "scale_bf16": 1.0, "scale_bf16_fast": 1.4,
    "y_f32": 2.5, "y_bf16": 2.3, "y_bf16_fast": 2.0,
    "slot_f32": 0.2, "slot_bf16": 0.2, "slot_bf16_fast": 0.1,
    "dp_mu_f32": 1.3, "dp_mu_bf16": 0.0, "dp_mu_bf16_fast": 0.0,
    "dp_s_f32": 2.6, "dp_s_bf16": 0.0, "dp_s_bf16_fast": 0.0,
    "dc_f32": 5.2, "dc_bf16": 0.1, "dc_bf16_fast": 0.1,
    "dx_f32": 1.8, "dx_bf16": 2.2, "dx_bf16_fast": 0.0,
    "dbias_f32": 1.6, "dbias_bf16": 2.1, "dbias_bf16_fast": 1.8,
    "post_part_f32": 0.8, "post_part_bf16": 0.8, "post_part_bf16_fast": 0.9,
    "inv_f32": 3.0, "inv_bf16": 1.6, "inv_bf16_fast": 2.3,
}
STORED_T = ("a2", "dp_mu", "dp_s", "dc")            # stored in the compute type; everything else is fp32


def ykey(name, dt, fast):
    return f"{name}_{dt}" + ("_fast" if fast else "")


def gpu_bound(name, dt, fast):
    """fp32 units of mag allowed on the device: max(4 x yardstick, 4)"""
    return max(4.0 * YARDSTICK[ykey(name, dt, fast)], 4.0)


def rnd(v, tdt):
    """the values of v rounded as the kernels round: to fp32, then to the storage type; dtype kept"""
    return v if tdt is None else v.to(F32).to(tdt).to(v.dtype)


# ------------------------------------------------------------------ cases
class Layer(collections.namedtuple("Layer", "order W1 W2 b2 ls pb")):
    """order 0..3; W1 [4C][C][kh][kw]; W2 [2C][4C + Cc] (rows [mu | s], columns [hidden | cond]); b2 [2C]; ls / pb [C] or None: the
    ActNorm behind the layer.  float64 holding values of the case's type (W1, W2) / fp32 values (b2, ls, pb)."""


class LCase(collections.namedtuple("LCase", "dt order C ld Cc rpb post B")):
    """a per-layer call: ipoke_mcf_fwd / _bwd / _inv"""
    @property
    def id(self):
        gen = "-general" if self.dt == "bf16" and 4 * self.C + self.Cc > 384 else ""
        return f"{self.dt}-{'ABCD'[self.order]}-C{self.C}ld{self.ld}-Cc{self.Cc}-rpb{self.rpb}{'-actnorm' if self.post else ''}-B{self.B}{gen}"

    @property
    def slot_w(self):
        """log-det slots per sample of the per-layer forward call: 64 / rows per workgroup (default 32 in bf16, 16 in f32)"""
        return 64 // (self.rpb or (32 if self.dt == "bf16" else 16))


# each axis once: orders, dtypes, C (scalar paths at C % 4 != 0, 16-byte paths, narrow and wide), ld (== C, C + 4, 64), Cc (the
# minimum, 64, 128, 256 -- 256 at C = 64 in bf16 is the general path), rows_per_block, the fused ActNorm, B
LAYER_CASES = [
    LCase("bf16", 0, 64, 64, 128, 16, True, 3),
    LCase("bf16", 1, 64, 64, 256, 0, False, 3),
    LCase("bf16", 2, 64, 64, 256, 64, True, 5),
    LCase("bf16", 3, 64, 64, 256, 16, False, 2),
    LCase("bf16", 2, 60, 64, 64, 32, True, 1),
    LCase("bf16", 3, 32, 36, 8, 64, True, 5),
    LCase("bf16", 0, 30, 34, 128, 0, False, 2),
    LCase("bf16", 1, 8, 64, 64, 16, True, 3),
    LCase("bf16", 2, 6, 6, 8, 32, False, 5),
    LCase("bf16", 3, 2, 6, 8, 64, False, 1),
    LCase("f32", 0, 64, 64, 128, 64, True, 3),
    LCase("f32", 1, 60, 64, 256, 32, True, 1),
    LCase("f32", 2, 32, 32, 4, 0, False, 5),
    LCase("f32", 3, 30, 64, 64, 64, False, 2),
    LCase("f32", 0, 8, 12, 128, 16, True, 3),
    LCase("f32", 1, 6, 10, 4, 16, False, 3),
    LCase("f32", 3, 2, 2, 64, 0, False, 5),
]


class UCase(collections.namedtuple("UCase", "C ld Cc B nl")):
    """a fused launch: ipoke_macow_unit_* (nl = 4) / ipoke_macow_unit2_* (nl = 8); bf16"""
    dt = "bf16"

    @property
    def id(self):
        return f"C{self.C}ld{self.ld}-Cc{self.Cc}-B{self.B}" + ("-two-units" if self.nl == 8 else "")


UNIT_CASES = [UCase(8, 8, 8, 2, 4), UCase(30, 32, 32, 3, 4), UCase(32, 64, 128, 1, 4), UCase(60, 64, 32, 5, 4), UCase(64, 64, 128, 3, 4)]
UNIT2_CASES = [UCase(8, 12, 32, 3, 8), UCase(64, 64, 128, 2, 8)]
UNIT_ORDERS = (0, 1, 2, 3)
UNIT_POST = (False, True, False, True)


# ------------------------------------------------------------------ phase references
def _shifted(xm, dy, dx):
    """xm [B][8][8][C] -> s[b, y, x] = xm[b, y + dy, x + dx], zero outside the map"""
    out = torch.zeros_like(xm)
    y0, y1, x0, x1 = max(0, -dy), min(8, 8 - dy), max(0, -dx), min(8, 8 - dx)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = xm[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def shiftconv_ref(x, W1, order, moved=None):
    """c[p][n] = sum over taps and channels of W1[n][ch][ky][kx] x[(y + ky + oy, x + kx + ox)][ch] -> (c, mag).
    moved = (tap, dy, dx): that tap's offset moved (the mutation check)"""
    kh, kw, oy, ox = OFFSETS[order]
    M, C = x.shape
    xm = x.reshape(-1, 8, 8, C)
    c = torch.zeros(M, W1.shape[0], dtype=x.dtype)
    mag = torch.zeros_like(c)
    for ky in range(kh):
        for kx in range(kw):
            dy, dx = ky + oy, kx + ox
            if moved is not None and moved[0] == ky * kw + kx:
                dy, dx = dy + moved[1], dx + moved[2]
            s = _shifted(xm, dy, dx).reshape(M, C)
            w = W1[:, :, ky, kx]
            c = c + s @ w.t()
            mag = mag + s.abs() @ w.abs().t()
    return c, mag


def shiftconv_adj_ref(dc, W1, order):
    """the adjoint of shiftconv_ref: out[q][ch] = sum over taps and n of dc[q - off(tap)][n] W1[n][ch][tap] -> (value, mag)"""
    kh, kw, oy, ox = OFFSETS[order]
    M, H = dc.shape
    dm = dc.reshape(-1, 8, 8, H)
    out = torch.zeros(M, W1.shape[1], dtype=dc.dtype)
    mag = torch.zeros_like(out)
    for ky in range(kh):
        for kx in range(kw):
            s = _shifted(dm, -(ky + oy), -(kx + ox)).reshape(M, H)
            w = W1[:, :, ky, kx]
            out = out + s @ w
            mag = mag + s.abs() @ w.abs()
    return out, mag


def hidden_ref(c, cmag, fast=False):
    """ELU(c) -> (a, mag): libm form expm1(c), fast form exp(c) - 1 (whose terms exp(c) and 1 cancel for small |c|)"""
    neg = c <= 0
    e = torch.exp(c.clamp(max=0.0))
    a = torch.where(neg, e - 1.0 if fast else torch.expm1(c.clamp(max=0.0)), c)
    return a, torch.where(neg, cmag + (e + 1.0 if fast else a.abs()), cmag)


def elu_grad_from_out(a):
    """ELU' from the stored output: 1 where a > 0, a + 1 elsewhere"""
    return torch.where(a > 0, torch.ones_like(a), a + 1.0)


def params_ref(a2, W2, b2):
    """(mu, s) = W2 a2 + bias2 -> (mu, s, mag_mu, mag_s)"""
    C = W2.shape[0] // 2
    p = a2 @ W2.t() + b2
    m = a2.abs() @ W2.abs().t() + b2.abs()
    return p[:, :C], p[:, C:], m[:, :C], m[:, C:]


def scale_ref(s, smag, fast=False):
    """scale = tanh(s / 2) + 1 (fast: 2 / (1 + exp(-s))) -> (scale, mag): one unit of s moves it by (1 - t^2) / 2, its own terms are
    |t| + 1"""
    t = torch.tanh(0.5 * s)
    sc = 2.0 / (1.0 + torch.exp(-s)) if fast else t + 1.0
    return sc, smag * 0.5 * (1.0 - t * t) + t.abs() + 1.0


def coupling_ref(x, mu, mumag, scale):
    """y = scale x + mu -> (y, mag)"""
    return scale * x + mu, (scale * x).abs() + mumag


def logdet_rows_ref(scale, fast=False):
    """per-row log-det terms -> (sum over the channels [M], mag [M]); fast: log(sc0 sc1) of adjacent channels.  mag includes what one
    unit in each scale propagates: ulp(sc) / sc, in units of 2^-23"""
    lg = torch.log(scale[:, 0::2] * scale[:, 1::2]) if fast else torch.log(scale)
    own = torch.log(scale.to(F64)).abs() + ulp_of(scale.to(F64), F32) / scale.to(F64) * 2.0 ** 23
    return lg.sum(1), own.sum(1)


def post_actnorm_ref(y, ymag, ls, pb):
    """the fused ActNorm: y exp(ls) + b -> (value, mag)"""
    e = torch.exp(ls)
    return y * e + pb, ymag * e + pb.abs()


def dparams_ref(g, x, scale, dld_rows, ls=None):
    """[dy' | ds]: dy' = g exp(ls) behind a fused ActNorm, ds = (dy' x + dld / scale) (1 - (scale - 1)^2) / 2
    -> (dy', ds, mag_dy', mag_ds, d ds / d dy')"""
    gy = g if ls is None else g * torch.exp(ls)
    t = scale - 1.0
    q = dld_rows.view(-1, 1) / scale
    k = 0.5 * (1.0 - t * t)
    return gy, (gy * x + q) * k, gy.abs(), ((gy * x).abs() + q.abs()) * 0.5 * (1.0 + t * t), (x * k).abs()


def dc_ref(dp, W2, a_hidden):
    """(dparams W2[:, :H]) ELU'(stored a) -> (dc, mag)"""
    H = a_hidden.shape[1]
    d = elu_grad_from_out(a_hidden)
    return (dp @ W2[:, :H]) * d, (dp.abs() @ W2[:, :H].abs()) * d.abs()


def dx_ref(gy, scale, dc, W1, order):
    """dy' scale + the adjoint shifted convolution of dc -> (dx, mag)"""
    v, m = shiftconv_adj_ref(dc, W1, order)
    return gy * scale + v, (gy * scale).abs() + m


def per_sample(v, B, parts=1):
    """sums over the rows of each of `parts` row slices of every sample: [M][n] -> [B * parts][n]"""
    return v.reshape(B * parts, 64 // parts, -1).sum(1)


def dbias_ref(gy, ds, B, parts=1):
    """column sums of [dy' | ds] per sample -> (value, mag)"""
    v = torch.cat([gy, ds], 1)
    return per_sample(v, B, parts), per_sample(v.abs(), B, parts)


def post_part_ref(g, y_post, pb, dld, B):
    """[d_log_scale | d_bias] of the fused ActNorm per sample: sum g (y_post - b) + 64 dld, sum g -> (value, mag)"""
    t = g * (y_post - pb)
    v = torch.cat([per_sample(t, B) + 64.0 * dld.view(-1, 1), per_sample(g, B)], 1)
    m = torch.cat([per_sample(g.abs() * (y_post.abs() + pb.abs()), B) + 64.0 * dld.abs().view(-1, 1), per_sample(g.abs(), B)], 1)
    return v, m


def layer_params(x, L, cond, tdt=None, fast=False):
    """(mu, scale, mag_mu, a_hidden) of a whole layer from its input state, rounded where the kernels stage"""
    c, cm = shiftconv_ref(rnd(x, tdt), L.W1, L.order)
    a = rnd(hidden_ref(c, cm, fast)[0], tdt)
    mu, s, mm, sm = params_ref(torch.cat([a, cond], 1), L.W2, L.b2)
    return mu, scale_ref(s, sm, fast)[0], mm, a


def strip_rows(order, step, B):
    """row indices [B * 8] of the strip the inverse reconstructs at `step`: rows (A, B) or columns (C, D) of the map, B and D backwards"""
    i = 7 - step if order & 1 else step
    j = torch.arange(8)
    pos = i * 8 + j if order < 2 else j * 8 + i
    return (torch.arange(B).view(-1, 1) * 64 + pos.view(1, -1)).reshape(-1)


def inverse_layer(y, L, cond, tdt=None, fast=False):
    """x = (y - mu) / (scale + 1e-12) strip by strip: the conditioner of a strip sees the strips reconstructed before it"""
    x = torch.zeros_like(y)
    B = y.shape[0] // 64
    for step in range(8):
        mu, sc, _, _ = layer_params(x, L, cond, tdt, fast)
        r = strip_rows(L.order, step, B)
        x[r] = (y[r] - mu[r]) / (sc[r] + 1e-12)
    return x


# ------------------------------------------------------------------ the chain
def chain(layers, x, cond, dy=None, dld=None, tdt=None, cdt=F64, fast=False, inverse_of=None):
    """Four or eight layers (any number) chained on the first C columns of x.  tdt None: float64, no rounding (the unforced reference).
    tdt a storage type with cdt = float32: the restatement.  Returns a workspace dict of per-layer lists: x (input state), y (output
    state, behind the ActNorm), a2, scale, ld_rows (log-det per row), c and s (the pre-activations); with dy / dld also dp (= [dy' | ds] rounded), dc, dbias [B][2C],
    post_part [B][2C] or None, g (incoming gradient of the layer), and dx; with inverse_of (an output state) x_rec."""
    q = lambda v: rnd(v, tdt)                                                                 # noqa: E731
    cv = lambda v: None if v is None else v.to(cdt)                                           # noqa: E731
    layers = [Layer(L.order, cv(L.W1), cv(L.W2), cv(L.b2), cv(L.ls), cv(L.pb)) for L in layers]
    cond = cond.to(cdt)
    B = x.shape[0] // 64
    C = layers[0].W1.shape[1]
    ws = {k: [] for k in ("x", "y", "a2", "scale", "ld_rows", "c", "s")}
    cur = x[:, :C].to(cdt)
    for L in layers:
        c, cm = shiftconv_ref(q(cur), L.W1, L.order)
        a2 = torch.cat([q(hidden_ref(c, cm, fast)[0]), cond], 1)
        mu, s, mm, sm = params_ref(a2, L.W2, L.b2)
        sc = scale_ref(s, sm, fast)[0]
        y, ym = coupling_ref(cur, mu, mm, sc)
        if L.ls is not None:
            y = post_actnorm_ref(y, ym, L.ls, L.pb)[0]
        for k, v in (("x", cur), ("y", y), ("a2", a2), ("scale", sc), ("ld_rows", logdet_rows_ref(sc, fast)[0]), ("c", c), ("s", s)):
            ws[k].append(v)
        cur = y
    if dy is not None:
        n = len(layers)
        for k in ("dp", "dc", "dbias", "post_part", "g"):
            ws[k] = [None] * n
        g, dld = dy[:, :C].to(cdt), dld.to(cdt)
        rows = dld.repeat_interleave(64)
        for k in range(n - 1, -1, -1):
            L = layers[k]
            ws["g"][k] = g
            if L.ls is not None:
                ws["post_part"][k] = post_part_ref(g, ws["y"][k], L.pb, dld, B)[0]
            gy, ds = dparams_ref(g, ws["x"][k], ws["scale"][k], rows, L.ls)[:2]
            ws["dbias"][k] = dbias_ref(gy, ds, B)[0]
            dp = q(torch.cat([gy, ds], 1))
            H = L.W1.shape[0]
            dc = q(dc_ref(dp, L.W2, ws["a2"][k][:, :H])[0])
            ws["dp"][k], ws["dc"][k] = dp, dc
            g = dx_ref(gy, ws["scale"][k], dc, L.W1, L.order)[0]
        ws["dx"] = g
    if inverse_of is not None:
        cur = inverse_of[:, :C].to(cdt)
        for L in reversed(layers):
            if L.ls is not None:
                cur = (cur - L.pb) / (torch.exp(L.ls) + 1e-8)
            cur = inverse_layer(cur, L, cond, tdt, fast)
        ws["x_rec"] = cur
    return ws


# ------------------------------------------------------------------ operands
def exact_layer(C, Cc, order, k=0, classes=1, post=False):
    """Integer weights.  Hidden unit n reads ONE channel through tap n % 6 with weight 1 and every third one a second channel through
    another tap; the mu row of channel c reads hidden columns (four of them, all 4C columns together, when classes == 1; one when the
    layer belongs to a chain) and two conditioning columns with weight 1.  classes = 4 (chains): layer k reads and updates only the
    channels c % 4 == k % 4 (mu = 0 for the others), which bounds the growth over eight layers by 3 x per update, two updates per
    channel."""
    kh, kw = OFFSETS[order][:2]
    H, K2 = 4 * C, 4 * C + Cc
    own = [c for c in range(C) if classes == 1 or c % classes == k % classes]
    W1 = torch.zeros(H, C, kh, kw, dtype=F64)
    for n in range(H):
        t = n % 6
        W1[n, own[(n // 6 + n) % len(own)], t // kw, t % kw] += 1.0
        if n % 3 == 0:
            t = (n + 3 + n // 6) % 6
            W1[n, own[(n // 2 + 1) % len(own)], t // kw, t % kw] += 1.0
    W2 = torch.zeros(2 * C, K2, dtype=F64)
    b2 = torch.zeros(2 * C, dtype=F64)
    for c in own:
        for j in (range(4) if classes == 1 else ((c + k) % 4,)):
            W2[c, j * C + (c * 3 + j) % C] += 1.0
        W2[c, H + (c * 3 + k) % Cc] += 1.0
        W2[c, H + (c * 5 + Cc // 2 + 1) % Cc] += 1.0
        b2[c] = (c * 7 + k) % 4
    ls = torch.zeros(C, dtype=F64) if post else None
    pb = ((torch.arange(C) * 3 + k) % 3).to(F64) if post else None
    return Layer(order, W1, W2, b2, ls, pb)


def exact_inputs(C, ld, Cc, B, top):
    """x [M][ld] integers in [0, top], a fixed table without any period over positions, channels or samples (a linear code modulo
    top + 1 would repeat every few channels and hide a channel offset of that period); cond [M][Cc] in [0, 3]; dy [M][ld] in
    {-2, 0, 2}; dld [B] in {-2, 0, 2}"""
    M = B * 64
    gen = torch.Generator().manual_seed(10000 * C + 100 * ld + B)
    x = randint64(0, top, (M, ld), gen)
    cond = randint64(0, 3, (M, Cc), gen)
    dy = 2.0 * randint64(-1, 1, (M, ld), gen)
    dld = 2.0 * ((torch.arange(B) + 1) % 3 - 1).to(F64)
    return x, cond, dy, dld


def inexact_layer(C, Cc, order, gen, tdt, post, k=0):
    kh, kw = OFFSETS[order][:2]
    H, K2 = 4 * C, 4 * C + Cc
    W1 = rnd(torch.randn(H, C, kh, kw, generator=gen, dtype=F64) * (0.9 / (6 * C) ** 0.5), tdt)
    W2 = torch.randn(2 * C, K2, generator=gen, dtype=F64) / K2 ** 0.5
    W2 *= 0.7 / (1.0 + 0.15 * k)             # (the state grows along a chain: later layers take smaller weights, so |s| stays <= 4)
    b2 = f32r(torch.randn(2 * C, generator=gen, dtype=F64) * 0.2)
    ls = pb = None
    if post:
        sign = torch.where(torch.arange(C) % 3 == 0, 1.0, -1.0).to(F64)
        ls = f32r(sign * (0.05 + 0.25 * torch.rand(C, generator=gen, dtype=F64)))
        pb = f32r(torch.randn(C, generator=gen, dtype=F64) * 0.3)
    return Layer(order, W1, rnd(W2, tdt), b2, ls, pb)


def inexact_inputs(C, ld, Cc, B, gen, tdt):
    M = B * 64
    x = f32r(torch.randn(M, ld, generator=gen, dtype=F64))
    h = torch.randn(M, Cc, generator=gen, dtype=F64)
    cond = rnd(torch.where(h > 0, h, torch.expm1(h)), tdt)                 # the prepared rows: ELU(h) in the compute type
    dy = f32r(torch.randn(M, ld, generator=gen, dtype=F64))
    dld = f32r(torch.randn(B, generator=gen, dtype=F64))
    return x, cond, dy, dld


def layer_operands(c, exact):
    """operands of a per-layer case: ([layer], x, cond, dy, dld)"""
    if exact:
        return ([exact_layer(c.C, c.Cc, c.order, post=c.post)],) + exact_inputs(c.C, c.ld, c.Cc, c.B, 7)
    gen = torch.Generator().manual_seed(1000 * c.C + 10 * c.Cc + c.order + 7 * c.B)
    tdt = TDT[c.dt]
    return ([inexact_layer(c.C, c.Cc, c.order, gen, tdt, c.post)],) + inexact_inputs(c.C, c.ld, c.Cc, c.B, gen, tdt)


def unit_operands(c, exact):
    """operands of a fused case: (4 or 8 layers A B(+ActNorm) C D(+ActNorm) [x 2], x, cond, dy, dld)"""
    if exact:
        ls = [exact_layer(c.C, c.Cc, UNIT_ORDERS[k % 4], k, 4, UNIT_POST[k % 4]) for k in range(c.nl)]
        return (ls,) + exact_inputs(c.C, c.ld, c.Cc, c.B, 3)
    gen = torch.Generator().manual_seed(77 * c.C + c.Cc + c.B)
    ls = [inexact_layer(c.C, c.Cc, UNIT_ORDERS[k % 4], gen, BF16, UNIT_POST[k % 4], k) for k in range(c.nl)]
    return (ls,) + inexact_inputs(c.C, c.ld, c.Cc, c.B, gen, BF16)


def shadows(L, C, Cc, dt, device):
    """the fragment-tiled weight operands of one layer, built directly from its effective matrices (no weight norm in between)"""
    d = ops.mcf_dims(C, Cc, dt)
    H = 4 * C
    w1 = L.W1.to(F32).to(device)
    v = L.W2.to(F32).to(device).reshape(2 * C, H + Cc, 1, 1)
    W2T = torch.zeros(d["Hr"], d["K3p"], device=device)
    W2T[:H, :2 * C] = L.W2[:, :H].to(F32).to(device).t()
    tdt = TDT[dt]
    sh = dict(W1=frag_tile(shadow_nt(w1, d["Cp"], d["Hr"], d["K1p"], dt)), W1T=frag_tile(shadow_t(w1, d["Hq"], d["Cr"], dt)),
              W2=frag_tile(shadow_nt(v, d["K2p"], d["N2r"], d["K2p"], dt)), W2T=frag_tile(W2T.to(tdt).contiguous()),
              bias=L.b2.to(F32).to(device).contiguous(), dims=d)
    if L.ls is not None:
        sh["ls"], sh["pb"] = L.ls.to(F32).to(device).contiguous(), L.pb.to(F32).to(device).contiguous()
    return sh


# ------------------------------------------------------------------ teacher-forced checkers
class Tally:
    """collects the worst error per quantity in fp32 units of mag (beyond the bf16 ulp of a value stored as bf16 and the propagated
    error); with enforce a miss raises at once, naming the worst element"""
    def __init__(self, dt, fast, enforce=True):
        self.dt, self.fast, self.enforce, self.worst = dt, fast, enforce, {}

    def cmp(self, name, got, ref, mag, prop=None, where=""):
        ref, mag = ref.to(F64), mag.to(F64)
        err = (got.to(F64) - ref).abs()
        if prop is not None:
            err = err - prop.to(F64)
        if name in STORED_T and self.dt == "bf16":
            err = err - ulp_of(ref, BF16)
        e = err.clamp(min=0.0) / ulp_of(mag, F32)
        w = float(e.max()) if e.numel() else 0.0
        self.worst[name] = max(self.worst.get(name, 0.0), w)
        if self.enforce:
            bound = gpu_bound(name, self.dt, self.fast)
            bad = ~(e <= bound)
            if bool(bad.any()):
                i = int(torch.argmax(torch.nan_to_num(e, nan=float("inf")).reshape(-1)))
                row, col = divmod(i, e.shape[-1]) if e.dim() > 1 else (i, 0)
                raise AssertionError(
                    f"{name} {where}: {int(bad.sum())} elements beyond {bound} units; worst {w:.2f} at row {row} (sample {row // 64}, position "
                    f"{row % 64}), column {col}: got {float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}, mag "
                    f"{float(mag.reshape(-1)[i])!r}")


def check_forward(layers, cond, ws, tally, slot_parts=None):
    """every phase of every layer on what the call stored: ws = {x: [layer inputs, fp32 values], y, a2, scale: per layer as stored,
    slots: per layer [B][parts] or absent}.  slot_parts: row slices per sample a slot covers (slots[k][:, s] = rows of slice s)."""
    tdt, fast = TDT[tally.dt], tally.fast
    for k, L in enumerate(layers):
        at = f"(layer {k})"
        H, C = L.W1.shape[0], L.W1.shape[1]
        x, a2, sc = ws["x"][k].to(F64), ws["a2"][k].to(F64), ws["scale"][k].to(F64)
        c, cm = shiftconv_ref(rnd(x, tdt), L.W1, L.order)
        tally.cmp("a2", ws["a2"][k][:, :H], *hidden_ref(c, cm, fast), where=at)
        assert_same(ws["a2"][k][:, H:H + cond.shape[1]].contiguous(), cond.to(ws["a2"][k].dtype), f"conditioning columns of a2 {at}")
        assert bool((a2[:, H + cond.shape[1]:] == 0).all()), f"padding columns of a2 {at}"
        mu, s, mm, sm = params_ref(a2[:, :H + cond.shape[1]], L.W2, L.b2)
        tally.cmp("scale", ws["scale"][k], *scale_ref(s, sm, fast), where=at)
        y, ym = coupling_ref(x, mu, mm, sc)
        if L.ls is not None:
            y, ym = post_actnorm_ref(y, ym, L.ls, L.pb)
        tally.cmp("y", ws["y"][k], y, ym, where=at)
        if ws.get("slots") is not None:
            parts = slot_parts or 1
            B = x.shape[0] // 64
            v, m = logdet_rows_ref(sc, fast)
            tally.cmp("slot", ws["slots"][k], per_sample(v, B, parts).reshape(B, parts), per_sample(m, B, parts).reshape(B, parts), where=at)


def check_backward(layers, ws, dy, dld, tally, parts=1):
    """d params, d c, the partial sums and d x of every layer, last layer first, on what the calls stored: ws = {x, y, a2, scale (from
    the forward call), dp, dc, dbias ([B * parts][2C]), post_part, dx}.  The gradient between the layers is the checker's own."""
    tdt, dt, fast = TDT[tally.dt], tally.dt, tally.fast
    B = dld.shape[0]
    rows = dld.repeat_interleave(64)
    g, eg = dy.to(F64), torch.zeros_like(dy, dtype=F64)
    for k in range(len(layers) - 1, -1, -1):
        L, at = layers[k], f"(layer {k})"
        H, C = L.W1.shape[0], L.W1.shape[1]
        x, a2, sc = ws["x"][k].to(F64), ws["a2"][k].to(F64), ws["scale"][k].to(F64)
        if L.ls is not None:
            v, m = post_part_ref(g, ws["y"][k].to(F64), L.pb, dld, B)
            prop = torch.cat([per_sample(eg * (ws["y"][k].to(F64) - L.pb).abs(), B), per_sample(eg, B)], 1)
            tally.cmp("post_part", ws["post_part"][k].to(F64).reshape(B, parts, -1).sum(1), v, m, prop, where=at)
        gy, ds, mg, md, dsdg = dparams_ref(g, x, sc, rows, L.ls)
        egy = eg if L.ls is None else eg * torch.exp(L.ls)
        dp = ws["dp"][k]
        tally.cmp("dp_mu", dp[:, :C], gy, mg, egy, where=at)
        tally.cmp("dp_s", dp[:, C:2 * C], ds, md, egy * dsdg, where=at)
        assert bool((dp[:, 2 * C:].to(F64) == 0).all()), f"padding columns of dparams_save {at}"
        v, m = dbias_ref(gy, ds, B)
        prop = per_sample(torch.cat([egy, egy * dsdg], 1), B)
        tally.cmp("dbias", ws["dbias"][k].to(F64).reshape(B, parts, -1).sum(1), v, m, prop, where=at)
        dc = ws["dc"][k]
        tally.cmp("dc", dc[:, :H], *dc_ref(dp.to(F64)[:, :2 * C], L.W2, a2[:, :H]), where=at)
        assert bool((dc[:, H:].to(F64) == 0).all()), f"padding columns of dc_save {at}"
        g, m = dx_ref(gy, sc, dc.to(F64)[:, :H], L.W1, L.order)
        eg = egy * sc
        if k == 0:
            tally.cmp("dx", ws["dx"], g, m, eg)
        else:                                   # the kernel's own running gradient may sit anywhere within its bound
            eg = eg + gpu_bound("dx", dt, fast) * ulp_of(m, F32)


def check_inverse_residual(L, cond, y, x_rec, tally, where=""):
    """one layer's inverse (behind the inverse of its ActNorm, if it has one) by its forward residual: mu, scale in float64 from
    round_T(x_rec); |(scale x_rec + mu) exp(ls) + b - y| within the fp32 bound plus one bf16 unit of every hidden activation carried
    through |W2| (none in f32)"""
    tdt = TDT[tally.dt]
    C = L.W1.shape[1]
    xr = x_rec.to(F64)
    c, cm = shiftconv_ref(rnd(xr, tdt), L.W1, L.order)
    a = hidden_ref(c, cm, tally.fast)[0]
    mu, s, mm, sm = params_ref(torch.cat([a, cond], 1), L.W2, L.b2)
    sc = scale_ref(s, sm, tally.fast)[0]
    ea = ulp_of(a, BF16) if tdt == BF16 else torch.zeros_like(a)
    H = a.shape[1]
    emu, es = ea @ L.W2[:C, :H].abs().t(), ea @ L.W2[C:, :H].abs().t()
    t = sc - 1.0
    prop = emu + xr.abs() * es * 0.5 * (1.0 - t * t)
    yy, ym = coupling_ref(xr, mu, mm, sc)
    if L.ls is not None:
        yy, ym = post_actnorm_ref(yy, ym, L.ls, L.pb)
        prop = prop * torch.exp(L.ls)
    tally.cmp("inv", y.to(F64), yy, ym, prop, where=where)


def identity_layer(C, Cc, order):
    """all-zero weights: mu = 0, s = 0, scale = 1 exactly in either algebra -- the layer and its inverse copy the state bit for bit"""
    kh, kw = OFFSETS[order][:2]
    return Layer(order, torch.zeros(4 * C, C, kh, kw, dtype=F64), torch.zeros(2 * C, 4 * C + Cc, dtype=F64), torch.zeros(2 * C, dtype=F64),
                 None, None)


def as_stored(ws, dt, B, slot_parts=1):
    """a chain's workspace in the types the calls store it in: a2 / dp / dc in the compute type, everything else fp32, the log-det of
    every layer as slots [B][slot_parts]"""
    tdt = TDT[dt]
    out = {}
    for k, v in ws.items():
        if k in ("a2", "dp", "dc"):
            out[k] = [t.to(F32).to(tdt) for t in v]
        elif isinstance(v, list):
            out[k] = [None if t is None else t.to(F32) for t in v]
        else:
            out[k] = v.to(F32)
    out["slots"] = [per_sample(t.to(F32).view(-1, 1), B, slot_parts).reshape(B, slot_parts) for t in ws["ld_rows"]]
    return out
