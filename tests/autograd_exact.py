"""Bit-exact checking of the differentiable convolution op (ipoke_amd/autograd_ops.py: ``_ConvFn``, ``_StemFn``, ``conv_weight``, ``conv``,
``effective_weight``) and of its inference twin ``first_stage._Conv.run``: the HOST layer that decides with which geometry the kernels of
tests/conv_exact.py are called -- which operand, which taps, which parity class, which output padding, which roles in the weight
gradient, how many slabs.

Everything in that layer is linear apart from ReLU.  With small integer x, w, bias and dy every product and every partial sum of the
four results (y, dX, dW, dbias) is exact in fp32 in any order, split or slab reduction, so they are compared with ``==`` against float64
autograd through ``torch.nn.functional.conv3d`` / ``conv_transpose3d`` on the CPU (2-D modules as depth 1): fp32 results equal, results
stored in the compute dtype equal to ``conv_exact.to_bf16_rne(expected)``, the padding columns of every channels-last result zero, every
element compared.  The generator computes from the float64 reference itself the sum of magnitudes behind every element of every result
and asserts it below 2^24 units of the result's quantum; it never clips.

Spectral norm, exact: ``ipoke_spectral_sigma`` without iteration computes sigma = sum_r u[r] (W v)[r].  With u = e_i, v = e_j and
mat(W)[i][j] = 2, 4 or 8 (``_matrix_geometry``'s view; for ConvTranspose storage the transposed one) sigma and 1 / sigma are powers of two,
W / sigma has a quantum of 1 / sigma, and the backward (G - <G, W / sigma> u v^T) / sigma (sn_bwd_dot_kernel / sn_bwd_apply_kernel: fmaf
sums of integers, two products with 1 / sigma) is exact.  The frame-batched form scales the accumulators of frame t by 1 / sigma_t in the
epilogue and rowscale_bwd_kernel forms g = dy act'(y) / sigma_t, <g, y - b> and the column sums: exact on such operands as long as the
saved y is the exact value (asserted: |y| <= 256 quanta where it is stored in bf16); sn_bwd_frames_kernel adds one non-zero rank-1 term
per element because the frames' one-hot pairs differ.  conv_weight_operand_kernel multiplies by 1 / sigma: exact.  The float64 reference
is autograd through W / (u_t^T mat(W) v_t) applied to the images of frame group t.

Every case lists the branch labels it must take (``BranchRecorder``): a later change of a dispatch rule cannot empty a case unnoticed.

Stated limits: ELU, leaky ReLU, tanh and sigmoid are exact on no operands, and the ``_prescaled`` hand-over needs a norm behind the
convolution; both stay with the kernel-level tests (tests/test_disc_kernels_gpu.py, tests/test_sn_kernels_gpu.py,
tests/test_c4_dispatch_gpu.py).  The ReLU cases cover the wiring those activations share (which saved tensor, which pitch, which code).
"""
import types
from ctypes import byref
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from ipoke_amd import _lib, nn as K
from ipoke_amd import autograd_ops as FT
from ipoke_amd import first_stage as FS
from tests import conv_exact as X

DTYPES = ("bf16", "f32")


def dt_id(dtype):
    return _lib.BF16 if dtype == "bf16" else _lib.F32


# ====================================================================== the case table
@dataclass
class Case:
    name: str
    dims: int
    cin: int
    cout: int
    k: tuple
    stride: tuple
    pad: tuple
    ext: tuple                       # input extents (D, H, W)
    labels: tuple                    # branch labels of the training op and of _Conv.run, both dtypes unless labels_f32 is given
    transposed: bool = False
    bias: bool = False
    act: str = "none"                # "none" | "relu"
    wkind: str = "plain"             # "plain" | "sn" | "sn_frames"
    frames: int = 1                  # sn_frames: 1 = effective_weight(mod, False, frames=1), > 1 = a hand-built _SnFrames
    N: int = 2
    inp: str = "cl"                  # "cl" | "src" (fp32 image read in place) | "src_view" (the same through a permuted, non-dense view)
    out_f32: bool = False
    lim: int = None                  # operand limit where the automatic one had to be lowered
    labels_f32: tuple = None
    dtypes: tuple = DTYPES
    run: bool = True                 # _Conv.run supports the geometry (no frame tables in inference)

    def want(self, dtype):
        return tuple(sorted(self.labels_f32 if (dtype == "f32" and self.labels_f32 is not None) else self.labels))

    def odhw(self):
        if self.transposed:
            op = (0, self.pad[1], self.pad[2])
            return tuple((i - 1) * s - 2 * p + k + o for i, s, p, k, o in zip(self.ext, self.stride, self.pad, self.k, op))
        return tuple((i + 2 * p - k) // s + 1 for i, s, p, k in zip(self.ext, self.stride, self.pad, self.k))

    def census_key(self):
        return (self.dims, tuple(self.k), tuple(self.stride), tuple(self.pad), self.transposed, self.wkind != "plain", self.bias)


W1 = ("wgrad:plain", "wgrad:single")
CASES = []


def _add(name, dims, cin, cout, k, stride, pad, ext, labels, **kw):
    CASES.append(Case(name, dims, cin, cout, tuple(k), tuple(stride), tuple(pad), tuple(ext), tuple(labels), **kw))


def _s3(st):
    return "".join(str(s) for s in st)


# ---- 3 x 3 x 3 / padding 1 Conv3d at every stride pattern with a 2: the data gradient by parity classes (_dgrad_phases) ...
for _i, _st in enumerate([(2, 2, 2), (2, 2, 1), (2, 1, 2), (1, 2, 2), (2, 1, 1), (1, 2, 1), (1, 1, 2)]):
    _even = _i % 2 == 0
    _ext, _ci, _co = ((4, 6, 8), 12, 20) if _even else ((5, 9, 10), 8, 16)
    _ph = "dgrad:phases%d" % (2 ** sum(s == 2 for s in _st))
    _add(f"c3d_s{_s3(_st)}", 3, _ci, _co, (3, 3, 3), _st, (1, 1, 1), _ext, ("fwd:generic", _ph, "run:generic") + W1)
    # ... the other extents / channel counts at the three patterns the encoders ship
    if _st in ((2, 2, 2), (1, 2, 2), (2, 1, 1)):
        _ext2, _ci2, _co2 = ((5, 9, 10), 8, 16) if _even else ((4, 6, 8), 12, 20)
        _add(f"c3d_s{_s3(_st)}_b", 3, _ci2, _co2, (3, 3, 3), _st, (1, 1, 1), _ext2, ("fwd:generic", _ph, "run:generic") + W1)
    # ... and with spectral norm, which must take the generic launch with a computed output padding
    _o = Case("", 3, 1, 1, (3, 3, 3), _st, (1, 1, 1), _ext, ()).odhw()
    _op = tuple(i - ((o - 1) * s - 2 + 3) for i, o, s in zip(_ext, _o, _st))
    _add(f"c3d_s{_s3(_st)}_sn", 3, _ci, _co, (3, 3, 3), _st, (1, 1, 1), _ext,
         ("fwd:generic", "dgrad:ct_outpad(%d,%d,%d)" % _op, "run:generic") + W1, wkind="sn")
# an extent of 1 along strided dimensions: the odd parity classes along depth are empty; in inference the depth-1 input takes _mid_operand
_add("c3d_s222_depth1", 3, 12, 20, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 6, 7), ("fwd:generic", "dgrad:phases8", "dgrad:empty_class", "run:mid") + W1)
_add("c3d_s122_depth1", 3, 8, 16, (3, 3, 3), (1, 2, 2), (1, 1, 1), (1, 5, 8), ("fwd:generic", "dgrad:phases4", "run:mid") + W1)
# ---- other Conv3d cases
_add("c3d_1x1_s2_even", 3, 12, 20, (1, 1, 1), (2, 2, 2), (0, 0, 0), (4, 6, 8), ("fwd:generic", "dgrad:ct_outpad(1,1,1)", "run:generic") + W1)
_add("c3d_1x1_s2_odd", 3, 8, 16, (1, 1, 1), (2, 2, 2), (0, 0, 0), (5, 9, 7), ("fwd:generic", "dgrad:ct_outpad(0,0,0)", "run:generic") + W1)
_add("c3d_1x1_s122", 3, 8, 16, (1, 1, 1), (1, 2, 2), (0, 0, 0), (3, 6, 9), ("fwd:generic", "dgrad:ct_outpad(0,1,0)", "run:generic") + W1)
_add("c3d_1x1_s211", 3, 12, 20, (1, 1, 1), (2, 1, 1), (0, 0, 0), (4, 5, 7), ("fwd:generic", "dgrad:ct_outpad(1,0,0)", "run:generic") + W1)
_add("c3d_s111", 3, 12, 20, (3, 3, 3), (1, 1, 1), (1, 1, 1), (3, 5, 6), ("fwd:generic", "dgrad:ct_outpad(0,0,0)", "run:generic") + W1)
_add("c3d_s111_sn", 3, 8, 16, (3, 3, 3), (1, 1, 1), (1, 1, 1), (4, 6, 5), ("fwd:generic", "dgrad:ct_outpad(0,0,0)", "run:generic") + W1, wkind="sn")
# conv1 of the 3-D encoder from the fp32 clip: folded (_StemFn, W even), in place when W is odd (FS._STEM_FOLD off is a test of its own)
_add("stem_folded", 3, 3, 20, (3, 7, 7), (2, 2, 2), (1, 3, 3), (4, 10, 12), ("fwd:stem", "wgrad:stem", "wgrad:single", "run:generic"), inp="src")
_add("stem_in_place_odd_w", 3, 3, 20, (3, 7, 7), (2, 2, 2), (1, 3, 3), (5, 9, 11),
     ("fwd:generic", "wgrad:plain", "wgrad:src_f32", "wgrad:single", "run:generic"), inp="src")
_add("disc_stem_sn", 3, 3, 20, (3, 7, 7), (1, 2, 2), (1, 3, 3), (3, 9, 12),
     ("fwd:generic", "wgrad:plain", "wgrad:src_f32", "wgrad:single", "run:generic"), inp="src", wkind="sn", lim=2)
_add("disc_stem_sn_view", 3, 3, 12, (3, 7, 7), (1, 2, 2), (1, 3, 3), (4, 8, 9),
     ("fwd:generic", "wgrad:plain", "wgrad:src_f32", "wgrad:single", "run:generic"), inp="src_view", wkind="sn")
# the clip entering as a channels-last copy (the generator side of the discriminator): data gradient of the (3, 7, 7) geometry
_add("disc_stem_sn_cl", 3, 3, 12, (3, 7, 7), (1, 2, 2), (1, 3, 3), (3, 8, 9), ("fwd:generic", "dgrad:ct_outpad(0,1,0)", "run:generic") + W1, wkind="sn")
# ---- 2-D cases
G2 = ("fwd:generic", "dgrad:ct_outpad(0,0,0)", "run:generic") + W1
_add("c2d_3x3_s1_bias", 2, 12, 20, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 7, 9), G2, bias=True)
_add("c2d_3x3_s1_bias_sn", 2, 12, 20, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 6, 7), G2, bias=True, wkind="sn")
_add("c2d_3x3_s2_even", 2, 12, 20, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 8, 6), ("fwd:generic", "dgrad:ct_outpad(0,1,1)", "run:generic") + W1, bias=True)
_add("c2d_3x3_s2_odd_sn", 2, 8, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 7, 9), G2, bias=True, wkind="sn")
_add("patchgan_4x4_s2_src", 2, 3, 12, (1, 4, 4), (1, 2, 2), (0, 1, 1), (1, 9, 12),
     ("fwd:generic", "wgrad:plain", "wgrad:src_f32", "wgrad:single", "run:generic"), bias=True, wkind="sn", inp="src")
_add("patchgan_4x4_s2", 2, 12, 20, (1, 4, 4), (1, 2, 2), (0, 1, 1), (1, 9, 8), ("fwd:generic", "dgrad:ct_outpad(0,1,0)", "run:generic") + W1,
     bias=True, wkind="sn")
_add("patchgan_4x4_s1", 2, 12, 20, (1, 4, 4), (1, 1, 1), (0, 1, 1), (1, 6, 7), G2, bias=True, wkind="sn")
_add("patchgan_4x4_s1_to1", 2, 40, 1, (1, 4, 4), (1, 1, 1), (0, 1, 1), (1, 5, 6), G2, bias=True, wkind="sn")
_add("c2d_1x1_f32_rows", 2, 12, 5, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 5, 7), G2, bias=True, out_f32=True)
_add("narrow_64_to_3", 2, 64, 3, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 7, 9),
     ("fwd:generic", "dgrad:ct_outpad(0,0,0)", "run:generic", "wgrad:swapped", "wgrad:single"), bias=True)
_add("narrow_32_to_5", 2, 32, 5, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 6, 5),
     ("fwd:generic", "dgrad:ct_outpad(0,0,0)", "run:generic", "wgrad:swapped", "wgrad:single"))
_add("vgg_first_relu_src", 2, 3, 20, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 7, 9),
     ("fwd:generic", "wgrad:plain", "wgrad:src_f32", "wgrad:single", "run:generic"), bias=True, act="relu", inp="src")
_add("c2d_relu_bias_cl", 2, 12, 20, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 6, 9), G2, bias=True, act="relu", lim=2)
# ---- transposed 3 x 3 / stride 2 / padding 1 / output_padding 1
CT = ("fwd:ct_phases", "dgrad:direct", "wgrad:mirrored", "wgrad:single", "run:phases")
_add("ct_plain", 2, 24, 12, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 5, 7), CT, transposed=True, bias=True)
_add("ct_plain_b", 2, 16, 40, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 4, 6), CT, transposed=True)
_add("ct_sn", 2, 24, 12, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 5, 7), CT, transposed=True, bias=True, wkind="sn")
_add("ct_sn_b", 2, 16, 40, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 3, 5), CT, transposed=True, bias=True, wkind="sn")
_add("ct_sn_frames1", 2, 24, 12, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 5, 7), CT, transposed=True, bias=True, wkind="sn_frames", frames=1, lim=2)
_add("ct_sn_frames3", 2, 16, 40, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 3, 5), CT[:-1], transposed=True, bias=True, wkind="sn_frames", frames=3,
     N=6, lim=2, run=False)
_add("ct_sn_frames3_relu", 2, 24, 12, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 5, 4), CT[:-1], transposed=True, bias=True, act="relu", wkind="sn_frames",
     frames=3, N=6, lim=2, run=False)
# wide layer: in inference the two-tap phases run as 2 x 2 windows with a zero row / column (bf16)
_add("ct_wide_pad2", 2, 128, 96, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 4, 4), CT[:-1] + ("run:phases_pad2",), transposed=True, bias=True,
     labels_f32=CT)
# ---- frame-batched spectral norm on a direct convolution (the decoder's 3 x 3 blocks)
_add("c2d_sn_frames3", 2, 12, 20, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 5, 6), G2[:2] + W1, bias=True, wkind="sn_frames", frames=3, N=6, lim=2, run=False)
# ---- weight-gradient launch modes: rows for two slabs in bf16 (four in f32); the halo kernel's own split count (bf16, 16384 rows)
_add("wgrad_slabs_32x32", 2, 12, 20, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 32, 32), G2[:3] + ("wgrad:plain", "wgrad:slabs"))
_add("wgrad_below_slabs", 2, 12, 20, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 15, 17), G2)
_add("wgrad_kernel_split", 2, 32, 32, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 64, 64), G2[:3] + ("wgrad:plain", "wgrad:kernel_split"), N=4,
     labels_f32=G2[:3] + ("wgrad:plain", "wgrad:slabs"))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ====================================================================== operands and the float64 reference
def mat_view(case, w):
    """mat(W) [cout][cin * taps] of _matrix_geometry / sn_view (ConvTranspose storage: the transposed view)"""
    return (w.transpose(0, 1) if case.transposed else w).reshape(case.cout, -1)


def _conv64(case, x, w5):
    if case.transposed:
        return F.conv_transpose3d(x, w5, None, stride=case.stride, padding=case.pad, output_padding=(0, case.pad[1], case.pad[2]))
    return F.conv3d(x, w5, None, stride=case.stride, padding=case.pad)


class Operands:
    """Integer operands of a case, the float64 expectation of (y, dX, dW, dbias) and the exactness bounds."""

    def __init__(self, case, seed=0, second=False):
        self.case = c = case
        gen = torch.Generator().manual_seed(1000 * seed + sum(map(ord, c.name)) + (7 if second else 0))
        taps = c.k[0] * c.k[1] * c.k[2]
        sig_max = {"plain": 1, "sn": 4, "sn_frames": 8 if c.frames > 1 else 4}[c.wkind]
        # (spectral cases: <G, W> runs over the whole weight, so their automatic limit is capped at 3 instead of 7)
        self.lim = L = c.lim if c.lim is not None else X.operand_limit(taps * c.cin, float(1 << 22) / sig_max ** 2, cap=7 if c.wkind == "plain" else 3)
        wshape = (c.cin, c.cout) + c.k if c.transposed else (c.cout, c.cin) + c.k
        self.x = X.int_operand((c.N, c.cin) + c.ext, L, gen)
        w = X.int_operand(wshape, L, gen)
        self.pairs = []
        if c.wkind != "plain":                      # one-hot (i, j) per frame, mat(W)[i][j] a different power of two per frame
            m = mat_view(c, w)
            for t in range(c.frames):
                i, j = (3 + 5 * t) % c.cout, (7 + 11 * t) % m.shape[1]
                sg = float(2 << t) if c.frames > 1 else (2.0 if len(c.name) % 2 else 4.0)
                assert (i, j) not in [(p[0], p[1]) for p in self.pairs]
                m[i, j] = sg
                self.pairs.append((i, j, sg))
            w = (m.reshape(c.cout, c.cin, *c.k).transpose(0, 1) if c.transposed else m.reshape(wshape)).contiguous()
            for i, j, sg in self.pairs:
                assert float(mat_view(c, w)[i, j]) == sg
        self.w5 = w
        self.w = w if c.dims == 3 else w.squeeze(2)
        self.b = X.int_operand((c.cout,), 4 * L, gen, 0.1) if c.bias else None
        self.dy = X.int_operand((c.N, c.cout) + c.odhw(), min(L, 4), gen)
        self.q = 1.0 / max([p[2] for p in self.pairs] or [1.0])
        self._reference()

    def sigmas(self, w5):
        m = mat_view(self.case, w5)
        return [m[i, j] for i, j, _ in self.pairs]

    def forward64(self, x, w5, b):
        c = self.case
        if c.wkind == "plain":
            pre = _conv64(c, x, w5)
        else:
            sg = self.sigmas(w5)
            per = c.N // len(sg)
            pre = torch.cat([_conv64(c, x[t * per:(t + 1) * per], w5 / s) for t, s in enumerate(sg)], 0)
        if b is not None:
            pre = pre + b.view(1, -1, 1, 1, 1)
        return torch.relu(pre) if c.act == "relu" else pre

    def _reference(self):
        c = self.case
        x = self.x.clone().requires_grad_(True)
        w5 = self.w5.clone().requires_grad_(True)
        b = None if self.b is None else self.b.clone().requires_grad_(True)
        y = self.forward64(x, w5, b)
        assert tuple(y.shape[2:]) == c.odhw(), (tuple(y.shape), c.odhw())
        y.backward(self.dy)
        self.y, self.dx, self.dw5 = y.detach(), x.grad, w5.grad
        self.dw = self.dw5 if c.dims == 3 else self.dw5.squeeze(2)
        self.db = None if b is None else b.grad
        # ---- sums of magnitudes behind every element, in units of each result's quantum
        q = self.q
        g = self.dy.abs() * ((self.y > 0).to(torch.float64) if c.act == "relu" else 1.0)
        xa = self.x.abs().requires_grad_(True)
        sg = [p[2] for p in self.pairs] or [1.0]
        per = c.N // len(sg)
        weff = [(self.w5.abs() / s).requires_grad_(True) for s in sg]
        conv_abs = torch.cat([_conv64(c, xa[t * per:(t + 1) * per], weff[t]) for t in range(len(sg))], 0)
        conv_abs.backward(g)
        sy = conv_abs.detach() + (0 if self.b is None else self.b.abs().view(1, -1, 1, 1, 1))
        self.bounds = {"y": float(sy.max()) / q, "dx": float(xa.grad.max()) / q, "db": float(g.sum((0, 2, 3, 4)).max())}
        if c.wkind == "plain":
            self.bounds["dw"] = float(weff[0].grad.max())
        else:
            # G_t = gradient w.r.t. W / sigma_t; dW = sum_t (G_t - <G_t, W / sigma_t> u_t v_t^T) / sigma_t; the frame-batched kernels take
            # <G_t, W / sigma_t> as <g_t, Y_t - b> over the frame's rows
            dots = [float((weff[t].grad * self.w5.abs()).sum()) for t in range(len(sg))]
            rows = [float((g[t * per:(t + 1) * per] * conv_abs.detach()[t * per:(t + 1) * per]).sum()) for t in range(len(sg))]
            self.bounds["dw"] = sum(float(weff[t].grad.max()) / sg[t] + dots[t] / sg[t] ** 2 for t in range(len(sg))) / q ** 2
            self.bounds["dots"] = max(dots + rows) / q ** 2
        for kind, v in self.bounds.items():
            X.assert_exact_bound(torch.tensor([v]))
        self.saved_y_exact = float(self.y.abs().max()) / q <= 256.0
        if c.act == "relu" or c.wkind == "sn_frames":
            assert self.saved_y_exact, f"{c.name}: the saved output reaches {float(self.y.abs().max()) / q} quanta (> 256): not a bf16 value"


_OPS = {}


def operands(case, seed=0, second=False):
    key = (case.name, seed, second)
    if key not in _OPS:
        _OPS[key] = Operands(case, seed, second)
    return _OPS[key]


# ====================================================================== comparison
def cl_of(t5, dtype, ld=None):
    """float64 [N, C, D, H, W] -> channels-last [N*D*H*W, ld] of the compute dtype on the CPU (padding columns zero)"""
    N, C = t5.shape[:2]
    ld = K.round_up(C, K.e16(dtype)) if ld is None else ld
    out = torch.zeros(t5.numel() // C, ld, dtype=X.tdtype(dt_id(dtype)))
    out[:, :C] = t5.permute(0, 2, 3, 4, 1).reshape(-1, C).to(out.dtype)
    return out


def assert_cl_equal(got, exp5, what):
    """got: [M, ld] device tensor (bf16 or fp32); exp5: float64 [N, C, D, H, W].  Every element, padding columns == 0."""
    got = got.detach().cpu()
    N, C, D, H, W = exp5.shape
    assert got.shape[0] == N * D * H * W and got.shape[1] >= C, f"{what}: shape {tuple(got.shape)} for {tuple(exp5.shape)}"
    E = torch.zeros(got.shape, dtype=torch.float64)
    E[:, :C] = exp5.permute(0, 2, 3, 4, 1).reshape(-1, C)
    d = types.SimpleNamespace(NB=N, Do=D, Ho=H, Wo=W, c_scatter=0, c_cstride=1, c_coff=0)
    X.assert_exact(got, E, None, got.dtype, d, what)


def assert_tensor_equal(got, exp, what):
    """fp32 tensor in PyTorch layout (dW, dbias) == float64 expectation, element for element"""
    assert got is not None, f"{what}: no gradient"
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(exp.shape), f"{what}: {got.dtype} {tuple(got.shape)} for {tuple(exp.shape)}"
    bad = (got.to(torch.float64) != exp) | torch.isnan(got)
    if bool(bad.any()):
        idx = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} mismatching elements; first at {idx}: got {float(got[idx])}, expected {float(exp[idx])} "
                             f"(difference {float(got[idx]) - float(exp[idx])})")


# ====================================================================== branch recorder
class BranchRecorder:
    """Context manager: wraps ``FT._dgrad_phases``, ``FT._conv_transpose_phases``, ``FT._launch_wgrad``, ``K.conv``, ``_StemFn.apply`` and
    the inference helpers ``_Conv._run_phases`` / ``_mid_operand`` and turns their calls into labels:

        fwd:generic | fwd:ct_phases | fwd:stem                       the forward launch of the training op
        dgrad:phases2/4/8 (+ dgrad:empty_class) | dgrad:ct_outpad(d,h,w) | dgrad:direct
        wgrad:plain | wgrad:mirrored | wgrad:swapped | wgrad:stem ; wgrad:src_f32 ; wgrad:single | wgrad:slabs | wgrad:kernel_split
        run:generic | run:mid | run:phases | run:phases_pad2         _Conv.run

    ``phase`` ("fwd", "bwd", "run") is set by the caller around each part."""

    def __init__(self, case):
        self.case, self.phase, self.labels, self.detail = case, "fwd", set(), []
        self._depth, self._sub, self._mid = 0, [], False

    def __enter__(self):
        rec = self
        self._saved = [(FT, "_dgrad_phases", FT._dgrad_phases), (FT, "_conv_transpose_phases", FT._conv_transpose_phases),
                       (FT, "_launch_wgrad", FT._launch_wgrad), (K, "conv", K.conv), (FS._Conv, "_run_phases", FS._Conv._run_phases),
                       (FS._Conv, "_mid_operand", FS._Conv._mid_operand)]
        o_dg, o_ct, o_lw, o_conv, o_rp, o_mid = (s[2] for s in self._saved)
        o_apply = FT._StemFn.apply

        def grouped(fn):
            def call(*a, **kw):
                rec._depth += 1
                rec._sub = []
                try:
                    return fn(*a, **kw)
                finally:
                    rec._depth -= 1
            return call

        def dg(gcl, w, cin, idhw, st, dt):
            out = grouped(o_dg)(gcl, w, cin, idhw, st, dt)
            classes = 2 ** sum(s == 2 for s in st)
            rec.labels.add(f"dgrad:phases{classes}")
            if len(rec._sub) < classes:
                rec.labels.add("dgrad:empty_class")
            assert all(s["scatter"] is not None and len(s["scatter"]) == 5 for s in rec._sub)
            return out

        def ct(*a, **kw):
            out = grouped(o_ct)(*a, **kw)
            rec.labels.add("fwd:ct_phases")
            assert len(rec._sub) == 4
            return out

        def rp(mod, *a, **kw):
            out = grouped(lambda *b, **k2: o_rp(mod, *b, **k2))(*a, **kw)
            pad2 = sum(tuple(s["k"]) == (1, 2, 2) for s in rec._sub) == 3
            rec.labels.add("run:phases_pad2" if pad2 else "run:phases")
            return out

        def mid(mod, *a, **kw):
            rec._mid = True
            return o_mid(mod, *a, **kw)

        def conv(x, w_op, kc, cout, k, stride, pad, dtype, **kw):
            info = dict(k=tuple(k), transposed=bool(kw.get("transposed", False)), out_pad=tuple(kw.get("out_pad", (0, 0, 0))),
                        scatter=kw.get("scatter"))
            if rec._depth:
                rec._sub.append(info)
            elif rec.phase == "run":
                rec.labels.add("run:mid" if rec._mid else "run:generic")
                rec._mid = False
            elif rec.phase == "fwd":
                rec.labels.add("fwd:generic")
            else:
                rec.labels.add("dgrad:ct_outpad(%d,%d,%d)" % info["out_pad"] if info["transposed"] else "dgrad:direct")
            rec.detail.append((rec.phase, info))
            return o_conv(x, w_op, kc, cout, k, stride, pad, dtype, **kw)

        def lw(wd, out, dt, stream, ask_kernel):
            c = rec.case
            pref = _lib.lib().ipoke_conv_wgrad_splitm(byref(wd), FT.ops._dt(dt), FT._WGRAD_HALO_WGS) if ask_kernel else 0
            role = ("stem" if not ask_kernel else "swapped" if wd.w_st != 1 else
                    "mirrored" if (c.transposed and (wd.Nout, wd.Kc_store) == (c.cin, c.cout)) else "plain")
            a_f32 = bool(wd.a_f32)
            res = o_lw(wd, out, dt, stream, ask_kernel)
            splitm = wd.splitm if wd.split_stride > 0 else 1
            rec.labels.add(f"wgrad:{role}")
            rec.labels.add("wgrad:kernel_split" if pref > 0 else ("wgrad:slabs" if splitm > 1 else "wgrad:single"))
            if a_f32:
                rec.labels.add("wgrad:src_f32")
            rec.detail.append(("wgrad", dict(role=role, splitm=splitm, pref=pref, a_f32=a_f32)))
            return res

        def stem_apply(*a):
            rec.labels.add("fwd:stem")
            return o_apply(*a)

        for (obj, name, _), new in zip(self._saved, (dg, ct, lw, conv, rp, mid)):
            setattr(obj, name, new)
        FT._StemFn.apply = staticmethod(stem_apply)
        return self

    def __exit__(self, *exc):
        for obj, name, old in self._saved:
            setattr(obj, name, old)
        del FT._StemFn.apply                        # (inherited from torch.autograd.Function again)
        return False

    def taken(self):
        return tuple(sorted(self.labels))


# ====================================================================== the labels the pure predicates give (no device)
def predicted_labels(case, dtype):
    """fwd / dgrad / wgrad-role labels restated from ``dgrad_phases_ok``, ``stem_folds`` and the ``swapped`` condition of
    ``_weight_gradient``'s comment (stride 1, odd kernel with 'same' padding, at most 16 padded output channels, an input at least four
    times as wide, a channels-last input, not transposed)."""
    c = case
    mod = FS._Conv(c.cin, c.cout, c.k, c.stride, c.pad, bias=c.bias, transposed=c.transposed, snorm=c.wkind != "plain", dims=c.dims)
    out = set()
    src = c.inp != "cl"
    ct_geom = c.transposed and c.k == (1, 3, 3) and c.stride == (1, 2, 2) and c.pad == (0, 1, 1)
    if src and FT.stem_folds(mod, torch.empty((c.N, c.cin) + c.ext)):
        return {"fwd:stem", "wgrad:stem"}
    out.add("fwd:ct_phases" if (ct_geom and not src) else "fwd:generic")
    if not src:
        if c.transposed:
            out.add("dgrad:direct")
        elif c.wkind == "plain" and c.dims == 3 and FT.dgrad_phases_ok(c.k, c.stride, c.pad, c.ext, c.odhw()):
            out.add("dgrad:phases%d" % 2 ** sum(s == 2 for s in c.stride))
            if any(s == 2 and i == 1 for s, i in zip(c.stride, c.ext)):
                out.add("dgrad:empty_class")
        else:
            out.add("dgrad:ct_outpad(%d,%d,%d)" % tuple(i - ((o - 1) * s - 2 * p + k) for i, o, s, p, k in zip(c.ext, c.odhw(), c.stride, c.pad, c.k)))
    e = K.e16(dtype)
    ldg, ldx = K.round_up(c.cout, e), K.round_up(c.cin, e)
    swapped = (not c.transposed and not src and ldg <= 16 and ldx >= 4 * ldg and c.stride == (1, 1, 1)
               and all(k % 2 == 1 and p == k // 2 for k, p in zip(c.k, c.pad)))
    out.add("wgrad:swapped" if swapped else "wgrad:mirrored" if c.transposed else "wgrad:plain")
    if src:
        out.add("wgrad:src_f32")
    return out


PREDICATE_KINDS = ("fwd:", "dgrad:", "wgrad:plain", "wgrad:mirrored", "wgrad:swapped", "wgrad:stem", "wgrad:src_f32")


# ====================================================================== running a case on the device
DEV = "cuda"


def build_module(case, ops_):
    c = case
    mod = FS._Conv(c.cin, c.cout, c.k, c.stride, c.pad, bias=c.bias, transposed=c.transposed, snorm=c.wkind != "plain", dims=c.dims).to(DEV)
    load_operands(mod, ops_)
    return mod


def load_operands(mod, ops_):
    """weight, bias and one-hot u / v of the operand set into the module, in place (a version bump of the parameters); gradients reset"""
    with torch.no_grad():
        weight_of(mod).copy_(ops_.w.to(torch.float32))
        if mod.bias is not None:
            mod.bias.copy_(ops_.b.to(torch.float32))
        if mod.snorm:
            set_one_hot(mod, ops_.pairs[0])
    for p in mod.parameters():
        p.grad = None


def set_one_hot(mod, pair):
    with torch.no_grad():
        mod.weight_u.zero_(); mod.weight_v.zero_()
        mod.weight_u[pair[0]] = 1.0; mod.weight_v[pair[1]] = 1.0


def weight_of(mod):
    return mod.weight_orig if mod.snorm else mod.weight


def weight_handle(case, mod, ops_):
    """what ``conv`` takes as ``w``: None (the plain parameter), a _SnWeight, or a _SnFrames (frames > 1: hand-built from one
    ``iterate = 0`` call per frame with that frame's one-hot pair)"""
    if case.wkind == "plain":
        return None
    if case.wkind == "sn":
        return FT.effective_weight(mod, False)
    if case.frames == 1:
        return FT.effective_weight(mod, False, frames=1)
    sigs, snaps = [], []
    for pair in ops_.pairs:
        set_one_hot(mod, pair)
        one = FT.effective_weight(mod, False)
        sigs.append(one.sig); snaps.append(one.snap)
    set_one_hot(mod, ops_.pairs[0])
    return FT._SnFrames(mod.weight_orig, torch.stack(sigs).contiguous(), torch.stack(snaps).contiguous(), mod.transposed, mod)


def device_input(case, ops_, dtype, x_ld=None):
    """(CL or None, src or None, the tensor whose .grad is dX or None)"""
    c = case
    if c.inp == "cl":
        t = cl_of(ops_.x, dtype, x_ld).to(DEV).requires_grad_(True)
        return K.CL(t, c.N, c.ext, c.cin), None, t
    x = ops_.x.to(torch.float32)
    if c.inp == "src_view":                       # stored (n, d, c, h, w): the five strides differ from the dense ones
        x = x.permute(0, 2, 1, 3, 4).contiguous().to(DEV).permute(0, 2, 1, 3, 4)
        assert not x.is_contiguous()
    else:
        x = x.to(DEV)
    if c.dims == 2:
        x = x[:, :, 0]
        st = (x.stride(0), x.stride(1), 0, x.stride(2), x.stride(3))
    else:
        st = tuple(x.stride(i) for i in range(5))
    return None, (x, c.N, c.cin, c.ext, st), None


ACT = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU}


def forward_op(case, mod, dtype, rec, xcl, src, ops_):
    """the training op's forward as the models call it (first_stage_train: the folded stem where ``stem_folds`` allows it); returns CL"""
    rec.phase = "fwd"
    if src is not None and FT.stem_folds(mod, src[0]):
        return FT.stem(src[0], mod.weight, dtype)
    return FT.conv(mod, xcl, dtype, act=ACT[case.act], out_f32=case.out_f32, src=src, w=weight_handle(case, mod, ops_))


def device_dy(case, ops_, dtype, mode="cl"):
    """dy as the op's consumer hands it over: "cl" (compute dtype, padded pitch; fp32 [M, cout] behind an fp32 output), "f32" (fp32 of
    the padded pitch into a compute-dtype op), "slice" (a non-contiguous column slice of a wider buffer)"""
    if case.out_f32:
        return ops_.dy.permute(0, 2, 3, 4, 1).reshape(-1, case.cout).to(torch.float32).to(DEV)
    t = cl_of(ops_.dy, dtype)
    if mode == "f32":
        return t.to(torch.float32).to(DEV)
    if mode == "slice":
        wide = torch.full((t.shape[0], 2 * t.shape[1] + 8), X.SENT, dtype=t.dtype)
        wide[:, 8:8 + t.shape[1]] = t
        v = wide.to(DEV)[:, 8:8 + t.shape[1]]
        assert not v.is_contiguous()
        return v
    return t.to(DEV)


def run_training_case(case, dtype, ops_=None, dy_mode="cl", x_ld=None, check_labels=True, mod=None, need=(True, True, True), ctx=None):
    """forward + backward of the training op on the device, every result against the float64 expectation.  ``need``: which of (x, weight,
    bias) require a gradient; ``ctx``: a context manager around forward and backward (``wgrad_side_stream``).  Returns the recorder (with
    ``mod`` and the dX holder as attributes)."""
    import contextlib
    ops_ = operands(case) if ops_ is None else ops_
    mod = build_module(case, ops_) if mod is None else mod
    for p in mod.parameters():
        p.grad = None
    weight_of(mod).requires_grad_(need[1])
    if case.bias:
        mod.bias.requires_grad_(need[2])
    with BranchRecorder(case) as rec:
        with (ctx if ctx is not None else contextlib.nullcontext()):
            xcl, src, holder = device_input(case, ops_, dtype, x_ld)
            if holder is not None:
                holder.requires_grad_(need[0])
            out = forward_op(case, mod, dtype, rec, xcl, src, ops_)
            assert tuple(out.dhw) == case.odhw() and out.C == case.cout
            assert_cl_equal(out.t, ops_.y, f"{case.name} {dtype} y")
            rec.phase = "bwd"
            out.t.backward(device_dy(case, ops_, dtype, dy_mode))
        torch.cuda.synchronize()
    rec.mod, rec.holder = mod, holder
    what = f"{case.name} {dtype}"
    if holder is not None and need[0]:
        assert holder.grad is not None and holder.grad.shape == holder.shape, f"{what}: dX missing or of another pitch"
        assert_cl_equal(holder.grad, ops_.dx, f"{what} dX")
    elif holder is not None:
        assert holder.grad is None and not any(l.startswith("dgrad:") for l in rec.labels), f"{what}: a data gradient nobody asked for: {rec.taken()}"
    if need[1]:
        assert_tensor_equal(weight_of(mod).grad, ops_.dw, f"{what} dW")
    else:
        assert weight_of(mod).grad is None and not any(l.startswith("wgrad:") for l in rec.labels), f"{what}: a weight gradient nobody asked for"
    if case.bias and need[2]:
        assert_tensor_equal(mod.bias.grad, ops_.db, f"{what} dbias")
    elif case.bias:
        assert mod.bias.grad is None
    if check_labels:
        want = tuple(l for l in case.want(dtype) if not l.startswith("run:"))
        assert rec.taken() == want, f"{what}: took {rec.taken()}, the table says {want}; launches: {rec.detail}"
    return rec


def run_inference_case(case, dtype, ops_=None, mod=None, check_labels=True):
    """``_Conv.run`` on the same operands: the forward output against the same expectation"""
    ops_ = operands(case) if ops_ is None else ops_
    mod = build_module(case, ops_) if mod is None else mod
    mod.invalidate()
    xcl, src, holder = device_input(case, ops_, dtype)
    if holder is not None:
        holder.requires_grad_(False)
    with BranchRecorder(case) as rec, torch.no_grad():
        rec.phase = "run"
        out = mod.run(xcl, dtype, act=ACT[case.act], out_f32=case.out_f32, src_f32=src)
        torch.cuda.synchronize()
    assert tuple(out.dhw) == case.odhw()
    assert_cl_equal(out.t, ops_.y, f"{case.name} {dtype} _Conv.run")
    want = tuple(l for l in case.want(dtype) if l.startswith("run:"))
    if check_labels:
        assert rec.taken() == want, f"{case.name} {dtype}: _Conv.run took {rec.taken()}, the table says {want}; launches: {rec.detail}"
    return rec
