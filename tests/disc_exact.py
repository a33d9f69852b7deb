"""Kernel-by-kernel checking of the adversarial step (csrc/vae_train.hip, csrc/vae_bwd.hip, csrc/norm.hip): the pooling kernels of the
discriminators, the feature-matching / reconstruction L1 terms, the element-wise helpers around them and the GroupNorm tangent of the
gradient penalty.  References, input generators and the harness; the test functions are in test_disc_kernels_cpu.py (which pins the
references and the input conditions) and test_disc_kernels_gpu.py (which runs the kernels).

* Guarded buffers: every tensor a kernel receives is the first ``rows`` rows of a ``[rows + GUARD][ld]`` buffer filled with ``SENT``;
  ``check_guard`` verifies afterwards that every element the kernel's contract does not let it write still holds ``SENT`` (and that the
  padding columns a contract zero-fills are zero).  Input padding and guard rows hold ``SENT`` too, so an over-read changes a result.
* ``maxpool_ref``: float64 values and the int32 input row of the FIRST maximum in (d, h, w) scan order, from an explicit tap stack and a
  first-true mask (``argmax`` leaves the order of ties open); ``maxpool_bwd_ref`` (an ``index_add_``) and ``gather_ref``.
* ``gn_jvp_ref``: the GroupNorm tangent and its backward in float64 through ``torch.func.jvp`` and ``torch.autograd.grad``;
  ``gn_jvp_f32_restated``: the closed forms of the comment above ``gn_jvp_sums_kernel`` in fp32 torch with two-pass statistics -- the
  yardstick of the fp32 tolerance, which never runs the code under test.
* Generators of the operands (integers for the exact comparisons) shared by the two test files, so that the conditions the CPU file
  asserts on them (ties, rows chosen twice or never, equal / greater / smaller pairs, mask density) hold for what the GPU file runs.
"""
import collections
import ctypes

import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from tests.conv_exact import act64, act_grad_from_out64, round_up  # noqa: F401  (re-exported for the test files)
from tests.optim_exact import assert_same, cast_like  # noqa: F401

SENT = 4096.0                 # exact in bf16 and fp32
IDX_SENT = -12345             # fills the int32 elements behind an index table
GUARD = 8                     # rows behind the last one a launch may touch
F64 = torch.float64
DTYPES = {"f32": (_lib.F32, torch.float32, 4), "bf16": (_lib.BF16, torch.bfloat16, 8)}     # C-ABI code, torch dtype, elements per 16 bytes


# ------------------------------------------------------------------ guarded buffers
def guarded(rows, ld, dtype, device, values=None, fill=SENT):
    """[rows + GUARD][ld] buffer of `fill`; values ([rows][c] float64 or None) go to the first columns of the first rows.  The kernel
    receives the buffer's address with pitch ld and `rows` rows."""
    buf = torch.full((rows + GUARD, ld), fill, dtype=dtype, device=device)
    if values is not None:
        assert values.shape[0] == rows and values.shape[1] <= ld
        buf[:rows, : values.shape[1]] = values.to(dtype)
    return buf


def check_guard(buf, rows, cols, zero_to=None, what=""):
    """columns >= cols of the first `rows` rows and every guard row still hold SENT; with zero_to, columns [cols, zero_to) hold zeros (the
    padding a contract zero-fills) and SENT begins at zero_to"""
    b = buf.to(F64)
    assert bool((b[rows:] == SENT).all()), f"{what}: write behind the last row"
    first = cols if zero_to is None else zero_to
    assert bool((b[:rows, first:] == SENT).all()), f"{what}: write into the columns >= {first} of the pitch"
    if zero_to is not None:
        assert bool((b[:rows, cols:zero_to] == 0).all()), f"{what}: padding columns [{cols}, {zero_to}) are not zero"


def ulp_f32(v):
    """unit in the last place of |v| in fp32 (normal range; float64 tensor)"""
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -100))) - 23)


def ulp_bf16(v):
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -100))) - 7)


def ulp_of(v, tdtype):
    return ulp_bf16(v) if tdtype == torch.bfloat16 else ulp_f32(v)


def assert_close_ulp(got, ref64, n_ulp, tdtype, what=""):
    """|got - ref| <= n_ulp units in the last place of ref in the output type; names the first element that misses"""
    g = got.to(F64)
    bad = ~((g - ref64).abs() <= n_ulp * ulp_of(ref64, tdtype))
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements beyond {n_ulp} ulp; first at element {i}: got {float(g.reshape(-1)[i])!r}, "
                             f"reference {float(ref64.reshape(-1)[i])!r}")


def randint64(lo, hi, shape, gen):
    """integers in [lo, hi] as float64 (CPU generator)"""
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64).to(F64)


# ------------------------------------------------------------------ max-pooling
class PoolGeom(collections.namedtuple("PoolGeom", "N C D H W k s p")):
    @property
    def out(self):
        return tuple((i + 2 * p - k) // s + 1 for i, k, s, p in zip((self.D, self.H, self.W), self.k, self.s, self.p))

    @property
    def rows_in(self):
        return self.N * self.D * self.H * self.W

    @property
    def rows_out(self):
        o = self.out
        return self.N * o[0] * o[1] * o[2]

    def dims(self):
        """the int32[17] geometry array of ipoke_maxpool3d_fwd / _bwd"""
        return (ctypes.c_int32 * 17)(self.N, self.C, self.D, self.H, self.W, *self.out, *self.k, *self.s, *self.p)


POOL_GEOMS = {
    "disc": PoolGeom(2, 8, 3, 6, 10, (3, 3, 3), (1, 2, 2), (1, 1, 1)),        # the temporal discriminator's geometry
    "vgg": PoolGeom(2, 8, 1, 7, 6, (1, 2, 2), (1, 2, 2), (0, 0, 0)),          # the VGG pools, odd H: the last row belongs to no window
    "lopsided": PoolGeom(1, 8, 4, 5, 7, (2, 3, 3), (2, 1, 2), (0, 1, 1)),
    "wrap": PoolGeom(4, 64, 4, 66, 64, (3, 3, 3), (1, 2, 2), (1, 1, 1)),      # 1 081 344 outputs: the grid-stride loop of 4096 blocks wraps
}
# backward variants: (channels or None for the geometry's own, extra pitch of dy, extra pitch of dx)
POOL_BWD_VARIANTS = {
    "own": (None, 8, 8),       # C and both pitches multiples of 8: the 8-channel vector kernel in bf16
    "c12": (12, 4, 4),         # C = 12, pitches 16
    "ldy12": (8, 4, 8),        # C = 8, ldy = 12, ldx = 16
}


def pool_data(g, seed):
    """x [rows_in][C], dy [rows_out][C], xdot [rows_in][C]: integers in [-3, 3] (float64, CPU) -- windows of up to 27 taps over seven
    values tie almost everywhere, and sums of <= 27 gradients stay exact in bf16"""
    gen = torch.Generator().manual_seed(seed)
    return (randint64(-3, 3, (g.rows_in, g.C), gen), randint64(-3, 3, (g.rows_out, g.C), gen), randint64(-3, 3, (g.rows_in, g.C), gen))


def pool_taps(g, device):
    """[taps][rows_out] input row of every (tap, output position) and whether the tap lies on the input; taps in (d, h, w) scan order"""
    Do, Ho, Wo = g.out
    o = torch.arange(g.rows_out, device=device)
    ow = o % Wo
    t = o // Wo
    oh = t % Ho
    t = t // Ho
    od = t % Do
    n = t // Do
    rows, valid = [], []
    for a in range(g.k[0]):
        d = od * g.s[0] - g.p[0] + a
        for b in range(g.k[1]):
            h = oh * g.s[1] - g.p[1] + b
            for e in range(g.k[2]):
                w = ow * g.s[2] - g.p[2] + e
                ok = (d >= 0) & (d < g.D) & (h >= 0) & (h < g.H) & (w >= 0) & (w < g.W)
                rows.append(torch.where(ok, ((n * g.D + d) * g.H + h) * g.W + w, torch.zeros_like(o)))
                valid.append(ok)
    return torch.stack(rows), torch.stack(valid)


def maxpool_ref(x, g):
    """x [rows_in][C] -> (y float64 [rows_out][C], idx int32 [rows_out][C]): the maximum over the taps that lie on the input and the input
    row of the FIRST tap, in (d, h, w) scan order, that holds it"""
    x = x.to(F64)
    rows, valid = pool_taps(g, x.device)
    assert bool(valid.any(0).all()), "a window without any tap on the input"
    neg = torch.full((), -float("inf"), dtype=F64, device=x.device)
    stack = torch.where(valid.unsqueeze(-1), x[rows], neg)                     # [taps][rows_out][C]
    y = stack.amax(0)
    found = torch.zeros(y.shape, dtype=torch.bool, device=x.device)
    idx = torch.full(y.shape, -1, dtype=torch.int64, device=x.device)
    for t in range(stack.shape[0]):
        first = (stack[t] == y) & ~found                                       # the first-true mask of this tap
        idx = torch.where(first, rows[t].unsqueeze(-1), idx)
        found |= first
    assert bool(found.all())
    return y, idx.to(torch.int32)


def maxpool_bwd_ref(dy, idx, rows_in):
    """dx [rows_in][C] float64: every output's gradient added to the input row it chose"""
    C = dy.shape[1]
    dx = torch.zeros(rows_in * C, dtype=F64, device=dy.device)
    flat = idx.to(torch.int64) * C + torch.arange(C, device=dy.device)
    dx.index_add_(0, flat.reshape(-1), dy.to(F64).reshape(-1))
    return dx.view(rows_in, C)


def gather_ref(x, idx):
    """y[o][c] = x[idx[o][c]][c]"""
    return torch.gather(x, 0, idx.to(torch.int64))


def selection_counts(idx, rows_in):
    """[rows_in][C]: how many windows chose each input element"""
    C = idx.shape[1]
    flat = idx.to(torch.int64) * C + torch.arange(C, device=idx.device)
    return torch.bincount(flat.reshape(-1), minlength=rows_in * C).view(rows_in, C)


# ------------------------------------------------------------------ L1 operands
def l1_pair_data(M, C, seed):
    """a, b [M][C] integers (float64, CPU), about a third of them equal"""
    gen = torch.Generator().manual_seed(seed)
    a = randint64(-2, 2, (M, C), gen)
    d = randint64(1, 2, (M, C), gen) * torch.where(torch.rand((M, C), generator=gen) < 0.5, -1.0, 1.0)
    same = torch.rand((M, C), generator=gen) < 1.0 / 3.0
    return a, torch.where(same, a, a + d)


# ------------------------------------------------------------------ GroupNorm tangent
GnCase = collections.namedtuple("GnCase", "name N S C_f32 C_bf16 G gamma act res shift")
GN_CASES = [
    GnCase("instance", 2, 130, 16, 16, 16, False, _lib.ACT_RELU, True, 0.0),     # cpg 1 < the vector width, ragged second chunk (2 rows)
    GnCase("cpg2-short", 2, 5, 16, 16, 8, True, _lib.ACT_NONE, False, 0.0),      # a single short chunk
    GnCase("cpg8", 3, 256, 32, 32, 4, True, _lib.ACT_RELU, True, 0.0),           # cpg = the bf16 vector width, two full chunks
    GnCase("idle", 2, 130, 24, 24, 3, True, _lib.ACT_RELU, False, 0.0),          # 256 threads over 6 / 3 column groups: idle threads
    GnCase("g0-loop", 1, 3, 1040, 2080, 4, True, _lib.ACT_NONE, False, 0.0),     # 260 column groups: the loop over 256 of them
    GnCase("three-chunks", 2, 257, 64, 64, 32, True, _lib.ACT_RELU, True, 0.0),  # the last chunk holds one row
]
GN_SHIFTED = GnCase("shifted", 2, 130, 16, 16, 4, True, _lib.ACT_RELU, False, 16.0)   # mean / std = 16 (fp32 only)
EPS = 1e-5


def gn_inputs(case, tdtype, seed=0):
    """the operands of a tangent case as the kernel sees them (rounded to tdtype, then float64; CPU): dict of x, xdot, q [N][S][C],
    gamma [C] or None (fp32 values), y (the primal output that carries the ReLU mask) or None, resdot or None"""
    C = case.C_bf16 if tdtype == torch.bfloat16 else case.C_f32
    gen = torch.Generator().manual_seed(1000 + seed)
    shape = (case.N, case.S, C)

    def rnd(scale=1.0, offset=0.0):
        return (torch.randn(shape, generator=gen, dtype=F64) * scale + offset).to(tdtype).to(F64)

    d = dict(C=C, x=rnd(1.0, case.shift), xdot=rnd(), q=rnd())
    d["gamma"] = (1.0 + 0.3 * torch.randn(C, generator=gen)).to(torch.float32).to(F64) if case.gamma else None
    beta = 0.2 * torch.randn(C, generator=gen, dtype=F64)
    res = rnd(0.5) if case.res else None
    d["resdot"] = rnd() if case.res else None
    d["y"] = None
    if case.act != _lib.ACT_NONE:
        pre = F.group_norm(d["x"].permute(0, 2, 1), case.G, d["gamma"], beta, EPS).permute(0, 2, 1)
        if res is not None:
            pre = pre + res
        d["y"] = act64(case.act, pre).to(tdtype).to(F64)
    return d


def act_mask(act, y):
    """the activation's derivative at the primal output y (a scalar one without activation)"""
    return torch.ones((), dtype=F64) if act == _lib.ACT_NONE else act_grad_from_out64(act, y)


def gn_jvp_ref(x, xdot, q, gamma, G, act, y=None, resdot=None, eps=EPS):
    """float64 reference of ipoke_groupnorm_jvp and ipoke_groupnorm_jvp_bwd: ydot by torch.func.jvp through F.group_norm, times the
    activation's derivative at the primal output y, plus the residual tangent; the backward by autograd of sum(ydot * q).
    Returns dict(ydot, dxdot, dx, dgamma, dresdot) (dresdot None without a residual); gamma None is a gain of ones."""
    C = x.shape[-1]
    x = x.clone().requires_grad_(True)
    xdot = xdot.clone().requires_grad_(True)
    gam = (torch.ones(C, dtype=F64) if gamma is None else gamma.clone()).to(x.device).requires_grad_(True)
    rd = None if resdot is None else resdot.clone().requires_grad_(True)
    da = act_mask(act, y)

    def norm(v):
        return F.group_norm(v.permute(0, 2, 1), G, gam, None, eps).permute(0, 2, 1)

    _, t = torch.func.jvp(norm, (x,), (xdot,))
    ydot = (t + rd if rd is not None else t) * da
    wrt = [x, xdot, gam] + ([rd] if rd is not None else [])
    grads = torch.autograd.grad((ydot * q).sum(), wrt)
    return dict(ydot=ydot.detach(), dx=grads[0], dxdot=grads[1], dgamma=grads[2], dresdot=grads[3] if rd is not None else None)


def gn_jvp_f32_restated(x, xdot, q, gamma, G, act, y=None, resdot=None, eps=EPS, dtype=torch.float32):
    """the closed forms of csrc/vae_train.hip (comment above gn_jvp_sums_kernel) in fp32 torch with two-pass statistics (mean first, then
    the moments of the centred values): what fp32 arithmetic gives without any cancellation in the statistics.  Same outputs as gn_jvp_ref.
    (dtype = float64 evaluates the same formulas in double: the check that they are the right derivative.)"""
    f = dtype
    N, S, C = x.shape
    cpg = C // G
    shp = (N, S, G, cpg)
    x, u, q = x.to(f).view(shp), xdot.to(f).view(shp), q.to(f).view(shp)
    gm = (torch.ones(C) if gamma is None else gamma).to(f).view(1, 1, G, cpg)
    da = act_mask(act, y).to(f)
    da = da.view(shp) if da.dim() else da
    mean = lambda v: v.mean(dim=(1, 3), keepdim=True)             # noqa: E731
    xc = x - mean(x)
    r = torch.rsqrt(mean(xc * xc) + eps)
    xh = xc * r
    ub, mm = mean(u), mean(xh * u)
    proj = r * (u - ub - xh * mm)
    yd = gm * proj
    if resdot is not None:
        yd = yd + resdot.to(f).view(shp)
    qd = q * da
    w = qd * gm
    aa, bb, cc = mean(w), mean(w * xh), mean(w * u)
    k0 = cc - aa * ub - 3.0 * bb * mm
    out = dict(ydot=yd * da, dxdot=r * (w - aa - xh * bb), dx=-r * r * (xh * k0 + mm * (w - aa) + bb * (u - ub)),
               dgamma=(qd * proj).sum(dim=(0, 1)).reshape(C), dresdot=qd.expand(shp) if resdot is not None else None)
    return {k: (v.reshape(N, S, C) if v is not None and k != "dgamma" else v) for k, v in out.items()}


def rel_err(got, ref):
    """max |got - ref| relative to the reference's maximum"""
    return float((got.to(F64) - ref).abs().max() / ref.abs().max().clamp(min=1e-300))
