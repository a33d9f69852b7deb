"""The kernels of csrc/image_gan.hip one by one against float64 (tests/image_gan_ref.py) on sentinel-guarded buffers, each launched twice
with bit-identical results.

Bounds.  ``ipoke_hinge_terms`` / ``ipoke_gp_direction``: the sums run in double and are rounded to fp32 once (2^-24 relative); the bound
4 * 2^-24 leaves room for the double sums' own order.  Gradient columns and ``v`` are a correctly rounded constant / a correctly rounded
product: exact against the float64 value rounded to fp32.  ``ipoke_act_jvp``: the product is formed in double and rounded once -- exact
in f32; in bf16 the fp32 value is rounded again, which can differ from the directly rounded product by one bf16 ulp.
``ipoke_groupnorm_tangent`` (the fixed-order form of ``ipoke_groupnorm_jvp``): double arithmetic on the stored operands, so 4 * 2^-24 of
the output's range in f32 and one bf16 ulp in bf16.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from ipoke_amd._lib import ptr
from tests import image_gan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 4096.0
GUARD = 64
EPS32 = 2.0 ** -24


def guarded(n, dtype=torch.float32, fill=None):
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(fill.reshape(-1).to(DEV))
    return buf, view


def intact(buf, n):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


def run(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ hinge terms
@functools.lru_cache(maxsize=None)
def hinge_case(M):
    p = torch.randn(M, generator=torch.Generator().manual_seed(M)) * 1.5
    p[0], p[1], p[2], p[M - 1] = 1.0, -1.0, 0.0, 1.0          # 1 - pred == 0, 1 + pred == 0, y == 0
    return p, {mode: R.hinge_terms_ref(p.double(), mode) for mode in (0, 1, 2)}


@pytest.mark.parametrize("mode", [_lib.HINGE_REAL, _lib.HINGE_FAKE, _lib.HINGE_GENERATOR])
@pytest.mark.parametrize("M,ld", [(8, 3), (72, 5), (700, 1)])
def test_hinge_terms_against_float64(M, ld, mode):
    p, refs = hinge_case(M)
    loss, sig, grad = refs[mode]
    lib = _lib.lib()
    npart = int(lib.ipoke_hinge_terms_partials())
    col = torch.full((M, ld), SENT)
    col[:, 0] = p
    pb, pv = guarded(M * ld, fill=col)
    ldg = ld + 1
    runs = []
    for _ in range(2):
        ob, ov = guarded(2)
        gb, gv = guarded(M * ldg)
        qb, qv = guarded(npart, dtype=torch.float64)
        run(lib.ipoke_hinge_terms(ptr(pv), ld, M, mode, ptr(ov), ptr(gv), ldg, ptr(qv), _lib.current_stream()))
        assert intact(ob, 2) and intact(gb, M * ldg) and intact(qb, npart) and intact(pb, M * ld), "a sentinel next to a buffer was overwritten"
        g2 = gv.view(M, ldg).cpu()
        assert bool((g2[:, 1:] == SENT).all()), "the gradient column's gaps were written"
        runs.append((ov.cpu().clone(), g2[:, 0].clone()))
    assert torch.equal(pv.view(M, ld).cpu(), col), "the input was modified"
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "a second run is not bit-identical"
    out, g = runs[0]
    e_loss, e_sig = abs(out[0].item() - loss) / abs(loss), abs(out[1].item() - sig) / sig
    print(f"hinge_terms M={M} ld={ld} mode={mode}: value rel err {e_loss:.2e}, mean sigmoid {e_sig:.2e} (bound {4 * EPS32:.2e})")
    assert e_loss <= 4 * EPS32 and e_sig <= 4 * EPS32
    assert torch.equal(g, grad.float()), "the gradient column is +-1/M rounded to fp32, and exactly 0 where the hinge is inactive"
    if mode == _lib.HINGE_REAL:
        assert g[0] == 0 and g[M - 1] == 0 and g[1] < 0 and g[2] < 0          # pred == 1: relu'(0) = 0
    if mode == _lib.HINGE_FAKE:
        assert g[1] == 0 and g[0] > 0 and g[2] > 0                            # pred == -1
    if mode == _lib.HINGE_GENERATOR:
        assert bool((g == g[0]).all()) and g[0] < 0


# ------------------------------------------------------------------------------------------------ activation tangent
@functools.lru_cache(maxsize=None)
def act_case(M, C):
    g = torch.Generator().manual_seed(10 * M + C)
    y = torch.randn(M, C, generator=g)
    y[torch.rand(M, C, generator=g) < 0.1] = 0.0                              # y == 0: the slope of y < 0
    return y, torch.randn(M, C, generator=g) * 3


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("act,name", [(_lib.ACT_LRELU02, "lrelu"), (_lib.ACT_RELU, "relu")])
@pytest.mark.parametrize("M,C,ld,Cpad", [(37, 64, 64, 64), (9, 64, 80, 72), (300, 5, 8, 8)])
def test_act_jvp_against_float64(M, C, ld, Cpad, act, name, dt):
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    y, xd = (v.to(tdt) for v in act_case(M, C))
    ref = R.act_jvp_ref(y.double(), xd.double(), name)
    pad = lambda v: torch.cat([v, torch.full((M, ld - C), SENT, dtype=tdt)], 1)
    yb, yv = guarded(M * ld, tdt, pad(y))
    xb, xv = guarded(M * ld, tdt, pad(xd))
    runs = []
    for _ in range(2):
        ob, ov = guarded(M * ld, tdt)
        run(_lib.lib().ipoke_act_jvp(ptr(yv), ld, ptr(xv), ld, ptr(ov), ld, M, C, Cpad, act, _lib.DTYPES[dt], _lib.current_stream()))
        assert intact(ob, M * ld) and intact(yb, M * ld) and intact(xb, M * ld)
        runs.append(ov.view(M, ld).cpu().clone())
    assert torch.equal(*runs), "a second run is not bit-identical"
    assert torch.equal(yv.view(M, ld).cpu(), pad(y)) and torch.equal(xv.view(M, ld).cpu(), pad(xd)), "an input was modified"
    out = runs[0]
    assert bool((out[:, C:Cpad] == 0).all()), "padded columns are written as zero"
    assert bool((out[:, Cpad:] == SENT).all()), "columns behind the padded width were written"
    got = out[:, :C].double()
    assert int((y == 0).sum()) > 0
    if dt == "f32":
        assert torch.equal(got, ref.float().double()), "f32: the product rounded once"
    else:
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
        assert bool(((got - ref).abs() <= ulp).all()), "bf16: within one ulp"


# ------------------------------------------------------------------------------------------------ penalty value and direction
@pytest.mark.parametrize("N,L", [(2, 3 * 32 * 32), (3, 777), (5, 16 * 256 + 1)])
def test_gp_direction_against_float64(N, L):
    g = torch.randn(N, L, generator=torch.Generator().manual_seed(L)) * 0.3
    mean, per, v = R.gp_direction_ref(g.double())
    lib = _lib.lib()
    npart = int(lib.ipoke_gp_direction_partials(N))
    gb, gv = guarded(N * L, fill=g)
    runs = []
    for _ in range(2):
        vb, vv = guarded(N * L)
        ob, ov = guarded(1 + N)
        qb, qv = guarded(npart, dtype=torch.float64)
        run(lib.ipoke_gp_direction(ptr(gv), N, L, ptr(vv), ptr(ov), ptr(qv), _lib.current_stream()))
        assert intact(vb, N * L) and intact(ob, 1 + N) and intact(qb, npart) and intact(gb, N * L)
        runs.append((ov.cpu().clone(), vv.view(N, L).cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "a second run is not bit-identical"
    assert torch.equal(gv.view(N, L).cpu(), g), "the input was modified"
    out, vg = runs[0]
    e_mean = abs(out[0].item() - mean) / mean
    e_per = ((out[1:].double() - per).abs() / per).max().item()
    print(f"gp_direction N={N} L={L}: mean rel err {e_mean:.2e}, per sample {e_per:.2e} (bound {4 * EPS32:.2e})")
    assert e_mean <= 4 * EPS32 and e_per <= 4 * EPS32
    assert torch.equal(vg, v.float()), "v = (2 / N) g rounded to fp32 once"


# ------------------------------------------------------------------------------------------------ GroupNorm tangent, fixed order
def gn_tangent_ref(x, u, q, gamma, G, slope):
    """float64: ydot by torch.func.jvp through group_norm + leaky_relu, and the gradients of <q, ydot> w.r.t. xdot, x and gamma."""
    x = x.clone().requires_grad_()
    u = u.clone().requires_grad_()
    gamma = gamma.clone().requires_grad_()
    beta = torch.zeros_like(gamma)
    xn, un = x.permute(0, 2, 1), u.permute(0, 2, 1)                                  # [N, C, S]
    f = lambda a: F.group_norm(a, G, gamma, beta, 1e-5)
    y, yd_lin = torch.func.jvp(f, (xn,), (un,))
    mask = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope)).detach() if slope is not None else torch.ones_like(y)
    yd = (yd_lin * mask).permute(0, 2, 1)
    act = (F.leaky_relu(y, slope) if slope is not None else y).permute(0, 2, 1).detach()
    dxd, dx, dg = torch.autograd.grad((yd * q).sum(), (u, x, gamma))
    return act, yd.detach(), dxd, dx, dg


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,S,C,act", [(2, 49, 128, _lib.ACT_LRELU02), (3, 16, 512, _lib.ACT_LRELU02), (2, 9, 64, _lib.ACT_NONE), (1, 300, 256, _lib.ACT_RELU)])
def test_groupnorm_tangent_against_float64(N, S, C, act, dt):
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    G, code = 16, _lib.DTYPES[dt]
    gen = torch.Generator().manual_seed(S * C)
    x = (torch.randn(N, S, C, generator=gen) * 1.3 + 0.4).to(tdt)
    u = torch.randn(N, S, C, generator=gen).to(tdt)
    q = torch.randn(N, S, C, generator=gen).to(tdt)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=gen)
    slope = {_lib.ACT_LRELU02: 0.2, _lib.ACT_RELU: 0.0, _lib.ACT_NONE: None}[act]
    y64, yd, dxd, dx, dg = gn_tangent_ref(x.double(), u.double(), q.double(), gamma.double(), G, slope)
    y = y64.to(tdt)                                                # the primal output as the norm kernel would store it
    # keep the mask unambiguous: the stored y decides, so take the reference's mask from the stored y as well
    assert bool(((y.double() > 0) == (y64 > 0)).all())
    M = N * S
    bufs = {k: guarded(M * C, tdt, v) for k, v in (("x", x), ("u", u), ("q", q), ("y", y))}
    gam = gamma.to(DEV)
    lib, s = _lib.lib(), _lib.current_stream()
    runs = []
    for _ in range(2):
        outs = {k: guarded(M * C, tdt) for k in ("yd", "dxd", "dx")}
        rb, rv = guarded(N * C)
        run(lib.ipoke_groupnorm_tangent(ptr(bufs["x"][1]), C, ptr(bufs["u"][1]), C, ptr(bufs["y"][1]), C, ptr(outs["yd"][1]), C, ptr(gam), N, S, C, G,
                                        act, 1e-5, code, s))
        run(lib.ipoke_groupnorm_tangent_bwd(ptr(bufs["x"][1]), C, ptr(bufs["u"][1]), C, ptr(bufs["y"][1]), C, ptr(bufs["q"][1]), C,
                                            ptr(outs["dxd"][1]), C, ptr(outs["dx"][1]), C, ptr(rv), ptr(gam), N, S, C, G, act, 1e-5, code, s))
        assert all(intact(b, M * C) for b, _ in list(outs.values()) + list(bufs.values())) and intact(rb, N * C)
        runs.append({**{k: v.view(N, S, C).cpu().clone() for k, (_, v) in outs.items()}, "rows": rv.view(N, C).cpu().clone()})
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), "a second run is not bit-identical"
    for k, src in (("x", x), ("u", u), ("q", q), ("y", y)):
        assert torch.equal(bufs[k][1].view(N, S, C).cpu(), src), f"input {k} was modified"
    for k, ref in (("yd", yd), ("dxd", dxd), ("dx", dx)):
        got = runs[0][k].double()
        tol = 4 * EPS32 * ref.abs().max()
        if dt == "bf16":
            tol = tol + 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
        worst = ((got - ref).abs() / tol).max().item()
        print(f"groupnorm_tangent N={N} S={S} C={C} act={act} {dt} {k}: err / tol {worst:.3f}")
        assert worst <= 1.0, k
    rows = runs[0]["rows"].double()                                # one fp32 rounding per sample's row
    e_g = ((rows.sum(0) - dg).abs().max() / rows.abs().sum(0).max()).item()
    print(f"groupnorm_tangent N={N} S={S} C={C} act={act} {dt} dgamma: err / sum of the rows' magnitudes {e_g:.2e}")
    assert e_g <= 2 * EPS32
