"""The references of tests/disc_exact.py pinned without a GPU, the conditions the generated inputs must meet for a green GPU test to mean
something, and the argument checks of the entry points (they return before any HIP call, so dummy addresses do)."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from tests import disc_exact as X

F64 = torch.float64


def pool_cases():
    """every (geometry, channels) the GPU file runs: the forward table and the backward variants"""
    out = {}
    for name, g in X.POOL_GEOMS.items():
        out[(name, g.C)] = g
        for c, _, _ in X.POOL_BWD_VARIANTS.values():
            if c is not None:
                out[(name, c)] = g._replace(C=c)
    return out


POOL_CASES = pool_cases()


# ------------------------------------------------------------------ max-pool reference
@pytest.mark.parametrize("name", list(X.POOL_GEOMS))
def test_maxpool_ref_equals_torch_on_tie_free_data(name):
    g = X.POOL_GEOMS[name]
    if name == "wrap":
        g = g._replace(C=4)            # the geometry, not the channel count, is what the reference has to get right
    x = torch.randperm(g.rows_in * g.C, generator=torch.Generator().manual_seed(3)).to(F64).view(g.rows_in, g.C) - 1000.0
    y, idx = X.maxpool_ref(x, g)
    x5 = x.view(g.N, g.D, g.H, g.W, g.C).permute(0, 4, 1, 2, 3)
    ty, ti = F.max_pool3d(x5, g.k, g.s, g.p, return_indices=True)
    assert tuple(ty.shape[2:]) == g.out
    n = torch.arange(g.N).view(-1, 1, 1, 1, 1)
    trow = (ti + n * g.D * g.H * g.W).permute(0, 2, 3, 4, 1).reshape(g.rows_out, g.C)
    assert torch.equal(y, ty.permute(0, 2, 3, 4, 1).reshape(g.rows_out, g.C))
    assert torch.equal(idx.long(), trow)
    # the adjoint pair: <maxpool_bwd(dy), xdot> == <dy, gather(xdot)>
    dy = X.randint64(-3, 3, (g.rows_out, g.C), torch.Generator().manual_seed(4))
    xd = X.randint64(-3, 3, (g.rows_in, g.C), torch.Generator().manual_seed(5))
    assert float((X.maxpool_bwd_ref(dy, idx, g.rows_in) * xd).sum()) == float((dy * X.gather_ref(xd, idx)).sum())


def test_maxpool_ref_takes_the_first_maximum():
    """brute force over one small tie-heavy case: the chosen row holds the maximum and no earlier tap of the window does"""
    g = X.POOL_GEOMS["lopsided"]
    x, _, _ = X.pool_data(g, 0)
    y, idx = X.maxpool_ref(x, g)
    Do, Ho, Wo = g.out
    ties = 0
    for o, c in itertools.product(range(g.rows_out), range(g.C)):
        ow, oh, od = o % Wo, (o // Wo) % Ho, (o // (Wo * Ho)) % Do
        n = o // (Wo * Ho * Do)
        best, arg, seen = None, -1, 0
        for a, b, e in itertools.product(range(g.k[0]), range(g.k[1]), range(g.k[2])):
            d, h, w = od * g.s[0] - g.p[0] + a, oh * g.s[1] - g.p[1] + b, ow * g.s[2] - g.p[2] + e
            if not (0 <= d < g.D and 0 <= h < g.H and 0 <= w < g.W):
                continue
            row = ((n * g.D + d) * g.H + h) * g.W + w
            v = float(x[row, c])
            if best is None or v > best:
                best, arg, seen = v, row, 1
            elif v == best:
                seen += 1
        ties += seen > 1
        assert float(y[o, c]) == best and int(idx[o, c]) == arg, (o, c)
    assert ties > g.rows_out * g.C // 2


# ------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("key", list(POOL_CASES), ids=lambda k: f"{k[0]}-c{k[1]}")
def test_pool_data_has_ties_and_shared_and_unchosen_rows(key):
    g = POOL_CASES[key]
    x, dy, xd = X.pool_data(g, 0)
    y, idx = X.maxpool_ref(x, g)
    rows, valid = X.pool_taps(g, "cpu")
    at_max = ((x[rows] == y) & valid.unsqueeze(-1)).sum(0)              # taps of each window that hold its maximum
    assert int((at_max >= 2).sum()) >= g.rows_out * g.C // 8, "too few tied maxima"      # (a 2 x 2 window over seven values ties in ~ 1 of 5)
    # a tie whose first and last maximum are different rows: `>=` in the scan would change idx
    last = torch.zeros_like(idx.long())
    for t in range(rows.shape[0]):
        hit = (x[rows[t]] == y) & valid[t].unsqueeze(-1)
        last = torch.where(hit, rows[t].unsqueeze(-1), last)
    assert int((last != idx.long()).sum()) > 0
    n = X.selection_counts(idx, g.rows_in)
    assert int((n == 0).sum()) > 0
    dx = X.maxpool_bwd_ref(dy, idx, g.rows_in)
    if any(k > s for k, s in zip(g.k, g.s)):          # overlapping windows (the 2 x 2 / 2 pools of VGG share no input element)
        assert int((n >= 2).sum()) > 0
        assert int(((n >= 2) & (dx != 0)).sum()) > 0, "the gradients that meet in one input element are all zero"
    else:
        assert int(n.max()) == 1
    assert bool((dy.abs() <= 3).all()) and int(n.max()) <= 27 and float(dx.abs().max()) <= 81     # exact in bf16


def test_l1_pair_data_has_all_three_signs():
    for M, C in ((300, 12), (16400, 12)):
        a, b = X.l1_pair_data(M, C, 0)
        n = a.numel()
        assert n // 4 < int((a == b).sum()) < n // 2
        assert int((a > b).sum()) > n // 5 and int((a < b).sum()) > n // 5
        assert float((a - b).abs().sum()) < 2 ** 24 / 2 ** 4


@pytest.mark.parametrize("case", [c for c in X.GN_CASES + [X.GN_SHIFTED] if c.act != _lib.ACT_NONE], ids=lambda c: c.name)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_relu_mask_of_the_tangent_cases_is_balanced(case, dt):
    d = X.gn_inputs(case, X.DTYPES[dt][1])
    frac = float((d["y"] > 0).to(F64).mean())
    assert 0.25 <= frac <= 0.75, frac


# ------------------------------------------------------------------ tangent references
@pytest.mark.parametrize("case", X.GN_CASES, ids=lambda c: c.name)
def test_restated_closed_forms_agree_with_float64_autograd(case):
    d = X.gn_inputs(case, torch.float32)
    args = (d["x"], d["xdot"], d["q"], d["gamma"], case.G, case.act, d["y"], d["resdot"])
    ref, f32 = X.gn_jvp_ref(*args), X.gn_jvp_f32_restated(*args)
    for k, r in ref.items():
        if r is None:
            assert f32[k] is None
            continue
        assert f32[k].dtype == torch.float32 and f32[k].shape == r.shape, k
        assert X.rel_err(f32[k], r) <= 1e-6, (k, X.rel_err(f32[k], r))


def test_closed_forms_are_exact_in_float64():
    """the same formulas evaluated in float64 equal autograd to rounding: the kernel's comment states the right derivative, constants
    included"""
    case = X.GN_CASES[2]
    d = X.gn_inputs(case, torch.float32)
    args = (d["x"], d["xdot"], d["q"], d["gamma"], case.G, case.act, d["y"], d["resdot"])
    ref = X.gn_jvp_ref(*args)
    f64 = X.gn_jvp_f32_restated(*args, dtype=F64)
    for k, r in ref.items():
        assert X.rel_err(f64[k], r) <= 1e-13, (k, X.rel_err(f64[k], r))


# ------------------------------------------------------------------ argument rejection (no HIP call is reached)
A0 = 0x10000             # a 16-byte aligned dummy address; nothing is dereferenced before the checks


def rejected(rc, *phrases):
    msg = _lib.lib().ipoke_last_error() or b""
    assert rc != 0, "accepted"
    for p in phrases:
        assert p.encode() in msg, (p, msg)


def jvp_fwd_args(dtype=_lib.F32, **kw):
    a = dict(x=A0, ldx=24, xdot=A0, ldxd=24, y=A0, ldy=24, resdot=A0, ldres=24, ydot=A0, ldyd=24, gamma=A0, N=2, S=5, C=16, G=4,
             act=_lib.ACT_RELU, eps=1e-5, ws=A0, dtype=dtype, stream=None)
    a.update(kw)
    return [a[k] for k in ("x", "ldx", "xdot", "ldxd", "y", "ldy", "resdot", "ldres", "ydot", "ldyd", "gamma", "N", "S", "C", "G", "act", "eps",
                           "ws", "dtype", "stream")]


def jvp_bwd_args(dtype=_lib.F32, **kw):
    a = dict(x=A0, ldx=24, xdot=A0, ldxd=24, y=A0, ldy=24, q=A0, ldq=24, dxdot=A0, lddxd=24, dx=A0, lddx=24, dresdot=A0, lddres=24,
             dgamma=A0, gamma=A0, N=2, S=5, C=16, G=4, act=_lib.ACT_RELU, eps=1e-5, ws=A0, dtype=dtype, stream=None)
    a.update(kw)
    return [a[k] for k in ("x", "ldx", "xdot", "ldxd", "y", "ldy", "q", "ldq", "dxdot", "lddxd", "dx", "lddx", "dresdot", "lddres", "dgamma",
                           "gamma", "N", "S", "C", "G", "act", "eps", "ws", "dtype", "stream")]


@pytest.mark.parametrize("dtype,bad_ld", [(_lib.F32, 22), (_lib.BF16, 20)])
def test_tangent_rejects_every_pitch_that_is_not_16_bytes(dtype, bad_ld):
    lib = _lib.lib()
    for name, field in (("ldx", "a.ldx"), ("ldxd", "a.ldxd"), ("ldy", "a.ldy"), ("ldres", "a.ldres"), ("ldyd", "a.ldyd")):
        rejected(lib.ipoke_groupnorm_jvp(*jvp_fwd_args(dtype, **{name: bad_ld})), "multiples of 16 bytes", field + " %")
    for name, field in (("ldx", "a.ldx"), ("ldxd", "a.ldxd"), ("ldy", "a.ldy"), ("ldq", "a.ldq"), ("lddxd", "a.lddxd"), ("lddx", "a.lddx"),
                        ("lddres", "a.lddresd")):
        rejected(lib.ipoke_groupnorm_jvp_bwd(*jvp_bwd_args(dtype, **{name: bad_ld})), "multiples of 16 bytes", field + " %")


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
def test_tangent_rejects_every_misaligned_base_address(dtype):
    lib = _lib.lib()
    for name in ("x", "xdot", "y", "resdot", "ydot"):
        rejected(lib.ipoke_groupnorm_jvp(*jvp_fwd_args(dtype, **{name: A0 + 8})), "base addresses: multiples of 16 bytes")
    for name in ("x", "xdot", "y", "q", "dxdot", "dx", "dresdot"):
        rejected(lib.ipoke_groupnorm_jvp_bwd(*jvp_bwd_args(dtype, **{name: A0 + 8})), "base addresses: multiples of 16 bytes")


def test_tangent_rejects_bad_groupings():
    lib = _lib.lib()
    for args, call in ((jvp_fwd_args, lib.ipoke_groupnorm_jvp), (jvp_bwd_args, lib.ipoke_groupnorm_jvp_bwd)):
        rejected(call(*args(C=16, G=3)), "bad GroupNorm tangent arguments", "C % G == 0")
        rejected(call(*args(C=2064, G=516, ldx=2064)), "at most 512 groups")
        # cpg = 6 neither divides nor is divided by 4 (fp32) / 8 (bf16)
        rejected(call(*args(_lib.F32, C=24, G=4)), "multiples of 16 bytes", "cpg % e16 == 0 || e16 % cpg == 0")
        rejected(call(*args(_lib.BF16, C=24, G=4)), "multiples of 16 bytes", "cpg % e16 == 0 || e16 % cpg == 0")
        rejected(call(*args(y=None)), "the activation mask needs the primal output")
        rejected(call(*args(C=18, G=2)), "multiples of 16 bytes", "a.C % e16 == 0")


def test_pools_and_colsum_reject_short_pitches():
    lib = _lib.lib()
    g = X.POOL_GEOMS["disc"]
    for dtype in (_lib.F32, _lib.BF16):
        rejected(lib.ipoke_maxpool3d_fwd(g.dims(), A0, g.C, A0, g.C - 1, A0, dtype, None), "row pitches must cover the channel count")
        rejected(lib.ipoke_maxpool3d_fwd(g.dims(), A0, g.C - 1, A0, g.C, A0, dtype, None), "row pitches must cover the channel count")
        rejected(lib.ipoke_maxpool3d_bwd(g.dims(), A0, g.C - 1, A0, A0, g.C, dtype, None), "row pitches must cover the channel count")
        rejected(lib.ipoke_maxpool3d_bwd(g.dims(), A0, g.C, A0, A0, g.C - 1, dtype, None), "row pitches must cover the channel count")
        rejected(lib.ipoke_avgpool_rows(A0, 12, A0, 11, 5, 49, 12, dtype, None), "bad arguments", "ldy >= C")
        rejected(lib.ipoke_avgpool_rows(A0, 11, A0, 12, 5, 49, 12, dtype, None), "bad arguments", "ldx >= C")
        rejected(lib.ipoke_avgpool_rows_bwd(A0, 11, A0, 12, 5, 49, 12, dtype, None), "bad arguments", "ldy >= C")
        rejected(lib.ipoke_avgpool_rows_bwd(A0, 12, A0, 11, 5, 49, 12, dtype, None), "bad arguments", "ldx >= C")
        rejected(lib.ipoke_gather_rows(A0, 12, A0, A0, 11, 7, 12, dtype, None), "bad arguments", "ldy >= C")
        rejected(lib.ipoke_l1_pair(A0, 12, A0, 12, 7, 12, ctypes.c_float(1.0), A0, A0, 11, dtype, None), "bad arguments", "ldg >= C")
    # colsum: the pitch is a multiple of 16 bytes of the SOURCE type and covers the channel count rounded up to it
    phrase = "row pitch must cover the channel count rounded up to 16 bytes"
    rejected(lib.ipoke_colsum(A0, 3, 10, 3, 0, A0, 0, A0, _lib.F32, None), phrase)             # 3 floats: not 16 bytes
    rejected(lib.ipoke_colsum(A0, 4, 10, 5, 0, A0, 0, A0, _lib.F32, None), phrase)             # 4 < round_up(5, 4)
    rejected(lib.ipoke_colsum(A0, 4, 10, 3, 0, A0, 0, A0, _lib.BF16, None), phrase)            # 4 bf16: 8 bytes
    rejected(lib.ipoke_colsum(A0, 8, 10, 9, 0, A0, 0, A0, _lib.BF16, None), phrase)            # 8 < round_up(9, 8)
    rejected(lib.ipoke_colsum(A0, 6, 10, 3, 1, A0, 0, A0, _lib.BF16, None), phrase)            # fp32 source: 6 floats is not 16 bytes
    rejected(lib.ipoke_act_bwd(A0, 16, A0, 16, A0, 12, 7, 12, 16, _lib.ACT_RELU, _lib.F32, None), "bad arguments", "ldo >= Cpad")
    rejected(lib.ipoke_l1_loss(A0, 2, A0, 3, 3, 35, 112, ctypes.c_float(1.0), A0, None, 0, None, None), "bad arguments", "ldy >= C")
