"""The references of tests/flow_exact.py pinned without a GPU (against float64 autograd of the same formula written with torch ops and
against the layers of oracle/flow_ref), the conditions the generated operands must meet for a green GPU test to mean something (every
exact partial sum below 2^24 / 2^8, integer LU inverses, non-involutive permutations, the branch each named case claims to enter), the
recorded fp32 yardsticks, and the two table layouts of the C ABI."""
import ctypes

import pytest
import torch

from ipoke_amd import _lib
from oracle import flow_ref
from tests import flow_exact as X
from tests.flow_exact import F64, SENT, YARDSTICK, err_units, restate

F32 = torch.float32
BF16 = torch.bfloat16


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def integer(t):
    return bool((t == t.round()).all())


# ------------------------------------------------------------------ ABI
def test_table_layouts_match_the_library():
    lib = _lib.lib()
    assert ctypes.sizeof(X.LuJob) == lib.ipoke_lu_job_size() == 80
    assert ctypes.sizeof(X.LsRef) == lib.ipoke_actnorm_logdet_ref_size() == 16
    assert X.LsRef.off.offset == 0 and X.LsRef.C.offset == 8 and X.LuJob.C.offset == 72
    assert "ipoke_actnorm_logdet_ref_size" in _lib.SIGNATURES


# ------------------------------------------------------------------ references against autograd and the oracle
def nchw(s, B, P):
    """state [B*P][C] -> [B][C][8 or P][...]: the oracle's layout with H x W = P x 1"""
    return s.reshape(B, P, -1).permute(0, 2, 1).unsqueeze(-1)


def oracle_actnorm(ls, b):
    m = flow_ref.ActNorm2dFlow(ls.numel()).double()
    with torch.no_grad():
        m.log_scale.copy_(ls.view(-1, 1, 1))
        m.bias.copy_(b.view(-1, 1, 1))
    m.initialized.fill_(1)
    return m


@pytest.mark.parametrize("c", X.ACTNORM_CASES, ids=lambda c: f"C{c.C}")
def test_actnorm_refs_equal_the_oracle_layer_and_autograd(c):
    B, P = 2, 35
    M = B * P
    x = X.real_state(M, c.ld, c.C)
    ls, b, p, ip = X.actnorm_params(c.C, False, c.C)
    m = oracle_actnorm(ls, b)
    xw = x[:, c.c0: c.c0 + c.C].clone().requires_grad_(True)
    y, ld = m(nchw(xw, B, P))
    y = y[:, p]                                                # the Shuffle behind it (flow_ref.Shuffle.forward)
    ref, _ = X.actnorm_fwd_ref(x, c.c0, c.C, ls, b, p)
    close(ref[:, c.c0: c.c0 + c.C], y.squeeze(-1).permute(0, 2, 1).reshape(M, c.C).detach())
    keep = [k for k in range(c.ld) if not c.c0 <= k < c.c0 + c.C]
    assert torch.equal(ref[:, keep], x[:, keep])
    close(ld.detach(), torch.full((B,), X.actnorm_logdet_ref(ls, [(0, c.C)], P), dtype=F64))
    # inverse: Shuffle reverse, then the layer's reverse
    back = m(nchw(ref[:, c.c0: c.c0 + c.C], B, P)[:, ip], reverse=True)
    inv, _ = X.actnorm_inv_ref(ref, c.c0, c.C, ls, b, ip)
    close(inv[:, c.c0: c.c0 + c.C], back.squeeze(-1).permute(0, 2, 1).reshape(M, c.C).detach())
    close(inv, x, 1e-7)                                        # (the +1e-8 of the inverse)
    # backward: autograd of sum(dy * out) + sum_b dld[b] * logdet[b] through the oracle layer
    gen = torch.Generator().manual_seed(5)
    dy, dld = torch.randn((M, c.ld), generator=gen, dtype=F64), torch.randn(B, generator=gen, dtype=F64)
    yst = y.squeeze(-1).permute(0, 2, 1).reshape(M, c.C)
    total = (yst * dy[:, c.c0: c.c0 + c.C]).sum() + (ld * dld).sum()
    gx, gls, gb = torch.autograd.grad(total, [xw, m.log_scale, m.bias])
    dx, part, _ = X.actnorm_bwd_ref(dy, x, c.c0, c.C, ls, p, dld, B, P)
    close(dx[:, c.c0: c.c0 + c.C], gx)
    assert torch.equal(dx[:, keep], dy[:, keep])
    close(part.sum(0)[: c.C], gls.reshape(-1), 1e-11)
    close(part.sum(0)[c.C:], gb.reshape(-1), 1e-11)


def test_actnorm_init_ref_equals_the_oracle_init():
    for M in X.INIT_MS:
        for pre in (False, True):
            x, ls0, b0 = X.actnorm_init_operands(M, pre)
            c = X.INIT_CASE
            m = oracle_actnorm(ls0, b0)
            m.data_init(nchw(x[:, c.c0: c.c0 + c.C], 1, M))
            ls, b = X.actnorm_init_ref(x, c.c0, c.C, ls0, b0)
            close(ls, m.log_scale.detach().reshape(-1), 1e-9)
            close(b, m.bias.detach().reshape(-1), 1e-9)
            assert float(x[:, c.c0].mean()) > 990 and bool((x[:, : c.c0] == SENT).all()) and bool((x[:, c.c0 + c.C:] == SENT).all())
            # channel 1: a spread small enough that the + 1e-6 on the std moves log_scale by far more than the GPU bound of its unit
            std = float(x[:, c.c0 + 1].std())
            if not pre:
                unit = float(X.ulp_of(X.actnorm_init_mags(x, c.c0, c.C, ls0, b0)[0][1], F32))
                assert std < 1e-2 and 1e-6 / (std + 1e-6) > 10 * X.gpu_bound("actnorm_init") * unit


@pytest.mark.parametrize("c", X.AFFINE_CASES, ids=lambda c: c.name)
def test_affine_refs_equal_the_oracle_and_autograd(c):
    o = X.affine_operands(c, False)
    B, P, Cp = c.B, c.P, c.Cp
    M = B * P
    raw = X.raw_sum(o["parts"], o["bias"])
    close(raw, sum(o["parts"][u] for u in range(c.nsplit)) + (0 if o["bias"] is None else o["bias"]))
    cols = X.tcols(Cp, c.t_off, c.t_stride)
    xt = o["x"][:, cols].clone().requires_grad_(True)
    rw = raw.clone().requires_grad_(True)
    mu, sc = flow_ref.affine_params(nchw(rw, B, P))
    y, ld = flow_ref.affine_fwd(nchw(xt, B, P), mu, sc)
    Q = X.aff_q(c)
    ref, rsc, slots, _, _ = X.affine_fwd_ref(o["x"], raw, c.t_off, c.t_stride, B, Q)
    flat = lambda t: t.squeeze(-1).permute(0, 2, 1).reshape(M, -1)          # noqa: E731
    close(ref[:, cols], flat(y).detach())
    close(rsc, flat(sc).detach())
    close(slots.sum(1), ld.detach(), 1e-11)
    keep = torch.ones(ref.shape[1], dtype=torch.bool)
    keep[cols] = False
    assert torch.equal(ref[:, keep], o["x"][:, keep])
    inv, _ = X.affine_inv_ref(ref, raw, c.t_off, c.t_stride)
    close(inv[:, cols], flat(flow_ref.affine_inv(y, mu, sc)).detach())
    close(inv, o["x"], 1e-9)
    # backward through autograd: sum(dy * y) + sum_b dld[b] * logdet[b]
    gen = torch.Generator().manual_seed(9)
    dy, dld = torch.randn(ref.shape, generator=gen, dtype=F64), torch.randn(B, generator=gen, dtype=F64)
    gx, graw = torch.autograd.grad((flat(y) * dy[:, cols]).sum() + (ld * dld).sum(), [xt, rw])
    r = X.affine_bwd_ref(dy, o["x"], rsc, dld, c.t_off, c.t_stride, B, P)
    close(r["dx"][:, cols], gx)
    assert torch.equal(r["dx"][:, keep], dy[:, keep])
    close(r["dparams"], graw, 1e-11)
    close(r["dbias"].sum(0), graw.sum(0), 1e-11)


def test_loss_ref_equals_the_oracle_loss_and_autograd():
    for (B, P, C, ld), w in zip(X.NLL_CASES, (1.0, 0.25, 1.0, 0.25, 1.0)):
        z, logdet = X.nll_operands(B, P, C)
        zz, ll = z.clone().requires_grad_(True), logdet.clone().requires_grad_(True)
        loss, d = flow_ref.FlowLoss(logdet_weight=w)(nchw(zz, B, P), ll)
        sc, dout, dld = X.flow_nll_ref(z, logdet, w, B)
        close(sc, torch.stack([loss, d["nll_loss"], d["nlogdet_loss"]]).detach())
        gz, gl = torch.autograd.grad(loss, [zz, ll])
        close(dout, gz)
        close(dld, gl)


def test_logdet_refs():
    s = X.randint64(-3, 3, (7, 5, 4), torch.Generator().manual_seed(7))
    expect = torch.tensor([sum(float(s[l, b, k]) for l in range(7) for k in range(4)) + 9.5 for b in range(5)], dtype=F64)
    assert torch.equal(X.logdet_finalize_ref(s, 2.5, 7.0), expect)
    assert X.logdet_finalize_ref(torch.zeros(0, 3, 4, dtype=F64), 2.5).tolist() == [2.5] * 3
    for n in X.LOGDET_NS:
        params, refs = X.actnorm_logdet_operands(n)
        spans = sorted(refs)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:])), "layers overlap"
        inside = torch.zeros(params.numel(), dtype=torch.bool)
        for o, c in refs:
            inside[o: o + c] = True
        assert bool((params[~inside] == SENT).all()) and bool((params[inside].abs() <= 3).all())
        assert X.actnorm_logdet_ref(params, refs, 64) == 64.0 * float(params[inside].sum())


@pytest.mark.parametrize("C", X.LU_CS)
def test_lu_refs_equal_the_oracle_layer_and_autograd(C):
    m = X.lu_operands(C, False)
    r = X.lu_prepare_ref(m)
    lay = flow_ref.InvertibleConvLU1d.__new__(flow_ref.InvertibleConvLU1d)
    torch.nn.Module.__init__(lay)
    lay.nf = C
    for k, name in (("perm", "permutated"), ("sign", "sign_s"), ("lmask", "lmask"), ("umask", "umask"), ("eye", "eye")):
        lay.register_buffer(name, m[k].clone())
    lay.l, lay.u, lay.log_s = (torch.nn.Parameter(m[k].clone()) for k in ("l", "u", "log_s"))
    wl, wu = lay.matrices()
    close(r["wl"], wl.detach())
    close(r["wu"], wu.detach())
    close(r["W"], (lay.permutated @ (wl @ wu)).detach())
    close(r["Winv"], (torch.inverse(wu) @ (torch.inverse(wl) @ torch.inverse(lay.permutated))).detach(), 1e-10)
    B, P8, ld = 2, 6, C + 2
    dy, x, dld = X.lu_wgrad_operands(B, P8, C, ld)
    y, logdet = lay(nchw(x[:, :C], B, P8))
    close(X.lu_apply_ref(x, C, r["W"], 0)[:, :C], y.squeeze(-1).permute(0, 2, 1).reshape(B * P8, C).detach(), 1e-11)
    assert torch.equal(X.lu_apply_ref(x, C, r["W"], 0)[:, C:], x[:, C:])
    close(X.lu_apply_ref(x, C, r["W"], 1)[:, :C], x[:, :C] @ r["W"], 1e-11)
    back = lay(y, reverse=True)
    close(X.lu_apply_ref(X.lu_apply_ref(x, C, r["W"], 0), C, r["Winv"], 0), x, 1e-9)
    close(back.squeeze(-1).permute(0, 2, 1).reshape(B * P8, C).detach(), x[:, :C], 1e-9)
    total = (y.squeeze(-1).permute(0, 2, 1).reshape(B * P8, C) * dy[:, :C]).sum() + (logdet.double() * dld).sum()
    gl, gu, gs = torch.autograd.grad(total, [lay.l, lay.u, lay.log_s])
    dl, du, dls = X.lu_wgrad_ref(dy[:, :C], x[:, :C], m, r["wl"], r["wu"], dld, P8)
    close(dl, gl, 1e-11)
    close(du, gu, 1e-11)
    close(dls, gs, 1e-11)


def test_layout_refs():
    x = X.randint64(-9, 9, (3, 5, 48), torch.Generator().manual_seed(1))
    s = X.nchw_to_state_ref(x)
    assert float(s[1 * 48 + 7, 3]) == float(x[1, 3, 7])
    assert torch.equal(X.state_to_nchw_ref(s, 3, 5, 48), x)
    assert torch.equal(X.extract_cols_ref(s, 1, 2, 2), torch.stack([s[:, 1], s[:, 3]], 1))
    assert torch.equal(X.cond_prepare_ref(x, _lib.ACT_RELU), X.nchw_to_state_ref(x.clamp(min=0)))


# ------------------------------------------------------------------ input conditions
LIM24, LIM8 = 2.0 ** 24, 2.0 ** 8


def test_permutations_are_neither_identity_nor_involutions():
    for C in (3, 5, 8, 33, 60, 64, 256):
        for seed in (C, 3, 7 + C):
            p = X.perm(C, seed)
            ar = torch.arange(C)
            assert sorted(p.tolist()) == ar.tolist() and not torch.equal(p, ar) and not torch.equal(p[p], ar)
            assert not torch.equal(torch.argsort(p), p)            # idx where inv_idx belongs changes the result


def test_exact_actnorm_operands():
    e = X.ACTNORM_EXT_BF16_C1                                     # the one-channel layer again, in a state wide enough for a bf16 ext
    assert (e.C, e.c0) == (X.ACTNORM_CASES[0].C, X.ACTNORM_CASES[0].c0) == (1, 0)
    assert X.round_up(1, 8) + 1 - 1 <= e.ld and X.round_up(1, 8) - 1 > X.ACTNORM_CASES[0].ld
    for c in X.ACTNORM_CASES + [e]:
        ls, b, p, ip = X.actnorm_params(c.C, True, c.C)
        x = X.int_state(X.ACTNORM_M, c.ld, c.C)
        assert integer(x) and integer(b) and bool((ls == 0).all()) and float(x.abs().max()) + float(b.abs().max()) < LIM8
        assert float(torch.exp(torch.zeros(1, dtype=F32)) + torch.tensor(1e-8, dtype=F32)) == 1.0
        for e_off, e_stride, e_C in X.ext_variants(c):
            assert e_C >= 1 and e_off + (e_C - 1) * e_stride < c.ld
    for c in X.ACTNORM_BWD_CASES:
        o = X.actnorm_bwd_operands(c, True)
        _, part, mag = X.actnorm_bwd_ref(o["dy"], o["x"], c.c0, c.C, torch.zeros(c.C, dtype=F64), o["idx"], o["dld"], c.B, c.P)
        assert float(mag.max()) < LIM24 and integer(part * 8) and integer(o["dld"] * 8)
        assert bool((o["dld"] != 0).all()), "a zero dld[b] hides the P dld[b] term of d log_scale"
        rows_par = 1024 // c.C
        assert 1 <= c.C <= 256 and c.c0 + c.C <= c.ld
        if c.name == "c3-idle":
            assert 1024 % c.C != 0 and rows_par > c.P
        if c.name == "c60":
            assert c.P % rows_par != 0 and 1024 - rows_par * c.C == 4
        if c.name == "c64-p20":
            assert c.P % rows_par != 0
        if c.name in ("c1", "c3-idle"):
            assert rows_par > c.P
        if c.name.startswith("c256"):
            assert c.C == 256 and rows_par == 4
    assert [c.name for c in X.ACTNORM_BWD_CASES if not c.params] == ["no-params"]


def test_exact_affine_operands_and_branches():
    for c in X.AFFINE_CASES:
        o = X.affine_operands(c, True)
        assert integer(o["parts"]) and integer(o["x"])
        raw = X.raw_sum(o["parts"], o["bias"])
        assert bool((raw[:, c.Cp:] == 0).all()), "s != 0"
        mag = o["parts"].abs().sum(0) + (0 if o["bias"] is None else o["bias"].abs())
        assert float(mag.max()) < LIM24
        y = X.affine_fwd_ref(o["x"], raw, c.t_off, c.t_stride, c.B, X.aff_q(c))
        assert float(y[3].max()) < LIM8 and bool((y[1] == 1).all()) and bool((y[2] == 0).all())      # ext in bf16; scale 1; log-det 0
        assert c.t_off + (c.Cp - 1) * c.t_stride < X.aff_ld(c)
        if c.nsplit > 1:
            assert bool((o["parts"][:, :, c.Cp:] != 0).any()), "the s partials are all zero"
    by = {c.name: c for c in X.AFFINE_CASES}
    rc = lambda c, inv=False: (c.P // X.aff_q(c, inv)) * c.Cp                                       # noqa: E731
    assert {c.nsplit for c in X.AFFINE_CASES} >= {1, 4, 32, 35} and {c.Cp for c in X.AFFINE_CASES} >= {1, 4, 30, 32}
    assert {(c.t_off // max(c.Cp, 1) if c.t_stride == 1 else c.t_off, c.t_stride) for c in X.AFFINE_CASES} >= {(0, 1), (1, 1), (0, 2), (1, 2)}
    for n in ("cp32-odd-q1", "cp30-35"):
        assert by[n].nsplit > 32                                                                    # the tail loop of affine_stage_raw
    assert by["cp32-odd-q1"].bias and not by["cp30-35"].bias
    assert all(c.raw_pad > 0 for c in X.AFFINE_CASES if c.name not in ("cp1", "cp32-noslot"))      # ldraw > 2 Cp
    for n in ("cp30-even-q1", "cp32-odd-q1"):
        assert X.aff_q(by[n]) == 1 and rc(by[n]) > 512                                              # forward: direct loads
    assert by["cp32-odd-q1"].Cp == 32
    assert X.aff_q(by["cp32-noslot"]) == 4 and rc(by["cp32-noslot"]) == 512                         # exactly the prefetch window
    assert X.aff_q(by["cp4-p50"]) == 1 and by["cp4-p50"].P % 4 != 0 and by["cp4-p50"].slot == 4     # Q = 1 through P % 4
    assert X.aff_q(by["cp30-p50"], True) == 1 and rc(by["cp30-p50"], True) > 512                    # inverse: direct loads
    assert all(rc(c, True) <= 512 for c in X.AFFINE_CASES if c.P % 4 == 0)
    for c in X.AFFINE_BWD_CASES:
        o = X.affine_bwd_operands(c, True)
        r = X.affine_bwd_ref(o["dy"], o["x"], o["scale"], o["dld"], c.t_off, c.t_stride, c.B, c.P)
        assert float(r["mag_dbias"].max()) < LIM24 and bool((o["dld"] != 0).all())
        dp = r["dparams"]
        assert integer(dp * 8) and float((dp * 8).abs().max()) <= LIM8, "dparams not exact in bf16"
        assert torch.equal(dp.to(BF16).to(F64), dp)
        assert c.t_off + (c.Cp - 1) * c.t_stride < X.affbwd_ld(c)
    by = {c.name: c for c in X.AFFINE_BWD_CASES}
    assert 1024 % by["cp48"].Cp != 0 and 1024 // 48 == 21
    assert 1024 // by["cp30-p20"].Cp > by["cp30-p20"].P and 1024 // by["cp4-p20"].Cp > by["cp4-p20"].P
    assert by["cp4-p20"].ldp_pad == 0 and by["cp48"].ldp_pad > 0 and not by["cp4-p20"].dbias


def test_exact_loss_and_logdet_operands():
    for B, P, C, ld in X.NLL_CASES:
        z, logdet = X.nll_operands(B, P, C)
        assert integer(z) and integer(logdet) and float((z * z).sum()) < LIM24 and float(logdet.abs().sum()) < LIM24
    # the branch each case of flow_nll_kernel enters, from the case tuples (buffers are 16-byte aligned unless shifted by one float)
    runs = [c + (0,) for c in X.NLL_CASES] + [c + (1,) for c in X.NLL_SHIFTED]
    assert all(c in X.NLL_CASES and c[3] % 4 == 0 for c in X.NLL_SHIFTED)                   # shifted: vector-eligible but for the address
    vector = [r for r in runs if r[3] % 4 == 0 and r[4] == 0]
    scalar = [r for r in runs if r[3] % 4 != 0 or r[4] != 0]
    assert any(C == ld for _, _, C, ld, _ in vector) and any(C < ld for _, _, C, ld, _ in vector)      # masked padding columns: both paths
    assert any(C == ld for _, _, C, ld, _ in scalar) and any(C < ld for _, _, C, ld, _ in scalar)
    assert any(ld % 4 != 0 for _, _, _, ld, _ in scalar) and any(sh for _, _, _, _, sh in scalar)
    assert any(B > X.NLL_BLOCK for B, _, _, _, _ in runs)             # more samples than one pass of the log-det loop
    assert any(B & (B - 1) for B, _, _, _, _ in runs) and any(not B & (B - 1) for B, _, _, _, _ in runs)
    for nslots, slot_w, B in X.FINALIZE_CASES:
        assert nslots * slot_w * 3 < LIM24
    assert any(n * w > 256 for n, w, _ in X.FINALIZE_CASES) and any(n == 0 for n, _, _ in X.FINALIZE_CASES)
    for n in X.LOGDET_NS:
        params, refs = X.actnorm_logdet_operands(n)
        assert sum(c for _, c in refs) * 3 * 64 < 2.0 ** 31 and sum(c for _, c in refs) * 3 < LIM24    # the sum, and the sum x 64
        assert n % (8 * 1024 // 64) != 0
        wide = [(o, c) for o, c in refs if c > 64]
        assert wide and all(float(params[o + 64]) != 0 for o, c in wide)    # the loop over the channels >= 64 runs, and its first one counts
    assert {c for _, c in X.actnorm_logdet_operands(515)[1]} == set(X.LOGDET_WIDTHS)


def test_exact_lu_operands():
    for C in X.LU_CS:
        m = X.lu_operands(C, True)
        r = X.lu_prepare_ref(m)
        for k in ("wl", "wu", "W", "Winv", "wli", "wui"):
            assert integer(r[k]) and float(r[k].abs().max()) < LIM24, k
        # every partial sum of the products and of the substitutions
        for a, b in ((r["wl"], r["wu"]), (r["wl"], r["wli"]), (r["wu"], r["wui"]), (r["wui"], r["wli"])):
            assert float((a.abs() @ b.abs()).max()) < LIM24
        assert torch.equal(r["W"] @ r["Winv"], torch.eye(C, dtype=F64))
        assert torch.equal(r["wl"] @ r["wli"], torch.eye(C, dtype=F64)) and torch.equal(r["wu"] @ r["wui"], torch.eye(C, dtype=F64))
        assert bool((m["log_s"] == 0).all()) and bool((m["sign"].abs() == 1).all())
        if C >= 3:
            assert not torch.equal(m["p"][m["p"]], torch.arange(C))
            assert bool(((m["l"] * (1 - m["lmask"])) != 0).any()) and bool(((m["u"] * (1 - m["umask"])) != 0).any())    # the masks matter
        if C >= 5:
            assert int((r["wl"] != 0).sum()) > C and int((torch.triu(r["wu"], 1) != 0).sum()) > 0
            assert not torch.equal(r["W"], r["W"].t())
    for M, C, ld in X.LU_APPLY_CASES:
        x, mat = X.lu_apply_operands(M, C, ld)
        assert float((x[:, :C].abs() @ mat.abs().t()).max()) < LIM24 and (C == 1 or not torch.equal(mat, mat.t()))
    assert [M % 64 for M, _, _ in X.LU_APPLY_CASES] == [0, 36, 0, 1] and any(ld > C for _, C, ld in X.LU_APPLY_CASES)
    for B, P8, C, ld in X.LU_WGRAD_CASES:
        dy, x, dld = X.lu_wgrad_operands(B, P8, C, ld)
        m = X.lu_operands(C, True)
        r = X.lu_prepare_ref(m)
        dW = dy[:, :C].abs().t() @ x[:, :C].abs()
        assert float((dW @ r["wu"].abs().t()).max()) < LIM24 and float((r["wl"].abs().t() @ dW).max()) < LIM24 and integer(dld * 8)
    assert [(C * C) % 256 for _, _, C, _ in X.LU_WGRAD_CASES] == [0, 25, 65, 64]
    assert [(B * P8) % 64 for B, P8, _, _ in X.LU_WGRAD_CASES] == [0, 0, 48, 16]


# ------------------------------------------------------------------ the fp32 yardsticks
def measured():
    """worst error of the fp32 restatement per output, in the unit of flow_exact's table, on the operands of the GPU tests"""
    w = {k: 0.0 for k in YARDSTICK}

    def up(key, got, ref, mag, tdt=F32):
        w[key] = max(w[key], err_units(got.to(tdt) if tdt == BF16 else got, ref, mag, tdt))

    for c in X.ACTNORM_CASES + [X.ACTNORM_EXT_BF16_C1]:
        for with_idx in (True, False):
            x = X.real_state(X.ACTNORM_M, c.ld, c.C)
            ls, b, p, ip = X.actnorm_params(c.C, False, c.C)
            if not with_idx:
                p = ip = None
            ref, mag = X.actnorm_fwd_ref(x, c.c0, c.C, ls, b, p)
            sl = slice(c.c0, c.c0 + c.C)
            up("actnorm_fwd", restate(X.actnorm_fwd_ref, x, c.c0, c.C, ls, b, p)[0][:, sl], ref[:, sl], mag)
            y = X.f32r(ref)
            ref, mag = X.actnorm_inv_ref(y, c.c0, c.C, ls, b, ip)
            got = restate(X.actnorm_inv_ref, y, c.c0, c.C, ls, b, ip)[0]
            up("actnorm_inv", got[:, sl], ref[:, sl], mag)
            up("actnorm_inv_ext_bf16", got[:, sl], ref[:, sl], mag, BF16)
    for c in X.ACTNORM_BWD_CASES:
        if c.params:
            o = X.actnorm_bwd_operands(c, False)
            args = (o["dy"], o["x"], c.c0, c.C, o["ls"], o["idx"], o["dld"], c.B, c.P)
            dx, part, mag = X.actnorm_bwd_ref(*args)
            gdx, gpart, _ = restate(X.actnorm_bwd_ref, *args)
            sl = slice(c.c0, c.c0 + c.C)
            up("actnorm_bwd_dx", gdx[:, sl], dx[:, sl], dx[:, sl].abs())
            up("actnorm_bwd_part", gpart, part, mag)
    for M in X.INIT_MS:
        for pre in (False, True):
            x, ls0, b0 = X.actnorm_init_operands(M, pre)
            c = X.INIT_CASE
            ref, got = X.actnorm_init_ref(x, c.c0, c.C, ls0, b0), restate(X.actnorm_init_ref, x, c.c0, c.C, ls0, b0)
            mags = X.actnorm_init_mags(x, c.c0, c.C, ls0, b0)
            up("actnorm_init", got[0], ref[0], mags[0])
            up("actnorm_init", got[1], ref[1], mags[1])
    for c in X.AFFINE_CASES:
        o = X.affine_operands(c, False)
        raw = X.raw_sum(o["parts"], o["bias"])
        cols = X.tcols(c.Cp, c.t_off, c.t_stride)
        Q = X.aff_q(c)
        ref, rsc, rsl, mag, smag = X.affine_fwd_ref(o["x"], raw, c.t_off, c.t_stride, c.B, Q)
        g32 = restate(X.raw_sum, o["parts"], o["bias"]).to(F64)           # the fp32 sum of the partials, as the kernel forms raw
        assert torch.equal(g32, raw) and float((o["parts"].abs().sum(0) * 1024).max()) < LIM24 and integer(o["parts"] * 1024)
        got = restate(X.affine_fwd_ref, o["x"], g32, c.t_off, c.t_stride, c.B, Q)
        up("affine_fwd", got[0][:, cols], ref[:, cols], mag)
        up("affine_ext_bf16", got[0][:, cols], ref[:, cols], mag, BF16)
        up("affine_scale", got[1], rsc, torch.tanh(0.5 * raw[:, c.Cp:]).abs() + 1.0)
        up("logdet_slot", got[2], rsl, smag)
        y = X.f32r(ref)
        ref, mag = X.affine_inv_ref(y, raw, c.t_off, c.t_stride)
        got = restate(X.affine_inv_ref, y, g32, c.t_off, c.t_stride)[0]
        up("affine_inv", got[:, cols], ref[:, cols], mag)
        up("affine_ext_bf16", got[:, cols], ref[:, cols], mag, BF16)
    for c in X.AFFINE_BWD_CASES:
        o = X.affine_bwd_operands(c, False)
        args = (o["dy"], o["x"], o["scale"], o["dld"], c.t_off, c.t_stride, c.B, c.P)
        r, g = X.affine_bwd_ref(*args), restate(X.affine_bwd_ref, *args)
        cols = X.tcols(c.Cp, c.t_off, c.t_stride)
        up("affine_bwd_dx", g["dx"][:, cols], r["dx"][:, cols], r["dx"][:, cols].abs())
        up("affine_bwd_dparams", g["dparams"], r["dparams"], r["mag_dparams"])
        up("affine_bwd_dparams_bf16", g["dparams"], r["dparams"], r["mag_dparams"], BF16)
        up("affine_bwd_dbias", g["dbias"], r["dbias"], r["mag_dbias"])
    for B, P, C, ld in X.NLL_CASES:
        if B & (B - 1):
            z, logdet = X.nll_operands(B, P, C)
            for wt in (1.0, 0.25):
                rs, rd, rl = X.flow_nll_ref(z, logdet, wt, B)
                gs, gd, gl = restate(X.flow_nll_ref, z, logdet, wt, B)
                up("nll_scalars", gs, rs, torch.stack([rs[1].abs() + wt * rs[2].abs(), rs[1].abs(), rs[2].abs()]))
                up("nll_dout", gd, rd, rd)
                up("nll_dout", gl, rl, rl)
    for C in X.LU_CS:
        m = {k: (X.f32r(v) if v.dtype == F64 else v) for k, v in X.lu_operands(C, False).items()}
        r = X.lu_prepare_ref(m)
        g = X.lu_prepare_ref({k: (v.to(F32) if v.dtype == F64 else v) for k, v in m.items()})
        for k, key, mag in (("wl", "lu_wl_wu", r["wl"]), ("wu", "lu_wl_wu", r["wu"]), ("W", "lu_W", r["mag_W"]), ("Winv", "lu_Winv", r["mag_Winv"])):
            nz = mag != 0
            assert bool((g[k][~nz] == 0).all())
            up(key, g[k][nz], r[k][nz], mag[nz])
    return w


def test_fp32_restatements_stay_within_the_recorded_yardsticks():
    w = measured()
    for k in sorted(w):
        print(f"yardstick {k:26s} measured {w[k]:7.3f}  recorded {YARDSTICK[k]:5.2f}  GPU bound {X.gpu_bound(k):5.1f}")
    over = {k: (v, YARDSTICK[k]) for k, v in w.items() if not v <= YARDSTICK[k]}
    assert not over, f"(measured, recorded) {over}"
    # the recorded values are the measured ones rounded up, not padded: at most twice the measurement or half a unit above it
    slack = {k: (v, YARDSTICK[k]) for k, v in w.items() if YARDSTICK[k] > max(2.0 * v, v + 0.5)}
    assert not slack, f"recorded yardsticks far above the measurement (measured, recorded) {slack}"
