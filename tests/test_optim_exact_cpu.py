"""The checker of tests/test_optim_exact_gpu.py, checked without a GPU: the table mirrors against the library's own sizes, the fmaf
emulation against exact rational arithmetic, the Adam emulation against torch.optim.Adam, the reference layouts and weight-norm formulas
against naive loops, and the mistakes the exact comparator exists to catch (mutants of the update, the rounding, the layout, the range
and the weight-norm backward)."""
import ctypes
import math
import random
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

from ipoke_amd import _lib
from tests import helpers
from tests import optim_exact as X

F64 = torch.float64


# ------------------------------------------------------------------ tables
def test_table_mirrors_match_the_library():
    lib = _lib.lib()
    for cls, fn in X.TABLE_SIZES.items():
        assert ctypes.sizeof(cls) == getattr(lib, fn)(), cls.__name__


def test_relayout_table_numbers_blocks_like_the_engine():
    jobs = [X.relayout_job(0, 54, 6, 6, 40, 9, -1, 0, 48, 32, 4096, 16, 64, 9, 1),
            X.relayout_job(100, 70, 1, 1, 130, 70, 0, 9000, 130, 72, -1, 0, 0, 0)]
    jobs, nb, bj = X.relayout_table(jobs)
    # job 0: n_ext = max(48, 64) = 64 -> 2 tiles of 32, k_ext = max(32, 16) = 32 -> 1; job 1: n_ext 130 -> 3 tiles of 64, k 72 -> 2
    assert [j.block_start for j in jobs] == [0, 2] and nb == 2 + 6 and bj == [0, 0] + [1] * 6
    assert [j.tiles_k for j in jobs] == [1, 2] and [j.tile for j in jobs] == [32, 64]


# ------------------------------------------------------------------ fmaf
def _f32_bits(x):
    return struct.unpack("<f", struct.pack("<I", x))[0]


def _round_f32(q):
    """Fraction -> nearest float32 value (ties to even), subnormals included; operands stay far from overflow"""
    if q == 0:
        return 0.0
    s = -1 if q < 0 else 1
    a = abs(q)
    e = math.floor(math.log2(a.numerator) - math.log2(a.denominator))
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = a / quantum
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return s * float(fl * quantum)


def _fma_triples():
    rnd = random.Random(7)
    out = []
    for _ in range(8000):                                        # random values over a wide exponent range, mixed signs
        a, b, c = (rnd.choice((-1, 1)) * rnd.uniform(1, 2) * 2.0 ** rnd.randint(-40, 40) for _ in range(3))
        out.append((a, b, c))
    for _ in range(1000):                                        # cancellation: c close to -a * b
        a, b = rnd.uniform(-4, 4), rnd.uniform(-4, 4)
        out.append((a, b, -X.f32(a * b) * (1 + rnd.choice((0.0, 2.0 ** -23, -2.0 ** -22)))))
    for _ in range(600):                                         # the product on a float32 midpoint, c perturbs it below double precision
        k = rnd.randint(1, 4000)
        a = 1.0 + k * 2.0 ** -12
        e = rnd.randint(-30, 30)
        sg = rnd.choice((-1.0, 1.0))
        out.append((sg * a * 2.0 ** e, a, rnd.choice((-1.0, 1.0)) * 2.0 ** (e - 70)))
    for _ in range(600):                                         # c on the grid, the product half an ulp minus a quarter double ulp
        e = rnd.randint(-20, 20)
        c = rnd.uniform(1, 2) * 2.0 ** e
        out.append((rnd.choice((-1, 1)) * (1 + 2.0 ** -15) * 2.0 ** (e - 24), 1 - 2.0 ** -15, c))
    for _ in range(1000):                                        # denormal products, addends and results
        a = rnd.uniform(-2, 2) * 2.0 ** rnd.randint(-90, -60)
        b = rnd.uniform(-2, 2) * 2.0 ** rnd.randint(-90, -60)
        c = rnd.choice((0.0, rnd.uniform(-2, 2) * 2.0 ** rnd.randint(-149, -126), rnd.uniform(-2, 2) * 2.0 ** -120))
        out.append((a, b, c))
    for _ in range(200):                                         # subnormal bit patterns directly
        out.append((_f32_bits(rnd.randint(1, 0x7FFFFF)), rnd.uniform(-3, 3), _f32_bits(rnd.randint(1, 0x7FFFFF)) * rnd.choice((-1, 1))))
    return [tuple(X.f32(x) for x in t) for t in out]


def test_fmaf_emulation_matches_exact_rational_arithmetic():
    triples = _fma_triples()
    assert len(triples) >= 10_000
    a, b, c = (torch.tensor([t[i] for t in triples], dtype=F64) for i in range(3))
    got = X.fma32(a, b, c)
    expect = torch.tensor([_round_f32(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in triples], dtype=F64)
    X.assert_same(got.float(), expect.float(), "fmaf emulation")
    # the construction does reach the corrected case, where rounding the float64 sum would be wrong
    naive = (a * b + c).float().double()
    assert int((naive != expect).sum()) >= 100


# ------------------------------------------------------------------ Adam against torch.optim.Adam
@pytest.mark.parametrize("foreach", [False, True])
def test_adam_emulation_matches_torch_adam(foreach):
    """torch.optim.Adam(amsgrad=True, weight_decay > 0) on the same trajectory: 7 steps, the learning rate changed between steps,
    gradients that flip sign and shrink so that v_max > v, grad_scale != 1 (applied on the torch side by scaling the gradient).

    The two differ in rounding only: torch takes its bias corrections in double from the double betas and orders the operations
    differently.  A per-step difference of the update is then a few fp32 roundings of m / den, and m is a sum of terms of either sign:
    its rounding error is relative to M, the same recursion run on |gr|, not to |m|.  1e-5 x lr_bc1 M / den, summed over the steps, is
    about ten times the ~10 roundings of 2^-24 each that the update goes through; 2 ulp of p cover the final roundings of p, which may
    fall on either side once the updates differ at all."""
    gen = torch.Generator().manual_seed(3)
    n = 4096
    p0 = torch.randn(n, generator=gen)
    beta1, beta2, eps, wd, gs = 0.9, 0.999, 1e-8, 1e-2, 0.25
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(beta1, beta2), eps=eps, weight_decay=wd, amsgrad=True, foreach=foreach)
    p, m, v, vx = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    M = torch.zeros(n, dtype=F64)
    bound = torch.zeros(n, dtype=F64)
    base = torch.randn(n, generator=gen)
    lrs = [1e-3, 3e-3, 5e-4, 2e-3, 1e-3, 7e-4, 4e-3]
    seen_vmax_gt_v = False
    for step, lr in enumerate(lrs, start=1):
        g = (base * (1.0 if step % 2 else -0.3) * (4.0 if step <= 2 else 0.5) + 0.01 * torch.randn(n, generator=gen)).float()
        for grp in opt.param_groups:
            grp["lr"] = lr
        ref.grad = (g * gs).float()
        opt.step()
        h = X.Hyper(lr, beta1, beta2, eps, wd, step, gs)
        gr = X.fma32(h.wd, p, X.rn(g.double() * h.grad_scale))
        p, m, v, vx = X.adam_update(p, g.double(), m, v, vx, h)
        seen_vmax_gt_v |= bool((vx > v).any())
        M = h.beta1 * M + (1 - h.beta1) * gr.abs()
        den = torch.sqrt(vx) / h.bc2_sqrt + h.eps
        bound += 1e-5 * h.lr_bc1 * M / den
    assert seen_vmax_gt_v
    diff = (p - ref.detach().double()).abs()
    ulp = torch.pow(2.0, torch.floor(torch.log2(p.abs())) - 23)
    allowed = 2 * ulp + bound
    assert bool((diff <= allowed).all()), float((diff - allowed).max())
    st = opt.state[ref]
    # the moments: m against M (it cancels); v and v_max carry the float beta2: 1 - (float)0.999 is 1.3e-5 above 1 - 0.999 relatively,
    # which the float bias correction (1 - beta2^t) takes out again in the update but not in the moment itself
    for name, ours, theirs, ref_mag, tol in (("m", m, st["exp_avg"], M, 1e-5), ("v", v, st["exp_avg_sq"], v, 2e-5),
                                             ("v_max", vx, st["max_exp_avg_sq"], vx, 2e-5)):
        rel = ((ours - theirs.double()).abs() / ref_mag.clamp(min=1e-30)).max().item()
        assert rel <= tol, (name, rel)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_operand_classes_reach_zero_gradients_and_denormals(wd):
    """with and without weight decay (the GPU tests run with 1e-2 and grad_scale 0.5): class 1 is a zero gradient, class 3 leaves
    denormal v and v_max, so that flushing fp32 denormals to zero anywhere in the update changes output bits"""
    gen = torch.Generator().manual_seed(13)
    state = [t.double() for t in X.adam_state(5000, gen)]
    p, g, m, v, vx = state
    out = X.adam_update(p, g, m, v, vx, X.Hyper(1e-3, 0.9, 0.999, 1e-8, wd, 1, 0.5))
    X.assert_class_reaches(state, out)
    ftz = [torch.where(t.abs() < X.FLT_MIN, torch.zeros_like(t), t) for t in state]
    out_ftz = X.adam_update(ftz[0], ftz[1], ftz[2], ftz[3], ftz[4], X.Hyper(1e-3, 0.9, 0.999, 1e-8, wd, 1, 0.5))
    out_ftz = [torch.where(t.abs() < X.FLT_MIN, torch.zeros_like(t), t) for t in out_ftz]
    assert int((out_ftz[2] != out[2]).sum()) > 0 and int((out_ftz[3] != out[3]).sum()) > 0


def test_dense_weight_norm_rows_fill_every_group():
    for K in (1, 3, 6, 64, 160, 764, 768, 772, 1728, 2304):
        pt = X.dense_pattern(K)
        ss = sum(x * x for x in pt)
        assert len(pt) >= K - 2 and ss & (ss - 1) == 0 and (ss.bit_length() - 1) % 2 == 0, (K, ss)
    v, _ = X.wn_rows(4, 772, torch.Generator().manual_seed(14))
    nz = (v[0] != 0).view(-1, 4).any(1)
    assert int(nz.sum()) >= 772 // 4 - 2


def test_hyper_parameters_repeat_the_host_code():
    h = X.Hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 3, 1.0)
    b1 = float(np.float32(0.9))
    assert h.lr_bc1 == X.f32(X.f32(1e-3) / X.f32(1.0 - b1 ** 3))
    assert h.beta1 == b1 and h.beta1 != 0.9


# ------------------------------------------------------------------ layouts and weight-norm formulas
def test_reference_layouts_match_the_shadow_helpers():
    gen = torch.Generator().manual_seed(4)
    for taps, N, C, kc_pad, rows_pad, n_pad, B_rows_pad in ((9, 40, 13, 16, 48, 48, 16), (6, 24, 7, 8, 32, 32, 16), (1, 70, 30, 32, 80, 72, 32)):
        w = torch.randn(N, C, taps, generator=gen)
        sc = torch.randn(N, generator=gen)
        params = w.reshape(-1)
        j = X.relayout_job(0, C * taps, taps, taps, N, C, 0, 0, rows_pad, kc_pad, 0, B_rows_pad, n_pad, C)
        A, B = X.relayout_operands(j, params, sc)
        wk = w.view(N, C, taps, 1)
        # the helpers scale in fp32 too; shadow_t / shadow_nt with row / column scale = the kernel's v * scale[n]
        assert torch.equal(A.float(), helpers.shadow_nt(wk, kc_pad, rows_pad, taps * kc_pad, "f32", row_scale=sc))
        assert torch.equal(B.float(), helpers.shadow_t(wk, n_pad, B_rows_pad, "f32", col_scale=sc))
        for esz, dt in ((2, torch.bfloat16), (4, torch.float32)):
            ks = 64 // esz
            if (taps * kc_pad) % ks == 0 and rows_pad % 16 == 0:
                flat = torch.zeros(A.numel(), dtype=F64)
                X.place(flat, A, 0, 1, esz)
                assert torch.equal(flat.view(A.shape).to(dt), helpers.frag_tile(A.to(dt)))


def test_reference_layout_matches_a_naive_loop():
    """strided source (s_k > s_n), B_rows_real below the real k, scale, padding on every side"""
    gen = torch.Generator().manual_seed(5)
    taps, N, K = 6, 5, 7
    j = X.relayout_job(3, taps, N * taps, taps, N, K, 2, 10, 8, 12, 500, 9, 8, 4)
    params = torch.randn(3 + N * K * taps + 4, generator=gen)
    scale = torch.randn(2 + N + 3, generator=gen)
    dst = torch.full((1000,), -1.0, dtype=F64)
    X.relayout_expect([j], params, scale, dst, 4)
    naive = torch.full((1000,), -1.0, dtype=F64)
    for n in range(j.A_rows_pad):
        for t in range(taps):
            for k in range(j.A_inner_pad):
                val = 0.0
                if n < N and k < K:
                    val = X.f32(float(params[3 + n * taps + k * N * taps + t]) * float(scale[2 + n]))
                naive[j.dstA + n * taps * j.A_inner_pad + t * j.A_inner_pad + k] = val
    for k in range(j.B_rows_pad):
        for t in range(taps):
            for n in range(j.B_inner_pad):
                val = 0.0
                if n < N and k < K and k < j.B_rows_real:
                    val = X.f32(float(params[3 + n * taps + k * N * taps + t]) * float(scale[2 + n]))
                naive[j.dstB + k * taps * j.B_inner_pad + t * j.B_inner_pad + n] = val
    X.assert_same(dst, naive, "layout", X.locate_relayout([j], 4))


def test_weight_norm_operands_are_exact_and_formulas_match_loops():
    gen = torch.Generator().manual_seed(6)
    for K in (1, 3, 6, 64, 772, 2304):
        rows = 7
        v, es = X.wn_rows(rows, K, gen)
        g = X.wn_gains(rows, gen)
        dw = torch.randint(-3, 4, (rows, K), generator=gen).float()
        scale, inv = X.wn_scale_ref(v, g)
        dg, dv = X.wn_bwd_ref(v, g, dw, inv)
        for r in range(rows):
            ss = sum(float(x) ** 2 for x in v[r])
            assert ss == 4.0 ** es[r]
            nrm = math.sqrt(ss)
            assert inv[r].item() == 1 / nrm and scale[r].item() == float(g[r]) / nrm
            dot = sum(float(a) * float(b) for a, b in zip(v[r], dw[r]))
            assert dg[r].item() == dot / nrm
            for k in range(0, K, max(1, K // 17)):
                assert dv[r, k].item() == float(g[r]) / nrm * float(dw[r, k]) - float(g[r]) * dot / nrm ** 3 * float(v[r, k])
        for name, x in (("scale", scale), ("inv", inv), ("dg", dg), ("dv", dv)):
            X.assert_exactly_representable(x, name)
        # against autograd through torch's weight-norm formula
        vv, gg = v.double().requires_grad_(True), g.double().requires_grad_(True)
        w = gg[:, None] * vv / vv.norm(dim=1, keepdim=True)
        w.backward(dw.double())
        assert torch.allclose(gg.grad, dg, rtol=0, atol=1e-12) and torch.allclose(vv.grad, dv, rtol=0, atol=1e-12)


def test_scaled_shadow_values_include_bf16_ties():
    """v * scale of the weight-norm operands lands on bf16 ties, so RNE and the other roundings differ on them"""
    gen = torch.Generator().manual_seed(8)
    v, _ = X.wn_rows(64, 64, gen)
    g = X.wn_gains(64, gen)
    scale, _ = X.wn_scale_ref(v, g)
    x = X.rn(v.double() * scale[:, None]).float()
    low = x.view(torch.int32) & 0xFFFF
    assert int((low == 0x8000).sum()) > 0


# ------------------------------------------------------------------ mutants the comparator must reject
def _adam_variant(p, g, m, v, vx, h, kind):
    rn, fma32 = X.rn, X.fma32
    if kind == "grad_scale_after_wd":
        gr = rn(fma32(h.wd, p, g) * h.grad_scale)
    else:
        gr = fma32(h.wd, p, rn(g * h.grad_scale))
    m = fma32(h.beta1, m, rn(X.f32(1.0 - h.beta1) * gr))
    v = fma32(h.beta2, v, rn(rn(X.f32(1.0 - h.beta2) * gr) * gr))
    vx = torch.maximum(vx, v)
    den_of = v if kind == "v_in_denominator" else vx
    denom = rn(rn(rn(torch.sqrt(den_of)) / h.bc2_sqrt) + h.eps)
    return fma32(-h.lr_bc1, rn(m / denom), p), m, v, vx


def _adam_case():
    gen = torch.Generator().manual_seed(9)
    return [t.double() for t in X.adam_state(5000, gen)]


@pytest.mark.parametrize("kind", ["v_in_denominator", "bias_correction_at_step_minus_1", "grad_scale_after_wd"])
def test_comparator_rejects_adam_mutants(kind):
    p, g, m, v, vx = _adam_case()
    step = 3
    h = X.Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-2, step, 0.5)
    good = X.adam_update(p, g, m, v, vx, h)
    assert torch.equal(good[0], _adam_variant(p, g, m, v, vx, h, None)[0])
    if kind == "bias_correction_at_step_minus_1":
        bad = X.adam_update(p, g, m, v, vx, X.Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-2, step - 1, 0.5))
    else:
        bad = _adam_variant(p, g, m, v, vx, h, kind)
    with pytest.raises(AssertionError):
        X.assert_same(bad[0].float(), good[0].float(), f"p under {kind}")


def test_comparator_rejects_round_toward_zero():
    gen = torch.Generator().manual_seed(10)
    v, _ = X.wn_rows(64, 64, gen)
    scale, _ = X.wn_scale_ref(v, X.wn_gains(64, gen))
    x = X.rn(v.double() * scale[:, None]).float().reshape(-1)
    rtz = (x.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)      # truncation is exact in bf16
    X.assert_same(x.to(torch.bfloat16), x.double(), "RNE")
    with pytest.raises(AssertionError):
        X.assert_same(rtz, x.double(), "round toward zero")


def _relayout_case():
    gen = torch.Generator().manual_seed(11)
    jobs = [X.relayout_job(0, 9 * 13, 9, 9, 40, 13, -1, 0, 48, 16, 48 * 9 * 16, 16, 48, 13),
            X.relayout_job(40 * 13 * 9, 70, 1, 1, 100, 70, 0, 20000, 100, 72, 30000, 72, 100, 70)]
    jobs, nb, _ = X.relayout_table(jobs)
    params = torch.randn(40 * 13 * 9 + 7000, generator=gen)
    scale = torch.randn(100, generator=gen)
    dst = X.sentinel(40000, F64)
    return jobs, nb, params, scale, dst


def test_comparator_rejects_swapped_n_and_k_in_the_b_operand():
    jobs, _, params, scale, dst = _relayout_case()
    good = X.relayout_expect(jobs, params, scale, dst.clone(), 2)
    bad = dst.clone()
    for j in jobs:
        A, B = X.relayout_operands(j, params, scale)
        X.place(bad, A, j.dstA, 0, 2)
        Bs = torch.zeros_like(B.view(j.B_rows_pad, j.taps, j.B_inner_pad))
        Aw = A.view(j.A_rows_pad, j.taps, j.A_inner_pad)
        r, c = min(j.B_rows_pad, j.A_rows_pad), min(j.B_inner_pad, j.A_inner_pad)
        Bs[:r, :, :c] = Aw[:r, :, :c]                    # B[n][k] instead of B[k][n]
        X.place(bad, Bs.reshape(j.B_rows_pad, -1), j.dstB, 0, 2)
    with pytest.raises(AssertionError):
        X.assert_same(bad.to(torch.bfloat16), good, "B with n and k swapped", X.locate_relayout(jobs, 2))


def test_comparator_rejects_a_dropped_last_tile():
    jobs, nb, params, scale, dst = _relayout_case()
    good = X.relayout_expect(jobs, params, scale, dst.clone(), 2)
    j = jobs[-1]
    t_id = nb - 1 - j.block_start
    n0, k0 = (t_id // j.tiles_k) * j.tile, (t_id % j.tiles_k) * j.tile
    # the elements the last tile writes: mark them through the reference layout of an all-ones source
    ones = torch.ones_like(params)
    mark = torch.zeros(dst.numel(), dtype=F64)
    A, B = X.relayout_operands(j, ones, torch.ones_like(scale))
    Am = torch.zeros_like(A.view(j.A_rows_pad, j.taps, j.A_inner_pad))
    Am[n0:n0 + j.tile, :, k0:k0 + j.tile] = 1
    X.place(mark, Am.reshape(j.A_rows_pad, -1), j.dstA, 0, 2)
    Bm = torch.zeros_like(B.view(j.B_rows_pad, j.taps, j.B_inner_pad))
    Bm[k0:k0 + j.tile, :, n0:n0 + j.tile] = 1
    X.place(mark, Bm.reshape(j.B_rows_pad, -1), j.dstB, 0, 2)
    assert int(mark.sum()) > 0
    bad = torch.where(mark > 0, dst, good)
    with pytest.raises(AssertionError, match="job 1"):
        X.assert_same(bad.to(torch.bfloat16), good, "dropped last tile", X.locate_relayout(jobs, 2))


def test_comparator_rejects_one_store_outside_the_range():
    p, g, m, v, vx = _adam_case()
    h = X.Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-2, 2, 0.5)
    lo, hi = 1000, 3000          # element 3000 is of class 0: its update changes it
    expect = p.clone()
    expect[lo:hi] = X.adam_update(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], vx[lo:hi], h)[0]
    bad = expect.clone()
    bad[hi] = X.adam_update(p[hi:hi + 1], g[hi:hi + 1], m[hi:hi + 1], v[hi:hi + 1], vx[hi:hi + 1], h)[0]
    X.assert_same(expect.float(), expect, "in range")
    with pytest.raises(AssertionError, match="outside"):
        X.assert_same(bad.float(), expect, "one store past the range", X.locate_segments([("range", lo, hi - lo)]))


def test_comparator_rejects_wn_bwd_without_its_projection():
    gen = torch.Generator().manual_seed(12)
    v, _ = X.wn_rows(32, 160, gen)
    g = X.wn_gains(32, gen)
    dw = torch.randint(-3, 4, (32, 160), generator=gen).float()
    _, inv = X.wn_scale_ref(v, g)
    _, dv = X.wn_bwd_ref(v, g, dw, inv)
    no_proj = (g.double() * inv)[:, None] * dw.double()
    with pytest.raises(AssertionError):
        X.assert_same(no_proj.float(), dv, "dv without the projection term")


# ------------------------------------------------------------------ weight norm on real rows
def test_weight_norm_references_match_float64_autograd():
    """wn_scale_ref / wn_bwd_ref against float64 autograd through torch._weight_norm (w = g v / ||v|| per output row)"""
    gen = torch.Generator().manual_seed(11)
    for K in (1, 3, 160, 4608):
        v = (0.05 * torch.randn(6, K, generator=gen)).to(F64).requires_grad_()
        g = torch.randn(6, 1, generator=gen).to(F64).requires_grad_()
        dw = torch.randn(6, K, generator=gen).to(F64)
        w = torch._weight_norm(v, g, 0)
        w.backward(dw)
        sc, inv = X.wn_scale_ref(v.detach(), g.detach()[:, 0])
        assert torch.allclose(w.detach(), sc[:, None] * v.detach(), rtol=1e-13, atol=0)
        dg, dv = X.wn_bwd_ref(v.detach(), g.detach()[:, 0], dw, inv)
        sabs = (v.detach() * dw).abs().sum(1)
        assert bool(((dg - g.grad[:, 0]).abs() <= 1e-13 * inv * sabs).all()), K
        mag = X.wn_bwd_mags(v.detach(), g.detach()[:, 0], dw, inv)[1]
        assert bool(((dv - v.grad).abs() <= 1e-13 * mag).all()), K


def test_weight_norm_real_case_operands_and_yardsticks():
    """the operands of the GPU tests (seeds 410 / 510) hold what they promise, and the fp32 restatement that follows the kernel's
    per-lane strides stays within the recorded yardsticks, in the units the GPU tests use"""
    worst = dict(scale=0.0, inv_norm=0.0, dg=0.0, dv=0.0)
    for seed in (410, 510):
        jobs, total_rows, nout, params, grads, vals = X.wn_real_case(seed)
        assert sorted({j.K for j in jobs}) == sorted(X.WN_REAL_K) and {j.v_off % 4 for j in jobs if j.K == 18432} == {0, 1, 2, 3}
        for j, (g, v, dw) in zip(jobs, vals):
            nrm = v.to(F64).norm(dim=1)
            assert 0.9e-3 < float(nrm[0]) < 1.3e-3 and 0.7e3 < float(nrm[1]) < 1.1e3
            sc, inv = X.wn_scale_ref(v, g)
            inv32 = inv.float()
            dg, dv = X.wn_bwd_ref(v, g, dw, inv32)
            mdg, mdv = X.wn_bwd_mags(v, g, dw, inv32)
            if j.K >= 64:
                # the radial row cancels: the result is far below its terms
                assert float(dv[2].abs().max()) < 0.05 * float(mdv[2].max())
                assert 0.5 < float(nrm[3] / (0.05 * j.K ** 0.5)) < 1.5
            r_sc, r_inv = X.wn_scale_restate(v, g, j.v_off)
            r_dg, r_dv = X.wn_bwd_restate(v, g, dw, inv32, j.v_off)          # (teacher-forced, as the GPU test is)
            worst["scale"] = max(worst["scale"], X.units(r_sc, sc, sc))
            worst["inv_norm"] = max(worst["inv_norm"], X.units(r_inv, inv, inv))
            worst["dg"] = max(worst["dg"], X.units(r_dg, dg, mdg))
            worst["dv"] = max(worst["dv"], X.units(r_dv, dv, mdv))
    print("weight-norm restatement, worst units:", worst)
    for k, e in worst.items():
        assert e <= X.WN_YARDSTICK[k], (k, e)


def test_weight_norm_real_comparator_has_teeth():
    """a norm accumulated in bf16-rounded squares, and a dot product that drops its last 4-group, exceed the bounds"""
    jobs, total_rows, nout, params, grads, vals = X.wn_real_case(410)
    j, (g, v, dw) = next((j, x) for j, x in zip(jobs, vals) if j.K == 4608 and j.v_off % 4 == 0)
    sc, inv = X.wn_scale_ref(v, g)
    bad_inv = 1.0 / torch.sqrt(((v * v).bfloat16().float()).sum(1))
    assert X.units(bad_inv, inv, inv) > X.wn_bound("inv_norm")
    inv32 = inv.float()
    dg, dv = X.wn_bwd_ref(v, g, dw, inv32)
    mdg, mdv = X.wn_bwd_mags(v, g, dw, inv32)
    v_short = v.clone()
    v_short[:, -4:] = 0
    b_dg, b_dv = X.wn_bwd_restate(v_short, g, dw, inv32, j.v_off)
    assert X.units(b_dg, dg, mdg) > X.wn_bound("dg")
    # bcoef with inv^2 instead of inv^3
    dot = (dw * v).sum(1)
    wrong = (g * inv32)[:, None] * dw - (g * dot * inv32 * inv32)[:, None] * v
    assert X.units(wrong, dv, mdv) > X.wn_bound("dv")
