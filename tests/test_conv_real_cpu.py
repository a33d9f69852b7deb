"""The real-valued comparator of tests/conv_exact.py, checked without a GPU: the operand rules, the recorded yardsticks (the fp32
restatement of every case's reduction length and operand distribution, and torch's fp32 activations, against float64), that the honest
fp32 chain passes on CPU-sized cases, and that the comparator has teeth: an operand passed through bf16 or an 11-bit significand, a row
scale applied after a bf16 rounding, exp(x) - 1 in an fp32 store at small arguments, a dropped K block and a missing slab all fail."""
import pytest
import torch

from ipoke_amd import _lib
from tests import conv_exact as X
from tests import test_conv_real_gpu as G

CPU = "cpu"
BF, F32 = _lib.BF16, _lib.F32
F64 = torch.float64


def c3(NB, H, W, Kc, Nout, **kw):
    return X.conv_desc(NB, (1, H, W), (1, H, W), (1, 3, 3), (1, 1, 1), (0, 1, 1), Kc, Nout, kw.pop("dtype", BF), **kw)


# ------------------------------------------------------------------ the honest fp32 chain and its mutants
def act32(act, v, naive_elu):
    if act == _lib.ACT_ELU:
        return torch.where(v > 0, v, torch.exp(v) - 1 if naive_elu else torch.expm1(v))
    return X.act64(act, v)


def emulate(case, a_map=None, w_map=None, drop_last_block=False, scale_after_bf16=False, naive_elu=None, drop_slab=None):
    """the C buffer an honest kernel would leave: block dot products rounded to fp32 and added in order, the epilogue in fp32 in the
    kernel's order (scale, bias, activation, derivative mask, old value), one rounding into the store dtype.  The keyword arguments
    are the mistakes the comparator must catch."""
    d = case.d
    M = X.rows_of(d)
    x = X.gather_rows(d, case.A_eff, torch.arange(M))
    w = X.weight_matrix(d, case.W)
    if a_map is not None:
        x = a_map(x)
    if w_map is not None:
        w = w_map(w)
    blk = X.k_block(case.dtype)
    K = x.shape[1]
    if drop_last_block:
        K = (K - 1) // blk * blk
    C = case.C0.clone()
    if case.splitk > 1 and not d.c_accumulate:
        nblk = -(-K // blk)
        per = -(-nblk // case.splitk) * blk
        for z in range(case.splitk):
            k0, k1 = z * per, min(K, (z + 1) * per)
            part = X.block_restatement(x[:, k0:k1], w[k0:k1], blk) if k1 > k0 else torch.zeros(M, d.Nout)
            if z == drop_slab:
                part = torch.zeros_like(part)
            C[z * M:(z + 1) * M, : d.Nout] = part
            C[z * M:(z + 1) * M, d.Nout:] = 0
        return C
    v = X.block_restatement(x[:, :K], w[:K], blk)
    if case.row_scale is not None:
        if scale_after_bf16:
            v = v.to(torch.bfloat16).to(torch.float32)
        v = v * case._scale_per_row(M).to(torch.float32).view(-1, 1)
    if case.bias is not None:
        v = v + case.bias
    naive = case.elu_fast() if naive_elu is None else naive_elu
    v = act32(d.act, v, naive)
    if case.dact is not None:
        v = v * X.act_grad_from_out64(d.dact_act, case.dact[:M, : d.Nout].to(torch.float32))
    rows = X.out_row_index(d, torch.arange(M))
    cols = d.c_coff + torch.arange(d.Nout) * max(1, d.c_cstride)
    if d.c_accumulate:
        v = C[rows][:, cols].to(torch.float32) + v
    C[rows.view(-1, 1), cols.view(1, -1)] = v.to(C.dtype)
    if not d.c_f32:
        n_pad = min(X.round_up(d.Nout, X.e16(case.dtype)), d.ldc - d.c_coff)
        if n_pad > d.Nout:
            C[rows.view(-1, 1), (d.c_coff + torch.arange(d.Nout, n_pad)).view(1, -1)] = 0
    return C


def to_bits(t, bits):
    """float64 values truncated to a `bits`-bit significand"""
    q = torch.pow(2.0, torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -200))) - (bits - 1))
    return torch.trunc(t / q) * q


def to_bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


HONEST = {
    "f32_k576": (lambda: c3(1, 8, 8, 64, 8, dtype=F32, c_f32=True, bias=True), F32, {}),
    "f32_elu_k324": (lambda: c3(1, 6, 6, 36, 12, dtype=F32, c_f32=True, bias=True, act=_lib.ACT_ELU), F32, {}),
    "bf16_elu_bf16_store": (lambda: c3(2, 4, 4, 32, 8, bias=True, act=_lib.ACT_ELU), BF, {}),
    "bf16_tanh_f32_store": (lambda: c3(2, 4, 4, 32, 6, bias=True, act=_lib.ACT_TANH, c_f32=True), BF, {}),
    "bf16_sigmoid_channel_range": (lambda: c3(2, 4, 4, 32, 6, bias=True, act=_lib.ACT_SIGMOID, ldc=24, c_coff=8), BF, {}),
    "bf16_row_scale_f32_store": (lambda: c3(4, 4, 4, 32, 8, row_scale=(2, 2), bias=True, c_f32=True), BF, {}),
    "bf16_a_f32_stem": (lambda: X.conv_desc(1, (2, 8, 8), (2, 4, 4), (3, 7, 7), (1, 2, 2), (1, 3, 3), 8, 8, BF, Kc_real=3, a_f32=True,
                                            bias=True, act=_lib.ACT_RELU), BF, {}),
    "f32_acc": (lambda: c3(1, 4, 4, 64, 8, dtype=F32, c_f32=True, c_acc=True), F32, {}),
    "bf16_slabs": (lambda: c3(1, 8, 8, 256, 16, c_f32=True, ldc=16, splitk=4), BF, {}),
    "bf16_dgrad_dact_tanh": (lambda: X.conv_desc(1, (1, 4, 4), (1, 8, 8), (1, 3, 3), (1, 2, 2), (0, 1, 1), 32, 8, BF, transposed=True,
                                                 dact_act=_lib.ACT_TANH), BF, {}),
    "bf16_dgrad_dact_lrelu": (lambda: X.conv_desc(1, (1, 4, 4), (1, 8, 8), (1, 3, 3), (1, 2, 2), (0, 1, 1), 32, 8, BF, transposed=True,
                                                  dact_act=_lib.ACT_LRELU02), BF, {}),
    "small_elu_bf16_store": (lambda: c3(2, 4, 4, 32, 8, act=_lib.ACT_ELU), BF, dict(w_exp=-14)),
    "small_elu_f32_store": (lambda: c3(2, 4, 4, 32, 8, act=_lib.ACT_ELU, c_f32=True), BF, dict(w_exp=-14)),
    "small_elu_f32_launch": (lambda: c3(1, 6, 6, 36, 8, dtype=F32, act=_lib.ACT_ELU, c_f32=True), F32, dict(w_exp=-14)),
}


def _case(name):
    make, dtype, opts = HONEST[name]
    return X.RealConvCase(make(), dtype, CPU, "cpu_" + name, seed=5, **opts)


@pytest.mark.parametrize("name", list(HONEST))
def test_honest_fp32_chain_passes(name):
    case = _case(name)
    worst = case.compare(name, got=emulate(case))
    print(f"{name}: honest chain at {worst:.3f} x its allowance")
    assert worst <= 0.5, "the honest chain should sit well inside the allowance (its contraction part is at the yardstick, a quarter of it)"
    # and an untouched buffer (nothing stored) fails
    with pytest.raises(AssertionError):
        case.compare(name, got=case.C0.clone())


MUTANTS = [
    ("f32_k576", dict(a_map=to_bf16)), ("f32_k576", dict(w_map=to_bf16)),
    ("f32_k576", dict(a_map=lambda t: to_bits(t, 11))), ("f32_k576", dict(w_map=lambda t: to_bits(t, 11))),
    ("bf16_row_scale_f32_store", dict(scale_after_bf16=True)),
    ("small_elu_f32_store", dict(naive_elu=True)), ("small_elu_f32_launch", dict(naive_elu=True)),
    ("f32_k576", dict(drop_last_block=True)), ("bf16_elu_bf16_store", dict(drop_last_block=True)),
    ("bf16_slabs", dict(drop_last_block=True)), ("bf16_slabs", dict(drop_slab=2)),
]


@pytest.mark.parametrize("name,mut", MUTANTS, ids=[f"{n}-{'-'.join(m)}-{i}" for i, (n, m) in enumerate(MUTANTS)])
def test_mutant_chain_fails(name, mut):
    case = _case(name)
    with pytest.raises(AssertionError, match="beyond their allowance"):
        case.compare(name, got=emulate(case, **mut))
    print(f"{name} {sorted(mut)}: {case.worst:.1f} x the allowance")
    assert case.worst > 2


def test_a_stray_store_fails():
    case = _case("bf16_sigmoid_channel_range")
    C = emulate(case)
    C[3, 2] = 1.0                                   # a column before c_coff
    with pytest.raises(AssertionError, match="outside the written region"):
        case.compare("stray", got=C)


# ------------------------------------------------------------------ operand rules
def test_operand_rules():
    for name in ("f32_k576", "f32_elu_k324", "small_elu_f32_launch"):
        case = _case(name)
        d = case.d
        idx = (X.pixel_offsets(d).unsqueeze(1) + torch.arange(d.Kc_real) * d.a_sc).reshape(-1)
        for what, t in (("A", case.A[idx]), ("W", case.W)):
            assert t.dtype == torch.float32
            assert X.not_representable(t, 8) >= 0.9 and X.not_representable(t, 11) >= 0.9, (name, what)
    # bf16 launch from an fp32 source: full-mantissa values in memory, their RNE bf16 in the reference
    case = _case("bf16_a_f32_stem")
    d = case.d
    idx = (X.pixel_offsets(d).unsqueeze(1) + torch.arange(d.Kc_real) * d.a_sc).reshape(-1)
    assert X.not_representable(case.A[idx], 8) >= 0.9 and X.not_representable(case.A_eff[idx], 8) == 0.0
    W3 = case.W.view(d.Nout, X.taps_of(d), d.Kc)
    assert bool((W3[:, :, d.Kc_real:] == 0).all()) and bool((W3[:, :, : d.Kc_real] != 0).any())
    # row scales: in [0.3, 3], no power of two, NaN in the unused slots
    case = _case("bf16_row_scale_f32_store")
    rs = case.row_scale
    used = rs[::2]
    assert bool(((used >= 0.3) & (used <= 3)).all()) and not bool((torch.frexp(used)[0] == 0.5).any()) and bool(torch.isnan(rs[1::2]).all())
    # pre-activations reach the curved part; the small-argument cases do not leave |x| < 2^-10
    case = _case("bf16_tanh_f32_store")
    case.expected_real()
    assert 0.5 < float(case.pre.std()) < 4
    case = _case("small_elu_f32_store")
    case.expected_real()
    assert 0 < float(case.pre.abs().max()) < 2.0 ** -10
    # saved outputs: the activation's own range, both zeros for the piecewise-linear ones
    g = torch.Generator().manual_seed(0)
    for act, lo, hi in ((_lib.ACT_ELU, -1, 3), (_lib.ACT_TANH, -1, 1), (_lib.ACT_SIGMOID, 0, 1)):
        s = X.saved_outputs(act, (4096,), torch.bfloat16, g).to(F64)
        assert float(s.min()) >= lo and float(s.max()) <= hi and float(s.max() - s.min()) > 0.9 * (hi - lo)
    for act in (_lib.ACT_RELU, _lib.ACT_LRELU02):
        s = X.saved_outputs(act, (4096,), torch.bfloat16, g)
        z = s[s == 0]
        assert bool((s > 0).any()) and bool((s < 0).any()) and bool(torch.signbit(z).any()) and bool((~torch.signbit(z)).any())
    # weight gradient
    wc = X.RealWgradCase(X.wgrad_desc(2, (1, 4, 4), (1, 3, 3), (0, 1, 1), 4, 5, F32), F32, CPU, "cpu_f32", seed=1)
    M = X.rows_of(wc.d)
    assert X.not_representable(wc.dY[:M, :5], 11) >= 0.9 and 0.05 < float(wc.dY[:M, :5].std()) < 0.2


# ------------------------------------------------------------------ yardsticks
def sample_rows(M, K):
    """every row where the CPU can afford it, else evenly spaced ones (2^22 operand elements)"""
    R = min(M, max(64, (1 << 22) // max(1, K)))
    return torch.arange(M) if R == M else torch.linspace(0, M - 1, R).round().to(torch.int64).unique()


def measure_conv_case(case):
    """worst error, in ulp32(S), of the block restatement of the case's own reduction on the case's own operands: the bare sums (what
    the split-K slabs hold) and the sums behind the case's scale, bias and old value, each step rounded to fp32"""
    d = case.d
    M = X.rows_of(d)
    m = sample_rows(M, X.taps_of(d) * d.Kc_real)
    x = X.gather_rows(d, case.A_eff, m)
    w = X.weight_matrix(d, case.W)
    acc = X.block_restatement(x, w, X.k_block(case.dtype))
    y, S = x @ w, x.abs() @ w.abs()
    worst = float(((acc.to(F64) - y).abs() / X.ulp32(S)).max())
    v = acc
    if case.row_scale is not None:
        s = case._scale_per_row(M)[m].view(-1, 1)
        v, y, S = v * s.to(torch.float32), y * s, S * s.abs()
    if case.bias is not None:
        v, y, S = v + case.bias, y + case.bias.to(F64), S + case.bias.to(F64).abs()
    if d.c_accumulate and case.splitk == 1:
        rows = X.out_row_index(d, m)
        cols = d.c_coff + torch.arange(d.Nout) * max(1, d.c_cstride)
        old = case.C0[rows][:, cols]
        v, y, S = old.to(torch.float32) + v, old.to(F64) + y, S + old.to(F64).abs()
    return max(worst, float(((v.to(F64) - y).abs() / X.ulp32(S)).max()))


def measure_wgrad_case(case):
    """the same for a weight gradient: blocks of 32 output rows, at most 256 of the (tap, channel) columns and 32 of the outputs"""
    d = case.d
    M = X.rows_of(d)
    x = X.gather_rows(d, case.A_eff, torch.arange(M))
    if x.shape[1] > 256:
        x = x[:, torch.linspace(0, x.shape[1] - 1, 256).round().to(torch.int64).unique()]
    dy = case.dY[:M, d.y_coff:d.y_coff + min(d.Nout, 32)].to(F64).t().contiguous()
    acc = X.block_restatement(dy, x, 32)
    return float(((acc.to(F64) - dy @ x).abs() / X.ulp32(dy.abs() @ x.abs())).max())


def all_conv_cases():
    for name, (make, dtype, family, override, opts) in G.REAL_CASES.items():
        opts = {k: v for k, v in opts.items() if k != "acc"}
        yield name, lambda make=make, dtype=dtype, opts=opts, name=name: X.RealConvCase(make(), dtype, CPU, name, seed=len(name), **opts)
    for name in HONEST:
        yield "cpu_" + name, lambda name=name: _case(name)


def all_wgrad_cases():
    for name in G.REAL_WCASES:
        def make(name=name):
            d, dtype, family = G.wgrad_problem(name, split=False)
            return X.RealWgradCase(d, dtype, CPU, name, seed=len(name))
        yield name, make
    for B, Kc, Nout, k, nb, family in G.BATCHED:
        key = G.batched_key(B, Kc, Nout, k)
        yield key, lambda B=B, Kc=Kc, Nout=Nout, k=k, key=key: X.RealWgradCase(G._wg(B, 8, 8, Kc, Nout, k=k), BF, CPU, key, seed=B)
    for kind in ("f32", "acc", "slabs"):
        yield "cpu_" + kind, lambda kind=kind: _wcase(kind)


def test_every_case_has_its_yardstick_and_the_restatement_keeps_it():
    for kind, cases, measure in (("fwd", all_conv_cases(), measure_conv_case), ("wgrad", all_wgrad_cases(), measure_wgrad_case)):
        table = X.REAL_YARDSTICK[kind]
        for name, make in cases:
            assert name in table, f"{kind} case {name} has no recorded yardstick"
            e = measure(make())
            print(f"yardstick {kind} {name}: measured {e:.3f}, recorded {table[name]}, bound {X.real_bound((kind, name))}")
            assert e <= table[name], (kind, name, e)


def test_activation_yardsticks():
    """torch's fp32 expm1 / tanh / sigmoid on the CPU against float64 over the cases' arguments (spread 1.5, and the small ones), in fp32
    ulps of the value; the derivative from the saved output in ulps of its terms' magnitudes"""
    g = torch.Generator().manual_seed(2)
    x = torch.cat([1.5 * torch.randn(1 << 16, generator=g), 2.0 ** -14 * torch.randn(1 << 14, generator=g)]).to(torch.float32)
    x64 = x.to(F64)
    for act, key in X.ACT_KEY.items():
        got = act32(act, x, False).to(F64)
        ref = X.act64(act, x64)
        e = float(((got - ref).abs() / X.ulp32(ref)).max())
        print(f"{key}: measured {e:.3f}, recorded {X.REAL_YARDSTICK[key]}")
        assert e <= X.REAL_YARDSTICK[key], (key, e)
    worst = 0.0
    for act in (_lib.ACT_ELU, _lib.ACT_TANH, _lib.ACT_SIGMOID, _lib.ACT_RELU, _lib.ACT_LRELU02):
        y = X.saved_outputs(act, (1 << 14,), torch.float32, g)
        got = X.act_grad_from_out64(act, y).to(F64)                 # float32 arithmetic on float32 operands
        ref = X.act_grad_from_out64(act, y.to(F64))
        mag = X.act_grad_mag64(act, y.to(F64))
        worst = max(worst, float(((got - ref).abs() / X.ulp32(mag)).max()))
    print(f"dact: measured {worst:.3f}, recorded {X.REAL_YARDSTICK['dact']}")
    assert worst <= X.REAL_YARDSTICK["dact"]


# ------------------------------------------------------------------ weight gradient comparator
def emulate_wgrad(case, drop_last_block=False, drop_slab=None, dy_map=None):
    d = case.d
    M = X.rows_of(d)
    T = X.taps_of(d)
    x = X.gather_rows(d, case.A_eff, torch.arange(M))                  # [M, T * Kc_real]
    dy = case.dY[:M, d.y_coff:d.y_coff + d.Nout].to(F64)
    if dy_map is not None:
        dy = dy_map(dy)
    dW = case.W0.clone()
    rows = M if not drop_last_block else (M - 1) // 32 * 32
    per = -(-(-(-rows // 32)) // case.nsplit) * 32
    for z in range(case.nsplit):
        m0, m1 = z * per, min(rows, (z + 1) * per)
        part = X.block_restatement(dy[m0:m1].t().contiguous(), x[m0:m1], 32) if m1 > m0 else torch.zeros(d.Nout, T * d.Kc_real)
        if z == drop_slab:
            part = torch.zeros_like(part)
        part = part.view(d.Nout, T, d.Kc_real)[:, :, : case.kst].permute(0, 2, 1).reshape(-1)
        pos = case._positions(z)
        dW[pos] = dW[pos] + part if d.accumulate else part
    return dW


def _wcase(kind):
    if kind == "f32":
        return X.RealWgradCase(X.wgrad_desc(4, (1, 8, 8), (1, 3, 3), (0, 1, 1), 8, 6, F32), F32, CPU, "cpu_f32", seed=2)
    if kind == "acc":
        return X.RealWgradCase(X.wgrad_desc(4, (1, 8, 8), (1, 3, 3), (0, 1, 1), 8, 6, BF, accumulate=True), BF, CPU, "cpu_acc", seed=3)
    d = X.wgrad_desc(4, (1, 8, 8), (1, 3, 3), (0, 1, 1), 8, 6, BF, splitm=4, split_stride=X.round_up(6 * 8 * 9 + 100, 64))
    return X.RealWgradCase(d, BF, CPU, "cpu_slabs", seed=4)


def test_weight_gradient_comparator():
    for kind in ("f32", "acc", "slabs"):
        case = _wcase(kind)
        worst = case.compare(kind, got=emulate_wgrad(case))
        print(f"wgrad {kind}: honest chain at {worst:.3f} ulp32(S)")
        assert worst <= 1.0
        with pytest.raises(AssertionError, match="beyond"):
            case.compare(kind, got=emulate_wgrad(case, drop_last_block=True))
    with pytest.raises(AssertionError, match="beyond"):
        _c = _wcase("slabs")
        _c.compare("slab left out", got=emulate_wgrad(_c, drop_slab=1))
    for m in (to_bf16, lambda t: to_bits(t, 11)):
        with pytest.raises(AssertionError, match="beyond"):
            _c = _wcase("f32")
            _c.compare("dY through a narrow format", got=emulate_wgrad(_c, dy_map=m))
    case = _wcase("slabs")
    dW = emulate_wgrad(case)
    dW[case._positions(0).max() + 3] = 0.0                            # the sentinel gap between two slabs
    with pytest.raises(AssertionError, match="outside"):
        case.compare("stray", got=dW)
