"""ipoke_conv_pair_dgrad: the conv2 and conv1 data gradients of a coupling net (NICEConvBlock, macow_utils.py:270-281) as one launch
-- dp1 = (dp2 @ W2) * ELU'(h1) in bf16, then the transposed 3x3 convolution of dp1 with conv1's filter accumulated into the fp32
gradient state, each 128-column tile of the GEMM being one K slice of the convolution.

Shapes: M = 64, 128, 192 rows (half a tile, one tile, a ragged second tile), hidden 256 / 2048 (2 / 16 slices), 8 / 24 / 32 conditioning
channels (the 64-column form stays on the two launches), dense and strided placement in a pre-filled target of pitch 136."""
import ctypes
import functools
from ctypes import byref

import pytest
import torch

from ipoke_amd import _lib, configs, ops
from tests import conv_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
LDC = 136
GUARD = X.GUARD_ROWS

SHAPES = [(B, hidden, cin) for B in (1, 2, 3) for hidden in (256, 2048) for cin in (8, 24, 32)]
PLACES = [(0, 1), (3, 2)]


def _descs(B, hidden, cin, c_coff, c_cstride):
    d2 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 1, 1), (1, 1, 1), (0, 0, 0))
    d1 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1), True)
    for d in (d2, d1):
        d.a_sn = 64 * hidden; d.a_sd = 0; d.a_sh = 8 * hidden; d.a_sw = hidden; d.a_sc = 1; d.Kc_real = hidden; d.Kc = hidden
    d2.ldw = hidden; d2.Nout = hidden; d2.w_kmajor = 1; d2.ld_dact = hidden; d2.dact_act = _lib.ACT_ELU; d2.c_f32 = 0; d2.ldc = hidden
    d1.ldw = 9 * hidden; d1.Nout = cin; d1.c_f32 = 1; d1.c_accumulate = 1; d1.ldc = LDC; d1.c_coff = c_coff; d1.c_cstride = c_cstride
    return d2, d1


@functools.lru_cache(maxsize=None)
def _scratch(B, hidden):
    L = _lib.lib()
    nbytes = L.ipoke_conv_acc_scratch_bytes(B * 64, 32, hidden // 128)
    s = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(L.ipoke_conv_acc_scratch_init(s.data_ptr(), _lib.current_stream()))
    torch.cuda.synchronize()
    return s


@functools.lru_cache(maxsize=None)
def _problem(kind, B, hidden, cin):
    """operands (device, bf16 / fp32) and the float64 expectation of dp1 and of the sums added to the target.  kind 'int': small
    integers and a saved h1 in {-1, -1/2, 1, 2} (ELU' factor 0, 1/2, 1, 1), every partial sum exact in fp32; 'real': randn."""
    gen = torch.Generator(device=DEV).manual_seed(1000 * B + hidden + cin + (7 if kind == "int" else 0))
    M = B * 64
    d2, d1 = _descs(B, hidden, cin, 0, 1)
    if kind == "int":
        lim2 = X.operand_limit(hidden, budget=float(1 << 14), cap=3)
        dp2 = X.int_operand((M, hidden), lim2, gen)
        w2 = X.int_operand((hidden, hidden), lim2, gen)
        w1 = X.int_operand((cin, 9 * hidden), 1, gen, zero_frac=0.5)
        pick = torch.randint(0, 4, (M, hidden), generator=gen, device=DEV)
        h1 = torch.tensor([-1.0, -0.5, 1.0, 2.0], dtype=torch.float64, device=DEV)[pick]
        base = X.int_operand((M + GUARD, LDC), 8, gen, zero_frac=0.1)
    else:
        dp2 = torch.randn(M, hidden, generator=gen, device=DEV, dtype=torch.float64)
        w2 = torch.randn(hidden, hidden, generator=gen, device=DEV, dtype=torch.float64) / hidden ** 0.5
        w1 = torch.randn(cin, 9 * hidden, generator=gen, device=DEV, dtype=torch.float64) / (9 * hidden) ** 0.5
        h1 = torch.randn(M, hidden, generator=gen, device=DEV, dtype=torch.float64)
        base = torch.randn(M + GUARD, LDC, generator=gen, device=DEV, dtype=torch.float64)
    dp2, w2, w1, h1 = (v.to(torch.bfloat16) for v in (dp2, w2, w1, h1))
    base = base.to(torch.float32)
    E1 = X.conv_sums(d2, dp2, w2) * X.act_grad_from_out64(_lib.ACT_ELU, h1.to(torch.float64))
    dp1 = X.to_bf16_rne(E1)
    Eadd = X.conv_sums(d1, dp1, w1)
    if kind == "int":       # every product and partial sum is exact in fp32, whatever the order: dp1 and the sums are multiples of 1/2
        X.assert_exact_bound(X.conv_sums(d2, dp2, w2, absolute=True))
        X.assert_exact_bound(X.conv_sums(d1, dp1, w1, absolute=True) + base[:M].abs().max().to(torch.float64), quantum=0.5)
    return dict(dp2=dp2, w2=w2, w1=w1, h1=h1, base=base, E1=E1, Eadd=Eadd)


def _bind(pr, B, hidden, cin, place):
    """descriptors on fresh output buffers: dp1 [M + guard][hidden] (sentinel-filled), target = a copy of the pre-filled base"""
    M = B * 64
    d2, d1 = _descs(B, hidden, cin, *place)
    dp1 = torch.full((M + GUARD, hidden), X.SENT, dtype=torch.bfloat16, device=DEV)
    tgt = pr["base"].clone()
    sc = _scratch(B, hidden)
    d2.A = pr["dp2"].data_ptr(); d2.W = pr["w2"].data_ptr(); d2.dact = pr["h1"].data_ptr(); d2.C = dp1.data_ptr()
    d1.A = dp1.data_ptr(); d1.W = pr["w1"].data_ptr(); d1.C = tgt.data_ptr()
    d1.acc_scratch = sc.data_ptr(); d1.acc_scratch_bytes = sc.numel()
    return d2, d1, dp1, tgt, sc


def _fused(d2, d1):
    _lib.check(_lib.lib().ipoke_conv_pair_dgrad(byref(d2), byref(d1), _lib.BF16, _lib.current_stream()))


def _counters_clean(sc):
    return int(sc[:16384].view(torch.int32).abs().max()) == 0


def _ids(v):
    return "-".join(str(x) for x in v)


@pytest.mark.parametrize("place", PLACES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_pair_dgrad_is_exact_on_integer_operands(shape, place):
    """dp1 and the accumulated gradient equal the float64 sums bit for bit (whatever the slice order); nothing outside them is written."""
    B, hidden, cin = shape
    M = B * 64
    pr = _problem("int", B, hidden, cin)
    d2, d1, dp1, tgt, sc = _bind(pr, B, hidden, cin, place)
    _fused(d2, d1)
    torch.cuda.synchronize()
    X.assert_exact(dp1[:M], pr["E1"], None, torch.bfloat16, d2, "dp1")
    assert bool((dp1[M:] == X.SENT).all()), "dp1: rows beyond M were written"
    want = pr["base"].to(torch.float64)
    c0, cs = place
    want[:M, c0:c0 + cs * cin:cs] += pr["Eadd"]
    X.assert_exact(tgt, want, None, torch.float32, None, "accumulated gradient")
    assert _counters_clean(sc)


@pytest.mark.parametrize("place", PLACES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_pair_dgrad_is_bit_identical_to_the_two_launches(shape, place):
    """Real-valued operands: the same 128 x 128 GEMM kernel family, then the skinny convolution with splitk = hidden / 128 -- the fused
    launch keeps the K-block order of both, so dp1 and the accumulated gradient agree in every bit."""
    B, hidden, cin = shape
    M = B * 64
    L = _lib.lib()
    pr = _problem("real", B, hidden, cin)
    d2, d1, dp1, tgt, sc = _bind(pr, B, hidden, cin, place)
    ops.conv_forward(d2, "bf16")
    assert L.ipoke_last_conv_kernel() == _lib.KERNEL_IGEMM
    d1.splitk = hidden // 128
    ops.conv_forward(d1, "bf16")
    assert L.ipoke_last_conv_kernel() == _lib.KERNEL_S8
    torch.cuda.synchronize()
    f2, f1, fdp1, ftgt, _ = _bind(pr, B, hidden, cin, place)
    _fused(f2, f1)
    torch.cuda.synchronize()
    assert not bool((dp1[:M] == X.SENT).all())
    assert torch.equal(fdp1.view(torch.int16), dp1.view(torch.int16)), f"dp1 differs: max {(fdp1[:M].float() - dp1[:M].float()).abs().max().item():.3e}"
    assert torch.equal(ftgt.view(torch.int32), tgt.view(torch.int32)), f"gradient differs: max {(ftgt - tgt).abs().max().item():.3e}"
    assert _counters_clean(sc)


@pytest.mark.parametrize("shape", [(3, 2048, 24), (2, 256, 32)], ids=_ids)
def test_pair_dgrad_is_deterministic_beside_a_copy_stream(shape):
    """The same launch again while a second stream runs large copies: the last arriver changes, the sums do not; counters back at zero."""
    B, hidden, cin = shape
    pr = _problem("real", B, hidden, cin)
    noise_src = torch.randn(64 << 20, device=DEV)
    side = torch.cuda.Stream()

    def run(disturb):
        d2, d1, dp1, tgt, sc = _bind(pr, B, hidden, cin, (3, 2))
        if disturb:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(disturb):
                    noise_src.clone()
        _fused(d2, d1)
        torch.cuda.synchronize()
        assert _counters_clean(sc)
        return dp1, tgt

    first = run(0)
    for k in range(1, 4):
        again = run(k)
        assert torch.equal(again[0].view(torch.int16), first[0].view(torch.int16)) and torch.equal(again[1].view(torch.int32), first[1].view(torch.int32))


def test_pair_dgrad_dispatch_rule():
    L = _lib.lib()
    big = 1 << 30
    for cin in (16, 32):                                    # the conditioning widths of the shipped z = 64 flow's fused couplings
        assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, cin, _lib.BF16, big) == 1
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 32, _lib.F32, big) == 0
    assert L.ipoke_conv_pair_dgrad_applicable(2560, 2048, 32, _lib.BF16, big) == 0          # 20 x 16 tiles: more than one round
    assert L.ipoke_conv_pair_dgrad_applicable(2048, 2048, 32, _lib.BF16, big) == 1          # 16 x 16
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 64, _lib.BF16, big) == 0          # the 64-column form: two launches
    need = 16384 + 10 * 16 * 128 * 32 * 4
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 32, _lib.BF16, need) == 1
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 32, _lib.BF16, need - 1) == 0      # scratch too small
    # a launch on a scratch that is too small is refused, not run
    pr = _problem("real", 1, 256, 8)
    d2, d1, dp1, tgt, sc = _bind(pr, 1, 256, 8, (0, 1))
    d1.acc_scratch_bytes = 16384 + 2 * 128 * 32 * 4 - 1
    assert L.ipoke_conv_pair_dgrad(byref(d2), byref(d1), _lib.BF16, _lib.current_stream()) != 0
    torch.cuda.synchronize()
    assert bool((dp1 == X.SENT).all())


def test_engine_fused_and_split_backward_are_bit_identical():
    """A reduced flow (hidden 256, B = 2): the backward pass with the fused launches and with the test hook that issues the two launches
    (same slices) -- every parameter gradient and dx bit for bit; the timing tags show which kernels ran."""
    from ipoke_amd.flow import SupervisedMacowTransformer
    from ipoke_amd.utils.detfill import deterministic_fill_
    arch = configs.flow_arch(32, hidden=256, num_steps=[2, 1, 1], factor=4)
    m = SupervisedMacowTransformer(arch, dtype="bf16", device="cuda", init="none", max_batch=2)
    deterministic_fill_(m, prefix="flow.")
    m.sync_buffers()
    m.train()
    eng = m.engine
    L = eng.lib
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 32, 8, 8, generator=g).cuda()
    cond = torch.randn(2, arch["h_channels"], 8, 8, generator=g).cuda()
    tags = (ctypes.c_int * 2)(16 + _lib.KERNEL_IGEMM, 16 + _lib.KERNEL_S8)      # (hidden < 1024: the GEMMs carry their family's tag)

    def run(split):
        _lib.check(L.ipoke_flow_test_split_pair_dgrad(eng.handle, int(split)))
        m.flat_grads.zero_()
        x = x0.clone().requires_grad_(True)
        out, logdet = m(x, cond)
        loss = (out ** 2).sum() * 0.5 - logdet.sum()
        torch.cuda.synchronize()
        _lib.check(L.ipoke_timing_start_all())
        loss.backward()
        torch.cuda.synchronize()
        counts = (ctypes.c_int * 2)(); mean = (ctypes.c_double * 2)()
        _lib.check(L.ipoke_timing_stop(tags, 2, counts, mean))
        return m.flat_grads.clone(), x.grad.clone(), (counts[0], counts[1])

    try:
        g_f, dx_f, n_f = run(False)
        g_s, dx_s, n_s = run(True)
        g_f2, dx_f2, _ = run(False)
    finally:
        L.ipoke_flow_test_split_pair_dgrad(eng.handle, 0)
    print(f"launches (GEMM family, stationary-input family): fused {n_f}, split {n_s}")
    assert n_f[0] == n_s[0] > 0 and n_s[1] == n_f[1] + n_f[0], (n_f, n_s)
    assert torch.isfinite(g_f).all() and g_f.abs().max() > 0
    assert torch.equal(g_f, g_f2) and torch.equal(dx_f, dx_f2), "the fused backward is not reproducible"
    assert torch.equal(g_f, g_s), f"gradients differ: max {(g_f - g_s).abs().max().item():.3e}"
    assert torch.equal(dx_f, dx_s), f"dx differs: max {(dx_f - dx_s).abs().max().item():.3e}"
