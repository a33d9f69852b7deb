"""The convolution and weight-gradient kernels on real-valued operands (tests/conv_exact.py: RealConvCase / RealWgradCase): every
kernel family and epilogue feature of tests/test_conv_exact_gpu.py once more, with operands that use the whole mantissa, row scales that
are no powers of two and activations on their curved part, against float64.  The contraction error is counted in fp32 ulps of the sum
of the terms' magnitudes and held to conv_exact.real_bound; every launch that takes no atomics runs twice and must give the same bits.

Each case prints its worst error in units of its allowance before it asserts (for a plain contraction the allowance is the bound
in ulp32(S); a bf16 store's own rounding is 0.50 of its allowance).

f32 launches (MI355X): with one accumulator over the whole reduction -- v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain that rounds
once per product -- ``igemm_f32_dtype_out_transposed`` reached 4.64 ulp32(S) against its bound of 4 and the 3x7x7 f32 stem 4.06
against 5.2 (an element-by-element fp32 chain on the CPU loses 3.2 and 4.3 on the same cases).  The f32 instantiations of the two
implicit-GEMM kernels now close the chain after every pass of their K loop (gemm.hip: fold_chain): 0.88 and 1.01."""
import pytest
import torch

from ipoke_amd import _lib
from tests import conv_exact as X
from tests.test_conv_exact_gpu import (BF, CASES, F32, FAMILY, IG, S8, WCASES, WFAMILY, _batched, _wg, c3, skinny)

pytestmark = pytest.mark.gpu
DEV = "cuda"

SKIP_FWD = ("halo16_default_rule_60x64x64",)                 # workload-sized: the integer family keeps it
SKIP_WGRAD = ("wgrad_halo_c4_size_k64_n32_300x128x128",)


def _dgrad(act):
    """the strided data gradient of a 3 x 3 stride-2 convolution with the derivative mask of `act` (general sweep)"""
    return X.conv_desc(2, (1, 16, 16), (1, 32, 32), (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 64, BF, transposed=True, dact_act=act)


# what the integer table lacks: id -> (descriptor factory, dtype, expected family, dispatch override, RealConvCase options)
EXTRA = {
    "igemm_dgrad_dact_tanh": (lambda: _dgrad(_lib.ACT_TANH), BF, IG, None, {}),
    "igemm_dgrad_dact_sigmoid": (lambda: _dgrad(_lib.ACT_SIGMOID), BF, IG, None, {}),
    "igemm_dgrad_dact_relu": (lambda: _dgrad(_lib.ACT_RELU), BF, IG, None, {}),
    "igemm_dgrad_dact_lrelu": (lambda: _dgrad(_lib.ACT_LRELU02), BF, IG, None, {}),
    "igemm_sigmoid_bf16_store": (lambda: c3(2, 16, 16, 32, 40, act=_lib.ACT_SIGMOID, bias=True), BF, IG, None, {}),
    "igemm_sigmoid_f32_store": (lambda: c3(2, 16, 16, 32, 40, act=_lib.ACT_SIGMOID, bias=True, c_f32=True), BF, IG, None, {}),
    "igemm_tanh_bf16_store": (lambda: c3(2, 16, 16, 32, 40, act=_lib.ACT_TANH, bias=True), BF, IG, None, {}),
    "igemm_tanh_f32_store": (lambda: c3(2, 16, 16, 32, 40, act=_lib.ACT_TANH, bias=True, c_f32=True), BF, IG, None, {}),
    "igemm_elu_bf16_compute_f32_store": (lambda: c3(2, 16, 16, 32, 40, act=_lib.ACT_ELU, bias=True, c_f32=True), BF, IG, None, {}),
    # an ELU launch that stores fp32 is kept off the halo / halo16 / c64 kernels (their sweeps take ELU as exp(x) - 1): the implicit
    # GEMM's general sweep, which uses expm1f for fp32 stores, gets the shapes those kernels would otherwise take
    "halo_outside_elu_f32_store": (lambda: c3(1, 128, 128, 64, 3, c_f32=True, act=_lib.ACT_ELU, bias=True), BF, IG, None, {}),
    "halo16_outside_elu_f32_store": (lambda: c3(2, 32, 32, 128, 128, act=_lib.ACT_ELU, bias=True, c_f32=True), BF, IG, "halo16", {}),
    "c64_outside_elu_f32_store": (lambda: c3(2, 32, 48, 64, 40, act=_lib.ACT_ELU, bias=True, c_f32=True), BF, IG, "c64", {}),
    "halo_small_elu_f32_store": (lambda: c3(1, 128, 128, 64, 3, c_f32=True, act=_lib.ACT_ELU), BF, IG, None, dict(w_exp=-14)),
    # K slices added atomically (no acc_scratch): held to the bound, not to reproducibility
    "s8_splitk_acc_atomic_k512_n32_b20": (lambda: c3(20, 8, 8, 512, 32, transposed=True, c_f32=True, ldc=32, c_acc=True,
                                                     splitk=skinny(1280, 512)), BF, S8, None, {}),
    # small arguments: weights scaled by a further 2^-14 and no bias, so S is tiny and the activation's own error is what is measured
    "small_elu_fast_path_bf16_store": (lambda: c3(4, 16, 16, 32, 128, act=_lib.ACT_ELU), BF, IG, None, dict(w_exp=-14)),
    "small_elu_general_f32_store": (lambda: c3(2, 16, 16, 32, 40, act=_lib.ACT_ELU, c_f32=True), BF, IG, None, dict(w_exp=-14)),
    "small_elu_f32_launch": (lambda: c3(2, 16, 16, 36, 72, dtype=F32, c_f32=True, act=_lib.ACT_ELU), F32, IG, None, dict(w_exp=-14)),
}
REAL_CASES = {k: v for k, v in CASES.items() if k not in SKIP_FWD}
REAL_CASES.update(EXTRA)


def _real_conv(d, dtype, opts, seed, key, device=DEV):
    opts = dict(opts)
    acc = None
    if opts.pop("acc", False):
        nbytes = _lib.lib().ipoke_conv_acc_scratch_bytes(X.rows_of(d), d.Nout, d.splitk)
        acc = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().ipoke_conv_acc_scratch_init(_lib.ptr(acc), _lib.current_stream()))
    return X.RealConvCase(d, dtype, device, key, seed=seed, acc_scratch=acc, **opts)


@pytest.mark.parametrize("name", list(REAL_CASES))
def test_conv_kernel_real(name):
    make, dtype, family, override, opts = REAL_CASES[name]
    d = make()
    if d.splitk == 0:
        pytest.fail("ipoke_conv3x3_skinny_splitk declined the shape")
    case = _real_conv(d, dtype, opts, len(name), name)
    if override is not None:
        with _lib.dispatch_override(override, 2):
            got, same = case.run_twice()
    else:
        got, same = case.run_twice()
    assert got == family, f"{name}: dispatched to {FAMILY.get(got, got)}, the table names {FAMILY[family]}"
    try:
        case.compare(name)
    finally:
        extra = f", ELU allowance {case.elu_allowance:.3e}" if hasattr(case, "elu_allowance") else ""
        print(f"real case {name} -> {FAMILY.get(got, got)}: worst {getattr(case, 'worst', float('nan')):.3f} x allowance "
              f"(contraction bound {X.real_bound(case.fwd_key)} ulp32(S)){extra}; atomic {case.atomic}; two runs identical {same}")
    assert same or case.atomic, f"{name}: two runs of a launch without atomics differ"


# ------------------------------------------------------------------ weight gradients
def _stem_a_f32():
    """the 3 x 7 x 7 stem's weight gradient from the fp32 NCDHW clip: 3 real channels in a padded chunk of 8, 3 stored (Kc_store)"""
    D, H, W = 4, 32, 32
    d = X.wgrad_desc(2, (D, H, W), (3, 7, 7), (1, 3, 3), 8, 64, BF, a_f32=True, out_dhw=(D, H // 2, W // 2), s=(1, 2, 2))
    S = D * H * W
    d.Kc_real = 3; d.Kc_store = 3
    d.a_sn, d.a_sc, d.a_sd, d.a_sh, d.a_sw = 3 * S, S, H * W, W, 1
    T = 3 * 7 * 7
    d.w_sn, d.w_sc, d.w_st = 3 * T, T, 1
    return d


REAL_WCASES = {k: v for k, v in WCASES.items() if k not in SKIP_WGRAD}
REAL_WCASES.update({
    "wgrad_stem_3x7x7_a_f32_kc_store": (_stem_a_f32, BF, None, 0),
    "wgrad_tn_3x3_k48_n40_accumulate": (lambda: _wg(3, 16, 16, 48, 40, accumulate=True), BF, _lib.WGRAD_TN_GLDS, 0),
})
BATCHED = [(20, 512, 64, 3, 2, _lib.WGRAD_LAT8), (7, 320, 136, 3, 1, _lib.WGRAD_LAT8), (3, 64, 48, 3, 3, _lib.WGRAD_LAT8),
           (20, 512, 48, 1, 2, _lib.WGRAD_TN_NARROW), (5, 256, 256, 1, 2, _lib.WGRAD_TN_GLDS)]


def batched_key(B, Kc, Nout, k):
    return f"batched_b{B}_k{Kc}_n{Nout}_{k}x{k}"


def wgrad_problem(name, split=True):
    """descriptor of a REAL_WCASES entry, with its split applied (the query asks the device: split=False where there is none)"""
    from ctypes import byref
    make, dtype, family, target = REAL_WCASES[name]
    d = make()
    if target and split:
        q = X.clone_desc(d)
        q.A = q.dY = 256
        sp = _lib.lib().ipoke_conv_wgrad_splitm(byref(q), dtype, target)
        assert sp > 1, f"{name}: no split preference (the halo-staged kernel does not apply)"
        d.splitm = sp
        d.split_stride = X.round_up(d.Nout * d.Kc * X.taps_of(d) + 1024, 64)
    return d, dtype, family


@pytest.mark.parametrize("name", list(REAL_WCASES))
def test_wgrad_kernel_real(name):
    d, dtype, family = wgrad_problem(name)
    case = X.RealWgradCase(d, dtype, DEV, name, seed=len(name))
    got, same = case.run_twice()
    if family is not None:
        assert got == family, f"{name}: dispatched to {WFAMILY.get(got, got)}, the table names {WFAMILY[family]}"
    try:
        case.compare(name)
    finally:
        print(f"real case {name} -> {WFAMILY.get(got, got)} (splitm {d.splitm}): worst {getattr(case, 'worst', float('nan')):.3f} ulp32(S), "
              f"bound {X.real_bound(case.key)}; atomic {case.atomic}; two runs identical {same}")
    assert same or case.atomic, f"{name}: two runs of a launch without atomics differ"


@pytest.mark.parametrize("B,Kc,Nout,k,nb,family", BATCHED)
def test_batched_wgrad_real(B, Kc, Nout, k, nb, family):
    cases = [X.RealWgradCase(_wg(B, 8, 8, Kc, Nout, k=k), BF, DEV, batched_key(B, Kc, Nout, k), seed=B + i) for i in range(nb)]
    got = _batched(cases, k)
    first = [c.dW.clone() for c in cases]
    for c in cases:
        c.dW.copy_(c.W0)
    _batched(cases, k)
    same = all(torch.equal(f.view(torch.uint8), c.dW.view(torch.uint8)) for f, c in zip(first, cases))
    assert got == family, (WFAMILY.get(got, got), WFAMILY[family])
    worst = 0.0
    try:
        for i, c in enumerate(cases):
            worst = max(worst, c.compare(f"batched problem {i}"))
    finally:
        print(f"real case batched B={B} Kc={Kc} Nout={Nout} k={k} x{nb} -> {WFAMILY.get(got, got)}: worst {worst:.3f} ulp32(S), "
              f"bound {X.real_bound(cases[0].key)}; two runs identical {same}")
    assert same, "two runs of the batched weight gradient differ"
