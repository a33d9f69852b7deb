"""Every convolution kernel path, bit-exact on integer operands (tests/conv_exact.py): each case names the kernel family the dispatcher
must send it to (ipoke_last_conv_kernel / ipoke_last_wgrad_kernel), with shapes just inside and just outside each family's predicate
(csrc/gemm.hip: s8_applicable, k64_applicable, k8_applicable, c64_applicable, halo16_applicable, halo_applicable; lat8_applicable,
halo_wgrad_applicable and the tn kernels of launch_tn).  Around every operand and output sits a sentinel that must survive.

The census at the end records every distinct convolution descriptor of one c4 training step at its benchmarked batch (B = 20) and of
one c5 decode (B = 32, z = 64, 480 frames), replays each on fresh sentinel buffers with exact operands -- same kernel, exact result --
and asserts that the two runs reach the round-6 kernels (the halo16 four-tap phase, the padded two-tap windows, k8, c64)."""
import collections
import struct
import time
from ctypes import byref

import pytest
import torch

from ipoke_amd import _lib, ops
from tests import conv_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = _lib.BF16, _lib.F32
FAMILY = {_lib.KERNEL_IGEMM: "igemm", _lib.KERNEL_S8: "s8/k64", _lib.KERNEL_HALO: "halo", _lib.KERNEL_HALO16: "halo16",
          _lib.KERNEL_C64: "c64", _lib.KERNEL_K8: "k8"}
WFAMILY = {_lib.WGRAD_TN: "tn", _lib.WGRAD_TN_GLDS: "tn_glds", _lib.WGRAD_TN_NARROW: "tn_narrow", _lib.WGRAD_LAT8: "lat8",
           _lib.WGRAD_HALO: "wgrad_halo"}
IG, S8, HALO, H16, C64, K8 = (_lib.KERNEL_IGEMM, _lib.KERNEL_S8, _lib.KERNEL_HALO, _lib.KERNEL_HALO16, _lib.KERNEL_C64, _lib.KERNEL_K8)


def c3(NB, H, W, Kc, Nout, **kw):
    """3 x 3, stride 1, padding 1 on H x W"""
    return X.conv_desc(NB, (1, H, W), (1, H, W), (1, 3, 3), (1, 1, 1), (0, 1, 1), Kc, Nout, kw.pop("dtype", BF), **kw)


def c27(NB, D, H, W, Kc, Nout, sd=1, **kw):
    Do = (D - 1) // sd + 1
    return X.conv_desc(NB, (D, H, W), (Do, H, W), (3, 3, 3), (sd, 1, 1), (1, 1, 1), Kc, Nout, kw.pop("dtype", BF), **kw)


def phase(NB, H, W, Kc, Nout, a, b, kh, kw_, **kw):
    """sub-pixel phase (a, b) of a stride-2 ConvTranspose2d on H x W as a stride-1 kh x kw_ window writing every second row / column of
    the 2H x 2W map (first_stage.py: _run_phases)"""
    Ho, Wo = 2 * H, 2 * W
    return X.conv_desc(NB, (1, H, W), (1, H, W), (1, kh, kw_), (1, 1, 1), (0, 0, 0), Kc, Nout, kw.pop("dtype", BF),
                       scatter=(Ho * Wo, 2 * Wo, 2, a * Wo + b), **kw)


def skinny(M, Kc):
    return _lib.lib().ipoke_conv3x3_skinny_splitk(M, Kc, BF)


# id -> (descriptor factory, dtype, expected family, dispatch override or None, ConvCase options)
CASES = {
    # ---- s8 / s8n32 (8 x 8 latent, Kc >= 256 in 64-channel chunks, Nout <= 64)
    "s8_k256_n32_b5": (lambda: c3(5, 8, 8, 256, 32), BF, S8, None, {}),
    "s8_k512_n60_b3": (lambda: c3(3, 8, 8, 512, 60), BF, S8, None, {}),
    "s8_k2048_n64_b7": (lambda: c3(7, 8, 8, 2048, 64), BF, S8, None, {}),
    "s8_transposed_k512_n64_b5": (lambda: c3(5, 8, 8, 512, 64, transposed=True), BF, S8, None, {}),
    "s8_splitk_slabs_k1024_n48_b20": (lambda: c3(20, 8, 8, 1024, 48, c_f32=True, ldc=48, splitk=skinny(1280, 1024)), BF, S8, None, {}),
    "s8_splitk_acc_dgrad_k512_n32_b20": (lambda: c3(20, 8, 8, 512, 32, transposed=True, c_f32=True, ldc=32, c_acc=True,
                                                    splitk=skinny(1280, 512)), BF, S8, None, dict(acc=True)),
    "s8_outside_k192": (lambda: c3(5, 8, 8, 192, 64), BF, IG, None, {}),
    "s8_outside_n72": (lambda: c3(5, 8, 8, 256, 72), BF, IG, None, {}),
    # ---- k64 (8 x 8, Kc <= 64, Nout >= 256, at most 256 tiles)
    "k64_k8_n256_b3": (lambda: c3(3, 8, 8, 8, 256), BF, S8, None, {}),
    "k64_k32_n2048_b3": (lambda: c3(3, 8, 8, 32, 2048), BF, S8, None, {}),
    "k64_k40_n256_b20": (lambda: c3(20, 8, 8, 40, 256), BF, S8, None, {}),
    "k64_k32_n2048_b20": (lambda: c3(20, 8, 8, 32, 2048), BF, S8, None, {}),
    "k64_outside_b40_n2048": (lambda: c3(40, 8, 8, 32, 2048), BF, IG, None, {}),
    "k64_outside_n248": (lambda: c3(20, 8, 8, 32, 248), BF, IG, None, {}),
    # ---- k8 (one 16-byte chunk of input channels, Nout <= 64 in 16s, M >= 65536, no epilogue)
    "k8_cin3_n16_m65536": (lambda: c3(4, 128, 128, 8, 16), BF, K8, None, dict(live_c=3)),
    "k8_cin8_n48_m65536": (lambda: c3(4, 128, 128, 8, 48), BF, K8, None, {}),
    "k8_cin8_n64_m65536_transposed": (lambda: c3(4, 128, 128, 8, 64, transposed=True), BF, K8, None, {}),
    "k8_cin3_n64_transposed": (lambda: c3(4, 128, 128, 8, 64, transposed=True), BF, K8, None, dict(live_c=3)),
    "k8_outside_m49152": (lambda: c3(3, 128, 128, 8, 64), BF, IG, None, {}),
    "k8_outside_bias": (lambda: c3(4, 128, 128, 8, 64, bias=True), BF, IG, None, {}),
    "k8_outside_n72": (lambda: c3(4, 128, 128, 8, 72), BF, IG, None, {}),
    # ---- c64 (filter resident in LDS: Kc 64 / 128 -> <= 64 outputs on maps of 16 x 16 patches)
    "c64_k64_n64_default_rule": (lambda: c3(8, 128, 128, 64, 64), BF, C64, None, {}),
    "c64_outside_k128_9tap": (lambda: c3(4, 32, 32, 128, 48), BF, IG, "c64", {}),      # 9 taps x 2 chunks > the 9 resident slices
    "c64_k64_n40_relu_bias": (lambda: c3(2, 32, 48, 64, 40, act=_lib.ACT_RELU, bias=True), BF, C64, "c64", {}),
    "c64_transposed_k64_n32": (lambda: c3(4, 32, 32, 64, 32, transposed=True), BF, C64, "c64", {}),
    "c64_phase00_1tap": (lambda: phase(2, 32, 32, 64, 64, 0, 0, 1, 1), BF, C64, "c64", {}),
    "c64_phase01_2tap": (lambda: phase(2, 32, 32, 64, 64, 0, 1, 1, 2), BF, C64, "c64", {}),
    "c64_phase10_2tap": (lambda: phase(2, 32, 32, 128, 64, 1, 0, 2, 1), BF, C64, "c64", {}),
    "c64_phase11_4tap": (lambda: phase(2, 32, 32, 64, 64, 1, 1, 2, 2), BF, C64, "c64", {}),
    "c64_phase11_4tap_k128_n56": (lambda: phase(3, 16, 32, 128, 56, 1, 1, 2, 2), BF, C64, "c64", {}),
    "c64_outside_n72": (lambda: c3(8, 32, 32, 64, 72), BF, HALO, "c64", {}),
    "c64_outside_h24": (lambda: c3(8, 24, 32, 64, 64), BF, HALO, "c64", {}),
    # ---- halo16 (2-D 9-tap, 3-D 27-tap, the four-tap phase and the padded two-tap windows)
    "halo16_k128_n96": (lambda: c3(2, 32, 32, 128, 96), BF, H16, "halo16", {}),
    "halo16_k128_n128_elu": (lambda: c3(2, 32, 32, 128, 128, act=_lib.ACT_ELU, bias=True), BF, H16, "halo16", {}),
    "halo16_k256_n200": (lambda: c3(2, 16, 32, 256, 200), BF, H16, "halo16", {}),
    "halo16_3d_k64_n96": (lambda: c27(2, 4, 16, 16, 64, 96), BF, H16, "halo16", {}),
    "halo16_3d_depth_stride2_k64_n128": (lambda: c27(2, 6, 16, 32, 64, 128, sd=2), BF, H16, "halo16", {}),
    "halo16_phase11_4tap": (lambda: phase(2, 16, 16, 128, 128, 1, 1, 2, 2), BF, H16, "halo16", {}),
    "halo16_phase01_padded_2x2_16": (lambda: phase(2, 16, 16, 128, 128, 0, 1, 2, 2), BF, H16, "halo16", dict(zero_taps=(2, 3))),
    "halo16_phase10_padded_2x2_16": (lambda: phase(2, 16, 16, 128, 128, 1, 0, 2, 2), BF, H16, "halo16", dict(zero_taps=(1, 3))),
    "halo16_phase01_padded_2x2_32": (lambda: phase(3, 32, 32, 256, 128, 0, 1, 2, 2), BF, H16, "halo16", dict(zero_taps=(2, 3))),
    "halo16_default_rule_60x64x64": (lambda: c3(60, 64, 64, 128, 128), BF, H16, None, {}),
    "halo16_outside_h24": (lambda: c3(2, 24, 32, 128, 128), BF, IG, "halo16", {}),
    "halo16_outside_k96": (lambda: c3(2, 32, 32, 96, 128), BF, IG, "halo16", {}),
    # ---- halo (2-D: >= 64 channels on large maps, or maps of <= 256 pixels; 3-D: 64 channels)
    "halo_k64_128x128_n3_f32out_tanh": (lambda: c3(1, 128, 128, 64, 3, c_f32=True, act=_lib.ACT_TANH, bias=True), BF, HALO, None, {}),
    "halo_k64_n64_elu_channel_range": (lambda: c3(4, 32, 32, 64, 64, ldc=160, c_coff=32, act=_lib.ACT_ELU, bias=True), BF, HALO, None, {}),
    "halo_k512_16x16_n256": (lambda: c3(20, 16, 16, 512, 256), BF, HALO, None, {}),
    "halo_3d_k64_n64": (lambda: c27(4, 4, 16, 16, 64, 64, act=_lib.ACT_RELU, bias=True), BF, HALO, None, {}),
    "halo_outside_w24": (lambda: c3(8, 32, 24, 64, 64), BF, IG, None, {}),
    "halo_outside_m1024": (lambda: c3(1, 32, 32, 64, 64), BF, IG, None, {}),
    # ---- implicit GEMM
    "igemm_1x1_k128_n192": (lambda: X.conv_desc(4, (1, 16, 16), (1, 16, 16), (1, 1, 1), (1, 1, 1), (0, 0, 0), 128, 192, BF), BF, IG, None, {}),
    "igemm_stem_3x7x7_a_f32": (lambda: X.conv_desc(2, (4, 32, 32), (4, 16, 16), (3, 7, 7), (1, 2, 2), (1, 3, 3), 8, 64, BF, Kc_real=3,
                                                   a_f32=True, bias=True, act=_lib.ACT_RELU), BF, IG, None, {}),
    "igemm_stem_3x7x7_f32": (lambda: X.conv_desc(2, (4, 32, 32), (4, 16, 16), (3, 7, 7), (1, 2, 2), (1, 3, 3), 4, 64, F32, Kc_real=3,
                                                 a_f32=True, c_f32=True, bias=True), F32, IG, None, {}),
    "igemm_patchgan_4x4_s2_lrelu": (lambda: X.conv_desc(2, (1, 32, 32), (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1), 64, 128, BF,
                                                        act=_lib.ACT_LRELU02, bias=True), BF, IG, None, {}),
    "igemm_strided_dgrad_dact_elu": (lambda: X.conv_desc(2, (1, 16, 16), (1, 32, 32), (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 64, BF,
                                                         transposed=True, dact_act=_lib.ACT_ELU), BF, IG, None, {}),
    "igemm_row_scale_bias": (lambda: c3(6, 16, 16, 32, 96, row_scale=(2, 2), bias=True), BF, IG, None, {}),
    "igemm_channel_range_k40": (lambda: c3(2, 16, 16, 40, 96, lda=64, a_coff=16, ldc=256, c_coff=64), BF, IG, None, {}),
    "igemm_f32_3x3_acc": (lambda: c3(2, 16, 16, 64, 80, dtype=F32, c_f32=True, c_acc=True), F32, IG, None, {}),
    "igemm_f32_3x3_bias_elu": (lambda: c3(2, 16, 16, 36, 72, dtype=F32, c_f32=True, act=_lib.ACT_ELU, bias=True), F32, IG, None, {}),
    "igemm_f32_dtype_out_transposed": (lambda: c3(2, 16, 16, 32, 40, dtype=F32, transposed=True), F32, IG, None, {}),
    "igemm_f32_8x8_k512_n64": (lambda: c3(3, 8, 8, 512, 64, dtype=F32, c_f32=True), F32, IG, None, {}),
    "igemm_3d_scatter_with_depth": (lambda: X.conv_desc(2, (4, 16, 16), (4, 16, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), 64, 64, BF,
                                                           scatter=(8 * 32 * 32, 2 * 32 * 32, 2 * 32, 2, 32 * 32 + 33)), BF, IG, None, {}),
    # ---- wide up-convolutions at 8 x 8 (256 -> 128 channels): the padded two-tap phases fall back to the implicit GEMM
    "upconv8_phase00_1tap": (lambda: phase(4, 8, 8, 256, 128, 0, 0, 1, 1), BF, IG, None, {}),
    "upconv8_phase01_padded_2x2": (lambda: phase(4, 8, 8, 256, 128, 0, 1, 2, 2), BF, IG, None, dict(zero_taps=(2, 3))),
    "upconv8_phase10_padded_2x2": (lambda: phase(4, 8, 8, 256, 128, 1, 0, 2, 2), BF, IG, None, dict(zero_taps=(1, 3))),
    "upconv8_phase11_4tap": (lambda: phase(4, 8, 8, 256, 128, 1, 1, 2, 2), BF, IG, None, {}),
}

def _run_conv(d, dtype, opts, seed):
    opts = dict(opts)
    acc = None
    if opts.pop("acc", False):
        nbytes = _lib.lib().ipoke_conv_acc_scratch_bytes(X.rows_of(d), d.Nout, d.splitk)
        acc = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
        _lib.check(_lib.lib().ipoke_conv_acc_scratch_init(_lib.ptr(acc), _lib.current_stream()))
    case = X.ConvCase(d, dtype, DEV, seed=seed, acc_scratch=acc, **opts)
    return case, case.run()


@pytest.mark.parametrize("name", list(CASES))
def test_conv_kernel_exact(name):
    make, dtype, family, override, opts = CASES[name]
    d = make()
    if d.splitk == 0:
        pytest.fail("ipoke_conv3x3_skinny_splitk declined the shape")
    if override is not None:
        with _lib.dispatch_override(override, 2):
            case, got = _run_conv(d, dtype, opts, seed=len(name))
    else:
        case, got = _run_conv(d, dtype, opts, seed=len(name))
    print(f"case {name} -> {FAMILY.get(got, got)}")
    assert got == family, f"{name}: dispatched to {FAMILY.get(got, got)}, the table names {FAMILY[family]}"
    case.compare(name)


# ------------------------------------------------------------------ weight gradients
def _wg(NB, H, W, Kc, Nout, k=3, D=1, **kw):
    kd = 3 if D > 1 else 1
    return X.wgrad_desc(NB, (D, H, W), (kd, k, k), (kd // 2, k // 2, k // 2), Kc, Nout, kw.pop("dtype", BF), **kw)


WCASES = {
    "wgrad_halo_k64_n128_64x64": (lambda: _wg(4, 64, 64, 64, 128), BF, _lib.WGRAD_HALO, 0),
    "wgrad_halo_slabs_k128_n64_32x32": (lambda: _wg(16, 32, 32, 128, 64), BF, _lib.WGRAD_HALO, 512),
    "wgrad_halo_3d_k64_n64": (lambda: _wg(4, 32, 32, 64, 64, D=4), BF, _lib.WGRAD_HALO, 256),
    "wgrad_halo_c4_size_k64_n32_300x128x128": (lambda: _wg(300, 128, 128, 64, 32), BF, _lib.WGRAD_HALO, 512),
    "wgrad_halo_outside_m4096": (lambda: _wg(4, 32, 32, 64, 64), BF, _lib.WGRAD_TN_GLDS, 0),
    "wgrad_tn_1x1_k128_n256": (lambda: _wg(4, 16, 16, 128, 256, k=1), BF, _lib.WGRAD_TN_GLDS, 0),
    "wgrad_tn_3x3_k48_n40_ragged": (lambda: _wg(3, 16, 16, 48, 40), BF, _lib.WGRAD_TN_GLDS, 0),
    # a map of fewer than 64 positions: a 64-row stage of the LDS-DMA kernel holds several samples (the second stage starts at sample 2)
    "wgrad_tn_3x3_k24_n32_4x8_map": (lambda: _wg(4, 4, 8, 24, 32), BF, _lib.WGRAD_TN_GLDS, 0),
    "wgrad_tn_f32_3x3_k36_n20": (lambda: _wg(2, 16, 16, 36, 20, dtype=F32), F32, _lib.WGRAD_TN, 0),
    "wgrad_tn_f32_1x1_split_atomic": (lambda: _wg(8, 16, 16, 64, 64, k=1, dtype=F32, splitm=4), F32, _lib.WGRAD_TN, 0),
}


@pytest.mark.parametrize("name", list(WCASES))
def test_wgrad_kernel_exact(name):
    make, dtype, family, target = WCASES[name]
    d = make()
    if target:
        q = X.clone_desc(d)
        q.A = q.dY = 256                                               # (the query validates the descriptor: aligned non-null operands)
        sp = _lib.lib().ipoke_conv_wgrad_splitm(byref(q), dtype, target)
        assert sp > 1, f"{name}: no split preference (the halo-staged kernel does not apply)"
        T = X.taps_of(d)
        d.splitm = sp
        d.split_stride = X.round_up(d.Nout * d.Kc * T + 1024, 64)     # slabs with a sentinel gap between them
    case = X.WgradCase(d, dtype, DEV, seed=len(name))
    got = case.run()
    print(f"case {name} -> {WFAMILY.get(got, got)} (splitm {d.splitm})")
    assert got == family, f"{name}: dispatched to {WFAMILY.get(got, got)}, the table names {WFAMILY[family]}"
    case.compare(name)


def _batched(cases, k, narrow=False):
    """ipoke_conv_wgrad_batched over the problems of several WgradCases (entries relative to the first one's buffers)"""
    base = cases[0]
    es = _lib.lib().ipoke_wgrad_batch_entry_size()
    assert es == struct.calcsize("qqqiiiiq")
    raw = b"".join(struct.pack("qqqiiiiq", c.A.data_ptr() - base.A.data_ptr(), c.dY.data_ptr() - base.dY.data_ptr(),
                               (c.dW.data_ptr() - base.dW.data_ptr()) // 4, k, k, k // 2, k // 2, 0) for c in cases)
    entries = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    d = X.clone_desc(base.d)
    _lib.check(_lib.lib().ipoke_conv_wgrad_batched(byref(d), entries.data_ptr(), len(cases), base.A.data_ptr(), base.dY.data_ptr(),
                                                   base.dW.data_ptr(), BF, _lib.current_stream()))
    torch.cuda.synchronize()
    return _lib.lib().ipoke_last_wgrad_kernel()


@pytest.mark.parametrize("B,Kc,Nout,k,nb,family", [(20, 512, 64, 3, 2, _lib.WGRAD_LAT8), (7, 320, 136, 3, 1, _lib.WGRAD_LAT8),
                                                   (3, 64, 48, 3, 3, _lib.WGRAD_LAT8), (20, 512, 48, 1, 2, _lib.WGRAD_TN_NARROW),
                                                   (5, 256, 256, 1, 2, _lib.WGRAD_TN_GLDS)])
def test_batched_wgrad_exact(B, Kc, Nout, k, nb, family):
    """wgrad3x3_lat8 (the coupling nets' conv1 / conv3 on the 8x8 latent) and the 64 x 256 'narrow' tiles of the LDS-DMA kernel"""
    cases = [X.WgradCase(_wg(B, 8, 8, Kc, Nout, k=k), BF, DEV, seed=B + i) for i in range(nb)]
    got = _batched(cases, k)
    print(f"case batched B={B} Kc={Kc} Nout={Nout} k={k} x{nb} -> {WFAMILY.get(got, got)}")
    assert got == family, (WFAMILY.get(got, got), WFAMILY[family])
    for i, c in enumerate(cases):
        c.compare(f"batched problem {i}")


# ------------------------------------------------------------------ census of the benchmarked shapes
def _record(monkeypatch):
    seen = collections.OrderedDict()
    orig = ops.conv_forward

    def conv_forward(d, dtype):
        orig(d, dtype)
        dt = ops._dt(dtype)
        key = X.desc_key(d, dt)
        if key not in seen:
            seen[key] = (X.strip_pointers(d), dt, _lib.lib().ipoke_last_conv_kernel())

    monkeypatch.setattr(ops, "conv_forward", conv_forward)
    return seen


def _c4_census(golden, monkeypatch):
    from tests.test_train_mode_gpu import clip, train_model
    g = golden("g13_first_stage_train_mode_128")
    m = train_model("bf16")
    X_, eps = clip(g, copies=20)
    seen = _record(monkeypatch)
    loss, X_hat, mu, lv = m.training_loss(X_, eps)
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    del m, X_, eps, loss, X_hat, mu, lv
    return seen


def _c5_census(monkeypatch):
    from ipoke_amd import configs
    from ipoke_amd.first_stage import SpadeCondMotionModel
    torch.manual_seed(0)
    model = SpadeCondMotionModel(configs.first_stage_config(128, 64, 16), dirs={}, dtype="bf16").to(DEV).eval()
    gen = torch.Generator().manual_seed(3)
    motion = torch.randn(32, 64, 8, 8, generator=gen).to(DEV)
    start = (torch.rand(32, 3, 128, 128, generator=gen) * 2 - 1).to(DEV)
    seen = _record(monkeypatch)
    out = model.decode(motion, start, 15)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert out.shape[:2] == (32, 15)
    del model, out
    return seen


def _phase(d):
    """(a, b) of a 2 x 2 sub-pixel window writing rows 2 i + a, columns 2 j + b of the up-sampled map, else None"""
    if not (d.c_scatter and d.Do == 1 and d.kh == 2 and d.kw == 2 and d.ph == 0 and d.pw == 0 and d.c_sw == 2):
        return None
    return divmod(int(d.c_row0), 2 * d.Wo)


def _replay(seen, tag):
    counts = collections.Counter()
    for i, ((d, flags), dtype, kern) in enumerate(seen.values()):
        counts[FAMILY.get(kern, kern)] += 1
        acc = None
        if flags["acc"]:
            nbytes = _lib.lib().ipoke_conv_acc_scratch_bytes(X.rows_of(d), d.Nout, d.splitk)
            acc = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
            _lib.check(_lib.lib().ipoke_conv_acc_scratch_init(_lib.ptr(acc), _lib.current_stream()))
        case = X.ConvCase(d, dtype, DEV, seed=i, has_bias=flags["bias"], has_row_scale=flags["row_scale"], has_dact=flags["dact"],
                          acc_scratch=acc)
        got = case.run()
        what = (f"{tag} descriptor {i}: NB={d.NB} in={d.Di}x{d.Hi}x{d.Wi} out={d.Do}x{d.Ho}x{d.Wo} k={d.kd}x{d.kh}x{d.kw} "
                f"s={d.sd},{d.sh},{d.sw} tr={d.transposed} Kc={d.Kc_real}/{d.Kc} Nout={d.Nout} dtype={dtype} scatter={d.c_scatter} "
                f"splitk={d.splitk} {flags}")
        assert got == kern, f"{what}: replay reached {FAMILY.get(got, got)}, the run reached {FAMILY.get(kern, kern)}"
        case.compare(what)
        del case
    torch.cuda.empty_cache()
    print(f"census {tag}: {len(seen)} distinct descriptors; per family: {dict(sorted(counts.items()))}")
    return counts


def test_census_of_the_benchmarked_shapes(golden, monkeypatch):
    """c4 training step at B = 20 (forward + backward, 300 decoded frames) and c5's decode (B = 32, z = 64, 480 frames): every distinct
    descriptor replayed exactly on the kernel the run reached; the round-6 paths must be among them."""
    t0 = time.time()
    c4 = _c4_census(golden, monkeypatch)
    c5 = _c5_census(monkeypatch)
    t1 = time.time()
    allv = list(c4.values()) + list(c5.values())
    # the round-6 kernels at the benchmarked sizes
    assert any(k == H16 and _phase(d) == (1, 1) for (d, fl), dt, k in allv), "no four-tap phase on conv3x3_halo16"
    assert any(k == H16 and _phase(d) in ((0, 1), (1, 0)) for (d, fl), dt, k in c5.values()), \
        "no padded two-tap window on conv3x3_halo16 in the c5 decode"
    assert any(k == K8 for (d, fl), dt, k in c4.values()), "conv3x3_k8 not reached by the c4 step"
    assert any(k == C64 and (d.Ho == 128 or (d.c_scatter and 2 * d.Ho == 128)) for (d, fl), dt, k in allv), \
        "conv3x3_c64 not reached on the 128 x 128 layers"
    n4 = _replay(c4, "c4 B=20")
    n5 = _replay(c5, "c5 B=32")
    print(f"census: runs {t1 - t0:.1f} s, replays {time.time() - t1:.1f} s; c4 {dict(n4)}; c5 {dict(n5)}")
