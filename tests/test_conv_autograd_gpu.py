"""The differentiable convolution op and ``_Conv.run`` bit-exactly against float64 autograd (tests/autograd_exact.py): one test per table
entry and dtype with ``==`` on every element of y, dX, dW, dbias and the padding columns and the recorded branch labels equal to the
table's; the module-level switches on and off give the same bits; the hand-over edges of backward; the state shared between calls (the
side stream of the weight gradients, one weight in two convolutions, the operand cache)."""
import pytest
import torch

from ipoke_amd import _lib, nn as K
from ipoke_amd import autograd_ops as FT
from ipoke_amd import first_stage as FS
from tests import autograd_exact as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(c.name, dt) for c in A.CASES for dt in c.dtypes]
IDS = [f"{n}-{dt}" for n, dt in PAIRS]


@pytest.mark.parametrize("name,dtype", PAIRS, ids=IDS)
def test_training_op_is_exact(name, dtype):
    A.run_training_case(A.BY_NAME[name], dtype)


@pytest.mark.parametrize("name,dtype", [p for p in PAIRS if A.BY_NAME[p[0]].run], ids=[i for i, p in zip(IDS, PAIRS) if A.BY_NAME[p[0]].run])
def test_conv_run_is_exact(name, dtype):
    A.run_inference_case(A.BY_NAME[name], dtype)


# ------------------------------------------------------------------ the module-level switches: same bits on the other branch
def _non_run(labels):
    return {l for l in labels if not l.startswith("run:")}


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("name", ["c3d_s222", "c3d_s221", "c3d_s122_b", "c3d_s211_b", "c3d_s121", "c3d_s222_depth1"])
def test_data_gradient_as_one_launch_gives_the_same_bits(name, dtype, monkeypatch):
    monkeypatch.setattr(FT, "_DG_PHASES", False)
    c = A.BY_NAME[name]
    rec = A.run_training_case(c, dtype, check_labels=False)
    opad = tuple(i - ((o - 1) * s - 2 * p + k) for i, o, s, p, k in zip(c.ext, c.odhw(), c.stride, c.pad, c.k))
    assert rec.labels == {"fwd:generic", "wgrad:plain", "wgrad:single", "dgrad:ct_outpad(%d,%d,%d)" % opad}


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("name", ["narrow_64_to_3", "narrow_32_to_5"])
def test_narrow_weight_gradient_without_swapped_roles_gives_the_same_bits(name, dtype, monkeypatch):
    monkeypatch.setattr(FT, "_WGRAD_SWAP", False)
    c = A.BY_NAME[name]
    rec = A.run_training_case(c, dtype, check_labels=False)
    assert rec.labels == (_non_run(c.want(dtype)) - {"wgrad:swapped"}) | {"wgrad:plain"}


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_stem_read_in_place_gives_the_same_bits(dtype, monkeypatch):
    monkeypatch.setattr(FS, "_STEM_FOLD", False)
    rec = A.run_training_case(A.BY_NAME["stem_folded"], dtype, check_labels=False)
    assert rec.labels == {"fwd:generic", "wgrad:plain", "wgrad:src_f32", "wgrad:single"}


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("name", ["ct_plain", "ct_plain_b", "ct_sn", "ct_wide_pad2"])
def test_transposed_convolution_as_one_launch_gives_the_same_bits(name, dtype, monkeypatch):
    monkeypatch.setattr(FS, "_CT_PHASES", False)
    rec = A.run_inference_case(A.BY_NAME[name], dtype, check_labels=False)
    assert rec.labels == {"run:generic"}


# ------------------------------------------------------------------ hand-over edges of backward
EDGE = ["c2d_3x3_s1_bias", "c2d_relu_bias_cl", "c3d_s222", "ct_plain", "ct_sn_frames3", "c2d_3x3_s1_bias_sn"]


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("name", EDGE)
def test_dy_as_a_non_contiguous_column_slice(name, dtype):
    A.run_training_case(A.BY_NAME[name], dtype, dy_mode="slice")


@pytest.mark.parametrize("name", EDGE)
def test_fp32_dy_into_a_bf16_op(name):
    A.run_training_case(A.BY_NAME[name], "bf16", dy_mode="f32")


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("name", ["c2d_3x3_s1_bias", "c3d_s222", "c3d_s121", "ct_plain", "narrow_32_to_5"])
def test_input_of_twice_the_pitch_gets_a_padded_data_gradient(name, dtype):
    c = A.BY_NAME[name]
    A.run_training_case(c, dtype, x_ld=2 * K.round_up(c.cin, K.e16(dtype)))


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("need", [(True, True, False), (True, False, True), (False, True, True), (False, False, True), (True, False, False)],
                         ids=["bias_frozen", "weight_frozen", "x_no_grad", "bias_only", "x_only"])
@pytest.mark.parametrize("name", ["c2d_3x3_s1_bias", "c2d_relu_bias_cl", "ct_sn_frames3", "c2d_3x3_s2_odd_sn"])
def test_only_the_gradients_asked_for(name, need, dtype):
    """a frozen weight launches no weight gradient, an input without grad no data gradient; the rest stays exact"""
    A.run_training_case(A.BY_NAME[name], dtype, need=need, check_labels=False)


def test_activation_on_an_fp32_output_raises_in_backward():
    c = A.BY_NAME["c2d_1x1_f32_rows"]
    o = A.operands(c)
    mod = A.build_module(c, o)
    xcl, _, _ = A.device_input(c, o, "bf16")
    out = FT.conv(mod, xcl, "bf16", act=_lib.ACT_RELU, out_f32=True)
    with pytest.raises(RuntimeError, match="fused activation on an fp32 output has no backward here"):
        out.t.backward(A.device_dy(c, o, "bf16"))


# ------------------------------------------------------------------ shared state
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("name", ["c2d_3x3_s1_bias", "c3d_s222", "narrow_64_to_3", "ct_sn", "ct_sn_frames3", "wgrad_slabs_32x32", "vgg_first_relu_src"])
def test_weight_gradient_on_the_side_stream_gives_the_same_bits(name, dtype):
    A.run_training_case(A.BY_NAME[name], dtype, ctx=FT.wgrad_side_stream(torch.cuda.Stream()))
    assert FT._WGRAD_SIDE["stream"] is None and FT._WGRAD_SIDE["params"] == []


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("side", [False, True], ids=["autograd", "side_stream"])
@pytest.mark.parametrize("prior", [False, True], ids=["fresh", "grad_populated"])
@pytest.mark.parametrize("name", ["c2d_3x3_s1_bias", "ct_plain"])
def test_one_weight_in_two_convolutions_sums_exactly(name, prior, side, dtype):
    """y1 = conv(x), y2 = conv(2 * flip(x)) with dy2 = flip(dy): dW = 3 dW_case, dbias = 2 dbias_case, on top of what ``.grad`` held"""
    import contextlib
    c = A.BY_NAME[name]
    o = A.operands(c)
    mod = A.build_module(c, o)
    w, b = A.weight_of(mod), mod.bias
    old_w = torch.full_like(w, 3.0) if prior else None
    old_b = torch.full_like(b, -5.0) if prior else None
    w.grad, b.grad = (None, None) if not prior else (old_w.clone(), old_b.clone())
    x1 = A.cl_of(o.x, dtype).to(DEV).requires_grad_(True)
    x2 = A.cl_of(2 * o.x.flip(0), dtype).to(DEV).requires_grad_(True)
    dy1, dy2 = A.cl_of(o.dy, dtype).to(DEV), A.cl_of(o.dy.flip(0), dtype).to(DEV)
    with (FT.wgrad_side_stream(torch.cuda.Stream()) if side else contextlib.nullcontext()):
        y1 = FT.conv(mod, K.CL(x1, c.N, c.ext, c.cin), dtype)
        y2 = FT.conv(mod, K.CL(x2, c.N, c.ext, c.cin), dtype)
        torch.autograd.backward([y1.t, y2.t], [dy1, dy2])
    torch.cuda.synchronize()
    A.assert_tensor_equal(w.grad, 3 * o.dw + (3.0 if prior else 0.0), f"{name} {dtype} shared dW")
    A.assert_tensor_equal(b.grad, 2 * o.db + (-5.0 if prior else 0.0), f"{name} {dtype} shared dbias")
    A.assert_cl_equal(x1.grad, o.dx, f"{name} {dtype} dX1")
    A.assert_cl_equal(x2.grad, o.dx.flip(0), f"{name} {dtype} dX2")
    assert not hasattr(w, "_side_grad")


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("name", ["c2d_3x3_s1_bias", "c3d_1x1_s2_even", "ct_plain"])
def test_operand_cache_follows_the_weight_version(name, dtype):
    """a cacheable case, the weight changed by an in-place torch op (version bump), the case again: the second result is the second
    reference; then once more behind ``clear_operand_cache()``"""
    c = A.BY_NAME[name]
    first, second = A.operands(c), A.operands(c, second=True)
    assert not torch.equal(first.w, second.w)
    FT.clear_operand_cache()
    rec = A.run_training_case(c, dtype, ops_=first)
    mod = rec.mod
    assert len(FT._OPCACHE) >= 2, "the case is not cacheable: forward and data-gradient operands were not kept"
    v0 = A.weight_of(mod)._version
    A.load_operands(mod, second)
    assert A.weight_of(mod)._version > v0
    A.run_training_case(c, dtype, ops_=second, mod=mod)
    A.run_training_case(c, dtype, ops_=second, mod=mod)          # (served from the cache: same version)
    A.load_operands(mod, first)
    FT.clear_operand_cache()
    assert len(FT._OPCACHE) == 0
    A.run_training_case(c, dtype, ops_=first, mod=mod)


def test_operand_cache_keeps_scopes_and_dtypes_apart():
    """one derived weight (not a parameter) under two scopes and two dtypes, interleaved: every call exact, one entry per key"""
    c = A.BY_NAME["c2d_3x3_s1_bias"]
    o = A.operands(c)
    FT.clear_operand_cache()
    w = o.w.to(torch.float32).to(DEV).requires_grad_(True)
    b = o.b.to(torch.float32).to(DEV).requires_grad_(True)
    for dtype, scope in [("bf16", 1), ("f32", 1), ("bf16", 2), ("f32", 2), ("bf16", 1), ("f32", 2)]:
        w.grad = b.grad = None
        x = A.cl_of(o.x, dtype).to(DEV).requires_grad_(True)
        y = FT.conv_weight(K.CL(x, c.N, c.ext, c.cin), w, b, c.k, c.stride, c.pad, dtype, scope=scope)
        A.assert_cl_equal(y.t, o.y, f"scope {scope} {dtype} y")
        y.t.backward(A.cl_of(o.dy, dtype).to(DEV))
        torch.cuda.synchronize()
        A.assert_cl_equal(x.grad, o.dx, f"scope {scope} {dtype} dX")
        A.assert_tensor_equal(w.grad, o.dw, f"scope {scope} {dtype} dW")
        A.assert_tensor_equal(b.grad, o.db, f"scope {scope} {dtype} dbias")
    keys = {(k[4], k[6]) for k in FT._OPCACHE if k[0] == w.data_ptr()}
    assert keys == {("bf16", 1), ("f32", 1), ("bf16", 2), ("f32", 2)}, keys
    assert len([k for k in FT._OPCACHE if k[0] == w.data_ptr()]) == 8          # forward and data-gradient operand per (dtype, scope)
    FT.clear_operand_cache()
