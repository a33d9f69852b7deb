"""The CPU side of tests/engine_exact.py: the yardsticks are re-measured and pinned, the reference is shown to be float64, the bounds are
shown to tell wrong wiring from rounding, and the input conditions the figures rely on are asserted.  Nothing here calls the library."""
import os

import numpy as np
import pytest
import torch

from tests import engine_exact as E
from tests.conftest import GOLDEN

F64 = torch.float64


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", E.CASES)
def test_yardsticks_are_the_recorded_ones(case, dtype):
    """the fp32 oracle / the bf16-operand oracle against float64 over seeds 1..4 and B = 1, 3, 4: measured <= recorded <= 2 x measured"""
    worst = E.measure_yardsticks(case, dtype)
    for q in E.QUANTITIES:
        rec = E.YARDSTICK[(case, dtype, q)]
        print(f"YARD {case} {dtype} {q} measured {worst[q]:.3e} recorded {rec:.3e} gpu bound {E.gpu_bound(case, dtype, q):.3e}")
    for q in E.QUANTITIES:
        rec = E.YARDSTICK[(case, dtype, q)]
        assert worst[q] <= rec <= 2.0 * worst[q], (case, dtype, q, worst[q], rec)


def test_yardstick_table_is_complete_and_f32_bounds_are_no_looser_than_the_end_to_end_ones():
    """One entry per (case, dtype, quantity), and the f32 bounds against test_flow_gpu.py's TOL["f32"] in ONE measure each, over every
    reference the GPU tests use.  logdet is absolute and grad relative in both files.  TOL's out and rev are absolute: the relative
    bound times max |ref| may exceed them (it does for out in most pairs: printed below), so the engine is held to both and the bound in force,
    min(8 x yardstick x max |ref|, TOL), is no looser by construction -- provided abs_bound really is TOL, and the cap is not below
    4 x the yardstick (the margin the per-kernel suites give), which would make it a bound read off nothing."""
    from tests.test_flow_gpu import TOL
    assert set(E.YARDSTICK) == {(c, d, q) for c in E.CASES for d in ("f32", "bf16") for q in E.QUANTITIES}
    assert E.abs_bound("f32", "out_abs") == TOL["f32"]["out"] and E.abs_bound("f32", "rev_abs") == TOL["f32"]["rev"]
    assert E.abs_bound("bf16", "out_abs") is None and E.abs_bound("f32", "dx_abs") is None
    binds = []
    for case in E.CASES:
        assert E.gpu_bound(case, "f32", "logdet") <= TOL["f32"]["logdet"] and E.gpu_bound(case, "f32", "grad") <= TOL["f32"]["grad"]
        assert E.gpu_bound(case, "f32", "dx") <= TOL["f32"]["grad"]         # (dx had no bound: held like the other gradients)
        for B in E.BATCHES + ((2, 5) if case == "plain" else ()):
            ref = E.reference(case, B)
            for q in ("out", "rev"):
                scale = float(ref[q].abs().max())
                relative_as_absolute = E.gpu_bound(case, "f32", q) * scale
                in_force = min(relative_as_absolute, E.abs_bound("f32", q + "_abs"))
                assert in_force <= TOL["f32"][q]
                assert TOL["f32"][q] >= 4.0 * E.YARDSTICK[(case, "f32", q)] * scale, (case, B, q)
                if relative_as_absolute > TOL["f32"][q]:
                    binds.append((case, B, q))
        for q in E.QUANTITIES:      # and the bf16 bounds stay far below an error of order one
            assert E.gpu_bound(case, "bf16", q) <= (0.7 if q == "logdet" else 0.06), (case, q)
    print("the absolute cap is the bound in force at", binds)
    assert all(q == "out" for _, _, q in binds)          # rev: the relative bound is the tighter one everywhere


@pytest.mark.parametrize("case", E.CASES)
def test_reference_is_float64_and_meets_the_input_conditions(case):
    """Every returned tensor is float64.  The conditions the figures rely on, for every reference the GPU tests use and every one the
    yardsticks are measured on: no ratio is taken over a vanishing tensor (|ref| max > 1e-3, every gradient tensor on its own), no affine
    scale tanh(s / 2) + 1 saturated (inside [0.05, 1.95]), max |logdet| inside what the flow goldens visit (g2, g2_lu, g16, g3: 74.6 ..
    1830.4; a floor of 20 keeps the absolute log-det figure meaningful)."""
    hi = []
    for name in ("g2_reduced_flow", "g2_reduced_flow_lu", "g16_condition_nice", "g3_full_flow_z32", "g3_full_flow_z64"):
        ld = np.abs(np.load(os.path.join(GOLDEN, name + ".npz"))["logdet"])
        hi.append(float(ld.max()))
    batches = E.BATCHES + ((2, 5) if case == "plain" else ())
    E.batched_reference(case)          # (the twelve draws of the yardsticks with one shared reverse pass)
    for seed in E.SEEDS:
        for B in (batches if seed == E.GPU_SEED else E.BATCHES):
            r = E.reference(case, B, seed)
            tensors = {"out": r["out"], "logdet": r["logdet"], "dx": r["dx"], "rev": r["rev"], **r["grads"]}
            for n, v in tensors.items():
                assert v.dtype == F64, (n, v.dtype)
                assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 1e-3, (case, B, seed, n)
            assert 0.05 < r["scale_min"] and r["scale_max"] < 1.95, (case, B, seed, r["scale_min"], r["scale_max"])
            assert 20.0 <= float(r["logdet"].abs().max()) <= max(hi), (case, B, seed)
            # the reverse pass of the reference inverts its forward pass, up to the reference's own guards: every ActNorm inverse
            # divides by exp(log_scale) + 1e-8 (1e-8 of the state per ActNorm, some forty of them)
            x = E.inputs(case, B, seed)[0].to(F64)
            assert float((r["rev"] - x).abs().max()) <= 1e-5


@pytest.mark.parametrize("case", ["plain", "use1x1"])
def test_reference_dx_agrees_with_a_central_finite_difference(case):
    """<dx, v> against (loss(x + h v) - loss(x - h v)) / 2h, h = 1e-6, one random direction: 1e-7 relative (only float64 gets there)"""
    B = 3
    r = E.reference(case, B)
    x, cond, d_out, dld = (t.to(F64) for t in E.inputs(case, B, E.GPU_SEED))
    m = E.typed_oracle(case, F64)
    # a standard normal direction, not normalised: the difference quotient's own rounding noise is ulp(loss) / h, about 4e-8 absolute,
    # and <dx, v> of a unit direction is below 1
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(77), dtype=F64)

    def loss(xx):
        with torch.no_grad():
            out, logdet = m(xx, cond)
            return float((out * d_out).sum() + (logdet * dld).sum())
    h = 1e-6
    fd = (loss(x + h * v) - loss(x - h * v)) / (2 * h)
    an = float((r["dx"] * v).sum())
    print(f"finite difference {fd!r}, <dx, v> {an!r}")
    assert abs(fd - an) <= 1e-7 * abs(an)
    assert abs(an) > 1e-2 * float(r["dx"].norm())       # (not a direction the loss is flat in)


@pytest.mark.parametrize("case", ["plain", "wide512"])
def test_bounds_discriminate_the_mutants(case):
    """Each wrong backward misses the float64 reference by at least 10 x the f32 bound in the quantity it must show up in."""
    B = 3
    ref = E.reference(case, B)
    ten = lambda q: 10.0 * E.gpu_bound(case, "f32", q)        # noqa: E731

    # d_logdet[0] used for every sample -> dx and the gradients
    mut = E.run_oracle(case, B, E.GPU_SEED, "f64", d_logdet=torch.full((B,), E.D_LOGDET[0]))
    e = E.errors(mut, ref)
    print(f"d_logdet[0] for all: dx {e['dx']:.3e} grad {e['grad']:.3e}")
    assert e["dx"] >= ten("dx") and e["grad"] >= ten("grad")
    assert e["out"] == 0.0 and e["logdet"] == 0.0              # (the forward pass is the reference's: the mutation is in the backward only)

    # the gradient state before the first op instead of after it (the other ping-pong buffer) -> dx
    e_dx = E.rel_err(ref["dx_after_first_op"], ref["dx"])
    print(f"other ping-pong buffer: dx {e_dx:.3e}")
    assert e_dx >= ten("dx")

    # one level's log-det term dropped from the backward -> the gradients of that level's ActNorm log scales (every one of them)
    for level in range(len(E.arch_of(case)["num_steps"])):
        mut = E.run_oracle(case, B, E.GPU_SEED, "f64", drop_level=level)
        ge = E.grad_errors(mut["grads"], ref)
        mine = {n: v for n, v in ge.items() if n.endswith("log_scale") and (f".layers.{level}." in n or f".priors.{level}." in n)}
        assert len(mine) >= 3
        print(f"level {level} log-det dropped: least log_scale gradient error {min(mine.values()):.3e} over {len(mine)} tensors")
        assert min(mine.values()) >= ten("grad"), (level, mine)
        assert E.rel_err(mut["dx"], ref["dx"]) >= ten("dx")     # (and the data gradient, through the log-det's dependence on the state)

    # d_out = out substituted for the independent draw -> everything: dx and every gradient tensor
    mut = E.run_oracle(case, B, E.GPU_SEED, "f64", d_out_is_out=True)
    ge = E.grad_errors(mut["grads"], ref)
    e_dx = E.rel_err(mut["dx"], ref["dx"])
    print(f"d_out = out: dx {e_dx:.3e}, least gradient tensor error {min(ge.values()):.3e}")
    assert e_dx >= ten("dx") and min(ge.values()) >= ten("grad"), min(ge, key=ge.get)


def test_bf16_operand_emulation_leaves_conv2d_as_it_was():
    """the replacement of F.conv2d is undone on exit, also after an exception, and rounds what it says it rounds"""
    import torch.nn.functional as F
    before = F.conv2d
    with pytest.raises(ZeroDivisionError):
        with E.bf16_conv_operands():
            assert F.conv2d is not before
            1 / 0
    assert F.conv2d is before
    x = torch.randn(1, 2, 4, 4, dtype=F64, requires_grad=True)
    w = torch.randn(3, 2, 1, 1, dtype=F64, requires_grad=True)
    with E.bf16_conv_operands():
        y = torch.nn.Conv2d(2, 3, 1, bias=False).double()(x)          # seven positional arguments
        y = F.conv2d(x, w)
    rb = lambda t: t.to(torch.bfloat16).to(F64)                        # noqa: E731
    assert torch.equal(y.detach(), F.conv2d(rb(x.detach()), rb(w.detach())))
    g = torch.randn_like(y)
    y.backward(g)
    xr = rb(x.detach()).requires_grad_(True)
    wr = rb(w.detach()).requires_grad_(True)
    F.conv2d(xr, wr).backward(rb(g))
    assert torch.equal(x.grad, xr.grad) and torch.equal(w.grad, wr.grad)
