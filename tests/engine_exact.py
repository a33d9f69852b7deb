"""The flow engine (csrc/flow_engine.hip: op program, workspace plan, gradient ping-pong, per-batch routing and tables, graph cache) held to
float64 as a whole: references, cases, error measure and bounds.  The test functions are in test_engine_exact_cpu.py (which measures and
pins the yardsticks, checks that the reference is float64 and that the bounds tell the mutants below from the real thing) and
test_engine_exact_gpu.py (which runs the engine).

* Reference: oracle/flow_ref.py's SupervisedMacowTransformer, filled by name (``deterministic_fill_``), in float64.  ``x`` requires grad,
  ``d_out`` is a normal draw independent of ``out``, ``d_logdet = [1, -0.5, 0, 0.25, -2][:B]`` (distinct per sample, a zero, both signs);
  loss = (out * d_out).sum() + (logdet * d_logdet).sum().  It returns out, logdet, dx, every parameter gradient and reverse(out).
  All runs of a case see the same float32-valued operands.
* Yardsticks: the same case run (a) by the oracle in float32 and (b) by the oracle in float64 with bf16 convolution operands
  (``F.conv2d`` replaced by G(conv2d(R(x), R(w))): R rounds to bf16 and passes the gradient, G rounds the incoming gradient to bf16).
  Both take the reference's ``out`` rounded to float32 as the input of the reverse pass, as the engine does; the twelve reverse passes
  of a yardstick run as one pass over their 32 samples (``reverse_batched``: samples do not see each other).
* Error measure (the existing engine tests' one): out, dx, the reverse and every gradient tensor -- worst |got - ref64| over the largest
  |ref64| of that tensor ("grad" is the worst tensor); logdet -- absolute.
* YARDSTICK[(case, dtype, quantity)]: the worst figure of the matching yardstick run over seeds 1..4 and B = 1, 3, 4, rounded up to two
  significant digits, on one thread (the fp32 sums of a convolution depend on the thread count).  Measured and pinned by test_engine_exact_cpu.py (measured <= recorded <= 2 x measured); none comes from the engine.
* gpu_bound: f32 8 x the yardstick (the engine's split-K partials, per-workgroup partial sums and matrix-core accumulation blocks add in
  another order than the oracle, the device's expf / tanhf / logf differ from the host's by a unit or two, and the yardstick is only the
  worst of twelve draws of the same rounding noise; the per-kernel suites give one kernel 4 x, a chain of about a hundred gets 8 x);
  bf16 2 x the yardstick (the yardstick already is a bf16 run of the whole chain, the engine another draw of the same noise; this dtype
  is here for the wiring, where an error is of order one).
* Against test_flow_gpu.py's TOL["f32"], like for like: logdet (absolute in both files) and grad (relative in both) are 8 to 100 times
  tighter.  TOL's out = 8e-5 and rev = 2e-4 are ABSOLUTE; times max |ref out| = 6.5 .. 12.5 the relative out bounds above come to
  as much as 1.3e-4, looser than 8e-5 in most of the (case, B) pairs the GPU tests use (the CPU test prints which; the rev bounds, at
  max |x| about 4, stay inside).  So the f32 engine is ALSO held to TOL's absolute figures for out and rev (``abs_bound``; printed as out_abs /
  rev_abs): the bound in force is the smaller of the two everywhere, and the cap still leaves 4 x the yardstick (the CPU test asserts
  both).

Cases, all on the 8 x 8 latent, B = 1, 3 and max_batch = 4, both dtypes:

    case            architecture                                               bf16 paths
    plain           configs.reduced_flow_arch()                                none of the fused launches (hidden 64)
    use1x1          + use1x1 (LU state of the oracle's constructor, seed 12)   the LU ops
    condition_nice  + condition_nice, h_channels = 32                          couplings that see the conditioning map
    wide512         flow_arch(16, hidden=512, num_steps=[1, 1], factor=4)      fused conv3 + coupling, the conv2 + conv3 pair, the
                                                                               paired data gradient, the fused units (at B = 1, 3, 4:
                                                                               WIDE_FUSED_B; the GPU test asserts the predicates)

Recorded yardsticks and the bounds derived from them (relative, logdet absolute):

    case / dtype           out               logdet            dx                grad              rev
    plain f32              1.3e-6 / 1.0e-5   4.4e-5 / 3.5e-4   9.8e-7 / 7.8e-6   2.4e-6 / 1.9e-5   1.9e-6 / 1.5e-5
    plain bf16             3.7e-3 / 7.4e-3   0.34 / 0.68       6.5e-3 / 1.3e-2   1.9e-2 / 3.8e-2   9.0e-3 / 1.8e-2
    use1x1 f32             9.4e-7 / 7.5e-6   3.9e-5 / 3.1e-4   1.1e-6 / 8.8e-6   2.8e-6 / 2.2e-5   3.7e-6 / 3.0e-5
    use1x1 bf16            4.1e-3 / 8.2e-3   0.13 / 0.26       5.6e-3 / 1.2e-2   1.7e-2 / 3.4e-2   1.7e-2 / 3.4e-2
    condition_nice f32     1.1e-6 / 8.8e-6   4.7e-5 / 3.8e-4   1.2e-6 / 9.6e-6   2.7e-6 / 2.2e-5   3.1e-6 / 2.5e-5
    condition_nice bf16    6.4e-3 / 1.3e-2   0.092 / 0.19      8.7e-3 / 1.8e-2   2.8e-2 / 5.6e-2   2.9e-2 / 5.8e-2
    wide512 f32            9.7e-7 / 7.8e-6   3.9e-5 / 3.1e-4   8.2e-7 / 6.6e-6   1.6e-6 / 1.3e-5   1.3e-6 / 1.0e-5
    wide512 bf16           2.6e-3 / 5.2e-3   0.088 / 0.18      2.8e-3 / 5.6e-3   1.2e-2 / 2.4e-2   4.7e-3 / 9.4e-3
    (yardstick / GPU bound; f32 out and rev are held to 8e-5 / 2e-4 absolute as well)
"""
import copy

import numpy as np
import torch

from ipoke_amd import configs
from ipoke_amd.utils.detfill import deterministic_fill_

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16

BATCHES = (1, 3, 4)
MAX_BATCH = 4
SEEDS = (1, 2, 3, 4)
GPU_SEED = 1                       # the GPU tests' draw (one of the yardstick's)
D_LOGDET = (1.0, -0.5, 0.0, 0.25, -2.0)
QUANTITIES = ("out", "logdet", "dx", "grad", "rev")
CASES = ("plain", "use1x1", "condition_nice", "wide512")
WIDE_FUSED_B = BATCHES             # every predicate accepts at M = 64, 192, 256 (asserted by the GPU test)
LU_SEED = 12


def arch_of(case):
    if case == "wide512":
        return configs.flow_arch(16, hidden=512, num_steps=[1, 1], factor=4)
    arch = configs.reduced_flow_arch()
    if case == "use1x1":
        arch["use1x1"] = True
    elif case == "condition_nice":
        arch["condition_nice"] = True
        arch["h_channels"] = 32
    elif case != "plain":
        raise KeyError(case)
    return arch


_oracles = {}
_typed = {}            # (case, dtype) -> the oracle in that dtype


def oracle(case):
    """the float32 oracle of a case with its weights (built once; never modified: the runs work on copies)"""
    if case not in _oracles:
        from oracle import flow_ref
        state = np.random.get_state()
        try:
            np.random.seed(LU_SEED)
            o = flow_ref.SupervisedMacowTransformer(copy.deepcopy(arch_of(case)))
        finally:
            np.random.set_state(state)
        lu_state = {k: v.clone() for k, v in o.state_dict().items() if ".shuffle_layers." in k}
        deterministic_fill_(o, prefix="flow.")
        if case == "use1x1":       # the constructor's P, L, U draws (a name-keyed fill is not a permutation)
            o.load_state_dict(lu_state, strict=False)
        _oracles[case] = o.eval()
    return _oracles[case]


def typed_oracle(case, dt):
    """the oracle of a case in float32 / float64 (one copy per dtype; the runs leave its weights alone)"""
    if (case, dt) not in _typed:
        _typed[(case, dt)] = copy.deepcopy(oracle(case)).to(dt)
    return _typed[(case, dt)]


def inputs(case, B, seed):
    """x, cond, d_out, d_logdet of a run: float32 values, the same for the reference, the yardstick runs and the engine"""
    arch = arch_of(case)
    gen = torch.Generator().manual_seed(1000 * seed + 10 * CASES.index(case) + B)
    x = torch.randn(B, arch["flow_in_channels"], 8, 8, generator=gen)
    cond = torch.randn(B, arch["h_channels"], 8, 8, generator=gen)
    d_out = torch.randn(B, arch["flow_in_channels"], 8, 8, generator=gen)
    return x, cond, d_out, torch.tensor(D_LOGDET[:B])


# ------------------------------------------------------------------ bf16 convolution operands
class _RoundOperand(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(BF16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g.to(BF16).to(g.dtype)


class bf16_conv_operands:
    """with-block: every F.conv2d inside takes its input and weight rounded to bf16 and hands a bf16-rounded gradient back"""

    def __enter__(self):
        from oracle import flow_ref
        self._F, self._conv2d = flow_ref.F, flow_ref.F.conv2d
        conv2d = self._conv2d

        def rounded(x, w, *args, **kw):         # nn.Conv2d passes seven positional arguments
            return _RoundGradient.apply(conv2d(_RoundOperand.apply(x), _RoundOperand.apply(w), *args, **kw))
        self._F.conv2d = rounded
        return self

    def __exit__(self, *exc):
        self._F.conv2d = self._conv2d
        return False


# ------------------------------------------------------------------ the oracle's runs
def run_oracle(case, B, seed, mode, *, d_logdet=None, d_out_is_out=False, drop_level=None, rev_in=None, record=None, reverse=True):
    """One run of the case: mode "f64" (the reference), "f32" or "bf16" (float64 with bf16 convolution operands).

    Returns {"out", "logdet", "dx", "rev", "grads": {name: tensor}, "dx_after_first_op"} in the run's dtype.  rev_in: the input of the
    reverse pass (default: this run's out).  The keyword mutations are the CPU test's: another d_logdet, d_out = out, the log-det terms
    of one level detached (dropped from the backward).  record: a dict that receives the range of the affine scales.  reverse=False
    leaves the reverse pass out ("rev" is None: reverse_batched makes the twelve of a yardstick in one pass)."""
    from oracle import flow_ref
    dt = F32 if mode == "f32" else F64
    m = typed_oracle(case, dt)
    for p in m.parameters():
        p.grad = None               # (the gradients of an earlier run stay with whoever holds them)
    x, cond, d_out, dld = inputs(case, B, seed)
    x, cond, d_out = x.to(dt).requires_grad_(True), cond.to(dt), d_out.to(dt)
    dld = (dld if d_logdet is None else d_logdet).to(dt)
    hooks, first = [], {}

    def keep_first(mod, args, output):          # the gradient state after the first op (ActNorm) of the program
        if isinstance(output, tuple) and output[0].requires_grad:      # (not the reverse pass)
            first["y"] = output[0]
            output[0].retain_grad()
    hooks.append(m.flow.layers[0][0].actnorm1.register_forward_hook(keep_first))
    if drop_level is not None:
        drop = lambda mod, args, output: (output[0], output[1].detach()) if isinstance(output, tuple) else None    # noqa: E731
        for mod in list(m.flow.layers[drop_level]) + [m.flow.priors[drop_level]]:
            hooks.append(mod.register_forward_hook(drop))
    affine_params = flow_ref.affine_params
    if record is not None:
        def recording(raw):
            mu, scale = affine_params(raw)
            s = scale.detach()
            record["scale_min"] = min(record.get("scale_min", 2.0), float(s.min()))
            record["scale_max"] = max(record.get("scale_max", 0.0), float(s.max()))
            return mu, scale
        flow_ref.affine_params = recording
    try:
        ctx = bf16_conv_operands() if mode == "bf16" else torch.enable_grad()
        with ctx:
            out, logdet = m(x, cond)
            if d_out_is_out:
                d_out = out.detach()
            ((out * d_out).sum() + (logdet * dld).sum()).backward()
            rev = None
            if reverse:
                with torch.no_grad():
                    z = out.detach() if rev_in is None else rev_in.to(dt)
                    rev = m(z, cond, reverse=True)
    finally:
        flow_ref.affine_params = affine_params
        for h in hooks:
            h.remove()
    return {"out": out.detach(), "logdet": logdet.detach(), "dx": x.grad, "rev": rev,
            "grads": {n: p.grad for n, p in m.named_parameters()}, "dx_after_first_op": first["y"].grad}


_refs = {}


def reference(case, B, seed=GPU_SEED):
    """the float64 run, computed once per (case, B, seed) and shared (never modified)"""
    key = (case, B, seed)
    if key not in _refs:
        rec = {}
        r = run_oracle(case, B, seed, "f64", record=rec)
        r.update(rec)
        _refs[key] = r
    return _refs[key]


GROUPS = tuple((seed, B) for seed in SEEDS for B in BATCHES)       # the twelve draws a yardstick is the worst of


def reverse_batched(case, mode, outs):
    """The reverse passes of the twelve draws in ONE pass over their 32 samples (the samples of a batch do not see each other; the walk
    over rows and columns makes the reverse the most expensive pass of a run): outs {(seed, B): the pass's input} -> {(seed, B): rev}"""
    dt = F32 if mode == "f32" else F64
    m = typed_oracle(case, dt)
    z = torch.cat([outs[g] for g in GROUPS]).to(dt)
    cond = torch.cat([inputs(case, B, seed)[1] for seed, B in GROUPS]).to(dt)
    with torch.no_grad(), (bf16_conv_operands() if mode == "bf16" else torch.no_grad()):
        rev = m(z, cond, reverse=True)
    res, lo = {}, 0
    for seed, B in GROUPS:
        res[(seed, B)] = rev[lo:lo + B]
        lo += B
    return res


def batched_reference(case):
    """the float64 runs of all twelve draws {(seed, B): reference}: those reference() has not made yet are made with one shared
    reverse pass; all of them are reference()'s afterwards"""
    missing = [g for g in GROUPS if (case, g[1], g[0]) not in _refs]
    if missing:
        new = {}
        for seed, B in missing:
            rec = {}
            new[(seed, B)] = run_oracle(case, B, seed, "f64", record=rec, reverse=False)
            new[(seed, B)].update(rec)
        outs = {g: (new[g]["out"] if g in new else _refs[(case, g[1], g[0])]["out"]) for g in GROUPS}
        rev = reverse_batched(case, "f64", outs)
        for (seed, B), r in new.items():
            r["rev"] = rev[(seed, B)]
            _refs[(case, B, seed)] = r
    return {(seed, B): _refs[(case, B, seed)] for seed, B in GROUPS}


# ------------------------------------------------------------------ error measure
def rel_err(got, ref64):
    """worst |got - ref| over the largest |ref| of the tensor"""
    return float((got.detach().to(F64).cpu() - ref64).abs().max() / ref64.abs().max())


def grad_errors(grads, ref):
    """{name: rel_err} over the reference's parameters (grads: name -> tensor, every name of the reference must be there)"""
    return {n: rel_err(grads[n], g) for n, g in ref["grads"].items()}


def errors(got, ref):
    """{quantity: figure} of a run against the reference (got: the keys of run_oracle; absent ones are left out)"""
    e = {}
    for q in ("out", "dx", "rev"):
        if got.get(q) is not None:
            e[q] = rel_err(got[q], ref[q])
            if q != "dx":
                e[q + "_abs"] = float((got[q].detach().to(F64).cpu() - ref[q]).abs().max())
    if got.get("logdet") is not None:
        e["logdet"] = float((got["logdet"].detach().to(F64).cpu() - ref["logdet"]).abs().max())
    if got.get("grads") is not None:
        e["grad"] = max(grad_errors(got["grads"], ref).values())
    return e


def round_up_2(v):
    """v rounded up to two significant digits"""
    if v <= 0:
        return 0.0
    e = int(np.floor(np.log10(v))) - 1
    return float(f"{np.ceil(v / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e:.1e}")


def measure_yardsticks(case, dtype):
    """{quantity: worst figure of the yardstick run of a dtype ("f32" / "bf16") over SEEDS x BATCHES}; its reverse pass starts from the
    reference's out rounded to float32"""
    ref = batched_reference(case)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # the fp32 sums of a convolution depend on how many threads share them: up to 27 % of a figure
    try:
        run = {(seed, B): run_oracle(case, B, seed, dtype, reverse=False) for seed, B in GROUPS}
        rev = reverse_batched(case, dtype, {g: ref[g]["out"].to(F32) for g in GROUPS})
    finally:
        torch.set_num_threads(threads)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for g in GROUPS:
        run[g]["rev"] = rev[g]
        e = errors(run[g], ref[g])
        for q in QUANTITIES:
            worst[q] = max(worst[q], e[q])
    return worst


# (case, dtype, quantity) -> recorded yardstick
YARDSTICK = {
    ("plain", "f32", "out"): 1.3e-06, ("plain", "f32", "logdet"): 4.4e-05, ("plain", "f32", "dx"): 9.8e-07,
    ("plain", "f32", "grad"): 2.4e-06, ("plain", "f32", "rev"): 1.9e-06,
    ("plain", "bf16", "out"): 0.0037, ("plain", "bf16", "logdet"): 0.34, ("plain", "bf16", "dx"): 0.0065,
    ("plain", "bf16", "grad"): 0.019, ("plain", "bf16", "rev"): 0.009,
    ("use1x1", "f32", "out"): 9.4e-07, ("use1x1", "f32", "logdet"): 3.9e-05, ("use1x1", "f32", "dx"): 1.1e-06,
    ("use1x1", "f32", "grad"): 2.8e-06, ("use1x1", "f32", "rev"): 3.7e-06,
    ("use1x1", "bf16", "out"): 0.0041, ("use1x1", "bf16", "logdet"): 0.13, ("use1x1", "bf16", "dx"): 0.0056,
    ("use1x1", "bf16", "grad"): 0.017, ("use1x1", "bf16", "rev"): 0.017,
    ("condition_nice", "f32", "out"): 1.1e-06, ("condition_nice", "f32", "logdet"): 4.7e-05, ("condition_nice", "f32", "dx"): 1.2e-06,
    ("condition_nice", "f32", "grad"): 2.7e-06, ("condition_nice", "f32", "rev"): 3.1e-06,
    ("condition_nice", "bf16", "out"): 0.0064, ("condition_nice", "bf16", "logdet"): 0.092, ("condition_nice", "bf16", "dx"): 0.0087,
    ("condition_nice", "bf16", "grad"): 0.028, ("condition_nice", "bf16", "rev"): 0.029,
    ("wide512", "f32", "out"): 9.7e-07, ("wide512", "f32", "logdet"): 3.9e-05, ("wide512", "f32", "dx"): 8.2e-07,
    ("wide512", "f32", "grad"): 1.6e-06, ("wide512", "f32", "rev"): 1.3e-06,
    ("wide512", "bf16", "out"): 0.0026, ("wide512", "bf16", "logdet"): 0.088, ("wide512", "bf16", "dx"): 0.0028,
    ("wide512", "bf16", "grad"): 0.012, ("wide512", "bf16", "rev"): 0.0047,
}

GPU_FACTOR = {"f32": 8.0, "bf16": 2.0}


def gpu_bound(case, dtype, quantity):
    return GPU_FACTOR[dtype] * YARDSTICK[(case, dtype, quantity)]


def abs_bound(dtype, quantity):
    """the absolute bound on "out_abs" / "rev_abs": test_flow_gpu.py's TOL["f32"] for out / rev (f32 only; None: not held)"""
    if dtype != "f32" or quantity not in ("out_abs", "rev_abs"):
        return None
    from tests.test_flow_gpu import TOL
    return TOL["f32"][quantity[:-4]]
