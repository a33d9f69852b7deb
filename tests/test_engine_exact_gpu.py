"""The flow engine as a whole against the float64 reference of tests/engine_exact.py: cotangents that differ per sample and the input
gradient (a), the backward in pieces (b), one engine taken through a sequence of batch sizes, eagerly and with captured graphs (c), a
reverse pass between a training forward and its backward (d), and the state / batch guards of the C boundary (e).  Every figure is
printed as ``ENGFIG case dtype B quantity error bound`` before it is asserted."""
import copy
import ctypes

import pytest
import torch

from tests import engine_exact as E

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -3          # ipoke_status of include/ipoke_hip.h


def build(case, dtype, max_batch=E.MAX_BATCH):
    """the engine of a case with the oracle's weights, permutations and LU state"""
    from ipoke_amd.flow import SupervisedMacowTransformer
    m = SupervisedMacowTransformer(copy.deepcopy(E.arch_of(case)), dtype=dtype, max_batch=max_batch, device="cuda", init="none")
    m.load_state_dict(E.oracle(case).state_dict())
    m.sync_buffers()
    assert m._initialized
    return m


def cuda_inputs(case, B, seed=E.GPU_SEED):
    return tuple(t.cuda() for t in E.inputs(case, B, seed))


def engine_pass(m, case, B, train_mode=True, between=None):
    """Training forward + backward through the module call under the cotangents of the case, x requiring grad.  The flat gradient buffer
    is filled with NaN first: the engine writes every parameter gradient exactly once, an unwritten one stays NaN and misses every bound.
    between: called after the forward pass, before the backward."""
    x, cond, d_out, dld = cuda_inputs(case, B)
    x.requires_grad_(True)
    m.train(train_mode)
    m.flat_grads.fill_(float("nan"))
    out, logdet = m(x, cond)
    assert out.requires_grad and logdet.requires_grad
    if between is not None:
        between()
    ((out * d_out).sum() + (logdet * dld).sum()).backward()
    torch.cuda.synchronize()
    flat = m.flat_grads.clone()
    grads = {}
    for name, off, shape, kind in m.engine.tensors:
        if kind == 0:
            n = 1
            for s in shape:
                n *= s
            grads[name] = flat[off:off + n].view(shape)
    return {"out": out.detach().clone(), "logdet": logdet.detach().clone(), "dx": x.grad.clone(), "grads": grads, "flat": flat}


def engine_reverse(m, case, B):
    """the engine's reverse pass of the reference's out (rounded to float32)"""
    cond = cuda_inputs(case, B)[1]
    return m(E.reference(case, B)["out"].to(torch.float32).cuda(), cond, reverse=True).clone()


def hold(case, dtype, B, got, ref, what=""):
    """print every figure, then assert each against gpu_bound -- f32 out and rev also, in absolute terms, against abs_bound (a NaN misses)"""
    assert set(got.get("grads", ref["grads"])) == set(ref["grads"])
    e = E.errors(got, ref)
    missed = []
    for q, v in e.items():
        bound = E.abs_bound(dtype, q) if q.endswith("_abs") else E.gpu_bound(case, dtype, q)
        if bound is None:
            continue
        print(f"ENGFIG {case} {dtype} {B} {q} {v:.3e} {bound:.3e}{what}")
        if not v <= bound:
            missed.append((q, v, bound))
    if any(q == "grad" for q, _, _ in missed):
        ge = E.grad_errors(got["grads"], ref)
        bound = E.gpu_bound(case, dtype, "grad")
        missed.append(("gradient tensors", sorted(((v, n) for n, v in ge.items() if not v <= bound), reverse=True)[:6]))
    assert not missed, (case, dtype, B, what, missed)


def noise_rule(got, ref, again, what):
    """test_backward_in_pieces_matches_and_covers_all_parameters' rule: within 4 x the run-to-run noise of the one-shot pass (the split-K
    data gradients may accumulate with fp32 atomics), or 1e-6 of the largest entry"""
    noise = (again - ref).abs().max().item()
    diff = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{what}: diff {diff:.3e}, noise {noise:.3e}, scale {scale:.3e}")
    assert diff <= max(4 * noise, 1e-6 * scale), (what, diff, noise, scale)


def coupling_widths(m):
    """[(cin, cout)] of the engine's coupling nets, from the shapes of conv1's and conv3's weights"""
    shapes = {name: shape for name, off, shape, kind in m.engine.tensors if kind == 0}
    out = []
    for name, shape in shapes.items():
        if name.endswith(".net.conv1.weight"):
            v = shapes[name[: -len("conv1.weight")] + "conv3.conv.weight_v"]
            out.append((shape[1], v[0] // 2))
    return out


def assert_fused_paths_apply(m, B):
    """wide512 in bf16: the fused launches take this batch size (the predicates with the arguments the engine passes at M = 64 B, hidden 512)"""
    import os
    from ipoke_amd import _lib
    L = _lib.lib()
    # The predicates say that the shapes are eligible; the engine's own switches are not readable through the boundary, so what they
    # hang on is asserted here: unit_split is kDefaultUnitSplit = 4 unless IPOKE_UNIT_SPLIT says otherwise (1 would take the two-unit
    # launches away), coupling_fuse is bf16 and the split-K predicate at M = 64 (below), c2_straight is bf16 and hidden % 64 == 0, and
    # the paired data gradient also wants condition_nice off.
    assert os.environ.get("IPOKE_UNIT_SPLIT") is None, "IPOKE_UNIT_SPLIT is set: the engine's default row split (4) is assumed here"
    assert m.engine.dtype_name == "bf16" and m.engine.cfg.hidden % 64 == 0 and not m.engine.cfg.condition_nice
    hidden, M = m.engine.cfg.hidden, 64 * B
    acc_bytes = L.ipoke_conv_acc_scratch_bytes(m.engine.max_batch * 64, 64, 32)
    widths = coupling_widths(m)
    # two levels of one step (four couplings) and a prior: (cin, cout) = (8, 8) x 4, (12, 4), (6, 6) x 4, (8, 4)
    assert sorted(widths) == sorted([(8, 8)] * 4 + [(12, 4)] + [(6, 6)] * 4 + [(8, 4)]) and hidden == 512
    assert L.ipoke_conv3x3_coupling_splitk(64, hidden, _lib.BF16) > 0                # (the engine's switch at creation)
    assert L.ipoke_conv3x3_coupling_splitk(M, hidden, _lib.BF16) > 0                 # conv3 + coupling in one launch
    for cin, cout in widths:
        assert L.ipoke_conv_pair_coupling_applicable(M, hidden, 2 * cout, _lib.BF16) == 1, (B, cout)     # conv2 + conv3 + coupling
        assert L.ipoke_conv_pair_dgrad_applicable(M, hidden, cin, _lib.BF16, acc_bytes) == 1, (B, cin)    # conv2 + conv1 data gradients
    for C in (16, 12):                                                               # two units per launch, forward and backward
        assert L.ipoke_macow_unit2_applicable(C, m.engine.cond_channels, _lib.BF16, 4, 0) == 1
        assert L.ipoke_macow_unit2_applicable(C, m.engine.cond_channels, _lib.BF16, 4, 1) == 1


# ------------------------------------------------------------------ a. cotangents and dx
@pytest.mark.parametrize("B", E.BATCHES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", E.CASES)
def test_cotangents_and_input_gradient(case, dtype, B):
    """out, logdet, every parameter gradient (read from the flat buffer), x.grad and the reverse of the reference's out, under an
    independent d_out and a d_logdet that differs per sample, in train() and in eval() with grad enabled (the input.requires_grad branch
    of SupervisedMacowTransformer.forward)."""
    ref = E.reference(case, B)
    m = build(case, dtype)
    if case == "wide512" and dtype == "bf16":
        assert B in E.WIDE_FUSED_B
        assert_fused_paths_apply(m, B)
    for train_mode in (True, False):
        got = engine_pass(m, case, B, train_mode)
        got["rev"] = engine_reverse(m, case, B)
        hold(case, dtype, B, got, ref, "" if train_mode else " (eval)")
    assert m.engine.handoff_timeouts() == (0, 0)


# ------------------------------------------------------------------ b. pieces
@pytest.mark.parametrize("case", ["plain", "use1x1"])
def test_backward_in_pieces_keeps_dx_and_the_gradients(case):
    """the same backward through grad_ready_hook at 2 pieces and at one piece per unit: the announced ranges cover every parameter once,
    dx and the gradients stay within the float64 bounds, and dx equals the one-shot dx by the noise rule"""
    from ipoke_amd import _lib
    dtype, B = "f32", 3
    ref = E.reference(case, B)
    m = build(case, dtype)
    one = engine_pass(m, case, B)
    again = engine_pass(m, case, B)
    hold(case, dtype, B, one, ref, " (one shot)")
    L = _lib.lib()
    nr = L.ipoke_flow_piece_ranges(m.engine.handle, 1 << 20, None, 0)
    buf = (ctypes.c_int64 * (3 * nr))()
    assert L.ipoke_flow_piece_ranges(m.engine.handle, 1 << 20, buf, nr) == nr
    units = len({buf[3 * i] for i in range(nr)})
    assert units > 2
    for n in (2, units):
        ranges = []
        m.engine.grad_ready_hook = (n, torch.cuda.Stream(), lambda b, e: ranges.append((b, e)))
        try:
            got = engine_pass(m, case, B)
        finally:
            m.engine.grad_ready_hook = None
        assert len(ranges) >= n
        covered = torch.zeros(m.engine.n_params, dtype=torch.int32)
        for b, e in ranges:
            covered[b:e] += 1
        assert int(covered.min()) == 1 and int(covered.max()) == 1
        hold(case, dtype, B, got, ref, f" ({n} pieces)")
        noise_rule(got["dx"], one["dx"], again["dx"], f"{case} dx at {n} pieces")
        noise_rule(got["flat"], one["flat"], again["flat"], f"{case} gradients at {n} pieces")


# ------------------------------------------------------------------ c. one engine through a batch sequence
SEQUENCE = (3, 1, 5, 2, 4, 1, 3)           # training sizes: five distinct ones (the staging buffers hold four), 1 and 3 revisited
INFERENCE = (5, 2, 4, 1, 3, 5, 2)          # the no_grad forward + reverse behind each, at another size; 5 and 2 revisited


def _inference(m, case, B):
    with torch.no_grad():
        x, cond = cuda_inputs(case, B)[:2]
        m.eval()
        out, logdet = m(x, cond)
        return {"out": out.clone(), "logdet": logdet.clone(), "rev": engine_reverse(m, case, B)}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("out", "logdet", "rev"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_engine_through_a_batch_sequence(dtype):
    """ensure_tables, make_plan, the staging buffers' eviction, the one-workspace-per-mode rule and require_saved_forward on a live
    engine: every training pass is held to float64, the inference passes are bit-equal on a revisit and to a freshly built flow, first
    eagerly, then in graph mode with three calls per visit -- by with_graph's rule eager, capture, replay.  That a capture and a replay
    took place is assumed, not observed: the boundary has no replay counter, and an entry whose capture failed stays eager for good and
    would give the same bits.  What is asserted is that graph mode, whatever it launched, returns the eager results across the batch
    changes.  The backward is never captured."""
    case, max_batch = "plain", 5
    assert all(a != b for a, b in zip(SEQUENCE, INFERENCE)) and len(set(SEQUENCE)) == 5 > 4
    m = build(case, dtype, max_batch)
    first = {}
    for B, Bi in zip(SEQUENCE, INFERENCE):
        hold(case, dtype, B, engine_pass(m, case, B), E.reference(case, B), " (sequence)")
        got = _inference(m, case, Bi)
        hold(case, dtype, Bi, got, E.reference(case, Bi), " (sequence, no_grad)")
        if Bi in first:
            assert _same(got, first[Bi]), f"revisit of B = {Bi} differs from its first visit"
        else:
            first[Bi] = got
    for Bi, want in first.items():
        assert _same(_inference(build(case, dtype, max_batch), case, Bi), want), f"B = {Bi} differs from a freshly built flow"
    assert m.engine.handoff_timeouts() == (0, 0)
    for B, Bi in zip(SEQUENCE, INFERENCE):
        m.set_graph_mode(False)
        hold(case, dtype, B, engine_pass(m, case, B), E.reference(case, B), " (graph sequence)")
        m.set_graph_mode(True)
        try:
            for call in range(3):
                assert _same(_inference(m, case, Bi), first[Bi]), f"graph mode, B = {Bi}, call {call} differs from the eager result"
        finally:
            m.set_graph_mode(False)
    assert m.engine.handoff_timeouts() == (0, 0)


# ------------------------------------------------------------------ d. a reverse between a training forward and its backward
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", E.CASES)
def test_reverse_between_forward_and_backward_changes_nothing(case, dtype):
    """the evaluation and training workspaces are separate and the backward reads none of the staging buffers the reverse overwrites"""
    B = 3
    m = build(case, dtype)
    z, cond2 = cuda_inputs(case, B, seed=2)[2], cuda_inputs(case, B, seed=2)[1]
    alone = m(z, cond2, reverse=True).clone()
    base = engine_pass(m, case, B)
    again = engine_pass(m, case, B)
    seen = {}
    got = engine_pass(m, case, B, between=lambda: seen.setdefault("rev", m(z, cond2, reverse=True).clone()))
    assert torch.equal(seen["rev"], alone)
    assert torch.equal(got["out"], base["out"]) and torch.equal(got["logdet"], base["logdet"])
    noise_rule(got["dx"], base["dx"], again["dx"], f"{case} {dtype} dx")
    noise_rule(got["flat"], base["flat"], again["flat"], f"{case} {dtype} gradients")
    hold(case, dtype, B, got, E.reference(case, B), " (reverse in between)")


# ------------------------------------------------------------------ e. the state guards through the C boundary
def test_state_and_batch_guards_refuse_before_anything_is_queued():
    """require_saved_forward (IPOKE_ERR_STATE) and common_checks (IPOKE_ERR_INVALID) return before a launch: every caller buffer keeps its
    sentinel, the engine's state survives the refused calls, and a valid backward afterwards is right.  A backward at B = 0 or
    max_batch + 1 is refused by require_saved_forward (no forward at that size can have succeeded), so its code is IPOKE_ERR_STATE."""
    from ipoke_amd import _lib
    from ipoke_amd._lib import ptr
    case, dtype, max_batch = "plain", "f32", E.MAX_BATCH
    m = build(case, dtype)
    eng, L = m.engine, _lib.lib()
    eng.prepare_weights()
    h, stream = eng.handle, _lib.current_stream()
    z, cc, rows = eng.z, eng.cond_channels, max_batch + 1            # every buffer holds max_batch + 1 samples
    SENT = -7.25
    full = lambda *shape: torch.full(shape, SENT, dtype=torch.float32, device="cuda")      # noqa: E731
    nws = 2 * max(L.ipoke_flow_workspace_bytes(h, max_batch, 1), L.ipoke_flow_workspace_bytes(h, max_batch, 0))
    assert nws > 0
    ws = torch.full((nws,), 0x5A, dtype=torch.uint8, device="cuda")
    xin, cin = torch.randn(rows, z, 8, 8, device="cuda"), torch.randn(rows, cc, 8, 8, device="cuda")
    d_out, d_ld = torch.randn(rows, z, 8, 8, device="cuda"), torch.randn(rows, device="cuda")
    out, logdet, dx, grads = full(rows, z, 8, 8), full(rows), full(rows, z, 8, 8), full(eng.n_params)

    def forward(B, save, x=xin, cond=cin, o=out, ld=logdet, w=ws):
        return L.ipoke_flow_forward(h, ptr(eng.params), ptr(eng.perm), ptr(eng.shadow), ptr(x), ptr(cond), B, ptr(o), ptr(ld), ptr(w), save, stream)

    def reverse(B):
        return L.ipoke_flow_reverse(h, ptr(eng.params), ptr(eng.perm), ptr(eng.shadow), ptr(xin), ptr(cin), B, ptr(out), ptr(ws), stream)

    def backward(B, do=d_out, dl=d_ld, g=grads, d=dx, w=ws):
        return L.ipoke_flow_backward(h, ptr(eng.params), ptr(eng.perm), ptr(eng.shadow), ptr(do), ptr(dl), B, ptr(g), ptr(d), ptr(w), stream)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in (out, logdet, dx, grads)) and bool((ws == 0x5A).all())

    # scratch buffers for the calls that are meant to run (their results are not looked at, but for the last one)
    o2, ld2, ws2 = torch.empty_like(out), torch.empty_like(logdet), torch.empty_like(ws)
    assert backward(3) == ERR_STATE and untouched()                               # before any forward
    assert forward(3, 0, o=o2, ld=ld2, w=ws2) == 0
    assert backward(3) == ERR_STATE and untouched()                               # after a forward that saved nothing
    assert forward(3, 1, o=o2, ld=ld2, w=ws2) == 0
    scratch_params = eng.params.detach().clone()                                  # (the initialisation pass rewrites parameters)
    assert L.ipoke_flow_init_forward(h, ptr(scratch_params), ptr(eng.perm), ptr(xin), 3, ptr(o2), ptr(ld2), ptr(ws2), stream) == 0
    assert backward(3) == ERR_STATE and untouched()                               # after ipoke_flow_init_forward
    x2, cond2, d_out2, d_ld2 = cuda_inputs(case, 2)
    assert forward(2, 1, x=x2.contiguous(), cond=cond2.contiguous(), o=o2, ld=ld2, w=ws2) == 0
    assert backward(3) == ERR_STATE and untouched()                               # after a training forward at another B
    for B in (0, max_batch + 1):
        assert forward(B, 0) == ERR_INVALID and forward(B, 1) == ERR_INVALID and untouched(), B
        assert reverse(B) == ERR_INVALID and untouched(), B
        assert backward(B) == ERR_STATE and untouched(), B
    # the saved forward at B = 2 still stands: its backward succeeds and is the reference's
    g2, dx2 = torch.full_like(grads, float("nan")), torch.empty(2, z, 8, 8, device="cuda")
    assert backward(2, do=d_out2.contiguous(), dl=d_ld2.contiguous(), g=g2, d=dx2, w=ws2) == 0
    torch.cuda.synchronize()
    assert untouched()
    got = {"out": o2[:2], "logdet": ld2[:2], "dx": dx2, "grads": {}}
    for name, off, shape, kind in eng.tensors:
        if kind == 0:
            n = 1
            for s in shape:
                n *= s
            got["grads"][name] = g2[off:off + n].view(shape)
    hold(case, dtype, 2, got, E.reference(case, 2), " (after the refused calls)")
    assert eng.handoff_timeouts() == (0, 0)
