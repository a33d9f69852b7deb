"""The differentiable ops behind the convolution, the block functions that compose them and the inference twin's statistics hand-over
against float64 at the op level (tests/ops_exact.py): every element of every result compared, every case holding the branch labels it
must take.  Each test prints its worst figures (``OPSFIG ...``) before it asserts."""
import pytest
import torch

from ipoke_amd import _lib, nn as K
from ipoke_amd import autograd_ops as FT
from tests import autograd_exact as A
from tests import conv_exact as CX
from tests import norm_exact as NX
from tests import gru_exact as GX
from tests import ops_exact as X
from tests import sn_exact as SX
from tests.ops_exact import DEV, DTYPES, ELU, F32, F64, NONE, RELU, SENT, assert_same

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("dt", ["f32", "bf16"])


def fig(what, figs):
    print("OPSFIG " + what + " " + " ".join(f"{k} {v:.2f}" for k, v in figs.items()))


# ------------------------------------------------------------------ _NormFn alone
@pytest.mark.parametrize("name,dt", X.NORM_PAIRS, ids=[f"{n}-{d}" for n, d in X.NORM_PAIRS])
def test_group_norm_op(name, dt):
    r = X.run_norm_op(X.NORM_OP[name], dt)
    fig(f"group_norm {name} {dt}", r.figs)


@BOTH
def test_two_interleaved_norm_calls_keep_their_statistics(dt):
    """forward A (small), forward B (a larger N S G: the workspace all norm calls share is overwritten or reallocated), backward A,
    backward B: both still meet the bounds -- the (mean, rstd) table of a call is its own copy"""
    a = X.NormRun(X.NORM_OP["op-affine-relu-pre"], dt)
    b = X.NormRun(X.NORM_OP["op-spade-shared-elu-130"], dt)
    a.forward()
    ws = FT._ws.get(("norm", a.x.device))
    off = _lib.lib().ipoke_groupnorm_stats_offset(a.c.N, a.c.S, a.c.G)
    table = slice(off, off + a.c.N * a.c.G * 2)
    stats_a = ws[table].clone()
    b.forward()
    ws_b = FT._ws.get(("norm", a.x.device))
    assert ws_b is not ws or not torch.equal(ws_b[table], stats_a), "the second call left the first call's table in the shared workspace: the case is empty"
    a.backward()
    b.backward()
    fig(f"interleaved A {dt}", a.check())
    fig(f"interleaved B {dt}", b.check())


def _inputs_of(c):
    return {"x"} | ({"affine"} if c.affine else set()) | ({"mod"} if c.mod else set()) | ({"res"} if c.res else set())


# x only, maps only, affine only, residual only, and two pairs -- wherever the case has the inputs
SUBSETS = [(n, s) for n in ("op-spade-shared-elu-130", "op-spade-per-sample-relu-pre", "op-affine-relu-post")
           for s in (("x",), ("mod",), ("affine",), ("res",), ("x", "res"), ("affine", "mod")) if set(s) <= _inputs_of(X.NORM_OP[n])]


@BOTH
@pytest.mark.parametrize("name,need", SUBSETS, ids=[f"{n}-{'+'.join(s)}" for n, s in SUBSETS])
def test_norm_gradients_only_for_the_inputs_that_ask(name, need, dt):
    X.run_norm_op(X.NORM_OP[name], dt, need=need)


@BOTH
@pytest.mark.parametrize("name", ["op-affine-relu-pre", "op-affine-relu-post", "op-instance-elu-post", "op-spade-shared-elu-130"])
def test_norm_residual_of_another_pitch(name, dt):
    """the residual's gradient goes back at the residual's own pitch (under res_post it is dy, cut or padded), narrower and wider than x's"""
    c = X.NORM_OP[name]
    e = DTYPES[dt][2]
    for ld_res in (c.C, c.C + 3 * e):
        X.run_norm_op(c, dt, ld=dict(res=ld_res))


@BOTH
@pytest.mark.parametrize("act", [NONE, RELU], ids=["identity", "kernel"])
def test_add_act_operands_of_two_pitches(act, dt):
    """``add_act(a, b)`` with b at another pitch than a: both gradients are dy act'(y) at their input's own pitch, bit for bit (integers)"""
    code, tdt, e = DTYPES[dt]
    M, C = 70, 16
    gen = torch.Generator().manual_seed(5)
    a64, b64, dy64 = (X.randint64(-4, 4, (M, C), gen) for _ in range(3))
    for lda, ldb in ((C, C + e), (C + 2 * e, C), (C + e, C + e)):
        a, b = X.cl_dev(a64, C, lda, tdt, SENT, True), X.cl_dev(b64, C, ldb, tdt, SENT, True)
        with X.Tape() as tape:
            y = FT.add_act(K.CL(a, 2, (1, 5, 7), C), K.CL(b, 2, (1, 5, 7), C), dt, act)
            y.t.backward(X.cl_dev(dy64, C, lda, tdt))
            torch.cuda.synchronize()
        assert tape.taken("add_act:") == ("add_act:identity" if act == NONE else "add_act:kernel",)
        s = a64 + b64
        ref_y = torch.relu(s) if act == RELU else s
        ref_g = dy64 * ((s > 0).to(F64) if act == RELU else 1.0)
        what = f"add_act {act} {dt} pitches {lda}/{ldb}"
        assert_same(y.t[:, :C].contiguous(), ref_y, what + " y")
        assert bool((y.t[:, C:] == 0).all())
        for t, ld in ((a, lda), (b, ldb)):
            assert t.grad is not None and t.grad.shape == t.shape, what + ": gradient of another pitch"
            assert_same(t.grad[:, :C].contiguous(), ref_g, what + " gradient")
            assert bool((t.grad[:, C:] == 0).all()), what + ": padding columns of a gradient"


# ------------------------------------------------------------------ convolution -> norm with the row-scale fold
@pytest.mark.parametrize("name,dt", X.CHAIN_PAIRS, ids=[f"{n}-{d}" for n, d in X.CHAIN_PAIRS])
def test_conv_norm_chain_both_routes(name, dt):
    """the folded route (sole_reader) and the convolution's own row-scale pass: each against float64, and against each other -- the
    gradient recorded under the fold is RNE(dx_unfolded / sigma_t) bit for bit, the data gradients are bit-identical"""
    cc = X.CHAIN[name]
    tdt = DTYPES[dt][1]
    fold = X.ChainRun(cc, dt, True)
    figs = fold.check()
    fig(f"chain {name} {dt} fold", figs)
    plain = X.ChainRun(cc, dt, False)
    fig(f"chain {name} {dt} plain", plain.check())
    N, S, C, G = X.chain_geometry(cc)
    sc = torch.tensor(fold.o["scales"], dtype=F64).repeat_interleave(N // cc.conv.frames).view(N, 1, 1)
    expect = X.rne(plain.g.reshape(N, S, C).to(F64) * sc, tdt)
    assert_same(fold.g.reshape(N, S, C).contiguous(), expect, f"chain {name} {dt}: folded gradient against RNE(dx / sigma_t) of the other route")
    assert_same(fold.x_t.grad.cpu(), plain.x_t.grad.cpu(), f"chain {name} {dt}: dX of the two routes")


@BOTH
@pytest.mark.parametrize("name", list(X.BLOCK_CHAINS))
def test_block_functions_state_the_folded_chain(name, dt):
    """``conv_block`` / ``convT_block`` of first_stage_train on a first_stage block holding the chain's operands: the same checks, so the
    block passes ``sole_reader`` (labels norm:fold, conv:prescaled), the block's activation and its norm's parameters"""
    run = X.ChainRun(X.CHAIN[name], dt, True, block=X.BLOCK_CHAINS[name])
    fig(f"{X.BLOCK_CHAINS[name]} {name} {dt}", run.check())


@BOTH
@pytest.mark.parametrize("frames", [1, 3])
def test_res_block_sum_on_the_skip_norm(frames, dt):
    """the res_post route of ``res_block``: wiring bit for bit, the labels, dres = the incoming gradient, and at x -- read by conv1 and by
    res_conv -- the sum of the two recorded contributions rounded once"""
    tdt = DTYPES[dt][1]
    tape, x, blk, dy, out = X.run_res_block_post(dt, frames)
    convs, norms = tape.of("conv"), tape.of("norm")
    assert len(convs) == 3 and len(norms) == 1 and not tape.of("add_act")
    c1, c2, rc = convs
    nm = norms[0]
    assert (c1.w is blk.conv1.conv.weight_orig and c2.w is blk.conv2.conv.weight_orig and rc.w is blk.res_conv.conv.weight_orig)
    assert c1.opts["act"] == RELU and c2.opts["act"] == NONE and rc.opts["act"] == NONE and nm.opts["act"] == RELU
    assert tape.taken() == ("conv:prescaled", "conv:rowscale", "norm:fold", "norm:res_post"), tape.taken()
    X.assert_fed_by(c2, "x", c1, "res_block: conv2 reads conv1")
    X.assert_fed_by(nm, "x", rc, "res_block: the skip norm reads res_conv")
    X.assert_fed_by(nm, "res", c2, "res_block: the residual is conv2's output")
    assert c1.ins["x"].ptr == x.data_ptr() == rc.ins["x"].ptr
    assert out.t.data_ptr() == nm.out.ptr
    assert_same(nm.g_in["res"].t, dy.cpu(), "res_block: dres is the incoming gradient")
    assert_same(c2.g_out[0].t, dy.cpu(), "res_block: conv2 receives it unchanged")
    assert nm.g_in["x"].ptr == rc.g_out[0].ptr, "the pre-scaled gradient reaches res_conv as the tensor the norm made"
    X.assert_sum_of_two(x.grad.cpu(), c1.g_in["x"].t, rc.g_in["x"].t, tdt, "res_block: gradient at x")
    # the norm against float64 of its own recorded inputs
    N, S, C = nm.opts["N"], nm.opts["S"], nm.opts["C"]
    c = NX._c("res-block-norm", N, S, C, C, False, RELU, "post", 0)
    o = dict(x=nm.ins["x"].t.reshape(N, S, C).to(F64), res=nm.ins["res"].t.reshape(N, S, C).to(F64), gamma=None, beta=None, mg=None, mb=None)
    ref = NX.fwd_ref(c, o)
    NX.assert_units(f"res_block norm y {dt}", nm.out.t.reshape(N, S, C), ref["y"], ref["mag"], NX.gpu_bound("y", "centred", dt), tdt)


# ------------------------------------------------------------------ the inference twin
@BOTH
@pytest.mark.parametrize("name", [h.name for h in X.HANDOVERS])
def test_chunk_statistics_hand_over(name, dt):
    """``K.group_norm(next_groups=...)`` -> the SPADE norm: the consumer's y against float64 of the producer's STORED output (norm_exact's
    consumer rule), whether the hand-over is taken, ignored (another group count) or not offered (C no multiple of next_groups)"""
    h = {x.name: x for x in X.HANDOVERS}[name]
    labels, offered, c, o, y = X.run_handover(h, dt)
    assert offered == (h.C % h.next_groups == 0) and (("norm:part",) if h.part else ()) == labels, (offered, labels)
    ref = NX.fwd_ref(c, o)
    u = NX.assert_units(f"hand-over {name} {dt} y", y, ref["y"], ref["mag"], NX.gpu_bound("y", "centred", dt), DTYPES[dt][1])
    fig(f"hand-over {name} {dt}", dict(y=u))


@BOTH
def test_fold_without_a_gradient_for_the_convolution(dt):
    """the convolution behind a sole-reader norm asks for no gradient at all: its backward never runs, so the norm must not fold (a
    pre-scaled gradient would stay on the convolution's meta); the norm's own gradients are right, twice through a retained graph"""
    cc = X.CHAIN["frames1-group-elu"]
    run = X.ChainRun(cc, dt, True, need=(False, False, False))
    assert "_prescaled" not in run.conv.meta, "a pre-scaled gradient was left behind for a backward that never runs"
    assert run.norm.opts["sole_reader"] and run.tape.taken() == ("norm:plain",), run.tape.taken()          # (offered in forward, not made in backward)
    N, S, C, G = X.chain_geometry(cc)
    o = dict(run.o)
    o["y"] = run.norm.out.t.reshape(N, S, C).to(F64)
    bc = X.chain_bwd_case(cc)
    ref = NX.bwd_ref(bc, o)
    _, mag = NX.bwd_restated(bc, o, F64)
    first = {}
    for k, p in (("dgamma", run.nmod.weight), ("dbeta", run.nmod.bias)):
        NX.assert_units(f"no-grad chain {dt} {k}", p.grad.cpu(), ref[k], mag[k], NX.bwd_bound(k, dt))
        first[k] = p.grad.clone()
        p.grad = None
    run.z.t.backward(run.dz)
    torch.cuda.synchronize()
    assert "_prescaled" not in run.conv.meta
    for k, p in (("dgamma", run.nmod.weight), ("dbeta", run.nmod.bias)):
        assert_same(p.grad, first[k], f"no-grad chain {dt}: {k} of the second backward")


@BOTH
def test_fold_twice_through_a_retained_graph(dt):
    """two backward passes through one folded chain: the hand-over is made and consumed each time, the same bits both times"""
    cc = X.CHAIN["s1-bias-in-elu"]
    run = X.ChainRun(cc, dt, True)
    first = (run.x_t.grad.clone(), A.weight_of(run.mod).grad.clone(), run.mod.bias.grad.clone())
    run.x_t.grad = None
    A.weight_of(run.mod).grad = None
    run.mod.bias.grad = None
    assert "_prescaled" not in run.conv.meta
    run.z.t.backward(run.dz)
    torch.cuda.synchronize()
    assert "_prescaled" not in run.conv.meta
    for a, b, k in zip((run.x_t.grad, A.weight_of(run.mod).grad, run.mod.bias.grad), first, ("dX", "dW", "dbias")):
        assert_same(a, b, f"retained chain {dt}: {k} of the second backward")


def test_a_changed_prescaled_gradient_is_refused():
    """``_output_gradient`` raises (before any launch) when the gradient that arrives is not the tensor the norm handed over"""
    m = dict(dtype="f32", cout=8, act=NONE, _prescaled=(torch.zeros(4, 8, device=DEV), None, None))
    with pytest.raises(RuntimeError, match="did not arrive unchanged"):
        FT._output_gradient(m, torch.zeros(4, 8, device=DEV), None, None, False)


# ------------------------------------------------------------------ ConvGRU
GRU_PAIRS = [(g, dt) for g in X.GRU_GEOMS for dt in ("f32", "bf16")]


@pytest.mark.parametrize("geom,dt", GRU_PAIRS, ids=[f"B{g[0]}T{g[1]}L{g[2]}C{g[3]}-{dt}" for g, dt in GRU_PAIRS])
def test_gru_op_and_cell_loop_are_exact(geom, dt):
    """every weight zero, integer buffers: outputs, d x0, d h0 and every weight / bias gradient bit for bit -- on ``update_gate``,
    ``reset_gate`` and ``out_gate`` of the right cell -- from the native op and from the cell-by-cell loop alike"""
    c = X.gru_case(*geom, dt)
    tdt = DTYPES[dt][1]
    ops_ = GX.operands(c, exact=True)
    ref = GX.unroll(c, ops_)
    assert any(bool((w != 0).any()) for w in ref["dw"][4 * (c.L - 1):]), "the last cell's gradients are all zero: the case is empty"
    rnn = X.gru_module(c, ops_)
    outs = {}
    for native in (True, False):
        out, x0, h0, tape = X.gru_run(c, ops_, rnn, native)
        what = f"gru {'native' if native else 'cells'} {c.id}"
        assert tape.taken("gru:") == (("gru:native",) if native else ("gru:cells",)), tape.taken()
        assert_same(GX.canon(out[:, :c.Ch].contiguous().cpu()), GX.canon(torch.cat(ref["out"], 0).to(tdt)), what + " out")
        assert_same(GX.canon(x0.grad[:, :c.Cx].contiguous().cpu()), GX.canon(ref["dx0"].to(tdt)), what + " d x0")
        assert_same(GX.canon(h0.grad[:, :c.Ch].contiguous().cpu()), GX.canon(ref["dh0"].to(tdt)), what + " d h0")
        for i, (g, r) in enumerate(zip(X.gru_grads(rnn), ref["dw"])):
            assert_same(GX.canon(g), GX.canon(r.to(F32)), f"{what}: gradient of weight tensor {i % 4} of cell {i // 4}")
        outs[native] = out
    assert_same(outs[True], outs[False], f"gru {c.id}: native against the cell loop")


@BOTH
@pytest.mark.parametrize("mode,ld_extra", [("cl", 0), ("f32", 0), ("slice", 0), ("cl", 1)], ids=["dtype", "fp32-dout", "sliced-dout", "wide-inputs"])
def test_gru_op_is_the_direct_call(mode, ld_extra, dt):
    """real operands: the op gives the bits of ``ipoke_gru_unroll_forward`` / ``_backward`` called directly on the same buffers (which
    tests/gru_exact.py holds to float64); d_out in fp32, as a column slice, inputs of a wider pitch"""
    c = X.gru_case(2, 3, 2, 32, dt)
    code, tdt, e = DTYPES[dt]
    ops_ = GX.operands(c, exact=False)
    rnn = X.gru_module(c, ops_)
    out, x0, h0, tape = X.gru_run(c, ops_, rnn, True, ld_extra=ld_extra * e, dout_mode=mode)
    dout = X.cl_dev(ops_["dout"].reshape(c.T * c.M, c.Ch), c.Ch, out.shape[1], tdt)
    d_out, d_x0, d_h0, d_ws = X.gru_direct(c, ops_, rnn, x0.detach(), h0.detach(), dout)
    what = f"gru op against the direct call {mode} {dt}"
    assert_same(out, d_out, what + " out")
    assert x0.grad.shape == x0.shape and h0.grad.shape == h0.shape
    assert_same(x0.grad[:, :c.Cx].contiguous(), X.rne(d_x0.to(F64), tdt), what + " d x0")
    assert_same(h0.grad[:, :c.Ch].contiguous(), X.rne(d_h0.to(F64), tdt), what + " d h0")
    assert bool((x0.grad[:, c.Cx:] == 0).all()) and bool((h0.grad[:, c.Ch:] == 0).all())
    for i, (g, r) in enumerate(zip(X.gru_grads(rnn), d_ws)):
        assert_same(g, r, f"{what}: gradient of weight tensor {i % 4} of cell {i // 4}")


# ------------------------------------------------------------------ latent and loss ops
@BOTH
@pytest.mark.parametrize("exact", [True, False], ids=["integers", "real-logvar"])
@pytest.mark.parametrize("absent", ["none", "dz", "dmu", "dlv"])
def test_reparameterize_op(absent, exact, dt):
    code, tdt, e = DTYPES[dt]
    M, Z = 37, 12
    ld = 2 * Z + e                                         # a pitch above 2 Z
    mu, lv, eps, dz, dmu, dlv = X.reparam_data(M, Z, exact, tdt, 6)
    mulv = X.cl_dev(torch.cat([mu, lv], 1), 2 * Z, ld, tdt, SENT, True)
    with X.Tape() as tape:
        z, m_, l_ = FT.reparameterize(mulv, eps.to(F32).to(DEV), Z, dt)
        outs, grads = [], []
        for name, t, g in (("dz", z, dz), ("dmu", m_, dmu), ("dlv", l_, dlv)):
            if name != absent:
                outs.append(t); grads.append(g.to(F32).to(DEV))
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
    what = f"reparameterize op {absent} absent {'exact' if exact else 'real'} {dt}"
    gz, gmu, glv = (None if absent == n else v for n, v in (("dz", dz), ("dmu", dmu), ("dlv", dlv)))
    zr, dr, zmag, dmag = X.reparam_ref(mu, lv, eps, gz, gmu, glv)
    assert_same(m_.cpu(), mu.to(F32), what + " mu")
    assert_same(l_.cpu(), lv.to(F32), what + " logvar")
    got = mulv.grad.cpu()
    assert got.shape == mulv.shape and bool((got[:, 2 * Z:] == 0).all()), what + ": pitch / padding of the gradient"
    if exact:
        assert_same(z.detach().cpu(), zr.to(F32), what + " z")
        assert_same(got[:, :2 * Z].contiguous(), dr, what + " d mulv")
        return
    z32, d32, _, _ = X.reparam_ref(mu, lv, eps, gz, gmu, glv, F32)
    yz, yd = float(NX.units(z32, zr, zmag).max()), float(NX.units(d32, dr, dmag).max())
    assert max(yz, yd) <= NX.YARDSTICK_CAP
    fig(what, dict(yard_z=yz, yard_d=yd, z=float(NX.units(z.detach().cpu(), zr, zmag).max()), d=float(NX.units(got[:, :2 * Z], dr, dmag, tdt).max())))
    NX.assert_units(what + " z", z.detach().cpu(), zr, zmag, max(4.0 * yz, 4.0))
    NX.assert_units(what + " d mulv", got[:, :2 * Z], dr, dmag, max(4.0 * yd, 4.0), tdt)


@pytest.mark.parametrize("case", SX.KL_CASES[:2], ids=lambda c: c.name)
def test_kl_op_under_an_upstream_factor(case):
    """value and both gradients of ``kl_loss`` with 3 x the loss differentiated: the bounds of sn_exact's test_kl_loss"""
    factor = 3.0
    mu, lv = SX.kl_operands(case)
    mu_d = mu.view(case.positions, case.Z).to(F32).to(DEV).requires_grad_(True)
    lv_d = lv.view(case.positions, case.Z).to(F32).to(DEV).requires_grad_(True)
    with X.Tape() as tape:
        kl = FT.kl_loss(mu_d, lv_d)
        (kl * factor).backward()
        torch.cuda.synchronize()
    ref = SX.kl_ref(mu, lv, case.positions, torch.tensor(0.0, dtype=F64))
    what = f"kl op {case.name}"
    figs = dict(value=NX.assert_units(what + " value", kl.detach().cpu().reshape(1), ref["loss"].reshape(1), ref["loss_mag"].reshape(1), SX.gpu_bound("kl_value")),
                dmu=NX.assert_units(what + " dmu", mu_d.grad.cpu().reshape(-1), factor * ref["dmu"], factor * ref["dmu"], SX.gpu_bound("kl_dmu")),
                dlv=NX.assert_units(what + " dlv", lv_d.grad.cpu().reshape(-1), factor * ref["dlv"], factor * ref["dlv_mag"], SX.gpu_bound("kl_dlv")))
    fig(what, figs)
    r = tape.of("kl")[0]
    assert set(r.g_in) == {"mu", "lv"} and float(r.g_out[0].t) == factor


@pytest.mark.parametrize("with_d_frame", [False, True], ids=["loss-only", "with-d_frame"])
def test_l1_tanh_op(with_d_frame):
    """targets in (frame, clip) order from a transposed, reshaped clip as first_stage_forward_loss builds them; an upstream factor of
    10; a d_frame arriving as well.  frame against float64 tanh (conv_exact.real_bound("act_tanh")); the loss and d pre against float64
    of the STORED frame, bound max(4 x yardstick, 4) with the fp32 restatement on the CPU as the yardstick"""
    B, T, C, H, W = 2, 4, 3, 8, 8
    w_l1 = 10.0
    Xc, pre, d_frame = X.l1_data(B, T, C, H, W, 3)
    scale = 1.0 / (B * (T - 1) * C * H * W)
    Xd = Xc.to(F32).to(DEV)
    tgt = Xd[:, 1:].transpose(0, 1).reshape(B * (T - 1), C, H, W)
    pre_d = pre.to(F32).to(DEV).requires_grad_(True)
    with X.Tape() as tape:
        loss, frame = FT.l1_tanh_loss(pre_d, tgt, scale)
        total = w_l1 * loss
        if with_d_frame:
            total = total + (frame * d_frame.to(F32).to(DEV)).sum()
        total.backward()
        torch.cuda.synchronize()
    what = f"l1_tanh op d_frame={with_d_frame}"
    fr = frame.detach().cpu()
    th = torch.tanh(pre)
    tanh_units = NX.assert_units(what + " frame", fr, th, th, CX.real_bound("act_tanh"))
    rows = X.l1_targets_rows(Xc)
    dfr = d_frame if with_d_frame else None
    l64, d64, S, dmag = X.l1_ref(fr, rows, scale, w_l1, dfr)
    l32, d32, _, _ = X.l1_ref(fr, rows, scale, w_l1, dfr, F32)
    y_loss = float(NX.units(l32.reshape(1), l64.reshape(1), S.reshape(1)).max())
    y_d = float(NX.units(d32, d64, dmag).max())
    assert max(y_loss, y_d) <= NX.YARDSTICK_CAP
    figs = dict(tanh=tanh_units, yard_loss=y_loss, yard_d=y_d,
                loss=NX.assert_units(what + " loss", loss.detach().cpu().reshape(1), l64.reshape(1), S.reshape(1), max(4.0 * y_loss, 4.0)),
                d=NX.assert_units(what + " d pre", pre_d.grad.cpu(), d64, dmag, max(4.0 * y_d, 4.0)))
    fig(what, figs)
    r = tape.of("l1_tanh")[0]
    assert float(r.g_out[0].t) == w_l1 and ((1 in r.g_out) == with_d_frame)


# ------------------------------------------------------------------ the block layer under the tape
@BOTH
@pytest.mark.parametrize("mode", ["act", "res", "f32"])
def test_conv_block_without_a_norm(mode, dt):
    """the activation inside the convolution (conv:act_bwd), a residual through ``add_act`` (add_act:kernel), an fp32 output whose tanh is
    left to the loss: y, dX, dW, dbias (and the residual's gradient) bit for bit"""
    tape = X.conv_block_plain(mode, dt)
    want = {"act": ("conv:act_bwd",), "res": ("add_act:kernel",), "f32": ()}[mode]
    assert tape.taken() == want, tape.taken()
    convs = tape.of("conv")
    assert len(convs) == 1 and convs[0].opts["act"] == (RELU if mode == "act" else NONE) and convs[0].opts["out_f32"] == (mode == "f32")
    if mode == "res":
        (aa,) = tape.of("add_act")
        X.assert_fed_by(aa, "a", convs[0], "conv_block: add_act reads the convolution")
        X.check_add_act_record(aa, dt, f"conv_block res {dt} add_act")
        assert_same(convs[0].g_out[0].t, aa.g_in["a"].t, "conv_block: the convolution receives add_act's gradient")


@BOTH
@pytest.mark.parametrize("frames", [1, 3])
def test_res_block_identity_skip(frames, dt):
    """x feeds conv1 and is the residual of conv2's norm: wiring, both norms against float64 of their recorded operands, and at x the sum
    of conv1's data gradient and the norm's dres rounded once"""
    tape, x, blk, out = X.run_res_block("identity", dt, frames)
    (c1, c2), (n1, n2) = tape.of("conv"), tape.of("norm")
    assert tape.taken() == ("conv:prescaled", "norm:fold"), tape.taken()
    assert c1.w is blk.conv1.conv.weight_orig and c2.w is blk.conv2.conv.weight_orig
    X.assert_fed_by(n1, "x", c1, "identity skip: norm1 reads conv1")
    X.assert_fed_by(c2, "x", n1, "identity skip: conv2 reads norm1")
    X.assert_fed_by(n2, "x", c2, "identity skip: norm2 reads conv2")
    assert n1.opts["act"] == ELU and n2.opts["act"] == NONE and not n2.opts["res_post"] and "res" not in n1.ins
    assert out.t.data_ptr() == n2.out.ptr and c1.ins["x"].ptr == x.data_ptr()
    X.assert_two_readers(x.grad.cpu(), c1, "x", n2, "res", dt, "identity skip: gradient at x")
    for i, n in enumerate((n1, n2)):
        figs, _ = X.check_norm_record(n, dt, f"identity skip norm{i + 1} {dt}", folded=True)
        fig(f"res_block identity norm{i + 1} {dt} frames {frames}", figs)


@BOTH
@pytest.mark.parametrize("frames", [1, 3])
def test_res_block_convolved_skip_without_a_norm(frames, dt):
    """no norm anywhere: out = add_act(conv2(conv1(x)), res_conv(x)) without activation (add_act:identity); x is read by conv1 and res_conv"""
    tape, x, blk, out = X.run_res_block("no-norm", dt, frames)
    rc, c1, c2 = tape.of("conv")
    (aa,) = tape.of("add_act")
    assert not tape.of("norm") and tape.taken() == ("add_act:identity", "conv:rowscale"), tape.taken()
    assert rc.w is blk.res_conv.conv.weight_orig and c1.w is blk.conv1.conv.weight_orig and c2.w is blk.conv2.conv.weight_orig
    assert rc.opts["act"] == RELU and c1.opts["act"] == RELU and c2.opts["act"] == NONE
    X.assert_fed_by(c2, "x", c1, "no-norm skip: conv2 reads conv1")
    X.assert_fed_by(aa, "a", c2, "no-norm skip: the sum's first operand")
    X.assert_fed_by(aa, "b", rc, "no-norm skip: the sum's second operand")
    X.check_add_act_record(aa, dt, f"no-norm skip add_act {dt}")
    assert out.t.data_ptr() == aa.out.ptr
    X.assert_two_readers(x.grad.cpu(), c1, "x", rc, "x", dt, "no-norm skip: gradient at x")


@BOTH
def test_basic_block_3d_with_downsample(dt):
    """BasicBlock(16 -> 32, stride (1, 2, 2)) on extents (3, 6, 8): wiring, the three norms against float64 of their recorded operands
    and recorded gradients, the two-reader sum at x (conv1 and the downsample's convolution)"""
    tape, x, blk, out = X.run_basic_block(dt)
    (c1, cd, c2), (n1, nd, n2) = tape.of("conv"), tape.of("norm")
    assert tape.taken() == ("norm:plain",), tape.taken()
    assert c1.w is blk.conv1.weight and cd.w is blk.downsample[0].weight and c2.w is blk.conv2.weight
    assert c1.opts["stride"] == (1, 2, 2) and cd.opts["stride"] == (1, 2, 2) and cd.opts["k"] == (1, 1, 1) and c2.opts["stride"] == (1, 1, 1)
    assert tuple(out.dhw) == (3, 3, 4)
    for a, name, b in ((n1, "x", c1), (nd, "x", cd), (c2, "x", n1), (n2, "x", c2), (n2, "res", nd)):
        X.assert_fed_by(a, name, b, "basic_block")
    assert n1.opts["act"] == RELU and nd.opts["act"] == NONE and n2.opts["act"] == RELU and not n2.opts["res_post"]
    assert n1.gamma is blk.bn1.weight and nd.gamma is blk.downsample[1].weight and n2.gamma is blk.bn2.weight
    X.assert_two_readers(x.grad.cpu(), c1, "x", cd, "x", dt, "basic_block: gradient at x")
    for n, nm in ((n1, "bn1"), (nd, "downsample"), (n2, "bn2")):
        figs, _ = X.check_norm_record(n, dt, f"basic_block {nm} {dt}")
        fig(f"basic_block {nm} {dt}", figs)


@BOTH
def test_spade_modulation_shared_against_repeated_maps(dt):
    """``spade_modulation`` -> ``group_norm(mod=...)``: per-sample maps, maps shared by three frames (norm:shared_maps), and the same
    with the maps repeated per sample by hand: the summed map gradients equal the sum of the per-frame gradients within
    bwd_bound per term; the three SPADE convolutions are differentiated once in every run"""
    tdt = DTYPES[dt][1]
    S, C = 64, 32
    one = X.run_spade(dt, 1, True)
    assert one[0].taken("norm:") == ("norm:plain",) and len(one[0].conv_backwards) == 3
    tape_s, nm_s, sp = X.run_spade(dt, 3, True)
    tape_r, nm_r, _ = X.run_spade(dt, 3, False)
    assert tape_s.taken() == ("conv:act_bwd", "norm:plain", "norm:shared_maps") and tape_r.taken() == ("conv:act_bwd", "norm:plain")
    for tape in (tape_s, tape_r):
        convs = tape.of("conv")
        assert len(convs) == 3 and len(tape.conv_backwards) == 3, "the three SPADE convolutions are differentiated once"
        assert tape is tape_r or all(c.w is w for c, w in zip(convs, (sp.conv.weight, sp.conv_gamma.weight, sp.conv_beta.weight)))
        X.assert_fed_by(convs[1], "x", convs[0], "spade: conv_gamma reads conv")
        X.assert_fed_by(convs[2], "x", convs[0], "spade: conv_beta reads conv")
    X.assert_fed_by(nm_s, "mg", tape_s.of("conv")[1], "spade: the norm's gamma map")
    X.assert_fed_by(nm_s, "mb", tape_s.of("conv")[2], "spade: the norm's beta map")
    assert nm_s.g_in["mg"].t.shape[0] == 2 * S and nm_r.g_in["mg"].t.shape[0] == 6 * S
    assert_same(tape_s.of("conv")[1].g_out[0].t, nm_s.g_in["mg"].t, "spade: conv_gamma receives the summed gradient")
    f_s, _ = X.check_norm_record(nm_s, dt, f"spade shared {dt}")
    f_r, mag_r = X.check_norm_record(nm_r, dt, f"spade repeated {dt}")
    fig(f"spade shared {dt}", f_s); fig(f"spade repeated {dt}", f_r)
    for k, name in (("dmg", "mg"), ("dmb", "mb")):
        per = nm_r.g_in[name].t[:, :C].to(F64).view(3, 2 * S, C)
        tol = (NX.bwd_bound(k, dt) * NX.ulp_f32(mag_r[k].reshape(3, 2 * S, C)) + (NX.ulp_bf16(per) if tdt == torch.bfloat16 else 0.0)).sum(0)
        tot = per.sum(0)
        if tdt == torch.bfloat16:
            tol = tol + NX.ulp_bf16(tot)
        err = (nm_s.g_in[name].t[:, :C].to(F64) - tot).abs()
        assert bool((err <= tol).all()), (k, float((err / tol).max()))


@BOTH
@pytest.mark.parametrize("frames", [1, 3])
def test_decode_frame_wiring(frames, dt):
    """one decoder stage (16, 8), z of 8 channels, 8 x 8 -> 16 x 16: which op reads which output, the two-reader sums at h and at the
    in_block's output, every norm against float64 of its recorded operands; no end-to-end tolerance"""
    tape, h, gen_, pre = X.run_decode_frame(dt, frames)
    convs, norms = tape.of("conv"), tape.of("norm")
    sp_c, sp_g, sp_b, i_rc, i_c1, i_c2, b_c1, b_c2, b_rc, oc = convs
    i_nrc, i_n1, i_n2, b_n, s_n = norms
    ib, bb, sp = gen_.in_block, gen_.blocks[0], gen_.spade_blocks[0]
    owners = (sp.conv.weight, sp.conv_gamma.weight, sp.conv_beta.weight, ib.res_conv.conv.weight_orig, ib.conv1.conv.weight_orig,
              ib.conv2.conv.weight_orig, bb.conv1.conv.weight_orig, bb.conv2.conv.weight_orig, bb.res_conv.conv.weight_orig, gen_.out_conv.conv.weight)
    assert all(c.w is w for c, w in zip(convs, owners))
    want = {"conv:act_bwd", "conv:prescaled", "conv:rowscale", "norm:fold", "norm:plain", "norm:res_post"} | ({"norm:shared_maps"} if frames > 1 else set())
    assert set(tape.taken()) == want, tape.taken()
    for a, name, b in ((i_nrc, "x", i_rc), (i_n1, "x", i_c1), (i_c2, "x", i_n1), (i_n2, "x", i_c2), (i_n2, "res", i_nrc), (b_c1, "x", i_n2), (b_rc, "x", i_n2),
                       (b_c2, "x", b_c1), (b_n, "x", b_rc), (b_n, "res", b_c2), (s_n, "x", b_n), (s_n, "mg", sp_g), (s_n, "mb", sp_b), (oc, "x", s_n),
                       (sp_g, "x", sp_c), (sp_b, "x", sp_c)):
        X.assert_fed_by(a, name, b, "decode_frame")
    assert b_c1.opts["transposed"] and b_rc.opts["transposed"] and not b_c2.opts["transposed"] and oc.opts["out_f32"] and oc.opts["act"] == NONE
    assert b_n.opts["res_post"] and not i_n2.opts["res_post"] and s_n.opts["mod_N"] == 2 and s_n.opts["groups"] == sp.groups
    assert pre.t.data_ptr() == oc.out.ptr and pre.t.dtype == F32 and len(tape.conv_backwards) == 10
    X.assert_two_readers(h.grad.cpu(), i_rc, "x", i_c1, "x", dt, "decode_frame: gradient at h")
    X.assert_sum_of_two(i_n2.g_out[0].t, b_c1.g_in["x"].t, b_rc.g_in["x"].t, DTYPES[dt][1], "decode_frame: gradient at the in_block's output")
    for n, nm, folded in ((i_nrc, "in.res", True), (i_n1, "in.1", True), (i_n2, "in.2", True), (b_n, "stage.skip", True), (s_n, "spade", False)):
        figs, _ = X.check_norm_record(n, dt, f"decode_frame {nm} {dt}", folded=folded)
        fig(f"decode_frame {nm} {dt} frames {frames}", figs)


@BOTH
def test_a_modulated_norm_behind_a_frame_batched_convolution_does_not_fold(dt):
    """a chain the predicate declines and the kernel can reach: SPADE maps on the sole-reader norm -> norm:plain, conv:rowscale"""
    cc = X.CHAIN["s1-bias-in-elu"]
    case, ops_ = cc.conv, A.operands(cc.conv)
    tdt = DTYPES[dt][1]
    N, S, C, G = X.chain_geometry(cc)
    mod = A.build_module(case, ops_)
    x_t = X.cl_of(ops_.x, dt).to(DEV).requires_grad_(True)
    _, mg = X.real_cl(N * S, C, 41, tdt, scale=0.5)
    _, mb = X.real_cl(N * S, C, 42, tdt, scale=0.5)
    _, dy = X.int_cl(N * S, C, 4, 43, tdt, grad=False)
    with X.Tape() as tape:
        y = FT.conv(mod, K.CL(x_t, case.N, case.ext, case.cin), dt, w=X.weight_handle(case, mod, ops_))
        z = FT.group_norm(y, G, dt, mod=(K.CL(mg, N, y.dhw, C), K.CL(mb, N, y.dhw, C)), sole_reader=True)
        z.t.backward(dy)
        torch.cuda.synchronize()
    assert tape.taken() == ("conv:rowscale", "norm:plain"), tape.taken()
    X.assert_cl_equal(tape.of("conv")[0].out.t, ops_.y, "declined chain: convolution output")
    nm = tape.of("norm")[0]
    X.assert_fed_by(nm, "x", tape.of("conv")[0], "declined chain")
    figs, _ = X.check_norm_record(nm, dt, f"declined chain norm {dt}")
    assert_same(tape.of("conv")[0].g_out[0].t, nm.g_in["x"].t, "declined chain: the convolution receives the norm's dx")
    fig(f"declined chain {dt}", figs)


@BOTH
@pytest.mark.parametrize("name", [h[0] for h in X.RUN_HANDOVERS])
def test_chunk_statistics_through_the_run_methods(name, dt):
    """``ResBlock.run(next_groups=...)`` -> ``Spade.run``: whether the block offers the statistics, whether the SPADE norm receives the CL
    that carries them and takes them (norm:part) or must ignore them; the consumer's y against float64 of the producer's stored output"""
    _, C, ng, part = next(h for h in X.RUN_HANDOVERS if h[0] == name)
    tape, prod, cons, offered, sp = X.run_handover_modules(name, dt)
    want_ng = sp.groups if ng is None else ng
    assert prod.opts["next_groups"] == want_ng and prod.opts["res_post"] and prod.opts["groups"] == C
    assert offered == prod.opts["offered"] == (C % want_ng == 0)
    assert cons.opts["groups"] == sp.groups and cons.opts["handed"] == (want_ng if offered else None) and cons.opts["part"] == part
    assert tape.taken("norm:") == (("norm:part",) if part else ())
    X.assert_fed_by(cons, "x", prod, f"hand-over through run {name}")
    figs, _ = X.check_norm_record(cons, dt, f"hand-over through run {name} {dt}")
    fig(f"hand-over through run {name} {dt}", figs)
