"""What tests/ops_exact.py rests on, checked without a device: every reference against a second statement, the exactness and input
conditions of the operand sets, the measured yardsticks against the recorded tables (rounded up, not padded, capped), the labels the
host predicates give for every case, the tape's bookkeeping, and the fold predicate of ``_rowscale_producer`` against the
requirement of the kernel entry it leads to."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from ipoke_amd import _lib, nn as K
from ipoke_amd import autograd_ops as FT
from ipoke_amd import first_stage_train as FST
from tests import autograd_exact as A
from tests import conv_exact as CX
from tests import norm_exact as NX
from tests import ops_exact as X
from tests.ops_exact import DTYPES, ELU, F32, F64, NONE, RELU

BOTH = pytest.mark.parametrize("dt", ["f32", "bf16"])


def close(a, b, rel=1e-10):
    scale = float(b.abs().max()) + 1e-300
    assert float((a - b).abs().max()) <= rel * scale, (float((a - b).abs().max()), scale)


# ------------------------------------------------------------------ the case tables
def test_norm_op_table_covers_what_it_must():
    for c in X.NORM_OPS:
        assert c.N <= 6 and c.S in (35, 64, 130) and c.C in (12, 16, 32) and c.G in (c.C, 4, 1), c
        assert c.name not in NX.BWD, "a name of norm_exact's own table would share its operands"
        assert ("bf16" in c.dtypes) == (c.C % 8 == 0), "ipoke_groupnorm takes channels in 16-byte units"
    has = lambda f: any(f(c) for c in X.NORM_OPS)          # noqa: E731
    assert has(lambda c: c.affine) and has(lambda c: not c.affine and c.G == c.C)
    for act in (NONE, RELU, ELU):
        assert has(lambda c: c.act == act)
        assert has(lambda c: c.act == act and c.mod)
    for res in ("pre", "post"):
        assert has(lambda c: c.res == res and c.act == RELU) and has(lambda c: c.res == res and c.act == ELU)
    assert has(lambda c: c.mod == -1) and has(lambda c: 0 < c.mod < c.N and c.N % c.mod == 0 and c.N // c.mod >= 3)
    assert {c.S for c in X.NORM_OPS} == {35, 64, 130} and {c.C for c in X.NORM_OPS} == {12, 16, 32}
    assert {("C" if c.G == c.C else c.G) for c in X.NORM_OPS} == {"C", 4, 1}
    # what the kernel entries refuse cannot be a case: act' from the pre-activation (res_post) never meets modulation
    assert not has(lambda c: c.res == "post" and c.mod)


@pytest.mark.parametrize("name,dt", X.NORM_PAIRS, ids=[f"{n}-{d}" for n, d in X.NORM_PAIRS])
def test_norm_op_labels_and_yardsticks(name, dt):
    """the labels the host predicates of ``group_norm`` give, and the fp32 restatement on the case's own operands within norm_exact's
    recorded yardsticks: the bounds of norm_exact apply unchanged"""
    c = X.NORM_OP[name]
    want = {"norm:plain"}
    if c.res == "post":
        want.add("norm:res_post")
    o = NX.bwd_inputs(X.bwd_case(c), dt)
    if c.mod and o["mg"].shape[0] != c.N:              # the condition of group_norm: mod[0].N != x.N
        assert c.N % o["mg"].shape[0] == 0
        want.add("norm:shared_maps")
    assert tuple(sorted(want)) == X.norm_labels(c)
    f = NX.measure_forward(X.fwd_case(c), dt, o)          # (the op keeps its (mean, rstd) table to itself: y is what the test bounds)
    assert f["y"] <= NX.YARDSTICK[f"y_centred_{dt}"], (name, dt, f["y"])
    b = NX.measure_backward(X.bwd_case(c), dt)
    for k, v in b.items():
        own = X.NORM_OP_YARDSTICK.get((name, dt, k))
        if own is None:
            assert v <= NX.BWD_YARDSTICK[f"{k}_{dt}"], (name, dt, k, v)
        else:                                             # recorded, not padded, and still below the unchanged bound of the device
            assert NX.BWD_YARDSTICK[f"{k}_{dt}"] < v <= own <= v + 0.1 + 1e-9 and own < NX.bwd_bound(k, dt), (name, dt, k, v, own)


@BOTH
@pytest.mark.parametrize("name", ["op-affine-relu-post", "op-instance-elu-post", "op-spade-shared-elu-130", "op-affine-relu-pre"])
def test_norm_reference_against_plain_autograd(name, dt):
    """``norm_exact.bwd_ref`` as ops_exact maps a case onto it (res "post" -> from_pre, shared maps -> summed) against float64 autograd
    through ``F.group_norm`` written out here: modulation by the maps of clip n % k, residual in front of or behind the activation"""
    c = X.NORM_OP[name]
    o = NX.bwd_inputs(X.bwd_case(c), dt)
    x = o["x"].clone().requires_grad_(True)
    gam = o["gamma"].clone().requires_grad_(True) if c.affine else None
    bet = o["beta"].clone().requires_grad_(True) if c.affine else None
    mg = o["mg"].clone().requires_grad_(True) if c.mod else None
    mb = o["mb"].clone().requires_grad_(True) if c.mod else None
    res = o["res"].clone().requires_grad_(True) if c.res else None
    pre = F.group_norm(x.permute(0, 2, 1), c.G, gam, bet, NX.EPS).permute(0, 2, 1)
    if c.mod:
        sel = torch.arange(c.N) % mg.shape[0]
        pre = pre * (1.0 + mg[sel]) + mb[sel]
    if c.res == "pre":
        pre = pre + res
    y = F.elu(pre) if c.act == ELU else torch.relu(pre) if c.act == RELU else pre
    if c.res == "post":
        y = y + res
    o["y"] = y.detach()                                   # (the unrounded output: the derivative of the reference then is autograd's)
    y.backward(o["dy"])
    ref = NX.bwd_ref(X.bwd_case(c), o)
    close(ref["dx"], x.grad)
    if c.affine:
        close(ref["dgamma"], gam.grad); close(ref["dbeta"], bet.grad)
    if c.mod:
        assert ref["dmg"].shape == mg.grad.shape
        close(ref["dmg"], mg.grad); close(ref["dmb"], mb.grad)
    if c.res == "pre":
        close(ref["dres"], res.grad)
    if c.res == "post":
        assert ref["dres"] is None and torch.equal(res.grad, o["dy"])
    close(NX.fwd_ref(X.fwd_case(c), o)["y"], y.detach())


# ------------------------------------------------------------------ the chains
@pytest.mark.parametrize("name,dt", X.CHAIN_PAIRS, ids=[f"{n}-{d}" for n, d in X.CHAIN_PAIRS])
def test_chain_conditions_labels_and_yardsticks(name, dt):
    cc = X.CHAIN[name]
    case = cc.conv
    X.chain_input_conditions(cc, dt)
    N, S, C, G = X.chain_geometry(cc)
    assert 8 <= case.cin <= 32 and 8 <= case.cout <= 32 and (6, 7) <= case.ext[1:] <= (8, 8) and case.frames in (1, 3)
    assert N // case.frames == 2, "two clips per frame"
    assert C % G == 0 and C % DTYPES[dt][2] == 0
    # the label: what the predicate gives for this geometry, and what the kernel entry accepts
    assert X.predicate_accepts_fold(N, S, C, case.frames, False, dt, cc.res_post)
    assert X.kernel_accepts_fold(N, S, C, case.frames, False, dt, cc.res_post)
    m = X.measure_chain(cc, dt)
    for k in X.CHAIN_QTY:
        if k in m:
            rec = X.CHAIN_YARDSTICK[(name, dt, k)]
            assert m[k] <= rec <= min(m[k] + 0.1 + 1e-9, NX.YARDSTICK_CAP), (name, dt, k, m[k], rec)
        else:
            assert (name, dt, k) not in X.CHAIN_YARDSTICK
    for k, key in (("y", f"y_centred_{dt}"), ("mean", f"mean_centred_{dt}"), ("rstd", f"rstd_centred_{dt}")):
        own = X.CHAIN_NORM_YARDSTICK.get((name, dt, k))
        assert m[k] <= (NX.YARDSTICK[key] if own is None else own), (name, dt, k, m[k])
    for k in NX.BWD_QTY:
        if "n" + k in m:
            own = X.CHAIN_NORM_YARDSTICK.get((name, dt, k))
            assert m["n" + k] <= (NX.BWD_YARDSTICK[f"{k}_{dt}"] if own is None else own), (name, dt, k, m["n" + k])
    assert all(v <= NX.YARDSTICK_CAP for v in X.CHAIN_NORM_YARDSTICK.values())


def test_chain_table_covers_the_geometries():
    cs = [c.conv for c in X.CHAINS]
    assert any(c.stride == (1, 1, 1) and c.bias and not c.transposed for c in cs) and any(c.stride == (1, 1, 1) and not c.bias for c in cs)
    assert any(c.stride == (1, 2, 2) and not c.transposed for c in cs) and any(c.transposed and c.stride == (1, 2, 2) for c in cs)
    assert {c.frames for c in cs} == {1, 3}
    assert any(c.res_post for c in X.CHAINS) and {c.kind for c in X.CHAINS} == {"in", "group"}
    assert len({c.conv.name for c in X.CHAINS} | set(A.BY_NAME)) == len(X.CHAINS) + len(A.BY_NAME), "an operand set shared with autograd_exact"


@pytest.mark.parametrize("name", ["s1-bias-in-elu", "ct-bias-in-relu", "s2-bias-in-none", "frames1-group-elu"])
def test_conv_reference_against_the_closed_form(name):
    """``conv_from_gradient`` (autograd through W / sigma_t(W)) against the closed form the kernels implement: g = dY / sigma_t,
    dX = the adjoint convolution of g with W, dW = the weight gradient of (x, g) - sum_t <dY_t, Y_t - b> / sigma_t u_t v_t^T, dbias = sum dY;
    the magnitudes against the same sums over absolute values"""
    cc = X.CHAIN[name]
    case, ops_ = cc.conv, A.operands(cc.conv)
    _, g, o = X.chain_reference_gradient(cc, "f32")
    per = case.N // case.frames
    sc = torch.tensor(o["scales"], dtype=F64).repeat_interleave(per).view(-1, 1, 1)
    dY5 = X.to_maps(g / sc, case.odhw())
    ref = X.conv_from_gradient(case, ops_, dY5)
    g5 = X.to_maps(g, case.odhw())
    w5 = ops_.w5

    def adjoint(gg, ww):
        x0 = torch.zeros_like(ops_.x).requires_grad_(True)
        return torch.autograd.grad(A._conv64(case, x0, ww), x0, gg)[0]

    def wgrad(xx, gg):
        w0 = torch.zeros_like(w5).requires_grad_(True)
        return torch.autograd.grad(A._conv64(case, xx, w0), w0, gg)[0]

    close(ref["dx"], adjoint(g5, w5))
    close(ref["S_dx"], adjoint(g5.abs(), w5.abs()))
    dw, s_dw = wgrad(ops_.x, g5), wgrad(ops_.x.abs(), g5.abs())
    r1, s1 = torch.zeros(case.cout, w5.numel() // case.cout, dtype=F64), torch.zeros(case.cout, w5.numel() // case.cout, dtype=F64)
    b = 0.0 if ops_.b is None else ops_.b.view(1, -1, 1, 1, 1)
    for t, (i, j, s) in enumerate(ops_.pairs):
        sel = slice(t * per, (t + 1) * per)
        pre = A._conv64(case, ops_.x[sel], w5 / s)
        assert torch.equal(pre + b, ops_.y[sel])
        r1[i, j] = (dY5[sel] * pre).sum() / s
        s1[i, j] = (dY5[sel].abs() * (A._conv64(case, ops_.x[sel].abs(), w5.abs() / s) + (0.0 if ops_.b is None else ops_.b.abs().view(1, -1, 1, 1, 1)))).sum() / s
    back = lambda m: m.reshape(case.cout, case.cin, *case.k).transpose(0, 1) if case.transposed else m.reshape(w5.shape)      # noqa: E731
    close(ref["dw"], dw - back(r1))
    close(ref["S_dw"], s_dw + back(s1))
    if case.bias:
        close(ref["db"], dY5.sum((0, 2, 3, 4)))
    # the blocked restatement states the same function: in float64 its three results are the reference's
    rs = X.conv_restated(case, ops_, dY5, "f32")
    for k in X.CHAIN_QTY:
        if ref[k] is not None:
            assert float(X.units32(rs[k], ref[k], ref["S_" + k]).max()) <= NX.YARDSTICK_CAP


# ------------------------------------------------------------------ latent and loss references
@pytest.mark.parametrize("absent", ["none", "dz", "dmu", "dlv"])
def test_reparam_reference_against_autograd(absent):
    mu, lv, eps, dz, dmu, dlv = X.reparam_data(37, 12, False, torch.float32, 6)
    m, l = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    z = m + eps * torch.exp(0.5 * l)
    outs = [(z, dz), (m * 1.0, dmu), (l * 1.0, dlv)]
    keep = [p for n, p in zip(("dz", "dmu", "dlv"), outs) if n != absent]
    torch.autograd.backward([p[0] for p in keep], [p[1] for p in keep])
    gz, gmu, glv = (None if absent == n else v for n, v in (("dz", dz), ("dmu", dmu), ("dlv", dlv)))
    zr, dr, zmag, dmag = X.reparam_ref(mu, lv, eps, gz, gmu, glv)
    close(zr, z.detach())
    close(dr, torch.cat([m.grad, l.grad], 1))
    assert bool((zmag >= zr.abs() * (1 - 1e-12)).all()) and bool((dmag >= dr.abs() * (1 - 1e-12)).all())
    mu, lv, eps, dz, dmu, dlv = X.reparam_data(37, 12, True, torch.bfloat16, 6)
    zr, dr, _, _ = X.reparam_ref(mu, lv, eps, dz, dmu, dlv)
    assert torch.equal(zr, zr.round()) and torch.equal(dr, dr.round()) and float(dr.abs().max()) < 256 and float(zr.abs().max()) < 256


@pytest.mark.parametrize("with_d_frame", [False, True])
def test_l1_reference_against_autograd(with_d_frame):
    B, T, C, H, W = 2, 4, 3, 8, 8
    Xc, pre, d_frame = X.l1_data(B, T, C, H, W, 3)
    scale = 1.0 / (B * (T - 1) * C * H * W)
    # the targets as first_stage_forward_loss builds them, then as channels-last rows
    tgt = Xc[:, 1:].transpose(0, 1).reshape(B * (T - 1), C, H, W)
    rows = tgt.permute(0, 2, 3, 1).reshape(-1, C)
    assert torch.equal(X.l1_targets_rows(Xc), rows)
    assert not torch.equal(rows, Xc[:, 1:].reshape(B * (T - 1), C, H, W).permute(0, 2, 3, 1).reshape(-1, C)), "(clip, frame) order gives the same rows"
    p = pre.clone().requires_grad_(True)
    frame = torch.tanh(p)
    s64 = float(torch.tensor(scale, dtype=F32))
    loss = s64 * (frame - rows).abs().sum()
    total = 10.0 * loss + ((frame * d_frame).sum() if with_d_frame else 0.0)
    total.backward()
    l64, d64, S, dmag = X.l1_ref(frame.detach(), rows, scale, 10.0, d_frame if with_d_frame else None)
    close(l64, loss.detach())
    close(d64, p.grad)
    assert float(S) >= float(l64) and bool((dmag >= d64.abs() * (1 - 1e-12)).all())


# ------------------------------------------------------------------ the tape
def test_tape_restores_what_it_wraps():
    names = ("conv_weight", "group_norm", "add_act", "gru_cell", "gru_unroll", "reparameterize", "kl_loss", "l1_tanh_loss", "_output_gradient")
    before = {(m.__name__, n): getattr(m, n) for m in (FT, FST) for n in names if hasattr(m, n)}
    kgn, nbwd = K.group_norm, FT._NormFn.backward
    with X.Tape():
        assert FT._NormFn.backward is not nbwd
        assert all(getattr(FT, n) is not before[(FT.__name__, n)] for n in names)
        assert FST.group_norm is FT.group_norm and FST.add_act is FT.add_act
        assert "apply" in FT._NormFn.__dict__ and "apply" in FT._AddActFn.__dict__ and K.group_norm is not kgn
    for m in (FT, FST):
        for n in names:
            if hasattr(m, n):
                assert getattr(m, n) is before[(m.__name__, n)]
    assert "apply" not in FT._NormFn.__dict__ and "apply" not in FT._AddActFn.__dict__ and K.group_norm is kgn and FT._NormFn.backward is nbwd


def test_tape_hooks_only_record_and_separate_two_readers():
    """on CPU tensors: a tensor that two taped ops read gets each op's contribution recorded separately, their sum arrives at the
    tensor unchanged, and the address of a passed gradient is kept"""
    tape = X.Tape()
    x = torch.arange(6.0).view(2, 3).requires_grad_(True)
    r1, r2 = tape._begin("a"), tape._begin("b")
    y = tape._tensor_in(r1, "x", x) * 2.0 + tape._tensor_in(r2, "x", x) * 5.0
    tape._end(r2, y)
    g = torch.ones(2, 3)
    y.backward(g)
    assert torch.equal(r1.g_in["x"].t, 2.0 * g) and torch.equal(r2.g_in["x"].t, 5.0 * g) and torch.equal(x.grad, 7.0 * g)
    assert r2.g_out[0].ptr == g.data_ptr() and r1.ins["x"].ptr == x.data_ptr()
    X.assert_sum_of_two(x.grad, r1.g_in["x"].t, r2.g_in["x"].t, torch.float32, "sum of two readers")
    with pytest.raises(AssertionError):
        X.assert_sum_of_two(x.grad, r1.g_in["x"].t, r1.g_in["x"].t, torch.float32, "sum of two readers")


# ------------------------------------------------------------------ the fold predicate against the kernel's requirement
def _bwd_desc(dt, N, S, C, frames, res_post):
    e = DTYPES[dt][2]
    d = _lib.NormBwdDesc()
    d.x, d.ldx, d.y, d.ldy, d.dy, d.lddy, d.dx, d.lddx = NX.A0, C, NX.A0, C, NX.A0, C, NX.A0, C
    d.N, d.S, d.C, d.G, d.eps, d.act, d.workspace = N, S, C, C // e, NX.EPS, RELU, NX.A0
    d.act_from_pre = int(res_post)
    d.rs_scale, d.rs_scale_stride, d.rs_rows_per_group, d.rs_dots, d.rs_workspace = NX.A0, 2, (N // max(frames, 1)) * S, NX.A0, NX.A0
    return d


@BOTH
def test_fold_predicate_never_accepts_what_the_kernel_refuses(dt):
    """over a grid of (N, S, C, frames, modulation, res_post): where ``_rowscale_producer`` accepts, the folded path of
    ipoke_groupnorm_bwd accepts (its requirement restated in ops_exact.kernel_accepts_fold); where the restated requirement refuses
    for the channel count, the library itself refuses the call before anything is launched"""
    code, _, e = DTYPES[dt]
    lib = _lib.lib()
    grid = itertools.product((1, 2, 3, 6), (1, 35, 64), (8, 12, 16, 32, 1024, 1784, 1792, 1800, 1912, 1920, 2040, 2048, 2056, 4096), (1, 2, 3), (False, True),
                             (False, True))
    accepted = declined_but_fine = 0
    for N, S, C, frames, mod, res_post in grid:
        pred = X.predicate_accepts_fold(N, S, C, frames, mod, dt, res_post)
        kern = X.kernel_accepts_fold(N, S, C, frames, mod, dt, res_post)
        assert not pred or kern, f"the predicate accepts N={N} S={S} C={C} frames={frames} mod={mod} res_post={res_post} {dt}, the kernel refuses it"
        accepted += pred
        declined_but_fine += kern and not pred
        lds_refuses = C % e == 0 and 4 * ((8 if res_post else 6) * C + 256 * e + 4) > 64 * 1024
        if lds_refuses and not mod and N % frames == 0 and C <= 4096:
            assert not kern
            rc = lib.ipoke_groupnorm_bwd(ctypes.byref(_bwd_desc(dt, N, S, C, frames, res_post)), code, None)
            assert rc != 0 and b"too many channels" in (lib.ipoke_last_error() or b""), (N, S, C, frames, res_post)
    assert accepted > 100 and declined_but_fine == 0, (accepted, declined_but_fine)
    # the edges by name: the widest norm each form takes
    first = {(False, "f32"): 2560, (False, "bf16"): 2392, (True, "f32"): 1920, (True, "bf16"): 1792}
    for res_post in (False, True):
        C = min(first[(res_post, dt)], 2056) - e
        assert X.kernel_accepts_fold(2, 35, C, 1, False, dt, res_post) == (C <= 2048)
        assert not X.kernel_accepts_fold(2, 35, first[(res_post, dt)], 1, False, dt, res_post)
    # a pitch above C, modulation, an activation or an fp32 output of the convolution: declined
    assert not X.predicate_accepts_fold(2, 35, 16, 1, False, dt, False, ld=16 + e)
    x = K.CL(torch.empty(0, 16), 2, (1, 1, 35), 16)
    for meta in (dict(sn_frames=None, act=NONE), dict(sn_frames=(torch.empty(1, 2),), act=RELU), dict(sn_frames=(torch.empty(1, 2),), act=NONE, out_f32=True)):
        x.conv_meta = meta
        assert FT._rowscale_producer(x, None, "f32") is None
    del x.conv_meta
    assert FT._rowscale_producer(x, None, "f32") is None


# ------------------------------------------------------------------ what _NormFn hands to the kernel entries (no launch)
class _StubLib:
    """the library with ``ipoke_groupnorm`` / ``ipoke_groupnorm_bwd`` replaced by recorders of the descriptor they are handed"""

    def __init__(self, real):
        self._real, self.fwd, self.bwd = real, [], []

    def __getattr__(self, name):
        return getattr(self._real, name)

    @staticmethod
    def _fields(arg):
        d = arg._obj
        return {f[0]: getattr(d, f[0]) for f in d._fields_}

    def ipoke_groupnorm(self, d, dtype, stream):
        self.fwd.append(self._fields(d))
        return 0

    def ipoke_groupnorm_bwd(self, d, dtype, stream):
        self.bwd.append(self._fields(d))
        return 0


@BOTH
@pytest.mark.parametrize("name", ["op-spade-shared", "op-spade-shared-elu-130", "op-spade-per-sample", "op-affine-relu-post", "op-affine-relu-pre"])
def test_norm_descriptors_without_a_launch(name, dt, monkeypatch):
    """``_NormFn`` on CPU tensors with the two kernel entries stubbed: the descriptors carry ``mod_samples`` / ``dmod_summed`` for shared
    maps in BOTH directions, the map gradients' buffers have the maps' row count and pitch, the residual's gradient its own pitch, the
    saved statistics are a copy outside the shared workspace (so dropping any of these is seen without a device)"""
    c = X.NORM_OP[name]
    code, tdt, e = DTYPES[dt]
    stub = _StubLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(X, "DEV", "cpu")
    r = X.NormRun(c, dt, ld=dict(res=c.C + 3 * e))
    r.forward()
    r.y.t.backward(r.dy)
    (f,), (b,) = stub.fwd, stub.bwd
    rows = r.o["mg"].shape[0] if c.mod else 0
    shared = c.mod > 0
    assert f["mod_samples"] == (rows if shared else 0) and b["mod_samples"] == (rows if shared else 0) and b["dmod_summed"] == int(shared)
    assert (f["N"], f["S"], f["C"], f["G"]) == (c.N, c.S, c.C, c.G) == (b["N"], b["S"], b["C"], b["G"])
    assert f["x"] == r.x.data_ptr() == b["x"] and f["ldx"] == r.ld["x"] == b["ldx"] and b["lddy"] == r.ld["x"] and b["lddx"] == r.ld["x"]
    assert r.x.grad.data_ptr() == b["dx"] and r.x.grad.shape == r.x.shape
    if c.mod:
        assert f["mod_gamma"] == r.mg.data_ptr() == b["mod_gamma"] and f["mod_beta"] == r.mb.data_ptr() and f["ld_mod"] == r.ld["mod"] == b["ld_mod"]
        assert b["ld_dmod"] == r.ld["mod"] and tuple(r.mg.grad.shape) == (rows * c.S, r.ld["mod"]) == tuple(r.mb.grad.shape)
        assert b["dmod_gamma"] == r.mg.grad.data_ptr() and b["dmod_beta"] == r.mb.grad.data_ptr()
    else:
        assert not f["mod_gamma"] and not b["mod_gamma"] and not b["dmod_gamma"]
    if c.res:
        assert f["res"] == r.res.data_ptr() and f["ld_res"] == r.ld["res"] and f["res_post"] == int(c.res == "post") == b["act_from_pre"]
        assert tuple(r.res.grad.shape) == tuple(r.res.shape)
        if c.res == "pre":
            assert b["dres"] == r.res.grad.data_ptr() and b["lddres"] == r.ld["res"]
        else:
            assert not b["dres"]
    ws = FT._ws[("norm", r.x.device)]
    assert f["workspace"] == ws.data_ptr() and b["stats"] and not (ws.data_ptr() <= b["stats"] < ws.data_ptr() + 4 * ws.numel())
    assert not b["rs_scale"]
