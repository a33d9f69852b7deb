"""The references of tests/sn_exact.py pinned without a GPU: the decomposition the first stage's parameter kernels implement against
autograd through torch.nn.utils.spectral_norm in float64, the KL and Adam references against autograd / torch.optim.Adam, the eps cases
against F.normalize; the conditions the generated operands must meet for a green GPU test to mean something (the loop each named case
claims to enter, ELU outputs at and next to -1, exact integer sums, sigma away from zero); and the recorded fp32 yardsticks."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from tests import sn_exact as X
from tests.sn_exact import BF16, DTYPES, F32, F64, YARDSTICK, as_seen, cast_like, err_units, f32r, restate


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------ the decomposition is the reference's mathematics
def rows_of(t):
    """[N][C][H][W] -> channels-last rows [N*H*W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def nchw_of(r, like):
    N, C, H, W = like.shape
    return r.reshape(N, H, W, C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("kind", ["conv", "conv_transpose"])
def test_composed_references_equal_autograd_through_spectral_norm(kind):
    """4 training-mode calls of a spectral-normed layer, one loss over all of them: autograd's gradient of weight_orig and bias and the
    final u, v against per-call sigma -> rowscale_bwd_ref (gs, dots, dbias) -> the weight gradient of the scaled rows -> sn_bwd_frames_ref"""
    torch.manual_seed(11)
    calls, cin, cout = 4, 6, 5
    if kind == "conv":
        mod, c, act = torch.nn.Conv2d(cin, cout, 3, padding=1), X.SnCase(cout, cin, 9, 0), _lib.ACT_ELU
        lin = lambda x, w: F.conv2d(x, w, None, padding=1)                                         # noqa: E731
    else:
        mod, c, act = torch.nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1), X.SnCase(cout, cin, 9, 1), _lib.ACT_LRELU02
        lin = lambda x, w: F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1)   # noqa: E731
    mod = torch.nn.utils.spectral_norm(mod.double(), eps=X.EPS).train()
    u, v = mod.weight_u.clone(), mod.weight_v.clone()
    xs = [torch.randn(2, cin, 4, 5, dtype=F64) for _ in range(calls)]
    outs = [X.act64(act, mod(x)) for x in xs]
    qs = [torch.randn_like(o) for o in outs]
    sum((o * q).sum() for o, q in zip(outs, qs)).backward()
    # ---- the same from the references
    w = mod.weight_orig.detach()
    b = mod.bias.detach()
    W = X.to_matrix(w.reshape(*w.shape[:2], 9), c)
    us, vs, sig, ys = [], [], [], []
    for x in xs:
        st = X.power_iteration_ref(W, u, v)
        u, v = st["u"], st["v"]
        us.append(u); vs.append(v); sig.append(st["sigma"])
        ys.append(X.act64(act, lin(x, w) / st["sigma"] + b.view(1, -1, 1, 1)))
    close(torch.stack(ys), torch.stack([o.detach() for o in outs]))
    close(u, mod.weight_u)
    close(v, mod.weight_v)
    inv = 1.0 / torch.stack(sig)
    rows = rows_of(ys[0]).shape[0]
    r = X.rowscale_bwd_ref(torch.cat([rows_of(q) for q in qs]), torch.cat([rows_of(y) for y in ys]), act, b, inv, rows)
    close(r["dbias"], mod.bias.grad, 1e-11)
    wp = w.clone().requires_grad_(True)
    gs = torch.cat([nchw_of(r["gs"][t * rows: (t + 1) * rows], ys[t]) for t in range(calls)])
    dW, = torch.autograd.grad(lin(torch.cat(xs), wp), wp, gs)                       # the weight gradient of the rows scaled by 1 / sigma_t
    out, _ = X.sn_bwd_frames_ref(X.to_matrix(dW.reshape(*w.shape[:2], 9), c), torch.stack(us), torch.stack(vs), inv, r["dots"])
    close(X.from_matrix(out, c).reshape(w.shape), mod.weight_orig.grad, 1e-11)


@pytest.mark.parametrize("c", X.SN_BWD_CASES[:2], ids=X.sn_id)
def test_sn_bwd_ref_equals_autograd(c):
    """(G - <G, W / sigma> u v^T) / sigma is the gradient of sum(G * W / (u . W v)) with u, v constants"""
    w, G, us, vs, _, _ = X.sn_bwd_operands(c, 1)
    W = X.to_matrix(w, c).clone().requires_grad_(True)
    sigma = us[0] @ W @ vs[0]
    Gm = X.to_matrix(G, c)
    g, = torch.autograd.grad((Gm * W / sigma).sum(), W)
    out, _ = X.sn_bwd_ref(Gm, W.detach(), us[0], vs[0], 1.0 / sigma.detach())
    close(out, g, 1e-11)
    assert torch.equal(X.to_matrix(X.from_matrix(Gm, c), c), Gm)


def test_power_iteration_edges_follow_f_normalize():
    for name in X.SN_EDGES:
        c = X.SN_EDGES[name]
        w, u, v = X.sn_edge_operands(name)
        W = X.to_matrix(w, c)
        st = X.power_iteration_ref(W, u, v)
        tv = W.t() @ u
        assert float(tv.norm()) < X.EPS
        v1 = F.normalize(tv, dim=0, eps=X.EPS)
        u1 = F.normalize(W @ v1, dim=0, eps=X.EPS)
        close(st["v"], v1)
        close(st["u"], u1)
        close(st["sigma"], u1 @ (W @ v1))
        assert torch.equal(st["v"], tv / X.EPS)
        if name == "zero":
            assert not bool(st["u"].any()) and not bool(st["v"].any()) and float(st["sigma"]) == 0.0 and float(1.0 / st["sigma"]) == float("inf")
        else:
            assert 0 < float(st["v"].norm()) < 0.5 and 0 < float(st["sigma"]) < 1e-10         # not unit length; sigma finite and positive
            # every intermediate is a normal fp32 number, squares included
            for t in (tv, st["tu"], st["u"] * st["tu"]):
                assert float((t * t)[t != 0].abs().min()) > 2.0 ** -120


def test_wop_ref_is_the_indexing_of_the_header():
    for c in X.WOP_CASES[:4]:
        kc = X.round_up(c.cin, 8) + 8
        w = f32r(torch.randn(X.storage_shape(c), dtype=F64, generator=torch.Generator().manual_seed(c.cout)))
        out = X.wop_ref(w, c, kc)
        for o, ci, t in [(0, 0, 0), (c.cout - 1, c.cin - 1, c.taps - 1), (c.cout // 2, c.cin // 2, c.taps // 2)]:
            assert float(out[o, t * kc + ci]) == float(w[ci, o, t] if c.transposed else w[o, ci, t])
        assert float(out.reshape(c.cout, c.taps, kc)[:, :, c.cin:].abs().max()) == 0.0
        s = X.scalar(0.3)
        assert torch.equal(X.wop_ref(w, c, kc, s)[:, : c.cin], f32r(s * out[:, : c.cin]))


def test_kl_ref_equals_autograd():
    c = X.KL_CASES[0]
    mu, lv = (t.clone().requires_grad_(True) for t in X.kl_operands(c))
    kl = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp()) / c.positions
    gm, gl = torch.autograd.grad(kl, [mu, lv])
    r = X.kl_ref(mu.detach(), lv.detach(), c.positions, torch.tensor(X.KL_LOSS0, dtype=F64))
    close(r["loss"], kl.detach() + X.KL_LOSS0)
    close(r["dmu"], gm)
    close(r["dlv"], gl)


def test_adam_ref_equals_torch_adam():
    h = X.adam_hyper()
    p0, gs = X.adam_operands()
    p0 = p0[:5000]
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([param], lr=float(h["lr"]), betas=(float(h["beta1"]), float(h["beta2"])), eps=float(h["eps"]),
                           weight_decay=float(h["weight_decay"]))
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for step in (1, 2, 3):
        g = gs[step - 1][:5000]
        param.grad = g * h["grad_scale"]
        opt.step()
        r = X.adam_ref(p, g, m, v, step, **h)
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[param]
        close(p, param.detach())
        close(m, st["exp_avg"])
        close(v, st["exp_avg_sq"])
    assert float(h["weight_decay"]) > 0 and float(h["grad_scale"]) not in (0.0, 1.0) and float(h["beta1"]) != float(h["beta2"])


# ------------------------------------------------------------------ operand conditions
def test_sn_cases_reach_their_loops_and_sigma_stays_away_from_zero():
    R = [c.cout for c in X.SN_CASES]
    C = [c.cin * c.taps for c in X.SN_CASES]
    assert min(R) < 4 and max(R) > 256 and any(k > 256 and k % 32 for k in C) and any(r % 4 for r in R) and any(c.transposed for c in X.SN_CASES)
    assert R.index(max(R)) != C.index(max(C))                  # max_rows and max_cols of the multi table come from different jobs
    for c in X.SN_CASES:
        w, u, v = X.sn_operands(c)
        W = X.to_matrix(w, c)
        for _ in range(7):
            st = X.power_iteration_ref(W, u, v)
            u, v = st["u"], st["v"]
            assert float(st["sigma"]) > 0.05
        assert float(X.power_iteration_ref(W, *X.sn_operands(c)[1:], iterate=False)["sigma"].abs()) > 1e-4


def test_grid_stride_cases_wrap():
    big = X.WOP_CASES[-1]
    assert big.cout * big.taps * X.round_up(big.cin, 4) > 4096 * 256
    jobs = X.wop_multi_cases()
    assert len(jobs) == 70 > 64 and X.WOP_MULTI_BIG < 64
    j = jobs[X.WOP_MULTI_BIG]
    assert j.cout * j.taps * X.round_up(j.cin, 8) > 65536 and all(q.cout * q.taps * X.round_up(q.cin, 8) < 65536 for q in jobs if q is not j)
    parts = sorted({min(256, -(-c.cout * c.cin * c.taps // 256)) for c in X.SN_BWD_CASES})
    assert parts == [37, 256] and 260 * 297 > 256 * 256
    sizes = [c.shape.cout * c.shape.cin * c.shape.taps for c in X.SN_BWD_FRAMES_CASES]
    assert max(sizes) > 2048 * 256 and {c.frames for c in X.SN_BWD_FRAMES_CASES} == {1, 5} and {c.sig_stride for c in X.SN_BWD_FRAMES_CASES} == {2, 3}
    assert all(c.snap_extra > 0 for c in X.SN_BWD_FRAMES_CASES) and {c.shape.transposed for c in X.SN_BWD_FRAMES_CASES} == {0, 1}
    assert X.SUM_WRAP_VECS > 4096 * 256
    n = [c.positions * c.Z for c in X.KL_CASES]
    assert n[0] == 3 * 64 * 32 and n[2] == 1 << 20 and n[3] == (1 << 20) + 4096
    sizes = X.adam_sizes()
    assert len(sizes) == 49 and 1 in sizes and max(sizes) > 65536


def test_rowscale_cases_reach_their_loops():
    by = {c.name: c for c in X.RS_CASES}
    for dt in ("f32", "bf16"):
        e16 = DTYPES[dt][2]
        for c in X.RS_CASES:
            C = c.C_bf16 if dt == "bf16" else c.C_f32
            ngroups, nbx = X.rs_blocks(c, C)
            nblk, trips = ngroups * nbx, -(-(X.round_up(C, e16) // e16) // 256)
            if c.name == "eight":
                eight = [len(range(rl, nblk - 112, 128)) for rl in range(16)]            # rowscale_final_kernel's two loops per row lane
                tail = [len(range(rl + 128 * n8, nblk, 16)) for rl, n8 in enumerate(eight)]
                assert nblk == 141 and min(eight) >= 1 and max(tail) >= 1 and min(tail) == 0
            else:
                assert nblk < 113
            assert trips == (2 if c.name == "trip" else 1)
    assert not by["nodbias"].dbias and not by["nobias"].bias and {c.act for c in X.RS_CASES[:4]} == set(X.ACT_IDS.values())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rowscale_operands_hold_the_edges(dt):
    tdt = DTYPES[dt][1]
    for c in X.RS_CASES:
        d = X.rs_operands(c, dt)
        y = d["y"]
        assert torch.equal(as_seen(y, tdt), y) and torch.equal(as_seen(d["dy"], tdt), d["dy"])
        if c.act == _lib.ACT_ELU:
            nxt = y[y > -1].min()
            assert int((y == -1).sum()) >= 2 * c.groups and float(nxt) == -1 + (2.0 ** -8 if tdt == BF16 else 2.0 ** -24)
            assert bool((y >= -1).all())
            r = X.rowscale_bwd_ref(d["dy"], y, c.act, d["bias"], d["scale"], c.rows)
            assert bool(torch.isfinite(r["dots"]).all()) and bool(torch.isfinite(r["dots_mag"]).all())
        if c.act == _lib.ACT_RELU:
            assert 0.3 < float((y == 0).double().mean()) < 0.7


def test_sum_operands_are_exact_where_the_test_says_so():
    for dt in ("f32", "bf16"):
        tdt = DTYPES[dt][1]
        for frames in X.SUM_FRAMES:
            i = X.sum_operands(frames, X.SUM_N, tdt, True)
            assert bool((i == i.round()).all()) and float(i.abs().max()) <= 8
            s = X.sum_frames_ref(i)
            assert torch.equal(cast_like(s, tdt).to(F64), s)                     # every integer sum is a bf16 / fp32 number
            r = X.sum_operands(frames, X.SUM_N, tdt, False)
            assert torch.equal(as_seen(r, tdt), r) and not bool((r == r.round()).all())
            for order in (range(frames), reversed(range(frames))):              # fp32 accumulation is exact in any order
                acc = torch.zeros(X.SUM_N, dtype=F32)
                for f in order:
                    acc = acc + r[f].to(F32)
                assert torch.equal(acc.to(F64), X.sum_frames_ref(r))
            if dt == "bf16" and frames > 1:
                assert not torch.equal(cast_like(X.sum_frames_ref(r), tdt).to(F64), X.sum_frames_ref(r))      # ... and really rounded in bf16


# ------------------------------------------------------------------ the yardsticks
@functools.lru_cache(maxsize=None)
def sn_phase_errors():
    e = dict(sn_tv=0.0, sn_v=0.0, sn_tu=0.0, sn_u=0.0, sn_sigma=0.0)
    sets = [(c, X.sn_operands(c)) for c in X.SN_CASES] + [(X.SN_EDGES[k], X.sn_edge_operands(k)) for k in X.SN_EDGES]
    for c, (w, u, v) in sets:
        W = X.to_matrix(w, c)
        for _ in range(2):
            tv, tv_mag = X.matvec_t_ref(W, u)
            e["sn_tv"] = max(e["sn_tv"], err_units(restate(X.matvec_t_ref, W, u)[0], tv, tv_mag))
            tv = f32r(tv)                                                     # "stored": what the next phase reads
            v = X.normalize_ref(tv)
            e["sn_v"] = max(e["sn_v"], err_units(restate(X.normalize_ref, tv), v, v))
            v = f32r(v)
            tu, tu_mag = X.matvec_ref(W, v)
            e["sn_tu"] = max(e["sn_tu"], err_units(restate(X.matvec_ref, W, v)[0], tu, tu_mag))
            tu = f32r(tu)
            u = X.normalize_ref(tu)
            e["sn_u"] = max(e["sn_u"], err_units(restate(X.normalize_ref, tu), u, u))
            u = f32r(u)
            s, s_mag = X.dot_ref(u, tu)
            e["sn_sigma"] = max(e["sn_sigma"], err_units(restate(X.dot_ref, u, tu)[0], s, s_mag))
    return e


@functools.lru_cache(maxsize=None)
def sn_bwd_errors():
    worst = 0.0
    for c in X.SN_BWD_CASES:
        w, G, us, vs, sig, _ = X.sn_bwd_operands(c, 1)
        args = (X.to_matrix(G, c), X.to_matrix(w, c), us[0], vs[0], sig[0, 1])
        ref, mag = X.sn_bwd_ref(*args)
        worst = max(worst, err_units(restate(X.sn_bwd_ref, *args)[0], ref, mag))
    return dict(sn_bwd=worst)


@functools.lru_cache(maxsize=None)
def sn_bwd_frames_errors():
    worst = 0.0
    for fc in X.SN_BWD_FRAMES_CASES:
        _, G, us, vs, sig, dots = X.sn_bwd_operands(fc.shape, fc.frames)
        args = (X.to_matrix(G, fc.shape), us, vs, sig[:, 1].contiguous(), dots)
        ref, mag = X.sn_bwd_frames_ref(*args)
        worst = max(worst, err_units(restate(X.sn_bwd_frames_ref, *args)[0], ref, mag))
    return dict(sn_bwd_frames=worst)


@functools.lru_cache(maxsize=None)
def rowscale_errors():
    e = dict(rowscale_gs=0.0, rowscale_dots=0.0, rowscale_dbias=0.0)
    for c in X.RS_CASES:
        for dt in c.dts:
            tdt = DTYPES[dt][1]
            d = X.rs_operands(c, dt)
            args = (d["dy"], d["y"], c.act, d["bias"], d["scale"], c.rows)
            ref, rs = X.rowscale_bwd_ref(*args), restate(X.rowscale_bwd_ref, *args)
            e["rowscale_gs"] = max(e["rowscale_gs"], err_units(cast_like(rs["gs"].to(F64), tdt), ref["gs"], ref["gs"], tdt))
            e["rowscale_dots"] = max(e["rowscale_dots"], err_units(rs["dots"], ref["dots"], ref["dots_mag"]))
            e["rowscale_dbias"] = max(e["rowscale_dbias"], err_units(rs["dbias"], ref["dbias"], ref["dbias_mag"]))
    return e


@functools.lru_cache(maxsize=None)
def sum_frames_errors():
    worst = 0.0
    for dt in ("f32", "bf16"):
        tdt = DTYPES[dt][1]
        for frames in X.SUM_FRAMES:
            r = X.sum_operands(frames, X.SUM_N, tdt, False)
            ref = X.sum_frames_ref(r)
            worst = max(worst, err_units(cast_like(restate(X.sum_frames_ref, r).to(F64), tdt), ref, ref, tdt))
    return dict(sum_frames=worst)


@functools.lru_cache(maxsize=None)
def adam_errors():
    e = dict(adam_p=0.0, adam_m=0.0, adam_v=0.0)
    h = X.adam_hyper()
    p, gs = X.adam_operands()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in zip(X.ADAM_STEPS, gs):
        ref, rs = X.adam_ref(p, g, m, v, step, **h), restate(X.adam_ref, p, g, m, v, step, **h)
        for k in "pmv":
            e["adam_" + k] = max(e["adam_" + k], err_units(rs[k], ref[k], ref[k + "_mag"]))
        p, m, v = f32r(ref["p"]), f32r(ref["m"]), f32r(ref["v"])
    return e


@functools.lru_cache(maxsize=None)
def kl_errors():
    e = dict(kl_value=0.0, kl_dmu=0.0, kl_dlv=0.0)
    for c in X.KL_CASES:
        mu, lv = X.kl_operands(c)
        l0 = torch.tensor(X.KL_LOSS0, dtype=F64)
        ref, rs = X.kl_ref(mu, lv, c.positions, l0), restate(X.kl_ref, mu, lv, c.positions, l0)
        e["kl_value"] = max(e["kl_value"], err_units(rs["loss"], ref["loss"], ref["loss_mag"]))
        e["kl_dmu"] = max(e["kl_dmu"], err_units(rs["dmu"], ref["dmu"], ref["dmu"]))
        e["kl_dlv"] = max(e["kl_dlv"], err_units(rs["dlv"], ref["dlv"], ref["dlv_mag"]))
    return e


MEASURES = [sn_phase_errors, sn_bwd_errors, sn_bwd_frames_errors, rowscale_errors, sum_frames_errors, adam_errors, kl_errors]


@pytest.mark.parametrize("measure", MEASURES, ids=lambda f: f.__name__)
def test_restatement_stays_within_the_recorded_yardstick(measure):
    for key, err in measure().items():
        print(f"yardstick {key}: restatement {err:.3f} units, recorded {YARDSTICK[key]}, GPU bound {X.gpu_bound(key)}")
        assert err <= YARDSTICK[key], (key, err)
        assert YARDSTICK[key] <= 2.0 * err + 1.0, f"{key}: the recorded yardstick is far above the measured {err:.3f}"


def test_every_yardstick_is_measured():
    measured = set()
    for f in MEASURES:
        measured |= set(f())
    assert measured == set(YARDSTICK)
