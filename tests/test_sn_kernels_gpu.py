"""The first stage's parameter kernels (csrc/vae_train.hip) one by one through the C ABI against the float64 references of
tests/sn_exact.py: the weight-operand writer, the power iteration phase by phase on the values the kernels stored, its multi-weight
form bit for bit against the single calls, the spectral-norm backward (single and per frame), the row-scale backward, the frame sum,
the multi-tensor Adam (p, m and v) and the KL term.  Exact where the arithmetic is, within sn_exact.gpu_bound elsewhere; every buffer
is followed by sentinels and every element is compared."""
import ctypes

import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd._lib import ptr
from tests import sn_exact as X
from tests.sn_exact import DTYPES, F32, F64, SENT, assert_close_ulp, assert_same, assert_units, check_guard, gpu_bound, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 64


def lib():
    return _lib.lib()


def run(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def stream():
    return _lib.current_stream()


def flat(n, values=None, dtype=F32, tail=TAIL):
    """n elements (SENT, or `values`) followed by `tail` elements of SENT"""
    b = torch.full((n + tail,), SENT, dtype=dtype, device=DEV)
    if values is not None:
        b[:n] = values.reshape(-1).to(dtype).to(DEV)
    return b


def tail_ok(b, n, what):
    assert bool((b[n:].to(F64) == SENT).all()), what + ": write behind the buffer"


def host(b, n=None):
    return (b if n is None else b[:n]).to(F64).cpu()


def units(key, got, ref, mag, tdt, what):
    """every element within gpu_bound(key) units; the worst is printed first (pytest -s), for the table of DESIGN.md"""
    print(f"measured {key}: {X.err_units(got, ref, mag, tdt):.3f} of {gpu_bound(key)} units ({what})")
    assert_units(got, ref, mag, gpu_bound(key), tdt, what)


def unchanged(b, before, what):
    assert torch.equal(b, before), what + ": an input changed"


# ------------------------------------------------------------------ operand writer
def wop_kc(c, e16):
    """a pitch per tap that always has padding columns"""
    kc = X.round_up(c.cin, e16)
    return kc + e16 if kc == c.cin else kc


def wop_weight(c, kc, seed):
    """the weight behind enough sentinels that even the padding columns' would-be sources lie inside the buffer"""
    w = X.f32r(torch.randn(X.storage_shape(c), generator=torch.Generator().manual_seed(seed), dtype=F64))
    return w, flat(w.numel(), w, tail=(kc - c.cin) * c.cout * c.taps + TAIL)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "inv_scale"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", X.WOP_CASES, ids=X.sn_id)
def test_weight_operand_is_bit_exact(c, dt, scaled):
    code, tdt, e16 = DTYPES[dt]
    kc = wop_kc(c, e16)
    assert kc > c.cin and kc % e16 == 0
    w, wb = wop_weight(c, kc, 7 + c.cout)
    s = X.scalar(0.37) if scaled else None
    sb = flat(1, s) if scaled else None
    out = guarded(c.cout, c.taps * kc, tdt, DEV)
    before = wb.clone()
    run(lib().ipoke_conv_weight_operand(ptr(wb), c.cout, c.cin, c.taps, c.transposed, ptr(sb), ptr(out), kc, code, stream()))
    what = f"weight operand {X.sn_id(c)} {dt}"
    assert_same(out[: c.cout].contiguous(), X.wop_ref(w, c, kc, s), what, lambda i: f"row {i // (c.taps * kc)} tap {i // kc % c.taps} column {i % kc}")
    check_guard(out, c.cout, c.taps * kc, None, what)
    unchanged(wb, before, what)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_weight_operand_multi_equals_the_single_calls(dt):
    code, tdt, e16 = DTYPES[dt]
    cases = X.wop_multi_cases()
    n = len(cases)
    kcs = [wop_kc(c, e16) for c in cases]
    ws = [wop_weight(c, kc, 40 + i) for i, (c, kc) in enumerate(zip(cases, kcs))]
    outs = [guarded(c.cout, c.taps * kc, tdt, DEV) for c, kc in zip(cases, kcs)]
    singles = [guarded(c.cout, c.taps * kc, tdt, DEV) for c, kc in zip(cases, kcs)]
    wp = (ctypes.c_void_p * n)(*[b.data_ptr() for _, b in ws])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    dims = (ctypes.c_int32 * (5 * n))(*[x for c, kc in zip(cases, kcs) for x in (c.cout, c.cin, c.taps, c.transposed, kc)])
    run(lib().ipoke_conv_weight_operand_multi(wp, op, dims, n, code, stream()))
    for i, (c, kc) in enumerate(zip(cases, kcs)):
        _lib.check(lib().ipoke_conv_weight_operand(ptr(ws[i][1]), c.cout, c.cin, c.taps, c.transposed, None, ptr(singles[i]), kc, code, stream()))
    torch.cuda.synchronize()
    for i, (c, kc) in enumerate(zip(cases, kcs)):
        what = f"weight operand multi job {i} ({X.sn_id(c)}) {dt}"
        where = lambda k, kc=kc, c=c: f"row {k // (c.taps * kc)} tap {k // kc % c.taps} column {k % kc}"        # noqa: E731
        assert_same(outs[i], singles[i], what + " against the single call", where)
        assert_same(outs[i][: c.cout].contiguous(), X.wop_ref(ws[i][0], c, kc), what, where)
        check_guard(outs[i], c.cout, c.taps * kc, None, what)


# ------------------------------------------------------------------ the power iteration, phase by phase
def sn_buffers(c, w, u, v, iterations=1, out_stride=2, snap_extra=0):
    R, C = c.cout, c.cin * c.taps
    nws = int(lib().ipoke_spectral_workspace_floats(c.cout, c.cin, c.taps))
    assert nws == 4 + R + C
    return dict(w=flat(w.numel(), w), u=flat(R, u), v=flat(C, v), out=flat(iterations * out_stride), snap=flat(iterations * (R + C + snap_extra)),
                ws=flat(nws, torch.zeros(nws)), R=R, C=C, nws=nws)


def sigma_call(c, b, iterate, out_off=0, snap_off=0, eps=X.EPS):
    run(lib().ipoke_spectral_sigma(ptr(b["w"]), c.cout, c.cin, c.taps, c.transposed, ptr(b["u"]), ptr(b["v"]), iterate, eps, ptr(b["out"][out_off:]),
                                   ptr(b["snap"][snap_off:]), ptr(b["ws"]), stream()))


def check_phases(c, w, u0, v0, b, iterate, what):
    """every phase of one call on the values the kernels stored; u0, v0: the vectors the call began with (float64)"""
    R, C = b["R"], b["C"]
    W = X.to_matrix(w, c)
    ws = host(b["ws"], b["nws"])
    tu_s, tv_s, u_s, v_s, out = ws[4: 4 + R], ws[4 + R:], host(b["u"], R), host(b["v"], C), host(b["out"], 2)
    if iterate:
        tv, mag = X.matvec_t_ref(W, u0)
        units("sn_tv", tv_s, tv, mag, F32, what + ": tv = W^T u")
        v = X.normalize_ref(tv_s)
        units("sn_v", v_s, v, v, F32, what + ": v = tv / max(||tv||, eps)")
    else:
        assert_same(b["v"][:C], v0, what + ": v without iteration")
        assert_same(b["u"][:R], u0, what + ": u without iteration")
    tu, mag = X.matvec_ref(W, v_s)
    units("sn_tu", tu_s, tu, mag, F32, what + ": tu = W v")
    if iterate:
        u = X.normalize_ref(tu_s)
        units("sn_u", u_s, u, u, F32, what + ": u = tu / max(||tu||, eps)")
    s, mag = X.dot_ref(u_s, tu_s)
    units("sn_sigma", out[0], s, mag, F32, what + ": sigma = u . tu")
    assert_same(b["out"][1:2].cpu(), 1.0 / b["out"][0:1].cpu(), what + ": 1 / sigma")          # the correctly rounded fp32 quotient
    assert_same(b["snap"][: R + C], torch.cat([b["u"][:R], b["v"][:C]]), what + ": snapshot = u | v")
    assert bool((ws[:4] == 0).all()), what + ": the reserved words of the workspace"
    for k, n in (("w", w.numel()), ("u", R), ("v", C), ("out", 2), ("snap", R + C), ("ws", b["nws"])):
        tail_ok(b[k], n, f"{what}: {k}")
    assert_same(b["w"][: w.numel()], w, what + ": the weight")
    return u_s, v_s


@pytest.mark.parametrize("c", X.SN_CASES, ids=X.sn_id)
def test_power_iteration_phase_by_phase(c):
    w, u, v = X.sn_operands(c)
    b = sn_buffers(c, w, u, v)
    for call in range(2):                                      # the second call begins with what the first one stored
        sigma_call(c, b, 1)
        u, v = check_phases(c, w, u, v, b, True, f"spectral_sigma {X.sn_id(c)} call {call}")
    assert abs(float(u.norm()) - 1) < 1e-5 and abs(float(v.norm()) - 1) < 1e-5


@pytest.mark.parametrize("c", X.SN_CASES, ids=X.sn_id)
def test_sigma_without_iteration_leaves_u_and_v(c):
    w, u, v = X.sn_operands(c)
    b = sn_buffers(c, w, u, v)
    sigma_call(c, b, 0)
    check_phases(c, w, u, v, b, False, f"spectral_sigma {X.sn_id(c)} iterate = 0")      # tu against W v and sigma against u . tu on the given u, v


def test_power_iteration_of_a_zero_weight():
    c = X.SN_EDGES["zero"]
    w, u, v = X.sn_edge_operands("zero")
    b = sn_buffers(c, w, u, v)
    sigma_call(c, b, 1)
    check_phases(c, w, u, v, b, True, "spectral_sigma zero weight")
    u_s, v_s, out = host(b["u"], b["R"]), host(b["v"], b["C"]), host(b["out"], 2)
    assert not bool(u_s.any()) and not bool(v_s.any()), "u = v = 0 (F.normalize of a zero vector), no NaN"
    assert float(out[0]) == 0.0 and float(out[1]) == float("inf")


def test_power_iteration_below_eps():
    c = X.SN_EDGES["eps"]
    w, u, v = X.sn_edge_operands("eps")
    b = sn_buffers(c, w, u, v)
    sigma_call(c, b, 1)
    check_phases(c, w, u, v, b, True, "spectral_sigma ||W^T u|| < eps")
    ws, v_s, out = host(b["ws"], b["nws"]), host(b["v"], b["C"]), host(b["out"], 2)
    tv_s = ws[4 + b["R"]:]
    assert float(tv_s.norm()) < X.EPS
    units("sn_v", v_s, tv_s / X.EPS, tv_s / X.EPS, F32, "v = tv / eps")
    assert 0 < float(v_s.norm()) < 0.5 and 0 < float(out[0]) < 1e-10 and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ many weights per launch
def multi_table():
    return [(c, X.sn_operands(c)) for c in X.SN_CASES] + [(X.SN_EDGES[k], X.sn_edge_operands(k)) for k in X.SN_EDGES]


OUT_STRIDE, SNAP_EXTRA = 3, 5


def run_sequential(table, iterations):
    bufs = []
    for c, (w, u, v) in table:
        b = sn_buffers(c, w, u, v, iterations, OUT_STRIDE, SNAP_EXTRA)
        for k in range(iterations):
            sigma_call(c, b, 1, k * OUT_STRIDE, k * (b["R"] + b["C"] + SNAP_EXTRA))
        bufs.append(b)
    return bufs


def run_multi(table, iterations):
    n = len(table)
    jobs = (_lib.SnJob * n)()
    bufs = []
    for j, (c, (w, u, v)) in zip(jobs, table):
        b = sn_buffers(c, w, u, v, iterations, OUT_STRIDE, SNAP_EXTRA)
        j.w = b["w"].data_ptr(); j.cout, j.cin, j.taps, j.transposed = c
        j.u = b["u"].data_ptr(); j.v = b["v"].data_ptr(); j.out = b["out"].data_ptr(); j.out_stride = OUT_STRIDE
        j.snap = b["snap"].data_ptr(); j.snap_stride = b["R"] + b["C"] + SNAP_EXTRA; j.workspace = b["ws"].data_ptr()
        bufs.append(b)
    size = n * int(lib().ipoke_sn_job_size())
    jobs_dev = torch.full((size + 256,), 0x55, dtype=torch.uint8, device=DEV)
    run(lib().ipoke_sn_jobs_upload(ctypes.byref(jobs), n, ptr(jobs_dev), stream()))
    assert bool((jobs_dev[size:] == 0x55).all()), "the job table was written past its size"
    rows = [c.cout for c, _ in table]
    cols = [c.cin * c.taps for c, _ in table]
    assert rows.index(max(rows)) != cols.index(max(cols))
    run(lib().ipoke_spectral_sigma_multi(ptr(jobs_dev), n, max(rows), max(cols), iterations, X.EPS, stream()))
    return bufs


SN_KEYS = ("out", "snap", "u", "v", "ws", "w")


def assert_runs_equal(a, b, table, what):
    for (c, _), x, y in zip(table, a, b):
        for k in SN_KEYS:
            assert_same(x[k], y[k], f"{what}: {k} of job {X.sn_id(c)}")


@pytest.mark.parametrize("iterations", [1, 7])
def test_sigma_multi_equals_the_sequential_single_calls(iterations):
    table = multi_table()
    seq, multi = run_sequential(table, iterations), run_multi(table, iterations)
    for (c, _), b in zip(table, multi):
        R, C = b["R"], b["C"]
        out, snap = host(b["out"]).reshape(-1)[: iterations * OUT_STRIDE].reshape(iterations, OUT_STRIDE), host(b["snap"])
        assert bool((out[:, 2:] == SENT).all()), f"job {X.sn_id(c)}: the gap of out_stride"
        snap = snap[: iterations * (R + C + SNAP_EXTRA)].reshape(iterations, R + C + SNAP_EXTRA)
        assert bool((snap[:, R + C:] == SENT).all()), f"job {X.sn_id(c)}: the gap of snap_stride"
        for k, n in (("w", b["w"].numel() - TAIL), ("u", R), ("v", C), ("out", iterations * OUT_STRIDE), ("snap", snap.numel()), ("ws", b["nws"])):
            tail_ok(b[k], n, f"job {X.sn_id(c)}: {k}")
        assert bool((host(b["ws"], 4) == 0).all()), f"job {X.sn_id(c)}: the reserved words of the workspace"
        assert_same(b["snap"][(iterations - 1) * (R + C + SNAP_EXTRA):][: R + C], torch.cat([b["u"][:R], b["v"][:C]]), "the last snapshot = final u | v")
    # {sigma, 1 / sigma} of every iteration, every snapshot, the final u and v (and the workspace's tu | tv): the same arithmetic, call by call
    assert_runs_equal(multi, seq, table, f"multi against sequential, {iterations} iterations")


def test_sigma_is_reproducible_run_to_run():
    table = multi_table()
    assert_runs_equal(run_multi(table, 7), run_multi(table, 7), table, "two runs of the multi form")
    assert_runs_equal(run_sequential(table, 3), run_sequential(table, 3), table, "two runs of the single calls")


# ------------------------------------------------------------------ spectral-norm backward
@pytest.mark.parametrize("c", X.SN_BWD_CASES, ids=X.sn_id)
def test_spectral_bwd(c):
    R, C = c.cout, c.cin * c.taps
    n = R * C
    w, G, us, vs, sig, _ = X.sn_bwd_operands(c, 1)
    nws = int(lib().ipoke_spectral_bwd_workspace_floats())
    parts = min(nws, -(-n // 256))

    def once():
        b = dict(w=flat(n, w), g=flat(n, G), snap=flat(R + C, torch.cat([us[0], vs[0]])), sig=flat(2, sig[0]), ws=flat(nws))     # ws: SENT, no initialisation
        keep = {k: b[k].clone() for k in ("w", "snap", "sig")}
        run(lib().ipoke_spectral_bwd(ptr(b["w"]), c.cout, c.cin, c.taps, c.transposed, ptr(b["g"]), ptr(b["snap"]), ptr(b["sig"]), ptr(b["ws"]), stream()))
        for k in keep:
            unchanged(b[k], keep[k], f"spectral_bwd {k}")
        return b

    b = once()
    ref, mag = X.sn_bwd_ref(X.to_matrix(G, c), X.to_matrix(w, c), us[0], vs[0], sig[0, 1])
    what = f"spectral_bwd {X.sn_id(c)}"
    units("sn_bwd", X.to_matrix(host(b["g"], n), c), ref, mag, F32, what)
    tail_ok(b["g"], n, what)
    assert bool((host(b["ws"])[parts:] == SENT).all()), what + f": the workspace behind its {parts} partials"
    again = once()
    assert_same(again["g"], b["g"], what + ": two runs")
    assert_same(again["ws"], b["ws"], what + ": two runs, partials")


@pytest.mark.parametrize("fc", X.SN_BWD_FRAMES_CASES, ids=lambda fc: f"{X.sn_id(fc.shape)}-f{fc.frames}-s{fc.sig_stride}")
def test_spectral_bwd_frames(fc):
    c, T = fc.shape, fc.frames
    R, C = c.cout, c.cin * c.taps
    n, ss = R * C, R + C + fc.snap_extra
    w, G, us, vs, sig, dots = X.sn_bwd_operands(c, T)
    snap = torch.full((T, ss), SENT, dtype=F64)
    snap[:, :R], snap[:, R: R + C] = us, vs
    sg = torch.full((T, fc.sig_stride), SENT, dtype=F64)
    sg[:, :2] = sig
    b = dict(w=flat(n, w), g=flat(n, G), snap=flat(T * ss, snap), sig=flat(T * fc.sig_stride, sg), dots=flat(T, dots))
    keep = {k: b[k].clone() for k in ("w", "snap", "sig", "dots")}
    run(lib().ipoke_spectral_bwd_frames(ptr(b["w"]), c.cout, c.cin, c.taps, c.transposed, ptr(b["g"]), ptr(b["snap"]), ss, ptr(b["sig"]), fc.sig_stride,
                                        ptr(b["dots"]), T, stream()))
    what = f"spectral_bwd_frames {X.sn_id(c)} frames {T}"
    for k in keep:
        unchanged(b[k], keep[k], f"{what}: {k}")
    ref, mag = X.sn_bwd_frames_ref(X.to_matrix(G, c), us, vs, sig[:, 1], dots)
    units("sn_bwd_frames", X.to_matrix(host(b["g"], n), c), ref, mag, F32, what)
    tail_ok(b["g"], n, what)


# ------------------------------------------------------------------ row-scale backward
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", X.RS_CASES, ids=lambda c: c.name)
def test_rowscale_bwd(case, dt):
    code, tdt, e16 = DTYPES[dt]
    d = X.rs_operands(case, dt)
    C, M, groups = d["C"], d["M"], case.groups
    Cpad = X.round_up(C, e16)
    lddy, ldy, ldgs = Cpad + e16, Cpad + 2 * e16, Cpad + 3 * e16
    nws = int(lib().ipoke_rowscale_bwd_workspace_floats(M, C, case.rows))
    sc = torch.full((groups, X.RS_SCALE_STRIDE), SENT, dtype=F64)
    sc[:, 0] = d["scale"]
    b = dict(dy=guarded(M, lddy, tdt, DEV, d["dy"].to(DEV)), y=guarded(M, ldy, tdt, DEV, d["y"].to(DEV)), gs=guarded(M, ldgs, tdt, DEV),
             scale=flat(groups * X.RS_SCALE_STRIDE, sc), dots=flat(groups), dbias=flat(C) if case.dbias else None,
             bias=flat(C, d["bias"]) if case.bias else None, ws=flat(nws))
    keep = {k: b[k].clone() for k in ("dy", "y", "scale")}
    q = _lib.RowScaleBwdDesc()
    q.dy, q.lddy, q.y, q.ldy, q.M, q.C, q.Cpad, q.act = b["dy"].data_ptr(), lddy, b["y"].data_ptr(), ldy, M, C, Cpad, case.act
    q.bias = b["bias"].data_ptr() if case.bias else None
    q.scale, q.scale_stride, q.rows_per_group = b["scale"].data_ptr(), X.RS_SCALE_STRIDE, case.rows
    q.gs, q.ldgs, q.dots = b["gs"].data_ptr(), ldgs, b["dots"].data_ptr()
    q.dbias = b["dbias"].data_ptr() if case.dbias else None
    q.workspace = b["ws"].data_ptr()
    run(lib().ipoke_rowscale_bwd(ctypes.byref(q), code, stream()))
    what = f"rowscale_bwd {case.name} {dt}"
    ref = X.rowscale_bwd_ref(d["dy"], d["y"], case.act, d["bias"], d["scale"], case.rows)
    units("rowscale_gs", b["gs"][:M, :C], ref["gs"], ref["gs"], tdt, what + ": gs")
    check_guard(b["gs"], M, C, Cpad, what + ": gs")                      # columns C .. Cpad zero, the rest of the pitch and the guard rows untouched
    units("rowscale_dots", b["dots"][:groups], ref["dots"], ref["dots_mag"], F32, what + ": dots")
    tail_ok(b["dots"], groups, what + ": dots")
    if case.dbias:
        units("rowscale_dbias", b["dbias"][:C], ref["dbias"], ref["dbias_mag"], F32, what + ": dbias")
        tail_ok(b["dbias"], C, what + ": dbias")
    tail_ok(b["ws"], nws, what + ": workspace")
    for k in keep:
        unchanged(b[k], keep[k], f"{what}: {k}")


# ------------------------------------------------------------------ frame sum
def sum_frames_run(frames, n, tdt, code, values):
    src, dst = flat(frames * n, values, tdt), flat(n, None, tdt)
    before = src.clone()
    run(lib().ipoke_sum_frames(ptr(src), ptr(dst), frames, n, code, stream()))
    unchanged(src, before, "sum_frames src")
    tail_ok(dst, n, "sum_frames")
    return dst[:n]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("frames", X.SUM_FRAMES)
def test_sum_frames(frames, dt):
    code, tdt, _ = DTYPES[dt]
    vi = X.sum_operands(frames, X.SUM_N, tdt, True)
    assert_same(sum_frames_run(frames, X.SUM_N, tdt, code, vi), X.sum_frames_ref(vi), f"sum_frames integers, {frames} frames {dt}")
    vr = X.sum_operands(frames, X.SUM_N, tdt, False)
    got, ref = sum_frames_run(frames, X.SUM_N, tdt, code, vr).cpu(), X.sum_frames_ref(vr)
    print(f"measured sum_frames: {X.err_units(got, ref, ref, tdt):.3f} of 1 units ({frames} frames {dt})")
    assert_close_ulp(got, ref, 1, tdt, f"sum_frames reals, {frames} frames {dt}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sum_frames_grid_stride_wrap(dt):
    code, tdt, e16 = DTYPES[dt]
    n = X.SUM_WRAP_VECS * e16
    v = torch.randint(-8, 9, (2, n), generator=torch.Generator().manual_seed(3), dtype=torch.int8).to(DEV)
    assert_same(sum_frames_run(2, n, tdt, code, v), (v[0].to(torch.int32) + v[1].to(torch.int32)).to(tdt), f"sum_frames wrap {dt}")


# ------------------------------------------------------------------ Adam
def test_adam_multi_updates_p_m_and_v():
    sizes, h = X.adam_sizes(), X.adam_hyper()
    count, total = len(sizes), sum(sizes)
    offs, o = [], X.ADAM_GAP
    for n in sizes:
        offs.append(o)
        o += n + X.ADAM_GAP
    idx = torch.cat([torch.arange(a, a + n) for a, n in zip(offs, sizes)]).to(DEV)
    gap = torch.ones(o + TAIL, dtype=torch.bool, device=DEV)
    gap[idx] = False
    p0, gs = X.adam_operands()
    arena = {k: flat(o) for k in "pgmv"}
    arena["p"][idx] = p0.to(F32).to(DEV)
    arena["m"][idx] = 0.0
    arena["v"][idx] = 0.0
    arrays = {k: (ctypes.c_void_p * count)(*[arena[k].data_ptr() + 4 * a for a in offs]) for k in "pgmv"}
    ns = (ctypes.c_int64 * count)(*sizes)
    f = {k: float(x) for k, x in h.items()}
    for step, g in zip(X.ADAM_STEPS, gs):
        arena["g"][idx] = g.to(F32).to(DEV)
        prev = {k: host(arena[k][idx]) for k in "pmv"}                  # the kernel's own previous state
        run(lib().ipoke_adam_multi(arrays["p"], arrays["g"], arrays["m"], arrays["v"], ns, count, f["lr"], f["beta1"], f["beta2"], f["eps"],
                                   f["weight_decay"], step, f["grad_scale"], stream()))
        ref = X.adam_ref(prev["p"], g, prev["m"], prev["v"], step, **h)
        for k in "mvp":
            units("adam_" + k, arena[k][idx], ref[k], ref[k + "_mag"], F32, f"adam step {step}: {k}")
        for k in "pgmv":
            assert bool((arena[k][gap] == SENT).all()), f"adam step {step}: write between or behind the tensors of {k}"
        assert_same(arena["g"][idx], g, f"adam step {step}: the gradient")


# ------------------------------------------------------------------ KL
def kl_run(case, mu, lv):
    n = case.positions * case.Z
    b = dict(mu=flat(n, mu), lv=flat(n, lv), loss=flat(1, torch.tensor([X.KL_LOSS0])), dmu=flat(n), dlv=flat(n))
    keep = {k: b[k].clone() for k in ("mu", "lv")}
    run(lib().ipoke_kl_loss(ptr(b["mu"]), ptr(b["lv"]), case.positions, case.Z, ptr(b["loss"]), ptr(b["dmu"]), ptr(b["dlv"]), stream()))
    for k in keep:
        unchanged(b[k], keep[k], f"kl_loss {k}")
    for k, m in (("loss", 1), ("dmu", n), ("dlv", n)):
        tail_ok(b[k], m, f"kl_loss {case.name}: {k}")
    return b


@pytest.mark.parametrize("case", X.KL_CASES, ids=lambda c: c.name)
def test_kl_loss(case):
    n = case.positions * case.Z
    mu, lv = X.kl_operands(case)
    b = kl_run(case, mu, lv)
    ref = X.kl_ref(mu, lv, case.positions, torch.tensor(X.KL_LOSS0, dtype=F64))
    what = f"kl_loss {case.name}"
    units("kl_value", b["loss"][:1], ref["loss"].reshape(1), ref["loss_mag"].reshape(1), F32, what + ": value (accumulated)")
    units("kl_dmu", b["dmu"][:n], ref["dmu"], ref["dmu"], F32, what + ": dmu")
    units("kl_dlv", b["dlv"][:n], ref["dlv"], ref["dlv_mag"], F32, what + ": dlv")
    if n <= 1 << 20:                                            # one workgroup: a deterministic value
        again = kl_run(case, mu, lv)
        for k in ("loss", "dmu", "dlv"):
            assert_same(again[k], b[k], f"{what}: two runs, {k}")
