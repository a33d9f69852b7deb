"""The masked-convolution flow kernels phase by phase (tests/mcf_exact.py has the references, the operands, the checkers and the
bounds; tests/test_mcf_kernels_cpu.py pins them): the per-layer calls ipoke_mcf_fwd / _bwd / _inv in f32 and bf16 (the bf16 general
path at 4C + Cc > 384 and the 32- and 64-row forward tilings included), the fused unit ipoke_macow_unit_fwd / _bwd / _inv with and
without the row split, two units per launch, the log-det slot layout and the host-side argument checks.  Exact family: every stored
tensor bit for bit against the float64 chain.  Inexact family: every phase of every layer on the inputs the kernel itself stored."""
import functools

import pytest
import torch

from ipoke_amd import _lib
from tests import mcf_exact as X
from tests.flow_exact import GUARD, SENT, assert_same, check_guard, guarded
from tests.mcf_exact import BF16, F32, F64, LAYER_CASES, TDT, UNIT2_CASES, UNIT_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = lambda cs: [c.id for c in cs]                                                            # noqa: E731
FAMILIES = ["exact", "inexact"]


def lib():
    return _lib.lib()


def stream():
    return _lib.current_stream()


def flat_guarded(n, values=None):
    """fp32 [n + GUARD] of SENT"""
    buf = torch.full((n + GUARD,), SENT, dtype=F32, device=DEV)
    if values is not None:
        buf[:n] = values.to(F32)
    return buf


def canon(t):
    """zeros of either sign alike"""
    return t + 0.0


def same(got, ref64, what):
    assert_same(canon(got.cpu()).contiguous(), canon(ref64).contiguous(), what)


def summary(tally, what):
    print(f"{what}: " + ", ".join(f"{k} {v:.2f}/{X.gpu_bound(k, tally.dt, tally.fast):g}" for k, v in sorted(tally.worst.items())))


@functools.lru_cache(maxsize=None)
def layer_reference(c, exact):
    layers, x, cond, dy, dld = X.layer_operands(c, exact)
    return layers, x, cond, dy, dld, X.chain(layers, x, cond, dy=dy, dld=dld)


@functools.lru_cache(maxsize=None)
def unit_reference(c, exact):
    layers, x, cond, dy, dld = X.unit_operands(c, exact)
    return layers, x, cond, dy, dld, X.chain(layers, x, cond, dy=dy, dld=dld)


def set_layer(d, sh, c, cond, order):
    d.ld, d.C, d.B = c.ld, c.C, c.B
    d.cond, d.Cc = cond.data_ptr(), c.Cc
    d.W1, d.W2, d.bias2 = sh["W1"].data_ptr(), sh["W2"].data_ptr(), sh["bias"].data_ptr()
    d.W1T, d.W2T = sh["W1T"].data_ptr(), sh["W2T"].data_ptr()
    d.order = order
    if "ls" in sh:
        d.post_log_scale, d.post_bias = sh["ls"].data_ptr(), sh["pb"].data_ptr()


# ------------------------------------------------------------------ 1. the per-layer calls
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("c", LAYER_CASES, ids=IDS(LAYER_CASES))
def test_layer_calls(c, family):
    """ipoke_mcf_fwd, _bwd and _inv of one layer.  Outputs in guarded buffers; the padding columns of a2_save, dparams_save and dc_save
    zero; the log-det slots [B][64 / rows per workgroup] and nothing behind them; the pass-through columns bit for bit."""
    exact = family == "exact"
    layers, x, cond, dy, dld, ref = layer_reference(c, exact)
    L, tdt, C, ld, B, M, H = layers[0], TDT[c.dt], c.C, c.ld, c.B, c.B * 64, 4 * c.C
    sh = X.shadows(L, C, c.Cc, c.dt, DEV)
    dm = sh["dims"]
    w = c.slot_w
    xs = guarded(M, ld, F32, DEV, x)
    condT = cond.to(tdt).to(DEV).contiguous()
    y, a2, sc = guarded(M, ld, F32, DEV), guarded(M, dm["K2p"], tdt, DEV), guarded(M, C, F32, DEV)
    slots = flat_guarded(B * 4)
    d = _lib.McfDesc()
    set_layer(d, sh, c, condT, L.order)
    d.x, d.y, d.rows_per_block = xs.data_ptr(), y.data_ptr(), c.rpb
    d.a2_save, d.scale_save, d.logdet_slot = a2.data_ptr(), sc.data_ptr(), slots.data_ptr()
    _lib.check(lib().ipoke_mcf_fwd(d, _lib.DTYPES[c.dt], stream()))
    # ---- backward on the saves of that call
    dyb, dx = guarded(M, ld, F32, DEV, dy), guarded(M, ld, F32, DEV)
    dldb = dld.to(F32).to(DEV)
    dp, dc = guarded(M, dm["K3p"], tdt, DEV), guarded(M, dm["Hq"], tdt, DEV)
    dbp, pp = guarded(B, 2 * C, F32, DEV), guarded(B, 2 * C, F32, DEV)
    b = _lib.McfDesc()
    set_layer(b, sh, c, condT, L.order)
    b.x, b.dy, b.dx, b.dld = xs.data_ptr(), dyb.data_ptr(), dx.data_ptr(), dldb.data_ptr()
    b.a2_save, b.scale_save = a2.data_ptr(), sc.data_ptr()
    b.dparams_save, b.dc_save, b.dbias_part = dp.data_ptr(), dc.data_ptr(), dbp.data_ptr()
    if c.post:
        b.y_post, b.post_part = y.data_ptr(), pp.data_ptr()
    _lib.check(lib().ipoke_mcf_bwd(b, _lib.DTYPES[c.dt], stream()))
    # ---- inverse of the layer without its ActNorm (the per-layer inverse has none): of the reference output
    L0 = L._replace(ls=None, pb=None)
    y0 = x.clone()
    y0[:, :C] = X.f32r(X.chain([L0], x, cond)["y"][0])
    yin, xrec = guarded(M, ld, F32, DEV, y0), guarded(M, ld, F32, DEV)
    i = _lib.McfDesc()
    set_layer(i, sh, c, condT, L.order)
    i.post_log_scale = i.post_bias = None
    i.x, i.y = yin.data_ptr(), xrec.data_ptr()
    _lib.check(lib().ipoke_mcf_inv(i, _lib.DTYPES[c.dt], stream()))
    torch.cuda.synchronize()
    y, a2, sc, slots, dx, dp, dc, dbp, pp, xrec = (t.cpu() for t in (y, a2, sc, slots, dx, dp, dc, dbp, pp, xrec))
    for buf, cols, what in ((y, ld, "y"), (a2, dm["K2p"], "a2_save"), (sc, C, "scale_save"), (dx, ld, "dx"), (dp, dm["K3p"], "dparams_save"),
                            (dc, dm["Hq"], "dc_save"), (dbp, 2 * C, "dbias_part"), (xrec, ld, "x_rec")):
        check_guard(buf, M if buf is not dbp else B, cols, what=what)
    assert bool((slots[B * w:] == SENT).all()) and bool((slots[:B * w] != SENT).all()), "log-det slots: [B][64 / rows per workgroup]"
    check_guard(pp, B if c.post else 0, 2 * C, what="post_part")
    same(y[:M, C:], x[:, C:], "pass-through columns of y")
    same(dx[:M, C:], dy[:, C:], "pass-through columns of dx")
    same(xrec[:M, C:], y0[:, C:], "pass-through columns of the inverse")
    ws = {"x": [x[:, :C]], "y": [y[:M, :C]], "a2": [a2[:M]], "scale": [sc[:M]], "slots": [slots[:B * w].view(B, w)],
          "dp": [dp[:M]], "dc": [dc[:M]], "dbias": [dbp[:B]], "post_part": [pp[:B]], "dx": dx[:M, :C]}
    tally = X.Tally(c.dt, False)
    X.check_forward(layers, cond, ws, tally, w)
    X.check_backward(layers, ws, dy[:, :C], dld, tally)
    if exact:
        same(ws["y"][0], ref["y"][0], "y")
        same(ws["a2"][0][:, :H], ref["a2"][0][:, :H], "a2_save")
        same(ws["scale"][0], ref["scale"][0], "scale_save")
        assert bool((ws["slots"][0] == 0).all()), "log-det"
        same(ws["dp"][0][:, :2 * C], ref["dp"][0], "dparams_save")
        same(ws["dc"][0][:, :H], ref["dc"][0], "dc_save")
        same(ws["dbias"][0], ref["dbias"][0], "dbias_part")
        same(ws["dx"], ref["dx"], "dx")
        if c.post:
            same(ws["post_part"][0], ref["post_part"][0], "post_part")
        same(xrec[:M, :C], x[:, :C], "inverse")
    else:
        X.check_inverse_residual(L0, cond, y0[:, :C], xrec[:M, :C], tally)
        summary(tally, c.id)


# ------------------------------------------------------------------ 2. / 3. the fused unit, one or two per launch
def run_unit(c, exact, S, rpb=16, inverse=True, reject=False):
    """forward, backward (and inverse) of a fused launch; returns what the calls stored (CPU) and the references.  reject: the forward
    call must return non-zero with a message and launch nothing (every output buffer still holds SENT)"""
    layers, x, cond, dy, dld, ref = unit_reference(c, exact)
    nl, C, ld, B, M, H = c.nl, c.C, c.ld, c.B, c.B * 64, 4 * c.C
    fwd, bwd, inv = ((lib().ipoke_macow_unit_fwd, lib().ipoke_macow_unit_bwd, lib().ipoke_macow_unit_inv) if nl == 4 else
                     (lib().ipoke_macow_unit2_fwd, lib().ipoke_macow_unit2_bwd, lib().ipoke_macow_unit2_inv))
    shs = [X.shadows(L, C, c.Cc, "bf16", DEV) for L in layers]
    dm = shs[0]["dims"]
    w = 64 // rpb if rpb else 1
    xs = guarded(M, ld, F32, DEV, x)
    condT = cond.to(BF16).to(DEV).contiguous()
    g = lambda cols, t=F32, rows=M: [guarded(rows, cols, t, DEV) for _ in range(nl)]          # noqa: E731
    o = dict(ys=g(ld), a2=g(dm["K2p"], BF16), sc=g(C), dps=g(dm["K3p"], BF16), dcs=g(dm["Hq"], BF16), xop=g(dm["Cp"], BF16),
             dbp=g(2 * C, F32, B * S), pp=g(2 * C, F32, B * S), slots=[flat_guarded(B * w) for _ in range(nl)], dx=guarded(M, ld, F32, DEV),
             dy=guarded(M, ld, F32, DEV, dy), dld=dld.to(F32).to(DEV))
    nb = lib().ipoke_macow_unit_xchg_bytes(B, S)
    o["xchg"] = torch.zeros(max(nb, 512) // 4, dtype=torch.int32, device=DEV)
    d = (_lib.McfDesc * nl)()
    ins = [xs] + o["ys"][:-1]
    for k in range(nl):
        set_layer(d[k], shs[k], c, condT, layers[k].order)
        d[k].x, d[k].y, d[k].rows_per_block = ins[k].data_ptr(), o["ys"][k].data_ptr(), rpb
        d[k].a2_save, d[k].scale_save, d[k].logdet_slot = o["a2"][k].data_ptr(), o["sc"][k].data_ptr(), o["slots"][k].data_ptr()
        d[k].dparams_save, d[k].dc_save, d[k].dbias_part = o["dps"][k].data_ptr(), o["dcs"][k].data_ptr(), o["dbp"][k].data_ptr()
        d[k].x_op_save = o["xop"][k].data_ptr()
        if layers[k].ls is not None:
            d[k].y_post, d[k].post_part = o["ys"][k].data_ptr(), o["pp"][k].data_ptr()
    d[nl - 1].dy, d[0].dx, d[0].dld = o["dy"].data_ptr(), o["dx"].data_ptr(), o["dld"].data_ptr()
    if S > 1:
        d[0].split, d[0].xchg = S, o["xchg"].data_ptr()
    if reject:
        assert fwd(d, _lib.DTYPES["bf16"], stream()) != 0 and lib().ipoke_last_error()
        torch.cuda.synchronize()
        for key in ("ys", "a2", "sc", "slots"):
            assert all(bool((t == SENT).all()) for t in o[key]), f"rejected call wrote {key}"
        assert int(o["xchg"].abs().sum()) == 0
        return None
    # the conditioning operand of the coupling behind the unit, both ways: every other channel ("skip") and a contiguous half
    zcs = []
    for off, stride, cin in ((1, 2, C // 2), (C // 2, 1, C - C // 2)):
        zld = -(-cin // 8) * 8 + 8
        zcs.append((off, stride, cin, zld, guarded(M, zld, BF16, DEV)))
    for off, stride, cin, zld, buf in zcs:
        z = d[nl - 1]
        z.zc_out, z.zc_off, z.zc_stride, z.zc_cin, z.zc_ld = buf.data_ptr(), off, stride, cin, zld
        _lib.check(fwd(d, _lib.DTYPES["bf16"], stream()))
    d[nl - 1].zc_out = None
    _lib.check(bwd(d, _lib.DTYPES["bf16"], stream()))
    if inverse:
        y_in = x.clone()
        y_in[:, :C] = X.f32r(ref["y"][-1])
        o["y_in"] = y_in
        yin, o["xrec"] = guarded(M, ld, F32, DEV, y_in), guarded(M, ld, F32, DEV)
        iv = (_lib.McfDesc * nl)()
        for k in range(nl):
            set_layer(iv[k], shs[k], c, condT, layers[k].order)
        iv[nl - 1].x, iv[0].y = yin.data_ptr(), o["xrec"].data_ptr()
        _lib.check(inv(iv, _lib.DTYPES["bf16"], stream()))
    torch.cuda.synchronize()
    o = {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu() if torch.is_tensor(v) else v) for k, v in o.items()}
    o["zcs"] = [(off, stride, cin, zld, buf.cpu()) for off, stride, cin, zld, buf in zcs]
    assert int(o["xchg"][0]) == 0, "hand-off time-outs"
    assert int((o["xchg"][64:] != 0).sum()) == 0, "the exchange scratch must be all-zero again after a launch"
    return o, dm, w


def check_unit(c, exact, S, o, dm, w):
    layers, x, cond, dy, dld, ref = unit_reference(c, exact)
    nl, C, ld, B, M, H = c.nl, c.C, c.ld, c.B, c.B * 64, 4 * c.C
    # ---- layout: guards, padding, pass-through, slots
    for k in range(nl):
        last = k == nl - 1 or (nl == 8 and k == 3)          # the states that also receive the pass-through channels
        check_guard(o["ys"][k], M, ld if last else C, what=f"y of layer {k}")
        if last:
            same(o["ys"][k][:M, C:], x[:, C:], f"pass-through columns of y of layer {k}")
        for key, cols, rows in (("a2", dm["K2p"], M), ("sc", C, M), ("dps", dm["K3p"], M), ("dcs", dm["Hq"], M), ("xop", dm["Cp"], M),
                                ("dbp", 2 * C, B * S)):
            check_guard(o[key][k], rows, cols, what=f"{key} of layer {k}")
        check_guard(o["pp"][k], B * S if layers[k].ls is not None else 0, 2 * C, what=f"post_part of layer {k}")
        sl = o["slots"][k]
        assert bool((sl[B * w:] == SENT).all()), "write behind the log-det slots"
        sl = sl[:B * w].view(B, w)
        assert bool((sl[:, :S] != SENT).all()) and bool((sl[:, S:] == SENT).all()), f"log-det slots of layer {k}: parts [b * w + s], s < split"
        xin = x[:, :C] if k == 0 else o["ys"][k - 1][:M, :C].to(F64)
        same(o["xop"][k][:M, :C], X.rnd(xin, BF16), f"x_op_save of layer {k}")
        assert bool((o["xop"][k][:M, C:].to(F64) == 0).all()), f"padding columns of x_op_save of layer {k}"
    check_guard(o["dx"], M, ld, what="dx")
    same(o["dx"][:M, C:], dy[:, C:], "pass-through columns of dx")
    for off, stride, cin, zld, buf in o["zcs"]:
        check_guard(buf, M, zld, what="zc_out")
        same(buf[:M, :cin], X.rnd(o["ys"][nl - 1][:M, off:off + (cin - 1) * stride + 1:stride].to(F64), BF16), f"zc_out ({off}, {stride})")
        assert bool((buf[:M, cin:].to(F64) == 0).all()), "padding columns of zc_out"
    ws = {"x": [x[:, :C]] + [o["ys"][k][:M, :C] for k in range(nl - 1)], "y": [t[:M, :C] for t in o["ys"]], "a2": [t[:M] for t in o["a2"]],
          "scale": [t[:M] for t in o["sc"]], "slots": [t[:B * w].view(B, w)[:, :S] for t in o["slots"]], "dp": [t[:M] for t in o["dps"]],
          "dc": [t[:M] for t in o["dcs"]], "dbias": [t[:B * S] for t in o["dbp"]], "post_part": [t[:B * S] for t in o["pp"]],
          "dx": o["dx"][:M, :C]}
    tally = X.Tally("bf16", True)
    X.check_forward(layers, cond, ws, tally, S)
    X.check_backward(layers, ws, dy[:, :C], dld, tally, S)
    if "xrec" in o:
        check_guard(o["xrec"], M, ld, what="x_rec")
        same(o["xrec"][:M, C:], o["y_in"][:, C:], "pass-through columns of the inverse")
        assert bool(torch.isfinite(o["xrec"][:M]).all())
    if not exact:
        summary(tally, f"{c.id} split {S}")
        return
    rows = dld.repeat_interleave(64)
    for k, L in enumerate(layers):
        at = f" of layer {k}"
        same(ws["y"][k], ref["y"][k], "y" + at)
        same(ws["a2"][k][:, :H], ref["a2"][k][:, :H], "a2_save" + at)
        same(ws["scale"][k], ref["scale"][k], "scale_save" + at)
        assert bool((ws["slots"][k] == 0).all()), "log-det" + at
        same(ws["dp"][k][:, :2 * C], ref["dp"][k], "dparams_save" + at)
        same(ws["dc"][k][:, :H], ref["dc"][k], "dc_save" + at)
        gy, ds = X.dparams_ref(ref["g"][k], ref["x"][k], ref["scale"][k], rows, L.ls)[:2]
        same(ws["dbias"][k], X.dbias_ref(gy, ds, B, S)[0], "dbias_part" + at)              # integer sums: every split part bit for bit
        if L.ls is not None:
            t = ref["g"][k] * (ref["y"][k] - L.pb)
            part = torch.cat([X.per_sample(t, B, S) + (64.0 / S) * dld.repeat_interleave(S).view(-1, 1), X.per_sample(ref["g"][k], B, S)], 1)
            same(ws["post_part"][k], part, "post_part" + at)
    same(ws["dx"], ref["dx"], "dx")
    if "xrec" in o:
        same(o["xrec"][:M, :C], x[:, :C], "inverse")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("c", UNIT_CASES, ids=IDS(UNIT_CASES))
def test_unit_calls(c, S, family):
    """ipoke_macow_unit_fwd / _bwd with split 1, 2, 4 and (once per case) ipoke_macow_unit_inv"""
    exact = family == "exact"
    o, dm, w = run_unit(c, exact, S, inverse=S == 1)
    check_unit(c, exact, S, o, dm, w)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("c", UNIT2_CASES, ids=IDS(UNIT2_CASES))
def test_two_units_per_launch(c, S):
    """ipoke_macow_unit2_fwd / _bwd / _inv: the exact family over eight layers, bit for bit against the float64 chain"""
    o, dm, w = run_unit(c, True, S, inverse=S == 2)
    check_unit(c, True, S, o, dm, w)


@pytest.mark.parametrize("c", UNIT_CASES, ids=IDS(UNIT_CASES))
def test_unit_inverse_layer_by_layer(c):
    """ipoke_macow_unit_inv in the inexact family.  The launch stores nothing between its four layers, so it is run with one real layer
    (and its ActNorm) at position k and identity layers elsewhere, which it must invert bit for bit: the forward residual of layer k is
    then the whole error of the launch."""
    layers, x, cond, dy, dld, ref = unit_reference(c, False)
    C, ld, B, M = c.C, c.ld, c.B, c.B * 64
    condT = cond.to(BF16).to(DEV).contiguous()
    tally = X.Tally("bf16", True)
    for k in range(4):
        used = [layers[j] if j == k else X.identity_layer(C, c.Cc, layers[j].order) for j in range(4)]
        shs = [X.shadows(L, C, c.Cc, "bf16", DEV) for L in used]
        y_in = x.clone()
        y_in[:, :C] = X.f32r(X.chain([layers[k]], x, cond)["y"][0])
        yin, xrec = guarded(M, ld, F32, DEV, y_in), guarded(M, ld, F32, DEV)
        iv = (_lib.McfDesc * 4)()
        for j in range(4):
            set_layer(iv[j], shs[j], c, condT, used[j].order)
        iv[3].x, iv[0].y = yin.data_ptr(), xrec.data_ptr()
        _lib.check(lib().ipoke_macow_unit_inv(iv, _lib.DTYPES["bf16"], stream()))
        torch.cuda.synchronize()
        xrec = xrec.cpu()
        check_guard(xrec, M, ld, what="x_rec")
        same(xrec[:M, C:], y_in[:, C:], "pass-through columns of the inverse")
        X.check_inverse_residual(layers[k], cond, y_in[:, :C], xrec[:M, :C], tally, where=f"(layer {k})")
    summary(tally, f"{c.id} inverse")


@pytest.mark.parametrize("rpb,S,ok", [(0, 1, True), (64, 1, True), (32, 1, True), (32, 2, True), (16, 4, True), (0, 2, False), (64, 2, False),
                                      (32, 4, False)])
def test_unit_logdet_slot_layout(rpb, S, ok):
    """d4[k].logdet_slot[b * w + s] with w = 64 / rows_per_block (1 when rows_per_block == 0); a split launch needs w >= split"""
    c = UNIT_CASES[0]
    if ok:
        o, dm, w = run_unit(c, False, S, rpb=rpb, inverse=False)
        assert w == (64 // rpb if rpb else 1)
        check_unit(c, False, S, o, dm, w)
        return
    run_unit(c, False, S, rpb=rpb, inverse=False, reject=True)


# ------------------------------------------------------------------ 4. argument checks (host side: nothing is launched)
class Roomy:
    """descriptors of a small valid call whose every buffer has room for the largest shape a mutation names (a check that did not
    fire would still launch inside them) and is filled with SENT"""
    def __init__(self, dt, n=1):
        self.dt = dt
        tdt = TDT[dt]
        self.C, self.ld, self.Cc, self.B = 8, 8, 16, 2
        f = lambda: torch.full((2 * 64 + GUARD, 1024), SENT, dtype=F32, device=DEV)            # noqa: E731
        self.w = torch.zeros(1 << 20, dtype=tdt, device=DEV)
        self.bias = torch.zeros(256, dtype=F32, device=DEV)
        self.cond = torch.zeros(2 * 64, 512, dtype=tdt, device=DEV)
        self.x, self.dy, self.dld = f(), f(), torch.zeros(8, dtype=F32, device=DEV)
        self.out = [f() for _ in range(9)]
        self.d = (_lib.McfDesc * n)()
        for k in range(n):
            d = self.d[k]
            d.ld, d.C, d.B, d.Cc, d.order, d.rows_per_block = self.ld, self.C, self.B, self.Cc, k % 4, 16
            d.x, d.cond = self.x.data_ptr(), self.cond.data_ptr()
            d.W1 = d.W2 = d.W1T = d.W2T = self.w.data_ptr()
            d.bias2 = self.bias.data_ptr()
            (d.y, d.a2_save, d.scale_save, d.logdet_slot, d.dx, d.dparams_save, d.dc_save, d.dbias_part, d.post_part) = (t.data_ptr() for t in self.out)
            d.dy, d.dld, d.y_post = self.dy.data_ptr(), self.dld.data_ptr(), self.x.data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in self.out)


def _mut(name):
    def f(r):
        d = r.d[0]
        if name == "C odd":
            d.C = 7
        elif name == "C > 64":
            d.C, d.ld = 66, 68
        elif name == "order = 4":
            d.order = 4
        elif name == "ld < C":
            d.ld = 6
        elif name == "Cc not a multiple of 16 bytes":
            d.Cc = 4 if r.dt == "bf16" else 2
        elif name == "rows_per_block = 48":
            d.rows_per_block = 48
        elif name == "fused ActNorm with C % 4 != 0":
            d.C, d.post_log_scale, d.post_bias = 6, r.bias.data_ptr(), r.bias.data_ptr()
        elif name == "fused ActNorm with log_scale only":
            d.post_log_scale = r.bias.data_ptr()
        elif name == "fused ActNorm with bias only":
            d.post_bias = r.bias.data_ptr()
        elif name == "backward without a2_save":
            d.a2_save = None
    return f


def test_the_calls_the_rejections_start_from_are_accepted():
    """the unmutated descriptors pass every argument check (zero weights: each call is the identity on its rows)"""
    for dt in ("bf16", "f32"):
        for fn in (lib().ipoke_mcf_fwd, lib().ipoke_mcf_bwd, lib().ipoke_mcf_inv):
            _lib.check(fn(Roomy(dt).d[0], _lib.DTYPES[dt], stream()))
    for nl, fns in ((4, (lib().ipoke_macow_unit_fwd, lib().ipoke_macow_unit_bwd, lib().ipoke_macow_unit_inv)),
                    (8, (lib().ipoke_macow_unit2_fwd, lib().ipoke_macow_unit2_bwd, lib().ipoke_macow_unit2_inv))):
        for fn in fns:
            r = Roomy("bf16", nl)
            xchg = torch.zeros(lib().ipoke_macow_unit_xchg_bytes(r.B, 2) // 4, dtype=torch.int32, device=DEV)
            r.d[0].split, r.d[0].xchg = 2, xchg.data_ptr()
            _lib.check(fn(r.d, _lib.DTYPES["bf16"], stream()))
            torch.cuda.synchronize()
            assert int(xchg.abs().sum()) == 0


LAYER_REJECTS = [("C odd", "fwd bwd inv"), ("C > 64", "fwd bwd inv"), ("order = 4", "fwd bwd inv"), ("ld < C", "fwd bwd inv"),
                 ("Cc not a multiple of 16 bytes", "fwd bwd inv"), ("rows_per_block = 48", "fwd"), ("fused ActNorm with C % 4 != 0", "fwd bwd"),
                 ("fused ActNorm with log_scale only", "fwd bwd"), ("fused ActNorm with bias only", "fwd bwd"), ("backward without a2_save", "bwd")]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("name,calls", LAYER_REJECTS, ids=[n for n, _ in LAYER_REJECTS])
def test_layer_calls_reject(name, calls, dt):
    fns = {"fwd": lib().ipoke_mcf_fwd, "bwd": lib().ipoke_mcf_bwd, "inv": lib().ipoke_mcf_inv}
    for call in calls.split():
        r = Roomy(dt)
        _mut(name)(r)
        assert fns[call](r.d[0], _lib.DTYPES[dt], stream()) != 0, f"{call}: {name}"
        assert lib().ipoke_last_error(), call
        assert r.untouched(), f"{call}: something was launched"


def test_unit_calls_reject_wide_conditioning():
    """Cc > 128 (f32 is refused in test_unit_double_gpu.py)"""
    for nl, fns in ((4, (lib().ipoke_macow_unit_fwd, lib().ipoke_macow_unit_bwd, lib().ipoke_macow_unit_inv)),
                    (8, (lib().ipoke_macow_unit2_fwd, lib().ipoke_macow_unit2_bwd, lib().ipoke_macow_unit2_inv))):
        for fn in fns:
            r = Roomy("bf16", nl)
            xchg = torch.zeros(lib().ipoke_macow_unit_xchg_bytes(r.B, 2) // 4, dtype=torch.int32, device=DEV)
            r.d[0].split, r.d[0].xchg = 2, xchg.data_ptr()
            for k in range(nl):
                r.d[k].Cc = 136
            assert fn(r.d, _lib.DTYPES[r.dt], stream()) != 0 and lib().ipoke_last_error()
            assert r.untouched(), "something was launched"
            assert int(xchg.abs().sum()) == 0
