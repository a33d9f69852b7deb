"""The flow's state kernels one by one against the float64 references of tests/flow_exact.py: layout changes, ActNorm (+ shuffle),
the affine coupling transform, the fused pair, log-det bookkeeping, the loss and the LU 1x1 convolution.  The exact operand set is
compared bit for bit, the inexact one within the bounds of flow_exact.gpu_bound; every buffer is guarded by sentinels."""
import ctypes

import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd._lib import ptr
from tests import flow_exact as X
from tests.flow_exact import DTYPES, F64, SENT, assert_same, assert_units, check_guard, guarded, gpu_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
EXACT = pytest.mark.parametrize("exact", [True, False], ids=["exact", "inexact"])


def lib():
    return _lib.lib()


def run(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def stream():
    return _lib.current_stream()


def dev(t, dtype=F32):
    return None if t is None else t.to(dtype).to(DEV)


def state(v):
    """a [M][ld] state in a guarded buffer: the kernels' ld is both pitch and width, so the guard is the rows behind it"""
    return guarded(v.shape[0], v.shape[1], F32, DEV, v.to(DEV))


def flat(n, values=None, dtype=F32, tail=64):
    """n elements (SENT, or `values`) followed by `tail` elements of SENT"""
    b = torch.full((n + tail,), SENT, dtype=dtype, device=DEV)
    if values is not None:
        b[:n] = values.reshape(-1).to(dtype).to(DEV)
    return b


def tail_ok(b, n, what):
    assert bool((b[n:].to(F64) == SENT).all()), what + ": write behind the buffer"


def rows(b, M):
    return b[:M].to(F64).cpu()


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("P", [64, 48])
@pytest.mark.parametrize("C", [1, 5, 64])
def test_nchw_to_state_and_back(C, P):
    B, ld = 3, C + 3
    x = X.randint64(-9, 9, (B, C, P), torch.Generator().manual_seed(C + P))
    xb, sb = flat(B * C * P, x), guarded(B * P, ld, F32, DEV)
    run(lib().ipoke_nchw_to_state(ptr(xb), ptr(sb), B, C, P, ld, stream()))
    assert_same(sb[: B * P, :C].contiguous(), X.nchw_to_state_ref(x), "nchw_to_state", lambda i: f"row {i // C} channel {i % C}")
    check_guard(sb, B * P, C, None, "nchw_to_state")           # the padding columns of the state still hold SENT
    ob = flat(B * C * P)
    run(lib().ipoke_state_to_nchw(ptr(sb), ptr(ob), B, C, P, ld, stream()))
    assert_same(ob[: B * C * P], x.reshape(-1), "state_to_nchw")
    tail_ok(ob, B * C * P, "state_to_nchw")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("off,stride", [(0, 1), (3, 1), (1, 2)])
@pytest.mark.parametrize("C", [1, 5, 64])
def test_extract_cols(C, off, stride, dt):
    code, tdt, e16 = DTYPES[dt]
    M, ld, ldo = 70, off + (C - 1) * stride + 3, X.round_up(C, e16) + e16
    s = X.int_state(M, ld, C + off, lim=9)
    sb, ob = state(s), guarded(M, ldo, tdt, DEV)
    run(lib().ipoke_extract_cols(ptr(sb), ld, off, stride, C, ptr(ob), ldo, M, code, stream()))
    what = f"extract_cols C={C} off={off} stride={stride} {dt}"
    assert_same(ob[:M, :C].contiguous(), X.extract_cols_ref(s, off, stride, C), what)
    assert bool((ob[:M, C:] == 0).all()) and bool((ob[M:].to(F64) == SENT).all()), what + ": padding / guard rows"


ACTS = {"none": _lib.ACT_NONE, "elu": _lib.ACT_ELU, "relu": _lib.ACT_RELU, "lrelu": _lib.ACT_LRELU02, "tanh": _lib.ACT_TANH,
        "sigmoid": _lib.ACT_SIGMOID}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("P", [64, 48])
def test_cond_prepare(P, act, dt):
    code, tdt, _ = DTYPES[dt]
    B, Cc = 2, 5
    h = X.randint64(-4, 4, (B, Cc, P), torch.Generator().manual_seed(P))
    hb, ob = flat(B * Cc * P, h), guarded(B * P, Cc, tdt, DEV)
    run(lib().ipoke_cond_prepare(ptr(hb), ptr(ob), B, Cc, P, ACTS[act], code, stream()))
    ref, what = X.cond_prepare_ref(h, ACTS[act]), f"cond_prepare {act} P={P} {dt}"
    if ACTS[act] in (_lib.ACT_NONE, _lib.ACT_RELU):
        assert_same(ob[: B * P].contiguous(), ref, what)
    else:
        X.assert_close_ulp(ob[: B * P].cpu(), ref, 1 if tdt == torch.bfloat16 else 2, tdt, what)
    assert bool((ob[B * P:].to(F64) == SENT).all()), what


# ------------------------------------------------------------------ ActNorm forward / inverse
def actnorm_setup(c, with_idx, with_params, exact):
    x = X.int_state(X.ACTNORM_M, c.ld, c.C) if exact else X.real_state(X.ACTNORM_M, c.ld, c.C)
    ls, b, p, ip = X.actnorm_params(c.C, exact, c.C)
    if not with_params:
        ls = b = None
    if not with_idx:
        p = ip = None
    return x, ls, b, p, ip


def win(t, c):
    return t[:, c.c0: c.c0 + c.C]


def check_window(got, ref, mag, c, exact, key, what):
    """the whole state bit-exact for the exact set; else the pass-through columns bit-exact and the window within the bound"""
    if exact:
        assert_same(got.to(F32), ref, what, lambda i: f"row {i // c.ld} column {i % c.ld}")
        return
    keep = torch.ones(c.ld, dtype=torch.bool)
    keep[c.c0: c.c0 + c.C] = False
    assert_same(got[:, keep].to(F32), ref[:, keep], what + " pass-through columns")
    assert_units(win(got, c), win(ref, c), mag, gpu_bound(key), F32, what)


@EXACT
@pytest.mark.parametrize("with_params", [True, False], ids=["params", "bare"])
@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "noidx"])
@pytest.mark.parametrize("c", X.ACTNORM_CASES, ids=lambda c: f"C{c.C}-c{c.c0}-ld{c.ld}")
def test_actnorm_forward_and_inverse(c, with_idx, with_params, exact):
    M = X.ACTNORM_M
    x, ls, b, p, ip = actnorm_setup(c, with_idx, with_params, exact)
    xb, yb, zb = state(x), guarded(M, c.ld, F32, DEV), guarded(M, c.ld, F32, DEV)
    lsd, bd, pd, ipd = dev(ls), dev(b), dev(p, torch.int32), dev(ip, torch.int32)
    run(lib().ipoke_actnorm_fwd(ptr(xb), ptr(yb), M, c.ld, c.c0, c.C, ptr(lsd), ptr(bd), ptr(pd), stream()))
    ref, mag = X.actnorm_fwd_ref(x, c.c0, c.C, ls, b, p)
    what = f"actnorm_fwd {c} idx={with_idx} params={with_params}"
    check_window(rows(yb, M), ref, mag, c, exact or not with_params, "actnorm_fwd", what)
    check_guard(yb, M, c.ld, None, what)
    # the inverse on the reference's output (rounded to fp32): for the exact set that is the kernel's own output, and x comes back
    y = X.f32r(ref)
    if exact:
        assert_same(yb[:M].contiguous(), y, what)
    yin = state(y)
    run(lib().ipoke_actnorm_inv(ptr(yin), ptr(zb), M, c.ld, c.c0, c.C, ptr(lsd), ptr(bd), ptr(ipd), stream()))
    ref, mag = X.actnorm_inv_ref(y, c.c0, c.C, ls, b, ip)
    what = what.replace("fwd", "inv")
    check_window(rows(zb, M), ref, mag, c, exact or not with_params, "actnorm_inv", what)
    check_guard(zb, M, c.ld, None, what)
    if exact or not with_params:
        assert_same(zb[:M].contiguous(), x, what + ": inv(fwd(x)) != x")


def ext_cases():
    """every ActNorm case x both column selections x f32 / bf16 x ext_ld padded to 16 bytes and one wider; the bf16 combinations of the
    one-channel case run on flow_exact.ACTNORM_EXT_BF16_C1 (see there)"""
    out = []
    for case in X.ACTNORM_CASES:
        for dt in ("f32", "bf16"):
            c = X.ACTNORM_EXT_BF16_C1 if (case.C, dt) == (1, "bf16") else case
            for v, (e_off, e_stride, e_C) in enumerate(X.ext_variants(c)):
                for wider in (0, 1):
                    ext_ld = X.round_up(e_C, DTYPES[dt][2]) + wider
                    assert ext_ld - e_C <= c.ld                # the entry point's contract: padding no wider than the state
                    out.append(pytest.param(c, e_off, e_stride, e_C, ext_ld, dt, id=f"C{c.C}-v{v}-{dt}-ld{ext_ld}"))
    return out


@EXACT
@pytest.mark.parametrize("c,e_off,e_stride,e_C,ext_ld,dt", ext_cases())
def test_actnorm_inverse_with_conditioning_operand(c, e_off, e_stride, e_C, ext_ld, dt, exact):
    code, tdt, _ = DTYPES[dt]
    M = X.ACTNORM_M
    x, ls, b, p, ip = actnorm_setup(c, True, True, exact)
    y = X.f32r(X.actnorm_fwd_ref(x, c.c0, c.C, ls, b, p)[0])
    yin, zb, eb = state(y), guarded(M, c.ld, F32, DEV), guarded(M, ext_ld, tdt, DEV)
    lsd, bd, ipd = dev(ls), dev(b), dev(ip, torch.int32)       # held in names: a temporary's memory is reused by the next allocation
    run(lib().ipoke_actnorm_inv_ext(ptr(yin), ptr(zb), M, c.ld, c.c0, c.C, ptr(lsd), ptr(bd), ptr(ipd), ptr(eb), ext_ld, e_off, e_stride, e_C,
                                    code, stream()))
    ref, mag = X.actnorm_inv_ref(y, c.c0, c.C, ls, b, ip)
    what = f"actnorm_inv_ext {c} e=({e_off},{e_stride},{e_C}) ext_ld={ext_ld} {dt}"
    check_window(rows(zb, M), ref, mag, c, exact, "actnorm_inv", what)
    check_guard(zb, M, c.ld, None, what)
    check_guard(eb, M, e_C, ext_ld, what + " ext")
    eref = X.extract_cols_ref(ref, e_off, e_stride, e_C)
    if exact:
        assert_same(eb[:M, :e_C].contiguous(), eref, what + " ext")
    else:
        mfull = ref.abs()
        mfull[:, c.c0: c.c0 + c.C] = mag
        emag = X.extract_cols_ref(mfull, e_off, e_stride, e_C)
        src = e_off + torch.arange(e_C) * e_stride             # the state column behind each ext column
        inwin = (src >= c.c0) & (src < c.c0 + c.C)
        key = "actnorm_inv_ext_bf16" if tdt == torch.bfloat16 else "actnorm_inv"
        got = eb[:M, :e_C].cpu()
        assert_units(got[:, inwin], eref[:, inwin], emag[:, inwin], gpu_bound(key), tdt, what + " ext, window columns")
        assert_same(got[:, ~inwin].contiguous(), eref[:, ~inwin], what + " ext, pass-through columns")     # copies: the rounding alone


# ------------------------------------------------------------------ ActNorm backward and init
@EXACT
@pytest.mark.parametrize("c", X.ACTNORM_BWD_CASES, ids=lambda c: c.name)
def test_actnorm_backward(c, exact):
    M = c.B * c.P
    o = X.actnorm_bwd_operands(c, exact)
    dyb, dxb = state(o["dy"]), guarded(M, c.ld, F32, DEV)
    part = flat(c.B * 2 * c.C)
    xb, dld = (state(o["x"]), dev(o["dld"])) if c.params else (None, None)
    lsd, idxd = dev(o["ls"]), dev(o["idx"], torch.int32)
    run(lib().ipoke_actnorm_bwd(ptr(dyb), ptr(xb), ptr(dxb), M, c.ld, c.c0, c.C, ptr(lsd), ptr(idxd), ptr(dld), c.B, c.P, ptr(part), stream()))
    dx, pref, pmag = X.actnorm_bwd_ref(o["dy"], o["x"], c.c0, c.C, o["ls"], o["idx"], o["dld"], c.B, c.P)
    what = f"actnorm_bwd {c.name}"
    check_window(rows(dxb, M), dx, win(dx, c).abs(), c, exact or not c.params, "actnorm_bwd_dx", what + " dx")
    check_guard(dxb, M, c.ld, None, what)
    if not c.params:
        # log_scale == NULL: the partial-sum buffer it was handed keeps SENT; and x, dld and part may all be NULL
        assert bool((part == SENT).all()), what + ": part written without parameters"
        dxb = guarded(M, c.ld, F32, DEV)
        run(lib().ipoke_actnorm_bwd(ptr(dyb), None, ptr(dxb), M, c.ld, c.c0, c.C, None, ptr(idxd), None, c.B, c.P, None, stream()))
        check_window(rows(dxb, M), dx, win(dx, c).abs(), c, True, "actnorm_bwd_dx", what + " dx, part NULL")
        check_guard(dxb, M, c.ld, None, what + " part NULL")
        return
    n = c.B * 2 * c.C
    if exact:
        assert_same(part[:n], pref, what + " part", lambda i: f"sample {i // (2 * c.C)} entry {i % (2 * c.C)} of [dls | dbias]")
    else:
        assert_units(part[:n].view(c.B, 2 * c.C), pref, pmag, gpu_bound("actnorm_bwd_part"), F32, what + " part")
    tail_ok(part, n, what)


@pytest.mark.parametrize("preinit", [False, True], ids=["zero", "nonzero"])
@pytest.mark.parametrize("M", X.INIT_MS)
def test_actnorm_init(M, preinit):
    c = X.INIT_CASE
    x, ls0, b0 = X.actnorm_init_operands(M, preinit)
    xb = state(x)
    ls, b = flat(c.C, ls0, tail=8), flat(c.C, b0, tail=8)
    run(lib().ipoke_actnorm_init(ptr(xb), M, c.ld, c.c0, c.C, ptr(ls), ptr(b), stream()))
    rls, rb = X.actnorm_init_ref(x, c.c0, c.C, ls0, b0)
    what = f"actnorm_init M={M} preinit={preinit}"
    mls, mb = X.actnorm_init_mags(x, c.c0, c.C, ls0, b0)
    assert_units(ls[: c.C], rls, mls, gpu_bound("actnorm_init"), F32, what + " log_scale")
    assert_units(b[: c.C], rb, mb, gpu_bound("actnorm_init"), F32, what + " bias")
    tail_ok(ls, c.C, what)
    tail_ok(b, c.C, what)


# ------------------------------------------------------------------ affine coupling transform
def raw_buffer(c, parts):
    """the split-K slabs as the kernel reads them: slab u at u * split_stride, rows of pitch ldraw, SENT everywhere else"""
    n, M, n2 = parts.shape
    ldraw = n2 + c.raw_pad
    ss = M * ldraw + 7
    buf = torch.full((n * ss + 64,), SENT, dtype=F64)
    for u in range(n):
        buf[u * ss: u * ss + M * ldraw].view(M, ldraw)[:, :n2] = parts[u]
    return dev(buf), ldraw, ss


def affine_desc(c, raw, ldraw, ss, bias, ld):
    d = _lib.AffineDesc()
    d.raw, d.nsplit, d.split_stride, d.ldraw = raw.data_ptr(), c.nsplit, ss, ldraw
    d.bias = None if bias is None else bias.data_ptr()
    d.Cp, d.t_off, d.t_stride, d.P, d.ld = c.Cp, c.t_off, c.t_stride, c.P, ld
    return d


def check_transformed(got, ref, mag, cols, exact, key, what):
    ld = ref.shape[1]
    if exact:
        assert_same(got.to(F32), ref, what, lambda i: f"row {i // ld} column {i % ld}")
        return
    keep = torch.ones(ld, dtype=torch.bool)
    keep[cols] = False
    assert_same(got[:, keep].to(F32), ref[:, keep], what + " untouched columns")
    assert_units(got[:, cols], ref[:, cols], mag, gpu_bound(key), F32, what)


def check_ext(eb, M, c, eref, emag, exact, ext_ld, tdt, what):
    check_guard(eb, M, c.Cp, ext_ld, what + " ext")
    if exact:
        assert_same(eb[:M, : c.Cp].contiguous(), eref, what + " ext")
    else:
        assert_units(eb[:M, : c.Cp], eref, emag, gpu_bound("affine_ext_bf16" if tdt == torch.bfloat16 else "affine_fwd"), tdt, what + " ext")


@EXACT
@pytest.mark.parametrize("c", X.AFFINE_CASES, ids=lambda c: c.name)
def test_affine_forward_and_inverse(c, exact):
    M, ld, Q = c.B * c.P, X.aff_ld(c), X.aff_q(c)
    o = X.affine_operands(c, exact)
    raw, ldraw, ss = raw_buffer(c, o["parts"])
    bias = dev(o["bias"])
    d = affine_desc(c, raw, ldraw, ss, bias, ld)
    cols = X.tcols(c.Cp, c.t_off, c.t_stride)
    code, tdt, _ = DTYPES[c.ext or "f32"]
    ext_ld = c.Cp + c.ext_pad

    def ext_buf():
        return guarded(M, ext_ld, tdt, DEV) if c.ext else None

    xb, yb, eb = state(o["x"]), guarded(M, ld, F32, DEV), ext_buf()
    sc = guarded(M, c.Cp, F32, DEV) if c.scale_out else None
    stride = c.slot or 0
    slots = flat(c.B * stride) if c.slot else None
    run(lib().ipoke_affine_fwd_ext(ctypes.byref(d), ptr(xb), ptr(yb), ptr(sc), ptr(slots), stride, c.B, ptr(eb), ext_ld, code, stream()))
    r = X.raw_sum(o["parts"], o["bias"])
    ref, rsc, rslots, mag, smag = X.affine_fwd_ref(o["x"], r, c.t_off, c.t_stride, c.B, Q)
    what = f"affine_fwd {c.name}"
    check_transformed(rows(yb, M), ref, mag, cols, exact, "affine_fwd", what)
    check_guard(yb, M, ld, None, what)
    if sc is not None:
        if exact:
            assert_same(sc[:M].contiguous(), torch.ones(M, c.Cp, dtype=F64), what + " scale_out")
        else:
            t = torch.tanh(0.5 * r[:, c.Cp:])
            assert_units(sc[:M], rsc, t.abs() + 1.0, gpu_bound("affine_scale"), F32, what + " scale_out")
        check_guard(sc, M, c.Cp, None, what + " scale_out")
    if slots is not None:
        s = slots[: c.B * stride].view(c.B, stride)
        if exact:
            assert_same(s[:, :Q].contiguous(), torch.zeros(c.B, Q, dtype=F64), what + " log-det slots")
        else:
            assert_units(s[:, :Q], rslots, smag, gpu_bound("logdet_slot"), F32, what + " log-det slots")
        assert bool((s[:, Q:] == SENT).all()), what + ": a slot beyond Q written"
        tail_ok(slots, c.B * stride, what)
    if eb is not None:
        check_ext(eb, M, c, ref[:, cols], mag, exact, ext_ld, tdt, what)
    # the inverse, on the reference's output rounded to fp32 (the exact set: the kernel's own output, and x comes back)
    y = X.f32r(ref)
    if exact:
        assert_same(yb[:M].contiguous(), y, what)
    zb, eb = guarded(M, ld, F32, DEV), ext_buf()
    yin = state(y)
    run(lib().ipoke_affine_inv_ext(ctypes.byref(d), ptr(yin), ptr(zb), c.B, ptr(eb), ext_ld, code, stream()))
    ref, mag = X.affine_inv_ref(y, r, c.t_off, c.t_stride)
    what = f"affine_inv {c.name}"
    check_transformed(rows(zb, M), ref, mag, cols, exact, "affine_inv", what)
    check_guard(zb, M, ld, None, what)
    if exact:
        assert_same(zb[:M].contiguous(), o["x"], what + ": inv(fwd(x)) != x")
    if eb is not None:
        check_ext(eb, M, c, ref[:, cols], mag, exact, ext_ld, tdt, what)


@EXACT
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", X.AFFINE_BWD_CASES, ids=lambda c: c.name)
def test_affine_backward(c, dt, exact):
    code, tdt, _ = DTYPES[dt]
    M, ld, ldp = c.B * c.P, X.affbwd_ld(c), 2 * c.Cp + c.ldp_pad
    o = X.affine_bwd_operands(c, exact)
    dyb, xb, dxb = state(o["dy"]), state(o["x"]), guarded(M, ld, F32, DEV)
    scb = guarded(M, c.Cp, F32, DEV, o["scale"].to(DEV))
    dpb = guarded(M, ldp, tdt, DEV)                            # the pitch is ldp, zero-filled from 2 Cp on
    dbias = flat(c.B * 2 * c.Cp) if c.dbias else None
    dld = dev(o["dld"])
    run(lib().ipoke_affine_bwd(c.Cp, c.t_off, c.t_stride, c.P, ld, ptr(dyb), ptr(xb), ptr(scb), ptr(dld), ptr(dxb), ptr(dpb), ldp,
                               ptr(dbias), c.B, code, stream()))
    r = X.affine_bwd_ref(o["dy"], o["x"], o["scale"], o["dld"], c.t_off, c.t_stride, c.B, c.P)
    cols = X.tcols(c.Cp, c.t_off, c.t_stride)
    what = f"affine_bwd {c.name} {dt}"
    check_transformed(rows(dxb, M), r["dx"], r["dx"][:, cols].abs(), cols, exact, "affine_bwd_dx", what + " dx")
    check_guard(dxb, M, ld, None, what)
    check_guard(dpb, M, 2 * c.Cp, ldp, what + " dparams")
    if exact:
        assert_same(dpb[:M, : 2 * c.Cp].contiguous(), r["dparams"], what + " dparams", lambda i: f"row {i // (2 * c.Cp)} column {i % (2 * c.Cp)}")
    else:
        key = "affine_bwd_dparams_bf16" if tdt == torch.bfloat16 else "affine_bwd_dparams"
        assert_units(dpb[:M, : 2 * c.Cp], r["dparams"], r["mag_dparams"], gpu_bound(key), tdt, what + " dparams")
    if dbias is not None:
        n = c.B * 2 * c.Cp
        if exact:
            assert_same(dbias[:n], r["dbias"], what + " dbias_part")
        else:
            assert_units(dbias[:n].view(c.B, 2 * c.Cp), r["dbias"], r["mag_dbias"], gpu_bound("affine_bwd_dbias"), F32, what + " dbias_part")
        tail_ok(dbias, n, what)


# ------------------------------------------------------------------ the fused pair, exact operands
PAIR = X.AffCase("pair", 4, 4, 1, 4, 5, True, 4, 64, 3, True, None, 0)
PAIR_AN = X.ActCase(8, 2, 11)                                   # the ActNorm window [2, 10) of the 11-column state covers the coupling's [4, 8)


def test_fused_coupling_actnorm_forward():
    c, a = PAIR, PAIR_AN
    M, ld, Q = c.B * c.P, X.aff_ld(c), 4
    assert ld == a.ld
    o = X.affine_operands(c, True)
    raw, ldraw, ss = raw_buffer(c, o["parts"])
    bias = dev(o["bias"])
    d = affine_desc(c, raw, ldraw, ss, bias, ld)
    ls, b, p, _ = X.actnorm_params(a.C, True, 3)
    xb, y1, y2, sc, slots = state(o["x"]), guarded(M, ld, F32, DEV), guarded(M, ld, F32, DEV), guarded(M, c.Cp, F32, DEV), flat(c.B * 4)
    lsd, bd, pd = dev(ls), dev(b), dev(p, torch.int32)
    run(lib().ipoke_affine_actnorm_fwd(ctypes.byref(d), ptr(xb), ptr(y1), ptr(y2), ptr(sc), ptr(slots), 4, c.B, a.c0, a.C, ptr(lsd), ptr(bd),
                                       ptr(pd), stream()))
    r1 = X.affine_fwd_ref(o["x"], X.raw_sum(o["parts"], o["bias"]), c.t_off, c.t_stride, c.B, Q)[0]
    r2 = X.actnorm_fwd_ref(r1, a.c0, a.C, ls, b, p)[0]
    assert_same(y1[:M].contiguous(), r1, "fused forward: the coupling's output")
    assert_same(y2[:M].contiguous(), r2, "fused forward: the ActNorm's output")
    assert_same(sc[:M].contiguous(), torch.ones(M, c.Cp, dtype=F64), "fused forward: scale_out")
    assert_same(slots[: c.B * 4], torch.zeros(c.B * 4, dtype=F64), "fused forward: log-det slots")
    for buf, w in ((y1, ld), (y2, ld), (sc, c.Cp)):
        check_guard(buf, M, w, None, "fused forward")
    tail_ok(slots, c.B * 4, "fused forward")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fused_actnorm_coupling_backward(dt):
    code, tdt, _ = DTYPES[dt]
    a = PAIR_AN
    c = X.AffBwdCase("pair", 4, 4, 1, 64, 3, 8, True)
    M, ld, ldp = c.B * c.P, a.ld, 2 * c.Cp + c.ldp_pad
    assert X.affbwd_ld(c) == ld
    o = X.affine_bwd_operands(c, True)                          # dy = the gradient at the ActNorm's output, x = the coupling's input
    gen = torch.Generator().manual_seed(77)
    x1 = X.randint64(-8, 8, (M, ld), gen)                       # the ActNorm's saved input
    ls, _, p, _ = X.actnorm_params(a.C, True, 3)
    g1, pref, _ = X.actnorm_bwd_ref(o["dy"], x1, a.c0, a.C, ls, p, o["dld"], c.B, c.P)
    r = X.affine_bwd_ref(g1, o["x"], o["scale"], o["dld"], c.t_off, c.t_stride, c.B, c.P)
    dxb, dpb = guarded(M, ld, F32, DEV), guarded(M, ldp, tdt, DEV)
    part, dbias = flat(c.B * 2 * a.C), flat(c.B * 2 * c.Cp)
    scb = guarded(M, c.Cp, F32, DEV, o["scale"].to(DEV))
    lsd, pd, dld = dev(ls), dev(p, torch.int32), dev(o["dld"])
    dyb, x1b, xb = state(o["dy"]), state(x1), state(o["x"])
    run(lib().ipoke_actnorm_affine_bwd(a.c0, a.C, ptr(lsd), ptr(pd), ptr(dyb), ptr(x1b), ptr(part), c.Cp, c.t_off, c.t_stride, c.P, ld, ptr(xb),
                                       ptr(scb), ptr(dld), ptr(dxb), ptr(dpb), ldp, ptr(dbias), c.B, code, stream()))
    what = f"fused backward {dt}"
    assert_same(dxb[:M].contiguous(), r["dx"], what + " dx")
    assert_same(dpb[:M, : 2 * c.Cp].contiguous(), r["dparams"], what + " dparams")
    assert_same(part[: c.B * 2 * a.C], pref, what + " part")
    assert_same(dbias[: c.B * 2 * c.Cp], r["dbias"], what + " dbias_part")
    check_guard(dxb, M, ld, None, what)
    check_guard(dpb, M, 2 * c.Cp, ldp, what + " dparams")
    tail_ok(part, c.B * 2 * a.C, what)
    tail_ok(dbias, c.B * 2 * c.Cp, what)


# ------------------------------------------------------------------ log-det bookkeeping
@pytest.mark.parametrize("with_dev", [True, False], ids=["const_dev", "no_const_dev"])
@pytest.mark.parametrize("nslots,slot_w,B", X.FINALIZE_CASES)
def test_logdet_finalize(nslots, slot_w, B, with_dev):
    s = X.randint64(-3, 3, (nslots, B, slot_w), torch.Generator().manual_seed(nslots))
    sb, out = flat(nslots * B * slot_w, s), flat(B, tail=8)
    cd = torch.tensor([7.0], device=DEV) if with_dev else None
    run(lib().ipoke_logdet_finalize(ptr(sb) if nslots else None, nslots, B, slot_w, 2.5, ptr(cd), ptr(out), stream()))
    assert_same(out[:B], X.logdet_finalize_ref(s, 2.5, 7.0 if with_dev else None), f"logdet_finalize {nslots} x {B} x {slot_w}",
                lambda i: f"sample {i}")
    tail_ok(out, B, "logdet_finalize")


@pytest.mark.parametrize("n", X.LOGDET_NS)
def test_actnorm_logdet(n):
    params, refs = X.actnorm_logdet_operands(n)
    table = X.table_to_device([X.LsRef(o, c, 0) for o, c in refs], DEV)
    out = flat(1, tail=8)
    pb = dev(params)
    run(lib().ipoke_actnorm_logdet(ptr(pb), ptr(table), n, 64, ptr(out), stream()))
    assert_same(out[:1], torch.tensor([X.actnorm_logdet_ref(params, refs, 64)], dtype=F64), f"actnorm_logdet n={n}")
    tail_ok(out, 1, "actnorm_logdet")


# ------------------------------------------------------------------ the loss
@pytest.mark.parametrize("grads", [True, False], ids=["grads", "nograds"])
@pytest.mark.parametrize("w", [1.0, 0.25])
@pytest.mark.parametrize("B,P,C,ld,shift", [c + (0,) for c in X.NLL_CASES] + [c + (1,) for c in X.NLL_SHIFTED])
def test_flow_nll(B, P, C, ld, shift, w, grads):
    """shift = 1: a vector-eligible case with its base address one float off a 16-byte boundary (the element-wise path, once with C < ld)"""
    z, logdet = X.nll_operands(B, P, C)
    M = B * P
    zfull = torch.full((M, ld), SENT, dtype=F64)
    zfull[:, :C] = z
    zb = flat(M * ld + shift, None)
    zb[shift: shift + M * ld] = dev(zfull).reshape(-1)
    zarg = zb[shift:]
    assert zb.data_ptr() % 16 == 0 and zarg.data_ptr() % 16 == 4 * shift
    dout, dld, sc = flat(M * ld), flat(B, tail=8), flat(3, tail=8)
    ldb = dev(logdet)
    run(lib().ipoke_flow_nll(ptr(zarg), ptr(ldb), B, P, C, ld, w, ptr(sc), ptr(dout) if grads else None, ptr(dld) if grads else None,
                             stream()))
    rs, rd, rdld = X.flow_nll_ref(z, logdet, w, B)
    what = f"flow_nll B={B} P={P} C={C} ld={ld} shift={shift} w={w}"
    pow2 = B & (B - 1) == 0
    mag = torch.stack([rs[1].abs() + abs(w) * rs[2].abs(), rs[1].abs(), rs[2].abs()])
    if pow2:
        assert_same(sc[:3], rs, what + " scalars", lambda i: ("loss", "nll", "nlogdet")[i])
    else:
        assert_units(sc[:3], rs, mag, gpu_bound("nll_scalars"), F32, what + " scalars")
    tail_ok(sc, 3, what)
    if not grads:
        assert bool((dout == SENT).all()) and bool((dld == SENT).all()), what + ": gradients written without buffers"
        return
    d = dout[: M * ld].view(M, ld)
    assert bool((d[:, C:] == 0).all()), what + ": padding columns of d_out are not zero"
    if pow2:
        assert_same(d[:, :C].contiguous(), rd, what + " d_out")
        assert_same(dld[:B], rdld, what + " dld")
    else:
        assert_units(d[:, :C], rd, rd, gpu_bound("nll_dout"), F32, what + " d_out")
        assert_units(dld[:B], rdld, rdld, gpu_bound("nll_dout"), F32, what + " dld")
    tail_ok(dout, M * ld, what)
    tail_ok(dld, B, what)


# ------------------------------------------------------------------ LU 1x1 convolution
@EXACT
def test_lu_prepare(exact):
    lay = X.LuLayout(X.LU_CS)
    assert ctypes.sizeof(X.LuJob) == lib().ipoke_lu_job_size()
    mats = [X.lu_operands(C, exact) for C in X.LU_CS]
    params, fbuf = lay.fill(mats)
    ws = flat(lay.n_ws, tail=0)
    pb, fb, jobs = dev(params), dev(fbuf), X.table_to_device(lay.jobs, DEV)
    run(lib().ipoke_lu_prepare(ptr(pb), ptr(fb), ptr(ws), ptr(jobs), len(lay.jobs), stream()))
    written = torch.zeros(lay.n_ws, dtype=torch.bool)
    for j, m in zip(lay.jobs, mats):
        C, n = j.C, j.C * j.C
        r = X.lu_prepare_ref({k: (X.f32r(v) if v.dtype == F64 else v) for k, v in m.items()})
        got = {k: ws[j.w_off + i * n: j.w_off + (i + 1) * n].view(C, C) for i, k in enumerate(("W", "Winv", "wl", "wu"))}
        written[j.w_off: j.w_off + 4 * n] = True
        what = f"lu_prepare C={C}"
        if exact:
            for k in got:
                assert_same(got[k].contiguous() + 0.0, r[k] + 0.0, f"{what} {k}", lambda i: f"row {i // C} column {i % C}")
            assert torch.equal(got["W"].double() @ got["Winv"].double(), torch.eye(C, dtype=F64, device=DEV)), what + ": W W^-1 != I"
        else:
            for k, key, mag in (("wl", "lu_wl_wu", r["wl"]), ("wu", "lu_wl_wu", r["wu"]), ("W", "lu_W", r["mag_W"]),
                                ("Winv", "lu_Winv", r["mag_Winv"])):
                zero = mag == 0                                 # the structural zeros of the triangular factors are exact zeros
                assert bool((got[k].cpu()[zero] == 0).all()), f"{what} {k}: a structural zero is not zero"
                assert_units(got[k].cpu()[~zero], r[k][~zero], mag[~zero], gpu_bound(key), F32, f"{what} {k}")
    assert bool((ws.cpu()[~written] == SENT).all()), "lu_prepare: write outside the jobs' workspace"


@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("M,C,ld", X.LU_APPLY_CASES)
def test_lu_apply(M, C, ld, transposed):
    x, mat = X.lu_apply_operands(M, C, ld)
    assert not torch.equal(mat, mat.t()) or C == 1
    xb, ob = state(x), guarded(M, ld, F32, DEV)
    mb = flat(C * C, mat)
    run(lib().ipoke_lu_apply(ptr(xb), ptr(ob), M, ld, C, ptr(mb), transposed, stream()))
    what = f"lu_apply M={M} C={C} ld={ld} transposed={transposed}"
    assert_same(ob[:M].contiguous(), X.lu_apply_ref(x, C, mat, transposed), what, lambda i: f"row {i // ld} column {i % ld}")
    check_guard(ob, M, ld, None, what)


@pytest.mark.parametrize("B,P8,C,ld", X.LU_WGRAD_CASES)
def test_lu_wgrad(B, P8, C, ld):
    M = B * P8
    lay = X.LuLayout([3, C])                                    # the layer under test is the second job of its table
    m = X.lu_operands(C, True)
    params, fbuf = lay.fill([X.lu_operands(3, True), m])
    j = lay.jobs[1]
    r = X.lu_prepare_ref(m)
    ws = torch.full((lay.n_ws,), SENT, dtype=F64)
    n = C * C
    ws[j.w_off + 2 * n: j.w_off + 3 * n], ws[j.w_off + 3 * n: j.w_off + 4 * n] = r["wl"].reshape(-1), r["wu"].reshape(-1)
    dy, x, dld = X.lu_wgrad_operands(B, P8, C, ld)
    dyf, xf = dy.clone(), x.clone()
    dyf[:, C:], xf[:, C:] = SENT, SENT                          # the columns beyond the layer belong to others
    grads = flat(lay.n_params, tail=0)
    jobs = X.table_to_device(lay.jobs, DEV)
    job1 = jobs[ctypes.sizeof(X.LuJob):]
    dyb, xb, pb, fb, wsb, dldb = state(dyf), state(xf), dev(params), dev(fbuf), dev(ws), dev(dld)
    run(lib().ipoke_lu_wgrad(ptr(dyb), ptr(xb), B, P8, ld, ptr(pb), ptr(fb), ptr(wsb), ptr(job1), ptr(dldb), ptr(grads), stream()))
    dl, du, dls = X.lu_wgrad_ref(dy[:, :C], x[:, :C], m, r["wl"], r["wu"], dld, P8)
    what = f"lu_wgrad B={B} P8={P8} C={C} ld={ld}"
    where = lambda i: f"row {i // C} column {i % C}"            # noqa: E731
    assert_same(grads[j.p_l: j.p_l + n] + 0.0, dl + 0.0, what + " dl", where)         # (+ 0.0: a masked-out -0 is a zero)
    assert_same(grads[j.p_u: j.p_u + n] + 0.0, du + 0.0, what + " du", where)
    assert_same(grads[j.p_logs: j.p_logs + C], dls, what + " dlog_s")
    mine = torch.zeros(lay.n_params, dtype=torch.bool)
    for o, cnt in ((j.p_l, n), (j.p_u, n), (j.p_logs, C)):
        mine[o: o + cnt] = True
    assert bool((grads.cpu()[~mine] == SENT).all()), what + ": write outside the layer's gradients"
