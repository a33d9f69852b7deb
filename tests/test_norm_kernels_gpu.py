"""The first stage's normalisation kernels and the small kernels around them, one by one against the float64 references of
tests/norm_exact.py: ipoke_groupnorm / ipoke_groupnorm_stats on every dispatch path and on shifted means, ipoke_groupnorm_bwd on its
apply paths, the layout converters, the bilinear resize and the reparameterisation.  Every buffer is guarded by sentinels and no element
is left out of a comparison in either dtype.  Each test prints its worst figures (``NORMFIG ...``) before it asserts."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from ipoke_amd._lib import ptr
from tests import norm_exact as X
from tests.norm_exact import DTYPES, F32, F64, SENT, assert_same, check_guard, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOTH = pytest.mark.parametrize("dt", ["f32", "bf16"])


def lib():
    return _lib.lib()


def run(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def flat(n, fill=SENT, dtype=torch.float32):
    return torch.full((n,), fill, dtype=dtype, device=DEV)


def vec(v, pad=8):
    """an fp32 [C] operand with SENT behind it"""
    return None if v is None else torch.cat([v.to(torch.float32).to(DEV), flat(pad)])


def fig(what, **figs):
    print("NORMFIG " + what + " " + " ".join(f"{k} {v:.2f}" for k, v in figs.items()))


# ------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=None)
def forward_operands(name, dt):
    """operands of a case on the device (drawn on the CPU, as test_norm_kernels_cpu.py checks them; the large cases on the device)"""
    c = X.CASE[name]
    if c.big:
        return X.fwd_inputs(c, dt, device=DEV)
    return {k: (v.to(DEV) if v is not None else None) for k, v in X.fwd_inputs(c, dt).items()}


def launch_forward(c, dt, o, ws=None):
    """one ipoke_groupnorm call on guarded buffers; ws: the next_part buffer a producer left (a consumer's workspace)"""
    code, tdt, _ = DTYPES[dt]
    ldx, ldy, ldr, ldm = X.pitches(c, dt)
    M = c.N * c.S
    b = dict(x=guarded(M, ldx, tdt, DEV, o["x"].reshape(M, c.C)), y=guarded(M, ldy, torch.float32 if c.y_f32 else tdt, DEV),
             gamma=vec(o["gamma"]), beta=vec(o["beta"]))
    b["mg"] = guarded(X.mod_rows(c) * c.S, ldm, tdt, DEV, o["mg"].reshape(-1, c.C)) if c.mod else None
    b["mb"] = guarded(X.mod_rows(c) * c.S, ldm, tdt, DEV, o["mb"].reshape(-1, c.C)) if c.mod else None
    b["res"] = guarded(M, ldr, tdt, DEV, o["res"].reshape(M, c.C)) if c.res else None
    b["wsf"] = lib().ipoke_groupnorm_workspace_floats(c.N, c.S, c.G)
    b["ws"] = flat(b["wsf"] + 64) if ws is None else ws
    assert b["ws"].numel() == b["wsf"] + 64
    if c.next_G:
        b["nf"] = lib().ipoke_groupnorm_workspace_floats(c.N, c.S, c.next_G)
        b["next"] = flat(b["nf"] + 64)
    d = X.make_desc(c, dt, *(b[k].data_ptr() if b[k] is not None else None for k in ("x", "y", "gamma", "beta", "mg", "mb", "res", "ws")),
                    next_part=b["next"].data_ptr() if c.next_G else None)
    run(lib().ipoke_groupnorm(ctypes.byref(d), code, _lib.current_stream()))
    return b


def check_forward(c, dt, o, b):
    """y, the (mean, rstd) table and the next_part triples against float64, every element; the guards of y, workspace and next_part"""
    tdt = DTYPES[dt][1]
    what = f"groupnorm {c.name} {dt}"
    M = c.N * c.S
    ref = X.fwd_ref(c, o)
    y = b["y"][:M, :c.C].reshape(c.N, c.S, c.C)
    off = lib().ipoke_groupnorm_stats_offset(c.N, c.S, c.G)
    st = b["ws"][off: off + c.N * c.G * 2].view(c.N, c.G, 2)
    u = lambda got, r, mag, store=None: float(X.units(got, r, mag, store).max())      # noqa: E731
    figs = dict(y=u(y, ref["y"], ref["mag"], None if c.y_f32 else tdt), mean=u(st[..., 0], ref["mean"], ref["mean"]),
                rstd=u(st[..., 1], ref["rstd"], ref["rstd"]))
    trip = None
    if c.next_G:
        nch = X.next_chunks(c)
        trip = b["next"][: c.N * nch * c.next_G * 3].view(c.N, nch, c.next_G, 3)
        noff = lib().ipoke_groupnorm_stats_offset(c.N, c.S, c.next_G)
        table = b["next"][noff: noff + c.N * c.next_G * 2].view(c.N, c.next_G, 2)      # the following norm's (mean, rstd) table
        nmean = trip[..., 1].to(F64) + table[..., 0].to(F64).view(c.N, 1, c.next_G)       # chunk means are relative to the group's pivot
        nref = X.chunk_stats_ref(y.to(F64), c)
        figs.update(nmean=u(nmean, nref["mean"], nref["mean_mag"]), nm2=u(trip[..., 2], nref["m2"], nref["m2_mag"]))
    fig(what, **figs)
    X.assert_units(what + " y", y, ref["y"], ref["mag"], X.gpu_bound("y", c.family, dt), None if c.y_f32 else tdt)
    X.assert_units(what + " mean", st[..., 0], ref["mean"], ref["mean"], X.gpu_bound("mean", c.family, dt))
    X.assert_units(what + " rstd", st[..., 1], ref["rstd"], ref["rstd"], X.gpu_bound("rstd", c.family, dt))
    check_guard(b["y"], M, c.C, None, what + " y")
    assert bool((b["ws"][b["wsf"]:] == SENT).all()), what + ": write behind the workspace"
    if c.producer:          # between the triples the producer left and the (mean, rstd) table nothing is written
        assert bool((b["ws"][c.N * X.next_chunks(c) * c.G * 3: off] == SENT).all()), what + ": write between the chunk statistics and the table"
    if c.next_G:
        assert_same(trip[..., 0].contiguous(), nref["cnt"], what + " next_part count")
        X.assert_units(what + " next_part mean", nmean, nref["mean"], nref["mean_mag"], X.gpu_bound("nmean", c.family, dt))
        X.assert_units(what + " next_part M2", trip[..., 2], nref["m2"], nref["m2_mag"], X.gpu_bound("nm2", c.family, dt))
        # beyond the triples only the pivots are written: the mean slots of the table; the rstd slots and everything else stay
        assert bool((b["next"][trip.numel(): noff] == SENT).all()), what + ": write behind the chunk statistics of next_part"
        assert bool((table[..., 1] == SENT).all()) and bool((b["next"][b["nf"]:] == SENT).all()), what + ": write behind next_part"
        assert bool(torch.isfinite(table[..., 0]).all()) and bool((table[..., 0] != SENT).all()), what + ": pivots not written"
    return y


def forward_chain(c, dt):
    """runs and checks a case; a consumer first runs its producer and reads what that call stored"""
    if c.producer:
        p = X.CASE[c.producer]
        po = forward_operands(p.name, dt)
        pb = launch_forward(p, dt, po)
        py = pb["y"][: p.N * p.S, : p.C].reshape(p.N, p.S, p.C).to(F64)
        o = {k: (v.to(DEV) if v is not None else None) for k, v in X.fwd_inputs(c, dt, x=py.cpu()).items()}
        return check_forward(c, dt, o, launch_forward(c, dt, o, ws=pb["next"]))
    o = forward_operands(c.name, dt)
    return check_forward(c, dt, o, launch_forward(c, dt, o))


@BOTH
@pytest.mark.parametrize("name", [c.name for c in X.FWD_CASES])
def test_groupnorm_forward(name, dt):
    c = X.CASE[name]
    assert X.path_of(c, dt)[0] == X.EXPECT_PATH[name]
    forward_chain(c, dt)


@pytest.mark.parametrize("name", [c.name for c in X.BIG_CASES])
def test_groupnorm_forward_32_mib(name):
    c = X.CASE[name]
    assert X.path_of(c, "bf16")[0] == X.EXPECT_PATH[name]
    forward_chain(c, "bf16")
    forward_operands.cache_clear()                  # 134 MB of float64 operands per case: not kept for the rest of the session


@BOTH
@pytest.mark.parametrize("name", ["tails-three", "chunks300-f32out", "shifted-three", "shifted-chunks300", "c1280"])
def test_groupnorm_stats_entry(name, dt):
    """ipoke_groupnorm_stats alone (what the backward calls to recompute the statistics): the same table, the same workspace bounds"""
    c = X.CASE[name]
    code, tdt, _ = DTYPES[dt]
    o = forward_operands(name, dt)
    ldx, M = X.pitches(c, dt)[0], c.N * c.S
    xb = guarded(M, ldx, tdt, DEV, o["x"].reshape(M, c.C))
    wsf = lib().ipoke_groupnorm_workspace_floats(c.N, c.S, c.G)
    ws = flat(wsf + 64)
    run(lib().ipoke_groupnorm_stats(ptr(xb), ldx, c.N, c.S, c.C, c.G, X.EPS, ptr(ws), code, _lib.current_stream()))
    off = lib().ipoke_groupnorm_stats_offset(c.N, c.S, c.G)
    st = ws[off: off + c.N * c.G * 2].view(c.N, c.G, 2)
    mean, rstd = X.group_stats(o["x"], c.G, F64)
    what = f"groupnorm_stats {name} {dt}"
    fig(what, mean=float(X.units(st[..., 0], mean, mean).max()), rstd=float(X.units(st[..., 1], rstd, rstd).max()))
    X.assert_units(what + " mean", st[..., 0], mean, mean, X.gpu_bound("mean", c.family, dt))
    X.assert_units(what + " rstd", st[..., 1], rstd, rstd, X.gpu_bound("rstd", c.family, dt))
    assert bool((ws[wsf:] == SENT).all()), what + ": write behind the workspace"
    # the chunk statistics in front of the table: counts exactly, chunks of 128 positions
    nch = (c.S + 127) // 128
    cnt = ws[: c.N * nch * c.G * 3].view(c.N, nch, c.G, 3)[..., 0]
    rows = torch.tensor([min(128, c.S - k * 128) for k in range(nch)], dtype=torch.float32, device=DEV) * (c.C // c.G)
    assert_same(cnt.contiguous(), rows.view(1, nch, 1).expand(c.N, nch, c.G).contiguous(), what + " chunk counts")


# ------------------------------------------------------------------ layout converters
@BOTH
@pytest.mark.parametrize("N,C,S,ld", [(1, 8, 5, 8), (3, 6, 35, 16), (2, 3, 7, 4), (2, 20, 300, 40)])
def test_layout_converters_bit_exact(N, C, S, ld, dt):
    code, tdt, _ = DTYPES[dt]
    gen = torch.Generator().manual_seed(N * 1000 + C)
    x = X.randint64(-100, 100, (N, C, S), gen)                         # exact in bf16
    src = torch.cat([x.reshape(-1).to(torch.float32).to(DEV), flat(64)])
    yb = guarded(N * S, ld, tdt, DEV)
    run(lib().ipoke_nchw_to_cl(ptr(src), ptr(yb), ld, N, C, S, code, _lib.current_stream()))
    what = f"nchw_to_cl N={N} C={C} S={S} ld={ld} {dt}"
    assert_same(yb[: N * S].contiguous(), X.nchw_to_cl_ref(x, ld), what, lambda i: f"row {i // ld} column {i % ld}")
    check_guard(yb, N * S, C, ld, what)                                # zeros up to the pitch, nothing behind the last row
    # the way back, from a buffer whose padding holds SENT: the padding is ignored
    cl = torch.zeros((N * S, C), dtype=F64)
    for n in range(N):
        cl[n * S:(n + 1) * S] = x[n].t()
    xb = guarded(N * S, ld, tdt, DEV, cl.to(DEV))
    out = flat(N * C * S + 64)
    run(lib().ipoke_cl_to_nchw(ptr(xb), ld, ptr(out), N, C, S, code, _lib.current_stream()))
    what = f"cl_to_nchw N={N} C={C} S={S} ld={ld} {dt}"
    assert_same(out[: N * C * S].view(N, C, S), X.cl_to_nchw_ref(cl, N, C, S).to(torch.float32), what,
                lambda i: f"sample {i // (C * S)} channel {i // S % C} position {i % S}")
    assert bool((out[N * C * S:] == SENT).all()), what + ": write behind the output"


# ------------------------------------------------------------------ bilinear resize
def bilinear_weights_mag(x, Ho, Wo):
    """sum |w_i p_i| of F.interpolate(bilinear, align_corners=True): the interpolation of |x| (its weights are >= 0)"""
    return F.interpolate(x.abs(), size=(Ho, Wo), mode="bilinear", align_corners=True)


BILINEAR_CASES = {
    "up": (2, 5, 4, 6, 9, 11), "down": (2, 3, 9, 12, 4, 5), "nonsquare": (1, 8, 3, 7, 10, 4), "ho1": (2, 3, 5, 6, 1, 9),
    "wo1": (2, 3, 5, 6, 7, 1), "hi1": (2, 4, 1, 6, 5, 11),
}


@pytest.mark.parametrize("name", list(BILINEAR_CASES))
def test_bilinear_against_float64(name):
    N, C, Hi, Wi, Ho, Wo = BILINEAR_CASES[name]
    gen = torch.Generator().manual_seed(7)
    x32 = (2.0 * torch.randn((N, C, Hi, Wi), generator=gen) + 0.7)
    x = x32.to(F64)
    ref = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True)
    mag = bilinear_weights_mag(x, Ho, Wo)
    yard = float(X.units(F.interpolate(x32, size=(Ho, Wo), mode="bilinear", align_corners=True), ref, mag).max())
    assert yard <= X.YARDSTICK_CAP, yard
    src = torch.cat([x32.reshape(-1).to(DEV), flat(64)])
    out = flat(N * Ho * Wo * C + 64)
    run(lib().ipoke_bilinear_cl(ptr(src), ptr(out), N, C, Hi, Wi, Ho, Wo, _lib.current_stream()))
    got = out[: N * Ho * Wo * C].view(N, Ho, Wo, C).permute(0, 3, 1, 2).cpu()
    what = f"bilinear {name}"
    fig(what, yardstick=yard, kernel=float(X.units(got, ref, mag).max()))
    X.assert_units(what, got, ref, mag, max(4.0 * yard, 4.0))
    assert bool((out[N * Ho * Wo * C:] == SENT).all()), what + ": write behind the output"


@pytest.mark.parametrize("name,shape", [("identity", (2, 5, 6, 7, 6, 7)), ("dyadic-9-17", (2, 3, 9, 9, 17, 17)), ("dyadic-5x3-9x5", (1, 4, 5, 3, 9, 5)),
                                        ("dyadic-129-257-wrap", (1, 16, 129, 129, 257, 257))])      # 1 056 784 outputs > 4096 blocks of 256: the grid wraps
def test_bilinear_bit_exact(name, shape):
    """identity size: a copy.  2^k + 1 -> 2^(k+1) + 1 on integers: every source coordinate is a multiple of 1/2 (exactly: the ratio
    2^k / 2^(k+1) and its products are), the weights are 0, 1/2, 1 and every output is a multiple of 1/4 below 2^9"""
    N, C, Hi, Wi, Ho, Wo = shape
    x = X.randint64(-100, 100, (N, C, Hi, Wi), torch.Generator().manual_seed(11))
    ref = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True)
    src = torch.cat([x.reshape(-1).to(torch.float32).to(DEV), flat(64)])
    out = flat(N * Ho * Wo * C + 64)
    run(lib().ipoke_bilinear_cl(ptr(src), ptr(out), N, C, Hi, Wi, Ho, Wo, _lib.current_stream()))
    assert_same(out[: N * Ho * Wo * C].view(N, Ho, Wo, C), ref.permute(0, 2, 3, 1).contiguous().to(torch.float32), f"bilinear {name}",
                lambda i: f"sample {i // (Ho * Wo * C)} row {i // (Wo * C) % Ho} column {i // C % Wo} channel {i % C}")
    assert bool((out[N * Ho * Wo * C:] == SENT).all())


# ------------------------------------------------------------------ reparameterisation
reparam_data = X.reparam_data


@BOTH
@pytest.mark.parametrize("exact", [True, False], ids=["integers", "real-logvar"])
@pytest.mark.parametrize("absent", ["none", "eps", "mu", "logvar"])
def test_reparameterize(absent, exact, dt):
    code, tdt, e = DTYPES[dt]
    M, Z = 37, 12
    ld = 2 * Z + e
    mu, lv, eps, _, _, _ = reparam_data(M, Z, exact, tdt, 5)
    mb = guarded(M, ld, tdt, DEV, torch.cat([mu, lv], dim=1).to(DEV))
    eb = torch.cat([eps.reshape(-1).to(torch.float32).to(DEV), flat(64)]) if absent != "eps" else None
    zb, mub, lvb = flat(M * Z + 64), (flat(M * Z + 64) if absent != "mu" else None), (flat(M * Z + 64) if absent != "logvar" else None)
    run(lib().ipoke_reparameterize(ptr(mb), ld, ptr(eb), ptr(zb), ptr(mub), ptr(lvb), M, Z, code, _lib.current_stream()))
    what = f"reparameterize {absent} absent {'exact' if exact else 'real'} {dt}"
    sig = torch.exp(0.5 * lv)
    zref = mu + eps * sig if absent != "eps" else mu
    got = zb[: M * Z].view(M, Z).cpu()
    if exact or absent == "eps":
        assert_same(got, zref.to(torch.float32), what + " z")
    else:
        mag = mu.abs() + (eps * sig).abs()
        z32 = mu.float() + eps.float() * torch.exp(0.5 * lv.float())
        yard = float(X.units(z32, zref, mag).max())
        assert yard <= X.YARDSTICK_CAP
        fig(what, yardstick=yard, kernel=float(X.units(got, zref, mag).max()))
        X.assert_units(what + " z", got, zref, mag, max(4.0 * yard, 4.0))
    for buf, r in ((mub, mu), (lvb, lv)):
        if buf is not None:
            assert_same(buf[: M * Z].view(M, Z).cpu(), r.to(torch.float32), what + " mu / logvar copies")
            assert bool((buf[M * Z:] == SENT).all())
    assert bool((zb[M * Z:] == SENT).all()), what + ": write behind z"


@BOTH
@pytest.mark.parametrize("exact", [True, False], ids=["integers", "real-logvar"])
@pytest.mark.parametrize("absent", ["none", "dz", "dmu", "dlv", "eps"])
def test_reparam_bwd(absent, exact, dt):
    code, tdt, e = DTYPES[dt]
    M, Z = 37, 12
    ld, ldo = 2 * Z + e, 2 * Z + 2 * e
    mu, lv, eps, dz, dmu, dlv = reparam_data(M, Z, exact, tdt, 6)
    mb = guarded(M, ld, tdt, DEV, torch.cat([mu, lv], dim=1).to(DEV))
    f = lambda name, v: torch.cat([v.reshape(-1).to(torch.float32).to(DEV), flat(64)]) if absent != name else None      # noqa: E731
    eb, dzb, dmub, dlvb = f("eps", eps), f("dz", dz), f("dmu", dmu), f("dlv", dlv)
    ob = guarded(M, ldo, tdt, DEV)
    run(lib().ipoke_reparam_bwd(ptr(mb), ld, ptr(eb), ptr(dzb), ptr(dmub), ptr(dlvb), ptr(ob), ldo, M, Z, code, _lib.current_stream()))
    what = f"reparam_bwd {absent} absent {'exact' if exact else 'real'} {dt}"
    zero = torch.zeros((M, Z), dtype=F64)
    g_dz, g_dmu, g_dlv = (zero if absent == n else v for n, v in (("dz", dz), ("dmu", dmu), ("dlv", dlv)))
    chain = g_dz * eps * 0.5 * torch.exp(0.5 * lv) if absent != "eps" else zero
    ref_mu, ref_lv = g_dz + g_dmu, g_dlv + chain
    got = ob[:M, : 2 * Z].to(F64).cpu()
    if exact:
        assert_same(ob[:M, : 2 * Z].contiguous().cpu(), torch.cat([ref_mu, ref_lv], dim=1), what)
    else:
        mag = torch.cat([g_dz.abs() + g_dmu.abs(), g_dlv.abs() + chain.abs()], dim=1)
        ref = torch.cat([ref_mu, ref_lv], dim=1)
        c32 = (g_dz.float() * eps.float() * 0.5 * torch.exp(0.5 * lv.float())) if absent != "eps" else zero.float()
        r32 = torch.cat([g_dz.float() + g_dmu.float(), g_dlv.float() + c32], dim=1)
        yard = float(X.units(r32, ref, mag).max())
        assert yard <= X.YARDSTICK_CAP
        fig(what, yardstick=yard, kernel=float(X.units(got, ref, mag, tdt).max()))
        X.assert_units(what, got, ref, mag, max(4.0 * yard, 4.0), tdt)
    check_guard(ob, M, 2 * Z, ldo, what)                               # columns [2Z, ldo) are zero


# ------------------------------------------------------------------ backward
@BOTH
@pytest.mark.parametrize("name", list(X.BWD))
def test_groupnorm_backward(name, dt):
    """ipoke_groupnorm_bwd against float64 autograd, every element of every output; integer dy makes dres / dmod_beta (and dbeta without
    modulation) bit-exact under ReLU or no activation; guards on every output and on both workspaces.  dmod_summed: the gradients of the
    shared maps summed over the frames, rounded once.  The row-scale fold: the stored dx against round(dx) / sigma_t (bf16: two bf16
    ulps, it is rounded twice), rs_dots / rs_dbias within what the dx bound lets every element be off by, carried through the sum, plus 4
    fp32 ulps of the sum's term magnitudes.  In bf16 that carries one bf16 ulp of every element and is wide (about half a typical dot at
    19 200 terms); the f32 run of the same case goes through the same indexing with a tolerance of 1e-5 of a typical dot."""
    c = X.BWD[name]
    code, tdt, _ = DTYPES[dt]
    o = X.bwd_inputs(c, dt)
    ref = {k: (v.to(DEV) if v is not None else None) for k, v in X.bwd_ref(c, o).items()}
    _, mag = X.bwd_restated(c, o, F64)
    mag = {k: v.to(DEV) for k, v in mag.items()}
    ldx, ldy, lddy, lddx, lddres, ldm, lddm = X.bwd_pitches(c, dt)
    M, C = c.N * c.S, c.C
    g2 = lambda v, ld, rows=M: guarded(rows, ld, tdt, DEV, v.reshape(rows, C).to(DEV))      # noqa: E731
    b = dict(x=g2(o["x"], ldx), y=g2(o["y"], ldy), dy=g2(o["dy"], lddy), dx=guarded(M, lddx, tdt, DEV))
    b["dres"] = guarded(M, lddres, tdt, DEV) if c.res else None
    b["mg"] = g2(o["mg"], ldm, o["mg"].shape[0] * c.S) if c.mod else None
    Mm = c.mod * c.S if c.summed else M                     # rows of the modulation gradients
    b["dmg"], b["dmb"] = (guarded(Mm, lddm, tdt, DEV), guarded(Mm, lddm, tdt, DEV)) if c.mod else (None, None)
    b["gamma"], b["beta"] = vec(o["gamma"]), vec(o["beta"])
    b["dgamma"], b["dbeta"] = (flat(C + 8), flat(C + 8)) if c.affine else (None, None)
    wsf = lib().ipoke_groupnorm_bwd_workspace_floats(c.N, c.S, C, c.G)
    ws = flat(wsf + 64)
    stats = torch.cat([o["stats"].reshape(-1).to(torch.float32).to(DEV), flat(8)]) if c.saved else None
    d = _lib.NormBwdDesc()
    d.x, d.ldx, d.y, d.ldy, d.dy, d.lddy, d.dx, d.lddx = b["x"].data_ptr(), ldx, b["y"].data_ptr(), ldy, b["dy"].data_ptr(), lddy, b["dx"].data_ptr(), lddx
    if c.act == _lib.ACT_NONE:
        d.y = None                                          # not read without an activation (the entry asks for it with one, act_from_pre too)
    if c.res:
        d.dres, d.lddres = b["dres"].data_ptr(), lddres
    if c.mod:
        d.mod_gamma, d.ld_mod, d.dmod_gamma, d.dmod_beta, d.ld_dmod = b["mg"].data_ptr(), ldm, b["dmg"].data_ptr(), b["dmb"].data_ptr(), lddm
        d.mod_samples = max(c.mod, 0)
    d.N, d.S, d.C, d.G, d.eps, d.act, d.act_from_pre = c.N, c.S, C, c.G, X.EPS, c.act, int(c.from_pre)
    if c.affine:
        d.gamma, d.beta, d.dgamma, d.dbeta = b["gamma"].data_ptr(), b["beta"].data_ptr(), b["dgamma"].data_ptr(), b["dbeta"].data_ptr()
    d.workspace = ws.data_ptr()
    d.stats = stats.data_ptr() if c.saved else None
    d.dmod_summed = int(c.summed)
    if c.rs:
        clips, stride, with_bias, with_dbias = c.rs
        frames = c.N // clips
        scale = flat(frames * stride + 8)                   # 1 / sigma_t at [t * stride], SENT between: a wrong stride shows
        scale[: frames * stride: stride] = torch.tensor(X.RS_SCALES[:frames], device=DEV)
        rswf = lib().ipoke_groupnorm_bwd_rs_workspace_floats(c.N, c.S, C)
        rsws, dots, dbias = flat(rswf + 64), flat(frames + 8), flat(C + 8)
        rsb = vec(o["rs_bias"]) if with_bias else None
        d.rs_scale, d.rs_scale_stride, d.rs_rows_per_group, d.rs_dots, d.rs_workspace = scale.data_ptr(), stride, clips * c.S, dots.data_ptr(), rsws.data_ptr()
        d.rs_bias = rsb.data_ptr() if with_bias else None
        d.rs_dbias = dbias.data_ptr() if with_dbias else None
    run(lib().ipoke_groupnorm_bwd(ctypes.byref(d), code, _lib.current_stream()))
    what = f"groupnorm_bwd {name} {dt}"
    got = dict(dx=b["dx"], dres=b["dres"], dmg=b["dmg"], dmb=b["dmb"])
    got = {k: (v[: (Mm if k in ("dmg", "dmb") else M), :C].reshape(-1, c.S, C) if v is not None else None) for k, v in got.items()}
    if c.rs:                # the fold: dx leaves as round(dx) / sigma_t; the frame's <dx, x - b> and the column sums of the same rounded dx
        fr = {k: v.to(DEV) for k, v in X.fold_ref(c, o, ref["dx"].cpu()).items()}
        B, bf = X.bwd_bound("dx", dt), tdt == torch.bfloat16
        per_el = B * X.ulp_f32(mag["dx"]) + (X.ulp_bf16(ref["dx"]) if bf else 0.0)          # what one element of the kernel's rounded dx may be off by
        err = (got["dx"].to(F64) - fr["dx"]).abs() - (2.0 * X.ulp_bf16(fr["dx"]) if bf else 0.0)
        u_dx = float((err.clamp(min=0) / X.ulp_f32(mag["dx"] * fr["sc"])).max())
        tol_dots = (per_el * fr["xm"]).view(frames, -1).sum(dim=1) + 4.0 * X.ulp_f32(fr["dots_mag"])
        tol_dbias = per_el.sum(dim=(0, 1)) + 4.0 * X.ulp_f32(fr["dbias_mag"])
        e_dots = (dots[:frames].to(F64) - fr["dots"]).abs()
        fig(what + " fold", dx=u_dx, dots=float((e_dots / tol_dots).max()))
        assert u_dx <= B, (what, "stored dx = round(dx) / sigma_t", u_dx, B)
        assert bool((e_dots <= tol_dots).all()), (what, "rs_dots", dots[:frames].tolist(), fr["dots"].tolist(), tol_dots.tolist())
        if with_dbias:
            e_db = (dbias[:C].to(F64) - fr["dbias"]).abs()
            assert bool((e_db <= tol_dbias).all()), (what, "rs_dbias", float((e_db / tol_dbias).max()))
        else:
            assert bool((dbias == SENT).all()), what + ": rs_dbias written though NULL was passed"
        assert bool((dots[frames:] == SENT).all()) and bool((dbias[C:] == SENT).all()), what + ": write behind rs_dots / rs_dbias"
        assert bool((rsws[rswf:] == SENT).all()), what + ": write behind the row-scale workspace"
        got["dx"], ref["dx"] = None, None                   # compared above in its folded form
    got.update(dgamma=b["dgamma"][:C] if c.affine else None, dbeta=b["dbeta"][:C] if c.affine else None)
    store = {"dx": tdt, "dres": tdt, "dmg": tdt, "dmb": tdt, "dgamma": None, "dbeta": None}
    fig(what, **{k: float(X.units(got[k], ref[k], mag[k], store[k]).max()) for k in X.BWD_QTY if ref[k] is not None})
    for k in X.BWD_QTY:
        assert (got[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            X.assert_units(f"{what} {k}", got[k], ref[k].reshape(got[k].shape), mag[k].reshape(got[k].shape), X.bwd_bound(k, dt), store[k])
    if c.act in (_lib.ACT_NONE, _lib.ACT_RELU) and not c.from_pre:           # integer dy: bit for bit
        for k in ("dres", "dmb"):
            if ref[k] is not None:
                assert_same(got[k].contiguous(), ref[k], f"{what} {k} (exact)")
        if c.affine and not c.mod:
            assert_same(got["dbeta"].contiguous(), ref["dbeta"], what + " dbeta (exact)")
    for k, ld in (("dx", lddx), ("dres", lddres), ("dmg", lddm), ("dmb", lddm)):
        if b[k] is not None:
            check_guard(b[k], Mm if k in ("dmg", "dmb") else M, C, None, f"{what} {k}")
    for k in ("dgamma", "dbeta"):
        if b[k] is not None:
            assert bool((b[k][C:] == SENT).all()), f"{what}: write behind {k}"
    assert bool((ws[wsf:] == SENT).all()), what + ": write behind the workspace"
