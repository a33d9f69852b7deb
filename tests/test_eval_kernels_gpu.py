"""The evaluation kernels (csrc/eval.hip) one by one through the C ABI against the float64 references of tests/eval_exact.py: the clip
resize with its running minimum and the conditional de-normalisation, the TF-SAME max pooling, the weighted row pooling, the activation
moments, PSNR / SSIM and the best-of-n SSIM phase by phase on the stored workspace, the sample statistics, the pairwise MSE, the time
cosine on every dispatch path, the uint8 export and the VGG normalisation.  Bit-exact where the arithmetic is, within
eval_exact.gpu_bound or the derived bounds of eval_exact's docstring elsewhere; every buffer lies between sentinels, which are checked
after every call, and every element is compared."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd._lib import ptr
from tests import eval_exact as X
from tests import eval_ref
from tests.eval_exact import (BF16, DTYPES, F32, F64, assert_close_ulp, assert_same, assert_units, bits32, check_fence, fenced,
                              gpu_bound)

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32, U8 = torch.int32, torch.uint8


def lib():
    return _lib.lib()


def run(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def refused(rc):
    assert rc != 0, "the call was accepted"
    torch.cuda.synchronize()


def stream():
    return _lib.current_stream()


def flat(n, dtype=F32, values=None):
    """(whole, body [n]) between two fences"""
    whole, body = fenced(1, n, dtype, DEV, None if values is None else values.reshape(1, -1))
    return whole, body[0]


def host(t):
    return t.to(F64).cpu()


def units(key, got, ref, mag, tdt, what):
    """every element within gpu_bound(key) units; the worst is printed first (pytest -s), for the table of DESIGN.md"""
    print(f"measured {key}: {X.err_units(got, ref, mag, tdt):.3f} of {gpu_bound(key)} units ({what})")
    assert_units(got, ref, mag, gpu_bound(key), tdt, what)


def one_ulp(key, got, ref, what):
    """within 1 fp32 ulp of the float64 value (a double result rounded once)"""
    print(f"measured {key}: {X.err_units(got, ref, ref, F32):.3f} of 1 ulp ({what})")
    assert_close_ulp(host(got), ref, 1, F32, what)


def untouched(whole, what):
    fill = X.fill_of(whole.dtype)
    assert bool((whole.to(F64) == fill).all()), what + ": written"


def raw(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def unchanged(whole, before, what):
    assert torch.equal(raw(whole), raw(before)), what + ": an input changed"               # bit for bit: operands may hold NaN


# ------------------------------------------------------------------ resize, running minimum, de-normalisation
def clip_source(x, layout):
    """x float64 [N][T][C][H][W] inside a fenced fp32 store whose rows are 3 pixels wider: (whole, view [N][T][C][H][W]).  contig: the
    store is [N][T][C]; perm: [N][C][T] read as [N][T][C]; slice: channels 1 .. C of a store with C + 2"""
    N, T, C, H, W = x.shape
    shape = {"contig": (N, T, C, H, W + 3), "perm": (N, C, T, H, W + 3), "slice": (N, T, C + 2, H, W + 3)}[layout]
    whole, body = flat(math.prod(shape))
    st = body.view(shape)
    v = st.permute(0, 2, 1, 3, 4) if layout == "perm" else st[:, :, 1: C + 1] if layout == "slice" else st
    v = v[..., :W]
    v.copy_(x.to(F32))
    assert not v.is_contiguous() and tuple(v.shape) == (N, T, C, H, W)
    return whole, v


def resize_call(v, c, dst, minval):
    s = v.stride()
    pl, pr = X.resize_pads(c)
    run(lib().ipoke_video_to_cl(ctypes.c_void_p(v.data_ptr()), s[0], s[1], s[2], s[3], s[4], c.N, c.T, c.C, c.Hi, c.Wi, ptr(dst), c.Ho, c.Wo,
                                pl, pr, ptr(minval), stream()))


def min_reset(minval):
    run(lib().ipoke_min_reset(ptr(minval), stream()))


def dst_buffer(c):
    pl, pr = X.resize_pads(c)
    Wp = pl + c.Wo + pr
    rows = c.N * c.T * c.Ho * Wp
    whole, body = fenced(rows, c.C, F32, DEV)
    return whole, body, body.view(c.N * c.T, c.Ho, Wp, c.C), pl


def interior(view, c, pl):
    return view[:, :, pl: pl + c.Wo]


def borders_are_zero(view, c, pl, what):
    for part in (view[:, :, :pl], view[:, :, pl + c.Wo:]):
        assert_same(part.contiguous(), torch.zeros_like(part).contiguous(), what + ": border columns")


@pytest.mark.parametrize("c", X.RESIZE_CASES, ids=lambda c: c.name)
def test_resize_values_borders_and_minimum(c):
    x = X.resize_operands(c)
    sw, v = clip_source(x, c.layout)
    before = sw.clone()
    dw, db, view, pl = dst_buffer(c)
    mw, mv = flat(1)
    min_reset(mv)
    resize_call(v, c, db, mv)
    what = f"resize {c.name}"
    ref, mag = X.resize_ref(x.reshape(-1, c.C, c.Hi, c.Wi), c.Ho, c.Wo)
    got = interior(view, c, pl).contiguous()
    if c.exact:
        assert_same(got, ref, what)
    else:
        units("resize", got, ref, mag, F32, what)
    borders_are_zero(view, c, pl, what)
    assert_same(mv, got.min().reshape(1), what + ": the minimum of the produced values")
    check_fence(dw, db.shape[0], c.C, c.C, what + " dst")
    check_fence(mw, 1, 1, 1, what + " minval")
    # dst == NULL: the minimum alone, the same bits
    m2w, m2 = flat(1)
    min_reset(m2)
    resize_call(v, c, None, m2)
    assert_same(m2, mv, what + ": the minimum without dst")
    check_fence(m2w, 1, 1, 1, what + " minval without dst")
    # minval == NULL: the same rows, nothing else
    d2w, d2b, _, _ = dst_buffer(c)
    m3w, _ = flat(1)
    resize_call(v, c, d2b, None)
    assert_same(d2b, db, what + ": dst without minval")
    check_fence(d2w, d2b.shape[0], c.C, c.C, what + " dst without minval")
    untouched(m3w, what + ": a minval that was not passed")
    unchanged(sw, before, what)


MIN_SEQUENCES = [("pos", "pos"), ("pos", None, "pos"), ("neg", None, "neg"), ("neg", "neg"), (None, "nzero"), (None, "nzero", "pzero"), ("pzero",),
                 ("pzero", "pzero", "pzero")]


@pytest.mark.parametrize("seq", MIN_SEQUENCES, ids=lambda s: "+".join(f or "mixed" for f in s))
def test_running_minimum_over_accumulated_calls(seq):
    """one minval over two or three launches, as fvd._resized_min chunks a data set.  mixed + nzero is the -0.0 case: a clip made of -0.0
    must not replace the negative minimum of the clip before it (bit pattern INT_MIN through the signed atomic), and
    ipoke_denorm_if_negative must then still run."""
    c = X.RESIZE_CASES[0]
    mw, mv = flat(1)
    min_reset(mv)
    expect, first = None, None
    for i, fam in enumerate(seq):
        x = X.resize_operands(c, fam, seed=i)
        _, v = clip_source(x, c.layout)
        dw, db, view, pl = dst_buffer(c)
        resize_call(v, c, db, mv)
        got = interior(view, c, pl)
        if fam in ("nzero", "pzero"):                                     # every produced value is that zero, bit for bit
            assert_same(got.contiguous(), x.new_full(got.shape, -0.0 if fam == "nzero" else 0.0), f"a clip of {fam}")
        m = got.min().reshape(1).clone()
        expect = m if expect is None or bool(m < expect) else expect       # a zero of either sign does not replace an equal or lower one
        print(f"running minimum after call {i} ({fam or 'mixed'}): {float(mv[0])!r}, expected {float(expect[0])!r}")
        assert_same(mv, expect, f"running minimum after call {i} of {seq}")
        check_fence(mw, 1, 1, 1, "minval")
        check_fence(dw, db.shape[0], c.C, c.C, "dst")
        if first is None:
            first = (dw, db, view, pl)
    if seq[0] is None:                                                    # the data set has negative pixels: the first clip is de-normalised
        dw, db, view, pl = first
        assert float(mv[0]) < 0
        before = interior(view, c, pl).clone()
        pr = X.resize_pads(c)[1]
        run(lib().ipoke_denorm_if_negative(ptr(db), c.N * c.T * c.Ho, c.Wo, pl, pr, c.C, ptr(mv), stream()))
        assert_same(interior(view, c, pl).contiguous(), X.denorm_ref(before.cpu()).contiguous(), "de-normalisation after the -0.0 clip")
        borders_are_zero(view, c, pl, "de-normalisation")
        check_fence(dw, db.shape[0], c.C, c.C, "de-normalised dst")
    if seq[0] == "pzero":
        assert bits32(mv).item() == 0, "+0.0 only must end at +0.0"


@pytest.mark.parametrize("C,pads", [(3, (2, 3)), (1, (0, 0)), (3, X.stem_pads(5))], ids=["c3-pad23", "c1-nopad", "c3-stem"])
@pytest.mark.parametrize("minval", [-0.5, -1e-30, 0.0, -0.0, 0.25], ids=["neg", "tiny-neg", "pzero", "nzero", "pos"])
def test_denorm_if_negative(minval, C, pads):
    rows, Wo = 7, 5
    pl, pr = pads
    Wp = pl + Wo + pr
    gen = torch.Generator().manual_seed(5)
    x = torch.zeros(rows, Wp, C)
    x[:, pl: pl + Wo] = torch.rand(rows, Wo, C, generator=gen) * 2 - 1
    xw, xb = fenced(rows * Wp, C, F32, DEV, x.reshape(-1, C))
    mw, mv = flat(1, F32, torch.tensor([minval]))
    before, mbefore = xw.clone(), mw.clone()
    run(lib().ipoke_denorm_if_negative(ptr(xb), rows, Wo, pl, pr, C, ptr(mv), stream()))
    what = f"denorm minval {minval!r}"
    if minval < 0:
        expect = x.clone()
        expect[:, pl: pl + Wo] = X.denorm_ref(x[:, pl: pl + Wo])
        assert_same(xb, expect, what)                                     # the interior is fl((x + 1) / 2), the padding keeps its zeros
        check_fence(xw, rows * Wp, C, C, what)
    else:
        unchanged(xw, before, what)
    unchanged(mw, mbefore, what + " minval")


# ------------------------------------------------------------------ max pooling, TF SAME
def pool_call(x, k, s, dt, dims=None):
    code, tdt, e16 = DTYPES[dt]
    N, C = x.shape[:2]
    dhw = tuple(x.shape[2:])
    d, odhw = X.pool_dims(N, C, dhw, k, s)
    dims = d if dims is None else dims
    ldx = X.round_up(C, e16) + e16
    ldy = ldx + e16
    rows_out = dims[0] * dims[5] * dims[6] * dims[7] + 8                 # what the geometry handed over asks for, were it accepted
    xw, xb = fenced(N * math.prod(dhw), ldx, tdt, DEV, X.to_rows(x))
    yw, yb = fenced(rows_out, ldy, tdt, DEV)
    arr = (ctypes.c_int * 20)(*dims)
    before = xw.clone()
    rc = lib().ipoke_pool3d_same(ctypes.cast(arr, ctypes.c_void_p), ptr(xb), ldx, ptr(yb), ldy, code, stream())
    return rc, xw, before, yw, yb, N * math.prod(odhw), ldy


@pytest.mark.parametrize("dt,C", X.POOL_CHANNELS, ids=lambda v: str(v))
@pytest.mark.parametrize("k,s,dhw", X.POOL_GEOMS, ids=lambda v: "x".join(map(str, v)))
def test_pool3d_same_is_bit_exact(k, s, dhw, dt, C):
    tdt = DTYPES[dt][1]
    x = X.pool_operands(C, dhw, tdt)
    rc, xw, before, yw, yb, rows, ldy = pool_call(x, k, s, dt)
    run(rc)
    what = f"pool3d_same {k} {s} {dhw} {dt} C={C}"
    assert_same(yb[:rows, :C].contiguous(), X.to_rows(X.pool_ref(x, k, s)), what)
    check_fence(yw, rows, ldy, C, what)
    untouched(yb[rows:], what + ": rows behind the output")
    unchanged(xw, before, what)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("k,s,dhw", [X.POOL_GEOMS[2], X.POOL_GEOMS[5]], ids=lambda v: "x".join(map(str, v)))
def test_pool3d_same_all_negative_input(k, s, dhw, dt):
    """every window that touches the zero border returns 0, every interior one its own negative maximum"""
    x = X.pool_operands(24, dhw, DTYPES[dt][1], negative=True)
    rc, xw, before, yw, yb, rows, ldy = pool_call(x, k, s, dt)
    run(rc)
    ref = X.to_rows(X.pool_ref(x, k, s))
    assert bool((ref == 0).any()) and bool((ref < 0).any())
    assert_same(yb[:rows, :24].contiguous(), ref, f"pool3d_same all-negative {k} {s} {dhw} {dt}")
    check_fence(yw, rows, ldy, 24, "pool3d_same all-negative")
    unchanged(xw, before, "pool3d_same all-negative")


@pytest.mark.parametrize("why", ["channels", "overhang"])
def test_pool3d_same_refusals_write_nothing(why):
    k, s, dhw = X.POOL_GEOMS[2]
    C = 12 if why == "channels" else 8                                   # 12 bf16 channels are no whole 16-byte chunks
    x = X.pool_operands(C, dhw, BF16)
    dims, odhw = X.pool_dims(X.POOL_N, C, dhw, k, s)
    if why == "overhang":
        dims[7] = odhw[2] + 1                                            # one more window along W: it would start beyond the padded extent
        assert (dims[7] - 1) * s[2] - dims[16] >= dims[19]
    rc, xw, before, yw, yb, rows, ldy = pool_call(x, k, s, "bf16", dims)
    refused(rc)
    untouched(yw, "refused pool3d_same")
    unchanged(xw, before, "refused pool3d_same")


# ------------------------------------------------------------------ weighted row pooling
@pytest.mark.parametrize("weights", X.ROWS_WEIGHTS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", X.ROWS_CASES, ids=lambda c: f"G{c.G}-S{c.S}-C{c.C}")
def test_pool_rows_weighted(c, dt, weights):
    code, tdt, _ = DTYPES[dt]
    x, w = X.rows_operands(c, tdt, weights)
    ldx, ldy = c.C + 3, c.C + 5
    xw, xb = fenced(c.G * c.S, ldx, tdt, DEV, x)
    yw, yb = fenced(c.G, ldy, tdt, DEV)
    ww, wb = flat(c.S, F32, w)
    before, wbefore = xw.clone(), ww.clone()
    run(lib().ipoke_pool_rows_weighted(ptr(xb), ldx, ptr(yb), ldy, c.G, c.S, c.C, ptr(wb), code, stream()))
    what = f"pool_rows_weighted {tuple(c)} {dt} {weights}"
    ref, mag = X.pool_rows_ref(x, w, c.G)
    got = host(yb[:, : c.C])
    if tdt == BF16:                                                       # one bf16 ulp of the value for the output's own rounding
        slack = X.ulp_of(ref, BF16)
        err = ((got - ref).abs() - slack).clamp(min=0)
        print(f"measured pool_rows: {float((err / X.ulp_of(mag, F32)).max()):.3f} of {gpu_bound('pool_rows')} units beyond one bf16 ulp ({what})")
        assert bool((err <= gpu_bound("pool_rows") * X.ulp_of(mag, F32)).all()), what
    else:
        units("pool_rows", got, ref, mag, F32, what)
    check_fence(yw, c.G, ldy, c.C, what)
    unchanged(xw, before, what)
    unchanged(ww, wbefore, what + " weights")


# ------------------------------------------------------------------ activation moments
@pytest.mark.parametrize("c", X.MOM_CASES, ids=lambda c: c.name)
def test_activation_moments(c):
    a = X.mom_operands(c)
    aw, ab = fenced(c.n, c.D, F32, DEV, a)
    muw, mub = flat(c.D, F64)
    sw, sb = fenced(c.D, c.D, F64, DEV)
    ww, wb = flat(c.n + 1, I32)
    before = aw.clone()
    run(lib().ipoke_activation_moments(ptr(ab), c.n, c.D, ptr(mub), ptr(sb), ptr(wb), stream()))
    what = f"activation moments {c.name}"
    valid, mu, mu_mag = X.moments_mean_ref(a)
    assert wb[0].item() == int(valid.sum()) and wb[1:].cpu().numpy().astype(bool).tolist() == valid.tolist(), what + ": the valid rows"
    got_mu, got_sigma = mub.cpu().numpy(), sb.cpu().numpy()
    bound = X.moments_bound(c.n)

    def compare(got, ref, mag, name):
        nan = np.isnan(ref.astype(np.float64))
        assert (np.isnan(got) == nan).all(), f"{what}: {name} is NaN elsewhere than the reference"
        if (~nan).any():
            e = np.abs(got.astype(np.longdouble) - ref)[~nan] / mag[~nan]
            print(f"measured moments_{name}: {float(e.max()) * 2.0 ** 53:.3f} of {c.n + 2} x 2^-53 x magnitude ({what})")
            assert float(e.max()) <= bound, f"{what}: {name} {float(e.max())} beyond {bound}"
    compare(got_mu, mu, mu_mag, "mu")
    sigma, sigma_mag = X.moments_cov_ref(a, got_mu)                       # on the STORED mean
    compare(got_sigma, sigma, sigma_mag, "sigma")
    fin = ~np.isnan(got_sigma)
    assert (fin == fin.T).all() and (got_sigma.view(np.int64)[fin] == got_sigma.T.view(np.int64)[fin]).all(), what + ": sigma is not symmetric"
    check_fence(muw, 1, c.D, c.D, what + " mu")
    check_fence(sw, c.D, c.D, c.D, what + " sigma")
    check_fence(ww, 1, c.n + 1, c.n + 1, what + " workspace")
    unchanged(aw, before, what)


# ------------------------------------------------------------------ PSNR / SSIM, phase by phase
def image_call(a, b):
    planes, H, W = a.shape
    nbytes = int(lib().ipoke_image_metrics_workspace_bytes(planes, H, W))
    ty, tx = X.ssim_tiles(H, W)
    assert nbytes == 64 + 8 * (planes * ty * tx + 1)
    ww, wb = flat(nbytes, U8)
    aw, ab = fenced(planes, H * W, F32, DEV, a.reshape(planes, -1))
    bw, bb = fenced(planes, H * W, F32, DEV, b.reshape(planes, -1))
    ow, ob = flat(2)
    before = (aw.clone(), bw.clone())
    run(lib().ipoke_psnr_ssim(ptr(ab), ptr(bb), planes, H, W, ptr(wb), ptr(ob), stream()))
    unchanged(aw, before[0], "psnr_ssim preds")
    unchanged(bw, before[1], "psnr_ssim target")
    check_fence(ww, 1, nbytes, nbytes, "psnr_ssim workspace")
    check_fence(ow, 1, 2, 2, "psnr_ssim out")
    mm = wb[:16].view(F32).cpu()
    sse = wb[32:40].view(F64).cpu()[0]
    parts = wb[64: 64 + 8 * planes * ty * tx].view(F64).cpu().view(planes, ty * tx)
    return mm, sse, parts, ob.cpu()


def check_stats_phase(a, b, mm, sse, what):
    assert_same(mm, X.mm_ref(a, b), what + ": mm = {-min, max} of both tensors")
    ref = X.sse_ref(a, b)
    n = a.numel()
    print(f"measured sse: {abs(float(sse) - float(ref)) / max(float(ref), 1e-300) * 2.0 ** 53:.3f} of {n} x 2^-53 relative ({what})")
    assert abs(float(sse) - float(ref)) <= n * 2.0 ** -53 * float(ref), what + ": sse"


def same_class(got, ref, key, what):
    """a non-finite reference: the same infinity or NaN; else within one fp32 ulp"""
    g, r = float(got), float(ref)
    if math.isnan(r) or math.isinf(r):
        assert (math.isnan(g) and math.isnan(r)) or g == r, f"{what}: got {g!r}, reference {r!r}"
    else:
        one_ulp(key, got.reshape(1), ref.reshape(1), what)


@pytest.mark.parametrize("kind", X.SSIM_RANGES)
@pytest.mark.parametrize("shape", X.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_psnr_ssim_phase_by_phase(shape, kind):
    a, b = X.image_operands(shape, kind)
    mm, sse, parts, out = image_call(a, b)
    what = f"psnr_ssim {shape} {kind}"
    check_stats_phase(a, b, mm, sse, what)
    same_class(out[0], X.psnr_ref(mm, sse, a.numel()), "psnr", what + ": psnr from the stored mm and sse")
    sums, cnt = X.tile_sums(X.ssim_map_ref(a, b, X.range_of_mm(mm).to(F64)))
    units("ssim_tile", parts, sums, cnt, F32, what + ": per-tile SSIM sums, range from the stored mm")
    count = shape[0] * (shape[1] - 10) * (shape[2] - 10)
    assert float(cnt.sum()) == count
    final = torch.tensor(math.fsum(parts.reshape(-1).tolist()) / count, dtype=F64)
    one_ulp("ssim", out[1:2], final.reshape(1), what + ": ssim from the stored partials")


@pytest.mark.parametrize("kind", X.MM_EDGES)
def test_psnr_ssim_minimum_and_maximum_edges(kind):
    a, b = X.image_operands(X.EDGE_SHAPE, kind)
    mm, sse, parts, out = image_call(a, b)
    what = f"psnr_ssim {kind}"
    check_stats_phase(a, b, mm, sse, what)
    same_class(out[0], X.psnr_ref(mm, sse, a.numel()), "psnr", what + ": psnr")


@pytest.mark.parametrize("kind", X.SSIM_EDGES)
def test_psnr_ssim_degenerate_images(kind):
    """identical images: PSNR +inf and SSIM 1; a constant target: -inf; constant and identical: NaN -- as the fp32 formula gives"""
    a, b = X.image_operands(X.EDGE_SHAPE, kind)
    mm, sse, parts, out = image_call(a, b)
    what = f"psnr_ssim {kind}"
    check_stats_phase(a, b, mm, sse, what)
    if kind == "identical":
        assert float(out[0]) == float("inf"), what
        assert abs(float(out[1]) - 1.0) <= 2.0 ** -23, f"{what}: ssim {float(out[1])!r}"
    elif kind == "constant-target":
        assert float(out[0]) == float("-inf"), what
        assert math.isfinite(float(out[1])), what
    else:
        assert math.isnan(float(out[0])) and math.isnan(float(out[1])), what


# ------------------------------------------------------------------ best-of-n SSIM
@pytest.mark.parametrize("c", X.SS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_sample_ssim_phase_by_phase(c):
    p, t = X.ss_operands(c)
    nbytes = int(lib().ipoke_sample_ssim_workspace_bytes(*c))
    ty, tx = X.ssim_tiles(c.H, c.W)
    tiles, planes, off = ty * tx, c.ns * c.s * c.C, X.ss_offsets(c.bs)
    assert nbytes == off + 8 * c.bs * planes * tiles
    ww, wb = flat(nbytes, U8)
    pw, pb = flat(p.numel(), F32, p)
    tw, tb = flat(t.numel(), F32, t)
    ow, ob = flat(c.bs * c.ns * c.s)
    before = (pw.clone(), tw.clone())
    run(lib().ipoke_sample_ssim(ptr(pb), ptr(tb), c.bs, c.ns, c.s, c.C, c.H, c.W, ptr(wb), ptr(ob), stream()))
    what = f"sample_ssim {tuple(c)}"
    unchanged(pw, before[0], what + " pred")
    unchanged(tw, before[1], what + " target")
    check_fence(ww, 1, nbytes, nbytes, what + " workspace")
    check_fence(ow, 1, ob.numel(), ob.numel(), what + " out")
    mm = wb[: 16 * c.bs].view(F32).cpu().view(c.bs, 4)
    assert bool((host(wb[16 * c.bs: off]) == X.U8_SENT).all()), what + ": the gap between mm and the partials"
    parts = wb[off:].view(F64).cpu().view(c.bs, planes, tiles)
    for e in range(c.bs):
        pe, te = p[e].reshape(planes, c.H, c.W), t[e, 0].reshape(c.s * c.C, c.H, c.W)
        assert_same(mm[e], X.mm_ref(pe, te), f"{what}: mm of example {e}")
        sums, cnt = X.tile_sums(X.ssim_map_ref(pe, te.repeat(c.ns, 1, 1), X.range_of_mm(mm[e]).to(F64)))
        units("ssim_tile", parts[e], sums, cnt, F32, f"{what}: per-tile sums of example {e}")
    count = c.C * (c.H - 10) * (c.W - 10)
    frames = parts.reshape(c.bs * c.ns * c.s, c.C * tiles)
    ref = torch.tensor([math.fsum(r.tolist()) / count for r in frames], dtype=F64)
    one_ulp("sample_ssim", ob, ref, what + ": per-frame means from the stored partials")


def test_sample_ssim_refuses_too_many_planes():
    ww, wb = flat(1024, U8)
    pw, pb = flat(256)
    tw, tb = flat(256)
    ow, ob = flat(16)
    refused(lib().ipoke_sample_ssim(ptr(pb), ptr(tb), 1, 65536, 1, 1, 11, 11, ptr(wb), ptr(ob), stream()))
    for w in (ww, pw, tw, ow):
        untouched(w, "refused sample_ssim")


# ------------------------------------------------------------------ sample statistics
def stats_call(v):
    bs, ns, s = v.shape
    vw, vb = flat(v.numel(), F32, v)
    outs = [flat(bs * s) for _ in range(3)]
    iw, ib = flat(bs, I32)
    before = vw.clone()
    run(lib().ipoke_sample_stats(ptr(vb), bs, ns, s, ptr(outs[0][1]), ptr(outs[1][1]), ptr(outs[2][1]), ptr(ib), stream()))
    unchanged(vw, before, "sample_stats vals")
    for w, b in outs:
        check_fence(w, 1, bs * s, bs * s, "sample_stats output")
    check_fence(iw, 1, bs, bs, "sample_stats index")
    return outs[0][1], outs[1][1], outs[2][1], ib


@pytest.mark.parametrize("bs,ns,s", X.STATS_CASES)
def test_sample_stats(bs, ns, s):
    v = X.stats_operands(bs, ns, s)
    nn, sd, mean, idx = stats_call(v)
    ref = X.stats_ref(v)
    what = f"sample_stats {bs} x {ns} x {s}"
    assert torch.equal(idx.cpu(), ref["index"]), what + ": index"
    assert_same(nn, ref["nn"], what + ": nn is a copy")
    one_ulp("stats_mean", mean, ref["mean"].reshape(-1), what + ": mean")
    if ns == 1:
        assert bool(torch.isnan(sd).all()) and bool((idx == 0).all()), what + ": one sample"
    else:
        one_ulp("stats_sd", sd, ref["sd"].reshape(-1), what + ": sd")


def test_sample_stats_ties_go_to_the_first_and_means_compare_in_double():
    v = X.stats_tie_operands()
    nn, sd, mean, idx = stats_call(v)
    ref = X.stats_ref(v)
    assert idx.cpu().tolist() == [1, 1] == ref["index"].tolist()
    assert_same(nn, ref["nn"], "sample_stats ties: nn")


# ------------------------------------------------------------------ pairwise MSE
@pytest.mark.parametrize("integer", [True, False], ids=["integers", "reals"])
@pytest.mark.parametrize("c", X.PAIR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_pair_mse(c, integer):
    x = X.pair_operands(c, integer)
    nbytes = int(lib().ipoke_pair_mse_workspace_bytes(*c))
    xw, xb = flat(x.numel(), F32, x)
    ww, wb = flat(nbytes // 8, F64)
    dw, db = flat(c.n_ex * c.ns * c.ns)
    before = xw.clone()
    run(lib().ipoke_pair_mse(ptr(xb), c.n_ex, c.ns, c.L, ptr(wb), ptr(db), stream()))
    what = f"pair_mse {tuple(c)} {'integers' if integer else 'reals'}"
    ref = X.pair_mse_ref(x)
    D = db.view(c.n_ex, c.ns, c.ns)
    if integer:
        assert_same(D, ref, what)                                         # every sum of squares is exact: the correctly rounded quotient
    else:
        one_ulp("pair_mse", db, ref.reshape(-1), what)
    assert_same(D, D.transpose(1, 2).contiguous(), what + ": symmetry")
    diag = torch.diagonal(D, dim1=1, dim2=2).contiguous()
    assert_same(diag, torch.zeros_like(diag), what + ": the diagonal")
    check_fence(dw, 1, db.numel(), db.numel(), what + " D")
    check_fence(ww, 1, nbytes // 8, nbytes // 8, what + " workspace")
    unchanged(xw, before, what)


@pytest.mark.parametrize("ns", [1, 65])
def test_pair_mse_refuses_sample_counts_it_cannot_hold(ns):
    xw, xb = flat(ns * 4)
    ww, wb = flat(65 * 32, F64)
    dw, db = flat(ns * ns)
    refused(lib().ipoke_pair_mse(ptr(xb), 1, ns, 4, ptr(wb), ptr(db), stream()))
    for w in (xw, ww, dw):
        untouched(w, "refused pair_mse")


# ------------------------------------------------------------------ time cosine
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", X.TC_REG_CASES + X.TC_LDS_CASES + X.TC_TINY_CASES, ids=X.tc_id)
def test_time_cosine(c, dt):
    code, tdt, _ = DTYPES[dt]
    x = X.tc_operands(c, tdt)
    nbytes = int(lib().ipoke_time_cosine_workspace_bytes(c.ns, c.s, c.C, c.HW))
    assert nbytes > 0
    ld = c.C + 3
    xw, xb = fenced(c.ns * c.s * c.HW, ld, tdt, DEV, x.reshape(c.ns * c.s * c.HW, c.C))
    ww, wb = flat(nbytes // 8, F64)
    dw, db = flat(c.ns * c.ns)
    before = xw.clone()
    run(lib().ipoke_time_cosine(ptr(xb), ld, c.C, c.HW, c.ns, c.s, code, ptr(wb), ptr(db), stream()))
    what = f"time_cosine {X.tc_id(c)} {dt}"
    ref, mag = X.time_cosine_ref(x)
    D = db.view(c.ns, c.ns)
    units("time_cosine", D, ref, mag, F32, what)
    assert_same(D, D.t().contiguous(), what + ": symmetry")
    assert_same(torch.diagonal(D).contiguous(), torch.zeros(c.ns), what + ": the diagonal")
    check_fence(dw, 1, db.numel(), db.numel(), what + " D")
    check_fence(ww, 1, nbytes // 8, nbytes // 8, what + " workspace")
    unchanged(xw, before, what)


def test_time_cosine_refuses_a_tile_that_fits_no_lds():
    ns, s = X.TC_REFUSED
    xw, xb = flat(256)
    ww, wb = flat(256, F64)
    dw, db = flat(ns * ns)
    refused(lib().ipoke_time_cosine(ptr(xb), 1, 1, 1, ns, s, _lib.F32, ptr(wb), ptr(db), stream()))
    for w in (xw, ww, dw):
        untouched(w, "refused time_cosine")


# ------------------------------------------------------------------ uint8 export
@pytest.mark.parametrize("name,H,W,xo,yo", [("vector", 8, 8, 0, 0), ("scalar-hw63", 7, 9, 0, 0), ("scalar-x-offset", 8, 8, 1, 0),
                                            ("scalar-y-offset", 8, 8, 0, 1)])
def test_video_to_u8(name, H, W, xo, yo):
    hw = H * W
    x = X.u8_operands(hw)
    n = x.numel()
    xw, xb = flat(n + 4)
    xb[xo: xo + n] = x.reshape(-1).to(DEV)
    yw, yb = flat(n + 4, U8)
    expect = yw.clone()
    expect[X.FENCE + yo: X.FENCE + yo + n] = X.u8_ref(x).reshape(-1).to(DEV)
    before = xw.clone()
    xp, yp = ctypes.c_void_p(xb.data_ptr() + 4 * xo), ctypes.c_void_p(yb.data_ptr() + yo)
    assert (xp.value % 16 == 0) == (xo == 0) and (yp.value % 4 == 0) == (yo == 0)
    run(lib().ipoke_video_to_u8(xp, yp, X.U8_FRAMES, H, W, stream()))
    bad = torch.nonzero(yw != expect).reshape(-1)
    assert bad.numel() == 0, f"video_to_u8 {name}: {bad.numel()} bytes differ, first at byte {int(bad[0]) - X.FENCE - yo} of y: " \
                             f"got {int(yw[bad[0]])}, expected {int(expect[bad[0]])}"
    unchanged(xw, before, f"video_to_u8 {name}")


# ------------------------------------------------------------------ VGG input normalisation
@pytest.mark.parametrize("N,H,W", X.VGG_SHAPES)
def test_vgg_normalize_is_the_fp32_expression(N, H, W):
    x = X.vgg_operands(N, H, W)
    xw, xb = flat(x.numel(), F32, x)
    yw, yb = flat(x.numel())
    before = xw.clone()
    run(lib().ipoke_vgg_normalize(ptr(xb), ptr(yb), N, H, W, stream()))
    assert_same(yb, eval_ref.normalize_input_vgg(x), f"vgg_normalize {N} x 3 x {H} x {W}", lambda i: f"channel {i // (H * W) % 3} element {i}")
    check_fence(yw, 1, x.numel(), x.numel(), "vgg_normalize")
    unchanged(xw, before, "vgg_normalize")
