"""The references of tests/eval_exact.py pinned without a GPU against the reference-named functions they stand for (F.interpolate,
fvd_ref.pool_same and the I3D head's pooling, np.mean / np.cov, metrics_ref.psnr / ssim, eval_ref's test-loop reductions, numpy's uint8
cast); the conditions the case tables must meet for a green GPU test to mean something (tile counts, block counts, the LDS tile width
each time-cosine case takes, ties, ranges, zero and tiny locations); and the recorded fp32 yardsticks."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fvd_ref, metrics_ref
from tests import eval_exact as X
from tests import eval_ref
from tests.eval_exact import BF16, DTYPES, F32, F64, YARDSTICK, err_units, restate


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------ resize
@pytest.mark.parametrize("c", X.RESIZE_CASES, ids=lambda c: c.name)
def test_resize_ref_is_f_interpolate(c):
    x = X.resize_operands(c).reshape(-1, c.C, c.Hi, c.Wi)
    ref, mag = X.resize_ref(x, c.Ho, c.Wo)
    aten = F.interpolate(x.to(F32), size=(c.Ho, c.Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    if c.exact:
        for n_in, n_out in ((c.Hi, c.Ho), (c.Wi, c.Wo)):
            lam = X.src_index(n_in, n_out)[2]
            assert bool((lam * 2 == (lam * 2).round()).all())                           # dyadic weights: every product and sum is exact
        assert bool((x == x.round()).all()) and float(x.abs().max()) <= 8 and bool((x < 0).any())
        assert torch.equal(aten.to(F64), ref) and torch.equal(restate(X.resize_ref, x, c.Ho, c.Wo)[0].to(F64), ref)
    else:
        assert err_units(aten, ref, mag) <= 4.0
        assert not torch.equal(aten.to(F64), ref)


def test_resize_operand_families_and_pads():
    c = X.RESIZE_CASES[0]
    assert float(X.resize_operands(c, "pos").min()) > 0 and float(X.resize_operands(c, "neg").max()) < 0
    nz, pz = X.resize_operands(c, "nzero"), X.resize_operands(c, "pzero")
    assert bool(torch.signbit(nz).all()) and not bool(torch.signbit(pz).any()) and not bool(nz.any()) and not bool(pz.any())
    # the blend of -0.0 pixels is -0.0 (IEEE: a zero weight times -0.0 is -0.0 too)
    assert bool(torch.signbit(restate(X.resize_ref, nz.reshape(-1, c.C, c.Hi, c.Wi), c.Ho, c.Wo)[0]).all())
    assert X.stem_pads(23) == (2, 4) and X.stem_pads(10) == (2, 3) and X.stem_pads(224) == (2, 3)
    assert {X.resize_pads(k) for k in X.RESIZE_CASES} >= {(0, 0), (2, 3), (2, 4)}
    assert {k.layout for k in X.RESIZE_CASES} == {"contig", "perm", "slice"} and {k.C for k in X.RESIZE_CASES} == {1, 3}
    assert torch.equal(X.denorm_ref(torch.tensor([-1.0, 0.5], dtype=F32)), torch.tensor([0.0, 0.75]))


# ------------------------------------------------------------------ max pooling
@pytest.mark.parametrize("k,s,dhw", X.POOL_GEOMS, ids=lambda v: "x".join(map(str, v)))
def test_pool_ref_is_the_oracles_pool_same(k, s, dhw):
    x = X.pool_operands(24, dhw, BF16)
    ref = X.pool_ref(x, k, s)
    assert torch.equal(ref, fvd_ref.pool_same(x, k, s))
    dims, odhw = X.pool_dims(X.POOL_N, 24, dhw, k, s)
    assert tuple(ref.shape[2:]) == odhw and len(dims) == 20
    neg = X.pool_operands(24, dhw, F32, negative=True)
    assert float(neg.max()) < 0
    out = X.pool_ref(neg, k, s)
    assert bool((out == 0).any()) == (sum(sum(X.fvd._same(e, kk, ss, i == 0)) for i, (e, kk, ss) in enumerate(zip(dhw, k, s))) > 0)



def test_pool_cases_hold_what_the_gpu_file_claims():
    for g in (X.POOL_GEOMS[2], X.POOL_GEOMS[5]):                          # the all-negative cases: border windows 0, interior ones negative
        out = X.pool_ref(X.pool_operands(24, g[2], F32, negative=True), g[0], g[1])
        assert bool((out == 0).any()) and bool((out < 0).any())
    k, s, dhw = X.POOL_GEOMS[2]
    dims, odhw = X.pool_dims(2, 8, dhw, k, s)
    assert odhw[2] * s[2] - dims[16] >= dims[19]                          # one more window along W starts beyond the padded extent
    assert {(dt, C) for dt, C in X.POOL_CHANNELS} >= {("bf16", 8), ("f32", 4)} and 12 % DTYPES["bf16"][2] != 0


# ------------------------------------------------------------------ weighted row pooling
@pytest.mark.parametrize("Tf", [2, 3])
def test_trunk_weights_are_the_heads_average_pool_and_time_mean(Tf):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(3, 6, Tf, 7, 7, generator=gen, dtype=F64)
    want = F.avg_pool3d(x, (2, 7, 7), (1, 1, 1)).squeeze(3).squeeze(3).mean(2)
    rows = x.permute(0, 2, 3, 4, 1).reshape(3 * Tf * 49, 6)
    got, _ = X.pool_rows_ref(rows, X.trunk_weights(Tf * 49).to(F64), 3)
    close(got, want, 1e-6)                                                # the weights are fp32
    assert {c.S for c in X.ROWS_CASES} == {1, 98, 147} and {c.C for c in X.ROWS_CASES} == {5, 1024} and {c.G for c in X.ROWS_CASES} == {1, 3}


def test_cancelling_weights_cancel():
    for c in X.ROWS_CASES[1:]:
        x, w = X.rows_operands(c, F32, "cancel")
        assert bool((w[0::2] > 0).all()) and bool((w[1::2] < 0).all())
        ref, mag = X.pool_rows_ref(x, w, c.G)
        assert float((ref.abs() / mag).median()) < 0.2


# ------------------------------------------------------------------ activation moments
@pytest.mark.parametrize("c", X.MOM_CASES, ids=lambda c: c.name)
def test_moments_refs_are_numpy_mean_and_cov(c):
    a = X.mom_operands(c)
    valid, mu, _ = X.moments_mean_ref(a)
    sigma, _ = X.moments_cov_ref(a, mu)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        wmu, wsig = fvd_ref.moments(a.numpy())
        wsig = np.asarray(wsig).reshape(c.D, c.D)
    assert valid.tolist() == [r not in c.nan_rows for r in range(c.n)]
    for got, want in ((mu, wmu), (sigma, wsig)):
        got = got.astype(np.float64)
        assert (np.isnan(got) == np.isnan(want)).all()
        fin = ~np.isnan(want)
        assert np.allclose(got[fin], want[fin], rtol=1e-9 if c.shift else 1e-11, atol=1e-9 if c.shift else 1e-12)
    if c.name == "d65":                                                   # NaN exactly in entry / row and column 3
        assert np.isnan(wmu).nonzero()[0].tolist() == [3] and (np.isnan(wsig) == (np.arange(65)[:, None] == 3) | (np.arange(65)[None] == 3)).all()
    if c.name in ("one-valid", "none-valid"):
        assert np.isnan(wsig).all() and np.isnan(wmu).all() == (c.name == "none-valid")
    if c.name == "shifted":
        assert float(a.mean()) > 9e3 and float(a.std(0).max()) < 3


def test_moments_cases_reach_their_blocks():
    assert {c.D for c in X.MOM_CASES} >= {1, 65, 400} and {c.n for c in X.MOM_CASES} >= {2, 37, 300}
    assert X.moments_bound(37) == 39 * 2.0 ** -53


# ------------------------------------------------------------------ PSNR / SSIM
@pytest.mark.parametrize("kind", X.SSIM_RANGES)
@pytest.mark.parametrize("shape", X.SSIM_SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_image_refs_are_the_restated_lightning_metrics(shape, kind):
    a, b = X.image_operands(shape, kind)
    mm = X.mm_ref(a, b)
    assert abs(float(X.psnr_ref(mm, X.sse_ref(a, b), a.numel())) - float(metrics_ref.psnr(a.to(F32)[None], b.to(F32)[None]))) <= 1e-5
    rng = max(a.max() - a.min(), b.max() - b.min())
    m = X.ssim_map_ref(a, b, rng)
    close(m, eval_ref.ssim_map(a[None], b[None])[0], 1e-10)
    assert abs(float(m.mean()) - float(metrics_ref.ssim(a[None], b[None]))) <= 1e-10
    sums, cnt = X.tile_sums(m)
    assert abs(float(sums.sum()) - float(m.sum())) <= 1e-9 and float(cnt.sum()) == m.numel()
    ra, rb = float(a.max() - a.min()), float(b.max() - b.min())
    assert (ra > rb) == (kind == "sym-preds") and ra != rb
    assert (float(a.min()) < 0) == (kind == "sym-preds")


def test_ssim_shapes_reach_their_tiles():
    want = {(1, 11, 11): (1, 1), (2, 42, 42): (1, 1), (3, 43, 75): (2, 3), (2, 74, 42): (2, 1), (300, 11, 12): (1, 1)}
    for shape in X.SSIM_SHAPES:
        assert X.ssim_tiles(*shape[1:]) == want[shape]
        nbytes = int(X._lib.lib().ipoke_image_metrics_workspace_bytes(*shape))
        assert nbytes == 64 + 8 * (shape[0] * math.prod(want[shape]) + 1)
    _, cnt = X.tile_sums(torch.zeros(1, 33, 65, dtype=F64))
    assert cnt.reshape(2, 3).tolist() == [[1024.0, 1024.0, 32.0], [32.0, 32.0, 1.0]]           # a 1-row and a 1-column ragged tile
    assert X.tile_sums(torch.zeros(1, 1, 1, dtype=F64))[1].item() == 1 and X.tile_sums(torch.zeros(1, 32, 32, dtype=F64))[1].item() == 1024
    assert X.SSIM_SHAPES[-1][0] > 256


def test_mm_edges_and_degenerate_images_follow_the_fp32_formula():
    for kind in X.MM_EDGES:
        a, b = X.image_operands(X.EDGE_SHAPE, kind)
        mm = X.mm_ref(a, b)
        if kind == "all-negative":
            assert float(a.max()) < 0 and float(b.max()) < 0 and bool((mm[[0, 2]] > 0).all()) and bool((mm[[1, 3]] < 0).all())
        elif kind == "pzero-darkest":
            assert X.bits32(mm)[[0, 2]].tolist() == [-2 ** 31, -2 ** 31]                        # -min = -0.0
        elif kind == "nzero-darkest":
            assert X.bits32(mm)[[0, 2]].tolist() == [0, 0] and bool(torch.signbit(a.min()))
        else:
            assert float(mm[0]) == -float(mm[1]) and float(mm[2]) == -float(mm[3])
    a, b = [t.to(F32)[None] for t in X.image_operands(X.EDGE_SHAPE, "identical")]
    assert float(metrics_ref.psnr(a, b)) == float("inf") and abs(float(metrics_ref.ssim(a, b)) - 1.0) <= 2.0 ** -23
    a, b = [t.to(F32)[None] for t in X.image_operands(X.EDGE_SHAPE, "constant-target")]
    assert float(metrics_ref.psnr(a, b)) == float("-inf") and math.isfinite(float(metrics_ref.ssim(a, b)))
    a, b = [t.to(F32)[None] for t in X.image_operands(X.EDGE_SHAPE, "constant-identical")]
    assert math.isnan(float(metrics_ref.psnr(a, b))) and math.isnan(float(metrics_ref.ssim(a, b)))


# ------------------------------------------------------------------ best-of-n SSIM
@pytest.mark.parametrize("c", X.SS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_sample_ssim_operands_and_reference(c):
    p, t = X.ss_operands(c)
    planes = c.ns * c.s * c.C
    vals = []
    for e in range(c.bs):
        pe, te = p[e].reshape(planes, c.H, c.W), t[e, 0].reshape(c.s * c.C, c.H, c.W)
        rng = max(pe.max() - pe.min(), te.max() - te.min())
        m = X.ssim_map_ref(pe, te.repeat(c.ns, 1, 1), rng)
        vals.append(m.reshape(c.ns, c.s, -1).mean(2))
        rp, rt = float(pe.max() - pe.min()), float(te.max() - te.min())
        assert (rp > rt, rp < rt, rp == rt) == (e == 0, e == 1, e == 2)
    close(torch.stack(vals), eval_ref.sample_ssim(p, t), 1e-10)
    flat = t.reshape(-1, c.H * c.W)
    assert len({tuple(r.tolist()) for r in flat}) == flat.shape[0]                               # every target plane is distinct
    assert X.ss_offsets(3) == 64 and X.ss_offsets(4) == 64 and X.ss_offsets(5) == 128
    assert int(X._lib.lib().ipoke_sample_ssim_workspace_bytes(*c)) == 64 + 8 * c.bs * planes * math.prod(X.ssim_tiles(c.H, c.W))


def test_sample_ssim_cases_cover_the_listed_sizes():
    assert {c.ns for c in X.SS_CASES} == {1, 3} and {c.s for c in X.SS_CASES} == {1, 2} and {c.C for c in X.SS_CASES} == {1, 3}
    assert {(c.H, c.W) for c in X.SS_CASES} == {(11, 11), (43, 44)} and all(c.bs == 3 for c in X.SS_CASES)
    assert X.ssim_tiles(43, 44) == (2, 2)


# ------------------------------------------------------------------ sample statistics
@pytest.mark.parametrize("bs,ns,s", X.STATS_CASES)
def test_stats_ref_is_the_test_loops_reduction(bs, ns, s):
    v = X.stats_operands(bs, ns, s)
    ref = X.stats_ref(v)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nn, sd, mean, idx = eval_ref.sample_stats(v)
    assert torch.equal(nn, ref["nn"]) and torch.equal(idx.to(torch.int32), ref["index"])
    close(mean, ref["mean"])
    if ns > 1:
        close(sd, ref["sd"])
    else:
        assert bool(torch.isnan(sd).all()) and bool(torch.isnan(ref["sd"]).all())


def test_stats_ties():
    v = X.stats_tie_operands()
    assert torch.equal(v[0, 1], v[0, 3]) and X.stats_ref(v)["index"].tolist() == [1, 1]
    m32, m64 = v[1].to(F32).mean(1), v[1].mean(1)
    assert float(m32[0]) == float(m32[1]) and float(m64[1]) < float(m64[0])                   # equal in fp32, not in double
    assert int(torch.argmin(m32)) == 0 and int(torch.argmin(m64)) == 1
    assert {ns for _, ns, _ in X.STATS_CASES} >= {1, 2, 65} and {s for _, _, s in X.STATS_CASES} >= {1, 65}


# ------------------------------------------------------------------ pairwise MSE
@pytest.mark.parametrize("c", X.PAIR_CASES[:4], ids=lambda c: "-".join(map(str, c)))
def test_pair_mse_ref(c):
    x = X.pair_operands(c, False)
    close(X.pair_mse_ref(x), eval_ref.pair_mse(x.reshape(c.n_ex, c.ns, c.L, 1)))
    i = X.pair_operands(c, True)
    assert bool((i == i.round()).all()) and float(i.abs().max()) <= 16 and 32 * 32 * c.L < 2 ** 53


def test_pair_mse_cases_reach_their_slots_and_blocks():
    pairs = {c.ns: c.ns * (c.ns - 1) // 2 for c in X.PAIR_CASES}
    assert pairs[23] == 253 and pairs[24] == 276 and pairs[64] == 2016 and 7 * 256 < 2016 <= 8 * 256
    assert {c.L for c in X.PAIR_CASES} >= {1, 63, 64, 65}
    big = X.PAIR_CASES[-1]
    assert big.n_ex == 700 and X.pair_blocks(big) == 2 < -(-big.L // 64)                      # the grid-stride loop takes a second trip
    for c in X.PAIR_CASES[:-1]:
        assert X.pair_blocks(c) == -(-c.L // 64)


# ------------------------------------------------------------------ time cosine
def test_time_cosine_ref_is_the_test_loops_cosine():
    c = X.TcCase(3, 4, 6, 5, "relu")
    x = X.tc_operands(c, F32)
    fmap = x.reshape(c.ns * c.s, c.HW, c.C).permute(0, 2, 1).reshape(c.ns * c.s, c.C, c.HW, 1)
    close(X.time_cosine_ref(x)[0], eval_ref.time_cosine(fmap, c.ns, c.s, dtype=F64), 1e-9)


def test_time_cosine_cases_reach_every_path():
    assert {(c.ns, c.s) for c in X.TC_REG_CASES} == {(ns, s) for ns in range(2, 9) for s in (1, 15, 16)}
    assert {c.HW * c.C for c in X.TC_REG_CASES} == {72, 1000}
    for c in X.TC_REG_CASES:
        assert X.tc_blocks(c.ns, c.s, c.C, c.HW) == -(-c.HW * c.C // 256)                      # the register path: 256 locations a block
    widths = []
    for c in X.TC_LDS_CASES:
        L, blocks = c.HW * c.C, X.tc_blocks(c.ns, c.s, c.C, c.HW)
        assert blocks < 1024
        loc = [w for w in (64, 32, 16, 8, 4) if -(-L // w) == blocks]
        assert len(loc) == 1 and c.ns * (c.s * loc[0] + 1) * 4 <= 65536 and (loc[0] == 64 or c.ns * (c.s * 2 * loc[0] + 1) * 4 > 65536)
        widths.append(loc[0])
    assert widths == X.TC_LDS_WIDTHS and set(widths) == {64, 32, 16, 8, 4}
    ns, s = X.TC_REFUSED
    assert X.tc_blocks(ns, s, 25, 40) == 1000 and ns * (s * 4 + 1) * 4 > 65536                 # no tile width fits: one location a unit
    assert all(72 % w and 1000 % w for w in (256, 64, 32, 16))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_time_cosine_families_hold_their_edges(dt):
    tdt = DTYPES[dt][1]
    x = X.tc_operands(X.TC_LDS_CASES[0], tdt)
    assert bool((x[:, :, 0::5] == 0).all()) and bool((x >= 0).all())
    assert bool((x[0, :, 7] == 0).all()) and bool((x[1:, :, 7] != 0).any())
    for c in X.TC_TINY_CASES:
        x = X.tc_operands(c, tdt)
        assert c.s == 2 and float((x * x).min()) > 2.0 ** -126                                 # no square is subnormal
        n = torch.sqrt((x * x).sum(1))
        assert 5e-16 < float(n[:, 0::2].min()) and float(n[:, 0::2].max()) < 1e-14
        u = n / (n + X.E1)
        assert float(u[:, 0::2].min()) > 1e-6 and bool((u[:, 1::2] < X.E2).any())             # the + 1e-10 and the max(., 1e-8) branches
        D, mag = X.time_cosine_ref(x)
        assert bool(torch.isfinite(D).all()) and float(mag.max()) > 0


# ------------------------------------------------------------------ uint8 export, VGG normalisation
def test_u8_lattice_and_reference():
    lat = X.u8_lattice()
    assert lat.numel() == 776
    inr = lat[:768]
    x = inr.reshape(1, 1, 3, 16, 16).clone()
    with np.errstate(all="ignore"):
        plain = ((inr.numpy() + 1.) * 127.5).astype(np.uint8)
    assert plain.dtype == np.uint8 and (X.u8_ref(inr.reshape(1, 3, 256)).permute(0, 2, 1).reshape(-1).numpy() == plain).all()
    assert (eval_ref.video_to_uint8(x).reshape(-1) == X.u8_ref(x.reshape(1, 3, 256)).reshape(-1).numpy()).all()
    exact = np.floor(np.clip((inr.numpy().astype(np.float64) + 1.0) * 127.5, 0, 255)).astype(np.uint8)       # one rounding, as a fused multiply-add
    assert int((exact != plain).sum()) > 0                                                     # ... truncates differently somewhere on the lattice
    assert set(plain.tolist()) == set(range(256))
    tail = X.u8_ref(lat[768:].reshape(1, 1, 8).repeat(1, 3, 1))[0, :, 0].tolist()
    assert tail == [0, 255, 0, 255, 255, 0, 255, 0]
    for hw in (63, 64):
        assert X.u8_operands(hw).numel() >= 776


def test_vgg_constants_differ_per_channel():
    y = eval_ref.normalize_input_vgg(torch.zeros(1, 3, 2, 2))
    assert len({float(y[0, c, 0, 0]) for c in range(3)}) == 3
    assert (5 * 7 * 3 * 2) % 256 != 0


# ------------------------------------------------------------------ the yardsticks
@functools.lru_cache(maxsize=None)
def resize_errors():
    worst = 0.0
    for c in X.RESIZE_CASES:
        if not c.exact:
            x = X.resize_operands(c).reshape(-1, c.C, c.Hi, c.Wi)
            ref, mag = X.resize_ref(x, c.Ho, c.Wo)
            worst = max(worst, err_units(restate(X.resize_ref, x, c.Ho, c.Wo)[0], ref, mag))
    return dict(resize=worst)


@functools.lru_cache(maxsize=None)
def pool_rows_errors():
    worst = 0.0
    for c in X.ROWS_CASES:
        for dt in ("f32", "bf16"):
            for weights in X.ROWS_WEIGHTS:
                x, w = X.rows_operands(c, DTYPES[dt][1], weights)
                ref, mag = X.pool_rows_ref(x, w, c.G)
                worst = max(worst, err_units(restate(X.pool_rows_ref, x, w, c.G)[0], ref, mag))
    return dict(pool_rows=worst)


def ssim_tile_error(a, b, mm):
    rng = X.range_of_mm(mm).to(F64)
    sums, cnt = X.tile_sums(X.ssim_map_ref(a, b, rng))
    got, _ = X.tile_sums(restate(X.ssim_map_ref, a, b, rng).to(F64))                          # an fp32 map summed in double, as the kernel's
    return err_units(got, sums, cnt)


@functools.lru_cache(maxsize=None)
def ssim_tile_errors():
    worst = 0.0
    for shape in X.SSIM_SHAPES:
        for kind in X.SSIM_RANGES:
            a, b = X.image_operands(shape, kind)
            worst = max(worst, ssim_tile_error(a, b, X.mm_ref(a, b)))
    for c in X.SS_CASES:
        p, t = X.ss_operands(c)
        for e in range(c.bs):
            pe, te = p[e].reshape(-1, c.H, c.W), t[e, 0].reshape(-1, c.H, c.W)
            worst = max(worst, ssim_tile_error(pe, te.repeat(c.ns, 1, 1), X.mm_ref(pe, te)))
    return dict(ssim_tile=worst)


@functools.lru_cache(maxsize=None)
def time_cosine_errors():
    worst = 0.0
    for c in X.TC_REG_CASES + X.TC_LDS_CASES + X.TC_TINY_CASES:
        for dt in ("f32", "bf16"):
            x = X.tc_operands(c, DTYPES[dt][1])
            ref, mag = X.time_cosine_ref(x)
            worst = max(worst, err_units(restate(X.time_cosine_ref, x)[0], ref, mag))
    return dict(time_cosine=worst)


MEASURES = [resize_errors, pool_rows_errors, ssim_tile_errors, time_cosine_errors]


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
