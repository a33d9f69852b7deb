"""The optimizer step and the weight-shadow refresh, bit-exact against tests/optim_exact.py: every Adam-amsgrad kernel (linear, per
segment, fused with the conv2 operand as a cast or as 64 x 64 tiles), the weight-norm row statistics and backward, the relayout into the
matrix-core operands and the multi-tensor row reductions, each with sentinels around every range, job and destination -- and one native
piecewise train step of a mid-size flow, whose parameters, moments and whole shadow buffer must equal the emulation applied to the
state before the step and the gradients it used."""
import ctypes

import pytest
import torch

from ipoke_amd import _lib, configs
from ipoke_amd._lib import ptr
from tests import optim_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": (_lib.BF16, torch.bfloat16, 2), "f32": (_lib.F32, torch.float32, 4)}
LR, B1, B2, EPS, WD, GS = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5


def lib():
    return _lib.lib()


def stream():
    return _lib.current_stream()


def embed(x, pad, fill=X.SENT):
    """x (CPU float32) in the middle of a sentinel-filled buffer: pad elements before and after"""
    out = torch.full((x.numel() + 2 * pad,), fill, dtype=torch.float32)
    out[pad:pad + x.numel()] = x
    return out


def hyper_args(h):
    return [ctypes.c_float(a) if isinstance(a, float) else a for a in h.args]


# ------------------------------------------------------------------ linear update: ipoke_adam_amsgrad_step / _step_grid
STEPS = [(1, 1e-3), (2, 3e-3), (3, 5e-4), (2000, 2e-4)]     # three steps with carried state, then a late step


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4097, (1 << 20) + 5])
def test_adam_step_linear(n):
    gen = torch.Generator().manual_seed(100 + n % 1000)
    pad = 64
    p, g, m, v, vx = X.adam_state(n, gen)
    grads = [g * s for s in (1.0, -0.5, 2.0, -1.0)]
    # the emulation once per length; every grid must give the same bits
    e = [t.double() for t in (p, m, v, vx)]
    expect = []
    for (step, lr), gg in zip(STEPS, grads):
        e = list(X.adam_update(e[0], gg.double(), e[1], e[2], e[3], X.Hyper(lr, B1, B2, EPS, WD, step, GS)))
        if step == 1 and n >= 5:          # every operand class present
            X.assert_class_reaches([t.double() for t in (p, gg, m, v, vx)], e)
        expect.append([embed(t.float(), pad) for t in e])
    where = X.locate_segments([("update", pad, n)])
    for mode in ("step", 1, 7, 128, 0):
        bufs = [embed(t, pad).to(DEV) for t in (p, m, v, vx)]
        for k, ((step, lr), gg) in enumerate(zip(STEPS, grads)):
            gd = embed(gg, pad).to(DEV)
            h = X.Hyper(lr, B1, B2, EPS, WD, step, GS)
            P = [ptr(b[pad:]) for b in bufs]
            if mode == "step":
                rc = lib().ipoke_adam_amsgrad_step(P[0], ptr(gd[pad:]), P[1], P[2], P[3], n, *hyper_args(h), stream())
            else:
                rc = lib().ipoke_adam_amsgrad_step_grid(P[0], ptr(gd[pad:]), P[1], P[2], P[3], n, *hyper_args(h), mode, stream())
            _lib.check(rc)
            torch.cuda.synchronize()
            for name, b, ex in zip(("p", "m", "v", "v_max"), bufs, expect[k]):
                X.assert_same(b.cpu(), ex, f"{name}, grid {mode}, step {step}", where)


# ------------------------------------------------------------------ ipoke_adam_amsgrad_segments
SEGS = [(3, 1), (9, 2), (17, 3), (30, 5), (41, 4095), (4141, 4097), (8243, 13), (8262, 20001), (28270, 6)]


@pytest.mark.parametrize("blocks", [2, 32])
def test_adam_segments(blocks):
    """offsets and lengths of every residue mod 4, seg_begin > 0, the last segment left out, begin / end cutting the first and the
    last segment of the launch; one segment long enough for the four-group loop of a 2-workgroup grid"""
    n = 28300
    gen = torch.Generator().manual_seed(200 + blocks)
    p, g, m, v, vx = X.adam_state(n, gen)
    seg_begin, nsegs = 1, 7
    begin, end = 10, 8262 + 20001 - 5
    h = X.Hyper(LR, B1, B2, EPS, WD, 3, GS)
    mask = torch.zeros(n, dtype=torch.bool)
    for off, ln in SEGS[seg_begin:seg_begin + nsegs]:
        mask[max(off, begin):min(off + ln, end)] = True
    new = X.adam_update(*(t.double() for t in (p, g, m, v, vx)), h)
    X.assert_class_reaches([t.double() for t in (p, g, m, v, vx)], new)
    expect = [torch.where(mask, a.float(), b) for a, b in zip(new, (p, m, v, vx))]
    table = X.to_device([X.AdamSeg(o, ln) for o, ln in SEGS], DEV)
    bufs = [t.to(DEV) for t in (p, m, v, vx)]
    gd = g.to(DEV)
    _lib.check(lib().ipoke_adam_amsgrad_segments(ptr(bufs[0]), ptr(gd), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ptr(table), seg_begin,
                                                 nsegs, begin, end, *hyper_args(h), blocks, stream()))
    torch.cuda.synchronize()
    where = X.locate_segments([(f"segment {i}", o, ln) for i, (o, ln) in enumerate(SEGS)])
    for name, b, ex in zip(("p", "m", "v", "v_max"), bufs, expect):
        X.assert_same(b.cpu(), ex, name, where)
    assert torch.equal(gd.cpu(), g)


# ------------------------------------------------------------------ ipoke_adam_amsgrad_cast_tiles / _shadow_tiles
TILE_SHAPES = [(64, 64), (128, 192), (512, 2048), (64, 128)]


def _tile_case():
    specs, off, dst = [], 12, 64
    for N, K in TILE_SHAPES:
        specs.append((off, dst, dst + N * K + 64, N, K))
        off += N * K + 8
        dst += 2 * (N * K + 64)
    jobs, ntot = X.adam_tile_table(specs)
    return jobs, ntot, off + 12, dst + 64


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["cast", "shadow"])
@pytest.mark.parametrize("max_blocks", [7, 64])
def test_adam_tiles(dtype, kind, max_blocks):
    """tile_begin inside the second tensor, the last tile left out, grids well below the 261 tiles so that workgroups get both odd and
    even tile counts (the RA / RB loop of adam_shadow_tile_kernel leaves through both of its exits; adam_cast_kernel's chunk loop)"""
    dt, tdt, _ = DTYPES[dtype]
    gen = torch.Generator().manual_seed(300 + max_blocks)
    jobs, ntot, n, nsh = _tile_case()
    tile_begin, ntiles = 3, ntot - 3 - 1
    p, g, m, v, vx = X.adam_state(n, gen)
    h = X.Hyper(LR, B1, B2, EPS, WD, 2, GS)
    new = X.adam_update(*(t.double() for t in (p, g, m, v, vx)), h)
    X.assert_class_reaches([t.double() for t in (p, g, m, v, vx)], new)
    mask = torch.zeros(n, dtype=torch.bool)
    sh_exp = torch.full((nsh,), X.SENT, dtype=torch.float64)
    for j in jobs:
        N, K = j.N, j.K
        tiles = (N // 64) * (K // 64)
        for lt in range(tiles):
            t = j.tile_start + lt
            if not (tile_begin <= t < tile_begin + ntiles):
                continue
            if kind == "cast":          # chunk = 4096 consecutive elements
                sl = slice(j.src_off + lt * 4096, j.src_off + (lt + 1) * 4096)
                mask[sl] = True
                sh_exp[j.dstA + lt * 4096:j.dstA + (lt + 1) * 4096] = new[0][sl]
            else:
                n0, k0 = (lt // (K // 64)) * 64, (lt % (K // 64)) * 64
                idx = j.src_off + (torch.arange(n0, n0 + 64).view(-1, 1) * K + torch.arange(k0, k0 + 64).view(1, -1))
                mask[idx.reshape(-1)] = True
                sh_exp[(j.dstA + idx - j.src_off).reshape(-1)] = new[0][idx.reshape(-1)]
                nn, kk = torch.arange(n0, n0 + 64).view(-1, 1), torch.arange(k0, k0 + 64).view(1, -1)
                sh_exp[(j.dstB + kk * N + nn).reshape(-1)] = new[0][(j.src_off + nn * K + kk).reshape(-1)]
    expect = [torch.where(mask, a.float(), b) for a, b in zip(new, (p, m, v, vx))]
    table = X.to_device(jobs, DEV)
    bufs = [t.to(DEV) for t in (p, m, v, vx)]
    gd = g.to(DEV)
    shadow = torch.full((nsh,), X.SENT, dtype=tdt, device=DEV)
    fn = lib().ipoke_adam_amsgrad_cast_tiles if kind == "cast" else lib().ipoke_adam_amsgrad_shadow_tiles
    _lib.check(fn(ptr(bufs[0]), ptr(gd), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ptr(shadow), ptr(table), len(jobs), tile_begin, ntiles,
                  *hyper_args(h), max_blocks, dt, stream()))
    torch.cuda.synchronize()
    where = X.locate_segments([(f"tensor {i} ({j.N} x {j.K})", j.src_off, j.N * j.K) for i, j in enumerate(jobs)])
    for name, b, ex in zip(("p", "m", "v", "v_max"), bufs, expect):
        X.assert_same(b.cpu(), ex, name, where)
    swhere = X.locate_segments([(f"tensor {i} operand {op}", o, j.N * j.K) for i, j in enumerate(jobs)
                                for op, o in (("A", j.dstA), ("B", j.dstB))])
    X.assert_same(shadow.cpu(), sh_exp, f"{kind} shadow", swhere)


# ------------------------------------------------------------------ weight norm: ipoke_wn_scale_multi(_range), ipoke_wn_bwd_multi(_range)
WN_K = [1, 3, 6, 64, 160, 764, 768, 772, 1728, 2304]


def _wn_case(seed):
    """40 jobs (every K of WN_K at v_off = 0, 1, 2, 3 mod 4), 5..8 rows each, gains and directions apart in the flat buffer with sentinel
    gaps, per-job output rows apart by two sentinel rows"""
    gen = torch.Generator().manual_seed(seed)
    specs, vals, off, out = [], [], 16, 0
    for i, (K, mod) in enumerate((K, mod) for K in WN_K for mod in range(4)):
        rows = 5 + i % 4
        g_off = off
        v_off = g_off + rows + 3
        v_off += (mod - v_off) % 4
        specs.append((v_off, g_off, out, rows, K))
        v, _ = X.wn_rows(rows, K, gen)
        vals.append((X.wn_gains(rows, gen), v, torch.randint(-3, 4, (rows, K), generator=gen).float()))
        off = v_off + rows * K + 5
        out += rows + 2
    jobs, total_rows = X.wn_table(specs)
    n = off + 16
    params = torch.full((n,), X.SENT)
    grads = torch.full((n,), X.SENT)
    for j, (g, v, dw) in zip(jobs, vals):
        params[j.g_off:j.g_off + j.rows] = g
        params[j.v_off:j.v_off + j.rows * j.K] = v.reshape(-1)
        grads[j.v_off:j.v_off + j.rows * j.K] = dw.reshape(-1)
    return jobs, total_rows, out + 8, params, grads, vals


def _row_range(jobs, total_rows, ranged):
    """(job_begin, njobs, row_begin, nrows): everything, or jobs 5..30 from the third row of job 5 to the fourth of job 30"""
    if not ranged:
        return 0, len(jobs), 0, total_rows
    r0, r1 = jobs[5].row_start + 2, jobs[30].row_start + 3
    return 5, 26, r0, r1 - r0


@pytest.mark.parametrize("ranged", [False, True])
def test_wn_scale(ranged):
    jobs, total_rows, nout, params, _, vals = _wn_case(400)
    jb, nj, r0, nr = _row_range(jobs, total_rows, ranged)
    scale_e = torch.full((nout,), X.SENT, dtype=torch.float64)
    inv_e = scale_e.clone()
    for j, (g, v, _) in zip(jobs, vals):
        sc, inv = X.wn_scale_ref(v, g)
        for r in range(j.rows):
            if r0 <= j.row_start + r < r0 + nr:
                scale_e[j.out_off + r], inv_e[j.out_off + r] = sc[r], inv[r]
    X.assert_exactly_representable(scale_e, "scale")
    table = X.to_device(jobs, DEV)
    pd = params.to(DEV)
    scale, inv = (torch.full((nout,), X.SENT, device=DEV) for _ in range(2))
    if ranged:
        _lib.check(lib().ipoke_wn_scale_multi_range(ptr(pd), ptr(scale), ptr(inv), ptr(table), jb, nj, r0, nr, stream()))
    else:
        _lib.check(lib().ipoke_wn_scale_multi(ptr(pd), ptr(scale), ptr(inv), ptr(table), len(jobs), total_rows, stream()))
    torch.cuda.synchronize()
    X.assert_same(scale.cpu(), scale_e, "scale")
    X.assert_same(inv.cpu(), inv_e, "inv_norm")
    assert torch.equal(pd.cpu(), params)


@pytest.mark.parametrize("ranged", [False, True])
def test_wn_bwd(ranged):
    """K = 764 / 768 on the register path, 772 and up on the two-pass path, unaligned rows on the scalar path"""
    jobs, total_rows, nout, params, grads, vals = _wn_case(500)
    jb, nj, r0, nr = _row_range(jobs, total_rows, ranged)
    inv_buf = torch.full((nout,), X.SENT)
    expect = grads.double()
    for j, (g, v, dw) in zip(jobs, vals):
        _, inv = X.wn_scale_ref(v, g)
        inv_buf[j.out_off:j.out_off + j.rows] = inv.float()
        dg, dv = X.wn_bwd_ref(v, g, dw, inv)
        for r in range(j.rows):
            if r0 <= j.row_start + r < r0 + nr:
                expect[j.g_off + r] = dg[r]
                expect[j.v_off + r * j.K:j.v_off + (r + 1) * j.K] = dv[r]
    X.assert_exactly_representable(expect, "dg / dv")
    table = X.to_device(jobs, DEV)
    pd, gd, invd = params.to(DEV), grads.to(DEV), inv_buf.to(DEV)
    if ranged:
        _lib.check(lib().ipoke_wn_bwd_multi_range(ptr(pd), ptr(gd), ptr(invd), ptr(table), jb, nj, r0, nr, stream()))
    else:
        _lib.check(lib().ipoke_wn_bwd_multi(ptr(pd), ptr(gd), ptr(invd), ptr(table), len(jobs), total_rows, stream()))
    torch.cuda.synchronize()
    X.assert_same(gd.cpu(), expect, "grads (dv, dg)", X.locate_rows(jobs, "dv"))
    assert torch.equal(pd.cpu(), params)


# ---- on real rows (optim_exact.wn_real_case): float64 references, errors in ulps of the terms' magnitudes, bounds from the restatement
@pytest.mark.parametrize("ranged", [False, True])
def test_wn_scale_real(ranged):
    jobs, total_rows, nout, params, _, vals = X.wn_real_case(410)
    jb, nj, r0, nr = _row_range(jobs, total_rows, ranged)
    table = X.to_device(jobs, DEV)
    pd = params.to(DEV)
    scale, inv = (torch.full((nout,), X.SENT, device=DEV) for _ in range(2))
    if ranged:
        _lib.check(lib().ipoke_wn_scale_multi_range(ptr(pd), ptr(scale), ptr(inv), ptr(table), jb, nj, r0, nr, stream()))
    else:
        _lib.check(lib().ipoke_wn_scale_multi(ptr(pd), ptr(scale), ptr(inv), ptr(table), len(jobs), total_rows, stream()))
    torch.cuda.synchronize()
    scale, inv = scale.cpu(), inv.cpu()
    untouched = torch.ones(nout, dtype=torch.bool)
    worst = dict(scale=0.0, inv_norm=0.0)
    for j, (g, v, _) in zip(jobs, vals):
        sc_e, inv_e = X.wn_scale_ref(v, g)
        sel = torch.tensor([r0 <= j.row_start + r < r0 + nr for r in range(j.rows)])
        idx = j.out_off + torch.nonzero(sel).reshape(-1)
        untouched[idx] = False
        worst["scale"] = max(worst["scale"], X.units(scale[idx], sc_e[sel], sc_e[sel]))
        worst["inv_norm"] = max(worst["inv_norm"], X.units(inv[idx], inv_e[sel], inv_e[sel]))
    print(f"weight norm scale / inv_norm on real rows: worst {worst} units, bounds {X.wn_bound('scale')} / {X.wn_bound('inv_norm')}")
    assert worst["scale"] <= X.wn_bound("scale") and worst["inv_norm"] <= X.wn_bound("inv_norm"), worst
    assert bool((scale[untouched] == X.SENT).all()) and bool((inv[untouched] == X.SENT).all()), "store outside the rows of the range"
    assert torch.equal(pd.cpu(), params)


@pytest.mark.parametrize("ranged", [False, True])
def test_wn_bwd_real(ranged):
    """register path (K <= 768, aligned), two-pass path (up to 18432 = 2048 channels x 9 taps) and the scalar path; two runs on fresh
    copies of the gradient buffer must agree bit for bit (a row always takes the same path)"""
    jobs, total_rows, nout, params, grads, vals = X.wn_real_case(510)
    jb, nj, r0, nr = _row_range(jobs, total_rows, ranged)
    inv_buf = torch.full((nout,), X.SENT)
    for j, (g, v, dw) in zip(jobs, vals):
        inv_buf[j.out_off:j.out_off + j.rows] = X.wn_scale_ref(v, g)[1].float()
    table = X.to_device(jobs, DEV)
    pd, invd = params.to(DEV), inv_buf.to(DEV)
    outs = []
    for _ in range(2):
        gd = grads.to(DEV)
        if ranged:
            _lib.check(lib().ipoke_wn_bwd_multi_range(ptr(pd), ptr(gd), ptr(invd), ptr(table), jb, nj, r0, nr, stream()))
        else:
            _lib.check(lib().ipoke_wn_bwd_multi(ptr(pd), ptr(gd), ptr(invd), ptr(table), len(jobs), total_rows, stream()))
        torch.cuda.synchronize()
        outs.append(gd.cpu())
    got = outs[0]
    untouched = torch.ones(got.numel(), dtype=torch.bool)
    worst = dict(dg=0.0, dv=0.0)
    for j, (g, v, dw) in zip(jobs, vals):
        inv32 = inv_buf[j.out_off:j.out_off + j.rows]
        dg, dv = X.wn_bwd_ref(v, g, dw, inv32)
        mdg, mdv = X.wn_bwd_mags(v, g, dw, inv32)
        sel = torch.tensor([r0 <= j.row_start + r < r0 + nr for r in range(j.rows)])
        rows = torch.nonzero(sel).reshape(-1)
        untouched[j.g_off + rows] = False
        worst["dg"] = max(worst["dg"], X.units(got[j.g_off + rows], dg[sel], mdg[sel]))
        for r in rows.tolist():
            sl = slice(j.v_off + r * j.K, j.v_off + (r + 1) * j.K)
            worst["dv"] = max(worst["dv"], X.units(got[sl], dv[r], mdv[r]))
            untouched[sl] = False
    print(f"weight norm dg / dv on real rows: worst {worst} units, bounds {X.wn_bound('dg')} / {X.wn_bound('dv')}")
    assert worst["dg"] <= X.wn_bound("dg") and worst["dv"] <= X.wn_bound("dv"), worst
    assert torch.equal(got[untouched].view(torch.int32), grads[untouched].view(torch.int32)), "store outside the rows of the range"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ"
    assert torch.equal(pd.cpu(), params)


# ------------------------------------------------------------------ relayout: ipoke_relayout_multi(_range)
def _relayout_jobs():
    """(job, source element count): taps 9 / 6 / 1, strided sources both ways, the 16-byte 1 x 1 path with k_real % 4 != 0, a
    misaligned src_off, weight-norm scales and none, no B operand, fragment-tiled operands, real extents off the tile grid"""
    J = X.relayout_job
    return [
        (lambda s, d: J(s, 13 * 9, 9, 9, 40, 13, 0, d[0], 48, 16, d[1], 16, 48, 13), 40 * 13 * 9),            # [n][k][t], scaled
        (lambda s, d: J(s, 9 * 6, 6, 6, 36, 9, -1, d[0], 48, 16, d[1], 16, 48, 9, 1), 36 * 9 * 6),            # masked conv, tiled
        (lambda s, d: J(s, 6, 20 * 6, 6, 20, 11, 40, d[0], 24, 12, d[1], 12, 24, 11), 20 * 11 * 6),           # [k][n][t]: s_k > s_n
        (lambda s, d: J(s, 72, 1, 1, 100, 70, 60, d[0], 100, 72, d[1], 72, 100, 70), 100 * 72),               # 16-byte path, k 70
        (lambda s, d: J(s + 2, 64, 1, 1, 64, 64, -1, d[0], 64, 64, -1, 0, 0, 0), 64 * 64 + 2),                # src_off % 4 = 2, no B
        (lambda s, d: J(s, 1, 30, 1, 30, 50, -1, d[0], 32, 52, d[1], 52, 32, 50), 30 * 50),                   # [k][n]: s_k > s_n
        (lambda s, d: J(s, 40, 1, 1, 8, 40, 160, d[0], 16, 64, d[1], 16, 32, 16, 1), 8 * 40),                 # conv1x1 v: tiled, B rows 16 < k 40
    ]


def _relayout_case(seed):
    gen = torch.Generator().manual_seed(seed)
    jobs, src, dst = [], 8, 64
    for make, nsrc in _relayout_jobs():
        j = make(src, (0, 0))
        szA = j.A_rows_pad * j.taps * j.A_inner_pad
        szB = j.B_rows_pad * j.taps * j.B_inner_pad if j.dstB >= 0 else 0
        j = make(src, (dst, dst + X.round_up(szA, 64) + 64 if szB else -1))
        jobs.append(j)
        src += X.round_up(nsrc, 4) + 8
        dst += X.round_up(szA, 64) + 64 + (X.round_up(szB, 64) + 64 if szB else 0)
    jobs, nb, block_job = X.relayout_table(jobs)
    params = torch.full((src + 8,), X.SENT)
    live = torch.randn(src + 8, generator=gen)
    tie = torch.rand(src + 8, generator=gen) < 0.15            # exact bf16 ties among the sources
    live = torch.where(tie, ((live.view(torch.int32) & ~0xFFFF) | 0x8000).view(torch.float32), live)
    for j, (_, nsrc) in zip(jobs, _relayout_jobs()):
        base = j.src_off - (2 if j.src_off % 4 else 0)
        params[base:base + nsrc] = live[base:base + nsrc]
    scale = torch.randn(200, generator=gen)
    return jobs, nb, block_job, params, scale, dst + 64


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("variant", ["table", "search", "range"])
def test_relayout(dtype, variant):
    """the whole destination after one launch: the block -> job table, the binary search (block_job = NULL), or the blocks of jobs 2..5
    only (the others keep their sentinels)"""
    dt, tdt, esz = DTYPES[dtype]
    jobs, nb, block_job, params, scale, ndst = _relayout_case(600)
    b0, b1, sel = 0, nb, jobs
    if variant == "range":
        b0, b1, sel = jobs[2].block_start, jobs[6].block_start, jobs[2:6]
    expect = X.relayout_expect(sel, params, scale, torch.full((ndst,), X.SENT, dtype=torch.float64), esz)
    table = X.to_device(jobs, DEV)
    bj = torch.tensor(block_job, dtype=torch.int32, device=DEV)
    pd, sd = params.to(DEV), scale.to(DEV)
    dst = torch.full((ndst,), X.SENT, dtype=tdt, device=DEV)
    bjp = None if variant == "search" else ptr(bj)
    if variant == "range":
        _lib.check(lib().ipoke_relayout_multi_range(ptr(pd), ptr(dst), ptr(sd), ptr(table), len(jobs), b0, b1 - b0, bjp, dt, stream()))
    else:
        _lib.check(lib().ipoke_relayout_multi(ptr(pd), ptr(dst), ptr(sd), ptr(table), len(jobs), nb, bjp, dt, stream()))
    torch.cuda.synchronize()
    X.assert_same(dst.cpu(), expect, f"relayout ({variant})", X.locate_relayout(jobs, esz))


def test_relayout_grid_stride_above_100000_blocks():
    """one table of more than 102 400 blocks from block_begin = 0: the launch is capped at 65 536 workgroups and the grid-stride loop runs.  The
    large job is a 64 x 64 weight in a 102 400 x 4096 zero-padded bf16 operand (0.84 GB); the small jobs come first in the table."""
    jobs, _, _, params, scale, nsmall = _relayout_case(700)
    big_rows, big_ld = 102400, 4096
    big_src = params.numel()
    w = torch.randn(64 * 64, generator=torch.Generator().manual_seed(701))
    params = torch.cat([params, w, torch.full((8,), X.SENT)])
    big = X.relayout_job(big_src, 64, 1, 1, 64, 64, -1, nsmall, big_rows, big_ld, -1, 0, 0, 0)
    jobs, nb, block_job = X.relayout_table(jobs + [big])
    assert nb > 100000
    table = X.to_device(jobs, DEV)
    bj = torch.tensor(block_job, dtype=torch.int32, device=DEV)
    ndst = nsmall + big_rows * big_ld + 64
    dst = torch.full((ndst,), X.SENT, dtype=torch.bfloat16, device=DEV)
    pd, sd = params.to(DEV), scale.to(DEV)
    _lib.check(lib().ipoke_relayout_multi_range(ptr(pd), ptr(dst), ptr(sd), ptr(table), len(jobs), 0, nb, ptr(bj), _lib.BF16, stream()))
    torch.cuda.synchronize()
    small = X.relayout_expect(jobs[:-1], params, scale, torch.full((nsmall,), X.SENT, dtype=torch.float64), 2)
    X.assert_same(dst[:nsmall].cpu(), small, "small jobs", X.locate_relayout(jobs[:-1], 2))
    big_e = torch.zeros(big_rows, big_ld, dtype=torch.bfloat16, device=DEV)
    big_e[:64, :64] = w.view(64, 64).to(torch.bfloat16).to(DEV)
    X.assert_same(dst[nsmall:nsmall + big_rows * big_ld], big_e, "large job")
    assert bool((dst[nsmall + big_rows * big_ld:] == X.SENT).all())


# ------------------------------------------------------------------ ipoke_reduce_rows, ipoke_reduce_rows_multi
def test_reduce_rows():
    gen = torch.Generator().manual_seed(800)
    R, ncols, pad = 37, 333, 16
    src = torch.randint(-1000, 1001, (R, ncols), generator=gen).float()
    dst = torch.full((ncols + 2 * pad,), X.SENT, device=DEV)
    _lib.check(lib().ipoke_reduce_rows(ptr(src.to(DEV)), ptr(dst[pad:]), R, ncols, stream()))
    torch.cuda.synchronize()
    X.assert_same(dst.cpu(), embed(src.double().sum(0).float(), pad).double(), "reduce_rows")


def test_reduce_rows_multi():
    """rows = R * rmul of 3 (rmul = 0 counts as 1), 18, 21 (not multiples of 16: the tail loop), columns over several block widths"""
    gen = torch.Generator().manual_seed(801)
    R = 3
    specs = [(0, 40, 47), (6, 130, 130), (7, 300, 305), (1, 5, 9)]       # (rmul, ncols, ld)
    src_off, dst_off, entries = 4, 8, []
    for rmul, ncols, ld in specs:
        entries.append(X.ReduceEntry(src_off, dst_off, ld, ncols, rmul, 0))
        src_off += R * max(rmul, 1) * ld + 4
        dst_off += ncols + 8
    src = torch.randint(-1000, 1001, (src_off,), generator=gen).float()
    expect = torch.full((dst_off + 8,), X.SENT, dtype=torch.float64)
    for e in entries:
        rows = R * max(e.rmul, 1)
        blk = src[e.src:e.src + rows * e.ld].view(rows, e.ld)[:, :e.ncols]
        expect[e.dst:e.dst + e.ncols] = blk.double().sum(0)
    dst = torch.full((dst_off + 8,), X.SENT, device=DEV)
    table = X.to_device(entries, DEV)
    _lib.check(lib().ipoke_reduce_rows_multi(ptr(src.to(DEV)), ptr(dst), ptr(table), len(entries), R, stream()))
    torch.cuda.synchronize()
    X.assert_same(dst.cpu(), expect, "reduce_rows_multi", X.locate_segments([(f"entry {i}", e.dst, e.ncols) for i, e in enumerate(entries)]))


# ------------------------------------------------------------------ the engine
def _flow(dtype):
    from ipoke_amd.flow import SupervisedMacowTransformer
    from ipoke_amd.utils.detfill import deterministic_fill_
    arch = configs.flow_arch(32, hidden=192, num_steps=[2, 1, 1], factor=4)
    m = SupervisedMacowTransformer(arch, dtype=dtype, device=DEV, init="none", max_batch=4)
    deterministic_fill_(m, prefix="flow.")
    m.sync_buffers()
    return m, arch


def _carried_state(opt, n, seed):
    gen = torch.Generator().manual_seed(seed)
    mm = torch.randn(n, generator=gen) * 1e-3
    vv = torch.rand(n, generator=gen) * 1e-6
    vx = vv + (torch.rand(n, generator=gen) < 0.5) * torch.rand(n, generator=gen) * 1e-6      # v_max > v on half the elements
    for t, s in ((opt.exp_avg, mm), (opt.exp_avg_sq, vv), (opt.max_exp_avg_sq, vx)):
        t.copy_(s.to(DEV))


def _check_step(eng, opt, before, grads, h, shadow_before, what):
    """parameters and moments against the emulation over the whole buffer; the whole shadow buffer (weight-norm scales and inverse
    norms included) against what ipoke_flow_prepare_weights writes from the updated parameters over the shadow from before the step"""
    p0, m0, v0, x0 = (t.double() for t in before)
    expect = X.adam_update(p0, grads.cpu().double(), m0, v0, x0, h)
    names = [name for name, off, shape, kind in eng.tensors if kind == 0]
    offs = [off for name, off, shape, kind in eng.tensors if kind == 0]
    ends = offs[1:] + [eng.n_params]
    where = X.locate_segments(list(zip(names, offs, [e - o for o, e in zip(offs, ends)])))
    for name, got, ex in (("params", eng.params, expect[0]), ("exp_avg", opt.exp_avg, expect[1]), ("exp_avg_sq", opt.exp_avg_sq, expect[2]),
                          ("max_exp_avg_sq", opt.max_exp_avg_sq, expect[3])):
        X.assert_same(got.cpu(), ex, f"{what}: {name}", where)
    fresh = shadow_before.clone()
    _lib.check(lib().ipoke_flow_prepare_weights(eng.handle, ptr(eng.params), ptr(fresh), stream()))
    torch.cuda.synchronize()
    diff = torch.nonzero(fresh != eng.shadow)
    assert diff.numel() == 0, (f"{what}: {diff.numel()} shadow bytes differ from a full refresh, first at byte {int(diff[0])} "
                               f"(shadow base {eng.lib.ipoke_flow_shadow_base(eng.handle)})")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_flow_adam_range_over_the_piece_ranges(dtype):
    """ipoke_flow_adam_range (bf16: the conv2 cast kernel, c2_straight; f32: the 64 x 64-tile kernel with the transposed operand, the
    segments and the relayout of the rest) over the ranges of a 6-piece backward pass, in callback order"""
    from ipoke_amd import optim as O
    m, _ = _flow(dtype)
    eng = m.engine
    eng.prepare_weights()
    opt = O.FusedAdamAmsgrad(m, lr=LR, weight_decay=WD)
    n = eng.n_params
    _carried_state(opt, n, 900)
    grads = m.bind_grads()
    grads.copy_((torch.randn(n, generator=torch.Generator().manual_seed(901)) * 1e-2).to(DEV))
    torch.cuda.synchronize()
    before = [t.cpu().clone() for t in (eng.params, opt.exp_avg, opt.exp_avg_sq, opt.max_exp_avg_sq)]
    shadow_before = eng.shadow.clone()
    nr = lib().ipoke_flow_piece_ranges(eng.handle, 6, None, 0)
    buf = (ctypes.c_int64 * (3 * nr))()
    assert lib().ipoke_flow_piece_ranges(eng.handle, 6, buf, nr) == nr
    step = 4
    h = X.Hyper(LR, B1, B2, EPS, WD, step, GS)
    for i in range(nr):
        b, e = buf[3 * i + 1], buf[3 * i + 2]
        _lib.check(lib().ipoke_flow_adam_range(eng.handle, ptr(eng.params), ptr(grads), ptr(opt.exp_avg), ptr(opt.exp_avg_sq),
                                               ptr(opt.max_exp_avg_sq), ptr(eng.shadow), b, e, *hyper_args(h), 128, stream()))
    torch.cuda.synchronize()
    _check_step(eng, opt, before, grads, h, shadow_before, f"adam_range {dtype}")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_native_piecewise_train_step(dtype):
    """one native train step as SecondStageTrainer.train_step runs it (FusedAdamAmsgrad.arm_native + ipoke_flow_backward_pieces, the
    update and refresh of every piece on the ready stream): the state after the step is the emulation of (parameters, moments before
    the step; the flat gradients the step used; its hyper-parameters), bit for bit.  No announced range separates a weight-norm gain
    from its direction: prepare_range recomputes the scale with the direction, so a split would read a stale or a future gain."""
    from ipoke_amd import optim as O
    m, arch = _flow(dtype)
    eng = m.engine
    gen = torch.Generator().manual_seed(950)
    x = torch.randn(4, 32, 8, 8, generator=gen).to(DEV)
    cond = torch.randn(4, arch["h_channels"], 8, 8, generator=gen).to(DEV)
    with torch.no_grad():
        m(x, cond)                                       # data-dependent initialisation pass
    m.mark_weights_updated()
    m.train()
    opt = O.FusedAdamAmsgrad(m, lr=7e-4, weight_decay=WD)
    n = eng.n_params
    _carried_state(opt, n, 951)
    opt.steps = 4
    grads = m.bind_grads()
    grads.zero_()
    out, logdet = m(x, cond)
    loss = (out ** 2).sum() * 0.5 - logdet.sum()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)), float(loss)
    before = [t.cpu().clone() for t in (eng.params, opt.exp_avg, opt.exp_avg_sq, opt.max_exp_avg_sq)]
    shadow_before = eng.shadow.clone()
    opt.begin_step()
    opt.arm_native(grad_scale=GS)
    ranges = []

    def announce(b, e, piece):
        ranges.append((piece, b, e))
    announce.wants_piece = True
    eng.grad_ready_hook = (6, torch.cuda.Stream(), announce)
    try:
        loss.backward()
    finally:
        eng.grad_ready_hook = None
    opt.finish_native()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(m.flat_grads).all())
    assert len(ranges) >= 6
    cover = torch.zeros(n, dtype=torch.int32)
    for _, b, e in ranges:
        cover[b:e] += 1
    assert int(cover.min()) == 1 and int(cover.max()) == 1
    info = (ctypes.c_int64 * 32)()
    pairs = 0
    for i in range(eng.n_ops):
        _lib.check(lib().ipoke_flow_op_info(eng.handle, i, info))
        p_g, p_v = info[11], info[12]
        if p_g < 0 or p_v < 0:
            continue
        rg = [k for k, (_, b, e) in enumerate(ranges) if b <= p_g < e]
        rv = [k for k, (_, b, e) in enumerate(ranges) if b <= p_v < e]
        assert rg == rv, f"op {i}: gain at {p_g} announced in range {rg}, direction at {p_v} in range {rv}"
        pairs += 1
    assert pairs > 0
    h = X.Hyper(7e-4, B1, B2, EPS, WD, 5, GS)
    _check_step(eng, opt, before, m.flat_grads, h, shadow_before, f"native step {dtype}")
