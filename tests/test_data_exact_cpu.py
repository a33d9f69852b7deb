"""CPU: the restatements of tests/data_exact.py against what anchors them, and the case table against what the GPU tests assume of it.

The poke rules are anchored to golden G11, the reference's own _get_flow / _get_poke run (data/base_dataset.py:507-693): select_ref +
fill_ref reproduce every stored case bit for bit.  The resize restatement is anchored to torch's float64 bilinear interpolation.  Every
case of the table is ``robust`` -- none of its decisions can hinge on the order of a sum -- and together the cases reach every rule, both
branches of the percentile interpolation and both value sources of a zero-poke sample: tests/test_data_exact_gpu.py compares the kernels
bit for bit on these cases and relies on all of that."""
import numpy as np
import torch

from tests import data_exact as X

N_POKES = 5


def test_restatement_reproduces_the_golden_cases(golden):
    g = golden("g11_data_path")
    assert int(g["n_cases"]) == 24
    for ci in range(24):
        size, ps, zero, equal, fix = (int(v) for v in g[f"meta{ci}"])
        flow = g[f"flow{ci}"]
        sel = X.select_ref(flow, ps, N_POKES, bool(fix), bool(zero), g[f"u{ci}"])
        assert sel.status == 0
        assert np.array_equal(sel.centers, g[f"centers{ci}"]), (ci, sel.centers.tolist(), g[f"centers{ci}"].tolist())
        poke, flow_out = X.fill_ref(flow, sel, bool(zero), ps // 2, bool(equal))
        p = torch.from_numpy(poke)
        assert np.array_equal(p.nonzero().numpy().astype(np.int16), g[f"poke_nz{ci}"]), ci
        assert np.array_equal(p[p != 0].numpy(), g[f"poke_val{ci}"]), ci
        assert np.array_equal(flow_out, np.zeros_like(flow) if zero else flow)


def test_every_case_is_robust():
    failing = [c.name for c in X.cases() if not X.robust(c)]
    assert failing == [], failing
    assert all(X.robust(c) for c in X.batch_of_five())
    for H, W, flows in X.mask_flows():
        for j, flow in enumerate(flows):
            mask, status, ok = X.flow_mask_ref(flow)
            assert ok, (H, W, j)
            assert status == (1 if j == 2 else 0), (H, W, j)


def test_table_reaches_every_rule_branch_and_source():
    rules, branches, sources, tied, sizes, pokes, fixes, windows = set(), set(), set(), set(), set(), set(), set(), set()
    short = first = last = 0
    for c in X.cases():
        sel = X.select_ref(c.flow, c.ps, c.n_pokes, c.fix, c.zero, c.u)
        assert sel.status == 0 and sel.rule == c.want_rule, (c.name, sel.rule, c.want_rule)
        assert (c.H - 2 * c.ps) * (c.W - 2 * c.ps) == c.n == sel.amp.size
        rules.add(sel.rule)
        sizes.add(c.ps)
        pokes.add(c.n_pokes)
        fixes.add(c.fix)
        windows.add(c.n)
        if c.zero:
            branches.add(sel.pct_branch)
            sources.add(sel.src_rule)
            tied.add(sel.pct_tied)
        short += len(sel.cand) < c.n_pokes and not c.fix and sel.np == len(sel.cand)
        ww = c.W - 2 * c.ps
        flat = (sel.centers[:sel.np, 0] - c.ps) * ww + sel.centers[:sel.np, 1] - c.ps
        first += sel.cand[0] in flat
        last += sel.cand[-1] in flat
    assert rules == {2, 1, 0, "pct"}, rules
    assert branches == {">=", "<"}, branches
    assert sources == {1, 0}, sources                      # value sources > mean + std, and the fallback > mean
    assert tied == {True, False}, tied                     # equal order statistics around the percentile, and distinct ones
    assert sizes == {1, 2, 3, 4, 5} and pokes == {1, 5, 16} and fixes == {False, True}
    assert {4, 1023, 1024, 1025, 2880} <= windows
    assert short >= 2 and first >= 3 and last >= 3
    assert any(c.H != c.W for c in X.cases())


def test_straddling_rows_straddle():
    """the rows built to fall on either side of a thread's chunk boundary do: two picked positions i, i + 1 with (i + 1) % per == 0"""
    seen = set()
    for c in X.cases():
        if "straddle" not in c.name:
            continue
        sel = X.select_ref(c.flow, c.ps, c.n_pokes, c.fix, c.zero, c.u)
        per = -(-c.n // X.K_THREADS)
        ww = c.W - 2 * c.ps
        flat = set(((sel.centers[:sel.np, 0] - c.ps) * ww + sel.centers[:sel.np, 1] - c.ps).tolist())
        assert any(i + 1 in flat and (i + 1) % per == 0 for i in flat), c.name
        assert sel.np == min(c.n_pokes, len(sel.cand))
        seen.add(per)
    assert seen == {2, 3}, seen


def test_overlapping_cases_overlap():
    """in the adjacent cases a later poke overwrites part of an earlier one with a different value, so the order of the fill shows in
    the tensor -- except for an ordinary sample with equal_poke_val off, where every poke copies the flow of the pixel it covers; the
    corner cases reach row and column poke_size - half and their mirror images"""
    shown = set()
    for c in X.cases():
        if "adjacent" not in c.name and "corners" not in c.name:
            continue
        sel = X.select_ref(c.flow, c.ps, c.n_pokes, c.fix, c.zero, c.u)
        half = c.ps // 2
        poke, _ = X.fill_ref(c.flow, sel, c.zero, half, c.equal)
        rev = X.SimpleNamespace(**{**vars(sel), "centers": sel.centers[:sel.np][::-1], "src": sel.src[:sel.np][::-1]})
        if "corners" in c.name:                           # far apart: these are about the patches' reach, not their order
            pass
        elif c.equal or c.zero:
            assert not np.array_equal(poke, X.fill_ref(c.flow, rev, c.zero, half, c.equal)[0]), c.name
            shown.add((c.equal, c.zero))
        else:
            assert np.array_equal(poke[:, c.ps:-c.ps, c.ps:-c.ps] != 0, np.abs(poke[:, c.ps:-c.ps, c.ps:-c.ps] - c.flow[:, c.ps:-c.ps, c.ps:-c.ps]) == 0)
        if "corners" in c.name:
            nz = np.abs(poke).sum(0).nonzero()
            assert nz[0].min() == c.ps - half and nz[1].min() == c.ps - half, c.name
            assert nz[0].max() == c.H - c.ps - 1 + half and nz[1].max() == c.W - c.ps - 1 + half, c.name
    assert shown == {(True, False), (False, True)}, shown


def test_resize_ref_equals_float64_interpolate():
    """to 1e-12 of max(1, largest |value|): torch forms its float64 coordinate as ox * fl(s), off by two roundings of a value up to 999,
    and the offset inputs carry values of 1e4, so an absolute 1e-12 lies below the float64 reference's own rounding (5.5e-12 measured);
    relative to the values the two agree to 1.2e-13"""
    worst = 0.0
    for i, ((B, C, Hi, Wi), (Ho, Wo), _) in enumerate(X.RESIZE_SHAPES):
        for x in X.resize_inputs((B, C, Hi, Wi), 100 + i):
            for div in X.RESIZE_DIVS:
                ref, m, sy, sx = X.resize_ref(x, Ho, Wo, div)
                a = torch.from_numpy(x) / torch.tensor(div, dtype=torch.float32)
                assert a.dtype == torch.float32
                want = torch.nn.functional.interpolate(a.double(), size=(Ho, Wo), mode="bilinear", align_corners=True).numpy()
                err = np.abs(ref - want).max() / max(1.0, np.abs(want).max())
                worst = max(worst, err)
                assert err <= 1e-12, ((Hi, Wi), (Ho, Wo), div, err)
                assert ref.shape == m.shape == sy.shape == sx.shape == (B, C, Ho, Wo)
                assert (np.abs(ref) <= m).all() and (sy <= 2 * m).all() and (sx <= 2 * m).all()
    print(f"resize_ref against float64 interpolate: worst error {worst:.3e} of max(1, |value|)")


def test_amplitude_cases_can_tell_a_fused_multiply_add():
    """on the table's random fields fl(fl(vx vx) + fl(vy vy)) and the once-rounded vx vx + fl(vy vy) differ somewhere, so the exact amplitude
    comparison of tests/test_data_exact_gpu.py has something to hold on to"""
    differing = 0
    for c in X.cases():
        vx, vy = (c.flow[k, c.ps:c.H - c.ps, c.ps:c.W - c.ps] for k in (0, 1))
        plain = np.sqrt(vx * vx + vy * vy)
        fused = np.sqrt((vx.astype(np.float64) * vx.astype(np.float64) + (vy * vy).astype(np.float64)).astype(np.float32))
        differing += not np.array_equal(plain, fused)
    assert differing >= 10, differing


def test_tie_cases_tie_and_their_sums_are_exact():
    """an amplitude equal to the threshold of the rule in force, picks on both sides of it in the candidate order, and statistics that no
    order of summation can change -- 0.5 and 0.5 exactly"""
    for c in X.tie_cases():
        sel = X.select_ref(c.flow, c.ps, c.n_pokes, c.fix, c.zero, c.u)
        assert sel.status == 0 and sel.rule == c.want_rule == 0, c.name
        assert X.sums_are_exact(sel.amp), c.name
        mean, std = X.R._stats(torch.from_numpy(sel.amp))
        assert float(mean) == 0.5 and float(std) == 0.5
        tied = np.flatnonzero(sel.amp.flatten() == np.float32(mean))
        assert tied.tolist() == [3] and 3 not in sel.cand
        ww = c.W - 2 * c.ps
        flat = (sel.centers[:sel.np, 0] - c.ps) * ww + sel.centers[:sel.np, 1] - c.ps
        assert (flat < 3).any() or sel.cand[0] > 3
        assert (flat > 3).sum() >= 2, c.name                # with >= for > these picks would each land one candidate earlier
    assert not any(X.sums_are_exact(X.select_ref(c.flow, c.ps, c.n_pokes, c.fix, c.zero, c.u).amp) for c in X.cases() if "smooth" in c.name)
