"""CPU: the restatement of the masked poke rules (tests/poke_mask_ref.py, the arithmetic of the kernels: double sums) against golden G20,
which scripts/make_goldens_masked_pokes.py wrote from the reference's own _get_poke with filter_flow on and _compute_mask_with_flow
(data/base_dataset.py:507-648, :343-351).  Exact: the golden's cases keep every compared value more than 1e-6 from its threshold, so the
reference's fp32 reductions and the double sums decide alike."""
import numpy as np
import torch

from oracle import data_ref
from tests import poke_mask_ref as R
from tests.conftest import t

N_POKES = 5


def _cases(g):
    for ci in range(int(g["n_cases"])):
        size, ps, zero, equal, fix, ki, mi = (int(v) for v in g[f"meta{ci}"])
        flow = t(g[f"flow_{size}_{g['kinds'][ki]}"])
        yield ci, flow, t(g[f"mask{ci}"]).bool(), ps, bool(zero), bool(equal), bool(fix), str(g["masks"][mi])


def test_golden_meets_its_condition_and_covers_every_rule(golden):
    g = golden("g20_masked_pokes")
    assert int(g["n_cases"]) == 90 and float(g["min_margin"]) > 1e-6
    rules, equal_off, fix_on = set(), 0, 0
    for ci, flow, mask, ps, zero, equal, fix, mname in _cases(g):
        rules.add(R.candidate_sets(flow, mask, ps, zero)[2])
        equal_off += not equal
        fix_on += fix
        if mname == "window":
            assert bool(mask[ps:-ps, ps:-ps].all()) and not bool(mask[:ps].any()) and not bool(mask[:, -ps:].any())
    # the first rule, its first fallback, the background set and the percentile set; the last fallback (amp > mean) needs a two-valued
    # field, which tests/test_poke_mask_gpu.py builds
    assert rules == {2, 1, "bg", "pct"}, rules
    assert equal_off == 1 and fix_on == 1


def test_restatement_equals_the_reference(golden):
    g = golden("g20_masked_pokes")
    for ci, flow, mask, ps, zero, equal, fix, mname in _cases(g):
        poke, centers = R.get_poke(flow, mask, ps, N_POKES, data_ref.UniformDraws(g[f"u{ci}"], N_POKES, fix, zero), zero=zero, fix_n_pokes=fix,
                                   equal_poke_val=equal)
        assert np.array_equal(centers.numpy(), g[f"centers{ci}"]), (ci, mname, centers.tolist(), g[f"centers{ci}"].tolist())
        assert np.array_equal(poke.nonzero().numpy().astype(np.int16), g[f"poke_nz{ci}"]), ci
        assert np.array_equal(poke[poke != 0].numpy(), g[f"poke_val{ci}"]), ci


def test_zero_poke_centres_lie_on_the_background(golden):
    """the property the feature exists for, on the reference's own outputs"""
    g = golden("g20_masked_pokes")
    for ci, flow, mask, ps, zero, equal, fix, mname in _cases(g):
        c = t(g[f"centers{ci}"])
        c = c[c[:, 0] >= 0]
        on_mask = mask[c[:, 0], c[:, 1]]
        if zero and mname in ("blob", "false", "flow"):
            assert not bool(on_mask.any()), ci
        if not zero and R.candidate_sets(flow, mask, ps, zero)[2] == 2:
            assert bool(on_mask.all()), ci


def test_all_true_mask_is_the_unmasked_path(golden):
    g = golden("g20_masked_pokes")
    seen = 0
    for ci, flow, mask, ps, zero, equal, fix, mname in _cases(g):
        if mname != "true":
            continue
        poke, centers = data_ref.get_poke(flow, ps, N_POKES, data_ref.UniformDraws(g[f"u{ci}"], N_POKES, fix, zero), zero=zero, fix_n_pokes=fix,
                                          equal_poke_val=equal)
        assert np.array_equal(centers.numpy(), g[f"centers{ci}"]), ci
        assert np.array_equal(poke.nonzero().numpy().astype(np.int16), g[f"poke_nz{ci}"]), ci
        assert np.array_equal(poke[poke != 0].numpy(), g[f"poke_val{ci}"]), ci
        seen += 1
    assert seen == 18


def test_flow_mask_restatement_equals_the_reference(golden):
    g = golden("g20_masked_pokes")
    n = 0
    for key in g:
        if key.startswith("fmask_"):
            mask, status = R.flow_mask(t(g["flow_" + key[len("fmask_"):]]))
            assert status == 0 and np.array_equal(mask.numpy().astype(np.uint8), g[key]), key
            assert 0 < int(mask.sum()) < mask.numel()
            n += 1
    assert n == 6
    mask, status = R.flow_mask(torch.full((2, 16, 16), 0.5))
    assert status == 1 and not bool(mask.any())
