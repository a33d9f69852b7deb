"""Foreground-masked poke sampling on the device (``PokeSimulator.get_poke(mask=...)``, ``flow_mask``, ``make_batch(mask=...)`` in
ipoke_amd/data.py; ``ipoke_poke_simulate_masked`` / ``ipoke_flow_mask`` in csrc/data.hip) against golden G20: the reference's own _get_poke
with filter_flow on and _compute_mask_with_flow (data/base_dataset.py:507-648, :343-351), written by scripts/make_goldens_masked_pokes.py
under the condition that no compared value lies within 1e-6 of its threshold.  Index work is bit-exact; poke values are copies of flow
entries.  The C-ABI calls of this file hand over buffers with guard rows in front and behind, which must come back untouched."""
import numpy as np
import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd._lib import check, ptr
from ipoke_amd.data import ClipAugmenter, FlowError, PokeSimulator
from oracle import data_ref
from tests import poke_mask_ref as R
from tests.conftest import t

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_POKES = 5
GUARD = 4096                       # elements in front of and behind every buffer the kernels are given
SENTINEL = {torch.float32: -12345.5, torch.int64: -7777, torch.int32: -7777, torch.uint8: 0xA5}


class Guarded:
    """a device buffer of ``shape`` between two guard rows filled with a sentinel"""

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.t = self.full[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        s = SENTINEL[self.full.dtype]
        return bool((self.full[:GUARD] == s).all()) and bool((self.full[-GUARD:] == s).all())


def _sim(size, poke_size, equal=True, fix=False, **extra):
    return PokeSimulator({"spatial_size": (size, size), "n_pokes": N_POKES, "poke_size": poke_size, "scale_poke_to_res": True,
                          "equal_poke_val": bool(equal), "fix_n_pokes": bool(fix), **extra})


def simulate_guarded(sim, flow, zero, u, mask):
    """ipoke_poke_simulate_masked through the C ABI on guarded buffers (mask None -> NULL) -> (poke, centers, flow_out, status)"""
    B, _, H, W = flow.shape
    lib = _lib.lib()
    bufs = dict(flow=Guarded(flow.shape, torch.float32, flow), u=Guarded(u.shape, torch.float32, u),
                zero=Guarded((B,), torch.int32, zero.to(torch.int32)), poke=Guarded(flow.shape, torch.float32),
                centers=Guarded((B, N_POKES, 2), torch.int64), flow_out=Guarded(flow.shape, torch.float32), status=Guarded((B,), torch.int32),
                ws=Guarded((lib.ipoke_poke_masked_workspace_bytes(B, H, W, sim.poke_size, N_POKES),), torch.uint8))
    if mask is not None:
        bufs["mask"] = Guarded(mask.shape, torch.uint8, mask.to(torch.uint8))
    check(lib.ipoke_poke_simulate_masked(ptr(bufs["flow"].t), B, H, W, sim.poke_size, N_POKES, int(sim.fix_n_pokes), int(sim.equal_poke_val),
                                         ptr(bufs["zero"].t), ptr(bufs["u"].t), ptr(bufs["mask"].t) if mask is not None else None,
                                         ptr(bufs["poke"].t), ptr(bufs["centers"].t), ptr(bufs["flow_out"].t), ptr(bufs["status"].t),
                                         ptr(bufs["ws"].t), _lib.current_stream()))
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.intact(), f"guard rows of {name} were written"
    assert torch.equal(bufs["flow"].t, flow) and torch.equal(bufs["u"].t, u)
    return tuple(bufs[k].t.clone() for k in ("poke", "centers", "flow_out", "status"))


def flow_mask_guarded(flow):
    B, _, H, W = flow.shape
    lib = _lib.lib()
    bufs = dict(flow=Guarded(flow.shape, torch.float32, flow), mask=Guarded((B, H, W), torch.uint8), status=Guarded((B,), torch.int32),
                ws=Guarded((lib.ipoke_flow_mask_workspace_bytes(B, H, W),), torch.uint8))
    check(lib.ipoke_flow_mask(ptr(bufs["flow"].t), B, H, W, ptr(bufs["mask"].t), ptr(bufs["status"].t), ptr(bufs["ws"].t), _lib.current_stream()))
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.intact(), f"guard rows of {name} were written"
    return bufs["mask"].t.clone(), bufs["status"].t.clone()


def _cases(g):
    for ci in range(int(g["n_cases"])):
        size, ps, zero, equal, fix, ki, mi = (int(v) for v in g[f"meta{ci}"])
        yield dict(ci=ci, size=size, ps=ps, zero=bool(zero), equal=bool(equal), fix=bool(fix), mask_kind=str(g["masks"][mi]),
                   flow=t(g[f"flow_{size}_{g['kinds'][ki]}"]), mask=t(g[f"mask{ci}"]), u=t(g[f"u{ci}"]))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_golden_cases(golden):
    g = golden("g20_masked_pokes")
    for c in _cases(g):
        ci = c["ci"]
        sim = _sim(c["size"], c["ps"], c["equal"], c["fix"])
        flow = c["flow"].unsqueeze(0).to(DEV)
        poke, centers, flow_out, status = simulate_guarded(sim, flow, torch.tensor([c["zero"]], device=DEV), c["u"].unsqueeze(0).to(DEV),
                                                           c["mask"].unsqueeze(0).to(DEV))
        assert int(status[0]) == 0, ci
        assert np.array_equal(centers[0].cpu().numpy(), g[f"centers{ci}"]), (ci, c["mask_kind"], centers[0].tolist(), g[f"centers{ci}"].tolist())
        p = poke[0].cpu()
        assert np.array_equal(p.nonzero().numpy().astype(np.int16), g[f"poke_nz{ci}"]), ci
        assert np.array_equal(p[p != 0].numpy(), g[f"poke_val{ci}"]), ci
        assert abs(flow_out.abs().sum().item() - float(g[f"flow_ret_abs{ci}"])) <= 1e-3 * max(1.0, float(g[f"flow_ret_abs{ci}"]))
        if c["zero"]:
            assert flow_out.abs().max().item() == 0.0
        else:
            assert torch.equal(flow_out[0].cpu(), c["flow"])
        # the public method is the same launch
        assert _same(sim.get_poke(flow, torch.tensor([c["zero"]]), c["u"].unsqueeze(0).to(DEV), mask=c["mask"].unsqueeze(0).to(DEV).bool()),
                     (poke, centers, flow_out, status)), ci


def test_flow_mask_golden_and_constant_map(golden):
    g = golden("g20_masked_pokes")
    for size in (64, 128):
        keys = [f"{size}_{k}" for k in g["kinds"]]
        flows = torch.stack([t(g["flow_" + k]) for k in keys] + [torch.full((2, size, size), 0.25)]).to(DEV)        # the last map is constant
        mask, status = flow_mask_guarded(flows)
        assert status.tolist() == [0, 0, 0, 1]
        for j, k in enumerate(keys):
            assert np.array_equal(mask[j].cpu().numpy(), g["fmask_" + k]), k
        assert not bool(mask[3].any())
        m2, s2 = _sim(size, 5).flow_mask(flows)
        assert m2.dtype == torch.bool and torch.equal(m2, mask.bool()) and torch.equal(s2, status)


def test_unmasked_path_is_unchanged(golden):
    """mask=None (the C entry point with a NULL mask) == ipoke_poke_simulate bit for bit on the 24 cases of G11, whose centres it still
    reproduces; an all-true mask gives an ordinary sample the same centres and pokes."""
    g = golden("g11_data_path")
    assert int(g["n_cases"]) == 24
    for ci in range(24):
        size, poke_size, zero, equal, fix = (int(v) for v in g[f"meta{ci}"])
        sim = _sim(size, poke_size, equal, fix)
        flow = t(g[f"flow{ci}"], DEV).unsqueeze(0)
        zero_t, u = torch.tensor([bool(zero)], device=DEV), t(g[f"u{ci}"], DEV).unsqueeze(0)
        plain = sim.get_poke(flow, zero_t, u)                                           # ipoke_poke_simulate
        assert np.array_equal(plain[1][0].cpu().numpy(), g[f"centers{ci}"]), ci
        assert _same(simulate_guarded(sim, flow, zero_t, u, None), plain), ci
        assert _same(sim.get_poke(flow, zero_t, u, mask=None), plain), ci
        if not zero:
            full = sim.get_poke(flow, zero_t, u, mask=torch.ones(1, size, size, dtype=torch.bool, device=DEV))
            assert torch.equal(full[1], plain[1]) and torch.equal(full[0], plain[0]), ci


def _batch_of_eight(g):
    """128 px / poke 5: ordinary and zero-poke samples under blob, all-true and all-false masks"""
    picked = [c for c in _cases(g) if (c["size"], c["ps"], c["equal"], c["fix"]) == (128, 5, True, False) and c["mask_kind"] in ("blob", "true", "false")]
    picked = picked[:4] + picked[-4:]
    assert len(picked) == 8 and {c["zero"] for c in picked} == {False, True} and {c["mask_kind"] for c in picked} == {"blob", "true", "false"}
    flows = torch.stack([c["flow"] for c in picked]).to(DEV)
    masks = torch.stack([c["mask"] for c in picked]).to(DEV)
    zero = torch.tensor([c["zero"] for c in picked], device=DEV)
    u = torch.stack([c["u"] for c in picked]).to(DEV)
    return picked, flows, masks, zero, u


def test_batched_equals_per_sample(golden):
    g = golden("g20_masked_pokes")
    picked, flows, masks, zero, u = _batch_of_eight(g)
    sim = _sim(128, 5)
    poke, centers, flow_out, status = simulate_guarded(sim, flows, zero, u, masks)
    assert int(status.sum()) == 0
    for j, c in enumerate(picked):
        assert np.array_equal(centers[j].cpu().numpy(), g[f"centers{c['ci']}"]), c["ci"]
        one = sim.get_poke(flows[j:j + 1], zero[j:j + 1], u[j:j + 1], mask=masks[j:j + 1])
        assert _same(one, (poke[j:j + 1], centers[j:j + 1], flow_out[j:j + 1], status[j:j + 1])), c["ci"]


def test_two_runs_are_bit_identical(golden):
    picked, flows, masks, zero, u = _batch_of_eight(golden("g20_masked_pokes"))
    sim = _sim(128, 5)
    assert _same(sim.get_poke(flows, zero, u, mask=masks), sim.get_poke(flows, zero, u, mask=masks))
    assert _same(sim.flow_mask(flows), sim.flow_mask(flows))


def _smooth_raw(B, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.randn(B, 2, 6, 6, device=DEV, generator=gen)
    return torch.nn.functional.interpolate(coarse, size=(256, 256), mode="bicubic", align_corners=False) * 10


@pytest.mark.parametrize("augmented", [False, True])
def test_properties_at_batch_size(augmented):
    """B = 64 smooth random flows at 128 px through make_batch(mask="flow"), plain and under a ClipAugmenter parameter set: ordinary samples
    whose first rule found candidates poke the foreground only, zero-poke samples with background in the window poke the background only,
    counts lie in [1, n_pokes] and centres in the window."""
    B, S, ps = 64, 128, 5
    sim = _sim(S, ps)
    raw = _smooth_raw(B, 11)
    zero = torch.arange(B) % 5 == 0
    kw = {}
    if augmented:
        aug = ClipAugmenter({"spatial_size": (S, S), "augment": True})
        i = np.arange(B)
        kw = dict(augment=aug.params(1.0 + 0.1 * (i % 3), 1.0 - 0.1 * (i % 2), 1.0 + 0.05 * (i % 4), 0.02 * (i % 5), (i % 7) * 4.0 - 12.0,
                                     (i % 5) * 3 - 6, (i % 3) * 4 - 4, device=DEV),
                  frames_u8=torch.randint(0, 256, (B, 1, S, S, 3), dtype=torch.uint8, device=DEV))
    batch = sim.make_batch(None if augmented else torch.zeros(B, 1, 3, S, S, device=DEV), raw, zero,
                           generator=torch.Generator(device=DEV).manual_seed(5), mask="flow", **kw)
    # the mask comes from the flow the pokes are taken from: after the warp, before the zeroing of the zero-poke samples
    flow = sim.get_flow(raw)
    if augmented:
        flow = aug.flow(flow, kw["augment"])
        assert not torch.equal(flow, sim.get_flow(raw))
    mask, mstatus = sim.flow_mask(flow)
    assert batch["mask"].dtype == torch.bool and torch.equal(batch["mask"], mask) and int(mstatus.sum()) == 0
    assert bool((batch["flow"][zero] == 0).all()) and torch.equal(batch["flow"][~zero], flow[~zero]) and bool(mask[zero].any())
    poke, centers = batch["poke"]
    assert int(batch["poke_status"].sum()) == 0
    n = (centers[:, :, 0] >= 0).sum(1)
    assert int(n.min()) >= 1 and int(n.max()) <= N_POKES
    valid = centers[centers[:, :, 0] >= 0]
    assert int(valid.min()) >= ps and int(valid.max()) < S - ps
    flow_c, mask_c, centers_c = flow.cpu(), mask.cpu(), centers.cpu()
    first_rule = background = 0
    for b in range(B):
        c = centers_c[b, :int(n[b])]
        on_mask = mask_c[b][c[:, 0], c[:, 1]]
        if bool(zero[b]):
            if not bool(mask_c[b, ps:-ps, ps:-ps].all()):
                assert not bool(on_mask.any()), b
                background += 1
        elif R.candidate_sets(flow_c[b], mask_c[b], ps, False)[2] == 2:
            assert bool(on_mask.all()), b
            first_rule += 1
    print(f"first rule non-empty in {first_rule} of {int((~zero).sum())} ordinary samples; background in the window in {background} of "
          f"{int(zero.sum())} zero-poke samples")
    assert first_rule >= 1 and background == int(zero.sum())                           # a flow-derived mask never covers the whole window


def test_last_fallback_rule_against_the_restatement():
    """A two-valued amplitude has its maximum at mean + std' with std' just below the unbiased std: mean + 2 std and mean + std select
    nothing, amp > mean selects the upper half -- the last fallback (:583), which no golden case reaches."""
    S, ps = 64, 5
    flow = torch.zeros(2, S, S)
    flow[0, :, :S // 2], flow[0, :, S // 2:] = 1.0, 3.0
    mask = torch.ones(S, S, dtype=torch.bool)
    assert R.candidate_sets(flow, mask, ps, False)[2] == 0
    u = torch.rand(1 + 2 * N_POKES, generator=torch.Generator().manual_seed(2))
    want_poke, want_centers = R.get_poke(flow, mask, ps, N_POKES, data_ref.UniformDraws(u.numpy(), N_POKES, False, False))
    poke, centers, _, status = simulate_guarded(_sim(S, ps), flow.unsqueeze(0).to(DEV), torch.tensor([False], device=DEV), u.unsqueeze(0).to(DEV),
                                                mask.unsqueeze(0).to(DEV))
    assert int(status[0]) == 0 and torch.equal(centers[0].cpu(), want_centers) and torch.equal(poke[0].cpu(), want_poke)
    assert int(want_centers[want_centers[:, 1] >= 0][:, 1].min()) >= S // 2


def test_no_candidate_is_reported():
    """a zero-poke sample of constant amplitude under a mask: 0 / 0 everywhere, no value source passes"""
    sim = _sim(64, 5)
    flow = torch.zeros(2, 2, 64, 64, device=DEV)
    flow[1] = torch.randn(2, 64, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    mask = torch.zeros(2, 64, 64, dtype=torch.bool, device=DEV)
    mask[:, 20:40, 20:40] = True
    zero = torch.tensor([True, True])
    poke, centers, _, status = sim.get_poke(flow, zero, strict=False, mask=mask)
    assert status.tolist() == [1, 0] and int(centers[0].max()) == -1 and poke[0].abs().max().item() == 0
    with pytest.raises(FlowError):
        sim.get_poke(flow, zero, mask=mask)


def test_make_batch_reads_the_config():
    raw = _smooth_raw(2, 3)
    images = torch.zeros(2, 1, 3, 64, 64, device=DEV)
    u = torch.rand(2, 1 + 2 * N_POKES, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    with pytest.raises(ValueError, match="grabCut"):
        _sim(64, 5, filter_flow=True).make_batch(images, raw, u=u)
    sim = _sim(64, 5, filter_flow=True, use_flow_for_weights=True)
    derived = sim.make_batch(images, raw, u=u)
    assert torch.equal(derived["mask"], sim.flow_mask(sim.get_flow(raw))[0])
    given = _sim(64, 5, filter_flow=True).make_batch(images, raw, u=u, mask=derived["mask"].to(torch.uint8))
    assert torch.equal(given["mask"], derived["mask"]) and _same(given["poke"], derived["poke"])
    plain = _sim(64, 5).make_batch(images, raw, u=u)
    assert "mask" not in plain
    with pytest.raises(ValueError):
        sim.get_poke(sim.get_flow(raw), u=u, mask=torch.ones(2, 32, 32, dtype=torch.bool, device=DEV))
