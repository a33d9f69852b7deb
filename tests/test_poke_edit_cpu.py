"""CPU side of the poke editing (csrc/data.hip ``ipoke_poke_stamp`` / ``ipoke_poke_randomize``; reference second_stage_video.py:798-833,
959-966): the restatement of tests/poke_ref.py against plain torch slice assignment -- ``p[:, a:b, c:d] = v`` with Python's own slicing, so
the slice rules are Python's --, the condition of the GPU tests' inputs, and the public surface (symbols, bindings, methods)."""
import ctypes

import numpy as np
import pytest
import torch

from ipoke_amd import _lib, configs
from ipoke_amd.data import PokeSimulator
from ipoke_amd.second_stage import PokeMotionModel
from tests import poke_cases, poke_ref
from tests.helpers import synthetic_batch


def torch_stamp(centers, half, H, W, values=None, flow=None, skip_negative=True):
    """the reference's loop (:962-966) on torch tensors"""
    B = centers.shape[0]
    poke = torch.zeros(B, 2, H, W)
    for b in range(B):
        cs = centers[b]
        keep = (cs >= 0).all(-1) if skip_negative else torch.ones(len(cs), dtype=torch.bool)
        for j in keep.nonzero().flatten().tolist():
            c = cs[j]
            v = values[b, j] if values is not None else flow[b, :, c[0], c[1]]
            poke[b][:, c[0] - half:c[0] + half + 1, c[1] - half:c[1] + half + 1] = v[:, None, None]
    return poke


@pytest.mark.parametrize("H,W,half", [(64, 64, 2), (32, 48, 3), (9, 7, 5)])
def test_slice_rules_are_pythons(H, W, half):
    for extent in (H, W):
        for c in range(-2 * extent - 3, 2 * extent + 3):
            lo, hi = poke_ref.slice_range(c, half, extent)
            assert list(range(extent))[c - half:c + half + 1] == list(range(lo, hi)), (c, half, extent)
    lo, hi = poke_ref.slice_range(0, 2, 64)
    assert (lo, hi) == (62, 3) and not poke_ref.covered(0, 0, 2, 64, 64).any()          # the reference's empty slice at (0, 0)


def test_stamp_restatement_against_slice_assignment():
    H, W, half = 64, 64, 2
    v = torch.tensor([[[1.0, -1.0], [2.0, -2.0], [3.0, -3.0], [4.0, -4.0]]])
    # overlap order: the later poke wins where the squares meet
    c = torch.tensor([[[30, 30], [31, 32], [-1, -1], [30, 31]]])
    want = torch_stamp(c, half, H, W, values=v)
    got = poke_ref.stamp(c.numpy(), half, H, W, values=v.numpy())
    assert np.array_equal(got, want.numpy())
    assert want[0, 0, 30, 31] == 4.0 and want[0, 0, 33, 34] == 2.0 and want[0, 0, 28, 28] == 1.0 and (want[0, 0] == 3.0).sum() == 0
    # the (0, 0) empty slice, alone
    z = poke_ref.stamp(np.zeros((1, 4, 2), dtype=np.int64), half, H, W, values=v.numpy())
    assert not z.any() and not torch_stamp(torch.zeros(1, 4, 2, dtype=torch.int64), half, H, W, values=v).any()
    # a centre on each edge of the valid window, and one step outside it on each side (row start wraps -> empty; stop clamps -> cut)
    for r, c_, n_px in [(half, half, 25), (H - 1 - half, W - 1 - half, 25), (half - 1, 30, 0), (30, half - 1, 0), (H - half, 30, 20), (30, W - half, 20),
                        (H - 1, W - 1, 9)]:
        cc = torch.tensor([[[r, c_]]])
        want = torch_stamp(cc, half, H, W, values=v[:, :1])
        assert np.array_equal(poke_ref.stamp(cc.numpy(), half, H, W, values=v[:, :1].numpy()), want.numpy())
        assert int((want[0, 0] != 0).sum()) == n_px, (r, c_)
    # -1 rows: skipped with skip_negative, Python's wrap-around without
    c = torch.tensor([[[-1, -1], [40, 40], [-1, 20], [-30, -40]]])
    for skip in (True, False):
        want = torch_stamp(c, half, H, W, values=v, skip_negative=skip)
        assert np.array_equal(poke_ref.stamp(c.numpy(), half, H, W, values=v.numpy(), skip_negative=skip), want.numpy())
    assert (torch_stamp(c, half, H, W, values=v) != 0).sum() == 2 * 25
    assert (torch_stamp(c, half, H, W, values=v, skip_negative=False)[0, 0] == 4.0).sum() == 25          # -30:-25 x -40:-35 wraps into the map


@pytest.mark.parametrize("B,H,W,half,n", [(2, 32, 48, 3, 6), (3, 64, 64, 2, 5), (1, 21, 13, 4, 12)])
def test_stamp_restatement_on_the_gpu_tests_inputs(B, H, W, half, n):
    """a non-square map among them; values given and values read from the flow at the centres"""
    centers, values, flow = poke_cases.stamp_case(B, H, W, half, n)
    assert np.array_equal(poke_ref.stamp(centers.numpy(), half, H, W, values=values.numpy()), torch_stamp(centers, half, H, W, values=values).numpy())
    assert np.array_equal(poke_ref.stamp(centers.numpy(), half, H, W, flow=flow.numpy()), torch_stamp(centers, half, H, W, flow=flow).numpy())


def torch_randomize(flow, centers, half, picked, u):
    """:815-828 with the pixel given: fp32 torch, Python's slicing"""
    B, _, H, W = flow.shape
    out = torch.zeros(u.shape[1], B, 2, H, W)
    for b in range(B):
        for j in range(u.shape[1]):
            if picked[b, j, 0] < 0:
                continue
            phase = torch.norm(flow[b, :, picked[b, j, 0], picked[b, j, 1]])
            angle = np.pi * u[b, j, 1:2]
            val = torch.tensor([torch.cos(angle) * phase, torch.sin(angle) * phase])[..., None, None]
            r, c = int(centers[b, 0, 0]), int(centers[b, 0, 1])
            out[j, b][:, r - half:r + half + 1, c - half:c + half + 1] = val
    return out


@pytest.mark.parametrize("case", poke_cases.CASES[:3])
def test_randomize_restatement_against_torch(case):
    """candidate set and order against ``nonzero`` of the reference's normalised fp32 amplitude (:798-808), pick mapping, values and support
    against the reference's fp32 lines"""
    B, H, W, half, n_s, n_c = case
    flow, centers, u = poke_cases.random_case(*case)
    assert (poke_cases.mean_gap(flow) > poke_cases.GAP).all()
    pokes, picked, status, phase = poke_ref.randomize(flow.numpy(), centers.numpy(), half, u.numpy())
    assert not status.any()
    amplitude = torch.norm(flow, 2, dim=1)
    amplitude = (amplitude - amplitude.amin((1, 2), keepdim=True)) / amplitude.amax((1, 2), keepdim=True)
    for b in range(B):
        valid = torch.gt(amplitude[b], amplitude[b].mean()).nonzero()
        assert np.array_equal(valid.numpy(), poke_ref.candidates(poke_ref.amplitude(flow.numpy())[b]))
        for j in range(n_s):
            k = min(int(np.floor(float(u[b, j, 0]) * len(valid))), len(valid) - 1)
            assert picked[b, j].tolist() == valid[k].tolist()
    want = torch_randomize(flow, centers, half, picked, u).numpy()
    assert np.array_equal(pokes != 0, want != 0)
    assert (np.abs(pokes - want) <= 8 * 2.0 ** -24 * phase.T[:, :, None, None, None]).all()


def test_randomize_restatement_edge_cases():
    flow, centers, u, want_status = poke_cases.edge_case()
    gap = poke_cases.mean_gap(flow)
    assert gap[2] == 0 and (np.delete(gap, 2) > poke_cases.GAP).all()
    pokes, picked, status, phase = poke_ref.randomize(flow.numpy(), centers.numpy(), 2, u.numpy())
    assert status.tolist() == want_status
    assert not pokes[:, [0, 2, 4]].any()                                     # empty slice / no candidate / padded centre
    assert (picked[1] == np.array([40, 13])).all() and (picked[[2, 4]] == -1).all() and (picked[0] >= 0).all()
    cand = poke_ref.candidates(poke_ref.amplitude(flow.numpy())[3])
    assert picked[3].tolist() == [cand[0].tolist(), cand[-1].tolist(), cand[0].tolist(), cand[-1].tolist()]    # u = 0 -> first, u -> 1 -> last
    assert (pokes[:, 3, 1] >= 0).all() and (pokes[0, 3, 0] > 0).any() and (pokes[2, 3, 0] < 0).any()            # the upper half plane


def test_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ipoke_poke_stamp", "ipoke_poke_randomize", "ipoke_poke_randomize_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    ws = _lib.lib().ipoke_poke_randomize_workspace_bytes
    assert ws(3, 64, 64, 4) == 3 * 4 * 2 * 4                                 # the amplitude map lives in LDS up to 128 x 128
    assert ws(1, 128, 128, 7) == 7 * 2 * 4 and ws(2, 144, 128, 3) == 2 * (3 * 2 + 144 * 128) * 4
    assert _lib.lib().ipoke_poke_stamp(None, None, None, 1, 8, 8, 1, 1, 1, None, None) == -1
    assert _lib.lib().ipoke_poke_randomize(None, None, None, 1, 8, 8, 1, 1, 1, None, None, None, None, None) == -1


def _model():
    arch = configs.flow_arch(32, hidden=64, num_steps=[2, 1, 1], factor=4)
    arch["flow_mid_channels_factor"] = 2
    conf = configs.second_stage_config(64, 32, 16, batch_size=2, arch=arch)
    return PokeMotionModel(conf, dirs={}, dtype="f32", device="cpu", max_batch=2)


def test_public_methods_exist_and_need_the_gpu():
    m = _model()
    sim = PokeSimulator(poke_cases.simulator_config(64, 64, 2, 5))
    for obj, name in ((m, "transfer_motion"), (m, "control_sensitivity_samples"), (sim, "stamp"), (sim, "randomize_pokes")):
        assert callable(getattr(obj, name, None)), name
    if torch.cuda.is_available():
        return                                                               # the errors below are those of a machine without a GPU
    batch = synthetic_batch(1, 16, 64)
    batch["nn"] = (batch["images"], batch["flow"], batch["sample_ids"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.transfer_motion(batch)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.control_sensitivity_samples(batch, n_pokes=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sim.stamp(batch["poke"][1], flow=batch["flow"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        sim.randomize_pokes(batch["flow"], batch["poke"][1], 2)


def test_public_methods_are_named_by_the_test_loop_errors():
    m = _model()
    assert callable(m.transfer_motion) and callable(m.control_sensitivity_samples)
    assert "transfer_motion" in m._TEST_MODES_MISSING["transfer"] and "control_sensitivity_samples" in m._TEST_MODES_MISSING["control_sensitivity"]
