"""Inputs shared by tests/test_poke_edit_cpu.py and tests/test_poke_edit_gpu.py: seeded flows, centres and uniforms for ``stamp`` /
``randomize_pokes``, and the condition under which the picks of ``randomize_pokes`` can be compared exactly."""
import numpy as np
import torch

from tests import poke_ref

# (B, H, W, half, n_s, n_c); the last one is past the 128 x 128 map that the kernel keeps in LDS (its workspace path)
CASES = [(3, 64, 64, 2, 4, 5), (2, 32, 48, 3, 1, 1), (1, 128, 128, 5, 7, 5), (1, 144, 128, 5, 3, 2)]
GAP = 1e-5
U_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))      # the largest fp32 below 1


def simulator_config(H, W, half, n_c):
    return {"spatial_size": (H, W), "poke_size": 2 * half + 1, "n_pokes": n_c}


def random_case(B, H, W, half, n_s, n_c):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B)
    flow = torch.randn(B, 2, H, W, generator=g)
    centers = torch.stack([torch.randint(0, H, (B, n_c), generator=g), torch.randint(0, W, (B, n_c), generator=g)], dim=-1)
    if n_c > 2:
        centers[:, -1] = -1                                         # a padding row
        centers[0, 1] = centers[0, 0] + 1                           # overlapping squares
    centers[0, 0] = torch.tensor([H - 1 - half, half])              # last row / first column of the window in which the square is whole
    u = torch.rand(B, n_s, 2, generator=g)
    return flow, centers, u


def edge_case():
    """B = 5 at 64 x 64, half = 2, n_s = 4: 0 first centre (0, 0) (the empty slice 62:3: nothing stamped, status 0); 1 exactly one candidate;
    2 constant amplitude (status 1); 3 u = 0 and u = the largest fp32 below 1; 4 a padded first centre (status 2)."""
    g = torch.Generator().manual_seed(77)
    flow = torch.randn(5, 2, 64, 64, generator=g)
    flow[1] = 0.0
    flow[1, :, 40, 13] = torch.tensor([0.75, -1.5])
    flow[2, 0], flow[2, 1] = 3.0, -4.0
    centers = torch.tensor([[0, 0], [20, 30], [31, 31], [63, 63], [-1, -1]]).view(5, 1, 2).repeat(1, 2, 1)
    centers[:, 1] = torch.tensor([10, 50])
    u = torch.rand(5, 4, 2, generator=g)
    u[3, :, 0] = torch.tensor([0.0, U_MAX, 0.0, U_MAX])
    u[3, :, 1] = torch.tensor([0.0, 0.0, U_MAX, U_MAX])
    return flow, centers, u, [0, 0, 1, 0, 2]


def mean_gap(flow):
    """per sample: the smallest |amplitude - mean| / mean.  The kernel's threshold is a double mean of fp32 amplitudes, the reference's an
    fp32 mean, the restatement's a float64 mean of float64 amplitudes: they differ by ~1e-7 relative, so exact picks are only defined for
    inputs without an amplitude that close to the mean (a constant map, whose every amplitude IS the mean, is the status-1 case and has no
    picks to compare)."""
    amp = poke_ref.amplitude(flow.numpy())
    mean = amp.reshape(len(amp), -1).mean(1)
    return np.abs(amp - mean[:, None, None]).reshape(len(amp), -1).min(1) / mean


def stamp_case(B, H, W, half, n):
    """centres on every edge of the map and of the window in which the square is whole, overlaps, (0, 0), -1 rows"""
    g = torch.Generator().manual_seed(H * W + n)
    special = torch.tensor([[0, 0], [half, half], [half - 1, W // 2], [H - 1 - half, W - 1 - half], [H - half, W // 2], [H - 1, W - 1],
                            [H // 2, half - 1], [H // 2, W - half], [H // 2, W // 2], [H // 2 + 1, W // 2 + 1], [0, W - 1], [-1, -1]])
    centers = torch.stack([torch.randint(0, H, (B, n), generator=g), torch.randint(0, W, (B, n), generator=g)], dim=-1)
    for b in range(B):
        idx = torch.randperm(len(special), generator=g)[:max(n - 1, 1)]
        centers[b, :len(idx)] = special[idx]
    values = torch.randn(B, n, 2, generator=g)
    flow = torch.randn(B, 2, H, W, generator=g)
    return centers, values, flow
