"""The kernels of the device data path (csrc/data.hip) one by one against the restatements of tests/data_exact.py, at small awkward shapes:

    ipoke_flow_resize      a derived per-element bound against the float64 interpolant of the fp32 quotient, and bit-exact wherever the
                           kernel's arithmetic rounds at most once
    ipoke_poke_simulate    (poke_select_kernel<false> + poke_fill_kernel) bit-exact: centres, status, poke, returned flow, and the normalised
                           amplitude the selection kernel leaves in the caller's workspace
    ipoke_flow_mask        bit-exact at the window sizes around the 1024-thread block

This is index work: one wrong element is another training sample, not a small error.  tests/test_data_exact_cpu.py shows that no decision
of any case used here can hinge on the order of a sum, so equality is asked for, not closeness."""
import functools

import numpy as np
import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd._lib import check, ptr
from ipoke_amd.data import FlowError, PokeSimulator
from tests import data_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 1024                      # sentinel elements behind an output buffer
NAMES = [c.name for c in X.cases() + X.tie_cases()]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------ flow resize
def _resize(x, Ho, Wo, div):
    B, C, Hi, Wi = x.shape
    n = B * C * Ho * Wo
    src = torch.from_numpy(x).to(DEV)
    full = torch.full((n + TAIL,), -12345.5, dtype=torch.float32, device=DEV)
    check(_lib.lib().ipoke_flow_resize(ptr(src), ptr(full), B, C, Hi, Wi, Ho, Wo, float(div), _lib.current_stream()))
    torch.cuda.synchronize()
    assert bool((full[n:] == -12345.5).all()), "written behind the output"
    return full[:n].view(B, C, Ho, Wo).cpu().numpy()


def test_flow_resize_within_the_derived_bound():
    """|got - ref| <= 2^-23 (8 m + 2 (Hi - 1) sy + 2 (Wi - 1) sx) per element (data_exact.resize_bound), on every shape, divisor and input."""
    worst, where = 0.0, None
    for i, (shape, (Ho, Wo), _) in enumerate(X.RESIZE_SHAPES):
        for k, x in enumerate(X.resize_inputs(shape, 100 + i)):
            for div in X.RESIZE_DIVS:
                got = _resize(x, Ho, Wo, div)
                ref, m, sy, sx = X.resize_ref(x, Ho, Wo, div)
                bound = X.resize_bound(m, sy, sx, shape[2], shape[3])
                err = np.abs(got.astype(np.float64) - ref)
                ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
                if not ratio <= worst:
                    worst, where = ratio, (shape, (Ho, Wo), div, k)
    print(f"flow resize: worst error / bound = {worst:.4f} at {where}")
    assert worst <= 1.0, (worst, where)


def test_flow_resize_exact_where_every_weight_is_zero():
    """the identity shape and the integer-ratio shape: the output is fl32(src / div) at the tap, bit for bit"""
    for i, (shape, (Ho, Wo), kind) in enumerate(X.RESIZE_SHAPES):
        if not kind:
            continue
        ys = np.arange(Ho) * ((shape[2] - 1) // max(Ho - 1, 1))
        xs = np.arange(Wo) * ((shape[3] - 1) // max(Wo - 1, 1))
        for x in X.resize_inputs(shape, 100 + i):
            for div in X.RESIZE_DIVS:
                want = (x / np.float32(div)).astype(np.float32)[:, :, ys[:, None], xs[None, :]]
                assert np.array_equal(_bits(_resize(x, Ho, Wo, div)), _bits(want)), (shape, kind, div)


@pytest.mark.parametrize("shape,out", [((1, 2, 1, 33), (1, 65)), ((2, 1, 33, 1), (65, 1))])
def test_flow_resize_exact_at_half_weights(shape, out):
    """One axis, ratio 1/2: every weight is 0 or 0.5, the coordinate is exact, and 0.5 a + 0.5 b rounds once, fused or not; so the output
    is the float64 interpolant of the fp32 quotients rounded to fp32, bit for bit.  A division after the interpolation rounds the
    quotient of the mean instead and differs in the last bit of some elements for a divisor of 3."""
    x = X._mantissas(np.random.RandomState(7), shape, 16.0)
    for div in X.RESIZE_DIVS:
        ref = X.resize_ref(x, out[0], out[1], div)[0]
        want = ref.astype(np.float32)
        assert np.array_equal(_bits(_resize(x, out[0], out[1], div)), _bits(want)), (shape, div)
    after = (X.resize_ref(x, out[0], out[1], 1.0)[0].astype(np.float32) / np.float32(3.0)).astype(np.float32)
    assert not np.array_equal(_bits(after), _bits(X.resize_ref(x, out[0], out[1], 3.0)[0].astype(np.float32))), "the case cannot tell the two orders apart"


# ------------------------------------------------------------------------------------------------------------------ poke select + fill
def _simulate(batch):
    """ipoke_poke_simulate on the samples of ``batch`` (one geometry) with a workspace of the caller's -> numpy (poke, centers, flow_out,
    status, amp [B, n]): the normalised amplitude is the first B n floats of the workspace (ipoke_poke_workspace_bytes, include/ipoke_hip.h)"""
    c0 = batch[0]
    B, H, W, n = len(batch), c0.H, c0.W, c0.n
    lib = _lib.lib()
    flow = torch.from_numpy(np.stack([c.flow for c in batch])).to(DEV)
    u = torch.from_numpy(np.stack([c.u for c in batch])).to(DEV)
    zero = torch.tensor([int(c.zero) for c in batch], dtype=torch.int32, device=DEV)
    poke, flow_out = torch.full_like(flow, -7.5), torch.full_like(flow, -7.5)
    centers = torch.full((B, c0.n_pokes, 2), -7777, dtype=torch.int64, device=DEV)
    status = torch.full((B,), -7777, dtype=torch.int32, device=DEV)
    nbytes = int(lib.ipoke_poke_workspace_bytes(B, H, W, c0.ps, c0.n_pokes))
    assert nbytes == B * (n * 4 + (1 + 4 * c0.n_pokes) * 4)
    ws = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    check(lib.ipoke_poke_simulate(ptr(flow), B, H, W, c0.ps, c0.n_pokes, int(c0.fix), int(c0.equal), ptr(zero), ptr(u), ptr(poke), ptr(centers),
                                  ptr(flow_out), ptr(status), ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "written behind the workspace"
    amp = ws[:B * n * 4].view(torch.float32).view(B, n)
    return tuple(v.cpu().numpy() for v in (poke, centers, flow_out, status, amp))


@functools.lru_cache(maxsize=None)
def _single(name):
    return _simulate([X.case(name)])


def _want(c):
    sel = X.select_ref(c.flow, c.ps, c.n_pokes, c.fix, c.zero, c.u)
    poke, flow_out = X.fill_ref(c.flow, sel, c.zero, c.ps // 2, c.equal)
    return sel, poke, flow_out


@pytest.mark.parametrize("name", NAMES)
def test_select_and_fill_bit_exact(name):
    """centres (int64, -1 padded), status, poke and returned flow of the unmasked launch pair == select_ref / fill_ref, and the public
    method is the same launch"""
    c = X.case(name)
    sel, want_poke, want_flow = _want(c)
    poke, centers, flow_out, status, _ = _single(name)
    assert status.tolist() == [sel.status] == [0]
    assert centers.dtype == np.int64 and np.array_equal(centers[0], sel.centers), (centers[0].tolist(), sel.centers.tolist())
    assert np.array_equal(_bits(poke[0]), _bits(want_poke))
    assert np.array_equal(_bits(flow_out[0]), _bits(want_flow))
    sim = PokeSimulator({"spatial_size": (c.H, c.W), "n_pokes": c.n_pokes, "poke_size": c.ps, "fix_n_pokes": c.fix, "equal_poke_val": c.equal})
    pub = sim.get_poke(torch.from_numpy(c.flow).unsqueeze(0).to(DEV), torch.tensor([c.zero]), torch.from_numpy(c.u).unsqueeze(0).to(DEV))
    for got, ours in zip(pub, (poke, centers, flow_out, status)):
        assert np.array_equal(got.cpu().numpy(), ours)


@pytest.mark.parametrize("name", NAMES)
def test_amplitude_is_not_contracted(name):
    """The normalised amplitude the selection kernel leaves in the workspace == select_ref's, BIT FOR BIT.  This is the check that pins
    "fp32 without contraction": numpy rounds vx vx, vy vy, their sum and the root one by one, and so must the kernel.  A fused
    fma(vx, vx, vy vy) differs from that in the last bit of a fraction of the elements and is wrong here, since a threshold comparison
    downstream may flip on it -- which is why the comparison is exact and not a tolerance."""
    c = X.case(name)
    amp = _single(name)[4]
    want = X.select_ref(c.flow, c.ps, c.n_pokes, c.fix, c.zero, c.u).amp
    assert amp.shape == (1, c.n) and np.array_equal(_bits(amp[0]), _bits(want.flatten()))


def test_batch_of_five_with_a_flagged_sample():
    """ordinary and zero-poke samples around a constant-flow sample in one launch, strict=False: the constant sample is flagged (status 1,
    centres -1, an all-zero poke), every other sample equals its single-sample result and the restatement bit for bit"""
    batch = X.batch_of_five()
    c0 = batch[0]
    sim = PokeSimulator({"spatial_size": (c0.H, c0.W), "n_pokes": c0.n_pokes, "poke_size": c0.ps, "fix_n_pokes": c0.fix, "equal_poke_val": c0.equal})
    flow = torch.from_numpy(np.stack([c.flow for c in batch])).to(DEV)
    zero = torch.tensor([c.zero for c in batch])
    u = torch.from_numpy(np.stack([c.u for c in batch])).to(DEV)
    poke, centers, flow_out, status = (v.cpu().numpy() for v in sim.get_poke(flow, zero, u, strict=False))
    assert status.tolist() == [0, 0, 1, 0, 0]
    assert (centers[2] == -1).all() and not poke[2].any()
    with pytest.raises(FlowError):
        sim.get_poke(flow, zero, u)
    raw = _simulate(batch)
    for got, ours in zip(raw[:4], (poke, centers, flow_out, status)):
        assert np.array_equal(got, ours)
    for j, c in enumerate(batch):
        if j == 2:
            continue
        one = _single(c.name)
        sel, want_poke, want_flow = _want(c)
        assert np.array_equal(centers[j], one[1][0]) and np.array_equal(centers[j], sel.centers), c.name
        assert np.array_equal(_bits(poke[j]), _bits(one[0][0])) and np.array_equal(_bits(poke[j]), _bits(want_poke)), c.name
        assert np.array_equal(_bits(flow_out[j]), _bits(one[2][0])) and np.array_equal(_bits(flow_out[j]), _bits(want_flow)), c.name
        assert np.array_equal(_bits(raw[4][j]), _bits(one[4][0])), c.name


# ------------------------------------------------------------------------------------------------------------------ flow mask
@pytest.mark.parametrize("H,W,flows", X.mask_flows(), ids=[f"{H}x{W}" for H, W in X.MASK_SHAPES])
def test_flow_mask_bit_exact(H, W, flows):
    """a smooth, a flat and a constant map per shape == poke_mask_ref.flow_mask; the constant one is flagged and its mask empty"""
    sim = PokeSimulator({"spatial_size": (H, W), "n_pokes": 1, "poke_size": 1})
    mask, status = sim.flow_mask(torch.from_numpy(flows).to(DEV))
    want = [X.flow_mask_ref(f) for f in flows]
    assert status.tolist() == [w[1] for w in want] == [0, 0, 1]
    for j, (wm, _, ok) in enumerate(want):
        assert ok
        assert torch.equal(mask[j].cpu(), wm), (H, W, j)
    assert not bool(mask[2].any())
    assert H * W == 2 or (bool(mask[0].any()) and bool(mask[1].any()))
