"""Clip augmentation on the device (csrc/data.hip ``ipoke_aug_frame_means`` / ``ipoke_aug_frames`` / ``ipoke_aug_flow``, ``ClipAugmenter`` and
``PokeSimulator.make_batch(augment=...)`` in ipoke_amd/data.py) against golden G18, which Pillow computed (scripts/make_augment_goldens.py)
and tests/test_augment_cpu.py pins against the numpy restatement.

Everything is bit-equal: the colour chain works on uint8 values with every float step at Pillow's precision and rounding, the geometry is
Pillow's 16.16 fixed point in integers, the flow is copied.  The golden stores uint8; the fp32 expectation is ``(u / 255) * 2 - 1`` in numpy
fp32, one IEEE operation per step.  Outputs are written into sentinel-filled buffers with guard zones on both sides: every element must be
written, none outside."""
import numpy as np
import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd.data import ClipAugmenter, PokeSimulator
from tests import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
SENT = {torch.float32: -77777.0, torch.int32: -777777}
N_CASES = 5


class Guarded:
    """``numel`` elements of a sentinel between two guard zones of it; ``view`` is what the kernel gets"""

    def __init__(self, shape, dtype):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + self.n].view(self.shape)

    def check(self, what):
        s = SENT[self.buf.dtype]
        assert bool((self.buf[:GUARD] == s).all()) and bool((self.buf[GUARD + self.n:] == s).all()), f"{what}: write outside the output"
        assert not bool((self.view == s).any()), f"{what}: elements left unwritten"
        return self.view


def case(g, ci):
    return {k: g[f"{k}{ci}"] for k in ("frames", "colour", "hue", "hue_add", "angle", "trans", "affine", "mean_l", "out", "flow", "flow_out")}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def params_of(c, S):
    aug = ClipAugmenter({"augment": True, "spatial_size": (S, S)})
    return aug, aug.params(c["colour"][:, 0], c["colour"][:, 1], c["colour"][:, 2], c["hue"], c["angle"], c["trans"][:, 0], c["trans"][:, 1], device=DEV)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_raw_entry_points_are_bit_equal_to_pillow(golden, ci):
    c = case(golden("g18_augment"), ci)
    B, T, S = c["frames"].shape[:3]
    frames, colour, hue_add, affine, flow = dev(c["frames"]), dev(c["colour"]), dev(c["hue_add"]), dev(c["affine"]), dev(c["flow"])
    mean_l, out, warped = Guarded((B, T), torch.int32), Guarded((B, T, 3, S, S), torch.float32), Guarded((B, 2, S, S), torch.float32)
    lib, stream = _lib.lib(), _lib.current_stream()
    _lib.check(lib.ipoke_aug_frame_means(_lib.ptr(frames), _lib.ptr(colour), B, T, S, _lib.ptr(mean_l.view), stream))
    _lib.check(lib.ipoke_aug_frames(_lib.ptr(frames), _lib.ptr(colour), _lib.ptr(hue_add), _lib.ptr(mean_l.view), _lib.ptr(affine), B, T, S,
                                    _lib.ptr(out.view), stream))
    _lib.check(lib.ipoke_aug_flow(_lib.ptr(flow), _lib.ptr(affine), B, 2, S, _lib.ptr(warped.view), stream))
    torch.cuda.synchronize()
    assert np.array_equal(mean_l.check("mean_l").cpu().numpy(), c["mean_l"])
    got = out.check("out").cpu().numpy()
    want = R.to_float(c["out"])
    assert got.dtype == want.dtype == np.float32 and want.shape == got.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} values differ"
    assert np.array_equal(warped.check("flow").cpu().numpy(), c["flow_out"])
    # the public methods, on a stream of their own: the same bits, [B, S, S, 3] -> [B, 3, S, S], and mean_l left in the parameters
    aug, p = params_of(c, S)
    assert torch.equal(p.affine, affine) and torch.equal(p.hue_add, hue_add) and torch.equal(p.colour, colour)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api, api_flow = aug.images(frames, p), aug.flow(flow, p)
        first = aug.images(frames[:, 0], p)
    side.synchronize()
    assert torch.equal(api, out.view) and torch.equal(api_flow, warped.view)
    assert first.shape == (B, 3, S, S) and torch.equal(first, out.view[:, 0]) and torch.equal(p.mean_l, mean_l.view[:, :1])


def test_frames_of_a_clip_share_the_parameters_and_not_the_mean(golden):
    """a clip of T frames == T single-frame launches with the same parameter set; samples do not read each other's parameters"""
    c = case(golden("g18_augment"), 2)
    B, T, S = c["frames"].shape[:3]
    aug, p = params_of(c, S)
    frames = dev(c["frames"])
    whole = aug.images(frames, p)
    assert len(set(c["mean_l"][0].tolist())) > 1
    for t in range(T):
        assert torch.equal(aug.images(frames[:, t].contiguous(), p), whole[:, t])
    for b in range(B):
        one = aug.params(*(v[b:b + 1] for v in (c["colour"][:, 0], c["colour"][:, 1], c["colour"][:, 2], c["hue"], c["angle"], c["trans"][:, 0],
                                                c["trans"][:, 1])), device=DEV)
        assert torch.equal(aug.images(frames[b:b + 1], one), whole[b:b + 1])


def test_make_batch_with_augmentation(golden):
    c = case(golden("g18_augment"), 2)
    B, T, S = c["frames"].shape[:3]
    aug, p = params_of(c, S)
    sim = PokeSimulator({"spatial_size": (S, S), "n_pokes": 5, "poke_size": 5, "scale_poke_to_res": True})
    gen = torch.Generator(device=DEV).manual_seed(4)
    raw = torch.nn.functional.interpolate(torch.randn(B, 2, 6, 6, device=DEV, generator=gen), size=(2 * S, 2 * S), mode="bicubic") * 10
    u = torch.rand(B, 11, device=DEV, generator=gen)
    frames = dev(c["frames"])
    zero = torch.tensor([False, True])
    batch = sim.make_batch(None, raw, zero, u, augment=p, frames_u8=frames)
    # images: the golden's; flow: the warp of get_flow, zeroed for the zero-poke sample; pokes: get_poke of the warped flow
    assert np.array_equal(batch["images"].cpu().numpy(), R.to_float(c["out"]))
    warped = aug.flow(sim.get_flow(raw), p)
    assert np.array_equal(warped.cpu().numpy(), R.augment_flow(sim.get_flow(raw).cpu().numpy(), c["affine"]))
    poke, centers, flow_out, status = sim.get_poke(warped, zero, u, strict=False)
    assert torch.equal(batch["poke"][0], poke) and torch.equal(batch["poke"][1], centers) and torch.equal(batch["poke_status"], status)
    assert torch.equal(batch["flow"], flow_out) and torch.equal(flow_out[0], warped[0]) and not flow_out[1].any()
    assert int(status.sum()) == 0 and poke.any()
    r, col = centers[0, int((centers[0, :, 0] >= 0).sum()) - 1].tolist()                        # the last poke is never overwritten
    assert torch.equal(poke[0, :, r, col], warped[0, :, r, col])
    # without the new arguments: what the method returned before them
    images = torch.zeros(B, T, 3, S, S, device=DEV)
    plain = sim.make_batch(images, raw, zero, u)
    flow = sim.get_flow(raw)
    poke0, centers0, flow_out0, status0 = sim.get_poke(flow, zero, u, None, strict=False)
    assert sorted(plain) == ["flow", "images", "poke", "poke_status"] and plain["images"] is images
    assert torch.equal(plain["flow"], flow_out0) and torch.equal(plain["poke"][0], poke0) and torch.equal(plain["poke"][1], centers0)
    assert torch.equal(plain["poke_status"], status0) and torch.equal(flow_out0[0], flow[0])
    assert not torch.equal(plain["poke"][0], poke)                                              # the warp moved the pokes' source
    with pytest.raises(ValueError, match="frames_u8"):
        sim.make_batch(images, raw, zero, u, augment=p)
