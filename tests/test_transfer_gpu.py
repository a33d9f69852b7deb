"""Motion transfer and the control-sensitivity samples (``PokeMotionModel.transfer_motion`` / ``control_sensitivity_samples``; reference
second_stage_video.py:786-852, 948-1015) on the reduced f32 model of tests/test_test_modes_gpu.py (64 x 64, T = 16, B = 2,
num_steps = [2, 1, 1], deterministic fill) with a poke embedder that takes the poke AND the start frame -- the only configuration in
which the reference's transfer runs.  Batches come from ``PokeSimulator.make_batch`` on seeded raw flows (real poke centres).

Bounds, all taken from existing tests: the f32 forward -> reverse round trip of a flow of this class, 4 x TOL["f32"]["rev"]
(tests/test_flow_gpu.py::test_condition_nice_wide_vs_oracle); against the CPU oracle the f32 bound of
tests/test_second_stage_options_gpu.py::test_condition_nice_second_stage (2e-4) for the latents and the videos.

The flow of this model is filled, not trained: its reverse pass is only tame near the conditioning a residual was computed under (in the
CPU oracle too, a residual reversed under an unrelated clip's conditioning, or a unit normal one, overflows to inf / nan).  So clip 2 is
clip 1 with 5 % noise on its frames, the comparison with the oracle feeds a residual of standard deviation 0.25 to both sides, and the
bit-for-bit comparisons are made on the bit patterns, which also holds where a value is not finite."""
import copy

import pytest
import torch

from ipoke_amd import configs
from ipoke_amd.data import FlowError, PokeSimulator
from ipoke_amd.second_stage import PokeMotionModel
from ipoke_amd.utils.detfill import deterministic_fill_
from tests.helpers import synthetic_batch
from tests.test_flow_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROUND_TRIP_F32 = 4 * TOL["f32"]["rev"]
ORACLE_F32 = 2e-4


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def _config(poke_and_image=True):
    arch = configs.flow_arch(32, hidden=64, num_steps=[2, 1, 1], factor=4)
    arch["flow_mid_channels_factor"] = 2
    conf = configs.second_stage_config(64, 32, 16, batch_size=2, arch=arch)
    conf["testing"]["n_control_sensitivity_pokes"] = 3
    if poke_and_image:
        conf["poke_embedder"] = configs.encoder2d_config(64, 2, flow_ae=False)
        conf["poke_embedder"]["architecture"]["poke_and_image"] = True
    return conf


def _build(poke_and_image=True):
    model = PokeMotionModel(_config(poke_and_image), dirs={}, dtype="f32", device=DEV, max_batch=2)
    for name in ("first_stage_model", "poke_embedder", "conditioner", "flow"):
        deterministic_fill_(getattr(model, name), prefix=name + ".")
    model.flow.sync_buffers()
    return model


@pytest.fixture(scope="module")
def model():
    return _build()


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    images = (torch.rand(2, 16, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    raw_flow = torch.randn(2, 2, 64, 64, generator=g).to(DEV)
    u = torch.rand(2, 11, generator=g).to(DEV)
    batch = PokeSimulator(_config()["data"]).make_batch(images, raw_flow, u=u)
    assert not batch["poke_status"].any() and (batch["poke"][1][:, 0] >= 0).all() and batch["poke"][0].any()
    batch["sample_ids"] = torch.arange(seed, seed + 2, device=DEV)[:, None].repeat(1, 16)
    return batch


@pytest.fixture(scope="module")
def batches():
    b1, b2 = _batch(31), _batch(32)
    noise = torch.randn(b1["images"].shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    b1["nn"] = ((b1["images"] + 0.05 * noise).clamp(-1, 1), b2["flow"], b2["sample_ids"])
    return b1, b2


def test_transfer_equals_the_steps_composed_by_hand(model, batches):
    batch, _ = batches
    torch.manual_seed(41)
    got = model.transfer_motion(batch)
    assert set(got) == {"r1", "z_r1_cond2", "z_random_cond2", "vid_r1_c2", "vid_random_cond2"} and all(v.is_cuda for v in got.values())
    assert got["r1"].shape == (2, 32, 8, 8) and got["vid_r1_c2"].shape == (2, 15, 3, 64, 64)
    torch.manual_seed(41)
    with torch.no_grad():
        X_2, poke1 = batch["nn"][0], batch["poke"][0]
        z_1, cond_1 = model.make_flow_input(batch)
        poke_emb, *_ = model.poke_embedder.encoder(torch.cat([poke1, X_2[:, 0]], dim=1))
        cond_2, *_ = model.conditioner.encoder(X_2[:, 0])
        cond_2 = torch.cat([cond_2, poke_emb], dim=1)
        r1, _ = model.flow(z_1, cond_1, reverse=False)
        z_a = model.flow(r1, cond_2, reverse=True)
        z_b = model.flow(torch.randn(r1.shape).type_as(r1), cond_2, reverse=True)
        want = {"r1": r1, "z_r1_cond2": z_a, "z_random_cond2": z_b, "vid_r1_c2": model.decode_first_stage(z_a, X_2),
                "vid_random_cond2": model.decode_first_stage(z_b, X_2)}
    for k in want:
        assert bits_equal(got[k], want[k]), k
    assert torch.isfinite(got["vid_r1_c2"]).all() and not bits_equal(got["z_r1_cond2"], z_1)
    torch.manual_seed(41)
    again = model.transfer_motion(batch)
    assert all(bits_equal(again[k], got[k]) for k in got)


def test_transfer_onto_the_same_clip_is_the_reconstruction(model, batches):
    batch, _ = batches
    same = dict(batch)
    same["nn"] = (batch["images"], batch["flow"], batch["sample_ids"])
    torch.manual_seed(43)
    got = model.transfer_motion(same)
    torch.manual_seed(43)
    with torch.no_grad():
        z_1, _ = model.make_flow_input(same)
        recon = model.decode_first_stage(z_1, same["images"])
    e_z = (got["z_r1_cond2"] - z_1).abs().max().item()
    e_v = (got["vid_r1_c2"] - recon).abs().max().item()
    print(f"identity transfer: latent err {e_z:.3e} (|z| max {z_1.abs().max().item():.2f}), video err {e_v:.3e}; bound {ROUND_TRIP_F32:.1e}")
    assert e_z <= ROUND_TRIP_F32 and e_v <= ROUND_TRIP_F32


def test_transfer_against_the_oracle(model, batches):
    from oracle import flow_ref, vae_ref
    batch, _ = batches
    conf = model.config
    cpu = lambda m, ref: (ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}), ref.eval())[1]
    o_fs = cpu(model.first_stage_model, vae_ref.SpadeCondMotionModel(conf["first_stage"]))
    o_pe = cpu(model.poke_embedder, vae_ref.FirstStageWrapper(conf["poke_embedder"]))
    o_co = cpu(model.conditioner, vae_ref.FirstStageWrapper(conf["conditioner_model"]))
    o_fl = cpu(model.flow, flow_ref.SupervisedMacowTransformer(copy.deepcopy(conf["architecture"])))
    residual = 0.25 * torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(5))
    real = torch.randn
    torch.randn = lambda *a, **k: residual.clone()                   # the one randn of the function: the same residual on both sides
    try:
        torch.manual_seed(47)
        got = model.transfer_motion(batch)
    finally:
        torch.randn = real
    torch.manual_seed(47)
    with torch.no_grad():
        X_1, X_2, poke1 = batch["images"].cpu(), batch["nn"][0].cpu(), batch["poke"][0].cpu()
        emb_1, *_ = o_pe.encoder(torch.cat([poke1, X_1[:, 0]], dim=1))
        cond_1 = torch.cat([o_co.encoder(X_1[:, 0])[0], emb_1], dim=1)
        z_1, _, _ = o_fs.enc_motion(X_1.transpose(1, 2))            # full_sequence; the noise from the CPU generator, as on the device path
        emb_12, *_ = o_pe.encoder(torch.cat([poke1, X_2[:, 0]], dim=1))
        cond_2 = torch.cat([o_co.encoder(X_2[:, 0])[0], emb_12], dim=1)
        r1, _ = o_fl(z_1, cond_1)
        z_a = o_fl(r1, cond_2, reverse=True)
        z_b = o_fl(residual, cond_2, reverse=True)
        want = {"r1": r1, "z_r1_cond2": z_a, "z_random_cond2": z_b, "vid_r1_c2": o_fs.decode(z_a, X_2[:, 0], 15),
                "vid_random_cond2": o_fs.decode(z_b, X_2[:, 0], 15)}
    errs = {k: (got[k].cpu() - want[k]).abs().max().item() for k in want}
    print("transfer against the oracle: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f"; bound {ORACLE_F32:.1e}")
    assert all(torch.isfinite(v).all() for v in want.values())
    assert all(e <= ORACLE_F32 for e in errs.values()), errs


def test_control_sensitivity_samples(model, batches):
    batch, _ = batches
    poke_obj = batch["poke"]
    u = torch.rand(2, 3, 2, generator=torch.Generator().manual_seed(3)).to(DEV)
    torch.manual_seed(51)
    pokes, samples, picked, status = model.control_sensitivity_samples(batch, u=u)
    assert batch["poke"] is poke_obj and "nn" in batch
    assert pokes.shape == (4, 2, 2, 64, 64) and samples.shape == (2, 4, 15, 3, 64, 64) and picked.shape == (2, 3, 2) and not status.any()
    assert samples.is_cuda and torch.equal(pokes[0], batch["poke"][0])
    sim = PokeSimulator(model.config["data"])
    want = sim.randomize_pokes(batch["flow"], batch["poke"][1], 3, u=u)
    assert torch.equal(pokes[1:], want[0]) and torch.equal(picked, want[1]) and pokes[1:].any()
    torch.manual_seed(51)
    for k in range(4):                                                                       # one latent per poke, in order
        video = model.forward_sample(dict(batch, poke=pokes[k]), 1, n_logged_vids=2)[0]
        assert bits_equal(samples[:, k], video), k
    # uniforms drawn by the method: first the uniforms (device generator), then the latents
    torch.manual_seed(52)
    a = model.control_sensitivity_samples(batch, n_pokes=1)
    torch.manual_seed(52)
    b = model.control_sensitivity_samples(batch, n_pokes=1)
    assert all(bits_equal(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape[0] == 2
    # the captured sampling graph: warm-up call, capture, replay -- all bit-identical to eager
    model.set_sample_graph(True)
    try:
        for _ in range(2):
            torch.manual_seed(51)
            g = model.control_sensitivity_samples(batch, u=u)
            assert bits_equal(g[1], samples) and torch.equal(g[0], pokes)
    finally:
        model.set_sample_graph(False)


def test_control_sensitivity_flags_a_constant_flow(model, batches):
    batch, _ = batches
    flat = dict(batch)
    flat["flow"] = batch["flow"].clone()
    flat["flow"][1, 0], flat["flow"][1, 1] = 0.5, -0.25
    u = torch.rand(2, 2, 2)
    state = torch.get_rng_state()
    with pytest.raises(FlowError, match=r"samples \[1\]"):
        model.control_sensitivity_samples(flat, n_pokes=2, u=u)
    assert torch.equal(torch.get_rng_state(), state)                                         # raised before any latent was drawn


def test_all_zero_centres_stamp_nothing(model):
    """``synthetic_batch`` has every centre at (0, 0): the empty slice 62:3, so the randomized pokes are all zero (and still sampled)"""
    batch = synthetic_batch(2, 16, 64, seed=3, device=DEV)
    torch.manual_seed(53)
    pokes, samples, picked, status = model.control_sensitivity_samples(batch, n_pokes=2)
    assert not status.any() and (picked >= 0).all() and not pokes[1:].any() and torch.equal(pokes[0], batch["poke"][0])
    assert samples.shape == (2, 3, 15, 3, 64, 64)


def test_transfer_without_poke_and_image_explains_itself(batches):
    batch, _ = batches
    model = PokeMotionModel(_config(poke_and_image=False), dirs={}, dtype="f32", device=DEV, max_batch=2)
    with pytest.raises(NotImplementedError, match="NameError.*poke1_src2"):
        model.transfer_motion(batch)
