"""The image autoencoder's adversarial phase (ipoke_amd/image_gan.py, csrc/image_gan.hip), host side.

* The plain-torch comparator tests/image_gan_ref.py in float64 against golden ``g22_image_gan`` (the reference's own ``ConvEncoder``,
  ``ConvDecoder``, ``define_D``, ``calculate_adaptive_weight``, scripts/make_goldens_image_gan.py): every value to 1e-6 relative.
  "Relative" is to max(1, |ref|) for a scalar, to the largest entry of the tensor for maps and sampled entries, and to the reference's
  abs-sum for the two checksums of a tensor.  The golden holds the reference's float64 run: its fp32 run carries 5e-6 of rounding of
  its own on the reconstruction, more than this bound (the script keeps the fp32 run as a conditioning check).
* State-dict names of ``NLayerDiscriminator`` / ``ConvAEGANModel``, the checkpoint path into the second stage, the kernels' refusals,
  the two-scheduler sequence against torch's, and the exported symbols.
"""
import ctypes

import numpy as np
import pytest
import torch

from ipoke_amd import _lib, configs
from ipoke_amd._lib import ptr
from ipoke_amd.utils.detfill import deterministic_fill_
from tests import image_gan_ref as R
from tests.conftest import t

REL = 1e-6
SCALARS = ("loss", "kl_loss", "logvar", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss", "d_loss", "p_true", "p_fake", "gp_loss")


def rel(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def map_err(got, ref):
    ref = t(ref).double()
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def checksum_err(tensors, names, cks, absmax=None, skip=()):
    e = R.checksum_errors(tensors, names, cks, absmax, skip)
    return e["sum"][1], e["smp_max"][1]


@pytest.fixture(scope="module")
def runs(golden):
    g = golden("g22_image_gan")
    out = {}
    for size in (32, 64):
        x = t(g[f"c{size}_in_image"]).double()
        out[size] = dict(probe=R.probe(R.build(size), x))
        S = R.build(size)
        out[size]["steps"] = [R.step(S, x), R.step(S, x)]
    return out


@pytest.mark.parametrize("size", [32, 64])
def test_comparator_discriminator_terms_equal_the_golden(golden, runs, size):
    g, p = golden("g22_image_gan"), runs[size]["probe"]
    c = f"c{size}_p_"
    assert tuple(p["pred"].shape) == ((2, 1, 2, 2) if size == 32 else (2, 1, 6, 6))
    assert map_err(p["pred"], g[c + "pred"]) <= REL and map_err(p["pred_fake"], g[c + "pred_fake"]) <= REL
    assert rel(p["loss_real"], g[c + "loss_real"]) <= REL and rel(p["loss_fake"], g[c + "loss_fake"]) <= REL
    assert abs(p["gp"] - float(g[c + "gp"])) <= REL * float(g[c + "gp"]) and map_err(p["gp_per_sample"], g[c + "gp_per_sample"]) <= REL
    assert p["gp_none"] == [str(k) for k in g[c + "gp_none"]] == ["disc.model.11.bias"]
    names = [str(k) for k in g[c + "grad_names"]]
    for term in ("real", "gp", "fake"):
        e_sum, e_smp = checksum_err(p["grads"][term], names, g[c + f"{term}_grad_checksums"], g[c + f"{term}_grad_absmax"])
        print(f"g22 c{size} {term}: checksum {e_sum:.2e} sampled {e_smp:.2e}")
        assert e_sum <= REL and e_smp <= REL, (term, e_sum, e_smp)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("size", [32, 64])
def test_comparator_step_equals_the_golden(golden, runs, size, step):
    g, r = golden("g22_image_gan"), runs[size]["steps"][step - 1]
    c = f"c{size}_s{step}_"
    assert r["last_layer_shape"] == tuple(g[f"c{size}_last_layer_shape"]) == (3,)
    for k in ("rec", "pred_true", "pred_fake", "pred_gen", "gp_per_sample"):
        assert map_err(r[k], g[c + k]) <= REL, k
    for k in SCALARS:
        assert rel(r["scalars"][k], g[c + k]) <= REL, (k, r["scalars"][k], float(g[c + k]))
    assert 0.0 < r["scalars"]["d_weight"] < 1e4 and r["pre0_margin"] >= 1e-6
    skip = set()
    for tag in ("d", "g"):
        names = [str(k) for k in g[c + f"{tag}_grad_names"]]
        assert set(names) == set(r[f"{tag}_grads"])
        zero = R.zero_gradient_biases(names, g[c + f"{tag}_grad_checksums"])
        assert len(zero) == ({32: 3, 64: 5}[size] if tag == "g" else 0)
        skip |= zero
        e_sum, e_smp = checksum_err(r[f"{tag}_grads"], names, g[c + f"{tag}_grad_checksums"], g[c + f"{tag}_grad_absmax"], zero)
        print(f"g22 c{size} step {step} {tag}-gradients: checksum {e_sum:.2e} sampled {e_smp:.2e}")
        assert e_sum <= REL and e_smp <= REL, (tag, e_sum, e_smp)
    e_sum, e_smp = checksum_err(r["uv"], [str(k) for k in g[c + "uv_names"]], g[c + "uv_checksums"])
    assert e_sum <= REL and e_smp <= REL
    e_sum, e_smp = checksum_err(r["params"], [str(k) for k in g[c + "param_names"]], g[c + "param_checksums"], None, skip)
    print(f"g22 c{size} step {step} parameters: checksum {e_sum:.2e} sampled {e_smp:.2e}")
    assert e_sum <= REL and e_smp <= REL


def test_golden_conditions_for_exactness(golden):
    g = golden("g22_image_gan")
    for size in (32, 64):
        assert float(g[f"c{size}_margin_hinge"]) >= 1e-4 and float(g[f"c{size}_margin_conv0"]) >= 1e-6 and float(g[f"c{size}_margin_kink"]) >= 3e-7
        # the reference's fp32 run and six runs with parameters disturbed by 2e-7 stay this close to the stored float64 run over both steps
        assert float(g[f"c{size}_fp32_maps"]) <= 2e-5 and float(g[f"c{size}_fp32_scalars"]) <= 2e-5
        for s in (1, 2):
            assert 0.0 < float(g[f"c{size}_s{s}_d_weight"]) < 1e4
    assert sum(int(g[f"c{s}_hinge_active"]) for s in (32, 64)) > 0 and sum(int(g[f"c{s}_hinge_inactive"]) for s in (32, 64)) > 0


def test_state_dict_names_equal_the_reference(golden):
    from ipoke_amd.image_gan import ConvAEGANModel, NLayerDiscriminator
    g = golden("g22_image_gan")
    d = NLayerDiscriminator(dtype="f32")
    ref_keys = [str(k) for k in g["c64_disc_keys"]]
    assert len(ref_keys) == 21 and list(d.state_dict()) == ref_keys
    ref_shapes = [tuple(int(v) for v in str(s).split(",") if v) for s in g["c64_disc_shapes"]]
    assert [tuple(v.shape) for v in d.state_dict().values()] == ref_shapes
    assert float(d.model[11].bias.detach().abs().max()) == 0.0 and float(d.model[0].bias.detach().abs().max()) == 0.0
    assert 0.015 < float(d.model[11].weight.detach().std()) < 0.025
    for size in (32, 64):
        m = ConvAEGANModel(configs.img_encoder_train_config(size), dtype="f32")
        assert list(m.state_dict()) == [str(k) for k in g[f"c{size}_keys"]]
    # a reference checkpoint's disc.* entries load
    m.load_state_dict({k: torch.zeros_like(v) for k, v in m.state_dict().items()}, strict=True)
    assert list(m.decoder.parameters())[-1] is m.decoder.out_conv.conv.bias


def test_checkpoint_loads_into_the_second_stage():
    from ipoke_amd.image_gan import ConvAEGANModel
    from tests.test_ae2d_cpu import second_stage_model
    m = second_stage_model()
    img = ConvAEGANModel(configs.img_encoder_train_config(64), dtype="f32")
    deterministic_fill_(img)
    m.load_conditioner({"state_dict": img.state_dict()})
    got = m.conditioner.state_dict()
    enc = {k: v for k, v in img.state_dict().items() if k.startswith("encoder.")}
    assert set(got) == set(enc) and len(enc) > 40
    assert all(torch.equal(got[k], enc[k]) for k in enc)


def test_refusal_of_the_plain_model_stays_and_the_trainer_owns_two_optimisers():
    from ipoke_amd.image_gan import ConvAEGANModel, ImageEncoderGANTrainer
    conf = configs.img_encoder_train_config(32)
    m = ConvAEGANModel(conf, dtype="f32")
    m.current_epoch = conf["training"]["pretrain"]
    with pytest.raises(NotImplementedError, match="define_D.*gradient penalty.*adaptive weight"):
        m.training_loss({"images": torch.zeros(1, 2, 3, 32, 32)})
    tr = ImageEncoderGANTrainer(m, lr=2e-4)
    assert len(tr.opt_d.params) == 13 and tr.opt_d.betas == (0.9, 0.999) and tr.opt.betas == (0.9, 0.999)
    assert {id(p) for p in tr.opt_d.params} == {id(p) for p in m.disc.parameters()}
    assert not ({id(p) for p in tr.opt.params} & {id(p) for p in tr.opt_d.params})
    sd = tr.state_dict()
    assert {"model", "opt", "scheduler", "opt_d", "scheduler_d"} <= set(sd)
    tr.scheduler_d.best = 3.0
    tr2 = ImageEncoderGANTrainer(ConvAEGANModel(conf, dtype="f32"))
    tr2.load_state_dict(tr.state_dict())
    assert tr2.scheduler_d.best == 3.0 and tr2.opt_d.lr == tr.opt_d.lr


# 30 values: improvements, plateaus (equal values, values inside the threshold), a rise, a slow decay
LOSSES = [10.0, 9.0, 8.5, 8.5, 8.5, 8.4999, 8.4995, 8.0, 8.0, 8.0, 8.0, 7.9, 7.8999, 7.8998, 7.0, 7.5, 7.4, 7.3, 6.999, 6.998,
          6.997, 6.99, 6.9, 6.9, 6.9, 6.9, 6.9, 6.9, 6.9, 6.8999]


def test_two_scheduler_sequence_equals_torch():
    """Both plateau schedulers act on the generator's optimiser, factor .5 first, then factor .1; the discriminator's rate is constant."""
    from ipoke_amd.image_gan import ConvAEGANModel, ImageEncoderGANTrainer
    assert len(LOSSES) == 30
    lr = 2e-4
    p = torch.nn.Parameter(torch.zeros(1))
    opt_g, opt_d = torch.optim.Adam([p], lr=lr), torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    kw = dict(mode="min", patience=0, min_lr=1e-8, threshold=0.001, threshold_mode="rel")
    sched_g = torch.optim.lr_scheduler.ReduceLROnPlateau(opt_g, factor=.5, **kw)
    sched_d = torch.optim.lr_scheduler.ReduceLROnPlateau(opt_g, factor=.1, **kw)
    tr = ImageEncoderGANTrainer(ConvAEGANModel(configs.img_encoder_train_config(32), dtype="f32"), lr=lr)
    traj_ref, traj = [], []
    for v in LOSSES:
        sched_g.step(v)
        sched_d.step(v)
        tr.on_validation_epoch_end(v)
        traj_ref.append((opt_g.param_groups[0]["lr"], opt_d.param_groups[0]["lr"]))
        traj.append((tr.opt.lr, tr.opt_d.lr))
    assert traj == traj_ref
    assert len({a for a, _ in traj}) >= 4 and {b for _, b in traj} == {lr}


def test_kernels_reject_bad_arguments_before_any_launch():
    lib = _lib.lib()
    a = torch.zeros(256)
    d = torch.zeros(int(lib.ipoke_hinge_terms_partials()) + int(lib.ipoke_gp_direction_partials(2)), dtype=torch.float64)
    err = lambda: lib.ipoke_last_error()
    H = lambda pred, ld, M, mode, out, grad, ldg, part: lib.ipoke_hinge_terms(pred, ld, M, mode, out, grad, ldg, part, None)
    assert H(ptr(a), 1, 8, 3, ptr(a), ptr(a), 1, ptr(d)) == -1 and b"real, fake or generator" in err()
    assert H(ptr(a), 0, 8, 0, ptr(a), ptr(a), 1, ptr(d)) == -1 and b"extents" in err()
    assert H(ptr(a), 1, 0, 0, ptr(a), ptr(a), 1, ptr(d)) == -1
    assert H(ptr(a), 1, 8, 0, ptr(a), ptr(a), 1, None) == -1 and b"partials" in err()
    assert H(None, 1, 8, 0, ptr(a), ptr(a), 1, ptr(d)) == -1
    J = lambda y, ldy, ldx, ldo, M, C, Cpad, act, dt: lib.ipoke_act_jvp(y, ldy, ptr(a), ldx, ptr(a), ldo, M, C, Cpad, act, dt, None)
    assert J(ptr(a), 8, 8, 8, 4, 8, 8, _lib.ACT_ELU, _lib.F32) == -1 and b"LeakyReLU(0.2) or ReLU" in err()
    assert J(ptr(a), 4, 8, 8, 4, 8, 8, _lib.ACT_LRELU02, _lib.F32) == -1 and b"pitches" in err()
    assert J(ptr(a), 8, 8, 8, 4, 8, 16, _lib.ACT_LRELU02, _lib.F32) == -1            # the output's pitch is below its padded width
    assert J(ptr(a), 8, 8, 8, 4, 8, 4, _lib.ACT_RELU, _lib.BF16) == -1               # padded width below the channel count
    assert J(ptr(a), 8, 8, 8, 4, 8, 8, _lib.ACT_RELU, 7) == -1 and b"dtype" in err()
    assert J(None, 8, 8, 8, 4, 8, 8, _lib.ACT_RELU, _lib.F32) == -1
    G = lambda g, N, L, v, out, part: lib.ipoke_gp_direction(g, N, L, v, out, part, None)
    assert G(ptr(a), 0, 8, ptr(a), ptr(a), ptr(d)) == -1 and b"extents" in err()
    assert G(ptr(a), 2, 0, ptr(a), ptr(a), ptr(d)) == -1
    assert G(ptr(a), 2, 8, ptr(a), ptr(a), None) == -1 and b"partials" in err()
    assert G(ptr(a), 2, 8, None, ptr(a), ptr(d)) == -1
    T = lambda C, G_, act, y, ldx: lib.ipoke_groupnorm_tangent(ptr(a), ldx, ptr(a), C, y, C, ptr(a), C, ptr(a), 1, 4, C, G_, act, 1e-5, _lib.F32, None)
    assert T(48, 16, _lib.ACT_NONE, None, 48) == -1 and b"divide 256" in err()       # 3 channels per group
    assert T(32, 5, _lib.ACT_NONE, None, 32) == -1
    assert T(32, 16, _lib.ACT_LRELU02, None, 32) == -1 and b"primal output" in err()
    assert T(32, 16, _lib.ACT_TANH, ptr(a), 32) == -1
    assert T(32, 16, _lib.ACT_NONE, None, 16) == -1 and b"pitches" in err()
    B = lambda q, rows, gamma: lib.ipoke_groupnorm_tangent_bwd(ptr(a), 32, ptr(a), 32, None, 32, q, 32, ptr(a), 32, ptr(a), 32, rows, gamma, 1, 4, 32,
                                                              16, _lib.ACT_NONE, 1e-5, _lib.F32, None)
    assert B(None, None, None) == -1 and B(ptr(a), ptr(a), None) == -1 and b"needs gamma" in err()
    assert lib.ipoke_hinge_terms_partials() >= 2 and lib.ipoke_gp_direction_partials(3) >= 3 and lib.ipoke_gp_direction_partials(0) == 0


def test_new_symbols_are_exported_and_declared():
    import os
    names = ("ipoke_hinge_terms", "ipoke_hinge_terms_partials", "ipoke_act_jvp", "ipoke_gp_direction", "ipoke_gp_direction_partials",
             "ipoke_groupnorm_tangent", "ipoke_groupnorm_tangent_bwd")
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipoke_hip.h")).read()
    for n in names:
        assert hasattr(handle, n) and n in _lib.SIGNATURES and n + "(" in header
    assert (_lib.HINGE_REAL, _lib.HINGE_FAKE, _lib.HINGE_GENERATOR) == (0, 1, 2)
