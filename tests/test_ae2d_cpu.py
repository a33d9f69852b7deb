"""The 2-D poke / image autoencoders (ipoke_amd/autoencoder2d.py), host side: state-dict compatibility with the reference and with the
second stage's loaders, the plateau scheduler against torch's, the golden's loss values against their float64 formula, and the two
refusals.  Golden ``g19_ae2d`` is the reference's own ``FirstStageWrapper`` in train mode (scripts/make_goldens_ae2d.py)."""
import numpy as np
import pytest
import torch

from ipoke_amd import configs
from ipoke_amd.autoencoder2d import ConvAEModel, ConvPokeAE, ReduceLROnPlateau
from ipoke_amd.utils.detfill import deterministic_fill_

CASES = {"a": lambda: ConvPokeAE(configs.poke_encoder_train_config(32), dtype="f32"),
         "b": lambda: ConvPokeAE(configs.poke_encoder_train_config(64, flow_ae=False, poke_and_image=True), dtype="f32"),
         "c": lambda: ConvAEModel(configs.img_encoder_train_config(64), dtype="f32")}


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_state_dict_keys_and_shapes_equal_the_reference(golden, tag):
    g = golden("g19_ae2d")
    sd = CASES[tag]().state_dict()
    ref_keys = [str(k) for k in g[f"{tag}_keys"]]
    assert list(sd) == ref_keys
    ref_shapes = [tuple(int(v) for v in str(s).split(",") if v) for s in g[f"{tag}_shapes"]]
    assert [tuple(v.shape) for v in sd.values()] == ref_shapes
    n_net = sum(v.numel() for k, v in sd.items() if "." in k and k.endswith(("weight", "bias", "weight_orig")))
    assert n_net == {"a": 380994, "b": 603938, "c": 603651}[tag]


def second_stage_model():
    from ipoke_amd.second_stage import PokeMotionModel
    arch = configs.flow_arch(32, hidden=64, num_steps=[2, 1, 1], factor=4)
    arch["flow_mid_channels_factor"] = 2
    return PokeMotionModel(configs.second_stage_config(64, 32, 16, batch_size=2, arch=arch), dirs={}, dtype="f32", device="cpu", max_batch=2)


def test_checkpoints_load_into_the_second_stage():
    """A checkpoint written from either autoencoder goes through the second stage's own loaders unchanged; the encoder arrives bit-equal."""
    m = second_stage_model()
    poke = ConvPokeAE(configs.poke_encoder_train_config(64), dtype="f32")
    deterministic_fill_(poke)
    m.load_poke_embedder({"state_dict": poke.state_dict()})
    got = m.poke_embedder.state_dict()
    enc = {k[len("model."):]: v for k, v in poke.state_dict().items() if k.startswith("model.encoder.")}
    assert set(got) == set(enc) and len(enc) > 40
    assert all(torch.equal(got[k], enc[k]) for k in enc)
    img = ConvAEModel(configs.img_encoder_train_config(64), dtype="f32")
    deterministic_fill_(img)
    m.load_conditioner({"state_dict": img.state_dict()})
    got = m.conditioner.state_dict()
    enc = {k: v for k, v in img.state_dict().items() if k.startswith("encoder.")}
    assert set(got) == set(enc) and len(enc) > 40
    assert all(torch.equal(got[k], enc[k]) for k in enc)


class _Lr:
    def __init__(self, lr):
        self.lr = lr


# 30 values: improvements, plateaus (equal values, values inside the thresholds), a rise, a slow decay
LOSSES = [10.0, 9.0, 8.5, 8.5, 8.5, 8.4999, 8.4995, 8.0, 8.0, 8.0, 8.0, 7.9, 7.8999, 7.8998, 7.0, 7.5, 7.4, 7.3, 6.999, 6.998,
          6.997, 6.99, 6.9, 6.9, 6.9, 6.9, 6.9, 6.9, 6.9, 6.8999]


@pytest.mark.parametrize("lr,kw", [(1e-3, dict(factor=.5, patience=1, min_lr=1e-8, threshold=1e-4, threshold_mode="abs")),    # conv_poke_encoder.py:179
                                   (2e-4, dict(factor=.5, patience=0, min_lr=1e-8, threshold=1e-3, threshold_mode="rel")),    # first_stage_image_conv.py:287
                                   (1e-6, dict(factor=.1, patience=2, min_lr=3e-8, threshold=1e-4, threshold_mode="rel", eps=1e-8, cooldown=1))])
def test_plateau_scheduler_equals_torch(lr, kw):
    assert len(LOSSES) == 30
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", **kw)
    host = _Lr(lr)
    mine = ReduceLROnPlateau(host, mode="min", **kw)
    traj_ref, traj = [], []
    for v in LOSSES:
        ref.step(v)
        mine.step(v)
        traj_ref.append(opt.param_groups[0]["lr"])
        traj.append(host.lr)
    assert traj == traj_ref
    assert len(set(traj)) >= 3                       # the sequence does exercise reductions
    again = ReduceLROnPlateau(_Lr(lr), mode="min", **kw)
    again.load_state_dict(mine.state_dict())
    assert again.state_dict() == mine.state_dict()


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_golden_loss_values_follow_the_formula(golden, tag):
    """nll and d nll / d logvar of the golden from its stored x, rec and logvar in float64 (the formula ipoke_l1_nll implements)."""
    g = golden("g19_ae2d")
    x = torch.from_numpy(g[f"{tag}_in_image"] if tag == "c" else g[f"{tag}_in_flow"]).double()
    rec = torch.from_numpy(g[f"{tag}_rec"]).double()
    lv, w = float(g[f"{tag}_logvar"]), float(g[f"{tag}_perc_weight"])
    N, C, H, W = x.shape
    a = (x - rec).abs().sum().item()
    p_sum = ((x - rec) ** 2).mean(dim=(1, 2, 3)).sum().item() if tag == "d" else 0.0
    data = (a + C * H * W * w * p_sum) * np.exp(-lv) / N
    assert abs(a - float(g[f"{tag}_abs_sum"])) <= 1e-9 * a
    # the golden's values are fp32 results of a sum over N * C * H * W terms
    assert abs(data + C * H * W * lv - float(g[f"{tag}_nll"])) <= 2e-6 * abs(float(g[f"{tag}_nll"]))
    assert abs(C * H * W - data - float(g[f"{tag}_dlogvar"])) <= 2e-6 * (C * H * W + data)


def test_refusals_name_their_reasons():
    conf = configs.img_encoder_train_config(64)
    m = ConvAEModel(conf, dtype="f32")
    m.current_epoch = conf["training"]["pretrain"]
    with pytest.raises(NotImplementedError, match="define_D.*gradient penalty.*adaptive weight"):
        m.training_loss({"images": torch.zeros(1, 2, 3, 64, 64)})
    for make, cf in ((ConvAEModel, configs.img_encoder_train_config(64)), (ConvPokeAE, configs.poke_encoder_train_config(64))):
        cf["architecture"]["deterministic"] = False
        with pytest.raises(NotImplementedError, match="deterministic"):
            make(cf, dtype="f32")


def test_l1_nll_rejects_bad_arguments_before_any_launch():
    """Negative status + message for arguments the kernel cannot take (checked on the host: no GPU needed)."""
    from ipoke_amd import _lib
    from ipoke_amd._lib import ptr
    lib = _lib.lib()
    a = torch.zeros(64)
    d = torch.zeros(int(lib.ipoke_l1_nll_partials()), dtype=torch.float64)
    call = lambda ld, act, p, w, part: lib.ipoke_l1_nll(ptr(a), ld, act, ptr(a), 1, 2, 4, 8, ptr(a), p, w, ptr(a), ptr(a), 2, None, 0, None, part, None)
    assert call(2, _lib.ACT_ELU, None, None, ptr(d)) == -1 and b"none or tanh" in lib.ipoke_last_error()
    assert call(1, _lib.ACT_NONE, None, None, ptr(d)) == -1                       # pitch below the channel count
    assert call(2, _lib.ACT_NONE, ptr(a), None, ptr(d)) == -1 and b"come together" in lib.ipoke_last_error()
    assert call(2, _lib.ACT_NONE, None, None, None) == -1 and b"partials" in lib.ipoke_last_error()
    assert lib.ipoke_l1_nll_partials() >= 256
