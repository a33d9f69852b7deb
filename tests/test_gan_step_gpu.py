"""The assembled first-stage adversarial training step (ipoke_amd/first_stage_gan.py, reference
first_stage_motion_model.py:160-277, with and without the VGG term) against the same step composed from the oracle's modules on
the CPU (oracle/vae_ref.py, oracle/disc_ref.py, oracle/vgg_ref.py -- each pinned to the reference by its own golden): loss values and the gradients
every optimiser sees, with frozen spectral-norm buffers and given random choices."""
import copy
import zlib

import numpy as np
import pytest
import torch

from ipoke_amd import configs
from ipoke_amd.discriminator import PatchDiscriminator, TemporalDiscriminator
from ipoke_amd.first_stage import SpadeCondMotionModel
from ipoke_amd.first_stage_gan import FirstStageGANTrainer
from ipoke_amd.autograd_ops import MultiTensorAdam
from ipoke_amd.utils.detfill import deterministic_fill_
from oracle import disc_ref, vae_ref, vgg_ref

pytestmark = pytest.mark.gpu
DT_CFG = {"bce_loss": False, "gp_weight": 1.0, "num_classes": 1, "patch_temp_disc": False, "fmap_weight": 1.0, "gen_weight": 1.0,
          "max_frames": 4}
DS_CFG = {"bce_loss": False, "gp_weight": 0.0, "fmap_weight": 1.0, "gen_weight": 1.0, "n_examples": 6}
# lr = 0: the first Adam step moves every element by +-lr according to the SIGN of its gradient, so elements whose gradient is
# round-off noise end up 2 lr apart between any two fp32 implementations and the generator-side losses (evaluated with the
# updated discriminators) drift by percents.  The update rule itself is tested against torch.optim.Adam in
# tests/test_vae_train_gpu.py; here every loss and gradient of the step is compared at identical parameters.
TRAIN = {"lr": 0.0, "weight_decay": 1e-5, "w_l1": 10.0, "w_kl": 1e-7, "w_vgg": 0.0}


def _abs_sum(d):
    return {k: v.detach().double().abs().sum().item() for k, v in d.items()}


@pytest.mark.parametrize("w_vgg", [0.0, 10.0])
def test_gan_step_matches_oracle_composition(monkeypatch, w_vgg):
    from ipoke_amd.vgg import VGGLoss
    TRAIN = dict(globals()["TRAIN"], w_vgg=w_vgg)
    size, z, T_ = 64, 32, 5
    cfg = configs.first_stage_config(size, z, T_)
    gen = torch.Generator().manual_seed(11)
    X = torch.rand(2, T_, 3, size, size, generator=gen) * 2 - 1
    eps = torch.randn(2, z, 8, 8, generator=gen)
    offset, true_ids, fake_ids = 0, np.array([0, 3, 4, 7, 8, 9]), np.array([1, 2, 5, 6, 7, 0])

    # ---- oracle composition (CPU, fp32)
    og = vae_ref.SpadeCondMotionModel(copy.deepcopy(cfg)).eval(); deterministic_fill_(og, prefix="first_stage.")
    ot = disc_ref.TemporalDiscriminator(size, DT_CFG).eval(); deterministic_fill_(ot, prefix="disc_t.")
    os_ = disc_ref.PatchDiscriminator(DS_CFG).eval(); deterministic_fill_(os_, prefix="disc_s.")
    kw = dict(lr=TRAIN["lr"], betas=(0.5, 0.9), weight_decay=TRAIN["weight_decay"])
    opt_t, opt_s = torch.optim.Adam(ot.parameters(), **kw), torch.optim.Adam(os_.parameters(), **kw)
    Xh, mu, lv = og(X, eps=eps)
    mf = DT_CFG["max_frames"]
    X_fake = torch.cat([X[:, 0].unsqueeze(1), Xh], 1)[:, offset:offset + mf].permute(0, 2, 1, 3, 4)
    X_true = X[:, offset:offset + mf].permute(0, 2, 1, 3, 4).clone().requires_grad_(True)
    pf, _ = ot(X_fake.detach()); pt, _ = ot(X_true)
    loss_dt = (ot.loss(pf, False) + ot.loss(pt, True)) / 2
    gp = ot.gp2(pt, X_true)
    (loss_dt + DT_CFG["gp_weight"] * gp).backward()
    ref = dict(loss_d_dt=loss_dt.item(), gp=gp.item(), g_dt=_abs_sum({k: p.grad for k, p in ot.named_parameters()}))
    opt_t.step()
    x_true = X.reshape(-1, 3, size, size)[true_ids]; x_fake = Xh.reshape(-1, 3, size, size)[fake_ids]
    pf, _ = os_(x_fake.detach()); pt, _ = os_(x_true)
    loss_ds = (os_.loss(pf, False) + os_.loss(pt, True)) / 2
    opt_s.zero_grad(); loss_ds.backward()
    ref.update(loss_d_ds=loss_ds.item(), g_ds=_abs_sum({k: p.grad for k, p in os_.named_parameters()}))
    opt_s.step()
    pg, _ = os_(x_fake); l_gs = -pg.mean()
    pg, ff = ot(X_fake); _, ft = ot(X_true.detach()); l_gt = -pg.mean(); l_fm = ot.fmap_loss(ff, ft)
    l_rec = vae_ref.first_stage_loss(X, Xh, mu, lv, TRAIN["w_l1"], TRAIN["w_kl"])
    ovgg = vgg_ref.VGGLoss()
    deterministic_fill_(ovgg.vgg, prefix="vgg19.")
    l_vgg = ovgg(X[:, 1:].reshape(-1, 3, size, size), Xh.reshape(-1, 3, size, size)) if w_vgg else torch.zeros(())
    og.zero_grad()
    (l_rec + w_vgg * l_vgg + l_gs + DT_CFG["gen_weight"] * l_gt + DT_CFG["fmap_weight"] * l_fm).backward()
    ref.update(loss_g_s=l_gs.item(), loss_g_t=l_gt.item(), loss_fmap_t=l_fm.item(), loss=l_rec.item(),
               g_gen=_abs_sum({k: p.grad for k, p in og.named_parameters() if p.grad is not None}))

    # ---- the HIP step
    m = SpadeCondMotionModel(copy.deepcopy(cfg), dirs={}, dtype="f32"); deterministic_fill_(m, prefix="first_stage."); m = m.cuda()
    dt_ = TemporalDiscriminator(size, DT_CFG, dtype="f32"); deterministic_fill_(dt_, prefix="disc_t."); dt_ = dt_.cuda()
    ds_ = PatchDiscriminator(DS_CFG, dtype="f32"); deterministic_fill_(ds_, prefix="disc_s."); ds_ = ds_.cuda()
    vgg = VGGLoss(dtype="f32")
    deterministic_fill_(vgg.vgg, prefix="vgg19.")
    tr = FirstStageGANTrainer(m, dt_, ds_, {"training": TRAIN, "d_t": DT_CFG, "d_s": DS_CFG, "data": {"max_frames": T_ - 1}},
                              vgg_loss=vgg.cuda() if w_vgg else None)
    seen = {}
    names = {id(tr.opt_dt): ("g_dt", dt_), id(tr.opt_ds): ("g_ds", ds_), id(tr.opt_g): ("g_gen", m)}
    orig = MultiTensorAdam.step

    def spy(self):
        tag, mod = names[id(self)]
        seen[tag] = _abs_sum({k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
        return orig(self)
    monkeypatch.setattr(MultiTensorAdam, "step", spy)
    log = tr.step(X.cuda(), eps.cuda(), offset, true_ids, fake_ids, power_iteration=False)
    torch.cuda.synchronize()
    for k in ("loss_d_dt", "loss_d_ds", "loss_g_s", "loss_g_t", "loss_fmap_t", "loss"):
        got, want = log[k].item(), ref[k]
        print(f"{k}: {got:.6f} vs {want:.6f}")
        assert abs(got - want) <= 2e-4 * max(1.0, abs(want)), k
    assert abs(log["loss_gp_dt"].item() - ref["gp"]) <= 1e-3 * ref["gp"]
    if w_vgg:
        print(f"loss_vgg: {log['loss_vgg'].item():.6f} vs {l_vgg.item():.6f}")
        assert abs(log["loss_vgg"].item() - l_vgg.item()) <= 2e-4 * max(1.0, abs(l_vgg.item()))
    for tag in ("g_dt", "g_ds", "g_gen"):
        worst = ("", 0.0)
        big = max(ref[tag].values())
        for k, want in ref[tag].items():
            got = seen[tag][k]
            if want < 1e-6 * big:                      # analytically zero gradients (bias in front of a normalisation)
                assert got <= 1e-4 * big, (tag, k, got, want)
                continue
            rel = abs(got - want) / want
            if rel > worst[1]:
                worst = (k, rel)
            # generator: the L1 sub-gradient sign(x_hat - x) flips where the residual is below the forward error (1e-3 level)
            assert rel <= (2e-2 if tag == "g_gen" else 5e-3), (tag, k, got, want)
        print(f"{tag}: worst gradient abs-sum deviation {worst[1]:.2e} ({worst[0]}) over {len(ref[tag])} tensors")
