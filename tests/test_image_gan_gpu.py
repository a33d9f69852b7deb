"""The image autoencoder's adversarial step on the GPU (ipoke_amd/image_gan.py) against golden ``g22_image_gan`` -- the reference's own
``ConvEncoder``, ``ConvDecoder``, ``define_D``, ``calculate_adaptive_weight`` with the step's lines restated
(scripts/make_goldens_image_gan.py) -- at 32 x 32 and 64 x 64, B = 2.

* The discriminator alone, term by term: prediction maps, hinge-real / hinge-fake values and gradients, the penalty (value, per
  sample, every parameter gradient; the head's bias gets exactly none).
* Two full steps: every entry of the returned dict (``d_weight`` among them), the prediction maps, the gradients both optimisers saw,
  the power-iteration vectors after the three iterations per step, and every parameter after each step.
* A step before ``training.pretrain`` equals ``ImageEncoderTrainer.step`` bit for bit; two runs of two steps are bit-identical; the
  shipped topology (64 x 64, the configuration's own model) runs two steps with finite outputs.

Bounds.  f32: the f32 row of ``TOL`` in tests/test_train_mode_gpu.py, mapped as tests/test_ae2d_gpu.py maps it -- x_max / x_mean: maps
(absolute; predictions and reconstructions are O(1)); loss: every scalar, relative to max(1, |ref|); sum / smp_max / smp_mean: the
gradient checksums; u: weight_u / weight_v; p_sum = sum and p_smp = smp_max: the parameters after a step.  bf16: 1.5 x the worst value
measured on the MI355X against the same golden over both sizes and both steps (the project's rule for bf16 bounds); the measured values
stand next to the bounds.  Convolution biases in front of a norm have an analytically zero gradient and are left out of the checksums
(``image_gan_ref.zero_gradient_biases``); what the GPU holds there is bounded as noise.
"""
import functools
import os

import numpy as np
import pytest
import torch

from ipoke_amd import _lib, configs
from ipoke_amd.utils.detfill import deterministic_fill_
from tests import image_gan_ref as R
from tests.conftest import GOLDEN, t
from tests.test_train_mode_gpu import TOL as TRAIN_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"

_F32 = TRAIN_TOL["f32"]
KEYS = ("x_max", "x_mean", "loss", "sum", "smp_max", "smp_mean", "u", "p_sum", "p_smp")
TOL = {"f32": dict(x_max=_F32["x_max"], x_mean=_F32["x_mean"], loss=_F32["loss"], sum=_F32["sum"], smp_max=_F32["smp_max"],
                   smp_mean=_F32["smp_mean"], u=_F32["u"], p_sum=_F32["sum"], p_smp=_F32["smp_max"]),
       # measured on the MI355X in f32 mode, worst of both sizes, the terms and both steps: x_max 7.0e-6, x_mean 6.3e-7, loss 4.0e-6 (d_weight,
       # step 2), sum 7.1e-6, smp_max 6.0e-6, smp_mean 2.0e-6, u 2.7e-7, p_sum 3.2e-8, p_smp 1.6e-7
       #
       # bf16 = 1.5 x the worst value measured on the MI355X against the same golden (size / where):
       #   x_max 4.545e-1 (64, step 2 rec), x_mean 1.584e-2 (64, step 2 rec), loss 2.092e-1 (64, step 2 d_weight), sum 1.727e-1 (64, step 2
       #   g-gradients), smp_max 5.820e-1 (64, step 2 g-gradients), smp_mean 1.654e-1 (32, step 2 g-gradients), u 1.413e-3 (32, step 2),
       #   p_sum 4.897e-4 (32, step 2), p_smp 3.907e-3 (64, step 2); the discriminator's terms alone stay below x_max 1.7e-2, loss 5.0e-3,
       #   sum 1.5e-2, smp_max 5.7e-2
       "bf16": dict(x_max=0.682, x_mean=2.38e-2, loss=0.314, sum=0.259, smp_max=0.873, smp_mean=0.248, u=2.12e-3, p_sum=7.35e-4, p_smp=5.86e-3)}
SCALARS = ("loss", "kl_loss", "logvar", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss", "d_loss", "p_true", "p_fake", "gp_loss")


def load():
    return dict(np.load(os.path.join(GOLDEN, "g22_image_gan.npz"), allow_pickle=False).items())


def make_model(size, dtype):
    from ipoke_amd.image_gan import ConvAEGANModel
    conf = configs.img_encoder_train_config(size)
    m = ConvAEGANModel(conf, dtype=dtype)
    deterministic_fill_(m)
    m.current_epoch = conf["training"]["pretrain"]
    return m.to(DEV).train()


def make_batch(x):
    return {"images": torch.stack([torch.zeros_like(x), x], dim=1)}             # the model reads images[:, -1]


def rel(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


class Worst(dict):
    """The worst figure per tolerance key, with where it occurred."""

    def add(self, key, value, where):
        if value >= self.get(key, (-1.0, ""))[0]:
            self[key] = (float(value), where)

    def maps(self, got, ref, where):
        d = (got.detach().double().cpu() - t(ref).double()).abs()
        self.add("x_max", d.max().item(), where)
        self.add("x_mean", d.mean().item(), where)

    def grads(self, tensors, names, cks, absmax, skip, where, keys=("sum", "smp_max", "smp_mean")):
        e = R.checksum_errors(tensors, names, cks, absmax, skip)
        self.add(keys[0], e["sum"][1], f"{where} {e['sum'][0]}")
        self.add(keys[1], e["smp_max"][1], f"{where} {e['smp_max'][0]}")
        if len(keys) > 2:
            self.add(keys[2], e["smp_mean"], where)


def grads_of(named):
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in named}


@functools.lru_cache(maxsize=None)
def measure_terms(size, dtype):
    """The discriminator alone, term by term, measured once."""
    g = load()
    c = f"c{size}_p_"
    x = t(g[f"c{size}_in_image"], DEV)
    disc = make_model(size, dtype).disc
    named = [("disc." + k, p) for k, p in disc.named_parameters()]
    names = [str(k) for k in g[c + "grad_names"]]
    assert names == [k for k, _ in named]
    w, f = Worst(), {}
    pred = disc(x)                                                              # power iteration 1
    assert tuple(pred.shape) == tuple(g[c + "pred"].shape) and pred.dtype == torch.float32
    w.maps(pred, g[c + "pred"], "pred")
    loss_real, _ = disc.hinge(pred, _lib.HINGE_REAL)
    loss_real.backward()
    w.add("loss", rel(loss_real.item(), g[c + "loss_real"]), "hinge-real")
    w.grads(grads_of(named), names, g[c + "real_grad_checksums"], g[c + "real_grad_absmax"], (), "hinge-real")
    disc.zero_grad(set_to_none=True)
    gp = disc.gp(x)                                                             # on the buffers iteration 1 left
    gp.backward()
    f["gp_none"] = [k for k, p in named if p.grad is None]
    w.add("loss", rel(gp.item(), g[c + "gp"]), "penalty")
    w.add("loss", max(rel(a, b) for a, b in zip(disc.last_gp_per_sample.tolist(), g[c + "gp_per_sample"])), "penalty per sample")
    w.grads(grads_of(named), names, g[c + "gp_grad_checksums"], g[c + "gp_grad_absmax"], (), "penalty")
    disc.zero_grad(set_to_none=True)
    pred_f = disc(0.5 * x.flip(0))                                              # iteration 2
    w.maps(pred_f, g[c + "pred_fake"], "pred_fake")
    loss_fake, _ = disc.hinge(pred_f, _lib.HINGE_FAKE)
    loss_fake.backward()
    w.add("loss", rel(loss_fake.item(), g[c + "loss_fake"]), "hinge-fake")
    w.grads(grads_of(named), names, g[c + "fake_grad_checksums"], g[c + "fake_grad_absmax"], (), "hinge-fake")
    torch.cuda.synchronize()
    return w, f


@functools.lru_cache(maxsize=None)
def measure_steps(size, dtype):
    """Two trainer steps from the golden's start, measured once."""
    from ipoke_amd.image_gan import ImageEncoderGANTrainer
    g = load()
    x = t(g[f"c{size}_in_image"], DEV)
    m = make_model(size, dtype)
    tr = ImageEncoderGANTrainer(m, lr=2e-4, weight_decay=0.0)
    named_g = [(k, p) for k, p in m.named_parameters() if not k.startswith("disc.")]
    named_d = [(k, p) for k, p in m.named_parameters() if k.startswith("disc.")]
    w, f = Worst(), {"noise": 0.0, "moved": 0.0, "finite": True}
    start = {k: p.detach().clone() for k, p in named_g}
    skip = set()
    for step in (1, 2):
        c = f"c{size}_s{step}_"
        out = tr.step(make_batch(x))
        torch.cuda.synchronize()
        assert set(out) == {"train/" + k for k in SCALARS}
        assert all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 for v in out.values()), "every entry is a device scalar"
        for k in SCALARS:
            w.add("loss", rel(out["train/" + k].item(), g[c + k]), f"step {step} {k}")
        w.maps(tr.last_rec, g[c + "rec"], f"step {step} rec")
        for tag, named in (("d", named_d), ("g", named_g)):
            names = [str(k) for k in g[c + f"{tag}_grad_names"]]
            cks = g[c + f"{tag}_grad_checksums"]
            assert set(names) == {k for k, _ in named} == {k for k, p in named if p.grad is not None}, "every parameter receives a gradient"
            zero = R.zero_gradient_biases(names, cks)
            skip |= zero
            grads = grads_of(named)
            w.grads(grads, names, cks, g[c + f"{tag}_grad_absmax"], zero, f"step {step} {tag}-gradients")
            for k in zero:
                wk = k[:-len(".bias")] + (".weight_orig" if k[:-len(".bias")] + ".weight_orig" in names else ".weight")
                f["noise"] = max(f["noise"], grads[k].abs().sum().item() / cks[names.index(wk)][1])
        sd = m.state_dict()
        e = R.checksum_errors(sd, [str(k) for k in g[c + "uv_names"]], g[c + "uv_checksums"])
        # u and v are unit vectors: the sampled entries are absolute already; the sums relative to the abs-sum
        w.add("u", max(e["sum"][1], e["smp_max"][1]), f"step {step} {e['smp_max'][0]}")
        w.grads(dict(named_g + named_d), [str(k) for k in g[c + "param_names"]], g[c + "param_checksums"], None, skip,
                f"step {step} parameters", keys=("p_sum", "p_smp"))
        f["finite"] = f["finite"] and all(bool(torch.isfinite(v).all()) for v in sd.values())
    f["n_zero"] = len(skip)
    f["moved"] = max((p.detach() - start[k]).abs().max().item() / 2e-4 for k, p in named_g if k in skip)
    return w, f


def report(what, size, dtype, w):
    print(f"image_gan[{what} {size}/{dtype}] " + "; ".join(f"{k} {w[k][0]:.3e} ({w[k][1]})" for k in KEYS if k in w))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("size", [32, 64])
def test_discriminator_terms_against_the_reference(size, dtype):
    w, f = measure_terms(size, dtype)
    report("terms", size, dtype, w)
    assert f["gp_none"] == ["disc.model.11.bias"], "the head's bias takes no part in the penalty: exactly no gradient"
    tol = TOL[dtype]
    assert all(w[k][0] <= tol[k] for k in w), {k: w[k] for k in w if w[k][0] > tol[k]}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("size", [32, 64])
def test_two_steps_against_the_reference(size, dtype):
    w, f = measure_steps(size, dtype)
    report("steps", size, dtype, w)
    print(f"image_gan[steps {size}/{dtype}] {f['n_zero']} norm-fed biases: gradient noise {f['noise']:.2e} of the weight's, moved {f['moved']:.2f} lr")
    assert f["finite"] and f["n_zero"] == {32: 3, 64: 5}[size]
    assert f["noise"] <= 1e-3
    # Adam's first two updates are at most lr and 1.0013 lr whatever the gradients (Cauchy-Schwarz on m_hat / sqrt(v_hat), betas 0.9, 0.999)
    assert f["moved"] <= 2.01
    tol = TOL[dtype]
    assert all(w[k][0] <= tol[k] for k in w), {k: w[k] for k in w if w[k][0] > tol[k]}


# ------------------------------------------------------------------------------------------------ the two phases, reproducibility
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_step_before_pretrain_equals_the_reconstruction_trainer(dtype):
    from ipoke_amd.autoencoder2d import ConvAEModel, ImageEncoderTrainer
    from ipoke_amd.image_gan import ImageEncoderGANTrainer
    x = t(load()["c32_in_image"], DEV)
    conf = configs.img_encoder_train_config(32)
    plain = ConvAEModel(conf, dtype=dtype)
    deterministic_fill_(plain)
    plain = plain.to(DEV)
    gan = make_model(32, dtype)
    gan.current_epoch = conf["training"]["pretrain"] - 1
    disc0 = {k: v.detach().clone() for k, v in gan.disc.state_dict().items()}
    a, b = ImageEncoderTrainer(plain), ImageEncoderGANTrainer(gan)
    for _ in range(2):
        da, db = a.step(make_batch(x)), b.step(make_batch(x))
        assert set(da) == set(db) and all(torch.equal(da[k], db[k]) for k in da)
    sa, sb = plain.state_dict(), gan.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(torch.equal(v, disc0[k]) for k, v in gan.disc.state_dict().items()), "the discriminator is untouched before pretrain"
    assert all(p.grad is None for p in gan.disc.parameters()) and b.opt_d.steps == 0


def two_steps(size, dtype, batch):
    from ipoke_amd.image_gan import ImageEncoderGANTrainer
    m = make_model(size, dtype)
    tr = ImageEncoderGANTrainer(m)
    outs = [{k: v.detach().cpu().clone() for k, v in tr.step(batch).items()} for _ in range(2)]
    torch.cuda.synchronize()
    return outs, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, tr


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_runs_of_two_steps_are_bit_identical(dtype):
    batch = make_batch(t(load()["c64_in_image"], DEV))
    (o1, s1, _), (o2, s2, _) = two_steps(64, dtype, batch), two_steps(64, dtype, batch)
    for a, b in zip(o1, o2):
        diff = [k for k in a if not torch.equal(a[k], b[k])]
        assert not diff, f"dict entries differ between two runs from the same state: {diff}"
    diff = [k for k in s1 if not torch.equal(s1[k], s2[k])]
    assert not diff, f"{len(diff)} tensors differ between two runs from the same state, e.g. {diff[:3]}"


def test_shipped_topology_runs_two_steps():
    """img_encoder.yaml's own model (64 x 64, three stages, bf16) on a batch of 8: finite outputs, both optimisers stepped, the trainer's
    state round-trips."""
    from ipoke_amd.image_gan import ImageEncoderGANTrainer
    x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(5)) * 2 - 1
    outs, sd, tr = two_steps(64, "bf16", make_batch(x.to(DEV)))
    assert len(tr.model.decoder.blocks) == 3
    assert all(bool(torch.isfinite(v)) for o in outs for v in o.values()) and all(bool(torch.isfinite(v).all()) for v in sd.values())
    assert tr.opt.steps == 2 and tr.opt_d.steps == 2
    assert all(0.0 < o["train/d_weight"].item() <= 1e4 and o["train/gp_loss"].item() > 0 for o in outs)
    val = tr.validation_step(make_batch(x.to(DEV)))
    assert set(val) == {"val/loss", "val/nll_loss", "val/logvar", "val/rec_loss"} and bool(torch.isfinite(val["val/loss"]))
    tr2 = ImageEncoderGANTrainer(make_model(64, "bf16"))
    tr2.load_state_dict(tr.state_dict())
    assert tr2.opt_d.steps == 2 and all(torch.equal(a, b) for a, b in zip(tr2.opt_d.exp_avg, tr.opt_d.exp_avg))
