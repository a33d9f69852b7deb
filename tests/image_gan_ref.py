"""CPU comparator of the image autoencoder's adversarial step (ipoke_amd/image_gan.py) in plain torch, any float dtype: the PatchGAN with
GroupNorm, its hinge terms and gradient penalty (by torch's double backward), the adaptive weight and one body of the training step,
plus the float64 formulas of the three kernels of csrc/image_gan.hip.  The autoencoder halves are the blocks of oracle/vae_ref.py.
tests/test_image_gan_cpu.py pins it to golden ``g22_image_gan`` (scripts/make_goldens_image_gan.py: the reference's own modules in float64).
"""
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ipoke_amd import configs
from ipoke_amd.utils.detfill import fill_value
from oracle import vae_ref as V

LOSS_STATE = ("logvar", "disc_factor", "disc_weight", "perc_weight")


def checksum(x, key):
    """sum, abs-sum and three name-keyed sampled elements (the golden's checksum)."""
    x = x.detach().double().flatten().cpu()
    idx = torch.randint(0, x.numel(), (3,), generator=torch.Generator().manual_seed(zlib.crc32(key.encode())))
    return np.array([x.sum().item(), x.abs().sum().item(), *x[idx].tolist()])


def zero_gradient_biases(names, cks):
    """Biases of convolutions directly in front of an InstanceNorm (the residual branches): their gradient is analytically zero, and
    what a run holds there is cancellation noise (1e-16 of the weight's gradient in the float64 golden).  Adam moves them by about lr
    per step on that noise."""
    out = set()
    for k, ck in zip(names, cks):
        if not k.endswith(".bias"):
            continue
        for leaf in (".weight_orig", ".weight"):
            w = k[:-len(".bias")] + leaf
            if w in names and 0.0 < ck[1] <= 1e-9 * cks[names.index(w)][1]:
                out.add(k)
    return out


def checksum_errors(tensors, names, cks, absmax=None, skip=()):
    """The gradient metrics of tests/test_train_mode_gpu.py: the worst error of a tensor's sum and abs-sum relative to the reference's
    abs-sum; the error of its sampled entries relative to its largest entry, worst and mean over the tensors."""
    worst_sum, worst_smp, smp = ("", 0.0), ("", 0.0), []
    for i, (k, ck) in enumerate(zip(names, cks)):
        if k in skip:
            continue
        cs = checksum(tensors[k], k)
        amax = tensors[k].detach().abs().max().item() if absmax is None else float(absmax[i])
        if ck[1] == 0.0:                                       # exactly no gradient in the reference: the abs-sum itself is the error
            e_sum = e_smp = cs[1]
        else:
            e_sum = max(abs(cs[0] - ck[0]), abs(cs[1] - ck[1])) / ck[1]
            e_smp = float(np.abs(cs[2:] - ck[2:]).max()) / max(amax, 1e-300)
        smp.append(e_smp)
        if e_sum >= worst_sum[1]:
            worst_sum = (k, e_sum)
        if e_smp >= worst_smp[1]:
            worst_smp = (k, e_smp)
    return dict(sum=worst_sum, smp_max=worst_smp, smp_mean=float(np.mean(smp)))


# ------------------------------------------------------------------------------------------------ networks
class _SN(nn.Module):
    """A spectral-normalised 4 x 4 convolution: weight_orig / sigma with sigma = u^T W v; in train mode u and v first move by one power
    iteration (without gradient) and the call works on copies of them."""

    def __init__(self, cin, cout, stride, bias):
        super().__init__()
        self.stride = stride
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None
        self.weight_orig = nn.Parameter(torch.zeros(cout, cin, 4, 4))
        self.register_buffer("weight_u", torch.zeros(cout))
        self.register_buffer("weight_v", torch.zeros(cin * 16))

    def forward(self, x):
        m = self.weight_orig.reshape(self.weight_orig.shape[0], -1)
        u, v = self.weight_u, self.weight_v
        if self.training:
            with torch.no_grad():
                v.copy_(F.normalize(torch.mv(m.t(), u), dim=0, eps=1e-12))
                u.copy_(F.normalize(torch.mv(m, v), dim=0, eps=1e-12))
            u, v = u.clone(), v.clone()
        return F.conv2d(x, self.weight_orig / torch.dot(u, torch.mv(m, v)), self.bias, stride=self.stride, padding=1)


class Disc(nn.Module):
    """Three-layer PatchGAN with GroupNorm(16): entries 0 | 2, 3 | 5, 6 | 8, 9 | 11 of ``model`` hold parameters, LeakyReLU(0.2) follows
    entry 0 and every GroupNorm."""

    def __init__(self, ndf=64):
        super().__init__()
        self.model = nn.ModuleDict({"0": _SN(3, ndf, 2, True),
                                    "2": _SN(ndf, 2 * ndf, 2, False), "3": nn.GroupNorm(16, 2 * ndf),
                                    "5": _SN(2 * ndf, 4 * ndf, 2, False), "6": nn.GroupNorm(16, 4 * ndf),
                                    "8": _SN(4 * ndf, 8 * ndf, 1, False), "9": nn.GroupNorm(16, 8 * ndf),
                                    "11": nn.Conv2d(8 * ndf, 1, 4, 1, 1)})

    def forward(self, x):
        m = self.model
        self.pre0 = m["0"](x)
        h = F.leaky_relu(self.pre0, 0.2)
        for c, n in (("2", "3"), ("5", "6"), ("8", "9")):
            h = F.leaky_relu(m[n](m[c](h)), 0.2)
        return m["11"](h)


def hinge(pred, real):
    return F.relu(1.0 - pred).mean() if real else F.relu(1.0 + pred).mean()


def penalty_per_sample(pred, x):
    """sum over a sample of (d sum(pred) / dx)^2, differentiable in the parameters (double backward)."""
    (g,) = torch.autograd.grad(pred.sum(), x, create_graph=True)
    return g.pow(2).reshape(x.shape[0], -1).sum(1)


class Decoder(nn.Module):
    def __init__(self, nf_in, channels):
        super().__init__()
        self.in_block = V.ResBlock(nf_in, channels[0], snorm=True, norm="group")
        self.blocks = nn.ModuleList(V.ResBlock(channels[i], nf, norm="group", upsampling=True, snorm=True) for i, nf in enumerate(channels[1:]))
        self.out_conv = V.Conv2dBlock(channels[-1], 3, 3, 1, 1, norm="none", activation="tanh")

    def forward(self, z):
        x = self.in_block(z)
        for b in self.blocks:
            x = b(x)
        return self.out_conv(x)


class State:
    pass


def build(size, dtype=torch.float64):
    """Encoder, decoder, discriminator and loss state under the package's state-dict names, filled by name; the two Adam optimisers."""
    conf = configs.img_encoder_train_config(size)
    arch, tr = conf["architecture"], conf["training"]
    n_stages = int(np.log2(size // arch["min_spatial_size"]))
    depths, nf = [32], 32
    for _ in range(n_stages - 1):
        nf = min(2 * nf, arch["nf_max"])
        depths.insert(0, nf)
    S = State()
    S.encoder = V.ConvEncoder(3, arch["nf_max"], n_stages)
    S.decoder = Decoder(arch["nf_max"], [arch["nf_max"]] + depths)
    S.disc = Disc()
    for prefix, net in (("encoder.", S.encoder), ("decoder.", S.decoder), ("disc.", S.disc)):
        net.train()
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(fill_value(prefix + k, v))
        net.to(dtype)
    for k in LOSS_STATE:
        setattr(S, k, fill_value(k, torch.zeros(())).to(dtype))
    S.logvar = nn.Parameter(S.logvar)
    S.gp_weight = tr["gp_weight"]
    S.named_g = [("encoder." + k, p) for k, p in S.encoder.named_parameters()] + [("logvar", S.logvar)] + \
                [("decoder." + k, p) for k, p in S.decoder.named_parameters()]
    S.named_d = [("disc." + k, p) for k, p in S.disc.named_parameters()]
    S.opt_g = torch.optim.Adam([p for _, p in S.named_g], lr=tr["lr"], weight_decay=tr["weight_decay"])
    S.opt_d = torch.optim.Adam([p for _, p in S.named_d], lr=tr["lr"], weight_decay=tr["weight_decay"])
    return S


def _grads(named):
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in named}


def step(S, x):
    """One body of the adversarial training step on the batch ``x``; returns everything the golden records of it."""
    r = {}
    rec = S.decoder(S.encoder(x)[0])
    nll = ((x - rec).abs() / torch.exp(S.logvar) + S.logvar).sum() / x.shape[0]
    r["rec_loss"] = (x - rec).abs().mean().item()
    # discriminator: hinge-real and the penalty on one graph (power iteration 1), hinge-fake (iteration 2), Adam
    S.opt_d.zero_grad()
    xt = x.detach().clone().requires_grad_()
    pred_true = S.disc(xt)
    r["pre0_margin"] = S.disc.pre0.detach().abs().min().item()
    loss_real = hinge(pred_true, True)
    loss_real.backward(retain_graph=True)
    reg = penalty_per_sample(pred_true, xt)
    (S.gp_weight * reg.mean()).backward()
    pred_fake = S.disc(rec.detach())
    loss_fake = hinge(pred_fake, False)
    loss_fake.backward()
    r["d_grads"] = _grads(S.named_d)
    S.opt_d.step()
    # generator: the term on the updated discriminator (iteration 3), the adaptive weight, Adam
    pred_gen = S.disc(rec)
    g_loss = -pred_gen.mean()
    last = list(S.decoder.parameters())[-1]
    n_g = torch.autograd.grad(nll, last, retain_graph=True)[0]
    g_g = torch.autograd.grad(g_loss, last, retain_graph=True)[0]
    d_weight = (torch.clamp(n_g.norm() / (g_g.norm() + 1e-4), 0.0, 1e4) * S.disc_weight).detach()
    loss = nll + d_weight * S.disc_factor * g_loss
    S.opt_g.zero_grad()
    loss.backward()
    r["g_grads"] = _grads(S.named_g)
    S.opt_g.step()
    r.update(rec=rec.detach(), pred_true=pred_true.detach(), pred_fake=pred_fake.detach(), pred_gen=pred_gen.detach(),
             gp_per_sample=reg.detach(), last_layer_shape=tuple(last.shape),
             scalars={"loss": loss.item(), "kl_loss": 0.0, "logvar": S.logvar.item(), "nll_loss": nll.item(), "rec_loss": r["rec_loss"],
                      "d_weight": d_weight.item(), "disc_factor": S.disc_factor.item(), "g_loss": g_loss.item(),
                      "d_loss": ((loss_real + loss_fake) / 2).item(), "p_true": torch.sigmoid(pred_true).mean().item(),
                      "p_fake": torch.sigmoid(pred_fake).mean().item(), "gp_loss": reg.mean().item()})
    r["uv"] = {p + k: v.detach().clone() for p, net in (("encoder.", S.encoder), ("decoder.", S.decoder), ("disc.", S.disc))
               for k, v in net.state_dict().items() if k.endswith(("weight_u", "weight_v"))}
    r["params"] = {k: p.detach().clone() for k, p in S.named_g + S.named_d}
    return r


def probe(S, x):
    """The discriminator alone, term by term, as the golden's ``p_*`` entries: hinge-real and penalty on ``x``, hinge-fake on
    ``0.5 * x.flip(0)``."""
    params = [p for _, p in S.named_d]
    xt = x.detach().clone().requires_grad_()
    pred = S.disc(xt)
    loss_real = hinge(pred, True)
    terms = {"real": torch.autograd.grad(loss_real, params, retain_graph=True)}
    reg = penalty_per_sample(pred, xt)
    terms["gp"] = torch.autograd.grad(reg.mean(), params, retain_graph=True, allow_unused=True)
    pred_f = S.disc(0.5 * x.flip(0))
    loss_fake = hinge(pred_f, False)
    terms["fake"] = torch.autograd.grad(loss_fake, params)
    grads = {t: {k: (torch.zeros_like(p) if g is None else g) for (k, p), g in zip(S.named_d, gs)} for t, gs in terms.items()}
    return dict(pred=pred.detach(), pred_fake=pred_f.detach(), loss_real=loss_real.item(), loss_fake=loss_fake.item(), gp=reg.mean().item(),
                gp_per_sample=reg.detach(), grads=grads, gp_none=[k for (k, _), g in zip(S.named_d, terms["gp"]) if g is None])


# ------------------------------------------------------------------------------------------------ the kernels in float64
def hinge_terms_ref(pred, mode):
    """ipoke_hinge_terms on a float64 column: (term, mean sigmoid, gradient column).  mode 0 real, 1 fake, 2 generator."""
    M = pred.numel()
    if mode == 2:
        return (-pred.mean()).item(), torch.sigmoid(pred).mean().item(), torch.full_like(pred, -1.0 / M)
    h = 1.0 - pred if mode == 0 else 1.0 + pred
    sign = -1.0 if mode == 0 else 1.0
    return h.clamp_min(0).mean().item(), torch.sigmoid(pred).mean().item(), torch.where(h > 0, sign / M, 0.0).to(pred.dtype)


def act_jvp_ref(y, xdot, act):
    """ipoke_act_jvp in float64: slope 1 for y > 0, else 0.2 (LeakyReLU) or 0 (ReLU) -- also at y == 0."""
    slope = 0.2 if act == "lrelu" else 0.0
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope)) * xdot


def gp_direction_ref(g):
    """ipoke_gp_direction in float64: (mean_n sum g_n^2, per-sample sums, v = (2 / N) g)."""
    s = g.pow(2).reshape(g.shape[0], -1).sum(1)
    return s.mean().item(), s, (2.0 / g.shape[0]) * g
