"""The 2-D poke and image autoencoders of iPOKE on the HIP kernels: the two small trainings whose encoder halves
``PokeMotionModel`` loads as ``poke_embedder`` and ``conditioner`` (reference models/conv_poke_encoder.py,
models/first_stage_image_conv.py, models/modules/autoencoders/fully_conv_models.py).

The parameter holders are the blocks of ``ipoke_amd.first_stage`` (reference state-dict names), the differentiable ops are those of
``ipoke_amd.autograd_ops`` (convolution, Group / InstanceNorm, spectral norm with power iteration, multi-tensor Adam).  New
here: the decoder, the autoencoder modules, the loss with a device-resident log-variance (``ipoke_l1_nll``, csrc/ae2d_loss.hip),
the two trainers and the plateau scheduler.

The image autoencoder's adversarial phase (epochs from ``training.pretrain`` on: PatchGAN ``define_D`` with gradient penalty and the
adaptive weight) lives in ``ipoke_amd.image_gan`` behind its own names, ``ConvAEGANModel`` and ``ImageEncoderGANTrainer``;
``ConvAEModel.training_loss`` here keeps refusing those epochs, and ``ImageEncoderTrainer`` stays the reconstruction phase.  Two quirks of
the reference that the new trainer keeps and states: both plateau schedulers act on the generator's optimiser (factor .5, then .1), and
Lightning's repetition of ``training_step`` per optimiser is not reproduced.

What is NOT built: the LPIPS perceptual term -- ``perceptual`` is a hook, ``None`` leaves the term out --, FID
validation, ``bce_loss``, ``PatchDiscriminator.gp`` and multi-GPU training of these two models.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import autograd_ops as A
from . import first_stage as FS
from . import first_stage_train as FT
from ._lib import check, ptr


# ---------------------------------------------------------------------------------------------- modules
class ConvDecoder(nn.Module):
    """fully_conv_models.py:96-133 with ``n_skip_stages = 0``."""

    def __init__(self, nf_in, in_channels, out_channels=3, dtype="bf16"):
        super().__init__()
        self.dtype, self.out_channels = dtype, out_channels
        self.n_stages = len(in_channels) - 1
        self.blocks = nn.ModuleList()
        self.in_block = FS.ResBlock(nf_in, in_channels[0], snorm=True, norm="group")
        for i, nf in enumerate(in_channels[1:]):
            # NB the upsampling blocks' Conv2dTransposeBlock maps the key "elu" to ReLU (util.py:41-42)
            self.blocks.append(FS.ResBlock(in_channels[i], nf, norm="group", upsampling=True, snorm=True))
        self.out_conv = FS.Conv2dBlock(in_channels[-1], out_channels, 3, 1, 1, norm="none", activation="tanh" if out_channels == 3 else "none")

    @property
    def out_act(self):
        return FS.ACT[self.out_conv.activation]


def encoder_depths(nf_max, n_stages):
    """``ConvEncoder.depths`` (fully_conv_models.py:33-59): the stages' widths, innermost first."""
    nf, depths = 32, [32]
    for _ in range(n_stages - 1):
        nf = min(2 * nf, nf_max)
        depths.insert(0, nf)
    return depths


def encode_train(enc, x, dt, pit):
    """``first_stage.ConvEncoder`` with gradients: x fp32 [N, C, H, W] -> the bottleneck's output (CL)."""
    N, C, H, W = x.shape
    first = enc.model[0]
    st = (x.stride(0), x.stride(1), 0, x.stride(2), x.stride(3))
    h = A.conv(first.conv, None, dt, src=(x, N, C, (1, H, W), st), w=A.effective_weight(first.conv, pit))
    h = A.norm(first.norm, h, dt, act=FS.ACT[first.activation])
    for blk in list(enc.model)[1:]:
        h = FT.res_block(blk, h, dt, pit=pit)
    return FT.res_block(enc.bottleneck[0], h, dt, pit=pit)


def decode_train(dec, h, dt, pit):
    """``ConvDecoder`` with gradients: the channels-last fp32 output of ``out_conv`` BEFORE its activation (the loss kernel applies it)."""
    x = FT.res_block(dec.in_block, h, dt, pit=pit)
    for blk in dec.blocks:
        x = FT.res_block(blk, x, dt, pit=pit)
    return FT.conv_block(dec.out_conv, x, dt, out_f32=True)


def _activate(pre, act):
    """act(pre) by the loss kernel's activation pass alone (no target): [M, C] fp32."""
    rec = torch.empty(pre.t.shape[0], pre.C, dtype=torch.float32, device=pre.t.device)
    check(_lib.lib().ipoke_l1_nll(ptr(pre.t), pre.t.shape[1], act, None, pre.N, pre.C, pre.S, 0, None, None, None, None, ptr(rec), pre.C,
                                  None, 0, None, None, _lib.current_stream()))
    return rec


def _to_nchw(rec, N, H, W):
    return rec.view(N, H, W, rec.shape[1]).permute(0, 3, 1, 2)


class _AutoencoderOps(nn.Module):
    """``train_forward`` / ``forward`` over ``self.encoder`` and ``self.decoder``."""

    def train_forward(self, x, power_iteration=True):
        """Differentiable encoder -> decoder pass.  Returns the CL of ``out_conv``'s fp32 output: for three channels the pre-tanh value.
        ``power_iteration``: one power iteration of every spectral-normalised convolution (torch's train mode)."""
        _lib.require_gpu()
        x = x.float().contiguous()
        h = encode_train(self.encoder, x, self.dtype, bool(power_iteration))
        return decode_train(self.decoder, h, self.dtype, bool(power_iteration))

    @torch.no_grad()
    def reconstruct(self, x):
        """Inference: fp32 NCHW reconstruction, the ops of ``train_forward(x, power_iteration=False)`` without a graph."""
        pre = self.train_forward(x, power_iteration=False)
        return _to_nchw(_activate(pre, self.decoder.out_act), pre.N, pre.dhw[1], pre.dhw[2]).contiguous()

    def invalidate_operands(self):
        """Drop cached weight operands (after an optimiser step or a state-dict load)."""
        for m in self.modules():
            m.__dict__.pop("_opcache", None)
        A.clear_operand_cache()


def _check_deterministic(arch):
    if not arch["deterministic"]:
        raise NotImplementedError("the shipped poke / image encoders are deterministic")


def _n_stages(config):
    return int(np.log2(config["data"]["spatial_size"][0] // config["architecture"]["min_spatial_size"]))


class ConvAutoencoder(_AutoencoderOps):
    """fully_conv_models.py:9-26 with both halves (``first_stage.FirstStageWrapper`` is the encoder half the second stage loads)."""

    def __init__(self, config, dtype="bf16"):
        super().__init__()
        self.config, self.dtype = config, dtype
        arch = config["architecture"]
        self.be_deterministic = arch["deterministic"]
        _check_deterministic(arch)
        n_stages = _n_stages(config)
        nf_in_enc = arch["nf_in"] + (3 if arch.get("poke_and_image", False) else 0)
        self.encoder = FS.ConvEncoder(nf_in_enc, arch["nf_max"], n_stages, dtype=dtype)
        self.decoder = ConvDecoder(arch["nf_max"], [arch["nf_max"]] + encoder_depths(arch["nf_max"], n_stages), out_channels=arch["nf_in"],
                                   dtype=dtype)

    def forward(self, x):
        return self.reconstruct(x)


# ---------------------------------------------------------------------------------------------- loss
class _L1NllFn(torch.autograd.Function):
    """(pre [M, ld], target [N, C, H, W], logvar, p [N, 1, 1, 1] or None, perc_weight) -> (nll, rec [M, C], stats): ``ipoke_l1_nll``.
    ``stats`` = {nll, sum |x - rec|, d nll / d logvar} (not differentiable, for logging).  Gradients flow to ``pre`` (from the nll and,
    through the activation, from whatever else reads ``rec``), to ``logvar`` and to ``p``."""

    @staticmethod
    def forward(ctx, pre_t, x, logvar, p, perc_weight, C, act):
        ctx.set_materialize_grads(False)
        N, _, H, W = x.shape
        S = H * W
        if x.dtype != torch.float32 or x.stride(1) != S or x.stride(2) != W or x.stride(3) != 1:
            x = x.float().contiguous()
        dev = pre_t.device
        lib = _lib.lib()
        rec = torch.empty(pre_t.shape[0], C, dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        grad = torch.empty_like(pre_t) if need else None
        out = torch.empty(3, dtype=torch.float32, device=dev)
        part = torch.empty(int(lib.ipoke_l1_nll_partials()), dtype=torch.float64, device=dev)
        p_flat = grad_p = None
        if p is not None:
            p_flat = p.detach().reshape(N).float().contiguous()
            grad_p = torch.empty(N, dtype=torch.float32, device=dev) if need else None
        lv = logvar.detach()
        check(lib.ipoke_l1_nll(ptr(pre_t), pre_t.shape[1], act, ptr(x), N, C, S, x.stride(0), ptr(lv), ptr(p_flat),
                               None if p is None else ptr(perc_weight), ptr(out), ptr(rec), C, ptr(grad), pre_t.shape[1], ptr(grad_p), ptr(part),
                               _lib.current_stream()))
        ctx.save_for_backward(grad, rec, out, grad_p)
        ctx.act, ctx.C, ctx.p_shape = act, C, None if p is None else tuple(p.shape)
        stats = out.clone()
        ctx.mark_non_differentiable(stats)
        return out[0], rec, stats

    @staticmethod
    def backward(ctx, d_nll, d_rec, _):
        grad, rec, out, grad_p = ctx.saved_tensors
        d_pre = d_lv = d_p = None
        if d_nll is not None:
            d_pre = grad * d_nll
            d_lv = out[2] * d_nll
            if grad_p is not None:
                d_p = (grad_p * d_nll).view(ctx.p_shape)
        if d_rec is not None:                    # the reconstruction also feeds the perceptual term
            g = d_rec * (1.0 - rec * rec) if ctx.act == _lib.ACT_TANH else d_rec
            if grad.shape[1] != ctx.C:
                g = torch.nn.functional.pad(g, (0, grad.shape[1] - ctx.C))
            d_pre = g if d_pre is None else d_pre + g
        return d_pre, None, d_lv, d_p, None, None, None


def nll_loss(pre, target, logvar, perc_weight, act, perceptual=None):
    """conv_poke_encoder.py:68-78 / first_stage_image_conv.py:138-149 on the decoder's output ``pre`` (CL, fp32): returns
    (nll, rec [N, C, H, W], stats, p).  ``perceptual``: callable (target_nchw, rec_nchw) -> [N, 1, 1, 1], differentiable in ``rec``; the
    reconstruction it reads comes from a first pass of the kernel, the loss from a second one that takes ``p``."""
    N, H, W = pre.N, pre.dhw[1], pre.dhw[2]
    p = None
    if perceptual is not None:
        _, rec0, _ = _L1NllFn.apply(pre.t, target, logvar, None, None, pre.C, act)
        p = perceptual(target, _to_nchw(rec0, N, H, W))
        if tuple(p.shape) != (N, 1, 1, 1):
            raise ValueError(f"perceptual must return [N, 1, 1, 1], got {tuple(p.shape)}")
    nll, rec, stats = _L1NllFn.apply(pre.t, target, logvar, p, perc_weight, pre.C, act)
    return nll, _to_nchw(rec, N, H, W), stats, p


class _LossState(nn.Module):
    """``logvar`` and the three weights both reference modules keep (conv_poke_encoder.py:24-27, first_stage_image_conv.py:29-32)."""

    def _register_loss_state(self):
        self.register_buffer("disc_factor", torch.tensor(1.), persistent=True)
        self.register_buffer("disc_weight", torch.tensor(1.), persistent=True)
        self.register_buffer("perc_weight", torch.tensor(1.), persistent=True)
        self.logvar = nn.Parameter(torch.ones(size=()) * 0.0)


class ConvPokeAE(_LossState):
    """conv_poke_encoder.py:16-47.  ``training_loss(batch)`` is the loss of ``training_step`` (:52-80)."""

    def __init__(self, config, dtype="bf16"):
        super().__init__()
        self.config = config
        arch = config["architecture"]
        self.be_deterministic = arch["deterministic"]
        self._register_loss_state()
        self.flow_ae = bool(arch.get("flow_ae", False))
        self.poke_and_image = bool(arch.get("poke_and_image", False))
        self.model = ConvAutoencoder(config, dtype=dtype)

    def select_input(self, batch):
        """(network input, target) as conv_poke_encoder.py:53-65."""
        poke = batch["poke"][0] if isinstance(batch["poke"], list) else batch["poke"]
        flow = batch["flow"]
        if self.poke_and_image:
            poke = torch.cat([poke, batch["images"][:, 0]], dim=1)
        return (flow if self.flow_ae else poke), flow

    def forward(self, batch):
        return self.model(self.select_input(batch)[0])

    def training_loss(self, batch, power_iteration=None, perceptual=None):
        x_in, target = self.select_input(batch)
        pit = self.training if power_iteration is None else bool(power_iteration)
        pre = self.model.train_forward(x_in, pit)
        return nll_loss(pre, target, self.logvar, self.perc_weight, self.model.decoder.out_act, perceptual)

    def invalidate_operands(self):
        self.model.invalidate_operands()


class ConvAEModel(_LossState, _AutoencoderOps):
    """first_stage_image_conv.py:21-83, reconstruction phase (epochs before ``training.pretrain``)."""

    def __init__(self, config, dtype="bf16"):
        super().__init__()
        self.config, self.dtype = config, dtype
        arch = config["architecture"]
        self.be_deterministic = arch["deterministic"]
        _check_deterministic(arch)
        self._register_loss_state()
        self.disc_start = config["training"]["pretrain"]
        self.current_epoch = 0
        n_stages = _n_stages(config)
        self.encoder = FS.ConvEncoder(arch["nf_in"], arch["nf_max"], n_stages, dtype=dtype)
        self.decoder = ConvDecoder(arch["nf_max"], [arch["nf_max"]] + encoder_depths(arch["nf_max"], n_stages), dtype=dtype)

    def select_input(self, batch):
        x = batch["images"][:, -1]
        return x, x

    def forward(self, x):
        return self.reconstruct(x)

    def training_loss(self, batch, power_iteration=None, perceptual=None):
        if self.current_epoch >= self.disc_start:
            raise NotImplementedError(
                f"epoch {self.current_epoch} >= training.pretrain = {self.disc_start}: the adversarial phase needs the PatchGAN discriminator "
                "(define_D), its gradient penalty and the adaptive weight, which are not built here")
        x, target = self.select_input(batch)
        pit = self.training if power_iteration is None else bool(power_iteration)
        pre = self.train_forward(x, pit)
        return nll_loss(pre, target, self.logvar, self.perc_weight, self.decoder.out_act, perceptual)


# ---------------------------------------------------------------------------------------------- scheduler
class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau for ``mode="min"`` on the host, acting on ``MultiTensorAdam.lr``."""

    def __init__(self, optimizer, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel", cooldown=0, min_lr=0.0, eps=1e-8):
        if mode != "min":
            raise ValueError("only mode='min' is implemented (both shipped schedulers monitor a loss)")
        if factor >= 1.0:
            raise ValueError("factor should be < 1.0")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError(f"threshold mode {threshold_mode} is unknown")
        self.optimizer = optimizer
        self.factor, self.patience, self.threshold, self.threshold_mode = float(factor), int(patience), float(threshold), threshold_mode
        self.cooldown, self.min_lr, self.eps = int(cooldown), float(min_lr), float(eps)
        self.best, self.num_bad_epochs, self.cooldown_counter, self.last_epoch = float("inf"), 0, 0, 0

    def is_better(self, a, best):
        if self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold)
        return a < best - self.threshold

    def step(self, metrics):
        current = float(metrics)
        self.last_epoch += 1
        if self.is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old = self.optimizer.lr
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.optimizer.lr = new
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, sd):
        self.__dict__.update(sd)


# ---------------------------------------------------------------------------------------------- trainers
class _AutoencoderTrainer:
    """``step(batch)`` = forward with one power iteration, loss, backward, Adam update -- everything on the device, no host read."""

    def __init__(self, model, params, lr, weight_decay, perceptual, scheduler):
        self.model, self.perceptual = model, perceptual
        self.opt = A.MultiTensorAdam(params, lr, betas=(0.9, 0.999), weight_decay=weight_decay, eps=1e-8)
        self.scheduler = ReduceLROnPlateau(self.opt, **scheduler)

    def _loss(self, batch, power_iteration):
        return self.model.training_loss(batch, power_iteration=power_iteration, perceptual=self.perceptual)

    def _rec_loss_mean(self, rec, stats, p):
        """mean of ``rec_loss`` = |x - rec| + perc_weight * p over its N * C * H * W elements."""
        mean = stats[1] / rec.numel()
        if p is not None:
            mean = mean + self.model.perc_weight * p.detach().mean()
        return mean

    def step(self, batch):
        self.model.train()
        self.opt.zero_grad()
        nll, rec, stats, p = self._loss(batch, True)
        nll.backward()
        self.opt.step()
        self.model.invalidate_operands()
        self.last_rec = rec.detach()
        return self._train_dict(nll.detach(), rec, stats, p)

    @torch.no_grad()
    def validation_step(self, batch):
        """``val/loss``, ``val/nll_loss``, ``val/logvar`` and the MEAN of the reference's ``val/rec_loss`` map, as device scalars.
        Spectral norm is evaluated without power iteration (torch's eval mode)."""
        self.model.eval()
        nll, rec, stats, p = self._loss(batch, False)
        return {"val/loss": nll, "val/nll_loss": nll, "val/logvar": self.model.logvar.detach(), "val/rec_loss": self._rec_loss_mean(rec, stats, p)}

    def on_validation_epoch_end(self, mean_val_loss):
        """The scheduler monitors the epoch's mean validation loss."""
        self.scheduler.step(mean_val_loss)

    def state_dict(self):
        return {"model": self.model.state_dict(), "opt": self.opt.state_dict(), "scheduler": self.scheduler.state_dict()}

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd["model"])
        self.model.invalidate_operands()
        self.opt.load_state_dict(sd["opt"])
        self.scheduler.load_state_dict(sd["scheduler"])


class PokeEncoderTrainer(_AutoencoderTrainer):
    """Training of ``ConvPokeAE``: Adam over ALL parameters including ``logvar`` (conv_poke_encoder.py:177) and
    ``ReduceLROnPlateau(factor=.5, patience=1, min_lr=1e-8, threshold=1e-4, 'abs')`` (:179-180).

    ``perceptual``: any callable ``(target_nchw, rec_nchw) -> [N, 1, 1, 1]`` differentiable in ``rec``; the trainer adds
    ``perc_weight * p`` as conv_poke_encoder.py:70-73 does.  It receives the two-channel flow maps as they are (the reference appends a
    zero channel for its three-channel LPIPS network; a callable that needs three channels does that itself).  With ``None`` the
    perceptual term is ABSENT from the loss: LPIPS is not part of this package."""

    def __init__(self, model, lr=1e-3, weight_decay=0.0, perceptual=None):
        super().__init__(model, list(model.parameters()), lr, weight_decay, perceptual,
                         dict(factor=.5, patience=1, min_lr=1e-8, threshold=1e-4, threshold_mode="abs"))

    def _train_dict(self, nll, rec, stats, p):
        return {"train/loss": nll, "train/logvar": self.model.logvar.detach(), "train/nll_loss": nll}


class ImageEncoderTrainer(_AutoencoderTrainer):
    """Training of ``ConvAEModel`` before ``training.pretrain``: the reference's parameter groups encoder / logvar / decoder share one
    learning rate and weight decay (first_stage_image_conv.py:275-282), so they are one multi-tensor Adam over the parameters in that order and ``ReduceLROnPlateau(factor=.5, patience=0, min_lr=1e-8, threshold=1e-3, 'rel')`` (:287-288).
    The discriminator's optimiser and scheduler belong to the adversarial phase, which ``ConvAEModel.training_loss`` refuses.
    ``perceptual`` as for ``PokeEncoderTrainer`` (three-channel images)."""

    def __init__(self, model, lr=2e-4, weight_decay=0.0, perceptual=None):
        params = list(model.encoder.parameters()) + [model.logvar] + list(model.decoder.parameters())
        super().__init__(model, params, lr, weight_decay, perceptual,
                         dict(factor=.5, patience=0, min_lr=1e-8, threshold=1e-3, threshold_mode="rel"))

    def _train_dict(self, nll, rec, stats, p):
        zero = torch.zeros((), device=nll.device)
        return {"train/loss": nll, "train/kl_loss": zero, "train/logvar": self.model.logvar.detach(), "train/nll_loss": nll,
                "train/rec_loss": self._rec_loss_mean(rec, stats, p), "train/d_weight": zero, "train/disc_factor": zero, "train/g_loss": zero}
