"""The adversarial phase of the image autoencoder on the HIP kernels (reference models/first_stage_image_conv.py:85-168): the PatchGAN
``define_D(3, 64, 'basic')`` of models/modules/discriminators/patchgan.py:255-325 with its gradient penalty, the adaptive weight on the
generator term (disc_utils.py:9-20) and the step that ties them to the autoencoder of ``ipoke_amd.autoencoder2d``.

``ConvAEModel`` / ``ImageEncoderTrainer`` stay what they are (the reconstruction phase; ``ConvAEModel.training_loss`` keeps refusing the
epochs from ``training.pretrain`` on).  The adversarial epochs live behind the new names ``ConvAEGANModel`` and
``ImageEncoderGANTrainer``.

The penalty's double backward (``gp``, ``create_graph=True`` in the reference) is evaluated forward-over-reverse, as
``TemporalDiscriminator.gp2`` does it: one ordinary backward gives g = d sum(pred) / dx, ``ipoke_gp_direction`` its value and the direction
v = (2 / B) g, and a primal-plus-tangent pass propagates D_v -- the same convolution kernels on the tangent (without their bias),
``ipoke_act_jvp`` for conv 0's fused LeakyReLU and ``ipoke_groupnorm_tangent`` for GroupNorm + LeakyReLU.  The last one is
``ipoke_groupnorm_jvp`` with ordered sums: that kernel adds with float atomics, and a step that contains it is not reproducible bit for
bit.  ``ipoke_hinge_terms`` gives each hinge / generator term, mean sigmoid(pred) and the gradient column in one pass.

Not built: LPIPS (``perceptual`` is a hook), FID validation, ``bce_loss``, ``PatchDiscriminator.gp``, multi-GPU.
"""
import torch
import torch.nn as nn

from . import _lib, autograd_ops as A, first_stage as FS, nn as K, ops
from ._lib import check, ptr
from .autoencoder2d import ConvAEModel, ImageEncoderTrainer, ReduceLROnPlateau, nll_loss


# ---------------------------------------------------------------------------------------------- ops
class _HingeFn(torch.autograd.Function):
    """(prediction column [M] fp32 at any pitch, mode) -> (term, mean sigmoid(pred)): ``ipoke_hinge_terms``."""

    @staticmethod
    def forward(ctx, p, mode):
        lib = _lib.lib()
        M = p.numel()
        ld = p.stride(0) if M > 1 else 1
        out = torch.empty(2, dtype=torch.float32, device=p.device)
        grad = torch.empty(M, dtype=torch.float32, device=p.device)
        part = torch.empty(int(lib.ipoke_hinge_terms_partials()), dtype=torch.float64, device=p.device)
        check(lib.ipoke_hinge_terms(ptr(p), ld, M, mode, ptr(out), ptr(grad), 1, ptr(part), _lib.current_stream()))
        ctx.save_for_backward(grad)
        prob = out[1].clone()
        ctx.mark_non_differentiable(prob)
        return out[0], prob

    @staticmethod
    def backward(ctx, d, _):
        (grad,) = ctx.saved_tensors
        return grad * d, None


class _ActJvpFn(torch.autograd.Function):
    """ydot = act'(y) * xdot (``ipoke_act_jvp``); the backward on xdot is the same launch, y gets none (act' is piecewise constant)."""

    @staticmethod
    def _run(y_t, xd_t, C, act, dt):
        out = torch.empty_like(xd_t)
        check(_lib.lib().ipoke_act_jvp(ptr(y_t), y_t.shape[1], ptr(xd_t), xd_t.shape[1], ptr(out), out.shape[1], y_t.shape[0], C, out.shape[1],
                                       act, ops._dt(dt), _lib.current_stream()))
        return out

    @staticmethod
    def forward(ctx, y_t, xd_t, C, act, dt):
        ctx.save_for_backward(y_t)
        ctx.args = (C, act, dt)
        return _ActJvpFn._run(y_t, xd_t, C, act, dt)

    @staticmethod
    def backward(ctx, q):
        (y_t,) = ctx.saved_tensors
        return None, _ActJvpFn._run(y_t, q.contiguous(), *ctx.args), None, None, None


class _NormTangentFn(torch.autograd.Function):
    """Tangent of GroupNorm + activation and its backward (``ipoke_groupnorm_tangent`` / ``_bwd``): gradients on xdot, on the primal
    input (through the statistics) and on gamma."""

    @staticmethod
    def forward(ctx, x_t, xd_t, y_t, gamma, meta):
        yd = torch.zeros_like(xd_t) if xd_t.shape[1] > meta["C"] else torch.empty_like(xd_t)
        g32 = gamma.detach().float().contiguous()
        check(_lib.lib().ipoke_groupnorm_tangent(ptr(x_t), x_t.shape[1], ptr(xd_t), xd_t.shape[1], ptr(y_t), y_t.shape[1], ptr(yd), yd.shape[1],
                                                 ptr(g32), meta["N"], meta["S"], meta["C"], meta["G"], meta["act"], 1e-5, ops._dt(meta["dtype"]),
                                                 _lib.current_stream()))
        ctx.save_for_backward(x_t, xd_t, y_t, g32)
        ctx.meta = meta
        return yd

    @staticmethod
    def backward(ctx, q):
        x_t, xd_t, y_t, g32 = ctx.saved_tensors
        m = ctx.meta
        q = q.contiguous()
        alloc = torch.zeros_like if xd_t.shape[1] > m["C"] else torch.empty_like
        dxd, dx = alloc(xd_t), alloc(x_t)
        rows = torch.empty(m["N"], m["C"], dtype=torch.float32, device=q.device)
        dgamma = torch.empty(m["C"], dtype=torch.float32, device=q.device)
        lib, s = _lib.lib(), _lib.current_stream()
        check(lib.ipoke_groupnorm_tangent_bwd(ptr(x_t), x_t.shape[1], ptr(xd_t), xd_t.shape[1], ptr(y_t), y_t.shape[1], ptr(q), q.shape[1],
                                              ptr(dxd), dxd.shape[1], ptr(dx), dx.shape[1], ptr(rows), ptr(g32), m["N"], m["S"], m["C"], m["G"],
                                              m["act"], 1e-5, ops._dt(m["dtype"]), s))
        check(lib.ipoke_reduce_rows(ptr(rows), ptr(dgamma), m["N"], m["C"], s))
        return dx, dxd, None, dgamma, None


def gp_direction(g):
    """g [N, ...] fp32 -> (v = (2 / N) g, out [1 + N] = {mean_n sum g_n^2, sum g_n^2 per sample}): ``ipoke_gp_direction``."""
    lib = _lib.lib()
    g = g.detach().float().contiguous()
    N = g.shape[0]
    v = torch.empty_like(g)
    out = torch.empty(1 + N, dtype=torch.float32, device=g.device)
    part = torch.empty(int(lib.ipoke_gp_direction_partials(N)), dtype=torch.float64, device=g.device)
    check(lib.ipoke_gp_direction(ptr(g), N, g.numel() // N, ptr(v), ptr(out), ptr(part), _lib.current_stream()))
    return v, out


class _frozen:
    """Inside the block the parameters take no gradient: a pass that is differentiated w.r.t. its input alone skips the weight-gradient
    half of every convolution's backward."""

    def __init__(self, module):
        self.params = [p for p in module.parameters() if p.requires_grad]

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


# ---------------------------------------------------------------------------------------------- discriminator
class NLayerDiscriminator(nn.Module):
    """``define_D(3, ndf, 'basic')`` = ``NLayerDiscriminator(3, ndf, n_layers=3, norm_layer=GroupNorm(16, affine))`` (patchgan.py:116-151,
    255-302) under the reference's 21 state-dict names: ``model.0`` the first 4 x 4 / stride 2 convolution (spectral norm, bias) with
    LeakyReLU(0.2); ``model.{2,5,8}`` the inner convolutions (spectral norm, no bias: GroupNorm has affine parameters) -- stride 2, 2, 1 --
    each followed by ``model.{3,6,9}`` = GroupNorm(16) and LeakyReLU(0.2); ``model.11`` the one-channel head, a plain convolution with
    bias.  A 32 x 32 image gives a 2 x 2 map, a 64 x 64 image 6 x 6.

    Fresh initialisation is what ``init_net`` effectively does: ``init.normal_(m.weight.data, 0, 0.02)`` and zero biases for every
    convolution.  On the spectral-normalised ones ``weight`` is the attribute the forward pre-hook recomputes from ``weight_orig`` at
    every call, so the normal init is overwritten there and ``weight_orig`` keeps ``nn.Conv2d``'s default initialisation; only the plain
    head really becomes N(0, 0.02).  Here: biases zero, head weight N(0, 0.02), ``weight_orig`` as ``first_stage._Conv`` draws it.
    """

    def __init__(self, ndf=64, n_layers=3, gp_weight=1.0, dtype="bf16"):
        super().__init__()
        self.dtype, self.gp_weight, self.bce_loss = dtype, float(gp_weight), False
        seq = [FS._Conv(3, ndf, 4, 2, 1, bias=True, snorm=True, dims=2), nn.Identity()]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            seq += [FS._Conv(ndf * prev, ndf * mult, 4, 2 if n < n_layers else 1, 1, bias=False, snorm=True, dims=2),
                    FS._Norm("group", ndf * mult), nn.Identity()]
        head = FS._Conv(ndf * mult, 1, 4, 1, 1, bias=True, snorm=False, dims=2)
        with torch.no_grad():
            head.weight.normal_(0.0, 0.02)
        self.model = nn.Sequential(*seq, head)

    def _layers(self):
        mods = list(self.model)
        return mods[0], [(mods[i], mods[i + 1]) for i in range(2, len(mods) - 1, 3)], mods[-1]

    @staticmethod
    def _to_pred(o, N):
        return o.t[:, :1].float().reshape(N, o.dhw[1], o.dhw[2], 1).permute(0, 3, 1, 2)

    def forward(self, x, power_iteration=None):
        """x [N, 3, H, W] on the GPU -> pred [N, 1, h, w] fp32.  ``power_iteration`` (default: ``self.training``): one power iteration of
        every spectral-normalised convolution.  The gradient flows to ``x`` when ``x.requires_grad`` (the generator side enters through
        a channels-last copy; otherwise the image is read in place)."""
        _lib.require_gpu()
        dt = self.dtype
        pit = self.training if power_iteration is None else bool(power_iteration)
        first, inner, head = self._layers()
        N, C, H, W = x.shape
        w0 = A.effective_weight(first, pit)
        if x.requires_grad:
            xcl = A.pad_cols(x.permute(0, 2, 3, 1).reshape(-1, C), K.round_up(C, K.e16(dt)), dt)
            h = A.conv(first, K.CL(xcl, N, (1, H, W), C), dt, act=_lib.ACT_LRELU02, w=w0)
        else:
            x = x.float()
            st = (x.stride(0), x.stride(1), 0, x.stride(2), x.stride(3))
            h = A.conv(first, None, dt, act=_lib.ACT_LRELU02, src=(x, N, C, (1, H, W), st), w=w0)
        for cv, nm in inner:
            h = A.norm(nm, A.conv(cv, h, dt, w=A.effective_weight(cv, pit)), dt, act=_lib.ACT_LRELU02)
        return self._to_pred(A.conv(head, h, dt, out_f32=True), N)

    def tangent(self, x, v):
        """pred_dot [N, 1, h, w]: the derivative of ``forward(x)`` along the input direction ``v`` (both [N, 3, H, W] fp32 without a
        gradient), differentiable in the parameters.  The spectral-norm buffers are not iterated."""
        _lib.require_gpu()
        dt = self.dtype
        first, inner, head = self._layers()
        N, C, H, W = x.shape
        x, v = x.float().contiguous(), v.float().contiguous()
        st = (x.stride(0), x.stride(1), 0, x.stride(2), x.stride(3))
        w0 = A.effective_weight(first, False)
        hp = A.conv(first, None, dt, act=_lib.ACT_LRELU02, src=(x, N, C, (1, H, W), st), w=w0)
        hd = A.conv_weight(None, w0, None, first.k, first.stride, first.pad, dt, src=(v, N, C, (1, H, W), st))        # linear part: no bias
        hd = K.CL(_ActJvpFn.apply(hp.t, hd.t, hp.C, _lib.ACT_LRELU02, dt), N, hp.dhw, hp.C)
        for cv, nm in inner:
            w = A.effective_weight(cv, False)
            xp, xd = A.conv(cv, hp, dt, w=w), A.conv(cv, hd, dt, w=w)
            hp = A.norm(nm, xp, dt, act=_lib.ACT_LRELU02)
            meta = dict(N=xp.N, S=xp.S, C=xp.C, G=nm.groups, dtype=dt, act=_lib.ACT_LRELU02)
            hd = K.CL(_NormTangentFn.apply(xp.t, xd.t, hp.t, nm.weight, meta), N, xp.dhw, xp.C)
        return self._to_pred(A.conv_weight(hd, head.weight, None, head.k, head.stride, head.pad, dt, out_f32=True), N)

    @staticmethod
    def hinge(pred, mode):
        """(term, mean sigmoid(pred)) of a prediction map: ``ipoke_hinge_terms``, mode ``_lib.HINGE_*``."""
        return _HingeFn.apply(pred.reshape(-1), mode)

    def loss(self, pred, real):
        """The hinge term (patchgan.py:304-314): mean relu(1 - pred) for real, mean relu(1 + pred) for fake predictions."""
        return self.hinge(pred, _lib.HINGE_REAL if real else _lib.HINGE_FAKE)[0]

    def generator_loss(self, pred):
        """-mean(pred) (first_stage_image_conv.py:122)."""
        return self.hinge(pred, _lib.HINGE_GENERATOR)[0]

    def gp(self, x):
        """The gradient penalty mean_b sum (d sum(pred) / dx)^2 (patchgan.py:316-325 and the ``.mean()`` of first_stage_image_conv.py:99) on
        the images ``x``: a scalar whose value is the penalty and whose gradient w.r.t. the parameters is the penalty's.  Unlike the
        reference's ``gp(pred, x)`` it runs its own passes, on the spectral-norm buffers as they are (no iteration): one forward and
        backward for g, then the primal-plus-tangent pass along v = (2 / B) g.  No PyTorch double backward is involved; the head's bias
        takes no part in the penalty and receives no gradient from it."""
        xg = x.detach().float().requires_grad_(True)
        with _frozen(self):
            (g,) = torch.autograd.grad(self.forward(xg, power_iteration=False).sum(), xg)
        v, out = gp_direction(g)
        self.last_gp_per_sample = out[1:]
        tsum = self.tangent(x.detach(), v).sum()
        return tsum + (out[0] - tsum).detach()

    def invalidate_operands(self):
        for m in self.modules():
            m.__dict__.pop("_opcache", None)
        A.clear_operand_cache()


# ---------------------------------------------------------------------------------------------- model
class ConvAEGANModel(ConvAEModel):
    """first_stage_image_conv.py:21-83 with its discriminator: ``ConvAEModel``'s encoder, decoder, ``logvar`` and buffers plus ``disc``.
    The state dict equals the reference module's for ``encoder.* / decoder.* / disc.* / logvar / disc_factor / disc_weight / perc_weight``
    (the reference also stores its LPIPS and Inception networks, which are not part of this package)."""

    def __init__(self, config, dtype="bf16"):
        super().__init__(config, dtype=dtype)
        self.disc = NLayerDiscriminator(64, 3, gp_weight=config["training"]["gp_weight"], dtype=dtype)

    def reconstruction_loss(self, batch, power_iteration=True, perceptual=None):
        """(pre, nll, rec, stats, p): the decoder's output and ``nll_loss`` on it, whatever the epoch."""
        x, target = self.select_input(batch)
        pre = self.train_forward(x, power_iteration)
        return (pre,) + nll_loss(pre, target, self.logvar, self.perc_weight, self.decoder.out_act, perceptual)


# ---------------------------------------------------------------------------------------------- trainer
class ImageEncoderGANTrainer(ImageEncoderTrainer):
    """Training of ``ConvAEGANModel``: one body of the reference's ``training_step`` (first_stage_image_conv.py:132-192) per ``step(batch)``.

    ``model.current_epoch < training.pretrain``: the step of ``ImageEncoderTrainer``, bit for bit; the discriminator is untouched.
    From ``pretrain`` on, in the reference's order: autoencoder forward (one power iteration) and nll; ``opt_d.zero_grad``; ``disc(x)``
    (power iteration 1) and the hinge-real backward; ``gp_weight * gp`` backward on the buffers that iteration left; ``disc(rec.detach())``
    (iteration 2) and the hinge-fake backward; ``opt_d.step`` (Adam, betas (0.9, 0.999), the discriminator only); ``disc(rec)`` with the
    updated weights (iteration 3) for ``g_loss``; ``d_weight = clamp(|d nll / d b| / (|d g_loss / d b| + 1e-4), 0, 1e4) * disc_weight`` with
    b the bias of ``decoder.out_conv`` (``list(decoder.parameters())[-1]``), detached; ``loss = nll + d_weight * disc_factor * g_loss``;
    ``opt_g.zero_grad``, backward, ``opt_g.step``.  Both bias gradients are column sums of the gradients on the decoder's output, which is
    also where the two terms are combined, so the generator's backward pass runs once; the gradients the reference's backward deposits
    in the discriminator there are discarded by the next step's ``opt_d.zero_grad`` and are not computed.  Everything stays on the
    device: no host read inside ``step``; ``d_weight`` and every entry of the returned dict are device scalars.

    Two quirks of the reference are kept.  (1) BOTH plateau schedulers act on the GENERATOR's optimiser (first_stage_image_conv.py:287-290
    passes ``opt_g`` twice): factor .5 then factor .1 in that order, each ``patience 0, min_lr 1e-8, threshold 1e-3 rel``; the
    discriminator's learning rate stays constant.  (2) Lightning calls ``training_step`` once per optimiser, so the reference runs the
    body twice per batch; that repetition is harness behaviour and is not reproduced: one ``step`` is one body.
    """

    def __init__(self, model, lr=2e-4, weight_decay=0.0, perceptual=None):
        super().__init__(model, lr=lr, weight_decay=weight_decay, perceptual=perceptual)
        self.opt_d = A.MultiTensorAdam(list(model.disc.parameters()), lr, betas=(0.9, 0.999), weight_decay=weight_decay, eps=1e-8)
        self.scheduler_d = ReduceLROnPlateau(self.opt, factor=.1, patience=0, min_lr=1e-8, threshold=1e-3, threshold_mode="rel")

    def _loss(self, batch, power_iteration):
        return self.model.reconstruction_loss(batch, power_iteration, self.perceptual)[1:]

    def step(self, batch):
        m = self.model
        if m.current_epoch < m.disc_start:
            return super().step(batch)
        m.train()
        disc = m.disc
        x, _ = m.select_input(batch)
        pre, nll, rec, stats, p = m.reconstruction_loss(batch, True, self.perceptual)
        # ---- discriminator (train_disc, :85-115)
        self.opt_d.zero_grad()
        loss_real, p_true = disc.hinge(disc(x.detach()), _lib.HINGE_REAL)
        loss_real.backward()
        gp = torch.zeros((), device=x.device)
        if disc.gp_weight > 0:
            gp = disc.gp(x)
            (disc.gp_weight * gp).backward()
        loss_fake, p_fake = disc.hinge(disc(rec.detach()), _lib.HINGE_FAKE)
        loss_fake.backward()
        self.opt_d.step()
        disc.invalidate_operands()
        # ---- generator term on the updated discriminator (:118-122); its weights take no gradient here
        with _frozen(disc):
            g_loss = disc.generator_loss(disc(rec))
            (dg_pre,) = torch.autograd.grad(g_loss, [pre.t], retain_graph=True)
        dn_pre, dn_lv = torch.autograd.grad(nll, [pre.t, m.logvar])
        # ---- adaptive weight (disc_utils.py:9-20): the bias of out_conv adds to every row of `pre`
        C = pre.C
        n_norm = dn_pre[:, :C].double().sum(0).norm()
        g_norm = dg_pre[:, :C].double().sum(0).norm()
        d_weight = (torch.clamp(n_norm / (g_norm + 1e-4), 0.0, 1e4).float() * m.disc_weight).detach()
        disc_factor = m.disc_factor.detach().clone()
        scale = d_weight * disc_factor
        loss = nll.detach() + scale * g_loss.detach()
        self.opt.zero_grad()
        torch.autograd.backward([pre.t], [dn_pre + scale * dg_pre])
        m.logvar.grad = dn_lv
        self.opt.step()
        m.invalidate_operands()
        self.last_rec = rec.detach()
        return {"train/loss": loss, "train/kl_loss": torch.zeros((), device=x.device), "train/logvar": m.logvar.detach(),
                "train/nll_loss": nll.detach(), "train/rec_loss": self._rec_loss_mean(rec, stats, p), "train/d_weight": d_weight,
                "train/disc_factor": disc_factor, "train/g_loss": g_loss.detach(), "train/d_loss": ((loss_real + loss_fake) / 2.).detach(),
                "train/p_true": p_true, "train/p_fake": p_fake, "train/gp_loss": gp.detach()}

    def on_validation_epoch_end(self, mean_val_loss):
        """Both schedulers monitor the epoch's mean validation loss and both act on the generator's optimiser, factor .5 first."""
        self.scheduler.step(mean_val_loss)
        self.scheduler_d.step(mean_val_loss)

    def state_dict(self):
        sd = super().state_dict()
        sd.update(opt_d=self.opt_d.state_dict(), scheduler_d=self.scheduler_d.state_dict())
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.opt_d.load_state_dict(sd["opt_d"])
        self.scheduler_d.load_state_dict(sd["scheduler_d"])
