"""First-stage VAE *training* on the HIP kernels: encoder -> ConvGRU -> SPADE decoder with
gradients, L1 + KL loss (reference models/first_stage_motion_model.py:469-522 forward, :263-276 loss terms,
utils/losses.py:47-48 KL).

The parameter holders are the modules of ``ipoke_amd.first_stage`` (reference state-dict names); the differentiable ops they are
run with -- convolution, norms, ConvGRU, latent and loss kernels, spectral norm, multi-tensor Adam -- are those of
``ipoke_amd.autograd_ops``.  This file is the VAE's graph over them (``basic_block`` .. ``first_stage_forward_loss``) and
``FirstStageTrainer``.

PyTorch autograd only records the graph.  In train mode every spectral-normalised conv runs one power iteration per
forward *call*, i.e. T-1 times per step for the decoder (util.py:52, 252): frame t is decoded with W / sigma_t.  Kept -- but
conv(x, W / sigma_t) = conv(x, W) / sigma_t and sigma_t is a per-frame SCALAR, so the T - 1 ConvGRU steps run first (sequential, 8 x 8)
and the decoder runs ONCE over the (frame, clip)-ordered batch of all frames with one operand of W_orig and 1 / sigma_t as a per-image
scale of the GEMM epilogue (ipoke_conv_desc.row_scale); the backward pass needs one weight gradient per convolution (rows pre-scaled
by 1 / sigma_t) plus the scalars <dY_t, Y_t> for sigma_t's own gradient (ipoke_rowscale_bwd, ipoke_spectral_bwd_frames).
``_FRAME_BATCH = False`` (a test hook) keeps the frame-by-frame evaluation (same mathematics, 15 x the decoder launches).
"""
import torch

from . import _lib, nn as K, ops
from . import first_stage as FS
from .autograd_ops import (MultiTensorAdam, add_act, begin_forward_pass, conv, conv_weight, effective_weight, group_norm, gru_cell,
                           gru_gate_weights, gru_native_ok, gru_unroll, kl_loss, l1_tanh_loss, norm, pad_cols,
                           precompute_power_iterations, refresh_operand_cache, reparameterize, stem, stem_folds, take_operand_cache,
                           wgrad_side_stream)

# test hooks (tests/test_train_mode_gpu.py runs every variant against the oracle)
_SN_AHEAD = True        # False: one power iteration per decoder call, at the call
_HOIST_SPADE = True     # False: per-frame SPADE maps as the reference computes them
_FRAME_BATCH = True     # all generated frames decoded as ONE batch (module docstring); False: frame by frame (c4 94.8 vs 57.2 ms)


# ------------------------------------------------------------------------------------------------ model pieces
def basic_block(blk, x, dtype):
    out = norm(blk.bn1, conv(blk.conv1, x, dtype), dtype, act=_lib.ACT_RELU)
    res = x if blk.downsample is None else norm(blk.downsample[1], conv(blk.downsample[0], x, dtype), dtype)
    return norm(blk.bn2, conv(blk.conv2, out, dtype), dtype, act=_lib.ACT_RELU, res=res)


def encode(enc, x, eps):
    """ResNetMotionEncoder.forward with gradients: x [B,3,T,H,W] fp32 -> (z, mu, logvar) as [M, Z] fp32 rows."""
    dt = enc.dtype
    B, C, T, H, W = x.shape
    st = (x.stride(0), x.stride(1), x.stride(2), x.stride(3), x.stride(4))
    if stem_folds(enc.conv1, x):
        h = stem(x, enc.conv1.weight, dt)
    else:
        h = conv(enc.conv1, None, dt, src=(x, B, C, (T, H, W), st))
    h = norm(enc.bn1, h, dt, act=_lib.ACT_RELU)
    layers = [enc.layer1, enc.layer2, enc.layer3] + ([enc.layer4] if enc.stride4 is not None else []) + ([enc.layer5] if enc.has5 else [])
    for layer in layers:
        for blk in layer:
            h = basic_block(blk, h, dt)
    if h.dhw[0] != 1:
        raise ValueError("temporal extent after the encoder must be 1")
    w_head = torch.cat([enc.conv_mu.weight, enc.conv_var.weight], 0)
    b_head = torch.cat([enc.conv_mu.bias, enc.conv_var.bias])
    mulv = conv_weight(h, w_head, b_head, (1, 3, 3), (1, 1, 1), (0, 1, 1), dt)
    z, mu, lv = reparameterize(mulv.t, ops.to_state(eps), enc.z_dim, dt)
    return z, mu, lv, h.dhw


def conv_block(blk, x, dtype, res=None, out_f32=False, pit=False, frames=None):
    w = effective_weight(blk.conv, pit, frames)
    if blk.norm is None:
        act = FS.ACT[blk.activation] if res is None else _lib.ACT_NONE
        if out_f32:
            act = _lib.ACT_NONE             # the loss kernel applies tanh
        y = conv(blk.conv, x, dtype, act=act, out_f32=out_f32, w=w)
        return y if res is None else add_act(y, res, dtype, FS.ACT[blk.activation])
    return norm(blk.norm, conv(blk.conv, x, dtype, w=w), dtype, act=FS.ACT[blk.activation], res=res, sole_reader=True)


def convT_block(blk, x, dtype, pit=False, frames=None):
    w = effective_weight(blk.conv, pit, frames)
    if blk.norm is None:
        return conv(blk.conv, x, dtype, act=blk.act, w=w)
    return norm(blk.norm, conv(blk.conv, x, dtype, w=w), dtype, act=blk.act, sole_reader=True)


def res_block(blk, x, dtype, pit=False, frames=None):
    first = convT_block if isinstance(blk.conv1, FS.Conv2dTransposeBlock) else conv_block
    rc = blk.res_conv if blk.convolve_res else None
    if rc is not None and rc.norm is not None and blk.conv2.norm is None and blk.conv2.activation == "none":
        # out = conv2(conv1(x)) + act(norm(res_conv(x))): the sum rides on the skip path's norm pass, forward (the residual joins behind
        # the activation) and backward (its gradient is dy; act' from the recomputed pre-activation value, the saved output is not read)
        y2 = conv_block(blk.conv2, first(blk.conv1, x, dtype, pit=pit, frames=frames), dtype, pit=pit, frames=frames)
        w = effective_weight(rc.conv, pit, frames)
        act = rc.act if isinstance(rc, FS.Conv2dTransposeBlock) else FS.ACT[rc.activation]
        return norm(rc.norm, conv(rc.conv, x, dtype, w=w), dtype, act=act, res=y2, sole_reader=True, res_post=True)
    if blk.convolve_res:
        rfirst = convT_block if isinstance(blk.res_conv, FS.Conv2dTransposeBlock) else conv_block
        res = rfirst(blk.res_conv, x, dtype, pit=pit, frames=frames)
    else:
        res = x
    return conv_block(blk.conv2, first(blk.conv1, x, dtype, pit=pit, frames=frames), dtype, res=res, pit=pit, frames=frames)


def spade_modulation(sp, y_nchw, size, dtype):
    N = y_nchw.shape[0]
    ycl = K.bilinear_cl(y_nchw, size)
    # the resized start frame as dense channels-last pixels of the compute dtype, zero padded to one 16-byte chunk: the same rounding an
    # in-place fp32 read applies on load, but the convolution and -- above all -- its weight gradient run on the LDS-DMA kernels instead
    # of the register-staged fp32-source ones (4 x ~400 us per c4 step for 2.3 GFLOP each)
    x = K.CL(pad_cols(ycl, K.e16(dtype), dtype), N, (1, size[0], size[1]), 3)
    h = conv(sp.conv, x, dtype, act=_lib.ACT_LRELU02)
    return conv(sp.conv_gamma, h, dtype), conv(sp.conv_beta, h, dtype)


def spade_modulations(gen, start_frame, dtype):
    """(gamma, beta) maps of every SPADE block for a clip's start frame.  util.py:494-500 recomputes them in every decoder call; they
    are a function of the start frame and of three plain (not spectral-normalised) convolutions only, so the frames of a clip share
    them: computed once per pass, every frame's GroupNorm reads the same maps, autograd sums the frames' gradients into them and the
    three convolutions are differentiated once -- the same values, (T - 2) / (T - 1) fewer SPADE convolutions in both directions."""
    size, mods = 8, []
    for sp in gen.spade_blocks:
        size *= 2
        mods.append(spade_modulation(sp, start_frame, (size, size), dtype))
    return mods


def decode_frame(gen, h, start_frame, dtype, pit, mods=None, frames=None):
    """SpadeCondConvDecoder.forward for one frame; returns the pre-tanh output [M, 3] fp32 (CL).  ``frames``: ``h`` holds the hidden states
    of ALL ``frames`` decoder calls of the pass ordered (frame, clip) and ``mods`` the clips' SPADE maps (shared by a clip's frames)."""
    x = res_block(gen.in_block, h, dtype, pit=pit, frames=frames)
    size = 8
    for i, (blk, sp) in enumerate(zip(gen.blocks, gen.spade_blocks)):
        x = res_block(blk, x, dtype, pit=pit, frames=frames)
        size *= 2
        mod = mods[i] if mods is not None else spade_modulation(sp, start_frame, (size, size), dtype)
        x = group_norm(x, sp.groups, dtype, mod=mod)
    return conv_block(gen.out_conv, x, dtype, out_f32=True)


def first_stage_forward_loss(model, X, eps, w_l1=10.0, w_kl=1e-7, power_iteration=None):
    """One differentiable pass of SpadeCondMotionModel + the L1 / KL loss terms.  Returns (loss, X_hat, mu, logvar)."""
    _lib.require_gpu()
    dt = model.dtype
    pit = model.training if power_iteration is None else bool(power_iteration)
    B, T = X.shape[0], X.shape[1]
    X = X.float().contiguous()
    X_in = X if model.full_sequence else X[:, 1:]
    z, mu, lv, dhw = encode(model.enc_motion, X_in.transpose(1, 2), eps)
    Z = model.enc_motion.z_dim
    m = K.CL(pad_cols(z, K.round_up(Z, K.e16(dt)), dt), B, dhw, Z)
    hidden = [m] * model.n_layers
    if model.use_motion_bias:
        mb = model.motion_bias.expand(B, -1, -1, -1).permute(0, 2, 3, 1).reshape(-1, Z)
        in_rnn = K.CL(pad_cols(mb, K.round_up(Z, K.e16(dt)), dt), B, dhw, Z)
    else:
        in_rnn = m
    x0 = X[:, 0].contiguous()
    n_out = B * (T - 1) * 3 * X.shape[-1] * X.shape[-2]
    l1 = 0.0
    frames = []
    begin_forward_pass()
    gate_w = [gru_gate_weights(cell) for cell in model.rnn.cells]
    mods = spade_modulations(model.gen, x0, dt) if _HOIST_SPADE else None
    # all frames as one batch: needs the hoisted SPADE maps and 32-bit row offsets at the widest 128 x 128 layer
    batched = _FRAME_BATCH and mods is not None and T > 2 and B * (T - 1) * X.shape[-1] * X.shape[-2] * 64 < (1 << 31)
    sn_pre = precompute_power_iterations(model.gen, T - 1) if (pit and (_SN_AHEAD or batched)) else []
    hs = []
    native_gru = batched and gru_native_ok(model.rnn, in_rnn, m, dt)
    for t in range(0 if native_gru else T - 1):
        xin = in_rnn
        new_hidden = []
        for cell, gw, h in zip(model.rnn.cells, gate_w, hidden):
            xin = gru_cell(cell, xin, h, dt, gw)
            new_hidden.append(xin)
        hidden = new_hidden
        if batched:
            hs.append(hidden[-1])
            continue
        pre = decode_frame(model.gen, hidden[-1], x0, dt, pit, mods)
        lt, frame = l1_tanh_loss(pre.t, X[:, t + 1], 1.0 / n_out)
        l1 = l1 + lt
        frames.append(frame.view(B, pre.dhw[1], pre.dhw[2], 3).permute(0, 3, 1, 2))
    if batched:
        # the ConvGRU is sequential in time, the decoder is not: ONE pass over the (frame, clip)-ordered batch of all T - 1 frames
        if native_gru:       # the T - 1 steps x n_layers cells issued by the library, one autograd node
            h_all = gru_unroll(model.rnn, in_rnn, m, T - 1, dt, gate_w)
        else:
            h_all = K.CL(torch.cat([h.t for h in hs], 0), B * (T - 1), hs[0].dhw, hs[0].C)
        pre = decode_frame(model.gen, h_all, x0, dt, pit, mods, frames=T - 1)
        tgt = X[:, 1:].transpose(0, 1).reshape(B * (T - 1), *X.shape[2:])           # targets in the same (frame, clip) order (one copy)
        l1, frame = l1_tanh_loss(pre.t, tgt, 1.0 / n_out)
        x_hat = frame.view(T - 1, B, pre.dhw[1], pre.dhw[2], 3).permute(1, 0, 4, 2, 3)
    for m_sn in sn_pre:                               # every decoder convolution consumed exactly its T - 1 iterations
        left = m_sn.__dict__.pop("_sn_pre", [])
        if left:
            raise RuntimeError(f"spectral-norm bookkeeping: {len(left)} precomputed power iterations were not consumed")
    mu4 = mu.view(B, dhw[1], dhw[2], Z).permute(0, 3, 1, 2)
    lv4 = lv.view(B, dhw[1], dhw[2], Z).permute(0, 3, 1, 2)
    kl = kl_loss(mu, lv)                                                             # utils/losses.py:47-48
    loss = w_l1 * l1 + w_kl * kl
    return loss, (x_hat if batched else torch.stack(frames, dim=1)), mu4, lv4


class FirstStageTrainer:
    """Minimal training harness of c4: ``step(X)`` = forward, L1 + KL loss, backward, Adam step (the reference's
    first-stage optimiser is ``Adam(lr, betas=(0.5, 0.9))`` over encoder + GRU + decoder, first_stage_motion_model.py:283-300)."""

    def __init__(self, model, lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5, eps=1e-8, vgg_loss=None, w_vgg=0.0, gamma=0.98):
        """``vgg_loss`` (ipoke_amd.vgg.VGGLoss) with ``w_vgg`` adds the perceptual term of first_stage_motion_model.py:263-271;
        ``gamma``: per-epoch learning-rate decay (first_stage.yaml:45), applied by ``on_epoch_end``."""
        self.model = model
        from . import warn_if_queues_late
        warn_if_queues_late("FirstStageTrainer")
        self.gamma = float(gamma)
        self.vgg_loss, self.w_vgg = vgg_loss, float(w_vgg)
        if self.w_vgg != 0.0 and vgg_loss is None:
            raise ValueError("w_vgg != 0 needs vgg_loss=ipoke_amd.vgg.VGGLoss(...) (load the torchvision VGG-19 weights into it)")
        self.opt = MultiTensorAdam(model.parameters(), lr, betas, weight_decay, eps)
        self.params = self.opt.params
        self.grad_hook = None           # called between backward and the update (data parallel: enable_data_parallel)
        self._dp_flat = None

    def enable_data_parallel(self, n_buckets=4):
        """One process per GPU (experiments/experiment.py:86-89 runs the first stage under DDP): after the backward pass the gradients
        are gathered into ONE persistent flat buffer (a multi-tensor copy), summed over the ranks in ``n_buckets`` large slices
        (``dist.allreduce_flat_``: xGMI is point-to-point, large messages keep every link busy) and handed to the optimizer as views
        of that buffer -- no copy back; the mean's 1 / world is folded into the fused Adam update."""
        from . import dist as D
        world = D.world_size()
        if world == 1:
            return
        sizes = [p.numel() for p in self.params]
        offs, n = [], 0
        for k in sizes:
            offs.append(n)
            n += -(-k // 4) * 4                       # 16-byte aligned views
        self._dp_flat = torch.zeros(n, dtype=torch.float32, device=self.params[0].device)
        views = [self._dp_flat[o:o + k].view(p.shape) for o, k, p in zip(offs, sizes, self.params)]
        self.opt.grad_scale = 1.0 / world

        # spectral-norm buffers: DDP broadcasts module buffers from rank 0 before every forward (broadcast_buffers=True in the reference's
        # Lightning run); the power iteration sees rank-local batches only through the weights, which are equal on every rank, so one
        # broadcast per step keeps sigma identical instead of letting round-off drift it apart
        sn_bufs = [b for k, b in self.model.named_buffers() if k.endswith("weight_u") or k.endswith("weight_v")]
        checked = {"mask": None}

        def sync_grads():
            have, missing = [], []
            for v, p in zip(views, self.params):
                (have if p.grad is not None else missing).append((v, p))
            # a parameter without a gradient on THIS rank still takes part in the sum (another rank may have one): its slot must hold
            # zeros, not the reduced values of the previous step
            for v, _ in missing:
                v.zero_()
            # ... and the set of such parameters must be the SAME on every rank: the optimizer skips a parameter whose .grad is None, so a
            # parameter that is missing here and present elsewhere would be updated there only and the replicas would diverge.  Verified
            # with one small all-reduce whenever the local set changes (normally once).
            mask = tuple(p.grad is None for p in self.params)
            if mask != checked["mask"]:
                cnt = torch.tensor([float(m_) for m_ in mask], dtype=torch.float32, device=self._dp_flat.device)
                D.allreduce_(cnt)
                bad = [i for i, c in enumerate(cnt.tolist()) if c not in (0.0, float(world))]
                if bad:
                    raise RuntimeError(f"data-parallel first stage: {len(bad)} parameter(s) (first index {bad[0]}) have a gradient on some ranks "
                                       "only; every rank must differentiate the same set of parameters")
                checked["mask"] = mask
            if hasattr(torch, "_foreach_copy_"):
                torch._foreach_copy_([v for v, _ in have], [p.grad for _, p in have])
            else:
                for v, p in have:
                    v.copy_(p.grad)
            D.allreduce_flat_(self._dp_flat, n_buckets)
            for v, p in have:
                p.grad = v
            if sn_bufs:          # ONE collective for all power-iteration vectors (two per spectral-norm layer before)
                flat_uv = torch.cat([b.reshape(-1) for b in sn_bufs])
                D.broadcast_(flat_uv, src=0)
                o = 0
                pieces = []
                for b in sn_bufs:
                    pieces.append(flat_uv[o:o + b.numel()].view_as(b)); o += b.numel()
                if hasattr(torch, "_foreach_copy_"):
                    torch._foreach_copy_(sn_bufs, pieces)
                else:
                    for b, q in zip(sn_bufs, pieces):
                        b.copy_(q)
        self.grad_hook = sync_grads


    def on_epoch_end(self):
        """Lightning steps the ExponentialLR scheduler once per epoch (first_stage_motion_model.py:383-388)."""
        self.opt.exponential_lr_step(self.gamma)

    def state_dict(self):
        return {"model": self.model.state_dict(), "opt": self.opt.state_dict()}

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd["model"])
        self.model.invalidate_operands()
        self.opt.load_state_dict(sd["opt"])

    def step(self, X, eps=None):
        m = self.model
        m.train()
        if eps is None:
            Z = m.enc_motion.z_dim
            s = m.enc_motion.min_ssize
            eps = torch.FloatTensor(X.shape[0], Z, s, s).normal_().to(X.device)      # CPU generator, motion_encoder.py:220
        self.opt.zero_grad()
        loss, X_hat, mu, lv = first_stage_forward_loss(m, X, eps)
        if self.w_vgg != 0.0:
            loss = loss + self.w_vgg * self.vgg_loss(X[:, 1:].reshape(-1, *X.shape[2:]).float(), X_hat.reshape(-1, *X_hat.shape[2:]))
        if getattr(self, "_wgrad_stream", None) is None:
            from .utils.streams import overlapping_stream
            self._wgrad_stream = overlapping_stream()
        with wgrad_side_stream(self._wgrad_stream):
            loss.backward()
        if self.grad_hook is not None:
            self.grad_hook()
        snap = take_operand_cache()
        self.opt.step()
        m.invalidate_operands()
        refresh_operand_cache(snap)
        return loss.detach(), X_hat.detach()
