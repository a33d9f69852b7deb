"""``PokeMotionModel``: the second-stage module of iPOKE with the reference's call surface
(models/second_stage_video.py:31-452, 632-662) on the HIP flow engine and the HIP first-stage VAE.

The reference class is a LightningModule whose ``__init__(config, dirs)`` loads three checkpoints from
``logs/...``; Lightning and those files do not exist here, so this is a plain ``nn.Module`` that keeps the
Lightning method names (``training_step``, ``configure_optimizers``, ``on_train_batch_start`` ...) and takes
the three sub-model configurations from ``config['first_stage']``, ``config['poke_embedder']`` and
``config['conditioner_model']`` (dictionaries with the reference's YAML keys).  Checkpoints are loaded with
``load_first_stage / load_poke_embedder / load_conditioner`` which mirror ``__initialize_*`` (:182-236).
``ipoke_amd.trainer.SecondStageTrainer`` is the loop that drives it (the counterpart of pl.Trainer.fit).
"""
import itertools
from functools import partial

import numpy as np
import os

import torch
import torch.nn as nn

from . import _lib, metrics, nn as K
from .data import PokeSimulator
from .first_stage import Conv2dTransposeBlock, FirstStageWrapper, SpadeCondMotionModel
from .flow import SupervisedMacowTransformer
from .fvd import FVD, calculate_FVD
from .loss import FlowLoss
from .optim import FusedAdamAmsgrad
from .utils.streams import overlapping_stream
from .vgg import metric_vgg16


def linear_var(act_it, start_it, end_it, start_val, end_val, clip_min, clip_max):
    """utils/general.py:221-228."""
    act_val = float(end_val - start_val) / (end_it - start_it) * (act_it - start_it) + start_val
    return float(np.clip(act_val, a_min=clip_min, a_max=clip_max))


class _GraphCache(dict):
    """The captured hipGraphs of one device function: a dict with one entry per input shape.  An entry goes "absent" -> "warm" (the first call of a
    shape ran eager, which builds every lazily cached weight operand) -> "ready" (the second call captured; it and every later call copy
    their inputs in and replay).  The graphs hold the ADDRESSES of the cached weight operands, so whatever drops those (a state-dict
    load) clears it (``PokeMotionModel._drop_graphs``).  What differs between the two users -- grad mode and streams of the capture, host draws per call, weight
    refresh before a replay, who owns the outputs -- stays with them (``_flow_input_graphed``, ``_sample_graphed``)."""

    enabled = False

    def set(self, enable):
        self.enabled = bool(enable)
        self.clear()

    def entry(self, *inputs):
        """The entry of the inputs' shapes and dtypes; "absent" on their first call."""
        return self.setdefault(tuple((tuple(x.shape), x.dtype) for x in inputs), {"state": "absent"})

    @staticmethod
    def warmed(ent, **remember):
        """absent -> warm: the caller has run the function eager; ``remember``: what the later calls need from that run."""
        ent.update(state="warm", **remember)

    @staticmethod
    def capture(ent, fn, inputs, device):
        """warm -> ready: capture ``fn`` on static copies of ``inputs`` (on ``device``)."""
        static = [x.to(device, copy=True) for x in inputs]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn(*static)
        ent.update(state="ready", graph=g, static=static, out=out)

    @staticmethod
    def replay(ent, inputs):
        """Copy ``inputs`` into the static buffers and replay.  Returns the graph's STATIC outputs: the next replay overwrites them."""
        for s, x in zip(ent["static"], inputs):
            s.copy_(x, non_blocking=True)
        ent["graph"].replay()
        return ent["out"]


class PokeMotionModel(nn.Module):
    def __init__(self, config, dirs=None, dtype="bf16", device=None, max_batch=None):
        super().__init__()
        self.config = config
        self.dirs = dirs or {}
        self.dtype = dtype
        self.embed_poke = True
        self.test_mode = config["general"].get("test", "none")
        tr = config["training"]
        self.spatial_mean_for_loss = bool(tr.get("spatial_mean", False))
        logdet_weight = config["logdet_weight"] if "logdet_weight" in config else 1.0      # looked up at top level (:41)
        if tr.get("adabelief", False):
            raise NotImplementedError("AdaBelief can never be selected by shipped configs (key mismatch, SURVEY §2 row 4b)")
        self.n_test_samples = config["testing"]["n_samples_per_data_point"]
        self.global_step = 0
        self.current_epoch = 0
        self._optimizer = None
        # state of the test loop (second_stage_video.py:150-180); the metric objects are built on first use
        self.metrics_dict = {"KPS": {}, "LPIPS": {}, "SSIM": {}, "PSNR": {}}
        self.div_scores = []
        self.vggm = None
        self._test_state = None
        # validation: attach_fvd() sets the metric; the clips kept for the epoch's FVD
        self.FVD = None
        self._fvd_fake, self._fvd_true, self._fvd_fake_x0, self._fvd_true_x0 = [], [], [], []
        self._enc_graphs, self._sample_graphs = _GraphCache(), _GraphCache()     # set_encoder_graph / set_sample_graph
        self._prefetched = {}                    # id(batch) -> FIFO of prefetch_flow_input results
        self._decode_stream = None               # sample_stream's second stream, picked on first use
        self._poke_simulator = None
        self.device_ = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")

        lr = tr["lr"]
        self.apply_lr_scaling = bool(tr.get("lr_scaling", False))
        if self.apply_lr_scaling:
            self.lr_scaling = partial(linear_var, start_it=0, end_it=tr["lr_scaling_max_it"], start_val=0.0, end_val=lr,
                                      clip_min=0.0, clip_max=lr)
        self.custom_lr_decrease = tr["custom_lr_decrease"]
        if self.custom_lr_decrease:
            self.lr_adaptation = partial(linear_var, start_it=tr["lr_scaling_max_it"], start_val=lr, end_val=0.0, clip_min=0.0,
                                         clip_max=lr)
            # on_train_epoch_start (:317-323): end_it = n_epochs * num_training_batches (capped at max_batches_per_epoch)
            self._lr_end_it = tr["n_epochs"] * tr.get("max_batches_per_epoch", 2000)

        # frozen first-stage model, poke embedder, conditioner
        self.first_stage_config = config["first_stage"]
        self.first_stage_model = SpadeCondMotionModel(self.first_stage_config, dirs=self.dirs, train=False, dtype=dtype)
        self.full_seq = bool(tr.get("full_seq", False))
        self.use_cond = config["conditioner"].get("use", True)
        self.poke_emb_config = config["poke_embedder"]
        self.poke_embedder = FirstStageWrapper(self.poke_emb_config, dtype=dtype)
        if self.use_cond:
            self.conditioner_config = config["conditioner_model"]
            self.conditioner = FirstStageWrapper(self.conditioner_config, dtype=dtype)
        arch = config["architecture"]
        self.augment_input = bool(arch.get("augmented_input", False))
        arch["flow_in_channels"] = self.first_stage_config["architecture"]["z_dim"]
        if self.augment_input:
            # noise channels appended to the latent (:66-79, :304-308).  The flow input is detached (:348), so the "trainable"
            # scale / shift never receive a gradient in the reference either: they are kept as parameters for the state dict only
            n_aug = int(arch["augment_channels"])
            arch["flow_in_channels"] += n_aug
            if arch.get("scale_augmentation", False):
                self.scale_augment = torch.nn.Parameter(torch.ones(n_aug), requires_grad=False)
            else:
                self.register_buffer("scale_augment", torch.ones(n_aug))
            if arch.get("shift_augmentation", False):
                self.shift_augment = torch.nn.Parameter(torch.zeros(n_aug), requires_grad=False)
            else:
                self.register_buffer("shift_augment", torch.zeros(n_aug))
        pe_arch = self.poke_emb_config["architecture"]
        self.embed_poke_and_image = bool(pe_arch.get("poke_and_image", False))
        self.poke_key = "flow" if pe_arch.get("flow_ae", False) else "poke"
        assert not (self.poke_key == "flow" and self.embed_poke_and_image)
        arch["h_channels"] = pe_arch["nf_max"] + (self.conditioner_config["architecture"]["nf_max"] if self.use_cond else 0)
        arch["flow_mid_channels"] = int(arch["flow_mid_channels_factor"] * arch["flow_in_channels"])
        arch["ssize"] = pe_arch["min_spatial_size"]
        fs_min = self.first_stage_config["architecture"]["min_spatial_size"]
        self.adapt_poke_emb_ssize = pe_arch["min_spatial_size"] != fs_min
        self.adapt_cond_ssize = self.use_cond and self.conditioner_config["architecture"]["min_spatial_size"] != fs_min
        if self.adapt_poke_emb_ssize:
            # second_stage_video.py:114-118 builds a stride-`factor` Conv2d when the poke latent is SMALLER than the first stage's
            # (factor > 1: 4x4 -> 2x2) and a stride-1/factor transposed block when it is LARGER (16x16 -> 32x32): both move the map AWAY
            # from the first-stage size, and the torch.cat of :311 fails in the reference itself.  Nothing to be compatible with.
            raise NotImplementedError("adapt_poke_emb_ssize: the reference's own adapter resizes in the wrong direction for either ratio "
                                      "(second_stage_video.py:114-118) and cannot run; use a poke embedder with the first stage's latent size")
        if self.adapt_cond_ssize:
            factor = float(fs_min) / self.conditioner_config["architecture"]["min_spatial_size"]
            if factor < 1 or factor != int(factor):
                # :123-126: `nn.Conv2d(..., stride=int(factor))` with factor < 1 is a stride-0 convolution ("non-positive stride")
                raise NotImplementedError("adapt_cond_ssize with a conditioner latent larger than the first stage's builds a stride-0 "
                                          "Conv2d in the reference (second_stage_video.py:123-126): no behaviour to reproduce")
            nf = self.conditioner_config["architecture"]["nf_max"]
            # Conv2dTransposeBlock(nf, nf, st=factor, ks=3, padding=1): ConvTranspose2d + ("elu" -> ReLU); trainable in name only --
            # it is applied under torch.no_grad (:268-290) and so never receives a gradient in the reference either
            self.conv_adapt_cond = Conv2dTransposeBlock(nf, nf, 3, int(factor), 1, norm="none", activation="elu", snorm=False)
        if arch.get("multistack", False):
            raise NotImplementedError("multistack flows are outside the shipped configs")
        mb = max_batch if max_batch is not None else max(config["data"]["batch_size"], 1)
        self.first_stage_model.to(self.device_); self.poke_embedder.to(self.device_)
        if self.use_cond:
            self.conditioner.to(self.device_)
        if self.adapt_cond_ssize:
            self.conv_adapt_cond.to(self.device_)
        self.flow = SupervisedMacowTransformer(arch, dtype=dtype, max_batch=mb, device=self.device_)
        self.loss_func = FlowLoss(spatial_mean=self.spatial_mean_for_loss, logdet_weight=logdet_weight)
        self.logged = {}

    # ---- Lightning-compatible no-ops ---------------------------------------------------------------
    def log(self, name, value, **kw):
        self.logged[name] = value

    def log_dict(self, d, **kw):
        self.logged.update(d)

    def optimizers(self):
        return self._optimizer

    # ---- checkpoints (second_stage_video.py:182-236) -----------------------------------------------
    @staticmethod
    def _sd(path_or_sd):
        sd = torch.load(path_or_sd, map_location="cpu") if isinstance(path_or_sd, str) else path_or_sd
        return sd["state_dict"] if "state_dict" in sd else sd

    def load_checkpoint(self, ckpt, strict=False):
        """Counterpart of ``SecondStageVideoModel``'s ``load_from_checkpoint(..., strict=False)`` (experiments/
        second_stage_video.py:22, experiments/experiment.py:107-143): a Lightning ``.ckpt`` (path or loaded dict) whose
        ``state_dict`` holds ``flow.flow.*`` (weight_g / weight_v, int64 shuffle indices, uint8 ``initialized`` flags),
        ``first_stage_model.*`` (spectral-norm ``weight_orig / weight_u / weight_v``), ``poke_embedder.*``, ``conditioner.*``."""
        res = self.load_state_dict(self._sd(ckpt), strict=strict)
        self.flow.sync_buffers()
        self.first_stage_model.enc_motion.conv1.invalidate()
        self._drop_graphs()
        return res

    def load_state_dict(self, *args, **kwargs):
        res = super().load_state_dict(*args, **kwargs)
        self._drop_graphs()
        return res

    def _drop_graphs(self):
        """Captured graphs hold the ADDRESSES of the cached weight operands: a state-dict load drops those caches (``_Cached``), so the
        graphs of ``set_sample_graph`` / ``set_encoder_graph`` are recaptured on their next use."""
        self._sample_graphs.clear()
        self._enc_graphs.clear()

    def load_first_stage(self, ckpt):
        self.first_stage_model.load_state_dict(self._sd(ckpt), strict=False)
        self.first_stage_model.enc_motion.conv1.invalidate()
        self._drop_graphs()

    def load_poke_embedder(self, ckpt):
        sd = self._sd(ckpt)
        sd = {".".join(k.split(".")[1:]): v for k, v in sd.items() if "encoder" in k or "decoder" in k}
        self.poke_embedder.load_state_dict(sd, strict=False)
        self._drop_graphs()

    def load_conditioner(self, ckpt):
        sd = {k: v for k, v in self._sd(ckpt).items() if "encoder" in k or "decoder" in k}
        self.conditioner.load_state_dict(sd, strict=False)
        self._drop_graphs()

    # ---- LR rule (:238-253) ---------------------------------------------------------------------------
    def on_train_epoch_start(self, num_training_batches=None):
        if self.custom_lr_decrease and num_training_batches is not None:
            self._lr_end_it = self.config["training"]["n_epochs"] * num_training_batches

    def on_train_batch_start(self, batch, batch_idx, dataloader_idx=0):
        max_it = self.config["training"]["lr_scaling_max_it"]
        opt = self.optimizers()
        if self.apply_lr_scaling and self.global_step < max_it:
            lr = self.lr_scaling(self.global_step)
            self.log("learning_rate", lr)
            for pg in opt.param_groups:
                pg["lr"] = lr
        if self.custom_lr_decrease and self.global_step >= max_it:
            lr = self.lr_adaptation(self.global_step, end_it=self._lr_end_it)
            for pg in opt.param_groups:
                pg["lr"] = lr

    # ---- hot path ---------------------------------------------------------------------------------------
    def _eval_frozen(self):
        """The frozen models are forced to eval mode before every use (:271-272)."""
        self.first_stage_model.eval(); self.poke_embedder.eval()
        if self.use_cond:
            self.conditioner.eval()

    def _poke_of(self, batch, use_kp_poke=False):
        if use_kp_poke:
            poke, *_ = batch["keypoint_poke"]
            return poke.to(torch.float)
        poke = batch[self.poke_key]
        return poke[0] if isinstance(poke, list) else poke

    def _cond_parts(self, x0, poke, side=None):
        """The conditioning encoders on start frame ``x0`` and ``poke``: (image code or None, poke code), joined by ``_join_cond``.  Two
        steps because the callers differ in what they issue in between (``make_flow_input``: the 3-D encoder).  ``side``: a stream for
        the two encoders; it starts behind the caller's stream here and is joined by the caller."""
        if self.embed_poke_and_image:
            poke = torch.cat([poke, x0], dim=1)
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            poke_emb, *_ = self.poke_embedder.encoder(poke)
            cond = None
            if self.use_cond:
                cond, *_ = self.conditioner.encoder(x0)
                if self.adapt_cond_ssize:
                    cond = self._adapt_cond(cond)
        return cond, poke_emb

    def _join_cond(self, cond, poke_emb):
        return torch.cat([cond, poke_emb], dim=1) if self.use_cond else poke_emb

    def _draw_latent(self, X, pinned=False):
        """The residual of one sample: CPU generator, then moved -- torch.randn(...).type_as(X) (:296-300), one draw per sample.
        ``pinned``: through pinned memory without blocking; a pageable copy makes the host wait for the stream to drain."""
        spatial = self.first_stage_config["architecture"]["min_spatial_size"]
        z = torch.randn((X.size(0), self.config["architecture"]["flow_in_channels"], spatial, spatial), pin_memory=pinned)
        return z.to(device=X.device, dtype=X.dtype, non_blocking=True) if pinned else z.type_as(X)

    def make_flow_input(self, batch, reverse=False, use_kp_poke=False):
        X = batch["images"]
        poke = self._poke_of(batch, use_kp_poke)
        self._eval_frozen()
        with torch.no_grad():
            parts = self._cond_parts(X[:, 0], poke)
            if reverse:
                flow_input = self._draw_latent(X)
            else:
                flow_input, *_ = self.encode_first_stage(X)       # its eps draw: after the 2-D encoders, before the augmentation noise
                if self.augment_input:
                    n_aug = self.config["architecture"]["augment_channels"]
                    noise = torch.randn((flow_input.size(0), n_aug, *flow_input.shape[-2:])).type_as(X)
                    noise = self.scale_augment.to(X.device)[None, :, None, None] * noise + self.shift_augment.to(X.device)[None, :, None, None]
                    flow_input = torch.cat([flow_input, noise], dim=1)
        return flow_input, self._join_cond(*parts)

    def _adapt_cond(self, cond):
        """conv_adapt_cond (second_stage_video.py:120-129, 286-287): the conditioner's 4x4 (...) latent brought to the first stage's size."""
        y = self.conv_adapt_cond.run(K.from_nchw(cond.float(), self.dtype), self.dtype)
        return K.to_nchw(y, self.dtype)

    def _motion_encoder_input(self, X):
        """The frames the 3-D encoder sees, [B, 3, T', H, W]."""
        if self.full_seq:
            X_in = X if self.first_stage_model.full_sequence or self.config["data"]["max_frames"] < 16 else X[:, :-1]
        else:
            X_in = X if self.first_stage_model.full_sequence else X[:, 1:]
        return X_in.transpose(1, 2)

    def encode_first_stage(self, X):
        with torch.no_grad():
            motion, mu, cov = self.first_stage_model.enc_motion(self._motion_encoder_input(X))
        return motion, mu

    def _cut_augmentation(self, motion):
        if self.augment_input:
            motion = motion[:, :-self.config["architecture"]["augment_channels"]].contiguous()
        return motion

    def decode_first_stage(self, motion, X, length=None):
        if length is None:
            length = X.size(1) - 1
        return self.first_stage_model.decode(motion, X[:, 0], length)

    def prefetch_flow_input(self, batch, stream, after=None):
        """Run the frozen encoders for ``batch`` on ``stream`` now; the next ``forward_density(batch)`` (same object) picks the
        result up.  The encoders do not depend on the flow's parameters, so this overlaps with the current step's
        backward pass (what a data-loader worker does for the reference's frozen first stage)."""
        cur = torch.cuda.current_stream()
        # the side stream starts after everything already queued on the caller's stream: the batch may have been produced
        # there (non-blocking H2D copies, GPU-side augmentation), and so are the lazily built weight operands of the first
        # call.  It is issued right after the forward pass, so the overlap with the backward pass is kept.
        # ``after``: an event recorded on the caller's stream behind which the side stream may start (the trainer records
        # it right after the forward pass and calls this once the backward pass is queued, so that the host does not hold
        # the backward chain back by the ~7 ms it takes to queue the encoders)
        if after is not None:
            stream.wait_event(after)
        else:
            stream.wait_stream(cur)
        with torch.cuda.stream(stream):
            if self._enc_graphs.enabled and not self.augment_input:
                flow_input, cond = self._flow_input_graphed(batch)
            else:
                flow_input, cond = self.make_flow_input(batch)
            ev = torch.cuda.Event(); ev.record(stream)
        for v in batch.values():                       # tensors the side stream reads must not be recycled under it
            for t_ in (v if isinstance(v, (list, tuple)) else [v]):
                if torch.is_tensor(t_) and t_.is_cuda:
                    t_.record_stream(stream)
        flow_input.record_stream(cur); cond.record_stream(cur)
        # keyed FIFO: the next batch may be prefetched before this one is consumed (and a loop may feed the same object twice)
        self._prefetched.setdefault(id(batch), []).append((batch, flow_input, cond, ev))

    # ---- the frozen encoders as ONE captured hipGraph -----------------------------------------------------------------------
    def set_encoder_graph(self, enable=True):
        """Replay the device side of ``make_flow_input`` (2-D poke / image encoders + the 3-D motion encoder: ~200 launches that Python
        needs ~4 ms to queue for 3.6 ms of kernels) from one captured hipGraph per input shape when it is PREFETCHED for the next step
        (``prefetch_flow_input``).  The replay is one host call, and inside the graph the two small 2-D encoders run BESIDE the 3-D encoder
        (a second captured stream: no allocator traffic at replay).  MEASURED AND NOT ADOPTED AS DEFAULT (round 4, c2): the hole behind the
        backward pass shrinks from 5.5 to 4.7 ms, but the step is 60.2-61.2 ms against 59.2-59.4 eager -- the forward pass of the next step
        picks up gaps it did not have (IPOKE_ENC_GRAPH=1 turns it on in SecondStageTrainer; bit-identical results either way).  The reparameterisation noise is still drawn on the CPU generator per call, at the same point of the host program as the
        eager path (motion_encoder.py:220), and copied into the graph's input buffer."""
        self._enc_graphs.set(enable)

    @property
    def encoder_graph_enabled(self):
        return self._enc_graphs.enabled

    def _flow_input_device(self, X, poke, eps, side):
        """Device side of ``make_flow_input`` (reverse = False) with the noise given; ``side``: a stream for the 2-D encoders."""
        parts = self._cond_parts(X[:, 0], poke, side=side)
        flow_input, _, _ = self.first_stage_model.enc_motion(self._motion_encoder_input(X), eps=eps)
        torch.cuda.current_stream().wait_stream(side)
        return flow_input, self._join_cond(*parts)

    def _flow_input_graphed(self, batch):
        X, poke = batch["images"], self._poke_of(batch)
        ent = self._enc_graphs.entry(X, poke)
        if ent["state"] == "absent":
            flow_input, cond = self.make_flow_input(batch)
            self._enc_graphs.warmed(ent, eps_shape=tuple(flow_input.shape))
            return flow_input, cond
        self._eval_frozen()
        enc = self.first_stage_model.enc_motion
        eps = None if enc.be_determinstic else torch.FloatTensor(*ent["eps_shape"]).normal_()      # CPU generator, motion_encoder.py:220
        inputs = (X, poke) if eps is None else (X, poke, eps)
        if ent["state"] == "warm":
            ent["side"] = torch.cuda.Stream()            # the captured second stream lives as long as the graph
            with torch.no_grad():
                self._enc_graphs.capture(ent, lambda sX, sP, sE=None: self._flow_input_device(sX, sP, sE, ent["side"]), inputs, X.device)
        # the graph writes into ITS static output buffers: a second replay (a prefetched batch k + 1 while batch k is still queued or in its
        # backward pass) would overwrite them -- hand out copies (two small tensors, ordered behind the replay on this stream)
        return tuple(o.clone() for o in self._enc_graphs.replay(ent, inputs))

    def forward_density(self, batch):
        queue = self._prefetched.get(id(batch))
        pf = queue.pop(0) if queue else None
        if queue is not None and not queue:
            del self._prefetched[id(batch)]
        if pf is not None and pf[0] is batch:
            torch.cuda.current_stream().wait_event(pf[3])
            flow_input, cond = pf[1], pf[2]
        else:
            flow_input, cond = self.make_flow_input(batch)
        out, logdet = self.flow(flow_input.detach(), cond, reverse=False)
        return out, logdet

    # ---- sampling -------------------------------------------------------------------------------------
    def _sample_device(self, X, poke, z):
        """The device side of one sample of ``forward_sample``: conditioning encoders -> reverse flow -> ConvGRU + SPADE decode.  No host
        synchronisation, no host RNG: this is what ``set_sample_graph`` captures."""
        return self.decode_first_stage(self._sample_motion(X, poke, z), X)

    def _sample_motion(self, X, poke, z):
        """First half of ``_sample_device``: conditioning encoders -> reverse flow (the motion latent of the first stage)."""
        cond = self._join_cond(*self._cond_parts(X[:, 0], poke))
        return self._cut_augmentation(self.flow(z, cond, reverse=True))

    def sample_stream(self, batches, n_logged_vids=1, add_first_frame=False, use_keypoint_pokes=False):
        """``forward_sample(batch)[0]`` for every batch of an iterable (the validation / test loops, `second_stage_video.py:490-584`,
        call it batch after batch), two batches in flight: the reverse flow of batch k+1 runs on the caller's stream while the ConvGRU +
        SPADE decode of batch k runs on a second stream.  The reverse flow is a serial chain of small launches (its inverse units occupy one
        workgroup per sample), the decoder is wide convolutions -- they fill different parts of the chip.  Per batch the same kernels run
        on the same data in the same order as in ``forward_sample`` (bit-identical results, tested); the latent is drawn from the CPU
        generator per batch in the same order.  Yields one CPU tensor per batch, in order, up to two batches late."""
        self._eval_frozen()
        if self._decode_stream is None:
            self._decode_stream = overlapping_stream()      # not any new stream: see utils/streams.py
        side = self._decode_stream

        # Schedule.  The decode stream never WAITS on the device for the flow: a stream parked in an event wait slows the other queue's
        # dispatch (utils/streams.py: a chain of small launches runs 1.9x slower beside a waiting stream, 3-15x on an unlucky one).
        # Instead the host queues the reverse flow of batch k+1 first and only then waits for the flow of batch k to finish -- it has
        # been running while k+1 was queued -- before it queues the decode of k on the second stream.
        @torch.no_grad()                     # per stage, not around the yields: a generator must not hold the caller's grad mode
        def issue_flow(batch):
            X = batch["images"]
            poke = self._poke_of(batch, use_keypoint_pokes)
            # same CPU generator draw as forward_sample, but through pinned memory: a pageable copy would make the host wait for the
            # stream to drain and give up its lead over the device
            motion = self._sample_motion(X, poke, self._draw_latent(X, pinned=True))
            flow_done = torch.cuda.Event(); flow_done.record()
            return X, motion, flow_done

        @torch.no_grad()
        def issue_decode(item):
            X, motion, flow_done = item
            flow_done.synchronize()                      # host-side: nothing waits on the device
            for t_ in (motion, X):
                t_.record_stream(side)
            with torch.cuda.stream(side):
                video = self.decode_first_stage(motion, X)
                if add_first_frame:
                    video = torch.cat([X[:, 0].unsqueeze(1), video], dim=1)
                video = video[:n_logged_vids]
                # the copy to the host is queued right behind this batch's decode
                host = torch.empty(video.shape, dtype=video.dtype, pin_memory=True)
                host.copy_(video, non_blocking=True)
                done = torch.cuda.Event(); done.record(side)
                return host, done

        def fetch(item):
            item[1].synchronize()
            return item[0].clone()            # out of the pinned staging buffer, like ``.cpu()``

        flowing, decoding = None, None       # batch whose reverse flow is queued / batch whose decode is queued
        for batch in itertools.chain(batches, [None]):       # None: nothing more to queue, the pipeline drains
            nxt = issue_flow(batch) if batch is not None else None
            if flowing is not None:
                out = issue_decode(flowing)
                if decoding is not None:
                    yield fetch(decoding)
                decoding = out
            flowing = nxt
        if decoding is not None:
            yield fetch(decoding)

    def set_sample_graph(self, enable=True):
        """BASELINE configs[4] ("flow inverse + VAE decode, hipGraph-captured"): replay the whole device side of ``forward_sample`` --
        the two conditioning encoders, the ~3 000-launch reverse flow, the 15-step ConvGRU and the frame-batched SPADE decoder
        (models/second_stage_video.py:326-382) -- as ONE captured hipGraph per input shape.  The latent is still drawn on the CPU
        generator per call, like the reference (:296-300), and copied into the graph's input buffer; results are bit-identical to the
        eager path (tests/test_bench_configs_gpu.py)."""
        self._sample_graphs.set(enable)

    def _sample_graphed(self, X, poke, z):
        ent = self._sample_graphs.entry(X, poke)
        if ent["state"] == "absent":
            self._sample_graphs.warmed(ent)
            return self._sample_device(X, poke, z)
        if ent["state"] == "warm":
            self._sample_graphs.capture(ent, self._sample_device, (X, poke, z), X.device)
        if self.flow.engine.shadow_stale:            # a replay skips the eager path's refresh of the flow's weight operands (same addresses)
            self.flow.engine.prepare_weights()
        return self._sample_graphs.replay(ent, (X, poke, z))            # the static buffer itself: consumed before the next replay

    def _sample_video(self, X, poke, z):
        if self._sample_graphs.enabled:
            return self._sample_graphed(X, poke, z)
        return self._sample_device(X, poke, z)

    def _sample_videos(self, X, pokes, add_first_frame=False):
        """The sampling loop: one device video [B, T (+ 1), 3, H, W] per poke of ``pokes``, each from a fresh latent.  The conditioning is
        recomputed per sample, as the reference's make_flow_input(batch, reverse=True) does (:333).  With the sample graph on, a yielded
        video is the graph's static buffer: use or copy it before asking for the next.  Runs in the consumer's grad mode (no_grad)."""
        for poke in pokes:
            video = self._sample_video(X, poke, self._draw_latent(X))
            if add_first_frame:
                video = torch.cat([X[:, 0].unsqueeze(1), video], dim=1)
            yield video

    @staticmethod
    def _stack_samples(videos, n):
        """``n`` videos [B', ...] from ``_sample_videos`` as one device buffer [B', n, ...]."""
        out = None
        for i, video in enumerate(videos):
            if out is None:
                out = torch.empty((video.shape[0], n) + tuple(video.shape[1:]), dtype=video.dtype, device=video.device)
            out[:, i].copy_(video)                 # (a graph replay hands out its static buffer: copied before the next replay)
        return out

    def forward_sample(self, batch, n_samples=1, n_logged_vids=1, show_progress=False, add_first_frame=False,
                       use_keypoint_pokes=False):
        self._eval_frozen()
        with torch.no_grad():
            pokes = [self._poke_of(batch, use_keypoint_pokes)] * n_samples
            return [video[:n_logged_vids].cpu() for video in self._sample_videos(batch["images"], pokes, add_first_frame)]

    def training_step(self, batch, batch_idx):
        out, logdet = self.forward_density(batch)
        loss, loss_dict = self.loss_func(out, logdet)
        self.log_dict(loss_dict)
        self.log("global_step", self.global_step)
        if self._optimizer is not None:
            self.log("learning_rate", self._optimizer.param_groups[0]["lr"])
        return loss

    # ---- validation loop (second_stage_video.py:490-584) --------------------------------------------------
    def attach_fvd(self, i3d=None, dtype="f32"):
        """The reference builds ``self.FVD = FVD(n_samples=...)`` with the Kinetics I3D weights in __init__ (:66); here the metric
        is attached explicitly (the I3D checkpoint is not part of the second-stage checkpoint)."""
        self.FVD = FVD(n_samples=self.config["logging"]["n_fvd_samples"], i3d=i3d, dtype=dtype)
        self._fvd_fake, self._fvd_true, self._fvd_fake_x0, self._fvd_true_x0 = [], [], [], []
        return self.FVD

    def validation_step(self, batch, batch_id):
        """NLL terms of the batch, and (for the first n_fvd_samples clips) one sampled video per clip kept for the FVD of the
        epoch; generated and true clips stay on the device.  ssim-val / psnr-val (:511-512) are computed on the device
        (ipoke_amd/metrics.py); lpips-val (:513) needs the lpips package's pretrained network and is not part of this path."""
        with torch.no_grad():
            out, logdet = self.forward_density(batch)
            loss, loss_dict = self.loss_func(out, logdet)
        self.log_dict({"val/" + key: loss_dict[key] for key in loss_dict})
        X = batch["images"]
        # second_stage_video.py:498-513: the sampled clips and ssim / psnr of every batch below the FVD sample budget, whether or not an
        # I3D is attached; only the clip lists kept for the epoch's FVD need the FVD object
        if batch_id <= int(self.config["logging"]["n_fvd_samples"] / X.size(0)):
            X_hat = self.forward_sample(batch, n_logged_vids=X.size(0))[0].to(X.device)
            if self.FVD is not None:
                self._fvd_fake.append(X_hat)
                self._fvd_true.append(X[:, 1:])
                self._fvd_fake_x0.append(torch.cat([X[:, 0].unsqueeze(1), X_hat], dim=1))
                self._fvd_true_x0.append(X)
            X_hat_log = X_hat.reshape(-1, *X_hat.shape[2:]).type_as(X)
            X_log = X[:, 1:].reshape(-1, *X_hat.shape[2:])
            both = metrics.psnr_ssim(X_hat_log, X_log)
            self.log("ssim-val", both[1])
            self.log("psnr-val", both[0])
        self.log("d_ref_nll-val", torch.abs(loss_dict["reference_nll_loss"] - loss_dict["nll_loss"]))
        self.log("loss-val", loss)
        return {"loss": loss, "batch_idx": batch_id, "loss_dict": loss_dict}

    def validation_epoch_end(self, outputs=None):
        bs = self.first_stage_config["logging"]["bs_i3d"]
        fvd_score = calculate_FVD(self.FVD.i3d, torch.cat(self._fvd_fake), torch.cat(self._fvd_true), batch_size=bs)
        self.log("FVD-val", fvd_score)
        fvd_x0 = calculate_FVD(self.FVD.i3d, torch.cat(self._fvd_fake_x0), torch.cat(self._fvd_true_x0), batch_size=bs)
        self.log("FVD-val-x0", fvd_x0)
        for lst in (self._fvd_fake, self._fvd_true, self._fvd_fake_x0, self._fvd_true_x0):
            lst.clear()
        return fvd_score, fvd_x0

    # ---- test loop (second_stage_video.py:665-752, 1037-1155) ------------------------------------------------
    _TEST_MODES_MISSING = {
        "samples": "the sample grids are written with the cv2 video writer (utils/logging.py save_video), which is not part of this package",
        "kps_acc": "the targeted keypoint error needs the HRNet pose estimator (utils/posenet_wrapper.py) and its checkpoint",
        "control_sensitivity": "the control-sensitivity study needs the HRNet pose estimator and the cv2 video writer; its pokes and samples, "
                               "without the files, come from control_sensitivity_samples()",
        "transfer": "the transfer grids are written with the cv2 video writer (utils/logging.py save_video); the transferred and sampled "
                    "videos, without the files, come from transfer_motion()",
    }

    def sample_videos_device(self, batch, n_samples=1, n_logged_vids=1, add_first_frame=False, use_keypoint_pokes=False):
        """``torch.stack(forward_sample(...), dim=1)`` without the ``.cpu()`` round trip: fp32 [B', n_samples, T, 3, H, W] on the device.
        The latents are drawn from the CPU generator in the reference's order, one ``torch.randn`` per sample, so a seeded call equals
        ``forward_sample`` bit for bit (the same kernels on the same data; tested)."""
        # no CPU path -- and "a GPU is visible" (require_gpu) is not enough: a model built with device="cpu" would hand the kernels
        # host addresses, which is an illegal memory access on the device, reported at some later call
        if self.device_.type != "cuda":
            raise RuntimeError(f"ipoke_amd has no CPU path: the model must be on the GPU (it was built on {self.device_})")
        self._eval_frozen()
        with torch.no_grad():
            pokes = [self._poke_of(batch, use_keypoint_pokes)] * n_samples
            videos = self._sample_videos(batch["images"], pokes, add_first_frame)
            return self._stack_samples((video[:n_logged_vids] for video in videos), n_samples)

    # ---- applications (second_stage_video.py:786-852, 948-1015): the tensors; writing mp4 / png files is left to the caller ------------
    def poke_simulator(self):
        """The ``PokeSimulator`` of ``config['data']`` (the reference reads ``poke_size`` from its test data set, :794, :951)."""
        if self._poke_simulator is None:
            self._poke_simulator = PokeSimulator(self.config["data"])
        return self._poke_simulator

    def transfer_motion(self, batch):
        """Motion transfer, ``_test_transfer`` (second_stage_video.py:948-1015) up to the video writer: the residual r1 of clip 1 (``batch``)
        under its own conditioning, replayed under the conditioning of clip 2 -- ``batch['nn'] = (X_2, flow_2, sample_ids2)`` -- whose
        start frame takes the place of clip 1's while the poke stays clip 1's: cond_2 = conditioner(X_2[:, 0]) (through ``_adapt_cond`` when
        configured) ++ poke_embedder(poke1 ++ X_2[:, 0]).  Returns device tensors: ``r1``, ``z_r1_cond2`` (r1 reversed under cond_2),
        ``z_random_cond2`` (a fresh residual reversed under cond_2), ``vid_r1_c2`` and ``vid_random_cond2`` (both decoded on X_2[:, 0]).

        Not computed, although the reference does: ``poke_2`` / ``poke_emb_2`` (:959-966, 980: clip 2's flow re-read at clip 1's centres,
        ``PokeSimulator.stamp(centers, flow=flow_2)`` here), which never reach ``cond_2``, and ``r2`` (:1004), which only commented-out code
        uses.  The random residual is ``torch.randn(r1.shape).type_as(r1)`` from the CPU generator, drawn after the forward pass -- the
        convention of ``forward_sample``; the reference's ``randn_like`` on the device is not reproducible across devices.  With
        ``augmented_input`` the noise channels are cut off before decoding, as in sampling."""
        _lib.require_gpu()
        if not self.embed_poke_and_image:
            # :975-981: poke1_src2 is only assigned under `if self.embed_poke_and_image` and read unconditionally
            raise NotImplementedError("transfer_motion without poke_and_image: the reference's own _test_transfer fails with a NameError "
                                      "(poke1_src2 is only defined when the poke embedder takes the poke AND the image, "
                                      "second_stage_video.py:975-981): no behaviour to reproduce")
        self.eval()
        with torch.no_grad():
            X_2 = batch["nn"][0]
            poke1 = self._poke_of(batch)
            z_1, cond_1 = self.make_flow_input(batch)
            cond_2 = self._join_cond(*self._cond_parts(X_2[:, 0], poke1))
            r1, _ = self.flow(z_1, cond_1, reverse=False)
            z_r1_cond2 = self.flow(r1, cond_2, reverse=True)
            residual_sample = torch.randn(r1.shape).type_as(r1)
            z_random_cond2 = self.flow(residual_sample, cond_2, reverse=True)
            vid_r1_c2 = self.decode_first_stage(self._cut_augmentation(z_r1_cond2), X_2)
            vid_random_cond2 = self.decode_first_stage(self._cut_augmentation(z_random_cond2), X_2)
        return {"r1": r1, "z_r1_cond2": z_r1_cond2, "z_random_cond2": z_random_cond2, "vid_r1_c2": vid_r1_c2,
                "vid_random_cond2": vid_random_cond2}

    def control_sensitivity_samples(self, batch, n_pokes=None, u=None):
        """The control-sensitivity study, ``_control_sensitivity`` (second_stage_video.py:786-852) up to the video writer: the batch's start
        frames sampled under the batch's own poke (slot 0) and under ``n`` pokes at each sample's first centre that are re-aimed at a random
        angle of the upper half plane, with the magnitude the flow has at a randomly chosen pixel above its mean amplitude
        (``PokeSimulator.randomize_pokes``).  n defaults to ``testing.n_control_sensitivity_pokes``; u: fp32 [B, n, 2] uniforms, drawn on the
        device when not given.  Returns ``(pokes [n + 1, B, 2, H, W], samples [B, n + 1, T, 3, H, W], picked int64 [B, n, 2], status)`` on the
        device; sample k is ``forward_sample`` of the batch with ``batch['poke'] = pokes[k]``.  Draw order: the uniforms, then one latent
        per poke (CPU generator).  ``batch`` is not modified (the reference overwrites ``batch['poke']``); samples without a candidate pixel
        raise ``FlowError`` before anything is sampled."""
        _lib.require_gpu()
        n = int(self.config["testing"]["n_control_sensitivity_pokes"] if n_pokes is None else n_pokes)
        self.eval()
        with torch.no_grad():
            X = batch["images"]
            poke0, centers = batch["poke"]
            randomized, picked, status = self.poke_simulator().randomize_pokes(batch["flow"], centers, n, u=u, strict=True)
            pokes = torch.cat([poke0.float()[None], randomized])
            per_sample = (self._poke_of({**batch, "poke": pokes[k]}) for k in range(n + 1))
            samples = self._stack_samples(self._sample_videos(X, per_sample), n + 1)
        return pokes, samples, picked, status

    def attach_metric_vgg(self, vgg=None, dtype="f32"):
        """The reference builds ``self.vggm = metric_vgg16()`` with torchvision's ImageNet weights (:155); here the extractor is attached
        explicitly (``ipoke_amd.vgg.metric_vgg16`` + ``load_torchvision_features``)."""
        self.vggm = (metric_vgg16(dtype=dtype) if vgg is None else vgg).to(self.device_)
        return self.vggm

    def _test(self):
        if self._test_state is None:
            self._test_state = {"real_u8": [], "fake_u8": [], "real": [], "fake": [], "ssim": metrics.SSIM_custom(), "psnr": metrics.PSNR_custom(),
                                "sample_ssim": metrics.SampleSSIM(self.n_test_samples)}
        return self._test_state

    def _test_batch_size(self, X):
        return self.config["testing"].get("test_batch_size", X.size(0))

    def _test_step_fvd(self, batch, batch_id):
        """:665-678 -- one sample per clip; uint8 [B, T, H, W, 3] real and generated-with-x0 clips (converted on the device)."""
        st = self._test()
        X = batch["images"]
        sample = self.sample_videos_device(batch, 1, n_logged_vids=X.size(0))[:, 0]
        gen = torch.cat([X[:, 0].unsqueeze(1), sample.type_as(X)], dim=1)
        st["real_u8"].append(metrics.video_to_uint8(X))
        st["fake_u8"].append(metrics.video_to_uint8(gen))
        if self.FVD is not None:
            st["real"].append(X); st["fake"].append(gen)

    def _test_step_metrics(self, batch, batch_id):
        """:681-743 without the keypoint and LPIPS terms."""
        if "keypoints_rel" in batch and "keypoints_abs" in batch:
            raise NotImplementedError("test mode 'accuracy' with keypoints in the batch: the keypoint term needs the HRNet pose estimator "
                                      "(utils/posenet_wrapper.py) and its checkpoint; drop 'keypoints_rel' / 'keypoints_abs' from the data keys")
        if self.config["testing"].get("lpips", False):
            raise NotImplementedError("testing.lpips: the LPIPS term needs the lpips package's pretrained network, which is not available")
        st = self._test()
        imgs = batch["images"]
        samples = self.sample_videos_device(batch, self.n_test_samples, n_logged_vids=self._test_batch_size(imgs), add_first_frame=True)
        target_vid = imgs[:samples.shape[0], 1:].unsqueeze(1)
        target_act = target_vid.reshape(-1, *target_vid.shape[3:])
        for n_sample in range(samples.shape[1]):
            samples_act = samples[:, n_sample, 1:].reshape(-1, *samples.shape[3:]).type_as(target_vid)
            both = metrics.psnr_ssim(samples_act, target_act)
            st["ssim"].update_value(both[1]); st["psnr"].update_value(both[0])
        st["sample_ssim"].update(samples[:, :, 1:], target_vid)

    def _test_step_diversity(self, batch, batch_id):
        """:746-752 -- the samples stay on the device."""
        if self.config["testing"].get("div_kp", False):
            raise NotImplementedError("testing.div_kp: the keypoint diversity score needs the HRNet pose estimator (utils/posenet_wrapper.py)")
        if self.config["testing"].get("lpips", False):
            raise NotImplementedError("testing.lpips: the LPIPS diversity term needs the lpips package's pretrained network, which is not available")
        return self.sample_videos_device(batch, self.n_test_samples, n_logged_vids=self._test_batch_size(batch["images"]))

    def _n_pokes(self):
        return self.config["testing"].get("n_pokes", self.config.get("data", {}).get("n_pokes", 1))

    def _test_end_fvd(self, st, outputs):
        savedir = os.path.join(self.dirs["generated"], "samples_fvd")
        os.makedirs(savedir, exist_ok=True)
        # np.stack over the per-batch arrays, as :1071-1072: [n_batches, B, T, H, W, 3] (the mp4 examples of :1075-1084 are not written)
        real_samples = torch.stack(st["real_u8"], dim=0).cpu().numpy()
        fake_samples = torch.stack(st["fake_u8"], dim=0).cpu().numpy()
        np.save(os.path.join(savedir, "real_samples.npy"), real_samples)
        np.save(os.path.join(savedir, "fake_samples.npy"), fake_samples)
        score = None
        if self.FVD is not None:
            score = calculate_FVD(self.FVD.i3d, torch.cat(st["fake"]), torch.cat(st["real"]), batch_size=self.first_stage_config["logging"]["bs_i3d"])
            self.log("FVD-test-x0", score)
        for k in ("real_u8", "fake_u8", "real", "fake"):
            st[k].clear()
        return score

    def _test_end_metrics(self, st, outputs):
        n_pokes = self._n_pokes()
        ssim_normal = st["ssim"].compute().cpu().numpy()
        self.metrics_dict["SSIM"] = ssim_normal
        self.metrics_dict["PSNR"] = st["psnr"].compute().cpu().numpy()
        ssim_nn, ssim_dict = st["sample_ssim"].compute(n_pokes=n_pokes)
        self.metrics_dict["SSIM NN"] = ssim_dict
        self.log("ssim-test", ssim_normal); self.log("ssim-nn-test", ssim_nn)
        st["sample_ssim"].reset(); st["ssim"].reset(); st["psnr"].reset()
        return ssim_normal

    def _test_end_diversity(self, st, outputs):
        if self.vggm is None:
            raise RuntimeError("test mode 'diversity' needs the VGG-16 feature extractor: call attach_metric_vgg() first")
        n_pokes = self._n_pokes()
        exmpls = torch.cat(outputs, dim=0)
        div_score = metrics.compute_div_score(exmpls, self.vggm, device=self.device_)
        div_score_mse = metrics.compute_div_score_mse(exmpls, device=self.device_)
        self.div_scores.append(div_score)
        savepath = os.path.join(self.dirs["generated"], "diversity")
        metrics_dir = os.path.join(self.dirs["generated"], "metrics")
        os.makedirs(savepath, exist_ok=True); os.makedirs(metrics_dir, exist_ok=True)
        # the reference's line (:1145); its third term needs the lpips package and is reported as not computed
        text = f"Similarity measure_vgg: {div_score}; similarity measure mse: {div_score_mse}; similarity measure lpips: {None}\n"
        np.save(os.path.join(savepath, f"samples_diversity_{n_pokes}_pokes.npy"), exmpls.cpu().numpy())
        with open(os.path.join(metrics_dir, "divscore.txt"), "a+") as f:
            f.writelines(text)
        return div_score

    # test mode -> (test_step, test_epoch_end)
    _TEST_MODES = {"fvd": (_test_step_fvd, _test_end_fvd), "accuracy": (_test_step_metrics, _test_end_metrics),
                   "diversity": (_test_step_diversity, _test_end_diversity)}

    def _test_mode_fns(self):
        if self.test_mode in self._TEST_MODES_MISSING:
            raise NotImplementedError(f"test mode '{self.test_mode}': {self._TEST_MODES_MISSING[self.test_mode]}")
        if self.test_mode not in self._TEST_MODES:
            raise ValueError(f'The specified test_mode is "{self.test_mode}", which is invalid...')
        return self._TEST_MODES[self.test_mode]

    def test_step(self, batch, batch_id):
        self.eval()
        with torch.no_grad():
            return self._test_mode_fns()[0](self, batch, batch_id)

    def test_step_end(self, out_step):
        return out_step

    def test_epoch_end(self, outputs=None):
        st = self._test()
        return self._test_mode_fns()[1](self, st, outputs)

    def configure_optimizers(self):
        tr = self.config["training"]
        self._optimizer = FusedAdamAmsgrad(self.flow, lr=tr["lr"], betas=(0.9, 0.999), weight_decay=tr["weight_decay"], amsgrad=True)
        if not self.custom_lr_decrease:
            raise NotImplementedError("the shipped configs use custom_lr_decrease=True (no scheduler object)")
        return [self._optimizer]
