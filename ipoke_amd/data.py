"""Batched, on-device counterparts of the reference data set's flow / poke preparation (data/base_dataset.py).

``PokeSimulator`` carries the attributes ``BaseDataset.__init__`` derives from the data config (:40-78, :185-186: spatial_size,
poke_size, n_pokes, fix_n_pokes, equal_poke_val, scale_poke_to_res) and offers

    get_flow(raw)                 _get_flow (:651-693)   raw flows [B, 2, Hs, Ws] -> [B, 2, H, W] (scaled to the resolution, bilinear)
    get_poke(flow, zero, u)       _get_poke (:507-648)   -> (poke [B, 2, H, W], poke_centers int64 [B, n_pokes, 2], flow_out, status)
    stamp(centers, values | flow) squares of given values, or of the flow at the centres, on a zero poke (models/second_stage_video.py
                                  :959-966, testing/gui.py:120-150)
    randomize_pokes(flow, centers, n)  the re-aimed pokes of the control-sensitivity study (models/second_stage_video.py:798-833)

so that a loader only has to deliver raw flows and frames; everything downstream of the file read happens in HBM.  The random
draws are uniforms supplied by the caller (or drawn here from a torch generator): see ``ipoke_poke_simulate`` in
include/ipoke_hip.h for how they map to the reference's ``np.random.randint`` calls.  No CPU path.
"""
import torch

from . import _lib
from ._lib import check, ptr


class FlowError(RuntimeError):
    """No poke candidate in a sample (the reference raises FlowError and draws another sample, base_dataset.py:588-589)."""


class PokeSimulator:
    def __init__(self, config):
        self.config = config
        assert "spatial_size" in config
        self.spatial_size = tuple(config["spatial_size"])
        self.n_pokes = int(config["n_pokes"])
        self.fix_n_pokes = bool(config.get("fix_n_pokes", False)) or self.n_pokes == 1
        self.scale_poke_to_res = bool(config.get("scale_poke_to_res", False))
        self.poke_size = config["poke_size"] if "poke_size" in config else self.spatial_size[0] / 128 * 10
        if int(self.poke_size) != self.poke_size:
            raise ValueError("poke_size must be integral (the reference slices tensors with it)")
        self.poke_size = int(self.poke_size)
        self.equal_poke_val = bool(config.get("equal_poke_val", True))
        self.valid_h = [self.poke_size, self.spatial_size[0] - self.poke_size]
        self.valid_w = [self.poke_size, self.spatial_size[1] - self.poke_size]

    def get_flow(self, raw):
        _lib.require_gpu()
        raw = raw.contiguous().float()
        B, C, Hs, Ws = raw.shape
        H, W = self.spatial_size
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=raw.device)
        div = Hs / H if self.scale_poke_to_res else 1.0
        check(_lib.lib().ipoke_flow_resize(ptr(raw), ptr(out), B, C, Hs, Ws, H, W, div, _lib.current_stream()))
        return out

    def get_poke(self, flow, zero_poke=None, u=None, generator=None, strict=True):
        """flow fp32 [B, 2, H, W] on the device; zero_poke: bool/int [B] (samples with seq_len_idx == -1) or None;
        u: fp32 [B, 1 + 2 n_pokes] uniforms in [0, 1) or None (drawn on the device from ``generator``)."""
        _lib.require_gpu()
        flow = flow.contiguous().float()
        B, C, H, W = flow.shape
        assert C == 2 and (H, W) == self.spatial_size
        dev = flow.device
        if u is None:
            u = torch.rand(B, 1 + 2 * self.n_pokes, device=dev, generator=generator)
        u = u.to(dev, torch.float32).contiguous()
        assert u.shape == (B, 1 + 2 * self.n_pokes)
        zero = None if zero_poke is None else zero_poke.to(dev).to(torch.int32).contiguous()
        poke = torch.empty_like(flow)
        flow_out = torch.empty_like(flow)
        centers = torch.empty(B, self.n_pokes, 2, dtype=torch.int64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.lib().ipoke_poke_workspace_bytes(B, H, W, self.poke_size, self.n_pokes), dtype=torch.uint8, device=dev)
        check(_lib.lib().ipoke_poke_simulate(ptr(flow), B, H, W, self.poke_size, self.n_pokes, int(self.fix_n_pokes), int(self.equal_poke_val),
                                             ptr(zero), ptr(u), ptr(poke), ptr(centers), ptr(flow_out), ptr(status), ptr(ws), _lib.current_stream()))
        if strict and bool(status.any()):
            raise FlowError(f"Empty indices array for samples {status.nonzero().flatten().tolist()}")
        return poke, centers, flow_out, status

    def stamp(self, centers, values=None, flow=None, skip_negative=True):
        """A poke [B, 2, H, W] from its centres: zeros with ``p[:, r-half:r+half+1, c-half:c+half+1] = v`` applied for poke 0, 1, ... in that
        order under Python's slice rules (half = poke_size // 2; see ``ipoke_poke_stamp`` in include/ipoke_hip.h).  centers: int64 [B, n, 2]
        as (row, col); the values are ``values`` fp32 [B, n, 2] (user arrows) or ``flow`` [B, 2, H, W] read at each centre (the poke of one
        clip re-read from another clip's flow).  ``skip_negative`` leaves out the -1 padding rows of ``poke_centers``."""
        _lib.require_gpu()
        if (values is None) == (flow is None):
            raise ValueError("stamp takes either values or flow")
        centers = centers.to(torch.int64).contiguous()
        B, n, two = centers.shape
        assert two == 2
        dev = centers.device
        H, W = self.spatial_size
        if values is not None:
            values = values.to(dev, torch.float32).contiguous()
            assert values.shape == (B, n, 2)
        else:
            flow = flow.to(dev, torch.float32).contiguous()
            assert flow.shape == (B, 2, H, W)
        if n == 0:                                # nothing to draw (and no address to hand over)
            return torch.zeros(B, 2, H, W, dtype=torch.float32, device=dev)
        poke = torch.empty(B, 2, H, W, dtype=torch.float32, device=dev)
        check(_lib.lib().ipoke_poke_stamp(ptr(centers), ptr(values), ptr(flow), B, H, W, n, int(self.poke_size // 2), int(bool(skip_negative)),
                                          ptr(poke), _lib.current_stream()))
        return poke

    def randomize_pokes(self, flow, centers, n, u=None, generator=None, strict=True):
        """``n`` re-aimed pokes per sample at the sample's first centre, of the magnitude the flow has at a randomly chosen moving pixel
        (``ipoke_poke_randomize``): -> (pokes [n, B, 2, H, W], picked int64 [B, n, 2], status int32 [B]).  u: fp32 [B, n, 2] uniforms in
        [0, 1) -- [..., 0] chooses the pixel, [..., 1] the angle -- or None (drawn on the device from ``generator``)."""
        _lib.require_gpu()
        flow = flow.contiguous().float()
        B, C, H, W = flow.shape
        assert C == 2 and (H, W) == self.spatial_size
        dev = flow.device
        centers = centers.to(dev, torch.int64).contiguous()
        assert centers.dim() == 3 and centers.shape[0] == B and centers.shape[1] >= 1 and centers.shape[2] == 2
        n = int(n)
        if u is None:
            u = torch.rand(B, n, 2, device=dev, generator=generator)
        u = u.to(dev, torch.float32).contiguous()
        assert u.shape == (B, n, 2)
        pokes = torch.empty(n, B, 2, H, W, dtype=torch.float32, device=dev)
        picked = torch.empty(B, n, 2, dtype=torch.int64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.lib().ipoke_poke_randomize_workspace_bytes(B, H, W, n), dtype=torch.uint8, device=dev)
        check(_lib.lib().ipoke_poke_randomize(ptr(flow), ptr(centers), ptr(u), B, H, W, centers.shape[1], n, int(self.poke_size // 2), ptr(pokes),
                                              ptr(picked), ptr(status), ptr(ws), _lib.current_stream()))
        if strict and bool(status.any()):
            bad = status.nonzero().flatten().tolist()
            raise FlowError(f"No pixel above the mean flow amplitude, or a padded first poke centre, for samples {bad} "
                            f"(status {status[bad].tolist()})")
        return pokes, picked, status

    def make_batch(self, images, raw_flow, zero_poke=None, u=None, generator=None):
        """The ``batch`` dict the second stage consumes (images, flow, poke = [poke, poke_centers]) from frames already on the device
        and raw flows: the part of BaseDataset.__getitem__ that follows the file reads."""
        flow = self.get_flow(raw_flow)
        # no host synchronisation on the loader path: samples without a candidate (the reference's FlowError) are flagged in
        # ``poke_status`` (int32 [B], 1 = resample), for the caller to inspect when it chooses to
        poke, centers, flow_out, status = self.get_poke(flow, zero_poke, u, generator, strict=False)
        return {"images": images, "flow": flow_out, "poke": [poke, centers], "poke_status": status}
