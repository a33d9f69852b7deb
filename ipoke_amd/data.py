"""Batched, on-device counterparts of the reference data set's flow / poke preparation (data/base_dataset.py).

``PokeSimulator`` carries the attributes ``BaseDataset.__init__`` derives from the data config (:40-78, :185-186: spatial_size,
poke_size, n_pokes, fix_n_pokes, equal_poke_val, scale_poke_to_res) and offers

    get_flow(raw)                 _get_flow (:651-693)   raw flows [B, 2, Hs, Ws] -> [B, 2, H, W] (scaled to the resolution, bilinear)
    get_poke(flow, zero, u)       _get_poke (:507-648)   -> (poke [B, 2, H, W], poke_centers int64 [B, n_pokes, 2], flow_out, status);
                                  with mask= the filter_flow branches (:520-538, :577-583)
    flow_mask(flow)               _compute_mask_with_flow (:343-351)   -> (mask bool [B, H, W], status)
    stamp(centers, values | flow) squares of given values, or of the flow at the centres, on a zero poke (models/second_stage_video.py
                                  :959-966, testing/gui.py:120-150)
    randomize_pokes(flow, centers, n)  the re-aimed pokes of the control-sensitivity study (models/second_stage_video.py:798-833)
    draw_keypoint_ids / keypoint_poke  _get_keypoint_poke (:462-497): the poke stamped from the displacement of chosen keypoints

``posture_nearest_neighbours`` is get_nn of data/flow_dataset.py (:628-713), the ``nn_ids`` table a loader stores once per data set;

and ``ClipAugmenter`` the augmentation the shipped training configs switch on (_get_color_transforms / _get_geometric_transforms,
:695-722: colour jitter on the frames, one reflect-padded affine warp for frames and flow), so that a loader only has to deliver raw flows
and uint8 frames; everything downstream of the file read happens in HBM.  The random
draws are uniforms supplied by the caller (or drawn here from a torch generator): see ``ipoke_poke_simulate`` in
include/ipoke_hip.h for how they map to the reference's ``np.random.randint`` calls.  No CPU path.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr


class FlowError(RuntimeError):
    """No poke candidate in a sample (the reference raises FlowError and draws another sample, base_dataset.py:588-589)."""


class AugmentParams:
    """One sample's colour and geometry parameters per entry, as ``ClipAugmenter.draw`` / ``params`` build them.  Host arrays [B]:
    ``brightness``, ``contrast``, ``saturation`` (the factors), ``hue`` (the hue value), ``angle`` (degrees), ``tx``, ``ty`` (pixels).
    Device tensors, the arguments of the kernels (include/ipoke_hip.h): ``colour`` fp32 [B, 3], ``hue_add`` int32 [B], ``affine`` int32 [B, 6]
    and ``mean_l`` int32 [B, T], which ``images`` fills for the clip it is given (None before)."""

    def __init__(self, size, brightness, contrast, saturation, hue, angle, tx, ty, device):
        self.size = int(size)
        self.brightness, self.contrast, self.saturation, self.hue, self.angle = (
            np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (brightness, contrast, saturation, hue, angle))
        self.tx, self.ty = (np.atleast_1d(np.asarray(v, dtype=np.int64)) for v in (tx, ty))
        B = len(self.brightness)
        if any(len(v) != B for v in (self.contrast, self.saturation, self.hue, self.angle, self.tx, self.ty)):
            raise ValueError("one value per sample for every parameter")
        if ((self.hue < -0.5) | (self.hue > 0.5)).any():
            raise ValueError(f"hue_factor is not in [-0.5, 0.5]: {self.hue.tolist()}")           # torchvision's adjust_hue
        colour = np.stack([self.brightness, self.contrast, self.saturation], 1).astype(np.float32)
        hue_add = np.array([int(h * 255) % 256 for h in self.hue], dtype=np.int32)               # np.uint8(hue_factor * 255): truncate, wrap
        affine = np.array([fixed_point_affine(a, x, y, self.size) for a, x, y in zip(self.angle, self.tx, self.ty)], dtype=np.int64)
        if (np.abs(affine) >= 2 ** 31).any():
            raise ValueError("the translation does not fit Pillow's 16.16 fixed point")
        self.colour = torch.from_numpy(colour).to(device)
        self.hue_add = torch.from_numpy(hue_add).to(device)
        self.affine = torch.from_numpy(affine.astype(np.int32)).to(device)
        self.mean_l = None

    def __len__(self):
        return len(self.brightness)


def fixed_point_affine(angle, tx, ty, size):
    """The inverse matrix FT.affine(angle, (tx, ty), 1.0, 0) computes, in double, for the reflect-padded 2 size x 2 size image (centre
    (size, size)), as the six 16.16 fixed-point integers Pillow's nearest-neighbour transform steps through."""
    a = math.radians(float(angle))
    m = [math.cos(a), math.sin(a), 0.0, -math.sin(a), math.cos(a), 0.0]
    cx = cy = float(size)
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty) + cx
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty) + cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def augment_images(frames_u8, params):
    """uint8 frames [B, T, S, S, 3] (or [B, S, S, 3]) -> fp32 [B, T, 3, S, S] (or [B, 3, S, S]) in [-1, 1]: the colour chain and the warp of
    ``params`` in one gather (``ipoke_aug_frame_means`` + ``ipoke_aug_frames``).  Current stream, no host synchronisation."""
    _lib.require_gpu()
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (4, 5):
        raise ValueError("frames_u8 must be uint8 [B, T, S, S, 3] or [B, S, S, 3]")
    single = frames_u8.dim() == 4
    frames = (frames_u8.unsqueeze(1) if single else frames_u8).contiguous()
    B, T, S, S2, C = frames.shape
    if (S, S2, C) != (params.size, params.size, 3) or B != len(params):
        raise ValueError(f"frames {tuple(frames_u8.shape)} do not match {len(params)} parameter sets at size {params.size}")
    dev = frames.device
    colour, hue_add, affine = params.colour.to(dev), params.hue_add.to(dev), params.affine.to(dev)
    mean_l = torch.empty(B, T, dtype=torch.int32, device=dev)
    out = torch.empty(B, T, 3, S, S, dtype=torch.float32, device=dev)
    stream = _lib.current_stream()
    check(_lib.lib().ipoke_aug_frame_means(ptr(frames), ptr(colour), B, T, S, ptr(mean_l), stream))
    check(_lib.lib().ipoke_aug_frames(ptr(frames), ptr(colour), ptr(hue_add), ptr(mean_l), ptr(affine), B, T, S, ptr(out), stream))
    params.mean_l = mean_l
    return out[:, 0] if single else out


def augment_flow(flow, params):
    """flow fp32 [B, C, S, S] under the warp of ``params`` (``ipoke_aug_flow``): values are copied, not rotated, as in the reference
    (:683-691).  Current stream, no host synchronisation."""
    _lib.require_gpu()
    flow = flow.contiguous().float()
    if flow.dim() != 4 or flow.shape[2:] != (params.size, params.size) or flow.shape[0] != len(params):
        raise ValueError(f"flow {tuple(flow.shape)} does not match {len(params)} parameter sets at size {params.size}")
    B, C, S, _ = flow.shape
    out = torch.empty_like(flow)
    check(_lib.lib().ipoke_aug_flow(ptr(flow), ptr(params.affine.to(flow.device)), B, C, S, ptr(out), _lib.current_stream()))
    return out


def posture_nearest_neighbours(keypoints, vid, ids=None, return_dist=False):
    """get_nn of the reference (data/flow_dataset.py:628-713, ``measure`` :635-646) for all queries in one launch pair
    (``ipoke_posture_nn``): for every query frame the nearest frame in posture space, D(i, j) = sum_k ||kps[i, k] - kps[j, k]||, once over
    all frames and once over the frames of other videos.

    keypoints: numpy array or tensor [N, K, 2], float32 or float64 (``datadict['keypoints_rel']``), converted to fp32; 1 <= K <= 64.
    vid: [N], any integer or string array (``datadict['vid']``), mapped to dense int32 codes on the host.  ids: the query frames [M], or
    None for all N.  Returns ``(nn_general, nn_other_vid)`` as int64 numpy arrays [M] -- ``nn_other_vid`` is what the reference's get_nn
    returns and its loader stores as ``nn_ids`` -- and with ``return_dist`` also the fp32 distances of the two answers [M, 2].

    Candidates are ordered by (D, j), a stable argsort (the reference's default argsort leaves ties open): ``nn_general`` is the second
    entry of that order, the query itself included, as ``sorted_ids[1]`` is.  Raises ValueError naming the first query for which no frame
    of another video exists, where the reference dies with an IndexError."""
    _lib.require_gpu()
    kp = keypoints.detach().cpu().numpy() if isinstance(keypoints, torch.Tensor) else np.asarray(keypoints)
    if kp.ndim != 3 or kp.shape[2] != 2 or kp.dtype not in (np.float32, np.float64):
        raise ValueError(f"keypoints must be float32 or float64 [N, K, 2], got {kp.dtype} {kp.shape}")
    N, K = kp.shape[:2]
    if N < 2 or not 1 <= K <= 64:
        raise ValueError(f"posture_nearest_neighbours needs N >= 2 frames and 1 <= K <= 64 keypoints, got N = {N}, K = {K}")
    if not np.isfinite(kp).all():
        raise ValueError("keypoints hold non-finite values")
    v = vid.detach().cpu().numpy() if isinstance(vid, torch.Tensor) else np.asarray(vid)
    if v.shape != (N,) or v.dtype.kind not in "iuUSO":
        raise ValueError(f"vid must be an integer or string array [{N}], got {v.dtype} {v.shape}")
    codes = np.unique(v, return_inverse=True)[1].reshape(N).astype(np.int32)
    if ids is None:
        q = None
        M = N
    else:
        q = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        if q.ndim != 1 or q.dtype.kind not in "iu" or q.size == 0:
            raise ValueError(f"ids must be a non-empty integer array [M], got {q.dtype} {q.shape}")
        q = q.astype(np.int64)
        bad = np.flatnonzero((q < 0) | (q >= N))
        if bad.size:
            raise ValueError(f"ids[{int(bad[0])}] = {int(q[bad[0]])} is outside [0, {N})")
        M = q.shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    kp_d = torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float32)).to(dev)
    vid_d = torch.from_numpy(codes).to(dev)
    ids_d = None if q is None else torch.from_numpy(q).to(dev)
    nn_general = torch.empty(M, dtype=torch.int64, device=dev)
    nn_other = torch.empty(M, dtype=torch.int64, device=dev)
    dist = torch.empty(M, 2, dtype=torch.float32, device=dev) if return_dist else None
    ws = torch.empty(max(int(L.ipoke_posture_nn_workspace_bytes(N, K, M)), 64), dtype=torch.uint8, device=dev)
    check(L.ipoke_posture_nn(ptr(kp_d), ptr(vid_d), ptr(ids_d), N, K, M, ptr(nn_general), ptr(nn_other), ptr(dist), ptr(ws), _lib.current_stream()))
    nn_general, nn_other = nn_general.cpu().numpy(), nn_other.cpu().numpy()
    lone = np.flatnonzero(nn_other < 0)
    if lone.size:
        m = int(lone[0])
        frame = m if q is None else int(q[m])
        raise ValueError(f"query {m} (frame {frame}, video {v[frame].item()!r}): no frame of another video exists")
    return (nn_general, nn_other, dist.cpu().numpy()) if return_dist else (nn_general, nn_other)


class ClipAugmenter:
    """The training augmentation of the reference data set (data/base_dataset.py:695-722) on the device, bit-equal to the per-frame PIL chain
    (:432-440 for the frames, :683-691 for the flow): brightness, contrast, hue and saturation jitter, then pad(size / 2, reflect) ->
    affine(angle, translate) -> center_crop(size), nearest neighbour.  One parameter set per sample, shared by all frames of its clip and
    by its flow (:204-206).  ``config`` is the ``data`` section (:86-93): augment, p_col, p_geom, augment_b/c/h/s, aug_deg, aug_trans,
    spatial_size.

    Out of scope: ``fancy_aug`` (use_fb_aug, :425-442), which blends a second colour draw in through the foreground mask into an
    ``img_aT`` entry no model here consumes -- the mask itself is on the device now (``PokeSimulator.flow_mask`` / ``get_poke(mask=)``),
    the blend is not; the warp of a caller's mask, which ``make_batch`` takes in the augmented frame; cv2.grabCut (_compute_mask,
    :327-341), the loader's; and ``_get_flip_transform`` (:724-729), which nothing calls."""

    def __init__(self, config):
        self.config = config
        self.spatial_size = tuple(int(v) for v in config["spatial_size"])
        if self.spatial_size[0] != self.spatial_size[1]:
            raise ValueError(f"spatial_size {self.spatial_size} is not square (the reference's own reshape at :690 assumes it)")
        self.size = self.spatial_size[0]
        self.augment = bool(config.get("augment", False))
        self.p_col, self.p_geom = float(config.get("p_col", 0)), float(config.get("p_geom", 0))
        self.ab, self.ac = float(config.get("augment_b", 0)), float(config.get("augment_c", 0))
        self.ah, self.a_s = float(config.get("augment_h", 0)), float(config.get("augment_s", 0))
        self.ad = float(config.get("aug_deg", 0))
        self.at = tuple(config.get("aug_trans", (0, 0)))

    def draw(self, B, rng, device=None):
        """Parameters for ``B`` samples from ``rng``, a ``numpy.random.RandomState``: per sample the calls of _get_color_transforms
        (:698-702) and then of _get_geometric_transforms (:714-717), in that order and with those arguments, so that an ``rng`` seeded like
        ``np.random`` yields the reference's values."""
        if not self.augment:
            raise ValueError("augment is off in this config: the reference then applies no transform at all (make_batch(augment=None))")
        S0, S1 = self.spatial_size
        rows = []
        for _ in range(int(B)):
            make = bool(rng.choice(np.arange(2), size=1, p=[1 - self.p_col, self.p_col])[0])
            brightness = float(rng.uniform(-self.ab, self.ab, 1)[0]) if self.ab > 0. and make else 0.
            contrast = float(rng.uniform(-self.ac, self.ac, 1)[0]) if self.ac > 0. and make else 0.
            hue = float(rng.uniform(-self.ah, 2 * self.ah, 1)[0]) if self.ah > 0. and make else 0.
            saturation = 1. + (float(rng.uniform(-self.a_s, self.a_s)) if self.a_s > 0. and make else 0)
            make = bool(rng.choice(np.arange(2), size=1, p=[1 - self.p_geom, self.p_geom])[0])
            angle = float(rng.uniform(-self.ad, self.ad, 1)[0]) if self.ad > 0. and make else 0.
            vert = int(rng.randint(int(-self.at[0] * S1 / 2), int(self.at[0] * S1 / 2), 1)[0]) if self.at[0] > 0 and make else 0
            hor = int(rng.randint(int(-self.at[1] * S0 / 2), int(self.at[1] * S0 / 2), 1)[0]) if self.at[1] > 0 and make else 0
            rows.append((1. + brightness, 1. + contrast, saturation, hue, angle, hor, vert))          # translate=(tval_hor, tval_vert)
        return self.params(*zip(*rows), device=device)

    def params(self, brightness, contrast, saturation, hue, angle, tx, ty, device=None):
        """The parameter object from explicit per-sample values: the three factors, the hue value in [-0.5, 0.5], the angle in degrees and
        the translation in pixels (tx to the right, ty down)."""
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        return AugmentParams(self.size, brightness, contrast, saturation, hue, angle, tx, ty, device)

    def images(self, frames_u8, params):
        self._check(params)
        return augment_images(frames_u8, params)

    def flow(self, flow, params):
        self._check(params)
        return augment_flow(flow, params)

    def _check(self, params):
        if params.size != self.size:
            raise ValueError(f"parameters built for size {params.size}, augmenter for {self.size}")


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
        # the mask path of _get_poke (:520-538) and its flow-derived source (:353-359); off in BaseDataset (:67, :188)
        self.filter_flow = bool(config.get("filter_flow", False))
        self.use_flow_for_weights = bool(config.get("use_flow_for_weights", False))
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

    def get_poke(self, flow, zero_poke=None, u=None, generator=None, strict=True, mask=None):
        """flow fp32 [B, 2, H, W] on the device; zero_poke: bool/int [B] (samples with seq_len_idx == -1) or None;
        u: fp32 [B, 1 + 2 n_pokes] uniforms in [0, 1) or None (drawn on the device from ``generator``).

        mask: bool or uint8 [B, H, W] on the device, nonzero = foreground -- the reference's ``self.mask["img_start"]`` under
        ``filter_flow`` (data/base_dataset.py:520-538, :577-583; on by default for Iper and Taichi, data/flow_dataset.py:357, 375).
        Ordinary samples then take their candidates from the amplitude inside the mask, zero-poke samples their centres from the
        mask's background (``ipoke_poke_simulate_masked`` in include/ipoke_hip.h).  None is the unmasked call, unchanged."""
        _lib.require_gpu()
        flow = flow.contiguous().float()
        B, C, H, W = flow.shape
        assert C == 2 and (H, W) == self.spatial_size
        dev = flow.device
        if mask is not None:
            if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (B, H, W):
                raise ValueError(f"mask must be bool or uint8 [{B}, {H}, {W}], got {mask.dtype} {tuple(mask.shape)}")
            mask = mask.to(dev).to(torch.uint8).contiguous()
        if u is None:
            u = torch.rand(B, 1 + 2 * self.n_pokes, device=dev, generator=generator)
        u = u.to(dev, torch.float32).contiguous()
        assert u.shape == (B, 1 + 2 * self.n_pokes)
        zero = None if zero_poke is None else zero_poke.to(dev).to(torch.int32).contiguous()
        poke = torch.empty_like(flow)
        flow_out = torch.empty_like(flow)
        centers = torch.empty(B, self.n_pokes, 2, dtype=torch.int64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        if mask is None:
            ws = torch.empty(_lib.lib().ipoke_poke_workspace_bytes(B, H, W, self.poke_size, self.n_pokes), dtype=torch.uint8, device=dev)
            check(_lib.lib().ipoke_poke_simulate(ptr(flow), B, H, W, self.poke_size, self.n_pokes, int(self.fix_n_pokes), int(self.equal_poke_val),
                                                 ptr(zero), ptr(u), ptr(poke), ptr(centers), ptr(flow_out), ptr(status), ptr(ws),
                                                 _lib.current_stream()))
        else:
            ws = torch.empty(_lib.lib().ipoke_poke_masked_workspace_bytes(B, H, W, self.poke_size, self.n_pokes), dtype=torch.uint8, device=dev)
            check(_lib.lib().ipoke_poke_simulate_masked(ptr(flow), B, H, W, self.poke_size, self.n_pokes, int(self.fix_n_pokes),
                                                        int(self.equal_poke_val), ptr(zero), ptr(u), ptr(mask), ptr(poke), ptr(centers),
                                                        ptr(flow_out), ptr(status), ptr(ws), _lib.current_stream()))
        if strict and bool(status.any()):
            raise FlowError(f"Empty indices array for samples {status.nonzero().flatten().tolist()}")
        return poke, centers, flow_out, status

    def flow_mask(self, flow):
        """The foreground mask the reference derives from the flow itself (_compute_mask_with_flow, data/base_dataset.py:343-351, the
        source ``use_flow_for_weights`` selects in _get_mask :353-362): over the whole map, the amplitude shifted to min 0 and scaled to
        max 1, thresholded at mean + std (``ipoke_flow_mask``).  flow fp32 [B, 2, H, W] on the device -> (mask bool [B, H, W], status
        int32 [B]: 1 for a constant map, whose mask is empty).  Current stream, no host synchronisation."""
        _lib.require_gpu()
        flow = flow.contiguous().float()
        B, C, H, W = flow.shape
        assert C == 2 and (H, W) == self.spatial_size
        dev = flow.device
        mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.lib().ipoke_flow_mask_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        check(_lib.lib().ipoke_flow_mask(ptr(flow), B, H, W, ptr(mask), ptr(status), ptr(ws), _lib.current_stream()))
        return mask.view(torch.bool), status

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

    def draw_keypoint_ids(self, B, K, rng):
        """The keypoints _get_keypoint_poke pokes (data/base_dataset.py:470-473) for ``B`` samples of ``K`` keypoints from ``rng``, a
        ``numpy.random.RandomState``: per sample the reference's calls in its order -- ``randint(1, n_pokes, 1)`` unless fix_n_pokes,
        then ``choice(K, n, replace=False)`` -- so that an ``rng`` seeded like ``np.random`` yields its ids.  int32 [B, n_pokes], -1 padded."""
        out = np.full((int(B), self.n_pokes), -1, dtype=np.int32)
        for b in range(int(B)):
            n = self.n_pokes if self.fix_n_pokes else int(rng.randint(1, self.n_pokes, 1)[0])
            out[b, :n] = rng.choice(int(K), n, replace=False)
        return out

    def keypoint_poke(self, kp_src, kp_tgt, poke_ids, device=None):
        """_get_keypoint_poke (data/base_dataset.py:462-497) for a batch (``ipoke_keypoint_poke``): kp_src, kp_tgt [B, K, 2] as relative
        (x, y) -- ``keypoints_rel`` of the clip's first and last frame --, numpy arrays or tensors, taken as float64 (the reference
        truncates double products); poke_ids int [B, n_pokes], -1 padded (``draw_keypoint_ids``).  Returns the reference's triple
        ``[poke fp32 [B, 2, H, W], poke_coords int32 [B, n_pokes, 2] as (row, col), poke_ids int32 [B, n_pokes]]`` on the device.  Both
        channels of a poke are (tgt - src) * spatial_size[0], the reference's own asymmetry.  Current stream."""
        _lib.require_gpu()
        dev = torch.device(device if device is not None else (kp_src.device if isinstance(kp_src, torch.Tensor) and kp_src.is_cuda else "cuda"))
        src = torch.as_tensor(kp_src).to(dev, torch.float64).contiguous()
        tgt = torch.as_tensor(kp_tgt).to(dev, torch.float64).contiguous()
        if src.dim() != 3 or src.shape[2] != 2 or tgt.shape != src.shape:
            raise ValueError(f"kp_src and kp_tgt must both be [B, K, 2], got {tuple(src.shape)} and {tuple(tgt.shape)}")
        B, K, _ = src.shape
        ids_host = poke_ids.detach().cpu().numpy() if isinstance(poke_ids, torch.Tensor) else np.asarray(poke_ids)
        if ids_host.ndim != 2 or ids_host.shape[0] != B or ids_host.shape[1] < 1 or ids_host.dtype.kind not in "iu":
            raise ValueError(f"poke_ids must be an integer array [{B}, n], got {ids_host.dtype} {ids_host.shape}")
        if (ids_host >= K).any():
            raise ValueError(f"poke_ids name a keypoint outside [0, {K})")
        ids = torch.from_numpy(np.where(ids_host < 0, -1, ids_host).astype(np.int32)).to(dev)
        n_max = ids.shape[1]
        H, W = self.spatial_size
        poke = torch.empty(B, 2, H, W, dtype=torch.float32, device=dev)
        coords = torch.empty(B, n_max, 2, dtype=torch.int32, device=dev)
        check(_lib.lib().ipoke_keypoint_poke(ptr(src), ptr(tgt), ptr(ids), B, K, n_max, H, W, int(self.poke_size / 2), int(self.valid_h[0]),
                                             int(self.valid_h[1]), int(self.valid_w[0]), int(self.valid_w[1]), ptr(poke), ptr(coords),
                                             _lib.current_stream()))
        return [poke, coords, ids]

    def make_batch(self, images, raw_flow, zero_poke=None, u=None, generator=None, augment=None, frames_u8=None, mask=None, keypoints=None,
                   keypoint_ids=None, rng=None):
        """The ``batch`` dict the second stage consumes (images, flow, poke = [poke, poke_centers]) from frames already on the device
        and raw flows: the part of BaseDataset.__getitem__ that follows the file reads.  With ``augment`` (the parameters of
        ``ClipAugmenter.draw`` / ``params``) the order is the reference's: _get_flow -> the warp -> _get_poke, so the pokes are taken from
        the warped flow, and ``images`` comes from the uint8 clip ``frames_u8`` [B, T, S, S, 3] through the colour chain and the same warp.

        ``mask`` is the foreground mask of ``filter_flow`` (see ``get_poke``).  ``"flow"`` computes it with ``flow_mask`` from the
        sample's flow after the warp and before the zero-poke zeroing, the flow _get_mask sees (:353-359: _compute_mask_with_flow
        calls _get_flow with ids whose last entry is not -1).  A tensor (bool / uint8 [B, H, W]) is used as given: the caller supplies
        it in the augmented frame, no warp is applied to it.  With None the config decides: ``filter_flow`` with
        ``use_flow_for_weights`` is ``"flow"``; ``filter_flow`` alone raises, since the reference's other source is cv2.grabCut on the
        start frame (_compute_mask, :327-341), which stays with the caller's loader.  Where a mask is in play the batch gains ``"mask"`` (bool [B, H, W]); without one it is the
        dict it was.

        ``keypoints=(kp_src, kp_tgt)`` adds ``batch["keypoint_poke"]``, the triple of ``keypoint_poke`` (what ``use_keypoint_pokes``
        reads): ``keypoint_ids`` are the chosen keypoints [B, n_pokes], or None to draw them with ``draw_keypoint_ids`` from ``rng`` (a
        ``numpy.random.RandomState``; None: a fresh one).  The keypoints are taken as given: the reference applies no warp to them
        either.  Without the argument the dict is exactly what it was."""
        if mask is None and self.filter_flow:
            if not self.use_flow_for_weights:
                raise ValueError("filter_flow is on: pass mask= (the reference's grabCut mask of the start frame, base_dataset.py:327-341, is "
                                 "the caller's job), or mask='flow' / use_flow_for_weights for the flow-derived one")
            mask = "flow"
        flow = self.get_flow(raw_flow)
        if augment is not None:
            if frames_u8 is None:
                raise ValueError("make_batch(augment=...) builds the images from frames_u8")
            if self.spatial_size != (augment.size, augment.size):
                raise ValueError(f"parameters built for size {augment.size}, simulator for {self.spatial_size}")
            flow = augment_flow(flow, augment)
            images = augment_images(frames_u8, augment)
        # no host synchronisation on the loader path: samples without a candidate (the reference's FlowError) are flagged in
        # ``poke_status`` (int32 [B], 1 = resample), for the caller to inspect when it chooses to
        if isinstance(mask, str):
            if mask != "flow":
                raise ValueError(f"mask={mask!r}: 'flow', a tensor or None")
            mask, _ = self.flow_mask(flow)                 # a constant map has an empty mask and no poke candidate: poke_status flags it
        poke, centers, flow_out, status = self.get_poke(flow, zero_poke, u, generator, strict=False, mask=mask)
        batch = {"images": images, "flow": flow_out, "poke": [poke, centers], "poke_status": status}
        if mask is not None:
            batch["mask"] = mask.to(flow.device).bool()
        if keypoints is not None:
            kp_src, kp_tgt = keypoints
            if keypoint_ids is None:
                keypoint_ids = self.draw_keypoint_ids(len(kp_src), np.shape(kp_src)[1], rng if rng is not None else np.random.RandomState())
            batch["keypoint_poke"] = self.keypoint_poke(kp_src, kp_tgt, keypoint_ids, device=flow.device)
        elif keypoint_ids is not None:
            raise ValueError("keypoint_ids without keypoints=(kp_src, kp_tgt)")
        return batch
