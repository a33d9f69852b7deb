"""Image metrics of the validation logging (reference utils/metrics.py:450-481, second_stage_video.py:511-512): ``SSIM_custom`` and
``PSNR_custom`` -- running means over validation batches of pytorch_lightning.metrics.functional.ssim / psnr (library defaults) -- on
the device: one pass for the ranges and the squared error, one separable-Gaussian pass for the SSIM map (csrc/eval.hip).

The reductions of the test loop (reference utils/metrics.py:60-124, 149-257; second_stage_video.py:665-752) follow below: the per-frame
SSIM of n samples against one broadcast target, the best-of-n statistics (``SampleSSIM``), the pairwise MSE and VGG time-cosine diversity
scores, the best-of-n keypoint error (``KPSMetric``, metrics.py:259-331) and the uint8 video export.  Each is one short launch sequence over the whole batch with a single host read at the very end."""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

_ws = {}


def psnr_ssim(preds, target):
    """(psnr, ssim) of two [N, C, H, W] tensors as a device tensor of two floats (no host synchronisation)."""
    _lib.require_gpu()
    if preds.shape != target.shape or preds.dim() != 4:
        raise ValueError(f"expected two [N, C, H, W] tensors of one shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    p, t = preds.float().contiguous(), target.float().contiguous()
    N, C, H, W = p.shape
    need = _lib.lib().ipoke_image_metrics_workspace_bytes(N * C, H, W)
    key = (p.device, torch.cuda.current_stream().cuda_stream)
    ws = _ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _ws[key] = torch.empty(need, dtype=torch.uint8, device=p.device)
    out = torch.empty(2, dtype=torch.float32, device=p.device)
    check(_lib.lib().ipoke_psnr_ssim(ptr(p), ptr(t), N * C, H, W, ptr(ws), ptr(out), _lib.current_stream()))
    return out


def psnr(preds, target):
    return psnr_ssim(preds, target)[0]


def ssim(preds, target):
    return psnr_ssim(preds, target)[1]


class _RunningMean:
    """metrics.py:450-481: ``update`` adds one batch value, ``compute`` returns the mean over the batches seen."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.acc, self.total = None, 0

    def update_value(self, v):
        self.acc = v if self.acc is None else self.acc + v
        self.total += 1

    def compute(self):
        return self.acc / self.total

    def __call__(self, preds, target):
        v = self.update(preds, target)
        return v


class SSIM_custom(_RunningMean):
    def update(self, preds, targets):
        v = ssim(preds, targets)
        self.update_value(v)
        return v


class PSNR_custom(_RunningMean):
    def update(self, preds, targets):
        v = psnr(preds, targets)
        self.update_value(v)
        return v


# ------------------------------------------------------------------------------------------------ test loop (csrc/eval.hip)
def _workspace(nbytes, device):
    key = (device, torch.cuda.current_stream().cuda_stream, "eval")
    ws = _ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _ws[key] = torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device=device)
    return ws


def sample_ssim(pred, target):
    """pred [bs, ns, s, C, H, W], target [bs, 1, s, C, H, W] -> fp32 [bs, ns, s]: per-frame mean of the SSIM map, data range per example
    (``SampleMetric.update`` with ``ssim(reduction='none')`` and ``.mean(dim=[1, 2, 3])``, metrics.py:169-189).  The target is not replicated."""
    _lib.require_gpu()
    if pred.dim() != 6 or target.dim() != 6 or target.shape[1] != 1 or tuple(pred.shape[2:]) != tuple(target.shape[2:]) or pred.shape[0] != target.shape[0]:
        raise ValueError(f"expected pred [bs, ns, s, C, H, W] and target [bs, 1, s, C, H, W], got {tuple(pred.shape)} and {tuple(target.shape)}")
    p, t = pred.float().contiguous(), target.float().contiguous()
    bs, ns, s, C, H, W = p.shape
    L = _lib.lib()
    ws = _workspace(L.ipoke_sample_ssim_workspace_bytes(bs, ns, s, C, H, W), p.device)
    out = torch.empty(bs, ns, s, dtype=torch.float32, device=p.device)
    check(L.ipoke_sample_ssim(ptr(p), ptr(t), bs, ns, s, C, H, W, ptr(ws), ptr(out), _lib.current_stream()))
    return out


def sample_stats(vals):
    """vals [bs, ns, s] -> (values of the arg-min-mean sample [bs, s], unbiased std over samples [bs, s], mean over samples [bs, s],
    chosen index [bs] int32) (metrics.py:193-204)."""
    _lib.require_gpu()
    v = vals.float().contiguous()
    bs, ns, s = v.shape
    nn, sd, mean = (torch.empty(bs, s, dtype=torch.float32, device=v.device) for _ in range(3))
    idx = torch.empty(bs, dtype=torch.int32, device=v.device)
    check(_lib.lib().ipoke_sample_stats(ptr(v), bs, ns, s, ptr(nn), ptr(sd), ptr(mean), ptr(idx), _lib.current_stream()))
    return nn, sd, mean, idx


class SampleSSIM:
    """``SampleSSIM`` / ``SampleMetric`` of the reference (metrics.py:149-217, 246-257) on the device kernels.  ``n_samples`` is
    ``testing.n_samples_per_data_point``; the reference's guard ``if self.n_samples < self.n_max_samples`` compares the number of processed
    EXAMPLES with it, so updates silently stop after that many examples -- kept as it is."""
    metric_name = "SSIM"

    def __init__(self, n_samples):
        self.n_max_samples = n_samples
        self.reset()

    def reset(self):
        self.nn_val_per_frame, self.std_per_frame, self.mean_per_frame = [], [], []
        self.n_samples = 0
        self.val = None

    def update(self, pred, target):
        if self.n_samples < self.n_max_samples:
            nn, sd, mean, _ = sample_stats(sample_ssim(pred, target))
            self.nn_val_per_frame.append(nn)
            self.std_per_frame.append(sd)
            self.mean_per_frame.append(mean)
            self.n_samples += pred.size(0)
            v = nn.mean(1).sum()
            self.val = v if self.val is None else self.val + v

    def compute(self, n_pokes=None):
        meanval = self.val.float().cpu() / self.n_samples
        name = self.metric_name
        data = {f"{name} NN": torch.cat(self.nn_val_per_frame, dim=0).mean(0).cpu().numpy(),
                f"Mean {name} per Frame": torch.cat(self.mean_per_frame, dim=0).mean(0).cpu().numpy(),
                "Std per Frame": torch.cat(self.std_per_frame, dim=0).mean(0).cpu().numpy()}
        data["Time"] = np.arange(data[f"{name} NN"].shape[0])
        if n_pokes is not None:
            data["Number of Pokes"] = np.full_like(data[f"{name} NN"], n_pokes, dtype=int)
        return meanval, data


def kps_frame_mse(pred, target):
    """pred [bs, ns, s, K, 2], target [bs, 1, s, K, 2] -> fp32 [bs, ns, s]: the per-frame mean over the K * 2 coordinates of the squared
    keypoint error (``KPSMetric.update``, metrics.py:294 and :299).  The target is not replicated."""
    _lib.require_gpu()
    if (pred.dim() != 5 or target.dim() != 5 or target.shape[1] != 1 or pred.shape[4] != 2 or tuple(pred.shape[2:]) != tuple(target.shape[2:])
            or pred.shape[0] != target.shape[0]):
        raise ValueError(f"expected pred [bs, ns, s, K, 2] and target [bs, 1, s, K, 2], got {tuple(pred.shape)} and {tuple(target.shape)}")
    p = pred.float().contiguous()
    t = target.to(p.device).float().contiguous()
    bs, ns, s, K, _ = p.shape
    out = torch.empty(bs, ns, s, dtype=torch.float32, device=p.device)
    check(_lib.lib().ipoke_kps_frame_mse(ptr(p), ptr(t), bs, ns, s, K, ptr(out), _lib.current_stream()))
    return out


class KPSMetric:
    """``KPSMetric`` of the reference (metrics.py:259-331) on the device kernels: the best-of-n keypoint error per frame, the counterpart of
    ``SampleSSIM``.  ``update`` takes the keypoints of the caller's own pose estimator, predicted [bs, ns, s, K, 2] and ground truth
    [bs, 1, s, K, 2]; it keeps the reference's state (nn_err_per_frame, std_per_frame, mean_per_frame, n_samples, nn_err) and its guard
    ``if self.n_samples < self.n_max_samples``, which compares the number of processed EXAMPLES with ``n_samples`` -- kept as it is.
    ``compute`` returns the dict of the reference's ``savedir=None`` branch (:313-320); the plot branch (``savedir``) is not built."""

    def __init__(self, n_samples=1000):
        self.n_max_samples = n_samples
        self.reset()

    def reset(self):
        self.nn_err_per_frame, self.std_per_frame, self.mean_per_frame = [], [], []
        self.n_samples = 0
        self.nn_err = None

    def update(self, kps_pred, kps_target):
        if self.n_samples < self.n_max_samples:
            nn, sd, mean, _ = sample_stats(kps_frame_mse(kps_pred, kps_target))
            self.nn_err_per_frame.append(nn)
            self.std_per_frame.append(sd)
            self.mean_per_frame.append(mean)
            self.n_samples += kps_pred.size(0)
            v = nn.mean(1).sum()
            self.nn_err = v if self.nn_err is None else self.nn_err + v

    def compute(self, n_pokes=0):
        nn_mse = torch.cat(self.nn_err_per_frame, dim=0).mean(0).cpu().numpy()
        return {"NN MSE": nn_mse,
                "Mean MSE per Frame": torch.cat(self.mean_per_frame, dim=0).mean(0).cpu().numpy(),
                "Std per Frame": torch.cat(self.std_per_frame, dim=0).mean(0).cpu().numpy(),
                "Time": np.arange(nn_mse.shape[0]),
                "Number of Pokes": np.full_like(nn_mse, n_pokes, dtype=int)}


def _offdiag_mean(D):
    """mean over all ordered pairs j != k of D [..., ns, ns] (diagonal written as 0 by the kernels), float64 on the device"""
    ns = D.shape[-1]
    return D.double().sum() / (D.numel() // (ns * ns) * ns * (ns - 1))


def pairwise_mse(exmpls):
    """exmpls [n_ex, ns, ...] -> D fp32 [n_ex, ns, ns], D[e, j, k] = mean((v_j - v_k) ** 2)."""
    _lib.require_gpu()
    x = exmpls.float().contiguous()
    n_ex, ns = x.shape[:2]
    Lel = x[0, 0].numel()
    L = _lib.lib()
    ws = _workspace(L.ipoke_pair_mse_workspace_bytes(n_ex, ns, Lel), x.device)
    D = torch.empty(n_ex, ns, ns, dtype=torch.float32, device=x.device)
    check(L.ipoke_pair_mse(ptr(x), n_ex, ns, Lel, ptr(ws), ptr(D), _lib.current_stream()))
    return D


def compute_div_score_mse(exmpls, device=None):
    """metrics.py:104-124: the mean of mean((v_j - v_k) ** 2) over all ordered pairs j != k of all examples [n_ex, ns, s, C, H, W]."""
    if device is not None:
        exmpls = exmpls.to(device)
    return float(_offdiag_mean(pairwise_mse(exmpls)).item())


def normalize_input_vgg(x):
    """metrics.py:64-72: (x + 1) / 2, then the ImageNet mean / std, fp32 [N, 3, H, W], as one element-wise pass."""
    _lib.require_gpu()
    x = x.float().contiguous()
    N, C, H, W = x.shape
    if C != 3:
        raise ValueError(f"normalize_input_vgg expects 3 channels, got {C}")
    y = torch.empty_like(x)
    check(_lib.lib().ipoke_vgg_normalize(ptr(x), ptr(y), N, H, W, _lib.current_stream()))
    return y


def time_cosine(fmap, ns, s):
    """One feature map (``nn.CL`` of the ns * s frames of an example, bf16 or f32) -> fp32 [ns, ns]: the mean over locations of the cosine
    over the TIME axis of the time-normalized activations (metrics.py:60-62, 88-94)."""
    if fmap.N != ns * s:
        raise ValueError(f"feature map holds {fmap.N} frames, expected ns * s = {ns * s}")
    L = _lib.lib()
    t = fmap.t
    ws = _workspace(L.ipoke_time_cosine_workspace_bytes(ns, s, fmap.C, fmap.S), t.device)
    D = torch.empty(ns, ns, dtype=torch.float32, device=t.device)
    dt = _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32
    check(L.ipoke_time_cosine(ptr(t), t.shape[1], fmap.C, fmap.S, ns, s, dt, ptr(ws), ptr(D), _lib.current_stream()))
    return D


def div_score_maps(exmpls, feature_extractor, device=None):
    """The [n_ex, n_maps, ns, ns] table behind ``compute_div_score`` (device tensor)."""
    n_ex, ns, s, c, h, w = exmpls.shape
    rows = []
    with torch.no_grad():
        for video in exmpls:
            if device is not None:
                video = video.to(device)
            fmap = feature_extractor(normalize_input_vgg(video.reshape(-1, c, h, w)))
            rows.append(torch.stack([time_cosine(f, ns, s) for f in fmap]))
    return torch.stack(rows)


def compute_div_score(exmpls, feature_extractor, device=None):
    """metrics.py:74-102: the plain mean over every (example, j != k, map) entry of the time-axis cosine; the maps weigh equally, as in
    the reference's flat list.  One host read at the end (the reference: n_ex * ns * (ns - 1) * 5 ``.item()`` calls)."""
    return float(_offdiag_mean(div_score_maps(exmpls, feature_extractor, device)).item())


def video_to_uint8(x):
    """second_stage_video.py:673-675: fp32 [B, T, 3, H, W] in [-1, 1] -> uint8 [B, T, H, W, 3] = trunc((x + 1) * 127.5) on the device,
    bit-equal to numpy's ``astype(np.uint8)``; values outside [-1, 1] (where numpy's cast is undefined) are clamped to [0, 255]."""
    _lib.require_gpu()
    x = x.float().contiguous()
    B, T, C, H, W = x.shape
    if C != 3:
        raise ValueError(f"video_to_uint8 expects 3 channels, got {C}")
    y = torch.empty(B, T, H, W, 3, dtype=torch.uint8, device=x.device)
    check(_lib.lib().ipoke_video_to_u8(ptr(x), ptr(y), B * T, H, W, _lib.current_stream()))
    return y
