"""CPU restatements of the test loop's reductions (reference utils/metrics.py:60-124, 149-217; second_stage_video.py:673-675) for the
sizes that have no golden vector.  tests/test_test_modes_cpu.py checks every one of them against golden g17_test_modes, which holds the
outputs of the reference's own functions (scripts/make_goldens_eval.py); the GPU tests then use them at the sizes the test loop runs.

PARITY UNPINNED, as in oracle/metrics_ref.py: ``ssim_map`` restates pytorch_lightning.metrics.functional.ssim(reduction='none'), and
``normalize_input_vgg`` computes what kornia.enhance.normalize.normalize does; neither library exists where the goldens are made."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.metrics_ref import _gaussian

VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)          # vgg16().features[:30]
VGG16_TAPS = (3, 8, 15, 22, 29)


def ssim_map(preds, target, kernel_size=(11, 11), sigma=(1.5, 1.5), k1=0.01, k2=0.03):
    """oracle/metrics_ref.py:ssim without the final mean: the cropped map [N, C, H - 10, W - 10] (``reduction='none'``)."""
    data_range = max(preds.max() - preds.min(), target.max() - target.min())
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    channel, dtype = preds.size(1), preds.dtype
    kernel = torch.matmul(_gaussian(kernel_size[0], sigma[0], dtype).t(), _gaussian(kernel_size[1], sigma[1], dtype))
    kernel = kernel.expand(channel, 1, kernel_size[0], kernel_size[1]).to(preds.device)
    pad_w, pad_h = (kernel_size[0] - 1) // 2, (kernel_size[1] - 1) // 2
    preds = F.pad(preds, (pad_w, pad_w, pad_h, pad_h), mode="reflect")
    target = F.pad(target, (pad_w, pad_w, pad_h, pad_h), mode="reflect")
    inputs = torch.cat((preds, target, preds * preds, target * target, preds * target))
    outputs = F.conv2d(inputs, kernel, groups=channel)
    n = preds.size(0)
    o = [outputs[x * n:(x + 1) * n] for x in range(5)]
    mu_pred_sq, mu_target_sq, mu_pred_target = o[0].pow(2), o[1].pow(2), o[0] * o[1]
    sigma_pred_sq, sigma_target_sq, sigma_pred_target = o[2] - mu_pred_sq, o[3] - mu_target_sq, o[4] - mu_pred_target
    upper = 2 * sigma_pred_target + c2
    lower = sigma_pred_sq + sigma_target_sq + c2
    ssim_idx = ((2 * mu_pred_target + c1) * upper) / ((mu_pred_sq + mu_target_sq + c1) * lower)
    return ssim_idx[..., pad_h:-pad_h, pad_w:-pad_w]


def sample_ssim(pred, target):
    """pred [bs, ns, s, C, H, W], target [bs, 1, s, C, H, W] -> [bs, ns, s] (metrics.py:178-193, one measure call per example)."""
    bs, ns, s, c, h, w = pred.shape
    vals = []
    for p, t in zip(pred, target):
        t = torch.cat([t] * ns, dim=0)
        vals.append(ssim_map(p.reshape(-1, c, h, w), t.reshape(-1, c, h, w)).mean(dim=[1, 2, 3]))
    return torch.stack(vals, dim=0).reshape(bs, ns, s)


def sample_stats(vals):
    """metrics.py:193-199 -> (nn per frame, std per frame, mean per frame, chosen index)."""
    min_ids = torch.argmin(vals.mean(-1), 1)
    gather = min_ids[:, None].repeat(1, vals.size(2))[:, None]
    return vals.gather(1, gather).squeeze(1), vals.std(dim=1), vals.mean(dim=1), min_ids


def pair_mse(exmpls):
    """[n_ex, ns, ...] -> float64 [n_ex, ns, ns] of mean((v_j - v_k) ** 2)."""
    x = exmpls.double().flatten(2)
    return ((x[:, :, None] - x[:, None, :]) ** 2).mean(-1)


def offdiag_mean(D):
    ns = D.shape[-1]
    mask = ~torch.eye(ns, dtype=torch.bool)
    return D.double()[..., mask].mean().item()


def normalize_input_vgg(x):
    out = (x + 1.) / 2.
    mean, std = torch.tensor([0.485, 0.456, 0.406]).type_as(out), torch.tensor([0.229, 0.224, 0.225]).type_as(out)
    return (out - mean[None, :, None, None]) / std[None, :, None, None]


def time_cosine(fmap, ns, s, dtype=torch.float32):
    """fmap [ns * s, C, h, w] -> [ns, ns]: metrics.py:88-94 for one map (normalize_activation over dim 0 of f[j] -- time -- and
    CosineSimilarity(dim=0)); the diagonal is left 0."""
    f = fmap.to(dtype).reshape(ns, s, *fmap.shape[1:])
    d = nn.CosineSimilarity(dim=0)
    norm = lambda x: x / (torch.sqrt(torch.sum(x ** 2, dim=0, keepdim=True)) + 1e-10)
    out = torch.zeros(ns, ns, dtype=dtype)
    for j in range(ns):
        for k in range(ns):
            if j != k:
                out[j, k] = d(norm(f[j]), norm(f[k])).mean()
    return out


def vgg16_features():
    """torchvision.models.vgg16().features[:30] as a plain nn.Sequential (same indices, so the state-dict keys are torchvision's)."""
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=False)]
            cin = v
    return nn.Sequential(*layers)


class Vgg16Taps(nn.Module):
    """The five maps after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of a ``vgg16_features`` stack."""

    def __init__(self, features):
        super().__init__()
        self.features = features

    def forward(self, x):
        out = []
        for i, layer in enumerate(self.features):
            x = layer(x)
            if i in VGG16_TAPS:
                out.append(x)
        return out


def filled_vgg16():
    from ipoke_amd.utils.detfill import deterministic_fill_
    feats = vgg16_features()
    deterministic_fill_(feats, prefix="vgg16.features.")
    return feats


def div_score(exmpls, extractor):
    """compute_div_score (metrics.py:74-102) composed from the pieces above: (score, [n_ex, 5, ns, ns] table)."""
    n_ex, ns, s, c, h, w = exmpls.shape
    rows = []
    with torch.no_grad():
        for video in exmpls:
            fmap = extractor(normalize_input_vgg(video.reshape(-1, c, h, w)))
            rows.append(torch.stack([time_cosine(f, ns, s) for f in fmap]))
    D = torch.stack(rows)
    return offdiag_mean(D), D


def video_to_uint8(x):
    """second_stage_video.py:673: [B, T, 3, H, W] -> uint8 [B, T, H, W, 3]."""
    return ((x + 1.) * 127.5).permute(0, 1, 3, 4, 2).cpu().numpy().astype(np.uint8)
