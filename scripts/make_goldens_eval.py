"""Golden vectors of the test loop's reductions: tests/golden/g17_test_modes.npz.

Runs the REFERENCE's own ``SampleMetric``, ``compute_div_score_mse`` and ``compute_div_score`` (utils/metrics.py) on the CPU through
oracle/ref_import.py and stores inputs and outputs only.  Run it where the reference checkout is available:

    python scripts/make_goldens_eval.py

Two third-party pieces the reference calls do not exist there; their stand-ins are PARITY UNPINNED (the wording of
oracle/metrics_ref.py: no vector of the library itself can be generated):

* ``pytorch_lightning.metrics.functional.ssim(reduction='none')`` -> ``tests.eval_ref.ssim_map``, a ``reduction='none'`` restatement of the
  published algorithm, passed to the reference's ``SampleMetric(measure=..., key='SSIM', reduction=False)`` constructor (what its
  ``SampleSSIM`` subclass does with the library function);
* ``kornia.enhance.normalize.normalize`` -> a real module inserted into ``sys.modules`` before the call that computes
  ``(x - mean[None, :, None, None]) / std[None, :, None, None]``.

The feature extractor handed to the reference's ``compute_div_score`` is a plain torch ``nn.Sequential`` VGG-16 topology
(``tests.eval_ref.vgg16_features``) whose weights are the name-keyed deterministic fill (ipoke_amd/utils/detfill.py, prefix
``vgg16.features.``): torchvision and its ImageNet checkpoint are not available.

The file is written with fixed zip time stamps, so a rerun reproduces it byte for byte."""
import io
import logging
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import                      # noqa: E402
from tests import eval_ref                         # noqa: E402

SSIM_TOL = 2e-5                                    # the GPU tests' bound on an SSIM value: arg-min gaps must be >= 100 x this


def install_kornia_normalize():
    def normalize(data, mean, std):
        return (data - mean[None, :, None, None]) / std[None, :, None, None]
    kornia, enhance, norm = types.ModuleType("kornia"), types.ModuleType("kornia.enhance"), types.ModuleType("kornia.enhance.normalize")
    kornia.__path__, enhance.__path__ = [], []
    norm.normalize = normalize
    kornia.enhance, enhance.normalize = enhance, norm
    sys.modules.update({"kornia": kornia, "kornia.enhance": enhance, "kornia.enhance.normalize": norm})


def make_case(seed, bs, ns, s, size=32):
    """Clips in [-1, 1]: smooth targets, samples = target + noise of a different strength per sample (distinct mean SSIMs)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(bs, 1, s, 3, size // 4, size // 4, generator=g) * 2 - 1
    target = torch.nn.functional.interpolate(base.reshape(-1, 3, size // 4, size // 4), size=(size, size), mode="bilinear", align_corners=False)
    target = (target.reshape(bs, 1, s, 3, size, size) + 0.05 * torch.randn(bs, 1, s, 3, size, size, generator=g)).clamp(-1, 1)
    strength = torch.stack([torch.randperm(ns, generator=g) for _ in range(bs)]).float()          # 0 .. ns-1, shuffled per example
    noise = torch.randn(bs, ns, s, 3, size, size, generator=g) * (0.08 + 0.12 * strength)[:, :, None, None, None, None]
    pred = (target + noise).clamp(-1, 1)
    return pred.contiguous(), target.contiguous()


def run_sample_metric(M, pred, target, n_max):
    seen = []

    def measure(p, t):
        m = eval_ref.ssim_map(p, t)
        seen.append(m.mean(dim=[1, 2, 3]).clone())
        return m
    metric = M.SampleMetric(measure, logging.getLogger("g17"), n_max, key="SSIM", reduction=False)
    metric.update(pred, target)
    meanval, d = metric.compute()
    bs, ns, s = pred.shape[:3]
    vals = torch.stack(seen).reshape(bs, ns, s)
    means = vals.mean(-1).sort(dim=1).values
    gap = (means[:, 1:] - means[:, :-1]).min().item()
    assert gap >= 100 * SSIM_TOL, f"per-sample mean SSIMs too close for an exact arg-min: gap {gap}"
    return {"vals": vals.numpy(), "nn": torch.cat(metric.nn_val_per_frame).numpy(), "std": torch.cat(metric.std_per_frame).numpy(),
            "mean": torch.cat(metric.mean_per_frame).numpy(), "argmin": torch.argmin(vals.mean(-1), 1).numpy().astype(np.int32),
            "meanval": np.float32(meanval.item()), "dict_nn": d["SSIM NN"], "dict_mean": d["Mean SSIM per Frame"], "dict_std": d["Std per Frame"]}


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)                        # one summation order whatever the host
    install_kornia_normalize()
    M = ref_import.ref("utils.metrics")
    M.tqdm = lambda it, *a, **k: it
    extractor = eval_ref.Vgg16Taps(eval_ref.filled_vgg16()).eval()
    out = {}
    for tag, (seed, bs, ns, s) in {"a": (17, 2, 3, 4), "b": (18, 1, 5, 4)}.items():
        pred, target = make_case(seed, bs, ns, s)
        out[f"{tag}_pred"], out[f"{tag}_target"] = pred.numpy(), target.numpy()
        for k, v in run_sample_metric(M, pred, target, n_max=5).items():
            out[f"{tag}_ssim_{k}"] = v
        out[f"{tag}_div_mse"] = np.float64(M.compute_div_score_mse(pred))
        out[f"{tag}_div_vgg"] = np.float64(M.compute_div_score(pred, extractor))
        with torch.no_grad():
            fm = extractor(eval_ref.normalize_input_vgg(pred[0].reshape(-1, 3, 32, 32)))
        dead = sum(int((f.reshape(ns, s, *f.shape[1:]).abs().amax(dim=1) == 0).sum()) for f in fm)
        assert dead > 0, "no VGG location is zero in every frame: the epsilon path would not be exercised"
        print(f"case {tag}: bs {bs} ns {ns} s {s}; div mse {out[f'{tag}_div_mse']:.6f}, div vgg {out[f'{tag}_div_vgg']:.6f}; "
              f"{dead} (sample, location) vectors are zero in every frame")
    path = os.path.join(ROOT, "tests", "golden", "g17_test_modes.npz")
    write_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
