"""Timing of the test loop's reductions at the size the test loop runs (ns = 50 samples, 128 x 128, s = 15 frames, one example) against
the same quantity composed from per-pair torch ops on the same device in the same call -- the reference's formulation
(utils/metrics.py:74-124, 169-204).  The yardstick is the torch composition, never the kernels against themselves.

    python scripts/probe_test_modes.py [--out profiles/test_modes.txt] [--reps 5]

Device events around each call; the two variants of a row are alternated after one warm-up each, and min / median / max of the
repetitions are printed (the spread).  The torch composition keeps the reference's ``.item()`` / ``.cpu()`` per pair, which is part of what
it costs.  The VGG forward pass is shared by both sides of the cosine row and timed apart."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ipoke_amd import metrics, nn as K          # noqa: E402
from ipoke_amd.utils.detfill import deterministic_fill_          # noqa: E402
from ipoke_amd.vgg import metric_vgg16          # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def timed(fn, reps):
    """one variant alone: warm-up, then ``reps`` timed calls -> (last result, sorted ms)"""
    fn(); torch.cuda.synchronize()
    runs = [once(fn) for _ in range(reps)]
    return runs[-1][0], sorted(t for _, t in runs)


def timed_pair(ours, theirs, reps):
    """two variants of one quantity in the same call, ALTERNATED (ours, theirs, ours, ...) after one warm-up each, so that whatever else
    loads the host or the device during the window falls on both"""
    ours(); theirs(); torch.cuda.synchronize()
    to, tr = [], []
    for _ in range(reps):
        o, t = once(ours); to.append(t)
        r, t = once(theirs); tr.append(t)
    return (o, sorted(to)), (r, sorted(tr))


def spread(ts):
    return f"{ts[0]:9.3f} / {ts[len(ts) // 2]:9.3f} / {ts[-1]:9.3f}"


def torch_pair_mse(video):
    divl = []
    ns = video.shape[0]
    for j in range(ns):
        for k in range(ns):
            if j != k:
                divl.append(((video[j] - video[k]) ** 2).mean().cpu().numpy())
    return float(sum(float(d) for d in divl) / len(divl))


def torch_time_cos(fmaps, ns, s):
    d = torch.nn.CosineSimilarity(dim=0)
    norm = lambda x: x / (torch.sqrt(torch.sum(x ** 2, dim=0, keepdim=True)) + 1e-10)
    divl = []
    for j in range(ns):
        for k in range(ns):
            if j != k:
                for f in fmaps:
                    f = f.reshape(ns, s, *f.shape[1:])
                    divl.append(d(norm(f[j]), norm(f[k])).mean().item())
    return sum(divl) / len(divl)


def torch_sample_ssim(pred, target, ssim_map):
    bs, ns, s, c, h, w = pred.shape
    vals = []
    for p, t in zip(pred, target):
        t = torch.cat([t] * ns, dim=0)
        vals.append(ssim_map(p.reshape(-1, c, h, w), t.reshape(-1, c, h, w)).mean(dim=[1, 2, 3]).cpu())
    v = torch.stack(vals).reshape(bs, ns, s)
    ids = torch.argmin(v.mean(-1), 1)[:, None].repeat(1, s)[:, None]
    return v.gather(1, ids).squeeze(1), v.std(dim=1), v.mean(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/test_modes.txt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ns", type=int, default=50)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--frames", type=int, default=15)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: no device, no number"
    from tests.eval_ref import ssim_map
    ns, s, size = a.ns, a.frames, a.size
    g = torch.Generator().manual_seed(0)
    exmpls = (torch.rand(1, ns, s, 3, size, size, generator=g) * 2 - 1).cuda()
    target = (torch.rand(1, 1, s, 3, size, size, generator=g) * 2 - 1).cuda()
    lines = [f"test-loop reductions, ns={ns} s={s} {size}x{size}, one example; ms min / median / max over {a.reps} alternated runs after one warm-up, device events"]

    def row(name, ours, theirs, same):
        (o, to), (r, tr) = timed_pair(ours, theirs, a.reps)
        lines.append(f"{name:28s} kernels {spread(to)}   torch per-pair {spread(tr)}   "
                     f"ratio (median) {tr[len(tr) // 2] / to[len(to) // 2]:7.1f}x   deviation {same(o, r):.2e}")

    row("pairwise MSE score", lambda: metrics.compute_div_score_mse(exmpls), lambda: torch_pair_mse(exmpls[0]), lambda o, r: abs(o - r) / r)
    row("sample SSIM + statistics", lambda: metrics.sample_stats(metrics.sample_ssim(exmpls, target))[:3],
        lambda: torch_sample_ssim(exmpls, target, ssim_map), lambda o, r: max((x.cpu() - y).abs().max().item() for x, y in zip(o, r)))
    vgg = metric_vgg16(dtype="f32")
    deterministic_fill_(vgg, prefix="vgg16.")
    vgg = vgg.cuda()
    with torch.no_grad():
        x = metrics.normalize_input_vgg(exmpls[0].reshape(-1, 3, size, size))
        fm, tv = timed(lambda: vgg(x), a.reps)
        lines.append(f"{'VGG-16 forward (both sides)':28s}         {spread(tv)}")
        nchw = [K.to_nchw(f, "f32") for f in fm]
        row("time cosine, five maps", lambda: float(torch.stack([metrics.time_cosine(f, ns, s) for f in fm]).double().sum().item()) / (5 * ns * (ns - 1)),
            lambda: torch_time_cos(nchw, ns, s), lambda o, r: abs(o - r))
    x5 = exmpls[0, :8].contiguous()
    (o, to), (r, tr) = timed_pair(lambda: metrics.video_to_uint8(x5).cpu().numpy(),
                                  lambda: ((x5 + 1.) * 127.5).permute(0, 1, 3, 4, 2).cpu().numpy().astype("uint8"), a.reps)
    lines.append(f"{'uint8 export, 8 clips -> host':28s} kernel  {spread(to)}   torch + numpy  {spread(tr)}   "
                 f"bit-equal {bool((o == r).all())}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
