#!/usr/bin/env python3
"""Time of the clip augmentation at the c2 step's shape: ``ClipAugmenter.images`` + ``.flow`` for B = 20 clips of T = 16 frames at 128 px,
with HIP events after a warm-up; and, where Pillow imports, the per-frame chain the reference runs in its loader workers
(data/base_dataset.py:432-440: three ImageEnhance blends, the HSV round trip, pad, transform, crop, ToTensor) for one frame on one CPU core.

    python scripts/time_augment.py [--iters 50]

A record for DESIGN.md, not a gate; nothing imports this file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ipoke_amd.data import ClipAugmenter               # noqa: E402

B, T, S = 20, 16, 128
CONFIG = {"augment": True, "p_col": .8, "p_geom": .8, "augment_b": 0.4, "augment_c": 0.5, "augment_h": 0.15, "augment_s": 0.4, "aug_deg": 15,
          "aug_trans": (0.1, 0.1), "spatial_size": (S, S)}


def device_time(iters):
    aug = ClipAugmenter(dict(CONFIG, p_col=1, p_geom=1))                # every sample jittered and warped
    p = aug.draw(B, np.random.RandomState(0))
    gen = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (B, T, S, S, 3), device="cuda", generator=gen, dtype=torch.uint8)
    flow = torch.randn(B, 2, S, S, device="cuda", generator=gen)
    for _ in range(5):
        aug.images(frames, p), aug.flow(flow, p)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        aug.images(frames, p), aug.flow(flow, p)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times = np.array(times)
    return float(np.median(times)), float(times.min()), float(times.max())


def pillow_time(iters):
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return None
    from tests import augment_ref
    rng = np.random.RandomState(0)
    frame = rng.randint(0, 256, (S, S, 3)).astype(np.uint8)
    matrix = augment_ref.affine_matrix(11.0, 5, -4, S)
    P = S // 2

    def chain():
        img = Image.fromarray(frame)
        img = ImageEnhance.Brightness(img).enhance(1.2)
        img = ImageEnhance.Contrast(img).enhance(0.8)
        h, s, v = img.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        np_h += np.uint8(20)
        img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
        img = ImageEnhance.Color(img).enhance(1.3)
        img = Image.fromarray(np.pad(np.asarray(img), ((P, P), (P, P), (0, 0)), mode="reflect"))
        img = img.transform((2 * S, 2 * S), Image.AFFINE, matrix, Image.NEAREST).crop((P, P, P + S, P + S))
        return torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(255) * 2.0 - 1.0

    for _ in range(5):
        chain()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        chain()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    torch.set_num_threads(1)
    med, lo, hi = device_time(args.iters)
    moved = B * T * (S * S * 3 + S * S * 3 * 4) + B * T * S * S * 3
    res = {"shape": [B, T, S], "device_ms_median": round(med, 4), "device_ms_min": round(lo, 4), "device_ms_max": round(hi, 4),
           "device_GBps": round(moved / med / 1e6, 1), "iters": args.iters}
    cpu = pillow_time(args.iters)
    if cpu is not None:
        res["pillow_ms_per_frame_one_core"] = round(cpu, 4)
        res["pillow_ms_per_step_16_cores"] = round(cpu * B * T / 16, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
