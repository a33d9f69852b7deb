#!/usr/bin/env python3
"""Golden G21: the reference's own keypoint pieces -- get_nn (data/flow_dataset.py:628-713), BaseDataset._get_keypoint_poke
(data/base_dataset.py:462-497) and KPSMetric (utils/metrics.py:259-331) -- run on synthetic keypoints.

    python scripts/make_goldens_keypoints.py       # CPU, needs the reference checkout (oracle/ref_import.py); writes
                                                   # tests/golden/g21_keypoints.npz

Run by hand where the reference checkout is; nothing imports it and no GPU test needs it.  The reference's functions are called on
SimpleNamespace stand-ins that carry exactly the attributes they read.

  nn    get_nn(ids, stand_in) for N = 600 frames, K = 17 keypoints, 12 videos of unequal length, every frame a query: its result, the
        nearest frame of another video.  The keypoints are stored as float32 (what the kernel is given) and handed to the reference as
        float64, so that its result is the float64 truth of those inputs.
  kp    _get_keypoint_poke at 64 px / poke 5 and 128 px / poke 10, fixed and drawn n_pokes, np.random seeded per case (the seed is
        stored: PokeSimulator.draw_keypoint_ids must make the same draws).  Keypoint 0 .. 7 of every case sit on the edges of the valid
        window -- column / row exactly poke_size and size - poke_size (inside, both ends are inclusive), one less and one more
        (outside) -- and keypoint 8 has x = the double just below c / size, whose double product with size lies within 1e-12 below the
        integer c and truncates to c - 1 where an fp32 product gives c.  Cases with fix_n_pokes draw all of these.
  kps   KPSMetric.update twice and compute(n_pokes=3) with bs = 2, ns = 5, s = 4, K = 17.

Condition for exactness: inputs whose decisive float64 distances tie, or lie closer than the tolerance of tests/kps_exact.py
(posture_tol), are re-seeded and never tolerated; so are KPSMetric inputs whose two best sample means lie closer than 1e-4 relative.  The
smallest margins met are printed and stored.
"""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import                                             # noqa: E402
from tests import kps_exact as E                                          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g21_keypoints.npz")
MAX_BYTES = 1024 * 1024
N_NN, K, N_VIDEOS = 600, 17, 12
N_POKES = 5
KP_CASES = ((64, 5, False), (64, 5, True), (128, 10, False), (128, 10, True))        # size, poke size, fix_n_pokes
KP_PER_CASE = 6
KPS_SHAPE = dict(bs=2, ns=5, s=4, K=17)
KPS_MARGIN = 1e-4


def nn_inputs(seed):
    rs = np.random.RandomState(seed)
    kps = rs.rand(N_NN, K, 2).astype(np.float32)
    cuts = np.sort(rs.choice(np.arange(20, N_NN - 20), N_VIDEOS - 1, replace=False))
    vid = np.searchsorted(cuts, np.arange(N_NN), side="right").astype(np.int64)
    return kps, vid


def nn_margin(kps, vid):
    """the smallest (gap - 2 tol) over all queries and both answers"""
    low = np.inf
    for i in range(len(kps)):
        tol, gap_g, gap_o = E.posture_gaps(kps, vid, i)
        low = min(low, gap_g - 2 * tol, gap_o - 2 * tol)
    return low


def kp_inputs(size, ps, seed):
    """K keypoints, source and target, as relative (x, y) doubles; 0 .. 7 on the window's edges, 8 just below an integer product"""
    rs = np.random.RandomState(seed)
    src = 0.15 + 0.7 * rs.rand(K, 2)
    tgt = src + 0.1 * (rs.rand(K, 2) - 0.5)
    lo, hi = ps, size - ps

    def at(c):                                   # a coordinate whose product with size truncates to c: the middle of the pixel
        return (c + 0.5) / size

    edge = [(lo, 30), (lo - 1, 30), (hi, 31), (hi + 1, 31), (29, lo), (29, lo - 1), (33, hi), (33, hi + 1)]          # (col, row)
    for k, (c, r) in enumerate(edge):
        src[k] = (at(c), at(r))
    c = size // 2 + 3
    src[8] = (np.nextafter(c / size, 0.0), at(size // 2))
    assert 0 < c - src[8, 0] * size < 1e-12 and int(src[8, 0] * size) == c - 1 and int(np.float32(src[8, 0]) * np.float32(size)) == c
    return src, tgt


def kps_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    s = KPS_SHAPE
    out = []
    for _ in range(2):
        target = torch.rand(s["bs"], 1, s["s"], s["K"], 2, generator=g)
        pred = target + 0.05 * torch.randn(s["bs"], s["ns"], s["s"], s["K"], 2, generator=g)
        out.append((pred, target))
    return out


def kps_margin(updates):
    low = np.inf
    for pred, target in updates:
        means = np.sort(E.kps_frame_mse(pred.numpy(), target.numpy()).mean(2), axis=1)
        low = min(low, float(((means[:, 1] - means[:, 0]) / means[:, 1]).min()))
    return low


def main():
    fd, bd, M = (ref_import.ref(m) for m in ("data.flow_dataset", "data.base_dataset", "utils.metrics"))
    np.int, np.bool = int, bool                    # the reference predates numpy 1.24 (set after the imports: scipy's star import of numpy)
    arrs = {}

    # ---- get_nn
    seed = 2100
    while True:
        kps, vid = nn_inputs(seed)
        low = nn_margin(kps, vid)
        if low > 0:
            break
        seed += 1
        assert seed < 2200, "no seed meets the distance condition"
    stand_in = types.SimpleNamespace(train=True, datadict={"keypoints_rel": kps.astype(np.float64), "vid": vid})
    ids = np.arange(N_NN)
    nn_other = np.asarray(fd.get_nn(ids, stand_in)).astype(np.int64)
    assert nn_other.shape == (N_NN,) and (vid[nn_other] != vid).all()
    print(f"nn: seed {seed}, smallest gap - 2 tol {low:.3e}")
    arrs.update(nn_kps=kps, nn_vid=vid, nn_other_vid=nn_other, nn_margin=np.float64(low), nn_seed=np.int64(seed))

    # ---- _get_keypoint_poke
    ci = 0
    for size, ps, fix in KP_CASES:
        for j in range(KP_PER_CASE):
            cseed = 21000 + 100 * size + 10 * int(fix) + j
            src, tgt = kp_inputs(size, ps, cseed)
            fake = types.SimpleNamespace(config={"n_pokes": K if fix else N_POKES, "spatial_size": (size, size), "poke_size": ps},
                                         datadict={"keypoints_rel": np.stack([src, tgt])}, subsample_step=1, max_frames=1, fix_n_pokes=fix,
                                         valid_h=[ps, size - ps], valid_w=[ps, size - ps])
            np.random.seed(cseed)
            poke, coords, pids = bd.BaseDataset._get_keypoint_poke(fake, (0, 1))
            assert poke.dtype == torch.float64
            arrs.update({f"kp_src{ci}": src, f"kp_tgt{ci}": tgt, f"kp_poke{ci}": poke.numpy().astype(np.float32),
                         f"kp_coords{ci}": coords.numpy().astype(np.int32), f"kp_ids{ci}": pids.numpy().astype(np.int32),
                         f"kp_meta{ci}": np.array([size, ps, int(fix), fake.config["n_pokes"], cseed])})
            ci += 1
    arrs["kp_n_cases"] = np.int64(ci)
    print(f"kp: {ci} cases")

    # ---- KPSMetric
    seed = 2150
    while True:
        updates = kps_inputs(seed)
        low = kps_margin(updates)
        if low > KPS_MARGIN:
            break
        seed += 1
    metric = M.KPSMetric(mock.MagicMock(), n_samples=1000)
    for u, (pred, target) in enumerate(updates):
        metric.update(pred, target)
        arrs[f"kps_pred{u}"], arrs[f"kps_target{u}"] = pred.numpy(), target.numpy()
    out = metric.compute(n_pokes=3)
    assert list(out) == ["NN MSE", "Mean MSE per Frame", "Std per Frame", "Time", "Number of Pokes"]
    for k, v in out.items():
        arrs["kps_out_" + k.replace(" ", "_")] = np.asarray(v)
    arrs["kps_nn_err"], arrs["kps_n_samples"] = np.float64(float(metric.nn_err)), np.int64(int(metric.n_samples))
    arrs["kps_margin"] = np.float64(low)
    print(f"kps: seed {seed}, smallest relative gap of the two best sample means {low:.3e}")

    np.savez_compressed(OUT, **arrs)
    nbytes = os.path.getsize(OUT)
    assert nbytes <= MAX_BYTES, nbytes
    print(f"wrote {OUT}: {nbytes / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
