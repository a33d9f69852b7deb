"""Float64 restatement of the three keypoint pieces of the reference, written from the cited lines, for tests/test_kps_cpu.py and
tests/test_kps_gpu.py:

    posture_nn          get_nn / measure (data/flow_dataset.py:628-713, :635-646), with a STABLE argsort: the reference's default argsort
                        leaves ties open, the kernels order candidates by (D, j)
    keypoint_poke       _get_keypoint_poke (data/base_dataset.py:462-497), the draws handed in
    draw_keypoint_ids   its np.random calls (:470-473)
    kps_frame_mse, KPSMetricRef   KPSMetric (utils/metrics.py:259-331)

and the tolerance rule of the posture distances.  numpy only; nothing here imports the package."""
import numpy as np

EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ posture nearest neighbours
def posture_dist(kps, i):
    """:638: np.linalg.norm(kps[idx][None] - kps, axis=-1).sum(-1) in float64"""
    kps = np.asarray(kps, dtype=np.float64)
    return np.linalg.norm(kps[i][None] - kps, axis=-1).sum(-1)


def posture_nn_one(kps, vid, i):
    """measure(idx) (:635-646) -> (nn_general, nn_other_vid or -1, D)"""
    D = posture_dist(kps, i)
    order = np.argsort(D, kind="stable")
    other = np.flatnonzero(vid[order] != vid[i])
    return int(order[1]), (int(order[other[0]]) if other.size else -1), D


def posture_nn(kps, vid, ids=None):
    """get_nn's loop (:657-668) -> (nn_general, nn_other_vid) int64 [M]; -1 where no frame of another video exists"""
    vid = np.asarray(vid)
    ids = np.arange(len(vid)) if ids is None else np.asarray(ids)
    out = np.array([posture_nn_one(kps, vid, int(i))[:2] for i in ids], dtype=np.int64).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def posture_tol(K, d_max):
    """Bound on the fp32 error of a K-term sum of hypotenuses of size up to d_max: each term carries the roundings of two differences, a
    product, a fused multiply-add and a square root (under 4 units of 2^-24 relative), the K - 1 additions one unit each on a partial sum
    of at most d_max -- (K + 4) units, doubled for the two distances a comparison involves."""
    return 2.0 * (K + 4) * EPS32 * d_max


def posture_dist_fp32(kps32, i):
    """the kernel's arithmetic emulated in numpy fp32: rounded differences, dy * dy + dx * dx with one rounding on the sum (the fused form
    rounds once; emulated in float64 and rounded), a correctly rounded root, the K terms added in index order"""
    kps32 = np.asarray(kps32, dtype=np.float32)
    d = kps32[i][None] - kps32
    dx, dy = d[..., 0], d[..., 1]
    sq = (dy.astype(np.float64) * dy.astype(np.float64) + (dx * dx).astype(np.float64)).astype(np.float32)
    term = np.sqrt(sq)
    acc = np.zeros(len(kps32), dtype=np.float32)
    for k in range(kps32.shape[1]):
        acc = acc + term[:, k]
    return acc


def posture_truth(kps, vid, i):
    """query i in float64 from one sort: (nn_general, nn_other_vid, tol, gap of nn_general to its neighbours in the order, gap of
    nn_other_vid to its runner-up, D[nn_general], D[nn_other_vid], max D); -1 / inf where no frame of another video exists"""
    vid = np.asarray(vid)
    D = posture_dist(kps, i)
    order = np.argsort(D, kind="stable")
    tol = posture_tol(np.shape(kps)[1], float(D.max()))
    # the second entry must be clear of the third AND of the first one, or two of them swap and nn_general changes
    gap_g = min(float(D[order[2]] - D[order[1]]) if len(order) > 2 else np.inf, float(D[order[1]] - D[order[0]]))
    oth = order[vid[order] != vid[i]]
    gap_o = float(D[oth[1]] - D[oth[0]]) if len(oth) > 1 else np.inf
    o = int(oth[0]) if len(oth) else -1
    return int(order[1]), o, tol, gap_g, gap_o, float(D[order[1]]), float(D[o]) if o >= 0 else np.inf, float(D.max())


def posture_gaps(kps, vid, i):
    """(tol, gap of nn_general, gap of nn_other_vid) of query i in float64"""
    return posture_truth(kps, vid, i)[2:5]


def real_case():
    """the real-valued posture case: N = 3001, K = 17, RandomState(0).rand as float32, videos of 40 frames"""
    kps = np.random.RandomState(0).rand(3001, 17, 2).astype(np.float32)
    return kps, (np.arange(3001) // 40).astype(np.int64)


def exact_case(N, K, n_vid, seed):
    """Integer keypoints in [0, 64) with y fixed per keypoint slot: every term is an integer |dx| and every sum is exact in fp32, so the
    kernel must reproduce the float64 order for EVERY query, ties (which go to the lower index) included -- random integers tie by
    themselves all the time.  n_vid contiguous videos.  Where N allows it (>= 64) the case also carries, by design:
        frame N // 2 = frame 3                         a duplicate AFTER the query 3, and for the query N // 2 one BEFORE it (it is then
                                                       its own nn_general, as a stable sort has it)
        frames 7 = 9 = 11                              a triple
        frames 20 and 40 = frame 30 with slot 0 one to the right / one to the left: a tie at distance 1, which goes to 20
        frame N - 1 = frame 10 with slot K - 1 moved by 2: with n_vid > 1 the nearest other-video frame of query 10, in the last
                                                       candidate chunk and its ragged tile
    -> (kps float32 [N, K, 2], vid int64 [N])"""
    rs = np.random.RandomState(seed)
    kps = np.zeros((N, K, 2), dtype=np.float32)
    kps[..., 0] = rs.randint(0, 64, (N, K))
    kps[..., 1] = rs.randint(0, 64, K)[None]
    vid = (np.arange(N) * n_vid // N).astype(np.int64)
    if N >= 64:
        kps[N // 2] = kps[3]
        kps[9] = kps[11] = kps[7]
        kps[30, 0, 0] = 30
        kps[20], kps[40] = kps[30], kps[30]
        kps[20, 0, 0], kps[40, 0, 0] = 31, 29
        kps[N - 1] = kps[10]
        kps[N - 1, K - 1, 0] = kps[10, K - 1, 0] + (2 if kps[10, K - 1, 0] < 60 else -2)
    return kps, vid


# ------------------------------------------------------------------------------------------------ keypoint pokes
def draw_keypoint_ids(B, K, n_pokes, fix_n_pokes, rng):
    """:470-473 per sample: randint(1, n_pokes, 1) unless fix_n_pokes, then choice(K, n, replace=False) -> int32 [B, n_pokes], -1 padded"""
    out = np.full((B, n_pokes), -1, dtype=np.int32)
    for b in range(B):
        n = n_pokes if fix_n_pokes else int(rng.randint(1, n_pokes, 1)[0])
        out[b, :n] = rng.choice(K, n, replace=False)
    return out


def keypoint_poke_one(kpsrc, kptgt, poke_ids, spatial_size, poke_size, n_pokes):
    """:475-497 for one sample, poke_ids the drawn ids (no padding) -> (poke float64 [2, H, W], coords int32 [n_pokes, 2], ids int32 [n_pokes])"""
    kpsrc, kptgt = np.asarray(kpsrc, dtype=np.float64), np.asarray(kptgt, dtype=np.float64)
    valid_h = [poke_size, spatial_size[0] - poke_size]
    valid_w = [poke_size, spatial_size[1] - poke_size]
    poke = np.zeros((2, *spatial_size), dtype=float)
    half = int(poke_size / 2)
    coords = []
    for idx in poke_ids:
        y = int(kpsrc[idx, 1] * spatial_size[1])
        x = int(kpsrc[idx, 0] * spatial_size[0])
        if valid_w[0] <= x <= valid_w[1] and valid_h[0] <= y <= valid_h[1]:
            diff = (kptgt[idx] - kpsrc[idx])[:, None, None] * spatial_size[0]
            poke[:, y - half:y + half + 1, x - half:x + half + 1] = diff
        coords.append([y, x])
    n = len(poke_ids)
    ids_out = np.full((n_pokes,), -1, dtype=np.int32)
    coords_out = np.full((n_pokes, 2), -1, dtype=np.int32)
    coords_out[:n] = np.asarray(coords, dtype=np.int32).reshape(n, 2)
    ids_out[:n] = poke_ids
    return poke, coords_out, ids_out


def keypoint_poke(kp_src, kp_tgt, poke_ids, spatial_size, poke_size):
    """the batch form the kernels compute: poke_ids int [B, n_pokes], -1 padded -> (poke fp32 [B, 2, H, W], coords, ids)"""
    poke_ids = np.asarray(poke_ids)
    rows = [keypoint_poke_one(kp_src[b], kp_tgt[b], poke_ids[b][poke_ids[b] >= 0], spatial_size, poke_size, poke_ids.shape[1])
            for b in range(len(poke_ids))]
    return (np.stack([r[0] for r in rows]).astype(np.float32), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]))


# ------------------------------------------------------------------------------------------------ KPSMetric
def kps_frame_mse(pred, target):
    """:294, :299: mean over the keypoints and coordinates of (pred - target)^2 -> float64 [bs, ns, s]"""
    d = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    return (d * d).mean(axis=(3, 4))


def sample_stats(vals):
    """:296-302 -> (values of the arg-min-mean sample [bs, s], unbiased std over the samples, mean over the samples, index [bs])"""
    vals = np.asarray(vals, dtype=np.float64)
    idx = vals.mean(axis=2).argmin(axis=1)
    nn = np.take_along_axis(vals, idx[:, None, None], axis=1)[:, 0]
    return nn, vals.std(axis=1, ddof=1), vals.mean(axis=1), idx


class KPSMetricRef:
    """the state, the example-count guard and the dict of the reference (:286-320), float64"""

    def __init__(self, n_samples=1000):
        self.n_max_samples = n_samples
        self.nn_err_per_frame, self.std_per_frame, self.mean_per_frame = [], [], []
        self.n_samples, self.nn_err = 0, 0.0

    def update(self, pred, target):
        if self.n_samples < self.n_max_samples:
            nn, sd, mean, _ = sample_stats(kps_frame_mse(pred, target))
            self.nn_err_per_frame.append(nn)
            self.std_per_frame.append(sd)
            self.mean_per_frame.append(mean)
            self.n_samples += len(pred)
            self.nn_err += nn.mean(1).sum()

    def compute(self, n_pokes=0):
        nn = np.concatenate(self.nn_err_per_frame, 0).mean(0)
        return {"NN MSE": nn, "Mean MSE per Frame": np.concatenate(self.mean_per_frame, 0).mean(0),
                "Std per Frame": np.concatenate(self.std_per_frame, 0).mean(0), "Time": np.arange(nn.shape[0]),
                "Number of Pokes": np.full_like(nn, n_pokes, dtype=int)}
