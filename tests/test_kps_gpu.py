"""The keypoint path on the device against the float64 restatement of tests/kps_exact.py and golden G21 (the reference's own get_nn,
_get_keypoint_poke and KPSMetric): ``ipoke_posture_nn`` / ``data.posture_nearest_neighbours``, ``ipoke_keypoint_poke`` /
``PokeSimulator.keypoint_poke`` / ``make_batch(keypoints=)``, ``ipoke_kps_frame_mse`` / ``metrics.KPSMetric``.  The C-ABI calls of this
file hand over buffers with guard rows in front and behind, which must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

from ipoke_amd import _lib, configs, data, metrics
from ipoke_amd._lib import check, ptr
from ipoke_amd.data import PokeSimulator
from ipoke_amd.second_stage import PokeMotionModel
from ipoke_amd.utils.detfill import deterministic_fill_
from tests import kps_exact as E
from tests.helpers import synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 17
GUARD = 4096                       # elements in front of and behind every buffer the kernels are given
SENTINEL = {torch.float32: -12345.5, torch.float64: -12345.5, torch.int64: -7777, torch.int32: -7777, torch.uint8: 0xA5}


class Guarded:
    """a device buffer of ``shape`` between two guard rows filled with a sentinel"""

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.t = self.full[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill))

    def intact(self):
        s = SENTINEL[self.full.dtype]
        return bool((self.full[:GUARD] == s).all()) and bool((self.full[-GUARD:] == s).all())


def _intact(bufs):
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.intact(), f"guard rows of {name} were written"


def grid_of(N, k, M):
    out = (ctypes.c_int32 * 4)()
    check(_lib.lib().ipoke_posture_nn_grid(N, k, M, out))
    return list(out)                                          # query blocks, chunks, chunk length, tile


def posture_nn_guarded(kps, vid, ids=None, want_dist=True):
    """ipoke_posture_nn through the C ABI on guarded buffers -> (nn_general, nn_other_vid, dist or None) as numpy arrays"""
    N, k = kps.shape[:2]
    M = N if ids is None else len(ids)
    L = _lib.lib()
    nbytes = L.ipoke_posture_nn_workspace_bytes(N, k, M)
    assert nbytes == grid_of(N, k, M)[1] * M * 24
    bufs = dict(kps=Guarded(kps.shape, torch.float32, kps), vid=Guarded((N,), torch.int32, vid.astype(np.int32)),
                nn_general=Guarded((M,), torch.int64), nn_other=Guarded((M,), torch.int64), ws=Guarded((nbytes,), torch.uint8))
    if ids is not None:
        bufs["ids"] = Guarded((M,), torch.int64, np.asarray(ids, dtype=np.int64))
    if want_dist:
        bufs["dist"] = Guarded((M, 2), torch.float32)
    check(L.ipoke_posture_nn(ptr(bufs["kps"].t), ptr(bufs["vid"].t), ptr(bufs["ids"].t) if ids is not None else None, N, k, M,
                             ptr(bufs["nn_general"].t), ptr(bufs["nn_other"].t), ptr(bufs["dist"].t) if want_dist else None, ptr(bufs["ws"].t),
                             _lib.current_stream()))
    _intact(bufs)
    assert np.array_equal(bufs["kps"].t.cpu().numpy(), kps)
    return (bufs["nn_general"].t.cpu().numpy(), bufs["nn_other"].t.cpu().numpy(), bufs["dist"].t.cpu().numpy() if want_dist else None)


# ------------------------------------------------------------------------------------------------ posture nearest neighbours, exact
EXACT = [  # N, K, M, videos, ids
    (2, 1, 2, 2, None),
    (3, K, 3, 2, None),
    (257, K, 257, 2, None),
    (257, K, 257, 40, None),
    (5003, K, 64, 40, "mixed"),
    (5003, 64, 7, 40, "spread"),
]


def _ids(kind, N, M):
    if kind is None:
        return None
    if kind == "mixed":                                       # unsorted, repeated, the designed frames among them
        base = [N - 2, 3, N // 2, 30, 10, 7, 9, 11, 3, 0, N - 1, 30]
        rest = np.random.RandomState(5).randint(0, N, M - len(base)).tolist()
        return np.array(base + rest, dtype=np.int64)
    return np.array([10, N - 1, 3, N // 2, 30, 4000, 10][:M], dtype=np.int64)


@pytest.mark.parametrize("N,k,M,n_vid,ids_kind", EXACT)
def test_exact_cases_equal_the_restatement_for_every_query(N, k, M, n_vid, ids_kind):
    kps, vid = E.exact_case(N, k, n_vid, seed=N + k)
    ids = _ids(ids_kind, N, M)
    qblocks, chunks, chunk_len, tile = grid_of(N, k, M)
    assert N % tile != 0                                      # the last tile is ragged
    if N > 64:
        assert chunks >= 3 and (chunks - 1) * chunk_len < N   # several candidate chunks, the last one not empty
    if M > 256:
        assert qblocks == 2
    got_g, got_o, dist = posture_nn_guarded(kps, vid, ids)
    want_g, want_o = E.posture_nn(kps, vid, ids)
    assert np.array_equal(got_g, want_g), np.flatnonzero(got_g != want_g)[:8]
    assert np.array_equal(got_o, want_o), np.flatnonzero(got_o != want_o)[:8]
    q = np.arange(N) if ids is None else ids
    for m in range(0, M, max(1, M // 16)):                    # the distances are exact integers
        D = E.posture_dist(kps, int(q[m]))
        assert dist[m, 0] == D[want_g[m]] and dist[m, 1] == D[want_o[m]]
    if N >= 64 and ids_kind is None:
        assert got_g[3] == N // 2 and got_g[N // 2] == N // 2 and got_g[[7, 9, 11]].tolist() == [9, 9, 9] and got_g[30] == 20
        assert got_o[10] == N - 1 and N - 1 >= (chunks - 1) * chunk_len
    # the public wrapper is the same launch
    pub = data.posture_nearest_neighbours(kps, vid, ids, return_dist=True)
    assert np.array_equal(pub[0], got_g) and np.array_equal(pub[1], got_o) and np.array_equal(pub[2], dist)
    assert pub[0].dtype == pub[1].dtype == np.int64


def test_one_video_gives_minus_one_and_the_wrapper_raises():
    kps, _ = E.exact_case(257, K, 1, seed=9)
    vid = np.zeros(257, dtype=np.int64)
    got_g, got_o, dist = posture_nn_guarded(kps, vid)
    assert np.array_equal(got_g, E.posture_nn(kps, vid)[0]) and (got_o == -1).all() and np.isinf(dist[:, 1]).all()
    with pytest.raises(ValueError, match=r"query 0 \(frame 0, video 0\): no frame of another video"):
        data.posture_nearest_neighbours(kps, vid)
    # string labels and chosen queries: the first query is named with its frame and its video
    with pytest.raises(ValueError, match=r"query 0 \(frame 5, video 'b'\)"):
        data.posture_nearest_neighbours(kps.astype(np.float64), np.array(["b"] * 257), ids=np.array([5, 6, 5]))


def test_string_videos_and_float64_keypoints_through_the_wrapper():
    kps, vid = E.exact_case(257, K, 2, seed=274)
    names = np.where(vid == 0, "walk_a", "turn_b")
    a = data.posture_nearest_neighbours(kps.astype(np.float64), names)
    b = data.posture_nearest_neighbours(torch.from_numpy(kps), torch.from_numpy(vid))
    want = E.posture_nn(kps, vid)
    assert all(np.array_equal(x, w) and np.array_equal(y, w) for x, y, w in zip(a, b, want))


# ------------------------------------------------------------------------------------------------ posture nearest neighbours, real values
_REAL = {}


def _real():
    """the float64 truth of the real case, computed once: per query the two answers, the tolerance, their gaps and distances"""
    if not _REAL:
        kps, vid = E.real_case()
        _REAL.update(kps=kps, vid=vid, rows=np.array([E.posture_truth(kps, vid, i) for i in range(len(kps))]))
    return _REAL


def test_real_case_within_the_fp32_bound():
    r = _real()
    kps, vid, rows = r["kps"], r["vid"], r["rows"]
    N = len(kps)
    assert grid_of(N, K, N)[0] == 12 and grid_of(N, K, N)[1] >= 3
    got_g, got_o, dist = posture_nn_guarded(kps, vid)
    lacking, worst_units, other_index = 0, 0.0, 0
    for i in range(N):
        want_g, want_o, tol, gap_g, gap_o, d_g, d_o, d_max = rows[i]
        dg, do = d_g, d_o                                     # float64 distances of the returned frames
        if got_g[i] != int(want_g) or got_o[i] != int(want_o):
            D = E.posture_dist(kps, i)
            dg, do = D[got_g[i]], D[got_o[i]]
            other_index += 1
        assert dg <= d_g + tol and do <= d_o + tol, i
        assert vid[got_o[i]] != vid[i] and got_g[i] != i
        if gap_g > 2 * tol:
            assert got_g[i] == int(want_g), i
        if gap_o > 2 * tol:
            assert got_o[i] == int(want_o), i
        lacking += min(gap_g, gap_o) <= 2 * tol
        err = max(abs(float(dist[i, 0]) - dg), abs(float(dist[i, 1]) - do))
        assert err <= tol, (i, err, tol)
        worst_units = max(worst_units, err / (E.EPS32 * d_max))
    print(f"posture nn, N = {N}: worst distance error {worst_units:.2f} x 2^-24 D_max; {lacking} queries lack the 2 tol gap, "
          f"{other_index} returned another index than the float64 order")
    assert lacking <= 0.01 * N


def test_golden_nn_other_vid_equals_the_reference(golden):
    g = golden("g21_keypoints")
    got_g, got_o = data.posture_nearest_neighbours(g["nn_kps"], g["nn_vid"])
    assert np.array_equal(got_o, g["nn_other_vid"])
    assert np.array_equal(got_g, E.posture_nn(g["nn_kps"], g["nn_vid"])[0])


def test_two_runs_are_bit_identical():
    r = _real()
    a = posture_nn_guarded(r["kps"], r["vid"])
    b = posture_nn_guarded(r["kps"], r["vid"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    kps, vid = E.exact_case(5003, 64, 40, seed=1)
    ids = np.arange(0, 5003, 79, dtype=np.int64)
    a, b = posture_nn_guarded(kps, vid, ids), posture_nn_guarded(kps, vid, ids)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ keypoint pokes
def _kp_cases(g):
    for ci in range(int(g["kp_n_cases"])):
        size, ps, fix, n_pokes, seed = (int(v) for v in g[f"kp_meta{ci}"])
        yield dict(ci=ci, size=size, ps=ps, fix=bool(fix), n_pokes=n_pokes, seed=seed, src=g[f"kp_src{ci}"], tgt=g[f"kp_tgt{ci}"],
                   poke=g[f"kp_poke{ci}"], coords=g[f"kp_coords{ci}"], ids=g[f"kp_ids{ci}"])


def _sim(size, ps, n_pokes=5, fix=False):
    return PokeSimulator({"spatial_size": (size, size), "n_pokes": n_pokes, "poke_size": ps, "fix_n_pokes": fix, "scale_poke_to_res": True})


def keypoint_poke_guarded(sim, src, tgt, ids):
    B, k, _ = src.shape
    n_max = ids.shape[1]
    H, W = sim.spatial_size
    bufs = dict(src=Guarded(src.shape, torch.float64, src), tgt=Guarded(tgt.shape, torch.float64, tgt), ids=Guarded(ids.shape, torch.int32, ids),
                poke=Guarded((B, 2, H, W), torch.float32), coords=Guarded((B, n_max, 2), torch.int32))
    check(_lib.lib().ipoke_keypoint_poke(ptr(bufs["src"].t), ptr(bufs["tgt"].t), ptr(bufs["ids"].t), B, k, n_max, H, W, sim.poke_size // 2,
                                         sim.valid_h[0], sim.valid_h[1], sim.valid_w[0], sim.valid_w[1], ptr(bufs["poke"].t), ptr(bufs["coords"].t),
                                         _lib.current_stream()))
    _intact(bufs)
    return bufs["poke"].t.cpu().numpy(), bufs["coords"].t.cpu().numpy()


def test_keypoint_pokes_are_bit_equal_to_the_golden(golden):
    g = golden("g21_keypoints")
    for c in _kp_cases(g):
        sim = _sim(c["size"], c["ps"], c["n_pokes"], c["fix"])
        ids = sim.draw_keypoint_ids(1, K, np.random.RandomState(c["seed"]))
        assert np.array_equal(ids[0], c["ids"])
        poke, coords = keypoint_poke_guarded(sim, c["src"][None], c["tgt"][None], ids)
        assert np.array_equal(poke[0], c["poke"]), c["ci"]
        assert np.array_equal(coords[0], c["coords"]), c["ci"]
        pub = sim.keypoint_poke(c["src"][None], c["tgt"][None], ids)
        assert isinstance(pub, list) and len(pub) == 3 and pub[0].dtype == torch.float32 and pub[1].dtype == pub[2].dtype == torch.int32
        assert np.array_equal(pub[0].cpu().numpy(), poke) and np.array_equal(pub[1].cpu().numpy(), coords)
        assert np.array_equal(pub[2].cpu().numpy()[0], c["ids"])


def test_keypoint_pokes_batched_equal_per_sample(golden):
    g = golden("g21_keypoints")
    cases = [c for c in _kp_cases(g) if (c["size"], c["fix"]) == (128, False)]
    sim = _sim(128, 10)
    src, tgt, ids = (np.stack([c[k] for c in cases]) for k in ("src", "tgt", "ids"))
    poke, coords = keypoint_poke_guarded(sim, src, tgt, ids)
    for b, c in enumerate(cases):
        assert np.array_equal(poke[b], c["poke"]) and np.array_equal(coords[b], c["coords"]), c["ci"]
    want = E.keypoint_poke(src, tgt, ids, (128, 128), 10)
    assert np.array_equal(poke, want[0]) and np.array_equal(coords, want[1])
    with pytest.raises(ValueError, match="outside"):
        sim.keypoint_poke(src, tgt, np.full_like(ids, K))


def _model():
    arch = configs.flow_arch(32, hidden=64, num_steps=[2, 1, 1], factor=4)
    arch["flow_mid_channels_factor"] = 2
    conf = configs.second_stage_config(64, 32, 16, batch_size=2, arch=arch)
    model = PokeMotionModel(conf, dirs={}, dtype="f32", device=DEV, max_batch=2)
    for name in ("first_stage_model", "poke_embedder", "conditioner", "flow"):
        deterministic_fill_(getattr(model, name), prefix=name + ".")
    model.flow.sync_buffers()
    return model


def test_make_batch_keypoint_poke_feeds_the_sampler(golden):
    """make_batch(keypoints=) -> sample_videos_device(use_keypoint_pokes=True) equals handing the same poke over as the ordinary poke"""
    g = golden("g21_keypoints")
    cases = [c for c in _kp_cases(g) if (c["size"], c["fix"]) == (64, False)][:2]
    sim = _sim(64, 5)
    src, tgt, ids = (np.stack([c[k] for c in cases]) for k in ("src", "tgt", "ids"))
    images = synthetic_batch(2, 16, 64, seed=3, device=DEV)["images"]
    gen = torch.Generator(device=DEV).manual_seed(4)
    coarse = torch.randn(2, 2, 6, 6, device=DEV, generator=gen)
    raw = torch.nn.functional.interpolate(coarse, size=(96, 96), mode="bicubic", align_corners=False) * 10
    u = torch.rand(2, 11, device=DEV, generator=gen)
    plain = sim.make_batch(images, raw, u=u)
    assert set(plain) == {"images", "flow", "poke", "poke_status"}                                  # without the argument: the dict it was
    batch = sim.make_batch(images, raw, u=u, keypoints=(src, tgt), keypoint_ids=ids)
    assert set(batch) == set(plain) | {"keypoint_poke"} and torch.equal(batch["poke"][0], plain["poke"][0])
    kp_poke, kp_coords, kp_ids = batch["keypoint_poke"]
    for b, c in enumerate(cases):
        assert np.array_equal(kp_poke[b].cpu().numpy(), c["poke"]) and np.array_equal(kp_coords[b].cpu().numpy(), c["coords"])
    assert kp_poke.abs().max().item() > 0 and not torch.equal(kp_poke, batch["poke"][0])
    drawn = sim.make_batch(images, raw, u=u, keypoints=(src, tgt), rng=np.random.RandomState(12))["keypoint_poke"][2]
    assert np.array_equal(drawn.cpu().numpy(), sim.draw_keypoint_ids(2, K, np.random.RandomState(12)))
    model = _model()
    torch.manual_seed(21)
    got = model.sample_videos_device(batch, n_samples=2, n_logged_vids=2, use_keypoint_pokes=True)
    torch.manual_seed(21)
    # the ordinary poke is batch[model.poke_key]: the flow entry for a flow_ae poke embedder (the default config), else the poke entry
    as_poke = kp_poke if model.poke_key == "flow" else [kp_poke, batch["poke"][1]]
    want = model.sample_videos_device({**batch, model.poke_key: as_poke}, n_samples=2, n_logged_vids=2)
    torch.manual_seed(21)
    other = model.sample_videos_device(batch, n_samples=2, n_logged_vids=2)
    assert got.shape == (2, 2, 15, 3, 64, 64) and torch.equal(got, want) and not torch.equal(got, other)


# ------------------------------------------------------------------------------------------------ KPSMetric
def kps_frame_mse_guarded(pred, target):
    bs, ns, s, k, _ = pred.shape
    bufs = dict(pred=Guarded(pred.shape, torch.float32, pred), target=Guarded(target.shape, torch.float32, target), out=Guarded((bs, ns, s), torch.float32))
    check(_lib.lib().ipoke_kps_frame_mse(ptr(bufs["pred"].t), ptr(bufs["target"].t), bs, ns, s, k, ptr(bufs["out"].t), _lib.current_stream()))
    _intact(bufs)
    return bufs["out"].t.cpu().numpy()


@pytest.mark.parametrize("bs,ns,s,k", [(1, 1, 1, 1), (2, 5, 4, 17), (3, 7, 300, 16)])
def test_kps_frame_mse_is_exact_on_integers(bs, ns, s, k):
    rs = np.random.RandomState(bs + ns + s + k)
    pred = rs.randint(-40, 41, (bs, ns, s, k, 2)).astype(np.float32)
    target = rs.randint(-40, 41, (bs, 1, s, k, 2)).astype(np.float32)
    want = E.kps_frame_mse(pred, target)
    assert (want * 2 * k).max() < 2 ** 24
    got = kps_frame_mse_guarded(pred, target)
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(metrics.kps_frame_mse(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV)).cpu().numpy(), got)


def test_kps_frame_mse_on_real_operands():
    rs = np.random.RandomState(3)
    bs, ns, s, k = 3, 6, 65, 17
    target = rs.rand(bs, 1, s, k, 2).astype(np.float32)
    pred = (target + 0.1 * rs.randn(bs, ns, s, k, 2)).astype(np.float32)
    want = E.kps_frame_mse(pred, target)
    got = kps_frame_mse_guarded(pred, target).astype(np.float64)
    bound = (2 * k + 2) * E.EPS32 * want.max()
    err = np.abs(got - want).max()
    print(f"kps frame mse: max abs err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_kps_metric_matches_the_golden(golden):
    g = golden("g21_keypoints")
    m = metrics.KPSMetric(1000)
    for u in range(2):
        m.update(torch.from_numpy(g[f"kps_pred{u}"]).to(DEV), torch.from_numpy(g[f"kps_target{u}"]).to(DEV))
    d = m.compute(n_pokes=3)
    assert list(d) == ["NN MSE", "Mean MSE per Frame", "Std per Frame", "Time", "Number of Pokes"]
    for key in ("NN MSE", "Mean MSE per Frame", "Std per Frame"):
        np.testing.assert_allclose(d[key], g["kps_out_" + key.replace(" ", "_")], atol=1e-6, rtol=0)
    assert np.array_equal(d["Time"], g["kps_out_Time"]) and np.array_equal(d["Number of Pokes"], g["kps_out_Number_of_Pokes"])
    assert abs(float(m.nn_err) - float(g["kps_nn_err"])) <= 1e-6 and m.n_samples == 4
