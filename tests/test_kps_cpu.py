"""CPU side of the keypoint path: the float64 restatement of tests/kps_exact.py against golden G21 (the reference's own get_nn,
_get_keypoint_poke and KPSMetric, written by scripts/make_goldens_keypoints.py), the C symbols and their argument checks, the draws of
``PokeSimulator.draw_keypoint_ids``, the host logic of ``metrics.KPSMetric`` on the restatement, and the input conditions the GPU tests
(tests/test_kps_gpu.py) rely on for the seeds they use."""
import ctypes

import numpy as np
import pytest
import torch

from ipoke_amd import _lib, metrics
from ipoke_amd.data import PokeSimulator
from tests import kps_exact as E

K = 17


def _kp_cases(g):
    for ci in range(int(g["kp_n_cases"])):
        size, ps, fix, n_pokes, seed = (int(v) for v in g[f"kp_meta{ci}"])
        yield dict(ci=ci, size=size, ps=ps, fix=bool(fix), n_pokes=n_pokes, seed=seed, src=g[f"kp_src{ci}"], tgt=g[f"kp_tgt{ci}"],
                   poke=g[f"kp_poke{ci}"], coords=g[f"kp_coords{ci}"], ids=g[f"kp_ids{ci}"])


def _sim(c):
    return PokeSimulator({"spatial_size": (c["size"], c["size"]), "n_pokes": c["n_pokes"], "poke_size": c["ps"], "fix_n_pokes": c["fix"]})


# ------------------------------------------------------------------------------------------------ the restatement against the golden
def test_posture_restatement_equals_the_reference(golden):
    g = golden("g21_keypoints")
    kps, vid = g["nn_kps"], g["nn_vid"]
    assert kps.shape == (600, K, 2) and kps.dtype == np.float32 and len(np.unique(vid)) == 12
    nn_general, nn_other = E.posture_nn(kps, vid)
    assert np.array_equal(nn_other, g["nn_other_vid"])
    assert (nn_general != np.arange(600)).all() and (vid[nn_other] != vid).all()
    # the golden's own condition: every decisive gap clears twice the tolerance
    low = min(min(gg - 2 * tol, go - 2 * tol) for tol, gg, go in (E.posture_gaps(kps, vid, i) for i in range(600)))
    assert low > 0 and abs(low - float(g["nn_margin"])) <= 1e-12


def test_keypoint_poke_restatement_equals_the_reference(golden):
    g = golden("g21_keypoints")
    sizes, fixed, edge_drawn, edge_left_out, below = set(), 0, 0, 0, 0
    for c in _kp_cases(g):
        n = int((c["ids"] >= 0).sum())
        poke, coords, ids = E.keypoint_poke_one(c["src"], c["tgt"], c["ids"][:n], (c["size"], c["size"]), c["ps"], c["n_pokes"])
        assert np.array_equal(poke.astype(np.float32), c["poke"]) and np.array_equal(coords, c["coords"]) and np.array_equal(ids, c["ids"]), c["ci"]
        sizes.add((c["size"], c["ps"]))
        fixed += c["fix"]
        lo, hi = c["ps"], c["size"] - c["ps"]
        for j in range(n):
            row, col = c["coords"][j]
            inside = lo <= row <= hi and lo <= col <= hi
            drawn = bool(c["poke"][:, row, col].any())
            assert drawn == inside or not inside, (c["ci"], j)
            if c["ids"][j] < 8:
                edge_drawn += inside
                edge_left_out += not inside
            if c["ids"][j] == 8:                                 # the product just below an integer truncates down in double, not in fp32
                cc = c["size"] // 2 + 3
                assert col == cc - 1 and int(np.float32(c["src"][8, 0]) * np.float32(c["size"])) == cc
                assert 0 < cc - c["src"][8, 0] * c["size"] < 1e-12
                below += 1
    assert sizes == {(64, 5), (128, 10)} and fixed == 12 and edge_drawn >= 48 and edge_left_out >= 48 and below >= 12


def test_kps_metric_restatement_equals_the_reference(golden):
    g = golden("g21_keypoints")
    m = E.KPSMetricRef(1000)
    for u in range(2):
        assert g[f"kps_pred{u}"].shape == (2, 5, 4, K, 2) and g[f"kps_target{u}"].shape == (2, 1, 4, K, 2)
        m.update(g[f"kps_pred{u}"], g[f"kps_target{u}"])
    d = m.compute(n_pokes=3)
    assert list(d) == ["NN MSE", "Mean MSE per Frame", "Std per Frame", "Time", "Number of Pokes"]
    for key in ("NN MSE", "Mean MSE per Frame", "Std per Frame"):
        np.testing.assert_allclose(d[key], g["kps_out_" + key.replace(" ", "_")], atol=1e-6, rtol=0)
    assert np.array_equal(d["Time"], g["kps_out_Time"]) and np.array_equal(d["Number of Pokes"], g["kps_out_Number_of_Pokes"])
    assert abs(m.nn_err - float(g["kps_nn_err"])) <= 1e-6 and m.n_samples == int(g["kps_n_samples"]) == 4
    assert float(g["kps_margin"]) > 1e-4


# ------------------------------------------------------------------------------------------------ symbols and argument checks
def test_symbols_exist_and_bad_arguments_return_minus_one():
    L = _lib.lib()
    for name in ("ipoke_posture_nn_workspace_bytes", "ipoke_posture_nn", "ipoke_posture_nn_grid", "ipoke_keypoint_poke", "ipoke_kps_frame_mse"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf))                # a host address: every call below must return before any launch
    assert L.ipoke_posture_nn(None, p, None, 8, K, 8, p, p, None, p, None) == -1
    assert L.ipoke_posture_nn(p, None, None, 8, K, 8, p, p, None, p, None) == -1
    assert L.ipoke_posture_nn(p, p, None, 8, K, 8, None, p, None, p, None) == -1
    assert L.ipoke_posture_nn(p, p, None, 8, K, 8, p, None, None, p, None) == -1
    assert L.ipoke_posture_nn(p, p, None, 8, K, 8, p, p, None, None, None) == -1
    assert L.ipoke_posture_nn(p, p, None, 1, K, 1, p, p, None, p, None) == -1                    # N < 2
    assert L.ipoke_posture_nn(p, p, None, 8, 0, 8, p, p, None, p, None) == -1                    # K outside 1 .. 64
    assert L.ipoke_posture_nn(p, p, None, 8, 65, 8, p, p, None, p, None) == -1
    assert L.ipoke_posture_nn(p, p, None, 8, K, 0, p, p, None, p, None) == -1
    assert b"K" in L.ipoke_last_error() or b"M" in L.ipoke_last_error()
    assert L.ipoke_posture_nn_workspace_bytes(8, 65, 8) == 0 and L.ipoke_posture_nn_workspace_bytes(1, K, 1) == 0
    assert L.ipoke_keypoint_poke(None, p, p, 1, K, 5, 64, 64, 2, 5, 59, 5, 59, p, p, None) == -1
    assert L.ipoke_keypoint_poke(p, p, p, 1, K, 5, 64, 64, 2, 5, 59, 5, 59, None, p, None) == -1
    assert L.ipoke_keypoint_poke(p, p, p, 1, K, 5, 64, 64, 2, 5, 59, 5, 59, p, None, None) == -1
    assert L.ipoke_kps_frame_mse(None, p, 1, 1, 1, K, p, None) == -1
    assert L.ipoke_kps_frame_mse(p, p, 1, 1, 1, K, None, None) == -1
    assert L.ipoke_kps_frame_mse(p, p, 1, 0, 1, K, p, None) == -1


def test_grid_query_gives_chunks_and_a_ragged_tile():
    """the shapes the GPU test uses: several candidate chunks and a last tile that is not full"""
    L = _lib.lib()
    out = (ctypes.c_int32 * 4)()
    for N, k, M, several in ((2, 1, 2, False), (3, K, 3, False), (257, K, 257, True), (5003, K, 64, True), (5003, 64, 7, True), (3001, K, 3001, True)):
        assert L.ipoke_posture_nn_grid(N, k, M, out) == 0
        qblocks, chunks, chunk_len, tile = list(out)
        assert qblocks == -(-M // 256) and chunk_len % tile == 0 and (chunks - 1) * chunk_len < N <= chunks * chunk_len
        assert N % tile != 0                                                  # ragged last tile
        assert (chunks > 1) == several
        assert L.ipoke_posture_nn_workspace_bytes(N, k, M) == chunks * M * 24


def test_python_wrappers_validate_on_the_host(monkeypatch):
    from ipoke_amd import data
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    kps = np.zeros((4, 3, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="outside"):
        data.posture_nearest_neighbours(kps, np.arange(4), ids=np.array([0, 4]))
    with pytest.raises(ValueError, match="outside"):
        data.posture_nearest_neighbours(kps, np.arange(4), ids=np.array([-1]))
    with pytest.raises(ValueError, match="K <= 64"):
        data.posture_nearest_neighbours(np.zeros((4, 65, 2)), np.arange(4))
    with pytest.raises(ValueError, match="N >= 2"):
        data.posture_nearest_neighbours(kps[:1], np.arange(1))
    with pytest.raises(ValueError, match="non-finite"):
        data.posture_nearest_neighbours(np.full((4, 3, 2), np.nan), np.arange(4))
    with pytest.raises(ValueError, match="vid"):
        data.posture_nearest_neighbours(kps, np.zeros(4))                      # float video labels


# ------------------------------------------------------------------------------------------------ host logic
def test_draw_keypoint_ids_makes_the_reference_draws(golden):
    g = golden("g21_keypoints")
    counts = set()
    for c in _kp_cases(g):
        ids = _sim(c).draw_keypoint_ids(1, K, np.random.RandomState(c["seed"]))
        assert ids.dtype == np.int32 and ids.shape == (1, c["n_pokes"]) and np.array_equal(ids[0], c["ids"]), c["ci"]
        assert np.array_equal(E.draw_keypoint_ids(1, K, c["n_pokes"], c["fix"], np.random.RandomState(c["seed"])), ids)
        counts.add((c["fix"], int((ids >= 0).sum())))
    assert {n for f, n in counts if f} == {K} and len({n for f, n in counts if not f}) >= 2
    # a batch draws sample after sample from one stream
    sim = PokeSimulator({"spatial_size": (64, 64), "n_pokes": 5, "poke_size": 5})
    a = sim.draw_keypoint_ids(3, K, np.random.RandomState(4))
    rs = np.random.RandomState(4)
    for b in range(3):
        n = int(rs.randint(1, 5, 1)[0])
        assert np.array_equal(a[b, :n], rs.choice(K, n, replace=False)) and (a[b, n:] == -1).all()


def test_kps_metric_keys_and_example_count_guard(golden, monkeypatch):
    """Host logic of KPSMetric with the two kernels replaced by their restatements: the reference's dict, its running state and its guard
    -- the number of processed EXAMPLES is compared with n_samples, so updates stop silently after that many."""
    g = golden("g21_keypoints")
    monkeypatch.setattr(metrics, "kps_frame_mse", lambda p, t_: torch.from_numpy(E.kps_frame_mse(p.numpy(), t_.numpy())))
    monkeypatch.setattr(metrics, "sample_stats", lambda v: tuple(torch.from_numpy(np.asarray(a)) for a in E.sample_stats(v.numpy())))
    updates = [(torch.from_numpy(g[f"kps_pred{u}"]), torch.from_numpy(g[f"kps_target{u}"])) for u in range(2)]
    m = metrics.KPSMetric(1000)
    for pred, target in updates:
        m.update(pred, target)
    d = m.compute(n_pokes=3)
    assert list(d) == ["NN MSE", "Mean MSE per Frame", "Std per Frame", "Time", "Number of Pokes"]
    for key in ("NN MSE", "Mean MSE per Frame", "Std per Frame"):
        np.testing.assert_allclose(d[key], g["kps_out_" + key.replace(" ", "_")], atol=1e-6, rtol=0)
    assert d["Time"].tolist() == [0, 1, 2, 3] and d["Number of Pokes"].tolist() == [3] * 4 and d["Number of Pokes"].dtype.kind == "i"
    assert m.compute()["Number of Pokes"].tolist() == [0] * 4                      # the reference's default n_pokes=0
    assert abs(float(m.nn_err) - float(g["kps_nn_err"])) <= 1e-6 and m.n_samples == 4
    m = metrics.KPSMetric(3)
    m.update(*updates[0])                                      # 0 < 3: taken
    m.update(*updates[1])                                      # 2 < 3: taken, now 4 examples
    m.update(*updates[0])                                      # 4 >= 3: silently ignored
    assert m.n_samples == 4 and len(m.nn_err_per_frame) == len(m.std_per_frame) == len(m.mean_per_frame) == 2
    m.reset()
    assert m.n_samples == 0 and m.nn_err_per_frame == [] and m.nn_err is None


# ------------------------------------------------------------------------------------------------ conditions of the GPU cases
def test_real_case_meets_its_gap_condition():
    """N = 3001, K = 17 on seed 0, ALL queries and both answers: at most 1 % may lack a float64 gap of 2 tol to the runner-up, and the fp32
    emulation of the kernel's arithmetic stays inside tol.  Measured here: one query of the 3001 lacks the gap (8.7e-6 between the two
    nearest candidates of one answer, against 2 tol of at most 7.0e-5); on every 7th query alone the smallest gap is far above 2 tol.
    For that one query the GPU test holds the returned index to the distance bound only, as it does wherever the gap is missing."""
    kps, vid = E.real_case()
    lacking, smallest, worst_units, two_tol = 0, np.inf, 0.0, 0.0
    for i in range(len(kps)):
        tol, gap_g, gap_o = E.posture_gaps(kps, vid, i)
        lacking += min(gap_g, gap_o) <= 2 * tol
        smallest = min(smallest, gap_g, gap_o)
        two_tol = max(two_tol, 2 * tol)
        if i % 7 == 0:
            D = E.posture_dist(kps, i)
            err = np.abs(E.posture_dist_fp32(kps, i).astype(np.float64) - D).max()
            assert err <= tol
            worst_units = max(worst_units, err / (E.EPS32 * D.max()))
    print(f"smallest gap {smallest:.3e}, largest 2 tol {two_tol:.3e}, {lacking} queries lack the gap; fp32 emulation: worst error "
          f"{worst_units:.2f} x 2^-24 D_max")
    assert lacking <= 0.01 * len(kps)


def test_exact_cases_are_exact_in_fp32():
    """the integer construction of the GPU test: y fixed per keypoint slot, so every term is an integer |dx| and every sum is below 2^24"""
    for N, k, n_vid in ((257, K, 2), (5003, 64, 40)):
        kps, vid = E.exact_case(N, k, n_vid, seed=N + k)
        g, o = E.posture_nn(kps, vid, [3, N // 2, 7, 9, 11, 30, 10])
        # the duplicates (the second entry of 3 = N // 2 and of 7 = 9 = 11, whoever asks), the tie and the far neighbour
        assert g.tolist()[:6] == [N // 2, N // 2, 9, 9, 9, 20] and o[6] == N - 1
        for i in (0, N // 2, N - 1):
            D = E.posture_dist(kps, i)
            assert np.array_equal(D, np.round(D)) and D.max() < 2 ** 24
            assert np.array_equal(E.posture_dist_fp32(kps, i).astype(np.float64), D)
