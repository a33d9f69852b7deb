"""CPU side of the test loop (reference second_stage_video.py:665-752, 1037-1155): the restatements of tests/eval_ref.py against golden
g17_test_modes (outputs of the reference's own SampleMetric / compute_div_score_mse / compute_div_score), the errors ``test_step`` raises
for what is not built, and the host logic of ``SampleSSIM``."""
import numpy as np
import pytest
import torch

from ipoke_amd import configs, metrics
from ipoke_amd.second_stage import PokeMotionModel
from tests import eval_ref
from tests.conftest import t
from tests.helpers import synthetic_batch

CASES = ("a", "b")


@pytest.mark.parametrize("tag", CASES)
def test_sample_ssim_restatement_against_golden(golden, tag):
    g = golden("g17_test_modes")
    vals = eval_ref.sample_ssim(t(g[f"{tag}_pred"]), t(g[f"{tag}_target"]))
    assert torch.equal(vals, t(g[f"{tag}_ssim_vals"]))                     # the same torch ops in the same order as the reference's loop
    nn, sd, mean, idx = eval_ref.sample_stats(vals)
    assert torch.equal(idx.int(), t(g[f"{tag}_ssim_argmin"]))
    for got, key in ((nn, "nn"), (sd, "std"), (mean, "mean")):
        assert torch.equal(got, t(g[f"{tag}_ssim_{key}"])), key
    # the golden's own condition: arg-min gaps of at least 100 x the GPU tests' SSIM bound
    means = vals.mean(-1).sort(dim=1).values
    assert (means[:, 1:] - means[:, :-1]).min().item() >= 100 * 2e-5


@pytest.mark.parametrize("tag", CASES)
def test_diversity_restatements_against_golden(golden, tag):
    g = golden("g17_test_modes")
    pred = t(g[f"{tag}_pred"])
    mse = eval_ref.offdiag_mean(eval_ref.pair_mse(pred))
    assert abs(mse - float(g[f"{tag}_div_mse"])) <= 1e-6 * float(g[f"{tag}_div_mse"])      # float64 restatement vs the reference's fp32 means
    torch.set_num_threads(1)
    score, D = eval_ref.div_score(pred, eval_ref.Vgg16Taps(eval_ref.filled_vgg16()).eval())
    assert abs(score - float(g[f"{tag}_div_vgg"])) <= 1e-6
    assert D.shape == (pred.shape[0], 5, pred.shape[1], pred.shape[1])


def test_ssim_map_is_the_scipy_checked_restatement_without_its_mean(golden):
    """``eval_ref.ssim_map`` (the stand-in behind the golden's SSIM values and the GPU tests' yardstick) averaged over everything is
    oracle/metrics_ref.ssim, the restatement tests/test_metrics_cpu.py holds against an independent scipy formulation."""
    from oracle import metrics_ref
    g = golden("g17_test_modes")
    p, tg = t(g["a_pred"])[0].reshape(-1, 3, 32, 32), t(g["a_target"])[0].repeat(3, 1, 1, 1, 1).reshape(-1, 3, 32, 32)
    m = eval_ref.ssim_map(p, tg)
    assert m.shape == (12, 3, 22, 22) and torch.equal(m.mean(), metrics_ref.ssim(p, tg))
    x = torch.rand(2, 1, 11, 13, generator=torch.Generator().manual_seed(1))
    assert torch.equal(eval_ref.ssim_map(x, x * 0.5).mean(), metrics_ref.ssim(x, x * 0.5))


def test_uint8_restatement_truncates():
    x = torch.tensor([-1.0, -0.9961, 0.0, 0.5, 0.99999, 1.0]).view(1, 1, 1, 1, 6).expand(1, 1, 3, 1, 6)
    assert eval_ref.video_to_uint8(x)[0, 0, 0, :, 0].tolist() == [0, 0, 127, 191, 254, 255]


def _model(test_mode, **testing):
    arch = configs.flow_arch(32, hidden=64, num_steps=[2, 1, 1], factor=4)
    arch["flow_mid_channels_factor"] = 2
    conf = configs.second_stage_config(64, 32, 16, batch_size=2, arch=arch)
    conf["general"]["test"] = test_mode
    conf["testing"].update(testing)
    return PokeMotionModel(conf, dirs={}, dtype="f32", device="cpu", max_batch=2)


@pytest.mark.parametrize("mode,needs", [("samples", "cv2"), ("kps_acc", "HRNet"), ("control_sensitivity", "HRNet"), ("transfer", "cv2")])
def test_unsupported_test_modes_name_what_is_missing(mode, needs):
    m = _model(mode)
    with pytest.raises(NotImplementedError, match=needs):
        m.test_step({"images": torch.zeros(1, 16, 3, 64, 64)}, 0)


def test_unknown_test_mode_raises_the_reference_error():
    m = _model("none")
    with pytest.raises(ValueError, match='The specified test_mode is "none", which is invalid'):
        m.test_step({"images": torch.zeros(1, 16, 3, 64, 64)}, 0)
    assert m.test_step_end("x") == "x"


def test_unsupported_terms_of_supported_modes():
    batch = {"images": torch.zeros(1, 16, 3, 64, 64)}
    with pytest.raises(NotImplementedError, match="HRNet"):
        _model("diversity", div_kp=True).test_step(batch, 0)
    with pytest.raises(NotImplementedError, match="lpips"):
        _model("diversity", lpips=True).test_step(batch, 0)
    with pytest.raises(NotImplementedError, match="lpips"):
        _model("accuracy", lpips=True).test_step(batch, 0)
    with pytest.raises(NotImplementedError, match="HRNet"):
        _model("accuracy").test_step(dict(batch, keypoints_rel=torch.zeros(1, 16, 17, 2), keypoints_abs=torch.zeros(1, 16, 17, 2)), 0)
    with pytest.raises(RuntimeError):                         # the supported path itself needs the GPU: no CPU fallback
        _model("diversity").test_step(synthetic_batch(1, 16, 64), 0)


def test_sample_ssim_keys_and_example_count_guard(golden, monkeypatch):
    """Host logic of SampleSSIM with the two kernels replaced by their restatements: the reference's key set, its running value, and its
    guard -- the number of processed EXAMPLES is compared with n_samples_per_data_point, so updates stop silently after that many."""
    g = golden("g17_test_modes")
    monkeypatch.setattr(metrics, "sample_ssim", eval_ref.sample_ssim)
    monkeypatch.setattr(metrics, "sample_stats", eval_ref.sample_stats)
    pred, target = t(g["a_pred"]), t(g["a_target"])
    m = metrics.SampleSSIM(3)
    m.update(pred, target)                                    # 2 examples < 3: taken
    meanval, d = m.compute(n_pokes=5)
    assert set(d) == {"SSIM NN", "Mean SSIM per Frame", "Std per Frame", "Time", "Number of Pokes"}
    assert abs(meanval.item() - float(g["a_ssim_meanval"])) <= 1e-6
    np.testing.assert_allclose(d["SSIM NN"], g["a_ssim_dict_nn"], atol=1e-6)
    np.testing.assert_allclose(d["Mean SSIM per Frame"], g["a_ssim_dict_mean"], atol=1e-6)
    np.testing.assert_allclose(d["Std per Frame"], g["a_ssim_dict_std"], atol=1e-6)
    assert d["Time"].tolist() == [0, 1, 2, 3] and d["Number of Pokes"].tolist() == [5] * 4 and d["Number of Pokes"].dtype.kind == "i"
    assert "Number of Pokes" not in m.compute()[1]
    m.update(pred, target)                                    # 2 < 3: taken, now 4 examples
    m.update(pred, target)                                    # 4 >= 3: silently ignored
    assert m.n_samples == 4 and len(m.nn_val_per_frame) == 2
    m.reset()
    assert m.n_samples == 0 and m.nn_val_per_frame == [] and m.val is None


def test_metric_vgg16_topology():
    from ipoke_amd.vgg import VGG, metric_vgg16
    m = metric_vgg16()
    want = [f"slice{s}.{i}.{p}" for s, ids in ((1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)), (5, (24, 26, 28))) for i in ids
            for p in ("weight", "bias")]
    assert list(m.state_dict()) == want and m.N_slices == 5
    assert [op[0] for op in m.program].count("tap") == 5 and [op[0] for op in m.program].count("pool") == 4
    feats = eval_ref.filled_vgg16()
    m.load_torchvision_features({"features." + k: v for k, v in feats.state_dict().items()})
    assert torch.equal(m.slice3["14"].weight, feats[14].weight) and all(not p.requires_grad for p in m.parameters())
    assert len(VGG().state_dict()) == 26 and "slice5.28.bias" in VGG().state_dict() and "slice2.2.weight" in VGG().state_dict()
    with pytest.raises(NotImplementedError):
        metric_vgg16(pretrained=True)
