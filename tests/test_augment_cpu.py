"""CPU side of the clip augmentation (csrc/data.hip ``ipoke_aug_frame_means`` / ``ipoke_aug_frames`` / ``ipoke_aug_flow``, ``ClipAugmenter``
in ipoke_amd/data.py; reference data/base_dataset.py:695-722, 432-440, 683-691): the numpy restatement of tests/augment_ref.py against golden
G18, which scripts/make_augment_goldens.py computed with Pillow (and, where Pillow imports, against Pillow directly), the host side of
``ClipAugmenter`` -- the 16.16 matrix, the draws, the errors -- and the public surface.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd.data import ClipAugmenter, PokeSimulator
from tests import augment_ref as R

SHIPPED = {"augment": True, "p_col": .8, "p_geom": .8, "augment_b": 0.4, "augment_c": 0.5, "augment_h": 0.15, "augment_s": 0.4, "aug_deg": 15,
           "aug_trans": (0.1, 0.1), "spatial_size": (128, 128)}
SHAPES = [(8, 2, 1), (30, 3, 2), (64, 2, 3), (128, 2, 2), (64, 4, 1)]                     # (S, B, T) of the golden's cases


def case(g, ci):
    return {k: g[f"{k}{ci}"] for k in ("frames", "colour", "hue", "hue_add", "angle", "trans", "affine", "mean_l", "out", "flow", "flow_out")}


def test_golden_holds_the_cases_and_parameter_sets(golden):
    g = golden("g18_augment")
    assert int(g["n_cases"]) == len(SHAPES)
    factors = []
    for ci, (S, B, T) in enumerate(SHAPES):
        c = case(g, ci)
        assert c["frames"].shape == (B, T, S, S, 3) and c["frames"].dtype == np.uint8 and c["out"].dtype == np.uint8
        assert c["flow"].shape == (B, 2, S, S) and c["flow"].dtype == np.float32 and c["flow_out"].dtype == np.float32
        factors.append(c["colour"])
        n_fill = sum(int((~R.source_index(a, S)[0]).sum()) for a in c["affine"])
        if ci < 4:
            assert n_fill > 0 and (np.abs(c["angle"]) > 90).any(), "one large rotation per size, whose fill shows"
    factors = np.concatenate(factors)
    assert (factors > 1).any(0).all() and (factors < 0).any(0)[1:].all()                     # both sides of the blend's clip
    assert any((case(g, ci)["hue"] < 0).any() for ci in range(5))
    lat = case(g, 4)
    colours = {tuple(p) for p in lat["frames"][0, 0].reshape(-1, 3).tolist()}
    assert len(colours) == 4096 and all(v % 17 == 0 for p in colours for v in p)
    # the identity set: factors 1, hue 0, no geometry -- and the hue round trip still changes pixels
    assert lat["colour"][0].tolist() == [1, 1, 1] and lat["hue_add"][0] == 0 and lat["angle"][0] == 0 and not lat["trans"][0].any()
    changed = int((lat["out"][0] != lat["frames"][0]).any(-1).sum())
    assert 0 < changed < 4096
    # 128 px: the shipped-range sample reads the reflection on all four sides
    valid, _, _ = R.source_index(case(g, 3)["affine"][0], 128)
    P, a = 64, [int(v) for v in case(g, 3)["affine"][0]]
    Y, X = np.meshgrid(np.arange(128) + P, np.arange(128) + P, indexing="ij")
    xi, yi = (a[2] + a[0] * X + a[1] * Y) >> 16, (a[5] + a[3] * X + a[4] * Y) >> 16
    assert valid.all() and (xi < P).any() and (xi >= P + 128).any() and (yi < P).any() and (yi >= P + 128).any()


@pytest.mark.parametrize("ci", range(len(SHAPES)))
def test_restatement_equals_the_golden(golden, ci):
    c = case(golden("g18_augment"), ci)
    S = c["frames"].shape[2]
    assert [R.hue_add_of(h) for h in c["hue"]] == c["hue_add"].tolist()
    affine = np.stack([R.affine_fixed(a, t[0], t[1], S) for a, t in zip(c["angle"], c["trans"])])
    assert np.array_equal(affine, c["affine"])
    out, mean_l = R.augment_frames(c["frames"], c["colour"], c["hue_add"], c["affine"])
    assert np.array_equal(mean_l, c["mean_l"]) and np.array_equal(out, c["out"])
    assert np.array_equal(R.augment_flow(c["flow"], c["affine"]), c["flow_out"])


def test_restatement_equals_pillow(golden):
    """one case through Pillow itself: ImageEnhance, the HSV round trip, np.pad, Image.transform and crop"""
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    c = case(golden("g18_augment"), 1)
    B, T, S = c["frames"].shape[:3]
    P = S // 2

    def geometry(img, b):
        a = np.asarray(img)
        padded = Image.fromarray(np.pad(a, ((P, P), (P, P)) + (((0, 0),) if a.ndim == 3 else ()), mode="reflect"))
        m = R.affine_matrix(float(c["angle"][b]), int(c["trans"][b, 0]), int(c["trans"][b, 1]), S)
        return padded.transform((2 * S, 2 * S), Image.AFFINE, m, Image.NEAREST).crop((P, P, P + S, P + S))

    for b in range(B):
        fb, fc, fs = (float(v) for v in c["colour"][b])
        for t in range(T):
            img = ImageEnhance.Contrast(ImageEnhance.Brightness(Image.fromarray(c["frames"][b, t])).enhance(fb)).enhance(fc)
            h, s, v = img.convert("HSV").split()
            h = Image.fromarray((np.asarray(h).astype(np.int32) + int(c["hue_add"][b])).astype(np.uint8), "L")
            img = ImageEnhance.Color(Image.merge("HSV", (h, s, v)).convert("RGB")).enhance(fs)
            assert np.array_equal(np.asarray(geometry(img, b)), c["out"][b, t]), (b, t)
        for ch in range(2):
            assert np.array_equal(np.asarray(geometry(Image.fromarray(c["flow"][b, ch], mode="F"), b)), c["flow_out"][b, ch])


def test_params_builds_the_kernel_arguments(golden):
    g = golden("g18_augment")
    for ci, (S, B, T) in enumerate(SHAPES):
        c = case(g, ci)
        aug = ClipAugmenter(dict(SHIPPED, spatial_size=(S, S)))
        p = aug.params(c["colour"][:, 0], c["colour"][:, 1], c["colour"][:, 2], c["hue"], c["angle"], c["trans"][:, 0], c["trans"][:, 1], device="cpu")
        assert len(p) == B and p.mean_l is None
        assert p.affine.dtype == torch.int32 and np.array_equal(p.affine.numpy(), c["affine"])
        assert p.hue_add.dtype == torch.int32 and np.array_equal(p.hue_add.numpy(), c["hue_add"])
        assert p.colour.dtype == torch.float32 and np.array_equal(p.colour.numpy(), c["colour"])
    # angles and translations beyond the golden's, against the restatement
    rng = np.random.RandomState(3)
    aug = ClipAugmenter(dict(SHIPPED, spatial_size=(4096, 4096)))
    ang, tx, ty = rng.uniform(-180, 180, 50), rng.randint(-4096, 4097, 50), rng.randint(-4096, 4097, 50)
    p = aug.params(np.ones(50), np.ones(50), np.ones(50), np.zeros(50), ang, tx, ty, device="cpu")
    assert np.array_equal(p.affine.numpy(), np.stack([R.affine_fixed(a, x, y, 4096) for a, x, y in zip(ang, tx, ty)]))
    ident = aug.params([1], [1], [1], [0], [0], [0], [0], device="cpu").affine[0].tolist()
    assert ident == [65536, 0, 32768, 0, 65536, 32768]
    # hue: truncation toward zero, then wrap
    p = ClipAugmenter(SHIPPED).params([1] * 5, [1] * 5, [1] * 5, [-0.5, -0.001, 0.0, 0.3, 0.5], [0] * 5, [0] * 5, [0] * 5, device="cpu")
    assert p.hue_add.tolist() == [129, 0, 0, 76, 127]


def replay(conf, rng):
    """the reference's two functions (:698-702, :714-717) for one sample, on ``rng`` in place of np.random"""
    make_trans = bool(rng.choice(np.arange(2), size=1, p=[1 - conf["p_col"], conf["p_col"]])[0])
    brightness_val = float(rng.uniform(-conf["augment_b"], conf["augment_b"], 1)[0]) if conf["augment_b"] > 0. and make_trans else 0.
    contrast_val = float(rng.uniform(-conf["augment_c"], conf["augment_c"], 1)[0]) if conf["augment_c"] > 0. and make_trans else 0.
    hue_val = float(rng.uniform(-conf["augment_h"], 2 * conf["augment_h"], 1)[0]) if conf["augment_h"] > 0. and make_trans else 0.
    saturation_val = 1. + (float(rng.uniform(-conf["augment_s"], conf["augment_s"])) if conf["augment_s"] > 0. and make_trans else 0)
    make_trans = bool(rng.choice(np.arange(2), size=1, p=[1 - conf["p_geom"], conf["p_geom"]])[0])
    at, size = conf["aug_trans"], conf["spatial_size"]
    rval = float(rng.uniform(-conf["aug_deg"], conf["aug_deg"], 1)[0]) if conf["aug_deg"] > 0. and make_trans else 0.
    tval_vert = int(rng.randint(int(-at[0] * size[1] / 2), int(at[0] * size[1] / 2), 1)[0]) if at[0] > 0 and make_trans else 0
    tval_hor = int(rng.randint(int(-at[1] * size[0] / 2), int(at[1] * size[0] / 2), 1)[0]) if at[1] > 0 and make_trans else 0
    return 1. + brightness_val, 1. + contrast_val, saturation_val, hue_val, rval, tval_hor, tval_vert


def test_draw_replays_the_reference_calls():
    B = 40
    p = ClipAugmenter(SHIPPED).draw(B, np.random.RandomState(7), device="cpu")
    rng = np.random.RandomState(7)
    want = np.array([replay(SHIPPED, rng) for _ in range(B)])
    got = np.stack([p.brightness, p.contrast, p.saturation, p.hue, p.angle, p.tx, p.ty], 1)
    assert np.array_equal(got, want)
    # both coin flips fall both ways among 40 samples, and a missed flip leaves its parameters at the identity
    col_off, geom_off = (want[:, :4] == [1, 1, 1, 0]).all(1), (want[:, 4:] == 0).all(1)
    assert 0 < col_off.sum() < B and 0 < geom_off.sum() < B
    assert np.array_equal(p.affine.numpy()[geom_off], np.tile([65536, 0, 32768, 0, 65536, 32768], (geom_off.sum(), 1)))
    # inside the configured ranges
    assert (np.abs(want[:, 0] - 1) <= 0.4).all() and (np.abs(want[:, 1] - 1) <= 0.5).all() and (np.abs(want[:, 2] - 1) <= 0.4).all()
    assert (want[:, 3] >= -0.15).all() and (want[:, 3] <= 0.3).all() and (np.abs(want[:, 4]) <= 15).all()
    assert (want[:, 5:] >= -6).all() and (want[:, 5:] < 6).all() and want[:, 5].any() and want[:, 6].any()
    assert np.array_equal(p.colour.numpy(), want[:, :3].astype(np.float32))
    assert p.hue_add.tolist() == [int(h * 255) % 256 for h in want[:, 3]]
    assert np.array_equal(p.affine.numpy(), np.stack([R.affine_fixed(r[4], r[5], r[6], 128) for r in want]))


def test_draw_is_the_identity_without_the_coin_flips():
    p = ClipAugmenter(dict(SHIPPED, p_col=0, p_geom=0)).draw(6, np.random.RandomState(1), device="cpu")
    assert (p.colour == 1).all() and (p.hue_add == 0).all() and not p.angle.any() and not p.tx.any() and not p.ty.any()
    assert (p.affine == torch.tensor([65536, 0, 32768, 0, 65536, 32768], dtype=torch.int32)).all()
    # no ranges configured: the same, whatever the coins say
    p = ClipAugmenter({"augment": True, "p_col": 1, "p_geom": 1, "spatial_size": (64, 64)}).draw(3, np.random.RandomState(1), device="cpu")
    assert (p.colour == 1).all() and (p.hue_add == 0).all() and (p.affine[:, 0] == 65536).all() and (p.affine[:, 1] == 0).all()


def test_errors():
    with pytest.raises(ValueError, match="square"):
        ClipAugmenter(dict(SHIPPED, spatial_size=(128, 64)))
    aug = ClipAugmenter(SHIPPED)
    for hue in (0.5001, -0.51):
        with pytest.raises(ValueError, match="hue"):
            aug.params([1], [1], [1], [hue], [0], [0], [0], device="cpu")
    with pytest.raises(ValueError, match="hue"):                                                      # 2 * augment_h can pass 0.5
        ClipAugmenter(dict(SHIPPED, augment_h=0.45, p_col=1)).draw(50, np.random.RandomState(0), device="cpu")
    with pytest.raises(ValueError):
        aug.params([1, 1], [1], [1], [0], [0], [0], [0], device="cpu")
    with pytest.raises(ValueError, match="augment is off"):
        ClipAugmenter(dict(SHIPPED, augment=False)).draw(1, np.random.RandomState(0), device="cpu")
    p = aug.params([1], [1], [1], [0], [0], [0], [0], device="cpu")
    with pytest.raises(ValueError, match="size"):
        ClipAugmenter(dict(SHIPPED, spatial_size=(64, 64))).images(torch.zeros(1, 1, 64, 64, 3, dtype=torch.uint8), p)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            aug.images(torch.zeros(1, 1, 128, 128, 3, dtype=torch.uint8), p)
        with pytest.raises(RuntimeError, match="no CPU path"):
            aug.flow(torch.zeros(1, 2, 128, 128), p)
    assert "augment" in PokeSimulator.make_batch.__code__.co_varnames and "frames_u8" in PokeSimulator.make_batch.__code__.co_varnames


def test_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ipoke_aug_frame_means", "ipoke_aug_frames", "ipoke_aug_flow"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.ipoke_aug_frame_means(None, None, 1, 1, 8, None, None) == -1
    assert lib.ipoke_aug_frames(None, None, None, None, None, 1, 1, 8, None, None) == -1
    assert lib.ipoke_aug_flow(None, None, 1, 2, 8, None, None) == -1
    # sizes are checked before anything is launched: odd, above 4096 (the fixed-point terms would pass 32 bits), non-positive
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B, T, S in [(1, 1, 7), (1, 1, 4098), (1, 1, 0), (0, 1, 8), (1, 0, 8), (1, 1, -2)]:
        assert lib.ipoke_aug_frame_means(p, p, B, T, S, p, None) == -1, (B, T, S)
        assert lib.ipoke_aug_frames(p, p, p, p, p, B, T, S, p, None) == -1, (B, T, S)
        assert lib.ipoke_aug_flow(p, p, B, T, S, p, None) == -1, (B, T, S)
    assert b"4096" in lib.ipoke_last_error() or b"shape" in lib.ipoke_last_error()
