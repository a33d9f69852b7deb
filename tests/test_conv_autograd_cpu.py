"""The case table of tests/autograd_exact.py without a device: every case's operands keep fp32 exact, the float64 reference agrees with
a second statement of the convolution (conv_exact.conv_sums / wgrad_sums read through a descriptor), the pure dispatch predicates give
the labels the table claims, and the table holds every convolution geometry the shipped models build."""
import pytest
import torch

from ipoke_amd import _lib, configs
from tests import autograd_exact as A
from tests import conv_exact as X


def test_every_case_keeps_fp32_exact():
    """Constructing the operands asserts every sum of magnitudes below 2^24 quanta and the saved outputs of the ReLU / frame-batched
    cases at most 256 quanta; the largest ratios per result kind are printed.  Limits: 7 (plain) and 3 (spectral) unless the table
    gives ``lim``."""
    worst = {}
    for c in A.CASES:
        o = A.operands(c)
        assert bool((o.x == 0).any()) and bool((o.x > 0).any()) and bool((o.x < 0).any())
        if c.act == "relu":
            assert bool((o.y == 0).any()) and bool((o.y > 0).any()), c.name
        for kind, v in o.bounds.items():
            if v > worst.get(kind, (0, ""))[0]:
                worst[kind] = (v, c.name)
        for i, j, sg in o.pairs:
            assert sg in (2.0, 4.0, 8.0) and float(A.mat_view(c, o.w5)[i, j]) == sg
        assert len({p[2] for p in o.pairs}) == len(o.pairs)
    for kind, (v, name) in sorted(worst.items()):
        print(f"largest sum of magnitudes / 2^24 for {kind}: {v / X.EXACT_LIMIT:.5f} ({name})")
        assert v < X.EXACT_LIMIT
    print("lowered limits:", {c.name: c.lim for c in A.CASES if c.lim is not None})


SECOND = ["c3d_s222", "c3d_s121", "c3d_1x1_s2_odd", "c2d_3x3_s2_even", "narrow_32_to_5", "ct_plain", "ct_plain_b", "c3d_s212_sn", "patchgan_4x4_s2"]


@pytest.mark.parametrize("name", SECOND)
def test_reference_matches_the_descriptor_statement(name):
    """y and dW of torch's float64 autograd against conv_sums / wgrad_sums on descriptors built here (spectral cases: y with W / sigma,
    and the gradient with respect to W / sigma recovered from dW = (G - <G, W / sigma> u v^T) / sigma)"""
    c = A.BY_NAME[name]
    o = A.operands(c)
    assert c.act == "none"
    taps = c.k[0] * c.k[1] * c.k[2]
    sg = o.pairs[0][2] if o.pairs else 1.0
    xcl = o.x.permute(0, 2, 3, 4, 1).reshape(-1, c.cin).contiguous()
    w_conv = (o.w5.transpose(0, 1) if c.transposed else o.w5).reshape(c.cout, c.cin, taps).permute(0, 2, 1).reshape(c.cout, taps * c.cin) / sg
    d = X.conv_desc(c.N, c.ext, c.odhw(), c.k, c.stride, c.pad, c.cin, c.cout, _lib.F32, transposed=c.transposed)
    y = X.conv_sums(d, xcl, w_conv.contiguous())
    if c.bias:
        y = y + o.b
    assert torch.equal(y, o.y.permute(0, 2, 3, 4, 1).reshape(-1, c.cout))
    g = o.dy.permute(0, 2, 3, 4, 1).reshape(-1, c.cout).contiguous()
    if c.transposed:          # dW[in][out][tap]: the weight gradient of the direct convolution with "input" dy and "output" x
        wd = X.wgrad_desc(c.N, c.odhw(), c.k, c.pad, c.cout, c.cin, _lib.F32, ldy=c.cin, out_dhw=c.ext, s=c.stride)
        G = X.wgrad_sums(wd, g, xcl).permute(0, 2, 1)                       # [cin, cout, taps]
    else:
        wd = X.wgrad_desc(c.N, c.ext, c.k, c.pad, c.cin, c.cout, _lib.F32, ldy=c.cout, out_dhw=c.odhw(), s=c.stride)
        G = X.wgrad_sums(wd, xcl, g).permute(0, 2, 1)                       # [cout, cin, taps]
    G = G.reshape(o.w5.shape).contiguous()
    if o.pairs:
        i, j, _ = o.pairs[0]
        dot = float((G * o.w5).sum()) / sg
        A.mat_view(c, G)[i, j] -= dot                                       # (non-transposed storage: a view of G)
        assert not c.transposed
        G = G / sg
    assert torch.equal(G, o.dw5)


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_predicates_give_the_tables_labels(dtype):
    """``dgrad_phases_ok``, ``stem_folds`` and the ``swapped`` condition restated from its comment against the table (the launch mode of
    the weight gradient -- single, slabs, the kernel's own split -- needs the library and is recorded on the device)"""
    for c in A.CASES:
        want = {l for l in c.want(dtype) if l.startswith(A.PREDICATE_KINDS)}
        assert A.predicted_labels(c, dtype) == want, c.name


def test_label_kinds_are_all_present():
    have = {l for c in A.CASES for dt in A.DTYPES for l in c.want(dt)}
    have = {l.split("(")[0] for l in have}
    for l in ("fwd:generic", "fwd:ct_phases", "fwd:stem", "dgrad:phases2", "dgrad:phases4", "dgrad:phases8", "dgrad:empty_class", "dgrad:ct_outpad",
              "dgrad:direct", "wgrad:plain", "wgrad:mirrored", "wgrad:swapped", "wgrad:stem", "wgrad:src_f32", "wgrad:single", "wgrad:slabs",
              "wgrad:kernel_split", "run:generic", "run:mid", "run:phases", "run:phases_pad2"):
        assert l in have, l


def _shipped_models():
    from ipoke_amd.autoencoder2d import ConvAEModel, ConvPokeAE
    from ipoke_amd.discriminator import PatchDiscriminator, TemporalDiscriminator
    from ipoke_amd.first_stage import FirstStageWrapper, SpadeCondMotionModel
    from ipoke_amd.vgg import VGG
    yield "first stage 64", SpadeCondMotionModel(configs.first_stage_config(64, 32, 16))
    yield "first stage 128", SpadeCondMotionModel(configs.first_stage_config(128, 32, 16))
    yield "2-D encoder", FirstStageWrapper(configs.encoder2d_config(128, 3))
    yield "temporal discriminator", TemporalDiscriminator(64, {"bce_loss": False, "gp_weight": 1.0, "num_classes": 1, "patch_temp_disc": False}, dtype="f32")
    yield "patch temporal discriminator", TemporalDiscriminator(64, {"bce_loss": False, "gp_weight": 1.0, "num_classes": 1, "patch_temp_disc": True}, dtype="f32")
    yield "spatial discriminator", PatchDiscriminator({"bce_loss": False, "gp_weight": 0.0}, dtype="f32")
    yield "poke autoencoder", ConvPokeAE(configs.poke_encoder_train_config(32), dtype="f32")
    yield "image autoencoder", ConvAEModel(configs.img_encoder_train_config(64), dtype="f32")
    yield "VGG", VGG()


def test_census_every_shipped_convolution_geometry_is_in_the_table():
    """Every ``_Conv`` of the shipped models, built on the CPU: its (dims, k, stride, pad, transposed, snorm, bias) occurs in the table."""
    from ipoke_amd.first_stage import _Conv
    table = {c.census_key() for c in A.CASES}
    seen, missing = set(), {}
    for name, model in _shipped_models():
        for mname, m in model.named_modules():
            if isinstance(m, _Conv):
                key = (m.dims, tuple(m.k), tuple(m.stride), tuple(m.pad), bool(m.transposed), bool(m.snorm), m.bias is not None)
                seen.add(key)
                if key not in table:
                    missing.setdefault(key, f"{name}: {mname}")
    print(f"{len(seen)} distinct geometries in the shipped models, {len(table)} in the table")
    assert not missing, missing
