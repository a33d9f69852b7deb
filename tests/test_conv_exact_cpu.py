"""The checker of tests/test_conv_exact_gpu.py, checked without a GPU: its float64 reference against naive loops, its operand bound, and
that the exact comparator catches the mistakes it exists for (a dropped tap x 8-channel chunk at a border pixel, a read of the neighbour
image instead of the zero halo, round-toward-zero instead of round-to-nearest-even, a store into a sentinel)."""
import pytest
import torch

from ipoke_amd import _lib
from tests import conv_exact as X

CPU = "cpu"


def naive_conv(d, A, W):
    """sum over taps and channels by explicit loops over output positions (the descriptor's own index arithmetic, written out)"""
    M = X.rows_of(d)
    Af = A.reshape(-1).to(torch.float64)
    Wm = X.weight_matrix(d, W).view(d.kd, d.kh, d.kw, d.Kc_real, d.Nout)
    out = torch.zeros(M, d.Nout, dtype=torch.float64)
    for m in range(M):
        ow = m % d.Wo; oh = (m // d.Wo) % d.Ho; od = (m // (d.Wo * d.Ho)) % d.Do; n = m // (d.Wo * d.Ho * d.Do)
        for a in range(d.kd):
            for b in range(d.kh):
                for c in range(d.kw):
                    src = []
                    for o, k, s, p, ext in ((od, a, d.sd, d.pd, d.Di), (oh, b, d.sh, d.ph, d.Hi), (ow, c, d.sw, d.pw, d.Wi)):
                        if d.transposed:
                            t = o + p - k
                            src.append(t // s if t >= 0 and t % s == 0 and t // s < ext else None)
                        else:
                            i = o * s - p + k
                            src.append(i if 0 <= i < ext else None)
                    if None in src:
                        continue
                    base = d.a_coff + n * d.a_sn + src[0] * d.a_sd + src[1] * d.a_sh + src[2] * d.a_sw
                    x = Af[base + torch.arange(d.Kc_real) * d.a_sc]
                    out[m] += x @ Wm[a, b, c]
    return out


def _case(lim=None, **kw):
    args = dict(NB=2, in_dhw=(1, 4, 4), out_dhw=(1, 4, 4), k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), Kc=16, Nout=5, dtype=_lib.BF16)
    args.update(kw)
    dtype = args["dtype"]
    d = X.conv_desc(**args)
    return X.ConvCase(d, dtype, CPU, seed=3, lim=lim)


@pytest.mark.parametrize("kw", [
    dict(),                                                                               # 3 x 3, stride 1
    dict(lda=40, a_coff=8, Kc=16, Nout=3),                                                # channel slice of a wider row
    dict(in_dhw=(1, 6, 6), out_dhw=(1, 3, 3), s=(1, 2, 2)),                               # stride 2
    dict(in_dhw=(1, 3, 3), out_dhw=(1, 6, 6), s=(1, 2, 2), transposed=True),              # transposed (data gradient of the stride-2 form)
    dict(in_dhw=(3, 4, 4), out_dhw=(3, 4, 4), k=(3, 3, 3), p=(1, 1, 1), Kc=8),             # 3 x 3 x 3
    dict(in_dhw=(1, 4, 4), out_dhw=(1, 4, 4), k=(1, 2, 2), p=(0, 0, 0), Nout=4,            # a four-tap sub-pixel phase, scattered rows
         scatter=(64, 16, 2, 8 + 1)),
    dict(in_dhw=(1, 5, 6), out_dhw=(1, 5, 6), Kc=8, Kc_real=8, a_f32=True, dtype=_lib.BF16, c_f32=True),   # fp32 planar source
])
def test_reference_matches_naive_loop(kw):
    case = _case(**kw)
    d = case.d
    ref = X.conv_sums(d, case.A_eff, case.W)
    assert torch.equal(ref, naive_conv(d, case.A_eff, case.W))
    assert ref.abs().max() > 0


def test_reference_matches_torch_convolutions():
    """independent of the descriptor arithmetic: torch's float64 conv2d / conv_transpose2d on the same integer operands"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1)
    N, C, H, Wd, O = 2, 8, 6, 4, 5
    x = X.int_operand((N, H, Wd, C), 8, g)
    w = X.int_operand((O, C, 3, 3), 8, g)
    for transposed, s in ((False, 1), (False, 2), (True, 2)):
        Ho, Wo = ((H - 1) * s - 2 + 3 + (s - 1), (Wd - 1) * s - 2 + 3 + (s - 1)) if transposed else ((H - 1) // s + 1, (Wd - 1) // s + 1)
        d = X.conv_desc(N, (1, H, Wd), (1, Ho, Wo), (1, 3, 3), (1, s, s), (0, 1, 1), C, O, _lib.F32, transposed=transposed)
        if transposed:        # tap k multiplies input (out + p - k) / s: ConvTranspose2d with weight [in = C][out = O] = w^T
            wop = w.permute(0, 2, 3, 1).reshape(O, 9 * C)
            ref = F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(1, 0, 2, 3), stride=s, padding=1, output_padding=s - 1)
        else:
            wop = w.permute(0, 2, 3, 1).reshape(O, 9 * C)
            ref = F.conv2d(x.permute(0, 3, 1, 2), w, stride=s, padding=1)
        got = X.conv_sums(d, x.reshape(-1), wop.reshape(-1))
        assert torch.equal(got, ref.permute(0, 2, 3, 1).reshape(-1, O)), (transposed, s)


def test_weight_gradient_reference_matches_naive_loop():
    d = X.wgrad_desc(2, (1, 4, 4), (1, 3, 3), (0, 1, 1), 8, 5, _lib.BF16, y_coff=8, ldy=24)
    case = X.WgradCase(d, _lib.BF16, CPU, seed=2, lim=3, zero_frac=0.2)
    got = X.wgrad_sums(case.d, case.A, case.dY)                     # [Nout, taps, Kc]
    Af = case.A.to(torch.float64)
    dy = case.dY.to(torch.float64)
    ref = torch.zeros_like(got)
    for m in range(X.rows_of(d)):
        ow, oh, n = m % 4, (m // 4) % 4, m // 16
        for b in range(3):
            for c in range(3):
                ih, iw = oh - 1 + b, ow - 1 + c
                if 0 <= ih < 4 and 0 <= iw < 4:
                    x = Af[n * d.a_sn + ih * d.a_sh + iw * d.a_sw + torch.arange(8)]
                    ref[:, b * 3 + c] += torch.outer(dy[m, 8:13], x)
    assert torch.equal(got, ref) and got.abs().max() > 0


def test_generator_bound_holds():
    """the operands of the widest taps x channels product (27 taps x 512 channels) and of a fp32 source stay inside the exact range:
    the measured sum |x * w| is below the asserted bound and the bound below 2^24"""
    for kw in (dict(in_dhw=(3, 4, 4), out_dhw=(3, 4, 4), k=(3, 3, 3), p=(1, 1, 1), Kc=512, Nout=4, bias=True),
               dict(Kc=8, a_f32=True, c_f32=True, bias=True),
               dict(Kc=64, row_scale=(1, 2), bias=True, Nout=8)):
        case = _case(**kw)
        d = case.d
        s = X.conv_sums(d, case.A_eff.abs(), case.W.to(torch.float64).abs(), absolute=True)
        assert float(s.max()) <= case.max_abs_sum < X.EXACT_LIMIT * case.quantum
    # the bound refuses operands that could round
    with pytest.raises(AssertionError, match="too large"):
        _case(Kc=512, k=(3, 3, 3), in_dhw=(3, 4, 4), out_dhw=(3, 4, 4), p=(1, 1, 1), lim=200)
    # typical magnitudes are far past bf16's exact integers (so a bf16 partial sum cannot stay exact)
    case = _case(Kc=64, Nout=8)
    assert float(X.conv_sums(case.d, case.A_eff, case.W).abs().median()) > 2 ** 9


def test_fp32_source_values_need_round_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x = X.frac_operand((4096,), g)
    nz = x != 0
    rne = x.to(torch.bfloat16).to(torch.float32)
    trunc = (x.view(torch.int32) & -65536).view(torch.float32)
    assert bool((rne != x)[nz].float().mean() > 0.9)                       # almost none is a bf16 value already
    assert bool((rne != trunc).any())                                       # truncation would differ
    lo = x.abs()[nz].min(); hi = x.abs().max()
    assert lo >= 1 and hi < 8


def _exact_output(case):
    E, tol = case.expected()
    return E.to(case.c_t), E, tol


def test_comparator_accepts_the_exact_result():
    for kw in (dict(), dict(c_f32=True), dict(act=_lib.ACT_RELU, bias=True), dict(act=_lib.ACT_TANH, bias=True),
               dict(dact_act=_lib.ACT_ELU), dict(row_scale=(1, 2), bias=True), dict(lda=40, a_coff=8, ldc=40, c_coff=16, Nout=9)):
        case = _case(**kw)
        got, E, tol = _exact_output(case)
        X.assert_exact(got, E, tol, case.c_t, case.d, str(kw))


def test_comparator_catches_a_dropped_tap_chunk_at_a_border_pixel():
    """one tap x 8-channel chunk missing at one border output pixel: a few units on outputs of magnitude ~1e3 -- inside 3e-2 * max|y|"""
    case = _case(Kc=64, Nout=8, in_dhw=(1, 8, 8), out_dhw=(1, 8, 8))
    d = case.d
    got, E, tol = _exact_output(case)
    m = 8 * 7 + 0                                       # image 0, row 7 (bottom border), column 0
    x = X.gather_rows(d, case.A_eff, torch.tensor([m]))[0].view(9, 64)
    w = X.weight_matrix(d, case.W).view(9, 64, 8)
    tap, c0 = 1, 16                                     # tap (0, 1): above the pixel, on the map
    lost = x[tap, c0:c0 + 8] @ w[tap, c0:c0 + 8]
    assert bool((lost != 0).any())
    bad = (E[m, :8] - lost).to(case.c_t)
    got[m, :8] = bad
    assert float(lost.abs().max()) < 3e-2 * float(E[: X.rows_of(d), :8].abs().max())      # what the loose tolerance lets through
    with pytest.raises(AssertionError, match=r"first at \(n=0, d=0, h=7, w=0"):
        X.assert_exact(got, E, tol, case.c_t, d)


def test_comparator_catches_a_read_of_the_neighbour_image():
    """the halo of image 1's top-left pixel read as image 0's last pixels instead of zeros"""
    case = _case(Kc=16, Nout=4, c_f32=True)
    d = case.d
    got, E, tol = _exact_output(case)
    m = 16                                              # image 1, (0, 0)
    A = case.A_eff.view(-1)
    w = X.weight_matrix(d, case.W).view(9, 16, 4)
    # tap (0, 0) of (n=1, 0, 0) is (n=1, -1, -1); flat row arithmetic lands on (n=0, 2, 3)
    x = A[0 * d.a_sn + 2 * d.a_sh + 3 * d.a_sw + torch.arange(16)]
    extra = x @ w[0]
    assert bool((extra != 0).any())
    got[m, :4] = (E[m, :4] + extra).to(case.c_t)
    with pytest.raises(AssertionError, match=r"n=1, d=0, h=0, w=0"):
        X.assert_exact(got, E, tol, case.c_t, d)


def test_comparator_catches_round_toward_zero():
    case = _case(Kc=64, Nout=8)
    got, E, tol = _exact_output(case)
    trunc = (E.to(torch.float32).view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    assert not torch.equal(trunc, got)
    with pytest.raises(AssertionError, match="mismatching"):
        X.assert_exact(trunc, E, tol, case.c_t, case.d)


@pytest.mark.parametrize("where", ["row_past_M", "column_past_range", "padded_column", "scatter_gap"])
def test_comparator_catches_a_write_into_a_sentinel(where):
    kw = dict(lda=40, a_coff=8, ldc=40, c_coff=16, Nout=5) if where == "column_past_range" else dict(Nout=5)
    if where == "scatter_gap":
        kw = dict(in_dhw=(1, 4, 4), out_dhw=(1, 4, 4), k=(1, 2, 2), p=(0, 0, 0), Nout=4, scatter=(64, 16, 2, 1))
    case = _case(**kw)
    d = case.d
    got, E, tol = _exact_output(case)
    M = X.rows_of(d)
    if where == "row_past_M":
        r, c = M + 5, 0
    elif where == "column_past_range":
        r, c = 3, 16 + 8              # c_coff + round_up(Nout, 8) is the first column the launch must leave alone
    elif where == "padded_column":
        r, c = 3, 6                   # [Nout, round_up(Nout, 8)): written as zero
    else:
        r, c = 0, 0                   # phase (0, 1) writes odd columns only: row 0 is phase (0, 0)'s
    assert float(E[r, c]) in (X.SENT, 0.0)
    got[r, c] = 7.0
    with pytest.raises(AssertionError, match="mismatching"):
        X.assert_exact(got, E, tol, case.c_t, d)


def test_weight_gradient_comparator_catches_a_stray_store():
    d = X.wgrad_desc(2, (1, 4, 4), (1, 3, 3), (0, 1, 1), 8, 5, _lib.BF16)
    d.w_sn = 8 * 9 + 4                                   # gaps between the out-channel rows hold sentinels
    case = X.WgradCase(d, _lib.BF16, CPU, seed=4, lim=2, zero_frac=0.2)
    ref = X.wgrad_sums(case.d, case.A, case.dY)
    case.dW[case._positions(0)] = ref.permute(0, 2, 1).reshape(-1).to(torch.float32)
    case.compare("exact")
    case.dW[8 * 9 + 1] = 0.0
    with pytest.raises(AssertionError, match="outside"):
        case.compare("stray")
