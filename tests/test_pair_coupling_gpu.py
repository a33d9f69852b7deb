"""ipoke_conv_pair_coupling: conv2 (+ bias, ELU), conv3 and the coupling transform of a coupling net (NICEConvBlock, macow_utils.py:270-281,
42-66) as one launch -- every 128-column tile of conv2's GEMM is one K slice of conv3, the slices meet inside the launch and the rows'
owners apply the coupling.

Shapes: M = 64, 128, 192 rows (half a tile, one tile, a ragged second tile), hidden 512 / 1024 / 2048 (4 slices: two 16-row slices per
owner; 8; 16), Cp 4 / 15 / 32 transformed channels, dense (t_off 0, t_stride 1) and interleaved (1, 2), in a state of pitch 64 and of the
ragged pitch 60, the three coupling modes, with and without the extra operand output, with and without the stored h2 -- and the
workload's own grid, B = 20 at hidden 2048."""
import functools
from ctypes import byref

import pytest
import torch

from ipoke_amd import _lib, configs, ops
from ipoke_amd._lib import AffineDesc, CouplingEpi, check
from tests import conv_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = X.GUARD_ROWS

SHAPES = [(B, hidden) for B in (1, 2, 3) for hidden in (512, 1024, 2048)]
# (Cp, ld, t_off, t_stride): every Cp dense and interleaved, in both pitches where the columns fit (1 + 2 * 31 > 59)
COUPLINGS = [(4, 64, 0, 1), (4, 60, 1, 2), (15, 64, 1, 2), (15, 60, 0, 1), (15, 60, 1, 2), (32, 64, 0, 1), (32, 64, 1, 2), (32, 60, 0, 1)]


def _ids(v):
    return "-".join(str(x) for x in v)


@functools.lru_cache(maxsize=None)
def _xchg():
    L = _lib.lib()
    x = torch.empty(L.ipoke_conv3x3_coupling_xchg_bytes(), dtype=torch.uint8, device=DEV)
    check(L.ipoke_conv3x3_coupling_xchg_init(x.data_ptr(), ops._s()))
    torch.cuda.synchronize()
    return x


def _scratch_is_clean(x):
    head = x[:256].view(torch.int32)
    return int(head[0].item()) == 0 and bool((x[256:] == 255).all().item())


def _descs(B, hidden, Cp):
    d2 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 1, 1), (1, 1, 1), (0, 0, 0))
    d3 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1))
    for d in (d2, d3):
        d.a_sn = 64 * hidden; d.a_sd = 0; d.a_sh = 8 * hidden; d.a_sw = hidden; d.a_sc = 1; d.Kc_real = hidden; d.Kc = hidden
    d2.ldw = hidden; d2.Nout = hidden; d2.act = _lib.ACT_ELU; d2.c_f32 = 0; d2.ldc = hidden
    d3.ldw = 9 * hidden; d3.Nout = 2 * Cp
    return d2, d3


@functools.lru_cache(maxsize=None)
def _problem(kind, B, hidden, cpl):
    """Operands on the device.  kind 'real': randn.  kind 'int': see test_pair_coupling_is_exact_on_integer_operands."""
    Cp, ld, t_off, t_stride = cpl
    M = B * 64
    gen = torch.Generator(device=DEV).manual_seed(1000 * B + hidden + 17 * Cp + ld + t_off + (7 if kind == "int" else 0))
    f64 = dict(generator=gen, device=DEV, dtype=torch.float64)
    if kind == "real":
        h1 = torch.randn(M, hidden, **f64)
        w2 = torch.randn(hidden, hidden, **f64) / hidden ** 0.5
        b2 = torch.randn(hidden, **f64) * 0.3
        w3 = torch.randn(2 * Cp, 9 * hidden, **f64) / (9 * hidden) ** 0.5 * 2
        b3 = torch.randn(2 * Cp, **f64) * 0.3
        state = torch.randn(M + GUARD, ld, **f64)
    else:
        # h1 in {0, 1} (a quarter ones), conv2 weights in {0, 1} (an eighth ones), bias in 0 .. 3: every pre-activation is a non-negative
        # integer of mean hidden / 32 + 1.5, ELU is the identity.  Every 16th hidden channel is QUIET: its weight row is a single one on
        # the diagonal and its bias 0, so h2 there is h1's 0 / 1.
        h1 = (torch.rand(M, hidden, **f64) < 0.25).to(torch.float64)
        w2 = (torch.rand(hidden, hidden, **f64) < 0.125).to(torch.float64)
        b2 = torch.randint(0, 4, (hidden,), generator=gen, device=DEV).to(torch.float64)
        quiet = torch.arange(0, hidden, 16, device=DEV)
        w2[quiet] = 0; w2[quiet, quiet] = 1; b2[quiet] = 0
        # conv3: the mu rows dense in {-1, 0, 1} over every channel (large sums, exact in fp32); the s rows have six +-1 entries each, on
        # quiet channels of six different 128-channel slices spread over the taps: s is an integer in [-6, 6] + bias, which the
        # tanh of the scale does not saturate on
        w3 = torch.zeros(2 * Cp, 9, hidden, dtype=torch.float64, device=DEV)
        w3[:Cp] = X.int_operand((Cp, 9, hidden), 1, gen, zero_frac=0.5)
        nsl = hidden // 128
        for j in range(Cp):
            for k in range(6):
                sl = (j + k * max(1, nsl // 6) + k) % nsl if nsl >= 6 else k % nsl
                ch = sl * 128 + 16 * ((j + 3 * k) % 8)
                w3[Cp + j, (2 * j + 4 * k) % 9, ch] += 1.0 if (j + k) % 3 else -1.0
        w3 = w3.reshape(2 * Cp, 9 * hidden)
        b3 = torch.cat([X.int_operand((Cp,), 8, gen, zero_frac=0.2), X.int_operand((Cp,), 1, gen, zero_frac=0.3)])
        state = X.int_operand((M + GUARD, ld), 8, gen, zero_frac=0.1)
        tc = t_off + torch.arange(Cp, device=DEV) * t_stride
        state[:, tc] = 0              # transformed channels: zero, so that mode 0 returns mu itself (scale * 0 + mu)
    h1, w2, w3 = (v.to(torch.bfloat16).contiguous() for v in (h1, w2, w3))
    b2, b3, state = (v.to(torch.float32).contiguous() for v in (b2, b3, state))
    gen_c = torch.Generator().manual_seed(99 + ld)
    an = dict(ls=(torch.randn(ld, generator=gen_c) * 0.2).to(DEV), b=torch.randn(ld, generator=gen_c).to(DEV),
              idx=torch.randperm(ld, generator=gen_c).to(torch.int32).to(DEV))
    return dict(h1=h1, w2=w2, b2=b2, w3=w3, b3=b3, state=state, an=an)


class Run:
    """descriptors on fresh, pattern-filled outputs (guard rows behind every one of them)"""

    def __init__(self, pr, B, hidden, cpl, mode, ext, store_h2=True):
        Cp, ld, t_off, t_stride = cpl
        M = B * 64
        self.M, self.B, self.hidden, self.mode = M, B, hidden, mode
        self.d2, self.d3 = _descs(B, hidden, Cp)
        fill = lambda shape, dt=torch.float32: torch.full(shape, X.SENT, dtype=dt, device=DEV)
        self.buf = dict(h2=fill((M + GUARD, hidden), torch.bfloat16), out=fill((M + GUARD, ld)), out2=fill((M + GUARD, ld)),
                        scale=fill((M + GUARD, Cp)), slots=fill((B + 4, 4)))
        self.ext_ld = -(-Cp // 8) * 8 + 8
        self.buf["ext"] = fill((M + GUARD, self.ext_ld), torch.bfloat16)
        b = self.buf
        self.d2.A = pr["h1"].data_ptr(); self.d2.W = pr["w2"].data_ptr(); self.d2.bias = pr["b2"].data_ptr()
        self.d2.C = b["h2"].data_ptr() if store_h2 else None
        self.d3.A = b["h2"].data_ptr() if store_h2 else None
        self.d3.W = pr["w3"].data_ptr()
        self.a = AffineDesc()
        self.a.bias = pr["b3"].data_ptr(); self.a.Cp = Cp; self.a.t_off = t_off; self.a.t_stride = t_stride; self.a.P = 64; self.a.ld = ld
        e = self.e = CouplingEpi()
        e.mode = mode; e.inp = pr["state"].data_ptr(); e.out = b["out"].data_ptr(); e.xchg = _xchg().data_ptr()
        if mode != 2:
            e.scale_out = b["scale"].data_ptr(); e.logdet_slot = b["slots"].data_ptr(); e.slot_stride = 4
        if mode == 1:
            an = pr["an"]
            e.out2 = b["out2"].data_ptr(); e.an_c0 = 0; e.an_C = ld
            e.an_log_scale = an["ls"].data_ptr(); e.an_bias = an["b"].data_ptr(); e.an_idx = an["idx"].data_ptr()
        elif ext:
            e.ext = b["ext"].data_ptr(); e.ext_ld = self.ext_ld

    def two_launches(self):
        L = _lib.lib()
        with _lib.dispatch_override("nt128", 2):
            ops.conv_forward(self.d2, "bf16")
        assert L.ipoke_last_conv_kernel() == _lib.KERNEL_IGEMM
        with _lib.dispatch_override("cpl_split", self.hidden // 128):
            check(L.ipoke_conv3x3_coupling(byref(self.d3), byref(self.a), byref(self.e), self.B, _lib.BF16, ops._s()))
        assert L.ipoke_last_conv_kernel() == _lib.KERNEL_S8
        torch.cuda.synchronize()
        return self

    def fused(self):
        L = _lib.lib()
        check(L.ipoke_conv_pair_coupling(byref(self.d2), byref(self.d3), byref(self.a), byref(self.e), self.B, _lib.BF16, ops._s()))
        assert L.ipoke_last_conv_kernel() == _lib.KERNEL_IGEMM
        torch.cuda.synchronize()
        return self


def _same_bits(x, y):
    v = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
    return torch.equal(x.view(v), y.view(v))


def _assert_identical(got, ref, skip=()):
    for k in ref.buf:
        if k in skip:
            continue
        x, y = ref.buf[k], got.buf[k]
        assert _same_bits(x, y), f"{k} differs: max {(x.float() - y.float()).abs().max().item():.3e}"


def _written(run, mode, ext):
    """the outputs this mode writes hold no fill pattern inside their rows (the fill is no value the operands produce everywhere)"""
    M = run.M
    names = {0: ("h2", "out", "scale"), 1: ("h2", "out", "out2", "scale"), 2: ("h2", "out")}[mode] + (("ext",) if ext and mode != 1 else ())
    for k in names:
        assert not bool((run.buf[k][:M] == X.SENT).all()), f"{k}: not written"
    if mode != 2:
        assert not bool((run.buf["slots"][:run.B] == X.SENT).any()), "log-det slots: not written"


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("cpl", COUPLINGS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_pair_coupling_is_bit_identical_to_the_two_launches(shape, cpl, mode):
    """Real-valued operands: conv2 on the 128 x 128 tile (one K pass), then conv3 + coupling at hidden / 128 slices -- the fused launch keeps
    the K-block order of both, so the state, out2, ext, scale_out, the log-det slots and the stored h2 agree in every bit, the guard rows
    and every buffer the mode does not write keep their fill, and the exchange scratch is back in its initial state."""
    B, hidden = shape
    pr = _problem("real", B, hidden, cpl)
    for ext in ((False, True) if mode != 1 else (False,)):
        ref = Run(pr, B, hidden, cpl, mode, ext).two_launches()
        _written(ref, mode, ext)
        got = Run(pr, B, hidden, cpl, mode, ext).fused()
        _assert_identical(got, ref)
        assert _scratch_is_clean(_xchg()), "exchange scratch not restored"
        if mode == 2:       # the reverse pass: h2 is not stored (conv2.C == NULL), everything else is the same
            got = Run(pr, B, hidden, cpl, mode, ext, store_h2=False).fused()
            _assert_identical(got, ref, skip=("h2",))
            assert bool((got.buf["h2"] == X.SENT).all())
            assert _scratch_is_clean(_xchg()), "exchange scratch not restored"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pair_coupling_at_the_workload_grid(mode):
    """B = 20, hidden 2048, Cp 32 interleaved in a 64-column state: the c2 train step's own launch (10 row tiles x 16 slices)."""
    B, hidden, cpl = 20, 2048, (32, 64, 1, 2)
    pr = _problem("real", B, hidden, cpl)
    ext = mode != 1
    ref = Run(pr, B, hidden, cpl, mode, ext).two_launches()
    _written(ref, mode, ext)
    got = Run(pr, B, hidden, cpl, mode, ext, store_h2=mode != 2).fused()
    _assert_identical(got, ref, skip=("h2",) if mode == 2 else ())
    assert _scratch_is_clean(_xchg())


@pytest.mark.parametrize("cpl", [(4, 64, 0, 1), (15, 60, 1, 2), (32, 64, 1, 2)], ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_pair_coupling_is_exact_on_integer_operands(shape, cpl):
    """Non-negative integer inputs, conv2 weights and bias, sparse enough that every pre-activation is an integer <= 256: ELU is the
    identity and h2 is exact in bf16.  conv3 weights in {-1, 0, 1}: every partial sum is exact in fp32, whatever the slice order.  The
    stored h2 equals the float64 sums; mode 0 on a state whose transformed channels are zero returns mu itself (scale * 0 + mu), and the
    raw s -- an integer in [-7, 7] by construction -- is recovered from scale_out = tanh(s / 2) + 1 (macow_utils.py:46-52) by rounding."""
    B, hidden = shape
    Cp, ld, t_off, t_stride = cpl
    M = B * 64
    pr = _problem("int", B, hidden, cpl)
    run = Run(pr, B, hidden, cpl, 0, False)
    E2 = X.conv_sums(run.d2, pr["h1"], pr["w2"]) + pr["b2"].to(torch.float64)
    assert float(E2.min()) >= 0 and float(E2.max()) <= 256, (float(E2.min()), float(E2.max()))
    h2 = E2.to(torch.bfloat16)
    assert torch.equal(h2.to(torch.float64), E2)
    X.assert_exact_bound(X.conv_sums(run.d3, h2, pr["w3"], absolute=True) + pr["b3"].abs().max().to(torch.float64))
    raw = X.conv_sums(run.d3, h2, pr["w3"]) + pr["b3"].to(torch.float64)
    mu, s = raw[:, :Cp], raw[:, Cp:]
    assert float(s.abs().max()) <= 7 and float(s.abs().max()) >= 2 and float(mu.abs().max()) > 64
    run.fused()
    X.assert_exact(run.buf["h2"][:M], E2, None, torch.bfloat16, run.d2, "h2")
    assert bool((run.buf["h2"][M:] == X.SENT).all()), "h2: rows beyond M were written"
    tc = t_off + torch.arange(Cp, device=DEV) * t_stride
    out = run.buf["out"]
    assert torch.equal(out[:M][:, tc].to(torch.float64), mu), f"mu differs: max {(out[:M][:, tc].to(torch.float64) - mu).abs().max().item():.3e}"
    rest = torch.ones(ld, dtype=torch.bool, device=DEV); rest[tc] = False
    assert torch.equal(out[:M][:, rest], pr["state"][:M][:, rest]) and bool((out[M:] == X.SENT).all())
    sc = run.buf["scale"][:M].to(torch.float64)
    s_back = 2 * torch.atanh((sc - 1).clamp(-1 + 1e-9, 1 - 1e-9))
    assert float((s_back - s_back.round()).abs().max()) < 1e-2         # (tanh(3.5) and tanh(3) are 3e-3 apart: no ambiguity)
    assert torch.equal(s_back.round(), s), f"s differs at {int((s_back.round() != s).sum())} elements"
    assert _scratch_is_clean(_xchg())


@pytest.mark.parametrize("case", [(3, 2048, (15, 60, 1, 2), 0), (2, 512, (32, 64, 0, 1), 1), (20, 2048, (32, 64, 1, 2), 2)], ids=lambda c: f"B{c[0]}_h{c[1]}_m{c[3]}")
def test_pair_coupling_is_deterministic_beside_a_copy_stream(case):
    """The same launch twice while a second stream keeps copying: workgroups arrive in another order, every output keeps its bits and the
    exchange scratch is clean afterwards."""
    B, hidden, cpl, mode = case
    pr = _problem("real", B, hidden, cpl)
    first = Run(pr, B, hidden, cpl, mode, mode != 1).fused()
    noise = torch.randn(64 << 20, device=DEV)
    side = torch.cuda.Stream()
    for k in (1, 3):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(k):
                noise.clone()
        again = Run(pr, B, hidden, cpl, mode, mode != 1).fused()
        _assert_identical(again, first)
        assert _scratch_is_clean(_xchg())


def test_pair_coupling_dispatch_rule():
    L = _lib.lib()
    assert L.ipoke_conv_pair_coupling_applicable(1280, 2048, 64, _lib.BF16) == 1          # c2
    assert L.ipoke_conv_pair_coupling_applicable(1280, 2048, 32, _lib.BF16) == 1
    assert L.ipoke_conv_pair_coupling_applicable(2560, 2048, 64, _lib.BF16) == 0          # c3's rows at this width: 20 x 16 workgroups
    assert L.ipoke_conv_pair_coupling_applicable(1280, 2048, 64, _lib.F32) == 0
    # a shape outside the rule is refused, not run
    cpl = (4, 64, 0, 1)
    pr = _problem("real", 1, 512, cpl)
    run = Run(pr, 1, 512, cpl, 0, False)
    assert L.ipoke_conv_pair_coupling(byref(run.d2), byref(run.d3), byref(run.a), byref(run.e), 1, _lib.F32, ops._s()) != 0
    run.d3.NB = 2
    assert L.ipoke_conv_pair_coupling(byref(run.d2), byref(run.d3), byref(run.a), byref(run.e), 1, _lib.BF16, ops._s()) != 0
    torch.cuda.synchronize()
    assert all(bool((v == X.SENT).all()) for v in run.buf.values())


def _engine(hidden, max_batch):
    from ipoke_amd.flow import SupervisedMacowTransformer
    from ipoke_amd.utils.detfill import deterministic_fill_
    arch = configs.flow_arch(32, hidden=hidden, num_steps=[2, 1, 1], factor=4)
    m = SupervisedMacowTransformer(arch, dtype="bf16", device="cuda", init="none", max_batch=max_batch)
    deterministic_fill_(m, prefix="flow.")
    m.sync_buffers()
    return m, arch


def test_engine_takes_the_fused_launch_at_the_c2_shape():
    """The flow at hidden 2048 and B = 20 (M = 1280): under the default rule the last convolution launch of a forward pass is the fused one
    (ipoke_last_conv_kernel reports the GEMM family, as for ipoke_conv_pair_dgrad); with the hook it is ipoke_conv3x3_coupling (the
    stationary-input family).  The in-situ timing counts one square-GEMM launch per coupling net either way, and the results agree
    bit for bit."""
    import ctypes
    m, arch = _engine(2048, 20)
    m.eval()
    eng = m.engine
    L = eng.lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(20, 32, 8, 8, generator=g).cuda()
    cond = torch.randn(20, arch["h_channels"], 8, 8, generator=g).cuda()
    tags = (ctypes.c_int * 2)(1, 16 + _lib.KERNEL_S8)

    def run(split):
        check(L.ipoke_flow_test_split_pair_coupling(eng.handle, int(split)))
        with torch.no_grad():
            m(x, cond)
            torch.cuda.synchronize()
            check(L.ipoke_timing_start_all())
            out, logdet = m(x, cond)
            torch.cuda.synchronize()
        last = L.ipoke_last_conv_kernel()
        counts = (ctypes.c_int * 2)(); mean = (ctypes.c_double * 2)()
        check(L.ipoke_timing_stop(tags, 2, counts, mean))
        return out, logdet, (counts[0], counts[1], last)

    try:
        o_f, l_f, n_f = run(False)
        o_s, l_s, n_s = run(True)
    finally:
        L.ipoke_flow_test_split_pair_coupling(eng.handle, 0)
    print(f"(square GEMM launches, stationary-input family launches, last conv kernel): fused {n_f}, split {n_s}")
    assert n_f[0] == n_s[0] > 0 and n_f[1] == n_s[1], (n_f, n_s)
    assert n_f[2] == _lib.KERNEL_IGEMM and n_s[2] == _lib.KERNEL_S8, (n_f, n_s)
    assert torch.equal(o_f, o_s) and torch.equal(l_f, l_s)
    assert tuple(eng.handoff_timeouts()) == (0, 0)


def test_engine_fused_and_split_passes_are_bit_identical():
    """A reduced flow widened so the rule applies (hidden 512, B = 2): forward + backward and the reverse pass with the fused launches and
    with the hook that issues the two launches (same tile, same slices) -- states, log-dets and every gradient bit for bit; the
    captured-graph replay of the reverse pass equals the eager pass."""
    m, arch = _engine(512, 2)
    m.train()
    eng = m.engine
    L = eng.lib
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 32, 8, 8, generator=g).cuda()
    z0 = torch.randn(2, 32, 8, 8, generator=g).cuda()
    cond = torch.randn(2, arch["h_channels"], 8, 8, generator=g).cuda()

    def run(split):
        check(L.ipoke_flow_test_split_pair_coupling(eng.handle, int(split)))
        m.flat_grads.zero_()
        x = x0.clone().requires_grad_(True)
        out, logdet = m(x, cond)
        loss = (out ** 2).sum() * 0.5 - logdet.sum()
        loss.backward()
        with torch.no_grad():
            rev = [m(z0, cond, reverse=True).clone()]                        # eager
            m.set_graph_mode(True)
            rev += [m(z0, cond, reverse=True).clone() for _ in range(3)]     # captured, then replayed
            m.set_graph_mode(False)
        torch.cuda.synchronize()
        return dict(out=out.detach().clone(), logdet=logdet.detach().clone(), grads=m.flat_grads.clone(), dx=x.grad.clone(), rev=rev)

    try:
        f = run(False)
        s = run(True)
        f2 = run(False)
    finally:
        L.ipoke_flow_test_split_pair_coupling(eng.handle, 0)
    assert torch.isfinite(f["grads"]).all() and f["grads"].abs().max() > 0 and torch.isfinite(f["rev"][0]).all()
    for k in ("out", "logdet", "grads", "dx"):
        assert torch.equal(f[k], f2[k]), f"{k}: the fused pass is not reproducible"
        assert torch.equal(f[k], s[k]), f"{k} differs: max {(f[k] - s[k]).abs().max().item():.3e}"
    for r in f["rev"][1:] + f2["rev"]:
        assert torch.equal(r, f["rev"][0]), "reverse pass: a replay differs from the eager pass"
    assert torch.equal(f["rev"][0], s["rev"][0]), f"reverse pass differs: max {(f['rev'][0] - s['rev'][0]).abs().max().item():.3e}"
