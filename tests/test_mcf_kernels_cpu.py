"""CPU: pins what test_mcf_kernels_gpu.py relies on -- the float64 references of tests/mcf_exact.py against the oracle's MaskedConvFlow
and MaCowUnit (forward, log-det, reverse, autograd), that the exact operand family is exact and fits the number formats, that its
operands separate an addressing error, the input conditions of the inexact family, and the recorded yardsticks."""
import pytest
import torch

from oracle import flow_ref
from tests import mcf_exact as X
from tests.mcf_exact import BF16, F32, F64, LAYER_CASES, UNIT2_CASES, UNIT_CASES, YARDSTICK

IDS = lambda cs: [c.id for c in cs]                                                            # noqa: E731
ALL_CASES = LAYER_CASES + UNIT_CASES + UNIT2_CASES


def operands(c, exact):
    return X.layer_operands(c, exact) if isinstance(c, X.LCase) else X.unit_operands(c, exact)


def to_map(rows):
    return rows.reshape(-1, 8, 8, rows.shape[1]).permute(0, 3, 1, 2)


def to_rows(m):
    return m.permute(0, 2, 3, 1).reshape(-1, m.shape[1])


# ------------------------------------------------------------------ the references against the oracle
def _load(flow, L):
    """the effective matrices of a Layer into an oracle MaskedConvFlow: weight_g = |v| makes the weight-normed weight v itself"""
    with torch.no_grad():
        flow.net.shift_conv.weight.copy_(L.W1)
        v = L.W2.reshape(L.W2.shape[0], -1, 1, 1)
        flow.net.conv1x1.conv.weight_v.copy_(v)
        flow.net.conv1x1.conv.weight_g.copy_(v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        flow.net.conv1x1.conv.bias.copy_(L.b2)
        flow.net.conv1x1.initialized.fill_(1)


def _load_actnorm(an, L):
    with torch.no_grad():
        an.log_scale.copy_(L.ls.view(-1, 1, 1)); an.bias.copy_(L.pb.view(-1, 1, 1)); an.initialized.fill_(1)


def _parity(modules, layers, x, h, cond, B):
    """modules: the oracle's layers in forward order (MaskedConvFlow / ActNorm2dFlow) for `layers`"""
    xo = to_map(x).clone().requires_grad_(True)
    cur, total = xo, 0
    for m in modules:
        cur, ld = m(cur) if isinstance(m, flow_ref.ActNorm2dFlow) else m(cur, h=h)
        total = total + ld
    (0.5 * (cur ** 2).sum() - total.sum()).backward()
    ws = X.chain(layers, x, cond)
    y = ws["y"][-1]
    ws = X.chain(layers, x, cond, dy=y, dld=-torch.ones(B, dtype=F64), inverse_of=y)
    const = sum(64.0 * float(L.ls.sum()) for L in layers if L.ls is not None)
    logdet = sum(X.per_sample(v.view(-1, 1), B) for v in ws["ld_rows"]).flatten() + const

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), what

    same(y, to_rows(cur.detach()), "y")
    same(logdet, total.detach(), "log-det")
    same(ws["dx"], to_rows(xo.grad), "d x")
    with torch.no_grad():
        rev = cur.detach()
        for m in reversed(modules):
            rev = m(rev, reverse=True) if isinstance(m, flow_ref.ActNorm2dFlow) else m(rev, h=h, reverse=True)
    same(ws["x_rec"], to_rows(rev), "reverse")
    if all(L.ls is None for L in layers):       # (an ActNorm's inverse divides by exp(ls) + 1e-8, macow2.py:520: no identity behind it)
        assert float((ws["x_rec"] - x).abs().max()) <= 1e-9, "round trip"


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_layer_reference_equals_the_oracle(order, post):
    C, Cc, B = 6, 5, 2
    gen = torch.Generator().manual_seed(10 * order + post)
    L = X.inexact_layer(C, Cc, order, gen, None, post)
    x = torch.randn(B * 64, C, generator=gen, dtype=F64)
    h = torch.randn(B, Cc, 8, 8, generator=gen, dtype=F64)
    cond = to_rows(torch.nn.functional.elu(h))
    ks = (2, 3) if order < 2 else (3, 2)
    flow = flow_ref.MaskedConvFlow(C, ks, "ABCD"[order], Cc).double()
    _load(flow, L)
    modules = [flow]
    if post:
        an = flow_ref.ActNorm2dFlow(C).double()
        _load_actnorm(an, L)
        modules.append(an)
    assert X.OFFSETS[order][:2] == ks
    _parity(modules, [L], x, h, cond, B)


def test_chain_reference_equals_the_oracle_unit():
    C, Cc, B = 4, 3, 2
    gen = torch.Generator().manual_seed(5)
    layers = [X.inexact_layer(C, Cc, X.UNIT_ORDERS[k], gen, None, X.UNIT_POST[k], k) for k in range(4)]
    x = torch.randn(B * 64, C, generator=gen, dtype=F64)
    h = torch.randn(B, Cc, 8, 8, generator=gen, dtype=F64)
    unit = flow_ref.MaCowUnit(C, (2, 3), Cc).double()
    flows = [unit.conv1, unit.conv2, unit.conv3, unit.conv4]
    for f, L in zip(flows, layers):
        _load(f, L)
    _load_actnorm(unit.actnorm1, layers[1]); _load_actnorm(unit.actnorm2, layers[3])
    modules = [unit.conv1, unit.conv2, unit.actnorm1, unit.conv3, unit.conv4, unit.actnorm2]
    _parity(modules, layers, x, h, to_rows(torch.nn.functional.elu(h)), B)
    with torch.no_grad():                                      # and the unit's own composition
        yo, ldo = unit(to_map(x), h=h)
    ws = X.chain(layers, x, to_rows(torch.nn.functional.elu(h)))
    assert float((ws["y"][-1] - to_rows(yo)).abs().max()) <= 1e-12


# ------------------------------------------------------------------ the exact family
@pytest.mark.parametrize("c", ALL_CASES, ids=IDS(ALL_CASES))
def test_exact_operands_are_exact(c):
    """the float64 chain is integer everywhere; every value staged or stored as bf16 stays <= 2^8, every partial sum < 2^24; the
    restatements in the case's type (both algebras) reproduce it bit for bit"""
    layers, x, cond, dy, dld = operands(c, True)
    assert all(bool((L.W1 >= 0).all()) and bool((L.W2[c.C:] == 0).all()) and bool((L.b2[c.C:] == 0).all()) for L in layers)
    assert bool((x >= 0).all()) and bool((dy % 2 == 0).all()) and bool((dld % 2 == 0).all())
    ws = X.chain(layers, x, cond, dy=dy, dld=dld)
    wmax = max(float(L.W1.abs().max()) for L in layers)
    for k, L in enumerate(layers):
        small = [ws["x"][k], ws["y"][k], ws["a2"][k], ws["dp"][k], ws["dc"][k], ws["g"][k]]
        for v in small + [ws["dbias"][k], ws["c"][k]] + ([ws["post_part"][k]] if L.ls is not None else []):
            assert torch.equal(v, v.round()), k
        assert all(float(v.abs().max()) <= 256.0 for v in small), (k, [float(v.abs().max()) for v in small])
        assert bool((ws["c"][k] >= 0).all()) and bool((ws["x"][k] >= 0).all()) and bool((ws["g"][k] % 2 == 0).all()), k
        assert bool((ws["scale"][k] == 1).all()) and bool((ws["ld_rows"][k] == 0).all()), k
        # partial sums: the contractions have at most 6 * 64 (W1), 4 * 64 + Cc (W2) and 6 * 256 (W1T) terms of at most 2^8 * |w|
        assert 256.0 * max(wmax, float(L.W2.abs().max())) * max(6 * 256, 4 * c.C + c.Cc) < 2.0 ** 24
        rows = dld.repeat_interleave(64)
        gy, ds = X.dparams_ref(ws["g"][k], ws["x"][k], ws["scale"][k], rows, L.ls)[:2]
        assert float(X.dbias_ref(gy, ds, c.B)[1].max()) < 2.0 ** 24
        if L.ls is not None:
            assert float(X.post_part_ref(ws["g"][k], ws["y"][k], L.pb, dld, c.B)[1].max()) < 2.0 ** 24
    assert float(ws["dx"].abs().max()) < 2.0 ** 24
    for fast in (False, True):
        # (the inverse in fp32 only: 1 + 1e-8 and 1 + 1e-12 round to 1 there, as on the device, and not in float64)
        r = X.chain(layers, x, cond, dy=dy, dld=dld, tdt=X.TDT[c.dt], cdt=F32, fast=fast, inverse_of=ws["y"][-1])
        assert torch.equal(r["x_rec"].to(F64), x[:, :c.C]), fast
        for key in ("y", "a2", "scale", "ld_rows", "dp", "dc", "dbias"):
            for k in range(len(layers)):
                assert torch.equal(r[key][k].to(F64), ws[key][k]), (key, k, fast)
        assert torch.equal(r["dx"].to(F64), ws["dx"])


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_exact_operands_separate_an_addressing_error(order):
    """every one of the six taps moved by one position in any direction changes the hidden activations; two hidden columns of W2 swapped or
    the conditioning columns dropped change mu -- in the single-layer operands and in every layer of the chained ones"""
    sets = [X.layer_operands(X.LCase("bf16", order, C, C, Cc, 16, False, 2), True) for C, Cc in ((8, 8), (64, 128), (2, 8))]
    uc = X.UCase(8, 8, 8, 2, 8)
    ul, ux, ucond, _, _ = X.unit_operands(uc, True)
    uws = X.chain(ul, ux, ucond)
    sets += [([L], uws["x"][k], ucond, None, None) for k, L in enumerate(ul) if L.order == order]
    for layers, x, cond, _, _ in sets:
        L = layers[0]
        C = L.W1.shape[1]
        a = X.shiftconv_ref(x[:, :C], L.W1, order)[0]
        for tap in range(6):
            for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                assert not torch.equal(X.shiftconv_ref(x[:, :C], L.W1, order, moved=(tap, dy, dx))[0], a), (tap, dy, dx)
        a2 = torch.cat([a, cond], 1)
        mu = X.params_ref(a2, L.W2, L.b2)[0]
        H = 4 * C
        hid = L.W2[:C, :H] != 0                      # two columns that different mu rows read
        r0 = int(torch.nonzero(hid.any(1))[0])
        i = int(torch.nonzero(hid[r0])[0])
        j = int(torch.nonzero(hid.any(0) & ~hid[r0])[0])
        sw = L.W2.clone(); sw[:, [i, j]] = sw[:, [j, i]]
        assert not torch.equal(X.params_ref(a2, sw, L.b2)[0], mu)
        nc = L.W2.clone(); nc[:, H:] = 0
        assert not torch.equal(X.params_ref(a2, nc, L.b2)[0], mu)


# ------------------------------------------------------------------ the inexact family
@pytest.mark.parametrize("c", ALL_CASES, ids=IDS(ALL_CASES))
def test_inexact_operands_meet_their_conditions(c):
    layers, x, cond, dy, dld = operands(c, False)
    ws = X.chain(layers, x, cond)
    for k, L in enumerate(layers):
        s, pre = ws["s"][k], ws["c"][k]
        assert float(s.abs().max()) <= 4.0, (k, float(s.abs().max()))
        neg = float((pre < 0).double().mean())
        assert 0.1 <= neg <= 0.9, (k, neg)
        assert bool(((pre < 0) & (pre > -0.05)).any()), "no small negative pre-activation"
        if L.ls is not None:
            assert bool((L.ls > 0).any()) and bool((L.ls < 0).any())
        tdt = X.TDT[c.dt]
        assert torch.equal(X.rnd(L.W1, tdt), L.W1) and torch.equal(X.rnd(L.W2, tdt), L.W2)
    assert torch.equal(X.rnd(cond, X.TDT[c.dt]), cond) and torch.equal(X.f32r(x), x)


# ------------------------------------------------------------------ the yardsticks
def measure(c, fast):
    """worst error per quantity of the fp32 restatement against float64, teacher-forced on the restatement's own stored values"""
    layers, x, cond, dy, dld = operands(c, False)
    parts = c.slot_w if isinstance(c, X.LCase) else 1
    r = X.chain(layers, x, cond, dy=dy, dld=dld, tdt=X.TDT[c.dt], cdt=F32, fast=fast)
    st = X.as_stored(r, c.dt, c.B, parts)
    tally = X.Tally(c.dt, fast, enforce=False)
    X.check_forward(layers, cond, st, tally, parts)
    X.check_backward(layers, st, dy[:, :c.C], dld, tally)
    if isinstance(c, X.LCase):
        y = st["y"][0].to(F64)
        L0 = layers[0]._replace(ls=None, pb=None)
        xr = X.inverse_layer(y.to(F32), X.Layer(L0.order, L0.W1.to(F32), L0.W2.to(F32), L0.b2.to(F32), None, None), cond.to(F32), X.TDT[c.dt], fast)
        X.check_inverse_residual(L0, cond, y, xr, tally)
    else:                                                  # the fused inverse, one layer (and its ActNorm) at a time
        for L in layers[:4]:
            y = X.f32r(X.chain([L], x, cond)["y"][0])
            xr = X.chain([L], x, cond, tdt=X.TDT[c.dt], cdt=F32, fast=fast, inverse_of=y)["x_rec"]
            X.check_inverse_residual(L, cond, y, xr, tally)
    return tally.worst


def test_yardsticks(capsys):
    """(on one thread: the blocking of the CPU's fp32 matrix products, and with it the restatement's rounding, follows the thread count)"""
    worst = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for c in ALL_CASES:
            fast = not isinstance(c, X.LCase)
            for name, v in measure(c, fast).items():
                key = X.ykey(name, c.dt, fast)
                worst[key] = max(worst.get(key, 0.0), v)
    finally:
        torch.set_num_threads(threads)
    with capsys.disabled():
        print("\nmeasured yardsticks:", {k: round(v, 2) for k, v in sorted(worst.items())})
    missing = set(YARDSTICK) - set(worst)
    assert not missing, missing
    for key, v in worst.items():
        assert v <= YARDSTICK[key], (key, v, YARDSTICK[key])


# ------------------------------------------------------------------ the bounds see an error at a single position
SEPARATION = [(LAYER_CASES[0], False), (LAYER_CASES[10], False), (UNIT_CASES[0], True)]


@pytest.mark.parametrize("c,fast", SEPARATION, ids=[c.id for c, _ in SEPARATION])
def test_the_checkers_see_one_wrong_element(c, fast):
    """the restatement's stored tensors pass the teacher-forced checkers at the GPU bounds; with ONE element of one tensor moved -- by
    four bf16 ulps where it is stored as bf16, by 2^-16 of its value where it is fp32 -- or one conditioning / padding element set, the
    checkers raise"""
    layers, x, cond, dy, dld = operands(c, False)
    parts = c.slot_w if isinstance(c, X.LCase) else 1
    r = X.chain(layers, x, cond, dy=dy, dld=dld, tdt=X.TDT[c.dt], cdt=F32, fast=fast)
    good = X.as_stored(r, c.dt, c.B, parts)

    def run(ws):
        tally = X.Tally(c.dt, fast)
        X.check_forward(layers, cond, ws, tally, parts)
        X.check_backward(layers, ws, dy[:, :c.C], dld, tally)

    run(good)
    k = len(layers) - 1
    H = 4 * c.C
    for key in ("a2", "scale", "y", "slots", "dp", "dc", "dbias", "post_part", "dx"):
        if key == "post_part" and layers[k].ls is None:
            continue
        bad = dict(good)
        t = (good[key] if key == "dx" else good[key][k]).clone()
        v = t[:, :H] if key == "a2" else t[:, :2 * c.C] if key == "dp" else t
        i = int(torch.argmax(v.abs().reshape(-1).float()))
        row, col = divmod(i, v.shape[1])
        rel = 2.0 ** -5 if t.dtype == BF16 and c.dt == "bf16" else 2.0 ** -16
        t[row, col] = (t[row, col].double() * (1.0 + rel)).to(t.dtype)
        bad[key] = t if key == "dx" else [t if j == k else u for j, u in enumerate(good[key])]
        with pytest.raises(AssertionError):
            run(bad)
    for key, col in (("a2", H), ("a2", H + c.Cc - 1), ("dp", 2 * c.C - 1)):
        bad = dict(good)
        t = good[key][k].clone()
        t[3, col] = t[3, col] + 1.0
        bad[key] = [t if j == k else u for j, u in enumerate(good[key])]
        with pytest.raises(AssertionError):
            run(bad)
    for key in ("a2", "dp", "dc"):                          # the zero padding the weight-gradient GEMMs read
        t = good[key][k]
        first = {"a2": H + c.Cc, "dp": 2 * c.C, "dc": H}[key]
        pad = torch.cat([t, torch.zeros(t.shape[0], 8, dtype=t.dtype)], 1)
        pad[5, first] = 1.0
        bad = dict(good)
        bad[key] = [pad if j == k else u for j, u in enumerate(good[key])]
        with pytest.raises(AssertionError):
            run(bad)
