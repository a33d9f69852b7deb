"""CPU: pins what test_gru_kernels_gpu.py relies on -- the float64 references of tests/gru_exact.py against autograd through the oracle's
ConvGRU, the recorded yardsticks, that the bounds separate the defects the suite exists for, that the exact operand set is exact --
and checks the host-side hooks of the unroll (workspace layout, the form decision and its LDS condition) and the argument checks."""
import ctypes
import re
from ctypes import byref

import pytest
import torch

from ipoke_amd import _lib
from oracle import vae_ref
from tests import gru_exact as X
from tests.gru_exact import F32, F64, YARDSTICK, Case

CASE_IDS = lambda cs: [c.id for c in cs]                                                      # noqa: E731


def lib():
    return _lib.lib()


def err():
    return lib().ipoke_last_error().decode()


# ------------------------------------------------------------------ the references against the oracle
@pytest.mark.parametrize("geom", [(2, 3, 2, 8, 8, 4, 4), (1, 2, 1, 4, 8, 2, 4), (2, 2, 3, 8, 8, 8, 8), (1, 1, 1, 8, 8, 4, 4)])
def test_unforced_reference_equals_autograd_through_the_oracle(geom):
    """the phases chained in float64 without any rounding against torch autograd through oracle.vae_ref.ConvGRU driven as
    SpadeCondMotionModel.forward drives it: the output sequence, d x0, d h0 (summed over the cells), every weight and bias gradient"""
    from ipoke_amd import autograd_ops as FT
    c = Case(*geom, "f32", 0, True, 0)
    B, T, L, Cx, Ch, H, W = geom
    ops = X.operands(c, False)
    ref = vae_ref.ConvGRU(Cx, Ch, L).double()
    with torch.no_grad():
        for l, cell in enumerate(ref.cells):
            w_ur, b_ur, w_o, b_o = ops["w"][4 * l: 4 * l + 4]
            cell.update_gate.weight.copy_(w_ur[:Ch]); cell.reset_gate.weight.copy_(w_ur[Ch:])
            cell.update_gate.bias.copy_(b_ur[:Ch]); cell.reset_gate.bias.copy_(b_ur[Ch:])
            cell.out_gate.weight.copy_(w_o); cell.out_gate.bias.copy_(b_o)
            gw, gb = FT.gru_gate_weights(cell)                    # the update-rows-first order of the unroll's w_ur
            assert torch.equal(gw, w_ur) and torch.equal(gb, b_ur)
    x = X.to_map(ops["x0"], H, W).clone().requires_grad_(True)
    h0 = X.to_map(ops["h0"], H, W).clone().requires_grad_(True)
    hidden, outs = [h0] * L, []
    for _ in range(T):
        hidden = ref(x, hidden)
        outs.append(hidden[-1])
    seq = torch.stack(outs, 0)
    seq.backward(torch.stack([X.to_map(ops["dout"][t], H, W) for t in range(T)], 0))
    got = X.unroll(c, ops)

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), what

    for t in range(T):
        same(got["out"][t], X.to_rows(seq[t].detach()), f"out[{t}]")
    same(got["dx0"], X.to_rows(x.grad), "d x0")
    same(got["dh0"], X.to_rows(h0.grad), "d h0")
    for l, cell in enumerate(ref.cells):
        dw_ur, db_ur, dw_o, db_o = got["dw"][4 * l: 4 * l + 4]
        same(dw_ur, torch.cat([cell.update_gate.weight.grad, cell.reset_gate.weight.grad], 0), f"d w_ur of cell {l}")
        same(db_ur, torch.cat([cell.update_gate.bias.grad, cell.reset_gate.bias.grad]), f"d b_ur of cell {l}")
        same(dw_o, cell.out_gate.weight.grad, f"d w_o of cell {l}")
        same(db_o, cell.out_gate.bias.grad, f"d b_o of cell {l}")


def test_teacher_forced_checkers_accept_the_unforced_reference():
    """on the float64 unroll as the workspace, every phase check reproduces its input to rounding noise of float64: the checkers and the
    chained reference are the same function"""
    c = Case(2, 3, 3, 8, 8, 4, 4, "f32", 0, True, 0)
    ops = X.operands(c, False)
    ws = X.unroll(c, ops)
    tl = X.Tally("f32", enforce=False)
    X.check_forward(c, ops, ws, tl)
    X.check_backward(c, ops, ws, tl)
    assert set(tl.worst) == set(X.PHASES) | set(X.FP32_OUT)
    assert max(tl.worst.values()) < 1e-3, tl.worst              # fp32 units


def test_dgrad_and_wgrad_refs_are_the_adjoints_of_conv_ref():
    gen = torch.Generator().manual_seed(3)
    a, w, dy = (torch.randn(s, generator=gen, dtype=F64) for s in ((2 * 4 * 8, 6), (5, 6, 3, 3), (2 * 4 * 8, 5)))
    y = X.conv_ref(a, w, None, 4, 8)[0]
    lhs = float((y * dy).sum())
    assert abs(lhs - float((a * X.dgrad_ref(dy, w, 4, 8)[0]).sum())) <= 1e-10 * abs(lhs)
    assert abs(lhs - float((w * X.wgrad_ref(a, dy, 4, 8)[0]).sum())) <= 1e-10 * abs(lhs)
    assert abs(lhs - float((a * X.dgrad_ref(dy, w, 4, 8, mirror=False)[0]).sum())) > 1e-3 * abs(lhs)


# ------------------------------------------------------------------ yardsticks
def measured():
    """worst error of the restatement (float32, rounded to the storage type where the kernels store) per phase, in the units of
    gru_exact's table, on the inexact operands of every case of the GPU tests"""
    w = {k: 0.0 for k in YARDSTICK}
    for c in X.ALL_CASES:
        ops = X.operands(c, False)
        ws = X.unroll(c, ops, X.TDT[c.dt], F32)
        tl = X.Tally(c.dt, enforce=False)
        X.check_forward(c, ops, ws, tl)
        X.check_backward(c, ops, ws, tl)
        for k, v in tl.worst.items():
            w[f"{k}_{c.dt}"] = max(w[f"{k}_{c.dt}"], v)
    for dt in ("f32", "bf16"):                                   # the operands of the stand-alone entry points' tests
        for Ch in X.STANDALONE_CH:
            o = X.standalone_operands(Ch, dt, False)
            for given in (True, False):
                ref = X.standalone_phases(o, Ch, given)
                got = X.standalone_phases({k: v.to(F32) for k, v in o.items()}, Ch, given)
                tl = X.Tally(dt, enforce=False)
                for k in ref:
                    tl.cmp(k, X.rnd(got[k][0], X.TDT[dt]), *ref[k])
                    w[f"{k}_{dt}"] = max(w[f"{k}_{dt}"], tl.worst[k])
    return w


def test_restatements_stay_within_the_recorded_yardsticks():
    w = measured()
    for k in sorted(w):
        name, dt = k.rsplit("_", 1)
        print(f"yardstick {k:14s} measured {w[k]:7.3f}  recorded {YARDSTICK[k]:5.2f}  GPU bound {X.gpu_bound(name, dt):5.1f}")
    assert set(YARDSTICK) == {f"{n}_{dt}" for n in X.PHASES + X.FP32_OUT for dt in ("f32", "bf16")}
    over = {k: (v, YARDSTICK[k]) for k, v in w.items() if not v <= YARDSTICK[k]}
    assert not over, f"(measured, recorded) {over}"
    # the recorded values are the measured ones rounded up, not padded: at most twice the measurement or half a unit above it
    slack = {k: (v, YARDSTICK[k]) for k, v in w.items() if YARDSTICK[k] > max(2.0 * v, v + 0.5)}
    assert not slack, f"(measured, recorded) {slack}"
    # a value rounded to bf16 is bounded by ONE unit on the device: the restatement has to stay below it
    assert all(YARDSTICK[f"{n}_bf16"] < 1.0 for n in X.PHASES)
    # the table of the module docstring is the recorded dict
    for n in X.PHASES + X.FP32_OUT:
        assert re.search(rf"\b{n}\s+{YARDSTICK[n + '_f32']}\s+{YARDSTICK[n + '_bf16']}(\s|$)", X.__doc__, flags=re.M), n


# ------------------------------------------------------------------ separation
MUTATIONS = [("tap", "ur"), ("mirror", "dur_r"), ("swap", "u"), ("gsrc", "do"), ("dx0_last", "dx0"), ("dh0_cell", "dh0")]


@pytest.mark.parametrize("c", X.SEPARATION_CASES, ids=CASE_IDS(X.SEPARATION_CASES))
@pytest.mark.parametrize("mut,target", MUTATIONS, ids=[m for m, _ in MUTATIONS])
def test_bounds_separate_the_defects_the_suite_exists_for(c, mut, target):
    """a workspace computed WITH one defect (a border tap of one cell's weight dropped in the forward convolution, the tap mirror omitted
    in one data-gradient operand, the u and r halves swapped, one of the gradient sources of g dropped, the last contribution to d x0
    dropped, one cell dropped from d h0) misses the GPU bound at the check that targets it, on the GPU test's own operands -- and the
    same workspace without the defect passes every check.  No kernel runs."""
    ops = X.operands(c, False)
    tdt = X.TDT[c.dt]
    good = X.Tally(c.dt, enforce=True)
    ws = X.unroll(c, ops, tdt, F32)
    X.check_forward(c, ops, ws, good)
    X.check_backward(c, ops, ws, good)
    bad = X.Tally(c.dt, enforce=False)
    ws = X.unroll(c, ops, tdt, F32, mut=mut)
    X.check_forward(c, ops, ws, bad)
    X.check_backward(c, ops, ws, bad)
    bound = X.gpu_bound(target, c.dt)
    print(f"{c.id} {mut}: {target} {bad.worst[target]:.1f} units against a bound of {bound}")
    assert bad.worst[target] > 2.0 * bound
    with pytest.raises(AssertionError, match=rf"^{target} "):
        enforce = X.Tally(c.dt, enforce=True)
        X.check_forward(c, ops, ws, enforce)
        X.check_backward(c, ops, ws, enforce)


# ------------------------------------------------------------------ the exact operand set
@pytest.mark.parametrize("c", X.ALL_CASES, ids=CASE_IDS(X.ALL_CASES))
def test_exact_operand_set_is_exact(c):
    """the float32 / storage-type restatement equals the float64 reference bit for bit, every stored value is an integer small enough for
    the type, and the buffers have the closed forms of gru_exact's docstring"""
    ops = X.operands(c, True)
    tdt = X.TDT[c.dt]
    ref = X.unroll(c, ops)
    res = X.unroll(c, ops, tdt, F32)
    X.assert_exact(c, res, ref, backward=True)
    for k in ("XH", "XHR", "UR", "O", "DO", "DUR", "DU", "DH1", "DH2", "G"):
        for row in ref[k]:
            for v in row:
                assert bool((v == v.round()).all()) and torch.equal(X.rnd(v, tdt), v), k      # integers the type holds
    for l in range(c.L):
        for t in range(c.T):
            cx = c.Cx if l == 0 else c.Ch
            assert bool((ref["U"][l][t] == 0.5).all()) and bool((ref["O"][l][t] == 0).all()) and bool((ref["UR"][l][t] == 0).all())
            assert torch.equal(ref["HN"][l][t], ops["h0"] / 2.0 ** (t + 1))
            assert torch.equal(ref["XHR"][l][t][:, cx:] * 2, ref["XH"][l][t][:, cx:])
            g = ref["G"][l][t]
            assert bool((g == 0).all()) == (l + 1 < c.L)
            assert torch.equal(ref["DO"][l][t], g / 2) and torch.equal(ref["DUR"][l][t][:, :c.Ch] * 4, -g * ref["XH"][l][t][:, cx:])
            assert bool((ref["DUR"][l][t][:, c.Ch:] == 0).all())
    assert bool((ref["dx0"] == 0).all()) and torch.equal(ref["dh0"], ref["G"][c.L - 1][0] / 2)
    # weight gradients: zero below the last cell, sums of integer products below 2^24 in the last
    for l in range(c.L):
        for j in range(4):
            v = ref["dw"][4 * l + j]
            assert bool((v == v.round()).all()) and bool((v != 0).any()) == (l == c.L - 1)
    a = torch.cat([v.abs() for v in ref["XH"][c.L - 1]], 0)
    d = torch.cat([v.abs() for v in ref["DUR"][c.L - 1]], 0)
    assert float(X.wgrad_ref(a, d, c.H, c.W)[0].max()) < 2.0 ** 24


# ------------------------------------------------------------------ the workspace layout hook
@pytest.mark.parametrize("c", X.ALL_CASES, ids=CASE_IDS(X.ALL_CASES))
def test_workspace_layout(c):
    lay = X.layout(c)
    d = c.desc()
    code, _, e16 = X.DTYPES[c.dt]
    esz = 16 // e16
    assert lay["bytes"] == lib().ipoke_gru_workspace_bytes(byref(d), code)
    names = ("XH", "XHR", "UR", "U", "O", "DO", "DUR")
    want = {"XH": c.Kc, "XHR": c.Kc, "UR": X.round_up(2 * c.Ch, e16), "U": c.Ch, "O": X.round_up(c.Ch, e16), "DO": X.round_up(c.Ch, e16),
            "DUR": X.round_up(2 * c.Ch, e16)}
    end = 0
    for k in names:
        off, wd = lay[k]
        assert wd == want[k] and off % 256 == 0 and off >= end, k             # 256-byte aligned, ascending, no overlap
        end = off + c.L * c.T * c.M * wd * esz
    assert lay["WOP"] % 256 == 0 and lay["WOP"] >= end and lay["wop_cell"] % 256 == 0
    o = lay["wop"]
    assert 0 == o["ur"] < o["urT"] < o["o"] < o["oT"] < lay["wop_cell"] and all(v % 256 == 0 for v in o.values())
    assert o["urT"] >= 2 * c.Ch * 9 * c.Kc * esz and o["o"] - o["urT"] >= c.Kc * 9 * 2 * c.Ch * esz and o["oT"] - o["o"] >= c.Ch * 9 * c.Kc * esz
    assert lay["wop_cell"] - o["oT"] >= c.Kc * 9 * c.Ch * esz
    assert lay["WOP"] + c.L * lay["wop_cell"] <= lay["bytes"]


def _desc(B, T, L, Cx, Ch, H, W):
    d = _lib.GruDesc()
    d.B, d.T, d.L, d.Cx, d.Ch, d.H, d.W = B, T, L, Cx, Ch, H, W
    return d


BAD_DESCS = [((2, 3, 2, 32, 32, 6, 8), "map extents must be powers of two"), ((2, 3, 2, 32, 32, 8, 12), "map extents must be powers of two"),
             ((2, 3, 2, 32, 64, 8, 8), "stacked cells take the hidden state of the cell below"), ((2, 3, 17, 32, 32, 8, 8), "bad geometry"),
             ((0, 3, 1, 32, 32, 8, 8), "bad geometry"), ((2, 3, 1, 12, 32, 8, 8), "channel counts must be multiples of 16 bytes")]


@pytest.mark.parametrize("geom,msg", BAD_DESCS)
def test_bad_descriptors_are_rejected_by_every_host_entry_point(geom, msg):
    d = _desc(*geom)
    out = (ctypes.c_int64 * 21)()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    arr = (ctypes.c_void_p * 68)(*([a] * 68))
    assert lib().ipoke_gru_workspace_bytes(byref(d), _lib.BF16) == -1
    assert lib().ipoke_gru_workspace_layout(byref(d), _lib.BF16, out, 21) == -1 and msg in err()
    assert lib().ipoke_gru_fused_applicable(byref(d), _lib.BF16, 64, 64, 64, a, a, a, X.LDS_LIMIT) == -1 and msg in err()
    assert lib().ipoke_gru_unroll_forward(byref(d), a, 64, a, 64, arr, a, a, 64, _lib.BF16, None) == -1 and msg in err()
    assert lib().ipoke_gru_unroll_backward(byref(d), a, 64, a, arr, a, a, _lib.BF16, None) == -1 and msg in err()


def test_layout_hook_argument_checks():
    d = _desc(2, 3, 2, 32, 32, 8, 8)
    out = (ctypes.c_int64 * 21)()
    assert lib().ipoke_gru_workspace_layout(None, _lib.BF16, out, 21) == -1 and "bad geometry" in err()
    assert lib().ipoke_gru_workspace_layout(byref(d), 7, out, 21) == -1 and "bad dtype" in err()
    assert lib().ipoke_gru_workspace_layout(byref(d), _lib.BF16, None, 21) == -1
    assert lib().ipoke_gru_workspace_layout(byref(d), _lib.BF16, out, 20) == -1
    assert lib().ipoke_gru_workspace_form(ctypes.addressof(out)) == -1          # no forward pass on record


# ------------------------------------------------------------------ the form decision
def applicable(Ch, L, dt="bf16", Cx=None, H=8, W=8, ldx=None, ldh=None, ldo=None, x0=4096, h0=8192, out=16384, limit=X.LDS_LIMIT):
    Cx = Ch if Cx is None else Cx
    d = _desc(2, 3, L, Cx, Ch, H, W)
    rc = lib().ipoke_gru_fused_applicable(byref(d), X.DTYPES[dt][0], Cx if ldx is None else ldx, Ch if ldh is None else ldh,
                                          Ch if ldo is None else ldo, x0, h0, out, limit)
    assert rc in (0, 1), err()
    return rc == 1


def lds_bytes(Ch, L):
    """the two dynamic-LDS carve-ups, from the buffers the kernels' comments list (Kc = 2 Ch, tile rows of 2 Kc + 32 resp. 2 Ch + 32 bytes)"""
    Kc = 2 * Ch
    fwd = 4 * 65 * (2 * Kc + 32) + (L * 64 * Ch + 2 * 64 * Ch) * 2 + L * 3 * Ch * 4
    bwd = 65 * (2 * Ch + 32) + 65 * (2 * Kc + 32) + (64 * Kc + 64 * Ch + L * 2 * 64 * Ch) * 2 + 64 * Ch * 4
    return fwd, bwd


def test_fused_form_needs_the_lds_of_both_directions():
    assert lds_bytes(64, 5) == (136064, 152000) and lds_bytes(64, 6) == (145024, 168384) and lds_bytes(64, 9)[0] == 171904
    assert lds_bytes(32, 15) == (116992, 160000) and lds_bytes(32, 16) == (121472, 168192)
    for L in range(1, 17):
        assert applicable(64, L) == (L <= 5), L
        assert applicable(32, L) == (L <= 15), L
        for Ch in (32, 64):
            for limit in (65536, 100000, 140000, 163840, 1 << 20):
                assert applicable(Ch, L, limit=limit) == (max(lds_bytes(Ch, L)) <= limit), (Ch, L, limit)
    assert not any(applicable(Ch, L, limit=65536) for Ch in (32, 64) for L in range(1, 17) if max(lds_bytes(Ch, L)) > 65536)
    assert applicable(32, 1, limit=65536) == (max(lds_bytes(32, 1)) <= 65536)
    for c in X.ALL_CASES:                                        # the intended form of every case of the GPU tests
        e16 = X.DTYPES[c.dt][2]
        assert applicable(c.Ch, c.L, c.dt, c.Cx, c.H, c.W, c.Cx + c.pad, c.Ch + c.pad, c.Ch + c.pad) == (c.form == 1 or
                                                                                                         (c.force0 and c in X.PHASE_CASES[:2])), c.id
        assert e16 and (c.pad * (16 // e16)) % 16 == 0


def test_fused_form_conditions_other_than_lds():
    assert applicable(64, 4) and applicable(32, 4)
    assert not applicable(32, 2, dt="f32", ldx=32, ldh=32, ldo=32)
    assert not applicable(32, 2, H=4, W=8) and not applicable(32, 2, H=8, W=16) and not applicable(32, 2, H=16, W=16)
    assert not applicable(32, 1, Cx=64) and not applicable(64, 1, Cx=32)
    assert not applicable(16, 2) and not applicable(128, 1)
    assert applicable(32, 2, ldx=40, ldh=48, ldo=36)
    assert not applicable(32, 2, ldx=36) and not applicable(32, 2, ldh=44) and not applicable(32, 2, ldo=34)
    assert not applicable(32, 2, x0=4096 + 8) and not applicable(32, 2, h0=8192 + 2) and not applicable(32, 2, out=16384 + 4)
    assert applicable(32, 2, out=16384 + 8)
    d = _desc(2, 3, 2, 32, 32, 8, 8)
    assert lib().ipoke_gru_fused_applicable(byref(d), _lib.BF16, 24, 32, 32, 4096, 4096, 4096, X.LDS_LIMIT) == -1 and "bad arguments" in err()


# ------------------------------------------------------------------ argument checks that need no device
def test_unroll_argument_checks():
    d = _desc(2, 3, 2, 32, 32, 8, 8)
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    arr = (ctypes.c_void_p * 8)(*([a] * 8))
    fwd, bwd = lib().ipoke_gru_unroll_forward, lib().ipoke_gru_unroll_backward
    for args in ((None, 32, a, 32, arr, a, a, 32), (a, 32, None, 32, arr, a, a, 32), (a, 32, a, 32, None, a, a, 32), (a, 32, a, 32, arr, None, a, 32),
                 (a, 32, a, 32, arr, a, None, 32), (a, 24, a, 32, arr, a, a, 32), (a, 32, a, 24, arr, a, a, 32), (a, 32, a, 32, arr, a, a, 24)):
        assert fwd(byref(d), *args, _lib.BF16, None) == -1 and "bad arguments" in err(), args
    assert fwd(byref(d), a, 32, a, 32, arr, a, a, 32, 9, None) == -1 and "bad dtype" in err()
    for args in ((None, 32, a, arr, a, a), (a, 32, None, arr, a, a), (a, 32, a, None, a, a), (a, 32, a, arr, None, a), (a, 32, a, arr, a, None),
                 (a, 24, a, arr, a, a)):
        assert bwd(byref(d), *args, _lib.BF16, None) == -1 and "bad arguments" in err(), args
    assert bwd(byref(d), a, 32, a, arr, a, a, _lib.BF16, None) == -1 and "no forward pass on record" in err()


def test_standalone_entry_points_reject_null_tensors():
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    L = lib()
    for i in (0, 1, 3, 5):
        args = [a, a, 8, a, 8, a, 4, 4, _lib.F32, None]
        args[i] = None
        assert L.ipoke_gru_gates(*args) == -1 and "null tensor" in err(), i
    for i in (0, 1, 2, 4):
        args = [a, a, a, 8, a, 8, 4, 4, _lib.F32, None]
        args[i] = None
        assert L.ipoke_gru_update(*args) == -1 and "null tensor" in err(), i
    for i in (0, 1, 2, 4, 6, 7, 8):
        args = [a, a, a, 8, a, 8, a, a, a, 8, 4, 4, _lib.F32, None]
        args[i] = None
        assert L.ipoke_gru_update_bwd(*args) == -1 and "null tensor" in err(), i
    for i in (0, 1, 3, 6, 7):                                    # d_u (argument 5) may be null
        args = [a, a, 8, a, 8, a, a, a, 8, 4, 4, _lib.F32, None]
        args[i] = None
        assert L.ipoke_gru_gates_bwd(*args) == -1 and "null tensor" in err(), i


def test_tile_operand_refs_are_permutations_with_the_documented_first_fragment():
    """the index maps of the two fragment-tiling kernels' comments: every weight element exactly once; lane l of fragment (0, 0) holds the
    8 consecutive k = 8 (l >> 4) .. of output column l & 15, k = tap Kc + channel -- mirrored taps and swapped roles in the transposed one"""
    N, Kc = 64, 64
    w = torch.arange(N * Kc * 9, dtype=F64).reshape(N, Kc, 3, 3)
    for fn in (X.tile_operand_ref, X.tile_operand_t_ref):
        t = fn(w, F32).to(torch.int64)
        assert sorted(t.tolist()) == list(range(N * Kc * 9))
    t = X.tile_operand_ref(w, F32)
    assert [int(v) for v in t[:8]] == [int(w[0, k, 0, 0]) for k in range(8)] and int(t[8]) == int(w[1, 0, 0, 0])
    assert int(t[16 * 8]) == int(w[0, 8, 0, 0]) and int(t[512 * 2]) == int(w[0, 0, 0, 1])          # lane 16: k = 8; K step 2 = tap 1
    t = X.tile_operand_t_ref(w, F32)
    assert [int(v) for v in t[:8]] == [int(w[n, 0, 2, 2]) for n in range(8)] and int(t[8]) == int(w[0, 1, 2, 2])
    assert int(t[512 * 2]) == int(w[0, 0, 2, 1])
