"""The ConvGRU unroll phase by phase against the float64 references of tests/gru_exact.py: ipoke_gru_unroll_forward / _backward driven
through ctypes in both forms, every phase of every (cell, step) checked on the operands the kernels themselves stored in the workspace
(teacher forcing), the exact operand set bit for bit; the fragment-tiled operands of the fused kernels; the four stand-alone cell entry
points.  Every test asserts the form the call took, and every buffer is guarded by sentinels."""
import ctypes
from ctypes import byref

import pytest
import torch

from ipoke_amd import _lib
from ipoke_amd._lib import ptr
from tests import gru_exact as X
from tests.gru_exact import DTYPES, F32, F64, SENT, assert_same, canon, check_guard, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = pytest.mark.parametrize("exact", [True, False], ids=["exact", "inexact"])
WS_FILL, WS_TAIL = 0x45, 4096             # the workspace starts as bytes of 0x45 (3156.3 in either type) and has a tail of them


def lib():
    return _lib.lib()


def run(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def flat(n, tail=64):
    return torch.full((n + tail,), SENT, dtype=F32, device=DEV)


class Unroll:
    """the buffers of one forward + backward call of a case, as first_stage_train.gru_unroll_forward / _GruUnrollFn.backward set them up"""

    def __init__(self, c, ops, ldo=None):
        self.c, self.ops, self.lay = c, ops, X.layout(c)
        self.code, self.tdt, _ = DTYPES[c.dt]
        self.ldx, self.ldh, self.ldo = c.Cx + c.pad, c.Ch + c.pad, (c.Ch + c.pad) if ldo is None else ldo
        self.x0 = guarded(c.M, self.ldx, self.tdt, DEV, ops["x0"].to(DEV))
        self.h0 = guarded(c.M, self.ldh, self.tdt, DEV, ops["h0"].to(DEV))
        self.dout = guarded(c.T * c.M, self.ldo, self.tdt, DEV, ops["dout"].reshape(c.T * c.M, c.Ch).to(DEV))
        self.out = guarded(c.T * c.M, self.ldo, self.tdt, DEV)
        self.ws = torch.full((self.lay["bytes"] + WS_TAIL,), WS_FILL, dtype=torch.uint8, device=DEV)
        self.w = [v.to(F32).to(DEV).contiguous() for v in ops["w"]]
        self.warr = (ctypes.c_void_p * len(self.w))(*[v.data_ptr() for v in self.w])
        self.dw = [flat(v.numel()) for v in self.w]
        self.dwarr = (ctypes.c_void_p * len(self.dw))(*[v.data_ptr() for v in self.dw])
        self.dx0 = guarded(c.M, c.Cx, F32, DEV)
        self.dh0 = guarded(c.M, c.Ch, F32, DEV)
        self.inputs = [t.clone() for t in (self.x0, self.h0, self.dout, *self.w)]
        self.d = c.desc()

    def form(self):
        return lib().ipoke_gru_workspace_form(ptr(self.ws))

    def forward(self):
        c = self.c
        try:
            _lib.check(lib().ipoke_gru_set_fused(0 if c.force0 else 1))
            run(lib().ipoke_gru_unroll_forward(byref(self.d), ptr(self.x0), self.ldx, ptr(self.h0), self.ldh, self.warr, ptr(self.ws), ptr(self.out),
                                               self.ldo, self.code, _lib.current_stream()))
        finally:
            _lib.check(lib().ipoke_gru_set_fused(-1))

    def backward(self):
        return lib().ipoke_gru_unroll_backward(byref(self.d), ptr(self.dout), self.ldo, ptr(self.ws), self.dwarr, ptr(self.dx0), ptr(self.dh0),
                                               self.code, _lib.current_stream())

    def read(self, backward):
        """the workspace and the outputs as gru_exact's checkers take them (CPU)"""
        c = self.c
        host = self.ws.cpu()
        ws = X.read_workspace(host, c, self.lay, ("XH", "XHR", "UR", "U", "O") + (("DO", "DUR") if backward else ()))
        o = self.out[: c.T * c.M, : c.Ch].cpu().reshape(c.T, c.M, c.Ch)
        ws["out"] = [o[t].contiguous() for t in range(c.T)]
        if backward:
            ws["dx0"], ws["dh0"] = self.dx0[: c.M].cpu(), self.dh0[: c.M].cpu()
            ws["dw"] = [b[: v.numel()].cpu().reshape(v.shape) for b, v in zip(self.dw, self.w)]
        return ws, host

    def guards(self, backward):
        c = self.c
        assert bool((self.ws[self.lay["bytes"]:] == WS_FILL).all()), "write behind the workspace"
        check_guard(self.out, c.T * c.M, c.Ch, None, "out")
        for t, was, name in zip((self.x0, self.h0, self.dout, *self.w), self.inputs, ("x0", "h0", "d_out") + ("weight",) * len(self.w)):
            assert torch.equal(t.view(torch.uint8), was.view(torch.uint8)), f"{name} was written (padding and guard rows included)"
        if backward:
            check_guard(self.dx0, c.M, c.Cx, None, "d_x0")
            check_guard(self.dh0, c.M, c.Ch, None, "d_h0")
            for i, (b, v) in enumerate(zip(self.dw, self.w)):
                assert bool((b[v.numel():] == SENT).all()), f"write behind gradient tensor {i}"
        else:
            assert bool((self.dx0 == SENT).all()) and bool((self.dh0 == SENT).all()) and all(bool((b == SENT).all()) for b in self.dw)


def check_tiled_operands(u, host):
    """gru_tile_operand_kernel / gru_tile_operand_t_kernel through the workspace slots the fused forward pass filled: every element is the
    bf16 rounding of the weight element the layout comments name"""
    c, lay = u.c, u.lay
    for l in range(c.L):
        w_ur, w_o = u.ops["w"][4 * l], u.ops["w"][4 * l + 2]
        base = lay["WOP"] + l * lay["wop_cell"]
        for slot, ref in (("ur", X.tile_operand_ref(w_ur)), ("urT", X.tile_operand_t_ref(w_ur)), ("o", X.tile_operand_ref(w_o)),
                          ("oT", X.tile_operand_t_ref(w_o))):
            off = base + lay["wop"][slot]
            got = host[off: off + 2 * ref.numel()].clone().view(torch.bfloat16)
            assert_same(got, ref, f"fragment-tiled operand {slot} of cell {l}", lambda i: f"fragment {i >> 9} lane {(i >> 3) & 63} element {i & 7}")


def unroll_case(c, exact):
    ops = X.operands(c, exact)
    u = Unroll(c, ops)
    u.forward()
    assert u.form() == c.form, f"the forward pass took form {u.form()}, the case is meant for form {c.form}"
    ws, host = u.read(False)
    u.guards(False)
    X.check_routing(c, ops, ws)
    ref = X.unroll(c, ops) if exact else None
    if exact:
        X.assert_exact(c, ws, ref, backward=False)
    else:
        tl = X.Tally(c.dt)
        X.check_forward(c, ops, ws, tl)
        print(f"{c.id} forward, worst units: " + ", ".join(f"{k} {v:.2f}" for k, v in tl.worst.items()))
        if c.form == 1:
            check_tiled_operands(u, host)
    run(u.backward())
    assert u.form() == c.form
    ws, host2 = u.read(True)
    u.guards(True)
    end_fwd = u.lay["DO"][0]
    assert torch.equal(host[:end_fwd], host2[:end_fwd]), "the backward pass wrote into the forward pass's operands"
    if exact:
        X.assert_exact(c, ws, ref, backward=True)
    else:
        tl = X.Tally(c.dt)
        X.check_backward(c, ops, ws, tl)
        print(f"{c.id} backward, worst units: " + ", ".join(f"{k} {v:.2f}" for k, v in tl.worst.items()))


def ids(cs):
    return [c.id for c in cs]


@EXACT
@pytest.mark.parametrize("c", X.FUSED_CASES + X.FUSED_PADDED, ids=ids(X.FUSED_CASES + X.FUSED_PADDED))
def test_fused_unroll_phase_by_phase(c, exact):
    unroll_case(c, exact)


@EXACT
@pytest.mark.parametrize("c", X.NOT_FITTING, ids=ids(X.NOT_FITTING))
def test_stack_too_deep_for_the_lds_takes_the_launch_per_phase_form(c, exact):
    """Ch = 64, L = 6: the forward kernel's LDS would fit, the backward kernel's would not -- both directions run launch per phase"""
    unroll_case(c, exact)


@EXACT
@pytest.mark.parametrize("c", X.PHASE_CASES, ids=ids(X.PHASE_CASES))
def test_launch_per_phase_unroll_phase_by_phase(c, exact):
    unroll_case(c, exact)


def test_backward_after_a_fused_forward_rejects_rows_it_cannot_read():
    """ldo = Ch + 4: the fused forward pass can write such rows, the fused backward kernel cannot read them, and the tiled operands leave no
    other form -- the documented error, from the host, before anything is launched"""
    c = X.FUSED_CASES[1]
    u = Unroll(c, X.operands(c, False), ldo=c.Ch + 4)
    u.forward()
    assert u.form() == 1
    torch.cuda.synchronize()
    before = u.ws.clone()
    rc = u.backward()
    torch.cuda.synchronize()
    assert rc == -1 and b"fragment-tiled operands" in lib().ipoke_last_error()
    assert torch.equal(before, u.ws)
    u.guards(False)


# ------------------------------------------------------------------ the stand-alone entry points
def standalone(Ch, dt, exact):
    code, tdt, _ = DTYPES[dt]
    o = X.standalone_operands(Ch, dt, exact)
    M, ld = X.STANDALONE_M, Ch + 3
    b = {k: guarded(M, (ld if k in ("h", "g", "d_hr") else v.shape[1]), tdt, DEV, v.to(DEV)) for k, v in o.items()}
    return o, b, M, ld, code, tdt


def compare(name, dt, exact, buf, M, cols, ref, what):
    got = buf[:M, cols].cpu().contiguous()
    if exact:
        assert_same(canon(got), canon(ref[0].to(got.dtype)), what)
    else:
        tl = X.Tally(dt)
        tl.cmp(name, got, *ref, where=what)


@EXACT
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Ch", X.STANDALONE_CH)
def test_standalone_gates_and_update(Ch, dt, exact):
    o, b, M, ld, code, tdt = standalone(Ch, dt, exact)
    ref = X.standalone_phases(o, Ch)
    hr, u, hn = guarded(M, ld + 1, tdt, DEV), guarded(M, Ch, tdt, DEV), guarded(M, ld + 2, tdt, DEV)
    run(lib().ipoke_gru_gates(ptr(b["ur"]), ptr(b["h"]), ld, ptr(hr), ld + 1, ptr(u), M, Ch, code, _lib.current_stream()))
    compare("u", dt, exact, u, M, slice(0, Ch), ref["u"], "ipoke_gru_gates u")
    compare("hr", dt, exact, hr, M, slice(0, Ch), ref["hr"], "ipoke_gru_gates hr")
    run(lib().ipoke_gru_update(ptr(b["o"]), ptr(b["u"]), ptr(b["h"]), ld, ptr(hn), ld + 2, M, Ch, code, _lib.current_stream()))
    compare("hn", dt, exact, hn, M, slice(0, Ch), ref["hn"], "ipoke_gru_update h'")
    for t, name in ((hr, "hr"), (u, "u"), (hn, "h'")):
        check_guard(t, M, Ch, None, name)
    for k, v in o.items():
        assert torch.equal(b[k][:M, : v.shape[1]].cpu().to(F64), v) and bool((b[k][M:] == SENT).all()), k


@EXACT
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Ch", X.STANDALONE_CH)
def test_standalone_update_bwd_and_gates_bwd(Ch, dt, exact):
    o, b, M, ld, code, tdt = standalone(Ch, dt, exact)
    ref = X.standalone_phases(o, Ch)
    d_o, d_u, d_h = guarded(M, Ch, tdt, DEV), guarded(M, Ch, tdt, DEV), guarded(M, ld + 1, tdt, DEV)
    run(lib().ipoke_gru_update_bwd(ptr(b["o"]), ptr(b["u"]), ptr(b["h"]), ld, ptr(b["g"]), ld, ptr(d_o), ptr(d_u), ptr(d_h), ld + 1, M, Ch, code,
                                   _lib.current_stream()))
    compare("do", dt, exact, d_o, M, slice(0, Ch), ref["do"], "ipoke_gru_update_bwd d o")
    compare("du", dt, exact, d_u, M, slice(0, Ch), ref["du"], "ipoke_gru_update_bwd d u")
    compare("dh1", dt, exact, d_h, M, slice(0, Ch), ref["dh1"], "ipoke_gru_update_bwd d h")
    for t, name in ((d_o, "d o"), (d_u, "d u"), (d_h, "d h")):
        check_guard(t, M, Ch, None, name)
    for given in (True, False):
        ref = X.standalone_phases(o, Ch, given)
        d_ur, d_h = guarded(M, 2 * Ch, tdt, DEV), guarded(M, ld + 1, tdt, DEV)
        run(lib().ipoke_gru_gates_bwd(ptr(b["ur"]), ptr(b["h"]), ld, ptr(b["d_hr"]), ld, ptr(b["d_u"]) if given else None, ptr(d_ur), ptr(d_h),
                                      ld + 1, M, Ch, code, _lib.current_stream()))
        what = "ipoke_gru_gates_bwd" + ("" if given else " (d_u = NULL)")
        compare("dur_u", dt, exact, d_ur, M, slice(0, Ch), ref["dur_u"], what + " d ur[:Ch]")
        compare("dur_r", dt, exact, d_ur, M, slice(Ch, 2 * Ch), ref["dur_r"], what + " d ur[Ch:]")
        compare("dh2", dt, exact, d_h, M, slice(0, Ch), ref["dh2"], what + " d h")
        check_guard(d_ur, M, 2 * Ch, None, "d ur")
        check_guard(d_h, M, Ch, None, "d h")
    for k, v in o.items():
        assert torch.equal(b[k][:M, : v.shape[1]].cpu().to(F64), v) and bool((b[k][M:] == SENT).all()), k
