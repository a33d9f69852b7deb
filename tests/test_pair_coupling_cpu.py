"""CPU: ipoke_conv_pair_coupling's applicability rule, its validation errors and the "cpl_split" / "nt128" dispatch switches -- everything the
entry decides before it touches the device."""
from ctypes import byref

import pytest

from ipoke_amd import _lib, ops
from ipoke_amd._lib import AffineDesc, CouplingEpi

FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every call below is refused by the validation


def _descs(B=2, hidden=512, Cp=16, ld=64, mode=0):
    d2 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 1, 1), (1, 1, 1), (0, 0, 0))
    d3 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1))
    for d in (d2, d3):
        d.a_sn = 64 * hidden; d.a_sd = 0; d.a_sh = 8 * hidden; d.a_sw = hidden; d.a_sc = 1; d.Kc_real = hidden; d.Kc = hidden
    d2.A = FAKE; d2.W = 2 * FAKE; d2.C = 4 * FAKE
    d2.ldw = hidden; d2.Nout = hidden; d2.act = _lib.ACT_ELU; d2.c_f32 = 0; d2.ldc = hidden
    d3.A = 4 * FAKE; d3.W = 5 * FAKE
    d3.ldw = 9 * hidden; d3.Nout = 2 * Cp
    a = AffineDesc()
    a.bias = 6 * FAKE; a.Cp = Cp; a.t_off = 0; a.t_stride = 1; a.P = 64; a.ld = ld
    e = CouplingEpi()
    e.mode = mode; e.inp = 7 * FAKE; e.out = 8 * FAKE; e.xchg = 9 * FAKE
    if mode == 1:
        e.out2 = 10 * FAKE; e.an_c0 = 0; e.an_C = ld
    return d2, d3, a, e


def test_applicability_rule():
    L = _lib.lib()
    ok = L.ipoke_conv_pair_coupling_applicable
    assert ok(1280, 2048, 64, _lib.BF16) == 1                 # c2: 10 row tiles x 16 slices
    assert ok(1280, 2048, 32, _lib.BF16) == 1
    assert ok(64, 512, 2, _lib.BF16) == 1
    assert ok(2048, 2048, 64, _lib.BF16) == 1                 # 16 x 16 = one round exactly
    assert ok(2112, 2048, 64, _lib.BF16) == 0
    assert ok(2560, 2048, 64, _lib.BF16) == 0                 # c3's rows at this width: 320 workgroups
    assert ok(2560, 1024, 64, _lib.BF16) == 1
    assert ok(1024, 4096, 64, _lib.BF16) == 1                 # 8 x 32
    assert ok(1280, 4096, 64, _lib.BF16) == 0                 # 10 x 32
    assert ok(1280, 2048, 64, _lib.F32) == 0
    assert ok(1280, 2048, 66, _lib.BF16) == 0                 # conv3 is at most 64 columns wide
    assert ok(1280, 2048, 0, _lib.BF16) == 0
    assert ok(1312, 2048, 64, _lib.BF16) == 0                 # rows: whole 8x8 maps
    for hidden in (128, 256, 768, 1536, 2112, 8192):          # 4, 8, 16 or 32 slices of 128 channels
        assert ok(128, hidden, 64, _lib.BF16) == 0, hidden
    for hidden in (512, 1024, 2048, 4096):
        assert ok(128, hidden, 64, _lib.BF16) == 1, hidden


def _refused(d2, d3, a, e, B=2, dtype=_lib.BF16, needle=None):
    L = _lib.lib()
    ref = lambda v: byref(v) if v is not None else None
    rc = L.ipoke_conv_pair_coupling(ref(d2), ref(d3), ref(a), ref(e), B, dtype, None)
    assert rc == -1, rc
    if needle:
        assert needle.encode() in L.ipoke_last_error(), L.ipoke_last_error()


def test_validation_errors_need_no_gpu():
    for k in range(4):
        args = list(_descs()); args[k] = None
        _refused(*args, needle="null descriptor")
    _refused(*_descs(), dtype=_lib.F32, needle="bf16 only")
    d2, d3, a, e = _descs(); e.xchg = None
    _refused(d2, d3, a, e, needle="exchange scratch")
    d2, d3, a, e = _descs(); d2.w_kmajor = 1; d2.ldw = 512
    _refused(d2, d3, a, e, needle="conv2")
    d2, d3, a, e = _descs(); d2.kh = d2.kw = 3; d2.ph = d2.pw = 1; d2.ldw = 9 * 512
    _refused(d2, d3, a, e, needle="conv2")
    d2, d3, a, e = _descs(); d2.act = _lib.ACT_NONE
    _refused(d2, d3, a, e, needle="ELU")
    d2, d3, a, e = _descs(); d2.c_f32 = 1
    _refused(d2, d3, a, e, needle="ELU")
    d2, d3, a, e = _descs(); d2.dact = 3 * FAKE; d2.ld_dact = 512; d2.dact_act = _lib.ACT_ELU
    _refused(d2, d3, a, e, needle="ELU")
    d2, d3, a, e = _descs(); d2.bias = 3 * FAKE + 4
    _refused(d2, d3, a, e, needle="16-byte aligned")
    d2, d3, a, e = _descs(); d2.ldc = 510
    _refused(d2, d3, a, e, needle="h2 rows")
    d2, d3, a, e = _descs(); d3.bias = 3 * FAKE
    _refused(d2, d3, a, e, needle="raw sums only")
    d2, d3, a, e = _descs(); d3.kh = d3.kw = 1; d3.ph = d3.pw = 0; d3.ldw = 512
    _refused(d2, d3, a, e, needle="conv3")
    d2, d3, a, e = _descs(); d3.transposed = 1
    _refused(d2, d3, a, e, needle="conv3")
    d2, d3, a, e = _descs(B=3); d3.NB = 2
    _refused(d2, d3, a, e, B=3, needle="conv3")
    _refused(*_descs(), B=3, needle="conv3")                                      # B does not match the maps
    d2, d3, a, e = _descs()                                                       # condition_nice: conv3 reads more channels than conv2 writes
    d3.Kc = d3.Kc_real = 640; d3.a_sw = 640; d3.a_sh = 8 * 640; d3.a_sn = 64 * 640; d3.ldw = 9 * 640; d2.ldc = 640
    _refused(d2, d3, a, e, needle="exactly conv2's output channels")
    d2, d3, a, e = _descs(); d3.A = 11 * FAKE
    _refused(d2, d3, a, e, needle="conv3 reads conv2's output")
    d2, d3, a, e = _descs(); d3.a_sw = 1024; d3.a_sh = 8 * 1024; d3.a_sn = 64 * 1024
    _refused(d2, d3, a, e, needle="conv3 reads conv2's output")
    d2, d3, a, e = _descs(); a.Cp = 8
    _refused(d2, d3, a, e, needle="coupling geometry")
    d2, d3, a, e = _descs(); a.t_off = 40; a.t_stride = 2
    _refused(d2, d3, a, e, needle="coupling geometry")
    d2, d3, a, e = _descs(); e.mode = 3
    _refused(d2, d3, a, e, needle="bad mode")
    d2, d3, a, e = _descs(); e.inp = None
    _refused(d2, d3, a, e, needle="bad mode")
    d2, d3, a, e = _descs(); e.out = None
    _refused(d2, d3, a, e, needle="bad outputs")
    d2, d3, a, e = _descs(mode=1); e.out2 = None
    _refused(d2, d3, a, e, needle="bad outputs")
    d2, d3, a, e = _descs(mode=1); e.ext = 12 * FAKE; e.ext_ld = 16
    _refused(d2, d3, a, e, needle="bad outputs")
    d2, d3, a, e = _descs(); e.logdet_slot = 12 * FAKE; e.slot_stride = 2
    _refused(d2, d3, a, e, needle="log-det slots")
    d2, d3, a, e = _descs(); e.ext = 12 * FAKE; e.ext_ld = 8
    _refused(d2, d3, a, e, needle="extra operand")
    for hidden in (256, 768):                                                     # a hidden width the rule does not take
        _refused(*_descs(hidden=hidden), needle="not taken")
    # without a stored h2 (conv2.C == NULL) conv3's input pointer is ignored: the same checks apply to everything else
    d2, d3, a, e = _descs(mode=2); d2.C = None; d3.A = None; d2.act = _lib.ACT_NONE
    _refused(d2, d3, a, e, needle="ELU")


def test_dispatch_switches():
    L = _lib.lib()
    for v in (4, 8, 16, 32, -1):
        assert L.ipoke_set_dispatch_override(b"cpl_split", v) == 0
    for v in (0, 2, 3, 12, 64):
        assert L.ipoke_set_dispatch_override(b"cpl_split", v) == -1
    assert L.ipoke_set_dispatch_override(b"nt128", 2) == 0 and L.ipoke_set_dispatch_override(b"nt128", -1) == 0
    assert L.ipoke_set_dispatch_override(b"nt128", 3) == -1
    assert L.ipoke_set_dispatch_override(b"nt256", 2) == -1
