"""CPU: ipoke_conv_pair_dgrad's applicability rule and its validation errors -- everything the entry decides before it touches the device."""
from ctypes import byref

from ipoke_amd import _lib, ops

FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every call below is refused by the validation


def _descs(B=2, hidden=256, cin=16):
    d2 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 1, 1), (1, 1, 1), (0, 0, 0))
    d1 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1), True)
    for d in (d2, d1):
        d.a_sn = 64 * hidden; d.a_sd = 0; d.a_sh = 8 * hidden; d.a_sw = hidden; d.a_sc = 1; d.Kc_real = hidden; d.Kc = hidden
    d2.A = FAKE; d2.W = 2 * FAKE; d2.dact = 3 * FAKE; d2.C = 4 * FAKE
    d2.ldw = hidden; d2.Nout = hidden; d2.w_kmajor = 1; d2.ld_dact = hidden; d2.dact_act = _lib.ACT_ELU; d2.c_f32 = 0; d2.ldc = hidden
    d1.A = 4 * FAKE; d1.W = 5 * FAKE; d1.C = 6 * FAKE
    d1.ldw = 9 * hidden; d1.Nout = cin; d1.c_f32 = 1; d1.c_accumulate = 1; d1.ldc = 136; d1.c_coff = 3; d1.c_cstride = 2
    d1.acc_scratch = 7 * FAKE; d1.acc_scratch_bytes = 1 << 30
    return d2, d1


def test_applicability_rule():
    L = _lib.lib()
    big = 1 << 30
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 32, _lib.BF16, big) == 1           # c2: 10 row tiles x 16 slices
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 16, _lib.BF16, big) == 1
    assert L.ipoke_conv_pair_dgrad_applicable(64, 256, 1, _lib.BF16, big) == 1
    assert L.ipoke_conv_pair_dgrad_applicable(2048, 2048, 32, _lib.BF16, big) == 1           # 16 x 16 = one round exactly
    assert L.ipoke_conv_pair_dgrad_applicable(2112, 2048, 32, _lib.BF16, big) == 0
    assert L.ipoke_conv_pair_dgrad_applicable(2560, 2048, 32, _lib.BF16, big) == 0           # c3's rows at this width: 320 workgroups
    assert L.ipoke_conv_pair_dgrad_applicable(2560, 1024, 32, _lib.BF16, big) == 1
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 32, _lib.F32, big) == 0
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 33, _lib.BF16, big) == 0           # wider couplings: two launches
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 64, _lib.BF16, big) == 0
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 0, _lib.BF16, big) == 0
    assert L.ipoke_conv_pair_dgrad_applicable(1312, 2048, 32, _lib.BF16, big) == 0           # rows: whole 8x8 maps
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2112, 32, _lib.BF16, big) == 0           # hidden: whole 128-column tiles
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 128, 32, _lib.BF16, big) == 0            # at least two slices
    need = 16384 + 10 * 16 * 128 * 32 * 4                                                   # counters + one slab per workgroup
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 32, _lib.BF16, need) == 1
    assert L.ipoke_conv_pair_dgrad_applicable(1280, 2048, 32, _lib.BF16, need - 1) == 0
    assert L.ipoke_conv_acc_scratch_bytes(1280, 32, 16) >= need                             # the documented sizing call covers it


def _refused(d2, d1, dtype=_lib.BF16, needle=None):
    L = _lib.lib()
    rc = L.ipoke_conv_pair_dgrad(byref(d2) if d2 is not None else None, byref(d1) if d1 is not None else None, dtype, None)
    assert rc == -1, rc
    if needle:
        assert needle.encode() in L.ipoke_last_error(), L.ipoke_last_error()


def test_validation_errors_need_no_gpu():
    d2, d1 = _descs()
    _refused(None, d1, needle="null descriptor")
    _refused(d2, None, needle="null descriptor")
    _refused(d2, d1, dtype=_lib.F32, needle="bf16 only")
    d2, d1 = _descs(); d2.w_kmajor = 0
    _refused(d2, d1, needle="conv2")
    d2, d1 = _descs(); d2.c_f32 = 1
    _refused(d2, d1, needle="conv2")
    d2, d1 = _descs(); d2.act = _lib.ACT_ELU
    _refused(d2, d1, needle="conv2")
    d2, d1 = _descs(); d2.dact_act = _lib.ACT_TANH
    _refused(d2, d1, needle="conv2")
    d2, d1 = _descs(); d1.kh = d1.kw = 1; d1.ph = d1.pw = 0
    _refused(d2, d1, needle="conv1")
    d2, d1 = _descs(); d1.A = 8 * FAKE
    _refused(d2, d1, needle="conv1 reads conv2's output")
    d2, d1 = _descs(); d1.a_sw = 512; d1.a_sh = 8 * 512; d1.a_sn = 64 * 512
    _refused(d2, d1, needle="conv1 reads conv2's output")
    d2, d1 = _descs(); d1.c_accumulate = 0
    _refused(d2, d1, needle="accumulates")
    d2, d1 = _descs(); d1.acc_scratch = None
    _refused(d2, d1, needle="scratch")
    d2, d1 = _descs(); d1.acc_scratch_bytes = 16384 + 2 * 128 * 32 * 4 - 1
    _refused(d2, d1, needle="not taken")
    d2, d1 = _descs(cin=40)
    _refused(d2, d1, needle="not taken")
    d2, d1 = _descs(B=3); d1.NB = 2
    _refused(d2, d1, needle="conv1")
