"""Two adjacent MaCowUnits in ONE launch per direction (ipoke_macow_unit2_fwd / _bwd / _inv: csrc/mcf_unit_split.hip, mcf_unit.hip)
against the same build's two four-layer launches, and the flow engine's default path against its hook that keeps a launch per unit
(ipoke_flow_test_split_unit2).  The arithmetic does not change -- same rows per workgroup, same tiles, same K order, one sum per layer
-- so every comparison is torch.equal.

f32: the fused unit kernels take bf16 matrix-core inputs only (ipoke_macow_unit_supported); the f32 cases assert that the two-unit
entry points refuse the dtype exactly as the four-layer ones do and leave every output untouched."""
import ctypes
import functools
from ctypes import c_void_p, cast, pointer

import pytest
import torch

from ipoke_amd import _lib, configs, ops
from ipoke_amd._lib import UnitPairDesc, check
from ipoke_amd.utils.detfill import deterministic_fill_
from oracle import flow_ref
from tests.helpers import mcf_shadows, tdt

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = "bf16"
NL = 8
SENT = 3.0                                  # fill of every output buffer: what a launch does not write must stay as it is
LD = {8: 8, 32: 64, 60: 64, 64: 64}          # state pitch per width: ld > C (pass-through columns) at C = 32 and 60
FWD, BWD, INV = 0, 1, 2


@functools.lru_cache(maxsize=None)
def _weights(C):
    """two units of width C with weights of their own; no weight-norm gain is zero (no layer is the identity)"""
    shs, posts = [], []
    for u in range(2):
        o = flow_ref.MaCowUnit(C, (2, 3), 128)
        deterministic_fill_(o, prefix=f"double{u}.unit{C}.")
        for name, v in o.state_dict().items():
            if name.endswith("weight_g"):
                assert float(v.abs().min()) > 0.0, name
        for l in (o.conv1, o.conv2, o.conv3, o.conv4):
            shs.append(mcf_shadows({k: v.detach().to(DEV) for k, v in l.state_dict().items()}, "", C, 128, DT))
        for an in (None, o.actnorm1, None, o.actnorm2):
            posts.append(None if an is None else (an.log_scale.detach().flatten().to(DEV).contiguous(),
                                                  an.bias.detach().flatten().to(DEV).contiguous()))
    assert not torch.equal(shs[0]["W1"], shs[4]["W1"]) and not torch.equal(posts[1][0], posts[5][0])
    return shs, posts


@functools.lru_cache(maxsize=None)
def _inputs(C, B):
    ld = LD[C]
    gen = torch.Generator().manual_seed(1000 + 10 * C + B)
    x = torch.randn(B, ld, 8, 8, generator=gen)
    h = torch.randn(B, 128, 8, 8, generator=gen)
    M = B * 64
    return dict(xs=ops.to_state(x.to(DEV)), cond=ops.cond_prepare(h.to(DEV), DT), dy=torch.randn(M, ld, generator=gen).to(DEV),
                dld=torch.randn(B, generator=gen).to(DEV))


def _buffers(C, B, S):
    ld, M, dims = LD[C], B * 64, _weights(C)[0][0]["dims"]
    f = lambda *shape, dt=torch.float32: torch.full(shape, SENT, device=DEV, dtype=dt)
    o = dict(ys=[f(M, ld) for _ in range(NL)], a2=[f(M, dims["K2p"], dt=tdt(DT)) for _ in range(NL)], sc=[f(M, C) for _ in range(NL)],
             dps=[f(M, dims["K3p"], dt=tdt(DT)) for _ in range(NL)], dcs=[f(M, dims["Hq"], dt=tdt(DT)) for _ in range(NL)],
             xop=[f(M, dims["Cp"], dt=tdt(DT)) for _ in range(NL)], dbp=[f(B * max(S, 1), 2 * C) for _ in range(NL)],
             pp=[f(B * max(S, 1), 2 * C) for _ in range(NL)], slot=f(NL, B, 4), dx=f(M, ld), gmid=f(M, ld), xmid=f(M, ld), xrec=f(M, ld),
             zc=f(M, C // 2 + 8, dt=tdt(DT)))
    nb = _lib.lib().ipoke_macow_unit_xchg_bytes(B, S)
    o["xchg"] = torch.zeros(max(nb, 8) // 4, dtype=torch.int32, device=DEV)
    return o


def _descs(C, B, S, lo, n, o, saved, dtype=DT):
    """descriptors of the layers [lo, lo + n) of the eight-layer chain: outputs into `o`, forward saves from `saved`"""
    shs, posts = _weights(C)
    inp = _inputs(C, B)
    d = (_lib.McfDesc * n)()
    for i in range(n):
        k = lo + i
        e, sh = d[i], shs[k]
        e.ld, e.C, e.B = LD[C], C, B
        e.cond, e.Cc = inp["cond"].data_ptr(), inp["cond"].shape[1]
        e.W1, e.W2, e.bias2, e.W1T, e.W2T = (sh[n_].data_ptr() for n_ in ("W1", "W2", "bias", "W1T", "W2T"))
        e.order = k % 4
        e.rows_per_block = 16
        e.x = (inp["xs"] if k == 0 else saved["ys"][k - 1]).data_ptr()
        e.y = o["ys"][k].data_ptr()
        e.a2_save, e.scale_save, e.logdet_slot = saved["a2"][k].data_ptr(), saved["sc"][k].data_ptr(), o["slot"][k].data_ptr()
        e.dparams_save, e.dc_save, e.dbias_part = o["dps"][k].data_ptr(), o["dcs"][k].data_ptr(), o["dbp"][k].data_ptr()
        e.x_op_save = o["xop"][k].data_ptr()
        if posts[k] is not None:
            e.post_log_scale, e.post_bias = posts[k][0].data_ptr(), posts[k][1].data_ptr()
            e.y_post, e.post_part = saved["ys"][k].data_ptr(), o["pp"][k].data_ptr()
    d[0].dld = inp["dld"].data_ptr()
    if S > 1:
        d[0].split, d[0].xchg = S, o["xchg"].data_ptr()
    return d


def _zc(d, C, o):
    d.zc_out, d.zc_off, d.zc_stride, d.zc_cin, d.zc_ld = o["zc"].data_ptr(), 1, 2, C // 2, o["zc"].shape[1]


def _scratch_zero(o):
    return int((o["xchg"] != 0).sum().item()) == 0          # word 0 (the time-out count) included


class Pair:
    """the (ActNorm + shuffle, coupling) pair in front of the lower unit; outputs per run"""
    def __init__(self, C, B, S):
        ld, M = LD[C], B * 64
        gen = torch.Generator().manual_seed(77 + C)
        self.Cp, self.t_off, self.t_stride, self.S, self.B, self.C = C // 2, 1 if C > 8 else 0, 2, S, B, C
        self.ldp = 2 * self.Cp + 8
        self.an_ls = (torch.randn(C, generator=gen) * 0.2).to(DEV)
        self.an_idx = torch.randperm(C, generator=gen).to(torch.int32).to(DEV)
        self.x1 = torch.randn(M, ld, generator=gen).to(DEV); self.x0 = torch.randn(M, ld, generator=gen).to(DEV)
        self.scale = (torch.rand(M, self.Cp, generator=gen) * 1.5 + 0.2).to(DEV)

    def attach(self, d0, o):
        M = self.B * 64
        o["pair_dp"] = torch.full((M, self.ldp), SENT, device=DEV).to(tdt(DT))
        o["pair_part"] = torch.full((self.B * self.S, 2 * self.C), SENT, device=DEV)
        o["pair_db"] = torch.full((self.B * self.S, 2 * self.Cp), SENT, device=DEV)
        q = UnitPairDesc()
        q.an_log_scale, q.an_idx, q.an_x, q.an_part = self.an_ls.data_ptr(), self.an_idx.data_ptr(), self.x1.data_ptr(), o["pair_part"].data_ptr()
        q.Cp, q.t_off, q.t_stride = self.Cp, self.t_off, self.t_stride
        q.x0, q.scale, q.dparams, q.ldp, q.dbias_part = self.x0.data_ptr(), self.scale.data_ptr(), o["pair_dp"].data_ptr(), self.ldp, o["pair_db"].data_ptr()
        q.dx = o["dx"].data_ptr()
        d0.pair = cast(pointer(q), c_void_p).value
        return q                                             # (kept alive by the caller)


def _run(direction, C, B, S, o, saved, double, with_zc=False, pair=None):
    L, s, inp = _lib.lib(), _lib.current_stream(), _inputs(C, B)
    keep = []
    if direction == FWD:
        if double:
            d = _descs(C, B, S, 0, 8, o, o)
            if with_zc:
                _zc(d[7], C, o)
            check(L.ipoke_macow_unit2_fwd(d, _lib.DTYPES[DT], s))
        else:
            for lo in (0, 4):
                d = _descs(C, B, S, lo, 4, o, o)
                if with_zc and lo == 4:
                    _zc(d[3], C, o)
                check(L.ipoke_macow_unit_fwd(d, _lib.DTYPES[DT], s))
    elif direction == BWD:
        if double:
            d = _descs(C, B, S, 0, 8, o, saved)
            d[7].dy, d[0].dx = inp["dy"].data_ptr(), o["dx"].data_ptr()
            if pair:
                keep.append(pair.attach(d[0], o))
            check(L.ipoke_macow_unit2_bwd(d, _lib.DTYPES[DT], s))
        else:
            d = _descs(C, B, S, 4, 4, o, saved)
            d[3].dy, d[0].dx = inp["dy"].data_ptr(), o["gmid"].data_ptr()
            check(L.ipoke_macow_unit_bwd(d, _lib.DTYPES[DT], s))
            d = _descs(C, B, S, 0, 4, o, saved)
            d[3].dy, d[0].dx = o["gmid"].data_ptr(), o["dx"].data_ptr()
            if pair:
                keep.append(pair.attach(d[0], o))
            check(L.ipoke_macow_unit_bwd(d, _lib.DTYPES[DT], s))
    else:
        y_in = saved["ys"][7]
        if double:
            d = _descs(C, B, 0, 0, 8, o, saved)
            d[7].x = d[0].x = y_in.data_ptr(); d[0].y = d[7].y = o["xrec"].data_ptr()
            check(L.ipoke_macow_unit2_inv(d, _lib.DTYPES[DT], s))
        else:
            d = _descs(C, B, 0, 4, 4, o, saved)
            d[3].x = d[0].x = y_in.data_ptr(); d[0].y = d[3].y = o["xmid"].data_ptr()
            check(L.ipoke_macow_unit_inv(d, _lib.DTYPES[DT], s))
            d = _descs(C, B, 0, 0, 4, o, saved)
            d[3].x = d[0].x = o["xmid"].data_ptr(); d[0].y = d[3].y = o["xrec"].data_ptr()
            check(L.ipoke_macow_unit_inv(d, _lib.DTYPES[DT], s))
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _reference(C, B, S):
    """the parent path, once per shape: two four-layer launches per direction (backward and inverse on the saves of this forward pass)"""
    o = _buffers(C, B, S)
    _run(FWD, C, B, S, o, o, False, with_zc=True)
    _run(BWD, C, B, S, o, o, False)
    _run(INV, C, B, S, o, o, False)
    assert _scratch_zero(o)
    return o


FWD_KEYS = ("ys", "a2", "sc")
BWD_KEYS = ("dps", "dcs", "xop", "dbp", "pp")


def _assert_equal(direction, C, got, ref, tag):
    if direction == FWD:
        for nme in FWD_KEYS:
            for k in range(NL):
                cols = C if nme == "ys" and k % 4 < 3 else None      # pass-through columns: the units' output states only
                assert torch.equal(got[nme][k][:, :cols], ref[nme][k][:, :cols]), (tag, nme, k)
        assert torch.equal(got["slot"], ref["slot"]), (tag, "the eight log-det slots")
        assert torch.equal(got["zc"], ref["zc"]), (tag, "zc")
    elif direction == BWD:
        for nme in BWD_KEYS:
            for k in range(NL):
                assert torch.equal(got[nme][k], ref[nme][k]), (tag, nme, k)
        assert torch.equal(got["dx"], ref["dx"]), (tag, "dx")
    else:
        assert torch.equal(got["xrec"], ref["xrec"]), (tag, "reconstructed input")


CASES = [(C, S, B) for C in (8, 32, 60, 64) for S in (2, 4) for B in (1, 3)]


@pytest.mark.parametrize("C,S,B", CASES)
def test_double_forward_is_bit_identical(C, S, B):
    ref = _reference(C, B, S)
    o = _buffers(C, B, S)
    with_zc = True                                           # (the reference carries the zc operand: every case checks it)
    _run(FWD, C, B, S, o, o, True, with_zc=with_zc)
    _assert_equal(FWD, C, o, ref, "first")
    assert _scratch_zero(o), "the exchange scratch must be all-zero again after a launch"
    assert torch.isfinite(o["ys"][7]).all() and not torch.equal(o["ys"][7][:, :C], o["ys"][3][:, :C])
    if LD[C] > C:                                            # pass-through columns reach both units' output states
        xs = _inputs(C, B)["xs"]
        assert torch.equal(o["ys"][3][:, C:], xs[:, C:]) and torch.equal(o["ys"][7][:, C:], xs[:, C:])
    again = _buffers(C, B, S)
    again["xchg"] = o["xchg"]                                # the same launch on the used scratch
    _run(FWD, C, B, S, again, again, True, with_zc=with_zc)
    _assert_equal(FWD, C, again, ref, "replay")
    assert _scratch_zero(again)


@pytest.mark.parametrize("C,S,B", CASES)
def test_double_backward_is_bit_identical(C, S, B):
    ref = _reference(C, B, S)
    o = _buffers(C, B, S)
    _run(BWD, C, B, S, o, ref, True)
    _assert_equal(BWD, C, o, ref, "first")
    assert _scratch_zero(o), "the exchange scratch must be all-zero again after a launch"
    assert torch.isfinite(o["dx"]).all()
    again = _buffers(C, B, S)
    again["xchg"] = o["xchg"]
    _run(BWD, C, B, S, again, ref, True)
    _assert_equal(BWD, C, again, ref, "replay")
    assert _scratch_zero(again)


@pytest.mark.parametrize("C,B", [(C, B) for C in (8, 32, 60, 64) for B in (1, 3)])
def test_double_inverse_is_bit_identical(C, B):
    ref = _reference(C, B, 2)
    o = _buffers(C, B, 0)
    _run(INV, C, B, 0, o, ref, True)
    _assert_equal(INV, C, o, ref, "inverse")
    assert torch.isfinite(o["xrec"]).all()
    # the round trip closes as well as the two-launch one does (same bits), and on the pass-through columns exactly
    if LD[C] > C:
        assert torch.equal(o["xrec"][:, C:], ref["ys"][7][:, C:])


@pytest.mark.parametrize("C,S,B", [(64, 4, 3), (60, 2, 3), (8, 4, 1)])
def test_double_backward_carries_the_pair_in_front(C, S, B):
    """the UnitPair attaches to the launch's LOWEST unit: same bits as the lower unit's own launch carrying it"""
    ref = _reference(C, B, S)
    pair = Pair(C, B, S)
    r = _buffers(C, B, S)
    _run(BWD, C, B, S, r, ref, False, pair=pair)
    o = _buffers(C, B, S)
    _run(BWD, C, B, S, o, ref, True, pair=pair)
    for nme in BWD_KEYS:
        for k in range(NL):
            assert torch.equal(o[nme][k], r[nme][k]), (nme, k)
    for nme in ("dx", "pair_dp", "pair_part", "pair_db"):
        assert torch.equal(o[nme], r[nme]), nme
    assert not torch.equal(o["dx"], ref["dx"])               # (the pair really changed what dx holds)
    assert _scratch_zero(o)


@pytest.mark.parametrize("direction", [FWD, BWD])
def test_double_launch_beside_a_copy_stream(direction):
    """uneven load beside the hand-offs: a copy stream on the other CUs, as in the row-split tests"""
    C, S, B = 64, 4, 3
    ref = _reference(C, B, S)
    side = torch.cuda.Stream()
    big = torch.empty(128 << 20, dtype=torch.uint8, device=DEV); big2 = torch.empty_like(big)
    for rep in range(2):
        o = _buffers(C, B, S)
        with torch.cuda.stream(side):
            for _ in range(3):
                big2.copy_(big)
        _run(direction, C, B, S, o, o if direction == FWD else ref, True, with_zc=True)
        _assert_equal(direction, C, o, ref, rep)
        assert _scratch_zero(o)
    torch.cuda.synchronize()


@pytest.mark.parametrize("direction", [FWD, BWD, INV])
@pytest.mark.parametrize("C,S,B", CASES)
def test_f32_is_refused_like_the_four_layer_calls(direction, C, S, B):
    """the f32 cases: no fused unit kernel takes f32 (parity mode runs the per-layer kernels); the two-unit calls refuse it as the
    four-layer ones do, launch nothing and say so in the rule"""
    L, s = _lib.lib(), _lib.current_stream()
    split = 0 if direction == INV else S
    assert L.ipoke_macow_unit2_applicable(C, 128, _lib.F32, split, direction) == 0
    assert L.ipoke_macow_unit2_applicable(C, 128, _lib.BF16, split, direction) == 1
    o = _buffers(C, B, S)
    d = _descs(C, B, split, 0, 8, o, o)
    d[7].dy, d[0].dx = _inputs(C, B)["dy"].data_ptr(), o["dx"].data_ptr()
    fn8, fn4 = ((L.ipoke_macow_unit2_fwd, L.ipoke_macow_unit_fwd), (L.ipoke_macow_unit2_bwd, L.ipoke_macow_unit_bwd),
                (L.ipoke_macow_unit2_inv, L.ipoke_macow_unit_inv))[direction]
    assert fn4(d, _lib.F32, s) != 0 and fn8(d, _lib.F32, s) != 0
    torch.cuda.synchronize()
    for nme in ("ys", "dps"):
        assert all(bool((t.float() == SENT).all()) for t in o[nme])


def test_double_rule_and_bad_arguments():
    L, s = _lib.lib(), _lib.current_stream()
    assert L.ipoke_macow_unit2_applicable(64, 128, _lib.BF16, 4, FWD) == 1 and L.ipoke_macow_unit2_applicable(64, 128, _lib.BF16, 2, BWD) == 1
    assert L.ipoke_macow_unit2_applicable(64, 128, _lib.BF16, 1, FWD) == 0          # the one-workgroup kernels keep four layers
    assert L.ipoke_macow_unit2_applicable(64, 128, _lib.BF16, 0, BWD) == 0
    assert L.ipoke_macow_unit2_applicable(64, 128, _lib.BF16, 0, INV) == 1
    assert L.ipoke_macow_unit2_applicable(66, 128, _lib.BF16, 4, FWD) == 0
    C, S, B = 8, 2, 1
    o = _buffers(C, B, S)
    d = _descs(C, B, 1, 0, 8, o, o)                                              # no split
    assert L.ipoke_macow_unit2_fwd(d, _lib.DTYPES[DT], s) != 0
    d = _descs(C, B, S, 0, 8, o, o)
    d[5].C = 16                                                                   # the two units must share their width
    assert L.ipoke_macow_unit2_fwd(d, _lib.DTYPES[DT], s) != 0
    d = _descs(C, B, S, 0, 8, o, o)
    _zc(d[3], C, o)                                                               # zc: the launch's last layer only
    assert L.ipoke_macow_unit2_fwd(d, _lib.DTYPES[DT], s) != 0
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in o["ys"])


# ---------------------------------------------------------------------------------------------------------------------------
# Engine level: the default path against ipoke_flow_test_split_unit2 on a reduced flow.
def _engine(z, hidden, max_batch):
    from ipoke_amd.flow import SupervisedMacowTransformer
    arch = configs.flow_arch(z, hidden=hidden, num_steps=[1, 1], factor=4)
    m = SupervisedMacowTransformer(arch, dtype="bf16", device="cuda", init="none", max_batch=max_batch)
    deterministic_fill_(m, prefix="flow.")
    m.sync_buffers()
    return m, arch


@pytest.mark.parametrize("z", [16, 64])
def test_engine_double_and_single_unit_passes_are_bit_identical(z):
    B = 2
    m, arch = _engine(z, 256, B)
    m.train()
    eng = m.engine
    L = eng.lib
    g = torch.Generator().manual_seed(5 + z)
    x0 = torch.randn(B, z, 8, 8, generator=g).cuda()
    z0 = torch.randn(B, z, 8, 8, generator=g).cuda()
    cond = torch.randn(B, arch["h_channels"], 8, 8, generator=g).cuda()
    tags = (ctypes.c_int * 3)(3, 4, 5)          # IPOKE_TAG_UNIT_FWD, _BWD, _INV

    def counted(raw):
        """unit counts (forward, backward, inverse) of one training pass + one reverse pass; raw: launches instead of units"""
        check(L.ipoke_timing_raw_launches(int(raw)))
        try:
            check(L.ipoke_timing_start())
            m.flat_grads.zero_()
            x = x0.clone().requires_grad_(True)
            out, logdet = m(x, cond)
            ((out ** 2).sum() * 0.5 - logdet.sum()).backward()
            with torch.no_grad():
                m(z0, cond, reverse=True)
            torch.cuda.synchronize()
            counts = (ctypes.c_int * 3)(); mean = (ctypes.c_double * 3)()
            check(L.ipoke_timing_stop(tags, 3, counts, mean))
        finally:
            L.ipoke_timing_raw_launches(0)
        return tuple(counts)

    def run(split):
        check(L.ipoke_flow_test_split_unit2(eng.handle, int(split)))
        m.flat_grads.zero_()
        x = x0.clone().requires_grad_(True)
        out, logdet = m(x, cond)
        loss = (out ** 2).sum() * 0.5 - logdet.sum()
        loss.backward()
        with torch.no_grad():
            fwd_eval = m(x0, cond)[0].clone()                                    # forward without saved states
            rev = [m(z0, cond, reverse=True).clone()]                            # eager
            m.set_graph_mode(True)
            rev += [m(z0, cond, reverse=True).clone() for _ in range(3)]         # captured, then replayed
            m.set_graph_mode(False)
        torch.cuda.synchronize()
        return dict(out=out.detach().clone(), logdet=logdet.detach().clone(), grads=m.flat_grads.clone(), dx=x.grad.clone(), fwd_eval=fwd_eval,
                    rev=rev, units=counted(False), launches=counted(True))

    try:
        f = run(0)                                                               # the default rule
        s = run(1)                                                               # a launch per unit
        a = run(-1)                                                              # two units per launch in every direction
        f2 = run(0)
    finally:
        L.ipoke_flow_test_split_unit2(eng.handle, 0)
    assert torch.isfinite(f["grads"]).all() and f["grads"].abs().max() > 0 and torch.isfinite(f["rev"][0]).all()
    for k in ("out", "logdet", "grads", "dx", "fwd_eval"):
        assert torch.equal(f[k], f2[k]), f"{k}: the default pass is not reproducible"
        assert torch.equal(f[k], s[k]), f"{k} differs: max {(f[k] - s[k]).abs().max().item():.3e}"
        assert torch.equal(a[k], s[k]), f"{k} differs (two units per launch everywhere): max {(a[k] - s[k]).abs().max().item():.3e}"
    for r in f["rev"][1:] + f2["rev"] + a["rev"]:
        assert torch.equal(r, f["rev"][0]), "reverse pass: a replay differs from the eager pass"
    assert torch.equal(f["rev"][0], s["rev"][0]), "reverse pass differs"
    assert tuple(eng.handoff_timeouts()) == (0, 0)
    # units of work are the same either way; two units per launch issue half the launches -- by default in the forward and the backward
    # pass (the reverse pass keeps a launch per unit: it did not pay by the project's margin over noise), with the hook in all three
    print(f"z={z}: units {f['units']} launches default {f['launches']} per unit {s['launches']} two per launch {a['launches']}")
    assert f["units"] == s["units"] == a["units"] == s["launches"] and min(f["units"]) > 0, (f["units"], s["units"], a["units"], s["launches"])
    assert all(2 * n2 == n1 for n2, n1 in zip(a["launches"], s["launches"])), (a["launches"], s["launches"])
    assert f["launches"] == (a["launches"][0], a["launches"][1], s["launches"][2]), (f["launches"], s["launches"], a["launches"])
