"""Developer probe: conv2, conv3 and the coupling transform of a coupling net, isolated -- back-to-back launches timed with HIP events
(50 iterations after 5 warm-ups) at the c2 shape (M = 1280, hidden 2048, Cp = 32 transformed channels by default):
  (a) the two launches the engine issued before: conv2 on the tile the cost rule picks (80 x 128 at M = 1280) + ipoke_conv3x3_coupling;
  (b) conv2 alone on the rule's tile;
  (c) conv2 alone on the 128 x 128 tile with one K pass (dispatch switch "nt128");
  (d) the fused launch ipoke_conv_pair_coupling, with and without the store of h2.
Usage: python scripts/probe_pair_coupling.py [B] [hidden] [Cp]"""
import os
import sys
from ctypes import byref

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ipoke_amd import _lib, ops
from ipoke_amd._lib import AffineDesc, CouplingEpi

B = int(sys.argv[1]) if len(sys.argv) > 1 else 20
hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
Cp = int(sys.argv[3]) if len(sys.argv) > 3 else 32
M, DEV, ld = 64 * B, "cuda", 64
L = _lib.lib()
g = torch.Generator(device=DEV).manual_seed(1)
h1 = torch.randn(M, hidden, generator=g, device=DEV).bfloat16()
w2 = (torch.randn(hidden, hidden, generator=g, device=DEV) / hidden ** 0.5).bfloat16()
w3 = (torch.randn(2 * Cp, 9 * hidden, generator=g, device=DEV) / (9 * hidden) ** 0.5).bfloat16()
b3 = torch.randn(2 * Cp, generator=g, device=DEV) * 0.3
state = torch.randn(M, ld, generator=g, device=DEV)
h2 = torch.zeros(M, hidden, device=DEV, dtype=torch.bfloat16)
out = torch.zeros(M, ld, device=DEV)
scale = torch.zeros(M, Cp, device=DEV)
slots = torch.zeros(B, 4, device=DEV)
xchg = torch.empty(L.ipoke_conv3x3_coupling_xchg_bytes(), dtype=torch.uint8, device=DEV)
_lib.check(L.ipoke_conv3x3_coupling_xchg_init(xchg.data_ptr(), _lib.current_stream()))

d2 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 1, 1), (1, 1, 1), (0, 0, 0))
d3 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1))
for d in (d2, d3):
    d.a_sn = 64 * hidden; d.a_sd = 0; d.a_sh = 8 * hidden; d.a_sw = hidden; d.a_sc = 1; d.Kc_real = hidden; d.Kc = hidden
d2.A = h1.data_ptr(); d2.W = w2.data_ptr(); d2.ldw = hidden; d2.Nout = hidden; d2.act = _lib.ACT_ELU; d2.C = h2.data_ptr(); d2.ldc = hidden
d3.A = h2.data_ptr(); d3.W = w3.data_ptr(); d3.ldw = 9 * hidden; d3.Nout = 2 * Cp
a = AffineDesc()
a.bias = b3.data_ptr(); a.Cp = Cp; a.t_off = 1 if 2 * Cp <= ld else 0; a.t_stride = 2 if 2 * Cp <= ld else 1; a.P = 64; a.ld = ld
e = CouplingEpi()
e.mode = 0; e.inp = state.data_ptr(); e.out = out.data_ptr(); e.scale_out = scale.data_ptr(); e.logdet_slot = slots.data_ptr()
e.slot_stride = 4; e.xchg = xchg.data_ptr()


def timed(fn, iters=50, warm=5, rounds=5):
    """(median round, fastest round) of `rounds` rounds, each the mean launch time (us) of `iters` back-to-back calls"""
    res = []
    for _ in range(rounds):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / iters)
    res.sort()
    return res[len(res) // 2], res[0]


def gemm():
    ops.conv_forward(d2, "bf16")


def coupling():
    _lib.check(L.ipoke_conv3x3_coupling(byref(d3), byref(a), byref(e), B, _lib.BF16, _lib.current_stream()))


def pair():
    gemm()
    coupling()


def fused():
    _lib.check(L.ipoke_conv_pair_coupling(byref(d2), byref(d3), byref(a), byref(e), B, _lib.BF16, _lib.current_stream()))


def fused_no_store():
    d2.C = None
    try:
        fused()
    finally:
        d2.C = h2.data_ptr()


applies = L.ipoke_conv_pair_coupling_applicable(M, hidden, 2 * Cp, _lib.BF16)
print(f"M={M} hidden={hidden} Cp={Cp} slices of ipoke_conv3x3_coupling={L.ipoke_conv3x3_coupling_splitk(M, hidden, _lib.BF16)}; "
      f"fused launch applies: {applies}")
res = {}
for rnd in range(2):            # interleaved: every variant twice
    res.setdefault("a_two_launches", []).append(timed(pair))
    res.setdefault("b_gemm_rule_tile", []).append(timed(gemm))
    res.setdefault("conv3_coupling", []).append(timed(coupling))
    with _lib.dispatch_override("nt128", 2):
        res.setdefault("c_gemm_nt128", []).append(timed(gemm))
    if applies:
        res.setdefault("d_fused", []).append(timed(fused))
        res.setdefault("d_fused_no_h2", []).append(timed(fused_no_store))
for k, v in res.items():       # v: one (median round, fastest round) per pass
    print(f"{k:18s} best pass's median round {min(m for m, _ in v):7.2f} us   fastest round {min(m0 for _, m0 in v):7.2f} us   "
          f"(median round of each pass: {', '.join(f'{m:.2f}' for m, _ in v)})")
head = xchg[:256].view(torch.int32)
print(f"hand-off time-outs: {int(head[0])}; scratch clean: {bool((xchg[256:] == 255).all())}")
