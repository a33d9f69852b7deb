"""Developer probe: the conv2 + conv1 data gradients of a coupling net, isolated -- back-to-back launches timed with HIP events
(50 iterations after 5 warm-ups) at the c2 shape (M = 1280, hidden 2048, 32 conditioning channels by default):
  (a) the two launches the engine issued before: the GEMM on the tile the cost rule picks (80 x 128 at M = 1280) + conv3x3_s8n32;
  (b) the GEMM alone on the 128 x 128 tile (dispatch switch "nn128"), and on the rule's tile for comparison;
  (c) the fused launch ipoke_conv_pair_dgrad.
Usage: python scripts/probe_pair_dgrad.py [B] [hidden] [cin]"""
import os
import sys
from ctypes import byref

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ipoke_amd import _lib, ops

B = int(sys.argv[1]) if len(sys.argv) > 1 else 20
hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
cin = int(sys.argv[3]) if len(sys.argv) > 3 else 32
M, DEV = 64 * B, "cuda"
L = _lib.lib()
g = torch.Generator(device=DEV).manual_seed(1)
dp2 = torch.randn(M, hidden, generator=g, device=DEV).bfloat16()
w2 = (torch.randn(hidden, hidden, generator=g, device=DEV) / hidden ** 0.5).bfloat16()
h1 = torch.randn(M, hidden, generator=g, device=DEV).bfloat16()
w1 = (torch.randn(cin, 9 * hidden, generator=g, device=DEV) / (9 * hidden) ** 0.5).bfloat16()
dp1 = torch.zeros(M, hidden, device=DEV, dtype=torch.bfloat16)
tgt = torch.zeros(M, 64, device=DEV)
sk = L.ipoke_conv3x3_skinny_splitk(M, hidden, _lib.BF16)
nbytes = L.ipoke_conv_acc_scratch_bytes(M, 64, 32)
scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
_lib.check(L.ipoke_conv_acc_scratch_init(scratch.data_ptr(), _lib.current_stream()))

d2 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 1, 1), (1, 1, 1), (0, 0, 0))
d1 = ops.conv_desc(B, (1, 8, 8), (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1), True)
for d in (d2, d1):
    d.a_sn = 64 * hidden; d.a_sd = 0; d.a_sh = 8 * hidden; d.a_sw = hidden; d.a_sc = 1; d.Kc_real = hidden; d.Kc = hidden
d2.A = dp2.data_ptr(); d2.W = w2.data_ptr(); d2.ldw = hidden; d2.Nout = hidden; d2.w_kmajor = 1
d2.dact = h1.data_ptr(); d2.ld_dact = hidden; d2.dact_act = _lib.ACT_ELU; d2.C = dp1.data_ptr(); d2.ldc = hidden
d1.A = dp1.data_ptr(); d1.W = w1.data_ptr(); d1.ldw = 9 * hidden; d1.Nout = cin; d1.C = tgt.data_ptr(); d1.c_f32 = 1; d1.c_accumulate = 1
d1.ldc = 64; d1.c_cstride = 2; d1.splitk = sk; d1.acc_scratch = scratch.data_ptr(); d1.acc_scratch_bytes = nbytes


def timed(fn, iters=50, warm=5, rounds=5):
    """(median round, fastest round) of `rounds` rounds, each the mean launch time (us) of `iters` back-to-back calls"""
    out = []
    for _ in range(rounds):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    out.sort()
    return out[len(out) // 2], out[0]


def pair():
    ops.conv_forward(d2, "bf16")
    ops.conv_forward(d1, "bf16")


def gemm():
    ops.conv_forward(d2, "bf16")


def skinny():
    ops.conv_forward(d1, "bf16")


def fused():
    _lib.check(L.ipoke_conv_pair_dgrad(byref(d2), byref(d1), _lib.BF16, _lib.current_stream()))


print(f"M={M} hidden={hidden} cin={cin} skinny splitk={sk}; fused launch applies: "
      f"{L.ipoke_conv_pair_dgrad_applicable(M, hidden, cin, _lib.BF16, nbytes)}")
res = {}
for rnd in range(2):            # interleaved: every variant twice
    res.setdefault("a_pair", []).append(timed(pair))
    res.setdefault("gemm_rule_tile", []).append(timed(gemm))
    res.setdefault("skinny", []).append(timed(skinny))
    with _lib.dispatch_override("nn128", 2):
        res.setdefault("b_gemm_128", []).append(timed(gemm))
    if L.ipoke_conv_pair_dgrad_applicable(M, hidden, cin, _lib.BF16, nbytes):
        res.setdefault("c_fused", []).append(timed(fused))
for k, v in res.items():       # v: one (median round, fastest round) per pass
    print(f"{k:16s} best pass's median round {min(m for m, _ in v):7.2f} us   fastest round {min(m0 for _, m0 in v):7.2f} us   "
          f"(median round of each pass: {', '.join(f'{m:.2f}' for m, _ in v)})")
