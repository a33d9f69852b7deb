#!/usr/bin/env python3
"""Time of the poke simulation with and without a foreground mask, in one call: B = 64 flows at 128 px, n_pokes = 5, poke_size 5, every
fifth sample a zero poke, a centred disc as the mask.  HIP events around each of 20 launches after 5 of warm-up, per variant:

    get_poke / get_poke_masked   ``PokeSimulator.get_poke`` without and with ``mask=`` (allocations and both kernels)
    abi / abi_masked             ``ipoke_poke_simulate`` / ``ipoke_poke_simulate_masked`` on buffers allocated once (both kernels only)
    abi_masked_all_true          the same under an all-true mask: the zero-poke samples find no background and run the 5th-percentile
                                 select as the unmasked launch does, so this is the like-for-like cost of the second window array

    python scripts/probe_poke_mask.py [--other-lib PATH/libipoke_hip.so] [--rounds 2]

Every measurement runs in a child process of its own under ``timeout``; with ``--other-lib`` (a build of another commit, handed to the
child as IPOKE_LIB_PATH) the children alternate between the two libraries, and for the other library only ``abi`` is timed, through
ctypes alone, since it need not export the masked entry points.  A failed child ends the run.  A record for DESIGN.md section 8 and
profiles/poke_mask.txt, not a gate; nothing imports this file.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S, POKE_SIZE, N_POKES, WARMUP, LAUNCHES = 64, 128, 5, 5, 5, 20
CHILD_SECONDS = 180


def timed(fn):
    import numpy as np
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(LAUNCHES):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)
    times = np.array(times)
    return {"median_us": round(float(np.median(times)), 2), "min_us": round(float(times.min()), 2), "max_us": round(float(times.max()), 2)}


def child():
    import torch
    from ipoke_amd import _lib
    from ipoke_amd._lib import ptr
    assert torch.cuda.is_available(), "the probe needs the GPU"
    dev = "cuda"
    handle = ctypes.CDLL(_lib.LIB_PATH)                       # not _lib.lib(): another commit's build need not export every bound symbol
    masked_abi = hasattr(handle, "ipoke_poke_simulate_masked")
    for name in ("ipoke_poke_workspace_bytes", "ipoke_poke_simulate") + (("ipoke_poke_masked_workspace_bytes", "ipoke_poke_simulate_masked")
                                                                         if masked_abi else ()):
        getattr(handle, name).restype, getattr(handle, name).argtypes = _lib.SIGNATURES[name]
    gen = torch.Generator(device=dev).manual_seed(3)
    coarse = torch.randn(B, 2, 6, 6, device=dev, generator=gen)
    flow = torch.nn.functional.interpolate(coarse, size=(S, S), mode="bicubic", align_corners=False).contiguous() * 10
    u = torch.rand(B, 1 + 2 * N_POKES, device=dev, generator=gen)
    zero = (torch.arange(B, device=dev) % 5 == 0).to(torch.int32)
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    mask = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (0.3 * S) ** 2).to(torch.uint8).expand(B, S, S).contiguous()
    poke, flow_out = torch.empty_like(flow), torch.empty_like(flow)
    centers = torch.empty(B, N_POKES, 2, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    stream = _lib.current_stream()
    res = {"lib": _lib.LIB_PATH, "shape": [B, S, POKE_SIZE, N_POKES], "launches": LAUNCHES}

    ws = torch.empty(handle.ipoke_poke_workspace_bytes(B, S, S, POKE_SIZE, N_POKES), dtype=torch.uint8, device=dev)

    def abi():
        rc = handle.ipoke_poke_simulate(ptr(flow), B, S, S, POKE_SIZE, N_POKES, 0, 1, ptr(zero), ptr(u), ptr(poke), ptr(centers), ptr(flow_out),
                                        ptr(status), ptr(ws), stream)
        assert rc == 0

    res["abi"] = timed(abi)
    assert int(status.sum()) == 0
    if masked_abi:
        from ipoke_amd.data import PokeSimulator
        ws2 = torch.empty(handle.ipoke_poke_masked_workspace_bytes(B, S, S, POKE_SIZE, N_POKES), dtype=torch.uint8, device=dev)

        def abi_masked():
            rc = handle.ipoke_poke_simulate_masked(ptr(flow), B, S, S, POKE_SIZE, N_POKES, 0, 1, ptr(zero), ptr(u), ptr(mask), ptr(poke), ptr(centers),
                                                   ptr(flow_out), ptr(status), ptr(ws2), stream)
            assert rc == 0

        res["abi_masked"] = timed(abi_masked)
        assert int(status.sum()) == 0
        disc = mask
        mask = torch.ones_like(disc)                          # no background: every zero-poke sample takes the percentile fallback
        res["abi_masked_all_true"] = timed(abi_masked)
        assert int(status.sum()) == 0
        mask = disc
        sim = PokeSimulator({"spatial_size": (S, S), "n_pokes": N_POKES, "poke_size": POKE_SIZE})
        res["get_poke"] = timed(lambda: sim.get_poke(flow, zero, u, strict=False))
        res["get_poke_masked"] = timed(lambda: sim.get_poke(flow, zero, u, strict=False, mask=mask))
        res["masked_over_unmasked"] = {"abi": round(res["abi_masked"]["median_us"] / res["abi"]["median_us"], 3),
                                       "abi_all_true": round(res["abi_masked_all_true"]["median_us"] / res["abi"]["median_us"], 3),
                                       "get_poke": round(res["get_poke_masked"]["median_us"] / res["get_poke"]["median_us"], 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.child:
        return child()
    libs = [None] + ([os.path.abspath(args.other_lib)] if args.other_lib else [])
    for _ in range(args.rounds):
        for lib in libs:
            env = dict(os.environ)
            env.pop("IPOKE_LIB_PATH", None)
            if lib:
                env["IPOKE_LIB_PATH"] = lib
            out = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child"], env=env,
                                 cwd=ROOT, capture_output=True, text=True)
            sys.stdout.write(out.stdout)
            sys.stdout.flush()
            if out.returncode != 0:                            # a fault, an abort or the time limit: start nothing more on the GPU
                sys.stderr.write(out.stderr[-4000:])
                return out.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
