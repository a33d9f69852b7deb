#!/usr/bin/env python3
"""Time the posture nearest-neighbour kernel (ipoke_posture_nn) at the size of the Iper training set and the reference's measure loop
(data/flow_dataset.py:635-646) in numpy on a sample of the same queries.

    python scripts/time_posture_nn.py [--n 180000] [--k 17] [--queries 200] [--launches 5] [--timeout 300]

Nothing imports this script.  The GPU step runs in a child process under its own time limit; if it fails or is killed the script stops
there and starts nothing more on the device.  The kernel time is taken with device events over ``--launches`` launches after one warm-up;
the numpy loop is timed on ``--queries`` queries and extrapolated to all N.  The child also checks the kernel's answers for those queries
against the float64 loop.  Operation count (kept with this script): per pair and keypoint two subtractions, one product, one fused
multiply-add (2), one square root and one addition = 7 fp32 operations -- the correctly rounded square root costs more instructions than
that, which is what the share of the vector peak below leaves unsaid."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_VECTOR = 157.3e12          # MI355X, FLOP/s (spec)
FLOP_PER_TERM = 7


def inputs(n, k):
    rs = np.random.RandomState(0)
    return rs.rand(n, k, 2).astype(np.float32), (np.arange(n) // 40).astype(np.int64)


def measure(kps, vid, idx):
    """the reference's measure(idx), float64"""
    sorted_ids = np.argsort(np.linalg.norm(kps[idx][None] - kps, axis=-1).sum(-1))
    nn_sa = sorted_ids[np.flatnonzero(vid[sorted_ids] != vid[idx])[0]]
    return sorted_ids[1], nn_sa


def gpu_step(args):
    import torch
    from ipoke_amd import _lib
    from ipoke_amd._lib import check, ptr
    assert torch.cuda.is_available(), "the kernel is timed on the GPU only"
    kps, vid = inputs(args.n, args.k)
    N, K = args.n, args.k
    L = _lib.lib()
    kp_d, vid_d = torch.from_numpy(kps).cuda(), torch.from_numpy(vid.astype(np.int32)).cuda()
    nn_g, nn_o = (torch.empty(N, dtype=torch.int64, device="cuda") for _ in range(2))
    ws = torch.empty(L.ipoke_posture_nn_workspace_bytes(N, K, N), dtype=torch.uint8, device="cuda")

    def launch():
        check(L.ipoke_posture_nn(ptr(kp_d), ptr(vid_d), None, N, K, N, ptr(nn_g), ptr(nn_o), None, ptr(ws), _lib.current_stream()))

    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    g, o = nn_g.cpu().numpy(), nn_o.cpu().numpy()
    q = np.linspace(0, N - 1, args.queries).astype(np.int64)
    kps64 = kps.astype(np.float64)
    agree = sum(int(measure(kps64, vid, int(i)) == (g[i], o[i])) for i in q[:32])
    print(json.dumps({"kernel_s": times, "agree_of_32": agree}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=180000)
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step == "gpu":
        return gpu_step(args)
    child = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", "gpu", "--n", str(args.n),
                            "--k", str(args.k), "--queries", str(args.queries), "--launches", str(args.launches)], capture_output=True, text=True)
    if child.returncode != 0:
        sys.stderr.write(child.stdout + child.stderr)
        sys.exit(f"the GPU step ended with status {child.returncode}: nothing more is started")
    res = json.loads(child.stdout.strip().splitlines()[-1])
    kernel = float(np.median(res["kernel_s"]))
    kps, vid = inputs(args.n, args.k)
    kps64 = kps.astype(np.float64)
    q = np.linspace(0, args.n - 1, args.queries).astype(np.int64)
    t0 = time.perf_counter()
    for i in q:
        measure(kps64, vid, int(i))
    per_query = (time.perf_counter() - t0) / len(q)
    flop = float(args.n) * args.n * args.k * FLOP_PER_TERM
    print(f"kernel: N = M = {args.n}, K = {args.k}: launches {['%.4f' % t for t in res['kernel_s']]} s, median {kernel:.4f} s; "
          f"{res['agree_of_32']} of 32 checked queries equal the float64 loop")
    print(f"numpy measure loop: {per_query * 1e3:.2f} ms per query on {len(q)} queries -> {per_query * args.n:.0f} s for all {args.n}")
    print(f"ratio (extrapolated): {per_query * args.n / kernel:.0f} x")
    print(f"achieved: {flop / kernel / 1e12:.2f} TFLOP/s at {FLOP_PER_TERM} operations per term = {100 * flop / kernel / PEAK_FP32_VECTOR:.1f} % of the "
          f"fp32 vector peak ({PEAK_FP32_VECTOR / 1e12:.1f} TFLOP/s)")
    print(json.dumps({"n": args.n, "k": args.k, "kernel_s": kernel, "numpy_s_per_query": per_query, "numpy_s_all": per_query * args.n,
                      "ratio": per_query * args.n / kernel, "tflops": flop / kernel / 1e12}))


if __name__ == "__main__":
    main()
