#!/usr/bin/env python3
"""Golden G20: the reference's own BaseDataset._get_poke with filter_flow on (data/base_dataset.py:507-648, the mask branches at :520-538
and :577-583) and its _compute_mask_with_flow (:343-351), run on synthetic flows built like those of golden G11.

    python scripts/make_goldens_masked_pokes.py       # CPU, needs the reference checkout (oracle/ref_import.py); writes
                                                      # tests/golden/g20_masked_pokes.npz

Run by hand where the reference checkout is; nothing imports it and no GPU test needs it.  The reference's methods are called on the
SimpleNamespace stand-in of oracle/make_goldens.py's g11_data, with ``filter_flow=True`` and ``mask={"img_start": m}``, and with
``np.random.randint`` fed from the stored uniforms through oracle.data_ref.UniformDraws.

Cases: 64 px / poke 5, 128 px / poke 5, 128 px / poke 10; the flow kinds blobs, dense and flat; ordinary and zero-poke samples; the masks
blob (a smooth ellipse), all-true, all-false, flow-derived, and one that is true on the whole candidate window and false on the border
(a zero-poke sample then has no background in the window and falls back to the 5th percentile).  equal_poke_val is off in one case and
fix_n_pokes on in one.  One flow per (size, kind) is shared by its cases, so that the file stays small.

Condition for exactness.  Every index decision compares an fp32 array against mean + k std or a percentile; the reference reduces in
fp32, the kernels in double, and the two thresholds may differ in the last place.  For every rule a case applies -- and for the
flow-derived mask -- no element of the array the rule is applied to may lie within MARGIN = 1e-6 of the rule's threshold; exact zeros
against an exactly zero threshold do not count, that comparison is exact in any arithmetic.  A flow or a mask that violates the condition
is re-seeded, never tolerated, and the smallest margin met is printed and stored.  The percentile rule is the demanding one: its
threshold lies between two neighbouring order statistics, which the condition thereby keeps 1e-6 and more apart (the 128 px blob field
takes some eighty seeds for that), and the flat field, which takes no seed and whose symmetry puts equal amplitudes on both sides of the
percentile, is re-seeded by laying seeded noise of 0.02 over its ramp of spread 6.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import data_ref, ref_import                                   # noqa: E402
from oracle.make_goldens import _synthetic_raw_flow, gen                  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g20_masked_pokes.npz")
MAX_BYTES = 1024 * 1024
MARGIN = 1e-6
N_POKES = 5
SIZES = ((64, 96, 5), (128, 160, 5), (128, 160, 10))                       # spatial size, raw flow size, poke size
KINDS = ("blobs", "dense", "flat")
MASKS = ("blob", "true", "false", "flow", "window")
EQUAL_OFF = (128, 5, "blobs", False, "blob")                               # (size, poke size, kind, zero, mask) of the equal_poke_val=False case
FIX_ON = (128, 10, "dense", False, "flow")                                 # ... of the fix_n_pokes=True case


class Violation(Exception):
    pass


def rule_margin(arr, thr):
    """smallest |x - thr| over the array a rule is applied to, exact zeros against an exactly zero threshold left out"""
    thr = torch.as_tensor(thr, dtype=arr.dtype)
    keep = ~((arr == 0) & (thr == 0))
    return float((arr - thr).abs()[keep].min()) if bool(keep.any()) else float("inf")


def case_margin(flow, mask, ps, zero):
    """The rules _get_poke applies to this case, in the reference's fp32 arithmetic, and the smallest margin among them."""
    amp = torch.norm(flow[:, ps:-ps, ps:-ps], 2, dim=0)
    amp = amp - amp.min()
    amp = amp / amp.max()
    mw = torch.from_numpy(mask[ps:-ps, ps:-ps])
    out = []

    def rule(arr, thr):
        out.append(rule_margin(arr, thr))
        return bool(torch.gt(arr, thr).any())

    if zero:
        mean, std = amp.mean(), amp.std()
        if not rule(amp, mean + std):
            rule(amp, mean)
        if bool(mw.all()):
            out.append(rule_margin(amp, float(np.percentile(amp.numpy(), 5))))
    else:
        filt = torch.where(mw, amp, torch.zeros_like(amp))
        mean, std = filt.mean(), filt.std()
        if not rule(filt, mean + std * 2.0):
            if not rule(amp, mean + std):
                rule(amp, mean)
    return min(out)


def flow_mask_margin(flow):
    amp = torch.norm(flow, 2, dim=0)
    amp = amp - amp.min()
    amp = amp / amp.max()
    return rule_margin(amp, amp.mean() + amp.std())


def blob_mask(size, seed):
    """a smooth ellipse somewhere in the middle of the frame"""
    g = gen(seed)
    r = torch.rand(4, generator=g).tolist()
    cy, cx = size * (0.35 + 0.3 * r[0]), size * (0.35 + 0.3 * r[1])
    ry, rx = size * (0.15 + 0.2 * r[2]), size * (0.12 + 0.2 * r[3])
    yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0


def main():
    np.int, np.bool = int, bool                                            # the reference predates numpy 1.24
    bd = ref_import.ref("data.base_dataset")
    tmp = tempfile.mkdtemp()
    arrs, smallest, ci = {}, float("inf"), 0
    for size, hs in sorted({(s, h) for s, h, _ in SIZES}):
        for ki, kind in enumerate(KINDS):
            seed, tries = 2000 * size + 10 * ki, 0
            while True:                                                    # re-seed the flow and the blob mask on a violation
                try:
                    group, low = flow_group(bd, tmp, size, hs, ki, kind, seed, ci, tries > 0)
                    print(f"  {size}px {kind}: seed {seed} after {tries} re-seedings")
                    break
                except Violation as v:
                    tries += 1
                    seed += 37
                    assert tries < 5000, f"{size}px {kind}: no seed meets the condition ({v})"
            arrs.update(group)
            ci += sum(1 for k in group if k.startswith("meta"))
            smallest = min(smallest, low)
    arrs["n_cases"] = np.int64(ci)
    arrs["min_margin"] = np.float64(smallest)
    arrs["kinds"], arrs["masks"] = np.array(KINDS), np.array(MASKS)
    np.savez_compressed(OUT, **arrs)
    nbytes = os.path.getsize(OUT)
    assert nbytes <= MAX_BYTES, nbytes
    print(f"wrote {OUT}: {ci} cases, {nbytes / 1024:.1f} KiB; smallest threshold margin {smallest:.3e} (condition: > {MARGIN:g})")


def flow_group(bd, tmp, size, hs, ki, kind, seed, ci0, reseeded):
    """All cases of one (size, kind): one flow, every poke size of that spatial size, ordinary and zero-poke samples, every mask."""
    raw = _synthetic_raw_flow(seed, hs, kind)
    if kind == "flat" and reseeded:
        # the flat field takes no seed, and its symmetry in y puts equal amplitudes on both sides of the percentile: a re-seeded flat
        # field is the same ramp under seeded noise 400 times smaller than its spread, still without outliers beyond two standard deviations
        raw = raw + 0.02 * torch.randn(2, hs, hs, generator=gen(seed)).numpy().astype(np.float32)
    path = os.path.join(tmp, f"flow_{size}_{kind}_{seed}.npy")
    np.save(path, raw)

    def fake_for(ps, mask, fix, equal):
        cfg = {"spatial_size": (size, size), "n_pokes": N_POKES, "poke_size": ps}
        fake = types.SimpleNamespace(config=cfg, datadict={"flow_paths": np.array([[path]])}, valid_lags=[0], scale_poke_to_res=True, geom_transfs=None,
                                     poke_size=ps, valid_h=[ps, size - ps], valid_w=[ps, size - ps], filter_flow=True, fix_n_pokes=fix,
                                     equal_poke_val=equal, mask={"img_start": mask})
        fake._get_flow = lambda ids, _f=fake, **kw: bd.BaseDataset._get_flow(_f, ids, **kw)
        return fake

    flow = bd.BaseDataset._get_flow(fake_for(5, None, False, True), (0, 3))
    fmask = bd.BaseDataset._compute_mask_with_flow(fake_for(5, None, False, True), 0)
    assert fmask.dtype == bool and fmask.shape == (size, size)
    low = flow_mask_margin(flow)
    if low <= MARGIN:
        raise Violation(f"flow-derived mask margin {low:.3e}")
    out = {f"flow_{size}_{kind}": flow.numpy(), f"fmask_{size}_{kind}": fmask.astype(np.uint8)}
    # every case's margin first: a violation anywhere re-seeds the whole group before the reference has run
    cases = []
    for ps in [p for s, _, p in SIZES if s == size]:
        for zero in (False, True):
            for mi, mname in enumerate(MASKS):
                cseed = seed * 100 + 10 * ps + 2 * mi + int(zero)
                if mname == "blob":
                    m = blob_mask(size, cseed)
                elif mname == "flow":
                    m = fmask
                elif mname == "window":
                    m = np.zeros((size, size), dtype=bool)
                    m[ps:size - ps, ps:size - ps] = True
                else:
                    m = np.full((size, size), mname == "true")
                key = (size, ps, kind, zero, mname)
                margin = case_margin(flow, m, ps, zero)
                if margin <= MARGIN:
                    raise Violation(f"case {key}: margin {margin:.3e}")
                low = min(low, margin)
                cases.append((ps, zero, mi, mname, cseed, m, key, margin))
    ci = ci0
    for ps, zero, mi, mname, cseed, m, key, margin in cases:
        equal, fix = key != EQUAL_OFF, key == FIX_ON
        fake = fake_for(ps, m, fix, equal)
        ids = (0, -1 if zero else 3)
        u = torch.rand(1 + 2 * N_POKES, generator=gen(cseed + 7)).numpy().astype(np.float32)
        keep = np.random.randint
        np.random.randint = data_ref.UniformDraws(u, N_POKES, fix, zero)
        try:
            poke, centers = bd.BaseDataset._get_poke(fake, ids)
        finally:
            np.random.randint = keep
        flow_ret = bd.BaseDataset._get_flow(fake, ids)             # the sample's "flow" entry: zeros for zero pokes
        n = int((centers[:, 0] >= 0).sum())
        print(f"  case {ci}: {kind:5s} {size}px poke_size {ps} zero={int(zero)} mask={mname:6s} equal={int(equal)} fix={int(fix)}: "
              f"{n} pokes, margin {margin:.2e}")
        out.update({f"mask{ci}": m.astype(np.uint8), f"u{ci}": u, f"centers{ci}": centers.numpy().astype(np.int64),
                    f"poke_nz{ci}": poke.nonzero().numpy().astype(np.int16), f"poke_val{ci}": poke[poke != 0].numpy(),
                    f"flow_ret_abs{ci}": np.float64(flow_ret.abs().sum().item()),
                    f"meta{ci}": np.array([size, ps, int(zero), int(equal), int(fix), ki, mi])})
        ci += 1
    return out, low


if __name__ == "__main__":
    main()
