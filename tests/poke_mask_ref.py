"""CPU restatement of the masked poke rules and of the flow-derived mask (TEST INFRASTRUCTURE ONLY), in the arithmetic the kernels use:
fp32 amplitudes, sums in double, thresholds as fp32 adds.  Follows reference data/base_dataset.py:

    _get_poke with filter_flow (:520-538, :577-583)
        ordinary sample   amp_filt = mask ? amp : 0 on the window; mean / unbiased std of amp_filt; candidates amp_filt > mean + 2 std,
                          then (set empty) amp > mean + std, then amp > mean: the fallbacks test the unfiltered amplitude
        zero-poke sample  mean / std and the value sources from the unfiltered amplitude (:530, :543-553); centres = the window
                          positions where the mask is false, or, where there is none, amp < percentile(amp, 5)
    _compute_mask_with_flow (:343-351)   the whole map's amplitude, shifted to min 0, scaled to max 1, > mean + std

``get_poke`` takes the draws through an injected ``randint`` like oracle/data_ref.py.  tests/test_poke_mask_cpu.py holds it to golden G20,
which scripts/make_goldens_masked_pokes.py wrote from the reference's own methods.
"""
import numpy as np
import torch


def _stats(a):
    """mean and unbiased std of an fp32 map from double sums, rounded to fp32"""
    d = a.double().flatten()
    mean = d.sum() / d.numel()
    var = ((d - mean) ** 2).sum() / (d.numel() - 1)
    return mean.float(), var.sqrt().float()


def _normalised_amplitude(flow):
    amp = torch.norm(flow, 2, dim=0)
    amp = amp - amp.min()
    return amp / amp.max()


def flow_mask(flow):
    """flow fp32 [2, H, W] -> (mask bool [H, W], status: 1 for a constant map)"""
    raw = torch.norm(flow, 2, dim=0)
    amp = _normalised_amplitude(flow)
    mean, std = _stats(amp)
    return torch.gt(amp, mean + std), int(not bool((raw.max() - raw.min()) > 0))


def candidate_sets(flow, mask, poke_size, zero):
    """(centre positions [k, 2], value-source positions [m, 2] or None, rule) in window coordinates, row-major.  rule: 2 / 1 / 0 for the
    ordinary rules mean + 2 std / mean + std / mean, "bg" / "pct" for the zero-poke centre sets."""
    H, W = flow.shape[1:]
    h0, h1, w0, w1 = poke_size, H - poke_size, poke_size, W - poke_size
    amp = _normalised_amplitude(flow[:, h0:h1, w0:w1])
    m = mask[h0:h1, w0:w1].bool()
    if zero:
        mean, std = _stats(amp)
        src = torch.gt(amp, mean + std).nonzero(as_tuple=False)
        if src.shape[0] == 0:
            src = torch.gt(amp, mean).nonzero(as_tuple=False)
        cand, rule = torch.logical_not(m).nonzero(as_tuple=False), "bg"
        if cand.shape[0] == 0:
            cand, rule = torch.lt(amp, np.percentile(amp.numpy(), 5)).nonzero(as_tuple=False), "pct"
        return cand, src, rule
    filt = torch.where(m, amp, torch.zeros_like(amp))
    mean, std = _stats(filt)
    cand, rule = torch.gt(filt, mean + std * 2.0).nonzero(as_tuple=False), 2
    if cand.shape[0] == 0:
        cand, rule = torch.gt(amp, mean + std).nonzero(as_tuple=False), 1
        if cand.shape[0] == 0:
            cand, rule = torch.gt(amp, mean).nonzero(as_tuple=False), 0
    return cand, None, rule


def get_poke(flow, mask, poke_size, n_pokes, randint, zero=False, fix_n_pokes=False, equal_poke_val=True):
    """flow [2, H, W], mask bool [H, W] -> (poke [2, H, W], poke_centers int64 [n_pokes, 2]); raises ValueError when no candidate remains."""
    cand, src, _ = candidate_sets(flow, mask, poke_size, zero)
    shift = torch.tensor([[poke_size, poke_size]])
    cand = cand + shift
    if cand.shape[0] == 0 or (zero and src.shape[0] == 0):
        raise ValueError("empty candidate set")
    n = n_pokes if fix_n_pokes else int(randint(1, min(n_pokes, int(cand.shape[0])) + 1))
    if zero:
        src_sel = (src + shift)[randint(src.shape[0], size=n)]
    sel = cand[randint(cand.shape[0], size=n)]
    half = int(poke_size / 2)
    poke = torch.zeros_like(flow)
    centers = torch.full((n_pokes, 2), -1, dtype=torch.int64)
    for i in range(n):
        r, c = int(sel[i, 0]), int(sel[i, 1])
        sr, sc = (int(src_sel[i, 0]), int(src_sel[i, 1])) if zero else (r, c)
        if equal_poke_val:
            val = flow[:, sr, sc].unsqueeze(-1).unsqueeze(-1)
        else:
            val = flow[:, sr - half:sr + half + 1, sc - half:sc + half + 1]
        poke[:, r - half:r + half + 1, c - half:c + half + 1] = val
    centers[:n] = sel
    return poke, centers
