"""CPU restatements for the kernel-by-kernel tests of the device data path (TEST INFRASTRUCTURE ONLY): ``ipoke_flow_resize``, the unmasked
``ipoke_poke_simulate`` (poke_select_kernel<false> + poke_fill_kernel) and ``ipoke_flow_mask`` of csrc/data.hip, in the arithmetic the
kernels use, plus the table of small awkward cases tests/test_data_exact_cpu.py and tests/test_data_exact_gpu.py both walk.

    resize_ref   fp32 division first, then the align_corners=True bilinear interpolant in float64 at the exact rational coordinates, with
                 the three magnitudes per element the error bound of the GPU test is built from
    select_ref   the unmasked rules: tests/poke_mask_ref.py under an all-true mask (the filtered amplitude then is the amplitude, and a
                 zero-poke sample finds no background and falls to the percentile rule), the draws through oracle/data_ref.UniformDraws
    robust       whether any decision of a case could hinge on the order of the kernel's double sums
    fill_ref     the poke tensor and the returned flow
    cases()      the table; tie_cases() the few cases that tie with a threshold, held to sums_are_exact in place of robust

The amplitude is formed HERE, sqrt(fl(fl(vx vx) + fl(vy vy))) on numpy float32 arrays, where every operation is rounded on its own.  The
rules of poke_mask_ref take it through ``torch.norm``, whose CPU build is free to fuse the multiply into the add; so they are handed the
surrogate flow (amplitude, 0), of which every evaluation of sqrt(a a + 0 0), fused or not, is a again: a a + 0 is one rounding either way
and the correctly rounded root of a correctly rounded square of a binary float is that float (no case here comes near under- or
overflow).  ``_amplitude`` asserts it.

Every field is built from ``RandomState.randint`` draws by exact float64 arithmetic and rounded to fp32 once, so the table is the same on
every machine: the seeds were chosen (on the CPU, by tests/test_data_exact_cpu.py) so that every case is ``robust``.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import data_ref
from tests import poke_mask_ref as R

F32 = np.float32
LAST = np.nextafter(F32(1), F32(0))                       # the largest fp32 below 1: the pick of the last candidate
K_THREADS = 1024                                          # kPokeThreads of csrc/data.hip


# ------------------------------------------------------------------------------------------------------------------ flow resize
def _axis(n_in, n_out):
    """per output index: the lower tap, the upper tap, the tap below the lower one where the exact coordinate is an integer (a computed
    coordinate a rounding below it interpolates in that cell), and the float64 weight of the upper tap"""
    o = np.arange(n_out, dtype=np.int64)
    if n_out == 1:
        num, den = np.zeros(1, dtype=np.int64), 1
    else:
        num, den = o * (n_in - 1), n_out - 1
    i0 = num // den
    w = (num % den).astype(np.float64) / den
    i1 = np.minimum(i0 + 1, n_in - 1)
    im = np.where((w == 0) & (i0 > 0), i0 - 1, i0)
    return i0, i1, im, w


def resize_ref(src_f32, Ho, Wo, div):
    """src fp32 [..., Hi, Wi] -> (ref float64 [..., Ho, Wo], m, sy, sx), the last three float64 of the same shape.

    a = fl32(src / div); ref = the bilinear interpolant of a with align_corners=True, in float64, at oy (Hi - 1) / (Ho - 1) (0 for
    Ho == 1), floor and fraction taken on the integers.  m = max |tap|, sy (sx) = the largest difference of two vertically (horizontally)
    adjacent taps: over the four taps of the cell, and, where a coordinate is exactly an integer, over the cell before it as well, since
    a coordinate computed in fp32 may land a rounding below the integer; the interpolant is continuous there, and its slope on that side
    is the other cell's."""
    src = np.asarray(src_f32)
    assert src.dtype == np.float32
    Hi, Wi = src.shape[-2:]
    a = (src / F32(div)).astype(np.float32).astype(np.float64)
    y0, y1, ym, wy = _axis(Hi, Ho)
    x0, x1, xm, wx = _axis(Wi, Wo)
    rows, cols = [ym, y0, y1], [xm, x0, x1]
    T = [[a[..., r[:, None], c[None, :]] for c in cols] for r in rows]
    wy, wx = wy[:, None], wx[None, :]
    top = (1.0 - wx) * T[1][1] + wx * T[1][2]
    bot = (1.0 - wx) * T[2][1] + wx * T[2][2]
    ref = (1.0 - wy) * top + wy * bot
    m = functools.reduce(np.maximum, [np.abs(T[i][j]) for i in range(3) for j in range(3)])
    sy = functools.reduce(np.maximum, [np.abs(T[i + 1][j] - T[i][j]) for i in range(2) for j in range(3)])
    sx = functools.reduce(np.maximum, [np.abs(T[i][j + 1] - T[i][j]) for i in range(3) for j in range(2)])
    return ref, m, sy, sx


def resize_bound(m, sy, sx, Hi, Wi):
    """|got - ref| per element: 2^-23 (8 m + 2 (Hi - 1) sy + 2 (Wi - 1) sx).  8 m: three fp32 interpolation steps over the taps, each a
    1 - w, two products and a sum (fused or not), under 2.5 roundings of 2^-24 relative to m apiece.  The sy term: the kernel's coordinate
    fl(oy fl(s)) is off by at most two relative roundings of a value <= Hi - 1, and the interpolant moves by at most sy per unit; the sx
    term likewise."""
    return 2.0 ** -23 * (8.0 * m + 2.0 * (Hi - 1) * sy + 2.0 * (Wi - 1) * sx)


# (B, C, Hi, Wi) -> (Ho, Wo); "identity" and "integer" are the shapes whose every weight is exactly 0
RESIZE_SHAPES = [
    ((1, 2, 7, 5), (3, 4), ""),
    ((2, 2, 4, 4), (9, 11), ""),                           # upsampling
    ((1, 2, 5, 9), (1, 1), ""),
    ((1, 2, 5, 9), (1, 6), ""),
    ((1, 2, 5, 9), (6, 1), ""),
    ((1, 1, 1, 1), (4, 4), ""),
    ((1, 2, 6, 6), (6, 6), "identity"),
    ((1, 2, 3, 1000), (2, 999), ""),
    ((3, 2, 64, 64), (420, 420), ""),                      # 1 058 400 elements: past one pass of the capped grid (4096 x 256)
    ((2, 2, 9, 13), (5, 7), "integer"),
]
RESIZE_DIVS = (1.0, 2.0, 3.0)


def _mantissas(rs, shape, scale):
    """full 24-bit mantissas, uniform in (-scale, scale): exact in fp32, the same on every machine"""
    return (rs.randint(-2 ** 23, 2 ** 23, size=shape).astype(np.float64) * (scale / 2.0 ** 23)).astype(np.float32)


def resize_inputs(shape, seed):
    """the two inputs of a resize shape: normal floats times 10, and a copy whose last channel is offset by 1e4"""
    x = (np.random.RandomState(seed).standard_normal(shape) * 10.0).astype(np.float32)
    y = x.copy()
    y[:, -1] += F32(1e4)
    return x, y


# ------------------------------------------------------------------------------------------------------------------ poke select
def _amplitude(flow, window):
    """fp32 sqrt(fl(fl(vx vx) + fl(vy vy))) on numpy arrays -> (amplitude on the window, the surrogate flow the rules are handed)"""
    f = np.asarray(flow, dtype=np.float32)
    h0, h1, w0, w1 = window
    vx, vy = f[0, h0:h1, w0:w1], f[1, h0:h1, w0:w1]
    amp = np.sqrt(vx * vx + vy * vy)
    assert amp.dtype == np.float32
    sur = torch.zeros(2, f.shape[1], f.shape[2])
    sur[0, h0:h1, w0:w1] = torch.from_numpy(amp)
    assert torch.equal(torch.norm(sur[:, h0:h1, w0:w1], 2, dim=0), torch.from_numpy(amp)), "the surrogate does not carry the amplitude"
    return amp, sur


def _ulp(x, k):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def _percentile_parts(amp):
    """np.percentile(amp, 5) as the kernel takes it apart: (value rounded to fp32, g, a[k], a[k + 1])"""
    flat = np.sort(amp.flatten())
    n = flat.size
    vi = 0.05 * (n - 1)
    k = int(np.floor(vi))
    return F32(np.percentile(amp, 5)), vi - k, flat[k], flat[min(k + 1, n - 1)]


def _sets(amp, zero, mean, std, pct):
    """candidate and value-source sets (flat window indices) of a normalised fp32 amplitude under the given fp32 statistics, with the
    thresholds formed as the kernel forms them: fl(mean + fl(std 2)), fl(mean + std), mean"""
    mean, std = F32(mean), F32(std)
    a = amp.flatten()
    t2, t1 = F32(mean + F32(std * F32(2))), F32(mean + std)
    c2, c1, c0 = a > t2, a > t1, a > mean
    if zero:
        return np.flatnonzero(a < F32(pct)), np.flatnonzero(c1 if c1.any() else c0)
    cand = c2 if c2.any() else c1 if c1.any() else c0
    return np.flatnonzero(cand), None


def select_ref(flow, poke_size, n_pokes, fix_n_pokes, zero, u):
    """flow fp32 [2, H, W], u fp32 [1 + 2 n_pokes] -> SimpleNamespace(
        centers int64 [n_pokes, 2] (row, col), -1 padded; src int64 [n_pokes, 2], the value-source positions (the centres themselves for an
        ordinary sample); np, the number of pokes; status (1: no candidate, then np = 0 and every centre is -1); rule: 2 / 1 / 0 / "pct";
        src_rule: 1 / 0 for a zero-poke sample (value sources > mean + std, or > mean), else None; pct_branch: ">=" / "<" for g >= 0.5 or
        g < 0.5 of the percentile interpolation, else None; pct_tied: whether the two order statistics around it are equal;
        amp fp32 [H - 2 ps, W - 2 ps], the normalised amplitude; cand / srcs, the whole sets as flat window indices)."""
    flow = torch.as_tensor(flow, dtype=torch.float32)
    H, W = flow.shape[1:]
    ps = int(poke_size)
    _, sur = _amplitude(flow.numpy(), (ps, H - ps, ps, W - ps))
    ww = W - 2 * ps
    with np.errstate(invalid="ignore"):
        cand, src, rule = R.candidate_sets(sur, torch.ones(H, W, dtype=torch.bool), ps, bool(zero))
        amp = R._normalised_amplitude(sur[:, ps:H - ps, ps:W - ps]).numpy()
    out = SimpleNamespace(centers=np.full((n_pokes, 2), -1, dtype=np.int64), src=np.full((n_pokes, 2), -1, dtype=np.int64), np=0, status=1,
                          rule=rule, src_rule=None, pct_branch=None, pct_tied=None, amp=amp,
                          cand=(cand[:, 0] * ww + cand[:, 1]).numpy(), srcs=None if src is None else (src[:, 0] * ww + src[:, 1]).numpy())
    if cand.shape[0] == 0 or (zero and src.shape[0] == 0):
        return out
    if zero:
        mean, std = R._stats(torch.from_numpy(amp))
        out.src_rule = 1 if bool((torch.from_numpy(amp) > mean + std).any()) else 0
        _, g, ak, ak1 = _percentile_parts(amp)
        out.pct_branch, out.pct_tied = (">=" if g >= 0.5 else "<"), bool(ak == ak1)
    draw = data_ref.UniformDraws(np.asarray(u, dtype=np.float32), n_pokes, bool(fix_n_pokes), bool(zero))
    n = n_pokes if fix_n_pokes else int(draw(1, min(n_pokes, int(cand.shape[0])) + 1))
    if zero:
        out.src[:n] = (src + ps)[draw(src.shape[0], size=n)].numpy()
    out.centers[:n] = (cand + ps)[draw(cand.shape[0], size=n)].numpy()
    if not zero:
        out.src[:n] = out.centers[:n]
    out.np, out.status = n, 0
    return out


def robust(case):
    """Whether the candidate and value-source sets of ``case`` stay what they are when the fp32 mean and the fp32 std each move one ulp up
    or down (nine combinations) and, for a zero-poke sample, the percentile value does too.  The kernel's double sums run in another order
    than torch's, so either statistic may in principle come out one fp32 ulp away; a case that passes here is decided alike by both.

    The percentile is moved only where the two order statistics around it differ: where they are equal, a + 0 g and b - 0 (1 - g) are
    that value in any arithmetic, nothing is rounded and nothing can differ."""
    sel = select_ref(case.flow, case.ps, case.n_pokes, case.fix, case.zero, case.u)
    amp = sel.amp
    if not np.isfinite(amp).all():                      # a constant map: 0 / 0 everywhere, no comparison passes whatever the statistics
        return sel.status == 1
    mean, std = (F32(v) for v in R._stats(torch.from_numpy(amp)))
    pct, moves = None, [0]
    if case.zero:
        pct, _, ak, ak1 = _percentile_parts(amp)
        moves = [0] if ak == ak1 else [-1, 0, 1]
    base = _sets(amp, case.zero, mean, std, pct)
    if not np.array_equal(base[0], sel.cand) or (case.zero and not np.array_equal(base[1], sel.srcs)):
        return False                                     # the two statements of the rules disagree: nothing to build on
    for dm in (-1, 0, 1):
        for ds in (-1, 0, 1):
            for dp in moves:
                got = _sets(amp, case.zero, _ulp(mean, dm), _ulp(std, ds), None if pct is None else _ulp(pct, dp))
                if not np.array_equal(got[0], base[0]) or (case.zero and not np.array_equal(got[1], base[1])):
                    return False
    return True


def flow_mask_ref(flow):
    """(mask bool [H, W], status) of poke_mask_ref.flow_mask on the surrogate of ``flow`` [2, H, W], and whether the mask is robust: the
    same under a mean and a std one fp32 ulp up or down"""
    f = np.asarray(flow, dtype=np.float32)
    H, W = f.shape[1:]
    _, sur = _amplitude(f, (0, H, 0, W))
    with np.errstate(invalid="ignore"):
        mask, status = R.flow_mask(sur)
        amp = R._normalised_amplitude(sur).numpy()
    ok = True
    if status == 0:
        mean, std = (F32(v) for v in R._stats(torch.from_numpy(amp)))
        for dm in (-1, 0, 1):
            for ds in (-1, 0, 1):
                ok = ok and np.array_equal(amp > F32(_ulp(mean, dm) + _ulp(std, ds)), mask.numpy())
    return mask, status, ok


# ------------------------------------------------------------------------------------------------------------------ poke fill
def fill_ref(flow, sel, zero, half, equal_val):
    """(poke [2, H, W], flow_out [2, H, W]) as numpy fp32: pokes 0 .. np - 1 written in that order, so the last one covering a pixel wins;
    the value is the flow at the source position (equal_val) or at the source position plus the offset inside the patch; flow_out is the
    flow, zeroed for a zero-poke sample."""
    f = np.asarray(flow, dtype=np.float32)
    poke = np.zeros_like(f)
    for j in range(sel.np):
        (r, c), (sr, sc) = sel.centers[j], sel.src[j]
        for dy in range(-half, half + 1):
            for dx in range(-half, half + 1):
                poke[:, r + dy, c + dx] = f[:, sr, sc] if equal_val else f[:, sr + dy, sc + dx]
    return poke, (np.zeros_like(f) if zero else f.copy())


# ------------------------------------------------------------------------------------------------------------------ fields
def _jitter(rs, shape):
    return rs.randint(-2 ** 23, 2 ** 23, size=shape).astype(np.float64) * 2.0 ** -29        # below 2^-6, the low bits of the mantissa


def smooth_field(H, W, seed):
    """a coarse integer grid, bilinearly upsampled on exact weights k / 16, plus low-order jitter: peaked, so rule 2 finds candidates"""
    rs = np.random.RandomState(seed)
    gh, gw = (H + 15) // 16 + 1, (W + 15) // 16 + 1
    g = rs.randint(-40, 41, size=(2, gh, gw)).astype(np.float64)
    y, x = np.arange(H), np.arange(W)
    y0, x0, wy, wx = y // 16, x // 16, (y % 16)[:, None] / 16.0, (x % 16)[None, :] / 16.0
    f = ((1 - wy) * ((1 - wx) * g[:, y0][:, :, x0] + wx * g[:, y0][:, :, x0 + 1])
         + wy * ((1 - wx) * g[:, y0 + 1][:, :, x0] + wx * g[:, y0 + 1][:, :, x0 + 1]))
    return (f + _jitter(rs, f.shape)).astype(np.float32)


def flat_field(H, W, seed):
    """amplitude close to uniform on [8, 16): nothing above mean + 2 std, the upper fifth above mean + std -- rule 1"""
    rs = np.random.RandomState(seed)
    f = np.stack([8.0 + rs.randint(0, 2 ** 23, size=(H, W)).astype(np.float64) * 2.0 ** -20, rs.randint(0, 2 ** 23, size=(H, W)).astype(np.float64) * 2.0 ** -23])
    return f.astype(np.float32)


def two_valued_field(H, W, seed=None):
    """amplitude 1 on the left half and 3 on the right, as in the masked suite's last-fallback test: the maximum sits at mean + std' with
    std' just below the unbiased std, so only amp > mean selects -- rule 0"""
    f = np.zeros((2, H, W), dtype=np.float32)
    f[0, :, :W // 2], f[0, :, W // 2:] = 1.0, 3.0
    return f


def integer_field(H, W, seed):
    """components in -3 .. 3: a dozen distinct amplitudes, most pixels tied with many others"""
    return np.random.RandomState(seed).randint(-3, 4, size=(2, H, W)).astype(np.float32)


def spike_field(H, W, seed, ps, spikes):
    """amplitudes in [1, 2) and a few spikes of 30 at the given window positions: those alone pass mean + 2 std"""
    rs = np.random.RandomState(seed)
    f = np.stack([1.0 + rs.randint(0, 2 ** 23, size=(H, W)).astype(np.float64) * 2.0 ** -23, np.zeros((H, W))])
    for k, (r, c) in enumerate(spikes):
        f[:, ps + r, ps + c] = (30.0 + k, 0.25 * k)                 # distinct values, so that which poke won shows in the tensor
    return f.astype(np.float32)


def tie_field(H, W, seed, ps):
    """amplitude 1 on half of the window (rounded down), 3 on as many pixels and 2 on the one left (window position 3): normalised 0, 1 and
    0.5, whose mean is 0.5 and whose unbiased std is 0.5, both exactly.  Nothing passes mean + std = 1, and the one pixel at 0.5 EQUALS
    the threshold of the last rule, amp > mean."""
    wh, ww = H - 2 * ps, W - 2 * ps
    n = wh * ww
    assert n % 2 == 1
    order = [i for i in np.random.RandomState(seed).permutation(n) if i != 3]
    vals = np.full(n, 2.0)
    vals[order[:n // 2]], vals[order[n // 2:]] = 1.0, 3.0
    f = np.zeros((2, H, W))
    f[0] = 2.0
    f[0, ps:H - ps, ps:W - ps] = vals.reshape(wh, ww)
    return f.astype(np.float32)


def low_tail_field(H, W, seed, ps):
    """a zero-poke field whose value sources fall back to > mean: on the window 3 % of the pixels have amplitude 0, 40 % 2 and the rest 3,
    so nothing passes mean + std, the 5th percentile lies among the tied 2s and the centres are the 0s"""
    rs = np.random.RandomState(seed)
    wh, ww = H - 2 * ps, W - 2 * ps
    n = wh * ww
    vals = np.full(n, 3.0)
    order = rs.permutation(n)
    n0 = max(1, (3 * n) // 100)
    vals[order[:n0]], vals[order[n0:n0 + (40 * n) // 100]] = 0.0, 2.0
    f = np.full((2, H, W), 0.0)
    f[0] = 2.0
    f[0, ps:H - ps, ps:W - ps] = vals.reshape(wh, ww)
    return f.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the case table
def _u(n_pokes, count=0.5, src=0.5, cen=0.5):
    """a row of uniforms: scalars are repeated, lists are taken as they are"""
    row = np.empty(1 + 2 * n_pokes, dtype=np.float32)
    row[0], row[1:1 + n_pokes], row[1 + n_pokes:] = count, src, cen
    return row


def _mid(idx, count):
    """uniforms that pick the candidates ``idx`` of ``count``: the middle of each one's interval"""
    return ((np.asarray(idx, dtype=np.float64) + 0.5) / count).astype(np.float32)


def _case(name, field, win, ps, n_pokes, fix, zero, equal, u, want_rule):
    """``win`` = the window (rows, cols); the map is 2 ps larger each way.  ``u``: a row, or a function (case, sets) -> row for rows that
    name particular candidates."""
    H, W = win[0] + 2 * ps, win[1] + 2 * ps
    c = SimpleNamespace(name=name, H=H, W=W, ps=ps, n_pokes=n_pokes, fix=bool(fix) or n_pokes == 1, zero=bool(zero), equal=bool(equal),
                        flow=field(H, W), want_rule=want_rule, n=win[0] * win[1])
    if callable(u):
        c.u = _u(n_pokes)
        sets = select_ref(c.flow, ps, n_pokes, c.fix, c.zero, c.u)
        u = u(c, sets)
    c.u = np.asarray(u, dtype=np.float32)
    assert c.u.shape == (1 + 2 * n_pokes,)
    return c


def _straddle(c, sets):
    """picks on either side of a thread's chunk boundary: two candidates at window positions i, i + 1 with i + 1 a multiple of
    per = ceil(n / 1024), then their neighbours in the candidate order"""
    per = -(-c.n // K_THREADS)
    pos = sets.cand
    j = next(j for j in range(len(pos) - 1) if pos[j + 1] == pos[j] + 1 and pos[j + 1] % per == 0)
    idx = [(j + k) % len(pos) for k in range(c.n_pokes)]
    return _u(c.n_pokes, count=LAST, src=_mid([k % len(sets.srcs) for k in range(c.n_pokes)], len(sets.srcs)) if c.zero else 0.5,
              cen=_mid(idx, len(pos)))


def _adjacent(c, sets):
    """neighbouring and equal picks: candidates j, j + 1, j + 1, j + 2, ... from the middle of the set, so that the patches overlap"""
    cnt = len(sets.cand)
    j = cnt // 2
    idx = [min(j + (k + 1) // 2, cnt - 1) for k in range(c.n_pokes)]
    return _u(c.n_pokes, count=LAST, src=_mid([(3 * k) % len(sets.srcs) for k in range(c.n_pokes)], len(sets.srcs)) if c.zero else 0.5,
              cen=_mid(idx, cnt))


def _corners(win):
    return [(0, 0), (0, win[1] - 1), (win[0] - 1, 0), (win[0] - 1, win[1] - 1)]


@functools.lru_cache(maxsize=None)
def cases():
    S, Fl, T, I = smooth_field, flat_field, two_valued_field, integer_field
    f = functools.partial
    two_equal = lambda n: _u(n, count=LAST, cen=[0.25, 0.25] + [0.75] * (n - 2)) if n > 1 else _u(n)
    out = [
        # windows at the 1024-thread block boundary, every poke size, both fix_n_pokes settings, n_pokes 1 / 5 / 16
        _case("w31x33_smooth_first", f(S, seed=1), (31, 33), 1, 5, False, False, True, _u(5, 0.0, 0.0, 0.0), 2),
        _case("w31x33_smooth_last", f(S, seed=2), (31, 33), 2, 16, False, False, True, _u(16, LAST, LAST, LAST), 2),
        _case("w32x32_smooth_equal", f(S, seed=3), (32, 32), 3, 5, True, False, True, two_equal(5), 2),
        _case("w32x32_smooth_one", f(S, seed=4), (32, 32), 4, 1, True, False, False, _u(1, 0.3, 0.3, 0.6), 2),
        _case("w32x32_flat_last", f(Fl, seed=5), (32, 32), 5, 16, True, False, True, _u(16, LAST, LAST, LAST), 1),
        _case("w25x41_smooth_straddle", f(S, seed=6), (25, 41), 3, 5, False, False, False, _straddle, 2),
        _case("w25x41_flat_straddle", f(Fl, seed=7), (25, 41), 2, 16, False, False, True, _straddle, 1),
        _case("w25x41_two_valued", T, (25, 41), 5, 5, False, False, True, _u(5, 0.7, 0.1, [0.0, LAST, 0.5, 0.5, 0.2]), 0),
        _case("w31x33_two_valued_first", T, (31, 33), 4, 16, True, False, False, _u(16, 0.0, 0.0, 0.0), 0),
        _case("w31x33_flat_first", f(Fl, seed=8), (31, 33), 1, 1, True, False, True, _u(1, 0.0, 0.0, 0.0), 1),
        # the 4-element minimum window, H = W = 2 ps + 2
        _case("w2x2_random", f(lambda H, W, seed: _mantissas(np.random.RandomState(seed), (2, H, W), 16.0), seed=9), (2, 2), 1, 5, False, False,
              True, _u(5, LAST, 0.5, LAST), 1),
        _case("w2x2_two_valued", T, (2, 2), 5, 5, True, False, False, _u(5, 0.0, 0.0, [0.0, LAST, 0.0, LAST, 0.5]), 0),
        _case("w2x2_zero", f(lambda H, W, seed: _mantissas(np.random.RandomState(seed), (2, H, W), 16.0), seed=10), (2, 2), 2, 5, False, True,
              True, _u(5, LAST, LAST, LAST), "pct"),
        # the larger non-square map
        _case("w40x72_smooth_straddle", f(S, seed=11), (40, 72), 4, 5, False, False, False, _straddle, 2),
        _case("w40x72_zero_smooth", f(S, seed=12), (40, 72), 4, 16, False, True, False, _straddle, "pct"),      # frac(0.05 (n - 1)) = 0.95
        # zero-poke samples: ties, both sides of frac = 0.5, the value-source fallback
        _case("w31x33_zero_integer", f(I, seed=13), (31, 33), 2, 5, False, True, True, _u(5, LAST, [0.0, LAST, 0.5, 0.5, 0.3], [0.0, LAST, 0.5, 0.5, 0.3]),
              "pct"),                                                                                            # frac = 0.1
        _case("w32x32_zero_adjacent_patch", f(S, seed=14), (32, 32), 3, 5, True, True, False, _adjacent, "pct"),        # frac = 0.15
        _case("w25x41_zero_smooth", f(S, seed=15), (25, 41), 3, 5, False, True, True, _u(5, 0.5, 0.9, 0.1), "pct"),   # frac = 0.2
        _case("w5x7_zero_integer", f(I, seed=16), (5, 7), 2, 5, False, True, True, _u(5, LAST, 0.0, 0.0), "pct"),      # frac = 0.7
        _case("w25x41_zero_low_tail", f(low_tail_field, seed=17, ps=3), (25, 41), 3, 5, False, True, True, _u(5, LAST, [0.0, LAST, 0.4, 0.4, 0.8], LAST), "pct"),
        _case("w6x9_zero_low_tail", f(low_tail_field, seed=18, ps=1), (6, 9), 1, 16, True, True, True, _u(16, 0.0, LAST, 0.0), "pct"),   # frac = 0.65
        # fewer candidates than n_pokes
        _case("w32x32_three_spikes", f(spike_field, seed=19, ps=2, spikes=[(3, 4), (3, 6), (20, 31)]), (32, 32), 2, 5, False, False, True,
              _u(5, LAST, 0.5, [0.0, LAST, 0.5, 0.0, 0.0]), 2),
        _case("w25x41_two_spikes", f(spike_field, seed=20, ps=3, spikes=[(0, 0), (24, 40)]), (25, 41), 3, 5, False, False, False,
              _u(5, LAST, 0.5, [LAST, 0.0, 0.5, 0.0, 0.0]), 2),
        # overlap and order: adjacent centres, equal_poke_val on and off; centres in the window's corners
        _case("w25x41_adjacent_equal", f(S, seed=21), (25, 41), 4, 5, True, False, True, _adjacent, 2),
        _case("w25x41_adjacent_patch", f(S, seed=21), (25, 41), 4, 5, True, False, False, _adjacent, 2),
        _case("w31x33_adjacent_patch16", f(S, seed=22), (31, 33), 5, 16, True, False, False, _adjacent, 2),
        _case("w25x41_corners_equal", f(spike_field, seed=23, ps=5, spikes=_corners((25, 41))), (25, 41), 5, 5, True, False, True,
              _u(5, 0.0, 0.5, _mid([0, 1, 2, 3, 0], 4)), 2),
        _case("w32x32_corners_patch", f(spike_field, seed=24, ps=3, spikes=_corners((32, 32))), (32, 32), 3, 5, True, False, False,
              _u(5, 0.0, 0.5, _mid([3, 2, 1, 0, 3], 4)), 2),
        # the rest of the batch of five (map 31 x 47, poke 3, n_pokes 5): see batch_of_five
        _case("w25x41_flat", f(Fl, seed=25), (25, 41), 3, 5, False, False, True, _u(5, 0.6, 0.5, [0.1, 0.9, 0.5, 0.3, 0.7]), 1),
        _case("w25x41_smooth", f(S, seed=26), (25, 41), 3, 5, False, False, True, _u(5, LAST, 0.5, [0.1, 0.9, 0.5, 0.3, 0.7]), 2),
        _case("w25x41_zero_integer", f(I, seed=27), (25, 41), 3, 5, False, True, True, _u(5, 0.4, [0.1, 0.9, 0.5, 0.3, 0.7], [0.7, 0.3, 0.5, 0.9, 0.1]), "pct"),
    ]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def tie_cases():
    """Cases in which an amplitude EQUALS the threshold it is compared with, so that > and >= part ways.  Such a case cannot be ``robust``
    (a threshold one ulp lower admits the tied pixel); it is held to more: ``sums_are_exact``, under which no order of summation rounds
    anything and the statistics are the same numbers everywhere."""
    f = functools.partial
    return [
        _case("w25x41_tie_with_mean", f(tie_field, seed=31, ps=3), (25, 41), 3, 5, True, False, True, _u(5, 0.5, 0.5, [0.0, 0.3, 0.6, LAST, 0.01]), 0),
        _case("w5x7_tie_with_mean", f(tie_field, seed=32, ps=2), (5, 7), 2, 16, False, False, False, _u(16, LAST, 0.5, [0.0, LAST] + [0.4] * 14), 0),
    ]


def sums_are_exact(amp):
    """Whether the mean and the unbiased variance of a normalised fp32 amplitude come out the same in double whatever the order of the
    sums and whether or not a multiply is fused into an add: every term and every partial sum is exactly representable (non-negative
    terms on a common binary grid whose total stays below 2^53 grid steps), and so are the mean, the deviations, their squares and the
    variance.  The root is then rounded once."""
    from fractions import Fraction

    def any_order(terms):
        nz = [v for v in terms if v]
        return not nz or sum(nz) * max(v.denominator for v in nz) < 2 ** 53

    def is_double(v):
        return Fraction(float(v)) == v

    a = [Fraction(float(v)) for v in np.asarray(amp, dtype=np.float32).flatten()]
    n = len(a)
    if not any_order(a):
        return False
    mean = sum(a) / n
    d2 = [(v - mean) ** 2 for v in a]
    return bool(is_double(mean) and all(is_double(v - mean) for v in a) and all(is_double(v) for v in d2) and any_order(d2)
                and is_double(sum(d2) / (n - 1)))


def case(name):
    return next(c for c in cases() + tie_cases() if c.name == name)


def batch_of_five():
    """ordinary and zero-poke samples of one geometry around a constant-flow sample, which has no candidate (status 1)"""
    picked = [case(n) for n in ("w25x41_smooth", "w25x41_zero_smooth", None, "w25x41_flat", "w25x41_zero_integer") if n]
    const = SimpleNamespace(**{**vars(picked[0]), "name": "constant", "flow": np.full_like(picked[0].flow, 0.25), "want_rule": None})
    picked.insert(2, const)
    assert len({(c.H, c.W, c.ps, c.n_pokes, c.fix, c.equal) for c in picked}) == 1
    return picked


MASK_SHAPES = [(1, 2), (31, 33), (32, 32), (25, 41), (3, 700)]          # none of them is run by tests/test_poke_mask_gpu.py (64^2, 128^2)


def mask_flows():
    """per shape a smooth field, a flat field and (last) a constant map"""
    return [(H, W, np.stack([smooth_field(H, W, 40 + i), flat_field(H, W, 50 + i), np.full((2, H, W), 0.5, dtype=np.float32)]))
            for i, (H, W) in enumerate(MASK_SHAPES)]
