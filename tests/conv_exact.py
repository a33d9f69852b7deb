"""Bit-exact checking of the convolution kernels (ipoke_conv_forward / ipoke_conv_wgrad): operands chosen so that fp32 arithmetic is
exact in any summation order, a float64 reference computed from the descriptor itself, sentinel-filled buffers around everything a
kernel may touch, and an exact comparator.

Operands are small integers (bf16- and fp32-exact), biases are integral and row scales powers of two.  The generator asserts that every
output satisfies sum |x * w| + |b| < 2^24 (in units of the operands' quantum), so every product and partial sum is exact in fp32 whatever
the accumulation order, split-K or slab reduction; the exact result y is then compared as ``got == y`` (fp32 outputs) or
``got == RNE_bf16(y)`` (bf16 outputs).  Activations whose value is not exact (leaky ReLU, ELU, tanh, sigmoid) are compared to 2 fp32
ulp / 1 bf16 ulp.  Every element outside the region a kernel may write holds ``SENT`` and must keep it; input elements outside the
region it may read hold ``SENT`` too, so an over-read changes a result by at least SENT * |w|.

The reference reads the operands through the descriptor's own strides (``a_sn .. a_sc``, ``a_coff``, ``ldw``, ``c_coff``, ``ldc``,
the scatter strides), so a descriptor recorded from a real run can be replayed on fresh buffers (``ConvCase`` / ``WgradCase``).
"""
import ctypes
from ctypes import byref

import torch

from ipoke_amd import _lib

SENT = 4096.0
EXACT_LIMIT = float(1 << 24)
INEXACT_ACTS = (_lib.ACT_ELU, _lib.ACT_LRELU02, _lib.ACT_TANH, _lib.ACT_SIGMOID)
GEOM = ("NB", "Di", "Hi", "Wi", "Do", "Ho", "Wo", "kd", "kh", "kw", "sd", "sh", "sw", "pd", "ph", "pw", "transposed")
GUARD_ROWS = 256          # output rows past the last one a launch may write: a 128- / 256-row tile that ignores M lands in them


def round_up(v, m):
    return (v + m - 1) // m * m


def e16(dtype):
    return 8 if dtype == _lib.BF16 else 4


def tdtype(dtype):
    return torch.bfloat16 if dtype == _lib.BF16 else torch.float32


def to_bf16_rne(x64):
    """float64 -> the bf16 value round-to-nearest-even gives (via fp32, exact for the integers used here)."""
    return x64.to(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------ geometry
def rows_of(d):
    return d.NB * d.Do * d.Ho * d.Wo


def _decompose(d, m):
    ow = m % d.Wo
    t = m // d.Wo
    oh = t % d.Ho
    t = t // d.Ho
    od = t % d.Do
    n = t // d.Do
    return n, od, oh, ow


def _in_coord(o, k, s, p, extent, transposed):
    """input coordinate of output coordinate o under tap k, and whether it lies on the input (else: zero halo)"""
    if transposed:
        t = o + p - k
        i = torch.div(t, s, rounding_mode="floor")
        ok = (t >= 0) & (t - i * s == 0) & (i < extent)
    else:
        i = o * s - p + k
        ok = (i >= 0) & (i < extent)
    return i, ok


def tap_offsets(d, m):
    """[taps, len(m)] element offsets into A of the first channel each (output row, tap) reads; -1 where the tap falls on the zero halo.
    Taps in (kd, kh, kw) row-major order, as the weight operand's k = tap * Kc + c."""
    n, od, oh, ow = _decompose(d, m)
    offs = []
    for a in range(d.kd):
        idd, okd = _in_coord(od, a, d.sd, d.pd, d.Di, d.transposed)
        for b in range(d.kh):
            ih, okh = _in_coord(oh, b, d.sh, d.ph, d.Hi, d.transposed)
            for c in range(d.kw):
                iw, okw = _in_coord(ow, c, d.sw, d.pw, d.Wi, d.transposed)
                off = d.a_coff + n * d.a_sn + idd * d.a_sd + ih * d.a_sh + iw * d.a_sw
                offs.append(torch.where(okd & okh & okw, off, torch.full_like(off, -1)))
    return torch.stack(offs)


def out_row_index(d, m):
    """row of C that holds output position m (dense, or the c_scatter placement)"""
    if not d.c_scatter:
        return m
    n, od, oh, ow = _decompose(d, m)
    return d.c_row0 + n * d.c_sn + od * d.c_sd + oh * d.c_sh + ow * d.c_sw


def taps_of(d):
    return d.kd * d.kh * d.kw


def a_extent(d):
    """elements of A a launch may read: every input pixel's channel run [a_coff, a_coff + Kc) (padding channels included)"""
    last = d.a_coff + (d.NB - 1) * d.a_sn + (d.Di - 1) * d.a_sd + (d.Hi - 1) * d.a_sh + (d.Wi - 1) * d.a_sw + (d.Kc - 1) * d.a_sc
    return last + 1


# ------------------------------------------------------------------ reference
def gather_rows(d, A, m, dtype64=torch.float64):
    """[len(m), taps * Kc_real] float64: the operand row of the implicit GEMM for output rows m (zeros on the halo)"""
    offs = tap_offsets(d, m)                                         # [taps, R]
    c = torch.arange(d.Kc_real, device=A.device) * d.a_sc
    idx = offs.unsqueeze(-1) + c                                     # [taps, R, Kc_real]
    valid = (offs >= 0).unsqueeze(-1).expand_as(idx)
    vals = A.reshape(-1)[idx.clamp(min=0)].to(dtype64)
    vals = torch.where(valid, vals, torch.zeros((), dtype=dtype64, device=A.device))
    return vals.permute(1, 0, 2).reshape(len(m), -1)


def weight_matrix(d, W):
    """[taps * Kc_real, Nout] float64 weights (the operand's padding channels Kc_real .. Kc dropped)"""
    T = taps_of(d)
    if d.w_kmajor:
        w = W.reshape(-1)[: T * d.Kc * d.ldw].view(T * d.Kc, d.ldw)[:, : d.Nout]
        w = w.reshape(T, d.Kc, d.Nout)[:, : d.Kc_real]
    else:
        w = W.reshape(-1)[: d.Nout * d.ldw].view(d.Nout, d.ldw)[:, : T * d.Kc]
        w = w.reshape(d.Nout, T, d.Kc)[:, :, : d.Kc_real].permute(1, 2, 0)
    return w.to(torch.float64).reshape(T * d.Kc_real, d.Nout)


def conv_sums(d, A, W, absolute=False, chunk_elems=1 << 26):
    """[M, Nout] float64 sum_{tap, c} x * w of every output (|x| * |w| with absolute=True: the exactness bound), chunked over rows"""
    M = rows_of(d)
    w = weight_matrix(d, W)
    if absolute:
        w = w.abs()
    out = torch.empty(M, d.Nout, dtype=torch.float64, device=A.device)
    step = max(64, chunk_elems // max(1, w.shape[0]))
    for r0 in range(0, M, step):
        m = torch.arange(r0, min(M, r0 + step), device=A.device)
        x = gather_rows(d, A, m)
        if absolute:
            x = x.abs()
        out[r0:r0 + len(m)] = x @ w
    return out


def act64(act, v):
    if act == _lib.ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == _lib.ACT_RELU:
        return torch.clamp(v, min=0)
    if act == _lib.ACT_LRELU02:
        return torch.where(v > 0, v, 0.2 * v)
    if act == _lib.ACT_TANH:
        return torch.tanh(v)
    if act == _lib.ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def act_grad_from_out64(act, y):
    if act == _lib.ACT_ELU:
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    if act == _lib.ACT_RELU:
        return (y > 0).to(y.dtype)
    if act == _lib.ACT_LRELU02:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.2))
    if act == _lib.ACT_TANH:
        return 1 - y * y
    if act == _lib.ACT_SIGMOID:
        return y * (1 - y)
    return torch.ones_like(y)


# ------------------------------------------------------------------ operands
def int_operand(shape, lim, gen, zero_frac=0.3):
    """integers in [-lim, lim] with about `zero_frac` of them zero (float64, on the generator's device)"""
    v = torch.randint(-lim, lim + 1, shape, generator=gen, dtype=torch.int64, device=gen.device).to(torch.float64)
    keep = torch.rand(shape, generator=gen, device=gen.device) >= zero_frac
    return v * keep


def frac_operand(shape, gen, zero_frac=0.2, ties=0.1):
    """fp32 values with |x| in [1, 8) or 0 that are NOT bf16 values (the on-load conversion must round them), about `ties` of them
    exactly half-way between two bf16 values (round-half-to-even decides)"""
    dev = gen.device
    mag = 2.0 ** torch.randint(0, 3, shape, generator=gen, device=dev).to(torch.float64)
    x = (1 + torch.rand(shape, generator=gen, dtype=torch.float64, device=dev)) * mag
    x = x.to(torch.float32)
    tie = torch.rand(shape, generator=gen, device=dev) < ties
    lo = x.to(torch.bfloat16).to(torch.float32)
    lo = torch.where(lo > x, lo - lo * 2.0 ** -7, lo)                       # bf16 value below x (1 ulp = 2^-7 relative in [2^e, 2^e+1))
    ulp = 2.0 ** (torch.floor(torch.log2(lo)) - 7)
    x = torch.where(tie, lo + ulp / 2, x)
    sign = torch.where(torch.rand(shape, generator=gen, device=dev) < 0.5, -1.0, 1.0)
    keep = torch.rand(shape, generator=gen, device=dev) >= zero_frac
    return (x * sign * keep).to(torch.float32)


def operand_limit(ktot, budget=float(1 << 22), cap=64):
    """largest integer magnitude L for both operands with ktot * L * L <= budget"""
    L = int((budget / max(1, ktot)) ** 0.5)
    return max(1, min(cap, L))


def assert_exact_bound(bound, quantum=1.0):
    mx = float(bound.max()) if bound.numel() else 0.0
    assert mx < EXACT_LIMIT * quantum, f"operands too large for exact fp32 sums: max sum |x*w| = {mx} (quantum {quantum})"


# ------------------------------------------------------------------ buffers
class ConvCase:
    """A descriptor with fresh sentinel-filled buffers, exact operands and the float64 expectation of every output element."""

    def __init__(self, d, dtype, device, seed=0, has_bias=None, has_row_scale=None, has_dact=None, acc_scratch=None, lim=None, live_c=None,
                 zero_taps=()):
        """live_c: channels >= live_c of A and W are zero (a narrow input padded to a 16-byte chunk, e.g. RGB); zero_taps: taps whose
        weights are zero (the zero row / column of a padded 2 x 2 sub-pixel window)"""
        self.d = d = clone_desc(d)
        self.dtype = dtype
        self.device = device
        gen = torch.Generator(device=device).manual_seed(seed)
        T = taps_of(d)
        ktot = T * d.Kc_real
        esz_t = tdtype(dtype)
        self.has_bias = has_bias if has_bias is not None else bool(d.bias)
        self.has_rs = has_row_scale if has_row_scale is not None else bool(d.row_scale)
        # exactness budget in units of the operands' quantum: fp32 activations converted to bf16 on load are multiples of 2^-7 (|x| < 8);
        # row scales 2^-2 .. 2^1 cost 3 bits; integral biases / old values up to 2^10
        frac = bool(d.a_f32) and dtype == _lib.BF16
        self.quantum = 2.0 ** -7 if frac else 1.0
        budget = float(1 << 22) / (8 if self.has_rs else 1)
        if frac:
            L = lim if lim is not None else max(1, min(64, int(budget * self.quantum / 8 / max(1, ktot))))
        else:
            L = lim if lim is not None else operand_limit(ktot, budget)
        # ---- A: sentinel everywhere, operands on every pixel's channels [0, Kc_real)
        a_n = a_extent(d)
        a_guard = min(max(d.a_sn, 1), 1 << 22) + 4096
        a_t = torch.float32 if d.a_f32 else esz_t
        A = torch.full((a_n + a_guard,), SENT, dtype=a_t, device=device)
        pix = self._pixel_offsets().to(device)
        c = torch.arange(d.Kc_real, device=device) * d.a_sc
        idx = (pix.unsqueeze(1) + c).reshape(-1)
        if frac:
            vals = frac_operand((idx.numel(),), gen).to(torch.float64)
        else:
            vals = int_operand((idx.numel(),), L, gen)
        if live_c is not None:
            vals = vals.view(-1, d.Kc_real)
            vals[:, live_c:] = 0
            vals = vals.reshape(-1)
        A[idx] = vals.to(a_t)
        self.A = A
        del A, idx, vals
        # the values the kernel computes with (bf16 RNE of fp32 activations)
        self.A_eff = (self.A.to(torch.bfloat16) if frac else self.A).to(torch.float64)
        # ---- W: [Nout][ldw] (or K-major [taps*Kc][ldw]) -- zero in the padding channels, as the weight operands of the product
        if d.w_kmajor:
            wshape = (T, d.Kc, d.ldw)
            Wv = torch.zeros(wshape, dtype=torch.float64, device=device)
            Wv[:, : d.Kc_real, : d.Nout] = int_operand((T, d.Kc_real, d.Nout), L, gen)
        else:
            Wv = torch.zeros(d.Nout, d.ldw, dtype=torch.float64, device=device)
            Wv[:, : T * d.Kc] = torch.nn.functional.pad(int_operand((d.Nout, T, d.Kc_real), L, gen),
                                                        (0, d.Kc - d.Kc_real)).reshape(d.Nout, T * d.Kc)
        if live_c is not None:
            if d.w_kmajor:
                Wv[:, live_c:] = 0
            else:
                Wv[:, : T * d.Kc].view(d.Nout, T, d.Kc)[:, :, live_c:] = 0
        for t in zero_taps:
            if d.w_kmajor:
                Wv[t] = 0
            else:
                Wv[:, t * d.Kc:(t + 1) * d.Kc] = 0
        self.W = Wv.reshape(-1).to(esz_t)
        # ---- epilogue operands
        self.bias = None
        if self.has_bias:
            self.bias = int_operand((d.Nout,), 1 << 10, gen, 0.1).to(torch.float32)
        self.row_scale = None
        if self.has_rs:
            nimg = d.NB
            groups = (nimg - 1) // max(1, d.rs_images) + 1
            rs = max(1, d.rs_stride)
            tab = torch.full((groups * rs,), float("nan"), device=device)
            tab[::rs] = 2.0 ** torch.randint(-2, 2, (groups,), generator=gen, device=device).to(torch.float32)
            self.row_scale = tab
        self.dact = None
        if has_dact if has_dact is not None else bool(d.dact):
            M = rows_of(d)
            # saved outputs whose act' is a power of two or 0.75 / 0.4375 for ELU, ReLU, tanh, sigmoid: the mask product stays exact
            saved = torch.tensor([-0.75, -0.5, 0.0, 0.5, 1.0, 2.0], dtype=torch.float64, device=device)
            pick = saved[torch.randint(0, len(saved), (M, d.ld_dact), generator=gen, device=device)]
            self.dact = pick.to(esz_t)
        # ---- C: sentinel (or integral old values with c_accumulate), GUARD_ROWS rows past the last one a launch may write
        self.splitk = max(1, d.splitk)
        M = rows_of(d)
        if self.splitk > 1 and not d.c_accumulate:
            c_rows = self.splitk * M
            self.c_t = torch.float32
        else:
            c_rows = int(out_row_index(d, torch.arange(M)).max()) + 1 if M else 0
            self.c_t = torch.float32 if d.c_f32 else esz_t
        self.c_rows = c_rows
        C0 = torch.full((c_rows + GUARD_ROWS, d.ldc), SENT, dtype=self.c_t, device=device)
        if d.c_accumulate:
            C0[:c_rows] = int_operand((c_rows, d.ldc), 1 << 10, gen, 0.1).to(self.c_t)
        self.C0 = C0
        self.C = C0.clone()
        self.acc_scratch = acc_scratch
        # ---- wire the descriptor to the new buffers
        d.A = self.A.data_ptr(); d.W = self.W.data_ptr(); d.C = self.C.data_ptr()
        d.bias = self.bias.data_ptr() if self.bias is not None else None
        d.row_scale = self.row_scale.data_ptr() if self.row_scale is not None else None
        d.dact = self.dact.data_ptr() if self.dact is not None else None
        if acc_scratch is not None:
            d.acc_scratch = acc_scratch.data_ptr(); d.acc_scratch_bytes = acc_scratch.numel()
        else:
            d.acc_scratch = None; d.acc_scratch_bytes = 0
        self._check_bound(ktot)

    def _pixel_offsets(self):
        d = self.d
        return pixel_offsets(d)

    def _scale_per_row(self, M):
        d = self.d
        img = torch.arange(M, device=self.device) // (d.Do * d.Ho * d.Wo)
        return self.row_scale.to(torch.float64)[(img // max(1, d.rs_images)) * max(1, d.rs_stride)]

    def _check_bound(self, ktot):
        """sum |x * w| <= ktot * max|x| * max|w|: with the scale, bias and old value, below 2^24 units of the smallest quantum"""
        d = self.d
        amax = float(self.A_eff[pixel_offsets(d).to(self.device).view(-1, 1) + torch.arange(d.Kc_real, device=self.device) * d.a_sc].abs().max())
        bound = ktot * amax * float(self.W.to(torch.float64).abs().max())
        q = self.quantum
        if self.row_scale is not None:
            bound *= 2.0
            q *= 0.25
        if self.bias is not None:
            bound += float(self.bias.abs().max())
        if d.c_accumulate:
            bound += float(1 << 10)
        assert_exact_bound(torch.tensor([bound]), q)
        self.max_abs_sum = bound

    def run(self):
        _lib.check(_lib.lib().ipoke_conv_forward(byref(self.d), self.dtype, _lib.current_stream()))
        torch.cuda.synchronize()
        return _lib.lib().ipoke_last_conv_kernel()

    def expected(self):
        """(expected C buffer in float64, mask of elements compared with the activation tolerance instead of exactly)"""
        d = self.d
        M = rows_of(d)
        y = conv_sums(d, self.A_eff, self.W)
        E = self.C0.to(torch.float64)
        tol = torch.zeros(E.shape, dtype=torch.bool, device=self.device)
        cols = d.c_coff + torch.arange(d.Nout, device=self.device) * max(1, d.c_cstride)
        if self.splitk > 1 and not d.c_accumulate:
            # partial slabs: only their sum over z is defined; slab 0 is replaced by the sum in compare()
            self.slab = True
            E[:M, : d.Nout] = y
            return E, tol
        self.slab = False
        v = y
        if self.row_scale is not None:
            v = v * self._scale_per_row(M).view(-1, 1)
        if self.bias is not None:
            v = v + self.bias.to(torch.float64)
        v = act64(d.act, v)
        if self.dact is not None:
            saved = self.dact.to(torch.float64)[:M, : d.Nout]
            v = v * act_grad_from_out64(d.dact_act, saved)
        rows = out_row_index(d, torch.arange(M, device=self.device))
        inexact = d.act in INEXACT_ACTS or (self.dact is not None and d.dact_act == _lib.ACT_LRELU02)
        if d.c_accumulate:
            v = E[rows][:, cols] + v
        E[rows.view(-1, 1), cols.view(1, -1)] = v
        if inexact:
            tol[rows.view(-1, 1), cols.view(1, -1)] = True
        if not d.c_f32 and self.splitk == 1:
            n_pad = min(round_up(d.Nout, e16(self.dtype)), d.ldc - d.c_coff)
            if n_pad > d.Nout:
                E[rows.view(-1, 1), (d.c_coff + torch.arange(d.Nout, n_pad, device=self.device)).view(1, -1)] = 0.0
        return E, tol

    def compare(self, what=""):
        E, tol = self.expected()
        got = self.C
        if self.slab:
            d = self.d
            M = rows_of(d)
            sl = got[: self.splitk * M].to(torch.float64).view(self.splitk, M, d.ldc)
            s = sl[:, :, : d.Nout].sum(0)
            G = torch.full_like(E, 0.0)
            G[:M, : d.Nout] = s
            Ecmp = torch.zeros_like(E)
            Ecmp[:M, : d.Nout] = E[:M, : d.Nout]
            assert_exact(G, Ecmp, None, torch.float32, self.d, f"{what} (split-K slab sum)")
            guard = got[self.splitk * M:].to(torch.float64)
            assert bool((guard == SENT).all()), f"{what}: write past the last split-K slab"
            return
        assert_exact(got, E, tol, self.c_t, self.d, what)


def pixel_offsets(d):
    """element offsets of the first used channel of every input pixel (n, d, h, w)"""
    n = torch.arange(d.NB).view(-1, 1, 1, 1) * d.a_sn
    z = torch.arange(d.Di).view(1, -1, 1, 1) * d.a_sd
    h = torch.arange(d.Hi).view(1, 1, -1, 1) * d.a_sh
    w = torch.arange(d.Wi).view(1, 1, 1, -1) * d.a_sw
    return (d.a_coff + n + z + h + w).reshape(-1)


def clone_desc(d):
    c = type(d)()
    ctypes.memmove(byref(c), byref(d), ctypes.sizeof(d))
    return c


def strip_pointers(d):
    """copy of a descriptor with its pointers cleared and the presence of each optional operand as flags (census record key)"""
    c = clone_desc(d)
    flags = dict(bias=bool(d.bias), row_scale=bool(d.row_scale), dact=bool(d.dact), acc=bool(d.acc_scratch))
    for f in ("A", "W", "C", "bias", "dact", "row_scale", "acc_scratch"):
        setattr(c, f, None)
    c.acc_scratch_bytes = 0
    return c, flags


def desc_key(d, dtype):
    c, flags = strip_pointers(d)
    return (dtype, bytes(memoryview(c).cast("B")), tuple(sorted(flags.items())))


def ulp(v, dt):
    """unit in the last place of |v| in fp32 / bf16 (normal range)"""
    bits = 23 if dt == torch.float32 else 7
    a = v.abs().clamp(min=2.0 ** -100)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - bits)


def describe_position(d, row, col):
    """(n, d, h, w, c) of an output element (dense rows; scattered rows are reported as their row index)"""
    if d is None or getattr(d, "c_scatter", 0):
        return f"row {row}, column {col}"
    M = rows_of(d)
    if row >= M:
        return f"row {row} (>= M = {M}), column {col}"
    n, od, oh, ow = (int(t) for t in _decompose(d, torch.tensor(row)))
    cs = max(1, getattr(d, "c_cstride", 1))
    c = (col - getattr(d, "c_coff", 0))
    return f"(n={n}, d={od}, h={oh}, w={ow}, c={c // cs if c % cs == 0 else f'column {col}'})"


def assert_exact(got, E, tol, out_t, d=None, what=""):
    """got (device tensor of the output dtype) against the float64 expectation E: exact (after rounding E to out_t) where tol is False,
    within 1 bf16 ulp / 2 fp32 ulp where it is True.  Raises AssertionError naming the first mismatching element and the difference."""
    g = got.to(torch.float64)
    e = (E.to(torch.float32).to(torch.bfloat16) if out_t == torch.bfloat16 else E.to(torch.float32)).to(torch.float64)
    bad = g != e
    if tol is not None and bool(tol.any()):
        slack = ulp(E, out_t) * (1 if out_t == torch.bfloat16 else 2)
        near = (g - E).abs() <= slack
        bad = torch.where(tol, ~near, bad)
    bad = bad | torch.isnan(g)
    nbad = int(bad.sum())
    if nbad:
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        row, col = divmod(flat, g.shape[1])
        gv, ev = float(g[row, col]), float(e[row, col])
        raise AssertionError(f"{what}: {nbad} mismatching elements; first at {describe_position(d, row, col)}: got {gv}, expected {ev} "
                             f"(difference {gv - ev})")


# ------------------------------------------------------------------ weight gradient
def wgrad_sums(d, A, dY, chunk_elems=1 << 26):
    """[Nout, taps, Kc_real] float64: sum_m dY[m][y_coff + n] * A[src(m, tap)][c]"""
    M = rows_of(d)
    T = taps_of(d)
    out = torch.zeros(d.Nout, T * d.Kc_real, dtype=torch.float64, device=A.device)
    step = max(64, chunk_elems // max(1, T * d.Kc_real))
    dy = dY.reshape(-1)
    for r0 in range(0, M, step):
        m = torch.arange(r0, min(M, r0 + step), device=A.device)
        x = gather_rows(d, A, m)
        g = dy[(m * d.ldy + d.y_coff).view(-1, 1) + torch.arange(d.Nout, device=A.device)].to(torch.float64)
        out += g.t() @ x
    return out.view(d.Nout, T, d.Kc_real)


class WgradCase:
    """ipoke_wgrad_desc with fresh buffers: A as in ConvCase, dY [M][ldy] with SENT outside [y_coff, y_coff + Nout), dW with SENT around
    the (n, c, tap) positions the launch stores (per slab with split_stride)."""

    def __init__(self, d, dtype, device, seed=0, lim=1, zero_frac=0.5):
        self.d = d = clone_desc(d)
        self.dtype = dtype
        self.device = device
        gen = torch.Generator(device=device).manual_seed(seed)
        t = tdtype(dtype)
        a_n = a_extent(d)
        A = torch.full((a_n + 4096 + min(max(d.a_sn, 1), 1 << 22),), SENT, dtype=torch.float32 if d.a_f32 else t, device=device)
        idx = (pixel_offsets(d).to(device).unsqueeze(1) + torch.arange(d.Kc_real, device=device) * d.a_sc).reshape(-1)
        A[idx] = int_operand((idx.numel(),), lim, gen, zero_frac).to(A.dtype)
        self.A = A
        M = rows_of(d)
        Y = torch.full((M + GUARD_ROWS, d.ldy), SENT, dtype=t, device=device)
        Y[:M, d.y_coff:d.y_coff + d.Nout] = int_operand((M, d.Nout), lim, gen, zero_frac).to(t)
        self.dY = Y
        T = taps_of(d)
        kst = d.Kc_store if d.Kc_store > 0 else d.Kc_real
        self.kst = kst
        self.nsplit = d.splitm if (d.splitm > 1 and d.split_stride > 0) else 1
        last = (d.Nout - 1) * d.w_sn + (kst - 1) * d.w_sc + (T - 1) * d.w_st + 1
        span = (self.nsplit - 1) * d.split_stride + last if self.nsplit > 1 else last
        self.W0 = torch.full((span + 4096,), SENT, dtype=torch.float32, device=device)
        if d.accumulate or (d.splitm > 1 and d.split_stride == 0):
            pos = self._positions(0).to(device)
            self.W0[pos] = int_operand((pos.numel(),), 1 << 10, gen, 0.1).to(torch.float32) if d.accumulate else 0.0
        self.dW = self.W0.clone()
        d.A = self.A.data_ptr(); d.dY = self.dY.data_ptr(); d.dW = self.dW.data_ptr()
        # sum over the rows of |x * dy| <= M * lim^2 (a tap meets each output row at most once)
        assert_exact_bound(torch.tensor([float(M) * lim * lim + (1 << 10)]))

    def _positions(self, z):
        d = self.d
        T = taps_of(d)
        n = torch.arange(d.Nout).view(-1, 1, 1) * d.w_sn
        c = torch.arange(self.kst).view(1, -1, 1) * d.w_sc
        t = torch.arange(T).view(1, 1, -1) * d.w_st
        return (z * d.split_stride + n + c + t).reshape(-1)

    def run(self):
        _lib.check(_lib.lib().ipoke_conv_wgrad(byref(self.d), self.dtype, _lib.current_stream()))
        torch.cuda.synchronize()
        return _lib.lib().ipoke_last_wgrad_kernel()

    def compare(self, what=""):
        d = self.d
        ref = wgrad_sums(d, self.A, self.dY)[:, :, : self.kst]            # [Nout, taps, kst]
        got = self.dW.to(torch.float64)
        W0 = self.W0.to(torch.float64)
        written = torch.zeros(got.shape, dtype=torch.bool, device=self.device)
        for z in range(self.nsplit):
            written[self._positions(z).to(self.device)] = True
        assert bool((got[~written] == W0[~written]).all()), f"{what}: weight-gradient store outside its (n, c, tap) positions"
        pos = self._positions(0).to(self.device)
        s = sum(got[self._positions(z).to(self.device)] for z in range(self.nsplit))
        exp = ref.permute(0, 2, 1).reshape(-1)                            # positions are ordered (n, c, tap)
        if d.accumulate:
            exp = exp + W0[pos]
        bad = s != exp.to(torch.float32).to(torch.float64)
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            nn_, rem = divmod(i, self.kst * taps_of(d))
            c, t = divmod(rem, taps_of(d))
            raise AssertionError(f"{what}: {int(bad.sum())} mismatching weight-gradient elements; first at (n={nn_}, c={c}, tap={t}): "
                                 f"got {float(s[i])}, expected {float(exp[i])} (difference {float(s[i] - exp[i])})")


# ------------------------------------------------------------------ descriptors
def conv_desc(NB, in_dhw, out_dhw, k, s, p, Kc, Nout, dtype, transposed=False, lda=None, a_coff=0, Kc_real=None, ldw=None, ldc=None,
              c_coff=0, c_f32=False, act=_lib.ACT_NONE, bias=False, row_scale=None, dact_act=None, splitk=1, c_acc=False, scatter=None,
              a_f32=False, w_kmajor=False):
    """ipoke_conv_desc of a channels-last convolution (pointers unset: ConvCase allocates the buffers).  lda: activation row pitch
    (default Kc); ldc: output pitch (default round_up(Nout, 16 bytes) for dtype outputs, Nout for fp32); scatter = (c_sn, c_sh, c_sw,
    c_row0) or (c_sn, c_sd, c_sh, c_sw, c_row0); row_scale = (rs_images, rs_stride); dact_act: the saved-output mask's activation.
    a_f32: fp32 activations in NCDHW planes (channel stride = pixels per image)."""
    d = _lib.ConvDesc()
    d.NB = NB
    d.Di, d.Hi, d.Wi = in_dhw
    d.Do, d.Ho, d.Wo = out_dhw
    d.kd, d.kh, d.kw = k
    d.sd, d.sh, d.sw = s
    d.pd, d.ph, d.pw = p
    d.transposed = int(transposed)
    d.Kc = Kc
    d.Kc_real = Kc if Kc_real is None else Kc_real
    D, H, W = in_dhw
    if a_f32:
        d.a_f32 = 1
        S = D * H * W
        d.a_sn, d.a_sc, d.a_sd, d.a_sh, d.a_sw = d.Kc_real * S, S, H * W, W, 1
    else:
        lda = Kc if lda is None else lda
        d.a_sw = lda; d.a_sh = W * lda; d.a_sd = H * W * lda; d.a_sn = D * H * W * lda; d.a_sc = 1
    d.a_coff = a_coff
    T = k[0] * k[1] * k[2]
    if w_kmajor:
        d.w_kmajor = 1
        d.ldw = Nout if ldw is None else ldw
    else:
        d.ldw = T * Kc if ldw is None else ldw
    d.Nout = Nout
    d.act = act
    d.bias = 1 if bias else None            # presence flags: ConvCase puts real buffers there
    d.c_f32 = int(c_f32)
    d.c_accumulate = int(c_acc)
    d.ldc = ldc if ldc is not None else (Nout if c_f32 else round_up(Nout, e16(dtype)))
    d.c_coff = c_coff
    d.c_cstride = 1
    d.splitk = splitk
    if scatter is not None:
        d.c_scatter = 1
        if len(scatter) == 5:
            d.c_sn, d.c_sd, d.c_sh, d.c_sw, d.c_row0 = scatter
        else:
            d.c_sn, d.c_sh, d.c_sw, d.c_row0 = scatter
    if row_scale is not None:
        d.row_scale = 1
        d.rs_images, d.rs_stride = row_scale
    if dact_act is not None:
        d.dact = 1
        d.dact_act = dact_act
        d.ld_dact = round_up(Nout, e16(dtype))
    return d


def wgrad_desc(NB, dhw, k, p, Kc, Nout, dtype, lda=None, ldy=None, y_coff=0, splitm=1, split_stride=0, accumulate=False, a_f32=False,
               out_dhw=None, s=(1, 1, 1), transposed=False):
    """ipoke_wgrad_desc of a channels-last convolution's weight gradient, dW in PyTorch's [out][in][taps] order"""
    d = _lib.WgradDesc()
    d.NB = NB
    d.Di, d.Hi, d.Wi = dhw
    d.Do, d.Ho, d.Wo = out_dhw if out_dhw is not None else dhw
    d.kd, d.kh, d.kw = k
    d.sd, d.sh, d.sw = s
    d.pd, d.ph, d.pw = p
    d.transposed = int(transposed)
    D, H, W = dhw
    lda = Kc if lda is None else lda
    d.a_f32 = int(a_f32)
    d.a_sw = lda; d.a_sh = W * lda; d.a_sd = H * W * lda; d.a_sn = D * H * W * lda; d.a_sc = 1
    d.Kc = d.Kc_real = Kc
    d.ldy = ldy if ldy is not None else round_up(Nout, e16(dtype)) + y_coff
    d.y_coff = y_coff
    d.Nout = Nout
    T = k[0] * k[1] * k[2]
    d.w_sn, d.w_sc, d.w_st = Kc * T, T, 1
    d.accumulate = int(accumulate)
    d.splitm = splitm
    d.split_stride = split_stride
    return d


# ====================================================================== the real-valued family
# The integer family above cannot see arithmetic: operands of at most 7 significant bits, power-of-two row scales, activations at
# integers and saved outputs whose derivative is a power of two make every product, sum and scale exact whatever the kernel rounds on
# the way.  The cases below put real values through the same descriptors (same buffers, sentinels and reference functions):
#
# * operands: A = randn (rounded to bf16 for bf16 launches; full-mantissa fp32 with a_f32 -- the value computed with is then its RNE
#   bf16, A_eff -- and in every f32 launch), W = randn * 1.5 / sqrt(taps * Kc_real) in the launch dtype (zero in the padding channels,
#   beyond live_c and in zero_taps), bias = randn, row scales uniform in [0.3, 3] and never a power of two, old values under
#   c_accumulate 8 * randn, saved outputs over the activation's own range in the storage dtype (both signs and both zeros for ReLU /
#   leaky ReLU), dY = 0.1 * randn in the launch dtype.
# * reference: float64 throughout.  S is the sum of the magnitudes of an output's terms: |s| sum |x||w| + |b| + |c_old| forward,
#   sum_m |dY||A| + |dW_old| for the weight gradient.  The error of a contraction is counted in ulp32(S) and bounded by
#   real_bound(key) = max(4 x yardstick, 4); the yardstick is the worst error of the fp32 restatement ``block_restatement`` (exact dot
#   products over one matrix-core step of the reduction, rounded to fp32 and added in order in fp32) of the case's own reduction on
#   the case's own descriptor and operand rules, measured by test_conv_real_cpu.py (every row where the CPU can afford it, evenly
#   spaced rows otherwise) and recorded per case in REAL_YARDSTICK -- never from a kernel's output.
# * behind the contraction: every activation has slope <= 1, so the pre-activation allowance carries over; the activation's own error
#   is real_bound("act_*") fp32 ulps of its value (yardstick: torch's fp32 expm1 / tanh / sigmoid on the CPU); the derivative mask
#   multiplies the allowance by |act'(saved)| and adds real_bound("dact") ulps of |act| * (magnitude of the terms of act'); a bf16 store
#   adds one bf16 ulp of the expected value.  The bf16-store ELU of a bf16 launch is by contract exp(x) - 1: its allowance is absolute,
#   four times the worst error of fl32(exp32(x)) - 1 on the CPU over the case's own arguments.  Every element is compared.
REAL_YARDSTICK = {
    # worst error of the block restatement of each case's own reduction on its own operands, in ulp32(S), rounded up to a tenth
    # (test_conv_real_cpu.py: measure_conv_case / measure_wgrad_case; a few thousand to 10^6 outputs per case, and the tail is long: the
    # root-mean-square is 0.1).  Forward cases of tests/test_conv_real_gpu.py and, as cpu_*, of test_conv_real_cpu.py:
    "fwd": {
        "s8_k256_n32_b5": 0.6, "s8_k512_n60_b3": 0.7, "s8_k2048_n64_b7": 0.8, "s8_transposed_k512_n64_b5": 0.6,
        "s8_splitk_slabs_k1024_n48_b20": 0.7, "s8_splitk_acc_dgrad_k512_n32_b20": 0.7, "s8_outside_k192": 0.6,
        "s8_outside_n72": 0.7, "k64_k8_n256_b3": 1.2, "k64_k32_n2048_b3": 0.9, "k64_k40_n256_b20": 1.1, "k64_k32_n2048_b20": 1.0,
        "k64_outside_b40_n2048": 1.1, "k64_outside_n248": 0.8, "k8_cin3_n16_m65536": 1.5, "k8_cin8_n48_m65536": 1.4,
        "k8_cin8_n64_m65536_transposed": 1.4, "k8_cin3_n64_transposed": 1.5, "k8_outside_m49152": 1.4, "k8_outside_bias": 1.4,
        "k8_outside_n72": 1.5, "c64_k64_n64_default_rule": 0.8, "c64_outside_k128_9tap": 0.8, "c64_k64_n40_relu_bias": 0.8,
        "c64_transposed_k64_n32": 0.7, "c64_phase00_1tap": 1.0, "c64_phase01_2tap": 0.8, "c64_phase10_2tap": 0.9,
        "c64_phase11_4tap": 1.0, "c64_phase11_4tap_k128_n56": 0.5, "c64_outside_n72": 0.8, "c64_outside_h24": 0.9,
        "halo16_k128_n96": 0.7, "halo16_k128_n128_elu": 0.7, "halo16_k256_n200": 0.8, "halo16_3d_k64_n96": 0.9,
        "halo16_3d_depth_stride2_k64_n128": 0.7, "halo16_phase11_4tap": 0.7, "halo16_phase01_padded_2x2_16": 0.6,
        "halo16_phase10_padded_2x2_16": 0.6, "halo16_phase01_padded_2x2_32": 0.8, "halo16_outside_h24": 1.0,
        "halo16_outside_k96": 0.9, "halo_k64_128x128_n3_f32out_tanh": 0.6, "halo_k64_n64_elu_channel_range": 0.8,
        "halo_k512_16x16_n256": 0.8, "halo_3d_k64_n64": 0.8, "halo_outside_w24": 0.8, "halo_outside_m1024": 0.7,
        "igemm_1x1_k128_n192": 0.7, "igemm_stem_3x7x7_a_f32": 1.0, "igemm_stem_3x7x7_f32": 1.3, "igemm_patchgan_4x4_s2_lrelu": 1.1,
        "igemm_strided_dgrad_dact_elu": 0.8, "igemm_row_scale_bias": 1.0, "igemm_channel_range_k40": 0.7, "igemm_f32_3x3_acc": 0.9,
        "igemm_f32_3x3_bias_elu": 0.9, "igemm_f32_dtype_out_transposed": 0.9, "igemm_f32_8x8_k512_n64": 0.8,
        "igemm_3d_scatter_with_depth": 0.7, "upconv8_phase00_1tap": 0.8, "upconv8_phase01_padded_2x2": 0.9,
        "upconv8_phase10_padded_2x2": 0.7, "upconv8_phase11_4tap": 0.7, "igemm_dgrad_dact_tanh": 0.7,
        "igemm_dgrad_dact_sigmoid": 0.8, "igemm_dgrad_dact_relu": 0.7, "igemm_dgrad_dact_lrelu": 0.7,
        "igemm_sigmoid_bf16_store": 0.6, "igemm_sigmoid_f32_store": 0.8, "igemm_tanh_bf16_store": 0.7, "igemm_tanh_f32_store": 0.7,
        "igemm_elu_bf16_compute_f32_store": 0.9, "halo_outside_elu_f32_store": 0.5, "halo16_outside_elu_f32_store": 1.0,
        "c64_outside_elu_f32_store": 0.8, "halo_small_elu_f32_store": 0.6, "s8_splitk_acc_atomic_k512_n32_b20": 0.5,
        "small_elu_fast_path_bf16_store": 0.8, "small_elu_general_f32_store": 0.6, "small_elu_f32_launch": 1.0, "cpu_f32_k576": 0.6,
        "cpu_f32_elu_k324": 0.7, "cpu_bf16_elu_bf16_store": 0.4, "cpu_bf16_tanh_f32_store": 0.4,
        "cpu_bf16_sigmoid_channel_range": 0.4, "cpu_bf16_row_scale_f32_store": 0.5, "cpu_bf16_a_f32_stem": 0.4, "cpu_f32_acc": 0.3,
        "cpu_bf16_slabs": 0.6, "cpu_bf16_dgrad_dact_tanh": 0.5, "cpu_bf16_dgrad_dact_lrelu": 0.5, "cpu_small_elu_bf16_store": 0.4,
        "cpu_small_elu_f32_store": 0.4, "cpu_small_elu_f32_launch": 0.5,
    },
    # weight gradients (blocks of 32 output rows)
    "wgrad": {
        "wgrad_halo_k64_n128_64x64": 0.6, "wgrad_halo_slabs_k128_n64_32x32": 0.7, "wgrad_halo_3d_k64_n64": 0.7,
        "wgrad_halo_outside_m4096": 0.6, "wgrad_tn_1x1_k128_n256": 0.5, "wgrad_tn_3x3_k48_n40_ragged": 0.6,
        "wgrad_tn_3x3_k24_n32_4x8_map": 0.7, "wgrad_tn_f32_3x3_k36_n20": 0.7, "wgrad_tn_f32_1x1_split_atomic": 0.5,
        "wgrad_stem_3x7x7_a_f32_kc_store": 0.5, "wgrad_tn_3x3_k48_n40_accumulate": 0.6, "batched_b20_k512_n64_3x3": 0.6,
        "batched_b7_k320_n136_3x3": 0.7, "batched_b3_k64_n48_3x3": 0.6, "batched_b20_k512_n48_1x1": 0.4,
        "batched_b5_k256_n256_1x1": 0.5, "cpu_f32": 0.5, "cpu_acc": 0.6, "cpu_slabs": 0.5,
    },
    # torch's fp32 activation on the CPU against float64, in fp32 ulps of the value; the derivative from the saved output
    # (measured 0.52, 0.57, 1.94, 0, 0.6 and 0.5)
    "act_elu": 0.6, "act_tanh": 0.6, "act_sigmoid": 2.0, "act_relu": 0.5, "act_lrelu": 0.7, "dact": 0.5,
}
ACT_KEY = {_lib.ACT_ELU: "act_elu", _lib.ACT_TANH: "act_tanh", _lib.ACT_SIGMOID: "act_sigmoid", _lib.ACT_RELU: "act_relu",
           _lib.ACT_LRELU02: "act_lrelu"}


def dtype_name(dtype):
    return "bf16" if dtype == _lib.BF16 else "f32"


def real_bound(key):
    """key: ("fwd" | "wgrad", case name) or the name of an activation entry"""
    y = REAL_YARDSTICK[key[0]][key[1]] if isinstance(key, tuple) else REAL_YARDSTICK[key]
    return max(4.0 * y, 4.0)


def ulp32(v):
    """fp32 unit in the last place of |v| (float64 tensor); the subnormal spacing below 2^-126"""
    a = v.abs().clamp(min=2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 23)


def block_restatement(x64, w64, block):
    """[R, K] x [K, N] float64 operands: dot products over `block` consecutive elements of K taken exactly and rounded to fp32, the
    blocks added in order in fp32 (one matrix-core step at a time).  Returns float32 [R, N]."""
    R, K = x64.shape
    acc = torch.zeros(R, w64.shape[1], dtype=torch.float32, device=x64.device)
    for k0 in range(0, K, block):
        acc = acc + (x64[:, k0:k0 + block] @ w64[k0:k0 + block]).to(torch.float32)
    return acc


def k_block(dtype):
    """elements of K per matrix-core step: 32 bf16 (v_mfma_f32_16x16x32_bf16) or 16 f32 (four v_mfma_f32_16x16x4_f32)"""
    return 32 if dtype == _lib.BF16 else 16


def not_representable(x, bits):
    """fraction of the non-zero values of x (fp32 / float64 values) whose significand needs more than `bits` bits"""
    v = x.to(torch.float64).reshape(-1)
    v = v[v != 0]
    if v.numel() == 0:
        return 0.0
    q = torch.pow(2.0, torch.floor(torch.log2(v.abs())) - (bits - 1))
    return float((torch.remainder(v, q) != 0).to(torch.float64).mean())


def real_operand(shape, dtype, gen, scale=1.0):
    """scale * randn in the launch dtype, as float64"""
    v = torch.randn(shape, generator=gen, device=gen.device, dtype=torch.float32) * scale
    return v.to(tdtype(dtype)).to(torch.float64)


def act_grad_mag64(act, y):
    """sum of the magnitudes of the terms of act'(y) as the kernel evaluates it from the saved output"""
    if act == _lib.ACT_ELU:
        return torch.where(y > 0, torch.ones_like(y), y.abs() + 1)
    if act == _lib.ACT_TANH:
        return 1 + y * y
    if act == _lib.ACT_SIGMOID:
        return y.abs() * (1 + y.abs())
    return act_grad_from_out64(act, y).abs()


def saved_outputs(act, shape, t, gen):
    """saved activation outputs over the activation's own range, in the storage dtype"""
    dev = gen.device
    u = torch.rand(shape, generator=gen, device=dev, dtype=torch.float32)
    if act == _lib.ACT_ELU:
        v = 4 * u - 1
    elif act == _lib.ACT_TANH:
        v = 2 * u - 1
    elif act == _lib.ACT_SIGMOID:
        v = u
    else:
        v = torch.randn(shape, generator=gen, device=dev, dtype=torch.float32)
        z = torch.rand(shape, generator=gen, device=dev)
        v = torch.where(z < 0.1, torch.zeros_like(v), v)
        v = torch.where(z < 0.05, -torch.zeros_like(v), v)
    return v.to(t)


class RealConvCase(ConvCase):
    """ConvCase with real-valued operands written over the integer ones (same buffers, same pointers, same sentinels), a float64
    expectation with a per-element allowance, and run_twice() for the bit-reproducibility of the launches that take no atomics."""

    def __init__(self, d, dtype, device, key, seed=0, acc_scratch=None, live_c=None, zero_taps=(), w_exp=0, **kw):
        """key: the case's name in REAL_YARDSTICK["fwd"]"""
        super().__init__(d, dtype, device, seed=seed, acc_scratch=acc_scratch, live_c=live_c, zero_taps=zero_taps, **kw)
        d = self.d
        gen = torch.Generator(device=device).manual_seed(seed + 7919)
        T = taps_of(d)
        # ---- A
        idx = (pixel_offsets(d).to(device).unsqueeze(1) + torch.arange(d.Kc_real, device=device) * d.a_sc).reshape(-1)
        full = bool(d.a_f32) or dtype == _lib.F32
        vals = torch.randn(idx.numel(), generator=gen, device=device, dtype=torch.float32)
        if not full:
            vals = vals.to(torch.bfloat16).to(torch.float32)
        if live_c is not None:
            vals = vals.view(-1, d.Kc_real).clone()
            vals[:, live_c:] = 0
            vals = vals.reshape(-1)
        self.A[idx] = vals.to(self.A.dtype)
        self.A_eff = (self.A.to(torch.bfloat16) if (d.a_f32 and dtype == _lib.BF16) else self.A).to(torch.float64)
        # ---- W: real values where the structure (padding channels, live_c, zero_taps) allows a weight
        wscale = 1.5 / (T * d.Kc_real) ** 0.5 * 2.0 ** w_exp
        live = d.Kc_real if live_c is None else live_c
        if d.w_kmajor:
            Wv = torch.zeros(T, d.Kc, d.ldw, dtype=torch.float64, device=device)
            Wv[:, :live, : d.Nout] = real_operand((T, live, d.Nout), dtype, gen, wscale)
            for t in zero_taps:
                Wv[t] = 0
        else:
            Wv = torch.zeros(d.Nout, d.ldw, dtype=torch.float64, device=device)
            w3 = torch.zeros(d.Nout, T, d.Kc, dtype=torch.float64, device=device)
            w3[:, :, :live] = real_operand((d.Nout, T, live), dtype, gen, wscale)
            for t in zero_taps:
                w3[:, t] = 0
            Wv[:, : T * d.Kc] = w3.reshape(d.Nout, T * d.Kc)
        self.W.copy_(Wv.reshape(-1).to(self.W.dtype))
        # ---- epilogue operands
        if self.bias is not None:
            self.bias.copy_(torch.randn(d.Nout, generator=gen, device=device, dtype=torch.float32))
        if self.row_scale is not None:
            rs = max(1, d.rs_stride)
            n = self.row_scale[::rs].numel()
            s = 0.3 + 2.7 * torch.rand(n, generator=gen, device=device, dtype=torch.float32)
            assert not bool((torch.frexp(s)[0] == 0.5).any()), "a row scale is a power of two"
            self.row_scale[::rs] = s
        if self.dact is not None:
            self.dact.copy_(saved_outputs(d.dact_act, tuple(self.dact.shape), self.dact.dtype, gen))
        if d.c_accumulate:
            self.C0[: self.c_rows] = (8 * torch.randn(self.c_rows, d.ldc, generator=gen, device=device, dtype=torch.float32)).to(self.c_t)
        self.C.copy_(self.C0)
        self.fwd_key = ("fwd", key)
        self.atomic = self.splitk > 1 and bool(d.c_accumulate) and acc_scratch is None

    def _check_bound(self, ktot):          # (the integer operands the base class drew are replaced: nothing to hold exact)
        self.max_abs_sum = None

    def elu_fast(self):
        """the bf16-store ELU of a bf16 launch: exp(x) - 1 by contract"""
        return self.dtype == _lib.BF16 and self.d.act == _lib.ACT_ELU and not self.d.c_f32

    def expected_real(self):
        """(E, tol, written): float64 expectation of the whole C buffer, the allowance of every element and the mask of the elements a
        launch writes (everything else must keep its bits).  Split-K slabs: E / tol hold the slab sum in rows [0, M)."""
        d = self.d
        dev = self.device
        M = rows_of(d)
        y = conv_sums(d, self.A_eff, self.W)
        S = conv_sums(d, self.A_eff, self.W, absolute=True)
        B = real_bound(self.fwd_key)
        E = self.C0.to(torch.float64)
        tol = torch.zeros_like(E)
        written = torch.zeros(E.shape, dtype=torch.bool, device=dev)
        if self.splitk > 1 and not d.c_accumulate:
            self.slab = True
            E[:M, : d.Nout] = y
            tol[:M, : d.Nout] = B * ulp32(S)
            return E, tol, written
        self.slab = False
        v = y
        if self.row_scale is not None:
            s = self._scale_per_row(M).view(-1, 1)
            v, S = v * s, S * s.abs()
        if self.bias is not None:
            b = self.bias.to(torch.float64)
            v, S = v + b, S + b.abs()
        rows = out_row_index(d, torch.arange(M, device=dev))
        cols = d.c_coff + torch.arange(d.Nout, device=dev) * max(1, d.c_cstride)
        old = None
        if d.c_accumulate:
            old = E[rows][:, cols]
            S = S + old.abs()
        t = B * ulp32(S)
        self.pre = v
        if d.act != _lib.ACT_NONE:
            a = act64(d.act, v)
            if self.elu_fast():
                neg = v[v <= 0].cpu()
                x32 = neg.to(torch.float32)
                worst = float(((torch.exp(x32) - 1).to(torch.float64) - torch.expm1(x32.to(torch.float64))).abs().max()) if neg.numel() else 0.0
                self.elu_allowance = 4 * worst
                t = t + torch.where(v <= 0, torch.full_like(v, self.elu_allowance), torch.zeros_like(v))
            else:
                t = t + real_bound(ACT_KEY[d.act]) * ulp32(a)
            v = a
        if self.dact is not None:
            saved = self.dact.to(torch.float64)[:M, : d.Nout]
            g = act_grad_from_out64(d.dact_act, saved)
            t = t * g.abs() + real_bound("dact") * ulp32(v.abs() * act_grad_mag64(d.dact_act, saved))
            v = v * g
        if old is not None:
            v = old + v
        if self.c_t == torch.bfloat16:
            t = t + ulp(v, torch.bfloat16)
        E[rows.view(-1, 1), cols.view(1, -1)] = v
        tol[rows.view(-1, 1), cols.view(1, -1)] = t
        written[rows.view(-1, 1), cols.view(1, -1)] = True
        if not d.c_f32 and self.splitk == 1:
            n_pad = min(round_up(d.Nout, e16(self.dtype)), d.ldc - d.c_coff)
            if n_pad > d.Nout:
                pc = (d.c_coff + torch.arange(d.Nout, n_pad, device=dev)).view(1, -1)
                E[rows.view(-1, 1), pc] = 0.0
                written[rows.view(-1, 1), pc] = True
        return E, tol, written

    def compare(self, what="", got=None):
        """got (default: the case's C) against the expectation; returns the worst error in units of the allowance / bound (the worst
        contraction error in ulp32(S) for slabs and launches with no activation), raises naming the first element that misses"""
        E, tol, written = self.expected_real()
        got = self.C if got is None else got
        d = self.d
        g = got.to(torch.float64)
        if self.slab:
            M = rows_of(d)
            sl = g[: self.splitk * M].view(self.splitk, M, d.ldc)
            assert bool((g[self.splitk * M:] == SENT).all()), f"{what}: write past the last split-K slab"
            G = E.clone()
            G[:M, : d.Nout] = sl[:, :, : d.Nout].sum(0)
            g = G
            written[:M, : d.Nout] = True
        keep = (g == self.C0.to(torch.float64)) | written
        if not bool(keep.all()):
            flat = int(torch.nonzero(~keep.reshape(-1))[0])
            row, col = divmod(flat, g.shape[1])
            raise AssertionError(f"{what}: store outside the written region at {describe_position(d, row, col)}: {float(g[row, col])}")
        err = (g - E).abs()
        bad = written & (~(err <= tol))
        rel = torch.where(written & (tol > 0), err / tol.clamp(min=2.0 ** -1000), torch.zeros_like(err))
        self.worst = float(rel.max()) if rel.numel() else 0.0
        if bool(bad.any()):
            flat = int(torch.nonzero(bad.reshape(-1))[0])
            row, col = divmod(flat, g.shape[1])
            raise AssertionError(f"{what}: {int(bad.sum())} elements beyond their allowance (worst {self.worst:.2f} x the allowance); first at "
                                 f"{describe_position(d, row, col)}: got {float(g[row, col])!r}, expected {float(E[row, col])!r}, "
                                 f"allowance {float(tol[row, col]):.3e}")
        return self.worst

    def run_twice(self):
        """two launches on fresh copies of the output; returns (kernel, bit-identical?)"""
        k = self.run()
        first = self.C.clone()
        self.C.copy_(self.C0)
        self.run()
        same = torch.equal(first.view(torch.uint8), self.C.view(torch.uint8))
        return k, same


class RealWgradCase(WgradCase):
    """WgradCase with real operands: A = randn, dY = 0.1 * randn in the launch dtype (fp32 A with a_f32: the value used is its RNE bf16
    in a bf16 launch), real old values under `accumulate`; slabs summed in float64 and compared in ulp32 of sum_m |dY||A| + |dW_old|."""

    def __init__(self, d, dtype, device, key, seed=0):
        """key: the case's name in REAL_YARDSTICK["wgrad"]"""
        super().__init__(d, dtype, device, seed=seed)
        d = self.d
        gen = torch.Generator(device=device).manual_seed(seed + 7919)
        idx = (pixel_offsets(d).to(device).unsqueeze(1) + torch.arange(d.Kc_real, device=device) * d.a_sc).reshape(-1)
        vals = torch.randn(idx.numel(), generator=gen, device=device, dtype=torch.float32)
        self.A[idx] = vals.to(self.A.dtype)
        self.A_eff = (self.A.to(torch.bfloat16) if (d.a_f32 and dtype == _lib.BF16) else self.A).to(torch.float64)
        M = rows_of(d)
        self.dY[:M, d.y_coff:d.y_coff + d.Nout] = (0.1 * torch.randn(M, d.Nout, generator=gen, device=device, dtype=torch.float32)).to(self.dY.dtype)
        if d.accumulate:
            pos = self._positions(0).to(device)
            self.W0[pos] = torch.randn(pos.numel(), generator=gen, device=device, dtype=torch.float32)
        self.dW.copy_(self.W0)
        self.key = ("wgrad", key)
        self.atomic = d.splitm > 1 and d.split_stride == 0

    def compare(self, what="", got=None):
        """returns the worst error in ulp32(S); raises naming the first element beyond real_bound(key)"""
        d = self.d
        dev = self.device
        ref = wgrad_sums(d, self.A_eff, self.dY)[:, :, : self.kst]
        S = wgrad_sums(d, self.A_eff.abs(), self.dY.abs())[:, :, : self.kst]
        g = (self.dW if got is None else got).to(torch.float64)
        W0 = self.W0.to(torch.float64)
        written = torch.zeros(g.shape, dtype=torch.bool, device=dev)
        for z in range(self.nsplit):
            written[self._positions(z).to(dev)] = True
        assert bool((g[~written] == W0[~written]).all()), f"{what}: weight-gradient store outside its (n, c, tap) positions"
        pos = self._positions(0).to(dev)
        s = sum(g[self._positions(z).to(dev)] for z in range(self.nsplit))
        exp = ref.permute(0, 2, 1).reshape(-1)
        S = S.permute(0, 2, 1).reshape(-1)
        if d.accumulate:
            exp = exp + W0[pos]
            S = S + W0[pos].abs()
        e = (s - exp).abs() / ulp32(S)
        B = real_bound(self.key)
        self.worst = float(e.max())
        bad = ~(e <= B)
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            nn_, rem = divmod(i, self.kst * taps_of(d))
            c, t = divmod(rem, taps_of(d))
            raise AssertionError(f"{what}: {int(bad.sum())} weight-gradient elements beyond {B} ulp32(S) (worst {self.worst:.2f}); first at "
                                 f"(n={nn_}, c={c}, tap={t}): got {float(s[i])!r}, expected {float(exp[i])!r}")
        return self.worst

    def run_twice(self):
        k = self.run()
        first = self.dW.clone()
        self.dW.copy_(self.W0)
        self.run()
        return k, torch.equal(first.view(torch.uint8), self.dW.view(torch.uint8))
