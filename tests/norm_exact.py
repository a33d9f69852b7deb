"""Kernel-by-kernel checking of the first stage's normalisation kernels (csrc/norm.hip: ipoke_groupnorm, ipoke_groupnorm_stats; csrc/vae_bwd.hip:
ipoke_groupnorm_bwd) and of the small kernels every first-stage test goes through (ipoke_nchw_to_cl / ipoke_cl_to_nchw, ipoke_bilinear_cl,
ipoke_reparameterize / ipoke_reparam_bwd).  References, operands, case tables and yardsticks; the test functions are in
test_norm_kernels_cpu.py (which pins the harness, the dispatch path of every case, the yardsticks and the input conditions) and
test_norm_kernels_gpu.py (which runs the kernels).

* Guarded buffers (disc_exact.guarded / check_guard): every operand is the first rows of a [rows + GUARD][ld] buffer of SENT; x, y, res and
  the modulation maps get pitches that exceed C and differ from each other (one dense case).  Input padding holds SENT, so a read outside
  the channels shows in a result; outputs, workspaces and next_part must still hold SENT wherever the contract does not let the call write.
* Forward reference: float64 F.group_norm on the values the kernel reads (rounded to the dtype first), then modulation, residual in front
  of or behind the activation and the activation in float64 (``fwd_ref``).  Compared with NO element left out: y, the (mean, rstd) table and
  -- where next_part is written -- its (count, mean, M2) triples against the float64 statistics of the STORED output, count exactly.
* The chunk statistics are (count, mean - pivot, M2): the pivot of a (sample, group) -- one of its values where the data is clearly shifted,
  else 0 -- waits in the mean slot of the following norm's (mean, rstd) table; the GPU file adds it back in float64 before it compares,
  and asserts that a producer writes nothing else beyond its triples.
* Backward reference: float64 autograd through that forward; the saved y handed to the kernel is the float64 forward rounded to the
  dtype, and the reference takes the activation's derivative from that same stored y (from the recomputed pre-activation for
  act_from_pre): teacher forcing, so the ReLU / ELU kinks need no exclusions.
* Operand families.  "centred": 2 randn + 0.7 (mean / std = 0.35, what the older tests draw -- nothing cancels there).  "shifted": per
  (sample, group) mean / std = 8, 64, 512 in turn with both signs, and one group that is exactly constant (variance 0,
  rstd = 1 / sqrt(eps), output = beta and the modulation only).  In bf16 the values are rounded first and the reference sees those.
  "shifted-out": producer -> consumer chains on both producer paths whose residual behind the activation is shifted per (sample, group
  of the next norm), so the chunk statistics, their pivots and the consumer's finalize work on shifted values; the consumer's rstd is
  held to the same tight units there, which also pins what the loose-looking M2 unit of the triples lets through.
* Bounds (the rule of flow_exact.py / mcf_exact.py; no number comes from the kernels).  The yardstick is ``fwd_ref(..., f=F32)``: an fp32
  restatement on the CPU that never runs the code under test -- two-pass statistics, the scale / shift form
  x (rstd gamma) + (beta - mean rstd gamma), the rest in fp32.  Error is counted in fp32 ulps of the sum of the magnitudes of an output's
  terms (``mag``: |x rstd gamma| + |beta| + |mean rstd gamma|, carried through the modulation as mag (1 + |mg|) + |mb|, plus |res|, plus
  exp(pre) + 1 on the negative branch of the ELU); rstd and mean in ulps of the value.  A kernel value may miss float64 by
  max(4 x yardstick, 4) such units; a bf16 store adds one bf16 ulp of the value.  The chunk statistics handed to the next norm: mean in
  ulps of sum |y| / count; M2 in ulps of M2 + 2 count maxdev^2 (maxdev = the chunk's largest |y - mean|): a one-pass statistic relative
  to a pivot taken from the data sums (y - pivot)^2 = M2 + count (pivot - mean)^2 and subtracts the second part again, and no value of
  the chunk is further from the mean than maxdev.  test_norm_kernels_cpu.py measures the yardsticks, holds them against YARDSTICK
  (rounded up, not padded) and caps them at 16 units, so that a weak yardstick cannot loosen a bound.

Recorded yardsticks (units as above; worst over the cases of the family, rounded up) -> GPU bounds max(4 x yardstick, 4):

    quantity   centred f32   centred bf16   shifted f32   shifted bf16
    y          5.2 -> 20.8   4.6 -> 18.4    2.2 -> 8.8    1.2 -> 4.8
    mean       8.7 -> 34.8   2.1 -> 8.4     2.5 -> 10     0.5 -> 4
    rstd       2.7 -> 10.8   2.3 -> 9.2     2.2 -> 8.8    3.9 -> 15.6
    nmean      2.7 -> 10.8   1.4 -> 5.6     -             -
    nm2        0.3 -> 4      0.2 -> 4       -             -

    shifted-out (the hand-over chains whose producer OUTPUT is shifted), f32 / bf16:
    y 2.5 -> 10 / 2.3 -> 9.2   mean 2.2 -> 8.8 / 1.4 -> 5.6   rstd 1.8 -> 7.2 / 2.8 -> 11.2   nmean 2.8 -> 11.2 / 0.5 -> 4   nm2 0.3 -> 4 / 0.3 -> 4

(Measured on one CPU thread.  mean in ulps of the VALUE: the InstanceNorm cases of the centred family hold channels whose mean over 35 or 40
positions of 2 randn + 0.7 comes out near 0, which is what the 8.7 measures; the large cases belong to the centred family.  The worst
kernel figures seen on the MI355X are in DESIGN.md section 2.)
"""
import collections
import ctypes
import zlib

import torch
import torch.nn.functional as F

from ipoke_amd import _lib
from tests.conv_exact import act64, act_grad_from_out64  # noqa: F401  (re-exported for the test files)
from tests.disc_exact import DTYPES, F64, GUARD, SENT, assert_same, check_guard, guarded, randint64, ulp_bf16, ulp_f32, ulp_of  # noqa: F401

F32 = torch.float32
EPS = 1e-5
A0 = 0x10000                  # a 16-byte aligned dummy address for the calls that launch nothing
RATIOS = (8.0, 64.0, 512.0)   # mean / std of the shifted family, per (sample, group) in turn

# worst error of the fp32 restatement against float64 (test_norm_kernels_cpu.py measures and asserts them)
YARDSTICK = {
    "y_centred_f32": 5.2, "y_centred_bf16": 4.6, "y_shifted_f32": 2.2, "y_shifted_bf16": 1.2,
    "mean_centred_f32": 8.7, "mean_centred_bf16": 2.1, "mean_shifted_f32": 2.5, "mean_shifted_bf16": 0.5,
    "rstd_centred_f32": 2.7, "rstd_centred_bf16": 2.3, "rstd_shifted_f32": 2.2, "rstd_shifted_bf16": 3.9,
    "nmean_centred_f32": 2.7, "nmean_centred_bf16": 1.4, "nm2_centred_f32": 0.3, "nm2_centred_bf16": 0.2,
    "y_shifted-out_f32": 2.5, "y_shifted-out_bf16": 2.3, "mean_shifted-out_f32": 2.2, "mean_shifted-out_bf16": 1.4,
    "rstd_shifted-out_f32": 1.8, "rstd_shifted-out_bf16": 2.8, "nmean_shifted-out_f32": 2.8, "nmean_shifted-out_bf16": 0.5,
    "nm2_shifted-out_f32": 0.3, "nm2_shifted-out_bf16": 0.3,
}
YARDSTICK_CAP = 16.0


def gpu_bound(qty, family, dt):
    """units allowed on the device: max(4 x yardstick, 4)"""
    return max(4.0 * YARDSTICK[f"{qty}_{family}_{dt}"], 4.0)


def rnd(v, tdt):
    """v (float64) rounded to the storage type and back"""
    return v.to(tdt).to(F64)


# ------------------------------------------------------------------ forward cases
# mod: 0 no SPADE modulation; -1 one map per sample; k > 0 = mod_samples (k < N: sample n reads the maps of n % k; k >= N: ignored)
# res: None, "pre" (in front of the activation) or "post" (behind it);  next_G > 0: the call also writes next_part;
# producer: this call reads the stored output of that case and takes its statistics from the part_chunks the producer left
NormCase = collections.namedtuple("NormCase", "name N S C G affine act res mod y_f32 next_G producer family dense big")


def _c(name, N, S, C, G, affine, act, res=None, mod=0, y_f32=False, next_G=0, producer=None, family="centred", dense=False, big=False):
    return NormCase(name, N, S, C, G, affine, act, res, mod, y_f32, next_G, producer, family, dense, big)


_A = _lib
FWD_CASES = [
    # ---- the one-launch kernel
    _c("cpg4-dense", 2, 35, 32, 8, True, _A.ACT_RELU, "pre", dense=True),        # several groups per slab, ragged 5 x 7, the one dense case
    _c("cpg3", 2, 19, 48, 16, True, _A.ACT_ELU),                                 # slab = lcm(3, 16 bytes)
    _c("instance", 3, 35, 32, 32, False, _A.ACT_LRELU02),                        # G = C, no affine
    _c("tails-one", 2, 51, 128, 16, True, _A.ACT_RELU, "pre"),                   # S = 51: rows rr, rr + 32 (rr < 19) of pass 1's four-row trips
    _c("post-one", 2, 35, 32, 8, True, _A.ACT_ELU, "post"),                      # the residual behind the activation
    _c("producer-pass", 2, 300, 32, 8, True, _A.ACT_ELU, "post", next_G=32),     # next_part by a separate pass over y: chunks of 256 + 44
    # ---- statistics -> finalize -> apply, forced at small S by SPADE modulation or an fp32 output
    _c("tails-three", 2, 51, 128, 16, True, _A.ACT_NONE, mod=-1),                # rp = 8 (f32) / 16 (bf16): four-, two- and one-row trips
    _c("chunks300-f32out", 2, 300, 16, 4, True, _A.ACT_NONE, y_f32=True),        # two chunks of 128 and a tail of 44
    _c("spade-shared", 4, 40, 32, 32, False, _A.ACT_NONE, mod=2),                # S < 128; shared maps; G = C = 32 > 16: finalize's second grid row
    _c("spade-ignored", 2, 130, 32, 32, False, _A.ACT_ELU, "pre", mod=5),        # mod_samples >= N is ignored; a chunk of 2 rows
    _c("post-three", 2, 140, 16, 16, False, _A.ACT_RELU, "post", y_f32=True),    # no affine, res_post, three passes
    _c("c1280", 1, 3, 1280, 16, True, _A.ACT_RELU, "pre", mod=-1),               # fp32: 320 column groups, two channel passes of 256 + 64
    _c("producer-apply", 2, 1100, 128, 2, True, _A.ACT_ELU, "post", next_G=128), # slabs of 64 channels x 1100 rows exceed 128 KB: next_part from the apply pass
    _c("consumer", 2, 1100, 128, 128, False, _A.ACT_NONE, mod=-1, producer="producer-apply"),
    _c("consumer-of-pass", 2, 300, 32, 32, False, _A.ACT_LRELU02, mod=1, producer="producer-pass"),
    _c("consumer-next", 2, 1100, 128, 128, False, _A.ACT_RELU, mod=-1, next_G=16, producer="producer-apply"),
    # ---- the shifted family on both sides
    _c("shifted-one", 2, 35, 32, 8, True, _A.ACT_RELU, "pre", family="shifted"),
    _c("shifted-instance-one", 3, 35, 32, 32, False, _A.ACT_NONE, family="shifted"),
    _c("shifted-three", 2, 51, 128, 16, True, _A.ACT_NONE, mod=-1, family="shifted"),
    _c("shifted-chunks300", 2, 300, 16, 8, True, _A.ACT_ELU, y_f32=True, family="shifted"),
    _c("shifted-instance-three", 4, 300, 32, 32, False, _A.ACT_NONE, mod=2, family="shifted"),
    # ---- the hand-over on shifted data ("shifted-out"): the residual behind the activation carries mean / std = 8, 64, 512 per (sample,
    # group of the NEXT norm), so the producer's chunk statistics, their pivots and the consumer's finalize see shifted values
    _c("shifted-producer-pass", 2, 300, 32, 8, True, _A.ACT_ELU, "post", next_G=32, family="shifted-out"),
    _c("shifted-producer-apply", 2, 1100, 128, 2, True, _A.ACT_ELU, "post", next_G=128, family="shifted-out"),
    _c("shifted-consumer-of-pass", 2, 300, 32, 32, False, _A.ACT_NONE, mod=1, producer="shifted-producer-pass", family="shifted-out"),
    _c("shifted-consumer", 2, 1100, 128, 128, False, _A.ACT_NONE, mod=-1, producer="shifted-producer-apply", family="shifted-out"),
]
# exactly 32 MiB in bf16 (bf16 only), operands and reference built on the device.  The large rule keeps the first on the one-launch kernel:
# groups of 64 channels = 128-byte rows, 32 KB tiles.  (A slab grows by whole groups only while the next width still divides C, so
# with a power-of-two C it stops at 2 x 16 bytes: no InstanceNorm reaches 128-byte rows.)  The same rule sends the second, the
# InstanceNorm of the same size, to the three passes -- below 32 MiB its 8 KB tiles would take the one-launch kernel.
BIG_CASES = [
    _c("large-one", 64, 256, 1024, 16, True, _A.ACT_NONE, big=True),
    _c("large-three", 64, 256, 1024, 1024, False, _A.ACT_NONE, big=True),
]
CASE = {c.name: c for c in FWD_CASES + BIG_CASES}

ONE, LARGE, PART, NEXT_APPLY, NEXT_PASS = (_A.NORM_PATH_ONE_LAUNCH, _A.NORM_PATH_LARGE, _A.NORM_PATH_PART, _A.NORM_PATH_NEXT_APPLY,
                                           _A.NORM_PATH_NEXT_PASS)
# the path every case is there to reach (both dtypes)
EXPECT_PATH = {
    "cpg4-dense": ONE, "cpg3": ONE, "instance": ONE, "tails-one": ONE, "post-one": ONE, "producer-pass": ONE | NEXT_PASS,
    "tails-three": 0, "chunks300-f32out": 0, "spade-shared": 0, "spade-ignored": 0, "post-three": 0, "c1280": 0,
    "producer-apply": NEXT_APPLY, "consumer": PART, "consumer-of-pass": PART, "consumer-next": PART | NEXT_APPLY,
    "shifted-producer-pass": ONE | NEXT_PASS, "shifted-producer-apply": NEXT_APPLY, "shifted-consumer-of-pass": PART, "shifted-consumer": PART,
    "shifted-one": ONE, "shifted-instance-one": ONE, "shifted-three": 0, "shifted-chunks300": 0, "shifted-instance-three": 0,
    "large-one": ONE | LARGE, "large-three": LARGE,
}


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def pitches(c, dt):
    """ldx, ldy, ld_res, ld_mod: all above C and different, except in the dense case (an fp32 output takes any pitch: an odd one)"""
    e = DTYPES[dt][2]
    if c.dense:
        return c.C, c.C, c.C, c.C
    return c.C + e, (c.C + 3 if c.y_f32 else c.C + 2 * e), c.C + 3 * e, c.C + 4 * e


def mod_rows(c):
    """samples the modulation maps hold"""
    return c.mod if 0 < c.mod < c.N else c.N


def next_chunks(c):
    return (c.S + 255) // 256


def make_desc(c, dt, x=A0, y=A0, gamma=A0, beta=A0, mg=A0, mb=A0, res=A0, ws=A0, next_part=A0):
    """the ipoke_norm_desc of a case (dummy addresses serve the calls that launch nothing)"""
    ldx, ldy, ldr, ldm = pitches(c, dt)
    d = _lib.NormDesc()
    d.x, d.ldx, d.y, d.ldy, d.y_f32 = x, ldx, y, ldy, int(c.y_f32)
    d.N, d.S, d.C, d.G, d.eps = c.N, c.S, c.C, c.G, EPS
    d.gamma, d.beta = (gamma, beta) if c.affine else (None, None)
    d.mod_gamma, d.mod_beta, d.ld_mod = (mg, mb, ldm) if c.mod else (None, None, 0)
    d.res, d.ld_res = (res, ldr) if c.res else (None, 0)
    d.act, d.workspace, d.mod_samples = c.act, ws, max(c.mod, 0)
    d.res_post = int(c.res == "post")
    d.next_part, d.next_G = (next_part, c.next_G) if c.next_G else (None, 0)
    d.part_chunks = next_chunks(c) if c.producer else 0
    return d


def path_of(c, dt):
    """(IPOKE_NORM_PATH_* bits, slab width) the library reports for the case"""
    p = _lib.lib().ipoke_groupnorm_path(ctypes.byref(make_desc(c, dt)), DTYPES[dt][0])
    assert p >= 0, (c.name, dt, p)
    return p & ((1 << _lib.NORM_PATH_CS_SHIFT) - 1), p >> _lib.NORM_PATH_CS_SHIFT


# ------------------------------------------------------------------ operands
def shifted_plan(c):
    """[N][G] (mean / std, sign) of the shifted family; the LAST group of sample 0 is the constant one (ratio 0)"""
    k = torch.arange(c.N * c.G).view(c.N, c.G)
    ratio = torch.tensor(RATIOS, dtype=F64)[k % 3]
    sign = torch.where((k // 3) % 2 == 0, 1.0, -1.0).to(F64)
    ratio[0, c.G - 1] = 0.0
    return ratio, sign


def draw_x(c, tdt, gen, device="cpu"):
    z = torch.randn((c.N, c.S, c.C), generator=gen, dtype=F64, device=device)
    if c.family != "shifted":
        return rnd(2.0 * z + 0.7, tdt)
    ratio, sign = (t.to(device) for t in shifted_plan(c))
    cpg = c.C // c.G
    x = z.view(c.N, c.S, c.G, cpg) + (ratio * sign).view(c.N, 1, c.G, 1)
    x[0, :, c.G - 1, :] = 3.0                                 # the constant group (exact in bf16)
    return rnd(x.reshape(c.N, c.S, c.C), tdt)


def fwd_inputs(c, dt, x=None, device="cpu"):
    """the operands of a forward case as the kernel reads them (rounded to the dtype, then float64): dict of x [N][S][C], gamma / beta [C]
    (fp32 values) or None, mg / mb [mod_rows][S][C] or None, res [N][S][C] or None.  x: the stored output of the producer for a consumer"""
    tdt = DTYPES[dt][1]
    gen = torch.Generator(device=device).manual_seed(seed_of(c.name))

    def r(shape, scale=1.0, offset=0.0):
        return rnd(torch.randn(shape, generator=gen, dtype=F64, device=device) * scale + offset, tdt)

    o = dict(x=draw_x(c, tdt, gen, device) if x is None else x.to(F64))
    o["gamma"] = rnd(1.0 + 0.3 * torch.randn(c.C, generator=gen, dtype=F64, device=device), F32) if c.affine else None
    o["beta"] = rnd(0.2 * torch.randn(c.C, generator=gen, dtype=F64, device=device), F32) if c.affine else None
    o["mg"] = r((mod_rows(c), c.S, c.C), 0.5) if c.mod else None
    o["mb"] = r((mod_rows(c), c.S, c.C), 0.5) if c.mod else None
    o["res"] = r((c.N, c.S, c.C), 0.7, 1.0) if c.res else None     # offset 1: no channel of a producer's output has a mean near 0
    if c.family == "shifted-out" and c.res and c.next_G:           # a producer whose OUTPUT is shifted per (sample, group of the next norm)
        ratio, sign = (t.to(device) for t in shifted_plan(c._replace(G=c.next_G)))
        z = 0.7 * torch.randn((c.N, c.S, c.C), generator=gen, dtype=F64, device=device)
        o["res"] = rnd((z.view(c.N, c.S, c.next_G, -1) + (ratio * sign).view(c.N, 1, c.next_G, 1)).reshape(c.N, c.S, c.C), tdt)
    return o


# ------------------------------------------------------------------ forward reference and restatement
def group_stats(x, G, f, eps=EPS):
    """two-pass (mean, rstd) [N][G] in dtype f: the mean first, then the mean of the squared deviations"""
    N, S, C = x.shape
    xg = x.to(f).view(N, S, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1)        # a group's values side by side: torch's cascade sum
    mean = xg.mean(dim=-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=-1)
    return mean.view(N, G), torch.rsqrt(var + eps)


def _per_channel(t, c):
    return t.repeat_interleave(c.C // c.G, dim=1).view(c.N, 1, c.C)


def fwd_ref(c, o, f=F64, restated=None):
    """f = float64: the reference (F.group_norm, then the epilogue in float64) with the magnitude of every output's terms.
    f = float32: the restatement that is the yardstick (two-pass statistics, scale / shift form, the rest in fp32);
    restated=True with float64 evaluates the restatement's formulas in double (the check that they state the same function).
    Returns dict(y, mean, rstd, mag) -- y [N][S][C], mean / rstd [N][G]."""
    x = o["x"].to(f)
    dev = x.device
    mean, rstd = group_stats(x, c.G, f)
    gam = (o["gamma"] if c.affine else torch.ones(c.C, dtype=F64, device=dev)).to(f)
    bet = (o["beta"] if c.affine else torch.zeros(c.C, dtype=F64, device=dev)).to(f)
    sc = _per_channel(rstd, c) * gam
    msc = _per_channel(mean, c) * sc
    if not (f != F64 if restated is None else restated):
        pre = F.group_norm(x.permute(0, 2, 1), c.G, gam if c.affine else None, bet if c.affine else None, EPS).permute(0, 2, 1)
    else:
        pre = x * sc + (bet - msc)
    mag = (x * sc).abs() + bet.abs() + msc.abs()
    if c.mod:
        sel = torch.arange(c.N, device=dev) % mod_rows(c)
        mg, mb = o["mg"].to(f)[sel], o["mb"].to(f)[sel]
        pre = pre * (1.0 + mg) + mb
        mag = mag * (1.0 + mg.abs()) + mb.abs()
    res = o["res"].to(f) if c.res else None
    if c.res == "pre":
        pre, mag = pre + res, mag + res.abs()
    y = act64(c.act, pre)
    if c.act == _lib.ACT_ELU:
        mag = mag + torch.where(pre < 0, torch.exp(pre) + 1.0, torch.zeros_like(pre))
    if c.res == "post":
        y, mag = y + res, mag + res.abs()
    return dict(y=y, mean=mean, rstd=rstd, mag=mag)


def chunk_stats_ref(y, c, f=F64):
    """(count, mean, M2) [N][chunks of 256][next_G] of a stored output y [N][S][C] in dtype f (two-pass), with the magnitudes the two
    are compared in: sum |y| / count for the mean, M2 + 2 count maxdev^2 for M2"""
    nG, cpg = c.next_G, c.C // c.next_G
    out = []
    for k in range(next_chunks(c)):
        blk = y[:, k * 256:(k + 1) * 256].to(f)
        rows = blk.shape[1]
        g = blk.reshape(c.N, rows, nG, cpg).permute(0, 2, 1, 3).reshape(c.N, nG, -1)
        mean = g.mean(dim=-1, keepdim=True)
        dev = g - mean
        cnt = torch.full((c.N, nG), float(rows * cpg), dtype=f, device=y.device)
        m2 = (dev * dev).sum(dim=-1)
        out.append(dict(cnt=cnt, mean=mean.view(c.N, nG), m2=m2, mean_mag=g.abs().mean(dim=-1),
                        m2_mag=m2 + 2.0 * cnt * dev.abs().amax(dim=-1) ** 2))
    return {k: torch.stack([b[k] for b in out], dim=1) for k in out[0]}


# ------------------------------------------------------------------ error in units
def units(got, ref, mag, store_dt=None):
    """|got - ref| in fp32 ulps of mag, element by element; a bf16 store is allowed one bf16 ulp of the value first"""
    err = (got.to(F64) - ref).abs()
    if store_dt == torch.bfloat16:
        err = (err - ulp_bf16(ref)).clamp(min=0)
    return err / ulp_f32(mag)


def worst(got, ref, mag, store_dt=None):
    return float(units(got, ref, mag, store_dt).max())


def assert_units(what, got, ref, mag, bound, store_dt=None):
    """every element within `bound` units; names the first one that misses.  Returns the worst figure."""
    u = units(got, ref, mag, store_dt)
    bad = ~(u <= bound)                                      # a NaN misses
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond {bound} units (worst {float(u.max()):.2f}); first at flat "
                             f"index {i}: got {float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}, "
                             f"magnitude {float(mag.reshape(-1)[i])!r}")
    return float(u.max())


def measure_forward(c, dt, o=None):
    """the yardstick of one case: worst error of the restatement against float64, per quantity"""
    tdt = DTYPES[dt][1]
    o = o or fwd_inputs(c, dt)
    ref, f32 = fwd_ref(c, o), fwd_ref(c, o, F32)
    out = dict(y=worst(f32["y"], ref["y"], ref["mag"]), mean=worst(f32["mean"], ref["mean"], ref["mean"]),
               rstd=worst(f32["rstd"], ref["rstd"], ref["rstd"]))
    if c.next_G:
        stored = ref["y"] if c.y_f32 else rnd(ref["y"], tdt)
        r64, r32 = chunk_stats_ref(stored, c), chunk_stats_ref(stored, c, F32)
        out["nmean"] = worst(r32["mean"], r64["mean"], r64["mean_mag"])
        out["nm2"] = worst(r32["m2"], r64["m2"], r64["m2_mag"])
    return out


def cpu_inputs(c, dt):
    """operands of a case on the CPU; a consumer reads the float64 forward of its producer, rounded as stored"""
    if c.producer:
        p = CASE[c.producer]
        return fwd_inputs(c, dt, x=rnd(fwd_ref(p, cpu_inputs(p, dt))["y"], DTYPES[dt][1]))
    return fwd_inputs(c, dt)


# ------------------------------------------------------------------ layout converters: index formulas
def nchw_to_cl_ref(x, ld):
    """x [N][C][S] -> [N * S][ld]: element (n, c, s) at row n S + s, column c; columns [C, ld) zero"""
    N, C, S = x.shape
    out = torch.zeros((N * S, ld), dtype=x.dtype, device=x.device)
    for n in range(N):
        for c in range(C):
            out[n * S:(n + 1) * S, c] = x[n, c]
    return out


def cl_to_nchw_ref(x, N, C, S):
    """x [N * S][>= C] -> [N][C][S]"""
    out = torch.zeros((N, C, S), dtype=x.dtype, device=x.device)
    for n in range(N):
        for c in range(C):
            out[n, c] = x[n * S:(n + 1) * S, c]
    return out


# ------------------------------------------------------------------ reparameterisation operands
def reparam_data(M, Z, exact, tdt, seed):
    """mu, logvar (values of the dtype), eps, dz, dmu, dlv (fp32 values) as float64; exact: integers with logvar = 0"""
    gen = torch.Generator().manual_seed(seed)
    if exact:
        mu, lv = randint64(-20, 20, (M, Z), gen), torch.zeros((M, Z), dtype=F64)
        eps, dz, dmu, dlv = (randint64(-8, 8, (M, Z), gen) for _ in range(4))
        return mu, lv, eps, 2.0 * dz, dmu, dlv               # dz eps / 2 stays an integer
    r = lambda s: torch.randn((M, Z), generator=gen, dtype=F64) * s      # noqa: E731
    mu, lv = rnd(r(1.0), tdt), rnd(r(1.5) - 1.0, tdt)
    eps, dz, dmu, dlv = (rnd(r(1.0), F32) for _ in range(4))
    return mu, lv, eps, dz, dmu, dlv


# ------------------------------------------------------------------ backward cases
# saved: the (mean, rstd) table of the forward pass is handed over (else stats = NULL: recomputed from x); from_pre: act_from_pre (the forward
# was act(pre) + res, act' from the recomputed pre-activation, no dres).  dy holds integers in [-4, 4] in every case, so that with ReLU or no
# activation dres / dmod_beta (= dy act'(y)) and the sums of dbeta are exact in both dtypes.
# summed: dmod_summed (gn_bwd_apply_frames_kernel) -- dmod_gamma / dmod_beta hold mod rows, the sum over the frames that share a map;
# rs = (clips, stride of rs_scale, rs_bias?, rs_dbias?): the row-scale fold -- samples ordered (frame, clip), frame of sample n = n // clips
BwdCase = collections.namedtuple("BwdCase", "name N S C G affine act res mod saved from_pre summed rs", defaults=(False, None))
BWD_CASES = [
    BwdCase("plain-saved", 2, 51, 32, 8, True, _A.ACT_RELU, True, 0, True, False),          # ragged S, rows past the chunk in the last lanes
    BwdCase("plain-recomputed", 2, 300, 16, 4, True, _A.ACT_ELU, False, 0, False, False),   # three chunks of 128; stats = NULL
    BwdCase("instance-none", 3, 35, 32, 32, False, _A.ACT_NONE, True, 0, True, False),
    BwdCase("spade-shared", 4, 40, 32, 32, False, _A.ACT_NONE, False, 2, True, False),      # mod_samples < N, gradients per sample
    BwdCase("spade-affine", 2, 130, 16, 4, True, _A.ACT_RELU, True, -1, False, False),
    BwdCase("from-pre", 2, 140, 16, 16, True, _A.ACT_ELU, False, 0, True, True),
    BwdCase("c1280", 1, 3, 1280, 16, True, _A.ACT_RELU, True, 0, True, False),              # fp32: two channel passes in both kernels
    # blocks of 128 positions (C = 32): S = 130 gives a second block with 2 live rows, S = 40 one block whose last 88 rows are past S
    BwdCase("summed", 4, 130, 32, 32, False, _A.ACT_RELU, True, 2, True, False, True),
    BwdCase("summed-short", 6, 40, 32, 8, True, _A.ACT_NONE, False, 2, False, False, True),
    # blocks of 512 positions: S = 600 gives two per sample
    BwdCase("fold", 4, 600, 16, 4, True, _A.ACT_RELU, True, 0, True, False, False, (2, 1, True, True)),       # two clips per frame
    BwdCase("fold-stride", 3, 35, 32, 8, True, _A.ACT_NONE, False, 0, False, False, False, (1, 3, False, False)),   # no bias, no dbias, stride 3
    BwdCase("fold-from-pre", 4, 51, 32, 32, False, _A.ACT_ELU, False, 0, True, True, False, (2, 2, True, False)),
]
BWD = {c.name: c for c in BWD_CASES}
BWD_QTY = ("dx", "dres", "dmg", "dmb", "dgamma", "dbeta")
RS_SCALES = (0.75, 1.5, 0.625, 1.25)          # 1 / sigma_t of the frames (a bf16 dx is rounded, scaled and rounded again: two bf16 ulps)
# worst error of the fp32 restatement of the closed forms (comments of csrc/vae_bwd.hip) against float64 autograd, in fp32 ulps of the sum of
# the terms' magnitudes (test_norm_kernels_cpu.py measures and asserts them); bound on the device max(4 x yardstick, 4)
BWD_YARDSTICK = {
    "dx_f32": 2.0, "dx_bf16": 2.2, "dres_f32": 0.0, "dres_bf16": 0.0, "dmg_f32": 2.1, "dmg_bf16": 2.2, "dmb_f32": 0.0, "dmb_bf16": 0.0,
    "dgamma_f32": 1.3, "dgamma_bf16": 1.6, "dbeta_f32": 0.5, "dbeta_bf16": 0.4,
}


def bwd_bound(qty, dt):
    return max(4.0 * BWD_YARDSTICK[f"{qty}_{dt}"], 4.0)


def bwd_pitches(c, dt):
    """ldx, ldy, lddy, lddx, lddres, ld_mod, ld_dmod: all above C and different"""
    e = DTYPES[dt][2]
    return tuple(c.C + k * e for k in range(1, 8))


def bwd_inputs(c, dt):
    """operands of a backward case as the kernel reads them (float64 of the rounded values; CPU): x, dy (integers), gamma / beta, mg (one map
    per modulation sample), res-free; y = the float64 forward rounded to the dtype (the saved output), stats = its (mean, rstd) in fp32"""
    tdt = DTYPES[dt][1]
    gen = torch.Generator().manual_seed(seed_of("bwd-" + c.name))
    shape = (c.N, c.S, c.C)
    o = dict(x=rnd(2.0 * torch.randn(shape, generator=gen, dtype=F64) + 0.7, tdt), dy=randint64(-4, 4, shape, gen))
    o["gamma"] = rnd(1.0 + 0.3 * torch.randn(c.C, generator=gen, dtype=F64), F32) if c.affine else None
    o["beta"] = rnd(0.2 * torch.randn(c.C, generator=gen, dtype=F64), F32) if c.affine else None
    rows = c.mod if 0 < c.mod < c.N else c.N
    o["mg"] = rnd(0.5 * torch.randn((rows, c.S, c.C), generator=gen, dtype=F64), tdt) if c.mod else None
    o["mb"] = rnd(0.5 * torch.randn((rows, c.S, c.C), generator=gen, dtype=F64), tdt) if c.mod else None
    o["res"] = rnd(0.7 * torch.randn(shape, generator=gen, dtype=F64), tdt) if (c.res or c.from_pre) else None
    o["rs_bias"] = rnd(0.5 * torch.randn(c.C, generator=gen, dtype=F64), F32) if c.rs else None
    fc = _c(c.name, c.N, c.S, c.C, c.G, c.affine, c.act, "post" if c.from_pre else ("pre" if c.res else None), c.mod)
    f = fwd_ref(fc, o)
    o["y"], o["stats"] = rnd(f["y"], tdt), torch.stack([rnd(f["mean"], F32), rnd(f["rstd"], F32)], dim=-1)
    return o


def _act_grad_pre64(act, pre):
    return act_grad_from_out64(act, act64(act, pre))


def bwd_ref(c, o):
    """float64 autograd through the float64 forward; the activation's derivative from the STORED y (from the float64 pre-activation for
    from_pre).  dict of dx, dres, dmg, dmb [N][S][C] (per sample), dgamma, dbeta [C]; None where the case has none"""
    x = o["x"].clone().requires_grad_(True)
    gam = o["gamma"].clone().requires_grad_(True) if c.affine else None
    bet = o["beta"].clone().requires_grad_(True) if c.affine else None
    pre = F.group_norm(x.permute(0, 2, 1), c.G, gam, bet, EPS).permute(0, 2, 1)
    mg = mb = None
    if c.mod:
        sel = torch.arange(c.N) % o["mg"].shape[0]
        mg, mb = o["mg"][sel].clone().requires_grad_(True), o["mb"][sel].clone().requires_grad_(True)
        pre = pre * (1.0 + mg) + mb
    dw = o["dy"] * (_act_grad_pre64(c.act, pre.detach()) if c.from_pre else act_grad_from_out64(c.act, o["y"]) if c.act != _lib.ACT_NONE
                    else torch.ones_like(o["dy"]))
    pre.backward(dw)
    out = dict(dx=x.grad, dres=dw if c.res else None, dmg=mg.grad if c.mod else None, dmb=mb.grad if c.mod else None,
               dgamma=gam.grad if c.affine else None, dbeta=bet.grad if c.affine else None)
    return frames_summed(c, out)


def frames_summed(c, out):
    """dmod_summed: the per-sample modulation gradients (or their magnitudes) summed over the frames n = t * mod + clip of a clip"""
    if c.summed:
        for k in ("dmg", "dmb"):
            out[k] = out[k].view(c.N // c.mod, c.mod, c.S, c.C).sum(dim=0)
    return out


def fold_ref(c, o, dx, scales=None):
    """the row-scale fold on a float64 dx [N][S][C]: (dx / sigma_t per frame, rs_dots [frames] = sum dx (x - b), rs_dbias [C] = sum dx)
    and the magnitudes of the two sums' terms.  scales: the frames' 1 / sigma_t where they are not RS_SCALES (tests/ops_exact.py)"""
    clips, stride, with_bias, _ = c.rs
    frames = c.N // clips
    sc = torch.tensor(RS_SCALES[:frames] if scales is None else list(scales), dtype=F64).repeat_interleave(clips).view(c.N, 1, 1)
    xb = o["x"] - (o["rs_bias"] if with_bias else 0.0)
    xm = o["x"].abs() + (o["rs_bias"].abs() if with_bias else 0.0)
    per = lambda t: t.view(frames, clips * c.S * c.C).sum(dim=1)      # noqa: E731
    return dict(dx=dx * sc, dots=per(dx * xb), dbias=dx.sum(dim=(0, 1)), sc=sc, dots_mag=per(dx.abs() * xm), dbias_mag=dx.abs().sum(dim=(0, 1)),
                xm=xm)


def bwd_restated(c, o, f=F32):
    """the closed forms of csrc/vae_bwd.hip in dtype f with two-pass statistics, and the magnitude of every output's terms:
    dw = dy act'(y), du = dw (1 + mg), xh = (x - mean) rstd, S1 = sum_group gamma du, S2 = sum_group gamma du xh,
    dx = rstd (du gamma - (S1 + xh S2) / count), dmod_gamma = dw (xh gamma + beta), dmod_beta = dres = dw, dgamma = sum du xh, dbeta = sum du"""
    N, S, C, G = c.N, c.S, c.C, c.G
    cpg = C // G
    x, dy = o["x"].to(f), o["dy"].to(f)
    mean, rstd = group_stats(x, G, f)
    fc = _c(c.name, N, S, C, G, c.affine, c.act, None, 0)
    mean_c, rstd_c = _per_channel(mean, fc), _per_channel(rstd, fc)
    gam = (o["gamma"] if c.affine else torch.ones(C, dtype=F64)).to(f)
    bet = (o["beta"] if c.affine else torch.zeros(C, dtype=F64)).to(f)
    xh = (x - mean_c) * rstd_c
    if c.from_pre:
        da = _act_grad_pre64(c.act, x * (rstd_c * gam) + (bet - mean_c * rstd_c * gam))
    else:
        da = act_grad_from_out64(c.act, o["y"].to(f)) if c.act != _lib.ACT_NONE else torch.ones_like(dy)
    dw = dy * da
    one_mg = 1.0 + o["mg"].to(f)[torch.arange(N) % o["mg"].shape[0]] if c.mod else None
    du = dw * one_mg if c.mod else dw
    grp = lambda t: t.view(N, S, G, cpg).sum(dim=(1, 3)).repeat_interleave(cpg, dim=1).view(N, 1, C)      # noqa: E731
    cnt = float(S * cpg)
    s1, s2 = grp(gam * du), grp(gam * du * xh)
    out = dict(dx=rstd_c * (du * gam - (s1 + xh * s2) / cnt), dres=dw if c.res else None,
               dmg=dw * (xh * gam + bet) if c.mod else None, dmb=dw if c.mod else None,
               dgamma=(du * xh).sum(dim=(0, 1)) if c.affine else None, dbeta=du.sum(dim=(0, 1)) if c.affine else None)
    a = torch.abs
    mabs = _per_channel(a(x).view(N, S, G, cpg).mean(dim=(1, 3)), fc)       # the terms of the mean: sum |x| / count
    xm = (a(x) + mabs) * rstd_c                               # the terms of xh = x rstd - mean rstd
    mag = dict(dx=a(rstd_c) * (a(du * gam) + (grp(a(gam * du)) + xm * grp(a(gam * du) * xm)) / cnt), dres=a(dw), dmb=a(dw),
               dmg=a(dw) * (xm * a(gam) + a(bet)), dgamma=(a(du) * xm).sum(dim=(0, 1)), dbeta=a(du).sum(dim=(0, 1)))
    return frames_summed(c, out), frames_summed(c, mag)


def measure_backward(c, dt):
    """the yardstick of one case: worst error of the fp32 restatement against float64 autograd, per quantity (the magnitudes in float64)"""
    o = bwd_inputs(c, dt)
    ref = bwd_ref(c, o)
    f32, _ = bwd_restated(c, o, F32)
    _, mag = bwd_restated(c, o, F64)
    return {k: worst(f32[k], ref[k], mag[k]) for k in BWD_QTY if ref[k] is not None}
