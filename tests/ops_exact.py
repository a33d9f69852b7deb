"""Op-level checking of the differentiable HIP ops behind the convolution (ipoke_amd/autograd_ops.py: ``_NormFn``, ``_AddActFn``,
``_GruUnrollFn``, ``gru_cell``, ``_ReparamFn``, ``_KLFn``, ``_L1TanhFn``), of the block functions of ipoke_amd/first_stage_train.py
that compose them and of the inference twin's statistics hand-over (``K.group_norm(next_groups=...)``): the HOST layer between the
kernels that tests/norm_exact.py, gru_exact.py, sn_exact.py and disc_exact.py hold to float64 one by one -- which pointer, which pitch,
which stride into the sigma table, which clone, which order of the returned gradients.  References, case tables, the tape and the
runners; the test functions are in test_ops_exact_cpu.py (no device: references against second statements, input conditions,
yardsticks, label predictions, the fold predicate against the kernel's requirement) and test_ops_exact_gpu.py.

* The tape (``Tape``): a context manager that wraps ``conv_weight``, ``group_norm``, ``add_act``, ``gru_cell``, ``gru_unroll`` and
  the three latent / loss functions (in autograd_ops and under the names first_stage_train imported).  Every call becomes an
  ``OpRecord``: its inputs and its output by device address and as a CPU copy, its options, and -- through tensor hooks that only
  record -- the gradient that arrives at the output and the gradient that leaves for each differentiable input.  An input that
  requires grad enters the op through a view of itself, so that the hook sees this op's contribution alone where two ops read one
  tensor; a view keeps the address, which is what ``_output_gradient`` checks of the pre-scaled gradient.
  A chain of ops is then three checks: every op's forward against float64 of its own recorded inputs; every op's backward against
  float64 of its own recorded inputs and its own recorded incoming gradient (teacher forcing: a rounding flip is not carried on, the
  activation's derivative comes from the stored y as in ``norm_exact.bwd_ref``, every element is compared); and the wiring, exactly:
  the recorded input of an op is bit-equal to the recorded output of the op the block's definition names, and the gradient at a
  tensor two ops read is the sum of the two recorded contributions rounded once.
* Labels (in the manner of ``autograd_exact.BranchRecorder``): norm:fold | norm:plain, norm:res_post, norm:shared_maps, norm:part,
  conv:prescaled | conv:rowscale | conv:act_bwd, add_act:kernel | add_act:identity, gru:native | gru:cells.  Every case lists the
  labels it must take; norm:fold | norm:plain is what the norm's BACKWARD decided (it left a pre-scaled gradient or not).
* ``_NormFn`` alone: operands of norm_exact's centred family with integer dy (``norm_exact.bwd_inputs``), pitches above C whose
  padding holds SENT in every input and zero in dy, bounds ``norm_exact.gpu_bound`` / ``bwd_bound`` unchanged (test_ops_exact_cpu.py
  measures the fp32 restatement on these cases and holds it to norm_exact's recorded yardsticks).
* Convolution -> norm with the row-scale fold: ``autograd_exact.Operands`` (one-hot u / v, sigma_t a power of two, integers) make
  the convolution's output exact; the norm behind it is real-valued.  The gradient recorded at the convolution's output is held to
  ``norm_exact.fold_ref`` by the rule of test_groupnorm_backward; dX, dW and dbias are held to float64 autograd through the
  convolution from THAT recorded gradient, the error counted in fp32 ulps of the sum of the magnitudes of a result's terms, bound
  max(4 x yardstick, 4).  The yardstick is the worst error of a blocked fp32 restatement of the same contraction (exact partial
  sums over one matrix-core step of the reduction -- ``conv_exact.k_block`` channels of one tap for dX, 32 rows for dW and dbias --
  rounded to fp32 and added in order) on the float64 reference gradient rounded to the dtype, measured by test_ops_exact_cpu.py and
  recorded in CHAIN_YARDSTICK (rounded up to a tenth, capped at ``norm_exact.YARDSTICK_CAP``).  No number comes from a kernel.
* What the kernels' own contracts rule out: ipoke_groupnorm and ipoke_groupnorm_bwd refuse C % 8 != 0 in bf16, so C = 12 runs in f32
  only (where the pitch of 12 has no padding; the padding columns of every case come from pitches above C instead), and a chain
  that the fold predicate declines because of its pitch cannot reach the norm kernel at all; the predicate's declining branches
  are compared with the kernel's requirement on the CPU.
"""
import collections
import copy
import ctypes

import torch

from ipoke_amd import _lib, nn as K
from ipoke_amd import autograd_ops as FT
from ipoke_amd import first_stage as FS
from ipoke_amd import first_stage_train as FST
from tests import autograd_exact as A
from tests import conv_exact as CX
from tests import gru_exact as GX
from tests import norm_exact as NX
from tests.autograd_exact import assert_cl_equal, cl_of, set_one_hot, weight_handle  # noqa: F401
from tests.disc_exact import assert_same, randint64  # noqa: F401
from tests.norm_exact import DTYPES, F32, F64, SENT

DEV = "cuda"
NONE, RELU, ELU = _lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_ELU


# ====================================================================== the tape
Snapshot = collections.namedtuple("Snapshot", "ptr t")          # device address and a CPU copy


def snap(t):
    return Snapshot(t.data_ptr(), t.detach().cpu().clone())


class OpRecord:
    def __init__(self, kind, opts, depth):
        self.kind, self.opts, self.depth = kind, opts, depth
        self.ins, self.outs, self.g_out, self.g_in = {}, [], {}, {}

    @property
    def out(self):
        return self.outs[0]

    def __repr__(self):
        return f"<{self.kind} {self.opts} ins={list(self.ins)} g_in={list(self.g_in)}>"


_TAPED = ("conv_weight", "group_norm", "add_act", "gru_cell", "gru_unroll", "reparameterize", "kl_loss", "l1_tanh_loss")


class Tape:
    """see the module docstring.  ``records``: the calls in order (calls made inside a taped call -- the convolutions of ``gru_cell`` --
    have depth > 0); ``labels``: the branch labels taken."""

    def __init__(self):
        self.records, self.labels, self._depth, self._saved, self.conv_backwards = [], set(), 0, [], []

    # ---- recording
    def _begin(self, kind, **opts):
        r = OpRecord(kind, opts, self._depth)
        self.records.append(r)
        self._depth += 1
        return r

    def _tensor_in(self, r, name, t):
        if t is None:
            return None
        r.ins[name] = snap(t)
        if not t.requires_grad:
            return t
        v = t.view_as(t)                            # this op's own edge into t: the hook sees this op's contribution alone
        v.register_hook(lambda g: None if g is None else r.g_in.__setitem__(name, snap(g)))          # (returns None: records only)
        return v

    def _cl_in(self, r, name, cl):
        if cl is None:
            return None
        v = self._tensor_in(r, name, cl.t)
        if v is cl.t:
            return cl
        c2 = copy.copy(cl)                          # (keeps conv_meta / stats_part)
        c2.t = v
        return c2

    def _end(self, r, *outs):
        self._depth -= 1
        for i, t in enumerate(outs):
            r.outs.append(snap(t))
            if t.requires_grad:
                t.register_hook(lambda g, i=i: None if g is None else r.g_out.__setitem__(i, snap(g)))          # (an unused output: None)
        return r

    # ---- the wrappers
    def __enter__(self):
        tape = self
        o = {n: getattr(FT, n) for n in _TAPED}
        o_norm_apply, o_add_apply, o_outgrad = FT._NormFn.apply, FT._AddActFn.apply, FT._output_gradient
        o_norm_bwd = self._norm_bwd = FT._NormFn.backward
        o_kgn = K.group_norm

        def conv_weight(x, w, bias, k, stride, pad, dtype, **kw):
            r = tape._begin("conv", k=tuple(k), stride=tuple(stride), pad=tuple(pad), dtype=dtype, act=kw.get("act", NONE),
                            out_f32=kw.get("out_f32", False), transposed=kw.get("transposed", False), wkind=type(w).__name__)
            r.w = w.w_orig if isinstance(w, (FT._SnWeight, FT._SnFrames)) else w
            r.bias = bias
            y = o["conv_weight"](tape._cl_in(r, "x", x), w, bias, k, stride, pad, dtype, **kw)
            r.meta = y.conv_meta
            tape._end(r, y.t)
            return y

        def group_norm(x, groups, dtype, gamma=None, beta=None, act=NONE, res=None, mod=None, sole_reader=False, res_post=False):
            r = tape._begin("norm", groups=groups, dtype=dtype, act=act, sole_reader=sole_reader, res_post=res_post, affine=gamma is not None,
                            N=x.N, S=x.S, C=x.C, mod_N=None if mod is None else mod[0].N)
            r.gamma, r.beta = gamma, beta
            m2 = None if mod is None else (tape._cl_in(r, "mg", mod[0]), tape._cl_in(r, "mb", mod[1]))
            y = o["group_norm"](tape._cl_in(r, "x", x), groups, dtype, gamma, beta, act=act, res=tape._cl_in(r, "res", res), mod=m2,
                                sole_reader=sole_reader, res_post=res_post)
            tape._end(r, y.t)
            return y

        def add_act(a, b, dtype, act):
            r = tape._begin("add_act", dtype=dtype, act=act, C=a.C)
            y = o["add_act"](tape._cl_in(r, "a", a), tape._cl_in(r, "b", b), dtype, act)
            tape._end(r, y.t)
            return y

        def gru_cell(cell, x, h, dtype, gate_w=None):
            tape.labels.add("gru:cells")
            r = tape._begin("gru_cell", dtype=dtype)
            y = o["gru_cell"](cell, tape._cl_in(r, "x", x), tape._cl_in(r, "h", h), dtype, gate_w)
            tape._end(r, y.t)
            return y

        def gru_unroll(rnn, in_rnn, h0, steps, dtype, gate_w=None):
            tape.labels.add("gru:native")
            r = tape._begin("gru_unroll", dtype=dtype, steps=steps)
            y = o["gru_unroll"](rnn, tape._cl_in(r, "x", in_rnn), tape._cl_in(r, "h", h0), steps, dtype, gate_w)
            tape._end(r, y.t)
            return y

        def reparameterize(mulv_t, eps_s, Z, dtype):
            r = tape._begin("reparam", Z=Z, dtype=dtype)
            r.ins["eps"] = snap(eps_s)
            z, mu, lv = o["reparameterize"](tape._tensor_in(r, "mulv", mulv_t), eps_s, Z, dtype)
            tape._end(r, z, mu, lv)
            return z, mu, lv

        def kl_loss(mu, lv):
            r = tape._begin("kl")
            y = o["kl_loss"](tape._tensor_in(r, "mu", mu), tape._tensor_in(r, "lv", lv))
            tape._end(r, y)
            return y

        def l1_tanh_loss(pre_t, x_nchw, scale):
            r = tape._begin("l1_tanh", scale=float(scale))
            r.ins["target"] = snap(x_nchw)
            loss, frame = o["l1_tanh_loss"](tape._tensor_in(r, "pre", pre_t), x_nchw, scale)
            tape._end(r, loss, frame)
            return loss, frame

        # ---- labels
        def norm_backward(ctx, dy):
            out = o_norm_bwd(ctx, dy)
            pm = ctx.meta.get("producer")              # the fold as backward decided it: the dx it returns is what it left for the convolution
            folded = pm is not None and pm.get("_prescaled") is not None and pm["_prescaled"][0] is out[0]
            tape.labels.add("norm:fold" if folded else "norm:plain")
            return out

        def norm_apply(x_t, gamma, beta, mg_t, mb_t, res_t, meta):
            if meta.get("res_post"):
                tape.labels.add("norm:res_post")
            if mg_t is not None and 0 < int(meta.get("mod_samples", 0)) < meta["N"]:
                tape.labels.add("norm:shared_maps")
            return o_norm_apply(x_t, gamma, beta, mg_t, mb_t, res_t, meta)

        def add_apply(a_t, b_t, C, act, dtype):
            tape.labels.add("add_act:identity" if act == NONE else "add_act:kernel")          # (what backward does)
            return o_add_apply(a_t, b_t, C, act, dtype)

        def output_gradient(m, dy, y_t, bias32, want_b):
            tape.conv_backwards.append(m)
            if m.get("_prescaled") is not None:
                tape.labels.add("conv:prescaled")
            elif m.get("sn_frames") is not None:
                tape.labels.add("conv:rowscale")
            elif m["act"] != NONE:
                tape.labels.add("conv:act_bwd")
            return o_outgrad(m, dy, y_t, bias32, want_b)

        def k_group_norm(x, groups, dtype, gamma=None, beta=None, act=NONE, res=None, mod=None, **kw):
            handed = getattr(x, "stats_part", None)
            r = tape._begin("knorm", groups=groups, dtype=dtype, act=act, res_post=kw.get("res_post", False), next_groups=kw.get("next_groups"),
                            N=x.N, S=x.S, C=x.C, handed=None if handed is None else handed[0])
            r.gamma, r.beta = gamma, beta
            for name, cl in (("x", x), ("res", res), ("mg", None if mod is None else mod[0]), ("mb", None if mod is None else mod[1])):
                if cl is not None:
                    r.ins[name] = snap(cl.t)
            out = o_kgn(x, groups, dtype, gamma, beta, act=act, res=res, mod=mod, **kw)
            r.opts["offered"] = getattr(out, "stats_part", None) is not None
            r.opts["part"] = handed is not None and getattr(x, "stats_part", None) is None
            if r.opts["part"]:
                tape.labels.add("norm:part")
            tape._end(r, out.t)
            return out

        new = dict(conv_weight=conv_weight, group_norm=group_norm, add_act=add_act, gru_cell=gru_cell, gru_unroll=gru_unroll,
                   reparameterize=reparameterize, kl_loss=kl_loss, l1_tanh_loss=l1_tanh_loss)
        for mod in (FT, FST):
            for n, f in new.items():
                if hasattr(mod, n):
                    self._saved.append((mod, n, getattr(mod, n)))
                    setattr(mod, n, f)
        for obj, n, f in ((FT, "_output_gradient", output_gradient), (K, "group_norm", k_group_norm)):
            self._saved.append((obj, n, getattr(obj, n)))
            setattr(obj, n, f)
        FT._NormFn.apply = staticmethod(norm_apply)
        FT._NormFn.backward = staticmethod(norm_backward)
        FT._AddActFn.apply = staticmethod(add_apply)
        return self

    def __exit__(self, *exc):
        for obj, n, old in reversed(self._saved):
            setattr(obj, n, old)
        self._saved = []
        FT._NormFn.backward = staticmethod(self._norm_bwd)
        del FT._NormFn.apply                        # (inherited from torch.autograd.Function again)
        del FT._AddActFn.apply
        return False

    def taken(self, prefix=None):
        return tuple(sorted(l for l in self.labels if prefix is None or l.startswith(prefix)))

    def of(self, kind, top_only=True):
        return [r for r in self.records if r.kind == kind and (r.depth == 0 or not top_only)]


def assert_fed_by(consumer, name, producer, what, out=0):
    """wiring, exact: the recorded input ``name`` of ``consumer`` is the recorded output of ``producer`` -- same address, same bits"""
    a, b = consumer.ins[name], producer.outs[out]
    assert a.ptr == b.ptr, f"{what}: input {name} lives at another address than the output that should feed it"
    assert a.t.dtype == b.t.dtype and torch.equal(a.t.view(torch.uint8), b.t.view(torch.uint8)), f"{what}: input {name} differs from the output that feeds it"


def rne(v64, tdt):
    """float64 -> the compute dtype (through fp32, as the kernels round)"""
    return v64.to(F32).to(tdt)


def assert_sum_of_two(total, a, b, tdt, what):
    """the gradient at a tensor two ops read == RNE(a + b) of the two recorded contributions, bit for bit"""
    assert_same(total.contiguous(), rne(a.to(F64) + b.to(F64), tdt), what)


# ====================================================================== operands on the device
def cl_dev(v, C, ld, tdt, fill=0.0, grad=False):
    """float64 [..., C] -> device rows [M, ld] of the compute dtype, the padding columns holding ``fill``"""
    rows = v.reshape(-1, C)
    t = torch.full((rows.shape[0], ld), fill, dtype=tdt)
    t[:, :C] = rows.to(tdt)
    return t.to(DEV).requires_grad_(grad)


def f32_dev(v, grad=False):
    return None if v is None else v.to(F32).to(DEV).requires_grad_(grad)


# ====================================================================== _NormFn alone
# res: None | "pre" (in front of the activation) | "post" (behind it: res_post); mod: 0 none, -1 one SPADE map per sample, k > 0 shared
# maps of k clips (mod[0].N = k < N: group_norm sets mod_samples and the kernel sums the frames' map gradients)
NormOp = collections.namedtuple("NormOp", "name N S C G affine act res mod dtypes", defaults=(("f32", "bf16"),))
NORM_OPS = [
    NormOp("op-affine-relu-pre", 4, 35, 32, 4, True, RELU, "pre", 0),
    NormOp("op-affine-elu-g1", 2, 130, 16, 1, True, ELU, None, 0),
    NormOp("op-instance-none", 3, 64, 32, 32, False, NONE, None, 0),
    NormOp("op-instance-elu-post", 2, 35, 16, 16, False, ELU, "post", 0),
    NormOp("op-affine-relu-post", 4, 64, 32, 4, True, RELU, "post", 0),
    NormOp("op-instance-relu-post-130", 3, 130, 16, 16, False, RELU, "post", 0),
    NormOp("op-instance-relu-pre-c12", 2, 35, 12, 12, False, RELU, "pre", 0, ("f32",)),
    NormOp("op-affine-none-c12-g4", 3, 64, 12, 4, True, NONE, None, 0, ("f32",)),
    NormOp("op-affine-elu-pre-c12-g1", 2, 130, 12, 1, True, ELU, "pre", 0, ("f32",)),
    NormOp("op-spade-per-sample", 2, 130, 32, 4, False, NONE, None, -1),
    NormOp("op-spade-per-sample-relu-pre", 3, 35, 16, 1, True, RELU, "pre", -1),
    NormOp("op-spade-per-sample-elu", 2, 64, 16, 16, False, ELU, None, -1),
    NormOp("op-spade-shared", 6, 64, 32, 4, False, NONE, None, 2),
    NormOp("op-spade-shared-relu-35", 4, 35, 16, 16, False, RELU, None, 2),
    NormOp("op-spade-shared-elu-130", 6, 130, 16, 4, True, ELU, "pre", 3),
]
NORM_OP = {c.name: c for c in NORM_OPS}
# the fp32 restatement of the backward on a case's own operands where it exceeds norm_exact's recorded figure (ELU with a residual or with
# maps, which norm_exact's table has with ReLU only; the sums of two or three frames): (case, dtype, quantity) -> units, rounded up.  The
# bounds on the device stay norm_exact's; test_ops_exact_cpu.py holds every figure here below that bound.
NORM_OP_YARDSTICK = {
    ("op-affine-elu-pre-c12-g1", "f32", "dres"): 0.9,
    ("op-spade-per-sample", "f32", "dmg"): 2.8,
    ("op-spade-per-sample-elu", "f32", "dmb"): 0.9,
    ("op-spade-shared-elu-130", "f32", "dres"): 0.9,
    ("op-spade-shared-elu-130", "f32", "dmg"): 2.2,
    ("op-spade-shared-elu-130", "f32", "dmb"): 1.2,
}
NORM_PAIRS = [(c.name, dt) for c in NORM_OPS for dt in c.dtypes]
ALL_INPUTS = ("x", "affine", "mod", "res")


def bwd_case(c):
    return NX.BwdCase(c.name, c.N, c.S, c.C, c.G, c.affine, c.act, c.res == "pre", c.mod, True, c.res == "post", c.mod > 0, None)


def fwd_case(c):
    return NX._c(c.name, c.N, c.S, c.C, c.G, c.affine, c.act, c.res, c.mod)


def norm_labels(c):
    return tuple(sorted({"norm:plain"} | ({"norm:res_post"} if c.res == "post" else set()) | ({"norm:shared_maps"} if c.mod > 0 else set())))


class NormRun:
    """one ``FT.group_norm`` call on the operands of ``norm_exact.bwd_inputs``: forward(), backward(), check().  ``need``: the inputs
    that require grad; ``ld``: pitches of x (= y, dy), the residual and the maps (default C + e, C + e, C + 2 e)."""

    def __init__(self, c, dt, need=ALL_INPUTS, ld=None):
        code, tdt, e = DTYPES[dt]
        self.c, self.dt, self.tdt, self.need = c, dt, tdt, tuple(need)
        self.o = o = NX.bwd_inputs(bwd_case(c), dt)
        C = c.C
        self.ld = dict(x=C + e, res=C + e, mod=C + 2 * e)
        self.ld.update(ld or {})
        self.x = cl_dev(o["x"], C, self.ld["x"], tdt, SENT, "x" in need)
        self.gamma = f32_dev(o["gamma"], "affine" in need) if c.affine else None
        self.beta = f32_dev(o["beta"], "affine" in need) if c.affine else None
        self.mg = cl_dev(o["mg"], C, self.ld["mod"], tdt, SENT, "mod" in need) if c.mod else None
        self.mb = cl_dev(o["mb"], C, self.ld["mod"], tdt, SENT, "mod" in need) if c.mod else None
        self.res = cl_dev(o["res"], C, self.ld["res"], tdt, SENT, "res" in need) if c.res else None
        self.dy = cl_dev(o["dy"], C, self.ld["x"], tdt, 0.0)

    def forward(self):
        c = self.c
        dhw = (1, 1, c.S)
        mod = None
        if c.mod:
            rows = self.o["mg"].shape[0]
            mod = (K.CL(self.mg, rows, dhw, c.C), K.CL(self.mb, rows, dhw, c.C))
        res = None if self.res is None else K.CL(self.res, c.N, dhw, c.C)
        self.y = FT.group_norm(K.CL(self.x, c.N, dhw, c.C), c.G, self.dt, self.gamma, self.beta, act=c.act, res=res, mod=mod,
                               res_post=c.res == "post")
        return self.y

    def backward(self):
        self.y.t.backward(self.dy)
        torch.cuda.synchronize()

    def check(self):
        """y and every gradient against float64 (bounds of norm_exact), the exact properties, and that no gradient exists that
        nobody asked for.  Returns the worst figures in units."""
        c, dt, tdt, o = self.c, self.dt, self.tdt, dict(self.o)
        N, S, C = c.N, c.S, c.C
        what = f"group_norm {c.name} {dt}"
        figs = {}
        y = self.y.t.detach().cpu()
        ref_f = NX.fwd_ref(fwd_case(c), o)
        figs["y"] = NX.assert_units(what + " y", y[:, :C].reshape(N, S, C), ref_f["y"], ref_f["mag"], NX.gpu_bound("y", "centred", dt), tdt)
        assert bool((y[:, C:] == 0).all()), what + ": padding columns of y"
        o["y"] = y[:, :C].reshape(N, S, C).to(F64)                 # teacher forcing: act' from the stored output
        bc = bwd_case(c)
        ref = NX.bwd_ref(bc, o)
        _, mag = NX.bwd_restated(bc, o, F64)
        g = lambda t: None if t is None or t.grad is None else t.grad.detach().cpu()          # noqa: E731
        got = dict(dx=g(self.x), dres=g(self.res), dmg=g(self.mg), dmb=g(self.mb), dgamma=g(self.gamma), dbeta=g(self.beta))
        asked = dict(dx="x", dres="res", dmg="mod", dmb="mod", dgamma="affine", dbeta="affine")
        leaf = dict(dx=self.x, dres=self.res, dmg=self.mg, dmb=self.mb, dgamma=self.gamma, dbeta=self.beta)
        for k, v in got.items():
            if leaf[k] is None or asked[k] not in self.need:
                assert v is None, f"{what}: a gradient {k} nobody asked for"
                continue
            assert v is not None and v.shape == leaf[k].shape and v.dtype == leaf[k].dtype, f"{what}: {k} missing or of another shape"
            if k in ("dgamma", "dbeta"):
                figs[k] = NX.assert_units(f"{what} {k}", v, ref[k], mag[k], NX.bwd_bound(k, dt))
                continue
            rows = c.mod if (k in ("dmg", "dmb") and c.mod > 0) else N
            assert v.shape[0] == rows * S, f"{what}: {k} has {v.shape[0]} rows for {rows} x {S}"
            assert bool((v[:, C:] == 0).all()), f"{what}: padding columns of {k}"
            body = v[:, :C].reshape(rows, S, C)
            if k == "dres" and c.res == "post":
                assert_same(v.contiguous(), self.dy.cpu()[:, :v.shape[1]].contiguous() if v.shape[1] <= self.dy.shape[1] else
                            torch.cat([self.dy.cpu(), torch.zeros(v.shape[0], v.shape[1] - self.dy.shape[1], dtype=v.dtype)], 1),
                            what + ": dres is the incoming gradient under res_post")
                continue
            figs[k] = NX.assert_units(f"{what} {k}", body, ref[k], mag[k], NX.bwd_bound(k, dt), tdt)
            if k in ("dres", "dmb") and c.act in (NONE, RELU) and c.res != "post":
                assert_same(body.contiguous(), ref[k], f"{what}: {k} is exact under ReLU / no activation")
        return figs


def run_norm_op(c, dt, need=ALL_INPUTS, ld=None, labels=True):
    with Tape() as tape:
        r = NormRun(c, dt, need, ld)
        r.forward()
        r.backward()
    if labels:
        assert tape.taken("norm:") == norm_labels(c), f"{c.name} {dt}: took {tape.taken()}, expected {norm_labels(c)}"
    r.tape = tape
    r.figs = r.check()
    return r


# ====================================================================== convolution -> norm with the row-scale fold
# conv: an autograd_exact.Case (frame-batched spectral norm, exact operands); kind: "in" (InstanceNorm) | "group" (16 groups, affine)
ChainCase = collections.namedtuple("ChainCase", "name conv kind act res_post dtypes", defaults=(False, ("f32", "bf16")))


def _chain(name, cin, cout, stride, ext, frames, N, bias, kind, act, transposed=False, lim=2, **kw):
    conv = A.Case("chain_" + name, 2, cin, cout, (1, 3, 3), (1, stride, stride), (0, 1, 1), ext, (), transposed=transposed, bias=bias,
                  wkind="sn_frames", frames=frames, N=N, lim=lim, run=False)
    return ChainCase(name, conv, kind, act, **kw)


CHAINS = [
    _chain("s1-bias-in-elu", 8, 16, 1, (1, 6, 7), 3, 6, True, "in", ELU),
    _chain("s1-nobias-group-relu", 16, 32, 1, (1, 8, 8), 3, 6, False, "group", RELU, lim=1),          # (the frames' dots run over 16 x 32 x 9 weights)
    _chain("s2-bias-in-none", 8, 16, 2, (1, 8, 8), 3, 6, True, "in", NONE),
    _chain("ct-bias-in-relu", 16, 8, 2, (1, 6, 7), 3, 6, True, "in", RELU, transposed=True),
    _chain("frames1-group-elu", 8, 32, 1, (1, 7, 6), 1, 2, True, "group", ELU),
    _chain("res-post-in-relu", 8, 16, 1, (1, 6, 7), 3, 6, True, "in", RELU, res_post=True),
    _chain("c12-in-relu-f32", 8, 12, 1, (1, 7, 7), 3, 6, True, "in", RELU, dtypes=("f32",)),
    _chain("ct-frames1-in-relu", 16, 8, 2, (1, 7, 6), 1, 2, True, "in", RELU, transposed=True),
]
# the chains that first_stage_train's block functions can state (power iteration off: one sigma for the batch): conv_block, convT_block
BLOCK_CHAINS = {"frames1-group-elu": "conv_block", "ct-frames1-in-relu": "convT_block"}
ACT_NAME = {NONE: "none", RELU: "relu", ELU: "elu"}
CHAIN = {c.name: c for c in CHAINS}
CHAIN_PAIRS = [(c.name, dt) for c in CHAINS for dt in c.dtypes]
CHAIN_QTY = ("dx", "dw", "db")
# worst error of the blocked fp32 restatement of each chain's three gradient contractions against float64, in ulp32(S), rounded up
# to a tenth (test_ops_exact_cpu.py measures and asserts them); bound on the device max(4 x yardstick, 4)
CHAIN_YARDSTICK = {
    ("s1-bias-in-elu", "f32", "dx"): 1.0, ("s1-bias-in-elu", "f32", "dw"): 0.5, ("s1-bias-in-elu", "f32", "db"): 0.1,
    ("s1-bias-in-elu", "bf16", "dx"): 0.0, ("s1-bias-in-elu", "bf16", "dw"): 0.2, ("s1-bias-in-elu", "bf16", "db"): 0.0,
    ("s1-nobias-group-relu", "f32", "dx"): 1.1, ("s1-nobias-group-relu", "f32", "dw"): 0.8,
    ("s1-nobias-group-relu", "bf16", "dx"): 0.3, ("s1-nobias-group-relu", "bf16", "dw"): 0.3,
    ("s2-bias-in-none", "f32", "dx"): 0.9, ("s2-bias-in-none", "f32", "dw"): 0.6, ("s2-bias-in-none", "f32", "db"): 0.0,
    ("s2-bias-in-none", "bf16", "dx"): 0.0, ("s2-bias-in-none", "bf16", "dw"): 0.0, ("s2-bias-in-none", "bf16", "db"): 0.0,
    ("ct-bias-in-relu", "f32", "dx"): 1.3, ("ct-bias-in-relu", "f32", "dw"): 1.1, ("ct-bias-in-relu", "f32", "db"): 0.1,
    ("ct-bias-in-relu", "bf16", "dx"): 0.0, ("ct-bias-in-relu", "bf16", "dw"): 0.3, ("ct-bias-in-relu", "bf16", "db"): 0.0,
    ("frames1-group-elu", "f32", "dx"): 0.7, ("frames1-group-elu", "f32", "dw"): 0.7, ("frames1-group-elu", "f32", "db"): 0.2,
    ("frames1-group-elu", "bf16", "dx"): 0.2, ("frames1-group-elu", "bf16", "dw"): 0.4, ("frames1-group-elu", "bf16", "db"): 0.1,
    ("res-post-in-relu", "f32", "dx"): 0.9, ("res-post-in-relu", "f32", "dw"): 0.8, ("res-post-in-relu", "f32", "db"): 0.1,
    ("res-post-in-relu", "bf16", "dx"): 0.5, ("res-post-in-relu", "bf16", "dw"): 0.2, ("res-post-in-relu", "bf16", "db"): 0.0,
    ("c12-in-relu-f32", "f32", "dx"): 1.0, ("c12-in-relu-f32", "f32", "dw"): 0.5, ("c12-in-relu-f32", "f32", "db"): 0.1,
    ("ct-frames1-in-relu", "f32", "dx"): 1.4, ("ct-frames1-in-relu", "f32", "dw"): 1.3, ("ct-frames1-in-relu", "f32", "db"): 0.2,
    ("ct-frames1-in-relu", "bf16", "dx"): 0.5, ("ct-frames1-in-relu", "bf16", "dw"): 0.5, ("ct-frames1-in-relu", "bf16", "db"): 0.0,
}
# the fp32 restatement of the norm on a chain's integer x where it exceeds norm_exact's recorded centred yardstick (the old table is
# left alone): (chain, dtype, quantity) -> units
CHAIN_NORM_YARDSTICK = {
}


def chain_bound(name, dt, qty):
    return max(4.0 * CHAIN_YARDSTICK[(name, dt, qty)], 4.0)


def chain_norm_bound(name, dt, qty):
    """the norm's bound in a chain: norm_exact's, or from the chain's own recorded yardstick where that is larger"""
    own = CHAIN_NORM_YARDSTICK.get((name, dt, qty))
    base = NX.gpu_bound(qty, "centred", dt) if qty in ("y", "mean", "rstd") else NX.bwd_bound(qty, dt)
    return base if own is None else max(base, 4.0 * own)


def chain_geometry(cc):
    case = cc.conv
    o = case.odhw()
    return case.N, o[0] * o[1] * o[2], case.cout, (case.cout if cc.kind == "in" else 16)


def chain_bwd_case(cc):
    N, S, C, G = chain_geometry(cc)
    bias = cc.conv.bias
    return NX.BwdCase(cc.name, N, S, C, G, cc.kind == "group", cc.act, False, 0, True, cc.res_post, False, (N // cc.conv.frames, 2, bias, bias))


def chain_fwd_case(cc):
    N, S, C, G = chain_geometry(cc)
    return NX._c(cc.name, N, S, C, G, cc.kind == "group", cc.act, "post" if cc.res_post else None, 0)


def to_rows(t5):
    """[N, C, D, H, W] -> [N, S, C]"""
    N, C = t5.shape[:2]
    return t5.permute(0, 2, 3, 4, 1).reshape(N, -1, C).contiguous()


def to_maps(rows, odhw):
    """[N, S, C] -> [N, C, D, H, W]"""
    N, S, C = rows.shape
    return rows.reshape(N, *odhw, C).permute(0, 4, 1, 2, 3).contiguous()


def chain_inputs(cc, dt):
    """what the norm of a chain reads, as norm_exact's dict: x = the convolution's exact output, integer dy, gamma / beta, the residual
    behind the activation, rs_bias = the convolution's bias; scales = the frames' 1 / sigma_t"""
    tdt = DTYPES[dt][1]
    ops_ = A.operands(cc.conv)
    N, S, C, G = chain_geometry(cc)
    gen = torch.Generator().manual_seed(NX.seed_of("chain-" + cc.name))
    o = dict(x=to_rows(ops_.y), dy=randint64(-4, 4, (N, S, C), gen), mg=None, mb=None)
    affine = cc.kind == "group"
    o["gamma"] = NX.rnd(1.0 + 0.3 * torch.randn(C, generator=gen, dtype=F64), F32) if affine else None
    o["beta"] = NX.rnd(0.2 * torch.randn(C, generator=gen, dtype=F64), F32) if affine else None
    o["res"] = NX.rnd(0.7 * torch.randn((N, S, C), generator=gen, dtype=F64), tdt) if cc.res_post else None
    o["rs_bias"] = ops_.b
    o["scales"] = [1.0 / p[2] for p in ops_.pairs]
    return o


def chain_input_conditions(cc, dt):
    """asserted, never clipped: every (sample, group) of the convolution's output holds at least two distinct values; the output is a
    value of the dtype (|y| <= 256 quanta where it is stored in bf16, asserted by the operand generator); every sum of the
    convolution's forward stays below 2^24 quanta (asserted by the operand generator too)"""
    ops_ = A.operands(cc.conv)
    N, S, C, G = chain_geometry(cc)
    x = to_rows(ops_.y).view(N, S, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1)
    assert bool(((x.amax(dim=-1) - x.amin(dim=-1)) > 0).all()), f"{cc.name}: a constant (sample, group) in the convolution's output"
    assert ops_.saved_y_exact and ops_.bounds["y"] < CX.EXACT_LIMIT
    tdt = DTYPES[dt][1]
    assert torch.equal(NX.rnd(ops_.y, tdt), ops_.y), f"{cc.name} {dt}: the convolution's output is not a value of the dtype"


def conv_from_gradient(case, ops_, dY5):
    """float64 autograd through the convolution (W / sigma_t per frame group, sigma_t a function of W) from the gradient dY at its output:
    dict of dx [N, cin, ...], dw (the weight's own layout, 5-D), db, and S_dx, S_dw, S_db: the sums of the magnitudes of their terms"""
    x = ops_.x.clone().requires_grad_(True)
    w5 = ops_.w5.clone().requires_grad_(True)
    b = None if ops_.b is None else ops_.b.clone().requires_grad_(True)
    ops_.forward64(x, w5, b).backward(dY5)
    sg = [p[2] for p in ops_.pairs]
    per = case.N // len(sg)
    xa = ops_.x.abs().requires_grad_(True)
    weff = [(ops_.w5.abs() / s).requires_grad_(True) for s in sg]
    conv_abs = torch.cat([A._conv64(case, xa[t * per:(t + 1) * per], weff[t]) for t in range(len(sg))], 0)
    conv_abs.backward(dY5.abs())
    ya = conv_abs.detach() + (0 if ops_.b is None else ops_.b.abs().view(1, -1, 1, 1, 1))
    S_dw = sum(weff[t].grad / sg[t] for t in range(len(sg)))
    rank1 = torch.zeros(case.cout, S_dw.numel() // case.cout, dtype=F64)
    for t, (i, j, s) in enumerate(ops_.pairs):
        rank1[i, j] += float((dY5[t * per:(t + 1) * per].abs() * ya[t * per:(t + 1) * per]).sum()) / s
    rank1 = rank1.reshape(case.cout, case.cin, *case.k).transpose(0, 1) if case.transposed else rank1.reshape(S_dw.shape)
    return dict(dx=x.grad, dw=w5.grad, db=None if b is None else b.grad, S_dx=xa.grad, S_dw=S_dw + rank1,
                S_db=dY5.abs().sum((0, 2, 3, 4)))


def conv_restated(case, ops_, dY5, dt):
    """the three contractions in blocked fp32: exact partial sums over one step of the reduction (k_block channels of one tap for the
    data gradient, 32 output rows for the weight and bias gradients and the frames' dots), rounded to fp32 and added in order"""
    kb = CX.k_block(DTYPES[dt][0])
    sg = [p[2] for p in ops_.pairs]
    per = case.N // len(sg)
    inv = torch.tensor([1.0 / s for s in sg], dtype=F64).repeat_interleave(per).view(-1, 1, 1, 1, 1)
    g5 = dY5 * inv                                          # the rows of both gradient GEMMs
    w5 = ops_.w5
    cdim = 1 if case.transposed else 0                      # the output-channel dimension of the weight's storage
    dx = torch.zeros(ops_.x.shape, dtype=F32)
    for kh in range(case.k[1]):
        for kw in range(case.k[2]):
            for c0 in range(0, case.cout, kb):
                wm = torch.zeros_like(w5)
                sl = [slice(None)] * 5
                sl[cdim], sl[3], sl[4] = slice(c0, c0 + kb), kh, kw
                wm[tuple(sl)] = w5[tuple(sl)]
                x0 = torch.zeros_like(ops_.x).requires_grad_(True)
                (part,) = torch.autograd.grad(A._conv64(case, x0, wm), x0, g5)
                dx = dx + part.to(F32)
    M = g5.numel() // case.cout
    pos = torch.arange(M).view(case.N, 1, *g5.shape[2:])
    dw = torch.zeros(w5.shape, dtype=F32)
    db = torch.zeros(case.cout, dtype=F32)
    dots = [torch.zeros((), dtype=F32) for _ in sg]
    ypre = torch.cat([A._conv64(case, ops_.x[t * per:(t + 1) * per], w5 / s) for t, s in enumerate(sg)], 0)          # Y - b, exact
    for m0 in range(0, M, 32):
        mask = ((pos >= m0) & (pos < m0 + 32)).to(F64)
        w0 = torch.zeros_like(w5).requires_grad_(True)
        (part,) = torch.autograd.grad(A._conv64(case, ops_.x, w0), w0, g5 * mask)
        dw = dw + part.to(F32)
        db = db + (dY5 * mask).sum((0, 2, 3, 4)).to(F32)
        for t in range(len(sg)):
            sel = slice(t * per, (t + 1) * per)
            dots[t] = dots[t] + (dY5[sel] * mask[sel] * ypre[sel]).sum().to(F32)
    r1 = torch.zeros(case.cout, dw.numel() // case.cout, dtype=F32)
    for t, (i, j, s) in enumerate(ops_.pairs):
        r1[i, j] = r1[i, j] + dots[t] * torch.tensor(1.0 / s, dtype=F32)
    r1 = r1.reshape(case.cout, case.cin, *case.k).transpose(0, 1) if case.transposed else r1.reshape(dw.shape)
    return dict(dx=dx, dw=dw - r1, db=db if ops_.b is not None else None)


def units32(got, ref, S, store_dt=None):
    """|got - ref| in ulp32(S), element by element; a bf16 store is allowed one bf16 ulp of the value first"""
    err = (got.to(F64) - ref).abs()
    if store_dt == torch.bfloat16:
        err = (err - NX.ulp_bf16(ref)).clamp(min=0)
    return err / CX.ulp32(S)


def assert_units32(what, got, ref, S, bound, store_dt=None):
    u = units32(got, ref, S, store_dt)
    bad = ~(u <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond {bound} units (worst {float(u.max()):.2f}); first at flat "
                             f"index {i}: got {float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}, S {float(S.reshape(-1)[i])!r}")
    return float(u.max())


def chain_reference_gradient(cc, dt):
    """the float64 gradient at the convolution's output on the CPU's own forward: (dx, dx / sigma_t rounded to the dtype) [N, S, C]"""
    tdt = DTYPES[dt][1]
    o = chain_inputs(cc, dt)
    o["y"] = NX.rnd(NX.fwd_ref(chain_fwd_case(cc), o)["y"], tdt)
    bc = chain_bwd_case(cc)
    dx = NX.bwd_ref(bc, o)["dx"]
    fr = NX.fold_ref(bc, o, NX.rnd(dx, tdt), scales=o["scales"])
    return dx, NX.rnd(fr["dx"], tdt), o


def measure_chain(cc, dt):
    """the yardsticks of a chain on the CPU: the three contractions of the convolution's backward in blocked fp32 against float64 (on
    the reference gradient rounded to the dtype) and the norm's fp32 restatement on the chain's integer x"""
    tdt = DTYPES[dt][1]
    case, ops_ = cc.conv, A.operands(cc.conv)
    _, g, o = chain_reference_gradient(cc, dt)
    sc = torch.tensor(o["scales"], dtype=F64).repeat_interleave(case.N // case.frames).view(-1, 1, 1)
    dY5 = to_maps(g / sc, case.odhw())
    ref, rs = conv_from_gradient(case, ops_, dY5), conv_restated(case, ops_, dY5, dt)
    out = {k: float(units32(rs[k], ref[k], ref["S_" + k]).max()) for k in CHAIN_QTY if ref[k] is not None}
    fc, bc = chain_fwd_case(cc), chain_bwd_case(cc)
    f64, f32 = NX.fwd_ref(fc, o), NX.fwd_ref(fc, o, F32)
    out.update(y=NX.worst(f32["y"], f64["y"], f64["mag"]), mean=NX.worst(f32["mean"], f64["mean"], f64["mean"]),
               rstd=NX.worst(f32["rstd"], f64["rstd"], f64["rstd"]))
    bref = NX.bwd_ref(bc, o)
    b32, _ = NX.bwd_restated(bc, o, F32)
    _, mag = NX.bwd_restated(bc, o, F64)
    out.update({"n" + k: NX.worst(b32[k], bref[k], mag[k]) for k in NX.BWD_QTY if bref[k] is not None})
    return out


class ChainRun:
    """conv (frame-batched spectral norm) -> norm(sole_reader) -> backward on the device, under the tape"""

    def __init__(self, cc, dt, sole_reader=True, need=(True, True, True), block=None):
        """block: "conv_block" | "convT_block" -- the same chain stated by first_stage_train's block function on a first_stage block"""
        code, tdt, e = DTYPES[dt]
        self.cc, self.dt, self.tdt, self.fold = cc, dt, tdt, sole_reader
        case = cc.conv
        self.ops = ops_ = A.operands(case)
        self.o = o = chain_inputs(cc, dt)
        N, S, C, G = chain_geometry(cc)
        blk = None
        if block == "conv_block":
            blk = FS.Conv2dBlock(case.cin, case.cout, 3, case.stride[1], 1, norm=cc.kind, activation=ACT_NAME[cc.act], snorm=True).to(DEV)
        elif block == "convT_block":            # (the key "elu" selects ReLU in this block)
            blk = FS.Conv2dTransposeBlock(case.cin, case.cout, 3, 2, 1, norm=cc.kind, activation="elu" if cc.act == RELU else ACT_NAME[cc.act], snorm=True).to(DEV)
        if blk is not None:
            assert sole_reader and case.frames == 1 and not cc.res_post
            A.load_operands(blk.conv, ops_)
        self.mod = mod = A.build_module(case, ops_) if blk is None else blk.conv
        A.weight_of(mod).requires_grad_(need[1])
        if case.bias:
            mod.bias.requires_grad_(need[2])
        self.nmod = nmod = FS._Norm("group" if cc.kind == "group" else "in", C).to(DEV) if blk is None else blk.norm
        if cc.kind == "group":
            with torch.no_grad():
                nmod.weight.copy_(o["gamma"].to(F32)); nmod.bias.copy_(o["beta"].to(F32))
        self.x_t = cl_of(ops_.x, dt).to(DEV).requires_grad_(need[0])
        self.res_t = cl_dev(o["res"], C, C, tdt, grad=True) if cc.res_post else None
        self.dz = cl_dev(o["dy"], C, C, tdt)
        with Tape() as self.tape:
            if blk is not None:
                self.z = getattr(FST, block)(blk, K.CL(self.x_t, case.N, case.ext, case.cin), dt, pit=False, frames=1)
            else:
                w = weight_handle(case, mod, ops_)
                self.y = FT.conv(mod, K.CL(self.x_t, case.N, case.ext, case.cin), dt, w=w)
                res = None if self.res_t is None else K.CL(self.res_t, N, self.y.dhw, C)
                self.z = FT.norm(nmod, self.y, dt, act=cc.act, res=res, sole_reader=sole_reader, res_post=cc.res_post)
            self.z.t.backward(self.dz, retain_graph=True)
            torch.cuda.synchronize()
        self.conv, self.norm = self.tape.of("conv")[0], self.tape.of("norm")[0]

    def want_labels(self):
        lab = {"norm:fold", "conv:prescaled"} if self.fold else {"norm:plain", "conv:rowscale"}
        return tuple(sorted(lab | ({"norm:res_post"} if self.cc.res_post else set())))

    def check(self):
        """labels, wiring, the convolution's exact output, the norm against float64 of that x, the recorded gradient against fold_ref,
        dX / dW / dbias against float64 from the recorded gradient.  Returns the worst figures."""
        cc, dt, tdt, o = self.cc, self.dt, self.tdt, dict(self.o)
        case, ops_ = cc.conv, self.ops
        N, S, C, G = chain_geometry(cc)
        what = f"chain {cc.name} {dt} {'fold' if self.fold else 'plain'}"
        figs = {}
        assert self.tape.taken() == self.want_labels(), f"{what}: took {self.tape.taken()}, expected {self.want_labels()}"
        assert_cl_equal(self.conv.out.t, ops_.y, what + ": convolution output")
        assert_fed_by(self.norm, "x", self.conv, what)
        fc, bc = chain_fwd_case(cc), chain_bwd_case(cc)
        z = self.norm.out.t
        assert z.shape[1] == C
        ref_f = NX.fwd_ref(fc, o)
        figs["y"] = NX.assert_units(what + " norm y", z.reshape(N, S, C), ref_f["y"], ref_f["mag"], chain_norm_bound(cc.name, dt, "y"), tdt)
        o["y"] = z.reshape(N, S, C).to(F64)
        ref = NX.bwd_ref(bc, o)
        _, mag = NX.bwd_restated(bc, o, F64)
        if cc.kind == "group":
            for k, p in (("dgamma", self.nmod.weight), ("dbeta", self.nmod.bias)):
                figs[k] = NX.assert_units(f"{what} {k}", p.grad.cpu(), ref[k], mag[k], chain_norm_bound(cc.name, dt, k))
        if cc.res_post:
            assert_same(self.res_t.grad.cpu(), self.dz.cpu(), what + ": dres is the incoming gradient")
        g = self.conv.g_out[0].t                            # what arrived at the convolution's output
        assert g.dtype == tdt and tuple(g.shape) == (N * S, C)
        B, bf = chain_norm_bound(cc.name, dt, "dx"), tdt == torch.bfloat16
        sc = torch.tensor(o["scales"], dtype=F64).repeat_interleave(N // case.frames).view(N, 1, 1)
        if self.fold:                                       # the rule of test_groupnorm_backward: round(dx) / sigma_t
            fr = NX.fold_ref(bc, o, ref["dx"], scales=o["scales"])
            err = (g.reshape(N, S, C).to(F64) - fr["dx"]).abs() - (2.0 * NX.ulp_bf16(fr["dx"]) if bf else 0.0)
            figs["g"] = float((err.clamp(min=0) / NX.ulp_f32(mag["dx"] * fr["sc"])).max())
            assert figs["g"] <= B, (what, "recorded gradient = round(dx) / sigma_t", figs["g"], B)
            dY = g.reshape(N, S, C).to(F64) / sc            # sigma_t is a power of two: round(dx) itself
        else:
            figs["g"] = NX.assert_units(what + " dx of the norm", g.reshape(N, S, C), ref["dx"], mag["dx"], B, tdt)
            dY = g.reshape(N, S, C).to(F64)
        cref = conv_from_gradient(case, ops_, to_maps(dY, case.odhw()))
        got = dict(dx=None if self.x_t.grad is None else self.x_t.grad.cpu(), dw=A.weight_of(self.mod).grad, db=None if not case.bias else self.mod.bias.grad)
        if got["dx"] is not None:
            assert got["dx"].shape == self.x_t.shape and bool((got["dx"][:, case.cin:] == 0).all()), what + ": dX pitch / padding"
            figs["dx"] = assert_units32(what + " dX", got["dx"][:, :case.cin].reshape(case.N, -1, case.cin), to_rows(cref["dx"]), to_rows(cref["S_dx"]),
                                        chain_bound(cc.name, dt, "dx"), tdt)
        if got["dw"] is not None:
            dw = got["dw"].cpu().unsqueeze(2)
            figs["dw"] = assert_units32(what + " dW", dw, cref["dw"], cref["S_dw"], chain_bound(cc.name, dt, "dw"))
        if got["db"] is not None:
            figs["db"] = assert_units32(what + " dbias", got["db"].cpu(), cref["db"], cref["S_db"], chain_bound(cc.name, dt, "db"))
        self.g = g
        return figs


# ====================================================================== ConvGRU
GRU_GEOMS = [(2, 3, 2, 32), (1, 1, 1, 16)]          # (B, T, L, C) at 8 x 8


def gru_case(B, T, L, C, dt):
    return GX.Case(B, T, L, C, C, 8, 8, dt, 0, False, 0)


def gru_module(c, ops_):
    """a first_stage.ConvGRU holding the operand set's weights: w_ur = update | reset (update first)"""
    rnn = FS.ConvGRU(c.Cx, c.Ch, 3, c.L, dtype=c.dt).to(DEV)
    with torch.no_grad():
        for l, cell in enumerate(rnn.cells):
            w_ur, b_ur, w_o, b_o = (t.to(F32).to(DEV) for t in ops_["w"][4 * l:4 * l + 4])
            cell.update_gate.weight.copy_(w_ur[:c.Ch]); cell.reset_gate.weight.copy_(w_ur[c.Ch:])
            cell.update_gate.bias.copy_(b_ur[:c.Ch]); cell.reset_gate.bias.copy_(b_ur[c.Ch:])
            cell.out_gate.weight.copy_(w_o); cell.out_gate.bias.copy_(b_o)
    return rnn


def gru_run(c, ops_, rnn, native, ld_extra=0, dout_mode="cl"):
    """forward and backward of the ConvGRU as first_stage_forward_loss drives it: ``gru_unroll`` (native) or the ``gru_cell`` loop.
    Returns (out [T * M, ld], x0 leaf, h0 leaf, tape).  dout_mode: "cl" | "f32" | "slice" (a column slice of a wider buffer)"""
    code, tdt, e = DTYPES[c.dt]
    for p in rnn.parameters():
        p.grad = None
    x0 = cl_dev(ops_["x0"], c.Cx, c.Cx + ld_extra, tdt, 0.0, True)
    h0 = cl_dev(ops_["h0"], c.Ch, c.Ch + ld_extra, tdt, 0.0, True)
    xin, h = K.CL(x0, c.B, (1, c.H, c.W), c.Cx), K.CL(h0, c.B, (1, c.H, c.W), c.Ch)
    with Tape() as tape:
        if native:
            assert FT.gru_native_ok(rnn, xin, h, c.dt)
            out = FT.gru_unroll(rnn, xin, h, c.T, c.dt).t
        else:
            hidden, outs = [h] * c.L, []
            for _ in range(c.T):
                x, new = xin, []
                for cell, hh in zip(rnn.cells, hidden):
                    x = FT.gru_cell(cell, x, hh, c.dt)
                    new.append(x)
                hidden = new
                outs.append(x.t)
            out = torch.cat(outs, 0)
        d = ops_["dout"].reshape(c.T * c.M, c.Ch)
        if dout_mode == "f32":
            dout = d.to(tdt).to(F32).to(DEV)
        elif dout_mode == "slice":
            wide = torch.full((d.shape[0], 2 * out.shape[1] + 8), SENT, dtype=tdt)
            wide[:, 8:8 + c.Ch] = d.to(tdt)
            wide[:, 8 + c.Ch:8 + out.shape[1]] = 0
            dout = wide.to(DEV)[:, 8:8 + out.shape[1]]
        else:
            dout = cl_dev(d, c.Ch, out.shape[1], tdt)
        out.backward(dout)
        torch.cuda.synchronize()
    return out.detach(), x0, h0, tape


def gru_grads(rnn):
    """the parameter gradients in gru_exact's order: per cell dw_ur (update | reset), db_ur, dw_o, db_o"""
    out = []
    for cell in rnn.cells:
        g = lambda p: torch.zeros_like(p) if p.grad is None else p.grad          # noqa: E731
        out += [torch.cat([g(cell.update_gate.weight), g(cell.reset_gate.weight)], 0), torch.cat([g(cell.update_gate.bias), g(cell.reset_gate.bias)]),
                g(cell.out_gate.weight), g(cell.out_gate.bias)]
    return [t.detach().cpu() for t in out]


def gru_direct(c, ops_, rnn, x0, h0, dout):
    """``ipoke_gru_unroll_forward`` / ``_backward`` called directly on the same buffers: (out, dx0 [M, Cx] f32, dh0 [M, Ch] f32, dws)"""
    code, tdt, e = DTYPES[c.dt]
    lib = _lib.lib()
    d = c.desc()
    ws = torch.empty(int(lib.ipoke_gru_workspace_bytes(ctypes.byref(d), code)), dtype=torch.uint8, device=DEV)
    weights = []
    for cell in rnn.cells:
        weights += [torch.cat([cell.update_gate.weight, cell.reset_gate.weight], 0), torch.cat([cell.update_gate.bias, cell.reset_gate.bias]),
                    cell.out_gate.weight, cell.out_gate.bias]
    w32 = [w.detach().float().contiguous() for w in weights]
    arr = (ctypes.c_void_p * len(w32))(*[w.data_ptr() for w in w32])
    ldo = K.round_up(c.Ch, e)
    out = torch.zeros(c.T * c.M, ldo, dtype=tdt, device=DEV)
    _lib.check(lib.ipoke_gru_unroll_forward(ctypes.byref(d), _lib.ptr(x0), x0.shape[1], _lib.ptr(h0), h0.shape[1], arr, _lib.ptr(ws), _lib.ptr(out), ldo,
                                            code, _lib.current_stream()))
    dws = [torch.empty(w.shape, dtype=F32, device=DEV) for w in w32]
    darr = (ctypes.c_void_p * len(dws))(*[w.data_ptr() for w in dws])
    dx0, dh0 = torch.empty(c.M, c.Cx, dtype=F32, device=DEV), torch.empty(c.M, c.Ch, dtype=F32, device=DEV)
    _lib.check(lib.ipoke_gru_unroll_backward(ctypes.byref(d), _lib.ptr(dout), ldo, _lib.ptr(ws), darr, _lib.ptr(dx0), _lib.ptr(dh0), code, _lib.current_stream()))
    torch.cuda.synchronize()
    return out, dx0, dh0, [t.cpu() for t in dws]


# ====================================================================== latent and loss ops
reparam_data = NX.reparam_data


def reparam_ref(mu, lv, eps, dz, dmu, dlv, f=F64):
    """(z, d mulv [M, 2Z], the magnitudes of both) in dtype f; an absent gradient is None"""
    mu, lv, eps = mu.to(f), lv.to(f), eps.to(f)
    zero = torch.zeros_like(mu)
    dz, dmu, dlv = (zero if v is None else v.to(f) for v in (dz, dmu, dlv))
    sig = torch.exp(0.5 * lv)
    chain = dz * eps * 0.5 * sig
    return (mu + eps * sig, torch.cat([dz + dmu, dlv + chain], 1), mu.abs() + (eps * sig).abs(),
            torch.cat([dz.abs() + dmu.abs(), dlv.abs() + chain.abs()], 1))


def l1_data(B, T, C, H, W, seed):
    """a clip X [B, T, C, H, W] in [-1, 1] (fp32 values), the decoder's pre-tanh rows [(T - 1) B H W, C] in (frame, clip) order, an fp32
    d_frame of the same shape; float64"""
    gen = torch.Generator().manual_seed(seed)
    X = NX.rnd(torch.rand((B, T, C, H, W), generator=gen, dtype=F64) * 2.0 - 1.0, F32)
    M = (T - 1) * B * H * W
    pre = NX.rnd(torch.randn((M, C), generator=gen, dtype=F64) * 1.5, F32)
    d_frame = NX.rnd(torch.randn((M, C), generator=gen, dtype=F64) * 0.01, F32)
    return X, pre, d_frame


def l1_targets_rows(X):
    """the targets of the (frame, clip)-ordered batch as channels-last rows [(T - 1) B H W, C], stated index by index"""
    B, T, C, H, W = X.shape
    out = torch.empty(((T - 1) * B * H * W, C), dtype=X.dtype)
    for t in range(1, T):
        for b in range(B):
            r0 = ((t - 1) * B + b) * H * W
            out[r0:r0 + H * W] = X[b, t].reshape(C, H * W).t()
    return out


def l1_ref(frame, tgt_rows, scale, d_loss, d_frame, f=F64):
    """from the STORED frame = tanh(pre): (loss, d pre, S of the loss, magnitude of d pre) in dtype f"""
    frame, tgt, scale = frame.to(f), tgt_rows.to(f), torch.tensor(scale, dtype=F32).to(f)
    diff = frame - tgt
    loss = scale * diff.abs().sum()
    up = scale * torch.sign(diff) * torch.tensor(d_loss, dtype=F32).to(f)
    d = up if d_frame is None else up + d_frame.to(f)
    mag = up.abs() + (0 if d_frame is None else d_frame.to(f).abs())
    return loss, d * (1.0 - frame * frame), scale * (frame.abs() + tgt.abs()).sum(), mag * (1.0 + frame * frame)


# ====================================================================== the fold predicate against the kernel's requirement
def kernel_accepts_fold(N, S, C, frames, mod, dt, res_post):
    """the IPK_REQUIREs of ipoke_groupnorm_bwd on the folded path (csrc/vae_bwd.hip), restated: channels and pitches in 16-byte units, no
    modulation, whole frames, C <= 2048, and the apply pass's per-channel constants (6 C floats, 8 C with act_from_pre) plus the fold's
    256 x 16 bytes + 4 floats within 64 KB of LDS.  The pitch of x is C here (what the predicate demands)."""
    e = DTYPES[dt][2]
    if C % e or C > 4096 or mod or N % frames:
        return False
    rows = (N // frames) * S
    if rows < S or rows % S or (N * S) % rows or C > 2048:
        return False
    return 4 * ((8 if res_post else 6) * C + 256 * e + 4) <= 64 * 1024


def predicate_accepts_fold(N, S, C, frames, mod, dt, res_post, ld=None):
    """``FT._rowscale_producer`` on a CL of that geometry (CPU tensors of no size: nothing is read)"""
    tdt, e = DTYPES[dt][1], DTYPES[dt][2]
    ld = K.round_up(C, e) if ld is None else ld
    x = K.CL(torch.empty(0, ld, dtype=tdt), N, (1, 1, S), C)
    x.conv_meta = dict(sn_frames=(torch.empty(frames, 2), torch.empty(frames, 1)), act=NONE, out_f32=False)
    m = None if not mod else (K.CL(torch.empty(0, ld, dtype=tdt), N, (1, 1, S), C),) * 2
    return FT._rowscale_producer(x, m, dt, res_post) is not None


# ====================================================================== res_block: the route whose sum rides on the skip path's norm
def load_int_sn(conv_mod, seed, sigma=2.0):
    """small integer weights and bias, one-hot u / v on an entry holding ``sigma``: the spectral norm divides by a power of two"""
    gen = torch.Generator().manual_seed(seed)
    w = CX.int_operand(tuple(A.weight_of(conv_mod).shape), 2, gen)
    m = w.reshape(w.shape[0], -1)
    i, j = 3 % m.shape[0], 7 % m.shape[1]
    m[i, j] = sigma
    with torch.no_grad():
        A.weight_of(conv_mod).copy_(m.reshape(w.shape).to(F32))
        if conv_mod.bias is not None:
            conv_mod.bias.copy_(CX.int_operand((conv_mod.cout,), 4, gen, 0.1).to(F32))
    set_one_hot(conv_mod, (i, j))


def run_res_block_post(dt, frames):
    """``res_block`` on ResBlock(8 -> 16, no norm on the main path, InstanceNorm + ReLU on the convolved skip): out = conv2(conv1(x)) +
    relu(norm(res_conv(x))).  Returns (tape, x leaf, block, dy)"""
    code, tdt, e = DTYPES[dt]
    blk = FS.ResBlock(8, 16, norm="none", activation="relu", snorm=True).to(DEV)
    for k, m in enumerate((blk.conv1.conv, blk.conv2.conv, blk.res_conv.conv)):
        load_int_sn(m, 40 + k)
    N, H, W = 2 * frames, 6, 7
    gen = torch.Generator().manual_seed(9)
    x = cl_dev(CX.int_operand((N * H * W, 8), 2, gen), 8, 8, tdt, 0.0, True)
    dy = cl_dev(randint64(-4, 4, (N * H * W, 16), gen), 16, 16, tdt)
    with Tape() as tape:
        out = FST.res_block(blk, K.CL(x, N, (1, H, W), 8), dt, pit=False, frames=frames)
        out.t.backward(dy)
        torch.cuda.synchronize()
    return tape, x, blk, dy, out


# ====================================================================== the inference twin: chunk statistics handed to the next norm
# producer: an InstanceNorm with ELU and a residual behind it that offers ``next_groups``; consumer: a SPADE norm of ``groups`` groups
Handover = collections.namedtuple("Handover", "name C next_groups groups part")
HANDOVERS = [
    Handover("taken", 32, 16, 16, True),                   # the consumer's group count is the handed one
    Handover("other-count", 32, 16, 8, False),             # it differs: the hand-over must be ignored
    Handover("not-offered", 24, 16, 12, False),            # C is no multiple of next_groups: nothing is offered
]


def run_handover(h, dt, N=2, S=300):
    """producer -> consumer through ``K.group_norm``; returns (labels, consumer case, consumer operands as the kernel read them, y)"""
    code, tdt, e = DTYPES[dt]
    gen = torch.Generator().manual_seed(NX.seed_of("handover-" + h.name))
    r = lambda shape, s=1.0, off=0.0: NX.rnd(torch.randn(shape, generator=gen, dtype=F64) * s + off, tdt)      # noqa: E731
    x, res, mg, mb = r((N, S, h.C), 2.0, 0.7), r((N, S, h.C), 0.7, 1.0), r((N, S, h.C), 0.5), r((N, S, h.C), 0.5)
    dhw = (1, 1, S)
    cl = lambda v: K.CL(cl_dev(v, h.C, h.C, tdt), N, dhw, h.C)      # noqa: E731
    with Tape() as tape, torch.no_grad():
        p = K.group_norm(cl(x), h.C, dt, act=ELU, res=cl(res), res_post=True, next_groups=h.next_groups)
        offered = getattr(p, "stats_part", None) is not None
        stored = p.t.detach().cpu().reshape(N, S, h.C).to(F64)
        y = K.group_norm(p, h.groups, dt, mod=(cl(mg), cl(mb)))
        torch.cuda.synchronize()
    c = NX._c("handover-" + h.name, N, S, h.C, h.groups, False, NONE, None, -1)
    return tape.taken("norm:"), offered, c, dict(x=stored, gamma=None, beta=None, mg=mg, mb=mb, res=None), y.t.detach().cpu().reshape(N, S, h.C)


# ====================================================================== per-op checks on what the tape recorded
def _rec_case(r, name, res_kind):
    o = r.opts
    mod = 0 if "mg" not in r.ins else (-1 if o.get("mod_N", o["N"]) == o["N"] else o["mod_N"])
    return NX._c(name, o["N"], o["S"], o["C"], o["groups"], r.gamma is not None, o["act"], res_kind, mod)


def _rec_inputs(r):
    o = r.opts
    N, S, C = o["N"], o["S"], o["C"]
    rows = lambda k: None if k not in r.ins else r.ins[k].t[:, :C].reshape(-1, S, C).to(F64)      # noqa: E731
    vec = lambda p: None if p is None else p.detach().cpu().to(F64)                                # noqa: E731
    return dict(x=rows("x"), res=rows("res"), mg=rows("mg"), mb=rows("mb"), gamma=vec(r.gamma), beta=vec(r.beta))


def check_norm_record(r, dt, what, folded=False):
    """a taped norm (training op or ``K.group_norm``) against float64 of its own recorded inputs and -- where a gradient arrived -- of its
    own recorded incoming gradient; dx of a folded norm leaves scaled and is held by the chains.  Returns (figures, magnitudes)"""
    tdt = DTYPES[dt][1]
    o = r.opts
    N, S, C = o["N"], o["S"], o["C"]
    res_kind = None if "res" not in r.ins else ("post" if o["res_post"] else "pre")
    c, inp = _rec_case(r, what, res_kind), _rec_inputs(r)
    ref = NX.fwd_ref(c, inp)
    y = r.out.t[:, :C].reshape(N, S, C)
    # the operands are whatever the block produced, not norm_exact's centred family: where the fp32 restatement on THESE operands is worse
    # than the recorded centred yardstick, the bound comes from its figure here (capped), as for a chain that exceeds the table
    yard = NX.worst(NX.fwd_ref(c, inp, F32)["y"], ref["y"], ref["mag"])
    assert yard <= NX.YARDSTICK_CAP, (what, yard)
    figs = dict(yard_y=yard, y=NX.assert_units(what + " y", y, ref["y"], ref["mag"], max(NX.gpu_bound("y", "centred", dt), 4.0 * yard), tdt))
    assert bool((r.out.t[:, C:] == 0).all()) or r.kind == "knorm", what + ": padding columns of y"
    if 0 not in r.g_out:
        return figs, None
    summed = c.mod > 0
    bc = NX.BwdCase(what, N, S, C, o["groups"], c.affine, o["act"], res_kind == "pre", c.mod, True, res_kind == "post", summed, None)
    inp["y"], inp["dy"] = y.to(F64), r.g_out[0].t[:, :C].reshape(N, S, C).to(F64)
    bref = NX.bwd_ref(bc, inp)
    _, mag = NX.bwd_restated(bc, inp, F64)
    for k, name in (("dx", "x"), ("dres", "res"), ("dmg", "mg"), ("dmb", "mb")):
        if name not in r.g_in or (k == "dx" and folded):
            continue
        got = r.g_in[name].t
        if k == "dres" and res_kind == "post":
            assert_same(got, r.g_out[0].t, what + ": dres is the incoming gradient")
            continue
        assert bool((got[:, C:] == 0).all()), f"{what}: padding columns of {k}"
        figs[k] = NX.assert_units(f"{what} {k}", got[:, :C].reshape(-1, S, C), bref[k], mag[k], NX.bwd_bound(k, dt), tdt)
    return figs, mag


def check_add_act_record(r, dt, what):
    """y = RNE(act(a + b)) and both gradients = g act'(y), bit for bit, from the recorded operands (ReLU or no activation)"""
    tdt, C = DTYPES[dt][1], r.opts["C"]
    assert r.opts["act"] in (NONE, RELU)
    s = r.ins["a"].t[:, :C].to(F64) + r.ins["b"].t[:, :C].to(F64)
    y = torch.relu(s) if r.opts["act"] == RELU else s
    assert_same(r.out.t[:, :C].contiguous(), rne(y, tdt), what + " y")
    g = r.g_out[0].t[:, :C].to(F64) * ((r.out.t[:, :C] > 0).to(F64) if r.opts["act"] == RELU else 1.0)
    for k in ("a", "b"):
        assert_same(r.g_in[k].t[:, :C].contiguous(), rne(g, tdt), f"{what} gradient of {k}")
        assert bool((r.g_in[k].t[:, C:] == 0).all())


def assert_two_readers(leaf_grad, r1, n1, r2, n2, dt, what):
    assert r1.ins[n1].ptr == r2.ins[n2].ptr, what + ": the two ops do not read one tensor"
    assert_sum_of_two(leaf_grad, r1.g_in[n1].t, r2.g_in[n2].t, DTYPES[dt][1], what)


def int_cl(shape_rows, C, lim, seed, tdt, grad=True):
    gen = torch.Generator().manual_seed(seed)
    v = CX.int_operand((shape_rows, C), lim, gen)
    return v, cl_dev(v, C, C, tdt, 0.0, grad)


def real_cl(rows, C, seed, tdt, grad=True, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    v = NX.rnd(torch.randn((rows, C), generator=gen, dtype=F64) * scale, tdt)
    return v, cl_dev(v, C, C, tdt, 0.0, grad)


# ---- conv_block without a norm: the activation in the convolution, a residual through add_act, an fp32 output
def conv_block_plain(mode, dt):
    """``conv_block`` on a Conv2dBlock without norm holding exact operands (autograd_exact's c2d cases): mode "act" (ReLU inside the
    convolution), "res" (-> add_act with ReLU), "f32" (out_f32: the block's tanh is left to the loss kernel).  Everything is an
    integer, every result compared with ==.  Returns the tape."""
    tdt = DTYPES[dt][1]
    case = A.BY_NAME["c2d_relu_bias_cl" if mode == "act" else "c2d_3x3_s1_bias"]
    ops_ = A.operands(case)
    blk = FS.Conv2dBlock(case.cin, case.cout, 3, 1, 1, norm="none", activation="tanh" if mode == "f32" else "relu").to(DEV)
    A.load_operands(blk.conv, ops_)
    x_t = cl_of(ops_.x, dt).to(DEV).requires_grad_(True)
    x = K.CL(x_t, case.N, case.ext, case.cin)
    gen = torch.Generator().manual_seed(21)
    res64 = CX.int_operand(tuple(ops_.y.shape), 3, gen)
    res_t = cl_of(res64, dt).to(DEV).requires_grad_(True) if mode == "res" else None
    with Tape() as tape:
        out = FST.conv_block(blk, x, dt, res=None if res_t is None else K.CL(res_t, case.N, case.odhw(), case.cout), out_f32=mode == "f32")
        dy = ops_.dy.permute(0, 2, 3, 4, 1).reshape(-1, case.cout).to(F32).to(DEV) if mode == "f32" else cl_of(ops_.dy, dt).to(DEV)
        out.t.backward(dy)
        torch.cuda.synchronize()
    xr = ops_.x.clone().requires_grad_(True)
    w5 = ops_.w5.clone().requires_grad_(True)
    b = ops_.b.clone().requires_grad_(True)
    y = ops_.forward64(xr, w5, b)
    rr = None
    if mode == "res":
        rr = res64.clone().requires_grad_(True)
        y = y + (rne(y.detach(), tdt).to(F64) - y.detach())          # add_act reads the convolution's STORED output
        y = torch.relu(y + rr)
    y.backward(ops_.dy)
    what = f"conv_block {mode} {dt}"
    if mode == "f32":
        assert out.t.dtype == F32 and tuple(out.t.shape) == (y.numel() // case.cout, case.cout)
        A.assert_tensor_equal(out.t, y.detach().permute(0, 2, 3, 4, 1).reshape(-1, case.cout), what + " y")
    else:
        assert_cl_equal(out.t, y.detach(), what + " y")
    assert_cl_equal(x_t.grad, xr.grad, what + " dX")
    A.assert_tensor_equal(blk.conv.weight.grad, w5.grad.squeeze(2), what + " dW")
    A.assert_tensor_equal(blk.conv.bias.grad, b.grad, what + " dbias")
    if mode == "res":
        assert_cl_equal(res_t.grad, rr.grad, what + " dres")
    return tape


# ---- res_block: identity skip, convolved skip without a norm
def run_res_block(route, dt, frames):
    """route "identity": ResBlock(16 -> 16, InstanceNorm, ELU): x is conv1's input and the residual of conv2's norm.  route "no-norm":
    ResBlock(8 -> 16) without any norm (the skip's norm taken out): the sum is an ``add_act`` without activation.  Returns (tape, x, blk)"""
    tdt = DTYPES[dt][1]
    if route == "identity":
        blk = FS.ResBlock(16, 16, norm="in", activation="elu", snorm=True).to(DEV)
        cin = 16
    else:
        blk = FS.ResBlock(8, 16, norm="none", activation="relu", snorm=True)
        blk.res_conv.norm = None
        blk, cin = blk.to(DEV), 8
    mods = [blk.conv1.conv, blk.conv2.conv] + ([blk.res_conv.conv] if blk.convolve_res else [])
    for k, m in enumerate(mods):
        load_int_sn(m, 60 + k)
    N, H, W = 2 * frames, 6, 7
    _, x = int_cl(N * H * W, cin, 2, 11, tdt)
    _, dy = int_cl(N * H * W, 16, 4, 12, tdt, grad=False)
    with Tape() as tape:
        out = FST.res_block(blk, K.CL(x, N, (1, H, W), cin), dt, pit=False, frames=frames)
        out.t.backward(dy)
        torch.cuda.synchronize()
    return tape, x, blk, out


# ---- basic_block: 3-D, with a downsample
def run_basic_block(dt):
    tdt = DTYPES[dt][1]
    torch.manual_seed(3)
    blk = FS.BasicBlock(16, 32, stride=(1, 2, 2)).to(DEV)
    with torch.no_grad():
        for nm in (blk.bn1, blk.bn2, blk.downsample[1]):
            nm.weight.copy_(1.0 + 0.3 * torch.randn(32)); nm.bias.copy_(0.2 * torch.randn(32))
    N, dhw = 2, (3, 6, 8)
    _, x = real_cl(N * 3 * 6 * 8, 16, 13, tdt)
    with Tape() as tape:
        out = FST.basic_block(blk, K.CL(x, N, dhw, 16), dt)
        _, dy = int_cl(out.t.shape[0], 32, 4, 14, tdt, grad=False)
        out.t.backward(dy)
        torch.cuda.synchronize()
    return tape, x, blk, out


# ---- spade_modulation -> group_norm(mod=...)
def run_spade(dt, frames, shared):
    """the SPADE maps of two clips' start frames feeding ``group_norm(mod=...)`` on frames x 2 samples ordered (frame, clip): shared (the
    maps' CLs as they are: mod_samples) or repeated per sample by hand.  Returns (tape, the norm's record, Spade module)"""
    tdt = DTYPES[dt][1]
    torch.manual_seed(5)
    sp = FS.Spade(32).to(DEV)
    gen = torch.Generator().manual_seed(17)
    y0 = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
    N, S, C = 2 * frames, 64, 32
    _, x = real_cl(N * S, C, 18, tdt, scale=2.0)
    _, dy = int_cl(N * S, C, 4, 19, tdt, grad=False)
    with Tape() as tape:
        mg, mb = FST.spade_modulation(sp, y0, (8, 8), dt)
        if not shared and frames > 1:
            mg, mb = (K.CL(m.t.repeat(frames, 1), N, m.dhw, m.C) for m in (mg, mb))
        out = FT.group_norm(K.CL(x, N, (1, 8, 8), C), sp.groups, dt, mod=(mg, mb))
        out.t.backward(dy)
        torch.cuda.synchronize()
    return tape, tape.of("norm")[0], sp


# ---- decode_frame
def run_decode_frame(dt, frames):
    tdt = DTYPES[dt][1]
    torch.manual_seed(7)
    gen_ = FS.SpadeCondConvDecoder(dict(dec_channels=(16, 8), spectral_norm=True, norm="in", z_dim=8), dtype=dt).to(DEV)
    g = torch.Generator().manual_seed(23)
    y0 = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(DEV)
    N = 2 * frames
    _, h = real_cl(N * 64, 8, 24, tdt)
    with Tape() as tape:
        mods = FST.spade_modulations(gen_, y0, dt)
        pre = FST.decode_frame(gen_, K.CL(h, N, (1, 8, 8), 8), y0, dt, False, mods, frames=frames)
        dy = NX.rnd(torch.randn(tuple(pre.t.shape), generator=g, dtype=F64), F32).to(F32).to(DEV)
        pre.t.backward(dy)
        torch.cuda.synchronize()
    return tape, h, gen_, pre


# ---- the inference twin through the real run methods
RUN_HANDOVERS = [("taken", 32, None, True), ("other-count", 32, 8, False), ("not-offered", 24, 16, False)]          # name, C, next_groups (None: Spade's own), part


def run_handover_modules(name, dt):
    """``ResBlock.run(next_groups=...)`` -> ``Spade.run``: returns (tape, producer record, consumer record, offered?)"""
    _, C, ng, _ = next(h for h in RUN_HANDOVERS if h[0] == name)
    tdt = DTYPES[dt][1]
    torch.manual_seed(9)
    blk, sp = FS.ResBlock(16, C, norm="none", upsampling=True).to(DEV), FS.Spade(C).to(DEV)
    N, S = 2, 400
    _, x = real_cl(N * 100, 16, 31, tdt, grad=False)
    _, mg = real_cl(N * S, C, 32, tdt, grad=False, scale=0.5)
    _, mb = real_cl(N * S, C, 33, tdt, grad=False, scale=0.5)
    mod = (K.CL(mg, N, (1, 20, 20), C), K.CL(mb, N, (1, 20, 20), C))
    with Tape() as tape, torch.no_grad():
        mid = blk.run(K.CL(x, N, (1, 10, 10), 16), dt, next_groups=sp.groups if ng is None else ng)
        offered = getattr(mid, "stats_part", None) is not None
        sp.run(mid, mod, dt)
        torch.cuda.synchronize()
    prod, cons = tape.of("knorm")
    return tape, prod, cons, offered, sp
