"""The differentiable HIP ops every trained model is built from (the first-stage VAE, the discriminators, the VGG features, the
2-D autoencoders): each is a ``torch.autograd.Function`` whose forward *and* backward are HIP kernels of libipoke_hip on
channels-last activations, over the parameter holders of ``ipoke_amd.first_stage`` (``_Conv``, ``_Norm``, ``ConvGRUCell``) --

    convolution         ipoke_conv_forward  | data gradient: the transposed (direct) convolution with the same weights
                                            | weight gradient: ipoke_conv_wgrad, written in PyTorch layout
                                            | bias gradient: ipoke_colsum, fused activation: ipoke_act_bwd
    Group/Instance/SPADE ipoke_groupnorm    | ipoke_groupnorm_bwd
    ConvGRU gates        ipoke_gru_*        | ipoke_gru_*_bwd
    reparameterize       ipoke_reparameterize | ipoke_reparam_bwd
    tanh + L1            ipoke_l1_loss (value and gradient in one pass)

    spectral norm        ipoke_spectral_sigma (power iteration + sigma) | ipoke_spectral_bwd; 1/sigma is folded into
                         ipoke_conv_weight_operand (fp32 PyTorch-layout weight -> matrix-core operand, one launch)
    KL                   ipoke_kl_loss (value and gradient in one pass)
    Adam                 ipoke_adam_multi (multi-tensor, torch.optim.Adam semantics)

PyTorch autograd only records the graph.  ``conv_weight`` is the convolution on a bare weight tensor, ``conv`` the same on a
``first_stage._Conv`` module, whose weight ``effective_weight`` hands out: the plain parameter, a ``_SnWeight`` (spectral norm, 1 / sigma
folded into the operand) or a ``_SnFrames`` (one operand of W_orig for a (frame, clip)-ordered batch, 1 / sigma_t as a per-image scale of
the GEMM epilogue; see ``ipoke_amd.first_stage_train``).  ``MultiTensorAdam`` lives here because it writes the parameters behind the
operand cache and has to clear it.
"""
import ctypes
import weakref
from ctypes import byref

import torch

from . import _lib, nn as K, ops
from . import first_stage as FS
from ._lib import NormBwdDesc, NormDesc, WgradDesc, check, ptr

_ws = {}


def _workspace(n_floats, device, tag):
    buf = _ws.get((tag, device))
    if buf is None or buf.numel() < n_floats:
        buf = torch.empty(max(int(n_floats), 1 << 16), dtype=torch.float32, device=device)
        _ws[(tag, device)] = buf
    return buf


def _tdt(dtype):
    return ops.torch_dtype(dtype)


def pad_cols(t, ld, dtype):
    """[M, C] (any float dtype) -> compute dtype [M, ld], zero padded."""
    if t.shape[1] == ld and t.dtype == _tdt(dtype):
        return t.contiguous()
    out = torch.zeros(t.shape[0], ld, dtype=_tdt(dtype), device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _fit_cols(g, ld, dtype):
    """A gradient [M, any pitch] for an input of pitch ``ld``: ``g`` itself where it fits, else its columns cut or zero padded."""
    if g.shape[1] == ld and g.dtype == _tdt(dtype):
        return g
    return pad_cols(g[:, :min(g.shape[1], ld)], ld, dtype)


def _matrix_geometry(w, transposed):
    """(rows, cols, taps) of a conv weight -- a tensor or its shape -- read as the matrix [rows][cols * taps]; ``transposed``: ConvTranspose
    storage [in][out][k]."""
    shape = getattr(w, "shape", w)
    taps = 1
    for k in shape[2:]:
        taps *= int(k)
    rows, cols = (shape[1], shape[0]) if transposed else (shape[0], shape[1])
    return int(rows), int(cols), taps


_OPCACHE = {}
_FWD_EPOCH = [0]      # forward passes so far: scopes cached operands of per-pass temporaries (the concatenated GRU gate weights)


def begin_forward_pass():
    """A new forward pass of a graph that shares derived weights among its steps (``gru_cell``'s ``gate_w``): a new operand scope."""
    _FWD_EPOCH[0] += 1
    if len(_OPCACHE) > 4096:
        clear_operand_cache()                      # scoped entries of passes whose backward never ran


def clear_operand_cache():
    """Called whenever parameters change behind autograd's back (MultiTensorAdam writes through raw pointers)."""
    _OPCACHE.clear()


def take_operand_cache():
    """Detach the cache's entries (ahead of an optimizer step that would drop them): ``refresh_operand_cache`` brings them back."""
    snap = dict(_OPCACHE)
    _OPCACHE.clear()
    return snap


def refresh_operand_cache(snap):
    """Behind an optimizer step that wrote the parameters through raw pointers (no version bump): rebuild the cached operands of every
    live PARAMETER in place -- same tensors, same cache keys -- with ONE multi-tensor launch, instead of dropping them and rebuilding
    each lazily at its first use (c4: 101 launches of ~8 us on the chain per step, 41.96 -> 41.43 ms).  Entries of derived weights (scoped: the per-pass
    GRU gate concatenations), of other streams and of dead or re-versioned tensors are dropped as before."""
    cur = torch.cuda.current_stream().cuda_stream
    by_dtype = {}
    for key, (wref, (out, kc)) in snap.items():
        p_, ver, shape, transposed, dtype, stream, scope = key
        owner = wref()
        if (owner is None or scope is not None or stream != cur or not isinstance(owner, torch.nn.Parameter) or owner.data_ptr() != p_
                or owner._version != ver or tuple(owner.shape) != shape or not owner.is_contiguous() or owner.dtype != torch.float32):
            continue
        by_dtype.setdefault(dtype, []).append((owner, out, _matrix_geometry(shape, transposed) + (int(bool(transposed)), int(kc)), key))
    for dtype, jobs in by_dtype.items():
        n = len(jobs)
        wp = (ctypes.c_void_p * n)(*[j[0].data_ptr() for j in jobs])
        op = (ctypes.c_void_p * n)(*[j[1].data_ptr() for j in jobs])
        dims = (ctypes.c_int32 * (5 * n))(*[v for j in jobs for v in j[2]])
        check(_lib.lib().ipoke_conv_weight_operand_multi(wp, op, dims, n, ops._dt(dtype), _lib.current_stream()))
        for owner, out, d, key in jobs:
            _OPCACHE[key] = snap[key]


def _weight_operand(w, dtype, transposed_conv, inv_scale=None, cacheable=False, scope=None, owner=None):
    """fp32 conv weight in PyTorch layout -> ([rows][taps*kc] operand of the compute dtype, kc); ``transposed_conv`` reads
    ConvTranspose storage [in][out][k] as the conv weight [out][in][k]; ``inv_scale``: device scalar (1/sigma).
    ``cacheable`` (module parameters without spectral norm: GRU, SPADE, VGG convolutions): the operand of a weight version is
    built once and reused by the 15 per-frame calls of a step and by the backward pass.  ``owner``: the tensor object the caller
    holds (``w`` itself may be a fresh ``detach()`` view); an entry is only valid while THAT object is alive -- a key made of the
    device address alone would hand a freed model's operand to whichever new tensor the allocator places there."""
    key = None
    owner = w if owner is None else owner
    if cacheable and inv_scale is None:
        key = (owner.data_ptr(), owner._version, tuple(w.shape), bool(transposed_conv), str(dtype), torch.cuda.current_stream().cuda_stream, scope)
        hit = _OPCACHE.get(key)
        if hit is not None:
            if hit[0]() is owner:
                return hit[1]
            del _OPCACHE[key]                      # the address was recycled by another tensor
    res = _build_weight_operand(w, dtype, transposed_conv, inv_scale)
    if key is not None:
        _OPCACHE[key] = (weakref.ref(owner), res)
    return res


def _build_weight_operand(w, dtype, transposed_conv, inv_scale=None):
    w = w.contiguous()
    rows, cols, taps = _matrix_geometry(w, transposed_conv)
    kc = K.round_up(cols, K.e16(dtype))
    out = torch.empty(rows, taps * kc, dtype=_tdt(dtype), device=w.device)
    check(_lib.lib().ipoke_conv_weight_operand(ptr(w), rows, cols, taps, int(bool(transposed_conv)),
                                               None if inv_scale is None else ptr(inv_scale), ptr(out), kc, ops._dt(dtype),
                                               _lib.current_stream()))
    return out, kc


_WGRAD_SWAP = True      # test hook (tests/test_vae_bwd_units_gpu.py): False = narrow-output convolutions' weight gradient without swapped roles (c4 48.5 vs 47.7 ms)
_WGRAD_HALO_WGS = 256   # workgroups the halo-staged weight gradient aims for (one per CU: 158 KB of LDS)
_WGRAD_WGS = 512        # workgroups a split-M weight gradient aims for (c4: 256 / 512 / 1024 / 2048 -> 156.5 / 151.0 / 156.5 / 160.6 ms: more slabs = more fp32 partial traffic)


class _SnWeight:
    """A spectral-normalised weight as the convolution consumes it: ``weight_orig`` plus the device-side {sigma, 1/sigma}
    and the u | v snapshot of this call (the buffers themselves move on with every later power iteration)."""

    def __init__(self, w_orig, sig, snap, transposed, mod):
        self.w_orig, self.sig, self.snap, self.transposed, self.mod = w_orig, sig, snap, transposed, mod


class _SnFrames:
    """A spectral-normalised weight for a batch of ``frames`` image groups ordered (frame, clip): ``weight_orig`` plus the tables of the
    frames' power iterations -- ``sig`` [frames, 2] = {sigma_t, 1 / sigma_t} and ``snaps`` [frames, rows + cols] = u_t | v_t
    (ipoke_spectral_sigma_multi).  frames = 1: one sigma for the whole batch (evaluation mode)."""

    def __init__(self, w_orig, sig, snaps, transposed, mod):
        self.w_orig, self.sig, self.snaps, self.transposed, self.mod = w_orig, sig, snaps, transposed, mod
        self.frames = int(sig.shape[0])


# taps (kh * 3 + kw) of the four sub-pixel phases (output parity (a, b): rows 2 i + a, columns 2 j + b), in the tap order of the
# stride-1 convolution that computes the phase (first_stage._Conv._phase_operands); the phases' first blocks are 0, 1, 3, 5
_CT_PERM = (4, 5, 3, 7, 1, 8, 6, 2, 0)
_CT_PHASE = {(0, 0): (0, 1), (0, 1): (1, 2), (1, 0): (3, 2), (1, 1): (5, 4)}
_ct_index = {}


def _conv_transpose_phases(x, wop, kc, cout, dt, bias, act, out_f32, row_scale=None):
    """Forward of a 3 x 3 / stride 2 / padding 1 / output_padding 1 ConvTranspose2d (util.py:52-55) from its [cout][9 * kc] operand:
    one gather puts the tap blocks in phase order, four stride-1 convolutions (1, 2, 2, 4 taps) write the four pixel parities."""
    idx = _ct_index.get(x.t.device)
    if idx is None:
        idx = _ct_index[x.t.device] = torch.tensor(_CT_PERM, device=x.t.device)
    wperm = wop.view(cout, 9, kc).index_select(1, idx).view(cout, 9 * kc)
    N, (_, Hi, Wi) = x.N, x.dhw
    Ho, Wo = 2 * Hi, 2 * Wi
    ldc = cout if out_f32 else K.round_up(cout, K.e16(dt))
    y = torch.empty(N * Ho * Wo, ldc, dtype=torch.float32 if out_f32 else _tdt(dt), device=x.t.device)
    for (a, b), (first, ntap) in _CT_PHASE.items():
        K.conv(x, wperm[:, first * kc:(first + ntap) * kc], kc, cout, (1, 1 + a, 1 + b), (1, 1, 1), (0, 0, 0), dt, bias=bias, act=act,
               out_f32=out_f32, out=y, odhw=(1, Hi, Wi), scatter=(Ho * Wo, 2 * Wo, 2, a * Wo + b), row_scale=row_scale)
    return K.CL(y, N, (1, Ho, Wo), cout)


_DG_PHASES = True       # test hook (tests/test_vae_bwd_units_gpu.py): False = strided 3 x 3 x 3 data gradients as one 27-tap launch (c4 48.0 vs 46.95 ms)
_dg_index = {}


def dgrad_phases_ok(k, st, pd, idhw, odhw):
    return (_DG_PHASES and tuple(k) == (3, 3, 3) and tuple(pd) == (1, 1, 1) and all(s_ in (1, 2) for s_ in st) and max(st) == 2
            and all(o == (i - 1) // s_ + 1 for i, o, s_ in zip(idhw, odhw, st)))


def _dgrad_phases(gcl, w, cin, idhw, st, dt):
    """Data gradient of a Conv3d(cin -> cout, 3, stride in {1, 2}^3, padding 1) (the 3-D encoder's layer transitions,
    motion_encoder.py:80-91): dX[i] = sum over (o, t) with o * s + t - 1 = i of W[:, :, t]^T dY[o].  Along a strided dimension an even
    position sees ONE tap (t = 1, o = i / 2) and an odd one TWO (t = 2 at o = (i - 1) / 2, t = 0 at o + 1); along an unstrided one all three
    (flipped).  One stride-1 convolution over dY per parity class, its taps a contiguous slice of ONE permuted operand, its outputs
    scattered to the class's positions (ipoke_conv_desc.c_scatter / c_sd) -- instead of 27 taps at every position of which 1 / 8 (or
    1 / 2) fall on a sample of dY."""
    N, odhw, cout = gcl.N, gcl.dhw, gcl.C
    kc = gcl.t.shape[1]
    sets = [([[2, 1, 0]] if s_ == 1 else [[1], [2, 0]]) for s_ in st]              # per dimension: taps of each parity class, in window order
    key = (w.device, tuple(st))
    plan = _dg_index.get(key)
    if plan is None:
        order, phases = [], []
        for rd, td in enumerate(sets[0]):
            for rh, th in enumerate(sets[1]):
                for rw, tw in enumerate(sets[2]):
                    phases.append(((rd, rh, rw), (len(td), len(th), len(tw)), len(order)))
                    order += [(a * 3 + b) * 3 + c for a in td for b in th for c in tw]
        plan = _dg_index[key] = (torch.tensor(order, device=w.device), phases)
    idx, phases = plan
    wt = w.detach().permute(1, 2, 3, 4, 0).reshape(cin, 27, cout)                      # [cin][tap][cout]
    wop = torch.zeros(cin, 27, kc, dtype=_tdt(dt), device=w.device) if kc != cout else torch.empty(cin, 27, kc, dtype=_tdt(dt), device=w.device)
    wop[:, :, :cout] = wt.index_select(1, idx)
    wop = wop.view(cin, 27 * kc)
    Di, Hi, Wi = idhw
    ld = K.round_up(cin, K.e16(dt))
    dx = torch.empty(N * Di * Hi * Wi, ld, dtype=_tdt(dt), device=w.device)
    if ld != cin:
        dx[:, cin:].zero_()
    mul = tuple(s_ for s_ in st)
    for (rd, rh, rw), (nd, nh, nw), first in phases:
        r = (rd, rh, rw)
        ext = tuple((i + 1) // 2 if (s_ == 2 and rr == 0) else (i // 2 if s_ == 2 else i) for i, s_, rr in zip(idhw, st, r))
        if min(ext) == 0:
            continue
        pad = tuple(1 if s_ == 1 else 0 for s_ in st)
        ntap = nd * nh * nw
        K.conv(gcl, wop[:, first * kc:(first + ntap) * kc], kc, cin, (nd, nh, nw), (1, 1, 1), pad, dt, out=dx, odhw=ext,
               scatter=(Di * Hi * Wi, mul[0] * Hi * Wi, mul[1] * Wi, mul[2], (rd * Hi + rh) * Wi + rw))
    return K.CL(dx, N, tuple(idhw), cin)


# ------------------------------------------------------------------------------------------------ convolution
# Weight gradients beside the data-gradient chain (FirstStageTrainer.step only): inside ``wgrad_side_stream()`` the weight-gradient half
# of _ConvFn.backward -- GEMM, slab reduction, spectral-norm terms -- is queued on a second stream behind the point of the chain where
# its inputs exist, and the result is parked on the parameter (``_side_grad``) instead of going through autograd's accumulation, which
# would read it on the caller's stream.  Leaving the context orders the caller's stream behind the second one and moves the parked
# gradients to ``.grad``.  Only leaf parameters take this path; everything else (derived weights, other trainers) is untouched.
_WGRAD_SIDE = {"stream": None, "params": []}      # FirstStageTrainer.step: c4 42.9 -> 41.8 ms


class wgrad_side_stream:
    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        _WGRAD_SIDE["stream"] = self.stream
        _WGRAD_SIDE["params"] = []
        return self

    def __exit__(self, *exc):
        side, params = _WGRAD_SIDE["stream"], _WGRAD_SIDE["params"]
        _WGRAD_SIDE["stream"] = None
        _WGRAD_SIDE["params"] = []
        cur = torch.cuda.current_stream()
        if side is not None:
            cur.wait_stream(side)
        for p_ in params:
            g_ = p_.__dict__.pop("_side_grad", None)
            if g_ is not None:
                # allocated from the side stream's pool, used on the caller's stream from here on: tell the allocator, so that the block
                # is not handed out again on the side stream while the optimizer still reads it
                if side is not None:
                    g_.record_stream(cur)
                p_.grad = g_ if p_.grad is None else p_.grad + g_
        return False


def _output_gradient(m, dy, y_t, bias32, want_b):
    """The rows of both gradient GEMMs of ``_ConvFn.backward``, g = dy * act'(y) (/ sigma_t), as compute dtype [M, ldg]: (g, dots,
    d_bias) with the frames' <dY_t, Y_t - b> and the bias gradient where the frame-batched spectral norm's pass yields them."""
    dt, cout = m["dtype"], m["cout"]
    M, ldg = dy.shape[0], K.round_up(cout, K.e16(dt))
    lib, s = _lib.lib(), _lib.current_stream()
    snf = m.get("sn_frames")
    pre = m.pop("_prescaled", None)
    if pre is not None:
        # the norm that reads this convolution's output alone already made that pass on its own registers (_NormFn.backward): dy IS
        # g = d(conv output) / sigma_t, the frames' dots and the bias gradient came with it
        if dy.data_ptr() != pre[0].data_ptr() or dy.shape[1] != ldg:
            raise RuntimeError("the pre-scaled gradient of a spectral-norm convolution did not arrive unchanged from its norm")
        return dy, pre[1], (pre[2] if want_b else None)
    if snf is not None:
        # one pass over (dy, y): g = dy * act'(y) / sigma_t (the rows of both gradient GEMMs), the frames' <dY_t, Y_t - b> for sigma_t's
        # own gradient, and the bias gradient
        sig = snf[0]
        frames = int(sig.shape[0])
        dyc = dy.contiguous()
        if dyc.dtype != _tdt(dt) or dyc.shape[1] < ldg:
            dyc = pad_cols(dyc, ldg, dt)
        g = torch.empty(M, ldg, dtype=_tdt(dt), device=dy.device)
        dots = torch.empty(frames, dtype=torch.float32, device=dy.device)
        d_bias = torch.empty(cout, dtype=torch.float32, device=dy.device) if want_b else None
        rd = _lib.RowScaleBwdDesc()
        rd.dy = dyc.data_ptr(); rd.lddy = dyc.shape[1]; rd.y = y_t.data_ptr(); rd.ldy = y_t.shape[1]
        rd.M, rd.C, rd.Cpad, rd.act = M, cout, ldg, m["act"]
        rd.bias = 0 if bias32 is None else bias32.data_ptr()
        sc = sig.view(-1)[1:]
        rd.scale = sc.data_ptr(); rd.scale_stride = 2; rd.rows_per_group = M // frames
        rd.gs = g.data_ptr(); rd.ldgs = ldg; rd.dots = dots.data_ptr(); rd.dbias = 0 if d_bias is None else d_bias.data_ptr()
        ws = _workspace(lib.ipoke_rowscale_bwd_workspace_floats(M, cout, M // frames), dy.device, "rowscale")
        rd.workspace = ws.data_ptr()
        check(lib.ipoke_rowscale_bwd(byref(rd), ops._dt(dt), s))
        return g, dots, d_bias
    if m["act"] != _lib.ACT_NONE:
        if m.get("out_f32", False):
            raise RuntimeError("fused activation on an fp32 output has no backward here (the loss kernel owns tanh)")
        g = torch.empty(M, ldg, dtype=_tdt(dt), device=dy.device)
        dyc = dy.contiguous()
        check(lib.ipoke_act_bwd(ptr(dyc), dyc.shape[1], ptr(y_t), y_t.shape[1], ptr(g), ldg, M, cout, ldg, m["act"], ops._dt(dt), s))
        return g, None, None
    return (pad_cols(dy, ldg, dt) if (dy.dtype != _tdt(dt) or dy.shape[1] != ldg) else dy.contiguous()), None, None


def _launch_wgrad(wd, out, dt, stream, ask_kernel):
    """``ipoke_conv_wgrad`` of the filled descriptor into the fp32 tensor ``out``.  The reduction runs over every output position (up to
    B*128*128 rows) while dW has only a handful of 128x128 tiles: split the rows over enough workgroups to fill the chip; every split
    stores its own slab, summed here (deterministic, and ~10x cheaper than fp32 atomics into the few thousand addresses of dW).
    ``ask_kernel``: the halo-staged 3x3 / 3x3x3 kernel (stride 1, large maps) tiles dW by 64 x 64 x 9 taps and names its own split count."""
    lib = _lib.lib()
    tiles = -(-wd.Nout // 128) * -(-(wd.kd * wd.kh * wd.kw * wd.Kc) // 128)
    rows = wd.NB * wd.Do * wd.Ho * wd.Wo
    splitm = max(1, min(rows // (8 * 16 * K.e16(dt)), _WGRAD_WGS // tiles))
    pref = lib.ipoke_conv_wgrad_splitm(byref(wd), ops._dt(dt), _WGRAD_HALO_WGS) if ask_kernel else 0
    if pref > 0:
        splitm = pref
    if splitm > 1:
        slabs = torch.empty(splitm, out.numel(), dtype=torch.float32, device=out.device)
        wd.splitm = splitm; wd.split_stride = out.numel(); wd.dW = slabs.data_ptr()
        check(lib.ipoke_conv_wgrad(byref(wd), ops._dt(dt), stream))
        check(lib.ipoke_reduce_rows(ptr(slabs), ptr(out), splitm, out.numel(), stream))
    else:
        wd.dW = out.data_ptr()
        check(lib.ipoke_conv_wgrad(byref(wd), ops._dt(dt), stream))


def _weight_gradient(m, w, x_t, g, dots):
    """dW of ``_ConvFn`` in PyTorch layout on the current stream, the spectral norm's own terms folded in."""
    dt, N, cin, cout, k, idhw, odhw = m["dtype"], m["N"], m["cin"], m["cout"], m["k"], m["dhw"], m["odhw"]
    lib, s = _lib.lib(), _lib.current_stream()
    ldg = g.shape[1]
    rows, cols, taps = _matrix_geometry(w, m["transposed"])
    d_w = d_w_out = torch.empty(w.shape, dtype=torch.float32, device=g.device)
    wd = WgradDesc()
    wd.kd, wd.kh, wd.kw = k
    wd.sd, wd.sh, wd.sw = m["stride"]
    wd.pd, wd.ph, wd.pw = m["pad"]
    wd.NB = N
    src = m.get("src")
    # A convolution onto a handful of channels (the decoder's last one, 64 -> 3 at 128 x 128): as written the GEMM would stream
    # the wide input once per tap against a 3-column operand (1.21 ms at B = 20, 14 TFLOP/s).  With the roles swapped -- the
    # weight gradient of the mirrored convolution from dY (8 padded channels) to X, G[c][t'][n] = sum_i X[i][c] dY[i + t' - pad][n],
    # valid for stride 1 and 'same' padding -- X is the dense 64-column operand read ONCE and the narrow dY is the one gathered
    # per tap; dW[n][c][t] = G[c][k - 1 - t][n].
    swapped = (_WGRAD_SWAP and not m["transposed"] and src is None and ldg <= 16 and x_t.shape[1] >= 4 * ldg and tuple(m["stride"]) == (1, 1, 1)
               and all(kk % 2 == 1 and pp == kk // 2 for kk, pp in zip(k, m["pad"])))
    # ConvTranspose y = C_W^T x: dW[in][out][tap] is the weight gradient of the direct conv with "input" dy, "output" x -- as when swapped
    mirrored = swapped or m["transposed"]
    a, adhw, b, bdhw = (g, odhw, x_t, idhw) if mirrored else (x_t, idhw, g, odhw)         # the rows gathered per tap | the dense rows
    wd.Di, wd.Hi, wd.Wi = adhw
    wd.Do, wd.Ho, wd.Wo = bdhw
    if a is None:                                 # the fp32 source image, read in place
        wd.A = src[0].data_ptr(); wd.a_f32 = 1
        wd.a_sn, wd.a_sc, wd.a_sd, wd.a_sh, wd.a_sw = src[4]
        wd.Kc_real = cin; wd.Kc = K.round_up(cin, K.e16(dt))
    else:
        ld = a.shape[1]
        wd.A = a.data_ptr(); wd.a_f32 = 0
        wd.a_sn = adhw[0] * adhw[1] * adhw[2] * ld; wd.a_sd = adhw[1] * adhw[2] * ld; wd.a_sh = adhw[2] * ld
        wd.a_sw = ld; wd.a_sc = 1
        wd.Kc_real = wd.Kc = ldg if mirrored else K.round_up(cin, K.e16(dt))
    wd.dY = b.data_ptr(); wd.ldy = b.shape[1]
    if swapped:
        wd.Nout = cin; wd.Kc_store = ldg
        wd.w_sn = taps * ldg; wd.w_st = ldg; wd.w_sc = 1
        d_w_out = torch.empty(cin, k[0], k[1], k[2], ldg, dtype=torch.float32, device=g.device)
    else:
        wd.Nout, wd.Kc_store = (cin, cout) if m["transposed"] else (cout, cin)
        wd.w_sn = wd.Kc_store * taps; wd.w_sc = taps; wd.w_st = 1
    _launch_wgrad(wd, d_w_out, dt, s, True)
    if swapped:
        d_w.copy_(d_w_out[..., :cout].flip(1, 2, 3).permute(4, 0, 1, 2, 3).reshape(w.shape))
    if m.get("sn") is not None:                  # d_w is the gradient w.r.t. weight_orig / sigma: fold sigma's own gradient in
        sig, snap, bws = m["sn"]
        check(lib.ipoke_spectral_bwd(ptr(w), rows, cols, taps, int(m["transposed"]), ptr(d_w), ptr(snap), ptr(sig), ptr(bws), s))
    if m.get("sn_frames") is not None:            # d_w holds sum_t dW_eff_t / sigma_t; sigma_t's own gradients are rank-1 terms
        sig, snaps = m["sn_frames"]
        check(lib.ipoke_spectral_bwd_frames(ptr(w), rows, cols, taps, int(m["transposed"]), ptr(d_w), ptr(snaps), snaps.stride(0),
                                            ptr(sig), sig.stride(0), ptr(dots), int(sig.shape[0]), s))
    return d_w


def _data_gradient(m, w, x_t, g):
    """dX of ``_ConvFn``: the adjoint convolution with the same weights, on the caller's stream (whose operand cache entries it sees)."""
    dt, N, cin, cout, k, st, pd = m["dtype"], m["N"], m["cin"], m["cout"], m["k"], m["stride"], m["pad"]
    idhw, odhw = m["dhw"], m["odhw"]
    sn = m.get("sn")
    inv = None if sn is None else sn[0][1:]
    gcl = K.CL(g, N, odhw, cout)
    if not m["transposed"] and sn is None and m.get("sn_frames") is None and w.dim() == 5 and dgrad_phases_ok(k, st, pd, idhw, odhw):
        dx = _dgrad_phases(gcl, w, cin, idhw, st, dt)
    elif not m["transposed"]:
        # conv weight [cout, cin, k] read as a ConvTranspose weight [in=cout, out=cin, k]
        wop, kc = _weight_operand(w.detach(), dt, True, inv, cacheable=m.get("w_param", False), scope=m.get("w_scope"), owner=w)
        opad = tuple(i - ((o - 1) * s_ - 2 * p + kk) for i, o, s_, p, kk in zip(idhw, odhw, st, pd, k))
        dx = K.conv(gcl, wop, kc, cin, k, st, pd, dt, transposed=True, out_pad=opad)
    else:
        wop, kc = _weight_operand(w.detach(), dt, False, inv, cacheable=m.get("w_param", False), scope=m.get("w_scope"), owner=w)   # [in, out, k] read as conv weight [cout'=in]
        dx = K.conv(gcl, wop, kc, cin, k, st, pd, dt)
    assert dx.dhw == tuple(idhw), (dx.dhw, idhw)
    d_x = dx.t
    if d_x.shape[1] != x_t.shape[1]:
        d_x = pad_cols(d_x[:, :min(d_x.shape[1], x_t.shape[1])], x_t.shape[1], dt)
    return d_x


class _ConvFn(torch.autograd.Function):
    """y = act(conv(x, w) + bias).  ``x`` is the CL tensor [M, ld] (or None with ``meta['src']`` an fp32 image)."""

    @staticmethod
    def forward(ctx, x_t, w, bias, meta):
        dt = meta["dtype"]
        sn = meta.get("sn")                       # (sig, snap): w is weight_orig, the operand carries 1/sigma
        snf = meta.get("sn_frames")               # (sig [F, 2], snaps [F, n]): w is weight_orig, ONE operand, 1/sigma_t in the epilogue
        meta["w_param"] = (isinstance(w, torch.nn.Parameter) or meta.get("w_scope") is not None) and sn is None
        wop, kc = _weight_operand(w.detach(), dt, meta["transposed"], None if sn is None else sn[0][1:], cacheable=meta["w_param"],
                                  scope=meta.get("w_scope"), owner=w)
        b = None if bias is None else bias.detach().float().contiguous()
        src = meta.get("src")
        x = None if src is not None else K.CL(x_t, meta["N"], meta["dhw"], meta["cin"])
        rs = None
        if snf is not None:
            frames = int(snf[0].shape[0])
            if meta["N"] % frames or meta.get("out_f32", False):
                raise RuntimeError("frame-batched spectral norm: the batch must hold whole frames and a dtype output")
            rs = (snf[0].view(-1)[1:], meta["N"] // frames, 2)
        if (meta["transposed"] and x is not None and tuple(meta["k"]) == (1, 3, 3) and tuple(meta["stride"]) == (1, 2, 2)
                and tuple(meta["pad"]) == (0, 1, 1) and tuple(meta["out_pad"]) == (0, 1, 1)):
            y = _conv_transpose_phases(x, wop, kc, meta["cout"], dt, b, meta["act"], meta.get("out_f32", False), row_scale=rs)
        else:
            y = K.conv(x, wop, kc, meta["cout"], meta["k"], meta["stride"], meta["pad"], dt, bias=b, act=meta["act"],
                       transposed=meta["transposed"], out_pad=meta["out_pad"], out_f32=meta.get("out_f32", False), src_f32=src, row_scale=rs)
        meta["odhw"] = y.dhw
        ctx.meta = meta
        ctx.bias32 = b if snf is not None else None
        if snf is not None:
            meta["_bias32"] = b                   # the norm behind this convolution may fold the row-scale pass of backward (_NormFn)
        ctx.save_for_backward(x_t, w, y.t if (meta["act"] != _lib.ACT_NONE or snf is not None) else None)
        ctx.has_bias = bias is not None
        return y.t

    @staticmethod
    def backward(ctx, dy):
        x_t, w, y_t = ctx.saved_tensors
        m = ctx.meta
        dt, cout = m["dtype"], m["cout"]
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        want_b = ctx.has_bias and need_b
        g, dots, d_bias = _output_gradient(m, dy, y_t, ctx.bias32, want_b)
        if m.get("sn_frames") is None and want_b:
            d_bias = torch.empty(cout, dtype=torch.float32, device=dy.device)
            ws = _workspace(_lib.lib().ipoke_colsum_workspace_floats(g.shape[0], cout), dy.device, "colsum")
            check(_lib.lib().ipoke_colsum(ptr(g), g.shape[1], g.shape[0], cout, 0, ptr(d_bias), 0, ptr(ws), ops._dt(dt), _lib.current_stream()))
        d_w = None
        side = _WGRAD_SIDE["stream"] if (need_w and w.is_leaf) else None
        if side is not None:
            # the weight-gradient half on the second stream, behind this point of the chain; the result is parked on the parameter
            here = torch.cuda.Event(); here.record()
            side.wait_event(here)
            for t_ in (g, x_t, dy, dots) + tuple(m.get("sn_frames") or ()) + tuple(m.get("sn") or ()):
                if torch.is_tensor(t_) and t_.is_cuda:
                    t_.record_stream(side)
            if m.get("src") is not None:
                m["src"][0].record_stream(side)
            with torch.cuda.stream(side):
                d_w = _weight_gradient(m, w, x_t, g, dots)
                if hasattr(w, "_side_grad"):
                    w._side_grad = w._side_grad + d_w
                else:
                    w._side_grad = d_w
                    _WGRAD_SIDE["params"].append(w)
            d_w = None
        elif need_w:                                  # frozen weights (the VGG feature extractor) skip this half
            d_w = _weight_gradient(m, w, x_t, g, dots)
        d_x = _data_gradient(m, w, x_t, g) if (x_t is not None and need_x) else None
        return d_x, d_w, d_bias, None



class _StemFn(torch.autograd.Function):
    """conv1 of the 3-D motion encoder (Conv3d(3, 64, (3, 7, 7), 2, (1, 3, 3)), motion_encoder.py:106-107) on the fp32 clip, with
    gradient w.r.t. the weight.  As in the inference path (first_stage.py::_stem) the clip is rewritten once as padded channels-last
    pixels of four channels, so that a 7-tap run along x is ONE aligned 64-byte read: forward = 21 taps of 32 channels on the LDS-DMA
    GEMM; the weight gradient is the same geometry through ``ipoke_conv_wgrad`` -- a dense bf16 operand for the LDS-DMA /
    transposed-read kernel instead of 147 taps of 3 strided floats through the register-staged one (c4, B = 20: 1 623 -> see DESIGN §7
    us for the weight gradient, 653 -> ~100 us forward) -- and the [64][21][32] result is unfolded into the parameter's layout."""

    @staticmethod
    def forward(ctx, x, w, dt):
        B, C, T, H, W = x.shape
        cout = w.shape[0]
        lib = _lib.lib()
        s = _lib.current_stream()
        Wp = W + 6
        clip = torch.empty(B * T * H * Wp, 4, dtype=_tdt(dt), device=x.device)
        check(lib.ipoke_clip_to_cl4(ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), x.stride(4), B, T, H, W, 3, 3,
                                    ptr(clip), ops._dt(dt), s))
        odhw = ((T + 2 - 3) // 2 + 1, (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1)
        buf = torch.zeros(cout, 3, 7, 8, 4, dtype=torch.float32, device=w.device)
        buf[:, :, :, :7, :3] = w.detach().float().permute(0, 2, 3, 4, 1)
        wop = buf.reshape(cout, 21 * 32).to(_tdt(dt)).contiguous()
        d = ops.conv_desc(B, (T, H, odhw[2]), odhw, (3, 7, 1), (2, 2, 1), (1, 3, 0))
        d.A = clip.data_ptr(); d.a_f32 = 0
        d.a_sn, d.a_sd, d.a_sh, d.a_sw, d.a_sc = T * H * Wp * 4, H * Wp * 4, Wp * 4, 8, 1
        d.a_coff = 0; d.Kc_real = 32; d.Kc = 32
        d.W = wop.data_ptr(); d.ldw = wop.shape[1]; d.Nout = cout
        d.bias = 0; d.act = _lib.ACT_NONE
        y = torch.empty(B * odhw[0] * odhw[1] * odhw[2], K.round_up(cout, K.e16(dt)), dtype=_tdt(dt), device=x.device)
        d.C = y.data_ptr(); d.ldc = y.shape[1]
        ops.conv_forward(d, dt)
        ctx.save_for_backward(clip)
        ctx.geom = (B, T, H, W, Wp, odhw, cout, dt, tuple(w.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        (clip,) = ctx.saved_tensors
        B, T, H, W, Wp, odhw, cout, dt, wshape = ctx.geom
        if not ctx.needs_input_grad[1]:
            return None, None, None
        ldg = K.round_up(cout, K.e16(dt))
        g = pad_cols(dy, ldg, dt) if (dy.dtype != _tdt(dt) or dy.shape[1] != ldg) else dy.contiguous()
        dwf = torch.empty(cout, 21 * 32, dtype=torch.float32, device=dy.device)
        wd = WgradDesc()
        wd.kd, wd.kh, wd.kw = 3, 7, 1
        wd.sd, wd.sh, wd.sw = 2, 2, 1
        wd.pd, wd.ph, wd.pw = 1, 3, 0
        wd.NB = B
        wd.Di, wd.Hi, wd.Wi = T, H, odhw[2]
        wd.Do, wd.Ho, wd.Wo = odhw
        wd.A = clip.data_ptr(); wd.a_f32 = 0
        wd.a_sn, wd.a_sd, wd.a_sh, wd.a_sw, wd.a_sc = T * H * Wp * 4, H * Wp * 4, Wp * 4, 8, 1
        wd.Kc_real = 32; wd.Kc = 32; wd.Kc_store = 32
        wd.dY = g.data_ptr(); wd.ldy = ldg; wd.Nout = cout
        wd.w_sn = 21 * 32; wd.w_st = 32; wd.w_sc = 1
        _launch_wgrad(wd, dwf, dt, _lib.current_stream(), False)
        d_w = dwf.view(cout, 3, 7, 8, 4)[:, :, :, :7, :3].permute(0, 4, 1, 2, 3).contiguous()
        assert tuple(d_w.shape) == wshape
        return None, d_w, None


def stem_folds(mod, x):
    """Whether conv1 on this clip can run folded (the reference's shipped geometry; otherwise the generic in-place path: c4 50.3 vs 48.45 ms)."""
    return (FS._STEM_FOLD and x.shape[1] == 3 and tuple(mod.k) == (3, 7, 7) and tuple(mod.stride) == (2, 2, 2)
            and tuple(mod.pad) == (1, 3, 3) and x.shape[4] % 2 == 0 and mod.bias is None and not mod.snorm and not mod.transposed)


def stem(x, w, dtype):
    """``_StemFn`` on the clip x [B, 3, T, H, W] fp32 (``stem_folds`` says whether it applies); returns CL."""
    B, _, T, H, W = x.shape
    return K.CL(_StemFn.apply(x, w, dtype), B, ((T + 2 - 3) // 2 + 1, (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1), w.shape[0])


def conv_weight(x, w, bias, k, stride, pad, dtype, act=_lib.ACT_NONE, out_f32=False, src=None, transposed=False, scope=None):
    """y = act(conv(x, w) + bias) with gradients on a bare weight: a tensor in PyTorch layout (``transposed``: ConvTranspose storage) or
    what ``effective_weight`` hands out.  ``x``: CL (or None with ``src`` = (fp32 tensor, N, C, dhw, strides (n, c, d, h, w))); returns CL.
    ``scope``: ``w`` is a derived tensor that several calls of this pass share -- its operand is cached under that scope."""
    N, dhw, cin = (src[1], src[3], src[2]) if src is not None else (x.N, x.dhw, x.C)
    w_t = w.w_orig if isinstance(w, (_SnWeight, _SnFrames)) else w
    cout = w_t.shape[1] if transposed else w_t.shape[0]
    meta = dict(N=N, dhw=tuple(dhw), cin=cin, cout=cout, k=k, stride=stride, pad=pad, transposed=transposed,
                out_pad=(0, pad[1], pad[2]) if transposed else (0, 0, 0), dtype=dtype, act=act, out_f32=out_f32, src=src)
    if scope is not None:
        meta["w_scope"] = scope
    if isinstance(w, _SnWeight):
        bws = getattr(w.mod, "_sn_bwd_ws", None)
        if bws is None or bws.device != w.w_orig.device:
            bws = w.mod._sn_bwd_ws = torch.zeros(int(_lib.lib().ipoke_spectral_bwd_workspace_floats()), dtype=torch.float32, device=w.w_orig.device)
        meta["sn"] = (w.sig, w.snap, bws)
    elif isinstance(w, _SnFrames):
        meta["sn_frames"] = (w.sig, w.snaps)
    y = _ConvFn.apply(None if src is not None else x.t, w_t, bias, meta)
    out = K.CL(y, N, meta["odhw"], cout)
    out.conv_meta = meta
    return out


def conv(mod, x, dtype, act=_lib.ACT_NONE, out_f32=False, src=None, w=None):
    """Differentiable ``_Conv.run``.  ``x``: CL (or None with ``src``); returns CL."""
    return conv_weight(x, effective_weight(mod) if w is None else w, mod.bias, mod.k, mod.stride, mod.pad, dtype, act=act, out_f32=out_f32,
                       src=src, transposed=mod.transposed)


def effective_weight(mod, power_iteration=False, frames=None):
    """The conv weight as ``conv`` takes it: the plain ``weight`` parameter, or for spectral norm a ``_SnWeight`` --
    torch spectral_norm semantics: u, v are buffers updated without grad by one power iteration per call in train mode;
    sigma = u^T W v carries grad (ipoke_spectral_sigma / ipoke_spectral_bwd), the division by sigma happens while the
    matrix-core operand is written.  ``frames``: the input is the batch of all ``frames`` decoder calls of this pass ordered
    (frame, clip) -> a ``_SnFrames`` with the whole table of the calls' sigmas (run ahead by ``precompute_power_iterations``); without
    power iteration one sigma serves the whole batch."""
    if not mod.snorm:
        return mod.weight
    w = mod.weight_orig
    pre = mod.__dict__.get("_sn_pre")
    if frames is not None:
        if power_iteration:
            tab = mod.__dict__.pop("_sn_tab", None)
            if tab is None or tab[0].shape[0] != frames or not pre or len(pre) != frames:
                raise RuntimeError("frame-batched spectral norm needs precompute_power_iterations(root, frames) before the decoder pass")
            pre.clear()                           # this ONE batched call consumes the module's T - 1 iterations
            return _SnFrames(w, tab[0], tab[1], mod.transposed, mod)
        one = effective_weight(mod, False)
        return _SnFrames(w, one.sig.view(1, 2), one.snap.view(1, -1), mod.transposed, mod)
    if power_iteration and pre:                   # this call's iteration was run ahead of the time loop (precompute_power_iterations)
        sig, snap = pre.pop(0)
        return _SnWeight(w, sig, snap, mod.transposed, mod)
    rows, cols, taps = _matrix_geometry(w, mod.transposed)
    lib = _lib.lib()
    ws = getattr(mod, "_sn_ws", None)
    if ws is None or ws.device != w.device:
        ws = mod._sn_ws = torch.zeros(int(lib.ipoke_spectral_workspace_floats(rows, cols, taps)), dtype=torch.float32, device=w.device)
    sig = torch.empty(2, dtype=torch.float32, device=w.device)
    snap = torch.empty(rows + cols * taps, dtype=torch.float32, device=w.device)
    check(lib.ipoke_spectral_sigma(ptr(w), rows, cols, taps, int(mod.transposed), ptr(mod.weight_u), ptr(mod.weight_v),
                                   int(bool(power_iteration)), 1e-12, ptr(sig), ptr(snap), ptr(ws), _lib.current_stream()))
    return _SnWeight(w, sig, snap, mod.transposed, mod)


def precompute_power_iterations(root, calls):
    """Run the ``calls`` power iterations that the next ``calls`` forward calls of every spectral-normalised convolution under
    ``root`` would perform (torch's spectral_norm iterates once per call; the decoder is called once per generated frame), three
    launches per iteration for ALL weights (ipoke_spectral_sigma_multi) instead of three per call.  Each module's queue ``_sn_pre``
    then hands the (sigma, snapshot) pairs to ``effective_weight`` call by call -- the same arithmetic in the same order per weight."""
    mods = [m for m in root.modules() if isinstance(m, FS._Conv) and m.snorm]
    if not mods or calls < 1:
        return []
    lib = _lib.lib()
    dev = mods[0].weight_orig.device
    geo = [_matrix_geometry(m.weight_orig, m.transposed) for m in mods]
    for m, (r, c, t) in zip(mods, geo):
        ws = getattr(m, "_sn_ws", None)
        if ws is None or ws.device != dev:
            m._sn_ws = torch.zeros(int(lib.ipoke_spectral_workspace_floats(r, c, t)), dtype=torch.float32, device=dev)
    key = (calls,) + tuple((m.weight_orig.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr(), m._sn_ws.data_ptr()) for m in mods)
    cache = root.__dict__.get("_sn_multi")
    if cache is None or cache["key"] != key:
        sizes = [r + c * t for r, c, t in geo]
        sig_all = torch.empty(len(mods), calls, 2, dtype=torch.float32, device=dev)
        snap_all = torch.empty(calls * sum(sizes), dtype=torch.float32, device=dev)
        jobs = (_lib.SnJob * len(mods))()
        snaps, off = [], 0
        for i, (m, (r, c, t), n) in enumerate(zip(mods, geo, sizes)):
            sv = snap_all[off:off + calls * n].view(calls, n)
            off += calls * n
            snaps.append(sv)
            j = jobs[i]
            j.w = m.weight_orig.data_ptr(); j.cout, j.cin, j.taps, j.transposed = r, c, t, int(m.transposed)
            j.u = m.weight_u.data_ptr(); j.v = m.weight_v.data_ptr()
            j.out = sig_all[i].data_ptr(); j.out_stride = 2
            j.snap = sv.data_ptr(); j.snap_stride = n
            j.workspace = m._sn_ws.data_ptr()
        jobs_dev = torch.empty(len(mods) * int(lib.ipoke_sn_job_size()), dtype=torch.uint8, device=dev)
        check(lib.ipoke_sn_jobs_upload(ctypes.byref(jobs), len(mods), ptr(jobs_dev), _lib.current_stream()))
        cache = dict(key=key, sig=sig_all, snap_all=snap_all, snaps=snaps, jobs_dev=jobs_dev, max_r=max(g[0] for g in geo),
                     max_c=max(g[1] * g[2] for g in geo))
        root.__dict__["_sn_multi"] = cache
    check(lib.ipoke_spectral_sigma_multi(ptr(cache["jobs_dev"]), len(mods), cache["max_r"], cache["max_c"], calls, 1e-12, _lib.current_stream()))
    for i, m in enumerate(mods):
        m.__dict__["_sn_pre"] = [(cache["sig"][i, k], cache["snaps"][i][k]) for k in range(calls)]
        m.__dict__["_sn_tab"] = (cache["sig"][i], cache["snaps"][i])             # the same iterations as whole tables (frame-batched decoding)
    return mods


# ------------------------------------------------------------------------------------------------ norms
class _NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_t, gamma, beta, mg_t, mb_t, res_t, meta):
        dt = meta["dtype"]
        N, S, C, G = meta["N"], meta["S"], meta["C"], meta["G"]
        y = torch.empty_like(x_t)
        d = NormDesc()
        d.x = x_t.data_ptr(); d.ldx = x_t.shape[1]; d.y = y.data_ptr(); d.ldy = y.shape[1]; d.y_f32 = 0
        d.N, d.S, d.C, d.G, d.eps = N, S, C, G, 1e-5
        g32 = b32 = None
        if gamma is not None:
            g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
            d.gamma = g32.data_ptr(); d.beta = b32.data_ptr()
        if mg_t is not None:
            d.mod_gamma = mg_t.data_ptr(); d.mod_beta = mb_t.data_ptr(); d.ld_mod = mg_t.shape[1]
            d.mod_samples = int(meta.get("mod_samples", 0))        # > 0: the frames of a clip share its SPADE maps (batch ordered (frame, clip))
        if res_t is not None:
            d.res = res_t.data_ptr(); d.ld_res = res_t.shape[1]; d.res_post = int(bool(meta.get("res_post", False)))
        d.act = meta["act"]
        ws = _workspace(_lib.lib().ipoke_groupnorm_workspace_floats(N, S, G), x_t.device, "norm")
        d.workspace = ws.data_ptr()
        check(_lib.lib().ipoke_groupnorm(byref(d), ops._dt(dt), _lib.current_stream()))
        if y.shape[1] > C:
            y[:, C:].zero_()
        off = _lib.lib().ipoke_groupnorm_stats_offset(N, S, G)
        stats = ws[off:off + N * G * 2].clone()               # (mean, rstd): kept for the backward pass
        ctx.meta = meta
        ctx.save_for_backward(x_t, y, g32, b32, mg_t, stats)
        ctx.has = (gamma is not None, mg_t is not None, res_t is not None)
        ctx.ld_res = None if res_t is None else res_t.shape[1]
        return y

    @staticmethod
    def backward(ctx, dy):
        x_t, y, g32, b32, mg_t, stats = ctx.saved_tensors
        m = ctx.meta
        dt = m["dtype"]
        N, S, C, G = m["N"], m["S"], m["C"], m["G"]
        has_affine, has_mod, has_res = ctx.has
        dy = dy.contiguous()
        dx = torch.zeros_like(x_t) if x_t.shape[1] > C else torch.empty_like(x_t)
        d = NormBwdDesc()
        d.x = x_t.data_ptr(); d.ldx = x_t.shape[1]; d.y = y.data_ptr(); d.ldy = y.shape[1]
        d.dy = dy.data_ptr(); d.lddy = dy.shape[1]; d.dx = dx.data_ptr(); d.lddx = dx.shape[1]
        d.N, d.S, d.C, d.G, d.eps = N, S, C, G, 1e-5
        d.act = m["act"]
        dres = dmg = dmb = dgamma = dbeta = None
        if has_res and m.get("res_post", False):
            # y = act(pre) + res: the residual's gradient is dy itself, act' comes from the pre-activation value recomputed from x (y is not read)
            dres = _fit_cols(dy, ctx.ld_res, dt)       # (the residual may have another pitch than x, whose pitch dy has)
            d.act_from_pre = 1
        elif has_res:
            dres = (torch.zeros if ctx.ld_res > C else torch.empty)(x_t.shape[0], ctx.ld_res, dtype=x_t.dtype, device=x_t.device)
            d.dres = dres.data_ptr(); d.lddres = dres.shape[1]
        mod_n = int(m.get("mod_samples", 0)) if has_mod else 0
        if has_mod:
            # the kernel writes columns 0 .. C-1 of every row; only padding columns (ld > C) need the zero fill
            alloc = torch.zeros if mg_t.shape[1] > C else torch.empty
            # mod_n: the frames of a clip share its maps -- the kernel walks the frames and writes the sum (c4 37.3 ms against 37.9 with
            # per-frame gradients summed in a pass of their own)
            dmg = alloc(mg_t.shape[0], mg_t.shape[1], dtype=mg_t.dtype, device=mg_t.device)
            dmb = alloc(mg_t.shape[0], mg_t.shape[1], dtype=mg_t.dtype, device=mg_t.device)
            d.dmod_gamma = dmg.data_ptr(); d.dmod_beta = dmb.data_ptr(); d.ld_dmod = dmg.shape[1]
            d.mod_gamma = mg_t.data_ptr(); d.ld_mod = mg_t.shape[1]; d.mod_samples = mod_n
            d.dmod_summed = int(bool(mod_n))
        if has_affine:
            dgamma = torch.empty(C, dtype=torch.float32, device=dy.device); dbeta = torch.empty_like(dgamma)
            d.gamma = g32.data_ptr(); d.beta = b32.data_ptr(); d.dgamma = dgamma.data_ptr(); d.dbeta = dbeta.data_ptr()
        ws = _workspace(_lib.lib().ipoke_groupnorm_bwd_workspace_floats(N, S, C, G), dy.device, "normbwd")
        d.workspace = ws.data_ptr()
        d.stats = stats.data_ptr()
        pm = m.get("producer") if ctx.needs_input_grad[0] else None      # (no gradient for x: the convolution's backward never runs)
        if pm is not None:
            # x is the un-activated output of a frame-batched spectral-norm convolution nobody else reads: dx leaves as dx / sigma_t with
            # the frames' <dx, x - b> and the bias gradient (the convolution's own pass over (dx, x), ipoke_rowscale_bwd, folded in)
            sig = pm["sn_frames"][0]
            frames = int(sig.shape[0])
            rs_dots = torch.empty(frames, dtype=torch.float32, device=dy.device)
            rs_db = torch.empty(C, dtype=torch.float32, device=dy.device) if pm.get("_bias32") is not None else None
            rs_ws = _workspace(_lib.lib().ipoke_groupnorm_bwd_rs_workspace_floats(N, S, C), dy.device, "normbwd_rs")
            d.rs_scale = sig.view(-1)[1:].data_ptr(); d.rs_scale_stride = 2; d.rs_rows_per_group = (N // frames) * S
            d.rs_bias = 0 if pm.get("_bias32") is None else pm["_bias32"].data_ptr()
            d.rs_dots = rs_dots.data_ptr(); d.rs_dbias = 0 if rs_db is None else rs_db.data_ptr(); d.rs_workspace = rs_ws.data_ptr()
            pm["_prescaled"] = (dx, rs_dots, rs_db)
        check(_lib.lib().ipoke_groupnorm_bwd(byref(d), ops._dt(dt), _lib.current_stream()))
        return dx, dgamma, dbeta, dmg, dmb, dres, None


def _rowscale_producer(x, mod, dtype, res_post=False):
    """The meta of the convolution that produced ``x`` when the norm's backward may fold its row-scale pass: a frame-batched
    spectral-norm convolution without activation whose dtype output this norm alone reads (c4 37.85 ms against 38.75 with the
    convolution's own ipoke_rowscale_bwd pass).  Declined where ipoke_groupnorm_bwd would refuse the folded form: its apply pass keeps
    6 C floats (8 C with the residual behind the activation) and the fold's 256 x 16 bytes + 4 floats in the 64 KB of LDS a launch gets --
    which bites with the residual behind the activation only (C <= 1919 in fp32, 1791 in bf16; without it the limit lies above 2048)."""
    pm = getattr(x, "conv_meta", None)
    if pm is None or mod is not None or pm.get("sn_frames") is None or pm["act"] != _lib.ACT_NONE or pm.get("out_f32", False):
        return None
    frames = int(pm["sn_frames"][0].shape[0])
    if x.N % frames or x.t.shape[1] != x.C or x.C > 2048:
        return None
    if 4 * ((8 if res_post else 6) * x.C + 256 * K.e16(dtype) + 4) > 64 * 1024:
        return None
    return pm


def group_norm(x, groups, dtype, gamma=None, beta=None, act=_lib.ACT_NONE, res=None, mod=None, sole_reader=False, res_post=False):
    """``res_post``: the residual joins behind the activation, y = act(norm(x)) + res."""
    meta = dict(N=x.N, S=x.S, C=x.C, G=groups, dtype=dtype, act=act, res_post=bool(res_post) and res is not None)
    if sole_reader:
        meta["producer"] = _rowscale_producer(x, mod, dtype, meta["res_post"])
    if mod is not None and mod[0].N != x.N:       # frames of a clip decoded as one batch ordered (frame, clip): shared SPADE maps
        assert x.N % mod[0].N == 0 and mod[0].S == x.S and mod[0].t.shape[0] == mod[0].N * x.S
        meta["mod_samples"] = mod[0].N
    y = _NormFn.apply(x.t, gamma, beta, None if mod is None else mod[0].t, None if mod is None else mod[1].t,
                      None if res is None else res.t, meta)
    return K.CL(y, x.N, x.dhw, x.C)


def norm(mod, x, dtype, act=_lib.ACT_NONE, res=None, sole_reader=False, res_post=False):
    """``sole_reader``: ``x`` is a convolution's output that nothing but this norm reads (see _rowscale_producer)."""
    if mod.kind == "group":
        return group_norm(x, mod.groups, dtype, mod.weight, mod.bias, act=act, res=res, sole_reader=sole_reader, res_post=res_post)
    return group_norm(x, mod.groups, dtype, act=act, res=res, sole_reader=sole_reader, res_post=res_post)


class _AddActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a_t, b_t, C, act, dtype):
        y = torch.zeros_like(a_t) if a_t.shape[1] > C else torch.empty_like(a_t)
        check(_lib.lib().ipoke_add_act(ptr(a_t), a_t.shape[1], ptr(b_t), b_t.shape[1], ptr(y), y.shape[1], a_t.shape[0], C, act,
                                       ops._dt(dtype), _lib.current_stream()))
        ctx.save_for_backward(y)
        ctx.args = (C, act, dtype)
        ctx.ld_b = b_t.shape[1]
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        C, act, dtype = ctx.args
        if act == _lib.ACT_NONE:
            return dy, _fit_cols(dy, ctx.ld_b, dtype), None, None, None
        dy = dy.contiguous()
        g = torch.empty_like(y)
        check(_lib.lib().ipoke_act_bwd(ptr(dy), dy.shape[1], ptr(y), y.shape[1], ptr(g), g.shape[1], y.shape[0], C, y.shape[1], act,
                                       ops._dt(dtype), _lib.current_stream()))
        return g, _fit_cols(g, ctx.ld_b, dtype), None, None, None


def add_act(a, b, dtype, act):
    return K.CL(_AddActFn.apply(a.t, b.t, a.C, act, dtype), a.N, a.dhw, a.C)


# ------------------------------------------------------------------------------------------------ ConvGRU
class _GruGatesFn(torch.autograd.Function):
    """(ur_pre [M,2Ch], h [M,ldh]) -> (h*sigmoid(r), sigmoid(u))"""

    @staticmethod
    def forward(ctx, ur_t, h_t, Ch, dtype):
        M = ur_t.shape[0]
        hr = torch.empty(M, Ch, dtype=ur_t.dtype, device=ur_t.device)
        u = torch.empty(M, Ch, dtype=ur_t.dtype, device=ur_t.device)
        check(_lib.lib().ipoke_gru_gates(ptr(ur_t), ptr(h_t), h_t.shape[1], ptr(hr), Ch, ptr(u), M, Ch, ops._dt(dtype),
                                         _lib.current_stream()))
        ctx.save_for_backward(ur_t, h_t)
        ctx.args = (Ch, dtype)
        return hr, u

    @staticmethod
    def backward(ctx, d_hr, d_u):
        ur_t, h_t = ctx.saved_tensors
        Ch, dtype = ctx.args
        M = ur_t.shape[0]
        d_hr = d_hr.contiguous(); d_u = d_u.contiguous()
        d_ur = torch.zeros_like(ur_t)
        d_h = torch.zeros_like(h_t)
        check(_lib.lib().ipoke_gru_gates_bwd(ptr(ur_t), ptr(h_t), h_t.shape[1], ptr(d_hr), d_hr.shape[1], ptr(d_u), ptr(d_ur),
                                             ptr(d_h), d_h.shape[1], M, Ch, ops._dt(dtype), _lib.current_stream()))
        return d_ur, d_h, None, None


class _GruUpdateFn(torch.autograd.Function):
    """(o_pre [M,Ch..], u [M,Ch], h) -> h*(1-u) + tanh(o_pre)*u"""

    @staticmethod
    def forward(ctx, o_t, u_t, h_t, Ch, dtype):
        M = o_t.shape[0]
        o_c = o_t[:, :Ch].contiguous()
        hn = torch.empty(M, Ch, dtype=o_t.dtype, device=o_t.device)
        check(_lib.lib().ipoke_gru_update(ptr(o_c), ptr(u_t), ptr(h_t), h_t.shape[1], ptr(hn), Ch, M, Ch, ops._dt(dtype),
                                          _lib.current_stream()))
        ctx.save_for_backward(o_c, u_t, h_t)
        ctx.args = (Ch, dtype, o_t.shape[1])
        return hn

    @staticmethod
    def backward(ctx, d_hn):
        o_c, u_t, h_t = ctx.saved_tensors
        Ch, dtype, ldo = ctx.args
        M = o_c.shape[0]
        d_hn = d_hn.contiguous()
        d_o = torch.empty_like(o_c); d_u = torch.empty_like(u_t); d_h = torch.zeros_like(h_t)
        check(_lib.lib().ipoke_gru_update_bwd(ptr(o_c), ptr(u_t), ptr(h_t), h_t.shape[1], ptr(d_hn), d_hn.shape[1], ptr(d_o), ptr(d_u),
                                              ptr(d_h), d_h.shape[1], M, Ch, ops._dt(dtype), _lib.current_stream()))
        if ldo != Ch:
            d_o = pad_cols(d_o, ldo, dtype)
        return d_o, d_u, d_h, None, None


def gru_gate_weights(cell):
    """update | reset gate weights and biases as one convolution (built once per forward pass, shared by its time steps)."""
    return (torch.cat([cell.update_gate.weight, cell.reset_gate.weight], 0), torch.cat([cell.update_gate.bias, cell.reset_gate.bias]))


def gru_cell(cell, x, h, dtype, gate_w=None):
    """ConvGRUCell.run with gradients (rnn.py:48-56)."""
    Ch = cell.hidden
    xh = torch.cat([x.t[:, :x.C], h.t[:, :Ch]], dim=1)
    xh_cl = K.CL(xh, x.N, x.dhw, x.C + Ch)
    # update and reset gates share their input: one GEMM with the concatenated weights (update first)
    w_ur, b_ur = gru_gate_weights(cell) if gate_w is None else gate_w
    # ``gate_w``: the same tensor for every time step of this pass (begin_forward_pass): its operand is built once
    ur = conv_weight(xh_cl, w_ur, b_ur, (1, 3, 3), (1, 1, 1), (0, 1, 1), dtype, scope=None if gate_w is None else _FWD_EPOCH[0]).t
    hr, u = _GruGatesFn.apply(ur[:, :2 * Ch].contiguous(), h.t, Ch, dtype)
    xhr = torch.cat([x.t[:, :x.C], hr], dim=1)
    o = conv(cell.out_gate, K.CL(xhr, x.N, x.dhw, x.C + Ch), dtype)
    hn = _GruUpdateFn.apply(o.t, u, h.t, Ch, dtype)
    return K.CL(hn, x.N, x.dhw, Ch)


def gru_native_ok(rnn, x, h, dtype):
    """The native unroll (csrc/gru.hip) covers the shipped ConvGRU: 3 x 3 gates, every cell as wide as its input, power-of-two maps
    (c4 51.1 ms against 56.9 cell by cell from Python, which is what runs otherwise)."""
    e = K.e16(dtype)
    cells = list(rnn.cells)
    H, W = x.dhw[1], x.dhw[2]
    return (x.dhw[0] == 1 and H & (H - 1) == 0 and W & (W - 1) == 0 and x.C % e == 0 and h.C % e == 0 and len(cells) <= 16
            and all(c.hidden == h.C and c.cin == (x.C if i == 0 else h.C) and c.update_gate.k == (1, 3, 3) and c.out_gate.k == (1, 3, 3)
                    and c.update_gate.pad == (0, 1, 1) and c.update_gate.bias is not None and c.out_gate.bias is not None
                    for i, c in enumerate(cells))
            and (len(cells) == 1 or x.C == h.C))


def _gru_desc(B, T, L, Cx, Ch, H, W):
    d = _lib.GruDesc()
    d.B, d.T, d.L, d.Cx, d.Ch, d.H, d.W = B, T, L, Cx, Ch, H, W
    return d


def gru_unroll_forward(weights, x0_t, h0_t, geom, dtype):
    """ipoke_gru_unroll_forward: ``weights`` = per cell (w_ur, b_ur, w_o, b_o) fp32; returns (out [T * M, ld], workspace)."""
    B, T, L, Cx, Ch, H, W = geom
    d = _gru_desc(*geom)
    lib = _lib.lib()
    nbytes = int(lib.ipoke_gru_workspace_bytes(byref(d), ops._dt(dtype)))
    if nbytes < 0:
        raise RuntimeError("ConvGRU geometry not supported by the native unroll")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x0_t.device)
    ldo = K.round_up(Ch, K.e16(dtype))
    out = torch.zeros(T * B * H * W, ldo, dtype=_tdt(dtype), device=x0_t.device) if ldo > Ch else torch.empty(T * B * H * W, ldo, dtype=_tdt(dtype),
                                                                                                             device=x0_t.device)
    w32 = [w.detach().float().contiguous() for w in weights]
    arr = (ctypes.c_void_p * len(w32))(*[w.data_ptr() for w in w32])
    check(lib.ipoke_gru_unroll_forward(byref(d), ptr(x0_t), x0_t.shape[1], ptr(h0_t), h0_t.shape[1], arr, ptr(ws), ptr(out), ldo, ops._dt(dtype),
                                       _lib.current_stream()))
    return out, ws


class _GruUnrollFn(torch.autograd.Function):
    """All T steps of the stacked ConvGRU (rnn.py:59-133 as first_stage_motion_model.py:503-514 drives it) as ONE autograd node whose two
    directions are issued natively (csrc/gru.hip): (x0 [M, ld], h0 [M, ld], per cell w_ur, b_ur, w_o, b_o) -> the last cell's hidden states of
    all steps, [T * M, ld] ordered (step, clip) -- the batch the frame-batched decoder consumes."""

    @staticmethod
    def forward(ctx, x0_t, h0_t, geom, dtype, *weights):
        out, ws = gru_unroll_forward(weights, x0_t.contiguous(), h0_t.contiguous(), geom, dtype)
        ctx.geom, ctx.dtype = geom, dtype
        ctx.shapes = (tuple(x0_t.shape), tuple(h0_t.shape))
        ctx.save_for_backward(ws, *weights)
        return out

    @staticmethod
    def backward(ctx, d_out):
        ws, *weights = ctx.saved_tensors
        B, T, L, Cx, Ch, H, W = ctx.geom
        dt = ctx.dtype
        M = B * H * W
        ldo = K.round_up(Ch, K.e16(dt))
        g = d_out.contiguous()
        if g.dtype != _tdt(dt) or g.shape[1] != ldo:
            g = pad_cols(g[:, :min(g.shape[1], ldo)], ldo, dt)
        dws = [torch.empty(w.shape, dtype=torch.float32, device=g.device) for w in weights]
        d_x0 = torch.empty(M, Cx, dtype=torch.float32, device=g.device)
        d_h0 = torch.empty(M, Ch, dtype=torch.float32, device=g.device)
        arr = (ctypes.c_void_p * len(dws))(*[w.data_ptr() for w in dws])
        d = _gru_desc(*ctx.geom)
        check(_lib.lib().ipoke_gru_unroll_backward(byref(d), ptr(g), ldo, ptr(ws), arr, ptr(d_x0), ptr(d_h0), ops._dt(dt), _lib.current_stream()))
        (sx, sh) = ctx.shapes
        return pad_cols(d_x0, sx[1], dt), pad_cols(d_h0, sh[1], dt), None, None, *dws


def gru_unroll(rnn, in_rnn, h0, steps, dtype, gate_w=None):
    """ConvGRU.run over ``steps`` steps from the shared initial state ``h0`` with the constant input ``in_rnn`` (differentiable):
    CL of steps * B images ordered (step, clip)."""
    cells = list(rnn.cells)
    if gate_w is None:
        gate_w = [gru_gate_weights(c) for c in cells]
    weights = []
    for c, (w_ur, b_ur) in zip(cells, gate_w):
        weights += [w_ur, b_ur, c.out_gate.weight, c.out_gate.bias]
    geom = (in_rnn.N, steps, len(cells), in_rnn.C, h0.C, in_rnn.dhw[1], in_rnn.dhw[2])
    out = _GruUnrollFn.apply(in_rnn.t, h0.t, geom, dtype, *weights)
    return K.CL(out, steps * in_rnn.N, in_rnn.dhw, h0.C)


# ------------------------------------------------------------------------------------------------ latent
class _ReparamFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mulv_t, eps_s, Z, dtype):
        M = mulv_t.shape[0]
        z = torch.empty(M, Z, device=mulv_t.device); mu = torch.empty_like(z); lv = torch.empty_like(z)
        check(_lib.lib().ipoke_reparameterize(ptr(mulv_t), mulv_t.shape[1], ptr(eps_s), ptr(z), ptr(mu), ptr(lv), M, Z,
                                              ops._dt(dtype), _lib.current_stream()))
        ctx.save_for_backward(mulv_t, eps_s)
        ctx.args = (Z, dtype)
        return z, mu, lv

    @staticmethod
    def backward(ctx, dz, dmu, dlv):
        mulv_t, eps_s = ctx.saved_tensors
        Z, dtype = ctx.args
        M = mulv_t.shape[0]
        out = torch.empty_like(mulv_t)
        cz = lambda t: None if t is None else t.contiguous().float()
        dz, dmu, dlv = cz(dz), cz(dmu), cz(dlv)
        check(_lib.lib().ipoke_reparam_bwd(ptr(mulv_t), mulv_t.shape[1], ptr(eps_s), ptr(dz), ptr(dmu), ptr(dlv), ptr(out),
                                           out.shape[1], M, Z, ops._dt(dtype), _lib.current_stream()))
        return out, None, None, None


class _KLFn(torch.autograd.Function):
    """-0.5 * mean_{b,h,w} sum_c (1 + lv - mu^2 - exp(lv))  (utils/losses.py:47-48) on the [M, Z] latents."""

    @staticmethod
    def forward(ctx, mu, lv):
        mu, lv = mu.contiguous(), lv.contiguous()
        loss = torch.zeros(1, device=mu.device)
        dmu = torch.empty_like(mu); dlv = torch.empty_like(lv)
        check(_lib.lib().ipoke_kl_loss(ptr(mu), ptr(lv), mu.shape[0], mu.shape[1], ptr(loss), ptr(dmu), ptr(dlv), _lib.current_stream()))
        ctx.save_for_backward(dmu, dlv)
        return loss[0]

    @staticmethod
    def backward(ctx, d):
        dmu, dlv = ctx.saved_tensors
        return dmu * d, dlv * d


class _L1TanhFn(torch.autograd.Function):
    """frame = tanh(pre) ; returns (sum_scale |frame - x|, frame) with d/dpre produced in the same pass."""

    @staticmethod
    def forward(ctx, pre_t, x_nchw, scale):
        N, C, H, W = x_nchw.shape
        S = H * W
        frame = torch.tanh(pre_t)                                     # [M, C] fp32: the returned reconstruction
        loss = torch.zeros(1, device=pre_t.device)
        grad = torch.empty_like(pre_t)
        part = torch.empty(int(_lib.lib().ipoke_l1_loss_partials()), device=pre_t.device)     # fixed-order sum: a reproducible value
        assert x_nchw.stride(1) == S and x_nchw.stride(2) == W and x_nchw.stride(3) == 1
        check(_lib.lib().ipoke_l1_loss(ptr(frame), frame.shape[1], ptr(x_nchw), N, C, S, x_nchw.stride(0), float(scale), ptr(loss),
                                       ptr(grad), grad.shape[1], ptr(part), _lib.current_stream()))
        ctx.save_for_backward(grad, frame)
        return loss[0], frame

    @staticmethod
    def backward(ctx, d_loss, d_frame):
        grad, frame = ctx.saved_tensors
        d = grad * d_loss
        if d_frame is not None:              # the reconstruction also feeds the discriminators (GAN terms)
            d = d + d_frame
        return d * (1.0 - frame * frame), None, None


# (mulv [M, >= 2Z], eps, Z, dtype) -> (z, mu, logvar) | (mu, logvar) -> KL | (pre-tanh [M, C], target NCHW, scale) -> (L1, frame)
reparameterize, kl_loss, l1_tanh_loss =_ReparamFn.apply, _KLFn.apply, _L1TanhFn.apply


class MultiTensorAdam:
    """torch.optim.Adam(lr, betas, weight_decay) semantics over a parameter list, one ``ipoke_adam_multi`` launch per 48
    tensors; parameters without a gradient are skipped like torch does.  ``param_groups[0]['lr']`` is the live learning rate
    (schedulers write it, as with a torch optimizer); ``exponential_lr_step(gamma)`` is the reference's per-epoch
    ``ExponentialLR`` (first_stage_motion_model.py:383-386).  One step counter for all tensors: identical to torch's
    per-parameter counters as long as every parameter receives a gradient in every step it takes part in (true for the three
    first-stage optimisers: each owns one network that is always differentiated as a whole)."""

    def __init__(self, params, lr=2e-4, betas=(0.5, 0.9), weight_decay=1e-5, eps=1e-8):
        self.params = [p for p in params if p.requires_grad]
        self.betas, self.weight_decay, self.eps = (float(betas[0]), float(betas[1])), float(weight_decay), float(eps)
        self.param_groups = [{"params": self.params, "lr": float(lr), "initial_lr": float(lr)}]
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.steps = 0
        self.grad_scale = 1.0           # folded into the update: 1 / world for gradients summed over data-parallel ranks

    @property
    def lr(self):
        return float(self.param_groups[0]["lr"])

    @lr.setter
    def lr(self, value):
        self.param_groups[0]["lr"] = float(value)

    def exponential_lr_step(self, gamma):
        """One epoch of torch.optim.lr_scheduler.ExponentialLR(self, gamma)."""
        self.lr = self.lr * float(gamma)

    def state_dict(self):
        return {"steps": self.steps, "lr": self.lr, "initial_lr": self.param_groups[0]["initial_lr"], "betas": self.betas,
                "weight_decay": self.weight_decay, "eps": self.eps, "exp_avg": [t.clone() for t in self.exp_avg],
                "exp_avg_sq": [t.clone() for t in self.exp_avg_sq]}

    def load_state_dict(self, sd):
        if len(sd["exp_avg"]) != len(self.params) or any(a.shape != p.shape for a, p in zip(sd["exp_avg"], self.params)):
            raise ValueError("optimizer state does not match this parameter list")
        with torch.no_grad():
            for dst, src in zip(self.exp_avg, sd["exp_avg"]):
                dst.copy_(src)                      # lands on the parameters' device whatever map_location loaded the file
            for dst, src in zip(self.exp_avg_sq, sd["exp_avg_sq"]):
                dst.copy_(src)
        self.steps = int(sd["steps"])
        self.lr = float(sd["lr"])
        self.param_groups[0]["initial_lr"] = float(sd.get("initial_lr", sd["lr"]))
        self.betas, self.weight_decay, self.eps = tuple(sd["betas"]), float(sd["weight_decay"]), float(sd["eps"])

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        ct = ctypes
        idx = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not idx:
            return
        self.steps += 1
        n = len(idx)
        grads = [self.params[i].grad.contiguous() for i in idx]
        arr = lambda ts: (ct.c_void_p * n)(*[t.data_ptr() for t in ts])
        sizes = (ct.c_int64 * n)(*[self.params[i].numel() for i in idx])
        clear_operand_cache()                      # the update writes through raw pointers: no version bump tells the cache
        check(_lib.lib().ipoke_adam_multi(arr([self.params[i].data for i in idx]), arr(grads), arr([self.exp_avg[i] for i in idx]),
                                          arr([self.exp_avg_sq[i] for i in idx]), sizes, n, self.lr, self.betas[0], self.betas[1],
                                          self.eps, self.weight_decay, self.steps, float(self.grad_scale), _lib.current_stream()))
