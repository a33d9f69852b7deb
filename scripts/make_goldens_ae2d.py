"""Golden vectors of the 2-D poke / image autoencoder training step: tests/golden/g19_ae2d.npz.

Runs the REFERENCE's own ``FirstStageWrapper`` (models/modules/autoencoders/fully_conv_models.py: ``ConvEncoder`` + ``ConvDecoder``) in
train mode on the CPU through oracle/ref_import.py.  Run it where the reference checkout is available:

    python scripts/make_goldens_ae2d.py

The reference's Lightning modules ``ConvPokeAE`` / ``ConvAEModel`` are NOT constructed: their ``__init__`` builds an LPIPS network whose
constructor fetches a checkpoint from a URL.  Their six loss lines (conv_poke_encoder.py:68-78 = first_stage_image_conv.py:138-149)
are restated in ``loss_lines`` below; parameter names are the ones those modules' state dicts have (``model.*`` / ``encoder.*`` +
``decoder.*``, ``logvar``, ``disc_factor``, ``disc_weight``, ``perc_weight``), every value the name-keyed deterministic fill.

Cases: (a) poke AE 32 x 32, B = 2, flow_ae; (b) poke AE 64 x 64, B = 3, poke_and_image (5 -> 2 channels); (c) image AE 64 x 64,
B = 2 (tanh); (d) case (a) with the perceptual stand-in p_n = mean((x - rec)^2).

The file is written with fixed zip time stamps, so a rerun reproduces it byte for byte."""
import io
import os
import sys
import zipfile
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ipoke_amd import configs                      # noqa: E402
from ipoke_amd.utils.detfill import fill_value     # noqa: E402
from oracle import ref_import                      # noqa: E402

LOSS_STATE = ("logvar", "disc_factor", "disc_weight", "perc_weight")


def checksum(t, key):
    """sum, abs-sum and three name-keyed sampled elements of a tensor (oracle/make_goldens.py::checksum restated)."""
    t = t.detach().double().flatten()
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    idx = torch.randint(0, t.numel(), (3,), generator=g)
    return np.array([t.sum().item(), t.abs().sum().item(), *t[idx].tolist()])


def standin(target, rec):
    """The perceptual stand-in of case (d): per-sample mean squared error, [N, 1, 1, 1]."""
    return ((target - rec) ** 2).mean(dim=(1, 2, 3), keepdim=True)


def loss_lines(x, rec, logvar, perc_weight, perceptual):
    """conv_poke_encoder.py:68-78 / first_stage_image_conv.py:138-149 (the perceptual term only when a stand-in is given)."""
    rec_loss = torch.abs(x.contiguous() - rec.contiguous())
    if perceptual is not None:
        p_loss = perceptual(x.contiguous(), rec.contiguous())
        rec_loss = rec_loss + perc_weight * p_loss
    nll_loss = rec_loss / torch.exp(logvar) + logvar
    nll_loss = torch.sum(nll_loss) / nll_loss.shape[0]
    return nll_loss


def build(W, config, prefix):
    """The reference autoencoder in train mode + the loss state, filled by state-dict name."""
    net = W.FirstStageWrapper(config).train()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(fill_value(prefix + k, v))
    state = {k: fill_value(k, torch.zeros(())) for k in LOSS_STATE}
    state["logvar"] = torch.nn.Parameter(state["logvar"])
    return net, state


def named(net, state, prefix):
    return [("logvar", state["logvar"])] + [(prefix + k, p) for k, p in net.named_parameters()]


def run_case(W, tag, config, prefix, inputs, select, perceptual, lr, out):
    x_in, target = select(inputs)
    net, state = build(W, config, prefix)
    keys = list(LOSS_STATE) + [prefix + k for k in net.state_dict()]
    shapes = [()] * len(LOSS_STATE) + [tuple(v.shape) for v in net.state_dict().values()]
    out[f"{tag}_keys"] = np.array(keys)
    out[f"{tag}_shapes"] = np.array([",".join(str(s) for s in sh) for sh in shapes])
    for k, v in inputs.items():
        out[f"{tag}_in_{k}"] = v.numpy()
    # ---- one train-mode pass: rec, loss, gradients, u / v after the pass's power iteration
    rec = net(x_in)
    nll = loss_lines(target, rec, state["logvar"], state["perc_weight"], perceptual)
    nll.backward()
    out[f"{tag}_rec"] = rec.detach().numpy()
    out[f"{tag}_nll"] = np.float64(nll.item())
    out[f"{tag}_abs_sum"] = np.float64((target - rec.detach()).abs().double().sum().item())
    out[f"{tag}_dlogvar"] = np.float64(state["logvar"].grad.item())
    out[f"{tag}_logvar"] = np.float32(state["logvar"].item())
    out[f"{tag}_perc_weight"] = np.float32(state["perc_weight"].item())
    params = named(net, state, prefix)
    out[f"{tag}_grad_names"] = np.array([k for k, _ in params])
    out[f"{tag}_grad_checksums"] = np.stack([checksum(p.grad, k) for k, p in params])
    uv = [(prefix + k, v) for k, v in net.state_dict().items() if k.endswith("weight_u") or k.endswith("weight_v")]
    out[f"{tag}_uv_names"] = np.array([k for k, _ in uv])
    out[f"{tag}_uv_checksums"] = np.stack([checksum(v, k) for k, v in uv])
    n_par = sum(p.numel() for _, p in params) - 1
    # ---- two Adam steps from the same start (fresh model: the pass above moved u / v)
    net, state = build(W, config, prefix)
    params = named(net, state, prefix)
    opt = torch.optim.Adam([p for _, p in params], lr=lr, weight_decay=0)
    losses = []
    for _ in range(2):
        opt.zero_grad()
        nll = loss_lines(target, net(x_in), state["logvar"], state["perc_weight"], perceptual)
        nll.backward()
        opt.step()
        losses.append(nll.item())
    out[f"{tag}_step_losses"] = np.array(losses, dtype=np.float64)
    out[f"{tag}_param_checksums"] = np.stack([checksum(p, k) for k, p in params])
    out[f"{tag}_param_absmax"] = np.array([p.detach().abs().max().item() for _, p in params])
    print(f"case {tag}: {n_par} network parameters, {len(keys)} keys; nll {out[f'{tag}_nll']:.6f}, sum|x-rec| {out[f'{tag}_abs_sum']:.4f}, "
          f"d logvar {out[f'{tag}_dlogvar']:.4f}; losses of the two steps {losses}")


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)                        # one summation order whatever the host
    W = ref_import.ref("models.modules.autoencoders.fully_conv_models")
    out = {}

    def flows(seed, B, size):
        g = torch.Generator().manual_seed(seed)
        return {"flow": 0.6 * torch.randn(B, 2, size, size, generator=g)}

    poke_in = lambda d: (d["flow"], d["flow"])
    a = flows(191, 2, 32)
    run_case(W, "a", configs.poke_encoder_train_config(32), "model.", a, poke_in, None, 1e-3, out)
    g = torch.Generator().manual_seed(192)
    b = {"flow": 0.6 * torch.randn(3, 2, 64, 64, generator=g), "poke": 0.6 * torch.randn(3, 2, 64, 64, generator=g),
         "image0": torch.rand(3, 3, 64, 64, generator=g) * 2 - 1}
    run_case(W, "b", configs.poke_encoder_train_config(64, flow_ae=False, poke_and_image=True), "model.", b,
             lambda d: (torch.cat([d["poke"], d["image0"]], dim=1), d["flow"]), None, 1e-3, out)
    g = torch.Generator().manual_seed(193)
    c = {"image": torch.rand(2, 3, 64, 64, generator=g) * 2 - 1}
    run_case(W, "c", configs.img_encoder_train_config(64), "", c, lambda d: (d["image"], d["image"]), None, 2e-4, out)
    run_case(W, "d", configs.poke_encoder_train_config(32), "model.", a, poke_in, standin, 1e-3, out)
    path = os.path.join(ROOT, "tests", "golden", "g19_ae2d.npz")
    write_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
