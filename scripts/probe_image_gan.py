"""Developer probe: time of ``ImageEncoderGANTrainer.step`` in the adversarial phase at the shipped size (img_encoder.yaml: 64 x 64,
batch 128), bf16 and f32, beside the reconstruction step of ``ImageEncoderTrainer`` on the same batch for scale.

    python scripts/probe_image_gan.py            # writes profiles/image_gan.txt

Each (mode, phase) is timed in a child process of its own under ``timeout`` (a child that hangs or faults ends there and nothing further
is started on the device); the parent never touches the GPU.  Nothing in ``ipoke_amd`` or ``bench.py`` imports this file."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, BATCH, WARMUP, STEPS, LIMIT_S = 64, 128, 5, 20, 240


def child(dtype, phase):
    import torch
    from ipoke_amd import configs
    from ipoke_amd.autoencoder2d import ConvAEModel, ImageEncoderTrainer
    from ipoke_amd.image_gan import ConvAEGANModel, ImageEncoderGANTrainer
    from ipoke_amd.utils.detfill import deterministic_fill_
    conf = configs.img_encoder_train_config(SIZE)
    model = (ConvAEGANModel if phase == "adversarial" else ConvAEModel)(conf, dtype=dtype)
    deterministic_fill_(model)
    model = model.cuda()
    if phase == "adversarial":
        model.current_epoch = conf["training"]["pretrain"]
    x = (torch.rand(BATCH, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    batch = {"images": x.unsqueeze(1)}
    trainer = (ImageEncoderGANTrainer if phase == "adversarial" else ImageEncoderTrainer)(model)
    for _ in range(WARMUP):
        trainer.step(batch)
    torch.cuda.synchronize()
    times = []
    for _ in range(STEPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = trainer.step(batch)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    print(f"image autoencoder {phase} step {SIZE}x{SIZE} B={BATCH} {dtype}: min {times[0]:.3f} median {times[len(times) // 2]:.3f} max {times[-1]:.3f} ms "
          f"over {STEPS} steps (warm-up {WARMUP}); loss {out['train/loss'].item():.4f}")


def main():
    lines, ok = [], True
    for dtype in ("bf16", "f32"):
        for phase in ("reconstruction", "adversarial"):
            r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", dtype, phase],
                               capture_output=True, text=True)
            if r.returncode != 0:
                lines.append(f"{phase} step {dtype}: child ended with status {r.returncode}; nothing further was started\n{r.stderr[-2000:]}")
                ok = False
                break
            lines.append(r.stdout.strip().splitlines()[-1])
        if not ok:
            break
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "image_gan.txt"), "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
