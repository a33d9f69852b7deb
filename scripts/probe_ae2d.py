"""Developer probe: time of ``PokeEncoderTrainer.step`` at the shipped size (poke_encoder.yaml: 128 x 128, batch 64), bf16 and f32.

    python scripts/probe_ae2d.py            # writes profiles/ae2d.txt

Each mode is timed in a child process of its own under ``timeout`` (a mode that hangs or faults ends there and nothing further is started on
the device); the parent never touches the GPU.  Nothing in ``ipoke_amd`` or ``bench.py`` imports this file."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, BATCH, WARMUP, STEPS, LIMIT_S = 128, 64, 5, 20, 240


def child(dtype):
    import torch
    from ipoke_amd import configs
    from ipoke_amd.autoencoder2d import ConvPokeAE, PokeEncoderTrainer
    from ipoke_amd.utils.detfill import deterministic_fill_
    model = ConvPokeAE(configs.poke_encoder_train_config(SIZE), dtype=dtype)
    deterministic_fill_(model)
    model = model.cuda()
    flow = (0.6 * torch.randn(BATCH, 2, SIZE, SIZE, generator=torch.Generator().manual_seed(3))).cuda()
    batch = {"flow": flow, "poke": flow}
    trainer = PokeEncoderTrainer(model)
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
    print(f"ae2d step {SIZE}x{SIZE} B={BATCH} {dtype}: min {times[0]:.3f} median {times[len(times) // 2]:.3f} max {times[-1]:.3f} ms over {STEPS} steps "
          f"(warm-up {WARMUP}); loss {out['train/loss'].item():.4f}")


def main():
    lines = []
    for dtype in ("bf16", "f32"):
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", dtype], capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"ae2d step {dtype}: child ended with status {r.returncode}; nothing further was started\n{r.stderr[-2000:]}")
            break
        lines.append(r.stdout.strip().splitlines()[-1])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ae2d.txt"), "w") as f:
        f.write(text)
    return 0 if len(lines) == 2 and "status" not in text else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main())
