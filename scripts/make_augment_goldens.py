#!/usr/bin/env python3
"""Golden G18: the clip augmentation of the reference (data/base_dataset.py:695-722, applied at :432-440 and :683-691) computed by Pillow.

    python scripts/make_augment_goldens.py            # CPU, needs Pillow; writes tests/golden/g18_augment.npz

Run by hand; nothing imports it.  The cases are built with Pillow itself -- ``ImageEnhance.Brightness/Contrast/Color``, the ``HSV`` round
trip of ``adjust_hue``, ``np.pad(mode="reflect")``, ``Image.transform(AFFINE, NEAREST)`` and ``crop`` -- which is the chain torchvision's
PIL backend runs for ``FT.adjust_*``, ``FT.pad``, ``FT.affine`` and ``FT.center_crop``.  While writing, the numpy restatement of
tests/augment_ref.py is asserted against Pillow: all 2^24 colours for RGB -> HSV, HSV -> RGB and RGB -> L, and every case of the file.
Inputs and expected outputs are stored as uint8 (the tests derive the fp32 expectation), the flow as fp32.  The file is written with fixed
zip timestamps, so it regenerates byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import augment_ref as R                     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g18_augment.npz")
MAX_BYTES = 256 * 1024
# config/first_stage.yaml:17-25
SHIPPED = {"augment_b": 0.4, "augment_c": 0.5, "augment_h": 0.15, "augment_s": 0.4, "aug_deg": 15, "aug_trans": (0.1, 0.1)}


# ------------------------------------------------------------------------------------------------ the chain, through Pillow
def pil_colour(img, brightness, contrast, saturation, hue_add):
    """FT.adjust_brightness / adjust_contrast / adjust_hue / adjust_saturation on a PIL RGB image"""
    img = ImageEnhance.Brightness(img).enhance(brightness)
    img = ImageEnhance.Contrast(img).enhance(contrast)
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(hue_add)                       # adjust_hue: np_h += np.uint8(hue_factor * 255), wrapping
    img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return ImageEnhance.Color(img).enhance(saturation)


def pil_geometry(img, angle, tx, ty):
    """FT.pad((S/2, S/2), reflect) -> FT.affine(angle, (tx, ty), 1.0, 0) -> FT.center_crop(S) on a PIL image (RGB or F)"""
    a = np.asarray(img)
    S = a.shape[0]
    P = S // 2
    pad = ((P, P), (P, P)) + (((0, 0),) if a.ndim == 3 else ())
    img = Image.fromarray(np.pad(a, pad, mode="reflect"))
    matrix = R.affine_matrix(angle, tx, ty, S)
    img = img.transform((2 * S, 2 * S), Image.AFFINE, matrix, Image.NEAREST)
    top = int(round((2 * S - S) / 2.0))
    return img.crop((top, top, top + S, top + S))


def pil_frames(frames, colour, hue_add, angle, trans):
    out = np.empty_like(frames)
    for b in range(frames.shape[0]):
        for t in range(frames.shape[1]):
            img = pil_colour(Image.fromarray(frames[b, t]), float(colour[b, 0]), float(colour[b, 1]), float(colour[b, 2]), int(hue_add[b]))
            out[b, t] = np.asarray(pil_geometry(img, float(angle[b]), int(trans[b, 0]), int(trans[b, 1])))
    return out


def pil_flow(flow, angle, trans):
    out = np.empty_like(flow)
    for b in range(flow.shape[0]):
        for c in range(flow.shape[1]):
            img = pil_geometry(Image.fromarray(flow[b, c], mode="F"), float(angle[b]), int(trans[b, 0]), int(trans[b, 1]))
            out[b, c] = np.asarray(img, dtype=np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the restatement against Pillow
def check_conversions():
    """all 2^24 triples through convert("HSV"), convert("RGB") of an HSV image and convert("L")"""
    v = np.arange(256, dtype=np.uint8)
    for r in range(0, 256, 16):
        cube = np.stack(np.meshgrid(v[r:r + 16], v, v, indexing="ij"), -1).reshape(16 * 256, 256, 3)
        rgb = Image.fromarray(cube, "RGB")
        assert np.array_equal(np.asarray(rgb.convert("HSV")), R.rgb_to_hsv(cube)), "RGB -> HSV"
        assert np.array_equal(np.asarray(rgb.convert("L")), R.luma(cube)), "RGB -> L"
        assert np.array_equal(np.asarray(Image.fromarray(cube, "HSV").convert("RGB")), R.hsv_to_rgb(cube)), "HSV -> RGB"
    print("conversions: 3 x 2^24 colours, 0 mismatches")


# ------------------------------------------------------------------------------------------------ inputs
def blocky_frame(rng, S, cell):
    """random colours on a coarse grid under a ramp (per pixel along x, per cell along y) with 2 % of the pixels random: every column
    differs from its neighbour, a wrong row shows at the sprinkled pixels and the cell borders, and the file still compresses"""
    n = -(-S // cell)
    base = np.kron(rng.randint(0, 256, (n, n, 3)), np.ones((cell, cell, 1), dtype=np.int64))[:S, :S]
    y, x = np.mgrid[0:S, 0:S]
    ramp = np.stack([x * 96 // S, (y // cell) * cell * 96 // S, 0 * x], -1)
    f = np.clip(base * 5 // 8 + ramp, 0, 255).astype(np.uint8)
    m = rng.rand(S, S) < 0.02
    f[m] = rng.randint(0, 256, (int(m.sum()), 3))
    return f


def noise_frame(rng, S):
    return rng.randint(0, 256, (S, S, 3)).astype(np.uint8)


def lattice_frame(order):
    """all 16^3 colours with channel values 0, 17, ..., 255 on 64 x 64 pixels: every grey, every tie between maxima, black and white"""
    v = np.arange(16) * 17
    c = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(4096, 3)[:, list(order)]
    return c.reshape(64, 64, 3).astype(np.uint8)


def coded_flow(B, S):
    """channel 0 encodes the column, channel 1 the row (and both the sample): a wrong source pixel cannot go unnoticed"""
    y, x = np.mgrid[0:S, 0:S].astype(np.float32)
    return np.stack([np.stack([(x - S / 2) * 0.25 + 1000 * b, -(y - S / 2) * 0.5 - 1000 * b]) for b in range(B)]).astype(np.float32)


def shipped_draw(rng, S):
    """one draw from the shipped ranges with both coin flips taken"""
    c = SHIPPED
    half = int(c["aug_trans"][0] * S / 2)
    tr = (int(rng.randint(-half, half)) if half > 0 else 0, int(rng.randint(-half, half)) if half > 0 else 0)
    return dict(b=1 + rng.uniform(-c["augment_b"], c["augment_b"]), c=1 + rng.uniform(-c["augment_c"], c["augment_c"]),
                hue=rng.uniform(-c["augment_h"], 2 * c["augment_h"]), s=1 + rng.uniform(-c["augment_s"], c["augment_s"]),
                angle=rng.uniform(-c["aug_deg"], c["aug_deg"]), trans=tr)


IDENTITY = dict(b=1.0, c=1.0, hue=0.0, s=1.0, angle=0.0, trans=(0, 0))


def big_geometry(S, **colour):
    """a large angle and translation: the fill shows"""
    return dict(dict(b=1.0, c=1.0, hue=0.0, s=1.0), angle=140.0, trans=(S // 2, -(S // 4)), **colour)


def build_cases():
    rng = np.random.RandomState(18)
    cases = []
    # (8, 2, 1)
    cases.append((np.stack([noise_frame(rng, 8)[None], noise_frame(rng, 8)[None]]),
                  [dict(shipped_draw(rng, 8), trans=(1, -1)), big_geometry(8, hue=-0.07)]))
    # (30, 3, 2): odd half-size, P = 15
    cases.append((np.stack([np.stack([noise_frame(rng, 30) for _ in range(2)]) for _ in range(3)]),
                  [shipped_draw(rng, 30), big_geometry(30, b=1.7, c=1.9, s=2.5), dict(shipped_draw(rng, 30), b=0.25, c=-0.4, s=-0.8, hue=-0.15)]))
    # (64, 2, 3)
    cases.append((np.stack([np.stack([blocky_frame(rng, 64, 8), noise_frame(rng, 64), blocky_frame(rng, 64, 4)]),
                            np.stack([blocky_frame(rng, 64, 16) for _ in range(3)])]),
                  [dict(shipped_draw(rng, 64), hue=-0.12), big_geometry(64, c=1.5, hue=0.5)]))
    # (128, 2, 2): the shipped size; 12 degrees with the largest shipped shift reflects on all four sides
    cases.append((np.stack([np.stack([blocky_frame(rng, 128, 8), blocky_frame(rng, 128, 16)]) for _ in range(2)]),
                  [dict(shipped_draw(rng, 128), angle=-14.5, trans=(6, -6)), big_geometry(128, s=0.3, hue=-0.5)]))
    # (64, 4, 1): the colour lattice under the identity, a shipped draw, and factors beyond both ends of the blend's clip
    cases.append((np.stack([lattice_frame(o)[None] for o in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1))]),
                  [IDENTITY, dict(shipped_draw(rng, 64), hue=-0.1), dict(IDENTITY, b=1.6, c=2.2, s=3.0, hue=0.3, angle=15.0, trans=(3, -3)),
                   dict(IDENTITY, b=0.5, c=-0.6, s=-1.5, hue=-0.31, angle=-15.0, trans=(-3, 2))]))
    return cases


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    check_conversions()
    out = {}
    cases = build_cases()
    out["n_cases"] = np.int32(len(cases))
    for ci, (frames, sets) in enumerate(cases):
        B, T, S = frames.shape[:3]
        assert len(sets) == B
        colour = np.array([[p["b"], p["c"], p["s"]] for p in sets], dtype=np.float32)
        hue = np.array([p["hue"] for p in sets], dtype=np.float64)
        hue_add = np.array([R.hue_add_of(h) for h in hue], dtype=np.int32)
        angle = np.array([p["angle"] for p in sets], dtype=np.float64)
        trans = np.array([p["trans"] for p in sets], dtype=np.int32)
        affine = np.stack([R.affine_fixed(angle[b], trans[b, 0], trans[b, 1], S) for b in range(B)])
        flow = coded_flow(B, S)
        want = pil_frames(frames, colour, hue_add, angle, trans)
        want_flow = pil_flow(flow, angle, trans)
        got, mean_l = R.augment_frames(frames, colour, hue_add, affine)
        assert np.array_equal(got, want), f"case {ci}: the restatement differs from Pillow in {int((got != want).sum())} values"
        assert np.array_equal(R.augment_flow(flow, affine), want_flow), f"case {ci}: flow"
        n_fill = sum(int((~R.source_index(a, S)[0]).sum()) for a in affine)
        print(f"case {ci}: S {S} B {B} T {T}: {want.size} values and {want_flow.size} flow values equal Pillow's; "
              f"{int((want != frames).any(-1).sum())} pixels changed, {n_fill} fill pixels")
        for k, v in dict(frames=frames, colour=colour, hue=hue, hue_add=hue_add, angle=angle, trans=trans, affine=affine, mean_l=mean_l,
                         out=want, flow=flow, flow_out=want_flow).items():
            out[f"{k}{ci}"] = v
    write_npz(OUT, out)
    size = os.path.getsize(OUT)
    assert size < MAX_BYTES, size
    print(f"wrote {OUT}: {size} bytes")


if __name__ == "__main__":
    main()
