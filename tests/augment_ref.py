"""numpy restatement of the clip augmentation of csrc/data.hip (``ipoke_aug_frame_means``, ``ipoke_aug_frames``, ``ipoke_aug_flow``): the
chain the reference runs per frame on PIL images (data/base_dataset.py:695-722) -- brightness, contrast, hue, saturation, then reflect-pad,
nearest-neighbour affine and centre crop -- as integer and float operations at the precisions Pillow uses.  No Pillow import here:
scripts/make_augment_goldens.py asserts these functions against Pillow itself (all 2^24 colours for the three conversions, every golden case
for the chain), and tests/test_augment_cpu.py pins them against the golden.

Every numpy expression below is one IEEE operation per step (numpy never contracts a product and a sum into an FMA), fp32 where the
operands are ``np.float32`` and double where they are ``np.float64``; the mixture in ``rgb_to_hsv`` is Pillow's and is needed for equality.
"""
import math

import numpy as np

F32 = np.float32


def blend(deg, x, f):
    """Image.blend(degenerate, image, f) on uint8 values: t = deg + f * (x - deg) in fp32, product and sum rounded separately; truncated
    for 0 <= f <= 1, clipped to [0, 255] first otherwise."""
    f = F32(f)
    deg = np.asarray(deg).astype(np.int32)
    x = np.asarray(x).astype(np.int32)
    t = deg.astype(F32) + f * (x - deg).astype(F32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def luma(rgb):
    """convert("L"): (19595 r + 38470 g + 7471 b + 0x8000) >> 16"""
    c = np.asarray(rgb).astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def frame_mean(rgb):
    """int(ImageStat.Stat(frame.convert("L")).mean[0] + 0.5) of one frame [S, S, 3]"""
    l = luma(rgb)
    return int(float(int(l.astype(np.int64).sum())) / float(l.size) + 0.5)


def _clip8(v):
    return np.clip(v, 0, 255)


def rgb_to_hsv(rgb):
    """convert("HSV") on uint8 [..., 3]"""
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = c.max(-1), c.min(-1)
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = ((maxc - v).astype(F32) / cr for v in (r, g, b))
        h_r = bc - gc                                                                  # fp32
        h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(F32)      # double, rounded to fp32 on assignment
        h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(F32)
        h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
        h = np.where(grey, F32(0), h)
        s = np.where(grey, F32(0), s)
    uh = _clip8((h.astype(np.float64) * 255.0).astype(np.int32))
    us = _clip8((s.astype(np.float64) * 255.0).astype(np.int32))
    return np.stack([uh, us, maxc], -1).astype(np.uint8)


def _round_away(x):
    return np.floor(x + F32(0.5)).astype(np.int32)


def hsv_to_rgb(hsv):
    """convert("RGB") of an HSV image, uint8 [..., 3]; fp32 throughout, rounding half away from zero"""
    c = np.asarray(hsv)
    h, s, v = c[..., 0].astype(F32), c[..., 1].astype(F32), c[..., 2].astype(F32)
    h6 = h * F32(6) / F32(255)
    i = np.floor(h6)
    f = h6 - i
    fs = s / F32(255)
    one = F32(1)
    p = _clip8(_round_away(v * (one - fs)))
    q = _clip8(_round_away(v * (one - fs * f)))
    t = _clip8(_round_away(v * (one - fs * (one - f))))
    vi = c[..., 2].astype(np.int32)
    k = i.astype(np.int32) % 6
    table = (((vi, t, p), (q, vi, p), (p, vi, t), (p, q, vi), (t, p, vi), (vi, p, q)))
    out = np.empty(c.shape, dtype=np.int32)
    for ch in range(3):
        out[..., ch] = np.choose(k, [table[j][ch] for j in range(6)])
    grey = c[..., 1] == 0
    out[grey] = vi[grey][:, None]
    return out.astype(np.uint8)


def colour_chain(rgb, brightness, contrast, saturation, hue_add, mean=None):
    """the four colour steps on one frame uint8 [S, S, 3] (or, with ``mean`` given, on any array of pixels of a frame whose
    brightness-adjusted mean luma is ``mean``): -> (uint8 result, mean)"""
    x = blend(0, rgb, brightness)
    if mean is None:
        mean = frame_mean(x)
    x = blend(mean, x, contrast)
    hsv = rgb_to_hsv(x)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(hue_add)) & 255
    x = hsv_to_rgb(hsv)
    x = blend(luma(x)[..., None], x, saturation)
    return x, mean


def hue_add_of(hue_val):
    """adjust_hue's ``np.uint8(hue_factor * 255)``: truncation toward zero, then wrap"""
    if not -0.5 <= hue_val <= 0.5:
        raise ValueError(f"hue_factor {hue_val} is not in [-0.5, 0.5]")
    return int(hue_val * 255) % 256


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def affine_matrix(angle, tx, ty, S):
    """the inverse matrix FT.affine(angle, (tx, ty), 1.0, 0) hands to Image.transform for the 2S x 2S padded image (centre (S, S)),
    in double"""
    a = math.radians(angle)
    m = [math.cos(a), math.sin(a), 0.0, -math.sin(a), math.cos(a), 0.0]
    cx = cy = float(S)
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty) + cx
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty) + cy
    return m


def affine_fixed(angle, tx, ty, S):
    """the 16.16 fixed-point form Pillow's nearest-neighbour path steps through: int32 [6]"""
    m = affine_matrix(angle, tx, ty, S)
    a = (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))
    assert all(-2 ** 31 <= v < 2 ** 31 for v in a)
    return np.array(a, dtype=np.int32)


def source_index(affine, S):
    """(valid bool [S, S], row int [S, S], col int [S, S]): the pixel of the unpadded frame each output pixel of the crop reads"""
    P = S // 2
    a = [int(v) for v in affine]
    Y, X = np.meshgrid(np.arange(S, dtype=np.int64) + P, np.arange(S, dtype=np.int64) + P, indexing="ij")
    xi = (a[2] + a[0] * X + a[1] * Y) >> 16
    yi = (a[5] + a[3] * X + a[4] * Y) >> 16
    valid = (xi >= 0) & (xi < 2 * S) & (yi >= 0) & (yi < 2 * S)

    def refl(p):
        return np.where(p < P, P - p, np.where(p >= P + S, 2 * (S - 1) - (p - P), p - P))

    return valid, np.where(valid, refl(yi), 0), np.where(valid, refl(xi), 0)


def warp(img, affine, fill=0):
    """pad(S/2, reflect) -> affine (nearest, fill) -> centre crop, as one gather; img [S, S] or [S, S, C]"""
    S = img.shape[0]
    assert img.shape[1] == S and S % 2 == 0
    valid, row, col = source_index(affine, S)
    out = img[row, col]
    out[~valid] = fill
    return out


def to_float(u8):
    """ToTensor and x * 2 - 1 on uint8 [..., S, S, 3] -> fp32 [..., 3, S, S]"""
    x = np.asarray(u8).astype(F32) / F32(255) * F32(2) - F32(1)
    return np.ascontiguousarray(np.moveaxis(x, -1, -3))


def augment_frames(frames, colour, hue_add, affine):
    """frames uint8 [B, T, S, S, 3]; colour [B, 3]; hue_add [B]; affine int32 [B, 6] -> (uint8 [B, T, S, S, 3], mean_l int32 [B, T])"""
    B, T = frames.shape[:2]
    out = np.empty_like(frames)
    means = np.empty((B, T), dtype=np.int32)
    for b in range(B):
        for t in range(T):
            x, means[b, t] = colour_chain(frames[b, t], colour[b, 0], colour[b, 1], colour[b, 2], hue_add[b])
            out[b, t] = warp(x, affine[b])
    return out, means


def augment_flow(flow, affine):
    """flow fp32 [B, C, S, S] -> the same geometry, values copied (fill 0)"""
    out = np.empty_like(flow)
    for b in range(flow.shape[0]):
        for c in range(flow.shape[1]):
            out[b, c] = warp(flow[b, c], affine[b], fill=0.0)
    return out
