// Input pipeline on the device (reference data/base_dataset.py): optical-flow resize (_get_flow :651-693) and the poke
// simulation from a flow field (_get_poke :507-648), batched -- one workgroup per sample for the statistics / selection,
// a pixel-parallel fill for the poke tensors.  Byte/index work plus a few reductions: nothing here touches the matrix cores.
#include "common.h"

#include <cmath>
#include <cstring>

using namespace ipoke;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
static int grid1(long n, int cap = 4096) { long g = (n + 255) / 256; if (g < 1) g = 1; if (g > cap) g = cap; return (int)g; }

// ---------------------------------------------------------------------------------------------- _get_flow
// dst[b][c][y][x] = bilinear(src[b][c] / div) with align_corners=True; the division comes first, as in the reference
__global__ void flow_resize_kernel(const float* __restrict__ src, float* __restrict__ dst, int BC, int Hi, int Wi, int Ho, int Wo, float div) {
  const long total = (long)BC * Ho * Wo;
  const float sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % Wo); long t = i / Wo;
    const int oy = (int)(t % Ho); const long bc = t / Ho;
    const float fy = oy * sy, fx = ox * sx;
    const int y0 = min((int)fy, Hi - 1), x0 = min((int)fx, Wi - 1);
    const int y1 = min(y0 + 1, Hi - 1), x1 = min(x0 + 1, Wi - 1);
    const float wy = fy - (float)y0, wx = fx - (float)x0;
    const float* p = src + bc * Hi * Wi;
    const float a = __fdiv_rn(p[y0 * Wi + x0], div), b = __fdiv_rn(p[y0 * Wi + x1], div);
    const float c = __fdiv_rn(p[y1 * Wi + x0], div), d = __fdiv_rn(p[y1 * Wi + x1], div);
    dst[i] = (1.f - wy) * ((1.f - wx) * a + wx * b) + wy * ((1.f - wx) * c + wx * d);
  }
}

// ---------------------------------------------------------------------------------------------- _get_poke
constexpr int kPokeThreads = 1024;
constexpr int kMaxPokes = 16;
struct PokeArgs {
  const float* flow; int B, H, W, poke_size, n_pokes, fix_n_pokes;
  const int* zero; const float* u; float* amp; int* sel; long long* centers; int* status;
  const uint8_t* mask; float* amp_filt;                        // the masked instantiation only
};

// |(vx, vy)| as torch.norm(flow, 2, dim=0) forms it in fp32: the two squares, their sum and the root each rounded on its own.  Plain operators
// with contraction switched off (the __f*_rn intrinsics may be fused, see the augmentation code below) and sqrtf, which hipcc rounds correctly
// by default: __fsqrt_rn is the hardware's approximate root here, one ulp off for a share of its arguments.
__device__ __forceinline__ float flow_amplitude(float vx, float vy) {
#pragma clang fp contract(off)
  const float xx = vx * vx, yy = vy * vy;
  const float ss = xx + yy;
  return sqrtf(ss);
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;
}
__device__ __forceinline__ float block_minmax(float v, bool want_max, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(v, o, 64); v = want_max ? fmaxf(v, w) : fminf(v, w); }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) t = want_max ? fmaxf(t, red[i]) : fminf(t, red[i]);
  return t;
}
// exclusive prefix of one int per thread; returns the prefix, *total = block sum
__device__ __forceinline__ int block_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { if (i < w) base += sh[i]; tot += sh[i]; }
  *total = tot;
  return base + inc - v;
}
// k-th smallest (0-based) of n non-negative floats by a 4 x 8-bit radix select on the bit patterns
__device__ float kth_smallest(const float* a, int n, int k, int* hist) {
  unsigned prefix = 0, mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const unsigned b = __float_as_uint(a[i]);
      if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255], 1);
    }
    __syncthreads();
    int acc = 0, d = 0;
    for (; d < 256; ++d) { if (acc + hist[d] > k) break; acc += hist[d]; }     // every thread walks the same 256 counters
    k -= acc;
    prefix |= (unsigned)d << shift; mask |= 255u << shift;
  }
  return __uint_as_float(prefix);
}

enum { SEL_GT2 = 0, SEL_GT1 = 1, SEL_GT0 = 2, SEL_LT = 3 };
__device__ __forceinline__ bool sel_test(int mode, float v, float t) { return mode == SEL_LT ? v < t : v > t; }

// positions (row-major order inside the window) of the picks[j]-th element passing the test, j < npick
__device__ void pick_positions(const float* a, int n, int mode, float thr, const int* picks, int npick, int* out, int* sh) {
  const int per = (n + blockDim.x - 1) / blockDim.x, lo = threadIdx.x * per, hi = min(n, lo + per);
  int cnt = 0;
  for (int i = lo; i < hi; ++i) cnt += sel_test(mode, a[i], thr);
  int total;
  const int off = block_scan(cnt, sh, &total);
  for (int j = 0; j < npick; ++j) {
    const int k = picks[j];
    if (k >= off && k < off + cnt) {
      int seen = off;
      for (int i = lo; i < hi; ++i)
        if (sel_test(mode, a[i], thr)) { if (seen == k) { out[j] = i; break; } ++seen; }
    }
  }
  __syncthreads();
}

// kMasked = false is _get_poke with filter_flow off.  kMasked = true (filter_flow on, :520-538 and :577-583) keeps a second window array:
// for an ordinary sample amp_filt = mask ? amp : 0, which supplies the statistics and the candidates of the first rule, while the two
// fallback rules test the unfiltered amp against those statistics; for a zero-poke sample the statistics and the value sources stay
// with amp, the second array holds the indicator of the mask's background, and the centres are its positions -- the 5th-percentile rule
// only when there is none.
template <bool kMasked>
__global__ __launch_bounds__(kPokeThreads) void poke_select_kernel(PokeArgs p) {
  __shared__ double red_d[16];
  __shared__ float red_f[16];
  __shared__ int sh_i[256];
  __shared__ int picks[kMaxPokes], pos[kMaxPokes], pos_src[kMaxPokes];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int h0 = p.poke_size, w0 = p.poke_size, wh = p.H - 2 * p.poke_size, ww = p.W - 2 * p.poke_size, n = wh * ww;
  const float* fx = p.flow + (long)b * 2 * p.H * p.W;
  const float* fy = fx + (long)p.H * p.W;
  float* a = p.amp + (long)b * n;
  const bool zero = p.zero && p.zero[b];
  const float* u = p.u + (long)b * (1 + 2 * p.n_pokes);
  // amplitude = torch.norm(flow, 2, dim=0) in fp32 without contraction, shifted to min 0, scaled to max 1
  float lo = INFINITY;
  for (int i = tid; i < n; i += blockDim.x) {
    const int y = h0 + i / ww, x = w0 + i % ww;
    const float vx = fx[y * p.W + x], vy = fy[y * p.W + x];
    const float v = flow_amplitude(vx, vy);
    a[i] = v; lo = fminf(lo, v);
  }
  lo = block_minmax(lo, false, red_f);
  float hi = -INFINITY;
  for (int i = tid; i < n; i += blockDim.x) { const float v = __fsub_rn(a[i], lo); a[i] = v; hi = fmaxf(hi, v); }
  hi = block_minmax(hi, true, red_f);
  double s = 0.0;
  const float* st = a;                                               // the array the statistics are taken of
  if constexpr (kMasked) {
    float* af = p.amp_filt + (long)b * n;
    const uint8_t* m = p.mask + (long)b * p.H * p.W;
    if (!zero) st = af;
    for (int i = tid; i < n; i += blockDim.x) {
      const float v = __fdiv_rn(a[i], hi);
      const bool fg = m[(h0 + i / ww) * p.W + w0 + i % ww] != 0;
      const float f = zero ? (fg ? 0.f : 1.f) : (fg ? v : 0.f);
      a[i] = v; af[i] = f; s += (double)(zero ? v : f);
    }
  } else {
    for (int i = tid; i < n; i += blockDim.x) { const float v = __fdiv_rn(a[i], hi); a[i] = v; s += (double)v; }
  }
  const double mean_d = block_sum_d(s, red_d) / (double)n;
  double q = 0.0;
  for (int i = tid; i < n; i += blockDim.x) { const double d = (double)st[i] - mean_d; q += d * d; }
  const float mean = (float)mean_d, stdv = (float)sqrt(block_sum_d(q, red_d) / (double)(n - 1));
  const float t2 = __fadd_rn(mean, __fmul_rn(stdv, 2.0f)), t1 = __fadd_rn(mean, stdv);

  // candidate counts of every rule in one pass
  int c2 = 0, c1 = 0, c0 = 0;
  for (int i = tid; i < n; i += blockDim.x) { const float v = a[i]; c2 += st[i] > t2; c1 += v > t1; c0 += v > mean; }
  int n2, n1, n0;
  block_scan(c2, sh_i, &n2); block_scan(c1, sh_i, &n1); block_scan(c0, sh_i, &n0);
  int cand_mode, cand_cnt = 0; float cand_thr;
  const float* cand_a = a;                                           // the array the centres are picked from
  int src_cnt = 0; float src_thr = t1;
  if (zero) {
    int nb = 0;
    if constexpr (kMasked) {                                         // the background of the mask, where there is any (:534-536)
      const float* af = p.amp_filt + (long)b * n;
      int cb = 0;
      for (int i = tid; i < n; i += blockDim.x) cb += af[i] > 0.5f;
      block_scan(cb, sh_i, &nb);
      if (nb > 0) { cand_a = af; cand_mode = SEL_GT0; cand_thr = 0.5f; cand_cnt = nb; }
    }
    if (nb == 0) {
      // np.percentile(amplitude, 5), linear interpolation between the two neighbouring order statistics
      const double vi = 0.05 * (double)(n - 1);
      const int k = (int)floor(vi);
      const double g = vi - (double)k;
      const float ak = kth_smallest(a, n, k, sh_i), ak1 = kth_smallest(a, n, min(k + 1, n - 1), sh_i);
      const double diff = (double)ak1 - (double)ak;
      const double pv = g >= 0.5 ? (double)ak1 - diff * (1.0 - g) : (double)ak + diff * g;
      cand_thr = (float)pv; cand_mode = SEL_LT;
      int cl = 0;
      for (int i = tid; i < n; i += blockDim.x) cl += a[i] < cand_thr;
      block_scan(cl, sh_i, &cand_cnt);
    }
    if (n1 > 0) { src_thr = t1; src_cnt = n1; } else { src_thr = mean; src_cnt = n0; }
  } else if (n2 > 0) { cand_a = st; cand_mode = SEL_GT2; cand_thr = t2; cand_cnt = n2; }
  else if (n1 > 0) { cand_mode = SEL_GT1; cand_thr = t1; cand_cnt = n1; }
  else { cand_mode = SEL_GT0; cand_thr = mean; cand_cnt = n0; }

  long long* cen = p.centers + (long)b * p.n_pokes * 2;
  int* sel = p.sel + (long)b * (1 + 4 * p.n_pokes);
  if (cand_cnt == 0 || (zero && src_cnt == 0)) {                      // the reference raises FlowError and resamples
    if (tid == 0) { p.status[b] = 1; sel[0] = 0; }
    for (int i = tid; i < 2 * p.n_pokes; i += blockDim.x) cen[i] = -1;
    return;
  }
  const int np = p.fix_n_pokes ? p.n_pokes : 1 + (int)floor((double)u[0] * (double)min(p.n_pokes, cand_cnt));
  if (tid < np) picks[tid] = (int)floor((double)u[1 + p.n_pokes + tid] * (double)cand_cnt);
  __syncthreads();
  pick_positions(cand_a, n, cand_mode == SEL_LT ? SEL_LT : SEL_GT0, cand_thr, picks, np, pos, sh_i);
  if (zero) {
    if (tid < np) picks[tid] = (int)floor((double)u[1 + tid] * (double)src_cnt);
    __syncthreads();
    pick_positions(a, n, SEL_GT0, src_thr, picks, np, pos_src, sh_i);
  }
  if (tid == 0) { p.status[b] = 0; sel[0] = np; }
  if (tid < p.n_pokes) {
    const bool on = tid < np;
    const int r = on ? h0 + pos[tid] / ww : -1, c = on ? w0 + pos[tid] % ww : -1;
    cen[2 * tid] = r; cen[2 * tid + 1] = c;
    int* e = sel + 1 + 4 * tid;
    e[0] = r; e[1] = c;
    e[2] = on ? (zero ? h0 + pos_src[tid] / ww : r) : -1;
    e[3] = on ? (zero ? w0 + pos_src[tid] % ww : c) : -1;
  }
}

// _compute_mask_with_flow (:343-351), one workgroup per sample over the whole H x W map: amplitude as above, shifted to min 0, scaled to
// max 1, mask = amplitude > mean + std (double sums in a fixed order, the threshold one fp32 add).  A constant map is 0 / 0 everywhere:
// no pixel passes and the sample is flagged.
__global__ __launch_bounds__(kPokeThreads) void flow_mask_kernel(const float* __restrict__ flow, int H, int W, float* __restrict__ amp,
                                                                  uint8_t* __restrict__ mask, int* __restrict__ status) {
  __shared__ double red_d[16];
  __shared__ float red_f[16];
  const int b = blockIdx.x, tid = threadIdx.x, n = H * W;
  const float* fx = flow + (long)b * 2 * n;
  const float* fy = fx + n;
  float* a = amp + (long)b * n;
  uint8_t* m = mask + (long)b * n;
  float lo = INFINITY;
  for (int i = tid; i < n; i += blockDim.x) {
    const float vx = fx[i], vy = fy[i];
    const float v = flow_amplitude(vx, vy);
    a[i] = v; lo = fminf(lo, v);
  }
  lo = block_minmax(lo, false, red_f);
  float hi = -INFINITY;
  for (int i = tid; i < n; i += blockDim.x) { const float v = __fsub_rn(a[i], lo); a[i] = v; hi = fmaxf(hi, v); }
  hi = block_minmax(hi, true, red_f);
  double s = 0.0;
  for (int i = tid; i < n; i += blockDim.x) { const float v = __fdiv_rn(a[i], hi); a[i] = v; s += (double)v; }
  const double mean_d = block_sum_d(s, red_d) / (double)n;
  double q = 0.0;
  for (int i = tid; i < n; i += blockDim.x) { const double d = (double)a[i] - mean_d; q += d * d; }
  const float thr = __fadd_rn((float)mean_d, (float)sqrt(block_sum_d(q, red_d) / (double)(n - 1)));
  for (int i = tid; i < n; i += blockDim.x) m[i] = a[i] > thr ? 1 : 0;
  if (tid == 0) status[b] = hi > 0.f ? 0 : 1;
}

// poke[b][ch][y][x] = value of the LAST poke whose window covers (y, x) (later pokes overwrite earlier ones), else 0;
// flow_out (optional): the sample's flow, zeroed for zero-poke samples (_get_flow :680-681)
__global__ void poke_fill_kernel(const float* __restrict__ flow, const int* __restrict__ sel_all, const int* __restrict__ zero, float* __restrict__ poke,
                                 float* __restrict__ flow_out, int B, int H, int W, int half, int n_pokes, int equal_val) {
  const long total = (long)B * H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W); long t = i / W;
    const int y = (int)(t % H); const int b = (int)(t / H);
    const int* sel = sel_all + (long)b * (1 + 4 * n_pokes);
    const float* f = flow + (long)b * 2 * H * W;
    float v0 = 0.f, v1 = 0.f;
    for (int j = sel[0] - 1; j >= 0; --j) {
      const int r = sel[1 + 4 * j], c = sel[2 + 4 * j];
      if (abs(y - r) <= half && abs(x - c) <= half) {
        const int sr = sel[3 + 4 * j] + (equal_val ? 0 : y - r), sc = sel[4 + 4 * j] + (equal_val ? 0 : x - c);
        v0 = f[sr * W + sc]; v1 = f[(long)H * W + sr * W + sc];
        break;
      }
    }
    float* o = poke + (long)b * 2 * H * W;
    o[y * W + x] = v0; o[(long)H * W + y * W + x] = v1;
    if (flow_out) {
      const bool z = zero && zero[b];
      float* fo = flow_out + (long)b * 2 * H * W;
      fo[y * W + x] = z ? 0.f : f[y * W + x]; fo[(long)H * W + y * W + x] = z ? 0.f : f[(long)H * W + y * W + x];
    }
  }
}

// ---------------------------------------------------------------------------------------------- clip augmentation
// _get_color_transforms / _get_geometric_transforms (:695-722) as the reference applies them per frame through PIL (:432-440) and to the
// flow (:683-691), restated on integers and floats at Pillow's precisions so that the result is bit-equal.  Products and sums are rounded
// separately everywhere: an FMA changes results.  Every function with float arithmetic switches contraction off for its body and uses the
// plain operators: the __f*_rn intrinsics are inline functions compiled under the default, contraction allowed, so hipcc fuses a
// __fmul_rn into the __fadd_rn that consumes it ((u / 255) * 2 - 1 written with them became one v_fma_f32).  `/` is IEEE division (hipcc's
// default, correctly rounded divide).
__device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// Image.blend(degenerate, image, f) on one uint8 value
__device__ __forceinline__ int aug_blend(int deg, int x, float f) {
#pragma clang fp contract(off)
  const float p = f * (float)(x - deg);
  const float t = (float)deg + p;
  if (f >= 0.f && f <= 1.f) return (int)t;
  return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}
// convert("L")
__device__ __forceinline__ int aug_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }
// convert("HSV"): fp32 ratios, the hue offset and the two scalings in double -- Pillow's mixture, and the only one that reproduces it
__device__ __forceinline__ void aug_rgb2hsv(int r, int g, int b, int* h, int* s) {
#pragma clang fp contract(off)
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  if (maxc == minc) { *h = 0; *s = 0; return; }
  const float cr = (float)(maxc - minc);
  const float sf = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float hf;
  if (r == maxc) hf = bc - gc;
  else if (g == maxc) hf = (float)(2.0 + (double)rc - (double)bc);
  else hf = (float)(4.0 + (double)gc - (double)rc);
  const double w = (double)hf / 6.0 + 1.0;               // in [5/6, 11/6]: fmod(w, 1) == w - floor(w), exactly
  hf = (float)(w - floor(w));
  *h = aug_clip8((int)((double)hf * 255.0));
  *s = aug_clip8((int)((double)sf * 255.0));
}
// round() of a value >= 0: half away from zero
__device__ __forceinline__ int aug_round(float v) {
#pragma clang fp contract(off)
  const float w = v + 0.5f;
  return aug_clip8((int)floorf(w));
}
// convert("RGB") of an HSV pixel, fp32
__device__ __forceinline__ void aug_hsv2rgb(int h, int s, int v, int* r, int* g, int* b) {
#pragma clang fp contract(off)
  if (s == 0) { *r = *g = *b = v; return; }
  const float h6 = (float)h * 6.f / 255.f;
  const float fi = floorf(h6), f = h6 - fi, fs = (float)s / 255.f, vf = (float)v;
  const float fsf = fs * f, fsg = fs * (1.f - f);
  const float vp = vf * (1.f - fs), vq = vf * (1.f - fsf), vt = vf * (1.f - fsg);
  const int p = aug_round(vp), q = aug_round(vq), t = aug_round(vt);
  switch ((int)fi % 6) {
    case 0: *r = v; *g = t; *b = p; break;
    case 1: *r = q; *g = v; *b = p; break;
    case 2: *r = p; *g = v; *b = t; break;
    case 3: *r = p; *g = q; *b = v; break;
    case 4: *r = t; *g = p; *b = v; break;
    default: *r = v; *g = p; *b = q; break;
  }
}
// ToTensor and post_T (:105): (u / 255) * 2 - 1
__device__ __forceinline__ float aug_to_float(int u) {
#pragma clang fp contract(off)
  const float x = (float)u / 255.f;
  const float y = x * 2.f;
  return y - 1.f;
}
// pad(S/2, reflect) -> Image.transform(AFFINE, NEAREST) -> center_crop(S) for output pixel (y, x): Pillow's 16.16 fixed-point walk, with
// its 32-bit wrap-around.  Returns false where the padded image has no pixel (fill), else the offset of the source pixel in the S x S frame.
__device__ __forceinline__ bool aug_source(const int* __restrict__ a, int S, int y, int x, int* src) {
  const int P = S >> 1;
  const unsigned X = (unsigned)(x + P), Y = (unsigned)(y + P);
  const int xi = (int)((unsigned)a[2] + (unsigned)a[0] * X + (unsigned)a[1] * Y) >> 16;
  const int yi = (int)((unsigned)a[5] + (unsigned)a[3] * X + (unsigned)a[4] * Y) >> 16;
  if (xi < 0 || xi >= 2 * S || yi < 0 || yi >= 2 * S) return false;
  const int sx = xi < P ? P - xi : xi >= P + S ? 2 * (S - 1) - (xi - P) : xi - P;      // numpy's "reflect": the edge is not repeated
  const int sy = yi < P ? P - yi : yi >= P + S ? 2 * (S - 1) - (yi - P) : yi - P;
  *src = sy * S + sx;
  return true;
}

constexpr int kAugMeanThreads = 256;
// mean_l[frame] = int(sum of L over the brightness-adjusted frame / S^2 + 0.5), one workgroup per frame, integer sums in a fixed order
__global__ __launch_bounds__(kAugMeanThreads) void aug_frame_means_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ colour, int T,
                                                                           int S, int* __restrict__ mean_l) {
#pragma clang fp contract(off)
  __shared__ unsigned long long red[kAugMeanThreads / 64];
  const int frame = blockIdx.x, n = S * S;
  const float fb = colour[(long)(frame / T) * 3];
  const uint8_t* p = frames + (long)frame * n * 3;
  unsigned long long sum = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    sum += (unsigned)aug_luma(aug_blend(0, p[3 * (long)i], fb), aug_blend(0, p[3 * (long)i + 1], fb), aug_blend(0, p[3 * (long)i + 2], fb));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int i = 0; i < kAugMeanThreads / 64; ++i) t += red[i];
    mean_l[frame] = (int)((double)t / (double)n + 0.5);
  }
}

// out[frame][c][y][x] = the colour chain of the source pixel of (y, x), as (u / 255) * 2 - 1; fill pixels are uint8 0, i.e. -1
__global__ void aug_frames_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ colour, const int* __restrict__ hue_add,
                                  const int* __restrict__ mean_l, const int* __restrict__ affine, long frames_n, int T, int S, float* __restrict__ out) {
  const long n = (long)S * S, total = frames_n * n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % S); long t = i / S;
    const int y = (int)(t % S); const long frame = t / S;
    const int b = (int)(frame / T);
    int r = 0, g = 0, bl = 0, src;
    if (aug_source(affine + (long)b * 6, S, y, x, &src)) {
      const uint8_t* p = frames + (frame * n + src) * 3;
      const float fb = colour[(long)b * 3], fc = colour[(long)b * 3 + 1], fs = colour[(long)b * 3 + 2];
      const int m = mean_l[frame];
      r = aug_blend(m, aug_blend(0, p[0], fb), fc); g = aug_blend(m, aug_blend(0, p[1], fb), fc); bl = aug_blend(m, aug_blend(0, p[2], fb), fc);
      int h, s;
      const int v = max(r, max(g, bl));
      aug_rgb2hsv(r, g, bl, &h, &s);
      aug_hsv2rgb((h + hue_add[b]) & 255, s, v, &r, &g, &bl);
      const int l = aug_luma(r, g, bl);
      r = aug_blend(l, r, fs); g = aug_blend(l, g, fs); bl = aug_blend(l, bl, fs);
    }
    float* o = out + frame * 3 * n + (long)y * S + x;
    o[0] = aug_to_float(r); o[n] = aug_to_float(g); o[2 * n] = aug_to_float(bl);
  }
}

// out[b][c][y][x] = flow[b][c] at the source pixel of (y, x), 0 where the padded image has none; the vectors are not rotated (:683-691)
__global__ void aug_flow_kernel(const float* __restrict__ flow, const int* __restrict__ affine, long planes, int C, int S, float* __restrict__ out) {
  const long n = (long)S * S, total = planes * n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % S); long t = i / S;
    const int y = (int)(t % S); const long plane = t / S;
    int src;
    out[i] = aug_source(affine + (plane / C) * 6, S, y, x, &src) ? flow[plane * n + src] : 0.f;
  }
}

// ==============================================================================================
extern "C" int ipoke_flow_resize(const float* src, float* dst, int B, int C, int Hi, int Wi, int Ho, int Wo, float divide_by, void* stream) {
  IPK_REQUIRE(src && dst && B >= 1 && C >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1 && divide_by != 0.f, "bad arguments");
  hipLaunchKernelGGL(flow_resize_kernel, dim3(grid1((long)B * C * Ho * Wo)), dim3(256), 0, STREAM(stream), src, dst, B * C, Hi, Wi, Ho, Wo, divide_by);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int64_t ipoke_poke_workspace_bytes(int B, int H, int W, int poke_size, int n_pokes) {
  const long n = (long)(H - 2 * poke_size) * (W - 2 * poke_size);
  return (int64_t)B * (n * (long)sizeof(float) + (1 + 4L * n_pokes) * (long)sizeof(int));
}

static int poke_simulate(const float* flow, int B, int H, int W, int poke_size, int n_pokes, int fix_n_pokes, int equal_poke_val,
                         const int* zero_poke, const float* u, const uint8_t* mask, float* poke, int64_t* centers, float* flow_out, int* status,
                         void* workspace, void* stream) {
  IPK_REQUIRE(flow && u && poke && centers && status && workspace, "null argument");
  IPK_REQUIRE(B >= 1 && poke_size >= 1 && n_pokes >= 1 && n_pokes <= kMaxPokes, "bad poke configuration");
  IPK_REQUIRE(H > 2 * poke_size + 1 && W > 2 * poke_size + 1, "the candidate window [poke_size, size - poke_size) is empty");
  const long n = (long)(H - 2 * poke_size) * (W - 2 * poke_size);
  PokeArgs a;
  a.flow = flow; a.B = B; a.H = H; a.W = W; a.poke_size = poke_size; a.n_pokes = n_pokes; a.fix_n_pokes = fix_n_pokes;
  a.zero = zero_poke; a.u = u; a.amp = reinterpret_cast<float*>(workspace); a.mask = mask;
  a.amp_filt = mask ? a.amp + (long)B * n : nullptr;
  a.sel = reinterpret_cast<int*>(a.amp + (mask ? 2 : 1) * (long)B * n); a.centers = reinterpret_cast<long long*>(centers); a.status = status;
  if (mask) hipLaunchKernelGGL(poke_select_kernel<true>, dim3(B), dim3(kPokeThreads), 0, STREAM(stream), a);
  else hipLaunchKernelGGL(poke_select_kernel<false>, dim3(B), dim3(kPokeThreads), 0, STREAM(stream), a);
  hipLaunchKernelGGL(poke_fill_kernel, dim3(grid1((long)B * H * W)), dim3(256), 0, STREAM(stream), flow, a.sel, zero_poke, poke, flow_out, B, H, W,
                     poke_size / 2, n_pokes, equal_poke_val);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_poke_simulate(const float* flow, int B, int H, int W, int poke_size, int n_pokes, int fix_n_pokes, int equal_poke_val,
                                   const int* zero_poke, const float* u, float* poke, int64_t* centers, float* flow_out, int* status, void* workspace,
                                   void* stream) {
  return poke_simulate(flow, B, H, W, poke_size, n_pokes, fix_n_pokes, equal_poke_val, zero_poke, u, nullptr, poke, centers, flow_out, status,
                       workspace, stream);
}

extern "C" int64_t ipoke_poke_masked_workspace_bytes(int B, int H, int W, int poke_size, int n_pokes) {
  const long n = (long)(H - 2 * poke_size) * (W - 2 * poke_size);
  return (int64_t)B * (2 * n * (long)sizeof(float) + (1 + 4L * n_pokes) * (long)sizeof(int));
}

extern "C" int ipoke_poke_simulate_masked(const float* flow, int B, int H, int W, int poke_size, int n_pokes, int fix_n_pokes, int equal_poke_val,
                                          const int* zero_poke, const float* u, const uint8_t* mask, float* poke, int64_t* centers,
                                          float* flow_out, int* status, void* workspace, void* stream) {
  return poke_simulate(flow, B, H, W, poke_size, n_pokes, fix_n_pokes, equal_poke_val, zero_poke, u, mask, poke, centers, flow_out, status,
                       workspace, stream);
}

extern "C" int64_t ipoke_flow_mask_workspace_bytes(int B, int H, int W) { return (int64_t)B * H * W * (long)sizeof(float); }

extern "C" int ipoke_flow_mask(const float* flow, int B, int H, int W, uint8_t* mask, int* status, void* workspace, void* stream) {
  IPK_REQUIRE(flow && mask && status && workspace, "null argument");
  IPK_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long)H * W >= 2 && (long)H * W < (1L << 30), "bad flow shape");
  hipLaunchKernelGGL(flow_mask_kernel, dim3(B), dim3(kPokeThreads), 0, STREAM(stream), flow, H, W, reinterpret_cast<float*>(workspace), mask, status);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

// ---------------------------------------------------------------------------------------------- poke editing
// Python's slice a:b on an axis of `extent` elements for a = c - half, b = c + half + 1: an index below zero wraps ONCE by the extent and
// then clamps at 0, one above the extent clamps at the extent; lo >= hi is the empty slice.
__device__ __forceinline__ void slice_range(long long c, int half, int extent, int* lo, int* hi) {
  long long a = c - half, b = c + half + 1;
  if (a < 0) { a += extent; if (a < 0) a = 0; } else if (a > extent) a = extent;
  if (b < 0) { b += extent; if (b < 0) b = 0; } else if (b > extent) b = extent;
  *lo = (int)a; *hi = (int)b;
}
__device__ __forceinline__ bool square_covers(long long r, long long c, int half, int H, int W, int y, int x) {
  int y0, y1, x0, x1;
  slice_range(r, half, H, &y0, &y1); slice_range(c, half, W, &x0, &x1);
  return y >= y0 && y < y1 && x >= x0 && x < x1;
}

// poke[b][:][y][x] = the value of the LAST poke whose square covers (y, x), else 0.  values [B][n][2], or (values == nullptr) the flow at
// the poke's centre: a centre outside the map has no flow value and is left out in that mode.
__global__ void poke_stamp_kernel(const long long* __restrict__ centers, const float* __restrict__ values, const float* __restrict__ flow,
                                  float* __restrict__ poke, int B, int H, int W, int n, int half, int skip_negative) {
  const long total = (long)B * H * W, HW = (long)H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W); long t = i / W;
    const int y = (int)(t % H); const int b = (int)(t / H);
    float v0 = 0.f, v1 = 0.f;
    for (int j = n - 1; j >= 0; --j) {
      const long long r = centers[((long)b * n + j) * 2], c = centers[((long)b * n + j) * 2 + 1];
      if (skip_negative && (r < 0 || c < 0)) continue;
      if (!values && (r < 0 || r >= H || c < 0 || c >= W)) continue;
      if (!square_covers(r, c, half, H, W, y, x)) continue;
      if (values) { v0 = values[((long)b * n + j) * 2]; v1 = values[((long)b * n + j) * 2 + 1]; }
      else { const float* f = flow + (long)b * 2 * HW + r * W + c; v0 = f[0]; v1 = f[HW]; }
      break;
    }
    float* o = poke + (long)b * 2 * HW + (long)y * W + x;
    o[0] = v0; o[HW] = v1;
  }
}

// _control_sensitivity (second_stage_video.py:798-833), one workgroup per sample: amplitude map -> mean (double, fixed order) -> the
// candidates above it in row-major order -> n_s picks and their re-aimed values.  The map lives in LDS when it fits (amp_ws == nullptr).
constexpr int kMaxRandomPokes = 64;
constexpr long kRandomizeLdsFloats = 16384;          // 128 x 128: 64 KB of the CU's 160 KB, beside ~1.5 KB of reduction scratch
struct RandomizeArgs {
  const float* flow; const long long* centers; const float* u; float* amp_ws; float* val; long long* picked; int* status;
  int B, H, W, n_c, n_s;
};

__global__ __launch_bounds__(kPokeThreads) void poke_randomize_select_kernel(RandomizeArgs p) {
  extern __shared__ float amp_lds[];
  __shared__ double red_d[16];
  __shared__ int sh_i[256];
  __shared__ int picks[kMaxRandomPokes], pos[kMaxRandomPokes];
  const int b = blockIdx.x, tid = threadIdx.x, n = p.H * p.W;
  const float* fx = p.flow + (long)b * 2 * n;
  const float* fy = fx + n;
  float* a = p.amp_ws ? p.amp_ws + (long)b * n : amp_lds;
  double s = 0.0;
  for (int i = tid; i < n; i += blockDim.x) {
    const float vx = fx[i], vy = fy[i];
    const float v = flow_amplitude(vx, vy);
    a[i] = v; s += (double)v;
  }
  const double mean_d = block_sum_d(s, red_d) / (double)n;
  // a > mean_d for an fp32 a  <=>  a > (mean_d rounded DOWN to fp32)
  const float thr = __double2float_rd(mean_d);
  int cnt = 0;
  for (int i = tid; i < n; i += blockDim.x) cnt += a[i] > thr;
  int n_valid;
  block_scan(cnt, sh_i, &n_valid);
  const long long r0 = p.centers[(long)b * p.n_c * 2], c0 = p.centers[(long)b * p.n_c * 2 + 1];
  // no candidate (a constant map: the reference's randint(0) raises) comes first, as in the reference; then the padded first centre
  const int status = n_valid == 0 ? 1 : (r0 < 0 || c0 < 0) ? 2 : 0;
  if (tid == 0) p.status[b] = status;
  long long* picked = p.picked + (long)b * p.n_s * 2;
  float* val = p.val + (long)b * p.n_s * 2;
  if (status != 0) {
    for (int i = tid; i < 2 * p.n_s; i += blockDim.x) { picked[i] = -1; val[i] = 0.f; }
    return;
  }
  const float* u = p.u + (long)b * p.n_s * 2;
  if (tid < p.n_s) { picks[tid] = min((int)floor((double)u[2 * tid] * (double)n_valid), n_valid - 1); pos[tid] = 0; }
  __syncthreads();
  pick_positions(a, n, SEL_GT0, thr, picks, p.n_s, pos, sh_i);
  if (tid < p.n_s) {
    const int q = pos[tid];
    const float phase = a[q], angle = __fmul_rn(3.14159265358979323846f, u[2 * tid + 1]);
    picked[2 * tid] = q / p.W; picked[2 * tid + 1] = q % p.W;
    val[2 * tid] = __fmul_rn(cosf(angle), phase); val[2 * tid + 1] = __fmul_rn(sinf(angle), phase);
  }
}

// pokes[j][b][:][y][x] = val[b][j] inside the square around the sample's FIRST centre, 0 elsewhere and for flagged samples
__global__ void poke_randomize_fill_kernel(const long long* __restrict__ centers, const float* __restrict__ val, const int* __restrict__ status,
                                           float* __restrict__ pokes, int B, int H, int W, int n_c, int n_s, int half) {
  const long HW = (long)H * W, total = (long)n_s * B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W); long t = i / W;
    const int y = (int)(t % H); t /= H;
    const int b = (int)(t % B), j = (int)(t / B);
    const bool on = status[b] == 0 && square_covers(centers[(long)b * n_c * 2], centers[(long)b * n_c * 2 + 1], half, H, W, y, x);
    float* o = pokes + ((long)j * B + b) * 2 * HW + (long)y * W + x;
    o[0] = on ? val[((long)b * n_s + j) * 2] : 0.f;
    o[HW] = on ? val[((long)b * n_s + j) * 2 + 1] : 0.f;
  }
}

extern "C" int ipoke_poke_stamp(const int64_t* centers, const float* values, const float* flow, int B, int H, int W, int n, int half,
                                int skip_negative, float* poke, void* stream) {
  IPK_REQUIRE(centers && poke && (values || flow), "null argument (values or flow must be given)");
  IPK_REQUIRE(B >= 1 && H >= 1 && W >= 1 && n >= 0 && half >= 0, "bad poke configuration");
  hipLaunchKernelGGL(poke_stamp_kernel, dim3(grid1((long)B * H * W)), dim3(256), 0, STREAM(stream), reinterpret_cast<const long long*>(centers),
                     values, flow, poke, B, H, W, n, half, skip_negative);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int64_t ipoke_poke_randomize_workspace_bytes(int B, int H, int W, int n_s) {
  const long n = (long)H * W;
  return (int64_t)B * ((long)n_s * 2 + (n > kRandomizeLdsFloats ? n : 0)) * (long)sizeof(float);
}

extern "C" int ipoke_poke_randomize(const float* flow, const int64_t* centers, const float* u, int B, int H, int W, int n_c, int n_s, int half,
                                    float* pokes, int64_t* picked, int* status, void* workspace, void* stream) {
  IPK_REQUIRE(flow && centers && u && pokes && picked && status && workspace, "null argument");
  IPK_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long)H * W < (1L << 30) && n_c >= 1 && half >= 0, "bad poke configuration");
  IPK_REQUIRE(n_s >= 1 && n_s <= kMaxRandomPokes, "1 <= n_s <= 64 sampled pokes per launch");
  const long n = (long)H * W;
  const bool in_lds = n <= kRandomizeLdsFloats;
  RandomizeArgs a;
  a.flow = flow; a.centers = reinterpret_cast<const long long*>(centers); a.u = u;
  a.val = reinterpret_cast<float*>(workspace); a.amp_ws = in_lds ? nullptr : a.val + (long)B * n_s * 2;
  a.picked = reinterpret_cast<long long*>(picked); a.status = status;
  a.B = B; a.H = H; a.W = W; a.n_c = n_c; a.n_s = n_s;
  const size_t lds = in_lds ? (size_t)n * sizeof(float) : 0;
  // the 128 x 128 map and the static scratch together pass the 64 KB a kernel may use without asking
  IPK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(poke_randomize_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(kRandomizeLdsFloats * sizeof(float))));
  hipLaunchKernelGGL(poke_randomize_select_kernel, dim3(B), dim3(kPokeThreads), lds, STREAM(stream), a);
  hipLaunchKernelGGL(poke_randomize_fill_kernel, dim3(grid1((long)n_s * B * n)), dim3(256), 0, STREAM(stream), a.centers, a.val, status, pokes, B, H,
                     W, n_c, n_s, half);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

// ---------------------------------------------------------------------------------------------- _get_keypoint_poke
// data/base_dataset.py:462-497, the loop at :479-487 for a batch: poke j of sample b is keypoint id = poke_ids[b][j] (< 0: padding),
// col = (int)(x * H), row = (int)(y * W) of its source position -- the products in double, truncated toward zero, spatial_size[0] for x
// and [1] for y as the reference has them --, drawn only inside the valid window (both ends inclusive) as the slice assignment of :484-485
// with the value (tgt - src) * H for BOTH channels (the reference's own asymmetry: spatial_size[0] scales x and y alike), formed in double
// and rounded to fp32 once.  A pixel takes the LAST poke that covers it; the coordinates are recorded whether or not the square was drawn.
struct KpPoke { bool drawn; int row, col; };
__device__ __forceinline__ KpPoke keypoint_poke_of(const double* __restrict__ kp_src, const int* __restrict__ poke_ids, int b, int j, int K, int n_max,
                                                   int H, int W, int h_lo, int h_hi, int w_lo, int w_hi, int* id_out) {
  KpPoke p;
  const int id = poke_ids[(long)b * n_max + j];
  p.drawn = false; p.row = p.col = -1;
  *id_out = id;
  if (id < 0 || id >= K) return p;                  // padding (or an id the host side would have refused): no poke, coordinates -1
  const double* s = kp_src + ((long)b * K + id) * 2;
  p.row = (int)(s[1] * (double)W);
  p.col = (int)(s[0] * (double)H);
  p.drawn = p.col >= w_lo && p.col <= w_hi && p.row >= h_lo && p.row <= h_hi;
  return p;
}

__global__ void keypoint_poke_kernel(const double* __restrict__ kp_src, const double* __restrict__ kp_tgt, const int* __restrict__ poke_ids, int B, int K,
                                     int n_max, int H, int W, int half, int h_lo, int h_hi, int w_lo, int w_hi, float* __restrict__ poke,
                                     int* __restrict__ coords) {
  const long HW = (long)H * W, total = (long)B * HW, stride = (long)gridDim.x * blockDim.x, first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = first; i < (long)B * n_max; i += stride) {
    int id;
    const KpPoke p = keypoint_poke_of(kp_src, poke_ids, (int)(i / n_max), (int)(i % n_max), K, n_max, H, W, h_lo, h_hi, w_lo, w_hi, &id);
    coords[2 * i] = p.row; coords[2 * i + 1] = p.col;
  }
  for (long i = first; i < total; i += stride) {
    const int x = (int)(i % W); long t = i / W;
    const int y = (int)(t % H); const int b = (int)(t / H);
    float v0 = 0.f, v1 = 0.f;
    for (int j = n_max - 1; j >= 0; --j) {
      int id;
      const KpPoke p = keypoint_poke_of(kp_src, poke_ids, b, j, K, n_max, H, W, h_lo, h_hi, w_lo, w_hi, &id);
      if (!p.drawn || !square_covers(p.row, p.col, half, H, W, y, x)) continue;
      const double* s = kp_src + ((long)b * K + id) * 2;
      const double* g = kp_tgt + ((long)b * K + id) * 2;
      v0 = (float)((g[0] - s[0]) * (double)H); v1 = (float)((g[1] - s[1]) * (double)H);
      break;
    }
    float* o = poke + (long)b * 2 * HW + (long)y * W + x;
    o[0] = v0; o[HW] = v1;
  }
}

extern "C" int ipoke_keypoint_poke(const double* kp_src, const double* kp_tgt, const int32_t* poke_ids, int B, int K, int n_max, int H, int W, int half,
                                   int h_lo, int h_hi, int w_lo, int w_hi, float* poke, int32_t* coords, void* stream) {
  IPK_REQUIRE(kp_src && kp_tgt && poke_ids && poke && coords, "null argument");
  IPK_REQUIRE(B >= 1 && K >= 1 && n_max >= 1 && H >= 1 && W >= 1 && half >= 0, "bad poke configuration");
  hipLaunchKernelGGL(keypoint_poke_kernel, dim3(grid1((long)B * H * W)), dim3(256), 0, STREAM(stream), kp_src, kp_tgt, poke_ids, B, K, n_max, H, W,
                     half, h_lo, h_hi, w_lo, w_hi, poke, coords);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

// ---------------------------------------------------------------------------------------------- clip augmentation
static int aug_check_size(int S) {
  IPK_REQUIRE(S >= 2 && S % 2 == 0 && S <= 4096, "the frame size must be even and at most 4096 (16.16 fixed point in 32 bits)");
  return IPOKE_OK;
}

extern "C" int ipoke_aug_frame_means(const uint8_t* frames, const float* colour, int B, int T, int S, int* mean_l, void* stream) {
  IPK_REQUIRE(frames && colour && mean_l, "null argument");
  IPK_REQUIRE(B >= 1 && T >= 1 && (long)B * T <= 0x7fffffffL, "bad clip shape");
  if (int rc = aug_check_size(S)) return rc;
  hipLaunchKernelGGL(aug_frame_means_kernel, dim3(B * T), dim3(kAugMeanThreads), 0, STREAM(stream), frames, colour, T, S, mean_l);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_aug_frames(const uint8_t* frames, const float* colour, const int* hue_add, const int* mean_l, const int* affine, int B, int T,
                                int S, float* out, void* stream) {
  IPK_REQUIRE(frames && colour && hue_add && mean_l && affine && out, "null argument");
  IPK_REQUIRE(B >= 1 && T >= 1, "bad clip shape");
  if (int rc = aug_check_size(S)) return rc;
  const long nf = (long)B * T;
  hipLaunchKernelGGL(aug_frames_kernel, dim3(grid1(nf * S * S)), dim3(256), 0, STREAM(stream), frames, colour, hue_add, mean_l, affine, nf, T, S, out);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_aug_flow(const float* flow, const int* affine, int B, int C, int S, float* out, void* stream) {
  IPK_REQUIRE(flow && affine && out, "null argument");
  IPK_REQUIRE(B >= 1 && C >= 1, "bad flow shape");
  if (int rc = aug_check_size(S)) return rc;
  const long planes = (long)B * C;
  hipLaunchKernelGGL(aug_flow_kernel, dim3(grid1(planes * S * S)), dim3(256), 0, STREAM(stream), flow, affine, planes, C, S, out);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
