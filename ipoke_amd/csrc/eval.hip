// Evaluation-side kernels: the FVD metric's I3D network around the implicit-GEMM convolutions (reference utils/metrics.py:
// preprocess :787-800, MaxPool3dTFPadding :939-960, I3D head :1085-1096, activation moments :733-771).
// All of them stream channels-last rows once: HBM-bound element-wise / window work, 16-byte accesses along the channels.
#include "common.h"

#include <cmath>
#include <cstring>

using namespace ipoke;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
static int grid1(long n, int cap = 4096) { long g = (n + 255) / 256; if (g < 1) g = 1; if (g > cap) g = cap; return (int)g; }

// ---------------------------------------------------------------------------------------------- clip -> padded channels-last rows
// float minimum through integer atomics: non-negative floats order like ints, negative ones reversed as unsigned.
// Chosen by the SIGN BIT, not by `v >= 0`: -0.0f compares >= 0 but its bit pattern is INT_MIN, which as a signed integer replaces every
// negative minimum already stored (*minval then ends as -0.0 and ipoke_denorm_if_negative skips a data set that has negative pixels).
// A NaN takes no part, as before.
__device__ __forceinline__ void atomic_min_f32(float* addr, float v) {
  if (v != v) return;
  if (__float_as_int(v) >= 0) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

// One ROUNDED product, as ATen's source index scale * o: contracted into the subtraction that follows it (an fma -- __fmul_rn is a plain
// product and does not prevent that), the weight would come from the exact product while the index comes from the rounded one, up to an
// ulp of the coordinate away from F.interpolate's weight.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// Bilinear resize with align_corners=True of every frame of a strided fp32 clip tensor (frame f of clip n at
// n*s_n + f*s_f, channel c at c*s_c, pixel (y, x) at y*s_h + x*s_w) to Ho x Wo, written as channels-last rows
// dst[(frame*Ho + y)*Wp + pad_l + x][C] with zero columns left and right (the I3D stem reads a 7-pixel window of a row as
// one 21-channel tap, so the TF-SAME zero padding along W is stored).  dst == nullptr: only the minimum is taken.
__global__ void video_to_cl_kernel(const float* __restrict__ src, long s_n, long s_f, long s_c, long s_h, long s_w, int T, int C, int Hi, int Wi,
                                   float* __restrict__ dst, long frames, int Ho, int Wo, int pad_l, int Wp, float* __restrict__ minval) {
  const long total = frames * Ho * Wp;
  const float sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  float lo = INFINITY;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xp = (int)(i % Wp); long t = i / Wp;
    const int oy = (int)(t % Ho); const long fr = t / Ho;
    const int ox = xp - pad_l;
    if (ox < 0 || ox >= Wo) {
      if (dst) for (int c = 0; c < C; ++c) dst[i * C + c] = 0.f;
      continue;
    }
    const float fy = mul_rounded((float)oy, sy), fx = mul_rounded((float)ox, sx);
    const int y0 = min((int)fy, Hi - 1), x0 = min((int)fx, Wi - 1);
    const int y1 = min(y0 + 1, Hi - 1), x1 = min(x0 + 1, Wi - 1);
    const float wy = fy - (float)y0, wx = fx - (float)x0;
    const float* p = src + (fr / T) * s_n + (fr % T) * s_f;
    for (int c = 0; c < C; ++c) {
      const float* q = p + c * s_c;
      const float v = (1.f - wy) * ((1.f - wx) * q[y0 * s_h + x0 * s_w] + wx * q[y0 * s_h + x1 * s_w]) +
                      wy * ((1.f - wx) * q[y1 * s_h + x0 * s_w] + wx * q[y1 * s_h + x1 * s_w]);
      if (dst) dst[i * C + c] = v;
      lo = fminf(lo, v);
    }
  }
  if (minval) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64));
    if ((threadIdx.x & 63) == 0) atomic_min_f32(minval, lo);
  }
}
// (x + 1) / 2 on the interior columns when the minimum over the whole data set was negative (metrics.py:794-798)
__global__ void denorm_if_negative_kernel(float* __restrict__ x, long rows, int Wo, int pad_l, int Wp, int C, const float* __restrict__ minval) {
  if (!(*minval < 0.f)) return;
  const long total = rows * Wo * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C); long t = i / C;
    const int ox = (int)(t % Wo); const long r = t / Wo;
    float* p = x + (r * Wp + pad_l + ox) * C + c;
    *p = (*p + 1.0f) / 2.0f;
  }
}

// ---------------------------------------------------------------------------------------------- max pooling, TF "SAME"
// The reference pads with ZEROS and then pools with ceil_mode: a window position inside the zero border contributes 0, one
// beyond it (ceil_mode overhang) nothing.  e* = input extent + back padding.  One thread = one 16-byte channel chunk of an
// output position.
struct PoolSame { int N, C, Di, Hi, Wi, Do, Ho, Wo, kd, kh, kw, sd, sh, sw, pd, ph, pw, ed, eh, ew; };
template <typename T>
__global__ void pool3d_same_kernel(PoolSame g, const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy) {
  constexpr int E = ET<T>::E16;
  typedef typename ET<T>::frag frag;
  const int chunks = g.C / E;
  const long total = (long)g.N * g.Do * g.Ho * g.Wo * chunks;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % chunks); const long r = i / chunks;
    const int ow = (int)(r % g.Wo); long t = r / g.Wo;
    const int oh = (int)(t % g.Ho); t /= g.Ho;
    const int od = (int)(t % g.Do); const int n = (int)(t / g.Do);
    float best[E];
#pragma unroll
    for (int e = 0; e < E; ++e) best[e] = -INFINITY;
    for (int a = 0; a < g.kd; ++a) {
      const int d = od * g.sd - g.pd + a; if (d >= g.ed) continue;
      for (int b = 0; b < g.kh; ++b) {
        const int h = oh * g.sh - g.ph + b; if (h >= g.eh) continue;
        for (int c = 0; c < g.kw; ++c) {
          const int w = ow * g.sw - g.pw + c; if (w >= g.ew) continue;
          if ((unsigned)d < (unsigned)g.Di && (unsigned)h < (unsigned)g.Hi && (unsigned)w < (unsigned)g.Wi) {
            const long row = ((long)(n * g.Di + d) * g.Hi + h) * g.Wi + w;
            const frag v = *reinterpret_cast<const frag*>(x + row * ldx + ch * E);
#pragma unroll
            for (int e = 0; e < E; ++e) best[e] = fmaxf(best[e], (float)v[e]);
          } else {
#pragma unroll
            for (int e = 0; e < E; ++e) best[e] = fmaxf(best[e], 0.f);
          }
        }
      }
    }
    frag o;
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = ET<T>::from_f32(best[e]);
    *reinterpret_cast<frag*>(y + r * ldy + ch * E) = o;
  }
}

// y[g][c] = sum_k w[k] * x[g*S + k][c]: AvgPool3d((2,7,7), 1) followed by the mean over the remaining time steps is one
// weighted mean over a clip's rows (the 1x1 logits convolution is linear and commutes with it)
template <typename T>
__global__ void pool_rows_weighted_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, long G, int S, int C, const float* __restrict__ w) {
  const long total = G * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C); const long gi = i / C;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += w[k] * ET<T>::to_f32(x[(gi * S + k) * ldx + c]);
    y[gi * ldy + c] = ET<T>::from_f32(s);
  }
}

// ---------------------------------------------------------------------------------------------- activation moments (float64)
// rows without a single non-NaN entry are dropped (metrics.py:765-767); mean, then the unbiased covariance as np.cov
__global__ void moments_valid_kernel(const float* __restrict__ a, int n, int D, int* __restrict__ valid, int* __restrict__ count) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int any = 0;
  for (int c = 0; c < D; ++c) any |= !(a[(long)r * D + c] != a[(long)r * D + c]);
  valid[r] = any;
  if (any) atomicAdd(count, 1);
}
__global__ void moments_mean_kernel(const float* __restrict__ a, int n, int D, const int* __restrict__ valid, const int* __restrict__ count, double* __restrict__ mu) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int r = 0; r < n; ++r) if (valid[r]) s += (double)a[(long)r * D + c];
  mu[c] = s / (double)(*count);
}
__global__ void moments_cov_kernel(const float* __restrict__ a, int n, int D, const int* __restrict__ valid, const int* __restrict__ count,
                                   const double* __restrict__ mu, double* __restrict__ sigma) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= D) return;
  const double mi = mu[i], mj = mu[j];
  double s = 0.0;
  for (int r = 0; r < n; ++r) if (valid[r]) s += ((double)a[(long)r * D + i] - mi) * ((double)a[(long)r * D + j] - mj);
  // np.cov clamps the degrees of freedom at 0: one valid row AND none give 0 / 0 = NaN (0 / -1 would be -0.0)
  const int dof = *count - 1;
  sigma[(long)i * D + j] = s / (double)(dof > 0 ? dof : 0);
}
// ------------------------------------------------------------------------------------------------ image metrics
// pytorch_lightning.metrics.functional.psnr / ssim as the reference's validation logging calls them (second_stage_video.py:511-512,
// metrics.py:450-481: defaults -- 11 x 11 Gaussian window of sigma 1.5, k1 = 0.01, k2 = 0.03, data ranges taken from the tensors).
// mm[0..3] = {-min(a), max(a), -min(b), max(b)} (one atomic flavour); sums in double.
// Chosen by the SIGN BIT, not by `v >= 0`: -0.0f (the negated minimum of an image whose darkest pixel is exactly 0) compares >= 0 but its
// bit pattern is INT_MIN, which as a signed integer never beats the 0xffffffff initial value.
__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
  if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}
__global__ void pair_stats_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, float* __restrict__ mm, double* __restrict__ sse) {
  float amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float x = a[i], y = b[i], d = x - y;
    amin = fminf(amin, x); amax = fmaxf(amax, x); bmin = fminf(bmin, y); bmax = fmaxf(bmax, y);
    acc += (double)d * (double)d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    amin = fminf(amin, __shfl_xor(amin, o, 64)); amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    bmin = fminf(bmin, __shfl_xor(bmin, o, 64)); bmax = fmaxf(bmax, __shfl_xor(bmax, o, 64));
    acc += __shfl_xor(acc, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomic_max_f32(mm + 0, -amin); atomic_max_f32(mm + 1, amax); atomic_max_f32(mm + 2, -bmin); atomic_max_f32(mm + 3, bmax);
    atomicAdd(sse, acc);
  }
}
__global__ void psnr_final_kernel(const float* __restrict__ mm, const double* __restrict__ sse, long n, float* __restrict__ out) {
  // psnr = 10 log10(range^2 / mse), range = max(target) - min(target)   (functional/psnr.py: data_range=None, base 10)
  const double range = (double)mm[3] + (double)mm[2];
  const double mse = sse[0] / (double)n;
  out[0] = (float)(10.0 * (2.0 * log(range) - log(mse)) / log(10.0));
}
// SSIM map of one plane tile: 32 x 32 output positions whose 11 x 11 windows lie inside the image (the reference pads by reflection and
// crops the padded border away again, functional/ssim.py), separable Gaussian of the five moments, per-block partial sum in double.
// The tile body is shared by ssim_kernel (one data range for the whole call) and sample_ssim_kernel (one per example): thread 0 returns
// the sum of the tile's SSIM values, every other thread an unspecified value.  256 threads.
__device__ __forceinline__ double ssim_tile_sum(const float* __restrict__ pa, const float* __restrict__ pb, int H, int W, int y0, int x0, float range) {
  constexpr int TS = 32, K = 11, IN = TS + K - 1;           // 42 x 42 inputs per tile
  __shared__ float sa[IN][IN + 1], sb[IN][IN + 1];
  __shared__ float hz[5][IN][TS + 1];                       // horizontally filtered moments
  __shared__ float gw[K];
  __shared__ double red[4];
  const int Ho = H - (K - 1), Wo = W - (K - 1);
  if (threadIdx.x < K) {
    float sum = 0.f, mine = 0.f;
    for (int i = 0; i < K; ++i) {
      const float d = (float)(i - K / 2) / 1.5f, gi = expf(-d * d / 2.f);
      sum += gi;
      if (i == (int)threadIdx.x) mine = gi;
    }
    gw[threadIdx.x] = mine / sum;
  }
  for (int i = threadIdx.x; i < IN * IN; i += 256) {
    const int r = i / IN, c = i - r * IN, y = y0 + r, x = x0 + c;
    const bool in = y < H && x < W;
    sa[r][c] = in ? pa[(long)y * W + x] : 0.f;
    sb[r][c] = in ? pb[(long)y * W + x] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < IN * TS; i += 256) {
    const int r = i / TS, c = i - r * TS;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float w = gw[k], x = sa[r][c + k], y = sb[r][c + k];
      m0 += w * x; m1 += w * y; m2 += w * x * x; m3 += w * y * y; m4 += w * x * y;
    }
    hz[0][r][c] = m0; hz[1][r][c] = m1; hz[2][r][c] = m2; hz[3][r][c] = m3; hz[4][r][c] = m4;
  }
  __syncthreads();
  const float c1 = (0.01f * range) * (0.01f * range), c2 = (0.03f * range) * (0.03f * range);
  double acc = 0.0;
  for (int i = threadIdx.x; i < TS * TS; i += 256) {
    const int r = i / TS, c = i - r * TS;
    if (y0 + r >= Ho || x0 + c >= Wo) continue;
    float mu_a = 0.f, mu_b = 0.f, e_aa = 0.f, e_bb = 0.f, e_ab = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float w = gw[k];
      mu_a += w * hz[0][r + k][c]; mu_b += w * hz[1][r + k][c]; e_aa += w * hz[2][r + k][c]; e_bb += w * hz[3][r + k][c]; e_ab += w * hz[4][r + k][c];
    }
    const float maa = mu_a * mu_a, mbb = mu_b * mu_b, mab = mu_a * mu_b;
    const float upper = 2.f * (e_ab - mab) + c2, lower = (e_aa - maa) + (e_bb - mbb) + c2;
    acc += (double)(((2.f * mab + c1) * upper) / ((maa + mbb + c1) * lower));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, const float* __restrict__ mm,
                                                   double* __restrict__ part) {
  const int tiles_x = (W - 10 + 31) / 32;
  const int plane = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const float range = fmaxf(mm[1] + mm[0], mm[3] + mm[2]);   // max(preds.max() - preds.min(), target.max() - target.min())
  const double sum = ssim_tile_sum(a + (long)plane * H * W, b + (long)plane * H * W, H, W, ty * 32, tx * 32, range);
  if (threadIdx.x == 0) part[(long)plane * gridDim.x + blockIdx.x] = sum;
}
__global__ void ssim_final_kernel(const double* __restrict__ part, long nparts, double count, float* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (long i = threadIdx.x; i < nparts; i += 256) acc += part[i];      // fixed order: reproducible
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) out[0] = (float)(red[0] / count);
}

// ---------------------------------------------------------------------------------------------- test loop: sample metrics
// Reductions of the test loop (reference second_stage_video.py:665-752, 1037-1155, utils/metrics.py:60-124, 149-217).  Every sum below is
// taken in a fixed order (per-block partials in caller-owned workspace, then one ordered pass over them); minima / maxima go through the
// integer atomics above, whose result does not depend on arrival order.  No float atomic adds: results are bit-reproducible.

// pair index p of the upper triangle (row-major: (0,1), (0,2), ..., (ns-2,ns-1)) -> (j, k), j < k
__device__ __forceinline__ void pair_decode(int p, int ns, int& j, int& k) {
  j = 0;
  while (p >= ns - 1 - j) { p -= ns - 1 - j; ++j; }
  k = j + 1 + p;
}

// mm[e][0..3] = {-min, max} of the ns * s predicted frames of example e and of its s target frames (SampleMetric.update calls the measure
// per example on [ns * s, C, H, W], metrics.py:182-188, so ssim's data range is per example)
__global__ void sample_range_kernel(const float* __restrict__ pred, long n_pred, const float* __restrict__ target, long n_tgt, float* __restrict__ mm) {
  const int e = blockIdx.y;
  const float* a = pred + (long)e * n_pred;
  const float* b = target + (long)e * n_tgt;
  float amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pred; i += (long)gridDim.x * blockDim.x) {
    const float x = a[i];
    amin = fminf(amin, x); amax = fmaxf(amax, x);
  }
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_tgt; i += (long)gridDim.x * blockDim.x) {
    const float y = b[i];
    bmin = fminf(bmin, y); bmax = fmaxf(bmax, y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    amin = fminf(amin, __shfl_xor(amin, o, 64)); amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    bmin = fminf(bmin, __shfl_xor(bmin, o, 64)); bmax = fmaxf(bmax, __shfl_xor(bmax, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    float* m = mm + 4 * e;
    if (amin <= amax) { atomic_max_f32(m + 0, -amin); atomic_max_f32(m + 1, amax); }      // (a block beyond the data saw nothing)
    if (bmin <= bmax) { atomic_max_f32(m + 2, -bmin); atomic_max_f32(m + 3, bmax); }
  }
}
// grid (tiles, ns * s * C, bs): plane q = (j * s + f) * C + c of example e against plane f * C + c of the example's target -- the target is
// read in place for every sample, never replicated
__global__ __launch_bounds__(256) void sample_ssim_kernel(const float* __restrict__ pred, const float* __restrict__ target, int ns, int sC, int H, int W,
                                                          const float* __restrict__ mm, double* __restrict__ part) {
  const int tiles_x = (W - 10 + 31) / 32;
  const int e = blockIdx.z, q = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int rem = q % sC;
  const long hw = (long)H * W;
  const float* m = mm + 4 * e;
  const float range = fmaxf(m[1] + m[0], m[3] + m[2]);
  const double sum = ssim_tile_sum(pred + ((long)e * ns * sC + q) * hw, target + ((long)e * sC + rem) * hw, H, W, ty * 32, tx * 32, range);
  if (threadIdx.x == 0) part[((long)e * ns * sC + q) * gridDim.x + blockIdx.x] = sum;
}
// one block per frame: the C * tiles partials of a frame are adjacent
__global__ void sample_ssim_final_kernel(const double* __restrict__ part, int per_frame, double count, float* __restrict__ out) {
  __shared__ double red[64];
  const double* p = part + (long)blockIdx.x * per_frame;
  double acc = 0.0;
  for (int i = threadIdx.x; i < per_frame; i += 64) acc += p[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(red[0] / count);
}

// metrics.py:193-204: one block (one wave) per example over vals[ns][s].  The sample with the smallest mean over the frames is chosen
// (argmin for SSIM too, as the reference; the first index wins a tie, as torch.argmin), then per frame: that sample's value, the unbiased
// standard deviation over the samples (ns == 1: NaN, as torch.std) and the mean over the samples.  Sums in double, serial: fixed order.
// The per-sample means are formed AND COMPARED in double, the reference's torch.argmin sees fp32 means: two samples whose means differ by
// less than an fp32 rounding (an exact fp32 tie that is none in double, or the reverse) may give the other of the two indices.
__global__ __launch_bounds__(64) void sample_stats_kernel(const float* __restrict__ vals, int ns, int s, float* __restrict__ nn, float* __restrict__ sd,
                                                          float* __restrict__ mean, int* __restrict__ index) {
  extern __shared__ double smean[];
  __shared__ int best;
  const float* v = vals + (long)blockIdx.x * ns * s;
  for (int j = threadIdx.x; j < ns; j += 64) {
    double acc = 0.0;
    for (int f = 0; f < s; ++f) acc += (double)v[j * s + f];
    smean[j] = acc / (double)s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = 0;
    for (int j = 1; j < ns; ++j) if (smean[j] < smean[b]) b = j;
    best = b;
    index[blockIdx.x] = b;
  }
  __syncthreads();
  for (int f = threadIdx.x; f < s; f += 64) {
    double acc = 0.0;
    for (int j = 0; j < ns; ++j) acc += (double)v[j * s + f];
    const double mu = acc / (double)ns;
    double sq = 0.0;
    for (int j = 0; j < ns; ++j) { const double d = (double)v[j * s + f] - mu; sq += d * d; }
    const long o = (long)blockIdx.x * s + f;
    nn[o] = v[best * s + f];
    sd[o] = (float)sqrt(sq / (double)(ns - 1));
    mean[o] = (float)mu;
  }
}

// metrics.py:104-124: D[e][j][k] = mean((v_j - v_k)^2) for all pairs of the ns samples of an example.  A block stages 64 elements of all
// ns videos in LDS -- every element is read from memory once per example -- and each thread keeps the running sums of its (up to 8) pairs
// in double registers across the tiles it visits; per-block partials, then one ordered pass.
constexpr int PM_TILE = 64, PM_MAXNS = 64, PM_PP = 8;         // 64 * 63 / 2 = 2016 pairs <= 8 * 256
__global__ __launch_bounds__(256) void pair_mse_kernel(const float* __restrict__ x, int ns, long L, double* __restrict__ part) {
  __shared__ float tile[PM_MAXNS][PM_TILE + 1];
  const int P = ns * (ns - 1) / 2;
  const float* xe = x + (long)blockIdx.y * ns * L;
  int pj[PM_PP], pk[PM_PP];
  double acc[PM_PP];
#pragma unroll
  for (int i = 0; i < PM_PP; ++i) {
    const int p = threadIdx.x + 256 * i;
    pj[i] = 0; pk[i] = 0; acc[i] = 0.0;
    if (p < P) pair_decode(p, ns, pj[i], pk[i]);
  }
  const long ntiles = (L + PM_TILE - 1) / PM_TILE;
  const int col = threadIdx.x & 63;
  for (long ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const long idx = ti * PM_TILE + col;
    for (int r = threadIdx.x >> 6; r < ns; r += 4) tile[r][col] = idx < L ? xe[(long)r * L + idx] : 0.f;     // a zero tail adds 0 to every pair
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PM_PP; ++i) {
      if ((int)threadIdx.x + 256 * i < P) {
        const float* a = tile[pj[i]];
        const float* b = tile[pk[i]];
        double t = acc[i];
#pragma unroll 8
        for (int c = 0; c < PM_TILE; ++c) { const double d = (double)a[c] - (double)b[c]; t = fma(d, d, t); }
        acc[i] = t;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PM_PP; ++i) {
    const int p = threadIdx.x + 256 * i;
    if (p < P) part[((long)blockIdx.y * gridDim.x + blockIdx.x) * P + p] = acc[i];
  }
}
// D[g] = (sum over the nblk partials of group g) / count, written to both triangles; the diagonal is 0.  One block per group (example / map).
__global__ void pair_final_kernel(const double* __restrict__ part, int nblk, int ns, double count, float* __restrict__ D) {
  const int P = ns * (ns - 1) / 2;
  const double* pg = part + (long)blockIdx.x * nblk * P;
  float* Dg = D + (long)blockIdx.x * ns * ns;
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) acc += pg[(long)b * P + p];
    int j, k;
    pair_decode(p, ns, j, k);
    const float v = (float)(acc / count);
    Dg[j * ns + k] = v; Dg[k * ns + j] = v;
  }
  for (int j = threadIdx.x; j < ns; j += blockDim.x) Dg[j * ns + j] = 0.f;
}

// metrics.py:60-62, 88-94 on one feature map of the ns * s frames of an example, channels-last rows x[(frame * HW + pos) * ld + c]:
// per location (pos, c) the s values of sample j form a vector over TIME; normalize_activation divides it by (its L2 norm + 1e-10), and
// CosineSimilarity(dim=0, eps=1e-8) (ATen: each operand divided by max(its norm, eps), then the dot product) contracts time again.  A
// location that is zero in every frame gives 0 / 1e-10 = 0 and contributes 0.  Output: the mean over locations of the ns x ns cosines.
// u[t] <- x[t] / (|x| + 1e-10), then u[t] / max(|u|, 1e-8): the reference's two divisions, in its order
template <int S_MAX>
__device__ __forceinline__ void time_normalize(float (&a)[S_MAX]) {
  float n2 = 0.f;
#pragma unroll
  for (int t = 0; t < S_MAX; ++t) n2 += a[t] * a[t];
  const float d1 = sqrtf(n2) + 1e-10f;
  float m2 = 0.f;
#pragma unroll
  for (int t = 0; t < S_MAX; ++t) { a[t] = a[t] / d1; m2 += a[t] * a[t]; }
  const float d2 = fmaxf(sqrtf(m2), 1e-8f);
#pragma unroll
  for (int t = 0; t < S_MAX; ++t) a[t] = a[t] / d2;
}
// Small ns: one thread per location, the NS x s values in registers (lanes run along the channels: coalesced rows), the pair sums of
// the locations a thread visits in double registers, one block reduction at the end.  s <= 16.
template <typename T, int NS>
__global__ __launch_bounds__(256) void time_cos_reg_kernel(const T* __restrict__ x, int ld, int C, long HW, int s, double* __restrict__ part) {
  constexpr int P = NS * (NS - 1) / 2, S_MAX = 16;
  __shared__ double red[4][P];
  double acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = 0.0;
  const long total = HW * C;
  for (long l = (long)blockIdx.x * 256 + threadIdx.x; l < total; l += (long)gridDim.x * 256) {
    const long pos = l / C; const int c = (int)(l - pos * C);
    float a[NS][S_MAX];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
#pragma unroll
      for (int t = 0; t < S_MAX; ++t) a[j][t] = t < s ? ET<T>::to_f32(x[((long)(j * s + t) * HW + pos) * ld + c]) : 0.f;
      time_normalize<S_MAX>(a[j]);
    }
    int p = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int k = j + 1; k < NS; ++k, ++p) {
        float dot = 0.f;
#pragma unroll
        for (int t = 0; t < S_MAX; ++t) dot += a[j][t] * a[k][t];
        acc[p] += (double)dot;
      }
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    double v = acc[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][p] = v;
  }
  __syncthreads();
  if (threadIdx.x < P) part[(long)blockIdx.x * P + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
// Larger ns (up to 64): a block stages LOC consecutive locations of all ns * s frames in LDS as u[j][t * LOC + lo] (row pitch s * LOC + 1:
// the threads of a wave read different samples j at one offset, the odd pitch spreads them over the banks), normalizes them in place, and
// each thread adds the products of its (up to 8) pairs over the tile to double registers.
template <typename T>
__global__ __launch_bounds__(256) void time_cos_lds_kernel(const T* __restrict__ x, int ld, int C, long HW, int ns, int s, int LOC, double* __restrict__ part) {
  extern __shared__ float u[];
  const int P = ns * (ns - 1) / 2, row = s * LOC, pitch = row + 1;
  int pj[PM_PP], pk[PM_PP];
  double acc[PM_PP];
#pragma unroll
  for (int i = 0; i < PM_PP; ++i) {
    const int p = threadIdx.x + 256 * i;
    pj[i] = 0; pk[i] = 0; acc[i] = 0.0;
    if (p < P) pair_decode(p, ns, pj[i], pk[i]);
  }
  const long total = HW * C, nchunks = (total + LOC - 1) / LOC;
  for (long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    for (int i = threadIdx.x; i < ns * row; i += 256) {
      const int fr = i / LOC, lo = i - fr * LOC;                   // fr = j * s + t
      const long l = ch * LOC + lo;
      float v = 0.f;                                               // locations beyond the map: zero vectors, contribute 0
      if (l < total) { const long pos = l / C; v = ET<T>::to_f32(x[((long)fr * HW + pos) * ld + (l - pos * C)]); }
      const int j = fr / s, t = fr - j * s;
      u[j * pitch + t * LOC + lo] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ns * LOC; i += 256) {
      const int j = i / LOC, lo = i - j * LOC;
      float* q = u + j * pitch + lo;
      float n2 = 0.f;
      for (int t = 0; t < s; ++t) n2 += q[t * LOC] * q[t * LOC];
      const float d1 = sqrtf(n2) + 1e-10f;
      float m2 = 0.f;
      for (int t = 0; t < s; ++t) { const float w = q[t * LOC] / d1; q[t * LOC] = w; m2 += w * w; }
      const float d2 = fmaxf(sqrtf(m2), 1e-8f);
      for (int t = 0; t < s; ++t) q[t * LOC] = q[t * LOC] / d2;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PM_PP; ++i) {
      if ((int)threadIdx.x + 256 * i < P) {
        const float* a = u + pj[i] * pitch;
        const float* b = u + pk[i] * pitch;
        double t = acc[i];
#pragma unroll 4
        for (int c = 0; c < row; ++c) t += (double)(a[c] * b[c]);
        acc[i] = t;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PM_PP; ++i) {
    const int p = threadIdx.x + 256 * i;
    if (p < P) part[(long)blockIdx.x * P + p] = acc[i];
  }
}

// second_stage_video.py:673-675: ((x + 1) * 127.5) truncated to uint8, [B, T, 3, H, W] -> [B, T, H, W, 3].  The add and the multiply are two
// rounded fp32 operations (never one fma), as numpy / torch evaluate them; for x in [-1, 1] the product lies in [0, 255] and the
// truncation equals numpy's astype(np.uint8).  Outside that range numpy's cast is undefined behaviour: here the value is clamped to
// [0, 255] (NaN -> 0).  One thread = four pixels of a frame (12 output bytes, three aligned words) when hw % 4 == 0, else one pixel.
__device__ __forceinline__ unsigned u8_of(float x) {
  const float v = __fmul_rn(__fadd_rn(x, 1.0f), 127.5f);
  return (unsigned)fminf(fmaxf(v, 0.f), 255.f);                 // fmaxf(NaN, 0) = 0
}
__global__ void video_to_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ y, long frames, long hw, int vec) {
  if (vec) {
    const long q4 = hw / 4, total = frames * q4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long fr = i / q4, px = (i - fr * q4) * 4;
      const float* p = x + fr * 3 * hw + px;
      const f32x4 r = *reinterpret_cast<const f32x4*>(p), g = *reinterpret_cast<const f32x4*>(p + hw), b = *reinterpret_cast<const f32x4*>(p + 2 * hw);
      unsigned o[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) { o[3 * k] = u8_of(r[k]); o[3 * k + 1] = u8_of(g[k]); o[3 * k + 2] = u8_of(b[k]); }
      unsigned* w = reinterpret_cast<unsigned*>(y + (fr * hw + px) * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = o[4 * k] | (o[4 * k + 1] << 8) | (o[4 * k + 2] << 16) | (o[4 * k + 3] << 24);
    }
  } else {
    const long total = frames * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long fr = i / hw, px = i - fr * hw;
      const float* p = x + fr * 3 * hw + px;
      unsigned char* w = y + i * 3;
      w[0] = (unsigned char)u8_of(p[0]); w[1] = (unsigned char)u8_of(p[hw]); w[2] = (unsigned char)u8_of(p[2 * hw]);
    }
  }
}
// metrics.py:64-72 normalize_input_vgg: ((x + 1) / 2 - mean[c]) / std[c] on [N, 3, H, W] (ImageNet statistics), one element-wise pass
__global__ void vgg_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, long n, long hw) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)((i / hw) % 3);
    const float m = c == 0 ? mean[0] : c == 1 ? mean[1] : mean[2], d = c == 0 ? sd[0] : c == 1 ? sd[1] : sd[2];
    y[i] = __fsub_rn(__fadd_rn(x[i], 1.0f) / 2.0f, m) / d;
  }
}



// ==============================================================================================
extern "C" int ipoke_video_to_cl(const float* src, int64_t s_n, int64_t s_f, int64_t s_c, int64_t s_h, int64_t s_w, int N, int T, int C, int Hi,
                                 int Wi, float* dst, int Ho, int Wo, int pad_l, int pad_r, float* minval, void* stream) {
  IPK_REQUIRE(src && (dst || minval) && N >= 1 && T >= 1 && C >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1 && pad_l >= 0 && pad_r >= 0, "bad arguments");
  const long frames = (long)N * T;
  const int Wp = pad_l + Wo + pad_r;
  hipLaunchKernelGGL(video_to_cl_kernel, dim3(grid1(frames * Ho * Wp)), dim3(256), 0, STREAM(stream), src, (long)s_n, (long)s_f, (long)s_c, (long)s_h,
                     (long)s_w, T, C, Hi, Wi, dst, frames, Ho, Wo, pad_l, Wp, minval);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
/* *minval = a huge float: the start value of the running minimum of ipoke_video_to_cl */
extern "C" int ipoke_min_reset(float* minval, void* stream) {
  IPK_REQUIRE(minval, "null argument");
  IPK_HIP(hipMemsetAsync(minval, 0x7f, sizeof(float), STREAM(stream)));
  return IPOKE_OK;
}
extern "C" int ipoke_denorm_if_negative(float* x, int64_t rows, int Wo, int pad_l, int pad_r, int C, const float* minval, void* stream) {
  IPK_REQUIRE(x && minval && rows >= 1 && Wo >= 1 && C >= 1, "bad arguments");
  hipLaunchKernelGGL(denorm_if_negative_kernel, dim3(grid1(rows * Wo * C)), dim3(256), 0, STREAM(stream), x, (long)rows, Wo, pad_l, pad_l + Wo + pad_r, C, minval);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_pool3d_same(const int* dims, const void* x, int ldx, void* y, int ldy, int dtype, void* stream) {
  IPK_REQUIRE(dims && x && y, "null argument");
  PoolSame g;
  std::memcpy(&g, dims, sizeof(g));
  const int e16 = dtype == IPOKE_BF16 ? 8 : 4;
  IPK_REQUIRE(dtype == IPOKE_BF16 || dtype == IPOKE_F32, "bad dtype");
  IPK_REQUIRE(g.N >= 1 && g.C >= 1 && g.Do >= 1 && g.Ho >= 1 && g.Wo >= 1 && g.kd >= 1 && g.kh >= 1 && g.kw >= 1, "bad pool geometry");
  IPK_REQUIRE(g.C % e16 == 0 && ldx % e16 == 0 && ldy % e16 == 0 && ldx >= g.C && ldy >= g.C, "channels and pitches: multiples of 16 bytes");
  IPK_REQUIRE(g.ed >= g.Di && g.eh >= g.Hi && g.ew >= g.Wi && g.pd >= 0 && g.ph >= 0 && g.pw >= 0, "padded extents must cover the input");
  // every window must see at least its first position inside the padded extent (ceil_mode never starts a window in the overhang)
  IPK_REQUIRE((g.Do - 1) * g.sd - g.pd < g.ed && (g.Ho - 1) * g.sh - g.ph < g.eh && (g.Wo - 1) * g.sw - g.pw < g.ew, "window starts beyond the padded extent");
  const long total = (long)g.N * g.Do * g.Ho * g.Wo * (g.C / e16);
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(pool3d_same_kernel<bf16_t>, dim3(grid1(total, 8192)), dim3(256), 0, STREAM(stream), g, (const bf16_t*)x, ldx, (bf16_t*)y, ldy);
  else
    hipLaunchKernelGGL(pool3d_same_kernel<float>, dim3(grid1(total, 8192)), dim3(256), 0, STREAM(stream), g, (const float*)x, ldx, (float*)y, ldy);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_pool_rows_weighted(const void* x, int ldx, void* y, int ldy, int64_t G, int S, int C, const float* w, int dtype, void* stream) {
  IPK_REQUIRE(x && y && w && G >= 1 && S >= 1 && C >= 1 && ldx >= C && ldy >= C, "bad arguments");
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(pool_rows_weighted_kernel<bf16_t>, dim3(grid1(G * C)), dim3(256), 0, STREAM(stream), (const bf16_t*)x, ldx, (bf16_t*)y, ldy, (long)G, S, C, w);
  else
    hipLaunchKernelGGL(pool_rows_weighted_kernel<float>, dim3(grid1(G * C)), dim3(256), 0, STREAM(stream), (const float*)x, ldx, (float*)y, ldy, (long)G, S, C, w);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

/* workspace: (n + 1) int32 */
extern "C" int ipoke_activation_moments(const float* act, int n, int D, double* mu, double* sigma, int* workspace, void* stream) {
  IPK_REQUIRE(act && mu && sigma && workspace && n >= 2 && D >= 1, "bad arguments");
  int* count = workspace; int* valid = workspace + 1;
  IPK_HIP(hipMemsetAsync(count, 0, sizeof(int), STREAM(stream)));
  hipLaunchKernelGGL(moments_valid_kernel, dim3((n + 255) / 256), dim3(256), 0, STREAM(stream), act, n, D, valid, count);
  hipLaunchKernelGGL(moments_mean_kernel, dim3((D + 63) / 64), dim3(64), 0, STREAM(stream), act, n, D, valid, count, mu);
  hipLaunchKernelGGL(moments_cov_kernel, dim3((D + 63) / 64, D), dim3(64), 0, STREAM(stream), act, n, D, valid, count, mu, sigma);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

/* Workspace of ipoke_psnr_ssim in bytes (planes of H x W fp32 pixels). */
extern "C" int64_t ipoke_image_metrics_workspace_bytes(int64_t planes, int H, int W) {
  const int64_t Ho = H > 10 ? H - 10 : 0, Wo = W > 10 ? W - 10 : 0;
  return 64 + 8 * (planes * ((Ho + 31) / 32) * ((Wo + 31) / 32) + 1);
}
/* out[0] = psnr(preds, target), out[1] = ssim(preds, target) of `planes` fp32 image planes [planes][H][W] (the N * C planes of NCHW
 * tensors): pytorch_lightning.metrics.functional.psnr / ssim with their defaults, as SSIM_custom / PSNR_custom call them
 * (metrics.py:450-481). */
extern "C" int ipoke_psnr_ssim(const float* preds, const float* target, int64_t planes, int H, int W, void* workspace, float* out, void* stream) {
  IPK_REQUIRE(preds && target && workspace && out && planes >= 1 && H >= 11 && W >= 11, "bad arguments (images must be at least 11 x 11)");
  hipStream_t s = STREAM(stream);
  float* mm = reinterpret_cast<float*>(workspace);
  double* sse = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(workspace) + 32);
  double* part = sse + 4;
  const long n = (long)planes * H * W;
  IPK_HIP(hipMemsetAsync(mm, 0xff, 4 * sizeof(float), s));       // 0xffffffff: below every float in the order of atomic_max_f32
  IPK_HIP(hipMemsetAsync(sse, 0, sizeof(double), s));
  hipLaunchKernelGGL(pair_stats_kernel, dim3(grid1(n, 2048)), dim3(256), 0, s, preds, target, n, mm, sse);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(psnr_final_kernel, dim3(1), dim3(1), 0, s, mm, sse, n, out);
  IPK_LAUNCH_CHECK();
  const int Ho = H - 10, Wo = W - 10, tiles = ((Ho + 31) / 32) * ((Wo + 31) / 32);
  hipLaunchKernelGGL(ssim_kernel, dim3(tiles, (unsigned)planes), dim3(256), 0, s, preds, target, H, W, mm, part);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), 0, s, part, (long)planes * tiles, (double)planes * Ho * Wo, out + 1);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

/* ---- test loop reductions (declared in include/ipoke_hip.h) ---- */
static long sample_ssim_tiles(int H, int W) { return (long)((H - 10 + 31) / 32) * ((W - 10 + 31) / 32); }
extern "C" int64_t ipoke_sample_ssim_workspace_bytes(int bs, int ns, int s, int C, int H, int W) {
  if (bs < 1 || ns < 1 || s < 1 || C < 1 || H < 11 || W < 11) return 0;
  return (((int64_t)bs * 16 + 63) / 64) * 64 + 8 * (int64_t)bs * ns * s * C * sample_ssim_tiles(H, W);
}
extern "C" int ipoke_sample_ssim(const float* pred, const float* target, int bs, int ns, int s, int C, int H, int W, void* workspace, float* out,
                                 void* stream) {
  IPK_REQUIRE(pred && target && workspace && out && bs >= 1 && ns >= 1 && s >= 1 && C >= 1 && H >= 11 && W >= 11,
              "bad arguments (images must be at least 11 x 11)");
  IPK_REQUIRE((long)ns * s * C <= 65535 && bs <= 65535, "ns * s * C and bs must fit a grid dimension");
  hipStream_t st = STREAM(stream);
  float* mm = reinterpret_cast<float*>(workspace);
  double* part = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(workspace) + (((int64_t)bs * 16 + 63) / 64) * 64);
  const long hw = (long)H * W, n_tgt = (long)s * C * hw, n_pred = n_tgt * ns;
  const int tiles = (int)sample_ssim_tiles(H, W), Ho = H - 10, Wo = W - 10;
  IPK_HIP(hipMemsetAsync(mm, 0xff, (size_t)bs * 4 * sizeof(float), st));       // below every float in the order of atomic_max_f32
  hipLaunchKernelGGL(sample_range_kernel, dim3(grid1(n_pred, 256), bs), dim3(256), 0, st, pred, n_pred, target, n_tgt, mm);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(sample_ssim_kernel, dim3(tiles, ns * s * C, bs), dim3(256), 0, st, pred, target, ns, s * C, H, W, mm, part);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(sample_ssim_final_kernel, dim3(bs * ns * s), dim3(64), 0, st, part, C * tiles, (double)C * Ho * Wo, out);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_sample_stats(const float* vals, int bs, int ns, int s, float* nn, float* sd, float* mean, int* index, void* stream) {
  IPK_REQUIRE(vals && nn && sd && mean && index && bs >= 1 && ns >= 1 && s >= 1 && ns <= 4096, "bad arguments");
  hipLaunchKernelGGL(sample_stats_kernel, dim3(bs), dim3(64), (size_t)ns * sizeof(double), STREAM(stream), vals, ns, s, nn, sd, mean, index);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
// utils/metrics.py:294, :299 (KPSMetric.update): out[e][j][f] = mean over the K * 2 coordinates of (pred - target)^2, one thread per frame, the
// terms added in index order in fp32 (each product and each sum rounded on its own); the target is read in place for every sample
__global__ void kps_frame_mse_kernel(const float* __restrict__ pred, const float* __restrict__ target, long total, int ns, int s, int K2,
                                     float* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long f = i % s, e = i / ((long)ns * s);
    const float* p = pred + i * K2;
    const float* t = target + (e * s + f) * K2;
    float acc = 0.f;
    for (int k = 0; k < K2; ++k) {
      const float d = __fsub_rn(p[k], t[k]);
      acc = __fadd_rn(acc, __fmul_rn(d, d));
    }
    out[i] = __fdiv_rn(acc, (float)K2);
  }
}
extern "C" int ipoke_kps_frame_mse(const float* pred, const float* target, int bs, int ns, int s, int K, float* out, void* stream) {
  IPK_REQUIRE(pred && target && out && bs >= 1 && ns >= 1 && s >= 1 && K >= 1, "bad arguments");
  const long total = (long)bs * ns * s;
  hipLaunchKernelGGL(kps_frame_mse_kernel, dim3(grid1(total, 2048)), dim3(256), 0, STREAM(stream), pred, target, total, ns, s, 2 * K, out);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
static int pair_mse_blocks(int n_ex, int64_t L) {
  const int64_t tiles = (L + PM_TILE - 1) / PM_TILE;
  int64_t b = 2048 / (n_ex > 0 ? n_ex : 1);
  if (b < 1) b = 1;
  return (int)(tiles < b ? tiles : b);
}
extern "C" int64_t ipoke_pair_mse_workspace_bytes(int n_ex, int ns, int64_t L) {
  if (n_ex < 1 || ns < 2 || L < 1) return 0;
  return 8 * (int64_t)n_ex * pair_mse_blocks(n_ex, L) * (ns * (ns - 1) / 2);
}
extern "C" int ipoke_pair_mse(const float* x, int n_ex, int ns, int64_t L, void* workspace, float* D, void* stream) {
  IPK_REQUIRE(x && workspace && D && n_ex >= 1 && n_ex <= 65535 && L >= 1, "bad arguments");
  IPK_REQUIRE(ns >= 2 && ns <= PM_MAXNS, "2 <= ns <= 64 samples per example");
  const int nblk = pair_mse_blocks(n_ex, L);
  double* part = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(pair_mse_kernel, dim3(nblk, n_ex), dim3(256), 0, STREAM(stream), x, ns, (long)L, part);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_final_kernel, dim3(n_ex), dim3(256), 0, STREAM(stream), part, nblk, ns, (double)L, D);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
constexpr int TC_REG_MAX_NS = 8, TC_LDS_BYTES = 64 * 1024;
static int time_cos_loc(int ns, int s) {       // locations per LDS tile: the largest of 64, 32, ..., 4 whose tile fits 64 KiB; 0: none does
  for (int loc = 64; loc >= 4; loc >>= 1)
    if ((int64_t)ns * (s * loc + 1) * 4 <= TC_LDS_BYTES) return loc;
  return 0;
}
static int time_cos_blocks(int ns, int s, int64_t total) {
  // work units of a launch: 256 locations per block on the register path, one LDS tile of `loc` locations otherwise
  int64_t per_unit = 256;
  if (ns > TC_REG_MAX_NS) {
    const int loc = time_cos_loc(ns, s);
    per_unit = loc > 0 ? loc : 1;
  }
  const int64_t units = (total + per_unit - 1) / per_unit;
  return (int)(units < 1 ? 1 : units > 1024 ? 1024 : units);
}
extern "C" int64_t ipoke_time_cosine_workspace_bytes(int ns, int s, int C, int64_t HW) {
  if (ns < 2 || s < 1 || C < 1 || HW < 1) return 0;
  return 8 * (int64_t)time_cos_blocks(ns, s, HW * C) * (ns * (ns - 1) / 2);
}
template <typename T>
static int time_cos_launch(const T* x, int ld, int C, long HW, int ns, int s, double* part, int nblk, hipStream_t st) {
  switch (ns) {
#define TC_CASE(N) case N: hipLaunchKernelGGL((time_cos_reg_kernel<T, N>), dim3(nblk), dim3(256), 0, st, x, ld, C, HW, s, part); break;
    TC_CASE(2) TC_CASE(3) TC_CASE(4) TC_CASE(5) TC_CASE(6) TC_CASE(7) TC_CASE(8)
#undef TC_CASE
    default: {
      const int loc = time_cos_loc(ns, s);
      hipLaunchKernelGGL(time_cos_lds_kernel<T>, dim3(nblk), dim3(256), (size_t)ns * (s * loc + 1) * sizeof(float), st, x, ld, C, HW, ns, s, loc, part);
    }
  }
  return 0;
}
extern "C" int ipoke_time_cosine(const void* fmap, int ld, int C, int64_t HW, int ns, int s, int dtype, void* workspace, float* D, void* stream) {
  IPK_REQUIRE(fmap && workspace && D && C >= 1 && HW >= 1 && ld >= C && s >= 1, "bad arguments");
  IPK_REQUIRE(dtype == IPOKE_BF16 || dtype == IPOKE_F32, "bad dtype");
  IPK_REQUIRE(ns >= 2 && ns <= PM_MAXNS, "2 <= ns <= 64 samples per example");
  IPK_REQUIRE(ns <= TC_REG_MAX_NS ? s <= 16 : time_cos_loc(ns, s) > 0, "sequence too long (register path: s <= 16; LDS path: ns * (4 s + 1) floats <= 64 KiB)");
  const int nblk = time_cos_blocks(ns, s, HW * C);
  double* part = reinterpret_cast<double*>(workspace);
  if (dtype == IPOKE_BF16) time_cos_launch<bf16_t>((const bf16_t*)fmap, ld, C, (long)HW, ns, s, part, nblk, STREAM(stream));
  else time_cos_launch<float>((const float*)fmap, ld, C, (long)HW, ns, s, part, nblk, STREAM(stream));
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_final_kernel, dim3(1), dim3(256), 0, STREAM(stream), part, nblk, ns, (double)HW * C, D);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_video_to_u8(const float* x, uint8_t* y, int64_t frames, int H, int W, void* stream) {
  IPK_REQUIRE(x && y && frames >= 1 && H >= 1 && W >= 1, "bad arguments");
  const long hw = (long)H * W;
  const int vec = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(x) % 16) == 0 && (reinterpret_cast<uintptr_t>(y) % 4) == 0;
  hipLaunchKernelGGL(video_to_u8_kernel, dim3(grid1(vec ? frames * (hw / 4) : frames * hw, 2048)), dim3(256), 0, STREAM(stream), x, y, (long)frames, hw, vec);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_vgg_normalize(const float* x, float* y, int64_t N, int H, int W, void* stream) {
  IPK_REQUIRE(x && y && N >= 1 && H >= 1 && W >= 1, "bad arguments");
  const long hw = (long)H * W, n = (long)N * 3 * hw;
  hipLaunchKernelGGL(vgg_normalize_kernel, dim3(grid1(n, 2048)), dim3(256), 0, STREAM(stream), x, y, n, hw);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
