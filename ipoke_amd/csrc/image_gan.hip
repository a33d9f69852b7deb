// Adversarial phase of the image autoencoder (reference models/first_stage_image_conv.py:85-168 with the PatchGAN of
// models/modules/discriminators/patchgan.py:255-325): the element-wise and reduction work next to the convolutions.
//
//   ipoke_hinge_terms       hinge-real / hinge-fake / generator term of a prediction column, mean sigmoid(pred) and d loss / d pred
//   ipoke_act_jvp           ydot = act'(y) * xdot: the tangent of an activation fused into a convolution (conv 0's LeakyReLU)
//   ipoke_gp_direction      per-sample sum g^2, their mean (the penalty's value) and v = (2 / N) g, the tangent direction
//   ipoke_groupnorm_tangent GroupNorm (+ activation) tangent and its backward with every sum in a fixed order
//
// All of them are HBM-bound streaming passes over small maps.  Every sum runs in double in a fixed order through caller-owned partials:
// no float atomics, no host synchronisation, a second run gives the same bits.
#include "common.h"

namespace ipoke {

constexpr int kHingeBlocks = 256;     // partial pairs of ipoke_hinge_terms
constexpr int kGpBlocks = 16;         // partials per sample of ipoke_gp_direction

__device__ __forceinline__ double gan_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// block-wide sum of doubles in a fixed order (256 threads); `red` holds 4 doubles
__device__ __forceinline__ double gan_block_sum(double v, double* red) {
  v = gan_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------- hinge terms
// mode 0: mean relu(1 - p), mode 1: mean relu(1 + p), mode 2: -mean p.  grad = d loss / d p: -+1/M where the hinge is active, exactly 0 where
// 1 -+ p <= 0 (relu's derivative at 0 is 0), -1/M everywhere for the generator term.
__global__ __launch_bounds__(256) void hinge_terms_kernel(const float* __restrict__ pred, int ld, long M, int mode, float* __restrict__ grad,
                                                          int ldg, double* __restrict__ partials) {
  __shared__ double red[4];
  const float gm = (float)(1.0 / (double)M);
  double loss = 0.0, sig = 0.0;
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
    const double p = (double)pred[m * ld];
    float g;
    if (mode == 2) {
      loss -= p; g = -gm;
    } else {
      const double h = mode == 0 ? 1.0 - p : 1.0 + p;
      const bool on = h > 0.0;
      if (on) loss += h;
      g = on ? (mode == 0 ? -gm : gm) : 0.f;
    }
    sig += 1.0 / (1.0 + exp(-p));
    grad[m * ldg] = g;
  }
  loss = gan_block_sum(loss, red);
  sig = gan_block_sum(sig, red);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = loss; partials[2 * blockIdx.x + 1] = sig; }
}
__global__ __launch_bounds__(256) void hinge_final_kernel(const double* __restrict__ partials, int n_part, long M, float* __restrict__ out) {
  __shared__ double red[4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n_part; i += 256) { a += partials[2 * i]; b += partials[2 * i + 1]; }
  a = gan_block_sum(a, red);
  b = gan_block_sum(b, red);
  if (threadIdx.x == 0) { out[0] = (float)(a / (double)M); out[1] = (float)(b / (double)M); }
}

// ---------------------------------------------------------------------------------------------- activation tangent
// ydot[m][c] = act'(y[m][c]) * xdot[m][c] for c < C, 0 for C <= c < Cpad; the product is formed in double and rounded once.
template <typename T>
__global__ __launch_bounds__(256) void act_jvp_kernel(const T* __restrict__ y, int ldy, const T* __restrict__ xd, int ldx, T* __restrict__ out,
                                                      int ldo, long M, int C, int Cpad, int act) {
  const long total = M * Cpad;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / Cpad; const int c = (int)(i - m * Cpad);
    float r = 0.f;
    if (c < C) {
      const float yy = ET<T>::to_f32(y[m * ldy + c]);
      const double d = yy > 0.f ? 1.0 : (act == IPOKE_ACT_LRELU02 ? 0.2 : 0.0);
      r = (float)(d * (double)ET<T>::to_f32(xd[m * ldx + c]));
    }
    out[m * ldo + c] = ET<T>::from_f32(r);
  }
}

// ---------------------------------------------------------------------------------------------- penalty value and direction
// g [N][L]: block (b, n) sums its slice of sample n in double and writes v = (2 / N) g for it
__global__ __launch_bounds__(256) void gp_direction_kernel(const float* __restrict__ g, int N, long L, float* __restrict__ v,
                                                           double* __restrict__ partials) {
  __shared__ double red[4];
  const int n = blockIdx.y;
  const double k = 2.0 / (double)N;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < L; i += (long)gridDim.x * 256) {
    const double x = (double)g[(long)n * L + i];
    acc += x * x;
    v[(long)n * L + i] = (float)(k * x);
  }
  acc = gan_block_sum(acc, red);
  if (threadIdx.x == 0) partials[(long)n * gridDim.x + blockIdx.x] = acc;
}
// out[0] = mean_n sum g_n^2, out[1 + n] = sum g_n^2
__global__ __launch_bounds__(256) void gp_direction_final_kernel(const double* __restrict__ partials, int n_part, int N, float* __restrict__ out) {
  __shared__ double red[4];
  double tot = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    double s = 0.0;
    for (int b = 0; b < n_part; ++b) s += partials[(long)n * n_part + b];
    out[1 + n] = (float)s;
    tot += s;
  }
  tot = gan_block_sum(tot, red);
  if (threadIdx.x == 0) out[0] = (float)(tot / (double)N);
}

// ---------------------------------------------------------------------------------------------- GroupNorm tangent, fixed order
// The formulas of ipoke_groupnorm_jvp (vae_train.hip: ydot = act'(y) gamma r (u - <u> - xhat <xhat u>) and its backward), one
// workgroup per (sample, group).  That kernel adds its group sums and the gamma gradient with float atomics, so two runs differ in
// the last bits; here the seven group sums are block sums of doubles in a fixed order (x relative to the group's first element, as
// there), the element-wise pass runs in double from them, and the gamma gradient leaves as one row per sample, [N][C], that the caller
// adds in sample order.  Thread t owns the elements t, t + 256, ... of the group (element e = position e / cpg, channel e % cpg):
// 256 % cpg == 0, so a thread stays on one channel and the channel's sum is the ordered sum of 256 / cpg thread sums.
struct GnTan {
  const void* x; int ldx; const void* xd; int ldxd; const void* y; int ldy;
  void* yd; int ldyd;
  const void* q; int ldq; void* dxd; int lddxd; void* dx; int lddx; float* dgamma_rows;
  const float* gamma; int N, S, C, G, act; float eps;
};
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gn_tangent_kernel(const GnTan a) {
  __shared__ double red[4];
  __shared__ double dgl[256];
  const int g = blockIdx.x, n = blockIdx.y, cpg = a.C / a.G;
  const long E = (long)a.S * cpg;
  const int j = threadIdx.x % cpg, c = g * cpg + j;
  const T* X = reinterpret_cast<const T*>(a.x);
  const T* U = reinterpret_cast<const T*>(a.xd);
  const T* Y = reinterpret_cast<const T*>(a.y);
  const T* Q = reinterpret_cast<const T*>(a.q);
  const double piv = (double)ET<T>::to_f32(X[(long)n * a.S * a.ldx + g * cpg]);
  const double gm = a.gamma ? (double)a.gamma[c] : 1.0;
  double s[7] = {0, 0, 0, 0, 0, 0, 0};
  for (long e = threadIdx.x; e < E; e += 256) {
    const long m = (long)n * a.S + e / cpg;
    const double x = (double)ET<T>::to_f32(X[m * a.ldx + c]) - piv, u = (double)ET<T>::to_f32(U[m * a.ldxd + c]);
    s[0] += x; s[1] += x * x; s[2] += u; s[3] += x * u;
    if constexpr (BWD) {
      double w = (double)ET<T>::to_f32(Q[m * a.ldq + c]) * gm;
      if (a.act != IPOKE_ACT_NONE) w *= (double)act_grad_from_out(a.act, ET<T>::to_f32(Y[m * a.ldy + c]));
      s[4] += w; s[5] += w * x; s[6] += w * u;
    }
  }
#pragma unroll
  for (int k = 0; k < (BWD ? 7 : 4); ++k) s[k] = gan_block_sum(s[k], red);
  const double inv = 1.0 / (double)E;
  const double mu = s[0] * inv, var = fmax(s[1] * inv - mu * mu, 0.0), r = 1.0 / sqrt(var + (double)a.eps);
  const double ub = s[2] * inv, mm = r * (s[3] * inv - mu * ub);
  const double aa = s[4] * inv, bb = r * (s[5] * inv - mu * aa), k0 = s[6] * inv - aa * ub - 3.0 * bb * mm;
  double dg = 0.0;
  for (long e = threadIdx.x; e < E; e += 256) {
    const long m = (long)n * a.S + e / cpg;
    const double xh = (((double)ET<T>::to_f32(X[m * a.ldx + c]) - piv) - mu) * r, u = (double)ET<T>::to_f32(U[m * a.ldxd + c]);
    const double da = a.act != IPOKE_ACT_NONE ? (double)act_grad_from_out(a.act, ET<T>::to_f32(Y[m * a.ldy + c])) : 1.0;
    const double proj = r * (u - ub - xh * mm);
    if constexpr (!BWD) {
      reinterpret_cast<T*>(a.yd)[m * a.ldyd + c] = ET<T>::from_f32((float)(gm * proj * da));
    } else {
      const double qd = (double)ET<T>::to_f32(Q[m * a.ldq + c]) * da, w = qd * gm;
      reinterpret_cast<T*>(a.dxd)[m * a.lddxd + c] = ET<T>::from_f32((float)(r * (w - aa - xh * bb)));
      reinterpret_cast<T*>(a.dx)[m * a.lddx + c] = ET<T>::from_f32((float)(-r * r * (xh * k0 + mm * (w - aa) + bb * (u - ub))));
      dg += qd * proj;
    }
  }
  if (BWD && a.dgamma_rows) {
    dgl[threadIdx.x] = dg;
    __syncthreads();
    if (threadIdx.x < cpg) {
      double t = 0.0;
      for (int k = threadIdx.x; k < 256; k += cpg) t += dgl[k];
      a.dgamma_rows[(long)n * a.C + c] = (float)t;
    }
  }
}

}  // namespace ipoke

using namespace ipoke;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" long ipoke_hinge_terms_partials(void) { return 2 * kHingeBlocks; }

extern "C" int ipoke_hinge_terms(const float* pred, int ld, int64_t M, int mode, float* out, float* grad, int ldg, double* partials,
                                 void* stream) {
  IPK_REQUIRE(pred && out && grad && partials, "pred, out, grad and the partials scratch are needed");
  IPK_REQUIRE(M > 0 && ld >= 1 && ldg >= 1, "bad extents");
  IPK_REQUIRE(mode == IPOKE_HINGE_REAL || mode == IPOKE_HINGE_FAKE || mode == IPOKE_HINGE_GENERATOR, "mode is real, fake or generator");
  long nb = ((long)M + 255) / 256;
  nb = nb > kHingeBlocks ? kHingeBlocks : nb;
  hipLaunchKernelGGL(hinge_terms_kernel, dim3((int)nb), dim3(256), 0, STREAM(stream), pred, ld, (long)M, mode, grad, ldg, partials);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(hinge_final_kernel, dim3(1), dim3(256), 0, STREAM(stream), (const double*)partials, (int)nb, (long)M, out);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_act_jvp(const void* y, int ldy, const void* xdot, int ldx, void* ydot, int ldo, int64_t M, int C, int Cpad, int act,
                             int dtype, void* stream) {
  IPK_REQUIRE(y && xdot && ydot && M > 0 && C > 0, "bad arguments");
  IPK_REQUIRE(Cpad >= C && ldy >= C && ldx >= C && ldo >= Cpad, "pitches must cover the channels (the output's its padded columns)");
  IPK_REQUIRE(act == IPOKE_ACT_LRELU02 || act == IPOKE_ACT_RELU, "the activation is LeakyReLU(0.2) or ReLU");
  IPK_REQUIRE(dtype == IPOKE_F32 || dtype == IPOKE_BF16, "bad dtype");
  const long total = (long)M * Cpad;
  long nb = (total + 255) / 256;
  nb = nb > 4096 ? 4096 : nb;
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(act_jvp_kernel<bf16_t>, dim3((int)nb), dim3(256), 0, STREAM(stream), (const bf16_t*)y, ldy, (const bf16_t*)xdot, ldx,
                       (bf16_t*)ydot, ldo, (long)M, C, Cpad, act);
  else
    hipLaunchKernelGGL(act_jvp_kernel<float>, dim3((int)nb), dim3(256), 0, STREAM(stream), (const float*)y, ldy, (const float*)xdot, ldx,
                       (float*)ydot, ldo, (long)M, C, Cpad, act);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" long ipoke_gp_direction_partials(int N) { return N > 0 ? (long)N * kGpBlocks : 0; }

extern "C" int ipoke_gp_direction(const float* g, int N, int64_t L, float* v, float* out, double* partials, void* stream) {
  IPK_REQUIRE(g && v && out && partials, "g, v, out and the partials scratch are needed");
  IPK_REQUIRE(N > 0 && N <= 65535 && L > 0, "bad extents");
  long nb = ((long)L + 255) / 256;
  nb = nb > kGpBlocks ? kGpBlocks : nb;
  hipLaunchKernelGGL(gp_direction_kernel, dim3((int)nb, N), dim3(256), 0, STREAM(stream), g, N, (long)L, v, partials);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_direction_final_kernel, dim3(1), dim3(256), 0, STREAM(stream), (const double*)partials, (int)nb, N, out);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

static int gn_tangent_fill(GnTan& a, const void* x, int ldx, const void* xd, int ldxd, const void* y, int ldy, const float* gamma, int N, int S,
                           int C, int G, int act, float eps) {
  IPK_REQUIRE(x && xd && N > 0 && N <= 65535 && S > 0 && C > 0 && G > 0 && C % G == 0, "bad arguments");
  IPK_REQUIRE(256 % (C / G) == 0, "the channels of a group must divide 256");
  IPK_REQUIRE(ldx >= C && ldxd >= C, "pitches must cover the channels");
  IPK_REQUIRE(act == IPOKE_ACT_NONE || act == IPOKE_ACT_RELU || act == IPOKE_ACT_LRELU02, "the activation is none, ReLU or LeakyReLU(0.2)");
  IPK_REQUIRE(act == IPOKE_ACT_NONE || (y && ldy >= C), "an activation needs the primal output");
  a = GnTan{};
  a.x = x; a.ldx = ldx; a.xd = xd; a.ldxd = ldxd; a.y = y; a.ldy = ldy; a.gamma = gamma;
  a.N = N; a.S = S; a.C = C; a.G = G; a.act = act; a.eps = eps;
  return IPOKE_OK;
}

extern "C" int ipoke_groupnorm_tangent(const void* x, int ldx, const void* xdot, int ldxd, const void* y, int ldy, void* ydot, int ldyd,
                                       const float* gamma, int N, int S, int C, int G, int act, float eps, int dtype, void* stream) {
  GnTan a; int rc = gn_tangent_fill(a, x, ldx, xdot, ldxd, y, ldy, gamma, N, S, C, G, act, eps); if (rc) return rc;
  IPK_REQUIRE(ydot && ldyd >= C, "ydot must cover the channels");
  IPK_REQUIRE(dtype == IPOKE_F32 || dtype == IPOKE_BF16, "bad dtype");
  a.yd = ydot; a.ldyd = ldyd;
  if (dtype == IPOKE_BF16) hipLaunchKernelGGL((gn_tangent_kernel<bf16_t, false>), dim3(G, N), dim3(256), 0, STREAM(stream), a);
  else hipLaunchKernelGGL((gn_tangent_kernel<float, false>), dim3(G, N), dim3(256), 0, STREAM(stream), a);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_groupnorm_tangent_bwd(const void* x, int ldx, const void* xdot, int ldxd, const void* y, int ldy, const void* q, int ldq,
                                           void* dxdot, int lddxd, void* dx, int lddx, float* dgamma_rows, const float* gamma, int N, int S,
                                           int C, int G, int act, float eps, int dtype, void* stream) {
  GnTan a; int rc = gn_tangent_fill(a, x, ldx, xdot, ldxd, y, ldy, gamma, N, S, C, G, act, eps); if (rc) return rc;
  IPK_REQUIRE(q && dxdot && dx && ldq >= C && lddxd >= C && lddx >= C, "q, dxdot and dx must cover the channels");
  IPK_REQUIRE(!dgamma_rows || gamma, "the gamma gradient needs gamma");
  IPK_REQUIRE(dtype == IPOKE_F32 || dtype == IPOKE_BF16, "bad dtype");
  a.q = q; a.ldq = ldq; a.dxd = dxdot; a.lddxd = lddxd; a.dx = dx; a.lddx = lddx; a.dgamma_rows = dgamma_rows;
  if (dtype == IPOKE_BF16) hipLaunchKernelGGL((gn_tangent_kernel<bf16_t, true>), dim3(G, N), dim3(256), 0, STREAM(stream), a);
  else hipLaunchKernelGGL((gn_tangent_kernel<float, true>), dim3(G, N), dim3(256), 0, STREAM(stream), a);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
