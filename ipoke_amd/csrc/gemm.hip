// Implicit-GEMM convolution kernels on the CDNA4 matrix cores (gfx950).
//
//   igemm_nt : C[m][n] = sum_k A[m][k] * W[n][k]      (forward conv, transposed conv, data gradients)
//   igemm_tn : dW[n][k] = sum_m dY[m][n] * A[m][k]    (weight gradients)
//
// A[m][k] is never materialised: row m is an output position (n, od, oh, ow), k = tap*Kc + c, and
// the loader gathers channel runs of the tap's input position from a channels-last (or arbitrarily
// strided fp32) tensor, zero-filling out-of-range taps.  Tiles are staged global -> VGPR -> LDS
// (double buffered, one barrier per K-block) so that fp32 sources are converted on the fly and, in
// the TN kernel, 8x8 (bf16) / 4x4 (f32) blocks are transposed in registers before they reach LDS.
// 256 threads = 4 wave64; each wave owns MREP x NREP 16x16 accumulator fragments.
#include "common.h"
#include <atomic>
#include <cstring>
#include <mutex>
#include <type_traits>

namespace ipoke {

static constexpr int kPitch = 144;   // 128 B of K per LDS row + 16 B pad

struct GeomDev {
  int M;
  int lDo, lHo, lWo;         // log2 of output dims (pow2 != 0), else unused: rows decode with Do, Ho, Wo by division
  int Do, Ho, Wo, pow2, S;   // output extents; S = Do*Ho*Wo output positions per sample
  int Di, Hi, Wi;
  int khw, kw, taps;         // kh*kw, kw, kd*kh*kw
  int sd, sh, sw, pd, ph, pw;
  int lsd, lsh, lsw;         // log2 strides (transposed mode)
  int transposed;
};

struct NtParams {
  GeomDev g;
  const void* A; int a_f32; long a_sn, a_sd, a_sh, a_sw, a_sc; int a_coff, Kc_real, Kc;
  const void* W; int ldw; int Nout; int Ktot;
  const float* bias; int act; const void* dact; int ld_dact, dact_act;
  void* C; int c_f32, c_acc; long ldc; int c_coff, c_cstride;
  int splitk, kb_per_split, n_pad;
  int tiles_m, tiles_n, xa, xb;
  int prio;            // != 0: raise the waves' issue priority (s_setprio)
  int c_scatter; long c_sn, c_sd, c_sh, c_sw, c_row0;      // output row of position (n, od, oh, ow) when c_scatter (ipoke_conv_desc)
  int w_kmajor;        // 1: W is [Ktot][ldw] -- element (k, n) at W[k * ldw + n] (1x1 kernels: the straight copy of a weight used by its own data gradient)
  const float* row_scale; int rs_images, rs_stride;  // accumulators of image n are multiplied by row_scale[(n / rs_images) * rs_stride] before the bias
  // deterministic split-K accumulation (c_acc && splitk > 1, ipoke_conv_desc.acc_scratch): per-tile arrival counters (zero between
  // launches) and the slab area [tile][split][BM][BN] fp32; null -> the K slices are added with atomics (order-dependent rounding)
  unsigned* acc_cnt; float* acc_part; long acc_part_bytes;
};

// one problem of a batched weight-gradient launch (blockIdx.z): byte/float offsets against the launch's bases
struct TnBatchEntry { long a_off, y_off, w_off; int kh, kw, ph, pw; long sh_off; };      // sh_off: element offset of the problem's operand copy (fused Adam)

struct TnParams {
  GeomDev g;
  const TnBatchEntry* batch; const unsigned char* a_base; const unsigned char* y_base; float* w_base;
  const void* A; int a_f32; long a_sn, a_sd, a_sh, a_sw, a_sc; int a_coff, Kc_real, Kc;
  const void* dY; int ldy, y_coff; int Nout; int Ktot;
  float* dW; long w_sn, w_sc, w_st; int accumulate;
  int splitm, mb_per_split, rows_fixed, Kc_store;
  int tiles_n, tiles_k;
  int xa, xb;          // LDS-DMA kernel: XCD-aware tile map (xa x xb = 8 sub-grids), 0: plain row-major order
  long split_stride;   // > 0: split z stores its slab at dW + z*split_stride instead of atomics
  int tile0, max_wgs;  // first output tile of this launch / cap on workgroups per launch (0: none)
  int z0;              // first problem (batch entry) of this launch
  // Adam-amsgrad in the epilogue (ipoke_wgrad_desc.adam; batched launches of dense 1x1 problems): the gradient tile never leaves
  // the registers -- the tile's parameters and moments are read, updated (adam_amsgrad_update, common.h: the arithmetic every
  // optimizer kernel shares) and written back together with the parameters' cast into the operand copy at ad_sh + sh_off.
  // Pointers are the bases of buffers in the layout of dW (the flat parameter buffer): problem z uses offset batch[z].w_off in all.
  float* ad_p; float* ad_m; float* ad_v; float* ad_vmax; bf16_t* ad_sh; AdamHyper ad_h;
  int ad_keep_grad;    // 1: the gradient tile is ALSO written to dW (tests that compare the update against an optimizer of their own)
};

// decode output row m -> input base coordinates
struct RowPos { long nb; int d0, h0, w0; int ok; };

__device__ __forceinline__ RowPos decode_row(const GeomDev& g, int m, long a_sn) {
  RowPos r;
  r.ok = m < g.M;
  int ow, oh, od, n;
  if (g.pow2) {
    ow = m & ((1 << g.lWo) - 1);
    const int t1 = m >> g.lWo;
    oh = t1 & ((1 << g.lHo) - 1);
    const int t2 = t1 >> g.lHo;
    od = t2 & ((1 << g.lDo) - 1);
    n = t2 >> g.lDo;
  } else {                    // e.g. the 15x15 / 14x14 maps of the 4x4 stride-1 PatchGAN convolutions
    const int t1 = m / g.Wo; ow = m - t1 * g.Wo;
    const int t2 = t1 / g.Ho; oh = t1 - t2 * g.Ho;
    n = t2 / g.Do; od = t2 - n * g.Do;
  }
  r.nb = (long)n * a_sn;
  if (!g.transposed) {
    r.d0 = od * g.sd - g.pd; r.h0 = oh * g.sh - g.ph; r.w0 = ow * g.sw - g.pw;
  } else {
    r.d0 = od + g.pd; r.h0 = oh + g.ph; r.w0 = ow + g.pw;
  }
  return r;
}

// input coordinates of (row, tap); returns validity
__device__ __forceinline__ bool tap_coords(const GeomDev& g, const RowPos& r, int tapcode, int& id, int& ih, int& iw) {
  const int td = tapcode & 0xff, th = (tapcode >> 8) & 0xff, tw = (tapcode >> 16) & 0xff;
  if (!g.transposed) {
    id = r.d0 + td; ih = r.h0 + th; iw = r.w0 + tw;
  } else {
    const int nd = r.d0 - td, nh = r.h0 - th, nw = r.w0 - tw;
    if ((nd | nh | nw) < 0) return false;
    if ((nd & (g.sd - 1)) | (nh & (g.sh - 1)) | (nw & (g.sw - 1))) return false;
    id = nd >> g.lsd; ih = nh >> g.lsh; iw = nw >> g.lsw;
  }
  return (unsigned)id < (unsigned)g.Di && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi;
}

template <typename T> struct Chunk;      // 16 bytes of T
template <> struct Chunk<bf16_t> { typedef bf16x8 type; };
template <> struct Chunk<float> { typedef f32x4 type; };

// gather one 16-byte chunk of A: channels [c, c+E16) of the tap's input position
template <typename T>
__device__ __forceinline__ u32x4 load_a_chunk(const void* A, int a_f32, long off, long a_sc, int a_coff, int c, int Kc_real) {
  constexpr int E16 = ET<T>::E16;
  u32x4 out = {0u, 0u, 0u, 0u};
  if (!a_f32) {
    if (c < Kc_real) out = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(A) + off + a_coff + c);
  } else {
    const float* src = reinterpret_cast<const float*>(A) + off;
    typename Chunk<T>::type v;
#pragma unroll
    for (int e = 0; e < E16; ++e) {
      const int ch = c + e;
      const float f = ch < Kc_real ? src[a_coff + (long)ch * a_sc] : 0.f;
      v[e] = ET<T>::from_f32(f);
    }
    out = *reinterpret_cast<u32x4*>(&v);
  }
  return out;
}

__device__ __forceinline__ void fill_taptab(int* tab, const GeomDev& g) {
  for (int t = threadIdx.x; t < g.taps; t += blockDim.x) {
    const FDiv fkhw(g.khw), fkw(g.kw);
    const int td = fkhw.div(t), rem = t - td * g.khw;
    const int th = fkw.div(rem), tw = rem - th * g.kw;
    tab[t] = td | (th << 8) | (tw << 16);
  }
}

template <typename T> struct Pack4;     // 4 consecutive outputs of the compute dtype
template <> struct Pack4<bf16_t> { typedef __attribute__((ext_vector_type(4))) __bf16 type; };
template <> struct Pack4<float> { typedef f32x4 type; };

// Contract (tests/test_conv_real_gpu.py): an fp32 store carries every activation to a few fp32 ulps of its value, whatever the
// compute dtype (act_apply: expm1f, tanhf, expf).  Only the bf16 STORE of a bf16 launch may take ELU as exp(x) - 1: that form cancels
// for small |x| and its error is absolute, about 2^-24 -- below half a bf16 ulp of the result for |x| >= 2^-15 and never more than
// four times what fl32(exp32(x)) - 1 loses on the host, which is what the tests allow it.  fast_act is that bf16-store form: the
// general sweep of nt_epilogue branches to expm1f for an fp32 store, and the halo / halo16 / c64 kernels, whose sweeps call
// fast_act unconditionally, are not dispatched for an ELU launch that stores fp32 (elu_f32_store below).
template <typename T>
__device__ __forceinline__ float fast_act(int act, float x) {
  // bf16 outputs carry 8 mantissa bits: the hardware exp is more than accurate enough for ELU there
  if (sizeof(T) == 2 && act == IPOKE_ACT_ELU) return x > 0.f ? x : __expf(x) - 1.f;
  return act_apply(act, x);
}

// Epilogue.  The accumulator tile is first parked in LDS (the operand ring is dead by now) and then swept by a
// compact, non-unrolled loop in which consecutive lanes own consecutive 4-column groups of a row: bias /
// activation / derivative-mask are applied once per group and the stores are full-width, row-contiguous.
// (An epilogue unrolled over the 16 register fragments costs more in instruction-cache misses than the whole
// K loop of the small GEMMs of the flow.)
// acc[i][j][r] = C[m0 + wm*MREP*16 + 16i + (lane&15)][n0 + wn*NREP*16 + 16j + 4*(lane>>4) + r]
//
// Fast path (interior tiles of the dtype-output GEMMs with no / ELU activation -- every NICE convolution of the flow): the
// general sweep below is ~1500 instructions of branches that each launch executes once, i.e. straight out of a cold
// instruction cache, and on gfx9 its bias / derivative-mask loads wait on vmcnt, which also counts the previous
// iteration's stores; measured 3.2-3.7 us per launch at the 80 x 128 tile.  The fast path is branch-free: a thread owns ONE
// 4-column group (so its bias is loaded once) in ITER rows, the derivative-mask loads of all rows are issued before the
// accumulators are parked, and ELU / mask are applied by select.
// row of C that holds output position m (dense, or scattered: ipoke_conv_desc.c_scatter)
__device__ __forceinline__ long out_row(const NtParams& p, int m) {
  if (!p.c_scatter) return m;
  const GeomDev& g = p.g;
  int ow, oh, od, n;
  if (g.pow2) {
    ow = m & ((1 << g.lWo) - 1);
    const int t1 = m >> g.lWo;
    oh = t1 & ((1 << g.lHo) - 1);
    const int t2 = t1 >> g.lHo;
    od = t2 & ((1 << g.lDo) - 1);
    n = t2 >> g.lDo;
  } else {
    const int t1 = m / g.Wo; ow = m - t1 * g.Wo;
    const int t2 = t1 / g.Ho; oh = t1 - t2 * g.Ho;
    n = t2 / g.Do; od = t2 - n * g.Do;
  }
  return p.c_row0 + (long)n * p.c_sn + (long)od * p.c_sd + (long)oh * p.c_sh + (long)ow * p.c_sw;
}

// per-image-group scale of the accumulators (ipoke_conv_desc.row_scale): 1/sigma_t of the frame the image belongs to
__device__ __forceinline__ float image_scale(const NtParams& p, int img) {
  return p.row_scale ? p.row_scale[(long)(img / p.rs_images) * p.rs_stride] : 1.f;
}
__device__ __forceinline__ int image_of_row(const GeomDev& g, int m) {
  return g.pow2 ? m >> (g.lDo + g.lHo + g.lWo) : m / g.S;
}

// DET: the instantiation carries the deterministic split-K accumulation (only the skinny tiles a <= 64-column accumulating launch can
// reach: the extra live ranges cost the wide tiles registers, two of them spilled)
template <int WM, int WN, int MREP, int NREP> struct NtDet { static constexpr bool value = WM == 4 && WN == 1 && MREP == 1 && NREP == 4; };
template <typename T, int WM, int WN, int MREP, int NREP, int NTHR = WM * WN * 64, bool DET = false>
__device__ __forceinline__ void nt_epilogue(const NtParams& p, f32x4 (&acc)[MREP][NREP], unsigned char* smem, int m0, int n0,
                                            int wm, int wn, int z, bool writer = true) {
  typedef typename Pack4<T>::type pack_t;
  constexpr int BM = WM * MREP * 16, BN = WN * NREP * 16;
  constexpr int EP = BN * 4 + 16;                      // staging pitch in bytes
  const GeomDev& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63;
  constexpr int G4F = BN / 4;
  if constexpr (DET) if (p.splitk > 1 && p.c_acc && p.acc_part != nullptr) {
    // Deterministic accumulation of the K slices into an fp32 tensor that already holds a value (the conv1 data gradient of every
    // coupling net adds into the gradient state, flow_engine.hip; the reference trains with deterministic=True,
    // experiments/experiment.py:33, 86).  The counter form of cdna_hip_programming.md Guideline 16: every slice parks its tile in
    // the slab [tile][z] with write-through (sc1) stores, drains them, and draws a ticket from the tile's counter; the workgroup
    // that draws the last ticket -- whichever it is -- reads the splitk slabs back with sc1 loads, sums them in a FIXED order
    // (groups of eight slices pairwise, the groups in order) and adds the sum to C with plain read-modify-writes: every element has
    // exactly one writer and the rounding no longer depends on the order in which the slices finish.  No spin, nothing to time out;
    // the counter is back at zero when the launch ends.
    typedef __amdgpu_buffer_rsrc_t rsrc_t;
    __syncthreads();
    if (writer) {
      unsigned char* base = smem + (wm * MREP * 16 + (lane & 15)) * EP + (wn * NREP * 16 + (lane >> 4) * 4) * 4;
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(base + i * 16 * EP + j * 64) = acc[i][j];
    }
    __syncthreads();
    const int tile = (m0 / BM) * p.tiles_n + n0 / BN;
    constexpr int SLAB = BM * BN * 4;                      // bytes
    const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<unsigned char*>(p.acc_part) + (long)tile * p.splitk * SLAB, 0,
                                                        p.splitk * SLAB, 0x00020000);
    for (int idx = tid; idx < BM * G4F; idx += NTHR) {
      const int row = idx / G4F, c4 = idx - row * G4F;
      const f32x4 v = *reinterpret_cast<const f32x4*>(smem + row * EP + c4 * 16);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, z * SLAB + (row * BN + 4 * c4) * 4, 0, 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's slab stores have reached the memory side
    __syncthreads();
    unsigned* flag = reinterpret_cast<unsigned*>(smem);    // (the staging tile is dead)
    if (tid == 0) *flag = __hip_atomic_fetch_add(p.acc_cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != (unsigned)(p.splitk - 1)) return;
    if (tid == 0) __hip_atomic_store(p.acc_cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int idx = tid; idx < BM * G4F; idx += NTHR) {
      const int row = idx / G4F, c4 = idx - row * G4F;
      const int m = m0 + row, n = n0 + 4 * c4;
      if (m >= g.M || n >= p.Nout) continue;
      const int off = (row * BN + 4 * c4) * 4;
      f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s0 = 0; s0 < p.splitk; s0 += 8) {
        f32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {                      // (always load, clamp the index: no branch around a load)
          const int sl = s0 + k < p.splitk ? s0 + k : p.splitk - 1;
          v[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, sl * SLAB + off, 0, 16));
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) if (s0 + k >= p.splitk) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        sum += ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
      }
      float* Cp = reinterpret_cast<float*>(p.C) + (long)m * p.ldc + p.c_coff;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < p.Nout) Cp[(long)(n + r) * p.c_cstride] += sum[r];
    }
    return;
  }
  if constexpr ((BM * G4F) % NTHR == 0 && NTHR % G4F == 0) {
    constexpr int ITER = BM * G4F / NTHR, RSTEP = NTHR / G4F;
    const bool fast = p.splitk == 1 && !p.c_scatter && !p.row_scale && !p.c_f32 && (p.Nout & 3) == 0 && m0 + BM <= g.M && n0 + BN <= p.Nout &&
                      ((p.ldc | p.c_coff) & 3) == 0 && (p.act == IPOKE_ACT_NONE || p.act == IPOKE_ACT_ELU) &&
                      (!p.dact || ((p.ld_dact & 3) == 0 && p.dact_act == IPOKE_ACT_ELU));
    if (fast) {
      const int c4 = tid % G4F, r0 = tid / G4F, n = n0 + 4 * c4;
      f32x4 b4 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p.bias) b4 = *reinterpret_cast<const f32x4*>(p.bias + n);
      pack_t dy[ITER];
#pragma unroll
      for (int k = 0; k < ITER; ++k) dy[k] = pack_t{};
      if (p.dact) {
        const T* dp = reinterpret_cast<const T*>(p.dact) + (long)(m0 + r0) * p.ld_dact + n;
#pragma unroll
        for (int k = 0; k < ITER; ++k) dy[k] = *reinterpret_cast<const pack_t*>(dp + (long)k * RSTEP * p.ld_dact);
      }
      __syncthreads();
      if (writer) {
        unsigned char* base = smem + (wm * MREP * 16 + (lane & 15)) * EP + (wn * NREP * 16 + (lane >> 4) * 4) * 4;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(base + i * 16 * EP + j * 64) = acc[i][j];
      }
      __syncthreads();
      const bool elu = p.act == IPOKE_ACT_ELU, mask = p.dact != nullptr;
      T* Cp = reinterpret_cast<T*>(p.C) + (long)(m0 + r0) * p.ldc + p.c_coff + n;
      const unsigned char* sp = smem + r0 * EP + c4 * 16;
#pragma unroll
      for (int k = 0; k < ITER; ++k) {
        f32x4 v = *reinterpret_cast<const f32x4*>(sp + k * RSTEP * EP);
        v += b4;
        pack_t o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = fast_act<T>(IPOKE_ACT_ELU, v[r]);
          float x = elu ? e : v[r];
          const float y = ET<T>::to_f32(dy[k][r]);
          x *= (mask && y <= 0.f) ? y + 1.f : 1.f;
          o[r] = ET<T>::from_f32(x);
        }
        *reinterpret_cast<pack_t*>(Cp + (long)k * RSTEP * p.ldc) = o;
      }
      return;
    }
    // split-K partial sums of an interior tile (conv3 of every coupling net): raw fp32 rows, nothing to apply
    if (p.splitk > 1 && !p.c_acc && m0 + BM <= g.M && n0 + BN <= p.ldc && (p.ldc & 3) == 0) {
      const int c4 = tid % G4F, r0 = tid / G4F;
      __syncthreads();
      if (writer) {
        unsigned char* base = smem + (wm * MREP * 16 + (lane & 15)) * EP + (wn * NREP * 16 + (lane >> 4) * 4) * 4;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(base + i * 16 * EP + j * 64) = acc[i][j];
      }
      __syncthreads();
      float* P = reinterpret_cast<float*>(p.C) + ((long)z * g.M + m0 + r0) * p.ldc + n0 + 4 * c4;
      const unsigned char* sp = smem + r0 * EP + c4 * 16;
#pragma unroll
      for (int k = 0; k < ITER; ++k)
        *reinterpret_cast<f32x4*>(P + (long)k * RSTEP * p.ldc) = *reinterpret_cast<const f32x4*>(sp + k * RSTEP * EP);
      return;
    }
  }
  __syncthreads();
  if (writer) {      // (waves of the second K half of an in-workgroup K split hold nothing of their own any more)
    unsigned char* base = smem + (wm * MREP * 16 + (lane & 15)) * EP + (wn * NREP * 16 + (lane >> 4) * 4) * 4;
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(base + i * 16 * EP + j * 64) = acc[i][j];
  }
  __syncthreads();
  const bool vec_ok = (p.Nout & 3) == 0;                 // 4-wide groups never straddle Nout
  constexpr int G4 = BN / 4;
  for (int idx = tid; idx < BM * G4; idx += blockDim.x) {
    const int row = idx / G4, c4 = idx - row * G4;
    const int m = m0 + row, n = n0 + 4 * c4;
    if (m >= g.M || n >= p.n_pad) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(smem + row * EP + c4 * 16);
    if (p.splitk > 1) {
      if (p.c_acc) {          // K slices added atomically into an fp32 tensor that already holds a value
        float* Cp = reinterpret_cast<float*>(p.C) + (long)m * p.ldc + p.c_coff;
        for (int r = 0; r < 4; ++r)
          if (n + r < p.Nout) atomicAdd(Cp + (long)(n + r) * p.c_cstride, v[r]);
      } else {
        float* P = reinterpret_cast<float*>(p.C) + ((long)z * g.M + m) * p.ldc + n;
        if (n + 3 < p.ldc) *reinterpret_cast<f32x4*>(P) = v;    // ldc is padded to a multiple of 4
        else for (int r = 0; r < 4; ++r) if (n + r < p.ldc) P[r] = v[r];
      }
      continue;
    }
    const bool full = vec_ok && n + 3 < p.Nout;
    if (p.row_scale) v *= image_scale(p, image_of_row(g, m));
    if (p.bias) {
      if (full) v += *reinterpret_cast<const f32x4*>(p.bias + n);
      else for (int r = 0; r < 4; ++r) if (n + r < p.Nout) v[r] += p.bias[n + r];
    }
    if (sizeof(T) == 2 && p.c_f32 && p.act == IPOKE_ACT_ELU) {
      // fp32 store of a bf16 launch: expm1f, not fast_act's exp(x) - 1 (one copy of it: this sweep is not the hot path)
#pragma nounroll
      for (int r = 0; r < 4; ++r) { const float x = v[r]; v[r] = x > 0.f ? x : expm1f(x); }
    } else if (p.act != IPOKE_ACT_NONE) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = fast_act<T>(p.act, v[r]);
    }
    if (p.dact) {
      const T* dp = reinterpret_cast<const T*>(p.dact) + (long)m * p.ld_dact + n;
      if (full && (p.ld_dact & 3) == 0) {
        const pack_t y = *reinterpret_cast<const pack_t*>(dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= act_grad_from_out(p.dact_act, ET<T>::to_f32(y[r]));
      } else {
        for (int r = 0; r < 4; ++r)
          if (n + r < p.Nout) v[r] *= act_grad_from_out(p.dact_act, ET<T>::to_f32(dp[r]));
      }
    }
    if (!full) {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (n + r >= p.Nout) v[r] = 0.f;
    }
    if (p.c_f32) {
      float* Cp = reinterpret_cast<float*>(p.C) + out_row(p, m) * p.ldc + p.c_coff;
      if (full && p.c_cstride == 1 && !p.c_acc && ((p.ldc | p.c_coff) & 3) == 0) {
        *reinterpret_cast<f32x4*>(Cp + n) = v;
      } else {
        for (int r = 0; r < 4; ++r) {
          if (n + r < p.Nout) {
            float* q = Cp + (long)(n + r) * p.c_cstride;
            *q = p.c_acc ? *q + v[r] : v[r];
          }
        }
      }
    } else {
      T* Cp = reinterpret_cast<T*>(p.C) + out_row(p, m) * p.ldc + p.c_coff + n;
      // columns up to n_pad are written (zero beyond Nout) so that consumers can read a padded K
      if (n + 3 < p.n_pad && ((p.ldc | p.c_coff) & 3) == 0) {
        pack_t o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = ET<T>::from_f32(v[r]);
        *reinterpret_cast<pack_t*>(Cp) = o;
      } else {
        for (int r = 0; r < 4; ++r)
          if (n + r < p.n_pad) Cp[r] = ET<T>::from_f32(v[r]);
      }
    }
  }
}

// f32 launches: v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain that rounds once per product, so one accumulator over the whole
// reduction loses several ulp32 of sum |x w| (4.6 measured at K = 288, tests/test_conv_real_gpu.py).  The f32 instantiations of the
// two implicit-GEMM kernels therefore close the chain after every pass of their K loop (32 or 64 elements) and add it to a second
// accumulator: the chain the rounding errors grow along is K / 32 long instead of K (about 1 ulp32 of sum |x w|).  bf16 launches
// round once per 32-element matrix-core step already and keep the single accumulator.
template <typename T, int MREP, int NREP>
__device__ __forceinline__ void fold_chain(f32x4 (&tot)[sizeof(T) == 4 ? MREP : 1][sizeof(T) == 4 ? NREP : 1], f32x4 (&acc)[MREP][NREP]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }
}
template <typename T, int MREP, int NREP>
__device__ __forceinline__ void take_chain(f32x4 (&tot)[sizeof(T) == 4 ? MREP : 1][sizeof(T) == 4 ? NREP : 1], f32x4 (&acc)[MREP][NREP]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) acc[i][j] = tot[i][j];
  }
}

// =============================================================================================
template <typename T, int WM, int WN, int MREP, int NREP>
__global__ __launch_bounds__(256) void igemm_nt_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  constexpr int BM = WM * MREP * 16, BN = WN * NREP * 16;
  constexpr int E16 = ET<T>::E16;
  constexpr int BK = 128 / (int)sizeof(T);
  constexpr int A_IT = (BM * 8 + 255) / 256, B_IT = (BN * 8 + 255) / 256;
  typedef typename ET<T>::frag frag_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sA = smem;
  unsigned char* sB = smem + 2 * BM * kPitch;
  constexpr int kRing = 2 * (BM + BN) * kPitch > BM * (BN * 4 + 16) ? 2 * (BM + BN) * kPitch : BM * (BN * 4 + 16);
  int* taptab = reinterpret_cast<int*>(smem + kRing);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const GeomDev& g = p.g;

  int tm, tn;
  {
    const int bid = blockIdx.x;
    if (p.xa > 0) {
      const int xcd = bid & 7, q = bid >> 3;
      const FDiv fxa(p.xa), fxb(p.xb);
      const int sub_m = fxa.div(p.tiles_m), sub_n = fxb.div(p.tiles_n);
      const FDiv fsm(sub_m);
      tm = fxa.mod(xcd) * sub_m + fsm.mod(q);
      tn = fxa.div(xcd) * sub_n + fsm.div(q);
    } else {
      const FDiv ftm(p.tiles_m);
      tm = ftm.mod(bid); tn = ftm.div(bid);
    }
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int z = blockIdx.y;
  const int nkb_total = (p.Ktot + BK - 1) / BK;
  const int kb_begin = z * p.kb_per_split;
  const int kb_end = min(nkb_total, kb_begin + p.kb_per_split);

  fill_taptab(taptab, g);

  // per-thread chunk bookkeeping
  RowPos arow[A_IT]; int a_tap[A_IT], a_c[A_IT]; int a_lds[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int ch = tid + 256 * i;
    const int row = ch >> 3, kc = ch & 7;
    const bool in_tile = row < BM;
    arow[i] = decode_row(g, m0 + row, p.a_sn);
    arow[i].ok = arow[i].ok && in_tile;
    const int kglob = kb_begin * BK + kc * E16;
    a_tap[i] = FDiv(p.Kc).div(kglob);
    a_c[i] = kglob - a_tap[i] * p.Kc;
    a_lds[i] = in_tile ? row * kPitch + kc * 16 : -1;
  }
  int b_row[B_IT], b_k[B_IT], b_lds[B_IT];
#pragma unroll
  for (int i = 0; i < B_IT; ++i) {
    const int ch = tid + 256 * i;
    const int row = ch >> 3, kc = ch & 7;
    b_row[i] = (row < BN && n0 + row < p.Nout) ? n0 + row : -1;
    b_k[i] = kb_begin * BK + kc * E16;
    b_lds[i] = row < BN ? row * kPitch + kc * 16 : -1;
  }
  __syncthreads();   // taptab ready

  u32x4 ra[A_IT], rb[B_IT];
  auto load_stage = [&]() {
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (arow[i].ok && a_tap[i] < g.taps) {
        int id, ih, iw;
        if (tap_coords(g, arow[i], taptab[a_tap[i]], id, ih, iw)) {
          const long off = arow[i].nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw;
          v = load_a_chunk<T>(p.A, p.a_f32, off, p.a_sc, p.a_coff, a_c[i], p.Kc_real);
        }
      }
      ra[i] = v;
      a_c[i] += BK;
      while (a_c[i] >= p.Kc) { a_c[i] -= p.Kc; ++a_tap[i]; }
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (b_row[i] >= 0 && b_k[i] < p.Ktot)       // (K columns past the reduction multiply zero A chunks -- but 0 x NaN is NaN: W may be a column slice of a wider operand)
        v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(p.W) + (long)b_row[i] * p.ldw + b_k[i]);
      rb[i] = v;
      b_k[i] += BK;
    }
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_IT; ++i)
      if (a_lds[i] >= 0) *reinterpret_cast<u32x4*>(sA + buf * BM * kPitch + a_lds[i]) = ra[i];
#pragma unroll
    for (int i = 0; i < B_IT; ++i)
      if (b_lds[i] >= 0) *reinterpret_cast<u32x4*>(sB + buf * BN * kPitch + b_lds[i]) = rb[i];
  };

  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 tot[sizeof(T) == 4 ? MREP : 1][sizeof(T) == 4 ? NREP : 1];
#pragma unroll
  for (int i = 0; i < (sizeof(T) == 4 ? MREP : 1); ++i)
#pragma unroll
    for (int j = 0; j < (sizeof(T) == 4 ? NREP : 1); ++j) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (kb_begin < kb_end) {
    load_stage();
    store_stage(0);
    __syncthreads();
    for (int kb = kb_begin; kb < kb_end; ++kb) {
      const int buf = (kb - kb_begin) & 1;
      const bool more = kb + 1 < kb_end;
      if (more) load_stage();
      const unsigned char* a_base = sA + buf * BM * kPitch + (wm * MREP * 16 + (lane & 15)) * kPitch + (lane >> 4) * 16;
      const unsigned char* b_base = sB + buf * BN * kPitch + (wn * NREP * 16 + (lane & 15)) * kPitch + (lane >> 4) * 16;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        frag_t fa[MREP], fb[NREP];
#pragma unroll
        for (int i = 0; i < MREP; ++i) fa[i] = *reinterpret_cast<const frag_t*>(a_base + i * 16 * kPitch + s * 64);
#pragma unroll
        for (int j = 0; j < NREP; ++j) fb[j] = *reinterpret_cast<const frag_t*>(b_base + j * 16 * kPitch + s * 64);
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) mma64(fa[i], fb[j], acc[i][j]);
      }
      fold_chain<T, MREP, NREP>(tot, acc);
      if (more) store_stage(buf ^ 1);
      __syncthreads();
    }
  }
  take_chain<T, MREP, NREP>(tot, acc);

  nt_epilogue<T, WM, WN, MREP, NREP, WM * WN * 64, NtDet<WM, WN, MREP, NREP>::value>(p, acc, smem, m0, n0, wm, wn, z);
}

// =============================================================================================
// Multi-stage LDS-DMA variant of igemm_nt for activations already in the compute dtype.
// Tiles go global -> LDS with global_load_lds_dwordx4 (no VGPR staging) into an NSTAGE-deep ring, so
// (NSTAGE-1) K-blocks of loads are in flight while one is consumed: the small-M GEMMs of the flow give
// each CU a single workgroup, and this depth is what hides the L2/HBM latency.  The DMA destination is
// lane-linear (8 lanes = one 128-byte row), so bank conflicts are avoided by permuting the SOURCE
// chunk: LDS position p of row r holds K-chunk p ^ ((r >> 1) & 7); fragment reads apply the same XOR.
// Waits are counted (s_waitcnt vmcnt(N)) and barriers are raw s_barrier so that loads survive them.
__device__ __attribute__((aligned(16))) unsigned int g_zero_chunk[4];

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// WK = 2: in-workgroup K split.  The waves form two groups that own the two 32-deep halves of every K-block and the same
// WM x WN output tiling; the partial accumulators meet in LDS once, before the epilogue.  A wave then owns a tile twice as
// wide for the same number of waves (e.g. 80 x 32 instead of 80 x 16 at 8 waves on an 80 x 128 tile): 7 instead of 12
// fragment reads per 10 MFMAs, 56 instead of 96 KB of LDS reads per K-block -- the fragment reads, not the matrix cores,
// bound the math side of these small-M GEMMs (every wave re-reads the whole A tile).
template <typename T, int WM, int WN, int MREP, int NREP, int NSTAGE, int KPB, bool SIMPLE, int WK = 1>
__global__ __launch_bounds__(WM * WN * WK * 64) void igemm_nt_glds_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  constexpr int NTHR = WM * WN * WK * 64;          // 4 or 8 wave64 (8 waves = two per SIMD: one's LDS reads hide under the other's MFMAs)
  constexpr int BM = WM * MREP * 16, BN = WN * NREP * 16;
  constexpr int E16 = ET<T>::E16;
  constexpr int BK = 128 / (int)sizeof(T);
  constexpr int A_IT = (BM * 8 + NTHR - 1) / NTHR, B_IT = (BN * 8 + NTHR - 1) / NTHR, L = A_IT + B_IT;
  constexpr int SUB = (BM + BN) * 128;            // one K-block of both operands
  constexpr int STAGE = KPB * SUB;                // ring slot: KPB K-blocks are consumed per barrier
  static_assert(BM % 8 == 0 && BN % 8 == 0, "tile rows must fill whole DMA instructions");
  static_assert((NSTAGE - 2) * L * KPB <= 63, "vmcnt field");
  typedef typename ET<T>::frag frag_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* dummy = smem + NSTAGE * STAGE;                         // 1 KB per wave: landing zone of padding DMAs
  int* taptab = reinterpret_cast<int*>(smem + NSTAGE * STAGE + NTHR * 16);
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);     // chain kernels win the SIMD's issue arbitration against co-resident side-stream waves

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wk = wave / (WM * WN), wr = wave % (WM * WN);
  const int wm = wr / WN, wn = wr % WN;
  const GeomDev& g = p.g;
  int tm, tn;
  {
    const int bid = blockIdx.x;
    if (p.xa > 0) {
      const int xcd = bid & 7, q = bid >> 3;
      const FDiv fxa(p.xa), fxb(p.xb);                   // (powers of two: pick_xcd_map)
      const int sub_m = fxa.div(p.tiles_m), sub_n = fxb.div(p.tiles_n);
      const FDiv fsm(sub_m);
      tm = fxa.mod(xcd) * sub_m + fsm.mod(q);
      tn = fxa.div(xcd) * sub_n + fsm.div(q);
    } else {
      const FDiv ftm(p.tiles_m);
      tm = ftm.mod(bid); tn = ftm.div(bid);
    }
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int z = blockIdx.y;
  const int nkb_total = (p.Ktot + BK - 1) / BK;
  const int kb_begin = z * p.kb_per_split;
  const int kb_end = min(nkb_total, kb_begin + p.kb_per_split);

  fill_taptab(taptab, g);

  // Per-chunk source bookkeeping.  SIMPLE (Kc a multiple of the K-block, no channel padding): a K-block lies in
  // ONE tap for every chunk, so the loop only adds BK to 32-bit element offsets and re-derives input positions on
  // the (wave-uniform, rare) tap change.  General: per-chunk tap tracking.  Host guarantees offsets < 2^31.
  constexpr unsigned kInvalid = 0xffffffffu;
  RowPos arow[A_IT]; int a_tap[A_IT], a_c[A_IT]; unsigned a_off[A_IT]; bool a_in[A_IT];
  auto a_resolve = [&](int i) {
    unsigned off = kInvalid;
    if (arow[i].ok && a_tap[i] < g.taps && a_c[i] < p.Kc_real) {
      int id, ih, iw;
      if (tap_coords(g, arow[i], taptab[a_tap[i]], id, ih, iw))
        off = (unsigned)(arow[i].nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw + p.a_coff + a_c[i]);
    }
    a_off[i] = off;
  };
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int ch = tid + NTHR * i;
    const int row = ch >> 3, pos = ch & 7;
    a_in[i] = row < BM;
    arow[i] = decode_row(g, m0 + row, p.a_sn);
    arow[i].ok = arow[i].ok && a_in[i];
    const int kglob = kb_begin * BK + (pos ^ ((row >> 1) & 7)) * E16;
    a_tap[i] = FDiv(p.Kc).div(kglob);
    a_c[i] = kglob - a_tap[i] * p.Kc;
  }
  unsigned b_off[B_IT]; int b_k[B_IT]; bool b_in[B_IT];
#pragma unroll
  for (int i = 0; i < B_IT; ++i) {
    const int ch = tid + NTHR * i;
    const int row = ch >> 3, pos = ch & 7;
    b_in[i] = row < BN;
    b_k[i] = kb_begin * BK + (pos ^ ((row >> 1) & 7)) * E16;
    b_off[i] = (row < BN && n0 + row < p.Nout) ? (unsigned)((long)(n0 + row) * p.ldw + b_k[i]) : kInvalid;
  }
  __syncthreads();   // taptab ready (nothing in flight yet)
#pragma unroll
  for (int i = 0; i < A_IT; ++i) a_resolve(i);

  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  int c_uni = FDiv(p.Kc).mod(kb_begin * BK);             // SIMPLE: channel offset of the K-block inside its tap (uniform)
  auto issue = [&](int slot_bytes, bool real) {
    unsigned char* sa = smem + slot_bytes;
    if (!real) {                                   // keep the vmcnt bookkeeping uniform past the last K-block
#pragma unroll
      for (int i = 0; i < L; ++i)
        __builtin_amdgcn_global_load_lds((glb_void*)zero, (lds_void*)(dummy + wave * 1024), 16, 0, 0);
      return;
    }
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const T* src = a_off[i] != kInvalid ? Abase + a_off[i] : zero;
      unsigned char* dst = (wave * 64 + NTHR * i) < BM * 8 ? sa + (wave * 64 + NTHR * i) * 16 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      // K columns past Ktot meet zero A chunks, but they must not be FETCHED: W may be a column slice of a wider operand (the parity-class
      // data gradients of first_stage_train._dgrad_phases), whose last row ends at the end of the allocation, and 0 x NaN = NaN
      const T* src = (b_off[i] != kInvalid && (SIMPLE || b_k[i] < p.Ktot)) ? Wbase + b_off[i] : zero;
      unsigned char* dst = (wave * 64 + NTHR * i) < BN * 8 ? sa + BM * 128 + (wave * 64 + NTHR * i) * 16 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
      if (!SIMPLE) b_k[i] += BK;
      if (b_off[i] != kInvalid) b_off[i] += BK;
    }
    if (SIMPLE) {
      c_uni += BK;
      if (c_uni >= p.Kc) {                          // uniform: every chunk enters the next tap together
        c_uni = 0;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) { ++a_tap[i]; a_c[i] -= p.Kc - BK; a_resolve(i); }
      } else {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) { a_c[i] += BK; if (a_off[i] != kInvalid) a_off[i] += BK; }
      }
    } else {
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        a_c[i] += BK;
        while (a_c[i] >= p.Kc) { a_c[i] -= p.Kc; ++a_tap[i]; }
        a_resolve(i);
      }
    }
  };

  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 tot[sizeof(T) == 4 ? MREP : 1][sizeof(T) == 4 ? NREP : 1];
#pragma unroll
  for (int i = 0; i < (sizeof(T) == 4 ? MREP : 1); ++i)
#pragma unroll
    for (int j = 0; j < (sizeof(T) == 4 ? NREP : 1); ++j) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // loop-invariant LDS offsets of this lane's fragments (XOR swizzle folded in)
  int a_rd[MREP][2], b_rd[NREP][2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int q = s * 4 + (lane >> 4);
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
      const int row = wm * MREP * 16 + i * 16 + (lane & 15);
      a_rd[i][s] = row * 128 + ((q ^ ((row >> 1) & 7)) * 16);
    }
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const int row = wn * NREP * 16 + j * 16 + (lane & 15);
      b_rd[j][s] = BM * 128 + row * 128 + ((q ^ ((row >> 1) & 7)) * 16);
    }
  }
  int kb_issue = kb_begin;                        // next K-block to be requested
  auto issue_slot = [&](int slot) {
#pragma unroll
    for (int u = 0; u < KPB; ++u) {
      issue(slot * STAGE + u * SUB, kb_issue < kb_end);
      ++kb_issue;
    }
  };
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s) issue_slot(s);

  auto load_frags = [&](const unsigned char* sub, int hs, frag_t* fa, frag_t* fb) {
#pragma unroll
    for (int i = 0; i < MREP; ++i) fa[i] = *reinterpret_cast<const frag_t*>(sub + a_rd[i][hs]);
#pragma unroll
    for (int j = 0; j < NREP; ++j) fb[j] = *reinterpret_cast<const frag_t*>(sub + b_rd[j][hs]);
  };
  int a_rdw[MREP], b_rdw[NREP];                  // WK = 2: offsets of this wave group's K half (a runtime select, done once)
#pragma unroll
  for (int i = 0; i < MREP; ++i) a_rdw[i] = wk ? a_rd[i][1] : a_rd[i][0];
#pragma unroll
  for (int j = 0; j < NREP; ++j) b_rdw[j] = wk ? b_rd[j][1] : b_rd[j][0];
  auto load_half = [&](const unsigned char* sub, frag_t* fa, frag_t* fb) {
#pragma unroll
    for (int i = 0; i < MREP; ++i) fa[i] = *reinterpret_cast<const frag_t*>(sub + a_rdw[i]);
#pragma unroll
    for (int j = 0; j < NREP; ++j) fb[j] = *reinterpret_cast<const frag_t*>(sub + b_rdw[j]);
  };
  int slot = 0;
  for (int kb = kb_begin; kb < kb_end; kb += KPB) {
    wait_vmcnt<(NSTAGE - 2) * L * KPB>();      // this wave's share of the oldest slot has landed
    __builtin_amdgcn_s_barrier();                     // ... and everybody else's; all reads of the slot refilled below are done
    issue_slot((slot + NSTAGE - 1) % NSTAGE);
    const unsigned char* base = smem + slot * STAGE;
    slot = (slot + 1) % NSTAGE;
    const int nsub = min(KPB, kb_end - kb);
    if constexpr (WK == 1) {
      // 2*nsub half-steps; fragments of half-step h+1 are fetched while the matrix cores work on h
      frag_t fa[2][MREP], fb[2][NREP];
      load_frags(base, 0, fa[0], fb[0]);
#pragma unroll
      for (int h = 0; h < 2 * KPB; ++h) {
        if (h < 2 * nsub) {
          if (h + 1 < 2 * nsub) load_frags(base + ((h + 1) >> 1) * SUB, (h + 1) & 1, fa[(h + 1) & 1], fb[(h + 1) & 1]);
#pragma unroll
          for (int i = 0; i < MREP; ++i)
#pragma unroll
            for (int j = 0; j < NREP; ++j) mma64(fa[h & 1][i], fb[h & 1][j], acc[i][j]);
        }
      }
    } else {
      // this wave group owns K half `wk` of every K-block of the slot
      frag_t fa[2][MREP], fb[2][NREP];
      load_half(base, fa[0], fb[0]);
#pragma unroll
      for (int t = 0; t < KPB; ++t) {
        if (t < nsub) {
          if (t + 1 < nsub) load_half(base + (t + 1) * SUB, fa[(t + 1) & 1], fb[(t + 1) & 1]);
#pragma unroll
          for (int i = 0; i < MREP; ++i)
#pragma unroll
            for (int j = 0; j < NREP; ++j) mma64(fa[t & 1][i], fb[t & 1][j], acc[i][j]);
        }
      }
    }
    fold_chain<T, MREP, NREP>(tot, acc);
  }
  take_chain<T, MREP, NREP>(tot, acc);
  wait_vmcnt<0>();                         // only padding DMAs (to the dummy zone) can still be in flight
  if constexpr (WK > 1) {                  // the two K halves meet: group 1 hands its partial sums to group 0 through LDS
    constexpr int EP = BN * 4 + 16;
    unsigned char* st2 = smem + BM * EP + (wm * MREP * 16 + (lane & 15)) * EP + (wn * NREP * 16 + (lane >> 4) * 4) * 4;
    __syncthreads();                       // every read of the ring is done
    if (wk == 1) {
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(st2 + i * 16 * EP + j * 64) = acc[i][j];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) acc[i][j] += *reinterpret_cast<const f32x4*>(st2 + i * 16 * EP + j * 64);
    }
  }
  nt_epilogue<T, WM, WN, MREP, NREP, NTHR, WK == 1 && NtDet<WM, WN, MREP, NREP>::value>(p, acc, smem, m0, n0, wm, wn, z, wk == 0);
}

// =============================================================================================
// weight gradient
template <typename T, int NR>
__global__ __launch_bounds__(256) void igemm_tn_kernel(const TnParams pin) {
  kernarg_prefetch<(int)sizeof(TnParams)>();
  TnParams p = pin;
  if (pin.batch) {                       // batched launch: blockIdx.z selects operands and the 2-D tap geometry
    const TnBatchEntry e = pin.batch[blockIdx.z + pin.z0];
    p.A = pin.a_base + e.a_off; p.dY = pin.y_base + e.y_off; p.dW = pin.w_base + e.w_off;
    p.g.khw = e.kh * e.kw; p.g.kw = e.kw; p.g.taps = e.kh * e.kw; p.g.ph = e.ph; p.g.pw = e.pw;
  }
  constexpr int TN_ = 128, TK_ = 128;          // output tile: 128 out-channels x 128 k
  constexpr int E16 = ET<T>::E16;
  constexpr int RM = 128 / (int)sizeof(T);     // reduction rows per stage
  constexpr int LOGE = E16 == 8 ? 3 : 2;
  constexpr int NBLK = (RM / E16) * (128 / E16);   // ExE blocks per operand tile (bf16: 128, f32: 256)
  constexpr int PER_OP = NBLK / 256 == 0 ? 1 : NBLK / 256;   // blocks per thread per operand (f32: 1)
  typedef typename ET<T>::frag frag_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sY = smem;                         // [2][128][kPitch]  rows = out-channel n, 128 B of m
  unsigned char* sX = smem + 2 * TN_ * kPitch;      // [2][128][kPitch]  rows = k
  int* taptab = reinterpret_cast<int*>(smem + 4 * 128 * kPitch);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const GeomDev& g = p.g;
  const int tile = (int)blockIdx.x + p.tile0;
  const int tn = FDiv(p.tiles_n).mod(tile), tk = FDiv(p.tiles_n).div(tile);
  const int n0 = tn * TN_, k0 = tk * TK_;
  const int z = blockIdx.y;
  const int nmb_total = (g.M + RM - 1) / RM;      // (RM: compile-time)
  const int mb_begin = z * p.mb_per_split, mb_end = min(nmb_total, mb_begin + p.mb_per_split);

  fill_taptab(taptab, g);

  // Work split.  bf16: threads 0..127 stage dY blocks, 128..255 stage A blocks (one 8x8 block each).
  //              f32 : every thread stages one 4x4 block of dY and one of A.
  // block id -> (mb, cb): cb fastest so that a wave's loads run along the contiguous dimension.
  constexpr int CB = 128 / E16;                 // column blocks per tile row (16 / 32)
  const bool do_y = (E16 == 8) ? (tid < 128) : true;
  const bool do_x = (E16 == 8) ? (tid >= 128) : true;
  const int blk = (E16 == 8) ? (tid & 127) : tid;
  const int cb = blk % CB, mbk = blk / CB;      // mbk in [0, RM/E16) = [0,8)
  (void)PER_OP;

  // A-operand column bookkeeping (fixed for the whole reduction)
  const int kcol = k0 + cb * E16;
  const int x_tap = FDiv(p.Kc).div(kcol), x_c = kcol - x_tap * p.Kc;
  const bool x_col_ok = do_x && kcol < p.Ktot;
  const int ncol = n0 + cb * E16;
  const bool y_col_ok = do_y && ncol < ((p.Nout + E16 - 1) / E16) * E16;
  __syncthreads();
  const int x_tapcode = x_col_ok ? taptab[x_tap] : 0;

  // Fast path (p.rows_fixed: a reduction block of RM rows covers whole samples, e.g. the 8x8 latent with bf16):
  // the spatial position -- hence tap validity and the in-sample offset -- of each of this thread's rows is
  // loop invariant; only the sample index advances.  Offsets are 32-bit element offsets (host-checked).
  constexpr unsigned kBad = 0xffffffffu;
  unsigned x_fix[E16];
  const int S = g.S;
  if (p.rows_fixed && do_x) {
#pragma unroll
    for (int i = 0; i < E16; ++i) {
      x_fix[i] = kBad;
      if (x_col_ok) {
        const RowPos r = decode_row(g, mbk * E16 + i, p.a_sn);        // row inside the reduction block
        int id, ih, iw;
        if (tap_coords(g, r, x_tapcode, id, ih, iw))
          x_fix[i] = (unsigned)(r.nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw);
      }
    }
  }
  const bool vec_f32 = p.a_f32 && p.a_sc == 1 && ((p.a_coff + x_c) & 3) == 0 && x_c + E16 <= p.Kc_real &&
                       ((p.a_sn | p.a_sd | p.a_sh | p.a_sw) & 3) == 0;
  auto load_x = [&](long off) -> u32x4 {
    if (vec_f32) {      // contiguous fp32 channels: two (bf16) / one (f32) 16-byte loads, converted in registers
      const float* src = reinterpret_cast<const float*>(p.A) + off + p.a_coff + x_c;
      typename Chunk<T>::type v;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ET<T>::from_f32(lo[e]);
      if constexpr (E16 == 8) {
        const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 + e] = ET<T>::from_f32(hi[e]);
      }
      return *reinterpret_cast<u32x4*>(&v);
    }
    return load_a_chunk<T>(p.A, p.a_f32, off, p.a_sc, p.a_coff, x_c, p.Kc_real);
  };

  // Staging registers: NR reduction stages are in flight per thread (one wave per SIMD owns 512 VGPRs; a stage is
  // 32 of them).  With a single stage in flight every iteration paid a full HBM/L2 latency for ~0.25 us of MFMA work.
  // bf16: a thread stages dY *or* A (8 chunks); f32: 4 chunks of dY then 4 of A.
  constexpr int XO = E16 == 8 ? 0 : 4;          // where the A chunks start inside a register set
  u32x4 rs[NR][8];
  auto load_stage = [&](int mb, u32x4* rset) {
    u32x4* ry = rset;
    u32x4* rx = rset + XO;
    const int mbase = mb * RM + mbk * E16;
    if (do_y) {
      const T* yp = reinterpret_cast<const T*>(p.dY) + (long)mbase * p.ldy + p.y_coff + ncol;
#pragma unroll
      for (int i = 0; i < E16; ++i) {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (y_col_ok && mbase + i < g.M) v = *reinterpret_cast<const u32x4*>(yp + (long)i * p.ldy);
        ry[i] = v;
      }
    }
    if (do_x) {
      if (p.rows_fixed) {
        const long nb = (long)(mb * (RM / S)) * p.a_sn;
#pragma unroll
        for (int i = 0; i < E16; ++i) {
          u32x4 v = {0u, 0u, 0u, 0u};
          if (x_fix[i] != kBad && mbase + i < g.M) v = load_x(nb + x_fix[i]);
          rx[i] = v;
        }
      } else {
#pragma unroll
        for (int i = 0; i < E16; ++i) {
          const int m = mbase + i;
          u32x4 v = {0u, 0u, 0u, 0u};
          if (x_col_ok && m < g.M) {
            const RowPos r = decode_row(g, m, p.a_sn);
            int id, ih, iw;
            if (tap_coords(g, r, x_tapcode, id, ih, iw))
              v = load_x(r.nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw);
          }
          rx[i] = v;
        }
      }
    }
  };
  // transpose an ExE block held as E16 row-chunks and store its E16 columns as rows of the LDS tile
  auto store_block = [&](unsigned char* tile, const u32x4* r) {
    const int key = cb & 7;                                   // == ((row / E16) & 7) for row = cb*E16 + j
    const int chunk = (mbk ^ key) * 16;
    if constexpr (E16 == 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        u32x4 o;
        const unsigned sel = (j & 1) ? 0x07060302u : 0x05040100u;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = __builtin_amdgcn_perm(r[2 * d + 1][j >> 1], r[2 * d][j >> 1], sel);
        *reinterpret_cast<u32x4*>(tile + (cb * 8 + j) * kPitch + chunk) = o;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u32x4 o = {r[0][j], r[1][j], r[2][j], r[3][j]};
        *reinterpret_cast<u32x4*>(tile + (cb * 4 + j) * kPitch + chunk) = o;
      }
    }
  };
  auto store_stage = [&](int buf, const u32x4* rset) {
    if (do_y) store_block(sY + buf * 128 * kPitch, rset);
    if (do_x) store_block(sX + buf * 128 * kPitch, rset + XO);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nst = mb_end - mb_begin;
  if (nst > 0) {
    // register set k holds stages == k (mod NR); LDS buffer = stage parity
#pragma unroll
    for (int k = 0; k < NR; ++k) if (k < nst) load_stage(mb_begin + k, rs[k]);
    store_stage(0, rs[0]);
    if (NR < nst) load_stage(mb_begin + NR, rs[0]);
    __syncthreads();
    for (int base = 0; base < nst; base += NR) {
#pragma unroll
      for (int u = 0; u < NR; ++u) {
        const int i = base + u;
        if (i < nst) {
          constexpr int kDummy = 0; (void)kDummy;
          const int buf = u & 1;
          const int yrow = wm * 64 + (lane & 15), xrow = wn * 64 + (lane & 15);
          const unsigned char* y_base = sY + buf * 128 * kPitch;
          const unsigned char* x_base = sX + buf * 128 * kPitch;
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const int q = s2 * 4 + (lane >> 4);
            frag_t fy[4], fx[4];
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
              const int row = yrow + ii * 16;
              fy[ii] = *reinterpret_cast<const frag_t*>(y_base + row * kPitch + ((q ^ ((row >> LOGE) & 7)) * 16));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int row = xrow + j * 16;
              fx[j] = *reinterpret_cast<const frag_t*>(x_base + row * kPitch + ((q ^ ((row >> LOGE) & 7)) * 16));
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
              for (int j = 0; j < 4; ++j) mma64(fy[ii], fx[j], acc[ii][j]);
          }
          if (i + 1 < nst) {
            store_stage(buf ^ 1, rs[(u + 1) % NR]);
            if (i + 1 + NR < nst) load_stage(mb_begin + i + 1 + NR, rs[(u + 1) % NR]);
          }
          __syncthreads();
        }
      }
    }
  }

  // epilogue: acc[i][j][r] = dW[n = n0 + wm*64 + 16i + (lane&15)][k = k0 + wn*64 + 16j + 4*(lane>>4) + r]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wm * 64 + i * 16 + (lane & 15);
    if (n >= p.Nout) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + wn * 64 + j * 16 + (lane >> 4) * 4;
      if (k >= p.Ktot) continue;
      const int tap = FDiv(p.Kc).div(k), c = k - tap * p.Kc;     // 4 consecutive k share the tap (Kc % 4 == 0)
      float* base = p.dW + (long)n * p.w_sn + (long)tap * p.w_st + (p.split_stride > 0 ? (long)z * p.split_stride : 0L);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (c + r < p.Kc_store) {
          float* q = base + (long)(c + r) * p.w_sc;
          if (p.splitm > 1 && p.split_stride == 0) atomicAdd(q, acc[i][j][r]);
          else *q = p.accumulate ? *q + acc[i][j][r] : acc[i][j][r];
        }
      }
    }
  }
}

// =============================================================================================
// host side
static int make_geom(GeomDev& g, int NB, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int kd, int kh, int kw,
                     int sd, int sh, int sw, int pd, int ph, int pw, int transposed) {
  g.lDo = ilog2_exact(Do); g.lHo = ilog2_exact(Ho); g.lWo = ilog2_exact(Wo);
  IPK_REQUIRE(Do >= 1 && Ho >= 1 && Wo >= 1 && (long)NB * Do * Ho * Wo < (1L << 31), "bad output extents");
  g.Do = Do; g.Ho = Ho; g.Wo = Wo; g.S = Do * Ho * Wo;
  g.pow2 = (g.lDo >= 0 && g.lHo >= 0 && g.lWo >= 0) ? 1 : 0;      // rows decode by shifts, else by division
  g.lsd = ilog2_exact(sd); g.lsh = ilog2_exact(sh); g.lsw = ilog2_exact(sw);
  IPK_REQUIRE(g.lsd >= 0 && g.lsh >= 0 && g.lsw >= 0, "strides must be powers of two");
  IPK_REQUIRE(kd >= 1 && kh >= 1 && kw >= 1 && kd * kh * kw <= 256, "unsupported kernel extent");
  g.M = NB * Do * Ho * Wo;
  g.Di = Di; g.Hi = Hi; g.Wi = Wi;
  g.khw = kh * kw; g.kw = kw; g.taps = kd * kh * kw;
  g.sd = sd; g.sh = sh; g.sw = sw; g.pd = pd; g.ph = ph; g.pw = pw;
  g.transposed = transposed;
  return IPOKE_OK;
}

// set_lds / device_max_lds: common.h (shared with gru.hip)
constexpr size_t kLdsC64 = 9 * 64 * 128 + 2 * 41 * 1024 + 1024, kLdsHalo16 = 2 * 41 * 1024 + 4 * 128 * 128 + 8 * 1024,
                 kLdsHalo = 2 * 24 * 1024 + 12 * 64 * 128 + 8 * 1024, kLdsS8 = 2 * 128 * 128 + 256 + 12 * 64 * 128 + 512 * 16,
                 kLdsLat8 = 3 * 2 * 128 * 128 + 256, kLdsK64 = 128 * 128 + 256 + 6 * 128 * 128;

// Scratch of the deterministic split-K accumulation (ipoke_conv_desc.acc_scratch): 4096 tile counters, then the slabs.
static constexpr long kAccCounterBytes = 4096 * 4;
extern "C" int64_t ipoke_conv_acc_scratch_bytes(int M, int Nout, int splitk) {
  if (M < 1 || Nout < 1 || splitk < 1) return -1;
  // upper bound over every tile shape the dispatcher may choose: rows padded to a 160-row tile, columns to a 128-column one
  return kAccCounterBytes + (int64_t)splitk * ((int64_t)M + 160) * round_up(Nout, 128) * 4;
}
extern "C" int ipoke_conv_acc_scratch_init(void* scratch, void* stream) {
  IPK_REQUIRE(scratch != nullptr, "null scratch");
  IPK_HIP(hipMemsetAsync(scratch, 0, (size_t)kAccCounterBytes, reinterpret_cast<hipStream_t>(stream)));
  return IPOKE_OK;
}
// the launchers call this once the tile shape is known
static int acc_scratch_fits(const NtParams& p, int BM, int BN, bool det_capable) {
  if (!(p.splitk > 1 && p.c_acc && p.acc_part)) return IPOKE_OK;
  IPK_REQUIRE(det_capable, "deterministic accumulation is built into the skinny tiles only (Nout <= 64, default dispatch)");
  const long tiles = (long)p.tiles_m * p.tiles_n;
  IPK_REQUIRE(tiles <= 4096 && tiles * p.splitk * BM * BN * 4 <= p.acc_part_bytes && (long)p.splitk * BM * BN * 4 < (1L << 31),
              "accumulation scratch too small for this launch (ipoke_conv_acc_scratch_bytes)");
  return IPOKE_OK;
}

// XCD-aware tile -> block mapping: XCD x (= blockIdx % 8) owns a (tiles_m/xa) x (tiles_n/xb) sub-grid so
// that its private L2 holds one slab of A rows and one slab of W rows; (xa, xb) minimises L2 fill bytes.
static void pick_xcd_map(NtParams& p) {
  p.xa = 0; p.xb = 0;
  const long nt = (long)p.tiles_m * p.tiles_n;
  if (nt % 8 == 0) {
    double best = -1;
    const double bytesA = (double)p.g.M * p.Ktot, bytesW = (double)p.Nout * p.Ktot;
    for (int xa = 1; xa <= 8; xa *= 2) {
      const int xb = 8 / xa;
      if (p.tiles_m % xa || p.tiles_n % xb) continue;
      const double cost = bytesA / xa + bytesW / xb;
      if (best < 0 || cost < best) { best = cost; p.xa = xa; p.xb = xb; }
    }
  }
}

// =============================================================================================
// 3x3 convolution (stride 1, pad 1) on 8x8 maps with a wide dense input and a skinny output: conv3 of every coupling net
// (2048 -> 2*cout <= 64 channels, split-K partials) and the data gradient of conv1 (2048 -> cin channels, accumulated
// into the gradient state).  As an implicit GEMM the K = 9 * 2048 reduction re-reads every input row nine times (once
// per tap) and every 64-row tile re-reads the whole filter: 92 MB of L2 -> LDS traffic per launch at B = 20 for 5 MB of
// input and 2.4 MB of filter.  Here the reduction runs chunk-major (64 input channels at a time, the 9 taps inside): a
// tile of two whole samples keeps the chunk's [128 rows x 64 channels] image in LDS ONCE and the nine taps read it
// through shifted row addresses -- a lane whose tap falls outside the 8x8 map reads a zero row instead -- so only the
// filter streams (29 MB per launch).
// The math side of these kernels is bound by LDS fragment reads, not by the matrix cores (measured with the DMA
// instructions compiled out: a 4 x 2 arrangement of 32 x 32 wave tiles needs 96 KB of ds_read_b128 per K-block and runs
// at 350 ns per K-block, ~130 B/clk of LDS reads, against 110 ns of MFMA time).  So the 8 waves are arranged as
// 2 (row halves) x 4 (K groups): a wave owns a 64 x 64 tile -- 16 fragment reads per 32 MFMAs, 32 KB per K-block -- of
// every fourth K-block (tap), four K-blocks are consumed per barrier, and the four groups' accumulators meet in LDS
// (two hand-over rounds) before the epilogue.
// Split-K is over channel chunks (blockIdx.y); the epilogue is nt_epilogue (partials / atomics / dense outputs).
//
// igemm_nn_pair_kernel (further down) carries a COPY of this body's K-block loop and of the four K groups' hand-over, with the input
// image taken from LDS: the two must keep the same K-block order (chunk-major, nine taps inside, group kq takes every fourth block) and
// the same hand-over sums -- tests/test_pair_dgrad_gpu.py compares them bit for bit and fails when they diverge.
//
// NSPLIT > 0 (conv3x3_s8_coupling_kernel): the K splits of a row tile meet INSIDE the launch and the coupling transform the
// convolution feeds (affine_fwd / affine_actnorm_fwd / affine_inv of elementwise.hip) runs in the same launch -- CouplingTail below,
// which igemm_nt_coupling_kernel (further down: conv2's GEMM in front of a COPY of this body's K-block loop, the input image taken
// from LDS) shares.  That copy must keep the K-block order and the four-group sum of this body: tests/test_pair_coupling_gpu.py
// compares the two bit for bit.
struct CouplingEpi {
  const float* bias; const float* in; float* out; float* out2; float* scale_out; float* logdet_slot;
  const float* an_ls; const float* an_bias; const int* an_idx; void* ext; void* xchg;
  int xchg_bytes, slot_stride, Cp, t_off, t_stride, ld, mode, an_c0, an_C, ext_ld, ext_bf16;
  int ld_sh, cp_sh, ts_sh;      // log2 of ld / Cp / t_stride when a power of two, else -1
};
static constexpr int kCplHeader = 256;                 // bytes: word 0 counts spin time-outs
static constexpr unsigned kCplEmpty = 0xffffffffu;     // a dword of the exchange scratch nobody has written yet (a NaN no sum produces)
static constexpr unsigned kCplSpinMax = 1u << 21;

// The coupling side of a fused launch: what conv3x3_s8_coupling_kernel and igemm_nt_coupling_kernel do around and behind the K loop of the
// skinny convolution.  ONE piece of code for both (tests/test_pair_coupling_gpu.py compares the two launches bit for bit): prefetch()
// ahead of the K loop, pin() behind the loop's last wait for vector memory, run() with the accumulators of the four K groups of the
// [128 rows x 64 columns] tile.
template <int NSPLIT>
struct CouplingTail {
  static constexpr int BM = 128, NTHR = 512, MREP = 4, NREP = 4, EP = 16 * NREP * 4 + 16;
  static constexpr int NOWN = NSPLIT == 0 ? 1 : (NSPLIT < 8 ? NSPLIT : 8), RPO = BM / NOWN;   // owners per tile, rows per owner (16 or 32)
  static constexpr int SLOT = RPO * 256;                                                      // one sender's rows for one owner, bytes
  static constexpr int NSL = RPO / 16;                                                        // 16-row slices per owner (1 or 2)
  // one slice per owner (NSPLIT >= 8): both halves of the workgroup share its elements (element u of thread t256 of the 256-thread
  // affine kernels goes to half u); two slices (NSPLIT = 4): a half per slice, two elements per thread
  static constexpr int NU = NSL == 1 ? 1 : 2;                 // transformed elements per thread (Cp <= 32)
  static constexpr int NC = NSL == 1 ? 2 : 4;                 // copied (untouched) elements per thread (ld <= 64)
  const CouplingEpi& e;
  bool owner, valid, with_an, col_fixed; int hf, t256, u0, ld, Cp, an_src; long row0; float an_e, an_b;
  float pre_c[NC], pre_t[NU]; f32x4 pre_bias;
  __device__ __forceinline__ explicit CouplingTail(const CouplingEpi& e_) : e(e_) {}
  __device__ __forceinline__ void div_ld(int i, int& q, int& r) const { if (e.ld_sh >= 0) { q = i >> e.ld_sh; r = i & (ld - 1); } else { q = i / ld; r = i - q * ld; } }
  __device__ __forceinline__ void div_cp(int i, int& q, int& r) const { if (e.cp_sh >= 0) { q = i >> e.cp_sh; r = i & (Cp - 1); } else { q = i / Cp; r = i - q * Cp; } }
  __device__ __forceinline__ bool is_transformed(int col) const {
    const int rel = col - e.t_off;
    if (e.ts_sh >= 0) return rel >= 0 && (rel & (e.t_stride - 1)) == 0 && (rel >> e.ts_sh) < Cp;
    return rel >= 0 && rel % e.t_stride == 0 && rel / e.t_stride < Cp;
  }
  // fused launch: what the coupling at the end needs besides the convolution's sums is requested NOW, ahead of the K loop -- the
  // slice's state rows, the bias and the ActNorm parameters of this thread's column (otherwise three dependent round trips behind
  // the hand-off).  Index arithmetic: shifts when ld / Cp / t_stride are powers of two (the integer-division sequences of the
  // general path cost the affine kernels ~1 us per launch).
  __device__ __forceinline__ void prefetch(const int M, const int m0, const int z) {
    const int tid = threadIdx.x;
    owner = NSPLIT > 0 && z < NOWN;
    hf = tid >> 8; t256 = tid & 255;
    u0 = NSL == 1 ? hf : 0;                              // first element index (of the 256-thread numbering) this thread handles
    row0 = (long)m0 + z * RPO + (NSL == 1 ? 0 : hf * 16);                           // first state row of this thread's slice
    valid = owner && row0 < M;
    with_an = e.mode == 1;
    ld = e.ld; Cp = e.Cp;
    pre_bias = f32x4{0.f, 0.f, 0.f, 0.f};
    col_fixed = false; an_src = 0; an_e = 1.f; an_b = 0.f;
#pragma unroll
    for (int u = 0; u < NC; ++u) pre_c[u] = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u) pre_t[u] = 0.f;
    if (valid) {
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        const int i = t256 + (NC * u0 + u) * 256;
        int pp, col; div_ld(i, pp, col);
        if (i < 16 * ld && !is_transformed(col)) pre_c[u] = e.in[row0 * ld + i];
      }
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int el = t256 + (u0 + u) * 256;
        int pp, i; div_cp(el, pp, i);
        if (el < 16 * Cp) pre_t[u] = e.in[(row0 + pp) * ld + e.t_off + (long)i * e.t_stride];
      }
      col_fixed = with_an && e.ld_sh >= 0 && ld <= 256;           // 256 % ld == 0: a thread keeps its column over the rows it writes
      if (col_fixed) {
        const int j = (t256 & (ld - 1)) - e.an_c0;
        if (j >= 0 && j < e.an_C) {
          an_src = e.an_idx ? e.an_idx[j] : j;
          if (e.an_ls) { an_e = expf(e.an_ls[an_src]); an_b = e.an_bias[an_src]; }
        }
      }
    }
    if (owner && e.bias && tid < RPO * 16) {
      const int j = (tid & 15) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) if (j + q < 2 * Cp) pre_bias[q] = e.bias[j + q];
    }
  }
  // the values requested ahead of the K loop have landed: pin that (behind a wait for vmcnt(0)), so that no use further down waits on
  // the vector-memory counter (which by then also counts the hand-off's write-through stores)
  __device__ __forceinline__ void pin() {
#pragma unroll
    for (int u = 0; u < NC; ++u) asm volatile("" : "+v"(pre_c[u]));
#pragma unroll
    for (int u = 0; u < NU; ++u) asm volatile("" : "+v"(pre_t[u]));
    asm volatile("" : "+v"(pre_bias));
    asm volatile("" : "+v"(an_src), "+v"(an_e), "+v"(an_b));
  }
  template <typename P>
  __device__ __forceinline__ void run(const P& p, unsigned char* smem, const int tile, const int z, const int mh, const int kq,
                                      f32x4 (&acc)[MREP][NREP]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- the K splits of this row tile meet inside the launch (reduce-scatter), then the rows' owners apply the coupling ----
    // Before: 16 partial tiles -> 5 MB of fp32 slabs -> kernel boundary -> affine_* re-reads and sums them (14 us + boundary +
    // 9 us per coupling, 215 couplings per pass).  Here the 128 rows of a tile are dealt in 16-row slices (= one block of the
    // affine kernels: a quarter of a sample, log-det slot q) to NOWN = min(NSPLIT, 8) of the tile's NSPLIT workgroups; every
    // workgroup sums its four K groups in LDS and sends each 16-byte chunk of a foreign row straight to that row's owner:
    // relaxed agent-scope (sc1, write-through) stores into the owner's slot [sender][row][64 floats], no fence, no flag.  The
    // data is the flag (form R2 of cdna_hip_programming.md Guideline 16, as in mcf_unit_split.hip): every DWORD of the scratch
    // holds kCplEmpty until its value arrives; the owner sweeps its slots with sc1 loads until no dword is empty, puts
    // kCplEmpty back (the scratch is in its initial state again when the launch ends: no memset node, replays from a hipGraph)
    // and sums the NSPLIT partial rows in exactly the order of affine_stage_raw (a pairwise tree over the split index).
    // Partners are adjacent in dispatch order (z is the fast index of the 1-D grid), groups complete in order: a partly
    // resident grid finishes group by group.  Spins are bounded; a time-out is counted in word 0 of the scratch.
    typedef __amdgpu_buffer_rsrc_t rsrc_t;
    const rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(e.xchg, 0, e.xchg_bytes, 0x00020000);
    // Barriers of this tail order LDS traffic only (s_waitcnt lgkmcnt(0) + s_barrier): __syncthreads() would also wait for the
    // write-through stores of the hand-off to be acknowledged by the memory side (~1 us each time).
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    lds_barrier();                   // the ring and the input buffers are dead
    {
      unsigned char* st = smem + kq * BM * EP + (mh * MREP * 16 + (lane & 15)) * EP + (lane >> 4) * 16;
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(st + i * 16 * EP + j * 64) = acc[i][j];
    }
    lds_barrier();
    f32x4 mine = f32x4{0.f, 0.f, 0.f, 0.f}; int mine_off = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = tid + NTHR * k, row = c >> 4, cq = c & 15;
      const unsigned char* s0 = smem + row * EP + cq * 16;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(s0), v1 = *reinterpret_cast<const f32x4*>(s0 + BM * EP),
                  v2 = *reinterpret_cast<const f32x4*>(s0 + 2 * BM * EP), v3 = *reinterpret_cast<const f32x4*>(s0 + 3 * BM * EP);
      const f32x4 v = (v0 + v2) + (v1 + v3);              // the order of the hand-over rounds of the unfused kernel
      const int o = row / RPO, r = row - o * RPO;
      if (o == z) { mine = v; mine_off = r * 256 + cq * 16; }
      else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_x,
                                                  kCplHeader + (((tile * NOWN + o) * NSPLIT + z) * RPO + r) * 256 + cq * 16, 0, 16);
    }
    if (!owner) return;              // (uniform) this workgroup owns no rows
    // LDS from here on: own [RPO][64] | bsum [4][RPO][64] | raw_s [RPO][64] | an_tile [NSL][16][ld] | red [8]
    float* own = reinterpret_cast<float*>(smem);
    float* bsum = own + RPO * 64;
    float* raw_s = bsum + 4 * RPO * 64;
    float* an_tile = raw_s + RPO * 64;
    float* red = an_tile + NSL * 16 * e.ld;
    constexpr int NCH = RPO * 16 / 128, NP = NSPLIT / 4;
    const int gq = tid >> 7, tl = tid & 127;
    u32x4 rv[NCH][NP]; int ro[NCH][NP];
    {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int m = 0; m < NP; ++m) {
          const int snd = gq + 4 * m;
          ro[ch][m] = snd == z ? -1 : kCplHeader + ((tile * NOWN + z) * NSPLIT + snd) * SLOT + (tl + 128 * ch) * 16;
          // (no branch around the load: every request goes out back to back; this workgroup's own slot reads the header)
          rv[ch][m] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ro[ch][m] >= 0 ? ro[ch][m] : 0, 0, 16);
        }
      lds_barrier();                 // every read of the parked tiles is done
      if (mine_off >= 0) *reinterpret_cast<f32x4*>(reinterpret_cast<unsigned char*>(own) + mine_off) = mine;
      unsigned spins = 0;
      for (;;) {
        bool ok = true;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
          for (int m = 0; m < NP; ++m)
            ok = ok && (ro[ch][m] < 0 || (rv[ch][m][0] != kCplEmpty && rv[ch][m][1] != kCplEmpty && rv[ch][m][2] != kCplEmpty && rv[ch][m][3] != kCplEmpty));
        if (ok) break;
        if (++spins >= kCplSpinMax) { atomicAdd(reinterpret_cast<unsigned*>(e.xchg), 1u); break; }
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
          for (int m = 0; m < NP; ++m)
            if (ro[ch][m] >= 0 && (rv[ch][m][0] == kCplEmpty || rv[ch][m][1] == kCplEmpty || rv[ch][m][2] == kCplEmpty || rv[ch][m][3] == kCplEmpty))
              rv[ch][m] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ro[ch][m], 0, 16);
      }
      lds_barrier();                 // own rows are in LDS
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        // affine_stage_raw's tree over 32 split slots (absent splits are zeros): v[u] += v[u + w] for w = 16, 8, 4, 2, 1
        f32x4 v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          v[m] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (m < NP) v[m] = (gq + 4 * m) == z ? *reinterpret_cast<const f32x4*>(own + (tl + 128 * ch) * 4) : __builtin_bit_cast(f32x4, rv[ch][m < NP ? m : 0]);
        }
        const f32x4 a0 = v[0] + v[4], a1 = v[1] + v[5], a2 = v[2] + v[6], a3 = v[3] + v[7];
        const f32x4 b = (a0 + a2) + (a1 + a3);
        *reinterpret_cast<f32x4*>(bsum + gq * RPO * 64 + (tl + 128 * ch) * 4) = b;
      }
      lds_barrier();
      if (tid < RPO * 16) {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bsum + tid * 4), b1 = *reinterpret_cast<const f32x4*>(bsum + RPO * 64 + tid * 4),
                    b2 = *reinterpret_cast<const f32x4*>(bsum + 2 * RPO * 64 + tid * 4), b3 = *reinterpret_cast<const f32x4*>(bsum + 3 * RPO * 64 + tid * 4);
        f32x4 t = (b0 + b2) + (b1 + b3);
        if (e.bias) {
          const int j = (tid & 15) * 4;
#pragma unroll
          for (int q = 0; q < 4; ++q) if (j + q < 2 * e.Cp) t[q] += pre_bias[q];
        }
        *reinterpret_cast<f32x4*>(raw_s + tid * 4) = t;
      }
      lds_barrier();
    }
    // the scratch goes back to its initial state (nothing waits for these stores; they drain under the coupling's arithmetic)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int m = 0; m < NP; ++m)
        if (ro[ch][m] >= 0)
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{kCplEmpty, kCplEmpty, kCplEmpty, kCplEmpty}, rs_x, ro[ch][m], 0, 16);
    // the coupling on this owner's slices: the bodies of affine_fwd_kernel / affine_actnorm_fwd_kernel / affine_inv_kernel
    // (elementwise.hip) -- same element -> (row, channel) map and the same order of every sum as their 256-thread blocks:
    // bit-identical outputs.  The inputs (pre_c / pre_t) and the ActNorm parameters of this thread's column were requested
    // before the K loop.
    {
      const int sl = NSL == 1 ? 0 : hf;                        // this thread's slice
      const float* rs = raw_s + sl * 16 * 64;
      float* tl_an = an_tile + sl * 16 * ld;
      float* lx = red + 8;                                     // [256]: the second element's log-scale (one slice per owner)
      if (valid) {      // untouched channels
        const int total = 16 * ld;
#pragma unroll
        for (int u = 0; u < NC; ++u) {
          const int i = t256 + (NC * u0 + u) * 256;
          int pp, col; div_ld(i, pp, col);
          if (i < total && !is_transformed(col)) {
            if (with_an) tl_an[i] = pre_c[u];
            if (e.out) e.out[row0 * ld + i] = pre_c[u];
          }
        }
        for (int i = t256 + 4 * 256 + u0 * 256; i < total; i += 256 * (NSL == 1 ? 2 : 1)) {          // (states wider than 64 columns)
          int pp, col; div_ld(i, pp, col);
          if (!is_transformed(col)) {
            const float v = e.in[row0 * ld + i];
            if (with_an) tl_an[i] = v;
            if (e.out) e.out[row0 * ld + i] = v;
          }
        }
      }
      float ld_acc = 0.f;
      if (valid) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const int el = t256 + (u0 + u) * 256;
          if (el < 16 * Cp) {
            int pp, i; div_cp(el, pp, i);
            const float mu = rs[pp * 64 + i];
            const float sc = tanhf(0.5f * rs[pp * 64 + Cp + i]) + 1.f;
            const int col = e.t_off + i * e.t_stride;
            const long off = (row0 + pp) * ld + col;
            float y;
            if (e.mode == 2) y = (pre_t[u] - mu) / (sc + 1e-12f);      // macow_utils.py:64
            else y = sc * pre_t[u] + mu;
            if (with_an) tl_an[pp * ld + col] = y;
            if (e.out) e.out[off] = y;
            if (e.ext) {
              if (e.ext_bf16) reinterpret_cast<bf16_t*>(e.ext)[(row0 + pp) * e.ext_ld + i] = ET<bf16_t>::from_f32(y);
              else reinterpret_cast<float*>(e.ext)[(row0 + pp) * e.ext_ld + i] = y;
            }
            if (e.scale_out) e.scale_out[(row0 + pp) * Cp + i] = sc;
            ld_acc += logf(sc);
          }
        }
        if (e.ext && e.ext_ld > Cp) {
          const int pad = e.ext_ld - Cp;
          for (int el = NSL == 1 ? tid : t256; el < 16 * pad; el += NSL == 1 ? 512 : 256) {
            const int pp = el / pad, i = Cp + (el - pp * pad);
            if (e.ext_bf16) reinterpret_cast<bf16_t*>(e.ext)[(row0 + pp) * e.ext_ld + i] = ET<bf16_t>::from_f32(0.f);
            else reinterpret_cast<float*>(e.ext)[(row0 + pp) * e.ext_ld + i] = 0.f;
          }
        }
      }
      if (e.mode != 2) {             // per-slice log-det: block_sum of a 256-thread block
        if constexpr (NSL == 1) {    // thread t256 of the block summed its first, then its second element
          if (hf == 1) lx[t256] = ld_acc;
          lds_barrier();
          if (hf == 0) ld_acc += lx[t256];
        }
        const float ws = wave_sum(ld_acc);
        if (lane == 0) red[wave] = ws;           // (red is written here only)
        lds_barrier();
        float tot = 0.f;
        for (int i = 0; i < 4; ++i) tot += red[sl * 4 + i];
        if (valid && t256 == 0 && (NSL > 1 || hf == 0) && e.logdet_slot)
          e.logdet_slot[(long)(row0 >> 6) * e.slot_stride + ((int)(row0 >> 4) & 3)] = tot;
      }
      if (with_an && valid) {        // ActNorm (+ shuffle) of the slice's rows: out2
        for (int el = NSL == 1 ? tid : t256; el < 16 * ld; el += NSL == 1 ? 512 : 256) {
          int pp, col; div_ld(el, pp, col);
          const int j = col - e.an_c0;
          float v;
          if (j >= 0 && j < e.an_C) {
            if (col_fixed) {
              v = tl_an[pp * ld + e.an_c0 + an_src];
              if (e.an_ls) v = v * an_e + an_b;
            } else {
              const int src = e.an_idx ? e.an_idx[j] : j;
              v = tl_an[pp * ld + e.an_c0 + src];
              if (e.an_ls) v = v * expf(e.an_ls[src]) + e.an_bias[src];
            }
          } else {
            v = tl_an[el];
          }
          e.out2[(row0 + pp) * ld + col] = v;
        }
      }
    }
  }
};

// NREP = 2: 32 output columns (the conv1 data gradient of a coupling that conditions on <= 32 channels): half the filter ring --
// 88 KB of LDS instead of 137, which fits beside ONE resident weight-gradient workgroup instead of waiting for a whole CU -- and
// half the matrix-core work.
template <int NSPLIT, int NREP = 4>
__device__ __forceinline__ void conv3x3_s8_body(const NtParams& p, const CouplingEpi& e, const int tile, const int z) {
  typedef bf16_t T;
  typedef typename ET<T>::frag frag_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int BM = 128, BN = 16 * NREP, NTHR = 512, R = 12;     // ring: three rounds of four filter K-blocks
  constexpr int ABUF = BM * 128, WSLOT = BN * 128;
  constexpr int A_IT = BM * 8 / NTHR;                      // DMA instructions per thread and input chunk (2)
  constexpr int MREP = 4;
  constexpr int WJ = BN / 16;                              // filter DMA instructions per wave and round (8 rows each)
  constexpr int EP = BN * 4 + 16;                          // nt_epilogue's staging pitch
  constexpr unsigned kInvalid = 0xffffffffu;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* abuf = smem;                              // 2 x ABUF: the input chunk, double-buffered
  unsigned char* zrow = smem + 2 * ABUF;                   // 256 bytes of zeros: the "outside the map" row
  unsigned char* ring = zrow + 256;                        // R filter K-blocks
  unsigned char* dummy = ring + R * WSLOT;                 // landing zone of padding DMAs, 1 KB per wave
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mh = wave & 1, kq = wave >> 1;
  const GeomDev& g = p.g;
  const int m0 = tile * BM;
  const int nchunks = p.Kc >> 6;
  const int c_begin = z * p.kb_per_split, c_end = min(nchunks, c_begin + p.kb_per_split);
  const int nch = max(0, c_end - c_begin), nkb = nch * 9, nrounds = (nkb + 3) >> 2;
  const int sgn = g.transposed ? -1 : 1;

  if (tid < 16) reinterpret_cast<f32x4*>(zrow)[tid] = f32x4{0.f, 0.f, 0.f, 0.f};

  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  unsigned a_src[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int ch = (wave + 8 * i) * 64 + lane, row = ch >> 3, pos = ch & 7, m = m0 + row;
    a_src[i] = kInvalid;
    if (m < g.M) {
      const long off = (long)(m >> 6) * p.a_sn + (long)((m >> 3) & 7) * p.a_sh + (long)(m & 7) * p.a_sw + p.a_coff;
      a_src[i] = (unsigned)(off + c_begin * 64 + ((pos ^ ((row >> 1) & 7)) * 8));
    }
  }
  // filter DMA of a round: wave w brings rows 32*(w >> 2) .. +31 (4 instructions of 8 rows) of K-block 4r + (w & 3)
  unsigned w_src[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    const int n = 8 * WJ * (wave >> 2) + 8 * j + (lane >> 3), pos = lane & 7;
    w_src[j] = n < p.Nout ? (unsigned)((long)n * p.ldw + c_begin * 64 + ((pos ^ ((n >> 1) & 7)) * 8)) : kInvalid;
  }
  int wi_g = wave & 3, wi_c = 0, wi_t = wave & 3;          // K-block index / (chunk, tap) of this wave's next filter request
  auto issue_w = [&]() {
    const bool in = wi_g < nkb;
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      const bool real = in && w_src[j] != kInvalid;
      const T* src = real ? Wbase + w_src[j] + (long)wi_t * p.Kc + wi_c * 64 : zero;
      unsigned char* dst = in ? ring + (wi_g % R) * WSLOT + (WJ * (wave >> 2) + j) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    wi_g += 4; wi_t += 4;
    if (wi_t >= 9) { wi_t -= 9; ++wi_c; }
  };
  int a_next = 0;                                          // next input chunk to request
  auto issue_a = [&]() {
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const bool real = a_next < nch && a_src[i] != kInvalid;
      const T* src = real ? Abase + a_src[i] + a_next * 64 : zero;
      unsigned char* dst = a_next < nch ? abuf + (a_next & 1) * ABUF + (wave + 8 * i) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    ++a_next;
  };
  CouplingTail<NSPLIT> ct(e);      // (NSPLIT == 0: unused)
  if constexpr (NSPLIT > 0) { static_assert(NREP == 4, "the coupling's raw sums are 64 columns wide"); ct.prefetch(g.M, m0, z); }
  issue_a();                 // chunk 0
  issue_w(); issue_w();      // rounds 0 and 1

  // fragment bookkeeping: row r of the tile is position (y, x) = ((r >> 3) & 7, r & 7) of sample r >> 6
  unsigned vmask[MREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i) {
    const int r = i * 16 + (lane & 15);                    // row inside this wave's sample (mh)
    const int y = (r >> 3) & 7, x = r & 7;
    unsigned vm = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = y + sgn * (t / 3 - 1), xx = x + sgn * (t % 3 - 1);
      if ((unsigned)yy < 8u && (unsigned)xx < 8u) vm |= 1u << t;
    }
    vmask[i] = vm;
  }
  const int qlo = lane >> 4;
  int b_rd[NREP];                                          // half-step 0; half-step 1 is the chunk position ^ 4, i.e. byte offset ^ 64
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int n = j * 16 + (lane & 15);
    b_rd[j] = n * 128 + ((qlo ^ ((n >> 1) & 7)) * 16);
  }
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int gk = kq, ci = 0, t = kq;                             // this wave's K-block of the round: index, chunk, tap
  for (int r = 0; r < nrounds; ++r) {
    wait_vmcnt<WJ>();                // everything but this wave's share of round r + 1 has landed (input chunks included)
    __builtin_amdgcn_s_barrier();
    // the first K-block of this round lies in chunk (4r)/9: request the chunk after it once (its buffer held chunk - 1,
    // whose last K-block was consumed before this barrier)
    if (a_next <= (4 * r) / 9 + 1) issue_a();          // (issued before the filter blocks: the wait above counts those only)
    issue_w();                       // round r + 2 into the slots of round r - 1
    if (gk < nkb) {
      const unsigned char* ab = abuf + (ci & 1) * ABUF + mh * 64 * 128;
      const unsigned char* wb = ring + (gk % R) * WSLOT;
      const int th = t / 3, tw = t - 3 * th;
      const int shift = sgn * ((th - 1) * 8 + (tw - 1));
      const unsigned char* arow[MREP]; int aswz[MREP];
#pragma unroll
      for (int i = 0; i < MREP; ++i) {
        const bool ok = (vmask[i] >> t) & 1u;
        const int sr = i * 16 + (lane & 15) + shift;       // row inside the sample
        arow[i] = ok ? ab + sr * 128 : zrow;
        aswz[i] = ok ? (sr >> 1) & 7 : 0;
      }
      frag_t fa[2][MREP], fb[2][NREP];
#pragma unroll
      for (int hs = 0; hs < 2; ++hs) {
#pragma unroll
        for (int i = 0; i < MREP; ++i) fa[hs][i] = *reinterpret_cast<const frag_t*>(arow[i] + (((hs * 4 + qlo) ^ aswz[i]) * 16));
#pragma unroll
        for (int j = 0; j < NREP; ++j) fb[hs][j] = *reinterpret_cast<const frag_t*>(wb + (b_rd[j] ^ (hs * 64)));
      }
#pragma unroll
      for (int hs = 0; hs < 2; ++hs)
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) mma64(fa[hs][i], fb[hs][j], acc[i][j]);
      // issue order: the eight fragments of the first half-step, then the second half-step's reads one per two MFMAs of the first.
      // (hipcc's own schedule reads just in time, four MFMAs per s_waitcnt lgkmcnt(0): eight exposed LDS latencies per K-block.)
      constexpr int NF = MREP + NREP, NM = MREP * NREP, PER = NM / NF;        // fragment reads / MFMAs per half-step
      __builtin_amdgcn_sched_group_barrier(0x100, NF, 0);
#pragma unroll
      for (int q = 0; q < NF; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM - NF * PER, 0);
    }
    gk += 4; t += 4;
    if (t >= 9) { t -= 9; ++ci; }
  }
  wait_vmcnt<0>();
  if constexpr (NSPLIT > 0) ct.pin();
  if constexpr (NSPLIT == 0) {
  // the four K groups meet: groups 2, 3 hand over to groups 0, 1, then group 1 to group 0 (nt_epilogue's staging layout)
  {
    unsigned char* st = smem + (mh * MREP * 16 + (lane & 15)) * EP + (lane >> 4) * 16;
    __syncthreads();                 // the ring and the input buffers are dead
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int give_lo = round == 0 ? 2 : 1, take_hi = round == 0 ? 2 : 1;      // givers: kq in [give_lo, 2*give_lo); takers: kq < take_hi
      if (kq >= give_lo && kq < 2 * give_lo) {
        unsigned char* d = st + (kq - give_lo) * BM * EP;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(d + i * 16 * EP + j * 64) = acc[i][j];
      }
      __syncthreads();
      if (kq < take_hi) {
        const unsigned char* d = st + kq * BM * EP;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) acc[i][j] += *reinterpret_cast<const f32x4*>(d + i * 16 * EP + j * 64);
      }
      if (round == 0) __syncthreads();
    }
  }
  nt_epilogue<T, 2, 1, MREP, NREP, NTHR, true>(p, acc, smem, m0, 0, mh, 0, z, kq == 0);
  } else {
    ct.run(p, smem, tile, z, mh, kq, acc);
  }
}

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_s8_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  CouplingEpi none{};
  conv3x3_s8_body<0>(p, none, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_s8n32_kernel(const NtParams p) {      // <= 32 output columns
  kernarg_prefetch<(int)sizeof(NtParams)>();
  CouplingEpi none{};
  conv3x3_s8_body<0, 2>(p, none, blockIdx.x, blockIdx.y);
}
template <int NSPLIT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_s8_coupling_kernel(const NtParams p, const CouplingEpi e) {
  kernarg_prefetch<(int)(sizeof(NtParams) + sizeof(CouplingEpi))>();
  conv3x3_s8_body<NSPLIT>(p, e, blockIdx.x / NSPLIT, blockIdx.x % NSPLIT);
}

// =============================================================================================
// 3x3 convolution (stride 1, pad 1) on the 8x8 latent with a NARROW dense input (<= 64 channels) and a wide output (round 6): conv1 of
// every coupling net (cin conditioning channels -> 2048 hidden, macow_utils.py:270) and, in the transposed form, the data gradient of
// conv3 (2 cout -> 2048).  The mirror image of conv3x3_s8: there the input is wide and the filter streams per (chunk, tap); here the
// WHOLE input of a tile of two samples is one [128 rows x 64 channels] image (16 KB, staged once: channels beyond Kc are zero chunks)
// and the reduction is nothing but the nine taps, read from that image through shifted row addresses (a lane outside the map reads a
// zero row) -- as an implicit GEMM every tap re-gathered its 80 input rows behind a fresh L2 -> LDS latency (nine K-blocks, 14 us per
// launch for 3 GFLOP).  A workgroup owns 128 rows x 128 output channels; the filter of a tap is a [128 x 64] block (16 KB) of the
// [Nout][9 * Kc] operand, the nine blocks stream through six slots in rounds of three; 8 waves = 2 row halves x 4 column groups of
// 64 x 32 wave tiles; the epilogue is nt_epilogue (bias, ELU, ELU' mask of the data-gradient form, dtype output).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_k64_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  typedef bf16_t T;
  typedef typename ET<T>::frag frag_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int BM = 128, BN = 128, NTHR = 512, R = 6, MREP = 4, NREP = 2;
  constexpr int ABUF = BM * 128, WSLOT = BN * 128;
  constexpr unsigned kInvalid = 0xffffffffu;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* abuf = smem;                              // the input image [128 rows][64 channels]
  unsigned char* zrow = smem + ABUF;                       // 256 bytes of zeros: the "outside the map" row
  unsigned char* ring = zrow + 256;                        // R filter blocks (one tap each)
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mh = wave & 1, nq = wave >> 1;
  const GeomDev& g = p.g;
  const FDiv ftm(p.tiles_m);
  const int tm = ftm.mod((int)blockIdx.x), tn = ftm.div((int)blockIdx.x);
  const int m0 = tm * BM, n0 = tn * BN;
  const int sgn = g.transposed ? -1 : 1;
  const int kchunks = p.Kc >> 3;                           // 16-byte chunks of real channels per row (1 .. 8)
  if (tid < 16) reinterpret_cast<f32x4*>(zrow)[tid] = f32x4{0.f, 0.f, 0.f, 0.f};

  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  // input image: instruction i of a thread fills rows 8 * (wave + 8 i) .. + 7 (lane / 8), chunk position lane % 8 <- source chunk ^ swz(row)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ch = (wave + 8 * i) * 64 + lane, row = ch >> 3, pos = ch & 7, m = m0 + row;
    const int sc = pos ^ ((row >> 1) & 7);
    const T* src = zero;
    if (m < g.M && sc < kchunks)
      src = Abase + (long)(m >> 6) * p.a_sn + (long)((m >> 3) & 7) * p.a_sh + (long)(m & 7) * p.a_sw + p.a_coff + sc * 8;
    __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(abuf + (wave + 8 * i) * 1024), 16, 0, 0);
  }
  // filter block of tap t: rows n0 .. n0 + 127 of W, 64 channels at column t * Kc; instruction j of a thread: rows 8 * (wave + 8 j) + lane / 8
  unsigned w_src[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 8 * (wave + 8 * j) + (lane >> 3), n = n0 + row, sc = (lane & 7) ^ ((row >> 1) & 7);
    w_src[j] = (n < p.Nout && sc < kchunks) ? (unsigned)((long)n * p.ldw + sc * 8) : kInvalid;
  }
  auto issue_w = [&](int t, int slot) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const T* src = (t < 9 && w_src[j] != kInvalid) ? Wbase + w_src[j] + (long)t * p.Kc : zero;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(ring + slot * WSLOT + (wave + 8 * j) * 1024), 16, 0, 0);
    }
  };
#pragma unroll
  for (int t = 0; t < R; ++t) issue_w(t, t);               // rounds 0 and 1 (taps 0 .. 5)

  // fragment bookkeeping: row r of this wave's sample (mh) is position (y, x) = (r >> 3, r & 7)
  unsigned vmask[MREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i) {
    const int r = i * 16 + (lane & 15);
    const int y = (r >> 3) & 7, x = r & 7;
    unsigned vm = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = y + sgn * (t / 3 - 1), xx = x + sgn * (t % 3 - 1);
      if ((unsigned)yy < 8u && (unsigned)xx < 8u) vm |= 1u << t;
    }
    vmask[i] = vm;
  }
  const int qlo = lane >> 4;
  int b_rd[NREP];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int n = nq * 32 + j * 16 + (lane & 15);
    b_rd[j] = n * 128 + ((qlo ^ ((n >> 1) & 7)) * 16);
  }
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool two_steps = p.Kc > 32;                        // channels 32 .. 63 exist

  auto tap_mma = [&](int t, int slot) {
    const unsigned char* ab = abuf + mh * 64 * 128;
    const unsigned char* wb = ring + slot * WSLOT;
    const int th = t / 3, tw = t - 3 * th;
    const int shift = sgn * ((th - 1) * 8 + (tw - 1));
    const unsigned char* arow[MREP]; int aswz[MREP];
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
      const bool ok = (vmask[i] >> t) & 1u;
      const int sr = i * 16 + (lane & 15) + shift;
      arow[i] = ok ? ab + sr * 128 : zrow;
      aswz[i] = ok ? (sr >> 1) & 7 : 0;
    }
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
      if (hs == 1 && !two_steps) break;
      frag_t fa[MREP], fb[NREP];
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[i] = *reinterpret_cast<const frag_t*>(arow[i] + (((hs * 4 + qlo) ^ aswz[i]) * 16));
#pragma unroll
      for (int j = 0; j < NREP; ++j) fb[j] = *reinterpret_cast<const frag_t*>(wb + (b_rd[j] ^ (hs * 64)));
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) mma64(fa[i], fb[j], acc[i][j]);
    }
  };

  // round 0 (taps 0-2, slots 0-2) | refill slots 0-2 with taps 6-8 | round 1 (taps 3-5, slots 3-5) | round 2 (taps 6-8, slots 0-2)
  wait_vmcnt<6>();                    // the input image and this wave's share of taps 0-2 (2 + 6 of 14 instructions may still fly: taps 3-5)
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int t = 0; t < 3; ++t) tap_mma(t, t);
  __builtin_amdgcn_s_barrier();       // everybody is done with slots 0-2
#pragma unroll
  for (int t = 6; t < 9; ++t) issue_w(t, t - 6);
  wait_vmcnt<6>();                    // taps 3-5 have landed (the 6 instructions just issued may fly)
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int t = 3; t < 6; ++t) tap_mma(t, t);
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int t = 6; t < 9; ++t) tap_mma(t, t - 6);
  nt_epilogue<T, 2, 4, MREP, NREP, NTHR>(p, acc, smem, m0, n0, mh, nq, 0);
}

// =============================================================================================
// 3x3 convolution (stride 1, pad 1, one depth slice) on maps of any size with >= 64 dense input channels: the 2-D convolutions
// of the SPADE decoder, the VGG feature stack and their data gradients.  As an implicit GEMM every tap re-fetches the input
// rows of its tile from L2 (nine passes of global_load_lds over the same pixels: at 128 x 128 x 64 channels the A stream is
// 600 MB per launch for 67 MB of input, and the launch runs at the L2 -> LDS rate, 6x off the HBM and the matrix-core time).
// Here a workgroup owns an 8 x 16 patch of output pixels of one image and stages the patch's INPUT with its one-pixel halo
// (10 x 18 pixels, zero outside the image) in LDS once per 64-channel chunk; the nine taps read it through shifted row
// addresses -- the same chunk-major reduction, filter ring, 2 x 4 wave arrangement and K-group hand-over as conv3x3_s8 above,
// minus the "outside the map" masks (the zero border is materialised by the staging DMA).  Output channels are tiled by 64
// over blockIdx.y.  transposed (data gradient): the taps are mirrored, the caller supplies the transposed filter operand.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_halo_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  typedef bf16_t T;
  typedef typename ET<T>::frag frag_t;
  typedef typename Pack4<T>::type pack_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int BM = 128, BN = 64, NTHR = 512, R = 12;
  constexpr int TH = 8, TW = 16, HW = TW + 2, HROWS = (TH + 2) * HW;       // 180 halo pixels
  constexpr int A_IT = 3;                                                   // 24 DMA slots of 8 pixel rows >= 180 rows
  constexpr int ABUF = 8 * A_IT * 1024, WSLOT = BN * 128;
  constexpr int MREP = 4, NREP = 4;
  constexpr int EP = BN * 4 + 16;
  constexpr unsigned kInvalid = 0xffffffffu;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* abuf = smem;                              // 2 x ABUF: the halo image of a chunk, double-buffered
  unsigned char* ring = smem + 2 * ABUF;                   // R filter K-blocks
  unsigned char* dummy = ring + R * WSLOT;                 // landing zone of padding DMAs, 1 KB per wave
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mh = wave & 1, kq = wave >> 1;
  const GeomDev& g = p.g;
  const int tiles_x = g.Wo / TW, tiles_y = g.Ho / TH;
  const int tile = blockIdx.x, tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, slice = tile / (tiles_x * tiles_y);
  const int img = slice / g.Do, dz = slice - img * g.Do;       // 3 x 3 x 3 (kdn = 3): the tile lies in depth slice dz of sample img
  const int y0 = ty * TH, x0 = tx * TW, n0 = blockIdx.y * BN;
  const int kdn = g.taps / 9;                                  // depth taps: "virtual chunks" v = chunk * kdn + kd, nine K-blocks each
  const int nch = (p.Kc >> 6) * kdn, nkb = nch * 9, nrounds = (nkb + 3) >> 2;
  const int sgn = g.transposed ? -1 : 1;

  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  unsigned a_src[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int row = (wave + 8 * i) * 8 + (lane >> 3), pos = lane & 7;
    const int py = row / HW, px = row - py * HW, y = y0 - 1 + py, x = x0 - 1 + px;
    a_src[i] = kInvalid;
    if (row < HROWS && (unsigned)y < (unsigned)g.Hi && (unsigned)x < (unsigned)g.Wi)
      a_src[i] = (unsigned)((long)img * p.a_sn + (long)y * p.a_sh + (long)x * p.a_sw + p.a_coff + ((pos ^ ((row >> 1) & 7)) * 8));
  }
  unsigned w_src[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nl = 32 * (wave >> 2) + 8 * j + (lane >> 3), n = n0 + nl, pos = lane & 7;
    w_src[j] = n < p.Nout ? (unsigned)((long)n * p.ldw + ((pos ^ ((nl >> 1) & 7)) * 8)) : kInvalid;
  }
  int wi_g = wave & 3, wi_c = 0, wi_t = wave & 3;
  auto issue_w = [&]() {
    const bool in = wi_g < nkb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool real = in && w_src[j] != kInvalid;
      const T* src = real ? Wbase + w_src[j] + (long)((wi_c % kdn) * 9 + wi_t) * p.Kc + (wi_c / kdn) * 64 : zero;
      unsigned char* dst = in ? ring + (wi_g % R) * WSLOT + (4 * (wave >> 2) + j) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    wi_g += 4; wi_t += 4;
    if (wi_t >= 9) { wi_t -= 9; ++wi_c; }
  };
  int a_next = 0;
  auto issue_a = [&]() {
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int dd = dz + (kdn == 3 ? sgn * (a_next % kdn - 1) : 0);                 // depth slice this virtual chunk reads
      const bool real = a_next < nch && a_src[i] != kInvalid && (unsigned)dd < (unsigned)g.Di;
      const T* src = real ? Abase + a_src[i] + (long)dd * p.a_sd + (a_next / kdn) * 64 : zero;
      unsigned char* dst = a_next < nch ? abuf + (a_next & 1) * ABUF + (wave + 8 * i) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    ++a_next;
  };
  issue_a();
  issue_w(); issue_w();

  const int qlo = lane >> 4;
  int b_rd[NREP];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int n = j * 16 + (lane & 15);
    b_rd[j] = n * 128 + ((qlo ^ ((n >> 1) & 7)) * 16);
  }
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int gk = kq, ci = 0, t = kq;
  for (int r = 0; r < nrounds; ++r) {
    wait_vmcnt<4>();
    __builtin_amdgcn_s_barrier();
    if (a_next <= (4 * r) / 9 + 1) issue_a();
    issue_w();
    if (gk < nkb) {
      const unsigned char* ab = abuf + (ci & 1) * ABUF;
      const unsigned char* wb = ring + (gk % R) * WSLOT;
      const int th = t / 3, tw = t - 3 * th;
      // halo row of output pixel (mh*4 + i, lane & 15) under this tap
      const int sr0 = (mh * 4 + 1 + sgn * (th - 1)) * HW + (lane & 15) + 1 + sgn * (tw - 1);
      frag_t fa[2][MREP], fb[2][NREP];
#pragma unroll
      for (int hs = 0; hs < 2; ++hs) {
#pragma unroll
        for (int i = 0; i < MREP; ++i) {
          const int sr = sr0 + i * HW;
          fa[hs][i] = *reinterpret_cast<const frag_t*>(ab + sr * 128 + (((hs * 4 + qlo) ^ ((sr >> 1) & 7)) * 16));
        }
#pragma unroll
        for (int j = 0; j < NREP; ++j) fb[hs][j] = *reinterpret_cast<const frag_t*>(wb + (b_rd[j] ^ (hs * 64)));
      }
#pragma unroll
      for (int hs = 0; hs < 2; ++hs)
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) mma64(fa[hs][i], fb[hs][j], acc[i][j]);
      // issue order as in conv3x3_s8_kernel: first half-step's fragments, then one read of the second per two MFMAs of the first
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    }
    gk += 4; t += 4;
    if (t >= 9) { t -= 9; ++ci; }
  }
  wait_vmcnt<0>();
  // the four K groups meet (as in conv3x3_s8), then group 0 parks the sums for the sweep
  unsigned char* st = smem + (mh * MREP * 16 + (lane & 15)) * EP + (lane >> 4) * 16;
  __syncthreads();
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const int give_lo = round == 0 ? 2 : 1, take_hi = round == 0 ? 2 : 1;
    if (kq >= give_lo && kq < 2 * give_lo) {
      unsigned char* d = st + (kq - give_lo) * BM * EP;
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(d + i * 16 * EP + j * 64) = acc[i][j];
    }
    __syncthreads();
    if (kq < take_hi) {
      const unsigned char* d = st + kq * BM * EP;
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) acc[i][j] += *reinterpret_cast<const f32x4*>(d + i * 16 * EP + j * 64);
    }
    __syncthreads();
  }
  if (kq == 0) {
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(st + i * 16 * EP + j * 64) = acc[i][j];
  }
  __syncthreads();
  // sweep: tile row `row` is output pixel (y0 + row / 16, x0 + row % 16) of image img
  const long mbase = ((long)slice * g.Ho + y0) * g.Wo + x0;
  const bool vec_ok = (p.Nout & 3) == 0;
  const float img_scale = image_scale(p, img);
  constexpr int G4 = BN / 4;
  for (int idx = tid; idx < BM * G4; idx += NTHR) {
    const int row = idx / G4, c4 = idx - row * G4;
    const long m = mbase + (long)(row >> 4) * g.Wo + (row & 15);
    const int n = n0 + 4 * c4;
    if (n >= p.n_pad) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(smem + row * EP + c4 * 16);
    const bool full = vec_ok && n + 3 < p.Nout;
    v *= img_scale;
    if (p.bias) {
      if (full) v += *reinterpret_cast<const f32x4*>(p.bias + n);
      else for (int r = 0; r < 4; ++r) if (n + r < p.Nout) v[r] += p.bias[n + r];
    }
    if (p.act != IPOKE_ACT_NONE) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = fast_act<T>(p.act, v[r]);
    }
    if (p.dact) {
      const T* dp = reinterpret_cast<const T*>(p.dact) + m * p.ld_dact + n;
      if (full && (p.ld_dact & 3) == 0) {
        const pack_t y = *reinterpret_cast<const pack_t*>(dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= act_grad_from_out(p.dact_act, ET<T>::to_f32(y[r]));
      } else {
        for (int r = 0; r < 4; ++r)
          if (n + r < p.Nout) v[r] *= act_grad_from_out(p.dact_act, ET<T>::to_f32(dp[r]));
      }
    }
    if (!full) {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (n + r >= p.Nout) v[r] = 0.f;
    }
    if (p.c_f32) {
      float* Cp = reinterpret_cast<float*>(p.C) + m * p.ldc + p.c_coff;
      if (full && p.c_cstride == 1 && ((p.ldc | p.c_coff) & 3) == 0) *reinterpret_cast<f32x4*>(Cp + n) = v;
      else for (int r = 0; r < 4; ++r) if (n + r < p.Nout) Cp[(long)(n + r) * p.c_cstride] = v[r];
    } else {
      T* Cp = reinterpret_cast<T*>(p.C) + m * p.ldc + p.c_coff + n;
      if (n + 3 < p.n_pad && ((p.ldc | p.c_coff) & 3) == 0) {
        pack_t o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = ET<T>::from_f32(v[r]);
        *reinterpret_cast<pack_t*>(Cp) = o;
      } else {
        for (int r = 0; r < 4; ++r)
          if (n + r < p.n_pad) Cp[r] = ET<T>::from_f32(v[r]);
      }
    }
  }
}

// =============================================================================================
// The same convolution for WIDE layers (>= 128 input channels, output channels in tiles of 128): the 3 x 3 x 3 stages of the 3-D
// encoder at 128 / 256 channels, the 3 x 3 layers of the decoder, discriminators and VGG stack on 16 x 16 and larger maps.
// As implicit GEMMs those launches stream (taps) x (input tile) + (output tiles) x (whole filter) through L2 -> LDS:
// 128 -> 128 channels on 4 x 64 x 64 x 20 positions moves 2.3 GB of re-fetched input rows and 1.8 GB of filter per launch and runs
// at the DMA rate (455 us, 26 % of the matrix peak).  Here a workgroup owns a 16 x 16 pixel patch of one depth slice and ALL 128
// output channels of a tile: the patch's input with its halo (18 x 18 pixels, zero outside the map) is staged once per
// (64-channel chunk, depth tap) and serves nine taps; the filter K-blocks (one tap x 64 channels x 128 outputs, 16 KB) stream
// through a three-slot ring.  Per output the DMA traffic is a third of the implicit GEMM's and the loop is bound by the matrix
// cores: 8 waves = 4 pixel-row groups x 2 channel halves, 64 x 64 outputs each, 32 MFMAs per wave and barrier.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_halo16_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  typedef bf16_t T;
  typedef typename ET<T>::frag frag_t;
  typedef typename Pack4<T>::type pack_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int BM = 256, BN = 128, NTHR = 512, R = 4;
  constexpr int TH = 16, TW = 16, HW = TW + 2, HROWS = (TH + 2) * HW;       // 324 halo pixels
  constexpr int A_IT = 6;                                                   // 48 DMA pieces of 8 pixel rows >= 324 rows ...
  constexpr int A_PIECES = (HROWS + 7) / 8;                                 // ... of which 41 hold pixels: the image buffer is 41 KB
  constexpr int ABUF = A_PIECES * 1024, WSLOT = BN * 128, W_IT = WSLOT / (8 * 1024);
  constexpr int MREP = 4, NREP = 4;
  constexpr int EP = BN * 4 + 16;
  constexpr unsigned kInvalid = 0xffffffffu;
  static_assert(W_IT == 2 && 2 * ABUF + R * WSLOT >= BM * EP, "layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* abuf = smem;                              // 2 x ABUF: the halo image of a (chunk, depth tap), double-buffered
  unsigned char* ring = smem + 2 * ABUF;                   // R filter K-blocks
  unsigned char* dummy = ring + R * WSLOT;                 // landing zone of padding DMAs, 1 KB per wave
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 3, wn = wave >> 2;
  const GeomDev& g = p.g;
  const int tiles_x = g.Wo / TW, tiles_y = g.Ho / TH;
  const int tile = blockIdx.x, tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, slice = tile / (tiles_x * tiles_y);
  const int img = slice / g.Do, dz = slice - img * g.Do;
  const int y0 = ty * TH, x0 = tx * TW, n0 = blockIdx.y * BN;
  // Depth taps: "virtual chunks" v = chunk * kdn + (kd - kd_lo), nine K-blocks each.  Taps whose input slice lies outside the clip
  // (the first / last output slices of a 3 x 3 x 3 convolution) contribute zeros: they are left out of the list -- a sixth of the
  // work at depth 4, a third at depth 2.  Input slice of tap kd: forward dz * sd - 1 + kd; data gradient (sd = 1, mirrored) dz + 1 - kd.
  int kd_lo = 0, kd_hi = 0;
  if (g.taps == 27) {
    if (g.transposed) { kd_lo = max(0, dz + 2 - g.Di); kd_hi = min(2, dz + 1); }
    else { kd_lo = max(0, 1 - dz * g.sd); kd_hi = min(2, g.Di - dz * g.sd); }
  }
  const int kdn = kd_hi - kd_lo + 1;
  // taps per (chunk, depth tap): the 3 x 3 window, or the 2 x 2 window without padding of the four-tap sub-pixel phase of a stride-2
  // ConvTranspose2d (round 6: kh = kw = 2, ph = pw = 0, scattered output rows; offsets 0 / +1 lie inside the one-pixel halo)
  const int ntap = g.khw, tlast = ntap - 1;
  const int nch = (p.Kc >> 6) * kdn, nkb = nch * ntap;
  const int sgn = g.transposed ? -1 : 1;

  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  unsigned a_src[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int row = (wave + 8 * i) * 8 + (lane >> 3), pos = lane & 7;
    const int py = row / HW, px = row - py * HW, y = y0 - 1 + py, x = x0 - 1 + px;
    a_src[i] = kInvalid;
    if (row < HROWS && (unsigned)y < (unsigned)g.Hi && (unsigned)x < (unsigned)g.Wi)
      a_src[i] = (unsigned)((long)img * p.a_sn + (long)y * p.a_sh + (long)x * p.a_sw + p.a_coff + ((pos ^ ((row >> 1) & 7)) * 8));
  }
  unsigned w_src[W_IT];
#pragma unroll
  for (int j = 0; j < W_IT; ++j) {
    const int nl = (wave * W_IT + j) * 8 + (lane >> 3), n = n0 + nl, pos = lane & 7;
    w_src[j] = n < p.Nout ? (unsigned)((long)n * p.ldw + ((pos ^ ((nl >> 1) & 7)) * 8)) : kInvalid;
  }
  // filter K-block wi_g = (virtual chunk, tap): element offset w_off = (kd * 9 + tap) * Kc + chunk * 64, kept incrementally
  int wi_g = 0, wi_t = 0, wi_kd = 0, wi_ch = 0;
  const long w_off0 = (long)kd_lo * ntap * p.Kc;
  long w_off = w_off0;
  auto issue_w = [&]() {
    const bool in = wi_g < nkb;
#pragma unroll
    for (int j = 0; j < W_IT; ++j) {
      const bool real = in && w_src[j] != kInvalid;
      const T* src = real ? Wbase + w_src[j] + w_off : zero;
      unsigned char* dst = in ? ring + (wi_g % R) * WSLOT + (wave * W_IT + j) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    ++wi_g;
    const bool tap_wrap = wi_t == tlast, kd_wrap = tap_wrap && wi_kd + 1 == kdn;
    wi_t = tap_wrap ? 0 : wi_t + 1;
    wi_kd = kd_wrap ? 0 : (tap_wrap ? wi_kd + 1 : wi_kd);
    wi_ch = kd_wrap ? wi_ch + 1 : wi_ch;
    w_off = kd_wrap ? w_off0 + (long)wi_ch * 64 : w_off + p.Kc;
  };
  int a_next = 0;
  auto issue_a = [&]() {
    const int kd = kd_lo + a_next % kdn;
    const int dd = g.taps == 27 ? (g.transposed ? dz + 1 - kd : dz * g.sd - 1 + kd) : dz;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const bool real = a_next < nch && a_src[i] != kInvalid && (unsigned)dd < (unsigned)g.Di;
      const T* src = real ? Abase + a_src[i] + (long)dd * p.a_sd + (a_next / kdn) * 64 : zero;
      unsigned char* dst = a_next < nch && wave + 8 * i < A_PIECES ? abuf + (a_next & 1) * ABUF + (wave + 8 * i) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    ++a_next;
  };
  issue_a();
  issue_w(); issue_w(); issue_w();

  const int qlo = lane >> 4;
  int b_rd[NREP];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int n = wn * 64 + j * 16 + (lane & 15);
    b_rd[j] = n * 128 + ((qlo ^ ((n >> 1) & 7)) * 16);
  }
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragments of K-block kb (tap t of the image in buffer ci & 1, filter slot kb % R)
  auto read_frags = [&](frag_t (&fa)[2][MREP], frag_t (&fb)[2][NREP], int kb, int ci_, int t_) {
    const unsigned char* ab = abuf + (ci_ & 1) * ABUF;
    const unsigned char* wb = ring + (kb % R) * WSLOT;
    const int th = g.kw == 3 ? t_ / 3 : t_ >> 1, tw = t_ - g.kw * th;
    // halo row of output pixel (wm*4 + i, lane & 15) under this tap
    const int sr0 = (wm * 4 + 1 + sgn * (th - g.ph)) * HW + (lane & 15) + 1 + sgn * (tw - g.pw);
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
#pragma unroll
      for (int i = 0; i < MREP; ++i) {
        const int sr = sr0 + i * HW;
        fa[hs][i] = *reinterpret_cast<const frag_t*>(ab + sr * 128 + (((hs * 4 + qlo) ^ ((sr >> 1) & 7)) * 16));
      }
#pragma unroll
      for (int j = 0; j < NREP; ++j) fb[hs][j] = *reinterpret_cast<const frag_t*>(wb + (b_rd[j] ^ (hs * 64)));
    }
  };
  auto mma_frags = [&](frag_t (&fa)[2][MREP], frag_t (&fb)[2][NREP]) {
#pragma unroll
    for (int hs = 0; hs < 2; ++hs)
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) mma64(fa[hs][i], fb[hs][j], acc[i][j]);
  };
  // Round r: [K-block r + 1 has landed] barrier | DMA of K-block r + 3 (and, every ninth round, of the next halo image) | fragment
  // reads of K-block r + 1 into the other register set | 32 MFMAs on K-block r, two MFMAs per read in issue order.  The LDS latency
  // of a round's reads is covered by the previous round's matrix work; a filter block has two rounds to land.  DMA order inside a
  // round is filter first, image second, so that the image (needed nine rounds later) is not the newest transfer when the next
  // rounds wait for their filter block: vmcnt counts 8, 8, 2, 2, ... over a nine-round period.  (Measured and dropped: one image
  // piece per round with a constant vmcnt -- the per-round address arithmetic costs more than the uniform rounds gain, 349 vs 319 us.)
  frag_t fa0[2][MREP], fb0[2][NREP], fa1[2][MREP], fb1[2][NREP];
  wait_vmcnt<2 * W_IT>();                        // image 0 and K-block 0
  __builtin_amdgcn_s_barrier();
  read_frags(fa0, fb0, 0, 0, 0);
  int ci = 0, t = 0;                             // image / tap of K-block r
  auto round = [&](int r, frag_t (&fa_cur)[2][MREP], frag_t (&fb_cur)[2][NREP], frag_t (&fa_nxt)[2][MREP], frag_t (&fb_nxt)[2][NREP]) {
    if (t == 1 || t == 2) wait_vmcnt<A_IT + W_IT>(); else wait_vmcnt<W_IT>();
    __builtin_amdgcn_s_barrier();
    const int tn = t == tlast ? 0 : t + 1, cn = t == tlast ? ci + 1 : ci;
    read_frags(fa_nxt, fb_nxt, r + 1, cn, tn);      // (past the last K-block: stale LDS contents, never multiplied)
    // first half of the matrix work, one fragment read per MFMA in issue order: with the sixteen reads in front, eight waves queue
    // 128 ds_read_b128 on the LDS pipe after every barrier before any of them reaches its first MFMA (no-DMA build: 0.95 -> 0.79 us
    // per round, against 0.54 of MFMA time)
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) mma64(fa_cur[0][i], fb_cur[0][j], acc[i][j]);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    // the round's transfers are issued between the two halves: behind the barrier they would keep every wave off the matrix cores
    issue_w();                                   // K-block r + 3 -> the slot of K-block r - 1
    if (t == 0) issue_a();                       // image ci + 1 -> the buffer of image ci - 1 (a padding transfer past the end)
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) mma64(fa_cur[1][i], fb_cur[1][j], acc[i][j]);
    t = tn; ci = cn;
  };
  for (int r = 0; r < nkb; r += 2) {
    round(r, fa0, fb0, fa1, fb1);
    if (r + 1 < nkb) round(r + 1, fa1, fb1, fa0, fb0);
  }
  wait_vmcnt<0>();
  __syncthreads();
  // park the sums for the sweep: tile row = pixel (wm*4 + i, lane & 15), column = wn*64 + 16 j + 4 (lane >> 4) + e
  {
    unsigned char* st = smem + ((wm * 4) * 16 + (lane & 15)) * EP + (wn * 64 + (lane >> 4) * 4) * 4;
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(st + i * 16 * EP + j * 64) = acc[i][j];
  }
  __syncthreads();
  const long mbase = p.c_scatter ? p.c_row0 + (long)img * p.c_sn + (long)y0 * p.c_sh + (long)x0 * p.c_sw : ((long)slice * g.Ho + y0) * g.Wo + x0;
  const long m_sh = p.c_scatter ? p.c_sh : g.Wo, m_sw = p.c_scatter ? p.c_sw : 1;
  const bool vec_ok = (p.Nout & 3) == 0;
  const float img_scale = image_scale(p, img);
  constexpr int G4 = BN / 4;
  for (int idx = tid; idx < BM * G4; idx += NTHR) {
    const int row = idx / G4, c4 = idx - row * G4;
    const long m = mbase + (long)(row >> 4) * m_sh + (long)(row & 15) * m_sw;
    const int n = n0 + 4 * c4;
    if (n >= p.n_pad) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(smem + row * EP + c4 * 16);
    const bool full = vec_ok && n + 3 < p.Nout;
    v *= img_scale;
    if (p.bias) {
      if (full) v += *reinterpret_cast<const f32x4*>(p.bias + n);
      else for (int e = 0; e < 4; ++e) if (n + e < p.Nout) v[e] += p.bias[n + e];
    }
    if (p.act != IPOKE_ACT_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fast_act<T>(p.act, v[e]);
    }
    if (p.dact) {
      const T* dp = reinterpret_cast<const T*>(p.dact) + m * p.ld_dact + n;
      if (full && (p.ld_dact & 3) == 0) {
        const pack_t y = *reinterpret_cast<const pack_t*>(dp);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= act_grad_from_out(p.dact_act, ET<T>::to_f32(y[e]));
      } else {
        for (int e = 0; e < 4; ++e)
          if (n + e < p.Nout) v[e] *= act_grad_from_out(p.dact_act, ET<T>::to_f32(dp[e]));
      }
    }
    if (!full) {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (n + e >= p.Nout) v[e] = 0.f;
    }
    if (p.c_f32) {
      float* Cp = reinterpret_cast<float*>(p.C) + m * p.ldc + p.c_coff;
      if (full && p.c_cstride == 1 && ((p.ldc | p.c_coff) & 3) == 0) *reinterpret_cast<f32x4*>(Cp + n) = v;
      else for (int e = 0; e < 4; ++e) if (n + e < p.Nout) Cp[(long)(n + e) * p.c_cstride] = v[e];
    } else {
      T* Cp = reinterpret_cast<T*>(p.C) + m * p.ldc + p.c_coff + n;
      if (n + 3 < p.n_pad && ((p.ldc | p.c_coff) & 3) == 0) {
        pack_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ET<T>::from_f32(v[e]);
        *reinterpret_cast<pack_t*>(Cp) = o;
      } else {
        for (int e = 0; e < 4; ++e)
          if (n + e < p.n_pad) Cp[e] = ET<T>::from_f32(v[e]);
      }
    }
  }
}

// =============================================================================================
// Stride-1 convolutions with <= 64 output channels and a filter that FITS IN LDS, on large maps: the 128 x 128 layers of the decoder
// (3 x 3, 64 -> 64 and the 64 -> 3 image head over all frames of a batch of clips: 7.9 M pixels in sampling) and the four sub-pixel
// phases of its last up-convolution (1 / 2 / 2 / 4 taps of 128 -> 64 channels, scattered output rows).  Their reductions are 2 - 9
// K-blocks deep: conv3x3_halo_kernel / the implicit GEMM spend ~8 us per 64 - 128-pixel workgroup on prologue, filter stream and
// epilogue (2.0 ms for 580 GFLOP and 1 GB of input; 0.6 ms per phase).  Here the WHOLE filter (taps x chunks x 8 KB <= 72 KB) is loaded
// once per workgroup and stays in LDS; persistent workgroups (one per CU) walk over 16 x 16-pixel patches, one 64-channel chunk of the
// patch's halo image (18 x 18 pixels = 41 KB, zero outside the map) per buffer, double-buffered -- the only stream --, one barrier
// per image.  Taps are the kh x kw window at offsets a - ph (ph - a for the data gradient), all within the one-pixel halo.
// 8 waves = 4 pixel-row groups x 2 halves of 32 output channels; fragments beyond Nout are skipped (the image head computes 16 of
// 64 columns); the epilogue runs from the accumulators.
// Measured with one phase taken out at a time (no MFMA / no epilogue / no image stream), 64 -> 64 at 128 x 128, 480 images: 937 us
// full, 681 / 663 / 756 us ablated -- the three phases of a patch (wait for the image 1.5 us, MFMAs 2.2 us, epilogue 2.4 us) run one after
// the other; deferring the epilogue by one image (its stores issued in front of the next patch's MFMAs) measured 964 us: not the stores'
// acknowledgement at the loop's vmcnt(0).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_c64_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  typedef bf16_t T;
  typedef typename ET<T>::frag frag_t;
  typedef typename Pack4<T>::type pack_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int TH = 16, TW = 16, HW = TW + 2, HROWS = (TH + 2) * HW;       // 324 halo pixels
  constexpr int A_IT = 6, A_PIECES = (HROWS + 7) / 8, ABUF = A_PIECES * 1024;
  constexpr int WBYTES = 9 * 64 * 128, W_IT = WBYTES / (8 * 1024);
  constexpr int MREP = 4, NREP = 2;
  static_assert(W_IT == 9, "filter pieces per wave");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* wbuf = smem;                              // [tap][chunk][64 output channels][64 input channels], rows swizzled
  unsigned char* abuf = smem + WBYTES;                     // 2 x ABUF halo images
  unsigned char* dummy = abuf + 2 * ABUF;                  // landing zone of padding DMAs (1 KB, shared)
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 3, wn = wave >> 2;
  const GeomDev& g = p.g;
  const int tiles_x = g.Wo / TW, tiles_y = g.Ho / TH, ntiles = (g.M / (g.Ho * g.Wo)) * tiles_x * tiles_y;
  const int ntaps = g.khw, nch = p.Kc >> 6, nimg = ntiles * nch;          // virtual images: (patch, chunk)
  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  const int lrow = lane >> 3, lpos = lane & 7;

  // ---- the filter, once: piece = ((tap * nch + chunk) * 8 + row group)
  {
    const int npieces = ntaps * nch * 8;
#pragma unroll
    for (int j = 0; j < W_IT; ++j) {
      const int piece = wave * W_IT + j;
      const int tc = piece >> 3, tap = tc / nch, ch = tc - tap * nch, nl = (piece & 7) * 8 + lrow;
      const bool real = piece < npieces && nl < p.Nout;
      const T* src = real ? Wbase + (long)nl * p.ldw + tap * p.Kc + ch * 64 + ((lpos ^ ((nl >> 1) & 7)) * 8) : zero;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(piece < npieces ? wbuf + piece * 1024 : dummy), 16, 0, 0);
    }
  }
  auto issue_image = [&](int v, int buf) {                 // v = tile * nch + chunk
    const bool have = v < nimg;
    const int tile = v / nch, ch = v - tile * nch;
    const int tx = tile % tiles_x, t2 = tile / tiles_x, ty = t2 % tiles_y, img = t2 / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int pi = wave + 8 * i, row = pi * 8 + lrow;
      const int py = row / HW, px = row - py * HW, y = y0 - 1 + py, x = x0 - 1 + px;
      const bool real = have && row < HROWS && (unsigned)y < (unsigned)g.Hi && (unsigned)x < (unsigned)g.Wi;
      const T* src = real ? Abase + (long)img * p.a_sn + (long)y * p.a_sh + (long)x * p.a_sw + p.a_coff + ch * 64 + ((lpos ^ ((row >> 1) & 7)) * 8) : zero;
      unsigned char* dst = have && pi < A_PIECES ? abuf + buf * ABUF + pi * 1024 : dummy;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
  };
  const int vstep = (int)gridDim.x * nch;                  // a workgroup's patches: blockIdx.x, blockIdx.x + gridDim.x, ...
  int v = (int)blockIdx.x * nch;                           // its images in order: the chunks of a patch, then the next patch
  auto next_image = [&](int vv) { return (vv % nch) + 1 < nch ? vv + 1 : vv - (nch - 1) + vstep; };
  issue_image(v, 0);

  const int qlo = lane >> 4;
  const int nfrag = min(NREP, max(0, (p.Nout - wn * 32 + 15) >> 4));      // 16-column fragments of this wave that hold outputs
  int b_rd[NREP];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int n = wn * 32 + j * 16 + (lane & 15);
    b_rd[j] = n * 128 + ((qlo ^ ((n >> 1) & 7)) * 16);
  }
  const bool vec_ok = (p.Nout & 3) == 0;
  int buf = 0;
  f32x4 acc[MREP][NREP];
  for (; v < nimg; v = next_image(v), buf ^= 1) {
    const int ch = v % nch;
    wait_vmcnt<0>();                               // this image (and, the first time, the filter) has landed
    __builtin_amdgcn_s_barrier();                  // ... everybody's share of it; the other buffer is no longer read
    issue_image(next_image(v), buf ^ 1);
    if (ch == 0) {
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (nfrag == 0) continue;
    const unsigned char* ab = abuf + buf * ABUF;
    for (int t = 0; t < ntaps; ++t) {
      const int ta = t / g.kw, tb = t - ta * g.kw;
      const int dy = g.transposed ? g.ph - ta : ta - g.ph, dx = g.transposed ? g.pw - tb : tb - g.pw;
      const int sr0 = (wm * 4 + 1 + dy) * HW + (lane & 15) + 1 + dx;
      const unsigned char* wb = wbuf + (t * nch + ch) * 64 * 128;
#pragma unroll
      for (int hs = 0; hs < 2; ++hs) {
        frag_t fa[MREP], fb[NREP];
#pragma unroll
        for (int i = 0; i < MREP; ++i) {
          const int sr = sr0 + i * HW;
          fa[i] = *reinterpret_cast<const frag_t*>(ab + sr * 128 + (((hs * 4 + qlo) ^ ((sr >> 1) & 7)) * 16));
        }
#pragma unroll
        for (int j = 0; j < NREP; ++j) fb[j] = *reinterpret_cast<const frag_t*>(wb + (b_rd[j] ^ (hs * 64)));
#pragma unroll
        for (int i = 0; i < MREP; ++i) {
          mma64(fa[i], fb[0], acc[i][0]);
          if (nfrag > 1) mma64(fa[i], fb[1], acc[i][1]);
        }
      }
    }
    if (ch + 1 < nch) continue;
    // ---- epilogue straight from the accumulators: acc[i][j][e] = pixel (wm*4 + i, lane & 15), channel wn*32 + 16 j + 4 (lane >> 4) + e
    const int tile = v / nch;
    const int tx = tile % tiles_x, t2 = tile / tiles_x, ty = t2 % tiles_y, img = t2 / tiles_y;
    const int oy = ty * TH + wm * 4, ox = tx * TW + (lane & 15);
    const float img_scale = image_scale(p, img);
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const int n = wn * 32 + j * 16 + qlo * 4;
      if (j >= nfrag || n >= p.n_pad) continue;
      const bool full = vec_ok && n + 3 < p.Nout;
      f32x4 b4 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p.bias) {
        if (full) b4 = *reinterpret_cast<const f32x4*>(p.bias + n);
        else for (int e = 0; e < 4; ++e) if (n + e < p.Nout) b4[e] = p.bias[n + e];
      }
#pragma unroll
      for (int i = 0; i < MREP; ++i) {
        const long m = p.c_scatter ? p.c_row0 + (long)img * p.c_sn + (long)(oy + i) * p.c_sh + (long)ox * p.c_sw
                                   : ((long)img * g.Ho + oy + i) * g.Wo + ox;
        f32x4 v4 = acc[i][j] * img_scale + b4;
        if (p.act != IPOKE_ACT_NONE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v4[e] = fast_act<T>(p.act, v4[e]);
        }
        if (!full) {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (n + e >= p.Nout) v4[e] = 0.f;
        }
        if (p.c_f32) {
          float* Cp = reinterpret_cast<float*>(p.C) + m * p.ldc + p.c_coff;
          if (full && p.c_cstride == 1 && ((p.ldc | p.c_coff) & 3) == 0) *reinterpret_cast<f32x4*>(Cp + n) = v4;
          else for (int e = 0; e < 4; ++e) if (n + e < p.Nout) Cp[(long)(n + e) * p.c_cstride] = v4[e];
        } else {
          T* Cp = reinterpret_cast<T*>(p.C) + m * p.ldc + p.c_coff + n;
          if (n + 3 < p.n_pad && ((p.ldc | p.c_coff) & 3) == 0) {
            pack_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ET<T>::from_f32(v4[e]);
            *reinterpret_cast<pack_t*>(Cp) = o;
          } else {
            for (int e = 0; e < 4; ++e)
              if (n + e < p.n_pad) Cp[e] = ET<T>::from_f32(v4[e]);
          }
        }
      }
    }
  }
  wait_vmcnt<0>();
}

// Dispatch switches of the two persistent / wide 3 x 3 kernels: 0 off, 1 (default) where measured faster, 2 wherever the kernel can run.
// The parity tests move them at run time through ipoke_set_dispatch_override (atomics because launches on distinct streams may come
// from distinct threads).
static std::atomic<int> g_c64_mode{1}, g_halo16_mode{1}, g_nn128_mode{1}, g_nt128_mode{1};
static std::atomic<int> g_cpl_split{0};      // "cpl_split": K slices of ipoke_conv3x3_coupling where they fit (0: the rule of coupling_splits)

// an ELU launch that stores fp32: the sweeps of the c64 / halo16 / halo kernels take ELU through fast_act (exp(x) - 1, the bf16-store
// form); such a launch goes to the implicit GEMM, whose general sweep uses expm1f for fp32 stores
static bool elu_f32_store(const NtParams& p) { return p.c_f32 && p.act == IPOKE_ACT_ELU; }

static bool c64_applicable(const NtParams& p) {
  // mode 1 (default): at >= 512 patches (two per CU)
  const int mode = g_c64_mode.load(std::memory_order_relaxed);
  const GeomDev& g = p.g;
  if (!mode || elu_f32_store(p)) return false;
  // window offsets a - ph (forward) / ph - a (data gradient) must lie within the one-pixel halo
  const int kh = g.kw > 0 ? g.khw / g.kw : 0;
  const int lo_y = g.transposed ? g.ph - (kh - 1) : -g.ph, hi_y = g.transposed ? g.ph : kh - 1 - g.ph;
  const int lo_x = g.transposed ? g.pw - (g.kw - 1) : -g.pw, hi_x = g.transposed ? g.pw : g.kw - 1 - g.pw;
  const int nch = p.Kc / 64;
  const bool can = !p.a_f32 && !p.dact && g.taps == g.khw && kh >= 1 && g.khw == kh * g.kw && g.Di == 1 && g.Do == 1 && g.pd == 0 &&
                   g.Hi == g.Ho && g.Wi == g.Wo && g.Ho % 16 == 0 && g.Wo % 16 == 0 && g.sd == 1 && g.sh == 1 && g.sw == 1 &&
                   lo_y >= -1 && hi_y <= 1 && lo_x >= -1 && hi_x <= 1 && (!g.transposed || (kh == 3 && g.kw == 3)) &&
                   (p.Kc == 64 || p.Kc == 128) && p.Kc_real == p.Kc && g.khw * nch <= 9 && (g.khw > 1 || p.c_scatter) && p.Nout <= 64 && (p.a_coff & 7) == 0 &&
                   p.ldw >= p.Ktot && (p.ldw & 7) == 0 && p.splitk == 1 && !p.c_acc && ((p.a_sn | p.a_sh | p.a_sw) & 7) == 0 && p.n_pad <= 64 &&
                   (reinterpret_cast<uintptr_t>(p.W) & 15) == 0;
  if (!can || kLdsC64 > device_max_lds()) return false;
  return mode == 2 || g.M / 256 >= 512;
}
static int launch_conv3x3_c64(NtParams& p, hipStream_t s) {
  const size_t lds = kLdsC64;
  auto kern = conv3x3_c64_kernel;
  IPK_SET_LDS_ONCE(kern, lds);
  const int ntiles = p.g.M / 256;
  p.tiles_m = ntiles; p.tiles_n = 1; p.xa = p.xb = 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)std::min(ntiles, 256)), dim3(512), lds, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

static bool halo16_applicable(const NtParams& p) {
  const int mode = g_halo16_mode.load(std::memory_order_relaxed);
  const GeomDev& g = p.g;
  // the four-tap sub-pixel phase of a stride-2 ConvTranspose2d (2 x 2 window, no padding, scattered output rows)
  const bool phase4 = g.taps == 4 && g.khw == 4 && g.kw == 2 && g.ph == 0 && g.pw == 0 && !g.transposed && g.Di == 1 && g.Do == 1 && g.pd == 0 &&
                      g.sd == 1 && p.c_scatter && !p.dact;
  if (!mode || p.a_f32 || elu_f32_store(p)) return false;
  if (!phase4 && (p.c_scatter || !(g.taps == 9 || g.taps == 27) || g.khw != 9 || g.kw != 3)) return false;
  const bool flat = phase4 || (g.taps == 9 && g.Di == 1 && g.Do == 1 && g.pd == 0 && g.sd == 1);
  const bool deep = !phase4 && g.taps == 27 && g.pd == 1 && (p.a_sd & 7) == 0 && (g.sd == 1 ? g.Di == g.Do : (!g.transposed && g.sd == 2));
  if (!(flat || deep)) return false;
  const bool can = g.Hi == g.Ho && g.Wi == g.Wo && g.Ho % 16 == 0 && g.Wo % 16 == 0 && g.sh == 1 && g.sw == 1 && (phase4 || (g.ph == 1 && g.pw == 1)) &&
                   p.Kc % 64 == 0 && p.Kc_real == p.Kc && (p.a_coff & 7) == 0 && p.ldw >= p.Ktot && p.splitk == 1 && !p.c_acc &&
                   ((p.a_sn | p.a_sh | p.a_sw) & 7) == 0 &&
                   (long)(g.M / g.S) * p.a_sn + (long)g.Di * p.a_sd + (long)g.Hi * p.a_sh + p.Kc < (1L << 31) && (long)p.Nout * p.ldw < (1L << 31);
  if (!can || kLdsHalo16 > device_max_lds()) return false;
  if (mode == 2) return true;
  // Measured (scripts/probe_halo16.py, B = 20, against the kernels used before): 128 -> 128 channels on 4 x 64 x 64: 304 vs 485 us;
  // 64 -> 128, depth stride 2, 8 x 64 x 64: 175 vs 302; 2-D 128 -> 128 on 64 x 64 at B = 32: 52 vs 73 -- but 256 -> 256 on
  // 2 x 32 x 32 (320 workgroups = 1.25 rounds of the chip): 207 vs 201, 2-D 64 x 64 at B = 20 (320): 47 vs 45, 16 x 16 maps (40 - 80
  // workgroups): 39 vs 19.  The kernel holds one workgroup per CU, so it is taken when the grid fills whole rounds of 256 to >= 80 %
  // and the 128-wide output tile is not mostly padding; 64-channel 2-D layers stay with conv3x3_halo_kernel.
  // (a deep layer of depth <= 2 skips a third of its taps here and not in the implicit GEMM: that outweighs a ragged last round)
  const long wgs = (long)(g.M / 256) * ceil_div(p.Nout, 128), rounds = (wgs + 255) / 256;
  const bool shallow = deep && g.Do <= 2 && g.Di <= 2 * g.sd;
  return (deep ? p.Kc >= 64 : p.Kc >= 128) && p.Nout >= 96 && wgs >= 256 && (wgs * 10 >= rounds * 256 * 8 || (shallow && wgs * 10 >= rounds * 256 * 6));
}
static int launch_conv3x3_halo16(NtParams& p, hipStream_t s) {
  const size_t lds = kLdsHalo16;
  auto kern = conv3x3_halo16_kernel;
  IPK_SET_LDS_ONCE(kern, lds);
  p.tiles_m = p.g.M / 256; p.tiles_n = ceil_div(p.Nout, 128); p.xa = p.xb = 0;
  dim3 grid((unsigned)p.tiles_m, (unsigned)p.tiles_n);
  hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

static bool halo_applicable(const NtParams& p) {
  const GeomDev& g = p.g;
  const bool flat = g.taps == 9 && g.Di == 1 && g.Do == 1 && g.pd == 0;
  const bool deep = g.taps == 27 && g.Di == g.Do && g.pd == 1 && (p.a_sd & 7) == 0;
  if (!(flat || deep) || p.c_scatter || elu_f32_store(p) || kLdsHalo > device_max_lds()) return false;
  if (deep) {     // measured against the 27-tap implicit GEMM (B = 20): 64 channels 16x64x64: 670 vs 997 us, 12x32x32: 126 vs 185 us; but 128
                  // channels 8x32x32: 271 vs 230, 256 channels 4x16x16: 141 vs 101, 512 channels: 255 vs 177 -> 64 input channels only
    if (p.Kc > 64) return false;
    return !p.a_f32 && g.khw == 9 && g.kw == 3 && g.Hi == g.Ho && g.Wi == g.Wo && g.Ho % 8 == 0 && g.Wo % 16 == 0 &&
           g.sd == 1 && g.sh == 1 && g.sw == 1 && g.ph == 1 && g.pw == 1 && p.Kc % 64 == 0 && p.Kc_real == p.Kc && (p.a_coff & 7) == 0 &&
           p.ldw >= p.Ktot && p.splitk == 1 && !p.c_acc && ((p.a_sn | p.a_sh | p.a_sw) & 7) == 0 &&
           (long)(g.M / g.S) * p.a_sn + (long)g.Di * p.a_sd + p.Kc < (1L << 31) && (long)p.Nout * p.ldw < (1L << 31) && g.M >= 4096;
  }
  return !p.a_f32 && g.taps == 9 && g.khw == 9 && g.kw == 3 && g.Di == 1 && g.Do == 1 && g.Hi == g.Ho && g.Wi == g.Wo &&
         g.Ho % 8 == 0 && g.Wo % 16 == 0 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 && g.ph == 1 && g.pw == 1 &&
         p.Kc % 64 == 0 && p.Kc_real == p.Kc && (p.a_coff & 7) == 0 && p.ldw >= p.Ktot && p.splitk == 1 && !p.c_acc &&
         ((p.a_sn | p.a_sh | p.a_sw) & 7) == 0 && (long)(g.M / g.S) * p.a_sn + (long)g.Hi * p.a_sh + p.Kc < (1L << 31) &&
         (long)p.Nout * p.ldw < (1L << 31) && g.M >= 4096 &&
         // measured against the implicit-GEMM kernel (B = 32): 64 channels at 128 x 128: 139 vs 181 us,
         // 64 -> 3: 129 vs 168, 256 channels at 16 x 16: 18 vs 32 us, 512 at 16 x 16 (N = 300): 486 vs 682; but 128 channels at
         // 64 x 64: 91 vs 86 and 256 at 32 x 32: 68 vs 67 -- there the nine-tap re-fetch is hidden and the generic tile map wins
         (p.Kc <= 64 || g.Ho * g.Wo <= 256);
}
static int launch_conv3x3_halo(NtParams& p, hipStream_t s) {
  const size_t lds = kLdsHalo;
  auto kern = conv3x3_halo_kernel;
  IPK_SET_LDS_ONCE(kern, lds);
  p.tiles_m = p.g.M / 128; p.tiles_n = ceil_div(p.Nout, 64); p.xa = p.xb = 0;
  dim3 grid((unsigned)p.tiles_m, (unsigned)p.tiles_n);
  hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

// chunks of 64 input channels per split such that (row tiles) x (splits) stays within one round of workgroups
static int conv3x3_s8_splits(int M, int Kc, int TS) {
  const int tiles = ceil_div(M, 64 * TS), nchunks = Kc / 64;
  int want = 256 / tiles; if (want < 1) want = 1; if (want > 32) want = 32; if (want > nchunks) want = nchunks;
  const int cps = ceil_div(nchunks, want);
  return ceil_div(nchunks, cps);
}

template <typename T, int WM, int WN, int MREP, int NREP, int NSTAGE, int KPB, bool SIMPLE, int WK = 1>
static int launch_nt_glds_impl(NtParams& p, hipStream_t s) {
  constexpr int BM = WM * MREP * 16, BN = WN * NREP * 16;
  constexpr int BK = 128 / (int)sizeof(T);
  p.tiles_m = ceil_div(p.g.M, BM);
  p.tiles_n = ceil_div(p.Nout, BN);
  const int nkb = ceil_div(p.Ktot, BK);
  if (p.splitk < 1) p.splitk = 1;
  p.kb_per_split = ceil_div(nkb, p.splitk);
  pick_xcd_map(p);
  { int rc = acc_scratch_fits(p, BM, BN, WK == 1 && NtDet<WM, WN, MREP, NREP>::value); if (rc) return rc; }
  size_t lds = (size_t)NSTAGE * KPB * (BM + BN) * 128 + WM * WN * WK * 64 * 16 + 256 * sizeof(int);
  if (lds < (size_t)WK * BM * (BN * 4 + 16)) lds = (size_t)WK * BM * (BN * 4 + 16);      // epilogue staging (+ the K halves' hand-over)
  auto kern = igemm_nt_glds_kernel<T, WM, WN, MREP, NREP, NSTAGE, KPB, SIMPLE, WK>;
  IPK_SET_LDS_ONCE(kern, lds);
  dim3 grid((unsigned)((long)p.tiles_m * p.tiles_n), (unsigned)p.splitk);
  hipLaunchKernelGGL(kern, grid, dim3(WM * WN * WK * 64), lds, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

template <typename T, int WM, int WN, int MREP, int NREP, int NSTAGE, int KPB = 1, int WK = 1>
static int launch_nt_glds(NtParams& p, hipStream_t s) {
  constexpr int BK = 128 / (int)sizeof(T);
  const bool simple = p.Kc % BK == 0 && p.Kc_real == p.Kc && p.ldw >= p.Ktot;
  return simple ? launch_nt_glds_impl<T, WM, WN, MREP, NREP, NSTAGE, KPB, true, WK>(p, s)
                : launch_nt_glds_impl<T, WM, WN, MREP, NREP, NSTAGE, KPB, false, WK>(p, s);
}

template <typename T, int WM, int WN, int MREP, int NREP>
static int launch_nt(NtParams& p, hipStream_t s) {
  constexpr int BM = WM * MREP * 16, BN = WN * NREP * 16;
  constexpr int BK = 128 / (int)sizeof(T);
  p.tiles_m = ceil_div(p.g.M, BM);
  p.tiles_n = ceil_div(p.Nout, BN);
  const int nkb = ceil_div(p.Ktot, BK);
  if (p.splitk < 1) p.splitk = 1;
  p.kb_per_split = ceil_div(nkb, p.splitk);
  pick_xcd_map(p);
  { int rc = acc_scratch_fits(p, BM, BN, NtDet<WM, WN, MREP, NREP>::value); if (rc) return rc; }
  const long nt = (long)p.tiles_m * p.tiles_n;
  size_t lds = 2 * (BM + BN) * kPitch;
  if (lds < (size_t)BM * (BN * 4 + 16)) lds = (size_t)BM * (BN * 4 + 16);
  lds += 256 * sizeof(int);
  auto kern = igemm_nt_kernel<T, WM, WN, MREP, NREP>;
  IPK_SET_LDS_ONCE(kern, lds);     // one flag per template instantiation
  dim3 grid((unsigned)nt, (unsigned)p.splitk);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// conv3x3_k8 (round 6): 3x3 / stride 1 / 'same' convolution (direct or transposed) whose INPUT is one 16-byte chunk of channels per
// pixel (Kc = 8, bf16) and whose output has <= 64 channels -- the data gradient of the decoder's last convolution (64 -> 3 channels at
// 128 x 128, util.py Conv2dBlock `out_conv`): 4.9 M output rows x 64 channels from a gradient of 3 (padded to 8) channels.  As an implicit
// GEMM it is K = 72 in two 64-wide K blocks per 64-row tile: 76 800 workgroups that each stage 18 KB through LDS for 9 MFLOP, 1.04 ms for
// 629 MB written (45 TFLOP/s).  Here nothing is staged: a wave owns 16 consecutive pixels of an image row; the fragment of a matrix-core
// K step is FOUR TAPS -- lane group g holds the 8 channels of tap 4 ks + g, i.e. ONE 16-byte load of the gradient at the shifted pixel
// (zero outside the image and for the three taps beyond the ninth) -- the whole filter (9 taps x 8 channels x 64 outputs = 9 KB) lives in
// 48 registers per lane, and with the operand roles of mma64 a lane ends up with four consecutive output channels of its pixel: 8-byte
// stores.  Persistent waves, the next group's three loads in flight under the twelve matrix-core instructions of the current one.
__global__ __launch_bounds__(256) void conv3x3_k8_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  const GeomDev& g = p.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m16 = lane & 15, kg = lane >> 4;
  const int nt = p.Nout >> 4;
  const bf16_t* W = reinterpret_cast<const bf16_t*>(p.W);
  const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A) + p.a_coff;
  bf16_t* C = reinterpret_cast<bf16_t*>(p.C) + p.c_coff;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 wf[3][4];
  int dy[3], dx[3];
  bool tv[3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const int tap = 4 * ks + kg;
    tv[ks] = tap < 9;
    const int a = tap / 3, b = tap - 3 * a;
    dy[ks] = g.transposed ? g.ph - a : a - g.ph;
    dx[ks] = g.transposed ? g.pw - b : b - g.pw;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      wf[ks][t] = (tv[ks] && t < nt) ? *reinterpret_cast<const bf16x8*>(W + (long)(16 * t + m16) * p.ldw + tap * 8) : zero;
  }
  const int ngroups = g.M >> 4;
  const int stride = (int)gridDim.x * 4;
  auto gather = [&](int grp, bf16x8 (&fa)[3]) {
    const int m = grp * 16 + m16;
    const int ox = m & (g.Wo - 1), oy = (m >> g.lWo) & (g.Ho - 1), n = m >> (g.lWo + g.lHo);
    const bf16_t* img = A + (long)n * p.a_sn;
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      const int iy = oy + dy[ks], ix = ox + dx[ks];
      const bool ok = tv[ks] && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
      fa[ks] = ok ? *reinterpret_cast<const bf16x8*>(img + (long)iy * p.a_sh + (long)ix * p.a_sw) : zero;
    }
  };
  int grp = (int)blockIdx.x * 4 + wave;
  if (grp >= ngroups) return;
  bf16x8 cur[3], nxt[3];
  gather(grp, cur);
  for (; grp < ngroups; grp += stride) {
    const bool more = grp + stride < ngroups;
    if (more) gather(grp + stride, nxt);
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 3; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nt) mma64(cur[ks], wf[ks][t], acc[t]);
    bf16_t* row = C + (long)(grp * 16 + m16) * p.ldc + 4 * kg;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nt) {
        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
        bf16x4_t o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (bf16_t)acc[t][q];
        *reinterpret_cast<bf16x4_t*>(row + 16 * t) = o;
      }
    }
    if (more) {
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) cur[ks] = nxt[ks];
    }
  }
}
static bool k8_applicable(const NtParams& p) {
  const GeomDev& g = p.g;
  return !p.a_f32 && !p.c_f32 && !p.c_acc && p.splitk == 1 && !p.dact && !p.bias && p.act == IPOKE_ACT_NONE && !p.row_scale && !p.c_scatter &&
         !p.w_kmajor && g.taps == 9 && g.khw == 9 && g.kw == 3 && g.Di == 1 && g.Do == 1 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 &&
         g.ph == 1 && g.pw == 1 && g.Hi == g.Ho && g.Wi == g.Wo && g.pow2 && (g.Wo & 15) == 0 && p.Kc == 8 && p.a_sc == 1 && (p.Nout & 15) == 0 &&
         p.Nout <= 64 && (p.a_coff & 7) == 0 && ((p.a_sn | p.a_sh | p.a_sw) & 7) == 0 && p.ldw >= 72 && (p.ldw & 7) == 0 &&
         (reinterpret_cast<uintptr_t>(p.W) & 15) == 0 && p.c_cstride == 1 && (p.c_coff & 3) == 0 && (p.ldc & 3) == 0 && (g.M & 15) == 0 &&
         g.M >= 65536 && (reinterpret_cast<uintptr_t>(p.A) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.C) & 7) == 0;
}
static int launch_conv3x3_k8(NtParams& p, hipStream_t s) {
  const int groups = p.g.M >> 4;
  const int blocks = std::min((groups + 3) / 4, 256 * 8);
  hipLaunchKernelGGL(conv3x3_k8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

static bool k64_applicable(const NtParams& p) {
  const GeomDev& g = p.g;
  return kLdsK64 <= device_max_lds() && !p.c_scatter && !p.a_f32 && !p.row_scale && g.taps == 9 && g.khw == 9 && g.kw == 3 && g.Di == 1 && g.Hi == 8 &&
         g.Wi == 8 && g.lDo == 0 && g.lHo == 3 && g.lWo == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 && g.ph == 1 && g.pw == 1 &&
         p.Kc <= 64 && (p.Kc & 7) == 0 && p.Kc_real == p.Kc && p.Nout >= 256 && p.splitk == 1 && !p.c_acc && (p.a_coff & 7) == 0 &&
         p.ldw >= p.Ktot && ((p.a_sn | p.a_sh | p.a_sw) & 7) == 0 && (long)(g.M >> 6) * p.a_sn + 7 * p.a_sh + 7 * p.a_sw + p.Kc < (1L << 31) &&
         (long)p.Nout * p.ldw < (1L << 31) && 128 * (128 * 4 + 16) <= (int)kLdsK64 &&
         // one workgroup per CU (115 KB of LDS): a second round loses to the implicit GEMM (B = 40: 14.9 against 13.4 us; B = 20 / 32: 8.2 / 8.5
         // against 9.9 / 11.0 isolated)
         (long)ceil_div(g.M, 128) * ceil_div(p.Nout, 128) <= 256;
}
static int launch_conv3x3_k64(NtParams& p, hipStream_t s) {
  p.tiles_m = ceil_div(p.g.M, 128); p.tiles_n = ceil_div(p.Nout, 128); p.xa = p.xb = 0;
  p.kb_per_split = 9;
  auto kern = conv3x3_k64_kernel;
  IPK_SET_LDS_ONCE(kern, kLdsK64);
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(512), kLdsK64, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

static constexpr int kS8SamplesPerTile = 2;      // 8x8 maps per 128-row tile of conv3x3_s8
static bool s8_shape(const NtParams& p) {      // (host only: no device query)
  const GeomDev& g = p.g;
  return !p.c_scatter && !p.a_f32 && g.taps == 9 && g.khw == 9 && g.kw == 3 && g.Di == 1 && g.Hi == 8 && g.Wi == 8 &&
         g.lDo == 0 && g.lHo == 3 && g.lWo == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 && g.ph == 1 && g.pw == 1 &&
         p.Kc % 64 == 0 && p.Kc_real == p.Kc && p.Kc >= 256 && p.Nout <= 64 && (p.a_coff & 7) == 0 && p.ldw >= p.Ktot &&
         ((p.a_sn | p.a_sh | p.a_sw) & 7) == 0 && (long)(g.M >> 6) * p.a_sn + 7 * p.a_sh + 7 * p.a_sw + p.Kc < (1L << 31) &&
         (long)p.Nout * p.ldw < (1L << 31);
}
static bool s8_applicable(const NtParams& p) { return kLdsS8 <= device_max_lds() && s8_shape(p); }
static int launch_conv3x3_s8(NtParams& p, hipStream_t s) {
  constexpr int BM = 128;
  p.tiles_m = ceil_div(p.g.M, BM); p.tiles_n = 1; p.xa = p.xb = 0;
  p.kb_per_split = ceil_div(p.Kc / 64, p.splitk);
  dim3 grid((unsigned)p.tiles_m, (unsigned)p.splitk);
  { int rc = acc_scratch_fits(p, BM, p.Nout <= 32 ? 32 : 64, true); if (rc) return rc; }
  if (p.Nout <= 32) {
    const size_t lds = 2 * BM * 128 + 256 + 12 * 32 * 128 + 512 * 16;
    auto kern = conv3x3_s8n32_kernel;
    IPK_SET_LDS_ONCE(kern, lds);
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, p);
  } else {
    const size_t lds = 2 * BM * 128 + 256 + 12 * 64 * 128 + 512 * 16;
    auto kern = conv3x3_s8_kernel;
    IPK_SET_LDS_ONCE(kern, lds);
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, p);
  }
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

// Split count for the skinny 3x3 convolutions of the coupling nets (conv3 forward, conv1 data gradient) at M output rows
// and Kc input channels: callers size their partial-sum slabs with it.  0: the kernel does not apply (caller's choice).
extern "C" int ipoke_conv3x3_skinny_splitk(int M, int Kc, int dtype) {
  if (dtype != IPOKE_BF16 || Kc % 64 != 0 || Kc < 256 || M % 64 != 0) return 0;
  return conv3x3_s8_splits(M, Kc, kS8SamplesPerTile);
}

static thread_local int g_last_kernel = IPOKE_KERNEL_NONE;     // (see ipoke_last_conv_kernel)
static int conv_params(NtParams& p, const ipoke_conv_desc* d, int dtype);

// K splits of the fused conv3 + coupling launch: the largest power of two (4 .. 32) that keeps tiles x splits within one round of
// the 256 CUs (the owners of a tile's rows wait for their partners: a group must be resident as a whole)
static int coupling_splits(int M, int Kc) {
  const int tiles = ceil_div(M, 128), nchunks = Kc / 64;
  int want = 256 / tiles; if (want > nchunks) want = nchunks; if (want > 32) want = 32;
  int ns = 0;
  for (int c = 4; c <= want; c *= 2) ns = c;
  return ns;
}
extern "C" int ipoke_conv3x3_coupling_splitk(int M, int Kc, int dtype) {
  if (dtype != IPOKE_BF16 || Kc % 64 != 0 || Kc < 256 || M % 64 != 0 || M < 64) return 0;
  return coupling_splits(M, Kc);
}
extern "C" int64_t ipoke_conv3x3_coupling_xchg_bytes(void) { return kCplHeader + 256L * 128 * 256; }     // tiles x splits <= 256 slots of 128 rows x 64 floats
extern "C" int ipoke_conv3x3_coupling_xchg_init(void* xchg, void* stream) {
  IPK_REQUIRE(xchg != nullptr, "null scratch");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  IPK_HIP(hipMemsetAsync(xchg, 0xff, (size_t)ipoke_conv3x3_coupling_xchg_bytes(), s));
  IPK_HIP(hipMemsetAsync(xchg, 0, kCplHeader, s));
  return IPOKE_OK;
}
template <int NSPLIT>
static int launch_conv3x3_s8_coupling(NtParams& p, const CouplingEpi& e, hipStream_t s) {
  const size_t lds = kLdsS8;
  auto kern = conv3x3_s8_coupling_kernel<NSPLIT>;
  IPK_SET_LDS_ONCE(kern, lds);
  p.tiles_m = ceil_div(p.g.M, 128); p.tiles_n = 1; p.xa = p.xb = 0; p.splitk = NSPLIT;
  p.kb_per_split = ceil_div(p.Kc / 64, NSPLIT);
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * NSPLIT)), dim3(512), lds, s, p, e);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_conv3x3_coupling(const ipoke_conv_desc* conv, const ipoke_affine_desc* a, const ipoke_coupling_epi* ep, int B,
                                      int dtype, void* stream) {
  IPK_REQUIRE(conv && a && ep, "null descriptor");
  IPK_REQUIRE(dtype == IPOKE_BF16, "the fused conv3 + coupling launch is bf16 only");
  IPK_REQUIRE(ep->xchg != nullptr && ((uintptr_t)ep->xchg & 15) == 0, "exchange scratch missing (ipoke_conv3x3_coupling_xchg_bytes / _init)");
  ipoke_conv_desc d = *conv;
  d.C = ep->xchg; d.c_f32 = 1; d.ldc = 64; d.splitk = 1; d.c_accumulate = 0;       // (no partial-sum slabs: validation only)
  NtParams p;
  int rc = conv_params(p, &d, dtype); if (rc) return rc;
  IPK_REQUIRE(!d.bias && d.act == IPOKE_ACT_NONE && !d.dact && !d.row_scale && !d.w_kmajor, "conv3 of a coupling: raw sums only (the bias is the coupling's)");
  IPK_REQUIRE(s8_applicable(p) && p.g.M == 64 * B && !p.g.transposed, "not the skinny 3x3 convolution of a coupling net on 8x8 maps");
  IPK_REQUIRE(a->Cp >= 1 && 2 * a->Cp == d.Nout && a->t_stride >= 1 && a->P == 64 && a->ld >= 1 && a->ld <= 256 &&
              a->t_off >= 0 && a->t_off + (a->Cp - 1) * a->t_stride < a->ld, "bad coupling geometry");
  IPK_REQUIRE(ep->mode >= 0 && ep->mode <= 2 && ep->in, "bad mode / null input state");
  IPK_REQUIRE(ep->mode == 1 ? (ep->out2 && ep->out2 != ep->in && ep->an_C >= 1 && ep->an_c0 >= 0 && ep->an_c0 + ep->an_C <= a->ld &&
                               (ep->an_log_scale == nullptr) == (ep->an_bias == nullptr) && !ep->ext)
                            : (ep->out != nullptr), "bad outputs");
  IPK_REQUIRE(!ep->logdet_slot || ep->slot_stride >= 4, "log-det slots are 4 wide (one per 16-row slice of a sample)");
  IPK_REQUIRE(!ep->ext || ep->ext_ld >= a->Cp, "bad extra operand output");
  int ns = coupling_splits(p.g.M, p.Kc);
  {      // test hook (ipoke_set_dispatch_override "cpl_split"): the slices of ipoke_conv_pair_coupling at shapes the rule gives other counts
    const int ov = g_cpl_split.load(std::memory_order_relaxed);
    if (ov > 0 && (long)ceil_div(p.g.M, 128) * ov <= 256 && ov <= p.Kc / 64) ns = ov;
  }
  IPK_REQUIRE(ns >= 4, "too many row tiles for an in-launch exchange (ipoke_conv3x3_coupling_splitk == 0)");
  CouplingEpi e{};
  e.bias = a->bias; e.in = ep->in; e.out = ep->out; e.out2 = ep->mode == 1 ? ep->out2 : nullptr;
  e.scale_out = ep->mode == 2 ? nullptr : ep->scale_out; e.logdet_slot = ep->mode == 2 ? nullptr : ep->logdet_slot;
  e.an_ls = ep->an_log_scale; e.an_bias = ep->an_bias; e.an_idx = ep->an_idx; e.ext = ep->ext; e.xchg = ep->xchg;
  e.xchg_bytes = (int)ipoke_conv3x3_coupling_xchg_bytes(); e.slot_stride = ep->slot_stride < 1 ? 1 : ep->slot_stride;
  e.Cp = a->Cp; e.t_off = a->t_off; e.t_stride = a->t_stride; e.ld = a->ld; e.mode = ep->mode; e.an_c0 = ep->an_c0; e.an_C = ep->an_C;
  e.ext_ld = ep->ext_ld; e.ext_bf16 = 1;
  auto log2_or = [](int v) { int sh = 0; while ((1 << sh) < v) ++sh; return (1 << sh) == v ? sh : -1; };
  e.ld_sh = log2_or(a->ld); e.cp_sh = log2_or(a->Cp); e.ts_sh = log2_or(a->t_stride);
  p.prio = 2;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  g_last_kernel = IPOKE_KERNEL_S8;
  switch (ns) {
    case 4: return launch_conv3x3_s8_coupling<4>(p, e, s);
    case 8: return launch_conv3x3_s8_coupling<8>(p, e, s);
    case 16: return launch_conv3x3_s8_coupling<16>(p, e, s);
    default: return launch_conv3x3_s8_coupling<32>(p, e, s);
  }
}

// kernel family the calling thread's last ipoke_conv_forward was dispatched to (ipoke_last_conv_kernel: the parity tests assert that
// the benchmarked sizes reach the kernel they mean to check under the DEFAULT dispatch rule)

template <typename T>
static int dispatch_nt(NtParams& p, hipStream_t s) {
  // Tile choice: fill the 256 CUs with one wave of tiles when the problem allows it.
  const int M = p.g.M, N = p.Nout;
  g_last_kernel = IPOKE_KERNEL_IGEMM;
  if constexpr (sizeof(T) == 2) {
    if (s8_applicable(p)) { g_last_kernel = IPOKE_KERNEL_S8; return launch_conv3x3_s8(p, s); }
    if (k64_applicable(p)) { g_last_kernel = IPOKE_KERNEL_S8; return launch_conv3x3_k64(p, s); }      // (same family tag: stationary input on the 8x8 latent)
    if (k8_applicable(p)) { g_last_kernel = IPOKE_KERNEL_K8; return launch_conv3x3_k8(p, s); }
    if (c64_applicable(p)) { g_last_kernel = IPOKE_KERNEL_C64; return launch_conv3x3_c64(p, s); }
    if (halo16_applicable(p)) { g_last_kernel = IPOKE_KERNEL_HALO16; return launch_conv3x3_halo16(p, s); }
    if (halo_applicable(p)) { g_last_kernel = IPOKE_KERNEL_HALO; return launch_conv3x3_halo(p, s); }
  }
  if (!p.a_f32) {
    if (N <= 64) return launch_nt_glds<T, 4, 1, 1, 4, 4>(p, s);         // 64 x 64, skinny N
    // developer hook (ipoke_set_dispatch_override "nt128" = 2, scripts/probe_pair_coupling.py): EVERY wide N-major GEMM of the process on
    // the 128 x 128 tile with one K pass -- the tile and the K order of ipoke_conv_pair_coupling
    if (g_nt128_mode.load(std::memory_order_relaxed) == 2) return launch_nt_glds<T, 2, 4, 4, 2, 2, 2>(p, s);
    {
      // Row-tile height: the flow's GEMMs have M = 64*B rows (1280 at B = 20) and N = 2048, i.e. 160 tiles of 128 x 128 on
      // 256 CUs.  80- or 160-row tiles give exactly 256 workgroups at B = 20 / 40; pick the height with the least
      // (rounds of 256 workgroups) x (rows per workgroup), preferring taller tiles on a tie.
      const long tn128 = ceil_div(N, 128);
      int best = 128; long best_cost = ((long)ceil_div(M, 128) * tn128 + 255) / 256 * 128;
      if (M % 160 == 0) { const long c = ((long)(M / 160) * tn128 + 255) / 256 * 160; if (c <= best_cost) { best = 160; best_cost = c; } }
      if (M % 80 == 0) { const long c = ((long)(M / 80) * tn128 + 255) / 256 * 80; if (c < best_cost) { best = 80; best_cost = c; } }
      if ((long)ceil_div(M, 128) * tn128 >= 100) {
        // 80 x 128: two K-halves x 4 waves of 80 x 32, 3 slots.  Isolated 21.9-24 us at conv2 against 24.7 for 8 waves of
        // 80 x 16 (fewer fragment reads); inside the train step both measure the same (side-stream contention dominates),
        // and the 2 x 2-slot variant, faster still in isolation, is slower there (106 KB of LDS per workgroup).  Deeper
        // rings measure no faster: the operand stream alone (no math) runs at ~70 GB/s per CU.
        if (best == 80) return launch_nt_glds<T, 1, 4, 5, 2, 3, 1, 2>(p, s);
        if (best == 160) return launch_nt_glds<T, 2, 4, 5, 2, 2, 2>(p, s);         // 160 x 128, 8 waves
        return launch_nt_glds<T, 2, 4, 4, 2, 2, 2>(p, s);                          // 128 x 128, 8 waves
      }
    }
    return launch_nt_glds<T, 2, 2, 2, 2, 4>(p, s);
  }
  if (N <= 64) return launch_nt<T, 4, 1, 1, 4>(p, s);                  // 64 x 64 tiles, skinny N (split-K upstream)
  const long t128 = (long)ceil_div(M, 128) * ceil_div(N, 128);
  if (M % 80 == 0 && M % 128 != 0 && (long)(M / 80) * ceil_div(N, 128) <= 256 && t128 < 256)
    return launch_nt<T, 1, 4, 5, 2>(p, s);                            // 80 x 128 (e.g. M = 1280 -> 256 tiles)
  if (M % 160 == 0 && M % 128 != 0 && (long)(M / 160) * ceil_div(N, 128) >= 128)
    return launch_nt<T, 2, 2, 5, 4>(p, s);                            // 160 x 128 (e.g. M = 2560 -> 256 tiles)
  if (t128 < 128) return launch_nt<T, 2, 2, 2, 4>(p, s);              // 64 x 128: more tiles for small problems
  return launch_nt<T, 2, 2, 4, 4>(p, s);                              // 128 x 128
}

// =============================================================================================
// Weight gradient, LDS-DMA variant (bf16, dense operands): dW[n][k] = sum_m dY[m][n] * A[src(m, tap)][c].
// Both operands are reduced over their SLOW memory dimension (rows m), which is what made the register-staged kernel
// spend half its time loading, transposing (v_perm) and storing.  Here a stage of 64 rows of each operand goes
// global -> LDS untouched with global_load_lds_dwordx4 (row-major [m][128] images, NSTAGE-deep ring) and the transposed
// matrix-core fragments are read with ds_read_b64_tr_b16: for a 16-lane group whose lane j supplies the address of
// row j/4, columns 4*(j%4).. of a 4x16 block, lane i receives column i of the block (4 consecutive m) -- two reads give
// the 8 reduction elements of a 16x16x32 MFMA operand (semantics measured with scripts/exp/tr_probe.hip).
// The 16-byte source chunks of row r are permuted by p ^ 2*h(r), h(r) = (r & 3) | ((r >> 3) & 1) << 2, so that the eight
// rows one LDS cycle touches fall into different bank groups.
__device__ __forceinline__ int tn_swz(int row) { return 2 * ((row & 3) | (((row >> 3) & 1) << 2)); }

// The transposing reads are inline assembly, not __builtin_amdgcn_ds_read_tr16_b64: hipcc's wait-count insertion treats every
// LDS read with a memory operand as a possible reader of ALL LDS-DMA writes in flight and puts `s_waitcnt vmcnt(0)` in front of the
// first fragment read of an iteration -- the stage issued a few instructions earlier had to land before the stage already in
// LDS could be read, i.e. DMA and math ran one after the other (conv2 shape, one phase at a time: DMA alone
// 11.9 us, reads + matrix cores alone 13.2 us, epilogue 4.1 us, whole kernel 29.2 us = their sum).  The assembly reads carry no
// memory operand; the kernel waits for them itself (tn_wait_frags ties the registers to the s_waitcnt).
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 tn_tr4_t;
template <int IMM> __device__ __forceinline__ tn_tr4_t tn_ds_tr(unsigned addr) {
  tn_tr4_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(IMM) : "memory");
  return v;
}
template <typename F> __device__ __forceinline__ void tn_wait_frags(F (&f)[6]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5])::"memory");
}

// =============================================================================================
// igemm_nn: C[m][n] = sum_k A[m][k] * W[k][n] -- the weight given K-MAJOR, i.e. as the row-major [k][n] matrix (NtParams.w_kmajor).
// This is the data gradient of a 1x1 convolution read from the weight's STRAIGHT copy W[out][in] (reduction over `out`, its row index):
// with it the coupling nets' conv2 -- 73 % of the flow's parameters -- needs no transposed shadow, the optimizer writes the one bf16
// copy itself and `relayout` never touches those tensors.
// Same ring, tile shapes, K split and epilogue as igemm_nt_glds_kernel; the difference is the W operand: a K-block of 64 reduction rows x
// BN = 128 columns goes global -> LDS untouched as 64 rows of 256 bytes (16-byte source chunks permuted by tn_swz against bank conflicts,
// exactly the operand images of igemm_tn_glds_kernel) and the matrix-core fragments -- 8 consecutive k for one column per lane -- are
// read with the transposing ds_read_b64_tr_b16 (two per fragment; inline assembly, see tn_ds_tr).
template <int WM, int WN, int MREP, int NSTAGE, int WK>
__global__ __launch_bounds__(WM * WN * WK * 64) void igemm_nn_glds_kernel(const NtParams p) {
  kernarg_prefetch<(int)sizeof(NtParams)>();
  typedef bf16_t T;
  constexpr int NREP = 2, NTHR = WM * WN * WK * 64, NWAVE = NTHR / 64;
  constexpr int BM = WM * MREP * 16, BN = WN * NREP * 16;
  static_assert(BN == 128, "the W image is 64 rows x 256 bytes");
  constexpr int A_IT = (BM * 8 + NTHR - 1) / NTHR, B_IT = 1024 / NTHR, L = A_IT + B_IT;
  constexpr int SUB = BM * 128 + 64 * 256;        // one K-block (64 k) of both operands
  static_assert((NSTAGE - 2) * L <= 63 && 1024 % NTHR == 0, "vmcnt field / whole DMA instructions");
  typedef typename ET<T>::frag frag_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* dummy = smem + NSTAGE * SUB;                           // 1 KB per wave: landing zone of padding DMAs
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wk = wave / (WM * WN), wr = wave % (WM * WN);
  const int wm = wr / WN, wn = wr % WN;
  const GeomDev& g = p.g;
  int tm, tn;
  {
    const int bid = blockIdx.x;
    if (p.xa > 0) {
      const int xcd = bid & 7, q = bid >> 3;
      const FDiv fxa(p.xa), fxb(p.xb);                   // (powers of two: pick_xcd_map)
      const int sub_m = fxa.div(p.tiles_m), sub_n = fxb.div(p.tiles_n);
      const FDiv fsm(sub_m);
      tm = fxa.mod(xcd) * sub_m + fsm.mod(q);
      tn = fxa.div(xcd) * sub_n + fsm.div(q);
    } else {
      const FDiv ftm(p.tiles_m);
      tm = ftm.mod(bid); tn = ftm.div(bid);
    }
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int nkb = (p.Ktot + 63) >> 6;
  constexpr unsigned kInvalid = 0xffffffffu;
  // A chunks: row r of the tile = GEMM row m0 + r (a 1x1 convolution on dense channels-last rows: row m starts at m * a_sw)
  unsigned a_off[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int ch = tid + NTHR * i, row = ch >> 3, pos = ch & 7;
    a_off[i] = (row < BM && m0 + row < g.M) ? (unsigned)((long)(m0 + row) * p.a_sw + p.a_coff + ((pos ^ ((row >> 1) & 7)) * 8)) : kInvalid;
  }
  // W chunks: DMA instruction i of this wave fills image rows 4 * (wave + NWAVE * i) + lane / 16, chunk lane % 16 <- source chunk ^ swz(row)
  unsigned b_off[B_IT]; int b_row[B_IT];
#pragma unroll
  for (int i = 0; i < B_IT; ++i) {
    const int row = 4 * (wave + NWAVE * i) + (lane >> 4), col = n0 + (((lane & 15) ^ tn_swz(row)) * 8);
    b_row[i] = row;
    b_off[i] = col < p.Nout ? (unsigned)((long)row * p.ldw + col) : kInvalid;
  }
  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  int kb_issue = 0;
  auto issue_slot = [&](int slot) {
    unsigned char* sa = smem + slot * SUB;
    const bool real = kb_issue < nkb;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const T* src = (real && a_off[i] != kInvalid) ? Abase + a_off[i] : zero;
      unsigned char* dst = (real && (wave * 64 + NTHR * i) < BM * 8) ? sa + (wave * 64 + NTHR * i) * 16 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
      if (a_off[i] != kInvalid) a_off[i] += 64;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const T* src = (real && b_off[i] != kInvalid && kb_issue * 64 + b_row[i] < p.Ktot) ? Wbase + b_off[i] : zero;
      unsigned char* dst = real ? sa + BM * 128 + (wave + NWAVE * i) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
      if (b_off[i] != kInvalid) b_off[i] += (unsigned)(64 * p.ldw);
    }
    ++kb_issue;
  };

  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets inside a K-block.  A: as igemm_nt_glds (16-byte units XOR-swizzled by (row >> 1) & 7); k-step s = 32 k
  int a_rd[MREP][2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const int q = s2 * 4 + (lane >> 4);
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
      const int row = wm * MREP * 16 + i * 16 + (lane & 15);
      a_rd[i][s2] = row * 128 + ((q ^ ((row >> 1) & 7)) * 16);
    }
  }
  // W: lane (i16, grp) reads k rows 8 * grp + (i16 >> 2) (+ 4: second read) of k-step s, columns base + 4 * (i16 & 3) .. + 3
  const int i16 = lane & 15, grp = lane >> 4;
  const int rrow = 8 * grp + (i16 >> 2);
  const int hsw = tn_swz(rrow);                  // the same for row + 4 and row + 32
  const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)smem;
  unsigned b_rd[NREP];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int col = (wn * NREP + j) * 16 + 4 * (i16 & 3);
    b_rd[j] = lds0 + (unsigned)(BM * 128 + rrow * 256 + (((col >> 3) ^ hsw) * 16) + ((col >> 2) & 1) * 8);
  }
  auto read_b = [&](frag_t (&fb)[NREP], unsigned sb, int kstep) {
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const unsigned a = b_rd[j] + sb + (unsigned)(kstep * 32 * 256);
      const tn_tr4_t lo = tn_ds_tr<0>(a), hi = tn_ds_tr<4 * 256>(a);
#pragma unroll
      for (int e = 0; e < 4; ++e) { fb[j][e] = lo[e]; fb[j][4 + e] = hi[e]; }
    }
  };
  auto wait_b = [&](frag_t (&fb)[NREP]) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[0]), "+v"(fb[1])::"memory"); };

#pragma unroll
  for (int s2 = 0; s2 < NSTAGE - 1; ++s2) issue_slot(s2);
  int slot = 0;
  for (int kb = 0; kb < nkb; ++kb) {
    wait_vmcnt<(NSTAGE - 2) * L>();               // this wave's share of the oldest slot has landed
    __builtin_amdgcn_s_barrier();                 // ... and everybody else's; all reads of the slot refilled below are done
    issue_slot((slot + NSTAGE - 1) % NSTAGE);
    const unsigned char* base = smem + slot * SUB;
    const unsigned sb = (unsigned)(slot * SUB);
    slot = (slot + 1) % NSTAGE;
    if constexpr (WK == 2) {                      // this wave group owns k-step `wk` of every K-block
      frag_t fa[MREP], fb[NREP];
      read_b(fb, sb, wk);
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[i] = *reinterpret_cast<const frag_t*>(base + (wk ? a_rd[i][1] : a_rd[i][0]));
      wait_b(fb);
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) mma64(fa[i], fb[j], acc[i][j]);
    } else {
      frag_t fa[2][MREP], fb[2][NREP];
      read_b(fb[0], sb, 0);
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[0][i] = *reinterpret_cast<const frag_t*>(base + a_rd[i][0]);
      wait_b(fb[0]);
      read_b(fb[1], sb, 1);                       // the second k-step's fragments travel under the first one's MFMAs
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[1][i] = *reinterpret_cast<const frag_t*>(base + a_rd[i][1]);
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) mma64(fa[0][i], fb[0][j], acc[i][j]);
      wait_b(fb[1]);
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) mma64(fa[1][i], fb[1][j], acc[i][j]);
    }
  }
  wait_vmcnt<0>();
  if constexpr (WK > 1) {                  // the two K halves meet: group 1 hands its partial sums to group 0 through LDS
    constexpr int EP = BN * 4 + 16;
    unsigned char* st2 = smem + BM * EP + (wm * MREP * 16 + (lane & 15)) * EP + (wn * NREP * 16 + (lane >> 4) * 4) * 4;
    __syncthreads();
    if (wk == 1) {
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(st2 + i * 16 * EP + j * 64) = acc[i][j];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) acc[i][j] += *reinterpret_cast<const f32x4*>(st2 + i * 16 * EP + j * 64);
    }
  }
  nt_epilogue<T, WM, WN, MREP, NREP, NTHR>(p, acc, smem, m0, n0, wm, wn, 0, wk == 0);
}

template <int WM, int WN, int MREP, int NSTAGE, int WK>
static int launch_nn_glds(NtParams& p, hipStream_t s) {
  constexpr int BM = WM * MREP * 16, BN = WN * 2 * 16;
  p.tiles_m = ceil_div(p.g.M, BM);
  p.tiles_n = ceil_div(p.Nout, BN);
  p.splitk = 1; p.kb_per_split = ceil_div(p.Ktot, 64);
  pick_xcd_map(p);
  size_t lds = (size_t)NSTAGE * (BM * 128 + 64 * 256) + WM * WN * WK * 64 * 16;
  if (lds < (size_t)WK * BM * (BN * 4 + 16)) lds = (size_t)WK * BM * (BN * 4 + 16);      // epilogue staging (+ the K halves' hand-over)
  auto kern = igemm_nn_glds_kernel<WM, WN, MREP, NSTAGE, WK>;
  IPK_SET_LDS_ONCE(kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)p.tiles_m * p.tiles_n)), dim3(WM * WN * WK * 64), lds, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
// K-major weights (w_kmajor): 1x1 kernels over dense bf16 rows
static int dispatch_nn(NtParams& p, hipStream_t s) {
  const GeomDev& g = p.g;
  IPK_REQUIRE(g.taps == 1 && !g.transposed && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 && g.ph == 0 && g.pw == 0 && !p.a_f32 &&
              p.Kc == p.Kc_real && p.Kc % 64 == 0 && (p.a_coff & 7) == 0 && (p.a_sw & 7) == 0 && (p.ldw & 7) == 0 && p.ldw >= p.Nout &&
              p.splitk == 1 && !p.c_scatter && p.a_sh == (long)g.Wi * p.a_sw && p.a_sn == (long)g.Hi * g.Wi * p.a_sw &&
              (long)g.M * p.a_sw + p.Kc < (1L << 31) && (long)p.Ktot * p.ldw < (1L << 31),
              "K-major weights: 1x1 kernel over dense bf16 channels-last rows, K a multiple of 64");
  const int M = g.M;
  const long tn128 = ceil_div(p.Nout, 128);
  int best = 128; long best_cost = ((long)ceil_div(M, 128) * tn128 + 255) / 256 * 128;
  if (M % 160 == 0) { const long c = ((long)(M / 160) * tn128 + 255) / 256 * 160; if (c <= best_cost) { best = 160; best_cost = c; } }
  if (M % 80 == 0) { const long c = ((long)(M / 80) * tn128 + 255) / 256 * 80; if (c < best_cost) { best = 80; best_cost = c; } }
  // developer hook (ipoke_set_dispatch_override "nn128" = 2, scripts/probe_pair_dgrad.py): EVERY K-major GEMM of the process on the 128 x 128 tile
  if (g_nn128_mode.load(std::memory_order_relaxed) == 2) best = 128;
  if (best == 80) return launch_nn_glds<1, 4, 5, 3, 2>(p, s);       // 80 x 128: two K halves x 4 waves of 80 x 32 (the c2 shape: 256 workgroups)
  if (best == 160) return launch_nn_glds<2, 4, 5, 3, 1>(p, s);      // 160 x 128, 8 waves of 80 x 32
  return launch_nn_glds<2, 4, 4, 3, 1>(p, s);                       // 128 x 128
}

// =============================================================================================
// The conv2 AND conv1 data gradients of a coupling net as one launch (ipoke_conv_pair_dgrad).
// conv1's data gradient -- the skinny transposed 3x3 convolution conv3x3_s8n32_kernel runs as 16 K slices of two 64-channel chunks --
// is a split-K reduction over the hidden channels, and a slice of 128 channels is exactly one 128-column N tile of conv2's GEMM.  A
// workgroup that owns the [128 rows (two samples) x 128 columns] tile of dp1 therefore holds, after its epilogue, the whole input
// image of one slice: it leaves the bf16 values in LDS as the two chunk images of conv3x3_s8_body (same swizzle, same zero row), runs
// that slice's 18 K-blocks against the matching slab of the conv1 filter operand and accumulates through the deterministic scratch
// path of nt_epilogue (slab = N tile, last arriver of a row tile sums in the fixed order).  No spin, no flag: the ticket is the only
// cross-workgroup mechanism.  Per coupling one chain launch, the L2 -> LDS re-read of dp1 and the skinny kernel's ramp disappear.
// The GEMM main loop is igemm_nn_glds_kernel<2, 4, 4, 3, 1>'s; the K-block loop, the hand-over of the four K groups and the
// accumulation are conv3x3_s8_body<0, 2>'s (a copy with the input image taken from LDS: the shipped skinny kernels keep their code),
// in the same order -- the results equal the two launches bit for bit when the skinny one runs hidden / 128 slices.
struct PairEpi {
  const void* W1; int ldw1, cin, transposed;      // conv1's filter operand [cin][9 * hidden] (tap-major), its output columns
  float* C2; long ldc2; int c_coff2, c_cstride2;  // the fp32 accumulation target
  unsigned* acc_cnt; float* acc_part;             // ipoke_conv_desc.acc_scratch
};
// LDS: GEMM ring [0, 96 KB) -- afterwards the fp32 staging tile [0, 66 KB) and the two chunk images + zero row [66 KB, 98.25 KB) --,
// the filter ring (12 K-blocks of 32 rows) at 100 KB and 1 KB per wave for padding DMAs at 148 KB
static constexpr int kPairImg = 128 * (128 * 4 + 16), kPairZrow = kPairImg + 2 * 128 * 128, kPairRing = 100 * 1024,
                     kPairDummy = kPairRing + 12 * 32 * 128;
static constexpr size_t kLdsPair = kPairDummy + 8 * 1024;
static_assert(kPairZrow + 256 <= kPairRing && 3 * (128 * 128 + 64 * 256) <= kPairRing, "LDS regions of igemm_nn_pair_kernel overlap");

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void igemm_nn_pair_kernel(const NtParams p, const PairEpi e) {
  kernarg_prefetch<(int)(sizeof(NtParams) + sizeof(PairEpi)) < 512 ? (int)(sizeof(NtParams) + sizeof(PairEpi)) : 512>();
  typedef bf16_t T;
  typedef typename ET<T>::frag frag_t;
  typedef typename Pack4<T>::type pack_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int WM = 2, WN = 4, MREP = 4, NREP = 2, NSTAGE = 3, NTHR = 512, NWAVE = 8, BM = 128, BN = 128;
  constexpr int A_IT = BM * 8 / NTHR, B_IT = 1024 / NTHR, L = A_IT + B_IT;
  constexpr int SUB = BM * 128 + 64 * 256;
  constexpr int EP = BN * 4 + 16;
  constexpr int R = 12, WSLOT = 32 * 128, WJ = 2, ABUF = BM * 128;      // the filter ring of conv3x3_s8_body<0, 2>
  constexpr int NKB = 18, NROUNDS = 5;                                  // 2 chunks x 9 taps, four K-blocks per round
  constexpr unsigned kInvalid = 0xffffffffu;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* img = smem + kPairImg;
  unsigned char* zrow = smem + kPairZrow;
  unsigned char* ring = smem + kPairRing;
  unsigned char* dummy = smem + kPairDummy;
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const GeomDev& g = p.g;
  int tm, tn;
  {
    const int bid = blockIdx.x;
    if (p.xa > 0) {
      const int xcd = bid & 7, q = bid >> 3;
      const FDiv fxa(p.xa), fxb(p.xb);                   // (powers of two: pick_xcd_map)
      const int sub_m = fxa.div(p.tiles_m), sub_n = fxb.div(p.tiles_n);
      const FDiv fsm(sub_m);
      tm = fxa.mod(xcd) * sub_m + fsm.mod(q);
      tn = fxa.div(xcd) * sub_n + fsm.div(q);
    } else {
      const FDiv ftm(p.tiles_m);
      tm = ftm.mod(bid); tn = ftm.div(bid);
    }
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int hid = p.Nout;                                // conv1's input channels = the GEMM's columns
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  if (tid < 16) reinterpret_cast<f32x4*>(zrow)[tid] = f32x4{0.f, 0.f, 0.f, 0.f};      // (outside every ring: first read after many barriers)

  // ---- conv1 filter slab of this slice: wave w brings rows 16 * (w >> 2) .. + 15 (2 instructions of 8 rows) of K-block 4r + (w & 3);
  // the first two rounds are requested NOW (they are the oldest requests: the GEMM loop's counted waits cover them)
  const T* W1 = reinterpret_cast<const T*>(e.W1);
  unsigned w_src[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    const int n = 8 * WJ * (wave >> 2) + 8 * j + (lane >> 3), pos = lane & 7;
    w_src[j] = n < e.cin ? (unsigned)((long)n * e.ldw1 + n0 + ((pos ^ ((n >> 1) & 7)) * 8)) : kInvalid;
  }
  int wi_g = wave & 3, wi_c = 0, wi_t = wave & 3;          // K-block index / (chunk, tap) of this wave's next filter request
  auto issue_w = [&]() {
    const bool in = wi_g < NKB;
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      const bool real = in && w_src[j] != kInvalid;
      const T* src = real ? W1 + w_src[j] + (long)wi_t * hid + wi_c * 64 : zero;
      unsigned char* dst = in ? ring + (wi_g % R) * WSLOT + (WJ * (wave >> 2) + j) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    wi_g += 4; wi_t += 4;
    if (wi_t >= 9) { wi_t -= 9; ++wi_c; }
  };
  issue_w(); issue_w();

  // ---- conv2 data gradient: the main loop of igemm_nn_glds_kernel<2, 4, 4, 3, 1>
  const int nkb = (p.Ktot + 63) >> 6;
  unsigned a_off[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int ch = tid + NTHR * i, row = ch >> 3, pos = ch & 7;
    a_off[i] = (m0 + row < g.M) ? (unsigned)((long)(m0 + row) * p.a_sw + p.a_coff + ((pos ^ ((row >> 1) & 7)) * 8)) : kInvalid;
  }
  unsigned b_off[B_IT]; int b_row[B_IT];
#pragma unroll
  for (int i = 0; i < B_IT; ++i) {
    const int row = 4 * (wave + NWAVE * i) + (lane >> 4), col = n0 + (((lane & 15) ^ tn_swz(row)) * 8);
    b_row[i] = row;
    b_off[i] = col < p.Nout ? (unsigned)((long)row * p.ldw + col) : kInvalid;
  }
  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  int kb_issue = 0;
  auto issue_slot = [&](int slot) {
    unsigned char* sa = smem + slot * SUB;
    const bool real = kb_issue < nkb;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const T* src = (real && a_off[i] != kInvalid) ? Abase + a_off[i] : zero;
      unsigned char* dst = real ? sa + (wave * 64 + NTHR * i) * 16 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
      if (a_off[i] != kInvalid) a_off[i] += 64;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const T* src = (real && b_off[i] != kInvalid && kb_issue * 64 + b_row[i] < p.Ktot) ? Wbase + b_off[i] : zero;
      unsigned char* dst = real ? sa + BM * 128 + (wave + NWAVE * i) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
      if (b_off[i] != kInvalid) b_off[i] += (unsigned)(64 * p.ldw);
    }
    ++kb_issue;
  };
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    int a_rd[MREP][2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int q = s2 * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < MREP; ++i) {
        const int row = wm * MREP * 16 + i * 16 + (lane & 15);
        a_rd[i][s2] = row * 128 + ((q ^ ((row >> 1) & 7)) * 16);
      }
    }
    const int i16 = lane & 15, grp = lane >> 4;
    const int rrow = 8 * grp + (i16 >> 2);
    const int hsw = tn_swz(rrow);
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)smem;
    unsigned b_rd[NREP];
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const int col = (wn * NREP + j) * 16 + 4 * (i16 & 3);
      b_rd[j] = lds0 + (unsigned)(BM * 128 + rrow * 256 + (((col >> 3) ^ hsw) * 16) + ((col >> 2) & 1) * 8);
    }
    auto read_b = [&](frag_t (&fb)[NREP], unsigned sb, int kstep) {
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        const unsigned a = b_rd[j] + sb + (unsigned)(kstep * 32 * 256);
        const tn_tr4_t lo = tn_ds_tr<0>(a), hi = tn_ds_tr<4 * 256>(a);
#pragma unroll
        for (int q = 0; q < 4; ++q) { fb[j][q] = lo[q]; fb[j][4 + q] = hi[q]; }
      }
    };
    auto wait_b = [&](frag_t (&fb)[NREP]) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[0]), "+v"(fb[1])::"memory"); };
#pragma unroll
    for (int s2 = 0; s2 < NSTAGE - 1; ++s2) issue_slot(s2);
    int slot = 0;
    for (int kb = 0; kb < nkb; ++kb) {
      wait_vmcnt<(NSTAGE - 2) * L>();
      __builtin_amdgcn_s_barrier();
      issue_slot((slot + NSTAGE - 1) % NSTAGE);
      const unsigned char* base = smem + slot * SUB;
      const unsigned sb = (unsigned)(slot * SUB);
      slot = (slot + 1) % NSTAGE;
      frag_t fa[2][MREP], fb[2][NREP];
      read_b(fb[0], sb, 0);
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[0][i] = *reinterpret_cast<const frag_t*>(base + a_rd[i][0]);
      wait_b(fb[0]);
      read_b(fb[1], sb, 1);
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[1][i] = *reinterpret_cast<const frag_t*>(base + a_rd[i][1]);
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) mma64(fa[0][i], fb[0][j], acc[i][j]);
      wait_b(fb[1]);
#pragma unroll
      for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) mma64(fa[1][i], fb[1][j], acc[i][j]);
    }
  }
  wait_vmcnt<0>();

  // ---- dp1 = bf16(acc * ELU'(h1)): the arithmetic of nt_epilogue's dense path.  A thread owns one 4-column group in 8 rows; the values
  // go into the chunk images (column c of the tile = channel c & 63 of chunk c >> 6, 16-byte units swizzled by (row >> 1) & 7) and
  // stay in registers for the store to C, which is issued behind the convolution's K loop (nothing in that loop waits for it)
  constexpr int G4F = BN / 4, ITER = BM * G4F / NTHR, RSTEP = NTHR / G4F;
  const int c4 = tid % G4F, r0 = tid / G4F;
  const bool mask = p.dact != nullptr;
  pack_t dy[ITER], o[ITER];
#pragma unroll
  for (int k = 0; k < ITER; ++k) dy[k] = pack_t{};
  if (mask) {      // (rows beyond M: the index is clamped, no branch around a load; their sums are zero)
#pragma unroll
    for (int k = 0; k < ITER; ++k) {
      const int m = min(m0 + r0 + k * RSTEP, g.M - 1);
      dy[k] = *reinterpret_cast<const pack_t*>(reinterpret_cast<const T*>(p.dact) + (long)m * p.ld_dact + n0 + 4 * c4);
    }
  }
  auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  lds_barrier();                     // the GEMM ring is dead
  {
    unsigned char* base = smem + (wm * MREP * 16 + (lane & 15)) * EP + (wn * NREP * 16 + (lane >> 4) * 4) * 4;
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
      for (int j = 0; j < NREP; ++j) *reinterpret_cast<f32x4*>(base + i * 16 * EP + j * 64) = acc[i][j];
  }
  __syncthreads();                   // (also: the derivative-mask loads have landed)
  {
    const unsigned char* sp = smem + r0 * EP + c4 * 16;
    const int pos = (c4 & 15) >> 1;
#pragma unroll
    for (int k = 0; k < ITER; ++k) {
      const int row = r0 + k * RSTEP;
      const f32x4 v = *reinterpret_cast<const f32x4*>(sp + k * RSTEP * EP);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = v[r];
        const float y = ET<T>::to_f32(dy[k][r]);
        x *= (mask && y <= 0.f) ? y + 1.f : 1.f;
        o[k][r] = ET<T>::from_f32(m0 + row < g.M ? x : 0.f);
      }
      *reinterpret_cast<pack_t*>(img + (c4 >> 4) * ABUF + row * 128 + ((pos ^ ((row >> 1) & 7)) * 16) + (c4 & 1) * 8) = o[k];
    }
  }

  // ---- conv1 data gradient of this slice: the K-block loop of conv3x3_s8_body<0, 2> (2 row halves x 4 K groups, chunk-major, nine
  // taps inside) on the images above
  constexpr int CREP = 2;            // 32 output columns
  const int mh = wave & 1, kq = wave >> 1;
  const int sgn = e.transposed ? -1 : 1;
  unsigned vmask[MREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i) {
    const int r = i * 16 + (lane & 15);
    const int y = (r >> 3) & 7, x = r & 7;
    unsigned vm = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = y + sgn * (t / 3 - 1), xx = x + sgn * (t % 3 - 1);
      if ((unsigned)yy < 8u && (unsigned)xx < 8u) vm |= 1u << t;
    }
    vmask[i] = vm;
  }
  const int qlo = lane >> 4;
  int w_rd[CREP];
#pragma unroll
  for (int j = 0; j < CREP; ++j) {
    const int n = j * 16 + (lane & 15);
    w_rd[j] = n * 128 + ((qlo ^ ((n >> 1) & 7)) * 16);
  }
  f32x4 acc2[MREP][CREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < CREP; ++j) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int gk = kq, ci = 0, t = kq;
  for (int r = 0; r < NROUNDS; ++r) {
    wait_vmcnt<WJ>();                // everything but this wave's share of round r + 1 has landed
    lds_barrier();                   // (round 0: the images are complete)
    issue_w();                       // round r + 2 into the slots of round r - 1
    if (gk < NKB) {
      const unsigned char* ab = img + ci * ABUF + mh * 64 * 128;
      const unsigned char* wb = ring + (gk % R) * WSLOT;
      const int th = t / 3, tw = t - 3 * th;
      const int shift = sgn * ((th - 1) * 8 + (tw - 1));
      const unsigned char* arow[MREP]; int aswz[MREP];
#pragma unroll
      for (int i = 0; i < MREP; ++i) {
        const bool ok = (vmask[i] >> t) & 1u;
        const int sr = i * 16 + (lane & 15) + shift;
        arow[i] = ok ? ab + sr * 128 : zrow;
        aswz[i] = ok ? (sr >> 1) & 7 : 0;
      }
      frag_t fa[2][MREP], fb[2][CREP];
#pragma unroll
      for (int hs = 0; hs < 2; ++hs) {
#pragma unroll
        for (int i = 0; i < MREP; ++i) fa[hs][i] = *reinterpret_cast<const frag_t*>(arow[i] + (((hs * 4 + qlo) ^ aswz[i]) * 16));
#pragma unroll
        for (int j = 0; j < CREP; ++j) fb[hs][j] = *reinterpret_cast<const frag_t*>(wb + (w_rd[j] ^ (hs * 64)));
      }
#pragma unroll
      for (int hs = 0; hs < 2; ++hs)
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < CREP; ++j) mma64(fa[hs][i], fb[hs][j], acc2[i][j]);
      // (issue order as in conv3x3_s8_body: the first half-step's fragments, then one read of the second per MFMA of the first)
      constexpr int NF = MREP + CREP, NM = MREP * CREP, PER = NM / NF;
      __builtin_amdgcn_sched_group_barrier(0x100, NF, 0);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM - NF * PER, 0);
    }
    gk += 4; t += 4;
    if (t >= 9) { t -= 9; ++ci; }
  }
  wait_vmcnt<0>();
  if (c4 * 4 + n0 < p.Nout) {        // dp1 to C (the conv1 weight gradient reads it)
    T* Cp = reinterpret_cast<T*>(p.C) + (long)(m0 + r0) * p.ldc + p.c_coff + n0 + 4 * c4;
#pragma unroll
    for (int k = 0; k < ITER; ++k)
      if (m0 + r0 + k * RSTEP < g.M) *reinterpret_cast<pack_t*>(Cp + (long)k * RSTEP * p.ldc) = o[k];
  }
  // the four K groups meet: groups 2, 3 hand over to groups 0, 1, then group 1 to group 0 (nt_epilogue's staging layout)
  constexpr int EP2 = 16 * CREP * 4 + 16;
  {
    unsigned char* st = smem + (mh * MREP * 16 + (lane & 15)) * EP2 + (lane >> 4) * 16;
    lds_barrier();                   // the ring and the images are dead
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int give_lo = round == 0 ? 2 : 1, take_hi = round == 0 ? 2 : 1;
      if (kq >= give_lo && kq < 2 * give_lo) {
        unsigned char* d = st + (kq - give_lo) * BM * EP2;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < CREP; ++j) *reinterpret_cast<f32x4*>(d + i * 16 * EP2 + j * 64) = acc2[i][j];
      }
      lds_barrier();
      if (kq < take_hi) {
        const unsigned char* d = st + kq * BM * EP2;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < CREP; ++j) acc2[i][j] += *reinterpret_cast<const f32x4*>(d + i * 16 * EP2 + j * 64);
      }
      if (round == 0) lds_barrier();
    }
  }
  // slab [row tile][N tile], ticket, fixed-order sum by the last arriver, one read-modify-write into C2: nt_epilogue's DET branch
  NtParams q = p;
  q.splitk = p.tiles_n; q.tiles_n = 1; q.c_acc = 1; q.c_f32 = 1; q.acc_cnt = e.acc_cnt; q.acc_part = e.acc_part;
  q.C = e.C2; q.ldc = e.ldc2; q.c_coff = e.c_coff2; q.c_cstride = e.c_cstride2; q.Nout = e.cin;
  nt_epilogue<T, 2, 1, MREP, CREP, NTHR, true>(q, acc2, smem, m0, 0, mh, 0, tn, kq == 0);
}

// =============================================================================================
// conv2 (+ bias, ELU), conv3 AND the coupling transform of a coupling net as one launch (ipoke_conv_pair_coupling): the forward
// counterpart of igemm_nn_pair_kernel.  conv3 -- the skinny 3x3 convolution conv3x3_s8_coupling_kernel runs as hidden / 128 K slices of
// two 64-channel chunks -- is a split-K reduction over the hidden channels, and a slice is exactly one 128-column N tile of conv2's
// GEMM: the workgroup that owns the [128 rows (two samples) x 128 columns] tile of h2 holds, after bias + ELU, the whole input image
// of slice z = its N tile.  It writes the bf16 values from its accumulators straight into the two chunk images of conv3x3_s8_body
// (same swizzle, same zero row; no fp32 staging tile), runs the slice's 18 K-blocks against the matching slab of conv3's filter
// operand and joins the reduce-scatter + coupling of CouplingTail -- the very code of the two-launch form, with its exchange scratch,
// sentinels and bounded spins: no new hand-off.  Per coupling one chain launch, the L2 -> LDS re-read of h2 and the skinny kernel's
// ramp disappear; with C == NULL (the reverse pass: nothing reads h2 afterwards) so does the store of h2.
// Block order: slice z is the FAST index of the 1-D grid (block = tile * NSPLIT + z), so the NSPLIT partners of a row tile are adjacent
// in dispatch order and a partly resident grid finishes tile by tile (the progress argument of CouplingTail::run).
// The GEMM main loop is igemm_nt_glds_kernel's (W read N-major) on the 128 x 128 tile of igemm_nn_pair_kernel, one K pass, 3 slots;
// the K-block loop of the convolution is conv3x3_s8_body's (chunk-major, nine taps inside, K group kq takes every fourth block) -- the
// results equal ipoke_conv_forward on the 128 x 128 tile followed by ipoke_conv3x3_coupling at hidden / 128 slices bit for bit.
//
// LDS (137.25 KB): the filter ring keeps its three rounds of four 8 KB K-blocks, but only round 0 has a region of its own -- rounds 1
// and 2 are requested INTO THE GEMM SLOTS AS THEY RETIRE (in place of the padding DMAs of the last two GEMM iterations: same number of
// DMA instructions per wave, the counted waits do not change), the chunk images take the slot of the last K-block, rounds 3 and 4
// follow rounds 0 and 1.  The parked tiles of CouplingTail::run (4 x 128 x 272 B from offset 0) fit underneath.
struct NtCplEpi { const void* W3; int ldw3, nout3; };      // conv3's filter operand [nout3][9 * hidden] (tap-major) and its output columns
static constexpr int kCplSub = 2 * 128 * 128, kCplF = 3 * kCplSub, kCplZrow = kCplF + 4 * 64 * 128, kCplDummy = kCplZrow + 256;
static constexpr int kCplBias = kCplDummy + 8 * 1024;      // conv2's 128 bias values of this N tile (1 KB: one DMA instruction)
static constexpr size_t kLdsNtCpl = kCplBias + 1024;
static_assert(kCplSub == 4 * 64 * 128 && kCplSub == 2 * 128 * 128, "a GEMM slot holds one filter round or the two chunk images");
static_assert(4 * 128 * (64 * 4 + 16) <= kLdsNtCpl, "the parked tiles of CouplingTail::run");
static_assert(kLdsNtCpl <= 160 * 1024, "LDS per workgroup");

template <int NSPLIT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void igemm_nt_coupling_kernel(const NtParams p, const NtCplEpi q3, const CouplingEpi e) {
  kernarg_prefetch<(int)(sizeof(NtParams) + sizeof(NtCplEpi) + sizeof(CouplingEpi)) < 512 ? (int)(sizeof(NtParams) + sizeof(NtCplEpi) + sizeof(CouplingEpi)) : 512>();
  typedef bf16_t T;
  typedef typename ET<T>::frag frag_t;
  typedef typename Pack4<T>::type pack_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int WN = 4, MREP = 4, NREP = 2, NSTAGE = 3, NTHR = 512, BM = 128, BN = 128;
  constexpr int A_IT = BM * 8 / NTHR, B_IT = BN * 8 / NTHR, L = A_IT + B_IT;
  constexpr int SUB = kCplSub;
  constexpr int CREP = 4, WSLOT = 64 * 128, WJ = 4, ABUF = BM * 128;    // the filter K-blocks and the input images of conv3x3_s8_body<NSPLIT>
  constexpr int NKB = 18, NROUNDS = 5;                                  // 2 chunks x 9 taps, four K-blocks per round
  static_assert(L == WJ, "a filter round takes the place of a GEMM slot's DMA instructions");
  constexpr unsigned kInvalid = 0xffffffffu;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* zrow = smem + kCplZrow;
  unsigned char* dummy = smem + kCplDummy;
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1); else if (p.prio == 2) __builtin_amdgcn_s_setprio(2); else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const GeomDev& g = p.g;
  const int tile = blockIdx.x / NSPLIT, z = blockIdx.x % NSPLIT;
  const int m0 = tile * BM, n0 = z * BN;
  const int hid = p.Nout;                                // conv3's input channels = the GEMM's columns
  const int nkb = p.Ktot >> 6;
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  if (tid < 16) reinterpret_cast<f32x4*>(zrow)[tid] = f32x4{0.f, 0.f, 0.f, 0.f};      // (outside every ring: first read after many barriers)
  // where the filter rounds and the images go: round r in region r % 3
  const int reg1 = (nkb % NSTAGE) * SUB, reg2 = ((nkb + 1) % NSTAGE) * SUB;
  unsigned char* img = smem + ((nkb + NSTAGE - 1) % NSTAGE) * SUB;

  // ---- what the epilogue and the coupling need from global memory is requested first (the oldest requests of the launch)
  // conv2's bias goes through LDS (every wave requests the same 128 floats; no bias: zeros): a register loaded here would make the
  // epilogue wait for every DMA in flight behind the GEMM loop
  {
    const void* src = (p.bias && lane < BN / 4) ? static_cast<const void*>(p.bias + n0 + 4 * lane) : static_cast<const void*>(zero);
    __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(smem + kCplBias), 16, 0, 0);
  }
  CouplingTail<NSPLIT> ct(e);
  ct.prefetch(g.M, m0, z);

  // ---- conv3 filter slab of this slice: wave w brings rows 32 * (w >> 2) .. + 31 (4 instructions of 8 rows) of K-block 4r + (w & 3)
  const T* W3 = reinterpret_cast<const T*>(q3.W3);
  unsigned w_src[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    const int n = 8 * WJ * (wave >> 2) + 8 * j + (lane >> 3), pos = lane & 7;
    w_src[j] = n < q3.nout3 ? (unsigned)((long)n * q3.ldw3 + n0 + ((pos ^ ((n >> 1) & 7)) * 8)) : kInvalid;
  }
  int wi_g = wave & 3, wi_c = 0, wi_t = wave & 3;          // K-block index / (chunk, tap) of this wave's next filter request
  int wi_reg = kCplF, wi_r3 = 0;                           // region of that round
  auto issue_w = [&]() {
    const bool in = wi_g < NKB;
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      const bool real = in && w_src[j] != kInvalid;
      const T* src = real ? W3 + w_src[j] + (long)wi_t * hid + wi_c * 64 : zero;
      unsigned char* dst = in ? smem + wi_reg + (wi_g & 3) * WSLOT + (WJ * (wave >> 2) + j) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
    wi_g += 4; wi_t += 4;
    if (wi_t >= 9) { wi_t -= 9; ++wi_c; }
    wi_r3 = wi_r3 == 2 ? 0 : wi_r3 + 1;
    wi_reg = wi_r3 == 0 ? kCplF : (wi_r3 == 1 ? reg1 : reg2);
  };
  issue_w();                                               // round 0

  // ---- conv2: the main loop of igemm_nt_glds_kernel on the 128 x 128 tile, one K pass
  unsigned a_off[A_IT], b_off[B_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int ch = tid + NTHR * i, row = ch >> 3, pos = ch & 7;
    a_off[i] = (m0 + row < g.M) ? (unsigned)((long)(m0 + row) * p.a_sw + p.a_coff + ((pos ^ ((row >> 1) & 7)) * 8)) : kInvalid;
  }
#pragma unroll
  for (int i = 0; i < B_IT; ++i) {
    const int ch = tid + NTHR * i, row = ch >> 3, pos = ch & 7;
    b_off[i] = (unsigned)((long)(n0 + row) * p.ldw + ((pos ^ ((row >> 1) & 7)) * 8));
  }
  const T* Abase = reinterpret_cast<const T*>(p.A);
  const T* Wbase = reinterpret_cast<const T*>(p.W);
  int kb_issue = 0;
  auto issue_slot = [&](int slot) {
    if (kb_issue < nkb) {
      unsigned char* sa = smem + slot * SUB;
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        const T* src = a_off[i] != kInvalid ? Abase + a_off[i] : zero;
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(sa + (wave * 64 + NTHR * i) * 16), 16, 0, 0);
        if (a_off[i] != kInvalid) a_off[i] += 64;
      }
#pragma unroll
      for (int i = 0; i < B_IT; ++i) {
        __builtin_amdgcn_global_load_lds((glb_void*)(Wbase + b_off[i]), (lds_void*)(sa + BM * 128 + (wave * 64 + NTHR * i) * 16), 16, 0, 0);
        b_off[i] += 64;
      }
    } else {
      issue_w();             // filter rounds 1 and 2 into the slots of K-blocks nkb - 3 and nkb - 2 (read before the barrier just passed)
    }
    ++kb_issue;
  };
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    int a_rd[MREP][2], b_rd[NREP][2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int qq = s2 * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < MREP; ++i) {
        const int row = wm * MREP * 16 + i * 16 + (lane & 15);
        a_rd[i][s2] = row * 128 + ((qq ^ ((row >> 1) & 7)) * 16);
      }
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        const int row = wn * NREP * 16 + j * 16 + (lane & 15);
        b_rd[j][s2] = BM * 128 + row * 128 + ((qq ^ ((row >> 1) & 7)) * 16);
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < NSTAGE - 1; ++s2) issue_slot(s2);
    int slot = 0;
    for (int kb = 0; kb < nkb; ++kb) {
      wait_vmcnt<(NSTAGE - 2) * L>();                 // this wave's share of the oldest slot has landed
      __builtin_amdgcn_s_barrier();                   // ... and everybody else's; all reads of the slot refilled below are done
      issue_slot((slot + NSTAGE - 1) % NSTAGE);
      const unsigned char* base = smem + slot * SUB;
      slot = (slot + 1) % NSTAGE;
      frag_t fa[2][MREP], fb[2][NREP];
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[0][i] = *reinterpret_cast<const frag_t*>(base + a_rd[i][0]);
#pragma unroll
      for (int j = 0; j < NREP; ++j) fb[0][j] = *reinterpret_cast<const frag_t*>(base + b_rd[j][0]);
#pragma unroll
      for (int i = 0; i < MREP; ++i) fa[1][i] = *reinterpret_cast<const frag_t*>(base + a_rd[i][1]);
#pragma unroll
      for (int j = 0; j < NREP; ++j) fb[1][j] = *reinterpret_cast<const frag_t*>(base + b_rd[j][1]);
#pragma unroll
      for (int hs = 0; hs < 2; ++hs)
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < NREP; ++j) mma64(fa[hs][i], fb[hs][j], acc[i][j]);
    }
  }
  // (filter rounds 1 and 2 are in flight: no wait here)

  // ---- h2 = bf16(ELU(acc + bias)), the arithmetic of nt_epilogue's dense path, from the accumulators into the chunk images: column c of
  // the tile = channel c & 63 of chunk c >> 6, 16-byte units swizzled by (row >> 1) & 7; rows beyond M are zero (as the DMA of
  // conv3x3_s8_body leaves them)
  auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  lds_barrier();                     // the GEMM slot the images take is dead
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int col = (wn * NREP + j) * 16 + (lane >> 4) * 4, cc = col & 63, pos = cc >> 3;
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(smem + kCplBias + col * 4);      // (the oldest request of the launch: long landed)
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
      const int row = wm * MREP * 16 + i * 16 + (lane & 15);
      const f32x4 v = acc[i][j] + b4;
      pack_t o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = ET<T>::from_f32(fast_act<T>(IPOKE_ACT_ELU, v[r]));
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
      const unsigned keep = m0 + row < g.M ? 0xffffffffu : 0u;      // (a mask, not a branch around the ELU)
      const u32x2 bits = __builtin_bit_cast(u32x2, o) & u32x2{keep, keep};
      *reinterpret_cast<u32x2*>(img + (col >> 6) * ABUF + row * 128 + ((pos ^ ((row >> 1) & 7)) * 16) + ((cc >> 2) & 1) * 8) = bits;
    }
  }
  lds_barrier();                     // the images are complete
  // the copy that goes to C: a thread takes one 4-column group in 8 rows (row-contiguous stores) and keeps it in registers; the stores
  // are issued behind the convolution's K loop, whose counted waits they would otherwise sit in
  constexpr int G4F = BN / 4, ITER = BM * G4F / NTHR, RSTEP = NTHR / G4F;
  const int c4 = tid % G4F, r0 = tid / G4F;
  const bool store_c = p.C != nullptr;
  pack_t oc[ITER];
#pragma unroll
  for (int k = 0; k < ITER; ++k) oc[k] = pack_t{};
  if (store_c) {
    const int pos = (c4 & 15) >> 1;
#pragma unroll
    for (int k = 0; k < ITER; ++k) {
      const int row = r0 + k * RSTEP;
      oc[k] = *reinterpret_cast<const pack_t*>(img + (c4 >> 4) * ABUF + row * 128 + ((pos ^ ((row >> 1) & 7)) * 16) + (c4 & 1) * 8);
    }
  }

  // ---- conv3 of this slice: the K-block loop of conv3x3_s8_body (2 row halves x 4 K groups, chunk-major, nine taps inside) on the images
  const int mh = wave & 1, kq = wave >> 1;
  unsigned vmask[MREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i) {
    const int r = i * 16 + (lane & 15);
    const int y = (r >> 3) & 7, x = r & 7;
    unsigned vm = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = y + (t / 3 - 1), xx = x + (t % 3 - 1);
      if ((unsigned)yy < 8u && (unsigned)xx < 8u) vm |= 1u << t;
    }
    vmask[i] = vm;
  }
  const int qlo = lane >> 4;
  int w_rd[CREP];
#pragma unroll
  for (int j = 0; j < CREP; ++j) {
    const int n = j * 16 + (lane & 15);
    w_rd[j] = n * 128 + ((qlo ^ ((n >> 1) & 7)) * 16);
  }
  f32x4 acc2[MREP][CREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < CREP; ++j) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int gk = kq, ci = 0, t = kq;
  int rd_reg = kCplF, rd_r3 = 0;
  for (int r = 0; r < NROUNDS; ++r) {
    wait_vmcnt<WJ>();                // everything but this wave's share of the newest round has landed
    lds_barrier();
    if (r >= 1) issue_w();           // round r + 2 into the region of round r - 1 (rounds 0 .. 2 were requested beside the GEMM)
    if (gk < NKB) {
      const unsigned char* ab = img + ci * ABUF + mh * 64 * 128;
      const unsigned char* wb = smem + rd_reg + (gk & 3) * WSLOT;
      const int th = t / 3, tw = t - 3 * th;
      const int shift = (th - 1) * 8 + (tw - 1);
      const unsigned char* arow[MREP]; int aswz[MREP];
#pragma unroll
      for (int i = 0; i < MREP; ++i) {
        const bool ok = (vmask[i] >> t) & 1u;
        const int sr = i * 16 + (lane & 15) + shift;
        arow[i] = ok ? ab + sr * 128 : zrow;
        aswz[i] = ok ? (sr >> 1) & 7 : 0;
      }
      frag_t fa[2][MREP], fb[2][CREP];
#pragma unroll
      for (int hs = 0; hs < 2; ++hs) {
#pragma unroll
        for (int i = 0; i < MREP; ++i) fa[hs][i] = *reinterpret_cast<const frag_t*>(arow[i] + (((hs * 4 + qlo) ^ aswz[i]) * 16));
#pragma unroll
        for (int j = 0; j < CREP; ++j) fb[hs][j] = *reinterpret_cast<const frag_t*>(wb + (w_rd[j] ^ (hs * 64)));
      }
#pragma unroll
      for (int hs = 0; hs < 2; ++hs)
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
          for (int j = 0; j < CREP; ++j) mma64(fa[hs][i], fb[hs][j], acc2[i][j]);
      // (issue order as in conv3x3_s8_body: the first half-step's fragments, then the second half-step's reads between the MFMAs of the first)
      constexpr int NF = MREP + CREP, NM = MREP * CREP, PER = NM / NF;
      __builtin_amdgcn_sched_group_barrier(0x100, NF, 0);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM - NF * PER, 0);
    }
    gk += 4; t += 4;
    if (t >= 9) { t -= 9; ++ci; }
    rd_r3 = rd_r3 == 2 ? 0 : rd_r3 + 1;
    rd_reg = rd_r3 == 0 ? kCplF : (rd_r3 == 1 ? reg1 : reg2);
  }
  wait_vmcnt<0>();
  ct.pin();
  if (store_c) {                     // h2 to C (the backward pass reads it)
    T* Cp = reinterpret_cast<T*>(p.C) + (long)(m0 + r0) * p.ldc + p.c_coff + n0 + 4 * c4;
#pragma unroll
    for (int k = 0; k < ITER; ++k)
      if (m0 + r0 + k * RSTEP < g.M) *reinterpret_cast<pack_t*>(Cp + (long)k * RSTEP * p.ldc) = oc[k];
  }
  ct.run(p, smem, tile, z, mh, kq, acc2);
}

// RM = reduction rows per ring slot (64).
// NARROW: outputs of <= 64 rows (conv3 of a coupling net, dW [2 Cp][9 * hidden]): a 64 (n) x 256 (k) tile instead of 128 x 128, whose second
// 64 columns would be padding -- half of every workgroup's dY stream, fragment reads and matrix-core work on zeros, and the conv3 weight
// gradients took as long as conv2's with 3.5x fewer FLOPs (7.1 ms of the weight-gradient queue per c2 step).  A stage is the dY image
// (its upper 64 columns stay zero) and TWO A images (k0 .. k0 + 127, k0 + 128 .. k0 + 255); the eight waves own 64 x 32 each, side by side in k.
template <int NSTAGE, int RM, bool NARROW = false, bool ADAM = false>
__global__ __launch_bounds__(512) void igemm_tn_glds_kernel(const TnParams pin) {
  kernarg_prefetch<(int)sizeof(TnParams)>();
  typedef bf16_t T;
  TnParams p = pin;
  if (pin.batch) {                       // batched launch: blockIdx.z selects operands and the 2-D tap geometry
    const TnBatchEntry e = pin.batch[blockIdx.z + pin.z0];
    p.A = pin.a_base + e.a_off; p.dY = pin.y_base + e.y_off; p.dW = pin.w_base + e.w_off;
    p.g.khw = e.kh * e.kw; p.g.kw = e.kw; p.g.taps = e.kh * e.kw; p.g.ph = e.ph; p.g.pw = e.pw;
    if constexpr (ADAM) { p.ad_p += e.w_off; p.ad_m += e.w_off; p.ad_v += e.w_off; p.ad_vmax += e.w_off; p.ad_sh += e.sh_off; }
  }
  typedef typename ET<T>::frag frag_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  static_assert(RM == 64, "stage height: two 32-row reduction steps, read and multiplied in a two-phase software pipeline");
  constexpr int NI = RM / 32;                   // DMA instructions per thread, operand and stage
  constexpr int TILE = RM * 256;                // one operand image: 64 rows x 128 columns of bf16
  constexpr int NIMG = NARROW ? 3 : 2;          // operand images per stage
  constexpr int STAGE = NIMG * TILE;
  constexpr int L = NIMG * NI;                  // DMA instructions per thread and stage
  static_assert((NSTAGE - 2) * L <= 63, "vmcnt field");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* taptab = reinterpret_cast<int*>(smem + NSTAGE * STAGE);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn2 = NARROW ? 0 : wave >> 2, wk = NARROW ? wave : wave & 3;     // wave tile: 64 (n) x 32 (k)
  const GeomDev& g = p.g;
  int tn, tk;
  if (p.xa > 0) {
    // XCD-aware tile map (blocks are dealt round-robin over the 8 XCDs, each with its own L2): XCD x owns a
    // (tiles_n / xa) x (tiles_k / xb) sub-grid, so that its L2 fetches 1/xa of dY and 1/xb of A instead of (with the plain
    // row-major order and tiles_n = 16) 1/8 of dY and ALL of A -- conv2 shape: 47 -> 31 MB of fabric reads per problem
    const int bid = (int)blockIdx.x, xcd = bid & 7, q = bid >> 3;
    const FDiv fxa(p.xa), fxb(p.xb);
    const int sub_n = fxa.div(p.tiles_n), sub_k = fxb.div(p.tiles_k);
    const FDiv fsn(sub_n);
    tn = fxa.mod(xcd) * sub_n + fsn.mod(q);
    tk = fxa.div(xcd) * sub_k + fsn.div(q);
  } else {
    const int tile = (int)blockIdx.x + p.tile0;
    const FDiv ftn(p.tiles_n);
    tn = ftn.mod(tile); tk = ftn.div(tile);
  }
  const int n0 = tn * 128, k0 = tk * (NARROW ? 256 : 128);
  const int z = blockIdx.y;
  const int nmb_total = (g.M + RM - 1) / RM;      // (RM: compile-time)
  const int mb_begin = z * p.mb_per_split, mb_end = min(nmb_total, mb_begin + p.mb_per_split);
  const int nst = mb_end - mb_begin;

  fill_taptab(taptab, g);
  __syncthreads();

  // ---- DMA bookkeeping: instruction i of this thread fills row rloc[i] = 4*(wave + 8*i) + lane/16, LDS chunk lane%16,
  //      with the source chunk (lane%16) ^ swz(row) -- the same for both instructions of a thread
  const int pchunk = lane & 15;
  const int rl0 = 4 * wave + (lane >> 4);
  const int schunk = pchunk ^ tn_swz(rl0);
  const T* dY = reinterpret_cast<const T*>(p.dY);
  const T* A = reinterpret_cast<const T*>(p.A);
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  const int ncol = n0 + schunk * 8;             // dY column of this lane's chunk
  const bool y_ok = ncol < p.ldy - p.y_coff && ncol < ((p.Nout + 7) & ~7);
  const int kcol = k0 + schunk * 8;             // A (im2col) column of this lane's chunk
  const int x_tap = FDiv(p.Kc).div(kcol), x_c = kcol - x_tap * p.Kc;
  const bool x_ok = kcol < p.Ktot && x_c < p.Kc_real;
  const int x_tapcode = x_ok ? taptab[x_tap] : 0;
  const int S = g.S;
  constexpr unsigned kBad = 0xffffffffu;
  unsigned x_fix[2] = {kBad, kBad};
  if (p.rows_fixed && x_ok) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const RowPos r = decode_row(g, rl0 + 32 * i, p.a_sn);      // row inside the reduction block (whole samples)
      int id, ih, iw;
      if (tap_coords(g, r, x_tapcode, id, ih, iw))
        x_fix[i] = (unsigned)(r.nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw + p.a_coff + x_c);
    }
  }
  // NARROW: the second A image (columns k0 + 128 ..)
  const int kcol2 = kcol + 128;
  const int x_tap2 = FDiv(p.Kc).div(kcol2), x_c2 = kcol2 - x_tap2 * p.Kc;
  const bool x_ok2 = NARROW && kcol2 < p.Ktot && x_c2 < p.Kc_real;
  const int x_tapcode2 = x_ok2 ? taptab[x_tap2] : 0;
  unsigned x_fix2[2] = {kBad, kBad};
  if (NARROW && p.rows_fixed && x_ok2) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const RowPos r = decode_row(g, rl0 + 32 * i, p.a_sn);
      int id, ih, iw;
      if (tap_coords(g, r, x_tapcode2, id, ih, iw))
        x_fix2[i] = (unsigned)(r.nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw + p.a_coff + x_c2);
    }
  }
  auto issue = [&](int slot, int mb, bool real) {
    unsigned char* sy = smem + slot * STAGE;
    unsigned char* sx = sy + TILE;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int m = mb * RM + rl0 + 32 * i;
      const T* src = zero;
      if (real && y_ok && m < g.M) src = dY + (long)m * p.ldy + p.y_coff + ncol;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(sy + (wave + 8 * i) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int m = mb * RM + rl0 + 32 * i;
      const T* src = zero;
      if (real && x_ok && m < g.M) {
        if (p.rows_fixed) {
          // rows_fixed: S = 64 (the 8x8 latent).  RM = 64: a stage is one sample, x_fix[i] its rows rl0 + 32 i;
          // RM = 32: stage mb is half (mb & 1) of sample mb >> 1
          const int half = RM == 64 ? i : (mb & 1);
          const long smp = RM == 64 ? (long)mb : (long)(mb >> 1);
          if (x_fix[half] != kBad) src = A + smp * p.a_sn + x_fix[half];
        } else {
          const RowPos r = decode_row(g, m, p.a_sn);
          int id, ih, iw;
          if (tap_coords(g, r, x_tapcode, id, ih, iw))
            src = A + r.nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw + p.a_coff + x_c;
        }
      }
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(sx + (wave + 8 * i) * 1024), 16, 0, 0);
    }
    if constexpr (NARROW) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int m = mb * RM + rl0 + 32 * i;
        const T* src = zero;
        if (real && x_ok2 && m < g.M) {
          if (p.rows_fixed) {
            const int half = RM == 64 ? i : (mb & 1);
            const long smp = RM == 64 ? (long)mb : (long)(mb >> 1);
            if (x_fix2[half] != kBad) src = A + smp * p.a_sn + x_fix2[half];
          } else {
            const RowPos r = decode_row(g, m, p.a_sn);
            int id, ih, iw;
            if (tap_coords(g, r, x_tapcode2, id, ih, iw))
              src = A + r.nb + (long)id * p.a_sd + (long)ih * p.a_sh + (long)iw * p.a_sw + p.a_coff + x_c2;
          }
        }
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(sx + TILE + (wave + 8 * i) * 1024), 16, 0, 0);
      }
    }
  };

  // ---- fragment read offsets (bytes inside an operand image), loop invariant
  // lane (i16 = lane & 15, grp = lane >> 4): reduction rows 8*grp + 4*half + (i16 >> 2) of k-step ks, columns base + 4*(i16 & 3)
  const int i16 = lane & 15, grp = lane >> 4;
  const int rrow = 8 * grp + (i16 >> 2);
  const int hsw = tn_swz(rrow);                  // swz(row) is the same for +4*half and +32*ks
  auto frag_off = [&](int colbase) {             // colbase: multiple of 16 inside the 128-wide image
    const int col = colbase + 4 * (i16 & 3);
    return rrow * 256 + (((col >> 3) ^ hsw) * 16) + ((col >> 2) & 1) * 8;
  };
  // LDS byte addresses of this lane's fragment reads in slot 0, reduction step 0
  const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)smem;
  unsigned y_rd[4], x_rd[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) y_rd[i] = lds0 + (unsigned)frag_off(wn2 * 64 + 16 * i);
#pragma unroll
  for (int j = 0; j < 2; ++j) x_rd[j] = lds0 + (unsigned)(TILE * (1 + (NARROW ? wk >> 2 : 0)) + frag_off((NARROW ? wk & 3 : wk) * 32 + 16 * j));
  // the six operand fragments of reduction step KS (rows 32 KS .. 32 KS + 31) of the stage at byte offset sb: twelve reads in flight
  auto read_frags = [&](frag_t (&f)[6], unsigned sb, auto ks_tag) {
    constexpr int KS = decltype(ks_tag)::value;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const unsigned a = (q < 4 ? y_rd[q & 3] : x_rd[q & 1]) + sb;
      const tn_tr4_t lo = tn_ds_tr<KS * 32 * 256>(a), hi = tn_ds_tr<KS * 32 * 256 + 4 * 256>(a);
#pragma unroll
      for (int e = 0; e < 4; ++e) { f[q][e] = lo[e]; f[q][4 + e] = hi[e]; }
    }
  };
  typedef std::integral_constant<int, 0> K0;
  typedef std::integral_constant<int, 1> K1;

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mma_frags = [&](frag_t (&f)[6]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) mma64(f[i], f[4 + j], acc[i][j]);
  };

  // reads of the next step's fragments (into fn) interleaved with the MFMAs of this step's (fc): three reads behind every second
  // MFMA in issue order -- with the twelve reads in front, eight waves queue 96 transposing reads on the LDS pipe before any of
  // them reaches its first MFMA (the same finding as in conv3x3_halo16)
  auto read_mma = [&](frag_t (&fn)[6], unsigned sb, auto ks_tag, frag_t (&fc)[6]) {
    constexpr int KS = decltype(ks_tag)::value;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = q >> 1, j = q & 1;
      mma64(fc[i], fc[4 + j], acc[i][j]);
      if (q < 6) {                                   // fragment q of the next step: two transposing reads
        const unsigned a = (q < 4 ? y_rd[q & 3] : x_rd[q & 1]) + sb;
        const tn_tr4_t lo = tn_ds_tr<KS * 32 * 256>(a), hi = tn_ds_tr<KS * 32 * 256 + 4 * 256>(a);
#pragma unroll
        for (int e = 0; e < 4; ++e) { fn[q][e] = lo[e]; fn[q][4 + e] = hi[e]; }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // Two-phase pipeline, one barrier per stage: while the matrix cores work on one 32-row step, the fragment reads of the next step
  // (and, in the second phase, the DMA of the stage NSTAGE ahead) are in flight:
  //   [wait FA] read FB = (it, 1) | mma FA | [stage it+1 landed, wait FB] barrier | DMA stage it+NSTAGE -> slot of it | read FA = (it+1, 0) | mma FB
  int issued = 0;
#pragma unroll
  for (int s2 = 0; s2 < NSTAGE; ++s2) { issue(s2, mb_begin + issued, issued < nst); ++issued; }
  wait_vmcnt<(NSTAGE - 1) * L>();                 // this wave's share of stage 0 has landed
  __builtin_amdgcn_s_barrier();                   // ... and everybody else's
  frag_t FA[6], FB[6];
  read_frags(FA, 0u, K0{});
  int slot = 0;
  for (int it = 0; it < nst; ++it) {
    const unsigned sb = (unsigned)(slot * STAGE);
    const int nslot = slot + 1 == NSTAGE ? 0 : slot + 1;
    tn_wait_frags(FA);
    __builtin_amdgcn_sched_barrier(0);
    read_mma(FB, sb, K1{}, FA);
    wait_vmcnt<(NSTAGE - 2) * L>();               // this wave's share of stage it + 1 has landed
    tn_wait_frags(FB);                            // ... and its reads of stage it are complete: the slot may be refilled
    __builtin_amdgcn_s_barrier();
    issue(slot, mb_begin + issued, issued < nst);
    ++issued;
    __builtin_amdgcn_sched_barrier(0);
    read_mma(FA, (unsigned)(nslot * STAGE), K0{}, FB);      // (past the last stage: a padding slot, never multiplied)
    slot = nslot;
  }
  tn_wait_frags(FA);
  wait_vmcnt<0>();

  // epilogue: acc[i][j][r] = dW[n = n0 + wn2*64 + 16i + (lane&15)][k = k0 + wk*32 + 16j + 4*(lane>>4) + r]
  if constexpr (ADAM) {
    // dense 1x1 problem (one tap, w_sc = 1, whole tiles: checked by the launcher).  Two rounds of four 4-element groups: the 16
    // sixteen-byte loads of a round are issued before its arithmetic (64 registers: the kernel stays within the 128 that let two
    // workgroups -- or one and a chain GEMM workgroup -- share a CU).  Non-temporal like the stand-alone optimizer kernels.
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x4 pp[2][2], mm[2][2], vv[2][2], vx[2][2];
      long off[2][2];
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * half + ii;
        const int n = n0 + wn2 * 64 + i * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int k = k0 + wk * 32 + j * 16 + (lane >> 4) * 4;
          off[ii][j] = (long)n * p.w_sn + k;
          pp[ii][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.ad_p + off[ii][j]));
          mm[ii][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.ad_m + off[ii][j]));
          vv[ii][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.ad_v + off[ii][j]));
          vx[ii][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.ad_vmax + off[ii][j]));
        }
      }
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (p.ad_keep_grad) *reinterpret_cast<f32x4*>(p.dW + off[ii][j]) = acc[2 * half + ii][j];
          adam_amsgrad_update4(pp[ii][j], acc[2 * half + ii][j], mm[ii][j], vv[ii][j], vx[ii][j], p.ad_h);
          __builtin_nontemporal_store(pp[ii][j], reinterpret_cast<f32x4*>(p.ad_p + off[ii][j]));
          __builtin_nontemporal_store(mm[ii][j], reinterpret_cast<f32x4*>(p.ad_m + off[ii][j]));
          __builtin_nontemporal_store(vv[ii][j], reinterpret_cast<f32x4*>(p.ad_v + off[ii][j]));
          __builtin_nontemporal_store(vx[ii][j], reinterpret_cast<f32x4*>(p.ad_vmax + off[ii][j]));
          typedef __attribute__((ext_vector_type(4))) __bf16 bf4_t;
          bf4_t o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = ET<T>::from_f32(pp[ii][j][r]);
          *reinterpret_cast<bf4_t*>(p.ad_sh + off[ii][j]) = o;
        }
    }
    return;
  }
  const bool vec4 = p.w_sc == 1 && !p.accumulate && !(p.splitm > 1 && p.split_stride == 0) && ((p.w_sn | p.w_st | p.split_stride) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(p.dW) & 15) == 0 && (p.Kc & 3) == 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn2 * 64 + i * 16 + (lane & 15);
    if (n >= p.Nout) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wk * 32 + j * 16 + (lane >> 4) * 4;
      if (k >= p.Ktot) continue;
      const int tap = FDiv(p.Kc).div(k), c = k - tap * p.Kc;     // 4 consecutive k share the tap (Kc % 4 == 0)
      float* base = p.dW + (long)n * p.w_sn + (long)tap * p.w_st + (p.split_stride > 0 ? (long)z * p.split_stride : 0L);
      if (vec4 && c + 3 < p.Kc_store) {                 // dense rows (1x1 convs): one 16-byte store instead of four
        *reinterpret_cast<f32x4*>(base + c) = acc[i][j];
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (c + r < p.Kc_store) {
          float* q = base + (long)(c + r) * p.w_sc;
          if (p.splitm > 1 && p.split_stride == 0) atomicAdd(q, acc[i][j][r]);
          else *q = p.accumulate ? *q + acc[i][j][r] : acc[i][j][r];
        }
      }
    }
  }
}

// =============================================================================================
// Weight gradient of a 3x3 / stride 1 / pad 1 convolution on the 8x8 latent with the INPUT STATIONARY (round 6): conv1 and conv3 of
// every coupling net (macow_utils.py:270-281) -- one side of the problem is narrow (conv3: <= 64 outputs over 9 x 2048 inputs, conv1:
// 2048 outputs over 9 x <= 64 inputs).  As an implicit GEMM (igemm_tn_glds above) the nine taps are nine K-columns: every tile
// re-gathers the shifted input rows per tap and stage -- 960 KB of operand stream per workgroup, a 20-stage chain of loaded L2 -> LDS
// latencies; the two families took 11 ms of the weight-gradient queue per c2 step for 1.3 TFLOP (4 % of the matrix peak).
// Here a workgroup owns a [64 outputs] x [64 inputs] x [9 taps] block of dW.  A stage is two whole samples: the dY image
// [128 rows x 64 n] and the input image [128 rows x 64 c], 16 KB each, global -> LDS untouched (3-slot ring, one barrier per stage);
// the nine taps read the SAME input image through shifted row addresses -- every lane of a transposing read (ds_read_b64_tr_b16)
// supplies the address of one row, so a row whose tap falls outside the 8x8 map points at a zero row.  320 KB of operand stream per
// workgroup at B = 20.  Eight waves = 2 reduction halves (rows 32 kg .. 32 kg + 31 of both samples) x 4 column groups (16 inputs
// each); a wave holds acc[9 taps][4] fragments (144 registers); the halves meet in LDS in a fixed order, and the block leaves
// through an LDS image of the PyTorch layout [n][c][tap] (9 x 64 consecutive floats per output row).
// 128-byte image rows: 16-byte chunk p of row r is stored at chunk p ^ lat8_swz(r) (applied on the DMA's source side).
__device__ __forceinline__ int lat8_swz(int row) { return 2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1)); }

struct Lat8Params {
  const TnBatchEntry* batch; const unsigned char* a_base; const unsigned char* y_base; float* w_base;
  int M;                 // 64 * B rows
  int lda, a_coff, Kc, Kc_store;      // input rows: [M][lda] bf16, first channel a_coff, Kc channels in the K index, Kc_store written
  int ldy, y_coff, Nout;              // dY rows: [M][ldy] bf16
  long w_sn;             // floats between output rows of dW ([n][c][3][3]: w_sn = Cin * 9)
  int tiles_n, tiles_c, z0;
};

template <int NSTAGE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void wgrad3x3_lat8_kernel(const Lat8Params p) {
  kernarg_prefetch<(int)sizeof(Lat8Params)>();
  typedef bf16_t T;
  typedef ET<T>::frag frag_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int IMG = 128 * 128;                // one operand image: 128 rows x 64 bf16
  constexpr int STAGE = 2 * IMG;
  constexpr int L = 4;                          // DMA instructions per thread and stage
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* zrow = smem + NSTAGE * STAGE;  // 128 bytes of zeros
  const TnBatchEntry e = p.batch[blockIdx.z + p.z0];
  const T* A = reinterpret_cast<const T*>(p.a_base + e.a_off);
  const T* dY = reinterpret_cast<const T*>(p.y_base + e.y_off);
  float* dW = p.w_base + e.w_off;
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kg = wave >> 2, wc = wave & 3;
  const int tile = blockIdx.x, tn = tile % p.tiles_n, tc = tile / p.tiles_n;
  const int n0 = tn * 64, c0 = tc * 64;
  const int nst = (p.M + 127) >> 7;
  if (tid < 8) reinterpret_cast<f32x4*>(zrow)[tid] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- DMA: instruction i of a thread fills rows 8 * (wave + 8 i) .. + 7 (lane / 8) of an image, chunk position lane % 8
  int d_row[2]; unsigned y_src[2], x_src[2]; bool y_ok[2], x_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 8 * (wave + 8 * i) + (lane >> 3), sch = (lane & 7) ^ lat8_swz(row);
    d_row[i] = row;
    const int ncol = n0 + sch * 8, ccol = c0 + sch * 8;
    y_ok[i] = ncol < ((p.Nout + 7) & ~7) && ncol + 8 <= p.ldy - p.y_coff;
    x_ok[i] = ccol < p.Kc;
    y_src[i] = (unsigned)(p.y_coff + ncol);
    x_src[i] = (unsigned)(p.a_coff + ccol);
  }
  auto issue = [&](int slot, int st, bool real) {
    unsigned char* sy = smem + slot * STAGE;
    unsigned char* sx = sy + IMG;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long m = (long)st * 128 + d_row[i];
      const T* src = (real && y_ok[i] && m < p.M) ? dY + m * p.ldy + y_src[i] : zero;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(sy + (wave + 8 * i) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long m = (long)st * 128 + d_row[i];
      const T* src = (real && x_ok[i] && m < p.M) ? A + m * p.lda + x_src[i] : zero;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(sx + (wave + 8 * i) * 1024), 16, 0, 0);
    }
  };

  // ---- fragment reads.  Lane (i16 = lane & 15, grp = lane >> 4) supplies row 32 kg + 8 grp + (i16 >> 2) (+ 4 for the upper half of
  //      the 8 reduction rows) of a sample, columns base + 4 (i16 & 3); it receives column base + i16, reduction rows 8 grp .. + 7
  const int i16 = lane & 15, grp = lane >> 4;
  const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned zaddr = lds0 + (unsigned)(NSTAGE * STAGE) + 8u * (unsigned)(i16 & 3);
  const int r_lo = 32 * kg + 8 * grp + (i16 >> 2);                  // row inside a sample (0 .. 63); the upper half is r_lo + 4
  auto img_off = [&](int row, int col) {                             // byte offset inside an image of (row, 4-column group at col)
    return row * 128 + (((col >> 3) ^ lat8_swz(row)) * 16) + ((col >> 2) & 1) * 8;
  };
  unsigned y_rd[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) y_rd[i][h] = lds0 + (unsigned)img_off(r_lo + 4 * h, 16 * i + 4 * (i16 & 3));
  const int xcol = 16 * wc + 4 * (i16 & 3);
  // validity of tap (dy, dx) for this lane's two rows: y = 4 kg + grp for both, x = (i16 >> 2) + 4 h
  const int py = 4 * kg + grp, px = i16 >> 2;
  auto x_addr = [&](int h, int dy, int dx) -> unsigned {              // address of the shifted row inside sample 0 of slot 0
    const int yy = py + dy, xx = px + 4 * h + dx;
    if ((unsigned)yy >= 8u || (unsigned)xx >= 8u) return zaddr;
    return lds0 + (unsigned)(IMG + img_off(r_lo + 4 * h + 8 * dy + dx, xcol));
  };

  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto tr_read = [&](unsigned addr) -> tn_tr4_t { return tn_ds_tr<0>(addr); };
  auto load_frag = [&](frag_t& f, unsigned a_lo, unsigned a_hi) {
    const tn_tr4_t lo = tr_read(a_lo), hi = tr_read(a_hi);
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) { f[e2] = lo[e2]; f[4 + e2] = hi[e2]; }
  };

  int issued = 0;
#pragma unroll
  for (int s2 = 0; s2 < NSTAGE - 1; ++s2) { issue(s2, issued, issued < nst); ++issued; }
  int slot = 0;
  for (int it = 0; it < nst; ++it) {
    wait_vmcnt<(NSTAGE - 2) * L>();               // this wave's share of stage `it` has landed ...
    __builtin_amdgcn_s_barrier();                 // ... everybody's, and everybody is done with the slot refilled below
    {
      const int fill = slot + NSTAGE - 1 >= NSTAGE ? slot - 1 : slot + NSTAGE - 1;
      issue(fill, issued, issued < nst); ++issued;
    }
    const unsigned sb = (unsigned)(slot * STAGE);
#pragma unroll
    for (int smp = 0; smp < 2; ++smp) {
      const unsigned so = sb + (unsigned)(smp * 64 * 128);
      frag_t fy[4], fx[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) load_frag(fy[i], y_rd[i][0] + so, y_rd[i][1] + so);
      {
        const unsigned a0 = x_addr(0, -1, -1), a1 = x_addr(1, -1, -1);
        load_frag(fx[0], a0 == zaddr ? zaddr : a0 + so, a1 == zaddr ? zaddr : a1 + so);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fy[0]), "+v"(fy[1]), "+v"(fy[2]), "+v"(fy[3]), "+v"(fx[0])::"memory");
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t < 8) {
          const int dy = (t + 1) / 3 - 1, dx = (t + 1) % 3 - 1;
          const unsigned a0 = x_addr(0, dy, dx), a1 = x_addr(1, dy, dx);
          load_frag(fx[(t + 1) & 1], a0 == zaddr ? zaddr : a0 + so, a1 == zaddr ? zaddr : a1 + so);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) mma64(fy[i], fx[t & 1], acc[t][i]);
        if (t < 8) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fx[(t + 1) & 1])::"memory");
      }
    }
    slot = slot + 1 == NSTAGE ? 0 : slot + 1;
  }
  wait_vmcnt<0>();
  __syncthreads();                                // the ring is dead

  // ---- epilogue: the two reduction halves meet (kg 1 parks, kg 0 adds: a fixed order), the block leaves as rows of 9 * 64 floats.
  // acc[t][i][r] = dW[n = n0 + 16 i + (lane & 15)][c = c0 + 16 wc + 4 (lane >> 4) + r][tap t]; two rounds of 32 output rows
  float* img = reinterpret_cast<float*>(smem);    // [32 n][64 c * 9 + pad]: 577 floats per row (odd pitch: conflict-free scalar access)
  constexpr int PITCH = 577;
  const int c_loc = 16 * wc + 4 * grp;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (kg == 1) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        float* row = img + (16 * ii + i16) * PITCH;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) row[(c_loc + r) * 9 + t] = acc[t][2 * half + ii][r];
      }
    }
    __syncthreads();
    if (kg == 0) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        float* row = img + (16 * ii + i16) * PITCH;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) row[(c_loc + r) * 9 + t] += acc[t][2 * half + ii][r];
      }
    }
    __syncthreads();
    const int ncols = 9 * max(0, min(64, p.Kc_store - c0));          // floats of a row that exist in dW
    for (int idx = tid; idx < 32 * 576; idx += 512) {
      const int rl = idx / 576, cc = idx - rl * 576;
      const int n = n0 + 32 * half + rl;
      if (n < p.Nout && cc < ncols) dW[(long)n * p.w_sn + (long)c0 * 9 + cc] = img[rl * PITCH + cc];
    }
    __syncthreads();
  }
}

// =============================================================================================
// Weight gradient of a 3x3 (kd = 1) or 3x3x3 (kd = 3) / stride 1 / "same" convolution on LARGE maps with the input stationary (round 6;
// the first stage's training step: BasicBlock conv1 / conv2 of the 3-D encoder, motion_encoder.py:45-74, and the 3x3 convolutions of the
// SPADE decoder, autoencoders/util.py:106-192).  The idea of wgrad3x3_lat8 one size up: a workgroup owns a [64 out] x [64 in] x [9 taps]
// block of dW for ONE depth tap and reduces over 16 x 16-pixel patches; a stage is the patch's dY image [256 px x 64 n] (32 KB) and its
// input image WITH HALO [18 x 18 px x 64 c] (41 KB, zero border materialised by the DMA), double-buffered; the nine in-plane taps are
// shifted row addresses of the transposing LDS reads (no validity masks: the halo is there).  As an implicit GEMM (igemm_tn_glds) every
// 64-row stage re-gathers the input rows per K-column of the tap it belongs to: 65 FLOP per byte of L2 -> LDS traffic; here 259.
// blockIdx.x = (n-chunk, c-chunk, depth tap), blockIdx.y = reduction split: patches z, z + splitm, ... ; a split stores its block into
// slab z (split_stride) like the implicit-GEMM kernels (the caller sums the slabs: deterministic), or straight into dW when splitm = 1.
struct HaloWgParams {
  const bf16_t* A; const bf16_t* dY; float* dW;
  int NB, D, H, W, kd;
  long a_sn, a_sd, a_sh, a_sw; int a_coff, Kc, Kc_store;
  int ldy, y_coff, Nout;
  long w_sn, w_sc, w_st, split_stride;
  int splitm, tiles_n, tiles_c, ppx, ppy;       // patches per row / column of a depth slice
};

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void wgrad3x3_halo_kernel(const HaloWgParams p) {
  kernarg_prefetch<(int)sizeof(HaloWgParams)>();
  typedef bf16_t T;
  typedef ET<T>::frag frag_t;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int YIMG = 256 * 128;               // dY image: 256 pixels x 64 n
  constexpr int XROWS = 18 * 18, XIMG = 328 * 128;      // input image with halo: 324 rows (+ 4 rows of padding to whole DMA instructions)
  constexpr int STAGE = YIMG + XIMG;            // 74 752 bytes
  constexpr int LY = 4, LX = 6, L = LY + LX;    // DMA instructions per thread and stage
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const T* zero = reinterpret_cast<const T*>(g_zero_chunk);
  unsigned char* dummy = smem + 2 * STAGE;      // 8 KB landing zone of the padding DMA instructions (one KB per wave)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kg = wave >> 2, wc = wave & 3;
  int tile = blockIdx.x;
  const int tn = tile % p.tiles_n; tile /= p.tiles_n;
  const int tc = tile % p.tiles_c, kdi = tile / p.tiles_c;
  const int n0 = tn * 64, c0 = tc * 64, dshift = kdi - (p.kd >> 1);
  const int z = blockIdx.y;
  const int per_slice = p.ppx * p.ppy;
  const long npatch = (long)p.NB * p.D * per_slice;

  // ---- DMA bookkeeping.  dY: instruction i fills pixels 8 (wave + 8 i) .. + 7 (lane / 8), chunk position lane % 8.
  //      X: instruction i fills halo rows 8 (wave + 8 i) .. + 7; rows >= 324 land in the dummy zone.
  int y_q[LY]; unsigned y_col[LY]; bool y_ok[LY];
#pragma unroll
  for (int i = 0; i < LY; ++i) {
    const int q = 8 * (wave + 8 * i) + (lane >> 3), sch = (lane & 7) ^ lat8_swz(q);
    const int ncol = n0 + sch * 8;
    y_q[i] = q; y_col[i] = (unsigned)(p.y_coff + ncol);
    y_ok[i] = ncol < ((p.Nout + 7) & ~7) && ncol + 8 <= p.ldy - p.y_coff;
  }
  int x_hy[LX], x_hx[LX]; unsigned x_col[LX]; bool x_ok[LX];
#pragma unroll
  for (int i = 0; i < LX; ++i) {
    const int hr = 8 * (wave + 8 * i) + (lane >> 3), sch = (lane & 7) ^ lat8_swz(hr);
    const int ccol = c0 + sch * 8;
    x_hy[i] = hr / 18; x_hx[i] = hr - 18 * x_hy[i];
    x_col[i] = (unsigned)(p.a_coff + ccol);
    x_ok[i] = hr < XROWS && ccol < p.Kc;
  }
  // patch pt -> (image, output depth, patch row, patch column); returns false when the depth tap leaves the volume
  auto decode = [&](long pt, int& img, int& d_out, int& py0, int& px0) {
    const int within = (int)(pt % per_slice);
    const long sl = pt / per_slice;
    d_out = (int)(sl % p.D); img = (int)(sl / p.D);
    py0 = (within / p.ppx) * 16; px0 = (within % p.ppx) * 16;
    const int d_in = d_out + dshift;
    return d_in >= 0 && d_in < p.D;
  };
  auto issue = [&](int buf, long pt) {
    int img, d_out, py0, px0;
    decode(pt, img, d_out, py0, px0);
    unsigned char* sy = smem + buf * STAGE;
    unsigned char* sx = sy + YIMG;
    const long m_base = (((long)img * p.D + d_out) * p.H + py0) * p.W + px0;       // dY row of the patch's first pixel
#pragma unroll
    for (int i = 0; i < LY; ++i) {
      const int qy = y_q[i] >> 4, qx = y_q[i] & 15;
      const T* src = y_ok[i] ? p.dY + (m_base + (long)qy * p.W + qx) * p.ldy + y_col[i] : zero;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(sy + (wave + 8 * i) * 1024), 16, 0, 0);
    }
    const long a_base = (long)img * p.a_sn + (long)(d_out + dshift) * p.a_sd;
#pragma unroll
    for (int i = 0; i < LX; ++i) {
      const int yy = py0 + x_hy[i] - 1, xx = px0 + x_hx[i] - 1;
      const bool in = x_ok[i] && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
      const T* src = in ? p.A + a_base + (long)yy * p.a_sh + (long)xx * p.a_sw + x_col[i] : zero;
      unsigned char* dst = 8 * (wave + 8 * i) < 328 ? sx + (wave + 8 * i) * 1024 : dummy + wave * 1024;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    }
  };
  // next patch of this split at or after pt whose depth tap stays inside the volume (npatch: none)
  auto next_valid = [&](long pt) {
    for (; pt < npatch; pt += p.splitm) {
      int a, b, c, d;
      if (decode(pt, a, b, c, d)) return pt;
    }
    return npatch;
  };

  // ---- fragment reads: lane (i16 = lane & 15, grp = lane >> 4) supplies pixel 32 ks + 8 grp + (i16 >> 2) (+ 4) of the patch
  const int i16 = lane & 15, grp = lane >> 4;
  const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)smem;
  auto img_off = [&](int row, int col) { return row * 128 + (((col >> 3) ^ lat8_swz(row)) * 16) + ((col >> 2) & 1) * 8; };
  const int q_lo = 8 * grp + (i16 >> 2);                    // pixel inside a 32-pixel reduction step (two patch rows)
  unsigned y_rd[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) y_rd[i][h] = lds0 + (unsigned)img_off(q_lo + 4 * h, 16 * i + 4 * (i16 & 3));
  const int xcol = 16 * wc + 4 * (i16 & 3);
  const int pyl = grp >> 1, pxl = 8 * (grp & 1) + (i16 >> 2);       // this lane's pixel of step 0: patch row pyl, column pxl (+ 4 h)

  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto load_frag = [&](frag_t& f, unsigned a_lo, unsigned a_hi) {
    const tn_tr4_t lo = tn_ds_tr<0>(a_lo), hi = tn_ds_tr<0>(a_hi);
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) { f[e2] = lo[e2]; f[4 + e2] = hi[e2]; }
  };
  auto x_addr = [&](unsigned xb, int ks, int h, int dy, int dx) -> unsigned {
    const int row = (2 * ks + pyl + 1 + dy) * 18 + pxl + 4 * h + 1 + dx;
    return xb + (unsigned)img_off(row, xcol);
  };

  long cur = next_valid(z);
  int buf = 0;
  if (cur < npatch) issue(0, cur);
  while (cur < npatch) {
    const long nxt = next_valid(cur + p.splitm);
    if (nxt < npatch) { issue(buf ^ 1, nxt); wait_vmcnt<L>(); } else { wait_vmcnt<0>(); }
    __builtin_amdgcn_s_barrier();                 // this stage has landed for everybody
    const unsigned yb = (unsigned)(buf * STAGE), xb = lds0 + (unsigned)(buf * STAGE + YIMG);
#pragma unroll 1
    for (int kk = 0; kk < 4; ++kk) {
      const int ks = 2 * kk + kg;                 // the two reduction halves take alternate 32-pixel steps
      const unsigned so = yb + (unsigned)(ks * 32 * 128);
      frag_t fy[4], fx[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) load_frag(fy[i], y_rd[i][0] + so, y_rd[i][1] + so);
      load_frag(fx[0], x_addr(xb, ks, 0, -1, -1), x_addr(xb, ks, 1, -1, -1));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fy[0]), "+v"(fy[1]), "+v"(fy[2]), "+v"(fy[3]), "+v"(fx[0])::"memory");
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t < 8) {
          const int dy = (t + 1) / 3 - 1, dx = (t + 1) % 3 - 1;
          load_frag(fx[(t + 1) & 1], x_addr(xb, ks, 0, dy, dx), x_addr(xb, ks, 1, dy, dx));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) mma64(fy[i], fx[t & 1], acc[t][i]);
        if (t < 8) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fx[(t + 1) & 1])::"memory");
      }
    }
    __builtin_amdgcn_s_barrier();                 // everybody is done with this buffer: the next iteration may refill it
    cur = nxt; buf ^= 1;
  }
  __syncthreads();

  // ---- epilogue (as wgrad3x3_lat8): the two reduction halves meet in LDS in a fixed order, the block leaves by output rows
  float* img = reinterpret_cast<float*>(smem);
  constexpr int PITCH = 577;
  const int c_loc = 16 * wc + 4 * grp;
  float* dst = p.dW + (p.split_stride > 0 ? (long)z * p.split_stride : 0L);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (kg == 1) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        float* row = img + (16 * ii + i16) * PITCH;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) row[(c_loc + r) * 9 + t] = acc[t][2 * half + ii][r];
      }
    }
    __syncthreads();
    if (kg == 0) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        float* row = img + (16 * ii + i16) * PITCH;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) row[(c_loc + r) * 9 + t] += acc[t][2 * half + ii][r];
      }
    }
    __syncthreads();
    const int cmax = max(0, min(64, p.Kc_store - c0));
    for (int idx = tid; idx < 32 * 576; idx += 512) {
      const int rl = idx / 576, cc = idx - rl * 576, c = cc / 9, t = cc - 9 * c;
      const int n = n0 + 32 * half + rl;
      if (n < p.Nout && c < cmax) dst[(long)n * p.w_sn + (long)(c0 + c) * p.w_sc + (long)(kdi * 9 + t) * p.w_st] = img[rl * PITCH + cc];
    }
    __syncthreads();
  }
}

static constexpr size_t kLdsHaloWg = 2 * (256 * 128 + 328 * 128) + 8 * 1024;
static bool halo_wgrad_applicable(const TnParams& p) {
  const GeomDev& g = p.g;
  const int kd = g.taps / 9;
  return !p.batch && !p.a_f32 && p.a_sc == 1 && (g.taps == 9 || g.taps == 27) && g.khw == 9 && g.kw == 3 && !g.transposed &&
         g.sd == 1 && g.sh == 1 && g.sw == 1 && g.ph == 1 && g.pw == 1 && g.pd == kd / 2 && g.Di == g.Do && g.Hi == g.Ho && g.Wi == g.Wo &&
         g.Ho % 16 == 0 && g.Wo % 16 == 0 && (g.taps == 27 || g.Di == 1) &&
         (p.a_coff & 7) == 0 && (p.Kc & 7) == 0 && p.Kc == p.Kc_real && ((p.a_sn | p.a_sd | p.a_sh | p.a_sw) & 7) == 0 &&
         (p.ldy & 7) == 0 && (p.y_coff & 7) == 0 && !p.accumulate && (p.splitm == 1 || p.split_stride > 0) && p.max_wgs <= 0 &&
         p.ad_p == nullptr && kLdsHaloWg <= device_max_lds() &&
         ((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.dY)) & 15) == 0 &&
         // worth it where the patches are many and the tile is not mostly padding
         (long)g.M >= 16384 && p.Kc >= 32 && p.Nout >= 32;
}
static int launch_halo_wgrad(const TnParams& t, hipStream_t s) {
  const GeomDev& g = t.g;
  HaloWgParams p;
  p.A = reinterpret_cast<const bf16_t*>(t.A); p.dY = reinterpret_cast<const bf16_t*>(t.dY); p.dW = t.dW;
  p.NB = g.M / g.S; p.D = g.Do; p.H = g.Ho; p.W = g.Wo; p.kd = g.taps / 9;
  p.a_sn = t.a_sn; p.a_sd = t.a_sd; p.a_sh = t.a_sh; p.a_sw = t.a_sw; p.a_coff = t.a_coff; p.Kc = t.Kc; p.Kc_store = t.Kc_store;
  p.ldy = t.ldy; p.y_coff = t.y_coff; p.Nout = t.Nout;
  p.w_sn = t.w_sn; p.w_sc = t.w_sc; p.w_st = t.w_st; p.split_stride = t.splitm > 1 ? t.split_stride : 0;
  p.splitm = t.splitm; p.tiles_n = ceil_div(t.Nout, 64); p.tiles_c = ceil_div(t.Kc, 64); p.ppx = g.Wo / 16; p.ppy = g.Ho / 16;
  auto kern = wgrad3x3_halo_kernel;
  IPK_SET_LDS_ONCE(kern, kLdsHaloWg);
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_n * p.tiles_c * p.kd), (unsigned)p.splitm), dim3(512), kLdsHaloWg, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
// Reduction splits the weight-gradient kernel the dispatcher will take for this problem wants for `target_wgs` workgroups (callers
// size their slabs with it); 0: no preference (the caller's own rule).
static int halo_wgrad_splits(const TnParams& p, int target_wgs) {
  const GeomDev& g = p.g;
  const long tiles = (long)ceil_div(p.Nout, 64) * ceil_div(p.Kc, 64) * (g.taps / 9);
  const long patches = (long)(g.M / g.S) * g.Do * (g.Ho / 16) * (g.Wo / 16);
  long sp = target_wgs / tiles; if (sp < 1) sp = 1;
  if (sp > patches / 4) sp = patches / 4 > 0 ? patches / 4 : 1;
  return (int)sp;
}

static bool lat8_applicable(const TnParams& p, int nbatch) {
  const GeomDev& g = p.g;
  return p.batch && nbatch >= 1 && !p.a_f32 && p.a_sc == 1 && g.taps == 9 && g.khw == 9 && g.kw == 3 && g.Di == 1 && g.Hi == 8 && g.Wi == 8 &&
         g.Do == 1 && g.Ho == 8 && g.Wo == 8 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 && g.ph == 1 && g.pw == 1 && !g.transposed &&
         p.a_sh == 8 * p.a_sw && p.a_sn == 64 * p.a_sw && (p.a_sw & 7) == 0 && (p.a_coff & 7) == 0 && (p.Kc & 7) == 0 && p.Kc == p.Kc_real &&
         (p.ldy & 7) == 0 && (p.y_coff & 7) == 0 && p.splitm == 1 && !p.accumulate && p.split_stride == 0 && p.w_sc == 9 && p.w_st == 1 &&
         p.w_sn >= (long)p.Kc_store * 9 && p.max_wgs <= 0 && g.M % 64 == 0 && p.ad_p == nullptr && kLdsLat8 <= device_max_lds() &&
         (long)g.M * p.a_sw < (1L << 31) && (long)g.M * p.ldy < (1L << 31) &&
         ((reinterpret_cast<uintptr_t>(p.a_base) | reinterpret_cast<uintptr_t>(p.y_base)) & 15) == 0;
}
static int launch_lat8(const TnParams& t, hipStream_t s, int nbatch) {
  Lat8Params p;
  p.batch = t.batch; p.a_base = t.a_base; p.y_base = t.y_base; p.w_base = t.w_base;
  p.M = t.g.M; p.lda = (int)t.a_sw; p.a_coff = t.a_coff; p.Kc = t.Kc; p.Kc_store = t.Kc_store;
  p.ldy = t.ldy; p.y_coff = t.y_coff; p.Nout = t.Nout; p.w_sn = t.w_sn;
  p.tiles_n = ceil_div(t.Nout, 64); p.tiles_c = ceil_div(t.Kc, 64); p.z0 = 0;
  const dim3 grid((unsigned)(p.tiles_n * p.tiles_c), 1, (unsigned)nbatch);
  auto kern = wgrad3x3_lat8_kernel<3>;
  IPK_SET_LDS_ONCE(kern, kLdsLat8);
  hipLaunchKernelGGL(kern, grid, dim3(512), kLdsLat8, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

static thread_local int g_last_wgrad_kernel = IPOKE_WGRAD_KERNEL_NONE;     // (see ipoke_last_wgrad_kernel)

template <typename T>
static int launch_tn(TnParams& p, hipStream_t s, int nbatch = 1) {
  constexpr int RM = 128 / (int)sizeof(T);
  g_last_wgrad_kernel = IPOKE_WGRAD_KERNEL_TN;
  p.tiles_n = ceil_div(p.Nout, 128);
  p.tiles_k = ceil_div(p.Ktot, 128);
  const int nmb = ceil_div(p.g.M, RM);
  {
    p.rows_fixed = (RM % p.g.S == 0) ? 1 : 0;
  }
  if (p.splitm < 1) p.splitm = 1;
  if (p.splitm > nmb) p.splitm = nmb;
  p.mb_per_split = ceil_div(nmb, p.splitm);
  if constexpr (sizeof(T) == 2) {
    // batched 3x3 problems on the 8x8 latent (conv1 / conv3 of the coupling nets): the stationary-input kernel
    if (lat8_applicable(p, nbatch)) { g_last_wgrad_kernel = IPOKE_WGRAD_KERNEL_LAT8; return launch_lat8(p, s, nbatch); }
    // 3x3 / 3x3x3 stride-1 problems on large maps (first-stage training): the halo-staged kernel
    if (nbatch == 1 && halo_wgrad_applicable(p)) { g_last_wgrad_kernel = IPOKE_WGRAD_KERNEL_HALO; return launch_halo_wgrad(p, s); }
  }
  const size_t lds = 4 * 128 * kPitch + 256 * sizeof(int);
  // LDS-DMA + transposed-read kernel: bf16, dense operands with 16-byte aligned rows
  // (batched launches: the engine's workspace offsets are 256-byte aligned)
  if (sizeof(T) == 2 && !p.a_f32 && p.a_sc == 1 && (p.a_coff & 7) == 0 && (p.Kc & 7) == 0 &&
      (p.ldy & 7) == 0 && (p.y_coff & 7) == 0 && ((p.a_sn | p.a_sd | p.a_sh | p.a_sw) & 7) == 0 &&
      (p.batch ? ((reinterpret_cast<uintptr_t>(p.a_base) | reinterpret_cast<uintptr_t>(p.y_base)) & 15) == 0
               : ((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.dY)) & 15) == 0)) {
    // ring depth: 2 slots (64 KB of LDS) let a weight-gradient workgroup share a CU with a chain GEMM workgroup (89 KB): the
    // same 29 us alone, 39 instead of 55 us inside the train step; three slots measure the same alone.  (Four slots of 32 rows in the
    // same 64 KB -- three stages in flight, twice the barriers -- measured 35.5 against 29.7 us alone and 63.3 against 62.0 ms per step
    // in round 3; removed.)
    constexpr int NST = 2;
    // the kernel's fixed-row addressing takes a 64-row stage for ONE sample (the 8 x 8 latent); on a smaller map a stage holds
    // several samples and every row is decoded on its own (igemm_tn_kernel steps mb * (RM / S) samples per stage instead)
    if (p.g.S != RM) p.rows_fixed = 0;
    // narrow outputs of the flow engine's batched launches (conv3 of the coupling nets): 64 x 256 tiles (see the kernel)
    const bool narrow = p.batch != nullptr && p.Nout <= 64 && p.Ktot >= 512 && p.max_wgs <= 0;
    if (narrow) p.tiles_k = ceil_div(p.Ktot, 256);
    g_last_wgrad_kernel = narrow ? IPOKE_WGRAD_KERNEL_TN_NARROW : IPOKE_WGRAD_KERNEL_TN_GLDS;
    const size_t lds2 = narrow ? (size_t)NST * 3 * 64 * 256 + 256 * sizeof(int) : (size_t)NST * 2 * 64 * 256 + 256 * sizeof(int);
    const bool adam = p.ad_p != nullptr;
    if (adam) IPK_REQUIRE(!narrow && p.batch && p.g.taps == 1 && p.w_sc == 1 && p.w_sn == p.Ktot && p.Nout % 128 == 0 && p.Ktot % 128 == 0 &&
                          p.splitm == 1 && !p.accumulate && p.Kc == p.Kc_real && (p.Kc_store == 0 || p.Kc_store == p.Kc) && (p.w_sn & 3) == 0,
                          "Adam in the weight-gradient epilogue: batched dense 1x1 problems in whole 128 x 128 tiles, one reduction split");
    auto kern = adam ? igemm_tn_glds_kernel<NST, 64, false, true> : narrow ? igemm_tn_glds_kernel<NST, 64, true> : igemm_tn_glds_kernel<NST, 64>;
    if (adam) { IPK_SET_LDS_ONCE(kern, lds2); } else if (narrow) { IPK_SET_LDS_ONCE(kern, lds2); } else { IPK_SET_LDS_ONCE(kern, lds2); }      // one flag per kernel
    const int ntiles = p.tiles_n * p.tiles_k;
    const int cap = p.max_wgs > 0 ? p.max_wgs : ntiles;
    p.xa = p.xb = 0;
    if (cap >= ntiles && ntiles % 8 == 0) {     // whole problem in one launch, blockIdx.x % 8 = XCD for every (y, z)
      double best = -1;
      for (int xa = 1; xa <= 8; xa *= 2) {
        const int xb = 8 / xa;
        if (p.tiles_n % xa || p.tiles_k % xb) continue;
        const double cost = (double)p.tiles_n / xa + (double)p.tiles_k / xb;       // operand columns an XCD's L2 has to hold
        if (best < 0 || cost < best) { best = cost; p.xa = xa; p.xb = xb; }
      }
    }
    for (int t0 = 0; t0 < ntiles; t0 += cap) {
      p.tile0 = t0;
      const int nt = std::min(cap, ntiles - t0);
      // the cap counts the problems of a batched launch too: as many whole problems per launch as fit under it
      const int zper = p.max_wgs > 0 ? std::max(1, p.max_wgs / std::max(1, nt * p.splitm)) : nbatch;
      for (int z0 = 0; z0 < nbatch; z0 += zper) {
        p.z0 = z0;
        dim3 grid2((unsigned)nt, (unsigned)p.splitm, (unsigned)std::min(zper, nbatch - z0));
        hipLaunchKernelGGL(kern, grid2, dim3(512), lds2, s, p);
        IPK_LAUNCH_CHECK();
      }
    }
    return IPOKE_OK;
  }
  IPK_REQUIRE(p.ad_p == nullptr, "Adam in the weight-gradient epilogue needs the LDS-DMA kernel (bf16, dense 16-byte aligned operands)");
  dim3 grid((unsigned)(p.tiles_n * p.tiles_k), (unsigned)p.splitm, (unsigned)nbatch);
  auto kern = igemm_tn_kernel<T, 2>;      // measured: 2 stages in flight beat 4 (54 vs 61 us at the NICE conv2 shape)
  IPK_SET_LDS_ONCE(kern, lds);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, p);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

}  // namespace ipoke

using namespace ipoke;

/* Test hook: moves a kernel-dispatch switch at run time ("c64" / "halo16": 0 off, 1 default rule, 2 wherever the kernel can run;
 * "nn128" / "nt128": 2 = the K-major / N-major GEMM on its 128 x 128 tile at any M; value < 0 goes back to the default rule 1;
 * "cpl_split": 4 / 8 / 16 / 32 K slices for ipoke_conv3x3_coupling where tiles x slices <= 256 and slices <= Kc / 64, < 0 the default rule). */
extern "C" int ipoke_set_dispatch_override(const char* name, int value) {
  IPK_REQUIRE(name != nullptr, "bad arguments");
  if (!strcmp(name, "cpl_split")) {
    IPK_REQUIRE(value < 0 || value == 4 || value == 8 || value == 16 || value == 32, "cpl_split: 4, 8, 16 or 32 slices (< 0: the default rule)");
    g_cpl_split.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    return IPOKE_OK;
  }
  IPK_REQUIRE(value <= 2, "bad arguments");
  std::atomic<int>* slot = !strcmp(name, "c64") ? &g_c64_mode : (!strcmp(name, "halo16") ? &g_halo16_mode : (!strcmp(name, "nn128") ? &g_nn128_mode :
                           (!strcmp(name, "nt128") ? &g_nt128_mode : nullptr)));
  IPK_REQUIRE(slot != nullptr, "unknown dispatch switch (c64 | halo16 | nn128 | nt128 | cpl_split)");
  slot->store(value < 0 ? 1 : value, std::memory_order_relaxed);
  return IPOKE_OK;
}

extern "C" int ipoke_last_conv_kernel(void) { return g_last_kernel; }
extern "C" int ipoke_last_wgrad_kernel(void) { return g_last_wgrad_kernel; }

namespace ipoke {
// descriptor -> kernel parameters (validation shared by ipoke_conv_forward and ipoke_conv3x3_coupling)
static int conv_params(NtParams& p, const ipoke_conv_desc* d, int dtype) {
  IPK_REQUIRE(d != nullptr, "null descriptor");
  IPK_REQUIRE(dtype == IPOKE_F32 || dtype == IPOKE_BF16, "bad dtype");
  const int esz = dtype == IPOKE_BF16 ? 2 : 4, e16 = 16 / esz;
  int rc = make_geom(p.g, d->NB, d->Di, d->Hi, d->Wi, d->Do, d->Ho, d->Wo, d->kd, d->kh, d->kw, d->sd, d->sh, d->sw,
                     d->pd, d->ph, d->pw, d->transposed);
  if (rc) return rc;
  IPK_REQUIRE(d->A && d->W && d->C, "null tensor");
  IPK_REQUIRE(d->Kc % e16 == 0 && d->Kc >= d->Kc_real && d->Kc_real > 0, "Kc must be a padded multiple of 16 bytes");
  if (!d->a_f32) {
    IPK_REQUIRE(d->a_sc == 1, "dtype activations must be channels-last");
    IPK_REQUIRE(d->Kc_real % e16 == 0 && d->a_coff % e16 == 0, "dtype activations need 16-byte aligned channel runs");
    IPK_REQUIRE(d->a_sn % e16 == 0 && d->a_sd % e16 == 0 && d->a_sh % e16 == 0 && d->a_sw % e16 == 0,
                "dtype activations need 16-byte aligned rows");
    IPK_REQUIRE(((uintptr_t)d->A & 15) == 0, "A must be 16-byte aligned");
  }
  IPK_REQUIRE(d->ldw % e16 == 0 && ((uintptr_t)d->W & 15) == 0, "weights need 16-byte aligned rows");
  IPK_REQUIRE(d->w_kmajor ? d->ldw >= d->Nout : (d->ldw >= round_up(p.g.taps * d->Kc, e16) || d->ldw >= p.g.taps * d->Kc), "ldw too small");
  p.A = d->A; p.a_f32 = d->a_f32; p.a_sn = d->a_sn; p.a_sd = d->a_sd; p.a_sh = d->a_sh; p.a_sw = d->a_sw; p.a_sc = d->a_sc;
  p.a_coff = d->a_coff; p.Kc_real = d->Kc_real; p.Kc = d->Kc;
  p.W = d->W; p.ldw = d->ldw; p.Nout = d->Nout; p.Ktot = p.g.taps * d->Kc;
  p.bias = d->bias; p.act = d->act; p.dact = d->dact; p.ld_dact = d->ld_dact; p.dact_act = d->dact_act;
  p.C = d->C; p.c_f32 = d->c_f32; p.c_acc = d->c_accumulate; p.ldc = d->ldc; p.c_coff = d->c_coff;
  p.c_cstride = d->c_cstride <= 0 ? 1 : d->c_cstride;
  p.splitk = d->splitk < 1 ? 1 : d->splitk;
  p.c_scatter = d->c_scatter; p.c_sn = d->c_sn; p.c_sd = d->c_sd; p.c_sh = d->c_sh; p.c_sw = d->c_sw; p.c_row0 = d->c_row0;
  p.row_scale = d->row_scale; p.rs_images = d->rs_images; p.rs_stride = d->rs_stride < 1 ? 1 : d->rs_stride;
  if (d->row_scale) IPK_REQUIRE(p.splitk == 1 && !d->c_accumulate && d->rs_images >= 1, "row scale: plain stores, rs_images >= 1");
  if (d->c_scatter) IPK_REQUIRE(p.splitk == 1 && !d->dact && !d->c_accumulate && d->c_row0 >= 0 && (p.g.Do == 1 || d->c_sd > 0), "output scatter: plain stores; maps with depth need c_sd");
  p.n_pad = d->Nout;
  if (!d->c_f32 && p.splitk == 1) {
    const long lim = d->ldc - d->c_coff;
    p.n_pad = (int)(round_up(d->Nout, e16) < lim ? round_up(d->Nout, e16) : lim);
  }
  p.acc_cnt = nullptr; p.acc_part = nullptr; p.acc_part_bytes = 0;
  if (p.splitk > 1 && d->c_accumulate) {
    IPK_REQUIRE(d->c_f32 && !d->bias && d->act == IPOKE_ACT_NONE && !d->dact, "split-K accumulates raw fp32 sums only");
    if (d->acc_scratch) {
      IPK_REQUIRE(((uintptr_t)d->acc_scratch & 15) == 0 && d->acc_scratch_bytes > kAccCounterBytes && d->Nout <= 64,
                  "bad accumulation scratch (16-byte aligned, ipoke_conv_acc_scratch_bytes; Nout <= 64)");
      p.acc_cnt = reinterpret_cast<unsigned*>(d->acc_scratch);
      p.acc_part = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(d->acc_scratch) + kAccCounterBytes);
      p.acc_part_bytes = d->acc_scratch_bytes - kAccCounterBytes;
    }
  } else if (p.splitk > 1) {
    IPK_REQUIRE(d->ldc % 4 == 0 && d->ldc >= d->Nout, "split-K partials need ldc >= Nout, multiple of 4");
  } else if (!d->c_f32) {
    IPK_REQUIRE(p.c_cstride == 1 && !d->c_accumulate, "dtype outputs are dense, non-accumulating");
  }
  return IPOKE_OK;
}
}  // namespace ipoke

extern "C" int ipoke_conv_forward(const ipoke_conv_desc* d, int dtype, void* stream) {
  NtParams p;
  int rc = conv_params(p, d, dtype); if (rc) return rc;
  const int esz = dtype == IPOKE_BF16 ? 2 : 4;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // s_setprio(2) in the chain's GEMMs: their waves win the issue arbitration against the co-resident weight-gradient /
  // optimizer waves of the side streams (64.6 -> 63.3 ms per step; levels 1 / 2 / 3 measure the same)
  p.prio = 2;
  const bool square = p.g.taps == 1 && d->Nout == p.Ktot && d->Nout >= 1024 && p.splitk == 1;
  TimedScope ts(square ? (d->w_kmajor ? IPOKE_TAG_NN_SQUARE : IPOKE_TAG_NT_SQUARE) : IPOKE_TAG_CONV_BASE, s);
  p.w_kmajor = d->w_kmajor;
  static const bool clog = getenv("IPOKE_CONV_LOG") != nullptr;      // developer probe: every call timed on its own (serialises the stream)
  hipEvent_t le0 = nullptr, le1 = nullptr;
  if (clog) { IPK_HIP(hipEventCreate(&le0)); IPK_HIP(hipEventCreate(&le1)); IPK_HIP(hipEventRecord(le0, s)); }
  if (p.w_kmajor) {
    IPK_REQUIRE(dtype == IPOKE_BF16, "K-major weights: bf16 only (the f32 mode keeps its transposed shadows)");
    g_last_kernel = IPOKE_KERNEL_IGEMM;
    rc = dispatch_nn(p, s);
  } else {
    rc = dtype == IPOKE_BF16 ? dispatch_nt<bf16_t>(p, s) : dispatch_nt<float>(p, s);
  }
  if (clog) {
    IPK_HIP(hipEventRecord(le1, s)); IPK_HIP(hipEventSynchronize(le1));
    float ms = 0.f; IPK_HIP(hipEventElapsedTime(&ms, le0, le1));
    const double st2 = p.g.transposed ? (double)p.g.sd * p.g.sh * p.g.sw : 1.0;
    fprintf(stderr, "CONV kern=%d tr=%d NB=%d in=%dx%dx%d out=%dx%dx%d k=%dx%dx%d s=%d,%d,%d Kc=%d Nout=%d a_f32=%d c_f32=%d splitk=%d scat=%d rs=%d M=%ld GF=%.2f us=%.1f\n",
            g_last_kernel, d->transposed, d->NB, d->Di, d->Hi, d->Wi, d->Do, d->Ho, d->Wo, d->kd, d->kh, d->kw, d->sd, d->sh, d->sw, d->Kc_real, d->Nout,
            d->a_f32, d->c_f32, p.splitk, d->c_scatter, d->row_scale != nullptr, (long)p.g.M,
            2e-9 * p.g.M * d->Nout * (double)p.g.taps * d->Kc_real / st2, ms * 1e3);
    (void)hipEventDestroy(le0); (void)hipEventDestroy(le1);
  }
  if (ts.slot >= 0) {          // algorithmic work of this launch (timing runs only)
    const GeomDev& g = p.g;
    const double stride = g.transposed ? (double)g.sd * g.sh * g.sw : 1.0;
    const double flops = 2.0 * g.M * d->Nout * (double)g.taps * d->Kc_real / stride;
    const double in_rows = (double)d->NB * g.Di * g.Hi * g.Wi;
    const double bytes = in_rows * d->Kc_real * (d->a_f32 ? 4 : esz) + (double)d->Nout * g.taps * d->Kc_real * esz +
                         (double)g.M * d->Nout * (d->c_f32 ? 4 : esz) * (p.splitk > 1 && !d->c_accumulate ? p.splitk : 1);
    ts.annotate(square ? 0 : IPOKE_TAG_CONV_BASE + g_last_kernel, flops, bytes);
  }
  return rc;
}

extern "C" int ipoke_conv_pair_dgrad_applicable(int M, int hidden, int cin, int dtype, int64_t acc_scratch_bytes) {
  if (dtype != IPOKE_BF16 || M < 64 || M % 64 != 0 || hidden < 256 || hidden % 128 != 0 || cin < 1 || cin > 32) return 0;
  const long tiles = (long)ceil_div(M, 128) * (hidden / 128);
  if (tiles > 256) return 0;                               // one round of workgroups
  return acc_scratch_bytes >= kAccCounterBytes + tiles * 128 * 32 * 4 ? 1 : 0;
}

extern "C" int ipoke_conv_pair_dgrad(const ipoke_conv_desc* conv2, const ipoke_conv_desc* conv1, int dtype, void* stream) {
  IPK_REQUIRE(conv2 != nullptr && conv1 != nullptr, "null descriptor");
  IPK_REQUIRE(dtype == IPOKE_BF16, "the fused data gradients are bf16 only");
  NtParams p, p1;
  int rc = conv_params(p, conv2, dtype); if (rc) return rc;
  rc = conv_params(p1, conv1, dtype); if (rc) return rc;
  const GeomDev& g = p.g; const GeomDev& g1 = p1.g;
  IPK_REQUIRE(conv2->w_kmajor && g.taps == 1 && !g.transposed && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 && g.ph == 0 && g.pw == 0 &&
              !p.a_f32 && p.Kc == p.Kc_real && p.Kc % 64 == 0 && (p.a_coff & 7) == 0 && (p.a_sw & 7) == 0 && (p.ldw & 7) == 0 &&
              p.ldw >= p.Nout && p.splitk == 1 && !p.c_scatter && p.a_sh == (long)g.Wi * p.a_sw && p.a_sn == (long)g.Hi * g.Wi * p.a_sw &&
              (long)g.M * p.a_sw + p.Kc < (1L << 31) && (long)p.Ktot * p.ldw < (1L << 31),
              "conv2: K-major weights, 1x1 kernel over dense bf16 channels-last rows, K a multiple of 64");
  IPK_REQUIRE(!p.bias && p.act == IPOKE_ACT_NONE && !p.c_f32 && !p.row_scale && ((p.ldc | p.c_coff) & 3) == 0 && p.ldc >= p.c_coff + p.Nout &&
              (!p.dact || ((p.ld_dact & 3) == 0 && p.dact_act == IPOKE_ACT_ELU && p.ld_dact >= p.Nout)) &&
              (long)g.M * p.ldc < (1L << 31) && (long)g.M * p.ld_dact < (1L << 31),
              "conv2: dense dtype output, no bias / activation, an ELU derivative mask at most");
  IPK_REQUIRE(!p1.c_scatter && !p1.a_f32 && g1.taps == 9 && g1.khw == 9 && g1.kw == 3 && g1.Di == 1 && g1.Hi == 8 && g1.Wi == 8 &&
              g1.lDo == 0 && g1.lHo == 3 && g1.lWo == 3 && g1.sd == 1 && g1.sh == 1 && g1.sw == 1 && g1.pd == 0 && g1.ph == 1 && g1.pw == 1 &&
              g1.M == g.M && p1.Kc == p.Nout && p1.Kc_real == p1.Kc && p1.ldw >= p1.Ktot && (long)p1.Nout * p1.ldw < (1L << 31),
              "conv1: 3x3 kernel, padding 1, on the 8x8 latent over conv2's output channels");
  IPK_REQUIRE(p1.A == p.C && p1.a_coff == p.c_coff && p1.a_sw == p.ldc && p1.a_sh == 8 * p.ldc && p1.a_sn == 64 * p.ldc,
              "conv1 reads conv2's output (same pointer, column offset and row stride)");
  IPK_REQUIRE(p1.c_f32 && p1.c_acc && !p1.bias && p1.act == IPOKE_ACT_NONE && !p1.dact && !p1.row_scale,
              "conv1 accumulates raw fp32 sums");
  IPK_REQUIRE(conv1->acc_scratch != nullptr && ((uintptr_t)conv1->acc_scratch & 15) == 0,
              "conv1 needs the accumulation scratch (ipoke_conv_acc_scratch_bytes / _init), 16-byte aligned");
  IPK_REQUIRE(ipoke_conv_pair_dgrad_applicable(g.M, p.Nout, p1.Nout, dtype, conv1->acc_scratch_bytes),
              "shape not taken by the fused launch (ipoke_conv_pair_dgrad_applicable)");
  IPK_REQUIRE(kLdsPair <= device_max_lds(), "the fused launch needs 156 KB of LDS per workgroup");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  p.prio = 2;                                              // (as ipoke_conv_forward: the chain's GEMMs win the issue arbitration)
  p.w_kmajor = 1;
  g_last_kernel = IPOKE_KERNEL_IGEMM;                      // ipoke_last_conv_kernel: the GEMM family, as for the conv2 launch this replaces
  PairEpi e;
  e.W1 = p1.W; e.ldw1 = p1.ldw; e.cin = p1.Nout; e.transposed = g1.transposed;
  e.C2 = reinterpret_cast<float*>(p1.C); e.ldc2 = p1.ldc; e.c_coff2 = p1.c_coff; e.c_cstride2 = p1.c_cstride;
  e.acc_cnt = reinterpret_cast<unsigned*>(conv1->acc_scratch);
  e.acc_part = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(conv1->acc_scratch) + kAccCounterBytes);
  p.tiles_m = ceil_div(g.M, 128); p.tiles_n = p.Nout / 128;
  p.splitk = 1; p.kb_per_split = ceil_div(p.Ktot, 64);
  pick_xcd_map(p);
  // tagged as ipoke_conv_forward tags the conv2 data gradient: that family's time now includes conv1's data gradient
  const bool square = p.Nout == p.Ktot && p.Nout >= 1024;
  TimedScope ts(square ? IPOKE_TAG_NN_SQUARE : IPOKE_TAG_CONV_BASE, s);
  auto kern = igemm_nn_pair_kernel;
  IPK_SET_LDS_ONCE(kern, kLdsPair);
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)p.tiles_m * p.tiles_n)), dim3(512), kLdsPair, s, p, e);
  IPK_LAUNCH_CHECK();
  if (ts.slot >= 0)
    ts.annotate(square ? 0 : IPOKE_TAG_CONV_BASE + IPOKE_KERNEL_IGEMM, 2.0 * g.M * p.Nout * ((double)p.Kc + 9.0 * p1.Nout),
                2.0 * ((double)g.M * p.Kc + (double)p.Nout * p.Kc + (double)g.M * p.Nout + 9.0 * p1.Nout * p.Nout) + 4.0 * g.M * p1.Nout);
  return IPOKE_OK;
}

extern "C" int ipoke_conv_pair_coupling_applicable(int M, int hidden, int nout3, int dtype) {
  if (dtype != IPOKE_BF16 || M < 64 || M % 64 != 0 || nout3 < 2 || nout3 > 64) return 0;
  if (hidden != 512 && hidden != 1024 && hidden != 2048 && hidden != 4096) return 0;      // 4, 8, 16 or 32 slices of 128 channels
  return (long)ceil_div(M, 128) * (hidden / 128) <= 256 ? 1 : 0;                            // one round of workgroups
}

namespace ipoke {
template <int NSPLIT>
static int launch_nt_coupling(const NtParams& p, const NtCplEpi& q3, const CouplingEpi& e, hipStream_t s) {
  auto kern = igemm_nt_coupling_kernel<NSPLIT>;
  IPK_SET_LDS_ONCE(kern, kLdsNtCpl);
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * NSPLIT)), dim3(512), kLdsNtCpl, s, p, q3, e);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
}  // namespace ipoke

extern "C" int ipoke_conv_pair_coupling(const ipoke_conv_desc* conv2, const ipoke_conv_desc* conv3, const ipoke_affine_desc* a,
                                        const ipoke_coupling_epi* ep, int B, int dtype, void* stream) {
  IPK_REQUIRE(conv2 && conv3 && a && ep, "null descriptor");
  IPK_REQUIRE(dtype == IPOKE_BF16, "the fused conv2 + conv3 + coupling launch is bf16 only");
  IPK_REQUIRE(ep->xchg != nullptr && ((uintptr_t)ep->xchg & 15) == 0, "exchange scratch missing (ipoke_conv3x3_coupling_xchg_bytes / _init)");
  const bool store_h2 = conv2->C != nullptr;
  // conv_params wants non-null tensors: without a stored h2 neither conv2->C nor conv3->A is ever dereferenced
  ipoke_conv_desc d2 = *conv2, d3 = *conv3;
  if (!store_h2) { d2.C = ep->xchg; d2.ldc = d2.Nout; d2.c_coff = 0; d3.A = ep->xchg; }
  d3.C = ep->xchg; d3.c_f32 = 1; d3.ldc = 64; d3.splitk = 1; d3.c_accumulate = 0;       // (no partial-sum slabs: validation only)
  NtParams p, p3;
  int rc = conv_params(p, &d2, dtype); if (rc) return rc;
  rc = conv_params(p3, &d3, dtype); if (rc) return rc;
  const GeomDev& g = p.g; const GeomDev& g3 = p3.g;
  IPK_REQUIRE(!d2.w_kmajor && g.taps == 1 && !g.transposed && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.pd == 0 && g.ph == 0 && g.pw == 0 &&
              !p.a_f32 && p.Kc == p.Kc_real && p.Kc % 64 == 0 && p.Kc >= 128 && (p.a_coff & 7) == 0 && (p.a_sw & 7) == 0 && (p.ldw & 7) == 0 &&
              p.ldw >= p.Ktot && p.splitk == 1 && !p.c_scatter && p.a_sh == (long)g.Wi * p.a_sw && p.a_sn == (long)g.Hi * g.Wi * p.a_sw &&
              (long)g.M * p.a_sw + p.Kc < (1L << 31) && (long)p.Nout * p.ldw < (1L << 31),
              "conv2: N-major weights, 1x1 kernel over dense bf16 channels-last rows, K a multiple of 64");
  IPK_REQUIRE(p.act == IPOKE_ACT_ELU && !p.dact && !p.c_f32 && !p.c_acc && !p.row_scale && (!p.bias || ((uintptr_t)p.bias & 15) == 0),
              "conv2: bias (16-byte aligned) + ELU into a dense dtype output");
  IPK_REQUIRE(!store_h2 || (((p.ldc | p.c_coff) & 3) == 0 && p.ldc >= p.c_coff + p.Nout && ((uintptr_t)p.C & 7) == 0 && (long)g.M * p.ldc < (1L << 31)),
              "conv2: h2 rows are 8-byte aligned, ldc >= c_coff + Nout");
  IPK_REQUIRE(!d3.bias && d3.act == IPOKE_ACT_NONE && !d3.dact && !d3.row_scale && !d3.w_kmajor, "conv3 of a coupling: raw sums only (the bias is the coupling's)");
  IPK_REQUIRE(s8_shape(p3) && g3.M == 64 * B && g3.M == g.M && !g3.transposed, "conv3: the skinny 3x3 convolution of a coupling net on 8x8 maps, conv2's rows");
  IPK_REQUIRE(p3.Kc == p.Nout, "conv3 reads exactly conv2's output channels (a wider input takes the two launches)");
  IPK_REQUIRE(!store_h2 || (p3.A == p.C && p3.a_coff == p.c_coff && p3.a_sw == p.ldc && p3.a_sh == 8 * p.ldc && p3.a_sn == 64 * p.ldc),
              "conv3 reads conv2's output (same pointer, column offset and row stride)");
  IPK_REQUIRE(a->Cp >= 1 && 2 * a->Cp == d3.Nout && a->t_stride >= 1 && a->P == 64 && a->ld >= 1 && a->ld <= 256 &&
              a->t_off >= 0 && a->t_off + (a->Cp - 1) * a->t_stride < a->ld, "bad coupling geometry");
  IPK_REQUIRE(ep->mode >= 0 && ep->mode <= 2 && ep->in, "bad mode / null input state");
  IPK_REQUIRE(ep->mode == 1 ? (ep->out2 && ep->out2 != ep->in && ep->an_C >= 1 && ep->an_c0 >= 0 && ep->an_c0 + ep->an_C <= a->ld &&
                               (ep->an_log_scale == nullptr) == (ep->an_bias == nullptr) && !ep->ext)
                            : (ep->out != nullptr), "bad outputs");
  IPK_REQUIRE(!ep->logdet_slot || ep->slot_stride >= 4, "log-det slots are 4 wide (one per 16-row slice of a sample)");
  IPK_REQUIRE(!ep->ext || ep->ext_ld >= a->Cp, "bad extra operand output");
  IPK_REQUIRE(ipoke_conv_pair_coupling_applicable(g.M, p.Nout, p3.Nout, dtype),
              "shape not taken by the fused launch (ipoke_conv_pair_coupling_applicable)");
  IPK_REQUIRE(kLdsNtCpl <= device_max_lds(), "the fused launch needs 138 KB of LDS per workgroup");
  CouplingEpi e{};
  e.bias = a->bias; e.in = ep->in; e.out = ep->out; e.out2 = ep->mode == 1 ? ep->out2 : nullptr;
  e.scale_out = ep->mode == 2 ? nullptr : ep->scale_out; e.logdet_slot = ep->mode == 2 ? nullptr : ep->logdet_slot;
  e.an_ls = ep->an_log_scale; e.an_bias = ep->an_bias; e.an_idx = ep->an_idx; e.ext = ep->ext; e.xchg = ep->xchg;
  e.xchg_bytes = (int)ipoke_conv3x3_coupling_xchg_bytes(); e.slot_stride = ep->slot_stride < 1 ? 1 : ep->slot_stride;
  e.Cp = a->Cp; e.t_off = a->t_off; e.t_stride = a->t_stride; e.ld = a->ld; e.mode = ep->mode; e.an_c0 = ep->an_c0; e.an_C = ep->an_C;
  e.ext_ld = ep->ext_ld; e.ext_bf16 = 1;
  auto log2_or = [](int v) { int sh = 0; while ((1 << sh) < v) ++sh; return (1 << sh) == v ? sh : -1; };
  e.ld_sh = log2_or(a->ld); e.cp_sh = log2_or(a->Cp); e.ts_sh = log2_or(a->t_stride);
  NtCplEpi q3; q3.W3 = p3.W; q3.ldw3 = p3.ldw; q3.nout3 = p3.Nout;
  if (!store_h2) p.C = nullptr;
  p.prio = 2;                                              // (as ipoke_conv_forward: the chain's GEMMs win the issue arbitration)
  p.w_kmajor = 0;
  p.tiles_m = ceil_div(g.M, 128); p.tiles_n = p.Nout / 128; p.xa = p.xb = 0;      // block = tile * slices + slice: no XCD map
  p.splitk = 1; p.kb_per_split = p.Ktot / 64;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  g_last_kernel = IPOKE_KERNEL_IGEMM;                      // ipoke_last_conv_kernel: the GEMM family, as for the conv2 launch this replaces
  // tagged as ipoke_conv_forward tags conv2: that family's time now includes conv3 and the coupling
  const bool square = p.Nout == p.Ktot && p.Nout >= 1024;
  TimedScope ts(square ? IPOKE_TAG_NT_SQUARE : IPOKE_TAG_CONV_BASE, s);
  switch (p.tiles_n) {
    case 4: rc = launch_nt_coupling<4>(p, q3, e, s); break;
    case 8: rc = launch_nt_coupling<8>(p, q3, e, s); break;
    case 16: rc = launch_nt_coupling<16>(p, q3, e, s); break;
    default: rc = launch_nt_coupling<32>(p, q3, e, s); break;
  }
  if (rc) return rc;
  if (ts.slot >= 0)
    ts.annotate(square ? 0 : IPOKE_TAG_CONV_BASE + IPOKE_KERNEL_IGEMM, 2.0 * g.M * p.Nout * ((double)p.Kc + 9.0 * p3.Nout),
                2.0 * ((double)g.M * p.Kc + (double)p.Nout * p.Kc + (store_h2 ? (double)g.M * p.Nout : 0.0) + 9.0 * p3.Nout * p.Nout) +
                    8.0 * g.M * a->ld);
  return IPOKE_OK;
}

static int fill_tn(TnParams& p, const ipoke_wgrad_desc* d, int dtype, bool batched) {
  IPK_REQUIRE(d != nullptr, "null descriptor");
  IPK_REQUIRE(dtype == IPOKE_F32 || dtype == IPOKE_BF16, "bad dtype");
  const int esz = dtype == IPOKE_BF16 ? 2 : 4, e16 = 16 / esz;
  int rc = make_geom(p.g, d->NB, d->Di, d->Hi, d->Wi, d->Do, d->Ho, d->Wo, d->kd, d->kh, d->kw, d->sd, d->sh, d->sw,
                     d->pd, d->ph, d->pw, d->transposed);
  if (rc) return rc;
  IPK_REQUIRE(batched || (d->A && d->dY && d->dW), "null tensor");
  IPK_REQUIRE(d->Kc % e16 == 0 && d->Kc >= d->Kc_real && d->Kc_real > 0, "Kc must be a padded multiple of 16 bytes");
  if (!d->a_f32) {
    IPK_REQUIRE(d->a_sc == 1 && d->Kc_real % e16 == 0 && d->a_coff % e16 == 0, "dtype activations: aligned channels-last");
    IPK_REQUIRE(d->a_sn % e16 == 0 && d->a_sd % e16 == 0 && d->a_sh % e16 == 0 && d->a_sw % e16 == 0, "aligned rows");
  }
  IPK_REQUIRE(d->ldy % e16 == 0 && d->y_coff % e16 == 0 && ((uintptr_t)d->dY & 15) == 0, "dY rows must be 16-byte aligned");
  IPK_REQUIRE(d->y_coff + round_up(d->Nout, e16) <= d->ldy, "dY pitch must cover the padded channel count");
  p.batch = nullptr; p.a_base = nullptr; p.y_base = nullptr; p.w_base = nullptr;
  p.A = d->A; p.a_f32 = d->a_f32; p.a_sn = d->a_sn; p.a_sd = d->a_sd; p.a_sh = d->a_sh; p.a_sw = d->a_sw; p.a_sc = d->a_sc;
  p.a_coff = d->a_coff; p.Kc_real = d->Kc_real; p.Kc = d->Kc;
  p.dY = d->dY; p.ldy = d->ldy; p.y_coff = d->y_coff; p.Nout = d->Nout; p.Ktot = p.g.taps * d->Kc;
  p.dW = d->dW; p.w_sn = d->w_sn; p.w_sc = d->w_sc; p.w_st = d->w_st; p.accumulate = d->accumulate;
  p.splitm = d->splitm < 1 ? 1 : d->splitm;
  p.split_stride = d->split_stride;
  p.tile0 = 0; p.z0 = 0; p.max_wgs = d->max_workgroups;
  IPK_REQUIRE(p.split_stride >= 0 && !(p.split_stride > 0 && d->accumulate), "split slabs are stored, not accumulated");
  p.Kc_store = d->Kc_store > 0 ? d->Kc_store : d->Kc_real;
  IPK_REQUIRE(p.Kc_store <= d->Kc_real, "Kc_store exceeds Kc_real");
  p.ad_p = p.ad_m = p.ad_v = p.ad_vmax = nullptr; p.ad_sh = nullptr; p.ad_h = AdamHyper{}; p.ad_keep_grad = 0;
  if (d->adam) {
    const ipoke_wgrad_adam& a = *d->adam;
    IPK_REQUIRE(batched && dtype == IPOKE_BF16 && a.params && a.m && a.v && a.vmax && a.operand && a.step >= 1,
                "Adam in the weight-gradient epilogue: batched bf16 launches, all five buffers, step >= 1");
    IPK_REQUIRE(((reinterpret_cast<uintptr_t>(a.params) | reinterpret_cast<uintptr_t>(a.m) | reinterpret_cast<uintptr_t>(a.v) |
                  reinterpret_cast<uintptr_t>(a.vmax)) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.operand) & 7) == 0, "unaligned optimizer buffers");
    p.ad_p = a.params; p.ad_m = a.m; p.ad_v = a.v; p.ad_vmax = a.vmax; p.ad_sh = reinterpret_cast<bf16_t*>(a.operand);
    p.ad_h = adam_make_hyper(a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step, a.grad_scale);
    p.ad_keep_grad = a.keep_grad;
  }
  return IPOKE_OK;
}

extern "C" int ipoke_conv_wgrad(const ipoke_wgrad_desc* d, int dtype, void* stream) {
  TnParams p;
  int rc = fill_tn(p, d, dtype, false); if (rc) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool square = p.g.taps == 1 && d->Nout == p.Ktot && d->Nout >= 1024;
  TimedScope ts(square ? IPOKE_TAG_TN_SQUARE : IPOKE_TAG_WGRAD, s);
  if (ts.slot >= 0) {
    const int esz = dtype == IPOKE_BF16 ? 2 : 4;
    const double in_rows = (double)d->NB * d->Di * d->Hi * d->Wi;
    ts.annotate(0, 2.0 * p.g.M * d->Nout * (double)p.g.taps * d->Kc_real,
                (double)p.g.M * d->Nout * esz + in_rows * d->Kc_real * (d->a_f32 ? 4 : esz) + (double)d->Nout * p.g.taps * d->Kc_real * 4 * p.splitm);
  }
  static const bool wlog = getenv("IPOKE_WGRAD_LOG") != nullptr;      // developer probe: every call timed on its own (serialises the stream)
  if (wlog) {
    hipEvent_t e0, e1;
    IPK_HIP(hipEventCreate(&e0)); IPK_HIP(hipEventCreate(&e1));
    IPK_HIP(hipEventRecord(e0, s));
    rc = dtype == IPOKE_BF16 ? launch_tn<bf16_t>(p, s) : launch_tn<float>(p, s);
    IPK_HIP(hipEventRecord(e1, s)); IPK_HIP(hipEventSynchronize(e1));
    float ms = 0.f; IPK_HIP(hipEventElapsedTime(&ms, e0, e1));
    fprintf(stderr, "WGRAD NB=%d in=%dx%dx%d out=%dx%dx%d k=%dx%dx%d s=%d,%d,%d Kc=%d Nout=%d a_f32=%d splitm=%d M=%ld GF=%.2f us=%.1f\n", d->NB, d->Di, d->Hi,
            d->Wi, d->Do, d->Ho, d->Wo, d->kd, d->kh, d->kw, d->sd, d->sh, d->sw, d->Kc_real, d->Nout, d->a_f32, p.splitm, (long)p.g.M,
            2e-9 * p.g.M * d->Nout * (double)p.g.taps * d->Kc_real, ms * 1e3);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return rc;
  }
  return dtype == IPOKE_BF16 ? launch_tn<bf16_t>(p, s) : launch_tn<float>(p, s);
}

/* Reduction splits (slabs) the kernel that ipoke_conv_wgrad will dispatch this problem to prefers when the caller aims at `target_workgroups`
 * workgroups: > 0 for the halo-staged 3x3 / 3x3x3 kernel (its tiles are 64 x 64 x 9 taps per depth tap), 0 = no preference (the caller's own
 * rule for the 128 x 128 tiles of the implicit GEMM).  d->splitm / split_stride / dW are ignored. */
extern "C" int ipoke_conv_wgrad_splitm(const ipoke_wgrad_desc* d, int dtype, int target_workgroups) {
  if (!d || dtype != IPOKE_BF16 || target_workgroups < 1) return 0;
  ipoke_wgrad_desc t = *d;
  t.splitm = 2; t.split_stride = 1; t.adam = nullptr;
  if (!t.dW) t.dW = reinterpret_cast<float*>(16);
  TnParams p;
  if (fill_tn(p, &t, dtype, false) != IPOKE_OK) return 0;
  if (!halo_wgrad_applicable(p)) return 0;
  return halo_wgrad_splits(p, target_workgroups);
}
extern "C" int ipoke_wgrad_batch_entry_size(void) { return (int)sizeof(TnBatchEntry); }

/* Batched weight gradients: `nbatch` problems of identical shape (all but the 2-D kernel extent / padding, which come
 * from the entry) in one launch.  entries_dev[i] = {a_off bytes, y_off bytes, w_off floats, kh, kw, ph, pw}. */
extern "C" int ipoke_conv_wgrad_batched(const ipoke_wgrad_desc* d, const void* entries_dev, int nbatch, const void* a_base,
                                        const void* y_base, float* w_base, int dtype, void* stream) {
  IPK_REQUIRE(entries_dev && nbatch >= 1 && a_base && y_base && w_base, "bad batch arguments");
  TnParams p;
  int rc = fill_tn(p, d, dtype, true); if (rc) return rc;
  p.batch = reinterpret_cast<const TnBatchEntry*>(entries_dev);
  p.a_base = reinterpret_cast<const unsigned char*>(a_base); p.y_base = reinterpret_cast<const unsigned char*>(y_base);
  p.w_base = w_base;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  TimedScope ts(p.g.taps == 1 && d->Nout == p.Ktot && d->Nout >= 1024 ? IPOKE_TAG_TN_SQUARE : 0, s, nbatch);
  return dtype == IPOKE_BF16 ? launch_tn<bf16_t>(p, s, nbatch) : launch_tn<float>(p, s, nbatch);
}

/* Benchmark helper: `n` back-to-back launches of the same convolution issued natively (no host round trips in between),
 * so that HIP events placed around the call measure kernel time rather than the caller's launch rate. */
extern "C" int ipoke_conv_forward_repeat(const ipoke_conv_desc* d, int dtype, int n, void* stream) {
  for (int i = 0; i < n; ++i) {
    const int rc = ipoke_conv_forward(d, dtype, stream);
    if (rc) return rc;
  }
  return IPOKE_OK;
}
