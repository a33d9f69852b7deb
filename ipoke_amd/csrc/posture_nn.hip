// Posture nearest neighbours (reference data/flow_dataset.py:628-713, get_nn with its `measure` at :635-646): for every query frame the
// nearest frame in posture space, D(i, j) = sum_k || kps[i][k] - kps[j][k] ||_2, once over all frames and once over the frames of other
// videos.  All pairs, a sum of square roots -- not a GEMM -- with the arg-min fused in, so that no N x N distance table exists.
//
// Grid: query blocks (256 queries, one per thread, keypoints in registers) x candidate chunks.  A workgroup walks its chunk in tiles of
// 64 candidates staged in LDS; every lane of a wave reads the same candidate keypoint at the same time, which the LDS serves as one
// broadcast (no bank conflict, one ds_read_b64 per term and wave), and the K terms are accumulated in index order in fp32 with every
// operation rounded on its own (no contraction).  A thread sees its candidates in ascending j, so a strict `<` keeps the lower index of a
// tie: the order is (D, j) lexicographic, that of a stable argsort.  Each workgroup writes per query its two smallest (D, j) and its
// smallest (D, j) of another video into the workspace; a second launch merges the chunks in ascending order with the same rule.  No
// atomics, no order that depends on scheduling: two runs are bit-identical.
#include "common.h"

#include <cmath>

using namespace ipoke;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {
constexpr int kQueries = 256;       // queries per workgroup = threads
constexpr int kTile = 64;           // candidates per LDS tile: 64 x 64 keypoints x 8 B = 32 KiB at the largest K
constexpr int kMaxChunks = 64;
constexpr int kTargetBlocks = 2048; // 8 workgroups per CU on 256 CUs before the chunk count stops growing
constexpr int kMaxK = 64;

struct NnGrid { int qblocks, chunks, chunk_len; };

// The chunk count grows until the grid holds kTargetBlocks workgroups; a chunk is a whole number of tiles (the last one is ragged).
NnGrid nn_grid(int N, int M) {
  NnGrid g;
  g.qblocks = (M + kQueries - 1) / kQueries;
  const long tiles = ((long)N + kTile - 1) / kTile;
  long want = (kTargetBlocks + g.qblocks - 1) / g.qblocks;
  if (want > kMaxChunks) want = kMaxChunks;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const long tiles_per_chunk = (tiles + want - 1) / want;
  g.chunk_len = (int)(tiles_per_chunk * kTile);
  g.chunks = (int)((tiles + tiles_per_chunk - 1) / tiles_per_chunk);
  return g;
}

struct NnArgs {
  const float2* kps; const int* vid; const long long* ids;
  int N, K, M, chunks, chunk_len;
  float* ws_d; int* ws_j;            // [3][chunks][M] each: smallest, second smallest, smallest of another video
};

__device__ __forceinline__ void keep_two(float d, int j, float& d1, int& j1, float& d2, int& j2) {
  const bool lt1 = d < d1, lt2 = d < d2;            // selects, not branches: the four values stay in registers
  d2 = lt1 ? d1 : lt2 ? d : d2; j2 = lt1 ? j1 : lt2 ? j : j2;
  d1 = lt1 ? d : d1; j1 = lt1 ? j : j1;
}

template <int KMAX>
__global__ __launch_bounds__(kQueries) void posture_nn_kernel(NnArgs a) {
  extern __shared__ float2 tile[];                  // [kTile][K] keypoints, then kTile video codes
  int* tile_vid = reinterpret_cast<int*>(tile + (size_t)kTile * a.K);
  const int tid = threadIdx.x, K = a.K;
  const int m = blockIdx.x * kQueries + tid;
  long long qi = -1;
  if (m < a.M) {
    qi = a.ids ? a.ids[m] : (long long)m;
    if (qi < 0 || qi >= a.N) qi = -1;               // an id outside the data set reads nothing and answers -1
  }
  float2 q[KMAX];
  int qvid = 0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) q[k] = make_float2(0.f, 0.f);
  if (qi >= 0) {
    qvid = a.vid[qi];
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) q[k] = a.kps[qi * K + k];
  }
  const float inf = INFINITY;
  float d1 = inf, d2 = inf, dv = inf;
  int j1 = -1, j2 = -1, jv = -1;
  const long c_begin = (long)blockIdx.y * a.chunk_len;
  const long c_end = min(c_begin + (long)a.chunk_len, (long)a.N);
  for (long t0 = c_begin; t0 < c_end; t0 += kTile) {
    const int nt = (int)min((long)kTile, c_end - t0);
    __syncthreads();                                // the previous tile has been read by every wave
    for (int e = tid; e < nt * K; e += kQueries) tile[e] = a.kps[t0 * K + e];
    if (tid < nt) tile_vid[tid] = a.vid[t0 + tid];
    __syncthreads();
    if (qi < 0) continue;
    for (int c = 0; c < nt; ++c) {
      const float2* ck = tile + c * K;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          const float2 p = ck[k];
          const float dx = __fsub_rn(q[k].x, p.x), dy = __fsub_rn(q[k].y, p.y);
          // sqrtf is the correctly rounded square root here (hipcc's default; __fsqrt_rn compiles to the bare 1-ulp v_sqrt_f32):
          // a perfect square gives its root exactly
          acc = __fadd_rn(acc, sqrtf(__fmaf_rn(dy, dy, __fmul_rn(dx, dx))));
        }
      }
      const int j = (int)(t0 + c);
      keep_two(acc, j, d1, j1, d2, j2);
      if (tile_vid[c] != qvid && acc < dv) { dv = acc; jv = j; }
    }
  }
  if (m < a.M) {
    const long plane = (long)a.chunks * a.M, o = (long)blockIdx.y * a.M + m;
    a.ws_d[o] = d1; a.ws_d[plane + o] = d2; a.ws_d[2 * plane + o] = dv;
    a.ws_j[o] = j1; a.ws_j[plane + o] = j2; a.ws_j[2 * plane + o] = jv;
  }
}

// chunks in ascending order, each chunk's entries in its own order: the same strict `<` as inside a chunk
__global__ void posture_nn_merge_kernel(const float* __restrict__ ws_d, const int* __restrict__ ws_j, int M, int chunks,
                                        long long* __restrict__ nn_general, long long* __restrict__ nn_other, float* __restrict__ dist) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const long plane = (long)chunks * M;
  float d1 = INFINITY, d2 = INFINITY, dv = INFINITY;
  int j1 = -1, j2 = -1, jv = -1;
  for (int c = 0; c < chunks; ++c) {
    const long o = (long)c * M + m;
    keep_two(ws_d[o], ws_j[o], d1, j1, d2, j2);
    keep_two(ws_d[plane + o], ws_j[plane + o], d1, j1, d2, j2);
    const float d = ws_d[2 * plane + o];
    if (d < dv) { dv = d; jv = ws_j[2 * plane + o]; }
  }
  nn_general[m] = j2;
  nn_other[m] = jv;
  if (dist) { dist[2 * m] = d2; dist[2 * m + 1] = dv; }
}

bool nn_shape_ok(int N, int K, int M) { return N >= 2 && K >= 1 && K <= kMaxK && M >= 1; }
}  // namespace

extern "C" size_t ipoke_posture_nn_workspace_bytes(int N, int K, int M) {
  if (!nn_shape_ok(N, K, M)) return 0;
  return (size_t)nn_grid(N, M).chunks * (size_t)M * 3 * (sizeof(float) + sizeof(int));
}

extern "C" int ipoke_posture_nn_grid(int N, int K, int M, int* out) {
  IPK_REQUIRE(out && nn_shape_ok(N, K, M), "N >= 2, 1 <= K <= 64, M >= 1");
  const NnGrid g = nn_grid(N, M);
  out[0] = g.qblocks; out[1] = g.chunks; out[2] = g.chunk_len; out[3] = kTile;
  return IPOKE_OK;
}

extern "C" int ipoke_posture_nn(const float* kps, const int32_t* vid, const int64_t* ids, int N, int K, int M, int64_t* nn_general,
                                int64_t* nn_other_vid, float* dist, void* ws, void* stream) {
  IPK_REQUIRE(kps && vid && nn_general && nn_other_vid && ws, "null argument");
  IPK_REQUIRE(N >= 2, "a nearest neighbour needs at least two frames");
  IPK_REQUIRE(K >= 1 && K <= kMaxK, "1 <= K <= 64 keypoints");
  IPK_REQUIRE(M >= 1 && (ids || M <= N), "M queries: ids, or without ids the frames 0 .. M-1 (M == N: all frames)");
  IPK_REQUIRE((reinterpret_cast<uintptr_t>(kps) & 7) == 0, "kps must be 8-byte aligned");
  const NnGrid g = nn_grid(N, M);
  IPK_REQUIRE(g.qblocks >= 1 && g.chunks >= 1 && g.chunks <= 65535, "grid out of range");
  NnArgs a;
  a.kps = reinterpret_cast<const float2*>(kps); a.vid = vid; a.ids = reinterpret_cast<const long long*>(ids);
  a.N = N; a.K = K; a.M = M; a.chunks = g.chunks; a.chunk_len = g.chunk_len;
  a.ws_d = reinterpret_cast<float*>(ws);
  a.ws_j = reinterpret_cast<int*>(a.ws_d + (size_t)3 * g.chunks * M);
  const dim3 grid(g.qblocks, g.chunks), block(kQueries);
  const size_t lds = (size_t)kTile * K * sizeof(float2) + kTile * sizeof(int);
  hipStream_t st = STREAM(stream);
  if (K <= 8) hipLaunchKernelGGL(posture_nn_kernel<8>, grid, block, lds, st, a);
  else if (K <= 17) hipLaunchKernelGGL(posture_nn_kernel<17>, grid, block, lds, st, a);
  else if (K <= 32) hipLaunchKernelGGL(posture_nn_kernel<32>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(posture_nn_kernel<64>, grid, block, lds, st, a);
  IPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(posture_nn_merge_kernel, dim3((M + 255) / 256), dim3(256), 0, st, a.ws_d, a.ws_j, M, g.chunks,
                     reinterpret_cast<long long*>(nn_general), reinterpret_cast<long long*>(nn_other_vid), dist);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
