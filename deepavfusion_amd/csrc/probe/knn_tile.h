// The 128 x 128 exact-fp32 score tile of the nearest-neighbour probe, shared by the two top-k kernels (knn.hip: lists of up to 8 in
// registers; knn_wide.hip: lists of up to 64 in the workspace).  Both call the same two functions below, so a score is the same
// fp32 FMA chain in the same order in either kernel, and their results can be compared bit for bit.
#pragma once
#include "common.h"

#define KNN_BQ 128         // queries per workgroup
#define KNN_BN 128         // bank rows per tile
#define KNN_BK 16          // d-slice through LDS
#define KNN_LDK 20         // padded LDS row of a d-slice (floats): ds_read_b128 of 16 rows x 4 groups without bank conflicts
#define KNN_LDS 130        // padded LDS row of the score tile

namespace {

struct KnnEntry { float v; int i; };

struct KnnArgs {
  const float* q[3];
  const float* x[3];
  long ldq, ldx;
  int M, Nq, N, D, V, k, tiles_per_split;
  KnnEntry* ws;
};

// strict total order: higher score first, ties to the lower bank index — the top-k set is then unique, whatever order the
// candidates arrive in, so the result does not depend on the bank split or on the query chunking
__device__ __forceinline__ bool knn_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// acc = scores of queries [q0, q0 + 128) x bank rows [n0, n0 + 128) in modality (Q, X), by a workgroup of four waves: each wave a
// 64 x 64 quarter as 4 x 4 blocks of 16 x 16 (one f32x4 accumulator each).  The d-loop streams 16-wide slices of queries and bank
// rows through LDS (the next slice's global loads in flight during the MFMAs).  Rows past Nq / N and columns past D read as 0.
__device__ __forceinline__ void knn_score_tile(const KnnArgs& p, const float* __restrict__ Q, const float* __restrict__ X, int q0,
                                               int n0, float* sA, float* sB, f32x4 (&acc)[4][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int g = lane >> 4, rr = lane & 15;
  const int D = p.D;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // thread loads 2 float4 of each operand per slice: element e = tid + 256 u -> row e / 4, columns 4 (e % 4) .. + 3
  f32x4 ra[2], rb[2];
  auto load = [&](int d0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + 256 * u, row = e >> 2, c = d0 + (e & 3) * 4;
      const int qr = q0 + row, nr = n0 + row;
      ra[u] = (qr < p.Nq && c < D) ? *(const f32x4*)(Q + (long)qr * p.ldq + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      rb[u] = (nr < p.N && c < D) ? *(const f32x4*)(X + (long)nr * p.ldx + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  load(0);
  for (int d0 = 0; d0 < D; d0 += KNN_BK) {
    __syncthreads();                        // every wave is done with the previous slice (and the previous view's scan)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + 256 * u, row = e >> 2, c = (e & 3) * 4;
      *(f32x4*)&sA[row * KNN_LDK + c] = ra[u];
      *(f32x4*)&sB[row * KNN_LDK + c] = rb[u];
    }
    __syncthreads();
    if (d0 + KNN_BK < D) load(d0 + KNN_BK);
    // lane (rr, g) holds d = d0 + 4 g + s of its row in element s: step s feeds k-slot g with that d, so every score is the
    // fp32 FMA chain over d in the fixed order (d0, s, g) — the same for every tile, split and query chunking
    f32x4 fa[4], fb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = *(const f32x4*)&sA[(wq + 16 * i + rr) * KNN_LDK + 4 * g];
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = *(const f32x4*)&sB[(wn + 16 * j + rr) * KNN_LDK + 4 * g];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
  }
}

// a finished tile -> sc[query row][bank column] in LDS, with a barrier on either side.  C/D layout of the MFMA: col = lane & 15
// (bank), row = 4 (lane >> 4) + reg (query)
__device__ __forceinline__ void knn_store_tile(float* sc, const f32x4 (&t)[4][4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wq = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int g = lane >> 4, rr = lane & 15;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) sc[(wq + 16 * i + 4 * g + e) * KNN_LDS + wn + 16 * j + rr] = t[i][j][e];
  __syncthreads();
}

}  // namespace
