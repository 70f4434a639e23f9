// Nearest-neighbour probe of the pre-training worker (util/knn_probe.py:102-131 of the reference): mean-pool + L2-normalise the
// encoder tokens, then score every query against every bank row in up to three modalities (+ their sum) and keep the top-k per row.
// The score matrix is never written: each workgroup holds a 128 x 128 tile of exact-fp32 MFMA scores (v_mfma_f32_16x16x4_f32) in
// LDS for one view at a time and folds it into per-row top-k lists kept in registers.
//
// This file sits below csrc/ on purpose: _lib.kernel_source_hash() covers csrc/*.hip and csrc/*.h only, and these kernels never run
// in the pre-training step whose PMC-measured traffic that hash certifies.
#include "common.h"
#include "dav_kernels.h"

#include "knn_tile.h"      // the 128 x 128 score tile, KnnEntry / KnnArgs, knn_better: shared with knn_wide.hip

namespace {

// insert (v, i) into the sorted list by a predicated swap chain (no dynamic register indexing); the last entry falls off
template <int KP>
__device__ __forceinline__ void knn_insert(float (&val)[KP], int (&idx)[KP], float v, int i) {
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const bool b = knn_better(v, i, val[j], idx[j]);
    const float tv = val[j];
    const int ti = idx[j];
    val[j] = b ? v : tv;
    idx[j] = b ? i : ti;
    v = b ? tv : v;
    i = b ? ti : i;
  }
}

template <int KP>
__device__ __forceinline__ void knn_offer(float (&val)[KP], int (&idx)[KP], float v, int i) {
  if (knn_better(v, i, val[KP - 1], idx[KP - 1])) knn_insert<KP>(val, idx, v, i);      // one compare for most candidates
}

__global__ __launch_bounds__(256) void mean_l2n_kernel(const float* __restrict__ x, int L, int D, long ld_row, long ld_batch,
                                                       float* __restrict__ out) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* xb = x + (long)b * ld_batch;
  float* ob = out + (long)b * D;
  float ss = 0.f;
  for (int d = tid; d < D; d += 256) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += xb[(long)l * ld_row + d];
    const float v = s / (float)L;
    ob[d] = v;
    ss = __builtin_fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float den = fmaxf(sqrtf((red[0] + red[1]) + (red[2] + red[3])), 1e-12f);      // F.normalize: v / max(||v||, eps)
  for (int d = tid; d < D; d += 256) ob[d] = ob[d] / den;
}

// One workgroup: KNN_BQ queries x the bank tiles [split * tiles_per_split, ...) of its split.  Four waves, each a 64 x 64
// quarter of the 128 x 128 score tile as 4 x 4 blocks of 16 x 16 (one f32x4 accumulator each).  Per tile and modality the
// d-loop streams 16-wide slices of queries and bank rows through LDS (the next slice's global loads in flight during the MFMAs);
// the finished scores go to LDS, and thread (row r = tid / 2, half h = tid % 2) offers the row's columns h, h + 2, ... to its
// list of that view.  The sum view (s_0 + s_1) + s_2 is formed in registers.  At the end the two halves of a row merge and the
// split's list goes to the workspace.
template <int KP>
__global__ __launch_bounds__(256) void knn_topk_kernel(KnnArgs p) {
  __shared__ __attribute__((aligned(16))) float sA[KNN_BQ * KNN_LDK];
  __shared__ __attribute__((aligned(16))) float sB[KNN_BN * KNN_LDK];
  __shared__ __attribute__((aligned(16))) float sc[KNN_BQ * KNN_LDS];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.x * KNN_BQ;
  const int ntiles = (p.N + KNN_BN - 1) / KNN_BN;
  const int t0 = blockIdx.y * p.tiles_per_split;
  const int t1 = min(t0 + p.tiles_per_split, ntiles);
  const int r = tid >> 1, h = tid & 1;

  float lv[4][KP];
  int li[4][KP];
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int j = 0; j < KP; ++j) { lv[v][j] = -INFINITY; li[v][j] = 0x7fffffff; }

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * KNN_BN;
    f32x4 sum[4][4];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      if (m >= p.M) break;
      f32x4 acc[4][4];
      knn_score_tile(p, p.q[m], p.x[m], q0, n0, sA, sB, acc);
      if (p.V > p.M) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) sum[i][j] = m == 0 ? acc[i][j] : sum[i][j] + acc[i][j];
      }
      knn_store_tile(sc, acc);
      for (int c = h; c < KNN_BN && n0 + c < p.N; c += 2) knn_offer<KP>(lv[m], li[m], sc[r * KNN_LDS + c], n0 + c);
    }
    if (p.V > p.M) {
      knn_store_tile(sc, sum);
      for (int c = h; c < KNN_BN && n0 + c < p.N; c += 2) knn_offer<KP>(lv[3], li[3], sc[r * KNN_LDS + c], n0 + c);
    }
  }

  // merge the two halves of every row, then write the split's list: ws[((split * V + v) * Nq + q) * k + j]
  __syncthreads();
  if (h == 1) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        sc[((r * 4 + v) * KP + j) * 2] = lv[v][j];
        sc[((r * 4 + v) * KP + j) * 2 + 1] = __int_as_float(li[v][j]);
      }
  }
  __syncthreads();
  const int q = q0 + r;
  if (h == 0 && q < p.Nq) {
    // slot s < M holds view s; slot 3 holds the sum view, view M
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (!(s < p.M || (s == 3 && p.V > p.M))) continue;
#pragma unroll
      for (int j = 0; j < KP; ++j)
        knn_offer<KP>(lv[s], li[s], sc[((r * 4 + s) * KP + j) * 2], __float_as_int(sc[((r * 4 + s) * KP + j) * 2 + 1]));
      KnnEntry* w = p.ws + (((long)blockIdx.y * p.V + (s < p.M ? s : p.M)) * p.Nq + q) * p.k;
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < p.k) w[j] = KnnEntry{lv[s][j], li[s][j]};
    }
  }
}

// one thread per (view, query): the splits' lists -> the final sorted top-k
__global__ __launch_bounds__(256) void knn_merge_kernel(const KnnEntry* __restrict__ ws, int S, int V, int Nq, int k,
                                                        float* __restrict__ top_val, int* __restrict__ top_idx) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)V * Nq) return;
  float val[8];
  int idx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { val[j] = -INFINITY; idx[j] = 0x7fffffff; }
  const long stride = (long)V * Nq * k;
  for (int s = 0; s < S; ++s) {
    const KnnEntry* e = ws + s * stride + t * k;
    for (int j = 0; j < k; ++j) {
      const KnnEntry c = e[j];
      knn_offer<8>(val, idx, c.v, c.i);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < k) { top_val[t * k + j] = val[j]; top_idx[t * k + j] = idx[j]; }
}

}  // namespace

extern "C" int dav_mean_l2n_f32(const float* x, int B, int L, int D, long ld_row, long ld_batch, float* out, hipStream_t stream) {
  if (B <= 0 || L <= 0 || D <= 0 || !x || !out || ld_row < D || ld_batch < 0) return DAV_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)out) & 3) return DAV_ERR_ALIGN;
  DAV_LAUNCH(mean_l2n_kernel, dim3(B), dim3(256), 0, stream, x, L, D, ld_row, ld_batch, out);
  return dav_launch_status();
}

extern "C" int dav_knn_topk_f32(const float* q0, const float* x0, const float* q1, const float* x1, const float* q2,
                                const float* x2, int M, int Nq, int N, int D, long ldq, long ldx, int sum_view, int k, int splits,
                                float* top_val, int* top_idx, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (M < 1 || M > 3 || Nq <= 0 || N <= 0 || D <= 0 || (sum_view != 0 && sum_view != 1) || splits < 1 || splits > 65535)
    return DAV_ERR_SHAPE;
  if (k < 1 || k > 8 || k > N) return DAV_ERR_SHAPE;
  if (D % 4 || ldq < D || ldx < D || !top_val || !top_idx) return DAV_ERR_SHAPE;
  const float* qs[3] = {q0, q1, q2};
  const float* xs[3] = {x0, x1, x2};
  for (int m = 0; m < M; ++m) {
    if (!qs[m] || !xs[m]) return DAV_ERR_SHAPE;
    if (((uintptr_t)qs[m] | (uintptr_t)xs[m]) & 15) return DAV_ERR_ALIGN;
  }
  if ((ldq | ldx) & 3 || ((uintptr_t)top_val | (uintptr_t)top_idx) & 3) return DAV_ERR_ALIGN;
  const int V = M + sum_view;
  if (!workspace || workspace_bytes < (size_t)splits * V * Nq * k * sizeof(KnnEntry)) return DAV_ERR_WORKSPACE;
  if ((uintptr_t)workspace & 7) return DAV_ERR_ALIGN;
  KnnArgs a;
  for (int m = 0; m < 3; ++m) { a.q[m] = m < M ? qs[m] : nullptr; a.x[m] = m < M ? xs[m] : nullptr; }
  a.ldq = ldq; a.ldx = ldx; a.M = M; a.Nq = Nq; a.N = N; a.D = D; a.V = V; a.k = k;
  const int ntiles = (N + KNN_BN - 1) / KNN_BN;
  a.tiles_per_split = (ntiles + splits - 1) / splits;
  a.ws = (KnnEntry*)workspace;
  const dim3 grid((Nq + KNN_BQ - 1) / KNN_BQ, splits);
  if (k == 1) DAV_LAUNCH(knn_topk_kernel<1>, grid, dim3(256), 0, stream, a);
  else if (k == 2) DAV_LAUNCH(knn_topk_kernel<2>, grid, dim3(256), 0, stream, a);
  else if (k <= 4) DAV_LAUNCH(knn_topk_kernel<4>, grid, dim3(256), 0, stream, a);
  else DAV_LAUNCH(knn_topk_kernel<8>, grid, dim3(256), 0, stream, a);
  const long nm = (long)V * Nq;
  DAV_LAUNCH(knn_merge_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, stream, (const KnnEntry*)workspace, splits, V, Nq,
             k, top_val, top_idx);
  return dav_launch_status();
}
