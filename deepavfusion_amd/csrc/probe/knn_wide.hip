// The weighted k-nearest-neighbour probe (Wu et al. 2018, DINO): top-k lists of up to 64 bank rows per query and view, and the
// vote over them.  This goes beyond the reference, whose probe reads the single nearest other clip (knn.hip).
//
// dav_knn_topk_wide_f32 scores with knn_tile.h, the tile code of dav_knn_topk_f32 — the same fp32 FMA chains in the same order — but
// its lists do not fit registers (4 views x 64 entries x 2 words), nor LDS (128 rows x 4 views x 64 x 8 B = 256 KB).  They live in
// the caller's workspace, one sorted list per (split, view, query), and a thread keeps only the admission threshold of its row in
// registers: the list's last entry.  A candidate costs one compare, as in the narrow kernel; the few that beat the threshold
// (about k ln(N / k) per row on unordered data) are inserted by the whole wave, lane j owning entry j: one coalesced load, one
// shuffle, one coalesced store.
//
// Like knn.hip this file is outside _lib.kernel_source_hash() (csrc/*.hip, csrc/*.h): nothing here runs in the pre-training step.
#include "common.h"
#include "dav_kernels.h"

#include "knn_tile.h"

#define KNN_WIDE_K 64      // longest list: one entry per lane of a wave

namespace {

// The wave inserts candidate (cv, ci) into the sorted list L[0 .. k) (k <= 64): lane j holds entry j, entries the candidate beats
// move down one place, the last falls off.  A candidate that beats nothing changes nothing.  -> the list's new last entry, which
// is the same value in every lane.
__device__ __forceinline__ KnnEntry knn_wave_insert(KnnEntry* L, int k, int lane, float cv, int ci) {
  KnnEntry e = lane < k ? L[lane] : KnnEntry{-INFINITY, 0x7fffffff};
  const bool b = knn_better(cv, ci, e.v, e.i);
  const float pv = __shfl_up(e.v, 1);
  const int pi = __shfl_up(e.i, 1);
  const int pb = __shfl_up((int)b, 1);
  if (b) {
    const bool shift = lane > 0 && pb;               // the entry above moves down too: take it; else the candidate lands here
    e = KnnEntry{shift ? pv : cv, shift ? pi : ci};
    if (lane < k) L[lane] = e;
  }
  return KnnEntry{__shfl(e.v, k - 1), __shfl(e.i, k - 1)};
}

// Thread (row r = tid / 2, half h = tid % 2) scans the columns h, h + 2, ... of its row of the score tile against the row's
// threshold (tv, ti).  Both halves of a row sit in one wave, which serialises its insertions, so the two share one list.  The
// trip count is the same for every lane (the ballot needs the whole wave); rows past Nq and columns past N never qualify.
__device__ __forceinline__ void knn_wide_scan(const float* sc, KnnEntry* lists, int k, int n0, int N, bool row_ok, float& tv,
                                              int& ti) {
  const int tid = threadIdx.x, lane = tid & 63, r = tid >> 1, h = tid & 1;
  for (int c = h; c < KNN_BN; c += 2) {
    const int n = n0 + c;
    const float v = sc[r * KNN_LDS + c];
    unsigned long long todo = __ballot(row_ok && n < N && knn_better(v, n, tv, ti));
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      // the partner half may have raised the row's threshold a moment ago: such a candidate then inserts nothing
      const KnnEntry last = knn_wave_insert(lists + (long)(src >> 1) * k, k, lane, __shfl(v, src), __shfl(n, src));
      if ((lane >> 1) == (src >> 1)) { tv = last.v; ti = last.i; }
    }
  }
}

// One workgroup: KNN_BQ queries x the bank tiles of its split, as knn_topk_kernel.  Wave w owns the query rows 32 w .. 32 w + 31 of
// the tile and their lists ws[((split * V + view) * Nq + q) * k + j], which it fills with (-inf, INT_MAX) before the first tile.
__global__ __launch_bounds__(256) void knn_topk_wide_kernel(KnnArgs p) {
  __shared__ __attribute__((aligned(16))) float sA[KNN_BQ * KNN_LDK];
  __shared__ __attribute__((aligned(16))) float sB[KNN_BN * KNN_LDK];
  __shared__ __attribute__((aligned(16))) float sc[KNN_BQ * KNN_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * KNN_BQ;
  const int ntiles = (p.N + KNN_BN - 1) / KNN_BN;
  const int t0 = blockIdx.y * p.tiles_per_split;
  const int t1 = min(t0 + p.tiles_per_split, ntiles);
  const int k = p.k;
  const int qw = q0 + 32 * wave;                         // first query row of this wave
  const bool row_ok = q0 + (tid >> 1) < p.Nq;
  const bool has_sum = p.V > p.M;

  KnnEntry* lists[4];                                    // slot s < M: view s; slot 3: the sum view, view M
#pragma unroll
  for (int s = 0; s < 4; ++s) lists[s] = p.ws + (((long)blockIdx.y * p.V + (s < 3 ? s : p.M)) * p.Nq + qw) * k;
  const int rows = min(32, p.Nq - qw);                   // <= 0 for a wave past the last query: it writes nothing
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!(s < p.M || (s == 3 && has_sum))) continue;
    for (int e = lane; e < rows * k; e += 64) lists[s][e] = KnnEntry{-INFINITY, 0x7fffffff};
  }
  float tv[4];
  int ti[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) { tv[s] = -INFINITY; ti[s] = 0x7fffffff; }

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * KNN_BN;
    f32x4 sum[4][4];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      if (m >= p.M) break;
      f32x4 acc[4][4];
      knn_score_tile(p, p.q[m], p.x[m], q0, n0, sA, sB, acc);
      if (has_sum) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) sum[i][j] = m == 0 ? acc[i][j] : sum[i][j] + acc[i][j];
      }
      knn_store_tile(sc, acc);
      knn_wide_scan(sc, lists[m], k, n0, p.N, row_ok, tv[m], ti[m]);
    }
    if (has_sum) {
      knn_store_tile(sc, sum);
      knn_wide_scan(sc, lists[3], k, n0, p.N, row_ok, tv[3], ti[3]);
    }
  }
}

// one wave per (view, query): the splits' sorted lists -> the final sorted top-k, the running list in registers (lane j: entry j)
__global__ __launch_bounds__(256) void knn_merge_wide_kernel(const KnnEntry* __restrict__ ws, int S, long VNq, int k,
                                                             float* __restrict__ top_val, int* __restrict__ top_idx) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= VNq) return;
  KnnEntry e = ws[t * k + min(lane, k - 1)];             // split 0 is sorted already
  if (lane >= k) e = KnnEntry{-INFINITY, 0x7fffffff};
  for (int s = 1; s < S; ++s) {
    const KnnEntry c = ws[(s * VNq + t) * k + min(lane, k - 1)];
    for (int j = 0; j < k; ++j) {
      const float cv = __shfl(c.v, j);
      const int ci = __shfl(c.i, j);
      if (!knn_better(cv, ci, __shfl(e.v, k - 1), __shfl(e.i, k - 1))) break;       // sorted: the rest of this list fails too
      const bool b = knn_better(cv, ci, e.v, e.i);
      const float pv = __shfl_up(e.v, 1);
      const int pi = __shfl_up(e.i, 1);
      const int pb = __shfl_up((int)b, 1);
      if (b) {
        const bool shift = lane > 0 && pb;
        e = KnnEntry{shift ? pv : cv, shift ? pi : ci};
      }
    }
  }
  if (lane < k) { top_val[t * k + lane] = e.v; top_idx[t * k + lane] = e.i; }
}

struct VoteArgs {
  const float* top_val;
  const int* top_idx;
  const int* labels;
  const uint8_t* multihot;
  float* scores;
  int* pred;
  float inv_t[4];
  int V, Nq, kk, k, N, C, self_offset;
};

// One wave per (view, query).  Lane j takes entry j of the row: the entries that are not the query's own row are numbered in
// order, the first k of them are the neighbours, and (w_j, class or bank row of j) go to LDS in that order.  Then lane c, c + 64, ... adds
// the neighbours' weights of class c one after the other — the same order for every class and every launch.
__global__ __launch_bounds__(256) void knn_vote_kernel(VoteArgs a) {
  __shared__ float sw[4][KNN_WIDE_K];
  __shared__ int sn[4][KNN_WIDE_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long t = (long)blockIdx.x * 4 + wave;            // (view, query)
  if (t >= (long)a.V * a.Nq) return;                     // whole waves leave; no barrier below
  const int v = (int)(t / a.Nq), q = (int)(t % a.Nq);
  const float inv_t = a.inv_t[v];
  const int self = a.self_offset < 0 ? -1 : q + a.self_offset;
  int used = 0;
  for (int j0 = 0; j0 < a.kk && used < a.k; j0 += 64) {
    const int j = j0 + lane;
    const int n = j < a.kk ? a.top_idx[t * a.kk + j] : -1;
    const bool keep = j < a.kk && n != self;
    const unsigned long long m = __ballot(keep);
    const int pos = used + __popcll(m & ((1ull << lane) - 1));
    if (keep && pos < a.k) {
      sw[wave][pos] = expf(a.top_val[t * a.kk + j] * inv_t);
      const bool in_bank = (unsigned)n < (unsigned)a.N;              // a row outside the bank votes for nothing
      sn[wave][pos] = !in_bank ? -1 : (a.labels ? a.labels[n] : n);  // class ids: the neighbour's class; multi-hot: its bank row
    }
    used += __popcll(m);
  }
  const int k = min(used, a.k);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float best = -INFINITY;
  int best_c = 0x7fffffff;
  float* out = a.scores + t * a.C;
  for (int c = lane; c < a.C; c += 64) {
    float s = 0.f;
    if (a.labels) {
      for (int j = 0; j < k; ++j) s += sn[wave][j] == c ? sw[wave][j] : 0.f;
    } else {
      for (int j = 0; j < k; ++j) {
        const int n = sn[wave][j];
        s += (n >= 0 && a.multihot[(long)n * a.C + c]) ? sw[wave][j] : 0.f;
      }
    }
    out[c] = s;
    if (s > best) { best = s; best_c = c; }              // classes ascend within a lane: the lower class keeps a tie
  }
  if (a.pred) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int oc = __shfl_xor(best_c, o);
      if (ov > best || (ov == best && oc < best_c)) { best = ov; best_c = oc; }
    }
    if (lane == 0) a.pred[t] = best_c;
  }
}

}  // namespace

extern "C" int dav_knn_topk_wide_f32(const float* q0, const float* x0, const float* q1, const float* x1, const float* q2,
                                     const float* x2, int M, int Nq, int N, int D, long ldq, long ldx, int sum_view, int k,
                                     int splits, float* top_val, int* top_idx, void* workspace, size_t workspace_bytes,
                                     hipStream_t stream) {
  if (M < 1 || M > 3 || Nq <= 0 || N <= 0 || D <= 0 || (sum_view != 0 && sum_view != 1) || splits < 1 || splits > 65535)
    return DAV_ERR_SHAPE;
  if (k < 1 || k > KNN_WIDE_K || k > N) return DAV_ERR_SHAPE;
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
  DAV_LAUNCH(knn_topk_wide_kernel, dim3((Nq + KNN_BQ - 1) / KNN_BQ, splits), dim3(256), 0, stream, a);
  const long nm = (long)V * Nq;
  DAV_LAUNCH(knn_merge_wide_kernel, dim3((unsigned)((nm + 3) / 4)), dim3(256), 0, stream, (const KnnEntry*)workspace, splits, nm, k,
             top_val, top_idx);
  return dav_launch_status();
}

extern "C" int dav_knn_vote_f32(const float* top_val, const int* top_idx, int V, int Nq, int kk, int k, const int* labels,
                                const uint8_t* multihot, int N, int C, const float* inv_t, int self_offset, float* scores, int* pred,
                                hipStream_t stream) {
  if (V < 1 || V > 4 || Nq <= 0 || kk <= 0 || N <= 0 || C <= 0 || k < 1 || k > KNN_WIDE_K || k > kk) return DAV_ERR_SHAPE;
  if (self_offset < -1 || (self_offset >= 0 && k > kk - 1)) return DAV_ERR_SHAPE;      // fewer than k entries may remain
  if (!top_val || !top_idx || !inv_t || !scores || (labels == nullptr) == (multihot == nullptr)) return DAV_ERR_SHAPE;
  if (labels && !pred) return DAV_ERR_SHAPE;
  if (((uintptr_t)top_val | (uintptr_t)top_idx | (uintptr_t)labels | (uintptr_t)scores | (uintptr_t)pred) & 3) return DAV_ERR_ALIGN;
  VoteArgs a;
  a.top_val = top_val; a.top_idx = top_idx; a.labels = labels; a.multihot = multihot; a.scores = scores;
  a.pred = labels ? pred : nullptr;
  for (int v = 0; v < 4; ++v) a.inv_t[v] = v < V ? inv_t[v] : 0.f;
  a.V = V; a.Nq = Nq; a.kk = kk; a.k = k; a.N = N; a.C = C; a.self_offset = self_offset;
  const long nm = (long)V * Nq;
  DAV_LAUNCH(knn_vote_kernel, dim3((unsigned)((nm + 3) / 4)), dim3(256), 0, stream, a);
  return dav_launch_status();
}
