// Multi-label probe metrics on the device: per-class average precision and ROC AUC of V score views against multi-hot truth, as
// util/knn_probe.py states sklearn's average_precision_score / roc_auc_score (average=None): scores descending, ties grouped into
// one threshold.
//
// One workgroup owns one (view, class) column and keeps it resident in LDS as 32-bit keys: a monotone integer image of the fp32
// score (ascending key = descending score, -0.0 and +0.0 one key, subnormals as they are — nothing is ever compared or
// multiplied as a float).  The keys of the positives are packed from the front of the column, those of the negatives from its
// back, and both runs are sorted in place by one bitonic network.  The truth bit needs no room beside the key that way, and the
// curve needs no merge: for the LAST positive i of every tie group
//     tp = i + 1,  dtp = tp - (first positive of the group),  ge / gt = negatives with score >= / > this one (binary searches)
//     AP  = 1/P sum dtp * tp / (tp + ge)                      (the thresholds without a positive add nothing)
//     AUC = sum dtp * (2 (Nneg - ge) + (ge - gt)) / (2 P Nneg)
// The second line is the trapezoid area under the distinct-threshold ROC written as the count of (positive, negative) pairs the
// score orders correctly, ties counting half: an exact integer, so the AUC carries ONE rounding.  The fp64 terms of the AP are added
// per thread in index order, then by a fixed butterfly, then over the waves in order: the same bits at every launch.
//
// The truth arrives as uint8 [n, C]; a first launch packs it into one bit mask per class in the workspace (read across the classes,
// so coalesced), which the V workgroups of a class then read as n / 32 consecutive words instead of n strided bytes.
//
// Like knn.hip this file is outside _lib.kernel_source_hash() (csrc/*.hip, csrc/*.h): nothing here runs in the pre-training step.
#include "common.h"
#include "dav_kernels.h"

#define APAUC_THREADS 1024
#define APAUC_HEAD 512      // bytes in front of the keys: 16 fp64 + 16 int64 wave partials, the two run counters

namespace {

struct ApAucArgs {
  const uint32_t* truth_bits;   // [C][W], W = ceil(n / 32): bit (i % 32) of word i / 32 is row i
  const uint32_t* scores;       // dense form: the fp32 scores as their bits, [V][n][C] with strides (vs, rs); else null
  const int* nbr;               // neighbour form: [V][n]
  const uint32_t* nbr_val;      // [V][n], fp32 bits
  const uint8_t* nbr_labels;    // [N][C]
  double* ap;
  double* auc;
  int* pos;
  long rs, vs;
  int n, C, N, W;
};

__global__ __launch_bounds__(256) void ap_auc_pack_truth_kernel(const uint8_t* __restrict__ y, long ldy, int n, int C, int W,
                                                                uint32_t* __restrict__ bits) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)W * C) return;
  const int w = (int)(t / C), c = (int)(t % C);          // adjacent lanes: adjacent classes of the same 32 rows
  uint32_t m = 0;
  for (int b = 0; b < 32; ++b) {
    const int row = 32 * w + b;
    if (row < n && y[row * ldy + c]) m |= 1u << b;
  }
  bits[(long)c * W + w] = m;
}

// fp32 bits -> key: ascending key = descending score; both zeros -> the key of +0.0
__device__ __forceinline__ uint32_t ap_auc_key(uint32_t u) {
  if ((u << 1) == 0) u = 0;
  return (u & 0x80000000u) ? u : (~u & 0x7fffffffu);
}

__device__ __forceinline__ void ap_auc_cswap(uint32_t* a, int i, int j) {
  const uint32_t x = a[i], y = a[j];
  if (x > y) { a[i] = y; a[j] = x; }
}

// first index of the ascending run a[0 .. len) whose key is >= d (strict = false) or > d (strict = true)
__device__ __forceinline__ int ap_auc_bound(const uint32_t* a, int len, uint32_t d, bool strict) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t x = a[mid];
    if (strict ? x <= d : x < d) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int ap_auc_log2_ceil(int len) { return len <= 1 ? 0 : 32 - __clz(len - 1); }

// One comparator of the stage (merge size 2^lk, step s; s < 0: the flip step that opens the merge) of the run a[0 .. len), for pair
// number t < 2^(lp - 1), lp = log2_ceil(len).  Every comparator puts the smaller key at the lower index, so the run behaves as if
// padded to 2^lp with keys above all others, which never move: a comparator that reaches past len is skipped.
__device__ __forceinline__ void ap_auc_comparator(uint32_t* a, int len, int lk, int s, int t) {
  int i, j;
  if (s < 0) {
    const int h = 1 << (lk - 1), o = t & (h - 1);
    i = ((t >> (lk - 1)) << lk) + o;
    j = i + ((h - o) << 1) - 1;                          // the mirror of i in its 2^lk block
  } else {
    i = ((t >> s) << (s + 1)) + (t & ((1 << s) - 1));
    j = i + (1 << s);
  }
  if (j < len) ap_auc_cswap(a, i, j);
}

__global__ __launch_bounds__(APAUC_THREADS) void ap_auc_kernel(ApAucArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red_ap = (double*)smem;                        // [16]
  long long* red_u = (long long*)(smem + 128);           // [16]
  int* count = (int*)(smem + 256);                       // [0]: positives placed, [1]: negatives placed
  uint32_t* keys = (uint32_t*)(smem + APAUC_HEAD);       // [n]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x, v = blockIdx.y, n = p.n;

  if (tid < 2) count[tid] = 0;
  __syncthreads();

  // ---- the column -> keys, positives from the front, negatives from the back (any order inside a run: it is sorted next) ----
  const uint32_t* tb = p.truth_bits + (long)c * p.W;
  const unsigned long long below = (1ull << lane) - 1;
  for (int i0 = wave * 64; i0 < n; i0 += APAUC_THREADS) {            // i0 is the same in every lane: the ballots see whole waves
    const int i = i0 + lane;
    const bool ok = i < n;
    uint32_t u = 0;
    bool yb = false;
    if (ok) {
      yb = (tb[i >> 5] >> (i & 31)) & 1u;
      if (p.scores) {
        u = p.scores[v * p.vs + i * p.rs + c];
      } else {
        const int r = p.nbr[(long)v * n + i];
        const bool lab = (unsigned)r < (unsigned)p.N && p.nbr_labels[(long)r * p.C + c];   // a row outside the bank has no label
        u = lab ? p.nbr_val[(long)v * n + i] : 0u;
      }
    }
    const unsigned long long mp = __ballot(ok && yb), mn = __ballot(ok && !yb);
    int bp = 0, bn = 0;
    if (lane == 0) {
      bp = atomicAdd(&count[0], __popcll(mp));
      bn = atomicAdd(&count[1], __popcll(mn));
    }
    bp = __shfl(bp, 0);
    bn = __shfl(bn, 0);
    if (ok) {
      const int at = yb ? bp + __popcll(mp & below) : n - 1 - (bn + __popcll(mn & below));
      keys[at] = ap_auc_key(u);
    }
  }
  __syncthreads();
  const int P = count[0], Nn = n - P;
  uint32_t* kp = keys;                                   // positives [0, P)
  uint32_t* kn = keys + P;                               // negatives [P, n)

  // ---- both runs through one bitonic network: the pairs of the positives first, then those of the negatives ----
  const int lpp = ap_auc_log2_ceil(P), lpn = ap_auc_log2_ceil(Nn);
  const int hp = lpp ? 1 << (lpp - 1) : 0, hn = lpn ? 1 << (lpn - 1) : 0;
  const int lmax = lpp > lpn ? lpp : lpn;
  for (int lk = 1; lk <= lmax; ++lk) {
    for (int s = -1, nxt = lk - 2; ; s = nxt, --nxt) {
      for (int t = tid; t < hp + hn; t += APAUC_THREADS) {
        if (t < hp) { if (lk <= lpp) ap_auc_comparator(kp, P, lk, s, t); }
        else if (lk <= lpn) ap_auc_comparator(kn, Nn, lk, s, t - hp);
      }
      __syncthreads();
      if (nxt < 0) break;
    }
  }

  // ---- the curve: one term per tie group of the positives ----
  double s_ap = 0.0;
  long long s_u = 0;
  for (int i = tid; i < P; i += APAUC_THREADS) {
    const uint32_t d = kp[i];
    if (i + 1 < P && kp[i + 1] == d) continue;           // not the last of its group
    const int tp = i + 1, dtp = tp - ap_auc_bound(kp, P, d, false);
    const int ge = ap_auc_bound(kn, Nn, d, true), gt = ap_auc_bound(kn, Nn, d, false);
    s_ap += (double)dtp * ((double)tp / (double)(tp + ge));
    s_u += (long long)dtp * (2ll * (Nn - ge) + (ge - gt));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s_ap += __shfl_xor(s_ap, o);
    s_u += __shfl_xor(s_u, o);
  }
  if (lane == 0) { red_ap[wave] = s_ap; red_u[wave] = s_u; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0;
    long long u2 = 0;
    for (int w = 0; w < APAUC_THREADS / 64; ++w) { a += red_ap[w]; u2 += red_u[w]; }
    const long o = (long)v * p.C + c;
    p.ap[o] = P > 0 ? a / (double)P : 0.0;
    p.auc[o] = (P > 0 && Nn > 0) ? (double)u2 / (2.0 * (double)P * (double)Nn) : __longlong_as_double(0x7ff8000000000000ll);
    if (v == 0) p.pos[c] = P;
  }
}

}  // namespace

static_assert(APAUC_HEAD + 4 * (size_t)dav_ap_auc_max_rows <= 160 * 1024, "a column of dav_ap_auc_max_rows keys fits the LDS of a CU");
static_assert(APAUC_HEAD % 16 == 0, "the keys start 16-byte aligned");

extern "C" int dav_ap_auc_f64(const uint8_t* y, long ldy, int n, int C, int V, const float* scores, long score_rs, long score_vs,
                              const int* nbr, const float* nbr_val, const uint8_t* nbr_labels, int N, double* ap, double* auc,
                              int* pos, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (n < 1 || C < 1 || V < 1 || V > 4 || n > dav_ap_auc_max_rows) return DAV_ERR_SHAPE;
  if (!y || ldy < C || !ap || !auc || !pos) return DAV_ERR_SHAPE;
  const bool dense = scores != nullptr, neigh = nbr != nullptr || nbr_val != nullptr || nbr_labels != nullptr;
  if (dense == neigh) return DAV_ERR_SHAPE;
  if (dense && (score_rs < C || score_vs < 0)) return DAV_ERR_SHAPE;
  if (neigh && (!nbr || !nbr_val || !nbr_labels || N < 1)) return DAV_ERR_SHAPE;
  if (((uintptr_t)scores | (uintptr_t)nbr | (uintptr_t)nbr_val | (uintptr_t)pos) & 3) return DAV_ERR_ALIGN;
  if (((uintptr_t)ap | (uintptr_t)auc) & 7) return DAV_ERR_ALIGN;
  const int W = (n + 31) / 32;
  if (!workspace || workspace_bytes < (size_t)C * W * 4) return DAV_ERR_WORKSPACE;
  if ((uintptr_t)workspace & 3) return DAV_ERR_ALIGN;
  const size_t lds = APAUC_HEAD + 4 * (size_t)n;
  static bool raised = false;                            // once: a workgroup may take the whole 160 KiB of its CU
  if (lds > 64 * 1024 && !raised) {
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)ap_auc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    raised = true;
  }
  ApAucArgs a;
  a.truth_bits = (const uint32_t*)workspace;
  a.scores = (const uint32_t*)scores; a.nbr = nbr; a.nbr_val = (const uint32_t*)nbr_val; a.nbr_labels = nbr_labels;
  a.ap = ap; a.auc = auc; a.pos = pos;
  a.rs = score_rs; a.vs = score_vs; a.n = n; a.C = C; a.N = N; a.W = W;
  DAV_LAUNCH(ap_auc_pack_truth_kernel, dim3((unsigned)(((long)W * C + 255) / 256)), dim3(256), 0, stream, y, ldy, n, C, W,
             (uint32_t*)workspace);
  DAV_LAUNCH(ap_auc_kernel, dim3(C, V), dim3(APAUC_THREADS), lds, stream, a);
  return dav_launch_status();
}
