// Gated forms of the two grouped weight-gradient launches (dav_gemm_tn_gang_bf16_gated, dav_gemm_tn_grouped_bf16_gated): "is this
// problem's C written or accumulated" is read from device memory WHEN THE LAUNCH RUNS, so that ONE captured launch serves every
// micro-step of a gradient-accumulation window (util.misc.GraphedStep with accum_iter > 1: the gate is open on the window's first
// micro-step only).
//
// This file IS the gemm translation unit of the library: it includes ../gemm.hip unchanged and adds the gated kernels behind it,
// because they are built from gemm.hip's internal pieces (tn2_body, TNGroup, the gang plan, the table writer's layout, the persistent
// tile kernel).  The Makefile compiles this file instead of gemm.hip.  Everything the step with accum_iter == 1 launches is compiled
// from gemm.hip as it stands (same text, same translation unit contents in front of it), and csrc/*.hip, csrc/*.h — what
// _lib.kernel_source_hash() and the PMC records under profiles/ cover — do not change when only the accumulation path does.
#include "../gemm.hip"

namespace {

// ---- gang launch: a table writer that applies the gate ------------------------------------------------------------------------
// gemm_tn_gang_write_kernel with one more argument.  The writer rebuilds the problem table in the workspace on every replay, so this
// is where a closed gate turns "written" (beta == 0) into "accumulated" (beta == 1); gemm_tn_gang_kernel reads beta from the table
// as before and is launched unchanged.
static_assert(sizeof(TGWrite) + sizeof(const int*) <= 4096, "kernel argument block");
constexpr int TG_BETA_WORD = (int)(offsetof(TNParams, beta) / 4), TG_PROB_WORDS = (int)(sizeof(TNParams) / 4);

__global__ __launch_bounds__(64) void gemm_tn_gang_write_gated_kernel(const TGWrite w, const int* __restrict__ write_gate) {
  TGHeader* hd = reinterpret_cast<TGHeader*>(w.ws);
  TNParams* probs = reinterpret_cast<TNParams*>(w.ws + sizeof(TGHeader));
  TGDesc* desc = reinterpret_cast<TGDesc*>(w.ws + sizeof(TGHeader) + (size_t)w.count_total * sizeof(TNParams));
  const int b = blockIdx.x, t = threadIdx.x;
  if (b < w.item_count) {
    const TGItem it = w.item[b];
    const int nr = it.nrnc >> 16, nc = it.nrnc & 0xffff, r0 = it.r0c0 >> 16, c0 = it.r0c0 & 0xffff;
    for (int i = t; i < nr * nc; i += 64) desc[it.desc_first + i] = TGDesc{it.prob, ((r0 + i / nc) << 16) | (c0 + i % nc)};
    return;
  }
  const bool closed = write_gate[0] == 0;
  const int* src = reinterpret_cast<const int*>(w.prob);
  int* dst = reinterpret_cast<int*>(probs + w.prob_first);
  for (int i = t; i < w.prob_count * TG_PROB_WORDS; i += 64) dst[i] = (closed && i % TG_PROB_WORDS == TG_BETA_WORD) ? 1 : src[i];
  if (w.write_header) {
    if (t < 8) hd->head[t] = 0;
    if (t < 9) hd->q_start[t] = w.q_start[t];
  }
}

// ---- grouped 128 x 128 launch: the effective beta from the gate -----------------------------------------------------------------
// gemm_tn_grouped_kernel with the problem copied out of the argument table (96 uniform bytes) and its beta replaced: a problem the
// host flagged as written keeps splits == 1, so the accumulate is a plain read-modify-write by the tile's one owner — correct, it
// just reads the old tile.
static_assert(sizeof(TNGroup) + sizeof(const int*) <= 4096, "kernel argument block");

template <int T, int WM_, int WN_, int RS = 64, int NST = 2, int MINW = 1, int TK = T>
__global__ __launch_bounds__(WM_* WN_ * 64, MINW) void gemm_tn_grouped_gated_kernel(const TNGroup g, const int* __restrict__ write_gate) {
  int pi = 0;
  const int count = g.count & 0xffff;
  while (pi + 1 < count && (int)blockIdx.x >= g.first_block[pi + 1]) ++pi;
  TNParams p = g.prob[pi];
  if (write_gate[0] == 0) p.beta = 1;
  const int local = blockIdx.x - g.first_block[pi];
  const int tiles = ((p.N + T - 1) / T) * ((p.K + TK - 1) / TK);
  int unit = local;
  if (g.count & TN_XCD_RUNS) {                       // one contiguous run of units per XCD, as in gemm_tn_grouped_kernel
    const int total = g.first_block[pi + 1] - g.first_block[pi];
    const int r = local & 7, j = local >> 3, q = total >> 3, rem = total & 7;
    unit = r * q + (r < rem ? r : rem) + j;
  }
  tn2_body<T, WM_, WN_, RS, NST, TK>(p, unit % tiles, unit / tiles);
}

}  // namespace

// Host side: the checks, split rule, unit order and launch geometry of tn_grouped_impl (gemm.hip).
extern "C" int dav_gemm_tn_grouped_bf16_gated(const DavTnProblem* probs, int count, const int* write_gate, hipStream_t stream) {
  if (!probs || !write_gate) return DAV_ERR_SHAPE;
  if (count <= 0 || count > TN_GROUP_MAX) return DAV_ERR_SHAPE;
  static thread_local TNGroup g;
  long total_tiles = 0;
  for (int i = 0; i < count; ++i) {
    const DavTnProblem& q = probs[i];
    if (q.Mc <= 0 || (q.Mc & 63) || q.N <= 0 || q.K <= 0 || (q.N & 7) || (q.K & 7) || (q.lda & 7) || (q.ldb & 7) || (q.flags & ~1)) return DAV_ERR_SHAPE;
    if (((uintptr_t)q.A | (uintptr_t)q.B | (uintptr_t)q.C) & 15 || (q.ldc & 3)) return DAV_ERR_ALIGN;
    total_tiles += (long)((q.N + 127) / 128) * ((q.K + 127) / 128);
  }
  int first = 0;
  for (int i = 0; i < count; ++i) {
    const DavTnProblem& q = probs[i];
    TNParams& p = g.prob[i];
    p.A = (const bf16_t*)q.A; p.B = (const bf16_t*)q.B; p.Mc = q.Mc; p.N = q.N; p.K = q.K; p.lda = q.lda; p.ldb = q.ldb;
    p.amap = RowMap{q.a_rowmap[0], q.a_rowmap[1], q.a_rowmap[2]};
    p.bmap = RowMap{q.b_rowmap[0], q.b_rowmap[1], q.b_rowmap[2]};
    p.C = q.C; p.ldc = q.ldc; p.beta = (q.flags & 1) ? 0 : 1; p.bias_grad = q.bias_grad; p.debug_plain_store = 0;
    const int tiles = ((q.N + 127) / 128) * ((q.K + 127) / 128), steps = q.Mc >> 6;
    int splits = (int)((1024 + total_tiles - 1) / total_tiles);
    const int max_splits = steps / 8 > 0 ? steps / 8 : 1;
    if (splits > max_splits) splits = max_splits;
    if (q.flags & 1) splits = 1;                         // written or accumulated, a flagged tile has one owner
    p.splits = splits;
    g.first_block[i] = first;
    first += tiles * splits;
  }
  g.first_block[count] = first;
  g.count = count | TN_XCD_RUNS;
  const TNGroup gl = g;                                  // (an automatic: a launch recorded by the batcher captures its arguments by value)
  DAV_LAUNCH((gemm_tn_grouped_gated_kernel<128, 4, 2>), dim3(first), dim3(512), (size_t)2 * 2 * 64 * 128 * 2, stream, gl, write_gate);
  return dav_launch_status();
}

// Host side: the checks, plan, writer chunking and persistent launch of dav_gemm_tn_gang_bf16 (gemm.hip) with the gated writer.
extern "C" int dav_gemm_tn_gang_bf16_gated(const DavTnProblem* probs, int count, void* workspace, size_t workspace_bytes, const int* write_gate,
                                           hipStream_t stream) {
  if (!probs || !workspace || !write_gate) return DAV_ERR_SHAPE;
  const int chk = tn_gang_check(probs, count);
  if (chk != DAV_OK) return chk;
  if ((uintptr_t)workspace & 15) return DAV_ERR_ALIGN;
  if (workspace_bytes < dav_gemm_tn_gang_workspace_bytes(probs, count)) return DAV_ERR_WORKSPACE;
  std::vector<TGPlanItem> items;
  int q_start[9];
  tn_gang_plan(probs, count, items, q_start);
  static const int dbg = getenv("DAV_TN_GANG_DEBUG") ? atoi(getenv("DAV_TN_GANG_DEBUG")) & 24 : 0;      // (placement bits only, as in product builds of the ungated launch)
  bool header = true;
  std::vector<std::vector<const TGPlanItem*>> by_prob(count);
  for (const TGPlanItem& it : items) by_prob[it.prob].push_back(&it);
  TGWrite w;
  auto reset = [&](int first) {
    w.ws = (char*)workspace; w.prob_first = first; w.prob_count = 0; w.item_count = 0; w.count_total = count; w.write_header = 0;
    for (int q = 0; q < 9; ++q) w.q_start[q] = q_start[q];
  };
  auto flush = [&]() {
    if (!w.prob_count && !w.item_count && !header) return;
    w.write_header = header ? 1 : 0; header = false;
    const TGWrite wl = w;
    DAV_LAUNCH(gemm_tn_gang_write_gated_kernel, dim3(wl.item_count + 1), dim3(64), 0, stream, wl, write_gate);
  };
  reset(0);
  for (int i = 0; i < count; ++i) {
    if (w.prob_count == TG_WCH) { flush(); reset(i); }
    const DavTnProblem& q = probs[i];
    TNParams& p = w.prob[w.prob_count++];
    p.A = (const bf16_t*)q.A; p.B = (const bf16_t*)q.B; p.Mc = q.Mc; p.N = q.N; p.K = q.K; p.lda = q.lda; p.ldb = q.ldb;
    p.amap = RowMap{q.a_rowmap[0], q.a_rowmap[1], q.a_rowmap[2]};
    p.bmap = RowMap{q.b_rowmap[0], q.b_rowmap[1], q.b_rowmap[2]};
    p.C = q.C; p.ldc = q.ldc; p.beta = (q.flags & 1) ? 0 : 1; p.bias_grad = q.bias_grad; p.debug_plain_store = 0; p.splits = 1;
    for (const TGPlanItem* it : by_prob[i]) {
      if (w.item_count == TG_WIT) { flush(); reset(i + 1); }
      w.item[w.item_count++] = TGItem{i, q_start[it->queue] + it->first, (it->r0 << 16) | it->c0, (it->nr << 16) | it->nc};
    }
  }
  flush();
  static std::mutex dev_mu;
  static int dev_cus[64] = {0};
  int n_wg = 256;
  {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return DAV_ERR_HIP;
    std::lock_guard<std::mutex> lk(dev_mu);
    if (!dev_cus[dev]) {
      if (hipFuncSetAttribute((const void*)gemm_tn_gang_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return DAV_ERR_HIP;
      int cus = 256;
      (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
      dev_cus[dev] = cus > 0 ? cus : 256;
    }
    n_wg = dev_cus[dev];
  }
  const int grid = (int)std::min<long>(n_wg, (long)q_start[8]);
  DAV_LAUNCH(gemm_tn_gang_kernel, dim3(grid), dim3(512), TNG_LDS, stream, (char*)workspace, count, dbg);
  return dav_launch_status();
}
