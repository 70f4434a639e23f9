// Audio resampling of the input stage on the GPU: the reference's loader reads every track at its own rate and applies
//   Resample(areader.rate, rate)(waveform) -> Pad -> RandomVol                     (datasets.py:176-181, util/audio_transforms.py:8-27)
// in a CPU worker; here the three run as ONE kernel over a batch of waveforms, in front of the log-mel kernel (csrc/mel.hip).
//
// The filter is torchaudio's default windowed-sinc polyphase resampler: with o = orig / gcd, n = new / gcd, K = 2 width + o taps
// per phase, and the input zero-padded by `width` in front,
//   r[f n + p] = sum_k taps[p][k] xpad[f o + k]            f = frame, p = phase, r cut to R = ceil(n L / o) samples.
// Every r[i] is ONE k-ordered fmaf chain from 0 over all K taps (samples outside the waveform enter as exact zeros), whichever
// path or tile computes it: a fused call and a plain call give the same bits.
//
// Epilogue (Pad's "append the flipped signal until long enough, then cut" has period 2 R): out[j] = c(gain r[m(j)]),
// m(j) = j' < R ? j' : 2 R - 1 - j', j' = j mod 2 R.  A computed r[i] is stored to every j that maps to it.
//
// Two paths, picked by the geometry alone (resample_tile below; never by a switch):
//  * wide (n >= 64 and K <= 480): a workgroup owns 32 frames of one clip.  The 32 overlapping frame windows are staged in LDS
//    DE-OVERLAPPED as X[k][a] = xpad[(f0 + a) o + k] (K x 32 floats, 60 KB at K = 480), so that a thread — which owns one phase p
//    and the 32 frame accumulators — reads the 32 samples of tap k as eight aligned 16-byte broadcast reads with immediate
//    offsets, and the tap itself from the k-major table (lanes read consecutive p: coalesced).  One LDS read per four fmaf.
//  * narrow (everything else: n = 1 is a plain FIR, n = 2): a workgroup owns up to 256 frames, staged as one contiguous stretch
//    of (T - 1) o + K samples (dynamic LDS: 3 KB at 48 -> 16 kHz, so many workgroups share a CU); a thread owns one output
//    (frame, phase), phase fastest.
// Both are bound by load latency unless loads are batched (B = 64, 10 s, 44.1 -> 16 kHz: 0.58 ms with one load per branch and
// one tap per iteration, 0.29 ms now; profiles/resample_bench.json): the staging loops keep four to eight loads in flight, the wide
// path fetches its taps four at a time, one chunk ahead of their use.
#include "common.h"
#include "dav_kernels.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WIDE_FRAMES = 32;       // frames per workgroup = accumulators per thread of the wide path
constexpr int RS_WIDE_MIN_N = 64;        // fewer phases than a wave leave most lanes of the wide path idle
constexpr int RS_WIDE_MAX_TAPS = 480;    // 480 x 32 floats = 60 KB of LDS
constexpr int RS_NARROW_FRAMES = 256;
constexpr int RS_NARROW_FLOATS = 14336;  // 56 KB of LDS: (T - 1) o + K samples

// sample i of a row, 0 outside [0, L): the load itself is unconditional (from the index clamped into the row) and the zero a
// select, so that the loads of an unrolled staging loop are issued together instead of one per branch
template <bool I16>
__device__ __forceinline__ float load_sample(const void* wave, size_t row, long long i, int L) {
  const long long c = i < 0 ? 0 : (i >= L ? L - 1 : i);
  const float v = I16 ? (float)reinterpret_cast<const int16_t*>(wave)[row + c] * (1.0f / 32768.0f)      // exact: 2^-15
                      : reinterpret_cast<const float*>(wave)[row + c];
  return i == c ? v : 0.f;
}

// r[i] (i < need <= R) -> every j < out_len with m(j) = i
__device__ __forceinline__ void emit(float* __restrict__ orow, long long i, float v, float g, int clamp, long long R, int out_len) {
  v = g * v;
  if (clamp) v = fminf(fmaxf(v, -1.0f), 1.0f);
  for (long long j = i; j < out_len; j += 2 * R) orow[j] = v;
  for (long long j = 2 * R - 1 - i; j < out_len; j += 2 * R) orow[j] = v;
}

struct ResampleArgs {
  const void* wave;
  const float* taps_kn;   // [K][n]
  const float* gain;
  float* out;
  long in_rs, out_rs;
  long long R;
  int is_i16, L, o, n, width, K, T, need, clamp, out_len;
};

// tap k of one phase against the 32 staged samples of tap k: eight 16-byte broadcast reads, 32 fmaf
__device__ __forceinline__ void wide_tap(float (&acc)[RS_WIDE_FRAMES], const float* __restrict__ X, int k, float t) {
  const f32x4* xr = reinterpret_cast<const f32x4*>(X + k * RS_WIDE_FRAMES);
#pragma unroll
  for (int a4 = 0; a4 < RS_WIDE_FRAMES / 4; ++a4) {
    const f32x4 x = xr[a4];
    acc[4 * a4 + 0] = fmaf(t, x.x, acc[4 * a4 + 0]);
    acc[4 * a4 + 1] = fmaf(t, x.y, acc[4 * a4 + 1]);
    acc[4 * a4 + 2] = fmaf(t, x.z, acc[4 * a4 + 2]);
    acc[4 * a4 + 3] = fmaf(t, x.w, acc[4 * a4 + 3]);
  }
}

template <bool I16>
__global__ __launch_bounds__(RS_THREADS) void resample_wide_kernel(ResampleArgs q) {
  __shared__ __attribute__((aligned(16))) float X[RS_WIDE_MAX_TAPS * RS_WIDE_FRAMES];
  const int b = blockIdx.y, f0 = blockIdx.x * RS_WIDE_FRAMES;
  const size_t row = (size_t)b * q.in_rs;
  // staging: a wave covers 8 taps x 32 frames per trip as four loads of 8 frames x 8 taps — runs of 8 consecutive samples from
  // global memory, 4 lanes per LDS bank on the way in; the four loads (eight with the unrolled trip) are in flight together
  const int lane = threadIdx.x & 63, kblocks = (q.K + 7) >> 3;
#pragma unroll 2
  for (int kb = threadIdx.x >> 6; kb < kblocks; kb += blockDim.x >> 6) {
    const int k = kb * 8 + (lane >> 3);
    float v[4];
#pragma unroll
    for (int ab = 0; ab < 4; ++ab)
      v[ab] = k < q.K ? load_sample<I16>(q.wave, row, (long long)(f0 + ab * 8 + (lane & 7)) * q.o + k - q.width, q.L) : 0.f;
    if (k < q.K) {
#pragma unroll
      for (int ab = 0; ab < 4; ++ab) X[k * RS_WIDE_FRAMES + ab * 8 + (lane & 7)] = v[ab];
    }
  }
  __syncthreads();
  const float g = q.gain ? q.gain[b] : 1.0f;
  float* orow = q.out + (size_t)b * q.out_rs;
  constexpr int KU = 4;       // taps fetched together, one chunk ahead of their use (8: every LDS read hoisted, 290 registers)
  for (int p = threadIdx.x; p < q.n; p += blockDim.x) {
    float acc[RS_WIDE_FRAMES];
#pragma unroll
    for (int a = 0; a < RS_WIDE_FRAMES; ++a) acc[a] = 0.f;
    const float* tp = q.taps_kn + p;
    float tn[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) tn[u] = u < q.K ? tp[(size_t)u * q.n] : 0.f;
    int k = 0;
    for (; k + KU <= q.K; k += KU) {
      float t[KU];
#pragma unroll
      for (int u = 0; u < KU; ++u) t[u] = tn[u];
      if (k + 2 * KU <= q.K) {
#pragma unroll
        for (int u = 0; u < KU; ++u) tn[u] = tp[(size_t)(k + KU + u) * q.n];
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) wide_tap(acc, X, k + u, t[u]);
    }
    for (; k < q.K; ++k) wide_tap(acc, X, k, tp[(size_t)k * q.n]);
#pragma unroll
    for (int a = 0; a < RS_WIDE_FRAMES; ++a) {
      const long long i = (long long)(f0 + a) * q.n + p;
      if (i < q.need) emit(orow, i, acc[a], g, q.clamp, q.R, q.out_len);
    }
  }
}

template <bool I16>
__global__ __launch_bounds__(RS_THREADS) void resample_narrow_kernel(ResampleArgs q) {
  extern __shared__ __attribute__((aligned(16))) float xs[];    // (T - 1) o + K samples: sized by the launch, <= RS_NARROW_FLOATS
  const int b = blockIdx.y, f0 = blockIdx.x * q.T;
  const size_t row = (size_t)b * q.in_rs;
  const int span = (q.T - 1) * q.o + q.K;
  const long long base = (long long)f0 * q.o - q.width;
#pragma unroll 4
  for (int i = threadIdx.x; i < span; i += RS_THREADS) xs[i] = load_sample<I16>(q.wave, row, base + i, q.L);
  __syncthreads();
  const float g = q.gain ? q.gain[b] : 1.0f;
  float* orow = q.out + (size_t)b * q.out_rs;
  for (int w = threadIdx.x; w < q.T * q.n; w += RS_THREADS) {
    const int f = w / q.n, p = w - f * q.n;
    const long long i = (long long)(f0 + f) * q.n + p;
    if (i >= q.need) continue;
    const float* tp = q.taps_kn + p;
    const float* xp = xs + f * q.o;                             // f o + k <= (T - 1) o + K - 1 < span
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < q.K; ++k) acc = fmaf(tp[(size_t)k * q.n], xp[k], acc);
    emit(orow, i, acc, g, q.clamp, q.R, q.out_len);
  }
}

// frames per workgroup for a geometry, 0 when it is refused; wide reports whether the wide path serves it
int resample_tile(int o, int n, int width, bool& wide) {
  wide = false;
  if (o < 1 || n < 1 || width < 1 || o > dav_resample_max_ratio || n > dav_resample_max_ratio) return 0;
  if (width > RS_NARROW_FLOATS) return 0;
  const int K = 2 * width + o;
  if (K > RS_NARROW_FLOATS) return 0;
  if (n >= RS_WIDE_MIN_N && K <= RS_WIDE_MAX_TAPS) {
    wide = true;
    return RS_WIDE_FRAMES;
  }
  const int fit = (RS_NARROW_FLOATS - K) / o + 1;
  return fit < RS_NARROW_FRAMES ? fit : RS_NARROW_FRAMES;
}

}  // namespace

extern "C" int dav_wave_resample_tile(int o, int n, int width) {
  bool wide;
  const int T = resample_tile(o, n, width, wide);
  return T > 0 ? T : DAV_ERR_SHAPE;
}

extern "C" int dav_wave_resample(const void* wave, int wave_is_i16, int B, int L, long in_rs, const float* taps_kn, int o, int n,
                                 int width, const float* gain, int clamp, float* out, int out_len, long out_rs,
                                 hipStream_t stream) {
  if (B <= 0 || L <= 0 || out_len <= 0 || B > 65535 || L > (1 << 30) || out_len > (1 << 30)) return DAV_ERR_SHAPE;
  bool wide;
  const int T = resample_tile(o, n, width, wide);
  if (T <= 0) return DAV_ERR_SHAPE;
  if (!wave || !taps_kn || !out || in_rs < L || out_rs < out_len) return DAV_ERR_SHAPE;
  if (((uintptr_t)wave & (wave_is_i16 ? 1 : 3)) || ((uintptr_t)taps_kn & 3) || ((uintptr_t)out & 3) || ((uintptr_t)gain & 3))
    return DAV_ERR_ALIGN;
  ResampleArgs q;
  q.wave = wave, q.taps_kn = taps_kn, q.gain = gain, q.out = out;
  q.in_rs = in_rs, q.out_rs = out_rs;
  q.R = ((long long)n * L + o - 1) / o;
  q.is_i16 = wave_is_i16 != 0, q.L = L, q.o = o, q.n = n, q.width = width, q.K = 2 * width + o, q.T = T;
  q.need = (int)(q.R < out_len ? q.R : out_len);
  q.clamp = clamp != 0, q.out_len = out_len;
  const long long frames = ((long long)q.need + n - 1) / n;
  const long long tiles = (frames + T - 1) / T;
  if (tiles > 0x7fffffffLL) return DAV_ERR_SHAPE;
  if (wide) {
    const int threads = n >= RS_THREADS ? RS_THREADS : (n + 63) / 64 * 64;
    if (q.is_i16) DAV_LAUNCH(resample_wide_kernel<true>, dim3((unsigned)tiles, B), dim3(threads), 0, stream, q);
    else DAV_LAUNCH(resample_wide_kernel<false>, dim3((unsigned)tiles, B), dim3(threads), 0, stream, q);
  } else {
    const size_t lds = ((size_t)(T - 1) * o + q.K) * sizeof(float);
    if (q.is_i16) DAV_LAUNCH(resample_narrow_kernel<true>, dim3((unsigned)tiles, B), dim3(RS_THREADS), lds, stream, q);
    else DAV_LAUNCH(resample_narrow_kernel<false>, dim3((unsigned)tiles, B), dim3(RS_THREADS), lds, stream, q);
  }
  return dav_launch_status();
}
