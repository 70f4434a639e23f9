// Source-separation audio on the GPU: the reference's SpectrogramMasking (eval_avsrcsep.py:264-277) turns a predicted mel-domain
// mask back into a waveform on the host, per sample and per source:
//   aT.Spectrogram(power=None)  ->  sigmoid(mask), one zero frame appended  ->  einsum('bmt,fm->bft', mask, mel_scale.fb)
//   ->  mask * stft  ->  aT.InverseSpectrogram (torch.istft)
// Here: dav_stft_c32 (the complex STFT), dav_istft_c32 (torch.istft, centre / one-sided / not normalised / length=None) and
// dav_sep_mask_istft, the whole chain in one launch in which neither the spectrum, nor the linear-frequency mask, nor the masked
// spectrum leaves the chip.  Everything is fp32; n_fft = 800 = 2^5 * 5^2 is no power of two, so both transforms are direct DFTs
// with cos / sin looked up at (k * n) mod n_fft in the exact tables MelSpectrogram builds, as csrc/mel.hip does.
//
// Forward (logmel_kernel's bin-pair trick): a thread owns the bins k and N/2 - k, whose twiddles agree up to (-1)^n, and keeps
// separate even-n / odd-n sums for each of its frames: one twiddle read feeds 2 bins x NF frames.
// Inverse (the same trick run backwards): a thread owns the samples n, N - n, N/2 + n and N/2 - n of each of its frames.  With the
// DC and Nyquist bins halved (exact) and their imaginary parts dropped (as irfft drops them),
//   x[n] N / 2 = sum_{k = 0 .. N/2} Re Y_k cos(2 pi k n / N) - Im Y_k sin(2 pi k n / N) = C - D;    x[N - n] N / 2 = C + D,
// and cos / sin(2 pi k (n + N/2) / N) = (-1)^k cos / sin(2 pi k n / N): with separate even-k / odd-k sums (ec, es, oc, os)
//   x[n] ~ (ec + oc) - (es + os),  x[N - n] ~ (ec + oc) + (es + os),  x[N/2 + n] ~ (ec - oc) - (es - os),  x[N/2 - n] ~ (ec - oc) + (es - os).
//
// Overlap-add is a GATHER: a workgroup of the inverse owns hop * G consecutive output samples and holds the dav_istft_frames =
// G + 2 h + 1 frames that cover them (h = (N/2 - 1) / hop frames of halo on each side), windowed, in LDS; an output sample adds
// the at most ceil(N / hop) frames that cover it in increasing frame order, adds w^2 of the same frames for the envelope, and
// divides.  No atomics: two calls agree bit for bit.  The fused kernel recomputes the STFT of the halo frames (12 frames for 9
// hops of output at the reference's geometries) rather than going through memory.
//
// Like probe/ and data/ this file is outside _lib.kernel_source_hash() (csrc/*.hip, csrc/*.h): nothing here runs in the
// pre-training step.
#include "common.h"
#include "dav_kernels.h"

namespace {

constexpr int SEP_FWD_FR = dav_stft_frames;       // frames per workgroup of the plain STFT (256 threads, one group)
constexpr int SEP_INV_FR = dav_istft_frames;      // frames a workgroup of the inverse / fused kernel holds, halo included
constexpr int SEP_GRP = 256;                      // threads of one group: a group owns SEP_INV_FR / 2 frames of the workgroup
constexpr int SEP_HALF = SEP_INV_FR / 2;
constexpr int SEP_INV_THREADS = 2 * SEP_GRP;
constexpr size_t SEP_LDS_MAX = 160 * 1024;

static_assert(SEP_INV_FR % 2 == 0, "the two thread groups of the inverse split its frames evenly");

__host__ __device__ inline int round4(int n) { return (n + 3) & ~3; }

// sample i of the centre-padded (reflect) row; S > N/2 makes one reflection enough
__device__ __forceinline__ float padded_sample(const float* __restrict__ w, int i, int S) {
  if (i < 0) i = -i;
  if (i >= S) i = 2 * (S - 1) - i;
  i = i < 0 ? 0 : (i >= S ? S - 1 : i);
  return w[i];
}

// X[f][k] = sum_n xs[f][n] e^{-2 pi i k n / N} for the NF frames of this group, all N/2 + 1 bins; X rows are XS complex apart
template <int NF>
__device__ __forceinline__ void fwd_dft(const float2* cs, const float* xs, int N, float2* X, int XS, int w, int nw) {
  const int half = N / 2;
  for (int k = w; 2 * k <= half; k += nw) {
    float ere[NF], eim[NF], ore[NF], oim[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) ere[f] = eim[f] = ore[f] = oim[f] = 0.f;
    int idx = 0;                                            // (k * n) mod N, updated incrementally: exact
#pragma unroll 4                                          // the LDS reads of four trips in flight: the loop is bound by their latency
    for (int n = 0; n < N; n += 2) {
      const float2 t0 = cs[idx];                            // (cos, sin) in one 8-byte read
      idx += k;
      if (idx >= N) idx -= N;
      const float2 t1 = cs[idx];
      idx += k;
      if (idx >= N) idx -= N;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const float2 x = *reinterpret_cast<const float2*>(xs + f * N + n);          // wave-uniform address: LDS broadcast
        ere[f] = fmaf(x.x, t0.x, ere[f]);
        eim[f] = fmaf(x.x, t0.y, eim[f]);
        ore[f] = fmaf(x.y, t1.x, ore[f]);
        oim[f] = fmaf(x.y, t1.y, oim[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {                          // Im X = -sum x sin;  sin(2 pi (N/2 - k) n / N) = -(-1)^n sin(2 pi k n / N)
      X[f * XS + k] = float2{ere[f] + ore[f], -(eim[f] + oim[f])};
      X[f * XS + half - k] = float2{ere[f] - ore[f], eim[f] - oim[f]};
    }
  }
}

// y[f][n] = w[n] (2 / N) sum_k Re Y_k cos - Im Y_k sin for the NF frames of this group; Y as staged by the callers: DC and Nyquist
// halved, their imaginary parts zero, the padding bin of an odd n_freqs zero
template <int NF>
__device__ __forceinline__ void inv_dft(const float2* cs, const float* win, const float2* Y, int XS, int N, float* y, int w, int nw) {
  const int half = N / 2;
  const float scale = 2.0f / (float)N;
  for (int n = w; 2 * n <= half; n += nw) {
    float ec[NF], es[NF], oc[NF], os[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) ec[f] = es[f] = oc[f] = os[f] = 0.f;
    int idx = 0;                                            // (k * n) mod N
#pragma unroll 4
    for (int k = 0; k < XS; k += 2) {
      const float2 t0 = cs[idx];
      idx += n;
      if (idx >= N) idx -= N;
      const float2 t1 = cs[idx];
      idx += n;
      if (idx >= N) idx -= N;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(Y + f * XS + k);            // bins k (even) and k + 1: re, im, re, im
        ec[f] = fmaf(v.x, t0.x, ec[f]);
        es[f] = fmaf(v.y, t0.y, es[f]);
        oc[f] = fmaf(v.z, t1.x, oc[f]);
        os[f] = fmaf(v.w, t1.y, os[f]);
      }
    }
    const int i0 = n, i1 = n ? N - n : 0, i2 = half + n, i3 = half - n;
    const float w0 = win[i0], w1 = win[i1], w2 = win[i2], w3 = win[i3];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const float a = ec[f] + oc[f], b = es[f] + os[f], c = ec[f] - oc[f], d = es[f] - os[f];
      float* yf = y + f * N;
      yf[i1] = ((a + b) * scale) * w1;
      yf[i0] = ((a - b) * scale) * w0;
      yf[i3] = ((c + d) * scale) * w3;
      yf[i2] = ((c - d) * scale) * w2;
    }
  }
}

// out[j] = (sum_t y_t[p - t hop]) / (sum_t w[p - t hop]^2), p = j + N/2, over the frames t that cover p, in increasing order;
// y holds the frames t_first .. t_first + SEP_INV_FR - 1
__device__ __forceinline__ void overlap_gather(const float* y, const float* win, int N, int hop, int frames, int t_first, int j0,
                                               int j1, float* __restrict__ orow, int tid, int nthreads) {
  for (int j = j0 + tid; j < j1; j += nthreads) {
    const int p = j + N / 2;
    int t_hi = p / hop;
    t_hi = t_hi < frames - 1 ? t_hi : frames - 1;
    const int t_lo = p - N + 1 <= 0 ? 0 : (p - N + hop) / hop;
    float acc = 0.f, env = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
      const int n = p - t * hop;                            // 0 <= n < N;  0 <= t - t_first < SEP_INV_FR (see sep_geometry)
      const float wn = win[n];
      acc += y[(t - t_first) * N + n];
      env = fmaf(wn, wn, env);
    }
    orow[j] = acc / env;
  }
}

struct SepArgs {
  const float* wave;      // [B][S], row stride wave_rs
  const float* spec;      // plain inverse: [B][n_freqs][frames] complex, row stride spec_rs (complex elements)
  const float* logits;    // fused: [B][K][n_mels][T]
  const float* window;
  const float* cos_tab;
  const float* sin_tab;
  const float* fbank;     // [n_freqs][n_mels]
  const int* band_lo;     // [n_mels]
  const int* band_hi;
  float* out;             // [B][K][L], row stride out_rs
  long wave_rs, spec_rs, out_rs;
  int S, N, hop, n_freqs, frames, XS, G, h, K, n_mels, T, L;
};

__global__ __launch_bounds__(SEP_GRP) void stft_kernel(SepArgs q, float* __restrict__ spec) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int N = q.N, XS = q.XS;
  float2* cs = reinterpret_cast<float2*>(sm);       // [N] (cos, sin)
  float* xs = sm + 2 * round4(N);                   // [SEP_FWD_FR][N] windowed samples
  float2* X = reinterpret_cast<float2*>(xs + round4(SEP_FWD_FR * N));      // [SEP_FWD_FR][XS]
  const int t0 = blockIdx.x * SEP_FWD_FR, b = blockIdx.y, tid = threadIdx.x;
  const float* w = q.wave + (size_t)b * q.wave_rs;
  for (int n = tid; n < N; n += SEP_GRP) cs[n] = float2{q.cos_tab[n], q.sin_tab[n]};
  for (int e = tid; e < SEP_FWD_FR * N; e += SEP_GRP) {
    const int f = e / N, n = e - f * N;
    xs[e] = t0 + f < q.frames ? padded_sample(w, (t0 + f) * q.hop - N / 2 + n, q.S) * q.window[n] : 0.f;
  }
  __syncthreads();
  fwd_dft<SEP_FWD_FR>(cs, xs, N, X, XS, tid, SEP_GRP);
  __syncthreads();
  float2* orow = reinterpret_cast<float2*>(spec) + (size_t)b * q.n_freqs * q.spec_rs;
  for (int e = tid; e < SEP_FWD_FR * q.n_freqs; e += SEP_GRP) {          // frame fastest: a bin row's frames are consecutive
    const int k = e / SEP_FWD_FR, f = e - k * SEP_FWD_FR;
    if (t0 + f < q.frames) orow[(size_t)k * q.spec_rs + t0 + f] = X[f * XS + k];
  }
}

// FUSED = false: Y is read from q.spec.  FUSED = true: the STFT of q.wave once, then for each of the K masks of the batch element
// M[f] = sum_m fbank[f][m] sigmoid(logit[m][t]), Y = M X.
template <bool FUSED>
__global__ __launch_bounds__(SEP_INV_THREADS) void istft_kernel(SepArgs q) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int N = q.N, XS = q.XS, half = N / 2;
  float2* cs = reinterpret_cast<float2*>(sm);       // [N] (cos, sin)
  float* win = sm + 2 * round4(N);                  // [N]
  float* ys = win + round4(N);                      // [SEP_INV_FR][N]: windowed samples going in, windowed inverse frames coming out
  float2* Y = reinterpret_cast<float2*>(ys + round4(SEP_INV_FR * N));     // [SEP_INV_FR][XS]
  float2* X = Y + SEP_INV_FR * XS;                  // fused only from here: [SEP_INV_FR][XS]
  float* sig = reinterpret_cast<float*>(X + SEP_INV_FR * XS);             // [SEP_INV_FR][n_mels]
  int* mlo = reinterpret_cast<int*>(sig + round4(SEP_INV_FR * q.n_mels)); // [n_freqs]: the filters with a weight on bin f are
  int* mhi = mlo + round4(q.n_freqs);               // [n_freqs]            inside [mlo[f], mhi[f])
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int grp = tid / SEP_GRP, wk = tid - grp * SEP_GRP;
  const int t_first = g * q.G - q.h;                // frame of slot 0 (may be < 0: such slots are empty)
  const int j0 = g * q.G * q.hop;
  const int j1 = j0 + q.G * q.hop < q.L ? j0 + q.G * q.hop : q.L;

  for (int n = tid; n < N; n += SEP_INV_THREADS) { cs[n] = float2{q.cos_tab[n], q.sin_tab[n]}; win[n] = q.window[n]; }
  if (FUSED) {
    const float* w = q.wave + (size_t)b * q.wave_rs;
    for (int e = tid; e < SEP_INV_FR * N; e += SEP_INV_THREADS) {
      const int s = e / N, n = e - s * N, t = t_first + s;
      ys[e] = t >= 0 && t < q.frames ? padded_sample(w, t * q.hop - half + n, q.S) * q.window[n] : 0.f;
    }
    for (int f = tid; f < q.n_freqs; f += SEP_INV_THREADS) {
      int lo = q.n_mels, hi = 0;
      for (int m = 0; m < q.n_mels; ++m)
        if (q.band_lo[m] <= f && f < q.band_hi[m]) { lo = m < lo ? m : lo; hi = m + 1; }
      mlo[f] = lo;
      mhi[f] = hi;
    }
    __syncthreads();
    fwd_dft<SEP_HALF>(cs, ys + grp * SEP_HALF * N, N, X + grp * SEP_HALF * XS, XS, wk, SEP_GRP);
  }
  for (int k = 0; k < q.K; ++k) {
    __syncthreads();                                // X complete / the gather of the previous mask done with ys
    if (FUSED) {
      const float* lg = q.logits + ((size_t)b * q.K + k) * q.n_mels * q.T;
      for (int e = tid; e < SEP_INV_FR * q.n_mels; e += SEP_INV_THREADS) {           // frame fastest, as the logits lie
        const int m = e / SEP_INV_FR, s = e - m * SEP_INV_FR, t = t_first + s;
        // the frame behind the last logit column is the zero column the reference appends
        sig[s * q.n_mels + m] = t >= 0 && t < q.T ? 1.0f / (1.0f + expf(-lg[(size_t)m * q.T + t])) : 0.f;
      }
      __syncthreads();
      for (int e = tid; e < SEP_INV_FR * XS; e += SEP_INV_THREADS) {
        const int s = e / XS, f = e - s * XS;
        float2 v = float2{0.f, 0.f};
        if (f < q.n_freqs) {
          float M = 0.f;
          for (int m = mlo[f]; m < mhi[f]; ++m) M = fmaf(q.fbank[(size_t)f * q.n_mels + m], sig[s * q.n_mels + m], M);
          const float2 x = X[e];
          v = (f == 0 || f == half) ? float2{0.5f * (M * x.x), 0.f} : float2{M * x.x, M * x.y};
        }
        Y[e] = v;
      }
    } else {
      const float2* sp = reinterpret_cast<const float2*>(q.spec) + (size_t)b * q.n_freqs * q.spec_rs;
      for (int e = tid; e < SEP_INV_FR * XS; e += SEP_INV_THREADS) {                  // frame fastest, as the spectrum lies
        const int f = e / SEP_INV_FR, s = e - f * SEP_INV_FR, t = t_first + s;
        float2 v = float2{0.f, 0.f};
        if (f < q.n_freqs && t >= 0 && t < q.frames) {
          v = sp[(size_t)f * q.spec_rs + t];
          if (f == 0 || f == half) v = float2{0.5f * v.x, 0.f};
        }
        Y[s * XS + f] = v;
      }
    }
    __syncthreads();
    inv_dft<SEP_HALF>(cs, win, Y + grp * SEP_HALF * XS, XS, N, ys + grp * SEP_HALF * N, wk, SEP_GRP);
    __syncthreads();
    overlap_gather(ys, win, N, q.hop, q.frames, t_first, j0, j1, q.out + ((size_t)b * q.K + k) * q.out_rs, tid, SEP_INV_THREADS);
  }
}

// sizes common to the three entry points; false: refused with DAV_ERR_SHAPE
bool sep_geometry(SepArgs& q, int n_fft, int hop, int frames) {
  if (n_fft <= 0 || (n_fft & 1) || hop <= 0 || frames < 2 || n_fft > (1 << 16) || hop > (1 << 20)) return false;
  if ((long long)hop * (frames - 1) + n_fft > 0x7fffffffLL) return false;
  q.N = n_fft, q.hop = hop, q.frames = frames;
  q.n_freqs = n_fft / 2 + 1;
  q.XS = (q.n_freqs + 1) & ~1;                       // an even number of complex bins per frame: 16-byte reads of bin pairs
  q.h = (n_fft / 2 - 1) / hop;                       // frames of halo on each side of a tile of the inverse
  q.G = SEP_INV_FR - 2 * q.h - 1;                    // hops of output a workgroup owns: the samples [g G hop, (g + 1) G hop) are
  q.L = hop * (frames - 1);                          // covered by the frames g G - h .. g G + G + h, SEP_INV_FR of them
  return true;
}

size_t stft_lds(const SepArgs& q) {
  return ((size_t)2 * round4(q.N) + round4(SEP_FWD_FR * q.N) + (size_t)2 * SEP_FWD_FR * q.XS) * sizeof(float);
}

size_t istft_lds(const SepArgs& q, bool fused) {
  size_t fl = (size_t)3 * round4(q.N) + round4(SEP_INV_FR * q.N) + (size_t)2 * SEP_INV_FR * q.XS;
  if (fused) fl += (size_t)2 * SEP_INV_FR * q.XS + round4(SEP_INV_FR * q.n_mels) + (size_t)2 * round4(q.n_freqs);
  return fl * sizeof(float);
}

template <typename Kern>
int raise_lds(Kern kernel, size_t lds, bool& raised) {
  if (lds > 64 * 1024 && !raised) {                  // once: a workgroup may take the whole 160 KiB of its CU
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEP_LDS_MAX));
    raised = true;
  }
  return DAV_OK;
}

}  // namespace

extern "C" int dav_stft_c32(const float* wave, int B, int S, long wave_rs, int n_fft, int hop, const float* window,
                            const float* cos_tab, const float* sin_tab, float* spec, long spec_rs, hipStream_t stream) {
  if (B <= 0 || B > 65535 || S <= 0 || n_fft <= 0 || hop <= 0 || S <= n_fft / 2) return DAV_ERR_SHAPE;
  SepArgs q = {};
  if (!sep_geometry(q, n_fft, hop, S / hop + 1)) return DAV_ERR_SHAPE;
  if (!wave || !window || !cos_tab || !sin_tab || !spec || wave_rs < S || spec_rs < q.frames) return DAV_ERR_SHAPE;
  const size_t lds = stft_lds(q);
  if (lds > SEP_LDS_MAX) return DAV_ERR_SHAPE;
  if (((uintptr_t)wave | (uintptr_t)window | (uintptr_t)cos_tab | (uintptr_t)sin_tab) & 3) return DAV_ERR_ALIGN;
  if ((uintptr_t)spec & 7) return DAV_ERR_ALIGN;
  static bool raised = false;
  if (raise_lds(stft_kernel, lds, raised) != DAV_OK) return DAV_ERR_HIP;
  q.wave = wave, q.window = window, q.cos_tab = cos_tab, q.sin_tab = sin_tab;
  q.wave_rs = wave_rs, q.spec_rs = spec_rs, q.S = S;
  DAV_LAUNCH(stft_kernel, dim3((q.frames + SEP_FWD_FR - 1) / SEP_FWD_FR, B), dim3(SEP_GRP), lds, stream, q, spec);
  return dav_launch_status();
}

extern "C" int dav_istft_c32(const float* spec, long spec_rs, int B, int frames, int n_fft, int hop, const float* window,
                             const float* cos_tab, const float* sin_tab, float* out, long out_rs, hipStream_t stream) {
  if (B <= 0 || B > 65535) return DAV_ERR_SHAPE;
  SepArgs q = {};
  if (!sep_geometry(q, n_fft, hop, frames) || q.G < 1) return DAV_ERR_SHAPE;
  if (!spec || !window || !cos_tab || !sin_tab || !out || spec_rs < frames || out_rs < q.L) return DAV_ERR_SHAPE;
  const size_t lds = istft_lds(q, false);
  if (lds > SEP_LDS_MAX) return DAV_ERR_SHAPE;
  if (((uintptr_t)out | (uintptr_t)window | (uintptr_t)cos_tab | (uintptr_t)sin_tab) & 3) return DAV_ERR_ALIGN;
  if ((uintptr_t)spec & 7) return DAV_ERR_ALIGN;
  static bool raised = false;
  if (raise_lds(istft_kernel<false>, lds, raised) != DAV_OK) return DAV_ERR_HIP;
  q.spec = spec, q.window = window, q.cos_tab = cos_tab, q.sin_tab = sin_tab, q.out = out;
  q.spec_rs = spec_rs, q.out_rs = out_rs, q.K = 1;
  const int tile = q.G * hop;
  DAV_LAUNCH(istft_kernel<false>, dim3((q.L + tile - 1) / tile, B), dim3(SEP_INV_THREADS), lds, stream, q);
  return dav_launch_status();
}

extern "C" int dav_sep_mask_istft(const float* wave, int B, int S, long wave_rs, const float* logits, int K, int n_mels, int T,
                                  int n_fft, int hop, const float* window, const float* cos_tab, const float* sin_tab,
                                  const float* fbank, const int* band_lo, const int* band_hi, float* out, long out_rs,
                                  hipStream_t stream) {
  if (B <= 0 || B > 65535 || K <= 0 || K > 65535 || n_mels <= 0 || n_mels > (1 << 16) || T <= 0 || S <= 0 || n_fft <= 0 || hop <= 0 ||
      S <= n_fft / 2)
    return DAV_ERR_SHAPE;
  SepArgs q = {};
  if (!sep_geometry(q, n_fft, hop, S / hop + 1) || q.G < 1) return DAV_ERR_SHAPE;
  if (T + 1 != q.frames) return DAV_ERR_SHAPE;       // the last frame's mask is the zero column the reference appends
  if (!wave || !logits || !window || !cos_tab || !sin_tab || !fbank || !band_lo || !band_hi || !out || wave_rs < S || out_rs < q.L)
    return DAV_ERR_SHAPE;
  q.n_mels = n_mels;
  const size_t lds = istft_lds(q, true);
  if (lds > SEP_LDS_MAX) return DAV_ERR_SHAPE;
  if (((uintptr_t)wave | (uintptr_t)logits | (uintptr_t)window | (uintptr_t)cos_tab | (uintptr_t)sin_tab | (uintptr_t)fbank |
       (uintptr_t)band_lo | (uintptr_t)band_hi | (uintptr_t)out) & 3)
    return DAV_ERR_ALIGN;
  static bool raised = false;
  if (raise_lds(istft_kernel<true>, lds, raised) != DAV_OK) return DAV_ERR_HIP;
  q.wave = wave, q.logits = logits, q.window = window, q.cos_tab = cos_tab, q.sin_tab = sin_tab;
  q.fbank = fbank, q.band_lo = band_lo, q.band_hi = band_hi, q.out = out;
  q.wave_rs = wave_rs, q.out_rs = out_rs, q.S = S, q.K = K, q.T = T;
  const int tile = q.G * hop;
  DAV_LAUNCH(istft_kernel<true>, dim3((q.L + tile - 1) / tile, B), dim3(SEP_INV_THREADS), lds, stream, q);
  return dav_launch_status();
}
