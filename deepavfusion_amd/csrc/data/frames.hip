// Frame transform of the input stage on the GPU: the image half of the reference's loader transforms,
//   RandomResizedCrop(size, scale=(crop_min, 1)) -> RandomHorizontalFlip -> ToTensor -> Normalize      (train.py:45-49)
//   Resize(int(size / 0.875)) -> CenterCrop(size) -> ToTensor -> Normalize                             (util/knn_probe.py:31-36)
// as ONE kernel over a batch of uint8 HWC frames: crop, antialiased bilinear resample, flip, /255, (x - mean) / std -> fp32 CHW.
//
// The resampling is the separable triangle filter of PIL's Image.resize(BILINEAR) / F.interpolate(bilinear, antialias=True):
// per axis, n_in source pixels -> n_out virtual outputs, scale = n_in / n_out, support = max(scale, 1), centre of output o
// c = (o + 0.5) scale, tap k weighs max(0, 1 - |k - c + 0.5| / support), weights divided by their sum.  With D = 2 max(n_in, n_out)
// the weight of tap k is the INTEGER max(0, D - |2 n_out k - (2 o + 1) n_in + n_out|) over D — exact, no rounding of the centre or
// of the weights (an fp32 centre near column 480 would be off by 3e-5 pixels = 8e-3 grey levels on noise); only the products with
// the pixel values and the two final divisions by the weight sums are rounded (fp32).  No uint8 rounding between or after the
// passes.  A tap outside [klo, khi) of the rule has weight 0, so the loops only need the union of the ranges.
//
// One wave per (band of FT_ROWS output rows, channel, sample); a lane owns 4 consecutive output columns (one 16-byte store per
// row).  For every source row the band needs, the lane filters it horizontally ONCE for its 4 columns and adds the result into the
// FT_ROWS row accumulators with the (wave-uniform) vertical weights: 1 + (2 support + 1) / FT_ROWS horizontal passes per output
// row instead of 2 support + 1.  Source bytes are read straight from global memory: a band touches a few KiB of one frame, which
// stays in the CU's vector cache.  Every source index is clamped into the frame and every parameter into a sane range, so a bad
// parameter row gives a wrong picture, never an out-of-bounds access or an unbounded loop.
#include "common.h"
#include "dav_kernels.h"

namespace {

constexpr int FT_ROWS = 8;         // output rows per wave (S % 16 == 0, so bands never straddle the end)
constexpr int FT_MAX = 16384;      // largest frame side / virtual output side: keeps 2 n_out k and (2 o + 1) n_in inside int32

struct FrameNorm { float scale[3], shift[3]; };     // out = v * scale[c] + shift[c]  with scale = 1 / (255 std), shift = -mean / std

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// taps [lo, hi) of virtual output o: lo = max(int(c - support + 0.5), 0), hi = min(int(c + support + 0.5), n_in), in integers
__device__ __forceinline__ void tap_range(int o, int n_in, int n_out, int D, int& lo, int& hi) {
  const int a = (2 * o + 1) * n_in + n_out;
  lo = a - D < 0 ? 0 : (a - D) / (2 * n_out);
  hi = (a + D) / (2 * n_out);
  hi = hi > n_in ? n_in : hi;
}

__global__ __launch_bounds__(64) void frame_transform_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                             const int* __restrict__ params, int S, FrameNorm nrm,
                                                             float* __restrict__ out) {
  const int b = blockIdx.z, c = blockIdx.y, oy0 = blockIdx.x * FT_ROWS;
  const int* p = params + b * 9;
  // the source window, clamped into the frame; the virtual output and the emitted window inside it, clamped likewise
  const int bi = clampi(p[0], 0, H - 1), bj = clampi(p[1], 0, W - 1);
  const int nh = clampi(p[2], 1, H - bi), nw = clampi(p[3], 1, W - bj);
  const int RH = clampi(p[4], 1, FT_MAX), RW = clampi(p[5], 1, FT_MAX);
  const int top = clampi(p[6], 0, RH > S ? RH - S : 0), left = clampi(p[7], 0, RW > S ? RW - S : 0);
  const int flip = p[8] != 0;
  const int Dy = 2 * (nh > RH ? nh : RH), Dx = 2 * (nw > RW ? nw : RW);
  const uint8_t* src = frames + (size_t)b * H * W * 3 + c;

  int ylo, yhi, t;
  tap_range(top + oy0, nh, RH, Dy, ylo, t);
  tap_range(top + oy0 + FT_ROWS - 1, nh, RH, Dy, t, yhi);
  int ycen[FT_ROWS];                                                  // (2 vy + 1) n_in - n_out per row of the band
#pragma unroll
  for (int r = 0; r < FT_ROWS; ++r) ycen[r] = (2 * (top + oy0 + r) + 1) * nh - RH;

  for (int ox0 = threadIdx.x * 4; ox0 < S; ox0 += 256) {
    int xlo[4], xhi[4], xcen[4];
    float xinv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int vx = left + (flip ? S - 1 - (ox0 + j) : ox0 + j);
      tap_range(vx, nw, RW, Dx, xlo[j], xhi[j]);
      xcen[j] = (2 * vx + 1) * nw - RW;
      int s = 0;
      for (int x = xlo[j]; x < xhi[j]; ++x) {
        const int d = abs(2 * RW * x - xcen[j]);
        s += d < Dx ? Dx - d : 0;
      }
      xinv[j] = 1.0f / (float)s;
    }
    float acc[FT_ROWS][4];
    int ysum[FT_ROWS];
#pragma unroll
    for (int r = 0; r < FT_ROWS; ++r) {
      ysum[r] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[r][j] = 0.f;
    }
    for (int y = ylo; y < yhi; ++y) {
      const uint8_t* row = src + (size_t)(bi + y) * W * 3;            // bi + y <= bi + nh - 1 <= H - 1
      float hv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float h = 0.f;
        for (int x = xlo[j]; x < xhi[j]; ++x) {
          const int d = abs(2 * RW * x - xcen[j]);
          const int w = d < Dx ? Dx - d : 0;
          h = fmaf((float)w, (float)row[(bj + x) * 3], h);            // bj + x <= bj + nw - 1 <= W - 1
        }
        hv[j] = h * xinv[j];
      }
#pragma unroll
      for (int r = 0; r < FT_ROWS; ++r) {
        const int d = abs(2 * RH * y - ycen[r]);
        const int w = d < Dy ? Dy - d : 0;
        ysum[r] += w;
        const float wf = (float)w;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = fmaf(wf, hv[j], acc[r][j]);
      }
    }
    const float sc = nrm.scale[c], sh = nrm.shift[c];
#pragma unroll
    for (int r = 0; r < FT_ROWS; ++r) {
      const float k = sc / (float)ysum[r];
      const f32x4 v = {fmaf(acc[r][0], k, sh), fmaf(acc[r][1], k, sh), fmaf(acc[r][2], k, sh), fmaf(acc[r][3], k, sh)};
      *reinterpret_cast<f32x4*>(out + (((size_t)b * 3 + c) * S + oy0 + r) * S + ox0) = v;
    }
  }
}

}  // namespace

extern "C" int dav_frame_transform_u8(const uint8_t* frames, int B, int H, int W, const int* params, int S, float mean0,
                                      float mean1, float mean2, float std0, float std1, float std2, float* out,
                                      hipStream_t stream) {
  if (B <= 0 || H <= 0 || W <= 0 || S <= 0 || S % 16) return DAV_ERR_SHAPE;
  if (B > 65535 || H > FT_MAX || W > FT_MAX || S > FT_MAX) return DAV_ERR_SHAPE;
  if (!frames || !params || !out || !(std0 > 0.f) || !(std1 > 0.f) || !(std2 > 0.f)) return DAV_ERR_SHAPE;
  if (((uintptr_t)out & 15) || ((uintptr_t)params & 3)) return DAV_ERR_ALIGN;
  const float mean[3] = {mean0, mean1, mean2}, sd[3] = {std0, std1, std2};
  FrameNorm nrm;
  for (int c = 0; c < 3; ++c) {
    nrm.scale[c] = 1.0f / (255.0f * sd[c]);
    nrm.shift[c] = -mean[c] / sd[c];
  }
  DAV_LAUNCH(frame_transform_kernel, dim3(S / FT_ROWS, 3, B), dim3(64), 0, stream, frames, H, W, params, S, nrm, out);
  return dav_launch_status();
}
