// Fusion attention maps: how strongly every image region of frame t attends to that frame's audio token in the spatial fusion
// block -- the audio-visual correlation map the reference draws per head (slowfast/visualization/visualization.py, vis_av_st_fusion:
// attn[:, :, HW t : HW (t + 1), THW + t], trilinear upsample to T x S x S, per-frame min-max).  include/csts_hip.h states the rule.
//
// Only heads * T' * HW of the (N, N) probabilities are wanted, so nothing of that matrix is formed: one wave-64 dot per wanted
// (query, key) pair against the row's log-sum-exp the attention forward already left.  Two launches behind the one entry:
//   apa_column_kernel  one workgroup per (b, head, t): the frame's audio key sits in registers, a wave walks the frame's queries;
//   apa_maps_kernel    one workgroup per (b, input frame j, head or head mean): the temporal mix of two coarse maps in LDS, the
//                      extrema of its bilinear upsample over the S x S lattice from the end pixels of every cell interval (a
//                      bilinear patch is extremal at its corners: 2h x 2w evaluations instead of S^2), the rescaled coarse map
//                      out; B * T' further workgroups of the same launch write the head mean of the column.
#include "common.h"

namespace {

constexpr int APA_KREG = CSTS_AUDIO_PIXEL_MAX_HD / 64;      // key elements a lane holds
constexpr int APA_MAX_SIDE = CSTS_AUDIO_PIXEL_MAX_SIDE;
constexpr int APA_MAX_CELLS = CSTS_AUDIO_PIXEL_MAX_HW;

// grid B * Hh * T', 256 threads.  qkv (B, N, 3C): q at column 0, k at column C; head k at k * hd.
__global__ __launch_bounds__(256) void apa_column_kernel(const void* __restrict__ qkv, int dt, const float* __restrict__ lse,
                                                         float* __restrict__ column, int Hh, int hd, int Tp, int HW,
                                                         float scale_log2) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int t = blockIdx.x % Tp;
  const int head = (blockIdx.x / Tp) % Hh;
  const int64_t b = blockIdx.x / (Tp * Hh);
  const int64_t N = (int64_t)Tp * HW + Tp, C3 = 3 * (int64_t)Hh * hd;
  const int64_t base = b * N * C3 + (int64_t)head * hd;
  const int64_t ko = base + ((int64_t)Tp * HW + t) * C3 + (int64_t)Hh * hd;
  float kreg[APA_KREG];
#pragma unroll
  for (int i = 0; i < APA_KREG; ++i) {
    const int d = lane + 64 * i;
    kreg[i] = d < hd ? ld_as_f32(qkv, dt, ko + d) : 0.f;
  }
  const float* L = lse + (b * Hh + head) * N + (int64_t)t * HW;
  float* out = column + ((b * Hh + head) * Tp + t) * (int64_t)HW;
  for (int c = wv; c < HW; c += 4) {                            // wave-uniform
    const int64_t qo = base + ((int64_t)t * HW + c) * C3;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < APA_KREG; ++i) {
      const int d = lane + 64 * i;
      if (d < hd) s += ld_as_f32(qkv, dt, qo + d) * kreg[i];
    }
    s = wave_sum(s);
    if (lane == 0) out[c] = exp2f(s * scale_log2 - L[c]);
  }
}

struct ApaAxis { int i0, i1; float lam; };

// One axis of the align_corners=False upsample, exactly: lattice point p of S on an axis of m cells sits at
// max((p + 0.5) m / S - 0.5, 0) = max(A / D, 0), A = (2p + 1) m - S, D = 2S.  Used for time (p = input frame) and space alike.
__device__ inline ApaAxis apa_axis(int p, int S, int m) {
  const int64_t A = (int64_t)(2 * p + 1) * m - S, D = 2 * (int64_t)S;
  ApaAxis a = {0, 0, 0.f};
  if (A > 0) {
    const int64_t q = A / D;
    a.i0 = (int)(q < m - 1 ? q : m - 1);
    a.lam = (float)(A - q * D) / (float)D;
  }
  a.i1 = min(a.i0 + 1, m - 1);
  return a;
}

// the head mean of the column at one cell: ((0 + c_0) + c_1 + ...) / Hh in fp32, heads ascending
__device__ __forceinline__ float apa_head_mean(const float* __restrict__ col, int Hh, int64_t head_stride) {
  float s = 0.f;
  for (int k = 0; k < Hh; ++k) s += col[k * head_stride];
  return s / (float)Hh;
}

// The end pixels of every run of lattice points that share the lower cell i0 = k: slot 2k the first, slot 2k + 1 the last;
// i0 < 0 marks an empty slot (a cell no lattice point falls into, when S < m).
__device__ inline void apa_end_pixels(ApaAxis* ends, int S, int m, int tid) {
  for (int k = tid; k < 2 * m; k += 256) ends[k].i0 = -1;
  __syncthreads();
  for (int p = tid; p < S; p += 256) {
    const ApaAxis a = apa_axis(p, S, m);
    if (p == 0 || apa_axis(p - 1, S, m).i0 != a.i0) ends[2 * a.i0] = a;
    if (p == S - 1 || apa_axis(p + 1, S, m).i0 != a.i0) ends[2 * a.i0 + 1] = a;
  }
}

// grid B * T * (Hh + 1) + B * T', 256 threads
__global__ __launch_bounds__(256) void apa_maps_kernel(const float* __restrict__ column, float* __restrict__ column_mean,
                                                       float* __restrict__ maps, float* __restrict__ range, int B, int Hh, int Tp,
                                                       int h, int w, int T, int S) {
  __shared__ float m[APA_MAX_CELLS];
  __shared__ ApaAxis ey[2 * APA_MAX_SIDE], ex[2 * APA_MAX_SIDE];
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = h * w;
  const int64_t head_stride = (int64_t)Tp * HW;
  const int map_blocks = B * T * (Hh + 1);
  if ((int)blockIdx.x >= map_blocks) {                          // the head mean of the column, frame (b, t)
    const int r = blockIdx.x - map_blocks;
    const int t = r % Tp;
    const int64_t b = r / Tp;
    const float* col = column + b * Hh * head_stride + (int64_t)t * HW;
    float* out = column_mean + (b * Tp + t) * (int64_t)HW;
    for (int c = tid; c < HW; c += 256) out[c] = apa_head_mean(col + c, Hh, head_stride);
    return;
  }
  const int g = blockIdx.x % (Hh + 1);
  const int j = (blockIdx.x / (Hh + 1)) % T;
  const int64_t b = blockIdx.x / ((Hh + 1) * T);
  const ApaAxis at = apa_axis(j, T, Tp);
  const float w0 = 1.0f - at.lam, w1 = at.lam;
  const float* cb = column + b * Hh * head_stride;
  for (int c = tid; c < HW; c += 256) {
    float a0, a1;
    if (g < Hh) {
      a0 = cb[g * head_stride + (int64_t)at.i0 * HW + c];
      a1 = cb[g * head_stride + (int64_t)at.i1 * HW + c];
    } else {
      a0 = apa_head_mean(cb + (int64_t)at.i0 * HW + c, Hh, head_stride);
      a1 = apa_head_mean(cb + (int64_t)at.i1 * HW + c, Hh, head_stride);
    }
    m[c] = w0 * a0 + w1 * a1;                                   // two products, one sum (no contraction)
  }
  apa_end_pixels(ey, S, h, tid);
  apa_end_pixels(ex, S, w, tid);
  __syncthreads();
  float lo = INFINITY, hi = -INFINITY;
  const int ny = 2 * h, nx = 2 * w;
  for (int e = tid; e < ny * nx; e += 256) {
    const ApaAxis y = ey[e / nx], x = ex[e % nx];
    if (y.i0 < 0 || x.i0 < 0) continue;
    const float m00 = m[y.i0 * w + x.i0], m01 = m[y.i0 * w + x.i1], m10 = m[y.i1 * w + x.i0], m11 = m[y.i1 * w + x.i1];
    const float top = fmaf(x.lam, m01 - m00, m00), bot = fmaf(x.lam, m11 - m10, m10);
    const float v = fmaf(y.lam, bot - top, top);                // the overlay's sample of the same point
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  lo = -wave_max(-lo);
  hi = wave_max(hi);
  if (lane == 0) { red[wv] = lo; red[4 + wv] = hi; }
  __syncthreads();
  lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  const int64_t o = (b * (Hh + 1) + g) * T + j;
  const float den = hi - lo + 1e-6f;
  for (int c = tid; c < HW; c += 256) maps[o * HW + c] = (m[c] - lo) / den;
  if (tid == 0) { range[2 * o] = lo; range[2 * o + 1] = hi; }
}

}  // namespace

extern "C" int csts_audio_pixel_attn(const void* qkv, int dt, const float* lse, int B, int heads, int head_dim, int Tp, int h,
                                     int w, int T, int S, float scale, float* column, float* column_mean, float* maps,
                                     float* range, hipStream_t stream) {
  CSTS_REQUIRE(qkv && lse && column && column_mean && maps && range, "bad args (no pointer may be NULL)");
  CSTS_REQUIRE(dt == CSTS_F32 || dt == CSTS_BF16, "dtype must be CSTS_F32 or CSTS_BF16");
  CSTS_REQUIRE(B >= 1 && heads >= 1 && head_dim >= 1 && head_dim <= CSTS_AUDIO_PIXEL_MAX_HD,
               "B >= 1, heads >= 1, 1 <= head_dim <= CSTS_AUDIO_PIXEL_MAX_HD (a lane holds the key in registers)");
  CSTS_REQUIRE(Tp >= 1 && h >= 1 && w >= 1 && h <= APA_MAX_SIDE && w <= APA_MAX_SIDE && (int64_t)h * w <= APA_MAX_CELLS,
               "1 <= h, w <= CSTS_AUDIO_PIXEL_MAX_SIDE and h * w <= CSTS_AUDIO_PIXEL_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(T >= 1 && T <= 65536 && Tp <= 65536 && S >= 1 && S <= 65536, "1 <= T, T', S <= 65536");
  const int64_t col_blocks = (int64_t)B * heads * Tp, map_blocks = (int64_t)B * T * (heads + 1) + (int64_t)B * Tp;
  const int64_t N = (int64_t)Tp * h * w + Tp;
  CSTS_REQUIRE(col_blocks < ((int64_t)1 << 31) && map_blocks < ((int64_t)1 << 31) && N * 3 * heads * head_dim < ((int64_t)1 << 31),
               "B * heads * T', B * (T * (heads + 1) + T') and one clip's N * 3C must stay below 2^31");
  hipLaunchKernelGGL(apa_column_kernel, dim3((unsigned)col_blocks), dim3(256), 0, stream, qkv, dt, lse, column, heads, head_dim, Tp,
                     h * w, scale * 1.4426950408889634f);
  CSTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(apa_maps_kernel, dim3((unsigned)map_blocks), dim3(256), 0, stream, (const float*)column, column_mean, maps,
                     range, B, heads, Tp, h, w, T, S);
  CSTS_LAUNCH_CHECK();
  return 0;
}
