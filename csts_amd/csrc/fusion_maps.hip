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
// The whole-recording track (csts_attention_track) reuses the pieces: the per-pair map is apa_pair_cell (time mix, head mean), the
// extrema and the rescale are apa_lattice_range / apa_rescale_store, the very device functions apa_maps_kernel runs, so a frame
// one pair hits carries that kernel's bits.
//   apt_accumulate_kernel  one workgroup per (output frame f, head or head mean): walks the frame's pair list, the sum in LDS
//                          cells each thread owns, then the mean;
//   apa_rescale_kernel     one workgroup per (f, g): the map into LDS, lattice extrema, rescaled map and range out.
// The live attention ring (csts_live_attention_add / csts_live_attention_rows, GazeStream(live=..., attention=True)) holds that
// track's per-frame sums for the frames a running stream still shows: frame t in slot t mod Ra.
//   live_attention_add_kernel   one workgroup per ring slot: the pairs of newly run windows that land on the slot's frame, added
//                               by apa_pair_cell in ascending p -- apt_accumulate_kernel's sum, carried from call to call;
//   live_attention_rows_kernel  one workgroup per (pushed frame, g): the newest frame at most max_age back that holds a map, its
//                               mean into LDS, then apa_lattice_range / apa_rescale_store as apa_rescale_kernel runs them.
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

// cell c of the map of (clip cb, input frame axis `at`, index g): fl(fl((1 - lambda) col[t0]) + fl(lambda col[t1])), for the head
// mean (g == Hh) on the head means of the two coarse maps.  Two products, one sum (no contraction).
__device__ __forceinline__ float apa_pair_cell(const float* __restrict__ cb, int g, int Hh, int64_t head_stride, int HW,
                                               const ApaAxis& at, int c) {
  const float w0 = 1.0f - at.lam, w1 = at.lam;
  float a0, a1;
  if (g < Hh) {
    a0 = cb[g * head_stride + (int64_t)at.i0 * HW + c];
    a1 = cb[g * head_stride + (int64_t)at.i1 * HW + c];
  } else {
    a0 = apa_head_mean(cb + (int64_t)at.i0 * HW + c, Hh, head_stride);
    a1 = apa_head_mean(cb + (int64_t)at.i1 * HW + c, Hh, head_stride);
  }
  return w0 * a0 + w1 * a1;
}

// (lo, hi) of the bilinear upsample of the LDS map m (h x w, written by this workgroup's threads; the barrier is in here) over
// the S x S lattice, from the end pixels.  Every thread returns the same pair.  256 threads.
__device__ inline void apa_lattice_range(const float* m, ApaAxis* ey, ApaAxis* ex, float* red, int h, int w, int S, int tid,
                                         float& lo_out, float& hi_out) {
  const int lane = tid & 63, wv = tid >> 6;
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
  lo_out = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  hi_out = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

// maps[o] = (m - lo) / (hi - lo + 1e-6), range[o] = (lo, hi)
__device__ __forceinline__ void apa_rescale_store(const float* m, float lo, float hi, int HW, int64_t o, float* __restrict__ maps,
                                                  float* __restrict__ range, int tid) {
  const float den = hi - lo + 1e-6f;
  for (int c = tid; c < HW; c += 256) maps[o * HW + c] = (m[c] - lo) / den;
  if (tid == 0) { range[2 * o] = lo; range[2 * o + 1] = hi; }
}

// grid B * T * (Hh + 1) + B * T', 256 threads
__global__ __launch_bounds__(256) void apa_maps_kernel(const float* __restrict__ column, float* __restrict__ column_mean,
                                                       float* __restrict__ maps, float* __restrict__ range, int B, int Hh, int Tp,
                                                       int h, int w, int T, int S) {
  __shared__ float m[APA_MAX_CELLS];
  __shared__ ApaAxis ey[2 * APA_MAX_SIDE], ex[2 * APA_MAX_SIDE];
  __shared__ float red[8];
  const int tid = threadIdx.x;
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
  const float* cb = column + b * Hh * head_stride;
  for (int c = tid; c < HW; c += 256) m[c] = apa_pair_cell(cb, g, Hh, head_stride, HW, at, c);
  float lo, hi;
  apa_lattice_range(m, ey, ex, red, h, w, S, tid, lo, hi);
  apa_rescale_store(m, lo, hi, HW, (b * (Hh + 1) + g) * T + j, maps, range, tid);
}

// grid F * (Hh + 1), 256 threads: mixed[f][g] = the mean of the maps of the pairs order[offsets[f] .. offsets[f + 1]), count[f].
// Thread tid owns cells tid, tid + 256, ... of the LDS sum: no barrier between pairs.  A list bound outside [0, P] is clamped
// and a pair outside [0, P) skipped (neither happens with the lists ops.attention_track builds), so no read leaves column/order.
__global__ __launch_bounds__(256) void apt_accumulate_kernel(const float* __restrict__ column, const int* __restrict__ order,
                                                             const int* __restrict__ offsets, int Wn, int Hh, int Tp, int HW,
                                                             int T, float* __restrict__ mixed, int* __restrict__ count) {
  __shared__ float m[APA_MAX_CELLS];
  const int tid = threadIdx.x;
  const int g = blockIdx.x % (Hh + 1);
  const int64_t f = blockIdx.x / (Hh + 1);
  const int64_t head_stride = (int64_t)Tp * HW;
  const int64_t P = (int64_t)Wn * T;
  const int beg = max(offsets[f], 0);
  const int end = (int)min((int64_t)offsets[f + 1], P);
  const int n = max(end - beg, 0);
  for (int c = tid; c < HW; c += 256) m[c] = 0.f;
  for (int i = beg; i < end; ++i) {                             // workgroup-uniform
    const int p = order[i];
    if (p < 0 || p >= P) continue;
    const ApaAxis at = apa_axis(p % T, T, Tp);
    const float* cb = column + (int64_t)(p / T) * Hh * head_stride;
    for (int c = tid; c < HW; c += 256) m[c] += apa_pair_cell(cb, g, Hh, head_stride, HW, at, c);
  }
  const float inv = n > 0 ? 1.f / (float)n : 0.f;
  float* out = mixed + (f * (Hh + 1) + g) * (int64_t)HW;
  for (int c = tid; c < HW; c += 256) out[c] = m[c] * inv;
  if (g == 0 && tid == 0) count[f] = n;
}

// grid F * G, 256 threads: maps / range of mixed[f][g]; a frame with valid[f] <= 0 gets maps 0 and range NaN.
__global__ __launch_bounds__(256) void apa_rescale_kernel(const float* __restrict__ mixed, const int* __restrict__ valid, int G,
                                                          int h, int w, int S, float* __restrict__ maps,
                                                          float* __restrict__ range) {
  __shared__ float m[APA_MAX_CELLS];
  __shared__ ApaAxis ey[2 * APA_MAX_SIDE], ex[2 * APA_MAX_SIDE];
  __shared__ float red[8];
  const int tid = threadIdx.x;
  const int HW = h * w;
  const int64_t o = blockIdx.x, f = o / G;
  if (valid && valid[f] <= 0) {                                 // workgroup-uniform
    for (int c = tid; c < HW; c += 256) maps[o * HW + c] = 0.f;
    if (tid == 0) { range[2 * o] = NAN; range[2 * o + 1] = NAN; }
    return;
  }
  for (int c = tid; c < HW; c += 256) m[c] = mixed[o * HW + c];
  float lo, hi;
  apa_lattice_range(m, ey, ex, red, h, w, S, tid, lo, hi);
  apa_rescale_store(m, lo, hi, HW, o, maps, range, tid);
}

// ---- live attention ring: sum (Ra, Hh + 1, HW) / count (Ra) / tag (Ra), the tag being the frame a slot holds (-1: empty).

// grid (Ra), 256 threads.  Workgroup s OWNS slot s: its (Hh + 1) * HW cells, its count and its tag -- every lane reads tag and
// count before the barrier, lane 0 writes them after the last cell (the hazard live_add_slot of stream.hip states: a slot split
// over several workgroups would let one read the tag another has rewritten).  The pairs p = w T + j are walked in ascending p
// and those with frames[p] = t >= 0, t mod Ra == s are taken by live_add_slot's rule: tag != t -> the slot restarts (sum =
// 0.f + m_p, count 1, tag t); tag == t -> sum += m_p, count += 1; m_p = apa_pair_cell(.., g, .., apa_axis(j, T, T'), c), the
// addend of apt_accumulate_kernel.  Two walks as there: the tags alone find the last restart (`start`, -1: the sum in the ring
// is carried on), the final tag and count; then each thread adds, for its own cells, the pairs from there on that carry the
// final tag.  frames[] is read by p alone: uniform loads.  VEC: HW % 4 == 0, a thread's 4 cells share g, 128-bit ring accesses.
template <bool VEC>
__global__ __launch_bounds__(256) void live_attention_add_kernel(const float* __restrict__ column, const int64_t* __restrict__ frames,
                                                                 int P, int Hh, int Tp, int HW, int T, float* __restrict__ sum,
                                                                 int* __restrict__ count, int64_t* __restrict__ tag, int Ra) {
  const int tid = threadIdx.x, slot = blockIdx.x;
  int64_t cur = tag[slot];
  int cnt = count[slot], start = -1, hits = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t t = frames[p];
    if (t < 0 || (int)(t % Ra) != slot) continue;
    ++hits;
    if (t != cur) { cur = t; cnt = 1; start = p; } else { ++cnt; }
  }
  if (hits == 0) return;                                        // workgroup-uniform: it depends on the table alone
  __syncthreads();                                              // every lane has read the old tag and count
  const int first = start < 0 ? 0 : start;
  const int cells = (Hh + 1) * HW;
  const int64_t head_stride = (int64_t)Tp * HW;
  float* dst = sum + (int64_t)slot * cells;
  constexpr int V = VEC ? 4 : 1;
  for (int at = tid * V; at < cells; at += 256 * V) {
    const int g = at / HW, c = at - g * HW;
    float acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.f;
    if (start < 0) {
      if constexpr (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(dst + at);
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = v[q];
      } else {
        acc[0] = dst[at];
      }
    }
    for (int p = first; p < P; ++p) {
      if (frames[p] != cur) continue;                           // from `start` on the slot's pairs all carry its final tag (>= 0)
      const ApaAxis ax = apa_axis(p % T, T, Tp);
      const float* cb = column + (int64_t)(p / T) * Hh * head_stride;
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] += apa_pair_cell(cb, g, Hh, head_stride, HW, ax, c + q);
    }
    if constexpr (VEC) {
      f32x4 o;
#pragma unroll
      for (int q = 0; q < V; ++q) o[q] = acc[q];
      *reinterpret_cast<f32x4*>(dst + at) = o;
    } else {
      dst[at] = acc[0];
    }
  }
  if (tid == 0) { count[slot] = cnt; tag[slot] = cur; }
}

// grid (K, Hh + 1), 256 threads: workgroup (k, g) answers frame n = f0 + k.  It walks j = n .. max(0, n - max_age) for the first
// slot whose tag is j and whose count is positive (workgroup-uniform: the ring is only read, by block index alone), stages
// sum * (1.f / (float)count) -- apt_accumulate_kernel's mean -- in LDS and runs apa_rescale_kernel's two device functions on it.
// Nothing found: mixed and maps 0, range NaN, out_frame -1, out_count 0.  mixed, maps + range, out_frame, out_count: NULL skips.
template <bool VEC>
__global__ __launch_bounds__(256) void live_attention_rows_kernel(const float* __restrict__ sum, const int* __restrict__ count,
                                                                  const int64_t* __restrict__ tag, int Ra, int64_t f0, int h, int w,
                                                                  int S, int max_age, float* __restrict__ mixed,
                                                                  float* __restrict__ maps, float* __restrict__ range,
                                                                  int64_t* __restrict__ out_frame, int* __restrict__ out_count) {
  __shared__ __attribute__((aligned(16))) float m[APA_MAX_CELLS];
  __shared__ ApaAxis ey[2 * APA_MAX_SIDE], ex[2 * APA_MAX_SIDE];
  __shared__ float red[8];
  const int tid = threadIdx.x;
  const int HW = h * w, G = gridDim.y, g = blockIdx.y;
  const int64_t k = blockIdx.x, n = f0 + k, o = k * G + g;
  const int64_t lo_j = n - max_age > 0 ? n - max_age : 0;
  int64_t found = -1;
  int slot = 0, cnt = 0;
  for (int64_t j = n; j >= lo_j; --j) {
    const int s = (int)(j % Ra);
    if (tag[s] == j && count[s] > 0) { found = j; slot = s; cnt = count[s]; break; }
  }
  if (g == 0 && tid == 0) {
    if (out_frame) out_frame[k] = found;
    if (out_count) out_count[k] = cnt;
  }
  if (found < 0) {
    for (int c = tid; c < HW; c += 256) {
      if (mixed) mixed[o * HW + c] = 0.f;
      if (maps) maps[o * HW + c] = 0.f;
    }
    if (maps && tid == 0) { range[2 * o] = NAN; range[2 * o + 1] = NAN; }
    return;
  }
  if (!mixed && !maps) return;
  const float inv = 1.f / (float)cnt;
  const float* src = sum + ((int64_t)slot * G + g) * HW;
  if constexpr (VEC) {
    for (int c = tid * 4; c < HW; c += 1024) {
      f32x4 v = *reinterpret_cast<const f32x4*>(src + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] *= inv;
      *reinterpret_cast<f32x4*>(m + c) = v;
      if (mixed) *reinterpret_cast<f32x4*>(mixed + o * HW + c) = v;
    }
  } else {
    for (int c = tid; c < HW; c += 256) {
      const float v = src[c] * inv;
      m[c] = v;
      if (mixed) mixed[o * HW + c] = v;
    }
  }
  if (!maps) return;
  float lo, hi;
  apa_lattice_range(m, ey, ex, red, h, w, S, tid, lo, hi);      // its first barrier orders the writes of m
  apa_rescale_store(m, lo, hi, HW, o, maps, range, tid);
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

extern "C" int csts_attention_rescale(const float* mixed, const int* valid, int nmaps_per_frame, int64_t F, int h, int w, int S,
                                      float* maps, float* range, hipStream_t stream) {
  CSTS_REQUIRE(mixed && maps && range, "bad args (only valid may be NULL)");
  CSTS_REQUIRE(maps != mixed, "maps must not be mixed (the workgroup reads its map after others may have written theirs)");
  CSTS_REQUIRE(h >= 1 && w >= 1 && h <= APA_MAX_SIDE && w <= APA_MAX_SIDE && (int64_t)h * w <= APA_MAX_CELLS,
               "1 <= h, w <= CSTS_AUDIO_PIXEL_MAX_SIDE and h * w <= CSTS_AUDIO_PIXEL_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(nmaps_per_frame >= 1 && F >= 1 && S >= 1 && S <= 65536, "nmaps_per_frame >= 1, F >= 1, 1 <= S <= 65536");
  CSTS_REQUIRE(F < ((int64_t)1 << 31) && F * nmaps_per_frame < ((int64_t)1 << 31), "F * nmaps_per_frame must stay below 2^31");
  hipLaunchKernelGGL(apa_rescale_kernel, dim3((unsigned)(F * nmaps_per_frame)), dim3(256), 0, stream, mixed, valid,
                     nmaps_per_frame, h, w, S, maps, range);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_attention_track(const float* column, const int* order, const int* offsets, int64_t F, int Wn, int heads, int Tp,
                                    int h, int w, int T, int S, float* mixed, float* maps, float* range, int* count,
                                    hipStream_t stream) {
  CSTS_REQUIRE(column && order && offsets && mixed && maps && range && count, "bad args (no pointer may be NULL)");
  CSTS_REQUIRE(Wn >= 1 && heads >= 1 && F >= 1, "Wn >= 1, heads >= 1, F >= 1");
  CSTS_REQUIRE(Tp >= 1 && h >= 1 && w >= 1 && h <= APA_MAX_SIDE && w <= APA_MAX_SIDE && (int64_t)h * w <= APA_MAX_CELLS,
               "1 <= h, w <= CSTS_AUDIO_PIXEL_MAX_SIDE and h * w <= CSTS_AUDIO_PIXEL_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(T >= 1 && T <= 65536 && Tp <= 65536 && S >= 1 && S <= 65536, "1 <= T, T', S <= 65536");
  CSTS_REQUIRE((int64_t)Wn * T < ((int64_t)1 << 31) && F < ((int64_t)1 << 31) && F * (heads + 1) < ((int64_t)1 << 31),
               "Wn * T and F * (heads + 1) must stay below 2^31");
  hipLaunchKernelGGL(apt_accumulate_kernel, dim3((unsigned)(F * (heads + 1))), dim3(256), 0, stream, column, order, offsets, Wn,
                     heads, Tp, h * w, T, mixed, count);
  CSTS_LAUNCH_CHECK();
  return csts_attention_rescale(mixed, count, heads + 1, F, h, w, S, maps, range, stream);
}

extern "C" int csts_live_attention_add(const float* column, const int64_t* frames_idx, int Wn, int heads, int Tp, int h, int w, int T,
                                       float* sum, int* count, int64_t* frame, int Ra, hipStream_t stream) {
  CSTS_REQUIRE(column && frames_idx && sum && count && frame, "bad args (no pointer may be NULL)");
  CSTS_REQUIRE(column != sum, "column must not be the ring's sum");
  CSTS_REQUIRE(Wn >= 1 && heads >= 1 && heads <= 65534 && Ra >= 1 && Ra <= 65535, "Wn >= 1, 1 <= heads <= 65534, 1 <= Ra <= 65535");
  CSTS_REQUIRE(Tp >= 1 && h >= 1 && w >= 1 && h <= APA_MAX_SIDE && w <= APA_MAX_SIDE && (int64_t)h * w <= APA_MAX_CELLS,
               "1 <= h, w <= CSTS_AUDIO_PIXEL_MAX_SIDE and h * w <= CSTS_AUDIO_PIXEL_MAX_HW");
  CSTS_REQUIRE(T >= 1 && T <= 65536 && Tp <= 65536 && (int64_t)Wn * T <= 65535, "1 <= T, T' <= 65536, Wn * T <= 65535");
  CSTS_REQUIRE((int64_t)(heads + 1) * h * w < ((int64_t)1 << 31), "(heads + 1) * h * w must stay below 2^31");
  const int HW = h * w;
  const bool vec = HW % 4 == 0 && aligned16(column) && aligned16(sum);
  if (vec) hipLaunchKernelGGL(live_attention_add_kernel<true>, dim3((unsigned)Ra), dim3(256), 0, stream, column, frames_idx, Wn * T,
                              heads, Tp, HW, T, sum, count, frame, Ra);
  else hipLaunchKernelGGL(live_attention_add_kernel<false>, dim3((unsigned)Ra), dim3(256), 0, stream, column, frames_idx, Wn * T,
                          heads, Tp, HW, T, sum, count, frame, Ra);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_live_attention_rows(const float* sum, const int* count, const int64_t* frame, int Ra, int64_t f0, int K, int heads,
                                        int h, int w, int S, int max_age, float* mixed, float* maps, float* range,
                                        int64_t* out_frame, int* out_count, hipStream_t stream) {
  CSTS_REQUIRE(sum && count && frame, "bad args (the ring may not be NULL)");
  CSTS_REQUIRE((maps == nullptr) == (range == nullptr), "maps and range come together: both or neither");
  CSTS_REQUIRE(mixed != sum && maps != sum, "no output may be the ring");
  CSTS_REQUIRE(Ra >= 1 && Ra <= 65535 && heads >= 1 && heads <= 65534 && K >= 1 && K <= 65535, "1 <= Ra, K <= 65535, 1 <= heads <= 65534");
  CSTS_REQUIRE(h >= 1 && w >= 1 && h <= APA_MAX_SIDE && w <= APA_MAX_SIDE && (int64_t)h * w <= APA_MAX_CELLS,
               "1 <= h, w <= CSTS_AUDIO_PIXEL_MAX_SIDE and h * w <= CSTS_AUDIO_PIXEL_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(S >= 1 && S <= 65536 && f0 >= 0 && max_age >= 0 && max_age <= 65535, "1 <= S <= 65536, f0 >= 0, 0 <= max_age <= 65535");
  if (!mixed && !maps && !out_frame && !out_count) return 0;
  const bool vec = (h * w) % 4 == 0 && aligned16(sum) && (!mixed || aligned16(mixed));
  const dim3 grid((unsigned)K, (unsigned)(heads + 1));
  if (vec) hipLaunchKernelGGL(live_attention_rows_kernel<true>, grid, dim3(256), 0, stream, sum, count, frame, Ra, f0, h, w, S, max_age,
                              mixed, maps, range, out_frame, out_count);
  else hipLaunchKernelGGL(live_attention_rows_kernel<false>, grid, dim3(256), 0, stream, sum, count, frame, Ra, f0, h, w, S, max_age,
                          mixed, maps, range, out_frame, out_count);
  CSTS_LAUNCH_CHECK();
  return 0;
}
