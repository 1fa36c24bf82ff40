// LayerNorm forward / backward (K2 of SURVEY.md 2.3) and the shared partial-sum reducer.
// Reference: block norms nn.LayerNorm(C, eps=1e-6) (attention.py:192,214) and the per-head
// nn.LayerNorm(hd, eps=1e-5) applied to pooled q/k/v (attention.py:108,112,116) -- same kernel, rows = B*N*h.
// A group of GL lanes per row, the row kept in registers (C <= 768), two-pass statistics in fp32.
// HBM-bound: algorithmic bytes = rows*C*(in + out) (+ 8 B/row of statistics).
#include "common.h"

#include <utility>

namespace {

constexpr int MAXV = 12;  // C <= 768
constexpr int LN_BWD_WAVES = 8;  // 512-thread blocks: few, fat partial rows for the second-stage reduction

// compile-time dtypes: no branch sits between a load and the next one, so a lane group keeps R rows x NCH loads in flight
template <bool F32> __device__ __forceinline__ float ldt(const void* p, int64_t i) {
  if constexpr (F32) return reinterpret_cast<const float*>(p)[i];
  else return h16_lo((unsigned)reinterpret_cast<const unsigned short*>(p)[i]);
}
template <bool F32> __device__ __forceinline__ void stt(void* p, int64_t i, float v) {
  if constexpr (F32) reinterpret_cast<float*>(p)[i] = v;
  else reinterpret_cast<bf16*>(p)[i] = (bf16)v;
}
template <bool F32> __device__ __forceinline__ void ld8t(const void* p, int64_t i, float (&o)[8]) {
  if constexpr (F32) {
    const float4* q = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i);
    const float4 a = q[0], b = q[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
    const uint4 r = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(p) + i);
    o[0] = h16_lo(r.x); o[1] = h16_hi(r.x);
    o[2] = h16_lo(r.y); o[3] = h16_hi(r.y);
    o[4] = h16_lo(r.z); o[5] = h16_hi(r.z);
    o[6] = h16_lo(r.w); o[7] = h16_hi(r.w);
  }
}
template <bool F32> __device__ __forceinline__ void st8t(void* p, int64_t i, const float (&o)[8]) {
  if constexpr (F32) {
    float4* q = reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + i);
    q[0] = make_float4(o[0], o[1], o[2], o[3]);
    q[1] = make_float4(o[4], o[5], o[6], o[7]);
  } else {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16)o[j];
    *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16*>(p) + i) = v;
  }
}
// a chunk of W consecutive channels: one element, or 16 bytes (32 of fp32) at once
template <int W, bool F32> __device__ __forceinline__ void ldw(const void* p, int64_t i, float (&o)[W]) {
  if constexpr (W == 8) ld8t<F32>(p, i, o);
  else o[0] = ldt<F32>(p, i);
}
template <int W, bool F32> __device__ __forceinline__ void stw(void* p, int64_t i, const float (&o)[W]) {
  if constexpr (W == 8) st8t<F32>(p, i, o);
  else stt<F32>(p, i, o[0]);
}
template <int GL> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = GL / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroups are dealt round-robin over the 8 XCDs; like the GEMMs (gemm.hip), give XCD x the CONTIGUOUS row range x of 8: a
// consumer then finds what the producer's workgroups of the same XCD have just written in that XCD's L2 instead of the memory-side
// cache (tools/launch_floor.hip, profiles/r4_stream_policy.txt part 5: 6 MB handed over in 1.65 us instead of 4.8 us; it holds up to
// ~1 MB per XCD).  Bijective for any grid size.  -DCSTS_LN_NO_XCD_MAP: the plain order (A/B builds).
__device__ __forceinline__ int64_t xcd_block(int64_t bid, int64_t nwg) {
#ifdef CSTS_LN_NO_XCD_MAP
  return bid;
#else
  const int64_t q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// One kernel body per direction.  A group of GL lanes owns a row and every lane NCH chunks of W consecutive channels, chunk i
// of lane `sub` starting at channel (sub + GL i) W; statistics by shuffles inside the group, 64 / GL rows per wave and R rows
// in flight per group.  Two roles:
//   W = 8  C % 8 == 0 and every operand 16-byte aligned (all the model produces: C in {96, 192, 384, 768}): 16-byte loads and
//          stores, GL = 16 / 32 / 64 by C, XCD-contiguous row ranges.
//   W = 1  everything else: one channel per lane and chunk, a whole wave per row (GL = 64, channel lane + 64 i), plain
//          workgroup order.  In the backward kernel the block -> rows map decides what each partial row of the workspace holds,
//          and so the bits of dgamma / dbeta: the XCD map must stay out of this role.
// ---------------------------------------------------------------------------------------------------------------
// A lane's chunks.  on(i): chunk i lies inside the row; at(i): its first channel, clamped into the row so that every lane may
// load; st(i): the same for a store, which happens under on(i) only, where the clamp changes nothing.  W = 8 forms on and at once
// per lane.  W = 1 forms all three anew from the compile-time i at each use and keeps nothing: there a lane has up to 12 chunks,
// and a live predicate and clamped offset per chunk cost the 12-chunk forms a wave per SIMD (forward) or spill (backward).
template <int W, int GL, int NCH> struct Lane {
  int sub, C;
  int c0[W == 8 ? NCH : 1];
  bool act[W == 8 ? NCH : 1];
  // called once per chunk before anything else, interleaved with the parameter loads (the order the W = 8 schedule was tuned in)
  __device__ __forceinline__ void form(int i) {
    if constexpr (W == 8) {
      const int c = (sub + GL * i) * 8;
      act[i] = c < C;
      c0[i] = min(c, C - 8);
    }
  }
  __device__ __forceinline__ bool on(int i) const {
    if constexpr (W == 8) return act[i];
    else return sub + GL * i < C;
  }
  __device__ __forceinline__ int st(int i) const {
    if constexpr (W == 8) return c0[i];
    else return sub + GL * i;
  }
  __device__ __forceinline__ int at(int i) const {
    if constexpr (W == 8) return c0[i];
    else return min(sub + GL * i, C - 1);
  }
  // gamma / beta of chunk i; the one-channel role reads nothing for a chunk outside the row
  __device__ __forceinline__ void param(const float* p, int i, float (&o)[W]) const {
    if constexpr (W == 8) ld8t<true>(p, at(i), o);
    else o[0] = on(i) ? p[sub + GL * i] : 0.f;
  }
};

// optional input of the forward kernel: x + addend is what gets normalised, and the sum is written to `sum` (dtype of x):
// the decoder's `feat + en_feat` skip (custom_multimodal_builder.py:467-479) folded into the next block's norm1.  What is normalised
// is the sum AS STORED (a 16-bit sum is rounded first): mean / rstd are those of `sum`, the x the backward reads with them
struct FwdAdd {
  const void* addend = nullptr;
  void* sum = nullptr;
};
template <int W, int GL, int NCH, int R, bool XF32, bool YF32>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, void* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int64_t rows,
                                                     int C, float eps, FwdAdd fa) {
  const int64_t bid = W == 8 ? xcd_block(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int64_t grp = (bid * 256 + threadIdx.x) / GL, ngrp = (int64_t)gridDim.x * 256 / GL;
  Lane<W, GL, NCH> ln{(int)(threadIdx.x % GL), C};
  float gm[NCH][W], bt[NCH][W];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    ln.form(i);
    ln.param(gamma, i, gm[i]);
    ln.param(beta, i, bt[i]);
  }
  const float invC = 1.f / C;
  for (int64_t row0 = grp * R; row0 < rows; row0 += ngrp * R) {
    float v[R][NCH][W];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = min(row0 + r, rows - 1);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        ldw<W, XF32>(x, row * C + ln.at(i), v[r][i]);
        if (fa.addend) {                                         // wave-uniform
          float a2[W];
          ldw<W, XF32>(fa.addend, row * C + ln.at(i), a2);
#pragma unroll
          for (int j = 0; j < W; ++j) {
            v[r][i][j] += a2[j];
            if constexpr (!XF32) v[r][i][j] = (float)(bf16)v[r][i][j];   // normalise the sum as stored: the x the backward reads with this mean / rstd
          }
          if (ln.on(i) && row0 + r < rows) stw<W, XF32>(fa.sum, row * C + ln.st(i), v[r][i]);
        }
      }
    }
    // Mean, rstd and the stores of a row.  W = 8 takes its rows one after the other; W = 1 takes its R rows through one phase after
    // the other (PH = 3 passes: the shuffles of up to four rows in flight together) -- the order each role was scheduled and timed
    // in.  The arithmetic of a row is the same either way.
    constexpr int PH = W == 8 ? 1 : 3;
    float mu[R], rs[R];
#pragma unroll
    for (int ph = 0; ph < PH; ++ph)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (PH == 1 || ph == 0) {
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < NCH; ++i)
            if (ln.on(i)) {
#pragma unroll
              for (int j = 0; j < W; ++j) s += v[r][i][j];
            }
          mu[r] = group_sum<GL>(s) * invC;
        }
        if (PH == 1 || ph == 1) {
          float q = 0.f;
#pragma unroll
          for (int i = 0; i < NCH; ++i)
            if (ln.on(i)) {
#pragma unroll
              for (int j = 0; j < W; ++j) { const float d = v[r][i][j] - mu[r]; q += d * d; }
            }
          rs[r] = rsqrtf(group_sum<GL>(q) * invC + eps);
        }
        const int64_t row = row0 + r;
        if ((PH == 1 || ph == 2) && row < rows) {
#pragma unroll
          for (int i = 0; i < NCH; ++i)
            if (ln.on(i)) {
              float o[W];
#pragma unroll
              for (int j = 0; j < W; ++j) o[j] = (v[r][i][j] - mu[r]) * rs[r] * gm[i][j] + bt[i][j];
              stw<W, YF32>(y, row * C + ln.st(i), o);
            }
          if (ln.sub == 0) {
            if (mean) mean[row] = mu[r];
            if (rstd) rstd[row] = rs[r];
          }
        }
      }
  }
}

// optional extras of the backward kernel: a bf16 copy of dx (+ per-sample scale applied to the copy only: row r uses
// scale[r / rps]) and a second incoming gradient (LayerNorm output with two consumers)
struct Copy16 {
  bf16* p = nullptr;
  const float* scale = nullptr;
  int64_t rps = 1;
  const void* dy2 = nullptr;     // a second incoming gradient of the same shape / dtype as dy: the kernel reads dy + dy2
};
#ifndef CSTS_LN_BWD_R
#define CSTS_LN_BWD_R 1            // rows per lane group and pass of the W = 8 ln_bwd_kernel at C <= 512.  Round 5: 1 instead of 2 (-0.1 ms per step, profiles/r5_stencil_ab.txt)
#endif
#ifndef CSTS_LN_BWD_MINW
#define CSTS_LN_BWD_MINW 1         // minimum waves per SIMD ln_bwd_kernel is compiled for (A/B builds: 6 with R = 1)
#endif
// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma
// per-group partial dgamma/dbeta are summed through LDS and written to ws[block][2*C]
template <int W, int GL, int NCH, int R, bool DYF32, bool XF32>
__global__ __launch_bounds__(512, CSTS_LN_BWD_MINW) void ln_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                         const float* __restrict__ gamma, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, void* __restrict__ dx,
                                                         const void* __restrict__ addend, float* __restrict__ ws, int64_t rows,
                                                         int C, const float* __restrict__ gamma1, Copy16 dx16) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [512 / GL groups][2*C]
  // blockIdx.y = segment: a second tensor of the same shape stacked behind the first (rows each), with its own gamma and
  // its own partial rows (the k and v LayerNorms of one attention in one launch)
  const int64_t ro = (int64_t)blockIdx.y * rows;
  if (blockIdx.y == 1) gamma = gamma1;
  ws += (int64_t)blockIdx.y * gridDim.x * 2 * C;
  const int gib = threadIdx.x / GL;                            // group in block
  constexpr int GPB = 512 / GL;
  const int64_t bid = W == 8 ? xcd_block(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int64_t grp = bid * GPB + gib, ngrp = (int64_t)gridDim.x * GPB;
  Lane<W, GL, NCH> ln{(int)(threadIdx.x % GL), C};
  float gm[NCH][W], dg[NCH][W], db[NCH][W];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    ln.form(i);
    ln.param(gamma, i, gm[i]);
#pragma unroll
    for (int j = 0; j < W; ++j) { dg[i][j] = 0.f; db[i][j] = 0.f; }
  }
  const float invC = 1.f / C;
  for (int64_t row0 = grp * R; row0 < rows; row0 += ngrp * R) {
    float d[R][NCH][W], xv[R][NCH][W], ad[R][NCH][W], mu[R], rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = ro + min(row0 + r, rows - 1);
      mu[r] = mean[row];
      rs[r] = rstd[row];
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        ldw<W, DYF32>(dy, row * C + ln.at(i), d[r][i]);
        if (dx16.dy2) {                                          // wave-uniform test
          float d2[W];
          ldw<W, DYF32>(dx16.dy2, row * C + ln.at(i), d2);
#pragma unroll
          for (int j = 0; j < W; ++j) d[r][i][j] += d2[j];
        }
        ldw<W, XF32>(x, row * C + ln.at(i), xv[r][i]);
        if (addend) ldw<W, XF32>(addend, row * C + ln.at(i), ad[r][i]);   // residual-branch gradient folded into dx (wave-uniform test)
        else {
#pragma unroll
          for (int j = 0; j < W; ++j) ad[r][i][j] = 0.f;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool live = row0 + r < rows;
      float s1 = 0.f, s2 = 0.f;
      float xh[NCH][W], g[NCH][W];
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const bool ok = live && ln.on(i);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const float dd = ok ? d[r][i][j] : 0.f;
          xh[i][j] = ok ? (xv[r][i][j] - mu[r]) * rs[r] : 0.f;
          g[i][j] = dd * gm[i][j];
          dg[i][j] += dd * xh[i][j];
          db[i][j] += dd;
          s1 += g[i][j];
          s2 += g[i][j] * xh[i][j];
        }
      }
      s1 = group_sum<GL>(s1) * invC;
      s2 = group_sum<GL>(s2) * invC;
      if (live) {
        const int64_t row = ro + row0 + r;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
          if (ln.on(i)) {
            float o[W];
#pragma unroll
            for (int j = 0; j < W; ++j) o[j] = rs[r] * (g[i][j] - s1 - xh[i][j] * s2) + ad[r][i][j];
            stw<W, XF32>(dx, row * C + ln.st(i), o);
            // the copy the next GEMMs read (they round to bf16 anyway), times the per-sample drop-path scale of the
            // branch that consumes it when the caller knows it (saves that branch a scale_rows pass over dx)
            if (dx16.p) {
              if (dx16.scale) {
                const float sc = dx16.scale[(row0 + r) / dx16.rps];
#pragma unroll
                for (int j = 0; j < W; ++j) o[j] *= sc;
              }
              stw<W, false>(dx16.p, row * C + ln.st(i), o);
            }
          }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (ln.on(i)) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        red[gib * 2 * C + ln.st(i) + j] = dg[i][j];
        red[gib * 2 * C + C + ln.st(i) + j] = db[i][j];
      }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
    float t = 0.f;
#pragma unroll(W == 8 ? 4 : GPB)   // each role's own unrolling; the order of the sum is ascending k either way
    for (int k = 0; k < GPB; ++k) t += red[k * 2 * C + i];
    ws[(int64_t)blockIdx.x * 2 * C + i] = t;
  }
}

// out[j] = sum_i ws[i][j]   (deterministic second stage of every cross-block reduction in the library)
// block = 32 columns x RL row-lanes; fixed summation order -> bitwise reproducible
template <int RL>
__global__ void reduce_rows_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t nrows, int64_t ncols,
                                   float scale) {
  __shared__ float red[RL][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t j = (int64_t)blockIdx.x * 32 + tx;
  float s = 0.f;
  if (j < ncols) {
    int64_t i = ty;
    for (; i + 3 * RL < nrows; i += 4 * RL) {
      const float a = ws[i * ncols + j], b = ws[(i + RL) * ncols + j], c = ws[(i + 2 * RL) * ncols + j],
                  d = ws[(i + 3 * RL) * ncols + j];
      s += a; s += b; s += c; s += d;
    }
    for (; i < nrows; i += RL) s += ws[i * ncols + j];
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && j < ncols) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < RL; ++r) t += red[r][tx];
    out[j] = t * scale;
  }
}

// the same second stage for MANY independent reductions in one launch: blockIdx.y picks the descriptor
__global__ __launch_bounds__(1024) void reduce_rows_batched_kernel(const csts_reduce_desc* __restrict__ descs) {
  __shared__ float red[32][33];
  const csts_reduce_desc d = descs[blockIdx.y];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t j = (int64_t)blockIdx.x * 32 + tx;
  if ((int64_t)blockIdx.x * 32 >= d.ncols) return;     // block-uniform
  float s = 0.f;
  if (j < d.ncols) {
    int64_t i = ty;
    for (; i + 3 * 32 < d.nrows; i += 4 * 32) {
      const float a = d.ws[i * d.ncols + j], b = d.ws[(i + 32) * d.ncols + j], c = d.ws[(i + 64) * d.ncols + j],
                  e = d.ws[(i + 96) * d.ncols + j];
      s += a; s += b; s += c; s += e;
    }
    for (; i < d.nrows; i += 32) s += d.ws[i * d.ncols + j];
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && j < d.ncols) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) t += red[r][tx];
    d.out[j] = t * d.scale;
  }
}

// wide, shallow reductions (split-K partial slabs of the grouped weight gradients: a handful of rows, up to millions of
// columns): one thread per 4 consecutive columns, rows summed in order -> 16-byte loads, no idle row lanes
__global__ __launch_bounds__(256) void reduce_rows_wide_kernel(const csts_reduce_desc* __restrict__ descs) {
  const csts_reduce_desc d = descs[blockIdx.y];
  const int64_t nvec = d.ncols >> 2;           // host guarantees ncols % 4 == 0 and 16-byte aligned pointers
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* p = reinterpret_cast<const float4*>(d.ws) + v;
    int64_t i = 0;
    for (; i + 3 < d.nrows; i += 4) {
      const float4 a = p[i * nvec], b = p[(i + 1) * nvec], c = p[(i + 2) * nvec], e = p[(i + 3) * nvec];
      s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
      s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
      s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w;
      s.x += e.x; s.y += e.y; s.z += e.z; s.w += e.w;
    }
    for (; i < d.nrows; ++i) {
      const float4 a = p[i * nvec];
      s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
    }
    reinterpret_cast<float4*>(d.out)[v] = make_float4(s.x * d.scale, s.y * d.scale, s.z * d.scale, s.w * d.scale);
  }
}

}  // namespace

extern "C" int csts_reduce_rows_wide(const csts_reduce_desc* device_descs, int n, int64_t max_ncols, hipStream_t stream) {
  CSTS_REQUIRE(device_descs != nullptr && n > 0 && n < 65536 && max_ncols > 0, "bad args");
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv(max_ncols / 4, 256), 4096);
  hipLaunchKernelGGL(reduce_rows_wide_kernel, dim3(gx, (unsigned)n), dim3(256), 0, stream, device_descs);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_reduce_rows_batched(const csts_reduce_desc* device_descs, int n, int64_t max_ncols, hipStream_t stream) {
  CSTS_REQUIRE(device_descs != nullptr && n > 0 && n < 65536 && max_ncols > 0, "bad args");
  hipLaunchKernelGGL(reduce_rows_batched_kernel, dim3((unsigned)cdiv(max_ncols, 32), (unsigned)n), dim3(1024), 0, stream,
                     device_descs);
  CSTS_LAUNCH_CHECK();
  return 0;
}

int csts_reduce_rows_launch(const float* ws, float* out, int64_t nrows, int64_t ncols, float scale, hipStream_t s) {
  const dim3 grid((unsigned)cdiv(ncols, 32));
  if (nrows > 64) hipLaunchKernelGGL(reduce_rows_kernel<32>, grid, dim3(1024), 0, s, ws, out, nrows, ncols, scale);
  else if (nrows > 8) hipLaunchKernelGGL(reduce_rows_kernel<8>, grid, dim3(256), 0, s, ws, out, nrows, ncols, scale);
  else hipLaunchKernelGGL(reduce_rows_kernel<2>, grid, dim3(64), 0, s, ws, out, nrows, ncols, scale);
  return 0;
}

extern "C" int csts_reduce_rows(const float* ws, float* out, int64_t nrows, int64_t ncols, float scale,
                                hipStream_t stream) {
  CSTS_REQUIRE(ws && out && nrows > 0 && ncols > 0, "bad args");
  csts_reduce_rows_launch(ws, out, nrows, ncols, scale, stream);
  CSTS_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The LayerNorm launches.  Every instantiated form {W, GL, NCH, R} of a direction stands in LN_FORMS once; ln_form() is the
// one place that decides which of them serves a call, and grids, LDS and workspace sizes follow from the form it names.
// ---------------------------------------------------------------------------------------------------------------
#ifndef CSTS_LN_FWD_R
#define CSTS_LN_FWD_R 2            // rows per lane group and pass of the W = 8 ln_fwd_kernel at C <= 512 (A/B build: 1)
#endif
#ifndef CSTS_LN_BWD_CAP
#define CSTS_LN_BWD_CAP 512        // workgroups of a LayerNorm-backward launch (two 512-thread workgroups per CU; A/B builds: 768 with CSTS_LN_BWD_MINW=6)
#endif
struct LnForm { int W, GL, NCH, R; };
template <bool BWD> static constexpr LnForm LN_FORMS[8] = {
    {8, 16, 1, BWD ? CSTS_LN_BWD_R : CSTS_LN_FWD_R}, {8, 32, 1, BWD ? CSTS_LN_BWD_R : CSTS_LN_FWD_R},   // C <= 128, <= 256
    {8, 64, 1, BWD ? CSTS_LN_BWD_R : CSTS_LN_FWD_R}, {8, 64, 2, BWD ? 1 : 2},                           // C <= 512, <= 768
    {1, 64, 2, 4}, {1, 64, 3, 4}, {1, 64, 6, 2}, {1, 64, 12, 1}};                                       // C <= 128, <= 192, <= 384, <= 768
static size_t ln_bwd_lds(const LnForm& f, int C) { return (size_t)(512 / f.GL) * 2 * C * sizeof(float); }   // [groups][2*C] partials
// The index into LN_FORMS of the form that serves 0 < C <= 768.  `aligned`: every operand is 16-byte aligned (and whatever else
// the entry asks of its shapes); 8 channels per lane need that, C % 8 == 0 and, backward, the partials inside 64 KiB of LDS.
static int ln_form(bool bwd, int C, bool aligned) {
  const int vec = C <= 128 ? 0 : (C <= 256 ? 1 : (C <= 512 ? 2 : 3));
  if (aligned && C % 8 == 0 && !(bwd && ln_bwd_lds(LN_FORMS<true>[vec], C) > 65536)) return vec;
  return 4 + (C <= 128 ? 0 : (C <= 192 ? 1 : (C <= 384 ? 2 : 3)));
}
static bool all_aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if (q != nullptr && !aligned16(q)) return false;
  return true;
}
// The grid of a backward launch, and with it the partial rows of the workspace, is that of the one-channel form whichever
// form runs: the workspace is sized before the operands are known.
static int64_t ln_bwd_blocks(int64_t rows, int C) {
  return std::min<int64_t>(cdiv(rows, LN_BWD_WAVES * LN_FORMS<true>[ln_form(true, C, false)].R), CSTS_LN_BWD_CAP);
}
// k = 4 form + 2 (first dtype is fp32) + (second dtype is fp32) as a compile-time constant: the one dispatch of both directions
template <class F, int... K> static void ln_pick(int k, F&& launch, std::integer_sequence<int, K...>) {
  ((k == K ? launch(std::integral_constant<int, K>{}) : void()), ...);
}

extern "C" int csts_layernorm_fwd(const void* x, int x_dt, const float* gamma, const float* beta, void* y, int y_dt,
                                  float* mean, float* rstd, int64_t rows, int C, float eps, hipStream_t stream) {
  return csts_layernorm_fwd_add(x, nullptr, nullptr, x_dt, gamma, beta, y, y_dt, mean, rstd, rows, C, eps, stream);
}

extern "C" int csts_layernorm_fwd_add(const void* x, const void* addend, void* sum_out, int x_dt, const float* gamma,
                                      const float* beta, void* y, int y_dt, float* mean, float* rstd, int64_t rows, int C,
                                      float eps, hipStream_t stream) {
  CSTS_REQUIRE(x && gamma && beta && y, "null pointer");
  CSTS_REQUIRE((addend == nullptr) == (sum_out == nullptr), "addend and sum_out: both or neither");
  CSTS_REQUIRE(rows > 0 && C > 0 && C <= 64 * MAXV, "C must be in (0, 768]");
  FwdAdd fa;
  fa.addend = addend; fa.sum = sum_out;
  const int form = ln_form(false, C, all_aligned16({x, y, gamma, beta, addend, sum_out}));
  const LnForm& f = LN_FORMS<false>[form];
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(rows * f.GL, 256 * f.R), 4096));
  ln_pick(4 * form + 2 * (x_dt == CSTS_F32) + (y_dt == CSTS_F32), [&](auto k) {
    constexpr LnForm F = LN_FORMS<false>[decltype(k)::value / 4];
    hipLaunchKernelGGL((ln_fwd_kernel<F.W, F.GL, F.NCH, F.R, (decltype(k)::value & 2) != 0, (decltype(k)::value & 1) != 0>), grid,
                       dim3(256), 0, stream, x, gamma, beta, y, mean, rstd, rows, C, eps, fa);
  }, std::make_integer_sequence<int, 32>{});
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t csts_layernorm_bwd_workspace(int64_t rows, int C) {
  return (size_t)ln_bwd_blocks(rows, C) * 2 * C * sizeof(float);
}

// One backward launch over `segs` stacked tensors (gamma[s]; ws holds ln_bwd_blocks partial rows of each) and, unless dgb[0] is
// NULL (the deferred second stage), the reduction of each segment's partial rows into dgb[s] = dgamma | dbeta.
static void ln_bwd_launch(int segs, bool aligned, const void* dy, int dy_dt, const void* x, int x_dt, const float* const (&gamma)[2],
                          const float* mean, const float* rstd, void* dx, const void* addend, float* const (&dgb)[2], float* ws,
                          int64_t rows, int C, Copy16 c16, hipStream_t stream) {
  const int form = ln_form(true, C, aligned);
  const int64_t nb = ln_bwd_blocks(rows, C);
  const dim3 grid((unsigned)nb, (unsigned)segs);
  const size_t sh = ln_bwd_lds(LN_FORMS<true>[form], C);
  ln_pick(4 * form + 2 * (dy_dt == CSTS_F32) + (x_dt == CSTS_F32), [&](auto k) {
    constexpr LnForm F = LN_FORMS<true>[decltype(k)::value / 4];
    hipLaunchKernelGGL((ln_bwd_kernel<F.W, F.GL, F.NCH, F.R, (decltype(k)::value & 2) != 0, (decltype(k)::value & 1) != 0>), grid,
                       dim3(512), sh, stream, dy, x, gamma[0], mean, rstd, dx, addend, ws, rows, C, gamma[1], c16);
  }, std::make_integer_sequence<int, 32>{});
  for (int s = 0; s < segs && dgb[0] != nullptr; ++s) csts_reduce_rows_launch(ws + s * nb * 2 * C, dgb[s], nb, 2 * C, 1.f, stream);
}

extern "C" int csts_layernorm_bwd(const void* dy, int dy_dt, const void* x, int x_dt, const float* gamma,
                                  const float* mean, const float* rstd, void* dx, int dx_dt, const void* addend,
                                  void* dx_bf16, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                                  int64_t rows, int C, hipStream_t stream) {
  return csts_layernorm_bwd_ex(dy, nullptr, dy_dt, x, x_dt, gamma, mean, rstd, dx, dx_dt, addend, dx_bf16, nullptr, 1, dgamma,
                               dbeta, workspace, ws_bytes, rows, C, stream);
}

extern "C" int csts_layernorm_bwd_ex(const void* dy, const void* dy2, int dy_dt, const void* x, int x_dt, const float* gamma,
                                     const float* mean, const float* rstd, void* dx, int dx_dt, const void* addend,
                                     void* dx_bf16, const float* copy_row_scale, int64_t rows_per_scale,
                                     float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, int64_t rows,
                                     int C, hipStream_t stream) {
  CSTS_REQUIRE(dy && x && gamma && mean && rstd && dx && workspace, "null pointer");
  CSTS_REQUIRE(copy_row_scale == nullptr || (dx_bf16 != nullptr && rows_per_scale > 0), "copy scale needs the bf16 copy and rows_per_scale > 0");
  Copy16 c16;
  c16.p = reinterpret_cast<bf16*>(dx_bf16); c16.scale = copy_row_scale; c16.rps = rows_per_scale > 0 ? rows_per_scale : 1;
  c16.dy2 = dy2;
  CSTS_REQUIRE(rows > 0 && C > 0 && C <= 64 * MAXV, "C must be in (0, 768]");
  CSTS_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "dgamma and dbeta: both or neither (neither = deferred second stage)");
  CSTS_REQUIRE(dgamma == nullptr || dbeta == dgamma + C, "dgamma/dbeta must be one contiguous [2*C] buffer");
  CSTS_REQUIRE(dx_dt == x_dt, "dx must have the dtype of x");
  const int64_t nb = ln_bwd_blocks(rows, C);
  CSTS_REQUIRE(ws_bytes >= (size_t)nb * 2 * C * sizeof(float), "workspace too small");
  ln_bwd_launch(1, all_aligned16({dy, dy2, x, dx, addend, dx_bf16, gamma}), dy, dy_dt, x, x_dt, {gamma, nullptr}, mean, rstd, dx,
                addend, {dgamma, nullptr}, reinterpret_cast<float*>(workspace), rows, C, c16, stream);
  CSTS_LAUNCH_CHECK();
  return 0;
}

/* two stacked tensors (rows each) with separate gammas, one launch; ws = 2 x csts_layernorm_bwd_workspace(rows, C) */
extern "C" int csts_layernorm_bwd2(const void* dy, int dy_dt, const void* x, int x_dt, const float* gamma0,
                                   const float* gamma1, const float* mean, const float* rstd, void* dx, int dx_dt,
                                   float* dgb0, float* dgb1, void* workspace, size_t ws_bytes, int64_t rows, int C,
                                   hipStream_t stream) {
  CSTS_REQUIRE(dy && x && gamma0 && gamma1 && mean && rstd && dx && workspace, "null pointer");
  CSTS_REQUIRE(rows > 0 && C > 0 && C <= 64 * MAXV, "C must be in (0, 768]");
  CSTS_REQUIRE(dx_dt == x_dt, "dx must have the dtype of x");
  CSTS_REQUIRE((dgb0 == nullptr) == (dgb1 == nullptr), "dgb0/dgb1: both or neither (neither = deferred second stage)");
  const int64_t nb = ln_bwd_blocks(rows, C);
  CSTS_REQUIRE(ws_bytes >= (size_t)2 * nb * 2 * C * sizeof(float), "workspace too small");
  // (rows * C) % 8 == 0: the second segment starts rows * C elements in and must be 16-byte aligned as well
  ln_bwd_launch(2, all_aligned16({dy, x, dx, gamma0, gamma1}) && ((rows * C) % 8 == 0), dy, dy_dt, x, x_dt, {gamma0, gamma1}, mean,
                rstd, dx, nullptr, {dgb0, dgb1}, reinterpret_cast<float*>(workspace), rows, C, Copy16{}, stream);
  CSTS_LAUNCH_CHECK();
  return 0;
}
