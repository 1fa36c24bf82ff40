// Element dropout (nn.Dropout(MVIT.DROPOUT_RATE) of the reference: custom_multimodal_builder.py:375-377 pos_drop,
// attention.py:159-161,390 / av_attention.py:148,353 proj_drop, common.py:26-34 Mlp.drop).
//
// The keep/drop decision of element e of a site is a pure function of (key, site, e, thr) -- include/csts_hip.h documents it:
// Philox4x32-10 with key (lo32(key), hi32(key)) on the counter (lo32(e >> 2), hi32(e >> 2), site, 0), word e & 3 of the block,
// dropped iff word < thr.  Forward, backward, the mask export and the host restatement all evaluate that one function, so they
// agree bit for bit whatever the grid.  The key is read from device memory: no host sync, graph-capturable (a replay reads
// whatever the captured key draw left in the buffer).
//
// Memory-bound elementwise passes: 8 elements per lane and iteration = two Philox blocks, 16-byte (bf16x8 / 2 x float4) loads
// and stores; the last partial group goes element by element.
#include "common.h"
#include "philox.h"

namespace {

using csts_philox::philox4x32_10;

// the four words of Philox block `blk` (= element index >> 2) of a site
__host__ __device__ __forceinline__ void dropout_block(uint32_t k0, uint32_t k1, uint32_t site, uint64_t blk, uint32_t w[4]) {
  w[0] = (uint32_t)blk; w[1] = (uint32_t)(blk >> 32); w[2] = site; w[3] = 0u;
  philox4x32_10(w, k0, k1);
}

__device__ __forceinline__ void load_key(const uint64_t* key, uint32_t& k0, uint32_t& k1) {
  const uint64_t k = *key;
  k0 = (uint32_t)k;
  k1 = (uint32_t)(k >> 32);
}

// y[e] = residual[e] + x[e] * (keep(e) ? scale : 0) * row_scale[(e / cols) / rows_per_scale]; residual / row_scale optional.
// x, y may alias (in place).  Pointers 16-byte aligned (the host entries check).
__global__ __launch_bounds__(256) void dropout_kernel(const void* x, int x_dt, const void* __restrict__ res, int r_dt,
                                                      const float* __restrict__ rs, int64_t rps, void* y, int y_dt,
                                                      const uint64_t* __restrict__ key, uint32_t site, uint32_t thr, float scale,
                                                      int64_t n, int64_t cols) {
  uint32_t k0, k1;
  load_key(key, k0, k1);
  const int64_t ngroups = (n + 7) / 8;
  const bool row_uniform = (cols & 7) == 0;        // the 8 elements of a group share one row
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = g * 8;
    uint32_t w[8];
    dropout_block(k0, k1, site, (uint64_t)e0 >> 2, w);
    dropout_block(k0, k1, site, ((uint64_t)e0 >> 2) + 1, w + 4);
    float m[8];
    float rsv = 1.f;
    if (rs && row_uniform) rsv = rs[(e0 / cols) / rps];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s = w[j] < thr ? 0.f : scale;
      if (rs && !row_uniform) s *= rs[((e0 + j) / cols) / rps];
      m[j] = s * rsv;
    }
    if (e0 + 8 <= n) {
      float v[8], r[8];
      ld8_as_f32(x, x_dt, e0, v);
      if (res) ld8_as_f32(res, r_dt, e0, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (res ? r[j] : 0.f) + v[j] * m[j];
      st8_from_f32(y, y_dt, e0, v);
    } else {
      for (int j = 0; j < 8 && e0 + j < n; ++j) {
        const float v = ld_as_f32(x, x_dt, e0 + j) * m[j];
        st_from_f32(y, y_dt, e0 + j, (res ? ld_as_f32(res, r_dt, e0 + j) : 0.f) + v);
      }
    }
  }
}

// out[e] = 1 if element e is dropped, else 0
__global__ __launch_bounds__(256) void dropout_mask_kernel(const uint64_t* __restrict__ key, uint32_t site, uint32_t thr,
                                                           uint8_t* __restrict__ out, int64_t n) {
  uint32_t k0, k1;
  load_key(key, k0, k1);
  const int64_t ngroups = (n + 7) / 8;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = g * 8;
    uint32_t w[8];
    dropout_block(k0, k1, site, (uint64_t)e0 >> 2, w);
    dropout_block(k0, k1, site, ((uint64_t)e0 >> 2) + 1, w + 4);
    if (e0 + 8 <= n) {
      uint64_t packed = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) packed |= (uint64_t)(w[j] < thr ? 1u : 0u) << (8 * j);
      *reinterpret_cast<uint64_t*>(out + e0) = packed;
    } else {
      for (int j = 0; j < 8 && e0 + j < n; ++j) out[e0 + j] = w[j] < thr ? 1 : 0;
    }
  }
}

int dropout_grid(int64_t n) { return (int)std::min<int64_t>(cdiv(cdiv(n, 8), 256), 256 * 16); }

int dropout_launch(const void* x, int x_dt, const void* res, int r_dt, const float* rs, int64_t rps, void* y, int y_dt,
                   const uint64_t* key, uint32_t site, uint32_t thr, float scale, int64_t rows, int64_t cols, hipStream_t stream) {
  CSTS_REQUIRE(x && y && key && rows > 0 && cols > 0, "bad args");
  CSTS_REQUIRE((x_dt == CSTS_F32 || x_dt == CSTS_BF16) && (y_dt == CSTS_F32 || y_dt == CSTS_BF16) &&
               (!res || r_dt == CSTS_F32 || r_dt == CSTS_BF16), "bad dtype");
  CSTS_REQUIRE(!rs || (rps > 0 && rows % rps == 0), "rows must be a multiple of rows_per_scale");
  CSTS_REQUIRE(aligned16(x) && aligned16(y) && (!res || aligned16(res)), "tensors must be 16-byte aligned");
  const int64_t n = rows * cols;
  hipLaunchKernelGGL(dropout_kernel, dim3(dropout_grid(n)), dim3(256), 0, stream, x, x_dt, res, r_dt, rs, rps, y, y_dt, key,
                     site, thr, scale, n, cols);
  CSTS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int csts_dropout_fwd(const void* z, const void* residual, const float* row_scale, int64_t rows_per_scale, void* y,
                                int dt, const uint64_t* key, uint32_t site, uint32_t thr, float scale, int64_t rows, int64_t cols,
                                hipStream_t stream) {
  return dropout_launch(z, dt, residual, dt, row_scale, rows_per_scale, y, dt, key, site, thr, scale, rows, cols, stream);
}

extern "C" int csts_dropout_bwd(const void* dy, int dy_dt, const float* row_scale, int64_t rows_per_scale, void* out, int out_dt,
                                const uint64_t* key, uint32_t site, uint32_t thr, float scale, int64_t rows, int64_t cols,
                                hipStream_t stream) {
  CSTS_REQUIRE(dy != out || dy_dt == out_dt, "in place needs one dtype");
  return dropout_launch(dy, dy_dt, nullptr, 0, row_scale, rows_per_scale, out, out_dt, key, site, thr, scale, rows, cols, stream);
}

extern "C" int csts_dropout_mask(const uint64_t* key, uint32_t site, uint32_t thr, uint8_t* out, int64_t n, hipStream_t stream) {
  CSTS_REQUIRE(key && out && n > 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "bad args");
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(dropout_grid(n)), dim3(256), 0, stream, key, site, thr, out, n);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_dropout_mask_host(uint32_t key0, uint32_t key1, uint32_t site, uint32_t thr, uint64_t first, int64_t count,
                                      uint8_t* out) {
  CSTS_REQUIRE(out && count >= 0, "bad args");
  uint32_t w[4];
  uint64_t have = ~(uint64_t)0;
  for (int64_t i = 0; i < count; ++i) {
    const uint64_t e = first + (uint64_t)i;
    if ((e >> 2) != have) {
      have = e >> 2;
      dropout_block(key0, key1, site, have, w);
    }
    out[i] = w[e & 3] < thr ? 1 : 0;
  }
  return 0;
}
