// LoRA fine-tuning kernels (mvd_lora_*): W_eff = W0 + s B A with A [r][in], B [out][r], 1 <= r <= 64, everything fp32 on the
// vector ALU (no fp16 / bf16 operand, the same code in both builds).
//   lora_project   the dense gradient dW [out][in] the backward pass already wrote is projected onto the adapters,
//                  gA = s B^T dW, gB = s dW A^T.  One streaming pass over dW: a workgroup stages a 32 x 128 tile of dW with the
//                  matching rows of A and B in LDS and writes the tile's partial sums (gA: over its 32 rows, gB: over its 128
//                  columns) to a workspace; a second launch adds the partials of a column / a row in tile order and scales.
//                  No atomic: every sum is ordered by indices alone (rows / columns ascending inside a tile, tiles ascending), so two
//                  runs agree bit for bit.
//   lora_merge     W = W0 + s B A over the same tiles, W0 from the compact copy taken at attach time; writes exactly out x in
//                  elements per target (the arena's padding behind a tensor is not touched).
// Both take a device table of targets and cover all of them in one launch: a workgroup finds its target by binary search over the
// targets' first tile.  Rows of dW / W / A are moved as 16-byte lane accesses when `in` is a multiple of 4 and the bases are
// 16-byte aligned (every arena tensor starts at a multiple of 64 floats), element by element otherwise.
#include "common.h"

namespace {

constexpr int LT_O = LORA_TILE_O, LT_I = LORA_TILE_I;
constexpr int LT_LD = LT_I + 4;  // LDS row stride: one 16-byte access of padding, so that rows do not start on one bank
constexpr int LT_C4 = LT_I / 4;  // float4 groups per tile row

// index of the last target whose first block (tile0 / red0) is <= b
template <bool RED>
__device__ inline int lora_find(const LoraTarget* tab, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((RED ? tab[mid].red0 : tab[mid].tile0) <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// src[0..3] of a row with n valid elements from column i on (i % 4 == 0); zero beyond the row
__device__ inline float4 row_load4(const float* row, int i, int n, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i >= n) return v;
  if (vec) return *(const float4*)(row + i);
  v.x = row[i];
  if (i + 1 < n) v.y = row[i + 1];
  if (i + 2 < n) v.z = row[i + 2];
  if (i + 3 < n) v.w = row[i + 3];
  return v;
}
__device__ inline void row_store4(float* row, int i, int n, bool vec, float4 v) {
  if (i >= n) return;
  if (vec) {
    *(float4*)(row + i) = v;
    return;
  }
  row[i] = v.x;
  if (i + 1 < n) row[i + 1] = v.y;
  if (i + 2 < n) row[i + 2] = v.z;
  if (i + 3 < n) row[i + 3] = v.w;
}

// part: per target [nrt][r][in] partial gA (summed over a tile's rows) at pa_off, [nct][out][r] partial gB at pb_off
__global__ __launch_bounds__(256) void lora_project_kernel(const LoraTarget* __restrict__ tab, int n, const float* __restrict__ dW,
                                                           const float* __restrict__ Ab, const float* __restrict__ Bb, int r,
                                                           float* __restrict__ part) {
  extern __shared__ float4 lora_lds4[];
  float* dWs = (float*)lora_lds4;  // [LT_O][LT_LD]
  float* As = dWs + LT_O * LT_LD;  // [r][LT_LD]
  float* Bs = As + r * LT_LD;      // [LT_O][r]
  const int t = threadIdx.x;
  const LoraTarget T = tab[lora_find<false>(tab, n, (int)blockIdx.x)];
  const int tile = (int)blockIdx.x - T.tile0, nct = (T.in + LT_I - 1) / LT_I;
  const int rt = tile / nct, ct = tile - rt * nct, o0 = rt * LT_O, i0 = ct * LT_I;
  const int out = T.out, in = T.in;
  const float* dw = dW + T.w_off;
  const float* A = Ab + T.a_off;
  const float* B = Bb + T.b_off;
  float* pA = part + T.pa_off + (size_t)rt * r * in;
  float* pB = part + T.pb_off + (size_t)ct * out * r;
  const bool vec = (in & 3) == 0 && al16(dw) && al16(A) && al16(pA);
  for (int idx = t; idx < LT_O * LT_C4; idx += 256) {
    const int row = idx / LT_C4, c4 = idx - row * LT_C4, o = o0 + row;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < out) v = row_load4(dw + (size_t)o * in, i0 + c4 * 4, in, vec);
    *(float4*)(dWs + row * LT_LD + c4 * 4) = v;
  }
  for (int idx = t; idx < r * LT_C4; idx += 256) {
    const int k = idx / LT_C4, c4 = idx - k * LT_C4;
    *(float4*)(As + k * LT_LD + c4 * 4) = row_load4(A + (size_t)k * in, i0 + c4 * 4, in, vec);
  }
  for (int idx = t; idx < LT_O * r; idx += 256) {
    const int row = idx / r;
    Bs[idx] = o0 + row < out ? B[(size_t)o0 * r + idx] : 0.f;
  }
  __syncthreads();
  // gA partial [k][4 columns] = sum over the tile's rows, ascending
  for (int it = t; it < r * LT_C4; it += 256) {
    const int k = it / LT_C4, c4 = it - k * LT_C4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int o = 0; o < LT_O; ++o) {
      const float b = Bs[o * r + k];
      const float4 d = *(const float4*)(dWs + o * LT_LD + c4 * 4);
      acc.x = fmaf(b, d.x, acc.x);
      acc.y = fmaf(b, d.y, acc.y);
      acc.z = fmaf(b, d.z, acc.z);
      acc.w = fmaf(b, d.w, acc.w);
    }
    row_store4(pA + (size_t)k * in, i0 + c4 * 4, in, vec, acc);
  }
  // gB partial [row][k] = sum over the tile's columns: four interleaved chains (column mod 4), ascending, then (x + y) + (z + w)
  for (int it = t; it < LT_O * r; it += 256) {
    const int row = it / r, k = it - row * r;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int c4 = 0; c4 < LT_C4; ++c4) {
      const float4 d = *(const float4*)(dWs + row * LT_LD + c4 * 4);
      const float4 a = *(const float4*)(As + k * LT_LD + c4 * 4);
      acc.x = fmaf(d.x, a.x, acc.x);
      acc.y = fmaf(d.y, a.y, acc.y);
      acc.z = fmaf(d.z, a.z, acc.z);
      acc.w = fmaf(d.w, a.w, acc.w);
    }
    if (o0 + row < out) pB[(size_t)o0 * r + it] = (acc.x + acc.y) + (acc.z + acc.w);
  }
}

// gA[e] = scale * sum over the row tiles, gB[e] = scale * sum over the column tiles, tiles ascending; overwrites
__global__ __launch_bounds__(256) void lora_reduce_kernel(const LoraTarget* __restrict__ tab, int n, const float* __restrict__ part, int r,
                                                          float scale, float* __restrict__ gAb, float* __restrict__ gBb) {
  const LoraTarget T = tab[lora_find<true>(tab, n, (int)blockIdx.x)];
  const size_t nA = (size_t)r * T.in, nB = (size_t)T.out * r;
  const int blk = (int)blockIdx.x - T.red0, nbA = (int)((nA + 255) / 256);
  if (blk < nbA) {
    const size_t e = (size_t)blk * 256 + threadIdx.x;
    if (e >= nA) return;
    const float* p = part + T.pa_off + e;
    const int nrt = (T.out + LT_O - 1) / LT_O;
    float acc = 0.f;
    for (int q = 0; q < nrt; ++q) acc += p[(size_t)q * nA];
    gAb[T.a_off + e] = scale * acc;
  } else {
    const size_t e = (size_t)(blk - nbA) * 256 + threadIdx.x;
    if (e >= nB) return;
    const float* p = part + T.pb_off + e;
    const int nct = (T.in + LT_I - 1) / LT_I;
    float acc = 0.f;
    for (int q = 0; q < nct; ++q) acc += p[(size_t)q * nB];
    gBb[T.b_off + e] = scale * acc;
  }
}

// W[o][i] = W0[o][i] + scale * sum_k B[o][k] A[k][i], k ascending; a thread owns 4 rows x 4 columns of the tile
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraTarget* __restrict__ tab, int n, const float* __restrict__ W0b,
                                                         const float* __restrict__ Ab, const float* __restrict__ Bb, int r, float scale,
                                                         float* __restrict__ Wb) {
  extern __shared__ float4 lora_lds4[];
  float* As = (float*)lora_lds4;  // [r][LT_LD]
  float* Bt = As + r * LT_LD;     // [r][LT_O]: B transposed, so that a thread's 4 rows are one 16-byte read
  const int t = threadIdx.x;
  const LoraTarget T = tab[lora_find<false>(tab, n, (int)blockIdx.x)];
  const int tile = (int)blockIdx.x - T.tile0, nct = (T.in + LT_I - 1) / LT_I;
  const int rt = tile / nct, ct = tile - rt * nct, o0 = rt * LT_O, i0 = ct * LT_I;
  const int out = T.out, in = T.in;
  const float* W0 = W0b + T.w0_off;
  const float* A = Ab + T.a_off;
  const float* B = Bb + T.b_off;
  float* W = Wb + T.w_off;
  const bool vec = (in & 3) == 0 && al16(W0) && al16(A) && al16(W);
  for (int idx = t; idx < r * LT_C4; idx += 256) {
    const int k = idx / LT_C4, c4 = idx - k * LT_C4;
    *(float4*)(As + k * LT_LD + c4 * 4) = row_load4(A + (size_t)k * in, i0 + c4 * 4, in, vec);
  }
  for (int idx = t; idx < LT_O * r; idx += 256) {
    const int row = idx / r, k = idx - row * r;
    Bt[k * LT_O + row] = o0 + row < out ? B[(size_t)o0 * r + idx] : 0.f;
  }
  __syncthreads();
  const int c4 = t & (LT_C4 - 1), rg = t / LT_C4;  // 32 column groups x 8 row groups
  float4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < r; ++k) {
    const float4 a = *(const float4*)(As + k * LT_LD + c4 * 4);
    const float4 b4 = *(const float4*)(Bt + k * LT_O + rg * 4);
    const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j].x = fmaf(b[j], a.x, acc[j].x);
      acc[j].y = fmaf(b[j], a.y, acc[j].y);
      acc[j].z = fmaf(b[j], a.z, acc[j].z);
      acc[j].w = fmaf(b[j], a.w, acc[j].w);
    }
  }
  const int i = i0 + c4 * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int o = o0 + rg * 4 + j;
    if (o >= out || i >= in) continue;
    float4 w = row_load4(W0 + (size_t)o * in, i, in, vec);
    if (scale != 0.f) {  // strength 0 is W0 itself, whatever the adapters hold
      w.x = fmaf(scale, acc[j].x, w.x);
      w.y = fmaf(scale, acc[j].y, w.y);
      w.z = fmaf(scale, acc[j].z, w.z);
      w.w = fmaf(scale, acc[j].w, w.w);
    }
    row_store4(W + (size_t)o * in, i, in, vec, w);
  }
}

}  // namespace

// Fills tile0 / red0 / pa_off / pb_off of n targets (out, in set) for rank r; the partial workspace is *part_floats floats.
void lora_plan(LoraTarget* tab, int n, int r, int* tiles, int* red_blocks, size_t* part_floats) {
  long long tile = 0, red = 0;
  size_t at = 0;
  auto pad = [](size_t v) { return (v + 63) & ~(size_t)63; };
  for (int i = 0; i < n; ++i) {
    LoraTarget& T = tab[i];
    const long long nrt = (T.out + LT_O - 1) / LT_O, nct = (T.in + LT_I - 1) / LT_I;
    T.tile0 = (int)tile;
    T.red0 = (int)red;
    tile += nrt * nct;
    red += ((long long)r * T.in + 255) / 256 + ((long long)T.out * r + 255) / 256;
    T.pa_off = (long long)at;
    at += pad((size_t)nrt * r * T.in);
    T.pb_off = (long long)at;
    at += pad((size_t)nct * T.out * r);
  }
  *tiles = tile > 0x7fffffffLL ? -1 : (int)tile;
  *red_blocks = red > 0x7fffffffLL ? -1 : (int)red;
  *part_floats = at;
}

int lora_project(const LoraTarget* tab, int n, int tiles, int red_blocks, const float* dW, const float* A, const float* B, int r,
                 float scale, float* part, float* gA, float* gB, hipStream_t s) {
  if (r < 1 || r > LORA_MAX_RANK) return mvd_fail("lora_project: the rank must be in 1..64");
  if (!tab || !dW || !A || !B || !part || !gA || !gB) return mvd_fail("lora_project: null argument");
  if (n < 1 || tiles < 1 || red_blocks < 1) return mvd_fail("lora_project: no target (or more than 2^31 tiles)");
  const size_t lds = ((size_t)LT_O * LT_LD + (size_t)r * LT_LD + (size_t)LT_O * r) * sizeof(float);
  hipLaunchKernelGGL(lora_project_kernel, dim3(tiles), dim3(256), lds, s, tab, n, dW, A, B, r, part);
  hipLaunchKernelGGL(lora_reduce_kernel, dim3(red_blocks), dim3(256), 0, s, tab, n, part, r, scale, gA, gB);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int lora_merge(const LoraTarget* tab, int n, int tiles, const float* W0, const float* A, const float* B, int r, float scale, float* W,
               hipStream_t s) {
  if (r < 1 || r > LORA_MAX_RANK) return mvd_fail("lora_merge: the rank must be in 1..64");
  if (!tab || !W0 || !A || !B || !W) return mvd_fail("lora_merge: null argument");
  if (n < 1 || tiles < 1) return mvd_fail("lora_merge: no target (or more than 2^31 tiles)");
  const size_t lds = ((size_t)r * LT_LD + (size_t)r * LT_O) * sizeof(float);
  hipLaunchKernelGGL(lora_merge_kernel, dim3(tiles), dim3(256), lds, s, tab, n, W0, A, B, r, scale, W);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
