// Small HBM-/latency-bound helpers: per-sample linears (timestep MLPs, FiLM projections), sinusoidal
// embedding, layout changes at the NCHW boundary, weight packing/folding, CFG + DDIM update.
#include "common.h"

namespace {

// out[r][n] (+)= sum_k act(a[r][k]) * w[n][k] + bias[n];  rows <= a few dozen (one per sample / view).
// One wave per output column, lanes split K, 8 rows per pass.
__global__ __launch_bounds__(256) void small_linear_kernel(const float* __restrict__ a, int lda, int rows, int K,
                                                           const half_t* __restrict__ w, const float* __restrict__ bias,
                                                           int N, int act_in, float* __restrict__ out, int ldo,
                                                           int accumulate, int vec) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const half_t* wr = w + (long)n * K;
  // rows < 0: the single input row is broadcast to -rows output rows (FiLM: one step embedding, many views)
  const int out_rows = rows < 0 ? -rows : rows;
  const int in_rows = rows < 0 ? 1 : rows;
  for (int r0 = 0; r0 < in_rows; r0 += 8) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (vec) {  // small_linear_form: K % 8 == 0, lda % 4 == 0, a and w 16-byte aligned
      for (int k = lane * 8; k < K; k += 512) {
        const h8 wv = *(const h8*)(wr + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (r0 + j < in_rows) {
            const float4 a0 = *(const float4*)(a + (long)(r0 + j) * lda + k);
            const float4 a1 = *(const float4*)(a + (long)(r0 + j) * lda + k + 4);
            float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float x = v[e];
              if (act_in == ACT_SILU) x = x / (1.0f + __expf(-x));
              acc[j] += x * (float)wv[e];
            }
          }
        }
      }
    } else {
      for (int k = lane; k < K; k += 64) {
        const float wv = (float)wr[k];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (r0 + j < in_rows) {
            float v = a[(long)(r0 + j) * lda + k];
            if (act_in == ACT_SILU) v = v / (1.0f + __expf(-v));
            acc[j] += v * wv;
          }
        }
      }
    }
    if (rows < 0) {
      float v = acc[0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      v += bias ? bias[n] : 0.f;
      for (int r = lane; r < out_rows; r += 64) {
        float* o = out + (long)r * ldo + n;
        *o = accumulate ? (*o + v) : v;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o);
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (r0 + j < rows) {
          float v = acc[j] + (bias ? bias[n] : 0.f);
          float* o = out + (long)(r0 + j) * ldo + n;
          *o = accumulate ? (*o + v) : v;
        }
      }
    }
  }
}

// ldm/modules/diffusionmodules/util.py:151-171
__global__ void timestep_embedding_kernel(const int64_t* __restrict__ t, int B, int dim, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (idx >= B * dim) return;
  const int b = idx / dim, j = idx - b * dim;
  float v = 0.f;
  if (j < 2 * half) {
    const int i = j < half ? j : j - half;
    const float f = expf(-9.210340371976184f * (float)i / (float)half);
    const float arg = (float)t[b] * f;
    v = j < half ? cosf(arg) : sinf(arg);
  }
  out[idx] = v;
}

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ in, int B, int C, int HW, float* __restrict__ out, int ldo,
                                    int cpad) {
  const long total = (long)B * HW * cpad;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % cpad);
    const long bp = idx / cpad;
    const int p = (int)(bp % HW), b = (int)(bp / HW);
    out[bp * ldo + c] = c < C ? in[((long)b * C + c) * HW + p] : 0.f;
  }
}

__global__ void nhwc_to_nchw_kernel(const float* __restrict__ in, int ld, int B, int C, int HW, float* __restrict__ out) {
  const long total = (long)B * C * HW;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int p = (int)(idx % HW);
    const long bc = idx / HW;
    const int c = (int)(bc % C), b = (int)(bc / C);
    out[idx] = in[((long)b * HW + p) * ld + c];
  }
}

// The two layout conversions as 32 x 32 tiles through LDS: 128-byte runs on both sides (the element-per-thread forms above read
// -- or write -- one float per cache line; the training step converts four source volumes and four gradient volumes of up to
// 100 MB per call).  Taken for C >= 16; the 4- and 8-channel latents keep the simple kernels.  Same values.
__global__ __launch_bounds__(256) void nchw_to_nhwc_tiled_kernel(const float* __restrict__ in, int C, int HW, float* __restrict__ out, int ldo,
                                                                 int cpad) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, p = p0 + tx;
    tile[ty + 8 * i][tx] = (c < C && p < HW) ? in[((long)b * C + c) * HW + p] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + ty + 8 * i, c = c0 + tx;
    if (p < HW && c < cpad) out[((long)b * HW + p) * ldo + c] = tile[tx][ty + 8 * i];
  }
}
__global__ __launch_bounds__(256) void nhwc_to_nchw_tiled_kernel(const float* __restrict__ in, int ld, int C, int HW, float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + ty + 8 * i, c = c0 + tx;
    tile[ty + 8 * i][tx] = (p < HW && c < C) ? in[((long)b * HW + p) * ld + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, p = p0 + tx;
    if (c < C && p < HW) out[((long)b * C + c) * HW + p] = tile[tx][ty + 8 * i];
  }
}

// dst fp16 [taps][N][Cin]; src fp32 [N][Cin][taps] (conv / linear) or [Cin][N][taps] (ConvTranspose).
// geglu: rows are re-ordered into alternating 32-row blocks (value | gate) so the GEMM epilogue can pair
// fragment 0 with fragment 1 of a wave.
// cin_src < Cin zero-pads the channel axis (e.g. the 4-channel latent conv padded to 8).
__global__ void pack_weight_kernel(const float* __restrict__ src, int N, int Cin, int taps, int transposed, int geglu,
                                   int cin_src, half_t* __restrict__ dst, int xp) {
  const long total = (long)taps * N * Cin;
  const int Cl = xp ? Cin / 3 : Cin;  // extended precision: [w_hi | w_hi | w_lo] against activations [a_hi | a_lo | a_hi]
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int cp = (int)(idx % Cin), seg = cp / Cl, c = cp - seg * Cl;
    const long tn = idx / Cin;
    const int nd = (int)(tn % N), t = (int)(tn / N);
    int n = nd;
    if (geglu) {
      const int j = nd >> 6, wi = nd & 63;
      n = wi < 32 ? 32 * j + wi : N / 2 + 32 * j + (wi - 32);
    }
    if (c >= cin_src) {
      dst[idx] = (half_t)0;
      continue;
    }
    const long s = transposed ? ((long)c * N + n) * taps + t : ((long)n * cin_src + c) * taps + t;
    const float w = src[s];
    const half_t hi = (half_t)w;
    dst[idx] = seg < 2 ? hi : (half_t)(w - (float)hi);
  }
}

// The same packing for conv weights (taps > 1, not transposed): one workgroup per (output row, 64 input channels) reads its
// 64 * taps source floats as one contiguous run and writes 128-byte row segments per tap (the element-per-thread form reads
// with a stride of taps * 4 bytes, once per tap).
__global__ __launch_bounds__(256) void pack_weight_taps_kernel(const float* __restrict__ src, int N, int Cin, int taps, int geglu, int cin_src,
                                                               half_t* __restrict__ dst, int xp) {
  __shared__ float sw[64 * 27];
  const int Cl = xp ? Cin / 3 : Cin;
  const int nd = blockIdx.y, c0 = blockIdx.x * 64;
  int n = nd;
  if (geglu) {
    const int j = nd >> 6, wi = nd & 63;
    n = wi < 32 ? 32 * j + wi : N / 2 + 32 * j + (wi - 32);
  }
  const int nc = min(64, cin_src - c0);  // source channels of this tile (<= 0: pure padding)
  const float* p = src + ((long)n * cin_src + c0) * taps;
  for (int i = threadIdx.x; i < nc * taps; i += 256) sw[i] = p[i];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * taps; i += 256) {
    const int t = i >> 6, cl = i & 63, c = c0 + cl;
    if (c >= Cl) continue;
    const float w = cl < nc ? sw[cl * taps + t] : 0.f;
    const half_t hi = (half_t)w;
    half_t* d = dst + ((long)t * N + nd) * Cin + c;
    d[0] = hi;
    if (xp) {
      d[Cl] = hi;
      d[2 * Cl] = (half_t)(w - (float)hi);
    }
  }
}

// The same with four output rows per workgroup and 16-byte stores (eight channels of one tap per thread): 8 x fewer store
// instructions and a quarter of the workgroups (a re-pack of a training step runs this 130 times).  Needs Cl % 8 == 0 and a
// 16-byte aligned dst; same values.
__global__ __launch_bounds__(256) void pack_weight_taps_vec_kernel(const float* __restrict__ src, int N, int Cin, int taps, int geglu,
                                                                   int cin_src, half_t* __restrict__ dst, int xp) {
  __shared__ float sw[4][64 * 27];
  const int Cl = xp ? Cin / 3 : Cin;
  const int nd0 = blockIdx.y * 4, c0 = blockIdx.x * 64;
  const int nc = min(64, cin_src - c0);  // source channels of this tile (<= 0: pure padding)
#pragma unroll
  for (int rw = 0; rw < 4; ++rw) {
    const int nd = nd0 + rw;
    if (nd >= N) break;
    int n = nd;
    if (geglu) {
      const int j = nd >> 6, wi = nd & 63;
      n = wi < 32 ? 32 * j + wi : N / 2 + 32 * j + (wi - 32);
    }
    const float* p = src + ((long)n * cin_src + c0) * taps;
    for (int i = threadIdx.x; i < nc * taps; i += 256) sw[rw][i] = p[i];
  }
  __syncthreads();
  const int per_row = taps * 8;  // (tap, 8-channel group) items of one output row
  for (int i = threadIdx.x; i < 4 * per_row; i += 256) {
    const int rw = i / per_row, rem = i - rw * per_row, t = rem >> 3, cl = (rem & 7) * 8, c = c0 + cl, nd = nd0 + rw;
    if (nd >= N || c >= Cl) continue;
    h8 hi, lo;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float w = cl + k < nc ? sw[rw][(cl + k) * taps + t] : 0.f;
      hi[k] = (half_t)w;
      lo[k] = (half_t)(w - (float)hi[k]);
    }
    half_t* d = dst + ((long)t * N + nd) * Cin + c;
    *(h8*)d = hi;
    if (xp) {
      *(h8*)(d + Cl) = hi;
      *(h8*)(d + 2 * Cl) = lo;
    }
  }
}

__global__ void permute_geglu_bias_kernel(const float* __restrict__ src, int N, float* __restrict__ dst) {
  const int nd = blockIdx.x * blockDim.x + threadIdx.x;
  if (nd >= N) return;
  const int j = nd >> 6, wi = nd & 63;
  dst[nd] = src[wi < 32 ? 32 * j + wi : N / 2 + 32 * j + (wi - 32)];
}

__global__ void f32_to_f16_kernel(const float* __restrict__ in, half_t* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (half_t)in[i];
}

// channels-last rows with stride lda -> dense fp16 rows (C % 4 == 0): operand copy for the LDS-DMA kernels
__global__ void rows_f32_to_f16_split_kernel(const float* __restrict__ in, int lda, long rows, int C, half_t* __restrict__ out) {
  const int q = C >> 2;
  const long total = rows * q;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / q;
    const int c = (int)(i - r * q) * 4;
    const float4 v = *(const float4*)(in + r * lda + c);
    h4 hi, lo;
    hi[0] = (half_t)v.x; hi[1] = (half_t)v.y; hi[2] = (half_t)v.z; hi[3] = (half_t)v.w;
    lo[0] = (half_t)(v.x - (float)hi[0]); lo[1] = (half_t)(v.y - (float)hi[1]);
    lo[2] = (half_t)(v.z - (float)hi[2]); lo[3] = (half_t)(v.w - (float)hi[3]);
    half_t* o = out + r * 3 * C + c;
    *(h4*)o = hi;
    *(h4*)(o + C) = lo;
    *(h4*)(o + 2 * C) = hi;
  }
}

__global__ void rows_f32_to_f16_kernel(const float* __restrict__ in, int lda, long rows, int C, half_t* __restrict__ out) {
  const int q = C >> 2;
  const long total = rows * q;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / q;
    const int c = (int)(i - r * q) * 4;
    const float4 v = *(const float4*)(in + r * lda + c);
    h4 o;
    o[0] = (half_t)v.x; o[1] = (half_t)v.y; o[2] = (half_t)v.z; o[3] = (half_t)v.w;
    *(h4*)(out + r * C + c) = o;
  }
}

// 3x3 conv applied to a nearest-x2 upsampled image == four 2x2 convs on the original image, one per output parity
// (py, px): rows {2y-1, 2y, 2y+1} of the upsampled image are input rows {y-1, y, y} (py = 0) or {y, y, y+1} (py = 1),
// so the taps that land on the same input pixel are summed once here (fp32) instead of multiplied separately:
// 16 instead of 36 tap-GEMMs per four output pixels.  src [N][Cin][3][3] -> dst [(py*2+px)*4 + a*2 + b][N][Cin].
__global__ void pack_upconv_weight_kernel(const float* __restrict__ src, int N, int Cin, half_t* __restrict__ dst) {
  const long total = (long)16 * N * Cin;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % Cin);
    const int n = (int)((idx / Cin) % N);
    const int slab = (int)(idx / ((long)Cin * N));
    const int b = slab & 1, a = (slab >> 1) & 1, px = (slab >> 2) & 1, py = slab >> 3;
    // kernel rows / cols folded onto input offset a (resp. b) for this parity
    const int ky0 = py == 0 ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 2), ky1 = py == 0 ? (a == 0 ? 0 : 2) : (a == 0 ? 1 : 2);
    const int kx0 = px == 0 ? (b == 0 ? 0 : 1) : (b == 0 ? 0 : 2), kx1 = px == 0 ? (b == 0 ? 0 : 2) : (b == 0 ? 1 : 2);
    const float* w = src + ((long)n * Cin + c) * 9;
    float acc = 0.f;
    for (int ky = ky0; ky <= ky1; ++ky)
      for (int kx = kx0; kx <= kx1; ++kx) acc += w[ky * 3 + kx];
    dst[idx] = (half_t)acc;
  }
}

__global__ void fill_rows_f16_kernel(half_t* __restrict__ out, int ld, int rows, const half_t* __restrict__ vec, int n) {
  const long total = (long)rows * n;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % n);
    out[(idx / n) * ld + c] = vec[c];
  }
}

// C[z][m][n] = scale * sum_k A_z(m,k) B_z(k,n) with strided operands (element (m,k) of A at a[z*a_zs + m*a_rs + k*a_cs], ...),
// fp64 accumulation, 16 x 16 tiles through LDS: the weight folds below (a few GFLOP at finalize / re-pack time; the one-thread-
// per-output form they replace ran at 1 TFLOP/s and was 40 % of a re-pack)
// (round 4: 64 x 64 tiles, a 4 x 4 block of outputs per thread -- eight LDS reads per sixteen fp64 fmas instead of two per fma;
// every output is still the k-ascending fp64 sum of exact fp32 x fp32 products, so the folded weights are bit for bit the same)
__global__ __launch_bounds__(256) void fold_gemm_kernel(const float* __restrict__ a, long a_zs, long a_rs, long a_cs,
                                                        const float* __restrict__ b, long b_zs, long b_rs, long b_cs, int M, int N, int K,
                                                        float scale, long c_zs, long c_rs, long c_cs, half_t* __restrict__ out,
                                                        float* __restrict__ out32) {
  __shared__ float sA[16][68], sB[16][68];  // [k][m], [k][n]
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, z = blockIdx.z;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const float* az = a + z * a_zs;
  const float* bz = b + z * b_zs;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // A tile: element (m = m0 + ml, k = k0 + kl); thread t covers ml = (t >> 4) + 16 e, kl = t & 15; B tile: (k = k0 + (t >> 4)
      // ... ) as before: kl = t >> 4, nl = (t & 15) + 16 e
      const int ml = ty + 16 * e, ka = k0 + tx;
      sA[tx][ml] = (m0 + ml < M && ka < K) ? az[(long)(m0 + ml) * a_rs + (long)ka * a_cs] : 0.f;
      const int nl = tx + 16 * e, kb = k0 + ty;
      sB[ty][nl] = (kb < K && n0 + nl < N) ? bz[(long)kb * b_rs + (long)(n0 + nl) * b_cs] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      double av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = (double)sA[kk][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = (double)sB[kk][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + ty + 16 * i, n = n0 + tx + 16 * j;
      if (m < M && n < N) {
        const long o = z * c_zs + (long)m * c_rs + (long)n * c_cs;
        const float v = (float)(acc[i][j] * (double)scale);
        if (out32) out32[o] = v;
        else out[o] = (half_t)v;
      }
    }
}

__global__ void relu_beta_tile_kernel(const float* __restrict__ beta, int Cc, int heads, half_t* __restrict__ out, int split) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int W4 = heads * Cc;
  if (idx >= W4) return;
  const float v = fmaxf(beta[idx % Cc], 0.f);
  const half_t hi = (half_t)v;
  out[idx] = hi;
  if (split) {
    out[W4 + idx] = (half_t)(v - (float)hi);
    out[2 * W4 + idx] = hi;
  }
}

// UNetWrapper.predict_with_unconditional_scale (morphable_diffusion.py:148) + denoise_apply_impl (:692-697)
__global__ void cfg_ddim_kernel(const float* __restrict__ ec, const float* __restrict__ eu, float scale,
                                const float* __restrict__ x, const float* __restrict__ noise, float s1m, float sqrt_at,
                                float sqrt_aprev, float dir_coef, float sigma, float* __restrict__ eps_out,
                                float* __restrict__ x_prev, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float e = ec[i];
    if (eu) e = eu[i] + scale * (e - eu[i]);
    if (eps_out) eps_out[i] = e;
    if (x_prev) {
      const float pred_x0 = (x[i] - s1m * e) / sqrt_at;
      float xp = sqrt_aprev * pred_x0 + dir_coef * e;
      if (noise) xp += sigma * noise[i];
      x_prev[i] = xp;
    }
  }
}

// The same CFG combine and x0 prediction (same expressions, same order), then one DPM-Solver++ multistep update
// (schedule.py DPMSolverSchedule):  x_next = c_x x + c_d x0 + c_c (x0 - x0_hist) + c_n noise,  x0_hist <- x0.
// x0_hist is read, then overwritten, by the same thread (in place); it is not read when use_hist == 0 (the first step: its
// contents are undefined there and 0 * NaN would not vanish).  eu, noise and eps_out may be null.
__device__ __forceinline__ void dpm_elem(float ec, const float eu, bool has_eu, float scale, float x, float z, bool has_z, float h,
                                         bool use_hist, const DpmCoef& k, float& e, float& pred_x0, float& xn) {
  e = ec;
  if (has_eu) e = eu + scale * (e - eu);
  pred_x0 = (x - k.s1m * e) / k.sqrt_at;
  xn = k.c_x * x + k.c_d * pred_x0;
  if (use_hist) xn += k.c_c * (pred_x0 - h);
  if (has_z) xn += k.c_n * z;
}

// vec != 0 (every pointer 16-byte aligned): elements [0, n & ~3) move as float4 (16-byte loads / stores), the scalar loop
// takes the tail; vec == 0: the scalar loop takes everything
__global__ void cfg_dpm_kernel(const float* __restrict__ ec, const float* __restrict__ eu, float scale, const float* __restrict__ x,
                               const float* __restrict__ noise, DpmCoef k, float* x0_hist, int use_hist,
                               float* __restrict__ eps_out, float* __restrict__ x_next, size_t n, int vec) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n4 = vec ? n / 4 : 0;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t q = tid; q < n4; q += stride) {
    const float4 c4 = reinterpret_cast<const float4*>(ec)[q];
    const float4 u4 = eu ? reinterpret_cast<const float4*>(eu)[q] : zero4;
    const float4 x4 = reinterpret_cast<const float4*>(x)[q];
    const float4 z4 = noise ? reinterpret_cast<const float4*>(noise)[q] : zero4;
    const float4 h4 = use_hist ? reinterpret_cast<const float4*>(x0_hist)[q] : zero4;
    float4 e4, p4, n4v;
    dpm_elem(c4.x, u4.x, eu, scale, x4.x, z4.x, noise, h4.x, use_hist, k, e4.x, p4.x, n4v.x);
    dpm_elem(c4.y, u4.y, eu, scale, x4.y, z4.y, noise, h4.y, use_hist, k, e4.y, p4.y, n4v.y);
    dpm_elem(c4.z, u4.z, eu, scale, x4.z, z4.z, noise, h4.z, use_hist, k, e4.z, p4.z, n4v.z);
    dpm_elem(c4.w, u4.w, eu, scale, x4.w, z4.w, noise, h4.w, use_hist, k, e4.w, p4.w, n4v.w);
    if (eps_out) reinterpret_cast<float4*>(eps_out)[q] = e4;
    reinterpret_cast<float4*>(x0_hist)[q] = p4;
    reinterpret_cast<float4*>(x_next)[q] = n4v;
  }
  for (size_t i = n4 * 4 + tid; i < n; i += stride) {
    float e, p, xn;
    dpm_elem(ec[i], eu ? eu[i] : 0.f, eu, scale, x[i], noise ? noise[i] : 0.f, noise, use_hist ? x0_hist[i] : 0.f, use_hist, k, e, p,
             xn);
    if (eps_out) eps_out[i] = e;
    x0_hist[i] = p;
    x_next[i] = xn;
  }
}

__global__ void add_rows_kernel(float* __restrict__ dst, const float* __restrict__ a, const float* __restrict__ b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = a[i] + (b ? b[i] : 0.f);
}

inline int grid_for(size_t n, int block = 256, int cap = 4096) {
  size_t g = (n + block - 1) / block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

// 1: the 16-byte path (h8 weight and float4 activation loads), 0: the scalar path.  Callers pass rows of larger tables
// (t_embed + b * td, v_embed + tgt * vd), so the operand pointers are part of the choice, as in launch_cfg_dpm.
int small_linear_form(const float* a, int lda, int K, const half_t* w) {
  return (K & 7) == 0 && (lda & 3) == 0 && (((uintptr_t)a | (uintptr_t)w) & 15) == 0;
}

int launch_small_linear(const float* a, int lda, int rows, int K, const half_t* w, const float* bias, int N,
                        int act_in, float* out, int ldo, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(small_linear_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, a, lda, rows, K, w, bias, N, act_in, out,
                     ldo, accumulate, small_linear_form(a, lda, K, w));
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_timestep_embedding(const int64_t* t, int B, int dim, float* out, hipStream_t s) {
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(cdiv(B * dim, 256)), dim3(256), 0, s, t, B, dim, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// 1: the 32 x 32 LDS-tiled kernel, 0: the element-per-thread kernel (cols: cpad, or C for nhwc_to_nchw)
int layout_form(int B, int C, int HW, int cols) { return C >= 16 && HW >= 32 && B <= 65535 && cdiv(cols, 32) <= 65535; }

int launch_nchw_to_nhwc(const float* in, int B, int C, int HW, float* out, int ldo, int cpad, hipStream_t s) {
  if (layout_form(B, C, HW, cpad))
    hipLaunchKernelGGL(nchw_to_nhwc_tiled_kernel, dim3(cdiv(HW, 32), cdiv(cpad, 32), B), dim3(256), 0, s, in, C, HW, out, ldo, cpad);
  else
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for((size_t)B * HW * cpad)), dim3(256), 0, s, in, B, C, HW, out,
                       ldo, cpad);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_nhwc_to_nchw(const float* in, int ld, int B, int C, int HW, float* out, hipStream_t s) {
  if (layout_form(B, C, HW, C))
    hipLaunchKernelGGL(nhwc_to_nchw_tiled_kernel, dim3(cdiv(HW, 32), cdiv(C, 32), B), dim3(256), 0, s, in, ld, C, HW, out);
  else
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for((size_t)B * HW * C)), dim3(256), 0, s, in, ld, B, C, HW, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// 0: the element-per-thread kernel, 1: the per-tap kernel, 2: the per-tap kernel with 16-byte stores
int pack_weight_form(int N, int Cin, int taps, int transposed, const half_t* dst, int xp) {
  if (!(taps > 1 && taps <= 27 && !transposed && N <= 65535)) return 0;
  const int Cl = xp ? Cin / 3 : Cin;
  return !(Cl & 7) && !((uintptr_t)dst & 15) ? 2 : 1;
}

int launch_pack_weight(const float* src, int N, int Cin, int taps, int transposed, int geglu, half_t* dst,
                       hipStream_t s, int cin_src, int xp) {
  if (xp && Cin % 3) return mvd_fail("pack_weight: the extended-precision layout needs Cin = 3 * Cl");
  if (cin_src <= 0) cin_src = xp ? Cin / 3 : Cin;
  if (const int form = pack_weight_form(N, Cin, taps, transposed, dst, xp)) {
    const int Cl = xp ? Cin / 3 : Cin;
    if (form == 2)
      hipLaunchKernelGGL(pack_weight_taps_vec_kernel, dim3(cdiv(Cl, 64), cdiv(N, 4)), dim3(256), 0, s, src, N, Cin, taps, geglu, cin_src,
                         dst, xp);
    else
      hipLaunchKernelGGL(pack_weight_taps_kernel, dim3(cdiv(Cl, 64), N), dim3(256), 0, s, src, N, Cin, taps, geglu, cin_src, dst, xp);
    HIP_CHECK_RET(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(pack_weight_kernel, dim3(grid_for((size_t)N * Cin * taps)), dim3(256), 0, s, src, N, Cin, taps,
                     transposed, geglu, cin_src, dst, xp);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_permute_geglu_bias(const float* src, int N, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(permute_geglu_bias_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, src, N, dst);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_f32_to_f16(const float* in, half_t* out, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(f32_to_f16_kernel, dim3(grid_for(n)), dim3(256), 0, s, in, out, n);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_rows_f32_to_f16(const float* in, int lda, long rows, int C, half_t* out, hipStream_t s) {
  if ((C & 3) || (lda & 3)) return mvd_fail("rows_f32_to_f16: C and lda must be multiples of 4");
  hipLaunchKernelGGL(rows_f32_to_f16_kernel, dim3(grid_for((size_t)rows * C / 4)), dim3(256), 0, s, in, lda, rows, C, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_rows_f32_to_f16_split(const float* in, int lda, long rows, int C, half_t* out, hipStream_t s) {
  if ((C & 3) || (lda & 3)) return mvd_fail("rows_f32_to_f16_split: C and lda must be multiples of 4");
  hipLaunchKernelGGL(rows_f32_to_f16_split_kernel, dim3(grid_for((size_t)rows * C / 4)), dim3(256), 0, s, in, lda, rows, C, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_pack_upconv_weight(const float* src, int N, int Cin, half_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(pack_upconv_weight_kernel, dim3(grid_for((size_t)16 * N * Cin)), dim3(256), 0, s, src, N, Cin, dst);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_fill_rows_f16(half_t* out, int ld, int rows, const half_t* vec, int n, hipStream_t s) {
  hipLaunchKernelGGL(fill_rows_f16_kernel, dim3(grid_for((size_t)rows * n)), dim3(256), 0, s, out, ld, rows, vec, n);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_fold_qk(const float* wq, const float* wk, int heads, int hd, int Cc, int I, float scale, half_t* out,
                   hipStream_t s, float* out32) {
  // W_qk[hn*Cc + j][i] = scale * sum_c Wk[hn*hd + c][j] * Wq[hn*hd + c][i]:  per head  C[j][i] = sum_c Wk^T(j,c) Wq(c,i)
  hipLaunchKernelGGL(fold_gemm_kernel, dim3(cdiv(I, 64), cdiv(Cc, 64), heads), dim3(256), 0, s, wk, (long)hd * Cc, 1L, (long)Cc, wq,
                     (long)hd * I, (long)I, 1L, Cc, I, hd, scale, (long)Cc * I, (long)I, 1L, out, out32);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_fold_ov(const float* wo, const float* wv, int heads, int hd, int Cc, int I, half_t* out, hipStream_t s,
                   float* out32) {
  // W_ov[i][hn*Cc + j] = sum_c Wo[i][hn*hd + c] * Wv[hn*hd + c][j]:  per head  C[i][j] = sum_c Wo(i, hn*hd + c) Wv(hn*hd + c, j)
  // (Wo is [I][heads * hd]: its rows are heads * hd floats apart -- I only where the inner width equals I, as in every checkpoint)
  hipLaunchKernelGGL(fold_gemm_kernel, dim3(cdiv(Cc, 64), cdiv(I, 64), heads), dim3(256), 0, s, wo, (long)hd, (long)heads * hd, 1L, wv,
                     (long)hd * Cc, (long)Cc, 1L, I, Cc, hd, 1.0f, (long)Cc, (long)heads * Cc, 1L, out, out32);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_fold_mm(const float* a, int lda, const float* b, int ldb, int M, int N, int K, half_t* out16, int ldc, float* out32,
                   hipStream_t s) {
  hipLaunchKernelGGL(fold_gemm_kernel, dim3(cdiv(N, 64), cdiv(M, 64), 1), dim3(256), 0, s, a, 0L, (long)lda, 1L, b, 0L, (long)ldb, 1L, M, N, K,
                     1.0f, 0L, (long)ldc, 1L, out16, out32);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_relu_beta_tile(const float* beta, int Cc, int heads, half_t* out, hipStream_t s, int split) {
  hipLaunchKernelGGL(relu_beta_tile_kernel, dim3(cdiv(heads * Cc, 256)), dim3(256), 0, s, beta, Cc, heads, out, split);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_cfg_ddim(const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise,
                    float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float dir_coef, float sigma,
                    float* eps_out, float* x_prev, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(cfg_ddim_kernel, dim3(grid_for(n)), dim3(256), 0, s, eps_c, eps_u, scale, x, noise,
                     sqrt_one_minus_at, sqrt_at, sqrt_aprev, dir_coef, sigma, eps_out, x_prev, n);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_cfg_dpm(const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise, DpmCoef k,
                   float* x0_hist, int use_hist, float* eps_out, float* x_next, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  if (!eps_c || !x || !x0_hist || !x_next) return mvd_fail("launch_cfg_dpm: null argument");
  const auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const int vec = al(eps_c) && al(eps_u) && al(x) && al(noise) && al(x0_hist) && al(eps_out) && al(x_next);
  const size_t work = vec ? n / 4 + (n & 3) : n;
  hipLaunchKernelGGL(cfg_dpm_kernel, dim3(grid_for(work)), dim3(256), 0, s, eps_c, eps_u, scale, x, noise, k, x0_hist, use_hist ? 1 : 0,
                     eps_out, x_next, n, vec);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// investigation aid (MVD_DEBUG_SUM): order-independent 64-bit checksum of a buffer's bit patterns
__global__ void bits_checksum_kernel(const unsigned* __restrict__ p, size_t nwords, unsigned long long* __restrict__ out) {
  unsigned long long a = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x)
    a += (unsigned long long)p[i] * 0x9E3779B97F4A7C15ull + (i & 0xFFFF);
  atomicAdd(out, a);
}
int launch_bits_checksum(const void* p, size_t bytes, unsigned long long* out, hipStream_t s) {
  hipMemsetAsync(out, 0, 8, s);
  hipLaunchKernelGGL(bits_checksum_kernel, dim3(512), dim3(256), 0, s, (const unsigned*)p, bytes / 4, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_add_rows(float* dst, const float* a, const float* b, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(add_rows_kernel, dim3(grid_for(n)), dim3(256), 0, s, dst, a, b, n);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

namespace {
__global__ void probe_null_kernel() {}
}  // namespace
int launch_probe_null(hipStream_t s) {
  hipLaunchKernelGGL(probe_null_kernel, dim3(1), dim3(64), 0, s);
  return hipGetLastError() == hipSuccess ? 0 : mvd_fail("probe_null launch failed");
}

namespace {
__global__ __launch_bounds__(256) void add_image_rows_kernel(const float* __restrict__ in, int ldi, const float* __restrict__ img, int C4,
                                                             long total4, int HW, float* __restrict__ out, int ldo) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
    const long row = i / C4;
    const int q = (int)(i - row * C4), p = (int)(row % HW);
    const float4 a = *(const float4*)(in + row * ldi + q * 4), k = *(const float4*)(img + ((long)p * C4 + q) * 4);
    *(float4*)(out + row * ldo + q * 4) = make_float4(a.x + k.x, a.y + k.y, a.z + k.z, a.w + k.w);
  }
}
}  // namespace
int launch_add_image_rows(const float* in, int ldi, const float* img, int C, int nb, int HW, float* out, int ldo, hipStream_t s) {
  if ((C & 3) || (ldi & 3) || (ldo & 3) || (((uintptr_t)in | (uintptr_t)img | (uintptr_t)out) & 15))
    return mvd_fail("add_image_rows: 16-byte aligned rows");
  const long total4 = (long)nb * HW * (C / 4);
  if (total4 <= 0) return 0;
  long blocks = (total4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(add_image_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, ldi, img, C / 4, total4, HW, out, ldo);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

namespace {
// nearest x2 upsample + fp16 cast of a channels-last image batch: out[b][y][x][c] = (half) in[b][y >> 1][x >> 1][c]
__global__ __launch_bounds__(256) void upsample2_f16_kernel(const float* __restrict__ in, int ldi, int B, int H, int W, int C4,
                                                            half_t* __restrict__ out) {
  const long total = (long)B * 4 * H * W * C4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i % C4);
    long p = i / C4;
    const int x = (int)(p % (2 * W));
    p /= 2 * W;
    const int y = (int)(p % (2 * H)), b = (int)(p / (2 * H));
    const float4 v = *(const float4*)(in + (((long)b * H + (y >> 1)) * W + (x >> 1)) * ldi + q * 4);
    h4 o;
    o[0] = (half_t)v.x; o[1] = (half_t)v.y; o[2] = (half_t)v.z; o[3] = (half_t)v.w;
    *(h4*)(out + i * 4) = o;
  }
}
}  // namespace
int launch_upsample2_f16(const float* in, int ldi, int B, int H, int W, int C, half_t* out, hipStream_t s) {
  if ((C & 3) || (ldi & 3) || (((uintptr_t)in | (uintptr_t)out) & 15)) return mvd_fail("upsample2_f16: 16-byte aligned rows");
  const long total = (long)B * 4 * H * W * (C / 4);
  if (total <= 0) return 0;
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(upsample2_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, ldi, B, H, W, C / 4, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

namespace {
// The UNet's first convolution in exact fp32 (round 6).  8 (padded) input channels make K = 72: as an MFMA implicit GEMM the layer
// is all operand staging (extended-precision form: a 35 us split cast + a 61 us GEMM for 3 GFLOP).  Here one thread owns one output
// channel and keeps its 72 weights in registers; the image row and its two neighbours (+ the zero halo) sit in LDS and every lane
// reads the same address, so the only vector-memory traffic is the coalesced output rows.  LDS returns 128 B per clock whether or
// not the lanes agree, so the reads are what has to be rationed: four adjacent output pixels share each input column (9 b128 reads
// per pixel instead of 18), which puts the LDS time at the multiply-adds' own.  One workgroup per image row: 1024 groups of 5 waves
// keep the four SIMDs evenly loaded.  Exact fp32 multiply-adds in a fixed order (row-major, column, channel).
// MEASURED (tools/conv_in_prof.py under rocprofv3, 32 samples of 32 x 32, 8 -> 320): 31.8 us per launch, the same as the plain
// fp16 MFMA form (32.2 us) and in front of the extended-precision form it replaces (split cast + 3x-K GEMM); in the step that is
// 0.01-0.04 ms (profiles/r06_zb_ab_conv_in_f32.txt).  Forms that lost: inputs through the scalar cache as SGPR operands (no gain
// in the step at all); 18 reads per pixel with 4 rows per group (LDS-bound).
template <int CIN, int P>  // 4 or 8 input channels (the checkpoint's [N][CIN][3][3] rows); P adjacent pixels per pass (divides W)
__global__ __launch_bounds__(512, 4) void conv_in_f32_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int N, int H, int W,
                                                           float* __restrict__ out, int ldo) {
  extern __shared__ float xs[];  // [3][W + 2][CIN]
  const int b = blockIdx.x / H, y = blockIdx.x % H;
  const int Wp = W + 2;
  for (int i = threadIdx.x; i < 3 * Wp * CIN; i += blockDim.x) {
    const int ch = i % CIN, px = (i / CIN) % Wp - 1, py = y + i / (CIN * Wp) - 1;
    xs[i] = (px >= 0 && px < W && py >= 0 && py < H) ? x[(((long)b * H + py) * W + px) * ldx + ch] : 0.f;
  }
  const int n = threadIdx.x < N ? threadIdx.x : N - 1;
  float wr[9][CIN];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int ch = 0; ch < CIN; ++ch) wr[t][ch] = w[(long)n * CIN * 9 + ch * 9 + t];
  const float bn = bias ? bias[n] : 0.f;
  __syncthreads();
  if (threadIdx.x >= N) return;
  float* orow = out + (((long)b * H + y) * W) * ldo + n;
  for (int px0 = 0; px0 < W; px0 += P) {
    float acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int col = 0; col < P + 2; ++col) {  // input column px0 + col - 1 feeds output pixel px0 + col - dx
        const float4* pv = (const float4*)(xs + (dy * Wp + px0 + col) * CIN);
        float v[CIN];
#pragma unroll
        for (int q = 0; q < CIN / 4; ++q) *(float4*)(v + 4 * q) = pv[q];
#pragma unroll
        for (int dx = 2; dx >= 0; --dx) {
          const int p = col - dx;
          if (p < 0 || p >= P) continue;
#pragma unroll
          for (int ch = 0; ch < CIN; ++ch) acc[p] = fmaf(wr[dy * 3 + dx][ch], v[ch], acc[p]);
        }
        if (col & 1) __builtin_amdgcn_sched_barrier(0);  // at most two columns of reads in flight: 72 weights + 16 stay under 128 VGPRs
      }
#pragma unroll
    for (int p = 0; p < P; ++p) orow[(long)(px0 + p) * ldo] = acc[p] + bn;
  }
}
}  // namespace
int launch_conv_in_f32(const float* x, int ldx, const float* w, int cin_src, const float* bias, int N, int B, int H, int W, float* out,
                       int ldo, hipStream_t s) {
  if ((cin_src != 4 && cin_src != 8) || N < 1 || N > 512) return mvd_fail("conv_in_f32: 4 or 8 input and at most 512 output channels");
  if (((uintptr_t)w) & 15) return mvd_fail("conv_in_f32: 16-byte aligned weights");
  if (B <= 0) return 0;
  const int threads = (N + 63) / 64 * 64;
  const size_t lds = (size_t)3 * (W + 2) * cin_src * sizeof(float);
  if (lds > 64 * 1024) return mvd_fail("conv_in_f32: image row too wide for the LDS strip");
  const dim3 grid((unsigned)(B * H)), block(threads);
  if (cin_src == 8 && W % 4 == 0)
    hipLaunchKernelGGL((conv_in_f32_kernel<8, 4>), grid, block, lds, s, x, ldx, w, bias, N, H, W, out, ldo);
  else if (cin_src == 8)
    hipLaunchKernelGGL((conv_in_f32_kernel<8, 1>), grid, block, lds, s, x, ldx, w, bias, N, H, W, out, ldo);
  else if (W % 4 == 0)
    hipLaunchKernelGGL((conv_in_f32_kernel<4, 4>), grid, block, lds, s, x, ldx, w, bias, N, H, W, out, ldo);
  else
    hipLaunchKernelGGL((conv_in_f32_kernel<4, 1>), grid, block, lds, s, x, ldx, w, bias, N, H, W, out, ldo);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

namespace {
// The UNet's LAST convolution (3 x 3, C -> 4) in exact fp32 (round 6; openaimodel.py:717-721).  Four output columns are 1 / 8 of the
// narrowest MFMA tile and the layer carries a sixth of the end-to-end error variance in fp16, so it ran as an extended-precision
// implicit GEMM: 66 us + a 3x-wide GroupNorm output for 0.75 GFLOP.  Here the activations arrive in fp32 (gn_group_kernel,
// split == 2) and a wave owns 16 adjacent pixels of an image row: lane (p, k) = pixels p and p + 8, every eighth 16-byte channel
// quad (so the eight k-lanes of a pixel read one 128-byte line), 4 outputs x 2 pixels of accumulators, weights [tap][quad][ch][out]
// in LDS (padded so the eight quads of a read land on distinct banks), a 3-step butterfly over k at the end.  Persistent
// workgroups (one per CU) stage the weights once.  Fixed summation order.
__global__ __launch_bounds__(256) void out_conv_f32_kernel(const float* __restrict__ a, int C, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int N, int B, int H, int W,
                                                           float* __restrict__ out, int ldo) {
  extern __shared__ float4 s_w[];  // [9][C / 32][34]: quad 8 j + k, channel i of the quad at (tap * J + j) * 34 + 4 k + (k >> 2) + i
  const int J = C >> 5, tid = threadIdx.x;
  for (int e = tid; e < 9 * C; e += 256) {
    const int t = e / C, c = e - t * C, q = c >> 2, i = c & 3, j = q >> 3, k = q & 7;
    float4 v;
    v.x = N > 0 ? w[((long)0 * C + c) * 9 + t] : 0.f;
    v.y = N > 1 ? w[((long)1 * C + c) * 9 + t] : 0.f;
    v.z = N > 2 ? w[((long)2 * C + c) * 9 + t] : 0.f;
    v.w = N > 3 ? w[((long)3 * C + c) * 9 + t] : 0.f;
    s_w[(t * J + j) * 34 + 4 * k + (k >> 2) + i] = v;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, p = lane & 7, k = lane >> 3;
  const int runs_per_row = W >> 4, total = B * H * runs_per_row;
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    bv.x = N > 0 ? bias[0] : 0.f; bv.y = N > 1 ? bias[1] : 0.f; bv.z = N > 2 ? bias[2] : 0.f; bv.w = N > 3 ? bias[3] : 0.f;
  }
  for (int run = blockIdx.x * 4 + wave; run < total; run += gridDim.x * 4) {
    const int xr = run % runs_per_row, y = (run / runs_per_row) % H, b = run / (runs_per_row * H);
    const int x0 = xr * 16 + p, x1 = x0 + 8;
    float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int py = y + dy - 1;
      if (py < 0 || py >= H) continue;  // wave-uniform
      const float* arow = a + (((long)b * H + py) * W) * C + 4 * k;
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int q0 = x0 + dx - 1, q1 = x1 + dx - 1;
          float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
          if (q0 >= 0 && q0 < W) v0 = *(const float4*)(arow + (long)q0 * C + 32 * j);
          if (q1 >= 0 && q1 < W) v1 = *(const float4*)(arow + (long)q1 * C + 32 * j);
          const float4* wp = s_w + ((dy * 3 + dx) * J + j) * 34 + 4 * k + (k >> 2);
          const float4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
#define MVD_OH(acc, v)                                                                                            \
  acc.x = fmaf(v.x, w0.x, acc.x); acc.y = fmaf(v.x, w0.y, acc.y); acc.z = fmaf(v.x, w0.z, acc.z); acc.w = fmaf(v.x, w0.w, acc.w); \
  acc.x = fmaf(v.y, w1.x, acc.x); acc.y = fmaf(v.y, w1.y, acc.y); acc.z = fmaf(v.y, w1.z, acc.z); acc.w = fmaf(v.y, w1.w, acc.w); \
  acc.x = fmaf(v.z, w2.x, acc.x); acc.y = fmaf(v.z, w2.y, acc.y); acc.z = fmaf(v.z, w2.z, acc.z); acc.w = fmaf(v.z, w2.w, acc.w); \
  acc.x = fmaf(v.w, w3.x, acc.x); acc.y = fmaf(v.w, w3.y, acc.y); acc.z = fmaf(v.w, w3.z, acc.z); acc.w = fmaf(v.w, w3.w, acc.w)
          MVD_OH(acc0, v0);
          MVD_OH(acc1, v1);
#undef MVD_OH
        }
      }
    }
#pragma unroll
    for (int m = 8; m < 64; m <<= 1) {  // over the eight channel-quad lanes of a pixel
      acc0.x += __shfl_xor(acc0.x, m); acc0.y += __shfl_xor(acc0.y, m); acc0.z += __shfl_xor(acc0.z, m); acc0.w += __shfl_xor(acc0.w, m);
      acc1.x += __shfl_xor(acc1.x, m); acc1.y += __shfl_xor(acc1.y, m); acc1.z += __shfl_xor(acc1.z, m); acc1.w += __shfl_xor(acc1.w, m);
    }
    if (k == 0) {
      float* o0 = out + (((long)b * H + y) * W + x0) * ldo;
      float* o1 = out + (((long)b * H + y) * W + x1) * ldo;
      const float r0[4] = {acc0.x + bv.x, acc0.y + bv.y, acc0.z + bv.z, acc0.w + bv.w};
      const float r1[4] = {acc1.x + bv.x, acc1.y + bv.y, acc1.z + bv.z, acc1.w + bv.w};
      for (int o = 0; o < N; ++o) {
        o0[o] = r0[o];
        o1[o] = r1[o];
      }
    }
  }
}
}  // namespace
int launch_out_conv_f32(const float* a, int C, const float* w, const float* bias, int N, int B, int H, int W, float* out, int ldo,
                        hipStream_t s) {
  if (N < 1 || N > 4 || (C & 31) || (W & 15) || C > 512) return mvd_fail("out_conv_f32: N <= 4, C % 32 == 0 (<= 512), W % 16 == 0");
  if (((uintptr_t)a) & 15) return mvd_fail("out_conv_f32: 16-byte aligned activations");
  if (B <= 0) return 0;
  const long runs = (long)B * H * (W / 16);
  long grid = (runs + 3) / 4;
  if (grid > 256) grid = 256;
  const size_t lds = (size_t)9 * (C / 32) * 34 * sizeof(float4);
  hipLaunchKernelGGL(out_conv_f32_kernel, dim3((unsigned)grid), dim3(256), lds, s, a, C, w, bias, N, B, H, W, out, ldo);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
