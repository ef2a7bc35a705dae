// The per-op test and bench hooks of the C ABI (include/mvd.h: "per-op hooks") that need no file-local function of another
// translation unit; the backward, adjoint and gather hooks are at the end of engine_train.hip.  Both build on hooks.h.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "hooks.h"
#include "rowchain.h"

namespace {

__global__ void split_rows_to_f32_kernel(const half_t* in, int rows, int C, float* out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)rows * C; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / C, c = i % C;
    const half_t hi = in[r * 3 * C + c], lo = in[r * 3 * C + C + c], h2 = in[r * 3 * C + 2 * C + c];
    out[i] = (float)hi == (float)h2 ? (float)hi + (float)lo : __builtin_nanf("");
  }
}
// fp32 [rows][C] -> fp16 rows ldo halfs apart (the pad columns are left as they are), and the reverse from rows ldi apart
__global__ void rows_f32_to_f16_ld_kernel(const float* in, size_t rows, int C, half_t* out, int ldo) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * C; i += (size_t)gridDim.x * blockDim.x)
    out[(i / C) * ldo + i % C] = (half_t)in[i];
}
// fp32 rows ldi floats apart -> 16-bit rows ldo apart (the pad columns of both are left as they are)
__global__ void rows_f32_ld_to_f16_ld_kernel(const float* in, int ldi, size_t rows, int C, half_t* out, int ldo) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * C; i += (size_t)gridDim.x * blockDim.x)
    out[(i / C) * ldo + i % C] = (half_t)in[(i / C) * ldi + i % C];
}
__global__ void rows_f16_ld_to_f32_kernel(const half_t* in, size_t rows, int C, int ldi, float* out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * C; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (float)in[(i / C) * ldi + i % C];
}
// q,k,v [B][T][C] fp32 -> the fused 16-bit image [B][Tstride][ld] (q | k | v in the first 3 C columns); what lies between is left as it is
__global__ void pack_qkv_image_kernel(const float* q, const float* k, const float* v, int B, int T, int C, int Tstride, int ld, half_t* qkv) {
  const long total = (long)B * T * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long r = i / C, row = (r / T) * Tstride + r % T;
    qkv[row * ld + c] = (half_t)q[i];
    qkv[row * ld + C + c] = (half_t)k[i];
    qkv[row * ld + 2 * C + c] = (half_t)v[i];
  }
}
__global__ void fill_pattern_f16_kernel(half_t* p, size_t n, unsigned seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = (half_t)(((float)(h & 0xFFFF) / 32768.0f) - 1.0f);
  }
}

inline hipStream_t S(void* s) { return (hipStream_t)s; }

}  // namespace

extern "C" {

// ---- parity hooks of the sparse voxel CNN (tests/test_gpu_sparse_cnn_ops.py): no context, the caller's device buffers, scratch and
// weight packs that live for the call (freed after the stream has been synchronised)
namespace {
struct OpScratch {
  std::vector<void*> bufs;
  ~OpScratch() {
    for (void* b : bufs) hipFree(b);
  }
  // elems of 4 bytes; poison: 0xFF bytes (NaN as a float, -1 as an int) before use
  int get(size_t elems, bool poison, hipStream_t s, void** out) {
    void* b = nullptr;
    if (hipMalloc(&b, std::max<size_t>(elems, 1) * 4) != hipSuccess) return mvd_fail("parity hook: scratch allocation failed");
    bufs.push_back(b);
    if (poison && hipMemsetAsync(b, 0xFF, std::max<size_t>(elems, 1) * 4, s) != hipSuccess) return mvd_fail("parity hook: memset failed");
    *out = b;
    return 0;
  }
};
int sparse_op_check(const char* who, int n_out, int Cin, int Cout, int layout, int form) {
  const std::string w(who);
  if (n_out <= 0 || Cin <= 0 || Cout <= 0 || Cin > 256 || Cout > 256) return mvd_fail((w + ": row or channel count out of range").c_str());
  if (layout < 0 || layout > 2) return mvd_fail((w + ": weight layout 0..2").c_str());
  if (form != 0 && form != 1) return mvd_fail((w + ": form 0 (site) or 1 (matrix-core)").c_str());
  if (form == 1 && !sparse_mfma_takes(Cin, Cout)) return mvd_fail((w + ": no matrix-core kernel for these channel counts").c_str());
  return 0;
}
}  // namespace

int mvd_op_sparse_conv(const float* in, const int32_t* nbr, int n_out, int Cin, int Cout, const float* w, int layout, const float* scale,
                       const float* shift, int form, float* out, void* stream) {
  if (!in || !nbr || !w || !out || !scale != !shift) return mvd_fail("mvd_op_sparse_conv: null argument");
  RET_IF(sparse_op_check("mvd_op_sparse_conv", n_out, Cin, Cout, layout, form));
  hipStream_t s = S(stream);
  OpScratch z;
  const size_t nw = (size_t)27 * Cin * Cout;
  float *wpk = nullptr, *wp = nullptr;
  RET_IF(z.get(nw, false, s, (void**)&wpk));
  if (form == 1) RET_IF(z.get(nw, false, s, (void**)&wp));
  int rc = launch_sparse_w_pack(w, Cin, Cout, layout, wpk, s);
  if (!rc && wp) rc = launch_sparse_w_frag(wpk, Cin, Cout, 0, 0, wp, s);
  if (!rc) rc = launch_sparse_conv(in, nbr, n_out, Cin, Cout, wpk, wp, scale, shift, out, s);
  return hook_sync("mvd_op_sparse_conv", s, rc);
}

int mvd_op_bn_rows_relu(const float* x, int n, int C, const float* gamma, const float* beta, float eps, float momentum, float* y,
                        float* stats_out, float* rmean, float* rvar, void* stream) {
  if (!x || !y || !gamma || !beta || !rmean != !rvar) return mvd_fail("mvd_op_bn_rows_relu: null argument");
  if (n <= 0 || C <= 0) return mvd_fail("mvd_op_bn_rows_relu: row or channel count out of range");
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_bn_rows_relu", s, launch_bn_rows_relu(x, y, n, C, gamma, beta, eps, stats_out, s, rmean, rvar, momentum));
}

int mvd_op_bn_rows_relu_bwd(const float* xraw, float* dy, int n, int C, const float* gamma, const float* beta, const float* stats,
                            int poison, float* dgamma, float* dbeta, void* stream) {
  if (!xraw || !dy || !gamma || !beta || !stats || !dgamma || !dbeta) return mvd_fail("mvd_op_bn_rows_relu_bwd: null argument");
  if (n <= 0 || C <= 0) return mvd_fail("mvd_op_bn_rows_relu_bwd: row or channel count out of range");
  if (C > 256 || 256 % C) return mvd_fail("mvd_op_bn_rows_relu_bwd: the channel count must divide 256");
  hipStream_t s = S(stream);
  OpScratch z;
  float* part = nullptr;
  RET_IF(z.get((size_t)cbwd_bn_scratch_floats(n, C), poison != 0, s, (void**)&part));
  return hook_sync("mvd_op_bn_rows_relu_bwd", s, cbwd_bn_rows_relu(xraw, dy, n, C, gamma, beta, stats, part, dgamma, dbeta, s));
}

int mvd_op_sparse_conv_bwd(const float* in, const int32_t* nbr, float* d_out, int n_in, int n_out, int Cin, int Cout, int strided,
                           int level0_subm, int deterministic, int form, const float* w, int layout, int poison, float* d_in, float* gw,
                           void* stream) {
  if (!in || !nbr || !d_out || !w || !d_in || !gw) return mvd_fail("mvd_op_sparse_conv_bwd: null argument");
  RET_IF(sparse_op_check("mvd_op_sparse_conv_bwd", n_out, Cin, Cout, layout, form));
  if (n_in <= 0) return mvd_fail("mvd_op_sparse_conv_bwd: row or channel count out of range");
  if (strided && level0_subm) return mvd_fail("mvd_op_sparse_conv_bwd: level0_subm is a submanifold layer");
  if (!strided && n_in != n_out) return mvd_fail("mvd_op_sparse_conv_bwd: a submanifold layer has n_in == n_out");
  if (form == 0 && deterministic) return mvd_fail("mvd_op_sparse_conv_bwd: the site form's data gradient adds with fp32 atomics");
  hipStream_t s = S(stream);
  const bool mfma = form == 1, lvl0 = mfma && level0_subm != 0, det = deterministic != 0;
  const SparseLayerScratch q = cbwd_sparse_layer_scratch(n_in, n_out, Cin, Cout, strided != 0, lvl0, det, mfma);
  OpScratch z;
  const size_t nw = (size_t)27 * Cin * Cout;
  float *wpk = nullptr, *wd = nullptr, *dwp = nullptr, *dw_part = nullptr;
  int *flag = nullptr, *inv = nullptr;
  RET_IF(z.get(nw, false, s, (void**)&wpk));
  if (mfma) RET_IF(z.get(nw, false, s, (void**)&wd));
  RET_IF(z.get(q.dwp, poison != 0, s, (void**)&dwp));
  RET_IF(z.get(q.dw_part, poison != 0, s, (void**)&dw_part));
  if (q.flag) RET_IF(z.get(q.flag, poison != 0, s, (void**)&flag));
  if (q.inv) RET_IF(z.get(q.inv, poison != 0, s, (void**)&inv));
  int rc = launch_sparse_w_pack(w, Cin, Cout, layout, wpk, s);  // the packs of build_sparse_layer (engine_weights.hip)
  if (!rc && mfma) rc = launch_sparse_w_frag(wpk, Cout, Cin, 1, strided ? 0 : 1, wd, s);
  if (!rc)
    rc = cbwd_sparse_layer(in, nbr, d_out, n_in, n_out, Cin, Cout, strided != 0, lvl0, det, wpk, wd, layout, dwp, dw_part, flag, inv, d_in,
                           gw, s);
  return hook_sync("mvd_op_sparse_conv_bwd", s, rc);
}

// ------------------------------------------------------------------------------------------ the asynchronous hooks
// tests/test_gpu_ops.py, tests/test_gpu_train_ops.py, tools/race_micro.py: operands in the reference's layouts, staged in the
// workspace; the launches are enqueued on the caller's stream and the call returns WITHOUT synchronising it, so these run beside
// work on another stream (the synchronous, argument-checking forms are the *_ex hooks further down)
int mvd_op_conv(mvd_ctx* c, const float* x_nchw, int B, int Cin, int H, int W, const float* w, const float* bias, int Cout,
                int ksize, int stride, int upsample, const float* resid_nchw, float* out_nchw, int force_splitk,
                void* stream) {
  RET_IF(hook_begin(c));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int cpad = (Cin + 7) / 8 * 8, taps = ksize * ksize;
  const int Hv = H << upsample, Wv = W << upsample;
  const int Ho = (Hv - 1) / stride + 1, Wo = (Wv - 1) / stride + 1;
  float* xn = ws_alloc<float>(c, (size_t)B * H * W * cpad);
  float* on = ws_alloc<float>(c, (size_t)B * Ho * Wo * Cout);
  float* rn = resid_nchw ? ws_alloc<float>(c, (size_t)B * Ho * Wo * Cout) : nullptr;
  WS_CHECK(xn && on);
  RET_IF(launch_nchw_to_nhwc(x_nchw, B, Cin, H * W, xn, cpad, cpad, s));
  ConvW cw;
  RET_IF(hook_pack_fwd(c, w, Cout, Cin, taps, 0, 0, 0, &cw, s));
  cw.bias = const_cast<float*>(bias);
  if (rn) RET_IF(launch_nchw_to_nhwc(resid_nchw, B, Cout, Ho * Wo, rn, Cout, Cout, s));
  if (force_splitk == -3) {  // the UNet's last layer at inference: exact fp32 on the vector ALU (launch_out_conv_f32)
    if (taps != 9 || stride != 1 || upsample || rn || cpad != Cin) return mvd_fail("op_conv: the fp32 output-head form is 3x3, stride 1, no residual");
    RET_IF(launch_out_conv_f32(xn, Cin, w, bias, Cout, B, H, W, on, Cout, s));
    RET_IF(launch_nhwc_to_nchw(on, Cout, B, Cout, Ho * Wo, out_nchw, s));
    return 0;
  }
  if (force_splitk == -2) {  // the UNet's first layer at inference: exact fp32 on the vector ALU (launch_conv_in_f32)
    if (taps != 9 || stride != 1 || upsample || rn) return mvd_fail("op_conv: the fp32 first-layer form is 3x3, stride 1, no residual");
    RET_IF(launch_conv_in_f32(xn, cpad, w, Cin, bias, Cout, B, H, W, on, Cout, s));
    RET_IF(launch_nhwc_to_nchw(on, Cout, B, Cout, Ho * Wo, out_nchw, s));
    return 0;
  }
  GemmArgs g;
  g.a = xn; g.a_f32 = 1; g.lda = cpad; g.w = &cw; g.out = on; g.ldc = Cout; g.resid = rn; g.ldr = Cout;
  g.use_bias = bias != nullptr; g.force_splitk = force_splitk;
  if (cpad % 64 == 0) {  // exercise the fp16-source paths (incl. the LDS-halo 3x3 kernels) the UNet uses
    const half_t* xh;
    RET_IF(hook_f16(c, xn, (size_t)B * H * W * cpad, &xh, s));
    g.a = xh;
    g.a_f32 = 0;
    const int bnx = Cout % 160 == 0 ? 160 : (Cout % 128 == 0 ? 128 : 0);
    if (taps == 9 && bnx && mvd_env_call::conv3x()) {  // ... and the conv3x form of the weights (k_conv3x.hip), as build_conv3x_streams does
      cw.wx = ws_alloc<half_t>(c, conv3x_stream_halfs(Cout, cpad, bnx));
      WS_CHECK(cw.wx);
      RET_IF(conv3x_pack(cw.w, Cout, cpad, bnx, cw.wx, s));
      cw.wx_bn = bnx;
    }
  }
  if (upsample && taps == 9 && stride == 1 && cpad == Cin && B * H * W >= 2048) {
    // the UNet's path for large upsample convs: four parity-folded 2x2 convs (fp32 source, as in the decoder)
    cw.w_up = ws_alloc<half_t>(c, (size_t)16 * Cout * Cin);
    WS_CHECK(cw.w_up);
    RET_IF(launch_pack_upconv_weight(w, Cout, Cin, cw.w_up, s));
    g.a = xn; g.a_f32 = 1;
    RET_IF(run_upconv2d(c, g, B, H, W, s));
  } else {
    RET_IF(run_conv2d(c, g, B, H, W, stride, upsample, s));
  }
  RET_IF(launch_nhwc_to_nchw(on, Cout, B, Cout, Ho * Wo, out_nchw, s));
  return 0;
}

int mvd_op_conv3d(mvd_ctx* c, const float* x, int B, int Cin, int D, int H, int W, const float* w, const float* bias,
                  int Cout, int stride, int transposed, const float* resid, float* out, void* stream) {
  RET_IF(hook_begin(c));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  if (Cin % 8) return mvd_fail("op_conv3d: Cin must be a multiple of 8");
  const int Do = transposed ? 2 * D : (D - 1) / stride + 1, Ho = transposed ? 2 * H : (H - 1) / stride + 1,
            Wo = transposed ? 2 * W : (W - 1) / stride + 1;
  float* xn = ws_alloc<float>(c, (size_t)B * D * H * W * Cin);
  float* on = ws_alloc<float>(c, (size_t)B * Do * Ho * Wo * Cout);
  WS_CHECK(xn && on);
  RET_IF(launch_nchw_to_nhwc(x, B, Cin, D * H * W, xn, Cin, Cin, s));
  ConvW cw;
  RET_IF(hook_pack_fwd(c, w, Cout, Cin, 27, transposed, 0, 0, &cw, s));
  cw.bias = const_cast<float*>(bias);
  if (resid) RET_IF(launch_nchw_to_nhwc(resid, B, Cout, Do * Ho * Wo, on, Cout, Cout, s));
  GemmArgs g;
  g.a = xn; g.a_f32 = 1; g.lda = Cin; g.w = &cw; g.out = on; g.ldc = Cout; g.use_bias = bias != nullptr;
  if (resid) { g.resid = on; g.ldr = Cout; }
  if (Cin % 64 == 0) {  // fp16-source path (LDS-DMA implicit GEMM), as in the frustum network's inner layers
    const half_t* xh;
    RET_IF(hook_f16(c, xn, (size_t)B * D * H * W * Cin, &xh, s));
    g.a = xh;
    g.a_f32 = 0;
  }
  if (transposed) RET_IF(run_convT3d(c, g, B, D, H, W, s));
  else RET_IF(run_conv3d(c, g, B, D, H, W, stride, s));
  RET_IF(launch_nhwc_to_nchw(on, Cout, B, Cout, Do * Ho * Wo, out, s));
  return 0;
}

int mvd_op_linear(mvd_ctx* c, const float* a, int M, int K, const float* w, const float* bias, int N, int geglu,
                  const float* resid, int a_half, int force_splitk, float* out, void* stream) {
  RET_IF(hook_begin(c));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  if (K % 8) return mvd_fail("op_linear: K must be a multiple of 8");
  ConvW cw;
  RET_IF(hook_pack_fwd(c, w, N, K, 1, 0, geglu, 0, &cw, s));
  float* bp = ws_alloc<float>(c, (size_t)N);
  WS_CHECK(bp);
  if (bias) {
    if (geglu) RET_IF(launch_permute_geglu_bias(bias, N, bp, s));
    else HIP_CHECK_RET(hipMemcpyAsync(bp, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
  }
  cw.bias = bias ? bp : nullptr;
  GemmArgs g;
  g.a = a; g.a_f32 = 1; g.lda = K; g.w = &cw; g.out = out; g.ldc = geglu ? N / 2 : N; g.geglu = geglu;
  g.use_bias = bias != nullptr;
  g.force_splitk = force_splitk;
  if (resid) {
    g.resid = resid; g.resid_f32 = 1; g.ldr = N;
  }
  if (a_half) {
    const half_t* ah;
    RET_IF(hook_f16(c, a, (size_t)M * K, &ah, s));
    g.a = ah; g.a_f32 = 0;
  }
  RET_IF(run_linear(c, g, 1, M, s));
  return 0;
}

int mvd_op_group_norm(mvd_ctx* c, const float* x_nchw, int B, int C, int HW, int groups, const float* gamma,
                      const float* beta, float eps, int act, float* out_nchw, void* stream) {
  RET_IF(hook_begin(c));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  float* xn = ws_alloc<float>(c, (size_t)B * HW * C);
  half_t* y = ws_alloc<half_t>(c, (size_t)B * HW * C);
  float* yf = ws_alloc<float>(c, (size_t)B * HW * C);
  WS_CHECK(xn && y && yf);
  RET_IF(launch_nchw_to_nhwc(x_nchw, B, C, HW, xn, C, C, s));
  NormW n;
  n.g = const_cast<float*>(gamma); n.b = const_cast<float*>(beta); n.C = C;
  RET_IF(run_group_norm(c, xn, C, B, HW, n, groups, eps, act, nullptr, y, C, s));
  hook_f16_to_f32(y, yf, (size_t)B * HW * C, s);
  HIP_CHECK_RET(hipGetLastError());
  RET_IF(launch_nhwc_to_nchw(yf, C, B, C, HW, out_nchw, s));
  return 0;
}

// depth_attn_kernel on the caller's data (tests/test_gpu_depth_attn.py).  Everything the launch may touch is poisoned first: the
// context's pad columns (ldx > Cc) and one guard row behind z hold 0xFFFF halfs, NaN in fp16 and in bfloat16.
int mvd_op_depth_attn(mvd_ctx* c, const float* qk, const float* context, const float* fill_row, int n_cond, int HW, int D, int Cc,
                      int heads, int ldx, int split, int nfill, int check_only, float* out, float* hi_out, void* stream) {
  RET_IF(hook_begin(c));
  if (depth_attn_check(D, Cc, heads, ldx, nfill)) return -1;  // the launcher's own refusals, before anything is sized by them
  if (check_only) return 0;
  if (n_cond < 0 || HW <= 0 || D <= 0 || Cc <= 0 || !out || (n_cond > 0 && (!qk || !context)) || (nfill > 0 && !fill_row))
    return mvd_fail("op_depth_attn: bad argument");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  if (ldx == 0) ldx = Cc;
  split = split ? 1 : 0;
  const int W4 = 4 * Cc, wz = split ? 3 : 1;
  const size_t npix = (size_t)n_cond * HW, rows = npix + nfill, crows = npix * D;
  half_t* cn = ws_alloc<half_t>(c, crows * ldx + 8);
  half_t* z = ws_alloc<half_t>(c, (rows + 1) * W4 * wz);
  half_t* fr = ws_alloc<half_t>(c, (size_t)W4 * 3);
  WS_CHECK(cn && z && fr);
  HIP_CHECK_RET(hipMemsetAsync(cn, 0xFF, (crows * ldx + 8) * sizeof(half_t), s));
  HIP_CHECK_RET(hipMemsetAsync(z, 0xFF, (rows + 1) * W4 * wz * sizeof(half_t), s));
  if (crows) hipLaunchKernelGGL(rows_f32_to_f16_ld_kernel, dim3(hook_blocks(crows * Cc)), dim3(256), 0, s, context, crows, Cc, cn, ldx);
  if (nfill > 0) {
    if (split) RET_IF(launch_rows_f32_to_f16_split(fill_row, W4, 1, W4, fr, s));
    else RET_IF(launch_f32_to_f16(fill_row, fr, W4, s));
  }
  RET_IF(launch_depth_attn(qk, cn, z, n_cond, HW, D, Cc, heads, s, split, nfill, nfill > 0 ? fr : nullptr, ldx));
  const size_t n = (rows + 1) * W4;
  if (split) {  // the guard row's three blocks are all NaN: NaN != NaN, so it comes back NaN
    hipLaunchKernelGGL(split_rows_to_f32_kernel, dim3(hook_blocks(n)), dim3(256), 0, s, z, (int)(rows + 1), W4, out);
    if (hi_out) hipLaunchKernelGGL(rows_f16_ld_to_f32_kernel, dim3(hook_blocks(n)), dim3(256), 0, s, z, rows + 1, W4, 3 * W4, hi_out);
  } else {
    hook_f16_to_f32(z, out, n, s);
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// The training backward's reductions one launch at a time (tests/test_gpu_norm_bwd_ops.py); the norm hooks themselves are at the end
// of engine_train.hip.  Result buffers are the caller's (0xFF presets, guard rows), arguments are checked before any launch.
int mvd_op_train_colsum(mvd_ctx* c, const float* v, int src_f16, int ld, int B, int rows, int C, float* out, int ldo, void* stream) {
  RET_IF(hook_begin(c));
  if (!v || !out || B <= 0 || rows <= 0 || C <= 0 || ld < C || ldo < C) return mvd_fail("op_train_colsum: bad argument");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const void* src = v;
  if (src_f16) {
    const half_t* h;
    RET_IF(hook_f16(c, v, (size_t)B * rows * ld, &h, s));
    src = h;
  }
  return hook_sync("op_train_colsum", s, bwd_colsum_samples(src, src_f16 ? 0 : 1, ld, B, rows, C, out, ldo, s));
}

int mvd_op_train_sum_rows(mvd_ctx* c, int n, const float* const* part, const int* R, const int* C, const long* ldp, float* const* out,
                          const int* accum, void* stream) {
  RET_IF(hook_begin(c));
  if (!part || !R || !C || !ldp || !out || !accum) return mvd_fail("op_train_sum_rows: bad argument");
  for (int k = 0; k < n && k < 4; ++k)
    if (!part[k] || !out[k] || R[k] <= 0 || C[k] <= 0 || ldp[k] < C[k]) return mvd_fail("op_train_sum_rows: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("op_train_sum_rows", s, bwd_sum_rows_multi(n, part, R, C, ldp, out, accum, s));
}

int mvd_op_train_outer_add(mvd_ctx* c, const float* a, int lda, const float* b, int ldb, float* out, int M, int N, int K, void* stream) {
  RET_IF(hook_begin(c));
  if (!a || !b || !out || M <= 0 || N <= 0 || K <= 0 || lda < M || ldb < N) return mvd_fail("op_train_outer_add: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("op_train_outer_add", s, bwd_outer_add(a, lda, b, ldb, out, M, N, K, s));
}

int mvd_bench_conv(mvd_ctx* c, int B, int C, int H, int W, int Cout, int iters, float* ms_out, void* stream) {
  RET_IF(hook_begin(c));
  if (!ms_out) return mvd_fail("mvd_bench_conv: null ms_out");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const size_t na = (size_t)B * H * W * C, nw = (size_t)9 * Cout * C;
  half_t* a = ws_alloc<half_t>(c, na);
  half_t* w = ws_alloc<half_t>(c, nw);
  float* o = ws_alloc<float>(c, (size_t)B * H * W * Cout);
  WS_CHECK(a && w && o);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(hook_blocks(na)), dim3(256), 0, s, a, na, 17u);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(hook_blocks(nw)), dim3(256), 0, s, w, nw, 91u);
  ConvW cw;
  cw.w = w; cw.N = Cout; cw.Cin = C; cw.taps = 9;
  const int bnx = Cout % 160 == 0 ? 160 : (Cout % 128 == 0 ? 128 : 0);
  if (C % 64 == 0 && bnx && mvd_env_call::conv3x()) {
    cw.wx = ws_alloc<half_t>(c, conv3x_stream_halfs(Cout, C, bnx));
    WS_CHECK(cw.wx);
    RET_IF(conv3x_pack(w, Cout, C, bnx, cw.wx, s));
    cw.wx_bn = bnx;
  }
  GemmArgs g;
  g.a = a; g.lda = C; g.w = &cw; g.out = o; g.ldc = Cout; g.use_bias = false;
  RET_IF(run_conv2d(c, g, B, H, W, 1, 0, s));  // warm-up
  return hook_time(s, iters, [&] { return run_conv2d(c, g, B, H, W, 1, 0, s); }, ms_out);
}

int mvd_bench_linear(mvd_ctx* c, int M, int K, int N, int flags, int iters, float* ms_out, void* stream) {
  RET_IF(hook_begin(c));
  if (!ms_out) return mvd_fail("mvd_bench_linear: null ms_out");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const size_t na = (size_t)M * K, nw = (size_t)N * K, no = (size_t)M * N;
  const bool cold = flags & 32;  // evict the operands (L2 + memory-side cache) before every timed launch
  const size_t flush_bytes = cold ? (size_t)768 << 20 : 0;
  half_t* a = ws_alloc<half_t>(c, na);
  half_t* w = ws_alloc<half_t>(c, nw);
  float* o = ws_alloc<float>(c, no);
  float* r = ws_alloc<float>(c, no);
  float* bias = ws_alloc<float>(c, (size_t)N + 64 * (size_t)N);
  char* flush = cold ? ws_alloc<char>(c, flush_bytes) : nullptr;
  float* a32 = (flags & 64) ? ws_alloc<float>(c, na) : nullptr;  // fp32 activations (converted while staged)
  WS_CHECK(a && w && o && r && bias && (!cold || flush) && (!(flags & 64) || a32));
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(hook_blocks(na)), dim3(256), 0, s, a, na, 17u);
  if (a32) hook_f16_to_f32(a, a32, na, s);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(hook_blocks(nw)), dim3(256), 0, s, w, nw, 91u);
  HIP_CHECK_RET(hipMemsetAsync(r, 0, no * sizeof(float), s));
  HIP_CHECK_RET(hipMemsetAsync(bias, 0, ((size_t)N + 64 * (size_t)N) * sizeof(float), s));
  ConvW cw;
  cw.w = w; cw.N = N; cw.Cin = K; cw.taps = 1; cw.bias = bias;
  GemmArgs g;
  g.a = a; g.lda = K; g.w = &cw; g.out = o; g.use_bias = (flags & 8) != 0;
  if (a32) { g.a = a32; g.a_f32 = 1; }
  g.geglu = (flags & 4) ? 1 : 0;
  g.ldc = g.geglu ? N / 2 : N;
  g.out_f32 = (flags & 2) ? 0 : 1;
  if (flags & 1) { g.resid = r; g.resid_f32 = 1; g.ldr = N; }
  const int nb = M % 32 == 0 ? 32 : 1;  // samples (per-sample bias rows)
  if (flags & 16) { g.rowbias = bias + N; g.rb_ld = N; }
  RET_IF(run_linear(c, g, nb, M, s));  // warm-up
  const auto launch = [&] { return run_linear(c, g, nb, M, s); };
  if (!cold) return hook_time(s, iters, launch, ms_out);
  HookTimer timer;  // each launch timed on its own, behind the flush
  float total = 0.f;
  for (int i = 0; i < iters; ++i) {
    HIP_CHECK_RET(hipMemsetAsync(flush, i & 0xFF, flush_bytes, s));
    RET_IF(timer.run(s, 1, launch, &total));
  }
  *ms_out = total / (float)iters;
  return 0;
}

int mvd_bench_group_norm(mvd_ctx* c, int B, int C, int HW, int groups, int flags, int iters, float* ms_out, void* stream) {
  RET_IF(hook_begin(c));
  if (!ms_out) return mvd_fail("mvd_bench_group_norm: null ms_out");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const size_t n = (size_t)B * HW * C;
  const int split = flags & 1, wo = split ? 3 : 1;
  float* x = ws_alloc<float>(c, n);
  half_t* tmp = ws_alloc<half_t>(c, n);
  half_t* y = ws_alloc<half_t>(c, n * wo);
  float* gb = ws_alloc<float>(c, (size_t)2 * C);
  WS_CHECK(x && tmp && y && gb);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(hook_blocks(n)), dim3(256), 0, s, tmp, n, 29u);
  hook_f16_to_f32(tmp, x, n, s);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(hook_blocks((size_t)2 * C)), dim3(256), 0, s, tmp, (size_t)2 * C, 5u);
  hook_f16_to_f32(tmp, gb, (size_t)2 * C, s);
  NormW nw;
  nw.g = gb; nw.b = gb + C; nw.C = C;
  RET_IF(run_group_norm(c, x, C, B, HW, nw, groups, 1e-5f, ACT_SILU, nullptr, y, C * wo, s, 0, split));  // warm-up
  // flags & 2: the APPLY pass alone (statistics given): what a GroupNorm costs once its statistics come out of the producer's epilogue
  float* partial = nullptr;
  int nslabs = 0;
  if (flags & 2) {
    partial = ws_alloc<float>(c, (size_t)B * gn_max_slabs() * groups * 2);
    WS_CHECK(partial);
    RET_IF(launch_gn_stats(x, C, B, HW, C, groups, nullptr, 0, partial, &nslabs, s));
  }
  return hook_time(s, iters, [&] {
    if (flags & 2) return launch_gn_apply(x, C, B, HW, C, groups, nullptr, 0, partial, nslabs, nw.g, nw.b, 1e-5f, ACT_SILU, y, C * wo, s, split);
    return run_group_norm(c, x, C, B, HW, nw, groups, 1e-5f, ACT_SILU, nullptr, y, C * wo, s, 0, split);
  }, ms_out);
}

// The row-chain kernel (k_rowchain.hip) on fp32 operands in the reference's layouts: packs the weight stream, runs the kernel
// once (iters > 0: `iters` more times between two events -> *ms_out = mean milliseconds) and returns the result in fp32.
int mvd_op_st_tail(mvd_ctx* c, int C, int rows, int T, const float* ao, const float* xin, const float* rowbias, const float* w_ao,
                   const float* b_ao, const float* ln_g, const float* ln_b, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w_po, const float* b_po, const float* resid, float* out, int flags, int iters,
                   float* ms_out, void* stream) {
  RET_IF(hook_begin(c));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int has_ao = flags & 1, has_po = (flags & 2) ? ((flags & 8) ? 2 : 1) : 0, split = (flags & 4) && !has_po;
  if (!rowchain_takes(C, rows, T)) return mvd_fail("op_st_tail: shape not supported by the row-chain kernel");
  const size_t n = (size_t)rows * C;
  half_t* stream_w = ws_alloc<half_t>(c, rowchain_stream_halfs(C, has_ao, has_po));
  float* tmp = ws_alloc<float>(c, (size_t)8 * C);
  half_t* aoh = has_ao ? ws_alloc<half_t>(c, n) : nullptr;
  half_t* oh = has_po ? nullptr : ws_alloc<half_t>(c, n * (split ? 3 : 1));
  WS_CHECK(stream_w && tmp && (!has_ao || aoh) && (has_po || oh));
  RcWeights w;
  w.w_ao = w_ao; w.ln_g = ln_g; w.ln_b = ln_b; w.w1 = w1; w.b1 = b1; w.w2 = w2; w.b2 = b2; w.w_po = w_po;
  RET_IF(rowchain_pack(w, C, has_ao, has_po, tmp, stream_w, s));
  if (has_ao) RET_IF(launch_f32_to_f16(ao, aoh, n, s));
  RowChain p;
  memset(&p, 0, sizeof p);
  p.stream = stream_w; p.rows = rows; p.T = T;
  p.ao = aoh; p.ld_ao = C; p.xin = xin; p.ld_x = C; p.b_ao = b_ao; p.rowbias = rowbias; p.rb_ld = C;
  p.b_po = b_po; p.resid = resid; p.ld_r = C;
  p.out = has_po ? (void*)out : (void*)oh; p.ld_o = has_po ? C : (split ? 3 * C : C); p.out_split = split ? C : 0;
  RET_IF(launch_rowchain(p, C, has_ao, has_po, s));
  if (iters > 0) {
    float ms = 0.f;
    RET_IF(hook_time(s, iters, [&] { return launch_rowchain(p, C, has_ao, has_po, s); }, &ms));
    if (ms_out) *ms_out = ms;
  }
  if (!has_po) {
    if (split) {  // [hi | lo | hi] rows -> hi + lo (NaN where the third block differs from the first)
      hipLaunchKernelGGL(split_rows_to_f32_kernel, dim3(hook_blocks(n)), dim3(256), 0, s, oh, rows, C, out);
    } else {
      hook_f16_to_f32(oh, out, n, s);
    }
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// The row-head kernel (k_rowchain.hip: proj_in -> t0, LayerNorm1, q | k | v) on fp32 operands in the reference's layouts, C = 320.
int mvd_op_st_head(mvd_ctx* c, int rows, int xp, const float* n0, const float* w_pi, const float* b_pi, const float* ln_g, const float* ln_b,
                   const float* w_q, const float* w_k, const float* w_v, float* t0_out, float* qkv_out, int iters, float* ms_out,
                   void* stream) {
  RET_IF(hook_begin(c));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int C = RH_C;
  const size_t n = (size_t)rows * C;
  half_t* stream_w = ws_alloc<half_t>(c, rowhead_stream_halfs(xp));
  float* tmp = ws_alloc<float>(c, (size_t)3 * C);
  half_t* n0h = ws_alloc<half_t>(c, n * (xp ? 3 : 1));
  half_t* qkvh = ws_alloc<half_t>(c, 3 * n);
  WS_CHECK(stream_w && tmp && n0h && qkvh);
  RhWeights w;
  w.w_pi = w_pi; w.ln_g = ln_g; w.ln_b = ln_b; w.w_q = w_q; w.w_k = w_k; w.w_v = w_v;
  RET_IF(rowhead_pack(w, xp, tmp, stream_w, s));
  if (xp) RET_IF(launch_rows_f32_to_f16_split(n0, C, rows, C, n0h, s));  // [hi | lo | hi] rows, as the GroupNorm's split mode writes
  else RET_IF(launch_f32_to_f16(n0, n0h, n, s));
  RowHead p;
  p.stream = stream_w; p.rows = rows; p.n0 = n0h; p.ld_n0 = xp ? 3 * C : C; p.b_pi = b_pi; p.t0 = t0_out; p.ld_t0 = C; p.qkv = qkvh; p.ld_qkv = 3 * C;
  RET_IF(launch_rowhead(p, xp, s));
  if (iters > 0) {
    float ms = 0.f;
    RET_IF(hook_time(s, iters, [&] { return launch_rowhead(p, xp, s); }, &ms));
    if (ms_out) *ms_out = ms;
  }
  hook_f16_to_f32(qkvh, qkv_out, 3 * n, s);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------- forward-form hooks
// tests/test_gpu_epilogue_forms.py: the forward kernels in the forms the inference path and the first-stage model launch them in
// (every GemmArgs field, extended precision, deferred split-K and its consumers, the folded GroupNorm, the row softmax).
// Operands are fp32 in the reference's layouts (activations channels-last); the production launch writes straight into the
// caller's result buffers, which the caller presets to 0xFF bytes with a guard row (and pad columns) behind what may be written.
// Arguments are checked before anything is allocated or launched; poison != 0 fills the free workspace (everything the launch
// allocates for itself: split-K slabs, operand copies) with 0xFF bytes once the operands are staged; the stream is synchronised.
namespace {
// the epilogue fields shared by mvd_op_linear_ex and mvd_op_conv_ex
struct ExEpi {
  const float *bias, *rowbias, *resid;
  int rb_ld, act, use_bias, out_f16, out_split, ldc, resid_f16, ldr, force_splitk;
  float alpha;
  float* slabs;
  size_t slabs_cap;
  int defer_epilogue;
  int* sk_used;
  void* out;
};
// rb_unaligned_ok: per-sample rows of any stride (a plain GEMM then runs on the gather kernel with its element-wise epilogue)
int ex_epi_check(const char* who, const ExEpi& e, int N, bool rb_unaligned_ok = false) {
  const std::string w(who);
  if (!e.out) return mvd_fail((w + ": null result").c_str());
  if (N <= 0 || (N & 3)) return mvd_fail((w + ": N must be a positive multiple of 4").c_str());
  if (e.act != ACT_NONE && e.act != ACT_SILU) return mvd_fail((w + ": act is 0 (none) or 1 (SiLU)").c_str());
  if (!(e.alpha == e.alpha) || e.alpha - e.alpha != 0.0f) return mvd_fail((w + ": alpha must be finite").c_str());
  if (e.use_bias && !e.bias) return mvd_fail((w + ": use_bias without a bias").c_str());
  if (e.rowbias && (e.rb_ld < N || (!rb_unaligned_ok && (e.rb_ld & 3)))) return mvd_fail((w + ": rb_ld must be a multiple of 4, >= N").c_str());
  if (e.resid && (e.ldr < N || (e.ldr & 3))) return mvd_fail((w + ": ldr must be a multiple of 4, >= N").c_str());
  if (e.out_split && !e.out_f16) return mvd_fail((w + ": out_split is a form of the fp16 result").c_str());
  if ((e.ldc & 3) || e.ldc < (e.out_split ? 3 : 1) * N) return mvd_fail((w + ": ldc must be a multiple of 4, >= N (3 N with out_split)").c_str());
  if (e.force_splitk < 0) return mvd_fail((w + ": force_splitk >= 0").c_str());
  if (e.slabs && !e.sk_used) return mvd_fail((w + ": a slab buffer needs sk_used").c_str());
  if (e.slabs && ((uintptr_t)e.slabs & 15)) return mvd_fail((w + ": the slab buffer must be 16-byte aligned").c_str());
  if ((uintptr_t)e.out & 15) return mvd_fail((w + ": the result must be 16-byte aligned").c_str());
  return 0;
}
// fills the GemmArgs from the checked fields; an fp16 residual is staged from the caller's fp32 rows
int ex_epi_fill(mvd_ctx* c, const ExEpi& e, size_t out_rows, int N, GemmArgs& g, hipStream_t s) {
  g.out = e.out; g.out_f32 = e.out_f16 ? 0 : 1; g.ldc = e.ldc; g.out_split = e.out_split ? N : 0;
  g.rowbias = e.rowbias; g.rb_ld = e.rb_ld; g.alpha = e.alpha; g.act = e.act; g.use_bias = e.use_bias != 0;
  g.force_splitk = e.force_splitk;
  if (e.resid) {
    g.resid = e.resid; g.resid_f32 = 1; g.ldr = e.ldr;
    if (e.resid_f16) {
      const half_t* rh;
      RET_IF(hook_f16(c, e.resid, out_rows * e.ldr, &rh, s));
      g.resid = rh; g.resid_f32 = 0;
    }
  }
  if (e.slabs) {
    g.slabs = e.slabs; g.slabs_cap = e.slabs_cap; g.sk_used = e.sk_used; g.defer_epilogue = e.defer_epilogue != 0;
  }
  return 0;
}
}  // namespace

int mvd_op_linear_ex(mvd_ctx* c, const float* a, int B, int rows, int K, const float* w, const float* bias, int N, const float* rowbias,
                     int rb_ld, float alpha, int act, int use_bias, int out_f16, int out_split, int ldc, const float* resid,
                     int resid_f16, int ldr, int a_half, int force_splitk, int xp, float* slabs, size_t slabs_cap, int defer_epilogue,
                     int* sk_used, int poison, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!a || !w) return mvd_fail("op_linear_ex: null operand");
  if (B <= 0 || rows <= 0 || rows % B || K <= 0 || (K & 7)) return mvd_fail("op_linear_ex: rows % B == 0 and K % 8 == 0 expected");
  const ExEpi e{bias, rowbias, resid, rb_ld, act, use_bias, out_f16, out_split, ldc, resid_f16, ldr, force_splitk, alpha,
                slabs, slabs_cap, defer_epilogue, sk_used, out};
  RET_IF(ex_epi_check("op_linear_ex", e, N, true));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int Kp = xp ? 3 * K : K;
  ConvW cw;
  RET_IF(hook_pack_fwd(c, w, N, K, 1, 0, 0, xp, &cw, s));
  cw.bias = const_cast<float*>(bias);
  GemmArgs g;
  g.a = a; g.a_f32 = 1; g.lda = K; g.w = &cw;
  if (xp || a_half) {
    half_t* ah = ws_alloc<half_t>(c, (size_t)rows * Kp);
    WS_CHECK(ah);
    if (xp) RET_IF(launch_rows_f32_to_f16_split(a, K, rows, K, ah, s));  // [a_hi | a_lo | a_hi]
    else RET_IF(launch_f32_to_f16(a, ah, (size_t)rows * K, s));
    g.a = ah; g.a_f32 = 0; g.lda = Kp;
  }
  RET_IF(ex_epi_fill(c, e, (size_t)rows, N, g, s));
  if (sk_used) *sk_used = 1;
  if (poison) RET_IF(hook_poison(c, s));
  return hook_sync("op_linear_ex", s, run_linear(c, g, B, rows, s));
}

// x / resid / out channels-last ([B][H][W][Cin], [B][Ho][Wo][ldr], [B*Ho*Wo + 1][ldc]); w [Cout][Cin][k][k].  tap_shift = 1 is the
// first-stage encoder's Downsample (zero padding on the right and bottom only): 3x3, stride 2, EVEN H and W only -- the encoder
// never runs it otherwise, and for an odd side the output grid of F.pad(x, (0, 1, 0, 1)) + conv(k3, s2, p0) is not run_conv2d's.
// upsample: the fused nearest x2 (run_conv2d), or with up_fold != 0 the four parity-folded 2x2 convolutions (run_upconv2d).
int mvd_op_conv_ex(mvd_ctx* c, const float* x, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout, int ksize,
                   int stride, int upsample, int up_fold, int tap_shift, const float* rowbias, int rb_ld, float alpha, int act,
                   int use_bias, int out_f16, int out_split, int ldc, const float* resid, int resid_f16, int ldr, int a_half,
                   int force_splitk, int xp, int conv3x_stream, float* slabs, size_t slabs_cap, int defer_epilogue, int* sk_used,
                   int poison, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!x || !w) return mvd_fail("op_conv_ex: null operand");
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 7)) return mvd_fail("op_conv_ex: Cin % 8 == 0 expected");
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || (upsample != 0 && upsample != 1))
    return mvd_fail("op_conv_ex: 1x1 or 3x3, stride 1 or 2, upsample 0 or 1");
  if (tap_shift != 0 && (tap_shift != 1 || ksize != 3 || stride != 2 || upsample || (H & 1) || (W & 1)))
    return mvd_fail("op_conv_ex: tap_shift = 1 is the 3x3 stride-2 Downsample of even H and W");
  if (up_fold && (!upsample || ksize != 3 || stride != 1 || xp || slabs))
    return mvd_fail("op_conv_ex: the parity-folded form is a 3x3 stride-1 upsample conv without xp or a slab buffer");
  const ExEpi e{bias, rowbias, resid, rb_ld, act, use_bias, out_f16, out_split, ldc, resid_f16, ldr, force_splitk, alpha,
                slabs, slabs_cap, defer_epilogue, sk_used, out};
  RET_IF(ex_epi_check("op_conv_ex", e, Cout));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int taps = ksize * ksize, Cp = xp ? 3 * Cin : Cin;
  const int Ho = ((H << upsample) - 1) / stride + 1, Wo = ((W << upsample) - 1) / stride + 1;
  const size_t rows_in = (size_t)B * H * W, rows_out = (size_t)B * Ho * Wo;
  ConvW cw;
  RET_IF(hook_pack_fwd(c, w, Cout, Cin, taps, 0, 0, xp, &cw, s));
  cw.bias = const_cast<float*>(bias);
  GemmArgs g;
  g.a = x; g.a_f32 = 1; g.lda = Cin; g.w = &cw; g.tap_shift = tap_shift;
  if (xp || a_half) {
    half_t* xh = ws_alloc<half_t>(c, rows_in * Cp);
    WS_CHECK(xh);
    if (xp) RET_IF(launch_rows_f32_to_f16_split(x, Cin, (long)rows_in, Cin, xh, s));
    else RET_IF(launch_f32_to_f16(x, xh, rows_in * Cin, s));
    g.a = xh; g.a_f32 = 0; g.lda = Cp;
  }
  const int bnx = Cout % 160 == 0 ? 160 : (Cout % 128 == 0 ? 128 : 0);
  if (conv3x_stream && taps == 9 && bnx && Cp % 64 == 0 && !g.a_f32) {  // the weights as a conv3x fragment stream too (k_conv3x.hip)
    cw.wx = ws_alloc<half_t>(c, conv3x_stream_halfs(Cout, Cp, bnx));
    WS_CHECK(cw.wx);
    RET_IF(conv3x_pack(cw.w, Cout, Cp, bnx, cw.wx, s));
    cw.wx_bn = bnx;
  }
  if (up_fold) {
    cw.w_up = ws_alloc<half_t>(c, (size_t)16 * Cout * Cin);
    WS_CHECK(cw.w_up);
    RET_IF(launch_pack_upconv_weight(w, Cout, Cin, cw.w_up, s));
  }
  RET_IF(ex_epi_fill(c, e, rows_out, Cout, g, s));
  if (sk_used) *sk_used = 1;
  if (poison) RET_IF(hook_poison(c, s));
  return hook_sync("op_conv_ex", s, up_fold ? run_upconv2d(c, g, B, H, W, s) : run_conv2d(c, g, B, H, W, stride, upsample, s));
}

// tests/test_gpu_conv3d_forms.py: run_conv3d / run_convT3d in the forms the two 3-D U-nets launch them in.  x [B][D][H][W][Cin],
// resid [rows][ldr] on the output grid, out [rows + 1][ldc] (fp32, or 16-bit with out_f16); w [Cout][Cin][27], transposed:
// [Cin][Cout][27].  in_place: the residual image is copied into the result buffer (rounded to 16 bits with out_f16) and the launch
// reads it from there, as the up path does where xf_l == xd_l.
// form (tests/test_gpu_conv3d_halo.py): 0 = the kernel igemm_go picks, 1 = conv3z (k_conv3x.hip) whatever the row count.
static int conv3d_hook(const char* who, mvd_ctx* c, const float* x, int B, int D, int H, int W, int Cin, const float* w, const float* bias,
                       int Cout, int stride, int transposed, int use_bias, const float* resid, int ldr, int in_place, int out_f16, int ldc,
                       int a_half, int force_splitk, int form, int poison, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (form != 0 && form != 1) return mvd_fail("op_conv3d_form: form must be 0 or 1");
  if (form == 1 && (transposed || stride != 1)) return mvd_fail("op_conv3d_form: form 1 (conv3z) is a stride-1 convolution");
  if (!x || !w || !out) return mvd_fail("op_conv3d_ex: null operand");
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 7)) return mvd_fail("op_conv3d_ex: Cin % 8 == 0 expected");
  if (Cout <= 0 || (Cout & 3)) return mvd_fail("op_conv3d_ex: Cout must be a positive multiple of 4");
  if ((transposed != 0 && transposed != 1) || (stride != 1 && stride != 2) || (transposed && stride != 1))
    return mvd_fail("op_conv3d_ex: stride 1 or 2, or transposed (with stride 1)");
  if (use_bias && !bias) return mvd_fail("op_conv3d_ex: use_bias without a bias");
  if (resid && (ldr < Cout || (ldr & 3))) return mvd_fail("op_conv3d_ex: ldr must be a multiple of 4, >= Cout");
  if (in_place && !resid) return mvd_fail("op_conv3d_ex: in_place needs a residual");
  if ((ldc & 3) || ldc < Cout) return mvd_fail("op_conv3d_ex: ldc must be a multiple of 4, >= Cout");
  if (force_splitk < 0) return mvd_fail("op_conv3d_ex: force_splitk >= 0");
  if ((uintptr_t)out & 15) return mvd_fail("op_conv3d_ex: the result must be 16-byte aligned");
  const int Do = transposed ? 2 * D : (D - 1) / stride + 1, Ho = transposed ? 2 * H : (H - 1) / stride + 1,
            Wo = transposed ? 2 * W : (W - 1) / stride + 1;
  const size_t rows_in = (size_t)B * D * H * W, rows_out = (size_t)B * Do * Ho * Wo;
  if (rows_out > (size_t)1 << 24 || rows_out * (size_t)ldc > (size_t)1 << 30 || rows_in * (size_t)Cin > (size_t)1 << 30)
    return mvd_fail("op_conv3d_ex: at most 2^24 output rows and 2^30 elements per image");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  ConvW cw;
  RET_IF(hook_pack_fwd(c, w, Cout, Cin, 27, transposed, 0, 0, &cw, s));
  cw.bias = const_cast<float*>(bias);
  const int bnz = transposed || stride != 1 ? 0 : conv3z_stream_bn(27, Cout, Cin);
  if (bnz && mvd_env_call::conv3x()) {  // ... and the conv3z form of the weights, as pack_conv3z_stream does
    cw.wx = ws_alloc<half_t>(c, conv3z_stream_halfs(Cout, Cin, bnz));
    WS_CHECK(cw.wx);
    RET_IF(conv3z_pack(cw.w, Cout, Cin, bnz, cw.wx, s));
    cw.wx_bn = bnz;
  }
  GemmArgs g;
  g.a = x; g.a_f32 = 1; g.lda = Cin; g.w = &cw; g.out = out; g.out_f32 = out_f16 ? 0 : 1; g.ldc = ldc;
  g.use_bias = use_bias != 0; g.force_splitk = force_splitk;
  if (a_half) {
    const half_t* xh;
    RET_IF(hook_f16(c, x, rows_in * Cin, &xh, s));
    g.a = xh; g.a_f32 = 0;
  }
  if (resid) {
    g.resid = resid; g.resid_f32 = 1; g.ldr = ldr;
    if (in_place) {
      if (out_f16) {
        hipLaunchKernelGGL(rows_f32_ld_to_f16_ld_kernel, dim3(hook_blocks(rows_out * Cout)), dim3(256), 0, s, resid, ldr, rows_out, Cout,
                           (half_t*)out, ldc);
        HIP_CHECK_RET(hipGetLastError());
      } else {
        HIP_CHECK_RET(hipMemcpy2DAsync(out, (size_t)ldc * 4, resid, (size_t)ldr * 4, (size_t)Cout * 4, rows_out, hipMemcpyDeviceToDevice, s));
      }
      g.resid = out; g.resid_f32 = out_f16 ? 0 : 1; g.ldr = ldc;
    }
  }
  if (poison) RET_IF(hook_poison(c, s));
  return hook_sync(who, s, transposed ? run_convT3d(c, g, B, D, H, W, s) : run_conv3d(c, g, B, D, H, W, stride, s, form));
}
int mvd_op_conv3d_ex(mvd_ctx* c, const float* x, int B, int D, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                     int stride, int transposed, int use_bias, const float* resid, int ldr, int in_place, int out_f16, int ldc,
                     int a_half, int force_splitk, int poison, void* out, void* stream) {
  return conv3d_hook("op_conv3d_ex", c, x, B, D, H, W, Cin, w, bias, Cout, stride, transposed, use_bias, resid, ldr, in_place, out_f16, ldc,
                     a_half, force_splitk, 0, poison, out, stream);
}
int mvd_op_conv3d_form(mvd_ctx* c, const float* x, int B, int D, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                       int stride, int transposed, int use_bias, const float* resid, int ldr, int in_place, int out_f16, int ldc,
                       int a_half, int force_splitk, int form, int poison, void* out, void* stream) {
  return conv3d_hook("op_conv3d_form", c, x, B, D, H, W, Cin, w, bias, Cout, stride, transposed, use_bias, resid, ldr, in_place, out_f16,
                     ldc, a_half, force_splitk, form, poison, out, stream);
}
// The form igemm_go gives a stride-1 / stride-2 3x3x3 layer whose weights carry every stream the engine packs for them: 0 = the
// kernels of before, 1 = conv3z; transposed layers: 0.  Evaluates the routing predicate (conv3z_routed) alone: no context, no device --
// and so not the gate igemm_go puts in front of it (env.conv3x && c->use_halo; training contexts pack no stream): the answer is
// that of an inference context with its default switches.
int mvd_conv3d_routed_form(int B, int D, int H, int W, int Cin, int Cout, int stride, int transposed, int a_half, int out_f16, int ldc,
                           int has_resid, int resid_f16, int ldr, int force_splitk) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2)) return mvd_fail("conv3d_routed_form: bad shape");
  if (transposed) return 0;
  static const half_t some = (half_t)0.f;  // never read: only "there is a stream" is asked
  ConvW cw;
  cw.N = Cout; cw.Cin = Cin; cw.taps = 27;
  cw.wx_bn = stride == 1 ? conv3z_stream_bn(27, Cout, Cin) : 0;
  cw.wx = cw.wx_bn ? const_cast<half_t*>(&some) : nullptr;
  GemmArgs g;
  g.a = &some; g.a_f32 = a_half ? 0 : 1; g.lda = Cin; g.w = &cw; g.out_f32 = out_f16 ? 0 : 1; g.ldc = ldc; g.force_splitk = force_splitk;
  if (has_resid) { g.resid = &some; g.resid_f32 = resid_f16 ? 0 : 1; g.ldr = ldr; }
  return conv3d_routed_form(g, B, D, H, W, stride);
}

// x: nslab slabs of channels-last [B][rows][ld] fp32, slab_stride floats apart.  form 0: run_group_norm's own choice; form 1: the
// two-pass pair (launch_gn_stats + launch_gn_apply) called directly, which takes one slab and writes neither `mat` nor fp32.
// out: [B * rows + 1][ldo] halfs (split = 1: [hi | lo | hi] rows; split = 2: fp32 rows of ldo / 2 floats); mat: [B * rows + 1][ldm].
int mvd_op_group_norm_ex(mvd_ctx* c, const float* x, int B, int rows, int C, int ld, int groups, const float* gamma, const float* beta,
                         float eps, int act, int form, const float* preadd, int pld, int split, int nslab, size_t slab_stride,
                         const float* bias2, const float* resid, int ldr, float* mat, int ldm, int ldo, int poison, void* out,
                         void* stream) {
  RET_IF(hook_begin(c));
  if (!x || !gamma || !beta || !out) return mvd_fail("op_group_norm_ex: null operand");
  if (B <= 0 || rows <= 0 || C <= 0 || groups <= 0 || C % groups || ld < C) return mvd_fail("op_group_norm_ex: C % groups == 0 and ld >= C expected");
  if (act < ACT_NONE || act > ACT_RELU || (form != 0 && form != 1) || split < 0 || split > 2) return mvd_fail("op_group_norm_ex: act 0..2, form 0..1, split 0..2");
  if (ldo < (split == 1 ? 3 : (split == 2 ? 2 : 1)) * C) return mvd_fail("op_group_norm_ex: ldo >= C halfs (3 C with split = 1, 2 C with split = 2)");
  if (nslab < 1 || (nslab > 1 && slab_stride < (size_t)B * rows * ld)) return mvd_fail("op_group_norm_ex: slabs overlap");
  if (preadd && pld < C) return mvd_fail("op_group_norm_ex: pld >= C expected");
  if ((resid && ldr < C) || (mat && ldm < C)) return mvd_fail("op_group_norm_ex: ldr, ldm >= C expected");
  const bool one_pass = !mvd_env().gn_two_pass && gn_group_eligible(ld, rows, C, groups, preadd ? pld : 0, ldo);
  if ((form == 1 || !one_pass) && (nslab > 1 || bias2 || resid || mat || split == 2))
    return mvd_fail("op_group_norm_ex: slabs, bias2, resid, mat and the fp32 result need the single-pass form");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  NormW n;
  n.g = const_cast<float*>(gamma); n.b = const_cast<float*>(beta); n.C = C;
  half_t* o = (half_t*)out;
  if (form == 0) {
    if (poison) RET_IF(hook_poison(c, s));
    return hook_sync("op_group_norm_ex", s,
                   run_group_norm(c, x, ld, B, rows, n, groups, eps, act, preadd, o, ldo, s, pld, split, nslab, slab_stride, bias2, resid,
                                  ldr, mat, ldm));
  }
  if (C > 2560 || groups > 32 || (C & 3) || (ld & 3) || (ldo & 3) || (preadd && (pld & 3)))
    return mvd_fail("op_group_norm_ex: the two-pass form takes C <= 2560, groups <= 32 and C, ld, ldo, pld % 4 == 0");
  float* partial = ws_alloc<float>(c, (size_t)B * gn_max_slabs() * groups * 2);
  WS_CHECK(partial);
  if (poison) RET_IF(hook_poison(c, s));
  int nsl = 0;
  int rc = launch_gn_stats(x, ld, B, rows, C, groups, preadd, pld, partial, &nsl, s);
  if (!rc) rc = launch_gn_apply(x, ld, B, rows, C, groups, preadd, pld, partial, nsl, gamma, beta, eps, act, o, ldo, s, split);
  return hook_sync("op_group_norm_ex", s, rc);
}

// plain == 0: launch_layernorm_slabs with every LnSlabs field (mat [rows + 1][C] is required); plain != 0: launch_layernorm on
// one slab, where only the fp16 copy `raw` ([rows + 1][ld_raw] halfs, may be NULL) is left of them.  out: [rows + 1][C] halfs.
int mvd_op_layer_norm_slabs(mvd_ctx* c, const float* slabs, int nslab, size_t slab_stride, int rows, int C, const float* bias,
                            const float* rowbias, int rb_ld, int T, const float* resid, int ldr, const float* gamma, const float* beta,
                            float eps, int plain, int ld_raw, int poison, float* mat, void* raw, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!slabs || !gamma || !beta || !out) return mvd_fail("op_layer_norm_slabs: null operand");
  if (rows <= 0 || C <= 0 || nslab < 1 || T < 1) return mvd_fail("op_layer_norm_slabs: bad argument");
  if (raw && ld_raw < C) return mvd_fail("op_layer_norm_slabs: ld_raw >= C expected");
  hipStream_t s = S(stream);
  if (plain) {
    if (nslab != 1 || bias || rowbias || resid || mat) return mvd_fail("op_layer_norm_slabs: the plain LayerNorm takes one slab and writes no mat");
    if (poison) RET_IF(hook_poison(c, s));
    return hook_sync("op_layer_norm_slabs", s, launch_layernorm(slabs, rows, C, gamma, beta, eps, (half_t*)out, s, (half_t*)raw, ld_raw));
  }
  if (!mat) return mvd_fail("op_layer_norm_slabs: mat is required");
  if (nslab > 1 && slab_stride < (size_t)rows * C) return mvd_fail("op_layer_norm_slabs: slabs overlap");
  if ((rowbias && rb_ld < C) || (resid && ldr < C)) return mvd_fail("op_layer_norm_slabs: rb_ld, ldr >= C expected");
  if (poison) RET_IF(hook_poison(c, s));
  return hook_sync("op_layer_norm_slabs", s,
                 launch_layernorm_slabs(slabs, nslab, slab_stride, rows, C, bias, rowbias, rb_ld, T, resid, ldr, mat, gamma, beta, eps,
                                        (half_t*)out, s, (half_t*)raw, ld_raw));
}

// The three steps of the folded GroupNorm(proj_context(volume)) (engine_unet.hip: ctx_fold) on caller data: x [B * rps][K], w [N][K],
// N / cpg groups.  partials [B * rps / 256 + 1][N / cpg][2], scale and shift [B + 1][N], out [B * rps + 1][N] halfs.
int mvd_op_folded_group_norm(mvd_ctx* c, const float* x, int B, int rps, int K, const float* w, int N, int cpg, const float* gamma,
                             const float* beta, float eps, int poison, float* partials, float* scale, float* shift, void* out,
                             void* stream) {
  RET_IF(hook_begin(c));
  if (!x || !w || !gamma || !beta || !partials || !scale || !shift || !out) return mvd_fail("op_folded_group_norm: null operand");
  if (B <= 0 || rps <= 0 || K <= 0 || (K & 7) || N <= 0 || (N & 3)) return mvd_fail("op_folded_group_norm: K % 8 == 0 and N % 4 == 0 expected");
  // what ctx_fold_ok asks of a context level
  if (rps % 256 || (cpg != 8 && cpg != 16 && cpg != 32) || (long)B * rps < 512)
    return mvd_fail("op_folded_group_norm: rps % 256 == 0, 8 / 16 / 32 channels per group and at least 512 rows expected");
  if (N % cpg || N / cpg > 32) return mvd_fail("op_folded_group_norm: at most 32 whole groups expected");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int rows = B * rps, G = N / cpg, ntile = rps / 256;
  ConvW cw;
  RET_IF(hook_pack_fwd(c, w, N, K, 1, 0, 0, 0, &cw, s));
  const half_t* xh;
  RET_IF(hook_f16(c, x, (size_t)rows * K, &xh, s));
  if (poison) RET_IF(hook_poison(c, s));
  GemmArgs g;
  g.a = xh; g.lda = K; g.w = &cw; g.use_bias = false; g.gn_partial = partials; g.gn_cpg = cpg; g.force_splitk = 1;
  int rc = run_linear(c, g, B, rows, s);
  if (!rc) rc = launch_gn_finalize(partials, B, ntile, rps, N, G, gamma, beta, eps, scale, shift, N, s);
  if (!rc) {
    g = GemmArgs();
    g.a = xh; g.lda = K; g.w = &cw; g.use_bias = false; g.out = out; g.out_f32 = 0; g.ldc = N;
    g.rowscale = scale; g.rs_ld = N; g.rowbias = shift; g.rb_ld = N; g.act = ACT_RELU; g.force_splitk = 1;
    rc = run_linear(c, g, B, rows, s);
  }
  return hook_sync("op_folded_group_norm", s, rc);
}

// softmax_rows_kernel (out_f32 == 0: fp16 probabilities) / softmax_rows_f32_kernel on [rows][cols] fp32 scores; out [rows + 1][cols]
int mvd_op_softmax_rows(mvd_ctx* c, const float* scores, int rows, int cols, int out_f32, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!scores || !out || rows <= 0 || cols <= 0) return mvd_fail("op_softmax_rows: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("op_softmax_rows", s,
                 out_f32 ? launch_softmax_rows_f32(scores, rows, cols, (float*)out, s) : launch_softmax_rows(scores, rows, cols, (half_t*)out, s));
}

// launch_rows_f32_to_f16_split: fp32 rows `lda` floats apart -> [hi | lo | hi] rows of 3 C halfs; out [rows + 1][3 C]
int mvd_op_rows_split(mvd_ctx* c, const float* x, int lda, int rows, int C, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!x || !out || rows <= 0 || C <= 0 || lda < C) return mvd_fail("op_rows_split: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("op_rows_split", s, launch_rows_f32_to_f16_split(x, lda, rows, C, (half_t*)out, s));
}


// tests/test_gpu_attention.py: attn_kernel and the two backward kernels on the engine's images, with everything the launches may touch
// beside their operands and results poisoned first (0xFFFF is NaN in fp16 and in bfloat16)
namespace {
int attn_ex_check(const char* who, const void* q, const void* k, const void* v, int B, int T, int heads, int d) {
  const std::string w(who);
  if (!q || !k || !v) return mvd_fail((w + ": null operand").c_str());
  if (B < 1 || T < 1 || heads < 1) return mvd_fail((w + ": B, T, heads >= 1 expected").c_str());
  if (d != 8 && d != 16 && d != 32 && d != 40 && d != 64 && d != 80 && d != 160) return mvd_fail((w + ": unsupported head dim").c_str());
  return 0;
}
// rows of [dq | dk | dv], 3 C floats each -> the three [rows][C] results
hipError_t hook_unpack_qkv(const float* dqkv, size_t rows, int C, float* dq, float* dk, float* dv, hipStream_t s) {
  float* outs[3] = {dq, dk, dv};
  for (int i = 0; i < 3; ++i) {
    const hipError_t e = hipMemcpy2DAsync(outs[i], (size_t)C * 4, dqkv + (size_t)i * C, (size_t)3 * C * 4, (size_t)C * 4, rows, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
}  // namespace

int mvd_op_attention_ex(mvd_ctx* c, const float* q, const float* k, const float* v, int B, int T, int heads, int d, int Tstride,
                        int ld_pad, int xcd, float* out, void* stream) {
  RET_IF(hook_begin(c));
  RET_IF(attn_ex_check("op_attention_ex", q, k, v, B, T, heads, d));
  if (!out) return mvd_fail("op_attention_ex: null operand");
  if (Tstride < 0 || (Tstride != 0 && Tstride < T)) return mvd_fail("op_attention_ex: Tstride >= T (or 0) expected");
  if (ld_pad < 0 || ld_pad % 8) return mvd_fail("op_attention_ex: ld_pad must be a multiple of 8");
  if (xcd < -1 || xcd > 1) return mvd_fail("op_attention_ex: xcd is -1, 0 or 1");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int C = heads * d, ld = 3 * C + ld_pad, Ts = Tstride ? Tstride : T;
  const size_t rows = (size_t)B * Ts + 1;
  half_t* qkv = ws_alloc<half_t>(c, rows * ld);
  half_t* o = ws_alloc<half_t>(c, rows * C);
  WS_CHECK(qkv && o);
  HIP_CHECK_RET(hipMemsetAsync(qkv, 0xFF, rows * ld * sizeof(half_t), s));
  HIP_CHECK_RET(hipMemsetAsync(o, 0xFF, rows * C * sizeof(half_t), s));
  hipLaunchKernelGGL(pack_qkv_image_kernel, dim3(hook_blocks((size_t)B * T * C)), dim3(256), 0, s, q, k, v, B, T, C, Ts, ld, qkv);
  int rc = launch_attention(qkv, ld, qkv + 2 * C, ld, o, C, B, T, heads, d, s, Ts, xcd);
  if (!rc) {
    hook_f16_to_f32(o, out, rows * C, s);
    if (hipGetLastError() != hipSuccess) rc = mvd_fail("op_attention_ex: launch failed");
  }
  return hook_sync("op_attention_ex", s, rc);
}

int mvd_op_attention_bwd_ex(mvd_ctx* c, const float* q, const float* k, const float* v, const float* d_out, int B, int T, int heads,
                            int d, float* dq, float* dk, float* dv, float* lse, float* delta, float* o_out, void* stream) {
  RET_IF(hook_begin(c));
  RET_IF(attn_ex_check("op_attention_bwd_ex", q, k, v, B, T, heads, d));
  if (!d_out || !dq || !dk || !dv || !lse || !delta || !o_out) return mvd_fail("op_attention_bwd_ex: null operand");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int C = heads * d;
  const size_t rows = (size_t)B * T, nstat = (size_t)B * heads * T + 1;
  half_t* qkv = ws_alloc<half_t>(c, (rows + 1) * 3 * C);
  half_t* o = ws_alloc<half_t>(c, (rows + 1) * C);
  half_t* do16 = ws_alloc<half_t>(c, (rows + 1) * C);
  half_t* dqkv = ws_alloc<half_t>(c, (rows + 1) * 3 * C);
  float* lse_d = ws_alloc<float>(c, nstat);
  float* delta_d = ws_alloc<float>(c, nstat);
  float* tmp = ws_alloc<float>(c, (rows + 1) * 3 * C);
  WS_CHECK(qkv && o && do16 && dqkv && lse_d && delta_d && tmp);
  HIP_CHECK_RET(hipMemsetAsync(qkv, 0xFF, (rows + 1) * 3 * C * sizeof(half_t), s));
  HIP_CHECK_RET(hipMemsetAsync(o, 0xFF, (rows + 1) * C * sizeof(half_t), s));
  HIP_CHECK_RET(hipMemsetAsync(do16, 0xFF, (rows + 1) * C * sizeof(half_t), s));
  HIP_CHECK_RET(hipMemsetAsync(dqkv, 0xFF, (rows + 1) * 3 * C * sizeof(half_t), s));
  HIP_CHECK_RET(hipMemsetAsync(lse_d, 0xFF, nstat * sizeof(float), s));
  HIP_CHECK_RET(hipMemsetAsync(delta_d, 0xFF, nstat * sizeof(float), s));
  hipLaunchKernelGGL(pack_qkv_image_kernel, dim3(hook_blocks(rows * C)), dim3(256), 0, s, q, k, v, B, T, C, T, 3 * C, qkv);
  int rc = launch_attention(qkv, 3 * C, qkv + 2 * C, 3 * C, o, C, B, T, heads, d, s);
  if (!rc) rc = bwd_cast_rows(d_out, C, (long)rows, C, C, do16, s);
  if (!rc) rc = bwd_attention(qkv, 3 * C, o, do16, C, dqkv, 3 * C, lse_d, delta_d, B, T, heads, d, s);
  if (!rc) {
    hook_f16_to_f32(dqkv, tmp, (rows + 1) * 3 * C, s);
    hook_f16_to_f32(o, o_out, (rows + 1) * C, s);
    if (hipGetLastError() != hipSuccess) rc = mvd_fail("op_attention_bwd_ex: launch failed");
    if (!rc && hook_unpack_qkv(tmp, rows + 1, C, dq, dk, dv, s) != hipSuccess) rc = mvd_fail("op_attention_bwd_ex: copy failed");
    if (!rc && (hipMemcpyAsync(lse, lse_d, nstat * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
                hipMemcpyAsync(delta, delta_d, nstat * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess))
      rc = mvd_fail("op_attention_bwd_ex: copy failed");
  }
  return hook_sync("op_attention_bwd_ex", s, rc);
}

// the DepthTransformer's fp32 training kernels (csrc/k_train.hip) on the caller's device buffers; no context
int mvd_op_train_depth_attn(const float* q, const float* k, const float* v, int R, int HW, int D, int hn, int hd, float* attn, float* z,
                            void* stream) {
  if (!q || !k || !v || !attn || !z) return mvd_fail("mvd_op_train_depth_attn: null argument");
  if (R <= 0 || HW <= 0 || R % HW || D <= 0 || hn <= 0 || hd <= 0) return mvd_fail("mvd_op_train_depth_attn: R a positive multiple of HW, D, hn, hd >= 1 expected");
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_train_depth_attn", s, train_depth_fwd(q, k, v, R, HW, D, hn, hd, 1.0f / sqrtf((float)hd), attn, z, s));
}

int mvd_op_train_depth_attn_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dz, int R, int HW, int D,
                                int hn, int hd, float* dq, float* dk, float* dv, void* stream) {
  if (!q || !k || !v || !attn || !dz || !dq || !dk || !dv) return mvd_fail("mvd_op_train_depth_attn_bwd: null argument");
  if (R <= 0 || HW <= 0 || R % HW || D <= 0 || hn <= 0 || hd <= 0) return mvd_fail("mvd_op_train_depth_attn_bwd: R a positive multiple of HW, D, hn, hd >= 1 expected");
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_train_depth_attn_bwd", s,
                 train_depth_bwd(q, k, v, attn, dz, R, HW, D, hn, hd, 1.0f / sqrtf((float)hd), dq, dk, dv, s));
}

int mvd_op_train_im2col3(const float* x, int B, int H, int W, int C, float* col, void* stream) {
  if (!x || !col || B <= 0 || H <= 0 || W <= 0 || C <= 0) return mvd_fail("mvd_op_train_im2col3: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_train_im2col3", s, train_im2col3(x, B, H, W, C, col, s));
}

int mvd_op_train_col2im3(const float* dcol, int B, int H, int W, int C, float* dx, void* stream) {
  if (!dcol || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0) return mvd_fail("mvd_op_train_col2im3: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_train_col2im3", s, train_col2im3(dcol, B, H, W, C, dx, s));
}

int mvd_op_train_perm_w3(const float* src, int N, int C, int to_mat, float* dst, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0) return mvd_fail("mvd_op_train_perm_w3: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_train_perm_w3", s, train_perm_w3(src, N, C, to_mat, dst, s));
}

// ---------------------------------------------------------------------------------------------- small-op hooks
// tests/test_gpu_small_ops.py: the kernels of k_misc.hip and k_enc.hip, the element-wise kernels of k_cond.hip and the samplers'
// batch assembly, one production launcher per call on the caller's buffers (0xFF presets, guard rows, pad columns).  Every
// argument is checked before anything is allocated or launched; the stream is synchronised before the call returns.

// launch_target_encoder without a context's weights: w[0] [16][4][3][3], w[1..7] [16][16][3][3] fp32, packed here as pack_conv
// does (launch_pack_weight, the init conv with cin_src = 4 into Cin = 8); bias[8], gamma[7], beta[7] of 16 floats; x [n][4][32][32],
// pre [n][48]; feats [n * 1024 (+ guard)][16]
int mvd_op_target_encoder(mvd_ctx* c, const float* x, const float* pre, int n_views, const float* const* w, const float* const* bias,
                          const float* const* gamma, const float* const* beta, float* feats, void* stream) {
  RET_IF(hook_begin(c));
  if (!x || !pre || !w || !bias || !gamma || !beta || !feats) return mvd_fail("op_target_encoder: null argument");
  if (n_views < 1 || n_views > 4096) return mvd_fail("op_target_encoder: 1 .. 4096 views expected");
  for (int i = 0; i < 8; ++i)
    if (!w[i] || !bias[i] || (i < 7 && (!gamma[i] || !beta[i]))) return mvd_fail("op_target_encoder: null layer parameter");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const half_t* wp[8];
  int cin[8];
  for (int i = 0; i < 8; ++i) {
    ConvW cw;
    RET_IF(hook_pack_fwd(c, w[i], 16, i ? 16 : 4, 9, 0, 0, 0, &cw, s));
    wp[i] = cw.w;
    cin[i] = cw.Cin;
  }
  return hook_sync("op_target_encoder", s, launch_target_encoder(x, pre, n_views, wp, bias, cin, gamma, beta, feats, s));
}

// launch_small_linear on a [in rows][lda] (any float-aligned pointer), w [N][K] fp32 (rounded to 16 bits here), out rows of ldo floats;
// rows < 0: the one input row is broadcast to -rows result rows.  *form_used: small_linear_form of the launch (1 vector, 0 scalar).
int mvd_op_small_linear(mvd_ctx* c, const float* a, int lda, int rows, int K, const float* w, const float* bias, int N, int act_in,
                        float* out, int ldo, int accumulate, int* form_used, void* stream) {
  RET_IF(hook_begin(c));
  if (!a || !w || !out) return mvd_fail("op_small_linear: null argument");
  if (rows == 0 || K < 1 || N < 1 || lda < K || ldo < N) return mvd_fail("op_small_linear: rows != 0, K, N >= 1, lda >= K, ldo >= N expected");
  if (act_in != ACT_NONE && act_in != ACT_SILU) return mvd_fail("op_small_linear: act_in is none (0) or SiLU (1)");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const half_t* wh;
  RET_IF(hook_f16(c, w, (size_t)N * K, &wh, s));
  if (form_used) *form_used = small_linear_form(a, lda, K, wh);
  return hook_sync("op_small_linear", s, launch_small_linear(a, lda, rows, K, wh, bias, N, act_in, out, ldo, accumulate ? 1 : 0, s));
}

int mvd_op_timestep_embedding(mvd_ctx* c, const int64_t* t, int B, int dim, float* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!t || !out || B < 1 || dim < 1) return mvd_fail("op_timestep_embedding: bad argument");
  hipStream_t s = S(stream);
  return hook_sync("op_timestep_embedding", s, launch_timestep_embedding(t, B, dim, out, s));
}

// op 0: launch_nchw_to_nhwc, in [B][C][HW] -> out rows of ld floats, columns [0, cpad) written (zero from C on); op 1:
// launch_nhwc_to_nchw, in rows of ld floats -> out [B][C][HW] (cpad unused).  *form_used: layout_form of the launch.
int mvd_op_layout(mvd_ctx* c, int op, const float* in, int B, int C, int HW, int ld, int cpad, float* out, int* form_used, void* stream) {
  RET_IF(hook_begin(c));
  if (!in || !out || B < 1 || C < 1 || HW < 1) return mvd_fail("op_layout: bad argument");
  if (op != 0 && op != 1) return mvd_fail("op_layout: op is 0 (to channels-last) or 1 (to NCHW)");
  if (op == 0 ? (cpad < C || ld < cpad) : ld < C) return mvd_fail("op_layout: bad stride");
  hipStream_t s = S(stream);
  if (form_used) *form_used = layout_form(B, C, HW, op == 0 ? cpad : C);
  return hook_sync("op_layout", s, op == 0 ? launch_nchw_to_nhwc(in, B, C, HW, out, ld, cpad, s) : launch_nhwc_to_nchw(in, ld, B, C, HW, out, s));
}

// launch_pack_weight into the caller's 16-bit buffer at out + dst_off halfs: [taps][N][Cin] with Cin the PACKED width (3 Cl with xp);
// src [N][cin_src][taps] (transposed: [cin_src][N][taps]).  *form_used: pack_weight_form of the launch.
int mvd_op_pack_weight(mvd_ctx* c, const float* src, int N, int Cin, int taps, int transposed, int geglu, int cin_src, int xp, int dst_off,
                       void* out, int* form_used, void* stream) {
  RET_IF(hook_begin(c));
  if (!src || !out || N < 1 || Cin < 1 || taps < 1 || taps > 27 || dst_off < 0) return mvd_fail("op_pack_weight: bad argument");
  if (xp && Cin % 3) return mvd_fail("op_pack_weight: the extended-precision layout needs Cin = 3 * Cl");
  if (cin_src < 1 || cin_src > (xp ? Cin / 3 : Cin)) return mvd_fail("op_pack_weight: 1 <= cin_src <= Cl expected");
  if (geglu && N % 64) return mvd_fail("op_pack_weight: geglu pairs 32-row blocks: N % 64 == 0");
  hipStream_t s = S(stream);
  half_t* dst = (half_t*)out + dst_off;
  if (form_used) *form_used = pack_weight_form(N, Cin, taps, transposed, dst, xp);
  return hook_sync("op_pack_weight", s, launch_pack_weight(src, N, Cin, taps, transposed ? 1 : 0, geglu ? 1 : 0, dst, s, cin_src, xp ? 1 : 0));
}

// The other packs, fills and moves, one launcher per op id (a / b: the operands, i0 .. i4: the launcher's integers in its own order;
// a 16-bit operand is given in fp32 and rounded here):
//   0 launch_pack_upconv_weight   a [N][Cin][9], i0 N, i1 Cin                                  out 16-bit [16][N][Cin]
//   1 launch_permute_geglu_bias   a [N], i0 N (N % 64 == 0)                                    out fp32 [N]
//   2 launch_relu_beta_tile       a [Cc], i0 Cc, i1 heads, i2 split                            out 16-bit [(split ? 3 : 1) heads Cc]
//   3 launch_fill_rows_f16        a [n] (16-bit), i0 ld, i1 rows, i2 n                         out 16-bit rows of ld
//   4 launch_rows_f32_to_f16      a rows of lda, i0 lda, i1 rows, i2 C                         out 16-bit [rows][C]
//   5 launch_upsample2_f16        a [B][H][W] rows of ldi, i0 ldi, i1 B, i2 H, i3 W, i4 C      out 16-bit [B][2H][2W][C]
//   6 launch_add_image_rows       a [nb HW] rows of ldi, b [HW][C], i0 ldi, i1 C, i2 nb, i3 HW, i4 ldo    out fp32 rows of ldo
//   7 launch_rows_f16_to_nchw     a [rows][C] (16-bit), i0 rows, i1 C                          out fp32 [C][rows]
//   8 launch_sparse_densify       a [nrows][C], b int32 [nvox] (-1 .. nrows - 1), i0 nvox, i1 C    out fp32 [C][nvox]
int mvd_op_move(mvd_ctx* c, int op, const float* a, const void* b, int i0, int i1, int i2, int i3, int i4, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!a || !out) return mvd_fail("op_move: null argument");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const half_t* h;
  int rc;
  switch (op) {
    case 0:
      if (i0 < 1 || i1 < 1) return mvd_fail("op_move: bad argument");
      rc = launch_pack_upconv_weight(a, i0, i1, (half_t*)out, s);
      break;
    case 1:
      if (i0 < 64 || i0 % 64) return mvd_fail("op_move: geglu pairs 32-row blocks: N % 64 == 0");
      rc = launch_permute_geglu_bias(a, i0, (float*)out, s);
      break;
    case 2:
      if (i0 < 1 || i1 < 1) return mvd_fail("op_move: bad argument");
      rc = launch_relu_beta_tile(a, i0, i1, (half_t*)out, s, i2 ? 1 : 0);
      break;
    case 3:
      if (i1 < 1 || i2 < 1 || i0 < i2) return mvd_fail("op_move: bad stride");
      RET_IF(hook_f16(c, a, (size_t)i2, &h, s));
      rc = launch_fill_rows_f16((half_t*)out, i0, i1, h, i2, s);
      break;
    case 4:
      if (i1 < 1 || i2 < 1 || i0 < i2) return mvd_fail("op_move: bad stride");
      rc = launch_rows_f32_to_f16(a, i0, (long)i1, i2, (half_t*)out, s);
      break;
    case 5:
      if (i1 < 1 || i2 < 1 || i3 < 1 || i4 < 1 || i0 < i4) return mvd_fail("op_move: bad stride");
      rc = launch_upsample2_f16(a, i0, i1, i2, i3, i4, (half_t*)out, s);
      break;
    case 6:
      if (!b || i1 < 1 || i2 < 1 || i3 < 1 || i0 < i1 || i4 < i1) return mvd_fail("op_move: bad stride");
      rc = launch_add_image_rows(a, i0, (const float*)b, i1, i2, i3, (float*)out, i4, s);
      break;
    case 7:
      if (i0 < 1 || i1 < 1) return mvd_fail("op_move: bad argument");
      RET_IF(hook_f16(c, a, (size_t)i0 * i1, &h, s));
      rc = launch_rows_f16_to_nchw(h, (long)i0, i1, (float*)out, s);
      break;
    case 8:
      if (!b || i0 < 1 || i1 < 1) return mvd_fail("op_move: bad argument");
      rc = launch_sparse_densify(a, (const int*)b, (long)i0, i1, (float*)out, s);
      break;
    default:
      return mvd_fail("op_move: unknown op");
  }
  return hook_sync("op_move", s, rc);
}

// The weight folds (fold_gemm_kernel), result fp32 (out_f32) or 16-bit in the caller's buffer:
//   0 launch_fold_qk   a = Wq [heads hd][I], b = Wk [heads hd][Cc] -> [heads Cc][I], scaled
//   1 launch_fold_ov   a = Wo [I][heads hd], b = Wv [heads hd][Cc] -> [I][heads Cc]
//   2 launch_fold_mm   a [M] rows of lda, b [K] rows of ldb -> [M] rows of ldc, columns [0, N)
int mvd_op_fold(mvd_ctx* c, int op, const float* a, const float* b, int heads, int hd, int Cc, int I, float scale, int M, int N, int K,
                int lda, int ldb, int ldc, int out_f32, void* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!a || !b || !out) return mvd_fail("op_fold: null argument");
  hipStream_t s = S(stream);
  half_t* o16 = out_f32 ? nullptr : (half_t*)out;
  float* o32 = out_f32 ? (float*)out : nullptr;
  if (op == 0 || op == 1) {
    if (heads < 1 || heads > 65535 || hd < 1 || Cc < 1 || I < 1) return mvd_fail("op_fold: heads, hd, Cc, I >= 1 expected");
    return hook_sync("op_fold", s, op == 0 ? launch_fold_qk(a, b, heads, hd, Cc, I, scale, o16, s, o32) : launch_fold_ov(a, b, heads, hd, Cc, I, o16, s, o32));
  }
  if (op != 2) return mvd_fail("op_fold: unknown op");
  if (M < 1 || N < 1 || K < 1 || lda < K || ldb < N || ldc < N) return mvd_fail("op_fold: M, N, K >= 1, lda >= K, ldb >= N, ldc >= N expected");
  return hook_sync("op_fold", s, launch_fold_mm(a, lda, b, ldb, M, N, K, o16, ldc, o32, s));
}

// launch_build_cfg_batch: x_noisy [B][TN][4][HW], x_input [B][4][HW], clip [B][dim], timesteps HOST [B] -> xin [copies B TN][HW][8],
// ctx [copies B TN][dim], tt [copies B TN]
int mvd_op_cfg_assemble(mvd_ctx* c, const float* x_noisy, const float* x_input, const float* clip, const int64_t* timesteps, int B, int TN,
                        int HW, int dim, int copies, float* xin, float* ctx, int64_t* tt, void* stream) {
  RET_IF(hook_begin(c));
  if (!x_noisy || !x_input || !clip || !timesteps || !xin || !ctx || !tt) return mvd_fail("op_cfg_assemble: null argument");
  if (B < 1 || TN < 1 || HW < 1 || dim < 1 || (copies != 1 && copies != 2)) return mvd_fail("op_cfg_assemble: B, TN, HW, dim >= 1 and 1 or 2 copies expected");
  hipStream_t s = S(stream);
  return hook_sync("op_cfg_assemble", s, launch_build_cfg_batch(x_noisy, x_input, clip, timesteps, B, TN, HW, dim, copies, xin, ctx, tt, s));
}

// launch_cfg_ddim over n device floats; eps_u, noise, eps_out and x_prev may each be NULL
int mvd_op_cfg_ddim(mvd_ctx* c, const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise, float s1m,
                    float sqrt_at, float sqrt_aprev, float dir_coef, float sigma, float* eps_out, float* x_prev, size_t n, void* stream) {
  RET_IF(hook_begin(c));
  if (!eps_c || n < 1 || (x_prev && !x)) return mvd_fail("op_cfg_ddim: eps_c, n >= 1 and x with x_prev expected");
  hipStream_t s = S(stream);
  return hook_sync("op_cfg_ddim", s, launch_cfg_ddim(eps_c, eps_u, scale, x, noise, s1m, sqrt_at, sqrt_aprev, dir_coef, sigma, eps_out, x_prev, n, s));
}

// The small reductions and mixes:
//   0 launch_fuse_views      a = vf [i0 views][i1 Nv][16], w [16][16], b bias [16] or NULL, i2 total_views, i3 accumulate -> out [Nv][16]
//   1 launch_mse             a, b [n] -> out [1]
//   2 launch_accumulate_f32  out [n] += a [n]  (n % 4 == 0)
//   3 launch_add_rows        out [n] = a [n] + b [n] (b may be NULL)
int mvd_op_small_mix(mvd_ctx* c, int op, const float* a, const float* b, const float* w, int i0, int i1, int i2, int i3, size_t n,
                     float* out, void* stream) {
  RET_IF(hook_begin(c));
  if (!a || !out) return mvd_fail("op_small_mix: null argument");
  hipStream_t s = S(stream);
  switch (op) {
    case 0:
      if (!w || i0 < 1 || i1 < 1 || i2 < 1) return mvd_fail("op_small_mix: bad argument");
      return hook_sync("op_small_mix", s, launch_fuse_views(a, i0, i1, i2, w, b, out, i3 ? 1 : 0, s));
    case 1:
      if (!b || n < 1) return mvd_fail("op_small_mix: bad argument");
      return hook_sync("op_small_mix", s, launch_mse(a, b, n, out, s));
    case 2:
      if (n < 1) return mvd_fail("op_small_mix: bad argument");
      return hook_sync("op_small_mix", s, launch_accumulate_f32(out, a, n, s));
    case 3:
      if (n < 1) return mvd_fail("op_small_mix: bad argument");
      return hook_sync("op_small_mix", s, launch_add_rows(out, a, b, n, s));
  }
  return mvd_fail("op_small_mix: unknown op");
}

}  // extern "C"
