// extern "C" surface of libmvd_hip.so (declared in include/mvd.h).
#include <array>
#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "engine.h"
#include "rowchain.h"

static thread_local std::string g_err;
int mvd_fail(const char* msg) {
  g_err = msg ? msg : "unknown error";
  return -1;
}
const char* mvd_error_text() { return g_err.c_str(); }

namespace {

__global__ void split_rows_to_f32_kernel(const half_t* in, int rows, int C, float* out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)rows * C; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / C, c = i % C;
    const half_t hi = in[r * 3 * C + c], lo = in[r * 3 * C + C + c], h2 = in[r * 3 * C + 2 * C + c];
    out[i] = (float)hi == (float)h2 ? (float)hi + (float)lo : __builtin_nanf("");
  }
}
__global__ void f16_to_f32_kernel(const half_t* in, float* out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (float)in[i];
}
// fp32 [rows][C] -> fp16 rows ldo halfs apart (the pad columns are left as they are), and the reverse from rows ldi apart
__global__ void rows_f32_to_f16_ld_kernel(const float* in, size_t rows, int C, half_t* out, int ldo) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * C; i += (size_t)gridDim.x * blockDim.x)
    out[(i / C) * ldo + i % C] = (half_t)in[i];
}
__global__ void rows_f16_ld_to_f32_kernel(const half_t* in, size_t rows, int C, int ldi, float* out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * C; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (float)in[(i / C) * ldi + i % C];
}
// q,k,v [rows][C] fp32 -> fp16 [rows][3C] (the layout of a fused q|k|v projection)
__global__ void pack_qkv_rows_kernel(const float* q, const float* k, const float* v, int rows, int C, half_t* qkv) {
  const long total = (long)rows * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / C), c = (int)(i % C);
    qkv[(long)r * 3 * C + c] = (half_t)q[i];
    qkv[(long)r * 3 * C + C + c] = (half_t)k[i];
    qkv[(long)r * 3 * C + 2 * C + c] = (half_t)v[i];
  }
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
// UNetWrapper.predict_with_unconditional_scale input assembly (morphable_diffusion.py:133-146), channels-last:
// rows [0,TN) = [x | x_input / 0.18215], rows [TN,2TN) = [x | 0]
// UNet input of one sample's TN views: rows [0, TN) of `out` = the conditional copies, rows [half_off, half_off + TN) the
// unconditional ones (copies == 2); half_off = TN for a single sample, B * TN when B samples share the UNet pass
__global__ void build_cfg_input_kernel(const float* x_noisy, const float* x_input, int TN, int HW, int copies, float* out,
                                       long half_off) {
  const long total = (long)copies * TN * HW * 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i & 7);
    const long bp = i >> 3;
    const int p = (int)(bp % HW), b = (int)(bp / HW);
    const int v = b % TN, half = b / TN;
    float val;
    if (ch < 4) val = x_noisy[((long)v * 4 + ch) * HW + p];
    else val = half == 0 ? x_input[(long)(ch - 4) * HW + p] / 0.18215f : 0.f;
    out[(((long)half * half_off + v) * HW + p) * 8 + ch] = val;
  }
}
__global__ void build_cfg_context_kernel(const float* clip, int TN, int dim, int copies, float* ctx, int64_t* t, int64_t step,
                                         long half_off) {
  const int total = copies * TN * dim;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / dim, j = i - b * dim;
    const long row = (long)(b / TN) * half_off + (b % TN);
    ctx[row * dim + j] = b < TN ? clip[j] : 0.f;
    if (j == 0) t[row] = step;
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
inline int nblk(size_t n) { size_t g = (n + 255) / 256; return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }

}  // namespace

extern "C" {

const char* mvd_last_error(void) { return g_err.c_str(); }
const char* mvd_compute_dtype(void) { return MVD_DTYPE_NAME; }

int mvd_create(const mvd_unet_config* ucfg, const mvd_volume_config* vcfg, int device, size_t workspace_bytes,
               mvd_ctx** out) {
  if (!ucfg || !vcfg || !out) return mvd_fail("mvd_create: null argument");
  HIP_CHECK_RET(hipSetDevice(device));
  mvd_ctx* c = new mvd_ctx();
  c->u = *ucfg;
  c->v = *vcfg;
  c->device = device;
  c->use_halo = mvd_env_engine().halo;
  if (workspace_bytes == 0) workspace_bytes = (size_t)8 << 30;
  hipError_t e = hipMalloc((void**)&c->ws.base, workspace_bytes);
  if (e != hipSuccess) {
    delete c;
    return mvd_fail("mvd_create: workspace allocation failed");
  }
  c->ws.size = workspace_bytes;
  *out = c;
  return 0;
}

static void lora_free(mvd_ctx* c);

void mvd_destroy(mvd_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  mvd_comm_destroy(c);
  lora_free(c);
  for (auto& kv : c->raw)
    if (!c->param_index.count(kv.first)) hipFree(kv.second.d);  // master parameters live in the arena
  float* arenas[5] = {c->arena_p, c->arena_g, c->arena_m, c->arena_v, c->arena_e};
  for (int i = 0; i < 5; ++i)
    if (arenas[i] && c->arena_owned[i]) hipFree(arenas[i]);
  hipFree(c->found_inf);
  hipFree(c->norm_part);
  hipFree(c->norm_dev);
  for (void* p : c->owned) hipFree(p);
  mesh_free(c->mesh);
  hipFree(c->cams);
  auto free_stage = [](mvd_ctx::CamStage& st) {
    if (st.h) hipHostFree(st.h);
    if (st.staged) hipEventDestroy(st.staged);
  };
  free_stage(c->cam_stage);
  for (auto& sl : c->slots) {
    mesh_free(sl.mesh);
    hipFree(sl.cams);
    free_stage(sl.cam_stage);
    hipFree(sl.volume);
  }
  hipFree(c->volume);
  hipFree(c->sp_ws.base);
  hipFree(c->ws.base);
  for (hipEvent_t ev : c->probe_ev) hipEventDestroy(ev);
  for (auto& gb : c->buckets)
    if (gb.ev) hipEventDestroy(gb.ev);
  for (int i = 0; i < 4; ++i) {
    if (c->bstreams[i]) hipStreamDestroy(c->bstreams[i]);
    if (c->bevents[i]) hipEventDestroy(c->bevents[i]);
  }
  if (c->bev_after) hipEventDestroy(c->bev_after);
  for (hipEvent_t ev : c->ev_grad_sync)
    if (ev) hipEventDestroy(ev);
  for (auto& cc : c->cond_const)
    if (cc.k) hipFree(cc.k);
  if (c->enc_scratch) hipFree(c->enc_scratch);
  for (hipEvent_t ev : c->ev_cond) hipEventDestroy(ev);
  for (hipEvent_t ev : {c->ev_fork, c->ev_join, c->ev_join2, c->ev_ctx, c->ev_emb0, c->ev_emb})
    if (ev) hipEventDestroy(ev);
  if (c->side) hipStreamDestroy(c->side);
  if (c->side2) hipStreamDestroy(c->side2);
  for (hipEvent_t ev : {c->ev_s2_fork, c->ev_s2_join})
    if (ev) hipEventDestroy(ev);
  delete c;
}

int mvd_upload_weight(mvd_ctx* c, const char* name, const float* data, const int64_t* shape, int ndim, int on_device) {
  if (!c || !name || !data) return mvd_fail("mvd_upload_weight: null argument");
  if (c->finalized) return mvd_fail("mvd_upload_weight: weights already finalized");
  const std::string k(name);
  if (k.rfind("model.diffusion_model.", 0) != 0 && k.rfind("spatial_volume.", 0) != 0 && k.rfind("time_embed.", 0) != 0 &&
      k.rfind("first_stage_model.decoder.", 0) != 0 && k.rfind("first_stage_model.post_quant_conv.", 0) != 0 &&
      k.rfind("first_stage_model.encoder.", 0) != 0 && k.rfind("first_stage_model.quant_conv.", 0) != 0 &&
      k.rfind("clip_image_encoder.model.visual.", 0) != 0)
    return 0;  // CLIP text tower / loss / schedule buffers: not on this path
  HIP_CHECK_RET(hipSetDevice(c->device));
  RawTensor t;
  t.numel = 1;
  for (int i = 0; i < ndim; ++i) {
    t.shape.push_back(shape[i]);
    t.numel *= (size_t)shape[i];
  }
  HIP_CHECK_RET(hipMalloc((void**)&t.d, std::max<size_t>(t.numel, 1) * sizeof(float)));
  HIP_CHECK_RET(hipMemcpy(t.d, data, t.numel * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  auto it = c->raw.find(k);
  if (it != c->raw.end()) hipFree(it->second.d);
  c->raw[k] = t;
  return 0;
}

int mvd_set_precision_level(mvd_ctx* c, int level) {
  if (!c) return mvd_fail("null context");
  if (c->finalized) return mvd_fail("mvd_set_precision_level: weights already finalized");
  if (level < 0 || level > 6) return mvd_fail("mvd_set_precision_level: level must be 0..6");
  c->precision_level = level;
  return 0;
}

int mvd_set_vae_precision(mvd_ctx* c, int exact) {
  if (!c) return mvd_fail("null context");
  if (c->finalized) return mvd_fail("mvd_set_vae_precision: weights already finalized");
  c->vae_exact = exact != 0;
  return 0;
}

int mvd_finalize_weights(mvd_ctx* c) {
  if (!c) return mvd_fail("null context");
  if (c->finalized) return 0;
  return engine_finalize(c);
}

int mvd_set_mesh(mvd_ctx* c, const float* vertices, const int32_t* coord, const int32_t* out_sh, const float* bounds, int Nv) {
  if (!c || !vertices || !coord || !out_sh || !bounds || Nv <= 0) return mvd_fail("mvd_set_mesh: bad argument");
  HIP_CHECK_RET(hipSetDevice(c->device));
  HIP_CHECK_RET(hipDeviceSynchronize());  // launches on ANY stream may still read the tables being replaced
  RET_IF(engine_set_mesh(c, vertices, coord, out_sh, bounds, Nv, nullptr));
  HIP_CHECK_RET(hipStreamSynchronize(nullptr));
  return 0;
}

int mvd_set_mesh_async(mvd_ctx* c, const float* vertices, const int32_t* coord, const int32_t* out_sh, const float* bounds, int Nv,
                       void* stream) {
  if (!c || !vertices || !coord || !out_sh || !bounds || Nv <= 0) return mvd_fail("mvd_set_mesh_async: bad argument");
  HIP_CHECK_RET(hipSetDevice(c->device));
  return engine_set_mesh(c, vertices, coord, out_sh, bounds, Nv, S(stream));
}

int mvd_select_sample(mvd_ctx* c, int slot) {
  if (!c) return mvd_fail("null context");
  HIP_CHECK_RET(hipSetDevice(c->device));
  return engine_select_sample(c, slot);
}

int mvd_set_cameras(mvd_ctx* c, const float* K, const float* RT, int N) {
  if (!c || !K || !RT || N <= 0) return mvd_fail("mvd_set_cameras: bad argument");
  HIP_CHECK_RET(hipSetDevice(c->device));
  HIP_CHECK_RET(hipDeviceSynchronize());
  RET_IF(engine_set_cameras(c, K, RT, N, nullptr));
  HIP_CHECK_RET(hipStreamSynchronize(nullptr));
  return 0;
}

int mvd_set_samples_async(mvd_ctx* c, int B, const int* slots, const float* const* vertices, const int32_t* const* coord,
                          const int32_t* const* out_sh, const float* const* bounds, const int* Nv, const float* const* K,
                          const float* const* RT, int N, void* stream) {
  if (!c || B <= 0 || !slots || !vertices || !coord || !out_sh || !bounds || !Nv || !K || !RT || N <= 0)
    return mvd_fail("mvd_set_samples_async: bad argument");
  for (int i = 0; i < B; ++i) {
    if (!vertices[i] || !coord[i] || !out_sh[i] || !bounds[i] || !K[i] || !RT[i] || Nv[i] <= 0 || slots[i] < 0 || slots[i] >= 64)
      return mvd_fail("mvd_set_samples_async: bad argument");
    for (int j = 0; j < i; ++j)
      if (slots[j] == slots[i]) return mvd_fail("mvd_set_samples_async: a slot appears twice");
  }
  HIP_CHECK_RET(hipSetDevice(c->device));
  return engine_set_samples(c, B, slots, vertices, coord, out_sh, bounds, Nv, K, RT, N, S(stream));
}

int mvd_rulebook_build(const int32_t* coord, const int32_t* out_sh, int Nv, int force_hash, int32_t* n_sites, int64_t* lens) {
  if (!coord || !out_sh || Nv <= 0 || !n_sites || !lens) return mvd_fail("mvd_rulebook_build: bad argument");
  return engine_rulebook_build(coord, out_sh, Nv, force_hash, n_sites, lens);
}
int mvd_rulebook_table(int which, int32_t* out) {
  if (!out) return mvd_fail("mvd_rulebook_table: bad argument");
  return engine_rulebook_table(which, out);
}

int mvd_set_cameras_async(mvd_ctx* c, const float* K, const float* RT, int N, void* stream) {
  if (!c || !K || !RT || N <= 0) return mvd_fail("mvd_set_cameras_async: bad argument");
  HIP_CHECK_RET(hipSetDevice(c->device));
  return engine_set_cameras(c, K, RT, N, S(stream));
}

int mvd_embed_time(mvd_ctx* c, const int64_t* t, int B, float* out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  WsScope ws_scope(c);
  const int td = c->v.time_dim;
  float* e0 = ws_alloc<float>(c, (size_t)B * td);
  float* e1 = ws_alloc<float>(c, (size_t)B * td);
  WS_CHECK(e0 && e1);
  RET_IF(launch_timestep_embedding(t, B, td, e0, S(stream)));
  RET_IF(launch_small_linear(e0, td, B, td, c->step_te0.w, c->step_te0.bias, td, ACT_NONE, e1, td, 0, S(stream)));
  RET_IF(launch_small_linear(e1, td, B, td, c->step_te2.w, c->step_te2.bias, td, ACT_SILU, out, td, 0, S(stream)));
  return 0;
}

int mvd_unet_forward(mvd_ctx* c, const float* x, const int64_t* timesteps, const float* context, int Bv, int n_ctx,
                     const float* src0, const float* src1, const float* src2, const float* src3, int depth0, float* out,
                     void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  if (n_ctx < 0 || n_ctx > Bv) return mvd_fail("mvd_unet_forward: n_ctx out of range");
  hipStream_t s = S(stream);
  const mvd_unet_config& u = c->u;
  WsScope ws_scope(c);
  const int HW = u.image_size * u.image_size;
  const int cin = u.in_channels;
  if (cin % 8) return mvd_fail("in_channels must be a multiple of 8");
  float* xn = ws_alloc<float>(c, (size_t)Bv * HW * cin);
  float* eps = ws_alloc<float>(c, (size_t)Bv * HW * u.out_channels);
  WS_CHECK(xn && eps);
  RET_IF(launch_nchw_to_nhwc(x, Bv, cin, HW, xn, cin, cin, s));
  const float* srcs[4] = {src0, src1, src2, src3};
  Ctx5 cl[4];
  for (int l = 0; l < 4 && n_ctx > 0; ++l) {
    if (!srcs[l]) return mvd_fail("mvd_unet_forward: missing source_dict level");
    const int sl = u.image_size >> l, Dl = depth0 >> l, C = u.volume_dims[l];
    float* t = ws_alloc<float>(c, (size_t)n_ctx * Dl * sl * sl * C);
    WS_CHECK(t);
    RET_IF(launch_nchw_to_nhwc(srcs[l], n_ctx, C, Dl * sl * sl, t, C, C, s));
    cl[l].p = t;
    cl[l].f32 = 1;
  }
  RET_IF(engine_unet(c, xn, cin, timesteps, context, Bv, n_ctx, depth0, cl, eps, s));
  RET_IF(launch_nhwc_to_nchw(eps, u.out_channels, Bv, u.out_channels, HW, out, s));
  return 0;
}

int mvd_unet_block(mvd_ctx* c, const char* path, const float* x, int B, int C, int H, int W, const int64_t* timesteps,
                   const float* context, const float* volume, int D, int n_ctx, float* out, int out_capacity, int* out_shape,
                   void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized || !path || !x || !out || !out_shape || B <= 0 || C <= 0 || (C & 7) || H <= 0 || W <= 0)
    return mvd_fail("mvd_unet_block: bad argument");
  if (n_ctx < 0 || n_ctx > B) return mvd_fail("mvd_unet_block: n_ctx out of range");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int HW = H * W;
  float* xn = ws_alloc<float>(c, (size_t)B * HW * C);
  // any block's output fits: an Upsample quadruples the pixels, no block is wider than 8 * model_channels
  float* on = ws_alloc<float>(c, (size_t)B * HW * 4 * (size_t)(c->u.model_channels * 8));
  WS_CHECK(xn && on);
  RET_IF(launch_nchw_to_nhwc(x, B, C, HW, xn, C, C, s));
  float* vn = nullptr;
  if (volume && n_ctx > 0) {
    int level = 0;
    for (int r = c->u.image_size; r > H; r >>= 1) ++level;
    if (level > 3 || D <= 0) return mvd_fail("mvd_unet_block: bad volume");
    const int Cc = c->u.volume_dims[level];
    vn = ws_alloc<float>(c, (size_t)n_ctx * D * HW * Cc);
    WS_CHECK(vn);
    RET_IF(launch_nchw_to_nhwc(volume, n_ctx, Cc, D * HW, vn, Cc, Cc, s));
  }
  int Co = 0, Ho = 0;
  RET_IF(engine_unet_block(c, path, xn, B, C, H, W, timesteps, context, vn, D, n_ctx, on, &Co, &Ho, s));
  if ((size_t)B * Co * Ho * Ho > (size_t)out_capacity) return mvd_fail("mvd_unet_block: output buffer too small");
  RET_IF(launch_nhwc_to_nchw(on, Co, B, Co, Ho * Ho, out, s));
  out_shape[0] = B; out_shape[1] = Co; out_shape[2] = Ho; out_shape[3] = Ho;
  return 0;
}

int mvd_vertex_features(mvd_ctx* c, const float* x_noisy, const float* t_embed, const float* v_embed,
                        const int32_t* view_idx, int n_local, int add_bias, float* fused_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c) return mvd_fail("null context");
  return engine_vertex_features(c, x_noisy, t_embed, v_embed, view_idx, n_local, add_bias, fused_out, S(stream));
}

int mvd_vertex_view_features(mvd_ctx* c, const float* x_noisy, const float* t_embed, const float* v_embed,
                             const int32_t* view_idx, int n_local, float* vf_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !vf_out) return mvd_fail("mvd_vertex_view_features: null argument");
  return engine_vertex_features(c, x_noisy, t_embed, v_embed, view_idx, n_local, 0, nullptr, S(stream), vf_out);
}

int mvd_vertex_features_stream_safe(mvd_ctx* c) {
  return (c && c->finalized && c->has_cond && engine_encoder_is_fused(c)) ? 1 : 0;
}

int mvd_fuse_vertex_features(mvd_ctx* c, const float* vf_all, int n_views, float* fused_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !vf_all || !fused_out) return mvd_fail("mvd_fuse_vertex_features: null argument");
  return engine_fuse_vertex_features(c, vf_all, n_views, fused_out, S(stream));
}

int mvd_stage_target_encoder(mvd_ctx* c, const float* x_noisy, const float* t_embed, const float* v_embed, int n_local,
                             float* feats_nchw, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !x_noisy || !t_embed || !v_embed || !feats_nchw || n_local <= 0) return mvd_fail("mvd_stage_target_encoder: bad argument");
  WsScope ws_scope(c);
  const int HW = c->u.image_size * c->u.image_size;
  float* feats = ws_alloc<float>(c, (size_t)n_local * HW * 16);
  WS_CHECK(feats);
  RET_IF(engine_target_encoder(c, x_noisy, t_embed, v_embed, n_local, feats, S(stream)));
  return launch_nhwc_to_nchw(feats, 16, n_local, 16, HW, feats_nchw, S(stream));
}

int mvd_stage_sparse_dense(mvd_ctx* c, const float* fused, int train_mode, float* dense_out, int32_t* shape_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized || !c->has_cond) return mvd_fail("spatial_volume weights not uploaded / finalized");
  if (!c->mesh.Nv) return mvd_fail("mvd_set_mesh must be called first");
  const MeshTables& m = c->mesh;
  if (shape_out) {
    shape_out[0] = c->sparse[8].cout;
    for (int a = 0; a < 3; ++a) shape_out[1 + a] = m.shape[2][a];
  }
  if (!dense_out) return 0;  // shape query
  if (!fused) return mvd_fail("mvd_stage_sparse_dense: null argument");
  const float* rows = nullptr;
  RET_IF(engine_sparse_net(c, fused, S(stream), train_mode != 0, &rows));
  return launch_sparse_densify(rows, m.grid2, (long)m.shape[2][0] * m.shape[2][1] * m.shape[2][2], c->sparse[8].cout, dense_out, S(stream));
}

int mvd_set_spatial_volume(mvd_ctx* c, int use, const int* spatial_dims) {
  if (!c) return mvd_fail("null context");
  if (c->finalized || !c->raw.empty()) return mvd_fail("mvd_set_spatial_volume: call it before the first mvd_upload_weight");
  const int def[4] = {64, 128, 256, 512};
  const int* d = spatial_dims ? spatial_dims : def;
  if (use) {  // SpatialTime3DNet: three stride-2 levels, GroupNorm(8), and its output is added to the 64-channel volume
    if (d[0] != 64) return mvd_fail("mvd_set_spatial_volume: spatial_dims[0] must be 64 (the volume's channel count)");
    for (int i = 0; i < 4; ++i)
      if (d[i] <= 0 || d[i] % 8) return mvd_fail("mvd_set_spatial_volume: every spatial_dims entry must be a positive multiple of 8");
    if (c->v.spatial_volume_size <= 0 || c->v.spatial_volume_size % 8)
      return mvd_fail("mvd_set_spatial_volume: use_spatial_volume needs spatial_volume_size % 8 == 0");
  }
  c->use_spatial_volume = use ? 1 : 0;
  for (int i = 0; i < 4; ++i) c->spatial_dims[i] = d[i];
  return 0;
}

int mvd_spatial_time_volume(mvd_ctx* c, const float* x_noisy, const float* t_embed, const float* v_embed, int n_views,
                            float* volume_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !x_noisy || !t_embed || !v_embed) return mvd_fail("mvd_spatial_time_volume: null argument");
  return engine_spatial_time_volume(c, x_noisy, t_embed, v_embed, n_views, volume_out, S(stream));
}

int mvd_stage_unproject(mvd_ctx* c, const float* feats, int n_views, float* out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !feats || !out) return mvd_fail("mvd_stage_unproject: null argument");
  return engine_stage_unproject(c, feats, n_views, out, S(stream));
}

int mvd_set_volume_ready_event(mvd_ctx* c, void* event) {
  if (!c) return mvd_fail("null context");
  c->vol_ready = (hipEvent_t)event;
  return 0;
}

int mvd_volume_from_fused(mvd_ctx* c, const float* fused, float* volume_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  c->vol_ready = nullptr;  // a registered hand-over event guarded the PREVIOUS volume (the caller registers a new one after this call)
  RET_IF(engine_volume_from_fused(c, fused, S(stream)));
  if (volume_out) {
    const int V = c->v.spatial_volume_size;
    RET_IF(launch_nhwc_to_nchw(c->volume, 64, 1, 64, V * V * V, volume_out, S(stream)));
  }
  return 0;
}

int mvd_volume_from_fused_train(mvd_ctx* c, const float* fused, float* volume_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  c->vol_ready = nullptr;
  RET_IF(engine_volume_from_fused(c, fused, S(stream), /*bn_batch_stats=*/true));
  if (volume_out) {
    const int V = c->v.spatial_volume_size;
    RET_IF(launch_nhwc_to_nchw(c->volume, 64, 1, 64, V * V * V, volume_out, S(stream)));
  }
  return 0;
}

int mvd_set_volume(mvd_ctx* c, const float* volume, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !volume) return mvd_fail("mvd_set_volume: null argument");
  if (!c->volume) return mvd_fail("mvd_set_volume: mvd_set_mesh must be called first");
  const int V = c->v.spatial_volume_size;
  c->vol_ready = nullptr;
  return launch_nchw_to_nhwc(volume, 1, 64, V * V * V, c->volume, 64, 64, S(stream));
}

int mvd_train_enable(mvd_ctx* c, int on) {
  if (!c) return mvd_fail("null context");
  if (c->finalized) return mvd_fail("mvd_train_enable: call it before mvd_finalize_weights");
  c->train_mode = on != 0;
  return 0;
}

int mvd_train_param_count(mvd_ctx* c) { return (c && c->train_mode && c->finalized) ? (int)c->params.size() : 0; }

int mvd_train_param_info(mvd_ctx* c, int i, char* name, size_t cap, int64_t* offset, int64_t* numel, int64_t* shape, int* ndim) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_param_info: context not finalized in training mode");
  if (i < 0 || i >= (int)c->params.size()) return mvd_fail("mvd_train_param_info: index out of range");
  const mvd_ctx::ParamRec& r = c->params[i];
  if (name) {
    if (r.key.size() + 1 > cap) return mvd_fail("mvd_train_param_info: name buffer too small");
    memcpy(name, r.key.c_str(), r.key.size() + 1);
  }
  if (offset) *offset = (int64_t)r.off;
  if (numel) *numel = (int64_t)r.numel;
  if (ndim) *ndim = (int)r.shape.size();
  if (shape)
    for (size_t k = 0; k < r.shape.size() && k < 8; ++k) shape[k] = r.shape[k];
  return 0;
}

int64_t mvd_train_arena_size(mvd_ctx* c) { return (c && c->train_mode && c->finalized) ? (int64_t)c->arena_n : 0; }

int mvd_train_adopt_arena(mvd_ctx* c, int which, float* ptr, int64_t numel) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_adopt_arena: context not finalized in training mode");
  if (which < 0 || which > 4 || !ptr || numel != (int64_t)c->arena_n) return mvd_fail("mvd_train_adopt_arena: bad argument");
  HIP_CHECK_RET(hipSetDevice(c->device));
  HIP_CHECK_RET(hipDeviceSynchronize());
  float** slot[5] = {&c->arena_p, &c->arena_g, &c->arena_m, &c->arena_v, &c->arena_e};
  float* old = *slot[which];
  if (old == ptr) return 0;
  const float* init = old ? old : (which == 4 ? c->arena_p : nullptr);  // a new EMA arena: LitEma's initial shadow, the parameters
  if (init) HIP_CHECK_RET(hipMemcpy(ptr, init, c->arena_n * sizeof(float), hipMemcpyDeviceToDevice));
  else HIP_CHECK_RET(hipMemset(ptr, 0, c->arena_n * sizeof(float)));
  if (old && c->arena_owned[which]) hipFree(old);
  *slot[which] = ptr;
  c->arena_owned[which] = false;
  if (which == 0) {
    for (auto& r : c->params) c->raw[r.key].d = ptr + r.off;
    // biases / norm gains are read in place from the master arena (engine_weights.hip: copy_f32): every such pointer is refreshed
    RET_IF(engine_repack(c));
  }
  return 0;
}

int mvd_train_zero_grad(mvd_ctx* c, void* stream) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_zero_grad: context not finalized in training mode");
  HIP_CHECK_RET(hipSetDevice(c->device));
  HIP_CHECK_RET(hipMemsetAsync(c->arena_g, 0, c->arena_n * sizeof(float), S(stream)));
  c->grad_touched[1] = c->grad_touched[2] = false;
  return 0;
}

// mvd_train_unet_step (lo == nullptr: the plain mean squared error) and mvd_train_unet_step_ex (lo: its loss stage)
static int train_unet_step(mvd_ctx* c, const float* x, const int64_t* timesteps, const float* context, int B, const float* src0,
                           const float* src1, const float* src2, const float* src3, int depth0, const float* target, float loss_scale,
                           int recompute, float* pred_out, float* loss_out, float* dsrc0, float* dsrc1, float* dsrc2, float* dsrc3,
                           void* stream, const TrainLossOpts* lo) {
  const std::string who = lo ? "mvd_train_unet_step_ex" : "mvd_train_unet_step";  // the entry point mvd_last_error names
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  if (!x || !timesteps || !context || !target || !pred_out || B <= 0) return mvd_fail((who + ": bad argument").c_str());
  hipStream_t s = S(stream);
  const mvd_unet_config& u = c->u;
  const int HW = u.image_size * u.image_size, cin = u.in_channels, oc = u.out_channels;
  if (lo) RET_IF(train_loss_check(who.c_str(), B, HW, oc, lo->loss_type, lo->huber_delta));
  WsScope ws_scope(c);
  if (cin % 8) return mvd_fail("in_channels must be a multiple of 8");
  float* xn = ws_alloc<float>(c, (size_t)B * HW * cin);
  float* eps = ws_alloc<float>(c, (size_t)B * HW * oc);
  float* tgt = ws_alloc<float>(c, (size_t)B * HW * oc);
  WS_CHECK(xn && eps && tgt);
  RET_IF(launch_nchw_to_nhwc(x, B, cin, HW, xn, cin, cin, s));
  RET_IF(launch_nchw_to_nhwc(target, B, oc, HW, tgt, oc, oc, s));
  const float* srcs[4] = {src0, src1, src2, src3};
  float* douts[4] = {dsrc0, dsrc1, dsrc2, dsrc3};
  Ctx5 cl[4];
  float* dcl[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t nvol[4];
  for (int l = 0; l < 4; ++l) {
    if (!srcs[l]) return mvd_fail((who + ": missing source_dict level").c_str());
    const int sl = u.image_size >> l, Dl = depth0 >> l, C = u.volume_dims[l];
    nvol[l] = (size_t)B * Dl * sl * sl * C;
    float* t = ws_alloc<float>(c, nvol[l]);
    WS_CHECK(t);
    RET_IF(launch_nchw_to_nhwc(srcs[l], B, C, Dl * sl * sl, t, C, C, s));
    cl[l].p = t;
    cl[l].f32 = 1;
    if (douts[l]) {
      dcl[l] = ws_alloc<float>(c, nvol[l]);
      WS_CHECK(dcl[l]);
      HIP_CHECK_RET(hipMemsetAsync(dcl[l], 0, nvol[l] * sizeof(float), s));
    }
  }
  RET_IF(engine_train_step(c, xn, cin, timesteps, context, B, depth0, cl, tgt, loss_scale, recompute, eps, loss_out, dcl, s, lo));
  c->grad_touched[1] = true;
  RET_IF(launch_nhwc_to_nchw(eps, oc, B, oc, HW, pred_out, s));
  for (int l = 0; l < 4; ++l)
    if (douts[l]) {
      const int sl = u.image_size >> l, Dl = depth0 >> l, C = u.volume_dims[l];
      RET_IF(launch_nhwc_to_nchw(dcl[l], C, B, C, Dl * sl * sl, douts[l], s));
    }
  return 0;
}

int mvd_train_unet_step(mvd_ctx* c, const float* x, const int64_t* timesteps, const float* context, int B, const float* src0,
                        const float* src1, const float* src2, const float* src3, int depth0, const float* target, float loss_scale,
                        int recompute, float* pred_out, float* loss_out, float* dsrc0, float* dsrc1, float* dsrc2, float* dsrc3,
                        void* stream) {
  return train_unet_step(c, x, timesteps, context, B, src0, src1, src2, src3, depth0, target, loss_scale, recompute, pred_out, loss_out,
                         dsrc0, dsrc1, dsrc2, dsrc3, stream, nullptr);
}

int mvd_train_unet_step_ex(mvd_ctx* c, const float* x, const int64_t* timesteps, const float* context, int B, const float* src0,
                           const float* src1, const float* src2, const float* src3, int depth0, const float* target, float loss_scale,
                           int recompute, const float* sample_w, const float* pixel_w, int loss_type, float huber_delta,
                           float* pred_out, float* loss_out, float* loss_per_sample, float* mse_per_sample, float* dsrc0, float* dsrc1,
                           float* dsrc2, float* dsrc3, void* stream) {
  // pixel_w [B,1,s,s] is the loss kernel's [B][HW] as it stands: one channel
  const TrainLossOpts lo{sample_w, pixel_w, loss_type, huber_delta, loss_per_sample, mse_per_sample};
  return train_unet_step(c, x, timesteps, context, B, src0, src1, src2, src3, depth0, target, loss_scale, recompute, pred_out, loss_out,
                         dsrc0, dsrc1, dsrc2, dsrc3, stream, &lo);
}

int mvd_op_train_loss(const float* pred, const float* target, int B, int HW, int C, const float* sample_w, const float* pixel_w,
                      int loss_type, float huber_delta, float loss_scale, float* dpred, float* loss_out, float* loss_per_sample,
                      float* mse_per_sample, void* stream) {
  if (!pred || !target) return mvd_fail("mvd_op_train_loss: null argument");
  RET_IF(train_loss_check("mvd_op_train_loss", B, HW, C, loss_type, huber_delta));
  hipStream_t s = S(stream);
  void* scratch = nullptr;  // the areas and the partial sums live for this call only
  HIP_CHECK_RET(hipMalloc(&scratch, train_loss_scratch_bytes(B, HW)));
  int rc = launch_train_loss(pred, target, B, HW, C, sample_w, pixel_w, loss_type, huber_delta, loss_scale, dpred, loss_out,
                             loss_per_sample, mse_per_sample, scratch, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_train_loss: stream synchronisation failed");
  hipFree(scratch);
  return rc;
}

int mvd_op_image_metrics(const void* pred, int pred_dtype, int pred_layout, const void* target, int target_dtype, int target_layout,
                         const unsigned char* mask, int mask_mode, int V, int H, int W, double* out, void* stream) {
  RET_IF(image_metrics_check("mvd_op_image_metrics", pred, pred_dtype, pred_layout, target, target_dtype, target_layout, mask, mask_mode,
                             V, H, W, out));
  hipStream_t s = S(stream);
  void* scratch = nullptr;  // the per-tile partial sums live for this call only
  HIP_CHECK_RET(hipMalloc(&scratch, image_metrics_scratch_bytes(V, H, W)));
  int rc = launch_image_metrics(pred, pred_dtype, pred_layout, target, target_dtype, target_layout, mask, mask_mode, V, H, W, out,
                                scratch, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_image_metrics: stream synchronisation failed");
  hipFree(scratch);
  return rc;
}

// ---- mesh texturing from views (csrc/k_mesh.hip): no context, the caller's device buffers
int mvd_op_mesh_project(const float* verts, const float* K, const float* RT, int N, int Nv, float z_near, int32_t* xy, int32_t* key,
                        void* stream) {
  RET_IF(mesh_project_check("mvd_op_mesh_project", verts, K, RT, N, Nv, z_near, xy, key));
  hipStream_t s = S(stream);
  int rc = launch_mesh_project(verts, K, RT, N, Nv, z_near, xy, key, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_project: stream synchronisation failed");
  return rc;
}

int mvd_op_mesh_raster(const int32_t* xy, const int32_t* key, const int32_t* faces, int N, int Nv, int Nf, int H, int W, int32_t* face_id,
                       int32_t* pix_key, int32_t* bad_faces, void* stream) {
  RET_IF(mesh_raster_check("mvd_op_mesh_raster", xy, key, faces, N, Nv, Nf, H, W, face_id, pix_key, bad_faces));
  hipStream_t s = S(stream);
  void* scratch = nullptr;  // the packed per-pixel winners live for this call only
  HIP_CHECK_RET(hipMalloc(&scratch, mesh_raster_scratch_bytes(N, H, W)));
  int rc = launch_mesh_raster(xy, key, faces, N, Nv, Nf, H, W, face_id, pix_key, bad_faces, scratch, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_raster: stream synchronisation failed");
  hipFree(scratch);
  return rc;
}

int mvd_op_mesh_vertex_colors(const void* images, int dtype, int layout, const int32_t* xy, const int32_t* key, const int32_t* faces,
                              const int32_t* face_id, const int32_t* pix_key, const float* verts, const float* normals,
                              const float* centres, int N, int Nv, int Nf, int H, int W, float power, int bias, int two_sided,
                              float fill_r, float fill_g, float fill_b, float* color, float* weight_sum, int32_t* n_seen, float* spread,
                              unsigned char* visible, void* stream) {
  RET_IF(mesh_vertex_colors_check("mvd_op_mesh_vertex_colors", images, dtype, layout, xy, key, faces, face_id, pix_key, verts, normals,
                                  centres, N, Nv, Nf, H, W, power, color, weight_sum, n_seen, spread));
  hipStream_t s = S(stream);
  int rc = launch_mesh_vertex_colors(images, dtype, layout, xy, key, faces, face_id, pix_key, verts, normals, centres, N, Nv, Nf, H, W,
                                     power, bias, two_sided, fill_r, fill_g, fill_b, color, weight_sum, n_seen, spread, visible, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_vertex_colors: stream synchronisation failed");
  return rc;
}

// ---- the morphable-model forward (csrc/k_morph.hip): no context, the caller's device buffers; parents is a host array
int mvd_op_morph_pose(const float* betas, const float* pose, const float* j_template, const float* j_dirs, const int32_t* parents, int F,
                      int NB, int J, float* j_rest, float* rot, float* pose_feature, float* joints, float* A, void* stream) {
  RET_IF(morph_pose_check("mvd_op_morph_pose", betas, pose, j_template, j_dirs, parents, F, NB, J, j_rest, rot, pose_feature, joints, A));
  hipStream_t s = S(stream);
  int rc = launch_morph_pose(betas, pose, j_template, j_dirs, parents, F, NB, J, j_rest, rot, pose_feature, joints, A, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_morph_pose: stream synchronisation failed");
  return rc;
}

int mvd_op_morph_skin(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                      const float* post, int F, int V, int L, int NB, int J, float* verts, void* stream) {
  RET_IF(morph_skin_check("mvd_op_morph_skin", basis, v_template, coef, weights, A, F, V, L, NB, J, verts));
  hipStream_t s = S(stream);
  int rc = launch_morph_skin(basis, v_template, coef, weights, A, post, F, V, L, J, verts, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_morph_skin: stream synchronisation failed");
  return rc;
}

int mvd_op_morph_landmarks(const float* verts, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary, int F, int V, int Nf,
                           int M, float* out, void* stream) {
  RET_IF(morph_landmarks_check("mvd_op_morph_landmarks", verts, faces, lmk_face, lmk_bary, F, V, Nf, M, out));
  hipStream_t s = S(stream);
  int rc = launch_morph_landmarks(verts, faces, lmk_face, lmk_bary, F, V, Nf, M, out, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_morph_landmarks: stream synchronisation failed");
  return rc;
}

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
int op_sync(const char* who, hipStream_t s, int rc) {
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail((std::string(who) + ": stream synchronisation failed").c_str());
  return rc;
}
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
  return op_sync("mvd_op_sparse_conv", s, rc);
}

int mvd_op_bn_rows_relu(const float* x, int n, int C, const float* gamma, const float* beta, float eps, float momentum, float* y,
                        float* stats_out, float* rmean, float* rvar, void* stream) {
  if (!x || !y || !gamma || !beta || !rmean != !rvar) return mvd_fail("mvd_op_bn_rows_relu: null argument");
  if (n <= 0 || C <= 0) return mvd_fail("mvd_op_bn_rows_relu: row or channel count out of range");
  hipStream_t s = S(stream);
  return op_sync("mvd_op_bn_rows_relu", s, launch_bn_rows_relu(x, y, n, C, gamma, beta, eps, stats_out, s, rmean, rvar, momentum));
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
  return op_sync("mvd_op_bn_rows_relu_bwd", s, cbwd_bn_rows_relu(xraw, dy, n, C, gamma, beta, stats, part, dgamma, dbeta, s));
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
  return op_sync("mvd_op_sparse_conv_bwd", s, rc);
}

int mvd_train_cond_backward(mvd_ctx* c, int cond_index, const float* x, const float* context, const float* d_out, int B, int H,
                            int W, int depth0, float* dx, float* dcontext, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized || !c->train_mode) return mvd_fail("mvd_train_cond_backward: context not finalized in training mode");
  if (cond_index < 0 || cond_index >= (int)c->conds.size() || !x || !context || !d_out || !dx || B <= 0)
    return mvd_fail("mvd_train_cond_backward: bad argument");
  hipStream_t s = S(stream);
  const CondW& cd = c->conds[cond_index];
  int level = 0;
  for (int r = c->u.image_size; r > H; r >>= 1) ++level;
  if (level > 3 || (c->u.image_size >> level) != H || H != W) return mvd_fail("mvd_train_cond_backward: resolution is not a UNet level");
  const int D = depth0 >> level, HW = H * W;
  WsScope ws_scope(c);
  float* xn = ws_alloc<float>(c, (size_t)B * HW * cd.dim);
  float* dn = ws_alloc<float>(c, (size_t)B * HW * cd.dim);
  float* gx = ws_alloc<float>(c, (size_t)B * HW * cd.dim);
  float* cn = ws_alloc<float>(c, (size_t)B * D * HW * cd.Cc);
  float* gc = ws_alloc<float>(c, (size_t)B * D * HW * cd.Cc);
  WS_CHECK(xn && dn && gx && cn && gc);
  RET_IF(launch_nchw_to_nhwc(x, B, cd.dim, HW, xn, cd.dim, cd.dim, s));
  RET_IF(launch_nchw_to_nhwc(d_out, B, cd.dim, HW, dn, cd.dim, cd.dim, s));
  RET_IF(launch_nchw_to_nhwc(context, B, cd.Cc, D * HW, cn, cd.Cc, cd.Cc, s));
  HIP_CHECK_RET(hipMemsetAsync(gc, 0, (size_t)B * D * HW * cd.Cc * sizeof(float), s));
  RET_IF(engine_train_cond_backward(c, cond_index, xn, cn, dn, B, H, W, level, depth0, gx, gc, s));
  c->grad_touched[1] = true;
  RET_IF(launch_nhwc_to_nchw(gx, cd.dim, B, cd.dim, HW, dx, s));
  if (dcontext) RET_IF(launch_nhwc_to_nchw(gc, cd.Cc, B, cd.Cc, D * HW, dcontext, s));
  return 0;
}

int mvd_train_conditioner_backward_batch(mvd_ctx* c, int B, const int* slots, const float* x_noisy, const int64_t* timesteps,
                                         const float* v_embed, int n_views, const int* target_index, const float* dsrc0,
                                         const float* dsrc1, const float* dsrc2, const float* dsrc3, float* dbg_dvolume,
                                         float* dbg_dfused, float* dbg_dfeats, float* dbg_dtembed, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized || !c->train_mode) return mvd_fail("mvd_train_conditioner_backward: context not finalized in training mode");
  if (B < 1 || !slots || !x_noisy || !timesteps || !v_embed || !target_index || !dsrc0 || !dsrc1 || !dsrc2 || !dsrc3)
    return mvd_fail("mvd_train_conditioner_backward: null argument");
  for (int i = 0; i < B; ++i)
    if (slots[i] < 0 || slots[i] >= 64) return mvd_fail("mvd_train_conditioner_backward: slot out of range (0..63)");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const float* srcs[4] = {dsrc0, dsrc1, dsrc2, dsrc3};
  float* dcl[4];
  int D = c->v.frustum_volume_depth, Sz = c->v.input_image_size / 8;
  for (int l = 0; l < 4; ++l) {  // NCDHW (the reference's layout) -> channels-last, all samples
    const int C = c->v.frustum_dims[l];
    const size_t n = (size_t)B * D * Sz * Sz * C;
    dcl[l] = ws_alloc<float>(c, n);
    WS_CHECK(dcl[l]);
    RET_IF(launch_nchw_to_nhwc(srcs[l], B, C, D * Sz * Sz, dcl[l], C, C, s));
    D = (D - 1) / 2 + 1;
    Sz = (Sz - 1) / 2 + 1;
  }
  c->grad_touched[2] = true;
  return engine_train_conditioner_backward_batch(c, B, slots, x_noisy, timesteps, v_embed, n_views, target_index, dcl, dbg_dvolume,
                                                 dbg_dfused, dbg_dfeats, dbg_dtembed, s);
}

int mvd_train_conditioner_backward(mvd_ctx* c, const float* x_noisy, int64_t timestep, const float* v_embed, int n_views,
                                   int target_index, const float* dsrc0, const float* dsrc1, const float* dsrc2, const float* dsrc3,
                                   float* dbg_dvolume, float* dbg_dfused, float* dbg_dfeats, float* dbg_dtembed, void* stream) {
  if (!c) return mvd_fail("mvd_train_conditioner_backward: null argument");
  const int slot = c->cur_slot;
  return mvd_train_conditioner_backward_batch(c, 1, &slot, x_noisy, &timestep, v_embed, n_views, &target_index, dsrc0, dsrc1, dsrc2, dsrc3,
                                              dbg_dvolume, dbg_dfused, dbg_dfeats, dbg_dtembed, stream);
}

int mvd_train_get_grad(mvd_ctx* c, const char* name, float* out, size_t numel, void* stream) {
  if (!c || !name || !out) return mvd_fail("mvd_train_get_grad: null argument");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  auto it = c->param_index.find(name);
  if (it == c->param_index.end()) return mvd_fail("mvd_train_get_grad: not a parameter of this context (training mode off?)");
  const mvd_ctx::ParamRec& r = c->params[it->second];
  if (r.numel != numel) return mvd_fail("mvd_train_get_grad: size mismatch");
  HIP_CHECK_RET(hipMemcpyAsync(out, c->arena_g + r.off, numel * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return 0;
}

int mvd_train_get_tensor(mvd_ctx* c, const char* name, float* out, size_t numel, void* stream) {
  if (!c || !name || !out) return mvd_fail("mvd_train_get_tensor: null argument");
  if (!c->train_mode || !c->finalized) return mvd_fail("mvd_train_get_tensor: context not finalized in training mode");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  auto it = c->raw.find(name);  // parameters (their storage is the master arena) and the resident buffers
  if (it == c->raw.end()) return mvd_fail("mvd_train_get_tensor: not a resident tensor of this context");
  if (it->second.numel != numel) return mvd_fail("mvd_train_get_tensor: size mismatch");
  HIP_CHECK_RET(hipMemcpyAsync(out, it->second.d, numel * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return 0;
}

int64_t mvd_train_bn_calls(mvd_ctx* c) { return c ? (int64_t)c->bn_train_calls : 0; }

// The arena ranges [off, off + len) one optimiser step updates, with their group: the reference's parameter groups
// (morphable_diffusion.py:627-646) -- 1: the UNet (all of it with finetune_unet, else the DepthTransformers: attention.py:140-142)
// at lr, 2: time_embed and spatial_volume at 10 lr (passed in as lr_aux).  Consecutive parameters of one group form one range; a
// group no backward pass wrote to since zero_grad is left out -- it keeps its parameters AND its moments.
struct StepRange {
  size_t off, len;
  int grp;
};
static void step_ranges(mvd_ctx* c, int finetune_unet, std::vector<StepRange>& out) {
  const std::string U = "model.diffusion_model.";
  auto group_of = [&](const std::string& k) -> int {
    if (k.rfind(U, 0) == 0) {
      if (finetune_unet) return 1;
      return (k.rfind(U + "middle_conditions.", 0) == 0 || k.rfind(U + "output_conditions.", 0) == 0) ? 1 : 0;
    }
    return 2;
  };
  out.clear();
  size_t i = 0;
  while (i < c->params.size()) {
    const int grp = group_of(c->params[i].key);
    size_t j = i;
    while (j + 1 < c->params.size() && group_of(c->params[j + 1].key) == grp) ++j;
    if (grp && c->grad_touched[grp]) {
      const size_t off = c->params[i].off, end = c->params[j].off + ((c->params[j].numel + 63) & ~(size_t)63);
      out.push_back({off, end - off, grp});
    }
    i = j + 1;
  }
}

// norm_dev[0] = || inv_scale * g || over the ranges, norm_dev[1] = the clipping coefficient for max_norm (1 when <= 0);
// *flag (may be null) raised when the sum of squares is not finite.  g: the arena the ranges index (gradients, or LoRA's)
static int grad_norm_pass(mvd_ctx* c, const float* g, const std::vector<StepRange>& rs, float inv_scale, float max_norm, int* flag,
                          hipStream_t s) {
  size_t total = 0;
  for (const StepRange& r : rs) total += (size_t)bwd_grad_sumsq_blocks(r.len);
  if (!c->norm_dev) HIP_CHECK_RET(hipMalloc((void**)&c->norm_dev, 2 * sizeof(float)));
  if (total > c->norm_part_cap) {
    if (c->norm_part) HIP_CHECK_RET(hipFree(c->norm_part));  // (synchronises: nothing still reads the old buffer)
    c->norm_part = nullptr;
    c->norm_part_cap = 0;
    HIP_CHECK_RET(hipMalloc((void**)&c->norm_part, total * sizeof(float)));
    c->norm_part_cap = total;
  }
  size_t at = 0;
  for (const StepRange& r : rs) {
    RET_IF(bwd_grad_sumsq(g + r.off, r.len, inv_scale, c->norm_part + at, s));
    at += (size_t)bwd_grad_sumsq_blocks(r.len);
  }
  return bwd_grad_norm_final(c->norm_part, (int)total, max_norm, c->norm_dev, flag, s);
}

int mvd_train_adamw_step(mvd_ctx* c, float lr, float lr_aux, float beta1, float beta2, float eps, float weight_decay, int step,
                         float inv_scale, int finetune_unet, int* skipped_out, void* stream) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_adamw_step: context not finalized in training mode");
  if (step < 1) return mvd_fail("mvd_train_adamw_step: step counts from 1");
  HIP_CHECK_RET(hipSetDevice(c->device));
  hipStream_t s = S(stream);
  for (float** a : {&c->arena_m, &c->arena_v})
    if (!*a) {
      HIP_CHECK_RET(hipMalloc((void**)a, c->arena_n * sizeof(float)));
      HIP_CHECK_RET(hipMemset(*a, 0, c->arena_n * sizeof(float)));
      c->arena_owned[a == &c->arena_m ? 2 : 3] = true;
    }
  HIP_CHECK_RET(hipMemsetAsync(c->found_inf, 0, sizeof(int), s));
  // The overflow check (a 3.7 GB read: ~1 ms) belongs to loss scaling -- GradScaler's "skip the step, halve the scale".  Without
  // a loss scale (inv_scale == 1: the bfloat16 build) the step is torch.optim.AdamW's own, which checks nothing.
  if (inv_scale != 1.0f) RET_IF(bwd_finite_check(c->arena_g, c->arena_n, c->found_inf, s));
  // one launch per contiguous range of a parameter group
  std::vector<StepRange> rs;
  step_ranges(c, finetune_unet, rs);
  for (const StepRange& r : rs)
    RET_IF(bwd_adamw(c->arena_p + r.off, c->arena_g + r.off, c->arena_m + r.off, c->arena_v + r.off, r.len, r.grp == 1 ? lr : lr_aux,
                     beta1, beta2, eps, weight_decay, step, inv_scale, c->found_inf, s));
  if (skipped_out) {
    HIP_CHECK_RET(hipMemcpyAsync(skipped_out, c->found_inf, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
  }
  return 0;
}

int mvd_train_grad_norm(mvd_ctx* c, float inv_scale, int finetune_unet, float* norm_out, void* stream) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_grad_norm: context not finalized in training mode");
  if (!norm_out) return mvd_fail("mvd_train_grad_norm: null argument");
  HIP_CHECK_RET(hipSetDevice(c->device));
  hipStream_t s = S(stream);
  std::vector<StepRange> rs;
  step_ranges(c, finetune_unet, rs);
  RET_IF(grad_norm_pass(c, c->arena_g, rs, inv_scale, 0.f, nullptr, s));
  HIP_CHECK_RET(hipMemcpyAsync(norm_out, c->norm_dev, sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}

int mvd_train_last_grad_norm(mvd_ctx* c, float* norm_out, void* stream) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_last_grad_norm: context not finalized in training mode");
  if (!norm_out || !c->norm_dev) return mvd_fail("mvd_train_last_grad_norm: no gradient norm has been computed");
  HIP_CHECK_RET(hipSetDevice(c->device));
  HIP_CHECK_RET(hipMemcpyAsync(norm_out, c->norm_dev, sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return 0;
}

int mvd_train_ema_swap(mvd_ctx* c, void* stream) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_ema_swap: context not finalized in training mode");
  if (!c->arena_e) return mvd_fail("mvd_train_ema_swap: no EMA arena (mvd_train_adopt_arena 4, or a step with ema_decay >= 0)");
  HIP_CHECK_RET(hipSetDevice(c->device));
  return bwd_swap_f32(c->arena_p, c->arena_e, c->arena_n, S(stream));
}

int mvd_train_adamw_step_ex(mvd_ctx* c, float lr, float lr_aux, float beta1, float beta2, float eps, float weight_decay, int step,
                            float inv_scale, int finetune_unet, int* skipped_out, float max_grad_norm, float ema_decay,
                            float* grad_norm_out, void* stream) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_train_adamw_step_ex: context not finalized in training mode");
  if (step < 1) return mvd_fail("mvd_train_adamw_step_ex: step counts from 1");
  if (ema_decay > 1.f) return mvd_fail("mvd_train_adamw_step_ex: ema_decay is at most 1 (negative: no EMA)");
  HIP_CHECK_RET(hipSetDevice(c->device));
  hipStream_t s = S(stream);
  for (float** a : {&c->arena_m, &c->arena_v})
    if (!*a) {
      HIP_CHECK_RET(hipMalloc((void**)a, c->arena_n * sizeof(float)));
      HIP_CHECK_RET(hipMemset(*a, 0, c->arena_n * sizeof(float)));
      c->arena_owned[a == &c->arena_m ? 2 : 3] = true;
    }
  const bool ema = ema_decay >= 0.f;
  if (ema && !c->arena_e) {  // LitEma's initial shadow: the parameters as they are before this update
    HIP_CHECK_RET(hipMalloc((void**)&c->arena_e, c->arena_n * sizeof(float)));
    c->arena_owned[4] = true;
    HIP_CHECK_RET(hipMemcpyAsync(c->arena_e, c->arena_p, c->arena_n * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  HIP_CHECK_RET(hipMemsetAsync(c->found_inf, 0, sizeof(int), s));
  std::vector<StepRange> rs;
  step_ranges(c, finetune_unet, rs);
  // One read of the gradients gives the norm, the clipping coefficient and -- with loss scaling -- the overflow flag (the
  // separate finite check of mvd_train_adamw_step is not run).  Without clipping, loss scaling or a norm to report: no pass.
  const bool clip = max_grad_norm > 0.f, scaled = inv_scale != 1.0f;
  const bool norm_pass = clip || scaled || grad_norm_out;
  if (norm_pass) RET_IF(grad_norm_pass(c, c->arena_g, rs, inv_scale, clip ? max_grad_norm : 0.f, scaled ? c->found_inf : nullptr, s));
  for (const StepRange& r : rs)
    RET_IF(bwd_adamw_ex(c->arena_p + r.off, c->arena_g + r.off, c->arena_m + r.off, c->arena_v + r.off,
                        ema ? c->arena_e + r.off : nullptr, r.len, r.grp == 1 ? lr : lr_aux, beta1, beta2, eps, weight_decay, step,
                        inv_scale, clip ? c->norm_dev + 1 : nullptr, ema_decay, c->found_inf, s));
  if (skipped_out) HIP_CHECK_RET(hipMemcpyAsync(skipped_out, c->found_inf, sizeof(int), hipMemcpyDeviceToHost, s));
  if (grad_norm_out) HIP_CHECK_RET(hipMemcpyAsync(grad_norm_out, c->norm_dev, sizeof(float), hipMemcpyDeviceToHost, s));
  if (skipped_out || grad_norm_out) HIP_CHECK_RET(hipStreamSynchronize(s));
  return 0;
}

int mvd_op_adamw_ex(float* p, const float* g, float* m, float* v, float* e, size_t n, float lr, float beta1, float beta2, float eps,
                    float wd, int step, float inv_scale, float max_grad_norm, float ema_decay, float* norm_out, void* stream) {
  if (!p || !g || !m || !v || !n) return mvd_fail("mvd_op_adamw_ex: null argument");
  if (step < 1) return mvd_fail("mvd_op_adamw_ex: step counts from 1");
  hipStream_t s = S(stream);
  const bool clip = max_grad_norm > 0.f;
  float* scratch = nullptr;  // [norm, coefficient | partials]
  if (clip || norm_out) {
    const int blocks = bwd_grad_sumsq_blocks(n);
    HIP_CHECK_RET(hipMalloc((void**)&scratch, (2 + (size_t)blocks) * sizeof(float)));
    int rc = bwd_grad_sumsq(g, n, inv_scale, scratch + 2, s);
    if (!rc) rc = bwd_grad_norm_final(scratch + 2, blocks, clip ? max_grad_norm : 0.f, scratch, nullptr, s);
    if (!rc && norm_out && hipMemcpyAsync(norm_out, scratch, sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
      rc = mvd_fail("mvd_op_adamw_ex: copy of the norm failed");
    if (rc) {
      hipFree(scratch);
      return rc;
    }
  }
  int rc = bwd_adamw_ex(p, g, m, v, e, n, lr, beta1, beta2, eps, wd, step, inv_scale, clip ? scratch + 1 : nullptr, ema_decay, nullptr, s);
  if (scratch) {  // a test hook: the scratch lives for this call only
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_adamw_ex: stream synchronisation failed");
    hipFree(scratch);
  }
  return rc;
}

// ---- LoRA (k_lora.hip) ---------------------------------------------------------------------------------------------------------
// the kernels on raw buffers: a table and the projection's partial sums that live for the call
static int lora_op_table(const char* who, int n, const int64_t* w_off, const int64_t* w0_off, const int64_t* out, const int64_t* in,
                         const int64_t* a_off, const int64_t* b_off, int r, std::vector<LoraTarget>& tab, int* tiles, int* red,
                         size_t* part_n) {
  static thread_local std::string msg;
  msg.clear();
  if (n < 1 || !w_off || !out || !in || !a_off || !b_off) msg = std::string(who) + ": null argument";
  else if (r < 1 || r > LORA_MAX_RANK) msg = std::string(who) + ": the rank must be in 1..64";
  for (int i = 0; msg.empty() && i < n; ++i) {
    if (out[i] < 1 || in[i] < 1 || out[i] >= (1 << 30) || in[i] >= (1 << 30) || w_off[i] < 0 || a_off[i] < 0 || b_off[i] < 0 ||
        (w0_off && w0_off[i] < 0)) {
      msg = std::string(who) + ": out and in must be positive, offsets non-negative";
      break;
    }
    LoraTarget T{};
    T.out = (int)out[i], T.in = (int)in[i];
    T.w_off = w_off[i], T.w0_off = w0_off ? w0_off[i] : 0, T.a_off = a_off[i], T.b_off = b_off[i];
    tab.push_back(T);
  }
  if (!msg.empty()) return mvd_fail(msg.c_str());
  lora_plan(tab.data(), n, r, tiles, red, part_n);
  if (*tiles < 1 || *red < 1) return mvd_fail("lora op: more than 2^31 tiles");
  return 0;
}

int mvd_op_lora_project_grouped(const float* dW, const float* A, const float* B, int n, const int64_t* w_off, const int64_t* out,
                                const int64_t* in, const int64_t* a_off, const int64_t* b_off, int r, float scale, float* gA, float* gB,
                                void* stream) {
  if (!dW || !A || !B || !gA || !gB) return mvd_fail("mvd_op_lora_project: null argument");
  std::vector<LoraTarget> tab;
  int tiles = 0, red = 0;
  size_t part_n = 0;
  RET_IF(lora_op_table("mvd_op_lora_project", n, w_off, nullptr, out, in, a_off, b_off, r, tab, &tiles, &red, &part_n));
  hipStream_t s = S(stream);
  float* scratch = nullptr;  // [partials | table]
  HIP_CHECK_RET(hipMalloc((void**)&scratch, part_n * sizeof(float) + tab.size() * sizeof(LoraTarget)));
  LoraTarget* d_tab = (LoraTarget*)(scratch + part_n);
  int rc = hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(LoraTarget), hipMemcpyHostToDevice, s) == hipSuccess
               ? 0 : mvd_fail("mvd_op_lora_project: table upload failed");
  if (!rc) rc = lora_project(d_tab, n, tiles, red, dW, A, B, r, scale, scratch, gA, gB, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_lora_project: stream synchronisation failed");
  hipFree(scratch);
  return rc;
}

int mvd_op_lora_merge_grouped(const float* W0, const float* A, const float* B, int n, const int64_t* w_off, const int64_t* w0_off,
                              const int64_t* out, const int64_t* in, const int64_t* a_off, const int64_t* b_off, int r, float scale,
                              float* W, void* stream) {
  if (!W0 || !A || !B || !W || !w0_off) return mvd_fail("mvd_op_lora_merge: null argument");
  std::vector<LoraTarget> tab;
  int tiles = 0, red = 0;
  size_t part_n = 0;
  RET_IF(lora_op_table("mvd_op_lora_merge", n, w_off, w0_off, out, in, a_off, b_off, r, tab, &tiles, &red, &part_n));
  hipStream_t s = S(stream);
  LoraTarget* d_tab = nullptr;
  HIP_CHECK_RET(hipMalloc((void**)&d_tab, tab.size() * sizeof(LoraTarget)));
  int rc = hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(LoraTarget), hipMemcpyHostToDevice, s) == hipSuccess
               ? 0 : mvd_fail("mvd_op_lora_merge: table upload failed");
  if (!rc) rc = lora_merge(d_tab, n, tiles, W0, A, B, r, scale, W, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_lora_merge: stream synchronisation failed");
  hipFree(d_tab);
  return rc;
}

int mvd_op_lora_project(const float* dW, const float* A, const float* B, int out, int in, int r, float scale, float* gA, float* gB,
                        void* stream) {
  const int64_t zero = 0, o = out, i = in;
  return mvd_op_lora_project_grouped(dW, A, B, 1, &zero, &o, &i, &zero, &zero, r, scale, gA, gB, stream);
}

int mvd_op_lora_merge(const float* W0, const float* A, const float* B, int out, int in, int r, float scale, float* W, void* stream) {
  const int64_t zero = 0, o = out, i = in;
  return mvd_op_lora_merge_grouped(W0, A, B, 1, &zero, &zero, &o, &i, &zero, &zero, r, scale, W, stream);
}

static void lora_free(mvd_ctx* c) {
  mvd_ctx::Lora& l = c->lora;
  for (int i = 0; i < 4; ++i)
    if (l.arena[i] && l.owned[i]) hipFree(l.arena[i]);
  hipFree(l.w0);
  hipFree(l.part);
  hipFree(l.d_tab);
  l = mvd_ctx::Lora();
}

int mvd_lora_detach(mvd_ctx* c, int keep_merged) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_lora_detach: context not finalized in training mode");
  if (!c->lora.rank) return 0;
  HIP_CHECK_RET(hipSetDevice(c->device));
  HIP_CHECK_RET(hipDeviceSynchronize());
  if (!keep_merged)
    for (const LoraTarget& T : c->lora.tab)
      HIP_CHECK_RET(hipMemcpy(c->arena_p + T.w_off, c->lora.w0 + T.w0_off, (size_t)T.out * T.in * sizeof(float), hipMemcpyDeviceToDevice));
  lora_free(c);
  return 0;
}

int mvd_lora_attach(mvd_ctx* c, const char* const* keys, int n, int rank, float alpha) {
  if (!c || !c->train_mode || !c->finalized) return mvd_fail("mvd_lora_attach: context not finalized in training mode");
  if (!keys || n < 1) return mvd_fail("mvd_lora_attach: no target");
  if (rank < 1 || rank > LORA_MAX_RANK) return mvd_fail("mvd_lora_attach: the rank must be in 1..64");
  HIP_CHECK_RET(hipSetDevice(c->device));
  static thread_local std::string msg;
  mvd_ctx::Lora l;
  auto pad = [](size_t v) { return (v + 63) & ~(size_t)63; };
  for (int i = 0; i < n; ++i) {
    auto it = keys[i] ? c->param_index.find(keys[i]) : c->param_index.end();
    if (it == c->param_index.end()) {
      msg = std::string("mvd_lora_attach: not a parameter of this context: ") + (keys[i] ? keys[i] : "(null)");
      return mvd_fail(msg.c_str());
    }
    const mvd_ctx::ParamRec& p = c->params[it->second];
    bool ok = p.shape.size() >= 2 && p.shape[0] >= 1 && p.shape[1] >= 1 && p.shape[0] < (1 << 30) && p.shape[1] < (1 << 30);
    for (size_t d = 2; d < p.shape.size(); ++d) ok = ok && p.shape[d] == 1;
    for (size_t j : l.param) ok = ok && j != it->second;  // (a key named twice)
    if (!ok) {
      msg = "mvd_lora_attach: " + p.key + " is not an (out, in[, 1...]) weight (or is named twice)";
      return mvd_fail(msg.c_str());
    }
    LoraTarget T{};
    T.out = (int)p.shape[0], T.in = (int)p.shape[1];
    T.w_off = (long long)p.off;
    T.w0_off = (long long)l.w0_n;
    l.w0_n += pad(p.numel);
    T.a_off = (long long)l.n;
    l.n += pad((size_t)rank * T.in);
    T.b_off = (long long)l.n;
    l.n += pad((size_t)T.out * rank);
    l.tab.push_back(T);
    l.param.push_back(it->second);
  }
  size_t part_n = 0;
  lora_plan(l.tab.data(), n, rank, &l.tiles, &l.red_blocks, &part_n);
  if (l.tiles < 1 || l.red_blocks < 1) return mvd_fail("mvd_lora_attach: more than 2^31 tiles");
  RET_IF(mvd_lora_detach(c, 0));  // (synchronises the device)
  l.rank = rank;
  l.scale = alpha / (float)rank;
  c->lora = l;
  mvd_ctx::Lora& L_ = c->lora;
  auto fail = [&](const char* m) {
    lora_free(c);
    return mvd_fail(m);
  };
  if (hipMalloc((void**)&L_.w0, L_.w0_n * sizeof(float)) != hipSuccess || hipMalloc((void**)&L_.part, part_n * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&L_.d_tab, (size_t)n * sizeof(LoraTarget)) != hipSuccess)
    return fail("mvd_lora_attach: allocation failed");
  for (int i = 0; i < 4; ++i) {
    if (hipMalloc((void**)&L_.arena[i], L_.n * sizeof(float)) != hipSuccess) return fail("mvd_lora_attach: allocation failed");
    L_.owned[i] = true;
    if (hipMemset(L_.arena[i], 0, L_.n * sizeof(float)) != hipSuccess) return fail("mvd_lora_attach: memset failed");
  }
  if (hipMemset(L_.w0, 0, L_.w0_n * sizeof(float)) != hipSuccess || hipMemset(L_.part, 0, part_n * sizeof(float)) != hipSuccess ||
      hipMemcpy(L_.d_tab, L_.tab.data(), (size_t)n * sizeof(LoraTarget), hipMemcpyHostToDevice) != hipSuccess)
    return fail("mvd_lora_attach: table upload failed");
  for (const LoraTarget& T : L_.tab)
    if (hipMemcpy(L_.w0 + T.w0_off, c->arena_p + T.w_off, (size_t)T.out * T.in * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess)
      return fail("mvd_lora_attach: snapshot of the base weights failed");
  return 0;
}

int mvd_lora_arena_size(mvd_ctx* c, int64_t* numel) {
  if (!c || !c->lora.rank || !numel) return mvd_fail("mvd_lora_arena_size: no adapters attached");
  *numel = (int64_t)c->lora.n;
  return 0;
}
int mvd_lora_target_count(mvd_ctx* c) { return (c && c->lora.rank) ? (int)c->lora.tab.size() : 0; }

int mvd_lora_info(mvd_ctx* c, int i, char* name, size_t cap, int64_t* a_off, int64_t* b_off, int64_t* out, int64_t* in) {
  if (!c || !c->lora.rank) return mvd_fail("mvd_lora_info: no adapters attached");
  if (i < 0 || i >= (int)c->lora.tab.size()) return mvd_fail("mvd_lora_info: index out of range");
  const LoraTarget& T = c->lora.tab[i];
  const std::string& key = c->params[c->lora.param[i]].key;
  if (name) {
    if (key.size() + 1 > cap) return mvd_fail("mvd_lora_info: name buffer too small");
    memcpy(name, key.c_str(), key.size() + 1);
  }
  if (a_off) *a_off = T.a_off;
  if (b_off) *b_off = T.b_off;
  if (out) *out = T.out;
  if (in) *in = T.in;
  return 0;
}

int mvd_lora_adopt_arena(mvd_ctx* c, int which, float* ptr, int64_t numel) {
  if (!c || !c->lora.rank) return mvd_fail("mvd_lora_adopt_arena: no adapters attached");
  if (which < 0 || which > 3 || !ptr || numel != (int64_t)c->lora.n) return mvd_fail("mvd_lora_adopt_arena: bad argument");
  HIP_CHECK_RET(hipSetDevice(c->device));
  HIP_CHECK_RET(hipDeviceSynchronize());
  float* old = c->lora.arena[which];
  if (old == ptr) return 0;
  HIP_CHECK_RET(hipMemcpy(ptr, old, c->lora.n * sizeof(float), hipMemcpyDeviceToDevice));
  if (c->lora.owned[which]) hipFree(old);
  c->lora.arena[which] = ptr;
  c->lora.owned[which] = false;
  return 0;
}

static int lora_merge_ctx(mvd_ctx* c, hipStream_t s) {
  const mvd_ctx::Lora& l = c->lora;
  return lora_merge(l.d_tab, (int)l.tab.size(), l.tiles, l.w0, l.arena[0], l.arena[0], l.rank, l.scale, c->arena_p, s);
}

int mvd_lora_set_scale(mvd_ctx* c, float scale, void* stream) {
  if (!c || !c->lora.rank) return mvd_fail("mvd_lora_set_scale: no adapters attached");
  HIP_CHECK_RET(hipSetDevice(c->device));
  c->lora.scale = scale;
  return lora_merge_ctx(c, S(stream));
}

static int lora_project_ctx(mvd_ctx* c, hipStream_t s) {
  const mvd_ctx::Lora& l = c->lora;
  return lora_project(l.d_tab, (int)l.tab.size(), l.tiles, l.red_blocks, c->arena_g, l.arena[0], l.arena[0], l.rank, l.scale, l.part,
                      l.arena[1], l.arena[1], s);
}

int mvd_lora_project(mvd_ctx* c, void* stream) {
  if (!c || !c->lora.rank) return mvd_fail("mvd_lora_project: no adapters attached");
  HIP_CHECK_RET(hipSetDevice(c->device));
  return lora_project_ctx(c, S(stream));
}

int mvd_lora_step(mvd_ctx* c, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float inv_scale,
                  float max_grad_norm, int* skipped_out, float* grad_norm_out, void* stream) {
  if (!c || !c->lora.rank) return mvd_fail("mvd_lora_step: no adapters attached");
  if (step < 1) return mvd_fail("mvd_lora_step: step counts from 1");
  HIP_CHECK_RET(hipSetDevice(c->device));
  hipStream_t s = S(stream);
  const mvd_ctx::Lora& l = c->lora;
  RET_IF(lora_project_ctx(c, s));
  HIP_CHECK_RET(hipMemsetAsync(c->found_inf, 0, sizeof(int), s));
  const bool clip = max_grad_norm > 0.f, scaled = inv_scale != 1.0f;
  if (clip || scaled || grad_norm_out) {
    const std::vector<StepRange> rs{{0, l.n, 1}};
    RET_IF(grad_norm_pass(c, l.arena[1], rs, inv_scale, clip ? max_grad_norm : 0.f, scaled ? c->found_inf : nullptr, s));
  }
  RET_IF(bwd_adamw_ex(l.arena[0], l.arena[1], l.arena[2], l.arena[3], nullptr, l.n, lr, beta1, beta2, eps, weight_decay, step, inv_scale,
                      clip ? c->norm_dev + 1 : nullptr, -1.f, c->found_inf, s));
  RET_IF(lora_merge_ctx(c, s));
  if (skipped_out) HIP_CHECK_RET(hipMemcpyAsync(skipped_out, c->found_inf, sizeof(int), hipMemcpyDeviceToHost, s));
  if (grad_norm_out) HIP_CHECK_RET(hipMemcpyAsync(grad_norm_out, c->norm_dev, sizeof(float), hipMemcpyDeviceToHost, s));
  if (skipped_out || grad_norm_out) HIP_CHECK_RET(hipStreamSynchronize(s));
  return 0;
}

int mvd_train_repack(mvd_ctx* c) {
  if (!c) return mvd_fail("null context");
  return engine_repack(c);
}
int mvd_train_repack_async(mvd_ctx* c, void* stream) {
  if (!c) return mvd_fail("null context");
  return engine_repack(c, S(stream), true);
}

int mvd_train_grad_bucket_count(mvd_ctx* c) { return c ? c->n_buckets : 0; }
int mvd_train_grad_bucket(mvd_ctx* c, int k, int max_ranges, int64_t* offs, int64_t* lens, int* n_ranges) {
  if (!c || k < 0 || k >= c->n_buckets || !n_ranges) return mvd_fail("mvd_train_grad_bucket: no such bucket");
  const mvd_ctx::GradBucket& b = c->buckets[k];
  *n_ranges = (int)b.off.size();
  if (!offs || !lens) return 0;  // count only
  if (max_ranges < (int)b.off.size()) return mvd_fail("mvd_train_grad_bucket: range arrays too small");
  for (size_t r = 0; r < b.off.size(); ++r) {
    offs[r] = (int64_t)b.off[r];
    lens[r] = (int64_t)b.len[r];
  }
  return 0;
}
int mvd_train_grad_bucket_wait(mvd_ctx* c, int k, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || k < 0 || k >= c->n_buckets || !c->buckets[k].ev) return mvd_fail("mvd_train_grad_bucket_wait: no such bucket");
  HIP_CHECK_RET(hipStreamWaitEvent(S(stream), c->buckets[k].ev, 0));
  return 0;
}
int mvd_train_set_bucket_snapshot(mvd_ctx* c, float* arena) {
  if (!c) return mvd_fail("null context");
  c->bucket_snapshot = arena;
  return 0;
}

int mvd_mse_loss(mvd_ctx* c, const float* a, const float* b, size_t n, float* out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !a || !b || !out || n == 0) return mvd_fail("mvd_mse_loss: bad argument");
  return launch_mse(a, b, n, out, S(stream));
}

int mvd_frustum_volumes(mvd_ctx* c, const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN,
                        float* out0, float* out1, float* out2, float* out3, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  WsScope ws_scope(c);
  FrustumOut fo;
  RET_IF(engine_frustum(c, t_embed, v_embed, view_idx, TN, &fo, S(stream)));
  float* outs[4] = {out0, out1, out2, out3};
  int D = c->v.frustum_volume_depth, Sz = c->v.input_image_size / 8;
  for (int l = 0; l < 4; ++l) {
    if (outs[l]) RET_IF(launch_nhwc_to_nchw(fo.lvl[l], c->v.frustum_dims[l], TN, c->v.frustum_dims[l], D * Sz * Sz, outs[l], S(stream)));
    D = (D - 1) / 2 + 1;
    Sz = (Sz - 1) / 2 + 1;
  }
  return 0;
}

int mvd_frustum_volumes_batch(mvd_ctx* c, int B, const int* slots, const float* volumes, const float* t_embed, const float* v_rows,
                              const int32_t* view_idx, float* out0, float* out1, float* out2, float* out3, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  if (B < 1 || !slots || !volumes || !t_embed || !v_rows || !view_idx) return mvd_fail("mvd_frustum_volumes_batch: bad argument");
  for (int i = 0; i < B; ++i)
    if (slots[i] < 0 || slots[i] >= 64) return mvd_fail("mvd_frustum_volumes_batch: slot out of range (0..63)");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int V = c->v.spatial_volume_size;
  float* vcl = ws_alloc<float>(c, (size_t)B * V * V * V * 64);  // NCDHW -> channels-last, all samples
  WS_CHECK(vcl);
  RET_IF(launch_nchw_to_nhwc(volumes, B, 64, V * V * V, vcl, 64, 64, s));
  FrustumOut fo;
  RET_IF(engine_frustum_batch(c, B, slots, vcl, t_embed, v_rows, view_idx, &fo, s));
  float* outs[4] = {out0, out1, out2, out3};
  int D = c->v.frustum_volume_depth, Sz = c->v.input_image_size / 8;
  for (int l = 0; l < 4; ++l) {
    if (outs[l]) RET_IF(launch_nhwc_to_nchw(fo.lvl[l], c->v.frustum_dims[l], B, c->v.frustum_dims[l], D * Sz * Sz, outs[l], s));
    D = (D - 1) / 2 + 1;
    Sz = (Sz - 1) / 2 + 1;
  }
  return 0;
}

// The final launch of a denoising step: (guided-eps inputs eps_c / eps_u (null without guidance), element count, stream) -> the
// sampler's update kernel (cfg_ddim_kernel or cfg_dpm_kernel)
typedef std::function<int(const float*, const float*, size_t, hipStream_t)> StepUpdate;

// The body shared by mvd_denoise_views_batch (DDIM) and mvd_denoise_views_ms (DPM-Solver++): CFG input rows -> UNet -> NCHW eps;
// only the update launch differs
static int denoise_views_common(const char* name, mvd_ctx* c, int B, const int* slots, const float* x_noisy, const float* x_input,
                                const float* clip, const int64_t* timesteps, const float* t_embed, const float* v_embed,
                                const int32_t* view_idx, int TN, float cfg_scale, const StepUpdate& update, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  if (B < 1 || TN < 1 || (B > 1 && !slots) || !timesteps) return mvd_fail((std::string(name) + ": bad argument").c_str());
  hipStream_t s = S(stream);
  const mvd_unet_config& u = c->u;
  if (u.in_channels != 8 || u.out_channels != 4) return mvd_fail("denoise_views: expects the 8-in / 4-out latent UNet");
  WsScope ws_scope(c);
  const int HW = u.image_size * u.image_size;
  const bool cfg = cfg_scale != 1.0f;
  const int copies = cfg ? 2 : 1, Bv = copies * B * TN;
  const int td = c->v.time_dim, vd = c->v.view_dim;
  // The frustum network feeds the DepthTransformers only (middle block onwards): engine_unet enqueues it (through this
  // producer) on its side stream after the full-resolution input blocks, beside the lower-resolution ones.
  FrustumOut fo;
  Ctx5 cl[4];
  const CtxProducer produce = [&](hipStream_t ps) -> int {
    if (B == 1 && !slots) RET_IF(engine_frustum(c, t_embed, v_embed, view_idx, TN, &fo, ps, /*half0=*/true));
    else RET_IF(engine_frustum_multi(c, B, slots, t_embed, v_embed, view_idx, TN, &fo, ps, /*half0=*/true));
    for (int l = 0; l < 4; ++l) {
      cl[l].p = fo.lvl[l];
      cl[l].f32 = 1;
    }
    if (fo.lvl0_half) {
      cl[0].p = fo.lvl0_half;
      cl[0].f32 = 0;
    }
    return 0;
  };
  float* xin = ws_alloc<float>(c, (size_t)Bv * HW * 8);
  float* ctx = ws_alloc<float>(c, (size_t)Bv * u.context_dim);
  int64_t* tt = ws_alloc<int64_t>(c, (size_t)Bv);
  float* eps = ws_alloc<float>(c, (size_t)Bv * HW * 4);
  float* eps_nchw = ws_alloc<float>(c, (size_t)Bv * HW * 4);
  WS_CHECK(xin && ctx && tt && eps && eps_nchw);
  // UNet batch order (morphable_diffusion.py:133-147): every conditional row first -- sample by sample, view by view --, then
  // the unconditional copies in the same order
  const long half_off = (long)B * TN;
  for (int b = 0; b < B; ++b) {
    hipLaunchKernelGGL(build_cfg_input_kernel, dim3(nblk((size_t)copies * TN * HW * 8)), dim3(256), 0, s,
                       x_noisy + (size_t)b * TN * 4 * HW, x_input + (size_t)b * 4 * HW, TN, HW, copies, xin + (size_t)b * TN * HW * 8,
                       half_off);
    hipLaunchKernelGGL(build_cfg_context_kernel, dim3(nblk((size_t)copies * TN * u.context_dim)), dim3(256), 0, s,
                       clip + (size_t)b * u.context_dim, TN, u.context_dim, copies, ctx + (size_t)b * TN * u.context_dim,
                       tt + (size_t)b * TN, timesteps[b], half_off);
  }
  HIP_CHECK_RET(hipGetLastError());
  (void)td; (void)vd;
  RET_IF(engine_unet(c, xin, 8, tt, ctx, Bv, B * TN, c->v.frustum_volume_depth, cl, eps, s, &produce));
  RET_IF(launch_nhwc_to_nchw(eps, 4, Bv, 4, HW, eps_nchw, s));
  const size_t n = (size_t)B * TN * 4 * HW;
  return update(eps_nchw, cfg ? eps_nchw + n : nullptr, n, s);
}

int mvd_denoise_views_batch(mvd_ctx* c, int B, const int* slots, const float* x_noisy, const float* x_input, const float* clip,
                            const int64_t* timesteps, const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN,
                            float cfg_scale, const float* noise, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                            float dir_coef, float sigma, float* eps_out, float* x_prev, void* stream) {
  const StepUpdate ddim = [&](const float* ec, const float* eu, size_t n, hipStream_t s) {
    return launch_cfg_ddim(ec, eu, cfg_scale, x_noisy, noise, sqrt_one_minus_at, sqrt_at, sqrt_aprev, dir_coef, sigma, eps_out,
                           x_prev, n, s);
  };
  return denoise_views_common("mvd_denoise_views_batch", c, B, slots, x_noisy, x_input, clip, timesteps, t_embed, v_embed, view_idx,
                              TN, cfg_scale, ddim, stream);
}

int mvd_denoise_views_ms(mvd_ctx* c, int B, const int* slots, const float* x_noisy, const float* x_input, const float* clip,
                         const int64_t* timesteps, const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN,
                         float cfg_scale, const float* noise, float s1m, float sqrt_at, float c_x, float c_d, float c_c, float c_n,
                         float* x0_hist, int first, float* eps_out, float* x_next, void* stream) {
  if (!x0_hist || !x_next) return mvd_fail("mvd_denoise_views_ms: x0_hist and x_next are required");
  const DpmCoef k{s1m, sqrt_at, c_x, c_d, c_c, c_n};
  const StepUpdate dpm = [&](const float* ec, const float* eu, size_t n, hipStream_t s) {
    return launch_cfg_dpm(ec, eu, cfg_scale, x_noisy, noise, k, x0_hist, first ? 0 : 1, eps_out, x_next, n, s);
  };
  return denoise_views_common("mvd_denoise_views_ms", c, B, slots, x_noisy, x_input, clip, timesteps, t_embed, v_embed, view_idx, TN,
                              cfg_scale, dpm, stream);
}

int mvd_op_cfg_ms(const float* eps_c, const float* eps_u, float scale, const float* x, const float* noise, float s1m, float sqrt_at,
                  float c_x, float c_d, float c_c, float c_n, float* x0_hist, int first, float* eps_out, float* x_next, size_t n,
                  void* stream) {
  return launch_cfg_dpm(eps_c, eps_u, scale, x, noise, DpmCoef{s1m, sqrt_at, c_x, c_d, c_c, c_n}, x0_hist, first ? 0 : 1, eps_out,
                        x_next, n, S(stream));
}

int mvd_denoise_views(mvd_ctx* c, const float* x_noisy, const float* x_input, const float* clip, int64_t timestep,
                      const float* t_embed, const float* v_embed, const int32_t* view_idx, int TN, float cfg_scale,
                      const float* noise, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float dir_coef,
                      float sigma, float* eps_out, float* x_prev, void* stream) {
  return mvd_denoise_views_batch(c, 1, nullptr, x_noisy, x_input, clip, &timestep, t_embed, v_embed, view_idx, TN, cfg_scale, noise,
                                 sqrt_one_minus_at, sqrt_at, sqrt_aprev, dir_coef, sigma, eps_out, x_prev, stream);
}


// ------------------------------------------------------------------------------------------ view exchange over RCCL
// the sharded step's ONE collective -- the all-gather of the per-view vertex features -- behind the C
// ABI, on a stream of the caller, with a communicator the library owns.  librccl.so is opened on first use (dlopen: the
// library itself has no link-time dependency on it, single-GPU users never load it).  The unique id travels over whatever
// side channel the host has (the Python mirror broadcasts it with torch.distributed).
namespace {
struct RcclApi {
  void* h = nullptr;
  int (*get_unique_id)(void*) = nullptr;
  int (*comm_init_rank)(void**, int, mvd_rccl_id, int) = nullptr;
  int (*comm_destroy)(void*) = nullptr;
  int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  const char* (*get_error_string)(int) = nullptr;
};
RcclApi* rccl_api() {
  // C++11 magic static: initialised exactly once, by one thread, before any caller sees it (a one-thread-per-GPU host may call
  // mvd_comm_init for several contexts at the same time)
  static const RcclApi api = [] {
    RcclApi a;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
      a.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (a.h) break;
    }
    if (a.h) {
      a.get_unique_id = (int (*)(void*))dlsym(a.h, "ncclGetUniqueId");
      a.comm_init_rank = (int (*)(void**, int, mvd_rccl_id, int))dlsym(a.h, "ncclCommInitRank");
      a.comm_destroy = (int (*)(void*))dlsym(a.h, "ncclCommDestroy");
      a.all_gather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(a.h, "ncclAllGather");
      a.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(a.h, "ncclAllReduce");
      a.group_start = (int (*)())dlsym(a.h, "ncclGroupStart");
      a.group_end = (int (*)())dlsym(a.h, "ncclGroupEnd");
      a.get_error_string = (const char* (*)(int))dlsym(a.h, "ncclGetErrorString");
      if (!a.get_unique_id || !a.comm_init_rank || !a.comm_destroy || !a.all_gather || !a.all_reduce) a.h = nullptr;
    }
    return a;
  }();
  return api.h ? const_cast<RcclApi*>(&api) : nullptr;
}
int rccl_fail(RcclApi* a, const char* what, int rc) {
  static thread_local std::string msg;
  msg = std::string(what) + ": " + (a && a->get_error_string ? a->get_error_string(rc) : "RCCL error");
  return mvd_fail(msg.c_str());
}
}  // namespace

int mvd_comm_unique_id(mvd_rccl_id* id_out) {
  RcclApi* a = rccl_api();
  if (!a) return mvd_fail("mvd_comm_unique_id: librccl.so could not be opened");
  const int rc = a->get_unique_id(id_out);
  return rc ? rccl_fail(a, "ncclGetUniqueId", rc) : 0;
}

int mvd_comm_init(mvd_ctx* c, const mvd_rccl_id* id, int rank, int world) {
  if (!c || !id || world < 1 || rank < 0 || rank >= world) return mvd_fail("mvd_comm_init: bad arguments");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  RcclApi* a = rccl_api();
  if (!a) return mvd_fail("mvd_comm_init: librccl.so could not be opened");
  if (c->comm) {
    a->comm_destroy(c->comm);
    c->comm = nullptr;
  }
  const int rc = a->comm_init_rank(&c->comm, world, *id, rank);
  if (rc) {
    c->comm = nullptr;
    return rccl_fail(a, "ncclCommInitRank", rc);
  }
  c->comm_rank = rank;
  c->comm_world = world;
  return 0;
}

int mvd_comm_destroy(mvd_ctx* c) {
  if (!c || !c->comm) return 0;
  RcclApi* a = rccl_api();
  if (a) a->comm_destroy(c->comm);
  c->comm = nullptr;
  c->comm_world = 1;
  c->comm_rank = 0;
  return 0;
}

int mvd_exchange_view_features(mvd_ctx* c, const float* local, float* all, int n_local, void* stream) {
  if (!c || !c->comm) return mvd_fail("mvd_exchange_view_features: no communicator (mvd_comm_init)");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!local || !all || n_local <= 0 || c->mesh.Nv <= 0) return mvd_fail("mvd_exchange_view_features: bad arguments / no mesh is set");
  RcclApi* a = rccl_api();
  if (!a) return mvd_fail("mvd_exchange_view_features: librccl.so could not be opened");
  // `all` holds comm_world * n_local views: the step's partition is even (SyncDDIMSampler.view_range), so a rank count that does
  // not divide the configured view count, or a slice of another size, is a caller error and not a gather of some other shape
  if (c->v.num_views > 0 && (long)c->comm_world * n_local != c->v.num_views)
    return mvd_fail("mvd_exchange_view_features: comm_world * n_local does not equal the configured view count");
  const size_t count = (size_t)n_local * c->mesh.Nv * 16;  // fp32 elements this rank contributes: [n_local][Nv][16]
  const int rc = a->all_gather(local, all, count, /* ncclFloat32 */ 7, c->comm, S(stream));
  return rc ? rccl_fail(a, "ncclAllGather", rc) : 0;
}

int mvd_comm_all_reduce(mvd_ctx* c, float* buf, size_t count, void* stream) {
  if (!c || !c->comm) return mvd_fail("mvd_comm_all_reduce: no communicator (mvd_comm_init)");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!buf || count == 0) return mvd_fail("mvd_comm_all_reduce: bad arguments");
  RcclApi* a = rccl_api();
  if (!a) return mvd_fail("mvd_comm_all_reduce: librccl.so could not be opened");
  const int rc = a->all_reduce(buf, buf, count, /* ncclFloat32 */ 7, /* ncclSum */ 0, c->comm, S(stream));
  return rc ? rccl_fail(a, "ncclAllReduce", rc) : 0;
}

// DDP's reducer on the gradient arena, entirely behind the C ABI (train_morphable_diffusion.py:302-303).  phase 0, right after
// mvd_train_unet_step: every bucket's ranges are all-reduced (sum, in place) on `comm_stream`, each bucket behind its own event
// -- one host call for all 26 buckets, no Python and no torch.distributed per bucket.  phase 1, after the conditioner's backward:
// `comm_stream` waits for `stream`, reduces every arena range no bucket covered, `stream` waits for `comm_stream`, and the arena is
// scaled by 1 / world on `stream`.  The arithmetic per element is the flat all-reduce's: sum over ranks, then the scale.
int mvd_train_sync_gradients(mvd_ctx* c, int phase, void* comm_stream, void* stream) {
  if (!c || !c->comm) return mvd_fail("mvd_train_sync_gradients: no communicator (mvd_comm_init)");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c->arena_g || c->arena_n == 0) return mvd_fail("mvd_train_sync_gradients: no gradient arena (mvd_train_enable)");
  if (phase != 0 && phase != 1) return mvd_fail("mvd_train_sync_gradients: phase is 0 (start) or 1 (finish)");
  RcclApi* a = rccl_api();
  if (!a) return mvd_fail("mvd_train_sync_gradients: librccl.so could not be opened");
  hipStream_t cs = S(comm_stream), ms = S(stream);
  auto reduce = [&](size_t off, size_t n) -> int {
    const int rc = a->all_reduce(c->arena_g + off, c->arena_g + off, n, 7, 0, c->comm, cs);
    return rc ? rccl_fail(a, "ncclAllReduce", rc) : 0;
  };
  if (phase == 0) {
    for (int k = 0; k < c->n_buckets; ++k) {
      const mvd_ctx::GradBucket& b = c->buckets[k];
      if (b.ev) HIP_CHECK_RET(hipStreamWaitEvent(cs, b.ev, 0));
      for (size_t r = 0; r < b.off.size(); ++r) RET_IF(reduce(b.off[r], b.len[r]));
    }
    c->grad_sync_started = true;
    return 0;
  }
  if (!c->ev_grad_sync[0]) {
    HIP_CHECK_RET(hipEventCreateWithFlags(&c->ev_grad_sync[0], hipEventDisableTiming));
    HIP_CHECK_RET(hipEventCreateWithFlags(&c->ev_grad_sync[1], hipEventDisableTiming));
  }
  HIP_CHECK_RET(hipEventRecord(c->ev_grad_sync[0], ms));  // the conditioner's backward wrote the rest of the arena on `stream`
  HIP_CHECK_RET(hipStreamWaitEvent(cs, c->ev_grad_sync[0], 0));
  std::vector<std::pair<size_t, size_t>> spans;
  if (c->grad_sync_started)
    for (int k = 0; k < c->n_buckets; ++k)
      for (size_t r = 0; r < c->buckets[k].off.size(); ++r) spans.push_back({c->buckets[k].off[r], c->buckets[k].off[r] + c->buckets[k].len[r]});
  std::sort(spans.begin(), spans.end());
  size_t pos = 0;
  for (auto& sp : spans) {
    if (sp.first < pos) return mvd_fail("mvd_train_sync_gradients: gradient buckets overlap");
    if (sp.first > pos) RET_IF(reduce(pos, sp.first - pos));
    pos = sp.second;
  }
  if (pos < c->arena_n) RET_IF(reduce(pos, c->arena_n - pos));
  c->grad_sync_started = false;
  HIP_CHECK_RET(hipEventRecord(c->ev_grad_sync[1], cs));
  HIP_CHECK_RET(hipStreamWaitEvent(ms, c->ev_grad_sync[1], 0));
  return launch_scale_copy(c->arena_g, c->arena_n, 1.0f / (float)c->comm_world, c->arena_g, ms);
}

// ------------------------------------------------------------------------------------------ test hooks
int mvd_op_conv(mvd_ctx* c, const float* x_nchw, int B, int Cin, int H, int W, const float* w, const float* bias, int Cout,
                int ksize, int stride, int upsample, const float* resid_nchw, float* out_nchw, int force_splitk,
                void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int cpad = (Cin + 7) / 8 * 8, taps = ksize * ksize;
  const int Hv = H << upsample, Wv = W << upsample;
  const int Ho = (Hv - 1) / stride + 1, Wo = (Wv - 1) / stride + 1;
  float* xn = ws_alloc<float>(c, (size_t)B * H * W * cpad);
  half_t* wp = ws_alloc<half_t>(c, (size_t)taps * Cout * cpad);
  float* on = ws_alloc<float>(c, (size_t)B * Ho * Wo * Cout);
  float* rn = resid_nchw ? ws_alloc<float>(c, (size_t)B * Ho * Wo * Cout) : nullptr;
  WS_CHECK(xn && wp && on);
  RET_IF(launch_nchw_to_nhwc(x_nchw, B, Cin, H * W, xn, cpad, cpad, s));
  RET_IF(launch_pack_weight(w, Cout, cpad, taps, 0, 0, wp, s, Cin));
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
  ConvW cw;
  cw.w = wp; cw.bias = const_cast<float*>(bias); cw.N = Cout; cw.Cin = cpad; cw.taps = taps;
  GemmArgs g;
  g.a = xn; g.a_f32 = 1; g.lda = cpad; g.w = &cw; g.out = on; g.ldc = Cout; g.resid = rn; g.ldr = Cout;
  g.use_bias = bias != nullptr; g.force_splitk = force_splitk;
  if (cpad % 64 == 0) {  // exercise the fp16-source paths (incl. the LDS-halo 3x3 kernels) the UNet uses
    half_t* xh = ws_alloc<half_t>(c, (size_t)B * H * W * cpad);
    WS_CHECK(xh);
    RET_IF(launch_f32_to_f16(xn, xh, (size_t)B * H * W * cpad, s));
    g.a = xh;
    g.a_f32 = 0;
    const int bnx = Cout % 160 == 0 ? 160 : (Cout % 128 == 0 ? 128 : 0);
    if (taps == 9 && bnx && mvd_env_call::conv3x()) {  // ... and the conv3x form of the weights (k_conv3x.hip), as build_conv3x_streams does
      cw.wx = ws_alloc<half_t>(c, conv3x_stream_halfs(Cout, cpad, bnx));
      WS_CHECK(cw.wx);
      RET_IF(conv3x_pack(wp, Cout, cpad, bnx, cw.wx, s));
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
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  if (Cin % 8) return mvd_fail("op_conv3d: Cin must be a multiple of 8");
  const int Do = transposed ? 2 * D : (D - 1) / stride + 1, Ho = transposed ? 2 * H : (H - 1) / stride + 1,
            Wo = transposed ? 2 * W : (W - 1) / stride + 1;
  float* xn = ws_alloc<float>(c, (size_t)B * D * H * W * Cin);
  half_t* wp = ws_alloc<half_t>(c, (size_t)27 * Cout * Cin);
  float* on = ws_alloc<float>(c, (size_t)B * Do * Ho * Wo * Cout);
  WS_CHECK(xn && wp && on);
  RET_IF(launch_nchw_to_nhwc(x, B, Cin, D * H * W, xn, Cin, Cin, s));
  RET_IF(launch_pack_weight(w, Cout, Cin, 27, transposed, 0, wp, s, Cin));
  if (resid) RET_IF(launch_nchw_to_nhwc(resid, B, Cout, Do * Ho * Wo, on, Cout, Cout, s));
  ConvW cw;
  cw.w = wp; cw.bias = const_cast<float*>(bias); cw.N = Cout; cw.Cin = Cin; cw.taps = 27;
  GemmArgs g;
  g.a = xn; g.a_f32 = 1; g.lda = Cin; g.w = &cw; g.out = on; g.ldc = Cout; g.use_bias = bias != nullptr;
  if (resid) { g.resid = on; g.ldr = Cout; }
  if (Cin % 64 == 0) {  // fp16-source path (LDS-DMA implicit GEMM), as in the frustum network's inner layers
    half_t* xh = ws_alloc<half_t>(c, (size_t)B * D * H * W * Cin);
    WS_CHECK(xh);
    RET_IF(launch_f32_to_f16(xn, xh, (size_t)B * D * H * W * Cin, s));
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
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  if (K % 8) return mvd_fail("op_linear: K must be a multiple of 8");
  half_t* wp = ws_alloc<half_t>(c, (size_t)N * K);
  float* bp = ws_alloc<float>(c, (size_t)N);
  WS_CHECK(wp && bp);
  RET_IF(launch_pack_weight(w, N, K, 1, 0, geglu, wp, s, K));
  if (bias) {
    if (geglu) RET_IF(launch_permute_geglu_bias(bias, N, bp, s));
    else HIP_CHECK_RET(hipMemcpyAsync(bp, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
  }
  ConvW cw;
  cw.w = wp; cw.bias = bias ? bp : nullptr; cw.N = N; cw.Cin = K; cw.taps = 1;
  GemmArgs g;
  g.a = a; g.a_f32 = 1; g.lda = K; g.w = &cw; g.out = out; g.ldc = geglu ? N / 2 : N; g.geglu = geglu;
  g.use_bias = bias != nullptr;
  g.force_splitk = force_splitk;
  if (resid) {
    g.resid = resid; g.resid_f32 = 1; g.ldr = N;
  }
  if (a_half) {
    half_t* ah = ws_alloc<half_t>(c, (size_t)M * K);
    WS_CHECK(ah);
    RET_IF(launch_f32_to_f16(a, ah, (size_t)M * K, s));
    g.a = ah; g.a_f32 = 0;
  }
  RET_IF(run_linear(c, g, 1, M, s));
  return 0;
}

int mvd_op_group_norm(mvd_ctx* c, const float* x_nchw, int B, int C, int HW, int groups, const float* gamma,
                      const float* beta, float eps, int act, float* out_nchw, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
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
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk((size_t)B * HW * C)), dim3(256), 0, s, y, yf, (size_t)B * HW * C);
  RET_IF(launch_nhwc_to_nchw(yf, C, B, C, HW, out_nchw, s));
  return 0;
}

int mvd_op_layer_norm(mvd_ctx* c, const float* x, int rows, int C, const float* gamma, const float* beta, float* out,
                      void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  half_t* y = ws_alloc<half_t>(c, (size_t)rows * C);
  WS_CHECK(y);
  RET_IF(launch_layernorm(x, rows, C, gamma, beta, 1e-5f, y, s));
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk((size_t)rows * C)), dim3(256), 0, s, y, out, (size_t)rows * C);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int mvd_op_attention(mvd_ctx* c, const float* q, const float* k, const float* v, int B, int T, int heads, int d, float* out,
                     void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int C = heads * d, rows = B * T;
  half_t* qkv = ws_alloc<half_t>(c, (size_t)rows * 3 * C);
  half_t* o = ws_alloc<half_t>(c, (size_t)rows * C);
  WS_CHECK(qkv && o);
  hipLaunchKernelGGL(pack_qkv_rows_kernel, dim3(nblk((size_t)rows * C)), dim3(256), 0, s, q, k, v, rows, C, qkv);
  RET_IF(launch_attention(qkv, 3 * C, qkv + 2 * C, 3 * C, o, C, B, T, heads, d, s));
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk((size_t)rows * C)), dim3(256), 0, s, o, out, (size_t)rows * C);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// depth_attn_kernel on the caller's data (tests/test_gpu_depth_attn.py).  Everything the launch may touch is poisoned first: the
// context's pad columns (ldx > Cc) and one guard row behind z hold 0xFFFF halfs, NaN in fp16 and in bfloat16.
int mvd_op_depth_attn(mvd_ctx* c, const float* qk, const float* context, const float* fill_row, int n_cond, int HW, int D, int Cc,
                      int heads, int ldx, int split, int nfill, int check_only, float* out, float* hi_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c) return mvd_fail("null context");
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
  if (crows) hipLaunchKernelGGL(rows_f32_to_f16_ld_kernel, dim3(nblk(crows * Cc)), dim3(256), 0, s, context, crows, Cc, cn, ldx);
  if (nfill > 0) {
    if (split) RET_IF(launch_rows_f32_to_f16_split(fill_row, W4, 1, W4, fr, s));
    else RET_IF(launch_f32_to_f16(fill_row, fr, W4, s));
  }
  RET_IF(launch_depth_attn(qk, cn, z, n_cond, HW, D, Cc, heads, s, split, nfill, nfill > 0 ? fr : nullptr, ldx));
  const size_t n = (rows + 1) * W4;
  if (split) {  // the guard row's three blocks are all NaN: NaN != NaN, so it comes back NaN
    hipLaunchKernelGGL(split_rows_to_f32_kernel, dim3(nblk(n)), dim3(256), 0, s, z, (int)(rows + 1), W4, out);
    if (hi_out) hipLaunchKernelGGL(rows_f16_ld_to_f32_kernel, dim3(nblk(n)), dim3(256), 0, s, z, rows + 1, W4, 3 * W4, hi_out);
  } else {
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk(n)), dim3(256), 0, s, z, out, n);
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// backward-kernel hooks (tests/test_gpu_train_ops.py): each against torch.autograd of the same op
int mvd_op_attention_bwd(mvd_ctx* c, const float* q, const float* k, const float* v, const float* d_out, int B, int T, int heads, int d,
                         float* dq, float* dk, float* dv, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c) return mvd_fail("null context");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int C = heads * d, rows = B * T;
  half_t* qkv = ws_alloc<half_t>(c, (size_t)rows * 3 * C);
  half_t* o = ws_alloc<half_t>(c, (size_t)rows * C);
  half_t* do16 = ws_alloc<half_t>(c, (size_t)rows * C);
  half_t* dqkv = ws_alloc<half_t>(c, (size_t)rows * 3 * C);
  float* lse = ws_alloc<float>(c, (size_t)B * heads * T);
  float* delta = ws_alloc<float>(c, (size_t)B * heads * T);
  float* tmp = ws_alloc<float>(c, (size_t)rows * 3 * C);
  WS_CHECK(qkv && o && do16 && dqkv && lse && delta && tmp);
  hipLaunchKernelGGL(pack_qkv_rows_kernel, dim3(nblk((size_t)rows * C)), dim3(256), 0, s, q, k, v, rows, C, qkv);
  RET_IF(launch_attention(qkv, 3 * C, qkv + 2 * C, 3 * C, o, C, B, T, heads, d, s));
  RET_IF(bwd_cast_rows(d_out, C, rows, C, C, do16, s));
  RET_IF(bwd_attention(qkv, 3 * C, o, do16, C, dqkv, 3 * C, lse, delta, B, T, heads, d, s));
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk((size_t)rows * 3 * C)), dim3(256), 0, s, dqkv, tmp, (size_t)rows * 3 * C);
  HIP_CHECK_RET(hipGetLastError());
  float* outs[3] = {dq, dk, dv};
  for (int i = 0; i < 3; ++i)
    HIP_CHECK_RET(hipMemcpy2DAsync(outs[i], (size_t)C * 4, tmp + (size_t)i * C, (size_t)3 * C * 4, (size_t)C * 4, rows, hipMemcpyDeviceToDevice, s));
  return 0;
}

// x, dy, dx: [B, rows, C] channels-last
int mvd_op_group_norm_bwd(mvd_ctx* c, const float* x, const float* dy, int B, int rows, int C, int groups, const float* gamma,
                          const float* beta, float eps, int act, float* dx, float* dgamma, float* dbeta, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c) return mvd_fail("null context");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  // the slabbed form the training step uses; MVD_GN_BWD_ONE_BLOCK=1: the one-workgroup-per-(sample, group) kernel
  const bool one_block = mvd_env().gn_bwd_one_block;
  const int S = one_block ? 1 : bwd_gn_slabs(B, groups, rows);
  float* dg = ws_alloc<float>(c, (size_t)B * S * C);
  float* db = ws_alloc<float>(c, (size_t)B * S * C);
  float* part = ws_alloc<float>(c, (size_t)B * groups * S * 4);
  WS_CHECK(dg && db && part);
  if (one_block)
    RET_IF(bwd_group_norm(x, C, nullptr, 0, dy, C, B, rows, C, groups, gamma, beta, eps, act, dx, C, 0, dg, db, nullptr, s));
  else
    RET_IF(bwd_group_norm_slab(x, C, nullptr, 0, dy, C, B, rows, C, groups, gamma, beta, eps, act, dx, C, 0, part,
                               part + (size_t)B * groups * S * 2, dg, db, nullptr, S, s));
  RET_IF(bwd_sum_rows_add(dg, B * S, C, C, dgamma, 0, s));
  return bwd_sum_rows_add(db, B * S, C, C, dbeta, 0, s);
}

int mvd_op_layer_norm_bwd(mvd_ctx* c, const float* x, const float* dy, int rows, int C, const float* gamma, float* dx, float* dgamma,
                          float* dbeta, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c) return mvd_fail("null context");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  float* part = ws_alloc<float>(c, (size_t)bwd_ln_max_blocks() * 2 * C);
  WS_CHECK(part);
  int nb = 0;
  RET_IF(bwd_layer_norm(x, C, dy, C, rows, C, gamma, 1e-5f, dx, C, 0, part, &nb, s));
  RET_IF(bwd_sum_rows_add(part, nb, C, 2 * C, dgamma, 0, s));
  return bwd_sum_rows_add(part + C, nb, C, 2 * C, dbeta, 0, s);
}

int mvd_bench_conv(mvd_ctx* c, int B, int C, int H, int W, int Cout, int iters, float* ms_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const size_t na = (size_t)B * H * W * C, nw = (size_t)9 * Cout * C;
  half_t* a = ws_alloc<half_t>(c, na);
  half_t* w = ws_alloc<half_t>(c, nw);
  float* o = ws_alloc<float>(c, (size_t)B * H * W * Cout);
  WS_CHECK(a && w && o);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(nblk(na)), dim3(256), 0, s, a, na, 17u);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(nblk(nw)), dim3(256), 0, s, w, nw, 91u);
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
  hipEvent_t e0, e1;
  HIP_CHECK_RET(hipEventCreate(&e0));
  HIP_CHECK_RET(hipEventCreate(&e1));
  HIP_CHECK_RET(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) RET_IF(run_conv2d(c, g, B, H, W, 1, 0, s));
  HIP_CHECK_RET(hipEventRecord(e1, s));
  HIP_CHECK_RET(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_CHECK_RET(hipEventElapsedTime(&ms, e0, e1));
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  *ms_out = ms / (float)iters;
  return 0;
}

int mvd_vae_decode(mvd_ctx* c, const float* z, int B, int h, int w, float* out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  if (!z || !out || B <= 0) return mvd_fail("mvd_vae_decode: bad argument");
  return engine_vae_decode(c, z, B, h, w, out, S(stream));
}

int mvd_vae_encode(mvd_ctx* c, const float* x, int B, int H, int W, float* moments, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  if (!x || !moments || B <= 0) return mvd_fail("mvd_vae_encode: bad argument");
  return engine_vae_encode(c, x, B, H, W, moments, S(stream));
}

int mvd_clip_encode(mvd_ctx* c, const float* x, int B, int H, int W, float* out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c || !c->finalized) return mvd_fail("weights not finalized");
  if (!x || !out || B <= 0) return mvd_fail("mvd_clip_encode: bad argument");
  return engine_clip_encode(c, x, B, H, W, out, S(stream));
}

int mvd_clip_embed_dim(mvd_ctx* c) { return (c && c->finalized && c->clip.present) ? c->clip.embed : 0; }

int mvd_probe_config(mvd_ctx* c, int mode, const char* family, int stride) {
  if (!c) return mvd_fail("mvd_probe_config: null context");
  if (mode < 0 || mode > 2 || (mode == 2 && !family)) return mvd_fail("mvd_probe_config: bad mode");
  c->probe_mode = mode;
  c->probe_only = family ? family : "";
  c->probe_stride = stride > 1 ? stride : 1;
  if (mode) {  // a new measurement starts
    c->probe_used = 0;
    c->probe_counter = 0;
    c->probe_fam.clear();
    c->probe_empty.clear();
    c->probe_null.clear();
  }
  return 0;
}

int mvd_probe_report(mvd_ctx* c, char* buf, size_t cap) {
  if (!c || !buf || cap < 3) return mvd_fail("mvd_probe_report: bad argument");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  std::string out = "[";
  bool first = true;
  for (auto& kv : c->probe_fam) {
    double ms = 0.0;
    for (size_t slot : kv.second.ev) {
      HIP_CHECK_RET(hipEventSynchronize(c->probe_ev[slot + 1]));
      float t = 0.f;
      HIP_CHECK_RET(hipEventElapsedTime(&t, c->probe_ev[slot], c->probe_ev[slot + 1]));
      ms += t;
    }
    char line[512];
    snprintf(line, sizeof line,
             "%s{\"family\": \"%s\", \"launches\": %ld, \"sampled\": %ld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e, "
             "\"all_flops\": %.6e, \"all_bytes\": %.6e}",
             first ? "" : ", ", kv.first.c_str(), kv.second.launches, kv.second.sampled, ms, kv.second.s_flops, kv.second.s_bytes,
             kv.second.flops, kv.second.bytes);
    out += line;
    first = false;
  }
  if (!c->probe_empty.empty()) {  // what a bracket costs by itself (survey mode), as a pseudo-family
    double ms = 0.0;
    for (size_t e : c->probe_empty) {
      HIP_CHECK_RET(hipEventSynchronize(c->probe_ev[e + 1]));
      float t = 0.f;
      HIP_CHECK_RET(hipEventElapsedTime(&t, c->probe_ev[e], c->probe_ev[e + 1]));
      ms += t;
    }
    char line[256];
    snprintf(line, sizeof line,
             "%s{\"family\": \"(empty bracket)\", \"launches\": %zu, \"sampled\": %zu, \"ms\": %.6f, \"flops\": 0, \"bytes\": 0, "
             "\"all_flops\": 0, \"all_bytes\": 0}",
             first ? "" : ", ", c->probe_empty.size(), c->probe_empty.size(), ms);
    out += line;
  }
  if (!c->probe_null.empty()) {  // event overhead + dispatch latency of a launch (survey mode), as a pseudo-family
    double ms = 0.0;
    for (size_t e : c->probe_null) {
      HIP_CHECK_RET(hipEventSynchronize(c->probe_ev[e + 1]));
      float t = 0.f;
      HIP_CHECK_RET(hipEventElapsedTime(&t, c->probe_ev[e], c->probe_ev[e + 1]));
      ms += t;
    }
    char line[256];
    snprintf(line, sizeof line,
             "%s{\"family\": \"(null-kernel bracket)\", \"launches\": %zu, \"sampled\": %zu, \"ms\": %.6f, \"flops\": 0, \"bytes\": 0, "
             "\"all_flops\": 0, \"all_bytes\": 0}",
             out.size() > 1 ? ", " : "", c->probe_null.size(), c->probe_null.size(), ms);
    out += line;
  }
  out += "]";
  if (out.size() + 1 > cap) return mvd_fail("mvd_probe_report: buffer too small");
  memcpy(buf, out.c_str(), out.size() + 1);
  return 0;
}

int mvd_bench_linear(mvd_ctx* c, int M, int K, int N, int flags, int iters, float* ms_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
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
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(nblk(na)), dim3(256), 0, s, a, na, 17u);
  if (a32) hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk(na)), dim3(256), 0, s, a, a32, na);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(nblk(nw)), dim3(256), 0, s, w, nw, 91u);
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
  hipEvent_t e0, e1;
  HIP_CHECK_RET(hipEventCreate(&e0));
  HIP_CHECK_RET(hipEventCreate(&e1));
  float total = 0.f;
  if (cold) {
    for (int i = 0; i < iters; ++i) {
      HIP_CHECK_RET(hipMemsetAsync(flush, i & 0xFF, flush_bytes, s));
      HIP_CHECK_RET(hipEventRecord(e0, s));
      RET_IF(run_linear(c, g, nb, M, s));
      HIP_CHECK_RET(hipEventRecord(e1, s));
      HIP_CHECK_RET(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_CHECK_RET(hipEventElapsedTime(&ms, e0, e1));
      total += ms;
    }
  } else {
    HIP_CHECK_RET(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) RET_IF(run_linear(c, g, nb, M, s));
    HIP_CHECK_RET(hipEventRecord(e1, s));
    HIP_CHECK_RET(hipEventSynchronize(e1));
    HIP_CHECK_RET(hipEventElapsedTime(&total, e0, e1));
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  *ms_out = total / (float)iters;
  return 0;
}

int mvd_bench_group_norm(mvd_ctx* c, int B, int C, int HW, int groups, int flags, int iters, float* ms_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const size_t n = (size_t)B * HW * C;
  const int split = flags & 1, wo = split ? 3 : 1;
  float* x = ws_alloc<float>(c, n);
  half_t* tmp = ws_alloc<half_t>(c, n);
  half_t* y = ws_alloc<half_t>(c, n * wo);
  float* gb = ws_alloc<float>(c, (size_t)2 * C);
  WS_CHECK(x && tmp && y && gb);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(nblk(n)), dim3(256), 0, s, tmp, n, 29u);
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk(n)), dim3(256), 0, s, tmp, x, n);
  hipLaunchKernelGGL(fill_pattern_f16_kernel, dim3(nblk((size_t)2 * C)), dim3(256), 0, s, tmp, (size_t)2 * C, 5u);
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk((size_t)2 * C)), dim3(256), 0, s, tmp, gb, (size_t)2 * C);
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
  hipEvent_t e0, e1;
  HIP_CHECK_RET(hipEventCreate(&e0));
  HIP_CHECK_RET(hipEventCreate(&e1));
  HIP_CHECK_RET(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) {
    if (flags & 2) RET_IF(launch_gn_apply(x, C, B, HW, C, groups, nullptr, 0, partial, nslabs, nw.g, nw.b, 1e-5f, ACT_SILU, y, C * wo, s, split));
    else RET_IF(run_group_norm(c, x, C, B, HW, nw, groups, 1e-5f, ACT_SILU, nullptr, y, C * wo, s, 0, split));
  }
  HIP_CHECK_RET(hipEventRecord(e1, s));
  HIP_CHECK_RET(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_CHECK_RET(hipEventElapsedTime(&ms, e0, e1));
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  *ms_out = ms / (float)iters;
  return 0;
}

// The row-chain kernel (k_rowchain.hip) on fp32 operands in the reference's layouts: packs the weight stream, runs the kernel
// once (iters > 0: `iters` more times between two events -> *ms_out = mean milliseconds) and returns the result in fp32.
int mvd_op_st_tail(mvd_ctx* c, int C, int rows, int T, const float* ao, const float* xin, const float* rowbias, const float* w_ao,
                   const float* b_ao, const float* ln_g, const float* ln_b, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w_po, const float* b_po, const float* resid, float* out, int flags, int iters,
                   float* ms_out, void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c) return mvd_fail("null context");
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
    hipEvent_t e0, e1;
    HIP_CHECK_RET(hipEventCreate(&e0));
    HIP_CHECK_RET(hipEventCreate(&e1));
    HIP_CHECK_RET(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) RET_IF(launch_rowchain(p, C, has_ao, has_po, s));
    HIP_CHECK_RET(hipEventRecord(e1, s));
    HIP_CHECK_RET(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK_RET(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (ms_out) *ms_out = ms / (float)iters;
  }
  if (!has_po) {
    if (split) {  // [hi | lo | hi] rows -> hi + lo (NaN where the third block differs from the first)
      hipLaunchKernelGGL(split_rows_to_f32_kernel, dim3(nblk(n)), dim3(256), 0, s, oh, rows, C, out);
    } else {
      hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk(n)), dim3(256), 0, s, oh, out, n);
    }
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// The row-head kernel (k_rowchain.hip: proj_in -> t0, LayerNorm1, q | k | v) on fp32 operands in the reference's layouts, C = 320.
int mvd_op_st_head(mvd_ctx* c, int rows, int xp, const float* n0, const float* w_pi, const float* b_pi, const float* ln_g, const float* ln_b,
                   const float* w_q, const float* w_k, const float* w_v, float* t0_out, float* qkv_out, int iters, float* ms_out,
                   void* stream) {
  if (c && hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  if (!c) return mvd_fail("null context");
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
    hipEvent_t e0, e1;
    HIP_CHECK_RET(hipEventCreate(&e0));
    HIP_CHECK_RET(hipEventCreate(&e1));
    HIP_CHECK_RET(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) RET_IF(launch_rowhead(p, xp, s));
    HIP_CHECK_RET(hipEventRecord(e1, s));
    HIP_CHECK_RET(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK_RET(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (ms_out) *ms_out = ms / (float)iters;
  }
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk(3 * n)), dim3(256), 0, s, qkvh, qkv_out, 3 * n);
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
int ex_begin(mvd_ctx* c) {
  if (!c) return mvd_fail("null context");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  return 0;
}
int ex_poison(mvd_ctx* c, hipStream_t s) {
  const size_t o = (c->ws.off + 255) & ~(size_t)255;
  if (o < c->ws.size) HIP_CHECK_RET(hipMemsetAsync(c->ws.base + o, 0xFF, c->ws.size - o, s));
  return 0;
}
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
      half_t* rh = ws_alloc<half_t>(c, out_rows * e.ldr);
      WS_CHECK(rh);
      RET_IF(launch_f32_to_f16(e.resid, rh, out_rows * e.ldr, s));
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
  RET_IF(ex_begin(c));
  if (!a || !w) return mvd_fail("op_linear_ex: null operand");
  if (B <= 0 || rows <= 0 || rows % B || K <= 0 || (K & 7)) return mvd_fail("op_linear_ex: rows % B == 0 and K % 8 == 0 expected");
  const ExEpi e{bias, rowbias, resid, rb_ld, act, use_bias, out_f16, out_split, ldc, resid_f16, ldr, force_splitk, alpha,
                slabs, slabs_cap, defer_epilogue, sk_used, out};
  RET_IF(ex_epi_check("op_linear_ex", e, N, true));
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int Kp = xp ? 3 * K : K;
  half_t* wp = ws_alloc<half_t>(c, (size_t)N * Kp);
  WS_CHECK(wp);
  RET_IF(launch_pack_weight(w, N, Kp, 1, 0, 0, wp, s, K, xp ? 1 : 0));  // xp: [w_hi | w_hi | w_lo], as pack_conv does
  ConvW cw;
  cw.w = wp; cw.bias = const_cast<float*>(bias); cw.N = N; cw.Cin = Kp; cw.taps = 1; cw.xp = xp ? 1 : 0; cw.cin_l = K;
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
  if (poison) RET_IF(ex_poison(c, s));
  return op_sync("op_linear_ex", s, run_linear(c, g, B, rows, s));
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
  RET_IF(ex_begin(c));
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
  half_t* wp = ws_alloc<half_t>(c, (size_t)taps * Cout * Cp);
  WS_CHECK(wp);
  RET_IF(launch_pack_weight(w, Cout, Cp, taps, 0, 0, wp, s, Cin, xp ? 1 : 0));
  ConvW cw;
  cw.w = wp; cw.bias = const_cast<float*>(bias); cw.N = Cout; cw.Cin = Cp; cw.taps = taps; cw.xp = xp ? 1 : 0; cw.cin_l = Cin;
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
    RET_IF(conv3x_pack(wp, Cout, Cp, bnx, cw.wx, s));
    cw.wx_bn = bnx;
  }
  if (up_fold) {
    cw.w_up = ws_alloc<half_t>(c, (size_t)16 * Cout * Cin);
    WS_CHECK(cw.w_up);
    RET_IF(launch_pack_upconv_weight(w, Cout, Cin, cw.w_up, s));
  }
  RET_IF(ex_epi_fill(c, e, rows_out, Cout, g, s));
  if (sk_used) *sk_used = 1;
  if (poison) RET_IF(ex_poison(c, s));
  return op_sync("op_conv_ex", s, up_fold ? run_upconv2d(c, g, B, H, W, s) : run_conv2d(c, g, B, H, W, stride, upsample, s));
}

// x: nslab slabs of channels-last [B][rows][ld] fp32, slab_stride floats apart.  form 0: run_group_norm's own choice; form 1: the
// two-pass pair (launch_gn_stats + launch_gn_apply) called directly, which takes one slab and writes neither `mat` nor fp32.
// out: [B * rows + 1][ldo] halfs (split = 1: [hi | lo | hi] rows; split = 2: fp32 rows of ldo / 2 floats); mat: [B * rows + 1][ldm].
int mvd_op_group_norm_ex(mvd_ctx* c, const float* x, int B, int rows, int C, int ld, int groups, const float* gamma, const float* beta,
                         float eps, int act, int form, const float* preadd, int pld, int split, int nslab, size_t slab_stride,
                         const float* bias2, const float* resid, int ldr, float* mat, int ldm, int ldo, int poison, void* out,
                         void* stream) {
  RET_IF(ex_begin(c));
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
    if (poison) RET_IF(ex_poison(c, s));
    return op_sync("op_group_norm_ex", s,
                   run_group_norm(c, x, ld, B, rows, n, groups, eps, act, preadd, o, ldo, s, pld, split, nslab, slab_stride, bias2, resid,
                                  ldr, mat, ldm));
  }
  if (C > 2560 || groups > 32 || (C & 3) || (ld & 3) || (ldo & 3) || (preadd && (pld & 3)))
    return mvd_fail("op_group_norm_ex: the two-pass form takes C <= 2560, groups <= 32 and C, ld, ldo, pld % 4 == 0");
  float* partial = ws_alloc<float>(c, (size_t)B * gn_max_slabs() * groups * 2);
  WS_CHECK(partial);
  if (poison) RET_IF(ex_poison(c, s));
  int nsl = 0;
  int rc = launch_gn_stats(x, ld, B, rows, C, groups, preadd, pld, partial, &nsl, s);
  if (!rc) rc = launch_gn_apply(x, ld, B, rows, C, groups, preadd, pld, partial, nsl, gamma, beta, eps, act, o, ldo, s, split);
  return op_sync("op_group_norm_ex", s, rc);
}

// plain == 0: launch_layernorm_slabs with every LnSlabs field (mat [rows + 1][C] is required); plain != 0: launch_layernorm on
// one slab, where only the fp16 copy `raw` ([rows + 1][ld_raw] halfs, may be NULL) is left of them.  out: [rows + 1][C] halfs.
int mvd_op_layer_norm_slabs(mvd_ctx* c, const float* slabs, int nslab, size_t slab_stride, int rows, int C, const float* bias,
                            const float* rowbias, int rb_ld, int T, const float* resid, int ldr, const float* gamma, const float* beta,
                            float eps, int plain, int ld_raw, int poison, float* mat, void* raw, void* out, void* stream) {
  RET_IF(ex_begin(c));
  if (!slabs || !gamma || !beta || !out) return mvd_fail("op_layer_norm_slabs: null operand");
  if (rows <= 0 || C <= 0 || nslab < 1 || T < 1) return mvd_fail("op_layer_norm_slabs: bad argument");
  if (raw && ld_raw < C) return mvd_fail("op_layer_norm_slabs: ld_raw >= C expected");
  hipStream_t s = S(stream);
  if (plain) {
    if (nslab != 1 || bias || rowbias || resid || mat) return mvd_fail("op_layer_norm_slabs: the plain LayerNorm takes one slab and writes no mat");
    if (poison) RET_IF(ex_poison(c, s));
    return op_sync("op_layer_norm_slabs", s, launch_layernorm(slabs, rows, C, gamma, beta, eps, (half_t*)out, s, (half_t*)raw, ld_raw));
  }
  if (!mat) return mvd_fail("op_layer_norm_slabs: mat is required");
  if (nslab > 1 && slab_stride < (size_t)rows * C) return mvd_fail("op_layer_norm_slabs: slabs overlap");
  if ((rowbias && rb_ld < C) || (resid && ldr < C)) return mvd_fail("op_layer_norm_slabs: rb_ld, ldr >= C expected");
  if (poison) RET_IF(ex_poison(c, s));
  return op_sync("op_layer_norm_slabs", s,
                 launch_layernorm_slabs(slabs, nslab, slab_stride, rows, C, bias, rowbias, rb_ld, T, resid, ldr, mat, gamma, beta, eps,
                                        (half_t*)out, s, (half_t*)raw, ld_raw));
}

// The three steps of the folded GroupNorm(proj_context(volume)) (engine_unet.hip: ctx_fold) on caller data: x [B * rps][K], w [N][K],
// N / cpg groups.  partials [B * rps / 256 + 1][N / cpg][2], scale and shift [B + 1][N], out [B * rps + 1][N] halfs.
int mvd_op_folded_group_norm(mvd_ctx* c, const float* x, int B, int rps, int K, const float* w, int N, int cpg, const float* gamma,
                             const float* beta, float eps, int poison, float* partials, float* scale, float* shift, void* out,
                             void* stream) {
  RET_IF(ex_begin(c));
  if (!x || !w || !gamma || !beta || !partials || !scale || !shift || !out) return mvd_fail("op_folded_group_norm: null operand");
  if (B <= 0 || rps <= 0 || K <= 0 || (K & 7) || N <= 0 || (N & 3)) return mvd_fail("op_folded_group_norm: K % 8 == 0 and N % 4 == 0 expected");
  // what ctx_fold_ok asks of a context level
  if (rps % 256 || (cpg != 8 && cpg != 16 && cpg != 32) || (long)B * rps < 512)
    return mvd_fail("op_folded_group_norm: rps % 256 == 0, 8 / 16 / 32 channels per group and at least 512 rows expected");
  if (N % cpg || N / cpg > 32) return mvd_fail("op_folded_group_norm: at most 32 whole groups expected");
  hipStream_t s = S(stream);
  WsScope ws_scope(c);
  const int rows = B * rps, G = N / cpg, ntile = rps / 256;
  half_t* wp = ws_alloc<half_t>(c, (size_t)N * K);
  half_t* xh = ws_alloc<half_t>(c, (size_t)rows * K);
  WS_CHECK(wp && xh);
  RET_IF(launch_pack_weight(w, N, K, 1, 0, 0, wp, s, K, 0));
  RET_IF(launch_f32_to_f16(x, xh, (size_t)rows * K, s));
  ConvW cw;
  cw.w = wp; cw.N = N; cw.Cin = K; cw.taps = 1;
  if (poison) RET_IF(ex_poison(c, s));
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
  return op_sync("op_folded_group_norm", s, rc);
}

// softmax_rows_kernel (out_f32 == 0: fp16 probabilities) / softmax_rows_f32_kernel on [rows][cols] fp32 scores; out [rows + 1][cols]
int mvd_op_softmax_rows(mvd_ctx* c, const float* scores, int rows, int cols, int out_f32, void* out, void* stream) {
  RET_IF(ex_begin(c));
  if (!scores || !out || rows <= 0 || cols <= 0) return mvd_fail("op_softmax_rows: bad argument");
  hipStream_t s = S(stream);
  return op_sync("op_softmax_rows", s,
                 out_f32 ? launch_softmax_rows_f32(scores, rows, cols, (float*)out, s) : launch_softmax_rows(scores, rows, cols, (half_t*)out, s));
}

// launch_rows_f32_to_f16_split: fp32 rows `lda` floats apart -> [hi | lo | hi] rows of 3 C halfs; out [rows + 1][3 C]
int mvd_op_rows_split(mvd_ctx* c, const float* x, int lda, int rows, int C, void* out, void* stream) {
  RET_IF(ex_begin(c));
  if (!x || !out || rows <= 0 || C <= 0 || lda < C) return mvd_fail("op_rows_split: bad argument");
  hipStream_t s = S(stream);
  return op_sync("op_rows_split", s, launch_rows_f32_to_f16_split(x, lda, rows, C, (half_t*)out, s));
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
}  // namespace

int mvd_op_attention_ex(mvd_ctx* c, const float* q, const float* k, const float* v, int B, int T, int heads, int d, int Tstride,
                        int ld_pad, int xcd, float* out, void* stream) {
  RET_IF(ex_begin(c));
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
  hipLaunchKernelGGL(pack_qkv_image_kernel, dim3(nblk((size_t)B * T * C)), dim3(256), 0, s, q, k, v, B, T, C, Ts, ld, qkv);
  int rc = launch_attention(qkv, ld, qkv + 2 * C, ld, o, C, B, T, heads, d, s, Ts, xcd);
  if (!rc) {
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk(rows * C)), dim3(256), 0, s, o, out, rows * C);
    if (hipGetLastError() != hipSuccess) rc = mvd_fail("op_attention_ex: launch failed");
  }
  return op_sync("op_attention_ex", s, rc);
}

int mvd_op_attention_bwd_ex(mvd_ctx* c, const float* q, const float* k, const float* v, const float* d_out, int B, int T, int heads,
                            int d, float* dq, float* dk, float* dv, float* lse, float* delta, float* o_out, void* stream) {
  RET_IF(ex_begin(c));
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
  hipLaunchKernelGGL(pack_qkv_image_kernel, dim3(nblk(rows * C)), dim3(256), 0, s, q, k, v, B, T, C, T, 3 * C, qkv);
  int rc = launch_attention(qkv, 3 * C, qkv + 2 * C, 3 * C, o, C, B, T, heads, d, s);
  if (!rc) rc = bwd_cast_rows(d_out, C, (long)rows, C, C, do16, s);
  if (!rc) rc = bwd_attention(qkv, 3 * C, o, do16, C, dqkv, 3 * C, lse_d, delta_d, B, T, heads, d, s);
  if (!rc) {
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk((rows + 1) * 3 * C)), dim3(256), 0, s, dqkv, tmp, (rows + 1) * 3 * C);
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk((rows + 1) * C)), dim3(256), 0, s, o, o_out, (rows + 1) * C);
    if (hipGetLastError() != hipSuccess) rc = mvd_fail("op_attention_bwd_ex: launch failed");
    float* outs[3] = {dq, dk, dv};
    for (int i = 0; i < 3 && !rc; ++i)
      if (hipMemcpy2DAsync(outs[i], (size_t)C * 4, tmp + (size_t)i * C, (size_t)3 * C * 4, (size_t)C * 4, rows + 1, hipMemcpyDeviceToDevice, s) != hipSuccess)
        rc = mvd_fail("op_attention_bwd_ex: copy failed");
    if (!rc && (hipMemcpyAsync(lse, lse_d, nstat * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
                hipMemcpyAsync(delta, delta_d, nstat * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess))
      rc = mvd_fail("op_attention_bwd_ex: copy failed");
  }
  return op_sync("op_attention_bwd_ex", s, rc);
}

// the DepthTransformer's fp32 training kernels (csrc/k_train.hip) on the caller's device buffers; no context
int mvd_op_train_depth_attn(const float* q, const float* k, const float* v, int R, int HW, int D, int hn, int hd, float* attn, float* z,
                            void* stream) {
  if (!q || !k || !v || !attn || !z) return mvd_fail("mvd_op_train_depth_attn: null argument");
  if (R <= 0 || HW <= 0 || R % HW || D <= 0 || hn <= 0 || hd <= 0) return mvd_fail("mvd_op_train_depth_attn: R a positive multiple of HW, D, hn, hd >= 1 expected");
  hipStream_t s = S(stream);
  return op_sync("mvd_op_train_depth_attn", s, train_depth_fwd(q, k, v, R, HW, D, hn, hd, 1.0f / sqrtf((float)hd), attn, z, s));
}

int mvd_op_train_depth_attn_bwd(const float* q, const float* k, const float* v, const float* attn, const float* dz, int R, int HW, int D,
                                int hn, int hd, float* dq, float* dk, float* dv, void* stream) {
  if (!q || !k || !v || !attn || !dz || !dq || !dk || !dv) return mvd_fail("mvd_op_train_depth_attn_bwd: null argument");
  if (R <= 0 || HW <= 0 || R % HW || D <= 0 || hn <= 0 || hd <= 0) return mvd_fail("mvd_op_train_depth_attn_bwd: R a positive multiple of HW, D, hn, hd >= 1 expected");
  hipStream_t s = S(stream);
  return op_sync("mvd_op_train_depth_attn_bwd", s,
                 train_depth_bwd(q, k, v, attn, dz, R, HW, D, hn, hd, 1.0f / sqrtf((float)hd), dq, dk, dv, s));
}

int mvd_op_train_im2col3(const float* x, int B, int H, int W, int C, float* col, void* stream) {
  if (!x || !col || B <= 0 || H <= 0 || W <= 0 || C <= 0) return mvd_fail("mvd_op_train_im2col3: bad argument");
  hipStream_t s = S(stream);
  return op_sync("mvd_op_train_im2col3", s, train_im2col3(x, B, H, W, C, col, s));
}

int mvd_op_train_col2im3(const float* dcol, int B, int H, int W, int C, float* dx, void* stream) {
  if (!dcol || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0) return mvd_fail("mvd_op_train_col2im3: bad argument");
  hipStream_t s = S(stream);
  return op_sync("mvd_op_train_col2im3", s, train_col2im3(dcol, B, H, W, C, dx, s));
}

int mvd_op_train_perm_w3(const float* src, int N, int C, int to_mat, float* dst, void* stream) {
  if (!src || !dst || N <= 0 || C <= 0) return mvd_fail("mvd_op_train_perm_w3: bad argument");
  hipStream_t s = S(stream);
  return op_sync("mvd_op_train_perm_w3", s, train_perm_w3(src, N, C, to_mat, dst, s));
}

}  // extern "C"
