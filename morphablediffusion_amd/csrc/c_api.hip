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
#include "mesh.h"
#include "rowchain.h"

static thread_local std::string g_err;
int mvd_fail(const char* msg) {
  g_err = msg ? msg : "unknown error";
  return -1;
}
const char* mvd_error_text() { return g_err.c_str(); }

namespace {

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

inline hipStream_t S(void* s) { return (hipStream_t)s; }
inline int nblk(size_t n) { size_t g = (n + 255) / 256; return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }

}  // namespace

// The UNet batch of B samples x TN views (morphable_diffusion.py:133-147): every conditional row first -- sample by sample, view
// by view --, then (copies == 2) the unconditional copies in the same order, half_off = B * TN rows further on.  timesteps: HOST.
int launch_build_cfg_batch(const float* x_noisy, const float* x_input, const float* clip, const int64_t* timesteps, int B, int TN, int HW,
                           int dim, int copies, float* xin, float* ctx, int64_t* tt, hipStream_t s) {
  const long half_off = (long)B * TN;
  for (int b = 0; b < B; ++b) {
    hipLaunchKernelGGL(build_cfg_input_kernel, dim3(nblk((size_t)copies * TN * HW * 8)), dim3(256), 0, s,
                       x_noisy + (size_t)b * TN * 4 * HW, x_input + (size_t)b * 4 * HW, TN, HW, copies, xin + (size_t)b * TN * HW * 8,
                       half_off);
    hipLaunchKernelGGL(build_cfg_context_kernel, dim3(nblk((size_t)copies * TN * dim)), dim3(256), 0, s, clip + (size_t)b * dim, TN, dim,
                       copies, ctx + (size_t)b * TN * dim, tt + (size_t)b * TN, timesteps[b], half_off);
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

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

// ---- UV texture atlases (csrc/k_mesh_uv.hip): no context, the caller's device buffers
int mvd_op_mesh_vertex_normals(const float* verts, const int32_t* faces, const int32_t* inc_ptr, const int32_t* inc_face, int F, int Nv,
                               int Nf, float* normals, int32_t* bad_faces, void* stream) {
  RET_IF(mesh_vertex_normals_check("mvd_op_mesh_vertex_normals", verts, faces, inc_ptr, inc_face, F, Nv, Nf, normals, bad_faces));
  hipStream_t s = S(stream);
  int rc = launch_mesh_vertex_normals(verts, faces, inc_ptr, inc_face, F, Nv, Nf, normals, bad_faces, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_vertex_normals: stream synchronisation failed");
  return rc;
}

int mvd_op_mesh_texel_bake(const void* images, int dtype, int layout, const int32_t* face_id, const int32_t* pix_key, const float* K,
                           const float* RT, const float* centres, float z_near, const float* verts, const float* normals,
                           const int32_t* faces, const int32_t* uv_xy, const int32_t* face_uv, const int32_t* tex_face, int N, int Nv,
                           int Nf, int Nt, int H, int W, int Ht, int Wt, float power, int bias, int two_sided, float fill_r, float fill_g,
                           float fill_b, float* texture, float* weight_sum, int32_t* n_seen, float* spread, unsigned char* visible,
                           float* pos, int32_t* txy, int32_t* tkey, void* stream) {
  MeshBakeArgs a;
  a.images = images, a.face_id = face_id, a.pix_key = pix_key, a.faces = faces, a.uv_xy = uv_xy, a.face_uv = face_uv, a.tex_face = tex_face;
  a.K = K, a.RT = RT, a.centres = centres, a.verts = verts, a.normals = normals;
  a.dtype = dtype, a.layout = layout, a.N = N, a.Nv = Nv, a.Nf = Nf, a.Nt = Nt, a.H = H, a.W = W, a.Ht = Ht, a.Wt = Wt, a.bias = bias;
  a.two_sided = two_sided, a.z_near = z_near, a.power = power, a.fill[0] = fill_r, a.fill[1] = fill_g, a.fill[2] = fill_b;
  a.texture = texture, a.weight_sum = weight_sum, a.spread = spread, a.pos = pos, a.n_seen = n_seen, a.txy = txy, a.tkey = tkey;
  a.visible = visible;
  RET_IF(mesh_texel_bake_check("mvd_op_mesh_texel_bake", a));
  hipStream_t s = S(stream);
  int rc = launch_mesh_texel_bake(a, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_texel_bake: stream synchronisation failed");
  return rc;
}

int mvd_op_mesh_texture_dilate(const float* texture, const unsigned char* valid, int Ht, int Wt, int passes, float* texture_out,
                               unsigned char* valid_out, void* stream) {
  RET_IF(mesh_texture_dilate_check("mvd_op_mesh_texture_dilate", texture, valid, Ht, Wt, passes, texture_out, valid_out));
  hipStream_t s = S(stream);
  void* scratch = nullptr;  // the second buffer of the ping-pong lives for this call only
  if (passes > 1) HIP_CHECK_RET(hipMalloc(&scratch, mesh_texture_dilate_scratch_bytes(Ht, Wt)));
  int rc = launch_mesh_texture_dilate(texture, valid, Ht, Wt, passes, texture_out, valid_out, scratch, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_texture_dilate: stream synchronisation failed");
  if (scratch) hipFree(scratch);
  return rc;
}

int mvd_op_mesh_render_uv(const int32_t* xy, const int32_t* key, const int32_t* face_id, const int32_t* faces, const int32_t* face_uv,
                          const float* uv, const float* texture, int N, int Nv, int Nf, int Nt, int H, int W, int Ht, int Wt, int layout,
                          float bg_r, float bg_g, float bg_b, float* images, void* stream) {
  RET_IF(mesh_render_uv_check("mvd_op_mesh_render_uv", xy, key, face_id, faces, face_uv, uv, texture, N, Nv, Nf, Nt, H, W, Ht, Wt, layout,
                              images));
  hipStream_t s = S(stream);
  int rc = launch_mesh_render_uv(xy, key, face_id, faces, face_uv, uv, texture, N, Nv, Nf, Nt, H, W, Ht, Wt, layout, bg_r, bg_g, bg_b, images,
                                 s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_render_uv: stream synchronisation failed");
  return rc;
}

// ---- closest point on a mesh (csrc/k_closest.hip): no context, the caller's device buffers
int mvd_mesh_closest_slabs(int Q, int Nf) { return mesh_closest_slabs(Q, Nf); }

int mvd_op_mesh_closest_point(const float* queries, const float* query_normals, const float* verts, const int32_t* faces, int Q, int Nv, int Nf,
                              float cos_min, float max_dist2, int slabs, uint64_t* key, int32_t* face, float* bary, float* point, float* dist2,
                              void* stream) {
  RET_IF(mesh_closest_check("mvd_op_mesh_closest_point", queries, verts, faces, Q, Nv, Nf, cos_min, max_dist2, slabs,
                            (const unsigned long long*)key, face, bary, point, dist2));
  hipStream_t s = S(stream);
  int rc = launch_mesh_closest_point(queries, query_normals, verts, faces, Q, Nv, Nf, cos_min, max_dist2, slabs, (unsigned long long*)key, face,
                                     bary, point, dist2, s);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail("mvd_op_mesh_closest_point: stream synchronisation failed");
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
  RET_IF(launch_build_cfg_batch(x_noisy, x_input, clip, timesteps, B, TN, HW, u.context_dim, copies, xin, ctx, tt, s));
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

}  // extern "C"
