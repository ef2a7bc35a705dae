// The 2-D multi-view landmark term of the fitter and the per-view contour landmarks -- include/mvd.h: mvd_op_morph_project,
// _project_bwd, mvd_op_morph_fit_data_2d, mvd_op_morph_contour_select, _contour_landmarks, _contour_bwd, and the stages
// mvd_morph_fit_2d_run enqueues.  fp32 on the vector ALU, every sum in an order fixed by indices alone, no atomics: two calls agree
// bit for bit, and frame f of a batch equals the same frame computed alone.  The projection is mesh.h's mesh_project_uv, the chain
// of mvd_op_mesh_project: one pixel convention in the library.
// Launches:
//   morph_project_kernel        a thread per (frame, view, point): uv and the validity of the observation.
//   morph_project_bwd_kernel    a thread per (frame, point) walks the views in index order: g_point = sum_c J_c^T g_uv.
//   morph_fit2d_stats_kernel    a thread per (frame, point), the points being the M static landmarks followed by the Md contour
//                               landmarks, walks the views in index order: uv of every observation, and over the counted ones the
//                               sums of w |r|^2, of w and their number; these are summed per block of 256 points in the vertex
//                               phase's shape (a butterfly over each wave, ((s0 + s1) + s2) + s3 over the 4 waves).
//   morph_fit2d_energy_kernel   one wave per frame: a lane-strided ascending sum over the blocks and one butterfly; W_f, 1 / W_f,
//                               E2_f and the count.
//   morph_fit2d_grad_kernel     a thread per (frame, point) walks the views again: g_lmk as the sum over the views, g_dyn per view.
//   morph_contour_select_kernel a thread per (frame, view): the yaw of the head in the view and the row of the contour table.
//   morph_contour_landmarks_kernel   a thread per (frame, view, contour landmark), mvd_op_morph_landmarks' fma form on the selected row.
//   morph_contour_bwd_kernel    a gather: a thread per (frame, listed vertex) walks the vertex's (row, landmark, corner) entries in
//                               table order and, inside an entry, the views in index order.
#include <cmath>

#include "mesh.h"
#include "morph.h"

namespace {

constexpr int T2 = 256;
static_assert(MORPH_2D_BLOCK == T2, "2-D term geometry");

__device__ inline float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__device__ inline bool finite5(float a, float b, float c, float d, float e) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d) && isfinite(e);
}

// g_point = J^T (du, dv) for u = (k0 X + k1 Y) / Z + k2, v = k4 Y / Z + k5, cam = R p + t: the chain differentiated as written
__device__ inline void project_pullback(const float* __restrict__ r, const float* __restrict__ k, float X, float Y, float Z, float du,
                                        float dv, float g[3]) {
  const float iz = 1.0f / Z;
  const float gX = (du * k[0]) * iz;
  const float gY = fmaf(du, k[1], dv * k[4]) * iz;
  const float gZ = (0.0f - fmaf(du, fmaf(k[1], Y, k[0] * X), dv * (k[4] * Y))) * (iz * iz);
#pragma unroll
  for (int j = 0; j < 3; ++j) g[j] = fmaf(r[8 + j], gZ, fmaf(r[4 + j], gY, r[j] * gX));
}

__global__ __launch_bounds__(T2) void morph_project_kernel(const float* __restrict__ points, const float* __restrict__ K,
                                                           const float* __restrict__ RT, int cam_frames, int F, int C, int M, float z_near,
                                                           float* __restrict__ uv, int* __restrict__ valid) {
  const int i = blockIdx.x * T2 + threadIdx.x;  // F C M 2 < 2^31
  if (i >= F * C * M) return;
  const int m = i % M, c = (i / M) % C, f = i / (M * C);
  const size_t cam = (size_t)(cam_frames == 1 ? 0 : f) * C + c;
  const float* p = points + ((size_t)f * M + m) * 3;
  float X, Y, Z, u, v;
  mesh_project_uv(RT + cam * 12, K + cam * 9, p[0], p[1], p[2], X, Y, Z, u, v);
  uv[(size_t)i * 2] = u, uv[(size_t)i * 2 + 1] = v;
  valid[i] = Z >= z_near && finite5(X, Y, Z, u, v);
}

__global__ __launch_bounds__(T2) void morph_project_bwd_kernel(const float* __restrict__ points, const float* __restrict__ K,
                                                               const float* __restrict__ RT, int cam_frames, const float* __restrict__ g_uv,
                                                               int F, int C, int M, float z_near, float* __restrict__ g_points) {
  const int i = blockIdx.x * T2 + threadIdx.x;
  if (i >= F * M) return;
  const int f = i / M, m = i - f * M;
  const float* p = points + (size_t)i * 3;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int c = 0; c < C; ++c) {
    const size_t cam = (size_t)(cam_frames == 1 ? 0 : f) * C + c;
    const float *r = RT + cam * 12, *k = K + cam * 9;
    float X, Y, Z, u, v, g[3];
    mesh_project_uv(r, k, p[0], p[1], p[2], X, Y, Z, u, v);
    if (!(Z >= z_near && finite5(X, Y, Z, u, v))) continue;
    const float* gu = g_uv + (((size_t)f * C + c) * M + m) * 2;
    project_pullback(r, k, X, Y, Z, gu[0], gu[1], g);
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] = acc[j] + g[j];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) g_points[(size_t)i * 3 + j] = acc[j];
}

struct Fit2dArgs {
  const float *lmk, *dyn_lmk, *K, *RT, *target_uv, *weight, *dyn_target_uv, *dyn_weight, *E_add;
  float *uv, *dyn_uv, *part, *E2, *g_lmk, *g_dyn;
  int* n_valid;
  int cam_frames, target_frames, F, C, M, Md, nblk;
  float z_near, px_scale, lambda2;
};

// observation (f, c, point i): point i < M is static landmark i, point M + d contour landmark d of view c
struct Obs2d {
  const float *r, *k;
  float X, Y, Z, u, v, w, tu, tv;
  size_t at;  // its index in uv / dyn_uv (and g_dyn)
  bool dyn, ok;
};

__device__ inline void observe(const Fit2dArgs& a, int f, int c, int i, Obs2d& o) {
  const size_t cam = (size_t)(a.cam_frames == 1 ? 0 : f) * a.C + c;
  o.r = a.RT + cam * 12, o.k = a.K + cam * 9;
  o.dyn = i >= a.M;
  const int n = o.dyn ? a.Md : a.M, j = o.dyn ? i - a.M : i;
  const float* p = o.dyn ? a.dyn_lmk + (((size_t)f * a.C + c) * n + j) * 3 : a.lmk + ((size_t)f * n + j) * 3;
  o.at = ((size_t)f * a.C + c) * n + j;
  const size_t tat = ((size_t)(a.target_frames == 1 ? 0 : f) * a.C + c) * n + j;
  mesh_project_uv(o.r, o.k, p[0], p[1], p[2], o.X, o.Y, o.Z, o.u, o.v);
  const float* wp = o.dyn ? a.dyn_weight : a.weight;
  o.w = wp ? wp[tat] : 1.0f;
  o.ok = o.w > 0.0f && o.Z >= a.z_near && finite5(o.X, o.Y, o.Z, o.u, o.v);
  o.tu = 0.0f, o.tv = 0.0f;
  if (o.ok) {  // the target of an observation that does not count is never read
    const float* tp = (o.dyn ? a.dyn_target_uv : a.target_uv) + tat * 2;
    o.tu = tp[0], o.tv = tp[1];
  }
}

__global__ __launch_bounds__(T2) void morph_fit2d_stats_kernel(Fit2dArgs a) {
  __shared__ float s_red[2][T2 / 64];
  __shared__ int s_cnt[T2 / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int blk = blockIdx.x, f = blockIdx.y;
  const int i = blk * T2 + t, n_pts = a.M + (a.dyn_lmk ? a.Md : 0);
  float e = 0.0f, ws = 0.0f;
  int cnt = 0;
  if (i < n_pts) {
    for (int c = 0; c < a.C; ++c) {
      Obs2d o;
      observe(a, f, c, i, o);
      float* dst = (o.dyn ? a.dyn_uv : a.uv) + o.at * 2;
      dst[0] = o.u, dst[1] = o.v;
      if (!o.ok) continue;
      const float ru = a.px_scale * (o.u - o.tu), rv = a.px_scale * (o.v - o.tv);
      e = fmaf(o.w, fmaf(rv, rv, ru * ru), e);
      ws = ws + o.w;
      ++cnt;
    }
  }
  e = wave_sum(e), ws = wave_sum(ws);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if (lane == 0) s_red[0][w] = e, s_red[1][w] = ws, s_cnt[w] = cnt;
  __syncthreads();
  if (t == 0) {
    const size_t at = (size_t)blk * a.F + f, sec = (size_t)a.nblk * a.F;
    a.part[at] = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
    a.part[sec + at] = ((s_red[1][0] + s_red[1][1]) + s_red[1][2]) + s_red[1][3];
    a.part[2 * sec + at] = __int_as_float(((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]);
  }
}

__global__ __launch_bounds__(64) void morph_fit2d_energy_kernel(Fit2dArgs a) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const size_t sec = (size_t)a.nblk * a.F;
  float ev = 0.0f, wv = 0.0f;
  int cnt = 0;
  for (int b = lane; b < a.nblk; b += 64) {
    const size_t at = (size_t)b * a.F + f;
    ev += a.part[at], wv += a.part[sec + at], cnt += __float_as_int(a.part[2 * sec + at]);
  }
  ev = wave_sum(ev), wv = wave_sum(wv);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if (lane == 0) {
    const float inv = wv > 0.0f ? 1.0f / wv : 0.0f;
    a.part[3 * sec + f] = inv;
    const float e2 = __fmul_rn(a.lambda2, __fmul_rn(ev, inv));
    a.E2[f] = a.E_add ? __fadd_rn(a.E_add[f], e2) : e2;
    a.n_valid[f] = cnt;
  }
}

__global__ __launch_bounds__(T2) void morph_fit2d_grad_kernel(Fit2dArgs a) {
  const int blk = blockIdx.x, f = blockIdx.y;
  const int i = blk * T2 + threadIdx.x, n_pts = a.M + (a.dyn_lmk ? a.Md : 0);
  if (i >= n_pts) return;
  const float inv = a.part[(size_t)3 * a.nblk * a.F + f];
  const float c0 = (2.0f * a.lambda2) * (a.px_scale * a.px_scale);
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int c = 0; c < a.C; ++c) {
    Obs2d o;
    observe(a, f, c, i, o);
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (o.ok && inv != 0.0f) {
      const float cf = (c0 * o.w) * inv;
      project_pullback(o.r, o.k, o.X, o.Y, o.Z, cf * (o.u - o.tu), cf * (o.v - o.tv), g);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = acc[j] + g[j];
    }
    if (o.dyn) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a.g_dyn[o.at * 3 + j] = g[j];
    }
  }
  if (i < a.M) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.g_lmk[((size_t)f * a.M + i) * 3 + j] = acc[j];
  }
}

// the row of a table of R = 2 h + 1 rows for a yaw in degrees: y = rint(min(yaw, h)); y >= 0: y; -h <= y < 0: h - y; y < -h: 2 h
__device__ inline int contour_row(float yaw_deg, int R) {
  if (!isfinite(yaw_deg)) return 0;
  const int h = (R - 1) / 2;
  const int y = (int)rintf(fmaxf(fminf(yaw_deg, (float)h), -1.0f - (float)h));
  return y >= 0 ? y : (y < -h ? 2 * h : h - y);
}

__global__ __launch_bounds__(T2) void morph_contour_select_kernel(const float* __restrict__ A, const float* __restrict__ RT, int cam_frames,
                                                                  int F, int C, int J, int neck_joint, int R, int* __restrict__ row,
                                                                  float* __restrict__ yaw) {
  const int i = blockIdx.x * T2 + threadIdx.x;
  if (i >= F * C) return;
  const int f = i / C, c = i - f * C;
  const float* G = A + ((size_t)f * J + neck_joint) * 12;
  const float* r = RT + ((size_t)(cam_frames == 1 ? 0 : f) * C + c) * 12;
  const float g0 = G[0], g1 = G[4], g2 = G[8];  // the first column of G_neck
  // Mx = S R_c G with S = diag(1, -1, -1): its first column
  const float m00 = fmaf(r[2], g2, fmaf(r[1], g1, r[0] * g0));
  const float m10 = 0.0f - fmaf(r[6], g2, fmaf(r[5], g1, r[4] * g0));
  const float m20 = 0.0f - fmaf(r[10], g2, fmaf(r[9], g1, r[8] * g0));
  const float deg = (0.0f - atan2f(0.0f - m20, sqrtf(fmaf(m10, m10, m00 * m00)))) * 57.29577951308232f;
  row[i] = contour_row(deg, R);
  if (yaw) yaw[i] = deg;
}

__global__ __launch_bounds__(T2) void morph_contour_landmarks_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                     const int* __restrict__ dyn_face, const float* __restrict__ dyn_bary,
                                                                     const int* __restrict__ row, int F, int C, int V, int Nf, int R, int Md,
                                                                     float* __restrict__ out) {
  const int i = blockIdx.x * T2 + threadIdx.x;  // F C Md 3 < 2^31
  if (i >= F * C * Md) return;
  const int d = i % Md, fc = i / Md, f = fc / C;
  const int rw = row[fc];
  float o[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if ((unsigned)rw < (unsigned)R) {
    const int e = rw * Md + d, face = dyn_face[e];
    if ((unsigned)face < (unsigned)Nf) {
      const int i0 = faces[(size_t)face * 3], i1 = faces[(size_t)face * 3 + 1], i2 = faces[(size_t)face * 3 + 2];
      if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
        const float w0 = dyn_bary[(size_t)e * 3], w1 = dyn_bary[(size_t)e * 3 + 1], w2 = dyn_bary[(size_t)e * 3 + 2];
        const float* x = verts + (size_t)f * V * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = fmaf(w2, x[(size_t)i2 * 3 + k], fmaf(w1, x[(size_t)i1 * 3 + k], w0 * x[(size_t)i0 * 3 + k]));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = o[k];
}

// g_verts is read and written at the listed vertices only, each by its own thread: the caller has put g_in (or zeros) there
__global__ __launch_bounds__(T2) void morph_contour_bwd_kernel(const float* __restrict__ g_dyn, const int* __restrict__ row,
                                                               const int* __restrict__ ct_vert, const int* __restrict__ ct_ptr,
                                                               const int* __restrict__ ct_ent, const float* __restrict__ dyn_bary, int F, int C,
                                                               int V, int R, int Md, int n_list, int n_ent, float* g_verts) {
  const int i = blockIdx.x * T2 + threadIdx.x;
  if (i >= F * n_list) return;
  const int f = i / n_list, li = i - f * n_list;
  const int v = ct_vert[li];
  if ((unsigned)v >= (unsigned)V) return;
  float* dst = g_verts + ((size_t)f * V + v) * 3;
  float acc[3] = {dst[0], dst[1], dst[2]};
  const int q0 = min(max(ct_ptr[li], 0), n_ent), q1 = min(max(ct_ptr[li + 1], q0), n_ent);
  const int* rw_f = row + (size_t)f * C;
  for (int q = q0; q < q1; ++q) {
    const int ent = ct_ent[q];  // (row * Md + landmark) * 3 + corner
    if ((unsigned)ent >= (unsigned)(3 * R * Md)) continue;
    const int rw = ent / (3 * Md), d = (ent / 3) % Md;
    const float wt = dyn_bary[ent];
    for (int c = 0; c < C; ++c) {
      if (rw_f[c] != rw) continue;
      const float* g = g_dyn + (((size_t)f * C + c) * Md + d) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] = fmaf(wt, g[k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) dst[k] = acc[k];
}

int camera_check(const char* who, const float* K, const float* RT, int cam_frames, int F, int C, float z_near) {
  if (!K || !RT) return morph_fail(who, ": null argument");
  if (F < 1 || C < 1) return morph_fail(who, ": F and C must be at least 1");
  if (cam_frames != 1 && cam_frames != F) return morph_fail(who, ": the cameras must have 1 or F frames");
  if (!(z_near > 0.0f) || !std::isfinite(z_near)) return morph_fail(who, ": z_near must be positive and finite");
  return 0;
}

}  // namespace

int morph_project_check(const char* who, const float* points, const float* K, const float* RT, int cam_frames, int F, int C, int M,
                        float z_near, const void* out_a, const void* out_b) {
  if (!points || !out_a || !out_b) return morph_fail(who, ": null argument");
  if (int rc = camera_check(who, K, RT, cam_frames, F, C, z_near)) return rc;
  if (M < 1) return morph_fail(who, ": M must be at least 1");
  if (morph_too_big(F, C, 1) || morph_too_big((long long)F * C, M, 3)) return morph_fail(who, ": F C M 2 must be below 2^31");
  return 0;
}

int launch_morph_project(const float* points, const float* K, const float* RT, int cam_frames, int F, int C, int M, float z_near, float* uv,
                         int* valid, hipStream_t s) {
  hipLaunchKernelGGL(morph_project_kernel, dim3((F * C * M + T2 - 1) / T2), dim3(T2), 0, s, points, K, RT, cam_frames, F, C, M, z_near, uv,
                     valid);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_morph_project_bwd(const float* points, const float* K, const float* RT, int cam_frames, const float* g_uv, int F, int C, int M,
                             float z_near, float* g_points, hipStream_t s) {
  hipLaunchKernelGGL(morph_project_bwd_kernel, dim3((F * M + T2 - 1) / T2), dim3(T2), 0, s, points, K, RT, cam_frames, g_uv, F, C, M, z_near,
                     g_points);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_fit_data_2d_check(const char* who, const Morph2dTerm& t, int F, int M, int Md, const float* lmk, const float* dyn_lmk,
                            const float* uv, const float* dyn_uv, const float* part, const float* E2, const int* n_valid, const float* g_lmk,
                            const float* g_dyn) {
  if (!lmk || !t.target_uv || !uv || !part || !E2 || !n_valid || !g_lmk) return morph_fail(who, ": null argument");
  if (int rc = camera_check(who, t.K, t.RT, t.cam_frames, F, t.C, t.z_near)) return rc;
  if (M < 1) return morph_fail(who, ": M must be at least 1");
  if (F > 65535) return morph_fail(who, ": at most 65535 frames");
  if (t.target_frames != 1 && t.target_frames != F) return morph_fail(who, ": the 2-D target must have 1 or F frames");
  if (!(t.px_scale >= 0.0f) || !std::isfinite(t.px_scale) || !(t.lambda2 >= 0.0f) || !std::isfinite(t.lambda2))
    return morph_fail(who, ": px_scale and lambda2 must be finite and not negative");
  if (morph_too_big(F, t.C, 1) || morph_too_big((long long)F * t.C, M, 3)) return morph_fail(who, ": F C M 2 must be below 2^31");
  const bool dyn = dyn_lmk || t.dyn_target_uv || t.dyn_weight || dyn_uv || g_dyn;
  if (dyn) {
    if (!dyn_lmk || !t.dyn_target_uv || !dyn_uv || !g_dyn) return morph_fail(who, ": the contour landmarks, their target and their outputs go together");
    if (Md < 1) return morph_fail(who, ": Md must be at least 1 with contour landmarks");
    if (morph_too_big((long long)F * t.C, Md, 3)) return morph_fail(who, ": F C Md 3 must be below 2^31");
    if (morph_too_big(1, (long long)M + Md, 1)) return morph_fail(who, ": M + Md must be below 2^31");
  }
  return 0;
}

int launch_morph_fit_data_2d(const Morph2dTerm& t, int F, int M, int Md, const float* lmk, const float* dyn_lmk, const float* E_add,
                             float* uv, float* dyn_uv, float* part, float* E2, int* n_valid, float* g_lmk, float* g_dyn, hipStream_t s) {
  Fit2dArgs a;
  a.lmk = lmk, a.dyn_lmk = dyn_lmk, a.K = t.K, a.RT = t.RT, a.target_uv = t.target_uv, a.weight = t.weight;
  a.dyn_target_uv = t.dyn_target_uv, a.dyn_weight = t.dyn_weight, a.E_add = E_add;
  a.uv = uv, a.dyn_uv = dyn_uv, a.part = part, a.E2 = E2, a.g_lmk = g_lmk, a.g_dyn = g_dyn, a.n_valid = n_valid;
  a.cam_frames = t.cam_frames, a.target_frames = t.target_frames, a.F = F, a.C = t.C, a.M = M, a.Md = dyn_lmk ? Md : 0;
  a.nblk = morph_2d_blocks(M, a.Md);
  a.z_near = t.z_near, a.px_scale = t.px_scale, a.lambda2 = t.lambda2;
  hipLaunchKernelGGL(morph_fit2d_stats_kernel, dim3(a.nblk, F), dim3(T2), 0, s, a);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(morph_fit2d_energy_kernel, dim3(F), dim3(64), 0, s, a);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(morph_fit2d_grad_kernel, dim3(a.nblk, F), dim3(T2), 0, s, a);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_contour_select_check(const char* who, const float* A, const float* RT, int cam_frames, int F, int C, int J, int neck_joint, int R,
                               const int* row) {
  if (!A || !RT || !row) return morph_fail(who, ": null argument");
  if (F < 1 || C < 1) return morph_fail(who, ": F and C must be at least 1");
  if (cam_frames != 1 && cam_frames != F) return morph_fail(who, ": the cameras must have 1 or F frames");
  if (J < 1 || J > MORPH_MAX_JOINTS) return morph_fail(who, ": J must be in 1..64");
  if (neck_joint < 0 || neck_joint >= J) return morph_fail(who, ": neck_joint must be in 0..J-1");
  if (R < 1 || R % 2 == 0) return morph_fail(who, ": the contour table must have an odd number of rows, at least 1");
  if (morph_too_big(F, C, 12)) return morph_fail(who, ": F C 12 must be below 2^31");
  return 0;
}

int launch_morph_contour_select(const float* A, const float* RT, int cam_frames, int F, int C, int J, int neck_joint, int R, int* row,
                                float* yaw, hipStream_t s) {
  hipLaunchKernelGGL(morph_contour_select_kernel, dim3((F * C + T2 - 1) / T2), dim3(T2), 0, s, A, RT, cam_frames, F, C, J, neck_joint, R, row,
                     yaw);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_contour_landmarks_check(const char* who, const float* verts, const int* faces, const int* dyn_face, const float* dyn_bary,
                                  const int* row, int F, int C, int V, int Nf, int R, int Md, const float* out) {
  if (!verts || !faces || !dyn_face || !dyn_bary || !row || !out) return morph_fail(who, ": null argument");
  if (F < 1 || C < 1 || V < 1 || Nf < 1 || R < 1 || Md < 1) return morph_fail(who, ": F, C, V, Nf, R and Md must be at least 1");
  if (morph_too_big(F, V, 3) || morph_too_big(F, C, 1) || morph_too_big((long long)F * C, Md, 3) || morph_too_big(R, Md, 3))
    return morph_fail(who, ": F V 3, F C Md 3 and R Md 3 must be below 2^31");
  return 0;
}

int launch_morph_contour_landmarks(const float* verts, const int* faces, const int* dyn_face, const float* dyn_bary, const int* row, int F,
                                   int C, int V, int Nf, int R, int Md, float* out, hipStream_t s) {
  hipLaunchKernelGGL(morph_contour_landmarks_kernel, dim3((F * C * Md + T2 - 1) / T2), dim3(T2), 0, s, verts, faces, dyn_face, dyn_bary, row,
                     F, C, V, Nf, R, Md, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_contour_bwd_check(const char* who, const float* g_dyn, const int* row, const int* ct_vert, const int* ct_ptr, const int* ct_ent,
                            const float* dyn_bary, int F, int C, int V, int R, int Md, int n_list, int n_ent, const float* g_verts) {
  if (!g_dyn || !row || !ct_vert || !ct_ptr || !ct_ent || !dyn_bary || !g_verts) return morph_fail(who, ": null argument");
  if (F < 1 || C < 1 || V < 1 || R < 1 || Md < 1 || n_list < 1 || n_ent < 1)
    return morph_fail(who, ": F, C, V, R, Md and the table's counts must be at least 1");
  if (morph_too_big(F, V, 3) || morph_too_big(F, C, 1) || morph_too_big((long long)F * C, Md, 3) || morph_too_big(R, Md, 3) ||
      morph_too_big(F, n_list, 1))
    return morph_fail(who, ": F V 3, F C Md 3, R Md 3 and F times the listed vertices must be below 2^31");
  return 0;
}

int launch_morph_contour_bwd(const float* g_dyn, const int* row, const int* ct_vert, const int* ct_ptr, const int* ct_ent,
                             const float* dyn_bary, int F, int C, int V, int R, int Md, int n_list, int n_ent, float* g_verts, hipStream_t s) {
  hipLaunchKernelGGL(morph_contour_bwd_kernel, dim3((F * n_list + T2 - 1) / T2), dim3(T2), 0, s, g_dyn, row, ct_vert, ct_ptr, ct_ent, dyn_bary,
                     F, C, V, R, Md, n_list, n_ent, g_verts);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
