// The morphable-model backward and fitter of the C ABI (include/mvd.h: mvd_op_morph_skin_ex, the mvd_op_morph_*_bwd and
// mvd_op_morph_fit_* entries, mvd_morph_fit_run) over k_morph.hip and k_morph_bwd.hip.  No context, the caller's device buffers;
// parents is a host array.  The per-op entries end in hooks.h's hook_sync; the loops of mvd_morph_fit_run and mvd_morph_fit_scan_run
// (the same loop with the target replaced by closest points of a scan, csrc/k_closest.hip) synchronise once.  Further down: the
// 2-D multi-view landmark term with the per-view contour landmarks (k_morph_2d.hip) and its loop, mvd_morph_fit_2d_run.
#include <algorithm>

#include "hooks.h"
#include "mesh.h"
#include "morph.h"

namespace {

inline hipStream_t S(void* s) { return (hipStream_t)s; }

// the float offsets of mvd_morph_fit_run's workspace, every buffer on a 256-byte boundary
struct FitLayout {
  size_t j_rest, rot, joints, A, coef, verts, blend, lmk, g_y, g_b, part_a, part_c, e_part, g, total;
  FitLayout(int F, int V, int NB, int J, int M) {
    const size_t f = (size_t)F, L = (size_t)NB + 9 * (size_t)(J - 1), P = (size_t)NB + 3 * (size_t)J + 3;
    size_t o = 0;
    auto take = [&](size_t n) {
      const size_t at = o;
      o += (n + 63) & ~(size_t)63;
      return at;
    };
    j_rest = take(f * J * 3), rot = take(f * J * 9), joints = take(f * J * 3), A = take(f * J * 12), coef = take(f * L);
    verts = take(f * V * 3), blend = take(f * V * 3), lmk = take(f * (size_t)M * 3), g_y = take(f * V * 3), g_b = take(f * V * 3);
    part_a = take((size_t)morph_bwd_chunks(V) * f * ((size_t)J * 12 + 3)), part_c = take((size_t)morph_bwd_slabs(V) * f * L);
    e_part = take((size_t)morph_bwd_chunks(V) * f), g = take(f * P);
    total = o;
  }
};

// mvd_morph_fit_scan_run's workspace: the fitter's, then the correspondence buffers (key: 8 bytes a query)
struct ScanLayout {
  FitLayout fit;
  size_t normals, corr_point, key, bary, dist2, w_part, bad, total;
  ScanLayout(int F, int V, int NB, int J, int M) : fit(F, V, NB, J, M) {
    const size_t n = (size_t)F * V;
    size_t o = fit.total;
    auto take = [&](size_t k) {
      const size_t at = o;
      o += (k + 63) & ~(size_t)63;
      return at;
    };
    normals = take(n * 3), corr_point = take(n * 3), key = take(n * 2), bary = take(n * 3), dist2 = take(n);
    w_part = take(((size_t)morph_bwd_chunks(V) + 1) * F), bad = take(1);
    total = o;
  }
};

// mvd_morph_fit_2d_run's workspace: the fitter's, then the 2-D term's buffers (row: one int32 a (frame, view))
struct Fit2dLayout {
  FitLayout fit;
  size_t g_y0, uv, dyn_lmk, dyn_uv, g_lmk, g_dyn, row, part, e3, total;
  Fit2dLayout(int F, int V, int NB, int J, int M, int Md, int C) : fit(F, V, NB, J, M) {
    const size_t fc = (size_t)F * C;
    size_t o = fit.total;
    auto take = [&](size_t k) {
      const size_t at = o;
      o += (k + 63) & ~(size_t)63;
      return at;
    };
    g_y0 = take((size_t)F * V * 3), uv = take(fc * M * 2), dyn_lmk = take(fc * Md * 3), dyn_uv = take(fc * Md * 2);
    g_lmk = take((size_t)F * M * 3), g_dyn = take(fc * Md * 3), row = take(fc);
    part = take((3 * (size_t)morph_2d_blocks(M, Md) + 1) * F), e3 = take(F);
    total = o;
  }
};

}  // namespace

int mvd_morph_bwd_chunks(int V) { return V < 1 ? 0 : morph_bwd_chunks(V); }
int mvd_morph_bwd_slabs(int V) { return V < 1 ? 0 : morph_bwd_slabs(V); }

int mvd_op_morph_skin_ex(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                         const float* post, const float* transl, int F, int V, int L, int NB, int J, float* verts, float* blend,
                         void* stream) {
  RET_IF(morph_skin_check("mvd_op_morph_skin_ex", basis, v_template, coef, weights, A, F, V, L, NB, J, verts));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_skin_ex", s,
                   launch_morph_skin_ex(basis, v_template, coef, weights, A, post, transl, 3, F, V, L, J, verts, blend, s));
}

int mvd_op_morph_skin_bwd(const float* g_y, const float* post, const float* weights, const float* A, const float* blend,
                          const float* basis, int F, int V, int L, int NB, int J, float* g_b, float* part_a, float* part_c, void* stream) {
  RET_IF(morph_skin_bwd_check("mvd_op_morph_skin_bwd", g_y, weights, A, blend, basis, F, V, L, NB, J, g_b, part_a, part_c));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_skin_bwd", s, launch_morph_skin_bwd(g_y, post, weights, A, blend, basis, F, V, L, J, g_b, part_a, part_c, s));
}

int mvd_op_morph_pose_bwd(const float* pose, const float* j_rest, const float* A, const float* j_dirs, const int32_t* parents,
                          const float* part_a, int nchunk, const float* part_c, int nslab, const float* g_joints, int F, int NB, int J,
                          float* g_betas, float* g_pose, float* g_transl, void* stream) {
  RET_IF(morph_pose_bwd_check("mvd_op_morph_pose_bwd", pose, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, F, NB, J, g_betas,
                              g_pose, g_transl));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_pose_bwd", s,
                   launch_morph_pose_bwd(pose, 3 * J, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, g_joints, F, NB, J, g_betas,
                                         NB, g_pose, 3 * J, g_transl, 3, s));
}

int mvd_op_morph_landmarks_bwd(const float* g_lmk, const float* g_in, const int32_t* csr_ptr, const int32_t* csr_ent, const float* lmk_bary,
                               int F, int V, int M, int n_ent, float* g_verts, void* stream) {
  RET_IF(morph_landmarks_bwd_check("mvd_op_morph_landmarks_bwd", g_lmk, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_verts));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_landmarks_bwd", s,
                   launch_morph_landmarks_bwd(g_lmk, g_in, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_verts, s));
}

int mvd_op_morph_fit_data(const float* verts, const float* target, int target_frames, const float* vertex_weight, float inv_vw_sum,
                          const float* lmk, const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale,
                          const int32_t* csr_ptr, const int32_t* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent,
                          float* g_y, float* e_part, float* E, void* stream) {
  RET_IF(morph_fit_data_check("mvd_op_morph_fit_data", verts, target, target_frames, lmk, target_lmk, target_lmk_frames, csr_ptr, csr_ent,
                              lmk_bary, F, V, M, n_ent, g_y, e_part, E));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_fit_data", s,
                   launch_morph_fit_data(verts, target, target_frames, vertex_weight, inv_vw_sum, lmk, target_lmk, target_lmk_frames,
                                         lmk_weight, lmk_scale, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_y, e_part, E, s));
}

int mvd_op_morph_fit_data_corr(const float* verts, const float* corr_point, const int32_t* corr_face, const float* vertex_weight,
                               const float* lmk, const float* target_lmk, int target_lmk_frames, const float* lmk_weight, float lmk_scale,
                               const int32_t* csr_ptr, const int32_t* csr_ent, const float* lmk_bary, int F, int V, int M, int n_ent,
                               float* g_y, float* e_part, float* w_part, float* E, int32_t* n_matched, void* stream) {
  RET_IF(morph_fit_data_corr_check("mvd_op_morph_fit_data_corr", verts, corr_point, corr_face, lmk, target_lmk, target_lmk_frames, csr_ptr,
                                   csr_ent, lmk_bary, F, V, M, n_ent, g_y, e_part, w_part, E, n_matched));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_fit_data_corr", s,
                   launch_morph_fit_data_corr(verts, corr_point, corr_face, vertex_weight, lmk, target_lmk, target_lmk_frames, lmk_weight,
                                              lmk_scale, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_y, e_part, w_part, E, n_matched, s));
}

int mvd_op_morph_fit_update(float* p, const float* g, float* m, float* v, const float* lr, const float* lam, const float* p0, int F, int P,
                            int step, float beta1, float beta2, float eps, void* stream) {
  RET_IF(morph_fit_update_check("mvd_op_morph_fit_update", p, g, m, v, lr, lam, p0, F, P, step, beta1, beta2, eps));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_fit_update", s, launch_morph_fit_update(p, g, m, v, lr, lam, p0, F, P, step, beta1, beta2, eps, s));
}

int mvd_morph_fit_workspace(int F, int V, int NB, int J, int M, int64_t* floats) {
  if (!floats) return morph_fail("mvd_morph_fit_workspace", ": null argument");
  if (F < 1 || V < 1 || NB < 1 || J < 1 || J > MORPH_MAX_JOINTS || M < 0)
    return morph_fail("mvd_morph_fit_workspace", ": F, V and NB must be at least 1, J in 1..64, M at least 0");
  *floats = (int64_t)FitLayout(F, V, NB, J, M).total;
  return 0;
}

int mvd_morph_fit_run(const float* basis, const float* v_template, const float* weights, const float* j_template, const float* j_dirs,
                      const int32_t* parents, const float* post, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary,
                      const int32_t* csr_ptr, const int32_t* csr_ent, int F, int V, int NB, int J, int Nf, int M, int n_ent,
                      const float* target, int target_frames, const float* vertex_weight, float inv_vw_sum, const float* target_lmk,
                      int target_lmk_frames, const float* lmk_weight, float lmk_scale, float* p, float* m, float* v, const float* lr,
                      const float* lam, const float* p0, int iters, int step0, float beta1, float beta2, float eps, float* workspace,
                      size_t workspace_floats, float* loss_history, void* stream) {
  const char* who = "mvd_morph_fit_run";
  if (!workspace || !loss_history) return morph_fail(who, ": null argument");
  if (iters < 1 || step0 < 0 || step0 > 0x7fffffff - iters) return morph_fail(who, ": iters must be at least 1 and step0 at least 0");
  if (F < 1 || V < 1 || NB < 1 || J < 1 || J > MORPH_MAX_JOINTS || M < 0)
    return morph_fail(who, ": F, V and NB must be at least 1, J in 1..64, M at least 0");
  if (morph_too_big(iters, F, 1)) return morph_fail(who, ": iters F must be below 2^31");
  const bool use_lmk = target_lmk != nullptr;
  if (use_lmk && (!faces || !lmk_face || M < 1 || Nf < 1)) return morph_fail(who, ": a landmark target needs the landmark embedding");
  const FitLayout lay(F, V, NB, J, use_lmk ? M : 0);
  if (workspace_floats < lay.total) return morph_fail(who, ": the workspace is smaller than mvd_morph_fit_workspace says");
  const int L = NB + 9 * (J - 1), P = NB + 3 * J + 3, nchunk = morph_bwd_chunks(V), nslab = morph_bwd_slabs(V);
  float* w = workspace;
  float *j_rest = w + lay.j_rest, *rot = w + lay.rot, *joints = w + lay.joints, *A = w + lay.A, *coef = w + lay.coef;
  float *verts = w + lay.verts, *blend = w + lay.blend, *lmk = use_lmk ? w + lay.lmk : nullptr, *g_y = w + lay.g_y, *g_b = w + lay.g_b;
  float *part_a = w + lay.part_a, *part_c = w + lay.part_c, *e_part = w + lay.e_part, *g = w + lay.g;
  // every argument error of every stage, before the first HIP call
  RET_IF(morph_pose_check(who, p, p, j_template, j_dirs, parents, F, NB, J, j_rest, rot, coef, joints, A));
  RET_IF(morph_skin_check(who, basis, v_template, coef, weights, A, F, V, L, NB, J, verts));
  if (use_lmk) RET_IF(morph_landmarks_check(who, verts, faces, lmk_face, lmk_bary, F, V, Nf, M, lmk));
  RET_IF(morph_fit_data_check(who, verts, target, target_frames, lmk, target_lmk, target_lmk_frames, csr_ptr, csr_ent, lmk_bary, F, V, M,
                              n_ent, g_y, e_part, loss_history));
  RET_IF(morph_skin_bwd_check(who, g_y, weights, A, blend, basis, F, V, L, NB, J, g_b, part_a, part_c));
  RET_IF(morph_pose_bwd_check(who, p, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, F, NB, J, g, g, g));
  RET_IF(morph_fit_update_check(who, p, g, m, v, lr, lam, p0, F, P, step0 + 1, beta1, beta2, eps));
  hipStream_t s = S(stream);
  int rc = 0;
  // p [F][P] = betas | pose | translation: the stages read and write it in place through row strides
  const float *betas = p, *pose = p + NB, *transl = p + NB + 3 * J;
  for (int it = 0; it < iters && !rc; ++it) {
    rc = launch_morph_pose_ex(betas, P, pose, P, j_template, j_dirs, parents, F, NB, J, j_rest, rot, nullptr, joints, A, coef, s);
    if (!rc) rc = launch_morph_skin_ex(basis, v_template, coef, weights, A, post, transl, P, F, V, L, J, verts, blend, s);
    if (!rc && use_lmk) rc = launch_morph_landmarks(verts, faces, lmk_face, lmk_bary, F, V, Nf, M, lmk, s);
    if (!rc)
      rc = launch_morph_fit_data(verts, target, target_frames, vertex_weight, inv_vw_sum, lmk, target_lmk, target_lmk_frames, lmk_weight,
                                 lmk_scale, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_y, e_part, loss_history + (size_t)it * F, s);
    if (!rc) rc = launch_morph_skin_bwd(g_y, post, weights, A, blend, basis, F, V, L, J, g_b, part_a, part_c, s);
    if (!rc)
      rc = launch_morph_pose_bwd(pose, P, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, nullptr, F, NB, J, g, P, g + NB, P,
                                 g + NB + 3 * J, P, s);
    if (!rc) rc = launch_morph_fit_update(p, g, m, v, lr, lam, p0, F, P, step0 + it + 1, beta1, beta2, eps, s);
  }
  return hook_sync(who, s, rc);
}

int mvd_morph_2d_blocks(int M, int Md) { return M < 0 || Md < 0 || M + (long long)Md < 1 ? 0 : morph_2d_blocks(M, Md); }

int mvd_op_morph_project(const float* points, const float* K, const float* RT, int cam_frames, int F, int C, int M, float z_near, float* uv,
                         int32_t* valid, void* stream) {
  RET_IF(morph_project_check("mvd_op_morph_project", points, K, RT, cam_frames, F, C, M, z_near, uv, valid));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_project", s, launch_morph_project(points, K, RT, cam_frames, F, C, M, z_near, uv, valid, s));
}

int mvd_op_morph_project_bwd(const float* points, const float* K, const float* RT, int cam_frames, const float* g_uv, int F, int C, int M,
                             float z_near, float* g_points, void* stream) {
  RET_IF(morph_project_check("mvd_op_morph_project_bwd", points, K, RT, cam_frames, F, C, M, z_near, g_uv, g_points));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_project_bwd", s, launch_morph_project_bwd(points, K, RT, cam_frames, g_uv, F, C, M, z_near, g_points, s));
}

int mvd_op_morph_fit_data_2d(const float* lmk, const float* dyn_lmk, const float* K, const float* RT, int cam_frames, const float* target_uv,
                             const float* weight, const float* dyn_target_uv, const float* dyn_weight, int target_frames, int F, int C, int M,
                             int Md, float z_near, float px_scale, float lambda2, const float* E_add, float* uv, float* dyn_uv, float* part,
                             float* E2, int32_t* n_valid, float* g_lmk, float* g_dyn, void* stream) {
  const Morph2dTerm t{K, RT, target_uv, weight, dyn_target_uv, dyn_weight, cam_frames, target_frames, C, z_near, px_scale, lambda2};
  RET_IF(morph_fit_data_2d_check("mvd_op_morph_fit_data_2d", t, F, M, Md, lmk, dyn_lmk, uv, dyn_uv, part, E2, n_valid, g_lmk, g_dyn));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_fit_data_2d", s,
                   launch_morph_fit_data_2d(t, F, M, Md, lmk, dyn_lmk, E_add, uv, dyn_uv, part, E2, n_valid, g_lmk, g_dyn, s));
}

int mvd_op_morph_contour_select(const float* A, const float* RT, int cam_frames, int F, int C, int J, int neck_joint, int R, int32_t* row,
                                float* yaw_deg, void* stream) {
  RET_IF(morph_contour_select_check("mvd_op_morph_contour_select", A, RT, cam_frames, F, C, J, neck_joint, R, row));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_contour_select", s, launch_morph_contour_select(A, RT, cam_frames, F, C, J, neck_joint, R, row, yaw_deg, s));
}

int mvd_op_morph_contour_landmarks(const float* verts, const int32_t* faces, const int32_t* dyn_lmk_face, const float* dyn_lmk_bary,
                                   const int32_t* row, int F, int C, int V, int Nf, int R, int Md, float* dyn_lmk, void* stream) {
  RET_IF(morph_contour_landmarks_check("mvd_op_morph_contour_landmarks", verts, faces, dyn_lmk_face, dyn_lmk_bary, row, F, C, V, Nf, R, Md,
                                       dyn_lmk));
  hipStream_t s = S(stream);
  return hook_sync("mvd_op_morph_contour_landmarks", s,
                   launch_morph_contour_landmarks(verts, faces, dyn_lmk_face, dyn_lmk_bary, row, F, C, V, Nf, R, Md, dyn_lmk, s));
}

int mvd_op_morph_contour_bwd(const float* g_dyn, const float* g_in, const int32_t* row, const int32_t* ct_vert, const int32_t* ct_ptr,
                             const int32_t* ct_ent, const float* dyn_lmk_bary, int F, int C, int V, int R, int Md, int n_list, int n_ent,
                             float* g_verts, void* stream) {
  const char* who = "mvd_op_morph_contour_bwd";
  RET_IF(morph_contour_bwd_check(who, g_dyn, row, ct_vert, ct_ptr, ct_ent, dyn_lmk_bary, F, C, V, R, Md, n_list, n_ent, g_verts));
  hipStream_t s = S(stream);
  const size_t bytes = (size_t)F * V * 3 * sizeof(float);
  int rc = 0;
  // the kernel adds in place at the listed vertices: every other vertex keeps g_in (or zero)
  if (!g_in) {
    if (hipMemsetAsync(g_verts, 0, bytes, s) != hipSuccess) rc = morph_fail(who, ": clearing g_verts failed");
  } else if (g_in != g_verts) {
    if (hipMemcpyAsync(g_verts, g_in, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = morph_fail(who, ": copying g_in failed");
  }
  if (!rc) rc = launch_morph_contour_bwd(g_dyn, row, ct_vert, ct_ptr, ct_ent, dyn_lmk_bary, F, C, V, R, Md, n_list, n_ent, g_verts, s);
  return hook_sync(who, s, rc);
}

int mvd_morph_fit_2d_workspace(int F, int V, int NB, int J, int M, int Md, int C, int64_t* floats) {
  const char* who = "mvd_morph_fit_2d_workspace";
  if (!floats) return morph_fail(who, ": null argument");
  if (F < 1 || V < 1 || NB < 1 || J < 1 || J > MORPH_MAX_JOINTS || M < 1 || Md < 0 || C < 1)
    return morph_fail(who, ": F, V, NB, M and C must be at least 1, J in 1..64, Md at least 0");
  if (morph_too_big(F, C, 1) || morph_too_big((long long)F * C, M, 3) || morph_too_big((long long)F * C, Md > 0 ? Md : 1, 3))
    return morph_fail(who, ": F C M 2 and F C Md 3 must be below 2^31");
  *floats = (int64_t)Fit2dLayout(F, V, NB, J, M, Md, C).total;
  return 0;
}

int mvd_morph_fit_2d_run(const float* basis, const float* v_template, const float* weights, const float* j_template, const float* j_dirs,
                         const int32_t* parents, const float* post, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary,
                         const int32_t* csr_ptr, const int32_t* csr_ent, const int32_t* dyn_lmk_face, const float* dyn_lmk_bary,
                         const int32_t* ct_vert, const int32_t* ct_ptr, const int32_t* ct_ent, int F, int V, int NB, int J, int Nf, int M,
                         int n_ent, int R, int Md, int n_list, int ct_n_ent, int neck_joint, const float* K, const float* RT, int cam_frames,
                         int C, const float* target_uv, const float* weight, const float* dyn_target_uv, const float* dyn_weight,
                         int target_frames, float z_near, float px_scale, float lambda2, const float* target, int target3_frames,
                         const float* vertex_weight, float inv_vw_sum, float* p, float* m, float* v, const float* lr, const float* lam,
                         const float* p0, int iters, int step0, float beta1, float beta2, float eps, float* workspace,
                         size_t workspace_floats, float* loss_history, int32_t* n_valid_history, void* stream) {
  const char* who = "mvd_morph_fit_2d_run";
  if (!workspace || !loss_history || !n_valid_history) return morph_fail(who, ": null argument");
  if (iters < 1 || step0 < 0 || step0 > 0x7fffffff - iters) return morph_fail(who, ": iters must be at least 1 and step0 at least 0");
  if (F < 1 || V < 1 || NB < 1 || J < 1 || J > MORPH_MAX_JOINTS || M < 1 || C < 1)
    return morph_fail(who, ": F, V, NB, M and C must be at least 1, J in 1..64");
  if (morph_too_big(iters, F, 1)) return morph_fail(who, ": iters F must be below 2^31");
  if (!faces || !lmk_face || !lmk_bary || !csr_ptr || !csr_ent || Nf < 1) return morph_fail(who, ": the 2-D term needs the landmark embedding");
  const bool dyn = dyn_target_uv != nullptr;
  if (!dyn && dyn_weight) return morph_fail(who, ": contour weights without a contour target");
  if (dyn && (!dyn_lmk_face || !dyn_lmk_bary || !ct_vert || !ct_ptr || !ct_ent || Md < 1))
    return morph_fail(who, ": a contour target is given, and the model has no contour tables");
  if (dyn && (neck_joint < 0 || neck_joint >= J)) return morph_fail(who, ": neck_joint must be in 0..J-1");
  const int md = dyn ? Md : 0;
  if (morph_too_big(F, C, 1) || morph_too_big((long long)F * C, M, 3) || morph_too_big((long long)F * C, dyn ? Md : 1, 3))
    return morph_fail(who, ": F C M 2 and F C Md 3 must be below 2^31");
  const Fit2dLayout lay(F, V, NB, J, M, md, C);
  if (workspace_floats < lay.total) return morph_fail(who, ": the workspace is smaller than mvd_morph_fit_2d_workspace says");
  const int L = NB + 9 * (J - 1), P = NB + 3 * J + 3, nchunk = morph_bwd_chunks(V), nslab = morph_bwd_slabs(V);
  float* w = workspace;
  float *j_rest = w + lay.fit.j_rest, *rot = w + lay.fit.rot, *joints = w + lay.fit.joints, *A = w + lay.fit.A, *coef = w + lay.fit.coef;
  float *verts = w + lay.fit.verts, *blend = w + lay.fit.blend, *lmk = w + lay.fit.lmk, *g_y = w + lay.fit.g_y, *g_b = w + lay.fit.g_b;
  float *part_a = w + lay.fit.part_a, *part_c = w + lay.fit.part_c, *e_part = w + lay.fit.e_part, *g = w + lay.fit.g;
  float *g_y0 = target ? w + lay.g_y0 : nullptr, *uv = w + lay.uv, *dyn_lmk = dyn ? w + lay.dyn_lmk : nullptr;
  float *dyn_uv = dyn ? w + lay.dyn_uv : nullptr, *g_lmk = w + lay.g_lmk, *g_dyn = dyn ? w + lay.g_dyn : nullptr, *part = w + lay.part;
  float* e3 = target ? w + lay.e3 : nullptr;
  int* row = (int*)(w + lay.row);
  const Morph2dTerm t{K, RT, target_uv, weight, dyn_target_uv, dyn_weight, cam_frames, target_frames, C, z_near, px_scale, lambda2};
  // every argument error of every stage, before the first HIP call
  RET_IF(morph_pose_check(who, p, p, j_template, j_dirs, parents, F, NB, J, j_rest, rot, coef, joints, A));
  RET_IF(morph_skin_check(who, basis, v_template, coef, weights, A, F, V, L, NB, J, verts));
  RET_IF(morph_landmarks_check(who, verts, faces, lmk_face, lmk_bary, F, V, Nf, M, lmk));
  if (dyn) {
    RET_IF(morph_contour_select_check(who, A, RT, cam_frames, F, C, J, neck_joint, R, row));
    RET_IF(morph_contour_landmarks_check(who, verts, faces, dyn_lmk_face, dyn_lmk_bary, row, F, C, V, Nf, R, Md, dyn_lmk));
    RET_IF(morph_contour_bwd_check(who, g_dyn, row, ct_vert, ct_ptr, ct_ent, dyn_lmk_bary, F, C, V, R, Md, n_list, ct_n_ent, g_y));
  }
  if (target)
    RET_IF(morph_fit_data_check(who, verts, target, target3_frames, nullptr, nullptr, 1, nullptr, nullptr, nullptr, F, V, 0, 0, g_y0, e_part,
                                e3));
  RET_IF(morph_fit_data_2d_check(who, t, F, M, md, lmk, dyn_lmk, uv, dyn_uv, part, loss_history, n_valid_history, g_lmk, g_dyn));
  RET_IF(morph_landmarks_bwd_check(who, g_lmk, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_y));
  RET_IF(morph_skin_bwd_check(who, g_y, weights, A, blend, basis, F, V, L, NB, J, g_b, part_a, part_c));
  RET_IF(morph_pose_bwd_check(who, p, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, F, NB, J, g, g, g));
  RET_IF(morph_fit_update_check(who, p, g, m, v, lr, lam, p0, F, P, step0 + 1, beta1, beta2, eps));
  hipStream_t s = S(stream);
  int rc = 0;
  const float *betas = p, *pose = p + NB, *transl = p + NB + 3 * J;
  for (int it = 0; it < iters && !rc; ++it) {
    rc = launch_morph_pose_ex(betas, P, pose, P, j_template, j_dirs, parents, F, NB, J, j_rest, rot, nullptr, joints, A, coef, s);
    if (!rc) rc = launch_morph_skin_ex(basis, v_template, coef, weights, A, post, transl, P, F, V, L, J, verts, blend, s);
    if (!rc) rc = launch_morph_landmarks(verts, faces, lmk_face, lmk_bary, F, V, Nf, M, lmk, s);
    if (!rc && dyn) rc = launch_morph_contour_select(A, RT, cam_frames, F, C, J, neck_joint, R, row, nullptr, s);
    if (!rc && dyn) rc = launch_morph_contour_landmarks(verts, faces, dyn_lmk_face, dyn_lmk_bary, row, F, C, V, Nf, R, Md, dyn_lmk, s);
    // the 3-D vertex term, if there is one: its gradient is where the landmarks' adjoint starts from, its energy is added to E2
    if (!rc && target)
      rc = launch_morph_fit_data(verts, target, target3_frames, vertex_weight, inv_vw_sum, nullptr, nullptr, 1, nullptr, 0.0f, nullptr, nullptr,
                                 nullptr, F, V, 0, 0, g_y0, e_part, e3, s);
    if (!rc)
      rc = launch_morph_fit_data_2d(t, F, M, md, lmk, dyn_lmk, e3, uv, dyn_uv, part, loss_history + (size_t)it * F,
                                    n_valid_history + (size_t)it * F, g_lmk, g_dyn, s);
    if (!rc) rc = launch_morph_landmarks_bwd(g_lmk, g_y0, csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_y, s);
    if (!rc && dyn) rc = launch_morph_contour_bwd(g_dyn, row, ct_vert, ct_ptr, ct_ent, dyn_lmk_bary, F, C, V, R, Md, n_list, ct_n_ent, g_y, s);
    if (!rc) rc = launch_morph_skin_bwd(g_y, post, weights, A, blend, basis, F, V, L, J, g_b, part_a, part_c, s);
    if (!rc)
      rc = launch_morph_pose_bwd(pose, P, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, nullptr, F, NB, J, g, P, g + NB, P,
                                 g + NB + 3 * J, P, s);
    if (!rc) rc = launch_morph_fit_update(p, g, m, v, lr, lam, p0, F, P, step0 + it + 1, beta1, beta2, eps, s);
  }
  return hook_sync(who, s, rc);
}

int mvd_morph_fit_scan_workspace(int F, int V, int NB, int J, int M, int64_t* floats) {
  if (!floats) return morph_fail("mvd_morph_fit_scan_workspace", ": null argument");
  if (F < 1 || V < 1 || NB < 1 || J < 1 || J > MORPH_MAX_JOINTS || M < 0)
    return morph_fail("mvd_morph_fit_scan_workspace", ": F, V and NB must be at least 1, J in 1..64, M at least 0");
  *floats = (int64_t)ScanLayout(F, V, NB, J, M).total;
  return 0;
}

int mvd_morph_fit_scan_run(const float* basis, const float* v_template, const float* weights, const float* j_template, const float* j_dirs,
                           const int32_t* parents, const float* post, const int32_t* faces, const int32_t* lmk_face, const float* lmk_bary,
                           const int32_t* csr_ptr, const int32_t* csr_ent, const int32_t* inc_ptr, const int32_t* inc_face, int F, int V,
                           int NB, int J, int Nf, int M, int n_ent, const float* scan_verts, const int32_t* scan_faces,
                           const int32_t* scan_vptr, const int32_t* scan_fptr, int Fs, int normal_gate, float cos_min, float max_dist2,
                           int refresh, const float* vertex_weight, const float* target_lmk, int target_lmk_frames,
                           const float* lmk_weight, float lmk_scale, float* p, float* m, float* v, const float* lr, const float* lam,
                           const float* p0, int iters, int step0, float beta1, float beta2, float eps, float* workspace,
                           size_t workspace_floats, float* loss_history, int32_t* matched_history, int32_t* corr_face, void* stream) {
  const char* who = "mvd_morph_fit_scan_run";
  if (!workspace || !loss_history || !matched_history || !corr_face || !scan_verts || !scan_faces || !scan_vptr || !scan_fptr)
    return morph_fail(who, ": null argument");
  if (iters < 1 || step0 < 0 || step0 > 0x7fffffff - iters) return morph_fail(who, ": iters must be at least 1 and step0 at least 0");
  if (refresh < 1) return morph_fail(who, ": refresh must be at least 1");
  if (F < 1 || V < 1 || NB < 1 || J < 1 || J > MORPH_MAX_JOINTS || M < 0)
    return morph_fail(who, ": F, V and NB must be at least 1, J in 1..64, M at least 0");
  if (morph_too_big(iters, F, 1)) return morph_fail(who, ": iters F must be below 2^31");
  if (Fs != 1 && Fs != F) return morph_fail(who, ": one scan or one per frame");
  if (scan_vptr[0] != 0 || scan_fptr[0] != 0) return morph_fail(who, ": the scan offsets must start at 0");
  for (int i = 0; i < Fs; ++i)
    if (scan_vptr[i + 1] <= scan_vptr[i] || scan_fptr[i + 1] <= scan_fptr[i])
      return morph_fail(who, ": every scan needs at least one vertex and one face, offsets ascending");
  const bool use_lmk = target_lmk != nullptr, gate = normal_gate != 0;
  if (use_lmk && (!faces || !lmk_face || M < 1 || Nf < 1)) return morph_fail(who, ": a landmark target needs the landmark embedding");
  if (gate && (!faces || !inc_ptr || !inc_face || Nf < 1)) return morph_fail(who, ": the normal gate needs the model's faces and their incidence");
  const ScanLayout lay(F, V, NB, J, use_lmk ? M : 0);
  if (workspace_floats < lay.total) return morph_fail(who, ": the workspace is smaller than mvd_morph_fit_scan_workspace says");
  const int L = NB + 9 * (J - 1), P = NB + 3 * J + 3, nchunk = morph_bwd_chunks(V), nslab = morph_bwd_slabs(V);
  float* w = workspace;
  float *j_rest = w + lay.fit.j_rest, *rot = w + lay.fit.rot, *joints = w + lay.fit.joints, *A = w + lay.fit.A, *coef = w + lay.fit.coef;
  float *verts = w + lay.fit.verts, *blend = w + lay.fit.blend, *lmk = use_lmk ? w + lay.fit.lmk : nullptr, *g_y = w + lay.fit.g_y;
  float *g_b = w + lay.fit.g_b, *part_a = w + lay.fit.part_a, *part_c = w + lay.fit.part_c, *e_part = w + lay.fit.e_part, *g = w + lay.fit.g;
  float *normals = w + lay.normals, *corr_point = w + lay.corr_point, *bary = w + lay.bary, *dist2 = w + lay.dist2, *w_part = w + lay.w_part;
  unsigned long long* key = (unsigned long long*)(w + lay.key);
  int* bad = (int*)(w + lay.bad);
  // every argument error of every stage, before the first HIP call
  RET_IF(morph_pose_check(who, p, p, j_template, j_dirs, parents, F, NB, J, j_rest, rot, coef, joints, A));
  RET_IF(morph_skin_check(who, basis, v_template, coef, weights, A, F, V, L, NB, J, verts));
  if (use_lmk) RET_IF(morph_landmarks_check(who, verts, faces, lmk_face, lmk_bary, F, V, Nf, M, lmk));
  if (gate) RET_IF(mesh_vertex_normals_check(who, verts, faces, inc_ptr, inc_face, F, V, Nf, normals, bad));
  for (int i = 0; i < Fs; ++i)
    RET_IF(mesh_closest_check(who, verts, scan_verts, scan_faces, Fs == 1 ? (int)std::min<long long>((long long)F * V, 0x7fffffff) : V,
                              scan_vptr[i + 1] - scan_vptr[i], scan_fptr[i + 1] - scan_fptr[i], cos_min, max_dist2, 0, key, corr_face, bary,
                              corr_point, dist2));
  RET_IF(morph_fit_data_corr_check(who, verts, corr_point, corr_face, lmk, target_lmk, target_lmk_frames, csr_ptr, csr_ent, lmk_bary, F, V, M,
                                   n_ent, g_y, e_part, w_part, loss_history, matched_history));
  RET_IF(morph_skin_bwd_check(who, g_y, weights, A, blend, basis, F, V, L, NB, J, g_b, part_a, part_c));
  RET_IF(morph_pose_bwd_check(who, p, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, F, NB, J, g, g, g));
  RET_IF(morph_fit_update_check(who, p, g, m, v, lr, lam, p0, F, P, step0 + 1, beta1, beta2, eps));
  hipStream_t s = S(stream);
  int rc = 0;
  const float *betas = p, *pose = p + NB, *transl = p + NB + 3 * J;
  for (int it = 0; it < iters && !rc; ++it) {
    rc = launch_morph_pose_ex(betas, P, pose, P, j_template, j_dirs, parents, F, NB, J, j_rest, rot, nullptr, joints, A, coef, s);
    if (!rc) rc = launch_morph_skin_ex(basis, v_template, coef, weights, A, post, transl, P, F, V, L, J, verts, blend, s);
    if (!rc && use_lmk) rc = launch_morph_landmarks(verts, faces, lmk_face, lmk_bary, F, V, Nf, M, lmk, s);
    if (!rc && it % refresh == 0) {
      if (gate) rc = launch_mesh_vertex_normals(verts, faces, inc_ptr, inc_face, F, V, Nf, normals, bad, s);
      if (!rc && Fs == 1)  // a shared scan: every frame's vertices in one launch
        rc = launch_mesh_closest_point(verts, gate ? normals : nullptr, scan_verts, scan_faces, F * V, scan_vptr[1], scan_fptr[1], cos_min,
                                       max_dist2, 0, key, corr_face, bary, corr_point, dist2, s);
      for (int f = 0; f < F && !rc && Fs != 1; ++f) {
        const size_t o = (size_t)f * V;
        rc = launch_mesh_closest_point(verts + o * 3, gate ? normals + o * 3 : nullptr, scan_verts + (size_t)scan_vptr[f] * 3,
                                       scan_faces + (size_t)scan_fptr[f] * 3, V, scan_vptr[f + 1] - scan_vptr[f],
                                       scan_fptr[f + 1] - scan_fptr[f], cos_min, max_dist2, 0, key + o, corr_face + o, bary + o * 3,
                                       corr_point + o * 3, dist2 + o, s);
      }
    }
    if (!rc)
      rc = launch_morph_fit_data_corr(verts, corr_point, corr_face, vertex_weight, lmk, target_lmk, target_lmk_frames, lmk_weight, lmk_scale,
                                      csr_ptr, csr_ent, lmk_bary, F, V, M, n_ent, g_y, e_part, w_part, loss_history + (size_t)it * F,
                                      matched_history + (size_t)it * F, s);
    if (!rc) rc = launch_morph_skin_bwd(g_y, post, weights, A, blend, basis, F, V, L, J, g_b, part_a, part_c, s);
    if (!rc)
      rc = launch_morph_pose_bwd(pose, P, j_rest, A, j_dirs, parents, part_a, nchunk, part_c, nslab, nullptr, F, NB, J, g, P, g + NB, P,
                                 g + NB + 3 * J, P, s);
    if (!rc) rc = launch_morph_fit_update(p, g, m, v, lr, lam, p0, F, P, step0 + it + 1, beta1, beta2, eps, s);
  }
  return hook_sync(who, s, rc);
}
