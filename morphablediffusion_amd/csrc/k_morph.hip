// The morphable-model forward -- include/mvd.h: mvd_op_morph_pose, mvd_op_morph_skin, mvd_op_morph_landmarks.  FLAME / SMPL-X
// parameters to vertices by linear blend skinning (the formulas of the reference's third_party/MICA/models/lbs.py), fp32 on the
// vector ALU with explicit fused multiply-adds in an order fixed by indices alone and no atomics: two calls agree bit for bit, and
// nothing here depends on the library's operand type (MVD_BF16).
// Launches:
//   morph_pose_kernel       one wave per frame: rest joints from the folded regressor (a lane per component, betas in ascending
//                           order), Rodrigues and the pose feature (a lane per joint), then the kinematic chain in joint order by one
//                           lane out of LDS -- the stage moves a few KB, and a single thread doing all of it spends 0.4 ms waiting
//                           on 6000 dependent loads at FLAME size.  The posed joints follow the reference's chain,
//                           t_j = G_p (j_rest_j - j_rest_p) + t_p.  The translation of the relative transform is carried directly,
//                           a_j = a_p - G_p (D_j j_rest_j) with D = R - I: the reference's t_j - G_j j_rest_j adds and subtracts the
//                           rest offsets, which cancels only up to rounding; this form is exactly [I|0] at a zero pose.
//   morph_skin_kernel       the bandwidth-bound stage.  A workgroup of 4 waves owns SKIN_VB = 16 vertices (48 basis columns) and a
//                           tile of SKIN_FT = 32 frames, 8 per wave.  All 256 threads stream the basis, SKIN_LC = 64 rows x 48
//                           columns per step, through two LDS tiles (12 loads per thread in flight under the previous tile's
//                           arithmetic), and the same rows of the 32 frames' coefficients beside them; wave w then runs over the
//                           rows of a tile in ascending order, lane c holding column c of its 8 frames in registers, the
//                           coefficients arriving as two broadcast 16-byte LDS reads per row (scalar loads from memory were
//                           measured first: their latency, exposed in a loop one wave runs alone, held the kernel to 0.8 TB/s).
//                           A wave with one live frame runs the same chain with one multiply-add per row.  The basis is so
//                           read once per 32 frames, and the order over l is the same whatever the tiling: frame f of a batch
//                           equals the frame computed alone.  16 vertices per workgroup, not more, because the columns are the
//                           only parallel axis (the order over l is fixed): FLAME's 5023 vertices give 314 workgroups for 256
//                           CUs.  The blended template goes through LDS to a (vertex, frame) thread layout for the skinning.
//   morph_landmarks_kernel  one thread per (frame, landmark); an index out of range is never dereferenced (NaN).
#include "morph.h"

#include <string>

namespace {

constexpr int MORPH_T = 256;
constexpr int SKIN_VB = 16, SKIN_CB = 3 * SKIN_VB;  // vertices and basis columns of a workgroup
constexpr int SKIN_LC = 64;                         // basis rows of an LDS tile
constexpr int SKIN_FW = 8, SKIN_FT = SKIN_FW * (MORPH_T / 64);  // frames of a wave, of a workgroup
constexpr int SKIN_NLD = SKIN_LC * SKIN_CB / MORPH_T;           // basis tile elements per thread
constexpr int SKIN_CLD = SKIN_FT + 4;                           // row stride of the coefficient tile [row][frame]: rows stay 16-byte
                                                                // aligned, and a wave storing one frame's 64 rows conflicts 4-way only
constexpr int SKIN_NCF = SKIN_LC * SKIN_FT / MORPH_T;           // coefficient tile elements per thread
static_assert(SKIN_NLD * MORPH_T == SKIN_LC * SKIN_CB && SKIN_CB <= 64 && SKIN_VB * SKIN_FT == 2 * MORPH_T && SKIN_LC == 64 && SKIN_FW == 8,
              "skin kernel geometry");

struct MorphPoseArgs {
  const float *betas, *pose, *j_template, *j_dirs;
  float *j_rest, *rot, *pose_feature, *joints, *A, *coef;  // coef [F][NB + 9 (J-1)] = betas | pose feature, or null
  int F, NB, J, ldb, ldp;                                   // ldb, ldp: floats between two frames' betas and poses
  signed char parents[MORPH_MAX_JOINTS];
};

// One wave per frame.  Stage 1: lane c (and c + 64, ...) sums component c of the rest joints over the betas in ascending order,
// adjacent lanes reading adjacent addresses of j_dirs.  Stage 2: lane j turns joint j's axis-angle into D_j = R_j - I.  Stage 3: lane
// 0 walks the tree in index order; the tables it reads are in LDS.
__global__ __launch_bounds__(64) void morph_pose_kernel(MorphPoseArgs a) {
  __shared__ float s_jr[MORPH_MAX_JOINTS * 3], s_D[MORPH_MAX_JOINTS * 9], s_A[MORPH_MAX_JOINTS * 12], s_t[MORPH_MAX_JOINTS * 3];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int J = a.J, NB = a.NB;
  const float* beta = a.betas + (size_t)f * a.ldb;
  const float* posef = a.pose + (size_t)f * a.ldp;
  float* coef = a.coef ? a.coef + (size_t)f * (NB + 9 * (J - 1)) : nullptr;
  if (coef)
    for (int n = lane; n < NB; n += 64) coef[n] = beta[n];
  for (int c = lane; c < J * 3; c += 64) {
    float s = a.j_template[c];
#pragma unroll 8
    for (int n = 0; n < NB; ++n) s = fmaf(beta[n], a.j_dirs[(size_t)n * J * 3 + c], s);  // unrolled: 8 loads in flight per chain step
    s_jr[c] = s;
    a.j_rest[(size_t)f * J * 3 + c] = s;
  }
  if (lane < J) {
    const int j = lane;
    const size_t fj = (size_t)f * J + j;
    const float rx = posef[j * 3], ry = posef[j * 3 + 1], rz = posef[j * 3 + 2];
    const float qx = rx + 1e-8f, qy = ry + 1e-8f, qz = rz + 1e-8f;
    const float angle = sqrtf(fmaf(qz, qz, fmaf(qy, qy, qx * qx)));
    const float x = rx / angle, y = ry / angle, z = rz / angle;
    const float sn = sinf(angle), oc = 1.0f - cosf(angle);
    // D = sin K + (1 - cos) K^2, K = [[0, -z, y], [z, 0, -x], [-y, x, 0]]; "0.0f -" keeps a zero pose at +0
    float D[9];
    D[0] = 0.0f - oc * fmaf(y, y, z * z);
    D[1] = fmaf(oc, x * y, 0.0f - sn * z);
    D[2] = fmaf(oc, x * z, sn * y);
    D[3] = fmaf(oc, x * y, sn * z);
    D[4] = 0.0f - oc * fmaf(x, x, z * z);
    D[5] = fmaf(oc, y * z, 0.0f - sn * x);
    D[6] = fmaf(oc, x * z, 0.0f - sn * y);
    D[7] = fmaf(oc, y * z, sn * x);
    D[8] = 0.0f - oc * fmaf(x, x, y * y);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      s_D[j * 9 + e] = D[e];
      a.rot[fj * 9 + e] = (e % 4 == 0 ? 1.0f : 0.0f) + D[e];
      if (j >= 1 && a.pose_feature) a.pose_feature[((size_t)f * (J - 1) + (j - 1)) * 9 + e] = D[e];
      if (j >= 1 && coef) coef[NB + (j - 1) * 9 + e] = D[e];
    }
  }
  __syncthreads();
  if (lane != 0) return;
  for (int j = 0; j < J; ++j) {
    const size_t fj = (size_t)f * J + j;
    float D[9], R[9], jr[3], u[3], G[9], at[3], tj[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) D[e] = s_D[j * 9 + e], R[e] = (e % 4 == 0 ? 1.0f : 0.0f) + D[e];
#pragma unroll
    for (int k = 0; k < 3; ++k) jr[k] = s_jr[j * 3 + k];
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = fmaf(D[i * 3 + 2], jr[2], fmaf(D[i * 3 + 1], jr[1], D[i * 3] * jr[0]));
    if (j == 0) {
#pragma unroll
      for (int e = 0; e < 9; ++e) G[e] = R[e];
#pragma unroll
      for (int i = 0; i < 3; ++i) at[i] = 0.0f - u[i], tj[i] = jr[i];
    } else {
      const int p = a.parents[j];
      float P[12], rel[3];
#pragma unroll
      for (int e = 0; e < 12; ++e) P[e] = s_A[p * 12 + e];
#pragma unroll
      for (int k = 0; k < 3; ++k) rel[k] = jr[k] - s_jr[p * 3 + k];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        at[i] = P[i * 4 + 3] - fmaf(P[i * 4 + 2], u[2], fmaf(P[i * 4 + 1], u[1], P[i * 4] * u[0]));
        // the posed joint as the reference chains it: t_j = G_p (j_rest_j - j_rest_p) + t_p
        tj[i] = fmaf(P[i * 4], rel[0], fmaf(P[i * 4 + 1], rel[1], fmaf(P[i * 4 + 2], rel[2], s_t[p * 3 + i])));
#pragma unroll
        for (int k = 0; k < 3; ++k) G[i * 3 + k] = fmaf(P[i * 4 + 2], R[6 + k], fmaf(P[i * 4 + 1], R[3 + k], P[i * 4] * R[k]));
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_A[j * 12 + i * 4 + k] = a.A[fj * 12 + i * 4 + k] = G[i * 3 + k];
      s_A[j * 12 + i * 4 + 3] = a.A[fj * 12 + i * 4 + 3] = at[i];
      s_t[j * 3 + i] = a.joints[fj * 3 + i] = tj[i];
    }
  }
}

// acc[i] += coefficient(row r, frame i) * basis(row r, this lane's column) over the rows of a tile in ascending order: the one chain
// of fused multiply-adds per frame, whether the wave holds one live frame or eight.  crow: the wave's 8 frames of row 0 (uniform).
template <int NF>
__device__ inline void skin_rows(const float* tile, const float* crow, int nrow, float* acc) {
#pragma unroll 4
  for (int r = 0; r < nrow; ++r) {
    const float bv = tile[r * SKIN_CB];
    if constexpr (NF == 1) {
      acc[0] = fmaf(crow[r * SKIN_CLD], bv, acc[0]);
    } else {
      const float4 ca = *reinterpret_cast<const float4*>(crow + r * SKIN_CLD), cb = *reinterpret_cast<const float4*>(crow + r * SKIN_CLD + 4);
      acc[0] = fmaf(ca.x, bv, acc[0]), acc[1] = fmaf(ca.y, bv, acc[1]), acc[2] = fmaf(ca.z, bv, acc[2]), acc[3] = fmaf(ca.w, bv, acc[3]);
      acc[4] = fmaf(cb.x, bv, acc[4]), acc[5] = fmaf(cb.y, bv, acc[5]), acc[6] = fmaf(cb.z, bv, acc[6]), acc[7] = fmaf(cb.w, bv, acc[7]);
    }
  }
}

__global__ __launch_bounds__(MORPH_T) void morph_skin_kernel(const float* __restrict__ basis, const float* __restrict__ v_template,
                                                             const float* __restrict__ coef, const float* __restrict__ weights,
                                                             const float* __restrict__ A, const float* __restrict__ post,
                                                             const float* __restrict__ transl, int ldt, int F, int V, int L, int J,
                                                             int nvb, float* __restrict__ verts, float* __restrict__ blend) {
  __shared__ float s_tile[2][SKIN_LC * SKIN_CB];
  __shared__ __align__(16) float s_coef[2][SKIN_LC * SKIN_CLD];
  __shared__ float s_b[SKIN_FT][SKIN_CB];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int vb = blockIdx.x % nvb, f0 = (blockIdx.x / nvb) * SKIN_FT;
  const int C = 3 * V, c0 = vb * SKIN_CB;
  const int ncol = min(SKIN_CB, C - c0);  // >= 3

  float stage[SKIN_NLD], cstage[SKIN_NCF];
  // tile element e = t + 256 i is (row e / 48, column e % 48): a wave reads whole 192-byte row segments
  auto load_tile = [&](int l0) {
#pragma unroll
    for (int i = 0; i < SKIN_NLD; ++i) {
      const int e = t + i * MORPH_T, row = e / SKIN_CB, col = e - row * SKIN_CB;
      stage[i] = (l0 + row < L && col < ncol) ? basis[(size_t)(l0 + row) * C + c0 + col] : 0.0f;
    }
    // coefficients of the same rows: this lane's row of frame w + 4 i (64 consecutive floats of a frame per wave); 0 past F or L
#pragma unroll
    for (int i = 0; i < SKIN_NCF; ++i) {
      const int fr = f0 + w + 4 * i;
      cstage[i] = (fr < F && l0 + lane < L) ? coef[(size_t)fr * L + l0 + lane] : 0.0f;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < SKIN_NLD; ++i) s_tile[buf][t + i * MORPH_T] = stage[i];
#pragma unroll
    for (int i = 0; i < SKIN_NCF; ++i) s_coef[buf][lane * SKIN_CLD + w + 4 * i] = cstage[i];
  };

  // wave w: frames fw0 .. fw0 + nfw - 1; a slot past the last frame gets zero coefficients and is never read
  const int fw0 = f0 + w * SKIN_FW;
  const int nfw = max(0, min(SKIN_FW, F - fw0));
  const int colc = min(lane, ncol - 1);  // lanes past the last column repeat it
  float acc[SKIN_FW];
#pragma unroll
  for (int i = 0; i < SKIN_FW; ++i) acc[i] = v_template[c0 + colc];

  const int ntile = (L + SKIN_LC - 1) / SKIN_LC;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int tl = 0; tl < ntile; ++tl) {
    const int buf = tl & 1, l0 = tl * SKIN_LC;
    if (tl + 1 < ntile) load_tile(l0 + SKIN_LC);  // in flight under this tile's arithmetic
    const int nrow = min(SKIN_LC, L - l0);
    if (nfw == 1)
      skin_rows<1>(s_tile[buf] + colc, s_coef[buf] + w * SKIN_FW, nrow, acc);
    else if (nfw > 1)
      skin_rows<SKIN_FW>(s_tile[buf] + colc, s_coef[buf] + w * SKIN_FW, nrow, acc);
    if (tl + 1 < ntile) store_tile(buf ^ 1);  // the tile read at step tl - 1: every wave is past it
    __syncthreads();
  }
  if (nfw > 0 && lane < SKIN_CB) {
#pragma unroll
    for (int i = 0; i < SKIN_FW; ++i) s_b[w * SKIN_FW + i][lane] = acc[i];
  }
  __syncthreads();

  // skinning: thread (vertex t % 16, frames t / 16 and t / 16 + 16)
  const int v = t & (SKIN_VB - 1), gv = vb * SKIN_VB + v;
  if (gv >= V) return;
  for (int h = 0; h < 2; ++h) {
    const int fl = (t >> 4) + h * (MORPH_T / SKIN_VB), f = f0 + fl;
    if (f >= F) continue;
    const float b0 = s_b[fl][3 * v], b1 = s_b[fl][3 * v + 1], b2 = s_b[fl][3 * v + 2];
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0f;
    const float* wr = weights + (size_t)gv * J;
    const float* Af = A + (size_t)f * J * 12;
    for (int j = 0; j < J; ++j) {
      const float wj = wr[j];
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = fmaf(wj, Af[j * 12 + e], T[e]);
    }
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = fmaf(T[i * 4], b0, fmaf(T[i * 4 + 1], b1, fmaf(T[i * 4 + 2], b2, T[i * 4 + 3])));
    if (transl) {  // a branch, not "+ 0": without a translation -0 stays -0
#pragma unroll
      for (int i = 0; i < 3; ++i) o[i] += transl[(size_t)f * ldt + i];
    }
    if (blend) {
      float* bd = blend + ((size_t)f * V + gv) * 3;
      bd[0] = b0, bd[1] = b1, bd[2] = b2;
    }
    float* dst = verts + ((size_t)f * V + gv) * 3;
    if (post) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        dst[i] = fmaf(post[i * 4], o[0], fmaf(post[i * 4 + 1], o[1], fmaf(post[i * 4 + 2], o[2], post[i * 4 + 3])));
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) dst[i] = o[i];
    }
  }
}

__global__ __launch_bounds__(MORPH_T) void morph_landmarks_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                  const int* __restrict__ lmk_face, const float* __restrict__ lmk_bary,
                                                                  int F, int V, int Nf, int M, float* __restrict__ out) {
  const int i = blockIdx.x * MORPH_T + threadIdx.x;  // F M 3 < 2^31
  if (i >= F * M) return;
  const int f = i / M, m = i - f * M;
  const int face = lmk_face[m];
  float o[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if ((unsigned)face < (unsigned)Nf) {
    const int i0 = faces[(size_t)face * 3], i1 = faces[(size_t)face * 3 + 1], i2 = faces[(size_t)face * 3 + 2];
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
      const float w0 = lmk_bary[m * 3], w1 = lmk_bary[m * 3 + 1], w2 = lmk_bary[m * 3 + 2];
      const float* x = verts + (size_t)f * V * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) o[k] = fmaf(w2, x[(size_t)i2 * 3 + k], fmaf(w1, x[(size_t)i1 * 3 + k], w0 * x[(size_t)i0 * 3 + k]));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = o[k];
}

}  // namespace

int morph_fail(const char* who, const char* what) { return mvd_fail((std::string(who) + what).c_str()); }

bool morph_too_big(long long a, long long b, long long c) { return a * b > 0x7fffffffLL / c; }  // a b c >= 2^31, without overflow

int morph_pose_check(const char* who, const float* betas, const float* pose, const float* j_template, const float* j_dirs,
                     const int* parents, int F, int NB, int J, const float* j_rest, const float* rot, const float* pose_feature,
                     const float* joints, const float* A) {
  if (!betas || !pose || !j_template || !j_dirs || !parents || !j_rest || !rot || !joints || !A) return morph_fail(who, ": null argument");
  if (F < 1 || NB < 1) return morph_fail(who, ": F and NB must be at least 1");
  if (J < 1 || J > MORPH_MAX_JOINTS) return morph_fail(who, ": J must be in 1..64");
  if (J > 1 && !pose_feature) return morph_fail(who, ": null pose_feature with more than one joint");
  if (morph_too_big(F, J, 12) || morph_too_big(NB, J, 3)) return morph_fail(who, ": F J 12 and NB J 3 must be below 2^31");
  if (parents[0] != -1) return morph_fail(who, ": parents[0] must be -1");
  for (int j = 1; j < J; ++j)
    if (parents[j] < 0 || parents[j] >= j) return morph_fail(who, ": parents[j] must be in 0..j-1 for j >= 1");
  return 0;
}

int launch_morph_pose(const float* betas, const float* pose, const float* j_template, const float* j_dirs, const int* parents, int F,
                      int NB, int J, float* j_rest, float* rot, float* pose_feature, float* joints, float* A, hipStream_t s) {
  return launch_morph_pose_ex(betas, NB, pose, 3 * J, j_template, j_dirs, parents, F, NB, J, j_rest, rot, pose_feature, joints, A, nullptr, s);
}

int launch_morph_pose_ex(const float* betas, int ldb, const float* pose, int ldp, const float* j_template, const float* j_dirs,
                         const int* parents, int F, int NB, int J, float* j_rest, float* rot, float* pose_feature, float* joints, float* A,
                         float* coef, hipStream_t s) {
  MorphPoseArgs a;
  a.betas = betas, a.pose = pose, a.j_template = j_template, a.j_dirs = j_dirs;
  a.j_rest = j_rest, a.rot = rot, a.pose_feature = pose_feature, a.joints = joints, a.A = A, a.coef = coef;
  a.F = F, a.NB = NB, a.J = J, a.ldb = ldb, a.ldp = ldp;
  for (int j = 0; j < MORPH_MAX_JOINTS; ++j) a.parents[j] = (signed char)(j < J ? parents[j] : -1);
  hipLaunchKernelGGL(morph_pose_kernel, dim3(F), dim3(64), 0, s, a);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_skin_check(const char* who, const float* basis, const float* v_template, const float* coef, const float* weights,
                     const float* A, int F, int V, int L, int NB, int J, const float* verts) {
  if (!basis || !v_template || !coef || !weights || !A || !verts) return morph_fail(who, ": null argument");
  if (F < 1 || V < 1 || L < 1 || NB < 1) return morph_fail(who, ": F, V, L and NB must be at least 1");
  if (J < 1 || J > MORPH_MAX_JOINTS) return morph_fail(who, ": J must be in 1..64");
  if ((long long)L != (long long)NB + 9LL * (J - 1)) return morph_fail(who, ": L must be NB + 9 (J - 1)");
  if (morph_too_big(F, V, 3)) return morph_fail(who, ": F V 3 must be below 2^31");
  return 0;
}

int launch_morph_skin(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                      const float* post, int F, int V, int L, int J, float* verts, hipStream_t s) {
  return launch_morph_skin_ex(basis, v_template, coef, weights, A, post, nullptr, 0, F, V, L, J, verts, nullptr, s);
}

int launch_morph_skin_ex(const float* basis, const float* v_template, const float* coef, const float* weights, const float* A,
                         const float* post, const float* transl, int ldt, int F, int V, int L, int J, float* verts, float* blend,
                         hipStream_t s) {
  const int nvb = (V + SKIN_VB - 1) / SKIN_VB, nft = (F + SKIN_FT - 1) / SKIN_FT;  // nvb nft <= F V / 512 + F + V + 1 < 2^31
  hipLaunchKernelGGL(morph_skin_kernel, dim3((unsigned)nvb * (unsigned)nft), dim3(MORPH_T), 0, s, basis, v_template, coef, weights, A, post,
                     transl, ldt, F, V, L, J, nvb, verts, blend);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int morph_landmarks_check(const char* who, const float* verts, const int* faces, const int* lmk_face, const float* lmk_bary, int F, int V,
                          int Nf, int M, const float* out) {
  if (!verts || !faces || !lmk_face || !lmk_bary || !out) return morph_fail(who, ": null argument");
  if (F < 1 || V < 1 || Nf < 1 || M < 1) return morph_fail(who, ": F, V, Nf and M must be at least 1");
  if (morph_too_big(F, V, 3) || morph_too_big(F, M, 3)) return morph_fail(who, ": F V 3 and F M 3 must be below 2^31");
  return 0;
}

int launch_morph_landmarks(const float* verts, const int* faces, const int* lmk_face, const float* lmk_bary, int F, int V, int Nf, int M,
                           float* out, hipStream_t s) {
  hipLaunchKernelGGL(morph_landmarks_kernel, dim3((F * M + MORPH_T - 1) / MORPH_T), dim3(MORPH_T), 0, s, verts, faces, lmk_face, lmk_bary, F,
                     V, Nf, M, out);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
