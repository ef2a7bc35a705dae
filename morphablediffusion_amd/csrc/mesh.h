// Device helpers shared by the mesh texturing kernels (k_mesh.hip: per-vertex fusion; k_mesh_uv.hip: per-texel bake and the
// UV render): the constants of include/mvd.h's mesh block, the fp32 projection chain, the integer vertex test, the view texel
// fetch, the weight and the bilinear sample at a snapped position.  One definition, so that a vertex and a texel that sit at
// the same point get the same integers, the same weight and the same colour.  Further down: the closest point of one triangle
// and the launchers of the closest-point query (k_closest.hip), which the scan fitter's loop (c_api_morph.hip) calls too.
#pragma once
#include "common.h"

constexpr int MESH_SUB = 4, MESH_ONE = 1 << MESH_SUB, MESH_KMAX = (1 << 24) - 1, MESH_GUARD_PX = 4096, MESH_GUARD = MESH_GUARD_PX << MESH_SUB;

// cam = R x + t, u = (K00 X + K01 Y) / Z + K02, v = K11 Y / Z + K12 in fp32; r: 12 floats of RT, k: 9 floats of K.  xs = ys = kk = 0
// marks an invalid point.  A NaN fails every comparison: Z >= z_near and the guard band are written so that it lands on the
// invalid side.
// The chain itself, shared with the 2-D landmark term (k_morph_2d.hip), which needs the camera-space point and the unsnapped pixel.
__device__ inline void mesh_project_uv(const float* __restrict__ r, const float* __restrict__ k, float x, float y, float z, float& X,
                                       float& Y, float& Z, float& u, float& w) {
  X = r[0] * x + r[1] * y + r[2] * z + r[3];
  Y = r[4] * x + r[5] * y + r[6] * z + r[7];
  Z = r[8] * x + r[9] * y + r[10] * z + r[11];
  u = (k[0] * X + k[1] * Y) / Z + k[2];
  w = k[4] * Y / Z + k[5];
}

__device__ inline void mesh_project_point(const float* __restrict__ r, const float* __restrict__ k, float x, float y, float z, float z_near,
                                          int& xs, int& ys, int& kk) {
  float X, Y, Z, u, w;
  mesh_project_uv(r, k, x, y, z, X, Y, Z, u, w);
  xs = 0, ys = 0, kk = 0;
  if (Z >= z_near && fabsf(u) <= (float)MESH_GUARD_PX && fabsf(w) <= (float)MESH_GUARD_PX) {
    xs = (int)rintf(u * (float)MESH_ONE);
    ys = (int)rintf(w * (float)MESH_ONE);
    const float q = rintf(z_near / Z * (float)MESH_KMAX);
    kk = q >= 1.0f ? (q <= (float)MESH_KMAX ? (int)q : MESH_KMAX) : 1;
  }
}

__device__ inline bool mesh_vertex_ok(int xs, int ys, int k) {
  return k >= 1 && k <= MESH_KMAX && xs >= -MESH_GUARD && xs <= MESH_GUARD && ys >= -MESH_GUARD && ys <= MESH_GUARD;
}

// channel c of pixel (i, j) of view n in [0, 1]
__device__ inline float mesh_texel(const void* __restrict__ img, int dtype, int layout, int H, int W, int n, int c, int i, int j) {
  const size_t o = layout == 0 ? (((size_t)n * 3 + c) * H + i) * W + j : (((size_t)n * H + i) * W + j) * 3 + c;
  if (dtype == 1) return (float)((const unsigned char*)img)[o] / 255.0f;
  return (fminf(fmaxf(((const float*)img)[o], -1.0f), 1.0f) + 1.0f) * 0.5f;
}

// weight of a view at a surface point: cos of the angle between the normal (any length) and the direction d to the camera centre,
// max(0, cos)^power (two_sided: |cos|^power); a zero normal or a zero direction weighs 0
__device__ inline float mesh_view_weight(float nx, float ny, float nz, float dx, float dy, float dz, float power, int two_sided) {
  const float nn = nx * nx + ny * ny + nz * nz, dd = dx * dx + dy * dy + dz * dz;
  float wgt = 0.0f;
  if (nn > 0.0f && dd > 0.0f) {
    float cs = (nx * dx + ny * dy + nz * dz) / sqrtf(nn * dd);
    cs = two_sided ? fabsf(cs) : fmaxf(cs, 0.0f);
    cs = fminf(cs, 1.0f);
    wgt = cs > 0.0f ? powf(cs, power) : 0.0f;
  }
  return wgt;
}

// bilinear, clamp to edge, at the snapped position (xs / 16, ys / 16) of view n: the fractions are exact
__device__ inline void mesh_view_bilinear(const void* __restrict__ img, int dtype, int layout, int H, int W, int n, int xs, int ys, float c[3]) {
  const int j0 = xs >> MESH_SUB, i0 = ys >> MESH_SUB;
  const float fx = (float)(xs & (MESH_ONE - 1)) * (1.0f / MESH_ONE), fy = (float)(ys & (MESH_ONE - 1)) * (1.0f / MESH_ONE);
  const int ja = min(max(j0, 0), W - 1), jb = min(max(j0 + 1, 0), W - 1);
  const int ia = min(max(i0, 0), H - 1), ib = min(max(i0 + 1, 0), H - 1);
  for (int ch = 0; ch < 3; ++ch) {
    const float c00 = mesh_texel(img, dtype, layout, H, W, n, ch, ia, ja), c01 = mesh_texel(img, dtype, layout, H, W, n, ch, ia, jb);
    const float c10 = mesh_texel(img, dtype, layout, H, W, n, ch, ib, ja), c11 = mesh_texel(img, dtype, layout, H, W, n, ch, ib, jb);
    const float top = c00 + fx * (c01 - c00), bot = c10 + fx * (c11 - c10);
    c[ch] = top + fy * (bot - top);
  }
}

// the three int64 edge functions of a triangle (x, y in 1/16 units, AFTER the orientation swap that makes A > 0) at (px, py):
// e[k] belongs to the vertex k of the swapped triangle (include/mvd.h: mvd_op_mesh_raster); |e[k]| < 2^35
__device__ inline void mesh_edge_functions(const int x[3], const int y[3], long long px, long long py, long long e[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const long long dx = x[b] - x[a], dy = y[b] - y[a];
    e[k] = dx * (py - y[a]) - dy * (px - x[a]);
  }
}

// Closest point of triangle (a, b, c) to q (include/mvd.h: mvd_op_mesh_closest_point): the seven-region test in the fixed order
// corner a, corner b, edge ab, corner c, edge ac, edge bc, interior, the regions selected by predication (every lane runs the same
// instructions).  Every product and sum is written out and contraction is off, so that the search and the finalize pass, which
// inline this function into different kernels, get the same bits.  w: barycentrics >= 0; p = fma(w2, c, fma(w1, b, w0 a));
// returns |q - p|^2.  A zero denominator gives parameter 0; a NaN anywhere gives a NaN distance, which no comparison accepts.
__device__ __forceinline__ float mesh_dot3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

__device__ __forceinline__ float mesh_closest_on_triangle(const float q[3], const float a[3], const float b[3], const float c[3], float w[3],
                                                          float p[3]) {
#pragma clang fp contract(off)
  const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
  const float acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
  const float d1 = mesh_dot3(abx, aby, abz, q[0] - a[0], q[1] - a[1], q[2] - a[2]);
  const float d2 = mesh_dot3(acx, acy, acz, q[0] - a[0], q[1] - a[1], q[2] - a[2]);
  const float d3 = mesh_dot3(abx, aby, abz, q[0] - b[0], q[1] - b[1], q[2] - b[2]);
  const float d4 = mesh_dot3(acx, acy, acz, q[0] - b[0], q[1] - b[1], q[2] - b[2]);
  const float d5 = mesh_dot3(abx, aby, abz, q[0] - c[0], q[1] - c[1], q[2] - c[2]);
  const float d6 = mesh_dot3(acx, acy, acz, q[0] - c[0], q[1] - c[1], q[2] - c[2]);
  const float vc = __builtin_fmaf(d1, d4, -(d3 * d2)), vb = __builtin_fmaf(d5, d2, -(d1 * d6)), va = __builtin_fmaf(d3, d6, -(d5 * d4));
  const float e1 = d4 - d3, e2 = d5 - d6;
  const bool ra = d1 <= 0.0f && d2 <= 0.0f, rb = d3 >= 0.0f && d4 <= d3, rc = d6 >= 0.0f && d5 <= d6;
  const bool rab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f, rac = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
  const bool rbc = va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f;
  // one division serves whichever edge comes first in the order; the interior has its own two
  const float num = rab ? d1 : rac ? d2 : e1, den = rab ? d1 - d3 : rac ? d2 - d6 : e1 + e2;
  const float t = den != 0.0f ? num / den : 0.0f;
  const float sum = (va + vb) + vc;
  const float v = fmaxf(sum != 0.0f ? vb / sum : 0.0f, 0.0f), u = fmaxf(sum != 0.0f ? vc / sum : 0.0f, 0.0f);
  float w0 = fmaxf((1.0f - v) - u, 0.0f), w1 = v, w2 = u;  // interior
  if (rbc) w0 = 0.0f, w1 = 1.0f - t, w2 = t;
  if (rac) w0 = 1.0f - t, w1 = 0.0f, w2 = t;
  if (rc) w0 = 0.0f, w1 = 0.0f, w2 = 1.0f;
  if (rab) w0 = 1.0f - t, w1 = t, w2 = 0.0f;
  if (rb) w0 = 0.0f, w1 = 1.0f, w2 = 0.0f;
  if (ra) w0 = 1.0f, w1 = 0.0f, w2 = 0.0f;
  w[0] = w0, w[1] = w1, w[2] = w2;
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = __builtin_fmaf(w2, c[k], __builtin_fmaf(w1, b[k], w0 * a[k]));
  return mesh_dot3(q[0] - p[0], q[1] - p[1], q[2] - p[2], q[0] - p[0], q[1] - p[1], q[2] - p[2]);
}

// k_closest.hip: the exhaustive closest-point query (include/mvd.h: mvd_op_mesh_closest_point).  mesh_closest_check is the argument
// errors (0 = fine) and touches no device; query_normals may be null; slabs 0 = mesh_closest_slabs(Q, Nf), a host function.
int mesh_closest_slabs(int Q, int Nf);
int mesh_closest_check(const char* who, const float* queries, const float* verts, const int* faces, int Q, int Nv, int Nf, float cos_min,
                       float max_dist2, int slabs, const unsigned long long* key, const int* face, const float* bary, const float* point,
                       const float* dist2);
int launch_mesh_closest_point(const float* queries, const float* query_normals, const float* verts, const int* faces, int Q, int Nv, int Nf,
                              float cos_min, float max_dist2, int slabs, unsigned long long* key, int* face, float* bary, float* point,
                              float* dist2, hipStream_t s);

inline bool mesh_bad_image(int N, int H, int W) { return H < 1 || W < 1 || H > 4096 || W > 4096 || (long long)N * H * W > 0x7fffffffLL; }
