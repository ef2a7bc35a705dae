// Coordinate maps of the mesh conditioner's gathers, shared by k_cond.hip (forward) and k_cond_bwd.hip (atomic and deterministic
// adjoints).  Forward gather, atomic adjoint and deterministic adjoint of a map call the SAME function: the adjoints are
// transposes, and the deterministic ones decide membership, only as long as all three compute the same fp32 coordinates.  A
// change to a map is made here and nowhere else.  Guards and clamps that differ between kernels stay in the kernels.
#pragma once
#include "common.h"

// torch.linspace(a, b, n)[i] in fp32 (symmetric evaluation, as ATen does)
static __device__ __forceinline__ float linspace_at(float a, float b, int n, int i) {
  const float step = (b - a) / (float)(n - 1);
  return i < n / 2 ? a + step * (float)i : b - step * (float)(n - 1 - i);
}

// vertex vi -> its position on the V^3 lattice along axis a; then the cell: floor and fraction per axis
static __device__ __forceinline__ float vertex_axis_pos(const float* __restrict__ verts, int vi, int a, int V, float vol_len) {
  const float g = verts[vi * 3 + a] / vol_len;
  return (g + 1.0f) * 0.5f * (float)(V - 1);
}
static __device__ __forceinline__ void vertex_cell(const float* __restrict__ verts, int vi, int V, float vol_len, int lo[3], float fr[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float pos = vertex_axis_pos(verts, vi, a, V, vol_len);
    const float f = floorf(pos);
    lo[a] = (int)f;
    fr[a] = pos - f;
  }
}

// lattice voxel (ix, iy, iz) -> pixel position in the S x S feature map of the view with projection rows P (depth clamped at 1e-4)
static __device__ __forceinline__ void lattice_to_map(const float* P, int ix, int iy, int iz, int V, float vol_len, int S, int persp,
                                                      float& px, float& py) {
  const float X = linspace_at(-vol_len, vol_len, V, ix), Y = linspace_at(-vol_len, vol_len, V, iy),
              Z = linspace_at(-vol_len, vol_len, V, iz);
  const float u = P[0] * X + P[1] * Y + P[2] * Z + P[3];
  const float v = P[4] * X + P[5] * Y + P[6] * Z + P[7];
  if (persp) {
    float w = P[8] * X + P[9] * Y + P[10] * Z + P[11];
    w = w < 1e-4f ? 1e-4f : w;
    const float hs = (float)(S - 1) * 0.5f;
    px = ((u / w) / hs - 1.0f + 1.0f) * 0.5f * (float)(S - 1);
    py = ((v / w) / hs - 1.0f + 1.0f) * 0.5f * (float)(S - 1);
  } else {
    px = (u + 1.0f) * 0.5f * (float)(S - 1);
    py = (v + 1.0f) * 0.5f * (float)(S - 1);
  }
}

// frustum point (x, y, d) of a target view -> position on the V^3 lattice
static __device__ __forceinline__ void frustum_to_lattice(const ViewCam& cam, int x, int y, int d, int D, int S, int V, float vol_len,
                                                          int persp, float& px, float& py, float& pz) {
  const float depth = linspace_at(0.f, 1.f, D, d) * (cam.far_ - cam.near_) + cam.near_;
  float wx, wy, wz;
  if (persp) {
    const float a = (float)x * depth, b = (float)y * depth, c = depth;
    wx = cam.Pinv[0] * a + cam.Pinv[1] * b + cam.Pinv[2] * c + cam.Pinv[3];
    wy = cam.Pinv[4] * a + cam.Pinv[5] * b + cam.Pinv[6] * c + cam.Pinv[7];
    wz = cam.Pinv[8] * a + cam.Pinv[9] * b + cam.Pinv[10] * c + cam.Pinv[11];
  } else {
    const float gx = 2.f * (float)x / (float)(S - 1) - 1.f, gy = 2.f * (float)y / (float)(S - 1) - 1.f;
    const float a = cam.Kinv[0] * gx + cam.Kinv[1] * gy + cam.Kinv[2];
    const float b = cam.Kinv[3] * gx + cam.Kinv[4] * gy + cam.Kinv[5];
    const float c = depth;
    wx = cam.Pinv[0] * a + cam.Pinv[1] * b + cam.Pinv[2] * c + cam.Pinv[3];
    wy = cam.Pinv[4] * a + cam.Pinv[5] * b + cam.Pinv[6] * c + cam.Pinv[7];
    wz = cam.Pinv[8] * a + cam.Pinv[9] * b + cam.Pinv[10] * c + cam.Pinv[11];
  }
  px = (wx / vol_len + 1.f) * 0.5f * (float)(V - 1);
  py = (wy / vol_len + 1.f) * 0.5f * (float)(V - 1);
  pz = (wz / vol_len + 1.f) * 0.5f * (float)(V - 1);
}

// lattice index i -> position on one axis of the sparse grid (g cells, origin mn, sh * voxel long)
static __device__ __forceinline__ float latent_axis_pos(float mn, float sh, int g, float voxel, int V, float vol_len, int i) {
  const float X = linspace_at(-vol_len, vol_len, V, i);
  const float gx = (X - mn) / voxel / sh * 2.f - 1.f;
  return (gx + 1.f) * 0.5f * (float)(g - 1);
}

// weight of the corner (bx, by, bz) of a cell at fractions (tx, ty, tz), of the tap (tap & 1, tap >> 1) of a pixel at (tx, ty)
static __device__ __forceinline__ float trilinear_weight(int bx, int by, int bz, float tx, float ty, float tz) {
  return (bx ? tx : 1.f - tx) * (by ? ty : 1.f - ty) * (bz ? tz : 1.f - tz);
}
static __device__ __forceinline__ float bilinear_weight(int tap, float tx, float ty) {
  return ((tap & 1) ? tx : 1.f - tx) * ((tap >> 1) ? ty : 1.f - ty);
}
