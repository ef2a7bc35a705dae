// Closest point on a triangle mesh by exhaustive search -- include/mvd.h: mvd_op_mesh_closest_point.  Exact, no spatial structure:
// the mesh it is asked about (a posed model) moves at every iteration of a fit, and brute force is what a numpy oracle can check.
// Launches:
//   closest_init_kernel      one thread per query: key = (bits(+inf) << 32) | 0xFFFFFFFF, "nothing found".
//   closest_search_kernel    a one-wave workgroup owns a tile of 256 queries, CP_QPT = 4 per lane in registers, and one slab of faces,
//                            walked in chunks of CP_CHUNK = 128 faces whose corners (and, with the normal gate, face normal and its
//                            length) a chunk's gather puts into LDS once, 64 bytes a face (8 KB: LDS does not bound the occupancy).  In the walk every lane reads the SAME
//                            LDS address -- a broadcast, no bank conflict -- and the six face edges' differences are computed once per
//                            lane and face for its four queries.  mesh_closest_on_triangle (csrc/mesh.h) selects its region by
//                            predication; the loop body has no branch that depends on the lane.  A face with an index outside
//                            [0, Nv) or a non-finite corner is stored as NaNs without being dereferenced: its distance is NaN and
//                            `d < best` never takes it; the same holds for a non-finite query.  A lane keeps (dist2, face) of the
//                            first smallest distance of its slab (faces ascending, strict <), then one 64-bit atomicMin of
//                            (bits(dist2) << 32) | face per query: dist2 >= 0, so its bits order as the floats do, and the smallest
//                            key is the smallest distance with ties to the smallest face, however faces are spread over slabs.
//                            The grid is tiles x slabs, flattened: 5023 queries are 20 tiles, and mesh_closest_slabs picks the slab
//                            count that brings the launch to one wave per SIMD of the chip (256 CUs x 4), never cutting a slab
//                            below one chunk.
//   closest_finalize_kernel  one thread per query: recomputes bary / point / dist2 of the winner with the same device function, so
//                            that dist2 equals the key's high word bit for bit; applies the distance gate; writes the no-match
//                            values (and puts the key back to "nothing found") otherwise.
#include "mesh.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace {

constexpr int CP_T = 64, CP_QPT = 4, CP_TILE = CP_T * CP_QPT, CP_CHUNK = 128, CP_FILL = 256 * 4;
constexpr unsigned long long CP_NONE = (0x7f800000ull << 32) | 0xffffffffull;

__device__ __forceinline__ bool cp_finite3(const float* p) { return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY; }

__global__ __launch_bounds__(256) void closest_init_kernel(unsigned long long* __restrict__ key, int Q) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < Q) key[q] = CP_NONE;
}

template <bool GATE>
__global__ __launch_bounds__(CP_T) void closest_search_kernel(const float* __restrict__ queries, const float* __restrict__ qn,
                                                              const float* __restrict__ verts, const int* __restrict__ faces, int Q, int Nv,
                                                              int Nf, int slabs, int per_slab, float cos_min,
                                                              unsigned long long* __restrict__ key) {
  __shared__ float4 tri[CP_CHUNK * 4];  // face j of the chunk: (ax ay az bx) (by bz cx cy) (cz - - -) (Nx Ny Nz |N|)
  const int tile = blockIdx.x / slabs, slab = blockIdx.x - tile * slabs, lane = threadIdx.x;
  const int f_lo = slab * per_slab;  // slabs <= Nf and per_slab = ceil(Nf / slabs): below 2 Nf, no overflow
  if (f_lo >= Nf) return;            // a slab past the last face (uniform over the workgroup)
  const int f_hi = min(Nf, f_lo + per_slab);

  const float nan = __builtin_nanf("");
  float q[CP_QPT][3], n[CP_QPT][3], nlen[CP_QPT], best[CP_QPT];
  int best_f[CP_QPT];
#pragma unroll
  for (int i = 0; i < CP_QPT; ++i) {
    const int qi = tile * CP_TILE + i * CP_T + lane;  // consecutive lanes read consecutive queries
    const bool in = qi < Q;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      q[i][k] = in ? queries[(size_t)qi * 3 + k] : nan;
      n[i][k] = GATE && in ? qn[(size_t)qi * 3 + k] : 0.0f;
    }
    nlen[i] = sqrtf(mesh_dot3(n[i][0], n[i][1], n[i][2], n[i][0], n[i][1], n[i][2]));
    best[i] = INFINITY, best_f[i] = -1;
  }

  for (int c0 = f_lo; c0 < f_hi; c0 += CP_CHUNK) {
    const int cn = min(CP_CHUNK, f_hi - c0);
    __syncthreads();  // the previous chunk has been walked
    for (int j = lane; j < cn; j += CP_T) {
      const int f = c0 + j;
      const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
      float a[3] = {nan, nan, nan}, b[3] = {nan, nan, nan}, c[3] = {nan, nan, nan};
      if ((unsigned)i0 < (unsigned)Nv && (unsigned)i1 < (unsigned)Nv && (unsigned)i2 < (unsigned)Nv) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = verts[(size_t)i0 * 3 + k], b[k] = verts[(size_t)i1 * 3 + k], c[k] = verts[(size_t)i2 * 3 + k];
        if (!(cp_finite3(a) && cp_finite3(b) && cp_finite3(c))) {
#pragma unroll
          for (int k = 0; k < 3; ++k) a[k] = b[k] = c[k] = nan;
        }
      }
      tri[j * 4 + 0] = make_float4(a[0], a[1], a[2], b[0]);
      tri[j * 4 + 1] = make_float4(b[1], b[2], c[0], c[1]);
      tri[j * 4 + 2] = make_float4(c[2], 0.0f, 0.0f, 0.0f);
      if (GATE) {
#pragma clang fp contract(off)
        const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2], acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
        const float nx = __builtin_fmaf(aby, acz, -(abz * acy)), ny = __builtin_fmaf(abz, acx, -(abx * acz)),
                    nz = __builtin_fmaf(abx, acy, -(aby * acx));
        tri[j * 4 + 3] = make_float4(nx, ny, nz, sqrtf(mesh_dot3(nx, ny, nz, nx, ny, nz)));
      }
    }
    __syncthreads();
    for (int j = 0; j < cn; ++j) {
      const float4 t0 = tri[j * 4 + 0], t1 = tri[j * 4 + 1], t2 = tri[j * 4 + 2];
      const float a[3] = {t0.x, t0.y, t0.z}, b[3] = {t0.w, t1.x, t1.y}, c[3] = {t1.z, t1.w, t2.x};
      float4 fn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (GATE) fn = tri[j * 4 + 3];
#pragma unroll
      for (int i = 0; i < CP_QPT; ++i) {
        float w[3], p[3];
        const float d = mesh_closest_on_triangle(q[i], a, b, c, w, p);
        bool take = d < best[i];
        if (GATE) {
#pragma clang fp contract(off)
          take = take && mesh_dot3(n[i][0], n[i][1], n[i][2], fn.x, fn.y, fn.z) >= cos_min * (nlen[i] * fn.w);
        }
        best[i] = take ? d : best[i];
        best_f[i] = take ? c0 + j : best_f[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CP_QPT; ++i) {
    const int qi = tile * CP_TILE + i * CP_T + lane;
    if (qi < Q && best_f[i] >= 0)
      atomicMin(key + qi, ((unsigned long long)__float_as_uint(best[i]) << 32) | (unsigned long long)(unsigned)best_f[i]);
  }
}

__global__ __launch_bounds__(256) void closest_finalize_kernel(const float* __restrict__ queries, const float* __restrict__ verts,
                                                               const int* __restrict__ faces, int Q, int Nv, int Nf, float max_dist2,
                                                               unsigned long long* __restrict__ key, int* __restrict__ face,
                                                               float* __restrict__ bary, float* __restrict__ point,
                                                               float* __restrict__ dist2) {
  const int qi = blockIdx.x * 256 + threadIdx.x;
  if (qi >= Q) return;
  const unsigned f = (unsigned)(key[qi] & 0xffffffffull);
  float w[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f}, d = INFINITY;
  int fo = -1;
  if (f < (unsigned)Nf) {  // a winner: the search has checked its indices and corners
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((unsigned)i0 < (unsigned)Nv && (unsigned)i1 < (unsigned)Nv && (unsigned)i2 < (unsigned)Nv) {
      float q[3], a[3], b[3], c[3], ww[3], pp[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        q[k] = queries[(size_t)qi * 3 + k], a[k] = verts[(size_t)i0 * 3 + k], b[k] = verts[(size_t)i1 * 3 + k], c[k] = verts[(size_t)i2 * 3 + k];
      const float dd = mesh_closest_on_triangle(q, a, b, c, ww, pp);
      if (dd <= max_dist2) {
        d = dd, fo = (int)f;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = ww[k], p[k] = pp[k];
      }
    }
  }
  if (fo < 0) key[qi] = CP_NONE;
  face[qi] = fo, dist2[qi] = d;
#pragma unroll
  for (int k = 0; k < 3; ++k) bary[(size_t)qi * 3 + k] = w[k], point[(size_t)qi * 3 + k] = p[k];
}

int closest_fail(const char* who, const char* what) { return mvd_fail((std::string(who) + what).c_str()); }

}  // namespace

// The planned slab count, a function of (Q, Nf) alone: enough slabs that tiles x slabs reaches one wave per SIMD of the chip, at
// most one per chunk of faces; 1 when the query tiles fill the chip by themselves.
int mesh_closest_slabs(int Q, int Nf) {
  if (Q < 1 || Nf < 1) return 1;
  const long long tiles = ((long long)Q + CP_TILE - 1) / CP_TILE, chunks = ((long long)Nf + CP_CHUNK - 1) / CP_CHUNK;
  const long long want = (CP_FILL + tiles - 1) / tiles;
  return (int)std::max(1LL, std::min(want, chunks));
}

int mesh_closest_check(const char* who, const float* queries, const float* verts, const int* faces, int Q, int Nv, int Nf, float cos_min,
                       float max_dist2, int slabs, const unsigned long long* key, const int* face, const float* bary, const float* point,
                       const float* dist2) {
  if (!queries || !verts || !faces || !key || !face || !bary || !point || !dist2) return closest_fail(who, ": null argument");
  if (Q < 1 || Nv < 1 || Nf < 1) return closest_fail(who, ": Q, Nv and Nf must be at least 1");
  if (Q > 0x2aaaaaaa || Nv > 0x2aaaaaaa || Nf > 0x2aaaaaaa) return closest_fail(who, ": 3 Q, 3 Nv and 3 Nf must be below 2^31");
  if (!(max_dist2 > 0.0f)) return closest_fail(who, ": max_dist2 must be positive (+inf: no gate)");
  if (!(cos_min >= -1.0f && cos_min <= 1.0f)) return closest_fail(who, ": cos_min must be in [-1, 1]");
  if (slabs < 0) return closest_fail(who, ": slabs must be 0 (planned) or a positive count");
  return 0;
}

int launch_mesh_closest_point(const float* queries, const float* query_normals, const float* verts, const int* faces, int Q, int Nv, int Nf,
                              float cos_min, float max_dist2, int slabs, unsigned long long* key, int* face, float* bary, float* point,
                              float* dist2, hipStream_t s) {
  const long long tiles = ((long long)Q + CP_TILE - 1) / CP_TILE;
  // more slabs than faces, or than a grid holds, would only add empty ones: the result does not depend on the count
  long long ns = std::min<long long>(slabs > 0 ? slabs : mesh_closest_slabs(Q, Nf), Nf);
  ns = std::max(1LL, std::min(ns, 0x7fffffffLL / tiles));
  const int per_slab = (int)(((long long)Nf + ns - 1) / ns);
  const unsigned qblocks = (unsigned)((Q + 255) / 256);
  hipLaunchKernelGGL(closest_init_kernel, dim3(qblocks), dim3(256), 0, s, key, Q);
  HIP_CHECK_RET(hipGetLastError());
  if (query_normals)
    hipLaunchKernelGGL(closest_search_kernel<true>, dim3((unsigned)(tiles * ns)), dim3(CP_T), 0, s, queries, query_normals, verts, faces, Q, Nv,
                       Nf, (int)ns, per_slab, cos_min, key);
  else
    hipLaunchKernelGGL(closest_search_kernel<false>, dim3((unsigned)(tiles * ns)), dim3(CP_T), 0, s, queries, query_normals, verts, faces, Q, Nv,
                       Nf, (int)ns, per_slab, cos_min, key);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(closest_finalize_kernel, dim3(qblocks), dim3(256), 0, s, queries, verts, faces, Q, Nv, Nf, max_dist2, key, face, bary,
                     point, dist2);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
