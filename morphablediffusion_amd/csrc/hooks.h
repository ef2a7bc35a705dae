// The scaffold of the per-op test and bench hooks (include/mvd.h: "per-op hooks"), shared by the two translation units that
// define them: c_api_hooks.hip (the forward, norm, attention and bench hooks) and engine_train.hip (the backward, adjoint and
// gather hooks, which call that file's file-local functions).  Everything here has internal linkage.
#pragma once
#include <string>

#include "engine.h"

// every hook starts here: no hook touches a null context
static inline int hook_begin(mvd_ctx* c) {
  if (!c) return mvd_fail("null context");
  if (hipSetDevice(c->device) != hipSuccess) return mvd_fail("hipSetDevice failed");
  return 0;
}

// the free part of the workspace -> 0xFF bytes (NaN as fp16, bf16 and fp32): a read of anything the op did not write shows
// in its result
static inline int hook_poison(mvd_ctx* c, hipStream_t s) {
  const size_t o = (c->ws.off + 255) & ~(size_t)255;
  if (o < c->ws.size) HIP_CHECK_RET(hipMemsetAsync(c->ws.base + o, 0xFF, c->ws.size - o, s));
  return 0;
}

// the end of a synchronous hook: the stream is synchronised whatever rc says, and a failure there is reported under `who`
static inline int hook_sync(const char* who, hipStream_t s, int rc) {
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = mvd_fail((std::string(who) + ": stream synchronisation failed").c_str());
  return rc;
}

// an fp32 operand the caller supplies as the fp16 image the production path reads
static inline int hook_f16(mvd_ctx* c, const float* src, size_t n, const half_t** out, hipStream_t s) {
  half_t* d = ws_alloc<half_t>(c, n);
  WS_CHECK(d);
  RET_IF(launch_f32_to_f16(src, d, n, s));
  *out = d;
  return 0;
}

// blocks of 256 threads for the hooks' own element-wise kernels (grid-stride: the grid does not change a result)
static inline int hook_blocks(size_t n) {
  const size_t g = (n + 255) / 256;
  return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}
static __global__ void f16_to_f32_kernel(const half_t* in, float* out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = (float)in[i];
}
// a 16-bit result back to the caller's fp32 buffer; the caller asks hipGetLastError
static inline void hook_f16_to_f32(const half_t* in, float* out, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(hook_blocks(n)), dim3(256), 0, s, in, out, n);
}

// w fp32 in the reference layout ([N][cin][taps], transposed: [cin][N][taps]) -> the forward pack in the workspace and the
// ConvW that describes it: Cl = cin rounded up to 8 columns, or [w_hi | w_hi | w_lo] rows of 3 Cl with xp (as pack_conv does).
// The bias and the other forms of the weights (conv3x stream, folded upsample slabs, adjoint pack) are the caller's.
static inline int hook_pack_fwd(mvd_ctx* c, const float* w, int N, int cin, int taps, int transposed, int geglu, int xp, ConvW* o,
                                hipStream_t s) {
  const int Cl = (cin + 7) & ~7;
  o->N = N;
  o->taps = taps;
  o->xp = xp ? 1 : 0;
  o->cin_l = Cl;
  o->Cin = xp ? 3 * Cl : Cl;
  o->w = ws_alloc<half_t>(c, (size_t)taps * N * o->Cin);
  WS_CHECK(o->w);
  return launch_pack_weight(w, N, o->Cin, taps, transposed, geglu, o->w, s, cin, o->xp);
}

// A pair of timing events that is destroyed on every exit path.  run(): `n` calls of `call` on `s` between the two events; the
// elapsed milliseconds are ADDED to *ms (a loop that must do something before each timed launch calls run(s, 1, ...) per launch).
struct HookTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HookTimer() = default;
  ~HookTimer() {
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
  }
  HookTimer(const HookTimer&) = delete;
  HookTimer& operator=(const HookTimer&) = delete;
  template <typename F>
  int run(hipStream_t s, int n, F&& call, float* ms) {
    if (!e0) HIP_CHECK_RET(hipEventCreate(&e0));
    if (!e1) HIP_CHECK_RET(hipEventCreate(&e1));
    HIP_CHECK_RET(hipEventRecord(e0, s));
    for (int i = 0; i < n; ++i) RET_IF(call());
    HIP_CHECK_RET(hipEventRecord(e1, s));
    HIP_CHECK_RET(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_CHECK_RET(hipEventElapsedTime(&t, e0, e1));
    *ms += t;
    return 0;
  }
};
// mean milliseconds of `iters` back-to-back calls
template <typename F>
static inline int hook_time(hipStream_t s, int iters, F&& call, float* mean_ms) {
  HookTimer t;
  float ms = 0.f;
  RET_IF(t.run(s, iters, call, &ms));
  *mean_ms = ms / (float)iters;
  return 0;
}
