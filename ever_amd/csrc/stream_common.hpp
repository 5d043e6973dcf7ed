// What the streaming translation units share — pointwise.hip: element-wise and layout kernels; pool.hip: pools and
// selections; resample.hip: bilinear resampling; relation.hip: FS-Relation — the NHWC element decode, the argument check of an
// NHWC map and the one-element-per-thread launch.  Header only.
#pragma once
#include "common.hpp"

namespace evk {

// Element i of a map [N][H][W][C / VEC] (cv = C / VEC elements per pixel): image, row, column, channel chunk.  H and W are
// the dims of the map that is being WALKED — the call site names it.
struct NhwcElem {
  int n, y, x, cb;
};
__device__ __forceinline__ NhwcElem nhwc_elem(size_t i, int H, int W, int cv) {
  NhwcElem e;
  e.cb = (int)(i % cv);
  size_t pix = i / cv;
  e.x = (int)(pix % W);
  pix /= W;
  e.y = (int)(pix % H);
  e.n = (int)(pix / H);
  return e;
}

// an NHWC map (H = HW, W = 1 for the kernels that take pixels as one axis) of 16-byte channel chunks
inline bool nhwc4_ok(int N, int H, int W, int C) { return N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0; }

// kernel<<<grid_for(n), 256>>>(args...) for a kernel that takes one of its n elements per thread, and the launch check
// under the entry point's name
template <typename... KArgs, typename... Args>
inline int launch_elems(const char* what, void (*kernel)(KArgs...), size_t n, void* stream, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, static_cast<KArgs>(args)...);
  return check_launch(what);
}

}  // namespace evk
