// Image products ("Image products"): the canvas of TrackBase::display_history
// (TrackBase.cpp:119-228) and the square-per-track image of ROS1Visualizer::publish_loopclosure_information
// (ROS1Visualizer.cpp:950-996), rendered over level 0 of the pyramids that are already in HBM.
//
// The reference draws its primitives one after the other and a later one overwrites an earlier one.  Here the
// primitives are numbered in that order and drawn all at once:
//   k_viz_base     gray -> 3 channels into the canvas (black where a camera is smaller than its cell) and the
//                  priority plane cleared, four pixels per thread
//   k_viz_prims    one thread per primitive pixel: atomicMax of (number << 24 | colour) into the pixel's plane word;
//                  the highest number is the primitive drawn last, whatever order the threads run in
//   k_viz_compose  the plane's winners written over the base, then the mask tint; four pixels per thread
// Integer work throughout: the output is the same bytes on every run.
#include "kernels.h"

namespace uvhp {

constexpr int kVizPix = 4;  // canvas pixels per thread of the base and compose kernels

// camera slot and x inside the camera's cell for canvas column x; false in the padding right of / below the image
__device__ __forceinline__ bool viz_locate(const VizJob &job, int x, int y, int &c, int &lx) {
  c = x / job.cw;
  lx = x - c * job.cw;
  return lx < job.w[c] && y < job.h[c];
}

// twelve canvas bytes at a 4-pixel group: three aligned words when the row length and the canvas allow it
template <bool kWords>
__device__ __forceinline__ void viz_store(uint8_t *p, const uint8_t (&b)[3 * kVizPix], int n) {
  if (kWords) {
    unsigned *q = reinterpret_cast<unsigned *>(p);
#pragma unroll
    for (int k = 0; k < 3; k++)
      q[k] = (unsigned)b[4 * k] | (unsigned)b[4 * k + 1] << 8 | (unsigned)b[4 * k + 2] << 16 | (unsigned)b[4 * k + 3] << 24;
  } else {
    for (int k = 0; k < 3 * n; k++) p[k] = b[k];
  }
}

template <bool kWords>
__global__ void __launch_bounds__(256) k_viz_base(VizJob job) {
  const int W = job.ncam * job.cw;
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * kVizPix, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x0 >= W || y >= job.ch) return;
  const int n = min(kVizPix, W - x0);  // (kWords: W is a multiple of kVizPix, so n == kVizPix)
  uint8_t b[3 * kVizPix];
#pragma unroll
  for (int k = 0; k < kVizPix; k++) {
    uint8_t g = 0;
    int c, lx;
    if (k < n && viz_locate(job, x0 + k, y, c, lx)) g = job.img[c][(size_t)y * job.stride[c] + lx];
    b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = g;
  }
  const size_t idx = (size_t)y * W + x0;
  viz_store<kWords>(job.canvas + 3 * idx, b, n);
  for (int k = 0; k < n; k++) job.plane[idx + k] = 0ull;
}

// Pixel k of a primitive, in the camera's own coordinates.
//   disc, radius 1: the plus; radius 2: rows dy = -2 and 2 with |dx| <= 1, rows |dy| <= 1 with |dx| <= 2
//   segment: 8-connected, n = max(|dx|, |dy|) steps; step i moves i along the major axis (x when |dx| >= |dy|) and
//            (2 i |d_minor| + n) div 2n along the minor one, each in the direction of its sign
//   rectangle: the four one-pixel edges (top, bottom, left, right; the corners come twice, in the same colour)
//   filled rectangle: row-major
__device__ __forceinline__ void viz_pixel(const DVizPrim &p, int kind, int k, int &x, int &y) {
  switch (kind) {
    case VIZ_DISC1: {
      const int dx = (k == 1) ? -1 : (k == 3) ? 1 : 0, dy = (k == 0) ? -1 : (k == 4) ? 1 : 0;
      x = p.x0 + dx;
      y = p.y0 + dy;
      return;
    }
    case VIZ_DISC2: {
      int dx, dy;
      if (k < 3) {
        dy = -2, dx = k - 1;
      } else if (k < 18) {
        dy = (k - 3) / 5 - 1, dx = (k - 3) % 5 - 2;
      } else {
        dy = 2, dx = k - 19;
      }
      x = p.x0 + dx;
      y = p.y0 + dy;
      return;
    }
    case VIZ_SEG: {
      const int dx = p.x1 - p.x0, dy = p.y1 - p.y0, ax = abs(dx), ay = abs(dy), n = max(ax, ay);
      const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
      const long long i = p.i0 + k;
      if (n == 0) {
        x = p.x0, y = p.y0;
      } else if (ax >= ay) {
        x = p.x0 + sx * (int)i;
        y = p.y0 + sy * (int)((2 * i * ay + n) / (2ll * n));
      } else {
        y = p.y0 + sy * (int)i;
        x = p.x0 + sx * (int)((2 * i * ax + n) / (2ll * n));
      }
      return;
    }
    case VIZ_RECT: {
      const int w = p.x1 - p.x0 + 1, h = p.y1 - p.y0 + 1;
      if (k < w) {
        x = p.x0 + k, y = p.y0;
      } else if (k < 2 * w) {
        x = p.x0 + k - w, y = p.y1;
      } else if (k < 2 * w + h) {
        x = p.x0, y = p.y0 + k - 2 * w;
      } else {
        x = p.x1, y = p.y0 + k - 2 * w - h;
      }
      return;
    }
    default: {  // VIZ_FILL
      const int w = p.x1 - p.x0 + 1;
      x = p.x0 + k % w;
      y = p.y0 + k / w;
      return;
    }
  }
}

__global__ void __launch_bounds__(256) k_viz_prims(VizJob job) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= job.npix) return;
  // the primitive whose pixel range holds g: the last one with first <= g
  int lo = 0, hi = job.nprim - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (job.prims[mid].first <= g)
      lo = mid;
    else
      hi = mid - 1;
  }
  const DVizPrim p = job.prims[lo];
  const int kind = p.kind_cam & 255, c = p.kind_cam >> 8;
  int x, y;
  viz_pixel(p, kind, g - p.first, x, y);
  // clipped to the camera's own image, not to its cell
  if (x < 0 || y < 0 || x >= job.w[c] || y >= job.h[c]) return;
  const size_t idx = (size_t)y * ((size_t)job.ncam * job.cw) + (size_t)c * job.cw + x;
  atomicMax(job.plane + idx, ((unsigned long long)(lo + 1) << 24) | p.colour);
}

template <bool kWords>
__global__ void __launch_bounds__(256) k_viz_compose(VizJob job) {
  const int W = job.ncam * job.cw;
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * kVizPix, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x0 >= W || y >= job.ch) return;
  const int n = min(kVizPix, W - x0);
  const size_t idx = (size_t)y * W + x0;
  unsigned long long pw[kVizPix];
  bool tint[kVizPix], any = false;
#pragma unroll
  for (int k = 0; k < kVizPix; k++) {
    pw[k] = 0ull;
    tint[k] = false;
    if (k >= n) continue;
    pw[k] = job.plane[idx + k];
    int c, lx;
    if (viz_locate(job, x0 + k, y, c, lx) && job.mask[c])
      tint[k] = job.mask[c][(size_t)y * job.w[c] + lx] > 127;
    any |= pw[k] != 0ull || tint[k];
  }
  if (!any) return;  // the base stands
  uint8_t b[3 * kVizPix];
  uint8_t *dst = job.canvas + 3 * idx;
  for (int k = 0; k < 3 * n; k++) b[k] = dst[k];
#pragma unroll
  for (int k = 0; k < kVizPix; k++) {
    if (pw[k] != 0ull) {
      const unsigned col = (unsigned)pw[k] & 0xffffffu;
      b[3 * k] = (uint8_t)col, b[3 * k + 1] = (uint8_t)(col >> 8), b[3 * k + 2] = (uint8_t)(col >> 16);
    }
    // addWeighted(mask, 0.1, img, 1.0, 0) with the mask colour (0, 0, 255): p + 25.5 rounded half to even
    if (tint[k]) {
      const int v = b[3 * k + 2];
      b[3 * k + 2] = (uint8_t)min(255, v + 25 + ((v & 1) ? 0 : 1));
    }
  }
  viz_store<kWords>(dst, b, n);
}

static dim3 viz_grid(const VizJob &job) {
  const int W = job.ncam * job.cw;
  return dim3((W + 64 * kVizPix - 1) / (64 * kVizPix), (job.ch + 3) / 4);
}
static bool viz_words(const VizJob &job) {
  return (job.ncam * job.cw) % kVizPix == 0 && (reinterpret_cast<uintptr_t>(job.canvas) & 3) == 0;
}

void launch_viz_base(hipStream_t s, const VizJob &job) {
  if (job.ncam <= 0 || job.cw <= 0 || job.ch <= 0) return;
  if (viz_words(job))
    hipLaunchKernelGGL(k_viz_base<true>, viz_grid(job), dim3(256), 0, s, job);
  else
    hipLaunchKernelGGL(k_viz_base<false>, viz_grid(job), dim3(256), 0, s, job);
}

void launch_viz_prims(hipStream_t s, const VizJob &job) {
  if (job.nprim <= 0 || job.npix <= 0) return;
  hipLaunchKernelGGL(k_viz_prims, dim3((job.npix + 255) / 256), dim3(256), 0, s, job);
}

void launch_viz_compose(hipStream_t s, const VizJob &job) {
  if (job.ncam <= 0 || job.cw <= 0 || job.ch <= 0) return;
  if (viz_words(job))
    hipLaunchKernelGGL(k_viz_compose<true>, viz_grid(job), dim3(256), 0, s, job);
  else
    hipLaunchKernelGGL(k_viz_compose<false>, viz_grid(job), dim3(256), 0, s, job);
}

}  // namespace uvhp
