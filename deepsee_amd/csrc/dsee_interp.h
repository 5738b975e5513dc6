// F.interpolate(x, (OH, OW), mode) for mode = bicubic | bilinear | nearest | area on a native NHWC image, one scale per axis: what
// dsee_bicubic_down (elementwise.hip), dsee_interp_down and dsee_resize_hw (resample.hip) share, so that for a square output
// dsee_resize_hw gives the bits of the two older entry points.
#pragma once
#include "dsee_common.h"

enum { INTERP_BILINEAR = 0, INTERP_NEAREST = 1, INTERP_AREA = 2, INTERP_BICUBIC = 3 };

// mode = bicubic is ONE kernel for every entry point (elementwise.hip: bicubic_hw_kernel), reached through this launcher
namespace dsee {
int launch_bicubic_hw(const float* x, float* y, int N, int H, int W, int OH, int OW, int cs_in, int cs_out, int clamp, hipStream_t st);
}

// source index and weight of the upper neighbour of ATen's upsample_bilinear2d (align_corners = False)
__device__ __forceinline__ void bilinear_tap(float scale, int dst, int in, int& i0, int& i1, float& l1) {
  const float s = fmaxf(scale * (dst + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

// mode = bilinear | nearest | area: the 3 channels of output pixel (oh, ow) of an OH x OW output into v, which the caller has set to
// zero; sh = (float)H / OH, sw = (float)W / OW from the host, so that the nearest index is the one ATen computes:
// min((int)floorf(dst * scale), in - 1)
__device__ __forceinline__ void dsee_interp_px(const float* __restrict__ img, int H, int W, int OH, int OW, int cs_in, int mode,
                                               float sh, float sw, int oh, int ow, float (&v)[3]) {
  if (mode == INTERP_NEAREST) {
    const int iy = min((int)floorf(oh * sh), H - 1), ix = min((int)floorf(ow * sw), W - 1);
    for (int c = 0; c < 3; ++c) v[c] = img[((size_t)iy * W + ix) * cs_in + c];
  } else if (mode == INTERP_BILINEAR) {
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_tap(sh, oh, H, y0, y1, ly);
    bilinear_tap(sw, ow, W, x0, x1, lx);
    for (int c = 0; c < 3; ++c) {
      const float a = img[((size_t)y0 * W + x0) * cs_in + c], b = img[((size_t)y0 * W + x1) * cs_in + c];
      const float d = img[((size_t)y1 * W + x0) * cs_in + c], e = img[((size_t)y1 * W + x1) * cs_in + c];
      v[c] = (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * d + lx * e);
    }
  } else {  // adaptive average: rows floor(i in / out) ... ceil((i + 1) in / out)
    const int ya = (int)(((long)oh * H) / OH), yb = (int)((((long)oh + 1) * H + OH - 1) / OH);
    const int xa = (int)(((long)ow * W) / OW), xb = (int)((((long)ow + 1) * W + OW - 1) / OW);
    for (int yy = ya; yy < yb; ++yy) {
      float row[3] = {0.f, 0.f, 0.f};
      for (int xx = xa; xx < xb; ++xx)
        for (int c = 0; c < 3; ++c) row[c] += img[((size_t)yy * W + xx) * cs_in + c];
      for (int c = 0; c < 3; ++c) v[c] += row[c];
    }
    const float inv = (float)((yb - ya) * (xb - xa));
    for (int c = 0; c < 3; ++c) v[c] /= inv;
  }
}
