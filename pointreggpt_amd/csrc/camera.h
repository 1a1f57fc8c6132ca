// camera.h — the pinhole camera arithmetic shared by geometry.hip and posesearch.hip: the SE(3) move and the pixel a camera-frame
// point lands in.  Built with -ffp-contract=off: every float op is written in the exact order torch / numpy evaluate the reference
// expressions, fused multiply-adds only where the host BLAS uses them (the 3x3 rotation: fma chain in k order — probed, see
// DESIGN.md), so the integer pixel indices and the float32 depths come out bit-identical to the reference.
#pragma once
#include "common.h"

namespace prg {

static constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // z-buffer sentinel: above every positive float's bit pattern

struct Cam {
  float fx, fy, cx, cy;
};
__device__ inline Cam load_cam(const float* K, int b) {
  const float* k = K + (size_t)b * 9;
  return Cam{k[0], k[4], k[2], k[5]};
}

// rotate + translate exactly like `pc @ R^T + t` on the host: fma chain over k = 0,1,2, then a separate add.
__device__ inline void se3_apply(const float* P, float x, float y, float z, float& ox, float& oy, float& oz) {
  // P row-major 4x4: R[j][k] = P[j*4+k], t[j] = P[j*4+3]
  float v;
  v = x * P[0]; v = __fmaf_rn(y, P[1], v); v = __fmaf_rn(z, P[2], v); ox = v + P[3];
  v = x * P[4]; v = __fmaf_rn(y, P[5], v); v = __fmaf_rn(z, P[6], v); oy = v + P[7];
  v = x * P[8]; v = __fmaf_rn(y, P[9], v); v = __fmaf_rn(z, P[10], v); oz = v + P[11];
}

// the pixel of one camera-frame point (sd:225-258): false when the z-buffer does not take it (z <= 0 or NaN, out of frame)
__device__ inline bool splat_pixel(const Cam& c, float x, float y, float z, int H, int W, size_t& pix) {
  if (!(z > 0.0f)) return false;  // also rejects NaN
  float fc = rintf(x * c.fx / z + c.cx);  // torch.round = round-half-even
  float fr = rintf(y * c.fy / z + c.cy);
  if (!(fc >= 0.0f && fc < (float)W && fr >= 0.0f && fr < (float)H)) return false;
  int col = (int)fc, row = (int)fr;
  pix = (size_t)row * W + col;
  return true;
}

// project one camera-frame point and min-merge it into the z-buffer (sd:225-258)
__device__ inline void splat(uint32_t* zbuf, const Cam& c, float x, float y, float z, int H, int W) {
  size_t pix;
  if (splat_pixel(c, x, y, z, H, W, pix)) atomicMin(zbuf + pix, __float_as_uint(z));
}

}  // namespace prg
