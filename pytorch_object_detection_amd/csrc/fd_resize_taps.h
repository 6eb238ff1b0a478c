// fd_resize_taps.h — the per-axis tap arithmetic of the device resize, shared by fd_resize.hip and
// fd_augment.hip so that there is one definition.  Both files compile with -ffp-contract=off: plain fp32, one rounding per
// operation; tests/resize_ref.py restates it in numpy bit for bit.
#pragma once
#include "fd_common.h"

#define FD_RESIZE_MAX_SIDE 65536      // fp32 holds every index and index + 0.5 exactly far beyond this
#define FD_RESIZE_COEF_BITS 11        // blending weights in units of 1 / 2048; 255 * 2^22 < 2^31

// Source taps and weights of destination index d on one axis (source length S >= 1, destination length D >= 1):
//   x = (d + 0.5) * (S / D) - 0.5;  i0 = floor(x), f = x - i0, both clamped to [0, S - 1];  c1 = round(f * 2048), c0 = 2048 - c1.
// i0 and i1 are inside [0, S - 1] for EVERY d (also d >= D), so no caller can be led outside the image.
__device__ __forceinline__ void resize_axis(int d, int S, int D, int& i0, int& i1, unsigned& c0, unsigned& c1) {
    const float scale = (float)S / (float)D;
    const float x = ((float)d + 0.5f) * scale - 0.5f;
    float fl = floorf(x);
    float f = x - fl;
    if (fl < 0.f) { fl = 0.f; f = 0.f; }
    if (fl >= (float)(S - 1)) { fl = (float)(S - 1); f = 0.f; }
    i0 = (int)fl;
    i1 = min(i0 + 1, S - 1);
    c1 = (unsigned)(int)floorf(f * 2048.0f + 0.5f);
    c0 = 2048u - c1;
}
