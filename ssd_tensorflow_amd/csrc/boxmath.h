// Box arithmetic that host entry points and kernels of several translation units share (annotate.hip, metrics.hip).  Every
// file that includes it is built with -ffp-contract=off (Makefile): the results are the reference's float64, operation by operation.
#pragma once
#include <hip/hip_runtime.h>

namespace ssd {

// prop2abs(*abs2prop(x0, x1, y0, y1, Size(1000, 1000)), Size(W, H)) (utils.py:85-108): float64 in the reference's order of
// operations, int() truncates toward zero.  The host entry point and the kernel share it.
__host__ __device__ inline void rect_on_image(int x0, int x1, int y0, int y1, int W, int H, int* out) {
    const double width = (double)(x1 - x0), height = (double)(y1 - y0);
    const double cx = (double)x0 + width / 2, cy = (double)y0 + height / 2;
    const double pcx = cx / 1000, pcy = cy / 1000, pw = width / 1000, ph = height / 1000;
    const double width2 = pw * W / 2, height2 = ph * H / 2;
    const double ax = pcx * W, ay = pcy * H;
    out[0] = (int)(ax - width2); out[1] = (int)(ax + width2); out[2] = (int)(ay - height2); out[3] = (int)(ay + height2);
}

}  // namespace ssd
