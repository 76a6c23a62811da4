// Channel weights of the gradient CAM family (dlib/cams/gradcam.py: GradCAM, GradCAMpp,
// XGradCAM, LayerCAM) on a WGAP classifier, shared by the plain (cam.hip) and the S3 / S2 /
// S1 (s3.hip) entries of tcam_grad_cam.
//
// The hook is the ReLU in front of AdaptiveAvgPool2d(1) + Linear, so the gradient of
// scores[:, c].sum() at the hook is g[k] = fp32(W[c, k] / hw) at every position: no encoder
// backward.  With that g (gradcam.py:122-129, 179-198, 384-394, 436-443):
//   GradCam    w_k = mean_p g            = g_k
//   GradCAMpp  w_k = sum_p g^2 relu(g)   = hw g_k^2 relu(g_k)   (the alpha division at :194
//                                                               acts on a copy)
//   XGradCAM   w_k = sum_p (g_k A_k[p]) / sum_p A_k[p]          (NaN where the sum is 0: the
//                                                               map's nansum drops the channel)
//              computed as (g_k S_k) / S_k with S_k = sum_p A_k[p]: g is the same at every
//              position, so this is the reference's ratio with two roundings instead of one
//              per position, whatever the cancellation in S_k; 0 / 0, a NaN and an infinite
//              sum give NaN as there.
//   LayerCAM   w_k[p] = relu(g_k)
// exps (optional): A is stored times 2^exps[k] (the f16x3 features); w_k is computed from the
// true W — for XGradCAM from the stored A, the power of two cancels in the ratio — and then
// multiplied by 2^-exps[k], which is exact.
//
// Workspace (floats): w[B][C], then XGradCAM's partial sums part[B][nchunks][C] of A over
// chunks of positions, written chunk by chunk and added in chunk order here: no atomics.
#pragma once
#include "common.h"

namespace {

constexpr int GRAD_CHUNK = 32;   // positions per partial sum of the S3 / S2 / S1 pass

__global__ void grad_weights_kernel(const float* __restrict__ fcw, const int32_t* __restrict__ cls,
                                    const int32_t* __restrict__ exps,
                                    const float* __restrict__ part, float* __restrict__ wout,
                                    int C, int hw, int nchunks, int method, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / C), k = (int)(i - (long)b * C);
    const float g = fcw[(long)cls[b] * C + k] / (float)hw;
    float wk;
    if (method == TCAM_GRAD_GRADCAM) {
        wk = g;
    } else if (method == TCAM_GRAD_GRADCAMPP) {
        wk = (float)hw * ((g * g) * relu_nan(g));
    } else if (method == TCAM_GRAD_XGRADCAM) {
        float S = 0.f;
        for (int ch = 0; ch < nchunks; ++ch) S += part[((long)b * nchunks + ch) * C + k];
        wk = (g * S) / S;
    } else {
        wk = relu_nan(g);
    }
    if (exps) wk = ldexpf(wk, -exps[k]);
    wout[i] = wk;
}

static inline bool grad_method_ok(int method) {
    return method == TCAM_GRAD_GRADCAM || method == TCAM_GRAD_GRADCAMPP ||
           method == TCAM_GRAD_XGRADCAM || method == TCAM_GRAD_LAYERCAM;
}

}  // namespace
