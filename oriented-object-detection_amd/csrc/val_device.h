// The validator's ProbIoU (covariance form of batch_probiou, eps 1e-7, fp32) and its validity test, shared by the matching kernel (valmatch.hip)
// and the confusion matrix (valreport.hip): the same fp32 operations in the same order in both, so the two see the same IoU bits for a pair.
#pragma once
#include <hip/hip_runtime.h>

namespace obb {

__device__ __forceinline__ bool finite5(float x, float y, float w, float h, float t) {
    return isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h) && isfinite(t);
}

__device__ __forceinline__ void cov_terms(float w, float h, float t, float &A, float &B, float &C) {  // _get_covariance_matrix
    const float a = w * w / 12.0f, b = h * h / 12.0f, c = cosf(t), s = sinf(t);
    A = a * c * c + b * s * s; B = a * s * s + b * c * c; C = (a - b) * c * s;
}

// batch_probiou for one pair; d1, d2 = clamp(A B - C^2, 0) of the two boxes
__device__ __forceinline__ float probiou_cov(float x1, float y1, float A1, float B1, float C1, float d1, float x2, float y2, float A2, float B2, float C2, float d2) {
    const float eps = 1e-7f;
    const float A = A1 + A2, B = B1 + B2, C = C1 + C2;
    const float den = A * B - C * C + eps;
    const float t1 = ((A * (y1 - y2) * (y1 - y2) + B * (x1 - x2) * (x1 - x2)) / den) * 0.25f;
    const float t2 = ((C * (x2 - x1) * (y1 - y2)) / den) * 0.5f;
    const float t3 = logf((A * B - C * C) / (4.0f * sqrtf(d1 * d2) + eps) + eps) * 0.5f;
    const float bd = fminf(fmaxf(t1 + t2 + t3, eps), 100.0f);
    const float hd = sqrtf(1.0f - expf(-bd) + eps);
    return 1.0f - hd;
}

}  // namespace obb
