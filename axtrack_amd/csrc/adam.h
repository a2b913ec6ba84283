// torch.optim.Adam's update of one element for train_conv.hip: the arithmetic of train.hip's AdamArgs / adam1, operation for
// operation, so that the conv block and the linear head take the same step (train.hip keeps its own copy unchanged).
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

// every factor is formed in f64 on the host and rounded once (1.f - 0.999f is off by 5e-5 of itself)
struct AdamArgs { float beta1, beta2, one_minus_beta1, one_minus_beta2, step_size, bc2_sqrt, eps, weight_decay; };

// step: the optimiser's step count after its increment
static inline AdamArgs adam_args(double lr, double beta1, double beta2, double eps, double weight_decay, long step)
{
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamArgs a;
    a.beta1 = (float)beta1;
    a.beta2 = (float)beta2;
    a.one_minus_beta1 = (float)(1.0 - beta1);
    a.one_minus_beta2 = (float)(1.0 - beta2);
    a.step_size = (float)(lr / bc1);
    a.bc2_sqrt = (float)std::sqrt(bc2);
    a.eps = (float)eps;
    a.weight_decay = (float)weight_decay;
    return a;
}

__device__ inline void adam1(float g, float &w, float &m, float &v, const AdamArgs &a)
{
    g = fmaf(a.weight_decay, w, g);
    m = a.beta1 * m + a.one_minus_beta1 * g;
    v = a.beta2 * v + a.one_minus_beta2 * (g * g);
    w = w - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}
