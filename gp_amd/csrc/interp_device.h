// Device helpers shared by the Cholesky-factor interpolation kernels (se_kernels.hip, interp_kernels.hip).
// Included inside each translation unit's anonymous namespace.
#pragma once

// cubic Hermite blend of one element (covariance.cpp:49-96, cubic_interpolated_gp.hpp:62-66) in the reference's operation order
__device__ __forceinline__ double hermite(double y1, double y2, double k1, double k2, double dx, double t)
{
    const double a = k1 * dx - (y2 - y1);
    const double b = -k2 * dx + (y2 - y1);
    return (1 - t) * y1 + t * y2 + t * (1 - t) * (a * (1 - t) + b * t);
}
