// What the host sides of the two RANSAC solvers (sim3.hip, pnp.hip) compute alike.  Plain C++, no HIP:
// tests/ransac_host_test.cpp runs it with g++ -ffp-contract=off against tests/sim3_model.py and tests/pnp_model.py.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

namespace orbgpu {

// The iteration cap of SetRansacParameters in both references (H4, P3): ceil(log(1 - p) / log(1 - eps^3)) in double over
// the float eps, within [1, max_iterations].  n: the correspondences that take part; min_inliers: as the caller adjusted it.
inline int ransac_max_iterations(int n, int min_inliers, float eps, double probability, int max_iterations)
{
    if (n == 0)
        return 1;
    int nit = 1;
    if (min_inliers != n) {
        const double v = std::ceil(std::log(1.0 - probability) / std::log(1.0 - std::pow((double)eps, 3.0)));
        nit = (v >= -2147483648.0 && v <= 2147483647.0) ? (int)v : INT_MAX;  // NaN, +-inf: larger than max_iterations
    }
    return std::max(1, std::min(nit, max_iterations));
}

// out[i] = bit i of mask, i < n; mask holds (n + 63) / 64 words
inline void mask_to_bytes(const uint64_t *mask, int n, uint8_t *out)
{
    for (int i = 0; i < n; i++)
        out[i] = (uint8_t)((mask[i >> 6] >> (i & 63)) & 1u);
}

} // namespace orbgpu
