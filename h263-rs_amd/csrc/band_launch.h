// band_launch.h -- the launch shape that the banded output kernels share (the resizes, the filters, the plane kernels, the ROI
// tensors): one wave per workgroup, blockIdx.x = band of output rows in XCD order, blockIdx.y = picture or region, blockIdx.z =
// column segment.  Plain C++: the kernels, their launchers (output_kernels.hip) and the CPU checkers (tests/sim_*) all read it from here.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BAND_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BAND_HD inline
#endif

namespace h263mi {

// a grid as plain numbers (no HIP type: the checkers walk it too)
struct LaunchDims {
    uint32_t x, y, z;
};

// The band of workgroup block_x.  Workgroups are dealt round-robin over the 8 XCDs, so XCD k (block_x & 7) takes the contiguous
// bands [k * chunk, (k + 1) * chunk): the source rows that two neighbouring bands share are fetched into one L2.  A band at or
// beyond the number of bands does not exist (the last XCD's run may be short): its wave leaves.
BAND_HD uint32_t xcd_band(uint32_t block_x, uint32_t chunk) { return (block_x & 7u) * chunk + (block_x >> 3); }

// `rows` output rows in bands of rows_per_band: bands = ceil(rows / rows_per_band), chunk = ceil(bands / 8) of them per XCD; the
// grid over them with `items` pictures or regions and `segs` column segments
inline LaunchDims band_grid(uint32_t rows, uint32_t rows_per_band, uint32_t items, uint32_t segs, uint32_t &bands, uint32_t &chunk)
{
    bands = (rows + rows_per_band - 1) / rows_per_band;
    chunk = (bands + 7) / 8;
    return LaunchDims{chunk * 8, items, segs};
}

}  // namespace h263mi
