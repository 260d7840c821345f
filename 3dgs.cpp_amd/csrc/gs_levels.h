// gs_levels.h -- the tile edge and the depth-order levels: the constants that the kernels (gs_kernels.h) and the host's
// level policy (gs_depth_policy.h) both go by.  Plain C++, no device header.
#pragma once
#include <stdint.h>

namespace gs {

constexpr int kTile = 16;  // TILE_WIDTH == TILE_HEIGHT, common.glsl:1-2

// candidates per bin that k_bin_fast orders in LDS at depth-order level 0 .. 3 (8 bytes of LDS each); level 4: k_bin_slabs,
// bins of up to 65535 taken in depth slabs of <= 12288; level 5 = the global path
constexpr int kBinSortLevels = 5;
constexpr int kBinSlabLevel = 4;
constexpr uint32_t kBinSortLimit[kBinSortLevels] = {4096, 8192, 12288, 16384, 65535};

}  // namespace gs
