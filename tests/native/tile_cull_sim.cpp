// The alpha-cut tile box (3dgs.cpp_amd/csrc/gs_tile_cull.h) as the CPU tests call it: the header alone, compiled with g++.
#include <cstdint>

#include "gs_tile_cull.h"

extern "C" {
// conic [n][3] (a, b, c), uv [n][2], cut [n], ref [n][4] (x0 y0 x1 y1, upper bounds exclusive) -> tight [n][4]
void tc_boxes(const float* conic, const float* uv, const float* cut, const int32_t* ref, uint64_t n, int32_t* tight) {
    for (uint64_t i = 0; i < n; ++i) {
        const gs::TileBox r{ref[4 * i], ref[4 * i + 1], ref[4 * i + 2], ref[4 * i + 3]};
        const gs::TileBox t = gs::tile_cull_box(conic[3 * i], conic[3 * i + 1], conic[3 * i + 2], uv[2 * i], uv[2 * i + 1], cut[i], r);
        tight[4 * i] = t.x0;
        tight[4 * i + 1] = t.y0;
        tight[4 * i + 2] = t.x1;
        tight[4 * i + 3] = t.y1;
    }
}
}
