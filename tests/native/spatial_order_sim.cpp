// gs::host::spatial_order (gs_host_math.h) behind a C interface: tests/test_limit_scenes.py hands it three position planes and compares the order
// with the numpy restatement (tests/limit_scenes.py::morton_order).
// Built by that test with g++; nothing here touches a GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "gs_host_math.h"

extern "C" {

// x, y, z: n coordinates each; order: n scene ids out, in the order they are read
void so_order(const float* x, const float* y, const float* z, uint64_t n, uint32_t* order) {
    const float* const planes[3] = {x, y, z};
    const std::vector<uint32_t> o = gs::host::spatial_order(planes, n);
    if (n) std::memcpy(order, o.data(), n * sizeof(uint32_t));
}

uint64_t so_spread21(uint64_t v) { return gs::host::morton_spread21(v); }

}  // extern "C"
