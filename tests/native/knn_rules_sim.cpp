// The WHOLE search of gs_knn_dist2 (csrc/gs_knn.hip) on the CPU, over the very text the kernels compile (gs_knn_rules.h): bounding
// box, Morton codes, a stable sort, the boxes of GS_KNN_BOX sorted points, and per query box the own box first and then the walk
// over the others with the workgroup-level rejection -- one position at a time, which is what the kernel's turn-wise walk decides
// too (its second test sees the radius a one-by-one walk would).  tests/test_knn_api.py builds this with g++ and holds its
// output to the brute force (tests/knn_reference.py); tests/test_gpu_knn.py holds the device's box_visits to it.
//
//   knn_rules_sim search POINTS n k [mutation]     POINTS: n x 3 binary32, raw.  Prints "n k boxes", then per point the bit
//                                                  patterns of mean_dist2 and dist2[0..k), then per box its visits (decimal).
//       mutation 1: reject on the values kept so far, before a lane holds k of them
//       mutation 2: the box bound from the boxes' centres
//       mutation 3: pass a candidate over by POSITION (equal coordinates) instead of by index
//   knn_rules_sim bounds CASES count               CASES: count x 12 binary32 (loA, hiA, loB, hiB).  Prints per case the bit
//                                                  patterns of box_box_bound(A, B) and of point_box_bound(loA, B).
// Nothing here touches a GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "../../include/gs3d_hip.h"
#include "gs_knn_rules.h"

namespace {

constexpr uint32_t kBox = GS_KNN_BOX;
const float kInf = std::numeric_limits<float>::infinity();

uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

struct Sorted {
    float x, y, z;
    uint32_t id;
};

std::vector<float> read_floats(const char* path, size_t count) {
    std::vector<float> v(count);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), 4, count, f) != count) {
        std::fprintf(stderr, "cannot read %zu floats from %s\n", count, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

template <int K>
void search(const std::vector<float>& pts, uint32_t n, int mutation) {
    // bounding box, codes, order
    float lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float v = pts[3 * i + a];
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
        }
    std::vector<uint32_t> code(n), order(n);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t c[3];
        for (int a = 0; a < 3; ++a) c[a] = gs_knn::morton_cell(pts[3 * i + a], lo[a], hi[a] - lo[a]);
        code[i] = gs_knn::morton_code(c[0], c[1], c[2]);
    }
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return code[a] < code[b]; });
    std::vector<Sorted> sorted(n);
    for (uint32_t j = 0; j < n; ++j) sorted[j] = {pts[3 * order[j]], pts[3 * order[j] + 1], pts[3 * order[j] + 2], order[j]};
    const uint32_t nb = (n + kBox - 1) / kBox;
    std::vector<gs_knn::Box> boxes(nb);
    for (uint32_t b = 0; b < nb; ++b) {
        gs_knn::Box& bx = boxes[b];
        for (int a = 0; a < 3; ++a) bx.lo[a] = kInf, bx.hi[a] = -kInf;
        for (uint32_t j = b * kBox; j < std::min(n, (b + 1) * kBox); ++j) {
            const float v[3] = {sorted[j].x, sorted[j].y, sorted[j].z};
            for (int a = 0; a < 3; ++a) {
                if (v[a] < bx.lo[a]) bx.lo[a] = v[a];
                if (v[a] > bx.hi[a]) bx.hi[a] = v[a];
            }
        }
    }

    const int ke = (int)std::min<uint32_t>(K, n - 1);
    std::vector<float> mean(n), dist2((size_t)n * K);
    std::vector<uint32_t> visits(nb);
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t q0 = b * kBox, lanes = std::min(kBox, n - q0);
        std::vector<float> best((size_t)lanes * K, kInf);
        auto row = [&](uint32_t t) -> float(&)[K] { return *reinterpret_cast<float(*)[K]>(&best[(size_t)t * K]); };
        float R = kInf;
        uint32_t staged = 0;
        auto examine = [&](uint32_t c) {
            const uint32_t base = c * kBox, cnt = std::min(kBox, n - base);
            for (uint32_t t = 0; t < lanes; ++t) {
                const Sorted& q = sorted[q0 + t];
                float(&mine)[K] = row(t);
                if (gs_knn::point_box_bound(q.x, q.y, q.z, boxes[c]) > mine[K - 1]) continue;
                for (uint32_t e = 0; e < cnt; ++e) {
                    const Sorted& p = sorted[base + e];
                    const bool self = mutation == 3 ? (p.x == q.x && p.y == q.y && p.z == q.z) : p.id == q.id;
                    if (!self) gs_knn::insert<K>(mine, gs_knn::dist2(q.x, q.y, q.z, p.x, p.y, p.z));
                }
            }
            float r = 0.0f;
            for (uint32_t t = 0; t < lanes; ++t) {
                float v = row(t)[K - 1];
                if (mutation == 1) {  // the largest value kept so far, nothing kept: 0
                    v = 0.0f;
                    for (int i = 0; i < K; ++i)
                        if (row(t)[i] < kInf) v = row(t)[i];
                }
                if (v > r) r = v;
            }
            R = r;
            ++staged;
        };
        examine(b);
        const uint32_t positions = gs_knn::walk_positions(b, nb);
        for (uint32_t p = 0; p < positions; ++p) {
            uint32_t c;
            if (!gs_knn::walk_box(b, nb, p, &c)) continue;
            float lb = gs_knn::box_box_bound(boxes[b], boxes[c]);
            if (mutation == 2) {
                const gs_knn::Box &A = boxes[b], &B = boxes[c];
                lb = gs_knn::dist2((A.lo[0] + A.hi[0]) * 0.5f, (A.lo[1] + A.hi[1]) * 0.5f, (A.lo[2] + A.hi[2]) * 0.5f,
                                   (B.lo[0] + B.hi[0]) * 0.5f, (B.lo[1] + B.hi[1]) * 0.5f, (B.lo[2] + B.hi[2]) * 0.5f);
            }
            if (lb > R) continue;
            examine(c);
        }
        visits[b] = staged;
        for (uint32_t t = 0; t < lanes; ++t) {
            const uint32_t id = sorted[q0 + t].id;
            mean[id] = gs_knn::mean_of<K>(row(t), ke);
            for (int i = 0; i < K; ++i) dist2[(size_t)id * K + i] = row(t)[i];
        }
    }
    std::printf("%u %d %u\n", n, K, nb);
    for (uint32_t i = 0; i < n; ++i) {
        std::printf("%u", bits(mean[i]));
        for (int e = 0; e < K; ++e) std::printf(" %u", bits(dist2[(size_t)i * K + e]));
        std::printf("\n");
    }
    for (uint32_t b = 0; b < nb; ++b) std::printf("%u\n", visits[b]);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 4 && std::strcmp(argv[1], "bounds") == 0) {
        const size_t count = std::strtoull(argv[3], nullptr, 10);
        const std::vector<float> v = read_floats(argv[2], 12 * count);
        for (size_t i = 0; i < count; ++i) {
            gs_knn::Box A, B;
            for (int a = 0; a < 3; ++a) A.lo[a] = v[12 * i + a], A.hi[a] = v[12 * i + 3 + a], B.lo[a] = v[12 * i + 6 + a], B.hi[a] = v[12 * i + 9 + a];
            std::printf("%u %u\n", bits(gs_knn::box_box_bound(A, B)), bits(gs_knn::point_box_bound(A.lo[0], A.lo[1], A.lo[2], B)));
        }
        return 0;
    }
    if (argc >= 5 && std::strcmp(argv[1], "search") == 0) {
        const uint32_t n = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        const int k = std::atoi(argv[4]), mutation = argc >= 6 ? std::atoi(argv[5]) : 0;
        if (n == 0 || k < 1 || k > GS_KNN_MAX_K) return 2;
        const std::vector<float> pts = read_floats(argv[2], 3 * (size_t)n);
        switch (k) {
            case 1: search<1>(pts, n, mutation); break;
            case 2: search<2>(pts, n, mutation); break;
            case 3: search<3>(pts, n, mutation); break;
            case 4: search<4>(pts, n, mutation); break;
            case 5: search<5>(pts, n, mutation); break;
            case 6: search<6>(pts, n, mutation); break;
            case 7: search<7>(pts, n, mutation); break;
            default: search<8>(pts, n, mutation); break;
        }
        return 0;
    }
    std::fprintf(stderr, "usage: knn_rules_sim search POINTS n k [mutation] | bounds CASES count\n");
    return 2;
}
