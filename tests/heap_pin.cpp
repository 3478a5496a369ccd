// Independent pin of the k-NN row ORDER (test infrastructure; built with g++ by tests/test_heap_pin.py).
//
// The reference's selectKNearestRoadEntities (reference src/knn.hpp:103-158) drives a vendored copy of the SGI STL
// heap (src/binary_heap.hpp).  libstdc++'s std::make_heap / std::pop_heap / std::push_heap are a third-party
// implementation of the same SGI algorithm, so running knn.hpp's loop on them gives an order that depends on
// neither the oracle's restatement of binary_heap.hpp (oracle/gd_oracle.c) nor the HIP kernel.
//
// stdin (binary): int32 K, int32 R, float radius, then R float32 keys (position.length2() of every road's
// observation, in road order).  stdout (binary): K int32 = road index per output slot, -1 for a zero-filled slot.
//
// With the argument "f64" (tests/road_reference.py) radius and keys are float64, and behind the K slots comes one
// float64: the smallest gap |a - b| / (max(a, b) + 1) between UNEQUAL keys over the comparisons the run actually
// performed (infinity when it compared none).  A float32 run of the same loop takes the same path -- and leaves the
// same order -- as long as no comparison it performs turns, i.e. as long as that gap exceeds twice the keys' error on
// the same scale (the + 1 m^2: a key's error is relative far out and absolute next to the agent).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

template <class T> struct Obs {
    T key;  // position.length2()
    int32_t road;
};

static double g_min_gap = std::numeric_limits<double>::infinity();

template <class T> static bool cmp(const Obs<T> &l, const Obs<T> &r) {  // knn.hpp:15-17
    if (sizeof(T) == 8 && l.key != r.key) {
        const double a = (double)l.key, b = (double)r.key;
        g_min_gap = std::min(g_min_gap, std::fabs(a - b) / (std::max(a, b) + 1.0));
    }
    return l.key < r.key;
}

// knn.hpp:83-97 (length() = sqrtf(length2()))
template <class T> static long radius_filter(Obs<T> *heap, long K, T radius) {
    long new_beyond = K, idx = 0;
    while (idx < new_beyond) {
        if (std::sqrt(heap[idx].key) <= radius) { ++idx; continue; }
        heap[idx] = heap[--new_beyond];
    }
    return new_beyond;
}

template <class T> static int run(bool report_gap) {
    int32_t K = 0, R = 0;
    T radius = 0;
    if (std::fread(&K, 4, 1, stdin) != 1 || std::fread(&R, 4, 1, stdin) != 1 || std::fread(&radius, sizeof(T), 1, stdin) != 1) return 2;
    if (K < 1 || R < 0) return 2;
    std::vector<T> keys(R);
    if (R && std::fread(keys.data(), sizeof(T), R, stdin) != (size_t)R) return 2;
    std::vector<Obs<T>> heap(K);
    const long first = std::min<long>(R, K);
    for (long i = 0; i < first; i++) heap[i] = Obs<T>{keys[i], (int32_t)i};  // :112-120
    long beyond;
    if (R < K) {
        beyond = radius_filter<T>(heap.data(), R, radius);  // :122-126
    } else {
        std::make_heap(heap.begin(), heap.end(), cmp<T>);  // :128
        for (long r = K; r < R; r++) {                     // :130-151
            const Obs<T> cur{keys[r], (int32_t)r};
            if (!cmp<T>(cur, heap[0])) continue;
            std::pop_heap(heap.begin(), heap.end(), cmp<T>);
            heap[K - 1] = cur;
            std::push_heap(heap.begin(), heap.end(), cmp<T>);
        }
        beyond = radius_filter<T>(heap.data(), K, radius);  // :156
    }
    std::vector<int32_t> out(K, -1);
    for (long i = 0; i < beyond; i++) out[i] = heap[i].road;
    std::fwrite(out.data(), 4, K, stdout);
    if (report_gap) std::fwrite(&g_min_gap, 8, 1, stdout);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "f64") == 0) return run<double>(true);
    return run<float>(false);
}
