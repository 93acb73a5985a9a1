// Stand-alone host check of dense_scatter (csrc/yawhip_dense.hip) for AddressSanitizer / UBSan builds: feeds the epilogue
// synthetic result blocks on every route and compares with a direct evaluation of the same products. No GPU call is made.
// The unit is included as text (dense_scatter is private to it); the other units come as the objects of the regular build:
//   hipcc --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Iyet_another_wizz_amd/csrc -x hip tools/dense_scatter_check.cpp \
//         -x none <yet_another_wizz_amd/build/*.hip.o except yawhip_dense.hip.o> -o dense_scatter_check && ./dense_scatter_check
// A program of its own, run on the CPU: never loaded into python, never part of the test suite.
#include "yawhip_dense.hip"

#include <cstdio>
#include <random>

int main() {
    std::mt19937_64 rng(7);
    int bad = 0, cases = 0;
    for (int P : {1, 3, 8})
        for (int n_bins : {1, 2, 5})
            for (int n_scales : {1, 2})
                for (int route = 0; route < 3; ++route)      // 0: counts, 1: weighted sums, 2: comb
                    for (int halve = 0; halve < 2; ++halve)
                        for (int with_factors = 0; with_factors < 2; ++with_factors) {
                            if (route == 2 && with_factors) continue;  // (comb carries its factors already)
                            yawhip_catalog cat;
                            cat.n_patches = P;
                            std::vector<int32_t> jobs;
                            for (int p = 0; p < P; ++p)
                                for (int q = 0; q < P; ++q)
                                    if ((p * 7 + q) % 5 != 1) { jobs.push_back(p); jobs.push_back(q); }
                            const int32_t n_jobs = (int32_t)(jobs.size() / 2);
                            std::vector<int32_t> slices((size_t)2 * n_bins * n_scales);
                            for (int k = 0; k < n_bins; ++k)
                                for (int s = 0; s < n_scales; ++s) {  // the second scale of odd bins is empty
                                    slices[2 * ((size_t)k * n_scales + s)] = 0;
                                    slices[2 * ((size_t)k * n_scales + s) + 1] = (s == 1 && (k & 1)) ? 0 : 1;
                                }
                            std::vector<double> factors((size_t)n_bins), hs((size_t)n_jobs * n_bins), comb((size_t)n_jobs * n_bins * n_scales);
                            std::vector<int64_t> hc((size_t)n_jobs * n_bins);
                            for (auto &f : factors) f = 0.5 + (double)(rng() % 1000) / 333.0;
                            for (auto &v : hs) v = (double)(rng() % 100000) / 7.0;
                            for (auto &v : hc) v = (int64_t)(rng() % 100000);
                            for (auto &v : comb) v = (double)(rng() % 100000) / 3.0;
                            std::vector<double> dense((size_t)n_scales * n_bins * P * P, 0.0), want(dense.size(), 0.0);
                            yawhip_dense_request r{&cat, &cat, n_jobs, halve, jobs.data(), dense.data(), nullptr};
                            dense_scatter(r, n_bins, n_scales, slices.data(), with_factors ? factors.data() : nullptr,
                                          route == 2 ? comb.data() : nullptr, route == 1, hc.data(), hs.data());
                            for (int32_t j = 0; j < n_jobs; ++j) {
                                const double half = (halve && jobs[2 * j] == jobs[2 * j + 1]) ? 0.5 : 1.0;
                                for (int k = 0; k < n_bins; ++k)
                                    for (int s = 0; s < n_scales; ++s) {
                                        if (!(slices[2 * ((size_t)k * n_scales + s) + 1] > slices[2 * ((size_t)k * n_scales + s)])) continue;
                                        double v = route == 2 ? comb[((size_t)j * n_bins + k) * n_scales + s]
                                                              : (route == 1 ? hs[(size_t)j * n_bins + k] : (double)hc[(size_t)j * n_bins + k]);
                                        if (route != 2 && with_factors) v = v * factors[(size_t)k];
                                        want[(((size_t)s * n_bins + k) * P + jobs[2 * j]) * P + jobs[2 * j + 1]] = v * half;
                                    }
                            }
                            ++cases;
                            if (memcmp(dense.data(), want.data(), dense.size() * sizeof(double)) != 0) {
                                ++bad;
                                fprintf(stderr, "differs: P %d bins %d scales %d route %d halve %d factors %d\n", P, n_bins, n_scales, route, halve, with_factors);
                            }
                        }
    printf("dense_scatter: %d cases, %d differ\n", cases, bad);
    return bad ? 1 : 0;
}
