// Standalone per-kernel timer for the 8-bit radix sort as production runs
// it: the dense key->slot kernel writes the slots and the pass-0 histogram
// (untimed), then the sort runs with a hipEvent between every pair of
// launches.  Scatter variants are alternated inside one process
// (old, new, old, new, ...) after two warm-up rounds, so clock and
// box-to-box spread cancel.
//
//   sort_stage_ab [n] [bits] [base_shift] [variant] [rounds] [iters]
//     base_shift  0 or 16 (16 = value-in-key layout, bf16 in the low half)
//     variant     ab (alternate lds, occ; default), lds, occ
//     rounds      timed rounds per variant (default 3, at least 1)
//     iters       sorts per round (default 20)
//
// Build: hipcc --offload-arch=gfx950 -O3 csrc/tests/sort_stage_ab.cpp
//        csrc/hip/sortwin.hip -o sort_stage_ab
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../hip/wfa_kernels.h"

#define CHK(x)                                                    \
    do {                                                          \
        hipError_t e = (x);                                       \
        if (e != hipSuccess) {                                    \
            fprintf(stderr, "HIP error %d (%s) at line %d\n", e,  \
                    hipGetErrorString(e), __LINE__);              \
            exit(1);                                              \
        }                                                         \
    } while (0)

static const int MAX_EV = 40;

struct Probe {
    hipEvent_t ev[MAX_EV];
    std::string name[MAX_EV];  // name[i] = launch that ended at ev[i]
    int n = 0;
};

static void on_launch(void* ctx, const char* kernel, int pass) {
    Probe* p = (Probe*)ctx;
    if (p->n >= MAX_EV) return;
    p->name[p->n] = "p" + std::to_string(pass) + " " + kernel;
    CHK(hipEventRecord(p->ev[p->n], 0));
    ++p->n;
}

struct Acc {
    std::vector<std::string> names;
    std::vector<double> us;
    double total = 0;
    void add(const std::string& nm, double v) {
        for (size_t i = 0; i < names.size(); ++i)
            if (names[i] == nm) {
                us[i] += v;
                return;
            }
        names.push_back(nm);
        us.push_back(v);
    }
};

int main(int argc, char** argv) {
    int64_t n = argc > 1 ? atoll(argv[1]) : 16777216;
    int bits = argc > 2 ? atoi(argv[2]) : 15;
    int base_shift = argc > 3 ? atoi(argv[3]) : 16;
    const char* vsel = argc > 4 ? argv[4] : "ab";
    int rounds = argc > 5 ? atoi(argv[5]) : 3;
    int iters = argc > 6 ? atoi(argv[6]) : 20;
    if (n < 1 || bits < 5 || (base_shift != 0 && base_shift != 16) ||
        base_shift + bits > 32 || rounds < 1 || iters < 1) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    std::vector<int> variants;  // wfa_sort_pairs2_ex: 1 = occ, 2 = lds
    if (!strcmp(vsel, "ab")) variants = {2, 1};
    else if (!strcmp(vsel, "lds")) variants = {2};
    else if (!strcmp(vsel, "occ")) variants = {1};
    else {
        fprintf(stderr, "variant must be ab, lds or occ\n");
        return 2;
    }
    const char* vname[3] = {"", "occ", "lds"};

    uint64_t* key;
    uint16_t* val;
    uint32_t *ka, *va, *kt, *vt, *hist, *nslots;
    CHK(hipMalloc(&key, 8 * n));
    CHK(hipMalloc(&val, 2 * n));
    CHK(hipMalloc(&ka, 4 * n));
    CHK(hipMalloc(&va, 4 * n));
    CHK(hipMalloc(&kt, 4 * n));
    CHK(hipMalloc(&vt, 4 * n));
    CHK(hipMalloc(&hist, 4 * wfa_sort_hist_u32(n)));
    CHK(hipMalloc(&nslots, 64));
    CHK(hipMemset(nslots, 0, 64));
    {
        // the flagship uses half of the key space it reserves (8192 dense
        // keys under max_keys 16384)
        std::vector<uint64_t> hk(n);
        std::vector<uint16_t> hv(n);
        const uint64_t used = (uint64_t)1 << (bits - 1);
        uint64_t x = 12345;
        for (int64_t i = 0; i < n; ++i) {
            x = x * 6364136223846793005ULL + 1442695040888963407ULL;
            hk[i] = (x >> 33) % used;
            hv[i] = (uint16_t)(x >> 17);
        }
        CHK(hipMemcpy(key, hk.data(), 8 * n, hipMemcpyHostToDevice));
        CHK(hipMemcpy(val, hv.data(), 2 * n, hipMemcpyHostToDevice));
    }
    Probe pr;
    for (int i = 0; i < MAX_EV; ++i) CHK(hipEventCreate(&pr.ev[i]));
    hipEvent_t e0;
    CHK(hipEventCreate(&e0));

    std::vector<uint32_t> ref_k, ref_v, got_k(n), got_v(n);
    std::vector<Acc> acc(3);
    std::vector<std::vector<double>> round_total(3);
    const int warm = 2;
    for (int r = -warm; r < rounds; ++r) {
        for (int v : variants) {
            Acc racc;
            for (int it = 0; it < iters; ++it) {
                wfa_key_dense_h(nullptr, key, n, (int64_t)1 << bits, ka, nslots,
                                nslots + 1, base_shift ? val : nullptr, hist,
                                base_shift);
                pr.n = 0;
                uint32_t *ok, *ov;
                CHK(hipEventRecord(e0, 0));
                wfa_sort_pairs2_ex(nullptr, ka, va, kt, vt, nullptr, nullptr, hist,
                                   n, bits, &ok, &ov, nullptr, /*iota*/ 1,
                                   base_shift, /*skip_hist0*/ 1, v, on_launch, &pr);
                CHK(hipDeviceSynchronize());
                hipEvent_t prev = e0;
                for (int i = 0; i < pr.n; ++i) {
                    float ms;
                    CHK(hipEventElapsedTime(&ms, prev, pr.ev[i]));
                    racc.add(pr.name[i], ms * 1000.0);
                    prev = pr.ev[i];
                }
                float ms;
                CHK(hipEventElapsedTime(&ms, e0, pr.ev[pr.n - 1]));
                racc.total += ms * 1000.0;
                if (r == -warm && it == 0) {
                    // outputs of every variant must be identical
                    CHK(hipMemcpy(got_k.data(), ok, 4 * n, hipMemcpyDeviceToHost));
                    CHK(hipMemcpy(got_v.data(), ov, 4 * n, hipMemcpyDeviceToHost));
                    if (ref_k.empty()) {
                        ref_k = got_k;
                        ref_v = got_v;
                    } else if (ref_k != got_k || ref_v != got_v) {
                        fprintf(stderr, "variant %s: outputs differ from %s\n",
                                vname[v], vname[variants[0]]);
                        return 1;
                    }
                }
            }
            if (r < 0) continue;
            printf("round %d %-3s whole sort %8.1f us\n", r, vname[v],
                   racc.total / iters);
            round_total[v].push_back(racc.total / iters);
            for (size_t i = 0; i < racc.names.size(); ++i)
                acc[v].add(racc.names[i], racc.us[i] / iters);
            acc[v].total += racc.total / iters;
        }
    }
    printf("n=%lld bits=%d base_shift=%d rounds=%d iters=%d (mean us)\n",
           (long long)n, bits, base_shift, rounds, iters);
    for (int v : variants) {
        const Acc& a = acc[v];
        int passes = (bits + 7) / 8;
        std::vector<double> per_pass(passes, 0.0);
        for (size_t i = 0; i < a.names.size(); ++i) {
            printf("  %-3s %-12s %8.1f\n", vname[v], a.names[i].c_str(),
                   a.us[i] / rounds);
            per_pass[atoi(a.names[i].c_str() + 1)] += a.us[i] / rounds;
        }
        for (int p = 0; p < passes; ++p)
            printf("  %-3s pass %d       %8.1f\n", vname[v], p, per_pass[p]);
        double lo = 1e30, hi = 0;
        for (double t : round_total[v]) {
            lo = t < lo ? t : lo;
            hi = t > hi ? t : hi;
        }
        printf("  %-3s whole sort   %8.1f  (rounds min %.1f max %.1f)\n", vname[v],
               a.total / rounds, lo, hi);
    }
    if (variants.size() == 2) printf("outputs identical: yes\n");
    return 0;
}
