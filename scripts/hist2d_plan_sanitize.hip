// The host plan of the joint histograms (csrc/mcpc_hist2d.h: hist2d_plan) and the classification body the kernel shares with the host
// (hist2d_cell: hist_key_bits, hist_key_table, hist_search_step, hist_column) under AddressSanitizer and UndefinedBehaviorSanitizer,
// as a program of its own.  For the shapes of tests/test_gpu_hist2d.py it walks every (job, segment, chain range, slot lane, record
// lane) the plan gives a launch, exactly as the kernel's loops do, counting through bounds-checked tables, and compares the counts
// with a naive loop that classifies by float comparison.  Host code only: nothing touches a device.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Imontecarlopredictivecoding_amd/csrc scripts/hist2d_plan_sanitize.hip \
//         -o scripts/bin/hist2d_plan_sanitize
//   scripts/bin/hist2d_plan_sanitize        (exit status 0 and no report: clean)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mcpc_hist2d.h"

using namespace mcpc;

static uint32_t bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

// the class of v by float comparison: the definition in include/mcpc.h
static int naive_class(float v, const std::vector<float>& e) {
    const int nb = (int)e.size() - 1;
    if (std::isnan(v)) return nb + 2;
    if (v < e[0]) return nb;
    if (v > e[nb]) return nb + 1;
    int i = nb - 1;
    while (i > 0 && !(e[i] <= v)) --i;
    return i;
}

static uint32_t rng_state = 12345u;
static float next_value() {
    rng_state = rng_state * 1664525u + 1013904223u;
    const uint32_t r = rng_state >> 8;
    static const float special[] = {0.0f, -0.0f, 1e-40f, -1e-42f, 1.0f, 2.0f, -2.0f, std::numeric_limits<float>::infinity(),
                                    -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    if (r % 16 == 0) return special[(r >> 4) % 10];
    return ((float)(r & 0xffff) / 65536.0f - 0.5f) * 5.0f;
}

static std::vector<float> edges_of(int nb, float lo, float hi, bool special) {
    if (special) return {-2.0f, -1.0f, 0.0f, 1e-40f, 1.0f, 2.0f};
    std::vector<float> e(nb + 1);
    for (int i = 0; i <= nb; ++i) e[i] = lo + (hi - lo) * (float)i / (float)nb;
    return e;
}

static int run_case(int B, int wx, int wy, int n_pairs, int nx, int ny, int pool, int n, bool special) {
    const std::vector<float> ex = edges_of(nx, -2.1f, 1.9f, special), ey = edges_of(ny, -1.7f, 2.3f, special);
    nx = (int)ex.size() - 1;
    ny = (int)ey.size() - 1;
    std::vector<float> rx((size_t)n * B * wx), ry((size_t)n * B * wy);
    for (float& v : rx) v = next_value();
    for (float& v : ry) v = next_value();
    std::vector<int> col(2 * (size_t)n_pairs);
    for (int i = 0; i < n_pairs; ++i) { col[2 * i] = (i * 7) % wx; col[2 * i + 1] = (i * 3 + 1) % wy; }

    const Hist2dPlan p = hist2d_plan(B, wx, wy, n_pairs, nx, ny, pool, n);
    const int64_t cells = (int64_t)(nx + 3) * (ny + 3);
    if (p.cells != cells || p.G < 1 || p.GL < p.G || (p.GL & (p.GL - 1)) || p.GL > kHist2dThreads || p.G * cells > kHist2dCounterWords ||
        p.groups * p.G < p.slots || (int64_t)p.seg * p.segments < n || (int64_t)p.chains_per * p.chain_ranges < (pool ? B : 1) ||
        (int64_t)p.seg * p.chains_per > INT32_MAX || p.lds_bytes > (size_t)kHistLdsWords * 4) {
        printf("plan out of its bounds: B=%d pairs=%d %dx%d pool=%d n=%d\n", B, n_pairs, nx, ny, pool, n);
        return 1;
    }
    uint32_t kx[kHist2dTable], ky[kHist2dTable], hi_x, hi_y;
    const int32_t top_x = hist_key_table(ex.data(), nx, kx, kHist2dTable, &hi_x);
    const int32_t top_y = hist_key_table(ey.data(), ny, ky, kHist2dTable, &hi_y);

    std::vector<int64_t> got((size_t)p.slots * cells, 0), want((size_t)p.slots * cells, 0);
    const int RL = kHist2dThreads / p.GL;
    for (int64_t job = 0; job < p.groups; ++job)
        for (int y = 0; y < p.segments; ++y)
            for (int z = 0; z < p.chain_ranges; ++z) {
                std::vector<uint32_t> cnt((size_t)p.G * cells, 0u);                        // the workgroup's LDS counters
                const int64_t s0 = job * p.G;
                const int g = (int)((p.slots - s0) < p.G ? (p.slots - s0) : p.G);
                const int64_t k0 = (int64_t)y * p.seg, k1 = (n - k0) < p.seg ? n : k0 + p.seg;
                for (int sl = 0; sl < g; ++sl)
                    for (int rl = 0; rl < RL; ++rl) {
                        const int64_t s = s0 + sl;
                        const int pair = (int)(pool ? s : s % n_pairs);
                        int64_t c_lo = pool ? (int64_t)z * p.chains_per : s / n_pairs, c_hi = pool ? c_lo + p.chains_per : c_lo + 1;
                        if (c_hi > B) c_hi = B;
                        for (int64_t c = c_lo; c < c_hi; ++c)
                            for (int64_t k = k0 + rl; k < k1; k += RL) {
                                const float fx = rx.at((size_t)((k * B + c) * wx + col[2 * pair]));
                                const float fy = ry.at((size_t)((k * B + c) * wy + col[2 * pair + 1]));
                                const int32_t cell = hist2d_cell(kx, ky, bits_of(fx), bits_of(fy), nx, ny, top_x, top_y, kx[0], hi_x, ky[0], hi_y);
                                cnt.at((size_t)(sl * cells + cell)) += 1u;
                            }
                    }
                for (int64_t i = 0; i < g * cells; ++i) got.at((size_t)(s0 * cells + i)) += cnt[(size_t)i];
            }
    for (int64_t c = 0; c < B; ++c)
        for (int pr = 0; pr < n_pairs; ++pr)
            for (int64_t k = 0; k < n; ++k) {
                const int cx = naive_class(rx[(size_t)((k * B + c) * wx + col[2 * pr])], ex);
                const int cy = naive_class(ry[(size_t)((k * B + c) * wy + col[2 * pr + 1])], ey);
                const int64_t slot = pool ? pr : c * n_pairs + pr;
                want[(size_t)(slot * cells + (int64_t)cx * (ny + 3) + cy)] += 1;
            }
    if (got != want) {
        printf("counts differ: B=%d pairs=%d %dx%d pool=%d n=%d\n", B, n_pairs, nx, ny, pool, n);
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0, cases = 0;
    for (int pool = 0; pool < 2; ++pool) {
        for (int B : {1, 3, 5})
            for (int n : {1, 7, 9, 33}) { bad += run_case(B, 5, 7, 5, 3, 5, pool, n, false); ++cases; }
        for (int n_pairs : {1, 3, MCPC_HIST2D_MAX_PAIRS}) { bad += run_case(3, 5, 7, n_pairs, 3, 5, pool, 9, false); ++cases; }
        bad += run_case(3, 5, 7, 3, 1, 1, pool, 33, false);
        bad += run_case(3, 5, 7, 3, 128, 90, pool, 33, false);
        bad += run_case(2, 2, 2, 2, 5, 5, pool, 289, true);                             // the edges at 0.0 and at a denormal
        bad += run_case(2, 5, 7, 2, 3, 5, pool, 4099, false);                           // several segments
        bad += run_case(128, 2, 2, 1, 40, 40, pool, 64, false);                         // a class-plane panel: 8 grids per workgroup
        cases += 5;
    }
    // shapes too large to walk: the plan alone
    for (int pool = 0; pool < 2; ++pool) {
        const Hist2dPlan a = hist2d_plan(1024, 128, 128, 64, 50, 50, pool, 9000), b = hist2d_plan(1 << 30, 1, 1, 1, 1, 1, pool, INT32_MAX);
        if ((int64_t)a.seg * a.segments < 9000 || (int64_t)b.seg * b.chains_per > INT32_MAX || (int64_t)b.seg * b.segments < INT32_MAX) ++bad;
    }
    printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
