// The host side of mcpc_state_gradients (csrc/mcpc_state_grad.h: sg_err_floats, sg_prep_ends; csrc/mcpc_plan.h: ce_job_table,
// lw_job_table; the chunk arithmetic of eval_setup / eval_chunks in csrc/mcpc_eval.hip) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own.  For the nets of tests/state_grad_cases.py and a few extreme ones it walks, chunk
// by chunk, what the three launches index: the prep launch's flat index -> (layer, row, quad) through bounds-checked tables of the
// scratch's size; every (row, unit) of the error rows the forward jobs store, and that the backward jobs read only what was stored.
// Host code only: nothing touches a device.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Imontecarlopredictivecoding_amd/csrc scripts/state_grad_plan_sanitize.hip \
//         -o scripts/bin/state_grad_plan_sanitize
//   scripts/bin/state_grad_plan_sanitize        (exit status 0 and no report: clean)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mcpc_plan.h"
#include "mcpc_state_grad.h"

using namespace mcpc;

static int pad16i(int n) { return (n + 15) / 16 * 16; }

static int run_case(std::vector<int> sizes, int n_out, int64_t R, int max_rows) {
    const int L = (int)sizes.size();
    int npad[kMaxLatent + 1] = {};
    for (int l = 0; l < L; ++l) npad[l] = pad16i(sizes[l]);
    const int out_pad = pad16i(n_out);
    std::vector<LwJob> ce, fwd, bwd;
    int n_head = 0;
    CeFinish F{};
    ce_job_table(L, npad, out_pad, ce, n_head, F);
    lw_job_table(L, npad, out_pad, fwd, bwd);
    // the chunk, as eval_setup forms it
    const int64_t want = max_rows > 0 ? max_rows : kCeDefaultRows;
    const int chunk = (int)(std::min<int64_t>((want + kLwChains - 1) / kLwChains, (R + kLwChains - 1) / kLwChains) * kLwChains);
    size_t floats[kMaxLatent + 1];
    sg_err_floats(L, npad, out_pad, chunk, floats);
    int bad = 0;
    for (int64_t r0 = 0; r0 < R; r0 += chunk) {
        const int rows = (int)std::min<int64_t>(chunk, R - r0);
        const int padded = (rows + kLwChains - 1) / kLwChains * kLwChains;
        if (padded > chunk || r0 % kLwChains) ++bad;
        // the prep launch: every quad of every layer exactly once, inside the scratch
        unsigned end4[kMaxLatent];
        if (!sg_prep_ends(L, npad, padded, end4)) { ++bad; continue; }
        std::vector<std::vector<uint8_t>> seen(L);
        for (int l = 0; l < L; ++l) seen[l].assign((size_t)chunk * npad[l] / 4, 0);
        for (unsigned idx = 0; idx < end4[L - 1]; ++idx) {
            int l = 0;
            for (int k = 0; k < kMaxLatent - 1; ++k) l += (k < L - 1 && idx >= end4[k]) ? 1 : 0;
            const unsigned loc = idx - (l > 0 ? end4[l - 1] : 0u);
            const int q = npad[l] / 4;
            if ((int)(loc / q) >= padded) ++bad;
            seen.at(l).at(loc) += 1;
        }
        for (int l = 0; l < L; ++l)
            for (size_t i = 0; i < (size_t)padded * npad[l] / 4; ++i) bad += seen[l][i] != 1;
        // the forward launch stores e_l (l >= 1) and e_o: every 16-unit tile of every padded row once, inside the error scratch
        std::vector<std::vector<uint8_t>> err(kMaxLatent + 1);
        for (int l = 0; l <= kMaxLatent; ++l) err[l].assign(floats[l] / 16, 0);
        for (int ct = 0; ct < padded / 16; ++ct)
            for (const LwJob& jb : ce) {
                const int j = jb.layer, ntiles = (j < L ? npad[j] : out_pad) / 16;
                for (int ut = jb.ut0; ut < std::min(jb.ut0 + kLwUnitTiles, ntiles); ++ut)
                    if (j > 0) err.at(j < L ? j : kMaxLatent).at((size_t)ct * ntiles + ut) += 1;
            }
        // the backward launch reads, as the B operand of layer l's jobs, every tile of e_{l+1} (e_o above the last layer) of its rows
        for (int ct = 0; ct < padded / 16; ++ct)
            for (const LwJob& jb : bwd) {
                const int l = jb.layer;
                if (l < 0 || l >= L || jb.ut0 >= npad[l] / 16) { ++bad; continue; }
                const bool last = l == L - 1;
                if (last && out_pad == 0) continue;
                const int kt = (last ? out_pad : npad[l + 1]) / 16;
                for (int k = 0; k < kt; ++k) bad += err.at(last ? kMaxLatent : l + 1).at((size_t)ct * kt + k) != 1;
            }
    }
    if (bad) printf("bad: L=%d n_out=%d R=%lld max_rows=%d\n", L, n_out, (long long)R, max_rows);
    return bad ? 1 : 0;
}

int main() {
    int bad = 0, cases = 0;
    for (int max_rows : {0, 64, 128, 100})
        for (int64_t R : {1, 60, 210, 48, 72}) {
            bad += run_case({6, 16, 16}, 24, R, max_rows);
            bad += run_case({200, 33, 17}, 40, R, max_rows);
            bad += run_case({272, 144}, 784, R, max_rows);
            bad += run_case({37}, 0, R, max_rows);
            bad += run_case({40, 24}, 0, R, max_rows);
            bad += run_case({16, 48, 24, 40, 33, 17}, 12, R, max_rows);
            bad += run_case({12, 784}, 10, R, max_rows);
            cases += 7;
        }
    bad += run_case({256, 256, 256}, 784, 16384 + 5, 0);
    bad += run_case({1, 2049}, 4097, 130, 0);
    cases += 2;
    // a chunk too large for one prep launch is told apart, not wrapped
    int npad[kMaxLatent] = {4096, 4096, 4096, 4096, 4096, 4096};
    unsigned end4[kMaxLatent];
    if (sg_prep_ends(6, npad, 1 << 20, end4)) ++bad;
    if (!sg_prep_ends(6, npad, 1 << 19, end4) || end4[5] != 6u * (1u << 19) * 1024u) ++bad;
    printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
