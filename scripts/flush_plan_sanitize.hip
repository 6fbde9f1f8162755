// The host planner (csrc/mcpc_plan.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: it plans
// cfg-M's learning call and the directed flush shapes of tests/test_run_plan_host.py (FLUSH_NETS x FLUSH_TUNINGS), twice into the
// same RunPlan (the storage a run keeps for the next one), and prints the JSON of the last.  Host code only: nothing touches a device.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Imontecarlopredictivecoding_amd/csrc scripts/flush_plan_sanitize.hip \
//         -o scripts/bin/flush_plan_sanitize
//   scripts/bin/flush_plan_sanitize > /dev/null        (exit status 0 and no report: clean)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "mcpc_plan.h"          // (sees no kernel: mcpc_types.h, mcpc_heb_forms.h, mcpc_host.h)

using namespace mcpc;

static int plan_case(const std::vector<int>& sizes, int n_out, int batch, const std::string& tuning, const mcpc_run_desc& r, RunPlan& run,
                     size_t* launches) {
    mcpc_net_desc d{};
    d.abi_version = MCPC_ABI_VERSION;
    d.n_latent = (int)sizes.size();
    d.n_in = 10;
    for (size_t l = 0; l < sizes.size(); ++l) { d.sizes[l] = sizes[l]; d.acts[l] = 1; d.ecoef[l] = 1.0f; }
    d.n_out = n_out;
    d.batch = batch;
    d.tuning = tuning.empty() ? nullptr : tuning.c_str();
    if (const int rc = check_net_desc(&d)) return rc;
    EnginePlan e;
    if (const int rc = parse_tuning(d.tuning, e.knobs)) return rc;
    if (const int rc = plan_engine(d, 256, (size_t)288 << 30, e)) return rc;
    if (const int rc = check_step_range(r)) return rc;
    for (int rep = 0; rep < 2; ++rep) plan_run(e, r, false, run);
    for (const RunItem& it : run.items) {
        if (it.flush < 0) continue;
        const FlushPlan& f = run.flushes[it.flush];
        for (int j = 1; j < e.L + e.has_head; ++j) {
            const LinFlush& lf = f.lin[j];
            if (strlen(lf.text) >= sizeof lf.text - 1) return fail(MCPC_ESTATE, "flush text of Linear %d fills its buffer", j);
            if ((size_t)lf.ksplit * ((size_t)e.lin[j].out_pad * e.lin[j].in_pad + e.lin[j].out_pad) > e.lin[j].slab_floats)
                return fail(MCPC_ESTATE, "Linear %d: %d splits exceed its slabs", j, lf.ksplit);
            for (int i = 0; i < lf.n_launch; ++i) {
                const FlushLaunch& l = lf.launch[i];
                if (l.family != HEB_DW && (l.form < 0 || l.form >= kNumHebForms)) return fail(MCPC_ESTATE, "Linear %d: launch without a form", j);
                ++*launches;
            }
        }
    }
    const std::string s = plan_json(e) + run_plan_json(e, run);
    printf("%s\n", s.c_str());
    return 0;
}

int main() {
    RunPlan run;
    size_t launches = 0;
    mcpc_run_desc r{};
    r.update_x = 1; r.xopt_kind = MCPC_XOPT_SGD; r.noise_mode = MCPC_NOISE_PHILOX; r.loss_kind = MCPC_LOSS_BERNOULLI;
    // cfg-M's learning call
    r.T = 5000; r.n_steps = 5000; r.acc_begin = 1000; r.acc_end = 5000;
    if (plan_case({30, 256, 256}, 784, 6000, "", r, run, &launches)) { fprintf(stderr, "cfg-M: %s\n", g_err.c_str()); return 1; }
    // ... and with many short segments (ring parts of 2 slots)
    r.T = 600; r.n_steps = 600; r.acc_begin = 0; r.acc_end = 600;
    if (plan_case({30, 256, 256}, 784, 256, "slot_cap=6", r, run, &launches)) { fprintf(stderr, "cfg-M, short segments: %s\n", g_err.c_str()); return 1; }
    // the directed shapes
    struct Net { std::vector<int> sizes; int n_out; };
    const Net nets[] = {{{16, 256, 256}, 272}, {{32, 256, 128, 128}, 272}, {{64, 256, 128}, 256}, {{128, 256}, 528}, {{128, 256}, 304},
                        {{128, 256}, 240}, {{512, 256}, 784}, {{32, 48, 100}, 60}};
    r.T = 10; r.n_steps = 10; r.acc_begin = 0; r.acc_end = 10;
    for (const Net& n : nets)
        for (const char* extra : {"", ",heb_fp32=1", ",heb171=1", ",heb171=1,heb_fp32=1", ",flush_streams=1", ",no_overlap=1", ",dw_ksplit=7",
                                  ",dw_ksplit=7,heb_fp32=1"})
            if (plan_case(n.sizes, n.n_out, 64, std::string("wide=1,slot_cap=12") + extra, r, run, &launches)) {
                fprintf(stderr, "directed shape (read-out %d, tuning %s): %s\n", n.n_out, extra, g_err.c_str());
                return 1;
            }
    fprintf(stderr, "planned %zu flush launches: clean\n", launches);
    return 0;
}
