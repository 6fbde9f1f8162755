// libmcpc.so, the evaluators of recorded states and the ancestral sampler: mcpc_chain_energies, mcpc_prediction_errors, mcpc_state_gradients,
// mcpc_sample_prior with their kernels (mcpc_chain_energy.h, mcpc_pred_err.h, mcpc_state_grad.h, mcpc_ancestral.h: the only unit that includes them).  They share the
// layer-wise tile (mcpc_lw_tile.h), the packed weights, mu_1's kernel (launch_mu1) and the engine's evaluator scratch with each other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <vector>

#include "mcpc_engine.h"
#include "mcpc_chain_energy.h"
#include "mcpc_pred_err.h"
#include "mcpc_state_grad.h"
#include "mcpc_ancestral.h"

using namespace mcpc;

namespace {
// The front the two evaluators share (mcpc_chain_energies, mcpc_prediction_errors).  What a call reads and launches over:
struct EvalCall {
    unsigned layers;        // bit l: latent layer l is read -- x_rec[l] is required, and prepared chunk by chunk
    unsigned lins;          // bit j (bit L: the read-out): Linear j is evaluated -- it must be bound; Linear 0 needs mu_1 of the call's inputs
    unsigned pe_table;      // the Linears of the prediction-error job table the call launches over; 0: it launches over the chain-energy table
    bool with_loss;         // the read-out's error is the loss's (its kind and mask reach the kernels)
};

// The evaluators' job tables, mu_1 buffer and scratch for chunks of `chunk` rows
int ce_ensure_scratch(mcpc_engine* e, int chunk, unsigned pe_table, hipStream_t stream) {
    if (!e->ce_jobs) {
        std::vector<LwJob>& jobs = e->ce_table;
        ce_job_table(e->L, e->npad, e->has_head ? e->out_pad : 0, jobs, e->ce_nhead, e->ce_finish);
        if (jobs.size() > 65535) return fail(MCPC_EINVAL, "chain energies: more than 65535 unit-tile jobs");
        if (const int rc = upload(e->ce_jobs, jobs, "the chain-energy job table")) return rc;
        e->ce_njobs = (int)jobs.size();
        if (const int rc = dmalloc(e->ce_mu1, (size_t)e->Bpad * e->npad[0])) return rc;
    }
    if (chunk > e->ce_rows) {
        // everything is given up before the first new allocation: one that fails leaves a consistent, empty scratch
        for (int l = 0; l < e->L; ++l) { give_up(e, e->ce_x[l], stream); give_up(e, e->ce_fx[l], stream); }
        give_up(e, e->ce_part, stream);
        e->ce_rows = 0;
        for (int l = 0; l < e->L; ++l) {
            int rc;
            if ((rc = dmalloc(e->ce_x[l], (size_t)chunk * e->npad[l])) || (rc = dmalloc(e->ce_fx[l], (size_t)chunk * e->npad[l]))) return rc;
        }
        if (const int rc = dmalloc(e->ce_part, (size_t)e->ce_njobs * chunk)) return rc;
        e->ce_rows = chunk;
    }
    if (pe_table && pe_table != e->pe_want) {
        std::vector<LwJob> jobs;
        pe_job_table(e->ce_table, pe_table, jobs);
        give_up(e, e->pe_jobs, stream);
        e->pe_want = 0;                  // (an upload that fails leaves no table, and no set of Linears it would be the table of)
        if (const int rc = upload(e->pe_jobs, jobs, "the prediction-error job table")) return rc;
        e->pe_want = pe_table;
        e->pe_njobs = (int)jobs.size();
    }
    return MCPC_OK;
}

// The checks of a call, before anything of the device is touched; `pre` ("<entry>: ") opens every message
int eval_check_call(const char* pre, const mcpc_engine* e, const float* const* x_rec, int32_t n_rec, int32_t max_rows) {
    if (!e) return fail(MCPC_EINVAL, "%snull engine", pre);
    if (!x_rec) return fail(MCPC_EINVAL, "%sx_rec is null", pre);
    if (n_rec < 0) return fail(MCPC_EINVAL, "%sn_rec=%d, must not be negative", pre, n_rec);
    if (max_rows < 0) return fail(MCPC_EINVAL, "%smax_rows=%d, must not be negative (0 = default)", pre, max_rows);
    return 0;
}
int eval_check_reads(const char* pre, const mcpc_engine* e, const float* const* x_rec, const EvalCall& c) {
    for (int l = 0; l < e->L; ++l)
        if (((c.layers >> l) & 1u) && !x_rec[l]) return fail(MCPC_EINVAL, "%sx_rec[%d] is null", pre, l);
    for (int j = 0; j < e->L + (e->has_head ? 1 : 0); ++j)
        if (((c.lins >> j) & 1u) && !e->lin[j].bound)
            return fail(MCPC_ESTATE, "%sLinear %d has no bound parameters (mcpc_bind_params + mcpc_params_changed first)", pre, j);
    return 0;
}

// An accepted call of R rows: the chunk, the scratch and the tables for it, mu_1 where it is read, and what the two kernels' parameters share
int eval_setup(mcpc_engine* e, const EvalCall& c, const float* inputs, int64_t R, int32_t max_rows, int32_t loss_kind, double loss_var,
               int32_t mask_start, hipStream_t stream, CeParams& Q) {
    HIP_TRY(hipSetDevice(e->d.device));
    // the chunk: a multiple of the 64-row tile, no longer than the call
    const int64_t want = max_rows > 0 ? max_rows : kCeDefaultRows;
    const int chunk = (int)(std::min<int64_t>((want + kLwChains - 1) / kLwChains, (R + kLwChains - 1) / kLwChains) * kLwChains);
    if (const int rc = ce_ensure_scratch(e, chunk, c.pe_table, stream)) return rc;
    free_completed_retired(e);
    if (c.lins & 1u) launch_mu1(e, inputs, e->ce_mu1, e->d.batch, e->Bpad, stream);      // mu_1 of THESE inputs (the step kernels' own kernel: the same bits)
    const int nlin = e->L + (e->has_head ? 1 : 0);
    for (int l = 0; l < e->L; ++l) { Q.x[l] = e->ce_x[l]; Q.fx[l] = e->ce_fx[l]; Q.npad[l] = e->npad[l]; Q.ecoef[l] = e->d.ecoef[l]; }
    for (int j = 1; j < nlin; ++j) { Q.Wf[j] = e->lin[j].Wf; Q.bias[j] = e->lin[j].bias_pad; }
    Q.npad[e->L] = e->has_head ? e->out_pad : 0;
    Q.mu1 = e->ce_mu1; Q.y = e->ypad; Q.wexp = e->wexp;
    Q.L = e->L; Q.B = e->d.batch; Q.n_out = e->d.n_out; Q.chunk = chunk;
    Q.loss_kind = c.with_loss ? loss_kind : MCPC_LOSS_NONE; Q.mask_start = c.with_loss ? mask_start : 0;
    Q.inv_var = loss_kind == MCPC_LOSS_GAUSSIAN ? (float)(1.0 / loss_var) : 1.0f;
    return MCPC_OK;
}

// The chunk loop: x_l and f(x_l) of the layers the call reads go to the scratch, then `launch(r0, rows, padded)` launches the entry's own
// kernels for rows [r0, r0 + rows) of the call, with Q.rows and Q.row_base set (padded: the rows of the tiles that hold one)
int eval_chunks(const mcpc_engine* e, const EvalCall& c, const float* const* x_rec, int64_t R, CeParams& Q, hipStream_t stream,
                const std::function<void(int64_t, int, int)>& launch) {
    for (int64_t r0 = 0; r0 < R; r0 += Q.chunk) {
        const int rows = (int)std::min<int64_t>(Q.chunk, R - r0);
        const int padded = (rows + kLwChains - 1) / kLwChains * kLwChains;
        for (int l = 0; l < e->L; ++l) {
            if (!((c.layers >> l) & 1u)) continue;
            const size_t total4 = (size_t)padded * e->npad[l] / 4;
            hipLaunchKernelGGL(mcpc_ce_prep_kernel, dim3(grid_for(total4)), dim3(256), 0, stream, x_rec[l] + (size_t)r0 * e->d.sizes[l],
                               e->ce_x[l], e->ce_fx[l], rows, padded, e->d.sizes[l], e->npad[l], e->d.acts[l]);
        }
        Q.rows = rows;
        Q.row_base = (int)(r0 % e->d.batch);
        launch(r0, rows, padded);
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

// The error rows of mcpc_state_gradients for chunks of `chunk` rows (the evaluators' scratch holds e->ce_rows >= chunk by now), and its
// backward job table
int sg_ensure_scratch(mcpc_engine* e, int chunk, hipStream_t stream) {
    if (!e->sg_bjobs) {
        std::vector<LwJob> fwd, bwd;
        lw_job_table(e->L, e->npad, e->has_head ? e->out_pad : 0, fwd, bwd);
        if (bwd.size() > 65535) return fail(MCPC_EINVAL, "state gradients: more than 65535 unit-tile jobs");
        if (const int rc = upload(e->sg_bjobs, bwd, "the state-gradient job table")) return rc;
        e->sg_nb = (int)bwd.size();
    }
    if (chunk > e->sg_rows) {
        // everything is given up before the first new allocation: one that fails leaves a consistent, empty scratch
        for (int l = 0; l < e->L; ++l) give_up(e, e->sg_err[l], stream);
        give_up(e, e->sg_err_o, stream);
        e->sg_rows = 0;
        size_t floats[kMaxLatent + 1];
        sg_err_floats(e->L, e->npad, e->has_head ? e->out_pad : 0, e->ce_rows, floats);
        for (int l = 1; l < e->L; ++l)
            if (const int rc = dmalloc(e->sg_err[l], floats[l])) return rc;
        if (e->has_head)
            if (const int rc = dmalloc(e->sg_err_o, floats[kMaxLatent])) return rc;
        e->sg_rows = e->ce_rows;
    }
    return MCPC_OK;
}
}  // namespace

extern "C" {

int mcpc_chain_energies(mcpc_engine* e, const float* inputs, const float* const* x_rec, int32_t n_rec, int32_t loss_kind, double loss_var,
                        int32_t mask_start, double* out, int32_t max_rows, void* stream_) {
    static const char pre[] = "chain energies: ";
    if (const int rc = eval_check_call(pre, e, x_rec, n_rec, max_rows)) return rc;
    if (!out) return fail(MCPC_EINVAL, "chain energies: out is null");
    // every layer is read and every Linear evaluated
    const bool with_loss = loss_kind != MCPC_LOSS_NONE;
    const EvalCall c{(1u << e->L) - 1u, (1u << (e->L + (e->has_head ? 1 : 0))) - 1u, 0u, with_loss};
    if (const int rc = eval_check_reads(pre, e, x_rec, c)) return rc;
    if (const int rc = check_loss(pre, e, loss_kind, loss_var, mask_start)) return rc;
    const int64_t R = (int64_t)n_rec * e->d.batch;
    if (R == 0) return MCPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    CeParams Q{};
    if (const int rc = eval_setup(e, c, inputs, R, max_rows, loss_kind, loss_var, mask_start, stream, Q)) return rc;
    Q.part = e->ce_part;
    Q.job0 = with_loss ? 0 : e->ce_nhead;
    Q.jobs = e->ce_jobs + Q.job0;
    const int njobs = e->ce_njobs - Q.job0;
    return eval_chunks(e, c, x_rec, R, Q, stream, [&](int64_t r0, int rows, int padded) {
        hipLaunchKernelGGL(mcpc_ce_kernel, dim3(padded / kLwChains, njobs), dim3(kLwThreads), 0, stream, Q);
        hipLaunchKernelGGL(mcpc_ce_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, (const double*)e->ce_part, out, e->ce_finish,
                           e->L, with_loss ? 1 : 0, rows, Q.chunk, (size_t)r0);
    });
}

int mcpc_prediction_errors(mcpc_engine* e, const float* inputs, const float* const* x_rec, int32_t n_rec, int32_t loss_kind, double loss_var,
                           int32_t mask_start, float* const* err, float* const* pred, float* err_out, float* pred_out, int32_t max_rows,
                           void* stream_) {
    static const char pre[] = "prediction errors: ";
    if (const int rc = eval_check_call(pre, e, x_rec, n_rec, max_rows)) return rc;
    const int L = e->L;
    // the Linears asked for (bit j; bit L = the read-out) and the latent layers their predictions read
    unsigned want = 0;
    for (int l = 0; l < L; ++l)
        if ((err && err[l]) || (pred && pred[l])) want |= 1u << l;
    if (err_out || pred_out) want |= 1u << L;
    if (!want) return fail(MCPC_EINVAL, "prediction errors: nothing is asked for (every destination is null)");
    if ((err_out || pred_out) && !e->has_head) return fail(MCPC_EINVAL, "prediction errors: err_out / pred_out need a read-out Linear (n_out > 0)");
    if (const int rc = check_loss_kind(pre, loss_kind)) return rc;
    if (err_out && loss_kind == MCPC_LOSS_NONE) return fail(MCPC_EINVAL, "prediction errors: err_out needs a loss (loss_kind is MCPC_LOSS_NONE)");
    if (err_out)
        if (const int rc = check_loss_values(pre, e, loss_kind, loss_var, mask_start)) return rc;
    const EvalCall c{pe_layers_read(want, L), want, want, err_out != nullptr};
    if (const int rc = eval_check_reads(pre, e, x_rec, c)) return rc;
    if (err_out && !e->target_bound) return fail(MCPC_ESTATE, "prediction errors: err_out requested but no target bound");
    const int64_t R = (int64_t)n_rec * e->d.batch;
    if (R == 0) return MCPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    PeParams P{};
    CeParams& Q = P.ce;
    if (const int rc = eval_setup(e, c, inputs, R, max_rows, loss_kind, loss_var, mask_start, stream, Q)) return rc;
    Q.jobs = e->pe_jobs;
    for (int l = 0; l < L; ++l) P.n[l] = e->d.sizes[l];
    P.n[L] = e->d.n_out;
    // 16-byte stores where every row of a destination starts on a 16-byte boundary
    auto vec_ok = [](const float* p, int n) { return p && n % 4 == 0 && ((uintptr_t)p & 15u) == 0; };
    for (int j = 0; j <= L; ++j) {
        const float* const ep = j < L ? (err ? err[j] : nullptr) : err_out;
        const float* const pp = j < L ? (pred ? pred[j] : nullptr) : pred_out;
        if (vec_ok(ep, P.n[j])) P.vec_err |= 1u << j;
        if (vec_ok(pp, P.n[j])) P.vec_pred |= 1u << j;
    }
    return eval_chunks(e, c, x_rec, R, Q, stream, [&](int64_t r0, int /*rows*/, int padded) {
        // (a chunk starts at a multiple of kLwChains rows: r0 * n_l floats keeps the 16-byte alignment where n_l % 4 == 0)
        for (int j = 0; j <= L; ++j) {
            float* const ep = j < L ? (err ? err[j] : nullptr) : err_out;
            float* const pp = j < L ? (pred ? pred[j] : nullptr) : pred_out;
            P.err[j] = ep ? ep + (size_t)r0 * P.n[j] : nullptr;
            P.pred[j] = pp ? pp + (size_t)r0 * P.n[j] : nullptr;
        }
        hipLaunchKernelGGL(mcpc_pe_kernel, dim3(padded / kLwChains, e->pe_njobs), dim3(kLwThreads), 0, stream, P);
    });
}

int mcpc_state_gradients(mcpc_engine* e, const mcpc_gradient_desc* d) {
    static const char pre[] = "state gradients: ";
    if (!e) return fail(MCPC_EINVAL, "%snull engine", pre);
    if (!d) return fail(MCPC_EINVAL, "%snull descriptor", pre);
    if (!d->x) return fail(MCPC_EINVAL, "%sx is null", pre);
    if (!d->grad) return fail(MCPC_EINVAL, "%sgrad is null", pre);
    if (d->n_rec < 0) return fail(MCPC_EINVAL, "%sn_rec=%d, must not be negative", pre, d->n_rec);
    if (d->max_rows < 0) return fail(MCPC_EINVAL, "%smax_rows=%d, must not be negative (0 = default)", pre, d->max_rows);
    const int L = e->L;
    for (int l = 0; l < L; ++l) {
        if (!d->x[l]) return fail(MCPC_EINVAL, "%sx[%d] is null", pre, l);
        if (!d->grad[l]) return fail(MCPC_EINVAL, "%sgrad[%d] is null", pre, l);
    }
    // every layer is read and every Linear evaluated
    const bool with_loss = d->loss_kind != MCPC_LOSS_NONE;
    const EvalCall c{(1u << L) - 1u, (1u << (L + (e->has_head ? 1 : 0))) - 1u, 0u, with_loss};
    if (const int rc = eval_check_reads(pre, e, d->x, c)) return rc;
    if (const int rc = check_loss(pre, e, d->loss_kind, d->loss_var, d->mask_start)) return rc;
    const int64_t R = (int64_t)d->n_rec * e->d.batch;
    if (R == 0) return MCPC_OK;
    hipStream_t stream = (hipStream_t)d->stream;
    SgParams P{};
    CeParams& Q = P.ce;
    if (const int rc = eval_setup(e, c, d->inputs, R, d->max_rows, d->loss_kind, d->loss_var, d->mask_start, stream, Q)) return rc;
    if (const int rc = sg_ensure_scratch(e, Q.chunk, stream)) return rc;
    // the forward launch walks the whole table: a read-out without a loss propagates an error of zeros, as the step kernels' does
    Q.part = d->energies ? e->ce_part : nullptr;
    Q.job0 = 0;
    Q.jobs = e->ce_jobs;
    P.bjobs = e->sg_bjobs;
    P.has_head = e->has_head ? 1 : 0;
    P.err_o = e->sg_err_o;
    for (int l = 0; l < L; ++l) {
        P.err[l] = e->sg_err[l];
        P.n[l] = e->d.sizes[l];
        P.act[l] = e->d.acts[l];
        // 16-byte stores where every row of a destination starts on a 16-byte boundary
        if (P.n[l] % 4 == 0 && ((uintptr_t)d->grad[l] & 15u) == 0) P.vec_grad |= 1u << l;
    }
    for (int j = 1; j < L + (e->has_head ? 1 : 0); ++j) P.Wb[j] = e->lin[j].Wb;
    SgPrep T{};
    T.L = L;
    for (int l = 0; l < L; ++l) { T.x[l] = e->ce_x[l]; T.fx[l] = e->ce_fx[l]; T.n[l] = P.n[l]; T.npad[l] = e->npad[l]; T.act[l] = P.act[l]; }
    const EvalCall none{0u, c.lins, 0u, with_loss};      // (eval_chunks prepares no layer: the launch below prepares them all at once)
    return eval_chunks(e, none, d->x, R, Q, stream, [&](int64_t r0, int rows, int padded) {
        // (a chunk starts at a multiple of kLwChains rows: r0 * n_l floats keeps the 16-byte alignment where n_l % 4 == 0)
        for (int l = 0; l < L; ++l) { T.rec[l] = d->x[l] + (size_t)r0 * P.n[l]; P.grad[l] = d->grad[l] + (size_t)r0 * P.n[l]; }
        T.rows = rows;
        if (sg_prep_ends(L, e->npad, padded, T.end4)) {
            hipLaunchKernelGGL(mcpc_grad_prep_kernel, dim3(grid_for(T.end4[L - 1])), dim3(256), 0, stream, T);
        } else {                                          // more than 2^32 quads in one chunk: layer by layer
            for (int l = 0; l < L; ++l)
                hipLaunchKernelGGL(mcpc_ce_prep_kernel, dim3(grid_for((size_t)padded * e->npad[l] / 4)), dim3(256), 0, stream, T.rec[l],
                                   e->ce_x[l], e->ce_fx[l], rows, padded, P.n[l], e->npad[l], P.act[l]);
        }
        hipLaunchKernelGGL(mcpc_grad_fwd_kernel, dim3(padded / kLwChains, e->ce_njobs), dim3(kLwThreads), 0, stream, P);
        hipLaunchKernelGGL(mcpc_grad_bwd_kernel, dim3(padded / kLwChains, e->sg_nb), dim3(kLwThreads), 0, stream, P);
        if (d->energies)
            hipLaunchKernelGGL(mcpc_ce_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, (const double*)e->ce_part, d->energies,
                               e->ce_finish, L, with_loss ? 1 : 0, rows, Q.chunk, (size_t)r0);
    });
}

int mcpc_sample_prior(mcpc_engine* e, const float* inputs, int64_t n, uint64_t seed, uint64_t step, uint64_t sample_base, int32_t loss_kind,
                      double loss_var, int32_t readout, float* const* x_out, float* out, int32_t max_rows, void* stream_) {
    static const char pre[] = "sample prior: ";
    if (!e) return fail(MCPC_EINVAL, "%snull engine", pre);
    if (n < 0) return fail(MCPC_EINVAL, "%sn=%lld, must not be negative", pre, (long long)n);
    constexpr uint64_t kChains = 1ull << 32;            // the Philox chain word is 32 bits
    if (sample_base > kChains || (uint64_t)n > kChains - sample_base)
        return fail(MCPC_EINVAL, "%ssample_base=%llu + n=%lld passes 2^32 (the generator's chain word is 32 bits)", pre,
                    (unsigned long long)sample_base, (long long)n);
    if (max_rows < 0) return fail(MCPC_EINVAL, "%smax_rows=%d, must not be negative (0 = default)", pre, max_rows);
    if (readout != MCPC_SAMPLE_HIDDEN && readout != MCPC_SAMPLE_MEAN && readout != MCPC_SAMPLE_DRAW)
        return fail(MCPC_EINVAL, "%sunknown readout %d", pre, readout);
    if (const int rc = check_loss_kind(pre, loss_kind)) return rc;
    const int L = e->L;
    if (out && !e->has_head) return fail(MCPC_EINVAL, "%sout needs a read-out Linear (n_out > 0)", pre);
    // the Linears to run: up to the read-out, or to the last latent layer asked for
    int last = out ? L : -1;
    if (!out && x_out)
        for (int l = 0; l < L; ++l)
            if (x_out[l]) last = l;
    if (last < 0) return fail(MCPC_EINVAL, "%snothing is asked for (every destination is null)", pre);
    if (out && readout != MCPC_SAMPLE_HIDDEN) {
        if (loss_kind == MCPC_LOSS_NONE) return fail(MCPC_EINVAL, "%sthe mean or a draw of the read-out needs a loss (loss_kind is MCPC_LOSS_NONE)", pre);
        if (readout == MCPC_SAMPLE_DRAW && loss_kind == MCPC_LOSS_GAUSSIAN && !(loss_var > 0.0))
            return fail(MCPC_EINVAL, "%sloss_var=%g, must be positive", pre, loss_var);
    }
    // (every ecoef is positive: mcpc_create refuses an engine with another one, so 1 / sqrt(ecoef) below is finite)
    for (int j = 0; j <= last; ++j)
        if (!e->lin[j].bound)
            return fail(MCPC_ESTATE, "%sLinear %d has no bound parameters (mcpc_bind_params + mcpc_params_changed first)", pre, j);
    if (n == 0) return MCPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(e->d.device));
    // the chunk: a multiple of the 64-row tile, no longer than the call; the scratch and the job table are the evaluators'
    const int64_t want = max_rows > 0 ? max_rows : kCeDefaultRows;
    const int chunk = (int)(std::min<int64_t>((want + kLwChains - 1) / kLwChains, (n + kLwChains - 1) / kLwChains) * kLwChains);
    if (const int rc = ce_ensure_scratch(e, chunk, 0u, stream)) return rc;
    free_completed_retired(e);
    int mode = kSpLogits;
    if (readout == MCPC_SAMPLE_MEAN && loss_kind == MCPC_LOSS_BERNOULLI) mode = kSpSigmoid;
    if (readout == MCPC_SAMPLE_DRAW) mode = loss_kind == MCPC_LOSS_BERNOULLI ? kSpBernoulli : kSpGaussian;
    const int n_in = e->d.n_in;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int rows = (int)std::min<int64_t>(chunk, n - r0);
        const int padded = (rows + kLwChains - 1) / kLwChains * kLwChains;
        // mu_1 of the chunk's inputs, by the runs' and the evaluators' own kernel, in the scratch no launch of this call reads as x_0
        launch_mu1(e, inputs ? inputs + (size_t)r0 * n_in : nullptr, e->ce_x[0], rows, padded, stream);
        for (int j = 0; j <= last; ++j) {
            const bool head = j == L;
            SpParams P{};
            P.fx_in = j > 0 ? e->ce_fx[j - 1] : nullptr;
            P.fx_out = j < last ? e->ce_fx[j] : nullptr;
            P.Wf = j > 0 ? e->lin[j].Wf : nullptr;
            P.bias = j > 0 ? e->lin[j].bias_pad : nullptr;
            P.mu1 = e->ce_x[0];
            P.wexp = e->wexp;
            P.jobs = e->ce_jobs + e->ce_finish.first[j];
            P.seed = seed; P.step = step; P.g0 = sample_base + (uint64_t)r0;
            P.kw = j > 0 ? e->npad[j - 1] : 0;
            P.npad = head ? e->out_pad : e->npad[j];
            P.n = head ? e->d.n_out : e->d.sizes[j];
            P.act = head ? 0 : e->d.acts[j];
            P.rows = rows;
            P.mode = head ? mode : kSpLatent;
            P.scale = head ? (mode == kSpGaussian ? (float)std::sqrt(loss_var) : 1.0f) : (float)(1.0 / std::sqrt((double)e->d.ecoef[j]));
            float* const base = head ? out : (x_out ? x_out[j] : nullptr);
            // (a chunk starts at a multiple of kLwChains rows: r0 * n floats keeps the 16-byte alignment where n % 4 == 0)
            P.dst = base ? base + (size_t)r0 * P.n : nullptr;
            P.vec = base && P.n % 4 == 0 && ((uintptr_t)base & 15u) == 0;
            hipLaunchKernelGGL(mcpc_sp_kernel, dim3(padded / kLwChains, e->ce_finish.count[j]), dim3(kLwThreads), 0, stream, P);
        }
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

}  // extern "C"
