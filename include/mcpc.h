/*
 * mcpc.h -- C ABI of libmcpc.so: the MI355X-native Monte Carlo Predictive Coding engine.
 *
 * Drop-in boundary for ONE hot path of gaspardol/MonteCarloPredictiveCoding: the body of
 * PCTrainer.train_on_batch's `for t in range(T)` loop
 * (reference predictive_coding/pc_trainer.py:712-981) together with the Langevin callback
 * random_step (reference utils/model.py:35-44), for networks of the shape built by
 * get_model (reference utils/model.py:47-69) and by the toy scripts
 * (reference figure_2.py:40-44, figure_3.py:50-55):
 *
 *     Sequential[ Linear, PCLayer, (act), Linear, PCLayer, (act), ..., Linear (, PCLayer) ]
 *
 * The reference has no FFI layer of its own (it is pure Python on torch); the entry points
 * below are what a binding for this path has to call, each annotated with the reference
 * lines it replaces.  Plain pointers and sizes only: no torch types.  All `float*`/`double*`
 * arguments are DEVICE pointers (HIP, gfx950) unless stated otherwise; `stream` is a
 * hipStream_t passed as void*.  Every function returns 0 on success or a negative MCPC_E*
 * code; mcpc_last_error() returns a human-readable message for the calling thread.
 *
 * Threading: one engine per (device, stream); an engine is not re-entrant.  All launches are
 * asynchronous on the given stream; the calls that wait for the device are mcpc_create / mcpc_destroy,
 * mcpc_sync_check and the two profiling getters.  mcpc_run does not wait for the stream, with three
 * bounded exceptions: a run with MCPC_XOPT_ADAM uploads its bias-correction table from one of two pinned
 * staging buffers and waits (hipEventSynchronize) for the upload issued two Adam runs earlier if that
 * has still not executed; and the first run that accumulates Hebbian sums allocates the spill ring
 * (hipMalloc); and the first run after an mcpc_bind_target that could take a specialised instantiation
 * of the in-place step kernel (fused SGD + Philox kick or Adam without noise, all-ReLU network,
 * Bernoulli loss, engine on the in-place kernel; not under tuning spec=0) and has at least spec_wait
 * steps (tuning, default 0: every such run) waits (hipEventSynchronize) for the three flag words that bind copied to
 * the host behind its kernels -- i.e. until the stream has executed everything queued up to and
 * including the bind.  A shorter run only polls that copy (hipEventQuery) and keeps the generic kernel
 * until it has landed.
 * Device buffers that have to grow (per-step tables, energy partials; geometrically) are replaced, the
 * old ones retired behind an event and freed by a later run once that event has completed.
 * The library reads no environment variables.
 */
#ifndef MCPC_H
#define MCPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCPC_ABI_VERSION 4
#define MCPC_MAX_LATENT 6

/* status codes */
#define MCPC_OK 0
#define MCPC_EINVAL (-1)       /* bad argument / unsupported configuration */
#define MCPC_EHIP (-2)         /* a HIP runtime call failed */
#define MCPC_ENOMEM (-3)       /* configuration does not fit the device (LDS / HBM) */
#define MCPC_ESTATE (-4)       /* call order violated (e.g. run before bind) */

/* activation applied to x_l before the next Linear (reference utils/model.py:49-52) */
#define MCPC_ACT_IDENTITY 0
#define MCPC_ACT_RELU 1
#define MCPC_ACT_TANH 2

/* output loss (reference utils/model.py:17-33); masked variants = mask_start > 0 */
#define MCPC_LOSS_NONE 0       /* loss_fn=None or zero_fn */
#define MCPC_LOSS_GAUSSIAN 1   /* fe_fn: (1/var)*0.5*(out-y)^2, summed */
#define MCPC_LOSS_BERNOULLI 2  /* bernoulli_fn: BCEWithLogits, summed */

/* optimizer on x (reference pc_trainer.py:465-475,871-877) */
#define MCPC_XOPT_SGD 0        /* optim.SGD(lr), no momentum / weight decay */
#define MCPC_XOPT_ADAM 1       /* optim.Adam(lr, betas, eps), state reset per run */

/* noise source for the Langevin kick x += sqrt(noise_var*lr)*xi (reference utils/model.py:35-44) */
#define MCPC_NOISE_NONE 0      /* PC / MAP inference */
#define MCPC_NOISE_PHILOX 1    /* fused counter-based Philox4x32-10 + Box-Muller */
#define MCPC_NOISE_EXTERNAL 2  /* xi read from ext_noise[l] (parity tests, arbitrary generators) */

/* which steps write loss / layer energies (reference pc_trainer.py:776-797,835-836) */
#define MCPC_ENERGY_NONE 0
#define MCPC_ENERGY_LAST 1
#define MCPC_ENERGY_ALL 2

typedef struct mcpc_engine mcpc_engine;

/* Static description of the network and the shard of chains this engine owns. */
typedef struct mcpc_net_desc {
    int32_t abi_version;                 /* MCPC_ABI_VERSION */
    int32_t n_latent;                    /* number of PCLayers L, 1..MCPC_MAX_LATENT */
    int32_t n_in;                        /* width of the pseudo-input fed to the first Linear */
    int32_t sizes[MCPC_MAX_LATENT];      /* n_1..n_L, top latent first (reference utils/model.py:54-65) */
    int32_t acts[MCPC_MAX_LATENT];       /* MCPC_ACT_* applied to x_l */
    float ecoef[MCPC_MAX_LATENT];        /* c_l in energy c_l*0.5*(mu-x)^2 (reference pc_layer.py:17-18, figure_3.py:47-48) */
    int32_t n_out;                       /* width of the read-out Linear; 0 = model ends with a PCLayer */
    int32_t batch;                       /* chains held by this engine (local shard) */
    int32_t device;                      /* HIP device ordinal */
    int64_t spill_budget_bytes;          /* HBM budget for the Hebbian spill ring; 0 = default: room for 384 steps in three parts (17 GB at 6000
                                          * chains of cfg-M's net), at least 6 GiB, at most a quarter of the device's memory */
    const char* tuning;                  /* NULL, or developer overrides of the schedule heuristics as "key=value,key=value"
                                          * (parsed once by mcpc_create, not kept): ws=0|2|3|4 step kernel (0: the barrier kernel, the
                                          * fallback and the independent form parity checks replay the default against; 2: the in-place
                                          * wave-specialised kernel for every run; 3: the unified-wave kernel for the runs it serves -- fused
                                          * SGD / Adam updates -- or an error when its LDS plan does not fit; default: in-place, with the
                                          * unified-wave kernel for small networks and for zero-loss calls; 4: the layer-wise kernels
                                          * mcpc_lw_fwd_kernel + mcpc_lw_bwd_kernel for every run, whatever the widths -- state, activations
                                          * and errors of all chains in global memory, two launches per step; together with no_lean, no_xl,
                                          * overlay16, rr or u_*, knobs of the LDS-resident kernels, it is MCPC_EINVAL),
                                          * wide=1 (the choice stays as without it, and the layer-wise kernels serve the engine ONLY where
                                          * mcpc_create would otherwise fail with MCPC_ENOMEM because no LDS plan holds the network or its
                                          * last latent layer is wider than 256 units under a read-out; composes with every other key: a
                                          * forced ws=0|2|3 whose plan does not fit falls to the layer-wise kernels too.  Without ws=4 or
                                          * wide=1 such a network is rejected with MCPC_ENOMEM.  On the layer-wise kernels the widths are
                                          * limited by device memory only -- per chain and unit 12 B of state, activation and error, 8 B of
                                          * Adam moments, and the Hebbian spill ring; MCPC_MAX_LATENT stays 6), u_row / u_gemm0 / u_kb / u_kbt /
                                          * u_eh / u_eb / u_ef=N (cost model the unified-wave kernel's rows are dealt by),
                                          * no_overlap=1, slot_cap=N, spill_gb=N, ring_parts=N,
                                          * flush_tail=N, flush_streams=1|2, cu_slack=N, dw_ksplit=N, ws_prio=0|1|2, stagger=N, no_lean=1,
                                          * no_ybits=1, overlay16=1, heb_fp32=1 (the Hebbian GEMM on the fp32 MFMA instead of its fp16
                                          * form), rr=0 (shards of more 16-chain units than CUs as ONE launch in hardware rounds instead of
                                          * the round schedule), rr_qmax=N (most steps per launch of the round schedule), no_xl=1 (state and
                                          * per-step constants of a workgroup's chains in global memory instead of LDS), spec=0 (every launch
                                          * of the in-place kernel on its generic instantiation, never a specialised one), spec_wait=N
                                          * (runs of fewer than N steps do not wait for the host copy of the target's flags: Threading,
                                          * above).  Unknown keys are an error.  Used by A/B runs and by the tests that pin the kernel forms against each other. */
} mcpc_net_desc;

/* One train_on_batch call (or a slice of it).  Steps are numbered 0..T-1 inside the call. */
typedef struct mcpc_run_desc {
    int32_t T;                   /* total steps of the reference call (PCTrainer T), for 'last' semantics */
    int32_t t_begin;             /* first step executed by this run */
    int32_t n_steps;             /* steps executed by this run (t_begin + n_steps <= T) */

    /* Scalar hyper-parameters are DOUBLES (ABI 4): they are Python floats in the reference, and torch rounds each to fp32 exactly
     * once, where it is used (alpha = -lr of SGD's add_; 1 - beta1 of Adam's lerp_; -lr / (1 - beta1^t) of its addcdiv_; 1 / _var of
     * fe_fn).  The library rounds at the same places; an fp32 field would round before the subtraction / division instead
     * (1 - double(0.9f) != 1 - 0.9). */
    int32_t loss_kind;           /* MCPC_LOSS_* */
    int32_t mask_start;          /* first output column that contributes: n_out - round(n_out*perc); 0 = unmasked */
    double loss_var;             /* Gaussian variance (_var) */

    int32_t xopt_kind;           /* MCPC_XOPT_* */
    int32_t adam_step0;          /* Adam step count before this run (0 at the start of a call) */
    double lr;
    double beta1, beta2, eps;    /* Adam */

    int32_t update_x;            /* 1: fused x update (the fast path). 0: gradients only -> xgrad (generic callbacks) */

    int32_t noise_mode;          /* MCPC_NOISE_* */
    double noise_var;            /* random_step's `var` (2.0 = correct Langevin) */
    uint64_t seed;               /* Philox key */
    uint64_t step_base;          /* Philox step counter of step 0 of this call (advances across calls) */
    uint64_t chain_base;         /* global id of this shard's first chain (sharding-invariant noise) */
    const float* ext_noise[MCPC_MAX_LATENT]; /* MCPC_NOISE_EXTERNAL: [n_steps][batch][n_l] per layer */

    int32_t acc_begin, acc_end;  /* accumulate parameter-gradient sums over steps [acc_begin, acc_end) of the call */
    int32_t acc_reset;           /* 1: zero the sums when this run starts accumulating (reference pc_trainer.py:853-859) */

    int32_t energy_mode;         /* MCPC_ENERGY_* */
    double* energies_out;        /* [T or 1][MCPC_MAX_LATENT+2]: loss, E_1..E_L (unused = 0), overall; device pointer */

    int32_t rec_begin, rec_stride, rec_count; /* record x_t / outputs at t = rec_begin + k*rec_stride, k < rec_count */
    float* rec_x[MCPC_MAX_LATENT];            /* [rec_count][batch][n_l] or NULL (reference pc_trainer.py:440-445,772-774) */
    float* rec_out;                           /* [rec_count][batch][n_out] or NULL (is_return_outputs, :769-770) */

    float* xgrad[MCPC_MAX_LATENT];            /* update_x == 0: dF/dx_l -> [batch][n_l] */
} mcpc_run_desc;

/* lifetime -------------------------------------------------------------------------------- */
int mcpc_abi_version(void);
/* What this binary is (ABI 4; nothing in the reference to mirror): one line of space-separated key=value words,
 *   "libmcpc abi=4 arch=gfx950 csrc=<sha256[:16] of the kernel sources + this header> commit=<git short hash[+dirty]|unknown>
 *    exp=0|1 stamps=0|1 flags=[<compiler flags>]"
 * exp=1: the library was built with a timing-experiment switch (csrc/mcpc_build.h: it computes WRONG results on purpose and must
 * never be tested or benchmarked as the product; the Python binding refuses it, bench.py asserts exp=0).  stamps=1: the diagnostic
 * build with in-kernel phase stamps (correct results).  The string is static storage, valid for the life of the process. */
const char* mcpc_build_info(void);
const char* mcpc_last_error(void);
int mcpc_create(const mcpc_net_desc* desc, mcpc_engine** out);
int mcpc_destroy(mcpc_engine* e);

/* Parameters of Linear j (j = 0..L-1 predicts latent layer j+1; j = L is the read-out), torch
 * nn.Linear layout W[out][in] row-major, bias[out] or NULL.  The engine keeps the pointers
 * (borrowed storage) and re-packs them into MFMA fragment order at mcpc_params_changed().
 * Replaces: nn.Linear.forward inside self._model(self.inputs), pc_trainer.py:733. */
int mcpc_bind_params(mcpc_engine* e, int j, const float* W, const float* bias);
/* Re-pack all bound parameters (call after binding and after every optimizer_p.step()). */
int mcpc_params_changed(mcpc_engine* e, void* stream);

/* Pseudo-input [batch][n_in] (NULL = zeros, the reference's usual call) and target [batch][n_out].
 * Replaces: `inputs`, loss_fn_kwargs['_target'] of train_on_batch, pc_trainer.py:500-524.
 * mcpc_bind_target never waits.  On an engine that may take a specialised instantiation of the
 * in-place kernel it also queues a 12-byte copy of what its kernels found (target exactly 0/1, target
 * inside [-1, 2]) to pinned host memory, and an event behind it; the next candidate mcpc_run waits
 * for, or polls, that event (Threading, above). */
int mcpc_bind_inputs(mcpc_engine* e, const float* inputs, void* stream);
int mcpc_bind_target(mcpc_engine* e, const float* target, void* stream);

/* Latent state x_l, [batch][n_l] row-major (PCLayer._x, pc_layer.py:230,300).  load copies the
 * caller's tensors into the engine's padded state; store writes the current state back. */
int mcpc_load_state(mcpc_engine* e, const float* const* x, void* stream);
int mcpc_store_state(mcpc_engine* e, float* const* x, void* stream);

/* Adam moments of the x optimizer after a run with MCPC_XOPT_ADAM: exp_avg / exp_avg_sq per latent layer, [batch][n_l]
 * (torch.optim.Adam's per-parameter state, reference pc_trainer.py:465-475).  Lets the caller keep optimizer_x alive across
 * calls the way the reference does when neither reset flag of train_on_batch is set (pc_trainer.py:742-752). */
int mcpc_store_adam_state(mcpc_engine* e, float* const* m, float* const* v, void* stream);

/* The hot loop: n_steps iterations of pc_trainer.py:712-981 (+ random_step) on every chain.
 * Asynchronous but for the bounded host waits listed under Threading (Adam table upload, first
 * spill-ring allocation, the bound target's flags once per bind). */
int mcpc_run(mcpc_engine* e, const mcpc_run_desc* run, void* stream);

/* Un-normalised parameter-gradient sums of Linear j accumulated by mcpc_run:
 *   dW[out][in] = scale * sum_t dF/dW(x_t),  db[out] = scale * sum_t dF/db(x_t)   (db may be NULL)
 * accumulate != 0 adds to the destination instead of overwriting (autograd's += into .grad).
 * Replaces: overall.backward()'s parameter part + the normalisation of pc_trainer.py:905-913. */
int mcpc_read_param_grads(mcpc_engine* e, int j, float* dW, float* db, float scale, int accumulate, void* stream);
/* Same, all Linears concatenated (W0,b0,W1,b1,...; absent biases skipped) into one flat buffer,
 * the bucket that is all-reduced once per call across shards. */
int mcpc_read_param_grads_flat(mcpc_engine* e, float* flat, int64_t n_floats, float scale, void* stream);
int64_t mcpc_param_count(const mcpc_engine* e);

/* ---- multi-GPU (the reference is single-device, `use_cuda = torch.cuda.is_available()`
 * figure_2.py:150): one process per GPU, the chains sharded, the weights replicated.  The ONLY collective of a learning
 * call is one sum of the gradient bucket over the shards, before the division by len(accumulate_p_at) * B_global
 * (pc_trainer.py:905-909 divides by len(inputs) = the whole batch).  For a host that is not on torch.distributed the
 * library drives RCCL itself (librccl.so.1 is loaded on first use; ncclAllReduce(sum, fp32) over xGMI):
 *   rank 0:   mcpc_comm_unique_id(id)         and ships the MCPC_COMM_ID_BYTES to the other ranks out of band
 *   all:      mcpc_comm_init(e, n_ranks, rank, id)            (collective: every rank must call it)
 *   per call: mcpc_read_param_grads_flat(e, flat, n, 1/(n_acc*B_global), stream); mcpc_allreduce_grads(e, flat, n, stream)
 * mcpc_allreduce_grads is asynchronous on `stream` and in place; with a communicator of one rank it is the identity.
 * mcpc_destroy releases the communicator. */
#define MCPC_COMM_ID_BYTES 128
int mcpc_comm_unique_id(void* id_out);
int mcpc_comm_init(mcpc_engine* e, int n_ranks, int rank, const void* id);
int mcpc_allreduce_grads(mcpc_engine* e, float* flat, int64_t n_floats, void* stream);
int mcpc_comm_destroy(mcpc_engine* e);

/* Fill out[batch][n_units] with the engine's Philox normals for (seed, step, layer): the device
 * generator exposed for bit-exactness tests against oracle/philox.py. raw != 0 writes the u32 stream. */
int mcpc_philox_normals(int device, uint64_t seed, uint64_t step, int layer, uint64_t chain_base,
                        int batch, int n_units, float* out, int raw, void* stream);

/* (z0[i], z1[i]) = the step kernels' Box-Muller transform (csrc/mcpc_device.h: box_muller) of the bit pair (a[i], b[i]), i < n: the
 * transform exposed on bits the caller chooses, so that its whole domain (2^24 radii from a >> 8, 2^24 angles from b >> 8) can be compared
 * with fp64 (tests/test_gpu_box_muller.py).  Diagnostic, no engine needed; stateless, asynchronous on `stream`.  a, b, z0, z1: device
 * memory of n elements each.  n = 0 launches nothing.  MCPC_EINVAL: a pointer NULL, n < 0. */
int mcpc_box_muller(int device, const uint32_t* a, const uint32_t* b, int64_t n, float* z0, float* z1, void* stream);

/* Streaming first and second moments of recorded steps: what a Langevin call is consumed as (the reference reduces the recorded steps in
 * torch: get_representations(rep_type="expectation"), utils/model.py:150-156; the histograms and means of figure_2.py / figure_3.py).
 * A host reduces the record ring of a sliced call on the device, between the slices of mcpc_run, instead of keeping the trajectory.
 */
#define MCPC_MOM_IDENTITY 0
#define MCPC_MOM_SIGMOID  1   /* g = the read-out's own sigmoid_f (csrc/mcpc_device.h): the Bernoulli mean the step kernels use */

/* For i < row_elems, with r_k = rec + (int64)(first + k*stride) * row_elems, k = 0..n-1 in ascending order:
 *   sum[i]   = (accumulate ? sum[i]   : 0) + g(r_0[i]) + g(r_1[i]) + ...        (fp64, added in exactly this order)
 *   sumsq[i] = (accumulate ? sumsq[i] : 0) + g(r_0[i])^2 + ...                   (sumsq may be NULL)
 * rec is a record buffer as mcpc_run writes it ([records][batch][width] fp32, row_elems = batch*width).  Stateless,
 * asynchronous on `stream`, no engine needed (like mcpc_philox_normals).
 * One thread owns an output element and walks the records with fp64 accumulators in registers: no atomics, no split of the record
 * axis, so the result depends neither on the launch shape nor on how the caller chunks the records (0..36 in one call, or 1 + 5 + 31
 * with accumulate = 1, give the same bits), and with MCPC_MOM_IDENTITY both sums are bitwise a sequential fp64 loop on the host (the
 * square of an fp32 value is exact in fp64).  n = 0 zeroes the accumulators when accumulate = 0 and does nothing otherwise.
 * MCPC_EINVAL: sum NULL, rec NULL with n > 0, row_elems < 1, stride < 1, first < 0, n < 0, unknown transform.  All offsets are 64-bit.
 * 16-B loads per lane when row_elems % 4 == 0 and rec, sum, sumsq are 16-B aligned; a scalar form otherwise.  The accumulators are
 * read and written once per call (16 B per element, 32 with sumsq): long chunks amortise them. */
int mcpc_moments_accumulate(int device, const float* rec, int64_t row_elems, int32_t first, int32_t stride, int32_t n,
                            int32_t transform, double* sum, double* sumsq, int accumulate, void* stream);

/* Streaming second moments BETWEEN units of recorded steps: fp64 sums of outer products, the raw material of a posterior covariance
 * within a layer and across layers (csrc/mcpc_cov.h).  The column space is the concatenation, in order, of n_blocks record buffers
 * (1..MCPC_MAX_LATENT + 1): rec[j] is contiguous fp32 [records][B][widths[j]] as mcpc_run writes rec_x[l] / rec_out, transforms[j] is
 * MCPC_MOM_IDENTITY or MCPC_MOM_SIGMOID (transforms NULL = all identity), D = widths[0] + ... .  With v_k(c) the D transformed values of
 * chain c in record first + k*stride, k = 0..n-1 (exactly the records mcpc_moments_accumulate takes):
 *   pool = 0:  outer[c][i][j] = (accumulate ? outer[c][i][j] : 0) + sum_k v_k(c)[i] * v_k(c)[j]            outer: [B][D][D] fp64
 *   pool = 1:  outer[i][j]    = (accumulate ? outer[i][j]    : 0) + sum_k sum_c v_k(c)[i] * v_k(c)[j]      outer: [D][D] fp64
 * The full matrix is written, both triangles, and outer[i][j] is bitwise outer[j][i] (accumulate = 1 adds the same value to both; they
 * stay bitwise equal where they were).  The first-order sums are mcpc_moments_accumulate's, called for the same blocks.
 * The products are exact in fp64 (fp32 inputs) and run on the fp64 MFMA; only the additions round.  Two runs of the same call give the
 * same bits: the decomposition depends on B and the widths alone and no sum is ordered by the hardware's scheduling (no atomics).  UNLIKE
 * mcpc_moments_accumulate the result is NOT bitwise invariant under how the records are chunked over calls (an MFMA adds four products in
 * an order of its own, and each call rounds once more into outer), nor is the diagonal bitwise that call's sumsq; both agree per entry
 * within (R + G + 2) * 2^-52 * sum |v[i] v[j]|, R = the rows contracted (n, times B when pooled), G = the pooled groups (0 for pool = 0).
 * pool = 1 needs a workspace of mcpc_cov_workspace_bytes(B, widths, n_blocks, 1) bytes (device memory, 8-B aligned, contents
 * irrelevant before and after; [groups][Dpad][Dpad] fp64 partials that a second kernel adds in ascending group order); pool = 0 needs
 * none (0 bytes, workspace may be NULL).  The library allocates nothing.  Stateless, asynchronous on `stream`, all offsets 64-bit.
 * n = 0 reads nothing: it zeroes outer when accumulate = 0 and does nothing otherwise.
 * mcpc_cov_workspace_bytes returns -1 (and a message in mcpc_last_error) for arguments mcpc_cov_accumulate would refuse.
 * MCPC_EINVAL: n_blocks outside 1..MCPC_MAX_LATENT + 1, widths NULL, a width < 1, B < 1, pool not 0 or 1, outer NULL, stride < 1,
 * first < 0, n < 0, an unknown transform, rec or a rec[j] NULL with n > 0, workspace NULL or too small with pool = 1 and n > 0, more
 * than 32768 padded columns, 2^26 or more jobs (chain groups x blocks of 4 x 4 tile pairs: one launch holds them all). */
int64_t mcpc_cov_workspace_bytes(int32_t B, const int32_t* widths, int32_t n_blocks, int32_t pool);
int mcpc_cov_accumulate(int device, const float* const* rec, const int32_t* widths, const int32_t* transforms, int32_t n_blocks,
                        int32_t B, int32_t first, int32_t stride, int32_t n, int32_t pool, double* outer, int accumulate,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Streaming histograms of recorded steps: integer counts of g(r) per unit, the marginal distribution a Langevin call is looked at
 * through (the reference bins recorded trajectories with plt.hist(..., bins=np.linspace(lo, hi, k)): figure_2.py, figure_3.py,
 * figure_4.py, figure_6.py); quantiles, credible intervals and densities follow from the counts (csrc/mcpc_hist.h).
 * rec is a record buffer as mcpc_run writes it, [records][B][width] fp32; records first + k*stride, k = 0..n-1, are taken, exactly as
 * in mcpc_moments_accumulate; transform is MCPC_MOM_IDENTITY or MCPC_MOM_SIGMOID.  edges is a HOST pointer to n_bins + 1 fp32 values,
 * finite and strictly ascending, 1 <= n_bins <= MCPC_HIST_MAX_BINS; the library validates it before any device work and hands the table
 * to the kernel by value in the launch arguments (at most 1028 B).  counts is int64 device memory with n_bins + 3 columns per row: the
 * bins, then under, over, nan.
 *   pool = 0:  counts [B][width][n_bins + 3], one row per chain and unit
 *   pool = 1:  counts [width][n_bins + 3], summed over the chains
 * A bin is decided by exact fp32 comparison against the edges; no arithmetic on the value decides it.  With v = g(r):
 *   NaN                                  -> column n_bins + 2
 *   v < edges[0] (-inf included)         -> column n_bins      (under)
 *   v > edges[n_bins] (+inf included)    -> column n_bins + 1  (over)
 *   otherwise                            -> the largest i <= n_bins - 1 with edges[i] <= v: half-open bins, the last one closed at
 *                                           edges[n_bins]
 * which is np.histogram(v.astype(float64), bins=edges.astype(float64)).  Denormals are compared as they are (with an edge at 0.0 the
 * value -1e-42 is under it) and -0.0 compares equal to 0.0: the kernel compares order-preserving integer keys of the bit patterns.
 * accumulate = 0 overwrites counts, whatever they held; accumulate != 0 adds.  Counts are integers: the result is exact, and it depends
 * neither on the launch shape nor on how the caller chunks the records (37 records in one call, or 1 + 5 + 31 with accumulate = 1, give
 * equal counts).  The counters of a workgroup live in LDS for the length of the call and reach counts once; workgroups that share a
 * row of counts (pool = 1, or a record axis split over workgroups when B * width alone cannot fill the chip) add into it with 64-bit
 * integer atomics, and an overwriting call zeroes counts first on the same stream.  Nothing outside counts is written.
 * The library allocates nothing and copies nothing.  Stateless, asynchronous on `stream`, no engine needed, all offsets 64-bit.
 * 16-B loads per lane when B * width % 4 == 0 and the first record taken is 16-B aligned; a scalar form otherwise.
 * n = 0 reads nothing: it zeroes counts when accumulate = 0 and does nothing otherwise.
 * MCPC_EINVAL, checked before any HIP call (nothing is launched then): counts or edges NULL, rec NULL with n > 0, B < 1, width < 1,
 * stride < 1, first < 0, n < 0, n_bins outside 1..MCPC_HIST_MAX_BINS, pool not 0 or 1, an unknown transform, edges not finite or not
 * strictly ascending. */
#define MCPC_HIST_MAX_BINS 256
int mcpc_hist_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n,
                         int32_t transform, const float* edges, int32_t n_bins, int32_t pool, int64_t* counts, int accumulate,
                         void* stream);

/* Streaming JOINT histograms of recorded steps: integer counts of pairs of columns of one or two record rings, the joint density a sum
 * or a marginal cannot show (two modes of a posterior, the banana of a ReLU pair; the reference bins the class-plane projection of a
 * probe in 2-D: figure_2.py, posterior_non_linear_model).  csrc/mcpc_hist2d.h.
 * rec_x and rec_y are record buffers as mcpc_run writes them (or derived records: mcpc_probe_records, mcpc_prediction_errors),
 * [records][B][width_x] and [records][B][width_y] fp32; they may be the same pointer.  Records first + k*stride, k = 0..n-1, are taken of
 * both.  pairs is a HOST pointer to n_pairs x 2 int32 column indices, a column of rec_x then a column of rec_y; a column may repeat, and a
 * pair may name one column of one record twice.  edges_x and edges_y are HOST pointers to nx + 1 and ny + 1 fp32 values, finite and
 * strictly ascending.  Pairs and edges are validated before any device work and reach the kernel by value in the launch arguments
 * (2.2 KiB).  transform_x / transform_y are MCPC_MOM_IDENTITY or MCPC_MOM_SIGMOID, per axis.
 * Each axis is classified exactly as mcpc_hist_accumulate classifies a value (order-preserving keys, NaN by its bits, -0.0 as +0.0, the
 * last bin closed, +-inf in over / under): class 0..n-1 the bins, then under, over, nan.  counts is int64 device memory,
 *   pool = 0:  counts [B][n_pairs][nx + 3][ny + 3]
 *   pool = 1:  counts [n_pairs][nx + 3][ny + 3], summed over the chains
 * the row index the x class and the column index the y class.  Every (chain, pair) grid of a fresh call sums to n (n * B pooled), and a
 * marginal of a grid is what mcpc_hist_accumulate counts for that column with the same edges.
 * accumulate = 0 overwrites counts, accumulate != 0 adds.  Counts are integers: the result depends neither on the launch shape, nor on
 * how the caller chunks the records, nor on the order of pairs (a permuted list gives the permuted grids).  Counters live in LDS for the
 * length of a workgroup and reach counts once, by plain stores where a workgroup owns its grids and by 64-bit integer atomics
 * otherwise (an overwriting call zeroes counts first on the same stream).  Nothing outside counts is written; the library allocates
 * nothing.  Stateless, asynchronous on `stream`, no engine needed, all offsets 64-bit.
 * n = 0 reads nothing: it zeroes counts when accumulate = 0 and does nothing otherwise.
 * MCPC_EINVAL, checked before any HIP call: counts, pairs or an edge pointer NULL, rec_x or rec_y NULL with n > 0, B, width_x or width_y
 * < 1, stride < 1, first < 0, n < 0, n_pairs outside 1..MCPC_HIST2D_MAX_PAIRS, a column index out of range, nx or ny outside
 * 1..MCPC_HIST2D_MAX_BINS, more than MCPC_HIST2D_MAX_CELLS cells, pool not 0 or 1, an unknown transform, edges not finite or not
 * strictly ascending. */
#define MCPC_HIST2D_MAX_BINS  128      /* per axis */
#define MCPC_HIST2D_MAX_CELLS 12288    /* (nx + 3) * (ny + 3) at most: one grid's u32 counters stay in LDS (48 KiB) */
#define MCPC_HIST2D_MAX_PAIRS 128      /* per call */
int mcpc_hist2d_accumulate(int device, const float* rec_x, int32_t width_x, const float* rec_y, int32_t width_y, int32_t B,
                           int32_t first, int32_t stride, int32_t n, int32_t transform_x, int32_t transform_y,
                           const int32_t* pairs, int32_t n_pairs, const float* edges_x, int32_t nx, const float* edges_y, int32_t ny,
                           int32_t pool, int64_t* counts, int accumulate, void* stream);

/* Streaming lagged products of recorded steps: the raw material of the autocorrelation function, the integrated autocorrelation time
 * and the effective sample size of a Langevin call, whose samples are strongly autocorrelated (csrc/mcpc_acov.h).  The first reducer
 * whose result depends on the ORDER of the records and that carries state from call to call.
 * rec is a record buffer as mcpc_run writes it, [records][B][width] fp32; records first + j*stride, j = 0..n-1, are taken, exactly as
 * in mcpc_moments_accumulate, and are samples n_seen .. n_seen + n - 1 of a STREAM that earlier calls began; transform is
 * MCPC_MOM_IDENTITY or MCPC_MOM_SIGMOID (g).  With E = B * width, K = max_lag (0..MCPC_ACOV_MAX_LAG) and s_j the stream's samples, the
 * caller owns the state, all device memory:
 *   lagged  fp64 [E][K + 1]   lagged[e][k] = sum of g(s_j[e]) * g(s_{j-k}[e]) over every sample j so far with j - k >= 0
 *   sum     fp64 [E]          sum of g(s_j[e])
 *   window  fp32 [K][E]       window[k][e] = g of the sample k + 1 places back from the stream's end, valid for k < min(K, samples so
 *                             far); read when the call starts, rewritten when it ends: this is how a lag crosses a chunk boundary, and
 *                             g is computed once per sample
 *   head    fp32 [K][E]       g of the stream's samples 0..K-1, written by whichever call sees them
 * n_seen = 0 starts a stream: lagged and sum are overwritten whatever they held and nothing is read from window.  Slots of window and
 * head that are not valid yet are left as they are.  After the last call head, window (the tail), sum and lagged are what a centred
 * estimator needs: c_k = (lagged_k - m ((sum - tail_k) + (sum - head_k)) + (N - k) m^2) / N with m = sum / N and head_k / tail_k the sums of
 * the first / last k samples.  No second pass over the records is made.
 * One thread owns an element and walks the samples in ascending order with its K + 1 fp64 accumulators and the last K values in
 * registers: no atomics, no split of the record axis.  A product of two fp32 values is exact in fp64, so every accumulator is bitwise
 * the sequential host loop acc[k] += (double)g_j * (double)g_{j-k}, whatever the launch shape and however the caller chunks the stream
 * (37 samples in one call, or 1 + 5 + 31 with n_seen advancing, give the same bits).  A lag without a term yet (j < k) is skipped, not
 * multiplied by a zero: an Inf in sample 0 leaves the lags above the samples seen at exactly 0.
 * The library allocates nothing.  Asynchronous on `stream`, no engine needed, all offsets 64-bit.  With K = 0 window and head hold
 * nothing and may be NULL.  n = 0 reads nothing: it zeroes lagged and sum when n_seen = 0 and does nothing otherwise.
 * MCPC_EINVAL, checked before any HIP call (nothing is launched then): lagged, sum, window or head NULL (the latter two with K > 0), rec
 * NULL with n > 0, B < 1, width < 1, stride < 1, first < 0, n < 0, n_seen < 0, max_lag outside 0..MCPC_ACOV_MAX_LAG, an unknown
 * transform. */
#define MCPC_ACOV_MAX_LAG 64
int mcpc_acov_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n,
                         int32_t transform, int32_t max_lag, int64_t n_seen, double* lagged, double* sum, float* window, float* head,
                         void* stream);

/* Rolling-window variance of recorded steps: how the variability of a chain changes along a call and across the boundary of two calls
 * (csrc/mcpc_roll.h; the reference takes a pandas rolling(window).std() of recorded trajectories on the host: figure_5.py,
 * variability_stimulus_onset_nonlinear).  The first reducer that is resolved in time.
 * rec is a record buffer as mcpc_run writes it, [records][B][width] fp32; records first + j*stride, j = 0..n-1, are taken, exactly as
 * in mcpc_acov_accumulate, and are samples n_seen .. n_seen + n - 1 of a STREAM that earlier calls began; transform is
 * MCPC_MOM_IDENTITY or MCPC_MOM_SIGMOID (g).  With E = B * width and W = window (>= 2) the caller owns the state, all device memory:
 *   s1, s2  fp64 [E]      the sums of g and g * g over the last min(W, samples so far) samples
 *   hist    fp32 [W][E]   a circular buffer: g of sample j lives in row j mod W; the last min(W, samples so far) samples are valid
 * Per element, samples in ascending order:
 *   s1 = s1 + (double)g;  s2 = s2 + (double)g * (double)g;                          the entering sample j
 *   if (j >= W) { s1 = s1 - (double)o;  s2 = s2 - (double)o * (double)o; }          o = g of sample j - W
 *   if (j >= W - 1 && (j - (W - 1)) % every == 0)                                   a full window: stream row (j - (W - 1)) / every
 *       { m = s1 / W;  v = (s2 - s1 * m) / (W - 1);  v = v < 0 ? 0 : v; }           not contracted; NaN stays NaN
 * A product of two fp32 values is exact in fp64, so v is bitwise this loop on the host, whatever the launch shape and however the
 * caller chunks the stream (150 samples in one call, or 1 + 3 + (W - 1) + W + (W + 1) + the rest with n_seen advancing, give the same
 * bits in the state and in both outputs).  A window that is not full emits nothing.  The rows a call emits are numbered from 0 in the
 * call's outputs, in stream order; there are as many as samples j of the call satisfy the condition above (at most n).  Either output
 * may be NULL, not both:
 *   out_elem  fp64 [rows][E]   v, written by the thread that owns the element
 *   out_pool  fp64 [rows][4]   over the elements whose v is finite: sum of sd = sqrt(v), sum of sd * sd, sum of v, and their count.  Summed
 *             wave-first, then over the workgroups in ascending order through `workspace`; the association depends on E and on the
 *             vector width alone, so a pooled row does not depend on the chunking either.  An element that is not finite is left out
 *             and shows as a missing count; it never poisons a row.  Its own s1 and s2 stay non-finite for the rest of the stream.
 * The leaving sample comes from the chunk itself when it lies in it (read again, g recomputed) and from hist otherwise; hist is written
 * for the call's last min(n, W) samples.  n_seen = 0 starts a stream: s1 and s2 are overwritten whatever they held and nothing is read
 * from hist.  One thread owns an element and walks the samples in ascending order: no atomics, no split of the record axis.
 * workspace: device memory of mcpc_roll_workspace_bytes(B, width, n) bytes (8-B aligned, contents irrelevant, free for reuse when the
 * call has completed on `stream`); needed with out_pool only.  mcpc_roll_workspace_bytes returns -1 (and a message in mcpc_last_error)
 * for B < 1, width < 1 or n < 0.  The library allocates nothing.  Asynchronous on `stream`, no engine needed, all offsets 64-bit.  16-B
 * loads per lane when E % 4 == 0 and the first record taken and hist are 16-B aligned; a scalar form otherwise.  n = 0 reads nothing: it
 * zeroes s1 and s2 when n_seen = 0 and does nothing otherwise.
 * MCPC_EINVAL, checked before any HIP call (nothing is launched then): s1, s2 or hist NULL, out_elem and out_pool both NULL, window < 2,
 * every < 1, rec NULL with n > 0, B < 1, width < 1, stride < 1, first < 0, n < 0, n_seen < 0, an unknown transform, workspace NULL when
 * out_pool is set and the call emits a row. */
int mcpc_roll_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n,
                         int32_t transform, int32_t window, int32_t every, int64_t n_seen, double* s1, double* s2, float* hist,
                         double* out_elem, double* out_pool, void* workspace, void* stream);
int64_t mcpc_roll_workspace_bytes(int32_t B, int32_t width, int32_t n);

/* Streaming posterior of a linear probe on recorded steps: class probabilities of a linear read-out of a latent layer with a link, reduced
 * per chain over the samples of a Langevin call (csrc/mcpc_probe.h; the reference adds softmax(classifier(representation)) over the recorded
 * representations on the host: figure_2.py, comparison_ideal_observer).  The first reducer that applies a function the caller supplies.
 * rec is a record buffer as mcpc_run writes rec_x[l], [records][B][width] fp32; records first + j*stride, j = 0..n-1, are taken in ascending
 * order, exactly as in mcpc_moments_accumulate.  W is device fp32 [n_classes][width] row-major (nn.Linear.weight), bias device fp32
 * [n_classes] or NULL for zeros; C = n_classes in 1..MCPC_PROBE_MAX_CLASSES, width >= 1 without an upper limit.  For chain c, record j, class i:
 *   logit    z = (double)bias[i]; for k = 0..width-1 ascending z = z + (double)W[i][k] * (double)r_j[c][k]; v_i = (float)z.  A product of two
 *            fp32 values is exact in fp64, so v_i is bitwise the sequential fp64 loop on the host.
 *   link     MCPC_PROBE_IDENTITY p_i = v_i;  MCPC_PROBE_SIGMOID p_i = sigmoid_f(v_i), the library's own, as MCPC_MOM_SIGMOID;
 *            MCPC_PROBE_SOFTMAX m = max_i v_i, e_i = expf(v_i - m), S = sum_i e_i in fp32 in one fixed order that depends on C alone (a
 *            binary tree over C rounded up to a power of two), p_i = e_i / S (the math library's expf, IEEE division).
 *   psum     [B][C] fp64     psum[c][i]   = (accumulate ? psum[c][i]   : 0) + sum_j (double)p_i        in ascending j
 *   psumsq   [B][C] fp64     psumsq[c][i] = (accumulate ? psumsq[c][i] : 0) + sum_j (double)p_i * (double)p_i      (may be NULL)
 *   votes    [B][C + 1] int64  column i < C counts the samples whose largest logit is v_i, the lowest index on a tie (np.argmax); column C
 *            counts the samples with a NaN among their logits, which cast no vote: a row adds up to the samples taken
 *   entsum   [B] fp64        entsum[c] += (double)H_j, H_j = logf(S) - sum_i p_i (v_i - m) in fp32, the entropy of the sample's softmax;
 *            needed with MCPC_PROBE_SOFTMAX only, ignored (may be NULL) otherwise
 * With MCPC_PROBE_IDENTITY psum, psumsq and votes are bitwise the host loop; with the other links the logits and votes are, and a softmax
 * probability is within (C + 16) * 2^-24 of the fp64 softmax of the same fp32 logits.  NaN and Inf propagate by IEEE into the sums of the
 * chain that holds them, and nowhere else.  accumulate = 0 overwrites every output, whatever it held; accumulate != 0 adds.
 * Every (chain, class) accumulator has one owner, which walks the samples in ascending order: no atomics, no split of the record axis, no
 * float sum ordered by scheduling, so the result depends neither on the launch shape nor on how the caller chunks the records (37 records
 * in one call, or 1 + 5 + 31 with accumulate = 1, give the same bits).  The library allocates nothing.  Stateless, asynchronous on
 * `stream`, no engine needed, all offsets 64-bit.  n = 0 reads nothing: it zeroes the outputs when accumulate = 0 and does nothing otherwise.
 * MCPC_EINVAL, checked before any HIP call (nothing is launched then): W, psum or votes NULL, entsum NULL with MCPC_PROBE_SOFTMAX, rec NULL
 * with n > 0, B < 1, width < 1, stride < 1, first < 0, n < 0, n_classes outside 1..MCPC_PROBE_MAX_CLASSES, an unknown link. */
#define MCPC_PROBE_MAX_CLASSES 64
#define MCPC_PROBE_IDENTITY 0
#define MCPC_PROBE_SIGMOID  1
#define MCPC_PROBE_SOFTMAX  2
int mcpc_probe_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n,
                          const float* W, const float* bias, int32_t n_classes, int32_t link, double* psum, double* psumsq,
                          int64_t* votes, double* entsum, int accumulate, void* stream);

/* The probe as a derived record: the link values mcpc_probe_accumulate forms, written out instead of summed.  out is fp32 device
 * memory [n][B][n_classes], contiguous; row k belongs to record first + k*stride and out[k][c][i] is p_i of chain c, bitwise what the
 * accumulating entry adds for that sample (one kernel, csrc/mcpc_probe.h), NaN propagation included.  out has the layout of a record
 * buffer: every stateless reducer takes it as `rec` (mcpc_hist_accumulate, mcpc_hist2d_accumulate, mcpc_cov_accumulate, ...), and an
 * identity-link probe on it is a projection of the class probabilities.  Nothing is summed, so the records are dealt out over
 * workgroups.  Stateless, asynchronous on `stream`, no engine needed, all offsets 64-bit.  n = 0 writes nothing and needs no device.
 * MCPC_EINVAL, checked before any HIP call: W or out NULL, rec NULL with n > 0, B < 1, width < 1, stride < 1, first < 0, n < 0,
 * n_classes outside 1..MCPC_PROBE_MAX_CLASSES, an unknown link. */
int mcpc_probe_records(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n,
                       const float* W, const float* bias, int32_t n_classes, int32_t link, float* out, void* stream);

/* The k smallest squared distances from every query row into a reference set, by brute force on the device (csrc/mcpc_knn.h): the hot
 * path of the nearest-neighbour KL estimator between two sample clouds (the reference asks two scipy KD-trees: figure_5.py,
 * utils/training_evaluation.py KLdivergence).  q is device fp32 [nq][d], ref device fp32 [nr][d], both contiguous; d in
 * 1..MCPC_KNN_MAX_DIM, k in 1..MCPC_KNN_MAX_K, nq and nr in 0..MCPC_KNN_MAX_ROWS.  best is device fp32 [nq][k]:
 *   best[i][0..k) = the k smallest, ascending, of D(i, j) = sum_c (q[i][c] - ref[j][c])^2 over all j (and, with accumulate != 0, the k
 *                   values best[i] held before: the k best of old best and this call's distances)
 *   D             a = 0; for c = 0..d-1 ascending: t = q[i][c] - ref[j][c] in fp32, a = fmaf(t, t, a).  Not |q|^2 + |r|^2 - 2 q.r, which
 *                 cancels at near neighbours; within (d + 3) * 2^-24 relative of the exact distance of the same fp32 rows.
 *   selection     by fminf / fmaxf alone.  A NaN distance (a non-finite reference row) is never selected; a query row that holds a NaN
 *                 keeps +inf; a NaN in the old best reads as +inf.  accumulate = 0 starts every slot at +inf, whatever best held: with
 *                 nr < k the last k - nr slots stay +inf.  No row is skipped as "self": ask for k = 2 of a set into itself.
 * min and max are exact: best is bitwise independent of the launch shape, of the order of the reference rows and of how the caller chunks
 * ref over calls with accumulate = 1, so a reference set larger than memory can be streamed.
 * workspace: device memory of mcpc_knn_workspace_bytes(nq, nr, d, k) bytes (4-B aligned, contents irrelevant, free for reuse when the
 * call has completed on `stream`); the size depends on the four arguments alone.  mcpc_knn_workspace_bytes returns -1 (and a message in
 * mcpc_last_error) for arguments mcpc_knn_accumulate would refuse.  The library allocates nothing.  Stateless, asynchronous on `stream`
 * (a hipStream_t), no engine needed, all offsets 64-bit.  nq = 0 does nothing; nr = 0 fills best with +inf when accumulate = 0 and does
 * nothing otherwise.
 * MCPC_EINVAL, checked before any HIP call (nothing is launched then): d, k, nq or nr out of range, q or best NULL with nq > 0, ref NULL
 * with nr > 0, a workspace that is NULL or smaller than mcpc_knn_workspace_bytes when that is not 0. */
#define MCPC_KNN_MAX_DIM 32
#define MCPC_KNN_MAX_K 4
#define MCPC_KNN_MAX_ROWS 2147483647LL
int mcpc_knn_accumulate(int device, const float* q, int64_t nq, const float* ref, int64_t nr, int32_t d, int32_t k, float* best,
                        int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream);
int64_t mcpc_knn_workspace_bytes(int64_t nq, int64_t nr, int32_t d, int32_t k);

/* The importance-sampled log marginal likelihood of every datum from read-outs of prior samples, on the device (csrc/mcpc_loglik.h):
 * the hot path of the reference's get_marginal_likelihood (utils/training_evaluation.py), which forms one fp32 [batch][samples] matrix
 * per batch and keeps one scalar.  y is device fp32 [n_data][width], the data; out device fp32 [n_samp][width], the read-outs of the
 * samples (logits for MCPC_LOSS_BERNOULLI, means for MCPC_LOSS_GAUSSIAN); both contiguous; n_data and n_samp in
 * 0..MCPC_LOGLIK_MAX_ROWS, width >= 1.  With c = out clamped to [-clamp, +clamp] (clamp = +inf: none; the reference clamps to 20; a
 * NaN stays a NaN),
 *   Bernoulli  nll(i, s) = b_s - sum_j y_ij c_sj                                  b_s = sum_j softplus(c_sj)
 *   Gaussian   nll(i, s) = (0.5 / loss_var) (a_i + b_s - 2 sum_j y_ij c_sj) + 0.5 width log(2 pi loss_var)
 *                                                                                 a_i = sum_j y_ij^2, b_s = sum_j c_sj^2
 * state is device fp64 [n_data][4]:
 *   state[i] = { m, s1, s2, cnt }   m = min_s nll(i, s), s1 = sum_s e^-(nll - m), s2 = sum_s e^-2(nll - m), cnt = samples taken,
 * so that log p(y_i) ~ log(s1 / cnt) - m, and s1^2 / s2 is the effective sample size of the importance weights.  A state without
 * samples is the EMPTY state { +inf, 0, 0, 0 }.
 *   arithmetic    fp64 throughout; the dot products on the fp64 MFMA with the operands converted from fp32 on load, a_i and b_s summed
 *                 in one fixed order, softplus(c) = max(c, 0) + log1p(exp(-|c|)).
 *   merge rule    of two states A, B of the same datum over disjoint samples (also LogLikelihood.merge in Python): m = min(mA, mB); if
 *                 m = +inf the result is the empty state; else fA = exp(m - mA), fB = exp(m - mB), the factor of an empty state taken
 *                 as 0 (inf - inf is never formed), and s1 = s1A fA + s1B fB, s2 = s2A fA^2 + s2B fB^2, cnt = cntA + cntB.
 *                 accumulate != 0 merges the old state[i] with this call's; accumulate = 0 overwrites whatever state held.
 *   non-finite    a sample whose nll for a datum is not finite is neither taken nor counted for that datum and affects no other
 *                 (datum, sample) pair; a datum row that holds a NaN ends with cnt = 0.
 * What is bitwise: two runs of the same call (the launch shape depends on n_data and n_samp alone, every sum and merge has one fixed
 * order, no atomics).  What holds only within a bound: the same samples chunked differently over calls with accumulate = 1, and
 * another order of the samples -- the running minimum rescales the sums at other points.  With gamma = (width + 16) 2^-53 and
 * delta(i, s) = gamma (sum_j |y_ij c_sj| + b_s) (Gaussian: gamma (0.5 / loss_var) (a_i + b_s + 2 sum_j |y_ij c_sj|)), log(s1 / cnt) - m
 * stays within 4 max_s delta(i, s) + (n_samp + 64) 2^-52 of the exact value, and s1^2 / s2 within that, relative (tests/loglik_cases.py).
 * workspace: device memory of mcpc_loglik_workspace_bytes(n_data, n_samp, width) bytes (8-B aligned, contents irrelevant, free for reuse
 * when the call has completed on `stream`); the size depends on the three arguments alone.  mcpc_loglik_workspace_bytes returns -1 (and
 * a message in mcpc_last_error) for arguments mcpc_loglik_accumulate would refuse.  The library allocates nothing.  Stateless,
 * asynchronous on `stream` (a hipStream_t), no engine needed, all offsets 64-bit.  n_data = 0 does nothing; n_samp = 0 writes empty
 * states when accumulate = 0 and does nothing otherwise.
 * MCPC_EINVAL, checked before any HIP call (nothing is launched then): width < 1, n_data or n_samp out of range, MCPC_LOSS_NONE or an
 * unknown loss_kind, MCPC_LOSS_GAUSSIAN with loss_var <= 0, clamp <= 0 or NaN, y or state NULL with n_data > 0, out NULL with
 * n_samp > 0, a workspace that is NULL or smaller than mcpc_loglik_workspace_bytes when that is not 0. */
#define MCPC_LOGLIK_MAX_ROWS 2147483647LL
int mcpc_loglik_accumulate(int device, const float* y, int64_t n_data, const float* out, int64_t n_samp, int32_t width,
                           int32_t loss_kind, double loss_var, double clamp, double* state, int32_t accumulate, void* workspace,
                           int64_t workspace_bytes, void* stream);
int64_t mcpc_loglik_workspace_bytes(int64_t n_data, int64_t n_samp, int32_t width);

/* The log-weight increment of annealed importance sampling, on the device (csrc/mcpc_ais.h): what turns the Langevin kernels into an
 * estimate of the evidence.  x is device fp32 [rows][width], the last latent layer of `rows` chains (the layout of one record, or of
 * mcpc_store_state's last tensor); W fp32 [n_out][width] (torch layout), the UNSCALED read-out; bias [n_out] or NULL (zeros); y fp32
 * [rows][n_out], the target row of each chain; act an MCPC_ACT_*; logw device fp64 [rows].  All contiguous.  For every row r
 *   o_u     = bias_u + sum_k f(x_rk) W_uk                                                              u < n_out
 *   l(a)    = sum over u >= mask_start of   MCPC_LOSS_BERNOULLI: softplus(a o_u) - y_ru a o_u
 *                                           MCPC_LOSS_GAUSSIAN:  (0.5 / loss_var) (a o_u - y_ru)^2
 *   logw[r] = (accumulate ? logw[r] : 0) + c0 l(a0) - c1 l(a1)
 * so that with f_k(x) = p(x) exp(-loss_k(x)) one call adds log f_k(x) - log f_{k-1}(x): the Bernoulli ladder that scales the read-out
 * takes (a0, c0, a1, c1) = (beta_{k-1}, 1, beta_k, 1), the geometric Gaussian ladder (1, beta_{k-1}, 1, beta_k).  A side whose c is
 * exactly 0 is not evaluated and contributes exactly 0.  No normalising constant is added: the caller owns them.
 *   arithmetic    fp64 throughout: the contraction on the fp64 MFMA with the operands converted from fp32 on load, f (ReLU, tanh,
 *                 identity) and the loss terms in fp64, softplus(z) = max(z, 0) + log1p(exp(-|z|)); every sum has one fixed order.
 *   independence  a row's result depends on that row, W, bias and the scalars alone: not on `rows`, on the other rows or on the launch
 *                 shape.  Two runs of the same call are bitwise equal.  No atomics, no workspace, nothing is allocated.
 *   non-finite    a NaN or Inf stays in its own row.
 * Against exact arithmetic a result stays within 2^-40 M_r, M_r = sum_u [ c0 |term0_u| + c1 |term1_u| + (|c0 a0 dl0/do_u| +
 * |c1 a1 dl1/do_u|) (|bias_u| + sum_k |f(x_rk) W_uk|) ] (tests/ais_cases.py derives it).
 * Stateless, asynchronous on `stream` (a hipStream_t), no engine needed, all offsets 64-bit.  rows = 0 launches nothing.
 * MCPC_EINVAL, checked before any HIP call (nothing is launched then): width < 1, n_out < 1, rows outside 0..MCPC_AIS_MAX_ROWS,
 * mask_start outside 0..n_out-1, an unknown act or loss_kind or MCPC_LOSS_NONE, MCPC_LOSS_GAUSSIAN with loss_var <= 0, a NaN scalar
 * (loss_var, a0, c0, a1, c1), x, W, y or logw NULL with rows > 0. */
#define MCPC_AIS_MAX_ROWS 2147483647LL
int mcpc_ais_increment(int device, const float* x, int64_t rows, int32_t width, int32_t act, const float* W, const float* bias,
                       int32_t n_out, const float* y, int32_t loss_kind, double loss_var, int32_t mask_start, double a0, double c0,
                       double a1, double c1, double* logw, int32_t accumulate, void* stream);

/* The per-chain arithmetic of a Metropolis-adjusted Langevin step (MALA; csrc/mcpc_mala.h): a Langevin proposal followed by a
 * Metropolis-Hastings decision leaves its target p(x) ~ exp(-F(x)) exactly invariant at any step size, where the unadjusted step of
 * mcpc_run does so only as lr -> 0.  The gradient g = dF/dx and the energy E = F come from the engine (mcpc_run with update_x = 0 and
 * xgrad set; the last column of mcpc_chain_energies); these two entries see them as arrays.  A STATE is n_layers contiguous fp32
 * tensors [rows][widths[l]], 1 <= n_layers <= MCPC_MAX_LATENT, handed over as a host array of device pointers and a host array of
 * widths (the layout of mcpc_store_state).  Row r is the chain with the global id chain_base + r.
 *
 * mcpc_mala_propose: x_out_l = (x_l - lr g_l) + s xi_l per element, in fp32, with lr and s = sqrt(noise_var * lr) rounded to fp32 as
 * mcpc_run rounds them and xi_l the normals of (seed, step, layer l, chain_base + r): what mcpc_philox_normals returns and a fused
 * Langevin step at the same (seed, step) consumes.  Four roundings, none contracted: fl(lr g), fl(x - .), fl(s xi), fl(. + .).
 * x_out must not overlap x or g.
 *
 * mcpc_mala_accept, per chain r, with (x, g, E) the current state and (x_prop, g_prop, E_prop) the proposal of `step` and what the
 * engine evaluated at it:
 *   log_alpha = E[r] - E_prop[r] - ( sum_l |x_l - x'_l + lr g'_l|^2  -  sum_l |x'_l - x_l + lr g_l|^2 ) / (2 noise_var lr)
 *   u         = ((w >> 8) + 1) * 2^-24,   w = word 0 of philox4x32_10(chain_base + r, (0xFF << 24) | 0, step lo, step hi; key seed)
 *   accept    = log(u) < log_alpha                                      (fp64; a NaN log_alpha rejects)
 * The second term is the log-ratio of the proposal densities, so any noise_var > 0 is valid, not only 2.  Layer index 0xFF lies outside
 * every layer the normals and mcpc_sample_prior use: no Philox word is consumed twice.
 *   arithmetic    fp64 from the fp32 inputs, every operation rounded separately, in one fixed order that holds the chain's own values
 *                 only (csrc/mcpc_mala.h spells it out): a row's result does not depend on `rows` or on the other rows, and two runs
 *                 are bitwise equal.  No atomics, no workspace, nothing is allocated.
 *   in place      an accepted chain's rows of x, g and E are overwritten with those of x_prop, g_prop and E_prop; a rejected chain
 *                 keeps its bits (it is not written).  A step thus costs ONE gradient and ONE energy evaluation, at the proposal.
 *   non-finite    a NaN or Inf stays in its own chain; a chain whose log_alpha is NaN rejects.
 *   optional      diag fp64 [rows][3] = (log_alpha, u, accepted as 0 / 1); n_accepted int32 [rows], incremented by 1 for an accepted
 *                 chain; x_next, a state: the proposal of step + 1 from the selected (x, g), bitwise what mcpc_mala_propose would
 *                 write (it saves a launch per step).  Each may be NULL.  x_next must not overlap any other argument.
 * Against exact arithmetic log_alpha stays within 2^-41 M_r, M_r = |E| + |E'| + sum_u [(|x - x'| + lr |g'|)^2 + (|x' - x| + lr |g|)^2] /
 * (2 noise_var lr), for up to 2038 units per chain (tests/mala_cases.py derives it).
 * Both: stateless, asynchronous on `stream` (a hipStream_t), no engine needed, all offsets 64-bit, nothing is read or written beyond
 * rows x widths[l].  rows = 0 launches nothing.  MCPC_EINVAL, checked before any HIP call (nothing is launched then): n_layers outside
 * 1..MCPC_MAX_LATENT, rows outside 0..MCPC_MALA_MAX_ROWS, lr or noise_var not positive and finite, widths NULL or a width < 1, and
 * with rows > 0 a NULL state array or a NULL tensor in it (x_next only when given), E or E_prop NULL. */
#define MCPC_MALA_MAX_ROWS 2147483647LL
int mcpc_mala_propose(int device, const float* const* x, const float* const* g, const int32_t* widths, int32_t n_layers, int64_t rows,
                      double lr, double noise_var, uint64_t seed, uint64_t step, uint64_t chain_base, float* const* x_out,
                      void* stream);
int mcpc_mala_accept(int device, float* const* x, float* const* g, double* E, const float* const* x_prop, const float* const* g_prop,
                     const double* E_prop, const int32_t* widths, int32_t n_layers, int64_t rows, double lr, double noise_var,
                     uint64_t seed, uint64_t step, uint64_t chain_base, double* diag, int32_t* n_accepted, float* const* x_next,
                     void* stream);

/* The per-chain arithmetic of a Hamiltonian Monte Carlo transition of L leapfrog steps (csrc/mcpc_hmc.h): one directed trajectory of
 * the unit-mass Hamiltonian H(x, p) = F(x) + |p|^2 / 2 with ONE Metropolis decision at its end, in place of L random-walk MALA steps
 * (Duane et al. 1987; Neal 2011).  States, gradients, energies, widths and chain ids are those of the MALA entries above.  The step
 * size is eps = sqrt(2 lr): the host forms eps = (float)sqrt(2.0 * lr) in double and rounds it once, h = 0.5f * eps is exact.  L = 1
 * in this parameterisation is the MALA proposal and decision at noise_var = 2.  All fp32 element arithmetic is rounded operation by
 * operation, none contracted into an fma.  A trajectory from (x, g, E) at `step`:
 *
 * mcpc_hmc_begin, once:        p = xi                    q_out = fl(p - fl(h g))          x_out = fl(x + fl(eps q_out))
 *                              K0[r] = 0.5 * sum_u (double)p_u (double)p_u
 *   with xi the normals of (seed, step, layer l, chain_base + r): the very normals mcpc_mala_propose takes.  q_out, x_out and K0 must
 *   not overlap x or g.
 * mcpc_hmc_leap, L - 1 times:  q = fl(q - fl(eps g_t))   x_t = fl(x_t + fl(eps q))        in place, g_t the gradient at x_t as it
 *   stands before the call.  No random numbers; step, seed and chain_base are not taken.
 * mcpc_hmc_accept, once, with g_t and E_t the gradient and the energy at the trajectory's end x_t:
 *                              p' = fl(q - fl(h g_t))    K1 = 0.5 * sum_u (double)p'_u (double)p'_u
 *   log_alpha = (E[r] - E_t[r]) + (K0[r] - K1)                          (two differences and one sum, each rounded)
 *   u         = ((w >> 8) + 1) * 2^-24,   w = word 0 of philox4x32_10(chain_base + r, (0xFD << 24) | 0, step lo, step hi; key seed)
 *   accept    = log(u) < log_alpha                                      (fp64; a NaN log_alpha rejects)
 *   Layer index 0xFD is unused elsewhere: the normals and mcpc_sample_prior take 0 .. MCPC_MAX_LATENT, mcpc_smc_ancestors 0xFE and
 *   mcpc_mala_accept 0xFF, so no Philox word is consumed twice.
 *   sums          each lane of the chain's wave adds its squares in ascending order (layers, groups of four units, units of a group),
 *                 the 64 lanes are summed by the xor butterfly 32..1, exactly as mcpc_mala_accept sums, then one product by 0.5.  A
 *                 row's result depends on that row alone and two runs are bitwise equal.  No atomics, no LDS, no workspace.
 *   in place      an accepted chain's rows of x, g and E are overwritten with those of x_t, g_t and E_t; a rejected chain keeps its
 *                 bits (it is not written).  x_t, g_t, q and K0 are never written.  A transition thus costs L gradient evaluations and
 *                 ONE energy evaluation, at the end point.
 *   non-finite    a NaN or Inf stays in its own chain; a chain whose log_alpha is NaN rejects.
 *   optional      diag fp64 [rows][3] = (log_alpha, u, accepted as 0 / 1); n_accepted int32 [rows], incremented by 1 for an accepted
 *                 chain.  Each may be NULL.
 * Against exact arithmetic on the same fp32 p, p' the device's and a fp64 restatement's K0 and log_alpha differ by at most 2^-41 K0 and
 * 2^-41 M_r, M_r = |E| + |E_t| + K0 + K1, for up to 2038 units per chain: the squares are exact, a sum of N of them in any order errs
 * by at most (N - 1) 2^-53 of itself, and three more roundings form log_alpha (tests/hmc_cases.py derives it).
 * All three: stateless, asynchronous on `stream` (a hipStream_t), no engine needed, all offsets 64-bit, nothing is read or written
 * beyond rows x widths[l].  rows = 0 launches nothing.  MCPC_EINVAL, checked before any HIP call (nothing is launched then): n_layers
 * outside 1..MCPC_MAX_LATENT, rows outside 0..MCPC_HMC_MAX_ROWS, lr not positive and finite, widths NULL or a width < 1, and with
 * rows > 0 a NULL state array or a NULL tensor in it, E, E_t or K0 NULL. */
#define MCPC_HMC_MAX_ROWS 2147483647LL
int mcpc_hmc_begin(int device, const float* const* x, const float* const* g, const int32_t* widths, int32_t n_layers, int64_t rows,
                   double lr, uint64_t seed, uint64_t step, uint64_t chain_base, float* const* q_out, float* const* x_out, double* K0,
                   void* stream);
int mcpc_hmc_leap(int device, float* const* x_t, float* const* q, const float* const* g_t, const int32_t* widths, int32_t n_layers,
                  int64_t rows, double lr, void* stream);
int mcpc_hmc_accept(int device, float* const* x, float* const* g, double* E, const float* const* x_t, const float* const* g_t,
                    const double* E_t, const float* const* q, const double* K0, const int32_t* widths, int32_t n_layers, int64_t rows,
                    double lr, uint64_t seed, uint64_t step, uint64_t chain_base, double* diag, int32_t* n_accepted, void* stream);

/* Resampling the replicas of annealed importance sampling (csrc/mcpc_smc.h): between two rungs, a datum whose R weights have
 * degenerated draws R ancestors among its own replicas, which turns AIS into a sequential Monte Carlo sampler (Del Moral, Doucet &
 * Jasra 2006).  Datum i owns rows i R .. i R + R - 1 (R = replicas); row r is the chain with the global id chain_base + r.
 *
 * mcpc_smc_ancestors, per datum i, in fp64, every operation rounded separately and nothing contracted into an fma:
 *   ok_j = isfinite(logw_j), cnt = #ok, m = max_ok logw_j;    e_j = ok_j ? exp(logw_j - m) : 0
 *   c_j = c_{j-1} + e_j,  q_j = q_{j-1} + e_j e_j             in replica order, sequentially (one lane walks them: np.cumsum)
 *   S = c_{R-1},  ess = (S S) / q_{R-1};                       resample = ess < threshold * (double)R   (a NaN does not resample)
 *   u = (w >> 8) * 2^-24 + 2^-25,   w = word 0 of philox4x32_10(chain_base + i R, (0xFE << 24) | 0, step lo, step hi; key seed)
 *   p_s = (((double)s + u) / (double)R) S,   a_s = #{j : c_j <= p_s} clamped to the last j with e_j > 0       (systematic resampling)
 *   ancestors[i R + s] = i R + a_s,   logw[i R + s] = m + log(S / cnt) for all R slots: the log of the mean weight over the finite
 *   replicas.  u is exact and inside (0, 1).  Layer index 0xFE lies outside every layer the normals (0 .. MCPC_MAX_LATENT - 1),
 *   mcpc_sample_prior (0 .. MCPC_MAX_LATENT) and mcpc_mala_accept (0xFF) use: no Philox word is consumed twice.
 *   not resampled a datum with ess >= threshold R, or with cnt = 0 (its ess is NaN), gets identity ancestors and its logw is NOT written.
 *   independence  a datum's result depends on its own R log-weights, threshold, seed, step and chain_base + i R alone: not on
 *                 n_data, the other data or the launch shape; two runs are bitwise equal.  No atomics, no workspace.
 *   non-finite    a NaN or Inf log-weight has weight 0: it is never an ancestor and never leaves its datum.
 *   optional      diag fp64 [n_data][4] = (ess, resampled as 0 / 1, u, m + log(S / cnt)); with cnt = 0: (NaN, 0, u, NaN).  May be NULL.
 *   One workgroup per datum, replicas doubles of LDS (32 KiB at the cap).  0 <= threshold <= 1: 0 never resamples, 1 always does
 *   unless the weights are exactly equal (ess = R is not below R).
 *   MCPC_EINVAL, checked before any HIP call: replicas outside 1..MCPC_SMC_MAX_REPLICAS, n_data < 0 or n_data * replicas above
 *   MCPC_SMC_MAX_ROWS, threshold outside [0, 1] or NaN, and with n_data > 0 logw or ancestors NULL.  n_data = 0 launches nothing.
 *
 * mcpc_smc_gather, out of place: x_out_l[r] = x_l[ancestors[r]], bitwise, for every layer l of a STATE (as the MALA entries take it:
 * host arrays of device pointers and of widths) in one launch, one wave per destination row.  An index outside 0 .. rows - 1 is
 * never dereferenced: that row copies itself and, when n_bad (one int32 on the device) is given, n_bad is incremented by 1 for it --
 * the counter exists for exactly this purpose.  x_out must not overlap x.  Nothing is read or written beyond rows x widths[l].
 *   MCPC_EINVAL, checked before any HIP call: n_layers outside 1..MCPC_MAX_LATENT, rows outside 0..MCPC_SMC_MAX_ROWS, widths NULL or
 *   a width < 1, and with rows > 0 a NULL state array or a NULL tensor in it, ancestors NULL.  rows = 0 launches nothing.
 * Both: stateless, asynchronous on `stream` (a hipStream_t), no engine needed, all offsets 64-bit. */
#define MCPC_SMC_MAX_REPLICAS 4096
#define MCPC_SMC_MAX_ROWS 2147483647LL
int mcpc_smc_ancestors(int device, double* logw, int64_t n_data, int32_t replicas, double threshold, uint64_t seed, uint64_t step,
                       uint64_t chain_base, int32_t* ancestors, double* diag, void* stream);
int mcpc_smc_gather(int device, const float* const* x, const int32_t* widths, int32_t n_layers, int64_t rows, const int32_t* ancestors,
                    float* const* x_out, int32_t* n_bad, void* stream);

/* Per-chain energies of recorded states, evaluated on the device (the reference has them per datapoint: is_return_batchelement_loss,
 * PCLayer(is_keep_energy_per_datapoint=True), get_energies(is_per_datapoint=True); pc_trainer.py:776-836, pc_layer.py:250-262).
 * A ROW is one chain at one recorded step.  x_rec[l], l < n_latent: [n_rec][batch][n_l] fp32, as mcpc_run writes rec_x[l] (n_rec = 1
 * with plain [batch][n_l] states evaluates a current state).  For row r = k * batch + chain the library forms the forward pass
 * mu_j = f(x_{j-1}) W_j^T + b_j on the engine's packed weights -- the step kernels' own GEMM and per-element arithmetic: a prediction is
 * bitwise theirs -- with mu_1 from `inputs` ([batch][n_in], NULL = zeros; the inputs bound with mcpc_bind_inputs are not consulted) and the
 * target row of the chain as bound with mcpc_bind_target, and writes
 *   out[r][0] = the read-out loss of the row (loss_kind / loss_var / mask_start as in mcpc_run_desc; 0 for MCPC_LOSS_NONE),
 *   out[r][1 + l] = E_{l+1} = c_l * 0.5 * |x_l - mu_l|^2 (unused columns 0),   out[r][MCPC_MAX_LATENT + 1] = their sum plus the loss.
 * Summed over the chains of record k this is the row mcpc_run writes into energies_out for the step that recorded k.
 * Every sum has one fixed order that holds the row's own values only (fp32 over the four units a lane holds and the unit tiles of its
 * wave, fp64 from there: lanes, waves, unit-tile jobs, layers): a row's result does not depend on the other rows, on n_rec, or on
 * max_rows.  The records are processed in chunks of max_rows rows (0 = default 16384; rounded up to a multiple of 64) through scratch
 * the engine allocates on the first call and enlarges when a later call asks for a longer chunk: 8 B per row and padded unit, plus 8 B
 * per row and 128-unit job.  The engine's state, sums and bound pointers are not touched.  Works on every engine form (the weight
 * fragments are the same).  Asynchronous on `stream` but for those allocations.
 * MCPC_EINVAL: null engine / x_rec / x_rec[l] / out, n_rec < 0, max_rows < 0, unknown loss_kind, a loss without a read-out, loss_var
 * <= 0, mask_start outside 0..n_out-1.  MCPC_ESTATE: parameters not bound, a loss without a bound target.  Nothing is launched then. */
int mcpc_chain_energies(mcpc_engine* e, const float* inputs, const float* const* x_rec, int32_t n_rec, int32_t loss_kind,
                        double loss_var, int32_t mask_start, double* out, int32_t max_rows, void* stream);

/* Prediction errors and predictions of recorded states, per unit: the other half of a predictive-coding network's population, as
 * DERIVED RECORDS.  Rows, x_rec, `inputs`, the target, loss_kind / loss_var / mask_start, max_rows and the scratch are those of
 * mcpc_chain_energies (the scratch is shared), and so is the forward pass: a prediction is bitwise the step kernels' and bitwise the one
 * mcpc_chain_energies squares.  Per row r = k * batch + chain the call writes, where the destination is not NULL,
 *   err[l][r][u]  = x_l - mu_l (NOT scaled by the layer's ecoef),        pred[l][r][u] = mu_l            l < n_latent, u < n_l
 *   err_out[r][u] = the read-out error the step kernels back-propagate   pred_out[r][u] = the read-out's output (logits)    u < n_out
 *                   (dloss / dout; exactly 0 for u < mask_start),
 * each unpadded fp32 [n_rec][batch][n_l], the layout mcpc_run writes rec_x[l] / rec_out in: every stateless reducer of this header
 * (mcpc_moments_accumulate, mcpc_cov_accumulate, mcpc_hist_accumulate, mcpc_acov_accumulate, mcpc_roll_accumulate) takes them as `rec`.
 * err / pred: arrays of n_latent pointers; an entry that is NULL, or err / pred itself NULL, means "not wanted".  Only the Linears asked
 * for are evaluated (a call that wants layer 2 alone launches no GEMM for layers 0 and 1), and only the records they read are consulted:
 * x_rec[l] for a wanted layer l and for the layer below a wanted layer or read-out; the other entries of x_rec may be NULL.  loss_kind,
 * loss_var, mask_start and the bound target matter to err_out alone.  No sums, no atomics: a value depends on its own row only, not on
 * the other rows, n_rec, max_rows or on what else is asked for.  Nothing is written outside rows < n_rec * batch and units < n_l.
 * Destinations need 4-byte alignment; one that is 16-byte aligned with n_l % 4 == 0 is written with 16-byte stores.
 * MCPC_EINVAL: null engine / x_rec / a needed x_rec[l], n_rec < 0, max_rows < 0, nothing wanted at all, err_out or pred_out on an engine
 * without a read-out, unknown loss_kind, err_out with MCPC_LOSS_NONE, loss_var <= 0 or mask_start outside 0..n_out-1 with err_out.
 * MCPC_ESTATE: parameters of a wanted Linear not bound, err_out without a bound target.  Nothing is launched then. */
int mcpc_prediction_errors(mcpc_engine* e, const float* inputs, const float* const* x_rec, int32_t n_rec, int32_t loss_kind,
                           double loss_var, int32_t mask_start, float* const* err, float* const* pred, float* err_out, float* pred_out,
                           int32_t max_rows, void* stream);

/* Gradient of the free energy, and the energies, of handed-over states: what a sampler of the caller's own needs at a proposal (the score
 * dF/dx for saliency, MALA, HMC), without the state passing through the engine.  Rows, x, `inputs`, the target, loss_kind / loss_var /
 * mask_start, max_rows and the x / f(x) scratch are those of mcpc_chain_energies.  Per row r = k * batch + chain the call writes
 *   grad[l][r][u] = dF/dx_l = e_l - f'(x_l) (e_{l+1} W_{l+1})    e_l = c_l (x_l - mu_l), the read-out's error above the last layer
 * unpadded fp32 [n_rec][batch][n_l] -- bitwise what mcpc_run writes into xgrad (update_x = 0) on the layer-wise step kernels after
 * mcpc_load_state of the same state: the same operands, exponents, k order and per-element arithmetic -- and, when `energies` is not
 * NULL, energies[r][:] bitwise as mcpc_chain_energies writes it for the same rows.  The call adds one padded fp32 row per unit of
 * layers 1 .. and of the read-out to the evaluators' scratch (allocated on the first call, enlarged with the chunk).  A value depends on
 * its own row alone: not on the other rows, n_rec, max_rows or on whether the energies are asked for.  Nothing is written outside rows
 * < n_rec * batch and units < n_l.  Destinations need 4-byte alignment; one that is 16-byte aligned with n_l % 4 == 0 is written with
 * 16-byte stores.  The engine's state, Adam moments, sums, Philox position, records and bound pointers are not touched.
 * The stream rides in the descriptor (mcpc_run_desc is the precedent for a descriptor): every other entry point takes it as its last
 * parameter, and this one will too once its side-stream scenario has a row in the table those entry points are tested from.
 * MCPC_EINVAL, before any device work: null engine / descriptor / x / grad / x[l] / grad[l], n_rec < 0, max_rows < 0, and what
 * mcpc_chain_energies refuses of a loss.  MCPC_ESTATE: parameters not bound, a loss without a bound target.  n_rec = 0: MCPC_OK. */
typedef struct mcpc_gradient_desc {
    const float* inputs;        /* [batch][n_in] or NULL (zeros) */
    const float* const* x;      /* [n_latent]: states [n_rec][batch][n_l] */
    int32_t n_rec;
    int32_t loss_kind;
    double loss_var;
    int32_t mask_start;
    float* const* grad;         /* [n_latent]: dF/dx_l [n_rec][batch][n_l]; every entry required */
    double* energies;           /* NULL, or [n_rec * batch][MCPC_MAX_LATENT + 2] as mcpc_chain_energies writes it */
    int32_t max_rows;           /* rows per scratch chunk, 0 = default; no result depends on it */
    void* stream;               /* a hipStream_t */
} mcpc_gradient_desc;
int mcpc_state_gradients(mcpc_engine* e, const mcpc_gradient_desc* d);

/* Ancestral samples of the generative model, drawn on the device: x_1 ~ N(mu_1, 1/c_1), x_2 ~ N(mu_2(x_1), 1/c_2), ..., the read-out (the
 * reference's utils.training_evaluation.sample_pc, which draws on the CPU and runs nn.Linear in torch).  A ROW is one sample; row i has
 * the global id g = sample_base + i.  n is independent of the engine's batch, as the rows of mcpc_chain_energies are; rows are processed
 * in chunks of max_rows (0 = default 16384; rounded up to a multiple of 64) through the scratch of mcpc_chain_energies (shared).
 * Latent layer j = 0 .. n_latent - 1, in this order:
 *   mu_j = f(x_{j-1}) W_j^T + b_j   mu_0 from `inputs` ([n][n_in], NULL = zeros).  The step kernels' own GEMM on the engine's packed
 *                                   weights: bitwise what mcpc_prediction_errors writes as pred[j] for the same x_{j-1}.
 *   x_j  = mu_j + s_j * z           z = the engine's normals for (seed, step, layer j, chain (uint32)g, group u / 4): exactly what
 *                                   mcpc_philox_normals(device, seed, step, j, sample_base, n, n_j, ...) returns;
 *                                   s_j = (float)(1 / sqrt((double)ecoef_j)); s_j * z and the sum are two fp32 roundings (no fma).
 * The prior is the one the energy c * 0.5 (x - mu)^2 implies, variance 1 / c: what unclamped Langevin sampling converges to.  The
 * reference's sample_pc ignores a custom coefficient (mean + randn); with the default ecoef = 1 the two agree.  Padded units stay zero.
 * Read-out (n_out > 0): o = f(x_{L-1}) W_L^T + b_L, bitwise pred_out, written to `out` as
 *   MCPC_SAMPLE_HIDDEN   o (loss_kind and loss_var are not consulted)
 *   MCPC_SAMPLE_MEAN     MCPC_LOSS_BERNOULLI: sigmoid_f(o), the library's own (MCPC_MOM_SIGMOID);  MCPC_LOSS_GAUSSIAN: o
 *   MCPC_SAMPLE_DRAW     MCPC_LOSS_BERNOULLI: u < sigmoid_f(o) ? 1.f : 0.f with u = (r >> 8) * 2^-24, r the raw Philox word of (seed, step,
 *                        layer n_latent, g, unit): the raw != 0 stream of mcpc_philox_normals for layer n_latent;
 *                        MCPC_LOSS_GAUSSIAN: o + (float)sqrt(loss_var) * z, two roundings, z the normals of layer n_latent.
 * x_out: NULL, or n_latent pointers, each NULL or unpadded [n][n_j]; out: [n][n_out] or NULL -- the layout of a record: every stateless
 * reducer of this header takes them as `rec`.  Only the Linears below the last destination asked for are launched.  Destinations need
 * 4-byte alignment; one that is 16-byte aligned with a width that is a multiple of 4 is written with 16-byte stores.  Nothing is written
 * beyond row n or unit n_j.  A sample depends on (seed, step, g), the weights and its input row alone: not on n, max_rows, on how a
 * caller splits [sample_base, sample_base + n) over calls or devices, or on the engine's form.  The engine's state, sums and bound
 * pointers are untouched; no target is needed.  Asynchronous on `stream` but for the growth of the scratch.  n = 0 launches nothing.
 * MCPC_EINVAL, before any launch: null engine, n < 0, sample_base + n > 2^32 (the generator's chain word is 32 bits), max_rows < 0,
 * unknown readout or loss_kind, out on an engine without a read-out, out and every x_out[j] NULL, and for a wanted `out`: MEAN or DRAW
 * with MCPC_LOSS_NONE, DRAW / Gaussian with loss_var <= 0.  (An ecoef_j <= 0 never reaches the call: mcpc_create refuses it.)
 * MCPC_ESTATE: parameters of a Linear the call runs not bound. */
#define MCPC_SAMPLE_HIDDEN 0   /* the read-out as it is: logits / means (sample_pc(is_return_hidden=True)) */
#define MCPC_SAMPLE_MEAN   1   /* Bernoulli: sigmoid_f(o), the library's own; Gaussian: o */
#define MCPC_SAMPLE_DRAW   2   /* a draw from the sensory distribution */
int mcpc_sample_prior(mcpc_engine* e, const float* inputs, int64_t n, uint64_t seed, uint64_t step, uint64_t sample_base,
                      int32_t loss_kind, double loss_var, int32_t readout, float* const* x_out, float* out, int32_t max_rows,
                      void* stream);

/* Synchronise `stream` and report device-side faults of the runs issued so far (the wave-specialised step kernel
 * bounds every intra-workgroup wait; a wait that runs out is recorded instead of hanging the GPU).
 * Returns MCPC_ESTATE if the last results must not be used.  The only call besides create/destroy that
 * synchronises the whole stream on every call (mcpc_run's bounded waits: Threading, above). */
int mcpc_sync_check(mcpc_engine* e, void* stream);

/* Introspection for benchmarks / DESIGN.md: bytes of LDS per workgroup, chains per workgroup, workgroups of the shard (units
 * of `chains_per_wg` chains that hold at least one chain of the batch; a launch of the round schedule holds a part of them, see
 * mcpc_step_kernel_name), spill slots. */
int mcpc_query(const mcpc_engine* e, int32_t* lds_bytes, int32_t* chains_per_wg, int32_t* n_workgroups,
               int32_t* spill_slots);
/* Name of the step kernel this engine launches, as it appears in a rocprofv3 kernel trace (static string); an engine on the layer-wise
 * kernels names the pair of launches a step is, "mcpc::mcpc_lw_fwd_kernel + mcpc::mcpc_lw_bwd_kernel", and mcpc_query reports the forward
 * kernel's LDS bytes, its chain tile and the workgroups of one forward launch. */
const char* mcpc_step_kernel_name(const mcpc_engine* e);
/* What the last mcpc_run actually launched -- the engine's preference above is not always what serves a run (injected noise, gradients-only
 * runs and Adam with noise keep the main plan's kernel): the step kernel's name as above; a run that also ran a plain launch beside the round
 * schedule names both, joined by " + ".  Launches of the in-place kernel that took one of its specialised instantiations (a trace shows them
 * as mcpc::mcpc_steps_ws2_spec_kernel<...>) are named behind the form they belong to, as " [mcpc_steps_ws2_spec_kernel: hot, hot+spill]"; a
 * run on the generic instantiation alone carries no such tag.  "" before the first run.  Host bookkeeping only: no device work, no synchronisation.  The string
 * is valid until the next mcpc_run on this engine. */
const char* mcpc_last_step_kernel_name(const mcpc_engine* e);
/* What the last Hebbian flush of Linear j >= 1 launched (Linear 0's sums take mcpc_dw0_kernel at the end of every accumulating run):
 * one "<kernel><<TE>,<RA>[,T]>x<groups>[*<activation groups>]" per launch of the tiled kernels, joined by "+" (heb7: the fp16-piece form
 * mcpc_heb7_kernel, heb: the fp32-MFMA form mcpc_heb_kernel, T: operands swapped), or "dw tiles=<64 x 64 wave tiles>" for the streaming
 * mcpc_dw_kernel; then "ksplit=<K-splits> rps=<spilled rows per split>" and the spill layout, "tm" (tile-major) or "rm" (row-major).
 * E.g. "heb7<17,2>x1+heb7<16,2>x2 ksplit=12 rps=1536 tm".  "" for j = 0, out of range, or before the first flush.  Host bookkeeping
 * only; valid until the next mcpc_run on this engine. */
const char* mcpc_last_flush_plan(const mcpc_engine* e, int j);

/* Timing hooks.  While profiling is enabled (mcpc_set_profiling(e, 1); every call of it resets the tallies), mcpc_run
 * brackets every step-kernel launch with HIP events on its stream (a launch of the round schedule advances only the workgroups it
 * holds: it counts as steps x workgroups / all workgroups whole-shard steps).  The getter synchronises on the recorded events and
 * returns the summed time, the number of launches and the whole-shard steps they cover (rounded), accumulated over all runs since
 * profiling was enabled (at most 65 536 launches). */
int mcpc_set_profiling(mcpc_engine* e, int enable);
int mcpc_last_step_kernel_ms(mcpc_engine* e, float* ms, int32_t* n_launches, int64_t* n_steps);
/* The shader clock the chip held DURING the step-kernel launches bracketed since profiling was enabled: one wave of workgroup 0 of
 * every launch of the in-place kernel reads s_memtime (shader cycles) and s_memrealtime (100 MHz) at both ends of the launch; the
 * quotient of the sums is the clock under that load (MI355X lowers it under MFMA-dense work: 1.8-2.0 GHz against the 2.4 GHz peak).
 * 0 when no such launch has run.  Waits for the device. */
int mcpc_last_shader_clock_ghz(mcpc_engine* e, float* ghz);

/* Diagnostic (tests only; nothing of the product path calls it): fill the 160 KiB of LDS of EVERY compute unit of `device` with the
 * 32-bit pattern `word` (e.g. 0x7fa00000, a signalling NaN), then return once the fill has completed.  LDS is not cleared between
 * kernels on gfx950, so the next launch on each CU finds the pattern in whatever LDS it does not write itself.  Used by
 * tests/test_gpu_lds_poison.py to show that no result depends on LDS content the step kernels did not produce. */
int mcpc_debug_poison_lds(int device, uint32_t word, void* stream);

/* Diagnostic (tests only; no device work): the unit-tile jobs of the two launches a step of the layer-wise kernels is, for a network of
 * `n_latent` layers of `sizes[l]` units and a read-out of `n_out` (0: none).  Writes up to `cap` (layer, first 16-unit tile) pairs of the
 * forward launch into fwd (layer n_latent = the read-out) and of the backward launch into bwd, their counts into n_fwd / n_bwd (also when
 * they exceed cap), and into tile[0..1] the chains and the 16-unit tiles one workgroup covers.  gridDim.y of a launch walks the jobs,
 * gridDim.x the chain tiles. */
int mcpc_debug_lw_jobs(int32_t n_latent, const int32_t* sizes, int32_t n_out, int32_t* fwd, int32_t* bwd, int32_t cap,
                       int32_t* n_fwd, int32_t* n_bwd, int32_t* tile);

/* Diagnostic (tests only; no device work): the job table of mcpc_chain_energies for a network as in mcpc_debug_lw_jobs.  Writes up to
 * `cap` (Linear, first 16-unit tile) pairs into jobs (Linear n_latent = the read-out), their count into n_jobs (also when it exceeds
 * cap), into n_head how many of them, at the front, belong to the read-out (a call without a loss launches the rest only), and into
 * tile[0..1] the rows and the 16-unit tiles one workgroup covers.  The jobs of one Linear are contiguous, first tile ascending. */
int mcpc_debug_chain_energy_jobs(int32_t n_latent, const int32_t* sizes, int32_t n_out, int32_t* jobs, int32_t cap, int32_t* n_jobs,
                                 int32_t* n_head, int32_t* tile);

/* Diagnostic (tests only; no device work, no device needed): everything mcpc_create would decide for `desc` on a device of `n_cu` compute
 * units and `total_mem` bytes of memory (read only when desc->spill_budget_bytes <= 0; 0 = unknown), as one JSON object: "form"
 * (in-place | barrier | layer-wise), "kernel" (mcpc_step_kernel_name), "Bpad", "workgroups" and "chains_per_wg" (mcpc_query), "npad",
 * "out_pad", "slots" / "half_slots" of the spill ring, "spill_tm" per Linear, "slabs" per Linear as [float offset, floats, K-splits held]
 * of its split-K slabs and their total "slab_floats"; "main" and "unified"."plan", the LDS plan and step table
 * of the main form and of the unified-wave kernel ("unified" also says whether the plan fits, is held and is preferred): "lds_bytes",
 * "regions" as [name, layer | -1, float offset, floats], "xl", "chunk" / "ring" / "overlay" of the in-place plan, and "table", one row
 * of numbers per entry in the order "fields" names (every KPhase field but the weight pointer; the unified table holds "rows" rows of
 * "n_phases" entries, one per wave); "lw", the layer-wise job table (forward jobs, then backward jobs); "rounds", the round schedule
 * with the [unit, rel] pairs of every launch of a cycle.  desc->device is ignored.  Writes at most cap - 1 characters and a NUL into
 * out, and the size the whole text needs (NUL included) into *needed.  Fails as mcpc_create would: same codes, same messages. */
int mcpc_debug_plan(const mcpc_net_desc* desc, int32_t n_cu, int64_t total_mem, char* out, int64_t cap, int64_t* needed);

/* Diagnostic (tests only; no device work, no device needed): the schedule mcpc_run would issue for `run` on the engine mcpc_debug_plan
 * describes, as one JSON object.  Only the fields of `run` that shape the schedule are read -- T, t_begin, n_steps (checked as mcpc_run
 * checks them), acc_begin, acc_end, update_x, xopt_kind, noise_mode, loss_kind -- and its pointers may be null.  "unified": the run is
 * served by the unified-wave kernel; "accumulates": a step of it lies in the accumulation window; "lean_ok"; "overlap": its Hebbian
 * flushes run beside the next segment, through a spill ring of "n_parts" parts, else serially; "items", one row of numbers per item in
 * the order "fields" names: steps [t0, t0 + n) as one plain launch (q = 0) or as one cycle of the round schedule (rr_k launches of q
 * steps, n = rr_m q), "acc" when they lie in the window -- then the item spills into slots [slot0, slot0 + n) of the ring, part "part",
 * and "flush" says that a flush of those n slots follows it; "flushes", one entry per flushing item, the flush as mcpc_run has planned
 * it before it launches anything: "rows" = n x Bpad; "lin", per Linear j >= 1 in the order "flush_fields" names, the K-splits and rows
 * per split of that flush and the bound of the splits that sizes the Linear's slabs (that of a flush of a whole ring part);
 * "launches", per Linear j >= 1 its launches in launch order, each a row in the order "launch_fields" names: "family" ("heb7", "heb" or
 * "dw": mcpc_heb7_kernel, mcpc_heb_kernel, mcpc_dw_kernel), "form" (the index of the tiled kernels' instantiation <te, ra, swapped> in
 * the list csrc/mcpc_hebbian.h holds, MCPC_HEB_FORMS; -1 for "dw"), the grid "n_mt" x "n_nt" x K-splits, "col0" (the first output
 * column), "stream" (0 or 1: which of the flush's streams; all 0 unless "two_streams") and "wave_tiles" ("dw" only); "reduce", per
 * Linear j >= 1 in the order "reduce_fields" names, the sign its sums enter the gradient with and the transposed dimensions of its
 * weight slab (0, 0: not transposed); "max_blocks", gridDim.x of the one reduction launch; "text", per Linear j >= 1 what
 * mcpc_last_flush_plan returns after that flush.  out / cap / needed and the failures as for mcpc_debug_plan. */
int mcpc_debug_run_plan(const mcpc_net_desc* desc, int32_t n_cu, int64_t total_mem, const mcpc_run_desc* run, char* out, int64_t cap,
                        int64_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* MCPC_H */
