// Body of a workgroup of the in-place wave-specialised step kernel: included as the body of mcpc_steps_ws2_kernel (WS2_BLOCK =
// blockIdx.x: the kernels of the plain schedule compile exactly as they did as stand-alone kernels) and twice inside
// mcpc_steps_ws2_mixed_kernel (one block per workgroup form).  Expects: CTT (always 1), MIX, P, lds, WS2_BLOCK, WS2_NBLOCKS, and WS2_MODE: the
// launch's compile-time mode (mcpc_ws2_lean.h: Ws2Mode) -- a field other than kModeDyn replaces the run-time test below by its value.
    using M = WS2_MODE;
    constexpr int NW = kWs2Pairs, NTW = kWs2NTW;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_g = wave8 < kWs2Pairs;                   // waves 0..NW-1 and NW..2NW-1 both spread evenly over the 4 SIMDs
    const int k = wave8 & (kWs2Pairs - 1);                 // pair id
    const int c = lane & 15, q = lane >> 4;
    const int unit = MIX ? P.wg_list[WS2_BLOCK] : (int)WS2_BLOCK;             // the workgroup's MFMA column tile of 16 chains
    const int chain0 = unit * 16;
    // first step of this unit in this launch (round schedule: a unit takes part in m of the k launches of a cycle and carries the
    // number it has already run)
    const int t_first = MIX ? P.t0 + P.wg_rel[WS2_BLOCK] * P.rr_q : P.t0;
    const int L = P.L;
    const int n_ent = P.n_phases;
    Ws2Sync* sync = reinterpret_cast<Ws2Sync*>(lds + P.lds_ws_sync);
    int dead = 0;                                          // set once a bounded wait of this wave ran out
    // every float of the plan starts a launch as zero (row tails and padding columns are never written afterwards)
    for (int i = tid; i < P.lds_floats / 4; i += kWs2Threads) st4(lds + 4 * i, splat(0.f));
    __syncthreads();
    if (tid < 2 * kWs2Pairs) reinterpret_cast<int*>(sync)[tid] = 0;
    const int upd_mode = M::UPD != kModeDyn ? (M::UPD == WS2_UPD_SGD_PHILOX ? 2 : (M::UPD == WS2_UPD_SGD ? 1 : 0))
                         : (P.update_x && P.xopt == MCPC_XOPT_SGD)
                             ? (P.noise_mode == MCPC_NOISE_PHILOX ? 2 : (P.noise_mode == MCPC_NOISE_NONE ? 1 : 0)) : 0;
    // lean epilogues (mcpc_ws2_lean.h): fused SGD update (or Adam without noise: the MAP warm-up), every chain of the
    // workgroup inside the batch, 32-bit offsets fit
    const bool lean_adam = M::UPD != kModeDyn ? M::UPD == WS2_UPD_ADAM : P.update_x && P.xopt == MCPC_XOPT_ADAM && P.noise_mode == MCPC_NOISE_NONE;
    const bool lean = M::UPD != kModeDyn || ((upd_mode != 0 || lean_adam) && chain0 < P.B && P.lean_ok);       // (padding chains of a last workgroup: LeanLane::livem)
    // the lean epilogues of a plan with the room keep the state (and what else they read every step) in LDS for the whole launch
    const bool xl = M::XL != kModeDyn ? M::XL != 0 : lean && P.xl != 0;
    // lean epilogues keep the exponent of every B row they write (mcpc_kernels.h: rowexp_track): the GEMM waves then scan no row
#ifdef MCPC_EXP_NOLEAN
    const bool rowexp = false;
#else
    const bool rowexp = M::ROWEXP != kModeDyn ? M::ROWEXP != 0 : lean;
#endif
    float* const rx = rowexp ? lds + P.lds_rowexp : nullptr;
    // f(x_l) of the state the launch starts from; afterwards the x updates keep FX_l current
    for (int l = 0; l < L; ++l) {
        const KLayer& Ly = P.layer[l];
        if (M::act(Ly.act) == MCPC_ACT_RELU) ws2_fill_fx<MCPC_ACT_RELU>(Ly, lds, chain0, tid, xl, rx, rowexp_fx(l));
        else if (M::act(Ly.act) == MCPC_ACT_TANH) ws2_fill_fx<MCPC_ACT_TANH>(Ly, lds, chain0, tid, xl, rx, rowexp_fx(l));
        else ws2_fill_fx<MCPC_ACT_IDENTITY>(Ly, lds, chain0, tid, xl, rx, rowexp_fx(l));
    }
    if (xl) ws2_fill_constants(P, lds, chain0, tid);
    __syncthreads();                                       // the only barrier

    if (is_g) {
        // =========================== G: fragments + MFMAs ==============================================
        if (P.ws_prio == 2) __builtin_amdgcn_s_setprio(2);
        // Loop-carried: the descriptor of the upcoming entry and the first two k-blocks of its fragments.  The GEMM
        // moves pre0/pre1 into its own register sets first thing, so the ONE prefetch site below refills the same
        // variables -- with separate "next" copies hipcc put `s_waitcnt vmcnt(0)` + 16 v_mov at the loop latch, i.e.
        // every entry waited out the L2 round trip of the prefetch it had just issued.
        // The GEMM waves visit only the entries they have work in (KPhase::next_g, KParams::g_first): a table round -- descriptor,
        // next-entry requests, progress counter -- for FWD_0, the energy entry or an x update without a back-projection bought nothing.
        int p = P.g_first;
        if (p < 0) return;                     // (no GEMM anywhere: a single latent layer without a read-out)
        const bool y_bounded = M::HEAD != kModeDyn ? M::HEAD == WS2_HEAD_BERNOULLI_BITS : P.has_head && *P.head.y_bounded != 0;      // (headb_fixed_exp: the bound target lies in [-1, 2])
        KPhase ph_next = load_phase(P.phases, p);
        int nt_next, aoff[NTW];
        frag_t pre0[NTW];
#pragma unroll
        for (int i = 0; i < NTW; ++i) { pre0[i] = frag_zero(); aoff[i] = 0; }
        ws2_prefetch<!M::generic>(ph_next, k, lane, P.dummy, nt_next, aoff, pre0);
        STAMP_DECL
#ifdef MCPC_STAMPS
        const unsigned long long clk_m0 = mcpc_stamp(), clk_r0 = wall_clock64();
#endif
        for (int s = 0; s < P.n_steps; ++s) {
            const int base = s * n_ent;
            f32x4 accb[NTW];                       // back-projection of the read-out error: 16 tiles over the pairs
#pragma unroll
            for (int i = 0; i < NTW; ++i) accb[i] = splat(0.f);
            int accb_run = kRunNone, accb_aexp = 0;      // the units accb is in (mcpc_gemm_f16.h: GemmScale); per lane = per chain
#pragma unroll 1
            for (;;) {
                const KPhase ph = ph_next;
                const int nt = nt_next;
                const int p_next = ph.next_g;
                const bool wraps = p_next <= p;                                     // the next entry with work belongs to the next step
                const bool has_next = !wraps || (s + 1 < P.n_steps);
                if (has_next) ph_next = load_phase(P.phases, p_next);
                const bool handoff = (ph.flags & PHF_WS2_HANDOFF) != 0;             // accb goes to the partner
                const bool is_headb = ph.type == PH_HEADB;
                const bool works = true;                                            // (only such entries are visited)
                const bool stores = !is_headb;
                f32x4 acc[NTW];
#pragma unroll
                for (int i = 0; i < NTW; ++i) acc[i] = splat(0.f);
                STAMP(0);
#ifdef MCPC_STAMPS_ENTRY
                const unsigned long long ge0 = mcpc_stamp();
                unsigned long long gwait = 0;
#endif
                if (works) {
                    if (ph.dep_e >= 0) ws2_wait_all(sync->prog_e, ws2_need(base, n_ent, p, ph.dep_e), P.err, dead);
#ifdef MCPC_STAMPS_ENTRY
                    gwait = mcpc_stamp() - ge0;
#endif
                    STAMP(1);
                    if (is_headb) {
                        if (nt > 0 MCPC_EXP_GEMM_GATE) {
                            // the chunks of the read-out add up in accb, in scaled units
                            const int hb_exp = headb_fixed_exp(M::loss_kind(P.head), y_bounded);        // (wave-uniform: a constant for a bounded read-out error)
                            const bool hb_word = hb_exp == kScaleAuto && rowexp && ph.b_row >= 0;
                            const int fixed_b = hb_word ? rowexp_read(rx, ph.b_row, c) : hb_exp;
                            GemmScale gs{load_wexp(P.wexp, ph.a_lin), GS_ACCUM, fixed_b, accb_run,
                                         P.head.npad <= kShortK * kKB ? 1 : 0, (hb_exp == kScaleAuto && !hb_word) ? 1 : 0};
                            gemm_tiles<NTW, NW, !M::generic>(accb, ph.A, aoff, nt, ph.nkb, ph.kw, lds + ph.b_lds, ph.ldb, lane, pre0, lds + P.lds_zero, gs);
                            accb_run = gs.run; accb_aexp = gs.a_exp;
                        }
                        STAMP(2);
                    } else {
                        if (handoff) {
#pragma unroll
                            for (int i = 0; i < NTW; ++i) acc[i] = accb[i];     // one entry covers all of accb
                            if (accb_run != kRunNone) gemm_unscale<NTW>(acc, accb_aexp, accb_run);      // (the hand-off entry has no GEMM of its own)
                        }
                        if (nt > 0 && ph.nkb > 0 MCPC_EXP_GEMM_GATE) {
                            // the row's exponent: from its producers' word (lean epilogues), else scanned by gemm_tiles
                            // (nothing branches on the word: its LDS round trip runs beside that of the first B block inside gemm_tiles)
                            const bool has_word = rowexp && ph.b_row >= 0;
                            const int fixed_b = has_word ? rowexp_read(rx, ph.b_row, c) : kScaleAuto;
                            GemmScale gs{load_wexp(P.wexp, ph.a_lin), GS_FRESH, fixed_b, kRunNone, -1, has_word ? 0 : 1};
                            gemm_tiles<NTW, NW, !M::generic>(acc, ph.A, aoff, nt, ph.nkb, ph.kw, lds + ph.b_lds, ph.ldb, lane, pre0, lds + P.lds_zero, gs);
                        }
                        STAMP(3);
                    }
                }
                // the one prefetch site: fragments of the next entry travel while this block is handed over
                ws2_prefetch<!M::generic>(ph_next, k, lane, P.dummy, nt_next, aoff, pre0);   // (past the last entry: the old descriptor again)
                STAMP(4);
                if (stores) {
                    // write-after-read: the rows this block goes to may still be read by GEMMs (dep_g) or epilogues (dep_se)
                    // of entries that share them -- waited for here, behind the GEMM, not in front of it
#ifdef MCPC_STAMPS_ENTRY
                    const unsigned long long gw0 = mcpc_stamp();
#endif
                    if (ph.dep_g >= 0) ws2_wait_all(sync->prog_g, ws2_need(base, n_ent, p, ph.dep_g), P.err, dead);
                    if (ph.dep_se >= 0) ws2_wait_all(sync->prog_e, ws2_need(base, n_ent, p, ph.dep_se), P.err, dead);
#ifdef MCPC_STAMPS_ENTRY
                    gwait += mcpc_stamp() - gw0;
#endif
                    // the block goes where its consumer reads it; E_k finishes it in place
                    const int kk = (k + ph.rot) & (NW - 1);
                    int ntw = (ph.ntiles - kk + NW - 1) / NW;
                    ntw = ntw < 0 ? 0 : (ntw > NTW ? NTW : ntw);
                    float* const out = lds + ph.out_lds;
                    const int col0 = (ph.type == PH_HEADF) ? 0 : 16 * ph.tile0;
#pragma unroll
                    for (int i = 0; i < NTW; ++i) {
                        if (i >= ntw) continue;
                        const int col = col0 + 16 * (kk + NW * i) + 4 * q;
                        st4(out + c * ph.out_ld + col, acc[i]);
                    }
                }
                if (lane == 0) ws_publish(&sync->prog_g[k], base + p + 1);
                STAMP(5);
#ifdef MCPC_STAMPS_ENTRY
                if (MCPC_STAMPS_ENTRY == 1) STAMP_ENTRY_ADD(p, gwait);
                else if (MCPC_STAMPS_ENTRY == 2) STAMP_ENTRY_ADD(p, mcpc_stamp() - ge0);
#endif
                p = p_next;
                if (wraps) break;
            }
        }
#if defined(MCPC_STAMPS) && !defined(MCPC_STAMPS_ENTRY)
        st_sum[6] = mcpc_stamp() - clk_m0;          // whole launch in s_memtime ticks ...
        st_sum[7] = wall_clock64() - clk_r0;        // ... and in 100 MHz wall-clock ticks: their ratio is the shader clock
#endif
#ifdef MCPC_STAMPS
        if (lane == 0 && P.dbg != nullptr)      // (null in the warm-up launch of setup_mixed_schedule)
            for (int i = 0; i < 16; ++i) P.dbg[((size_t)WS2_BLOCK * (2 * kWs2Pairs) + wave8) * 16 + i] = st_sum[i];
#endif
        return;
    }

    // =============================== E: epilogues ===========================================================
    if (P.ws_prio == 1) __builtin_amdgcn_s_setprio(2);
    // profiling: the shader clock the chip holds under this launch, from one wave of workgroup 0 (two scalar clock reads at each end
    // of the launch; the values go to a buffer nothing else reads)
    const bool clk_wave = P.clk != nullptr && WS2_BLOCK == 0 && k == 0;
    unsigned long long clk_c0 = 0, clk_w0 = 0;
    if (clk_wave) { clk_c0 = __builtin_amdgcn_s_memtime(); clk_w0 = __builtin_amdgcn_s_memrealtime(); }
    LeanLane LL;
    LL.c = c; LL.q = q;
    // (CTT is 1.  The one-trip `ct` loops left in this body and in the epilogues are the ones without which the compiled kernels change:
    // profiles/ctt_removal_asm.txt)
#pragma unroll
    for (int ct = 0; ct < CTT; ++ct) {
        LL.chain = (uint32_t)(chain0 + 16 * ct + c); LL.lrow = (uint32_t)(16 * ct + c);
        const bool live = chain0 + 16 * ct + c < P.B;
        LL.livem = live ? ~0u : 0u;
    }
    // 0/1 targets are read bit-packed (a wave-uniform flag the library set when the target was bound)
    const bool ybin = M::HEAD != kModeDyn ? M::HEAD == WS2_HEAD_BERNOULLI_BITS : lean && P.has_head && *P.head.y_binary != 0;
    // sum_t e_1 of this launch in registers (lean path, top layer of at most one tile per wave, rot == 0 for FWD entries)
    const bool e0_in_regs = lean && P.layer[0].ntiles <= NW;
    bool e0_dirty = false;
    f32x4 e0acc;
#pragma unroll
    for (int ct = 0; ct < CTT; ++ct) e0acc = splat(0.f);
    if (e0_in_regs && (M::SPILL != kModeDyn ? M::SPILL != WS2_SPILL_OFF : t_first + P.n_steps > P.acc_begin && t_first < P.acc_end)) lean_load_e0(P, k, LL, e0acc);   // (a launch that accumulates)
    STAMP_DECL
    for (int s = 0; s < P.n_steps; ++s) {
        const int t = t_first + s;
        const int s_tab = MIX ? t - P.t0 : s;          // index into per-step tables (Adam coefficients, external noise): they start at P.t0
        const int base = s * n_ent;
        const bool do_energy = (P.energy_mode == MCPC_ENERGY_ALL) || (P.energy_mode == MCPC_ENERGY_LAST && t == P.T - 1);
        // (a specialised launch lies on one side of the accumulation window with every step: ws2_select_mode)
        const int slot = M::SPILL == WS2_SPILL_OFF ? -1 : (M::SPILL != kModeDyn || (t >= P.acc_begin && t < P.acc_end)) ? (t - P.spill_t0) : -1;
        int rec_idx = -1;
        if (P.rec_count > 0 && t >= P.rec_begin) {
            const int kk = (t - P.rec_begin) / P.rec_stride;
            if (kk < P.rec_count && P.rec_begin + kk * P.rec_stride == t) rec_idx = kk;
        }
        // energies of this step: lane c of every E wave carries the wave's partial sum of column c (layers 0..5, loss) in a
        // register; the LDS scratch is written once per step, at the ENERGY entry (an LDS read-modify-write behind every
        // epilogue cost the E waves seven LDS round trips per step)
        float* red = lds + P.lds_red + (s & 1) * (kMaxLatent + 1) * kMaxWaves;
        float en_acc = 0.f;
#pragma unroll 1
        for (int p = 0; p < n_ent; ++p) {
            const KPhase ph = load_phase(P.phases, p);
#ifdef MCPC_STAMPS_ENTRY
            const unsigned long long ee0 = mcpc_stamp();
            unsigned long long ewait = 0;
#endif
            if (ph.type == PH_ENERGY) {
                if (do_energy && lane <= kMaxLatent) red[lane * kMaxWaves + k] = en_acc;
                if (lane == 0) ws_publish(&sync->prog_e[k], base + p + 1);
                if (do_energy && k == 0) {
                    // every E wave has written its partial sums of this step
                    ws2_wait_all(sync->prog_e + 0, base + p + 1, P.err, dead);
                    if (lane <= kMaxLatent) {
                        double v = 0.0;
                        const bool used = (lane < L) || (lane == kMaxLatent && P.has_head);
                        if (used) {
#pragma unroll
                            for (int w = 0; w < kWs2Pairs; ++w) v += (double)red[lane * kMaxWaves + w];
                        }
                        const int erow = (P.energy_mode == MCPC_ENERGY_ALL) ? t : 0;
                        // a row has one slot per 16-chain tile, and a workgroup is one such tile: every slot has exactly one writer
                        double* const ep = P.epart + ((size_t)erow * P.epart_slots + (size_t)unit) * (kMaxLatent + 1) + lane;
                        ep[0] = v;
                    }
                }
                continue;
            }
            if (!(ph.flags & PHF_WS_EPI)) {
                if (lane == 0) ws_publish(&sync->prog_e[k], base + p + 1);
                continue;
            }
            const int kk = (k + ph.rot) & (NW - 1);
            int nt = (ph.ntiles - kk + NW - 1) / NW;
            nt = nt < 0 ? 0 : (nt > NTW ? NTW : nt);
#ifndef MCPC_EXP_NOLEAN
            if (lean) {
                const int act = M::act(P.layer[ph.layer].act);
                const int* const pg = &sync->prog_g[k];
                const int need = base + p + 1;
#ifdef MCPC_STAMPS_ENTRY       // (diagnostic build: the wait for the partner's block apart from the epilogue's own time)
                if (((ph.flags & PHF_WS_GEMM) && ph.nkb > 0) || (ph.flags & PHF_WS2_HANDOFF)) {
                    const unsigned long long ew0 = mcpc_stamp();
                    ws_wait_one(pg, need, P.err, dead);
                    ewait = mcpc_stamp() - ew0;
                }
#endif
#ifdef MCPC_EXP_NOEPI
                if (P.n_steps < 0)
#endif
                if (ph.type == PH_FWD) {
                    float esum;
                    if (ph.layer == 0 && M::spills(slot)) e0_dirty = true;
                    // (two `if`s here and a `done` flag in the read-out entry, not if / else: the generic kernel compiles to other code with the
                    // plain form, like the one-trip `ct` loops that are left -- profiles/ctt_removal_asm.txt)
                    if (xl) {
                        if (act == MCPC_ACT_RELU) esum = lean_fwd<CTT, NW, NTW, MCPC_ACT_RELU, true, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, pg, need, P.err, dead, e0acc, e0_in_regs, rx, (unsigned)(s + 1));
                        else if (act == MCPC_ACT_TANH) esum = lean_fwd<CTT, NW, NTW, MCPC_ACT_TANH, true, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, pg, need, P.err, dead, e0acc, e0_in_regs, rx, (unsigned)(s + 1));
                        else esum = lean_fwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, true, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, pg, need, P.err, dead, e0acc, e0_in_regs, rx, (unsigned)(s + 1));
                    }
                    if (!xl) {
                    if (act == MCPC_ACT_RELU) esum = lean_fwd<CTT, NW, NTW, MCPC_ACT_RELU, false, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, pg, need, P.err, dead, e0acc, e0_in_regs, rx, (unsigned)(s + 1));
                    else if (act == MCPC_ACT_TANH) esum = lean_fwd<CTT, NW, NTW, MCPC_ACT_TANH, false, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, pg, need, P.err, dead, e0acc, e0_in_regs, rx, (unsigned)(s + 1));
                    else esum = lean_fwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, false, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, pg, need, P.err, dead, e0acc, e0_in_regs, rx, (unsigned)(s + 1));
                    }
                    if (do_energy) { esum = wave_sum(esum); if (lane == ph.layer) en_acc += esum; }
                } else if (ph.type == PH_HEADF) {
                    float lsum;
                    bool done = false;
                    if (xl) {
                        if (ybin) lsum = lean_headf<CTT, NW, NTW, true, true, false, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, do_energy, pg, need, P.err, dead, true, rx);
                        else lsum = lean_headf<CTT, NW, NTW, true, false, false, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, do_energy, pg, need, P.err, dead, false, rx);
                        done = true;
                    }
                    if (!done) lsum = lean_headf<CTT, NW, NTW, false, false, false, false, M>(P, ph, lds, nt, kk, LL, slot, rec_idx, do_energy, pg, need, P.err, dead, ybin, rx);
                    if (do_energy) { lsum = wave_sum(lsum); if (lane == kMaxLatent) en_acc += lsum; }
                } else if (ph.type == PH_BWD) {
                    if (xl) {
                        if (lean_adam) {
                            if (act == MCPC_ACT_RELU) lean_bwd<CTT, NW, NTW, MCPC_ACT_RELU, false, true, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, s_tab, rx, (unsigned)(s + 1));
                            else if (act == MCPC_ACT_TANH) lean_bwd<CTT, NW, NTW, MCPC_ACT_TANH, false, true, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, s_tab, rx, (unsigned)(s + 1));
                            else lean_bwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, false, true, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, s_tab, rx, (unsigned)(s + 1));
                        } else if (upd_mode == 2) {
                            if (act == MCPC_ACT_RELU) lean_bwd<CTT, NW, NTW, MCPC_ACT_RELU, true, false, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                            else if (act == MCPC_ACT_TANH) lean_bwd<CTT, NW, NTW, MCPC_ACT_TANH, true, false, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                            else lean_bwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, true, false, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                        } else {
                            if (act == MCPC_ACT_RELU) lean_bwd<CTT, NW, NTW, MCPC_ACT_RELU, false, false, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                            else if (act == MCPC_ACT_TANH) lean_bwd<CTT, NW, NTW, MCPC_ACT_TANH, false, false, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                            else lean_bwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, false, false, true, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                        }
                    } else if (lean_adam) {
                        if (act == MCPC_ACT_RELU) lean_bwd<CTT, NW, NTW, MCPC_ACT_RELU, false, true, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, s_tab, rx, (unsigned)(s + 1));
                        else if (act == MCPC_ACT_TANH) lean_bwd<CTT, NW, NTW, MCPC_ACT_TANH, false, true, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, s_tab, rx, (unsigned)(s + 1));
                        else lean_bwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, false, true, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, s_tab, rx, (unsigned)(s + 1));
                    } else if (upd_mode == 2) {
                        if (act == MCPC_ACT_RELU) lean_bwd<CTT, NW, NTW, MCPC_ACT_RELU, true, false, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                        else if (act == MCPC_ACT_TANH) lean_bwd<CTT, NW, NTW, MCPC_ACT_TANH, true, false, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                        else lean_bwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, true, false, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                    } else {
                        if (act == MCPC_ACT_RELU) lean_bwd<CTT, NW, NTW, MCPC_ACT_RELU, false, false, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                        else if (act == MCPC_ACT_TANH) lean_bwd<CTT, NW, NTW, MCPC_ACT_TANH, false, false, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                        else lean_bwd<CTT, NW, NTW, MCPC_ACT_IDENTITY, false, false, false, false, M>(P, ph, lds, nt, kk, LL, t, pg, need, P.err, dead, 0, rx, (unsigned)(s + 1));
                    }
                }
                if (lane == 0) ws_publish(&sync->prog_e[k], base + p + 1);
#ifdef MCPC_STAMPS_ENTRY
                if (MCPC_STAMPS_ENTRY == 3) STAMP_ENTRY_ADD(p, ewait);
                else if (MCPC_STAMPS_ENTRY == 4) STAMP_ENTRY_ADD(p, mcpc_stamp() - ee0);
#endif
                continue;
            }
#endif
            f32x4 acc[NTW], pa[NTW], pb[NTW];
#pragma unroll
            for (int i = 0; i < NTW; ++i) { acc[i] = splat(0.f); pa[i] = splat(0.f); pb[i] = splat(0.f); }
            const KLayer& Ly = P.layer[ph.layer];
            STAMP(8);
            // operands of the epilogue travel while the partner still computes
            issue_epilogue_loads<CTT, NW, NTW>(P, ph, lds, nt, kk, lane, chain0, pa, pb);
            STAMP(9);
            const bool from_g = ((ph.flags & PHF_WS_GEMM) && ph.nkb > 0) || (ph.flags & PHF_WS2_HANDOFF);
            if (from_g) {
#ifdef MCPC_STAMPS_ENTRY
                const unsigned long long ew0 = mcpc_stamp();
#endif
                ws_wait_one(&sync->prog_g[k], base + p + 1, P.err, dead);
#ifdef MCPC_STAMPS_ENTRY
                ewait = mcpc_stamp() - ew0;
#endif
                STAMP(10);
                const float* const src = lds + ph.out_lds;
                const int col0 = (ph.type == PH_HEADF) ? 0 : 16 * ph.tile0;
#pragma unroll
                for (int i = 0; i < NTW; ++i) {
                    const int col = col0 + 16 * (kk + NW * (i < nt ? i : 0)) + 4 * q;     // unused slots re-read slot 0
#pragma unroll
                    for (int ct = 0; ct < CTT; ++ct) acc[i] = ld4(src + (16 * ct + c) * ph.out_ld + col);
                }
            }
#ifdef MCPC_EXP_NOEPI   // timing experiment only (wrong results): E waves skip the epilogue arithmetic and stores
            if (P.n_steps < 0)
#endif
            if (ph.type == PH_FWD) {
                float esum;
                if (Ly.act == MCPC_ACT_RELU) esum = fwd_epilogue<CTT, NW, NTW, MCPC_ACT_RELU, false>(P, ph, lds, nt, kk, lane, chain0, acc, pa, pb, slot, rec_idx);
                else if (Ly.act == MCPC_ACT_TANH) esum = fwd_epilogue<CTT, NW, NTW, MCPC_ACT_TANH, false>(P, ph, lds, nt, kk, lane, chain0, acc, pa, pb, slot, rec_idx);
                else esum = fwd_epilogue<CTT, NW, NTW, MCPC_ACT_IDENTITY, false>(P, ph, lds, nt, kk, lane, chain0, acc, pa, pb, slot, rec_idx);
                if (do_energy) { esum = wave_sum(esum); if (lane == ph.layer) en_acc += esum; }
            } else if (ph.type == PH_HEADF) {
                float lsum = ws2_headf_epilogue<CTT, NW, NTW>(P, ph, lds, nt, kk, lane, chain0, acc, pa, pb, slot, rec_idx, do_energy);
                if (do_energy) { lsum = wave_sum(lsum); if (lane == kMaxLatent) en_acc += lsum; }
            } else if (ph.type == PH_BWD) {
                if (Ly.act == MCPC_ACT_RELU) bwd_epilogue_mode<CTT, NW, NTW, MCPC_ACT_RELU, true>(P, ph, nt, kk, lane, chain0, acc, pa, pb, s_tab, t, upd_mode, lds);
                else if (Ly.act == MCPC_ACT_TANH) bwd_epilogue_mode<CTT, NW, NTW, MCPC_ACT_TANH, true>(P, ph, nt, kk, lane, chain0, acc, pa, pb, s_tab, t, upd_mode, lds);
                else bwd_epilogue_mode<CTT, NW, NTW, MCPC_ACT_IDENTITY, true>(P, ph, nt, kk, lane, chain0, acc, pa, pb, s_tab, t, upd_mode, lds);
            }
            if (lane == 0) ws_publish(&sync->prog_e[k], base + p + 1);
            if (ph.type == PH_FWD) STAMP(11); else if (ph.type == PH_HEADF) STAMP(12); else STAMP(13);
#ifdef MCPC_STAMPS_ENTRY
            if (MCPC_STAMPS_ENTRY == 3) STAMP_ENTRY_ADD(p, ewait);
            else if (MCPC_STAMPS_ENTRY == 4) STAMP_ENTRY_ADD(p, mcpc_stamp() - ee0);
#endif
        }
    }
    if (xl) lean_store_x<CTT, NW>(P, lds, k, LL);              // the state of this wave's tiles goes back to global memory
    if constexpr (M::SPILL != WS2_SPILL_OFF) spill_max_publish(P.spillmax, lds + P.lds_spillmax, lane);  // what this workgroup spilled at most, per tensor (every E wave, when it is through)
    if (clk_wave && lane == 0) {
        atomicAdd(P.clk, __builtin_amdgcn_s_memtime() - clk_c0);
        atomicAdd(P.clk + 1, __builtin_amdgcn_s_memrealtime() - clk_w0);
    }
    if (e0_in_regs && e0_dirty) lean_flush_e0(P, k, LL, e0acc);      // (FWD entries have rot == 0: this wave's tile is k)
#ifdef MCPC_STAMPS
    if (lane == 0 && P.dbg != nullptr)
        for (int i = 0; i < 16; ++i) P.dbg[((size_t)WS2_BLOCK * 8 + wave8) * 16 + i] = st_sum[i];
#endif
