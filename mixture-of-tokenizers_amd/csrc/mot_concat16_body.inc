// mot_concat16_body.inc -- the workgroup program of the concat + linear gather-GEMM (see mot_concat16.hip, which includes this text
// once per kernel: in concat16_gemm_kernel, whose arguments arrive as the kernel parameter `P`, and in concat16_slots_kernel, which
// fills `P` for its slot first).  Expects the template parameters MT, NT, NS, NH, RES and `const C16Args P` in scope.
    constexpr int BM = 64 * MT, BN = 128 * NT, WMR = 32 * MT, WNR = 32 * NT, PD = NS - 1;
    constexpr int kStageB = BN * 64, kStageA = BM * 64, kDma = BN * 4 / kC16Threads;
    static_assert(PD == 1 || PD == 2, "one or two steps ahead");
    extern __shared__ __attribute__((aligned(16))) char lds_c[];
    char *sA = lds_c + NS * kStageB;
    uint16_t *sIds = (uint16_t *)(sA + kStageA);                                  // [BM * bpt]
    float *sRn = (float *)(lds_c + NS * kStageB + kStageA + ((BM * P.bpt * 2 + 15) & ~15));   // [byte_rows] rms factors of the byte rows (1 when that part is not normalised)
    float *sSS = sRn + P.byte_rows;                                               // [BM] (NH = 2) a row's sum of squares over the first column pass
    const uint32_t oB = lds_off(lds_c), oA = lds_off(sA), oIds = lds_off(sIds), oRn = lds_off(sRn);
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, li = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = (wave >> 2) * WMR, wn = (wave & 3) * WNR;
    const int64_t j0 = (int64_t)blockIdx.x * BM;
    const int nrows = (int)min((int64_t)BM, P.n - j0);
    const int K = P.K, bpt = P.bpt;
    // ---- W by LDS-DMA: wave-instruction j = i * 8 + wave writes 1 KiB = stage rows 16 j .. 16 j + 15, lane -> (row, physical piece).
    // Stage row q of a wave's strip holds W row strip + (q % 32) * NT + q / 32: MFMA column li of tile b is output column
    // li * NT + b, so that a lane ends up with NT CONSECUTIVE outputs of a row (packed stores in the epilogue).
    uint32_t goff[kDma];   // byte offset into W of this lane's piece of step 0, per DMA instruction
#pragma unroll
    for (int i = 0; i < kDma; ++i) {
        const int q = (i * 8 + wave) * 16 + (lane >> 2), strip = q / WNR, within = q - strip * WNR;
        const int nrow = strip * WNR + (within & 31) * NT + (within >> 5);
        goff[i] = (uint32_t)(nrow * K + 8 * (((lane & 3) ^ (q >> 2)) & 3)) * 2u;
    }
    C16_STAMP(0);
    const int nsteps = K / 32;
    const char *Wb = (const char *)P.W;   // the W rows of the current column pass
    auto b_request = [&](int s) {   // (a step past the end re-reads the last one into a stage nobody reads: the loop stays branch-free)
        char *sB = lds_c + (s % NS) * kStageB;
        const uint32_t ko = 64u * (uint32_t)min(s, nsteps - 1);
#pragma unroll
        for (int i = 0; i < kDma; ++i) {
            const char *g = Wb + (goff[i] + ko);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                             (__attribute__((address_space(3))) void *)(sB + (i * 8 + wave) * 1024), 16, 0, 0);
        }
    };
    b_request(0);
    if (PD == 2) b_request(1);
    // ---- the tile's own inputs.  Everything that does not depend on another load is requested first (the token id, the byte ids,
    // the byte rows' rms factors), so that the prologue costs two memory round trips -- ids, then the token rows for their norm --
    // instead of one per item.
    const bool a_thread = tid < BM * 4;   // (whole waves: BM * 4 is a multiple of 64)
    const int arow = tid >> 2, apiece = tid & 3;
    int tok = a_thread ? P.tokens[j0 + min(arow, nrows - 1)] : 0;
    const int n_ids = nrows * bpt;        // (rows past the batch repeat the last valid token: computed, never stored)
    if (P.ids16) {   // compact ids from the wave-local index pass: 8 bytes per thread and trip
        for (int i0 = tid * 4; i0 < BM * bpt; i0 += 4 * kC16Threads) {
            uint16_t v[4];
            if (i0 + 3 < n_ids && (bpt & 3) == 0) {
                const uint2 w = *(const uint2 *)(P.ids16 + j0 * bpt + i0);
                v[0] = (uint16_t)w.x; v[1] = (uint16_t)(w.x >> 16); v[2] = (uint16_t)w.y; v[3] = (uint16_t)(w.y >> 16);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u, r = min(i / bpt, nrows - 1);
                    v[u] = P.ids16[(j0 + r) * bpt + i % bpt];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u < BM * bpt) sIds[i0 + u] = v[u];
        }
    } else {
        for (int i0 = tid; i0 < BM * bpt; i0 += 4 * kC16Threads) {   // four loads in flight per thread
            int64_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = min(i0 + u * kC16Threads, BM * bpt - 1);
                v[u] = P.ids[(j0 + min(i / bpt, nrows - 1)) * bpt + i % bpt];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * kC16Threads;
                if ((uint64_t)v[u] >= (uint64_t)P.byte_rows) { if (P.status) atomicOr(P.status, kStatusByteOor); v[u] = 0; }
                if (i < BM * bpt) sIds[i] = (uint16_t)v[u];
            }
        }
    }
    // rms factors of the byte rows: from the caller's table, or (small tables: norm_byte_here) computed here, a thread per row --
    // the table is L2-resident and a separate launch for 458 rows costs more than the 29 KB every workgroup re-reads
    for (int i = tid; i < (int)P.byte_rows; i += kC16Threads) {
        float r = 1.f;
        if (P.byte_rnorm) r = P.byte_rnorm[i];
        else if (P.norm_byte_here) {
            float ss = 0.f;
            const __bf16 *brow = P.byte_table + (int64_t)i * P.Db;
            for (int p0 = 0; p0 < P.Db / 8; p0 += 4) {   // four loads in flight
                bf16x8c v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *(const bf16x8c *)(brow + 8 * min(p0 + u, P.Db / 8 - 1));
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (p0 + u < P.Db / 8) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) ss += (float)v[u][e] * (float)v[u][e];
                    }
            }
            r = rms_scale(ss, P.Db, P.eps);
        }
        sRn[i] = r;
    }
    // ---- this thread's piece of the gathered operand: row arow, logical 16-byte piece apiece of every 64-byte step row
    float rn_tok = 1.f;
    if ((uint64_t)(uint32_t)tok >= (uint64_t)P.tok_rows) { if (P.status) atomicOr(P.status, kStatusTokenOor); tok = 0; }
    const __bf16 *trow = P.tok_table + (int64_t)tok * P.Dt;
    if (P.norm_tok) {   // the four threads of a row share its sum of squares (the row comes back out of L2 in the steps below)
        float ss = 0.f;
        if (a_thread)
            for (int p0 = apiece; p0 < P.Dt / 8; p0 += 32) {   // eight loads in flight
                bf16x8c v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *(const bf16x8c *)(trow + 8 * min(p0 + 4 * u, P.Dt / 8 - 1));
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (p0 + 4 * u < P.Dt / 8) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) ss += (float)v[u][e] * (float)v[u][e];
                    }
            }
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        rn_tok = rms_scale(ss, P.Dt, P.eps);
    }
    const uint32_t a_dst = oA + arow * 64 + ((apiece ^ (arow >> 2)) & 3) * 16;
    // the walk over this thread's pieces: k = 8 apiece, + 32 per step; inside the byte part (slot, within) advance with it.
    // Branch-free (and one global load per request whatever the part) so that hipcc can COUNT the loads in flight at the commit.
    int ak = 8 * apiece, slot = 0, within = 0;
    {   // the first of them inside the byte part
        const int d = P.Dt - 8 * apiece;
        const int first = P.byte_lo == 0 ? 8 * apiece : (d > 0 ? (d + 31) / 32 : 0) * 32 - d;
        slot = first / P.Db; within = first - slot * P.Db;
    }
    const int dslot = 32 / P.Db, dwithin = 32 - dslot * P.Db;
    C16_STAMP(1);
    __syncthreads();   // sIds, sRn  (hipcc drains the DMA of the first stages here: once per tile)
    C16_STAMP(2);
    auto a_request = [&](i32x4c &raw, float &scale) {
        const int kt = ak - P.tok_lo;
        const bool in_tok = (unsigned)kt < (unsigned)P.Dt;
        const int sl = min(slot, bpt - 1);   // (requests past the last step read a valid row and are never used)
        const int id = (int)lds_u16_now(oIds + (arow * bpt + sl) * 2);
        const float rb = lds_f32_now(oRn + id * 4);
        const __bf16 *src = in_tok ? trow + kt : P.byte_table + (int64_t)id * P.Db + within;
        // (asm: hipcc answers a plain load among LDS-DMA with vmcnt(0) at its use; the commit below counts instead.  The registers
        //  stay pending until that wait: nothing else may touch them -- they are outputs here and operands of the wait only)
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(raw) : "v"(src) : "memory");
        scale = in_tok ? rn_tok : rb;
        int w2 = within + dwithin, s2 = slot + dslot;
        if (w2 >= P.Db) { w2 -= P.Db; ++s2; }
        within = in_tok ? within : w2;
        slot = in_tok ? slot : s2;
        ak += 32;
    };
    // scale in fp32, round once to bf16 (the reference's norm() output), into the step's tile (the caller has waited for the piece)
    auto a_commit = [&](const i32x4c &raw_bits, float scale) {
        const bf16x8c raw = __builtin_bit_cast(bf16x8c, raw_bits);
        bf16x8c v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (__bf16)((float)raw[e] * scale);
        *(__attribute__((address_space(3))) bf16x8c *)(uintptr_t)a_dst = v;
    };
    f32x16c acc[MT][NT];
    // fragment addresses: row = (wm | wn) + 32 t + li, piece (2 kk + h) ^ (row >> 2): the tile index t only adds t * 2048, kk flips bit 5
    const uint32_t fa0 = oA + (wm + li) * 64 + ((h ^ (li >> 2)) & 3) * 16;
    const uint32_t fb0 = (wn + li) * 64 + ((h ^ (li >> 2)) & 3) * 16;
    i32x4c r0_raw = {0, 0, 0, 0}, r1_raw = {0, 0, 0, 0};
    float r0_scale = 1.f, r1_scale = 1.f;
    constexpr bool kAllGather = BM * 4 == kC16Threads;   // every thread carries a piece: no branch around the requests
    constexpr int kInflight = PD == 2 ? kDma + 1 : 0;
    const int ak_first = ak, slot_first = slot, within_first = within;
    C16_PASS_BEGIN
    if (NH > 1 && hh > 0) {   // the next column pass: its rows of W, the walk over the gathered operand from the start
        __syncthreads();      // every wave is done with the staging area of the previous pass (it lies in the stages of W)
        Wb = (const char *)P.W + (size_t)hh * BN * K * 2;
        b_request(0);
        if (PD == 2) b_request(1);
        ak = ak_first; slot = slot_first; within = within_first;
    }
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    if (kAllGather || a_thread) {
        a_request(r0_raw, r0_scale);
        if (PD == 2) a_request(r1_raw, r1_scale);
        asm volatile("s_waitcnt vmcnt(%1)" : "+v"(r0_raw) : "n"(PD - 1) : "memory");
        a_commit(r0_raw, r0_scale);
    }
    if (NH > 1 && hh > 0) {   // (pass 0: the barrier of the prologue) this wave's DMA of the first stages is older than the piece it just
        if (!(kAllGather || a_thread)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // waited for; every wave's must have landed
        c16_barrier();
    }
    // ---- the step.  One wave's share of step s is NP = 2 NT "positions" (kk, b) of MT MFMAs each; all eight waves run in lockstep
    // between the two barriers of a step, so whatever is not an MFMA has to be issued BETWEEN MFMAs or the matrix pipes idle:
    //   * the fragments of W roll through four register slots, read three positions ahead (LDS latency under the MFMAs of the
    //     positions in between), the first three of a step right behind the previous step's second barrier;
    //   * the NT DMA instructions of W step s + PD go out one per position, the gathered piece s + PD at position NP - 3 (its
    //     LDS id read drains the LDS queue: every fragment of the step is requested by then);
    //   * waits are COUNTED: lgkmcnt(n) leaves the younger fragment reads in flight, vmcnt(NT + 1) the requests of this step.
    // Order: [barrier 1: the gathered tile s is committed] fragments of the gathered tile; positions; wait for piece s + 1 and the
    // DMA of W step s + 1 (loads retire in order: one count covers both); [barrier 2: everyone has read tile s, W step s + 1 is
    // in LDS for everyone] first fragments of W step s + 1; commit piece s + 1.
    constexpr int NP = 2 * NT;
    i32x4c af[2 * MT], bq[4];
    auto frag_b = [&bq](auto idx, uint32_t fb) {   // fragment idx = (kk, b) of the stage at fb -> slot idx % 4
        constexpr int i = decltype(idx)::value;
        C16_FRAG(bq[i % 4], fb ^ ((i / NT) * 32), (i % NT) * 2048);
    };
    auto dma_piece = [&](int s, auto ic) {
        constexpr int i = decltype(ic)::value;
        char *sB = lds_c + (s % NS) * kStageB;
        const char *g = Wb + (goff[i] + 64u * (uint32_t)min(s, nsteps - 1));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                         (__attribute__((address_space(3))) void *)(sB + (i * 8 + wave) * 1024), 16, 0, 0);
    };
    auto step = [&](int s, i32x4c &ld_raw, float &ld_scale, i32x4c &cm_raw, const float &cm_scale) {
        c16_barrier();
        const uint32_t fb = oB + (s % NS) * kStageB + fb0;
        static_for<0, 2 * MT>([&af, fa0](auto jc) {
            constexpr int j = decltype(jc)::value;
            C16_FRAG(af[j], fa0 ^ ((j / MT) * 32), (j % MT) * 2048);
        });
        static_for<0, NP>([&, &af = af, &bq = bq](auto pc) {
            constexpr int p = decltype(pc)::value, kk = p / NT, b = p % NT;
            if constexpr (p == (NP >= 3 ? NP - 3 : 0))
                if (kAllGather || a_thread) a_request(ld_raw, ld_scale);
            // LDS reads behind barrier 1, in order: the 2 MT fragments of the gathered tile, then W fragments 3, 4, ... (one per position)
            constexpr int issued = 2 * MT + (p < NP - 3 ? p : NP - 3);
            constexpr int need_b = p >= 3 ? 2 * MT + p - 3 : -1;
            constexpr int need_a = p == 0 ? MT - 1 : (p == NT ? 2 * MT - 1 : -1);
            constexpr int need = need_b > need_a ? need_b : need_a;
            if constexpr (need >= 0) {
                if constexpr (MT == 2) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(bq[p % 4]), "+v"(af[kk * MT]), "+v"(af[kk * MT + 1]) : "n"(issued - need - 1));
                else asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(bq[p % 4]), "+v"(af[kk * MT]) : "n"(issued - need - 1));
            } else {
                asm volatile("" : "+v"(bq[p % 4]));
            }
#pragma unroll
            for (int a = 0; a < MT; ++a)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8c, af[kk * MT + a]), __builtin_bit_cast(bf16x8c, bq[p % 4]),
                                                                    acc[a][b], 0, 0, 0);
            if constexpr (p + 3 < NP) frag_b(std::integral_constant<int, p + 3>{}, fb);
            if constexpr (p < kDma) dma_piece(s + PD, pc);
        });
        if (kAllGather || a_thread) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(cm_raw) : "n"(kInflight) : "memory");
        else if (PD == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kDma) : "memory");   // a wave without pieces: its DMA of step s + 1
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        c16_barrier();
        const uint32_t fbn = oB + ((s + 1) % NS) * kStageB + fb0;
        static_for<0, 3>([&](auto ic) { frag_b(ic, fbn); });
        if (kAllGather || a_thread) a_commit(cm_raw, cm_scale);
    };
    static_for<0, 3>([&](auto ic) { frag_b(ic, oB + fb0); });   // (the stage landed in front of the barrier above)
    C16_STAMP(3);
    if (PD == 2) {
        for (int s = 0; s < nsteps; s += 2) {
            step(s, r0_raw, r0_scale, r1_raw, r1_scale);
            if (s + 1 < nsteps) step(s + 1, r1_raw, r1_scale, r0_raw, r0_scale);
        }
    } else {
        for (int s = 0; s < nsteps; ++s) step(s, r0_raw, r0_scale, r0_raw, r0_scale);
    }
    // What was requested past the last step is still on its way INTO registers the compiler considers free from here on: the
    // fragment reads behind the last barrier, the gathered pieces.  Hold the registers until everything has landed.
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(r0_raw), "+v"(r1_raw), "+v"(bq[0]), "+v"(bq[1]), "+v"(bq[2]), "+v"(bq[3]) : : "memory");
    C16_STAMP(4);
    // ---- epilogue.  C/D layout: MFMA column li of tile b = output column wn + li NT + b, row = wm + 32 a + (reg & 3) + 8 (reg >> 2) + 4 h.
    // y = bf16(acc + bias): F.linear on bf16 operands returns a bf16 tensor (train_gpt.py:185-186); norm() upcasts it (172-173, 443).
    // The tile leaves through LDS in halves of 32 MT rows (they fit in the stages of W): a lane packs its NT consecutive outputs of a
    // row; then 32 lanes take a row, sum its squares, scale and store whole 16-byte pieces.
    const int cb = NH > 1 ? hh * BN : 0;   // first output column of this pass
    float bv[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) bv[b] = P.bias ? (float)P.bias[cb + wn + li * NT + b] : 0.f;
    __syncthreads();   // every wave is done with the last step's tiles
    C16_STAMP(5);
    __bf16 *stage = (__bf16 *)lds_c;   // [WMR][BN]
    static_assert(WMR * BN * 2 <= NS * kStageB, "a half tile fits in the stages");
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if ((wave >> 2) == half) {
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lr = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;   // row inside the half
                    uint32_t *dst = (uint32_t *)(stage + lr * BN + wn + li * NT);
#pragma unroll
                    for (int b = 0; b < NT; b += 2) {
                        typedef __bf16 bf16x2c __attribute__((ext_vector_type(2)));
                        bf16x2c pr;
                        pr[0] = (__bf16)(acc[a][b][r] + bv[b]);
                        pr[1] = (__bf16)(acc[a][b + 1][r] + bv[b + 1]);
                        dst[b / 2] = __builtin_bit_cast(uint32_t, pr);
                    }
                }
        }
        c16_barrier();   // (LDS only: the first half's stores to HBM stay in flight under the second half's staging)
        constexpr int PP = NT / 2;   // 16-byte pieces of a row per lane: BN / 8 pieces over 32 lanes
        for (int lr = wave * 2 + h; lr < WMR; lr += 16) {
            const int row = half * WMR + lr;
            bf16x8c v[PP];
            float ss = 0.f;
            const __bf16 *res_row = nullptr;
            if constexpr (RES) {   // the row's token (rows past the batch repeat the last one: computed, never stored)
                int tk = P.tokens[j0 + min(row, nrows - 1)];
                if ((uint64_t)(uint32_t)tk >= (uint64_t)P.tok_rows) tk = 0;   // (flagged in the prologue)
                res_row = P.tok_table + (int64_t)tk * P.Dm + cb;
            }
#pragma unroll
            for (int p = 0; p < PP; ++p) {
                v[p] = *(const bf16x8c *)(stage + lr * BN + 8 * (li + 32 * p));
                if constexpr (RES) {
                    const bf16x8c t = *(const bf16x8c *)(res_row + 8 * (li + 32 * p));
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[p][e] = (__bf16)((float)v[p][e] + (float)t[e]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) ss += (float)v[p][e] * (float)v[p][e];
            }
            float rs = 1.f;
            const bool first_of_two = NH > 1 && hh + 1 < NH;   // the row's other columns are still to come: no factor yet
            if (P.norm_out) {
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) ss += __shfl_xor(ss, o, 64);
                if (first_of_two) {
                    if (li == 0) sSS[row] = ss;
                } else {
                    if (NH > 1) ss += sSS[row];
                    rs = rms_scale(ss, P.Dm, P.eps);
                    if (P.row_rnorm && li == 0 && row < nrows) P.row_rnorm[j0 + row] = rs;
#pragma unroll
                    for (int p = 0; p < PP; ++p)
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[p][e] = (__bf16)((float)v[p][e] * rs);
                }
            }
            if (row < nrows) {
                __bf16 *orow = P.out + (j0 + row) * (int64_t)P.Dm + cb;
#pragma unroll
                for (int p = 0; p < PP; ++p) {
                    if (first_of_two && P.norm_out) *(bf16x8c *)(orow + 8 * (li + 32 * p)) = v[p];   // (comes back in the last pass: keep it in L2)
                    else __builtin_nontemporal_store(v[p], (bf16x8c *)(orow + 8 * (li + 32 * p)));
                }
                if (NH > 1 && !first_of_two && P.norm_out) {
                    // the first pass's columns of this row, un-normalised so far: this lane re-reads the pieces IT stored (device-scope
                    // loads: not through this CU's L1) and rescales them
                    for (int c0 = 0; c0 < cb; c0 += BN)
#pragma unroll
                        for (int p = 0; p < PP; ++p) {
                            uint32_t *q = (uint32_t *)(orow - cb + c0 + 8 * (li + 32 * p));
                            i32x4c w;
#pragma unroll
                            for (int e = 0; e < 4; ++e) w[e] = (int)__hip_atomic_load(q + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            bf16x8c u = __builtin_bit_cast(bf16x8c, w);
#pragma unroll
                            for (int e = 0; e < 8; ++e) u[e] = (__bf16)((float)u[e] * rs);
                            __builtin_nontemporal_store(u, (bf16x8c *)q);
                        }
                }
            }
        }
        if (half == 0) c16_barrier();   // the staging area is rewritten
        C16_STAMP(6 + half);
    }
    C16_PASS_END
