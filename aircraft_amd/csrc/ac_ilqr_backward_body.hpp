// (no include guard: on purpose) The ONE body of the Riccati backward kernels, included once per kernel under two switches:
//   k_ilqr_backward<NODE, NEWTON, BOX>        (ac_ilqr.hpp)       AC_ILQR_SHOOT 0, AC_ILQR_RATE 0
//   k_ilqr_backward_shoot<NODE, NEWTON, BOX>  (ac_ilqr.hpp)       AC_ILQR_SHOOT 1: the defects of multiple shooting, `sh`
//   k_ilqr_backward_rate<NODE, NEWTON, BOX>   (ac_ilqr_rate.hpp)  AC_ILQR_RATE 1: u_{k-1} carried as seven more states (`rate_g`,
//                                                                 `rate_h`, `Kp`; the formulas head ac_ilqr_rate.hpp)
// Textual, not a function the kernels call: each kernel keeps the name AND the code it had before its switch existed (an inlined
// body changes how the compiler sees the __restrict__ kernel arguments, and with it the schedule).
    static_assert(!(AC_ILQR_SHOOT && AC_ILQR_RATE), "the rate terms over a multiple-shooting iterate are not written");
    typedef IlqrRing<NODE, NEWTON, AC_ILQR_SHOOT != 0, AC_ILQR_RATE != 0> R;
    __shared__ float smem[R::kWork + R::kDepth * R::kNodeFloats];  // ONE array: work area, then the node ring
    float* S = smem;
    float* ring = smem + R::kWork;
    const int t = threadIdx.x, rb = t >> 4, j = t & 15;
    const long b = blockIdx.x;  // grid = B
    float* sV = S;            // [13][13]
    float* sVA = S + 169;     // [13][13]
    float* sVB = S + 338;     // [13][7]
    float* sQux = S + 429;    // [7][13]
    float* sQuu = S + 520;    // [7][7]
    float* sK = S + 569;      // [7][13]
    float* svx = S + 660;     // [13]
    float* sqx = S + 673;     // [13]
    float* squ = S + 686;     // [7]
#if AC_ILQR_SHOOT
    float* svd = S + 693;     // [13]: v = V_x + V_xx d_k
#endif
#if AC_ILQR_RATE
    float* sVxp = S + 736;    // [13][7]
    float* sVpp = S + 827;    // [7][7]
    float* sKp = S + 876;     // [7][7]
    float* svp = S + 925;     // [7]
#endif

    // gather node k into ring slot `slot` (wave-uniform); element e of an array lives B floats after element e-1
    auto issue = [&](long k, int slot) {
        float* dst = ring + slot * R::kNodeFloats;
        const float* a = A + (k * 169) * B + b;
        ilqr_glds(a + (long)t * B, dst);
        ilqr_glds(a + (long)(t + 64) * B, dst + 64);
        if (t < 169 - 128) ilqr_glds(a + (long)(t + 128) * B, dst + 128);
        const float* bm = Bm + (k * 91) * B + b;
        ilqr_glds(bm + (long)t * B, dst + 169);
        if (t < 91 - 64) ilqr_glds(bm + (long)(t + 64) * B, dst + 169 + 64);
        {   // lanes 0-12 x_k, 13-19 u_k, 20-32 q_k, 33-45 xref_k, 46-58 glin_k
            const float* src = X + (k * 13 + t) * B + b;
            if (t >= 13) src = U + (k * 7 + (t - 13)) * B + b;
            if constexpr (NODE) {
                if (t >= 20) src = N.q + (k * 13 + (t - 20)) * B + b;
                if (t >= 33) src = N.xref + (k * 13 + (t - 33)) * B + b;
                if (t >= 46) src = N.glin + (k * 13 + (t - 46)) * B + b;
            }
            if (t < (NODE ? 59 : 20)) ilqr_glds(src, dst + 260);
        }
        if constexpr (NEWTON) {
            const float* hz = Hz + (k * 441) * B + b;
#pragma unroll
            for (int c = 0; c < 7; ++c)
                if (c * 64 + t < 441) ilqr_glds(hz + (long)(c * 64 + t) * B, dst + 320 + c * 64);
        }
        if constexpr (R::kUglin) {  // (always issued, so that the vmcnt bookkeeping is static; without the array: u_k again, unused)
            const float* ug = N.uglin ? N.uglin + (k * 7) * B + b : U + (k * 7) * B + b;
            if (t < 7) ilqr_glds(ug + (long)t * B, dst + 761);
        }
#if AC_ILQR_SHOOT
        {  // lanes 0-12 F_k, 13-25 x_{k+1}
            const float* src = sh.F + (k * 13 + t) * B + b;
            if (t >= 13) src = X + ((k + 1) * 13 + (t - 13)) * B + b;
            if (t < 26) ilqr_glds(src, dst + R::kShoot);
        }
#endif
#if AC_ILQR_RATE
        {  // lanes 0-6 g_k, 7-13 h_k
            const float* src = (t < 7 ? rate_g + (k * 7 + t) * B : rate_h + (k * 7 + (t - 7)) * B) + b;
            if (t < 14) ilqr_glds(src, dst + R::kRate);
        }
#endif
    };
    const float ug_on = (R::kUglin && N.uglin) ? 1.f : 0.f;

    // terminal condition (ordinary loads, before any LDS-DMA is in flight)
    float qterm = 0.f;
    if (j < 13) {
        const float xn = X[(H * 13 + j) * B + b];
        float xr, gl;
        N.template row<NODE>(C, H, true, j, b, qterm, xr, gl);
        if (rb == 0) svx[j] = fmaf(qterm, xn - xr, gl);
        for (int i = rb; i < 13; i += 4) sV[i * 13 + j] = (i == j) ? qterm : 0.f;
    }
#if AC_ILQR_RATE
    if (j < 7) {  // terminal: V_p = 0, V_xp = 0, V_pp = 0
        if (rb == 0) svp[j] = 0.f;
        for (int i = rb; i < 13; i += 4) sVxp[i * 7 + j] = 0.f;
        for (int i = rb; i < 7; i += 4) sVpp[i * 7 + j] = 0.f;
    }
#endif
    float dv1 = 0.f, dv2 = 0.f;
    IlqrBoxNode bx;  // (BOX only)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int d = 0; d < R::kDepth; ++d)
        if (H - 1 - d >= 0) issue(H - 1 - d, d);
    ilqr_sync();

    for (long it = 0; it < H; ++it) {
        const long k = H - 1 - it;
        const int slot = (int)(it % R::kDepth);
        // node k's gather has landed once at most (kDepth - 1) younger ones are outstanding; in the tail fewer were issued
        if (it + R::kDepth - 1 < H) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(R::kInstr * (R::kDepth - 1)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const float* nd = ring + slot * R::kNodeFloats;
        const float* sA = nd;         // [13][13]
        const float* sB = nd + 169;   // [13][7]
        // stage gradients
        float qjj = 0.f;  // diagonal entry j of the stage Hessian
        if (j < 13) {
            float xr = C.x_ref[j], gl = 0.f;
            qjj = C.q[j];
            if constexpr (NODE) { qjj = nd[280 + j]; xr = nd[293 + j]; gl = nd[306 + j]; }
            if (rb == 0) sqx[j] = fmaf(qjj, nd[260 + j] - xr, gl);
        }
#if AC_ILQR_SHOOT
        {
            // sV / svx still hold the expansion of node k + 1: hand it out, and fold the gap into the gradient this node reads
            if (sh.Vx != nullptr && j < 13) {
                if (rb == 0) sh.Vx[(k * 13 + j) * B + b] = svx[j];
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    if (rb + 4 * n < 13) sh.Vxx[((k * 13 + rb + 4 * n) * 13 + j) * B + b] = sV[(rb + 4 * n) * 13 + j];
            }
            if (j < 13 && rb == 1) {
                float s = svx[j];
#pragma unroll
                for (int m = 0; m < 13; ++m) s = fmaf(sV[j * 13 + m], nd[R::kShoot + m] - nd[R::kShoot + 13 + m], s);
                svd[j] = s;
            }
        }
#endif
#if AC_ILQR_RATE
        const float* srg = nd + R::kRate;      // [7] rate gradient
        const float* srh = nd + R::kRate + 7;  // [7] rate curvature
        const float gj = (j < 7) ? srg[j] : 0.f, hj = (j < 7) ? srh[j] : 0.f;
        if (j < 7 && rb == 0) squ[j] = fmaf(C.r[j], nd[273 + j], C.u_lin[j]) + gj + svp[j];  // l_u + g + V'p
#else
        if (j < 7 && rb == 0) {
            float g = fmaf(C.r[j], nd[273 + j], C.u_lin[j]);
            if constexpr (R::kUglin) g = fmaf(ug_on, nd[761 + j], g);
            squ[j] = g;
        }
#endif
        ilqr_sync();
        // This lane's columns of A_k and B_k stay in registers for the node (read once from the ring slot).
        float acol[13], bcol[13];
#pragma unroll
        for (int m = 0; m < 13; ++m) {
            acol[m] = (j < 13) ? sA[m * 13 + j] : 0.f;
            bcol[m] = (j < 7) ? sB[m * 7 + j] : 0.f;
        }
        // VA = V A, VB = V B: one read of row i of V serves both products
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int i = rb + 4 * n;
            if (i < 13) {
                float sa = 0.f, sb = 0.f;
#pragma unroll
                for (int m = 0; m < 13; ++m) {
                    const float v = sV[i * 13 + m];
                    sa = fmaf(v, acol[m], sa);
                    sb = fmaf(v, bcol[m], sb);
                }
                if (j < 13) sVA[i * 13 + j] = sa;
                if (j < 7) sVB[i * 7 + j] = sb;
            }
        }
        ilqr_sync();
        // Qx, Qu (per column, every row group), Qxx rows of column j (registers), Qux, Quu
        float qxx[4] = {0.f, 0.f, 0.f, 0.f};
        float qx = 0.f, qu = 0.f;
        const float* hz = nd + 320;  // [21][21] (NEWTON only)
        {
            float vacol[13], vbcol[13], vxs[13];  // column j of VA / VB, and V_x
#if AC_ILQR_RATE
            float vxpcol[13];  // column j of V'xp (read in the loop below: a loop of its own gives the rate kernels another schedule)
#endif
#pragma unroll
            for (int m = 0; m < 13; ++m) {
                vacol[m] = (j < 13) ? sVA[m * 13 + j] : 0.f;
                vbcol[m] = (j < 7) ? sVB[m * 7 + j] : 0.f;
#if AC_ILQR_RATE
                vxpcol[m] = (j < 7) ? sVxp[m * 7 + j] : 0.f;
#endif
#if AC_ILQR_SHOOT
                vxs[m] = svd[m];
#else
                vxs[m] = svx[m];
#endif
            }
            qx = (j < 13) ? sqx[j] : 0.f;
            qu = (j < 7) ? squ[j] : 0.f;
#pragma unroll
            for (int m = 0; m < 13; ++m) { qx = fmaf(acol[m], vxs[m], qx); qu = fmaf(bcol[m], vxs[m], qu); }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int i = rb + 4 * n;
                if (i < 13 && j < 13) {
                    float s = (i == j) ? qjj : 0.f;
                    if constexpr (NEWTON) s += hz[i * 21 + j];
#pragma unroll
                    for (int m = 0; m < 13; ++m) s = fmaf(sA[m * 13 + i], vacol[m], s);
                    qxx[n] = s;
                }
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int i = rb + 4 * n;
                if (i < 7) {  // column i of B_k (RATE: and of V'xp) serves row i of Qux and of Quu
                    float sx = NEWTON ? ((j < 13) ? hz[(13 + i) * 21 + j] : 0.f) : 0.f;
#if AC_ILQR_RATE
                    float su = (i == j) ? C.r[j < 7 ? j : 0] + C.reg + hj : 0.f;
#else
                    float su = (i == j) ? C.r[j < 7 ? j : 0] + C.reg : 0.f;
#endif
                    if constexpr (NEWTON) su += (j < 7) ? hz[(13 + i) * 21 + 13 + j] : 0.f;
#if AC_ILQR_RATE
                    su += (j < 7) ? sVpp[i * 7 + j] : 0.f;
#endif
#pragma unroll
                    for (int m = 0; m < 13; ++m) {
                        const float bi = sB[m * 7 + i];
                        sx = fmaf(bi, vacol[m], sx);
                        su = fmaf(bi, vbcol[m], su);
#if AC_ILQR_RATE
                        const float pi = sVxp[m * 7 + i];
                        sx = fmaf(pi, acol[m], sx);     // V'px A
                        su = fmaf(bi, vxpcol[m], su);   // B'V'xp
                        su = fmaf(pi, bcol[m], su);     // V'px B
#endif
                    }
                    if (j < 13) sQux[i * 13 + j] = sx;
                    if (j < 7) sQuu[i * 7 + j] = su;
                }
            }
        }
        ilqr_sync();  // Qux, Quu complete; sqx / squ / svx (/ svp) fully read
        if (j < 7 && rb == 0) squ[j] = qu;  // now holds Qu
        ilqr_sync();
        // Cholesky Quu = L L' once (every lane, in registers; reciprocal diagonal via rsq, no divisions), then
        // K(:, j) = -Quu^-1 Qux(:, j), kff = -Quu^-1 Qu (RATE: and Kp(:, j), 13 + 7 + 1 right-hand sides)
        float Qs[7][7];  // symmetrised Quu
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int m = 0; m <= i; ++m) { Qs[i][m] = 0.5f * (sQuu[i * 7 + m] + sQuu[m * 7 + i]); Qs[m][i] = Qs[i][m]; }
        float Qf[7][7], kfb[7];  // BOX: the free block of Quu (unit rows / columns at the clamped controls) and delta*
        if constexpr (BOX) {
            float qub[7], uk[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) { qub[i] = squ[i]; uk[i] = nd[273 + i]; }
            bx.solve(C, uk, Qs, qub, Qf, kfb, (threadIdx.x == 0 && box.act != nullptr) ? box.act + (k * 7) * B + b : nullptr, B);
        }
        const float (&Qc)[7][7] = BOX ? Qf : Qs;  // what is factorised
        float L[7][7], rinv[7];
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            float d = Qc[m][m];
#pragma unroll
            for (int p = 0; p < m; ++p) d = fmaf(-L[m][p], L[m][p], d);
            d = fmaxf(d, 1e-12f);
            rinv[m] = __builtin_amdgcn_rsqf(d);
            rinv[m] = rinv[m] * fmaf(-0.5f * d * rinv[m], rinv[m], 1.5f);  // one Newton step: full fp32 accuracy
            L[m][m] = d * rinv[m];
#pragma unroll
            for (int i = m + 1; i < 7; ++i) {
                float s = Qc[i][m];
#pragma unroll
                for (int p = 0; p < m; ++p) s = fmaf(-L[i][p], L[m][p], s);
                L[i][m] = s * rinv[m];
            }
        }
        auto solve = [&](float rhs[7]) {  // in place: rhs <- Quu^-1 rhs
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                float s = rhs[i];
#pragma unroll
                for (int p = 0; p < i; ++p) s = fmaf(-L[i][p], rhs[p], s);
                rhs[i] = s * rinv[i];
            }
#pragma unroll
            for (int i = 6; i >= 0; --i) {
                float s = rhs[i];
#pragma unroll
                for (int p = i + 1; p < 7; ++p) s = fmaf(-L[p][i], rhs[p], s);
                rhs[i] = s * rinv[i];
            }
        };
        float kf[7], quv[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) { quv[i] = squ[i]; kf[i] = quv[i]; }
        if constexpr (BOX) {  // kff = delta*: exactly the bound minus U_k on a clamped row
#pragma unroll
            for (int i = 0; i < 7; ++i) kf[i] = kfb[i];
        } else {
            solve(kf);
#pragma unroll
            for (int i = 0; i < 7; ++i) kf[i] = -kf[i];
        }
        float kcol[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (j < 13) {
#pragma unroll
            for (int i = 0; i < 7; ++i) kcol[i] = sQux[i * 13 + j];
            if constexpr (BOX) {
#pragma unroll
                for (int i = 0; i < 7; ++i) kcol[i] = bx.on(i) ? 0.f : kcol[i];
            }
            solve(kcol);
#pragma unroll
            for (int i = 0; i < 7; ++i) kcol[i] = -kcol[i];
            if constexpr (BOX) {  // rows of K at clamped controls: +0.0f, not the -0.0f of the line above
#pragma unroll
                for (int i = 0; i < 7; ++i) kcol[i] = bx.on(i) ? 0.f : kcol[i];
            }
            if (rb == 0) {
#pragma unroll
                for (int i = 0; i < 7; ++i) { sK[i * 13 + j] = kcol[i]; K[((k * 7 + i) * 13 + j) * B + b] = kcol[i]; }
            }
        }
#if AC_ILQR_RATE
        float kpcol[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // Kp(:, j) = -Quu^-1 Qup(:, j),  Qup(:, j) = -h_j e_j
        if (j < 7) {
#pragma unroll
            for (int i = 0; i < 7; ++i) kpcol[i] = (i == j) ? -hj : 0.f;
            if constexpr (BOX) {
#pragma unroll
                for (int i = 0; i < 7; ++i) kpcol[i] = bx.on(i) ? 0.f : kpcol[i];
            }
            solve(kpcol);
#pragma unroll
            for (int i = 0; i < 7; ++i) kpcol[i] = -kpcol[i];
            if constexpr (BOX) {  // the same rows of Kp
#pragma unroll
                for (int i = 0; i < 7; ++i) kpcol[i] = bx.on(i) ? 0.f : kpcol[i];
            }
            if (rb == 0) {
#pragma unroll
                for (int i = 0; i < 7; ++i) { sKp[i * 7 + j] = kpcol[i]; Kp[((k * 7 + i) * 7 + j) * B + b] = kpcol[i]; }
            }
        }
#endif
        float quukf[7];  // Quu kff (every lane)
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            float t = 0.f;
#pragma unroll
            for (int m = 0; m < 7; ++m) t = fmaf(Qs[i][m], kf[m], t);
            quukf[i] = t;
        }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                kff[(k * 7 + i) * B + b] = kf[i];
                dv1 += kf[i] * quv[i];
                dv2 += 0.5f * kf[i] * quukf[i];
            }
        }
        ilqr_sync();  // sK (and sKp) visible
        // V_x(j) = Qx + K' Quu kff + K' Qu + Qux' kff ;  V_xx(i, j) = Qxx + K' Quu K + K' Qux + Qux' K
        float vx = 0.f, vrow[4] = {0.f, 0.f, 0.f, 0.f};
        if (j < 13) {
            float w[7], quxj[7];  // w = Quu K(:, j) + Qux(:, j)
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                float sq = 0.f;
#pragma unroll
                for (int m = 0; m < 7; ++m) sq = fmaf(Qs[i][m], kcol[m], sq);
                quxj[i] = sQux[i * 13 + j];
                w[i] = sq + quxj[i];
            }
            vx = qx;
#pragma unroll
            for (int i = 0; i < 7; ++i) vx += kcol[i] * (quukf[i] + quv[i]) + quxj[i] * kf[i];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int i = rb + 4 * n;
                if (i < 13) {
                    float sv = qxx[n];
#pragma unroll
                    for (int m = 0; m < 7; ++m) sv += sK[m * 13 + i] * w[m] + sQux[m * 13 + i] * kcol[m];
                    vrow[n] = sv;
                }
            }
        }
#if AC_ILQR_RATE
        // V_p(j), V_xp(:, j), V_pp(:, j) from Kp(:, j) the same way
        float vp = 0.f, vxprow[4] = {0.f, 0.f, 0.f, 0.f}, vpprow[2] = {0.f, 0.f};
        if (j < 7) {
            float wp[7];  // wp = Quu Kp(:, j) + Qup(:, j)
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                float sq = 0.f;
#pragma unroll
                for (int m = 0; m < 7; ++m) sq = fmaf(Qs[i][m], kpcol[m], sq);
                wp[i] = sq + ((i == j) ? -hj : 0.f);
            }
            vp = -gj;
#pragma unroll
            for (int i = 0; i < 7; ++i) vp += kpcol[i] * (quukf[i] + quv[i]) + ((i == j) ? -hj * kf[i] : 0.f);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int i = rb + 4 * n;
                if (i < 13) {
                    float sv = 0.f;
#pragma unroll
                    for (int m = 0; m < 7; ++m) sv += sK[m * 13 + i] * wp[m] + sQux[m * 13 + i] * kpcol[m];
                    vxprow[n] = sv;
                }
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int i = rb + 4 * n;
                if (i < 7) {
                    float sv = (i == j) ? hj : 0.f;
#pragma unroll
                    for (int m = 0; m < 7; ++m) sv += sKp[m * 7 + i] * wp[m];
                    sv -= srh[i] * sKp[i * 7 + j];   // Qup' Kp: row i of Qup' is -h_i e_i'
                    vpprow[n] = sv;
                }
            }
        }
#endif
        ilqr_sync();  // every lane has read the old V / Qux before they are overwritten
        if (j < 13) {
            if (rb == 0) svx[j] = vx;
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (rb + 4 * n < 13) sV[(rb + 4 * n) * 13 + j] = vrow[n];
        }
#if AC_ILQR_RATE
        if (j < 7) {
            if (rb == 0) svp[j] = vp;
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (rb + 4 * n < 13) sVxp[(rb + 4 * n) * 7 + j] = vxprow[n];
#pragma unroll
            for (int n = 0; n < 2; ++n)
                if (rb + 4 * n < 7) sVpp[(rb + 4 * n) * 7 + j] = vpprow[n];
        }
#endif
        ilqr_sync();
        // symmetrise V (RATE: and V_pp): entry (i, j) <- mean with (j, i); both read before either is written
        float sym[4] = {0.f, 0.f, 0.f, 0.f};
        if (j < 13) {
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (rb + 4 * n < 13) sym[n] = 0.5f * (vrow[n] + sV[j * 13 + rb + 4 * n]);
        }
#if AC_ILQR_RATE
        float symp[2] = {0.f, 0.f};
        if (j < 7) {
#pragma unroll
            for (int n = 0; n < 2; ++n)
                if (rb + 4 * n < 7) symp[n] = 0.5f * (vpprow[n] + sVpp[j * 7 + rb + 4 * n]);
        }
#endif
        ilqr_sync();
        if (j < 13) {
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (rb + 4 * n < 13) sV[(rb + 4 * n) * 13 + j] = sym[n];
        }
#if AC_ILQR_RATE
        if (j < 7) {
#pragma unroll
            for (int n = 0; n < 2; ++n)
                if (rb + 4 * n < 7) sVpp[(rb + 4 * n) * 7 + j] = symp[n];
        }
#endif
        ilqr_sync();
        if (k - R::kDepth >= 0) issue(k - R::kDepth, slot);  // every read of this slot has retired (lgkmcnt(0) above)
    }
    if (threadIdx.x == 0) { dV[b] = dv1; dV[B + b] = dv2; }
    if constexpr (BOX) {
        if (threadIdx.x == 0 && box.stat != nullptr) { box.stat[b] = bx.iters; box.stat[B + b] = bx.capped; }
    }
